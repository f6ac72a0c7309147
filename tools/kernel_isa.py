"""One hash per kernel of csrc/*.hip over its normalised gfx950 assembly (no GPU needed): the gate of a refactor that must not change
a kernel.

  python tools/kernel_isa.py [--root CHECKOUT] [--jobs N] [OUT.txt]        (default: print to stdout)

Compiles each .hip file device-only to assembly with the flags of csrc/build.sh (into a temporary directory, the library is
untouched), cuts out every kernel -- from its label to its function-end label, the kernel-descriptor block in between included --
and normalises the text: comments and blank lines go, and the per-file function index leaves the block labels and the function-end
label, so that a kernel's text does not depend on its position in its file or on the file it is compiled in.  One line per kernel:
demangled name, SHA-256 of the normalised text, line count; sorted by name, not keyed by file.  The last line hashes the listing.
Two checkouts hold the same kernels exactly when their listings are equal (--root runs the tool of one checkout on another).
The tool hashes text; it knows nothing about what the text says.
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def demangle(names):
  for filt in ('/opt/rocm/lib/llvm/bin/llvm-cxxfilt', 'c++filt'):
    try:
      out = subprocess.run([filt], input='\n'.join(names) + '\n', capture_output=True, text=True, check=True).stdout.split('\n')
      return dict(zip(names, out))
    except Exception:
      continue
  return {n: n for n in names}


def assemble(root, path, tmp):
  csrc = os.path.dirname(path)
  out = os.path.join(tmp, os.path.basename(path) + '.s')
  cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(root, 'include'), '-I' + csrc, '-Wall',
         '-Wno-unused-function', '-Wno-pass-failed', '--cuda-device-only', '-S', path, '-o', out]
  r = subprocess.run(cmd, capture_output=True, text=True)
  if r.returncode != 0:
    raise RuntimeError('%s\n%s' % (' '.join(cmd), r.stderr))
  return open(out).read()


def normalise(lines):
  out = []
  for line in lines:
    line = line.split(';', 1)[0].rstrip()
    if not line.strip():
      continue
    line = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', line)
    line = re.sub(r'\.L([A-Za-z]+)\d+_(\d+)', r'.L\1_\2', line)       # .LBB<function>_<block>, jump tables and their like
    out.append(re.sub(r'\s+', ' ', line.strip()))
  return out


def kernels_of(text):
  """{mangled name: normalised lines} of every symbol that has a kernel descriptor."""
  lines = text.split('\n')
  names = [m.group(1) for m in (re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln) for ln in lines) if m]
  found = {}
  for name in names:
    begin = next(i for i, ln in enumerate(lines) if ln.startswith(name + ':'))
    end = next(i for i in range(begin, len(lines)) if re.match(r'\.Lfunc_end\d+:', lines[i]))
    found[name] = normalise(lines[begin:end + 1])
  return found


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument('--jobs', type=int, default=8)
  ap.add_argument('out', nargs='?')
  args = ap.parse_args()
  csrc = os.path.join(args.root, 'graph-neural-pde_amd', 'csrc')
  files = sorted(f for f in os.listdir(csrc) if f.endswith('.hip'))
  found = set()        # (mangled name, text): kernels of unnamed namespaces may share a name across files, and a header's kernel compiled
                       # in several files to one text is one kernel
  with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
    for f, text in zip(files, pool.map(lambda f: assemble(args.root, os.path.join(csrc, f), tmp), files)):
      found.update((name, tuple(body)) for name, body in kernels_of(text).items())
  pretty = demangle(sorted({n for n, _ in found}))
  rows = sorted((pretty[n], hashlib.sha256('\n'.join(body).encode()).hexdigest(), len(body)) for n, body in found)
  listing = ''.join('%s  %s  %d\n' % r for r in rows)
  listing += '# %d kernels, listing sha256 %s\n' % (len(rows), hashlib.sha256(listing.encode()).hexdigest())
  if args.out:
    open(args.out, 'w').write(listing)
    print(listing.rstrip().split('\n')[-1])
  else:
    sys.stdout.write(listing)


if __name__ == '__main__':
  main()
