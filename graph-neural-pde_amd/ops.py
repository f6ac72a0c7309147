"""Torch-facing wrappers of the C ABI (include/gnpde.h).  PyTorch is plumbing here: it owns the
device memory and the stream; every arithmetic step runs in libgnpde_hip.so."""
import ctypes
import torch

from . import _lib
from ._lib import ptr, check, require_hip, f32c, stream_of


def _scalar_dev(t, like):
  """Learnable scalars are read by the kernels from device memory."""
  t = t.detach()
  if t.device != like.device or t.dtype != torch.float32:
    t = t.to(like.device, torch.float32)
  return t.reshape(-1)


_PAD_X, _PAD_W = {}, {}


def _linear_operands(x, weight, bias, out):
  """(x, weight, b, out, n, d, m) as the projection kernels get them: validated, out allocated, and for n >= 4096 with a K the 16-byte
  loads do not cover the zero-padded copies of both operands."""
  require_hip(x, weight, bias)
  x, weight = _lib.f32rows(x, 'x'), f32c(weight, 'weight')
  n, d = x.shape
  m = weight.shape[0]
  if weight.shape[1] != d:
    raise _lib.GnpdeError('linear: weight is %s but x has %d features' % (tuple(weight.shape), d))
  if out is None:
    out = torch.empty(n, m, dtype=torch.float32, device=x.device)
  else:
    # the kernels get out's address and row stride as they are: anything they would not write as [n, m] rows is refused before a launch
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
      raise _lib.GnpdeError('linear: out must be a float32 tensor (got %s)' % (getattr(out, 'dtype', type(out).__name__),))
    if out.device != x.device:
      raise _lib.GnpdeError('linear: out is on %s but x is on %s' % (out.device, x.device))
    if tuple(out.shape) != (n, m):
      raise _lib.GnpdeError('linear: out is %s, the product is [%d, %d]' % (tuple(out.shape), n, m))
    if m > 1 and out.stride(1) != 1:
      raise _lib.GnpdeError('linear: out must have unit column stride (strides %s)' % (tuple(out.stride()),))
  b = None if bias is None else f32c(bias, 'bias')
  if n >= 4096 and (d % 16 != 0 or x.stride(0) % 4 != 0 or weight.stride(0) % 4 != 0):
    # a width the 16-byte operand loads / complete 16-wide K blocks of the MFMA kernels do not cover (BLEND: d = 162) takes their
    # guarded scalar-load variant -- 383 us against ~60 at the ogbn-arxiv shape.  Zero-padded copies of both operands (K up to the
    # next multiple of 16) add exact zeros to every dot product and put the product on the fast kernels.
    d16 = (d + 15) // 16 * 16
    # the padded operand buffers are kept (one per shape and device; the padding columns are zeroed once and never written again):
    # this sits on the training path, once per evaluation -- ~119 MB of allocation + memset per call at the ogbn-arxiv BLEND shape
    key = (n, d, d16, str(x.device))
    xp = _PAD_X.get(key)
    if xp is None:
      if len(_PAD_X) >= 4:
        _PAD_X.clear()
      xp = _PAD_X[key] = torch.zeros(n, d16, dtype=torch.float32, device=x.device)
    xp[:, :d].copy_(x)
    # the padded weight buffer is reused per shape (padding columns zeroed once); the weight itself is copied in on every call -- it is
    # m x d floats, and no identity / version key can see an in-place update made through .data (round-5 advisor item)
    wkey = (m, d, d16, str(x.device))
    wp = _PAD_W.get(wkey)
    if wp is None:
      if len(_PAD_W) >= 8:
        _PAD_W.clear()
      wp = _PAD_W[wkey] = torch.zeros(m, d16, dtype=torch.float32, device=x.device)
    wp[:, :d].copy_(weight)
    x, weight, d = xp, wp, d16
  return x, weight, b, out, n, d, m


def linear(x, weight, bias=None, out=None, relu_input=False):
  """out = x @ weight.T + bias on the fp32 matrix cores (gnpde_linear); relu_input: out = relu(x) @ weight.T + bias
  (gnpde_relu_linear, the decoder of GNN.forward).  x may have padded rows (unit column stride).  out, when given, is a float32
  [n, m] tensor on x's device with unit column stride (a column window of a wider matrix is fine); anything else raises GnpdeError
  before a launch."""
  x, weight, b, out, n, d, m = _linear_operands(x, weight, bias, out)
  fn = _lib.lib().gnpde_relu_linear if relu_input else _lib.lib().gnpde_linear
  check(fn(ptr(x), n, d, x.stride(0), ptr(weight), m, weight.stride(0), ptr(b), ptr(out), out.stride(0), stream_of(x)))
  return out


def linear_launches(x, weight, out=None):
  """The launches linear(x, weight, out=out) makes (gnpde_linear_plan), as _lib.LinearLaunchStruct records in launch order: the same
  operand preparation, zero-padded copies included, and no launch."""
  x, weight, _, out, n, d, m = _linear_operands(x, weight, None, out)
  L = _lib.lib()
  args = (x.data_ptr(), n, d, x.stride(0), weight.data_ptr(), m, weight.stride(0), out.data_ptr(), out.stride(0))
  count = L.gnpde_linear_plan(*args, None, 0)
  if count < 0:
    check(count)
  plan = (_lib.LinearLaunchStruct * max(count, 1))()
  if L.gnpde_linear_plan(*args, plan, count) != count:
    raise _lib.GnpdeError('linear_plan: the launch count changed between two calls')
  return list(plan[:count])


def linear_plan(x, weight, out=None):
  """Names of the kernel instantiations linear(x, weight, out=out) launches, in order ('small<2>', 'staged2<8>', 'lds<4,128>',
  'tile<1,1,0>', ...: the dispatch table of csrc/linear.hip).  The launch decision, for tests and A/B scripts."""
  return [l.line for l in linear_launches(x, weight, out)]


def qk_tables(x, weight, bias, att_dim, out=None):
  """(q, k, ldqk, buffer) of the q||k projection in the layout the SOLVERS use for this shape: two tables [n, A] when a key row is
  shorter than a cache line and gnpde_linear_split_supported says so, else interleaved rows [n, 2A] (measurement aids: bench.py times
  the projection and the attention on what the solver launches)."""
  require_hip(x, weight, bias)
  x, weight = _lib.f32rows(x, 'x'), f32c(weight, 'weight')
  n, d = x.shape
  m = weight.shape[0]
  L = _lib.lib()
  if out is None:
    out = torch.empty(n * m, dtype=torch.float32, device=x.device)
  flat = out.reshape(-1)
  if m == 2 * att_dim and L.gnpde_linear_split_supported(ptr(x), n, d, x.stride(0), ptr(weight), m, weight.stride(0), att_dim):
    q, k = flat[:n * att_dim].view(n, att_dim), flat[n * att_dim:].view(n, att_dim)
    check(L.gnpde_linear_split(ptr(x), n, d, x.stride(0), ptr(weight), m, weight.stride(0), ptr(None if bias is None else f32c(bias, 'bias')),
                               ptr(q), ptr(k), att_dim, stream_of(x)))
    return q, k, att_dim, out
  qk = linear(x, weight, bias, out=flat.view(n, m))
  return qk, qk[:, att_dim:], m, out


def qk_tables_plan(x, weight, att_dim, out=None):
  """Names of the launches of qk_tables(x, weight, ., att_dim, out): ['staged2<KB>+split'] where the two tables are written
  (gnpde_linear_split_plan), else linear_plan of the interleaved product."""
  require_hip(x, weight)
  x, weight = _lib.f32rows(x, 'x'), f32c(weight, 'weight')
  n, d = x.shape
  m = weight.shape[0]
  L = _lib.lib()
  if out is None:
    out = torch.empty(n * m, dtype=torch.float32, device=x.device)
  flat = out.reshape(-1)
  if m == 2 * att_dim and L.gnpde_linear_split_supported(ptr(x), n, d, x.stride(0), ptr(weight), m, weight.stride(0), att_dim):
    one = _lib.LinearLaunchStruct()
    rc = L.gnpde_linear_split_plan(x.data_ptr(), n, d, x.stride(0), weight.data_ptr(), m, weight.stride(0), flat.data_ptr(),
                                   flat[n * att_dim:].data_ptr(), att_dim, ctypes.byref(one))
    if rc != 1:
      check(rc)
    return [one.line]
  return linear_plan(x, weight, out=flat.view(n, m))


def edge_to_csr_mean(graph, src_edge, out=None):
  """w_csr[p] = mean over heads of src_edge[perm[p]]; src_edge is [E] or [E,h] in edge order."""
  require_hip(src_edge)
  src = f32c(src_edge.detach(), 'edge weights')
  h = 1 if src.dim() == 1 else src.shape[1]
  if src.shape[0] != graph.e:
    raise _lib.GnpdeError('edge weights have %d rows but the graph has %d edges' % (src.shape[0], graph.e))
  if out is None:
    out = torch.empty(max(graph.e, 1), dtype=torch.float32, device=src.device)
  if graph.e == 0:
    return out.zero_()
  check(_lib.lib().gnpde_edge_to_csr_mean(graph.ref(), ptr(src), h, ptr(out), stream_of(src)))
  return out


def make_epilogue(alpha, beta, x0, alpha_sigmoid, stage=_lib.STAGE_RHS, dt=0.0, y=None, k1=None, k2=None, k3=None,
                  out_k=None, out_y=None, prev=(), coef=()):
  e = _lib.EpilogueStruct()
  e.n_prev = len(prev)
  for j, t in enumerate(prev):
    e.prev[j] = t.data_ptr()
  for j, c in enumerate(coef):
    e.coef[j] = float(c)
  e.alpha, e.beta = alpha.data_ptr(), (beta.data_ptr() if beta is not None else None)
  e.x0 = x0.data_ptr() if x0 is not None else None
  e.alpha_sigmoid, e.stage, e.dt = int(alpha_sigmoid), int(stage), float(dt)
  for name, t in (('y', y), ('k1', k1), ('k2', k2), ('k3', k3), ('out_k', out_k), ('out_y', out_y)):
    setattr(e, name, t.data_ptr() if t is not None else None)
  return e


def linear_epilogue(z, wout_t, u, epi):
  """stage(alpha' (z Wout - u) + beta x0) in one launch (gnpde_linear_epilogue; the out-projection of the GAT function's
  mix_features form): z [n, A], wout_t [d, A] (Wout transposed), u [n, d]; epi: an EpilogueStruct (make_epilogue) whose operands
  and outputs are [n, d] with u's row stride."""
  require_hip(z, wout_t, u)
  z, wout_t, u = _lib.f32rows(z, 'z'), _lib.f32rows(wout_t, 'wout_t'), _lib.f32rows(u, 'u')
  if z.shape[0] != u.shape[0] or wout_t.shape != (u.shape[1], z.shape[1]):
    raise _lib.GnpdeError('linear_epilogue: z %s, wout_t %s and u %s do not fit' % (tuple(z.shape), tuple(wout_t.shape), tuple(u.shape)))
  check(_lib.lib().gnpde_linear_epilogue(ptr(z), z.shape[0], z.shape[1], z.stride(0), ptr(wout_t), u.shape[1], wout_t.stride(0),
                                         ptr(u), u.stride(0), ctypes.byref(epi), stream_of(u)))


def _check_shadow(t, like, name):
  """A bf16 shadow [n, d] of the fp32 state `like`: same shape, same row stride (elements), unit column stride."""
  require_hip(t)
  if t.dtype != torch.bfloat16 or t.dim() != 2 or t.shape != like.shape or t.stride(1) != 1 or t.stride(0) != like.stride(0):
    raise _lib.GnpdeError('%s must be a bfloat16 [%d, %d] matrix with row stride %d (the state\'s)'
                          % (name, like.shape[0], like.shape[1], like.stride(0)))
  return t


def to_bf16(x, out=None):
  """The bf16 shadow of a float32 state [n, d] (round to nearest even, gnpde_to_bf16): same shape and row stride as x -- a padded
  state (row stride > d) gets a padded shadow whose padding columns are left as allocated (zero)."""
  require_hip(x)
  x = _lib.f32rows(x, 'x')
  n, d = x.shape
  ld = x.stride(0)
  if out is None:
    out = torch.zeros(n, ld, dtype=torch.bfloat16, device=x.device)[:, :d]
  else:
    _check_shadow(out, x, 'out')
  check(_lib.lib().gnpde_to_bf16(ptr(x), n, d, ld, ptr(out), stream_of(x)))
  return out


def spmm_lo(graph, w_csr, u_lo, out=None):
  """Plain aggregation out = A widen(u_lo), gathered from the bf16 shadow u_lo [n, d] (gnpde_spmm_lo); fp32 accumulation and output.
  d % 4 != 0 needs a padded shadow (row stride % 4 == 0, as ops.to_bf16 of a padded state gives) and returns a padded output."""
  require_hip(u_lo, w_csr)
  if u_lo.dtype != torch.bfloat16 or u_lo.dim() != 2 or u_lo.stride(1) != 1:
    raise _lib.GnpdeError('u_lo must be a bfloat16 matrix with unit column stride')
  n, d = u_lo.shape
  ld = u_lo.stride(0)
  if out is None:
    out = torch.zeros(n, ld, dtype=torch.float32, device=u_lo.device)[:, :d]
  elif out.dtype != torch.float32 or out.shape != u_lo.shape or out.stride(1) != 1 or out.stride(0) != ld:
    raise _lib.GnpdeError('out must be float32 with the shape and row stride of u_lo')
  L = _lib.lib()
  ws = graph.workspace('spmm%d' % d, L.gnpde_spmm_workspace_bytes(graph.ref(), d))
  check(L.gnpde_spmm_lo(graph.ref(), ptr(w_csr), ptr(u_lo), d, ld, ptr(out), ptr(ws), ws.numel(), stream_of(u_lo)))
  return out


def spmm_rhs(graph, w_csr, u, alpha, beta=None, x0=None, alpha_sigmoid=True, out=None, gather_lo=None, tickets=None, **stage_kw):
  """f = alpha' (A u - u) + beta x0 with A given by (graph, w_csr); optional fused solver stage.
  tickets (optional): a zeroed device buffer of gnpde_spmm_ticket_bytes(graph) bytes; where the row-pair kernel runs, the launch then
  folds its hub rows itself instead of enqueuing the fold launch (gnpde_spmm_rhs_tickets) and leaves the buffer zero again.
  gather_lo = (u_lo, out_y_lo): the neighbour rows are gathered from the bf16 shadow u_lo of u (ops.to_bf16) instead of u, and the
  bf16 rounding of the stage's out_y is written to out_y_lo (None: not written) by the same launch (gnpde_spmm_rhs_lo)."""
  require_hip(u, w_csr, x0)
  u = _lib.f32rows(u, 'u') if gather_lo is not None else f32c(u, 'u')
  n, d = u.shape
  if n < graph.n:  # (a sharded state carries halo rows after the graph's own rows)
    raise _lib.GnpdeError('state has %d rows but the graph has %d nodes' % (n, graph.n))
  alpha_d = _scalar_dev(alpha, u)
  beta_d = _scalar_dev(beta, u) if x0 is not None else None
  x0c = f32c(x0, 'x0') if x0 is not None else None
  if x0c is not None and (x0c.shape[1] != d or x0c.shape[0] < graph.n):
    raise _lib.GnpdeError('x0 shape %s does not cover the %d x %d state' % (tuple(x0c.shape), graph.n, d))
  if 'stage' not in stage_kw:
    if out is None:
      out = torch.empty_like(u)
    stage_kw = dict(stage=_lib.STAGE_RHS, out_k=out)
  epi = make_epilogue(alpha_d, beta_d, x0c, alpha_sigmoid, **stage_kw)
  L = _lib.lib()
  ws = graph.workspace('spmm%d' % d, L.gnpde_spmm_workspace_bytes(graph.ref(), d))
  if gather_lo is not None:
    u_lo, out_y_lo = gather_lo
    _check_shadow(u_lo, u, 'gather_lo[0]')
    if out_y_lo is not None:
      _check_shadow(out_y_lo, u, 'gather_lo[1]')
    check(L.gnpde_spmm_rhs_lo(graph.ref(), ptr(w_csr), ptr(u), ptr(u_lo), d, u.stride(0), ctypes.byref(epi), ptr(out_y_lo), ptr(ws),
                              ws.numel(), stream_of(u)))
    return out
  if tickets is not None:
    require_hip(tickets)
    check(L.gnpde_spmm_rhs_tickets(graph.ref(), ptr(w_csr), ptr(u), d, u.stride(0), ctypes.byref(epi), ptr(ws), ws.numel(), ptr(tickets),
                                   tickets.numel() * tickets.element_size(), stream_of(u)))
    return out
  check(L.gnpde_spmm_rhs(graph.ref(), ptr(w_csr), ptr(u), d, u.stride(0), ctypes.byref(epi), ptr(ws), ws.numel(),
                         stream_of(u)))
  return out


def spmm_plan(graph, u_addr, d, ld, epi=None, plain_out_addr=0, ws_addr=0, padded_rows=False, lo=False, tickets=False, defer=False,
              fork=False):
  """The launch an aggregation with these operands takes (gnpde_spmm_plan -> _lib.SpmmLaunchStruct): kernel family and template line,
  lanes, grid, fork and hub-row fold.  Addresses are integers read for their alignment only; epi is an epilogue (make_epilogue) or None
  for the plain aggregation to plain_out_addr.  Nothing is launched and no device is needed; a call the launch would refuse raises."""
  plan = _lib.SpmmLaunchStruct()
  flags = (_lib.SPMM_PLAN_LO * bool(lo) | _lib.SPMM_PLAN_TICKETS * bool(tickets) | _lib.SPMM_PLAN_DEFER * bool(defer) |
           _lib.SPMM_PLAN_FORK * bool(fork))
  check(_lib.lib().gnpde_spmm_plan(graph.ref(), int(u_addr), d, ld, None if epi is None else ctypes.byref(epi), int(plain_out_addr),
                                   int(ws_addr), int(bool(padded_rows)), flags, ctypes.byref(plan)))
  return plan


def spmm(graph, w_csr, u, out=None):
  """Plain aggregation out = A u."""
  require_hip(u, w_csr)
  u = f32c(u, 'u')
  n, d = u.shape
  if out is None:
    out = torch.empty_like(u)
  L = _lib.lib()
  ws = graph.workspace('spmm%d' % d, L.gnpde_spmm_workspace_bytes(graph.ref(), d))
  check(L.gnpde_spmm(graph.ref(), ptr(w_csr), ptr(u), d, u.stride(0), ptr(out), ptr(ws), ws.numel(), stream_of(u)))
  return out


def sddmm(graph, a, b, scale=None, scale_sigmoid=False, out=None):
  """out_csr[p] = s * a[row_p] . b[col_p] over the graph's entries (CSR order)."""
  require_hip(a, b)
  a, b = f32c(a, 'a'), f32c(b, 'b')
  if out is None:
    out = torch.empty(max(graph.e, 1), dtype=torch.float32, device=a.device)
  sc = _scalar_dev(scale, a) if scale is not None else None
  check(_lib.lib().gnpde_sddmm(graph.ref(), ptr(a), a.stride(0), ptr(b), b.stride(0), a.shape[1], ptr(sc),
                               int(bool(scale_sigmoid)), ptr(out), stream_of(a)))
  return out


def softmax_rows_bwd(graph, att_edge, dw_csr, edge_w_csr=None, scale=None, scale_sigmoid=False):
  """ds [E,h] (CSR order) of the row softmax + head mean, see gnpde_softmax_rows_bwd."""
  require_hip(att_edge, dw_csr)
  att_edge = f32c(att_edge, 'attention')
  h = att_edge.shape[1]
  ds = torch.empty(max(graph.e, 1), h, dtype=torch.float32, device=att_edge.device)
  sc = _scalar_dev(scale, att_edge) if scale is not None else None
  check(_lib.lib().gnpde_softmax_rows_bwd(graph.ref(), ptr(att_edge), h, ptr(dw_csr), ptr(edge_w_csr), ptr(sc),
                                          int(bool(scale_sigmoid)), ptr(ds), stream_of(att_edge)))
  return ds


def attention_rows_bwd(graph, att, r_csr, heads, scale=None, scale_sigmoid=False):
  """ds [E,h] (CSR order) from q, k in one pass (gnpde_attention_rows_bwd); None when the shape has no kernel."""
  require_hip(r_csr)
  dk = att.att_dim // att.heads
  if att.heads not in (1, 2, 4, 8) or dk not in (4, 8, 16):
    return None
  ds = torch.empty(max(graph.e, 1), heads, dtype=torch.float32, device=r_csr.device)
  sc = _scalar_dev(scale, r_csr) if scale is not None else None
  check(_lib.lib().gnpde_attention_rows_bwd(graph.ref(), ctypes.byref(att), ptr(r_csr), ptr(sc), int(bool(scale_sigmoid)),
                                            ptr(ds), stream_of(r_csr)))
  return ds


def hub_bwd_workspace(graph, heads, att_dim, like):
  """Scratch for the chunked hub rows of attention_rows_bwd_dq / head_rowsum (gnpde_hub_bwd_workspace_floats), or None for a graph
  without hub rows."""
  floats = _lib.lib().gnpde_hub_bwd_workspace_floats(graph.ref(), int(heads), int(att_dim))
  return torch.empty(floats, dtype=torch.float32, device=like.device) if floats else None


def attention_rows_bwd_dq(graph, att, r, rpos=None, scale=None, scale_sigmoid=False, dq=None, hub_ws=None):
  """ds [E,h] (CSR order) of gnpde_attention_rows_bwd_dq.  r [E]: in CSR order, or in the order rpos (int32 [E]) maps CSR positions
  into.  dq: None, or a [n, heads*d_k] view with unit column stride that receives d q (rows without entries are left alone).
  hub_ws: None (a block per hub row) or hub_bwd_workspace (chunked hub rows).  A shape without a kernel raises."""
  require_hip(r)
  ds = torch.empty(max(graph.e, 1), att.heads, dtype=torch.float32, device=r.device)
  sc = _scalar_dev(scale, r) if scale is not None else None
  if dq is not None and (dq.stride(1) != 1 or dq.shape != (graph.n, att.att_dim) or dq.dtype != torch.float32):
    raise _lib.GnpdeError('attention_rows_bwd_dq: dq must be fp32 [n, heads*d_k] with unit column stride')
  if rpos is not None and (rpos.dtype != torch.int32 or rpos.numel() < graph.e):
    raise _lib.GnpdeError('attention_rows_bwd_dq: rpos must be int32 [E]')
  if hub_ws is not None and hub_ws.numel() < _lib.lib().gnpde_hub_bwd_workspace_floats(graph.ref(), att.heads, att.att_dim):
    raise _lib.GnpdeError('attention_rows_bwd_dq: hub_ws is too small')
  check(_lib.lib().gnpde_attention_rows_bwd_dq(graph.ref(), ctypes.byref(att), ptr(r), ptr(rpos), ptr(sc), int(bool(scale_sigmoid)), ptr(ds),
                                               ptr(dq), dq.stride(0) if dq is not None else 0, ptr(hub_ws), stream_of(r)))
  return ds


def head_rowsum(graph, ds, feat, heads, dk, scale, out, pos=None, hub_ws=None):
  """out[seg, :] = scale * sum over the rows of `graph` of ds[pos[t] or t, head] * feat[colidx[t], :] (gnpde_head_rowsum) into the
  [n, heads*dk] view `out`; rows without entries are left alone.  A shape without a kernel raises."""
  require_hip(ds, feat)
  if feat.stride(1) != 1 or out.stride(1) != 1 or out.shape != (graph.n, heads * dk) or ds.shape[1] != heads or not ds.is_contiguous():
    raise _lib.GnpdeError('head_rowsum: feat / out need unit column stride, out [n, heads*dk], ds contiguous [E, heads]')
  if pos is not None and (pos.dtype != torch.int32 or pos.numel() < graph.e):
    raise _lib.GnpdeError('head_rowsum: pos must be int32 [E]')
  if hub_ws is not None and hub_ws.numel() < graph.n_long_chunks * heads * dk:
    raise _lib.GnpdeError('head_rowsum: hub_ws is too small')
  check(_lib.lib().gnpde_head_rowsum(graph.ref(), ptr(pos), ptr(ds), int(heads), int(dk), ptr(feat), feat.stride(0), float(scale), ptr(out),
                                     out.stride(0), ptr(hub_ws), stream_of(feat)))
  return out


def edge_attention_bwd(graph, att, r_csr, scale=None, scale_sigmoid=False):
  """ds [E,h] (CSR order) for any normaliser (softmax / squareplus over rows / columns), see gnpde_edge_attention_bwd."""
  require_hip(r_csr)
  L = _lib.lib()
  ds = torch.empty(max(graph.e, 1), att.heads, dtype=torch.float32, device=r_csr.device)
  ws = graph.workspace('att_bwd', L.gnpde_attention_bwd_workspace_bytes(graph.ref(), ctypes.byref(att)))
  sc = _scalar_dev(scale, r_csr) if scale is not None else None
  check(L.gnpde_edge_attention_bwd(graph.ref(), ctypes.byref(att), ptr(r_csr), ptr(sc), int(bool(scale_sigmoid)), ptr(ds),
                                   ptr(ws), ws.numel(), stream_of(r_csr)))
  return ds


def quantile(v, q):
  """torch.quantile(v, q) (default linear interpolation) of a float32 device vector as a 0-d device tensor, by radix select
  (gnpde_quantile): no sort, same float32 rank arithmetic as torch, no 16 M element limit."""
  require_hip(v)
  v = f32c(v.detach().reshape(-1), 'quantile input')
  L = _lib.lib()
  out = torch.empty(1, dtype=torch.float32, device=v.device)
  ws = torch.empty(int(L.gnpde_quantile_workspace_bytes()), dtype=torch.uint8, device=v.device)
  check(L.gnpde_quantile(ptr(v), v.numel(), float(q), ptr(out), ptr(ws), ws.numel(), stream_of(v)))
  return out.reshape(())


def threshold_edges(edge_index, score, threshold, norm_idx, n_nodes):
  """(edge_index[:, score > threshold], renormalised kept scores): stable compaction + per-endpoint renormalisation in one
  native sequence (gnpde_threshold_edges); one host read for the kept count."""
  require_hip(edge_index, score, threshold)
  ei = edge_index.detach()
  if ei.dtype != torch.int64 or not ei.is_contiguous():
    ei = ei.to(torch.int64).contiguous()
  sc = f32c(score.detach().reshape(-1), 'score')
  thr = threshold.detach().to(torch.float32).reshape(1)
  E = ei.shape[1]
  if E == 0:
    return ei.clone(), sc.clone()
  L = _lib.lib()
  out_ei = torch.empty_like(ei)
  out_w = torch.empty(max(E, 1), dtype=torch.float32, device=ei.device)
  cnt = torch.zeros(1, dtype=torch.int64, device=ei.device)
  ws = torch.empty(int(L.gnpde_threshold_edges_workspace_bytes(E, int(n_nodes))), dtype=torch.uint8, device=ei.device)
  check(L.gnpde_threshold_edges(ptr(ei), ptr(sc), E, ptr(thr), int(norm_idx), int(n_nodes), ptr(out_ei), ptr(out_w), ptr(cnt),
                                ptr(ws), ws.numel(), stream_of(sc)))
  k = int(cnt.item())
  return out_ei[:, :k].contiguous(), out_w[:k].clone()


# ---- edge-sampling rewiring of the fully-adjacent layer (csrc/edge_sampling.hip; definitions in include/gnpde.h) ----------------
SAMPLING_FLAGS = ((_lib.SAMPLING_EMPTY_COLUMN, 'a node has no incoming edge (its importance is 0 / 0)'),
                  (_lib.SAMPLING_NONFINITE, 'a logit is not finite'),
                  (_lib.SAMPLING_ZERO_MASS, 'the weights sum to zero'),
                  (_lib.SAMPLING_INDEX_RANGE, 'an edge index lies outside [0, n)'))
INT32_MAX = 2 ** 31 - 1


def _sampling_device(device, who):
  device = torch.device('cuda' if device is None else device)
  if device.type != 'cuda':
    raise _lib.GnpdeError('%s runs only on a HIP device (got %s); there is no CPU fallback' % (who, device.type))
  if not torch.cuda.is_available():
    raise _lib.GnpdeError('%s runs only on a HIP device and none is available; there is no CPU fallback' % who)
  if device.index is None:
    device = torch.device('cuda', torch.cuda.current_device())
  return device


def _stream_on(device):
  return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _draw_args(count, seed, stream, call, who):
  count, seed, stream, call = int(count), int(seed), int(stream), int(call)
  if count < 0:
    raise _lib.GnpdeError('%s: count = %d is negative' % (who, count))
  if not (0 <= stream < 2 ** 32 and 0 <= call < 2 ** 32):
    raise _lib.GnpdeError('%s: stream = %d / call = %d outside [0, 2^32)' % (who, stream, call))
  return count, seed & (2 ** 64 - 1), stream, call


def _node_count(n, who):
  n = int(n)
  if not 1 <= n <= INT32_MAX:
    raise _lib.GnpdeError('%s: n = %d outside 1 .. INT32_MAX' % (who, n))
  return n


def _raise_flags(flag, who, table=SAMPLING_FLAGS):
  """Raise with the texts of the bits set in a kernel's device flag word (table: SAMPLING_FLAGS or DEEPWALK_FLAGS)."""
  bits = int(flag.item())
  if bits:
    raise _lib.GnpdeError('%s: %s' % (who, '; '.join(text for bit, text in table if bits & bit)))


def _edge_list(edge_index, name):
  if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
    raise _lib.GnpdeError('%s must be a [2, E] tensor' % name)
  require_hip(edge_index)
  if edge_index.dtype != torch.int64:
    raise _lib.GnpdeError('%s must be int64 (got %s)' % (name, edge_index.dtype))
  ei = edge_index.detach()
  return ei if ei.is_contiguous() else ei.contiguous()


def philox_words(seed, stream, call, first_block, n_words, device=None):
  """n_words 32-bit words of the Philox4x32-10 stream (seed, stream, call), starting at counter block first_block, as an int64
  device vector (values in [0, 2^32)): word w is word (w & 3) of block first_block + (w >> 2) (gnpde_philox_words)."""
  n_words, seed, stream, call = _draw_args(n_words, seed, stream, call, 'philox_words')
  first_block = int(first_block)
  if not 0 <= first_block < 2 ** 64:
    raise _lib.GnpdeError('philox_words: first_block = %d outside [0, 2^64)' % first_block)
  device = _sampling_device(device, 'philox_words')
  out = torch.empty(n_words, dtype=torch.int32, device=device)
  if n_words:
    check(_lib.lib().gnpde_philox_words(seed, stream, call, first_block, n_words, ptr(out), _stream_on(device)))
  return out.to(torch.int64) & 0xffffffff


def random_nodes(n, count, seed, stream, call, device=None):
  """count node indices uniform over [0, n) as an int64 device vector: draw i = (word i of the stream * n) >> 32
  (gnpde_random_nodes).  1 <= n <= INT32_MAX."""
  count, seed, stream, call = _draw_args(count, seed, stream, call, 'random_nodes')
  n = _node_count(n, 'random_nodes')
  device = _sampling_device(device, 'random_nodes')
  out = torch.empty(count, dtype=torch.int64, device=device)
  if count:
    check(_lib.lib().gnpde_random_nodes(n, count, seed, stream, call, ptr(out), _stream_on(device)))
  return out


def node_importance(edge_index, att_mean, n):
  """[n] float32: per node, the mean of att_mean ([E] float32, in the order of edge_index's columns) over its INCOMING edges
  (column index = the node), summed in a fixed order (gnpde_node_importance).  Raises GnpdeError when a node has no incoming
  edge."""
  from .graph import graph_of
  ei = _edge_list(edge_index, 'node_importance: edge_index')
  require_hip(att_mean)
  n = _node_count(n, 'node_importance')
  att = f32c(att_mean.detach().reshape(-1), 'att_mean')
  if att.numel() != ei.shape[1]:
    raise _lib.GnpdeError('node_importance: %d values for %d edges' % (att.numel(), ei.shape[1]))
  if att.device != ei.device:
    raise _lib.GnpdeError('node_importance: att_mean is on %s but edge_index is on %s' % (att.device, ei.device))
  if ei.shape[1] > INT32_MAX:
    raise _lib.GnpdeError('node_importance: %d edges exceed int32 positions' % ei.shape[1])
  if ei.shape[1] == 0:
    raise _lib.GnpdeError('node_importance: ' + SAMPLING_FLAGS[0][1])
  graph = graph_of(edge_index if edge_index.is_contiguous() else ei, n, ei.device)
  out = torch.empty(n, dtype=torch.float32, device=ei.device)
  flag = torch.zeros(1, dtype=torch.int32, device=ei.device)
  check(_lib.lib().gnpde_node_importance(graph.ref(), ptr(att), ptr(out), ptr(flag), stream_of(att)))
  _raise_flags(flag, 'node_importance')
  return out


def sample_nodes(logits, count, seed, stream, call):
  """count draws with replacement from softmax(logits) ([n] float32 on a HIP device) as an int64 vector: the fixed-point
  multinomial of gnpde_sample_nodes (include/gnpde.h has the definition).  Raises GnpdeError for a non-finite logit."""
  if not isinstance(logits, torch.Tensor) or logits.dim() != 1:
    raise _lib.GnpdeError('sample_nodes: logits must be a vector')
  require_hip(logits)
  count, seed, stream, call = _draw_args(count, seed, stream, call, 'sample_nodes')
  s = f32c(logits.detach(), 'logits')
  n = _node_count(s.numel(), 'sample_nodes')
  out = torch.empty(count, dtype=torch.int64, device=s.device)
  if count == 0:
    return out
  L = _lib.lib()
  flag = torch.zeros(1, dtype=torch.int32, device=s.device)
  ws = torch.empty(int(L.gnpde_sample_nodes_workspace_bytes(n)), dtype=torch.uint8, device=s.device)
  check(L.gnpde_sample_nodes(ptr(s), n, count, seed, stream, call, ptr(out), ptr(flag), ptr(ws), ws.numel(), stream_of(s)))
  _raise_flags(flag, 'sample_nodes')
  return out


def edge_union(a, b, n):
  """The unique columns of cat(a, b) ([2, *] int64 device edge lists over n nodes), ascending by (row, col): what
  torch.unique(torch.cat([a, b], dim=1), dim=1) returns (gnpde_edge_union); one host read for the count."""
  a = _edge_list(a, 'edge_union: a')
  b = _edge_list(b, 'edge_union: b')
  if a.device != b.device:
    raise _lib.GnpdeError('edge_union: a is on %s but b is on %s' % (a.device, b.device))
  n = _node_count(n, 'edge_union')
  ea, eb = a.shape[1], b.shape[1]
  if ea + eb == 0:
    return torch.empty(2, 0, dtype=torch.int64, device=a.device)
  L = _lib.lib()
  out = torch.empty(2, ea + eb, dtype=torch.int64, device=a.device)
  cnt = torch.zeros(1, dtype=torch.int64, device=a.device)
  flag = torch.zeros(1, dtype=torch.int32, device=a.device)
  ws = torch.empty(int(L.gnpde_edge_union_workspace_bytes(ea, eb)), dtype=torch.uint8, device=a.device)
  check(L.gnpde_edge_union(ptr(a), ea, ptr(b), eb, n, ptr(out), ptr(cnt), ptr(flag), ptr(ws), ws.numel(), stream_of(a)))
  _raise_flags(flag, 'edge_union')
  return out[:, :int(cnt.item())].contiguous()


def select_edges(edge_index, score, threshold):
  """edge_index[:, score >= threshold], the kept columns in their order (gnpde_select_edges): stable compaction, no weights, no
  renormalisation (threshold_edges keeps `>` and renormalises).  threshold: a device scalar (e.g. ops.quantile's) or a number."""
  ei = _edge_list(edge_index, 'select_edges: edge_index')
  require_hip(score)
  sc = f32c(score.detach().reshape(-1), 'score')
  E = ei.shape[1]
  if sc.numel() != E:
    raise _lib.GnpdeError('select_edges: %d scores for %d edges' % (sc.numel(), E))
  if sc.device != ei.device:
    raise _lib.GnpdeError('select_edges: score is on %s but edge_index is on %s' % (sc.device, ei.device))
  if E == 0:
    return ei.clone()
  if isinstance(threshold, torch.Tensor):
    require_hip(threshold)
    thr = threshold.detach().to(torch.float32).reshape(1)
  else:
    thr = torch.full((1,), float(threshold), dtype=torch.float32, device=ei.device)
  L = _lib.lib()
  out = torch.empty_like(ei)
  cnt = torch.zeros(1, dtype=torch.int64, device=ei.device)
  ws = torch.empty(int(L.gnpde_select_edges_workspace_bytes(E)), dtype=torch.uint8, device=ei.device)
  check(L.gnpde_select_edges(ptr(ei), ptr(sc), E, ptr(thr), ptr(out), ptr(cnt), ptr(ws), ws.numel(), stream_of(sc)))
  return out[:, :int(cnt.item())].contiguous()


def full_adjacency(n, device=None):
  """All n^2 pairs [2, n^2] int64, row-major, the diagonal included (the reference's utils.get_full_adjacency).  n^2 <= INT32_MAX:
  positions of an edge set are int32."""
  n = int(n)
  if n < 1 or n * n > INT32_MAX:
    raise _lib.GnpdeError('full_adjacency: n = %d (n^2 must lie in 1 .. INT32_MAX: edge positions are int32)' % n)
  device = _sampling_device(device, 'full_adjacency')
  out = torch.empty(2, n * n, dtype=torch.int64, device=device)
  check(_lib.lib().gnpde_full_adjacency(n, ptr(out), _stream_on(device)))
  return out


# ---- DeepWalk positional encodings (csrc/deepwalk.hip; definitions in include/gnpde.h) -------------------------------------------
DEEPWALK_FLAGS = ((_lib.DEEPWALK_BAD_START, 'a start node lies outside [0, n)'),
                  (_lib.DEEPWALK_BAD_GRAPH, 'a rowptr / col entry of the walk graph lies outside the graph'),
                  (_lib.DEEPWALK_BAD_WALK, 'a walk entry lies outside [0, n)'))
DEEPWALK_MAX_WALK_LENGTH = 127
DEEPWALK_MAX_DIM = 256
DEEPWALK_LDS_FLOATS = 16384
STREAM_POS_WALKS, STREAM_NEG_WALKS, STREAM_EPOCH_ORDER = 16, 17, 18     # graph_rewiring's edge sampling uses streams 0 and 1


class WalkGraph(object):
  """CSR of the walk graph on the device: rowptr [n + 1] and col [E] int32, a node's out-neighbours with multiplicity, ascending."""

  def __init__(self, rowptr, col, n):
    self.rowptr, self.col, self.n = rowptr, col, int(n)


def walk_csr(edge_index, n):
  """WalkGraph of edge_index ([2, E] int64 on a HIP device): the out-neighbours of u are the dst of the edges (u, dst), with
  multiplicity, ascending by dst.  Torch device ops, once per graph; one host read checks the index range."""
  ei = _edge_list(edge_index, 'walk_csr: edge_index')
  n = _node_count(n, 'walk_csr')
  E = ei.shape[1]
  if E > INT32_MAX:
    raise _lib.GnpdeError('walk_csr: %d edges exceed int32 positions' % E)
  if E and (int(ei.min()) < 0 or int(ei.max()) >= n):
    raise _lib.GnpdeError('walk_csr: an edge index lies outside [0, n)')
  key = torch.sort(ei[0] * n + ei[1]).values
  src = torch.div(key, n, rounding_mode='floor')
  rowptr = torch.zeros(n + 1, dtype=torch.int64, device=ei.device)
  if E:
    rowptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
  return WalkGraph(rowptr.to(torch.int32), (key - src * n).to(torch.int32), n)


def _walk_args(starts, walk_length, seed, stream, call, first_walk, repeats, who):
  if not isinstance(starts, torch.Tensor) or starts.dim() != 1:
    raise _lib.GnpdeError('%s: starts must be a vector' % who)
  require_hip(starts)
  if starts.dtype != torch.int64:
    raise _lib.GnpdeError('%s: starts must be int64 (got %s)' % (who, starts.dtype))
  L, repeats, first_walk = int(walk_length), int(repeats), int(first_walk)
  if not 1 <= L <= DEEPWALK_MAX_WALK_LENGTH:
    raise _lib.GnpdeError('%s: walk_length = %d outside 1 .. %d' % (who, L, DEEPWALK_MAX_WALK_LENGTH))
  if repeats < 1 or not 0 <= first_walk < 2 ** 64:
    raise _lib.GnpdeError('%s: repeats = %d / first_walk = %d out of range' % (who, repeats, first_walk))
  _, seed, stream, call = _draw_args(0, seed, stream, call, who)
  st = starts.detach()
  return (st if st.is_contiguous() else st.contiguous()), L, seed, stream, call, first_walk, repeats


def random_walks(edge_index, n, starts, walk_length, seed, stream, call, first_walk=0, *, repeats=1, dtype=torch.int64, flag=None):
  """[R, walk_length + 1] uniform random walks (gnpde_random_walks; include/gnpde.h has the definition): walk r starts at
  starts[r % len(starts)], R = len(starts) * repeats, and is walk first_walk + r of the Philox stream (seed, stream, call).
  edge_index: [2, E] int64 on a HIP device, or a WalkGraph (ops.walk_csr) to build the CSR once.  flag: a device int32 the caller
  reads itself (no host read here); otherwise a start outside [0, n) raises."""
  who = 'random_walks'
  st, L, seed, stream, call, first_walk, repeats = _walk_args(starts, walk_length, seed, stream, call, first_walk, repeats, who)
  g = edge_index if isinstance(edge_index, WalkGraph) else walk_csr(edge_index, n)
  if g.n != int(n):
    raise _lib.GnpdeError('random_walks: the walk graph has %d nodes, not %d' % (g.n, int(n)))
  if g.rowptr.device != st.device:
    raise _lib.GnpdeError('random_walks: starts is on %s but the graph is on %s' % (st.device, g.rowptr.device))
  R = st.numel() * repeats
  out = torch.empty(R, L + 1, dtype=torch.int32, device=st.device)
  if R:
    own = flag is None
    if own:
      flag = torch.zeros(1, dtype=torch.int32, device=st.device)
    check(_lib.lib().gnpde_random_walks(ptr(g.rowptr), ptr(g.col), g.col.numel(), g.n, ptr(st), st.numel(), R, L, seed, stream, call, first_walk,
                                        ptr(out), ptr(flag), stream_of(st)))
    if own:
      _raise_flags(flag, who, DEEPWALK_FLAGS)
  return out if dtype == torch.int32 else out.to(dtype)


def negative_walks(n, starts, walk_length, seed, stream, call, first_walk=0, *, repeats=1, dtype=torch.int64, flag=None):
  """[R, walk_length + 1]: column 0 the start node (starts[r % len(starts)]), every other column uniform over [0, n)
  (gnpde_negative_walks): PyG's negative sample of Node2Vec on this package's Philox streams."""
  who = 'negative_walks'
  st, L, seed, stream, call, first_walk, repeats = _walk_args(starts, walk_length, seed, stream, call, first_walk, repeats, who)
  n = _node_count(n, 'negative_walks')
  R = st.numel() * repeats
  out = torch.empty(R, L + 1, dtype=torch.int32, device=st.device)
  if R:
    own = flag is None
    if own:
      flag = torch.zeros(1, dtype=torch.int32, device=st.device)
    check(_lib.lib().gnpde_negative_walks(n, ptr(st), st.numel(), R, L, seed, stream, call, first_walk, ptr(out), ptr(flag), stream_of(st)))
    if own:
      _raise_flags(flag, who, DEEPWALK_FLAGS)
  return out if dtype == torch.int32 else out.to(dtype)


def random_permutation(n, seed, stream, call, device=None):
  """A permutation of range(n) as an int64 device vector: the indices sorted by (word i of the stream) << 32 | i
  (gnpde_random_permutation).  1 <= n <= INT32_MAX."""
  _, seed, stream, call = _draw_args(0, seed, stream, call, 'random_permutation')
  n = _node_count(n, 'random_permutation')
  device = _sampling_device(device, 'random_permutation')
  L = _lib.lib()
  out = torch.empty(n, dtype=torch.int64, device=device)
  ws = torch.empty(int(L.gnpde_random_permutation_workspace_bytes(n)), dtype=torch.uint8, device=device)
  check(L.gnpde_random_permutation(n, seed, stream, call, ptr(out), ptr(ws), ws.numel(), _stream_on(device)))
  return out


def deepwalk_check_shape(walk_length, context_size, d, who='deepwalk_step'):
  """Raise for a shape the native step refuses (the limits of include/gnpde.h)."""
  L, C, d = int(walk_length), int(context_size), int(d)
  if not 1 <= L <= DEEPWALK_MAX_WALK_LENGTH:
    raise _lib.GnpdeError('%s: walk_length = %d outside 1 .. %d' % (who, L, DEEPWALK_MAX_WALK_LENGTH))
  if not 2 <= C <= L:
    raise _lib.GnpdeError('%s: walk_length >= context_size >= 2 is required (walk_length %d, context_size %d)' % (who, L, C))
  if d % 4 != 0 or not 4 <= d <= DEEPWALK_MAX_DIM:
    raise _lib.GnpdeError('%s: the embedding width %d must be a multiple of 4 in 4 .. %d' % (who, d, DEEPWALK_MAX_DIM))
  if (L + 1) * d + (L + 2 - C) * (C - 1) > DEEPWALK_LDS_FLOATS:
    raise _lib.GnpdeError('%s: (walk_length + 1) * width + windows * (context_size - 1) = %d exceeds %d floats (64 KiB of LDS)'
                          % (who, (L + 1) * d + (L + 2 - C) * (C - 1), DEEPWALK_LDS_FLOATS))


def _state_rows(t, name):
  if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
    raise _lib.GnpdeError('deepwalk_step: %s must be a float32 matrix' % name)
  require_hip(t)
  if t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.stride(0) % 4 != 0 or t.data_ptr() % 16 != 0:
    raise _lib.GnpdeError('deepwalk_step: %s is updated in place: unit column stride, a row stride that is a multiple of 4 and '
                          '16-byte alignment are required' % name)
  return t


def _walks_i32(rw, L, name):
  if not isinstance(rw, torch.Tensor) or rw.dim() != 2 or rw.dtype not in (torch.int32, torch.int64):
    raise _lib.GnpdeError('deepwalk_step: %s must be an int32 / int64 matrix [R, walk_length + 1]' % name)
  require_hip(rw)
  if L is not None and rw.shape[1] != L + 1:
    raise _lib.GnpdeError('deepwalk_step: %s has %d columns, pos_rw has %d' % (name, rw.shape[1], L + 1))
  rw = rw.detach().to(torch.int32)
  return rw if rw.is_contiguous() else rw.contiguous()


def deepwalk_workspace(r_pos, r_neg, walk_length, context_size, d, device):
  need = int(_lib.lib().gnpde_deepwalk_step_workspace_bytes(int(r_pos), int(r_neg), int(walk_length), int(context_size), int(d)))
  if need == 0:
    raise _lib.GnpdeError('deepwalk_step: the workspace query failed (%s)'
                          % (_lib.lib().gnpde_last_error().decode(errors='replace') or "the sort's temporary-storage query needs a device"))
  return torch.empty(need, dtype=torch.uint8, device=device)


def deepwalk_step(emb, m, v, t, pos_rw, neg_rw, context_size, lr=0.01, betas=(0.9, 0.999), eps=1e-8, *, loss_out=None, flag=None, workspace=None):
  """One skip-gram-with-negative-sampling step with the SparseAdam update, in place on emb, m, v ([n, d] float32 on a HIP device;
  emb may have padded rows): gnpde_deepwalk_step, include/gnpde.h has the definition.  pos_rw [R_pos, L + 1], neg_rw [R_neg, L + 1]:
  the walks (int32 or int64).  t: the global step count from 1.  Returns the step's loss as a 0-d device tensor; nothing is read by
  the host unless `flag` is None (then a walk entry outside [0, n) raises).  loss_out: a 1-element float32 device view to write
  the loss to; workspace: a buffer from deepwalk_workspace to reuse."""
  emb = _state_rows(emb, 'emb')
  m, v = _state_rows(m, 'm'), _state_rows(v, 'v')
  if m.shape != emb.shape or v.shape != emb.shape or m.stride(0) != v.stride(0):
    raise _lib.GnpdeError('deepwalk_step: m and v must have the shape of emb and one row stride')
  n, d = emb.shape
  pos = _walks_i32(pos_rw, None, 'pos_rw')
  L = pos.shape[1] - 1
  neg = _walks_i32(neg_rw, L, 'neg_rw')
  deepwalk_check_shape(L, context_size, d)
  n = _node_count(n, 'deepwalk_step')
  if pos.shape[0] < 1 or neg.shape[0] < 1:
    raise _lib.GnpdeError('deepwalk_step: at least one positive and one negative walk are needed')
  if not (emb.device == m.device == v.device == pos.device == neg.device):
    raise _lib.GnpdeError('deepwalk_step: the tensors are on different devices')
  if workspace is None:
    workspace = deepwalk_workspace(pos.shape[0], neg.shape[0], L, context_size, d, emb.device)
  own = flag is None
  if own:
    flag = torch.zeros(1, dtype=torch.int32, device=emb.device)
  if loss_out is None:
    loss_out = torch.empty(1, dtype=torch.float32, device=emb.device)
  check(_lib.lib().gnpde_deepwalk_step(ptr(emb), emb.stride(0), ptr(m), ptr(v), m.stride(0), n, d, int(t), ptr(pos), pos.shape[0], ptr(neg),
                                       neg.shape[0], L, int(context_size), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                       ptr(loss_out), ptr(flag), ptr(workspace), workspace.numel(), stream_of(emb)))
  if own:
    _raise_flags(flag, 'deepwalk_step', DEEPWALK_FLAGS)
  return loss_out.reshape(())


# ---- hyperbolic positional encodings (csrc/hyperbolic.hip; definitions in include/gnpde.h) ---------------------------------------
POINCARE_MAX_DIM = 128
STREAM_HYP_POS_WALKS, STREAM_HYP_NEG_WALKS, STREAM_HYP_EPOCH_ORDER = 19, 20, 21     # DeepWalk's streams are 16, 17, 18
POINCARE_BALL_EDGE = 1 - 1e-5


def _up4(x):
  return (x + 3) // 4 * 4


def poincare_check_shape(walk_length, context_size, d, who='poincare_step'):
  """Raise for a shape the native Poincare step refuses (the limits of include/gnpde.h)."""
  L, C, d = int(walk_length), int(context_size), int(d)
  if not 1 <= L <= DEEPWALK_MAX_WALK_LENGTH:
    raise _lib.GnpdeError('%s: walk_length = %d outside 1 .. %d' % (who, L, DEEPWALK_MAX_WALK_LENGTH))
  if not 2 <= C <= L:
    raise _lib.GnpdeError('%s: walk_length >= context_size >= 2 is required (walk_length %d, context_size %d)' % (who, L, C))
  if d != 2 and (d % 4 != 0 or not 4 <= d <= POINCARE_MAX_DIM):
    raise _lib.GnpdeError('%s: the embedding width %d must be 2 or a multiple of 4 in 4 .. %d' % (who, d, POINCARE_MAX_DIM))
  floats = (L + 1) * max(d, 4) + _up4(L + 1) + 2 * _up4((L + 2 - C) * (C - 1))
  if floats > DEEPWALK_LDS_FLOATS:
    raise _lib.GnpdeError('%s: (walk_length + 1) * width + the walk_length + 1 norms + 2 * windows * (context_size - 1) = %d exceeds %d '
                          'floats (64 KiB of LDS)' % (who, floats, DEEPWALK_LDS_FLOATS))


def poincare_workspace(r_pos, r_neg, walk_length, context_size, d, device):
  need = int(_lib.lib().gnpde_poincare_step_workspace_bytes(int(r_pos), int(r_neg), int(walk_length), int(context_size), int(d)))
  if need == 0:
    raise _lib.GnpdeError('poincare_step: the workspace query failed (%s)'
                          % (_lib.lib().gnpde_last_error().decode(errors='replace') or "the sort's temporary-storage query needs a device"))
  return torch.empty(need, dtype=torch.uint8, device=device)


def poincare_step(emb, pos_rw, neg_rw, context_size, lr=1.0, radius=2.0, temperature=1.0, *, loss_out=None, flag=None, workspace=None):
  """One row-normalised Riemannian SGD step on the Poincare ball, in place on emb ([n, d] float32 on a HIP device, every row inside
  the unit ball; padded rows allowed): gnpde_poincare_step, include/gnpde.h has the definition.  pos_rw [R_pos, L + 1], neg_rw
  [R_neg, L + 1]: the walks (int32 or int64).  Returns the step's loss as a 0-d device tensor; nothing is read by the host unless
  `flag` is None (then a walk entry outside [0, n) raises).  loss_out: a 1-element float32 device view to write the loss to;
  workspace: a buffer from poincare_workspace to reuse."""
  who = 'poincare_step'
  if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or emb.dtype != torch.float32:
    raise _lib.GnpdeError('poincare_step: emb must be a float32 matrix')
  require_hip(emb)
  n, d = emb.shape
  pos = _walks_i32(pos_rw, None, 'pos_rw')
  L = pos.shape[1] - 1
  neg = _walks_i32(neg_rw, L, 'neg_rw')
  poincare_check_shape(L, context_size, d)
  quantum = 2 if d == 2 else 4
  if emb.stride(1) != 1 or emb.stride(0) < d or emb.stride(0) % quantum != 0 or emb.data_ptr() % (4 * quantum) != 0:
    raise _lib.GnpdeError('poincare_step: emb is updated in place: unit column stride, a row stride that is a multiple of %d and '
                          '%d-byte alignment are required' % (quantum, 4 * quantum))
  n = _node_count(n, who)
  if pos.shape[0] < 1 or neg.shape[0] < 1:
    raise _lib.GnpdeError('poincare_step: at least one positive and one negative walk are needed')
  if not (emb.device == pos.device == neg.device):
    raise _lib.GnpdeError('poincare_step: the tensors are on different devices')
  if not (float(lr) >= 0 and float(temperature) > 0):
    raise _lib.GnpdeError('poincare_step: lr >= 0 and temperature > 0 are required (lr %r, temperature %r)' % (lr, temperature))
  if workspace is None:
    workspace = poincare_workspace(pos.shape[0], neg.shape[0], L, context_size, d, emb.device)
  own = flag is None
  if own:
    flag = torch.zeros(1, dtype=torch.int32, device=emb.device)
  if loss_out is None:
    loss_out = torch.empty(1, dtype=torch.float32, device=emb.device)
  check(_lib.lib().gnpde_poincare_step(ptr(emb), emb.stride(0), n, d, ptr(pos), pos.shape[0], ptr(neg), neg.shape[0], L, int(context_size),
                                       float(lr), float(radius), float(temperature), ptr(loss_out), ptr(flag), ptr(workspace),
                                       workspace.numel(), stream_of(emb)))
  if own:
    _raise_flags(flag, who, DEEPWALK_FLAGS)
  return loss_out.reshape(())


KNN_MAX_K = 128
METRICS ={'sqeuclidean': _lib.METRIC_SQEUCLIDEAN, 'poincare': _lib.METRIC_POINCARE}


def _metric(metric, who):
  if metric not in METRICS:
    raise _lib.GnpdeError('%s: unknown metric %r (one of %s)' % (who, metric, ', '.join(sorted(METRICS))))
  return METRICS[metric]


def _rows_for_tiles(x, who):
  """The [n, d] float32 device matrix the tile kernels read (padded rows with unit column stride in place)."""
  if not isinstance(x, torch.Tensor) or x.dim() != 2:
    raise _lib.GnpdeError('%s: x must be a [n, d] tensor' % who)
  require_hip(x)
  x = _lib.f32rows(x.detach(), who + ' input')
  n, d = x.shape
  if n < 1 or d < 1:
    raise _lib.GnpdeError('%s: empty input [%d, %d]' % (who, n, d))
  if n >= 2 ** 31 or x.stride(0) >= 2 ** 31:
    raise _lib.GnpdeError('%s: n = %d exceeds int32 indices' % (who, n))
  return x


def knn(x, k, return_dist=False, metric='sqeuclidean'):
  """The k nearest rows of every row of x ([n, d] float32 on a HIP device; padded rows with unit column stride are read in
  place), the row itself included: indices int64 [n, k], ascending by (key, index), and with return_dist the distances [n, k]
  (gnpde_knn_metric: key tiles on the fp32 matrix cores, selection in LDS).  metric 'sqeuclidean': the key and the returned
  distance are the squared Euclidean distance (replaces the pykeops argKmin of the reference's graph_rewiring.KNN).  metric
  'poincare': rows are points of the Poincare ball, the key is r = |x_i - x_j|^2 / ((1 - |x_i|^2)(1 - |x_j|^2)) and the returned
  distance the hyperbolic arccosh(1 + 2 r) (include/gnpde.h has the definition; replaces hyperbolize + NearestNeighbors(metric=
  'precomputed') of the reference's apply_dist_KNN).  A row is its own first neighbour at distance exactly 0.
  1 <= k <= min(n, 128)."""
  m = _metric(metric, 'knn')
  x = _rows_for_tiles(x, 'knn')
  n, d = x.shape
  k = int(k)
  if k < 1 or k > n or k > KNN_MAX_K:
    raise _lib.GnpdeError('knn: k = %d outside 1 .. min(n = %d, %d) (d = %d)' % (k, n, KNN_MAX_K, d))
  L = _lib.lib()
  idx = torch.empty(n, k, dtype=torch.int64, device=x.device)
  dist = torch.empty(n, k, dtype=torch.float32, device=x.device) if return_dist else None
  ws = torch.empty(max(int(L.gnpde_knn_workspace_bytes(n, d, k)), 1), dtype=torch.uint8, device=x.device)
  check(L.gnpde_knn_metric(ptr(x), n, d, x.stride(0), k, m, ptr(idx), ptr(dist), ptr(ws), ws.numel(), stream_of(x)))
  return (idx, dist) if return_dist else idx


def key_to_distance(key, metric='sqeuclidean'):
  """The distance a key stands for, in float64: sqrt(key) ('sqeuclidean') or arccosh(1 + 2 key) ('poincare', as
  log1p(2 r + 2 sqrt(r (r + 1))))."""
  import math
  key = float(key)
  if METRICS[metric] == _lib.METRIC_POINCARE:
    return math.log1p(2.0 * key + 2.0 * math.sqrt(key * (key + 1.0))) if math.isfinite(key) else key
  return math.sqrt(key)


def distance_to_key(dist, metric='sqeuclidean'):
  """The largest float32 key whose float64 distance (key_to_distance) is <= dist: the radius graph {distance <= dist} is the set
  {key <= that key}.  dist >= 0.  Exact inverse of key_to_distance on float32 keys."""
  import math
  import numpy as np
  dist = float(dist)
  if not dist >= 0.0:
    raise _lib.GnpdeError('radius_graph: threshold = %r is no distance (>= 0)' % (dist,))
  if math.isinf(dist):
    return float('inf')
  if METRICS[metric] == _lib.METRIC_POINCARE:
    guess = math.sinh(0.5 * dist) ** 2 if dist < 700.0 else float('inf')     # (cosh t - 1) / 2
  else:
    guess = dist * dist
  top = np.float32(np.finfo(np.float32).max)
  key = np.float32(min(guess, float(top)))
  with np.errstate(over='ignore'):
    while key > 0 and key_to_distance(key, metric) > dist:
      key = np.nextafter(key, np.float32(0))
    while key < top and key_to_distance(np.nextafter(key, top), metric) <= dist:
      key = np.nextafter(key, top)
  return float(key)


def radius_graph(x, *, quantile=None, threshold=None, metric='sqeuclidean', max_edges=2 ** 28, return_threshold=False):
  """edge_index [2, E] int64, sorted by (row, column), of every pair (i, j) -- self loops included -- of the rows of x ([n, d]
  float32 on a HIP device, padded rows read in place) whose distance is within a radius: what np.where(dist <= thresh) gives on
  the dense distance matrix (the reference's distances_kNN.apply_dist_threshold), without that matrix.
  Exactly one of:  quantile = q in [0, 1]: the radius is the key of rank floor((n^2 - 1) q) among all n^2 keys, which selects the
  set np.quantile's interpolated threshold selects (include/gnpde.h has the argument);  threshold = a distance (Euclidean for
  'sqeuclidean', hyperbolic for 'poincare'), turned into a key on the host (distance_to_key).
  Raises GnpdeError when E > max_edges, after the count and before anything of size E is allocated.
  return_threshold: (edge_index, tau_key, tau_distance) -- the key that was used (float32 value) and key_to_distance of it in
  float64, so that threshold=tau_distance selects the same set; for a quantile it is the LOWER order statistic, not numpy's
  interpolated number."""
  m = _metric(metric, 'radius_graph')
  if (quantile is None) == (threshold is None):
    raise _lib.GnpdeError('radius_graph: give exactly one of quantile= and threshold=')
  if quantile is not None:
    q = float(quantile)
    if not (0.0 <= q <= 1.0):
      raise _lib.GnpdeError('radius_graph: quantile = %r outside [0, 1]' % (quantile,))
    tau_key = None
  else:
    tau_key = distance_to_key(threshold, metric)
  x = _rows_for_tiles(x, 'radius_graph')
  n, d = x.shape
  dev = x.device
  L = _lib.lib()
  ws = torch.empty(max(int(L.gnpde_radius_workspace_bytes(n, d)), 1), dtype=torch.uint8, device=dev)
  tau_dev = None
  if tau_key is None:
    tau_dev = torch.empty(2, dtype=torch.float32, device=dev)
    check(L.gnpde_radius_quantile(ptr(x), n, d, x.stride(0), m, q, ptr(tau_dev), ptr(ws), ws.numel(), stream_of(x)))
  rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
  given = 0.0 if tau_key is None else tau_key
  check(L.gnpde_radius_count(ptr(x), n, d, x.stride(0), m, ptr(tau_dev), given, ptr(rowptr), ptr(ws), ws.numel(), stream_of(x)))
  E = int(rowptr[-1].item())
  if E > int(max_edges):
    raise _lib.GnpdeError('radius_graph: %d edges exceed max_edges = %d' % (E, int(max_edges)))
  ei = torch.empty(2, E, dtype=torch.int64, device=dev)
  if E > 0:
    check(L.gnpde_radius_fill(ptr(x), n, d, x.stride(0), m, ptr(tau_dev), given, ptr(ei), E, ptr(ws), ws.numel(), stream_of(x)))
  if not return_threshold:
    return ei
  if tau_key is None:
    tau_key = float(tau_dev[0].item())
  return ei, tau_key, key_to_distance(tau_key, metric)


def two_hop(graph, weight):
  """(edge_index [2, nnz] int64, value [nnz]) of coalesce(A ++ offdiag(A A)) / 2 for the operator A = (graph, weight in the
  caller's edge order): the densification step of the rewiring block (gnpde_two_hop_count / _fill); one host read for nnz."""
  require_hip(weight)
  w = f32c(weight.detach().reshape(-1), 'weight')
  dev = w.device
  if graph.e == 0:
    return torch.zeros(2, 0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
  L = _lib.lib()
  w_csr = w[graph.perm_long].contiguous()
  rowptr, col = graph.t['rowptr'], graph.t['colidx']
  ws = graph.workspace('two_hop', int(L.gnpde_two_hop_workspace_bytes(graph.n)))   # kept on the graph: a training forward re-runs this
  out_rowptr = torch.empty(graph.n + 1, dtype=torch.int64, device=dev)
  check(L.gnpde_two_hop_count(ptr(rowptr), ptr(col), graph.n, ptr(out_rowptr), ptr(ws), ws.numel(), stream_of(w)))
  nnz = int(out_rowptr[-1].item())
  out_ei = torch.empty(2, nnz, dtype=torch.int64, device=dev)
  out_w = torch.empty(nnz, dtype=torch.float32, device=dev)
  if nnz > 0:
    check(L.gnpde_two_hop_fill(ptr(rowptr), ptr(col), ptr(w_csr), graph.n, ptr(out_rowptr), ptr(out_ei), nnz, ptr(out_w),
                               ptr(ws), ws.numel(), stream_of(w)))
  return out_ei, out_w


GDC_MAX_K = 128
GDC_MAX_TERMS = 4096        # M of the truncated series
GDC_DENSE_CAP = 2 << 30     # bytes of the [n, n] matrix the dense mode agrees to write


def gdc_terms(method, param, tol=1e-6):
  """The coefficients theta_0 .. theta_M of S = sum_m theta_m T^m that `gdc` uses (pure Python, float64):
  'ppr' (param = alpha): theta_m = alpha (1 - alpha)^m;  'heat' (param = t): theta_m = e^-t t^m / m!;  'coeff' (param = a list): the
  list as given.  M is the smallest with 1 - sum_{m <= M} theta_m <= tol."""
  import math
  if method == 'coeff':
    theta = [float(c) for c in param]
    if not theta or len(theta) > GDC_MAX_TERMS + 1 or any(not math.isfinite(c) or c < 0 for c in theta):
      raise ValueError('gdc: coeffs must be 1 .. %d finite non-negative numbers' % (GDC_MAX_TERMS + 1))
    return theta
  tol = float(tol)
  if not 0.0 < tol < 1.0:
    raise ValueError('gdc: tol = %r outside (0, 1)' % tol)
  if method == 'ppr':
    alpha = float(param)
    if not 0.0 < alpha <= 1.0:
      raise ValueError('gdc: ppr alpha = %r outside (0, 1]' % alpha)
    term = lambda m: alpha * (1.0 - alpha) ** m
  elif method == 'heat':
    t = float(param)
    if not (t >= 0.0 and math.isfinite(t)):
      raise ValueError('gdc: heat t = %r is not a finite non-negative number' % t)
    term = lambda m: math.exp(m * math.log(t) - t - math.lgamma(m + 1.0)) if t > 0.0 else (1.0 if m == 0 else 0.0)
  else:
    raise ValueError("gdc: method %r is not 'ppr', 'heat' or 'coeff'" % (method,))
  theta = []
  while True:
    theta.append(term(len(theta)))
    if 1.0 - math.fsum(theta) <= tol:
      return theta
    if len(theta) > GDC_MAX_TERMS:
      raise ValueError('gdc: the series needs more than %d terms for tol = %g (%s, %r)' % (GDC_MAX_TERMS, tol, method, param))


def _segment_sums(w_sorted, counts, divide=False):
  """Sums of the consecutive segments of w_sorted with the given lengths (int64 device tensor), formed in a fixed order
  (gnpde_gdc_segment_sums: no atomics); divide: w_sorted is divided by its segment's sum in place (0 for a zero sum)."""
  offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=w_sorted.device)
  torch.cumsum(counts, 0, out=offsets[1:])
  sums = torch.zeros(counts.numel(), dtype=torch.float32, device=w_sorted.device)
  if counts.numel() and w_sorted.numel():
    check(_lib.lib().gnpde_gdc_segment_sums(ptr(w_sorted), ptr(offsets), counts.numel(), ptr(sums), int(bool(divide)),
                                            stream_of(w_sorted)))
  return sums


def _sums_by(index, w, n):
  """sums[i] = sum of w over index == i, deterministic (stable sort + fixed-order segment sums)."""
  order = torch.sort(index, stable=True).indices
  return _segment_sums(w[order].contiguous(), torch.bincount(index, minlength=n))


def _gdc_normalise(row, col, w, n, kind):
  """Step 2 / 5 of the definition on a coalesced list; the reciprocal of zero is 0."""
  if kind is None:
    return w
  inv = lambda s, p: torch.where(s > 0, s.double().pow(p).float(), torch.zeros_like(s))
  if kind == 'sym':
    r = inv(_sums_by(row, w, n), -0.5)
    return w * r[row] * r[col]
  if kind in ('col', 'row'):
    idx = col if kind == 'col' else row
    s = _sums_by(idx, w, n)[idx]
    return torch.where(s > 0, w / s, torch.zeros_like(w))
  raise ValueError("gdc: normalisation %r is not 'sym', 'col', 'row' or None" % (kind,))


def gdc_transition(edge_index, edge_weight, n, self_loop_weight=1.0, normalization_in='sym'):
  """Steps 1-2 of the definition in include/gnpde.h (device tensors): (row, col, w) of T, coalesced and sorted by (row, col)."""
  dev = edge_index.device
  row, col = edge_index[0].long(), edge_index[1].long()
  w = torch.ones(row.numel(), dtype=torch.float32, device=dev) if edge_weight is None else f32c(edge_weight.detach().reshape(-1), 'edge_weight')
  if w.numel() != row.numel():
    raise ValueError('gdc: %d weights for %d edges' % (w.numel(), row.numel()))
  # every term of the series must be non-negative: the error bound is relative and the selection keys order positive floats
  if edge_weight is not None and w.numel() and not bool((torch.isfinite(w) & (w >= 0)).all()):
    raise ValueError('gdc: edge weights must be finite and non-negative')
  self_loop_weight = float(self_loop_weight or 0.0)
  if not 0.0 <= self_loop_weight < float('inf'):
    raise ValueError('gdc: self_loop_weight = %r is not a finite non-negative number' % (self_loop_weight,))
  if row.numel() and (int(torch.minimum(row.min(), col.min())) < 0 or int(torch.maximum(row.max(), col.max())) >= n):
    raise ValueError('gdc: edge index outside [0, %d)' % n)
  if self_loop_weight:
    loop = torch.arange(n, dtype=torch.int64, device=dev)
    row, col = torch.cat([row, loop]), torch.cat([col, loop])
    w = torch.cat([w, torch.full((n,), self_loop_weight, dtype=torch.float32, device=dev)])
  key, order = torch.sort(row * n + col, stable=True)
  uniq, counts = torch.unique_consecutive(key, return_counts=True)
  w = _segment_sums(w[order].contiguous(), counts)
  row, col = torch.div(uniq, n, rounding_mode='floor'), uniq % n
  return row, col, _gdc_normalise(row, col, w, n, normalization_in)


def _rank_select(pieces, k0, k1, device):
  """[2] float32 device tensor: the order statistics of ascending ranks k0, k1 (0 = the smallest) among all values of the float32
  device tensors that pieces() yields -- the same pieces on each of its four calls (gnpde_rank_select_*: the streaming radix select
  of gnpde_quantile with integer ranks; nothing is sorted or kept)."""
  L = _lib.lib()
  ws = torch.empty(int(L.gnpde_quantile_workspace_bytes()), dtype=torch.uint8, device=device)
  out = torch.empty(2, dtype=torch.float32, device=device)
  stream = _stream_on(device)
  check(L.gnpde_rank_select_begin(int(k0), int(k1), ptr(ws), ws.numel(), stream))
  for p in range(4):
    for v in pieces():
      check(L.gnpde_rank_select_hist(ptr(v), v.numel(), p, ptr(ws), ws.numel(), stream))
    check(L.gnpde_rank_select_pick(p, ptr(ws), ws.numel(), stream))
  check(L.gnpde_rank_select_values(ptr(out), ptr(ws), ws.numel(), stream))
  return out


def _avg_degree_eps(pieces, n_fed, keep, device):
  """torch_geometric's GDC.__calculate_eps__ without the sort: the mean (float32) of the keep-th and (keep + 1)-th largest of the
  n_fed >= keep + 1 values fed, as a 0-d device tensor."""
  two = _rank_select(pieces, n_fed - keep - 1, n_fed - keep, device)
  return (two[0] + two[1]) * 0.5


def gdc(edge_index, edge_weight, n, *, method, alpha=None, t=None, coeffs=None, k=None, eps=None, avg_degree=None, self_loop_weight=1.0,
        normalization_in='sym', normalization_out='col', tol=1e-6, block=256, dense_out=False, dense_cap_bytes=GDC_DENSE_CAP,
        return_eps=False):
  """Graph diffusion rewiring (the definition is in include/gnpde.h): S = sum_m theta_m T^m for 'ppr' (alpha), 'heat' (t) or
  'coeff' (coeffs), truncated by gdc_terms(.., tol); per column the k largest strictly positive entries (k) or the entries >= eps
  (eps); output normalisation over the kept entries.  Returns (edge_index [2, E'] int64 with row = i, col = j for a kept S[i, j],
  edge_weight [E']) grouped by ascending column, within a column by value descending and equal values by ascending row;
  bit-identical from run to run.  dense_out: no sparsification, the normalised [n, n] matrix (refused above dense_cap_bytes).
  Columns are processed in blocks of `block` (a multiple of 4, <= 256) on an [n, block] slab; no [n, n] array exists otherwise.
  Zero entries are never emitted (torch_geometric's dense top-k emits them, in arbitrary order).
  avg_degree (instead of eps): the threshold is the mean of the (avg_degree n)-th and (avg_degree n + 1)-th largest of all n^2
  entries (torch_geometric's __calculate_eps__), found by a streaming radix select that forms every column block once per digit
  pass (four extra sweeps of the diffusion, no sort, no [n, n] array); 1 <= avg_degree < n.  A cut that falls among the zeros keeps
  every positive entry.  return_eps: the threshold used is returned as a third value (a float)."""
  n = int(n)
  if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
    raise ValueError('gdc: edge_index must be [2, E]')
  if n < 1 or n >= 2 ** 31:
    raise ValueError('gdc: n = %d outside 1 .. 2^31 - 1' % n)
  block = int(block)
  if block < 4 or block > 256 or block % 4:
    raise ValueError('gdc: block = %d is not a multiple of 4 in 4 .. 256' % block)
  if normalization_in not in ('sym', 'col', 'row') or normalization_out not in ('sym', 'col', 'row', None):
    raise ValueError('gdc: unknown normalisation (%r in, %r out)' % (normalization_in, normalization_out))
  param = {'ppr': alpha, 'heat': t, 'coeff': coeffs}.get(method)
  if method not in ('ppr', 'heat', 'coeff') or param is None:
    raise ValueError("gdc: method %r needs its parameter (ppr: alpha, heat: t, coeff: coeffs)" % (method,))
  theta = gdc_terms(method, param, tol)
  if not dense_out:
    if (k is not None) + (eps is not None) + (avg_degree is not None) != 1:
      raise ValueError('gdc: give exactly one of k (top-k per column), eps (threshold) and avg_degree (threshold by edge count)')
    if avg_degree is not None and not 1 <= int(avg_degree) < n:
      raise ValueError('gdc: avg_degree = %r outside 1 .. n - 1 (avg_degree >= n keeps the whole dense matrix)' % (avg_degree,))
    if k is not None and not 1 <= int(k) <= GDC_MAX_K:
      raise ValueError('gdc: k = %r outside 1 .. %d' % (k, GDC_MAX_K))
    if eps is not None and not float(eps) > 0.0:
      raise ValueError('gdc: eps = %r is not positive (zeros are never kept)' % (eps,))
  elif 4 * n * n > int(dense_cap_bytes):
    raise _lib.GnpdeError('gdc: the dense %d x %d matrix exceeds the cap of %d bytes' % (n, n, int(dense_cap_bytes)))
  for t in (edge_index, edge_weight):
    if t is not None and not t.is_cuda:
      raise _lib.GnpdeError('gdc runs only on a HIP device (got a %s tensor); there is no CPU fallback' % t.device.type)
  from .graph import CSRGraph
  dev = edge_index.device
  L = _lib.lib()
  row, col, w = gdc_transition(edge_index.detach(), edge_weight, n, self_loop_weight, normalization_in)
  graph = CSRGraph(torch.stack([row, col]), n, dev)            # sorted by (row, col): CSR order is the list's own
  w_csr = w[graph.perm_long].contiguous() if graph.e else w
  theta_dev = torch.tensor(theta, dtype=torch.float32, device=dev)
  kk = 0 if (dense_out or k is None) else int(k)
  ws = torch.empty(max(int(L.gnpde_gdc_workspace_bytes(graph.ref(), block, kk)), 256), dtype=torch.uint8, device=dev)
  slab = torch.empty(n, block, dtype=torch.float32, device=dev)
  stream = stream_of(slab)
  run_block = lambda j0: check(L.gnpde_gdc_block(graph.ref(), ptr(w_csr), ptr(theta_dev), len(theta), j0, block, ptr(slab), ptr(ws),
                                                 ws.numel(), stream))
  i64 = dict(dtype=torch.int64, device=dev)
  if dense_out:
    dense = torch.empty(n, n, dtype=torch.float32, device=dev)
    for j0 in range(0, n, block):
      run_block(j0)
      check(L.gnpde_gdc_dense(graph.ref(), ptr(slab), j0, block, int(normalization_out == 'col'), ptr(dense), int(dense_cap_bytes),
                              ptr(ws), ws.numel(), stream))
    if normalization_out == 'row':
      s = dense.sum(dim=1, keepdim=True)
      dense = torch.where(s > 0, dense / s, torch.zeros_like(dense))
    elif normalization_out == 'sym':
      r = dense.sum(dim=1)
      r = torch.where(r > 0, r.double().pow(-0.5).float(), torch.zeros_like(r))
      dense = dense * r[:, None] * r[None, :]
    return dense
  native_col = normalization_out == 'col'
  if kk:
    keys = torch.empty(n, kk, **i64)               # uint64 bit patterns
    offsets = torch.zeros(n + 1, **i64)
    for j0 in range(0, n, block):
      run_block(j0)
      check(L.gnpde_gdc_topk(graph.ref(), ptr(slab), j0, block, kk, ptr(keys), ptr(offsets[1:]), ptr(ws), ws.numel(), stream))
    torch.cumsum(offsets[1:].clone(), 0, out=offsets[1:])
    total = int(offsets[-1].item())                # the one host read
    out_ei = torch.empty(2, total, **i64)
    out_w = torch.empty(total, dtype=torch.float32, device=dev)
    if total:
      check(L.gnpde_gdc_emit(ptr(keys), ptr(offsets), n, kk, int(native_col), ptr(out_ei), total, ptr(out_w), stream))
  else:
    if avg_degree is not None:
      def slabs():
        for j0 in range(0, n, block):
          run_block(j0)
          yield slab.reshape(-1)
      # columns past n of the last slab are zeros: they sit below every rank read here (all values are >= 0)
      n_fed = n * block * ((n + block - 1) // block)
      eps = float(_avg_degree_eps(slabs, n_fed, int(avg_degree) * n, dev).item())
      eps = max(eps, float(torch.finfo(torch.float32).tiny))       # a cut among the zeros: every positive entry
    eps = float(eps)
    parts = []
    counts = torch.zeros(block, **i64)
    offsets = torch.zeros(block + 1, **i64)
    for j0 in range(0, n, block):
      run_block(j0)
      counts.zero_()
      check(L.gnpde_gdc_threshold_count(graph.ref(), ptr(slab), j0, block, eps, ptr(counts), ptr(ws), ws.numel(), stream))
      torch.cumsum(counts, 0, out=offsets[1:])
      total = int(offsets[-1].item())              # one host read per block: the output size is data dependent
      if total == 0:
        continue
      ei = torch.empty(2, total, **i64)
      ew = torch.empty(total, dtype=torch.float32, device=dev)
      check(L.gnpde_gdc_threshold_fill(graph.ref(), j0, block, eps, ptr(offsets), ptr(ei), total, ptr(ew), ptr(ws), ws.numel(), stream))
      # within a column: value descending, equal values by ascending row (the fill wrote ascending rows; both sorts are stable)
      order = torch.sort(ew, descending=True, stable=True).indices
      order = order[torch.sort(ei[1][order], stable=True).indices]
      parts.append((ei[:, order], ew[order]))
    out_ei = torch.cat([p[0] for p in parts], dim=1) if parts else torch.zeros(2, 0, **i64)
    out_w = torch.cat([p[1] for p in parts]) if parts else torch.zeros(0, dtype=torch.float32, device=dev)
    if native_col and out_w.numel():
      _segment_sums(out_w, torch.bincount(out_ei[1], minlength=n), divide=True)
  if normalization_out in ('row', 'sym') and out_w.numel():
    out_w = _gdc_normalise(out_ei[0], out_ei[1], out_w, n, normalization_out)
  if return_eps:
    return out_ei, out_w, (eps if not kk else None)
  return out_ei, out_w


GDC_PUSH_SLOW_BYTES = 1 << 30    # budget of the slow path's per-workgroup scratch areas (36 n bytes each) when slow_groups is not given
GDC_PUSH_SLOW_GROUPS = 256       # and their largest number then (one per compute unit)
GDC_PUSH_RESIDUALS_MAX_N = 4096


def _push_status(status):
  if status:
    raise _lib.GnpdeError('gdc_push: the push kernel reported status %d (1: round guard reached, 2: a column index out of range, '
                          '4: offsets that are not those of the count pass, the source was not written)' % status)


def gdc_push(edge_index, n, alpha, eps, self_loop_weight=1, normalization_in='sym', *, edge_weight=None, batch=None, capacity=-1,
             slow_groups=None, return_info=False, return_residuals=False):
  """Approximate personalised PageRank of EVERY node by forward push (gnpde_gdc_push_*; the definition is in include/gnpde.h): the
  `exact = False` branch of torch_geometric's GDC (diffusion_matrix_approx) without anything dense.  edge_index: the unweighted
  graph; unit self loops are added for self_loop_weight = 1 (None / 0: none), duplicates removed.  p_s(u) is the estimate of
  source s at node u, 0 <= PPR - p < eps deg(u) on an undirected graph.  Returns (edge_index [2, E] int64, values [E]
  float32) sorted by (row, col), one entry per p_s(u) > 0:
    normalization_in 'row': entry [s, u] = p_s(u);  'sym': [s, u] = deg(s)^1/2 p_s(u) deg(u)^-1/2 (0 for degree 0);
    'col': the transpose of the row form, entry [u, s] = p_s(u).
  Bit-identical from run to run and for every batch (sources per launch), capacity (distinct nodes of the LDS hash: -1 the
  built-in 1536, 0 forces every source through the slow path) and slow_groups (scratch areas of the slow path, 36 n bytes each;
  default: as many as fit GDC_PUSH_SLOW_BYTES, at most GDC_PUSH_SLOW_GROUPS; only the areas a call uses are cleared).  Host
  synchronisations: the graph preparation (index check, torch.unique), one read of the output size between the count and the
  fill pass, one read of the fill pass's status word.  return_info: a third value, dict(slow_sources=, residuals=) -- residuals
  [n, n] float32 dense (row s = r_s) with return_residuals, n <= 4096.  Refused, as the reference refuses them: edge weights and
  self_loop_weight other than None / 1 (NotImplementedError)."""
  n = int(n)
  if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
    raise ValueError('gdc_push: edge_index must be [2, E]')
  if n < 1 or n > INT32_MAX:
    raise ValueError('gdc_push: n = %d outside 1 .. 2^31 - 1' % n)
  if edge_weight is not None:
    raise NotImplementedError('gdc_push: a weighted graph needs the exact path (the reference asserts exact for edge weights); '
                              'the push is defined on the unweighted graph')
  if self_loop_weight not in (None, 0, 1):
    raise NotImplementedError('gdc_push: self_loop_weight = %r is not None or 1 (the reference asserts exact or self_loop_weight == 1)'
                              % (self_loop_weight,))
  alpha, eps = float(alpha), float(eps)
  if not 0.0 < alpha < 1.0:
    raise ValueError('gdc_push: alpha = %r outside (0, 1)' % alpha)
  if not (0.0 < eps < float('inf')):
    raise ValueError('gdc_push: eps = %r is not a positive finite number' % eps)
  if normalization_in not in ('sym', 'col', 'row'):
    raise ValueError('gdc_push: normalization_in %r is not sym, col or row' % (normalization_in,))
  if batch is not None and int(batch) < 1:
    raise ValueError('gdc_push: batch = %r is not positive' % (batch,))
  if return_residuals and n > GDC_PUSH_RESIDUALS_MAX_N:
    raise _lib.GnpdeError('gdc_push: the dense residual read-out is for n <= %d (n = %d)' % (GDC_PUSH_RESIDUALS_MAX_N, n))
  if not edge_index.is_cuda:
    raise _lib.GnpdeError('gdc_push runs only on a HIP device (got a %s tensor); there is no CPU fallback' % edge_index.device.type)
  from .graph import CSRGraph
  dev = edge_index.device
  L = _lib.lib()
  row, col = edge_index[0].detach().long(), edge_index[1].detach().long()
  if row.numel() and (int(torch.minimum(row.min(), col.min())) < 0 or int(torch.maximum(row.max(), col.max())) >= n):
    raise ValueError('gdc_push: edge index outside [0, %d)' % n)
  if self_loop_weight:
    loop = torch.arange(n, dtype=torch.int64, device=dev)
    row, col = torch.cat([row, loop]), torch.cat([col, loop])
  key = torch.unique(row * n + col)                              # sorted: CSR order is the list's own
  row, col = torch.div(key, n, rounding_mode='floor'), key % n
  graph = CSRGraph(torch.stack([row, col]), n, dev)
  deg = torch.bincount(row, minlength=n)
  batches = [(0, n)] if batch is None else [(s0, min(int(batch), n - s0)) for s0 in range(0, n, int(batch))]
  widest = max(ns for _, ns in batches)
  if slow_groups is None:
    per_group = int(L.gnpde_gdc_push_workspace_bytes(n, 1, 2)) - int(L.gnpde_gdc_push_workspace_bytes(n, 1, 1))
    slow_groups = max(1, min(GDC_PUSH_SLOW_GROUPS, GDC_PUSH_SLOW_BYTES // max(per_group, 1)))
  slow_groups = int(slow_groups)
  ws_bytes = int(L.gnpde_gdc_push_workspace_bytes(n, widest, slow_groups))
  if ws_bytes == 0:
    raise _lib.GnpdeError('gdc_push: slow_groups = %d outside 1 .. 1024' % slow_groups)
  ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
  stream = stream_of(ws)
  i64 = dict(dtype=torch.int64, device=dev)
  common = (alpha, eps, int(capacity), slow_groups)
  info = torch.zeros(2, **i64)
  offsets = torch.zeros(n + 1, **i64)
  for s0, ns in batches:
    check(L.gnpde_gdc_push_count(graph.ref(), s0, ns, *common, ptr(offsets[1 + s0:]), ptr(info), ptr(ws), ws.numel(), stream))
  torch.cumsum(offsets[1:].clone(), 0, out=offsets[1:])
  total, n_slow, status = torch.cat([offsets[-1:], info]).tolist()          # the host read of the output size
  _push_status(status)
  out_ei = torch.empty(2, total, **i64)
  out_p = torch.empty(total, dtype=torch.float32, device=dev)
  info_fill = torch.zeros(2, **i64)
  if total:
    for s0, ns in batches:
      check(L.gnpde_gdc_push_fill(graph.ref(), s0, ns, *common, ptr(offsets[s0:]), ptr(out_ei), total, ptr(out_p), ptr(info_fill),
                                  ptr(ws), ws.numel(), stream))
  resid = None
  if return_residuals:
    resid = torch.empty(n, n, dtype=torch.float32, device=dev)
    for s0, ns in batches:
      check(L.gnpde_gdc_push_residuals(graph.ref(), s0, ns, *common, ptr(resid[s0:]), ptr(info_fill), ptr(ws), ws.numel(), stream))
  if total or return_residuals:
    _push_status(int(info_fill[1].item()))       # a source the fill pass refused would leave its output unwritten
  src, dst, w = out_ei[0], out_ei[1], out_p
  if normalization_in == 'sym':
    root = deg.double().sqrt()
    inv = torch.where(deg > 0, 1.0 / root.clamp(min=1.0), torch.zeros_like(root))
    w = (root[src] * w.double() * inv[dst]).float()
  elif normalization_in == 'col':
    order = torch.sort(dst * n + src).indices                   # (row, col) pairs are unique
    out_ei, w = torch.stack([dst[order], src[order]]), w[order].contiguous()
  if return_info:
    return out_ei, w, dict(slow_sources=int(n_slow), residuals=resid)
  return out_ei, w


def gdc_sparse_threshold(edge_index, w, n, *, eps=None, avg_degree=None, normalization_out='col', return_eps=False):
  """torch_geometric's sparsify_sparse + output transition_matrix on a sparse list sorted by (row, col) (gdc_push's): keep the
  entries >= eps, or with avg_degree the entries >= the mean of the (avg_degree n)-th and (avg_degree n + 1)-th largest values
  (every entry when there are no more than avg_degree n; a streaming radix select, nothing is sorted); then the output
  normalisation over the kept entries with fixed-order sums.  The order is kept.  return_eps: the threshold used (a float, None
  when every entry is kept) is returned as a third value."""
  if (eps is None) == (avg_degree is None):
    raise ValueError('gdc_sparse_threshold: give exactly one of eps and avg_degree')
  if normalization_out not in ('sym', 'col', 'row', None):
    raise ValueError('gdc_sparse_threshold: normalization_out %r is not sym, col, row or None' % (normalization_out,))
  if eps is not None and not float(eps) > 0.0:
    raise ValueError('gdc_sparse_threshold: eps = %r is not positive' % (eps,))
  require_hip(edge_index, w)
  n = int(n)
  w = f32c(w, 'values')
  thr = None
  if eps is not None:
    thr = torch.full((1,), float(eps), dtype=torch.float32, device=w.device)
  else:
    keep = int(avg_degree) * n
    if keep < 1:
      raise ValueError('gdc_sparse_threshold: avg_degree = %r is not positive' % (avg_degree,))
    if w.numel() > keep:
      thr = _avg_degree_eps(lambda: (w,), w.numel(), keep, w.device).reshape(1)
  if thr is not None and w.numel():
    pos = torch.arange(w.numel(), dtype=torch.int64, device=w.device)
    kept = select_edges(torch.stack([pos, pos]), w, thr)[0]
    edge_index, w = edge_index[:, kept].contiguous(), w[kept].contiguous()
  if normalization_out is not None and w.numel():
    w = _gdc_normalise(edge_index[0], edge_index[1], w, n, normalization_out)
  if return_eps:
    return edge_index, w, (None if thr is None else float(thr.item()))
  return edge_index, w


def edge_attention_bwd_heads(graph, att, datt_edge, post=0):
  """ds [E,h] (CSR order) from a per-head gradient in edge order (gnpde_edge_attention_bwd_heads); post: 0 raw-score gradient,
  1 times the score (exp kernels), 2 times LeakyReLU' (GAT)."""
  require_hip(datt_edge)
  datt_edge = f32c(datt_edge, 'attention gradient')
  L = _lib.lib()
  ds = torch.empty(max(graph.e, 1), att.heads, dtype=torch.float32, device=datt_edge.device)
  ws = graph.workspace('att_bwd', L.gnpde_attention_bwd_workspace_bytes(graph.ref(), ctypes.byref(att)))
  check(L.gnpde_edge_attention_bwd_heads(graph.ref(), ctypes.byref(att), ptr(datt_edge), int(post), ptr(ds), ptr(ws), ws.numel(),
                                         stream_of(datt_edge)))
  return ds


def lincomb(base, terms, out=None):
  """base + sum_j c_j v_j in one pass (gnpde_lincomb); terms = [(v_j, c_j), ...], all tensors contiguous float32 of
  base's shape.  `out` may be base (in-place update)."""
  require_hip(base)
  if out is None:
    out = torch.empty_like(base)
  vs = (ctypes.c_void_p * len(terms))(*[t[0].data_ptr() for t in terms])
  cs = (ctypes.c_float * len(terms))(*[float(t[1]) for t in terms])
  for v, _ in terms:
    if v.dtype != torch.float32 or not v.is_contiguous() or v.numel() != base.numel():
      raise _lib.GnpdeError('lincomb: operands must be contiguous float32 tensors of one size')
  if base.dtype != torch.float32 or not base.is_contiguous() or not out.is_contiguous():
    raise _lib.GnpdeError('lincomb: operands must be contiguous float32 tensors of one size')
  check(_lib.lib().gnpde_lincomb(ptr(base), vs, cs, len(terms), base.numel(), ptr(out), stream_of(base)))
  return out


def tall_skinny_gram(a, b, slabs=512):
  """a^T b for a [N, m], b [N, d] with N >> m, d  (weight gradients [A, N] x [N, d]).  The vendor GEMM gives such a
  product one workgroup per 16 x 32 output tile -- a handful of CUs streaming all of N (0.3 ms at the ogbn-arxiv
  shape, measured); as a batched product over row slabs it fills the chip, and the slab sum is a fixed-order
  reduction."""
  n = a.shape[0]
  rows = n // slabs
  if rows < 64:
    return a.t().mm(b)
  main = rows * slabs
  out = torch.bmm(a[:main].view(slabs, rows, a.shape[1]).transpose(1, 2), b[:main].view(slabs, rows, b.shape[1])).sum(dim=0)
  if main < n:
    out = out + a[main:].t().mm(b[main:])
  return out


NMF_MAX_COMPONENTS = 256
NMF_X_NONFINITE, NMF_X_NEGATIVE, NMF_INIT_NONFINITE, NMF_INIT_NEGATIVE, NMF_INDEX_RANGE = 1, 2, 4, 8, 16
NMF_FLAGS = ((NMF_X_NONFINITE, 'X has a non-finite entry'), (NMF_X_NEGATIVE, 'X has a negative entry'),
             (NMF_INIT_NONFINITE, 'the initial W or H has a non-finite entry'), (NMF_INIT_NEGATIVE, 'the initial W or H has a negative entry'),
             (NMF_INDEX_RANGE, 'an edge index lies outside [0, n)'))


def _nmf_rows(t, name):
  """A float32 device matrix with unit column stride (its rows may be padded), as the sweep takes it."""
  if not isinstance(t, torch.Tensor) or t.dim() != 2:
    raise _lib.GnpdeError('nmf: %s must be a 2-d tensor' % name)
  if not t.is_cuda:
    raise _lib.GnpdeError('nmf: %s is a %s tensor; the factorisation runs only on a HIP device, there is no CPU fallback' % (name, t.device.type))
  if t.dtype != torch.float32:
    raise _lib.GnpdeError('nmf: %s must be float32 (got %s)' % (name, t.dtype))
  if t.shape[1] > 1 and t.stride(1) != 1:
    raise _lib.GnpdeError('nmf: %s must have unit column stride (strides %s)' % (name, tuple(t.stride())))
  return t


def nmf_cd_sweep(W, G, P, workspace=None):
  """One half-sweep of sklearn's coordinate-descent NMF (gnpde_nmf_cd_sweep, include/gnpde.h has the definition): W [n, k] is updated
  in place from G [k, k] (symmetric) and P [n, k]; W and P may be column slices of wider buffers (padded rows).  Returns the
  projected-gradient violation as a 0-d float64 device tensor; nothing is read by the host."""
  W, G, P = _nmf_rows(W, 'W'), _nmf_rows(G, 'G'), _nmf_rows(P, 'P')
  n, k = W.shape
  if not 1 <= k <= NMF_MAX_COMPONENTS:
    raise _lib.GnpdeError('nmf: k = %d components outside 1 .. %d' % (k, NMF_MAX_COMPONENTS))
  if not 1 <= n <= INT32_MAX:
    raise _lib.GnpdeError('nmf: n = %d rows outside 1 .. INT32_MAX' % n)
  if tuple(G.shape) != (k, k) or tuple(P.shape) != (n, k) or G.device != W.device or P.device != W.device:
    raise _lib.GnpdeError('nmf: W is %s but G is %s and P is %s (want [k, k] and [n, k] on one device)' % (tuple(W.shape), tuple(G.shape), tuple(P.shape)))
  if not G.is_contiguous():
    G = G.contiguous()
  L = _lib.lib()
  need = int(L.gnpde_nmf_cd_sweep_workspace_bytes(n))
  if workspace is None or workspace.numel() < need:
    workspace = torch.empty(need, dtype=torch.uint8, device=W.device)
  out = torch.empty((), dtype=torch.float64, device=W.device)
  check(L.gnpde_nmf_cd_sweep(ptr(W), W.stride(0) if n > 1 else k, ptr(G), ptr(P), P.stride(0) if n > 1 else k, n, k, ptr(out), ptr(workspace),
                             workspace.numel(), stream_of(W)))
  return out


def _nmf_operand(X):
  """(n, m, X H^T product, X^T W product, sum of entries, sum of squares (double), flag bits) of a dense matrix or a sparse triple."""
  if isinstance(X, torch.Tensor):
    X = _nmf_rows(X, 'X')
    if not X.is_contiguous():
      X = X.contiguous()
    n, m = X.shape
    Xt = X.t()
    bad = (~torch.isfinite(X)).any().to(torch.int32) * NMF_X_NONFINITE + (X < 0).any().to(torch.int32) * NMF_X_NEGATIVE
    return n, m, (lambda Ht: X.mm(Ht)), (lambda W: Xt.mm(W)), X.sum(dtype=torch.float64), (X.double() ** 2).sum(), bad
  if not (isinstance(X, (tuple, list)) and len(X) == 3):
    raise _lib.GnpdeError('nmf: X is a dense float32 [n, m] tensor or (edge_index, weight, (n, m))')
  from .graph import CSRGraph
  edge_index, w, shape = X
  ei = _edge_list(edge_index, 'nmf: edge_index')
  n, m = int(shape[0]), int(shape[1])
  if n != m:
    raise _lib.GnpdeError('nmf: a sparse X must be square (got %d x %d): its products run on the aggregation kernel' % (n, m))
  if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.numel() != ei.shape[1]:
    raise _lib.GnpdeError('nmf: weight must be a vector with one value per edge')
  require_hip(w)
  w = f32c(w.detach(), 'nmf: weight')
  bad = (~torch.isfinite(w)).any().to(torch.int32) * NMF_X_NONFINITE + (w < 0).any().to(torch.int32) * NMF_X_NEGATIVE
  if ei.numel():
    bad = bad + ((ei < 0) | (ei >= n)).any().to(torch.int32) * NMF_INDEX_RANGE
    ei = ei.clamp(0, n - 1)
  # one entry per (row, col), sorted by (row, col) as ops.gdc returns them
  key, inverse = torch.unique(ei[0] * n + ei[1], return_inverse=True)
  if key.numel() != w.numel():
    raise _lib.GnpdeError('nmf: the sparse X repeats %d (row, col) pairs; coalesce it first' % (w.numel() - key.numel()))
  if w.numel():
    w = torch.empty_like(w).index_copy_(0, inverse, w)
  ei = torch.stack([torch.div(key, n, rounding_mode='floor'), key % n])
  graph = CSRGraph(ei, n, ei.device)
  graph_t, t_from_csr = graph.transposed_positions()
  w_csr = w[graph.perm_long].contiguous() if w.numel() else w
  w_t = w_csr[t_from_csr.long()[:graph.e]].contiguous() if w.numel() else w
  return n, m, (lambda Ht: spmm(graph, w_csr, Ht)), (lambda W: spmm(graph_t, w_t, W)), w.sum(dtype=torch.float64), (w.double() ** 2).sum(), bad


def nmf_iteration(x_ht, xt_w, W, Ht, workspace=None):
  """One iteration in place on W [n, k] and Ht [m, k]: the W half-sweep with G = H H^T, P = x_ht(Ht), then the H half-sweep with
  G = W^T W, P = xt_w(W); returns the summed violation (0-d float64 device tensor).  x_ht, xt_w: the two products with X."""
  v = nmf_cd_sweep(W, tall_skinny_gram(Ht, Ht), x_ht(Ht), workspace)
  return v + nmf_cd_sweep(Ht, tall_skinny_gram(W, W), xt_w(W), workspace)


def nmf(X, n_components, *, W=None, H=None, max_iter=200, tol=1e-4, seed=0, check_every=1):
  """X ~ W H with W [n, k], H [k, m] >= 0: sklearn.decomposition.NMF(solver='cd', beta_loss='frobenius', shuffle=False) without
  regularisation (include/gnpde.h has the definition).  X: a dense float32 [n, m] device tensor, or (edge_index [2, E] int64, weight
  [E], (n, n)) -- a square sparse matrix, every (row, col) pair once.  X H^T and X^T W run on the aggregation kernel (`spmm`;
  torch.mm for a dense X), the k x k Grams through `tall_skinny_gram`, the updates in `nmf_cd_sweep`.
  W and H together: the initial factors (sklearn's init='custom'); neither: avg |N(0, 1)| with avg = sqrt(mean(X) / k) from a
  torch.Generator on the device seeded with `seed` (sklearn's init='random' on another generator).
  The fit stops after iteration `it` when violation_it / violation_1 <= tol, or at once when violation_1 == 0; the host reads the
  two violations once per `check_every` iterations and nothing else.  Returns (W, H, n_iter, reconstruction_err):
  reconstruction_err = sqrt(max(0, |X|^2 - 2 <W, X H^T> + <W^T W, H H^T>)) as a 0-d float64 device tensor, summed in double.
  Refused: a CPU tensor, negative or non-finite entries in X, W or H, more than 256 components."""
  k = int(n_components)
  if not 1 <= k <= NMF_MAX_COMPONENTS:
    raise _lib.GnpdeError('nmf: n_components = %d outside 1 .. %d' % (k, NMF_MAX_COMPONENTS))
  max_iter, check_every = int(max_iter), int(check_every)
  if max_iter < 1 or check_every < 1:
    raise _lib.GnpdeError('nmf: max_iter = %d and check_every = %d must be positive' % (max_iter, check_every))
  if (W is None) != (H is None):
    raise _lib.GnpdeError('nmf: give both W and H (a custom init) or neither (the random init)')
  n, m, x_ht, xt_w, x_sum, x_sq, bad = _nmf_operand(X)
  dev = bad.device
  if W is None:
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    avg = torch.sqrt(x_sum / (float(n) * float(m) * k)).to(torch.float32)
    Ht = (avg * torch.randn(k, m, generator=gen, dtype=torch.float32, device=dev).abs()).t().contiguous()
    W = avg * torch.randn(n, k, generator=gen, dtype=torch.float32, device=dev).abs()
  else:
    W, H = _nmf_rows(W, 'W'), _nmf_rows(H, 'H')
    if tuple(W.shape) != (n, k) or tuple(H.shape) != (k, m) or W.device != dev or H.device != dev:
      raise _lib.GnpdeError('nmf: the initial W is %s and H is %s; want [%d, %d] and [%d, %d] on %s' % (tuple(W.shape), tuple(H.shape), n, k, k, m, dev))
    bad = bad + ((~torch.isfinite(W)).any() | (~torch.isfinite(H)).any()).to(torch.int32) * NMF_INIT_NONFINITE
    bad = bad + ((W < 0).any() | (H < 0).any()).to(torch.int32) * NMF_INIT_NEGATIVE
    W, Ht = W.detach().clone().contiguous(), H.detach().t().contiguous()
  _raise_flags(bad, 'nmf', NMF_FLAGS)
  L = _lib.lib()
  ws = torch.empty(int(L.gnpde_nmf_cd_sweep_workspace_bytes(max(n, m))), dtype=torch.uint8, device=dev)
  first = None
  n_iter = max_iter
  for it in range(1, max_iter + 1):
    v = nmf_iteration(x_ht, xt_w, W, Ht, ws)
    if it == 1:
      first = v
    if it % check_every == 0 or it == 1:
      v_now, v_first = torch.stack([v, first]).tolist()
      if v_first == 0.0 or v_now / v_first <= tol:
        n_iter = it
        break
  Wd, Hd = W.double(), Ht.double()
  err2 = x_sq - 2.0 * (Wd * x_ht(Ht).double()).sum() + (Wd.t().mm(Wd) * Hd.t().mm(Hd)).sum()
  return W, Ht.t().contiguous(), n_iter, torch.sqrt(torch.clamp(err2, min=0.0))


def head_spmm(graph, ds_csr, feat, heads, dk, scale, by_column, out=None):
  """Head-wise weighted segment sum (gnpde_head_spmm): [N, heads*dk] (optionally into a column slice `out`)."""
  require_hip(ds_csr, feat)
  if feat.stride(1) != 1:
    feat = feat.contiguous()
  if out is None:
    out = torch.empty(graph.n, heads * dk, dtype=torch.float32, device=feat.device)
  elif out.stride(1) != 1 or out.shape != (graph.n, heads * dk):
    raise _lib.GnpdeError('head_spmm: out must be [n, heads*dk] with unit column stride')
  check(_lib.lib().gnpde_head_spmm(graph.ref(), int(bool(by_column)), ptr(ds_csr), heads, dk, ptr(feat), feat.stride(0),
                                   float(scale), ptr(out), out.stride(0), stream_of(feat)))
  return out


def attention_struct(att_type, heads, att_dim, norm_idx, square_plus, q=None, k=None, ldqk=0, leaky_slope=0.2,
                     gat_a=None, output_var=None, lengthscale=None, edge_w_csr=None, transposed=None):
  a = _lib.AttentionStruct()
  a.type, a.heads, a.att_dim = int(att_type), int(heads), int(att_dim)
  a.norm_idx, a.square_plus, a.leaky_slope = int(norm_idx), int(bool(square_plus)), float(leaky_slope)
  a.q = q.data_ptr() if q is not None else None
  a.k = k.data_ptr() if k is not None else None
  a.ldqk = int(ldqk)
  for name, t in (('gat_a', gat_a), ('output_var', output_var), ('lengthscale', lengthscale),
                  ('edge_w_csr', edge_w_csr)):
    setattr(a, name, t.data_ptr() if t is not None else None)
  # the struct only holds raw addresses: keep the tensors alive as long as the struct (a temporary passed by
  # the caller would otherwise be freed, and its memory reused, before the kernels read it)
  a._keepalive = (q, k, gat_a, output_var, lengthscale, edge_w_csr, transposed)
  if transposed is not None:      # (graph_t, t_from_csr) of graph.CSRGraph.transposed_positions(): the column normaliser as a fused row pass
    gt, t_from_csr = transposed
    a.graph_t = ctypes.pointer(gt.struct)
    a.t_from_csr = t_from_csr.data_ptr()
  return a


def attention_plan(graph, att, want_w_mean=True, want_att=False, want_prods=False, ws_addr=256, fork=False, defer=False, hubs_only=False,
                   stats_only=False, pass_=0):
  """The launches a row attention with these operands takes (gnpde_attention_plan -> _lib.AttentionLaunchStruct): route, template line
  of the row kernels, sweeps, grids, hub handling.  att is an attention_struct whose addresses are read for their alignment (and for
  being null) only; graph (and the struct's graph_t) may live on the host.  Nothing is launched and no device is needed; a call the
  launch would refuse raises."""
  plan = _lib.AttentionLaunchStruct()
  flags = (_lib.ATT_PLAN_W_MEAN * bool(want_w_mean) | _lib.ATT_PLAN_ATT_EDGE * bool(want_att) | _lib.ATT_PLAN_PRODS_EDGE * bool(want_prods) |
           _lib.ATT_PLAN_FORK * bool(fork) | _lib.ATT_PLAN_DEFER * bool(defer) | _lib.ATT_PLAN_HUBS_ONLY * bool(hubs_only) |
           _lib.ATT_PLAN_STATS_ONLY * bool(stats_only))
  check(_lib.lib().gnpde_attention_plan(graph.ref(), ctypes.byref(att), flags, int(pass_), int(ws_addr), ctypes.byref(plan)))
  return plan


def edge_attention(graph, att, want_w_mean=True, want_att=False, want_prods=False, like=None):
  """Run the three attention passes.  Returns (w_mean_csr [e] | None, att [E,h] | None, prods [E,h] | None),
  the [E,h] tensors in the caller's edge order."""
  dev = like.device
  L = _lib.lib()
  ws = graph.workspace('att', L.gnpde_attention_workspace_bytes(graph.ref(), ctypes.byref(att)))
  w = torch.empty(max(graph.e, 1), dtype=torch.float32, device=dev) if want_w_mean else None
  a_out = torch.empty(graph.e, att.heads, dtype=torch.float32, device=dev) if want_att else None
  p_out = torch.empty(graph.e, att.heads, dtype=torch.float32, device=dev) if want_prods else None
  check(L.gnpde_edge_attention(graph.ref(), ctypes.byref(att), ptr(w), ptr(a_out), ptr(p_out), ptr(ws), ws.numel(),
                               stream_of(like)))
  return w, a_out, p_out


def attn_rhs_fused(graph, att, proj_w, proj_b, u, alpha, beta=None, x0=None, alpha_sigmoid=True, out=None, **stage_kw):
  """One-pass GRAND-nl evaluation (gnpde_attn_rhs_fused); same epilogue / stage arguments as spmm_rhs."""
  require_hip(u, proj_w, proj_b, x0)
  u = f32c(u, 'u')
  n, d = u.shape
  alpha_d = _scalar_dev(alpha, u)
  beta_d = _scalar_dev(beta, u) if x0 is not None else None
  x0c = f32c(x0, 'x0') if x0 is not None else None
  if 'stage' not in stage_kw:
    if out is None:
      out = torch.empty_like(u)
    stage_kw = dict(stage=_lib.STAGE_RHS, out_k=out)
  epi = make_epilogue(alpha_d, beta_d, x0c, alpha_sigmoid, **stage_kw)
  L = _lib.lib()
  ws = graph.workspace('fused%d_%d' % (d, att.heads), L.gnpde_attn_rhs_fused_workspace_bytes(graph.ref(), d, att.heads))
  check(L.gnpde_attn_rhs_fused(graph.ref(), ctypes.byref(att), ptr(proj_w), ptr(proj_b), ptr(u), d, u.stride(0),
                               ctypes.byref(epi), ptr(ws), ws.numel(), stream_of(u)))
  return out


def tune(key, value):
  """Kernel-variant knob for A/B measurements (gnpde_tune)."""
  check(_lib.lib().gnpde_tune(int(key), int(value)))


def agg_fold_launch(keep):
  """1: the row-pair aggregation keeps the fold launch for its hub rows where it would fold them inside its own launch (A/B and bit
  reference, gnpde_agg_fold_launch); 0: the default."""
  check(_lib.lib().gnpde_agg_fold_launch(int(keep)))


class RhsDescriptor(object):
  """Python owner of a gnpde_rhs_t: keeps every tensor the descriptor points to alive."""

  def __init__(self, kind, graph, d, ld, alpha, beta, x0, alpha_sigmoid, w_csr=None, proj_w=None, proj_b=None,
               att=None, n_state_rows=0, proj_rows=None, padded_rows=False, out_w=None):
    self.graph = graph
    self.keep = [alpha, beta, x0, w_csr, proj_w, proj_b, out_w]
    r = _lib.RhsStruct()
    r.kind = int(kind)
    r.graph = ctypes.pointer(graph.struct)
    r.d, r.ld = int(d), int(ld)
    r.n_state_rows = int(n_state_rows)
    r.flags = _lib.RHS_PADDED_ROWS if padded_rows else 0
    if proj_rows is not None:
      r.proj_row_begin, r.proj_row_end = int(proj_rows[0]), int(proj_rows[1])
    r.alpha = alpha.data_ptr()
    r.beta = beta.data_ptr() if beta is not None else None
    r.x0 = x0.data_ptr() if x0 is not None else None
    r.alpha_sigmoid = int(alpha_sigmoid)
    r.w_csr = w_csr.data_ptr() if w_csr is not None else None
    r.proj_w = proj_w.data_ptr() if proj_w is not None else None
    r.proj_b = proj_b.data_ptr() if proj_b is not None else None
    r.proj_m = int(proj_w.shape[0]) if proj_w is not None else 0
    if att is not None:
      r.att = att
    if out_w is not None:      # the GAT function's mix_features form: Wout transposed, [d, A] (GNPDE_RHS_MIX_FEATURES)
      r.flags |= _lib.RHS_MIX_FEATURES
      r.out_w = out_w.data_ptr()
      r.out_ld = int(out_w.stride(0))
    self.struct = r

  def ref(self):
    return ctypes.byref(self.struct)


def rhs_eval(desc, u, out=None):
  """One evaluation f(u) of a descriptor (gnpde_rhs_eval)."""
  require_hip(u)
  padded = bool(desc.struct.flags & _lib.RHS_PADDED_ROWS)
  u = _lib.f32rows(u, 'u') if padded else f32c(u, 'u')
  if u.stride(0) != desc.struct.ld:
    raise _lib.GnpdeError('rhs_eval: the state has row stride %d but the descriptor was built for %d' % (u.stride(0), desc.struct.ld))
  if out is None:
    # every operand of a descriptor shares ONE row stride: a padded view [n, ld][:, :d] needs a padded result buffer
    # (torch.empty_like would hand back a dense [n, d] one and the kernel would write past its end)
    out = _lib.alloc_state(u.shape[0], u.shape[1], u.device) if padded and _lib.is_padded(u) else torch.empty_like(u)
  elif out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.stride(0) != desc.struct.ld or out.shape != u.shape:
    raise _lib.GnpdeError('rhs_eval: out must be float32 %s with the descriptor\'s row stride %d' % (tuple(u.shape), desc.struct.ld))
  L = _lib.lib()
  ws = desc.graph.workspace('rhs%d_%d' % (desc.struct.kind, desc.struct.d), L.gnpde_rhs_workspace_bytes(desc.ref()))
  check(L.gnpde_rhs_eval(desc.ref(), ptr(u), ptr(out), ptr(ws), ws.numel(), stream_of(u)))
  return out


class _NativeSolver(object):
  """A native solver handle and the name of the entry point that destroys it."""
  _destroy = None

  def close(self):
    if getattr(self, 'handle', None) is not None and self.handle.value:
      try:
        getattr(_lib.lib(), self._destroy)(self.handle)
      except Exception:
        pass
      self.handle = None

  def __del__(self):
    self.close()


def _stats(fn, handle):
  """The counters of a device-controlled solve's last run (gnpde_*_stats)."""
  v = [ctypes.c_int32(0) for _ in range(5)]
  check(fn(handle, *[ctypes.byref(x) for x in v]))
  return dict(zip(('evals', 'accepted', 'rejected', 'launches', 'syncs'), [x.value for x in v]))


class Dopri5Solver(_NativeSolver):
  """gnpde_dopri5_t: dopri5 with the step-size controller on the device; one trial step = one hipGraph replay, the host reads
  the controller record once per `trials_per_sync` trial steps."""
  _destroy = 'gnpde_dopri5_destroy'

  def __init__(self, desc, rtol, atol, device):
    self.desc = desc
    L = _lib.lib()
    nbytes = L.gnpde_dopri5_workspace_bytes(desc.ref())
    self.ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    handle = ctypes.c_void_p()
    check(L.gnpde_dopri5_create(ctypes.byref(handle), desc.ref(), float(rtol), float(atol), ptr(self.ws), self.ws.numel()))
    self.handle = handle

  def run(self, y0, t0, t1, out, trials_per_sync=1, max_evals=0):
    """Integrate from y0 at t0 to t1 into `out`; False if it stopped because more than max_evals evaluations were spent."""
    require_hip(y0, out)
    y0, out_ = _lib.f32rows(y0, 'y0'), out
    if out_.dtype != torch.float32 or out_.dim() != 2 or out_.stride(1) != 1 or out_.shape != y0.shape:
      raise _lib.GnpdeError('dopri5 output must be float32 [n, d] with unit column stride')
    fin = ctypes.c_int32(0)
    check(_lib.lib().gnpde_dopri5_run(self.handle, ptr(y0), y0.stride(0), float(t0), float(t1), ptr(out_), out_.stride(0),
                                      int(trials_per_sync), int(max_evals), ctypes.byref(fin), stream_of(y0)))
    return bool(fin.value)

  def set_early_stop(self, evaluator, max_trial_steps=None):
    """Evaluate `evaluator` (EarlyStopEvaluator or None) after the trial steps, inside the captured trial-step graph, gated by
    the device controller, and stop after `max_trial_steps` trial steps (gnpde_dopri5_set_early_stop).  `self.times` then
    holds the time of every accepted step (index = step tag; [0] = t0) after a run."""
    L = _lib.lib()
    if evaluator is None:
      check(L.gnpde_dopri5_set_early_stop(self.handle, None, None, None, 0, None, 0, 0))
      self.evaluator, self.times = None, None
      return
    cap = int(max_trial_steps) + 2
    self.times = torch.zeros(cap, dtype=torch.float64, device=evaluator.state.device)
    check(L.gnpde_dopri5_set_early_stop(self.handle, evaluator.ref(), ptr(evaluator.state),
                                        ptr(evaluator.trace) if evaluator.trace_capacity else None, evaluator.trace_capacity,
                                        ptr(self.times), cap, int(max_trial_steps)))
    self.evaluator, self.max_trial_steps = evaluator, int(max_trial_steps)

  def set_pair(self, name):
    """The embedded pair of the following runs: 'dopri5' or 'adaptive_heun' (gnpde_dopri5_set_pair)."""
    check(_lib.lib().gnpde_dopri5_set_pair(self.handle, {'adaptive_heun': 0, 'dopri5': 1}[name]))
    self.pair = name

  def set_row_order(self, order32):
    """Fold a node relabelling into the solve's copies: solver row r <-> caller's row order32[r] (int32 device tensor or None)."""
    check(_lib.lib().gnpde_dopri5_set_row_order(self.handle, ptr(order32)))
    self._row_order = order32          # (kept alive: the solver holds the address)

  def set_outputs(self, times, out=None):
    """Outputs at several times (gnpde_dopri5_set_outputs).  times: the output times behind t0, strictly ascending, the last one the t1
    of the following runs; out: float32 [len(times), n, d], unit column stride, dense slabs -- the accepted trial steps write
    out[j] for j < len(times) - 1 (through the row order if one is set), the last output is `run`'s.  times None / empty detaches.
    The same `out` with other times of the same count keeps the captured trial steps."""
    L = _lib.lib()
    if times is None or len(times) == 0:
      check(L.gnpde_dopri5_set_outputs(self.handle, None, 0, None, 0))
      self.out_times, self._t_out, self._outs = None, None, None
      return
    times = tuple(float(v) for v in times)
    require_hip(out)
    if (out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] != len(times) or out.stride(2) != 1
        or out.stride(0) != out.shape[1] * out.stride(1)):
      raise _lib.GnpdeError('dopri5 outputs must be float32 [len(times), n, d] with unit column stride and dense slabs')
    t_dev = getattr(self, '_t_out', None)
    host = torch.tensor(times, dtype=torch.float64)
    if t_dev is None or t_dev.numel() != len(times):
      t_dev = host.to(out.device)
    else:
      t_dev.copy_(host)
    check(L.gnpde_dopri5_set_outputs(self.handle, ptr(t_dev), len(times), ptr(out), out.stride(1)))
    self.out_times, self._t_out, self._outs = times, t_dev, out      # (kept alive: the captured trial steps hold the addresses)

  # ---- recorded solve (training without the adjoint method): gnpde_dopri5_set_tape / _tape_backward ---------------------------
  def set_tape(self, capacity_steps):
    """Record the accepted steps of the following runs (None / 0 detaches).  The tape is zero-filled device memory owned here."""
    L = _lib.lib()
    if not capacity_steps:
      check(L.gnpde_dopri5_set_tape(self.handle, None, 0, 0))
      self.tape, self.tape_capacity = None, 0
      return
    nbytes = int(L.gnpde_dopri5_tape_bytes(self.desc.ref(), int(capacity_steps)))
    if nbytes == 0:
      raise _lib.GnpdeError('recorded dopri5: %s' % L.gnpde_last_error().decode(errors='replace'))
    self.tape = None          # (the old tape is released before the new one is allocated)
    self.tape = torch.zeros(nbytes, dtype=torch.uint8, device=self.ws.device)
    check(L.gnpde_dopri5_set_tape(self.handle, ptr(self.tape), self.tape.numel(), int(capacity_steps)))
    self.tape_capacity = int(capacity_steps)
    # (a new tape invalidates every forward pass recorded on the old one: the counter only ever grows -- odeint._RecordedDopri5.backward
    # compares the stamp of its forward pass with it)
    self.tape_generation = getattr(self, 'tape_generation', 0) + 1

  def tape_steps(self):
    return int(_lib.lib().gnpde_dopri5_tape_steps(self.handle))

  def tape_record(self):
    """([h of every accepted step of the last recorded run], x = fraction of the last step at which the end time lies)."""
    n = self.tape_steps()
    hs = (ctypes.c_float * max(n, 1))()
    x = ctypes.c_float(0.0)
    check(_lib.lib().gnpde_dopri5_tape_record(self.handle, hs, n, ctypes.byref(x)))
    return [float(hs[i]) for i in range(n)], float(x.value)

  def tape_slots(self):
    """(address of buffer 0 of the record, floats between consecutive buffers): buffer 6 s + i = u_i of accepted step s."""
    slots, stride = ctypes.c_void_p(), ctypes.c_size_t(0)
    check(_lib.lib().gnpde_dopri5_tape_slots(self.handle, ctypes.byref(slots), ctypes.byref(stride)))
    return slots, int(stride.value)

  def tape_backward(self, graph_t, w_t, grad_out):
    """(dL/dy0 [n, d], r_t [e] in graph_t's CSR order, sum_g [n, ld], dot [1]) of the last recorded run; no host synchronisation."""
    require_hip(grad_out, w_t)
    L = _lib.lib()
    g = _lib.f32rows(grad_out, 'grad_out')
    n, d = g.shape
    ld = self.desc.struct.ld
    dev = g.device
    nbytes = int(L.gnpde_dopri5_tape_backward_workspace_bytes(self.handle, graph_t.ref()))
    ws = getattr(self, '_sweep_ws', None)
    if ws is None or ws.numel() < nbytes:
      self._sweep_ws = None
      ws = self._sweep_ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    gy0 = torch.empty(n, d, dtype=torch.float32, device=dev)
    r_t = torch.empty(max(graph_t.e, 1), dtype=torch.float32, device=dev)
    sum_g = torch.empty(n, ld, dtype=torch.float32, device=dev)
    dot = torch.empty(1, dtype=torch.float32, device=dev)
    check(L.gnpde_dopri5_tape_backward(self.handle, graph_t.ref(), ptr(w_t), ptr(g), g.stride(0), ptr(gy0), gy0.stride(0), ptr(r_t),
                                       ptr(sum_g), ptr(dot), ptr(ws), ws.numel(), stream_of(g)))
    return gy0, r_t, sum_g[:, :d], dot

  def stats(self):
    return _stats(_lib.lib().gnpde_dopri5_stats, self.handle)


class AdjointAdaptiveSolver(_NativeSolver):
  """gnpde_adjoint_adaptive_t: one backward interval of the adjoint with an adaptive adjoint method ('adaptive_heun' / 'dopri5') on the
  Laplacian function, the controller on the device (one hipGraph replay per trial step)."""
  _destroy = 'gnpde_adjoint_adaptive_destroy'

  def __init__(self, desc, graph_t, w_t, method, rtol, atol, device):
    self.desc, self.graph_t, self.w_t = desc, graph_t, w_t
    self.method = {'adaptive_heun': _lib.ADAPTIVE_HEUN, 'dopri5': _lib.ADAPTIVE_DOPRI5}[method]
    L = _lib.lib()
    nbytes = int(L.gnpde_adjoint_adaptive_workspace_bytes(desc.ref(), graph_t.ref(), self.method))
    if nbytes == 0:
      raise _lib.GnpdeError('adaptive adjoint: %s' % L.gnpde_last_error().decode(errors='replace'))
    self.ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    handle = ctypes.c_void_p()
    check(L.gnpde_adjoint_adaptive_create(ctypes.byref(handle), desc.ref(), graph_t.ref(), ptr(w_t), self.method, float(rtol), float(atol),
                                          ptr(self.ws), self.ws.numel()))
    self.handle = handle

  def run(self, y, a, g, s0, s1, dt0, trials_per_sync=8, max_evals=0):
    """a (in: dL/dy at the later time) and g (device float32[2]: accumulated g_alpha, g_beta) are updated in place; False if it
    stopped because more than max_evals evaluations were spent."""
    require_hip(y, a, g)
    y, a = _lib.f32rows(y, 'y'), _lib.f32rows(a, 'a')
    fin = ctypes.c_int32(0)
    check(_lib.lib().gnpde_adjoint_adaptive_run(self.handle, ptr(y), y.stride(0), ptr(a), a.stride(0), ptr(g), float(s0), float(s1), float(dt0),
                                                int(trials_per_sync), int(max_evals), ctypes.byref(fin), stream_of(y)))
    return bool(fin.value)

  def stats(self):
    return _stats(_lib.lib().gnpde_adjoint_adaptive_stats, self.handle)


def rhs_stage(desc, u, stage, ws=None, **kw):
  """f(u) of a descriptor with an explicit stage epilogue (gnpde_rhs_stage); alpha / beta / x0 come from
  the descriptor."""
  e = _lib.EpilogueStruct()
  e.stage = int(stage)
  e.dt = float(kw.get('dt', 0.0))
  for name in ('y', 'k1', 'k2', 'k3', 'out_k', 'out_y'):
    t = kw.get(name)
    setattr(e, name, t.data_ptr() if t is not None else None)
  prev, coef = kw.get('prev', ()), kw.get('coef', ())
  e.n_prev = len(prev)
  for j, t in enumerate(prev):
    e.prev[j] = t.data_ptr()
  for j, c in enumerate(coef):
    e.coef[j] = float(c)
  L = _lib.lib()
  if ws is None:
    ws = desc.graph.workspace('rhs%d_%d' % (desc.struct.kind, desc.struct.d), L.gnpde_rhs_workspace_bytes(desc.ref()))
  check(L.gnpde_rhs_stage(desc.ref(), ptr(u), ctypes.byref(e), ptr(ws), ws.numel(), stream_of(u)))


def rk_error_ratio(y0, y1, ks, coefs, atol, rtol, out, ws):
  """Device-side error ratio of an embedded RK step (gnpde_rk_error_ratio); `out` is a 1-element tensor."""
  n, d = y0.shape
  karr = (ctypes.c_void_p * len(ks))(*[k.data_ptr() for k in ks])
  carr = (ctypes.c_float * len(ks))(*[float(c) for c in coefs])
  check(_lib.lib().gnpde_rk_error_ratio(ptr(y0), ptr(y1), karr, carr, len(ks), float(atol), float(rtol), n, d,
                                        y0.stride(0), ptr(out), ptr(ws), stream_of(y0)))
  return out


def dopri5_interp(y0, y1, ks, mid_coefs, h, x, out):
  """Quartic end-point interpolation of an accepted dopri5 step in one pass (gnpde_dopri5_interp)."""
  n, d = y0.shape
  karr = (ctypes.c_void_p * len(ks))(*[k.data_ptr() for k in ks])
  carr = (ctypes.c_float * len(ks))(*[float(c) for c in mid_coefs])
  check(_lib.lib().gnpde_dopri5_interp(ptr(y0), ptr(y1), karr, carr, float(h), float(x), n, d, y0.stride(0), ptr(out),
                                       stream_of(y0)))
  return out


class EarlyStopEvaluator(object):
  """Device-side early-stopping evaluator (gnpde_decoder_t + its int32 state / trace).

  weight [C, d_dec], bias [C] or None: the decoder m2; labels [N] integer; masks: three bool [N] tensors
  (train, val, test).  After evaluations, `read()` returns python numbers (ONE device->host copy)."""

  def __init__(self, weight, bias, labels, train_mask, val_mask, test_mask, max_trace=0):
    require_hip(weight)
    dev = weight.device
    self.weight = weight.detach().to(torch.float32).contiguous()
    self.bias = None if bias is None else bias.detach().to(device=dev, dtype=torch.float32).contiguous()
    lab = labels.detach().to(dev).reshape(-1)
    self.labels = lab.to(torch.int32).contiguous()
    n = self.labels.numel()
    masks = []
    for m in (train_mask, val_mask, test_mask):
      m = m.detach().to(dev).reshape(-1)
      if m.dtype != torch.bool:
        # node-index splits: the reference's ogbn-arxiv Data carries train_mask = split_idx['train'] etc.
        # (reference src/data.py:90), which `logits[mask]` / `y[mask]` index the same way as a bool mask
        idx = m.long()
        if idx.numel() > 0 and (int(idx.min()) < 0 or int(idx.max()) >= n):
          raise _lib.GnpdeError('early stop: split index outside [0, %d)' % n)
        m = torch.zeros(n, dtype=torch.bool, device=dev)
        m[idx] = True
      elif m.numel() != n:
        raise _lib.GnpdeError('early stop: mask of %d entries for %d labels' % (m.numel(), n))
      masks.append(m)
    self.split = (masks[0].to(torch.uint8) | (masks[1].to(torch.uint8) << 1) | (masks[2].to(torch.uint8) << 2)).contiguous()
    self.sizes = [int(v) for v in torch.stack([m.sum() for m in masks]).tolist()]
    self.n = n
    self.state = torch.zeros(_lib.EARLY_STATE_INTS, dtype=torch.int32, device=dev)
    self.trace = torch.zeros((max(int(max_trace), 1), 4), dtype=torch.int32, device=dev)
    self.trace_capacity = int(max_trace)
    self.struct = _lib.DecoderStruct(weight=ptr(self.weight), bias=ptr(self.bias), labels=ptr(self.labels),
                                     split=ptr(self.split), n_classes=int(self.weight.shape[0]),
                                     d_dec=int(self.weight.shape[1]))

  def ref(self):
    return ctypes.byref(self.struct)

  def relabelled(self, view):
    """The same evaluator for states whose rows are in the order of a graph.LocalityView: labels and split masks permuted,
    decoder, best-so-far state and trace SHARED with this one (the hit counts are integers over the same nodes, so every
    accuracy is unchanged and `read()` of either returns the same record)."""
    views = self.__dict__.setdefault('_relabelled', [])
    for v, ev in views:
      if v is view:
        return ev
    ev = object.__new__(EarlyStopEvaluator)
    ev.__dict__.update({k: v for k, v in self.__dict__.items() if k != '_relabelled'})
    ev.labels = self.labels.index_select(0, view.order).contiguous()
    ev.split = self.split.index_select(0, view.order).contiguous()
    ev.struct = _lib.DecoderStruct(weight=ptr(self.weight), bias=ptr(self.bias), labels=ptr(ev.labels), split=ptr(ev.split),
                                   n_classes=int(self.weight.shape[0]), d_dec=int(self.weight.shape[1]))
    views[:] = views[-1:] + [(view, ev)]
    return ev

  def reset(self):
    check(_lib.lib().gnpde_early_stop_reset(ptr(self.state), stream_of(self.state)))

  def evaluate(self, y, step):
    """Count the hits of state y [N, d] and fold them into the best-so-far (no host synchronisation)."""
    require_hip(y)
    if y.dtype != torch.float32 or y.dim() != 2 or y.stride(1) != 1 or y.shape[0] != self.n:
      raise _lib.GnpdeError('early stop: state must be float32 [%d, d] with unit column stride' % self.n)
    check(_lib.lib().gnpde_early_stop_eval(self.ref(), ptr(y), int(y.shape[1]), int(y.stride(0)), int(y.shape[0]), int(step),
                                           ptr(self.state), ptr(self.trace) if self.trace_capacity else None,
                                           self.trace_capacity, stream_of(y)))

  def read(self):
    """{'best': (train, val, test) accuracies, 'step': tag of the best step, 'evals': count, 'trace': [[...]]}"""
    st = self.state[:8].tolist()
    acc = lambda hits: [h / s if s else float('nan') for h, s in zip(hits, self.sizes)]  # noqa: E731
    out = {'best': acc(st[3:6]), 'best_hits': st[3:6], 'step': st[6], 'evals': st[7], 'trace': None}
    if self.trace_capacity:
      rows = self.trace[:min(st[7], self.trace_capacity)].tolist()
      out['trace'] = [{'acc': acc(r[:3]), 'hits': r[:3], 'step': r[3]} for r in rows]
    return out


class FixedStepSolver(_NativeSolver):
  """gnpde_solver_t: euler / midpoint / rk4 over a fixed grid, the whole loop captured in one hipGraph."""
  _destroy = 'gnpde_solver_destroy'

  def __init__(self, desc, method, dts, device):
    self.desc = desc
    self.method = {'euler': _lib.METHOD_EULER, 'rk4': _lib.METHOD_RK4, 'midpoint': _lib.METHOD_MIDPOINT}[method]
    self.dts = [float(v) for v in dts]
    L = _lib.lib()
    nbytes = L.gnpde_solver_workspace_bytes(desc.ref(), self.method)
    self.ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    arr = (ctypes.c_float * len(self.dts))(*self.dts)
    handle = ctypes.c_void_p()
    check(L.gnpde_solver_create(ctypes.byref(handle), desc.ref(), self.method, arr, len(self.dts), ptr(self.ws),
                                self.ws.numel()))
    self.handle = handle
    self.n_rhs_evals = L.gnpde_solver_num_rhs_evals(handle)

  def set_early_stop(self, evaluator):
    """Evaluate `evaluator` (EarlyStopEvaluator or None) after every step, inside the same hipGraph."""
    L = _lib.lib()
    if evaluator is None:
      check(L.gnpde_solver_set_early_stop(self.handle, None, None, None, 0))
    else:
      check(L.gnpde_solver_set_early_stop(self.handle, evaluator.ref(), ptr(evaluator.state),
                                          ptr(evaluator.trace) if evaluator.trace_capacity else None,
                                          evaluator.trace_capacity))
    self.evaluator = evaluator

  def set_gather(self, dtype):
    """Gather operand of the aggregation in the following runs (gnpde_solver_set_gather): 'bf16' attaches a bf16 shadow per
    stage-input buffer (device memory owned here), 'fp32' detaches.  Raises for a shape out of scope and while a tape is attached."""
    L = _lib.lib()
    if dtype not in _lib.GATHER_DTYPES:
      raise ValueError("gather dtype must be 'fp32' or 'bf16' (got %r)" % (dtype,))
    if dtype == 'fp32':
      check(L.gnpde_solver_set_gather(self.handle, _lib.GATHER_FP32, None, 0))
      self.gather_mem = None
    else:
      nbytes = int(L.gnpde_solver_gather_bytes(self.desc.ref(), self.method))
      if nbytes == 0:
        raise _lib.GnpdeError('bf16 gather operand: %s' % L.gnpde_last_error().decode(errors='replace'))
      mem = torch.zeros(nbytes, dtype=torch.uint8, device=self.ws.device)
      check(L.gnpde_solver_set_gather(self.handle, _lib.GATHER_BF16, ptr(mem), mem.numel()))
      self.gather_mem = mem
    self.gather_dtype = dtype

  def set_outputs(self, plan, out=None, order32=None):
    """Outputs at several times (gnpde_solver_set_outputs).  plan: [(step, frac), ...] -- output j is taken after step `step`
    (1-based) at the fraction `frac` of it (odeint.output_plan); out: float32 [len(plan), n, d], unit column stride, dense slabs;
    order32: solver row r is written to row order32[r] of every output (int32 device tensor or None).  The scratch state buffer of
    the interior outputs is device memory owned here.  plan None / empty detaches."""
    L = _lib.lib()
    if not plan:
      check(L.gnpde_solver_set_outputs(self.handle, 0, None, None, None, 0, None))
      self.output_plan, self._outs, self._out_scratch = None, None, None
      return
    plan = tuple((int(i), float(f)) for i, f in plan)
    require_hip(out)
    if (out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] != len(plan) or out.stride(2) != 1
        or out.stride(0) != out.shape[1] * out.stride(1)):
      raise _lib.GnpdeError('solver outputs must be float32 [len(plan), n, d] with unit column stride and dense slabs')
    scratch = None
    if any(f != 1.0 for _, f in plan):
      n = self.desc.graph.n
      scratch = torch.zeros(n * self.desc.struct.ld + 64, dtype=torch.float32, device=out.device)
    steps = (ctypes.c_int32 * len(plan))(*[i for i, _ in plan])
    fracs = (ctypes.c_float * len(plan))(*[f for _, f in plan])
    check(L.gnpde_solver_set_output_order(self.handle, ptr(order32)))
    check(L.gnpde_solver_set_outputs(self.handle, len(plan), steps, fracs, ptr(out), out.stride(1), ptr(scratch)))
    self.output_plan, self._outs, self._out_scratch, self._out_order = plan, out, scratch, order32      # (kept alive: the graph holds the addresses)

  def set_tape(self, on=True):
    """Record the stage inputs of the following runs (gnpde_solver_set_tape): the tape is zero-filled device memory owned here."""
    L = _lib.lib()
    if not on:
      check(L.gnpde_solver_set_tape(self.handle, None, 0))
      self.tape = None
      return
    nbytes = int(L.gnpde_solver_tape_bytes(self.desc.ref(), self.method, len(self.dts)))
    if nbytes == 0:
      raise _lib.GnpdeError('recorded fixed-grid solve: %s' % L.gnpde_last_error().decode(errors='replace'))
    self.tape = torch.zeros(nbytes, dtype=torch.uint8, device=self.ws.device)
    check(L.gnpde_solver_set_tape(self.handle, ptr(self.tape), self.tape.numel()))
    self.tape_generation = getattr(self, 'tape_generation', 0) + 1      # (only ever grows: stale-tape stamp of odeint._RecordedFixedGrid)

  def run(self, y, use_graph=True):
    """Integrate y in place."""
    require_hip(y)
    if y.dtype != torch.float32 or y.dim() != 2 or y.stride(1) != 1 or y.stride(0) != self.desc.struct.ld:
      raise _lib.GnpdeError('solver state must be float32 [n, d] with unit column stride and the descriptor\'s row stride')
    check(_lib.lib().gnpde_solver_run(self.handle, ptr(y), int(bool(use_graph)), stream_of(y)))
    return y


class AdjointSolver(_NativeSolver):
  """gnpde_adjoint_t: the fixed-grid adjoint solve (state, adjoint and parameter gradients integrated backwards), one hipGraph."""
  _destroy = 'gnpde_adjoint_destroy'

  def __init__(self, desc, graph_t, t_from_csr, proj_wt, w_t, method, dts, device):
    self.desc, self.graph_t = desc, graph_t
    self.keep = [t_from_csr, proj_wt, w_t]
    # ('dopri5_tape': no grid -- the sweep over a recorded dopri5 solve, set_dopri5_tape before every run)
    self.method = {'euler': _lib.METHOD_EULER, 'rk4': _lib.METHOD_RK4, 'midpoint': _lib.METHOD_MIDPOINT,
                   'dopri5_tape': _lib.METHOD_DOPRI5_TAPE}[method]
    self.dts = [float(v) for v in dts]
    L = _lib.lib()
    nbytes = L.gnpde_adjoint_workspace_bytes(desc.ref(), graph_t.ref(), self.method)
    if nbytes == 0:
      raise _lib.GnpdeError('native adjoint: %s' % L.gnpde_last_error().decode(errors='replace'))
    self.ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    self.n_grad = int(L.gnpde_adjoint_grad_floats(desc.ref()))
    arr = (ctypes.c_float * len(self.dts))(*self.dts)
    handle = ctypes.c_void_p()
    check(L.gnpde_adjoint_create(ctypes.byref(handle), desc.ref(), graph_t.ref(), ptr(t_from_csr), ptr(proj_wt), ptr(w_t), self.method,
                                 arr, len(self.dts), ptr(self.ws), self.ws.numel()))
    self.handle = handle
    self.n_rhs_evals = L.gnpde_adjoint_num_rhs_evals(handle)

  def set_tape(self, tape, r_acc=None, csr_from_t=None):
    """Reverse sweep through the recorded forward solve whose stage inputs `tape` holds (FixedStepSolver.set_tape; same method and
    grid): run() then maps a = dL/dy(T) to dL/dy0.  r_acc [e] (GRAND-l): receives the weighted edge products -- in the order of the
    TRANSPOSED graph when `swapped` (the cotangent-side form of the sweep: always for GRAND-l, with `csr_from_t` for the others), else in
    CSR order.  csr_from_t [e] int32: the inverse of t_from_csr."""
    L = _lib.lib()
    if tape is None:
      check(L.gnpde_adjoint_set_tape(self.handle, None, 0, None, None))
    else:
      require_hip(tape)
      check(L.gnpde_adjoint_set_tape(self.handle, ptr(tape), tape.numel(), ptr(r_acc), ptr(csr_from_t)))
    self.tape, self.r_acc, self.csr_from_t = tape, r_acc, csr_from_t
    self.swapped = bool(L.gnpde_adjoint_tape_swapped(self.handle))

  def set_dopri5_tape(self, forward, csr_from_t=None):
    """Reverse sweep through the last recorded run of `forward` (a Dopri5Solver with a tape, GRAND-nl / GAT): run(use_graph=False)
    then maps a = dL/d(out) to dL/dy0 with one VJP stage per recorded evaluation (gnpde_adjoint_set_dopri5_tape).  The step record is
    host data the forward run already read; nothing synchronises here."""
    hs, x = forward.tape_record()
    slots, stride = forward.tape_slots()
    arr = (ctypes.c_float * max(len(hs), 1))(*hs)
    check(_lib.lib().gnpde_adjoint_set_dopri5_tape(self.handle, slots, stride, arr, len(hs), float(x), ptr(csr_from_t)))
    self.tape, self.csr_from_t = forward.tape, csr_from_t
    self.swapped = bool(_lib.lib().gnpde_adjoint_tape_swapped(self.handle))
    self.n_rhs_evals = _lib.lib().gnpde_adjoint_num_rhs_evals(self.handle)

  def run(self, y, a, grads, use_graph=True):
    """y, a [n, ld] integrated backwards in place; grads [n_grad] receives the parameter gradients."""
    require_hip(y, a, grads)
    ld = self.desc.struct.ld
    for t in (y, a):
      if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) != ld:
        raise _lib.GnpdeError('adjoint solve: state and adjoint must be float32 [n, d] with the descriptor\'s row stride')
    if grads.dtype != torch.float32 or not grads.is_contiguous() or grads.numel() < self.n_grad:
      raise _lib.GnpdeError('adjoint solve: gradient buffer of %d floats needed' % self.n_grad)
    check(_lib.lib().gnpde_adjoint_run(self.handle, ptr(y), ptr(a), ptr(grads), int(bool(use_graph)), stream_of(y)))
