"""CPU oracle of the edge-sampling rewiring (graph_rewiring.add_edges / edge_sampling, GNN_FA): pure numpy / torch restatements of
what include/gnpde.h defines -- the Philox4x32-10 streams, the uniform node draw, the fixed-point multinomial (with `exp` in
float64), the node importance (float64), the union (torch.unique) and the `>=` selection (torch.quantile + mask) -- and of the
fully-adjacent layer on top of the repository's CPU right-hand sides (oracle/restate.py).

The multinomial is compared through a `Band`, because the device forms its integer weights from fp32 arithmetic:

  device   t'_j = expf(fl(s_j - m)),  w'_j = floor(t'_j 2^32)          oracle   t_j = exp(s_j - m) in float64,  w_j = floor(t_j 2^32)

  with u = 2^-24 (fp32 unit roundoff), d_j = s_j - m <= 0 (m, the maximum of the SAME fp32 logits, is exact on both sides):
    fl(s_j - m) = d_j (1 + e1), |e1| <= u                    -> a factor exp(d_j e1), within |d_j| u (1 + o(1)) of 1
    expf is accurate to EXPF_ULPS = 2 units in the last place (the HIP math API documents 1; one more for margin), and one
      unit in the last place is at most 2 u relative           -> a factor within 2 EXPF_ULPS u of 1
    a logit that itself carries an absolute error a_j (the importance: an fp32 sum of deg_j non-negative terms and one division,
      |error| <= (deg_j + 1) u value_j) moves d_j by at most a_j + a_max    -> a factor within (a_j + a_max)(1 + o(1)) of 1
    the two truncations differ by less than 1
  so  |w'_j - w_j| <= b_j = w_j ((|d_j| + 2 EXPF_ULPS) u + a_j + a_max) SLACK + 1   (SLACK = 1.01 covers the second-order terms),
      |C'_j - C_j| <= B_j = b_0 + ... + b_j   (both are exact integer sums),
      |target' - target| <= B_n + 1           (target = floor(r C_n / 2^64), r < 2^64).
  The oracle's draw j (C_{j-1} <= target < C_j) is DETERMINED -- the device must give j -- when
      target - C_{j-1} >= B_{j-1} + B_n + 1   and   C_j - target > B_j + B_n + 1;
  otherwise the device may also answer the neighbour on the side of the boundary that is too close."""
import numpy as np
import torch

from oracle import restate as R

U32 = np.uint64(0xffffffff)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
UNIT = 2.0 ** -24
EXPF_ULPS = 2
SLACK = 1.01
CAP_SHARE = 0.01                 # share of the draws the band may leave undetermined

# Random123 known answers (kat_vectors, philox4x32 10 rounds): (counter words, key words, output words)
KNOWN_ANSWERS = (
  ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
  ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
  ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
  """counter: four uint64 arrays holding 32-bit words, key: two 32-bit words -> four arrays of output words."""
  c = [np.asarray(v, dtype=np.uint64) & U32 for v in counter]
  k0, k1 = np.uint64(key[0]) & U32, np.uint64(key[1]) & U32
  for _ in range(10):
    p0, p1 = M0 * c[0], M1 * c[2]                      # 32 x 32 -> 64 bits, no overflow
    c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & U32]
    k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
  return c


def known_answer(counter, key):
  return tuple(int(v[0]) for v in philox4x32_10([np.array([w], dtype=np.uint64) for w in counter], key))


def words(seed, stream, call, first_block, n_words):
  """The stream's words as a uint64 array (values < 2^32): word w = word (w & 3) of block first_block + (w >> 2); key = the
  seed's two words, counter = (block low, block high, stream, call)."""
  n_blocks = (int(n_words) + 3) // 4
  b = (np.arange(n_blocks, dtype=np.uint64) + np.uint64(first_block))
  seed = int(seed) & (2 ** 64 - 1)
  out = philox4x32_10([b & U32, b >> np.uint64(32), np.full(n_blocks, stream, dtype=np.uint64), np.full(n_blocks, call, dtype=np.uint64)],
                      (seed & 0xffffffff, seed >> 32))
  return np.stack(out, axis=1).reshape(-1)[:int(n_words)]


def random_nodes(n, count, seed, stream, call):
  return torch.from_numpy(((words(seed, stream, call, 0, count) * np.uint64(n)) >> np.uint64(32)).astype(np.int64))


def logit_weights(logits):
  """(w, d): the oracle's integer weights floor(exp(s - max) 2^32) (float64 exp; Python ints) and d = s - max (float64)."""
  s = np.asarray(logits, dtype=np.float32).astype(np.float64)
  d = s - s.max()
  w = np.floor(np.exp(d) * 4294967296.0)
  return [int(v) for v in w], d


def draw_targets(total, count, seed, stream, call):
  """target_i = floor(r_i total / 2^64), r_i = (word 2i << 32) | word 2i + 1."""
  w = words(seed, stream, call, 0, 2 * count)
  return [((int(w[2 * i]) << 32 | int(w[2 * i + 1])) * total) >> 64 for i in range(count)]


def cumulative(w):
  out, acc = [], 0
  for v in w:
    acc += v
    out.append(acc)
  return out


def first_above(cum, targets):
  """First j with cum[j] > target, per target (cum: ascending Python ints below 2^64)."""
  return np.searchsorted(np.array(cum, dtype=np.uint64), np.array(targets, dtype=np.uint64), side='right').astype(np.int64)


def sample_nodes(logits, count, seed, stream, call):
  w, _ = logit_weights(logits)
  cum = cumulative(w)
  return torch.from_numpy(first_above(cum, draw_targets(cum[-1], count, seed, stream, call)))


class Band(object):
  """The inclusion rule of the module docstring for `count` draws from `logits` (fp32 values; logit_err: optional absolute
  error bound per logit, float64)."""

  def __init__(self, logits, count, seed, stream, call, logit_err=None):
    w, d = logit_weights(logits)
    n = len(w)
    a = np.zeros(n) if logit_err is None else np.asarray(logit_err, dtype=np.float64)
    rel = ((np.abs(d) + 2 * EXPF_ULPS) * UNIT + a + (a.max() if n else 0.0)) * SLACK
    b = [int(np.ceil(wj * r)) + 1 for wj, r in zip(w, rel)]
    self.cum, self.bound = cumulative(w), cumulative(b)
    self.targets = draw_targets(self.cum[-1], count, seed, stream, call)
    self.draws = first_above(self.cum, self.targets)
    slack_n = self.bound[-1] + 1
    self.low_open = np.zeros(count, dtype=bool)      # the draw may also be j - 1
    self.high_open = np.zeros(count, dtype=bool)     # ... or j + 1
    for i, (t, j) in enumerate(zip(self.targets, self.draws)):
      j = int(j)
      if j > 0 and t - self.cum[j - 1] < self.bound[j - 1] + slack_n:
        self.low_open[i] = True
      if j < n - 1 and not self.cum[j] - t > self.bound[j] + slack_n:
        self.high_open[i] = True

  def undetermined(self):
    return int((self.low_open | self.high_open).sum())

  def check(self, got):
    got = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.int64)
    assert got.shape == self.draws.shape, (got.shape, self.draws.shape)
    diff = got - self.draws
    ok = (diff == 0) | ((diff == -1) & self.low_open) | ((diff == 1) & self.high_open)
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, 'draws %s: device %s, oracle %s (low open %s, high open %s)' % (
      bad[:5].tolist(), got[bad[:5]].tolist(), self.draws[bad[:5]].tolist(), self.low_open[bad[:5]].tolist(), self.high_open[bad[:5]].tolist())


# the real-valued multinomial cases of the GPU test: (n, low, high, seed of the logits); 10 000 draws each
REAL_CASES = ((65, 0.0, 1.0, 11), (1025, 0.0, 1.0, 12), (4099, 0.0, 1.0, 13), (65, -5.0, 5.0, 14), (1025, -5.0, 5.0, 15), (4099, -5.0, 5.0, 16))
REAL_DRAWS = 10000
REAL_STREAM = (2024, 0, 3)       # seed, stream, call


def real_logits(case):
  n, lo, hi, seed = REAL_CASES[case]
  g = torch.Generator().manual_seed(seed)
  return (torch.rand(n, generator=g) * (hi - lo) + lo).to(torch.float32)


def real_band(case):
  return Band(real_logits(case).numpy(), REAL_DRAWS, *REAL_STREAM)


def node_importance(edge_index, att_mean, n):
  """float64: (sum of att_mean over the edges with column j) / (their number); also the in-degrees."""
  dst = edge_index[1]
  sums = torch.zeros(n, dtype=torch.float64).scatter_add_(0, dst, att_mean.double())
  deg = torch.zeros(n, dtype=torch.float64).scatter_add_(0, dst, torch.ones(dst.numel(), dtype=torch.float64))
  return sums / deg, deg


def edge_union(a, b):
  return torch.unique(torch.cat([a, b], dim=1), dim=1)


def select_edges(edge_index, score, q):
  thr = torch.quantile(score, q)
  return edge_index[:, score >= thr], thr


def to_undirected(edge_index):
  return torch.unique(torch.cat([edge_index, edge_index.flip(0)], dim=1), dim=1)


def both_directions(a, b):
  return torch.cat([torch.stack([a, b]), torch.stack([b, a])], dim=1)


def full_adjacency(n):
  """The reference's utils.get_full_adjacency (:161-167): edge i n + j = (i, j)."""
  idx = torch.arange(n, dtype=torch.int64)
  return torch.stack([idx.repeat_interleave(n), idx.repeat(n)])


# ---- the model of the GPU tests and its restatement -----------------------------------------------------------------------------
N, FEAT, HIDDEN, CLASSES, HEADS = 96, 24, 16, 5, 4
MODEL_SEED = 7                  # seed of the data, the graph and the parameters
SAMPLING_SEED = 1237            # opt['edge_sampling_seed']: picked on the ORACLE alone so that MARGIN holds (test_edge_sampling_cpu asserts it)
ATT_TOL = 1e-5                  # tests/helpers.TOL: the parity bar of the attention and block tests (relative to the largest entry)
# the end-to-end test's first solve is euler with step 0.5: its own seeds, picked on the oracle alone like SAMPLING_SEED
E2E_FIRST_SOLVE = dict(time=2.0, step_size=0.5, method='euler')
E2E_SEEDS = {'laplacian': 1281, 'transformer': 1256}
MARGIN = 10 * ATT_TOL           # the mean attentions nearest the quantile stand clear of it by more than this, relative to the largest


def make_model(dev, cls=None, **over):
  """GNN_FA (or cls) on `dev` with data, graph and EVERY parameter drawn from one seeded generator, so that a CPU copy and a device
  copy hold the same numbers."""
  import gnpde_amd as G
  from helpers import Data, Fixture, random_graph
  opt = dict(Fixture('gnn_constant_transformer_rk4').opt)
  opt.update(hidden_dim=HIDDEN, attention_dim=16, heads=HEADS, function='laplacian', block='attention', method='rk4', step_size=1.0,
             time=2.0, input_dropout=0.5, dropout=0.5, fa_layer=True, edge_sampling_add_type='random', edge_sampling_add=0.64,
             edge_sampling_rmv=0.0, edge_sampling_sym=False, edge_sampling_space='attention', edge_sampling_seed=SAMPLING_SEED)
  opt.update(over)
  g = torch.Generator().manual_seed(MODEL_SEED)
  x = torch.randn(N, FEAT, generator=g)
  data = Data(x.to(dev), random_graph(N, 4, seed=MODEL_SEED).to(dev))
  model = (cls or G.GNN_FA)(opt, G.DummyDataset(data, CLASSES), dev).to(dev)
  with torch.no_grad():
    for name, p in model.named_parameters():
      if p.dim() >= 2:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
      elif name.endswith('.bias'):
        p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(dev))
  return model, data, opt


def _cpu(t):
  return t.detach().cpu()


def _layer(lay):
  return _cpu(lay.Q.weight), _cpu(lay.Q.bias), _cpu(lay.K.weight), _cpu(lay.K.bias)


def block_solve(model, y0, edge, method, step_size):
  """One forward of the model's AttODEblock on the edge set `edge` (CPU): x0 <- y0, attention once from y0 with the block's
  layer (laplacian function) or per evaluation with the function's own layer (transformer function)."""
  opt = model.opt
  f = model.odeblock.odefunc
  alpha, beta = _cpu(f.alpha_train), _cpu(f.beta_train)
  T = float(model.odeblock.t[1])
  if opt['function'] == 'laplacian':
    att, _ = R.transformer_attention(y0, edge, *_layer(model.odeblock.multihead_att_layer), opt['heads'])
    rhs = lambda t, y: R.rhs_laplacian(y, edge, att, alpha, beta, y0, opt['no_alpha_sigmoid'], opt['add_source'])
  else:
    qk = _layer(f.multihead_att_layer)
    rhs = lambda t, y: R.rhs_transformer(y, edge, *qk, opt['heads'], alpha, beta, y0, opt['no_alpha_sigmoid'], opt['add_source'])
  return R.odeint_fixed(rhs, y0, T, step_size, method)


def mean_attention(model, z, edge):
  """Head-mean attention of the block's layer at state z on `edge` (what edge_sampling thresholds)."""
  att, _ = R.transformer_attention(z, edge, *_layer(model.odeblock.multihead_att_layer), model.opt['heads'])
  return att.mean(dim=1)


def restated_forward(model, x, first_edge, added_edge):
  """The eval-mode forward of GNN_FA restated on the CPU.  first_edge: the edge set of the first solve; added_edge: what add_edges
  returned (given, so that the restatement does not depend on the random stream).  Returns a dict: z (after the first solve),
  mean_att / threshold / kept (when edge_sampling_rmv != 0), edge (the edge set of the second solve), out."""
  opt = model.opt
  x, first_edge, added_edge = _cpu(x), _cpu(first_edge), _cpu(added_edge)
  res = {}
  h = torch.nn.functional.linear(x, _cpu(model.m1.weight), _cpu(model.m1.bias))
  z = res['z'] = block_solve(model, h, first_edge, opt['method'], opt['step_size'])
  edge = added_edge
  if opt['edge_sampling_rmv'] != 0:
    res['mean_att'] = mean_attention(model, z, edge)
    edge, res['threshold'] = select_edges(edge, res['mean_att'], opt['edge_sampling_rmv'])
    res['kept'] = edge
    if opt['edge_sampling_sym']:
      edge = to_undirected(edge)
  res['edge'] = edge
  z2 = block_solve(model, z, edge, 'rk4', 1)
  res['out'] = torch.nn.functional.linear(torch.relu(z2), _cpu(model.m2.weight), _cpu(model.m2.bias))
  return res


def random_pairs(n, M, seed, call):
  """The 2 M columns add_edges('random') joins to the edge set at call number `call`."""
  return both_directions(random_nodes(n, M, seed, 0, call), random_nodes(n, M, seed, 1, call))


def threshold_clearance(mean_att, threshold):
  """Distance of the mean attention nearest the threshold, relative to the largest mean attention."""
  return float((mean_att - threshold).abs().min() / mean_att.abs().max())
