"""Differentiable evaluation of the right-hand side, so that the
reference's training loop (`loss.backward()` through the solver steps, run_GNN.py:92) works on these
classes.  The FORWARD value is always the native kernels' (identical to inference).

* GRAND-l (`LaplacianODEFunc`): the backward is native too.  With f = a (A x - x) + b x0,
    dL/dx   = a (A^T g - g)          one launch of the same aggregation kernel on the transposed CSR
    dL/dw_e = a g_row . x_col        gnpde_sddmm (only when the edge weights carry gradients: attention block)
    dL/da, dL/db                     two dot products over [N,d]
* GRAND-nl with scaled-dot attention and ANY normaliser (softmax or squareplus, over rows or -- attention_norm_idx = 1,
  what run_GNN.py trains Cora / Citeseer / Pubmed / CoauthorCS with -- columns): native VJP --
  recompute q||k and the attention (native), then  A^T g  (aggregation on the transposed CSR), dw = SDDMM,
  ds = gnpde_softmax_rows_bwd, dq / dk = gnpde_head_spmm over rows / columns, dx += [dq dk] [Wq; Wk] on
  the MFMA projection kernel; the [A,N]x[N,d] weight-gradient GEMMs go to the vendor BLAS through torch.
* the other score functions (cosine / pearson / exp_kernel incl. the BLEND split kernel, GAT incl. mix_features): node-level
  transforms in PyTorch with autograd, everything per edge native (section "Native VJP of the attention for EVERY score
  function" below).
* every head shape: gnpde_head_spmm takes any heads and d_k up to attention_dim = 256 (2A for the BLEND split kernel; GAT
  up to 64 heads), the float4 kernel where d_k % 4 == 0 with attention_dim / 4 a power of two, a generic one otherwise.
* what is left to the composite of PyTorch device ops (index_select / index_add, the reference's op sequence; it announces
  itself once): the second-order regularisers (twice_differentiable_rhs: a kernel-backed autograd function is not twice
  differentiable), opt['gnpde_composite_backward'] (the A/B reference of the gradient tests), and attention widths beyond
  256 (GAT: more than 64 heads).
"""
import logging
import math

import torch

from . import _lib, ops
from .graph import graph_of

_log = logging.getLogger('gnpde_amd')
_warned = set()


def _alpha(func):
  return func.alpha_train if func.opt['no_alpha_sigmoid'] else torch.sigmoid(func.alpha_train)


def _dalpha(g, f, x, alpha_train, beta_train, gx0, sig, aggregate):
  """d/d alpha_train of  f = a (A x - x) + b x0.  With a = sigmoid(alpha_train) > 0 the bracket is (f - b x0) / a, so
  sum g . (A x - x) costs two dot products on tensors that already exist (da/dalpha_train = a (1 - a) cancels the
  division); with a raw alpha (which may be 0) the aggregation is recomputed."""
  if sig:
    s = _dot(g, f)
    if gx0 is not None:
      s = s - beta_train.reshape(()) * gx0
    return s * (1 - torch.sigmoid(alpha_train.reshape(())))
  return _dot(g, aggregate() - x)


def _dot(a, b):
  """sum(a * b) as one reduction kernel (no state-sized product tensor)."""
  return torch.dot(a.reshape(-1), b.reshape(-1))


# --------------------------------------------------------------------------------------------------
# GRAND-l: native forward and backward
# --------------------------------------------------------------------------------------------------
class _LaplacianRhs(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, edge_values, alpha_train, beta_train, x0, func):
    graph = func._graph(x)
    w_csr = func._weights_csr(graph)
    with torch.no_grad():
      f = ops.rhs_eval(func._descriptor(x), x)
    ctx.func, ctx.graph = func, graph
    # the weights of a solve are constant: one snapshot (and one transposed copy, see backward) serves every evaluation
    snap = func._cache.get('w_snapshot')
    # keyed on the graph OBJECT (held by the snapshot, compared with `is`) and the monotonically increasing generation
    # of the weight buffer's contents -- never on id(): the id of an attention tensor freed by an eval forward is
    # reused by the next training forward's tensor, which would make a stale snapshot compare equal
    gen = next(e['gen'] for e in func._cache['w_csr'] if e['graph'] is graph)
    if snap is None or snap[0] is not graph or snap[3] != gen:
      snap = (graph, w_csr.clone(), {}, gen)
      func._cache['w_snapshot'] = snap
    ctx.w_extra = snap[2]
    w_csr = snap[1]
    ctx.save_for_backward(x, w_csr, edge_values, alpha_train, beta_train, x0 if x0 is not None else x.new_zeros(0), f)
    ctx.has_source = x0 is not None
    return f

  @staticmethod
  def backward(ctx, g):
    x, w_csr, edge_values, alpha_train, beta_train, x0, f = ctx.saved_tensors
    func, graph = ctx.func, ctx.graph
    sig = not func.opt['no_alpha_sigmoid']
    g = _lib.f32c(g)
    gt = graph.transposed()
    need = ctx.needs_input_grad
    dx = dw = dalpha = dbeta = None
    with torch.no_grad():
      if need[0]:
        # edge e sits at CSR position p of `graph` and at position p' of the transposed graph: go through edge order
        w_t = ctx.w_extra.get('w_t')
        if w_t is None:
          w_edge = torch.empty_like(w_csr[:graph.e])
          w_edge[graph.perm_long] = w_csr[:graph.e]
          w_t = ops.edge_to_csr_mean(gt, w_edge)
          ctx.w_extra['w_t'] = w_t
        dx = ops.spmm_rhs(gt, w_t, g, alpha_train, None, None, sig)       # a (A^T g - g)
      if need[1]:
        dw_csr = ops.sddmm(graph, g, x, scale=alpha_train, scale_sigmoid=sig)
        dw_e = torch.empty(graph.e, dtype=torch.float32, device=g.device)
        dw_e[graph.perm_long] = dw_csr[:graph.e]
        if edge_values.dim() == 2:                                         # [E,h] attention: mean over heads
          dw = (dw_e / edge_values.shape[1]).unsqueeze(1).expand_as(edge_values).contiguous()
        else:
          dw = dw_e
      gx0 = _dot(g, x0) if ctx.has_source and (need[2] or need[3]) else None
      if need[2]:
        dalpha = _dalpha(g, f, x, alpha_train, beta_train, gx0, sig, lambda: ops.spmm(graph, w_csr, x)).reshape(alpha_train.shape)
      if need[3] and ctx.has_source:
        dbeta = gx0.reshape(beta_train.shape)
    return dx, dw, dalpha, dbeta, None, None


# --------------------------------------------------------------------------------------------------
# GRAND-nl, scaled-dot attention, softmax over the row: native forward and backward
# --------------------------------------------------------------------------------------------------
def _native_transformer_vjp_ok(func):
  lay, opt = func.multihead_att_layer, func.opt
  # scaled-dot scores with ANY normaliser (softmax / squareplus over rows / columns) and any head shape the head-SpMM of
  # d q / d k takes (attention_dim <= 256)
  return (opt['attention_type'] == 'scaled_dot' and not opt['mix_features'] and not getattr(lay, 'split_kernel', False) and
          _head_spmm_shape_ok(lay.attention_dim, lay.h))


def _head_spmm_shape_ok(A, h):
  """The head shapes gnpde_head_spmm takes: h >= 1 heads of A / h columns each, A <= 256."""
  return h >= 1 and A >= h and A % h == 0 and A <= 256


class _TransformerRhs(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, wq, bq, wk, bk, alpha_train, beta_train, x0, func):
    # the same three steps as the library's single-call evaluation (projection, fused row attention, aggregation
    # with the epilogue), issued separately so that q||k and the head-mean weights can be kept for the backward
    # instead of being recomputed there (31 MB next to the 87 MB state at the ogbn-arxiv shape)
    lay = func.multihead_att_layer
    A = lay.attention_dim
    sig = not func.opt['no_alpha_sigmoid']
    with torch.no_grad():
      graph = func._graph(x)
      wqk, bqk = lay.qk_weights()
      qk = ops.linear(x, wqk, bqk)
      st, keep = lay.attention_struct(graph, q=qk, k=qk[:, A:], ldqk=2 * A)
      w_csr, _, _ = ops.edge_attention(graph, st, True, False, False, like=x)
      f = ops.spmm_rhs(graph, w_csr, x, alpha_train, beta_train if x0 is not None else None, x0, sig)
    ctx.func, ctx.graph = func, graph
    ctx.has_source = x0 is not None
    ctx.save_for_backward(x, x0 if x0 is not None else x.new_zeros(0), alpha_train, beta_train, f, qk, w_csr)
    return f

  @staticmethod
  def backward(ctx, g):
    x, x0, alpha_train, beta_train, f, qk, w_csr = ctx.saved_tensors
    func, graph = ctx.func, ctx.graph
    lay = func.multihead_att_layer
    sig = not func.opt['no_alpha_sigmoid']
    A, h, dk = lay.attention_dim, lay.h, lay.d_k
    g = _lib.f32c(g)
    need = ctx.needs_input_grad
    with torch.no_grad():
      wqk, bqk = lay.qk_weights()
      st, keep = lay.attention_struct(graph, q=qk, k=qk[:, A:], ldqk=2 * A)
      # d/dx through the aggregation and the -x term: a (A^T g - g)
      gt = graph.transposed()
      w_edge = torch.empty(graph.e, dtype=torch.float32, device=g.device)
      w_edge[graph.perm_long] = w_csr[:graph.e]
      dx = ops.spmm_rhs(gt, ops.edge_to_csr_mean(gt, w_edge), g, alpha_train, None, None, sig)
      # through the attention weights: r_e = g_row . x_col (unscaled), alpha applied inside the softmax backward
      r = ops.sddmm(graph, g, x)
      if func.opt['attention_norm_idx'] == 0 and not func.opt['square_plus']:
        ds = ops.attention_rows_bwd(graph, st, r, h, scale=alpha_train, scale_sigmoid=sig)   # scores + softmax + its backward
        if ds is None:     # head shapes without a one-pass kernel: per-head attention in edge order, then its backward
          _, att_edge, _ = ops.edge_attention(graph, st, False, True, False, like=x)
          ds = ops.softmax_rows_bwd(graph, att_edge, r, edge_w_csr=lay._reweight_csr(graph), scale=alpha_train, scale_sigmoid=sig)
      else:                # squareplus and / or normalisation over the column: the general segment backward
        ds = ops.edge_attention_bwd(graph, st, r, scale=alpha_train, scale_sigmoid=sig)
      inv = 1.0 / math.sqrt(dk)
      dqk = torch.empty(x.shape[0], 2 * A, dtype=torch.float32, device=x.device)
      ops.head_spmm(graph, ds, qk[:, A:], h, dk, inv, by_column=False, out=dqk[:, :A])
      ops.head_spmm(graph, ds, qk[:, :A], h, dk, inv, by_column=True, out=dqk[:, A:])
      dx = dx + ops.linear(dqk, wqk.t().contiguous())          # [N,2A] x [2A,d] on the MFMA kernel
      dwq = dbq = dwk = dbk = dalpha = dbeta = None
      if need[1] or need[3]:
        dw_all = ops.tall_skinny_gram(dqk, x)                   # [2A,N] x [N,d], both weight gradients at once
        dwq, dwk = (dw_all[:A] if need[1] else None), (dw_all[A:] if need[3] else None)
      if need[2] or need[4]:
        db_all = dqk.sum(dim=0)
        dbq, dbk = (db_all[:A] if need[2] else None), (db_all[A:] if need[4] else None)
      gx0 = _dot(g, x0) if ctx.has_source and (need[5] or need[6]) else None
      if need[5]:
        # raw alpha: sum_i g_i . (A x)_i = sum_e w_e (g_row . x_col), no second aggregation pass
        if sig:
          dalpha = _dalpha(g, f, x, alpha_train, beta_train, gx0, True, None).reshape(alpha_train.shape)
        else:
          dalpha = (torch.dot(w_csr[:graph.e], r[:graph.e]) - _dot(g, x)).reshape(alpha_train.shape)
      if need[6] and ctx.has_source:
        dbeta = gx0.reshape(beta_train.shape)
    return (dx if need[0] else None), dwq, dbq, dwk, dbk, dalpha, dbeta, None, None



# --------------------------------------------------------------------------------------------------
# Native VJP of the attention for EVERY score function (round 2)
#
# att[E,h] = normalise_{row|col}( g(qt_i, kt_j) [* edge_w] )  with  g = scale * <qt_i, kt_j>          ("dot")
#                                                               g = amp * exp(-|qt_i - kt_j|^2 / 2)   ("exp")
#                                                               g = LeakyReLU(ts_i + td_j)            ("gat")
# where (qt, kt) are NODE-level transforms of the projections:  scaled_dot: q, k;  cosine: q / |q| per head;  pearson: centred,
# then normalised;  exp_kernel: q / l;  BLEND split kernel: [q_x / l_x ; q_p / l_p] per head (amp = (ov_x ov_p)^2).
# The node-level part ([N,A] tensors: Linear layers, normalisations, length scales) is ordinary PyTorch with autograd;
# everything per EDGE is native, forward (the inference kernels, unchanged values) and backward:
#   ds = gnpde_edge_attention_bwd_heads(datt)            normaliser backward for any of softmax / squareplus x row / column
#   dot: d qt = scale * sum_row ds kt_j,  d kt = scale * sum_col ds qt_i                      (gnpde_head_spmm)
#   exp: with c = ds * score:  d qt_i = sum_row c (kt_j - qt_i),  d kt_j = sum_col c (qt_i - kt_j),  d amp = sum c / amp
#   gat: with c = ds * LeakyReLU':  d ts_i = sum_row c,  d td_j = sum_col c
# --------------------------------------------------------------------------------------------------
def _heads(t, h):
  return t.view(t.shape[0], h, -1)


def transformed_qk(layer, x):
  """(qt, kt, kind, scale, amp) of SpGraphTransAttentionLayer with autograd history (node-level only)."""
  opt, h = layer.opt, layer.h
  t = opt['attention_type']
  lin = torch.nn.functional.linear
  if getattr(layer, 'split_kernel', False):
    f0, lab = opt['feat_hidden_dim'], opt['feat_hidden_dim'] + opt['pos_enc_hidden_dim']
    p = x[:, f0:lab]
    xf = torch.cat((x[:, :f0], x[:, lab:]), dim=1)
    def both(lx, lp):
      a = _heads(lin(xf, lx.weight, lx.bias) / layer.lengthscale_x, h)
      b = _heads(lin(p, lp.weight, lp.bias) / layer.lengthscale_p, h)
      return torch.cat((a, b), dim=2).reshape(x.shape[0], -1)      # per head: d_k feature rows, then d_k positional rows
    return both(layer.Qx, layer.Qp), both(layer.Kx, layer.Kp), 'exp', 1.0, (layer.output_var_x * layer.output_var_p) ** 2
  q, k = layer.Q(x), layer.K(x)
  if t == 'scaled_dot':
    return q, k, 'dot', 1.0 / math.sqrt(layer.d_k), None
  if t == 'exp_kernel':
    return q / layer.lengthscale, k / layer.lengthscale, 'exp', 1.0, layer.output_var ** 2
  qh, kh = _heads(q, h), _heads(k, h)
  if t == 'pearson':
    qh = qh - qh.mean(dim=2, keepdim=True)
    kh = kh - kh.mean(dim=2, keepdim=True)
  # cosine of the reference clamps |q||k| jointly at 1e-5 (degenerate rows only); the derivative is taken off the clamp
  qh = qh / qh.norm(dim=2, keepdim=True).clamp_min(1e-20)
  kh = kh / kh.norm(dim=2, keepdim=True).clamp_min(1e-20)
  return qh.reshape(q.shape), kh.reshape(k.shape), 'dot', 1.0, None


class _EdgeAttention(torch.autograd.Function):
  """att [E,h] (edge order) from node-level (qt, kt): forward = the inference kernels on the layer's own descriptor (values
  unchanged), backward = native per-edge work, see the section comment."""

  @staticmethod
  def forward(ctx, qt, kt, amp, struct_fn, graph, kind, scale, heads):
    with torch.no_grad():
      st, keep = struct_fn()
      _, att, prods = ops.edge_attention(graph, st, want_w_mean=False, want_att=True, want_prods=True, like=qt)
    ctx.struct_fn, ctx.graph, ctx.kind, ctx.scale, ctx.heads = struct_fn, graph, kind, scale, heads
    ctx.has_amp = amp is not None
    ctx.save_for_backward(qt, kt, amp if amp is not None else qt.new_zeros(0))
    ctx.mark_non_differentiable(prods)      # the raw scores the reference also returns: values only
    return att, prods

  @staticmethod
  def backward(ctx, datt, _dprods):
    qt, kt, amp = ctx.saved_tensors
    graph, kind, h = ctx.graph, ctx.kind, ctx.heads
    dk = qt.shape[1] // h
    with torch.no_grad():
      st, keep = ctx.struct_fn()
      ds = ops.edge_attention_bwd_heads(graph, st, datt, post=1 if kind == 'exp' else 0)
      qc, kc = _lib.f32c(qt.detach()), _lib.f32c(kt.detach())
      damp = None
      if kind == 'dot':
        dq = ops.head_spmm(graph, ds, kc, h, dk, ctx.scale, by_column=False)
        dkk = ops.head_spmm(graph, ds, qc, h, dk, ctx.scale, by_column=True)
      else:
        ones = torch.ones_like(qc)
        dq = ops.head_spmm(graph, ds, kc, h, dk, 1.0, by_column=False) - ops.head_spmm(graph, ds, ones, h, dk, 1.0, by_column=False) * qc
        dkk = ops.head_spmm(graph, ds, qc, h, dk, 1.0, by_column=True) - ops.head_spmm(graph, ds, ones, h, dk, 1.0, by_column=True) * kc
        if ctx.has_amp and ctx.needs_input_grad[2]:
          damp = (ds[:graph.e].sum() / amp.reshape(())).reshape(amp.shape)
    return dq, dkk, damp, None, None, None, None, None


class _GatAttention(torch.autograd.Function):
  """GAT attention [E,h] from the node-level terms ts, td [N,h] (forward: the inference kernels on wx and a)."""

  @staticmethod
  def forward(ctx, ts, td, struct_fn, graph, heads):
    with torch.no_grad():
      st, keep = struct_fn()
      _, att, _ = ops.edge_attention(graph, st, want_w_mean=False, want_att=True, like=ts)
    ctx.struct_fn, ctx.graph, ctx.heads = struct_fn, graph, heads
    return att

  @staticmethod
  def backward(ctx, datt):
    graph, h = ctx.graph, ctx.heads
    with torch.no_grad():
      st, keep = ctx.struct_fn()
      c = ops.edge_attention_bwd_heads(graph, st, datt, post=2)
      ones = torch.ones(graph.n, h, dtype=torch.float32, device=datt.device)     # head sums: the head-SpMM with d_k = 1
      dts = ops.head_spmm(graph, c, ones, h, 1, 1.0, by_column=False)
      dtd = ops.head_spmm(graph, c, ones, h, 1, 1.0, by_column=True)
    return dts, dtd, None, None, None


class _AggregateRhs(torch.autograd.Function):
  """f = a (A x - x) + b x0 with A given by a per-edge attention [E,h] (or [E]) that carries gradients: native forward and
  backward (A^T g on the transposed CSR, d att = SDDMM / H, d alpha, d beta) without touching a function object's caches."""

  @staticmethod
  def forward(ctx, x, att, alpha_train, beta_train, x0, graph, sig):
    with torch.no_grad():
      w_csr = ops.edge_to_csr_mean(graph, att)
      f = ops.spmm_rhs(graph, w_csr, x, alpha_train, beta_train if x0 is not None else None, x0, sig)
    ctx.graph, ctx.sig, ctx.has_source = graph, sig, x0 is not None
    ctx.att_shape = tuple(att.shape)
    ctx.save_for_backward(x, w_csr, alpha_train, beta_train, x0 if x0 is not None else x.new_zeros(0), f)
    return f

  @staticmethod
  def backward(ctx, g):
    x, w_csr, alpha_train, beta_train, x0, f = ctx.saved_tensors
    graph, sig = ctx.graph, ctx.sig
    need = ctx.needs_input_grad
    g = _lib.f32c(g)
    dx = datt = dalpha = dbeta = None
    with torch.no_grad():
      if need[0]:
        gt = graph.transposed()
        w_edge = torch.empty(graph.e, dtype=torch.float32, device=g.device)
        w_edge[graph.perm_long] = w_csr[:graph.e]
        dx = ops.spmm_rhs(gt, ops.edge_to_csr_mean(gt, w_edge), g, alpha_train, None, None, sig)
      if need[1]:
        dw_csr = ops.sddmm(graph, g, x, scale=alpha_train, scale_sigmoid=sig)
        dw_e = torch.empty(graph.e, dtype=torch.float32, device=g.device)
        dw_e[graph.perm_long] = dw_csr[:graph.e]
        if len(ctx.att_shape) == 2:
          datt = (dw_e / ctx.att_shape[1]).unsqueeze(1).expand(ctx.att_shape).contiguous()
        else:
          datt = dw_e
      gx0 = _dot(g, x0) if ctx.has_source and (need[2] or need[3]) else None
      if need[2]:
        dalpha = _dalpha(g, f, x, alpha_train, beta_train, gx0, sig, lambda: ops.spmm(graph, w_csr, x)).reshape(alpha_train.shape)
      if need[3] and ctx.has_source:
        dbeta = gx0.reshape(beta_train.shape)
    return dx, datt, dalpha, dbeta, None, None, None


def native_layer_attention(layer, x, edge):
  """(attention [E,h], prods placeholder) of SpGraphTransAttentionLayer with autograd history, per-edge work native."""
  xc = _lib.f32c(x)
  graph = graph_of(edge, xc.shape[0], xc.device)
  qt, kt, kind, scale, amp = transformed_qk(layer, xc)
  A = layer.kernel_att_dim

  def struct_fn():    # the layer's own inference descriptor (raw projections, its score type): unchanged forward values
    wqk, bqk = layer.qk_weights()
    qk = ops.linear(xc.detach(), wqk, bqk)
    return layer.attention_struct(graph, q=qk, k=qk[:, A:], ldqk=2 * A)

  return _EdgeAttention.apply(_lib.f32c(qt), _lib.f32c(kt), amp, struct_fn, graph, kind, scale, layer.h)   # (att, prods)


def _native_layer_vjp_ok(layer):
  return _head_spmm_shape_ok(layer.kernel_att_dim, layer.h)      # (2A for the BLEND split kernel)


def native_gat_attention(layer, x, edge):
  """GAT attention [E,h] and wx with autograd history (per-edge work native)."""
  xc = _lib.f32c(x)
  graph = graph_of(edge, xc.shape[0], xc.device)
  h, dk = layer.h, layer.d_k
  wx = torch.mm(xc, layer.W)                                           # [N, A]; head j owns columns [j d_k, (j+1) d_k)
  hx = wx.view(-1, h, dk)
  a = layer.a.reshape(2 * dk)
  ts = (hx * a[:dk].view(1, 1, dk)).sum(dim=2)                          # [N,h]
  td = (hx * a[dk:].view(1, 1, dk)).sum(dim=2)

  def struct_fn():
    wxn = ops.linear(xc.detach(), layer.proj_weight())
    return layer.attention_struct(graph, q=wxn, ldqk=layer.attention_dim)

  return _GatAttention.apply(ts.contiguous(), td.contiguous(), struct_fn, graph, h), wx


# --------------------------------------------------------------------------------------------------
# composites of PyTorch device ops: twice-differentiable form for the second-order regularisers, the A/B reference of
# opt['gnpde_composite_backward'], and the fallback for attention widths beyond what gnpde_head_spmm takes (> 256)
# --------------------------------------------------------------------------------------------------
def _segment_softmax(src, index, n):
  mx = torch.full((n,) + tuple(src.shape[1:]), float('-inf'), dtype=src.dtype, device=src.device)
  mx = mx.scatter_reduce(0, index.view(-1, 1).expand_as(src), src.detach(), 'amax', include_self=True)
  out = (src - mx[index]).exp()
  den = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device).index_add_(0, index, out)
  return out / (den[index] + 1e-16)


def _squareplus(src, index, n):
  out = src - src.max()
  out = (out + torch.sqrt(out ** 2 + 4)) / 2
  den = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device).index_add_(0, index, out)
  return out / (den[index] + 1e-16)


def _aggregate(edge, w, x):
  out = torch.zeros_like(x)
  return out.index_add_(0, edge[0], x.index_select(0, edge[1]) * w.unsqueeze(-1))


def composite_transformer(func, x):
  """f(x) of ODEFuncTransformerAtt from differentiable device ops (reference op order)."""
  lay, opt = func.multihead_att_layer, func.opt
  edge = func.edge_index
  att, _ = _layer_attention(lay, x, edge)
  f = _alpha(func) * (_aggregate(edge, att.mean(dim=1), x) - x)
  if opt['add_source']:
    f = f + func.beta_train * func.x0
  return f


def composite_gat(func, x):
  """f(x) of ODEFuncAtt (mix_features False) from differentiable device ops."""
  lay, opt = func.multihead_att_layer, func.opt
  edge, n, h, dk = func.edge_index, x.shape[0], lay.h, lay.d_k
  hx = torch.mm(x, lay.W).view(-1, h, dk).transpose(1, 2)
  edge_h = torch.cat((hx[edge[0]], hx[edge[1]]), dim=1).transpose(0, 1)
  e = torch.nn.functional.leaky_relu(torch.sum(lay.a * edge_h, dim=0), lay.alpha)
  att = _segment_softmax(e, edge[opt['attention_norm_idx']], n)
  f = _alpha(func) * (_aggregate(edge, att.mean(dim=1), x) - x)
  if opt['add_source']:
    f = f + func.beta_train * func.x0
  return f


def composite_laplacian(func, x):
  """f(x) of LaplacianODEFunc from differentiable device ops."""
  w = func._edge_values()
  if w.dim() == 2:
    w = w.mean(dim=1)
  f = _alpha(func) * (_aggregate(func.edge_index, w, x) - x)
  if func.opt['add_source']:
    f = f + func.beta_train * func.x0
  return f


def twice_differentiable_rhs(func, x):
  """f(x) as a composite of PyTorch device ops, for callers that differentiate THROUGH the backward (the regularisers
  of base_classes.py with create_graph=True).  Same arithmetic as the kernels; announced once."""
  _lib.require_hip(x)
  kind = func.__class__.__name__
  comp = {'LaplacianODEFunc': composite_laplacian, 'ODEFuncTransformerAtt': composite_transformer,
          'ODEFuncAtt': composite_gat}.get(kind)
  if comp is None:
    raise NotImplementedError('no twice-differentiable form of %s' % kind)
  if kind == 'ODEFuncAtt' and func.opt['mix_features']:
    raise NotImplementedError('training with mix_features is not supported yet')
  _announce(kind + ' (second-order regulariser)')
  return comp(func, x)


class _CompositeBackwardRhs(torch.autograd.Function):

  @staticmethod
  def forward(ctx, func, composite, x, *params):
    with torch.no_grad():
      f = ops.rhs_eval(func._descriptor(x), x)
    ctx.func, ctx.composite, ctx.params = func, composite, params
    ctx.save_for_backward(x)
    return f

  @staticmethod
  def backward(ctx, g):
    (x,) = ctx.saved_tensors
    with torch.enable_grad():
      xr = x.detach().requires_grad_(True)
      f = ctx.composite(ctx.func, xr)
      grads = torch.autograd.grad(f, [xr] + list(ctx.params), g, allow_unused=True)
    return (None, None) + tuple(grads)


def layer_attention_with_grad(layer, x, edge):
  """(attention [E,h], prods [E,h]) of SpGraphTransAttentionLayer with autograd history (composite); used
  when a block differentiates through the attention it computes once per forward pass."""
  if _native_layer_vjp_ok(layer) and not layer.opt.get('gnpde_composite_backward', False):
    return native_layer_attention(layer, x, edge)
  _announce('SpGraphTransAttentionLayer')
  return _layer_attention(layer, x, edge)


def _layer_attention(layer, x, edge):
  opt = layer.opt
  n, h, dk = x.shape[0], layer.h, layer.d_k
  t = opt['attention_type']
  if getattr(layer, 'split_kernel', False):       # BLEND: feature kernel times positional kernel (reference :133-171)
    f0, lab = opt['feat_hidden_dim'], opt['feat_hidden_dim'] + opt['pos_enc_hidden_dim']
    p = x[:, f0:lab]
    xf = torch.cat((x[:, :f0], x[:, lab:]), dim=1)
    heads = lambda lin, inp: lin(inp).view(-1, h, dk).transpose(1, 2)  # noqa: E731
    dx = heads(layer.Qx, xf)[edge[0]] - heads(layer.Kx, xf)[edge[1]]
    dp = heads(layer.Qp, p)[edge[0]] - heads(layer.Kp, p)[edge[1]]
    prods = layer.output_var_x ** 2 * torch.exp(-torch.sum(dx ** 2, dim=1) / (2 * layer.lengthscale_x ** 2)) \
        * layer.output_var_p ** 2 * torch.exp(-torch.sum(dp ** 2, dim=1) / (2 * layer.lengthscale_p ** 2))
    src = dst = None
  else:
    q = layer.Q(x).view(-1, h, dk).transpose(1, 2)
    k = layer.K(x).view(-1, h, dk).transpose(1, 2)
    src, dst = q[edge[0]], k[edge[1]]
  if src is None:
    pass
  elif t == 'scaled_dot':
    prods = torch.sum(src * dst, dim=1) / math.sqrt(dk)
  elif t == 'exp_kernel':
    prods = layer.output_var ** 2 * torch.exp(-(torch.sum((src - dst) ** 2, dim=1) / (2 * layer.lengthscale ** 2)))
  else:
    if t == 'pearson':
      src = src - src.mean(dim=1, keepdim=True)
      dst = dst - dst.mean(dim=1, keepdim=True)
    prods = torch.nn.functional.cosine_similarity(src, dst, dim=1, eps=1e-5)
  if opt['reweight_attention'] and layer.edge_weights is not None:
    prods = prods * layer.edge_weights.unsqueeze(1)
  idx = edge[opt['attention_norm_idx']]
  att = _squareplus(prods, idx, n) if opt['square_plus'] else _segment_softmax(prods, idx, n)
  return att, prods


def _announce(name):
  if name not in _warned:
    _warned.add(name)
    _log.warning('%s: gradients requested -- forward is native, backward uses the interim PyTorch composite '
                 '(native VJP: SURVEY.md section 8f row 1)', name)


def rhs_with_grad(func, x):
  """Called by ODEFunc.forward when autograd is recording."""
  _lib.require_hip(x)
  x = _lib.f32c(x)
  kind = func.__class__.__name__
  if kind == 'LaplacianODEFunc':
    return _LaplacianRhs.apply(x, func._edge_values(), func.alpha_train, func.beta_train, func._source(x), func)
  if kind == 'ODEFuncTransformerAtt':
    if _native_transformer_vjp_ok(func) and not func.opt.get('gnpde_composite_backward', False):
      lay = func.multihead_att_layer
      return _TransformerRhs.apply(x, lay.Q.weight, lay.Q.bias, lay.K.weight, lay.K.bias, func.alpha_train,
                                   func.beta_train, func._source(x), func)
    lay = func.multihead_att_layer
    if _native_layer_vjp_ok(lay) and not func.opt['mix_features'] and not func.opt.get('gnpde_composite_backward', False):
      # any other score function: node-level transforms in PyTorch, everything per edge native (section comment above)
      att, _ = native_layer_attention(lay, x, func.edge_index)
      return _AggregateRhs.apply(x, att, func.alpha_train, func.beta_train, func._source(x), func._graph(x),
                                 not func.opt['no_alpha_sigmoid'])
    composite = composite_transformer
  elif kind == 'ODEFuncAtt':
    lay = func.multihead_att_layer
    if 1 <= lay.h <= 64 and not func.opt.get('gnpde_composite_backward', False):
      att, wx = native_gat_attention(lay, x, func.edge_index)
      graph, sig = func._graph(x), not func.opt['no_alpha_sigmoid']
      if not func.opt['mix_features']:
        return _AggregateRhs.apply(x, att, func.alpha_train, func.beta_train, func._source(x), graph, sig)
      # mix_features (reference src/function_GAT_attention.py:33-38): A(x) (x W) Wout replaces A(x) x
      zero = torch.zeros((), device=x.device)
      ax = _AggregateRhs.apply(wx.contiguous(), att, torch.ones((), device=x.device), zero, None, graph, False) + wx   # = A wx
      f = _alpha(func) * (torch.mm(ax, lay.Wout) - x)
      if func.opt['add_source']:
        f = f + func.beta_train * func.x0
      return f
    if func.opt['mix_features']:
      raise NotImplementedError('mix_features has no composite backward')
    composite = composite_gat
  else:
    raise NotImplementedError('no backward for %s' % kind)
  _announce(kind)
  params = [p for p in func.parameters() if p.requires_grad]
  return _CompositeBackwardRhs.apply(func, composite, x, *params)
