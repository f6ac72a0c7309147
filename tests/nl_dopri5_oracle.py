"""Shared by tests/test_nltrain_oracle_cpu.py and tests/test_nl_dopri5_tape_gpu.py: the CPU oracle's right-hand side of a GRAND-nl / GAT
block from its options and a dict of parameters (names as in the block's state_dict), and a differentiable replay of the accepted
steps of a dopri5 solve with GIVEN step sizes (torchdiffeq 0.2.1 rk_common.py _runge_kutta_step, interp.py)."""
import torch

from oracle import restate as R
from oracle import tape_reverse as TR

PRE = 'odefunc.multihead_att_layer.'


def oracle_rhs(opt, p, ei, x0, calls=None):
  """f(t, y) of the block's function on the oracle (plain torch, any dtype, differentiable in y and in every tensor of p)."""
  edge, _ = R.add_remaining_self_loops(ei, None, opt['self_loop_weight'], int(ei.max()) + 1)
  alpha, beta = p['odefunc.alpha_train'], p['odefunc.beta_train']
  if opt['function'] == 'GAT':
    def rhs(t, y):
      if calls is not None:
        calls[0] += 1
      return R.rhs_gat(y, edge, p[PRE + 'W'], p[PRE + 'a'], opt['heads'], alpha, beta, x0, opt['no_alpha_sigmoid'], opt['add_source'],
                       opt['leaky_relu_slope'], opt['attention_norm_idx'])
    return rhs
  if opt['beltrami'] and opt['attention_type'] == 'exp_kernel':       # the BLEND split kernel
    lay = {k[len(PRE):]: v for k, v in p.items() if k.startswith(PRE)}

    def rhs(t, y):
      if calls is not None:
        calls[0] += 1
      att = R.transformer_attention_split(y, edge, lay, opt['heads'], opt['feat_hidden_dim'], opt['pos_enc_hidden_dim'],
                                          opt['attention_norm_idx'], opt['square_plus'], None, opt['reweight_attention'])[0]
      return R.rhs_from_attention(y, edge, att, alpha, beta, x0, opt['no_alpha_sigmoid'], opt['add_source'])
    return rhs
  kw = dict(attention_type=opt['attention_type'], norm_idx=opt['attention_norm_idx'], square_plus=opt['square_plus'])
  if opt['attention_type'] == 'exp_kernel':
    kw.update(output_var=p[PRE + 'output_var'], lengthscale=p[PRE + 'lengthscale'])

  def rhs(t, y):
    if calls is not None:
      calls[0] += 1
    return R.rhs_transformer(y, edge, p[PRE + 'Q.weight'], p[PRE + 'Q.bias'], p[PRE + 'K.weight'], p[PRE + 'K.bias'], opt['heads'],
                             alpha, beta, x0, opt['no_alpha_sigmoid'], opt['add_source'], **kw)
  return rhs


def replay(f, y0, hs, x):
  """The accepted steps of a dopri5 solve with the GIVEN step sizes hs and the end point at the fraction x of the last one, every
  operation differentiable: what autograd sees of torchdiffeq's loop once the controller's decisions are constants."""
  dt_ = y0.dtype
  y, k0 = y0, f(None, y0)
  for h in hs:
    h = torch.as_tensor(h, dtype=dt_)
    ks = [k0]
    u = y
    for row in TR.A:
      u = y + sum(kj * (torch.tensor(c, dtype=dt_) * h) for kj, c in zip(ks, row) if c != 0.0)
      ks.append(f(None, u))
    ya, y, k0 = y, u, ks[6]
  ym = ya + sum(kj * (torch.tensor(c, dtype=dt_) * h) for kj, c in zip(ks, TR.MID) if c != 0.0)
  x = torch.as_tensor(x, dtype=dt_)
  fa, fb = ks[0], ks[6]
  ca = 2 * h * (fb - fa) - 8 * (y + ya) + 16 * ym
  cb = h * (5 * fa - 3 * fb) + 18 * ya + 14 * y - 32 * ym
  cc = h * (fb - 4 * fa) - 11 * ya - 5 * y + 16 * ym
  cd = h * fa
  return ya + x * cd + x ** 2 * cc + x ** 3 * cb + x ** 4 * ca
