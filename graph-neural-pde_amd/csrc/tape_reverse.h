// The reverse walk through the ACCEPTED steps of a recorded Dormand-Prince solve for a GENERAL right-hand side f, stated ONCE: what
// autograd does through torchdiffeq 0.2.1's dopri5 loop when opt['adjoint'] is off (rk_common.py _runge_kutta_step, interp.py).  It is
// the algebra of oracle/tape_reverse.py with J(u_i)^T in the place of a (A^T . - .):
//     step     u_0 = y,  u_i = y + h sum_{j<i} a_ij k_j,  u_6 = y1,  k_i = f(u_i),  k_0 = k_6 of the step before
//     reverse  W_6 = G_y1 + J(u_6)^T G_k6
//              G_ki = D_i + h sum_{m>i} a_mi W_m  (a_6j = b_j),   W_i = J(u_i)^T G_ki          i = 5..1
//              G_y  = D_y + sum_m W_m,   G_k0 -> the step before as its G_k6;   k_0 = f(y0) of the first step closes the sweep
// with the direct terms D_i, D_y, G_y1, G_k6 of the quartic end-point interpolant in the last step.  Every evaluation of the sweep is one
// vector-Jacobian product whose epilogue forms the NEXT cotangent; this header answers, per evaluation, which tape slot holds the
// state-side operand, which earlier W's enter the next cotangent with which coefficients, and which coefficient dL/d(out) gets.  The
// order of the terms is the order of the float operations and so part of the gradients' bits.
// Run by the sweep of csrc/adjoint.hip (gnpde_adjoint_set_dopri5_tape; Real = float) and by tests/tape_reverse_probe.cpp (Real = double).
// (The Laplacian sweep gnpde_dopri5_tape_backward of csrc/dopri5.hip keeps its own statement of the same walk: its bits are pinned by
//  tests/test_tape_gpu.py -- moving it here is a follow-up)
// Plain C++ -- no HIP header -- so that a host compiler can build it into a test program.
#pragma once
#include "embedded_pair.h"

namespace gnpde {

// The buffers of the walk.  W_6 is kept as its two summands: kTrW1 + 5 holds J(u_6)^T G_k6 alone and kTrGy -- G_y1 while the step is
// walked -- enters wherever W_6 does, with the same coefficient.  G_k alternates between two buffers (evaluation i reads kTrGk0 + (i & 1),
// its epilogue writes the other one); kTrOut holds dL/d(out) and receives dL/dy0 in the end.
// kTrZero is all zeros and is only ever read.
enum { kTrOut = 0, kTrZero = 1, kTrGy = 2, kTrGk0 = 3, kTrW1 = 5, kTrBuffers = 11 };
constexpr int kTrMaxTerms = 7;

// direct terms of the last step: out = p_y y + p_y1 y1 + p_ym y_mid + p_k0 k_0 + p_k6 k_6 (interp.py: every operand enters linearly),
// y_mid = y + h sum_j c_mid_j k_j.  d[j] dL/d(out) reaches k_j directly, dy dL/d(out) reaches y, gy1 dL/d(out) reaches y1.
template <typename Real>
struct InterpDirect {
  Real d[7], dy, gy1;
};

template <typename Real>
inline InterpDirect<Real> interp_direct(Real x_, Real h_) {
  const double x = static_cast<double>(x_), x2 = x * x, x3 = x2 * x, x4 = x3 * x, hd = static_cast<double>(h_);
  const double p_ym = 16 * x2 - 32 * x3 + 16 * x4, p_y = 1 - 11 * x2 + 18 * x3 - 8 * x4, p_y1 = -5 * x2 + 14 * x3 - 8 * x4;
  const double p_k0 = hd * (x - 4 * x2 + 5 * x3 - 2 * x4), p_k6 = hd * (x2 - 3 * x3 + 2 * x4);
  InterpDirect<Real> D;
  for (int j = 0; j < 7; ++j) D.d[j] = static_cast<Real>(p_ym * hd * kDopri5.c_mid[j]);
  D.d[0] = static_cast<Real>(p_ym * hd * kDopri5.c_mid[0] + p_k0);
  D.d[6] = static_cast<Real>(p_ym * hd * kDopri5.c_mid[6] + p_k6);
  D.dy = static_cast<Real>(p_y + p_ym);
  D.gy1 = static_cast<Real>(p_y1);
  return D;
}

// One evaluation of the sweep: V = J(u)^T G with u = tape buffer `slot` (buffer 6 s + i of the record: u_i of accepted step s; u_6 is
// u_0 of the next step) and G = buffer g_in; V is stored to w_out (if >= 0), and
//     buffer[out] = buffer[base] + (((0 + coef[0] buffer[term[0]]) + coef[1] buffer[term[1]]) + ... + coef[n_terms] V)
// -- the terms in this order, V last, the base added to the finished sum (the GNPDE_STAGE_LINCOMB epilogue).  The parameter gradients
// of the evaluation have weight 1: the cotangents are not normalised (b_1 = 0 rules the c / (b h) form of the rk4 sweep out).
template <typename Real>
struct TapeStage {
  long long slot;
  int g_in, w_out, base, out;
  int n_terms;
  int term[kTrMaxTerms];
  Real coef[kTrMaxTerms + 1];
};

// evaluation i = 6..1 of accepted step `step` (size h): after it W_i and G_k(i-1) exist.  a_mi h is rounded as the forward solve rounds it
// (fl(a) * h in Real); terms with a zero coefficient are not read.
template <typename Real>
inline TapeStage<Real> tape_reverse_stage(int step, int i, Real h, bool last, const InterpDirect<Real>& D) {
  TapeStage<Real> t{};
  t.slot = 6LL * step + i;
  t.g_in = kTrGk0 + (i & 1);
  t.out = kTrGk0 + ((i - 1) & 1);
  t.w_out = kTrW1 + (i - 1);
  t.base = kTrZero;
  int n = 0;
  auto a_h = [&](int m) { return static_cast<Real>(kDopri5.a[m - 1][i - 1]) * h; };      // a_{m, i-1} h
  for (int m = 6; m > i; --m) {
    const Real c = a_h(m);
    if (c == Real(0)) continue;
    t.term[n] = kTrW1 + (m - 1); t.coef[n] = c; ++n;
  }
  const Real c6 = a_h(6);
  if (c6 != Real(0)) { t.term[n] = kTrGy; t.coef[n] = c6; ++n; }                         // the G_y1 summand of W_6
  if (last && D.d[i - 1] != Real(0)) { t.term[n] = kTrOut; t.coef[n] = D.d[i - 1]; ++n; }
  t.n_terms = n;
  t.coef[n] = a_h(i);
  return t;
}

// the first evaluation k_0 = f(y0):  dL/dy0 = G_y + J(y0)^T G_k0, into kTrOut
template <typename Real>
inline TapeStage<Real> tape_reverse_first() {
  TapeStage<Real> t{};
  t.slot = 0;
  t.g_in = kTrGk0;
  t.w_out = -1;
  t.base = kTrGy;
  t.out = kTrOut;
  t.n_terms = 0;
  t.coef[0] = Real(1);
  return t;
}

// G_y = G_y1 + J(u_6)^T G_k6 + W_5 + ... + W_1 (+ D_y dL/d(out) in the last step), in place on kTrGy:  buffer[kTrGy] += sum coef term
template <typename Real>
struct TapeSum {
  int n_terms;
  int term[kTrMaxTerms];
  Real coef[kTrMaxTerms];
};

template <typename Real>
inline TapeSum<Real> tape_reverse_gy(bool last, const InterpDirect<Real>& D) {
  TapeSum<Real> t{};
  for (int m = 6; m >= 1; --m) { t.term[6 - m] = kTrW1 + (m - 1); t.coef[6 - m] = Real(1); }
  t.n_terms = 6;
  if (last && D.dy != Real(0)) { t.term[6] = kTrOut; t.coef[6] = D.dy; t.n_terms = 7; }
  return t;
}

// The whole walk over S accepted steps of sizes h[0..S-1], the end point at the fraction x of the last one.  ops:
//   int scale(int dst, Real c)               buffer[dst] = c buffer[kTrOut]
//   int stage(const TapeStage<Real>&)        one evaluation, as above (its parameter gradients are the callee's business)
//   int sum(const TapeSum<Real>&)            the G_y pass
// The first non-zero status ends it.  6 S + 1 evaluations.
template <typename Real, class Ops>
inline int tape_reverse_walk(int S, const Real* h, Real x, Ops&& ops) {
  if (S < 1) return 0;
  const InterpDirect<Real> D = interp_direct<Real>(x, h[S - 1]);
  if (const int rc = ops.scale(kTrGy, D.gy1)) return rc;
  if (const int rc = ops.scale(kTrGk0, D.d[6])) return rc;
  for (int step = S - 1; step >= 0; --step) {
    const bool last = step == S - 1;
    for (int i = 6; i >= 1; --i)
      if (const int rc = ops.stage(tape_reverse_stage<Real>(step, i, h[step], last, D))) return rc;
    if (const int rc = ops.sum(tape_reverse_gy<Real>(last, D))) return rc;
  }
  return ops.stage(tape_reverse_first<Real>());
}

}  // namespace gnpde
