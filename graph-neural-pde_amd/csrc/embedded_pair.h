// The embedded Runge-Kutta pairs and their step-size controller, stated ONCE for the device-controlled forward solve (dopri5.hip) and the
// adaptive adjoint (adjoint_adaptive.hip): torchdiffeq 0.2.1's dopri5.py / adaptive_heun.py (weights), rk_common.py _adaptive_step
// (accept / reject, end point), misc.py _optimal_step_size (next step size) and interp.py (quartic end-point interpolant).
// The first part is plain C++ -- no HIP header -- so that a host compiler can build it into a test program (tests/embedded_pair_probe.cpp);
// the second part (block sum, row copy, pair selection) needs common.h and exists under hipcc only.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GNPDE_HD __host__ __device__
#else
#define GNPDE_HD
#endif

namespace gnpde {

constexpr int kMaxStages = 6;

// stage weights a[r] = weights of the input of stage r + 1 (row S - 1 of a first-same-as-last pair is the solution), solution / error
// (Shampine's variant for Dormand-Prince: 5th - 4th order solution) / mid-point weights over K_0..K_S
struct Tableau {
  int S, fsal, order;
  double a[kMaxStages][kMaxStages];
  double c_sol[kMaxStages + 1], c_err[kMaxStages + 1], c_mid[kMaxStages + 1];
};

// adaptive_heun: ONE evaluation per trial step, k1 = f(y + h k0), y1 = y + h (k0 + k1) / 2; the next step's first derivative is k1
// (rk_common.py takes f1 = k[..., -1] for every pair, also this one, whose last stage is not the solution)
const Tableau kHeun = {1, 0, 2, {{1.0}}, {0.5, 0.5}, {0.5, -0.5}, {0.5, 0.0}};
const Tableau kDopri5 = {
  6, 1, 5,
  {{1.0 / 5},
   {3.0 / 40, 9.0 / 40},
   {44.0 / 45, -56.0 / 15, 32.0 / 9},
   {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
   {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656},
   {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}},
  {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0.0},
  {35.0 / 384 - 1951.0 / 21600, 0.0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720, -2187.0 / 6784 + 12231.0 / 42400,
   11.0 / 84 - 649.0 / 6300, -1.0 / 60},
  {6025192743.0 / 30085553152.0 / 2, 0.0, 51252292925.0 / 65400821598.0 / 2, -2691868925.0 / 45128329728.0 / 2,
   187940372067.0 / 1594534317056.0 / 2, -1776094331.0 / 19743644256.0 / 2, 11237099.0 / 235043384.0 / 2}};

// What the controller decides about one trial step of size dt from t towards t1 whose error ratio (fl32) is ratio32: accepted if
// ratio <= 1; `done` if the accepted step reaches t1, with x = fl32((t1 - t) / dt) the fraction of the step at which t1 lies (0 otherwise);
// t_next = t + dt if accepted, else t; dt_next = dt * clamp(0.9 / ratio^(1 / order), lo, 10) in float64, lo = 1 after an accepted step with
// ratio < 1, else 0.2; ratio == 0 -> x 10.  Values in, values out: the callers keep their records in registers.
struct StepDecision {
  int accept, done;
  float x;
  double t_next, dt_next;
};

GNPDE_HD inline StepDecision step_decide(double t, double dt, double t1, float ratio32, int order) {
  const double ratio = static_cast<double>(ratio32);
  StepDecision d = {0, 0, 0.0f, t, dt};
  if (ratio <= 1.0) {
    const double t_next = t + dt;
    if (t_next >= t1) {
      d.x = static_cast<float>((t1 - t) / (t_next - t));
      d.done = 1;
    }
    d.t_next = t_next;
    d.accept = 1;
  }
  double factor;
  if (ratio == 0.0) {
    factor = 10.0;
  } else {
    const double lo = ratio < 1.0 ? 1.0 : 0.2;
    factor = fmin(10.0, fmax(0.9 / pow(ratio, 1.0 / order), lo));
  }
  d.dt_next = dt * factor;
  return d;
}

// Trial steps the host may queue before it reads the controller record again: as many as cannot pass t1 even if each were accepted
// with the controller's largest growth (x 10) -- dt (10^m - 1) / 9 < t1 - t  =>  m steps cannot finish -- at most trials_per_sync; one
// while nothing is known about dt on the host (before the first read).
inline int plan_batch(double t, double dt, double t1, int trials_per_sync, bool have_record) {
  int batch = 1;
  double reach = dt, step = dt;
  while (have_record && batch < trials_per_sync && t + reach < t1) {
    step *= 10.0;
    reach += step;
    ++batch;
  }
  return batch;
}

// torchdiffeq's quartic through (y0, f0) at 0, (y1, f1) at h and ym at h / 2 (interp.py _interp_fit), evaluated at the fraction x of the
// step (_interp_evaluate).  T: float or a float vector; h, x: float.
template <typename T>
GNPDE_HD inline T quartic(T y0, T y1, T f0, T f1, T ym, float h, float x) {
  const T ca = 2.0f * h * (f1 - f0) - 8.0f * (y1 + y0) + 16.0f * ym;
  const T cb = h * (5.0f * f0 - 3.0f * f1) + 18.0f * y0 + 14.0f * y1 - 32.0f * ym;
  const T cc = h * (f1 - 4.0f * f0) - 11.0f * y0 - 5.0f * y1 + 16.0f * ym;
  const T cd = h * f0;
  T tot = y0 + x * cd;
  float xp = x * x;
  tot += xp * cc;
  xp *= x;
  tot += xp * cb;
  xp *= x;
  tot += xp * ca;
  return tot;
}

}  // namespace gnpde

#if defined(__HIPCC__)
#include "common.h"

namespace gnpde {

inline const Tableau* tableau_of(int pair) {
  return pair == GNPDE_ADAPTIVE_HEUN ? &kHeun : pair == GNPDE_ADAPTIVE_DOPRI5 ? &kDopri5 : nullptr;
}

// sum of one double per thread over a block of kBlock threads (tree over red[kBlock], halving); every thread gets it, red[0] keeps it
__device__ __forceinline__ double block_sum_double(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// dst[r, 0:d] = src[r, 0:d] between two row strides (state in / result out; a pitched hipMemcpy2D is far slower) -- misc.hip
int launch_copy_rows(const float* src, int ld_src, float* dst, int ld_dst, long long n, int d, hipStream_t st);

// grid of the row copies: a block per kBlock elements, at most 8192, at least one
inline unsigned copy_rows_grid(long long n, int d) {
  long long blocks = (n * d + kBlock - 1) / kBlock;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  return static_cast<unsigned>(blocks);
}

// the five counters every device-controlled solve keeps, into the nullable outputs of its *_stats entry point
template <typename Solver>
inline void store_stats(const Solver* s, int32_t* n_evals, int32_t* n_accepted, int32_t* n_rejected, int32_t* n_launches, int32_t* n_syncs) {
  if (n_evals) *n_evals = s->n_evals;
  if (n_accepted) *n_accepted = s->n_accepted;
  if (n_rejected) *n_rejected = s->n_rejected;
  if (n_launches) *n_launches = s->n_launches;
  if (n_syncs) *n_syncs = s->n_syncs;
}

}  // namespace gnpde
#endif
