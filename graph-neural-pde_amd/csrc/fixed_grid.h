// The stage schedule of the fixed-grid methods (torchdiffeq 0.2.1 `euler`, `midpoint`, `rk4` == 3/8 rule in the compact form of
// gnpde.h), stated ONCE: which GNPDE_STAGE_* evaluation j of a step is and which buffers are its y, k1 and out_y.  Run by the forward
// solver over recycled buffers and over tape slots (solver.hip), the row-partitioned solver (sharded.hip), the continuous adjoint and the
// reverse sweep of a recorded solve (adjoint.hip).  Plain C++ over gnpde.h -- no HIP header -- so that a host compiler can build it into a
// test program (tests/fixed_grid_probe.cpp).
#pragma once
#include "gnpde.h"

namespace gnpde {

// right-hand-side evaluations of one step
inline int evals_per_step(int method) { return method == GNPDE_METHOD_RK4 ? 4 : method == GNPDE_METHOD_MIDPOINT ? 2 : 1; }

// distinct buffers the stage inputs of a solve cycle through: the state and one more (euler ping-pong, midpoint), four for compact rk4
inline int stage_input_buffers(int method) { return method == GNPDE_METHOD_RK4 ? 4 : 2; }

// Epilogue of evaluation j of one step of size dt.  u[0..S-1] are the inputs of the step's S evaluations (u[0] = the state at the step's
// start), u[S] is where the step's result goes (u[S] == u[0]: in place).  `base` carries what does not change from stage to stage (alpha,
// beta, x0; nothing in the adjoint sweeps); a field the stage does not read stays as in `base`.
inline gnpde_epilogue_t stage_epilogue(gnpde_epilogue_t e, int method, int j, float dt, float* const* u) {
  e.dt = dt;
  e.out_y = u[j + 1];
  if (method == GNPDE_METHOD_EULER) {
    e.stage = GNPDE_STAGE_EULER;
    e.y = u[0];
  } else if (method == GNPDE_METHOD_MIDPOINT) {
    // torchdiffeq Midpoint._step_func: y_mid = y + f(y) * (dt / 2);  y += dt * f(y_mid)
    e.stage = GNPDE_STAGE_LINCOMB;
    e.y = u[0];
    e.n_prev = 0;
    e.out_k = nullptr;
    e.coef[0] = j == 0 ? 0.5f * dt : dt;
  } else {
    // compact rk4: RK2C and RK4C read the step's start, RK3C and RK4C the input of the evaluation before the last one
    e.stage = GNPDE_STAGE_RK1C + j;
    if (j == 1 || j == 3) e.y = u[0];
    if (j >= 2) e.k1 = u[j - 1];
  }
  return e;
}

// b_j h: the weight of evaluation j in the step's sum, for the parameter gradients of the adjoint sweeps (euler and rk4; the reverse
// sweep through a midpoint step has its own algebra).  The operation order is part of the gradients' bits.
inline float stage_weight(int method, int j, float dt) {
  if (method != GNPDE_METHOD_RK4) return dt;
  const double c8 = static_cast<double>(dt) * 0.125;
  return j == 0 || j == 3 ? static_cast<float>(c8) : static_cast<float>(3.0 * c8);
}

// One step: eval(j, u[j], epilogue of evaluation j) for every evaluation; the first non-zero status ends it.
template <class Eval>
int enqueue_step(const gnpde_epilogue_t& base, int method, float dt, float* const* u, Eval&& eval) {
  for (int j = 0; j < evals_per_step(method); ++j)
    if (const int rc = eval(j, u[j], stage_epilogue(base, method, j, dt, u))) return rc;
  return 0;
}

}  // namespace gnpde
