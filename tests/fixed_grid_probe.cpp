// Host program of tests/test_fixed_grid_cpu.py: runs the stage schedule of csrc/fixed_grid.h over five dummy buffers and prints, per
// evaluation, the stage, the positions in u[] of the input, y, k1 and out_y (-1: not one of the buffers), coef[0] and the weight.
#include <cstdio>
#include "fixed_grid.h"

using namespace gnpde;

int main() {
  static float bufs[5][1];
  float* u[5] = {bufs[0], bufs[1], bufs[2], bufs[3], bufs[4]};
  auto pos = [&](const float* p) {
    for (int i = 0; i < 5; ++i)
      if (p == u[i]) return i;
    return -1;
  };
  const int methods[] = {GNPDE_METHOD_EULER, GNPDE_METHOD_MIDPOINT, GNPDE_METHOD_RK4};
  const float dts[] = {0.5f, 0.2f, 1.0f, 0.1f, 0.3f, 2.2f / 7.0f};
  for (int m : methods) {
    std::printf("method %d %d %d\n", m, evals_per_step(m), stage_input_buffers(m));
    for (float dt : dts) {
      const int rc = enqueue_step(gnpde_epilogue_t{}, m, dt, u, [&](int j, const float* in, const gnpde_epilogue_t& e) {
        std::printf("eval %d %a %d %d %d %d %d %d %a %a %a\n", m, dt, j, e.stage, pos(in), pos(e.y), pos(e.k1), pos(e.out_y), e.dt, e.coef[0],
                    stage_weight(m, j, dt));
        return e.out_k != nullptr || e.n_prev != 0 || e.k2 != nullptr || e.k3 != nullptr || e.alpha != nullptr ? 1 : 0;
      });
      if (rc) return 1;
    }
  }
  // what the table does not set stays as in `base`; a non-zero status ends the step
  float alpha = 0.f, x0 = 0.f;
  gnpde_epilogue_t base{};
  base.alpha = &alpha;
  base.x0 = &x0;
  base.alpha_sigmoid = 1;
  for (int m : methods)
    for (int j = 0; j < evals_per_step(m); ++j) {
      const gnpde_epilogue_t e = stage_epilogue(base, m, j, 0.5f, u);
      std::printf("base %d %d %d\n", m, j, e.alpha == &alpha && e.beta == nullptr && e.x0 == &x0 && e.alpha_sigmoid == 1 ? 1 : 0);
    }
  int calls = 0;
  const int rc = enqueue_step(base, GNPDE_METHOD_RK4, 0.5f, u, [&](int j, const float*, const gnpde_epilogue_t&) { ++calls; return j == 1 ? 7 : 0; });
  std::printf("status %d %d\n", rc, calls);
  return 0;
}
