// Host program of tests/test_embedded_pair_cpu.py: prints what csrc/embedded_pair.h states -- the tableaux, the controller's decision and
// the host's batch rule over fixed tables -- with every floating-point value as a hex float, inputs included.
#include <cmath>
#include <cstdio>
#include "embedded_pair.h"

using namespace gnpde;

static void print_tableau(const char* name, const Tableau& t) {
  std::printf("tableau %s %d %d %d\n", name, t.S, t.fsal, t.order);
  for (int r = 0; r < kMaxStages; ++r)
    for (int j = 0; j < kMaxStages; ++j) std::printf("a %s %d %d %a\n", name, r, j, t.a[r][j]);
  for (int j = 0; j <= kMaxStages; ++j) std::printf("c %s %d %a %a %a\n", name, j, t.c_sol[j], t.c_err[j], t.c_mid[j]);
}

int main() {
  print_tableau("adaptive_heun", kHeun);
  print_tableau("dopri5", kDopri5);

  const float ratios[] = {0.0f, 1e-30f, 0.5f, 1.0f - 0x1p-24f, 1.0f, 1.0f + 0x1p-23f, 7.0f, 1e30f};
  // (t, dt, t1): t + dt just below, equal to and just above t1; t1 far away; values that are no sums of few powers of two
  const double end = 0.25 + 0.125;
  const double spans[][3] = {{0.25, 0.125, std::nextafter(end, 1.0)}, {0.25, 0.125, end}, {0.25, 0.125, std::nextafter(end, 0.0)},
                             {0.25, 0.125, 1.0}, {0.1, 0.03, 0.13}, {0.1, 0.03, 0.1 + 0.03}, {0.7, 1e-3, 4.0}, {0.0, 3.7, 1.0}};
  const int orders[] = {2, 5};
  for (int order : orders)
    for (float ratio : ratios)
      for (const double* s : spans) {
        const StepDecision d = step_decide(s[0], s[1], s[2], ratio, order);
        std::printf("decide %d %a %a %a %a %d %d %a %a %a\n", order, static_cast<double>(ratio), s[0], s[1], s[2], d.accept, d.done,
                    static_cast<double>(d.x), d.t_next, d.dt_next);
      }

  const double dt = 0x1p-6;
  const double starts[] = {0.0, 0.25};
  const double steps_to_end[] = {0.5, 1.0, 1.5, 11.0, 11.5, 111.0, 112.0, 1111.0, 2000.0};      // t1 - t in units of dt
  const int per_sync[] = {1, 3, 8};
  for (int tps : per_sync)
    for (int have = 0; have < 2; ++have)
      for (double t : starts)
        for (double m : steps_to_end) {
          const double t1 = t + m * dt;
          std::printf("plan %d %d %a %a %a %d\n", tps, have, t, dt, t1, plan_batch(t, dt, t1, tps, have != 0));
        }
  return 0;
}
