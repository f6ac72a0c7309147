// Host program of tests/test_tape_reverse_schedule_cpu.py: drives the reverse walk csrc/tape_reverse.h states (Real = double) over a
// recorded solve of the scalar ODE y' = theta sin(y) + phi and prints dL/dy0, dL/dtheta, dL/dphi for L = out; and prints the
// coefficient tables the walk is built from.  usage: probe theta phi y0 x h_0 h_1 ...   (hex or decimal floats)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tape_reverse.h"

using namespace gnpde;

namespace {

struct Scalar {
  double theta, phi;
  std::vector<double> tape;          // u_i of step s at 6 s + i
  double buf[kTrBuffers];
  double d_theta = 0.0, d_phi = 0.0;
  int evals = 0;

  double f(double u) const { return theta * std::sin(u) + phi; }

  int scale(int dst, double c) { buf[dst] = c * buf[kTrOut]; return 0; }

  int stage(const TapeStage<double>& t) {
    const double u = tape[static_cast<size_t>(t.slot)], g = buf[t.g_in];
    const double v = theta * std::cos(u) * g;           // J(u)^T G
    d_theta += g * std::sin(u);
    d_phi += g;
    ++evals;
    if (t.w_out >= 0) buf[t.w_out] = v;
    double acc = 0.0;
    for (int j = 0; j < t.n_terms; ++j) acc = buf[t.term[j]] * t.coef[j] + acc;
    acc = v * t.coef[t.n_terms] + acc;
    buf[t.out] = buf[t.base] + acc;
    return 0;
  }

  int sum(const TapeSum<double>& t) {
    double acc = buf[kTrGy];
    for (int j = 0; j < t.n_terms; ++j) acc += t.coef[j] * buf[t.term[j]];
    buf[kTrGy] = acc;
    return 0;
  }
};

}  // namespace

int main(int argc, char** argv) {
  for (int r = 0; r < 6; ++r)
    for (int j = 0; j <= r; ++j) std::printf("a %d %d %a\n", r, j, kDopri5.a[r][j]);
  for (int j = 0; j < 7; ++j) std::printf("mid %d %a\n", j, kDopri5.c_mid[j]);
  if (argc < 6) return 0;
  Scalar s{};
  s.theta = std::strtod(argv[1], nullptr);
  s.phi = std::strtod(argv[2], nullptr);
  const double y0 = std::strtod(argv[3], nullptr), x = std::strtod(argv[4], nullptr);
  std::vector<double> hs;
  for (int i = 5; i < argc; ++i) hs.push_back(std::strtod(argv[i], nullptr));
  const int S = static_cast<int>(hs.size());
  // the forward solve, recorded as csrc/dopri5.hip records it: u_0..u_5 of every accepted step, y1 as u_0 of the next slot
  s.tape.assign(6 * static_cast<size_t>(S) + 1, 0.0);
  double y = y0, k0 = s.f(y0), k[7], out = y0;
  for (int n = 0; n < S; ++n) {
    const double h = hs[n];
    k[0] = k0;
    s.tape[6 * n] = y;
    double u = y;
    for (int i = 1; i <= 6; ++i) {
      double acc = 0.0;
      for (int j = 0; j < i; ++j) acc += kDopri5.a[i - 1][j] * h * k[j];
      u = y + acc;
      s.tape[6 * n + i] = u;
      k[i] = s.f(u);
    }
    if (n == S - 1) {
      double ym = y;
      for (int j = 0; j < 7; ++j) ym += kDopri5.c_mid[j] * h * k[j];
      out = y * (1 - 11 * x * x + 18 * x * x * x - 8 * x * x * x * x) + u * (-5 * x * x + 14 * x * x * x - 8 * x * x * x * x) +
            ym * (16 * x * x - 32 * x * x * x + 16 * x * x * x * x) + k[0] * h * (x - 4 * x * x + 5 * x * x * x - 2 * x * x * x * x) +
            k[6] * h * (x * x - 3 * x * x * x + 2 * x * x * x * x);
    }
    y = u;
    k0 = k[6];
  }
  for (double& b : s.buf) b = 0.0;
  s.buf[kTrOut] = 1.0;          // dL/d(out) of L = out
  if (tape_reverse_walk<double>(S, hs.data(), x, s)) return 1;
  std::printf("out %a\n", out);
  std::printf("evals %d\n", s.evals);
  std::printf("grad %a %a %a\n", s.buf[kTrOut], s.d_theta, s.d_phi);
  return 0;
}
