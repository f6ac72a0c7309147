// Host program of tests/test_select_cpu.py: prints what the plain-C++ part of csrc/select.h computes -- the order-preserving key of a
// float and its inverse, the bin of a histogram that holds a rank, the column-split rule -- over fixed tables, inputs included.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include "select.h"

using namespace gnpde;

static unsigned bits_of(float f) {
  unsigned u;
  std::memcpy(&u, &f, sizeof(u));
  return u;
}

int main() {
  // ascending; -0 sorts below +0
  const float inf = HUGE_VALF, tiny = 0x1p-149f, least = FLT_MIN;
  const float values[] = {-inf, -FLT_MAX, std::nextafterf(-FLT_MAX, 0.f), std::nextafterf(-1.f, -2.f), -1.f, std::nextafterf(-1.f, 0.f),
                          std::nextafterf(-least, -1.f), -least, std::nextafterf(-least, 0.f), -2 * tiny, -tiny, -0.f, 0.f, tiny, 2 * tiny,
                          std::nextafterf(least, 0.f), least, std::nextafterf(least, 1.f), std::nextafterf(1.f, 0.f), 1.f,
                          std::nextafterf(1.f, 2.f), std::nextafterf(FLT_MAX, 0.f), FLT_MAX, inf};
  for (float v : values) {
    const unsigned key = ordered_key(v);
    std::printf("key %08x %08x %08x\n", bits_of(v), key, bits_of(ordered_value(key)));
  }

  // empty bins before, between and after the occupied ones; one count above 2^32
  const u64 hists[][10] = {{0, 0, 3, 0, 5, (1ull << 32) + 7, 0, 1, 0, 0}, {2, 1, 1, 0, 0, 4, 1, 0, 9, 6}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 1}};
  const int ranges[][2] = {{0, 10}, {2, 8}, {4, 6}, {9, 10}};
  for (int h = 0; h < 3; ++h) {
    std::printf("hist %d", h);
    for (u64 c : hists[h]) std::printf(" %llu", c);
    std::printf("\n");
    for (const int* rg : ranges) {
      u64 total = 0;
      for (int b = rg[0]; b < rg[1]; ++b) total += hists[h][b];
      if (total == 0) continue;
      // both sides of every bin edge (cumulative count - 1 and the count itself), rank 0 and the last rank
      u64 cum = 0;
      for (int b = rg[0]; b <= rg[1]; ++b) {
        for (int side = 0; side < 2; ++side) {
          if (cum + side == 0 || cum + side > total) continue;
          u64 rank = cum + side - 1;
          const u64 asked = rank;
          const int bin = rank_bin(hists[h], rg[0], rg[1], &rank);
          std::printf("rank %d %d %d %llu %d %llu\n", h, rg[0], rg[1], asked, bin, rank);
        }
        if (b < rg[1]) cum += hists[h][b];
      }
    }
  }

  // the two callers' arguments: knn.hip (one workgroup per CU, S <= 32, S k <= 4096 merge keys) and posdist.hip (two per CU, S <= 32)
  const long long ns[] = {1, 64, 65, 2708, 169343};
  const int ks[] = {1, 32, 128}, cus[] = {1, 256}, forced[] = {0, 1, 3, 64};
  for (long long n : ns)
    for (int cu : cus)
      for (int f : forced) {
        for (int k : ks) std::printf("splits knn %lld %d %d %d %d\n", n, k, cu, f, column_splits(n, 1, 32, 4096 / k, cu, f));
        std::printf("splits radius %lld 0 %d %d %d\n", n, cu, f, column_splits(n, 2, 32, 32, cu, f));
      }
  return 0;
}
