// Philox4x32-10 (Random123; Salmon, Moraes, Dror, Shaw, SC'11) written out for the device, and the stream layout every random
// draw of this library uses (include/gnpde.h, "Random numbers"): no state, word i of a stream is a pure function of
// (seed, stream, call, i), so a draw does not depend on the launch shape.  Shared by edge_sampling.hip and deepwalk.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace gnpde {

struct Words4 {
  unsigned w[4];
};

// key (k0, k1), counter (c0 .. c3).  Round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2,
// c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by the Weyl constants between rounds.
__device__ __forceinline__ Words4 philox4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
  constexpr unsigned kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(kM0, c0), lo0 = kM0 * c0;
    const unsigned hi1 = __umulhi(kM1, c2), lo1 = kM1 * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += kW0; k1 += kW1;
  }
  Words4 out;
  out.w[0] = c0; out.w[1] = c1; out.w[2] = c2; out.w[3] = c3;
  return out;
}

// block `b` of stream (seed, stream, call): key = the seed's words, counter = (b low, b high, stream, call)
__device__ __forceinline__ Words4 stream_block(unsigned long long seed, unsigned stream, unsigned call, unsigned long long b) {
  return philox4x32_10(static_cast<unsigned>(seed), static_cast<unsigned>(seed >> 32), static_cast<unsigned>(b),
                       static_cast<unsigned>(b >> 32), stream, call);
}

}  // namespace gnpde
