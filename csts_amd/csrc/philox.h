// Philox4x32-10 (Salmon et al., SC'11), shared by the counter-based random streams of the library: element dropout
// (dropout.hip) and the spatial sampling variates (spatial.hip).  include/csts_hip.h documents how each one forms its counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csts_philox {

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;

__host__ __device__ __forceinline__ void mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  const uint64_t p = (uint64_t)a * b;
  hi = (uint32_t)(p >> 32);
  lo = (uint32_t)p;
}

// ten rounds, the key bumped by the Weyl constants between rounds; c is the counter on entry and the output block on return
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0, lo0, hi1, lo1;
    mulhilo(M0, c[0], hi0, lo0);
    mulhilo(M1, c[2], hi1, lo1);
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += W0;
    k1 += W1;
  }
}

// a 53-bit double in [0, 1) from two words: (a >> 5) * 2^26 + (b >> 6), times 2^-53 (exact)
__host__ __device__ __forceinline__ double uniform53(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

}  // namespace csts_philox
