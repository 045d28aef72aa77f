// Philox4x32-10 and the word -> uniform rule, shared by every kernel that draws noise (misc.hip: lvae_rng_fill_f32; batch_feed.hip: the
// augmenting gather). oracle/philox_ref.py restates both in numpy; the bits are pinned by tests/test_philox_cpu.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lvae {

__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                             uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

// counter words: (element index lo, hi, call-site id, step) -> draws of different steps / call sites never overlap
__device__ __forceinline__ void philox4(uint64_t ctr, uint32_t stream_id, uint32_t step, uint64_t seed, uint32_t out[4]) {
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = stream_id, c3 = step;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// [2^-25, 1 - 2^-24]: (k + 0.5) * 2^-24 for k = r >> 8 < 2^24, in fp32. From k = 2^23 on, k + 0.5 is a tie and rounds to even, which for the
// one input k = 2^24 - 1 is 2^24, i.e. exactly 1.0 (probability 2^-24 per draw): clamped to the largest float below 1, so that a uniform draw
// never reaches its upper end and a keep-probability of 1 keeps everything. Every other draw is what it was without the clamp.
__device__ __forceinline__ float u01(uint32_t r) { return fminf(((r >> 8) + 0.5f) * (1.f / 16777216.f), 0x1.fffffep-1f); }

}  // namespace lvae
