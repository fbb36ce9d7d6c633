// Philox-4x32-10 counter-based RNG (Salmon et al., SC'11), shared by the parameter init
// (optim.hip), the deep tower's dropout mask (gemm_s3.hip, dropout.hip) and the FM part's (head.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dl {

__device__ __forceinline__ uint4 philox(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c.z;
    c = make_uint4((unsigned)(p1 >> 32) ^ c.y ^ k.x, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k.y,
                   (unsigned)p0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}

// The dropout mask of the deep tower (include/dlamd.h "Dropout"): the keep bits of elements
// (row, 4 cg .. 4 cg + 3) of tensor `layer` at step `step` — bit j set iff word j of
// philox(counter (row, cg, layer, step), key seed) is below thr.
__device__ __forceinline__ uint32_t drop_keep4(uint32_t row, uint32_t cg, uint32_t layer, uint32_t step,
                                               uint2 key, uint32_t thr) {
  const uint4 r = philox(make_uint4(row, cg, layer, step), key);
  return (uint32_t)(r.x < thr) | ((uint32_t)(r.y < thr) << 1) | ((uint32_t)(r.z < thr) << 2) |
         ((uint32_t)(r.w < thr) << 3);
}

// The keep bit of the single element (row, col): the FM part's dropout (head.hip), where a lane
// owns one FM column of a sample.
__device__ __forceinline__ bool drop_keep1(uint32_t row, uint32_t col, uint32_t layer, uint32_t step, uint2 key,
                                           uint32_t thr) {
  return (drop_keep4(row, col >> 2, layer, step, key, thr) >> (col & 3u)) & 1u;
}

// the step the mask is drawn for: opt[7], the global step as a float (exact below 2^24), read on
// the device so a replayed graph draws a new mask every step
__device__ __forceinline__ uint32_t drop_step(const float* opt) { return (uint32_t)opt[7]; }

}  // namespace dl
