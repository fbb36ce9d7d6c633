// Dropout of the deep tower outside the s3 GEMM epilogues (include/dlamd.h "Dropout"): the
// tower input x0, its gradient dx0 and the last layer's gradient, where no GEMM of ours writes
// the tensor.  The mask is the pure function of (seed, step, layer, row, column) the GEMM
// epilogues draw (philox.h drop_keep4) and is never stored: one thread per group of four
// consecutive columns of a row, one Philox call each.
#include "common.h"
#include "philox.h"

namespace dl {

__global__ __launch_bounds__(256) void dropout_apply_kernel(float* x, int M, int N, int ld, uint32_t thr, float inv,
                                                            uint2 key, uint32_t layer, const float* opt,
                                                            uint8_t* mask_out) {
  const int ng = (N + 3) >> 2;
  const long long total = (long long)M * ng;
  const uint32_t step = drop_step(opt);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(i / ng), cg = (int)(i - (long long)row * ng);
    const int col = 4 * cg;
    const uint32_t kb = drop_keep4((uint32_t)row, (uint32_t)cg, layer, step, key, thr);
    if (x) {
      float* px = x + (long long)row * ld + col;
      if (col + 4 <= N && (reinterpret_cast<uintptr_t>(px) & 15) == 0) {
        float4 v = *reinterpret_cast<const float4*>(px);
        v.x = (kb & 1u) ? v.x * inv : 0.f; v.y = (kb & 2u) ? v.y * inv : 0.f;
        v.z = (kb & 4u) ? v.z * inv : 0.f; v.w = (kb & 8u) ? v.w * inv : 0.f;
        *reinterpret_cast<float4*>(px) = v;
      } else {
        for (int e = 0; e < 4 && col + e < N; ++e) px[e] = ((kb >> e) & 1u) ? px[e] * inv : 0.f;
      }
    }
    if (mask_out) {
      uint8_t* pm = mask_out + (long long)row * N + col;
      for (int e = 0; e < 4 && col + e < N; ++e) pm[e] = (uint8_t)((kb >> e) & 1u);
    }
  }
}

}  // namespace dl

using namespace dl;

extern "C" int dl_dropout_apply(float* x, int32_t M, int32_t N, int32_t ld, uint32_t keep_thr, float inv,
                                uint64_t seed, int32_t layer, const float* opt, uint8_t* mask_out, void* stream) {
  DL_CHECK_ARG(x || mask_out, "NULL x and mask_out");
  DL_CHECK_ARG(opt, "opt is NULL");
  DL_CHECK_ARG(M >= 0 && N >= 0 && (!x || ld >= N), "bad shape %d x %d (ld %d)", M, N, ld);
  DL_CHECK_ARG(layer >= 0 && inv >= 1.f && inv < 3.4e38f, "bad dropout layer %d / factor %g", layer, (double)inv);
  if (M == 0 || N == 0) return 0;
  const long long total = (long long)M * ((N + 3) / 4);
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(dropout_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, M, N, ld,
                     keep_thr, inv, make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)), (uint32_t)layer, opt,
                     mask_out);
  DL_RETURN_LAUNCH("dl_dropout_apply");
}
