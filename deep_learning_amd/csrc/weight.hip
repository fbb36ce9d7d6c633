// Per-sample loss weights: the batch's effective weights and the loss normaliser.
//
// Reference: tf.losses.log_loss(label, out, weights=...) with TF 1.x's default reduction
// SUM_BY_NONZERO_WEIGHTS (models/deepfm_pipeline.py:183 leaves weights at 1):
//   loss = sum_b w_b l_b / N_nz,  N_nz = #{b : w_b != 0}  (0 when N_nz == 0: div_no_nan)
// with w_b = weight_b * (1 + (pos_weight - 1) * y_b).  dl_weight_norm writes w_b and
// {inv_norm, N_nz} on the device before the batch's step begins, so the head kernels and the loss
// accumulation read the normaliser where the unweighted step bakes the host constant 1 / B in.
#include "common.h"

namespace dl {

constexpr int kWeightThreads = 1024;

// One block: every thread walks its samples in a fixed stride, four loads in flight; the nonzero
// count is an integer (wave ballots' popcounts, then a fixed-order sum of the 16 wave counts), so
// N_nz and inv_norm are the same bits on every run — no float atomics, no memset.
// A weight that is negative, NaN or infinite makes the batch a bad batch: DL_STATUS_BAD_WEIGHT in
// the batch's validation word (one atomicOr for the block), and that sample's w_eff is written as 0
// (the step is skipped; its forward still runs and must not spread a NaN into gradient buffers).
__global__ __launch_bounds__(kWeightThreads) void weight_norm_kernel(const float* __restrict__ weight,
                                                                     const float* __restrict__ label, int B,
                                                                     float pos_weight, float* __restrict__ w_eff,
                                                                     float* __restrict__ norm,
                                                                     int32_t* __restrict__ err) {
#pragma clang fp contract(off)
  __shared__ int cnt[kWeightThreads / 64];
  __shared__ int any_bad;
  if (threadIdx.x == 0) any_bad = 0;
  __syncthreads();
  const float pm1 = pos_weight - 1.f;
  int nz = 0;
  bool bad = false;
  constexpr int kU = 4;
  for (int b0 = threadIdx.x; b0 < B; b0 += kU * kWeightThreads) {
    float wv[kU], yv[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int b = b0 + u * kWeightThreads;
      wv[u] = (b < B && weight) ? weight[b] : 1.f;
      yv[u] = b < B ? label[b] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int b = b0 + u * kWeightThreads;
      if (b >= B) break;
      const bool ok = wv[u] >= 0.f && wv[u] <= 3.402823466e38f;   // finite and >= 0 (NaN fails both)
      // two separately rounded f32 operations (no FMA): the host restates them bit for bit
      const float f = 1.f + pm1 * yv[u];
      const float w = ok ? wv[u] * f : 0.f;
      bad |= !ok;
      nz += w != 0.f;
      w_eff[b] = w;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) nz += __shfl_xor(nz, o, 64);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = nz;
  if (bad) any_bad = 1;   // every writer stores the same value
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int w = 0; w < kWeightThreads / 64; ++w) n += cnt[w];
    norm[0] = n ? (float)(1.0 / (double)n) : 0.f;
    norm[1] = (float)n;
    if (any_bad && err) atomicOr(err, DL_STATUS_BAD_WEIGHT);
  }
}

// dl_loss_accumulate with the data term's scale read from the device normaliser (norm[1] = N_nz:
// the term is sum / N_nz in double, 0 when N_nz == 0); everything else as loss_accumulate_kernel
// (optim.hip), the status ring included.
__global__ __launch_bounds__(256) void loss_accumulate_weighted_kernel(const float* __restrict__ slab, int rows,
                                                                       int pitch, int col,
                                                                       const float* __restrict__ norm,
                                                                       float* __restrict__ opt, float reg_coef,
                                                                       double* __restrict__ acc,
                                                                       int32_t* __restrict__ ring) {
  __shared__ double part[256];
  if (ring && threadIdx.x == 0) {
    const int k = __float_as_int(opt[DL_OPT_SEQ]) + 1;
    opt[DL_OPT_SEQ] = __int_as_float(k);
    const int* st = opt_status(opt);
    const uint32_t word = ((uint32_t)st[0] & 0xffffu) | ((uint32_t)st[DL_OPT_SKIP - DL_OPT_STATUS] << 16);
    *reinterpret_cast<volatile unsigned long long*>(ring + 2 * (k & 3)) =
        (unsigned long long)(uint32_t)k | ((unsigned long long)word << 32);
  }
  if (step_poisoned(opt)) return;
  double s = 0.0;
  for (int r = threadIdx.x; r < rows; r += blockDim.x) s += (double)slab[(long long)r * pitch + col];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double nz = (double)norm[1];
    acc[0] += part[0] * (nz > 0.0 ? 1.0 / nz : 0.0);
    acc[1] += (double)reg_coef * reg_sum_value(reinterpret_cast<const int64_t*>(opt + DL_OPT_REG));
    acc[2] += 1.0;
  }
}

}  // namespace dl

using namespace dl;

extern "C" int dl_weight_norm(const float* weight, const float* label, int32_t B, float pos_weight, float* w_eff,
                              float* norm, int32_t* err, void* stream) {
  DL_CHECK_ARG(label && w_eff && norm, "NULL argument");
  DL_CHECK_ARG(B > 0 && B <= (1 << 24), "B %d not in [1, 2^24]", B);
  DL_CHECK_ARG(pos_weight > 0.f && pos_weight <= 3.402823466e38f, "pos_weight %g must be finite and > 0",
               (double)pos_weight);
  hipLaunchKernelGGL(weight_norm_kernel, dim3(1), dim3(kWeightThreads), 0, as_stream(stream), weight, label, B,
                     pos_weight, w_eff, norm, err);
  DL_RETURN_LAUNCH("dl_weight_norm");
}

extern "C" int dl_loss_accumulate_weighted(const float* slab, int32_t rows, int32_t pitch, int32_t col,
                                           const float* norm, float* opt, float reg_coef, double* acc,
                                           int32_t* status_ring, void* stream) {
  DL_CHECK_ARG(slab && norm && opt && acc && rows >= 1 && col >= 0 && col < pitch, "bad arguments");
  hipLaunchKernelGGL(loss_accumulate_weighted_kernel, dim3(1), dim3(256), 0, as_stream(stream), slab, rows, pitch,
                     col, norm, opt, reg_coef, acc, status_ring);
  DL_RETURN_LAUNCH("dl_loss_accumulate_weighted");
}
