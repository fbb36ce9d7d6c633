// Cross network of Deep & Cross (DCN) beside the dnn_* tower, forward and backward.
//
// Reference: test_model/DCN.py:73-96 on the engine's own tower input x0 [B, ld] (D = deep_in
// columns, L layers):
//   x_0 = x0;  s_l = x_l . w_l;  x_{l+1} = x0 * s_l + b_l + x_l   (l = 0..L-1)
//   z_cross = x_L . c      (the cross part of the one output layer over [cross_out | deep_out])
// Backward, g_L = dz * c, top down: t_l = g_{l+1} . x0; dw_l += t_l x_l; db_l += g_{l+1};
// dx0 += g_{l+1} s_l; g_l = g_{l+1} + t_l w_l; at the end dx0 += g_0; dc += dz x_L.
//
// Both kernels: one wave64 per sample, the row in registers (K = ceil(D / 64) values a lane,
// column lane + 64 k), cross-lane sums for the dot products, the parameters staged once per block
// in LDS (pitch 64 K, zero past D, so no lane needs a column guard), a capped grid whose waves
// stride over the batch with the next sample's row in flight.  The forward keeps only s [B, L]
// and z_cross [B]: the backward rebuilds every x_l from x0, s and b with the forward's own
// operations (cross_next) and no dot product, so x_L never goes to HBM.  The backward leaves
// per-block partial sums of (dc, dw_l, db_l) in a slab row laid out as the parameter vector
// [c | w_0 .. w_{L-1} | b_0 .. b_{L-1}] (pitch D); dl_adam_dense sums the rows in slab order.
// No atomics: the same inputs give the same bits on every run.
#include "common.h"

namespace dl {

constexpr int kCrossMaxD = 1024;   // 16 values a lane
constexpr int kCrossMaxL = 4;

__device__ __forceinline__ float cross_next(float x0, float s, float b, float xl) {
  return __builtin_fmaf(x0, s, b) + xl;
}

// the (2L + 1) parameter vectors into LDS at pitch P (columns [D, P) zero)
__device__ __forceinline__ void cross_stage(float* lds, const float* __restrict__ prm, int D, int P, int nvec) {
  for (int i = threadIdx.x; i < nvec * P; i += blockDim.x) {
    const int v = i / P, c = i - v * P;
    lds[i] = c < D ? prm[(long long)v * D + c] : 0.f;
  }
  __syncthreads();
}

template <int K>
__device__ __forceinline__ void cross_load_row(const float* __restrict__ x0, int ld, int D, int b, int B, int lane,
                                               float (&r)[K]) {
  const float* row = x0 + (long long)(b < B ? b : 0) * ld;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = lane + 64 * k;
    r[k] = (b < B && c < D) ? row[c] : 0.f;
  }
}

template <int K>
__global__ __launch_bounds__(256) void cross_fwd_kernel(int B, int D, int L, const float* __restrict__ x0, int ld,
                                                        const float* __restrict__ prm, float* __restrict__ s_out,
                                                        float* __restrict__ z_out) {
  constexpr int P = 64 * K;
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [2L + 1][P]
  cross_stage(lds, prm, D, P, 2 * L + 1);
  const float* c = lds;
  const float* w = lds + P;
  const float* bb = lds + (1 + L) * P;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  float xn[K];
  cross_load_row<K>(x0, ld, D, wave, B, lane, xn);
  for (int b = wave; b < B; b += nwaves) {
    float x[K], xl[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = xl[k] = xn[k];
    cross_load_row<K>(x0, ld, D, b + nwaves, B, lane, xn);
    for (int l = 0; l < L; ++l) {
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) part += xl[k] * w[l * P + lane + 64 * k];
      const float s = wave_sum(part);
      if (lane == 0) s_out[(long long)b * L + l] = s;
#pragma unroll
      for (int k = 0; k < K; ++k) xl[k] = cross_next(x[k], s, bb[l * P + lane + 64 * k], xl[k]);
    }
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) part += xl[k] * c[lane + 64 * k];
    const float z = wave_sum(part);
    if (lane == 0) z_out[b] = z;
  }
}

// LM: the layer slots held in registers (L <= LM)
template <int K, int LM>
__global__ __launch_bounds__(256) void cross_bwd_kernel(int B, int D, int L, const float* __restrict__ x0, int ld,
                                                        const float* __restrict__ prm, const float* __restrict__ s_in,
                                                        const float* __restrict__ dz, float* __restrict__ dx0,
                                                        int dx_ld, int dx_col0, int dx_cols,
                                                        float* __restrict__ slab) {
  constexpr int P = 64 * K;
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [2L + 1][P]
  cross_stage(lds, prm, D, P, 2 * L + 1);
  const float* c = lds;
  const float* w = lds + P;
  const float* bb = lds + (1 + L) * P;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  float gc[K], gw[LM][K], gb[LM][K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    gc[k] = 0.f;
#pragma unroll
    for (int l = 0; l < LM; ++l) gw[l][k] = gb[l][k] = 0.f;
  }
  float xn[K];
  cross_load_row<K>(x0, ld, D, wave, B, lane, xn);
  for (int b = wave; b < B; b += nwaves) {
    float x[K], xs[LM][K];   // xs[l] = x_{l+1}
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = xn[k];
    cross_load_row<K>(x0, ld, D, b + nwaves, B, lane, xn);
    // this sample's dx0 columns, in flight during the layers
    float* drow = dx0 + (long long)b * dx_ld - dx_col0;
    float dv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int col = lane + 64 * k;
      dv[k] = (col >= dx_col0 && col < dx_col0 + dx_cols) ? drow[col] : 0.f;
    }
    float sl[LM];
#pragma unroll
    for (int l = 0; l < LM; ++l) sl[l] = l < L ? s_in[(long long)b * L + l] : 0.f;
    const float g0 = dz[b];
#pragma unroll
    for (int l = 0; l < LM; ++l) {
      if (l < L) {
#pragma unroll
        for (int k = 0; k < K; ++k)
          xs[l][k] = cross_next(x[k], sl[l], bb[l * P + lane + 64 * k], l ? xs[l ? l - 1 : 0][k] : x[k]);
      }
    }
    float g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float xL = x[k];
#pragma unroll
      for (int l = 0; l < LM; ++l)
        if (l == L - 1) xL = xs[l][k];
      gc[k] += g0 * xL;
      g[k] = g0 * c[lane + 64 * k];
    }
#pragma unroll
    for (int l = LM - 1; l >= 0; --l) {
      if (l < L) {
        float part = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) part += g[k] * x[k];
        const float t = wave_sum(part);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          gw[l][k] += t * (l ? xs[l ? l - 1 : 0][k] : x[k]);
          gb[l][k] += g[k];
          dv[k] += g[k] * sl[l];
          g[k] += t * w[l * P + lane + 64 * k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int col = lane + 64 * k;
      if (col >= dx_col0 && col < dx_col0 + dx_cols) drow[col] = dv[k] + g[k];
    }
  }
  // block sum in wave order through the staging buffer (the parameters are no longer needed)
  __syncthreads();
  for (int q = 0; q < 4; ++q) {
    if (wid == q) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int col = lane + 64 * k;
        lds[col] = q ? lds[col] + gc[k] : gc[k];
#pragma unroll
        for (int l = 0; l < LM; ++l) {
          if (l < L) {
            float* pw = lds + (1 + l) * P + col;
            float* pb = lds + (1 + L + l) * P + col;
            *pw = q ? *pw + gw[l][k] : gw[l][k];
            *pb = q ? *pb + gb[l][k] : gb[l][k];
          }
        }
      }
    }
    __syncthreads();
  }
  float* out = slab + (long long)blockIdx.x * (2 * L + 1) * D;
  for (int i = threadIdx.x; i < (2 * L + 1) * D; i += blockDim.x) {
    const int v = i / D, col = i - v * D;
    out[i] = lds[v * P + col];
  }
}

}  // namespace dl

using namespace dl;

extern "C" int dl_cross_grid(int32_t B) {
  // ~16 samples a block at least (four a wave), at most 512 blocks: the slab dl_adam_dense sums
  // has a bounded number of rows whatever the batch
  int g = (B + 15) / 16;
  if (g > 512) g = 512;
  return g < 1 ? 1 : g;
}

static int cross_check(const char* name, int32_t B, int32_t D, int32_t L, const float* x0, int32_t ld,
                       const float* prm) {
  DL_CHECK_ARG(B >= 0, "%s: B %d < 0", name, B);
  DL_CHECK_ARG(D >= 1 && D <= kCrossMaxD, "%s: D %d not in [1, %d]", name, D, kCrossMaxD);
  DL_CHECK_ARG(L >= 1 && L <= kCrossMaxL, "%s: cross layers %d not in [1, %d]", name, L, kCrossMaxL);
  DL_CHECK_ARG(x0 && prm && ld >= D, "%s: x0 and params required, ld >= D", name);
  return 0;
}

static int cross_k(int D) {
  const int k = (D + 63) / 64;
  return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
}

extern "C" int dl_cross_fwd(int32_t B, int32_t D, int32_t L, const float* x0, int32_t ld, const float* params,
                            float* s, float* z_cross, void* stream) {
  if (int rc = cross_check("dl_cross_fwd", B, D, L, x0, ld, params)) return rc;
  DL_CHECK_ARG(s && z_cross, "dl_cross_fwd: s and z_cross required");
  if (B == 0) return 0;
  // the forward leaves no slab, so its grid is not the backward's: 8 samples a wave at least, up to
  // 2,048 blocks (at B = 65,536, D = 429, L = 2: 32 us against 50 us on dl_cross_grid's 512)
  const int K = cross_k(D), grid = B >= 32 * 2048 ? 2048 : (B + 31) / 32;
  const size_t lds = (size_t)(2 * L + 1) * 64 * K * sizeof(float);
#define DL_CROSS_FWD(KK)                                                                                        \
  case KK:                                                                                                      \
    hipLaunchKernelGGL(cross_fwd_kernel<KK>, dim3(grid), dim3(256), lds, as_stream(stream), B, D, L, x0, ld,    \
                       params, s, z_cross);                                                                     \
    break;
  switch (K) {
    DL_CROSS_FWD(1) DL_CROSS_FWD(2) DL_CROSS_FWD(4) DL_CROSS_FWD(8) DL_CROSS_FWD(16)
  }
#undef DL_CROSS_FWD
  DL_RETURN_LAUNCH("dl_cross_fwd");
}

extern "C" int dl_cross_bwd(int32_t B, int32_t D, int32_t L, const float* x0, int32_t ld, const float* params,
                            const float* s, const float* dz, float* dx0, int32_t dx_ld, int32_t dx_col0,
                            int32_t dx_cols, float* slab, int32_t slab_rows, void* stream) {
  if (int rc = cross_check("dl_cross_bwd", B, D, L, x0, ld, params)) return rc;
  DL_CHECK_ARG(s && dz && slab, "dl_cross_bwd: s, dz and slab required");
  DL_CHECK_ARG(dx_cols >= 0 && dx_col0 >= 0 && dx_col0 + dx_cols <= D && dx_ld >= dx_cols && (dx0 || !dx_cols),
               "dl_cross_bwd: dx0 columns [%d, %d) outside x0's %d, or dx_ld %d too small", dx_col0,
               dx_col0 + dx_cols, D, dx_ld);
  const int grid = dl_cross_grid(B);
  DL_CHECK_ARG(slab_rows >= grid, "dl_cross_bwd: slab needs %d rows", grid);
  if (B == 0) return 0;
  const int K = cross_k(D), LM = L <= 1 ? 1 : L <= 2 ? 2 : 4;
  const size_t lds = (size_t)(2 * L + 1) * 64 * K * sizeof(float);
#define DL_CROSS_BWD(KK, LL)                                                                                    \
  case KK * 8 + LL:                                                                                             \
    hipLaunchKernelGGL((cross_bwd_kernel<KK, LL>), dim3(grid), dim3(256), lds, as_stream(stream), B, D, L, x0,  \
                       ld, params, s, dz, dx0, dx_ld, dx_col0, dx_cols, slab);                                  \
    break;
#define DL_CROSS_BWD_K(KK) DL_CROSS_BWD(KK, 1) DL_CROSS_BWD(KK, 2) DL_CROSS_BWD(KK, 4)
  switch (K * 8 + LM) {
    DL_CROSS_BWD_K(1) DL_CROSS_BWD_K(2) DL_CROSS_BWD_K(4) DL_CROSS_BWD_K(8) DL_CROSS_BWD_K(16)
  }
#undef DL_CROSS_BWD_K
#undef DL_CROSS_BWD
  DL_RETURN_LAUNCH("dl_cross_bwd");
}
