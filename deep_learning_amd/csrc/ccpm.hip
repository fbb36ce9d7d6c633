// CCPM: convolutional field interactions beside the dnn_* tower, forward and backward.
//
// Reference: test_model/CCPM.py:45-68 (Conv2D(3x3, same, relu) + MaxPool2D(2x2) stacked on the sample's
// embedded-field map, Flatten, Dense(1) without its bias) on the F embedded fields of the engine's tower
// input x0 (columns [x_col0, x_col0 + F E), E floats a field).  With X[h, w] = e_w[h] (h < E, w < F),
// H_0' = E, W_0' = F, one input channel, per layer l < L:
//   u_l[h, w, c] = b_l[c] + sum_{dh, dw in -1..1} sum_{c'} K_l[dh+1, dw+1, c', c] a_{l-1}[h+dh, w+dw, c']  (zero outside)
//   a_l[i, j, c] = max over the 2x2 window of relu(u_l);  H_l = H_{l-1} / 2, W_l = W_{l-1} / 2 (floor: a
//   trailing odd row or column is read by the convolution and dropped by the pool)
//   z_ccpm = sum_n a_{L-1}[n] p[n],  n = (i W_L + j) C_L + c  (channels-last Flatten)
// Backward: ReLU's derivative is 0 at u <= 0; the pool's gradient goes to the window's first maximum in
// (row, column) order.  params: [p | K_0 | b_0 | K_1 | b_1 | ...], K_l row-major [3][3][C_{l-1}][C_l].
//
// Mapping (both kernels): one block of 256 threads per sample, samples block-strided; everything per
// sample lives in LDS.  The sample's map is copied as it lies in x0 (field-major, pitch E + 1 so that the
// stride-2 window reads of neighbouring cells fall on different banks); every pooled map is channels-last
// [H_l][W_l][C_l], the order of p.  Convolution, ReLU and pool are one pass: thread = one pooled element
// (i, j, c), c fastest; per input channel it loads the 4x4 input patch under the 2x2 window and the 9
// weights K_l[., ., c', c] into registers and forms the window's four u (36 FMAs from 25 LDS reads: the
// threads of one cell read the same patch words, which broadcast, and consecutive weights), keeps the
// maximum and, in the backward, the window's decision (0..3, or 4 for "no gradient": max <= 0) as a byte.
// Only the pooled maps are stored.  The backward recomputes the forward, then per layer from the last:
// g_l = da_l where the decision passes; the sample's (dK_l, db_l) as thread = parameter element x a group
// of cells, the groups' partial sums added in group order through LDS; da_{l-1}[h, w, c'] as a gather over
// the 9 taps x C_l of the cells whose decision is the position (h - dh, w - dw): no scatter, no atomics.
// dX goes the same way, straight into dx0 (+=).  The batch sums accumulate in an LDS image of the
// parameter vector (thread n owns element n) and leave as one slab row per block; dl_adam_dense sums the
// rows in slab order.  The same inputs give the same bits on every run.
#include <math.h>

#include "common.h"

namespace dl {

constexpr int kCcpmMaxL = 3;
constexpr int kCcpmMaxC = 8;
constexpr int kCcpmMaxF = 64;
constexpr int kCcpmThreads = 256;

// Shapes and LDS offsets (in floats unless said), filled on the host.
struct CcpmPlan {
  int L, F, E;
  int H[kCcpmMaxL + 1], W[kCcpmMaxL + 1], C[kCcpmMaxL + 1];   // index l + 1: layer l's pooled map; 0: the input
  int n[kCcpmMaxL + 1];                                       // elements of map l + 1 (n[0]: E * F)
  int koff[kCcpmMaxL];                                        // K_l in params (b_l follows its 9 C' C values)
  int npar;                                                   // p + all K, b
  int o_prm, o_acc, o_x, o_a[kCcpmMaxL], o_scr, o_dec[kCcpmMaxL];   // o_dec: bytes from the dec base
  int o_decbase;                                              // floats
  int lds_bytes;
};

static bool ccpm_plan(CcpmPlan& P, int F, int E, int L, const int32_t* filters, bool bwd) {
  if (L < 1 || L > kCcpmMaxL || !filters) return false;
  P.L = L, P.F = F, P.E = E;
  P.H[0] = E, P.W[0] = F, P.C[0] = 1, P.n[0] = E * F;
  for (int l = 0; l < L; ++l) {
    if (filters[l] < 1 || filters[l] > kCcpmMaxC) return false;
    P.H[l + 1] = P.H[l] / 2, P.W[l + 1] = P.W[l] / 2, P.C[l + 1] = filters[l];
    if (P.H[l + 1] < 1 || P.W[l + 1] < 1) return false;
    P.n[l + 1] = P.H[l + 1] * P.W[l + 1] * P.C[l + 1];
  }
  int o = P.n[L];
  for (int l = 0; l < L; ++l) {
    P.koff[l] = o;
    o += (9 * P.C[l] + 1) * P.C[l + 1];
  }
  P.npar = o;
  const int np4 = (P.npar + 3) & ~3;
  o = 0;
  P.o_prm = o, o += np4;
  P.o_acc = o, o += bwd ? np4 : 0;
  P.o_x = o, o += (F * (E + 1) + 3) & ~3;
  for (int l = 0; l < L; ++l) P.o_a[l] = o, o += (P.n[l + 1] + 3) & ~3;
  P.o_scr = o, o += kCcpmThreads + 8;
  P.o_decbase = o;
  int ob = 0;
  for (int l = 0; l < L; ++l) P.o_dec[l] = ob, ob += bwd ? (P.n[l + 1] + 3) & ~3 : 0;
  P.lds_bytes = o * 4 + ob;
  return true;
}

// One layer: in (element (h, w, c') at h * sh + w * sw + c' * sc, Hi x Wi x Ci) -> the pooled map out
// [Ho][Wo][Co]; K [3][3][Ci][Co] and b [Co] in LDS.  DEC: the windows' decisions too.
template <bool DEC>
__device__ __forceinline__ void ccpm_layer(const float* in, int sh, int sw, int sc, int Hi, int Wi, int Ci,
                                           const float* K, const float* b, float* out, unsigned char* dec, int Ho,
                                           int Wo, int Co) {
  const int n = Ho * Wo * Co;
  for (int idx = threadIdx.x; idx < n; idx += blockDim.x) {
    const int c = idx % Co, cell = idx / Co;
    const int j = cell % Wo, i = cell / Wo;
    const float bias = b[c];
    float u00 = bias, u01 = bias, u10 = bias, u11 = bias;
    for (int ci = 0; ci < Ci; ++ci) {
      float k[9], p[16];
#pragma unroll
      for (int t = 0; t < 9; ++t) k[t] = K[(t * Ci + ci) * Co + c];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int hh = 2 * i - 1 + r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int ww = 2 * j - 1 + s;
          const bool ok = hh >= 0 && hh < Hi && ww >= 0 && ww < Wi;
          p[r * 4 + s] = ok ? in[hh * sh + ww * sw + ci * sc] : 0.f;
        }
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float kk = k[a * 3 + d];
          u00 = __builtin_fmaf(kk, p[a * 4 + d], u00);
          u01 = __builtin_fmaf(kk, p[a * 4 + d + 1], u01);
          u10 = __builtin_fmaf(kk, p[(a + 1) * 4 + d], u10);
          u11 = __builtin_fmaf(kk, p[(a + 1) * 4 + d + 1], u11);
        }
      }
    }
    float m = u00;
    int arg = 0;
    if (u01 > m) m = u01, arg = 1;
    if (u10 > m) m = u10, arg = 2;
    if (u11 > m) m = u11, arg = 3;
    out[idx] = fmaxf(m, 0.f);
    if (DEC) dec[idx] = (unsigned char)(m > 0.f ? arg : 4);
  }
}

// x0's field columns of sample b into the map buffer (pitch E + 1), then every layer.
template <bool DEC>
__device__ __forceinline__ void ccpm_forward(const CcpmPlan& P, float* lds, const float* __restrict__ row) {
  const int E = P.E, FE = P.F * P.E;
  float* X = lds + P.o_x;
  for (int idx = threadIdx.x; idx < FE; idx += blockDim.x) {
    const int w = idx / E, h = idx - w * E;
    X[w * (E + 1) + h] = row[idx];
  }
  __syncthreads();
  unsigned char* decb = reinterpret_cast<unsigned char*>(lds + P.o_decbase);
  for (int l = 0; l < P.L; ++l) {
    const float* K = lds + P.o_prm + P.koff[l];
    const float* bb = K + 9 * P.C[l] * P.C[l + 1];
    if (l == 0)
      ccpm_layer<DEC>(X, 1, E + 1, 0, P.H[0], P.W[0], 1, K, bb, lds + P.o_a[0], decb + P.o_dec[0], P.H[1], P.W[1],
                      P.C[1]);
    else
      ccpm_layer<DEC>(lds + P.o_a[l - 1], P.W[l] * P.C[l], P.C[l], 1, P.H[l], P.W[l], P.C[l], K, bb, lds + P.o_a[l],
                      decb + P.o_dec[l], P.H[l + 1], P.W[l + 1], P.C[l + 1]);
    __syncthreads();
  }
}

// Block sum in a fixed order (thread-strided partials, the wave's butterfly, waves in order); every
// thread gets the result.  scr: nw + 1 floats.
__device__ __forceinline__ float ccpm_block_sum(float v, float* scr) {
  v = wave_sum(v);
  const int nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) scr[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < nw; ++w) t += scr[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(kCcpmThreads) void ccpm_fwd_kernel(CcpmPlan P, int B, const float* __restrict__ x0,
                                                                int ld, int x_col0, const float* __restrict__ prm,
                                                                const float* __restrict__ z_add,
                                                                float* __restrict__ z_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  for (int i = threadIdx.x; i < P.npar; i += blockDim.x) lds[P.o_prm + i] = prm[i];
  __syncthreads();
  const int nL = P.n[P.L];
  const float* aL = lds + P.o_a[P.L - 1];
  const float* pv = lds + P.o_prm;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    ccpm_forward<false>(P, lds, x0 + (long long)b * ld + x_col0);
    float s = 0.f;
    for (int n = threadIdx.x; n < nL; n += blockDim.x) s = __builtin_fmaf(aL[n], pv[n], s);
    const float z = ccpm_block_sum(s, lds + P.o_scr);
    if (threadIdx.x == 0) z_out[b] = z_add ? z + z_add[b] : z;
  }
}

__global__ __launch_bounds__(kCcpmThreads) void ccpm_bwd_kernel(CcpmPlan P, int B, const float* __restrict__ x0,
                                                                int ld, int x_col0, const float* __restrict__ prm,
                                                                const float* __restrict__ dz,
                                                                float* __restrict__ dx0, int dx_ld, int dx_col0,
                                                                float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* acc = lds + P.o_acc;
  for (int i = threadIdx.x; i < P.npar; i += blockDim.x) {
    lds[P.o_prm + i] = prm[i];
    acc[i] = 0.f;
  }
  __syncthreads();
  const int L = P.L, E = P.E, nt = blockDim.x, tid = threadIdx.x;
  unsigned char* decb = reinterpret_cast<unsigned char*>(lds + P.o_decbase);
  float* scr = lds + P.o_scr;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    ccpm_forward<true>(P, lds, x0 + (long long)b * ld + x_col0);
    const float dzb = dz[b];
    {
      // dp += dz a_L;  g_{L-1} = dz p where the window passes
      const int nL = P.n[L];
      const float* aL = lds + P.o_a[L - 1];
      const unsigned char* dc = decb + P.o_dec[L - 1];
      float* g = lds + P.o_a[L - 1];
      for (int n = tid; n < nL; n += nt) {
        acc[n] = __builtin_fmaf(dzb, aL[n], acc[n]);
        g[n] = dc[n] < 4 ? dzb * lds[P.o_prm + n] : 0.f;
      }
    }
    __syncthreads();
    for (int l = L - 1; l >= 0; --l) {
      const int Ci = P.C[l], Co = P.C[l + 1], Hi = P.H[l], Wi = P.W[l], Ho = P.H[l + 1], Wo = P.W[l + 1];
      const float* in = l ? lds + P.o_a[l - 1] : lds + P.o_x;
      const int sh = l ? Wi * Ci : 1, sw = l ? Ci : E + 1, sc = l ? 1 : 0;
      const float* g = lds + P.o_a[l];
      const unsigned char* dc = decb + P.o_dec[l];
      const float* K = lds + P.o_prm + P.koff[l];
      const int ncell = Ho * Wo, nK = 9 * Ci * Co, NP = nK + Co;
      // (dK_l, db_l): a chunk of at most nt parameter elements at a time, the threads beyond the chunk
      // taking further groups of cells
      for (int base = 0; base < NP; base += nt) {
        const int chunk = NP - base < nt ? NP - base : nt;
        const int G = nt / chunk, gid = tid / chunk, e = tid - gid * chunk, n = base + e;
        float s = 0.f;
        if (gid < G) {
          if (n < nK) {
            const int c = n % Co, ci = (n / Co) % Ci, t = n / (Co * Ci);
            const int dh = t / 3 - 1, dw = t % 3 - 1;
            for (int cell = gid; cell < ncell; cell += G) {
              const int d = dc[cell * Co + c];
              if (d < 4) {
                const int j = cell % Wo, i = cell / Wo;
                const int hh = 2 * i + (d >> 1) + dh, ww = 2 * j + (d & 1) + dw;
                if (hh >= 0 && hh < Hi && ww >= 0 && ww < Wi)
                  s = __builtin_fmaf(g[cell * Co + c], in[hh * sh + ww * sw + ci * sc], s);
              }
            }
          } else {
            const int c = n - nK;
            for (int cell = gid; cell < ncell; cell += G) s += g[cell * Co + c];
          }
          scr[gid * chunk + e] = s;
        }
        __syncthreads();
        if (tid < chunk) {
          float t = 0.f;
          for (int q = 0; q < G; ++q) t += scr[q * chunk + tid];
          acc[P.koff[l] + base + tid] += t;
        }
        __syncthreads();
      }
      // da_{l-1}: a gather over the taps and output channels
      if (l > 0) {
        float* gp = lds + P.o_a[l - 1];
        const unsigned char* dp = decb + P.o_dec[l - 1];
        const int nprev = P.n[l];
        for (int idx = tid; idx < nprev; idx += nt) {
          float s = 0.f;
          if (dp[idx] < 4) {
            const int ci = idx % Ci, pos = idx / Ci;
            const int w = pos % Wi, h = pos / Wi;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
              const int y = h - (t / 3 - 1), x = w - (t % 3 - 1);
              if (y >= 0 && y < 2 * Ho && x >= 0 && x < 2 * Wo) {
                const int cell = (y >> 1) * Wo + (x >> 1), want = (y & 1) * 2 + (x & 1);
                for (int c = 0; c < Co; ++c)
                  if (dc[cell * Co + c] == want) s = __builtin_fmaf(K[(t * Ci + ci) * Co + c], g[cell * Co + c], s);
              }
            }
          }
          gp[idx] = s;
        }
        __syncthreads();
      } else {
        float* drow = dx0 + (long long)b * dx_ld + dx_col0;
        const int FE = P.F * E;
        for (int idx = tid; idx < FE; idx += nt) {
          const int w = idx / E, h = idx - w * E;
          float s = 0.f;
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const int y = h - (t / 3 - 1), x = w - (t % 3 - 1);
            if (y >= 0 && y < 2 * Ho && x >= 0 && x < 2 * Wo) {
              const int cell = (y >> 1) * Wo + (x >> 1), want = (y & 1) * 2 + (x & 1);
              for (int c = 0; c < Co; ++c)
                if (dc[cell * Co + c] == want) s = __builtin_fmaf(K[t * Co + c], g[cell * Co + c], s);
            }
          }
          drow[idx] += s;
        }
        __syncthreads();   // the next sample overwrites the maps
      }
    }
  }
  float* out = slab + (long long)blockIdx.x * P.npar;
  for (int i = tid; i < P.npar; i += nt) out[i] = acc[i];
}

}  // namespace dl

using namespace dl;

extern "C" int dl_ccpm_grid(int32_t B) {
  // one slab row per block, at most 512 as dl_afm_grid: the slab dl_adam_dense sums is bounded
  return B < 1 ? 1 : B > 512 ? 512 : B;
}

static int ccpm_check(const char* name, CcpmPlan& P, bool bwd, int32_t B, int32_t F, int32_t E, int32_t L,
                      const int32_t* filters, const float* x0, int32_t ld, int32_t x_col0, const float* prm) {
  DL_CHECK_ARG(B >= 0, "%s: B %d < 0", name, B);
  DL_CHECK_ARG(F >= 2 && F <= kCcpmMaxF, "%s: F %d fields not in [2, %d]", name, F, kCcpmMaxF);
  DL_CHECK_ARG(E == 8 || E == 16 || E == 32, "%s: E %d not one of 8, 16, 32", name, E);
  DL_CHECK_ARG(L >= 1 && L <= kCcpmMaxL && filters, "%s: L %d layers not in [1, %d]", name, L, kCcpmMaxL);
  for (int l = 0; l < L; ++l)
    DL_CHECK_ARG(filters[l] >= 1 && filters[l] <= kCcpmMaxC, "%s: C %d filters of layer %d not in [1, %d]", name,
                 filters[l], l, kCcpmMaxC);
  DL_CHECK_ARG((F >> L) >= 1 && (E >> L) >= 1, "%s: %d layers halve the %d x %d map below 1", name, L, E, F);
  DL_CHECK_ARG(x0 && prm && x_col0 >= 0 && (long long)x_col0 + (long long)F * E <= ld,
               "%s: x0 and params required, field columns [%d, %d) within ld %d", name, x_col0, x_col0 + F * E, ld);
  DL_CHECK_ARG(ccpm_plan(P, F, E, L, filters, bwd) && P.lds_bytes <= 64 * 1024, "%s: shape does not fit", name);
  return 0;
}

extern "C" int dl_ccpm_fwd(int32_t B, int32_t F, int32_t E, int32_t L, const int32_t* filters, const float* x0,
                           int32_t ld, int32_t x_col0, const float* params, const float* z_add, float* z_out,
                           void* stream) {
  CcpmPlan P;
  if (int rc = ccpm_check("dl_ccpm_fwd", P, false, B, F, E, L, filters, x0, ld, x_col0, params)) return rc;
  DL_CHECK_ARG(z_out, "dl_ccpm_fwd: z_out required");
  if (B == 0) return 0;
  const int grid = B > 2048 ? 2048 : B;
  hipLaunchKernelGGL(ccpm_fwd_kernel, dim3(grid), dim3(kCcpmThreads), P.lds_bytes, as_stream(stream), P, B, x0, ld,
                     x_col0, params, z_add, z_out);
  DL_RETURN_LAUNCH("dl_ccpm_fwd");
}

extern "C" int dl_ccpm_bwd(int32_t B, int32_t F, int32_t E, int32_t L, const int32_t* filters, const float* x0,
                           int32_t ld, int32_t x_col0, const float* params, const float* dz, float* dx0,
                           int32_t dx_ld, int32_t dx_col0, float* slab, int32_t slab_rows, void* stream) {
  CcpmPlan P;
  if (int rc = ccpm_check("dl_ccpm_bwd", P, true, B, F, E, L, filters, x0, ld, x_col0, params)) return rc;
  DL_CHECK_ARG(dz && dx0 && slab, "dl_ccpm_bwd: dz, dx0 and slab required");
  DL_CHECK_ARG(dx_col0 >= 0 && (long long)dx_col0 + (long long)F * E <= dx_ld,
               "dl_ccpm_bwd: dx0 columns [%d, %d) outside dx_ld %d", dx_col0, dx_col0 + F * E, dx_ld);
  const int grid = dl_ccpm_grid(B);
  DL_CHECK_ARG(slab_rows >= grid, "dl_ccpm_bwd: slab needs %d rows", grid);
  if (B == 0) return 0;
  hipLaunchKernelGGL(ccpm_bwd_kernel, dim3(grid), dim3(kCcpmThreads), P.lds_bytes, as_stream(stream), P, B, x0, ld,
                     x_col0, params, dz, dx0, dx_ld, dx_col0, slab);
  DL_RETURN_LAUNCH("dl_ccpm_bwd");
}
