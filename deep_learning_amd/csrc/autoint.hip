// AutoInt's interacting layers (Song et al. 2019, eq. 5-8) beside the dnn_* tower, forward and backward:
// multi-head self-attention over the embedded fields with a residual projection and a ReLU, stacked.
//
// On the F embedded fields of the engine's tower input x0 (columns [x_col0, x_col0 + F E), E floats a
// field), X^0 = the fields [F, E], D_0 = E, D_l = D, d = D / heads, for l = 1 .. L with X = X^{l-1}:
//   Q = X Wq_l   K = X Wk_l   V = X Wv_l   R = X Wr_l                      [F, D] each, W*_l [D_{l-1}, D]
//   per head h (columns h d .. h d + d - 1):  S = Q_h K_h^T (unscaled), A = softmax over the keys, O_h = A V_h
//   U = O + R    X^l = relu(U)
//   z = sum_{f, c} w[f D + c] X^L[f, c]
// params: [w (F D) | Wq_1 | Wk_1 | Wv_1 | Wr_1 | Wq_2 ..], every matrix row-major.
// Backward: dX^L = dz w, dU = dX^l [U > 0], dR = dO = dU, per head dV = A^T dO, dA = dO V^T,
//   dS = A (dA - rho) with rho[i] = dO[i] . O[i], dQ = dS K, dK = dS^T Q; dW*_l = X^T d*,
//   dX^{l-1} = dQ Wq^T + dK Wk^T + dV Wv^T + dR Wr^T; dX^0 is added into dx0.
//
// A block of 4 waves takes one sample at a time, samples block-strided.  The sample's X and
// T = [Q | K | V | R] [F, 4 D] lie in LDS.
//   projections: one GEMM M = F, K = D_{l-1}, N = 4 D on v_mfma_f32_16x16x4_f32 (exact f32, one k-ordered
//     chain; operand mapping as pnn.hip / cin.hip: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col =
//     lane & 15], accumulator register r = row 4 (lane >> 4) + r, column lane & 15).  A wave owns column
//     tiles; its B operand (the weights, read through L1: at most 16 KB a layer) stays in registers over the
//     row tiles.
//   attention: wave = head, lane = query row i.  The lane holds q_i and walks the keys with an online
//     max / sum (expf), so A never exists as an array.  K_h[k] and V_h[k] are LDS broadcasts.
//   backward attention: the query pass again (m, 1 / l, rho = dO . O per row into LDS, dQ in registers), then a
//     key pass, lane = key k, walking the queries in order: dK[k] and dV[k] are sums over the queries in
//     the lane's own registers, a fixed order and no cross-lane traffic.  Both passes form a score by the
//     same fma chain, so the recomputed score never exceeds the stored maximum.
//   weight gradients X^T dT (M = D_{l-1}, K = F, N = 4 D) on the MFMA, accumulated over the block's samples
//     in registers (a wave owns at most 4 tiles a layer) and written to the block's slab row once; dw
//     likewise in the (head, row) thread's registers.
//   input gradient dT Wc^T (M = F, K = 4 D, N = D_{l-1}) on the MFMA, held in registers across the barrier
//     that ends T's reads, then masked into T's R columns (the next layer down's dU) or added into dx0.
// The backward keeps X^0 .. X^{L-1} in LDS (the ReLU mask of layer l is X^l > 0) and nothing in HBM.
// No atomics, no memset; the same inputs give the same bits on every run.
#include <math.h>

#include "common.h"

namespace dl {

typedef float ai_f4 __attribute__((ext_vector_type(4)));

constexpr int kAiMaxL = 3;
constexpr int kAiMaxF = 64;
constexpr int kAiThreads = 256;        // 4 waves: wave = head in the attention
constexpr int kAiFwdGrid = 2048, kAiBwdGrid = 512;
constexpr int kAiLds = 65536;

// Shapes and LDS offsets (floats), filled on the host.
struct AiPlan {
  int L, F, E, Hn, D;
  int woff[kAiMaxL];   // [Wq | Wk | Wv | Wr] of layer l in params
  int npar;
  int PX, PT;          // pitches of an X map and of T
  int o_x[kAiMaxL];    // X^0 .. X^{L-1} (forward kernel: o_x[0] only, overwritten layer by layer)
  int o_t, o_st, o_red;
  int lds_bytes;
};

static void ai_plan(AiPlan& P, int F, int E, int L, int Hn, int D, bool bwd) {
  P.L = L, P.F = F, P.E = E, P.Hn = Hn, P.D = D;
  int o = F * D;
  for (int l = 0; l < L; ++l) P.woff[l] = o, o += 4 * (l ? D : E) * D;
  P.npar = o;
  P.PX = (E > D ? E : D) + 1;
  P.PT = 4 * D + 4;
  o = 0;
  for (int l = 0; l < kAiMaxL; ++l) {
    P.o_x[l] = o;
    if (l == 0 || (bwd && l < L)) o += F * P.PX;
  }
  P.o_t = o, o += F * P.PT;
  P.o_st = o, o += bwd ? 3 * kAiThreads : 0;
  P.o_red = o, o += 4;
  P.lds_bytes = o * 4;
}

// T[m][n] = sum_k X[m][k] Wc[k][n] for n < ncols (Wc = [Wq | Wk | Wv | Wr], [Dp, D] each).  All threads
// call it; no barrier inside.
__device__ __forceinline__ void ai_proj(const float* X, int PX, int F, int Dp, const float* __restrict__ W, int D,
                                        int ncols, float* T, int PT) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, g = lane >> 4, r = lane & 15;
  const int MT = (F + 15) >> 4, NT = (ncols + 15) >> 4, KS = Dp >> 2;
  for (int nt = wid; nt < NT; nt += kAiThreads / 64) {
    const int n = 16 * nt + r;   // < 4 D: 4 D is a multiple of 16
    const int j = n / D, cc = n - j * D;
    const float* bp = W + j * Dp * D + g * D + cc;
    float bv[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) bv[ks] = ks < KS ? bp[4 * ks * D] : 0.f;
    for (int mt = 0; mt < MT; ++mt) {
      const int m = 16 * mt + r;
      const bool mok = m < F;
      const float* ap = X + (mok ? m : 0) * PX + g;
      ai_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (ks < KS) {
          const float av = mok ? ap[4 * ks] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[ks], acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = 16 * mt + 4 * g + rr;
        if (row < F && n < ncols) T[row * PT + n] = acc[rr];
      }
    }
  }
}

// Query row i of head h: the online softmax over the keys.  o is the unnormalised sum of p V, l the sum of
// p, m the row's maximum score.
template <int d>
__device__ __forceinline__ void ai_attend(const float* T, int PT, int D, int F, int h, int i, float (&q)[d],
                                          float (&o)[d], float& m, float& l) {
  const float* qp = T + i * PT + h * d;
#pragma unroll
  for (int c = 0; c < d; ++c) q[c] = qp[c], o[c] = 0.f;
  m = -INFINITY, l = 0.f;
  const float* kp = T + D + h * d;
  const float* vp = T + 2 * D + h * d;
  for (int k = 0; k < F; ++k) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < d; ++c) s = __builtin_fmaf(q[c], kp[k * PT + c], s);
    const float mn = fmaxf(m, s);
    const float sc = m == -INFINITY ? 0.f : expf(m - mn);
    const float p = expf(s - mn);
    l = __builtin_fmaf(l, sc, p);
#pragma unroll
    for (int c = 0; c < d; ++c) o[c] = __builtin_fmaf(o[c], sc, p * vp[k * PT + c]);
    m = mn;
  }
}

__device__ __forceinline__ void ai_load_x0(float* X, int PX, const float* __restrict__ x0, int ld, int x_col0,
                                           long long b, int F, int E) {
  const float* xr = x0 + b * ld + x_col0;
  for (int idx = threadIdx.x; idx < F * E; idx += kAiThreads) {
    const int f = idx / E, e = idx - f * E;
    X[f * PX + e] = xr[idx];
  }
}

template <int d>
__global__ __launch_bounds__(kAiThreads) void ai_fwd_kernel(AiPlan P, int B, const float* __restrict__ x0, int ld,
                                                            int x_col0, const float* __restrict__ prm,
                                                            const float* __restrict__ z_add,
                                                            float* __restrict__ z_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = P.F, E = P.E, D = P.D, PX = P.PX, PT = P.PT, tid = threadIdx.x;
  const int h = tid >> 6, i = tid & 63;
  const bool act = h < P.Hn && i < F;
  float* X = lds + P.o_x[0];
  float* T = lds + P.o_t;
  float* red = lds + P.o_red;
  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();   // the sample before: X and red are read no more
    ai_load_x0(X, PX, x0, ld, x_col0, b, F, E);
    for (int l = 0; l < P.L; ++l) {
      __syncthreads();
      ai_proj(X, PX, F, l ? D : E, prm + P.woff[l], D, 4 * D, T, PT);
      __syncthreads();
      if (act) {
        float q[d], o[d], m, lsum;
        ai_attend<d>(T, PT, D, F, h, i, q, o, m, lsum);
        const float* rp = T + i * PT + 3 * D + h * d;
        float* xo = X + i * PX + h * d;   // X^{l-1} was read by the projection alone
#pragma unroll
        for (int c = 0; c < d; ++c) xo[c] = fmaxf(o[c] / lsum + rp[c], 0.f);
      }
    }
    __syncthreads();
    float zs = 0.f;
    for (int idx = tid; idx < F * D; idx += kAiThreads) {
      const int f = idx / D, c = idx - f * D;
      zs = __builtin_fmaf(prm[idx], X[f * PX + c], zs);
    }
    zs = wave_sum(zs);
    if ((tid & 63) == 0) red[tid >> 6] = zs;
    __syncthreads();
    if (tid == 0) {
      const float z = ((red[0] + red[1]) + red[2]) + red[3];
      z_out[b] = z_add ? z + z_add[b] : z;
    }
  }
}

template <int d>
__global__ __launch_bounds__(kAiThreads) void ai_bwd_kernel(AiPlan P, int B, const float* __restrict__ x0, int ld,
                                                            int x_col0, const float* __restrict__ prm,
                                                            const float* __restrict__ dz, float* __restrict__ dx0,
                                                            int dx_ld, int dx_col0, float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = P.F, E = P.E, D = P.D, L = P.L, PX = P.PX, PT = P.PT, tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6, g = lane >> 4, r = lane & 15;
  const int h = wid, i = lane;
  const bool act = h < P.Hn && i < F;
  float* T = lds + P.o_t;
  float* st_m = lds + P.o_st;
  float* st_il = st_m + kAiThreads;
  float* st_rho = st_il + kAiThreads;
  float* srow = slab + (long long)blockIdx.x * P.npar;
  float wacc[d];   // dw[i D + h d + c] over the block's samples
#pragma unroll
  for (int c = 0; c < d; ++c) wacc[c] = 0.f;
  ai_f4 dwa[kAiMaxL][4];   // the wave's tiles of dWc_l over the block's samples
#pragma unroll
  for (int li = 0; li < kAiMaxL; ++li)
#pragma unroll
    for (int j = 0; j < 4; ++j) dwa[li][j] = ai_f4{0.f, 0.f, 0.f, 0.f};

  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();
    ai_load_x0(lds + P.o_x[0], PX, x0, ld, x_col0, b, F, E);
    const float dzv = dz[b];
    // the forward again: X^1 .. X^{L-1} kept; the last layer leaves T = [Q | K | V | dU^L] and its share of dw
    for (int l = 0; l < L; ++l) {
      __syncthreads();
      ai_proj(lds + P.o_x[l], PX, F, l ? D : E, prm + P.woff[l], D, 4 * D, T, PT);
      __syncthreads();
      if (act) {
        float q[d], o[d], m, lsum;
        ai_attend<d>(T, PT, D, F, h, i, q, o, m, lsum);
        float* rp = T + i * PT + 3 * D + h * d;
        if (l + 1 < L) {
          float* xo = lds + P.o_x[l + 1] + i * PX + h * d;
#pragma unroll
          for (int c = 0; c < d; ++c) xo[c] = fmaxf(o[c] / lsum + rp[c], 0.f);
        } else {
          const float* wp = prm + i * D + h * d;
#pragma unroll
          for (int c = 0; c < d; ++c) {
            const float u = o[c] / lsum + rp[c];
            wacc[c] = __builtin_fmaf(dzv, fmaxf(u, 0.f), wacc[c]);
            rp[c] = u > 0.f ? dzv * wp[c] : 0.f;   // the thread's own R entries
          }
        }
      }
    }
#pragma unroll
    for (int li = kAiMaxL - 1; li >= 0; --li) {
      if (li < L) {
        const int Dp = li ? D : E;
        const float* Xp = lds + P.o_x[li];
        const float* Wl = prm + P.woff[li];
        // below the top layer: Q K V again (T's R columns already hold this layer's dU)
        if (li < L - 1) ai_proj(Xp, PX, F, Dp, Wl, D, 3 * D, T, PT);
        __syncthreads();
        // query pass: the row's statistics and dQ[i]
        float dq[d];
        if (act) {
          float q[d], o[d], m, lsum;
          ai_attend<d>(T, PT, D, F, h, i, q, o, m, lsum);
          const float il = 1.f / lsum;
          float gq[d];
          const float* gp = T + i * PT + 3 * D + h * d;
          float rho = 0.f;
#pragma unroll
          for (int c = 0; c < d; ++c) gq[c] = gp[c], rho = __builtin_fmaf(gq[c], o[c], rho), dq[c] = 0.f;
          rho *= il;
          const float* kp = T + D + h * d;
          const float* vp = T + 2 * D + h * d;
          for (int k = 0; k < F; ++k) {
            float s = 0.f, da = 0.f;
#pragma unroll
            for (int c = 0; c < d; ++c) {
              s = __builtin_fmaf(q[c], kp[k * PT + c], s);
              da = __builtin_fmaf(gq[c], vp[k * PT + c], da);
            }
            const float ds = expf(s - m) * il * (da - rho);
#pragma unroll
            for (int c = 0; c < d; ++c) dq[c] = __builtin_fmaf(ds, kp[k * PT + c], dq[c]);
          }
          st_m[tid] = m, st_il[tid] = il, st_rho[tid] = rho;
        }
        __syncthreads();
        // key pass: lane = key, the queries in order
        float dk[d], dv[d];
        if (act) {
          float kk[d], vv[d];
          const float* kp = T + i * PT + D + h * d;
#pragma unroll
          for (int c = 0; c < d; ++c) kk[c] = kp[c], vv[c] = kp[D + c], dk[c] = 0.f, dv[c] = 0.f;
          for (int qi = 0; qi < F; ++qi) {
            const float* qp = T + qi * PT + h * d;
            const float* gp = qp + 3 * D;
            float s = 0.f, da = 0.f;
#pragma unroll
            for (int c = 0; c < d; ++c) {
              s = __builtin_fmaf(qp[c], kk[c], s);
              da = __builtin_fmaf(gp[c], vv[c], da);
            }
            const float a = expf(s - st_m[h * 64 + qi]) * st_il[h * 64 + qi];
            const float ds = a * (da - st_rho[h * 64 + qi]);
#pragma unroll
            for (int c = 0; c < d; ++c) {
              dk[c] = __builtin_fmaf(ds, qp[c], dk[c]);
              dv[c] = __builtin_fmaf(a, gp[c], dv[c]);
            }
          }
        }
        __syncthreads();   // Q K V are read no more
        if (act) {
          float* tp = T + i * PT + h * d;
#pragma unroll
          for (int c = 0; c < d; ++c) tp[c] = dq[c], tp[D + c] = dk[c], tp[2 * D + c] = dv[c];
        }
        __syncthreads();   // T = dT = [dQ | dK | dV | dU]
        // dWc_l += X^{l-1}^T dT
        {
          const int MT = (Dp + 15) >> 4, NT = (4 * D) >> 4, KS = (F + 3) >> 2;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int t = wid + 4 * j;
            if (t < MT * NT) {
              const int mt = t % MT, nt = t / MT;
              const int m = 16 * mt + r;
              const bool mok = m < Dp;
              const float* ap = Xp + (mok ? m : 0) + g * PX;
              const float* bp = T + 16 * nt + r + g * PT;
              ai_f4 acc = dwa[li][j];
              for (int ks = 0; ks < KS; ++ks) {
                const bool kok = 4 * ks + g < F;
                const float av = (mok && kok) ? ap[4 * ks * PX] : 0.f;
                const float bv = kok ? bp[4 * ks * PT] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
              }
              dwa[li][j] = acc;
            }
          }
        }
        // dX^{l-1} = dT Wc^T, kept in registers until T's reads are over
        ai_f4 dxa[2];
        const int MTx = (F + 15) >> 4, NTx = (Dp + 15) >> 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          dxa[j] = ai_f4{0.f, 0.f, 0.f, 0.f};
          const int t = wid + 4 * j;
          if (t < MTx * NTx) {
            const int mt = t % MTx, nt = t / MTx;
            const int m = 16 * mt + r, n = 16 * nt + r;
            const bool mok = m < F, nok = n < Dp;
            ai_f4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int jm = 0; jm < 4; ++jm) {
              const float* ap = T + (mok ? m : 0) * PT + jm * D + g;
              const float* bp = Wl + jm * Dp * D + (nok ? n : 0) * D + g;
              for (int ks = 0; ks < (D >> 2); ++ks) {
                const float av = mok ? ap[4 * ks] : 0.f;
                const float bv = nok ? bp[4 * ks] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
              }
            }
            dxa[j] = acc;
          }
        }
        __syncthreads();   // dT is read no more
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int t = wid + 4 * j;
          if (t < MTx * NTx) {
            const int mt = t % MTx, nt = t / MTx;
            const int n = 16 * nt + r;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const int f = 16 * mt + 4 * g + rr;
              if (f < F && n < Dp) {
                if (li > 0)   // dU of the layer below: the ReLU's mask is its output X^l > 0
                  T[f * PT + 3 * D + n] = Xp[f * PX + n] > 0.f ? dxa[j][rr] : 0.f;
                else
                  dx0[b * dx_ld + dx_col0 + f * E + n] += dxa[j][rr];
              }
            }
          }
        }
      }
    }
  }
  // the block's slab row, once
  if (act) {
    float* o = srow + i * D + h * d;
#pragma unroll
    for (int c = 0; c < d; ++c) o[c] = wacc[c];
  }
#pragma unroll
  for (int li = 0; li < kAiMaxL; ++li) {
    if (li < L) {
      const int Dp = li ? D : E;
      const int MT = (Dp + 15) >> 4, NT = (4 * D) >> 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = wid + 4 * j;
        if (t < MT * NT) {
          const int mt = t % MT, nt = t / MT;
          const int n = 16 * nt + r, jm = n / D, cc = n - jm * D;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int dp = 16 * mt + 4 * g + rr;
            if (dp < Dp) srow[P.woff[li] + jm * Dp * D + dp * D + cc] = dwa[li][j][rr];
          }
        }
      }
    }
  }
}

}  // namespace dl

using namespace dl;

extern "C" int dl_autoint_grid(int32_t B) {
  // one slab row per block, a block one sample at a time, at most 512 rows: with at most 14,336 parameters
  // the slab dl_adam_dense sums stays within 30 MB whatever the batch
  return B < 1 ? 1 : (B > kAiBwdGrid ? kAiBwdGrid : B);
}

static int ai_check(const char* name, int32_t B, int32_t F, int32_t E, int32_t L, int32_t heads, int32_t D,
                    const float* x0, int32_t ld, int32_t x_col0, const float* prm) {
  DL_CHECK_ARG(B >= 0, "%s: B %d < 0", name, B);
  DL_CHECK_ARG(F >= 2 && F <= kAiMaxF, "%s: F %d fields not in [2, %d]", name, F, kAiMaxF);
  DL_CHECK_ARG(E == 8 || E == 16 || E == 32, "%s: E %d not one of 8, 16, 32", name, E);
  DL_CHECK_ARG(L >= 1 && L <= kAiMaxL, "%s: L %d layers not in [1, %d]", name, L, kAiMaxL);
  DL_CHECK_ARG(heads == 1 || heads == 2 || heads == 4, "%s: %d heads not one of 1, 2, 4", name, heads);
  DL_CHECK_ARG(D == 8 || D == 16 || D == 32, "%s: D %d not one of 8, 16, 32", name, D);
  DL_CHECK_ARG(D / heads >= 2, "%s: D / heads = %d / %d below 2", name, D, heads);
  DL_CHECK_ARG(x0 && prm && x_col0 >= 0 && (long long)x_col0 + (long long)F * E <= ld,
               "%s: x0 and params required, field columns [%d, %d) within ld %d", name, x_col0, x_col0 + F * E, ld);
  return 0;
}

#define DL_AI_DISPATCH(dd, ...)                            \
  switch (dd) {                                            \
    case 2: { constexpr int kD = 2; __VA_ARGS__; break; }   \
    case 4: { constexpr int kD = 4; __VA_ARGS__; break; }   \
    case 8: { constexpr int kD = 8; __VA_ARGS__; break; }   \
    case 16: { constexpr int kD = 16; __VA_ARGS__; break; } \
    case 32: { constexpr int kD = 32; __VA_ARGS__; break; } \
  }

extern "C" int dl_autoint_fwd(int32_t B, int32_t F, int32_t E, int32_t L, int32_t heads, int32_t D, const float* x0,
                              int32_t ld, int32_t x_col0, const float* params, const float* z_add, float* z_out,
                              void* stream) {
  if (int rc = ai_check("dl_autoint_fwd", B, F, E, L, heads, D, x0, ld, x_col0, params)) return rc;
  DL_CHECK_ARG(z_out, "dl_autoint_fwd: z_out required");
  AiPlan P;
  ai_plan(P, F, E, L, heads, D, false);
  DL_CHECK_ARG(P.lds_bytes <= kAiLds, "dl_autoint_fwd: shape does not fit");
  if (B == 0) return 0;
  const int grid = B > kAiFwdGrid ? kAiFwdGrid : B;
  DL_AI_DISPATCH(D / heads, hipLaunchKernelGGL(ai_fwd_kernel<kD>, dim3(grid), dim3(kAiThreads), P.lds_bytes,
                                               as_stream(stream), P, B, x0, ld, x_col0, params, z_add, z_out));
  DL_RETURN_LAUNCH("dl_autoint_fwd");
}

extern "C" int dl_autoint_bwd(int32_t B, int32_t F, int32_t E, int32_t L, int32_t heads, int32_t D, const float* x0,
                              int32_t ld, int32_t x_col0, const float* params, const float* dz, float* dx0,
                              int32_t dx_ld, int32_t dx_col0, float* slab, int32_t slab_rows, void* stream) {
  if (int rc = ai_check("dl_autoint_bwd", B, F, E, L, heads, D, x0, ld, x_col0, params)) return rc;
  DL_CHECK_ARG(dz && dx0 && slab, "dl_autoint_bwd: dz, dx0 and slab required");
  DL_CHECK_ARG(dx_col0 >= 0 && (long long)dx_col0 + (long long)F * E <= dx_ld,
               "dl_autoint_bwd: dx0 columns [%d, %d) outside dx_ld %d", dx_col0, dx_col0 + F * E, dx_ld);
  const int grid = dl_autoint_grid(B);
  DL_CHECK_ARG(slab_rows >= grid, "dl_autoint_bwd: slab needs %d rows", grid);
  AiPlan P;
  ai_plan(P, F, E, L, heads, D, true);
  DL_CHECK_ARG(P.lds_bytes <= kAiLds, "dl_autoint_bwd: shape does not fit");
  if (B == 0) return 0;
  DL_AI_DISPATCH(D / heads, hipLaunchKernelGGL(ai_bwd_kernel<kD>, dim3(grid), dim3(kAiThreads), P.lds_bytes,
                                               as_stream(stream), P, B, x0, ld, x_col0, params, dz, dx0, dx_ld,
                                               dx_col0, slab));
  DL_RETURN_LAUNCH("dl_autoint_bwd");
}
