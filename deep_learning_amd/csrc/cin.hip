// Compressed Interaction Network (xDeepFM, Lian et al. 2018, eq. 6-8) beside the dnn_* tower, forward and
// backward.  Direct form, identity activation, no bias, no split-half.
//
// On the F embedded fields of the engine's tower input x0 (columns [x_col0, x_col0 + F E), E floats a
// field), X^0 = the fields [F, E], H_0 = F, for the L layers of H_k feature maps:
//   X^k[h, e] = sum_{i < H_{k-1}} sum_{j < F} W^k[h, i, j] X^{k-1}[i, e] X^0[j, e]
//   z_cin     = sum_k sum_h c[off_k + h] sum_e X^k[h, e]
// params: [c (sum H_k) | W^1 | W^2 | ..], W^k stored [H_{k-1} F, H_k]: row kk = i F + j, column h.
// Backward, D^k[h, e] = dz c[off_k + h] + G^k[h, e] (G^L = 0):
//   dW^k[h, (i, j)] = sum_b sum_e D^k[h, e] X^{k-1}[i, e] X^0[j, e]      dc[off_k + h] = sum_b dz sum_e X^k[h, e]
//   dZ[(i, j), e] = sum_h W^k[h, (i, j)] D^k[h, e]
//   G^{k-1}[i, e] = sum_j dZ[(i, j), e] X^0[j, e]      dX^0[j, e] += sum_i dZ[(i, j), e] X^{k-1}[i, e]
//   (k = 1: G^0 goes into dX^0 too)
//
// Every layer is a GEMM over the (sample, e) columns with K = H_{k-1} F, on v_mfma_f32_16x16x4_f32 (exact
// f32, a k-ordered fma chain; operand mapping as pnn.hip: A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15], accumulator register r = row 4 (lane >> 4) + r, column lane & 15).
// A block owns a unit of kCinNC = 32 columns at a time (4 / 2 / 1 samples at E = 8 / 16 / 32), units
// block-strided; the unit's maps X^0 .. X^{L-1} lie in LDS as [row][kCinP], and the operand
// Z[(i, j), col] = X^{k-1}[i, col] X^0[j, col] is one multiply of two LDS words in the lane that feeds it to
// the MFMA: Z exists nowhere else.  W^k streams through LDS in chunks of rows, staged by all threads.
//   forward GEMM (cin_layer): A = W^k (rows h, 16 a tile), B = Z, k = kk; work item = (column tile, row
//     tile), at most 8, dealt to the waves; the accumulators stay in registers over the chunks.
//   weight gradient (cin_dw): A = D^k (rows h), B = Z^T (k = the unit's 32 columns, n = kk); work item =
//     (row tile, 16 rows of kk), dealt to the waves; the tile is added into the block's own slab row in
//     HBM (stored by the block's first unit): one thread owns an element for the whole launch.
//   input gradient (cin_dz): A = W^k transposed (rows j of one i, padded to 16), B = D^k (k = h); a wave
//     owns a column tile and every (nw / 2)-th i.  A lane then holds dZ of 4 j's of its column: G^{k-1}
//     is 4 fmas a tile and two lane-xor adds in a fixed order, dX^0's share accumulates in the lane's own
//     registers over i and is added into dx0 by the column tile's waves in wave order.
// No atomics, no memset; the same inputs give the same bits on every run.
#include <math.h>

#include "common.h"

namespace dl {

typedef float cin_f4 __attribute__((ext_vector_type(4)));

constexpr int kCinMaxL = 3;
constexpr int kCinMaxH = 64;
constexpr int kCinMaxF = 64;
constexpr int kCinMaxW = 262144;       // sum_k H_k H_{k-1} F: bounds the slab (128 rows) at 128 MB
constexpr int kCinNC = 32;             // (sample, e) columns a block owns at a time
constexpr int kCinNCT = kCinNC / 16;   // column tiles
constexpr int kCinP = kCinNC + 2;      // pitch of the maps: rows j, j + 1, .. at k-step columns fall on distinct banks
constexpr int kCinLds = 65536;         // dynamic LDS a block may take
constexpr int kCinFwdThreads = 256, kCinBwdThreads = 512;
constexpr int kCinFwdGrid = 1024, kCinBwdGrid = 128;
constexpr int kCinFwdChunk = 4096;     // floats of the forward's W chunk (the backward takes what is left)

// pitch of a W chunk staged for the forward GEMM (rows kk, 16 consecutive h a lane group): HP / 16 odd
__host__ __device__ __forceinline__ int cin_hp(int H) {
  const int h16 = (H + 15) & ~15;
  return (h16 & 16) ? h16 : h16 + 16;
}
// pitch of a W chunk staged for the input gradient (rows (i, j), k-step columns h): = 2 mod 32
__host__ __device__ __forceinline__ int cin_hq(int H) {
  return H <= 32 ? 34 : 66;
}

// Shapes and LDS offsets (floats), filled on the host.
struct CinPlan {
  int L, F, E;
  int H[kCinMaxL + 1];       // H[0] = F
  int coff[kCinMaxL];        // layer k + 1's part of c
  int woff[kCinMaxL];        // W^{k+1} in params
  int SH, npar;
  int o_x[kCinMaxL];         // X^0 .. X^{L-1} (forward kernel: o_x[0] only)
  int o_a, o_b;              // two maps of RB rows
  int o_s;                   // kCinNC floats
  int o_w, wfloats;          // the W chunk
  int lds_bytes;
};

static bool cin_plan(CinPlan& P, int F, int E, int L, const int32_t* layers, bool bwd) {
  if (L < 1 || L > kCinMaxL || !layers) return false;
  P.L = L, P.F = F, P.E = E, P.H[0] = F;
  long long nw = 0;
  int sh = 0, hmax = 0;
  for (int k = 0; k < L; ++k) {
    if (layers[k] < 1 || layers[k] > kCinMaxH) return false;
    P.H[k + 1] = layers[k];
    P.coff[k] = sh, sh += layers[k];
    nw += (long long)layers[k] * P.H[k] * F;
    if (layers[k] > hmax) hmax = layers[k];
  }
  if (nw > kCinMaxW) return false;
  P.SH = sh;
  int o = sh;
  for (int k = 0; k < L; ++k) P.woff[k] = o, o += P.H[k + 1] * P.H[k] * F;
  P.npar = o;
  const int rb = bwd && F > hmax ? F : hmax;
  o = 0;
  P.o_x[0] = o, o += F * kCinP;
  for (int k = 1; k < L; ++k) P.o_x[k] = o, o += bwd ? P.H[k] * kCinP : 0;
  P.o_a = o, o += rb * kCinP;
  P.o_b = o, o += rb * kCinP;
  P.o_s = o, o += kCinNC;
  o = (o + 3) & ~3;
  P.o_w = o;
  int need = 4 * cin_hp(hmax);                                       // 4 rows of the forward's chunk
  if (bwd && F * cin_hq(hmax) > need) need = F * cin_hq(hmax);       // one i of the input gradient's
  int have = kCinLds / 4 - o;
  if (!bwd && have > kCinFwdChunk) have = kCinFwdChunk < need ? need : kCinFwdChunk;
  if (have < need) return false;
  P.wfloats = have;
  P.lds_bytes = (o + have) * 4;
  return true;
}

// x0's field columns of the unit's samples (from b0, zero past B) into the map X0[f][col = bl E + e]
__device__ __forceinline__ void cin_load_x0(float* X0, const float* __restrict__ x0, int ld, int x_col0, long long b0,
                                            int B, int F, int E) {
  const int FE = F * E;
  for (int idx = threadIdx.x; idx < F * kCinNC; idx += blockDim.x) {
    const int bl = idx / FE, c = idx - bl * FE;
    const int f = c / E, e = c - f * E;
    const long long b = b0 + bl;
    X0[f * kCinP + bl * E + e] = b < B ? x0[b * ld + x_col0 + c] : 0.f;
  }
}

// rows [r0, r0 + nr) of W [K][H] into LDS [nr][pitch], zero past K and past H
__device__ __forceinline__ void cin_stage(float* ch, const float* __restrict__ W, int H, int K, int r0, int nr,
                                          int pitch) {
  for (int idx = threadIdx.x; idx < nr * pitch; idx += blockDim.x) {
    const int r = idx / pitch, h = idx - r * pitch;
    ch[idx] = (r0 + r < K && h < H) ? W[(long long)(r0 + r) * H + h] : 0.f;
  }
}

// out[h][col] = sum_kk W[kk][h] Xp[i][col] X0[j][col] for the unit's columns; all threads call it; ends
// on a barrier.  out is neither Xp nor X0.
__device__ __forceinline__ void cin_layer(const float* Xp, int Hp, const float* X0, int F,
                                          const float* __restrict__ W, int Hk, float* out, float* ch, int wfloats) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6, g = lane >> 4;
  const int K = Hp * F, HP = cin_hp(Hk), MT = (Hk + 15) >> 4, nitems = MT * kCinNCT;
  const int KC = (wfloats / HP) & ~3;
  cin_f4 acc[2] = {cin_f4{0.f, 0.f, 0.f, 0.f}, cin_f4{0.f, 0.f, 0.f, 0.f}};
  for (int kk0 = 0; kk0 < K; kk0 += KC) {
    const int left = (K - kk0 + 3) & ~3, nr = left < KC ? left : KC;
    __syncthreads();
    cin_stage(ch, W, Hk, K, kk0, nr, HP);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int item = wid + q * nw;
      if (item < nitems) {
        const int ct = item % kCinNCT, mt = item / kCinNCT;
        const int col = 16 * ct + (lane & 15);
        int kk = kk0 + g, i = kk / F, j = kk - i * F;
        const float* ap = ch + g * HP + 16 * mt + (lane & 15);
        cin_f4 a = acc[q];
        for (int ks = 0; ks < (nr >> 2); ++ks) {
          const float zv = kk < K ? Xp[i * kCinP + col] * X0[j * kCinP + col] : 0.f;
          a = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * ks * HP], zv, a, 0, 0, 0);
          kk += 4, j += 4;
          while (j >= F) j -= F, ++i;
        }
        acc[q] = a;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int item = wid + q * nw;
    if (item < nitems) {
      const int ct = item % kCinNCT, mt = item / kCinNCT;
      const int col = 16 * ct + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = 16 * mt + 4 * g + r;
        if (h < Hk) out[h * kCinP + col] = acc[q][r];
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kCinFwdThreads) void cin_fwd_kernel(CinPlan P, int B, const float* __restrict__ x0,
                                                                 int ld, int x_col0, const float* __restrict__ prm,
                                                                 const float* __restrict__ z_add,
                                                                 float* __restrict__ z_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int E = P.E, F = P.F, spu = kCinNC / E, tid = threadIdx.x;
  const long long nunits = ((long long)B + spu - 1) / spu;
  float* X0 = lds + P.o_x[0];
  float* scr = lds + P.o_s;
  for (long long u = blockIdx.x; u < nunits; u += gridDim.x) {
    const long long b0 = u * spu;
    __syncthreads();
    cin_load_x0(X0, x0, ld, x_col0, b0, B, F, E);
    // (cin_layer's first barrier orders the map before its first read)
    float zs = 0.f;   // thread col < kCinNC: sum_k sum_h c[off_k + h] X^k[h][col]
    const float* Xp = X0;
    for (int k = 0; k < P.L; ++k) {
      float* out = lds + ((k & 1) ? P.o_b : P.o_a);
      cin_layer(Xp, P.H[k], X0, F, prm + P.woff[k], P.H[k + 1], out, lds + P.o_w, P.wfloats);
      if (tid < kCinNC) {
        const float* c = prm + P.coff[k];
        for (int h = 0; h < P.H[k + 1]; ++h) zs = __builtin_fmaf(c[h], out[h * kCinP + tid], zs);
      }
      Xp = out;
    }
    if (tid < kCinNC) scr[tid] = zs;
    __syncthreads();
    if (tid < spu && b0 + tid < B) {
      float z = 0.f;
      for (int e = 0; e < E; ++e) z += scr[tid * E + e];
      z_out[b0 + tid] = z_add ? z + z_add[b0 + tid] : z;
    }
  }
}

// dW^k tiles of the unit into the block's slab row (sw = the row's W^k part, [K][Hk]): stored by the
// block's first unit, added to by the later ones.  Reads LDS only; no barrier.
__device__ __forceinline__ void cin_dw(const float* Xp, int Hp, const float* X0, int F, const float* D, int Hk,
                                       float* __restrict__ sw, bool first) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6, g = lane >> 4;
  const int K = Hp * F, MT = (Hk + 15) >> 4, NT = (K + 15) >> 4;
  for (int it = wid; it < MT * NT; it += nw) {
    const int mt = it % MT, t = it / MT;
    const int kk = 16 * t + (lane & 15);
    const bool valid = kk < K;
    const int kc = valid ? kk : 0, i = kc / F, j = kc - i * F;
    const int ha = 16 * mt + (lane & 15);
    const bool hok = ha < Hk;
    const float* dp = D + (hok ? ha : 0) * kCinP + g;
    const float* xp = Xp + i * kCinP + g;
    const float* xj = X0 + j * kCinP + g;
    cin_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < kCinNC / 4; ++ks) {
      const float av = hok ? dp[4 * ks] : 0.f;
      const float bv = valid ? xp[4 * ks] * xj[4 * ks] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
    if (valid) {
      float* o = sw + (long long)kk * Hk;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = 16 * mt + 4 * g + r;
        if (h < Hk) o[h] = first ? acc[r] : o[h] + acc[r];
      }
    }
  }
}

// dZ = W^k^T D^k, never stored: nxt[i][col] = (cp ? dzc[col] cp[i] : 0) + sum_j dZ[(i, j)][col] X0[j][col], and
// dx0[(b, e) of col][j] += sum_i dZ[(i, j)][col] Xp[i][col]; with to_dx (k = 1) nxt is added into dx0 too.
// All threads call it; ends on a barrier.
__device__ __forceinline__ void cin_dz(const float* Xp, int Hp, const float* X0, int F, const float* __restrict__ W,
                                       int Hk, const float* D, float* nxt, const float* __restrict__ cp,
                                       const float* dzc, bool to_dx, float* ch, int wfloats,
                                       float* __restrict__ dx0, int dx_ld, int dx_col0, long long b0, int B, int E) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6, g = lane >> 4;
  const int K = Hp * F, KS = (Hk + 3) >> 2, HQ = cin_hq(Hk), JT = (F + 15) >> 4;
  const int ct = wid % kCinNCT, q = wid / kCinNCT, nq = nw / kCinNCT;
  const int col = 16 * ct + (lane & 15);
  float dreg[kCinMaxH / 4];   // the B operand: D[h = 4 ks + g][col]
#pragma unroll
  for (int ks = 0; ks < kCinMaxH / 4; ++ks) {
    const int h = 4 * ks + g;
    dreg[ks] = (ks < KS && h < Hk) ? D[h * kCinP + col] : 0.f;
  }
  cin_f4 dxa[4];   // dX^0's share: rows j = 16 jt + 4 g + r of this lane's column
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) dxa[jt] = cin_f4{0.f, 0.f, 0.f, 0.f};
  const int IG = wfloats / (F * HQ);
  for (int i0 = 0; i0 < Hp; i0 += IG) {
    const int ni = Hp - i0 < IG ? Hp - i0 : IG;
    __syncthreads();
    cin_stage(ch, W, Hk, K, i0 * F, ni * F, HQ);
    __syncthreads();
    for (int i = i0 + q; i < i0 + ni; i += nq) {
      const float xpv = Xp[i * kCinP + col];
      float gs = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        if (jt < JT) {
          const int jrow = 16 * jt + (lane & 15);
          const bool jok = jrow < F;
          const float* ap = ch + ((i - i0) * F + (jok ? jrow : 0)) * HQ + g;
          cin_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < kCinMaxH / 4; ++ks) {
            if (ks < KS) {
              const float av = jok ? ap[4 * ks] : 0.f;
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, dreg[ks], acc, 0, 0, 0);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = 16 * jt + 4 * g + r;
            if (j < F) {
              gs = __builtin_fmaf(acc[r], X0[j * kCinP + col], gs);
              dxa[jt][r] = __builtin_fmaf(acc[r], xpv, dxa[jt][r]);
            }
          }
        }
      }
      gs += __shfl_xor(gs, 16, 64);
      gs += __shfl_xor(gs, 32, 64);
      if (g == 0) nxt[i * kCinP + col] = cp ? __builtin_fmaf(dzc[col], cp[i], gs) : gs;
    }
  }
  __syncthreads();
  // the column tile's waves add their shares in wave order
  const int bl = col / E, e = col - bl * E;
  const long long b = b0 + bl;
  float* drow = dx0 + (b < B ? b : 0) * dx_ld + dx_col0 + e;
  for (int qq = 0; qq < nq; ++qq) {
    if (q == qq && b < B) {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * jt + 4 * g + r;
          if (jt < JT && j < F) drow[j * E] += dxa[jt][r];
        }
      }
    }
    __syncthreads();
  }
  if (to_dx) {
    const int FE = F * E;
    for (int idx = threadIdx.x; idx < F * kCinNC; idx += blockDim.x) {
      const int sl = idx / FE, c = idx - sl * FE;
      const int f = c / E, ee = c - f * E;
      if (b0 + sl < B) dx0[(b0 + sl) * dx_ld + dx_col0 + c] += nxt[f * kCinP + sl * E + ee];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCinBwdThreads) void cin_bwd_kernel(CinPlan P, int B, const float* __restrict__ x0,
                                                                 int ld, int x_col0, const float* __restrict__ prm,
                                                                 const float* __restrict__ dz,
                                                                 float* __restrict__ dx0, int dx_ld, int dx_col0,
                                                                 float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int E = P.E, F = P.F, L = P.L, spu = kCinNC / E, tid = threadIdx.x;
  const long long nunits = ((long long)B + spu - 1) / spu;
  float* X0 = lds + P.o_x[0];
  float* dzc = lds + P.o_s;
  float* ch = lds + P.o_w;
  float* srow = slab + (long long)blockIdx.x * P.npar;
  // thread tid < SH owns dc[tid]: its layer and row
  int ck = -1, chh = 0;
  for (int k = 0; k < L; ++k)
    if (tid >= P.coff[k] && tid < P.coff[k] + P.H[k + 1]) ck = k, chh = tid - P.coff[k];
  float dcacc = 0.f;
  for (long long u = blockIdx.x; u < nunits; u += gridDim.x) {
    const long long b0 = u * spu;
    const bool first = u == blockIdx.x;
    __syncthreads();
    cin_load_x0(X0, x0, ld, x_col0, b0, B, F, E);
    if (tid < kCinNC) {
      const long long b = b0 + tid / E;
      dzc[tid] = b < B ? dz[b] : 0.f;
    }
    // the forward again: X^1 .. X^{L-1} kept, X^L in map a for dc alone
    for (int k = 0; k < L; ++k) {
      float* out = k + 1 < L ? lds + P.o_x[k + 1] : lds + P.o_a;
      cin_layer(lds + P.o_x[k], P.H[k], X0, F, prm + P.woff[k], P.H[k + 1], out, ch, P.wfloats);
      if (ck == k) {
        float s = 0.f;
        for (int c = 0; c < kCinNC; ++c) s = __builtin_fmaf(dzc[c], out[chh * kCinP + c], s);
        dcacc += s;
      }
    }
    __syncthreads();
    float* cur = lds + P.o_a;
    float* nxt = lds + P.o_b;
    {   // D^L = dz c
      const int HL = P.H[L];
      const float* c = prm + P.coff[L - 1];
      for (int idx = tid; idx < HL * kCinNC; idx += blockDim.x) {
        const int h = idx / kCinNC, col = idx - h * kCinNC;
        cur[h * kCinP + col] = dzc[col] * c[h];
      }
    }
    __syncthreads();
    for (int k = L - 1; k >= 0; --k) {
      const float* Xp = lds + P.o_x[k];
      cin_dw(Xp, P.H[k], X0, F, cur, P.H[k + 1], srow + P.woff[k], first);
      cin_dz(Xp, P.H[k], X0, F, prm + P.woff[k], P.H[k + 1], cur, nxt, k > 0 ? prm + P.coff[k - 1] : nullptr, dzc,
             k == 0, ch, P.wfloats, dx0, dx_ld, dx_col0, b0, B, E);
      float* t = cur;
      cur = nxt, nxt = t;
    }
  }
  if (tid < P.SH) srow[tid] = dcacc;
}

// the f32 matrix-rate yardstick: 8 independent accumulator chains of v_mfma_f32_16x16x4_f32 a wave
__global__ __launch_bounds__(256) void mfma_f32_probe_kernel(float* __restrict__ out, int iters) {
  const float a = 1.f + 1e-6f * threadIdx.x, b = 1e-3f * (threadIdx.x & 7);
  cin_f4 acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = cin_f4{(float)q, 0.f, 0.f, 0.f};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[q], 0, 0, 0);
  }
  cin_f4 t = acc[0];
#pragma unroll
  for (int q = 1; q < 8; ++q) t += acc[q];
  out[(long long)blockIdx.x * blockDim.x + threadIdx.x] = t[0] + t[1] + t[2] + t[3];
}

}  // namespace dl

using namespace dl;

extern "C" int dl_mfma_f32_probe(float* out, int64_t n_out, int32_t blocks, int32_t iters, void* stream) {
  DL_CHECK_ARG(out && blocks >= 1 && iters >= 1 && n_out >= (int64_t)blocks * 256,
               "dl_mfma_f32_probe: out needs %lld floats", (long long)blocks * 256);
  hipLaunchKernelGGL(mfma_f32_probe_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), out, iters);
  DL_RETURN_LAUNCH("dl_mfma_f32_probe");
}

extern "C" int dl_cin_grid(int32_t B) {
  // one slab row per block, a block at least 4 samples, at most 128 rows: with at most 262,144 weights the
  // slab dl_adam_dense sums stays within 128 MB whatever the batch
  int g = (B + 3) / 4;
  if (g > kCinBwdGrid) g = kCinBwdGrid;
  return g < 1 ? 1 : g;
}

static int cin_check(const char* name, CinPlan& P, bool bwd, int32_t B, int32_t F, int32_t E, int32_t L,
                     const int32_t* layers, const float* x0, int32_t ld, int32_t x_col0, const float* prm) {
  DL_CHECK_ARG(B >= 0, "%s: B %d < 0", name, B);
  DL_CHECK_ARG(F >= 2 && F <= kCinMaxF, "%s: F %d fields not in [2, %d]", name, F, kCinMaxF);
  DL_CHECK_ARG(E == 8 || E == 16 || E == 32, "%s: E %d not one of 8, 16, 32", name, E);
  DL_CHECK_ARG(L >= 1 && L <= kCinMaxL && layers, "%s: L %d layers not in [1, %d]", name, L, kCinMaxL);
  long long nw = 0;
  for (int k = 0, hp = F; k < L; hp = layers[k], ++k) {
    DL_CHECK_ARG(layers[k] >= 1 && layers[k] <= kCinMaxH, "%s: H %d feature maps of layer %d not in [1, %d]", name,
                 layers[k], k, kCinMaxH);
    nw += (long long)layers[k] * hp * F;
  }
  DL_CHECK_ARG(nw <= kCinMaxW, "%s: %lld layer weights, more than %d", name, nw, kCinMaxW);
  DL_CHECK_ARG(x0 && prm && x_col0 >= 0 && (long long)x_col0 + (long long)F * E <= ld,
               "%s: x0 and params required, field columns [%d, %d) within ld %d", name, x_col0, x_col0 + F * E, ld);
  DL_CHECK_ARG(cin_plan(P, F, E, L, layers, bwd) && P.lds_bytes <= kCinLds, "%s: shape does not fit", name);
  return 0;
}

extern "C" int dl_cin_fwd(int32_t B, int32_t F, int32_t E, int32_t L, const int32_t* layers, const float* x0,
                          int32_t ld, int32_t x_col0, const float* params, const float* z_add, float* z_out,
                          void* stream) {
  CinPlan P;
  if (int rc = cin_check("dl_cin_fwd", P, false, B, F, E, L, layers, x0, ld, x_col0, params)) return rc;
  DL_CHECK_ARG(z_out, "dl_cin_fwd: z_out required");
  if (B == 0) return 0;
  const int spu = kCinNC / E;
  long long grid = ((long long)B + spu - 1) / spu;
  if (grid > kCinFwdGrid) grid = kCinFwdGrid;
  hipLaunchKernelGGL(cin_fwd_kernel, dim3((unsigned)grid), dim3(kCinFwdThreads), P.lds_bytes, as_stream(stream), P, B,
                     x0, ld, x_col0, params, z_add, z_out);
  DL_RETURN_LAUNCH("dl_cin_fwd");
}

extern "C" int dl_cin_bwd(int32_t B, int32_t F, int32_t E, int32_t L, const int32_t* layers, const float* x0,
                          int32_t ld, int32_t x_col0, const float* params, const float* dz, float* dx0,
                          int32_t dx_ld, int32_t dx_col0, float* slab, int32_t slab_rows, void* stream) {
  CinPlan P;
  if (int rc = cin_check("dl_cin_bwd", P, true, B, F, E, L, layers, x0, ld, x_col0, params)) return rc;
  DL_CHECK_ARG(dz && dx0 && slab, "dl_cin_bwd: dz, dx0 and slab required");
  DL_CHECK_ARG(dx_col0 >= 0 && (long long)dx_col0 + (long long)F * E <= dx_ld,
               "dl_cin_bwd: dx0 columns [%d, %d) outside dx_ld %d", dx_col0, dx_col0 + F * E, dx_ld);
  const int grid = dl_cin_grid(B);
  DL_CHECK_ARG(slab_rows >= grid, "dl_cin_bwd: slab needs %d rows", grid);
  if (B == 0) return 0;
  hipLaunchKernelGGL(cin_bwd_kernel, dim3(grid), dim3(kCinBwdThreads), P.lds_bytes, as_stream(stream), P, B, x0, ld,
                     x_col0, params, dz, dx0, dx_ld, dx_col0, slab);
  DL_RETURN_LAUNCH("dl_cin_bwd");
}
