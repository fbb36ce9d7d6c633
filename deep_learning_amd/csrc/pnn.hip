// Inner-product PNN: the product layer's quadratic term added to the dnn_* tower's first layer.
//
// Reference: test_model/PNN.py:78-83 (use_inner) on the F embedded fields of the tower input x0
// (columns [x_col0, x_col0 + F E), E floats a field), theta [D1][F]:
//   T_i = sum_f theta[i][f] e_f;  lp_i = sqrt(sum_e T_i[e]^2);  h0 = relu(x0 W_0 + b_0 + lp)
// The tower's first layer has stored x0 W_0 + b_0 in C (epi 0); dl_pnn_inner_fwd finishes it in place.
// Backward, d = dL/d(pre-activation) = the ReluGrad-masked dh[0]:
//   dT_i = d_i T_i / lp_i (0 where lp_i == 0);  dtheta[i][f] = sum_b sum_e dT_i[e] e_f[e];
//   de_f += sum_i theta[i][f] dT_i
//
// Mapping (v_mfma_f32_16x16x4_f32: exact f32, a k-ordered fma chain).  The accumulator tile holds
// T^T: its 16 rows are (sample, e) — two samples at E = 8, one at 16, two tiles a sample at 32 —
// its 16 columns hidden units, k = the field (zero-padded to 4).  A = x0's fields, one register a
// k-step a lane (A[row = lane & 15][k = lane >> 4]); B = theta from LDS (B[k][col = lane & 15],
// staged once per block and D1-chunk as [i][P], P / 4 odd: conflict-free).  A lane then holds 4
// consecutive e of one hidden unit, so the sum of squares over e is 4 fmas in registers and one
// (E = 8) or two lane-xor adds, in a fixed order; T never leaves the registers.
//   forward: a wave owns a sample unit (16 or 32 rows) and walks the column tiles; the lane group
//     that owns (sample, 16 columns) adds lp into C, applies the ReLU and writes the 16 sign bits
//     as one halfword (a ballot).
//   backward: the block owns the sample unit, wave w the column tiles w, w + nw, ...
//     dtheta^T[f][i] = sum_(b,e) e_f[e] dT[(b,e)][i] sums over the tile's ROW index, so the scaled
//     accumulator registers are the B operand as they stand (k-step s takes register s: k = lane >> 4
//     is row 4 (lane >> 4) + s; the A operand is loaded from x0 in that order); its accumulators stay
//     in registers over all the block's samples and leave as one slab row per block.
//     de[(b,e)][f] = sum_i dT[(b,e)][i] theta[i][f] sums over the COLUMN index: one transpose of the
//     4 registers through a wave-private LDS tile.  The waves' de tiles are added in wave order from
//     LDS and added into dx0 with whole-row accesses.
// No atomics, no memset; the same inputs give the same bits on every run.
#include <math.h>

#include "common.h"

namespace dl {

typedef float pnn_f4 __attribute__((ext_vector_type(4)));

constexpr int kPnnMaxF = 64;
constexpr int kPnnLds = 65536;          // dynamic LDS a block may take
constexpr int kPnnBwdTiles = 4;         // column tiles a backward wave owns per D1-chunk
constexpr int kPnnTP = 20;              // pitch of the transpose tile (16-B aligned rows, conflict-free)

__host__ __device__ __forceinline__ int pnn_pitch(int F) {   // theta's LDS pitch: >= F rounded to 4, P / 4 odd
  const int f4 = (F + 3) & ~3;
  return (f4 & 4) ? f4 : f4 + 4;
}

__device__ __forceinline__ void pnn_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS accesses landed
  __builtin_amdgcn_wave_barrier();
}

// theta rows [i0, i0 + rows) into LDS [rows][P], zero past D1 and past F
__device__ __forceinline__ void pnn_stage(float* ths, const float* __restrict__ theta, int D1, int F, int P, int i0,
                                          int rows) {
  for (int idx = threadIdx.x; idx < rows * P; idx += blockDim.x) {
    const int i = idx / P, f = idx - i * P;
    ths[idx] = (i0 + i < D1 && f < F) ? theta[(long long)(i0 + i) * F + f] : 0.f;
  }
}

// the unit's fields as the A operand of T: xa[mt][ks] = x0[(b, e) = row 16 mt + (lane & 15)][f = 4 ks + (lane >> 4)]
template <int E, int MT, int KSM>
__device__ __forceinline__ void pnn_load_a(float (&xa)[MT][KSM], const float* __restrict__ x0, int ld, int x_col0,
                                           long long b0, int B, int F, int lane) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = 16 * mt + (lane & 15);
    const long long b = b0 + row / E;
    const float* p = x0 + (b < B ? b : 0) * ld + x_col0 + row % E;
#pragma unroll
    for (int ks = 0; ks < KSM; ++ks) {
      const int f = 4 * ks + (lane >> 4);
      xa[mt][ks] = (b < B && f < F) ? p[f * E] : 0.f;
    }
  }
}

// one column tile of T^T (rows (b, e), columns i = 16 nt + (lane & 15)) and lp^2 of this lane's
// (sample, column): the squares summed over the lane's 4 rows, then over the sample's lane groups
template <int E, int MT, int KSM>
__device__ __forceinline__ float pnn_tile(const float (&xa)[MT][KSM], const float* ths, int P, int KS, int nt,
                                          int lane, pnn_f4 (&acc)[MT]) {
  const float* tb = ths + (16 * nt + (lane & 15)) * P + (lane >> 4);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = pnn_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KSM; ++ks) {
    if (ks < KS) {
      const float bv = tb[4 * ks];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[mt][ks], bv, acc[mt], 0, 0, 0);
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ss = __builtin_fmaf(acc[mt][r], acc[mt][r], ss);
  }
  ss += __shfl_xor(ss, 16, 64);
  if (E >= 16) ss += __shfl_xor(ss, 32, 64);
  return ss;
}

template <int E, int FT>
__global__ __launch_bounds__(256) void pnn_fwd_kernel(int B, int F, int D1, int DC, const float* __restrict__ x0,
                                                      int ld, int x_col0, const float* __restrict__ theta,
                                                      float* __restrict__ C, int ldc, uint16_t* __restrict__ bits,
                                                      int ldbits) {
  constexpr int MT = E == 32 ? 2 : 1, KSM = 4 * FT, SPU = 16 * MT / E;
  extern __shared__ __attribute__((aligned(16))) float lds[];   // theta chunk [DC][P]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6, g = lane >> 4;
  const int P = pnn_pitch(F), KS = (F + 3) >> 2;
  const long long nunits = ((long long)B + SPU - 1) / SPU;
  // the lane group that writes (sample, 16 columns), and its sample within the unit
  const bool writer = E == 8 ? (g & 1) == 0 : g == 0;
  const int sl = E == 8 ? g >> 1 : 0;
  for (int i0 = 0; i0 < D1; i0 += DC) {
    const int rows = min(DC, (D1 - i0 + 15) & ~15);
    __syncthreads();
    pnn_stage(lds, theta, D1, F, P, i0, rows);
    __syncthreads();
    const int NT = rows >> 4;
    for (long long u = (long long)blockIdx.x * nw + wid; u < nunits; u += (long long)gridDim.x * nw) {
      float xa[MT][KSM];
      pnn_load_a<E, MT, KSM>(xa, x0, ld, x_col0, u * SPU, B, F, lane);
      const long long b = u * SPU + sl;
      const bool rowok = writer && b < B;
      float* crow = C + (rowok ? b : 0) * ldc;
      int i = i0 + (lane & 15);
      float cnext = rowok && i < D1 ? crow[i] : 0.f;
      for (int nt = 0; nt < NT; ++nt, i += 16) {
        const float cv = cnext;
        if (nt + 1 < NT) cnext = rowok && i + 16 < D1 ? crow[i + 16] : 0.f;
        pnn_f4 acc[MT];
        const float lp = sqrtf(pnn_tile<E, MT, KSM>(xa, lds, P, KS, nt, lane, acc));
        const bool ok = rowok && i < D1;
        const float pre = cv + lp;
        if (ok) crow[i] = fmaxf(pre, 0.f);
        if (bits) {
          const unsigned long long m = __ballot(ok && pre > 0.f);
          if (rowok && (lane & 15) == 0) bits[b * ldbits + ((i0 >> 4) + nt)] = (uint16_t)((m >> (16 * g)) & 0xffffu);
        }
      }
    }
  }
}

template <int E, int FT>
__global__ __launch_bounds__(512) void pnn_bwd_kernel(int B, int F, int D1, int DC, const float* __restrict__ x0,
                                                      int ld, int x_col0, const float* __restrict__ theta,
                                                      const float* __restrict__ d, int ldd, float* __restrict__ dx0,
                                                      int dx_ld, int dx_col0, float* __restrict__ slab) {
  constexpr int MT = E == 32 ? 2 : 1, KSM = 4 * FT, SPU = 16 * MT / E, NTW = kPnnBwdTiles;
  constexpr int FP = 16 * FT + 1;                                    // pitch of a wave's de tile
  constexpr int WS = 16 * MT * FP > MT * 16 * kPnnTP ? 16 * MT * FP : MT * 16 * kPnnTP;   // floats a wave owns
  // per wave: the transpose tiles [MT][16][kPnnTP], later its de tile [16 MT][FP] | theta chunk [DC][P]
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6, g = lane >> 4;
  float* wbuf = lds + wid * WS;
  float* ths = lds + nw * WS;
  const int P = pnn_pitch(F), KS = (F + 3) >> 2;
  const long long nunits = ((long long)B + SPU - 1) / SPU;
  const int sl = E == 8 ? g >> 1 : 0;
  const long long n = (long long)D1 * F;
  float* out = slab + (long long)blockIdx.x * n;
  for (int i0 = 0; i0 < D1; i0 += DC) {
    const int rows = min(DC, (D1 - i0 + 15) & ~15);
    __syncthreads();
    pnn_stage(ths, theta, D1, F, P, i0, rows);
    __syncthreads();
    const int NT = rows >> 4;
    pnn_f4 dth[NTW][FT];   // dtheta^T tiles: rows f = 16 ft + 4 g + r, column i = 16 nt + (lane & 15)
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) dth[j][ft] = pnn_f4{0.f, 0.f, 0.f, 0.f};
    }
    for (long long u = blockIdx.x; u < nunits; u += gridDim.x) {
      const long long b0 = u * SPU;
      float xa[MT][KSM];
      pnn_load_a<E, MT, KSM>(xa, x0, ld, x_col0, b0, B, F, lane);
      // the A operand of dtheta^T: xt[mt][ft][s] = x0[(b, e) = row 16 mt + 4 g + s][f = 16 ft + (lane & 15)]
      float xt[MT][FT][4];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int row = 16 * mt + 4 * g;   // 4 consecutive e of one sample
        const long long b = b0 + row / E;
        const float* p = x0 + (b < B ? b : 0) * ld + x_col0 + row % E;
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) {
          const int f = 16 * ft + (lane & 15);
#pragma unroll
          for (int s = 0; s < 4; ++s) xt[mt][ft][s] = (b < B && f < F) ? p[f * E + s] : 0.f;
        }
      }
      const long long b = b0 + sl;
      pnn_f4 de[MT][FT];   // rows (b, e) = 16 mt + 4 g + r, column f = 16 ft + (lane & 15)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) de[mt][ft] = pnn_f4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        const int nt = wid + j * nw;
        if (nt < NT) {
          pnn_f4 acc[MT];
          const float ss = pnn_tile<E, MT, KSM>(xa, ths, P, KS, nt, lane, acc);
          const float lp = sqrtf(ss);
          const int i = i0 + 16 * nt + (lane & 15);
          const float dv = (b < B && i < D1) ? d[b * ldd + i] : 0.f;
          const float sc = lp > 0.f ? dv / lp : 0.f;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            acc[mt] *= sc;   // dT
            *reinterpret_cast<pnn_f4*>(wbuf + (mt * 16 + (lane & 15)) * kPnnTP + 4 * g) = acc[mt];
          }
          // dtheta^T += X^T dT: k = the tile's rows, register s of every lane group in k-step s
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
              for (int s = 0; s < 4; ++s)
                dth[j][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(xt[mt][ft][s], acc[mt][s], dth[j][ft], 0, 0, 0);
            }
          }
          pnn_lds_order();
          // de += dT theta: k = the tile's columns, dT transposed through the wave's LDS tile
          const float* tb = ths + (16 * nt + g) * P + (lane & 15);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            float av[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) av[mt] = wbuf[(mt * 16 + 4 * s + g) * kPnnTP + (lane & 15)];
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
              const float bv = 16 * ft + (lane & 15) < P ? tb[4 * s * P + 16 * ft] : 0.f;
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
                de[mt][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv, de[mt][ft], 0, 0, 0);
            }
          }
          pnn_lds_order();
        }
      }
      // the waves' de tiles, added in wave order, into dx0's rows
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
          for (int r = 0; r < 4; ++r) wbuf[(16 * mt + 4 * g + r) * FP + 16 * ft + (lane & 15)] = de[mt][ft][r];
        }
      }
      __syncthreads();
      const int FE = F * E;
      for (int idx = threadIdx.x; idx < SPU * FE; idx += blockDim.x) {
        const int bl = idx / FE, c = idx - bl * FE;
        if (b0 + bl < B) {
          const int f = c / E, row = bl * E + (c - f * E);
          float t = lds[row * FP + f];
          for (int w = 1; w < nw; ++w) t += lds[w * WS + row * FP + f];
          dx0[(b0 + bl) * dx_ld + dx_col0 + c] += t;
        }
      }
      __syncthreads();
    }
    // this chunk's rows of the block's slab row, in theta's layout
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int nt = wid + j * nw, i = i0 + 16 * nt + (lane & 15);
      if (nt < NT && i < D1) {
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int f = 16 * ft + 4 * g + r;
            if (f < F) out[(long long)i * F + f] = dth[j][ft][r];
          }
        }
      }
    }
  }
}

}  // namespace dl

using namespace dl;

extern "C" int dl_pnn_grid(int32_t B) {
  // at most 512 blocks, as dl_afm_grid: the slab dl_adam_dense sums is bounded whatever the batch
  int g = (B + 15) / 16;
  if (g > 512) g = 512;
  return g < 1 ? 1 : g;
}

static int pnn_check(const char* name, int32_t B, int32_t F, int32_t E, int32_t D1, const float* x0, int32_t ld,
                     int32_t x_col0, const float* theta) {
  DL_CHECK_ARG(B >= 0, "%s: B %d < 0", name, B);
  DL_CHECK_ARG(F >= 2 && F <= kPnnMaxF, "%s: F %d fields not in [2, %d]", name, F, kPnnMaxF);
  DL_CHECK_ARG(E == 8 || E == 16 || E == 32, "%s: E %d not one of 8, 16, 32", name, E);
  DL_CHECK_ARG(D1 >= 1, "%s: D1 %d < 1", name, D1);
  DL_CHECK_ARG(x0 && theta && x_col0 >= 0 && (long long)x_col0 + (long long)F * E <= ld,
               "%s: x0 and theta required, field columns [%d, %d) within ld %d", name, x_col0, x_col0 + F * E, ld);
  return 0;
}

#define DL_PNN_CASES(M) M(8, 1) M(8, 2) M(8, 3) M(8, 4) M(16, 1) M(16, 2) M(16, 3) M(16, 4) M(32, 1) M(32, 2) \
  M(32, 3) M(32, 4)

extern "C" int dl_pnn_inner_fwd(int32_t B, int32_t F, int32_t E, int32_t D1, const float* x0, int32_t ld,
                                int32_t x_col0, const float* theta, float* C, int32_t ldc, uint16_t* bits,
                                int32_t ldbits, void* stream) {
  if (int rc = pnn_check("dl_pnn_inner_fwd", B, F, E, D1, x0, ld, x_col0, theta)) return rc;
  DL_CHECK_ARG(C && ldc >= D1, "dl_pnn_inner_fwd: C required, ldc %d >= D1 %d", ldc, D1);
  DL_CHECK_ARG(!bits || ldbits >= (D1 + 15) / 16, "dl_pnn_inner_fwd: ldbits %d < %d halfwords", ldbits,
               (D1 + 15) / 16);
  if (B == 0) return 0;
  const int P = pnn_pitch(F), nw = 4, FT = (F + 15) / 16;
  // theta's chunk of hidden units: all of D1 (to 16) when it fits the block's LDS
  int DC = (kPnnLds / (P * (int)sizeof(float))) & ~15;
  if (DC > ((D1 + 15) & ~15)) DC = (D1 + 15) & ~15;
  const size_t lds = (size_t)DC * P * sizeof(float);
  const int spu = E == 8 ? 2 : 1;
  long long grid = (((long long)B + spu - 1) / spu + nw - 1) / nw;
  if (grid > 1024) grid = 1024;
#define DL_PNN_FWD(EE, FF)                                                                                      \
  case EE * 8 + FF:                                                                                             \
    hipLaunchKernelGGL((pnn_fwd_kernel<EE, FF>), dim3((unsigned)grid), dim3(64 * nw), lds, as_stream(stream),   \
                       B, F, D1, DC, x0, ld, x_col0, theta, C, ldc, bits, ldbits);                              \
    break;
  switch (E * 8 + FT) { DL_PNN_CASES(DL_PNN_FWD) }
#undef DL_PNN_FWD
  DL_RETURN_LAUNCH("dl_pnn_inner_fwd");
}

extern "C" int dl_pnn_inner_bwd(int32_t B, int32_t F, int32_t E, int32_t D1, const float* x0, int32_t ld,
                                int32_t x_col0, const float* theta, const float* d, int32_t ldd, float* dx0,
                                int32_t dx_ld, int32_t dx_col0, float* slab, int32_t slab_rows, void* stream) {
  if (int rc = pnn_check("dl_pnn_inner_bwd", B, F, E, D1, x0, ld, x_col0, theta)) return rc;
  DL_CHECK_ARG(d && dx0 && slab && ldd >= D1, "dl_pnn_inner_bwd: d, dx0 and slab required, ldd %d >= D1 %d", ldd, D1);
  DL_CHECK_ARG(dx_col0 >= 0 && (long long)dx_col0 + (long long)F * E <= dx_ld,
               "dl_pnn_inner_bwd: dx0 columns [%d, %d) outside dx_ld %d", dx_col0, dx_col0 + F * E, dx_ld);
  const int grid = dl_pnn_grid(B);
  DL_CHECK_ARG(slab_rows >= grid, "dl_pnn_inner_bwd: slab needs %d rows", grid);
  if (B == 0) return 0;
  // 8 waves, or 4 where their de tiles would take more than half the LDS; theta's chunk of hidden
  // units: what the rest holds, at most kPnnBwdTiles column tiles a wave
  const int P = pnn_pitch(F), FT = (F + 15) / 16, MT = E == 32 ? 2 : 1;
  const int de_tile = 16 * MT * (16 * FT + 1), tr_tile = MT * 16 * kPnnTP;
  const int ws = de_tile > tr_tile ? de_tile : tr_tile;
  const int nw = (size_t)8 * ws * sizeof(float) > kPnnLds / 2 ? 4 : 8;
  int DC = ((kPnnLds - nw * ws * (int)sizeof(float)) / (P * (int)sizeof(float))) & ~15;
  if (DC > 16 * nw * kPnnBwdTiles) DC = 16 * nw * kPnnBwdTiles;
  if (DC > ((D1 + 15) & ~15)) DC = (D1 + 15) & ~15;
  const size_t lds = ((size_t)nw * ws + (size_t)DC * P) * sizeof(float);
#define DL_PNN_BWD(EE, FF)                                                                                      \
  case EE * 8 + FF:                                                                                             \
    hipLaunchKernelGGL((pnn_bwd_kernel<EE, FF>), dim3(grid), dim3(64 * nw), lds, as_stream(stream), B, F, D1,   \
                       DC, x0, ld, x_col0, theta, d, ldd, dx0, dx_ld, dx_col0, slab);                           \
    break;
  switch (E * 8 + FT) { DL_PNN_CASES(DL_PNN_BWD) }
#undef DL_PNN_BWD
  DL_RETURN_LAUNCH("dl_pnn_inner_bwd");
}
