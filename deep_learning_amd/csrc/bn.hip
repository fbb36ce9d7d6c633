// Batch normalisation of a hidden layer of the deep tower, between the layer's GEMM and its ReLU.
//
// Reference: test_model/NFM.py:160-167, 244-252 (nn.BatchNorm1d after linear_i, torch's defaults).
// The layer's GEMM has stored the pre-activation c = x W + b in C [B, ldc] (epi 0):
//   training:  mu_j = mean_b c;  var_j = mean_b (c - mu_j)^2 (biased);  xhat = (c - mu) / sqrt(var + eps)
//              y = gamma xhat + beta;  h = relu(y);  running statistics updated (unbiased variance)
//   inference: the same from the running statistics
//   backward, dy = the ReluGrad-masked dh:  dbeta = sum_b dy;  dgamma = sum_b dy xhat
//              dc = gamma / sqrt(var + eps) (dy - dbeta / B - xhat dgamma / B)
//
// Mapping.  Every pass streams whole [B, D] f32 matrices once: bandwidth-bound.  A thread owns one
// group of 4 columns (one 16-B piece of a row) for its whole life, so the per-column constants and
// the column sums live in registers; the groups are padded to whole halfwords of the sign record
// (ngrp = 4 ceil(D / 16)) so the four lanes of a halfword are one aligned lane quad.  A block of 256
// threads is RY = 256 / ngrp row lanes of ngrp groups (D = 400: 2 x 100, 200 threads live): the
// lanes of a row lane read one contiguous piece of a row, 16 B each.  Block b owns the rows
// [b R, (b + 1) R) and walks them RY at a time, 4 rows a thread in flight (200 x 4 x 16 B = 12.8 KB a
// matrix a block).  The grid is at most 1024 blocks (4 a CU) of at least 32 rows: a CU then has 51 KB
// (one matrix) to 102 KB (two) of loads in flight, above the ~32 KB per CU at which the copy
// yardstick's stream saturates HBM, and the backward's slab stays below 7 % of the traffic.
//   statistics: per block the sums of (c - K) and (c - K)^2 with K the block's first row (a sample
//     of the column: the shift keeps both sums at the column's spread, whatever its offset), the row
//     lanes added in order through LDS -> (n, mean, M2) of the block.  A small second kernel (16
//     columns x 16 block lanes a block) merges the blocks in order by Chan's formula in float64,
//     keeps mu as a hi + lo pair of floats and 1 / sqrt(var + eps), and updates the running
//     statistics under the step guard.
//   forward finish: xhat = ((c - mu_hi) - mu_lo) invstd, hx <- xhat (training), C <- relu(y), and the
//     halfword of sign bits from the quad's four nibbles (two lane-xor ors).
//   backward sums: dgamma, dbeta of the block as one slab row (dl_adam_dense's input).
//   backward apply: a second small kernel merges the slab rows in order (float64) into sums; the
//     apply pass rewrites dy in place.
// No atomics, no memset; the same inputs give the same bits on every run.
#include <math.h>

#include "common.h"

namespace dl {

typedef float bn_f4 __attribute__((ext_vector_type(4)));

constexpr int kBnThreads = 256;
constexpr int kBnMaxGrid = 1024;   // 4 blocks a CU
constexpr int kBnMinRows = 32;     // rows a block owns at least
constexpr int kBnUnroll = 4;       // rows a thread keeps in flight

static int bn_rows(int B) {   // rows a block owns
  const int r = (B + kBnMaxGrid - 1) / kBnMaxGrid;
  return r < kBnMinRows ? kBnMinRows : r;
}
static int bn_grid(int B) { return B < 1 ? 1 : (B + bn_rows(B) - 1) / bn_rows(B); }
static int bn_dp(int D) { return (D + 15) / 16 * 16; }

// the column-group geometry of a block: cgw groups x ry row lanes, `chunks` blocks across the columns
struct BnGeo {
  int ngrp, cgw, ry, chunks;
};
static BnGeo bn_geo(int D) {
  BnGeo g;
  g.ngrp = bn_dp(D) / 4;
  g.cgw = g.ngrp < kBnThreads ? g.ngrp : kBnThreads;
  g.ry = kBnThreads / g.cgw;
  g.chunks = (g.ngrp + kBnThreads - 1) / kBnThreads;
  return g;
}

// one thread's place: column group g (nv live columns of its 4), row lane yy
struct BnLane {
  int g, nv, yy;
  bool live;
};
__device__ __forceinline__ BnLane bn_lane(int D, int cgw, int ry) {
  BnLane l;
  const int t = threadIdx.x;
  l.yy = t / cgw;
  l.g = blockIdx.y * kBnThreads + (t - l.yy * cgw);
  const int rest = D - 4 * l.g;
  l.nv = rest < 0 ? 0 : rest > 4 ? 4 : rest;
  l.live = l.yy < ry && l.nv > 0;
  return l;
}

// 4 columns of a row from p (16-B aligned when nv == 4); the columns past D read as 0
__device__ __forceinline__ bn_f4 bn_ld(const float* __restrict__ p, int nv) {
  if (nv == 4) return *reinterpret_cast<const bn_f4*>(p);
  bn_f4 v = {0.f, 0.f, 0.f, 0.f};
  if (nv > 0) v.x = p[0];
  if (nv > 1) v.y = p[1];
  if (nv > 2) v.z = p[2];
  return v;
}
__device__ __forceinline__ void bn_st(float* __restrict__ p, bn_f4 v, int nv) {
  if (nv == 4) {
    *reinterpret_cast<bn_f4*>(p) = v;
    return;
  }
  if (nv > 0) p[0] = v.x;
  if (nv > 1) p[1] = v.y;
  if (nv > 2) p[2] = v.z;
}
// nv floats of a vector of any alignment (once a thread)
__device__ __forceinline__ bn_f4 bn_ld_vec(const float* __restrict__ p, int nv) {
  bn_f4 v = {0.f, 0.f, 0.f, 0.f};
  if (nv > 0) v.x = p[0];
  if (nv > 1) v.y = p[1];
  if (nv > 2) v.z = p[2];
  if (nv > 3) v.w = p[3];
  return v;
}

// the row lanes' partial sums of one column group added in lane order; row lane 0 gets the total
__device__ __forceinline__ bn_f4 bn_fold(bn_f4* sh, bn_f4 v, const BnLane& l, int cgw, int ry) {
  sh[threadIdx.x] = v;
  __syncthreads();
  if (l.yy == 0)
    for (int y = 1; y < ry; ++y) v += sh[y * cgw + threadIdx.x];
  __syncthreads();
  return v;
}

// ---------------------------------------------------------------------------
// statistics, pass 1: part[block][3][Dp] = {K, sum (c - K), sum (c - K)^2} over the block's rows
__global__ __launch_bounds__(kBnThreads) void bn_stats_part_kernel(const float* __restrict__ C, int ldc, int B, int D,
                                                                   int R, int cgw, int ry, int Dp,
                                                                   float* __restrict__ part) {
  __shared__ bn_f4 sh[kBnThreads];
  const BnLane l = bn_lane(D, cgw, ry);
  const int r0 = blockIdx.x * R, r1 = min(B, r0 + R);
  bn_f4 K = {0.f, 0.f, 0.f, 0.f}, s1 = K, s2 = K;
  if (l.live) {
    const float* col = C + 4 * l.g;
    K = bn_ld(col + (long long)r0 * ldc, l.nv);
    for (int r = r0 + l.yy; r < r1; r += ry * kBnUnroll) {
      bn_f4 v[kBnUnroll];
#pragma unroll
      for (int u = 0; u < kBnUnroll; ++u)
        if (r + u * ry < r1) v[u] = bn_ld(col + (long long)(r + u * ry) * ldc, l.nv);
#pragma unroll
      for (int u = 0; u < kBnUnroll; ++u)
        if (r + u * ry < r1) {
          const bn_f4 d = v[u] - K;
          s1 += d;
          s2 += d * d;
        }
    }
  }
  s1 = bn_fold(sh, s1, l, cgw, ry);
  s2 = bn_fold(sh, s2, l, cgw, ry);
  if (l.yy == 0 && 4 * l.g < Dp) {
    float* o = part + (long long)blockIdx.x * 3 * Dp + 4 * l.g;
    *reinterpret_cast<bn_f4*>(o) = K;
    *reinterpret_cast<bn_f4*>(o + Dp) = s1;
    *reinterpret_cast<bn_f4*>(o + 2 * Dp) = s2;
  }
}

// (n, mean, M2) <- merged with (nb, mb, Mb)
__device__ __forceinline__ void bn_chan(double& n, double& mean, double& M2, double nb, double mb, double Mb) {
  if (nb == 0.0) return;
  const double nn = n + nb, delta = mb - mean, f = nb / nn;
  mean += delta * f;
  M2 += Mb + delta * delta * n * f;
  n = nn;
}

// statistics, pass 2: 16 columns x 16 block lanes a block; block lane k merges its run of blocks in
// order, lane 0 then the 16 runs in order
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ part, int G, int R, int B, int D,
                                                             int Dp, float eps, float momentum,
                                                             float* __restrict__ stat, float* __restrict__ run_mean,
                                                             float* __restrict__ run_var,
                                                             const float* __restrict__ opt) {
  __shared__ double sn[256], sm[256], sM[256];
  const int jl = threadIdx.x & 15, bl = threadIdx.x >> 4;
  const int j = blockIdx.x * 16 + jl;
  const int run = (G + 15) / 16;
  double n = 0.0, mean = 0.0, M2 = 0.0;
  if (j < D) {
    const int b1 = min(G, (bl + 1) * run);
    for (int b = bl * run; b < b1; ++b) {
      const float* p = part + (long long)b * 3 * Dp + j;
      const double nb = (double)(min(B, (b + 1) * R) - b * R);
      const double K = p[0], s1 = p[Dp], s2 = p[2 * Dp];
      const double Mb = s2 - s1 * s1 / nb;
      bn_chan(n, mean, M2, nb, K + s1 / nb, Mb > 0.0 ? Mb : 0.0);
    }
  }
  sn[threadIdx.x] = n;
  sm[threadIdx.x] = mean;
  sM[threadIdx.x] = M2;
  __syncthreads();
  if (bl != 0) return;
  for (int k = 1; k < 16; ++k) bn_chan(n, mean, M2, sn[k * 16 + jl], sm[k * 16 + jl], sM[k * 16 + jl]);
  if (j >= D) {   // the pad columns of stat read as zeros
    stat[j] = 0.f;
    stat[Dp + j] = 0.f;
    stat[2 * Dp + j] = 0.f;
    return;
  }
  const double var = M2 / (double)B;
  const float hi = (float)mean;
  stat[j] = hi;
  stat[Dp + j] = (float)(mean - (double)hi);
  stat[2 * Dp + j] = (float)(1.0 / sqrt(var + (double)eps));
  if (run_mean && !(opt && step_poisoned(opt))) {
    const double m = (double)momentum;
    run_mean[j] = (float)((1.0 - m) * (double)run_mean[j] + m * mean);
    run_var[j] = (float)((1.0 - m) * (double)run_var[j] + m * var * ((double)B / (double)(B - 1)));
  }
}

// ---------------------------------------------------------------------------
// forward finish: C <- relu(gamma xhat + beta); TRAIN: xhat from stat, hx <- xhat; else from the
// running statistics
template <bool TRAIN>
__global__ __launch_bounds__(kBnThreads) void bn_fwd_kernel(float* __restrict__ C, int ldc, int B, int D, int R, int cgw,
                                                            int ry, int Dp, const float* __restrict__ stat,
                                                            const float* __restrict__ run_mean,
                                                            const float* __restrict__ run_var, float eps,
                                                            const float* __restrict__ params, float* __restrict__ hx,
                                                            int ldx, uint16_t* __restrict__ bits, int ldbits) {
  const BnLane l = bn_lane(D, cgw, ry);
  if (l.yy >= ry || 4 * l.g >= Dp) return;   // whole quads leave: cgw and Dp / 4 are multiples of 4
  const int r0 = blockIdx.x * R, r1 = min(B, r0 + R);
  bn_f4 hi, lo = {0.f, 0.f, 0.f, 0.f}, inv;
  if (TRAIN) {
    hi = *reinterpret_cast<const bn_f4*>(stat + 4 * l.g);
    lo = *reinterpret_cast<const bn_f4*>(stat + Dp + 4 * l.g);
    inv = *reinterpret_cast<const bn_f4*>(stat + 2 * Dp + 4 * l.g);
  } else {
    hi = bn_ld_vec(run_mean + 4 * l.g, l.nv);
    const bn_f4 rv = bn_ld_vec(run_var + 4 * l.g, l.nv);
#pragma unroll
    for (int i = 0; i < 4; ++i) inv[i] = (float)(1.0 / sqrt((double)rv[i] + (double)eps));
  }
  const bn_f4 ga = bn_ld_vec(params + 4 * l.g, l.nv), be = bn_ld_vec(params + D + 4 * l.g, l.nv);
  const int q = l.g & 3;
  for (int r = r0 + l.yy; r < r1; r += ry * kBnUnroll) {
    bn_f4 v[kBnUnroll];
#pragma unroll
    for (int u = 0; u < kBnUnroll; ++u)
      if (r + u * ry < r1 && l.nv) v[u] = bn_ld(C + (long long)(r + u * ry) * ldc + 4 * l.g, l.nv);
#pragma unroll
    for (int u = 0; u < kBnUnroll; ++u) {
      const int rr = r + u * ry;
      if (rr >= r1) break;   // (the same for the whole quad: one row lane)
      unsigned m = 0;
      if (l.nv) {
        const bn_f4 xh = ((v[u] - hi) - lo) * inv;
        bn_f4 y, h;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          y[i] = __builtin_fmaf(ga[i], xh[i], be[i]);
          const bool pos = y[i] > 0.f && i < l.nv;
          h[i] = pos ? y[i] : 0.f;
          m |= (pos ? 1u : 0u) << i;
        }
        if (TRAIN) bn_st(hx + (long long)rr * ldx + 4 * l.g, xh, l.nv);
        bn_st(C + (long long)rr * ldc + 4 * l.g, h, l.nv);
      }
      if (bits) {   // the quad's four nibbles -> one halfword
        m <<= 4 * q;
        m |= (unsigned)__shfl_xor((int)m, 1, 64);
        m |= (unsigned)__shfl_xor((int)m, 2, 64);
        if (q == 0) bits[(long long)rr * ldbits + (l.g >> 2)] = (uint16_t)m;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward sums: slab[block] = [sum dy xhat (D) | sum dy (D)] over the block's rows
__global__ __launch_bounds__(kBnThreads) void bn_bwd_sums_kernel(const float* __restrict__ dy, int ldd,
                                                                 const float* __restrict__ hx, int ldx, int B, int D,
                                                                 int R, int cgw, int ry, float* __restrict__ slab) {
  __shared__ bn_f4 sh[kBnThreads];
  const BnLane l = bn_lane(D, cgw, ry);
  const int r0 = blockIdx.x * R, r1 = min(B, r0 + R);
  bn_f4 dg = {0.f, 0.f, 0.f, 0.f}, db = dg;
  if (l.live) {
    for (int r = r0 + l.yy; r < r1; r += ry * kBnUnroll) {
      bn_f4 a[kBnUnroll], x[kBnUnroll];
#pragma unroll
      for (int u = 0; u < kBnUnroll; ++u)
        if (r + u * ry < r1) {
          a[u] = bn_ld(dy + (long long)(r + u * ry) * ldd + 4 * l.g, l.nv);
          x[u] = bn_ld(hx + (long long)(r + u * ry) * ldx + 4 * l.g, l.nv);
        }
#pragma unroll
      for (int u = 0; u < kBnUnroll; ++u)
        if (r + u * ry < r1) {
          dg += a[u] * x[u];
          db += a[u];
        }
    }
  }
  dg = bn_fold(sh, dg, l, cgw, ry);
  db = bn_fold(sh, db, l, cgw, ry);
  if (l.yy == 0 && l.nv) {
    float* o = slab + (long long)blockIdx.x * 2 * D + 4 * l.g;
    for (int i = 0; i < l.nv; ++i) {
      o[i] = dg[i];
      o[D + i] = db[i];
    }
  }
}

// sums [2][Dp] = the slab's rows added in order (float64), zeros in the pad columns
__global__ __launch_bounds__(256) void bn_bwd_merge_kernel(const float* __restrict__ slab, int G, int D, int Dp,
                                                           float* __restrict__ sums) {
  __shared__ double sa[256];
  const int jl = threadIdx.x & 15, bl = threadIdx.x >> 4;
  const int j = blockIdx.x * 16 + jl, which = blockIdx.y;
  const int run = (G + 15) / 16;
  double a = 0.0;
  if (j < D) {
    const int b1 = min(G, (bl + 1) * run);
    for (int b = bl * run; b < b1; ++b) a += (double)slab[(long long)b * 2 * D + which * D + j];
  }
  sa[threadIdx.x] = a;
  __syncthreads();
  if (bl != 0) return;
  for (int k = 1; k < 16; ++k) a += sa[k * 16 + jl];
  sums[which * Dp + j] = (float)a;
}

// backward apply: dy <- gamma invstd (dy - dbeta / B - xhat dgamma / B), in place
__global__ __launch_bounds__(kBnThreads) void bn_bwd_apply_kernel(float* __restrict__ dy, int ldd,
                                                                  const float* __restrict__ hx, int ldx, int B, int D,
                                                                  int R, int cgw, int ry, int Dp,
                                                                  const float* __restrict__ params,
                                                                  const float* __restrict__ stat,
                                                                  const float* __restrict__ sums) {
  const BnLane l = bn_lane(D, cgw, ry);
  if (!l.live) return;
  const int r0 = blockIdx.x * R, r1 = min(B, r0 + R);
  const bn_f4 ga = bn_ld_vec(params + 4 * l.g, l.nv);
  const bn_f4 a = ga * *reinterpret_cast<const bn_f4*>(stat + 2 * Dp + 4 * l.g);
  const float fb = (float)B;
  const bn_f4 mg = *reinterpret_cast<const bn_f4*>(sums + 4 * l.g) / fb;
  const bn_f4 mb = *reinterpret_cast<const bn_f4*>(sums + Dp + 4 * l.g) / fb;
  for (int r = r0 + l.yy; r < r1; r += ry * kBnUnroll) {
    bn_f4 d[kBnUnroll], x[kBnUnroll];
#pragma unroll
    for (int u = 0; u < kBnUnroll; ++u)
      if (r + u * ry < r1) {
        d[u] = bn_ld(dy + (long long)(r + u * ry) * ldd + 4 * l.g, l.nv);
        x[u] = bn_ld(hx + (long long)(r + u * ry) * ldx + 4 * l.g, l.nv);
      }
#pragma unroll
    for (int u = 0; u < kBnUnroll; ++u)
      if (r + u * ry < r1) bn_st(dy + (long long)(r + u * ry) * ldd + 4 * l.g, a * ((d[u] - mb) - x[u] * mg), l.nv);
  }
}

// The layer's own bias under batch norm: dL/db = sum_b dc is 0 identically (the normalisation removes
// any constant added to a column), but the weight gradient's bias row holds the f32 rounding noise of
// that sum, which Adam's m / (sqrt(v) + eps) would turn into steps of the order of lr.  The row of
// every split-K slab is set to the exact value, 0.
__global__ __launch_bounds__(256) void bn_zero_row_kernel(float* __restrict__ slab, int nslab, long long stride,
                                                          long long offset, int cols) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)nslab * cols) return;
  slab[(i / cols) * stride + offset + (i % cols)] = 0.f;
}

static bool bn_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace dl

using namespace dl;

#define DL_BN_CHECK_MATRIX(name, p, ld, D)                                                           \
  DL_CHECK_ARG((ld) >= (D) && (ld) % 4 == 0, "%s: " #ld " %d must be a multiple of 4 and >= D %d", name, ld, D); \
  DL_CHECK_ARG(bn_aligned(p), "%s: " #p " must be 16-B aligned", name)

extern "C" int dl_bn_grid(int32_t B) { return bn_grid(B); }

extern "C" int dl_bn_zero_bias_grad(float* slab, int32_t nslab, int64_t stride, int64_t offset, int32_t cols,
                                    void* stream) {
  DL_CHECK_ARG(slab && nslab >= 1 && cols >= 1, "dl_bn_zero_bias_grad: bad arguments");
  DL_CHECK_ARG(offset >= 0 && offset + cols <= stride, "dl_bn_zero_bias_grad: row [%lld, +%d) past the slab's %lld",
               (long long)offset, cols, (long long)stride);
  const long long n = (long long)nslab * cols;
  hipLaunchKernelGGL(bn_zero_row_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), slab, nslab,
                     (long long)stride, (long long)offset, cols);
  DL_RETURN_LAUNCH("dl_bn_zero_bias_grad");
}

extern "C" int64_t dl_bn_ws_floats(int32_t B, int32_t D) {
  return B < 1 || D < 1 ? 0 : (int64_t)bn_grid(B) * 3 * bn_dp(D);
}

extern "C" int dl_bn_stats(int32_t B, int32_t D, const float* C, int32_t ldc, float eps, float momentum, float* stat,
                           float* run_mean, float* run_var, const float* opt, float* ws, int64_t ws_floats,
                           void* stream) {
  DL_CHECK_ARG(C && stat && ws, "dl_bn_stats: NULL pointer");
  DL_CHECK_ARG(D >= 1, "dl_bn_stats: D %d < 1", D);
  DL_CHECK_ARG(B >= 2, "dl_bn_stats: B %d < 2 (batch statistics need two rows)", B);
  DL_BN_CHECK_MATRIX("dl_bn_stats", C, ldc, D);
  DL_CHECK_ARG(bn_aligned(stat) && bn_aligned(ws), "dl_bn_stats: stat and ws must be 16-B aligned");
  DL_CHECK_ARG(eps > 0.f && momentum > 0.f && momentum <= 1.f, "dl_bn_stats: eps %g must be > 0, momentum %g in (0, 1]",
               (double)eps, (double)momentum);
  DL_CHECK_ARG((run_mean == nullptr) == (run_var == nullptr), "dl_bn_stats: run_mean and run_var go together");
  DL_CHECK_ARG(ws_floats >= dl_bn_ws_floats(B, D), "dl_bn_stats: ws needs %lld floats, has %lld",
               (long long)dl_bn_ws_floats(B, D), (long long)ws_floats);
  const BnGeo g = bn_geo(D);
  const int G = bn_grid(B), R = bn_rows(B), Dp = bn_dp(D);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(bn_stats_part_kernel, dim3(G, g.chunks), dim3(kBnThreads), 0, s, C, ldc, B, D, R, g.cgw, g.ry, Dp,
                     ws);
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(Dp / 16), dim3(256), 0, s, ws, G, R, B, D, Dp, eps, momentum, stat,
                     run_mean, run_var, opt);
  DL_RETURN_LAUNCH("dl_bn_stats");
}

extern "C" int dl_bn_fwd(int32_t B, int32_t D, float* C, int32_t ldc, const float* stat, const float* run_mean,
                         const float* run_var, float eps, const float* params, float* hx, int32_t ldx, uint16_t* bits,
                         int32_t ldbits, void* stream) {
  DL_CHECK_ARG(C && params, "dl_bn_fwd: NULL pointer");
  DL_CHECK_ARG(D >= 1 && B >= 1, "dl_bn_fwd: D %d < 1 or B %d < 1", D, B);
  DL_BN_CHECK_MATRIX("dl_bn_fwd", C, ldc, D);
  if (stat) {
    DL_CHECK_ARG(hx, "dl_bn_fwd: training (stat given) needs hx");
    DL_BN_CHECK_MATRIX("dl_bn_fwd", hx, ldx, D);
    DL_CHECK_ARG(bn_aligned(stat), "dl_bn_fwd: stat must be 16-B aligned");
  } else {
    DL_CHECK_ARG(run_mean && run_var && !hx, "dl_bn_fwd: inference (no stat) needs run_mean and run_var and no hx");
    DL_CHECK_ARG(eps > 0.f, "dl_bn_fwd: eps %g must be > 0", (double)eps);
  }
  DL_CHECK_ARG(!bits || ldbits >= (D + 15) / 16, "dl_bn_fwd: ldbits %d < %d halfwords", ldbits, (D + 15) / 16);
  const BnGeo g = bn_geo(D);
  const int G = bn_grid(B), R = bn_rows(B), Dp = bn_dp(D);
  hipStream_t s = as_stream(stream);
  if (stat)
    hipLaunchKernelGGL(bn_fwd_kernel<true>, dim3(G, g.chunks), dim3(kBnThreads), 0, s, C, ldc, B, D, R, g.cgw, g.ry, Dp,
                       stat, run_mean, run_var, eps, params, hx, ldx, bits, ldbits);
  else
    hipLaunchKernelGGL(bn_fwd_kernel<false>, dim3(G, g.chunks), dim3(kBnThreads), 0, s, C, ldc, B, D, R, g.cgw, g.ry, Dp,
                       stat, run_mean, run_var, eps, params, hx, ldx, bits, ldbits);
  DL_RETURN_LAUNCH("dl_bn_fwd");
}

extern "C" int dl_bn_bwd_sums(int32_t B, int32_t D, const float* dy, int32_t ldd, const float* hx, int32_t ldx,
                              float* slab, int32_t slab_rows, void* stream) {
  DL_CHECK_ARG(dy && hx && slab, "dl_bn_bwd_sums: NULL pointer");
  DL_CHECK_ARG(D >= 1, "dl_bn_bwd_sums: D %d < 1", D);
  DL_CHECK_ARG(B >= 2, "dl_bn_bwd_sums: B %d < 2", B);
  DL_BN_CHECK_MATRIX("dl_bn_bwd_sums", dy, ldd, D);
  DL_BN_CHECK_MATRIX("dl_bn_bwd_sums", hx, ldx, D);
  DL_CHECK_ARG(slab_rows == bn_grid(B), "dl_bn_bwd_sums: slab needs %d rows (dl_bn_grid), has %d", bn_grid(B),
               slab_rows);
  const BnGeo g = bn_geo(D);
  hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3(bn_grid(B), g.chunks), dim3(kBnThreads), 0, as_stream(stream), dy, ldd, hx,
                     ldx, B, D, bn_rows(B), g.cgw, g.ry, slab);
  DL_RETURN_LAUNCH("dl_bn_bwd_sums");
}

extern "C" int dl_bn_bwd_apply(int32_t B, int32_t D, float* dy, int32_t ldd, const float* hx, int32_t ldx,
                               const float* params, const float* stat, const float* slab, int32_t slab_rows,
                               float* sums, void* stream) {
  DL_CHECK_ARG(dy && hx && params && stat && slab && sums, "dl_bn_bwd_apply: NULL pointer");
  DL_CHECK_ARG(D >= 1, "dl_bn_bwd_apply: D %d < 1", D);
  DL_CHECK_ARG(B >= 2, "dl_bn_bwd_apply: B %d < 2", B);
  DL_BN_CHECK_MATRIX("dl_bn_bwd_apply", dy, ldd, D);
  DL_BN_CHECK_MATRIX("dl_bn_bwd_apply", hx, ldx, D);
  DL_CHECK_ARG(bn_aligned(stat) && bn_aligned(sums), "dl_bn_bwd_apply: stat and sums must be 16-B aligned");
  DL_CHECK_ARG(slab_rows == bn_grid(B), "dl_bn_bwd_apply: slab needs %d rows (dl_bn_grid), has %d", bn_grid(B),
               slab_rows);
  const BnGeo g = bn_geo(D);
  const int G = bn_grid(B), Dp = bn_dp(D);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(bn_bwd_merge_kernel, dim3(Dp / 16, 2), dim3(256), 0, s, slab, G, D, Dp, sums);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(G, g.chunks), dim3(kBnThreads), 0, s, dy, ldd, hx, ldx, B, D, bn_rows(B),
                     g.cgw, g.ry, Dp, params, stat, sums);
  DL_RETURN_LAUNCH("dl_bn_bwd_apply");
}
