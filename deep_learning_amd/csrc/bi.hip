// Bi-Interaction pooling of the embedded fields (NFM) as E more columns of the dnn_* tower input.
//
// Reference: test_model/NFM.py:192-197, 226 (fm_second_order = 1/2 ((sum_f e_f)^2 - sum_f e_f^2), fed
// to the deep layers).  Over the F fields of x0 [B, ld], field f in columns [x_col0 + f E, + E):
//   forward:   q[e] = sum_{f<g} e_f[e] e_g[e], formed as the prefix chain
//                     q = sum_f e_f * P_f,  P_f = sum_{g<f} e_g
//              in field order (the subtractive form 1/2 (s^2 - sum e^2) rounds at the size of s^2, 14
//              times this chain's error on fields of a common mean and 1000 times where a field
//              dominates, and is not used).  Both running sums are kept as a float
//              pair (the product's rounding error by one fma, the sums' by Knuth's two-sum): the plain
//              f32 chain random-walks to 3e-5 at F = 64, E = 32 on fields ~ N(0, 1/2) (|q| ~ 40), above
//              the project's 1e-5 parity rule; the pair leaves the final rounding of q alone.  The
//              kernel is bandwidth-bound, the ~20 extra flops a field cost no time.
//   backward:  s = sum_g e_g;  de_f += dq * (s - e_f)   (added INTO dx0's field columns)
//
// Mapping.  Both kernels stream a sample's F E contiguous floats once (the backward twice, the
// second time from cache, plus the read-modify-write of dx0): bandwidth-bound, no reuse between
// samples, nothing to keep in LDS.  A thread owns one group of 4 embedding columns (one 16-B piece of
// every field) of one sample for the whole field loop, so P, q and s live in registers and the chain's
// order is the field order, whatever the launch.  A block of 256 threads is E / 4 column groups x
// RY = 1024 / E sample lanes: the lanes of a sample read one contiguous E-float piece, and a wave
// covers 256 / E whole samples.  The field loop is unrolled 8 deep (the backward's second pass 4 deep
// on two matrices): 8 independent 16-B loads a thread in flight, 32 KB a block.  Block b owns the
// samples [b R, (b + 1) R) with R = max(32, ceil(B / 1024)): at most 1024 blocks (4 a CU), as
// dl_bn_grid, so a CU has up to 128 KB of loads in flight, above the ~32 KB per CU at which the copy
// yardstick's stream saturates HBM; nothing is summed across blocks, so the cap is about launch
// size only.  When x0 / q / dq / dx0, their pitches and column offsets are all multiples of 16 B
// every access is one 16-B instruction (the engine's case); otherwise the same arithmetic runs on
// 4-B accesses.  No LDS, no atomics, no memset; the same inputs give the same bits on every run.
#include "common.h"

namespace dl {

typedef float bi_f4 __attribute__((ext_vector_type(4)));

constexpr int kBiThreads = 256;
constexpr int kBiMaxGrid = 1024;   // 4 blocks a CU
constexpr int kBiMinRows = 32;     // samples a block owns at least
constexpr int kBiUnroll = 8;       // fields a thread keeps in flight
constexpr int kBiMaxF = 64, kBiMaxE = 64;

static int bi_rows(int B) {   // samples a block owns
  const int r = (B + kBiMaxGrid - 1) / kBiMaxGrid;
  return r < kBiMinRows ? kBiMinRows : r;
}
static int bi_grid(int B) { return B < 1 ? 1 : (B + bi_rows(B) - 1) / bi_rows(B); }

template <bool kVec>
__device__ __forceinline__ bi_f4 bi_ld(const float* p) {
  if (kVec) return *reinterpret_cast<const bi_f4*>(p);
  bi_f4 v = {p[0], p[1], p[2], p[3]};
  return v;
}
template <bool kVec>
__device__ __forceinline__ void bi_st(float* p, bi_f4 v) {
  if (kVec) {
    *reinterpret_cast<bi_f4*>(p) = v;
    return;
  }
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
  p[3] = v.w;
}
__device__ __forceinline__ bi_f4 bi_fma(bi_f4 a, bi_f4 b, bi_f4 c) {
  bi_f4 r = {__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y), __builtin_fmaf(a.z, b.z, c.z),
             __builtin_fmaf(a.w, b.w, c.w)};
  return r;
}

// s + e = a + b exactly (Knuth); the additions must stay separate roundings
__device__ __forceinline__ void bi_two_sum(bi_f4 a, bi_f4 b, bi_f4& s, bi_f4& e) {
#pragma clang fp contract(off)
  s = a + b;
  const bi_f4 bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
// p + e = a * b exactly
__device__ __forceinline__ void bi_two_prod(bi_f4 a, bi_f4 b, bi_f4& p, bi_f4& e) {
#pragma clang fp contract(off)
  p = a * b;
  e = bi_fma(a, b, -p);
}

// x0 and q may be the same matrix (the engine's case: q is x0's columns after the fields), so neither
// is __restrict__; a thread has read all it needs of its sample before it writes, and no other thread
// reads what it writes (the entry point refuses overlapping column ranges).
template <bool kVec>
__global__ __launch_bounds__(kBiThreads) void bi_fwd_kernel(int B, int F, int E, int R, const float* x0, int ld,
                                                            int x_col0, float* q, int ldq, int q_col0) {
  const int cgw = E >> 2, ry = kBiThreads / cgw;
  const int yy = threadIdx.x / cgw, g = threadIdx.x - yy * cgw;
  if (yy >= ry) return;
  const int r0 = blockIdx.x * R, r1 = min(B, r0 + R);
  for (int r = r0 + yy; r < r1; r += ry) {
    const float* xr = x0 + (int64_t)r * ld + x_col0 + 4 * g;
    bi_f4 P = {0.f, 0.f, 0.f, 0.f}, Pl = P, acc = P, accl = P;   // P + Pl = the prefix sum, acc + accl = q
    for (int f0 = 0; f0 < F; f0 += kBiUnroll) {
      bi_f4 v[kBiUnroll];
#pragma unroll
      for (int u = 0; u < kBiUnroll; ++u)
        if (f0 + u < F) v[u] = bi_ld<kVec>(xr + (f0 + u) * E);
#pragma unroll
      for (int u = 0; u < kBiUnroll; ++u)
        if (f0 + u < F) {
          bi_f4 p, pe, e;
          bi_two_prod(v[u], P, p, pe);
          pe = bi_fma(v[u], Pl, pe);
          bi_two_sum(acc, p, acc, e);
          accl += e + pe;
          bi_two_sum(P, v[u], P, e);
          Pl += e;
        }
    }
    bi_st<kVec>(q + (int64_t)r * ldq + q_col0 + 4 * g, acc + accl);
  }
}

// dq may be columns of dx0 itself (the engine's case), outside the field columns this kernel writes.
template <bool kVec>
__global__ __launch_bounds__(kBiThreads) void bi_bwd_kernel(int B, int F, int E, int R, const float* __restrict__ x0,
                                                            int ld, int x_col0, const float* dq, int lddq,
                                                            int dq_col0, float* dx0, int dx_ld, int dx_col0) {
  const int cgw = E >> 2, ry = kBiThreads / cgw;
  const int yy = threadIdx.x / cgw, g = threadIdx.x - yy * cgw;
  if (yy >= ry) return;
  const int r0 = blockIdx.x * R, r1 = min(B, r0 + R);
  constexpr int kU = kBiUnroll / 2;
  for (int r = r0 + yy; r < r1; r += ry) {
    const float* xr = x0 + (int64_t)r * ld + x_col0 + 4 * g;
    float* dr = dx0 + (int64_t)r * dx_ld + dx_col0 + 4 * g;
    const bi_f4 d = bi_ld<kVec>(dq + (int64_t)r * lddq + dq_col0 + 4 * g);
    bi_f4 s = {0.f, 0.f, 0.f, 0.f};
    for (int f0 = 0; f0 < F; f0 += kBiUnroll) {
      bi_f4 v[kBiUnroll];
#pragma unroll
      for (int u = 0; u < kBiUnroll; ++u)
        if (f0 + u < F) v[u] = bi_ld<kVec>(xr + (f0 + u) * E);
#pragma unroll
      for (int u = 0; u < kBiUnroll; ++u)
        if (f0 + u < F) s += v[u];
    }
    for (int f0 = 0; f0 < F; f0 += kU) {
      bi_f4 v[kU], a[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u)
        if (f0 + u < F) {
          v[u] = bi_ld<kVec>(xr + (f0 + u) * E);
          a[u] = bi_ld<kVec>(dr + (f0 + u) * E);
        }
#pragma unroll
      for (int u = 0; u < kU; ++u)
        if (f0 + u < F) bi_st<kVec>(dr + (f0 + u) * E, bi_fma(d, s - v[u], a[u]));
    }
  }
}

static bool bi_vec_ok(const void* p, int ld, int col0) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0 && col0 % 4 == 0;
}

static int bi_check(const char* name, int32_t B, int32_t F, int32_t E, const float* x0, int32_t ld, int32_t x_col0) {
  DL_CHECK_ARG(B >= 0, "%s: B %d < 0", name, B);
  DL_CHECK_ARG(F >= 2 && F <= kBiMaxF, "%s: F %d fields not in [2, %d]", name, F, kBiMaxF);
  DL_CHECK_ARG(E >= 4 && E <= kBiMaxE && E % 4 == 0, "%s: E %d not a multiple of 4 in [4, %d]", name, E, kBiMaxE);
  DL_CHECK_ARG(x0 && x_col0 >= 0 && (long long)x_col0 + (long long)F * E <= ld,
               "%s: x0 required, field columns [%d, %d) within ld %d", name, x_col0, x_col0 + F * E, ld);
  return 0;
}

}  // namespace dl

using namespace dl;

extern "C" int dl_bi_grid(int32_t B) { return bi_grid(B); }

extern "C" int dl_bi_fwd(int32_t B, int32_t F, int32_t E, const float* x0, int32_t ld, int32_t x_col0, float* q,
                         int32_t ldq, int32_t q_col0, void* stream) {
  if (int rc = bi_check("dl_bi_fwd", B, F, E, x0, ld, x_col0)) return rc;
  DL_CHECK_ARG(q && q_col0 >= 0 && (long long)q_col0 + E <= ldq, "dl_bi_fwd: q required, columns [%d, %d) within ldq %d",
               q_col0, q_col0 + E, ldq);
  // q inside x0's own rows (same matrix, same pitch): its columns must miss the fields'
  DL_CHECK_ARG(q != x0 || ld != ldq || q_col0 >= x_col0 + F * E || q_col0 + E <= x_col0,
               "dl_bi_fwd: q columns [%d, %d) overlap the field columns [%d, %d) of the same matrix", q_col0,
               q_col0 + E, x_col0, x_col0 + F * E);
  if (B == 0) return 0;
  const bool vec = bi_vec_ok(x0, ld, x_col0) && bi_vec_ok(q, ldq, q_col0);
  const dim3 grid(bi_grid(B)), block(kBiThreads);
  if (vec)
    hipLaunchKernelGGL(bi_fwd_kernel<true>, grid, block, 0, as_stream(stream), B, F, E, bi_rows(B), x0, ld, x_col0, q,
                       ldq, q_col0);
  else
    hipLaunchKernelGGL(bi_fwd_kernel<false>, grid, block, 0, as_stream(stream), B, F, E, bi_rows(B), x0, ld, x_col0, q,
                       ldq, q_col0);
  DL_RETURN_LAUNCH("dl_bi_fwd");
}

extern "C" int dl_bi_bwd(int32_t B, int32_t F, int32_t E, const float* x0, int32_t ld, int32_t x_col0, const float* dq,
                         int32_t lddq, int32_t dq_col0, float* dx0, int32_t dx_ld, int32_t dx_col0, void* stream) {
  if (int rc = bi_check("dl_bi_bwd", B, F, E, x0, ld, x_col0)) return rc;
  DL_CHECK_ARG(dq && dq_col0 >= 0 && (long long)dq_col0 + E <= lddq,
               "dl_bi_bwd: dq required, columns [%d, %d) within lddq %d", dq_col0, dq_col0 + E, lddq);
  DL_CHECK_ARG(dx0 && dx_col0 >= 0 && (long long)dx_col0 + (long long)F * E <= dx_ld,
               "dl_bi_bwd: dx0 required, columns [%d, %d) within dx_ld %d", dx_col0, dx_col0 + F * E, dx_ld);
  // dq inside dx0's own rows: its columns must miss the field columns this kernel rewrites
  DL_CHECK_ARG(dq != dx0 || lddq != dx_ld || dq_col0 >= dx_col0 + F * E || dq_col0 + E <= dx_col0,
               "dl_bi_bwd: dq columns [%d, %d) overlap dx0's field columns [%d, %d) of the same matrix", dq_col0,
               dq_col0 + E, dx_col0, dx_col0 + F * E);
  if (B == 0) return 0;
  const bool vec = bi_vec_ok(x0, ld, x_col0) && bi_vec_ok(dq, lddq, dq_col0) && bi_vec_ok(dx0, dx_ld, dx_col0);
  const dim3 grid(bi_grid(B)), block(kBiThreads);
  if (vec)
    hipLaunchKernelGGL(bi_bwd_kernel<true>, grid, block, 0, as_stream(stream), B, F, E, bi_rows(B), x0, ld, x_col0, dq,
                       lddq, dq_col0, dx0, dx_ld, dx_col0);
  else
    hipLaunchKernelGGL(bi_bwd_kernel<false>, grid, block, 0, as_stream(stream), B, F, E, bi_rows(B), x0, ld, x_col0,
                       dq, lddq, dq_col0, dx0, dx_ld, dx_col0);
  DL_RETURN_LAUNCH("dl_bi_bwd");
}
