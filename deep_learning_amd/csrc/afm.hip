// Attentional pairwise interactions (AFM) beside the dnn_* tower, forward and backward.
//
// Reference: test_model/AFM.py:63-129 (its pairwise-interaction and attention layers) on the F
// embedded fields of the engine's tower input x0 (columns [x_col0, x_col0 + F E), E floats a field):
//   q_ij = e_i * e_j;  u_ij = q_ij W + b;  s_ij = h . relu(u_ij);  a = softmax over the P pairs;
//   z_afm = (sum a_ij q_ij) . p = sum a_ij t_ij,   t_ij = q_ij . p
// Backward, with z = z_afm:  ds_ij = a_ij dz (t_ij - z);  g_ij = ds_ij (h * [u_ij > 0]);
//   dq_ij = a_ij dz p + W g_ij;  de_i += dq_ij * e_j;  de_j += dq_ij * e_i;
//   dp = sum dz a_ij q_ij;  dh = sum ds_ij relu(u_ij);  db = sum g_ij;  dW = sum q_ij (x) g_ij.
// params: [p (E) | h (A) | b (A) | W (E A, row-major [E][A])].
//
// Mapping (both kernels): lane = field, round-robin pairing.  A sample owns G = 32 lanes (F <= 32:
// two samples a wave) or 64; in round r = 1 .. F / 2 lane i forms the pair (i, (i + r) mod F) (an
// even F's last round holds each pair twice: lanes i < F / 2 only), so every pair is computed once,
// de_i accumulates in lane i's registers and the partner's share arrives by a lane rotate: a fixed
// order, no atomics, nothing of size P in LDS.  The sample's fields sit in LDS (pitch E + 4), the
// parameters are staged once per block with A zero-padded (uniform reads broadcast).  The softmax
// is an online max / sum per lane, merged across the sample's lanes.  The backward takes the
// forward's (max, sum), so pass 1 (scores -> a, kept per round in LDS, and z) needs no max pass;
// pass 2 forms g, dq and de, and leaves each round's q, g and ds relu(u) rows in LDS, from which
// the wave sums dW, db and dh with lane = (k, block of e) over the round's 64 rows.  The batch sums
// leave as one slab row per block in the parameter vector's layout (dl_adam_dense sums the rows
// in slab order).  The same inputs give the same bits on every run.
#include <math.h>

#include "common.h"

namespace dl {

constexpr int kAfmMaxF = 64;
constexpr int kAfmMaxA = 32;

__device__ __forceinline__ float afm_group_sum(float v, int G) {
  for (int o = G >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float afm_group_max(float v, int G) {
  for (int o = G >> 1; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// the parameters into LDS: [p (E) | h (AP) | b (AP) | W [E][AP]], columns [A, AP) zero
template <int E>
__device__ __forceinline__ void afm_stage(float* lds, const float* __restrict__ prm, int A, int AP) {
  for (int i = threadIdx.x; i < E; i += blockDim.x) lds[i] = prm[i];
  for (int i = threadIdx.x; i < AP; i += blockDim.x) {
    lds[E + i] = i < A ? prm[E + i] : 0.f;
    lds[E + AP + i] = i < A ? prm[E + A + i] : 0.f;
  }
  for (int i = threadIdx.x; i < E * AP; i += blockDim.x) {
    const int e = i / AP, k = i - e * AP;
    lds[E + 2 * AP + i] = k < A ? prm[E + 2 * A + e * A + k] : 0.f;
  }
  __syncthreads();
}

// the wave's samples' fields into its LDS rows (row = slot * G + field, pitch E + 4; a sample past
// the batch reads as zeros)
template <int E>
__device__ __forceinline__ void afm_load_fields(float* fld, const float* __restrict__ x0, int ld, int x_col0,
                                                int b0, int B, int F, int G, int lane) {
  constexpr int ES = E + 4;
  for (int sl = 0; sl * G < 64; ++sl) {
    const int b = b0 + sl;
    const float* row = x0 + (long long)(b < B ? b : 0) * ld + x_col0;
    for (int idx = lane; idx < F * E; idx += 64) {
      const int f = idx / E, e = idx - f * E;
      fld[(sl * G + f) * ES + e] = b < B ? row[idx] : 0.f;
    }
  }
}

// 4 attention units of one pair: u = b + q W (columns k0 .. k0 + 3)
template <int E>
__device__ __forceinline__ float4 afm_u4(const float (&q)[E], const float* Bs, const float* Ws, int AP, int k0) {
  float4 u = *reinterpret_cast<const float4*>(Bs + k0);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float4 w = *reinterpret_cast<const float4*>(Ws + e * AP + k0);
    u.x = __builtin_fmaf(q[e], w.x, u.x);
    u.y = __builtin_fmaf(q[e], w.y, u.y);
    u.z = __builtin_fmaf(q[e], w.z, u.z);
    u.w = __builtin_fmaf(q[e], w.w, u.w);
  }
  return u;
}

// s = h . relu(b + q W)
template <int E>
__device__ __forceinline__ float afm_score(const float (&q)[E], const float* Hs, const float* Bs, const float* Ws,
                                           int AP, int A4) {
  float s = 0.f;
  for (int k0 = 0; k0 < A4; k0 += 4) {
    const float4 u = afm_u4<E>(q, Bs, Ws, AP, k0);
    const float4 h = *reinterpret_cast<const float4*>(Hs + k0);
    s += h.x * fmaxf(u.x, 0.f) + h.y * fmaxf(u.y, 0.f) + h.z * fmaxf(u.z, 0.f) + h.w * fmaxf(u.w, 0.f);
  }
  return s;
}

// q = e_i * e_j (zeros for a lane without a pair) and t = q . p
template <int E>
__device__ __forceinline__ float afm_pair(const float (&ei)[E], const float* ej, const float* Ps, bool v,
                                          float (&q)[E], float (&ejr)[E]) {
  float t = 0.f;
#pragma unroll
  for (int e = 0; e < E; e += 4) {
    const float4 x = *reinterpret_cast<const float4*>(ej + e);
    ejr[e] = x.x, ejr[e + 1] = x.y, ejr[e + 2] = x.z, ejr[e + 3] = x.w;
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    q[e] = v ? ei[e] * ejr[e] : 0.f;
    t = __builtin_fmaf(q[e], Ps[e], t);
  }
  return t;
}

template <int E>
__global__ __launch_bounds__(256) void afm_fwd_kernel(int B, int F, int A, int AP, const float* __restrict__ x0,
                                                      int ld, int x_col0, const float* __restrict__ prm,
                                                      const float* __restrict__ z_add, float* __restrict__ stats,
                                                      float* __restrict__ z_out) {
  constexpr int ES = E + 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];   // params | per wave: fields [64][ES]
  afm_stage<E>(lds, prm, A, AP);
  const float* Ps = lds;
  const float* Hs = lds + E;
  const float* Bs = Hs + AP;
  const float* Ws = Bs + AP;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float* fld = lds + (E + 2 * AP + E * AP) + wid * 64 * ES;
  const int G = F <= 32 ? 32 : 64, SPW = 64 / G;
  const int i = lane & (G - 1), sl = lane / G;
  const int R = F >> 1, A4 = (A + 3) & ~3;
  const long long unit = (long long)nw * SPW, span = unit * gridDim.x;
  const int iters = (int)((B + span - 1) / span);
  for (int it = 0; it < iters; ++it) {
    const long long base = ((long long)it * gridDim.x + blockIdx.x) * unit + (long long)wid * SPW;
    const int b0 = base < B ? (int)base : B;
    afm_load_fields<E>(fld, x0, ld, x_col0, b0, B, F, G, lane);
    __syncthreads();
    const int b = b0 + sl;
    const bool act = b < B && i < F;
    float ei[E];
#pragma unroll
    for (int e = 0; e < E; ++e) ei[e] = act ? fld[(sl * G + i) * ES + e] : 0.f;
    float m = -INFINITY, l = 0.f, acc = 0.f;
    for (int r = 1; r <= R; ++r) {
      int j = i + r;
      if (j >= F) j -= F;
      const bool v = act && (2 * r != F || i < R);
      float q[E], ejr[E];
      const float t = afm_pair<E>(ei, fld + (sl * G + (v ? j : 0)) * ES, Ps, v, q, ejr);
      const float s = afm_score<E>(q, Hs, Bs, Ws, AP, A4);
      if (v) {
        const float d = s - m;           // m = -inf at the lane's first pair: exp(-inf) = 0
        const float x = expf(-fabsf(d));
        if (d > 0.f) {
          l = __builtin_fmaf(l, x, 1.f);
          acc = __builtin_fmaf(acc, x, t);
          m = s;
        } else {
          l += x;
          acc = __builtin_fmaf(x, t, acc);
        }
      }
    }
    const float M = afm_group_max(m, G);
    const float sc = m == -INFINITY ? 0.f : expf(m - M);
    const float L = afm_group_sum(l * sc, G);
    const float Z = afm_group_sum(acc * sc, G) / L;
    if (act && i == 0) {
      z_out[b] = z_add ? Z + z_add[b] : Z;
      stats[2 * (long long)b] = M;
      stats[2 * (long long)b + 1] = L;
    }
    __syncthreads();
  }
}

template <int E, int AP>
__global__ __launch_bounds__(256) void afm_bwd_kernel(int B, int F, int A, const float* __restrict__ x0, int ld,
                                                      int x_col0, const float* __restrict__ prm,
                                                      const float* __restrict__ stats, const float* __restrict__ dz,
                                                      float* __restrict__ dx0, int dx_ld, int dx_col0,
                                                      float* __restrict__ slab) {
  constexpr int ES = E + 4, GS = AP + 4, NE = E * AP / 64;
  constexpr int kPar = E + 2 * AP + E * AP;
  // params | per wave: fields [64][ES], a [R][64], q [64][ES], g [64][GS], ds relu(u) [64][GS]
  extern __shared__ __attribute__((aligned(16))) float lds[];
  afm_stage<E>(lds, prm, A, AP);
  const float* Ps = lds;
  const float* Hs = lds + E;
  const float* Bs = Hs + AP;
  const float* Ws = Bs + AP;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int R = F >> 1, A4 = (A + 3) & ~3;
  const int per_wave = 2 * 64 * ES + R * 64 + 2 * 64 * GS;
  float* fld = lds + kPar + wid * per_wave;
  float* abuf = fld + 64 * ES;
  float* Qb = abuf + R * 64;
  float* Gb = Qb + 64 * ES;
  float* Rb = Gb + 64 * GS;
  const int G = F <= 32 ? 32 : 64, SPW = 64 / G;
  const int i = lane & (G - 1), sl = lane / G;
  const int kk = lane % AP, e0 = (lane / AP) * NE;   // this lane's elements of dW: rows e0 .. e0 + NE - 1, column kk
  float ol[E], dWa[NE], dbk = 0.f, dhk = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) ol[e] = 0.f;
#pragma unroll
  for (int n = 0; n < NE; ++n) dWa[n] = 0.f;
  const long long unit = (long long)nw * SPW, span = unit * gridDim.x;
  const int iters = (int)((B + span - 1) / span);
  for (int it = 0; it < iters; ++it) {
    const long long base = ((long long)it * gridDim.x + blockIdx.x) * unit + (long long)wid * SPW;
    const int b0 = base < B ? (int)base : B;
    afm_load_fields<E>(fld, x0, ld, x_col0, b0, B, F, G, lane);
    __syncthreads();
    const int b = b0 + sl;
    const bool act = b < B && i < F;
    float ei[E];
#pragma unroll
    for (int e = 0; e < E; ++e) ei[e] = act ? fld[(sl * G + i) * ES + e] : 0.f;
    const float dzb = act ? dz[b] : 0.f;
    const float M = act ? stats[2 * (long long)b] : 0.f;
    const float L = act ? stats[2 * (long long)b + 1] : 1.f;
    // pass 1: a of every pair, and z = sum a t
    float zs = 0.f;
    for (int r = 1; r <= R; ++r) {
      int j = i + r;
      if (j >= F) j -= F;
      const bool v = act && (2 * r != F || i < R);
      float q[E], ejr[E];
      const float t = afm_pair<E>(ei, fld + (sl * G + (v ? j : 0)) * ES, Ps, v, q, ejr);
      const float s = afm_score<E>(q, Hs, Bs, Ws, AP, A4);
      const float a = v ? expf(s - M) / L : 0.f;
      abuf[(r - 1) * 64 + lane] = a;
      zs = __builtin_fmaf(a, t, zs);
    }
    const float z = afm_group_sum(zs, G);
    // pass 2
    float de[E];
#pragma unroll
    for (int e = 0; e < E; ++e) de[e] = 0.f;
    for (int r = 1; r <= R; ++r) {
      int j = i + r;
      if (j >= F) j -= F;
      const bool v = act && (2 * r != F || i < R);
      float q[E], ejr[E], dq[E];
      const float t = afm_pair<E>(ei, fld + (sl * G + (v ? j : 0)) * ES, Ps, v, q, ejr);
      const float a = abuf[(r - 1) * 64 + lane];
      const float adz = a * dzb;
      const float ds = adz * (t - z);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        dq[e] = adz * Ps[e];
        ol[e] = __builtin_fmaf(adz, q[e], ol[e]);
      }
#pragma unroll
      for (int e = 0; e < E; e += 4)
        *reinterpret_cast<float4*>(Qb + lane * ES + e) = make_float4(q[e], q[e + 1], q[e + 2], q[e + 3]);
      for (int k0 = 0; k0 < A4; k0 += 4) {
        const float4 u = afm_u4<E>(q, Bs, Ws, AP, k0);
        const float4 h = *reinterpret_cast<const float4*>(Hs + k0);
        float4 g, rr;
        g.x = v && u.x > 0.f ? ds * h.x : 0.f;
        g.y = v && u.y > 0.f ? ds * h.y : 0.f;
        g.z = v && u.z > 0.f ? ds * h.z : 0.f;
        g.w = v && u.w > 0.f ? ds * h.w : 0.f;
        rr.x = v ? ds * fmaxf(u.x, 0.f) : 0.f;
        rr.y = v ? ds * fmaxf(u.y, 0.f) : 0.f;
        rr.z = v ? ds * fmaxf(u.z, 0.f) : 0.f;
        rr.w = v ? ds * fmaxf(u.w, 0.f) : 0.f;
        *reinterpret_cast<float4*>(Gb + lane * GS + k0) = g;
        *reinterpret_cast<float4*>(Rb + lane * GS + k0) = rr;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float4 w = *reinterpret_cast<const float4*>(Ws + e * AP + k0);
          dq[e] += w.x * g.x + w.y * g.y + w.z * g.z + w.w * g.w;
        }
      }
      for (int k0 = A4; k0 < AP; k0 += 4) {
        *reinterpret_cast<float4*>(Gb + lane * GS + k0) = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(Rb + lane * GS + k0) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      // this lane's share, then the partner's: lane i is the second field of pair (i - r, i)
      int src = i - r;
      if (src < 0) src += F;
      const int src_lane = sl * G + (src & (G - 1));
#pragma unroll
      for (int e = 0; e < E; ++e) {
        de[e] = __builtin_fmaf(dq[e], ejr[e], de[e]);
        de[e] += __shfl(v ? dq[e] * ei[e] : 0.f, src_lane, 64);
      }
      __syncthreads();
      // the round's 64 rows into dW, db, dh
      for (int l2 = 0; l2 < 64; ++l2) {
        const float gk = Gb[l2 * GS + kk];
        dbk += gk;
        dhk += Rb[l2 * GS + kk];
        if constexpr (NE >= 4) {
#pragma unroll
          for (int n = 0; n < NE; n += 4) {
            const float4 x = *reinterpret_cast<const float4*>(Qb + l2 * ES + e0 + n);
            dWa[n] = __builtin_fmaf(x.x, gk, dWa[n]);
            dWa[n + 1] = __builtin_fmaf(x.y, gk, dWa[n + 1]);
            dWa[n + 2] = __builtin_fmaf(x.z, gk, dWa[n + 2]);
            dWa[n + 3] = __builtin_fmaf(x.w, gk, dWa[n + 3]);
          }
        } else {
#pragma unroll
          for (int n = 0; n < NE; ++n) dWa[n] = __builtin_fmaf(Qb[l2 * ES + e0 + n], gk, dWa[n]);
        }
      }
      __syncthreads();
    }
    // de through the fields' rows, then added into dx0 with whole-row accesses
    if (act) {
#pragma unroll
      for (int e = 0; e < E; ++e) fld[(sl * G + i) * ES + e] = de[e];
    }
    __syncthreads();
    for (int s2 = 0; s2 < SPW; ++s2) {
      if (b0 + s2 < B) {
        float* drow = dx0 + (long long)(b0 + s2) * dx_ld + dx_col0;
        for (int idx = lane; idx < F * E; idx += 64) {
          const int f = idx / E, e = idx - f * E;
          drow[idx] += fld[(s2 * G + f) * ES + e];
        }
      }
    }
    __syncthreads();
  }
  // block sums in wave order through the staging buffer (the parameters are no longer needed)
#pragma unroll
  for (int e = 0; e < E; ++e) ol[e] = wave_sum(ol[e]);
  __syncthreads();
  float* red = lds;
  for (int w = 0; w < nw; ++w) {
    if (wid == w) {
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < E; ++e) red[e] = w ? red[e] + ol[e] : ol[e];
      }
      if (kk < A) {
        if (lane < AP) {
          red[E + kk] = w ? red[E + kk] + dhk : dhk;
          red[E + A + kk] = w ? red[E + A + kk] + dbk : dbk;
        }
#pragma unroll
        for (int n = 0; n < NE; ++n) {
          float* pw = red + E + 2 * A + (e0 + n) * A + kk;
          *pw = w ? *pw + dWa[n] : dWa[n];
        }
      }
    }
    __syncthreads();
  }
  const int n = E + 2 * A + E * A;
  float* out = slab + (long long)blockIdx.x * n;
  for (int k = threadIdx.x; k < n; k += blockDim.x) out[k] = red[k];
}

// The f32 vector-rate yardstick (scripts/afm_bench.py): 16 independent FMA chains a thread,
// 32 * iters FLOP a thread, nothing from memory; one float a thread written so the work stays.
__global__ __launch_bounds__(256) void vfma_probe_kernel(float* __restrict__ out, int iters, float a, float b) {
  float acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = (float)(threadIdx.x + k);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = __builtin_fmaf(acc[k], a, b);
  }
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) t += acc[k];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = t;
}

}  // namespace dl

using namespace dl;

extern "C" int dl_vfma_probe(float* out, int64_t n_out, int32_t blocks, int32_t iters, void* stream) {
  DL_CHECK_ARG(out && blocks >= 1 && iters >= 0 && n_out >= (int64_t)blocks * 256,
               "dl_vfma_probe: out needs %lld floats", (long long)blocks * 256);
  hipLaunchKernelGGL(vfma_probe_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), out, iters, 0.999f, 0.001f);
  DL_RETURN_LAUNCH("dl_vfma_probe");
}

extern "C" int dl_afm_grid(int32_t B) {
  // at most 512 blocks, as dl_cross_grid: the slab dl_adam_dense sums is bounded whatever the batch
  int g = (B + 15) / 16;
  if (g > 512) g = 512;
  return g < 1 ? 1 : g;
}

static int afm_check(const char* name, int32_t B, int32_t F, int32_t E, int32_t A, const float* x0, int32_t ld,
                     int32_t x_col0, const float* prm) {
  DL_CHECK_ARG(B >= 0, "%s: B %d < 0", name, B);
  DL_CHECK_ARG(F >= 2 && F <= kAfmMaxF, "%s: F %d fields not in [2, %d]", name, F, kAfmMaxF);
  DL_CHECK_ARG(E == 8 || E == 16 || E == 32, "%s: E %d not one of 8, 16, 32", name, E);
  DL_CHECK_ARG(A >= 1 && A <= kAfmMaxA, "%s: A %d attention units not in [1, %d]", name, A, kAfmMaxA);
  DL_CHECK_ARG(x0 && prm && x_col0 >= 0 && (long long)x_col0 + (long long)F * E <= ld,
               "%s: x0 and params required, field columns [%d, %d) within ld %d", name, x_col0, x_col0 + F * E, ld);
  return 0;
}

static int afm_ap(int A) { return A <= 8 ? 8 : A <= 16 ? 16 : 32; }

extern "C" int dl_afm_fwd(int32_t B, int32_t F, int32_t E, int32_t A, const float* x0, int32_t ld, int32_t x_col0,
                          const float* params, const float* z_add, float* stats, float* z_out, void* stream) {
  if (int rc = afm_check("dl_afm_fwd", B, F, E, A, x0, ld, x_col0, params)) return rc;
  DL_CHECK_ARG(stats && z_out, "dl_afm_fwd: stats and z_out required");
  if (B == 0) return 0;
  const int AP = afm_ap(A), nw = 4, spw = F <= 32 ? 2 : 1;
  const size_t lds = (size_t)(E + 2 * AP + E * AP + nw * 64 * (E + 4)) * sizeof(float);   // <= 41 KB
  long long grid = ((long long)B + nw * spw - 1) / (nw * spw);
  if (grid > 2048) grid = 2048;
#define DL_AFM_FWD(EE)                                                                                          \
  case EE:                                                                                                      \
    hipLaunchKernelGGL(afm_fwd_kernel<EE>, dim3((unsigned)grid), dim3(64 * nw), lds, as_stream(stream), B, F,   \
                       A, AP, x0, ld, x_col0, params, z_add, stats, z_out);                                     \
    break;
  switch (E) { DL_AFM_FWD(8) DL_AFM_FWD(16) DL_AFM_FWD(32) }
#undef DL_AFM_FWD
  DL_RETURN_LAUNCH("dl_afm_fwd");
}

extern "C" int dl_afm_bwd(int32_t B, int32_t F, int32_t E, int32_t A, const float* x0, int32_t ld, int32_t x_col0,
                          const float* params, const float* stats, const float* dz, float* dx0, int32_t dx_ld,
                          int32_t dx_col0, float* slab, int32_t slab_rows, void* stream) {
  if (int rc = afm_check("dl_afm_bwd", B, F, E, A, x0, ld, x_col0, params)) return rc;
  DL_CHECK_ARG(stats && dz && dx0 && slab, "dl_afm_bwd: stats, dz, dx0 and slab required");
  DL_CHECK_ARG(dx_col0 >= 0 && (long long)dx_col0 + (long long)F * E <= dx_ld,
               "dl_afm_bwd: dx0 columns [%d, %d) outside dx_ld %d", dx_col0, dx_col0 + F * E, dx_ld);
  const int grid = dl_afm_grid(B);
  DL_CHECK_ARG(slab_rows >= grid, "dl_afm_bwd: slab needs %d rows", grid);
  if (B == 0) return 0;
  // the waves of a block: as many of 4, 2, 1 as keep its LDS within 64 KB (E = 32, A = 32, F = 64: one)
  const int AP = afm_ap(A), R = F / 2;
  const size_t par = (size_t)(E + 2 * AP + E * AP), per_wave = (size_t)(2 * 64 * (E + 4) + R * 64 + 2 * 64 * (AP + 4));
  int nw = 4;
  while (nw > 1 && (par + nw * per_wave) * sizeof(float) > 65536) nw >>= 1;
  const size_t lds = (par + nw * per_wave) * sizeof(float);
#define DL_AFM_BWD(EE, AA)                                                                                      \
  case EE * 64 + AA:                                                                                            \
    hipLaunchKernelGGL((afm_bwd_kernel<EE, AA>), dim3(grid), dim3(64 * nw), lds, as_stream(stream), B, F, A,    \
                       x0, ld, x_col0, params, stats, dz, dx0, dx_ld, dx_col0, slab);                           \
    break;
#define DL_AFM_BWD_E(EE) DL_AFM_BWD(EE, 8) DL_AFM_BWD(EE, 16) DL_AFM_BWD(EE, 32)
  switch (E * 64 + AP) { DL_AFM_BWD_E(8) DL_AFM_BWD_E(16) DL_AFM_BWD_E(32) }
#undef DL_AFM_BWD_E
#undef DL_AFM_BWD
  DL_RETURN_LAUNCH("dl_afm_bwd");
}
