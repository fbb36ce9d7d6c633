// Exact tie-aware ROC-AUC on the GPU — the evaluation metric of the reference
// (sklearn.metrics.roc_auc_score at models/deepfm_pipeline.py:311,344, wdl.py:343-358).
// No library kernels: the sort is the hand-written stable radix sort of rsort.hip (the one
// the batch index build uses), the scan below is this file's own.
//
// AUC = sum over tie groups g of pos_g * (neg_below_g + 0.5 * neg_g) / (P * N)
// (a positive counts every negative scored below it and half of each negative tied with it).
// Steps:
//   1. keys[i] = order-preserving bits of score i; rsort_pairs sorts (key, i) stably
//   2. per sorted position j: label bit of the sample it holds, head bit (first of a tie group)
//      packed as one int64 v[j] = label + (head << 32); exclusive scan of v gives, at every
//      position, the positives before it (low word) and the number of groups that started
//      before it (high word)
//   3. at every group head j (group g = high word): start[g] = j, cpos[g] = positives before j
//   4. per group: e = next group's start (or n), pos_g = cpos[g+1] - cpos[g], neg_g = e - s - pos_g,
//      neg_below = s - cpos[g]; 2 * numerator += pos_g * (2 * neg_below + neg_g) — an exact
//      int64 sum (order-free, deterministic), divided once in double at the end.
#include "common.h"
#include "rsort.h"

namespace dl {
namespace {

constexpr int kScanThreads = 256;
constexpr int kScanPer = 16;                            // elements per thread
constexpr int kScanTile = kScanThreads * kScanPer;      // 4096

struct AucWs {
  uint32_t* keys;        // float keys (input order)
  uint32_t* skeys;       // sorted keys
  int32_t* sidx;         // sorted sample indices
  uint64_t* v;           // packed label / head bits, then their exclusive scan (in place)
  uint64_t* tsum;        // per-tile sums, then their exclusive scan
  int32_t* gstart;       // start position of group g
  int32_t* gcpos;        // positives before group g
  int32_t* n_valid;      // rsort's count (every key is valid)
  unsigned long long* acc;   // [0] = 2 * numerator, [1] = P, [2] = groups
  void* sort_ws;
  size_t sort_ws_bytes;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
int scan_tiles(int n) { return (n + kScanTile - 1) / kScanTile; }

AucWs carve(void* ws, int n) {
  char* p = static_cast<char*>(ws);
  AucWs w;
  const int T = scan_tiles(n);
  w.keys = reinterpret_cast<uint32_t*>(p); p += align256(4ull * n);
  w.skeys = reinterpret_cast<uint32_t*>(p); p += align256(4ull * n);
  w.sidx = reinterpret_cast<int32_t*>(p); p += align256(4ull * n);
  w.v = reinterpret_cast<uint64_t*>(p); p += align256(8ull * n);
  w.tsum = reinterpret_cast<uint64_t*>(p); p += align256(8ull * (T + 1));
  w.gstart = reinterpret_cast<int32_t*>(p); p += align256(4ull * (n + 1));
  w.gcpos = reinterpret_cast<int32_t*>(p); p += align256(4ull * (n + 1));
  w.n_valid = reinterpret_cast<int32_t*>(p); p += 256;
  w.acc = reinterpret_cast<unsigned long long*>(p); p += 256;
  w.sort_ws = p;
  w.sort_ws_bytes = rsort_workspace_bytes(n);
  return w;
}

size_t ws_bytes(int n) {
  const int T = scan_tiles(n);
  return 3 * align256(4ull * n) + align256(8ull * n) + align256(8ull * (T + 1)) + 2 * align256(4ull * (n + 1)) +
         512 + rsort_workspace_bytes(n);
}

// order-preserving map of a float to uint32 (-0.0 folded onto +0.0: they tie, as np.diff says)
__device__ __forceinline__ uint32_t float_key(float x) {
  uint32_t u = __float_as_uint(x == 0.f ? 0.f : x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void auc_keys_kernel(const float* __restrict__ scores, int64_t s_stride, int n,
                                                       uint32_t* __restrict__ keys, unsigned long long* acc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 4) acc[threadIdx.x] = 0;
  if (i < n) keys[i] = float_key(scores[(int64_t)i * s_stride]);
}

// v[j] = label of the sample at sorted position j + (j starts a tie group) << 32
__global__ __launch_bounds__(256) void auc_flags_kernel(const uint32_t* __restrict__ sk, const int32_t* __restrict__ si,
                                                        const float* __restrict__ labels, int64_t l_stride, int n,
                                                        uint64_t* __restrict__ v) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = sk[j];
  const int idx = min(max(si[j], 0), n - 1);
  const uint64_t lab = labels[(int64_t)idx * l_stride] > 0.5f ? 1u : 0u;
  const uint64_t head = (j == 0 || sk[j - 1] != k) ? 1u : 0u;
  v[j] = lab | (head << 32);
}

// Block-wide exclusive scan of one uint64 per thread; *total = the block's sum.
__device__ __forceinline__ uint64_t block_exscan(uint64_t x, uint64_t* wsum, uint64_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  __syncthreads();
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint64_t base = 0, all = 0;
#pragma unroll
  for (int i = 0; i < kScanThreads / 64; ++i) {
    base += i < w ? wsum[i] : 0;
    all += wsum[i];
  }
  *total = all;
  return base + inc - x;
}

// Pass 1: the sum of each 4096-element tile.
__global__ __launch_bounds__(kScanThreads) void scan_tile_sums(const uint64_t* __restrict__ v, int n,
                                                               uint64_t* __restrict__ tsum) {
  __shared__ uint64_t wsum[kScanThreads / 64];
  const long long t0 = (long long)blockIdx.x * kScanTile;
  uint64_t s = 0;
#pragma unroll
  for (int r = 0; r < kScanPer; ++r) {
    const long long e = t0 + r * kScanThreads + threadIdx.x;
    s += e < n ? v[e] : 0;
  }
  uint64_t all;
  block_exscan(s, wsum, &all);
  if (threadIdx.x == 0) tsum[blockIdx.x] = all;
}

// Pass 2 (one block): exclusive scan of the tile sums in place; tsum[T] = the grand total.
__global__ __launch_bounds__(kScanThreads) void scan_tile_prefix(uint64_t* __restrict__ tsum, int T) {
  __shared__ uint64_t wsum[kScanThreads / 64];
  const int per = (T + kScanThreads - 1) / kScanThreads;
  const int a = threadIdx.x * per, b = min(T, a + per);
  uint64_t s = 0;
  for (int i = a; i < b; ++i) s += tsum[i];
  uint64_t all;
  uint64_t run = block_exscan(s, wsum, &all);
  for (int i = a; i < b; ++i) {
    const uint64_t c = tsum[i];
    tsum[i] = run;
    run += c;
  }
  if (threadIdx.x == 0) tsum[T] = all;
}

// Pass 3: each tile's exclusive scan (thread-contiguous runs of kScanPer elements), offset by
// the tile's prefix; at every group head j: gstart[g] = j, gcpos[g] = positives before j.
// HEADS = false: the plain scan of full 64-bit values (dl_gauc's term prefix), nothing recorded.
template <bool HEADS>
__global__ __launch_bounds__(kScanThreads) void scan_tile_apply(uint64_t* __restrict__ v, int n,
                                                                const uint64_t* __restrict__ tsum,
                                                                int32_t* __restrict__ gstart,
                                                                int32_t* __restrict__ gcpos) {
  __shared__ uint64_t wsum[kScanThreads / 64];
  const long long e0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanPer;
  uint64_t x[kScanPer];
  uint64_t s = 0;
#pragma unroll
  for (int r = 0; r < kScanPer; ++r) {
    x[r] = e0 + r < n ? v[e0 + r] : 0;
    s += x[r];
  }
  uint64_t all;
  uint64_t run = block_exscan(s, wsum, &all) + tsum[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kScanPer; ++r) {
    const long long e = e0 + r;
    if (e < n) {
      v[e] = run;
      if (HEADS && (x[r] >> 32)) {   // a group head: run's high word = groups before it = its group index
        const uint32_t g = (uint32_t)(run >> 32);
        gstart[g] = (int32_t)e;
        gcpos[g] = (int32_t)(run & 0xffffffffu);
      }
    }
    run += x[r];
  }
}

// Per group g: its positives times (2 x negatives below it + its own negatives).
__global__ __launch_bounds__(256) void auc_groups_kernel(const int32_t* __restrict__ gstart,
                                                         const int32_t* __restrict__ gcpos,
                                                         const uint64_t* __restrict__ tsum, int T, int n,
                                                         unsigned long long* acc) {
  const uint64_t tot = tsum[T];
  const long long G = (long long)(tot >> 32);
  const long long P = (long long)(tot & 0xffffffffu);
  unsigned long long num = 0;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (long long)gridDim.x * blockDim.x) {
    const long long s = gstart[g];
    const long long e = g + 1 < G ? gstart[g + 1] : n;
    const long long c0 = gcpos[g];
    const long long c1 = g + 1 < G ? gcpos[g + 1] : P;
    const long long pos = c1 - c0;
    const long long neg = (e - s) - pos;
    const long long below = s - c0;
    num += (unsigned long long)(pos * (2 * below + neg));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) num += __shfl_xor(num, o, 64);
  if ((threadIdx.x & 63) == 0 && num) atomicAdd(acc, num);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    acc[1] = (unsigned long long)P;
    acc[2] = (unsigned long long)G;
  }
}

__global__ void auc_final_kernel(const unsigned long long* acc, int n, double* out) {
  const double P = (double)acc[1], N = (double)n - P;
  out[0] = (P == 0.0 || N == 0.0) ? __builtin_nan("") : (double)acc[0] / (2.0 * P * N);
}

// ---------------------------------------------------------------------------
// Per-group AUC (dl_gauc): the pipeline above, segmented by a group id.
//   1. sort (float_key(score), i) as dl_auc does: skeys / sidx, score-ascending
//   2. gkey[j] = group id of the sample at score position j (checked: an id outside [0, 2^31)
//      raises the error word and is keyed 0, the result is then NaN); a second stable sort of
//      (gkey[j], j) gives spos: position k holds score position spos[k], group-major and
//      score-ascending within each group
//   3. per position k: label bit, tie-run head (new key, or new group), group head;
//      scan A of label | run head << 32 records every tie run's start and positive prefix
//      (rstart / rcpos, as dl_auc's groups), scan B of run head | group head << 32 every group's
//      start and first run (gstart / grun)
//   4. per tie run t of group g: pos (2 below + neg) with below = the group's own negatives before
//      the run = (start_t - gstart_g) - (rcpos_t - rcpos[grun_g]), an exact uint64, 0 past the last
//      run; scan C (plain) of the terms
//   5. per group: 2 x numerator = the term prefix's difference at the group's run boundaries,
//      P_g and n_g likewise; one double term w_g num2_g / (2 P_g N_g) for a valid group, summed per
//      4096-group tile in a fixed order (thread-serial, then a shuffle tree), the tile partials by
//      one block: no atomics, the same bits on every call.
struct GaucWs {
  int32_t* err;          // [0] the error word (DL_STATUS_BAD_ID), [1] rsort's count
  uint32_t* keys;        // float keys (input order), then the group keys at score positions
  uint32_t* skeys;       // score-sorted keys
  int32_t* sidx;         // score-sorted sample indices
  uint32_t* sgk;         // group-major group keys
  int32_t* spos;         // group-major score positions
  uint64_t* va;          // label | run head, its scan, then the run terms and their scan
  uint64_t* vb;          // run head | group head, then its scan
  uint64_t* tsa;         // tile sums of the three scans
  uint64_t* tsb;
  uint64_t* tsc;
  int32_t* rstart;       // tie run t: start position, positives before it
  int32_t* rcpos;
  int32_t* gstart;       // group g: start position, its first tie run
  int32_t* grun;
  double* part;          // per group tile: the double sum, covered samples, valid groups (as uint64 bits)
  void* sort_ws;
  size_t sort_ws_bytes;
};

size_t gauc_carve(void* ws, int n, GaucWs* w) {
  char* p = static_cast<char*>(ws);
  const int T = scan_tiles(n);
  GaucWs g;
  g.err = reinterpret_cast<int32_t*>(p); p += 256;
  g.keys = reinterpret_cast<uint32_t*>(p); p += align256(4ull * n);
  g.skeys = reinterpret_cast<uint32_t*>(p); p += align256(4ull * n);
  g.sidx = reinterpret_cast<int32_t*>(p); p += align256(4ull * n);
  g.sgk = reinterpret_cast<uint32_t*>(p); p += align256(4ull * n);
  g.spos = reinterpret_cast<int32_t*>(p); p += align256(4ull * n);
  g.va = reinterpret_cast<uint64_t*>(p); p += align256(8ull * n);
  g.vb = reinterpret_cast<uint64_t*>(p); p += align256(8ull * n);
  g.tsa = reinterpret_cast<uint64_t*>(p); p += align256(8ull * (T + 1));
  g.tsb = reinterpret_cast<uint64_t*>(p); p += align256(8ull * (T + 1));
  g.tsc = reinterpret_cast<uint64_t*>(p); p += align256(8ull * (T + 1));
  g.rstart = reinterpret_cast<int32_t*>(p); p += align256(4ull * (n + 1));
  g.rcpos = reinterpret_cast<int32_t*>(p); p += align256(4ull * (n + 1));
  g.gstart = reinterpret_cast<int32_t*>(p); p += align256(4ull * (n + 1));
  g.grun = reinterpret_cast<int32_t*>(p); p += align256(4ull * (n + 1));
  g.part = reinterpret_cast<double*>(p); p += align256(24ull * T);
  g.sort_ws = p;
  g.sort_ws_bytes = rsort_workspace_bytes(n);
  if (w) *w = g;
  return (size_t)(p - static_cast<char*>(ws)) + g.sort_ws_bytes;
}

__global__ __launch_bounds__(256) void gauc_keys_kernel(const float* __restrict__ scores, int64_t s_stride, int n,
                                                        uint32_t* __restrict__ keys, int32_t* err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 2) err[threadIdx.x] = 0;
  if (i < n) keys[i] = float_key(scores[(int64_t)i * s_stride]);
}

// gkey[j] = the group id of the sample at score position j
__global__ __launch_bounds__(256) void gauc_gkeys_kernel(const int32_t* __restrict__ si,
                                                         const int64_t* __restrict__ groups, int64_t g_stride, int n,
                                                         uint32_t* __restrict__ gkey, int32_t* err) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int idx = min(max(si[j], 0), n - 1);
  const int64_t id = groups[(int64_t)idx * g_stride];
  const bool ok = id >= 0 && id <= 0x7fffffffLL;
  if (!ok) atomicOr(err, 1);   // DL_STATUS_BAD_ID
  gkey[j] = ok ? (uint32_t)id : 0u;
}

__global__ __launch_bounds__(256) void gauc_flags_kernel(const uint32_t* __restrict__ sk, const int32_t* __restrict__ si,
                                                         const uint32_t* __restrict__ sgk,
                                                         const int32_t* __restrict__ spos,
                                                         const float* __restrict__ labels, int64_t l_stride, int n,
                                                         uint64_t* __restrict__ va, uint64_t* __restrict__ vb) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int j = min(max(spos[k], 0), n - 1);
  const int idx = min(max(si[j], 0), n - 1);
  const uint64_t lab = labels[(int64_t)idx * l_stride] > 0.5f ? 1u : 0u;
  uint64_t gh = 1, rh = 1;
  if (k > 0) {
    const int jp = min(max(spos[k - 1], 0), n - 1);
    gh = sgk[k - 1] != sgk[k] ? 1u : 0u;
    rh = (gh || sk[jp] != sk[j]) ? 1u : 0u;
  }
  va[k] = lab | (rh << 32);
  vb[k] = rh | (gh << 32);
}

// term[t] of tie run t (0 past the last run), written over va
__global__ __launch_bounds__(256) void gauc_terms_kernel(const int32_t* __restrict__ rstart,
                                                         const int32_t* __restrict__ rcpos,
                                                         const int32_t* __restrict__ gstart,
                                                         const int32_t* __restrict__ grun,
                                                         const uint64_t* __restrict__ vb,
                                                         const uint32_t* __restrict__ sgk,
                                                         const uint64_t* __restrict__ tsa,
                                                         const uint64_t* __restrict__ tsb, int T, int n,
                                                         uint64_t* __restrict__ term) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const long long R = (long long)(tsa[T] >> 32), P = (long long)(tsa[T] & 0xffffffffu);
  const long long G = (long long)(tsb[T] >> 32);
  if (t >= R) {
    term[t] = 0;
    return;
  }
  const long long s = min(max(rstart[t], 0), n - 1);
  const long long e = t + 1 < R ? rstart[t + 1] : n;
  const long long c0 = rcpos[t];
  const long long c1 = t + 1 < R ? rcpos[t + 1] : P;
  const bool gh = s == 0 || sgk[s - 1] != sgk[s];
  long long g = (long long)(vb[s] >> 32) - (gh ? 0 : 1);   // heads before s: its own index at a head
  g = min(max(g, 0LL), max(G - 1, 0LL));
  const long long gs = gstart[g];
  const long long gc = rcpos[min(max(grun[g], 0), n - 1)];
  const long long pos = c1 - c0;
  const long long neg = (e - s) - pos;
  const long long below = (s - gs) - (c0 - gc);
  term[t] = (uint64_t)(pos * (2 * below + neg));
}

__device__ __forceinline__ double block_sum_f64(double x, double* sh) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  double r = 0;
#pragma unroll
  for (int i = 0; i < kScanThreads / 64; ++i) r += sh[i];
  return r;
}

__device__ __forceinline__ uint64_t block_sum_u64(uint64_t x, uint64_t* sh) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  uint64_t r = 0;
#pragma unroll
  for (int i = 0; i < kScanThreads / 64; ++i) r += sh[i];
  return r;
}

// One block per tile of 4096 group indices: part[b] = {sum of terms, covered samples, valid groups}.
__global__ __launch_bounds__(kScanThreads) void gauc_groups_kernel(const int32_t* __restrict__ gstart,
                                                                   const int32_t* __restrict__ grun,
                                                                   const int32_t* __restrict__ rcpos,
                                                                   const uint64_t* __restrict__ sterm,
                                                                   const uint64_t* __restrict__ tsa,
                                                                   const uint64_t* __restrict__ tsb,
                                                                   const uint64_t* __restrict__ tsc, int T, int n,
                                                                   int weighting, double* __restrict__ part) {
  __shared__ double shd[kScanThreads / 64];
  __shared__ uint64_t shu[kScanThreads / 64];
  const long long R = (long long)(tsa[T] >> 32), P = (long long)(tsa[T] & 0xffffffffu);
  const long long G = (long long)(tsb[T] >> 32);
  const uint64_t total = tsc[T];
  double sum = 0;
  uint64_t covered = 0, valid = 0;
  for (int r = 0; r < kScanPer; ++r) {
    const long long g = (long long)blockIdx.x * kScanTile + r * kScanThreads + threadIdx.x;
    if (g >= G) continue;
    const long long s = gstart[g], e = g + 1 < G ? gstart[g + 1] : n;
    const long long t0 = min(max(grun[g], 0), n - 1);
    const long long t1 = g + 1 < G ? min(max(grun[g + 1], 0), n - 1) : R;
    const long long pg = (t1 < R ? rcpos[t1] : P) - rcpos[t0];
    const uint64_t num2 = (t1 < R ? sterm[t1] : total) - sterm[t0];
    const long long ng = e - s, neg = ng - pg;
    if (pg > 0 && neg > 0) {
      const double auc = (double)num2 / (2.0 * (double)pg * (double)neg);
      sum += weighting == 0 ? (double)ng * auc : auc;
      covered += (uint64_t)ng;
      valid += 1;
    }
  }
  const double bs = block_sum_f64(sum, shd);
  const uint64_t bc = block_sum_u64(covered, shu);
  const uint64_t bv = block_sum_u64(valid, shu);
  if (threadIdx.x == 0) {
    part[3 * blockIdx.x] = bs;
    reinterpret_cast<uint64_t*>(part)[3 * blockIdx.x + 1] = bc;
    reinterpret_cast<uint64_t*>(part)[3 * blockIdx.x + 2] = bv;
  }
}

__global__ __launch_bounds__(kScanThreads) void gauc_final_kernel(const double* __restrict__ part,
                                                                  const uint64_t* __restrict__ tsb, int T,
                                                                  int weighting, const int32_t* __restrict__ err,
                                                                  double* __restrict__ out) {
  __shared__ double shd[kScanThreads / 64];
  __shared__ uint64_t shu[kScanThreads / 64];
  double sum = 0;
  uint64_t covered = 0, valid = 0;
  for (int b = threadIdx.x; b < T; b += kScanThreads) {
    sum += part[3 * b];
    covered += reinterpret_cast<const uint64_t*>(part)[3 * b + 1];
    valid += reinterpret_cast<const uint64_t*>(part)[3 * b + 2];
  }
  sum = block_sum_f64(sum, shd);
  covered = block_sum_u64(covered, shu);
  valid = block_sum_u64(valid, shu);
  if (threadIdx.x == 0) {
    const double nan = __builtin_nan("");
    if (err[0]) {
      out[0] = out[1] = out[2] = out[3] = nan;
    } else {
      const double den = weighting == 0 ? (double)covered : (double)valid;
      out[0] = valid ? sum / den : nan;
      out[1] = (double)covered;
      out[2] = (double)valid;
      out[3] = (double)(tsb[T] >> 32);
    }
  }
}

// ---------------------------------------------------------------------------
// dl_eval_stats: log-loss / score / label sums in double, two stages in a fixed order.
constexpr int kStatsPer = 8;           // elements per thread and round
constexpr int kStatsMaxBlocks = 1024;

int stats_blocks(int64_t n) {
  const int64_t b = (n + kScanThreads * kStatsPer - 1) / (kScanThreads * kStatsPer);
  return (int)std::min<int64_t>(std::max<int64_t>(b, 1), kStatsMaxBlocks);
}

__global__ __launch_bounds__(kScanThreads) void stats_partial_kernel(const float* __restrict__ scores, int64_t s_stride,
                                                                     const float* __restrict__ labels, int64_t l_stride,
                                                                     long long n, double eps,
                                                                     double* __restrict__ part) {
  __shared__ double shd[kScanThreads / 64];
  double loss = 0, sp = 0, sy = 0;
  for (long long i = (long long)blockIdx.x * kScanThreads + threadIdx.x; i < n;
       i += (long long)gridDim.x * kScanThreads) {
    const double p = (double)scores[i * s_stride];
    const bool y = labels[i * l_stride] > 0.5f;
    loss += y ? -log(p + eps) : -log(1.0 - p + eps);
    sp += p;
    sy += y ? 1.0 : 0.0;
  }
  loss = block_sum_f64(loss, shd);
  sp = block_sum_f64(sp, shd);
  sy = block_sum_f64(sy, shd);
  if (threadIdx.x == 0) {
    part[3 * blockIdx.x] = loss;
    part[3 * blockIdx.x + 1] = sp;
    part[3 * blockIdx.x + 2] = sy;
  }
}

__global__ __launch_bounds__(kScanThreads) void stats_final_kernel(const double* __restrict__ part, int blocks,
                                                                   long long n, double* __restrict__ out) {
  __shared__ double shd[kScanThreads / 64];
  double loss = 0, sp = 0, sy = 0;
  for (int b = threadIdx.x; b < blocks; b += kScanThreads) {
    loss += part[3 * b];
    sp += part[3 * b + 1];
    sy += part[3 * b + 2];
  }
  loss = block_sum_f64(loss, shd);
  sp = block_sum_f64(sp, shd);
  sy = block_sum_f64(sy, shd);
  if (threadIdx.x == 0) {
    out[0] = loss;
    out[1] = sp;
    out[2] = sy;
    out[3] = (double)n;
  }
}

// dl_eval_stats_weighted: the same two stages over five sums {w l, w p, w y, w, [w != 0]}.  A
// weight outside [0, inf) enters as NaN, so the four weighted sums come out NaN.
constexpr int kWStats = 5;

__global__ __launch_bounds__(kScanThreads) void wstats_partial_kernel(const float* __restrict__ scores, int64_t s_stride,
                                                                      const float* __restrict__ labels, int64_t l_stride,
                                                                      const float* __restrict__ weights,
                                                                      int64_t w_stride, long long n, double eps,
                                                                      double* __restrict__ part) {
  __shared__ double shd[kScanThreads / 64];
  double v[kWStats] = {};
  for (long long i = (long long)blockIdx.x * kScanThreads + threadIdx.x; i < n;
       i += (long long)gridDim.x * kScanThreads) {
    const double p = (double)scores[i * s_stride];
    const bool y = labels[i * l_stride] > 0.5f;
    const float wf = weights[i * w_stride];
    const double w = (wf >= 0.f && wf <= 3.402823466e38f) ? (double)wf : __longlong_as_double(0x7ff8000000000000ll);
    v[0] += w * (y ? -log(p + eps) : -log(1.0 - p + eps));
    v[1] += w * p;
    v[2] += y ? w : 0.0;
    v[3] += w;
    v[4] += wf != 0.f ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < kWStats; ++k) {
    const double t = block_sum_f64(v[k], shd);
    if (threadIdx.x == 0) part[kWStats * blockIdx.x + k] = t;
  }
}

__global__ __launch_bounds__(kScanThreads) void wstats_final_kernel(const double* __restrict__ part, int blocks,
                                                                    double* __restrict__ out) {
  __shared__ double shd[kScanThreads / 64];
  double v[kWStats] = {};
  for (int b = threadIdx.x; b < blocks; b += kScanThreads)
#pragma unroll
    for (int k = 0; k < kWStats; ++k) v[k] += part[kWStats * b + k];
#pragma unroll
  for (int k = 0; k < kWStats; ++k) {
    const double t = block_sum_f64(v[k], shd);
    if (threadIdx.x == 0) out[k] = t;
  }
}

}  // namespace
}  // namespace dl

using namespace dl;

extern "C" int64_t dl_auc_workspace_bytes(int64_t n) {
  if (n <= 0 || n > 0x7fffffff) return -1;
  return (int64_t)ws_bytes((int)n);
}

extern "C" int dl_auc(const float* scores, int64_t s_stride, const float* labels, int64_t l_stride, int64_t n,
                      void* ws, int64_t ws_bytes_, double* out, void* stream) {
  DL_CHECK_ARG(scores && labels && out && ws, "NULL argument");
  DL_CHECK_ARG(n > 0 && n <= 0x7fffffff, "n = %lld out of range", (long long)n);
  DL_CHECK_ARG(ws_bytes_ >= dl_auc_workspace_bytes(n), "workspace too small (%lld < %lld)", (long long)ws_bytes_,
               (long long)dl_auc_workspace_bytes(n));
  const int m = (int)n;
  hipStream_t s = as_stream(stream);
  AucWs w = carve(ws, m);
  const int g = (m + 255) / 256;
  hipLaunchKernelGGL(auc_keys_kernel, dim3(g), dim3(256), 0, s, scores, s_stride, m, w.keys, w.acc);
  RsSource src{};
  src.kind = 0;
  src.keys = w.keys;
  if (int rc = rsort_pairs(src, m, 0, 32, w.sort_ws, w.sort_ws_bytes, w.skeys, w.sidx, w.n_valid, s)) {
    set_error("dl_auc: radix sort failed (%d)", rc);
    return rc;
  }
  hipLaunchKernelGGL(auc_flags_kernel, dim3(g), dim3(256), 0, s, w.skeys, w.sidx, labels, l_stride, m, w.v);
  const int T = scan_tiles(m);
  hipLaunchKernelGGL(scan_tile_sums, dim3(T), dim3(kScanThreads), 0, s, w.v, m, w.tsum);
  hipLaunchKernelGGL(scan_tile_prefix, dim3(1), dim3(kScanThreads), 0, s, w.tsum, T);
  hipLaunchKernelGGL(scan_tile_apply<true>, dim3(T), dim3(kScanThreads), 0, s, w.v, m, w.tsum, w.gstart, w.gcpos);
  hipLaunchKernelGGL(auc_groups_kernel, dim3(std::min(g, 2048)), dim3(256), 0, s, w.gstart, w.gcpos, w.tsum, T, m,
                     w.acc);
  hipLaunchKernelGGL(auc_final_kernel, dim3(1), dim3(1), 0, s, w.acc, m, out);
  DL_RETURN_LAUNCH("dl_auc");
}

extern "C" int64_t dl_gauc_workspace_bytes(int64_t n) {
  if (n <= 0 || n > 0x7fffffff) return -1;
  return (int64_t)gauc_carve(nullptr, (int)n, nullptr);
}

extern "C" int dl_gauc(const float* scores, int64_t s_stride, const float* labels, int64_t l_stride,
                       const int64_t* groups, int64_t g_stride, int64_t n, int32_t weighting, void* ws,
                       int64_t ws_bytes_, double* out, void* stream) {
  DL_CHECK_ARG(scores && labels && groups && out && ws, "NULL argument");
  DL_CHECK_ARG(n > 0 && n <= 0x7fffffff, "n = %lld out of range", (long long)n);
  DL_CHECK_ARG(weighting == 0 || weighting == 1, "weighting = %d (0: group size, 1: uniform)", (int)weighting);
  DL_CHECK_ARG(((uintptr_t)ws & 255) == 0, "workspace not 256-B aligned");
  DL_CHECK_ARG(ws_bytes_ >= dl_gauc_workspace_bytes(n), "workspace too small (%lld < %lld)", (long long)ws_bytes_,
               (long long)dl_gauc_workspace_bytes(n));
  const int m = (int)n;
  hipStream_t s = as_stream(stream);
  GaucWs w;
  gauc_carve(ws, m, &w);
  const int g = (m + 255) / 256;
  hipLaunchKernelGGL(gauc_keys_kernel, dim3(g), dim3(256), 0, s, scores, s_stride, m, w.keys, w.err);
  RsSource src{};
  src.kind = 0;
  src.keys = w.keys;
  if (int rc = rsort_pairs(src, m, 0, 32, w.sort_ws, w.sort_ws_bytes, w.skeys, w.sidx, w.err + 1, s)) {
    set_error("dl_gauc: radix sort of the scores failed (%d)", rc);
    return rc;
  }
  // the score keys are sorted: their buffer takes the group keys (31 bits, never rsort's dropped key)
  hipLaunchKernelGGL(gauc_gkeys_kernel, dim3(g), dim3(256), 0, s, w.sidx, groups, g_stride, m, w.keys, w.err);
  if (int rc = rsort_pairs(src, m, 0, 31, w.sort_ws, w.sort_ws_bytes, w.sgk, w.spos, w.err + 1, s)) {
    set_error("dl_gauc: radix sort of the group ids failed (%d)", rc);
    return rc;
  }
  hipLaunchKernelGGL(gauc_flags_kernel, dim3(g), dim3(256), 0, s, w.skeys, w.sidx, w.sgk, w.spos, labels, l_stride, m,
                     w.va, w.vb);
  const int T = scan_tiles(m);
  hipLaunchKernelGGL(scan_tile_sums, dim3(T), dim3(kScanThreads), 0, s, w.va, m, w.tsa);
  hipLaunchKernelGGL(scan_tile_prefix, dim3(1), dim3(kScanThreads), 0, s, w.tsa, T);
  hipLaunchKernelGGL(scan_tile_apply<true>, dim3(T), dim3(kScanThreads), 0, s, w.va, m, w.tsa, w.rstart, w.rcpos);
  hipLaunchKernelGGL(scan_tile_sums, dim3(T), dim3(kScanThreads), 0, s, w.vb, m, w.tsb);
  hipLaunchKernelGGL(scan_tile_prefix, dim3(1), dim3(kScanThreads), 0, s, w.tsb, T);
  hipLaunchKernelGGL(scan_tile_apply<true>, dim3(T), dim3(kScanThreads), 0, s, w.vb, m, w.tsb, w.gstart, w.grun);
  hipLaunchKernelGGL(gauc_terms_kernel, dim3(g), dim3(256), 0, s, w.rstart, w.rcpos, w.gstart, w.grun, w.vb, w.sgk,
                     w.tsa, w.tsb, T, m, w.va);
  hipLaunchKernelGGL(scan_tile_sums, dim3(T), dim3(kScanThreads), 0, s, w.va, m, w.tsc);
  hipLaunchKernelGGL(scan_tile_prefix, dim3(1), dim3(kScanThreads), 0, s, w.tsc, T);
  hipLaunchKernelGGL(scan_tile_apply<false>, dim3(T), dim3(kScanThreads), 0, s, w.va, m, w.tsc, nullptr, nullptr);
  hipLaunchKernelGGL(gauc_groups_kernel, dim3(T), dim3(kScanThreads), 0, s, w.gstart, w.grun, w.rcpos, w.va, w.tsa,
                     w.tsb, w.tsc, T, m, (int)weighting, w.part);
  hipLaunchKernelGGL(gauc_final_kernel, dim3(1), dim3(kScanThreads), 0, s, w.part, w.tsb, T, (int)weighting, w.err,
                     out);
  DL_RETURN_LAUNCH("dl_gauc");
}

extern "C" int64_t dl_eval_stats_workspace_bytes(int64_t n) {
  if (n <= 0 || n > 0x7fffffff) return -1;
  return 24ll * stats_blocks(n);
}

extern "C" int dl_eval_stats(const float* scores, int64_t s_stride, const float* labels, int64_t l_stride, int64_t n,
                             double eps, void* ws, int64_t ws_bytes_, double* out, void* stream) {
  DL_CHECK_ARG(scores && labels && out && ws, "NULL argument");
  DL_CHECK_ARG(n > 0 && n <= 0x7fffffff, "n = %lld out of range", (long long)n);
  DL_CHECK_ARG(((uintptr_t)ws & 7) == 0, "workspace not 8-B aligned");
  DL_CHECK_ARG(ws_bytes_ >= dl_eval_stats_workspace_bytes(n), "workspace too small (%lld < %lld)",
               (long long)ws_bytes_, (long long)dl_eval_stats_workspace_bytes(n));
  hipStream_t s = as_stream(stream);
  const int blocks = stats_blocks(n);
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(stats_partial_kernel, dim3(blocks), dim3(kScanThreads), 0, s, scores, s_stride, labels, l_stride,
                     (long long)n, eps, part);
  hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(kScanThreads), 0, s, part, blocks, (long long)n, out);
  DL_RETURN_LAUNCH("dl_eval_stats");
}

extern "C" int64_t dl_eval_stats_weighted_workspace_bytes(int64_t n) {
  if (n <= 0 || n > 0x7fffffff) return -1;
  return 8ll * kWStats * stats_blocks(n);
}

extern "C" int dl_eval_stats_weighted(const float* scores, int64_t s_stride, const float* labels, int64_t l_stride,
                                      const float* weights, int64_t w_stride, int64_t n, double eps, void* ws,
                                      int64_t ws_bytes_, double* out, void* stream) {
  DL_CHECK_ARG(scores && labels && weights && out && ws, "NULL argument");
  DL_CHECK_ARG(n > 0 && n <= 0x7fffffff, "n = %lld out of range", (long long)n);
  DL_CHECK_ARG(((uintptr_t)ws & 7) == 0, "workspace not 8-B aligned");
  DL_CHECK_ARG(ws_bytes_ >= dl_eval_stats_weighted_workspace_bytes(n), "workspace too small (%lld < %lld)",
               (long long)ws_bytes_, (long long)dl_eval_stats_weighted_workspace_bytes(n));
  hipStream_t s = as_stream(stream);
  const int blocks = stats_blocks(n);
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(wstats_partial_kernel, dim3(blocks), dim3(kScanThreads), 0, s, scores, s_stride, labels,
                     l_stride, weights, w_stride, (long long)n, eps, part);
  hipLaunchKernelGGL(wstats_final_kernel, dim3(1), dim3(kScanThreads), 0, s, part, blocks, out);
  DL_RETURN_LAUNCH("dl_eval_stats_weighted");
}

// ---------------------------------------------------------------------------
// The measured HBM yardstick (bench.py roofline.peak_measured): a streaming copy, each block one
// chunk of 8 x 256 16-B pieces, all eight non-temporal loads in flight before the non-temporal
// stores — the fastest of the copy forms scripts/ubench_copy.hip measured on this chip (5.56
// TB/s at 1 and 4 GiB; grid-stride plain copies 4.2-4.7, torch's copy_ 5.0-5.2,
// profiles/r06d/ubench_copy.txt): what a read-once / write-once stream reaches here, beside the
// 8 TB/s specification the roofline fractions are priced against.
typedef unsigned int hbm_u4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void hbm_copy_kernel(const hbm_u4* __restrict__ src, hbm_u4* __restrict__ dst,
                                                       long long n16) {
  const long long c0 = (long long)blockIdx.x * 2048;
  hbm_u4 v[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const long long i = c0 + u * 256 + threadIdx.x;
    if (i < n16) v[u] = __builtin_nontemporal_load(src + i);
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const long long i = c0 + u * 256 + threadIdx.x;
    if (i < n16) __builtin_nontemporal_store(v[u], dst + i);
  }
}

extern "C" int dl_hbm_copy(const void* src, void* dst, int64_t bytes, void* stream) {
  DL_CHECK_ARG(src && dst && bytes >= 0 && bytes % 16 == 0, "dl_hbm_copy: bad arguments (bytes %lld)",
               (long long)bytes);
  DL_CHECK_ARG(((uintptr_t)src | (uintptr_t)dst) % 16 == 0, "dl_hbm_copy: 16-B alignment");
  if (bytes == 0) return 0;
  const long long n16 = bytes / 16;
  DL_CHECK_ARG((n16 + 2047) / 2048 < (1LL << 31), "dl_hbm_copy: too many bytes");
  hipLaunchKernelGGL(hbm_copy_kernel, dim3((unsigned)((n16 + 2047) / 2048)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const hbm_u4*>(src), reinterpret_cast<hbm_u4*>(dst), n16);
  DL_RETURN_LAUNCH("dl_hbm_copy");
}
