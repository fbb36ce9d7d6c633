/*
 * dlamd.h — C ABI of the MI355X-native CTR training hot path (libdlamd.so).
 *
 * The reference (RodJohn/deep_learning) is TensorFlow-1.x graph code: its hot
 * path is TF's own C++ kernels behind `sess.run(op)` ("Third-party
 * native arithmetic").  Each entry point below replaces one group of those TF
 * ops at a reference call site (cited per function).  Host code (Python,
 * deep_learning_amd/_lib.py) binds this header through ctypes.
 *
 * Conventions:
 *   - extern "C" only; device pointers (row-major, contiguous); explicit dims.
 *   - every call is asynchronous on the given HIP stream (`stream` is a
 *     hipStream_t passed as void*; NULL = default stream); no allocation and no
 *     host synchronisation inside any call, so a caller may capture a whole
 *     training step into a hipGraph.
 *   - return 0 on success, otherwise a nonzero code; the message is available
 *     from dl_last_error() (thread-local).  No C++ exception crosses the ABI.
 *   - out-of-range ids never fault: they read as zero rows and raise the
 *     caller-provided device error word (`err`, may be NULL) which the host
 *     turns into an exception (TF's InvalidArgumentError "indices[...] = k is
 *     not in [0, N)").
 */
#ifndef DLAMD_H
#define DLAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DL_ABI_VERSION 1

int dl_abi_version(void);
const char* dl_last_error(void);
/* hipDeviceSynchronize + error check (host utility, never inside a step). */
int dl_device_sync(void);

/* ------------------------------------------------------------------------
 * Embedding layout shared by the forward and backward embedding kernels.
 * One instance describes how a model maps a batch onto the table rows:
 *   FM fields  = [C cont fields (row fm_cont_offset+j, value cont[b][j]) if fm_cont]
 *              + [S single cate fields (row id+fm_cate_offset, value 1)]
 *              + [fm_extra pooled fields (vectors already in x0 at x0_pool_col,
 *                 first-order values already in fm_out at column fm_single)]
 *   deep input = x0[b][x0_cont_col..+C] = cont, x0[b][x0_vec_col..+V] = vector,
 *                x0[b][x0_cat_col + f*E ..] = table[id_f + deep_cate_offset]
 *   fm_out[b]  = [first (F = fm_single + fm_extra) | second (E)]
 * -------------------------------------------------------------------- */
typedef struct dl_emb_layout {
  int64_t n_rows;           /* rows of table [n_rows, E] and first-order [n_rows]   */
  int64_t fm_cont_offset;   /* deepfm_pipeline.py:58-61,89 (0); deepfm_multi.py:139 */
  int64_t fm_cate_offset;   /* deepfm_pipeline.py:89 (+C)                            */
  int64_t deep_cate_offset; /* deepfm_pipeline.py:120 (0: raw ids — ledger item 1)   */
  int32_t batch;            /* B                                                     */
  int32_t emb_dim;          /* E in {4, 8, 16, 32, 64}                               */
  int32_t cont_fields;      /* C                                                     */
  int32_t vector_size;      /* V                                                     */
  int32_t cate_fields;      /* S single-valued ids per sample                        */
  int32_t cate_ld;          /* int64 elements between samples in the id matrix       */
  int32_t fm_cont;          /* 1: the C cont fields are FM fields                    */
  int32_t use_fm;           /* 0: no FM outputs (dnn / wdl)                           */
  int32_t fm_extra;         /* M pooled multi-hot fields appended to the FM           */
  int32_t zero_row0;        /* 1: row 0 reads as zeros and gets no gradient (:83-86) */
  int32_t x0_ld;            /* floats between samples in x0                          */
  int32_t x0_cont_col;      /* -1: cont not copied into x0                           */
  int32_t x0_vec_col;       /* -1: vector not copied into x0                         */
  int32_t x0_cat_col;       /* column of the first single-cate embedding in x0 (-1:
                               not written — dl_embed_fwd / _slots / _indexed only, the
                               embeddings then read by dl_gemm_s3_nt_gather)          */
  int32_t x0_pool_col;      /* column of the first pooled vector in x0 (fm_extra>0)  */
  int32_t fm_ld;            /* floats between samples in fm_out                      */
  int32_t dx0_ld;           /* floats between samples in dx0 (backward)              */
  int32_t dx0_cat_col;      /* column of the first single-cate gradient in dx0       */
  int32_t multi_width;      /* multi-hot id columns after the S singles that the batch
                               index also covers (record path of deepfm_multi_cate; 0 = none):
                               index refs per sample = (use_fm ? S : 0) + S + multi_width */
  int32_t cont_rows_compact;/* 1: the FM cont-field rows are addressed as rows 0..C-1 of the
                               row buffer handed over (the gathered rows of the record and
                               sharded paths; their gradients in a [C] buffer), while which
                               of them is the zero row is still decided on the table row
                               fm_cont_offset + f (deepfm_multi.py:139 puts them after the
                               cate ids; deepfm_pipeline.py:58-61 at the top)           */
  int32_t x0_bf16;          /* 1: the forward's x0 is a bf16 matrix (uint16, x0_ld elements per
                               sample; the bf16 tower's first operand, config C5): cate, cont
                               and vector columns are written rounded to nearest-even.
                               Requires fm_extra == 0 (pooled vectors are read back as f32) */
} dl_emb_layout;

/* Embedding gather + FM first/second order + deep-input assembly (forward).
 * Replaces GatherV2 x3, ConcatV2 (row-0 zero), Mul/Sum/Square/Sub at
 * models/deepfm_pipeline.py:83-123 (also dnn_pipeline.py:72-83, wdl.py:132-179,
 * deepfm_multi_cate.py:127-171 for the single fields).
 * fm_sum [B, E] keeps sum_f e_f for the backward (may be NULL when !use_fm). */
int dl_embed_fwd(const dl_emb_layout* L, const float* table, const float* first_order,
                 const int64_t* cate, const float* cont, const float* vector,
                 float* x0, float* fm_out, float* fm_sum, int32_t* err, void* stream);
/* dl_embed_fwd over a slot plane [n_rows][2E] (dl_rec_flush with DL_REC_PLANE_SLOTS): row r's
 * embedding in columns 0..E-1, its first-order weight in column E — an FM reference's row and
 * weight in one 128-B slot (E = 16), one random request instead of two (predict on a flushed
 * lazy table; same outputs as dl_embed_fwd on separate planes, bit for bit). */
int dl_embed_fwd_slots(const dl_emb_layout* L, const float* slots, const int64_t* cate, const float* cont,
                       const float* vector, float* x0, float* fm_out, float* fm_sum, int32_t* err, void* stream);
/* The FM side of predict's fused front (with dl_gemm_s3_nt_gather_tab): dl_embed_fwd_slots
 * (slot_plane = 1) or dl_embed_fwd on the p plane (slot_plane = 0, models without FM) with
 * x0_cat_col = -1, which instead of the deep rows writes their byte offsets in the plane into
 * gtab ([ceil(B / 256)][fields][272] u32, 0xFFFFFF00 for a masked or invalid id — the first
 * tower layer's LDS table as it stands: 16 samples of a field one 64-B write).  x0 may be NULL
 * when x0_cont_col and x0_vec_col are -1 too (nothing of x0 written), fm_sum may be NULL
 * (predict: no backward reads it).  Same fm_out and x0 cont / vector columns as
 * dl_embed_fwd_slots bit for bit. */
int dl_embed_fwd_gtab_ok(const dl_emb_layout* L);   /* 1: the layout qualifies (E = 8 / 16, FM slots in <= 4 passes) */
int dl_embed_fwd_gtab(const dl_emb_layout* L, const float* plane, int32_t slot_plane, const int64_t* cate,
                      const float* cont, const float* vector, float* x0, float* fm_out, float* fm_sum, uint32_t* gtab,
                      int32_t* err, void* stream);

/* Backward of dl_embed_fwd for the FM (single fields) and deep lookups.
 * dz [B] = dL/dlogit, w_head = head weights whose first F+E entries weight
 * [first | second]; dx0 = dL/dx0.  Scatter-adds row gradients into the dense
 * gradient tables g_table [n_rows, E], g_first [n_rows] (f32 atomics), marks
 * touched rows in `touched` [n_rows] (uint8), and writes the hot cont-field
 * rows as per-block partials into cont_slab [grid][C*(E+1)] which
 * dl_embed_cont_reduce folds in.  Replaces the Gather gradients
 * (UnsortedSegmentSum) + StridedSliceGrad of deepfm_pipeline.py:188. */
int dl_embed_bwd(const dl_emb_layout* L, const float* table, const int64_t* cate,
                 const float* cont, const float* dz, const float* w_head,
                 const float* fm_sum, const float* dx0, float* g_table, float* g_first,
                 uint8_t* touched, float* cont_slab, int32_t cont_slab_blocks, void* stream);
int dl_embed_bwd_grid(const dl_emb_layout* L);   /* grid size = cont_slab blocks */
int dl_embed_cont_reduce(const dl_emb_layout* L, const float* cont_slab, int32_t blocks,
                         float* g_table, float* g_first, uint8_t* touched, void* stream);

/* Indexed forward (row-sharded tables): the row of reference ref = b*n_slot + slot
 * (index order of dl_index_build) is inv_base + inv[ref] in `rows` / `rows_first`
 * (the rows exchanged for this batch; rows below inv_base hold the replicated
 * cont-field rows read by the FM cont fields). */
int dl_embed_fwd_indexed(const dl_emb_layout* L, const float* rows, const float* rows_first,
                         const int32_t* inv, int32_t inv_base, const float* cont,
                         const float* vector, float* x0, float* fm_out, float* fm_sum,
                         void* stream);

/* The record forward on a flushed table (single GPU, lazy-exact Adam; every row caught up to
 * step opt[7]: after dl_rec_flush, before any further update): dl_embed_fwd with the cate rows
 * read straight from the row records (rec.hip layout) — each reference reads only its record's
 * first 128-B line (p, and the first-order weight beside it); a row whose stamp is not opt[7]
 * sets DL_STATUS_LAG (the host raises) instead of being read stale.  Same outputs as
 * dl_rec_gather + dl_embed_fwd_indexed at lag 0.  The C FM cont-field rows (every sample's) come
 * compact in rows_rep / rows_rep1 (dl_rec_gather with no unique rows); needs
 * L->cont_rows_compact when there are any.  Single-valued fields only (multi_width 0). */
int dl_embed_fwd_rec_flat(const dl_emb_layout* L, const float* rec, int32_t rec_ld, int32_t rec_flags,
                          const float* rows_rep, const float* rows_rep1, const int64_t* cate,
                          const float* cont, const float* vector, const float* opt, float* x0,
                          float* fm_out, float* fm_sum, int32_t* err, void* stream);

/* Hot cont-field rows only (the FM cont part of dl_embed_bwd): per-block
 * partials into cont_slab[0 .. min(cont_slab_blocks, dl_embed_bwd_grid)), folded in by
 * dl_embed_cont_reduce (blocks beyond the samples' share hold zeros, so passing only the
 * blocks that hold samples gives the same partials). */
int dl_embed_cont_bwd(const dl_emb_layout* L, const float* table, const float* cont,
                      const float* dz, const float* w_head, const float* fm_sum, float* cont_slab,
                      int32_t cont_slab_blocks, void* stream);

/* Batch reference index (index.hip): every (sample, slot) reference — slots are
 * the S FM cate fields (if use_fm) then the S deep fields — keyed by
 * (owner << 27 | local) with owner = row % world, local = row / world (rows below
 * replicated_below: owner = world, local = row); sorted (radix), deduplicated:
 * uniq_keys[0..n_uniq), segment offsets seg_off[0..n_uniq] into sorted_refs
 * (ref = b * n_slot + slot), inverse map inv[ref] -> unique id (-1 invalid; may be
 * NULL), owner_counts[world+1] unique rows per owner (may be NULL).
 * Invalid refs (row 0 under zero_row0, out-of-range -> err) are excluded. */
int64_t dl_index_workspace_bytes(int64_t n_refs);
int dl_index_build(const dl_emb_layout* L, const int64_t* cate, int32_t world,
                   int32_t replicated_below, void* ws, int64_t ws_bytes, uint32_t* sorted_keys,
                   int32_t* sorted_refs, uint32_t* uniq_keys, int32_t* seg_off, int32_t* n_uniq,
                   int32_t* inv, int32_t* owner_counts, int32_t* err, void* stream);
/* Two id sets indexed by ONE sort (single GPU, world 1): the table references of (L, cate) and
 * a second set (L2, cate2: the wdl wide ids, wdl.py:44-47 / :132 read wdl_weights through
 * embedding_lookup) keyed into owner groups 0 and 1 of one radix sort + segmented unique —
 * one launch sequence over n1 + n2 references in place of two builds over n1 and n2.
 * Outputs are exactly dl_index_build(L, cate, 1, 0, ...)'s for the first set (uniq_keys,
 * seg_off, n_uniq, inv; sorted_refs within its segments) and dl_index_build(L2, cate2, ...)'s
 * for the second (uniq2, seg_off2, n_uniq2, inv2, sorted_refs2), references numbered per set.
 * sorted_keys / sorted_refs / inv / uniq_keys / seg_off hold n1 + n2 (+1) entries; the second
 * set's arrays n2 (+1).  Workspace: dl_index_workspace_bytes(n1 + n2). */
int dl_index_build_pair(const dl_emb_layout* L, const int64_t* cate, const dl_emb_layout* L2,
                        const int64_t* cate2, void* ws, int64_t ws_bytes, uint32_t* sorted_keys,
                        int32_t* sorted_refs, uint32_t* uniq_keys, int32_t* seg_off, int32_t* n_uniq,
                        int32_t* inv, uint32_t* uniq2, int32_t* sorted_refs2, int32_t* seg_off2,
                        int32_t* n_uniq2, int32_t* inv2, int32_t* err, void* stream);
/* Generic form for the sharded owners: sort n int32 keys (< 2^key_bits; a key of -1 — an empty
 * slot of a fixed-capacity exchange block — is dropped) with their positions, dedup:
 * uniq_keys [n_uniq], seg_off [n_uniq+1] into sorted_pos, and inv[i] = unique id of keys[i]
 * (may be NULL).  Workspace: dl_index_workspace_bytes(n). */
int dl_sort_unique(const int32_t* keys, int64_t n_keys, int32_t key_bits, void* ws, int64_t ws_bytes,
                   int32_t* sorted_keys, int32_t* sorted_pos, int32_t* uniq_keys, int32_t* seg_off,
                   int32_t* n_uniq, int32_t* inv, void* stream);
/* Deterministic (atomic-free) embedding backward over the index: each unique
 * row's gradient is the ordered sum of its references.  compact=0: plain stores
 * into the dense gradient tables g_out [n_rows, E] / g1_out [n_rows] + touched
 * flags (single GPU); compact=1: g_out [u][E], g1_out [u] per unique id (the
 * sharded path sends these to the owners).  rows_u: gathered rows per unique id
 * (sharded) or NULL to read `table`.  upos (compact only, may be NULL): unique row u's slot in
 * rows_u / g_out / g1_out (the fixed-capacity exchange blocks of dl_shard_route; a slot of -1
 * is skipped) in place of u. */
int dl_embed_bwd_sorted(const dl_emb_layout* L, const float* table, const float* rows_u,
                        const uint32_t* uniq_keys, const int32_t* seg_off, const int32_t* n_uniq,
                        const int32_t* sorted_refs, int32_t world, int64_t max_uniq,
                        const float* dz, const float* w_head, const float* fm_sum,
                        const float* dx0, float* g_out, float* g1_out, uint8_t* touched,
                        int32_t compact, const int32_t* upos, void* stream);

/* Multi-hot nonzero-mean pooling (deepfm_multi_cate.py:71-111).
 * ids [B, ids_ld] int64 (padding id 0); slot m covers columns
 * [slot_start[m], slot_end[m]) of the multi-hot block that starts at column
 * ids_col.  Writes pooled vectors to x0[b][x0_pool_col + m*E ..], pooled
 * first-order to fm_out[b][fm_col + m] (if first_order != NULL) and the
 * integer counts cnt_emb / cnt_first [B, M] (float-valued, bit-exact). */
int dl_pool_fwd(const dl_emb_layout* L, const float* table, const float* first_order,
                const int64_t* ids, int32_t ids_col, const int32_t* slot_start,
                const int32_t* slot_end, int32_t n_slots, int32_t fm_col, float* x0,
                float* fm_out, float* cnt_emb, float* cnt_first, int32_t* err, void* stream);
/* Pooling over record rows (lazy Adam, L->multi_width > 0): the row of multi position l
 * of sample b is inv_base + inv[b*ns + (use_fm ? S : 0) + S + l] of rows/rows_first
 * (dl_rec_gather output, dl_index_build inv; -1 = padding id). */
int dl_pool_fwd_indexed(const dl_emb_layout* L, const float* rows, const float* rows_first,
                        const int32_t* inv, int32_t inv_base, const int32_t* slot_start,
                        const int32_t* slot_end, int32_t n_slots, int32_t fm_col, float* x0,
                        float* fm_out, float* cnt_emb, float* cnt_first, void* stream);
/* Backward of pooling: d pooled = dsecond*(fm_sum - pooled) + dx0[pool cols];
 * each slot id gets d/cnt (div_no_nan gradient), first-order likewise. */
int dl_pool_bwd(const dl_emb_layout* L, const int64_t* ids, int32_t ids_col,
                const int32_t* slot_start, const int32_t* slot_end, int32_t n_slots,
                int32_t fm_col, const float* x0, const float* fm_sum, const float* dz,
                const float* w_head, const float* dx0, int32_t dx0_pool_col,
                const float* cnt_emb, const float* cnt_first, float* g_table,
                float* g_first, uint8_t* touched, void* stream);
/* Weighted nonzero-mean pooling (models/dnn_multi_textline.py:94-103, the deep-only
 * multi-hot lookup of the textline DNN): pooled = div_no_nan(sum_l value_l * V[id_l], cnt)
 * with cnt = count_nonzero(sum_E V[id_l]) of the UNweighted rows (:94-95).  values [B,
 * values_ld] f32, the value of multi position l (same column numbering as the slot ranges,
 * relative to ids_col).  The frozen word2vec table of slot 'tag' (:45-47,85-88) is a
 * separate dl_pool_fwd_weighted call with that table and no backward.  The backward
 * scatter-adds value_l * d pooled / cnt into g_table (f32 atomics) and marks touched. */
int dl_pool_fwd_weighted(const dl_emb_layout* L, const float* table, const int64_t* ids,
                         int32_t ids_col, const float* values, int32_t values_ld,
                         const int32_t* slot_start, const int32_t* slot_end, int32_t n_slots,
                         float* x0, float* cnt_emb, int32_t* err, void* stream);
int dl_pool_bwd_weighted(const dl_emb_layout* L, const int64_t* ids, int32_t ids_col,
                         const float* values, int32_t values_ld, const int32_t* slot_start,
                         const int32_t* slot_end, int32_t n_slots, const float* dx0,
                         int32_t dx0_pool_col, const float* cnt_emb, float* g_table,
                         uint8_t* touched, void* stream);

/* ------------------------------------------------------------------------
 * Dense tower: fp32 GEMM on v_mfma_f32_16x16x4_f32 (exact fp32, k-ordered fma).
 * C[i][j] (op) sum_r A(i,r) B(r,j); A(i,r) = ta ? A[r*lda+i] : A[i*lda+r];
 * B(r,j) = tb ? B[j*ldb+r] : B[r*ldb+j].
 * epi: 0 store, 1 ReLU (bias folded as a ones column), 2 multiply by
 * (mask[i*ldm+j] > 0) (ReluGrad), 3 split-K partial slabs:
 * C + z*c_split_stride for split z of `splits` (K chunks of a multiple of 16).
 * Requirements: lda, ldb, ldc multiples of 4; the contiguous extent of each
 * operand a multiple of 4 (zero padded). Replaces MatMul+Add+Relu
 * (deepfm_pipeline.py:150-152) and their gradients. */
int dl_gemm_f32(int32_t ta, int32_t tb, int32_t M, int32_t N, int32_t K, const float* A,
                int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc, int32_t epi,
                const float* mask, int32_t ldm, int32_t splits, int64_t c_split_stride,
                void* stream);
/* dst[c*ldd + r] = src[r*lds + c] (r < rows, c < cols): W^T for the dX product, so
 * both dX operands are read from LDS images in their HBM layout. */
int dl_transpose_f32(const float* src, int32_t rows, int32_t cols, int32_t lds, float* dst, int32_t ldd,
                     void* stream);
/* dst[r*ldd + c] = bf16(src[r*lds + c]), round to nearest even (bf16 tower operands). */
int dl_cast_bf16(const float* src, int32_t rows, int32_t cols, int32_t lds, uint16_t* dst, int32_t ldd,
                 void* stream);
/* dst[c*ldd + r] = bf16(src[r*lds + c]) (src f32 when src_f32, else bf16): the k-contiguous
 * operand copies of the bf16 tower (W^T, X^T, dY^T). */
int dl_transpose_bf16(const void* src, int32_t src_f32, int32_t rows, int32_t cols, int32_t lds,
                      uint16_t* dst, int32_t ldd, void* stream);
/* bf16 variant for the Wide&Deep tower (config C5): A, B bf16 (uint16 bits),
 * fp32 accumulate, C fp32 or bf16 (c_bf16 = 1). Same semantics otherwise.  ta = 0, tb = 1
 * with lda, ldb multiples of 8 and 16-B aligned operands takes the fast k-contiguous
 * kernel (b128 LDS images, BK = 64); other forms a general element-staged kernel. */
int dl_gemm_bf16(int32_t ta, int32_t tb, int32_t M, int32_t N, int32_t K, const uint16_t* A,
                 int32_t lda, const uint16_t* B, int32_t ldb, void* C, int32_t ldc,
                 int32_t c_bf16, int32_t epi, const void* mask, int32_t ldm, int32_t splits,
                 int64_t c_split_stride, void* stream);

/* fp32 tower products on the bf16 matrix cores, three-plane split (gemm_s3.hip):
 * every f32 operand splits exactly into bf16 planes hi + mid + lo and a product takes the
 * six significant plane products (hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi) in f32
 * accumulation: f32 accuracy (dropped terms <= 2^-25 |a.b|) at up to 2.7x the f32 MFMA rate.
 * Replaces dl_gemm_f32 for deepfm_pipeline.py:150-152 and its gradients.
 *
 * dl_split3: planes of src [rows][cols] (ld lds) at dst + q * plane_stride (q = 0 hi,
 *   1 mid, 2 lo), [r][c] with ld ldd, or [c][r] when `transpose`.  In a library built with
 *   DL_S3_KPERM (dl_s3_kperm() == 1) the k index (the row position: c, or r when transposed;
 *   K = cols, or rows) of every whole 32-deep chunk is stored permuted — position
 *   8q + j (j < 4) holds k = 4q + j, position 8q + 4 + j holds k = 16 + 4q + j — the order
 *   dl_gemm_s3_nt reads; a trailing partial chunk keeps natural order.
 * dl_gemm_s3_nt: C[M][N] = A[M][K] . B[N][K]^T (+ epilogue: 0 store, 1 ReLU, 2 mask
 *   (C = mask[i][j] > 0 ? C : 0, mask f32 with ld ldm)); A f32 (lda % 4 == 0, 16-B
 *   aligned), B as planes from dl_split3 (ldb % 8 == 0, plane stride b_plane); K % 8 == 0.
 * dl_gemm_s3_tn: split-K weight gradient, slab z of C (at C + z * c_split_stride, ld ldc)
 *   = sum over k in split z of X[k][m] Y[k][n]; X [K][lda], Y [K][ldb] f32, N <= 416;
 *   splits of ceil(K / splits) rounded up to 64 rows (ceil(K / that) slabs). */
int dl_split3(const float* src, int32_t rows, int32_t cols, int32_t lds, int32_t transpose, uint16_t* dst,
              int32_t ldd, int64_t plane_stride, void* stream);
int dl_s3_kperm(void);
int dl_gemm_s3_nt(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const uint16_t* B,
                  int32_t ldb, int64_t b_plane, float* C, int32_t ldc, int32_t epi, const float* mask,
                  int32_t ldm, void* stream);
int dl_gemm_s3_tn(int32_t M, int32_t N, int32_t K, const float* X, int32_t lda, const float* Y, int32_t ldb,
                  float* C, int32_t ldc, int32_t splits, int64_t c_split_stride, void* stream);
/* dl_gemm_s3_nt_bits: dl_gemm_s3_nt with the ReLU sign bitmask — bits [M][ldbits] uint16,
 * bit (c & 15) of halfword [i][c >> 4] = (C[i][c] > 0), ldbits >= ceil(N / 16).  epi 1 (ReLU)
 * also writes the bitmask when bits != NULL; epi 3 applies the ReluGrad mask from it
 * (C = bit ? C : 0) in place of epi 2's f32 mask rows: 2 bytes per 16 columns read instead of
 * 64 (the tower's dX, deepfm_pipeline.py:150-152 gradients). */
int dl_gemm_s3_nt_bits(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const uint16_t* B,
                       int32_t ldb, int64_t b_plane, float* C, int32_t ldc, int32_t epi, const float* mask,
                       int32_t ldm, uint16_t* bits, int32_t ldbits, void* stream);
/* dl_gemm_s3_nt_gather: dl_gemm_s3_nt_bits (epi 0 / 1) for the first tower layer of the
 * flushed-table forward with the embedding lookup fused into its A stream (the north star's
 * "gather into tiles feeding MFMA"; replaces the GatherV2 -> ConcatV2 -> MatMul chain of
 * deepfm_pipeline.py:117-153 / dnn_pipeline.py:72-96 at predict): columns [0, fields * emb_dim)
 * of A's row m are not read from A but from table row (ids[m * ids_ld + f] + id_offset) —
 * f = k / emb_dim, column k % emb_dim, table rows table_ld floats apart (the slot or p plane
 * of dl_rec_flush) — a row outside [0, n_rows), or row 0 with zero_row0, reads as zeros (the
 * lookup's zero row; the lookup itself reports invalid ids).  The remaining columns come from A
 * (the cont / vector / bias columns the lookup writes with x0_cat_col = -1).  Bit-identical
 * to dl_embed_fwd(_slots) writing those columns followed by dl_gemm_s3_nt_bits.  Requires
 * emb_dim in {8, 16, 32, 64}, fields * emb_dim a multiple of 32 and <= K, fields <= 40,
 * n_rows * table_ld * 4 < 0xFFFFFF00 bytes (one buffer range). */
int dl_gemm_s3_nt_gather(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* table,
                         int64_t n_rows, int32_t table_ld, const int64_t* ids, int32_t ids_ld, int64_t id_offset,
                         int32_t zero_row0, int32_t fields, int32_t emb_dim, const uint16_t* B, int32_t ldb,
                         int64_t b_plane, float* C, int32_t ldc, int32_t epi, uint16_t* bits, int32_t ldbits,
                         void* stream);
/* dl_gemm_s3_nt_gather_rows: the training form — the deep rows of the batch's compact caught-up
 * rows (dl_rec_gather's rows_u) through the batch index's inverse map: row idx_base + idx[m *
 * idx_ld + f] (idx < 0: the zero row), and the gathered columns also written into A (x0) by the
 * first column tile's blocks, for the weight gradient that streams x0 (the lookup then runs with
 * x0_cat_col = -1).  Bit-identical to dl_embed_fwd_indexed writing those columns followed by
 * dl_gemm_s3_nt_bits. */
int dl_gemm_s3_nt_gather_rows(int32_t M, int32_t N, int32_t K, float* A, int32_t lda, const float* rows,
                              int64_t n_rows, int32_t rows_ld, const int32_t* idx, int32_t idx_ld, int32_t idx_base,
                              int32_t fields, int32_t emb_dim, const uint16_t* B, int32_t ldb, int64_t b_plane,
                              float* C, int32_t ldc, int32_t epi, uint16_t* bits, int32_t ldbits, void* stream);
/* dl_gemm_s3_nt_gather_tab: dl_gemm_s3_nt_gather with the rows resolved beforehand — the deep
 * rows' byte offsets come in gtab (dl_embed_fwd_gtab's table, staged into the block's LDS as it
 * stands, one contiguous copy instead of the ids' loads and range checks: entry
 * [m / 256][f * 272 + m % 256], 0xFFFFFF00 = a zero row); A's other columns from A (x0 with its
 * cont / ones columns written).  Bit-identical to dl_embed_fwd(_slots) + dl_gemm_s3_nt_bits
 * and to dl_gemm_s3_nt_gather.  gtab holds ceil(M / 256) * fields * 272 u32, 16-B aligned. */
int dl_gemm_s3_nt_gather_tab(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* table,
                             int64_t n_rows, int32_t table_ld, const uint32_t* gtab, int32_t fields, int32_t emb_dim,
                             const uint16_t* B, int32_t ldb, int64_t b_plane, float* C, int32_t ldc, int32_t epi,
                             uint16_t* bits, int32_t ldbits, void* stream);

/* ------------------------------------------------------------------------
 * Dropout of the deep tower (the reference's dropout_keep_deep: tf.nn.dropout after the tower
 * input and after every ReLU layer, deepfm_pipeline.py:148-153).  The mask is a pure function,
 * never stored:
 *   keep(seed, step, layer, row, col) = word (col & 3) of
 *       Philox-4x32-10(counter = (row, col >> 2, layer, step), key = (seed & 0xffffffff, seed >> 32))
 *       < keep_thr,       keep_thr = min(floor(keep * 2^32), 2^32 - 1)
 * (the counter's and the output's words in the order x, y, z, w of Salmon et al.'s definition;
 * all fields unsigned 32-bit).  One Philox call yields the four consecutive columns
 * 4 (col >> 2) .. + 3 of one row: what one lane of the s3 NT epilogue stores.  row and col are
 * the element's indices in the tensor as the engine lays it out (x0's columns in its internal
 * order); layer 0 is the tower input, layer i + 1 the output of hidden layer i; step is
 * (uint32) opt[7], read on the device, so a replayed graph draws a new mask every step.  A kept
 * element is multiplied by inv = float32(1) / float32(keep) (computed by the caller, one f32
 * multiply), a dropped one is 0.
 * dl_gemm_s3_nt_drop: dl_gemm_s3_nt_bits, epi 1 or 3 only.
 *   epi 1: v = relu(acc); C = keep ? v * inv : 0; bitmask bit = (v > 0) & keep (bits may be
 *          NULL; bits of columns >= N in the last halfword are 0).
 *   epi 3: C = bit ? C * inv : 0 — reads the combined mask epi 1 wrote, no RNG.
 * dl_dropout_apply: x[M][ld] (columns [0, N) only) = keep ? x * inv : 0 in place; mask_out (may
 *   be NULL; uint8 [M][N]) receives the keep bits; x == NULL: only mask_out is written. */
int dl_gemm_s3_nt_drop(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const uint16_t* B,
                       int32_t ldb, int64_t b_plane, float* C, int32_t ldc, int32_t epi, const float* mask,
                       int32_t ldm, uint16_t* bits, int32_t ldbits, uint32_t keep_thr, float inv, uint64_t seed,
                       int32_t layer, const float* opt, void* stream);
int dl_dropout_apply(float* x, int32_t M, int32_t N, int32_t ld, uint32_t keep_thr, float inv, uint64_t seed,
                     int32_t layer, const float* opt, uint8_t* mask_out, void* stream);

/* Dropout of the FM part (the reference's dropout_keep_fm: tf.nn.dropout(first_order_mul, keep_fm[0])
 * and tf.nn.dropout(second_order, keep_fm[1]), deepfm_pipeline.py:98,110).  The same function,
 * key, threshold and inv; row is the sample's index in the batch, and two more layer ids, far
 * from the tower's 0 .. len(hidden):
 *   DL_DROP_LAYER_FM1: first order, col = the FM column j in [0, F), in fm_out's own column
 *                      order (cont fields, cate fields, pooled slots);
 *   DL_DROP_LAYER_FM2: second order, col = the embedding dim d in [0, E).
 * A keep of exactly 1 (keep_thr = 2^32 - 1, inv = 1) keeps every element with factor 1 and no
 * threshold compare is made, so keeps (1, k) leave the first-order part as without dropout.
 *   forward:  fm_out'[b][j] = keep ? fm_out[b][j] * inv : 0 before the output layer (fm_out in
 *             memory is not rewritten; fm_sum stays the undropped sum);
 *   backward: dfm[b][j] = keep ? (dz[b] * w_head[j]) * inv : 0 replaces dz[b] * w_head[j]
 *             wherever an FM backward forms that product — this order of multiplication in
 *             every kernel; the second-order gradient is dfm[b][F + d] * (fm_sum[b][d] - v).
 * dl_head_fwd_bwd_fmdrop: dl_head_fwd_bwd whose lanes draw the keep bit of the FM column they
 *   loaded and mask / scale it before the reduction (z, score, dz, dh and the slab are those of
 *   dl_head_fwd_bwd on the dropped features, bit for bit), and which writes the keep bits to
 *   fm_keep [B][2] (16-B aligned): bit c of word k is column 64 k + c, columns >= fm_cols 0.
 *   F: the first-order columns [0, F); the rest, [F, fm_cols), are the second order's.
 * dl_fm_drop: what the FM backward twins read instead of drawing the mask again — the stored
 *   bits and the two factors.  dl_embed_bwd_fmdrop, dl_embed_bwd_sorted_fmdrop,
 *   dl_embed_cont_bwd_fmdrop, dl_pool_bwd_fmdrop and dl_rec_bwd_adam_fmdrop are their plain
 *   namesakes with that descriptor before the stream; the plain entry points and their
 *   kernels are unchanged. */
#define DL_DROP_LAYER_FM1 (1 << 16)
#define DL_DROP_LAYER_FM2 ((1 << 16) + 1)
typedef struct dl_fm_drop {
  const uint64_t* fm_keep; /* [B][2], written by dl_head_fwd_bwd_fmdrop */
  float inv1;              /* first order: float32(1) / float32(keep_fm[0]) */
  float inv2;              /* second order */
} dl_fm_drop;
int dl_embed_bwd_fmdrop(const dl_emb_layout* L, const float* table, const int64_t* cate,
                        const float* cont, const float* dz, const float* w_head,
                        const float* fm_sum, const float* dx0, float* g_table, float* g_first,
                        uint8_t* touched, float* cont_slab, int32_t cont_slab_blocks, const dl_fm_drop* drop,
                        void* stream);
int dl_embed_cont_bwd_fmdrop(const dl_emb_layout* L, const float* table, const float* cont,
                             const float* dz, const float* w_head, const float* fm_sum, float* cont_slab,
                             int32_t cont_slab_blocks, const dl_fm_drop* drop, void* stream);
int dl_embed_bwd_sorted_fmdrop(const dl_emb_layout* L, const float* table, const float* rows_u,
                               const uint32_t* uniq_keys, const int32_t* seg_off, const int32_t* n_uniq,
                               const int32_t* sorted_refs, int32_t world, int64_t max_uniq,
                               const float* dz, const float* w_head, const float* fm_sum,
                               const float* dx0, float* g_out, float* g1_out, uint8_t* touched,
                               int32_t compact, const int32_t* upos, const dl_fm_drop* drop, void* stream);
int dl_pool_bwd_fmdrop(const dl_emb_layout* L, const int64_t* ids, int32_t ids_col,
                       const int32_t* slot_start, const int32_t* slot_end, int32_t n_slots,
                       int32_t fm_col, const float* x0, const float* fm_sum, const float* dz,
                       const float* w_head, const float* dx0, int32_t dx0_pool_col,
                       const float* cnt_emb, const float* cnt_first, float* g_table,
                       float* g_first, uint8_t* touched, const dl_fm_drop* drop, void* stream);

/* ------------------------------------------------------------------------
 * Output layer + sigmoid + eps-log-loss, forward and backward fused
 * (deepfm_pipeline.py:157-183, dnn_pipeline.py:119-131):
 * z = [fm_out(F+E) | h(H)] . w + w[F+E+H];  p = sigmoid(z);
 * loss_b = -y ln(p+eps) - (1-y) ln(1-p+eps);  dz = (dL/dp) p (1-p) / B;
 * dh = dz * w_h * (h > 0) written into dh [B, ldh] (cols < H);
 * per-block partials: slab[block][0..F+E+H) = sum dz*feat, [F+E+H] = sum dz,
 * [F+E+H+1] = sum loss_b.  `fm_cols` = F+E (0 for dnn). inv_batch = 1/B_global. */
int dl_head_fwd_bwd(int32_t B, int32_t fm_cols, int32_t H, const float* fm_out, int32_t fm_ld,
                    const float* h, int32_t ldh, const float* w, const float* label,
                    float eps, float inv_batch, float* score, float* z_out, float* dz,
                    float* dh, float* slab, int32_t slab_blocks, void* stream);
/* With FM-part dropout ("Dropout" above). */
int dl_head_fwd_bwd_fmdrop(int32_t B, int32_t fm_cols, int32_t H, const float* fm_out, int32_t fm_ld,
                           const float* h, int32_t ldh, const float* w, const float* label,
                           float eps, float inv_batch, float* score, float* z_out, float* dz,
                           float* dh, float* slab, int32_t slab_blocks, int32_t F, uint32_t keep_thr1, float inv1,
                           uint32_t keep_thr2, float inv2, uint64_t seed, const float* opt, uint64_t* fm_keep,
                           void* stream);
int dl_head_grid(int32_t B);
/* Blocks (= slab rows) of dl_wdl_head_fwd_bwd[_bf16] for batch B. */
int dl_wdl_head_grid(int32_t B);

/* ------------------------------------------------------------------------
 * Cross network of Deep & Cross beside the dnn_* tower (test_model/DCN.py:73-96), on the
 * tower input x0 [B, ld] (its first D columns), L layers:
 *   x_0 = x0;  s_l = x_l . w_l;  x_{l+1} = x0 * s_l + b_l + x_l  (l < L);  z_cross = x_L . c
 * params: (2L + 1) vectors of D floats, [c | w_0 .. w_{L-1} | b_0 .. b_{L-1}], in x0's column
 * order.  D <= 1024 and 1 <= L <= 4; anything else is refused.
 * dl_cross_fwd writes s [B, L] and z_cross [B] (x_L is never stored: HBM traffic is one read of
 * x0).  dl_cross_bwd rebuilds every x_l from x0, s and b, and with g_L = dz c, top down,
 *   t_l = g_{l+1} . x0;  dw_l += t_l x_l;  db_l += g_{l+1};  dx0 += g_{l+1} s_l;  g_l = g_{l+1} + t_l w_l
 * then dx0 += g_0 and dc += dz x_L.  dx0 [B, dx_ld] holds x0's columns [dx_col0, dx_col0 + dx_cols)
 * only (the embedding columns) and is added into; the batch sums of (dc, dw_l, db_l) are left as
 * per-block partials slab[block][(2L + 1) D] in the layout of params (dl_cross_grid(B) blocks, at
 * most 512; dl_adam_dense sums them in slab order).  No atomics: the same inputs give the same
 * bits on every run.  dl_head_fwd_bwd_cross[_weighted]: dl_head_fwd_bwd[_weighted] with
 * z_extra[b] (z_cross) added to the logit before the sigmoid. */
int dl_cross_grid(int32_t B);
int dl_cross_fwd(int32_t B, int32_t D, int32_t L, const float* x0, int32_t ld, const float* params,
                 float* s, float* z_cross, void* stream);
int dl_cross_bwd(int32_t B, int32_t D, int32_t L, const float* x0, int32_t ld, const float* params,
                 const float* s, const float* dz, float* dx0, int32_t dx_ld, int32_t dx_col0,
                 int32_t dx_cols, float* slab, int32_t slab_rows, void* stream);
int dl_head_fwd_bwd_cross(int32_t B, int32_t fm_cols, int32_t H, const float* fm_out, int32_t fm_ld,
                          const float* h, int32_t ldh, const float* w, const float* label,
                          float eps, float inv_batch, const float* z_extra, float* score, float* z_out,
                          float* dz, float* dh, float* slab, int32_t slab_blocks, void* stream);
int dl_head_fwd_bwd_cross_weighted(int32_t B, int32_t fm_cols, int32_t H, const float* fm_out, int32_t fm_ld,
                                   const float* h, int32_t ldh, const float* w, const float* label,
                                   float eps, const float* w_eff, const float* norm, const float* z_extra,
                                   float* score, float* z_out, float* dz, float* dh, float* slab,
                                   int32_t slab_blocks, void* stream);

/* ------------------------------------------------------------------------
 * Attentional pairwise interactions (AFM) beside the dnn_* tower: the pairwise-interaction and
 * attention layers of test_model/AFM.py:63-129 (variables :75-85, pair loop :92-101, attention
 * :104-118, projection :121-129) on the F embedded fields of x0 [B, ld], field i in columns
 * [x_col0 + i E, x_col0 + (i + 1) E).  Over the P = F (F - 1) / 2 pairs i < j:
 *   q_ij = e_i * e_j;  u_ij = q_ij W + b;  s_ij = h . relu(u_ij);
 *   a_ij = exp(s_ij - max s) / sum exp(s - max s);  z_afm = (sum a_ij q_ij) . p
 * params: [p (E) | h (A) | b (A) | W (E A, row-major [E][A])].  2 <= F <= 64, E one of 8, 16, 32,
 * 1 <= A <= 32; anything else is refused.
 * dl_afm_fwd writes z_out[b] = z_afm[b] + (z_add ? z_add[b] : 0) (z_add: the cross network's
 * z_cross, so the head's one z_extra carries both) and stats [B, 2] = {max s, sum exp(s - max)};
 * nothing per pair goes to HBM.  dl_afm_bwd recomputes q, u and s from x0 and, with
 *   ds_ij = a_ij dz (q_ij . p - z_afm);  g_ij = ds_ij (h * [u_ij > 0]);  dq_ij = a_ij dz p + W g_ij
 * adds de_i += dq_ij * e_j, de_j += dq_ij * e_i INTO dx0 [B, dx_ld] columns [dx_col0, dx_col0 + F E)
 * and leaves the batch sums of (dp, dh, db, dW) as per-block partials slab[block][E + 2 A + E A]
 * in the layout of params (dl_afm_grid(B) blocks, at most 512; dl_adam_dense sums them in slab
 * order).  No atomics: the same inputs give the same bits on every run. */
int dl_afm_grid(int32_t B);
int dl_afm_fwd(int32_t B, int32_t F, int32_t E, int32_t A, const float* x0, int32_t ld, int32_t x_col0,
               const float* params, const float* z_add, float* stats, float* z_out, void* stream);
int dl_afm_bwd(int32_t B, int32_t F, int32_t E, int32_t A, const float* x0, int32_t ld, int32_t x_col0,
               const float* params, const float* stats, const float* dz, float* dx0, int32_t dx_ld,
               int32_t dx_col0, float* slab, int32_t slab_rows, void* stream);
/* ------------------------------------------------------------------------
 * Inner-product PNN (test_model/PNN.py:78-83, use_inner) on the first layer of the dnn_* tower:
 * over the F embedded fields of x0 [B, ld], field f in columns [x_col0 + f E, x_col0 + (f + 1) E),
 * with theta [D1][F] (row-major, the variable product-quadratic-inner):
 *   T_i = sum_f theta[i][f] e_f;  lp_i = sqrt(sum_e T_i[e]^2)
 * 2 <= F <= 64, E one of 8, 16, 32, D1 >= 1; anything else is refused and nothing is written.
 * T is formed per sample on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fma chain over the
 * fields) and never goes to HBM.
 * dl_pnn_inner_fwd finishes the layer in place: C [B, ldc] holds the pre-activation x0 W_0 + b_0
 * (the first layer's GEMM with epi 0) and becomes relu(C + lp) in columns [0, D1); with bits != NULL
 * the ReLU sign record is written in dl_gemm_s3_nt_bits' layout (bit c & 15 of halfword
 * bits[b * ldbits + (c >> 4)] = (C + lp > 0), zero bits past D1 in the last halfword;
 * ldbits >= ceil(D1 / 16)).
 * dl_pnn_inner_bwd recomputes T and lp and, with d [B, ldd] = dL/d(pre-activation) (the
 * ReluGrad-masked dh[0]) and dT_i = d_i T_i / lp_i (0 where lp_i == 0: tf.norm's NaN gradient at 0
 * is not reproduced), adds de_f = sum_i theta[i][f] dT_i INTO dx0 [B, dx_ld] columns
 * [dx_col0, dx_col0 + F E) and leaves dtheta[i][f] = sum_b sum_e dT_i[e] e_f[e] as per-block
 * partials slab[block][D1 F] in theta's layout (dl_pnn_grid(B) blocks, at most 512; dl_adam_dense
 * sums them in slab order).  No atomics: the same inputs give the same bits on every run. */
int dl_pnn_grid(int32_t B);
int dl_pnn_inner_fwd(int32_t B, int32_t F, int32_t E, int32_t D1, const float* x0, int32_t ld, int32_t x_col0,
                     const float* theta, float* C, int32_t ldc, uint16_t* bits, int32_t ldbits, void* stream);
int dl_pnn_inner_bwd(int32_t B, int32_t F, int32_t E, int32_t D1, const float* x0, int32_t ld, int32_t x_col0,
                     const float* theta, const float* d, int32_t ldd, float* dx0, int32_t dx_ld, int32_t dx_col0,
                     float* slab, int32_t slab_rows, void* stream);
/* ------------------------------------------------------------------------
 * Batch normalisation of a hidden layer (test_model/NFM.py:160-167, 244-252: nn.BatchNorm1d after
 * linear_i, before the activation) on the tower's stored pre-activation C [B, ldc] (the layer's
 * GEMM with epi 0), columns [0, D):
 *   mu_j = mean_b C[b][j];  var_j = mean_b (C[b][j] - mu_j)^2;  xhat = (C - mu) / sqrt(var + eps)
 *   y = gamma xhat + beta;  h = relu(y)
 * params [2 D] = [gamma | beta] (the layer's Adam vector).  With Dp = 16 ceil(D / 16):
 * stat [3 Dp] = [mu_hi | mu_lo | 1 / sqrt(var + eps)] (mu = mu_hi + mu_lo, so C - mu keeps f32
 * accuracy at any offset), sums [2 Dp] = [dgamma | dbeta].  ldc, ldx, ldd are multiples of 4 and
 * >= D, every matrix 16-B aligned; D < 1, a pitch below D and (statistics, backward) B < 2 are
 * refused and nothing is written.  Columns past D keep their bits.
 * dl_bn_grid(B): the row blocks of every kernel here (at most 1024, at least 32 rows each) = the
 * slab rows of the backward.
 * dl_bn_stats: per block the shifted sums (K = the block's first row; sum (c - K), sum (c - K)^2),
 * i.e. the block's (n, mean, M2), merged in block order in float64 by Chan's formula (never
 * E[c^2] - mu^2) into stat; with run_mean != NULL, and unless opt's step is poisoned
 * (dl_step_begin), running_mean <- (1 - m) running_mean + m mu and running_var <- (1 - m)
 * running_var + m var B / (B - 1).  ws: dl_bn_ws_floats(B, D) floats.
 * dl_bn_fwd finishes the layer in place: C becomes relu(gamma xhat + beta); with stat != NULL
 * (training) xhat comes from stat and is written to hx [B, ldx]; with stat == NULL (inference)
 * from run_mean / run_var / eps, and hx must be NULL.  With bits != NULL the ReLU sign record is
 * written in dl_gemm_s3_nt_bits' layout (bit c & 15 of halfword bits[b * ldbits + (c >> 4)] =
 * (y > 0), zero bits past D in the last halfword; ldbits >= ceil(D / 16)).
 * dl_bn_bwd_sums, dy [B, ldd] = dL/dy (the ReluGrad-masked dh): slab[block][2 D] = the block's
 * [sum_b dy xhat | sum_b dy], params' layout (dl_adam_dense sums the rows in slab order).
 * dl_bn_bwd_apply merges the slab's rows in order into sums and rewrites dy in place into
 *   dc = gamma / sqrt(var + eps) (dy - dbeta / B - xhat dgamma / B).
 * dl_bn_zero_bias_grad: the layer's own bias has dL/db = sum_b dc = 0 identically under batch norm;
 * the weight gradient's bias row (cols floats at `offset` of each of nslab split-K slabs, `stride`
 * floats apart) holds that sum's f32 rounding noise, which Adam would normalise into steps of the
 * order of lr, and is set to the exact 0.
 * No atomics, no memset: the same inputs give the same bits on every run. */
int dl_bn_zero_bias_grad(float* slab, int32_t nslab, int64_t stride, int64_t offset, int32_t cols, void* stream);
int dl_bn_grid(int32_t B);
int64_t dl_bn_ws_floats(int32_t B, int32_t D);
int dl_bn_stats(int32_t B, int32_t D, const float* C, int32_t ldc, float eps, float momentum, float* stat,
                float* run_mean, float* run_var, const float* opt, float* ws, int64_t ws_floats, void* stream);
int dl_bn_fwd(int32_t B, int32_t D, float* C, int32_t ldc, const float* stat, const float* run_mean,
              const float* run_var, float eps, const float* params, float* hx, int32_t ldx, uint16_t* bits,
              int32_t ldbits, void* stream);
int dl_bn_bwd_sums(int32_t B, int32_t D, const float* dy, int32_t ldd, const float* hx, int32_t ldx, float* slab,
                   int32_t slab_rows, void* stream);
int dl_bn_bwd_apply(int32_t B, int32_t D, float* dy, int32_t ldd, const float* hx, int32_t ldx,
                    const float* params, const float* stat, const float* slab, int32_t slab_rows, float* sums,
                    void* stream);
/* ------------------------------------------------------------------------
 * Bi-Interaction pooling (test_model/NFM.py:192-197, 226: fm_second_order fed to the deep layers)
 * over the F embedded fields of x0 [B, ld], field f in columns [x_col0 + f E, x_col0 + (f + 1) E):
 *   q[e] = sum_{f<g} e_f[e] e_g[e]  ( = 1/2 ((sum_f e_f)^2 - sum_f e_f^2) )
 * formed as the prefix chain q = sum_f e_f * P_f, P_f = sum_{g<f} e_g: one fma a field in field
 * order, never the difference of the two large sums.  2 <= F <= 64, E a multiple of 4 in [4, 64],
 * every column range within its pitch; anything else is refused and nothing is written.
 * dl_bi_grid(B): the sample blocks of both kernels (at most 1024, at least 32 samples each).
 * dl_bi_fwd writes q [B, ldq] columns [q_col0, q_col0 + E) and nothing else; q may be x0 itself
 * (then its columns must miss the fields').
 * dl_bi_bwd, with dq [B, lddq] columns [dq_col0, dq_col0 + E) = dL/dq and s = sum_g e_g, adds
 *   de_f = dq * (s - e_f)
 * INTO dx0 [B, dx_ld] columns [dx_col0, dx_col0 + F E) (the contract of dl_afm_bwd and
 * dl_pnn_inner_bwd: the three compose in any order) and writes nothing else; dq may be columns of
 * dx0 itself outside that range.  Accesses are 16 B wide when every pointer, pitch and column
 * offset is a multiple of 16 B, 4 B wide otherwise, with the same arithmetic.  No parameters, no
 * workspace, no atomics, no memset: the same inputs give the same bits on every run. */
int dl_bi_grid(int32_t B);
int dl_bi_fwd(int32_t B, int32_t F, int32_t E, const float* x0, int32_t ld, int32_t x_col0, float* q, int32_t ldq,
              int32_t q_col0, void* stream);
int dl_bi_bwd(int32_t B, int32_t F, int32_t E, const float* x0, int32_t ld, int32_t x_col0, const float* dq,
              int32_t lddq, int32_t dq_col0, float* dx0, int32_t dx_ld, int32_t dx_col0, void* stream);
/* The f32 vector-rate yardstick of scripts/afm_bench.py: `blocks` blocks of 256 threads, each thread
 * 16 independent chains of `iters` FMAs (32 * iters FLOP a thread, no memory traffic); out needs
 * blocks * 256 floats (n_out is checked). */
int dl_vfma_probe(float* out, int64_t n_out, int32_t blocks, int32_t iters, void* stream);

/* ------------------------------------------------------------------------
 * CCPM: convolutional field interactions beside the dnn_* tower: the Conv2D(3x3, same, relu) +
 * MaxPool2D(2x2) stack, Flatten and Dense(1) (without its bias) of test_model/CCPM.py:45-68 on the F
 * embedded fields of x0 [B, ld], field w in columns [x_col0 + w E, x_col0 + (w + 1) E).  With
 * X[h, w] = e_w[h], H = E, W = F, one input channel, for the L layers of filters[l] = C_l channels:
 *   u_l[h, w, c] = b_l[c] + sum_{dh, dw in -1..1} sum_c' K_l[dh+1, dw+1, c', c] a_{l-1}[h+dh, w+dw, c']
 *   a_l[i, j, c] = max over the 2x2 window of relu(u_l), H_l = H_{l-1} / 2, W_l = W_{l-1} / 2 (floor)
 *   z_ccpm = sum a_{L-1}[i, j, c] p[(i W_L + j) C_L + c]
 * params: [p (H_L W_L C_L) | K_0 (9 C_0, [3][3][1][C_0]) | b_0 | K_1 ([3][3][C_0][C_1]) | b_1 | ...].
 * 1 <= L <= 3, 1 <= C_l <= 8, 2 <= F <= 64, E one of 8, 16, 32, F >> L >= 1; anything else is refused
 * and nothing is written.  filters is a host array of L values.
 * dl_ccpm_fwd writes z_out[b] = z_ccpm[b] + (z_add ? z_add[b] : 0) (z_add: the logit of the cross
 * network and the attentional interactions, so the head's one z_extra carries all three).
 * dl_ccpm_bwd recomputes the forward from x0 (ReLU's derivative 0 at u <= 0, the pool's gradient to the
 * window's first maximum in (row, column) order), adds dX INTO dx0 [B, dx_ld] columns
 * [dx_col0, dx_col0 + F E) and leaves the batch sums of the parameter gradients as per-block partials
 * slab[block][n] in the layout of params (dl_ccpm_grid(B) blocks, at most 512; dl_adam_dense sums them
 * in slab order).  Every per-sample map lives in LDS; no atomics: the same inputs give the same bits
 * on every run. */
int dl_ccpm_grid(int32_t B);
int dl_ccpm_fwd(int32_t B, int32_t F, int32_t E, int32_t L, const int32_t* filters, const float* x0, int32_t ld,
                int32_t x_col0, const float* params, const float* z_add, float* z_out, void* stream);
int dl_ccpm_bwd(int32_t B, int32_t F, int32_t E, int32_t L, const int32_t* filters, const float* x0, int32_t ld,
                int32_t x_col0, const float* params, const float* dz, float* dx0, int32_t dx_ld, int32_t dx_col0,
                float* slab, int32_t slab_rows, void* stream);

/* ------------------------------------------------------------------------
 * Compressed Interaction Network (xDeepFM, Lian et al. 2018, eq. 6-8; direct form, identity activation,
 * no bias, no split-half) beside the dnn_* tower, on the F embedded fields of x0 [B, ld], field f in
 * columns [x_col0 + f E, x_col0 + (f + 1) E).  With X^0 = the fields [F, E], H_0 = F, for the L layers
 * of layers[k - 1] = H_k feature maps:
 *   X^k[h, e] = sum_{i < H_{k-1}} sum_{j < F} W^k[h, i, j] X^{k-1}[i, e] X^0[j, e]
 *   z_cin = sum_k sum_h c[off_k + h] sum_e X^k[h, e]
 * params: [c (sum H_k) | W^1 | W^2 | ..], W^k stored [H_{k-1} F, H_k] (row i F + j, column h).
 * 1 <= L <= 3, 1 <= H_k <= 64, 2 <= F <= 64, E one of 8, 16, 32, sum_k H_k H_{k-1} F <= 262,144;
 * anything else is refused and nothing is written.  layers is a host array of L values.
 * dl_cin_fwd writes z_out[b] = z_cin[b] + (z_add ? z_add[b] : 0) (z_add: the logit of the cross network,
 * the attentional interactions and the CCPM branch, so the head's one z_extra carries all four).
 * dl_cin_bwd recomputes the maps from x0, adds dX^0 INTO dx0 [B, dx_ld] columns
 * [dx_col0, dx_col0 + F E) and leaves the batch sums of the parameter gradients as per-block partials
 * slab[block][n] in the layout of params (dl_cin_grid(B) blocks, at most 128: at most 128 MB;
 * dl_adam_dense sums them in slab order).  Every layer is a GEMM on the exact f32 MFMA whose operand
 * X^{k-1}[i] * X^0[j] is formed in registers; no atomics: the same inputs give the same bits on every run. */
int dl_cin_grid(int32_t B);
int dl_cin_fwd(int32_t B, int32_t F, int32_t E, int32_t L, const int32_t* layers, const float* x0, int32_t ld,
               int32_t x_col0, const float* params, const float* z_add, float* z_out, void* stream);
int dl_cin_bwd(int32_t B, int32_t F, int32_t E, int32_t L, const int32_t* layers, const float* x0, int32_t ld,
               int32_t x_col0, const float* params, const float* dz, float* dx0, int32_t dx_ld, int32_t dx_col0,
               float* slab, int32_t slab_rows, void* stream);
/* The f32 matrix-rate yardstick of scripts/cin_bench.py: `blocks` blocks of 4 waves, each wave 8 independent
 * chains of `iters` v_mfma_f32_16x16x4_f32 (8 * 2048 * iters FLOP a wave, no memory traffic); out needs
 * blocks * 256 floats (n_out is checked). */
int dl_mfma_f32_probe(float* out, int64_t n_out, int32_t blocks, int32_t iters, void* stream);

/* ------------------------------------------------------------------------
 * AutoInt's interacting layers (Song et al. 2019, eq. 5-8) beside the dnn_* tower, on the F embedded fields
 * of x0 [B, ld], field f in columns [x_col0 + f E, x_col0 + (f + 1) E).  With X^0 = the fields [F, E],
 * D_0 = E, D_l = D, d = D / heads, for l = 1 .. L and X = X^{l-1}:
 *   Q = X Wq_l, K = X Wk_l, V = X Wv_l, R = X Wr_l   ([F, D]; W*_l [D_{l-1}, D] row-major, no bias)
 *   per head h (columns h d .. h d + d - 1): A_h = softmax_k(Q_h[i] . K_h[k]) (unscaled), O_h = A_h V_h
 *   X^l = relu(O + R)        z_autoint = sum_{f, c} w[f D + c] X^L[f, c]
 * params: [w (F D) | Wq_1 | Wk_1 | Wv_1 | Wr_1 | Wq_2 | ..].
 * 1 <= L <= 3, heads one of 1, 2, 4, D one of 8, 16, 32 with D / heads >= 2, 2 <= F <= 64, E one of 8, 16,
 * 32; anything else is refused and nothing is written.
 * dl_autoint_fwd writes z_out[b] = z_autoint[b] + (z_add ? z_add[b] : 0) (z_add: the logit of the branches
 * before it, so the head's one z_extra carries them all).
 * dl_autoint_bwd recomputes the layers from x0 (in LDS: no workspace), adds dX^0 INTO dx0 [B, dx_ld] columns
 * [dx_col0, dx_col0 + F E) and leaves the batch sums of the parameter gradients as per-block partials
 * slab[block][n] in the layout of params (dl_autoint_grid(B) blocks, at most 512: at most 30 MB;
 * dl_adam_dense sums them in slab order).  The projections and their gradients run on the exact f32 MFMA,
 * the attention on the vector unit with an online softmax; no atomics: the same inputs give the same bits
 * on every run. */
int dl_autoint_grid(int32_t B);
int dl_autoint_fwd(int32_t B, int32_t F, int32_t E, int32_t L, int32_t heads, int32_t D, const float* x0, int32_t ld,
                   int32_t x_col0, const float* params, const float* z_add, float* z_out, void* stream);
int dl_autoint_bwd(int32_t B, int32_t F, int32_t E, int32_t L, int32_t heads, int32_t D, const float* x0, int32_t ld,
                   int32_t x_col0, const float* params, const float* dz, float* dx0, int32_t dx_ld, int32_t dx_col0,
                   float* slab, int32_t slab_rows, void* stream);

/* Wide&Deep cross logit, forward and backward fused (models/wdl.py:225-275):
 * z = sum_f w[wide_f] + sum_j w[Fw+j] h_j + bias[0] (w = wdl_weights [w_rows]; the
 * deep-output rows Fw..Fw+H alias wide ids); sigmoid + eps-log-loss as dl_head_fwd_bwd.
 * Wide-row gradients dz are added to g_w (int64 fixed point, units 1/DL_WIDE_GRAD_SCALE:
 * integer atomics, so the segment sum is deterministic) (+ touched); the dense part leaves
 * slab[block][0..H) = sum dz*h, [H] = sum dz, [H+1] = sum loss (fold with
 * dl_slab_fold_rows into g_w rows Fw..Fw+H).  g_w = NULL: forward only (predict). */
int dl_wdl_head_fwd_bwd(int32_t B, int32_t Fw, int32_t H, const int64_t* wide, int32_t wide_ld,
                        const float* h, int32_t ldh, const float* w, const float* bias, int64_t w_rows,
                        const float* label, float eps, float inv_batch, float* score, float* z_out,
                        float* dz, float* dh, int64_t* g_w, uint8_t* touched, float* slab,
                        int32_t slab_blocks, int32_t* err, void* stream);
/* As dl_wdl_head_fwd_bwd with dh written as bf16 (round-to-nearest-even): the bf16
 * tower's dY operand (config C5), 8-B aligned, same leading dimension ldh as h. */
int dl_wdl_head_fwd_bwd_bf16(int32_t B, int32_t Fw, int32_t H, const int64_t* wide, int32_t wide_ld,
                             const float* h, int32_t ldh, const float* w, const float* bias, int64_t w_rows,
                             const float* label, float eps, float inv_batch, float* score, float* z_out,
                             float* dz, uint16_t* dh, int64_t* g_w, uint8_t* touched, float* slab,
                             int32_t slab_blocks, int32_t* err, void* stream);
/* ------------------------------------------------------------------------
 * Sample weights: tf.losses.log_loss(label, out, weights=w), TF 1.x's default reduction
 * SUM_BY_NONZERO_WEIGHTS (the reference leaves weights at 1):
 *   loss = sum_b w_b l_b / N_nz,  N_nz = #{b : w_b != 0}  (0 when N_nz == 0: div_no_nan),
 *   dz_b = (dl_b/dp) (w_b inv_norm) p (1 - p),  inv_norm = N_nz ? 1 / N_nz : 0,
 * with the effective weight w_b = weight_b * (1 + (pos_weight - 1) * y_b).
 *
 * dl_weight_norm: from weight [B] (NULL: all ones), label [B] and pos_weight (finite, > 0) writes
 * w_eff [B] (two separately rounded f32 operations: f = 1 + (pos_weight - 1) y, w = weight f) and
 * norm = {inv_norm, N_nz} (two floats; N_nz counted in integers in a fixed order, inv_norm =
 * (float)(1.0 / (double)N_nz): all-ones weights give the f32 the unweighted step's 1 / B is).
 * A weight that is negative, NaN or infinite sets DL_STATUS_BAD_WEIGHT in err[0] (the batch's
 * validation word, beside DL_STATUS_BAD_ID: the step applies nothing) and gets w_eff = 0.  Runs
 * after dl_validate_batch's reset of the word, before dl_step_begin.  One block; B <= 2^24.
 *
 * The *_weighted head entry points are their unweighted namesakes with (w_eff, norm) in place of
 * inv_batch: scale = w_eff[b] * norm[0] stands where inv_batch stands, and the slab's loss column
 * sums w_eff[b] * loss_b.  With all-ones weights they write the namesake's bits. */
int dl_weight_norm(const float* weight, const float* label, int32_t B, float pos_weight, float* w_eff,
                   float* norm, int32_t* err, void* stream);
int dl_head_fwd_bwd_weighted(int32_t B, int32_t fm_cols, int32_t H, const float* fm_out, int32_t fm_ld,
                             const float* h, int32_t ldh, const float* w, const float* label, float eps,
                             const float* w_eff, const float* norm, float* score, float* z_out, float* dz,
                             float* dh, float* slab, int32_t slab_blocks, void* stream);
int dl_head_fwd_bwd_fmdrop_weighted(int32_t B, int32_t fm_cols, int32_t H, const float* fm_out, int32_t fm_ld,
                                    const float* h, int32_t ldh, const float* w, const float* label, float eps,
                                    const float* w_eff, const float* norm, float* score, float* z_out, float* dz,
                                    float* dh, float* slab, int32_t slab_blocks, int32_t F, uint32_t keep_thr1,
                                    float inv1, uint32_t keep_thr2, float inv2, uint64_t seed, const float* opt,
                                    uint64_t* fm_keep, void* stream);
int dl_wdl_head_fwd_bwd_weighted(int32_t B, int32_t Fw, int32_t H, const int64_t* wide, int32_t wide_ld,
                                 const float* h, int32_t ldh, const float* w, const float* bias, int64_t w_rows,
                                 const float* label, float eps, const float* w_eff, const float* norm, float* score,
                                 float* z_out, float* dz, float* dh, int64_t* g_w, uint8_t* touched, float* slab,
                                 int32_t slab_blocks, int32_t* err, void* stream);
int dl_wdl_head_fwd_bwd_bf16_weighted(int32_t B, int32_t Fw, int32_t H, const int64_t* wide, int32_t wide_ld,
                                      const float* h, int32_t ldh, const float* w, const float* bias, int64_t w_rows,
                                      const float* label, float eps, const float* w_eff, const float* norm,
                                      float* score, float* z_out, float* dz, uint16_t* dh, int64_t* g_w,
                                      uint8_t* touched, float* slab, int32_t slab_blocks, int32_t* err, void* stream);
/* dl_loss_accumulate (below) with the data term's scale read from the device normaliser:
 * acc[0] += sum_r slab[r * pitch + col] / N_nz (N_nz = norm[1]; nothing added when it is 0). */
int dl_loss_accumulate_weighted(const float* slab, int32_t rows, int32_t pitch, int32_t col, const float* norm,
                                float* opt, float reg_coef, double* acc, int32_t* status_ring, void* stream);

/* g[row0+j] += sum over `blocks` slab rows of slab[blk*width + col0 + j], j < n, as int64
 * fixed point (units 1/DL_WIDE_GRAD_SCALE, the wide gradient's form). */
int dl_slab_fold_rows(const float* slab, int32_t blocks, int32_t width, int32_t col0, int32_t n,
                      int64_t* g, int64_t row0, uint8_t* touched, void* stream);

/* ------------------------------------------------------------------------
 * TF1 Adam (training_ops.cc ApplyAdam, dense semantics: every element's m, v
 * decay each step — SURVEY.md ledger item 6).  `opt` is a device float[16]:
 * [0] beta1_power [1] beta2_power [2] lr [3] alpha [4] beta1 [5] beta2
 * [6] epsilon [7] step (as float, exact < 2^24), [8..15] per-step accumulators
 * (zeroed by dl_adam_begin_step; [8..9] = opt + DL_OPT_REG is the step's regulariser sum as
 * int64 fixed point, the sq_out / acc_out target), [16] the status word (int32
 * bits, sticky until the host clears it: what the host reports), [17] the skip
 * word (int32 bits of the CURRENT step only, rewritten by dl_step_guard /
 * dl_step_begin), [18] the global step at which the last bad batch was skipped,
 * [19] how many batches were skipped since the host last cleared the status;
 * DL_OPT_LEN floats in all.
 * dl_adam_begin_step computes alpha = lr_t*sqrt(1-b2p)/(1-b1p) with
 * lr_t = lr*rate^floor(step/decay_steps) and then advances b1p*=b1, b2p*=b2,
 * step+=1 (TF's _finish + global_step).
 *
 * A nonzero SKIP word poisons the step: dl_adam_begin_step and every call that
 * writes parameters or Adam state (dl_adam_*, dl_rec_bwd_adam, dl_rec_apply_*)
 * return without writing them; gradient buffers they would consume are still
 * reset.  A batch whose ids fail validation therefore changes nothing, as TF's
 * failing sess.run applies nothing before raising InvalidArgumentError
 * (deepfm_pipeline.py:219-221), and the next batch applies normally (the skip word
 * belongs to one step); the host reads the sticky status word back and raises.
 * Internal faults (DL_STATUS_LAG / DL_STATUS_INDEX) set both words and keep every
 * later step skipped until the host clears the status. */
#define DL_OPT_LEN 32
#define DL_OPT_REG 8        /* int64 fixed point (units 1/DL_REG_SUM_SCALE) in opt[8..9]: the step's regulariser sum */
/* Regulariser sums (every sq_out / acc_out / sq_untouched below) are signed 64-bit fixed point
 * in units of 1/DL_REG_SUM_SCALE, 8-byte aligned: each block adds its fixed-order partial as an
 * integer, so the sum is the same bits whatever order the blocks land in (|sum| < 2^31). */
#define DL_REG_SUM_SCALE 4294967296.0 /* 2^32 */
#define DL_OPT_STATUS 16
#define DL_OPT_SKIP 17
#define DL_OPT_BAD_STEP 18
#define DL_OPT_BAD_COUNT 19
#define DL_OPT_SEQ 20       /* int32 bits: steps reported through dl_loss_accumulate's status ring */
#define DL_OPT_BAD_RANKS 21 /* int32 bits: sharded step — bit p set when rank p's batch held a bad id */
#define DL_STATUS_BAD_ID 1   /* a categorical / wide id outside [0, N) */
#define DL_STATUS_LAG 2      /* a row record lagged past the alpha ring (flush schedule broken) */
#define DL_STATUS_INDEX 4    /* a batch-index entry out of range (index consumers report, never skip silently) */
#define DL_STATUS_OVERFLOW 8 /* sharded step: a rank had more unique rows for an owner than a block holds */
#define DL_STATUS_DESYNC 16  /* sharded step: the ranks' headers named different global steps */
#define DL_STATUS_BAD_WEIGHT 32 /* a sample weight that is negative, NaN or infinite (dl_weight_norm) */
int dl_adam_begin_step(float* opt, float decay_rate, float decay_steps, void* stream);
/* The step's skip word := the batch's validation bits (batch_err[0], written by
 * dl_index_build / dl_validate_batch) | the sticky internal-fault bits; a bad batch
 * also sets opt[DL_OPT_STATUS], records the global step it was skipped at and counts
 * itself.  Issued before dl_adam_begin_step so the step of a bad batch is poisoned
 * from its start. */
int dl_step_guard(const int32_t* batch_err, float* opt, void* stream);
/* The batch's id-validation word, before its step begins: reset != 0 zeroes err[0] first
 * (one word per batch, not sticky); then every cate id (cate non-NULL, [L->batch][L->cate_ld]:
 * single columns against their deep row id + deep_cate_offset and, with FM, their FM row
 * id + fm_cate_offset; multi-hot columns against id + deep_cate_offset, all in [0, n_rows))
 * and every wide id (wide non-NULL, [batch][wide_ld], first wide_cols: [0, wide_rows)) sets
 * DL_STATUS_BAD_ID in err[0] if out of range.  For the batches no dl_index_build validates
 * (dense-layout gathers) and wdl's wide ids (models/wdl.py:225-228). */
int dl_validate_batch(const dl_emb_layout* L, const int64_t* cate, const int64_t* wide, int32_t wide_cols,
                      int32_t wide_ld, int64_t wide_rows, int32_t reset, int32_t* err, void* stream);
/* dl_step_guard, dl_adam_begin_step and (hist non-NULL) dl_adam_hist_record in one
 * launch, same operations in the same order: the step's opening graph node. */
int dl_step_begin(const int32_t* batch_err, float* opt, float decay_rate, float decay_steps, float* hist,
                  int32_t hist_len, void* stream);
/* The running loss of a training loop (the load-style fit's per-epoch mean, wdl.py:305-313):
 * acc[0] += sum_r slab[r * pitch + col] * inv_b (the step's data term; double, fixed order),
 * acc[1] += reg_coef * the step's regulariser sum (opt + DL_OPT_REG), acc[2] += 1; nothing for a skipped
 * step.  acc: double[3] on the device, read by the host once per epoch.  (Wide&Deep with lazy
 * wide records adds the wide L2 term per record step through dl_wide_rec_update / _flush acc.)
 * status_ring (may be NULL): int32[8] of pinned host memory; every call (skipped steps too)
 * advances the step sequence opt[DL_OPT_SEQ] to k and writes k to ring[2(k & 3)] and the status
 * word to ring[2(k & 3) + 1] in one 8-byte store: the host's per-step status report without a
 * device-to-host copy. */
int dl_loss_accumulate(const float* slab, int32_t rows, int32_t pitch, int32_t col, double inv_b, float* opt,
                       float reg_coef, double* acc, int32_t* status_ring, void* stream);
/* Dense parameter whose gradient is the sum of `nslab` partial slabs
 * (g = sum_s slab[s*slab_stride + i]); l2 * p is added for i < l2_count;
 * p_prev (may be NULL) receives the pre-update values; sq_out (may be NULL, int64 fixed
 * point, DL_REG_SUM_SCALE) gets sum p_pre^2 over the L2-regularised elements added — the
 * loss's l2_regularizer term of the step, read back without copying the parameters. */
/* dl_adam_dense_split3: dl_adam_dense_reg on a tower weight W [rows][cols] (n = rows * cols,
 * no p_prev) that also writes the updated W's three bf16 planes in dl_split3's two layouts —
 * wp[q][r][c] and wtp[q][c][r], plane stride rows * cols — in place of two dl_split3 launches
 * after the update (the s3 GEMMs' operands; deepfm_pipeline.py:184-188 ApplyAdam on W). */
int dl_adam_dense_split3(float* p, float* m, float* v, const float* slab, int32_t nslab, int64_t slab_stride,
                         int32_t rows, int32_t cols, float reg, int64_t reg_count, int32_t reg_kind, const float* opt,
                         int64_t* acc_out, uint16_t* wp, uint16_t* wtp, void* stream);
/* dl_adam_dense_bf16: the same for the bf16 tower (C5): the updated W's bf16 copy wb [rows][cols]
 * and its transpose wbt [cols][rows] (dl_cast_bf16 / dl_transpose_bf16's rounding). */
int dl_adam_dense_bf16(float* p, float* m, float* v, const float* slab, int32_t nslab, int64_t slab_stride,
                       int32_t rows, int32_t cols, float reg, int64_t reg_count, int32_t reg_kind, const float* opt,
                       int64_t* acc_out, uint16_t* wb, uint16_t* wbt, void* stream);
int dl_adam_dense(float* p, float* m, float* v, const float* slab, int32_t nslab,
                  int64_t slab_stride, int64_t n, float l2, int64_t l2_count, const float* opt,
                  float* p_prev, int64_t* sq_out, void* stream);
/* One tower weight's update for dl_adam_dense_layers: W [rows][cols] (p, m, v), its gradient as
 * `nslab` partial slabs `slab_stride` floats apart, the regulariser (reg_kind 0 = L2, 1 = L1) on
 * the first reg_count elements with its loss term added to *acc_out (may be NULL), and the
 * operand copies wp / wtp the update writes (dl_adam_dense_split3 / dl_adam_dense_bf16). */
typedef struct dl_adam_layer {
  float* p;
  float* m;
  float* v;
  const float* slab;
  int64_t slab_stride;
  int64_t reg_count;
  int64_t* acc_out;
  uint16_t* wp;
  uint16_t* wtp;
  int32_t nslab;
  int32_t rows, cols;
  int32_t reg_kind;
  float reg;
  int32_t pad_;
} dl_adam_layer;
/* dl_adam_dense_layers: dl_adam_dense_split3 (copies = 3) or dl_adam_dense_bf16 (copies = 1) on
 * up to DL_ADAM_MAX_LAYERS tower weights in one launch — the same per-element operations, so the
 * same results as one launch per layer (the regulariser sum: the same total, other block
 * partials).  One launch instead of one per hidden layer at the end of the backward. */
#define DL_ADAM_MAX_LAYERS 4
int dl_adam_dense_layers(int32_t n_layers, const dl_adam_layer* layers, int32_t copies, const float* opt,
                         void* stream);
/* dl_adam_dense with the regulariser kind explicit: reg_kind 0 = L2 as above, 1 = L1
 * (tf.contrib.layers.l1_regularizer at models/dnn.py:88-90: g += reg * sign(p) for
 * i < reg_count, acc_out += |p_pre|). */
int dl_adam_dense_reg(float* p, float* m, float* v, const float* slab, int32_t nslab,
                      int64_t slab_stride, int64_t n, float reg, int64_t reg_count, int32_t reg_kind,
                      const float* opt, float* p_prev, int64_t* acc_out, void* stream);
/* Embedding tables, every row updated: g = g_table row if touched else 0;
 * consumed gradients are reset to 0.  rows_flags: DL_ROWS_CLEAR_TOUCHED resets the
 * flags (on the last table that shares them); DL_ROWS_SPARSE_ADAM selects the update
 * TF applies to a Variable read by embedding_lookup directly (Adam._apply_sparse_shared:
 * m = m*b1 + g*(1-b1), v = v*b2 + (g*g)*(1-b2), p -= lr*m/(sqrt(v)+eps); wdl.py:44-47,132,
 * deepfm.py:57-60, dnn.py:49-54), else ApplyAdam's (the pipeline models' tables, whose
 * gradient is densified by the row-0 concat, deepfm_pipeline.py:83-86).
 * width = E (table) or 1 (first-order).  DL_ROWS_GRAD_FIXED (width 1): g is int64 fixed
 * point in units of 1/DL_WIDE_GRAD_SCALE (the wdl wide-weight gradient of
 * dl_wdl_head_fwd_bwd / dl_slab_fold_rows).
 * State form: `v` holds the ROOT state s = sqrt(v) for the embedding tables (every call
 * without DL_ROWS_GRAD_FIXED) — the form the row records keep, so the g = 0 step is
 * s' = s*sqrt(b2) (one reciprocal, no square root); a g != 0 step forms v = s*s, applies
 * the update above and stores sqrt(v').  With DL_ROWS_GRAD_FIXED (the wdl wide weights)
 * `v` is TF's v.  Callers convert at the boundary (engine.py adam_state / set_adam_state). */
#define DL_ROWS_CLEAR_TOUCHED 1
#define DL_ROWS_SPARSE_ADAM 2
#define DL_ROWS_GRAD_FIXED 4
#define DL_WIDE_GRAD_SCALE 281474976710656.0 /* 2^48 */
int dl_adam_rows(float* p, float* m, float* v, void* g, uint8_t* touched, int64_t n_rows,
                 int32_t width, float l2, int32_t rows_flags, const float* opt, int64_t* sq_out,
                 void* stream);

/* ------------------------------------------------------------------------
 * Lazy-exact Adam on interleaved row records (rec.hip).  Same result as the
 * dense sweep of dl_adam_rows (bit-identical: the skipped zero-gradient steps
 * are replayed with the same float operations when a row is next read), but a
 * step only touches the rows its batch references.  Record of rec_ld floats
 * (rec_ld >= 3E+4, multiple of 32): [p(E) | w1 m1 s1 stamp | m(E) | s(E) | pad],
 * s = sqrt(v) (the root state of dl_adam_rows); stamp = int32 bits of the last step applied.  hist = ring of hist_len (power
 * of two) per-step alphas; the caller keeps every row's lag < hist_len by
 * calling dl_rec_flush at least once per hist_len steps.
 * Replaces, for the table and first-order Variables, the dense ApplyAdam of
 * deepfm_pipeline.py:184-188 / dnn_pipeline.py:132-136 and the sparse-apply Adam
 * of wdl.py:277-285 / deepfm.py:157-162 / dnn.py:92-93.
 * rec_flags: DL_REC_FIRST = the record carries a first-order weight (FM models);
 * DL_REC_SPARSE_ADAM = the table is updated in TF's sparse-apply form (see
 * dl_adam_rows), else ApplyAdam's.  The catch-up replays the same form. */
#define DL_REC_FIRST 1
#define DL_REC_SPARSE_ADAM 2
/* dl_rec_flush only: p_plane is a slot plane [n_rows][2E] — row r's p in columns 0..E-1 and its
 * first-order weight in column E (128-B slots for E = 16; columns E+1.. unwritten), w1_plane unused */
#define DL_REC_PLANE_SLOTS 4
/* hist[step & (hist_len-1)] = alpha of the step dl_adam_begin_step just began. */
int dl_adam_hist_record(const float* opt, float* hist, int32_t hist_len, void* stream);
/* rows_u[i] = p(row_i) caught up to step opt[7]-lag (rows_u1[i] = w1), row_i =
 * L->fm_cont_offset + i for i < n_rep (the replicated FM cont-field rows) else the row of uniq_keys[i-n_rep] (batch index,
 * dl_index_build keys; n_uniq = NULL: max_uniq keys, e.g. an owner's received local
 * rows with world = 1).  Records are only read.  mv_u (may be NULL) receives the
 * moment stash for dl_rec_bwd_adam / dl_rec_apply_segments, dl_rec_stash_floats(E) floats a row:
 * m(E) | m1 s1 lag 0 (the backward takes s from the record it rewrites, decayed over `lag`
 * zero-gradient steps: the same bits), or, in builds with DL_STASH_M=0, m(E) | s(E) | m1 s1 0 0.
 * lag = 1 inside a training step, 0 for predict. */
int32_t dl_rec_stash_floats(int32_t emb_dim);
int dl_rec_gather(const dl_emb_layout* L, const float* rec, int32_t rec_ld, int32_t rec_flags,
                  int32_t n_rep, const uint32_t* uniq_keys, const int32_t* n_uniq, int64_t max_uniq,
                  int32_t world, const float* hist, int32_t hist_len, const float* opt, int32_t lag,
                  float* rows_u, float* rows_u1, float* mv_u, void* stream);
/* Fused backward + Adam: per unique row the ordered segment sum of its references
 * (as dl_embed_bwd_sorted) is applied with step opt[7]'s alpha to the caught-up
 * state of dl_rec_gather (rows_u, rows_u1, mv_u — full arrays, replicated rows
 * first; mv_u = NULL: the record is re-read and its catch-up replayed, using
 * hist), and the record is written with stamp = step.  The replicated rows
 * (L->fm_cont_offset + j, j < n_rep) instead add their gradient into g_rep[j][E] /
 * g1_rep[j] (finished by dl_rec_apply_rows with row0 = L->fm_cont_offset). */
/* Multi-hot pooling state for dl_rec_bwd_adam (deepfm_multi_cate.py:71-111): slot ranges
 * within the multi block, the head column of the pooled first-order outputs, dx0's pooled
 * columns, the pooled x0 (L->x0_pool_col), the nonzero counts of dl_pool_fwd_indexed and
 * the per-slot gradients' scratch, [B][n_slots] rows of g_pitch floats (>= E + 1, a multiple of
 * 4): row (b, m) of g_pool at g_pool + (b*n_slots + m)*g_pitch and its first-order gradient at
 * g1_pool[(b*n_slots + m)*g_pitch] — with g1_pool = g_pool + E and g_pitch = 32 (E = 16) both
 * sit in one 128-B line, so a multi-hot reference's gradient costs one line fetch, not two. */
typedef struct dl_pool_desc {
  const int32_t* slot_start;
  const int32_t* slot_end;
  int32_t n_slots;
  int32_t fm_col;
  int32_t dx0_pool_col;
  int32_t g_pitch;
  const float* x0;
  const float* cnt_emb;
  const float* cnt_first;
  float* g_pool;
  float* g1_pool;
} dl_pool_desc;
/* pool: required when L->multi_width > 0 (multi refs add (dp/cnt) to the row gradient
 * and dz*w_head[fm_col+m]/cnt_first to the first-order one), else may be NULL.
 * hot_ws (may be NULL; dl_rec_bwd_workspace_bytes(batch * index slots, E) bytes, 16-B aligned):
 * the rows with more than 32 references (Zipf-hot ids) are summed in chunks of 1,024
 * references spread over the whole grid, the chunk sums added in chunk order — the same
 * canonical sum as the single-block pass used without it (and by dl_embed_bwd_sorted). */
int dl_rec_bwd_adam(const dl_emb_layout* L, float* rec, int32_t rec_ld, int32_t rec_flags, int32_t n_rep,
                    const float* rows_u, const float* rows_u1, const float* mv_u,
                    const uint32_t* uniq_keys, const int32_t* seg_off, const int32_t* n_uniq,
                    const int32_t* sorted_refs, int32_t world, int64_t max_uniq, const float* dz,
                    const float* w_head, const float* fm_sum, const float* dx0, float* g_rep,
                    float* g1_rep, const float* hist, int32_t hist_len, const float* opt,
                    const dl_pool_desc* pool, void* hot_ws, int64_t hot_ws_bytes, void* stream);
/* With FM-part dropout ("Dropout" above): the segment sums and the pooled-slot gradients take dfm. */
int dl_rec_bwd_adam_fmdrop(const dl_emb_layout* L, float* rec, int32_t rec_ld, int32_t rec_flags, int32_t n_rep,
                           const float* rows_u, const float* rows_u1, const float* mv_u,
                           const uint32_t* uniq_keys, const int32_t* seg_off, const int32_t* n_uniq,
                           const int32_t* sorted_refs, int32_t world, int64_t max_uniq, const float* dz,
                           const float* w_head, const float* fm_sum, const float* dx0, float* g_rep,
                           float* g1_rep, const float* hist, int32_t hist_len, const float* opt,
                           const dl_pool_desc* pool, void* hot_ws, int64_t hot_ws_bytes, const dl_fm_drop* drop,
                           void* stream);
int64_t dl_rec_bwd_workspace_bytes(int64_t nrefs, int32_t emb_dim);
/* Sharded owners without a sort: link every received position into its row's arrival
 * chain (head[local_rows] starts at -1; next[n]).  Then apply: one leader per row sums its
 * arrivals g[pos][E], g1[pos] in ascending position order (as dl_rec_apply_segments over a
 * stable sort), catches the record up and steps it; head is reset to -1 afterwards. */
int dl_rec_chain_link(const int32_t* ids, int64_t n, int32_t* head, int32_t* next, void* stream);
int dl_rec_apply_chain(float* rec, int32_t rec_ld, int32_t emb_dim, int32_t rec_flags, const int32_t* ids,
                       int64_t n, int32_t* head, const int32_t* next, const float* g, const float* g1,
                       const float* hist, int32_t hist_len, const float* opt, void* stream);
/* Rows [row0, row0+n): step-t update with dense gradients g[n][E], g1[n] (zeroed after). */
int dl_rec_apply_rows(float* rec, int32_t rec_ld, int32_t emb_dim, int32_t rec_flags, int64_t row0,
                      int64_t n, float* g, float* g1, const float* hist, int32_t hist_len,
                      const float* opt, void* stream);
/* Sharded owners, deterministic: per unique received row (dl_sort_unique over the received
 * ids) the ordered sum of its arrivals g[pos][E], g1[pos] is applied (step opt[7]).  With
 * mv (the owner gather's moment stash, [n][dl_rec_stash_floats(E)]) the row's caught-up state is taken from
 * rows[pos][E] / rows1[pos] / mv[pos] at its first arrival — the owner gather's outputs —
 * and the record is only written; without it the record is read and caught up again. */
int dl_rec_apply_segments(float* rec, int32_t rec_ld, int32_t emb_dim, int32_t rec_flags, const int32_t* uniq,
                          const int32_t* seg_off, const int32_t* n_uniq, int64_t max_uniq, int64_t n,
                          const int32_t* sorted_pos, const float* g, const float* g1, const float* rows,
                          const float* rows1, const float* mv, const float* hist, int32_t hist_len,
                          const float* opt, void* stream);
/* Every row caught up to step opt[7] (before export/checkpoint, and every hist_len steps).
 * p_plane [n_rows][E] / w1_plane [n_rows] (may be NULL): every row's caught-up p and first-order
 * weight written out densely — the table predict's plain lookup then reads (dl_embed_fwd on the
 * planes: 64-B rows instead of the records' 128-B first lines); with DL_REC_PLANE_SLOTS in
 * rec_flags, one slot plane [n_rows][2E] holding both (dl_embed_fwd_slots). */
int dl_rec_flush(float* rec, int32_t rec_ld, int32_t emb_dim, int32_t rec_flags, int64_t n_rows,
                 const float* hist, int32_t hist_len, const float* opt, float* p_plane, float* w1_plane,
                 void* stream);

/* ------------------------------------------------------------------------
 * Row-sharded tables (shard.hip).  Owner side of the all-to-all lookup:
 * out[i] = table[ids[i]], out_first[i] = first[ids[i]] (first may be NULL);
 * and of the gradient return: G[ids[i]] += g[i] (f32 atomics: a row may come
 * from several peers), touched[ids[i]] = 1. */
int dl_shard_gather(const float* table, const float* first, const int32_t* ids, int64_t n,
                    int32_t emb_dim, float* out, float* out_first, void* stream);
int dl_shard_scatter_add(const float* g, const float* g_first, const int32_t* ids, int64_t n,
                         int32_t emb_dim, float* G, float* G_first, uint8_t* touched, void* stream);
/* Fixed-capacity exchange blocks of the sharded step (one hipGraph per step).
 * Arrays of 2W - 1 blocks of `cap` slots: block p < W = what peer p sends this rank (block
 * `rank`: this rank's own requests, in place), block W + p - (p > rank) = this rank's requests
 * to / answers from peer p.  dl_shard_route, from the batch index (unique keys grouped by owner,
 * owner_counts [W + 1] with the replicated group last): ids[block(p) cap + j] = the j-th unique
 * row owned by p (local row), -1 past its count; hdr[block(p) * 4] = {count, flags, rank, 0}
 * with flags = DL_STATUS_BAD_ID if err[0] and DL_STATUS_OVERFLOW if any owner's count exceeds
 * cap (or the replicated group rep_cap); rep_ids[j] = the replicated rows (-1 past the count);
 * upos[u] (may be NULL; u < n_max) = unique row u's slot block(p) cap + j, or
 * (2W - 1) cap + j for the replicated group, -1 past a capacity; inv (may be NULL, n_refs
 * entries) remapped in place from unique ids to slots.  The forward then reads rows_u[slot],
 * the backward writes its gradients at slots (dl_embed_bwd_sorted upos), and the exchanges
 * (dl_shard_exchange) move whole blocks.
 * dl_shard_stamp: before the request exchange, every outgoing header gets this rank's sticky
 * fault bits and its global step.
 * dl_shard_step_begin (after it): the step's guard from every rank's header — a bad id on any
 * rank skips the step everywhere (status DL_STATUS_BAD_ID, opt[DL_OPT_BAD_RANKS] |= the ranks),
 * an overflow / sticky fault on any rank or different steps (DL_STATUS_DESYNC) poison this and
 * every later step everywhere until the host clears the status — then dl_adam_begin_step and
 * (hist non-NULL) dl_adam_hist_record, as dl_step_begin.  hdr2 (may be NULL; blocks of cap2
 * slots): a second id set's headers (wdl's wide ids), counted and flagged alike. */
int dl_shard_route(const uint32_t* uniq_keys, const int32_t* n_uniq, const int32_t* owner_counts, int32_t world,
                   int32_t rank, int64_t cap, int32_t rep_cap, const int32_t* err, int32_t* ids, int32_t* hdr,
                   int32_t* rep_ids, int32_t* upos, int32_t* inv, int64_t n_refs, int64_t n_max, void* stream);
int dl_shard_stamp(int32_t* hdr, int32_t world, int32_t rank, const float* opt, void* stream);
int dl_shard_step_begin(const int32_t* hdr, const int32_t* hdr2, int32_t world, int64_t cap, int64_t cap2, float* opt,
                        float decay_rate, float decay_steps, float* hist, int32_t hist_len, void* stream);
/* out[i] = sum_s slab[s*stride + i] (dense gradients before the all-reduce). */
int dl_slab_sum(const float* slab, int32_t nslab, int64_t stride, int64_t n, float* out, void* stream);
/* out[i] = local row of uniq key i (i < min(n_uniq, cap)): the id send list. */
int dl_keys_to_local(const uint32_t* keys, const int32_t* n_uniq, int64_t cap, int32_t* out,
                     void* stream);

/* Row-sharded wdl_weights (wdl.py:241-285): row r on rank r % world, local r / world.
 * dl_shard_gather_scalar: out[i] = w[ids[i]] (owner side of the wide lookup);
 * dl_shard_add_fixed: G[ids[i]] += g[i] (int64 fixed point, integer atomics: order-free);
 * dl_wide_fold_owned: the deep-output rows row0 + j (j < H) this rank owns get
 *   G[(row0+j)/world] += fixed(gdeep[j]) (gdeep: the all-reduced sums of dz*h);
 * dl_wide_owned_values: out[j] = w[(row0+j)/world] if owned here, else 0 (sum over ranks =
 *   the replicated deep-output rows);
 * dl_wide_local_ids: out[k] = offset + inv[k] (-1 where inv < 0): wide ids into the
 *   rank's local wide table (exchanged rows). */
int dl_shard_gather_scalar(const float* w, const int32_t* ids, int64_t n, float* out, void* stream);
int dl_shard_add_fixed(const int64_t* g, const int32_t* ids, int64_t n, int64_t* G, uint8_t* touched,
                       void* stream);
int dl_wide_fold_owned(const float* gdeep, int32_t H, int64_t row0, int32_t world, int32_t rank, int64_t* G,
                       uint8_t* touched, void* stream);
int dl_wide_owned_values(const float* w, int32_t H, int64_t row0, int32_t world, int32_t rank, float* out,
                         void* stream);
int dl_wide_local_ids(const int32_t* inv, int64_t n, int64_t offset, int64_t* out, void* stream);
/* Lazy-exact TF1 Adam for Wide&Deep's wide weights (wide.hip; models/wdl.py:241-285, L2 on
 * every row: TF's dense gradient l2 * w reaches every row each step).  rec [w_rows][4] =
 * {w, m, v, stamp}; a row's skipped steps are replayed on read (g = l2 * w, adam_elem),
 * bit-identical to the dense dl_adam_rows sweep.
 * dl_wide_rec_gather: the deep-output rows Fw..Fw+H and the unique wide rows uniq_rows[u]
 * (dl_index_build keys, world 1) caught up to step opt[7] - lag into the head's local table
 * wloc = [— (Fw) | deep rows (H) | unique rows]; stash[u] (may be NULL) = {w, m, v, row bits};
 * rep_sq[u] (may be NULL) = the sum of w^2 over the steps replayed for unique row u (each
 * step's pre-update state: that step's L2 loss term for the row), counted by the update.
 * dl_wide_seg_grad: the batch's wide-weight gradient per unique wide row from the wide index
 *   (dl_index_build over the wide ids: sorted references `refs`, segment offsets `seg_off`, count
 *   n_uniq on the device): q[u] = sum over the row's references e of wide_fixed(dz[e / Fw]), int64
 *   fixed point (DL_WIDE_GRAD_SCALE) — the same bits as the head's per-reference atomics, without
 *   them (the head then runs with g_w = NULL).  long_ws: int32 [max_uniq + 1] scratch (hot rows).
 * dl_wide_rec_update: step opt[7] on the unique rows (gradient gloc[Fw + H + u] + the deep
 * term gloc[row] of a row in Fw..Fw+H, exact int64, + l2 w) from the stash, then on the deep
 * rows not covered; gloc reset; the pre-update w^2 of those rows as per-block partial sums
 * written to sq_out[0 .. dl_wide_update_blocks(max_uniq, H)) (may be NULL; the caller sums).
 * acc (may be NULL; double[65536], one slot per block index): the running loss's wide L2
 * term — every pre-update w^2 of the rows this step applies, and of the steps replayed for
 * them (rep_sq, or the deep rows' own replay) — added per block.
 * dl_wide_rec_flush: every row caught up to step opt[7]; the pre-update w^2 of the rows the
 * last step left untouched (the loss's L2 term for them) added to sq_untouched (int64 fixed
 * point, DL_REG_SUM_SCALE); every replayed
 * step's pre-update w^2 added to acc's slots (may be NULL).  Summed over acc after a flush, the
 * slots hold sum_t sum_r w_r(t-1)^2 over the steps since acc was zeroed on a flushed table. */
int dl_wide_rec_gather(const float* rec, int64_t w_rows, const uint32_t* uniq_rows, const int32_t* n_uniq,
                       int64_t max_uniq, int32_t Fw, int32_t H, const float* hist, int32_t hist_len,
                       const float* opt, float l2, int32_t lag, float* wloc, float* stash, float* rep_sq,
                       void* stream);
int64_t dl_wide_update_blocks(int64_t max_uniq, int32_t H);
int dl_wide_seg_grad(const float* dz, int32_t Fw, const int32_t* refs, const int32_t* seg_off, const int32_t* n_uniq,
                     int64_t max_uniq, int64_t nrefs, int64_t* q, int32_t* long_ws, const float* opt, void* stream);
int dl_wide_rec_update(float* rec, const int32_t* n_uniq, int64_t max_uniq, const float* stash, int64_t* gloc,
                       int32_t Fw, int32_t H, float l2, const float* hist, int32_t hist_len,
                       const float* opt, uint8_t* dmark, float* sq_out, const float* rep_sq, double* acc,
                       void* stream);
int dl_wide_rec_flush(float* rec, int64_t w_rows, float l2, const float* hist, int32_t hist_len,
                      const float* opt, int64_t* sq_untouched, double* acc, void* stream);
#define DL_LOSS_ACC_SLOTS 65536   /* slots of the wide running-loss accumulator (>= any grid above) */
/* FTRL-proximal for the same wide weights (wide.hip; TF1 FtrlOptimizer(lr, learning_rate_power =
 * -0.5, initial_accumulator_value = 0.1, l1, l2), ApplyFtrl / SparseApplyFtrl without shrinkage).
 * Per touched row, g the exact fixed-point sum of the row's references:
 *   n' = n + g^2;  z += g - (sqrt(n') - sqrt(n)) / lr * w;
 *   w = |z| > l1 ? (sign(z) l1 - z) / (sqrt(n') / lr + 2 l2) : 0
 * lr (finite, > 0), l1, l2 (finite, >= 0) are kernel scalars; lr is not decayed.  An untouched
 * row keeps its bits: rec [w_rows][4] = {w, z, n, 0} carries no stamp, and there is no replay,
 * no lag and no flush.  No atomics on the data path: the same inputs give the same bits.
 * dl_wide_ftrl_gather: the deep-output rows Fw..Fw+H and the unique wide rows uniq_rows[u]
 *   (u < min(n_uniq[0], max_uniq); n_uniq NULL: max_uniq) as they stand into wloc = [— (Fw) | deep
 *   rows (H) | unique rows]; stash[u] = {w, z, n, row bits} when training (NULL: the predict
 *   form).  A row outside [0, w_rows) raises DL_STATUS_INDEX (and poisons the step).
 * dl_wide_ftrl_update: pass A, the step on the stashed unique rows from gloc[Fw + H + u] (+ the
 *   deep term gloc[row] of a row in Fw..Fw+H, exact int64; dmark[row - Fw] set); pass B, the deep
 *   rows dmark did not cover.  gloc and dmark are reset; a poisoned step writes no record.
 * dl_ftrl_rows: the same step on the rows with touched[r] != 0 of the plane arrays w, z, n
 *   ([rows] each; g_fixed the head's DL_WIDE_GRAD_SCALE gradient); g_fixed and touched of
 *   those rows are reset, also by a poisoned step.  touched 4-B aligned. */
int dl_wide_ftrl_gather(const float* rec, int64_t w_rows, const uint32_t* uniq_rows, const int32_t* n_uniq,
                        int64_t max_uniq, int32_t Fw, int32_t H, const float* opt, float* wloc, float* stash,
                        void* stream);
int dl_wide_ftrl_update(float* rec, const int32_t* n_uniq, int64_t max_uniq, const float* stash, int64_t* gloc,
                        int32_t Fw, int32_t H, float lr, float l1, float l2, const float* opt, uint8_t* dmark,
                        void* stream);
int dl_ftrl_rows(float* w, float* z, float* n, int64_t* g_fixed, uint8_t* touched, int64_t rows, float lr, float l1,
                 float l2, const float* opt, void* stream);

/* ------------------------------------------------------------------------
 * RCCL collectives of the row-sharded step (comm.cpp; SURVEY.md §8(b)3
 * comm_init / all_to_allv / all_reduce), for a host that binds this library
 * directly.  One communicator per rank (one GPU each); calls are stream-ordered.
 * RCCL errors return 2000 + ncclResult_t.  The Python engine (shard.py) reaches the
 * same RCCL through torch.distributed (backend "nccl").
 *   dl_comm_get_unique_id: rank 0 creates the id (dl_comm_unique_id_bytes() bytes)
 *     and ships it to the other ranks out of band (the reference-side launcher's job);
 *   dl_all_to_allv: rows of row_bytes each, grouped by peer in rank order; counts are
 *     host arrays of nranks row counts (the step's owner-count all-gather gives them);
 *   dl_all_reduce_f32: sum, in place when send == recv;
 *   dl_all_gather: `bytes` per rank into recv[nranks][bytes]. */
int dl_comm_unique_id_bytes(void);
int dl_comm_get_unique_id(void* id_out);
int dl_comm_init(const void* unique_id, int32_t nranks, int32_t rank, void** comm_out);
int dl_comm_destroy(void* comm);
int dl_all_to_allv(void* comm, const void* send, const int64_t* send_counts, void* recv,
                   const int64_t* recv_counts, int64_t row_bytes, void* stream);
int dl_all_reduce_f32(void* comm, const float* send, float* recv, int64_t n, void* stream);
int dl_all_gather(void* comm, const void* send, void* recv, int64_t bytes, void* stream);
/* The sharded step's exchanges (dl_shard_route's block layout; replaces the id / row / gradient
 * all-to-alls of SURVEY §8(e) with fixed sizes, so the whole step is one hipGraph): for each of
 * n_arrays device arrays of 2W - 1 blocks of block_bytes[a] bytes (host arrays), every block
 * this rank sends to / receives from every other peer, in one RCCL group.  dir 0 (to the
 * owners): send block W + p - (p > rank), receive peer p's into block p; dir 1 (back to the
 * senders): send block p, receive into block W + p - (p > rank).  world 1: no-op. */
int dl_shard_exchange(void* comm, int32_t n_arrays, void* const* bases, const int64_t* block_bytes, int32_t dir,
                      void* stream);

/* ------------------------------------------------------------------------
 * Utilities. */
/* Counter-based (Philox-4x32-10) init: dist 0 normal(mean, scale), 1 uniform[mean, mean+scale). */
int dl_init_random(float* p, int64_t n, int32_t dist, float mean, float scale, uint64_t seed,
                   uint64_t offset, void* stream);

/* ------------------------------------------------------------------------
 * Evaluation metric (metrics.hip): exact tie-aware ROC-AUC, the semantics of
 * sklearn.metrics.roc_auc_score that the reference calls on the collected scores
 * (models/deepfm_pipeline.py:311,344; wdl.py:343-358; deepfm.py:229).
 * scores[i * s_stride], labels[i * l_stride] (label > 0.5 = positive), n <= 2^31-1.
 * Writes the AUC to out[0] (device double; NaN when only one class is present, where
 * sklearn raises).  The numerator is an exact integer count (ties: 1/2), so the result
 * is deterministic.  Workspace: dl_auc_workspace_bytes(n). */
int64_t dl_auc_workspace_bytes(int64_t n);
int dl_auc(const float* scores, int64_t s_stride, const float* labels, int64_t l_stride, int64_t n,
           void* ws, int64_t ws_bytes, double* out, void* stream);
/* Per-group AUC (GAUC, metrics.hip): the weighted mean over groups of each group's own tie-aware
 * AUC (dl_auc's semantics on the group's samples alone: roc_auc_score per group).  A group is the
 * set of samples with equal groups[i * g_stride] (int64, the dtype of cate_feats; ids in
 * [0, 2^31)); it is valid iff it holds a positive and a negative (label > 0.5 = positive).  Ties
 * are by the order-preserving float key (-0.0 ties with +0.0) and only within a group.
 *   weighting 0: w_g = n_g, the group's sample count (impression-weighted GAUC);
 *   weighting 1: w_g = 1 (mean of per-group AUC); anything else is refused on the host.
 *   out[0] = sum_valid w_g AUC_g / sum_valid w_g (NaN when no group is valid)
 *   out[1] = samples in valid groups, out[2] = valid groups, out[3] = all groups (exact integers).
 * Every group's 2 x numerator = sum over its tie runs of pos (2 below + neg), below = the group's
 * own negatives scored lower, and its counts are exact integers; floating point enters at
 * w_g num2_g / (2 P_g N_g) per group, summed in double in a fixed order over the sorted group
 * positions (per-tile partials, then one block): two calls on the same input give the same bits.
 * An id outside [0, 2^31) is never read as another id: it raises the error word — the first
 * int32 of ws, DL_STATUS_BAD_ID, rewritten by every call — and all of out[0..3] is NaN; the host
 * turns the word into an exception (deep_learning_amd.metrics.group_auc: ValueError).
 * Workspace: dl_gauc_workspace_bytes(n) (-1 for n <= 0 or n > 2^31-1), 256-B aligned. */
int64_t dl_gauc_workspace_bytes(int64_t n);
int dl_gauc(const float* scores, int64_t s_stride, const float* labels, int64_t l_stride, const int64_t* groups,
            int64_t g_stride, int64_t n, int32_t weighting, void* ws, int64_t ws_bytes, double* out, void* stream);
/* Log-loss and calibration sums of the same scores: p = the f32 score widened to double, y = the
 * label bit (label > 0.5):
 *   out[0] = sum -y log(p + eps) - (1 - y) log(1 - p + eps)   (the loss of dl_head_fwd_bwd, in double)
 *   out[1] = sum p, out[2] = sum y, out[3] = n.
 * Double sums in a fixed order, no atomics: per-block partials into ws, then one block sums them.
 * Workspace: dl_eval_stats_workspace_bytes(n) (-1 for n <= 0 or n > 2^31-1), 8-B aligned. */
int64_t dl_eval_stats_workspace_bytes(int64_t n);
int dl_eval_stats(const float* scores, int64_t s_stride, const float* labels, int64_t l_stride, int64_t n, double eps,
                  void* ws, int64_t ws_bytes, double* out, void* stream);
/* dl_eval_stats with per-sample weights w (f32 widened to double, finite and >= 0):
 *   out[0] = sum w l, out[1] = sum w p, out[2] = sum w y, out[3] = sum w, out[4] = #{w != 0}
 * (l, p, y as in dl_eval_stats).  A weight that is negative, NaN or infinite makes all of
 * out[0..3] NaN.  Same two fixed-order double stages.
 * Workspace: dl_eval_stats_weighted_workspace_bytes(n) (-1 for n <= 0 or n > 2^31-1), 8-B aligned. */
int64_t dl_eval_stats_weighted_workspace_bytes(int64_t n);
int dl_eval_stats_weighted(const float* scores, int64_t s_stride, const float* labels, int64_t l_stride,
                           const float* weights, int64_t w_stride, int64_t n, double eps, void* ws, int64_t ws_bytes,
                           double* out, void* stream);
/* Streaming copy of `bytes` (a multiple of 16, both pointers 16-B aligned) from src to dst: the
 * measured HBM yardstick bench.py reports beside the 8 TB/s specification (roofline.peak_measured). */
int dl_hbm_copy(const void* src, void* dst, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DLAMD_H */
