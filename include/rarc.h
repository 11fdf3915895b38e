/*
 * rarc.h — C-ABI of librarc_hip.so, the MI355X (gfx950) backend for RAG-ARC's
 * dense-retrieval hot path.
 *
 * The reference (DataArcTech/RAG-ARC) has no FFI of its own: the hot path is
 * Python that calls faiss / numpy.  Each entry point below replaces the
 * arithmetic behind one reference call site (cited as file:line relative to the
 * reference tree).  INTEGRATION.md shows the ctypes stubs a maintainer adds on
 * the reference side.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (HBM); h_* is a host pointer.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - every function returns 0 on success, a negative RARC_E_* code otherwise;
 *     nothing throws across the boundary; rarc_last_error() returns a
 *     thread-local human-readable message for the last failure.
 *   - the library allocates nothing: the caller owns all buffers, including the
 *     scratch workspace whose size rarc_search_workspace_bytes() reports.
 *   - functions are re-entrant per (device, stream); the caller selects the
 *     device (hipSetDevice) before calling.
 *   - doc ids are row indices (int64); scores are fp32.
 *   - ordering everywhere: score descending, ties by id ascending.
 */
#ifndef RARC_H
#define RARC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RARC_VERSION 600 /* 0.6.0: the encoder's QUERY PATH (RarcEnc32Layer.*_wq, rarc_enc32_pack_query_weight: forwards of 32 / 64 / 128 tokens as weight streams), rarc_stream_read (the measured HBM read ceiling a bench line reports next to the nominal one); 0.5.1: rarc_similar_pairs (all-pairs cosine >= threshold: the graph store's entity dedup); 0.5.0: rarc_search_wide (rows to 4096 padded dims, k to 8192), rarc_compact_rows (delete by compaction), rarc_vmem_* (growable arenas), RARC_E_IO / RARC_IO_TRUNCATE; 0.4.1: RarcEnc32Layer.f1_colmax (FFN1 with its GELU fused into the GEMM epilogue); 0.4.0: shard-file streaming (rarc_file_to_device, rarc_device_to_file), host WordPiece (rarc_wordpiece_*); 0.3.2: RMSNorm folded into the reranker LM's projections (RarcLmLayer.qkv_w_folded, gate_up_w_folded),
                            * rarc_enc_gemm_zero_bias; 0.3.1: relative-position attention bias in both encoder forwards (MPNet family: RarcEncModel / RarcEnc32Model
                            * rel_bias, rel_span); 0.3.0: fp32-class encoder forward (rarc_enc32_*) */

#define RARC_OK 0
#define RARC_E_INVALID -1     /* bad argument (null pointer, unsupported d/k, ...) */
#define RARC_E_HIP -2         /* a HIP runtime call or kernel launch failed */
#define RARC_E_WORKSPACE -3   /* workspace too small / misaligned */
#define RARC_E_UNSUPPORTED -4 /* shape outside what the kernels were built for */
#define RARC_E_IO -5          /* a file operation failed (open, read, write, fsync: ENOSPC, EIO, a short file ...) */

/* Limits of the fused scan kernels (int8 prefilter: d_pad <= 1024; fp16 scan: d_pad <= 768). */
#define RARC_MAX_QUERIES 256 /* queries per scan pass (register-resident) */
#define RARC_MAX_K 1024      /* largest k' the finalize kernel selects */
#define RARC_DIM_ALIGN 128   /* stored row length is a multiple of this */

/* status bits written per query by rarc_search_f16 (d_status[q]) */
#define RARC_Q_OK 0u
#define RARC_Q_UNCERTAIN 1u /* exactness certificate failed (fp16 scan only): call rarc_repair_f16 */
#define RARC_Q_OVERFLOW 2u  /* candidate buffer overflowed: call rarc_repair_f16 */
/* diagnostics in the second byte of a flagged query's word (which limit it ran into; hosts treat any non-zero word alike) */
#define RARC_Q_WHY_SEGMENT 0x100u    /* a scan workgroup's candidate segment for this query filled up */
#define RARC_Q_WHY_G1 0x200u         /* more rows at or above the k-th approximate score than the rescore buffer holds, no cut found */
#define RARC_Q_WHY_G2 0x400u         /* rows within the error bound of the k-th exact score exceed the buffer (unbanded path) */
#define RARC_Q_WHY_BAND_TIES 0x800u  /* banded rescore: a band of equal approximate scores does not fit */
#define RARC_Q_WHY_BAND_GUARD 0x1000u /* banded rescore: iteration guard exhausted */

int rarc_version(void);
const char* rarc_last_error(void);

/* Smallest multiple of RARC_DIM_ALIGN that is >= d. */
int rarc_padded_dim(int d);

/*
 * L2-normalise rows in fp32, in place or out of place (d_out may equal d_in).
 * Replaces faiss.normalize_L2 at
 *   encapsulation/database/vector_db/VectorStore_Faiss.py:150-154 (called from :178, :259).
 * Semantics (restated from faiss fvec_renorm_L2): nr = sum x^2 in fp32;
 * if nr > 0: x *= (float)(1.0 / sqrt(nr)); zero rows are left unchanged.
 * The summation order is the canonical 8-lane order documented in DESIGN.md.
 * ld_in / ld_out are row strides in elements.
 */
int rarc_l2norm_rows_f32(const float* d_in, int64_t ld_in, float* d_out, int64_t ld_out,
                         int64_t n_rows, int d, void* stream);

/*
 * Cosine similarities in float64, as the chunker computes them (numpy branch of
 *   core/file_management/chunker/spliter.py:307-332  cosine_similarity(X, Y)
 * = np.dot(X, Y.T) / np.outer(|X|, |Y|), entries that come out NaN/inf (a zero row) set to 0), and the distances of
 * consecutive rows  1 - cosine(x_i, x_{i+1})  of
 *   core/file_management/chunker/spliter.py:354-371  calculate_cosine_distances.
 * Inputs are fp32 rows on the device (what an Embeddings provider returns), sums run in fp64: products of fp32
 * values are exact there, so only the order of the additions differs from numpy (|delta| ~ 1e-16 relative).
 * d_out: [nx][ny] doubles / [n_rows - 1] doubles.
 */
int rarc_cosine_matrix_f32(const float* d_x, int64_t ld_x, int nx, const float* d_y, int64_t ld_y, int ny, int d,
                           double* d_out, void* stream);
int rarc_adjacent_cosine_distance_f32(const float* d_x, int64_t ld_x, int n_rows, int d, double* d_out, void* stream);

/*
 * Ingest: fp32 rows -> (optionally L2-normalised) -> fp16 corpus rows of length
 * d_pad (zero padded).  Replaces `_normalize_vectors` + `index.add` at
 *   VectorStore_Faiss.py:178, :199-202
 * for an HBM-resident fp16 flat index.  d_row_norm2 (optional, n_rows floats)
 * receives the squared L2 norm of each stored (fp16-rounded) row.
 */
int rarc_ingest_f16(const float* d_in, int64_t ld_in, uint16_t* d_corpus_f16, int d_pad,
                    float* d_row_norm2, int64_t n_rows, int d, int normalize, void* stream);

/*
 * Quantisation metadata of an fp16 corpus shard, needed by the int8-prefilter scan of
 * rarc_search_f16 (no reference counterpart: it is part of `index.add`,
 * VectorStore_Faiss.py:199-202, for this backend).  d_qmeta is a caller-owned float array of
 * rarc_quant_meta_floats(n_rows) elements, ZEROED by the caller before the first call:
 *   [0]            R = max over stored rows of ||d - d8/s||_2 (the int8 image's residual norm);
 *                  only ever raised, so it stays valid when rows are appended
 *   [1]            rho: a bound of ||d - d_scanned|| over all rows when the scan reads a ROUNDED image of the
 *                  stored rows (fp32 storage, rarc_search_f32: the caller sets it); 0 otherwise
 *   [2..3]         reserved
 *   [4+2t], [5+2t] scale s_t of the 32-row tile t (127 / max|x| rounded down to fp16) and 1/s_t
 * The call (re)computes the entries of every tile that intersects rows [first_row, n_rows): after
 * appending rows, pass the old row count as first_row.  The corpus buffer must hold ceil32(n_rows)
 * rows (the rows beyond n_rows may hold anything finite).
 */
size_t rarc_quant_meta_floats(int64_t n_rows);
int rarc_quant_meta_f16(const uint16_t* d_corpus_f16, int64_t n_rows, int d_pad, int64_t first_row,
                        float* d_qmeta, void* stream);

/*
 * Test hook: the dense matrix of int8-prefilter scores of a small shard (n_rows <= 2^22),
 * d_out [nq][n_rows] fp32, computed with the scan's own quantisation routine.  Lets a test check
 * |canonical - approx| <= eps8[q] for every (query, row) pair; not used by any search.
 */
int rarc_debug_q8_scores(const uint16_t* d_corpus_f16, int64_t n_rows, int d_pad, const float* d_qmeta,
                         const void* d_qblock, int nq, float* d_out, void* stream);
/* The same for fp8 rows (d_qmeta from rarc_quant_meta_f8, d_pad a multiple of 256): the scan's fp8 quantisation with the
 * per-row multipliers of the tile metadata.  Same limits; not used by any search. */
int rarc_debug_q8_scores_f8(const uint8_t* d_corpus_f8, int64_t n_rows, int d_pad, const float* d_qmeta,
                            const void* d_qblock, int nq, float* d_out, void* stream);

/*
 * Query preparation: fp32 queries [nq][ld_in] -> the "query block" the search reads:
 * (optionally L2-normalised) fp32 copy [RARC_MAX_QUERIES][d_pad] (zero padded), fp16 copy (seed
 * pass / fp16 scan), int8 copy + scale (int8 prefilter), and the per-query error bounds of both
 * approximate scorers.  Replaces `np.array([embedding]).astype(np.float32)` +
 * `_normalize_vectors` at VectorStore_Faiss.py:258-259.
 *   d_qmeta  : the corpus' quantisation metadata (its R enters the int8 error bound); NULL when
 *              the search will be run without it
 *   d_qblock : rarc_query_block_bytes(d_pad) bytes, 256-byte aligned, caller-owned
 */
size_t rarc_query_block_bytes(int d_pad);
int rarc_prep_queries(const float* d_in, int64_t ld_in, int nq, int d, int d_pad, int normalize,
                      float corpus_max_norm, const float* d_qmeta, void* d_qblock, void* stream);

/*
 * Re-running a search whose first attempt was flagged (RARC_Q_OVERFLOW / RARC_Q_UNCERTAIN): the k-th entry of the
 * incomplete answer is the canonical score of a real row, hence a lower bound of the true k-th best score.  After
 * rarc_prep_queries of the flagged queries, rarc_qblock_set_floor stores that bound per query (d_prev_ids /
 * d_prev_scores: [nq][k], the rows of the first answer that belong to these queries; entries with id < 0 give no
 * bound) and the next rarc_search_* starts from it instead of from a sample statistic: the candidate lists hold
 * only rows within one error bound of the final threshold.  rarc_prep_queries resets the bounds to -inf.
 */
int rarc_qblock_set_floor(void* d_qblock, int d_pad, const int64_t* d_prev_ids, const float* d_prev_scores, int k,
                          int nq, void* stream);

/* Bytes of device scratch rarc_search_f16 / rarc_repair_f16 need (256-byte aligned base).
 * After a search, the uint32 at byte offset RARC_WS_ANYFLAG_OFFSET of the workspace is the OR of
 * all d_status words of that search (0 == nothing to repair). */
#define RARC_WS_ANYFLAG_OFFSET 5124
size_t rarc_search_workspace_bytes(int cand_cap);

/*
 * Flat inner-product search over an fp16 corpus shard resident in HBM.
 * Replaces faiss.IndexFlatIP.search at VectorStore_Faiss.py:262-263 for
 * nq <= RARC_MAX_QUERIES queries at once (the reference calls it with nq = 1).
 *
 *   d_corpus_f16 : [ceil32(n_rows)][d_pad] fp16, row-major
 *   d_qmeta      : quantisation metadata (rarc_quant_meta_f16).  Non-NULL selects the int8
 *                  prefilter scan: rows are discarded on int8 MFMA scores under a rigorous error
 *                  bound, every possible top-k row is rescored canonically (exact by construction).
 *                  NULL selects the fp16 MFMA scan with k' selection + exactness certificate
 *                  (d_pad <= 768 only; kept for comparison).
 *   d_qblock     : output of rarc_prep_queries for these queries (same d_pad, same d_qmeta)
 *   k            : results per query (k <= kprime)
 *   kprime       : rows the pruning thresholds are built on (k <= kprime <= RARC_MAX_K); the fp16
 *                  path also rescored exactly this many
 *   id_base      : added to local row indices (global id of this shard's row 0)
 *   d_out_ids    : [nq][k] int64, -1 where fewer than k rows exist
 *   d_out_scores : [nq][k] fp32 canonical scores, -inf padding
 *   d_status     : [RARC_MAX_QUERIES + 1] uint32, ZEROED BY THE CALLER: entry q < nq receives
 *                  the RARC_Q_* bits of query q (a query whose bit is set must be repaired
 *                  with rarc_repair_f16 before its row is trusted); the last entry
 *                  receives the OR of all of them (one word to read back per batch)
 *   bin_lo/bin_hi: score range covered by the pruning histogram
 *                  (cosine: -1, +1; ip: -/+ max|q|*max|d|)
 */
int rarc_search_f16(const uint16_t* d_corpus_f16, int64_t n_rows, int d_pad, const float* d_qmeta,
                    const void* d_qblock, int nq, int k, int kprime, int64_t id_base, float bin_lo,
                    float bin_hi, int64_t* d_out_ids, float* d_out_scores, uint32_t* d_status,
                    void* d_workspace, size_t workspace_bytes, int cand_cap, void* stream);

/*
 * Exact repair / verification of ONE query row: scans the whole shard with the
 * canonical fp32 scorer, collects every row that beats the current k-th result
 * and re-sorts.  After it returns the row is exact regardless of d_status.
 * d_found (1 uint32) receives the number of rows that beat the previous k-th
 * entry (0 == the previous answer was already exact).
 */
int rarc_repair_f16(const uint16_t* d_corpus_f16, int64_t n_rows, int d_pad, const void* d_qblock,
                    int q, int k, int64_t id_base, int64_t* d_out_ids, float* d_out_scores,
                    uint32_t* d_found, void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * Batched exact verification: for queries q_first .. q_first + nq - 1 (nq <= 8) of the prepared query block, count the
 * rows of the shard whose canonical key (score desc, id asc) beats the k-th entry of the query's answer in
 * d_ids / d_scores ([256][k] rows of the batch).  d_counts[i] includes the k - 1 better entries of the answer itself
 * when they are real rows, so an exact answer gives d_counts[i] == (number of valid entries among its first k - 1).
 * A row is read once for all nq queries: the whole batch of 256 is checked against an exact scan in 32 passes.
 * d_counts has TWENTY-FOUR words (ABI 400; it was sixteen): d_counts[16 + i] = rows at or above the k-th entry that were
 * not looked up because one thread had met 64 of them for that query already (> 0 means the pair count is a lower bound:
 * "check truncated", not "answer wrong").  d_counts[8 + i] = the rows at or above the k-th entry whose (id, canonical score) pair is an
 * entry of the answer BIT FOR BIT — an exact answer gives d_counts[8 + i] == (number of valid entries among all k): an entry
 * with a wrong score, a wrong id or a row that does not reach the k-th key is not counted.  (An all-padding answer, k-th id
 * -1, is not pair-checked: d_counts[8 + i] stays 0.)
 * row_format: 0 fp16 rows, 1 fp8 rows + d_row_scale, 2 fp32 rows.
 */
int rarc_verify_batch(const void* d_rows, const float* d_row_scale, int row_format, int64_t n_rows, int d_pad,
                      const void* d_qblock, int q_first, int nq, int k, int64_t id_base, const int64_t* d_ids,
                      const float* d_scores, uint32_t* d_counts, void* stream);

/*
 * Optional int8 "shadow" image of an fp16 corpus.  The int8-prefilter scan converts every fp16 row to
 * int8 on each search; with d_pad a multiple of 256 the conversion can be done once, at ingest
 * (rarc_quant_shadow_f16 = rarc_quant_meta_f16 + the image, int8 [ceil32(n_rows)][d_pad], caller-owned),
 * and rarc_search_f16_shadow then scans the image instead: half the HBM traffic per search and no
 * conversion arithmetic, for 50 % more HBM footprint.  Candidates are identical by construction (same
 * bytes, same bound), the canonical rescore still reads the fp16 rows: results are bit-identical to
 * rarc_search_f16.
 */
int rarc_quant_shadow_f16(const uint16_t* d_corpus_f16, int64_t n_rows, int d_pad, int64_t first_row,
                          float* d_qmeta, int8_t* d_shadow8, void* stream);
int rarc_search_f16_shadow(const uint16_t* d_corpus_f16, const int8_t* d_shadow8, int64_t n_rows, int d_pad,
                           const float* d_qmeta, const void* d_qblock, int nq, int k, int kprime,
                           int64_t id_base, float bin_lo, float bin_hi, int64_t* d_out_ids,
                           float* d_out_scores, uint32_t* d_status, void* d_workspace, size_t workspace_bytes,
                           int cand_cap, void* stream);

/*
 * fp8 corpus (BASELINE.json config 5's storage): rows of OCP e4m3fn bytes, d_pad a multiple of 256
 * (rarc_padded_dim_f8), plus one fp32 scale per row: value[m] = d_row_scale[r] * decode(byte[m]).
 * Half the HBM footprint and scan traffic of fp16.  The calls mirror their fp16 counterparts:
 *   rarc_ingest_f8      normalise (as rarc_ingest_f16), scale = max|x| / 448, byte = encode(x / scale)
 *                       (round to nearest even, saturating); d_row_norm2 optional
 *   rarc_quant_meta_f8  metadata for the int8-prefilter scan: rarc_quant_meta_floats_f8(n_rows) floats,
 *                       [0] = R as for fp16, then per 32-row tile: scale, 1/scale, 32 row multipliers
 *   rarc_search_f8      int8-prefilter scan + canonical finalize; the canonical score of a row is
 *                       d_row_scale[r] * (canonical fp32 dot of the query with the decoded bytes)
 *   rarc_repair_f8      exact single-query repair / verification
 * The query block is the one rarc_prep_queries writes (same d_pad; pass the fp8 d_qmeta).
 */
int rarc_padded_dim_f8(int d);
int rarc_ingest_f8(const float* d_in, int64_t ld_in, uint8_t* d_corpus_f8, int d_pad, float* d_row_scale,
                   float* d_row_norm2, int64_t n_rows, int d, int normalize, void* stream);
size_t rarc_quant_meta_floats_f8(int64_t n_rows);
int rarc_quant_meta_f8(const uint8_t* d_corpus_f8, const float* d_row_scale, int64_t n_rows, int d_pad,
                       int64_t first_row, float* d_qmeta, void* stream);
int rarc_search_f8(const uint8_t* d_corpus_f8, const float* d_row_scale, int64_t n_rows, int d_pad,
                   const float* d_qmeta, const void* d_qblock, int nq, int k, int kprime, int64_t id_base,
                   float bin_lo, float bin_hi, int64_t* d_out_ids, float* d_out_scores, uint32_t* d_status,
                   void* d_workspace, size_t workspace_bytes, int cand_cap, void* stream);
int rarc_repair_f8(const uint8_t* d_corpus_f8, const float* d_row_scale, int64_t n_rows, int d_pad,
                   const void* d_qblock, int q, int k, int64_t id_base, int64_t* d_out_ids, float* d_out_scores,
                   uint32_t* d_found, void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * fp32 corpus — the reference's own storage (np.float32 rows in IndexFlatIP, VectorStore_Faiss.py:170,199-202):
 * returned scores are canonical fp32 dots of the fp32 query with the fp32 rows, no storage rounding at all
 * (what SURVEY.md §8(b) lists as the fp32 variant of rarc_score_topk).  The scan kernels still stream a 2-byte
 * image: the index holds fp32 rows [ceil32(n)][d_pad] for the rescore AND their fp16 image for the scan (6 bytes per
 * element); candidates are discarded on the image's int8 scores under a bound that includes the image's rounding.
 *   rarc_ingest_f32  normalise exactly as rarc_ingest_f16, store the fp32 row (zero padded) and its fp16 image
 *   metadata         rarc_quant_meta_f16 on the IMAGE; then the caller writes d_qmeta[1] = rho >= max ||d32 - d16||
 *                    (2^-11 * max||d|| + 2^-25 * sqrt(d_pad) covers normal and subnormal halves)
 *   rarc_search_f32  int8-prefilter scan of the image + canonical finalize on the fp32 rows
 *   rarc_repair_f32  exact single-query repair / verification on the fp32 rows
 */
int rarc_ingest_f32(const float* d_in, int64_t ld_in, float* d_corpus_f32, uint16_t* d_image_f16, int d_pad,
                    float* d_row_norm2, int64_t n_rows, int d, int normalize, void* stream);
int rarc_search_f32(const float* d_corpus_f32, const uint16_t* d_image_f16, int64_t n_rows, int d_pad,
                    const float* d_qmeta, const void* d_qblock, int nq, int k, int kprime, int64_t id_base,
                    float bin_lo, float bin_hi, int64_t* d_out_ids, float* d_out_scores, uint32_t* d_status,
                    void* d_workspace, size_t workspace_bytes, int cand_cap, void* stream);
/*
 * ABI 600 — one batch in one call: rarc_prep_queries + the rarc_search_* of the row format, i.e. the whole of
 *   VectorStore_Faiss.py:258-263 (`np.array([embedding]).astype(float32)`, `_normalize_vectors`, `index.search`)
 * for up to 256 queries, with what the two-call form needs a launch each for folded into the kernels that run anyway:
 *   d_status   RARC_MAX_QUERIES + 1 words; ZEROED by the query-prep kernel (the two-call form expects zeros from its caller)
 *   flag_host  pinned host word or NULL: zeroed by the query-prep kernel and set non-zero by the finalize kernel when any query
 *              is flagged — what a host otherwise copies out of d_status[RARC_MAX_QUERIES] behind the search; read it after an
 *              event recorded behind this call has completed
 *   gate_event hipEvent_t or NULL: the SCAN waits for it, the query prep and the seed pass in front of the scan do not.  Two
 *              search contexts (each its own query block, workspace and stream) that gate their scans on each other's
 *              completion run one batch's prep / seed under the other's finalize instead of behind it (config 2: 5 % per batch).
 * row_format 0: fp16 rows (d_aux NULL) · 1: fp8 rows, d_aux = float row scales · 2: fp32 rows, d_aux = their fp16 image ·
 *            3: fp16 rows, d_aux = int8 shadow image.  Everything else as in rarc_prep_queries / rarc_search_*.
 */
typedef struct RarcSearchBatch {
  const void* d_rows; const void* d_aux; int row_format; int64_t n_rows; int d_pad; const float* d_qmeta;
  const float* d_queries; int64_t ld_queries; int nq; int d; int normalize; float corpus_max_norm; void* d_qblock;
  int k, kprime; int64_t id_base; float bin_lo, bin_hi;
  int64_t* d_out_ids; float* d_out_scores; uint32_t* d_status; uint32_t* flag_host;
  void* d_workspace; size_t workspace_bytes; int cand_cap;
  void* gate_event;
} RarcSearchBatch;
int rarc_search_batch(const RarcSearchBatch* batch, void* stream);

/*
 * Measurement helper (ABI 600): stream n_bytes of device memory through every CU once (16-byte loads, eight in flight per lane,
 * one persistent workgroup per CU) and return nothing but a checksum — the READ ceiling of this part's HBM as a kernel
 * of the scan's shape can reach it, which bench.py reports next to the nominal 8 TB/s ("report against both").
 * d_sink: 8 bytes of device memory.  Time it with events on `stream`.
 */
int rarc_stream_read(const void* d_src, size_t n_bytes, void* d_sink, void* stream);

/*
 * Okapi BM25 (core/retrieval/bm25.py: BM25Retriever over rank_bm25 0.2.2's BM25Okapi.get_scores), ABI 600.
 * Index: a term-major CSR built on the host — d_post_off [n_terms + 1] int64, d_post_doc int32 (ascending within each
 * term), d_post_w fp64 (the reference's per-posting fraction tf*(k1+1) / (tf + k1*((1-b) + b*dl/avgdl))).
 * Queries: d_q_off [nq + 1] int32 into d_q_term int32 / d_q_idf fp64 (tokens in query order, duplicates kept, OOV tokens
 * left out).  score[d] = sum over the query's tokens in order of idf * w, fp64, no fused multiply-add: bit-identical to
 * the reference.  Limits: 1 <= n_docs <= 2^31 - 1 - 8192, nq <= 65535.
 * rarc_bm25_topk: the k best per query (1 <= k <= min(1024, n_docs)), score descending, doc index ascending among equal
 * scores, into d_out_ids [nq][k] / d_out_scores [nq][k].  Documents no token reaches score 0.0 and take part.
 * rarc_bm25_scores: every score, d_out_scores [nq][n_docs].
 * d_workspace: rarc_bm25_workspace_bytes(nq, n_query_tokens, n_docs, k) bytes (k = 0 for rarc_bm25_scores); 0 = bad sizes.
 */
size_t rarc_bm25_workspace_bytes(int nq, int64_t n_query_tokens, int64_t n_docs, int k);
int rarc_bm25_topk(const int64_t* d_post_off, const int32_t* d_post_doc, const double* d_post_w, int64_t n_terms,
                   int64_t n_docs, const int32_t* d_q_off, const int32_t* d_q_term, const double* d_q_idf, int nq,
                   int64_t n_query_tokens, int k, void* d_workspace, size_t workspace_bytes, int64_t* d_out_ids,
                   double* d_out_scores, void* stream);
int rarc_bm25_scores(const int64_t* d_post_off, const int32_t* d_post_doc, const double* d_post_w, int64_t n_terms,
                     int64_t n_docs, const int32_t* d_q_off, const int32_t* d_q_term, const double* d_q_idf, int nq,
                     int64_t n_query_tokens, void* d_workspace, size_t workspace_bytes, double* d_out_scores,
                     void* stream);

int rarc_repair_f32(const float* d_corpus_f32, int64_t n_rows, int d_pad, const void* d_qblock, int q, int k,
                    int64_t id_base, int64_t* d_out_ids, float* d_out_scores, uint32_t* d_found, void* d_workspace,
                    size_t workspace_bytes, void* stream);

/*
 * Merge G sorted candidate lists per query into the global top-k
 * (score desc, id asc).  Used after the RCCL all-gather of per-shard results
 * (SURVEY.md §8e).  Inputs are [G][nq][k]; outputs [nq][k].
 */
int rarc_topk_merge(const int64_t* d_ids, const float* d_scores, int n_lists, int nq, int k,
                    int64_t* d_out_ids, float* d_out_scores, void* stream);
/*
 * The same merge over lists in the form that crosses the all-gather as ONE tensor: int32 [n_lists][nq][k][3] =
 * (id low word, id high word, fp32 score bits).  rarc_pack_results writes one rank's [nq][k][3] block.
 */
int rarc_pack_results(const int64_t* d_ids, const float* d_scores, int nq, int k, int32_t* d_packed, void* stream);
int rarc_topk_merge_packed(const int32_t* d_packed, int n_lists, int nq, int k, int64_t* d_out_ids,
                           float* d_out_scores, void* stream);

/*
 * Reciprocal-rank fusion, bit-exact with RRFusion.fuse at core/utils/Fusion.py:45-76.
 * For query b, list r holds d_len[b*n_lists + r] keys at
 * d_keys[(b*n_lists + r)*max_len ...] in rank order (rank = position + 1).
 * score(key) = sum over occurrences, in (list, position) order, of
 * 1.0 / (rrf_k + rank) in fp64; output order = score desc, ties in first-insertion
 * order; d_out_n[b] = number of fused entries written (<= top_k).
 */
int rarc_rrf_fuse(const int64_t* d_keys, const int32_t* d_len, int nq, int n_lists, int max_len,
                  double rrf_k, int top_k, int64_t* d_out_keys, double* d_out_scores,
                  int32_t* d_out_n, void* stream);

/*
 * Reranker score -> order step of Qwen3Reranker (core/rerank/Reranker_Qwen3.py:41-49, :70-74):
 * p_yes = exp(log_softmax([z_no, z_yes])[1]) evaluated the way the reference's
 * fp16 tensors evaluate it, then a stable descending sort.  Inputs are fp16
 * logits [nq][n]; outputs: fp16 scores (as uint16 bit patterns) and the
 * permutation (int32) per query.
 */
int rarc_rerank_order(const uint16_t* d_z_no, const uint16_t* d_z_yes, int nq, int n,
                      uint16_t* d_out_scores_f16, int32_t* d_out_perm, void* stream);

/*
 * Maximal-marginal-relevance selection — the greedy loop of _mmr_select (VectorStore_Faiss.py:16-62) over candidates
 * that are already on the device (the resident rows of the fetch_k nearest neighbours, gathered: no re-embedding).
 * float64 arithmetic; candidate 0 first, then k - 1 rounds of  lambda·<q, e_i> − (1 − lambda)·max(0, max_sel <e_s, e_i>),
 * first maximum wins (python's max).  normalize != 0: query and candidates are divided by their norms first (cosine
 * stores, :308-312).  d_out: min(k, n) candidate indices in selection order.  d_work: rarc_mmr_workspace_doubles(n, d).
 */
size_t rarc_mmr_workspace_doubles(int n, int d);
int rarc_mmr_select(const float* d_cand, int64_t ld, const double* d_query, int n, int d, int normalize, int k,
                    double lambda, double* d_work, int32_t* d_out, void* stream);

/* rarc_mmr_select for a BATCH of queries, the candidates read straight from resident rows: one workgroup per query, no gather,
 * no widened copy.  For every query the picks are, index for index, what rarc_mmr_select returns for the same candidates
 * gathered to fp32 (fp16 widened exactly; fp8 decoded to fp32 and multiplied by the row scale in fp32; fp32 as is; elements
 * 0 .. d-1 of each row) and the same float64 query: every sum is the same sequential float64 sum over m = 0 .. d-1.
 *   d_rows      fmt 0: fp16 rows [n_rows][d_pad] · 1: fp8 e4m3fn rows, d_rowscale = float [n_rows] · 2: fp32 rows.
 *               16-byte aligned, d <= d_pad, d_pad a multiple of 16
 *   d_queries   float64, query q at d_queries + q * ldq (ldq >= d)
 *   d_cand_ids  int64 [nq][n], n <= 1024: what a search for n results returns — ids INCLUDING id_base.  A query's candidates
 *               are its entries that name a row (id - id_base in [0, n_rows)), in order; -1 padding is skipped
 *   d_out_ids   int64 [nq][k]: the selected candidates' ids in selection order, -1 beyond min(k, candidates of the query);
 *               k >= the number of candidates: the candidates in their given order
 *   d_ws        rarc_mmr_rows_workspace_bytes(nq, n, d) bytes (0 for sizes the call refuses), 8-byte aligned
 * RARC_E_UNSUPPORTED: n > 1024 · RARC_E_WORKSPACE: workspace too small / misaligned · RARC_E_INVALID: null pointer, bad
 * sizes, unknown fmt, fp8 rows without scales.  Nothing is launched on a refused call.
 */
size_t rarc_mmr_rows_workspace_bytes(int nq, int n, int d);
int rarc_mmr_select_rows(const void* d_rows, int fmt, const float* d_rowscale, int64_t n_rows, int d_pad, int d,
                         const double* d_queries, int64_t ldq, int nq, const int64_t* d_cand_ids, int n, int64_t id_base,
                         int normalize, int k, double lambda, int64_t* d_out_ids, void* d_ws, size_t ws_bytes, void* stream);

/*
 * Deterministic synthetic corpus / query generator (bench + full-size property
 * tests): counter-based integer hash -> 52-bit uniform -> N(0,1) by the inverse normal CDF (Wichura AS 241,
 * exactly rounded double operations only) -> integer on a 2^-20 grid -> exact
 * integer sum of squares -> fp64 scale -> fp16 (RNE).  Bit-identical to
 * oracle/rarc_oracle.c:synth_rows_f16.  Row r of the stream `seed` depends only
 * on (seed, first_row + r, d).
 */
int rarc_synth_rows_f16(uint16_t* d_out_f16, int d_pad, int d, int64_t first_row, int64_t n_rows,
                        uint64_t seed, void* stream);
int rarc_synth_rows_f32(float* d_out_f32, int64_t ld_out, int d, int64_t first_row,
                        int64_t n_rows, uint64_t seed, void* stream);

/*
 * Encoder forward (BERT family) — what HuggingFaceEmbeddings reaches through
 * sentence-transformers at core/file_management/embeddings/huggingface.py:122-126
 * ([external] BERT forward -> CLS pooling -> optional normalise).  Token ids in, embeddings out.
 * All tensors fp16 (uint16 bit patterns) unless noted; weights use torch.nn.Linear layout [out][in].
 *   rarc_enc_embed_ln : out[t] = LayerNorm(word[ids[t]] + pos[t % seq_len] + type0); `vocab` = rows of d_word:
 *                       an id outside [0, vocab) is clamped into the table (memory safety only — callers
 *                       validate ids on the host, as the python binding does)
 *   rarc_enc_gemm     : C[M][N] = A[M][K] · W[N][K]^T + bias[N], act 0 = none, 1 = erf-GELU, 3 = SwiGLU over gate/up
 *                       columns interleaved in groups of 8 (C is then [M][N/2]; large shapes only, see RarcLmLayer);
 *                       M, N multiples of 128, K multiple of 64 (MFMA 32x32x16 f16, fp32 accumulate)
 *   rarc_enc_attention: ctx = softmax(Q K^T / sqrt(dh) + key mask) V per (sequence, head) from the
 *                       fused qkv [n_seq*seq_len][3*hidden]; keys >= d_lens[seq] are masked; dh 32 or 64
 *   rarc_enc_add_ln   : out = LayerNorm(x + resid)
 *   rarc_enc_pool     : out[b] = hidden[b*seq_len + 0] as fp32 (optionally L2-normalised)          [CLS pooling]
 *   rarc_enc_pool_mean: out[b] = mean over the d_lens[b] real tokens of hidden[b*seq_len + t], fp32  [mean pooling]
 * Limits, refused with an error code before anything is launched: n_tokens, n_rows, n_seq, seq_len > 0 everywhere;
 * embed_ln / add_ln: hidden a POSITIVE multiple of 64, <= 1024; attention: hidden = n_heads * {32, 64}, seq_len <= 512;
 * pool: hidden a positive multiple of 8; pool_mean: the same, <= 1024.  d_lens[b] is clamped into [1, seq_len].
 */
int rarc_enc_embed_ln(const int32_t* d_ids, const uint16_t* d_word, const uint16_t* d_pos,
                      const uint16_t* d_type0, const uint16_t* d_gamma, const uint16_t* d_beta, float eps,
                      int n_tokens, int seq_len, int hidden, int vocab, uint16_t* d_out, void* stream);
int rarc_enc_gemm(const uint16_t* d_a, const uint16_t* d_w, const uint16_t* d_bias, uint16_t* d_c, int m,
                  int n, int k, int act, void* stream);
/* The same product for a caller whose bias is KNOWN to be zeros (the reranker LM's projections have none): d_zero_bias holds
 * n zeros; act 0 or 3.  Lets the large shapes run the tile kernel without a seam between output tiles (round 3), which has
 * no bias path; every other shape is rarc_enc_gemm. */
int rarc_enc_gemm_zero_bias(const uint16_t* d_a, const uint16_t* d_w, const uint16_t* d_zero_bias, uint16_t* d_c, int m,
                            int n, int k, int act, void* stream);
int rarc_enc_attention(const uint16_t* d_qkv, const int32_t* d_lens, int n_seq, int seq_len, int hidden,
                       int n_heads, uint16_t* d_ctx, void* stream);
int rarc_enc_add_ln(const uint16_t* d_x, const uint16_t* d_resid, const uint16_t* d_gamma,
                    const uint16_t* d_beta, float eps, int n_rows, int hidden, uint16_t* d_out, void* stream);
int rarc_enc_pool(const uint16_t* d_hidden, int n_seq, int seq_len, int hidden, int normalize,
                  float* d_out, void* stream);
int rarc_enc_pool_mean(const uint16_t* d_hidden, const int32_t* d_lens, int n_seq, int seq_len, int hidden,
                       int normalize, float* d_out, void* stream);

/*
 * Whole encoder forward in one call: the launch loop over the layers runs on the host side of this
 * library, not in the caller (at small batches the per-call overhead of a foreign-function binding is
 * longer than the kernels).  `model` and `model->layers` are HOST structs of DEVICE pointers.
 * `normalize`: bit 0 = L2-normalise the pooled vector, bit 1 = mean pooling over the real tokens instead of CLS.
 * n_seq*seq_len must be a multiple of 128 (pad seq_len to a multiple of 32 with masked tokens and n_seq to a
 * multiple of 4 with sequences of length 1); d_lens[s] in [1, seq_len] (clamped into that range).  d_ws: scratch of
 * rarc_enc_workspace_bytes(hidden, inter, n_seq*seq_len) bytes.  d_out: fp32 [n_seq][hidden].
 */
typedef struct RarcEncLayer {
  const uint16_t *qkv_w, *qkv_b; /* fused [3*hidden][hidden], [3*hidden] (query, key, value) */
  const uint16_t *o_w, *o_b, *ln1_g, *ln1_b;
  const uint16_t *f1_w, *f1_b, *f2_w, *f2_b, *ln2_g, *ln2_b;
} RarcEncLayer;
typedef struct RarcEncModel {
  int hidden, heads, inter, n_layers;
  float ln_eps;
  const uint16_t *word, *pos, *type0, *emb_g, *emb_b;
  const RarcEncLayer* layers; /* host array [n_layers] */
  int vocab;   /* rows of `word`  (REQUIRED > 0: token ids are clamped into [0, vocab)) */
  int max_pos; /* rows of `pos`   (REQUIRED >= seq_len) */
  /* MPNet family (the reference's default checkpoint, sentence-transformers/all-mpnet-base-v2, huggingface.py:6): one
   * relative-position bias shared by all layers, added to the scaled scores before the softmax
   * (transformers MPNetEncoder.compute_position_bias).  It depends on key - query only:
   * rel_bias fp32 [heads][2*rel_span - 1], entry [h][key - query + rel_span - 1]; null = none (BERT).
   * REQUIRED rel_span >= seq_len when set.  (MPNet's position ids start at 2 and it has no token types: pass
   * pos = table + 2 rows, max_pos = rows - 2, type0 = zeros.) */
  const float* rel_bias;
  int rel_span;
} RarcEncModel;
size_t rarc_enc_workspace_bytes(int hidden, int inter, int n_tokens);
int rarc_enc_forward(const RarcEncModel* model, const int32_t* d_ids, const int32_t* d_lens, int n_seq,
                     int seq_len, int normalize, void* d_ws, size_t ws_bytes, float* d_out, void* stream);

/*
 * The same forward at the REFERENCE's precision (fp32-class; `precision = "fp32"` of the embedding provider).
 * `SentenceTransformer(model_name, **model_kwargs)` (huggingface.py:96-98) loads fp32 weights and `.encode` (:122-126)
 * runs an fp32 forward; rarc_enc_forward above is an fp16 approximation of it (1e-3 class), this one agrees with an
 * fp32 forward to fp32 rounding noise.  The GEMMs run on the fp16 MFMA over SPLIT operands: x*s = hi + lo (two fp16
 * numbers, s a power of two per row, together 22 bits of x), C = [A_lo|A_hi|A_hi] * [W_hi|W_lo|W_hi]^T / (s_a s_w): one
 * fp16 GEMM over K' = 3K with fp32 accumulation.  Residual stream, LayerNorm, GELU (libm erff), softmax (libm expf),
 * attention products and pooling are fp32.
 *   rarc_enc32_split_weight : W fp32 [n][k] (torch Linear layout) -> d_w3 fp16 [n][3k] = [hi | lo | hi], d_rw fp32 [n] = 1/s_w
 *   rarc_enc32_split_rows   : X fp32 [m][k] -> d_a3 fp16 [m][3k] = [lo | hi | hi], d_ra fp32 [m] = 1/s_a   (k % 4 == 0, k <= 4096)
 *   rarc_enc32_gemm         : C fp32 [m][n] = X W^T + bias from the two split images (m, n multiples of 128, k of 64)
 *   rarc_enc32_forward      : token ids -> fp32 embeddings; arguments as rarc_enc_forward; hidden <= 1024, inter <= 4096
 */
typedef struct RarcEnc32Layer {
  const uint16_t* qkv_w3; const float *qkv_rw, *qkv_b;           /* fused [3*hidden][3*hidden] split rows, [3*hidden], [3*hidden] */
  const uint16_t* o_w3;   const float *o_rw, *o_b, *ln1_g, *ln1_b;
  const uint16_t* f1_w3;  const float *f1_rw, *f1_b;
  const uint16_t* f2_w3;  const float *f2_rw, *f2_b, *ln2_g, *ln2_b;
  const float* f1_colmax;   /* ABI 401.  float [hidden + 1]: c[k] = max_j |W1[j][k]| of the fp32 FFN1 weight, c[hidden] = max_j |b1[j]|;
                               NULL = none.  With it, batches that fill the chip run FFN1 with bias + GELU + the split of its output
                               fused into the GEMM (the row's power-of-two scale comes from the bound sum_k |x_k| c[k] + c[hidden]
                               >= max_j |gelu(x·W1_j + b1_j)|, known before the GEMM); without it FFN1 is a product + a row pass. */
  /* ABI 600 — the QUERY PATH's weight images (rarc_enc32_pack_query_weight), one per projection, NULL = none.  With all four
   * present in every layer, a forward of 32 / 64 / 128 tokens (one to four 32-token queries: the reference's embed_query,
   * core/file_management/embeddings/huggingface.py:136-145) runs its projections as weight streams over these images instead
   * of the 128 x 128 tile kernels over *_w3.  uint16 (fp16 bits) [n / 32][k / 16][2][64][8]: per 32 output features and 16-wide
   * k step the W_hi fragment, then the W_lo fragment, each in the lane order of a v_mfma_f32_32x32x16_f16 A operand. */
  const uint16_t *qkv_wq, *o_wq, *f1_wq, *f2_wq;
} RarcEnc32Layer;
typedef struct RarcEnc32Model {
  int hidden, heads, inter, n_layers;
  float ln_eps;
  const float *word, *pos, *type0, *emb_g, *emb_b; /* fp32 tables and LayerNorm parameters */
  const RarcEnc32Layer* layers;                    /* host array [n_layers] */
  int vocab, max_pos;                              /* REQUIRED, as in RarcEncModel */
  const float* rel_bias;                           /* relative-position attention bias, as in RarcEncModel (null = none) */
  int rel_span;
} RarcEnc32Model;
int rarc_enc32_split_weight(const float* d_w, int n, int k, uint16_t* d_w3, float* d_rw, void* stream);
/* d_w3: the split rows of an [n][k] weight (rarc_enc32_split_weight) -> d_wq: n*k*2 halves, the query path's image of the same
 * weight (RarcEnc32Layer.*_wq).  n a multiple of 32, k a multiple of 128. */
int rarc_enc32_pack_query_weight(const uint16_t* d_w3, int n, int k, uint16_t* d_wq, void* stream);
int rarc_enc32_split_rows(const float* d_x, int m, int k, uint16_t* d_a3, float* d_ra, void* stream);
int rarc_enc32_gemm(const uint16_t* d_a3, const float* d_ra, const uint16_t* d_w3, const float* d_rw,
                    const float* d_bias, float* d_c, int m, int n, int k, void* stream);
size_t rarc_enc32_workspace_bytes(int hidden, int inter, int n_tokens);
int rarc_enc32_forward(const RarcEnc32Model* model, const int32_t* d_ids, const int32_t* d_lens, int n_seq,
                       int seq_len, int normalize, void* d_ws, size_t ws_bytes, float* d_out, void* stream);

/*
 * Reranker LM forward — what Qwen3Reranker.compute_logits takes from the causal LM
 * (core/rerank/Reranker_Qwen3.py:41-49: `self.lm(**inputs).logits[:, -1, :]` at the ids of "no" and "yes") for
 * the LEFT-padded batches process_inputs builds (:29-39).  Qwen3-style decoder: RMSNorm, fused q|k|v projection
 * with grouped K/V heads, per-head q/k RMSNorm, rotary embedding (rotate-half), causal attention, SwiGLU MLP, no
 * biases; fp16 weights (torch.nn.Linear layout [out][in]) and activations, fp32 accumulation.
 *   d_ids    int32 [n_seq][seq_len], left padded;  d_start int32 [n_seq]: index of each sequence's first real token
 *            (positions run 0..seq_len-1 over the padded sequence, as in the reference's forward)
 *   d_out    fp16 [n_seq][2]: (logit of no_id, logit of yes_id) at the last position — the input of rarc_rerank_order
 * n_seq*seq_len a multiple of 128; head_dim 64 or 128; hidden, inter, (n_q+2*n_kv)*head_dim multiples of 128.
 * `model`, `model->layers` are HOST structs of DEVICE pointers; zero_bias: max(hidden, 2*inter, qkv width) zeros.
 */
typedef struct RarcLmLayer {
  const uint16_t *in_norm, *qkv_w, *q_norm, *k_norm, *o_w, *post_norm, *gate_up_w, *down_w;
  /* OPTIONAL (null = not supplied; ABI 320): qkv_w with its columns multiplied by in_norm, gate_up_w with its columns
   * multiplied by post_norm (products in fp32, rounded to fp16 once).  With both present, batches large enough for the 256-row
   * tile kernels run WITHOUT the RMSNorm passes: RMSNorm(x)·Wᵀ = r ⊙ (x·(W ⊙ γ)ᵀ) with r = rsqrt(mean(x²) + eps) per row, so
   * the projection reads the residual stream itself and scales its output rows, and the output / down projections add into
   * the residual stream in their epilogue.  Same function, one rounding moved: the reference rounds the normed
   * activations to fp16 before the product. */
  const uint16_t *qkv_w_folded, *gate_up_w_folded;
  /* qkv_w [(n_q+2*n_kv)*head_dim][hidden] = q_proj | k_proj | v_proj rows;
   * gate_up_w [2*inter][hidden] = gate_proj and up_proj rows INTERLEAVED in groups of 8: rows 16b .. 16b+7 are
   * gate_proj rows 8b .. 8b+7, rows 16b+8 .. 16b+15 the up_proj rows of the same features (so that one lane of the
   * GEMM's 32 x 32 MFMA blocks holds gate and up of a feature and the SwiGLU is its epilogue; inter % 8 == 0) */
} RarcLmLayer;
typedef struct RarcLmModel {
  int hidden, n_layers, n_q_heads, n_kv_heads, head_dim, inter, vocab;
  float rms_eps, rope_theta;
  const uint16_t *embed, *lm_head, *final_norm, *zero_bias;
  const RarcLmLayer* layers; /* host array [n_layers] */
} RarcLmModel;
size_t rarc_lm_workspace_bytes(const RarcLmModel* model, int n_tokens);
int rarc_lm_yes_no_logits(const RarcLmModel* model, const int32_t* d_ids, const int32_t* d_start, int n_seq,
                          int seq_len, int no_id, int yes_id, void* d_ws, size_t ws_bytes, uint16_t* d_out_f16,
                          void* stream);

/*
 * Shared prompt prefixes.  The prompts Qwen3Reranker.rerank scores for ONE query (Reranker_Qwen3.py:23-27,57-66) are
 * identical up to the document text — chat prefix, instruction, query: ~80 of ~220 tokens — and in a causal LM the keys and
 * values of those tokens do not depend on what follows them.  rarc_lm_prefix_kv runs the n_prefix LEFT-padded prefixes
 * [n_prefix][prefix_len] once and stores every layer's raw k | v rows in d_cache (rarc_lm_prefix_cache_bytes(model,
 * n_prefix * prefix_len) bytes); rarc_lm_yes_no_logits_prefixed then runs only the REMAINDERS d_ids [n_seq][seq_len] (left
 * padded), sequence s attending to the cache rows of prefix d_prefix_of[s] (from d_prefix_start[prefix]) and then to its own
 * tokens; rotary positions continue from prefix_len.  Same logits as rarc_lm_yes_no_logits on the concatenated prompts up to
 * fp16 rounding (rotary embeddings are relative; the softmax sums run in a different order).  n_prefix * prefix_len and
 * n_seq * seq_len multiples of 128.  d_prefix_of[s] = -1: no prefix for s.
 */
size_t rarc_lm_prefix_cache_bytes(const RarcLmModel* model, int n_prefix_tokens);
int rarc_lm_prefix_kv(const RarcLmModel* model, const int32_t* d_ids, const int32_t* d_start, int n_prefix, int prefix_len,
                      void* d_ws, size_t ws_bytes, void* d_cache, size_t cache_bytes, void* stream);
int rarc_lm_yes_no_logits_prefixed(const RarcLmModel* model, const int32_t* d_ids, const int32_t* d_start, int n_seq,
                                   int seq_len, const int32_t* d_prefix_of, const void* d_cache, int n_prefix,
                                   int prefix_len, const int32_t* d_prefix_start, int no_id, int yes_id, void* d_ws,
                                   size_t ws_bytes, uint16_t* d_out_f16, void* stream);

/*
 * Decoder-LM embeddings — the same forward with the ending of a sentence-transformers decoder embedder (Qwen3-Embedding:
 * Transformer -> Pooling(lasttoken) -> Normalize; the reference's provider wraps any such model,
 * core/file_management/embeddings/huggingface.py:12-22,96-98).  For LEFT-padded batches the last position is every
 * sequence's last real token, so the embedding is the final RMSNorm of the last residual row, with the roundings of the
 * logits path (the reference's fp16 model): nv[c] = half(final_norm[c] * half(x[c] * inv)), inv in fp32.
 *   d_out    fp32 [n_seq][ld_out], columns [0, out_dim) written, the rest untouched
 *   out_dim  1 .. hidden: the first out_dim components (Matryoshka truncation, sentence-transformers' truncate_dim)
 *   normalize 0: (float)nv[c];  1: nv[c] / max(||nv[0..out_dim)||, 1e-12), the sum of squares in fp32 over the out_dim
 *            components kept (truncation first, then Normalize); an all-zero row gives zeros
 * model->lm_head is not read and may be null (Qwen3Model checkpoints have no head).  Shapes, d_ids / d_start, the workspace
 * (rarc_lm_workspace_bytes) and the prefix arguments are those of the logits calls; additionally 1 <= out_dim <= hidden and
 * ld_out >= out_dim.  The last layer still runs on the last positions only when its compact buffers fit.
 */
int rarc_lm_embed_last(const RarcLmModel* model, const int32_t* d_ids, const int32_t* d_start, int n_seq, int seq_len,
                       int out_dim, int normalize, void* d_ws, size_t ws_bytes, float* d_out, int64_t ld_out, void* stream);
int rarc_lm_embed_last_prefixed(const RarcLmModel* model, const int32_t* d_ids, const int32_t* d_start, int n_seq,
                                int seq_len, const int32_t* d_prefix_of, const void* d_cache, int n_prefix,
                                int prefix_len, const int32_t* d_prefix_start, int out_dim, int normalize, void* d_ws,
                                size_t ws_bytes, float* d_out, int64_t ld_out, void* stream);

/*
 * Decoder layer pieces — each kernel of the forward above alone, launched through the dispatch the forward itself uses (the
 * tests compare every one with a float64 reference; the GEMMs between them are rarc_enc_gemm).  fp16 tensors as uint16 bits.
 *   rarc_lm_rope_table    : d_table [n_rows][head_dim]: cos of the head_dim/2 pairs, then their sin, of angle row * theta^(-2i/head_dim)
 *   rarc_lm_rmsnorm       : d_delta != null: x += delta (one fp16 rounding, WRITTEN BACK to d_x); d_y != null:
 *                           y = half(w * half(x * rsqrt(mean(x^2) + eps))); d_y = null only adds (d_w may then be null)
 *   rarc_lm_rowscale_parts: r[t] = rsqrt(sum(d_ssq[t][0..n_parts)) / hidden + eps): the row scales from the partial sums of
 *                           squares (one per 32 columns) the residual GEMM epilogue leaves; n_parts = hidden / 32
 *   rarc_lm_swiglu        : out[t][j] = half(half(silu(g)) * u) from d_gate_up [n_rows][2*inter], columns in groups of 16: 8 gates,
 *                           then the 8 ups of the same features
 *   rarc_lm_attention     : ctx [n_seq*seq_len][n_q*head_dim] from the fused q|k|v rows [n_seq*seq_len][(n_q+2*n_kv)*head_dim]:
 *                           per-head RMSNorm (d_q_norm / d_k_norm [head_dim]) + rotary embedding of q and k, causal softmax
 *                           over the keys of a left-padded sequence, optionally after the raw k|v rows of a shared prefix
 *                           (d_prefix_kv [n_prefix][prefix_len][2*n_kv*head_dim], null = none; d_prefix_of [n_seq] in
 *                           [-1, n_prefix), -1 = no prefix for that sequence; d_prefix_start [n_prefix]).  d_rope: a
 *                           rarc_lm_rope_table of rope_rows rows.  Keys run in a virtual index u: u < P = prefix_len is cache
 *                           row u, u >= P own row start + (u - P); query row i sits at u = P + (i - start) and sees
 *                           [prefix_start, u].  Rotary position of u: u with a prefix, u + start without (the row's index in the
 *                           padded sequence).  d_start[s] is clamped into [0, seq_len - 1], d_prefix_start[p] into [0, P - 1].
 *                           `kernel`: 0 = what the forward would run (RARC_LM_ATTN=stream included), 1 = the streaming kernel,
 *                           2 = the LDS-resident kernel; 2 is refused (RARC_E_UNSUPPORTED) when round32(P + seq_len) keys do not
 *                           fit (288 keys at head_dim 128, 544 at 64) — no fallback.  n_seq * seq_len need NOT be a multiple
 *                           of 128 (that is the GEMMs' limit).
 *                           What is read: of a sequence's own rows before `start` only the q columns (never k | v); of the
 *                           cache only the rows of prefixes some sequence names, and of those the rows from
 *                           32 * (prefix_start / 32) on.  Rows in [32 * (prefix_start / 32), prefix_start) and rows of the
 *                           sequence behind a query take part with probability exactly 0: they MUST BE FINITE (0 * NaN would
 *                           reach the output), their values do not matter.  Everything else may hold anything, NaN included.
 *                           A padding query (row i < start) sees no key and gets a ZERO context row without a prefix; with one
 *                           it sees cache rows [prefix_start, P - (start - i)] (its row is written, nothing ever reads it).
 *   rarc_lm_last_logits   : d_out fp16 [n_seq][2] = <half(w * half(x * inv)), lm_head[{no_id, yes_id}]> of row
 *                           s * row_stride + row_off of d_x ([..][hidden]); the forward's two forms: (seq_len, seq_len - 1) and
 *                           (1, 0).  d_lm_head [vocab][hidden]
 *   rarc_lm_last_embed    : the same row and roundings, the normed row itself as fp32 (rarc_lm_embed_last's out_dim / normalize /
 *                           ld_out)
 *   rarc_lm_gather_last   : d_dst[s] = d_src[s * seq_len + seq_len - 1] for s < n_seq, ZERO rows for n_seq <= s < n_rows; rows of
 *                           `width` halves
 * Limits, refused with an error code before anything is launched: every count (n_rows, n_seq, seq_len, hidden, inter, width,
 * n_q, n_kv, vocab, and n_prefix / prefix_len with a cache) > 0; head_dim 64 or 128; n_q % n_kv == 0; hidden a multiple of 8
 * (rmsnorm) or of 128 with n_parts == hidden / 32 (rowscale_parts: its partial sums load as float4); inter and width multiples
 * of 8; rope_rows >= prefix_len + seq_len; prefix_len <= 4096; 0 <= row_off < row_stride; token ids in [0, vocab);
 * 1 <= out_dim <= hidden, ld_out >= out_dim; n_rows >= n_seq (gather_last); theta > 0, n_rows * head_dim / 2 < 2^31 (rope_table).
 */
int rarc_lm_rope_table(int n_rows, int head_dim, float theta, uint16_t* d_table, void* stream);
int rarc_lm_rmsnorm(uint16_t* d_x, const uint16_t* d_delta, const uint16_t* d_w, float eps, int n_rows, int hidden, uint16_t* d_y,
                    void* stream);
int rarc_lm_rowscale_parts(const float* d_ssq, int n_parts, float eps, int n_rows, int hidden, float* d_r, void* stream);
int rarc_lm_swiglu(const uint16_t* d_gate_up, int n_rows, int inter, uint16_t* d_out, void* stream);
int rarc_lm_attention(const uint16_t* d_qkv, const int32_t* d_start, int n_seq, int seq_len, int n_q, int n_kv, int head_dim,
                      const uint16_t* d_q_norm, const uint16_t* d_k_norm, float eps, const uint16_t* d_rope, int rope_rows,
                      const uint16_t* d_prefix_kv, const int32_t* d_prefix_of, const int32_t* d_prefix_start, int n_prefix,
                      int prefix_len, int kernel, uint16_t* d_ctx, void* stream);
int rarc_lm_last_logits(const uint16_t* d_x, const uint16_t* d_final_norm, const uint16_t* d_lm_head, float eps, int n_seq,
                        int row_stride, int row_off, int hidden, int vocab, int no_id, int yes_id, uint16_t* d_out, void* stream);
int rarc_lm_last_embed(const uint16_t* d_x, const uint16_t* d_final_norm, float eps, int n_seq, int row_stride, int row_off,
                       int hidden, int out_dim, int normalize, float* d_out, int64_t ld_out, void* stream);
int rarc_lm_gather_last(const uint16_t* d_src, int seq_len, int width, int n_seq, int n_rows, uint16_t* d_dst, void* stream);

/*
 * Batch WordPiece tokenisation on the host (no device involved) — what sits between the texts the reference hands to
 * `SentenceTransformer.encode` (core/file_management/embeddings/huggingface.py:116-126) and the encoder forward above: the
 * BERT tokeniser (native and multi-threaded in the reference's dependency too).  Same algorithm as the python restatement
 * encapsulation/embeddings/wordpiece.py (pinned to transformers.BertTokenizer), for ASCII texts, on n_threads cores.
 *   rarc_wordpiece_create   vocab_blob: the vocabulary's tokens separated by '\n', id = position (a vocab.txt image);
 *                           never_split_blob: the SPECIAL tokens, '\n'-separated — cut out of the raw text wherever they
 *                           occur, before anything else (unk / cls / sep / pad / mask and whatever else the caller lists);
 *                           the handle is the one object this library allocates — release it with _destroy
 *   rarc_wordpiece_encode   text i = bytes [text_offsets[i], text_offsets[i+1]) of text_blob;  h_ids [n_texts][ld_ids] int32
 *                           receives [CLS] ids[: max_length - 2] [SEP] padded to max_length with the pad id, h_lens[i] the
 *                           number of real ids — or -1 for a text with a byte >= 0x80, which is NOT tokenised here (its
 *                           Unicode normalisation steps are left to the python tokeniser; row i is then untouched)
 */
typedef struct RarcWordPiece RarcWordPiece;
int rarc_wordpiece_create(const char* vocab_blob, size_t blob_bytes, int do_lower_case, const char* unk_token,
                          const char* cls_token, const char* sep_token, const char* pad_token, const char* never_split_blob,
                          size_t never_split_bytes, int max_input_chars_per_word, RarcWordPiece** out);
void rarc_wordpiece_destroy(RarcWordPiece* wp);
int rarc_wordpiece_encode(const RarcWordPiece* wp, const char* text_blob, const int64_t* text_offsets, int n_texts,
                          int max_length, int32_t* h_ids, int64_t ld_ids, int32_t* h_lens, int n_threads);

/*
 * Shard files: bulk movement of stored rows between a file and HBM — the native I/O behind save_local / load_local,
 * counterpart of faiss.write_index / faiss.read_index at
 *   encapsulation/database/vector_db/VectorStore_Faiss.py:438 (save_local :432-450) and :467 (load_local :452-482)
 * for an index whose rows are resident in HBM.  A shard never exists as a host array: both calls stream
 * `n_seg` byte ranges (file offset h_file_off[s], h_bytes[s] bytes <-> device offset h_dev_off[s] from d_base) through a
 * ring of pinned host slots cut from h_staging (caller-owned PINNED memory, 4096-byte aligned; 2 * n_threads slots of
 * staging_bytes / (2 n_threads) bytes, >= 64 KiB each).  n_threads workers each alternate file transfer and DMA (two slots
 * per worker; the DMA is enqueued on `stream`), so disk and PCIe overlap and the host footprint is the ring whatever the
 * shard size.
 *   RARC_IO_DIRECT  also open the file O_DIRECT: chunks whose offset, length and slot are 4096-aligned bypass the page
 *                   cache (storage DMA -> pinned slot -> GPU DMA); a file system without O_DIRECT is served buffered
 *   RARC_IO_FSYNC   rarc_device_to_file: fsync before returning
 *   RARC_IO_TRUNCATE rarc_device_to_file: cut the file at the end of the furthest segment first (a caller overwriting a
 *                   LONGER file in one call; without it the file is never truncated: the .rarc writer sizes the file, writes
 *                   its header and small sections itself and lets this call fill the row section — DESIGN.md 3)
 * rarc_device_to_file creates the file if needed; rarc_file_to_device fails if the file is shorter than a segment.  File
 * errors (open, read / write, fsync: ENOSPC, EIO ...) return RARC_E_IO, HIP errors RARC_E_HIP.
 * Both are synchronous (the bytes are in place on return; `stream` is drained).  d_capacity_bytes bounds every
 * segment's device range.  `stats` (optional) receives what was moved and how fast.
 */
#define RARC_IO_DIRECT 1
#define RARC_IO_FSYNC 2
#define RARC_IO_TRUNCATE 4
typedef struct RarcIoStats {
  int64_t bytes;            /* bytes moved */
  double seconds;           /* wall time of the call's transfer phase */
  double file_seconds;      /* pread / pwrite time summed over the workers */
  double copy_wait_seconds; /* time the workers waited for their DMA, summed */
  int64_t direct_bytes;     /* of `bytes`, how many went through O_DIRECT */
  int64_t n_chunks, slot_bytes;
  int n_threads, direct;    /* direct: 1 if the O_DIRECT descriptor could be opened */
} RarcIoStats;
int rarc_file_to_device(const char* path, int n_seg, const int64_t* h_file_off, const int64_t* h_bytes,
                        const int64_t* h_dev_off, void* d_base, int64_t d_capacity_bytes, void* h_staging,
                        size_t staging_bytes, int n_threads, int flags, void* stream, RarcIoStats* stats);
int rarc_device_to_file(const char* path, int n_seg, const int64_t* h_file_off, const int64_t* h_bytes,
                        const int64_t* h_dev_off, const void* d_base, int64_t d_capacity_bytes, void* h_staging,
                        size_t staging_bytes, int n_threads, int flags, void* stream, RarcIoStats* stats);

/*
 * Exact top-k beyond what the register-resident scans take: rows wider than 1024 padded dimensions (up to 4096) and k up
 * to 8192 — faiss.IndexFlatIP takes any d and any k (encapsulation/database/vector_db/VectorStore_Faiss.py:101-115, :262-263;
 * the reference's other embedding source returns 1536- / 3072-d vectors, encapsulation/llm/openai_llm.py:139-161).
 * The score matrix goes through the encoder's MFMA GEMM one chunk of rows at a time (fp16 scores, never more than 64 MB of
 * them), a select pass nominates rows against a rising, rigorous threshold, and the finalize rescores the nominees with the
 * canonical fp32 inner product and orders them (score desc, id asc): ids and scores are the oracle's, bit for bit
 * (csrc/wide.hip has the bound).  fmt 0: fp16 rows; fmt 2: fp32 rows + their fp16 image (what the GEMM reads; rho >=
 * ||row - image||, as qmeta[1]).  d_qblock as written by rarc_prep_queries (which takes d_pad up to 4096).  d_status:
 * uint32 [256], a query whose candidate list filled up carries RARC_Q_OVERFLOW — call again with a larger cand_cap
 * (cand_cap >= n_rows cannot overflow; it must be at least max(16384, 2k) rounded up to 256, plus 256: the first chunk of rows — and a multiple of 8).
 */
size_t rarc_wide_workspace_bytes(int d_pad, int cand_cap);
int rarc_search_wide(const void* d_rows, const uint16_t* d_image16, int fmt, int64_t n_rows, int d_pad, float max_norm,
                     float rho, const void* d_qblock, int nq, int k, int64_t id_base, int64_t* d_out_ids,
                     float* d_out_scores, uint32_t* d_status, void* d_ws, size_t ws_bytes, int cand_cap, void* stream);

/*
 * Metric "l2": exact squared-Euclidean top-k (faiss.IndexFlatL2; VectorStore_Faiss.py:73-146 takes "l2" next to "cosine" and
 * "ip") on the same chunked GEMM + select + canonical finalize.  With dot() the canonical fp32 inner product,
 *     dist = max(0, (dot(q, q) + dot(x, x)) - 2 dot(q, x))      every operation fp32, x the stored row
 * ordered by (dist ascending, id ascending) — faiss's own expansion for batched L2 with summation and tie order pinned
 * (csrc/wide.hip has the bound that makes the nominee lists complete).
 * rarc_row_sqnorms: d_xn[r] = dot(x_r, x_r) for r in [first_row, n_rows) — fmt 0: fp16 rows [n_rows][d_pad], fmt 2: fp32 rows.
 * Derived data: recompute it for appended rows, from the first hole after rarc_compact_rows, for all rows after a load.
 * rarc_search_wide_l2: the arguments of rarc_search_wide plus d_xn (fp32 [n_rows]); d_out_scores receives the squared
 * distances, smallest first (+inf with id -1 beyond the stored rows); workspace and overflow protocol are rarc_search_wide's.
 * Takes every d_pad <= 4096 and k <= 8192 (there is no register-resident L2 scan).
 */
int rarc_row_sqnorms(const void* d_rows, int fmt, int64_t n_rows, int d_pad, int64_t first_row, float* d_xn, void* stream);
int rarc_search_wide_l2(const void* d_rows, const uint16_t* d_image16, int fmt, int64_t n_rows, int d_pad, float max_norm,
                        float rho, const float* d_xn, const void* d_qblock, int nq, int k, int64_t id_base, int64_t* d_out_ids,
                        float* d_out_scores, uint32_t* d_status, void* d_ws, size_t ws_bytes, int cand_cap, void* stream);
/* Test hook for the bound behind the two searches above (csrc/wide.hip): after a search on d_ws (same d_pad and cand_cap, same
 * stream or one ordered behind it) copies out what the search left there, d_out fp32 [4][256]: per query eps, the final
 * threshold thr (+inf for the padding queries), and after rarc_search_wide_l2 epsd = eps_k + delta and the canonical |q|^2
 * (undefined after rarc_search_wide).  Reads the workspace only; not used by any search. */
int rarc_debug_wide_bounds(const void* d_ws, size_t ws_bytes, int d_pad, int cand_cap, float* d_out, void* stream);
/* Test hook for the int8 scale of a prepared query (csrc/rarc_common.h: rarc_query_scale8, the function rarc_prep_queries'
 * kernel calls): for mx = max |element| of the prepared query, *sq = the multiplier of q8 = rint(v * sq) and *qi = 1 / sq, the
 * fp32 number the scan dequantises with.  Both are finite and positive for every mx (zero, subnormal, infinite and NaN
 * included) and mx * sq <= 127.4.  Host code only: touches no device, runs on a machine without one. */
int rarc_debug_query_scale8(float mx, float* sq, float* qi);
/* Test hooks for the dynamic tail of the int8-prefilter scan (csrc/scan_q8.hip).  Host code only: touch no device.
 * _plan: what the launcher decides for a launch over tiles [t_begin, n_tiles) on `grid` workgroups, rows of d_pad dimensions in
 * row format fmt, a dynamic share of pct per cent and a size limit of min_mib MiB of rows per workgroup: *t_dyn = first tile
 * handed out by ticket (== n_tiles: no tail), *r0 = tile rounds of a first-level chunk, *unit = rounds the loop consumes at once.
 * _chunks: the ranges of tickets k_first .. k_first + n - 1, t0[i] / t_end[i] = first tile and end of chunk i (tiles t0, t0 +
 * stride, ... below t_end; t0 >= n_tiles: past the end).  _counter_offset: byte offset in the search workspace of the uint32
 * ticket counter of the launch-th scan launch of a search (0-3; -1 otherwise), zero after a search whose launch had no tail. */
int rarc_debug_q8_tail_plan(uint32_t t_begin, uint32_t n_tiles, uint32_t grid, int d_pad, int fmt, int pct, int min_mib,
                            uint32_t* t_dyn, uint32_t* r0, uint32_t* unit);
int rarc_debug_q8_tail_chunks(uint32_t k_first, uint32_t n, uint32_t stride, uint32_t unit, uint32_t t_dyn, uint32_t r0,
                              uint32_t n_tiles, uint32_t* t0, uint32_t* t_end);
int64_t rarc_debug_q8_tail_counter_offset(int launch);

/*
 * Exact top-k over a LIST of rows of one index — the search behind a metadata filter (a LangChain-style `filter=` on the
 * store's search calls; the reference's FAISS store has no filter at all: encapsulation/database/vector_db/VectorStore_Faiss.py:212-274
 * ignores its kwargs).  Every listed row is scored once per query with the canonical fp32 inner product and ranked by the key
 * of rarc_search_wide's finalize: the answer is the unfiltered ranking (score desc, id asc; metric "l2": dist asc, id asc) with
 * the rows outside the list struck out, cut at k — ids and score bits are the oracle's.  No approximate pass, no bound, no
 * overflow: d_status (uint32 [256]) comes back all RARC_Q_OK.
 *   d_rows    fmt 0: fp16 rows [n_rows][d_pad]; fmt 2: fp32 rows.  d_pad a multiple of 128, <= 4096
 *   d_qblock  as written by rarc_prep_queries (the fp32 queries are what is read), 1 <= nq <= 256
 *   d_list    m row numbers (int64).  THE CALLER'S CONTRACT, not checked: strictly ascending, each in [0, n_rows).
 *             m == 0 is valid (d_list may then be NULL): every answer is padding
 *   k         1 <= k <= 8192; d_out_ids / d_out_scores [nq][k], (-1, -inf) beyond min(k, m) — metric "l2": (-1, +inf)
 *   l2, d_xn  l2 != 0: squared distances max(0, (|q|^2 + |x|^2) - 2 q.x) as rarc_search_wide_l2 forms them, d_xn = the rows'
 *             squared norms (rarc_row_sqnorms, fp32 [n_rows]); l2 == 0: d_xn is not read
 *   d_ws      rarc_search_rows_workspace_bytes(nq, k) bytes — each query's k best so far plus one slab of the list: it does
 *             not grow with m (0 = nq or k out of range)
 * A row fetched from HBM serves up to eight queries of the batch; one query (the reference's call) is a gather of m rows.
 *
 * rarc_strike_rows — the over-fetch way to the same answer: d_ids / d_scores [nq][kprime] is an ordinary answer (ids =
 * id_base + row, padding -1), d_bits a bitmask over the rows (uint32 [ceil(n_rows / 32)], bit r & 31 of word r >> 5).  Entries
 * whose row has no bit are struck, each query's first k survivors kept in order into d_out_ids / d_out_scores [nq][k]
 * (padding as above behind them), d_count[q] = survivors found (at most k).  A query with d_count[q] < min(k, allowed rows) did
 * not see all of its answer among the kprime: answer it with rarc_search_rows.
 */
size_t rarc_search_rows_workspace_bytes(int nq, int k);
int rarc_search_rows(const void* d_rows, int fmt, int64_t n_rows, int d_pad, const void* d_qblock, int nq, const int64_t* d_list,
                     int64_t m, int k, int64_t id_base, const float* d_xn, int l2, int64_t* d_out_ids, float* d_out_scores,
                     uint32_t* d_status, void* d_ws, size_t ws_bytes, void* stream);
int rarc_strike_rows(const int64_t* d_ids, const float* d_scores, int nq, int kprime, const uint32_t* d_bits, int64_t n_rows,
                     int64_t id_base, int k, int l2, int64_t* d_out_ids, float* d_out_scores, uint32_t* d_count, void* stream);

/*
 * The same two with the filter chosen PER QUERY: the queries of concurrent callers, each with a filter of its own, in one call
 * (FlatIndexF16.search_filtered_many).  Each query's answer is what rarc_search_rows / rarc_strike_rows give for its own list /
 * mask, bit for bit.
 *
 * rarc_search_rows_grouped — the queries arrive sorted by group (queries that share one list), cut into TILES:
 *   d_lists   the groups' lists, one behind the other (int64; each group's part strictly ascending, each entry in [0, n_rows):
 *             the caller's contract as above).  May be NULL when m_max == 0
 *   d_tiles   int64 [n_tiles][4] on the device = (first query, queries in the tile, offset of the group's list in d_lists, the
 *             list's length m_g).  A tile holds queries of ONE group, at most QT of them: QT = 1 for nq == 1, 4 for
 *             d_pad > 2048, else 8.  Every query of [0, nq) lies in exactly one tile; 1 <= n_tiles <= nq.  A group of more
 *             than QT queries is several tiles over the same list; m_g == 0 answers padding
 *   m_max     the largest m_g of the table (it decides how many slab rounds are launched)
 * Everything else — limits, metric "l2", d_status, the workspace (rarc_search_rows_grouped_workspace_bytes(nq, k) ==
 * rarc_search_rows_workspace_bytes(nq, k)) — as rarc_search_rows.  Launches per slab round: one score kernel over every
 * tile, one select for the queries whose list goes on; then one select for every answer.
 *
 * rarc_strike_rows_grouped — rarc_strike_rows with d_bits_off int64 [nq]: query q is struck against the mask that starts at word
 * d_bits_off[q] of d_bits (all masks of the call in one buffer, each uint32 [ceil(n_rows / 32)]); a negative entry keeps every
 * row (an unfiltered query in the same call).  One launch.
 */
size_t rarc_search_rows_grouped_workspace_bytes(int nq, int k);
int rarc_search_rows_grouped(const void* d_rows, int fmt, int64_t n_rows, int d_pad, const void* d_qblock, int nq,
                             const int64_t* d_lists, const int64_t* d_tiles, int n_tiles, int64_t m_max, int k, int64_t id_base,
                             const float* d_xn, int l2, int64_t* d_out_ids, float* d_out_scores, uint32_t* d_status, void* d_ws,
                             size_t ws_bytes, void* stream);
int rarc_strike_rows_grouped(const int64_t* d_ids, const float* d_scores, int nq, int kprime, const uint32_t* d_bits,
                             const int64_t* d_bits_off, int64_t n_rows, int64_t id_base, int k, int l2, int64_t* d_out_ids,
                             float* d_out_scores, uint32_t* d_count, void* stream);

/*
 * All pairs (i < j) of n embeddings whose cosine reaches a threshold — the entity de-duplication of the reference's graph
 * store (encapsulation/database/graph_db/Base_Neo4j.py:538-583: sklearn.metrics.pairwise.cosine_similarity over every entity
 * embedding, then a python loop over i < j keeping similarity >= 0.95); SURVEY 8(f) rank 4.  The n x n matrix is never
 * formed: the rows are normalised into an fp16 image, the score GEMM of rarc_search_wide (select in its epilogue) nominates
 * the pairs whose approximate cosine reaches threshold - eps (eps bounds the fp16 / fp32-accumulation error), and each
 * nominated pair is scored exactly (double-precision dot product of the fp32 rows, double-precision norms) and kept if that
 * reaches the threshold (csrc/pairs.hip).
 * d_rows: fp32 [n_rows][ld], device, any scale; 1 <= d <= 4096; 0 < threshold <= 1.
 * Output, in no particular order: d_out_pairs int64 [out_cap][2] = (i, j), d_out_scores double [out_cap];
 * *d_out_count (uint64) = how many pairs reached the threshold, also when that exceeds out_cap.
 * *d_flags (uint32): bit 0 = a column's nomination list (cand_cap entries) overflowed — call again with a larger cand_cap
 * (cand_cap >= n_rows cannot overflow); bit 1 = more pairs than out_cap — call again with out_cap >= *d_out_count.
 */
size_t rarc_similar_pairs_workspace_bytes(int64_t n_rows, int d, int cand_cap);
int rarc_similar_pairs(const float* d_rows, int64_t ld, int64_t n_rows, int d, double threshold, void* d_ws, size_t ws_bytes,
                       int cand_cap, int64_t* d_out_pairs, double* d_out_scores, int64_t out_cap,
                       unsigned long long* d_out_count, uint32_t* d_flags, void* stream);

/*
 * The exact k-nearest-neighbour graph of n embeddings: every row's top_k other rows by cosine — the event disambiguation of
 * the reference's graph store (encapsulation/database/graph_db/event_graphrag_neo4j.py:600-672, _disambiguate_events_with_gds:
 * gds.knn.write over every Event embedding with topK: 10, similarityCutoff: 0.85, one SIMILAR_TO edge per neighbour; it needs
 * a Neo4j server with the GDS plugin — the failure is swallowed when it is absent, :671-672 — and GDS's kNN is NN-descent:
 * approximate).  Here the answer is exact: the fp16 image and the score GEMM of rarc_similar_pairs nominate, per column (the
 * row whose neighbours are sought), what reaches a threshold that rises to (top_k-th best approximate score so far) - 2 eps
 * as chunks of rows go by; every nominee is then scored exactly and the top_k best kept (csrc/knn.hip).
 * d_rows: fp32 [n_rows][ld], device, any scale; 1 <= d <= 4096; 1 <= top_k <= 256; -1 <= cutoff <= 1.
 * Row i of the answer is the rows j != i (by index: an identical copy of row i is a neighbour) with cos(i, j) >= cutoff,
 * ordered by (cosine descending, j ascending), cut at top_k: d_out_ids int64 [n_rows][top_k], d_out_scores double
 * [n_rows][top_k] — the float64 cosine rarc_similar_pairs returns for the pair, bit for bit; a zero row has cosine 0 with
 * everything — d_out_count int32 [n_rows]; slots past the count hold (-1, -inf).
 * *d_flags (uint32): bit 0 = a column's nomination list (cand_cap entries) overflowed: the answer is incomplete — call again
 * with a larger cand_cap (cand_cap >= n_rows rounded up to 256 cannot overflow).
 * The workspace is rarc_knn_graph_workspace_bytes(n_rows, d, top_k, cand_cap) bytes (0 for arguments rarc_knn_graph refuses).
 */
size_t rarc_knn_graph_workspace_bytes(int64_t n_rows, int d, int top_k, int cand_cap);
int rarc_knn_graph(const float* d_rows, int64_t ld, int64_t n_rows, int d, int top_k, double cutoff, void* d_ws, size_t ws_bytes,
                   int cand_cap, int64_t* d_out_ids, double* d_out_scores, int32_t* d_out_count, uint32_t* d_flags, void* stream);

/*
 * Louvain communities of an undirected edge list — step 2 of the reference's entity de-duplication
 * (encapsulation/database/graph_db/Base_Neo4j.py:646-658: gds.louvain.stream(graph, {maxIterations: 10}) over the SIMILAR edges
 * rarc_similar_pairs finds), without a Neo4j server and its GDS plugin.  The algorithm is defined in integers (DESIGN 4.13c,
 * restated by tests/louvain_ref.py); the answer does not depend on the order of the edges or on thread timing (csrc/louvain.hip).
 * The loops over sweeps and levels are the caller's (graph_db/communities.py): three words are read per sweep, two per level.
 * Limits of every entry: 2 <= n < 2^31 - 1 vertices, 1 <= m < 2^30 edges (every product of the rule then fits int64).
 *
 * rarc_graph_csr — one level's graph in d_graph (rarc_graph_csr_workspace_bytes(n, m) bytes, 0 for a refused shape):
 *   d_pairs int64 [m][2], (i, j) with 0 <= i < j < n, each pair once (a pair outside that range is skipped);
 *   d_weights uint32 [m] or null (every weight 1); d_loops uint32 [n] or null (no self-loops).
 *   Adjacency in both directions (degree count, scan, fill: the order inside a row is arbitrary and nothing depends on it),
 *   weighted degrees, M2, and the vertices listed by degree class for the sweep.
 * rarc_louvain_init — slot 0 of d_state (rarc_louvain_workspace_bytes(n, m) bytes) becomes c(v) = v; d_out3 = {0, Qn, 0}.
 * rarc_louvain_sweep — sweep number `sweep` (>= 0: it selects the movers) reads slot `cur` (0 | 1) and writes the other one:
 *   labels, tot_C, sizes; d_out3 int64 [3] = {vertices moved, Qn of the new labelling, movers that had a target: moved, or held
 *   back by the singleton rule — a sweep without any is idle}.  The caller keeps the sweep by passing
 *   the other slot as `cur` next time and discards it by passing the same one.
 * rarc_louvain_aggregate — after a level: the communities of slot `cur` are renumbered 0 .. n_c - 1 in ascending label order,
 *   d_labels int64 [n0] (original vertex -> vertex of this level) is composed with that map in place, and the next level's
 *   input is written: d_out_pairs int64 [m][2], d_out_weights uint32 [m] (weight per community pair, arbitrary order),
 *   d_out_loops uint32 [n] (inside weight); d_out_counts int64 [2] = {n_c, m_c}.
 * rarc_louvain_labels — d_labels int64 [n0] of any labelling with values in [0, n0) -> the smallest member of each label's
 *   class, in place; d_ws: rarc_louvain_labels_workspace_bytes(n0) bytes.
 * rarc_louvain_limits — out4 = {largest degree of the 8-lane form, of the wave form, of the LDS-table form, LDS table slots};
 *   a vertex of a larger degree takes the global-memory table.
 */
size_t rarc_graph_csr_workspace_bytes(int64_t n, int64_t m);
int rarc_graph_csr(const int64_t* d_pairs, const uint32_t* d_weights, const uint32_t* d_loops, int64_t n, int64_t m, void* d_graph,
                   size_t graph_bytes, void* stream);
size_t rarc_louvain_workspace_bytes(int64_t n, int64_t m);
int rarc_louvain_init(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, void* d_state, size_t state_bytes, int64_t* d_out3,
                      void* stream);
int rarc_louvain_sweep(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, void* d_state, size_t state_bytes, int cur, int sweep,
                       int64_t* d_out3, void* stream);
int rarc_louvain_aggregate(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, void* d_state, size_t state_bytes, int cur,
                           int64_t* d_labels, int64_t n0, int64_t* d_out_pairs, uint32_t* d_out_weights, uint32_t* d_out_loops,
                           int64_t* d_out_counts, void* stream);
size_t rarc_louvain_labels_workspace_bytes(int64_t n0);
int rarc_louvain_labels(int64_t* d_labels, int64_t n0, void* d_ws, size_t ws_bytes, void* stream);
int rarc_louvain_limits(int* out4);

/*
 * Personalized PageRank over the graph rarc_graph_csr wrote, for a batch of nq queries at once — what a graph store is queried
 * with (gds.pageRank.stream(graph, {sourceNodes, dampingFactor: 0.85, maxIterations: 20}); HippoRAG-style retrievers run one
 * per query).  The rule is fixed point (restated by tests/ppr_ref.py): ONE = 2^40 units of mass, damping as
 * damping_q16 / 65536, every sum an integer sum — the same bits for any order of the edges, either form of the step and any
 * batch (csrc/ppr.hip).  The undirected graph's weights are uint32 >= 1 with a total below 2^31.
 * Limits of every entry: 2 <= n < 2^31 - 1, 1 <= m < 2^30 (as rarc_graph_csr), 1 <= nq <= 256; refused before any launch.
 * d_ws: rarc_ppr_workspace_bytes(n, m, nq) bytes (0 for a refused shape), 256-byte aligned: the state int64 [n][nq],
 * vertex-major (teleport, p, and p // W in two slots), and the per-query delta and done words.
 *
 * rarc_ppr_seed — d_seeds int64 [nq][n_slots] (a vertex, or -1 = unused; 1 <= n_slots <= 64; a vertex may repeat),
 *   d_seed_weights uint32 [nq][n_slots], each <= 2^20.  Writes the teleport vector t_q(v) = sum over q's slots naming v of
 *   (w << 40) // Wq (Wq = the sum of q's weights; Wq = 0: the query scores 0 everywhere), p_0 = t, slot 0, and clears delta / done.
 * rarc_ppr_step — one iteration p'(v) = ((65536 - a) t(v) + a flow(v)) >> 16, flow(v) = sum over neighbours u of
 *   w_uv (p(u) // W(u)) (an isolated v: flow(v) = p(v)), for every query not frozen; it reads slot `cur` (0 | 1; 0 after the seed)
 *   and writes the other: pass cur ^ 1 next time.  delta_q = max_v |p' - p|; a query with delta_q <= tolerance (in units of
 *   2^-40) is frozen: done_q = 1 and its column is not updated again.  d_done_out: uint32 [nq] that receives the done words,
 *   or null — a caller without a tolerance reads nothing between steps.
 *   Two forms, picked by nq: up to 32 queries the lanes of a wave share a vertex's neighbours (vertex-parallel), beyond that a
 *   lane is a query (query-parallel); a vertex of more than 64 neighbours is split across the waves of a workgroup in both.
 * rarc_ppr_scores — d_out_scores double [nq][n] = p / 2^40, exact.
 * rarc_ppr_topk — per query the top_k (1 .. 8192) vertices of positive score by (score descending, vertex ascending):
 *   d_out_ids int64 [nq][top_k], d_out_scores double [nq][top_k], d_out_count int32 [nq] = min(top_k, vertices with a positive
 *   score); slots past the count hold (-1, -inf).  The sort key carries the vertex in 24 bits: n >= 2^24 returns
 *   RARC_E_UNSUPPORTED (rarc_ppr_scores has no such limit).  `cur` as rarc_ppr_step would get it next: the keys are built in
 *   the slot that step would overwrite, so stepping may go on afterwards.
 * rarc_ppr_limits — out6 = {largest degree a single wave walks (a larger one is split), largest nq of the vertex-parallel form,
 *   largest nq, largest n_slots, largest top_k, bits of a vertex in the top-k key}.
 */
size_t rarc_ppr_workspace_bytes(int64_t n, int64_t m, int nq);
int rarc_ppr_seed(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, const int64_t* d_seeds, const uint32_t* d_seed_weights,
                  int nq, int n_slots, void* d_ws, size_t ws_bytes, void* stream);
int rarc_ppr_step(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, int nq, int damping_q16, int64_t tolerance, int cur,
                  void* d_ws, size_t ws_bytes, uint32_t* d_done_out, void* stream);
int rarc_ppr_scores(int64_t n, int64_t m, int nq, const void* d_ws, size_t ws_bytes, double* d_out_scores, void* stream);
int rarc_ppr_topk(int64_t n, int64_t m, int nq, int top_k, int cur, void* d_ws, size_t ws_bytes, int64_t* d_out_ids,
                  double* d_out_scores, int32_t* d_out_count, void* stream);
int rarc_ppr_limits(int* out6);

/*
 * Passage retrieval from the PPR state: the mass of the entities pushed through the mention links (chunk)-[:MENTIONS]->(entity)
 * onto the chunks, and the chunks ranked — how a PPR-based graph retriever (HippoRAG's, upstream RAG-ARC's) ends.  The rule
 * continues the one above (restated by tests/passage_ref.py): a mention map is a set of triples (c, e, w),
 * 0 <= c < n_chunks, 0 <= e < n, w an integer in [1, 2^12), every (c, e) once, given as a CSR by chunk: d_row_ptr int64
 * [n_chunks + 1], d_ent int32 [nnz], d_w uint32 [nnz].  With p_q the state of query q,
 *   S_q(c) = (sum over c's mentions (e, w) of w * p_q(e)) >> 12 < 2^40,   score = S / 2^28 (exact)
 * — integer sums: the same bits for any order of the mentions, either form of the kernel and any batch.
 * Limits: n, m, nq as above, 1 <= n_chunks < 2^31 - 1, nnz >= 1, d_ws and d_cws 256-byte aligned, every array aligned to its
 * element; refused before any launch.  The host entry cannot read the device arrays, so the kernel guards itself: a chunk's
 * range [row_ptr[c], row_ptr[c + 1]) is clamped to [0, nnz], an entry with e outside [0, n) or w outside [1, 2^12)
 * contributes nothing, a listed chunk outside [0, n_chunks) is skipped — no index leaves its buffer, whatever they hold.
 * d_cws: rarc_ppr_chunks_workspace_bytes(n_chunks, nq) bytes (0 for a refused shape): S, the top-k keys and the counts.
 *
 * rarc_ppr_chunks — reads p of the PPR workspace d_ws (`cur` as rarc_ppr_step would get it next; the workspace is only read,
 *   so stepping may go on) and writes S as int64 [n_chunks][nq], chunk-major, into d_cws.  d_split int32 [n_split]: the chunks
 *   of more than 64 mentions (rarc_ppr_chunks_limits), each split across the waves of a workgroup; may be null when n_split = 0.
 *   A chunk of more than 64 mentions that the list omits scores 0.  Two forms by nq, as rarc_ppr_step.
 * rarc_ppr_chunks_scores — d_out_scores double [nq][n_chunks] = S / 2^28.
 * rarc_ppr_chunks_topk — per query the top_k (1 .. 8192) chunks of positive score by (score descending, chunk ascending):
 *   ids int64 [nq][top_k], scores double [nq][top_k], count int32 [nq]; (-1, -inf) past the count.  n_chunks >= 2^24 returns
 *   RARC_E_UNSUPPORTED (the key carries the chunk in 24 bits; rarc_ppr_chunks_scores has no such limit).
 * rarc_ppr_chunks_limits — out4 = {most mentions a single wave walks (a chunk of more is split), bits of a mention weight,
 *   the shift of a score (S / 2^28), bits of a chunk in the top-k key}.
 */
size_t rarc_ppr_chunks_workspace_bytes(int64_t n_chunks, int nq);
int rarc_ppr_chunks(int64_t n, int64_t m, int nq, int cur, const void* d_ws, size_t ws_bytes, const int64_t* d_row_ptr,
                    const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz, const int32_t* d_split, int64_t n_split,
                    void* d_cws, size_t cws_bytes, void* stream);
int rarc_ppr_chunks_scores(int64_t n_chunks, int nq, const void* d_cws, size_t cws_bytes, double* d_out_scores, void* stream);
int rarc_ppr_chunks_topk(int64_t n_chunks, int nq, int top_k, void* d_cws, size_t cws_bytes, int64_t* d_out_ids, double* d_out_scores,
                         int32_t* d_out_count, void* stream);
int rarc_ppr_chunks_limits(int* out4);

/*
 * k-hop neighbourhoods over the graph rarc_graph_csr wrote, for a batch of nq queries at once: which vertices lie within
 * `hops` edges of a query's seeds, and how far each is — MATCH (s)-[*..h]-(v), as one bit-parallel multi-source breadth-first
 * search.  The rule (restated by tests/khop_ref.py): edge weights are ignored; hop_q(v) is the fewest edges from
 * any seed of q to v, a seed has hop 0, v is in q's neighbourhood iff hop_q(v) <= hops.  The state is one bit per (vertex,
 * query, level), ceil(nq / 64) 64-bit words per vertex and level; every join is an OR or an integer sum — the same bits for
 * any order of the edges and any batch, and row q of a batch equals the one-query call (csrc/khop.hip).
 * Limits of every entry: 2 <= n < 2^31 - 1, 1 <= m < 2^30 (as rarc_graph_csr), 1 <= nq <= 256, 0 <= hops <= 8 (hops > 8:
 * RARC_E_UNSUPPORTED); pointers aligned to their element, workspaces to 256 bytes; refused before any launch.
 * d_ws: rarc_khop_workspace_bytes(n, m, nq, hops) bytes (0 for a refused shape); every entry of one search takes the same
 * n, m, nq and hops.
 *
 * rarc_khop_seed — d_seeds int64 [nq][n_slots] (a vertex, or -1 = unused; 1 <= n_slots <= 64; a vertex may repeat, a row may
 *   be empty; a vertex outside [0, n) is skipped).  Clears the state and writes level 0.
 * rarc_khop_step — level `hop` (1 <= hop <= hops) becomes the neighbours of level hop - 1 that no earlier level holds; call it
 *   once per hop, in order, after the seed.  d_grew_out: a uint32 that receives 1 if any query reached a new vertex, else 0,
 *   or null.  Once it is 0 every later level is empty, and the remaining steps may be left out: the answer is the same.
 *   A vertex of more than 64 neighbours (rarc_khop_limits) is split across the threads of a workgroup.
 * rarc_khop_counts — d_out_counts int32 [nq][hops + 1]: the vertices at hop h exactly; never capped.
 * rarc_khop_levels — d_out_levels uint8 [nq][n]: hop_q(v), or 255 for "not within hops".
 * rarc_khop_list — per query the neighbourhood by (hop ascending, vertex ascending), its first min(size, max_vertices) entries
 *   (1 <= max_vertices <= 65536; more: RARC_E_UNSUPPORTED): d_out_ids int64 [nq][max_vertices], d_out_hops int32
 *   [nq][max_vertices], d_out_count int32 [nq]; slots past the count hold (-1, -1).
 * rarc_khop_chunks — the neighbourhood pushed through a mention map (the CSR and the split list exactly as rarc_ppr_chunks
 *   takes them, guarded the same way): S_q(c) = sum over c's mentions (e, w) with hop_q(e) <= hops of w * decay[hop_q(e)],
 *   written as int64 [n_chunks][nq] into d_cws (rarc_ppr_chunks_workspace_bytes), where rarc_ppr_chunks_scores and
 *   rarc_ppr_chunks_topk read it unchanged (score S / 2^28).  `decay`: a HOST array uint32 [hops + 1], every entry in
 *   [0, 2^16]; with the mention weights of a chunk adding up to less than 2^12, S < 2^28.
 * rarc_khop_limits — out5 = {largest hops, largest nq, largest n_slots, largest max_vertices, largest degree walked without a
 *   split}.
 */
size_t rarc_khop_workspace_bytes(int64_t n, int64_t m, int nq, int hops);
int rarc_khop_seed(int64_t n, int64_t m, const int64_t* d_seeds, int nq, int n_slots, int hops, void* d_ws, size_t ws_bytes, void* stream);
int rarc_khop_step(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, int nq, int hops, int hop, void* d_ws, size_t ws_bytes,
                   uint32_t* d_grew_out, void* stream);
int rarc_khop_counts(int64_t n, int64_t m, int nq, int hops, void* d_ws, size_t ws_bytes, int32_t* d_out_counts, void* stream);
int rarc_khop_levels(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, uint8_t* d_out_levels, void* stream);
int rarc_khop_list(int64_t n, int64_t m, int nq, int hops, int max_vertices, void* d_ws, size_t ws_bytes, int64_t* d_out_ids,
                   int32_t* d_out_hops, int32_t* d_out_count, void* stream);
int rarc_khop_chunks(int64_t n, int64_t m, int nq, int hops, const uint32_t* decay, const void* d_ws, size_t ws_bytes,
                     const int64_t* d_row_ptr, const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz,
                     const int32_t* d_split, int64_t n_split, void* d_cws, size_t cws_bytes, void* stream);
int rarc_khop_limits(int* out5);

/*
 * k-hop subgraphs: the relations inside each query's neighbourhood — MATCH (a)-[r]-(b) WHERE a, b IN nodes — from the state
 * rarc_khop_seed and rarc_khop_step left in d_ws, which is only read: the other k-hop answers follow from the same traversal.
 * The rule (restated by tests/subgraph_ref.py): d_rel is the CALLER's relation table, int64 [r][2] rows (a, b) in
 * any orientation; a pair may repeat and a may equal b.  Row e has level max(hop_q(a), hop_q(b)) and belongs to q's subgraph iff
 * that is <= hops; a row with an end outside [0, n) belongs to none.  The graph's CSR is not read, and the table enters only
 * through its row numbers, which are what the answer holds.  n, m, nq, hops, d_ws: as the traversal's, refused the same way.
 * Limits: 1 <= r < 2^31 - 1; 1 <= max_edges <= 65536 (more: RARC_E_UNSUPPORTED); d_rel and the ids 8-byte aligned, the other
 * outputs 4, the workspaces 256; refused before any launch.
 *
 * rarc_khop_edges_workspace_bytes — the size of d_ews, the tile counts of the rows (0 for a refused shape); the k-hop
 *   workspace and its size do not change.
 * rarc_khop_edges — d_out_level_counts int32 [nq][hops + 1]: the rows at level h exactly, never capped.  Per query the rows by
 *   (level ascending, row ascending), the first min(size, max_edges) of them: d_out_ids int64 [nq][max_edges] (row numbers of
 *   d_rel), d_out_levels int32 [nq][max_edges], d_out_count int32 [nq]; slots past the count hold (-1, -1).  d_out_ids,
 *   d_out_levels and d_out_count may be null together: then only the level counts are written (no list is placed).
 * rarc_khop_edges_limits — out2 = {largest max_edges, rows per tile of the count / scan / write passes}.
 */
size_t rarc_khop_edges_workspace_bytes(int64_t r, int nq, int hops);
int rarc_khop_edges(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, const int64_t* d_rel, int64_t r, int max_edges,
                    void* d_ews, size_t ews_bytes, int64_t* d_out_ids, int32_t* d_out_levels, int32_t* d_out_count,
                    int32_t* d_out_level_counts, void* stream);
int rarc_khop_edges_limits(int* out2);

/*
 * Connecting paths: how the sources of one traversal are joined — MATCH p = allShortestPaths((a)-[*..L]-(b)) — from the state
 * rarc_khop_seed and rarc_khop_step left in d_ws for ns sources stepped to hops = max_length, which is only read.  The rule
 * (restated by tests/paths_ref.py): a source is a seed set as rarc_khop_seed takes it; for a pair p = (ia, ib) of
 * source indices d_p = min over v of hop_ia(v) + hop_ib(v), and -1 where no vertex gives a value <= max_length or an index lies
 * outside [0, ns); v is on p's paths at position i iff hop_ia(v) == i and hop_ib(v) == d_p - i.  ia == ib is allowed and a pair
 * may repeat.  Every join is an AND, an OR, an integer min or count: the same bits for any order of the edges and any batch, and
 * row p of a batch equals the one-pair call (csrc/khop.hip).
 * Limits: n, m as the traversal's, 1 <= ns <= 256, 1 <= np <= 256, 0 <= max_length <= 8 (more: RARC_E_UNSUPPORTED); d_pairs and
 * the distances 4-byte aligned, the workspaces 256; refused before any launch.
 *
 * rarc_khop_paths — d_pairs int32 [np][2] on the device; d_out_dist int32 [np] receives d_p.  d_pws, of
 *   rarc_khop_workspace_bytes(n, m, np, max_length) bytes, becomes a k-hop state of np columns whose level i holds the vertices
 *   at position i: rarc_khop_counts, rarc_khop_levels, rarc_khop_list and rarc_khop_chunks read it with nq = np and
 *   hops = max_length, positions in the place of hops.
 * rarc_khop_path_edges — the arguments, outputs and limits of rarc_khop_edges, d_ws being the PATH state and nq = np: a row
 *   (a, b) of d_rel is at level i + 1 iff one end is on the pair's paths at position i and the other at position i + 1.  A row
 *   between two vertices of one position, a row with a == b and a row with an end outside [0, n) are at no level; level 0 is
 *   empty.  The table is trusted as it is for subgraphs: the CSR is not read.  d_ews: rarc_khop_edges_workspace_bytes(r, np,
 *   max_length) bytes.
 * rarc_khop_paths_limits — out3 = {largest max_length, largest ns, largest np}.
 */
int rarc_khop_paths(int64_t n, int64_t m, int ns, int np, int max_length, const void* d_ws, size_t ws_bytes, const int32_t* d_pairs,
                    void* d_pws, size_t pws_bytes, int32_t* d_out_dist, void* stream);
int rarc_khop_path_edges(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, const int64_t* d_rel, int64_t r,
                         int max_edges, void* d_ews, size_t ews_bytes, int64_t* d_out_ids, int32_t* d_out_levels, int32_t* d_out_count,
                         int32_t* d_out_level_counts, void* stream);
int rarc_khop_paths_limits(int* out3);

/*
 * Typed traversal: MATCH (s)-[:CAUSAL|SEQUENTIAL*..h]-(v) — k-hop over the relation types each query allows, still one launch
 * for a batch of mixed filters.  The rule (restated by tests/typed_ref.py): a type is an integer in [0, 32); an
 * undirected pair carries a uint32 mask, the OR of 1 << t over the relations that join it; query q carries a uint32 filter F_q
 * and may cross a pair iff mask & F_q != 0 (a pair of mask 0 is crossed by nobody); hop_q(v) is the fewest crossable edges from
 * any seed of q to v and a seed has hop 0 whatever its filter.  The state is the one rarc_khop_seed starts and every k-hop reader
 * takes: rarc_khop_counts, _levels, _list, _chunks, _paths read a typed traversal unchanged.  Every join is an AND or an OR: the
 * same bits for any order of the pairs and any batch.
 *
 * rarc_graph_types — the typed adjacency of a graph rarc_graph_csr built, in d_out (rarc_graph_types_workspace_bytes(n, m)
 *   bytes, 0 for a refused shape): t_adj int32 [2m] | t_mask uint32 [2m] | cursor uint32 [n] | bad u32, slot arrays of their own
 *   over the blob's row_ptr (the slot order of the blob's adj is not reproducible, so nothing can be aligned to it).  d_pairs is
 *   THE pair list the graph was built from, d_masks uint32 [m] beside it; a pair rarc_graph_csr skipped is skipped.  A pair that
 *   finds a row full is not written and counted: the entry waits for the stream and returns RARC_E_INVALID if there was one.
 * rarc_khop_step_typed — rarc_khop_step under d_filters uint32 [nq] on the device, over d_types; the same `grew` word.
 * rarc_khop_edges_typed, rarc_khop_path_edges_typed — rarc_khop_edges and rarc_khop_path_edges for a typed table: d_rel_types
 *   int32 [r] holds a type id per row (one outside [0, 32) is in no answer) or, with rel_masks = 1, the row's uint32 mask; row e
 *   is listed for q only if F_q holds its type (its mask & F_q != 0).  For paths the caller repeats the one filter per pair.
 * Limits and alignment as the untyped entries'; d_types 256-byte aligned, filters, masks and row types 4; refused before any
 * launch.
 */
size_t rarc_graph_types_workspace_bytes(int64_t n, int64_t m);
int rarc_graph_types(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, const int64_t* d_pairs, const uint32_t* d_masks,
                     void* d_out, size_t out_bytes, void* stream);
int rarc_khop_step_typed(const void* d_graph, size_t graph_bytes, const void* d_types, size_t types_bytes, const uint32_t* d_filters,
                         int64_t n, int64_t m, int nq, int hops, int hop, void* d_ws, size_t ws_bytes, uint32_t* d_grew_out, void* stream);
int rarc_khop_edges_typed(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, const int64_t* d_rel, int64_t r,
                          const int32_t* d_rel_types, int rel_masks, const uint32_t* d_filters, int max_edges, void* d_ews, size_t ews_bytes,
                          int64_t* d_out_ids, int32_t* d_out_levels, int32_t* d_out_count, int32_t* d_out_level_counts, void* stream);
int rarc_khop_path_edges_typed(int64_t n, int64_t m, int nq, int hops, const void* d_ws, size_t ws_bytes, const int64_t* d_rel, int64_t r,
                               const int32_t* d_rel_types, int rel_masks, const uint32_t* d_filters, int max_edges, void* d_ews,
                               size_t ews_bytes, int64_t* d_out_ids, int32_t* d_out_levels, int32_t* d_out_count,
                               int32_t* d_out_level_counts, void* stream);

/*
 * Typed personalized PageRank: gds.pageRank.stream over a relationship-filtered projection, one launch group for a batch of
 * mixed filters.  The rule (restated by tests/typed_ppr_ref.py): for query q with filter F_q it is the rule of
 * rarc_ppr_step on the graph whose edges are those with mask & F_q != 0, each at its full weight — W_q(u) = the sum of the
 * weights of u's allowed edges, c(u) = p(u) // W_q(u), flow(v) = the sum over v's allowed edges of w_uv c(u), flow(v) = p(v) where
 * W_q(v) = 0 (a vertex isolated under the filter keeps its mass); p', delta_q, freezing, scores and ranking as untyped.  Row q of
 * any batch is the one-query answer on the filtered edge list, bit for bit, for any order of the pairs and of the queries; an
 * all-ones filter over non-zero masks is the untyped call; filter 0 crosses nothing: p = t, delta = 0.  A pair's mask is the
 * OR and its weight the sum over its duplicates, so a pair of types {0, 1} is crossed at its whole weight under filter {0}:
 * per-type weights are not kept.
 *
 * rarc_graph_types_weighted — rarc_graph_types with a weight plane: d_out (rarc_graph_types_weighted_workspace_bytes(n, m) bytes,
 *   0 for a refused shape) receives what rarc_graph_types writes, byte for byte at the same offsets, followed by t_w uint32 [2m],
 *   the weight of each slot.  d_weights uint32 [m] beside the pairs — THE weights the graph was built with — or null = all 1.
 *   The first rarc_graph_types_workspace_bytes(n, m) bytes are a valid d_types of the typed k-hop entries: a graph keeps one copy.
 * rarc_ppr_seed_typed — rarc_ppr_seed with c_0(v) = t_q(v) // W_q(v), under d_filters uint32 [nq] on the device.
 * rarc_ppr_step_typed — rarc_ppr_step under d_filters: the same workspace, slots, forms and launches over the same degree lists
 *   (by total degree); per slot it reads neighbour, mask and weight from d_types.  rarc_ppr_scores, rarc_ppr_topk and
 *   rarc_ppr_chunks* read the state unchanged.
 * Limits as the untyped entries'; d_types 256-byte aligned and of exactly the weighted size (the unweighted blob has no weight
 * plane: RARC_E_WORKSPACE), d_filters 4-byte aligned; refused before any launch.
 */
size_t rarc_graph_types_weighted_workspace_bytes(int64_t n, int64_t m);
int rarc_graph_types_weighted(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, const int64_t* d_pairs, const uint32_t* d_masks,
                              const uint32_t* d_weights, void* d_out, size_t out_bytes, void* stream);
int rarc_ppr_seed_typed(const void* d_graph, size_t graph_bytes, const void* d_types, size_t types_bytes, const uint32_t* d_filters, int64_t n,
                        int64_t m, const int64_t* d_seeds, const uint32_t* d_seed_weights, int nq, int n_slots, void* d_ws, size_t ws_bytes,
                        void* stream);
int rarc_ppr_step_typed(const void* d_graph, size_t graph_bytes, const void* d_types, size_t types_bytes, const uint32_t* d_filters, int64_t n,
                        int64_t m, int nq, int damping_q16, int64_t tolerance, int cur, void* d_ws, size_t ws_bytes, uint32_t* d_done_out,
                        void* stream);

/*
 * Entity merging: step 4 of the reference's de-duplication (Base_Neo4j.py:714-890, _merge_clusters) — every class of a labelling
 * becomes one entity, and the pair list, the mention CSR and the relation table are contracted onto the survivors without
 * leaving the device.  The rule (restated by tests/merge_ref.py) is in integers; every result is the same bits for
 * any order of the pairs and mentions, and from run to run (csrc/merge.hip).  Pointers aligned to their element, workspaces to
 * 256 bytes, each *_workspace_bytes returning 0 for a refused shape; everything is refused before any launch.
 *
 * rarc_sort_reduce — np.unique + bincount: d_keys uint64 [count], of which only the low key_bits bits are used (a higher bit must
 *   be 0); d_values uint32 [count], or null = every value is 1.  1 <= key_bits <= 62, 1 <= count < 2^31.  d_out_keys uint64
 *   [count]: the distinct keys ascending; d_out_sums uint64 [count]: the sum of the values of each (64 bits: nothing wraps);
 *   d_out2 int64 [2] = {distinct keys, largest sum}; slots past the distinct keys are unspecified.  An LSD radix sort over
 *   ceil(key_bits / 8) passes, stable, then a segmented sum.  The inputs are only read.
 * rarc_sort_reduce_limits — out4 = {keys per tile, bits per pass, largest key_bits, log2 of the count limit}.
 * rarc_merge_plan — d_labels int64 [n]: any labelling with values in [0, n) (a label outside makes its vertex a class of its own);
 *   d_richness uint32 [n] or null (all 0).  1 <= n < 2^31 - 1.  The primary of a class is its member of largest richness, among
 *   equals the smallest index; the primaries are numbered 0 .. n_c - 1 in ascending index.  d_primary int64 [n]: old -> its
 *   primary; d_new_id int64 [n]: old -> new; d_kept int64 [n]: its first n_c entries are new -> old; d_removed int64 [n]: its
 *   first n - n_c entries are the others, ascending; d_out_count int64 [1] = n_c.
 * rarc_merge_pairs — d_pairs int64 [m][2], d_weights uint32 [m] or null (unit), 1 <= m < 2^31; d_new_id int64 [n] as the plan
 *   wrote it.  Both ends are mapped; a pair whose ends land on one entity is left out and counted; the others become (min, max),
 *   equal pairs merge, their weights add.  d_out_pairs int64 [m][2] by (i, j) ascending, d_out_weights uint32 [m] (the low 32
 *   bits of each sum: the largest sum is reported); d_out5 int64 [5] = {pairs written, largest summed weight, pairs left out,
 *   their total weight, pairs skipped for an end outside [0, n)}.
 * rarc_merge_mentions — the CSR by chunk exactly as rarc_ppr_chunks takes it (guarded the same way: ranges clamped to [0, nnz], an
 *   entity outside [0, n) or a weight of 0 skipped and counted), 1 <= n_chunks < 2^31 - 1, 1 <= nnz < 2^31.  Entities are mapped,
 *   equal (chunk, entity) merge, their weights add.  d_out_row_ptr int64 [n_chunks + 1], d_out_ent int32 [nnz] (each row by
 *   entity ascending), d_out_w uint32 [nnz], d_out_split int32 [n_chunks]: the chunks of more than 64 mentions
 *   (rarc_ppr_chunks_limits), ascending; d_out6 int64 [6] = {mentions written, largest summed weight, 0, 0, mentions skipped,
 *   chunks in the split list}.  A largest weight >= 2^12 is the caller's to refuse before it uses the result.
 * rarc_merge_relations — d_rel int64 [r][2] as rarc_khop_edges takes it, 1 <= r < 2^31 - 1.  Rows keep their identity and order:
 *   a row is left out iff its ends were DIFFERENT entities that land on ONE (a == b stays), or an end lies outside [0, n).
 *   d_out_rel int64 [r][2]: the mapped ends of the rows that stay; d_out_rows int64 [r]: the old row of each; d_out3 int64 [3] =
 *   {rows written, rows left out as internal, rows left out for an end out of range}.
 */
size_t rarc_sort_reduce_workspace_bytes(int64_t count);
int rarc_sort_reduce(const uint64_t* d_keys, const uint32_t* d_values, int64_t count, int key_bits, void* d_ws, size_t ws_bytes,
                     uint64_t* d_out_keys, uint64_t* d_out_sums, int64_t* d_out2, void* stream);
int rarc_sort_reduce_limits(int* out4);
size_t rarc_merge_plan_workspace_bytes(int64_t n);
int rarc_merge_plan(const int64_t* d_labels, const uint32_t* d_richness, int64_t n, void* d_ws, size_t ws_bytes, int64_t* d_primary,
                    int64_t* d_new_id, int64_t* d_kept, int64_t* d_removed, int64_t* d_out_count, void* stream);
size_t rarc_merge_pairs_workspace_bytes(int64_t m);
int rarc_merge_pairs(const int64_t* d_pairs, const uint32_t* d_weights, int64_t m, const int64_t* d_new_id, int64_t n, void* d_ws,
                     size_t ws_bytes, int64_t* d_out_pairs, uint32_t* d_out_weights, int64_t* d_out5, void* stream);
size_t rarc_merge_mentions_workspace_bytes(int64_t n_chunks, int64_t nnz);
int rarc_merge_mentions(const int64_t* d_row_ptr, const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz,
                        const int64_t* d_new_id, int64_t n, void* d_ws, size_t ws_bytes, int64_t* d_out_row_ptr, int32_t* d_out_ent,
                        uint32_t* d_out_w, int32_t* d_out_split, int64_t* d_out6, void* stream);
size_t rarc_merge_relations_workspace_bytes(int64_t r);
int rarc_merge_relations(const int64_t* d_rel, int64_t r, const int64_t* d_new_id, int64_t n, void* d_ws, size_t ws_bytes,
                         int64_t* d_out_rel, int64_t* d_out_rows, int64_t* d_out3, void* stream);

/*
 * Graph ingest: what the reference's store_graph(documents) does per batch of documents (event_graphrag_neo4j.py: _store_mentions,
 * _store_entity_relations, _create_chunk_entity_relations MERGE into what is there) — raw extraction rows, in any orientation, with
 * duplicates, typed and weighted, become the unique sorted lists EntityGraph.from_device and MentionMap.from_device_csr adopt, and
 * a resident list is extended by a batch, without the rows or the list crossing to the host.  The rule (restated by
 * tests/ingest_ref.py) is in integers: the same bytes for any order of the rows and from run to run (csrc/merge.hip: one key per
 * row, rarc_sort_reduce's sort and segmented sum, a writer).  Pointers aligned to their element, workspaces to 256 bytes, each
 * *_workspace_bytes returning 0 for a refused shape; everything is refused before any launch; launches only — the caller reads the
 * count words back.  0 <= base count, 0 <= r, 1 <= base count + r < 2^31 (rarc_sort_reduce's count limit); a side of length 0 may
 * pass null pointers.
 *
 * rarc_ingest_pairs — d_rows int64 [r][2] in any orientation; d_row_weights uint32 [r] or null (1 each); d_row_types int32 [r] or
 *   null.  The base: d_base_pairs int64 [m0][2], unique pairs i < j in ANY order (what an EntityGraph keeps), d_base_weights uint32
 *   [m0] or null (1 each), d_base_masks uint32 [m0] or null.  2 <= n < 2^31 - 1 as rarc_graph_csr takes it.  Typed iff d_out_masks
 *   is given: then every side present must carry its types / masks, else none may (RARC_E_INVALID).  A new row is skipped and
 *   counted under the first that applies of {an end outside [0, n), a == b, weight 0, a type outside [0, 32)}; a base row outside
 *   its contract (i >= j, out of range, weight 0) is skipped and counted apart.  Every other row gives its weight to the pair
 *   (min, max) and its mask — 1 << type, a base row's whole mask — to the pair's mask: W = the 64-bit sum, mask = the OR.  Unit
 *   mode, when neither side has weights: every W is 1.  d_out_pairs int64 [m0 + r][2] by (i, j) ascending; d_out_weights uint32
 *   [m0 + r] (the low 32 bits of W; may be null in unit mode, else written as 1); d_out_masks uint32 [m0 + r] or null; d_out8 int64
 *   [8] = {edges, largest W, total W, rows skipped out of range, as self-loops, for weight 0, for a bad type, base rows skipped}.
 *   No slot at or past `edges` is written.  A largest W >= 2^32 or a total >= 2^31 is the caller's to refuse.
 * rarc_ingest_mentions — d_rows int64 [r][2] of (chunk, entity); d_row_weights uint32 [r] or null (1 each).  The base: the CSR by
 *   chunk of a mention map over base_chunks <= n_chunks chunks and nnz0 entries, as rarc_ppr_chunks takes it (ranges clamped to
 *   [0, nnz0]; an entry with an entity outside [0, n_entities) or a weight outside [1, 2^12) skipped and counted apart).  1 <=
 *   n_chunks < 2^31 - 1, 1 <= n_entities < 2^31 - 1.  A new row is skipped and counted under the first that applies of {a chunk
 *   outside [0, n_chunks), an entity outside [0, n_entities), a weight outside [1, 2^12)}.  W(c, e) = the sum of the weights.  The
 *   output is rarc_merge_mentions': d_out_row_ptr int64 [n_chunks + 1], d_out_ent int32 [nnz0 + r] (each row ascending, no
 *   repeats), d_out_w uint32 [nnz0 + r], d_out_split int32 [n_chunks]: the chunks of more than 64 mentions, ascending; d_out8 int64
 *   [8] = {mentions written, largest W, chunks in the split list, rows skipped for the chunk, for the entity, for the weight, 0,
 *   base entries skipped}.  A largest W >= 2^12 is the caller's to refuse before it uses the result.
 * rarc_ingest_limits — out4 = {relation types of a mask, bits of a mention weight, the split degree, log2 of the count limit}.
 */
size_t rarc_ingest_pairs_workspace_bytes(int64_t m0, int64_t r);
int rarc_ingest_pairs(const int64_t* d_rows, const uint32_t* d_row_weights, const int32_t* d_row_types, int64_t r,
                      const int64_t* d_base_pairs, const uint32_t* d_base_weights, const uint32_t* d_base_masks, int64_t m0, int64_t n,
                      void* d_ws, size_t ws_bytes, int64_t* d_out_pairs, uint32_t* d_out_weights, uint32_t* d_out_masks, int64_t* d_out8,
                      void* stream);
size_t rarc_ingest_mentions_workspace_bytes(int64_t n_chunks, int64_t nnz0, int64_t r);
int rarc_ingest_mentions(const int64_t* d_rows, const uint32_t* d_row_weights, int64_t r, const int64_t* d_base_row_ptr,
                         const int32_t* d_base_ent, const uint32_t* d_base_w, int64_t base_chunks, int64_t nnz0, int64_t n_chunks,
                         int64_t n_entities, void* d_ws, size_t ws_bytes, int64_t* d_out_row_ptr, int32_t* d_out_ent, uint32_t* d_out_w,
                         int32_t* d_out_split, int64_t* d_out8, void* stream);
int rarc_ingest_limits(int* out4);

/*
 * Connected components: which vertices of the graph rarc_graph_csr built are joined at all, how many pieces it has and how large
 * they are — CALL gds.wcc.stream(graph) — next to the resident CSR.  The rule (restated by
 * tests/components_ref.py): a parent word p[v] per vertex, p[v] = v at first.  A round starts from a star forest and hooks — for
 * every adjacency entry (u, v), with ru = p[u] and rv = p[v] as they stood at the start of the round and rv < ru, p[ru] =
 * min(p[ru], rv) — and then jumps: every vertex follows p to its root and stores it.  The first round whose hooks lower no
 * parent ends the run; label(v) = p[v] is then the smallest vertex of v's component (the convention of rarc_louvain_labels).
 * Every join is an integer min over a set: the state after every round, and so the number of rounds, is the same for any order
 * of the edges and from run to run; no graph takes more than 2 ceil(log2 n) + 2 rounds (csrc/components.hip).
 * Limits: n, m as rarc_graph_csr's; the workspace and the graph 256-byte aligned, the other pointers to their element; refused
 * before any launch.
 *
 * rarc_components_workspace_bytes — the size of d_ws (0 for a refused shape); every entry of one run takes the same n, m, d_ws.
 * rarc_components_init — p[v] = v.
 * rarc_components_round — one hook and one jump over the CSR in d_graph.  d_changed int32 [1] on the device: 1 if a hook lowered
 *   a parent, else 0 — then the labels are final and a further round changes nothing.  The loop is the caller's, one word a
 *   round.  A vertex of at most 8 neighbours takes 8 lanes, one of at most 64 a quarter wave, a larger one a workgroup
 *   (rarc_components_limits); a vertex issues one atomic min.
 * rarc_components_finish — d_labels int64 [n] = p; d_dense int32 [n] or null: the rank of label(v) among the distinct labels,
 *   ascending; d_sizes int64 [n] or null: its first n_components entries are the sizes by dense id; d_out3 int64 [3] =
 *   {n_components, size of the largest component, its label — among equals the smallest}.  Reads the state as it is: before the
 *   run has ended the labels are those of the forest so far.
 * rarc_components_limits — out4 = {largest degree of the 8-lane form, of the quarter-wave form, of the first workgroup list, the
 *   additive constant of the round bound}.
 */
size_t rarc_components_workspace_bytes(int64_t n, int64_t m);
int rarc_components_init(int64_t n, int64_t m, void* d_ws, size_t ws_bytes, void* stream);
int rarc_components_round(const void* d_graph, size_t graph_bytes, int64_t n, int64_t m, void* d_ws, size_t ws_bytes, int32_t* d_changed,
                          void* stream);
int rarc_components_finish(int64_t n, int64_t m, void* d_ws, size_t ws_bytes, int64_t* d_labels, int32_t* d_dense, int64_t* d_sizes,
                           int64_t* d_out3, void* stream);
int rarc_components_limits(int* out4);

/*
 * Co-occurrence projection: the entity graph a mention map implies — two entities are joined when a chunk mentions both, weighted
 * by how many chunks do: MATCH (a)<-[:MENTIONS]-(c)-[:MENTIONS]->(b) WHERE id(a) < id(b) RETURN a, b, count(c) — next to the
 * resident CSR, without an edge list crossing to the host.  The rule (restated by tests/cooccur_ref.py) is in
 * integers.  The CSR by chunk is taken exactly as rarc_ppr_chunks and rarc_merge_mentions take it, guarded the same way: ranges
 * clamped to [0, nnz], an entry with an entity outside [0, n) or a weight outside [1, 2^12) skipped and counted.  d_c = the valid
 * entries of chunk c.  A chunk contributes iff 2 <= d_c <= max_mentions (2 <= max_mentions <= 4096); one of more is counted and
 * gives nothing.  A contributing chunk gives every two valid entries a < b of its row the value 1 (mode 0, "count") or w_a * w_b
 * (mode 1, "product", below 2^24); two equal entities in a row (a malformed row) give nothing.  T = sum d_c (d_c - 1) / 2 over the
 * contributing chunks; W(a, b) = the sum of the values of (a, b) over all chunks.  Every sum is an integer sum over a set: the same
 * bits for any order of the mentions and from run to run.  An entity id is never used as an index (csrc/cooccur.hip).
 * Limits: 1 <= n_chunks < 2^31 - 1, 1 <= nnz < 2^31, 2 <= n < 2^31 - 1.  Pointers aligned to their element, workspaces to 256
 * bytes, each *_workspace_bytes returning 0 for a refused shape; everything is refused before any launch.
 *
 * rarc_cooccur_count — every chunk's valid count, its pairs and their exclusive scan (the write offsets), and the lists of the
 *   chunks of each degree class, into d_ws.  d_out4 int64 [4] = {T, contributing chunks, chunks over max_mentions, entries
 *   skipped}.  T >= 2^31 (rarc_sort_reduce's count limit) is the caller's to refuse, T == 0 its empty answer: neither may reach
 *   rarc_cooccur_emit.
 * rarc_cooccur_emit — after rarc_cooccur_count on the same CSR and d_ws.  d_keys uint64 [T]: key = a << bits | b with bits =
 *   ceil(log2 n), so key_bits = 2 bits <= 62 is what rarc_sort_reduce is then given; d_values uint32 [T] for mode 1, null (or
 *   ignored) for mode 0, where every value is 1.  Slots come from the scanned offsets, no atomic cursor: the pairs of a row's
 *   i-th valid entry are one contiguous run.  A wave expands a chunk of at most 64 valid entries, a workgroup with the row in LDS
 *   a larger one (rarc_cooccur_limits).  T as rarc_cooccur_count reported it, 1 <= T < 2^31: no slot at or past it is written.
 *   Two equal entities leave the key a << bits | a (value 0 in mode 1), which rarc_cooccur_edges drops.
 * rarc_cooccur_edges — d_keys, d_sums uint64 [distinct] as rarc_sort_reduce wrote them (distinct keys ascending, 64-bit sums), 1 <=
 *   distinct < 2^31; min_weight >= 1.  Keeps the keys with a < b and W >= min_weight, in their order: d_out_pairs int64
 *   [distinct][2] by (a, b) ascending, d_out_weights uint32 [distinct] (the low 32 bits of W: the largest is reported); d_out3
 *   int64 [3] = {edges written, largest W over all keys with a < b, edges below min_weight}.  A largest W >= 2^32 (mode 1 only)
 *   is the caller's to refuse before it uses the result.  Its workspace is rarc_cooccur_edges_workspace_bytes(distinct).
 * rarc_cooccur_limits — out4 = {largest degree of the wave form, largest max_mentions, bits of a product value, log2 of the T
 *   limit}.
 */
size_t rarc_cooccur_workspace_bytes(int64_t n_chunks, int64_t nnz);
int rarc_cooccur_count(const int64_t* d_row_ptr, const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz, int64_t n,
                       int max_mentions, void* d_ws, size_t ws_bytes, int64_t* d_out4, void* stream);
int rarc_cooccur_emit(const int64_t* d_row_ptr, const int32_t* d_ent, const uint32_t* d_w, int64_t n_chunks, int64_t nnz, int64_t n,
                      int mode, const void* d_ws, size_t ws_bytes, uint64_t* d_keys, uint32_t* d_values, int64_t total, void* stream);
size_t rarc_cooccur_edges_workspace_bytes(int64_t distinct);
int rarc_cooccur_edges(const uint64_t* d_keys, const uint64_t* d_sums, int64_t distinct, int64_t n, int64_t min_weight, void* d_ws,
                       size_t ws_bytes, int64_t* d_out_pairs, uint32_t* d_out_weights, int64_t* d_out3, void* stream);
int rarc_cooccur_limits(int* out4);

/*
 * Deleting rows of a resident index: stable in-place compaction.  The reference deletes by clearing the index and
 * embedding every surviving text again (encapsulation/database/vector_db/VectorStore_Faiss.py:374-415); the surviving
 * rows are in HBM already, so here they move down over the holes: row i of the result is the i-th surviving row.
 * d_rows: n_rows rows of row_bytes (a multiple of 4) — the fp16 / fp8 / fp32 rows, and likewise the fp8 row scales
 * (row_bytes 4), the fp32 index's fp16 image, the int8 shadow.  d_adj: device int64 [n_holes], d_adj[j] = h_j - j for
 * the sorted distinct hole rows h_j; first_hole = h_0.  d_tmp: caller-owned scratch (>= one row; the rows move through
 * it chunk by chunk).  The vacated tail [n_rows - n_holes, n_rows) is zeroed.  Tile metadata is NOT updated: call
 * rarc_quant_meta_* from first_hole afterwards.
 */
int rarc_compact_rows(void* d_rows, int64_t row_bytes, int64_t n_rows, const int64_t* d_adj, int64_t n_holes,
                      int64_t first_hole, void* d_tmp, size_t tmp_bytes, void* stream);

/*
 * Growable device arenas: where `index.add` appends to (encapsulation/database/vector_db/VectorStore_Faiss.py:199-202 —
 * faiss grows a std::vector there).  An arena owns VIRTUAL addresses for the largest size it may reach (no memory) and is
 * backed slab by slab as rows arrive: the base pointer never moves and nothing is copied, so the peak footprint of a
 * growing index is its live rows rounded up to one slab (a reallocating buffer holds old + new: up to 3x).
 * The second kind of object this library allocates (with the tokenizer handle): release it with rarc_vmem_destroy, after
 * the last kernel that reads it.  Arenas are slab-aligned sub-ranges of ONE address space the first create reserves for
 * the process and never frees (RARC_VMEM_SPACE_TIB TiB, default 16; addresses that were backed once are not handed out
 * again, so the space lasts for that many TiB of slabs mapped over the life of the process); every piece of physical memory is one SLAB
 * (slab_bytes, 0 = RARC_VMEM_DEFAULT_SLAB, rounded up to the device's mapping granularity), ONE slab size per process — a
 * create with another size returns RARC_E_UNSUPPORTED, a create the space has no room for RARC_E_WORKSPACE.
 * min_reserve_bytes (0 = reserve_bytes): when no free range holds reserve_bytes, the largest one that holds at least this
 * much is taken whole — rarc_vmem_reserved reports what the arena got.  (What this HIP
 * runtime does with anything else is written down in csrc/vmem.hip and reproducible with tools/vmem_probe.py.)
 * rarc_vmem_grow(min_bytes): back at least the first min_bytes, in whole slabs (never shrinks; on failure — HBM
 * exhausted — what was mapped stays mapped and usable).  Not tied to a stream: mapping is a host-side operation,
 * visible to later launches.
 */
#define RARC_VMEM_DEFAULT_SLAB (16u << 20)
typedef struct RarcVmem RarcVmem;
int rarc_vmem_create(int device, size_t reserve_bytes, size_t min_reserve_bytes, size_t slab_bytes, RarcVmem** out);
int rarc_vmem_grow(RarcVmem* arena, size_t min_bytes);
void* rarc_vmem_base(const RarcVmem* arena);
size_t rarc_vmem_mapped(const RarcVmem* arena);
size_t rarc_vmem_reserved(const RarcVmem* arena);
size_t rarc_vmem_slab(const RarcVmem* arena);
size_t rarc_vmem_granularity(const RarcVmem* arena);
int rarc_vmem_destroy(RarcVmem* arena);

/*
 * Measurement hooks (bench.py): while profiling is on, every rarc_search_f16 brackets its scan
 * kernel with a pair of HIP events recorded on the search's own stream.  rarc_profile_end
 * synchronises, returns the summed scan time and the number of launches measured, and releases
 * the events.  One profiling session at a time per process (the event list is guarded by a mutex, so searches
 * issued from other threads while a session is open are measured too, in launch order).
 */
int rarc_profile_begin(int max_launches);
int rarc_profile_end(double* total_scan_ms, int* n_launches);

#ifdef __cplusplus
}
#endif
#endif /* RARC_H */
