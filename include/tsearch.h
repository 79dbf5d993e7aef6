/*
 * tsearch.h - C ABI of libtsearch.so, the MI355X (gfx950) brute-force theorem-search engine.
 *
 * The reference (uw-math-ai/TheoremSearch) has no FFI of its own: its hot path is Python
 * calling third-party Python.  These entry points are what a ctypes
 * binding for that path binds; each one names the reference call it stands in for.  The only
 * caller in this repository is theoremsearch_amd/_ffi.py; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; every function returns an int status (TS_OK or a negative TS_ERR_*);
 *     ts_last_error() gives the thread-local message of the last failure.
 *   - the caller owns every host buffer it passes; the library owns the device memory behind
 *     the opaque handles.
 *   - rows are row-major; dtype codes TS_F32 (IEEE binary32) and TS_BF16 (bfloat16 bit patterns,
 *     uint16_t).
 *   - search results: for every query, k entries ordered by score descending, then index
 *     ascending; NaN scores are never returned; when fewer than k rows qualify the tail is
 *     (score = -inf, index = -1).
 *   - a stream argument is a hipStream_t passed as void* (NULL = the index's own stream).  With
 *     host output buffers the call returns after the results have landed; with device buffers
 *     it returns after enqueueing the work on that stream.  The index's own stream is a blocking
 *     stream: it is ordered with the legacy null stream, so NULL is also the right value for work
 *     that lives on the default stream of the caller (torch.cuda.current_stream().cuda_stream is 0
 *     there).  A call that arrives on a different stream than the previous call on the same handle
 *     is ordered behind that call by the library (the handle's scratch buffers are shared); for
 *     that the library records an event at the END of every call on the stream of that call and never touches
 *     that stream again: a caller-owned stream may be destroyed as soon as the caller's own work on it is done.
 *     A call made while its stream is being captured into a HIP graph records no such event: the caller orders replays of
 *     that graph against other calls on the handle itself.
 *   - device queries may be read in place (no copy is made when they already have the form the kernels multiply):
 *     they must stay unchanged until the work the call enqueued has run.
 *   - one handle may be used from several threads (the Streamlit apps share one model and one
 *     library across session threads, streamlit_app.py:52); calls on one handle are serialised
 *     inside, different handles are independent.
 */
#ifndef TSEARCH_H
#define TSEARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library itself is built with hidden visibility: what this header declares is what it exports */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define TS_VERSION 100 /* 0.1.0 */

#define TS_OK 0
#define TS_ERR_INVALID (-1)     /* bad argument */
#define TS_ERR_HIP (-2)         /* a HIP runtime call failed (message has hipGetErrorString) */
#define TS_ERR_NOMEM (-3)       /* device or host allocation failed */
#define TS_ERR_NODEVICE (-4)    /* no usable gfx950 device */
#define TS_ERR_UNSUPPORTED (-5) /* valid request this build has no kernel for */
#define TS_ERR_INTERNAL (-6)

#define TS_F32 0
#define TS_BF16 1

#define TS_METRIC_IP 0  /* inner product: pgvector "<#>" on stored-normalised rows, streamlit_app.py:275-282 */
#define TS_METRIC_COS 1 /* cosine: sentence_transformers.util.cos_sim, app_showcase_model.py:93 */

#define TS_ALGO_AUTO 0
#define TS_ALGO_SCAN 1 /* streaming dot-product scan with per-wave running top-k (any dtype, any d) */
/* MFMA contraction with thresholded candidate selection, bf16 or fp32 index: d = 384, 512, 768 or 1024 on the hand-laid kernels;
 * any other d that is a multiple of 64, from 128 up to a 4,096-byte row (bf16 d <= 2048, fp32 d <= 960), on the general-width
 * kernel; wider rows whose d is a multiple of 256, up to a 16,384-byte row (bf16 d = 2304 .. 8192, fp32 d = 1280 .. 4096), on
 * the k-chunked kernel (both: 256 queries per pass; only under the default two-level search, and for fp32 not with
 * TS_MFMA_F32=0, which takes fp32 indexes off the matrix path at every width).  Other widths: TS_ERR_UNSUPPORTED.  Scores are reproducible per width and storage type: the
 * same (query, row) pair gets the same score bits whatever the batch size and the launch shape. */
#define TS_ALGO_MFMA 2

#define TS_MAX_K 256

typedef struct ts_index ts_index;
typedef struct ts_timer ts_timer;

/* Per-call counters of ts_search_ex (all optional; zero-filled first). */
typedef struct ts_search_stats {
    int32_t algo;            /* TS_ALGO_SCAN or TS_ALGO_MFMA actually used */
    int32_t levels;          /* MFMA path: number of threshold levels run */
    int32_t fallback_queries; /* MFMA path: queries re-run through the scan (candidate overflow); -1 = not read back */
    int32_t screened;        /* MFMA path: 1 = the full pass ran as the int8 screen + exact rescore (same answers, bit for bit), else 0 */
    int64_t candidates;      /* MFMA path: candidates appended in the last level; -1 = not read back */
} ts_search_stats;

/* ---- library / device -------------------------------------------------------------------- */

int ts_version(void);
const char *ts_last_error(void);
/* Number of visible HIP devices (0 on a CPU-only host; never fails for "no device"). */
int ts_device_count(int *count);
int ts_device_info(int device, char *name, int name_len, int64_t *total_mem_bytes, int32_t *compute_units);
int ts_device_synchronize(int device);

/* ---- the index: the [N x d] theorem-embedding matrix resident in HBM -------------------------
 * Stands in for the corpus tensor of the in-process form (torch.load of corpus_embeddings.pt,
 * app_showcase_model.py:52) and for the theorem_embedding_* tables of the in-database form
 * (rds_schema.sql:43-56).  dtype is the storage type; metric TS_METRIC_COS L2-normalises every
 * row once at upload (x / max(||x||, 1e-12), what util.cos_sim redoes on every call), then
 * rounds to bf16 when dtype is TS_BF16.  row_offset is the global id of row 0 (sharded use).
 */
int ts_index_create(int device, int64_t n, int32_t d, int dtype, int metric, ts_index **out);
/* Waits for the handle's work in flight, then frees it.  TS_ERR_UNSUPPORTED while views of it are alive (ts_index_view). */
int ts_index_destroy(ts_index *ix);
int ts_index_set_row_offset(ts_index *ix, int64_t row_offset);
/* The index's own HIP stream (hipStream_t as void*): what stream = NULL means in the calls below. */
int ts_index_stream(const ts_index *ix, void **stream);
/* Makes `stream` (hipStream_t as void*, not NULL) wait for the end of the LAST call on this handle, whatever stream that
 * call ran on (stream-ordered, no host wait): a side stream that consumes a search's device results - the exchange + merge
 * of the sharded search - needs no event of its own on the search's stream. */
int ts_index_wait_order(ts_index *ix, void *stream);
/* The ONE host-only entry (SURVEY.md 8b "ts_search_cpu"; BASELINE.json configs[0], the reference's CPU-runnable case:
 * util.cos_sim + argsort over ~1k theorems, compare_embeddings.py:24-31,55-92).  Stateless and explicit: no device entry
 * falls back to it, nothing selects it by itself; Python reaches it only through TheoremIndex(..., device=-1).
 * rows [n x d] and queries [nq x d] are HOST arrays (fp32, or bf16 bit patterns), prepared on every call exactly as
 * ts_index_upload / ts_search prepare them on the device (metric cos: x / max(||x||, 1e-12) with the norm in fp64; store_dtype
 * TS_BF16: rounded to nearest even); scores are fp32 dot products of the prepared values; results in the library's order
 * (score descending, row ascending; NaN never ranks), padded with (-inf, -1).  threads <= 0: one per hardware thread. */
int ts_search_cpu(const void *rows, int rows_dtype, int64_t n, int32_t d, int store_dtype, int metric,
                  const void *queries, int q_dtype, int32_t nq, int32_t k, float *out_scores, int64_t *out_idx,
                  int32_t threads);
/* Device-to-device copy of `bytes` bytes on `device`, enqueued on `stream` (hipStream_t as void*; NULL = the legacy null
 * stream): lets a Python caller that only holds raw device addresses stage a query batch in a buffer of its own before a
 * search on another stream reads it (ShardedSearcher with several searches in flight: the caller's stream then waits for
 * this copy, not for the whole search). */
int ts_copy_device(int device, void *dst, const void *src, int64_t bytes, void *stream);
/* Waits until everything this handle has enqueued (on its own stream and on the stream of its last call) is done. */
int ts_index_synchronize(ts_index *ix);
int ts_index_info(const ts_index *ix, int64_t *n, int32_t *d, int32_t *dtype, int32_t *metric,
                  int64_t *ld_elems, int64_t *row_offset, void **device_rows);

/* Tuning / diagnostic options of one handle (the TS_* knobs of DESIGN.md section 8, e.g. "TS_MFMA_FIRST_ROWS").  Their
 * initial values are read from the environment once, when the handle is created; afterwards only these calls change
 * them (the search path never calls getenv).  reset = back to the built-in default.  The reference has no counterpart.
 * "TS_MFMA_SCREEN" (default 1): the thresholded full pass of a bf16 d = 768 index that owns its rows runs as an int8 screen
 * (an int8 image of the rows, 768 bytes per row more) followed by an exact rescore of the screened rows from the bf16 rows.
 * "TS_MFMA_SCREEN_WIDE" (default 0): the same for bf16 d = 1024 indexes - opt-in because the image costs 1,024 bytes per row
 * (10.24 GB at 10M rows; allocated and filled on the first screened search, kept up to date lazily after uploads / appends).
 * "TS_MFMA_SCREEN_F32" (default 0): the same for fp32 indexes at d = 768 and d = 1024 on the 16x16 kernel (never the 32x32x2
 * kernel, TS_MFMA_F32=32, and only the usual two-level search: not with TS_MFMA_STAT=0 or TS_MFMA_SAMPLE=0) - int8 screen, then an exact fp32 rescore that repeats the fp32 pass's fmaf chain; a screened search
 * holds up to 256 queries per launch instead of 64 or 128.  Opt-in because the image costs d bytes per row on top of the rows
 * (+25 %: 7.68 GB at 10M x 768).  TS_MFMA_SCREEN=0 switches every screen off.
 * "TS_MFMA_SCREEN_LATE" (default 1): the screen's launch of an unmasked bf16 d = 768 search of 193 .. 256 queries runs the
 * late-test form of the tile kernel (a tile's block tests stand among the next tile's MFMAs); 0 = the kernel that tests every
 * tile at its own end, which every other screened launch runs either way.  The same pairs, no memory of its own.
 * Contract of all of them: ids and score bits of every search are identical with the option on and off, for every batch size and
 * whichever form the unscreened pass would take (TS_MFMA_PAIR, TS_MFMA_GRID at bf16 d = 1024) - for every query that neither
 * call sent to the exact re-run, which has the scan's arithmetic either way; views and attached rows are never screened.
 * ts_search_stats.screened tells which pass a call ran.
 * "TS_MFMA_WIDE_SERIAL" (default 0): 1 = the k-chunked kernel (rows wider than 4,096 bytes) runs the plain form of its chunk
 * loop, two barriers per k-chunk instead of one: the timing partner of the default; ids and score bits are the same. */
int ts_index_set_option(ts_index *ix, const char *name, int32_t value);
int ts_index_reset_option(ts_index *ix, const char *name);

/* Rows [row0, row0 + nrows) from host memory (src_dtype TS_F32 or TS_BF16, dense [nrows x d]).
 * Replaces building the corpus tensor (app_create_embeddings.py:81-89) and the per-row INSERT /
 * upsert of vectors (parsed_papers_to_vector_rds/rds.py:37-91, ec2/generate_embeddings/__main__.py:85-99). */
int ts_index_upload(ts_index *ix, const void *host_rows, int src_dtype, int64_t row0, int64_t nrows);
/* The same from device memory (row stride src_ld elements), enqueued on `stream`: encoder output
 * goes straight into the index without a host hop. */
int ts_index_upload_device(ts_index *ix, const void *dev_rows, int src_dtype, int64_t src_ld,
                           int64_t row0, int64_t nrows, void *stream);
/* Growth ("incremental append mirroring the upsert-by-slogan_id semantics",
 * ec2/generate_embeddings/__main__.py:85-99 - a slogan_id that is not in the table yet is INSERTed).  ts_index_reserve
 * makes room for `capacity_rows` rows without changing n; ts_index_append* add nrows rows behind the last one (growing
 * the allocation 1.5x when it is full: one device-to-device move of the rows) and return the global id of the first
 * new row.  Not on views / subset indexes, and refused (TS_ERR_UNSUPPORTED) while views of the index are alive.
 * Views and subsets made earlier do not see the new rows. */
int ts_index_reserve(ts_index *ix, int64_t capacity_rows);
int ts_index_append(ts_index *ix, const void *host_rows, int src_dtype, int64_t nrows, int64_t *first_row);
int ts_index_append_device(ts_index *ix, const void *dev_rows, int src_dtype, int64_t src_ld, int64_t nrows,
                           void *stream, int64_t *first_row);
/* Zero-copy: the index adopts rows that already sit in device memory - e.g. the tensor an encoder
 * wrote.  They must be what the kernels multiply: the index's storage dtype, row stride = ld (d padded to 64 elements),
 * normalised already when the metric is cosine; the allocation must hold capacity_rows >= n rounded up to 256 rows (whole
 * 32-row tiles are read; rows past n are never returned).  The caller keeps ownership: the memory must stay alive and
 * unchanged while searches run; the index's own allocation is released; an attached index cannot grow. */
int ts_index_attach_device(ts_index *ix, void *dev_rows, int64_t capacity_rows);
/* Stored rows back to the host in the storage dtype, dense [nrows x d] (what the kernels multiply). */
int ts_index_download(ts_index *ix, void *host_rows, int64_t row0, int64_t nrows);

/* ---- search --------------------------------------------------------------------------------
 * out_scores [nq x k] float, out_idx [nq x k] int64 (global ids = local row + row_offset).
 * Replaces  util.cos_sim(q, db)[0] + np.argsort(-s)[:5]        (app_scratchpad.py:129-130)
 *           util.cos_sim(q, db)[0] + torch.topk(s, k, sorted)   (app_showcase_model.py:93-96)
 *           ORDER BY e.embedding <#> q ASC LIMIT k              (streamlit_app.py:282-283)
 * queries: [nq x d] dense, q_dtype TS_F32 or TS_BF16, in host (q_on_device = 0) or device memory.
 * With metric COS the queries are L2-normalised first; with a bf16 index they are rounded to bf16.
 * 1 <= k <= TS_MAX_K.
 * A batch (more than 4 queries; when k > 64, where the scan serves one query per pass, more than 1 - more than 2 on the fp32
 * general-width kernel: measured) over at least 16,384
 * rows runs on the matrix path where the index has one: bf16 / fp32 at d = 384, 512, 768, 1024 (hand-laid kernels), and at
 * every other multiple of 64 from 128 up to a 4,096-byte row (the general-width kernel), and at every multiple of 256 with a
 * wider row of up to 16,384 bytes (the k-chunked kernel: bf16 d = 2304 .. 8192, fp32 d = 1280 .. 4096).  The same holds for
 * ts_search_ex, ts_search_filtered*, ts_search_rowset and ts_search_biased_ex.  Anything else runs on the streaming scan,
 * four queries per pass.  Either way the answer is the exact top k; matrix-path scores are reproducible per width and storage
 * type (the same score bits for a (query, row) pair in any batch) and may differ from the scan's in the last bits.
 */
int ts_search(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
              float *out_scores, int64_t *out_idx, int out_on_device, void *stream);
int ts_search_ex(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                 float *out_scores, int64_t *out_idx, int out_on_device, void *stream, int algo,
                 ts_search_stats *stats);

/* Parses pgvector's text form of vectors - "[0.1,-2e-3,...]", one per row, whatever stands between the rows (ids, tabs,
 * newlines: the output of COPY (SELECT slogan_id, embedding ...) TO STDOUT or of SELECT embedding::text) - into a dense
 * fp32 matrix, each value by one strtof as pgvector's own vector_in does.  Feeds ts_index_upload from the RDS tables
 * the upsert pipeline fills (ec2/generate_embeddings/embeddings.py:27-40 sends embedding.tolist(); rds_schema.sql
 * embedding_* tables) without a Python float per value.  Stops after max_rows rows or at the last complete row of the
 * buffer; *consumed = bytes up to the end of that row, so a stream can be fed in pieces.  Host only, no device. */
int ts_parse_pgvector_text(const char *text, int64_t len, int32_t d, float *out, int64_t max_rows, int64_t *rows_parsed,
                           int64_t *consumed);

/* A second HANDLE on the rows of `src` (no copy): its own stream, scratch buffers and lock, so that two searches of the
 * same corpus can be in flight on two streams - the small kernels at the head of one search (query preparation, the
 * threshold sample and its select) then overlap the tail of the previous one (final select, re-run check, merge).
 * What a serving loop over independent query batches wants; the reference has no counterpart (one process, one query
 * at a time, streamlit_app.py:165-173).  Read-only; must be destroyed before `src`; set_row_offset / subsets of `src`
 * made later are not seen by the view. */
int ts_index_view(ts_index *src, ts_index **out);

/* A second index holding copies of the given rows of `src` (global ids, strictly ascending, host memory); searches
 * of it return the ORIGINAL global ids, in the same canonical order.  The filtered search for query batches and for
 * filters that stay fixed over many searches (a sidebar state, app_showcase_model.py:96-129; the WHERE clause of
 * streamlit_app.py:175-283): the copy costs 2 * nrows * ld * elem bytes of HBM traffic once, after which every
 * search runs the unfiltered kernels over nrows rows.  Rows are copied as stored (no second normalisation).
 * Uploading into a subset index and ts_rank_of on it are not supported. */
int ts_index_subset(ts_index *src, const int64_t *rows, int64_t nrows, ts_index **out);

/* Search restricted to the rows whose bit is set in row_mask (uint32 words, bit r & 31 of word r >> 5 = row r,
 * ceil(n / 32) words, host or device memory): the k best ALLOWED rows, exactly.  Stands in for the metadata
 * filters of the apps - the WHERE clause in front of ORDER BY ... LIMIT k (streamlit_app.py:175-243,253-283) and
 * the post-filter loop over the top-200 (app_showcase_model.py:96-129), which can return fewer than top_k hits
 * although more exist.  The caller evaluates the predicates to the bitmask; the scan kernel tests the bit before
 * a row can enter a top-k list (N / 8 extra bytes per pass). */
int ts_search_filtered(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                       const uint32_t *row_mask, int mask_on_device, float *out_scores, int64_t *out_idx,
                       int out_on_device, void *stream);

/* The same with an algorithm hint (TS_ALGO_SCAN is honoured; TS_ALGO_MFMA is refused with TS_ERR_UNSUPPORTED when the mask is
 * too sparse or lives on the device, or the index has no matrix path - see TS_ALGO_MFMA for the widths served, hand-laid and
 * general; TS_ALGO_AUTO decides by the mask's density) and the per-call counters.  On the matrix path the mask's bit is tested
 * where a score passes the threshold, on the hand-laid and on the general-width kernel alike; scores are reproducible per
 * width and storage type. */
int ts_search_filtered_ex(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                          const uint32_t *row_mask, int mask_on_device, float *out_scores, int64_t *out_idx,
                          int out_on_device, void *stream, int algo, ts_search_stats *stats);

/* Top-k of  score(row) + weight * bias[row]  over ALL rows of the index (or all rows row_mask allows; row_mask may be NULL):
 * the citation-weighted ranking of streamlit_app.py:348-364 -
 *     weighted_score = similarity + w * CASE WHEN citations > 0 THEN ln(citations) ELSE 0 END   ORDER BY weighted_score DESC
 * - computed over the whole corpus instead of over the max(50, 10 k) nearest rows the SQL ranks (streamlit_app.py:317): the
 * pool form misses a heavily cited theorem that is not among the 10 k nearest; this one cannot (SURVEY.md section 8f rank 4:
 * "score + w * ln(citations) as a fused per-row bias, one fp32 side array").  bias: float[n] in host or device memory, one
 * value per row of THIS index (the caller puts ln(citations) or 0 there); the term is added in fp32 where the key of a row
 * is made (fmaf(weight, bias[row], score)), so the order is weighted score descending, then row ascending.  out_scores
 * receives the weighted scores, out_sims (optional, same shape and place) the raw similarities.  Runs on the scan kernel
 * (four queries per pass at the HBM rate; n * 4 more bytes per pass); not on subset indexes. */
int ts_search_biased(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                     const float *bias, int bias_on_device, float weight, const uint32_t *row_mask, int mask_on_device,
                     float *out_scores, float *out_sims, int64_t *out_idx, int out_on_device, void *stream);

/* The same ranking with an algorithm hint and the per-call counters: the batched form (a page of queries, an evaluation set).
 * The answer is the exact weighted top k whatever the path.
 *   TS_ALGO_SCAN  what ts_search_biased runs, bit for bit.
 *   TS_ALGO_MFMA  the biased matrix search: a dense threshold sample, then ONE pass of the general-width matrix kernel per 256
 *                 queries with fmaf(weight, bias[row], score) in its epilogue - that value is tested against the query's
 *                 threshold, written into the key and returned.  Served: a bf16 or fp32 index whose width is a multiple of 64
 *                 from 128 up to a 4,096-byte row (bf16 d <= 2048, fp32 d <= 1024; 384 / 512 / 768 / 1024 included), or a
 *                 multiple of 256 with a wider row of up to 16,384 bytes (bf16 d = 2304 .. 8192, fp32 d = 1280 .. 4096: the
 *                 k-chunked kernel with the same epilogue).
 *                 TS_ERR_UNSUPPORTED for a subset index, any other width, without the two-level search (TS_MFMA_STAT=0 or
 *                 TS_MFMA_SAMPLE=0), an fp32 index with TS_MFMA_F32=0, a mask in device memory, or a host mask too sparse by
 *                 the rule of ts_search_filtered_ex (fewer than a tenth of the rows, or a batch the matrix path does not take).
 *   TS_ALGO_AUTO  the matrix search for more than 4 queries (fp32 indexes: more than 8; k > 64: more than 1) over at least
 *                 TS_MFMA_MIN_ROWS rows where it is served, else the scan (measured: DESIGN.md section 3.4).
 * The threshold is an estimate from the sample (Gaussian similarities plus the KNOWN additive term); a
 * query that gets fewer than min(k, allowed rows) candidates back is re-run exactly on the scan kernel, so the estimate can
 * cost time, never an answer.  Matrix-path scores are reproducible per width and storage type: the same bits for a (query,
 * row) pair in any batch or grid; they may differ from the scan's in the last bits, and re-run queries carry the scan's
 * arithmetic.  stats as for ts_search_ex: algo, levels (2; 1 on an index so small that the pass runs unthresholded),
 * fallback_queries (re-run queries), candidates, screened = 0. */
int ts_search_biased_ex(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                        const float *bias, int bias_on_device, float weight, const uint32_t *row_mask, int mask_on_device,
                        float *out_scores, float *out_sims, int64_t *out_idx, int out_on_device, void *stream, int algo,
                        ts_search_stats *stats);

/* ---- metadata filters evaluated on the device -----------------------------------------------------
 * The WHERE clause in front of ORDER BY <#> LIMIT k (streamlit_app.py:175-283) and the sidebar predicates of the showcase app
 * (app_showcase_model.py:102-121), evaluated to the row bitmask of ts_search_filtered by one kernel over the rows' metadata
 * held as columns in HBM, instead of by a host predicate per row.
 *
 * ts_meta: up to 32 columns over n rows of one device.  A scalar column is int32 per row (a dictionary code, a year, a count,
 * a 0 / 1 flag); TS_META_NULL is SQL NULL.  ts_meta_set_column uploads rows [row0, row0 + nrows) from host memory and may be
 * called again for any range (the upsert by slogan_id); rows of a scalar column that were never uploaded are NULL.  A list
 * column (the authors) is set whole, as CSR: offsets[n + 1] ascending from 0, codes[offsets[n]] all >= 0; a NULL list is
 * stored as an empty one.  A column keeps the kind of its first upload.  n is fixed: a table does not grow with
 * ts_index_append, and a search whose index has another n is refused.
 *
 * A program is a list of at most 32 atoms in at most 16 groups (distinct values of `group`, any integers):
 *   - a row passes when every group holds; a group holds when at least one of its atoms is true; the empty program
 *     (natoms = 0) allows every row;
 *   - TS_ATOM_RANGE: lo <= v <= hi;  TS_ATOM_IN: bit v of `set` (v < 0 or v >= set_bits: not in the set);  `negate` inverts
 *     either - but an atom whose value is TS_META_NULL is not true, negated or not.  That is SQL's three-valued logic as a
 *     WHERE clause sees it (a comparison with NULL is not true, and neither is its NOT);
 *   - TS_ATOM_IS_NULL: v == TS_META_NULL; with `negate`, v != TS_META_NULL;
 *   - TS_ATOM_ANY_IN (list columns only): some code of the row's list has its bit in `set`; false on an empty list; `negate`
 *     is refused.
 * TS_ERR_INVALID with a message for every malformed program: more than 32 atoms or 16 groups, a kind out of range, a column
 * out of range, never set or of the other kind (scalar atoms on a list column, ANY_IN on a scalar one), lo > hi, negate
 * outside 0 / 1, a missing set (NULL with set_bits > 0) or set_bits outside [0, INT32_MAX].  Sets are host bitsets (uint32 words, bit c & 31 of word
 * c >> 5 = code c, ceil(set_bits / 32) words), copied by the call.
 *
 * ts_meta_eval runs the program over all n rows on `stream` (hipStream_t as void*; NULL = the legacy null stream) and waits
 * for the count: *out owns a device bitmask in the layout of ts_search_filtered - n bits, allocated in whole 256-row blocks,
 * every bit past n zero - and knows how many rows it allows.  A row set is immutable (later ts_meta_set_column calls do not
 * change it) and belongs to the device of its ts_meta.  There is no host evaluator. */
typedef struct ts_meta ts_meta;
typedef struct ts_rowset ts_rowset;

#define TS_META_NULL INT32_MIN
#define TS_META_MAX_COLS 32
#define TS_META_MAX_ATOMS 32
#define TS_META_MAX_GROUPS 16

int ts_meta_create(int device, int64_t n, int32_t ncols, ts_meta **out);
int ts_meta_destroy(ts_meta *m);
int ts_meta_set_column(ts_meta *m, int32_t col, const int32_t *values, int64_t row0, int64_t nrows);
int ts_meta_set_lists(ts_meta *m, int32_t col, const int64_t *offsets, const int32_t *codes);

#define TS_ATOM_RANGE 0
#define TS_ATOM_IN 1
#define TS_ATOM_ANY_IN 2
#define TS_ATOM_IS_NULL 3
typedef struct ts_atom {
    int32_t kind, col, lo, hi;
    int32_t negate;      /* 0 / 1 */
    int32_t group;       /* atoms of one group are OR-ed, the groups are AND-ed */
    const uint32_t *set; /* host bitset over the column's codes (IN, ANY_IN) */
    int64_t set_bits;
} ts_atom;

int ts_meta_eval(ts_meta *m, const ts_atom *atoms, int32_t natoms, ts_rowset **out, void *stream);
/* n, the rows allowed and the device address of the mask (each may be NULL) */
int ts_rowset_info(const ts_rowset *r, int64_t *n, int64_t *allowed, void **device_mask);
/* the mask to host memory: ceil(n / 32) words */
int ts_rowset_download(ts_rowset *r, uint32_t *host_words);
int ts_rowset_destroy(ts_rowset *r);

/* ts_search_filtered_ex / ts_search_biased_ex with the mask and its count taken from a row set.  Because the count is known,
 * a device mask is decided as a counted host mask is: a batch the matrix path takes runs there when the row set allows at
 * least a tenth of the rows (TS_ALGO_MFMA is refused with TS_ERR_UNSUPPORTED when it is sparser), everything else on the
 * scan.  (A bare device mask handed to ts_search_filtered_ex keeps its rule: the scan.)  TS_ERR_INVALID when the row set has
 * another n than the index or lives on another device; on a subset index the mask is over the subset's own rows, as for
 * ts_search_filtered.  The row set must stay alive until the enqueued work has run. */
int ts_search_rowset(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                     const ts_rowset *rows, float *out_scores, int64_t *out_idx, int out_on_device, void *stream,
                     int algo, ts_search_stats *stats);
int ts_search_biased_rowset(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                            const float *bias, int bias_on_device, float weight, const ts_rowset *rows,
                            float *out_scores, float *out_sims, int64_t *out_idx, int out_on_device, void *stream,
                            int algo, ts_search_stats *stats);

/* ---- a row set per query: one matrix pass for a batch whose queries sit behind different filters -------
 * Query q is searched behind sets[which[q]], or behind no filter when which[q] == -1 (`which`: host memory, nq entries;
 * sets: host array of nsets <= TS_MAX_ROWSETS handles, entries nobody names may be NULL).  Output row q is what
 * ts_search_rowset defines for query q alone behind its set (ts_search_ex for -1): the exact top k of the allowed rows, by
 * score descending, then id ascending, padded with -inf / -1, ids global.
 *
 * Routing (csrc/rowsets_plan.h holds the rules):
 *   - all queries name one set: the call IS ts_search_rowset with that set (all -1: ts_search_ex), its paths and its bits;
 *   - otherwise the queries whose set allows at least a tenth of the rows ride ONE pass of the general-width matrix kernel per
 *     256 of them (a dense threshold sample and a threshold per query from that query's own rows, the query's mask bit tested
 *     only for scores that pass its threshold, a final select that sends a query with too few or too many candidates to an
 *     exact re-run behind its own set) - when the index is bf16 or fp32, has at least TS_MFMA_MIN_ROWS rows and a width that
 *     is a multiple of 64 from 128 up to a 4,096-byte row (384 / 512 / 768 / 1024 included), under the default two-level
 *     search, and those queries number more than one scan pass serves (4; fp32: 8; k > 64: 1) and name at least two sets;
 *   - every other query (a sparse or empty set, a width or option the pass does not serve, the k-chunked widths, a small
 *     remainder) is grouped by set, one call of the existing search per set under TS_ALGO_AUTO; a set that allows nothing
 *     returns the padding without a launch.
 * algo: TS_ALGO_SCAN runs every set's queries on the scan (the A/B partner of the pass); TS_ALGO_MFMA is refused with
 * TS_ERR_UNSUPPORTED unless every query rides the pass; a delegated call hands algo on.
 *
 * Score bits of a query of the shared pass are the general-width kernel's single MFMA chain, as for ts_search_biased_ex: at
 * the widths that kernel serves for ts_search_rowset they equal that call's bits; at 384 / 512 / 768 / 1024 they are the
 * general-width kernel's, not the hand-laid kernels'.  Nothing more is promised across the two paths.
 *
 * TS_ERR_INVALID: nsets outside [0, TS_MAX_ROWSETS], a which[q] outside [-1, nsets), a named set that is NULL, has another n
 * or lives on another device than the index, k outside [1, TS_MAX_K], NULL queries or outputs.  TS_ERR_UNSUPPORTED: a subset
 * index.  nq == 0 does nothing.  The call waits for its pass (the re-run list is read back per block of 256 queries); the
 * row sets must stay alive until it returns. */
#define TS_MAX_ROWSETS 256
typedef struct ts_rowsets_stats {
    int32_t algo;             /* TS_ALGO_MFMA when at least one query ran in the shared pass, else TS_ALGO_SCAN
                                 (a delegated call: what the call it became reports) */
    int32_t sets_used;        /* distinct entries of sets[] that which[] names */
    int32_t pass_queries;     /* queries answered by the shared matrix pass(es) */
    int32_t scan_queries;     /* queries answered by per-set calls of the existing search (a delegated call: all of them;
                                 the queries of an empty set count here) */
    int32_t scan_calls;       /* ... and how many such calls (an empty set makes none) */
    int32_t fallback_queries; /* pass queries re-run exactly */
    int64_t candidates;       /* as ts_search_stats, summed over the blocks of the pass */
} ts_rowsets_stats;

int ts_search_rowsets(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                      const ts_rowset *const *sets, int32_t nsets, const int32_t *which, float *out_scores,
                      int64_t *out_idx, int out_on_device, void *stream, int algo, ts_rowsets_stats *stats);

/* ---- a weight and a row set per query: the citation-weighted search of a batch of sessions in one matrix pass -------
 * ts_search_rowsets for the biased ranking: query q is ranked by fmaf(weights[q], bias[row], score) over the rows
 * sets[which[q]] allows (every row when which[q] == -1).  `bias`: n floats, host or device, one array for the call;
 * `weights`: host memory, nq finite floats.  Output row q is what ts_search_biased_rowset defines for query q alone with
 * weights[q] behind its set (ts_search_biased_ex with no mask for -1): the exact weighted top k of the allowed rows, by
 * weighted score descending, then id ascending, padded with -inf / -1, ids global; rows whose weighted score is NaN (an
 * infinite bias under weight 0, a NaN bias) are ranked as the biased search ranks them.  out_sims (optional) receives the
 * raw similarities, fmaf(-weights[q], bias[row], weighted score), as ts_search_biased.
 *
 * Routing (csrc/biased_rowsets_plan.h holds the rules).  A query's CLASS is the pair (which[q],
 * weights[q] by value):
 *   - all queries in one class: the call IS ts_search_biased_rowset for that set and weight (ts_search_biased_ex for -1), its
 *     paths and its bits;
 *   - otherwise the queries whose set allows at least a tenth of the rows ride ONE pass of the general-width matrix kernel per
 *     256 of them - the weight of the bias term and the mask taken per query, a threshold per query from its own sample rows,
 *     its own weight and a histogram of the raw bias over its set's rows (one histogram per distinct set and call), an exact
 *     re-run behind the query's own set with its own weight for a query the final select rejects - under the conditions of
 *     ts_search_rowsets' pass (index, width, options, more queries than one scan pass serves), when they span at least two
 *     classes;
 *   - every other query is grouped by class, one ts_search_biased_rowset / ts_search_biased_ex call per class under
 *     TS_ALGO_AUTO; a set that allows nothing returns the padding without a launch.
 * algo: TS_ALGO_SCAN runs every class on the scan; TS_ALGO_MFMA is refused with TS_ERR_UNSUPPORTED unless every query rides
 * the pass; a delegated call hands algo on.
 *
 * Score bits follow ts_search_rowsets' promise: on the shared pass they are the general-width kernel's single MFMA chain plus
 * the one fmaf; on a delegated or per-class call they are whatever that call gives.  The exact re-run can cost time, never an
 * answer.
 *
 * TS_ERR_INVALID: NULL bias, NULL weights with nq > 0, a weight that is not finite, and everything ts_search_rowsets rejects.
 * TS_ERR_UNSUPPORTED: a subset index.  nq == 0 does nothing.  A host bias is copied to the device once per split call.  The
 * call waits for its pass; the row sets must stay alive until it returns.  `stats`: ts_rowsets_stats with the same meanings
 * (scan_calls counts the per-class calls). */
int ts_search_biased_rowsets(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                             const float *bias, int bias_on_device, const float *weights, const ts_rowset *const *sets,
                             int32_t nsets, const int32_t *which, float *out_scores, float *out_sims, int64_t *out_idx,
                             int out_on_device, void *stream, int algo, ts_rowsets_stats *stats);

/* ---- grouped search: the k best distinct groups, one row per group ------------------------------------
 * What a user of the search engine ranks is papers and theorems, not rows: a paper contributes tens of rows that lie close
 * together, and theorem_slogan holds several slogans per theorem, which the production query collapses with
 * SELECT DISTINCT ON (ts.theorem_id) before it ranks (streamlit_app.py:254-259, 320-325).  In SQL terms:
 * DISTINCT ON (group) ... ORDER BY group, score DESC, then ORDER BY score DESC LIMIT k - exactly, however large a group is.
 *
 * For query i: take the rows the row set allows (all rows when rows is NULL) whose score is not NaN, in the canonical order
 * (score descending, then global row ascending).  The group of a row is its int32 value in scalar column `col` of `m`; a row
 * whose value is TS_META_NULL is a group of its own (orphans are never merged); every other value, negative ones included,
 * is a group id.  The answer is the first k rows in that order that are the first of their group: each is its group's best
 * row (among equal best scores the lowest row), and the groups come in the order of their best rows.  out_groups (optional,
 * [nq x k]) receives their codes.  Padding is (-inf, -1, TS_META_NULL) when fewer than k groups have an allowed, rankable row.
 *
 * Method: the searches themselves are ts_search_ex / ts_search_rowset, untouched.  Stage 1 searches
 * at depth first = min(TS_MAX_K, max(2 k, k + 16)) and collapses each list to its group-firsts on the device; a list that
 * holds k groups, or padding (the allowed rows are exhausted), is certified: a prefix of the row order determines a prefix of
 * the group order.  Stage 2 searches the other queries again, gathered, at depth deep = TS_MAX_K (TS_ALGO_AUTO unless the
 * caller forced the scan).  Stage 3 serves what is still open one query at a time on the scan, behind a mask without the
 * groups found so far (ts_rowset_exclude's kernel), until k groups are found or no row is left: at most k passes over the
 * corpus per such query - it can cost time, never an answer.  ts_grouped_stats tells what ran.
 *
 * ts_search_grouped waits for its result (the ladder reads the certificates back), with host and with device outputs.  m and
 * rows must have the index's n and device (the rules of ts_search_rowset and ts_index_group_sums); col must be a scalar
 * column that was set; 1 <= k <= TS_MAX_K; TS_ALGO_MFMA is refused exactly where ts_search_ex / ts_search_rowset would refuse
 * stage 1.  Views and attached rows are served, row_offset is honoured; a subset index is TS_ERR_UNSUPPORTED.
 * Not served: the citation-weighted ranking under grouping, sharded indexes (ts_shards_*, ts_comm_*: a sharded caller merges the
 * per-shard grouped results and runs ts_collapse_topk on the merged lists when no group spans shards), subset indexes, bare
 * masks without a row set, and the host-only search (ts_search_cpu).
 *
 * ts_collapse_topk: the collapse step alone, for sorted lists from anywhere.  scores / idx [nq x k_in], each list in the
 * canonical order; column [n] holds the group code of local row id - row_offset; an id outside [row_offset, row_offset + n),
 * or an entry with a NaN score, is padding.  Entry j is kept when its code is TS_META_NULL or no earlier entry of the list has
 * its code; the kept entries are written in order into k_out slots per query (out_scores, out_idx, out_groups - optional),
 * padded with (-inf, -1, TS_META_NULL).  out_found (optional) [nq]: the group-firsts of the WHOLE list (may exceed k_out);
 * out_complete (optional) [nq]: 1 when found >= k_out or the list held padding - the slots are then the exact answer given
 * that the list was a prefix of the query's row order.  The list is never re-sorted.  on_device: every pointer, column
 * included, is device memory and the work is enqueued on `stream`; else every pointer is host memory and the call waits.
 * 1 <= k_in <= TS_MAX_K, 1 <= k_out, nq >= 0, n >= 0, row_offset >= 0.
 *
 * ts_rowset_exclude: the row set  base AND NOT (code of the row in codes) AND NOT (row in local_rows)  over column col of m
 * ("hide these papers"): a row set like any other.  base may be NULL (every row).  ncodes, nrows in [0, 256]; a code equal to
 * TS_META_NULL or a row outside [0, n) is TS_ERR_INVALID; the lists need not be sorted or unique (the call sorts its copies).
 * Waits for the count, as ts_meta_eval does.
 *
 * ts_group_depth: first and deep of the ladder for k (each pointer may be NULL); needs no device. */
typedef struct ts_grouped_stats {
    int32_t algo;             /* path of stage 1: TS_ALGO_SCAN or TS_ALGO_MFMA */
    int32_t depth;            /* first depth used */
    int32_t deep_queries;     /* queries that entered stage 2 */
    int32_t excluded_queries; /* queries that entered stage 3 */
    int32_t exclusion_passes; /* scan passes run in stage 3, all queries */
} ts_grouped_stats;

int ts_search_grouped(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                      ts_meta *m, int32_t col, const ts_rowset *rows, float *out_scores, int64_t *out_idx,
                      int32_t *out_groups, int out_on_device, void *stream, int algo, ts_grouped_stats *stats);
int ts_collapse_topk(int device, const float *scores, const int64_t *idx, int32_t nq, int32_t k_in, int32_t k_out,
                     const int32_t *column, int64_t n, int64_t row_offset, float *out_scores, int64_t *out_idx,
                     int32_t *out_groups, int32_t *out_found, int32_t *out_complete, int on_device, void *stream);
int ts_rowset_exclude(ts_meta *m, int32_t col, const ts_rowset *base, const int32_t *codes, int32_t ncodes,
                      const int64_t *local_rows, int32_t nrows, ts_rowset **out, void *stream);
int ts_group_depth(int32_t k, int32_t *first, int32_t *deep);

/* Rank of one given row per query in the canonical order of that query's scores over the whole index (0 = best):
 * the number of rows whose (score, -row) beats the target's.  One streaming pass that counts; replaces ranking the
 * full [nq x N] matrix and looking the relevant document up - np.argsort(-sim_matrix) followed by the position of
 * the exact document in mrr_at_k with k=None (compare_embeddings.py:96-123) - for corpora whose score matrix
 * does not fit.  target_rows are global ids (row_offset applies); out_rank[i] = -1 and out_score[i] = NaN when
 * the row is not in this index or its score is NaN.  Host pointers; out_score may be NULL. */
int ts_rank_of(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, const int64_t *target_rows,
               int64_t *out_rank, float *out_score, void *stream);

/* Ranks of many target rows per query in the same canonical order (score descending, global row ascending): the number of
 * rows whose (score, -row) beats the target's.  Query i's targets are target_rows[target_offsets[i] .. target_offsets[i+1]).
 * out_rank / out_score are aligned with target_rows; -1 / NaN for rows outside this index or with a NaN score.
 * A list may be empty and may repeat a row (repeats share one rank).  Target rows are global ids (row_offset applies);
 * subset indexes are refused.  Queries are prepared as ts_search prepares them.  Host pointers; out_score may be NULL.
 * bf16 and fp32 indexes at every d that is a multiple of 64 from 128 up to a 4,096-byte row (bf16 up to d = 2048, fp32 up to
 * d = 1024), and at every d that is a multiple of 256 with a wider row of up to 16,384 bytes (bf16 d = 2304 .. 8192, fp32
 * d = 1280 .. 4096: the k-chunked form of the pass; the option "TS_MFMA_GRID" sets the workgroups of its counting launch):
 * one matrix pass over the corpus per block of 256 queries and per 16 targets of the longest list (a gather launch
 * computes the targets' scores by the same arithmetic first; at the k-chunked widths a score has the bits the batched search
 * returns for the row).  Other widths (d = 64, widths that are no multiple of 64, rows wider than 4,096 bytes whose d is no
 * multiple of 256): one ts_rank_of pass per target column - correct and slow.
 * Arithmetic contract: the ranks are consistent with the scores returned here (distinct targets of one query have
 * distinct ranks, ordered by (score, -row)).  Where the fp64 truth cannot separate a target from its neighbours, a rank may
 * differ from ts_rank_of's and from the search paths' positions by the count of those neighbours. */
int ts_rank_many(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq,
                 const int64_t *target_offsets, const int64_t *target_rows,
                 int64_t *out_rank, float *out_score, void *stream);

/* The sharded form of ts_rank_of: how many rows of THIS index rank before a document with the given score and global id
 * (score descending, global id ascending), wherever that document lives.  The shard that holds the document gets its
 * score from ts_rank_of; the sum of ts_count_above over all shards is the document's rank in the whole corpus (the
 * document itself never counts).  out_counts[i] = -1 for a NaN score.  Host pointers. */
int ts_count_above(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq, const float *target_scores,
                   const int64_t *target_ids, int64_t *out_counts, void *stream);

/* The many-targets form of ts_count_above, and the sharded form of ts_rank_many: for query i and each of its targets t in
 * [target_offsets[i], target_offsets[i+1]), out_counts[t] = the number of rows of THIS index that rank before a document with
 * score target_scores[t] and global id target_ids[t] (score descending, then global id ascending).  The document may be a row
 * of this index (it never counts itself) or lie before or behind it.  out_counts[t] = -1 for a NaN score.  A list may be
 * empty, longer than 16 (several passes) and may repeat a document.  Host pointers; subset indexes are refused; the argument
 * checks are those of ts_rank_many.
 * At the widths ts_rank_many's matrix pass serves: one counting pass per block of 256 queries and per 16 targets of the
 * longest list, no gather launch (the keys are made on the host).  Other widths: one ts_count_above per target column.
 * Contract: summed over the shards of a corpus, the counts are the document's rank in the whole corpus, given that the score
 * handed in is the one ts_rank_many returned for the document on the shard that owns it, and that all shards share storage
 * type and width - every shard then scores its rows by the same arithmetic (matrix pass or scan) as the owner scored the
 * document. */
int ts_count_above_many(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq,
                        const int64_t *target_offsets, const float *target_scores, const int64_t *target_ids,
                        int64_t *out_counts, void *stream);

/* Full [nq x n] fp32 score matrix (small N only): util.cos_sim(q_emb, s_emb) of
 * compare_embeddings.py:24,61.  out row stride is n. */
int ts_scores(ts_index *ix, const void *queries, int q_dtype, int q_on_device, int32_t nq,
              float *out, int out_on_device, void *stream);

/* ---- moments of the stored rows -----------------------------------------------------------------------
 * What a PCA over the whole table needs (experiments/pca_plotting.py streams the table out of Postgres twice for it), from the
 * rows where they lie in HBM (a sums pass and a Gram pass): the host side is a d x d eigenproblem (theoremsearch_amd/pca.py).
 *
 * ts_index_moments: count, column sums and Gram matrix X^T X of the STORED rows (what the kernels multiply: normalised for
 * metric cos, rounded for bf16) over all rows, or over the rows a row set allows (rows may be NULL).  out_sum [d] and
 * out_gram [d x d] (row-major, full and symmetric: out_gram[i][j] and out_gram[j][i] are the same bits) are host doubles;
 * out_gram may be NULL (sums and count only).
 * ts_index_group_sums: count and column sums per code of scalar column `col` of `m`: a row whose int32 value v satisfies
 * 0 <= v < ngroups goes to group v; TS_META_NULL and every other value go nowhere.  out_counts [ngroups], out_sums
 * [ngroups x d], host.
 *
 * Served: bf16 and fp32 indexes (owned, attached, views, subsets), d a multiple of 64 in [128, 1024], 1 <= ngroups <= 256;
 * anything else TS_ERR_UNSUPPORTED.  TS_ERR_INVALID for NULL arguments, a list column or a column never set, and a row set or a
 * meta table with another n or on another device (the rules of ts_search_rowset).  n = 0 or a row set that allows nothing:
 * count 0 and zeros.  A row the row set disallows, and the padding past n, contribute nothing whatever their bytes are (NaN
 * and Inf included), and so do the rows of ts_index_group_sums whose code goes nowhere; a non-finite value in a row that counts
 * propagates as it does in numpy (NaN / Inf in every sum and product that row's column takes part in) - with one difference in
 * ts_index_group_sums: the row multiplies every group's indicator, 0 x NaN is NaN, so that column is non-finite in EVERY
 * group's sum, not only in the row's own.  Products are added in fp32 over at most L = 8,192 consecutive rows and those
 * sums in double, in a fixed order: |error| <= (L + 2) 2^-23 sum_r |x_ri x_rj| per element, and the same bits on every call
 * with the same index and arguments.  Counts are integers.  Both calls wait for their result.  Moments are additive: those
 * of a sharded corpus are the sums over its shards.
 * ts_moments_plan: the constants of that pass for tests and tools - L, the panel width, and for (dtype, d, n, cu_count) the
 * number of row ranges and the bytes of the partial tiles (each pointer may be NULL); needs no device. */
int ts_index_moments(ts_index *ix, const ts_rowset *rows, int64_t *out_count, double *out_sum, double *out_gram, void *stream);
int ts_index_group_sums(ts_index *ix, const ts_meta *m, int32_t col, int32_t ngroups, const ts_rowset *rows,
                        int64_t *out_counts, double *out_sums, void *stream);
int ts_moments_plan(int32_t dtype, int32_t d, int64_t n, int32_t cu_count, int32_t *flush_rows, int32_t *panel,
                    int32_t *ranges, int64_t *partial_bytes);

/* Merge `nparts` partial top-k lists per query (e.g. the all-gathered per-shard results,
 * SURVEY.md section 8e) into the global top-k_out under the same ordering rule.
 * scores/idx: [nparts x nq x k_in]; entries with idx < 0 are padding. */
int ts_merge_topk(int device, const float *scores, const int64_t *idx, int32_t nparts, int32_t nq,
                  int32_t k_in, int32_t k_out, float *out_scores, int64_t *out_idx, int on_device,
                  void *stream);

/* The same for results that were exchanged as one packed block per part (one all-gather instead of
 * two): part p starts at packed + p * part_stride_bytes and holds its scores [nq x k_in] float at
 * offset 0 and its ids [nq x k_in] int64 at idx_offset_bytes (a multiple of 8).  Device memory only;
 * enqueued on `stream`. */
int ts_merge_topk_packed(int device, const void *packed, int64_t part_stride_bytes, int64_t idx_offset_bytes,
                         int32_t nparts, int32_t nq, int32_t k_in, int32_t k_out, float *out_scores,
                         int64_t *out_idx, void *stream);

/* ---- row-sharded search over RCCL (BASELINE.json configs[3]) -------------------------------
 * The corpus row-shards over the GPUs of one node: GPU g holds rows [g N / G, (g+1) N / G) in its own ts_index whose
 * row_offset makes the ids global; every GPU searches its shard for the (replicated) query batch; ONE ncclAllGather
 * over xGMI exchanges the packed per-shard top-k (12 * nq * k bytes per rank) and a merge kernel reduces the G * k
 * candidates per query.  The exchange lives in this library (RCCL bound by dlopen at first use; TS_RCCL_LIB names the
 * file when the process has not loaded one yet): no torch.distributed, no MPI on the search path.
 *
 * ts_comm_*: one member per PROCESS (one process per GPU, the torch.distributed.run model).  Rank 0 calls
 * ts_comm_unique_id and hands the 128 bytes to the other ranks by whatever channel the launcher has (a file, a TCP
 * store); every rank then calls ts_comm_create (collective).  ts_comm_search enqueues on `stream` the local search of
 * `shard`, the all-gather and the merge; every rank receives the global answer (device or host buffers as in
 * ts_search).  ts_comm_allgather is the bare collective on device buffers (recv holds world * bytes). */
typedef struct ts_comm ts_comm;
#define TS_COMM_ID_BYTES 128
int ts_comm_unique_id(void *id_out, int32_t id_bytes);
int ts_comm_create(int device, int32_t world, int32_t rank, const void *id, int32_t id_bytes, ts_comm **out);
int ts_comm_destroy(ts_comm *c);
int ts_comm_info(const ts_comm *c, int32_t *world, int32_t *rank, int32_t *device);
int ts_comm_allgather(ts_comm *c, const void *send_dev, void *recv_dev, int64_t bytes, void *stream);
int ts_comm_search(ts_comm *c, ts_index *shard, const void *queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                   float *out_scores, int64_t *out_idx, int out_on_device, void *stream);

/* ts_shards_*: ONE process drives all the GPUs (ncclCommInitAll, one stream per device) - what a serving process such
 * as the Streamlit app would hold instead of one ts_index.  devices = NULL means 0 .. ngpu-1; a device id may repeat
 * (several shards on one GPU, for rehearsing the path on a one-GPU box: the exchange then uses device copies, RCCL
 * refuses two ranks on one GPU).  ts_shards_upload routes global rows to their shards; ts_shards_shard lends the
 * ts_index of shard g (rows [*lo, *hi)) for device uploads / options / profiling; ts_shards_search takes host queries
 * and returns host results. */
typedef struct ts_shards ts_shards;
int ts_shards_create(int32_t ngpu, const int32_t *devices, int64_t n_total, int32_t d, int dtype, int metric,
                     ts_shards **out);
int ts_shards_destroy(ts_shards *s);
int ts_shards_info(const ts_shards *s, int32_t *ngpu, int64_t *n_total, int32_t *uses_rccl);
int ts_shards_shard(ts_shards *s, int32_t g, ts_index **ix, int64_t *lo, int64_t *hi);
int ts_shards_upload(ts_shards *s, const void *host_rows, int src_dtype, int64_t row0, int64_t nrows);
int ts_shards_search(ts_shards *s, const void *queries, int q_dtype, int32_t nq, int32_t k, float *out_scores,
                     int64_t *out_idx);

/* ---- encoder epilogue ------------------------------------------------
 * Pooling + optional L2 normalisation + cast of a transformer's last hidden state, fused in one kernel that
 * writes straight into a buffer the search (or ts_index_upload_device) consumes - what sentence-transformers
 * does with mean pooling / last-token pooling + F.normalize + .to(dtype) after the forward
 * (SentenceTransformer.encode(..., normalize_embeddings=True): parsed_papers_to_vector_rds/embeddings.py:31-37,
 * ec2/generate_embeddings/embeddings.py:24-30, streamlit_app.py:173).
 * hidden: device [n x seq x d], h_dtype TS_F32 | TS_BF16, dense.  attention_mask: device int64 [n x seq]
 * (1 = token, 0 = padding).  pooling: TS_POOL_MEAN (sum of unmasked tokens / max(count, 1e-9)),
 * TS_POOL_LAST (last unmasked token), TS_POOL_CLS (token 0).  out: device [n x out_ld], out_dtype TS_F32 | TS_BF16. */
#define TS_POOL_MEAN 0
#define TS_POOL_LAST 1
#define TS_POOL_CLS 2
int ts_pool_normalize(int device, const void *hidden, int h_dtype, const int64_t *attention_mask, int64_t n,
                      int32_t seq, int32_t d, int pooling, int normalize, void *out, int out_dtype,
                      int64_t out_ld, void *stream);

/* Residual add + LayerNorm of the encoder, one kernel: out = LayerNorm(a + b) * gamma + beta over rows of d elements
 * (BertSelfOutput / BertOutput of the sentence-transformer the reference loads, compare_embeddings.py:11-12: 25 add +
 * 25 layer_norm launches per BERT-base forward in PyTorch).  a, b, out: device [rows x d] dense; gamma, beta: device [d];
 * all of `dtype` (TS_F32 | TS_BF16), 16-byte aligned; the sum, the mean and the variance are taken in fp32.
 * d a multiple of 8 (bf16) / 4 (fp32), at most 2048 / 1024.  `out` may alias a or b. */
int ts_add_layernorm(int device, const void *a, const void *b, const void *gamma, const void *beta, float eps, int64_t rows,
                     int32_t d, int dtype, void *out, void *stream);

/* The encoder's input layer, one kernel: out[i] = LayerNorm(word[ids[i]] + type[type_ids[i]] + pos[i % seq]) * gamma + beta
 * (BertEmbeddings of the sentence-transformer the reference loads, compare_embeddings.py:11-12: three gathers, two adds and a
 * layer_norm launch per forward in PyTorch).  ids, type_ids: device int64 [tokens] (type_ids may be NULL: row 0); word / pos /
 * type: device tables [n_word | n_pos | n_type][d]; gamma, beta: device [d]; out: device [tokens][d]; all of `dtype`
 * (TS_F32 | TS_BF16), 16-byte aligned; sums, mean and variance in fp32.  d as for ts_add_layernorm.  Ids outside a table are
 * clamped to it. */
int ts_embed_layernorm(int device, const int64_t *ids, const int64_t *type_ids, const void *word, const void *pos, const void *type,
                       int64_t n_word, int64_t n_pos, int64_t n_type, const void *gamma, const void *beta, float eps,
                       int64_t tokens, int32_t seq, int32_t d, int dtype, void *out, void *stream);

/* Self-attention of the encoder for short sequences, one kernel: out = softmax(Q K^T / sqrt(64) + key mask) V per (sequence,
 * head), bf16, straight from the fused query / key / value projection (BertSelfAttention of the sentence-transformer the
 * reference loads, compare_embeddings.py:11-12; a query is one sentence: app_showcase_model.py:92).  qkv: device bf16
 * [batch][seq][3][heads][64] (the output of one GEMM over the concatenated projection weights); attention_mask: device int64
 * [batch][seq], 0 = padding key, or NULL; out: device bf16 [batch][seq][heads * 64].  head_dim must be 64 and seq at most 128
 * (TS_ERR_UNSUPPORTED otherwise: the caller keeps its library attention); up to 64 tokens every score tile of a (sequence, head)
 * is held at once, 65 .. 128 tokens walk the query tiles against K / V fragments held in registers.  Scores and softmax in fp32, probabilities rounded to
 * bf16 for the second product (as flash attention does).  A query row without a single allowed key (a sequence whose mask is
 * all zeros) comes back as zeros (torch's softmax gives NaN there). */
int ts_attention_short(int device, const void *qkv, const int64_t *attention_mask, int32_t batch, int32_t seq, int32_t heads,
                      int32_t head_dim, void *out, void *stream);

/* fp32 attention of the encoder at the reference's fp32 storage (SentenceTransformer(name) without a dtype, streamlit_app.py:55,173),
 * head size 64 / 128 / 256 up to 512 / 256 / 128 tokens: softmax(Q K^T * scale + key mask [+ causal]) V on the exact-fp32 matrix
 * instructions, straight from the stacked projection's output qkv [batch][seq][(q_heads + 2 kv_heads) * head_dim] (query heads, key
 * heads, value heads) to out [batch][seq][q_heads * head_dim]; grouped-query when kv_heads < q_heads.  attention_mask: int64
 * [batch][seq] key mask or NULL.  pieces (may be NULL): also the bf16 pieces [batch * seq][3 * q_heads * head_dim] of the output
 * (ts_split_pieces pattern 0) for the fp32-class GEMM behind it; out may then be NULL (only the pieces are written).  Replaces torch's scaled_dot_product_attention and the four
 * layout copies around it in the three fused forwards.  A query row without a single allowed key (a padding token on the left of
 * a causal sequence, a sequence whose mask is all zeros) comes back as zeros, in out and in pieces. */
int ts_attention_float(int device, const void *qkv, const void *qkv_bias, const int64_t *attention_mask, int32_t batch, int32_t seq,
                       int32_t q_heads, int32_t kv_heads, int32_t head_dim, int causal, float scale, void *out, void *pieces, void *stream);
/* The same operation as ts_attention_float - arguments, layouts, masks, bias, pieces - without its V^T-fits-LDS limit: V^T passes
 * through two LDS buffers in chunks of 128 / 64 / 32 keys (head size 64 / 128 / 256) under a workgroup per (sequence, query head,
 * 64 queries), and every (query tile, key tile) step is ts_attention_float's arithmetic in the same order: wherever both serve a
 * shape, out and pieces are the same bits.  Serves head sizes 64 / 128 / 256 at any seq from 1 to 32,768 with
 * batch * q_heads * ceil(seq / 64) <= 2^31 - 1 (TS_ERR_UNSUPPORTED otherwise).  A query row without a single allowed key (a
 * padding token on the left of a causal sequence, a sequence whose mask is all zeros, a whole chunk of padding in front of it)
 * comes back as zeros, in out and in pieces. */
int ts_attention_tiled(int device, const void *qkv, const void *qkv_bias, const int64_t *attention_mask, int32_t batch, int32_t seq,
                       int32_t q_heads, int32_t kv_heads, int32_t head_dim, int causal, float scale, void *out, void *pieces, void *stream);
/* The same for the decoder-style encoder the production app embeds with (Qwen/Qwen3-Embedding-0.6B, streamlit_app.py:55;
 * Qwen3Attention: grouped-query, causal, head size 128): out = softmax(Q K^T / sqrt(128) + causal + key mask) V per (sequence,
 * query head); query head h reads key / value head h / (q_heads / kv_heads).  qkv: device bf16 [batch * seq][(q_heads + 2 kv_heads)
 * * 128] - query heads, key heads, value heads of each token, the output of one GEMM over the stacked projection weights after
 * ts_qk_norm_rope; attention_mask: device int64 [batch][seq], 0 = padding key, or NULL; out: device bf16 [batch * seq][q_heads * 128].
 * head_dim must be 128 and seq at most 128 (TS_ERR_UNSUPPORTED otherwise: the caller keeps its library attention); up to 64
 * tokens every score tile of a (sequence, head) is held at once, 65 .. 128 tokens walk the query tiles against K fragments held in
 * registers and a V^T image in LDS.  A query row
 * without a single allowed key (a padding token on the left of a causal sequence) comes back as zeros. */
int ts_attention_gqa(int device, const void *qkv, const int64_t *attention_mask, int32_t batch, int32_t seq, int32_t q_heads,
                    int32_t kv_heads, int32_t head_dim, int causal, void *out, void *stream);
/* bf16 attention at any length: out = softmax(Q K^T * scale + key mask [+ causal]) V for head sizes 64 / 128 / 256, grouped-query when
 * kv_heads < q_heads (query head h reads key / value head h / (q_heads / kv_heads)), at any seq from 1 to 32,768 with
 * batch * q_heads * ceil(seq / 64) <= 2^31 - 1 (TS_ERR_UNSUPPORTED otherwise).  qkv: device bf16 [batch][seq][(q_heads + 2 kv_heads)
 * * head_dim] - query heads, key heads, value heads of each token, the stacked projection's output (ts_attention_short's
 * [batch][seq][3][heads][64] is the same memory with q_heads = kv_heads = heads); attention_mask: device int64 [batch][seq], 0 =
 * padding key, or NULL; out: device bf16 [batch][seq][q_heads * head_dim]; both 16-byte aligned; scale > 0.  Flash-style: a workgroup
 * per (sequence, query head, 64 queries) walks K and V in chunks of 128 / 64 / 32 keys through LDS; per chunk fp32 scores on the bf16
 * matrix instructions, a running maximum and sum in fp32 (rescaled at every chunk), the unnormalised probabilities rounded to bf16
 * (to nearest even) for the second product, fp32 accumulation, one division at the end.  ts_attention_short / ts_attention_gqa
 * round the normalised probabilities: the entries agree within their rounding bounds, not bit for bit.  A query row without a
 * single allowed key (a padding token on the left of a causal sequence, a sequence whose mask is all zeros, a whole chunk of
 * padding in front of it) comes back as zeros. */
int ts_attention_flash(int device, const void *qkv, const int64_t *attention_mask, int32_t batch, int32_t seq, int32_t q_heads,
                      int32_t kv_heads, int32_t head_dim, int causal, float scale, void *out, void *stream);
/* ts_attention_flash / ts_attention_tiled with a sliding window (Gemma3's local layers): query q reads key k only if
 * |q - k| < window, and the key mask allows k, and k <= q under causal - transformers' convention on both sides; positions are
 * token indices within the sequence.  Every other argument, layout, refusal and the arithmetic are the parent entry's; window < 1
 * is TS_ERR_INVALID.  The same kernels walk only the chunks of 128 / 64 / 32 keys (aligned to multiples of the chunk from key 0)
 * that hold a key some query of the workgroup's 64 may read, so the result is the parent entry's under the equivalent key mask,
 * bit for bit, in less time; window >= seq hides nothing, launches the parent's kernel and returns its bits.  A query row without a
 * single allowed key comes back as zeros. */
int ts_attention_flash_window(int device, const void *qkv, const int64_t *attention_mask, int32_t batch, int32_t seq, int32_t q_heads,
                              int32_t kv_heads, int32_t head_dim, int causal, int32_t window, float scale, void *out, void *stream);
int ts_attention_tiled_window(int device, const void *qkv, const void *qkv_bias, const int64_t *attention_mask, int32_t batch,
                              int32_t seq, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int causal, int32_t window,
                              float scale, void *out, void *pieces, void *stream);

/* The decoder-style encoder the production app embeds with (Qwen/Qwen3-Embedding-0.6B, streamlit_app.py:55;
 * ec2/generate_embeddings/embedders.py:1-4): RMSNorm, rotary positions, grouped-query attention, gated MLP.  Three kernels for
 * what its layers do around the GEMMs; each follows the roundings of the torch modules it replaces.
 *
 * ts_add_rmsnorm: s = a + b (rounded to `dtype`; b may be NULL: s = a), out_norm = gamma * round(s * rsqrt(mean(s^2) + eps))
 * over rows of d elements (Qwen3DecoderLayer's residual add followed by the next Qwen3RMSNorm); out_sum (may be NULL) receives
 * s, the new residual.  d as for ts_add_layernorm; buffers 16-byte aligned; out_sum may alias a or b. */
int ts_add_rmsnorm(int device, const void *a, const void *b, const void *gamma, float eps, int64_t rows, int32_t d, int dtype,
                   void *out_sum, void *out_norm, void *stream);
/* Per-head RMSNorm of queries and keys + rotary position embedding, in place on the fused projection's output
 * (Qwen3Attention: q_norm / k_norm over the head, apply_rotary_pos_emb).  qkv: device [tokens][(q_heads + 2 kv_heads) * 128]
 * (query heads, key heads, value heads; values untouched); q_weight, k_weight: device [128]; cos_table, sin_table: device
 * [seq][128] of `dtype` (fp32 angles cast to the model's type, as Qwen3RotaryEmbedding does); token t has position t % seq.
 * head_dim must be 128 (TS_ERR_UNSUPPORTED otherwise). */
int ts_qk_norm_rope(int device, void *qkv, const void *q_weight, const void *k_weight, const void *cos_table, const void *sin_table,
                    float eps, int64_t tokens, int32_t seq, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int dtype,
                    void *stream);
/* fp32 values as bf16 pieces for an fp32-class GEMM on the bf16 matrix pipe (encoder forward at the reference's fp32 storage,
 * streamlit_app.py:55,173): hi = bf16(x), lo = bf16(x - hi); out [rows x 3k] bf16 = [hi | lo | hi] (pattern 0, activations) or
 * [hi | hi | lo] (pattern 1, weights), so that ONE bf16 GEMM with fp32 accumulation over depth 3k yields
 * x_hi w_hi + x_lo w_hi + x_hi w_lo - the fp32 product up to ~2^-17 |x||w| per term.  x fp32 [rows x k], k a multiple of 4. */
int ts_split_pieces(int device, const void *x, int64_t rows, int32_t k, int pattern, void *out, void *stream);
/* The producers of the encoder forward writing the pieces of their fp32 output themselves ([hi | lo | hi], 3 d bf16 per row), next
 * to the fp32 output the residual path needs: the GEMM that follows reads them without a ts_split_pieces pass in between.  Same
 * arithmetic as ts_add_layernorm / ts_add_rmsnorm / ts_gemma_norm with dtype TS_F32.  a_bias / bias / qkv_bias (each may be NULL): the
 * bias of the GEMM that produced the input, added on the way in - that GEMM then runs without one (torch.addmm with an output type
 * copies the broadcast bias into its result before the GEMM: one more pass over the output per GEMM). */
int ts_add_layernorm_pieces(int device, const void *a, const void *a_bias, const void *b, const void *gamma, const void *beta, float eps,
                            int64_t rows, int32_t d, void *out, void *pieces, void *stream);
int ts_add_rmsnorm_pieces(int device, const void *a, const void *b, const void *gamma, float eps, int64_t rows, int32_t d,
                          void *out_sum, void *out_norm, void *pieces, void *stream);
int ts_gemma_norm_pieces(int device, const void *y, const void *x, const void *w_post, const void *w_next, float eps, int64_t rows,
                         int32_t d, void *out_sum, void *out_norm, void *pieces, void *stream);
/* fp32 activation straight into pieces [rows x 3n]: kind 0 = gelu (erf form) of x [rows x n] (BertIntermediate behind its GEMM + bias);
 * kind 1 = silu(gate) * up, kind 2 = gelu_tanh(gate) * up of x [rows x 2n] (gate columns, then up columns). */
int ts_act_pieces(int device, const void *x, const void *bias, int64_t rows, int32_t n, int kind, void *pieces, void *stream);
/* Gated-MLP activation (Qwen3MLP: SiLU(gate_proj(x)) * up_proj(x)) on the output of ONE GEMM over the stacked gate / up
 * weights: gate_up device [rows][2 * inter] (gate columns, then up columns) -> out device [rows][inter]. */
int ts_swiglu(int device, const void *gate_up, int64_t rows, int32_t inter, int dtype, void *out, void *stream);

/* The reference's second embedder, google/embeddinggemma-300m (ec2/generate_embeddings/embedders.py:1-4; Gemma3TextModel:
 * "sandwich" RMSNorms around every sublayer, q / k norms over heads of 256, rotary positions, GeGLU).  Three kernels for what its
 * layers do around the GEMMs, with the roundings of the torch modules they replace (Gemma3RMSNorm: v * rsqrt(mean(v^2) + eps) *
 * (1 + w) in fp32, rounded once).
 *
 * ts_gemma_norm: s = x + norm(y; w_post) (the residual add in `dtype`; y may be NULL: s = x), out_norm = norm(s; w_next) over rows
 * of d elements - the post-sublayer norm, the residual add and the pre-norm of what follows in one kernel; out_sum (may be NULL)
 * receives s.  d as for ts_add_layernorm; buffers 16-byte aligned. */
int ts_gemma_norm(int device, const void *y, const void *x, const void *w_post, const void *w_next, float eps, int64_t rows,
                  int32_t d, int dtype, void *out_sum, void *out_norm, void *stream);
/* ts_qk_norm_rope for Gemma3Attention: heads of 256, Gemma3RMSNorm (weights q_weight / k_weight [256]), rotate_half at 128;
 * cos / sin: [seq][256] of `dtype` (the layer type's table: sliding and full attention layers use different bases). */
int ts_gemma_qk_norm_rope(int device, void *qkv, const void *q_weight, const void *k_weight, const void *cos_table,
                          const void *sin_table, float eps, int64_t tokens, int32_t seq, int32_t q_heads, int32_t kv_heads,
                          int32_t head_dim, int dtype, void *stream);
/* Gemma3MLP's activation on the fused projection's output: out = gelu_tanh(gate) * up (gate_up [rows][2 * inter]: gate columns,
 * then up columns), the activation rounded to `dtype` before the product as torch does. */
int ts_geglu(int device, const void *gate_up, int64_t rows, int32_t inter, int dtype, void *out, void *stream);

/* ---- kernel timing inside the library ----------------------------------------------------------
 * With profiling enabled, every launch of the dominant kernel of a search (the full-corpus pass of
 * the MFMA path, or the scan kernel) is bracketed by a hipEvent pair on the stream it runs on.
 * ts_index_profile_read waits for the recorded events and returns the number of bracketed launches,
 * their summed duration and the corpus rows one launch covers; it then clears the record. */
int ts_index_profile_enable(ts_index *ix, int enable);
int ts_index_profile_read(ts_index *ix, int64_t *launches, double *total_ms, int64_t *rows_per_launch);

/* Clock probe of the MFMA full pass (diagnostic build of the kernel, selected with option TS_MFMA_VARIANT = 3; timing of
 * that build is not representative): the kernel stamps s_memtime (shader cycles) and s_memrealtime (100 MHz) around its
 * tile loop; this returns the median over workgroups of the last probed launch: in-kernel clock in GHz, shader cycles
 * per unit (32 rows x 384 k), units per workgroup.  Zeros when no probe has run.
 * (MI355X_MICROARCH.md "DVFS give-back" item 6.) */
int ts_index_probe_read(ts_index *ix, double *ghz, double *cycles_per_unit, double *units_per_workgroup);

/* ---- timing on a given stream (hipEvent pairs; bench.py measures kernels with these) ------- */
int ts_timer_create(int device, ts_timer **out);
int ts_timer_start(ts_timer *t, void *stream);
int ts_timer_stop(ts_timer *t, void *stream);
int ts_timer_elapsed_ms(ts_timer *t, float *ms); /* synchronises on the stop event */
int ts_timer_destroy(ts_timer *t);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* TSEARCH_H */
