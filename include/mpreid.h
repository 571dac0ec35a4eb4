/* mpreid.h — C ABI of libmpreid_hip.so: the MI355X (gfx950) implementation of MP-ReID's evaluation
 * hot path.  Plain pointers and sizes only; every pointer named "device" is HBM memory of the
 * current HIP device; every call is ordered on `stream` (a hipStream_t passed as void*).
 *
 * The reference (a pure-Python repo) has no FFI layer; the interface each entry point stands
 * behind is the Python function cited next to it.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add (it is the one mp-reid_amd/mpreid/_lib.py uses).
 *
 * Return value: 0 on success, otherwise a negative mpreid error or a positive hipError_t;
 * mpreid_last_error() returns a thread-local description.  Nothing falls back to the CPU.
 */
#ifndef MPREID_H
#define MPREID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPREID_OK 0
#define MPREID_ERR_ARG (-1)
#define MPREID_ERR_WORKSPACE (-2)
#define MPREID_ERR_UNSUPPORTED (-3)
#define MPREID_ERR_NODEVICE (-4)
#define MPREID_ERR_RETRY_DENSE (-5) /* sparse re-ranking hit a data-dependent capacity: repeat with MPREID_RERANK_DENSE */

/* Environment: the library reads ONE tuning string, MPREID_TUNE="key=value,key=value" (once per process), that selects
 * between BIT-IDENTICAL forms of a stage; no other variable changes which kernel runs.  Keys (default):
 *   gemm_big (1)            0 = never the 256x256 persistent GEMM, 1 = when its grid fills the chip, 2 = whenever divisible
 *   gemm_stagger, gemm_stagger_all (0)   start delay (ticks) of the persistent workgroups
 *   gemm_walk (-1 auto)     tile order inside an XCD's group of 8 tile rows: 0 row-fastest, 1 column-fastest when the output
 *                           has <= 4 tile columns (N = 768: out-proj, FC2), 2 column-fastest always, 3 / 4 groups of 4 / 16 tile
 *                           rows; auto = column-fastest for <= 4 tile columns with operand rows >= 8 KB (the split FC2: -2.4 %);
 *                           groups of 4 rows whenever groups of 8 do not divide among the XCDs but groups of 4 do
 *   gemm_ragged (1)         XCD-owned row groups also when the groups do not divide among the XCDs (>= 24 groups: one XCD gets one
 *                           group less, a short last group leaves unused slots); 0 = round 5's rule (such shapes take the blocked walk)
 *   gemm_grid (0 = all CUs) persistent GEMM workgroups on fewer CUs (experiments: profiles/r06_cu_partition_experiment.log)
 *   dist_sym_p2 (1)         all-pairs distances of ONE tensor (q == g), fp16 modes: 0 = the 256x256 kernel's symmetric form,
 *                           1 = the two-workgroups-per-CU kernel from 16 tile rows on (N >= 3841; one-pass fp16 mode only: the 3-term
 *                           split operands stay on the first), 2 = whenever the padded size allows, 3 = also the 3-term split;
 *                           dist_sym_p2_naps / dist_sym_p2_grid (0): late start of every CU's second workgroup / grid size
 *                           (experiments); dist_sym_p2_abl: ablation variants, -DMPREID_ABLATION builds only
 *   jaccard_wave (-1 auto), jaccard_wave_rows (10240), jaccard_table (0)   form of the Jaccard stage
 *   csc_atomic (0)                       inverted index: the round-1 atomic build
 *   rerank_overlap (-1 auto)             exact query rows in line (0) / on a side stream (1)
 *   wide_sort_lds (4096), wide_jaccard_rows (24576)   WIDE re-ranking: largest neighbour sort held in LDS (larger ones
 *                           use workspace scratch), gallery rows per Jaccard chunk -- same bits either way
 *   pair_blocks (2048)      mpreid_pair_bucket_counts: number of workgroups the launcher aims for -- same counts
 *   verbose (0)             which attention instantiation runs (template arguments, once per device) and occupancy, on stderr;
 *                           which GEMM kernel a launch takes (128x128 / persistent 256x256 -- "(symmetric)" for the stored
 *                           distances of one tensor -- and its tile walk / two workgroups per CU), tiles and grid: one line per
 *                           distinct launch of the process
 * Unknown keys are reported on stderr and ignored.  Switches that change RESULTS exist only in -DMPREID_ABLATION builds. */

typedef void *mpreid_stream_t; /* hipStream_t */

int mpreid_version(void);
/* 1 when the library was compiled with -DMPREID_ABLATION (the timing-ablation switches that skip matrix instructions or
 * stores are honoured: wrong results by design), 0 for the product build.  The Python host refuses an ablation build unless
 * MPREID_ALLOW_ABLATION=1 (mpreid/_lib.py). */
int mpreid_is_ablation_build(void);
const char *mpreid_last_error(void);
/* number of visible HIP devices (0 when there is none); never throws, does not create a context */
int mpreid_device_count(void);
/* name/CU count of the current device */
int mpreid_device_info(char *name, int name_len, int *cu_count, size_t *hbm_bytes);

/* ---- distance path ----------------------------------------------------------------------- */
/* Arithmetic modes of the feat x feat^T GEMM */
#define MPREID_GEMM_F32_EXACT 0 /* v_mfma_f32_32x32x2_f32: k-ascending fmaf chain, bit-reproducible  */
#define MPREID_GEMM_F16_FAST 1  /* fp16 inputs, fp32 accumulate, one pass (|err| ~1e-4 on unit rows)  */
#define MPREID_GEMM_F16_SPLIT3 2 /* x = hi + lo (fp16 pair): hi.hi' + lo.hi' + hi.lo' on the fp16 matrix cores,
                                    fp32 accumulate; |err| <= 1e-6 on unit rows (the exact chain's own rounding
                                    level) -- meets the 1e-5 entry bound, not bit-reproducible against the oracle */

/* squared L2 norm of each row, out[n].  Order of summation is fixed (see oracle/mpreid_oracle.c). */
int mpreid_sqnorm_f32(const float *x_dev, int64_t n, int d, float *out_dev, mpreid_stream_t stream);

/* utils/metrics.py:112-114 — torch.nn.functional.normalize(feats, dim=1, p=2) with eps (1e-12). */
int mpreid_l2_normalize_f32(const float *x_dev, int64_t n, int d, float eps, float *out_dev,
                            mpreid_stream_t stream);

/* utils/metrics.py:7-13 euclidean_distance(qf, gf): out[i*ldo + j] = |q_i|^2 + |g_j|^2 - 2 q_i.g_j
 * q [nq][d], g [ng][d] fp32 row-major; out fp32, leading dimension ldo >= ng (lets a rank write its
 * gallery shard's column block of a wider matrix).  ws: mpreid_distance_workspace_bytes(). */
size_t mpreid_distance_workspace_bytes(int64_t nq, int64_t ng, int d, int mode);
int mpreid_euclidean_distance_f32(const float *q_dev, const float *g_dev, int64_t nq, int64_t ng, int d,
                                  float *out_dev, int64_t ldo, int mode, void *ws_dev, size_t ws_bytes,
                                  mpreid_stream_t stream);
/* utils/metrics.py:15-25 cosine_similarity(qf, gf): arccos(clip(q.g/(|q||g|), -1+1e-5, 1-1e-5)) */
int mpreid_cosine_similarity_f32(const float *q_dev, const float *g_dev, int64_t nq, int64_t ng, int d,
                                 float *out_dev, int64_t ldo, int mode, void *ws_dev, size_t ws_bytes,
                                 mpreid_stream_t stream);

/* ---- k-reciprocal re-ranking, utils/reranking.py:29-100 ------------------------------------ */
typedef struct {
    int64_t n;            /* nq + ng */
    int32_t k1, k2, half_k1;
    int32_t v_cap;        /* ELL row capacity of V before query expansion */
    int32_t vqe_cap;      /* row capacity after query expansion (max union size, measured) */
    int64_t v_nnz;        /* nnz(V) before query expansion */
    int64_t vqe_nnz;      /* nnz(V) after query expansion (== v_nnz when k2 == 1) */
    int64_t jaccard_pairs;/* sum over queries i, columns c in nz(V[i]) of nnz(V[:,c]) */
    int64_t krecip_r_sum; /* sum over rows of |R(i, k1)| (k-reciprocal set sizes before expansion) */
    int64_t fallback_rows;/* sparse algorithm: rows whose candidate list could not be certified (done densely) */
    int64_t cand_total;   /* sparse algorithm: neighbour candidates emitted by the fused GEMM (sum over rows) */
    int32_t algo;         /* MPREID_RERANK_DENSE / _SPARSE / _SPARSE_SPLIT3 / _WIDE: what the call actually ran */
    /* filled when timing != 0 (hipEvents on the stream).  DENSE: gemm = N x N exact distances, topk = row maxima +
     * neighbour selection.  SPARSE: gemm = fp16 operands + sample pass + thresholds + fused candidate GEMM, topk =
     * exact refinement + fallback rows, dq = exact distance rows of the queries. */
    float ms_gemm, ms_topk, ms_krecip, ms_qe, ms_csc, ms_jaccard, ms_total, ms_dq;
} mpreid_rerank_stats;

/* Three algorithms, the same bits out (tests/test_gpu_rerank.py, tests/test_gpu_rerank_wide.py):
 *   DENSE   the N x N fp32 distance matrix is computed (exact fp32 MFMA), kept in HBM and scanned for the first
 *           max(k1+1, k2) neighbours of every row.  Any N, local_distmat / only_local supported.
 *   SPARSE  the N x N matrix is never materialised: a one-pass fp16 GEMM on the matrix cores emits, per row, the
 *           ~180 entries that can still be among its neighbours or be its maximum (thresholds from a 1/16 column
 *           sample, a proven error bound), those are re-evaluated with the exact fp32 chain, and the exact distance
 *           rows exist only for the queries ([nq][N], what the Jaccard blend reads).  Rows that cannot be certified
 *           fall back to the dense computation of that row.  Needs N >= 2048, max(k1+1, k2) <= 64, no local_distmat.
 *   AUTO    SPARSE when it applies, else DENSE.  A sparse call may return MPREID_ERR_RETRY_DENSE (degenerate data:
 *           too many fallback rows, a query-expansion row above 4096 entries, row norms >= 3e4): repeat it with
 *           MPREID_RERANK_DENSE and a workspace sized for DENSE.  AUTO never chooses WIDE.
 *   WIDE    DENSE's arithmetic for ANY k1 >= 0, k2 >= 1 (clamped against N as numpy slicing clamps them) and any N whose
 *           workspace fits the device: every table whose size grows with k (selection keys, reciprocity positions,
 *           expansion lists, weights, query-expansion accumulators, the Jaccard stage's per-query tables) lives in the
 *           workspace instead of LDS.  local_distmat / only_local supported.  A completeness path: several times slower
 *           than DENSE where both apply (DESIGN.md section 2 has the measured ratio). */
#define MPREID_RERANK_AUTO 0
#define MPREID_RERANK_DENSE 1
#define MPREID_RERANK_SPARSE 2
/* the sparse algorithm with the blend term's distance rows (lambda * d / max, queries x gallery) from the fp16 matrix
 * cores (3-term split, |error| <= 1e-6 on unit-norm features) instead of the exact fp32 chain: neighbour table, V, V_qe
 * and the Jaccard term are bit-identical to the other modes, |final - exact final| <= lambda * 1e-6 / max.  Never chosen
 * by AUTO. */
#define MPREID_RERANK_SPARSE_SPLIT3 3
#define MPREID_RERANK_WIDE 4
/* Bytes of device workspace re_ranking needs for this problem (DENSE: dominated by the N x N fp32 distance matrix,
 * 4*N*N; SPARSE: by the sample distances N*N/4 bytes and the query rows 4*nq*N). */
size_t mpreid_rerank_workspace_bytes(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local);      /* DENSE */
size_t mpreid_rerank_workspace_bytes_ex(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local, int algo);
/* 1 when `algo` accepts this problem, 0 when the call would end with MPREID_ERR_UNSUPPORTED for one of the limits below
 * (or the arguments are invalid).  No side effects, no device needed, the launchers' own expressions: ask it before
 * choosing an algorithm instead of retrying a refused call.  AUTO: SPARSE applies, or DENSE fits. */
int mpreid_rerank_fits(int64_t nq, int64_t ng, int d, int k1, int k2, int has_local, int algo);

/* re_ranking(probFea, galFea, k1, k2, lambda_value, local_distmat=None, only_local=False)
 *   q [nq][d], g [ng][d] fp32 device; local_dev: NULL or [N][N] fp32 device (N = nq+ng);
 *   out_dev [nq][ldo] fp32 receives final_dist[:nq, nq:]  (ldo >= ng).
 * lambda is a double because the reference rounds (1 - lambda) from a Python float straight to
 * float16 and lambda to float32.  The call synchronises `stream` internally (sizes of the sparse
 * structures are read back) and returns after the result is complete.
 * stats may be NULL; with timing != 0 per-stage times are measured with hipEvents on `stream`.
 * Limits (the reference has none, utils/reranking.py:53-54; it is called with k1 = 50, k2 = 15, utils/metrics.py:127).
 * DENSE, SPARSE and AUTO have two (mpreid_rerank_fits answers them without a call):
 *   max(k1 + 1, k2) <= 256 -- the neighbour selection sorts its winners in one 256-entry LDS network and the reciprocity
 *   masks are 256 bits per row -> MPREID_ERR_UNSUPPORTED above that;
 *   the expansion lists of one row live in LDS: 8 * min(N, (k1 + 1) * (1 + ceil(k1 / 2))) + N / 8 + 8 * (k1 + 1) + 2 KB must
 *   fit a workgroup's 160 KB, i.e. k1 <= ~190 at N >= 20 000 (k1 <= 255 for N <= 18 000) -> MPREID_ERR_UNSUPPORTED above
 *   that (a loud failure, never a wrong result).  (Their query-expansion and Jaccard kernels also keep 8 and 14 bytes of
 *   LDS per entry of the LARGEST V_qe row, a data-dependent size: a call inside the two limits whose rows grow past
 *   ~11 000 entries ends with MPREID_ERR_UNSUPPORTED as well.)
 * WIDE has neither: N = nq + ng < 2^31 - 64 and the workspace are its only limits.  Its workspace, with K = min(k1 + 1, N),
 * KR = max(K, min(k2, N)), vcap = min(K * (1 + half_k1), N), qcap = min(N, k2 * vcap) (0 when k2 = 1), fcap = qcap or vcap
 * when k2 = 1, P = KR rounded up to a power of two, W = min(N, 1024) workgroups, every term rounded up to 256 bytes:
 *   4 N d + 4 N + 4 N ld (x 2 with local_distmat; ld = N rounded up to 64) + 4 N            features, norms, D, MT, row max
 *   + 4 N KR + 8 N K + 4 N K + 8 W P (only when P > 4096)                                   neighbour table, index-sorted copy,
 *                                                                                           reciprocity positions, sort scratch
 *   + 8 N + 6 N vcap + 4 W vcap                                                             V rows, weight scratch
 *   + 4 N + 6 N qcap + 4 W N                                                                V_qe rows, accumulator rows
 *   + 12 (N + 1) + 6 ng fcap + 64                                                           inverted index, counters
 * (mpreid_rerank_workspace_bytes_ex(..., MPREID_RERANK_WIDE) returns it: 6.7 GB at N = 20 000, d = 768, k = 50 / 15.)
 * The row-sharded phases below (mpreid_rr_*, mpreid/distributed.py) run the DENSE / SPARSE kernels and keep the two limits.
 *   N = nq + ng < 2^31 - 64. */
/* mpreid_rerank_f32 (+ mpreid_rerank_workspace_bytes, mpreid_rerank_debug_copy) is the DENSE algorithm: it never returns
 * the data-dependent MPREID_ERR_RETRY_DENSE.  mpreid_rerank_f32_ex takes the algorithm (AUTO / SPARSE: faster, may ask for
 * the dense retry with a workspace from mpreid_rerank_workspace_bytes_ex(..., MPREID_RERANK_DENSE)). */
int mpreid_rerank_f32(const float *q_dev, const float *g_dev, int64_t nq, int64_t ng, int d, int k1, int k2,
                      double lambda_value, const float *local_dev, int only_local, float *out_dev,
                      int64_t ldo, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream,
                      mpreid_rerank_stats *stats, int timing);

int mpreid_rerank_f32_ex(const float *q_dev, const float *g_dev, int64_t nq, int64_t ng, int d, int k1, int k2,
                         double lambda_value, const float *local_dev, int only_local, float *out_dev,
                         int64_t ldo, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream,
                         mpreid_rerank_stats *stats, int timing, int algo);

/* debug/inspection taps used by the parity tests: copies of intermediate results of the LAST
 * mpreid_rerank_f32 call that used workspace ws_dev (valid until the workspace is reused).
 *   rank_out [N][k1+1] int32 (initial_rank[:, :k1+1]); v_cnt/vqe_cnt [N] int32 nnz per row. */
int mpreid_rerank_debug_copy(const void *ws_dev, int64_t nq, int64_t ng, int d, int k1, int k2, int has_local,
                             int32_t *rank_out_host, int32_t *v_cnt_host, int32_t *vqe_cnt_host,
                             mpreid_stream_t stream);   /* layout of the DENSE algorithm (mpreid_rerank_f32) */
int mpreid_rerank_debug_copy_ex(const void *ws_dev, int64_t nq, int64_t ng, int d, int k1, int k2, int has_local,
                                int32_t *rank_out_host, int32_t *v_cnt_host, int32_t *vqe_cnt_host,
                                mpreid_stream_t stream, int algo);

/* ---- eval_func ranking, utils/metrics.py:28-88 ---------------------------------------------------------
 * For every query: the 0-based positions, in the ascending (distance, gallery index) order of its row, of the
 * gallery items whose pid equals the query's pid (what the reference reads off np.argsort + matches).
 * pos_out [nq][rcap] int32 ascending, padded with -1; cnt_out [nq] = number of relevant items, or -1 when a
 * query has more than min(rcap, 8192) of them (LIMIT: the sorted relevant keys of a query live in LDS -- the launch sizes
 * its dynamic LDS for rcap rounded up to a power of two, 64 ... 8192 entries; the caller ranks such a row on the host --
 * utils/metrics.py:eval_func_device does -- Market-1501 / MSMT17 queries have at most a few hundred relevant gallery
 * images).  CMC / AP are finished
 * on the host from the positions (float64, numpy's summation order): mp-reid_amd/utils/metrics.py. */
int mpreid_eval_rank_positions(const float *dist_dev, int64_t ld, int nq, int ng, const int64_t *q_pids_dev,
                               const int64_t *g_pids_dev, int rcap, int32_t *pos_out_dev, int32_t *cnt_out_dev,
                               mpreid_stream_t stream);

/* The same under the Market-1501 protocol: for every query the gallery items with the query's pid AND the query's camera
 * are junk and leave the ranking -- the filter the reference's eval_func promises (utils/metrics.py:28-88, docstring
 * :29-31), keeps commented out at line 54, and runs in its other evaluation tail
 * (processor/processor_uniprompt_stage2.py:476-505).  A gallery item is RELEVANT when it has the query's pid and is not
 * junk; its position is the number of KEPT (non-junk) items with a smaller (distance, gallery index) key.
 * pos_out [nq][rcap] int32: the ascending positions of the relevant items among the kept ones, padded with -1;
 * cnt_out [nq] = number of relevant items (0: the query is invalid under the protocol), or -1 when the row exceeds the
 * LDS capacity.  LIMIT: relevant AND junk keys share the sorted list in LDS, so the count that hits min(rcap, 8192) is the
 * number of PID MATCHES of the query (relevant + junk), not the number of relevant items: size rcap from the pid counts,
 * as for mpreid_eval_rank_positions.  The camera ids are read for pid matches only; the pass over the row reads no labels. */
int mpreid_eval_rank_positions_cam(const float *dist_dev, int64_t ld, int nq, int ng, const int64_t *q_pids_dev,
                                   const int64_t *g_pids_dev, const int64_t *q_camids_dev, const int64_t *g_camids_dev,
                                   int rcap, int32_t *pos_out_dev, int32_t *cnt_out_dev, mpreid_stream_t stream);

/* The same for a BATCH of (split, query) pairs over one resident matrix, in one launch -- multi-trial protocols
 * (VehicleID's ten trials, reference test.py:46-63; RegDB; MMMP's exp_setting pairs) evaluate several (query set, gallery
 * set) pairs over one set of images: the pool is encoded once, one pool x pool matrix [n_rows][n_cols] (leading dimension
 * ld >= n_cols) stays on the device and every split reads its sub-matrix through index lists.  Pair b ranks row q_row[b] of
 * the matrix against the columns g_idx[g_off[s] .. g_off[s + 1]) of split s = q_split[b]; the semantics are those of
 * mpreid_eval_rank_positions -- of mpreid_eval_rank_positions_cam when q_camids_dev / g_camids_dev are given (both or
 * neither) -- applied to the gathered row dist[q_row[b]][g_idx[...]].  The tie-break index of an item is its POSITION IN
 * THE SPLIT'S LIST, not its column: the positions equal a stable argsort of the gathered row whatever order the list is in.
 * q_pids / q_camids [nqt] are the pairs' labels; g_pids / g_camids [g_off[n_splits]] are the labels of the list entries,
 * aligned with g_idx (the caller gathers them once: the kernel reads labels coalesced and gathers distances only).
 * pos_out [nqt][rcap], cnt_out [nqt], the -1 padding and the cnt = -1 hand-back (more than min(rcap, 8192) pid matches in
 * the pair's list) are as above; same LDS geometry.  LIMIT: the CONTENTS of q_row (< n_rows), q_split (< n_splits), g_off
 * (ascending from 0) and g_idx (< n_cols) are device data and are NOT checked here: the caller validates them before
 * upload (utils/metrics.py:eval_func_splits_device does). */
int mpreid_eval_rank_positions_splits(const float *dist_dev, int64_t ld, int64_t n_rows, int64_t n_cols, int nqt,
                                      const int32_t *q_row_dev, const int32_t *q_split_dev, const int64_t *q_pids_dev,
                                      const int64_t *q_camids_dev, int n_splits, const int64_t *g_off_dev,
                                      const int32_t *g_idx_dev, const int64_t *g_pids_dev, const int64_t *g_camids_dev,
                                      int rcap, int32_t *pos_out_dev, int32_t *cnt_out_dev, mpreid_stream_t stream);

/* ---- ranked gallery lists: the first k entries of np.argsort(distmat, axis=1), utils/metrics.py:39 ----------
 * For every row i of the resident block dist [nq][ng] (leading dimension ld >= ng; column j is GLOBAL gallery index
 * col0 + j): the first k items in ascending (distance, global index) order -- -0 equal to +0, ties by the smaller index,
 * i.e. np.argsort(row, kind="stable")[:k] of a NaN-free row -- as idx [nq][k] int32 (global indices) and val [nq][k] fp32
 * (the matrix entries' own bits); cnt [nq] = min(k, kept items), entries past it are idx = -1, val = +inf.
 * Labels (all four pointers, or all NULL; g_pids / g_camids [ng] are aligned with the block's columns, the caller offsets
 * them): gallery items with the query's pid AND the query's camera are junk and do not enter the list -- the rule of
 * mpreid_eval_rank_positions_cam.
 * carry != 0: idx / val / cnt hold on entry a valid ascending list built from OTHER columns (cnt entries are taken, whatever
 * the values behind them); the result is the first k of the union of that list and this block, so a gallery of any size
 * is ranked block by block without its nq x ng matrix (mpreid/ops.py:search_topk).  carry == 0: the three are outputs only.
 * Exact for any number of entries equal to the k-th distance (radix select over the 64-bit (distance, index) keys, then
 * an LDS sort of at most 2048 keys: csrc/ranklist.hip); the result does not depend on the order in which atomics arrive.
 * No alignment is assumed of dist_dev, ld or ng (callers pass column slices of wider matrices).
 * MPREID_ERR_ARG: k < 1, nq < 0, ng < 0, only some of the four label pointers, col0 + ng >= 2^31.  LIMIT: k <=
 * MPREID_RANK_TOPK_MAX -> MPREID_ERR_UNSUPPORTED above that; one workgroup per query, so a search with a handful of queries
 * does not fill the chip.  nq == 0, or ng == 0 with carry, is a no-op; ng == 0 without carry writes empty lists. */
#define MPREID_RANK_TOPK_MAX 1024
int mpreid_rank_topk(const float *dist_dev, int64_t ld, int nq, int ng, int64_t col0, int k,
                     const int64_t *q_pids_dev, const int64_t *g_pids_dev,
                     const int64_t *q_camids_dev, const int64_t *g_camids_dev,   /* all four, or all NULL */
                     int carry, int32_t *idx_io_dev, float *val_io_dev, int32_t *cnt_io_dev,
                     mpreid_stream_t stream);

/* ---- query expansion in feature space (AQE on the queries, DBA on the gallery rows; not in the reference) ----------
 * Every output row is the similarity-weighted mean of the rows of src its list names:
 *   kk = cnt[i] clamped to [0, k]; entries past it are ignored
 *   s_j = max(1 - 0.5 * dist[i][j], 0)   fp32, one rounding: the cosine of two unit rows from their squared distance
 *   w_j = 1 when alpha == 0 (also for s_j == 0); s_j multiplied alpha - 1 times, left to right in fp32, when alpha is an
 *         integer 1 ... 8; powf(s_j, alpha) otherwise (that case alone is not bit-defined)
 *   acc = 0; for j = 0 ... kk - 1 in LIST order: acc = fl(acc + fl(w_j * src[idx[i][j]][e])) -- a separate multiply and add
 *   out[i][e] = fl(acc / float(kk)), a true divide; a row with an empty list becomes zeros
 * idx / dist / cnt are exactly what mpreid_rank_topk writes ([rows][k], [rows][k], [rows]) for the all-pairs distances of
 * the L2-NORMALISED rows, while src holds the RAW rows: the normalised copy only chooses the neighbours and the weights
 * (utils/metrics.py:expand_features is the host definition, mpreid/ops.py:expand_features the driver).
 * src [n_src][d] fp32 with leading dimension ld_src, out [rows][d] with ld_out; no alignment beyond 4 bytes is assumed
 * (16-byte loads are used when both pointers and both leading dimensions allow it: the same bits).  One launch, no atomics;
 * an element's bits do not depend on the launch geometry.  rows == 0 is a no-op.
 * MPREID_ERR_ARG: k < 1, d < 1, rows < 0, n_src < 0, ld_src < d, ld_out < d, alpha < 0 or NaN, a null pointer, out overlapping
 * src (other rows still read src).  MPREID_ERR_UNSUPPORTED: k > MPREID_RANK_TOPK_MAX (the list of a row lives in LDS).
 * LIMIT: the CONTENTS of idx (0 <= idx < n_src in the first cnt entries of a row) are device data and are NOT checked here:
 * the lists of mpreid_rank_topk over n_src columns satisfy it. */
int mpreid_qe_aggregate_f32(const float *src_dev, int64_t n_src, int d, int64_t ld_src,
                            const int32_t *idx_dev, const float *dist_dev, const int32_t *cnt_dev,
                            int64_t rows, int k, float alpha,
                            float *out_dev, int64_t ld_out, mpreid_stream_t stream);

/* ---- verification statistics over all query x gallery pairs (not in the reference) ---------------------------------
 * PAIRS: (i, j) with i < nq, j < ng and dist[i][j] finite (NaN and +-inf entries are no pairs).  With the camera ids given
 * (both pointers, or both NULL: no filter) the pairs with g_pids[j] == q_pids[i] and g_camids[j] == q_camids[i] are dropped
 * -- the junk of mpreid_eval_rank_positions_cam.  A kept pair is POSITIVE iff the pids are equal, NEGATIVE otherwise; every
 * query contributes, with or without a positive.
 * ORDER: distances compare through the 32-bit key u = bits(d + 0.0f); key = u >= 2^31 ? ~u : u | 2^31 -- the upper half
 * of the ranking key of the kernels above: ascending distance, -0 equal to +0.
 * COUNTS: bound_keys [n_bounds] are strictly ascending keys; the bucket of a kept pair is the number of bounds smaller than
 * its key (0 ... n_bounds), so bucket b holds the pairs with bound[b-1] < key <= bound[b] and the inclusive prefix sums over
 * the buckets are tp[b] / fp[b] = number of positive / negative pairs with d <= t_b.  counts [2][n_bounds + 1] u64:
 * positive row, then negative row.  accumulate == 0 zeroes counts first (stream-ordered); accumulate != 0 adds, so column
 * blocks of a matrix that is never held whole sum exactly.  Integer sums: the result does not depend on the launch
 * geometry or on the order of the atomics.  ROC curves, TPR at a false-positive budget and the distance histograms are
 * sums and differences of these counts (utils/metrics.py: pair_counts / tpr_at_fpr; mpreid/ops.py: pair_select).
 * One pass over the matrix, tiled in both directions (csrc/pairstats.hip); stream-ordered, no host synchronisation.
 * No alignment is assumed of dist_dev or ld (16-byte loads when both allow it, 4-byte loads otherwise: the same counts).
 * nq == 0 or ng == 0: zero counts (unless accumulating), no launch.
 * MPREID_ERR_ARG: n_bounds < 1 or > MPREID_PAIR_BOUNDS_MAX, exactly one camera pointer NULL, ld < ng, nq < 0, ng < 0, a
 * null bounds / counts pointer.  MPREID_ERR_UNSUPPORTED: more than 2^31 - 1 tiles of the grid.
 * LIMIT: the CONTENTS of bound_keys (strictly ascending) are device data and are NOT checked here: the caller validates
 * them before upload (mpreid/ops.py:pair_bucket_counts does). */
#define MPREID_PAIR_BOUNDS_MAX 4096
int mpreid_pair_bucket_counts(const float *dist_dev, int64_t ld, int nq, int ng,
                              const int64_t *q_pids_dev, const int64_t *g_pids_dev,
                              const int64_t *q_cams_dev, const int64_t *g_cams_dev,   /* both NULL: no filter */
                              const uint32_t *bound_keys_dev, int n_bounds,            /* strictly ascending keys */
                              int accumulate, unsigned long long *counts_dev,          /* [2][n_bounds + 1] */
                              mpreid_stream_t stream);

/* ---- row-sharded re-ranking: the same kernels, phase by phase over a row range ------------
 * Rows [r_lo, r_lo+rows) of the N x N problem belong to the calling rank; between the phases the caller
 * all-gathers (RCCL) the rank table, the sparse V rows and the sparse V_qe rows.  mpreid/distributed.py
 * (re_ranking_sharded) is the driver; results do not depend on the number of ranks. */
/* phase 1: D rows + row maxima (+ first kr neighbours when rank_local != NULL); norms_all = mpreid_sqnorm_f32 */
int mpreid_rr_dist_rows(const float *feat_all_dev, const float *norms_all_dev, int64_t n, int d, int64_t r_lo,
                        int64_t rows, float *d_local_dev, int64_t ld, float *rowmax_local_dev,
                        int32_t *rank_local_dev, int kr, mpreid_stream_t stream);
/* ELL row capacity of V before query expansion: min(N, (k1+1)*(1+half_k1)) */
int mpreid_rr_vcap(int64_t n, int k1);
/* phase 2: V rows (ELL, row stride mpreid_rr_vcap) of the local rows from the global rank table [N][kr] */
/* scratch_dev: mpreid_rr_krecip_scratch_bytes(n) bytes (reciprocity bits of all n rows of the table) */
size_t mpreid_rr_krecip_scratch_bytes(int64_t n);
int mpreid_rr_krecip(const float *d_local_dev, int64_t ld, int64_t n, const float *rowmax_local_dev,
                     const int32_t *rank_all_dev, int k1, int kr, int64_t r_lo, int64_t rows, int32_t *vcnt_dev,
                     int32_t *vidx_dev, uint16_t *vval_dev, void *scratch_dev, mpreid_stream_t stream);
/* SPARSE forms of phases 1 and 2 (no [rows][n] distance block; n >= 2048, kr <= 64): phase 1 returns the first kr
 * neighbours, the row maxima and the exact distances of the neighbours of the local rows; MPREID_ERR_RETRY_DENSE
 * (degenerate data) means "use mpreid_rr_dist_rows + mpreid_rr_krecip for this row block" -- every rank may decide
 * for itself, the bits are the same.  The Jaccard phase is mpreid_rr_jaccard as before. */
size_t mpreid_rr_sparse_workspace_bytes(int64_t n, int d, int64_t rows, int kr);
int mpreid_rr_neighbours_sparse(const float *feat_all_dev, const float *norms_all_dev, int64_t n, int d, int64_t r_lo,
                                int64_t rows, int kr, int32_t *rank_local_dev, float *rowmax_local_dev,
                                float *rankd_local_dev, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);
int mpreid_rr_krecip_sparse(const float *feat_all_dev, const float *norms_all_dev, int64_t n, int d,
                            const float *rowmax_local_dev, const int32_t *rank_all_dev, const float *rankd_local_dev,
                            int k1, int kr, int64_t r_lo, int64_t rows, int32_t *vcnt_dev, int32_t *vidx_dev,
                            uint16_t *vval_dev, void *scratch_dev, mpreid_stream_t stream);
/* re-stride ELL rows (for the all-gather: common width = global max count) */
int mpreid_rr_pack_rows(const int32_t *cnt_dev, const int32_t *idx_dev, const uint16_t *val_dev, int64_t rows,
                        int src_stride, int dst_stride, int32_t *idx_out_dev, uint16_t *val_out_dev,
                        mpreid_stream_t stream);
/* CSR transport of sparse rows (what the all-gathers of V and V_qe move: nnz entries of 6 bytes instead of rows x the
 * global maximum row length): rowptr [rows + 1] = exclusive prefix sums of cnt; ell_to_csr packs the first cnt[r] entries of
 * every ELL row back to back; csr_to_ell is the inverse (entries past cnt[r] of the ELL rows are left untouched). */
int mpreid_rr_rowptr(const int32_t *cnt_dev, int64_t rows, long long *rowptr_dev, mpreid_stream_t stream);
int mpreid_rr_ell_to_csr(const long long *rowptr_dev, const int32_t *idx_dev, const uint16_t *val_dev, int64_t rows, int stride,
                         int32_t *idx_out_dev, uint16_t *val_out_dev, mpreid_stream_t stream);
int mpreid_rr_csr_to_ell(const long long *rowptr_dev, const int32_t *idx_dev, const uint16_t *val_dev, int64_t rows, int stride,
                         int32_t *idx_out_dev, uint16_t *val_out_dev, mpreid_stream_t stream);
/* phase 3: local query expansion of the local rows from the global V (row stride vstride) */
int mpreid_rr_qe_count(int64_t n, const int32_t *rank_all_dev, int kr, int k2, int64_t r_lo, int64_t rows,
                       const int32_t *vcnt_all_dev, const int32_t *vidx_all_dev, int vstride,
                       int32_t *ucnt_local_dev, mpreid_stream_t stream);
int mpreid_rr_qe_fill(int64_t n, const int32_t *rank_all_dev, int kr, int k2, int64_t r_lo, int64_t rows,
                      const int32_t *vcnt_all_dev, const int32_t *vidx_all_dev, const uint16_t *vval_all_dev,
                      int vstride, int qcap, int32_t *qcnt_local_dev, int32_t *qidx_local_dev,
                      uint16_t *qval_local_dev, mpreid_stream_t stream);
/* phase 4: inverted index of the global V_qe + Jaccard / blend for query rows [q_lo, q_lo+qrows);
 * out [qrows][ldo] = final_dist[q_lo : q_lo+qrows, nq:].  Scratch: ccnt [N+1] u32, cptr [N+1] i64,
 * crow / cval [sum of qcnt_all]. */
/* chist_dev: NULL (atomic build of the inverted index) or mpreid_rr_jaccard_hist_bytes(n) bytes: block histograms of the
 * atomics-free build, which also lets the Jaccard kernel gather exact column sub-ranges per row chunk */
size_t mpreid_rr_jaccard_hist_bytes(int64_t n);
int mpreid_rr_jaccard(int64_t n, int64_t nq, int64_t q_lo, int64_t qrows, const float *d_q_dev, int64_t ld,
                      const float *rowmax_q_dev, const int32_t *qcnt_all_dev, const int32_t *qidx_all_dev,
                      const uint16_t *qval_all_dev, int qstride, double lambda_value, uint32_t *ccnt_dev,
                      long long *cptr_dev, int32_t *crow_dev, uint16_t *cval_dev, uint32_t *chist_dev, float *out_dev,
                      int64_t ldo, mpreid_stream_t stream);
/* phase 4 with the inverted-index BUILD sharded by column range over the ranks (utils/reranking.py:80-82 is the build,
 * :84-93 the Jaccard loop): mpreid_rr_jaccard builds the whole index on every rank; here rank r
 *   1. mpreid_rr_csc_count: counts the indexed entries (rows [nq, n)) of its columns [c_lo, c_hi) -> ccnt[c_lo .. c_hi);
 *      chist (mpreid_rr_jaccard_hist_bytes(n) bytes) keeps per-block offsets for step 2          -> ALL-GATHER ccnt [n] u32
 *   2. mpreid_rr_csc_fill: cptr [n + 1] = exclusive scan of the gathered counts (ccnt_all is consumed), the packed entries of
 *      its columns at their GLOBAL positions cpk[cptr[c_lo] .. cptr[c_hi]) (cpk: cptr[n] u32 words) and the rows
 *      [c_lo, c_hi) of the chunk-boundary table hb [n][mpreid_rr_csc_chunks(n, nq) + 1] u32
 *                                                       -> ALL-GATHER the cpk pieces (contiguous, rank order) and the hb rows
 *   3. mpreid_rr_jaccard_indexed: Jaccard + blend of the rank's queries over the assembled index.
 * Needs n * qstride < 2^32 and at least one indexed row (0 <= nq < n): all three entry points check both and return
 * MPREID_ERR_ARG otherwise (mpreid_rr_csc_chunks returns the chunk count, > 0, or that negative code).
 * Bit-identical to mpreid_rr_jaccard for any number of column shards. */
int mpreid_rr_csc_chunks(int64_t n, int64_t nq);
int mpreid_rr_csc_count(int64_t n, int64_t nq, const int32_t *qcnt_all_dev, const int32_t *qidx_all_dev, int qstride,
                        int64_t c_lo, int64_t c_hi, uint32_t *chist_dev, uint32_t *ccnt_dev, mpreid_stream_t stream);
int mpreid_rr_csc_fill(int64_t n, int64_t nq, const int32_t *qcnt_all_dev, const int32_t *qidx_all_dev,
                       const uint16_t *qval_all_dev, int qstride, int64_t c_lo, int64_t c_hi, uint32_t *ccnt_all_dev,
                       uint32_t *chist_dev, long long *cptr_dev, uint32_t *cpk_dev, uint32_t *hb_dev, mpreid_stream_t stream);
int mpreid_rr_jaccard_indexed(int64_t n, int64_t nq, int64_t q_lo, int64_t qrows, const float *d_q_dev, int64_t ld,
                              const float *rowmax_q_dev, const int32_t *qcnt_all_dev, const int32_t *qidx_all_dev,
                              const uint16_t *qval_all_dev, int qstride, double lambda_value, const long long *cptr_dev,
                              const uint32_t *cpk_dev, const uint32_t *hb_dev, float *out_dev, int64_t ldo,
                              mpreid_stream_t stream);

/* ---- CLIP ViT-B/16 image encoder, model/clip/model.py:415-479 + model/make_model.py:81-115 -- */
typedef struct {
    int32_t img_h, img_w;   /* INPUT.SIZE_TEST */
    int32_t patch, stride;  /* 16, MODEL.STRIDE_SIZE[0] */
    int32_t h_res, w_res;   /* patch grid; tokens L = h_res*w_res + 1 */
    int32_t width, layers, heads, out_dim; /* 768, 12, 12, 512 */
    int32_t neck_after;     /* TEST.NECK_FEAT == 'after': apply the eval BatchNorm necks */
    int32_t cls_only_last;  /* 1: last block computes only the CLS row (the only row the output uses) */
    int32_t precision;      /* MPREID_VIT_F16 or MPREID_VIT_SPLIT (the all-fp32 mode is mpreid_vit_forward_f32) */
} mpreid_vit_cfg;

/* Arithmetic of the encoder's linear layers and attention products (model/clip/model.py runs them in fp32,
 * processor/processor.py:187-198 has no autocast):
 *   F16    fp16 operands, fp32 accumulate: the fast mode; relative feature error ~4e-4 (operand rounding of 24 GEMMs),
 *          which moves mAP by 1e-4..3e-4 on hard data -- does NOT meet the 1e-4 mAP bound.
 *   SPLIT  every operand is an fp16 PAIR x = hi + lo (22 significant bits) and every product runs as
 *          hi.hi' + lo.hi' + hi.lo' with fp32 accumulation on the same fp16 matrix cores: fp32-grade results (relative
 *          feature error ~1e-6, |dmAP| <= 1e-4) at 3x the matrix work.  The parity mode that is also the measured mode.
 * In SPLIT mode every *_w pointer of the weight structs is an fp16 pair matrix [out][2*in] = [hi(in) | lo(in)] of
 * W * 2^e (e per matrix, so that the largest |entry| is in [2^9, 2^10)), and the matching *_s field is 2^-e
 * (mpreid_split_pack_f32 produces the layout).
 * Range of the fp16 modes (both): ACTIVATIONS are split / rounded unscaled, so every GEMM input -- the normalised pixels, the
 * LayerNorm outputs, q / k / v, the softmax-weighted values, the QuickGELU outputs -- must stay below 65 504 in magnitude.
 * Above that a `hi` half is +-inf, the products turn into NaN and the NaN reaches the image's feature row through the
 * residual stream (it is NOT clamped or hidden): R1_mAP_eval.compute() tests the features and raises RuntimeError
 * ("non-finite") instead of ranking them; use the all-fp32 mode for such a checkpoint / input range.  Trained CLIP towers
 * stay 1-2 orders of magnitude below the bound where it applies: the +-2000 "massive activation" channels live in the
 * fp32 residual stream, which is never an fp16 operand; LayerNorm outputs are at most sqrt(width) * max|gamma| + max|beta|.
 * Small values: an element below 2^-3 in magnitude keeps an ABSOLUTE error of 2^-25 (its `lo` half is an fp16 subnormal),
 * which is the level of fp32 rounding noise relative to O(1) activations; tests/test_gpu_vit.py pins both edges
 * (test_split_mode_on_clip_like_outliers: x30-100 LayerNorm gammas, +-1900 residual channels, +-60 FC1 pre-activations within
 * 2e-5 of the float64 graph and within a few times plain fp32's own error; test_split_mode_input_scale_edges). */
#define MPREID_VIT_F16 0
#define MPREID_VIT_SPLIT 1
/* Limits: tokens L = h_res * w_res + 1 <= MPREID_VIT_MAX_TOKENS (1025 = a 512 x 512 input at stride 16) in all three modes ->
 * MPREID_ERR_UNSUPPORTED above that.  L <= 256 (256 x 128 at stride 16 or 12): K / V of a head resident in LDS, one workgroup
 * per (image, head); 256 < L <= 1025 (256 x 256: L = 257 at stride 16, 442 at stride 12): the fp16 / split attention streams
 * K / V through LDS in 64-key blocks with an online softmax (same operands and product terms per mode), and the fp32 mode
 * keeps K / V resident up to L = 320 and streams them in 128-key chunks above.  Rows do not depend on the batch either way. */
#define MPREID_VIT_MAX_TOKENS 1025
/* (precision 2 was MPREID_VIT_SPLIT_LNFOLD in round 3: the LayerNorms folded into the linear layers behind them.  Removed in
 * round 4 -- measured 0.5 % SLOWER than MPREID_VIT_SPLIT, and tools/ws_poison_check.py found its 128 x 128-kernel form not
 * reproducible run to run at small batches; mpreid_vit_forward returns MPREID_ERR_UNSUPPORTED for it.  The in_proj_c / fc_c
 * fields below are kept for layout compatibility and are not read.) */

typedef struct { /* device pointers; *_w are fp16 [out][in] row-major (torch Linear layout) */
    const void *in_proj_w;   /* [3*width][width] fp16 */
    const float *in_proj_b;  /* [3*width] */
    const void *out_proj_w;  /* [width][width] fp16 */
    const float *out_proj_b;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    const void *fc_w;        /* [4*width][width] fp16 */
    const float *fc_b;
    const void *proj_w;      /* [width][4*width] fp16 */
    const float *proj_b;
    float in_proj_s, out_proj_s, fc_s, proj_s;   /* SPLIT mode: 2^-e of the matching weight matrix (ignored in F16 mode) */
    const float *in_proj_c, *fc_c;               /* not read (see MPREID_VIT_SPLIT above) */
} mpreid_vit_layer;

typedef struct { /* device pointers */
    const void *conv_w;         /* [width][3*patch*patch] fp16, inner order (c, kh, kw) */
    const float *class_emb;     /* [width] */
    const float *pos_emb;       /* [L][width] */
    const float *ln_pre_g, *ln_pre_b, *ln_post_g, *ln_post_b;
    const float *proj;          /* [width][out_dim] fp32 */
    const float *bn_scale, *bn_shift;           /* [width]   eval BN folded: y = x*scale + shift (or NULL) */
    const float *bn_proj_scale, *bn_proj_shift; /* [out_dim] */
    const mpreid_vit_layer *layers;             /* HOST array of cfg.layers entries */
    float conv_s;                               /* SPLIT mode: 2^-e of conv_w */
} mpreid_vit_weights;

/* ---- the image batch every encoder forward takes ----------------------------------------------------------------
 * Test-time-augmentation views of the reference's Uni-Prompt evaluation ("option A",
 * processor/processor_uniprompt_stage2.py:605-633), applied to the NORMALISED pixels while the first kernel of a tower
 * reads them (the ViT's patch gather, the RN50 stem's first convolution) instead of materialising a transformed
 * [B,3,H,W] tensor per view: the same bits as the view tensor materialised on the host. */
#define MPREID_VIEW_ORIGINAL 0
#define MPREID_VIEW_FLIP 1        /* torch.flip(img, [3]) */
#define MPREID_VIEW_PSEUDO_IR 2   /* img.mean(dim=1, keepdim=True).repeat(1, 3, 1, 1) -- in the HOST arithmetic of torch.mean,
                                   * ((c0 + c1) + c2) / 3 with a correctly rounded division: the reference's CPU path, bit for
                                   * bit.  torch's device kernel multiplies the sum by a rounded 1/3 (<= 1 ulp apart per pixel):
                                   * features of a device-materialised view agree to ~1e-6, not to the bit
                                   * (tests/test_gpu_preprocess.py::test_pseudo_ir_view_against_a_device_materialised_view) */
#define MPREID_VIEW_PSEUDO_RGB 3  /* img[:, 0:1].repeat(1, 3, 1, 1) */
/* A HOST struct.  EXACTLY ONE of the two pointers is non-NULL:
 *   f32_dev     [B][3][img_h][img_w] fp32, val_transforms applied (already mean / std normalised)
 *   u8_hwc_dev  [B][img_h][img_w][3] uint8, what the loader has after Resize (4x fewer input bytes): ToTensor and Normalize
 *               of val_transforms (datasets/make_dataloader.py:57-61) run inside the first kernel, in the reference's order
 *               and rounding, (x / 255 - mean[c]) / std[c] with two correctly rounded divisions -- the same bits as the
 *               host-transformed fp32 tensor, no intermediate tensor
 * mean / std (INPUT.PIXEL_MEAN / PIXEL_STD) are read only with uint8 input.  view is one of MPREID_VIEW_* (0 for a plain
 * forward).  NULL, both or neither pointer, or a view outside 0..3: MPREID_ERR_ARG, before anything is launched. */
typedef struct {
    const float *f32_dev;
    const uint8_t *u8_hwc_dev;
    float mean[3], std[3];
    int32_t view;
} mpreid_image_in;

size_t mpreid_vit_workspace_bytes(const mpreid_vit_cfg *cfg, int batch);
/* img: the batch (above); cv_emb_dev NULL or [B][width] (SIE_COE * cv_embed[idx], model/make_model.py:89-96);
 * out_dev [B][width+out_dim] fp32. */
int mpreid_vit_forward(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_image_in *img, int batch,
                       const float *cv_emb_dev, float *out_dev, void *ws_dev, size_t ws_bytes,
                       mpreid_stream_t stream);
/* The encoder's attention step alone, for unit tests and tools: the dispatchers mpreid_vit_forward calls, on the caller's
 * buffers.  qkv_dev [batch * tokens][3 * width] = q | k | v per token row, head h in columns h * 64 .. h * 64 + 63 of each
 * third, 16-byte aligned; fp32 with precision MPREID_VIT_SPLIT, fp16 with MPREID_VIT_F16.  out_dev, fp16:
 *   MPREID_VIT_F16     [batch * tokens][width]        softmax(q k^T / 8) v
 *   MPREID_VIT_SPLIT   [batch * tokens][2 * width]    [hi(width) | lo(width)], hi = fp16(o), lo = fp16(o - hi)
 * q_tiles 0: every token row of every image is written; q_tiles n > 0: the first min(16 n, tokens) rows of every image
 * (the forward's last block asks for 1: the CLS row's tile) and no other byte of out_dev; the rows a partial call writes carry
 * the bits of the same rows of a q_tiles = 0 call, in every kernel form (tests/test_gpu_attention_direct_forms.py).  width = 64 * heads,
 * 2 <= tokens <= MPREID_VIT_MAX_TOKENS; anything else is MPREID_ERR_ARG before a launch. */
int mpreid_vit_attention(const void *qkv_dev, int precision, int batch, int tokens, int width, int heads, int q_tiles,
                         void *out_dev, mpreid_stream_t stream);

/* All-fp32 mode of the same encoder (parity / debugging; SURVEY.md section 7 hard part 5): activations and weights
 * fp32, linear layers on the exact fp32 matrix instruction, attention on fp32 vector FMAs -- relative feature error
 * ~1e-6 against the fp32 CPU path instead of ~4e-4, at ~1/8 of the throughput.  The structs are the ones above,
 * but conv_w and every layer's *_w point to FP32 [out][in] matrices.  Head dimension 64 only. */
size_t mpreid_vit_workspace_bytes_f32(const mpreid_vit_cfg *cfg, int batch);
int mpreid_vit_forward_f32(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w_f32, const mpreid_image_in *img, int batch,
                           const float *cv_emb_dev, float *out_dev, void *ws_dev, size_t ws_bytes,
                           mpreid_stream_t stream);
/* The attention step of the all-fp32 mode alone, for unit tests and tools: the host rule mpreid_vit_forward_f32 runs in every
 * block (K / V resident in LDS up to tokens = 320, streamed in 128-key chunks above), on the caller's buffers.  qkv_dev fp32
 * [batch * tokens][3 * width] in the column layout of mpreid_vit_attention, out_dev fp32 [batch * tokens][width] =
 * softmax(q k^T / 8) v, both 16-byte aligned.  Every row is written and no other byte of out_dev.  width = 64 * heads,
 * 2 <= tokens <= MPREID_VIT_MAX_TOKENS; anything else is MPREID_ERR_ARG before a launch. */
int mpreid_vit_attention_f32(const float *qkv_dev, int batch, int tokens, int width, int heads,
                             float *out_dev /* [batch * tokens][width] */, mpreid_stream_t stream);
/* ---- MoE image encoder: model/clip/model.py:163-258 (MoEResidualAttentionBlock), 283-330 (MoETransformer) -------------
 * With MODEL.MOE.ENABLED the first moe_layers blocks of the image tower replace their MLP by num_experts expert MLPs behind a
 * softmax gate, every token goes to its top_k experts, and the routing is decided ONCE, in block 0, and reused by every
 * later MoE block (their own gate.weight is never read).  Eval semantics (dropout is the identity):
 *   x1 = x + attn(ln_1(x)); h = ln_2(x1)
 *   block 0 only: logits = h @ gate^T (fp32, no bias); p = softmax(logits); (p_sel, sel) = topk(p, top_k), equal
 *                 probabilities: the lower expert index first; w = p_sel / sum(p_sel)
 *   out = x1 + sum over e in sel(token), ASCENDING e, of w_e * (c_proj_e(QuickGELU(c_fc_e(h))) + b_proj_e)
 * A token's result depends on no other token or image of the batch, and not on the launch geometry.
 * Precision: the SPLIT mode (above) and nothing else -- MPREID_VIT_F16 in cfg->precision gives MPREID_ERR_UNSUPPORTED and there
 * is no all-fp32 MoE forward (the text tower's precedent).  Why: the router takes a discrete decision, so it runs in fp32 end
 * to end (LayerNorm as the tower's, fmaf dot products in a fixed order, no fp16 operand anywhere), and the expert GEMMs must
 * stay within the 2e-5 parity bound of the split mode, which fp16 operands miss by a factor of twenty.
 * cls_only_last: honoured when the last block is a dense block, exactly as in mpreid_vit_forward.  When the last block is an
 * MoE block (moe_layers == layers) that block runs on ALL token rows; the features are the same either way.
 * Limits: 1 <= top_k <= min(num_experts, MPREID_MOE_MAX_TOPK), num_experts <= MPREID_MOE_MAX_EXPERTS, 0 <= moe_layers <=
 * layers (the Python side resolves -1 and values above layers), width % 128 == 0, width == 64 * heads, batch * tokens <= MPREID_MOE_MAX_ROWS, tokens as for the dense
 * forward: MPREID_ERR_UNSUPPORTED otherwise.  NULL or misaligned pointers (16 bytes; the workspace: 256) and batch <= 0:
 * MPREID_ERR_ARG; a short or NULL workspace: MPREID_ERR_WORKSPACE -- all of them before anything is launched.  Stream-ordered,
 * no host synchronisation inside: the per-expert token counts never leave the device. */
#define MPREID_MOE_MAX_EXPERTS 64
#define MPREID_MOE_MAX_TOPK 8
/* token rows (batch * tokens) of one call, forward or unit seam: MPREID_ERR_UNSUPPORTED above that.  The dispatch scans its
 * per-workgroup counts in ONE workgroup, serially over ceil(rows / 1024) entries: microseconds at the 65 536 rows of an
 * encoder call (508 images of 129 tokens), of the order of 0.1 ms at this limit (8128 such images; estimated, not measured). */
#define MPREID_MOE_MAX_ROWS (1 << 20)
typedef struct {                 /* device pointers; one MoE block */
    const float *gate_w;         /* fp32 [E][width]; read in block 0 only (may be NULL elsewhere) */
    const void *fc_w;            /* fp16 pairs [E][4*width][2*width] = per expert the layout of mpreid_split_pack_f32 */
    const float *fc_b;           /* [E][4*width] */
    const void *proj_w;          /* fp16 pairs [E][width][2*4*width] */
    const float *proj_b;         /* [E][width] */
    const float *fc_s, *proj_s;  /* DEVICE arrays [E]: 2^-e of each expert's matrix */
} mpreid_moe_layer;
typedef struct {
    int32_t num_experts, top_k, moe_layers;
    const mpreid_moe_layer *layers;   /* HOST array of moe_layers entries */
} mpreid_vit_moe;
/* w->layers[l] of an MoE block (l < moe_layers): fc_w / fc_b / proj_w / proj_b / fc_s / proj_s are not read and may be NULL. */
size_t mpreid_vit_workspace_bytes_moe(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe, int batch);   /* 0: a bad request */
int mpreid_vit_forward_moe(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_moe *moe,
                           const mpreid_image_in *img, int batch, const float *cv_emb_dev, float *out_dev, void *ws_dev,
                           size_t ws_bytes, mpreid_stream_t stream);
/* The unit seams, for tests and tools.
 * mpreid_moe_route: x_dev fp32 [rows][width]; ln_g / ln_b the LayerNorm in front of the gate, or BOTH NULL when x already
 * holds h; gate_dev fp32 [E][width]; sel_out int32 [rows][K] in descending probability (ties: lower index first); w_out fp32
 * [rows][K] renormalised (K == 1: exactly 1.0f); logits_out fp32 [rows][E] or NULL.  Rows are b * L + l (the reference's flat
 * order is l * B + b).
 * mpreid_moe_mlp_split: x[row] += sum over the row's experts (ascending) of w * (expert MLP of a[row]), a_pairs_dev the fp16
 * pair rows [rows][hi(width) | lo(width)] that layernorm produces in split mode; the workspace (mpreid_moe_workspace_bytes,
 * 256-byte aligned) holds the dispatch tables and the per-slot intermediates; nothing else is written.
 * LIMIT: the CONTENTS of sel_dev (0 <= sel < E, distinct within a row) are device data and are NOT checked here: the caller
 * validates them (mpreid_moe_route produces valid ones).  An entry outside the range, or a repeated one, contributes nothing. */
size_t mpreid_moe_workspace_bytes(int64_t rows, int width, int num_experts, int top_k);   /* 0: outside the limits */
int mpreid_moe_route(const float *x_dev, int64_t rows, int width, const float *ln_g_dev, const float *ln_b_dev,
                     const float *gate_dev, int num_experts, int top_k, int32_t *sel_out, float *w_out, float *logits_out,
                     mpreid_stream_t stream);
int mpreid_moe_mlp_split(const void *a_pairs_dev, int64_t rows, int width, const int32_t *sel_dev, const float *w_dev,
                         int num_experts, int top_k, const mpreid_moe_layer *layer, float *x_inout_dev, void *ws_dev,
                         size_t ws_bytes, mpreid_stream_t stream);
/* ---- The gradient through one routed MLP and the gradient of the router (csrc/moe_grad.hip) ------------------------------
 * The building blocks of the MoE tower's backward (mpreid_vit_backward_moe, below), as unit seams.  Stage 2 freezes every expert
 * matrix, so these deliver the gradient THROUGH the experts and the gradient OF the routing weights; the expert matrices' own
 * gradients are not implemented: mpreid_moe_expert_grads keeps their place, and a non-NULL member is MPREID_ERR_UNSUPPORTED.
 *   per slot s = (row r, expert e = sel[r][k]):  u_s = c_fc_e(h_r), t_s = QuickGELU(u_s), y_s = c_proj_e(t_s) + b_proj_e
 *   d_w[r][k] = <dy_r, y_s>;  dt_s = (w[r][k] dy_r) . Wproj_e;  du_s = dt_s * QuickGELU'(u_s)
 *   d_a[r] = sum over the row's experts, ASCENDING e, of du_s . Wfc_e
 * u and y are recomputed by the forward's own grouped GEMMs (y has the forward's bits); the two gradient GEMMs are exact fp32
 * (one k-ascending fmaf chain per element, the arithmetic of the dense sweep's mpreid_gemm_f32_linear) on fp32 transposed
 * copies of the expert matrices.
 * mpreid_moe_mlp_backward: a_pairs / sel / w / layer as for mpreid_moe_mlp_split; dy_dev fp32 [rows][width]; d_a_out fp32
 * [rows][width] is WRITTEN; d_w_out fp32 [rows][top_k] (entry k belongs to sel[r][k]) is written, or added to with one rounded
 * add per entry when accumulate_d_w != 0 (the tower sums it over its MoE blocks).  Either output may be NULL (not both); the
 * other's bits do not change.  Stateless, stream-ordered, no host synchronisation, every error before a launch.
 * LIMIT: as for mpreid_moe_mlp_split the CONTENTS of sel_dev are not checked.  An entry outside 0 .. E-1 contributes nothing,
 * gets d_w = 0 and is never used as an address; of a repeated expert the last entry is the one the forward used, the earlier
 * ones get d_w = 0.
 * Workspace (mpreid_moe_grad_workspace_bytes, 256-byte aligned), per routed slot (<= rows * top_k + 128 * num_experts of
 * them): the forward's 20 * width bytes (hidden pairs, y) and 16 * width bytes more (u, overwritten by du); per row 8 * top_k
 * bytes of tables.  Nothing else is written.
 * mpreid_moe_route_backward: logits [rows][E], sel / w [rows][K] of mpreid_moe_route, d_w [rows][K] (NULL: zeros).
 *   c_r = sum_k w[r][k] d_w[r][k];  d_logits[r][sel[r][k]] = w[r][k] (d_w[r][k] - c_r), every other entry exactly 0
 *   (top_k == 1: all exactly 0);  with aux_coef != 0 also  d_logits[r][j] += p_rj (g_j - sum_e p_re g_e),
 *   g_e = aux_coef * E * f_e / rows, p = softmax(logits), f_e = the share of rows whose sel holds e
 *   l_aux = E * sum_e f_e P_e,  P_e = mean_r p_re   (model/clip/model.py:342-377 on ONE layer of logits; NOT times aux_coef)
 * aux_coef == 0 adds nothing: the bits are those of the routing term alone.  d_logits_out or l_aux_out may be NULL.  Its
 * workspace (mpreid_moe_route_backward_workspace_bytes, 256-byte aligned): one float per row, and 4 * num_experts bytes per
 * 1024 rows of expert counts. */
typedef struct {                 /* fp32 device copies, per expert the TRANSPOSE of the checkpoint's [out][in] matrix */
    const float *fc_t;           /* [E][width][4*width] */
    const float *proj_t;         /* [E][4*width][width] */
} mpreid_moe_layer_t;
typedef struct {                 /* the expert matrices' own gradients: NOT IMPLEMENTED, every member must be NULL */
    float *fc_w, *fc_b, *proj_w, *proj_b;
} mpreid_moe_expert_grads;
size_t mpreid_moe_grad_workspace_bytes(int64_t rows, int width, int num_experts, int top_k);   /* 0: outside the limits */
int mpreid_moe_mlp_backward(const void *a_pairs_dev, int64_t rows, int width, const int32_t *sel_dev, const float *w_dev,
                            int num_experts, int top_k, const mpreid_moe_layer *layer, const mpreid_moe_layer_t *layer_t,
                            const float *dy_dev, float *d_a_out, float *d_w_out, int accumulate_d_w,
                            const mpreid_moe_expert_grads *d_experts /* NULL */, void *ws_dev, size_t ws_bytes,
                            mpreid_stream_t stream);
/* ---- The MoE tower's training forward and backward (csrc/vit.hip, csrc/vit_grad.hip) ---------------------------------------
 * mpreid_vit_forward_train_moe: mpreid_vit_forward_train for a tower with at least one MoE block.  With MoE the reference's
 * tower hands out x11 = x12 = the transformer's output (model/clip/model.py:448-454), so f_last is the CLS row of the LAST
 * block's OUTPUT (the dense tower's: of its input).  f | f_proj keep the bits of mpreid_vit_forward_moe of a tower without a
 * neck (the same launches; cfg.cls_only_last is honoured as there).  logits_out [B * L][E] (rows b * L + l; the reference's
 * flat order is l * B + b) and l_aux_out [1] = the load-balancing loss of those logits, each optional.  Workspace:
 * mpreid_vit_forward_train_moe_workspace_bytes.  moe_layers == 0: MPREID_ERR_UNSUPPORTED (that is the dense tower).
 * mpreid_vit_backward_moe: mpreid_vit_backward for that tower -- the gradients of
 *   sum(f_last o d_f_last) + sum(f o d_f) + sum(f_proj o d_f_proj) + aux_coef * l_aux
 * with the dense entry point's contract: stateless, stream-ordered, no host synchronisation, gradients written not
 * accumulated, NULL members skipped without changing the other outputs' bits, every error found before a launch (a NaN or
 * infinite aux_coef is MPREID_ERR_ARG),
 * cfg.cls_only_last ignored.  Dense blocks (l >= moe_layers) go through the dense sweep's own code; of an MoE block the
 * attention half does too, and the MLP half is mpreid_moe_mlp_backward's.  The routing (w, sel) of block 0 serves every MoE
 * block, so d_w is summed over them (swept last block first, one rounded add per block) and reaches block 0's gate:
 *   d gate.weight [E][width] = d_logits^T . h,  dh += d_logits . gate.weight   (h = the fp32 ln_2 output the router saw)
 * d_gate_w_out (block 0's; later gates are never read, so they have no gradient) and l_aux_out may be NULL.  Of an MoE block
 * grads->layers[l].fc_w / fc_b / proj_w / proj_b must be NULL (it has no dense MLP) and wt->layers[l].fc_t / proj_t are not
 * read; the expert matrices' own gradients are not implemented (there is no member to ask for them).  moe_t: per MoE block the
 * fp32 transposed expert matrices (mpreid_moe_layer_t), a HOST array of moe_layers entries.
 * Workspace (mpreid_vit_backward_moe_workspace_bytes): the dense sweep's, plus per row 8 * (top_k + num_experts) + 4 * top_k
 * bytes (routing, logits, d_logits, d_w) and mpreid_moe_grad_workspace_bytes(batch * tokens, width, num_experts, top_k).
 * Limits: those of mpreid_vit_backward and of mpreid_vit_forward_moe (rows * top_k <= 2^23 follows from them). */
typedef struct {
    const mpreid_moe_layer_t *layers;   /* HOST array of moe_layers entries */
} mpreid_vit_moe_t;
size_t mpreid_vit_forward_train_moe_workspace_bytes(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe, int batch);
int mpreid_vit_forward_train_moe(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_moe *moe,
                                 const mpreid_image_in *img, int batch, const float *cv_emb_dev, float *f_last_out, float *f_out,
                                 float *f_proj_out, float *logits_out, float *l_aux_out, void *ws_dev, size_t ws_bytes,
                                 mpreid_stream_t stream);
size_t mpreid_vit_backward_moe_workspace_bytes(const mpreid_vit_cfg *cfg, const mpreid_vit_moe *moe, int batch);
size_t mpreid_moe_route_backward_workspace_bytes(int64_t rows, int num_experts);   /* 0: outside the limits */
int mpreid_moe_route_backward(const float *logits_dev, int64_t rows, int num_experts, int top_k, const int32_t *sel_dev,
                              const float *w_dev, const float *d_w_dev, float aux_coef, float *d_logits_out, float *l_aux_out,
                              void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);

/* ---- CLIP text tower, model/clip/model.py:609-619 after the embedding lookup (= model/make_model_uniprompt.py:58-68) ----
 * x = prompts + pos_emb; cfg.layers residual blocks with CAUSAL attention (key j takes part in query row i iff j <= i,
 * model/clip/model.py:582-588); ln_final; row eot[b] of prompt b; @ text_projection.  No BatchNorm neck.
 * Precision: the SPLIT mode of the image encoder (above) and nothing else -- fp16 pair operands, hi.hi' + lo.hi' + hi.lo' on
 * the matrix cores, fp32 accumulation, fp32 residual stream / LayerNorm / softmax.  The text side is never the throughput
 * path, so there is NO fp16 and NO all-fp32 text mode and the config has no precision field: a caller that asks for one
 * (mpreid.ops.TextEncoder / text_attention) gets MPREID_ERR_UNSUPPORTED.  The layers are mpreid_vit_layer entries in their
 * SPLIT-mode layouts (pair matrices from mpreid_split_pack_f32 and the matching *_s).
 * Limits: width == 64 * heads, width % 128 == 0, width <= 1024, 2 <= tokens <= MPREID_TEXT_MAX_TOKENS (K / V of one head stay
 * in LDS, one workgroup per (prompt, head)); anything else is MPREID_ERR_UNSUPPORTED.  NULL pointers, batch <= 0, buffers that
 * are not 16-byte aligned (the workspace: 256): MPREID_ERR_ARG; a short or NULL workspace: MPREID_ERR_WORKSPACE -- all of
 * them before anything is launched.  A row of the output does not depend on the batch it is computed in, and not on the
 * prompt rows behind its eot row.
 * LIMIT: the CONTENTS of eot_dev (0 <= eot[b] < tokens) are device data and are NOT checked here: the caller validates them
 * (mpreid.ops.TextEncoder.forward does, on the host).  A value outside the range reads the nearest row of its own prompt. */
#define MPREID_TEXT_MAX_TOKENS 128
typedef struct { int32_t tokens, width, layers, heads, out_dim; } mpreid_text_cfg;      /* 77, 512, 12, 8, 512 */
typedef struct {                       /* device pointers; SPLIT-mode layouts of mpreid_vit_layer */
    const float *pos_emb;              /* [tokens][width] */
    const float *ln_final_g, *ln_final_b;
    const float *proj;                 /* text_projection, fp32 [width][out_dim] */
    const mpreid_vit_layer *layers;    /* HOST array of cfg.layers entries */
} mpreid_text_weights;
size_t mpreid_text_workspace_bytes(const mpreid_text_cfg *cfg, int batch);   /* needs no device; 0 for a NULL / empty request */
int mpreid_text_forward(const mpreid_text_cfg *cfg, const mpreid_text_weights *w,
                        const float *prompts_dev,   /* [B][tokens][width] fp32: the embedded prompts, positional embedding NOT added */
                        const int32_t *eot_dev,     /* [B]: the row each prompt is read out at */
                        int batch, float *out_dev,  /* [B][out_dim] fp32 */
                        void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);
/* The causal attention kernel alone, for unit tests and tools.  qkv_dev fp32 [batch * tokens][3 * width] in the column
 * layout of mpreid_vit_attention; out_dev fp16 [batch * tokens][2 * width] = [hi(width) | lo(width)]; both 16-byte aligned.
 * Every row of every prompt is written and no other byte.  Limits and errors as above. */
int mpreid_text_attention(const void *qkv_dev, int batch, int tokens, int width, int heads, void *out_dev,
                          mpreid_stream_t stream);

/* ---- The text tower's gradient with respect to the prompts (prompt learning: every tower weight stays frozen) ----
 * grad_prompts = d loss / d prompts given grad_out = d loss / d (the output of mpreid_text_forward).  No weight gradient, no
 * optimizer, no loss.  The call is stateless: it re-runs the forward's own split-precision blocks, keeping each block's input,
 * then walks the layers back.  Per layer it recomputes q | k | v, the block's mid-point and the fp32 FC1 pre-activation with the
 * forward's launchers, so the gradient is taken at the activations the forward really produces.  Every gradient GEMM
 * (dX = dY . W) is the exact fp32 GEMM over mpreid_text_weights_t: fp32 TRANSPOSED copies [in][out] of the frozen matrices
 * (gradients of a prompt-learning loss sit far below fp16's range, so they never pass through fp16 pair operands).  Causal
 * attention, LayerNorm and QuickGELU are differentiated by fp32 kernels without atomics: the same bits from run to run.
 * Properties: prompt b's gradient does not depend on the batch it is computed in; rows behind eot[b] are exactly 0.0; the
 * result is exactly homogeneous in grad_out under power-of-two scaling (short of underflow); every element of grad_prompts
 * is written.  Limits and errors as for mpreid_text_forward (all before anything is launched); prompts_dev, grad_prompts_dev
 * and the transposed matrices 16-byte aligned, the workspace 256; the contents of eot_dev are validated by the caller. */
typedef struct {   /* device pointers, fp32, [in][out] = the checkpoint's [out][in] transposed; also mpreid_vit_layer_t (below) */
    const float *in_proj_t;            /* [width][3 * width] */
    const float *out_proj_t;           /* [width][width] */
    const float *fc_t;                 /* [width][4 * width] */
    const float *proj_t;               /* [4 * width][width] */
} mpreid_text_layer_t;
typedef struct {
    const float *proj_t;               /* text_projection transposed, [out_dim][width] */
    const mpreid_text_layer_t *layers; /* HOST array of cfg.layers entries */
} mpreid_text_weights_t;
size_t mpreid_text_backward_workspace_bytes(const mpreid_text_cfg *cfg, int batch);   /* needs no device; 0 for a bad request */
int mpreid_text_backward(const mpreid_text_cfg *cfg, const mpreid_text_weights *w, const mpreid_text_weights_t *wt,
                         const float *prompts_dev, const int32_t *eot_dev, const float *grad_out_dev /* [B][out_dim] */,
                         int batch, float *grad_prompts_dev /* [B][tokens][width], every element written */,
                         void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);
/* The causal attention backward kernel alone, for unit tests and tools: qkv_dev fp32 [batch * tokens][3 * width] as for
 * mpreid_text_attention, d_o_dev fp32 [batch * tokens][width] -> d_qkv_dev fp32 [batch * tokens][3 * width] = dq | dk | dv; all
 * 16-byte aligned.  Every element of d_qkv_dev is written and no other byte. */
int mpreid_text_attention_backward(const float *qkv_dev, const float *d_o_dev, int batch, int tokens, int width, int heads,
                                   float *d_qkv_dev, mpreid_stream_t stream);
/* LayerNorm's input gradient (biased variance, eps 1e-5, statistics recomputed from x_dev): rows of `width` fp32 values,
 * dx = (gamma o dy - mean(gamma o dy) - xhat * mean(gamma o dy o xhat)) / sigma; accumulate != 0 adds it to what dx_dev holds.
 * dx_dev must not overlap the inputs. */
int mpreid_layernorm_backward_f32(const float *x_dev, const float *dy_dev, const float *gamma_dev, int64_t rows, int width,
                                  int accumulate, float *dx_dev, mpreid_stream_t stream);
/* Three row kernels of every tower alone, for unit tests and tools; each goes through the launcher the towers call.
 * Errors, all before anything is launched: a NULL pointer, a misaligned one, form outside 0..2, n % 4 != 0, a negative
 * count: MPREID_ERR_ARG; a width that is not a multiple of 128 in 128..1024: MPREID_ERR_UNSUPPORTED.  rows, batch or n
 * of 0 is MPREID_OK and launches nothing.
 *
 * mpreid_layernorm_f32: LayerNorm over rows of `width` fp32 values (biased variance, eps 1e-5, fp32 statistics), in the
 * three output forms of the towers.  form 0: fp32 [rows][width], out_dev may be x_dev (ln_pre runs in place); form 1: fp16
 * [rows][width]; form 2: the fp16 pair [rows][hi(width) | lo(width)] of the split precision.  All four pointers 16-byte
 * aligned.  Every element of the output is written and no other byte. */
int mpreid_layernorm_f32(const float *x_dev, int64_t rows, int width, const float *gamma_dev, const float *beta_dev,
                         int form /* 0 fp32 [rows][W] (out_dev may be x_dev), 1 fp16 [rows][W], 2 fp16 pairs [rows][2W] */,
                         void *out_dev, mpreid_stream_t stream);
/* The head of every tower: LayerNorm of ONE row per item, that row @ proj, optional eval-BatchNorm necks.  Item b is at
 * x_dev + b * item_stride floats; its row is row 0 (row_of_dev NULL: the CLS row) or row row_of_dev[b] clamped into
 * [0, tokens - 1]; rows are `width` wide.  y_dev [batch][width] receives the normalised rows (before any neck);
 * out_dev[b][out_col + o] = sum_k y[b][k] * proj_dev[k][o] (proj_dev [width][out_dim]), through y * bnp_scale[o] +
 * bnp_shift[o] when that neck is given; with ln_to_out != 0 out_dev[b][0 : width] = y[b], through y * bn_scale[k] +
 * bn_shift[k] when that neck is given.  Rows of out_dev are out_stride floats apart.  A neck is both of its pointers or
 * neither.  x_dev 16-byte aligned, everything else 4.  out_stride >= out_col + out_dim, and out_col >= width with
 * ln_to_out.  No element of out_dev outside the columns named is written. */
int mpreid_tower_head_f32(const float *x_dev, int64_t item_stride, const int32_t *row_of_dev /* NULL: row 0 */, int tokens,
                          int batch, int width, int out_dim, const float *ln_g_dev, const float *ln_b_dev, const float *proj_dev,
                          const float *bn_scale_dev, const float *bn_shift_dev, const float *bnp_scale_dev,
                          const float *bnp_shift_dev, float *y_dev, float *out_dev, int out_stride, int out_col, int ln_to_out,
                          mpreid_stream_t stream);
/* QuickGELU's backward, in place: d[i] *= s + 1.702 u[i] s (1 - s), s = sigmoid(1.702 u[i]); n a multiple of 4, both
 * pointers 16-byte aligned. */
int mpreid_quickgelu_backward_f32(const float *u_dev, float *d_dev /* in place */, int64_t n, mpreid_stream_t stream);

/* ---- The image tower's gradient (stage 2): training forward, attention gradient, the sweep and the parameter gradients ----
 * The three features stage 2 differentiates, the one backward kernel the image tower cannot borrow from the text tower, and
 * the sweep over the layers with every parameter gradient.
 *
 * mpreid_vit_forward_train: the dense tower in MPREID_VIT_SPLIT precision, the launch sequence of mpreid_vit_forward plus one
 * copy of batch rows.  Outputs, all fp32, 4-byte aligned, every element written:
 *   f_last_dev [B][width]     the CLS row of the LAST block's input (model/clip/model.py:458-468; with one layer that is
 *                             ln_pre's output); no ln_post
 *   f_dev      [B][width]     ln_post(x_layers)[:, 0]
 *   f_proj_dev [B][out_dim]   f @ proj
 * No BatchNorm neck is applied whatever cfg.neck_after says (the stage-2 head owns BNNeck).  f | f_proj carries the bits of
 * mpreid_vit_forward's out_dev with neck_after = 0, with cls_only_last on and off.  layers < 1 or a precision other than
 * MPREID_VIT_SPLIT: MPREID_ERR_UNSUPPORTED; the other limits, the workspace (mpreid_vit_workspace_bytes) and the argument
 * errors are mpreid_vit_forward's; all of them before anything is launched. */
int mpreid_vit_forward_train(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_image_in *img, int batch,
                             const float *cv_emb_dev, float *f_last_dev, float *f_dev, float *f_proj_dev, void *ws_dev,
                             size_t ws_bytes, mpreid_stream_t stream);
/* The unmasked attention gradient: qkv_dev fp32 [batch * tokens][3 * width] in the column layout of mpreid_vit_attention,
 * d_o_dev fp32 [batch * tokens][width] -> d_qkv_dev fp32 [batch * tokens][3 * width] = dq | dk | dv; all 16-byte aligned.
 *   P = softmax(q k^T / 8), dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(P o dP)), dQ = dS K / 8, dK = dS^T Q / 8
 * ONE form for every token count, two kernels of 512 threads over the workspace (16 bytes per (image, head, query row):
 * the row's score maximum, exponential sum, dP at its strongest key, and rowsum(P o (dP - that))):
 *   rows pass   a workgroup per (image, head, 8 query rows), a wave per row; K and V stream through LDS in 64-key blocks of
 *               fp32 [64][68] (68: the 16-byte reads of 16 consecutive rows cover all 64 banks); writes the row statistics and dQ.
 *               LDS = 39 168 + 64 * (tokens rounded up to 64) bytes: 51 456 at 129 .. 192 tokens (3 workgroups per CU),
 *               55 552 at 193 .. 256, 59 648 at 257 .. 320, 67 840 at 442, 108 800 at 1025 (1 per CU).
 *   columns pass  a workgroup per (image, head, 8 keys), a wave per key; Q and dO stream in 64-row blocks; P and dS are rebuilt
 *               from the stored statistics; writes dK and dV.  LDS = 43 264 bytes at every token count (3 workgroups per CU).
 * There is no resident form and so no boundary between forms.  No atomics; every sum has one fixed order: a score is one
 * fmaf chain over the 64 features wherever it is recomputed; a row statistic is summed by lane l over the keys l, l + 64, ...
 * ascending, then the butterfly 32 .. 1; dQ / dK / dV elements are one fmaf chain over the keys / query rows, ascending.
 * So: the same bits from run to run, and for an image alone or inside a batch; exactly homogeneous in d_o under
 * power-of-two scaling (short of underflow); an all-zero d_o gives zeros.  dS is taken about the row's strongest key
 * (DESIGN section 14), which keeps the digits of saturated rows.  Every element of d_qkv_dev is written and no other byte.
 * Limits: width == 64 * heads, width % 128 == 0, width <= 1024, 2 <= tokens <= MPREID_VIT_MAX_TOKENS, else
 * MPREID_ERR_UNSUPPORTED; NULL or misaligned pointers, batch <= 0: MPREID_ERR_ARG; a NULL or short workspace (16-byte
 * aligned): MPREID_ERR_WORKSPACE -- all before anything is launched. */
size_t mpreid_vit_attention_backward_workspace_bytes(int batch, int tokens, int heads);   /* needs no device; 0 for a bad request */
int mpreid_vit_attention_backward(const float *qkv_dev, const float *d_o_dev, int batch, int tokens, int width, int heads,
                                  float *d_qkv_dev, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);

/* mpreid_vit_backward: the three feature gradients of mpreid_vit_forward_train -> the gradient of every tower parameter, of
 * cv_emb and of the embedded sequence.  Stateless and stream-ordered, no host synchronisation, as mpreid_text_backward: it
 * re-runs the forward's own split-precision launches (every block on all rows, whatever cfg.cls_only_last says) keeping the
 * embedded sequence and each block's input x_l, seeds dx at the CLS rows from d_f_dev and d_f_proj_dev (ln_post and proj are
 * differentiated there; every other row of dx starts as exact zero), walks the layers back recomputing q | k | v, the
 * attention output, the block's mid-point and the fp32 FC1 pre-activation with the forward's launchers, adds d_f_last_dev
 * to the CLS rows once the last block has been swept, and sweeps ln_pre.  Any seed may be NULL (= zero).  No gradient passes
 * through fp16: dX = dY . W is the exact fp32 GEMM over mpreid_vit_weights_t (fp32 transposed copies [in][out]); a weight
 * gradient dW[n][k] = sum_m dY[m][n] X[m][k] is the same GEMM over two transposed operands [cols][rows rounded up to 4, pad
 * zero] written by a transposing kernel, so it is one k-ascending chain over the token rows.  X is what the forward's GEMM
 * multiplied: the fp16 pair unpacked to hi + lo for LayerNorm-2 outputs, the attention output and the patches, the fp32 value
 * the pair was split from for LayerNorm-1 outputs and the MLP's hidden layer (they differ by 2^-22 relative).  Bias, beta
 * and gamma gradients are column sums (mpreid_colsum_f32 below) in a fixed order.  No atomics: the same bits from run to run.
 *
 * grads: optional; fp32 device pointers in the checkpoint's layout (matrices [out][in], conv_w [width][3 * patch * patch],
 * pos_emb [L][width], proj [width][out_dim]) plus cv_emb [batch][width], the gradient of the cv_emb_dev rows as given.
 * NULL members (or a NULL struct) are skipped, cost nothing and leave the other outputs' bits unchanged.  Gradients are
 * WRITTEN, not accumulated.  d_tokens_dev: optional [batch][L][width], the gradient of ln_pre's input, 16-byte aligned.
 * Workspace, bytes per token row of width W (rows rounded up to 256): the forward's regions (mpreid_vit_workspace_bytes),
 * 4 W the embedded sequence, layers x 4 W the x_l, 4 W dx, 16 W the hidden layer's gradient, 4 W a LayerNorm output's
 * gradient, 12 W dq | dk | dv, 4 W the transposed attention output, 2 x 4 max(4 W, 3 patch^2, out_dim) the two transposed
 * operands, 16 bytes per (head, row) attention statistics, and the reductions' partial sums (8 x 4 W bytes per 128 rows)
 * and row statistics (8 bytes per row).  Errors, all before anything is launched: NULL or misaligned pointers, batch <= 0,
 * batch * L above 65 535 * 128 rows (the column reduction's grid): MPREID_ERR_ARG; a short workspace (256-byte aligned): MPREID_ERR_WORKSPACE; layers < 1, a precision other than
 * MPREID_VIT_SPLIT or a shape outside mpreid_vit_forward's: MPREID_ERR_UNSUPPORTED.  (An MoE tower: mpreid_vit_backward_moe.) */
typedef mpreid_text_layer_t mpreid_vit_layer_t;   /* a block's transposed matrices: ONE struct for both towers (above) */
typedef struct {
    const mpreid_vit_layer_t *layers;  /* HOST array of cfg.layers entries */
} mpreid_vit_weights_t;
typedef struct {                       /* device pointers, fp32, torch layout; NULL = not wanted */
    float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *fc_w, *fc_b, *proj_w, *proj_b, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
} mpreid_vit_layer_grads;
typedef struct {
    float *conv_w, *class_emb, *pos_emb, *ln_pre_g, *ln_pre_b, *ln_post_g, *ln_post_b, *proj, *cv_emb;
    const mpreid_vit_layer_grads *layers;   /* HOST array of cfg.layers entries */
} mpreid_vit_grads;
size_t mpreid_vit_backward_workspace_bytes(const mpreid_vit_cfg *cfg, int batch);   /* needs no device; 0 for a bad request */
int mpreid_vit_backward(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_weights_t *wt,
                        const mpreid_image_in *img, int batch, const float *cv_emb_dev, const float *d_f_last_dev,
                        const float *d_f_dev, const float *d_f_proj_dev, const mpreid_vit_grads *grads, float *d_tokens_dev,
                        void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);
/* the MoE tower's sweep: described with mpreid_vit_forward_train_moe ("The MoE tower's training forward and backward") */
int mpreid_vit_backward_moe(const mpreid_vit_cfg *cfg, const mpreid_vit_weights *w, const mpreid_vit_weights_t *wt,
                            const mpreid_vit_moe *moe, const mpreid_vit_moe_t *moe_t, const mpreid_image_in *img, int batch,
                            const float *cv_emb_dev, const float *d_f_last_dev, const float *d_f_dev, const float *d_f_proj_dev,
                            float aux_coef, const mpreid_vit_grads *grads, float *d_gate_w_out, float *d_tokens_dev,
                            float *l_aux_out, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);
/* The two small kernels of the parameter gradients alone, for unit tests and tools.
 * mpreid_transpose_pad_f32: dst [cols][rows_pad] = src [rows][cols] transposed, columns rows .. rows_pad - 1 zero.
 * mpreid_colsum_f32: out_sum[c] = sum_m dy[m][c] and out_sumx[c] = sum_m dy[m][c] xhat[m][c], xhat = (x - mean) / sigma per row
 * of x [rows][cols] (biased variance, eps 1e-5); either output may be NULL (out_sumx needs x).  Fixed order: rows in pieces of
 * 128, a column's piece added rows ascending, the pieces' sums added ascending; row statistics: lane l of a wave adds the
 * elements l, l + 64, ... ascending, then the butterfly 32 .. 1.  Every step is one rounded fp32 operation (no fused
 * multiply-add).  Workspace 256-byte aligned.  Limits, MPREID_ERR_ARG before a launch: rows_pad >= rows, rows_pad < 2^31,
 * cols <= 65 535 * 32 (transpose); rows <= 65 535 * 128 (column sums); a NULL or short workspace: MPREID_ERR_WORKSPACE. */
int mpreid_transpose_pad_f32(const float *src_dev, int64_t rows, int cols, float *dst_dev, int64_t rows_pad, mpreid_stream_t stream);
size_t mpreid_colsum_workspace_bytes(int64_t rows, int cols);   /* needs no device; 0 for a bad request */
int mpreid_colsum_f32(const float *dy_dev, const float *x_dev, int64_t rows, int cols, float *out_sum_dev, float *out_sumx_dev,
                      void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);

/* ---- Stage-1 prompt learning (processor/processor_uniprompt_stage1.py:66-100): loss, context gradients, Adam ----
 * Three small fp32 entry points around mpreid_text_forward / mpreid_text_backward.  No atomics and a fixed summation order: the
 * same bits from run to run.  Every output element is written and no other byte; every argument error is found before anything
 * is launched; stream-ordered, no host synchronisation.  Float buffers 4-byte aligned, labels / indices 8, the workspace 256.
 *
 * The symmetric supervised contrastive loss (loss/supcontrast.py at temperature 1, called twice, :90-93) and its gradients.
 * S = img . txt^T [batch][batch], M_ab = (labels[a] == labels[b]), n_a = sum_b M_ab, P = softmax over the rows of S, Q = softmax
 * over its columns:
 *   loss[0] = loss_i2t = -(1/B) sum_a (1/n_a) sum_b M_ab log P_ab        loss[1] = loss_t2i = -(1/B) sum_b (1/n_b) sum_a M_ab log Q_ab
 *   G_ab = -(1/B) ((M_ab / n_a - P_ab) + (M_ab / n_b - Q_ab))            d_txt = G^T . img        d_img = G . txt
 * (d_txt, d_img: the gradients of loss[0] + loss[1]; either may be NULL and is then not computed -- the other outputs keep
 * their bits.)  Stabilised with the row and the column maxima: log P_ab = (S_ab - max_a) - log sum_b exp(S_ab - max_a).
 * Summation order: S_ab is ONE fmaf chain over the features, ascending.  A row's (column's) exp sum and its masked log-probability
 * sum: lane l of one wave adds the entries l, l + 64, ... in ascending order, then the butterfly 32, 16, 8, 4, 2, 1.  A loss: thread
 * t of 256 adds the row terms t, t + 256, ... ascending, butterfly per wave, then the four wave sums in order; divided by B last.
 * A gradient element is one fmaf chain over the other side's rows, ascending.  batch == 1 gives losses and gradients of 0.0.
 * Limits: 1 <= batch <= MPREID_SUPCON_MAX_BATCH (the two [B][B] logit matrices live in the workspace; above: MPREID_ERR_UNSUPPORTED),
 * dim >= 1.  The labels are only compared with each other: any int64 values. */
#define MPREID_SUPCON_MAX_BATCH 1024
size_t mpreid_supcon_workspace_bytes(int batch, int dim);   /* needs no device; 0 for a bad request */
int mpreid_supcon_pair_f32(const float *img_dev, const float *txt_dev /* both [batch][dim] */, const int64_t *labels_dev,
                           int batch, int dim, float *loss_dev /* [2] */, float *d_txt_dev, float *d_img_dev /* [batch][dim] or NULL */,
                           void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);
/* The same call with the gradients of ONE of the two losses, what a single SupConLoss call differentiates (the drop-in
 * loss/supcontrast.py): directions = 1 keeps the row-softmax term of G (d loss[0]), 2 the column-softmax term (d loss[1]), 3 is
 * mpreid_supcon_pair_f32 bit for bit.  Both losses are written whatever the directions. */
int mpreid_supcon_f32(const float *img_dev, const float *txt_dev, const int64_t *labels_dev, int batch, int dim, int directions,
                      float *loss_dev, float *d_txt_dev, float *d_img_dev, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);
/* The gradient of a context tensor from the prompt gradient (what autograd's index backward does for ctx[idx]):
 *   out[s][t][e] = sum over b ascending with idx[b] == s of src[b][tok0 + t][e],   s < n_seg, t < n_tok, e < width
 * a sequential fp32 sum in batch order starting from 0.0; segments without a member are exactly 0.0.  src_dev [batch][tokens][width]
 * (what mpreid_text_backward writes), idx_dev int64 [batch], out_dev [n_seg][n_tok][width].  0 <= tok0, tok0 + n_tok <= tokens;
 * n_tok * width < 2^24.  LIMIT: the CONTENTS of idx_dev are device data and are NOT checked here: the caller validates them
 * (mpreid.ops.rows_segment_sum does); a value outside 0 .. n_seg - 1 belongs to no segment and is never used as an address. */
int mpreid_rows_segment_sum_f32(const float *src_dev, const int64_t *idx_dev, int batch, int tokens, int width, int tok0,
                                int n_tok, int n_seg, float *out_dev, mpreid_stream_t stream);
/* One step of torch.optim.Adam (decoupled == 0: L2 weight decay added to the gradient) or torch.optim.AdamW (decoupled != 0) on
 * n fp32 elements, in place; step >= 1 is the number of this step, 0 <= beta < 1, eps > 0, lr and weight_decay >= 0 and finite.
 * The host computes in double, from the float arguments, and rounds once to fp32: w1 = 1 - beta1, w2 = 1 - beta2,
 * a = lr / (1 - beta1^step), r = sqrt(1 - beta2^step), lw = lr * weight_decay.  Per element, each line rounded once:
 *   decoupled == 0: g = fmaf(weight_decay, p, grad)          decoupled != 0: p = fmaf(-lw, p, p), g = grad
 *   m = fmaf(w1, g - m, m)        v = fmaf(w2, g * g, beta2 * v)        p = fmaf(-a, m / (sqrtf(v) / r + eps), p)
 * (IEEE division and square root).  Groups of four elements go through 16-byte accesses when all four buffers are 16-byte
 * aligned, the n % 4 elements behind them (all of them otherwise) one by one: the same arithmetic, the same bits.  grad_dev must
 * not overlap the other three. */
int mpreid_adam_step_f32(float *param_dev, const float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev, int64_t n, int step,
                         float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                         mpreid_stream_t stream);

/* ---- Stage-2 training (processor/processor_uniprompt_stage2.py:95-135): one optimizer step over a table of tensors, and the
 * scales of the split-precision re-pack that follows it ----
 * Both entry points take a HOST table of tensors.  Every tensor is cut into work chunks of MPREID_OPTIM_CHUNK elements and the
 * chunks of up to MPREID_OPTIM_TENSORS_PER_LAUNCH tensors go to ONE launch, whose tensor descriptors travel by value in the kernel
 * arguments: the table is read during the call and may be freed or changed right after it, nothing is uploaded.  A launch's grid is
 * capped at 2048 workgroups of 256 that stride over the chunks, so a large matrix and a bias of one launch share the chip.
 * Stream-ordered, no host synchronisation, no atomics; every argument error -- a NULL table, n_entries < 1, a NULL or not 4-byte
 * aligned pointer, n < 1 or >= 2^38, a class index out of range, a non-finite or negative lr or weight_decay, step < 1 -- is
 * MPREID_ERR_ARG before anything is launched.  Only the n elements of each buffer are read or written.
 *
 * mpreid_optim_step_multi_f32: one step of SGD with momentum, Adam or AdamW on every tensor of the table, in place.
 * entries[i].hyper picks one of n_classes <= MPREID_OPTIM_MAX_CLASSES {lr, weight_decay} classes (the reference's parameter
 * groups collapse to three: weights, biases, the large-FC weights).  Launches: mpreid_optim_step_launches(n_entries) =
 * ceil(n_entries / 64), 3 for the about 155 trained tensors of a dense ViT-B/16 (a launch is also closed at 2^30 chunks, which no
 * table that fits a device reaches).
 * ADAM / ADAMW: the constants and the per-element lines of mpreid_adam_step_f32 above, a and lw derived per class -- every tensor
 * is left BIT-IDENTICAL to one mpreid_adam_step_f32 call on it with its class's lr and weight_decay (ADAMW: decoupled != 0).
 * SGD: torch.optim.SGD(momentum = mu, dampening = 0, nesterov = False), mu >= 0 and finite; per element, each line rounded once:
 *   g = fmaf(weight_decay, p, grad)        buf = g at step 1, else buf = fmaf(mu, buf, g)        p = fmaf(-lr, buf, p)
 * state1_dev is buf (SGD) or exp_avg (Adam), state2_dev exp_avg_sq; SGD ignores state2_dev, which may be NULL; beta1, beta2 and eps
 * are ignored by SGD, momentum by the other two.  Groups of four elements go through 16-byte accesses where the four (SGD: three)
 * buffers of an entry are 16-byte aligned, one by one otherwise: the same bits.  No two buffers of the table may overlap. */
#define MPREID_OPTIM_SGD 0
#define MPREID_OPTIM_ADAM 1
#define MPREID_OPTIM_ADAMW 2
#define MPREID_OPTIM_MAX_CLASSES 8
#define MPREID_OPTIM_CHUNK 4096
#define MPREID_OPTIM_TENSORS_PER_LAUNCH 64
typedef struct {
    float *param_dev;
    const float *grad_dev;
    float *state1_dev, *state2_dev;
    int64_t n;
    int32_t hyper, reserved_;
} mpreid_optim_entry;
typedef struct {
    float lr, weight_decay;
} mpreid_optim_class;
int mpreid_optim_step_launches(int n_entries);   /* needs no device; 0 for n_entries < 1 */
int mpreid_optim_step_multi_f32(const mpreid_optim_entry *entries, int n_entries, const mpreid_optim_class *classes, int n_classes,
                                int algo, int step, float beta1, float beta2, float eps, float momentum, mpreid_stream_t stream);
/* mpreid_absmax_multi_f32: out_dev[i] = the largest finite |x| of tensor i; NaN and +-Inf count as 0 (an all-NaN tensor gives 0.0) --
 * torch.nan_to_num(src, 0, 0, 0).abs().max(), and a maximum does not depend on the order: the bits are defined.  Two fixed levels:
 * one partial per chunk into the workspace, then one workgroup per tensor over its partials; every out_dev[i] is written.
 * Launches: 2 per 64 tensors.  The workspace (256-byte aligned) holds one float per chunk of the table. */
typedef struct {
    const float *src_dev;
    int64_t n;
} mpreid_absmax_entry;
size_t mpreid_absmax_multi_workspace_bytes(const mpreid_absmax_entry *entries, int n_entries);   /* needs no device; 0 for a bad table */
int mpreid_absmax_multi_f32(const mpreid_absmax_entry *entries, int n_entries, float *out_dev /* [n_entries] */, void *ws_dev,
                            size_t ws_bytes, mpreid_stream_t stream);

/* ---- Stage-2 head (processor/processor_uniprompt_stage2.py:114-119, loss/make_loss.py): BNNeck in training mode, the bias-free
 * classifiers, the label-smoothed identity loss, the batch-hard triplet loss, and their gradients ----
 * Small fp32 entry points between the tower's output features and the scalar loss.  No atomics and a fixed summation order: the
 * same bits from run to run.  Every output element is written and no other byte; every argument error is found before anything
 * is launched; stream-ordered, no host synchronisation; a NULL optional output is not computed and leaves the other outputs'
 * bits unchanged.  Float and int32 buffers 4-byte aligned, labels 8, the workspace 256.  Inputs are taken to be finite.
 *
 * Row cross-entropy with label smoothing (loss/softmax_loss.py:24-35; epsilon = 0: F.cross_entropy with mean reduction).
 * K = classes, t_ac = (1 - epsilon) [c == y_a] + epsilon / K, logp_ac = (x_ac - max_a) - log sum_c exp(x_ac - max_a):
 *   row_loss[a] = -sum_c t_ac logp_ac = (1 - epsilon) (lse_a - (x_ay - max_a)) + (epsilon / K) (K lse_a - sum_c (x_ac - max_a))
 *   loss = (scale / rows) sum_a row_loss[a]          d_logits_ac = (scale / rows) (p_ac - t_ac)          argmax[a] = lowest index of max_a
 * (the target of the label's class is computed as 1 - epsilon (K - 1) / K: exactly 1 at K = 1, where loss and gradient are 0.0;
 * the exp sum leaves out the maximum's own term, exactly 1, and lse_a = log1p of the rest; at the maximum's class p - t is formed
 * from q = rest / (1 + rest) = 1 - p, so a row whose label holds nearly all the probability keeps its digits).
 * One workgroup of 256 threads per row, looping over the classes: any classes >= 1.  Summation order: thread t adds the entries
 * t, t + 256, ... ascending, butterfly 32, 16, 8, 4, 2, 1 per wave, then the four wave sums in order; the loss the same over the rows.
 * logits_dev [rows][classes] with leading dimension ld >= classes; d_logits_dev [rows][classes] dense, argmax_dev int32 [rows]: both
 * optional.  row_loss_dev [rows] is an output.  LIMIT: the CONTENTS of labels_dev are device data and are NOT checked here (the
 * caller does: mpreid.ops.xent_rows); a label outside 0 .. classes - 1 belongs to no class -- its one-hot term is absent from
 * loss and gradient -- and is never used as an address. */
int mpreid_xent_rows_f32(const float *logits_dev, int64_t ld, const int64_t *labels_dev, int rows, int classes, float epsilon,
                         float scale, float *loss_dev /* [1] */, float *row_loss_dev, float *d_logits_dev, int32_t *argmax_dev,
                         mpreid_stream_t stream);
/* Batch-hard triplet loss (loss/triplet_loss.py:51-134 with its default arguments, normalize_feature = False).
 *   d_ab = sqrt(max(sum_e (x_ae - x_be)^2, 1e-12)), ONE fmaf chain over the features, ascending
 * DIFFERENCE from the reference: its euclidean_dist forms |x_a|^2 + |x_b|^2 - 2 x_a . x_b, which in fp32 loses the digits of close
 * pairs (on the diagonal it gives noise of the order of 1e-3 where the exact value is the clamp, 1e-6); this is the
 * exact-arithmetic value of that expression.
 * Per anchor a: p = the largest d_ab among the rows with the anchor's label (the anchor included, as in the reference), n = the
 * smallest among the others, ties to the lowest index (lane l of one wave scans b = l, l + 64, ... ascending, then the butterfly);
 * ap = d_ap (1 + hard_factor), an = d_an (1 - hard_factor), these are dist_ap / dist_an;
 *   soft_margin == 0: term = max(0, ap - an + margin), w = [ap - an + margin > 0]
 *   soft_margin != 0: term = log(1 + exp(ap - an)) = max(z, 0) + log1p(exp(-|z|)), w = sigmoid(ap - an)       (margin unused)
 *   loss = (scale / B) sum_a term_a  (summed as above: thread t of 256, butterfly, four waves)
 *   d_feat = sum_a (scale / B) w_a ((1 + hard_factor) (x_a - x_p) / d_ap  [rows a: +, p: -]  -  (1 - hard_factor) (x_a - x_n) / d_an  [a: +, n: -])
 * a pair whose squared distance is below 1e-12 contributes nothing (the clamp).  d_feat row r is written by one workgroup that
 * walks the anchors in ascending order and adds, one fmaf each, what r receives as that anchor (positive term, negative term),
 * as its positive, as its negative.  An anchor without any negative: n_idx = -1, dist_an = +inf, no loss and no gradient.
 * Unequal group sizes are answered (the reference's view(N, -1) raises there).
 * Limits: 1 <= batch <= MPREID_TRIPLET_MAX_BATCH (the [B][B] matrix lives in the workspace; above: MPREID_ERR_UNSUPPORTED),
 * dim >= 1.  The labels are only compared with each other: any int64 values.  d_feat_dev [batch][dim] is optional. */
#define MPREID_TRIPLET_MAX_BATCH 1024
size_t mpreid_triplet_workspace_bytes(int batch, int dim);   /* needs no device; 0 for a bad request */
int mpreid_triplet_hard_f32(const float *feat_dev /* [batch][dim] */, const int64_t *labels_dev, int batch, int dim, float margin,
                            int soft_margin, float hard_factor, float scale, float *loss_dev /* [1] */, float *dist_ap_dev,
                            float *dist_an_dev /* [batch] */, int32_t *p_idx_dev, int32_t *n_idx_dev /* [batch] */,
                            float *d_feat_dev, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);
/* nn.BatchNorm1d in training mode on x_dev [batch][dim], one thread per column, rows ascending:
 *   mean = (sum_b x) / B (sequential), var = (sum_b (x - mean)^2) / B (two-pass, one fmaf chain), invstd = 1 / sqrt(var + eps),
 *   y = fmaf((x - mean) * invstd, gamma, beta); mean_dev and invstd_dev [dim] are saved for the backward pass.
 * running_mean_dev / running_var_dev (both or neither) are updated in place: r += momentum (mean - r), with the unbiased
 * variance (sum_b (x - mean)^2) / (B - 1).  batch == 1 is refused (MPREID_ERR_ARG), as torch refuses it in training. */
int mpreid_bn1d_train_forward_f32(const float *x_dev, const float *gamma_dev, const float *beta_dev, int batch, int dim, float eps,
                                  float momentum, float *y_dev, float *mean_dev, float *invstd_dev, float *running_mean_dev,
                                  float *running_var_dev, mpreid_stream_t stream);
/* Its backward pass, xhat = (x - mean) * invstd recomputed: dgamma = sum_b dy xhat (one fmaf chain), dbeta = sum_b dy (optional),
 *   dx = (gamma invstd / B) ((B dy - sum dy) - xhat sum(dy xhat)) [+ dx_add, when given: another gradient of x, [batch][dim]]
 * dx_dev may not overlap any input. */
int mpreid_bn1d_train_backward_f32(const float *x_dev, const float *dy_dev, const float *gamma_dev, const float *mean_dev,
                                   const float *invstd_dev, const float *dx_add_dev, int batch, int dim, float *dx_dev,
                                   float *dgamma_dev, float *dbeta_dev, mpreid_stream_t stream);
/* The small fp32 matrix product behind a bias-free nn.Linear, on the vector units (not the matrix cores: bit-defined):
 *   C[m][n] = sum_k A(m, k) B(n, k),   A(m, k) = a_dev[m a_rs + k a_cs],   B(n, k) = b_dev[n b_rs + k b_cs],   C dense rows of ldc
 * each element ONE fmaf chain over k ascending from 0.0; c_add_dev (optional, laid out as C) is added to it last.  With f [B][D], W [C][D], dS [B][C]:
 *   S = f W^T: (f, D, 1, W, D, 1, B, C, D)      d_f = dS W: (dS, C, 1, W, 1, D, B, D, C)      dW = dS^T f: (dS, 1, C, f, 1, D, C, D, B)
 * Strides >= 1 in elements; c_dev may not overlap the inputs. */
int mpreid_matmul_f32(const float *a_dev, int64_t a_rs, int64_t a_cs, const float *b_dev, int64_t b_rs, int64_t b_cs, int m, int n,
                      int k, const float *c_add_dev, float *c_dev, int64_t ldc, mpreid_stream_t stream);
/* The total of a head step from its loss terms (each already carries its weight): terms_dev holds n_id identity terms, then
 * n_tri triplet terms, then n_i2t image-to-text terms (at most 64 in all), each group added in order from 0.0:
 *   out[1] = identity part, out[2] = triplet part, out[3] = image-to-text part, out[0] = out[3] + (out[1] + out[2]) */
int mpreid_stage2_total_f32(const float *terms_dev, int n_id, int n_tri, int n_i2t, float *out_dev /* [4] */,
                            mpreid_stream_t stream);

/* processor/processor_uniprompt_stage2.py:636-640: out[rows][dim] = mean over the views of
 * feats[n_views][rows][dim] (sequential sum in view order, true division), then F.normalize(p=2, dim=1,
 * eps=1e-12) when normalize != 0. */
int mpreid_tta_mean_f32(const float *feats_dev, int n_views, int64_t rows, int dim, int normalize, float *out_dev,
                        mpreid_stream_t stream);

/* T.Resize(cfg.INPUT.SIZE_TEST) of val_transforms (datasets/make_dataloader.py:57-58) for a ragged batch of decoded
 * uint8 RGB images: bit-exact with PIL.Image.resize((out_w, out_h), BILINEAR) (Pillow 8-bit two-pass resample,
 * which is what torchvision's Resize calls for PIL inputs).  Image b is src_dev[offsets_dev[b] ...] as [h][w][3]
 * with (h, w) = hw_dev[2b], hw_dev[2b+1]; max_in_h >= every h.  dst_dev is [batch][out_h][out_w][3], the input
 * layout of mpreid_image_in.u8_hwc_dev. */
size_t mpreid_resize_workspace_bytes(int batch, int max_in_h, int out_w);
int mpreid_resize_bilinear_u8(const uint8_t *src_dev, const int64_t *offsets_dev, const int32_t *hw_dev, int batch,
                              int max_in_h, int out_h, int out_w, uint8_t *dst_dev, void *ws_dev, size_t ws_bytes,
                              mpreid_stream_t stream);
/* The same resample with a filter argument: MPREID_RESIZE_BILINEAR is mpreid_resize_bilinear_u8 bit for bit;
 * MPREID_RESIZE_BICUBIC is T.Resize(cfg.INPUT.SIZE_TRAIN, interpolation=3) of train_transforms
 * (datasets/make_dataloader_uniprompt.py:54), bit-exact with PIL.Image.resize((out_w, out_h), BICUBIC): bicubic_filter with
 * a = -0.5, support 2 x filterscale, a negative coefficient rounded as (int)(-0.5 + w * 2^22), overshoot clamped to 0 .. 255.
 * Any other filter is MPREID_ERR_ARG; the workspace is the one of mpreid_resize_workspace_bytes. */
#define MPREID_RESIZE_BILINEAR 0
#define MPREID_RESIZE_BICUBIC 1
int mpreid_resize_u8(const uint8_t *src_dev, const int64_t *offsets_dev, const int32_t *hw_dev, int batch, int max_in_h,
                     int out_h, int out_w, int filter, uint8_t *dst_dev, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);

/* ---- The random part of train_transforms (datasets/make_dataloader_uniprompt.py:55-60) on a batch that is already resized:
 * RandomHorizontalFlip, Pad(pad), RandomCrop(H x W), ToTensor, Normalize and timm's RandomErasing(mode='pixel', max_count=1)
 * in ONE kernel.  Every random decision is taken on the host and arrives in params (HOST, int32 [batch][8]):
 *   {flip, crop_top, crop_left, erase_top, erase_left, erase_h, erase_w, 0}        erase_h == 0: no erasing
 * The value of out[b][c][y][x]:
 *   (y, x) in the erase box   a standard normal: Philox4x32-10 with key (seed lo, seed hi) and counter (q lo, q hi,
 *                             sample_id[b] lo, sample_id[b] hi), e = (c * erase_h + (y - erase_top)) * erase_w + (x - erase_left)
 *                             the element's index in the (3, erase_h, erase_w) box, q = e >> 2, output word e & 3.  Words 0/1 and
 *                             2/3 are Box-Muller pairs: u1 = ((w_a >> 8) + 1) * 2^-24, u2 = (w_b >> 8) * 2^-24, the even word
 *                             takes sqrt(-2 ln u1) * cos(2 pi u2), the odd word the sine.  The noise depends on (seed, sample_id,
 *                             box) only, not on the batch or the position in it.  (timm fills the box from torch's CPU generator:
 *                             these are i.i.d. N(0, 1) values, not those bits.)
 *   otherwise                 sy = y + crop_top - pad, sx = x + crop_left - pad; outside the image the padded pixel, uint8 0;
 *                             inside img[b][sy][flip ? W - 1 - sx : sx][c]; then ((v / 255) - mean[c]) / std[c] in fp32 with two
 *                             correctly rounded divisions, the rule of mpreid_image_in's uint8 input.
 * img_hwc_dev uint8 [batch][H][W][3], out_dev fp32 [batch][3][H][W]; sample_id, mean[3] and std[3] are HOST arrays.  Every row
 * is checked before the first launch -- flip in {0, 1}; 0 <= crop_top, crop_left <= 2 pad; erase_h in [0, H), erase_w in
 * [0, W), both zero or neither, the box inside the image; the last field 0 -- and a violation is MPREID_ERR_ARG with a message
 * that names the image and the field; nothing is launched then.  The table travels by value in the kernel arguments,
 * MPREID_AUG_IMAGES_PER_LAUNCH images per launch (no upload, no workspace); stream-ordered, no host synchronisation. */
#define MPREID_AUG_IMAGES_PER_LAUNCH 64
int mpreid_train_augment_f32(const uint8_t *img_hwc_dev, int batch, int H, int W, int pad, const int32_t *params,
                             const int64_t *sample_id, uint64_t seed, const float *mean, const float *std, float *out_dev,
                             mpreid_stream_t stream);

/* ---- CLIP "RN50" image encoder (MODEL.NAME == 'RN50': model/clip/model.py:10-148 ModifiedResNet, Bottleneck,
 * AttentionPool2d) + the RN50 eval branch of build_transformer.forward (model/make_model.py:82-86, 102-115):
 * out = cat(avg_pool2d(x4), attnpool(x4)[0]) (after the eval BatchNorm necks for NECK_FEAT == 'after').
 * NHWC fp16 activations, every conv an implicit MFMA GEMM with its BatchNorm folded in (see
 * mpreid_conv_f16_nhwc), residual add + ReLU in the GEMM epilogue. ---- */
typedef struct { /* one folded convolution; device pointers */
    const void *w;        /* fp16 [cout_pad][taps*cin], k order (kh, kw, c) */
    const float *bias;    /* fp32 [cout_pad] */
    int32_t cin, cout, cout_pad, taps;  /* cin % 64 == 0, cout % 8 == 0, cout_pad % 128 == 0, taps 1 or 9 */
} mpreid_rn50_conv;

typedef struct { /* Bottleneck (model/clip/model.py:10-53) */
    mpreid_rn50_conv conv1, conv2, conv3, down;  /* down.w == NULL when the block has no downsample branch */
    int32_t stride;                              /* AvgPool2d(stride) after conv2 and in front of down: 1 or 2 */
} mpreid_rn50_block;

typedef struct {
    int32_t img_h, img_w;   /* multiples of 32 */
    int32_t width;          /* 64: stem 32/32/64 channels, layers 64/128/256/512 planes */
    int32_t n_blocks;       /* sum of the layers tuple (3+4+6+3 = 16) */
    int32_t heads, out_dim; /* attention pool: embed dim = 32*width, heads, output_dim (1024) */
} mpreid_rn50_cfg;
/* Limits: attention-pool tokens T = (img_h / 16) * (img_w / 16) + 1 <= MPREID_RN50_MAX_TOKENS (1025, 512 x 512) for
 * mpreid_rn50_forward (the fp16 tower) -> MPREID_ERR_UNSUPPORTED above that.  Its pool keeps the [T][heads] score table in
 * LDS beside the u vectors while that fits (T <= 252 at width 64), and passes it through the workspace above.  The split
 * and fp32 towers (one-query pool with T floats of LDS per (image, head)) take any T up to 40 960. */
#define MPREID_RN50_MAX_TOKENS 1025

typedef struct { /* device pointers unless noted */
    const float *stem1_w;   /* conv1+bn1 folded, fp32 [width/2][3][3][3] = [cout][c][kh][kw] */
    const float *stem1_b;   /* fp32 [width/2] */
    mpreid_rn50_conv stem2, stem3;          /* cin = cout = 64 storage channels (32 real ones in stem2) */
    const mpreid_rn50_block *blocks;        /* HOST array of n_blocks entries */
    const float *pos_emb;                   /* attnpool.positional_embedding fp32 [S+1][E] */
    const void *kt_w;                       /* fp16 [E][E] = k_proj.weight TRANSPOSED (k_proj.bias cancels in the softmax) */
    const void *v_w; const float *v_b;      /* fp16 [E][E] = v_proj.weight, fp32 [E] */
    const void *q_w; const float *q_b;      /* fp16 [E][E], fp32 [E] */
    const void *c_w; const float *c_b;      /* fp16 [out_pad128][E], fp32 [out_pad128] */
    const float *bn_scale, *bn_shift;       /* eval BN necks folded, fp32 [E + out_dim], or NULL */
} mpreid_rn50_weights;

size_t mpreid_rn50_workspace_bytes(const mpreid_rn50_cfg *cfg, int batch);
/* img: the batch (mpreid_image_in above); this tower has no in-kernel view: view != 0 -> MPREID_ERR_UNSUPPORTED (the split
 * and fp32 towers below take every view).  out_dev [B][32*width + out_dim] fp32. */
int mpreid_rn50_forward(const mpreid_rn50_cfg *cfg, const mpreid_rn50_weights *w, const mpreid_image_in *img, int batch,
                        float *out_dev, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);

/* All-fp32 mode of the RN50 tower (MODEL.NAME 'RN50' + MODEL.ENCODER_PRECISION 'fp32'; the reference runs the tower in
 * fp32): fp32 NHWC activations, every convolution a GEMM on the exact fp32 matrix instruction (3x3: im2col, k order
 * (kh, kw, c)), BatchNorm folded on the host, fp32 attention pool -- relative feature error ~1e-6 against the fp32 CPU path
 * instead of the fp16 tower's 2.6e-3, at ~1/10 of its throughput.  Weight matrices are fp32 [cout][taps*cin] with the REAL
 * channel counts (no padding). */
typedef struct { const float *w; const float *bias; int32_t cin, cout, taps; } mpreid_rn50_conv_f32;
typedef struct { mpreid_rn50_conv_f32 conv1, conv2, conv3, down; int32_t stride; } mpreid_rn50_block_f32;  /* down.w NULL: none */
typedef struct {
    const float *stem1_w, *stem1_b;              /* conv1+bn1 folded, [width/2][3][3][3], [width/2] */
    mpreid_rn50_conv_f32 stem2, stem3;
    const mpreid_rn50_block_f32 *blocks;         /* HOST array of n_blocks entries */
    const float *pos_emb;                        /* [S+1][E] */
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b;   /* [E][E], [E] */
    const float *c_w, *c_b;                      /* [out_dim][E], [out_dim] */
    const float *bn_scale, *bn_shift;            /* eval BN necks folded, [E + out_dim], or NULL */
} mpreid_rn50_weights_f32;
size_t mpreid_rn50_workspace_bytes_f32(const mpreid_rn50_cfg *cfg, int batch);
int mpreid_rn50_forward_f32(const mpreid_rn50_cfg *cfg, const mpreid_rn50_weights_f32 *w, const mpreid_image_in *img, int batch,
                            float *out_dev, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);

/* SPLIT-precision mode of the RN50 tower (MODEL.NAME 'RN50' + MODEL.ENCODER_PRECISION 'split', the default): fp32 NHWC
 * activations; the convolutions of layer1-4 and the attention pool's k / v projections run on the fp16 matrix cores over
 * fp16 PAIRS hi + lo, three products per multiply-add with fp32 accumulation (the GE_S_* GEMMs of the ViT's split mode):
 * fp32-grade features at several times the all-fp32 mode's throughput.  The stem's first convolution (K = 27), the one-query attention and the 1-row
 * projections q / c stay on the exact fp32 path (`f32`: stem1_*, pos_emb, q_*, c_*, bn_* are read; its stem2 / stem3 /
 * blocks / k_* / v_* are not).  A split convolution: w = fp16 pair matrix [npad][2 * kseg] = [hi(kseg) | lo(kseg)] of the
 * BatchNorm-folded weights [cout][taps * cin] (k order (kh, kw, c)) times 2^e, zero-padded to kseg = taps * cin rounded up to
 * 64 columns and npad = cout rounded up to 128 rows (mpreid_split_pack_f32); bias fp32 [npad] (zero past cout);
 * oscale = 2^-e.  cin % 4 == 0.  Range: as for the ViT's split mode (activations below 65 504).
 * taps == 9 (the 3x3 convolutions run as IMPLICIT GEMMs over the nine shifted views of the pair activations, no im2col
 * matrix): kseg = cin rounded up to 64 (the padded channel count of ONE tap) and w = fp16 slabs
 * [npad][tap = kh*3+kw][kseg / 64][hi(64) | lo(64)] of W * 2^e (channels >= cin and rows >= cout zero). */
typedef struct { const void *w; const float *bias; int32_t cin, cout, taps, kseg, npad; float oscale; } mpreid_rn50_conv_split;
typedef struct { mpreid_rn50_conv_split conv1, conv2, conv3, down; int32_t stride; } mpreid_rn50_block_split;   /* down.w NULL: none */
typedef struct {
    mpreid_rn50_weights_f32 f32;
    const mpreid_rn50_block_split *blocks;       /* HOST array of n_blocks entries */
    mpreid_rn50_conv_split k, v;                 /* attention pool k_proj / v_proj as 1x1 "convolutions" over the tokens */
    mpreid_rn50_conv_split stem2, stem3;         /* the stem's second and third convolution (f32.stem2 / stem3 are not read) */
} mpreid_rn50_weights_split;
size_t mpreid_rn50_workspace_bytes_split(const mpreid_rn50_cfg *cfg, int batch);
int mpreid_rn50_forward_split(const mpreid_rn50_cfg *cfg, const mpreid_rn50_weights_split *w, const mpreid_image_in *img, int batch,
                              float *out_dev, void *ws_dev, size_t ws_bytes, mpreid_stream_t stream);

/* One convolution layer of the RN50 tower as the encoder runs it (unit tests, micro-benchmarks):
 * NHWC fp16 in [batch][h][w][cin] (cin % 64 == 0), stride 1, taps = 1 (1x1) or 9 (3x3, pad 1); weights fp16
 * [cout_pad][taps*cin] (k order: tap = kh*3+kw, then channel; cout_pad % 128 == 0, rows >= cout zero) with the
 * BatchNorm of model/clip/model.py:17-24 folded in, bias fp32 [cout_pad]; optional fp16 identity [M][cout] added
 * before the ReLU (Bottleneck.forward, model/clip/model.py:39-53); out fp16 [batch*h*w][cout]; zero_page_dev =
 * 128 bytes of zeros. */
int mpreid_conv_f16_nhwc(const void *act_dev, int batch, int h, int w, int cin, const void *wgt_dev, const float *bias_dev,
                         int cout, int cout_pad, int taps, const void *identity_dev, int relu, void *out_dev,
                         const void *zero_page_dev, mpreid_stream_t stream);

/* One convolution of the SPLIT-precision RN50 tower as mpreid_rn50_forward_split runs it (unit tests, micro-benchmarks):
 * the tower's own layer routine behind a C entry point, every operand and output form it has.  M = batch * h * w
 * pixels; every row count is padded to Mp = M rounded up to 256.  conv: weights in the layouts documented at
 * mpreid_rn50_conv_split above, taps 1 or 9 (stride 1, pad 1).
 * Operand -- exactly one of
 *   in_dev         fp32 NHWC [M][ld_in], the first conv->cin channels real (ld_in >= cin, ld_in % 4 == 0, 16-byte aligned;
 *                  channels >= cin are not read); relu_in != 0: max(x, 0) is applied on the way.  Packed into
 *                  pair_scratch_dev, fp16 [Mp][2 * kseg] = [hi(kseg) | lo(kseg)], rows >= M and channels >= cin zero
 *   in_pairs_dev   that pair matrix, delivered by the caller (taps 1: all Mp rows are read; taps 9: rows < M);
 *                  ld_in / relu_in / pair_scratch_dev are ignored
 * Output, y = acc * oscale + bias with acc = sum over k of hi.hi' + lo.hi' + hi.lo' in fp32:
 *   res 0, out_pairs_dev NULL      out_dev fp32 [Mp][npad] = y
 *   res 1 (taps 1)                 out_dev += y;    res 2 (taps 1): out_dev = max(out_dev, 0) + y (the destination is a
 *                                  block input whose ReLU was never written back)
 *   res 0, out_pairs_dev           fp16 pairs [Mp][2 * pair_c] = [hi | lo] of relu(y), hi = fp16(v), lo = fp16(v - hi);
 *                                  columns [cout, pair_c) zero in both halves; out_dev is not touched (may be NULL).
 *                                  pair_c % 64 == 0, cout <= pair_c <= npad (taps 9: pair_c == 64 when cout <= 64, else
 *                                  pair_c <= cout rounded up to 128)
 *   res 1 / 2, out_pairs_dev       (taps 1, pair_c == npad) out_dev as above AND the pairs of relu(out_dev)
 * Rows: taps 1 computes all Mp rows -- fp32 rows and pair rows in [M, Mp) ARE written (y of the zero rows of the packed
 * operand, i.e. the bias, or whatever rows [M, Mp) of in_pairs_dev hold); taps 9 writes rows < M only.  All npad
 * (2 * pair_c) columns of a written row are written, with one exception: a taps 9 convolution with cout <= 64 runs in ONE
 * 64-wide tile and writes fp32 columns [0, 64) only (the tower never reads a padded column).  Written fp32 columns
 * >= cout hold y of the zero weight rows (0 + bias 0).
 * zero_page_dev: 256 bytes of zeros (taps 9; may be NULL for taps 1).  Argument errors: MPREID_ERR_ARG; those on the
 * operand, res and the pair output's shape are found before anything is launched, the remaining ones of the GEMM
 * launchers (alignment, sizes) after the pack of in_dev into pair_scratch_dev has been queued. */
int mpreid_rn50_conv_split_layer(const mpreid_rn50_conv_split *conv, const float *in_dev, int ld_in, int relu_in,
                                 const void *in_pairs_dev, int batch, int h, int w, int res, float *out_dev, void *out_pairs_dev,
                                 int pair_c, void *pair_scratch_dev, const void *zero_page_dev, mpreid_stream_t stream);

/* fp16 GEMM used by the encoder, exposed for the roofline bench and unit tests:
 * C[M][N] (fp32) = A[M][K] (fp16) x B[N][K]^T (fp16).  M, N multiples of 128... see DESIGN.md. */
int mpreid_gemm_f16_nt(const void *a_dev, const void *b_dev, float *c_dev, int64_t m, int64_t n, int64_t k,
                       mpreid_stream_t stream);
/* same GEMM with a fused epilogue: 0 = fp32 out, 1 = +bias -> fp16, 2 = out(fp32) += acc + bias,
 * 3 = QuickGELU(acc + bias) -> fp16, 7 = relu(acc + bias) -> fp16, 8 = out(fp16) = relu(acc + bias + out), one
 * rounding (the RN50 1x1 convolutions).  Used by the unit tests and tools/gemm_bench.py. */
int mpreid_gemm_f16_nt_ex(const void *a_dev, const void *b_dev, void *out_dev, const float *bias_dev, int64_t m,
                          int64_t n, int64_t k, int epilogue, mpreid_stream_t stream);
/* The linear layer of the encoder's SPLIT precision mode, exposed for unit tests and tools/gemm_bench.py:
 * a2 [M][2*kseg], b2 [N][2*kseg] fp16 pairs [hi | lo]; acc = sum over k of hi.hi' + lo.hi' + hi.lo' (fp32);
 * epilogue 10: out fp32 [M][N] = acc*oscale + bias; 11: out fp32 [M][N] += acc*oscale + bias;
 * 12: out fp16 pair [M][2N] = hi | lo of QuickGELU(acc*oscale + bias). */
int mpreid_gemm_f16_split_nt(const void *a2_dev, const void *b2_dev, void *out_dev, const float *bias_dev, int64_t m,
                             int64_t n, int64_t kseg, float oscale, int epilogue, mpreid_stream_t stream);
/* x [rows][cols] fp32 -> y [rows][2*cols] fp16 pair: hi = fp16(x*scale), lo = fp16(x*scale - hi); scale a power of two */
int mpreid_split_pack_f32(const float *x_dev, int64_t rows, int cols, float scale, void *y_dev, mpreid_stream_t stream);
/* fp32 -> fp16 (RNE) conversion of a flat array */
int mpreid_cast_f32_to_f16(const float *x_dev, void *y_dev, int64_t n, mpreid_stream_t stream);

/* ---- measurement hooks (bench.py roofline leg) --------------------------------------------- */
/* kernel classes of the encoder that are not fp16 GEMMs (mpreid_profile_entry.epilogue); flops_total then holds
 * ALGORITHMIC BYTES for the HBM-bound ones (layer norm: 4 B read + output bytes per element; attention: q, k, v read +
 * output written) */
#define MPREID_PROF_LAYERNORM 100
#define MPREID_PROF_ATTENTION 101
#define MPREID_PROF_EVALRANK 102   /* eval_rank_kernel: m = nq, n = ng; work = 4*nq*ng bytes (the matrix read once).  The splits
                                    * entry point files m = pairs, n = n_cols, k = n_splits; work = 4 * sum over the pairs of the
                                    * pair's gallery list length (the gathered distances) */
/* the MoE kernels (csrc/moe.hip): m = token rows, n = num_experts, k = top_k (the grouped GEMMs: n = N, k = 2 * kseg).  The
 * work figure is 0: the slot count is device data -- tools/moe_bench.py computes 2 * slots * N * 3 * kseg from the routing. */
#define MPREID_PROF_MOE_ROUTER 110
#define MPREID_PROF_MOE_DISPATCH 111   /* the three dispatch launches together */
#define MPREID_PROF_MOE_FC1 112
#define MPREID_PROF_MOE_FC2 113
#define MPREID_PROF_MOE_COMBINE 114
/* the MoE gradient kernels (csrc/moe_grad.hip); the grouped fp32 GEMMs: n = N, k = K, work 0 as above (2 * slots * N * K) */
#define MPREID_PROF_MOE_GRAD_U 115         /* FC1 once more through the fp32 epilogue: the pre-activation u */
#define MPREID_PROF_MOE_GRAD_DW 116
#define MPREID_PROF_MOE_GRAD_DT 117        /* (w dy) . Wproj_e times QuickGELU'(u) */
#define MPREID_PROF_MOE_GRAD_DH 118        /* du . Wfc_e */
#define MPREID_PROF_MOE_GRAD_COMBINE 119
#define MPREID_PROF_MOE_GRAD_ROUTER 120    /* the router gradient's launches together */
typedef struct {
    int32_t epilogue;        /* GemmEpi id of the fp16 GEMM class, or MPREID_PROF_* */
    int32_t n, k;            /* GEMM N and K (split epilogues: K = 2 * kseg halfs per operand row; 3 * kseg is executed) */
    int64_t m;               /* GEMM M (padded rows): classes are keyed by (epilogue, M, N, K) */
    int64_t launches;        /* launches recorded while profiling was enabled */
    double total_ms;         /* sum of per-launch durations (hipEvents on the launch stream) */
    double flops_total;      /* sum over the recorded launches of 2*M*N*K */
} mpreid_profile_entry;
/* While enabled, every fp16 GEMM launch is bracketed by two hipEvents on its stream. */
int mpreid_profile_enable(int on);
int mpreid_profile_reset(void);
/* Synchronises the recorded events; entries sorted by total time, returns the class count. */
int mpreid_profile_query(mpreid_profile_entry *out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* MPREID_H */
