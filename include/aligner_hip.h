/*
 * aligner_hip.h -- C ABI of the MI355X-native DP matrix-fill + traceback path.
 *
 * This is the drop-in boundary for ONE hot path of ikramanop/aligner: the pairwise-alignment DP fill and
 * traceback behind `AlignerTrait::perform_alignment` (aligner-core/src/lib.rs:27-40), implemented by
 * `SimpleGlobalAligner` / `SimpleLocalAligner` (aligner-core/src/simple/mod.rs:42-145, :168-264) and by the
 * legacy `SimpleAligner::{global,local}_alignment` (src/align/aligner_core.rs:96-183, :185-269).
 * The reference has no FFI of its own; a thin Rust shim implements `AlignerTrait` for
 * `Hip{Global,Local}Aligner<T>` on top of these entry points.  Plain pointers and sizes only; the library never
 * frees caller memory and never returns owned pointers other than the opaque handles below.
 *
 * Conventions (same as the reference): query = columns (x, length N), target = rows (y, length M); the substitution
 * lookup is matrix[[target_code, query_code]] (simple/mod.rs:85,198); residues are one byte holding the enum
 * discriminant (`Into<usize>`, enums.rs:98-102,149-153); direction codes are the `Direction` discriminants
 * Top=0, Left=1, Diagonal=2, Beginning=3 (enums.rs:9-15).
 */
#ifndef ALIGNER_HIP_H
#define ALIGNER_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ALN_ABI_VERSION 2

/* Which reference routine is reproduced bit-for-bit. */
enum aln_semantics {
    ALN_CORE_GLOBAL = 0,   /* SimpleGlobalAligner::perform_alignment   simple/mod.rs:42-145  */
    ALN_CORE_LOCAL = 1,    /* SimpleLocalAligner::perform_alignment    simple/mod.rs:168-264 */
    ALN_LEGACY_GLOBAL = 2, /* SimpleAligner::global_alignment          src/align/aligner_core.rs:96-183  */
    ALN_LEGACY_LOCAL = 3,  /* SimpleAligner::local_alignment           src/align/aligner_core.rs:185-269 */
    ALN_PWM_LOCAL = 4      /* PWMAligner::perform_alignment            aligner-core/src/pwm/mod.rs:29-126:
                            * `target` = the aligner's query (rows), matrix = 4 x W position-weight matrix whose column x scores
                            * PWM position x; `query` is ignored (N = W).  Aligned output: q_aln holds uint32_t PWM column
                            * numbers (0 = gap; capacity N+M+2 entries, 4-byte aligned), t_aln the residue codes / blank. */
};

/* Status codes.  1 mirrors `Err(Error::UnnecessaryArgument)` (lib.rs:51; simple/mod.rs:49-51,175-177).
 * 2..4 are conditions on which the reference PANICS; a drop-in shim maps them back to panic!(). */
enum aln_status {
    ALN_OK = 0,
    ALN_ERR_UNNECESSARY_ARGUMENT = 1,
    ALN_ERR_EMPTY_SEQUENCE = 2,      /* last().unwrap() on an empty Vec      simple/mod.rs:103-104        */
    ALN_ERR_CODE_OUT_OF_RANGE = 3,   /* ndarray index out of bounds          simple/mod.rs:85,198         */
    ALN_ERR_NO_POSITIVE_CELL = 4,    /* argmax on a border -> usize underflow simple/mod.rs:214-215       */
    ALN_ERR_DEVICE = 5,              /* HIP runtime / kernel failure (aln_last_error() has the text)      */
    ALN_ERR_OOM = 6,
    ALN_ERR_INVALID_ARGUMENT = 7,
    ALN_ERR_UNSUPPORTED = 8,
    ALN_ERR_MATRIX_SHAPE = 9,        /* Err(Error::MatrixShapeError): PWM without exactly 4 rows, pwm/mod.rs:40-42 */
    ALN_ERR_CAPACITY = 10            /* aln_scan_select: more windows passed than the caller's capacity holds (the count is the true one) */
};

/* What the caller wants back (bitmask in aln_params.outputs). */
enum aln_outputs {
    ALN_OUT_SCORE = 1,       /* f / score / end cell */
    ALN_OUT_TRACEBACK = 2,   /* aligned code strings, start cell, aln_len */
    ALN_OUT_DIRECTIONS = 4,  /* (M+1)x(N+1) Direction bytes = AlignmentResult.direction_matrix (pair API only) */
    ALN_OUT_H_MATRIX = 8     /* (M+1)x(N+1) f64 = AlignmentResult.alignment_matrix (pair API only; generic kernels: 1.2 ms for a 1k x 1k pair against 0.3 ms without) */
};

/* Arguments of perform_alignment(del, ext, matrix, heuristics) + the output selection. */
typedef struct aln_params {
    int32_t semantics;          /* enum aln_semantics */
    int32_t heuristics_present; /* Some(Heuristics) -> ALN_ERR_UNNECESSARY_ARGUMENT for the core semantics */
    double del;                 /* gap opening ("deletions"); the single i32 gap cost for the legacy semantics */
    double ext;                 /* gap extension; ignored by the legacy semantics */
    const double *matrix;       /* host pointer, element [t][q] at matrix[t*row_stride + q] */
    uint32_t rows, cols;        /* matrix shape; codes >= shape -> ALN_ERR_CODE_OUT_OF_RANGE */
    int64_t row_stride;         /* in elements (ndarray stride of axis 0) */
    uint32_t outputs;           /* bitmask of enum aln_outputs; 0 = SCORE|TRACEBACK */
    uint8_t blank_code;         /* T::blank(): 98 for Protein and DNA (enums.rs:81,144) */
    uint8_t force_f64;          /* 1: run the f64 kernels even if the inputs are integral (testing) */
    uint8_t force_serial;       /* 1: run the strict reference-order kernel (one lane per pair; testing/fallback) */
    uint8_t force_generic;      /* 1: run the generic (non-profiled) integer kernels (testing) */
    uint32_t max_passes;        /* CORE_LOCAL with del != ext: cap on speculative fills before the serial kernel; 0 = 4 */
} aln_params;

/* Fixed-size per-pair summary (48 bytes); also the record gathered across GPUs. */
typedef struct aln_pair_result {
    double f;                   /* Alignment.f: 0.0 for CORE_GLOBAL (simple/mod.rs:139), H max for local (:247) */
    double score;               /* H[M][N] for the global semantics, H max for the local ones */
    uint32_t end_y, end_x;      /* cell the traceback starts from (1-based matrix coordinates) */
    uint32_t start_y, start_x;  /* cell where the traceback loop stopped */
    uint32_t aln_len;           /* length of both aligned strings (includes the reference's duplicated seed pair) */
    int32_t status;             /* enum aln_status for this pair */
    uint32_t passes;            /* bits 0-6: full fill passes (1 unless CORE_LOCAL with del != ext); bit 7: strict-order fallback;
                                   bits 8-15: localized repairs of strip 0; bits 16-19: 1 + checkpoint at which the last one re-converged;
                                   bits 20-23: why a repair escalated to a full pass (1 hazard beyond the last checkpoint, 2 strip 0's
                                   bottom row moved, 3 no re-convergence, 4 repair limit); diagnostics only */
    uint32_t flags;             /* bit0: integer kernels were used (also for a real-valued scheme whose numbers are all multiples of
                                   2^-k, k <= 8: it is filled as the integer scheme times 2^k and f / score are scaled back, exactly); bit1: the strip-pipelined single-pair route;
                                   bit2: generic kernels, one workgroup per pair (real-valued matrix / H output, <= 4 pairs per call);
                                   bit3: the fast integer kernels (i32 keys 4*H + tag, int8 query profile) filled this pair -- the
                                   batch kernel, two pairs per wave, the single-pair route and their strict-order fallbacks */
} aln_pair_result;

typedef struct aln_ctx aln_ctx;      /* one per process: one GPU or a list of GPUs; thread-safe */
typedef struct aln_batch aln_batch;  /* a batch of pairs staged in HBM */

/* ---- context.  The reference runs its aligners on the caller's threads with no shared state (ten std::threads in
 * statistics/mod.rs:255-286); here every thread of the process shares one context.  A context owns, per GPU, a pool of
 * slots (device buffers, a stream, pinned staging) that calls lease -- nothing is allocated per call once the pool is warm.
 * aln_create: one GPU.  aln_create_multi: the listed GPUs of this process (n_devices = 0: every visible one); single calls go
 * to the devices in turn, a batch call is cut into chunks that the devices take from a common queue, and every device writes
 * its chunks' summaries and strings straight into the caller's host buffers over its own PCIe link (the host array IS the
 * gather; the multi-process form gathers device-side with RCCL, aligner_amd/distributed.py).
 * Creation warms the context (~0.1 s per GPU in all): the code objects are loaded and one synthetic 1000 x 1000 pair goes through
 * aln_align_pair, so that the first real call finds pool slot 0, its buffers and every kernel of that route in place (a first
 * 1000 x 1000 pair: 0.4 ms instead of 26-60; aligner-cli aligns one pair per process).  ALN_NO_WARMUP=1 leaves it to the first call. ---- */
aln_ctx *aln_create(int device_id, int *status);
aln_ctx *aln_create_multi(int n_devices, const int *device_ids, int *status);
int aln_device_count(const aln_ctx *ctx);
void aln_destroy(aln_ctx *ctx);
const char *aln_last_error(void);        /* thread-local text of the last ALN_ERR_DEVICE / _OOM */
int aln_abi_version(void);
int aln_device_info(aln_ctx *ctx, int *compute_units, size_t *hbm_bytes, char *name, size_t name_cap);   /* first device */

/* ---- one pair, blocking (replaces one perform_alignment call).  q_aln / t_aln: capacity N+M+2 bytes each.
 * directions: optional (M+1)*(N+1) bytes; h_matrix: optional (M+1)*(N+1) doubles. ---- */
int aln_align_pair(aln_ctx *ctx, const aln_params *params, const uint8_t *query, size_t N, const uint8_t *target,
                   size_t M, aln_pair_result *out, uint8_t *q_aln, uint8_t *t_aln, uint8_t *directions,
                   double *h_matrix);

/* ---- batch driver: semantics == map of aln_align_pair over independent pairs (the reference's only batch site is
 * statistics/mod.rs:255-286).  Pair i: query = seqs[q_off[i] .. +q_len[i]), target = seqs[t_off[i] .. +t_len[i]).
 * All pointers are HOST memory (any malloc'ed / Vec memory; nothing has to be pinned).  The call is a pipeline: the batch is
 * cut into chunks of the caller's pair order and chunk i+1 is uploaded, chunk i filled and traced back, chunk i-1 downloaded
 * at the same time; residues are checked against the matrix shape on the device.
 * tb_buf (optional): pair i's aligned query at tb_off[i], aligned target at tb_off[i] + q_len[i] + t_len[i] + 2; bytes of a
 * string's capacity beyond aln_len are unspecified.  Any tb_off is accepted; the cumulative layout
 * tb_off[i+1] = tb_off[i] + 2 * (q_len[i] + t_len[i] + 2) is copied back without a per-pair scatter.
 * ALN_PWM_LOCAL: q_len[i] is ignored (N = matrix cols); tb_off[i] must be a multiple of 4; pair i's uint32 column numbers
 * start at tb_off[i], its residue string at tb_off[i] + 4 * (cols + t_len[i] + 2). ---- */
int aln_align_batch(aln_ctx *ctx, const aln_params *params, const uint8_t *seqs, const uint64_t *q_off,
                    const uint64_t *q_len, const uint64_t *t_off, const uint64_t *t_len, size_t n_pairs,
                    aln_pair_result *results, uint8_t *tb_buf, const uint64_t *tb_off);

/* The chunks aln_align_batch cuts these pairs into on a context of n_devices GPUs (host arithmetic only; no GPU needed):
 * returns their number and writes up to cap (first pair, pair count) entries.  Chunks are ranges of the caller's pair order of
 * 5e9 .. 1.6e10 cells; the devices take them from a common queue. */
size_t aln_plan_chunks(const aln_params *params, const uint64_t *q_len, const uint64_t *t_len, size_t n_pairs, int n_devices,
                       uint64_t *first, uint64_t *count, size_t cap);

/* ---- staged form of the batch driver (one device: the context's first): inputs resident in HBM, results left in HBM
 * until fetched.
 * create = validate + H2D + allocate; run = fill (+ exact re-fills) + traceback, asynchronous on `stream`
 * (a hipStream_t passed as void*, NULL = the context's own stream); fetch = D2H. ---- */
aln_batch *aln_batch_create(aln_ctx *ctx, const aln_params *params, const uint8_t *seqs, const uint64_t *q_off,
                            const uint64_t *q_len, const uint64_t *t_off, const uint64_t *t_len, size_t n_pairs,
                            int *status);
int aln_batch_run(aln_batch *b, void *stream);
int aln_batch_sync(aln_batch *b);
int aln_batch_fetch(aln_batch *b, aln_pair_result *results, uint8_t *tb_buf, const uint64_t *tb_off);
void aln_batch_destroy(aln_batch *b);
uint64_t aln_batch_cells(const aln_batch *b);                 /* sum of M_i * N_i over valid pairs */
size_t aln_batch_size(const aln_batch *b);
void *aln_batch_results_device(aln_batch *b);                 /* device pointer: aln_pair_result[n_pairs] (for RCCL) */
uint64_t aln_batch_direction_bytes(const aln_batch *b);       /* bytes of packed directions one run writes */
/* mean kernel time per run since aln_batch_enable_timing(b, 1), from HIP events recorded on the launch stream
 * around the fill kernel and the traceback kernel (last 256 runs; call after aln_batch_sync) */
int aln_batch_timing(aln_batch *b, double *fill_ms, double *traceback_ms, uint32_t *fill_launches);
void aln_batch_enable_timing(aln_batch *b, int on);

/* ---- window scan (the repeat search's loop, latent-repeat-search engine/calc.rs:19-147): one residue array resident in HBM
 * (one device: the context's first), scanned again and again by ONE position-weight matrix (ALN_PWM_LOCAL only; anything else is
 * ALN_ERR_UNSUPPORTED).  A pass is a geometry: window k starts at j = first + k * step (every j < len) and holds the rows
 * seq[j .. min(j + width, len)) -- the last windows are truncated, not dropped; reverse = 1 reads the reversed strand (built on
 * the device from the resident one; the residues are uploaded once).  The window descriptors are expanded on the device and
 * filled by the same kernels aln_align_batch takes for the same windows.
 * create: residue codes must be < 4 (else ALN_ERR_CODE_OUT_OF_RANGE).  windows: their number for a geometry.
 * score: f of every window into f[windows] (8 bytes per window come back).
 * select: the same fill, then on the device z = (f - mean) / sd (IEEE division; NaN fails, +inf passes) and the windows with
 * z >= z_min in ascending window order; those are filled again with directions and walked on the same stream.  Returns the true
 * number of hits in *count and the first min(count, cap) of them: window indices, summaries and (tb_buf optional) strings, hit h's
 * at h * aln_scan_string_stride(...) in the ALN_PWM_LOCAL layout of aln_align_batch (u32 column numbers, then the residues at
 * 4 * (cols + that window's length + 2)).  The caller's buffers hold cap entries: 4 * cap bytes of indices, 48 * cap of results,
 * cap * aln_scan_string_stride(...) of tb_buf; nothing beyond entry min(count, cap) - 1 is written.  count > cap: ALN_ERR_CAPACITY.
 * params->outputs is ignored.
 * hits: a HELD select pass.  Fill, z test and compaction exactly as select; the count is read where the pass waits anyway, the
 * hit buffers are sized for it (no capacity, no second fill; ALN_ERR_OOM and nothing held if that memory cannot be had) and ALL
 * hits are filled again with directions and walked.  Summaries, strings and the hit list stay on the device; only *count comes
 * back (8 bytes device -> host).  The hit set, its order, every summary and every string are select's for the same arguments with
 * enough capacity.  A failed window fails the call with its status, as in select, and nothing is held.  Held state belongs to
 * the scan and lasts until the next score / select / hits on it or destroy.
 * held_list: window index and f of held hits first .. first + n - 1 (ascending window order); 12 * n bytes come back.
 * held_frequencies: counts[c * cols + (col - 1)] = the number of listed hits whose alignment puts residue c on PWM column col
 * (1-based), over positions whose column number is not 0 and whose residue is not Blank: the sum of the hits' frequency matrices
 * (alignment.rs:55-65), accumulated on the device in unsigned integers, so exact and the same in any order.  keep[] are positions
 * in the held list in any order; a position listed twice counts twice; n_keep == 0 gives zeros.  4 * n_keep bytes go up,
 * 32 * cols come back.
 * held_strings: summaries and strings of the listed held hits, entry k's strings at k * aln_scan_string_stride(...), layout of
 * select; 4 * n_keep bytes go up, n_keep * (48 + stride) come back.
 * held_* without held state, first + n > count, a keep[k] >= count, a null pointer with a non-zero length:
 * ALN_ERR_INVALID_ARGUMENT, nothing written.
 * stats: the last pass's kernel times in ms (fill, selection, hit re-fill + walk) + its download's wall time, and the bytes it
 * moved (host -> device, device -> host).  After a held_* call: ms[2] its kernels, ms[3] the call's wall time, and its bytes. ---- */
typedef struct aln_scan aln_scan;
typedef struct aln_scan_geometry {
    uint64_t first, step, width;
    uint32_t reverse;
    uint32_t reserved;
} aln_scan_geometry;

aln_scan *aln_scan_create(aln_ctx *ctx, const uint8_t *seq, size_t len, int *status);
void aln_scan_destroy(aln_scan *scan);
size_t aln_scan_windows(const aln_scan *scan, const aln_scan_geometry *geometry);
int aln_scan_score(aln_scan *scan, const aln_params *params, const aln_scan_geometry *geometry, double *f);
int aln_scan_select(aln_scan *scan, const aln_params *params, const aln_scan_geometry *geometry, double mean, double sd,
                    double z_min, size_t cap, uint64_t *count, uint32_t *indices, aln_pair_result *results, uint8_t *tb_buf);
int aln_scan_hits(aln_scan *scan, const aln_params *params, const aln_scan_geometry *geometry, double mean, double sd, double z_min,
                  uint64_t *count);
int aln_scan_held_list(aln_scan *scan, uint64_t first, uint64_t n, uint32_t *indices, double *f);
int aln_scan_held_frequencies(aln_scan *scan, const uint32_t *keep, uint64_t n_keep, double *counts /* 4 * cols */);
int aln_scan_held_strings(aln_scan *scan, const uint32_t *keep, uint64_t n_keep, aln_pair_result *results, uint8_t *tb_buf);
uint64_t aln_scan_string_stride(const aln_scan *scan, uint32_t cols, const aln_scan_geometry *geometry);
int aln_scan_stats(const aln_scan *scan, double *ms, uint64_t *bytes);

/* ---- shuffled copies (calculate_p_value, aligner-core/src/statistics/mod.rs:240-320): every pair's target is copied per_pair
 * times, each copy losing `trim` tail residues (uniform in 0..max_trim) and then shuffled, and the query is aligned against every
 * copy, score only.  The copies are drawn on the device (one device: the context's first) from SplitMix64 streams specified bit for
 * bit in aligner_amd/csrc/aln_shuffle_rules.h: copy s of pair i depends on (seed, pair_base + i, s) only, so a job split across
 * calls with matching pair_base gives the same copies.  The queries and the original targets are uploaded once.
 * scores: f[i * per_pair + s] is the f of copy s of pair i; lengths (optional) its length L - trim; status (optional) per pair: the
 * status of the first copy that failed (ALN_ERR_CODE_OUT_OF_RANGE, ALN_ERR_EMPTY_SEQUENCE, ALN_ERR_NO_POSITIVE_CELL ...), ALN_OK
 * if none did; the other pairs are unaffected.  Without a status array a failed pair is the call's return value.  Any non-PWM
 * semantics and every scheme aln_align_batch accepts, on the routes it would pick for the copies; ALN_PWM_LOCAL:
 * ALN_ERR_UNSUPPORTED.  Any t_len[i] < max_trim, per_pair outside 1 .. 2^20: ALN_ERR_INVALID_ARGUMENT for the whole call.
 * targets: the copies themselves, copy s of pair i at out[out_off[i] + s * t_len[i]], its first L - trim bytes (the rest of the
 * t_len[i] bytes are 0). ---- */
typedef struct aln_shuffle_spec {
    uint64_t seed;
    uint64_t pair_base;   /* stream index of pair 0 (reproducible sharding) */
    uint32_t per_pair;    /* shuffled copies per pair: 4999 in calculate_p_value; 1 .. 2^20 */
    uint32_t max_trim;    /* tail residues dropped, uniform in 0..max_trim: 6 in the reference */
} aln_shuffle_spec;       /* 24 bytes */

int aln_shuffle_scores(aln_ctx *ctx, const aln_params *params, const aln_shuffle_spec *spec, const uint8_t *seqs,
                       const uint64_t *q_off, const uint64_t *q_len, const uint64_t *t_off, const uint64_t *t_len,
                       size_t n_pairs, double *f, uint32_t *lengths, int32_t *status);
int aln_shuffle_targets(aln_ctx *ctx, const aln_shuffle_spec *spec, const uint8_t *seqs, const uint64_t *t_off,
                        const uint64_t *t_len, size_t n_pairs, uint8_t *out, const uint64_t *out_off);

/* ---- resident pair set (the loop of HeuristicAligner, aligner-core/src/heuristic/mod.rs:36-78, for many pairs in lock step): the
 * residues of n_pairs pairs are uploaded once (one device: the context's first; layout of aln_align_batch), and every run aligns a
 * list of them, each under a real-valued matrix of its own, on the f64 kernels.
 * run: params->rows / cols give the shape shared by all matrices, at most ALN_PAIRSET_MAX_ENTRIES entries (each wave of the fill
 * kernel keeps its pair's matrix in LDS: 4 x 8 KiB per workgroup, four workgroups per CU); params->matrix must be NULL; del, ext,
 * max_passes, blank_code and force_serial as elsewhere; outputs is ignored (scores and strings are always produced and held).
 * ALN_CORE_LOCAL and ALN_CORE_GLOBAL; the legacy and PWM semantics: ALN_ERR_UNSUPPORTED.  matrices: n_active compact row-major
 * matrices, entry k scores pair active[k]; results[k] is that pair's summary.  Per-pair failures (ALN_ERR_CODE_OUT_OF_RANGE,
 * ALN_ERR_EMPTY_SEQUENCE, ALN_ERR_NO_POSITIVE_CELL) are that pair's status and leave the others untouched; the call returns ALN_OK.
 * A run is cut into chunks by the cell bounds of aln_align_batch (ALN_CHUNK_CELLS overrides); a pair's bytes do not depend on the
 * chunking, the order of `active` or the other pairs' matrices.  Summaries and walked strings of all active pairs stay on the
 * device until the next run or destroy.  ALN_ERR_INVALID_ARGUMENT, nothing written: rows * cols outside 1 .. ALN_PAIRSET_MAX_ENTRIES,
 * a matrix in params, an active[k] >= n_pairs or listed twice, a null pointer with a non-zero length.
 * frequencies: counts[k * rows * cols + t * cols + q] = the columns of listed pair which[k]'s held strings that put target residue t
 * on query residue q, neither being blank (Alignment::get_frequency_matrix, alignment.rs:13-23, the duplicated seed pair included),
 * counted on the device in unsigned integers: exact, the same in any order.  A failed pair's counts are zero.  4 * n bytes go up,
 * 4 * rows * cols * n come back.
 * strings: summaries and strings of the listed pairs in the layout of aln_align_batch (pair which[k]: aligned query at tb_off[k],
 * aligned target q_len + t_len + 2 bytes later; tb_buf optional).  Bytes of a string's capacity beyond aln_len, and both strings of a
 * failed pair, are zero.
 * A which[k] that was not in the last run, a fetch without a run: ALN_ERR_INVALID_ARGUMENT, nothing written.
 * stats: ms[0] fill kernels and ms[1] traceback kernels of the last run, ms[2] kernels of the last fetch, ms[3] wall time of the
 * last call; bytes moved by the last call (host -> device, device -> host).
 *
 * The loop's matrices can stay on the device as well (additions of the same ABI version; run, frequencies and strings are unchanged):
 * heuristics: uploads every pair's transform parameters once (frequencies[i * rows .. + rows), kd[i], r_squared[i] of pair i) and
 * reserves the STORE, one rows x cols f64 matrix per pair, rows * cols in 1 .. ALN_PAIRSET_MAX_ENTRIES.  If the memory cannot be had:
 * ALN_ERR_OOM, parameters and store as before.  A later call replaces the parameters and clears the store.
 * reestimate: for listed pair which[k], store[which[k]] = transform_matrix(source, that pair's parameters), computed by one wave per
 * pair (aligner_amd/csrc/aln_pairset.hip) in the operation order of aligner_amd/csrc/aln_transform_rules.h: the bits of
 * aln_transform_matrices.  The source is shared_matrix (rows * cols doubles) if given, otherwise the frequency counts of the pair's
 * held strings of the last run, counted as `frequencies` counts them.  status[k] = 0, or ALN_TRANSFORM_NO_ROOT, and then the store
 * entry is left as it was.  ALN_ERR_INVALID_ARGUMENT, nothing written: no parameters set; a pair listed twice or out of range;
 * without a shared matrix a pair that was not in the last run, no held run, or a held run of another shape than the store's.
 * 4 bytes per listed pair go up (8 without a shared matrix: the pair and its held entry; rows * cols * 8 once with one), 4 come back.
 * run_stored: `run` with entry k scored by store[active[k]]; the listed entries are gathered on the device, so the call's uploads
 * are those of `run` less its 8 * rows * cols * n_active bytes of matrices, plus 4 bytes per pair for the list.  Checks, chunking,
 * held state and per-pair failures as `run`; in addition ALN_ERR_INVALID_ARGUMENT for no parameters set, params->rows / cols other
 * than the store's, and a listed pair whose store entry was never written.
 * matrices: downloads the listed store entries (8 * rows * cols bytes each) in the order listed; an entry that was never written or
 * out of range: ALN_ERR_INVALID_ARGUMENT, nothing written.
 * stats after these calls: ms[2] = the transform kernel (reestimate) or the gather kernel (run_stored, matrices), bytes[] as above. ---- */
#define ALN_PAIRSET_MAX_ENTRIES 1024u
typedef struct aln_pairset aln_pairset;
aln_pairset *aln_pairset_create(aln_ctx *ctx, const uint8_t *seqs, const uint64_t *q_off, const uint64_t *q_len, const uint64_t *t_off,
                                const uint64_t *t_len, size_t n_pairs, int *status);
int aln_pairset_run(aln_pairset *ps, const aln_params *params, const double *matrices, const uint32_t *active, size_t n_active,
                    aln_pair_result *results);
int aln_pairset_frequencies(aln_pairset *ps, const uint32_t *which, size_t n, uint32_t *counts);
int aln_pairset_strings(aln_pairset *ps, const uint32_t *which, size_t n, aln_pair_result *results, uint8_t *tb_buf,
                        const uint64_t *tb_off);
int aln_pairset_stats(const aln_pairset *ps, double *ms /* 4 */, uint64_t *bytes /* 2 */);
void aln_pairset_destroy(aln_pairset *ps);
int aln_pairset_heuristics(aln_pairset *ps, uint32_t rows, uint32_t cols, const double *frequencies /* n_pairs * rows */,
                           const double *kd /* n_pairs */, const double *r_squared /* n_pairs */);
int aln_pairset_reestimate(aln_pairset *ps, const double *shared_matrix /* rows * cols, or NULL */, const uint32_t *which, size_t n,
                           int32_t *status);
int aln_pairset_run_stored(aln_pairset *ps, const aln_params *params, const uint32_t *active, size_t n_active, aln_pair_result *results);
int aln_pairset_matrices(aln_pairset *ps, const uint32_t *which, size_t n, double *out);

/* ---- resident sequence set (the request path, aligner-web dispatcher/handlers.rs:104,253-264 generate_pairs: every pair i < j of
 * a FASTA; blast_p_value_cmp.rs and calc: rows of (query, target) drawn from one table): S sequences are uploaded once (one device:
 * the context's first) and a call names a BLOCK of the S x S pair grid.  The descriptors are expanded on the device, every pair is
 * scored by the kernels aln_align_batch would take for it, and either the scores or the held hits come back.
 * block: upper = 0: every (q, t) of the rectangle, pair k = (q_first + k / t_count, t_first + k % t_count); upper = 1 (q_first ==
 * t_first and q_count == t_count required): the pairs i < j of that square in generate_pairs order, row-major (0,1) (0,2) .. (0,n-1)
 * (1,2) .., n (n - 1) / 2 pairs (aligner_amd/csrc/aln_seqset_rules.h has the numbering).  Sequence q is the query (columns),
 * sequence t the target (rows).
 * Pair k is exactly what aln_align_batch computes for (query = sequence q, target = sequence t), for every scheme and every non-PWM
 * semantics it accepts (ALN_PWM_LOCAL: ALN_ERR_UNSUPPORTED); a pair's bytes do not depend on the block it was named through, on the
 * chunking (the cell bounds of aln_align_batch and 2^22 pairs per chunk; ALN_CHUNK_CELLS overrides) or on the other pairs.
 * score: f[k] = the batch's results[k].f.  Per-pair failures (ALN_ERR_EMPTY_SEQUENCE, ALN_ERR_CODE_OUT_OF_RANGE,
 * ALN_ERR_NO_POSITIVE_CELL) go into status[k] and the call returns ALN_OK; without a status array the first failed pair's status is
 * the return value (as aln_shuffle_scores).  8 bytes per pair come back, 4 more with status.  params->outputs is ignored.
 * hits: a HELD pass (as aln_scan_hits).  The same fill; on the device the pairs with status ALN_OK and f >= f_min (plain IEEE
 * compare: a NaN f_min selects nothing) are compacted per chunk in ascending pair order by an ordered prefix sum (no atomic appends).
 * A chunk's hits (pair number and f, 16 bytes each) are read where the pass waits for that chunk anyway and appended to one ascending
 * list, which is kept on the HOST: the re-fill of the hits is planned from it like a batch of its own (routes and direction layout
 * depend on every hit's shape), so its descriptors and queue are uploaded (60 bytes per hit).  The held buffers are sized for exactly
 * the count (ALN_ERR_OOM and nothing held if that memory cannot be had), and ALL hits are filled again with directions and walked.
 * Their summaries and strings stay on the device; the call itself returns *count.  Failed pairs are never hits and do not fail the
 * call.  Held state lasts until the set's next score / hits or destroy.
 * held_list: pair index (in the block of the hits call), query and target sequence numbers and f of held hits first .. first + n - 1,
 * ascending pair order; served from the host's list (no device traffic, the stats of the pass stay).
 * held_strings: summaries and strings of the listed positions of the held list (any order; a position may be listed twice) in the
 * layout of aln_align_batch: entry k's aligned query at tb_off[k], aligned target q_len + t_len + 2 bytes later; tb_buf optional.
 * Bytes of a string's capacity beyond aln_len, and both strings of a failed entry, are zero.
 * held_* without held state, first + n > count, a keep[k] >= count, a null pointer with a non-zero length:
 * ALN_ERR_INVALID_ARGUMENT, nothing written.
 * ALN_ERR_INVALID_ARGUMENT for the whole call, nothing written: an invalid block (a range past n_seqs, upper with unequal ranges,
 * reserved != 0, no pairs), a null matrix, a null output; create with n_seqs >= 2^32.
 * stats: ms[0] fill kernels of the last score / hits pass, ms[1] its hit re-fill and walk, ms[2] kernels of the last held fetch,
 * ms[3] wall time of the last call; bytes moved by the last call (host -> device, device -> host). ---- */
typedef struct aln_seqset aln_seqset;
typedef struct aln_seqset_block {
    uint64_t q_first, q_count;   /* sequences used as query (columns) */
    uint64_t t_first, t_count;   /* sequences used as target (rows)   */
    uint32_t upper;              /* 0: the rectangle; 1: the pairs i < j of the square (ranges must be equal) */
    uint32_t reserved;           /* 0 */
} aln_seqset_block;              /* 40 bytes */

aln_seqset *aln_seqset_create(aln_ctx *ctx, const uint8_t *seqs, const uint64_t *off, const uint64_t *len, size_t n_seqs, int *status);
void aln_seqset_destroy(aln_seqset *set);
uint64_t aln_seqset_pairs(const aln_seqset *set, const aln_seqset_block *block);          /* 0 for an invalid block */
int aln_seqset_score(aln_seqset *set, const aln_params *params, const aln_seqset_block *block, double *f, int32_t *status /* optional, per pair */);
int aln_seqset_hits(aln_seqset *set, const aln_params *params, const aln_seqset_block *block, double f_min, uint64_t *count);
int aln_seqset_held_list(aln_seqset *set, uint64_t first, uint64_t n, uint64_t *pair_index, uint32_t *q_seq, uint32_t *t_seq, double *f);
int aln_seqset_held_strings(aln_seqset *set, const uint32_t *keep, uint64_t n_keep, aln_pair_result *results, uint8_t *tb_buf,
                            const uint64_t *tb_off);
int aln_seqset_stats(const aln_seqset *set, double *ms /* 4 */, uint64_t *bytes /* 2 */);

/* ---- the k best targets per query (an addition of the same ABI version): the question of a database search.  A HELD pass like
 * aln_seqset_hits -- the same chunking, fill, gather, per-pair failures and re-fill -- whose selection is per query row instead of
 * one global threshold: of every query q of a rectangle (upper = 1: ALN_ERR_UNSUPPORTED, a pair would belong to both of its
 * sequences), the min(k, candidates) candidates that come first.
 * candidate: a pair of the row with status ALN_OK, f == f and f >= f_min (plain IEEE compares: a NaN f_min selects nothing; -inf
 * admits every pair that succeeded); with ALN_BEST_SKIP_SELF also q != t as sequence numbers.  A failed pair is never a candidate and
 * does not fail the call.
 * order: (f, t) before (f', t') iff f > f', or f == f' and t < t' (-0.0 == +0.0): total within a row, so the kept set does not depend
 * on the launch geometry, the chunking or anything else (aligner_amd/csrc/aln_best_rules.h is the rule as code).
 * The selection runs on the device (aln_best.hip): per-row running lists of min(k, t_count) slots of 12 bytes, allocated for the
 * call (ALN_ERR_OOM and nothing held if they cannot be had), and after the last chunk one ascending (pair number, f) list, 16 bytes
 * per kept pair, comes down -- nothing per pair of the block does.  *count = the sum over the query rows of min(k, candidates).  The list is held as
 * the hits of aln_seqset_hits are: held_list and held_strings serve it with their contracts unchanged, in ascending pair order
 * (query by query, targets ascending); the rank within a query follows from f and t by the order.  A kept f of -0.0 is listed as
 * +0.0 (equal under the order); held_strings' summary carries the fill's own bits.  Held state lasts until the set's next score /
 * hits / best or destroy.
 * ALN_ERR_INVALID_ARGUMENT, nothing held and *count untouched: k outside 1 .. ALN_SEQSET_BEST_MAX, a flag bit other than
 * ALN_BEST_SKIP_SELF, a null count, an invalid block.  ALN_PWM_LOCAL: ALN_ERR_UNSUPPORTED.  A refused call leaves earlier held state
 * as it was.
 * stats after a best pass: ms[0] fill, ms[1] re-fill and walk, ms[2] the selection kernels (a later held fetch overwrites it). ---- */
#define ALN_SEQSET_BEST_MAX 64u
#define ALN_BEST_SKIP_SELF 1u
int aln_seqset_best(aln_seqset *set, const aln_params *params, const aln_seqset_block *block, uint32_t k, double f_min, uint32_t flags,
                    uint64_t *count);

/* ---- significance of held hits (an addition of the same ABI version): is a held hit better than chance?  For every listed position
 * of the held list (of aln_seqset_hits or aln_seqset_best; any order, a position may be listed twice) the query, sequence q, is aligned
 * score only against spec->per_pair trimmed and shuffled copies of the target, sequence t -- the copies of aln_shuffle_scores, drawn
 * on the device from the set's own resident residues (none are uploaded), filled by the launches aln_shuffle_scores makes, planned
 * and chunked as it plans and chunks (whole hits per chunk; ALN_CHUNK_CELLS overrides the cell bound) -- and what the copies of a hit
 * leave is reduced on the device to one 48-byte record, in the order aligner_amd/csrc/aln_signif_rules.h states: 64 partial
 * accumulators, accumulator l taking copies l, l + 64, ... in ascending order, folded at distances 32, 16, .. 1; every operation
 * rounded on its own.  The bits of a record therefore depend on (seed, stream, scheme, the two sequences, the held f) only.
 * stream: copy s of a hit comes from the stream (seed, pair_base + pair_index, s) of aln_shuffle_rules.h, pair_index being the hit's
 * pair number in the block of the held pass (what held_list reports; uint64 arithmetic, wrapping) -- not its position in the held
 * list or in keep: a pair's copies do not depend on f_min, k, the other hits or the order of keep, and are the copies
 * aln_shuffle_scores draws for that pair under pair_base + pair_index.
 * params: the scheme of the copies (any non-PWM semantics and every scheme aln_shuffle_scores accepts; passing the scheme of the held
 * pass is the caller's business); outputs is ignored.  n_ge compares against the held list's f.
 * A failed copy (trimmed to nothing: ALN_ERR_EMPTY_SEQUENCE; no positive cell: ALN_ERR_NO_POSITIVE_CELL ...) is left out of the sums
 * and shows as n_ok < per_pair, with the first such copy and its status in the record; it fails neither the hit nor the call.
 * f, lengths (optional, n_keep * per_pair each): entry k * per_pair + s is the f (a failed copy: as its summary has it) and the
 * length L - trim of copy s of keep[k].  Device memory does not grow with n_keep * per_pair: the copies' scores live in a buffer of
 * the largest chunk, and with f they come down chunk by chunk.  Up: 48 bytes per listed hit (its place in the residue buffers, its
 * stream, its held f), the matrix, and the plan's queue for chunks with copies routed off the batch kernel.  Down: 48 bytes per hit,
 * 8 more per copy with f.
 * The held summaries and strings are not touched: held_list and held_strings answer afterwards as before.
 * ALN_ERR_INVALID_ARGUMENT for the whole call, nothing written, held state intact: no held state, a keep[k] >= count, a null pointer
 * with a non-zero length, per_pair outside 1 .. 2^20, a listed hit whose target is shorter than max_trim.  ALN_PWM_LOCAL:
 * ALN_ERR_UNSUPPORTED.
 * stats afterwards: ms[2] the kernels of this call (shuffle, fill, reduce, with the copies between them), ms[3] its wall time; bytes[]
 * as above; ms[0] and ms[1] stay the held pass's. ---- */
typedef struct aln_signif_record {
    double   sum;        /* of f over the copies with status ALN_OK          */
    double   sum_sq;     /* of f * f over them (product rounded, then added) */
    double   f_max;      /* largest such f; -inf when n_ok == 0              */
    uint32_t n_ok;       /* copies with status ALN_OK                        */
    uint32_t n_ge;       /* of those, f_copy >= f_hit (plain IEEE compare)   */
    int32_t  status;     /* status of the first failed copy, ALN_OK if none  */
    uint32_t first_bad;  /* its copy number, 0xffffffff if none              */
    uint64_t reserved;   /* 0: fills the record to 48 bytes                  */
} aln_signif_record;     /* 48 bytes */

int aln_seqset_held_significance(aln_seqset *set, const aln_params *params, const aln_shuffle_spec *spec, const uint32_t *keep,
                                 uint64_t n_keep, aln_signif_record *records, double *f, uint32_t *lengths);

/* ---- reports of held hits (additions of the same ABI version): how identical, how covering and how gapped is a held hit?  The
 * columns of a held entry's two aligned strings (x = query[j], y = target[j], j = 0 .. aln_len - 1, as held_strings returns them) are
 * classed and counted on the device (aln_report.hip), in the classes of the reference's midline (Alignment::get_alignment,
 * aligner-core/src/alignment.rs:25-42); aligner_amd/csrc/aln_report_rules.h is the rule as code.
 * columns: all aln_len of them, or with ALN_REPORT_SKIP_SEED aln_len - 1 (0 when aln_len is 0): the LAST column is the end cell's
 * residue pair, with which the reference's traceback seeds both strings before the walk (simple/mod.rs:102-105, 213-216) and which
 * the walk emits again itself.  Without the flag the counts are those of the reference's own midline and frequency matrix, with it
 * the alignment's.
 * class of a column, exactly one: identical (x == y, x != blank); positive (both non-blank, x != y, S[y][x] >= 0.0 -- a plain IEEE
 * compare: 0.0 and -0.0 are positive, a NaN is not; a code beyond the matrix is not); mismatch (both non-blank, x != y, not
 * positive); q_gap (x == blank, y != blank); t_gap (y == blank, x != blank); both blank: counted in `columns` only.
 * q_gap_open: a q_gap column j with j == 0 or column j - 1 not q_gap; t_gap_open alike.
 * A held entry whose summary status is not ALN_OK: all counts 0 and that status.
 * params: matrix / rows / cols / row_stride / blank_code only (the scheme of the classes; passing the held pass's is the caller's
 * business).  The one bit the rule reads of an entry goes up as a table of rows * cols bits; rows * cols > 8192: ALN_ERR_UNSUPPORTED.
 * held_report: the listed positions of the held list (of hits or best; any order, a position may be listed twice).  Up: 4 bytes per
 * listed hit and the bit table.  Down: 40 bytes per listed hit.
 * held_filter: ALL held hits are reported into a buffer of the set (40 bytes each, on the device) and the entries that pass the
 * filter are compacted in ascending held order (the ordered prefix sum of the selections: no atomic appends).  An entry is kept iff
 * status == ALN_OK, columns >= min_columns, (double)identical >= min_identity * (double)columns, (double)(columns - q_gap) >=
 * min_q_cover * (double)N and (double)(columns - t_gap) >= min_t_cover * (double)M, N and M the lengths of its query and target
 * sequences; one multiplication and one compare each, rounded on its own: a NaN threshold keeps nothing.  positions (and reports,
 * optional) receive the first `capacity` kept entries; *count is the number kept in all, also beyond capacity.  Only the kept come
 * down: 4 bytes per written position, 40 more with its record.
 * The held summaries and strings are not touched: held_list, held_strings and held_significance answer afterwards as before.
 * ALN_ERR_INVALID_ARGUMENT, nothing written, held state intact: no held state, a keep[k] >= count, a null pointer with a non-zero
 * length, a null params / matrix / filter / count, rows * cols == 0, a flag bit other than ALN_REPORT_SKIP_SEED, filter->reserved
 * != 0.  ALN_PWM_LOCAL: ALN_ERR_UNSUPPORTED.
 * stats afterwards: ms[2] the kernels of this call, ms[3] its wall time, bytes[] as above; ms[0] and ms[1] stay the held pass's. ---- */
#define ALN_REPORT_SKIP_SEED 1u
typedef struct aln_hit_report {
    uint32_t columns;      /* columns counted                                   */
    uint32_t identical;
    uint32_t positive;
    uint32_t mismatch;
    uint32_t q_gap;        /* blank in the aligned query                        */
    uint32_t t_gap;        /* blank in the aligned target                       */
    uint32_t q_gap_open;   /* runs of q_gap columns                             */
    uint32_t t_gap_open;
    int32_t  status;       /* the held entry's; not ALN_OK: every count is 0    */
    uint32_t reserved;     /* 0                                                 */
} aln_hit_report;          /* 40 bytes */
typedef struct aln_hit_filter {
    double   min_identity; /* identical / columns                               */
    double   min_q_cover;  /* (columns - q_gap) / N                             */
    double   min_t_cover;  /* (columns - t_gap) / M                             */
    uint32_t min_columns;
    uint32_t reserved;     /* 0 */
} aln_hit_filter;          /* 32 bytes */

int aln_seqset_held_report(aln_seqset *set, const aln_params *params, uint32_t flags, const uint32_t *keep, uint64_t n_keep,
                           aln_hit_report *reports);
int aln_seqset_held_filter(aln_seqset *set, const aln_params *params, uint32_t flags, const aln_hit_filter *filter, uint32_t *positions,
                           aln_hit_report *reports /* optional */, uint64_t capacity, uint64_t *count);

/* ---- heuristic alignment of the pairs of a sequence set (additions of the same ABI version): the request path's two halves joined --
 * every pair of a FASTA (generate_pairs), each run through the loop of HeuristicAligner (heuristic/mod.rs:36-78).
 * create_from_set: a pair set whose pair i is pair first + i of the block, in the block's numbering (sequence q the query, sequence
 * t the target).  It BORROWS the set's residue buffer: nothing is uploaded or copied, the host tables come from one walk over the
 * block.  Every aln_pairset_* call works on it with its contract unchanged.  The set counts its derived pair sets: aln_seqset_destroy
 * with some alive releases everything but the residues, which go with the last derived pair set; any other call on the destroyed
 * handle (create_from_set included) is the caller's error.  Passes on the set and runs on a derived pair set may interleave (different
 * slots and streams, read-only residues).  ALN_ERR_INVALID_ARGUMENT, nothing created: a null set or block, an invalid block,
 * first + n_pairs beyond the block's pairs.  ALN_ERR_UNSUPPORTED: n_pairs > 0xFFFFFFF0.
 * The loop's decision lives in the library (on any pair set, after aln_pairset_heuristics).  Its state is resident: best f per pair
 * (f64) and the GOING LIST, both on the device.
 * loop_begin: best[i] = 0.0, store[i] = transform(shared_matrix, pair i's parameters) as `reestimate` computes it; status[i] = 0 or
 * ALN_TRANSFORM_NO_ROOT (heuristic/mod.rs:52-57); the going list becomes the pairs with status 0, ascending.  8 * rows * cols bytes
 * go up, 4 per pair come back.  Without heuristics, a null matrix or status: ALN_ERR_INVALID_ARGUMENT.
 * loop_step: one iteration for all going pairs.  The going list is aligned under the store exactly as `run_stored` aligns it (same
 * checks, chunking, per-pair failures and held state; the descriptors are planned on the host and uploaded), but the list is read
 * where it lies and no summary comes back for it.  Then, on the device, each held entry (pair i) is classified by
 * aligner_amd/csrc/aln_loop_rules.h: status != ALN_OK: finished, cause 1 (the status is in its summary); else f > best[i] (plain
 * IEEE compare: a NaN does not go on): best[i] = f and store[i] is re-estimated from the pair's held strings as `reestimate` does
 * it -- ALN_TRANSFORM_NO_ROOT: finished, cause 2, store[i] left as it was; otherwise the pair goes on; else: finished, cause 0
 * (heuristic/mod.rs:64-75), store[i] being the matrix of its last run.  Both lists are compacted in ascending going order by an
 * ordered prefix sum (no atomic appends; tiles of 2048 entries, 256 tiles a trip), and the next step reads its list there.
 * Back come finished[k] (pair numbers, ascending going order), cause[k], finished_results[k] (48 bytes each, gathered on the device)
 * for k < counts[1] + counts[2], and counts = {pairs run, finished with cause 0, finished with cause 1 or 2, going on}; the
 * arrays must hold as many entries as pairs are going (counts[3] of the step before; the status-0 pairs after loop_begin).  Nothing
 * comes back for a pair that goes on: 12 bytes per step beside.  The held run lasts until the next step or run: aln_pairset_strings
 * and aln_pairset_matrices on the finished pairs fetch what HeuristicAligner returns.  With nothing going: counts all 0, ALN_OK.
 * ALN_ERR_INVALID_ARGUMENT, state untouched: no loop_begin since the last aln_pairset_heuristics, params of another shape than the
 * store's, a matrix in params, a null output while pairs are going.  ALN_ERR_UNSUPPORTED: semantics other than the two core ones.
 * aln_pairset_run / run_stored / reestimate between two steps are the caller's business: they replace the held run and may rewrite
 * store entries, but touch neither best nor the going list.
 * stats after a step: ms[0], ms[1] as after a run, ms[2] the gather, transform and compaction kernels; bytes as moved. ---- */
aln_pairset *aln_pairset_create_from_set(aln_seqset *set, const aln_seqset_block *block, uint64_t first, uint64_t n_pairs, int *status);
int aln_pairset_loop_begin(aln_pairset *ps, const double *shared_matrix, int32_t *status /* n_pairs */);
int aln_pairset_loop_step(aln_pairset *ps, const aln_params *params, uint32_t *finished, uint32_t *cause,
                          aln_pair_result *finished_results, uint32_t *counts /* 4: run, done, failed, more */);

/* ---- transform_matrix (aligner-helpers/src/matrices/mod.rs:19-68) for n matrices at once, on the HOST (no GPU is touched): matrix i
 * (rows x cols, compact row-major) is rescaled under frequencies[i * rows .. + rows), kd[i], r_squared[i] into matrices_out (which may
 * be matrices_in); status[i] = 0, or ALN_TRANSFORM_NO_ROOT where the reference returns Err(WrongMatrixSpecified) (matrix i of the
 * output is then left as it was).  Plain f64 arithmetic in the order aligner_amd/csrc/aln_transform_rules.h specifies, which is the
 * order of the numpy mirror (aligner_amd/heuristic.py): the same bits.  rows * cols above 8192, a null pointer with n != 0:
 * ALN_ERR_INVALID_ARGUMENT. ---- */
#define ALN_TRANSFORM_NO_ROOT 1
int aln_transform_matrices(size_t n, uint32_t rows, uint32_t cols, const double *matrices_in, const double *frequencies,
                           const double *kd, const double *r_squared, double *matrices_out, int32_t *status);
/* The same contract, status codes and bits, computed on the context's first device by the kernel of aln_pairset_reestimate (host
 * buffers in and out; in place allowed).  rows * cols in 1 .. ALN_PAIRSET_MAX_ENTRIES; beyond that, a null context, a null pointer
 * with n != 0: ALN_ERR_INVALID_ARGUMENT. */
int aln_transform_matrices_device(aln_ctx *ctx, size_t n, uint32_t rows, uint32_t cols, const double *matrices_in,
                                  const double *frequencies, const double *kd, const double *r_squared, double *matrices_out,
                                  int32_t *status);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNER_HIP_H */
