// aln_launch.h -- the launchers and code-object warm-ups that the kernel files (aln_kernels.hip, aln_traceback.hip, aln_scan.hip,
// aln_shuffle.hip, aln_signif.hip, aln_pairset.hip, aln_seqset.hip, aln_loop.hip, aln_best.hip, aln_cluster.hip, aln_prefilter.hip,
// aln_search.hip, aln_profile.hip, aln_msa.hip, aln_cigar.hip, aln_wordjoin.hip, aln_seedjoin.hip, aln_seedchain.hip and aln_strand.hip) define and
// aln_host.hip calls.  Every one of those files includes this header, so the compiler holds each definition against the
// declaration the host compiles against: they are extern "C", and a signature that drifted would still link.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <utility>

#include "aln_device.h"
#include "aln_cluster_rules.h"
#include "aln_profile_rules.h"
#include "aln_msa_rules.h"
#include "aln_cigar_rules.h"
#include "../../include/aligner_hip_seedchain.h"

// what every kernel of aln_cluster.hip takes: n label slots (node numbers 0 .. n - 1, those of `nodes` being nodes), m listed edges
struct ClusterArgs {
    aln_cluster_nodes nodes;
    uint64_t n, m;
    uint32_t mode;
    const uint32_t *len;             // n lengths, or null: all equal
    const uint32_t *ea, *eb;         // m endpoints each; ALN_CLUSTER_NONE in both: a dropped edge
    uint32_t *label;                 // n
    uint32_t *aux0, *aux1, *aux2;    // n each.  components: the roots (aux0).  greedy: state, mark, block
    uint64_t *key;                   // n: greedy, a member's best representative; finish, a cluster's first in priority order
    uint32_t *size, *cedges;         // n each, by label
    uint32_t *misc;                  // 8 words: [0] changed | undecided, [1] clusters, then 64-bit edges, self edges, singletons
};

// what aln_profile_kernel takes: the held store (read only), the hits' endpoints, the labelling, the centres' slots and the outputs
struct ProfileArgs {
    const HeldEntry *held; const aln_pair_result *res; const uint8_t *tb;      // n_held entries of the held store
    const aln_hit_report *rep;       // n_held reports, or null: no filter
    aln_hit_filter filter;
    const uint32_t *hit_q, *hit_t;   // n_held endpoints each
    const uint32_t *label, *len;     // n_seqs each
    const uint32_t *slot_of;         // n_seqs: the profile of a centre, ALN_CLUSTER_NONE without one
    const uint64_t *off;             // n_centers: profile i's first element of out
    uint32_t n_held, n_seqs, n_centers, n_codes, blank, flags;
    uint32_t *out;                   // the profiles, zeroed
    aln_profile_record *rec;         // n_centers
    unsigned long long *misc;        // ALN_PROFILE_MISC_WORDS counters, zeroed
};

// what the kernels of aln_msa.hip take: the held store (read only), the plan's tables and, for the fill, the offsets and the outputs
struct MsaArgs {
    const HeldEntry *held; const aln_pair_result *res; const uint8_t *tb;      // n_held entries of the held store
    const aln_hit_report *rep;       // n_held reports, or null: no filter (the plan only)
    aln_hit_filter filter;
    const uint32_t *hit_q, *hit_t;   // n_held endpoints each
    const uint32_t *label, *len;     // n_seqs each
    const uint32_t *slot_of;         // n_seqs: the family of a centre, ALN_CLUSTER_NONE without one
    const uint64_t *ins_off;         // n_centers: centre i's first entry of ins and col (len + 1 entries each)
    uint64_t n_ins;                  // the entries of ins, and of col
    uint32_t n_held, n_seqs, n_centers, blank;
    uint32_t *ins, *col;             // the insert widths (zeroed before the plan) and the columns of the residues
    uint32_t *mark;                  // n_held: the slot of a contributing hit, else ALN_CLUSTER_NONE
    aln_msa_record *rec;             // n_centers
    unsigned long long *misc;        // ALN_MSA_MISC_WORDS counters, zeroed before the plan
    // the fill
    const uint8_t *seqs; const uint64_t *seq_off;   // the set's residues and where every sequence starts
    const uint64_t *byte_off, *row_off;             // n_centers each: family i's first byte of out and first entry of list / row_hit
    uint32_t *taken;                 // n_centers tickets, zeroed before the fill
    uint32_t *list;                  // total_rows: a family's contributing hits in ticket order (entry 0 of a family unused)
    uint32_t *hit_row;               // n_held: the row of a contributing hit
    uint32_t *row_hit;               // total_rows: the held position of every row
    uint8_t *out;                    // bytes, filled with the blank code before the fill
    uint64_t bytes, total_rows;
};

// what the kernels of aln_cigar.hip take: the held store (read only), the plan's tables and, for the fill, the words
struct CigarArgs {
    const HeldEntry *held; const aln_pair_result *res; const uint8_t *tb;      // n_held entries of the held store
    const uint32_t *list;            // n_list listed positions
    uint32_t n_list, n_held, blank, flags;
    uint64_t tiles;                  // tiles of 256 listed hits
    aln_cigar_record *rec;           // n_list
    uint64_t *off;                   // n_list + 1: where every listed hit's words start, and the total
    uint64_t *tile_sum, *tile_off;   // tiles each
    unsigned long long *misc;        // ALN_CIGAR_MISC_WORDS counters, zeroed before the plan
    // the fill
    uint32_t *ops;                   // total words
    uint64_t total;
    const uint8_t *rev;              // n_list, or null: not 0 where a listed hit's words go in reverse order (aln_strand_rules.h)
};

static inline uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// Beyond 64 KiB of dynamic LDS a kernel has to be told (hipFuncAttributeMaxDynamicSharedMemorySize).  The attribute belongs to the
// kernel on a device, not to a stream or a thread, and callers on several threads launch one kernel with different sizes: so it only
// ever goes up -- the highest size asked for so far, per (device, kernel), raised under a lock before the launch that needs it.  A
// launch can then never find the attribute below its own size, whatever another thread set in between.  (One definition for the
// whole library: an inline function's statics are shared by every translation unit.)
inline hipError_t aln_lds_opt_in(const void *kern, uint32_t lds_bytes)
{
    if (lds_bytes <= 64u * 1024u) return hipSuccess;
    static std::mutex lock;
    static std::map<std::pair<int, const void *>, uint32_t> highest;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> hold(lock);
    uint32_t &high = highest[std::make_pair(dev, kern)];
    if (lds_bytes <= high) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) high = lds_bytes;
    return e;
}
// the launch of a kernel that may need the opt-in (the launch's own error stays with the stream's next check, as for every launch)
template <typename... P, typename... A>
static inline void aln_launch_lds(void (*kern)(P...), dim3 g, dim3 b, uint32_t lds_bytes, hipStream_t s, A &&...args)
{
    (void)aln_lds_opt_in(reinterpret_cast<const void *>(kern), lds_bytes);
    hipLaunchKernelGGL(kern, g, b, lds_bytes, s, std::forward<A>(args)...);
}

extern "C" {

// ---- aln_kernels.hip: the fills.  One code object per kernel unit (aligner_amd/build.py, KERNEL_UNITS), each with its warm-up
int aln_warm_generic(void);
int aln_warm_fast_cl(void);
int aln_warm_fast_rest(void);
int aln_warm_single(void);
int aln_warm_fast_cl_solo(void);
int aln_warm_fast_rest_solo(void);
// the batch fill: picks the kernel (generic unit) and, for the fast integer path, hands on to the unit that holds it
void aln_launch_fill(const FillArgs *a, int is_int, int fast, uint32_t grid, uint32_t lds_bytes, hipStream_t s);
void aln_launch_fill_fast_cl(const FillArgs *a, uint32_t grid, uint32_t lds_bytes, hipStream_t s);
void aln_launch_fill_fast_rest(const FillArgs *a, uint32_t grid, uint32_t lds_bytes, hipStream_t s);
void aln_launch_fill_fast_cl_solo(const FillArgs *a, uint32_t grid, uint32_t lds_bytes, hipStream_t s);
void aln_launch_fill_fast_rest_solo(const FillArgs *a, uint32_t grid, uint32_t lds_bytes, hipStream_t s);
void aln_launch_fill_duo(const FillArgs *a, uint32_t grid, uint32_t lds_bytes, hipStream_t s);
void aln_launch_wgpipe(const WgArgs *a, int is_int, uint32_t lds_bytes, hipStream_t s);
void aln_launch_validate(const uint8_t *seqs, PairDesc *descs, uint32_t n_pairs, uint32_t rows, uint32_t cols, int pwm, hipStream_t s);
// the single-pair route; aln_single_waves: strips per workgroup of its fill
uint32_t aln_single_waves(int semantics, uint32_t R, uint32_t rows, uint32_t cols, uint32_t N, uint32_t ns);
void aln_launch_single_init(const SingleArgs *a, uint32_t n_bytes, hipStream_t s);
void aln_launch_single(const SingleArgs *a, uint32_t N, int with_serial, hipStream_t s);
void aln_launch_single_repair(const SingleArgs *a, uint32_t N, hipStream_t s);

// ---- aln_traceback.hip: the walks over the direction store, the aligned strings, the direction unpack, the dyadic rescaling
int aln_warm_tb(void);
void aln_launch_traceback(const TraceArgs *a, hipStream_t s);
void aln_launch_traceback_wave(const TraceArgs *a, hipStream_t s);
void aln_launch_traceback_overlap(const TraceArgs *a, uint32_t waves, hipStream_t s);
void aln_launch_traceback_expand(const TraceArgs *a, hipStream_t s);
void aln_launch_traceback_single(const TraceSingleArgs *a, uint32_t N, hipStream_t s);
void aln_launch_traceback_expand_single(const TraceArgs *a, uint32_t pair, hipStream_t s);
void aln_launch_unpack(const uint8_t *dirs, const PairDesc *descs, uint32_t pair, int semantics, uint8_t *out, uint64_t cells, hipStream_t s);
void aln_launch_scale_results(aln_pair_result *results, uint32_t n, double factor, hipStream_t s);

// ---- aln_scan.hip: the window scan
void aln_scan_launch_expand(PairDesc *descs, uint32_t *order, uint64_t n, uint64_t first, uint64_t step, uint64_t width, uint64_t len,
                            uint64_t base, uint32_t cols, hipStream_t s);
void aln_scan_launch_f(const aln_pair_result *res, double *f, uint64_t n, int32_t *bad, hipStream_t s);
uint64_t aln_scan_tiles(uint64_t n);
void aln_scan_launch_select(const aln_pair_result *res, uint64_t n, double mean, double sd, double z_min, uint32_t *tile_count,
                            uint32_t *tile_off, uint32_t *count, uint32_t *idx, uint32_t cap, hipStream_t s);
void aln_scan_launch_hits(PairDesc *descs, uint32_t *order, uint32_t n_slots, const uint32_t *idx, const uint32_t *count, uint32_t cap,
                          uint64_t first, uint64_t step, uint64_t width, uint64_t len, uint64_t base, uint32_t cols, uint64_t dir_stride,
                          uint64_t tb_stride, uint64_t tag_stride, hipStream_t s);
void aln_scan_launch_held_f(const aln_pair_result *res, double *f, uint32_t n, hipStream_t s);
void aln_scan_launch_freq(const PairDesc *descs, const aln_pair_result *res, const uint8_t *tb, const uint32_t *keep, uint32_t n_keep,
                          uint32_t n_held, uint32_t cols, uint32_t blank, uint32_t *counts, double *out, hipStream_t s);
void aln_scan_launch_gather(const aln_pair_result *res, const uint8_t *tb, const uint32_t *keep, uint32_t n_keep, uint32_t n_held,
                            uint64_t stride, aln_pair_result *out_res, uint8_t *out_tb, hipStream_t s);
void aln_scan_launch_reverse(uint8_t *seq, uint64_t len, hipStream_t s);

// ---- aln_shuffle.hip: shuffled copies
void aln_shuffle_launch(const uint8_t *seqs, uint8_t *out, const ShufflePair *pairs, uint32_t p0, uint64_t n, uint32_t per_pair, uint64_t seed,
                        uint64_t pair_base, uint32_t max_trim, uint64_t out_base, uint32_t slot, hipStream_t s);
void aln_shuffle_launch_expand(PairDesc *descs, uint32_t *order, const ShufflePair *pairs, uint32_t p0, uint64_t n, uint32_t per_pair,
                               uint64_t seed, uint64_t pair_base, uint32_t max_trim, uint64_t region, uint64_t out_base, hipStream_t s);
void aln_shuffle_launch_gather(const aln_pair_result *res, double *f, uint64_t n, uint32_t per_pair, uint32_t *first, hipStream_t s);
// the same with a stream table: pair i's copies come from the streams (seed, stream[i], s)
void aln_shuffle_launch_table(const uint8_t *seqs, uint8_t *out, const ShufflePair *pairs, uint32_t p0, uint64_t n, uint32_t per_pair, uint64_t seed,
                              const uint64_t *stream, uint32_t max_trim, uint64_t out_base, uint32_t slot, hipStream_t s);
void aln_shuffle_launch_expand_table(PairDesc *descs, uint32_t *order, const ShufflePair *pairs, uint32_t p0, uint64_t n, uint32_t per_pair,
                                     uint64_t seed, const uint64_t *stream, uint32_t max_trim, uint64_t region, uint64_t out_base, hipStream_t s);

// ---- aln_signif.hip: the records of a chunk's hits out of their copies' summaries
void aln_signif_launch_reduce(const aln_pair_result *res, const double *f_hit, uint32_t n_hits, uint32_t per_pair, aln_signif_record *rec,
                              double *f, hipStream_t s);

// ---- aln_pairset.hip: the strings of a held store (a pair set's or a sequence set's), per-pair matrices
void aln_pairset_launch_freq(const HeldEntry *held, const aln_pair_result *res, const uint8_t *tb, const uint32_t *list, uint32_t n_list,
                             uint32_t n_held, uint32_t rows, uint32_t cols, uint32_t blank, uint32_t *counts, hipStream_t s);
void aln_held_launch_gather(const HeldEntry *held, const aln_pair_result *res, const uint8_t *tb, const uint32_t *list,
                            const uint64_t *out_off, uint32_t n_list, uint32_t n_held, aln_pair_result *out_res, uint8_t *out_tb, hipStream_t s);
int aln_pairset_launch_transform(const PairsetTransformArgs *a, hipStream_t s);
void aln_pairset_launch_pick(const double *store, const uint32_t *list, uint32_t n_list, uint32_t e, double *out, hipStream_t s);

// ---- aln_loop.hip: the heuristic loop's step
void aln_loop_launch_classify(const aln_pair_result *res, const uint32_t *going, uint32_t n, double *best, uint32_t *cls, hipStream_t s);
void aln_loop_launch_settle(const uint32_t *entry, const int32_t *transform_status, uint32_t n, uint32_t *cls, hipStream_t s);
uint32_t aln_loop_tiles(uint32_t n);
// kind: 0 improved, 1 going, 2 finished
void aln_loop_launch_select(const uint32_t *cls, uint32_t n, uint32_t kind, const uint32_t *going, const aln_pair_result *res,
                            uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint32_t *out_pair, uint32_t *out_word,
                            aln_pair_result *out_res, hipStream_t s);

// ---- aln_seqset.hip: the resident sequence set
void aln_seqset_launch_expand(PairDesc *descs, uint32_t *order, uint64_t n, uint64_t k0, const aln_seqset_block *block, const uint64_t *seq_off,
                              const uint32_t *seq_len, hipStream_t s);
void aln_seqset_launch_gather(const aln_pair_result *res, double *f, int32_t *status, uint64_t n, unsigned long long *bad, hipStream_t s);
uint64_t aln_seqset_tiles(uint64_t n);
void aln_seqset_launch_select(const aln_pair_result *res, uint64_t n, uint64_t k0, double f_min, uint32_t *tile_count, uint32_t *tile_off,
                              uint32_t *count, uint64_t *hit_k, double *hit_f, hipStream_t s);

// ---- aln_report.hip: reports of held hits
void aln_report_launch(const HeldEntry *held, const aln_pair_result *res, const uint8_t *tb, const uint32_t *list, uint32_t n_list,
                       uint32_t n_held, const uint32_t *bits, uint32_t rows, uint32_t cols, uint32_t blank, uint32_t flags, aln_hit_report *rep,
                       hipStream_t s);
void aln_report_launch_filter(const aln_hit_report *rep, const HeldEntry *held, uint32_t n_held, const aln_hit_filter *filter,
                              uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint64_t cap, uint32_t *positions,
                              aln_hit_report *out, hipStream_t s);

// ---- aln_cluster.hip: clusters of an edge list
void aln_cluster_launch_held_edges(const aln_pair_result *res, const aln_hit_report *rep, const HeldEntry *held, const aln_hit_filter *filter,
                                   uint64_t m, uint32_t *ea, uint32_t *eb, hipStream_t s);
void aln_cluster_launch_init(const ClusterArgs *a, hipStream_t s);
void aln_cluster_launch_hook(const ClusterArgs *a, hipStream_t s);
void aln_cluster_launch_compress(const ClusterArgs *a, hipStream_t s);
void aln_cluster_launch_greedy_round(const ClusterArgs *a, hipStream_t s);
void aln_cluster_launch_greedy_assign(const ClusterArgs *a, hipStream_t s);
uint64_t aln_cluster_tiles(uint64_t n);
void aln_cluster_launch_finish(const ClusterArgs *a, uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint64_t cap,
                               aln_cluster_record *out, hipStream_t s);

// ---- aln_best.hip: the k best targets per query
int aln_warm_best(void);
void aln_best_launch_chunk(const double *f, const int32_t *status, uint64_t n, uint64_t k0, const aln_seqset_block *block, double f_min,
                           uint32_t flags, uint32_t slots, uint64_t *cand_key, uint32_t *cand_t, uint32_t *cand_n, uint64_t *run_key,
                           uint32_t *run_t, uint32_t *run_n, hipStream_t s);
uint64_t aln_best_tiles(uint64_t rows);
void aln_best_launch_count(const uint32_t *run_n, uint64_t rows, uint32_t *tile_count, uint64_t *tile_off, uint64_t *total, hipStream_t s);
void aln_best_launch_emit(const uint64_t *run_key, const uint32_t *run_t, const uint32_t *run_n, uint64_t rows, uint32_t slots,
                          const aln_seqset_block *block, const uint64_t *tile_off, uint64_t cap, uint64_t *out_k, double *out_f, hipStream_t s);

// ---- aln_prefilter.hip: the k-mer prefilter of a sequence set (aln_prefilter_rules.h)
// table: n_seqs rows of `stride` elements; n_words: n_seqs
void aln_prefilter_launch_index(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t n_seqs, uint32_t k,
                                uint32_t alphabet, uint32_t elements, uint32_t stride, uint32_t *table, uint32_t *n_words, hipStream_t s);
// workgroups of the sharing kernel for query rows q_rows and targets t_count (0: more than a grid holds)
uint32_t aln_prefilter_share_blocks(uint64_t q_rows, uint64_t t_count);
// pairs k0 .. k0 + n - 1 of the block, whose queries are rows q_lo .. q_lo + q_rows - 1 and whose targets lie in t_lo .. t_lo +
// t_count - 1 (absolute sequence numbers): shared[k - k0] and keep[k - k0] of every one of them
void aln_prefilter_launch_share(const uint32_t *table, const uint32_t *n_words, uint32_t stride, const aln_seqset_block *block, uint64_t k0,
                                uint64_t n, uint64_t q_lo, uint64_t q_rows, uint64_t t_lo, uint64_t t_count, uint32_t min_shared,
                                uint32_t min_per_1024, uint32_t *shared, uint8_t *keep, hipStream_t s);
// tile_count / tile_off: aln_seqset_tiles(n) words each; the kept pairs of the chunk in ascending order: out_k (block pair numbers)
// and out_shared, `room` entries each; count[0]: how many
void aln_prefilter_launch_compact(const uint8_t *keep, const uint32_t *shared, uint64_t n, uint64_t k0, uint32_t *tile_count,
                                  uint32_t *tile_off, uint32_t *count, uint64_t room, uint64_t *out_k, uint32_t *out_shared, hipStream_t s);
// descriptor i of the chunk = pair list[i] of the block (the sibling of aln_seqset_launch_expand)
void aln_prefilter_launch_expand_list(PairDesc *descs, uint32_t *order, uint64_t n, const uint64_t *list, const aln_seqset_block *block,
                                      const uint64_t *seq_off, const uint32_t *seq_len, hipStream_t s);

// ---- aln_search.hip: the k best targets per query over a candidate list (aln_search_rules.h)
int aln_warm_search(void);
// row_first: q_count + 1 words
void aln_search_launch_rows(const uint64_t *list, uint64_t count, uint64_t q_count, uint64_t t_count, uint32_t *row_first, hipStream_t s);
// list positions c0 .. c0 + n - 1 (f / status by chunk position) -> the running lists of the touched rows row0 .. row0 + rows - 1;
// piece_key / piece_t: n entries
void aln_search_launch_chunk(const uint64_t *list, const uint32_t *row_first, const double *f, const int32_t *status, uint64_t c0, uint64_t n,
                             uint64_t row0, uint64_t rows, const aln_seqset_block *block, double f_min, uint32_t flags, uint32_t slots,
                             uint64_t *piece_key, uint32_t *piece_t, uint64_t *run_key, uint32_t *run_t, uint32_t *run_n, hipStream_t s);

// ---- aln_profile.hip: the profiles of a sequence set's families (aln_profile_rules.h)
int aln_warm_profile(void);
void aln_profile_launch_slots(const uint32_t *centers, uint32_t n_centers, uint32_t n_seqs, uint32_t *slot_of, aln_profile_record *rec, hipStream_t s);
void aln_profile_launch(const ProfileArgs *a, hipStream_t s);

// ---- aln_msa.hip: the family alignments of a sequence set (aln_msa_rules.h)
int aln_warm_msa(void);
void aln_msa_launch_plan(const MsaArgs *a, const uint32_t *centers, uint32_t *slot_of, hipStream_t s);
void aln_msa_launch_fill(const MsaArgs *a, hipStream_t s);

// ---- aln_cigar.hip: the CIGARs of a sequence set's held hits (aln_cigar_rules.h)
int aln_warm_cigar(void);
void aln_cigar_launch_plan(const CigarArgs *a, hipStream_t s);
void aln_cigar_launch_fill(const CigarArgs *a, hipStream_t s);

// ---- aln_wordjoin.hip: the sorted word index of a sequence set and the join over its posting lists (aln_wordjoin_rules.h)
// (keys, plan, expand and the sort's argument rules are aln_postings.h's, which aln_seedjoin.hip instantiates too; offsets serves both)
int aln_warm_wordjoin(void);
// rocPRIM's device radix sort of n 64-bit numbers over bits begin_bit .. end_bit - 1, in -> out; the host owns the temporary storage,
// whose size for n numbers the first call gives.  Both return a hipError_t; n < 2^31; a range that ends at bit 64 begins at bit 0
int aln_wordjoin_sort_temp_bytes(uint64_t n, size_t *bytes);
int aln_wordjoin_launch_sort(void *temp, size_t temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, uint32_t begin_bit, uint32_t end_bit,
                             hipStream_t s);
// keys: `total` entries, one per residue position of the packed set
void aln_wordjoin_launch_keys(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t n_seqs, uint64_t total, uint32_t k,
                              uint32_t alphabet, uint64_t *keys, hipStream_t s);
// sorted: n keys ascending -> entries: the distinct keys that are words, ascending (`room` entries), count[0]: how many; n_words (n_seqs,
// zeroed before): the entries per sequence.  tile_count / tile_off: aln_select_tiles(n) words each
void aln_wordjoin_launch_distinct(const uint64_t *sorted, uint64_t n, uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint64_t room,
                                  uint64_t *entries, uint64_t n_seqs, uint32_t *n_words, hipStream_t s);
// piece_first / piece_len: n_entries each; occ: block->q_count totals, zeroed before
void aln_wordjoin_launch_plan(const uint64_t *entries, uint64_t n_entries, const aln_seqset_block *block, uint32_t *piece_first, uint32_t *piece_len,
                              uint64_t *occ, hipStream_t s);
// offsets: n_entries exclusive sums of the piece lengths of the entries whose query lies in q_lo .. q_lo + q_rows - 1; total[0]: their
// sum (the host has bounded it below 2^32).  tile_count / tile_off: aln_select_tiles(n_entries) words each
void aln_wordjoin_launch_offsets(const uint64_t *entries, const uint32_t *piece_len, uint64_t n_entries, uint64_t q_lo, uint64_t q_rows,
                                 uint32_t *tile_count, uint32_t *tile_off, uint32_t *total, uint32_t *offsets, hipStream_t s);
// out: n_out pair numbers of the block (`pairs` pairs); errors[0] counts the positions that found none
void aln_wordjoin_launch_expand(const uint64_t *entries, const uint32_t *piece_first, const uint32_t *piece_len, const uint32_t *offsets,
                                uint64_t n_entries, uint64_t n_out, const aln_seqset_block *block, uint64_t pairs, uint64_t q_lo, uint64_t q_rows,
                                uint64_t *out, uint32_t *errors, hipStream_t s);
// sorted: n pair numbers ascending -> the kept (pair number, shared) appended in order: out_k and out_shared, `room` entries each;
// count[0]: how many.  shared (n words) and keep (n bytes) are scratch; tile_count / tile_off: aln_select_tiles(n) words each
void aln_wordjoin_launch_append(const uint64_t *sorted, uint64_t n, const aln_seqset_block *block, uint64_t pairs, const uint32_t *n_words,
                                uint64_t n_seqs, uint32_t min_shared, uint32_t min_per_1024, uint32_t *shared, uint8_t *keep, uint32_t *tile_count,
                                uint32_t *tile_off, uint32_t *count, uint64_t room, uint64_t *out_k, uint32_t *out_shared, hipStream_t s);

// ---- aln_seedjoin.hip: the positional word index of a sequence set and the seed join over it (aln_seedjoin_rules.h)
int aln_warm_seedjoin(void);
// rocPRIM's device radix sort of n (64-bit key, 32-bit value) pairs, stable, under the rules of aln_wordjoin_launch_sort (aln_postings.h)
int aln_seedjoin_sort_pairs_temp_bytes(uint64_t n, size_t *bytes);
int aln_seedjoin_launch_sort_pairs(void *temp, size_t temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *vals_in,
                                   uint32_t *vals_out, uint64_t n, uint32_t begin_bit, uint32_t end_bit, hipStream_t s);
// keys, pos: `total` entries each, one per residue position of the packed set
void aln_seedjoin_launch_keys(const uint8_t *seqs, const uint64_t *seq_off, const uint32_t *seq_len, uint64_t n_seqs, uint64_t total, uint32_t k,
                              uint32_t alphabet, uint64_t *keys, uint32_t *pos, hipStream_t s);
// sorted: n keys ascending -> count[0]: the keys that are words
void aln_seedjoin_launch_count(const uint64_t *sorted, uint64_t n, uint32_t *count, hipStream_t s);
// keys: the n occurrences of the index, ascending.  piece_first / piece_len: n each; row_seeds: block->q_count totals, zeroed before;
// counters[0], zeroed before: the distinct words with more than max_occ occurrences (max_occ == 0: none)
void aln_seedjoin_launch_plan(const uint64_t *keys, uint64_t n, const aln_seqset_block *block, uint32_t max_occ, uint32_t *piece_first,
                              uint32_t *piece_len, uint64_t *row_seeds, uint32_t *counters, hipStream_t s);
// out: the sort keys of the n_out seeds of query rows q_lo .. q_lo + q_rows - 1, whose pairs are numbers k_lo .. k_end - 1 of the
// block (offsets: aln_wordjoin_launch_offsets over keys and piece_len); errors[0] counts the seeds that name no such pair
void aln_seedjoin_launch_expand(const uint64_t *keys, const uint32_t *pos, const uint32_t *piece_first, const uint32_t *piece_len,
                                const uint32_t *offsets, uint64_t n, uint64_t n_out, const aln_seqset_block *block, uint64_t k_lo, uint64_t k_end,
                                uint64_t q_lo, uint64_t q_rows, uint64_t *out, uint32_t *errors, hipStream_t s);
// sorted: n sort keys ascending -> the kept (k_lo + pair, seeds, diag) appended in order: out_k, out_seeds and out_diag, `room` entries
// each; count[0]: how many; pairs_seen[0]: the pairs with a seed.  slots: n 64-bit words, zeroed before; errors[0] counts the keys
// beyond chunk_pairs.  tile_count / tile_off: aln_select_tiles(n) words each
void aln_seedjoin_launch_append(const uint64_t *sorted, uint64_t n, uint64_t k_lo, uint64_t chunk_pairs, uint32_t band, uint32_t min_seeds,
                                uint64_t *slots, uint32_t *errors, uint32_t *tile_count, uint32_t *tile_off, uint32_t *pairs_seen, uint32_t *count,
                                uint64_t room, uint64_t *out_k, uint32_t *out_seeds, int32_t *out_diag, hipStream_t s);

// ---- aln_seedchain.hip: the seed chains of a sequence set's candidate list (aln_seedchain_rules.h)
int aln_warm_seedchain(void);
// the resident set (n_seqs records, `total` residues) and its seed index P (n occurrences: keys ascending, pos beside them)
struct aln_seedchain_index {
    const uint8_t *seqs; const uint64_t *seq_off; const uint32_t *seq_len; uint64_t n_seqs, total;
    const uint64_t *keys; const uint32_t *pos; uint64_t n;
};
// candidates 0 .. n - 1 (cand_q / cand_t: their records): seeds[c] = A, chained[c] = the anchors it chains (0 where it overflows),
// offsets[c] = the chained anchors in front of it, total[0] = all of them; records[c]: the record of a pair that chains nothing (the
// chunks write the others).  errors[0] counts what never happens on a sound index
void aln_seedchain_launch_count(const aln_seedchain_index *x, const aln_seedchain_spec *sp, const uint32_t *cand_q, const uint32_t *cand_t, uint64_t n,
                                uint32_t *seeds, uint32_t *chained, uint64_t *offsets, uint64_t *total, aln_chain_record *records, uint32_t *errors,
                                hipStream_t s);
// candidates c0 .. c0 + m - 1, at most 2^22 of them: expand their anchors (8 bytes each) into `anchors` and chain them with `state`
// (16 bytes each) beside; both hold `room` = the run's chained anchors, the run's first at offset `base`
void aln_seedchain_launch_chunk(const aln_seedchain_index *x, const aln_seedchain_spec *sp, const uint32_t *cand_q, const uint32_t *cand_t, uint64_t c0,
                                uint64_t m, const uint32_t *seeds, const uint32_t *chained, const uint64_t *offsets, uint64_t base, uint64_t room,
                                uint64_t *anchors, void *state, aln_chain_record *records, uint32_t *errors, hipStream_t s);
// the kept entries of n in list order: their places, pair numbers and records, `room` each; count[0]: how many.  tile_count /
// tile_off: aln_select_tiles(n) words each
void aln_seedchain_launch_filter(const aln_chain_record *records, const uint64_t *cand_k, uint64_t n, int32_t min_score, uint32_t min_span,
                                 uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint64_t room, uint32_t *out_pos, uint64_t *out_k,
                                 aln_chain_record *out_records, hipStream_t s);

// ---- aln_strand.hip: the mirrors of a stranded sequence set (aln_strand_rules.h)
// seqs: 2 * total + 256 bytes, the first `total` the n records packed in order; off, len: theirs; map: 256 bytes
void aln_strand_launch_mirror(uint8_t *seqs, const uint64_t *off, const uint32_t *len, uint64_t n, uint64_t total, const uint8_t *map, hipStream_t s);

}
