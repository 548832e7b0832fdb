/*
 * abi_seedchain.c -- the seed-chain family of include/aligner_hip_seedchain.h called from C99 by a caller who has read nothing but the
 * header.  Built with `gcc -std=c99 -Wall -Werror -Iinclude` (aligner_amd/build.py: build_seedchain_harness); pins the layouts of
 * aln_seedchain_spec, aln_chain_record and aln_seedchain_summary at compile time and allocates every output buffer with exactly the
 * size the header gives, followed by a guard zone that is checked at the end.
 *
 * usage: abi_seedchain               no GPU: prints `layout <struct> <sizeof> <field> <offset> <size> ...` per struct
 *                                    (tests/test_seedchain_rules_cpu.py compares them with the ctypes classes)
 *        abi_seedchain <case file>   on a GPU: seed_index, seed_join, candidate_chains, candidate_chain_filter, candidates,
 *                                    candidate_diags and candidate_chain_records on the case's sequence set
 *                                    (tests/test_seedchain_gpu.py writes the case and compares the printout)
 *
 * case file: whitespace-separated decimal integers:
 *   n_seqs  len[n_seqs]  codes[sum of len]  k alphabet max_occ max_gap max_skew gap_scale max_pair_seeds chunk_anchors  min_score min_span
 * output: `rc <call> <returned>` per call; `count <n>`; `chain <score> <anchors> <q_start> <q_end> <t_start> <t_end> <seeds> <flags>` per
 * candidate; `summary <anchors> <with_anchor> <overflowed> <chunks>`; `kept <n>`; `cand <index> <q> <t> <seeds> <diag>` and `rec ...`
 * (the fields of `chain`) per kept candidate; `guards ok`.  Exit status 0 iff every call returned ALN_OK and no guard was touched.
 */
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aligner_hip_seedchain.h"

#define PIN(name, cond) typedef char pin_##name[(cond) ? 1 : -1]
PIN(spec_size, sizeof(aln_seedchain_spec) == 48);
PIN(spec_k, offsetof(aln_seedchain_spec, k) == 0);
PIN(spec_alphabet, offsetof(aln_seedchain_spec, alphabet) == 4);
PIN(spec_max_occ, offsetof(aln_seedchain_spec, max_occ) == 8);
PIN(spec_max_gap, offsetof(aln_seedchain_spec, max_gap) == 12);
PIN(spec_max_skew, offsetof(aln_seedchain_spec, max_skew) == 16);
PIN(spec_gap_scale, offsetof(aln_seedchain_spec, gap_scale) == 20);
PIN(spec_max_pair_seeds, offsetof(aln_seedchain_spec, max_pair_seeds) == 24);
PIN(spec_chunk_anchors, offsetof(aln_seedchain_spec, chunk_anchors) == 28);
PIN(spec_flags, offsetof(aln_seedchain_spec, flags) == 32);
PIN(spec_reserved, offsetof(aln_seedchain_spec, reserved) == 36);
PIN(record_size, sizeof(aln_chain_record) == 32);
PIN(record_score, offsetof(aln_chain_record, score) == 0);
PIN(record_anchors, offsetof(aln_chain_record, anchors) == 4);
PIN(record_q_start, offsetof(aln_chain_record, q_start) == 8);
PIN(record_q_end, offsetof(aln_chain_record, q_end) == 12);
PIN(record_t_start, offsetof(aln_chain_record, t_start) == 16);
PIN(record_t_end, offsetof(aln_chain_record, t_end) == 20);
PIN(record_seeds, offsetof(aln_chain_record, seeds) == 24);
PIN(record_flags, offsetof(aln_chain_record, flags) == 28);
PIN(summary_size, sizeof(aln_seedchain_summary) == 32);
PIN(summary_anchors, offsetof(aln_seedchain_summary, anchors) == 0);
PIN(summary_with_anchor, offsetof(aln_seedchain_summary, with_anchor) == 8);
PIN(summary_overflowed, offsetof(aln_seedchain_summary, overflowed) == 16);
PIN(summary_chunks, offsetof(aln_seedchain_summary, chunks) == 24);

#define FIELD(type, field) printf(" %s %u %u", #field, (unsigned)offsetof(type, field), (unsigned)sizeof(((type *)0)->field))

static void print_layouts(void)
{
    printf("layout aln_seedchain_spec %u", (unsigned)sizeof(aln_seedchain_spec));
    FIELD(aln_seedchain_spec, k); FIELD(aln_seedchain_spec, alphabet); FIELD(aln_seedchain_spec, max_occ); FIELD(aln_seedchain_spec, max_gap);
    FIELD(aln_seedchain_spec, max_skew); FIELD(aln_seedchain_spec, gap_scale); FIELD(aln_seedchain_spec, max_pair_seeds);
    FIELD(aln_seedchain_spec, chunk_anchors); FIELD(aln_seedchain_spec, flags); FIELD(aln_seedchain_spec, reserved);
    printf("\n");
    printf("layout aln_chain_record %u", (unsigned)sizeof(aln_chain_record));
    FIELD(aln_chain_record, score); FIELD(aln_chain_record, anchors); FIELD(aln_chain_record, q_start); FIELD(aln_chain_record, q_end);
    FIELD(aln_chain_record, t_start); FIELD(aln_chain_record, t_end); FIELD(aln_chain_record, seeds); FIELD(aln_chain_record, flags);
    printf("\n");
    printf("layout aln_seedchain_summary %u", (unsigned)sizeof(aln_seedchain_summary));
    FIELD(aln_seedchain_summary, anchors); FIELD(aln_seedchain_summary, with_anchor); FIELD(aln_seedchain_summary, overflowed);
    FIELD(aln_seedchain_summary, chunks);
    printf("\n");
}

/* ---------------------------------------------------------------- guarded buffers */
#define GUARD 64
#define GUARD_BYTE 0xA5
#define MAX_BUFS 64
static unsigned char *g_bufs[MAX_BUFS];
static size_t g_sizes[MAX_BUFS];
static int g_nbufs = 0;

static void *guarded(size_t bytes)
{
    unsigned char *p = (unsigned char *)malloc(bytes + GUARD);
    if (!p || g_nbufs == MAX_BUFS) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, 0, bytes);
    memset(p + bytes, GUARD_BYTE, GUARD);
    g_bufs[g_nbufs] = p; g_sizes[g_nbufs] = bytes; ++g_nbufs;
    return p;
}
static int guards_ok(void)
{
    int ok = 1;
    for (int i = 0; i < g_nbufs; ++i)
        for (int k = 0; k < GUARD; ++k)
            if (g_bufs[i][g_sizes[i] + k] != GUARD_BYTE) ok = 0;
    return ok;
}

static FILE *g_in;
static int64_t read_i64(void)
{
    int64_t v = 0;
    if (fscanf(g_in, "%" SCNd64, &v) != 1) { fprintf(stderr, "case file: an integer is missing\n"); exit(2); }
    return v;
}

static int g_fail = 0;
static void rc(const char *what, int got)
{
    printf("rc %s %d\n", what, got);
    if (got != ALN_OK) { printf("error %s\n", aln_last_error()); g_fail = 1; }
}

static void print_record(const char *tag, const aln_chain_record *r)
{
    printf("%s %d %u %u %u %u %u %u %u\n", tag, (int)r->score, (unsigned)r->anchors, (unsigned)r->q_start, (unsigned)r->q_end, (unsigned)r->t_start,
           (unsigned)r->t_end, (unsigned)r->seeds, (unsigned)r->flags);
}

int main(int argc, char **argv)
{
    if (argc < 2) { print_layouts(); return 0; }
    g_in = fopen(argv[1], "r");
    if (!g_in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int status = 0;
    aln_ctx *ctx = aln_create(0, &status);
    if (!ctx) { printf("rc create %d\nerror %s\n", status, aln_last_error()); return 1; }

    const uint64_t n_seqs = (uint64_t)read_i64();
    uint64_t *s_len = (uint64_t *)guarded(8 * n_seqs), *s_off = (uint64_t *)guarded(8 * n_seqs);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_seqs; ++i) { s_len[i] = (uint64_t)read_i64(); s_off[i] = total; total += s_len[i]; }
    uint8_t *codes = (uint8_t *)guarded(total);
    for (uint64_t i = 0; i < total; ++i) codes[i] = (uint8_t)read_i64();
    aln_seedchain_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.k = (uint32_t)read_i64(); spec.alphabet = (uint32_t)read_i64(); spec.max_occ = (uint32_t)read_i64();
    spec.max_gap = (uint32_t)read_i64(); spec.max_skew = (uint32_t)read_i64(); spec.gap_scale = (uint32_t)read_i64();
    spec.max_pair_seeds = (uint32_t)read_i64(); spec.chunk_anchors = (uint32_t)read_i64();
    const int32_t min_score = (int32_t)read_i64();
    const uint32_t min_span = (uint32_t)read_i64();
    aln_seedjoin_spec join;
    memset(&join, 0, sizeof join);
    join.k = spec.k; join.alphabet = spec.alphabet; join.min_seeds = 1; join.max_occ = spec.max_occ;

    aln_seqset *set = aln_seqset_create(ctx, codes, s_off, s_len, (size_t)n_seqs, &status);
    rc("seqset_create", status);
    if (set) {
        rc("seed_index", aln_seqset_seed_index(set, spec.k, spec.alphabet, NULL));
        aln_seqset_block blk;
        memset(&blk, 0, sizeof blk);
        blk.q_first = 0; blk.q_count = n_seqs; blk.t_first = 0; blk.t_count = n_seqs; blk.upper = 1;
        uint64_t count = 0;
        rc("seed_join", aln_seqset_seed_join(set, &join, &blk, NULL, &count));
        printf("count %" PRIu64 "\n", count);
        aln_chain_record *chains = (aln_chain_record *)guarded(sizeof(aln_chain_record) * count);
        aln_seedchain_summary *summary = (aln_seedchain_summary *)guarded(sizeof(aln_seedchain_summary));
        rc("candidate_chains", aln_seqset_candidate_chains(set, &spec, 0, count, chains, summary));
        for (uint64_t c = 0; c < count; ++c) print_record("chain", &chains[c]);
        printf("summary %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", summary->anchors, summary->with_anchor, summary->overflowed, summary->chunks);
        uint64_t kept = 0;
        rc("candidate_chain_filter", aln_seqset_candidate_chain_filter(set, &spec, min_score, min_span, summary, &kept));
        printf("kept %" PRIu64 "\n", kept);
        uint64_t *index = (uint64_t *)guarded(8 * kept);
        uint32_t *q = (uint32_t *)guarded(4 * kept), *t = (uint32_t *)guarded(4 * kept), *seeds = (uint32_t *)guarded(4 * kept);
        int32_t *diag = (int32_t *)guarded(4 * kept);
        aln_chain_record *recs = (aln_chain_record *)guarded(sizeof(aln_chain_record) * kept);
        rc("candidates", aln_seqset_candidates(set, 0, kept, index, q, t, seeds));
        rc("candidate_diags", aln_seqset_candidate_diags(set, 0, kept, diag));
        rc("candidate_chain_records", aln_seqset_candidate_chain_records(set, 0, kept, recs));
        for (uint64_t c = 0; c < kept; ++c) {
            printf("cand %" PRIu64 " %u %u %u %d\n", index[c], (unsigned)q[c], (unsigned)t[c], (unsigned)seeds[c], (int)diag[c]);
            print_record("rec", &recs[c]);
        }
        aln_seqset_destroy(set);
    }
    aln_destroy(ctx);
    fclose(g_in);
    const int ok = guards_ok();
    printf("guards %s\n", ok ? "ok" : "TOUCHED");
    return (g_fail || !ok) ? 1 : 0;
}
