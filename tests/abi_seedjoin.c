/*
 * abi_seedjoin.c -- the seed-join family of include/aligner_hip_seedjoin.h called from C99 by a caller who has read nothing but the
 * header.  Built with `gcc -std=c99 -Wall -Werror -Iinclude` (aligner_amd/build.py: build_seedjoin_harness); pins the layouts of
 * aln_seedjoin_spec and aln_seedjoin_summary at compile time and allocates every output buffer with exactly the size the header gives,
 * followed by a guard zone that is checked at the end.
 *
 * usage: abi_seedjoin                no GPU: prints `layout <struct> <sizeof> <field> <offset> <size> ...` per struct
 *                                    (tests/test_seedjoin_rules_cpu.py compares them with the ctypes classes)
 *        abi_seedjoin <case file>    on a GPU: seed_index, seed_join, candidates, candidate_diags, candidate_hits and held_list on the
 *                                    case's sequence set (tests/test_seedjoin_gpu.py writes the case and compares the printout)
 *
 * case file: whitespace-separated tokens; an integer is decimal, a double the 16 hex digits of its 64 bits:
 *   n_seqs  len[n_seqs]  codes[sum of len]  rows cols  matrix[rows * cols]  del ext  f_min  blank  k alphabet min_seeds band max_occ
 *   chunk_seeds
 * output: `rc <call> <returned>` per call; `occurrences <n>`; `summary <seeds> <pairs> <dropped> <chunks>`; `count <n>`;
 * `cand <index> <q> <t> <seeds> <diag>` per candidate; `held <n>`; `hit <index> <q> <t> <f as hex>` per held hit; `guards ok`.
 * Exit status 0 iff every call returned ALN_OK and no guard was touched.
 */
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aligner_hip_seedjoin.h"

#define PIN(name, cond) typedef char pin_##name[(cond) ? 1 : -1]
PIN(spec_size, sizeof(aln_seedjoin_spec) == 32);
PIN(spec_k, offsetof(aln_seedjoin_spec, k) == 0);
PIN(spec_alphabet, offsetof(aln_seedjoin_spec, alphabet) == 4);
PIN(spec_min_seeds, offsetof(aln_seedjoin_spec, min_seeds) == 8);
PIN(spec_band, offsetof(aln_seedjoin_spec, band) == 12);
PIN(spec_max_occ, offsetof(aln_seedjoin_spec, max_occ) == 16);
PIN(spec_chunk_seeds, offsetof(aln_seedjoin_spec, chunk_seeds) == 20);
PIN(spec_flags, offsetof(aln_seedjoin_spec, flags) == 24);
PIN(spec_reserved, offsetof(aln_seedjoin_spec, reserved) == 28);
PIN(summary_size, sizeof(aln_seedjoin_summary) == 32);
PIN(summary_seeds, offsetof(aln_seedjoin_summary, seeds) == 0);
PIN(summary_pairs, offsetof(aln_seedjoin_summary, pairs_with_seed) == 8);
PIN(summary_dropped, offsetof(aln_seedjoin_summary, words_dropped) == 16);
PIN(summary_chunks, offsetof(aln_seedjoin_summary, chunks) == 24);

#define FIELD(type, field) printf(" %s %u %u", #field, (unsigned)offsetof(type, field), (unsigned)sizeof(((type *)0)->field))

static void print_layouts(void)
{
    printf("layout aln_seedjoin_spec %u", (unsigned)sizeof(aln_seedjoin_spec));
    FIELD(aln_seedjoin_spec, k); FIELD(aln_seedjoin_spec, alphabet); FIELD(aln_seedjoin_spec, min_seeds); FIELD(aln_seedjoin_spec, band);
    FIELD(aln_seedjoin_spec, max_occ); FIELD(aln_seedjoin_spec, chunk_seeds); FIELD(aln_seedjoin_spec, flags); FIELD(aln_seedjoin_spec, reserved);
    printf("\n");
    printf("layout aln_seedjoin_summary %u", (unsigned)sizeof(aln_seedjoin_summary));
    FIELD(aln_seedjoin_summary, seeds); FIELD(aln_seedjoin_summary, pairs_with_seed); FIELD(aln_seedjoin_summary, words_dropped);
    FIELD(aln_seedjoin_summary, chunks);
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
static uint64_t read_u64(void)
{
    uint64_t v = 0;
    if (fscanf(g_in, "%" SCNu64, &v) != 1) { fprintf(stderr, "case file: an integer is missing\n"); exit(2); }
    return v;
}
static double read_f64(void)
{
    uint64_t bits = 0;
    double d;
    if (fscanf(g_in, "%" SCNx64, &bits) != 1) { fprintf(stderr, "case file: a double is missing\n"); exit(2); }
    memcpy(&d, &bits, 8);
    return d;
}
static uint64_t f64_bits(double d)
{
    uint64_t bits;
    memcpy(&bits, &d, 8);
    return bits;
}

static int g_fail = 0;
static void rc(const char *what, int got)
{
    printf("rc %s %d\n", what, got);
    if (got != ALN_OK) { printf("error %s\n", aln_last_error()); g_fail = 1; }
}

int main(int argc, char **argv)
{
    if (argc < 2) { print_layouts(); return 0; }
    g_in = fopen(argv[1], "r");
    if (!g_in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int status = 0;
    aln_ctx *ctx = aln_create(0, &status);
    if (!ctx) { printf("rc create %d\nerror %s\n", status, aln_last_error()); return 1; }

    const uint64_t n_seqs = read_u64();
    uint64_t *s_len = (uint64_t *)guarded(8 * n_seqs), *s_off = (uint64_t *)guarded(8 * n_seqs);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_seqs; ++i) { s_len[i] = read_u64(); s_off[i] = total; total += s_len[i]; }
    uint8_t *codes = (uint8_t *)guarded(total);
    for (uint64_t i = 0; i < total; ++i) codes[i] = (uint8_t)read_u64();
    const uint32_t rows = (uint32_t)read_u64(), cols = (uint32_t)read_u64();
    double *matrix = (double *)guarded(8 * (size_t)rows * cols);
    for (uint64_t i = 0; i < (uint64_t)rows * cols; ++i) matrix[i] = read_f64();
    aln_params p;
    memset(&p, 0, sizeof p);
    p.semantics = ALN_CORE_LOCAL;
    p.del = read_f64(); p.ext = read_f64();
    p.matrix = matrix; p.rows = rows; p.cols = cols; p.row_stride = cols;
    p.outputs = ALN_OUT_SCORE | ALN_OUT_TRACEBACK;
    const double f_min = read_f64();
    p.blank_code = (uint8_t)read_u64();
    aln_seedjoin_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.k = (uint32_t)read_u64(); spec.alphabet = (uint32_t)read_u64();
    spec.min_seeds = (uint32_t)read_u64(); spec.band = (uint32_t)read_u64();
    spec.max_occ = (uint32_t)read_u64(); spec.chunk_seeds = (uint32_t)read_u64();

    aln_seqset *set = aln_seqset_create(ctx, codes, s_off, s_len, (size_t)n_seqs, &status);
    rc("seqset_create", status);
    if (set) {
        uint64_t *occurrences = (uint64_t *)guarded(8);
        rc("seed_index", aln_seqset_seed_index(set, spec.k, spec.alphabet, occurrences));
        printf("occurrences %" PRIu64 "\n", occurrences[0]);
        aln_seqset_block blk;
        memset(&blk, 0, sizeof blk);
        blk.q_first = 0; blk.q_count = n_seqs; blk.t_first = 0; blk.t_count = n_seqs; blk.upper = 1;
        aln_seedjoin_summary *summary = (aln_seedjoin_summary *)guarded(sizeof(aln_seedjoin_summary));
        uint64_t count = 0;
        rc("seed_join", aln_seqset_seed_join(set, &spec, &blk, summary, &count));
        printf("summary %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", summary->seeds, summary->pairs_with_seed, summary->words_dropped,
               summary->chunks);
        printf("count %" PRIu64 "\n", count);
        uint64_t *index = (uint64_t *)guarded(8 * count);
        uint32_t *q = (uint32_t *)guarded(4 * count), *t = (uint32_t *)guarded(4 * count), *seeds = (uint32_t *)guarded(4 * count);
        int32_t *diag = (int32_t *)guarded(4 * count);
        rc("candidates", aln_seqset_candidates(set, 0, count, index, q, t, seeds));
        rc("candidate_diags", aln_seqset_candidate_diags(set, 0, count, diag));
        for (uint64_t c = 0; c < count; ++c)
            printf("cand %" PRIu64 " %u %u %u %d\n", index[c], (unsigned)q[c], (unsigned)t[c], (unsigned)seeds[c], (int)diag[c]);
        uint64_t held = 0;
        rc("candidate_hits", aln_seqset_candidate_hits(set, &p, f_min, &held));
        printf("held %" PRIu64 "\n", held);
        uint64_t *h_index = (uint64_t *)guarded(8 * held);
        uint32_t *h_q = (uint32_t *)guarded(4 * held), *h_t = (uint32_t *)guarded(4 * held);
        double *h_f = (double *)guarded(8 * held);
        rc("held_list", aln_seqset_held_list(set, 0, held, h_index, h_q, h_t, h_f));
        for (uint64_t h = 0; h < held; ++h) printf("hit %" PRIu64 " %u %u %016" PRIx64 "\n", h_index[h], (unsigned)h_q[h], (unsigned)h_t[h], f64_bits(h_f[h]));
        aln_seqset_destroy(set);
    }
    aln_destroy(ctx);
    fclose(g_in);
    const int ok = guards_ok();
    printf("guards %s\n", ok ? "ok" : "TOUCHED");
    return (g_fail || !ok) ? 1 : 0;
}
