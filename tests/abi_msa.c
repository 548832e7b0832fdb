/*
 * abi_msa.c -- the family-alignment calls of include/aligner_hip_msa.h called from C99 by a caller who has read nothing but the header.
 * Built with `gcc -std=c99 -Wall -Werror -Iinclude` (aligner_amd/build.py: build_msa_harness); pins the layout of the family's two
 * records at compile time and allocates every buffer with exactly the size the header's comment gives, followed by a guard zone that
 * is checked at the end.
 *
 * usage: abi_msa               no GPU: prints one `layout <type> <sizeof> <field> <offset> <size> ...` line per record (fields in
 *                              declaration order; tests/test_msa_rules_cpu.py compares them with the ctypes classes)
 *        abi_msa <case file>   on a GPU: a held pass over the full square of the case's sequence set, then aln_seqset_held_msa_plan and
 *                              aln_seqset_held_msa_fill without and with the filter on the case's labels and centres
 *                              (tests/test_msa_gpu.py writes the case and compares the printout with the reference)
 *
 * case file: whitespace-separated tokens in the fixed order main() reads them; an integer is decimal, a double the 16 hex digits of
 * its 64 bits:  n_seqs  len[n_seqs]  codes[sum of len]  rows cols  matrix[rows * cols]  del ext  f_min  blank  min_identity min_q_cover
 *               label[n_seqs]  n_centers  centers[n_centers]
 * output: `rc <label> <filter> <returned>` per call, then `records` (center rows width inserted per centre), `summary` (held
 * contributing self_pairs between_members unlisted overflow bytes total_rows), `row_hit` (every entry) and `out` (every byte) lines.
 * Exit status 0 iff every call returned ALN_OK and no guard was touched.
 */
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aligner_hip_msa.h"

#define PIN(name, cond) typedef char pin_##name[(cond) ? 1 : -1]
PIN(record_size, sizeof(aln_msa_record) == 16);
PIN(record_center, offsetof(aln_msa_record, center) == 0);
PIN(record_rows, offsetof(aln_msa_record, rows) == 4);
PIN(record_width, offsetof(aln_msa_record, width) == 8);
PIN(record_inserted, offsetof(aln_msa_record, inserted) == 12);
PIN(summary_size, sizeof(aln_msa_summary) == 48);
PIN(summary_held, offsetof(aln_msa_summary, held) == 0);
PIN(summary_contributing, offsetof(aln_msa_summary, contributing) == 8);
PIN(summary_self_pairs, offsetof(aln_msa_summary, self_pairs) == 16);
PIN(summary_between_members, offsetof(aln_msa_summary, between_members) == 20);
PIN(summary_unlisted, offsetof(aln_msa_summary, unlisted) == 24);
PIN(summary_overflow, offsetof(aln_msa_summary, overflow) == 28);
PIN(summary_bytes, offsetof(aln_msa_summary, bytes) == 32);
PIN(summary_total_rows, offsetof(aln_msa_summary, total_rows) == 40);

#define FIELD(type, field) printf(" %s %u %u", #field, (unsigned)offsetof(type, field), (unsigned)sizeof(((type *)0)->field))

static void print_layouts(void)
{
    printf("layout aln_msa_record %u", (unsigned)sizeof(aln_msa_record));
    FIELD(aln_msa_record, center); FIELD(aln_msa_record, rows); FIELD(aln_msa_record, width); FIELD(aln_msa_record, inserted);
    printf("\n");
    printf("layout aln_msa_summary %u", (unsigned)sizeof(aln_msa_summary));
    FIELD(aln_msa_summary, held); FIELD(aln_msa_summary, contributing); FIELD(aln_msa_summary, self_pairs);
    FIELD(aln_msa_summary, between_members); FIELD(aln_msa_summary, unlisted); FIELD(aln_msa_summary, overflow);
    FIELD(aln_msa_summary, bytes); FIELD(aln_msa_summary, total_rows);
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

static int g_fail = 0;
static void rc(const char *what, int with_filter, int got)
{
    printf("rc %s %d %d\n", what, with_filter, got);
    if (got != ALN_OK) { printf("error %s\n", aln_last_error()); g_fail = 1; }
}

int main(int argc, char **argv)
{
    if (argc < 2) { print_layouts(); return 0; }
    g_in = fopen(argv[1], "r");
    if (!g_in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int status = 0;
    aln_ctx *ctx = aln_create(0, &status);
    if (!ctx) { printf("rc create 0 %d\nerror %s\n", status, aln_last_error()); return 1; }

    const uint64_t n_seqs = read_u64();
    uint64_t *s_len = (uint64_t *)guarded(8 * n_seqs), *s_off = (uint64_t *)guarded(8 * n_seqs);
    uint64_t total_codes = 0;
    for (uint64_t i = 0; i < n_seqs; ++i) { s_len[i] = read_u64(); s_off[i] = total_codes; total_codes += s_len[i]; }
    uint8_t *codes = (uint8_t *)guarded(total_codes);
    for (uint64_t i = 0; i < total_codes; ++i) codes[i] = (uint8_t)read_u64();
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
    aln_hit_filter flt;
    memset(&flt, 0, sizeof flt);
    flt.min_identity = read_f64(); flt.min_q_cover = read_f64();
    uint32_t *label = (uint32_t *)guarded(4 * n_seqs);
    for (uint64_t i = 0; i < n_seqs; ++i) label[i] = (uint32_t)read_u64();
    const uint64_t n_centers = read_u64();
    uint32_t *centers = (uint32_t *)guarded(4 * n_centers);
    for (uint64_t i = 0; i < n_centers; ++i) centers[i] = (uint32_t)read_u64();

    aln_seqset *set = aln_seqset_create(ctx, codes, s_off, s_len, (size_t)n_seqs, &status);
    rc("seqset_create", 0, status);
    if (set) {
        aln_seqset_block blk;
        memset(&blk, 0, sizeof blk);
        blk.q_first = 0; blk.q_count = n_seqs; blk.t_first = 0; blk.t_count = n_seqs; blk.upper = 0;      /* the full square */
        uint64_t count = 0;
        rc("seqset_hits", 0, aln_seqset_hits(set, &p, &blk, f_min, &count));
        printf("held %" PRIu64 "\n", count);
        for (int with_filter = 0; with_filter <= 1; ++with_filter) {
            aln_msa_record *rec = (aln_msa_record *)guarded(sizeof(aln_msa_record) * n_centers);
            aln_msa_summary *sum = (aln_msa_summary *)guarded(sizeof(aln_msa_summary));
            rc("held_msa_plan", with_filter,
               aln_seqset_held_msa_plan(set, with_filter ? &p : NULL, 0, with_filter ? &flt : NULL, label, centers, n_centers, rec, sum));
            printf("records");
            for (uint64_t i = 0; i < n_centers; ++i)
                printf(" %u %u %u %u", (unsigned)rec[i].center, (unsigned)rec[i].rows, (unsigned)rec[i].width, (unsigned)rec[i].inserted);
            printf("\nsummary %" PRIu64 " %" PRIu64 " %u %u %u %u %" PRIu64 " %" PRIu64 "\n", sum->held, sum->contributing, (unsigned)sum->self_pairs,
                   (unsigned)sum->between_members, (unsigned)sum->unlisted, (unsigned)sum->overflow, sum->bytes, sum->total_rows);
            /* the fill's buffers have exactly the sizes the plan's summary gives */
            uint8_t *out = (uint8_t *)guarded((size_t)sum->bytes);
            uint32_t *row_hit = (uint32_t *)guarded(4 * (size_t)sum->total_rows);
            rc("held_msa_fill", with_filter, aln_seqset_held_msa_fill(set, out, sum->bytes, row_hit, sum->total_rows));
            printf("row_hit");
            for (uint64_t i = 0; i < sum->total_rows; ++i) printf(" %u", (unsigned)row_hit[i]);
            printf("\nout");
            for (uint64_t i = 0; i < sum->bytes; ++i) printf(" %u", (unsigned)out[i]);
            printf("\n");
        }
        aln_seqset_destroy(set);
    }
    aln_destroy(ctx);
    fclose(g_in);
    const int ok = guards_ok();
    printf("guards %s\n", ok ? "ok" : "TOUCHED");
    return (g_fail || !ok) ? 1 : 0;
}
