/*
 * abi_cigar.c -- the CIGAR calls of include/aligner_hip_cigar.h called from C99 by a caller who has read nothing but the header.
 * Built with `gcc -std=c99 -Wall -Werror -Iinclude` (aligner_amd/build.py: build_cigar_harness); pins the layout of the family's two
 * records at compile time and allocates every buffer with exactly the size the header's comment gives, followed by a guard zone that
 * is checked at the end.
 *
 * usage: abi_cigar               no GPU: prints one `layout <type> <sizeof> <field> <offset> <size> ...` line per record (fields in
 *                                declaration order; tests/test_cigar_rules_cpu.py compares them with the ctypes classes)
 *        abi_cigar <case file>   on a GPU: a held pass over the full square of the case's sequence set, then aln_seqset_held_cigar_plan
 *                                and aln_seqset_held_cigar_fill on the case's list, once per listed flags word
 *                                (tests/test_cigar_gpu.py writes the case and compares the printout with the reference)
 *
 * case file: whitespace-separated tokens in the fixed order main() reads them; an integer is decimal, a double the 16 hex digits of
 * its 64 bits:  n_seqs  len[n_seqs]  codes[sum of len]  rows cols  matrix[rows * cols]  del ext  f_min  blank  n  which[n]
 *               n_flags  flags[n_flags]
 * output: `rc <label> <flags> <returned>` per call, then `records` (the eight words per listed hit), `summary` (held listed total_ops
 * failed padded overflow), `offsets` (n + 1 entries) and `ops` (every word) lines.
 * Exit status 0 iff every call returned ALN_OK and no guard was touched.
 */
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aligner_hip_cigar.h"

#define PIN(name, cond) typedef char pin_##name[(cond) ? 1 : -1]
PIN(record_size, sizeof(aln_cigar_record) == 32);
PIN(record_n_ops, offsetof(aln_cigar_record, n_ops) == 0);
PIN(record_q_start, offsetof(aln_cigar_record, q_start) == 4);
PIN(record_q_end, offsetof(aln_cigar_record, q_end) == 8);
PIN(record_t_start, offsetof(aln_cigar_record, t_start) == 12);
PIN(record_t_end, offsetof(aln_cigar_record, t_end) == 16);
PIN(record_matches, offsetof(aln_cigar_record, matches) == 20);
PIN(record_block, offsetof(aln_cigar_record, block) == 24);
PIN(record_status, offsetof(aln_cigar_record, status) == 28);
PIN(summary_size, sizeof(aln_cigar_summary) == 48);
PIN(summary_held, offsetof(aln_cigar_summary, held) == 0);
PIN(summary_listed, offsetof(aln_cigar_summary, listed) == 8);
PIN(summary_total_ops, offsetof(aln_cigar_summary, total_ops) == 16);
PIN(summary_failed, offsetof(aln_cigar_summary, failed) == 24);
PIN(summary_padded, offsetof(aln_cigar_summary, padded) == 28);
PIN(summary_overflow, offsetof(aln_cigar_summary, overflow) == 32);
PIN(summary_reserved, offsetof(aln_cigar_summary, reserved) == 36);
PIN(flags, ALN_CIGAR_EXTENDED == 1 && ALN_CIGAR_CLIPS == 2);

#define FIELD(type, field) printf(" %s %u %u", #field, (unsigned)offsetof(type, field), (unsigned)sizeof(((type *)0)->field))

static void print_layouts(void)
{
    printf("layout aln_cigar_record %u", (unsigned)sizeof(aln_cigar_record));
    FIELD(aln_cigar_record, n_ops); FIELD(aln_cigar_record, q_start); FIELD(aln_cigar_record, q_end); FIELD(aln_cigar_record, t_start);
    FIELD(aln_cigar_record, t_end); FIELD(aln_cigar_record, matches); FIELD(aln_cigar_record, block); FIELD(aln_cigar_record, status);
    printf("\n");
    printf("layout aln_cigar_summary %u", (unsigned)sizeof(aln_cigar_summary));
    FIELD(aln_cigar_summary, held); FIELD(aln_cigar_summary, listed); FIELD(aln_cigar_summary, total_ops); FIELD(aln_cigar_summary, failed);
    FIELD(aln_cigar_summary, padded); FIELD(aln_cigar_summary, overflow); FIELD(aln_cigar_summary, reserved);
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
static void rc(const char *what, unsigned flags, int got)
{
    printf("rc %s %u %d\n", what, flags, got);
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
    const uint64_t n = read_u64();
    uint32_t *which = (uint32_t *)guarded(4 * n);
    for (uint64_t i = 0; i < n; ++i) which[i] = (uint32_t)read_u64();
    const uint64_t n_flags = read_u64();
    uint32_t *flags = (uint32_t *)guarded(4 * n_flags);
    for (uint64_t i = 0; i < n_flags; ++i) flags[i] = (uint32_t)read_u64();

    aln_seqset *set = aln_seqset_create(ctx, codes, s_off, s_len, (size_t)n_seqs, &status);
    rc("seqset_create", 0, status);
    if (set) {
        aln_seqset_block blk;
        memset(&blk, 0, sizeof blk);
        blk.q_first = 0; blk.q_count = n_seqs; blk.t_first = 0; blk.t_count = n_seqs; blk.upper = 0;      /* the full square */
        uint64_t count = 0;
        rc("seqset_hits", 0, aln_seqset_hits(set, &p, &blk, f_min, &count));
        printf("held %" PRIu64 "\n", count);
        for (uint64_t v = 0; v < n_flags; ++v) {
            aln_cigar_record *rec = (aln_cigar_record *)guarded(sizeof(aln_cigar_record) * n);
            aln_cigar_summary *sum = (aln_cigar_summary *)guarded(sizeof(aln_cigar_summary));
            rc("held_cigar_plan", (unsigned)flags[v], aln_seqset_held_cigar_plan(set, flags[v], which, n, rec, sum));
            printf("records");
            for (uint64_t i = 0; i < n; ++i)
                printf(" %u %u %u %u %u %u %u %d", (unsigned)rec[i].n_ops, (unsigned)rec[i].q_start, (unsigned)rec[i].q_end, (unsigned)rec[i].t_start,
                       (unsigned)rec[i].t_end, (unsigned)rec[i].matches, (unsigned)rec[i].block, (int)rec[i].status);
            printf("\nsummary %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u\n", sum->held, sum->listed, sum->total_ops, (unsigned)sum->failed,
                   (unsigned)sum->padded, (unsigned)sum->overflow);
            /* the fill's buffers have exactly the sizes the plan's summary gives */
            uint32_t *ops = (uint32_t *)guarded(4 * (size_t)sum->total_ops);
            uint64_t *off = (uint64_t *)guarded(8 * (size_t)(n + 1));
            rc("held_cigar_fill", (unsigned)flags[v], aln_seqset_held_cigar_fill(set, ops, sum->total_ops, off, n + 1));
            printf("offsets");
            for (uint64_t i = 0; i <= n; ++i) printf(" %" PRIu64, off[i]);
            printf("\nops");
            for (uint64_t i = 0; i < sum->total_ops; ++i) printf(" %u", (unsigned)ops[i]);
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
