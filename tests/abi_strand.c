/*
 * abi_strand.c -- the strand calls of include/aligner_hip_strand.h called from C99 by a caller who has read nothing but the header.
 * Built with `gcc -std=c99 -Wall -Werror -Iinclude` (aligner_amd/build.py: build_strand_harness); pins the layout of the family's
 * record at compile time and allocates every buffer with exactly the size the header's comment gives, followed by a guard zone that is
 * checked at the end.
 *
 * usage: abi_strand              no GPU: prints one `layout <type> <sizeof> <field> <offset> <size> ...` line for the record (fields in
 *                                declaration order; tests/test_strand_rules_cpu.py compares them with the ctypes class)
 *        abi_strand <case file>  on a GPU: aln_seqset_create_stranded on the case's records and map, aln_seqset_strand_records,
 *                                aln_seqset_strand_residues over all 2n resident records, a held pass over the full square of the 2n,
 *                                then aln_seqset_held_strand_cigar_plan and _fill on the case's list, once per listed flags word
 *                                (tests/test_strand_gpu.py writes the case and compares the printout with the reference)
 *
 * case file: whitespace-separated tokens in the fixed order main() reads them; an integer is decimal, a double the 16 hex digits of
 * its 64 bits:  n_seqs  len[n_seqs]  codes[sum of len]  map[256]  rows cols  matrix[rows * cols]  del ext  f_min  blank  n  which[n]
 *               n_flags  flags[n_flags]
 * output: `rc <label> <flags> <returned>` per call, `stranded <n>`, `residues` (every byte of the 2n records in order), then per flags
 * word `records` (the eight words per listed hit), `strands` (q_rec t_rec strand q_mirror t_mirror reserved reserved2 per listed hit),
 * `summary` (held listed total_ops failed padded overflow), `offsets` (n + 1 entries) and `ops` (every word) lines.
 * Exit status 0 iff every call returned ALN_OK and no guard was touched.
 */
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aligner_hip_strand.h"

#define PIN(name, cond) typedef char pin_##name[(cond) ? 1 : -1]
PIN(strand_size, sizeof(aln_strand_record) == 16);
PIN(strand_q_rec, offsetof(aln_strand_record, q_rec) == 0);
PIN(strand_t_rec, offsetof(aln_strand_record, t_rec) == 4);
PIN(strand_strand, offsetof(aln_strand_record, strand) == 8);
PIN(strand_q_mirror, offsetof(aln_strand_record, q_mirror) == 9);
PIN(strand_t_mirror, offsetof(aln_strand_record, t_mirror) == 10);
PIN(strand_reserved, offsetof(aln_strand_record, reserved) == 11);
PIN(strand_reserved2, offsetof(aln_strand_record, reserved2) == 12);
PIN(record_size, sizeof(aln_cigar_record) == 32);

#define FIELD(type, field) printf(" %s %u %u", #field, (unsigned)offsetof(type, field), (unsigned)sizeof(((type *)0)->field))

static void print_layouts(void)
{
    printf("layout aln_strand_record %u", (unsigned)sizeof(aln_strand_record));
    FIELD(aln_strand_record, q_rec); FIELD(aln_strand_record, t_rec); FIELD(aln_strand_record, strand); FIELD(aln_strand_record, q_mirror);
    FIELD(aln_strand_record, t_mirror); FIELD(aln_strand_record, reserved); FIELD(aln_strand_record, reserved2);
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
    uint8_t *map = (uint8_t *)guarded(256);
    for (int i = 0; i < 256; ++i) map[i] = (uint8_t)read_u64();
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

    aln_seqset *set = aln_seqset_create_stranded(ctx, codes, s_off, s_len, (size_t)n_seqs, map, &status);
    rc("seqset_create_stranded", 0, status);
    if (set) {
        printf("stranded %" PRIu64 "\n", aln_seqset_strand_records(set));
        /* all 2n resident records, packed: exactly 2 * total bytes */
        uint64_t *r_off = (uint64_t *)guarded(8 * 2 * n_seqs);
        for (uint64_t i = 0; i < 2 * n_seqs; ++i) r_off[i] = (i < n_seqs ? 0 : total_codes) + s_off[i % n_seqs];
        uint8_t *resident = (uint8_t *)guarded(2 * total_codes);
        rc("strand_residues", 0, aln_seqset_strand_residues(set, 0, 2 * n_seqs, r_off, resident));
        printf("residues");
        for (uint64_t i = 0; i < 2 * total_codes; ++i) printf(" %u", (unsigned)resident[i]);
        printf("\n");
        aln_seqset_block blk;
        memset(&blk, 0, sizeof blk);
        blk.q_first = 0; blk.q_count = 2 * n_seqs; blk.t_first = 0; blk.t_count = 2 * n_seqs; blk.upper = 0;      /* the full square of the 2n */
        uint64_t count = 0;
        rc("seqset_hits", 0, aln_seqset_hits(set, &p, &blk, f_min, &count));
        printf("held %" PRIu64 "\n", count);
        for (uint64_t v = 0; v < n_flags; ++v) {
            aln_cigar_record *rec = (aln_cigar_record *)guarded(sizeof(aln_cigar_record) * n);
            aln_cigar_summary *sum = (aln_cigar_summary *)guarded(sizeof(aln_cigar_summary));
            aln_strand_record *str = (aln_strand_record *)guarded(sizeof(aln_strand_record) * n);
            rc("held_strand_cigar_plan", (unsigned)flags[v], aln_seqset_held_strand_cigar_plan(set, flags[v], which, n, rec, str, sum));
            printf("records");
            for (uint64_t i = 0; i < n; ++i)
                printf(" %u %u %u %u %u %u %u %d", (unsigned)rec[i].n_ops, (unsigned)rec[i].q_start, (unsigned)rec[i].q_end, (unsigned)rec[i].t_start,
                       (unsigned)rec[i].t_end, (unsigned)rec[i].matches, (unsigned)rec[i].block, (int)rec[i].status);
            printf("\nstrands");
            for (uint64_t i = 0; i < n; ++i)
                printf(" %u %u %u %u %u %u %u", (unsigned)str[i].q_rec, (unsigned)str[i].t_rec, (unsigned)str[i].strand, (unsigned)str[i].q_mirror,
                       (unsigned)str[i].t_mirror, (unsigned)str[i].reserved, (unsigned)str[i].reserved2);
            printf("\nsummary %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u\n", sum->held, sum->listed, sum->total_ops, (unsigned)sum->failed,
                   (unsigned)sum->padded, (unsigned)sum->overflow);
            /* the fill's buffers have exactly the sizes the plan's summary gives */
            uint32_t *ops = (uint32_t *)guarded(4 * (size_t)sum->total_ops);
            uint64_t *off = (uint64_t *)guarded(8 * (size_t)(n + 1));
            rc("held_strand_cigar_fill", (unsigned)flags[v], aln_seqset_held_strand_cigar_fill(set, ops, sum->total_ops, off, n + 1));
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
