/*
 * abi_families.c -- every exported family of include/aligner_hip.h called from C99 by a caller who has read nothing but the header.
 *
 * tests/abi_harness.c covers aln_align_pair / aln_align_batch; this program covers the rest: the context helpers, the staged batch,
 * the window scan and its held hits, the shuffled copies, the matrix transforms, the pair set with its stored matrices, the sequence
 * set with hits, k best, significance, report and filter, and the device loop.  It is built with `gcc -std=c99 -Wall -Werror
 * -Iinclude` (aligner_amd/build.py: build_families_harness), pins the layout of every public record at compile time and allocates
 * every buffer with exactly the size the header's comment gives; every buffer is followed by a guard zone that is checked at the end.
 *
 * usage: abi_families               no GPU: prints one `layout <type> <sizeof> <field> <offset> <size> ...` line per record (fields in
 *                                   declaration order; tests/test_abi_layout_cpu.py compares them with the ctypes and Rust mirrors)
 *                                   and both ABI versions; exit status 0 iff they agree
 *        abi_families <case file>   on a GPU: calls every family in the order of main() and prints all it gets back
 *                                   (tests/test_abi_families_gpu.py writes the case and compares the printout with the references)
 *
 * case file: plain text, records `<key> <n> <v1> .. <vn>` in the fixed order main() reads them; an integer is decimal, a double is
 * the 16 hex digits of its 64 bits.  Sequences and pairs are named by their number in the sequence set (`set_len`, `set_codes`).
 *
 * output: one `<key> <values>` line per fact.  A double is printed as `<16 hex digits>/<%.17g>`; the comparison is on the hex bits.
 * Every call prints `rc <label> <returned> <expected>`; the expected value is ALN_OK except for the four planted refusals, whose
 * codes come from the case file (`refusals`).  Exit status 0 iff every call returned what was expected and no guard zone was touched.
 */
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aligner_hip.h"

/* compile-time layout pins (C99 has no _Static_assert): the sizes and offsets every binding relies on */
#define PIN(name, cond) typedef char pin_##name[(cond) ? 1 : -1]
PIN(result_size, sizeof(aln_pair_result) == 48);
PIN(result_f, offsetof(aln_pair_result, f) == 0);
PIN(result_score, offsetof(aln_pair_result, score) == 8);
PIN(result_end_y, offsetof(aln_pair_result, end_y) == 16);
PIN(result_start_y, offsetof(aln_pair_result, start_y) == 24);
PIN(result_aln_len, offsetof(aln_pair_result, aln_len) == 32);
PIN(result_status, offsetof(aln_pair_result, status) == 36);
PIN(result_passes, offsetof(aln_pair_result, passes) == 40);
PIN(result_flags, offsetof(aln_pair_result, flags) == 44);
PIN(params_size, sizeof(aln_params) == 64);
PIN(params_del, offsetof(aln_params, del) == 8);
PIN(params_matrix, offsetof(aln_params, matrix) == 24);
PIN(params_rows, offsetof(aln_params, rows) == 32);
PIN(params_stride, offsetof(aln_params, row_stride) == 40);
PIN(params_outputs, offsetof(aln_params, outputs) == 48);
PIN(params_blank, offsetof(aln_params, blank_code) == 52);
PIN(params_passes, offsetof(aln_params, max_passes) == 56);
PIN(geometry_size, sizeof(aln_scan_geometry) == 32);
PIN(geometry_first, offsetof(aln_scan_geometry, first) == 0);
PIN(geometry_step, offsetof(aln_scan_geometry, step) == 8);
PIN(geometry_width, offsetof(aln_scan_geometry, width) == 16);
PIN(geometry_reverse, offsetof(aln_scan_geometry, reverse) == 24);
PIN(geometry_reserved, offsetof(aln_scan_geometry, reserved) == 28);
PIN(spec_size, sizeof(aln_shuffle_spec) == 24);
PIN(spec_seed, offsetof(aln_shuffle_spec, seed) == 0);
PIN(spec_pair_base, offsetof(aln_shuffle_spec, pair_base) == 8);
PIN(spec_per_pair, offsetof(aln_shuffle_spec, per_pair) == 16);
PIN(spec_max_trim, offsetof(aln_shuffle_spec, max_trim) == 20);
PIN(block_size, sizeof(aln_seqset_block) == 40);
PIN(block_q_first, offsetof(aln_seqset_block, q_first) == 0);
PIN(block_q_count, offsetof(aln_seqset_block, q_count) == 8);
PIN(block_t_first, offsetof(aln_seqset_block, t_first) == 16);
PIN(block_t_count, offsetof(aln_seqset_block, t_count) == 24);
PIN(block_upper, offsetof(aln_seqset_block, upper) == 32);
PIN(block_reserved, offsetof(aln_seqset_block, reserved) == 36);
PIN(signif_size, sizeof(aln_signif_record) == 48);
PIN(signif_sum, offsetof(aln_signif_record, sum) == 0);
PIN(signif_sum_sq, offsetof(aln_signif_record, sum_sq) == 8);
PIN(signif_f_max, offsetof(aln_signif_record, f_max) == 16);
PIN(signif_n_ok, offsetof(aln_signif_record, n_ok) == 24);
PIN(signif_n_ge, offsetof(aln_signif_record, n_ge) == 28);
PIN(signif_status, offsetof(aln_signif_record, status) == 32);
PIN(signif_first_bad, offsetof(aln_signif_record, first_bad) == 36);
PIN(signif_reserved, offsetof(aln_signif_record, reserved) == 40);
PIN(report_size, sizeof(aln_hit_report) == 40);
PIN(report_columns, offsetof(aln_hit_report, columns) == 0);
PIN(report_identical, offsetof(aln_hit_report, identical) == 4);
PIN(report_positive, offsetof(aln_hit_report, positive) == 8);
PIN(report_mismatch, offsetof(aln_hit_report, mismatch) == 12);
PIN(report_q_gap, offsetof(aln_hit_report, q_gap) == 16);
PIN(report_t_gap, offsetof(aln_hit_report, t_gap) == 20);
PIN(report_q_gap_open, offsetof(aln_hit_report, q_gap_open) == 24);
PIN(report_t_gap_open, offsetof(aln_hit_report, t_gap_open) == 28);
PIN(report_status, offsetof(aln_hit_report, status) == 32);
PIN(report_reserved, offsetof(aln_hit_report, reserved) == 36);
PIN(filter_size, sizeof(aln_hit_filter) == 32);
PIN(filter_min_identity, offsetof(aln_hit_filter, min_identity) == 0);
PIN(filter_min_q_cover, offsetof(aln_hit_filter, min_q_cover) == 8);
PIN(filter_min_t_cover, offsetof(aln_hit_filter, min_t_cover) == 16);
PIN(filter_min_columns, offsetof(aln_hit_filter, min_columns) == 24);
PIN(filter_reserved, offsetof(aln_hit_filter, reserved) == 28);

/* ---------------------------------------------------------------- layout printout */
#define FIELD(type, field) printf(" %s %u %u", #field, (unsigned)offsetof(type, field), (unsigned)sizeof(((type *)0)->field))
#define LAYOUT_BEGIN(type) printf("layout %s %u", #type, (unsigned)sizeof(type))
#define LAYOUT_END() printf("\n")

static void print_layouts(void)
{
    LAYOUT_BEGIN(aln_params);
    FIELD(aln_params, semantics); FIELD(aln_params, heuristics_present); FIELD(aln_params, del); FIELD(aln_params, ext);
    FIELD(aln_params, matrix); FIELD(aln_params, rows); FIELD(aln_params, cols); FIELD(aln_params, row_stride);
    FIELD(aln_params, outputs); FIELD(aln_params, blank_code); FIELD(aln_params, force_f64); FIELD(aln_params, force_serial);
    FIELD(aln_params, force_generic); FIELD(aln_params, max_passes);
    LAYOUT_END();
    LAYOUT_BEGIN(aln_pair_result);
    FIELD(aln_pair_result, f); FIELD(aln_pair_result, score); FIELD(aln_pair_result, end_y); FIELD(aln_pair_result, end_x);
    FIELD(aln_pair_result, start_y); FIELD(aln_pair_result, start_x); FIELD(aln_pair_result, aln_len); FIELD(aln_pair_result, status);
    FIELD(aln_pair_result, passes); FIELD(aln_pair_result, flags);
    LAYOUT_END();
    LAYOUT_BEGIN(aln_scan_geometry);
    FIELD(aln_scan_geometry, first); FIELD(aln_scan_geometry, step); FIELD(aln_scan_geometry, width); FIELD(aln_scan_geometry, reverse);
    FIELD(aln_scan_geometry, reserved);
    LAYOUT_END();
    LAYOUT_BEGIN(aln_shuffle_spec);
    FIELD(aln_shuffle_spec, seed); FIELD(aln_shuffle_spec, pair_base); FIELD(aln_shuffle_spec, per_pair); FIELD(aln_shuffle_spec, max_trim);
    LAYOUT_END();
    LAYOUT_BEGIN(aln_seqset_block);
    FIELD(aln_seqset_block, q_first); FIELD(aln_seqset_block, q_count); FIELD(aln_seqset_block, t_first); FIELD(aln_seqset_block, t_count);
    FIELD(aln_seqset_block, upper); FIELD(aln_seqset_block, reserved);
    LAYOUT_END();
    LAYOUT_BEGIN(aln_signif_record);
    FIELD(aln_signif_record, sum); FIELD(aln_signif_record, sum_sq); FIELD(aln_signif_record, f_max); FIELD(aln_signif_record, n_ok);
    FIELD(aln_signif_record, n_ge); FIELD(aln_signif_record, status); FIELD(aln_signif_record, first_bad); FIELD(aln_signif_record, reserved);
    LAYOUT_END();
    LAYOUT_BEGIN(aln_hit_report);
    FIELD(aln_hit_report, columns); FIELD(aln_hit_report, identical); FIELD(aln_hit_report, positive); FIELD(aln_hit_report, mismatch);
    FIELD(aln_hit_report, q_gap); FIELD(aln_hit_report, t_gap); FIELD(aln_hit_report, q_gap_open); FIELD(aln_hit_report, t_gap_open);
    FIELD(aln_hit_report, status); FIELD(aln_hit_report, reserved);
    LAYOUT_END();
    LAYOUT_BEGIN(aln_hit_filter);
    FIELD(aln_hit_filter, min_identity); FIELD(aln_hit_filter, min_q_cover); FIELD(aln_hit_filter, min_t_cover);
    FIELD(aln_hit_filter, min_columns); FIELD(aln_hit_filter, reserved);
    LAYOUT_END();
}

/* ---------------------------------------------------------------- buffers of exactly the documented size, each with a guard zone */
#define GUARD 64
#define GUARD_BYTE 0xA5
#define SENTINEL 0xCD
#define MAX_BUFS 1024
static struct { const char *label; uint8_t *p; size_t n; } g_bufs[MAX_BUFS];
static int g_nbufs, g_bad;

static void *galloc(const char *label, size_t n, int fill)
{
    uint8_t *p = (uint8_t *)malloc(n + GUARD);
    if (!p || g_nbufs == MAX_BUFS) { printf("fatal out of memory or buffer slots at %s\n", label); exit(2); }
    memset(p, fill, n);
    memset(p + n, GUARD_BYTE, GUARD);
    g_bufs[g_nbufs].label = label; g_bufs[g_nbufs].p = p; g_bufs[g_nbufs].n = n;
    ++g_nbufs;
    return p;
}

static int holds(const void *p, size_t n, int byte)
{
    size_t i;
    for (i = 0; i < n; ++i) if (((const uint8_t *)p)[i] != (uint8_t)byte) return 0;
    return 1;
}

static void check_guards_and_free(void)
{
    int i, damaged = 0;
    for (i = 0; i < g_nbufs; ++i) {
        if (!holds(g_bufs[i].p + g_bufs[i].n, GUARD, GUARD_BYTE)) { printf("guard_damaged %s %lu\n", g_bufs[i].label, (unsigned long)g_bufs[i].n); ++damaged; }
        free(g_bufs[i].p);
    }
    printf("guards %d damaged %d\n", g_nbufs, damaged);
    g_bad += damaged;
    g_nbufs = 0;
}

/* ---------------------------------------------------------------- the case file */
static FILE *g_fp;

static size_t rd_head(const char *key)
{
    char got[64];
    unsigned long n;
    if (fscanf(g_fp, "%63s %lu", got, &n) != 2 || strcmp(got, key) != 0) { printf("fatal case file: wanted %s\n", key); exit(2); }
    return (size_t)n;
}

static uint64_t *rd_u64s(const char *key, size_t *n)
{
    size_t i;
    uint64_t *v;
    *n = rd_head(key);
    v = (uint64_t *)galloc(key, 8 * *n, 0);
    for (i = 0; i < *n; ++i) if (fscanf(g_fp, "%" SCNu64, &v[i]) != 1) { printf("fatal case file: %s\n", key); exit(2); }
    return v;
}

static uint32_t *rd_u32s(const char *key, size_t *n)
{
    size_t i;
    uint32_t *v;
    *n = rd_head(key);
    v = (uint32_t *)galloc(key, 4 * *n, 0);
    for (i = 0; i < *n; ++i) if (fscanf(g_fp, "%" SCNu32, &v[i]) != 1) { printf("fatal case file: %s\n", key); exit(2); }
    return v;
}

static uint8_t *rd_u8s(const char *key, size_t *n)
{
    size_t i;
    uint8_t *v;
    *n = rd_head(key);
    v = (uint8_t *)galloc(key, *n, 0);
    for (i = 0; i < *n; ++i) { unsigned c; if (fscanf(g_fp, "%u", &c) != 1) { printf("fatal case file: %s\n", key); exit(2); } v[i] = (uint8_t)c; }
    return v;
}

static double *rd_f64s(const char *key, size_t *n)
{
    size_t i;
    double *v;
    *n = rd_head(key);
    v = (double *)galloc(key, 8 * *n, 0);
    for (i = 0; i < *n; ++i) {
        uint64_t bits;
        if (fscanf(g_fp, "%" SCNx64, &bits) != 1) { printf("fatal case file: %s\n", key); exit(2); }
        memcpy(&v[i], &bits, 8);
    }
    return v;
}

/* ---------------------------------------------------------------- the printout */
static void pf(double x)
{
    uint64_t bits;
    memcpy(&bits, &x, 8);
    printf(" %016" PRIx64 "/%.17g", bits, x);
}

static void p_f64(const char *key, const double *v, size_t n) { size_t i; printf("%s", key); for (i = 0; i < n; ++i) pf(v[i]); printf("\n"); }
static void p_u64(const char *key, const uint64_t *v, size_t n) { size_t i; printf("%s", key); for (i = 0; i < n; ++i) printf(" %" PRIu64, v[i]); printf("\n"); }
static void p_u32(const char *key, const uint32_t *v, size_t n) { size_t i; printf("%s", key); for (i = 0; i < n; ++i) printf(" %" PRIu32, v[i]); printf("\n"); }
static void p_i32(const char *key, const int32_t *v, size_t n) { size_t i; printf("%s", key); for (i = 0; i < n; ++i) printf(" %" PRId32, v[i]); printf("\n"); }
static void p_u8(const char *key, const uint8_t *v, size_t n) { size_t i; printf("%s", key); for (i = 0; i < n; ++i) printf(" %u", (unsigned)v[i]); printf("\n"); }

/* `<key> <k> status f score end_y end_x start_y start_x aln_len passes flags`, one line per summary */
static void p_results(const char *key, const aln_pair_result *r, size_t n)
{
    size_t k;
    for (k = 0; k < n; ++k) {
        printf("%s %lu %d", key, (unsigned long)k, (int)r[k].status);
        pf(r[k].f); pf(r[k].score);
        printf(" %u %u %u %u %u %u %u\n", (unsigned)r[k].end_y, (unsigned)r[k].end_x, (unsigned)r[k].start_y, (unsigned)r[k].start_x,
               (unsigned)r[k].aln_len, (unsigned)r[k].passes, (unsigned)r[k].flags);
    }
}

/* the strings of entries in the layout of aln_align_batch: query at tb_off[k], target cap[k] = q_len + t_len + 2 bytes later */
static void p_strings(const char *key, const aln_pair_result *r, size_t n, const uint8_t *tb, const uint64_t *tb_off, const uint64_t *cap)
{
    size_t k;
    char name[96];
    for (k = 0; k < n; ++k) {
        const uint32_t len = r[k].status == ALN_OK ? r[k].aln_len : 0;
        sprintf(name, "%s_q %lu", key, (unsigned long)k); p_u8(name, tb + tb_off[k], len);
        sprintf(name, "%s_t %lu", key, (unsigned long)k); p_u8(name, tb + tb_off[k] + cap[k], len);
    }
}

static void p_reports(const char *key, const aln_hit_report *r, size_t n)
{
    size_t k;
    for (k = 0; k < n; ++k)
        printf("%s %lu %u %u %u %u %u %u %u %u %d %u\n", key, (unsigned long)k, (unsigned)r[k].columns, (unsigned)r[k].identical,
               (unsigned)r[k].positive, (unsigned)r[k].mismatch, (unsigned)r[k].q_gap, (unsigned)r[k].t_gap, (unsigned)r[k].q_gap_open,
               (unsigned)r[k].t_gap_open, (int)r[k].status, (unsigned)r[k].reserved);
}

static int chk(const char *label, int got, int want)
{
    printf("rc %s %d %d\n", label, got, want);
    if (got != want) {
        const char *e = aln_last_error();
        printf("unexpected %s: %s\n", label, e ? e : "");
        ++g_bad;
    }
    return got;
}

static void ms_and_bytes(const char *key, int st, const double *ms, const uint64_t *bytes)
{
    int i, ok = st == ALN_OK;
    for (i = 0; i < 4; ++i) if (!(ms[i] >= 0.0)) ok = 0;
    printf("%s nonnegative %d bytes %" PRIu64 " %" PRIu64 "\n", key, ok, bytes[0], bytes[1]);
}

/* ---------------------------------------------------------------- the sequence set every family draws its residues from */
static uint8_t *g_codes;
static uint64_t *g_off, *g_len;
static size_t g_nseq;

/* the tables of aln_align_batch for pairs named as (query sequence, target sequence) numbers */
static void pair_tables(const char *label, const uint64_t *qt, size_t n, uint64_t **q_off, uint64_t **q_len, uint64_t **t_off, uint64_t **t_len)
{
    size_t i;
    *q_off = (uint64_t *)galloc(label, 8 * n, 0); *q_len = (uint64_t *)galloc(label, 8 * n, 0);
    *t_off = (uint64_t *)galloc(label, 8 * n, 0); *t_len = (uint64_t *)galloc(label, 8 * n, 0);
    for (i = 0; i < n; ++i) {
        (*q_off)[i] = g_off[qt[2 * i]]; (*q_len)[i] = g_len[qt[2 * i]];
        (*t_off)[i] = g_off[qt[2 * i + 1]]; (*t_len)[i] = g_len[qt[2 * i + 1]];
    }
}

/* the cumulative string layout tb_off[k + 1] = tb_off[k] + 2 * (q_len + t_len + 2); returns the total */
static uint64_t string_layout(const char *label, const uint64_t *q_len, const uint64_t *t_len, size_t n, uint64_t **tb_off, uint64_t **cap)
{
    size_t k;
    uint64_t total = 0;
    *tb_off = (uint64_t *)galloc(label, 8 * n, 0); *cap = (uint64_t *)galloc(label, 8 * n, 0);
    for (k = 0; k < n; ++k) { (*cap)[k] = q_len[k] + t_len[k] + 2; (*tb_off)[k] = total; total += 2 * (*cap)[k]; }
    return total;
}

static aln_params make_params(int semantics, double del, double ext, const double *matrix, uint32_t rows, uint32_t cols)
{
    aln_params p;
    memset(&p, 0, sizeof p);
    p.semantics = semantics; p.del = del; p.ext = ext; p.matrix = matrix; p.rows = rows; p.cols = cols; p.row_stride = cols; p.blank_code = 98;
    return p;
}

/* ---------------------------------------------------------------- one scan pass set: windows, score, select, hits and the held fetches */
static void scan_family(aln_scan *scan, const char *tag, const double *pwm, uint32_t cols, double del, double ext, const uint64_t *geom, uint32_t reverse,
                        const double *msz, size_t cap, size_t seq_len)
{
    char key[96];
    aln_params p = make_params(ALN_PWM_LOCAL, del, ext, pwm, 4, cols);
    aln_scan_geometry g;
    size_t n, k;
    uint64_t count = 0, held = 0, stride;
    double ms[4] = {0, 0, 0, 0};
    uint64_t bytes[2] = {0, 0};
    int st;
    memset(&g, 0, sizeof g);
    g.first = geom[0]; g.step = geom[1]; g.width = geom[2]; g.reverse = reverse;
    n = aln_scan_windows(scan, &g);
    stride = aln_scan_string_stride(scan, cols, &g);
    printf("scan.%s.windows %lu stride %" PRIu64 "\n", tag, (unsigned long)n, stride);
    {   /* score: 8 bytes per window */
        double *f = (double *)galloc("scan f", 8 * n, 0);
        sprintf(key, "scan.%s.score", tag); chk(key, aln_scan_score(scan, &p, &g, f), ALN_OK);
        sprintf(key, "scan.%s.f", tag); p_f64(key, f, n);
    }
    {   /* select: cap entries of 4, 48 and stride bytes */
        uint32_t *idx = (uint32_t *)galloc("select indices", 4 * cap, 0);
        aln_pair_result *res = (aln_pair_result *)galloc("select results", sizeof(aln_pair_result) * cap, 0);
        uint8_t *tb = (uint8_t *)galloc("select strings", (size_t)stride * cap, 0);
        sprintf(key, "scan.%s.select", tag); st = chk(key, aln_scan_select(scan, &p, &g, msz[0], msz[1], msz[2], cap, &count, idx, res, tb), ALN_OK);
        printf("scan.%s.select_count %" PRIu64 "\n", tag, count);
        if (st == ALN_OK && count <= cap) {
            sprintf(key, "scan.%s.select_idx", tag); p_u32(key, idx, (size_t)count);
            sprintf(key, "scan.%s.select_res", tag); p_results(key, res, (size_t)count);
            for (k = 0; k < count; ++k) {      /* u32 column numbers, then the residues at 4 * (cols + that window's length + 2) */
                const uint64_t start = g.first + (uint64_t)idx[k] * g.step;
                const uint64_t wlen = start + g.width <= seq_len ? g.width : seq_len - start;
                uint32_t numbered[4096];
                const uint32_t len = res[k].aln_len < 4096 ? res[k].aln_len : 4096;
                memcpy(numbered, tb + k * stride, 4 * (size_t)len);
                sprintf(key, "scan.%s.select_num %lu", tag, (unsigned long)k); p_u32(key, numbered, len);
                sprintf(key, "scan.%s.select_seq %lu", tag, (unsigned long)k); p_u8(key, tb + k * stride + 4 * (cols + wlen + 2), len);
            }
        }
        sprintf(key, "scan.%s.select_stats", tag);
        st = aln_scan_stats(scan, ms, bytes); chk(key, st, ALN_OK); ms_and_bytes(key, st, ms, bytes);
    }
    {   /* hits: only the count comes back; then the held fetches */
        sprintf(key, "scan.%s.hits", tag); st = chk(key, aln_scan_hits(scan, &p, &g, msz[0], msz[1], msz[2], &held), ALN_OK);
        printf("scan.%s.held_count %" PRIu64 "\n", tag, held);
        if (st == ALN_OK) {
            const size_t h = (size_t)held, nk = h + 1;      /* keep: the held list backwards, and position 0 a second time */
            uint32_t *idx = (uint32_t *)galloc("held indices", 4 * h, 0);
            double *f = (double *)galloc("held f", 8 * h, 0);
            uint32_t *keep = (uint32_t *)galloc("held keep", 4 * nk, 0);
            double *counts = (double *)galloc("held counts", 8 * 4 * (size_t)cols, 0);
            aln_pair_result *res = (aln_pair_result *)galloc("held results", sizeof(aln_pair_result) * nk, 0);
            uint8_t *tb = (uint8_t *)galloc("held strings", (size_t)stride * nk, 0);
            sprintf(key, "scan.%s.held_list", tag); chk(key, aln_scan_held_list(scan, 0, held, idx, f), ALN_OK);
            sprintf(key, "scan.%s.held_idx", tag); p_u32(key, idx, h);
            sprintf(key, "scan.%s.held_f", tag); p_f64(key, f, h);
            for (k = 0; k < h; ++k) keep[k] = (uint32_t)(h - 1 - k);
            keep[h] = 0;
            if (h == 0) { printf("scan.%s.no_held_hits\n", tag); return; }
            sprintf(key, "scan.%s.held_frequencies", tag); chk(key, aln_scan_held_frequencies(scan, keep, nk, counts), ALN_OK);
            sprintf(key, "scan.%s.held_counts", tag); p_f64(key, counts, 4 * (size_t)cols);
            sprintf(key, "scan.%s.held_strings", tag); chk(key, aln_scan_held_strings(scan, keep, nk, res, tb), ALN_OK);
            sprintf(key, "scan.%s.held_res", tag); p_results(key, res, nk);
            for (k = 0; k < nk; ++k) {
                const uint64_t start = g.first + (uint64_t)idx[keep[k]] * g.step;
                const uint64_t wlen = start + g.width <= seq_len ? g.width : seq_len - start;
                uint32_t numbered[4096];
                const uint32_t len = res[k].aln_len < 4096 ? res[k].aln_len : 4096;
                memcpy(numbered, tb + k * stride, 4 * (size_t)len);
                sprintf(key, "scan.%s.held_num %lu", tag, (unsigned long)k); p_u32(key, numbered, len);
                sprintf(key, "scan.%s.held_seq %lu", tag, (unsigned long)k); p_u8(key, tb + k * stride + 4 * (cols + wlen + 2), len);
            }
            sprintf(key, "scan.%s.held_stats", tag);
            st = aln_scan_stats(scan, ms, bytes); chk(key, st, ALN_OK); ms_and_bytes(key, st, ms, bytes);
        }
    }
}

int main(int argc, char **argv)
{
    size_t n, i, k;
    int st = 0;
    aln_ctx *ctx;
    double *b62, *real, *gaps;
    uint32_t *refusals;
    aln_params local, global, realp;

    printf("abi_version_header %d\n", ALN_ABI_VERSION);
    if (argc < 2) {
        print_layouts();
        printf("abi_version_library %d\n", aln_abi_version());
        return aln_abi_version() == ALN_ABI_VERSION ? 0 : 1;
    }
    printf("abi_version_library %d\n", aln_abi_version());
    g_fp = fopen(argv[1], "r");
    if (!g_fp) { perror(argv[1]); return 2; }
    setvbuf(stdout, NULL, _IOFBF, 1 << 16);

    b62 = rd_f64s("matrix_b62", &n);        /* 24 x 24 */
    real = rd_f64s("matrix_real", &n);      /* 24 x 24, not a multiple of 2^-k: the f64 kernels */
    gaps = rd_f64s("gaps", &n);             /* local del ext, global del ext, real del ext */
    refusals = rd_u32s("refusals", &n);     /* scan semantics, best on upper, strings before a run, select capacity */
    g_len = rd_u64s("set_len", &g_nseq);
    g_codes = rd_u8s("set_codes", &n);
    g_off = (uint64_t *)galloc("set_off", 8 * g_nseq, 0);
    for (i = 1; i < g_nseq; ++i) g_off[i] = g_off[i - 1] + g_len[i - 1];
    local = make_params(ALN_CORE_LOCAL, gaps[0], gaps[1], b62, 24, 24);
    global = make_params(ALN_CORE_GLOBAL, gaps[2], gaps[3], b62, 24, 24);
    realp = make_params(ALN_CORE_LOCAL, gaps[4], gaps[5], real, 24, 24);

    /* ================================================================ context */
    ctx = aln_create(0, &st);
    if (!ctx) { printf("fatal aln_create: %d %s\n", st, aln_last_error()); return 3; }
    {
        int cus = 0;
        size_t hbm = 0;
        char name[128];
        int ids[1] = {0};
        aln_ctx *second;
        memset(name, 0, sizeof name);
        chk("device_info", aln_device_info(ctx, &cus, &hbm, name, sizeof name), ALN_OK);
        printf("device compute_units %d hbm_bytes %lu name %s\n", cus, (unsigned long)hbm, name);
        second = aln_create_multi(1, ids, &st);
        chk("create_multi", second ? ALN_OK : st ? st : -1, ALN_OK);
        printf("devices %d second %d\n", aln_device_count(ctx), second ? aln_device_count(second) : -1);
        if (second) aln_destroy(second);
    }

    /* ================================================================ staged batch (and the host-only chunk plan of its pairs) */
    {
        size_t n2, np;
        uint64_t *qt = rd_u64s("batch_pairs", &n2), *q_off, *q_len, *t_off, *t_len, *tb_off, *cap, total;
        uint64_t *first, *count;
        aln_batch *b;
        aln_params p = local;
        np = n2 / 2;
        pair_tables("batch tables", qt, np, &q_off, &q_len, &t_off, &t_len);
        first = (uint64_t *)galloc("plan first", 8 * np, 0); count = (uint64_t *)galloc("plan count", 8 * np, 0);
        k = aln_plan_chunks(&p, q_len, t_len, np, 1, first, count, np);
        printf("plan.chunks %lu\n", (unsigned long)k);
        p_u64("plan.first", first, k < np ? k : np); p_u64("plan.count", count, k < np ? k : np);
        p.outputs = ALN_OUT_SCORE | ALN_OUT_TRACEBACK;
        b = aln_batch_create(ctx, &p, g_codes, q_off, q_len, t_off, t_len, np, &st);
        chk("batch.create", b ? ALN_OK : st ? st : -1, ALN_OK);
        if (b) {
            double fill_ms = -1.0, tb_ms = -1.0;
            uint32_t launches = 0;
            aln_pair_result *res = (aln_pair_result *)galloc("batch results", sizeof(aln_pair_result) * np, 0);
            uint8_t *tb;
            total = string_layout("batch layout", q_len, t_len, np, &tb_off, &cap);
            tb = (uint8_t *)galloc("batch strings", (size_t)total, 0);
            aln_batch_enable_timing(b, 1);
            chk("batch.run", aln_batch_run(b, NULL), ALN_OK);
            chk("batch.sync", aln_batch_sync(b), ALN_OK);
            st = chk("batch.timing", aln_batch_timing(b, &fill_ms, &tb_ms, &launches), ALN_OK);
            printf("batch.timing_values nonnegative %d launches %u\n", st == ALN_OK && fill_ms >= 0.0 && tb_ms >= 0.0, (unsigned)launches);
            chk("batch.fetch", aln_batch_fetch(b, res, tb, tb_off), ALN_OK);
            p_results("batch.res", res, np);
            p_strings("batch.str", res, np, tb, tb_off, cap);
            printf("batch.cells %" PRIu64 " size %lu direction_bytes %" PRIu64 " results_device %d\n", aln_batch_cells(b), (unsigned long)aln_batch_size(b),
                   aln_batch_direction_bytes(b), aln_batch_results_device(b) != NULL);
            aln_batch_destroy(b);
        }
    }

    /* ================================================================ window scan, forward and reverse, integer and real-valued PWM */
    {
        size_t seq_len, ncap;
        uint8_t *seq = rd_u8s("scan_seq", &seq_len);
        uint64_t *geom = rd_u64s("scan_geom", &n);            /* first step width */
        double *pwm_int = rd_f64s("scan_pwm_int", &n);
        const uint32_t cols = (uint32_t)(n / 4);
        double *pwm_real = rd_f64s("scan_pwm_real", &n);
        double *sgaps = rd_f64s("scan_gaps", &n);
        double *msz = rd_f64s("scan_select", &n);             /* mean sd z_min of int.fwd, int.rev, real.fwd, real.rev */
        uint64_t *scap = rd_u64s("scan_cap", &ncap);
        aln_scan *scan = aln_scan_create(ctx, seq, seq_len, &st);
        chk("scan.create", scan ? ALN_OK : st ? st : -1, ALN_OK);
        if (scan) {
            scan_family(scan, "int.fwd", pwm_int, cols, sgaps[0], sgaps[1], geom, 0, msz + 0, (size_t)scap[0], seq_len);
            scan_family(scan, "int.rev", pwm_int, cols, sgaps[0], sgaps[1], geom, 1, msz + 3, (size_t)scap[0], seq_len);
            scan_family(scan, "real.fwd", pwm_real, cols, sgaps[0], sgaps[1], geom, 0, msz + 6, (size_t)scap[0], seq_len);
            scan_family(scan, "real.rev", pwm_real, cols, sgaps[0], sgaps[1], geom, 1, msz + 9, (size_t)scap[0], seq_len);
            {   /* planted refusal: "ALN_PWM_LOCAL only; anything else is ALN_ERR_UNSUPPORTED" */
                aln_scan_geometry g;
                aln_params p = make_params(ALN_CORE_LOCAL, sgaps[0], sgaps[1], pwm_int, 4, cols);
                size_t nw;
                double *f;
                memset(&g, 0, sizeof g);
                g.first = geom[0]; g.step = geom[1]; g.width = geom[2];
                nw = aln_scan_windows(scan, &g);
                f = (double *)galloc("refused scan f", 8 * nw, SENTINEL);
                chk("refusal.scan_semantics", aln_scan_score(scan, &p, &g, f), (int)refusals[0]);
                printf("refusal.scan_semantics.sentinel %d\n", holds(f, 8 * nw, SENTINEL));
            }
            {   /* planted refusal: select with a capacity below the true count: ALN_ERR_CAPACITY, *count the true one; with cap = 0
                 * min(count, cap) = 0 entries are written */
                aln_scan_geometry g;
                aln_params p = make_params(ALN_PWM_LOCAL, sgaps[0], sgaps[1], pwm_int, 4, cols);
                uint64_t count = 0;
                uint32_t *idx = (uint32_t *)galloc("refused select indices", 4, SENTINEL);
                aln_pair_result *res = (aln_pair_result *)galloc("refused select results", sizeof(aln_pair_result), SENTINEL);
                uint8_t *tb = (uint8_t *)galloc("refused select strings", 64, SENTINEL);
                memset(&g, 0, sizeof g);
                g.first = geom[0]; g.step = geom[1]; g.width = geom[2];
                chk("refusal.select_capacity", aln_scan_select(scan, &p, &g, msz[0], msz[1], msz[2], 0, &count, idx, res, tb), (int)refusals[3]);
                printf("refusal.select_capacity.count %" PRIu64 " sentinel %d\n", count,
                       holds(idx, 4, SENTINEL) && holds(res, sizeof(aln_pair_result), SENTINEL) && holds(tb, 64, SENTINEL));
            }
            aln_scan_destroy(scan);
        }
    }

    /* ================================================================ shuffled copies */
    {
        size_t n2, np, ns;
        uint64_t *qt = rd_u64s("shuffle_pairs", &n2), *q_off, *q_len, *t_off, *t_len, *out_off, total = 0;
        uint64_t *sv = rd_u64s("shuffle_spec", &ns);          /* seed pair_base per_pair max_trim */
        aln_shuffle_spec spec;
        uint8_t *out;
        double *f;
        uint32_t *lengths;
        int32_t *status;
        np = n2 / 2;
        pair_tables("shuffle tables", qt, np, &q_off, &q_len, &t_off, &t_len);
        spec.seed = sv[0]; spec.pair_base = sv[1]; spec.per_pair = (uint32_t)sv[2]; spec.max_trim = (uint32_t)sv[3];
        out_off = (uint64_t *)galloc("shuffle out_off", 8 * np, 0);
        for (i = 0; i < np; ++i) { out_off[i] = total; total += t_len[i] * spec.per_pair; }     /* copy s of pair i at out_off[i] + s * t_len[i] */
        out = (uint8_t *)galloc("shuffle out", (size_t)total, 0xEE);
        chk("shuffle.targets", aln_shuffle_targets(ctx, &spec, g_codes, t_off, t_len, np, out, out_off), ALN_OK);
        for (i = 0; i < np; ++i) {
            char key[64];
            sprintf(key, "shuffle.copies %lu %" PRIu64, (unsigned long)i, t_len[i]);
            p_u8(key, out + out_off[i], (size_t)(t_len[i] * spec.per_pair));
        }
        f = (double *)galloc("shuffle f", 8 * np * spec.per_pair, 0);
        lengths = (uint32_t *)galloc("shuffle lengths", 4 * np * spec.per_pair, 0);
        status = (int32_t *)galloc("shuffle status", 4 * np, 0);
        chk("shuffle.scores", aln_shuffle_scores(ctx, &local, &spec, g_codes, q_off, q_len, t_off, t_len, np, f, lengths, status), ALN_OK);
        p_f64("shuffle.f", f, np * spec.per_pair);
        p_u32("shuffle.lengths", lengths, np * spec.per_pair);
        p_i32("shuffle.status", status, np);
    }

    /* ================================================================ matrix transforms, host and device, the same inputs */
    {
        size_t nm, nt;
        uint64_t *tn = rd_u64s("transform_n", &nt);
        double *min = rd_f64s("transform_matrices", &nm), *fr = rd_f64s("transform_freq", &n), *kd = rd_f64s("transform_kd", &n),
               *r2 = rd_f64s("transform_r2", &n);
        double *host = (double *)galloc("transform host out", 8 * nm, SENTINEL), *dev = (double *)galloc("transform device out", 8 * nm, SENTINEL);
        int32_t *hs = (int32_t *)galloc("transform host status", 4 * (size_t)tn[0], 0), *ds = (int32_t *)galloc("transform device status", 4 * (size_t)tn[0], 0);
        chk("transform.host", aln_transform_matrices((size_t)tn[0], 24, 24, min, fr, kd, r2, host, hs), ALN_OK);
        chk("transform.device", aln_transform_matrices_device(ctx, (size_t)tn[0], 24, 24, min, fr, kd, r2, dev, ds), ALN_OK);
        p_i32("transform.host_status", hs, (size_t)tn[0]); p_i32("transform.device_status", ds, (size_t)tn[0]);
        for (i = 0; i < tn[0]; ++i) {        /* a matrix without a root is left as it was: here, the sentinel */
            char key[64];
            sprintf(key, "transform.host_out %lu %d", (unsigned long)i, holds(host + 576 * i, 8 * 576, SENTINEL)); p_f64(key, host + 576 * i, 576);
            sprintf(key, "transform.device_out %lu %d", (unsigned long)i, holds(dev + 576 * i, 8 * 576, SENTINEL)); p_f64(key, dev + 576 * i, 576);
        }
    }

    /* ================================================================ pair set: per-pair matrices, then the stored ones */
    {
        size_t n2, np, na, nw, nr;
        uint64_t *qt = rd_u64s("pairset_pairs", &n2), *q_off, *q_len, *t_off, *t_len;
        uint32_t *active = rd_u32s("pairset_active", &na);
        double *mats = rd_f64s("pairset_matrices", &n);        /* n_active compact 24 x 24 matrices, entry k scores pair active[k] */
        uint32_t *which = rd_u32s("pairset_which", &nw);
        double *fr = rd_f64s("pairset_freq", &n), *kd = rd_f64s("pairset_kd", &n), *r2 = rd_f64s("pairset_r2", &n);
        uint32_t *reest = rd_u32s("pairset_reestimate", &nr);   /* the pairs re-estimated from their held strings */
        aln_pairset *ps;
        aln_params p = realp;
        double ms[4] = {0, 0, 0, 0};
        uint64_t bytes[2] = {0, 0};
        np = n2 / 2;
        p.matrix = NULL;                                       /* "params->matrix must be NULL" */
        pair_tables("pairset tables", qt, np, &q_off, &q_len, &t_off, &t_len);
        ps = aln_pairset_create(ctx, g_codes, q_off, q_len, t_off, t_len, np, &st);
        chk("pairset.create", ps ? ALN_OK : st ? st : -1, ALN_OK);
        if (ps) {
            uint64_t *wq = (uint64_t *)galloc("pairset which q_len", 8 * nw, 0), *wt = (uint64_t *)galloc("pairset which t_len", 8 * nw, 0);
            uint64_t *tb_off, *cap, total;
            aln_pair_result *res = (aln_pair_result *)galloc("pairset run results", sizeof(aln_pair_result) * na, 0);
            aln_pair_result *sres = (aln_pair_result *)galloc("pairset string results", sizeof(aln_pair_result) * nw, SENTINEL);
            uint32_t *counts = (uint32_t *)galloc("pairset counts", 4 * 576 * nw, 0);
            uint8_t *tb;
            int32_t *status = (int32_t *)galloc("pairset reestimate status", 4 * nw, 0), *status2 = (int32_t *)galloc("pairset reestimate status", 4 * nr, 0);
            double *store = (double *)galloc("pairset store", 8 * 576 * nw, 0);
            for (k = 0; k < nw; ++k) { wq[k] = q_len[which[k]]; wt[k] = t_len[which[k]]; }
            total = string_layout("pairset layout", wq, wt, nw, &tb_off, &cap);
            tb = (uint8_t *)galloc("pairset strings", (size_t)total, SENTINEL);
            /* planted refusal: "a fetch without a run: ALN_ERR_INVALID_ARGUMENT, nothing written" */
            chk("refusal.strings_before_run", aln_pairset_strings(ps, which, nw, sres, tb, tb_off), (int)refusals[2]);
            printf("refusal.strings_before_run.sentinel %d\n", holds(sres, sizeof(aln_pair_result) * nw, SENTINEL) && holds(tb, (size_t)total, SENTINEL));
            chk("pairset.run", aln_pairset_run(ps, &p, mats, active, na, res), ALN_OK);
            p_results("pairset.run_res", res, na);
            chk("pairset.frequencies", aln_pairset_frequencies(ps, which, nw, counts), ALN_OK);
            for (k = 0; k < nw; ++k) { char key[64]; sprintf(key, "pairset.counts %lu", (unsigned long)k); p_u32(key, counts + 576 * k, 576); }
            chk("pairset.strings", aln_pairset_strings(ps, which, nw, sres, tb, tb_off), ALN_OK);
            p_results("pairset.str_res", sres, nw);
            p_strings("pairset.str", sres, nw, tb, tb_off, cap);
            st = chk("pairset.stats", aln_pairset_stats(ps, ms, bytes), ALN_OK); ms_and_bytes("pairset.stats", st, ms, bytes);
            chk("pairset.heuristics", aln_pairset_heuristics(ps, 24, 24, fr, kd, r2), ALN_OK);
            chk("pairset.reestimate_shared", aln_pairset_reestimate(ps, real, which, nw, status), ALN_OK);
            p_i32("pairset.reestimate_shared_status", status, nw);
            chk("pairset.reestimate_held", aln_pairset_reestimate(ps, NULL, reest, nr, status2), ALN_OK);
            p_i32("pairset.reestimate_held_status", status2, nr);
            chk("pairset.matrices", aln_pairset_matrices(ps, which, nw, store), ALN_OK);
            for (k = 0; k < nw; ++k) { char key[64]; sprintf(key, "pairset.store %lu", (unsigned long)k); p_f64(key, store + 576 * k, 576); }
            chk("pairset.run_stored", aln_pairset_run_stored(ps, &p, active, na, res), ALN_OK);
            p_results("pairset.stored_res", res, na);
            chk("pairset.stored_strings", aln_pairset_strings(ps, which, nw, sres, tb, tb_off), ALN_OK);
            p_results("pairset.stored_str_res", sres, nw);
            p_strings("pairset.stored_str", sres, nw, tb, tb_off, cap);
            aln_pairset_destroy(ps);
        }
    }

    /* ================================================================ sequence set */
    {
        size_t nr, nk, ns, nf, nb;
        uint64_t *rect = rd_u64s("set_rect", &nr);             /* q_first q_count t_first t_count: starts at neither 0 */
        double *fmin = rd_f64s("set_fmin", &n);
        double *flt = rd_f64s("set_filter", &nf);              /* min_identity min_q_cover min_t_cover */
        uint64_t *fcols = rd_u64s("set_filter_columns", &n);
        uint64_t *best = rd_u64s("best_k", &nb);
        double *best_fmin = rd_f64s("best_fmin", &n);
        uint32_t *skeep = rd_u32s("signif_keep", &nk);         /* positions of the best pass's held list */
        uint64_t *sv = rd_u64s("signif_spec", &ns);            /* seed pair_base per_pair max_trim */
        double *lfr = rd_f64s("loop_freq", &n), *lkd = rd_f64s("loop_kd", &n), *lr2 = rd_f64s("loop_r2", &n);
        aln_seqset *set = aln_seqset_create(ctx, g_codes, g_off, g_len, g_nseq, &st);
        aln_seqset_block up, re, bad;
        uint64_t np_up, np_re, count = 0;
        double ms[4] = {0, 0, 0, 0};
        uint64_t bytes[2] = {0, 0};
        chk("set.create", set ? ALN_OK : st ? st : -1, ALN_OK);
        if (!set) { check_guards_and_free(); return 4; }
        memset(&up, 0, sizeof up); memset(&re, 0, sizeof re);
        up.q_first = up.t_first = 0; up.q_count = up.t_count = g_nseq; up.upper = 1;
        re.q_first = rect[0]; re.q_count = rect[1]; re.t_first = rect[2]; re.t_count = rect[3];
        bad = up; bad.q_count = g_nseq + 1;
        np_up = aln_seqset_pairs(set, &up); np_re = aln_seqset_pairs(set, &re);
        printf("set.pairs upper %" PRIu64 " rectangle %" PRIu64 " invalid %" PRIu64 "\n", np_up, np_re, aln_seqset_pairs(set, &bad));
        {   /* score: the upper block under core local, the rectangle under core global */
            double *f = (double *)galloc("set f upper", 8 * (size_t)np_up, 0), *f2 = (double *)galloc("set f rect", 8 * (size_t)np_re, 0);
            int32_t *s1 = (int32_t *)galloc("set status upper", 4 * (size_t)np_up, 0), *s2 = (int32_t *)galloc("set status rect", 4 * (size_t)np_re, 0);
            chk("set.score_upper", aln_seqset_score(set, &local, &up, f, s1), ALN_OK);
            p_f64("set.upper_f", f, (size_t)np_up); p_i32("set.upper_status", s1, (size_t)np_up);
            chk("set.score_rect", aln_seqset_score(set, &global, &re, f2, s2), ALN_OK);
            p_f64("set.rect_f", f2, (size_t)np_re); p_i32("set.rect_status", s2, (size_t)np_re);
        }
        st = chk("set.hits", aln_seqset_hits(set, &local, &up, fmin[0], &count), ALN_OK);
        printf("set.hits_count %" PRIu64 "\n", count);
        if (st == ALN_OK && count) {
            const size_t h = (size_t)count;
            uint64_t *pi = (uint64_t *)galloc("hits pair_index", 8 * h, 0), *hq = (uint64_t *)galloc("hits q_len", 8 * h, 0),
                     *ht = (uint64_t *)galloc("hits t_len", 8 * h, 0), *tb_off, *cap, total, kept = 0;
            uint32_t *q = (uint32_t *)galloc("hits q", 4 * h, 0), *t = (uint32_t *)galloc("hits t", 4 * h, 0), *keep = (uint32_t *)galloc("hits keep", 4 * h, 0);
            uint32_t *pos = (uint32_t *)galloc("filter positions", 4 * h, 0);
            double *f = (double *)galloc("hits f", 8 * h, 0);
            aln_pair_result *res = (aln_pair_result *)galloc("hits results", sizeof(aln_pair_result) * h, 0);
            aln_hit_report *rep = (aln_hit_report *)galloc("hits reports", sizeof(aln_hit_report) * h, 0);
            aln_hit_report *frep = (aln_hit_report *)galloc("filter reports", sizeof(aln_hit_report) * h, 0);
            aln_hit_filter filter;
            uint8_t *tb;
            chk("set.held_list", aln_seqset_held_list(set, 0, count, pi, q, t, f), ALN_OK);
            p_u64("set.held_pair", pi, h); p_u32("set.held_q", q, h); p_u32("set.held_t", t, h); p_f64("set.held_f", f, h);
            for (k = 0; k < h; ++k) { keep[k] = (uint32_t)k; hq[k] = g_len[q[k] < g_nseq ? q[k] : 0]; ht[k] = g_len[t[k] < g_nseq ? t[k] : 0]; }
            total = string_layout("hits layout", hq, ht, h, &tb_off, &cap);
            tb = (uint8_t *)galloc("hits strings", (size_t)total, 0);
            chk("set.held_strings", aln_seqset_held_strings(set, keep, count, res, tb, tb_off), ALN_OK);
            p_results("set.held_res", res, h);
            p_strings("set.held_str", res, h, tb, tb_off, cap);
            chk("set.held_report", aln_seqset_held_report(set, &local, ALN_REPORT_SKIP_SEED, keep, count, rep), ALN_OK);
            p_reports("set.report", rep, h);
            memset(&filter, 0, sizeof filter);
            filter.min_identity = flt[0]; filter.min_q_cover = flt[1]; filter.min_t_cover = flt[2]; filter.min_columns = (uint32_t)fcols[0];
            chk("set.held_filter", aln_seqset_held_filter(set, &local, ALN_REPORT_SKIP_SEED, &filter, pos, frep, count, &kept), ALN_OK);
            printf("set.filter_count %" PRIu64 "\n", kept);
            p_u32("set.filter_positions", pos, (size_t)(kept < count ? kept : count));
            p_reports("set.filter_report", frep, (size_t)(kept < count ? kept : count));
        }
        {   /* planted refusal: "upper = 1: ALN_ERR_UNSUPPORTED"; a refused call leaves *count and the held state as they were */
            uint64_t *c = (uint64_t *)galloc("refused best count", 8, SENTINEL);
            chk("refusal.best_upper", aln_seqset_best(set, &local, &up, (uint32_t)best[0], best_fmin[0], ALN_BEST_SKIP_SELF, c), (int)refusals[1]);
            printf("refusal.best_upper.sentinel %d\n", holds(c, 8, SENTINEL));
        }
        {   /* the k best targets of every query of the whole grid, and the significance of some of them */
            aln_seqset_block all;
            memset(&all, 0, sizeof all);
            all.q_count = all.t_count = g_nseq;
            count = 0;
            st = chk("set.best", aln_seqset_best(set, &local, &all, (uint32_t)best[0], best_fmin[0], ALN_BEST_SKIP_SELF, &count), ALN_OK);
            printf("set.best_count %" PRIu64 "\n", count);
            if (st == ALN_OK && count) {
                const size_t h = (size_t)count;
                uint64_t *pi = (uint64_t *)galloc("best pair_index", 8 * h, 0);
                uint32_t *q = (uint32_t *)galloc("best q", 4 * h, 0), *t = (uint32_t *)galloc("best t", 4 * h, 0);
                double *f = (double *)galloc("best f", 8 * h, 0);
                aln_shuffle_spec spec;
                aln_signif_record *rec = (aln_signif_record *)galloc("signif records", sizeof(aln_signif_record) * nk, 0);
                double *sf;
                uint32_t *sl;
                chk("set.best_list", aln_seqset_held_list(set, 0, count, pi, q, t, f), ALN_OK);
                p_u64("set.best_pair", pi, h); p_u32("set.best_q", q, h); p_u32("set.best_t", t, h); p_f64("set.best_f", f, h);
                spec.seed = sv[0]; spec.pair_base = sv[1]; spec.per_pair = (uint32_t)sv[2]; spec.max_trim = (uint32_t)sv[3];
                sf = (double *)galloc("signif f", 8 * nk * spec.per_pair, 0);
                sl = (uint32_t *)galloc("signif lengths", 4 * nk * spec.per_pair, 0);
                chk("set.significance", aln_seqset_held_significance(set, &realp, &spec, skeep, nk, rec, sf, sl), ALN_OK);
                for (k = 0; k < nk; ++k) {
                    printf("set.signif %lu", (unsigned long)k);
                    pf(rec[k].sum); pf(rec[k].sum_sq); pf(rec[k].f_max);
                    printf(" %u %u %d %u %" PRIu64 "\n", (unsigned)rec[k].n_ok, (unsigned)rec[k].n_ge, (int)rec[k].status, (unsigned)rec[k].first_bad, rec[k].reserved);
                }
                p_f64("set.signif_f", sf, nk * spec.per_pair);
                p_u32("set.signif_lengths", sl, nk * spec.per_pair);
            }
        }
        st = chk("set.stats", aln_seqset_stats(set, ms, bytes), ALN_OK); ms_and_bytes("set.stats", st, ms, bytes);

        /* ============================================================ device loop on the pairs of the upper block */
        {
            aln_pairset *ps = aln_pairset_create_from_set(set, &up, 0, np_up, &st);
            aln_params p = local;
            p.matrix = NULL;
            chk("loop.create_from_set", ps ? ALN_OK : st ? st : -1, ALN_OK);
            if (ps) {
                const size_t np = (size_t)np_up;
                int32_t *status = (int32_t *)galloc("loop begin status", 4 * np, 0);
                size_t going = 0;
                unsigned step = 0;
                chk("loop.heuristics", aln_pairset_heuristics(ps, 24, 24, lfr, lkd, lr2), ALN_OK);
                st = chk("loop.begin", aln_pairset_loop_begin(ps, b62, status), ALN_OK);
                p_i32("loop.begin_status", status, np);
                for (i = 0; i < np; ++i) going += status[i] == 0;
                while (st == ALN_OK && going && step < 64) {      /* "the arrays must hold as many entries as pairs are going" */
                    char key[64];
                    uint32_t counts[4] = {0, 0, 0, 0};
                    uint32_t *fin = (uint32_t *)galloc("loop finished", 4 * going, 0), *cause = (uint32_t *)galloc("loop cause", 4 * going, 0);
                    aln_pair_result *res = (aln_pair_result *)galloc("loop results", sizeof(aln_pair_result) * going, 0);
                    size_t done;
                    ++step;
                    sprintf(key, "loop.step%u", step);
                    st = chk(key, aln_pairset_loop_step(ps, &p, fin, cause, res, counts), ALN_OK);
                    done = (size_t)counts[1] + counts[2];
                    if (done > going) done = going;
                    sprintf(key, "loop.step%u.counts", step); p_u32(key, counts, 4);
                    sprintf(key, "loop.step%u.finished", step); p_u32(key, fin, done);
                    sprintf(key, "loop.step%u.cause", step); p_u32(key, cause, done);
                    sprintf(key, "loop.step%u.res", step); p_results(key, res, done);
                    going = counts[3];
                }
                printf("loop.steps %u going %lu\n", step, (unsigned long)going);
                {   /* "with nothing going: counts all 0, ALN_OK" */
                    uint32_t counts[4] = {9, 9, 9, 9};
                    chk("loop.idle_step", aln_pairset_loop_step(ps, &p, NULL, NULL, NULL, counts), ALN_OK);
                    p_u32("loop.idle_counts", counts, 4);
                }
                aln_pairset_destroy(ps);
            }
        }
        aln_seqset_destroy(set);
    }
    aln_destroy(ctx);
    fclose(g_fp);
    check_guards_and_free();
    printf("done bad %d\n", g_bad);
    return g_bad ? 1 : 0;
}
