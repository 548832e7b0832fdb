/*
 * abi_cluster.c -- the clustering family of include/aligner_hip_cluster.h called from C99 by a caller who has read nothing but the
 * header.  Built with `gcc -std=c99 -Wall -Werror -Iinclude` (aligner_amd/build.py: build_cluster_harness); pins the layout of the
 * family's two records at compile time and allocates every buffer with exactly the size the header's comment gives, followed by a
 * guard zone that is checked at the end.
 *
 * usage: abi_cluster               no GPU: prints one `layout <type> <sizeof> <field> <offset> <size> ...` line per record (fields in
 *                                  declaration order; tests/test_cluster_rules_cpu.py compares them with the ctypes classes)
 *        abi_cluster <case file>   on a GPU: aln_cluster_edges on the case's edge list, then a held pass on the case's sequence set
 *                                  and aln_seqset_held_cluster without and with the filter; each in both modes
 *                                  (tests/test_cluster_gpu.py writes the case and compares the printout with the reference)
 *
 * case file: whitespace-separated tokens in the fixed order main() reads them; an integer is decimal, a double the 16 hex digits of
 * its 64 bits:  n_nodes  with_len  len[n_nodes] (if with_len)  n_edges  a b (per edge)  capacity
 *               n_seqs  len[n_seqs]  codes[sum of len]  rows cols  matrix[rows * cols]  del ext  f_min  blank  min_identity min_q_cover
 * output: `rc <label> <returned>` per call, then `label`, `records` (label size longest edges per cluster) and `summary` (nodes
 * clusters edges self_edges singletons rounds reserved) lines.  Exit status 0 iff every call returned ALN_OK and no guard was touched.
 */
#include <inttypes.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aligner_hip_cluster.h"

#define PIN(name, cond) typedef char pin_##name[(cond) ? 1 : -1]
PIN(record_size, sizeof(aln_cluster_record) == 16);
PIN(record_label, offsetof(aln_cluster_record, label) == 0);
PIN(record_size_at, offsetof(aln_cluster_record, size) == 4);
PIN(record_longest, offsetof(aln_cluster_record, longest) == 8);
PIN(record_edges, offsetof(aln_cluster_record, edges) == 12);
PIN(summary_size, sizeof(aln_cluster_summary) == 48);
PIN(summary_nodes, offsetof(aln_cluster_summary, nodes) == 0);
PIN(summary_clusters, offsetof(aln_cluster_summary, clusters) == 8);
PIN(summary_edges, offsetof(aln_cluster_summary, edges) == 16);
PIN(summary_self_edges, offsetof(aln_cluster_summary, self_edges) == 24);
PIN(summary_singletons, offsetof(aln_cluster_summary, singletons) == 32);
PIN(summary_rounds, offsetof(aln_cluster_summary, rounds) == 40);
PIN(summary_reserved, offsetof(aln_cluster_summary, reserved) == 44);
PIN(none, ALN_CLUSTER_NONE == 0xFFFFFFFFu);
PIN(modes, ALN_CLUSTER_COMPONENTS == 0u && ALN_CLUSTER_GREEDY == 1u);

#define FIELD(type, field) printf(" %s %u %u", #field, (unsigned)offsetof(type, field), (unsigned)sizeof(((type *)0)->field))

static void print_layouts(void)
{
    printf("layout aln_cluster_record %u", (unsigned)sizeof(aln_cluster_record));
    FIELD(aln_cluster_record, label); FIELD(aln_cluster_record, size); FIELD(aln_cluster_record, longest); FIELD(aln_cluster_record, edges);
    printf("\n");
    printf("layout aln_cluster_summary %u", (unsigned)sizeof(aln_cluster_summary));
    FIELD(aln_cluster_summary, nodes); FIELD(aln_cluster_summary, clusters); FIELD(aln_cluster_summary, edges);
    FIELD(aln_cluster_summary, self_edges); FIELD(aln_cluster_summary, singletons); FIELD(aln_cluster_summary, rounds);
    FIELD(aln_cluster_summary, reserved);
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
static void rc(const char *what, uint32_t mode, int got)
{
    printf("rc %s %u %d\n", what, (unsigned)mode, got);
    if (got != ALN_OK) { printf("error %s\n", aln_last_error()); g_fail = 1; }
}
static void print_result(const uint32_t *label, uint64_t n, const aln_cluster_record *rec, uint64_t capacity, const aln_cluster_summary *s)
{
    const uint64_t wrote = s->clusters < capacity ? s->clusters : capacity;
    printf("label");
    for (uint64_t i = 0; i < n; ++i) printf(" %u", (unsigned)label[i]);
    printf("\nrecords");
    for (uint64_t i = 0; i < wrote; ++i) printf(" %u %u %u %u", (unsigned)rec[i].label, (unsigned)rec[i].size, (unsigned)rec[i].longest, (unsigned)rec[i].edges);
    printf("\nsummary %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u\n", s->nodes, s->clusters, s->edges, s->self_edges, s->singletons,
           (unsigned)s->rounds, (unsigned)s->reserved);
}

int main(int argc, char **argv)
{
    if (argc < 2) { print_layouts(); return 0; }
    g_in = fopen(argv[1], "r");
    if (!g_in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int status = 0;
    aln_ctx *ctx = aln_create(0, &status);
    if (!ctx) { printf("rc create 0 %d\nerror %s\n", status, aln_last_error()); return 1; }

    /* ---- an edge list of the caller's */
    const uint64_t n = read_u64(), with_len = read_u64();
    uint32_t *len = with_len ? (uint32_t *)guarded(4 * n) : NULL;
    for (uint64_t i = 0; with_len && i < n; ++i) len[i] = (uint32_t)read_u64();
    const uint64_t m = read_u64();
    uint32_t *ea = (uint32_t *)guarded(4 * m), *eb = (uint32_t *)guarded(4 * m);
    for (uint64_t k = 0; k < m; ++k) { ea[k] = (uint32_t)read_u64(); eb[k] = (uint32_t)read_u64(); }
    const uint64_t capacity = read_u64();
    for (uint32_t mode = ALN_CLUSTER_COMPONENTS; mode <= ALN_CLUSTER_GREEDY; ++mode) {
        uint32_t *label = (uint32_t *)guarded(4 * n);
        aln_cluster_record *rec = (aln_cluster_record *)guarded(sizeof(aln_cluster_record) * capacity);
        aln_cluster_summary *sum = (aln_cluster_summary *)guarded(sizeof(aln_cluster_summary));
        rc("cluster_edges", mode, aln_cluster_edges(ctx, mode, n, len, ea, eb, m, label, rec, capacity, sum));
        print_result(label, n, rec, capacity, sum);
    }

    /* ---- the held hits of a sequence set */
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
    aln_hit_filter flt;
    memset(&flt, 0, sizeof flt);
    flt.min_identity = read_f64(); flt.min_q_cover = read_f64();
    aln_seqset *set = aln_seqset_create(ctx, codes, s_off, s_len, (size_t)n_seqs, &status);
    rc("seqset_create", 0, status);
    if (set) {
        aln_seqset_block blk;
        memset(&blk, 0, sizeof blk);
        blk.q_first = 0; blk.q_count = n_seqs; blk.t_first = 0; blk.t_count = n_seqs; blk.upper = 1;
        uint64_t count = 0;
        rc("seqset_hits", 0, aln_seqset_hits(set, &p, &blk, f_min, &count));
        printf("held %" PRIu64 "\n", count);
        for (int with_filter = 0; with_filter <= 1; ++with_filter)
            for (uint32_t mode = ALN_CLUSTER_COMPONENTS; mode <= ALN_CLUSTER_GREEDY; ++mode) {
                uint32_t *label = (uint32_t *)guarded(4 * n_seqs);
                aln_cluster_record *rec = (aln_cluster_record *)guarded(sizeof(aln_cluster_record) * n_seqs);
                aln_cluster_summary *sum = (aln_cluster_summary *)guarded(sizeof(aln_cluster_summary));
                rc(with_filter ? "held_cluster_filter" : "held_cluster", mode,
                   aln_seqset_held_cluster(set, with_filter ? &p : NULL, with_filter ? ALN_REPORT_SKIP_SEED : 0u, with_filter ? &flt : NULL, mode, label, rec,
                                           n_seqs, sum));
                print_result(label, n_seqs, rec, n_seqs, sum);
            }
        aln_seqset_destroy(set);
    }
    aln_destroy(ctx);
    fclose(g_in);
    const int ok = guards_ok();
    printf("guards %s\n", ok ? "ok" : "TOUCHED");
    return (g_fail || !ok) ? 1 : 0;
}
