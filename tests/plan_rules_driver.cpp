// plan_rules_driver.cpp -- runs the batch plan of aligner_amd/csrc/aln_plan_rules.h on the CPU (tests/test_plan_rules_cpu.py builds it
// with g++; no HIP).  Usage: plan_rules_driver CASES.  One case per line of CASES (plan_cases.case_line writes them):
//   name tables n_total first n allow_overlap many_chunks cus  <12 call facts>  <22 knob words>  lists
// tables: n_total records of four u64 (q_off, q_len, t_off, t_len); lists: "-" or a file that receives the plan's pair lists and
// every pair's cost.  One line per case goes to stdout: the name, then key=value words.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "aln_plan_rules.h"

static uint64_t fnv(const void *p, size_t bytes)
{
    uint64_t h = 1469598103934665603ull;
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
template <class T> static uint64_t fnv(const std::vector<T> &v) { return fnv(v.data(), v.size() * sizeof(T)); }

static AlnKnob knob(std::istream &in)
{
    AlnKnob k;
    int set;
    in >> set >> k.v;
    k.set = set != 0;
    return k;
}
static bool flag(std::istream &in) { int v; in >> v; return v != 0; }

static void list(FILE *f, const char *name, const std::vector<uint32_t> &v)
{
    fprintf(f, "%s", name);
    for (uint32_t x : v) fprintf(f, " %u", x);
    fprintf(f, "\n");
}

// the fields slot_ensure sizes from a range's own plan, against the bounds of that range raised over all ranges
static const char *bound_missed(const AlnPlanBounds &b, const Chunk &k)
{
    if (k.seq_span > b.seq_span) return "seq_span";
    if (k.n > b.n) return "n";
    if (k.dir_bytes > b.dir_bytes) return "dir_bytes";
    if (k.tb_bytes > b.tb_bytes) return "tb_bytes";
    if (k.tag_bytes > b.tag_bytes) return "tag_bytes";
    if ((uint64_t)k.grid * 4 * k.scratch_stride > b.scratch) return "scratch";
    if (k.coop && k.coop_bytes > b.coop) return "coop";
    return nullptr;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream cases(argv[1]);
    if (!cases) return 3;
    std::string line;
    Chunk k;
    while (std::getline(cases, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string name, tables, lists;
        size_t n_total, first, n;
        int allow, many;
        uint32_t cus;
        in >> name >> tables >> n_total >> first >> n >> allow >> many >> cus;
        AlnPlanCall c;
        c.pwm = flag(in); c.fast = flag(in); c.is_int = flag(in); c.want_h = flag(in); c.want_tb = flag(in); c.store_dirs = flag(in);
        in >> c.semantics >> c.rows >> c.cols;
        c.hazard = flag(in); c.force_serial = flag(in); c.pair_matrices = flag(in);
        AlnPlanKnobs kn;
        kn.single_r = knob(in); kn.no_single = flag(in); kn.no_coop = flag(in); kn.big_to_single = knob(in); kn.no_wgpipe = flag(in);
        kn.wg_r = knob(in); kn.tb_overlap = knob(in); kn.tb_overlap_any = flag(in); in >> kn.coop_lean; kn.coop_tail = knob(in);
        kn.chain_wgs = knob(in); kn.fill_wgs = knob(in); kn.no_duo = flag(in);
        { int set; in >> set >> kn.chunk_cells; kn.chunk_cells_set = set != 0; }
        in >> lists;
        if (!in) { fprintf(stderr, "bad case line: %s\n", line.c_str()); return 4; }
        std::vector<uint64_t> tab(4 * n_total), q_off(n_total), q_len(n_total), t_off(n_total), t_len(n_total);
        if (n_total) {
            FILE *f = fopen(tables.c_str(), "rb");
            if (!f || fread(tab.data(), 32, n_total, f) != n_total) { fprintf(stderr, "cannot read %s\n", tables.c_str()); return 5; }
            fclose(f);
        }
        for (size_t i = 0; i < n_total; ++i) { q_off[i] = tab[4 * i]; q_len[i] = tab[4 * i + 1]; t_off[i] = tab[4 * i + 2]; t_len[i] = tab[4 * i + 3]; }

        k.reset();
        AlnShareTrace tr;
        aln_plan_chunk(cus, c, kn, q_off.data(), q_len.data(), t_off.data(), t_len.data(), first, n, allow != 0, many != 0, k, &tr);
        printf("%s first=%zu n=%zu n_small=%zu cells=%" PRIu64 " max_cells=%" PRIu64 " dir_bytes=%" PRIu64 " tb_bytes=%" PRIu64 " tag_bytes=%" PRIu64
               " hmat_elems=%" PRIu64 " max_len=%u grid=%u zrow_bytes=%u lds_bytes=%u prof_stride=%u tb_waves=%u single_max_n=%u cascade_rows=%u"
               " duo_qo=%u scratch_stride=%" PRIu64 " granule_bytes=%" PRIu64 " tbmap_entries=%" PRIu64 " granule_stride_max=%" PRIu64
               " counter_bytes=%zu overlap=%d coop=%d coop_linger=%d coop_lean=%d coop_tail=%u coop_bytes=%" PRIu64 " seq_direct=%d seq_lo=%" PRIu64
               " seq_span=%" PRIu64,
               name.c_str(), k.first, k.n, k.n_small, k.cells, k.max_cells, k.dir_bytes, k.tb_bytes, k.tag_bytes, k.hmat_elems, k.max_len, k.grid,
               k.zrow_bytes, k.lds_bytes, k.prof_stride, k.tb_waves, k.single_max_n, k.cascade_rows, k.duo_qo, k.scratch_stride, k.granule_bytes,
               k.tbmap_entries, k.granule_stride_max, k.counter_bytes, (int)k.overlap, (int)k.coop, (int)k.coop_linger, (int)k.coop_lean, k.coop_tail,
               k.coop_bytes, (int)k.seq_direct, k.seq_lo, k.seq_span);
        printf(" h_descs=%" PRIu64 " h_order=%" PRIu64 " h_single_pairs=%" PRIu64 " h_single_r=%" PRIu64 " h_wg_pairs=%" PRIu64 " h_wg_r=%" PRIu64
               " n_single=%zu n_wg=%zu",
               fnv(k.descs), fnv(k.order), fnv(k.single_pairs), fnv(k.single_r), fnv(k.wg_pairs), fnv(k.wg_r), k.single_pairs.size(), k.wg_pairs.size());
        const AlnPlanBounds b = aln_plan_bounds(cus, c, q_off.data(), q_len.data(), t_off.data(), t_len.data(), first, n);
        printf(" need_seq_span=%" PRIu64 " need_n=%" PRIu64 " need_dir_bytes=%" PRIu64 " need_tb_bytes=%" PRIu64 " need_tag_bytes=%" PRIu64
               " need_scratch=%" PRIu64 " need_coop=%" PRIu64,
               b.seq_span, b.n, b.dir_bytes, b.tb_bytes, b.tag_bytes, b.scratch, b.coop);
        uint64_t stored = 0;
        for (const PairDesc &d : k.descs) stored += aln_pair_stored_dir_bytes(d);
        printf(" stored_dir_bytes=%" PRIu64, stored);
        if (tr.could_share) printf(" lean_waves=%" PRIu64 " lean_tail=%" PRIu64, tr.lp.waves, tr.lp.tail);
        if (lists != "-") {
            FILE *f = fopen(lists.c_str(), "w");
            if (!f) return 6;
            list(f, "order", k.order); list(f, "single", k.single_pairs); list(f, "single_r", k.single_r); list(f, "wg", k.wg_pairs); list(f, "wg_r", k.wg_r);
            fprintf(f, "cost");
            for (const PairDesc &d : k.descs) fprintf(f, " %" PRIu64, aln_pair_cost(d));
            fprintf(f, "\n");
            fclose(f);
        }

        // the chunks of the whole list on one device, as aln_align_batch cuts them; with several, every range's own plan against
        // the bounds raised over all ranges (what a slot of the pipeline is sized with before it runs)
        std::vector<std::pair<size_t, size_t>> ranges;
        if (n_total) aln_make_chunks(c, kn, q_len.data(), t_len.data(), n_total, 1, ranges, 12.0 * (double)cus);
        printf(" chunks=");
        for (size_t i = 0; i < ranges.size(); ++i) printf("%s%zu:%zu", i ? "," : "", ranges[i].first, ranges[i].second);
        if (ranges.empty()) printf("none");
        if (ranges.size() > 1) {
            AlnPlanBounds all;
            for (const auto &r : ranges) all.raise(aln_plan_bounds(cus, c, q_off.data(), q_len.data(), t_off.data(), t_len.data(), r.first, r.second));
            const char *missed = nullptr;
            size_t at = 0;
            Chunk kr;
            for (size_t i = 0; i < ranges.size() && !missed; ++i) {
                kr.reset();
                aln_plan_chunk(cus, c, kn, q_off.data(), q_len.data(), t_off.data(), t_len.data(), ranges[i].first, ranges[i].second, false,
                               ranges.size() > 4, kr);
                missed = bound_missed(all, kr);
                at = i;
            }
            if (missed) printf(" bounds=%s@%zu", missed, at);
            else printf(" bounds=hold");
        }
        printf("\n");
    }
    return 0;
}
