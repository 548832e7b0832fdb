"""Helpers of the sequence-set call-history tests (tests/test_set_history_*.py).  Not a test module (no test_ prefix).

A resident sequence set keeps grow-only device buffers, one block of counters and host state (the held pass and its serial, the two
indexes' k, the candidate list, the last CIGAR and MSA plans) from call to call.  These helpers walk ONE handle through
call_history.schedule(k) -- every ordered pair of catalogue entries exactly once -- and hold every answer against references that are
computed from the CPU oracle and the Python rule restatements alone:

* set_a() / set_b(): the two seeded sets.  CATALOGUE / B_CATALOGUE / B_ROTATION: the calls, each with fixed arguments.
* Refs: the expected bytes of (entry, the part of the state the entry reads), memoised, saved and loaded as call_history does.
* Model: the state model, pure Python.  step(entry) answers the key of the expected bytes, or the kind of the expected refusal.
* walk(): the walker over any backend.  GpuBackend calls the library through ctypes on marker-filled buffers; FakeBackend answers from
  the references and can have one defect switched on (tests/test_set_history_cpu.py shows that the walker catches each).
* planned_chunks(): aln_seqset_cut (aligner_amd/csrc/aln_seqset_rules.h) under a forced ALN_CHUNK_CELLS, restated.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import call_history as CH  # noqa: E402
import cigar_ref  # noqa: E402
import cluster_ref  # noqa: E402
import msa_ref  # noqa: E402
import prefilter_ref  # noqa: E402
import profile_ref  # noqa: E402
import report_ref  # noqa: E402
import shuffle_ref  # noqa: E402
import signif_ref  # noqa: E402
import strand_cases  # noqa: E402
import strand_ref  # noqa: E402
import wordjoin_ref  # noqa: E402

INV = 7                              # ALN_ERR_INVALID_ARGUMENT (asserted against _ffi by the GPU backend)
CORE_GLOBAL, CORE_LOCAL = 0, 1
BLANK = 98
MARK = 0x5A                          # every output buffer starts as bytes of this
COUNT_MARK = 0xABCDEF
FIELDS = ("f", "score", "end_y", "end_x", "start_y", "start_x", "aln_len", "status")
RES = np.dtype([("f", "<f8"), ("score", "<f8"), ("end_y", "<u4"), ("end_x", "<u4"), ("start_y", "<u4"), ("start_x", "<u4"),
                ("aln_len", "<u4"), ("status", "<i4")])
SEED, PER_PAIR, MAX_TRIM, SIGNIF_KEEP = 0x5E7A11, 7, 6, 16
N_CODES = 20
MIN_IDENTITY = 0.3
CIGAR_FLAGS = cigar_ref.EXTENDED | cigar_ref.CLIPS
B_CIGAR_FLAGS = cigar_ref.CLIPS
CHUNK_CELLS = 6000000                # ALN_CHUNK_CELLS of the chunked walk: the large pass and the large score run in 3 chunks or more

# ---------------------------------------------------------------- the sets
SPECIAL = (0, 1, 2, 15, 16, 17, 255, 256, 257, 511, 512, 513, 700)
FAMILIES = ((13, 6, 180), (19, 4, 120), (23, 2, 90))          # (first record, members, ancestor length)
N_A = 48


def _member(rng, anc, k):
    """a family member: substitutions, and (but for the first) a planted insert and a planted deletion, so that centre-star inserts exist"""
    s = anc.copy()
    mut = rng.random(len(s)) < 0.10
    s[mut] = rng.integers(0, 20, int(mut.sum()))
    if k:
        at = int(rng.integers(20, len(s) - 30))
        s = np.insert(s, at, rng.integers(0, 20, 2 + k % 4))
        at = int(rng.integers(10, len(s) - 20))
        s = np.delete(s, np.arange(at, at + 1 + k % 3))
    return s.astype(np.uint8)


def set_a(seed=20261020):
    """48 proteins: the SPECIAL lengths (the long ones share mutated pieces of one ancestor, so that their pairs align at length), three
    planted families of 6, 4 and 2 members, and 23 unrelated records of 30 .. 200 residues."""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 20, 700).astype(np.uint8)
    seqs = []
    for n in SPECIAL:
        s = rng.integers(0, 20, n).astype(np.uint8)
        if n >= 255:
            a = int(rng.integers(0, 700 - n + 1))
            piece = anc[a:a + n].copy()
            mut = rng.random(n) < 0.35
            piece[mut] = rng.integers(0, 20, int(mut.sum()))
            keep = rng.random(n) < 0.7
            s[keep] = piece[keep]
        seqs.append(s)
    for first, members, length in FAMILIES:
        assert first == len(seqs)
        fam = rng.integers(0, 20, length).astype(np.uint8)
        seqs += [_member(rng, fam, k) for k in range(members)]
    while len(seqs) < N_A:
        seqs.append(rng.integers(0, 20, int(rng.integers(30, 201))).astype(np.uint8))
    return seqs


def set_b():
    """10 nucleotide records of strand_cases.parity_records: a planted minus-strand pair (A, B), a plus-strand pair (A, NEAR), a palindrome"""
    recs = strand_cases.parity_records()[:10]
    assert max(strand_cases.A, strand_cases.B, strand_cases.PAL, strand_cases.NEAR) < len(recs)
    return recs


def resident_b(recs):
    return recs + [strand_cases.revcomp(r) for r in recs]


def schemes():
    from aligner_amd.matrices import get_blosum62, nucleotide_matrix
    return {"local": (CORE_LOCAL, get_blosum62(), 11.0, 2.0), "global": (CORE_GLOBAL, get_blosum62(), 4.0, 4.0),
            "dna": (CORE_LOCAL, nucleotide_matrix(), strand_cases.DEL, strand_cases.EXT)}


def upper(first, count):
    return (first, count, first, count, 1)


def rect(qf, qc, tf, tc):
    return (qf, qc, tf, tc, 0)


# ---------------------------------------------------------------- the catalogue: one call with fixed arguments per entry
BIG = upper(0, N_A)
PRODUCERS = {
    "hits_large": dict(block=BIG, f_min=24.0, scheme="local"),
    "hits_small": dict(block=rect(13, 3, 17, 5), f_min=300.0, scheme="local"),
    "best3": dict(block=rect(13, 16, 5, 36), k=3, scheme="local"),
    "hits_global": dict(block=rect(0, 4, 0, 6), f_min=-1e300, scheme="global"),
    "cand_hits": dict(f_min=60.0, scheme="local"),
}
SCORES = {"score_large": BIG, "score_row": rect(12, 1, 0, N_A)}
KMERS = {"kmer2": 2, "kmer3": 3}
PREFILTERS = {"pf1": dict(k=2, block=BIG, min_shared=40, per=0), "pf2": dict(k=3, block=rect(13, 12, 0, N_A), min_shared=3, per=40)}
WORD_K = 5
WORDJOIN = dict(k=WORD_K, block=BIG, min_shared=2, per=0)
CONSUMERS = ("strings", "report", "filter", "cluster_components", "cluster_greedy", "profiles", "msa", "cigars", "signif")
FILLS = ("cigar_fill", "msa_fill")
# The order decides which state every transition of the schedule meets.  This one was picked (by trying seeded shuffles against the
# model alone) so that every consumer is accepted at least once after every producer, the list's included, and both fills answer.
CATALOGUE = ("hits_large", "profiles", "kmer3", "word5", "report", "signif", "cigars", "pf2", "word_join", "best3", "msa_fill", "cluster_greedy",
             "cluster_components", "strings", "hits_small", "kmer2", "score_large", "pf1", "filter", "cand_hits", "score_row", "hits_global",
             "cigar_fill", "msa")
assert sorted(CATALOGUE) == sorted(tuple(PRODUCERS) + tuple(SCORES) + ("kmer2", "kmer3", "pf1", "pf2", "word5", "word_join") + CONSUMERS + FILLS)
assert 16 <= len(CATALOGUE) <= 24
LISTS = {"pf1": "pf1", "pf2": "pf2", "word_join": "wj"}

B_CATALOGUE = ("b_hits", "b_score_minus", "b_scig", "b_pcig", "b_sfill")
B_ROTATION = ("b_hits", "b_scig", "b_sfill", "b_pcig", "b_sfill", "b_hits", "b_sfill", "b_scig", "b_score_minus", "b_sfill", "b_hits", "b_pcig")
KINDS = ("nothing_held", "no_index", "no_list", "stale_plan", "other_family")


def block_pairs(block):
    return prefilter_ref.block_pairs(block)


def block_nodes(block):
    qf, qc, tf, tc, _up = block
    return sorted(set(range(qf, qf + qc)) | set(range(tf, tf + tc)))


# ---------------------------------------------------------------- references
def align_pairs(orc, seqs, pairs, scheme, threads=16):
    """(RES array, [(aligned query, aligned target)]) of the listed (q, t) pairs from the oracle"""
    sem, m, d, e = scheme
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    packed = np.concatenate(list(seqs) + [np.zeros(0, np.uint8)]).astype(np.uint8)
    q = np.array([p[0] for p in pairs], dtype=np.int64)
    t = np.array([p[1] for p in pairs], dtype=np.int64)
    ref, tb, tb_off = orc.align_batch(sem, packed, off[q], lens[q], off[t], lens[t], d, e, m, n_threads=threads, blank=BLANK)
    r = np.frombuffer(ref, dtype=CH.ORC_DTYPE)
    res = np.zeros(len(pairs), dtype=RES)
    for name in FIELDS:
        res[name] = r[name]
    strs = []
    for i in range(len(pairs)):
        n = int(res["aln_len"][i]) if res["status"][i] == 0 else 0
        a, cap = int(tb_off[i]), int(lens[q[i]] + lens[t[i]] + 2)
        strs.append((tb[a:a + n].copy(), tb[a + cap:a + cap + n].copy()))
    return res, strs


class Held:
    """the reference of a held pass: the list (index, q, t, f), the summaries and the strings of every held hit"""

    def __init__(self, block, scheme_name, index, pairs, res, strs):
        self.block, self.scheme = block, scheme_name
        self.index = np.asarray(index, dtype=np.uint64)
        self.q = np.array([pairs[i][0] for i in index], dtype=np.uint32)
        self.t = np.array([pairs[i][1] for i in index], dtype=np.uint32)
        self.res = res[np.asarray(index, dtype=np.int64)] if len(index) else res[:0]
        self.strs = [strs[i] for i in index]
        self.f = self.res["f"].copy()

    def __len__(self):
        return len(self.index)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def struct_fields(prefix, arr):
    return {prefix + "." + name: bits(np.ascontiguousarray(arr[name])) for name in arr.dtype.names if not name.startswith("reserved")}


class Refs:
    """Expected values by name "entry@key".  With an oracle they are computed on demand and memoised; without one (a child process,
    the fake backend after load) they are what load() read."""

    def __init__(self, seqs_a, recs_b, orc=None):
        self.a = [np.asarray(s, dtype=np.uint8) for s in seqs_a]
        self.recs_b = recs_b
        self.b = resident_b(recs_b)
        self.len_a = np.array([len(s) for s in self.a], dtype=np.uint64)
        self.len_b = np.array([len(s) for s in self.b], dtype=np.uint64)
        self.orc, self.memo, self._pairs, self._held, self._lists, self._labels = orc, {}, {}, {}, {}, {}

    # ---- what everything else is derived from
    def pairs(self, which, block, scheme):
        key = (which, block, scheme)
        if key not in self._pairs:
            pairs = block_pairs(block)
            self._pairs[key] = (pairs,) + align_pairs(self.orc, self.a if which == "A" else self.b, pairs, schemes()[scheme])
        return self._pairs[key]

    def cand_list(self, name):
        if name not in self._lists:
            if name == "wj":
                w = WORDJOIN
                self._lists[name] = (w["block"],) + wordjoin_ref.word_join(self.a, w["k"], 20, w["min_shared"], w["per"], w["block"])
            else:
                p = PREFILTERS[name]
                self._lists[name] = (p["block"],) + prefilter_ref.prefilter(self.a, p["k"], 20, p["min_shared"], p["per"], p["block"])
        return self._lists[name]

    def held(self, hid):
        """hid: a producer's name, "cand_hits:<list>", or "b_hits" """
        if hid in self._held:
            return self._held[hid]
        if hid == "b_hits":
            n = len(self.recs_b)
            block = rect(0, n, 0, 2 * n)
            pairs, res, strs = self.pairs("B", block, "dna")
            index = np.flatnonzero((res["status"] == 0) & (res["f"] >= strand_cases.F_MIN))
            h = Held(block, "dna", index, pairs, res, strs)
        elif hid.startswith("cand_hits:"):
            block, idx, _q, _t, _sh = self.cand_list(hid.split(":")[1])
            spec = PRODUCERS["cand_hits"]
            pairs, res, strs = self.pairs("A", block, spec["scheme"])
            index = [i for i in idx if res["status"][i] == 0 and res["f"][i] >= spec["f_min"]]
            h = Held(block, spec["scheme"], index, pairs, res, strs)
        else:
            spec = PRODUCERS[hid]
            pairs, res, strs = self.pairs("A", spec["block"], spec["scheme"])
            if "k" in spec:                            # the k best of every query: higher f first, equal f by the lower target, no (i, i)
                index = []
                tc = spec["block"][3]
                for row in range(spec["block"][1]):
                    mine = [i for i in range(row * tc, (row + 1) * tc) if res["status"][i] == 0 and pairs[i][0] != pairs[i][1]]
                    mine.sort(key=lambda i: (-float(res["f"][i]), pairs[i][1]))
                    index += sorted(mine[:spec["k"]])
            else:
                index = np.flatnonzero((res["status"] == 0) & (res["f"] >= spec["f_min"]))
            h = Held(spec["block"], spec["scheme"], index, pairs, res, strs)
        self._held[hid] = h
        return h

    def labels(self, hid):
        """(labels, centres) for profiles and msa: the components of the CPU cluster model of the held pass"""
        if hid not in self._labels:
            h = self.held(hid)
            lab, _recs, _summ, _mem = cluster_ref.cluster(cluster_ref.COMPONENTS, len(self.a), h.q, h.t, self.len_a, block_nodes(h.block))
            lab = np.array(lab, dtype=np.uint32)
            size = {}
            for v in lab.tolist():
                size[v] = size.get(v, 0) + 1
            centers = np.array([v for v in range(len(lab)) if lab[v] == v and size[v] > 1], dtype=np.uint32)
            self._labels[hid] = (lab, centers)
        return self._labels[hid]

    # ---- the entries
    def get(self, name):
        if name not in self.memo:
            entry, key = name.split("@")
            self.memo[name] = {k: np.asarray(v) for k, v in self.compute(entry, key).items()}
        return self.memo[name]

    def compute(self, entry, key):
        if entry in PRODUCERS or entry == "b_hits":
            h = self.held(entry if key == "-" else entry + ":" + key)
            return dict(count=len(h), index=h.index, q=h.q, t=h.t, f=bits(h.f))
        if entry in SCORES or entry == "b_score_minus":
            if entry in SCORES:
                _p, res, _s = self.pairs("A", SCORES[entry], "local")
            else:
                n = len(self.recs_b)
                _p, res, _s = self.pairs("B", rect(0, n, n, n), "dna")
            return dict(f=bits(np.where(res["status"] == 0, res["f"], 0.0)), pair_status=res["status"])
        if entry in KMERS:
            return dict(n_words=np.array([len(prefilter_ref.words(s, KMERS[entry], 20)) for s in self.a], dtype=np.uint32))
        if entry == "word5":
            return dict(n_words=np.array([len(wordjoin_ref.words(s, WORD_K, 20)) for s in self.a], dtype=np.uint32))
        if entry in LISTS:
            _block, idx, q, t, sh = self.cand_list(LISTS[entry])
            return dict(count=len(idx), index=np.array(idx, dtype=np.uint64), q=np.array(q, dtype=np.uint32), t=np.array(t, dtype=np.uint32),
                        shared=np.array(sh, dtype=np.uint32))
        if entry.startswith("b_"):
            return self.compute_b(entry)
        h = self.held(key)
        sem, m, d, e = schemes()[h.scheme]
        n = len(h)
        if entry == "strings":
            keep = np.array(list(range(n - 1, -1, -max(1, n // 11)))[:12] + [n - 1], dtype=np.uint32)       # descending, with a repeat
            cap = (self.len_a[h.q[keep]] + self.len_a[h.t[keep]] + 2).astype(np.int64)
            off = np.concatenate([[0], np.cumsum(2 * cap)[:-1]]).astype(np.uint64)
            tb = np.zeros(int((2 * cap).sum()), dtype=np.uint8)
            for k, pos in enumerate(keep):
                qa, ta = h.strs[int(pos)]
                tb[int(off[k]):int(off[k]) + len(qa)] = qa
                tb[int(off[k]) + int(cap[k]):int(off[k]) + int(cap[k]) + len(ta)] = ta
            out = dict(_arg_keep=keep, _arg_off=off, tb=tb, slack=np.full(8192, MARK, dtype=np.uint8))
            out.update(struct_fields("res", h.res[keep]))
            return out
        if entry in ("report", "filter"):
            rep = report_ref.reports(h.strs, m, report_ref.SKIP_SEED, h.res["status"], BLANK)
            if entry == "report":
                out = dict(_arg_held=n)
                out.update(struct_fields("rep", rep))
                return out
            kept = np.flatnonzero(report_ref.keep(rep, self.len_a[h.q], self.len_a[h.t], min_identity=MIN_IDENTITY)).astype(np.uint32)
            out = dict(_arg_held=n, count=len(kept), positions=kept)
            out.update(struct_fields("rep", rep[kept]))
            return out
        if entry.startswith("cluster_"):
            mode = cluster_ref.COMPONENTS if entry == "cluster_components" else cluster_ref.GREEDY
            lab, recs, summ, _mem = cluster_ref.cluster(mode, len(self.a), h.q, h.t, self.len_a, block_nodes(h.block))
            out = dict(label=np.array(lab, dtype=np.uint32), records=np.array(recs, dtype=np.uint32).reshape(-1, 4))
            out.update({"summary." + k: v for k, v in summ.items()})
            return out
        if entry == "profiles":
            lab, centers = self.labels(key)
            flat, recs, summ = profile_ref.profiles(h.q, h.t, h.res, h.strs, lab.tolist(), centers, self.len_a, N_CODES, BLANK, profile_ref.SKIP_SEED,
                                                    None, self.a)
            out = dict(_arg_label=lab, _arg_centers=centers, out=flat, records=np.array(recs, dtype=np.uint32).reshape(-1, 4))
            out.update({"summary." + k: v for k, v in summ.items()})
            return out
        if entry in ("msa", "msa_fill"):
            lab, centers = self.labels(key)
            mats, lists, recs, summ = msa_ref.alignments(h.q, h.t, h.res, h.strs, lab.tolist(), centers, self.len_a, self.a, BLANK)
            flat, row_hit = msa_ref.flat(mats, lists)
            if entry == "msa_fill":
                return dict(_arg_bytes=len(flat), _arg_rows=len(row_hit), out=flat, row_hit=row_hit)
            out = dict(_arg_label=lab, _arg_centers=centers, _n_ins=sum(r[3] for r in recs), records=np.array(recs, dtype=np.uint32).reshape(-1, 4),
                       out=flat, row_hit=row_hit)
            out.update({"summary." + k: v for k, v in summ.items()})
            return out
        if entry in ("cigars", "cigar_fill"):
            entries = [(h.strs[i][0], h.strs[i][1], int(h.res["aln_len"][i]), int(h.res["status"][i]), int(h.res["start_x"][i]),
                        int(h.res["start_y"][i]), int(self.len_a[h.q[i]])) for i in range(n)]
            recs, off, words, summ = cigar_ref.listed(entries, list(range(n)), n, BLANK, CIGAR_FLAGS)
            words, off = np.array(words, dtype=np.uint32), np.array(off, dtype=np.uint64)
            if entry == "cigar_fill":
                return dict(_arg_n=n, _arg_total=len(words), words=words, offsets=off)
            out = dict(_arg_held=n, records=np.array(recs, dtype=np.int64).reshape(-1, 8), offsets=off, words=words, bytes_up=4 * n, bytes_down=32 * n + 32)
            out.update({"summary." + k: v for k, v in summ.items()})
            return out
        if entry == "signif":
            ok = np.flatnonzero(self.len_a[h.t] >= MAX_TRIM)
            keep = ok[::max(1, len(ok) // SIGNIF_KEEP)][:SIGNIF_KEEP].astype(np.uint32)
            copies, lengths = [], np.zeros((len(keep), PER_PAIR), dtype=np.uint32)
            for k, pos in enumerate(keep):
                for s in range(PER_PAIR):
                    c = shuffle_ref.copy_of(self.a[int(h.t[pos])], SEED, int(h.index[pos]), s, MAX_TRIM)[1]
                    lengths[k, s] = len(c)
                    copies.append((self.a[int(h.q[pos])], np.asarray(c, dtype=np.uint8)))
            seqs = [x for pair in copies for x in pair]
            res, _strs = align_pairs(self.orc, seqs, [(2 * i, 2 * i + 1) for i in range(len(copies))], (sem, m, d, e)) if copies else (np.zeros(0, RES), [])
            f = np.where(res["status"] == 0, res["f"], 0.0).reshape(len(keep), PER_PAIR)
            rec = signif_ref.reduce_many(f, res["status"].reshape(len(keep), PER_PAIR), h.f[keep])
            out = dict(_arg_keep=keep, _global=int(h.scheme == "global"), f=bits(f), lengths=lengths, bytes_down=48 * len(keep) + 8 * PER_PAIR * len(keep))
            out.update(struct_fields("rec", rec))
            return out
        raise KeyError(entry)

    def compute_b(self, entry):
        h = self.held("b_hits")
        n, held = len(self.recs_b), len(h)
        entries = [(h.strs[i][0], h.strs[i][1], int(h.res["aln_len"][i]), int(h.res["status"][i]), int(h.res["start_x"][i]),
                    int(h.res["start_y"][i]), int(self.len_b[h.q[i]])) for i in range(held)]
        which = list(range(held))
        if entry == "b_pcig":
            recs, off, words, summ = cigar_ref.listed(entries, which, held, BLANK, B_CIGAR_FLAGS)
            strands, up = None, 4
        else:
            pairs = list(zip(h.q.tolist(), h.t.tolist()))
            recs, strands, off, words, summ = strand_ref.listed(entries, pairs, self.len_b, which, n, held, BLANK, B_CIGAR_FLAGS)
            up = 5
        words, off = np.array(words, dtype=np.uint32), np.array(off, dtype=np.uint64)
        if entry == "b_sfill":
            return dict(_arg_n=held, _arg_total=len(words), words=words, offsets=off)
        out = dict(_arg_held=held, records=np.array(recs, dtype=np.int64).reshape(-1, 8), offsets=off, words=words, bytes_up=up * held,
                   bytes_down=32 * held + 32)
        if strands is not None:
            out["strands"] = np.array(strands, dtype=np.uint32).reshape(-1, 5)
        out.update({"summary." + k: v for k, v in summ.items()})
        return out

    def save(self, path):
        CH.save_expected(path, self.memo)

    def load(self, path):
        self.memo.update(CH.load_expected(path))
        return self


# ---------------------------------------------------------------- the state model
class State:
    def __init__(self):
        self.held = None            # the id of the held pass ("hits_large", "cand_hits:pf1", ...)
        self.serial = 0             # passes so far (every score, hits and best that got as far as replacing the held hits)
        self.kmer_k = 0
        self.word_k = 0
        self.cand = None            # "pf1" | "pf2" | "wj"
        self.cigar_plan = None      # (family, held id, serial)
        self.msa_plan = None        # (held id, serial)

    def text(self):
        return "held=%s serial=%d kmer_k=%d word_k=%d cand=%s cigar_plan=%s msa_plan=%s" % (self.held, self.serial, self.kmer_k, self.word_k, self.cand,
                                                                                            self.cigar_plan, self.msa_plan)


class Model:
    """What a handle must answer.  The rules are the comments of aln_host.hip and INTEGRATION.md: a pass (score, hits, best, over a
    block or over the list) replaces the held hits once it is past its own refusals, a score holds nothing; an index call drops the
    candidate list, prefilter and word_join need the index of their own k; a fill needs the last plan of its family, made of the hits
    that are held now; a refused call changes nothing."""

    def __init__(self, which="A"):
        self.which, self.s = which, State()

    def step(self, entry):
        """(name of the expected value or None, refusal kind or None, name of the arguments' expected value): the state moves on"""
        s = self.s
        if entry in ("hits_large", "hits_small", "best3", "hits_global", "b_hits"):
            s.held, s.serial = entry, s.serial + 1
            return entry + "@-", None, entry + "@-"
        if entry == "cand_hits":
            if s.cand is None:
                return None, "no_list", "cand_hits@pf1"
            s.held, s.serial = "cand_hits:" + s.cand, s.serial + 1
            return "cand_hits@" + s.cand, None, "cand_hits@" + s.cand
        if entry in SCORES or entry == "b_score_minus":
            s.held, s.serial = None, s.serial + 1
            return entry + "@-", None, entry + "@-"
        if entry in KMERS:
            s.kmer_k, s.cand = KMERS[entry], None
            return entry + "@-", None, entry + "@-"
        if entry == "word5":
            s.word_k, s.cand = WORD_K, None
            return entry + "@-", None, entry + "@-"
        if entry in LISTS:
            need, have = (WORD_K, s.word_k) if entry == "word_join" else (PREFILTERS[entry]["k"], s.kmer_k)
            if need != have:
                return None, "no_index", entry + "@-"
            s.cand = LISTS[entry]
            return entry + "@-", None, entry + "@-"
        default = "b_hits" if self.which == "B" else "hits_small"
        if entry in ("cigar_fill", "msa_fill", "b_sfill"):
            plan = s.msa_plan if entry == "msa_fill" else s.cigar_plan
            family = "stranded" if entry == "b_sfill" else "plain"
            name = {"cigar_fill": "cigar_fill@", "msa_fill": "msa_fill@", "b_sfill": "b_sfill@"}[entry]
            sized = name + ("-" if self.which == "B" else (plan[-2] if plan else default))
            if s.held is None:
                return None, "nothing_held", sized
            if plan is None or plan[-1] != s.serial:
                return None, "stale_plan", sized
            if entry != "msa_fill" and plan[0] != family:
                return None, "other_family", sized
            return sized, None, sized
        # consumers of the held hits
        key = "-" if self.which == "B" else (s.held or default)
        name = entry + "@" + key
        if s.held is None:
            return None, "nothing_held", name
        if entry in ("cigars", "b_pcig"):
            s.cigar_plan = ("plain", s.held, s.serial)
        elif entry == "b_scig":
            s.cigar_plan = ("stranded", s.held, s.serial)
        elif entry == "msa":
            s.msa_plan = (s.held, s.serial)
        return name, None, name


def prerequisites(state, entry):
    """the shortest list of calls that puts a fresh handle of A into the part of `state` that `entry` reads"""
    out = []
    if entry in ("pf1", "pf2") and state.kmer_k:
        out.append("kmer%d" % state.kmer_k)
    if entry == "word_join" and state.word_k:
        out.append("word5")
    cand = state.cand if entry == "cand_hits" else (state.held.split(":")[1] if state.held and ":" in state.held else None)
    if cand:
        out += {"pf1": ["kmer2", "pf1"], "pf2": ["kmer3", "pf2"], "wj": ["word5", "word_join"]}[cand]
    if entry in CONSUMERS + FILLS and state.held:
        out.append(state.held.split(":")[0])
        if entry == "cigar_fill" and state.cigar_plan and state.cigar_plan[-1] == state.serial:
            out.append("cigars")
        if entry == "msa_fill" and state.msa_plan and state.msa_plan[-1] == state.serial:
            out.append("msa")
    return out


def rotated_schedule():
    seq = CH.schedule(len(CATALOGUE))
    assert CATALOGUE[seq[0]] in PRODUCERS            # (the circuit is closed: any rotation of it holds every transition once)
    return seq


def dry_run(calls=None):
    """[(step, which, previous entry, entry, expected name | None, refusal kind | None, arguments' name, state before as text)] of the walk"""
    a, b = Model("A"), Model("B")
    seq = rotated_schedule()[:calls]
    out, prev_a, prev_b = [], None, None
    for i, e in enumerate(seq):
        for which, model, entry, prev in (("A", a, CATALOGUE[e], prev_a), ("B", b, B_ROTATION[i % len(B_ROTATION)], prev_b)):
            before = model.s.text()
            want, kind, args = model.step(entry)
            out.append((i, which, prev, entry, want, kind, args, before))
        prev_a, prev_b = CATALOGUE[e], B_ROTATION[i % len(B_ROTATION)]
    return out


def needed(calls=None):
    names = set()
    for _i, _w, _p, _e, want, _k, args, _b in dry_run(calls):
        names.add(args)
        if want:
            names.add(want)
    return sorted(names)


# ---------------------------------------------------------------- the walker
def compare(got, want):
    return CH.compare(got, want)


def check(got, want):
    """None, or what is wrong with one call's answer; want: the expected value, or None for a refusal"""
    if want is None:
        if int(got["status"]) != INV:
            return "status %d, want the refusal %d" % (int(got["status"]), INV)
        if not got.get("_untouched", True):
            return "a refused call wrote into %s" % got.get("_touched", "an output")
        return None
    if int(got["status"]) != 0:
        return "status %d (%s), want 0" % (int(got["status"]), got.get("_error", ""))
    return compare(got, want)


def walk(backend, refs, calls=None, stop_at_first=False, fresh=True):
    """Runs the schedule on the backend's handle of A, one call on B's handle after every call on A's, and holds every answer
    against refs.  Returns dict(calls, refusals per kind, failures): a failure names the step, the transition, the state and the
    first differing field and position."""
    plan = dry_run(calls)
    a = Model("A")
    failures, refusals, n_calls = [], dict.fromkeys(KINDS, 0), 0
    for i, which, prev, entry, want, kind, args, before in plan:
        state_before = None
        if which == "A":
            state_before = State()
            state_before.__dict__.update(a.s.__dict__)
            a.step(entry)
        got = backend.call(which, entry, refs.get(args), i)
        n_calls += 1
        if kind:
            refusals[kind] += 1
        diff = check(got, refs.get(want) if want else None)
        if int(got["status"]) not in (0, INV):            # an error of the device or the runtime, not an answer: nothing more is started
            failures.append(dict(step=i, which=which, prev=prev, entry=entry, message="step %d on %s: %s -> %s: %s [%s]; the walk ends here" % (
                i, which, prev, entry, diff, before)))
            break
        if diff is not None:
            msg = "step %d on %s: %s -> %s: %s [%s]" % (i, which, prev, entry, diff, before)
            if fresh and which == "A" and hasattr(backend, "fresh"):
                pre = prerequisites(state_before, entry)
                again = backend.fresh(entry, [(p, None) for p in pre], refs, args, want)
                msg += "; a fresh handle after %s %s the reference" % (pre, "agrees with" if again is None else "differs from (%s)" % again)
            failures.append(dict(step=i, which=which, prev=prev, entry=entry, message=msg))
            if stop_at_first:
                break
    return dict(calls=n_calls, refusals=refusals, failures=failures)


def planned_chunks(lengths, block, target):
    """aln_seqset_cut under a forced target of `target` cells: the number of chunks of a pass over the block (cap 2^22 positions)"""
    cells = [float(lengths[q]) * float(lengths[t]) for q, t in block_pairs(block)]
    total = float(sum(cells))
    if total <= 1.5 * target:
        return 1
    chunks, acc, done, n = 0, 0.0, 0.0, 0
    for k, c in enumerate(cells):
        acc += c
        n += 1
        if acc >= target and (total - done - acc >= 0.25 * target or k + 1 == len(cells)):
            chunks, done, acc, n = chunks + 1, done + acc, 0.0, 0
    return chunks + (1 if n else 0)


# ---------------------------------------------------------------- the fake backend (the CPU test's): answers from the references
DEFECTS = ("tail", "count", "stale_fill", "old_index", "leak")


class FakeBackend:
    """A handle pair that answers from the references under the model's own rules -- with one defect switched on, wrongly:
    tail        a held list shorter than the one before it keeps that one's tail
    count       the filter's count is the count whichever family wrote last
    stale_fill  a CIGAR fill answers from the last plan although a pass has replaced the held hits since
    old_index   a prefilter answers from the index that is there, whatever its k
    leak        both handles share the last CIGAR plan: B's stranded fill answers from A's plain plan
    first_effect: the step at which the defect first changed an answer."""

    def __init__(self, refs, defect=None):
        assert defect is None or defect in DEFECTS
        self.refs, self.defect, self.first_effect = refs, defect, None
        self.m = {"A": Model("A"), "B": Model("B")}
        self.prev_list = None         # the held list before this one (tail)
        self.last_count = None        # (count)
        self.plan_words = {"A": None, "B": None}      # name of the last accepted plan's fill value, per handle (stale_fill)
        self.shared_plan = None       # (which, name) of the last accepted CIGAR plan on either handle (leak)

    def effect(self, step):
        if self.first_effect is None:
            self.first_effect = step

    def call(self, which, entry, args, step):
        model = self.m[which]
        before = State()
        before.__dict__.update(model.s.__dict__)
        want, kind, _args = model.step(entry)
        out = dict(self.refs.get(want)) if want else None
        if want and "count" in out and entry != "filter":
            if self.defect == "tail" and (entry in PRODUCERS or entry == "b_hits") and which == "A":
                prev = self.prev_list
                if prev is not None and len(prev["index"]) > len(out["index"]):
                    n = len(out["index"])
                    for k in ("index", "q", "t", "f"):
                        out[k] = np.concatenate([out[k], prev[k][n:]])
                    out["count"] = np.asarray(len(out["index"]))
                    self.effect(step)
                self.prev_list = {k: np.asarray(out[k]) for k in ("index", "q", "t", "f")}
            self.last_count = int(out["count"])
        if want and entry == "filter" and self.defect == "count" and self.last_count is not None:
            if self.last_count != int(out["count"]):
                self.effect(step)
            out["count"] = np.asarray(self.last_count)
        if want and entry == "filter":
            self.last_count = int(out["count"])
        if want and entry in ("cigars", "b_scig", "b_pcig"):
            fill = {"cigars": "cigar_fill@" + str(before.held), "b_scig": "b_sfill@-", "b_pcig": None}[entry]
            self.plan_words[which] = fill
            self.shared_plan = (which, fill, entry)
        if entry == "cigar_fill" and self.defect == "stale_fill" and kind == "stale_plan" and self.plan_words["A"]:
            out = dict(self.refs.get(self.plan_words["A"]))
            self.effect(step)
        if entry in ("pf1", "pf2") and self.defect == "old_index" and kind == "no_index" and before.kmer_k:
            p = PREFILTERS[entry]
            idx, q, t, sh = prefilter_ref.prefilter(self.refs.a, before.kmer_k, 20, p["min_shared"], p["per"], p["block"])
            out = dict(count=len(idx), index=np.array(idx, dtype=np.uint64), q=np.array(q, dtype=np.uint32), t=np.array(t, dtype=np.uint32),
                       shared=np.array(sh, dtype=np.uint32))
            model.s.cand = LISTS[entry]
            self.effect(step)
        if entry == "b_sfill" and self.defect == "leak" and self.shared_plan and self.shared_plan[0] == "A":
            out = dict(self.refs.get(self.shared_plan[1]))
            self.effect(step)
        if out is None:
            return dict(status=np.asarray(INV), _untouched=True)
        out["status"] = np.asarray(0)
        return out

    def fresh(self, entry, pre, refs, args, want):
        return None                   # (a fresh fake has no history: it is the reference)


# ---------------------------------------------------------------- the GPU backend
def _marked(shape, dtype):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8).reshape(-1)[:] = MARK
    return a


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class GpuBackend:
    """The two handles on one context, every call through ctypes on buffers that start as MARK bytes and are sized from the expected
    value of the arguments' name (the caller's knowledge of what it asks for, never of what comes back: counts are read first)."""

    def __init__(self, seqs_a, recs_b):
        from aligner_amd import _ffi, runtime
        from aligner_amd.enums import DNA
        from aligner_amd.seqset import SeqSet
        assert _ffi.ERR_INVALID_ARGUMENT == INV
        self.ffi, self.runtime, self.lib = _ffi, runtime, _ffi.load()
        self.SeqSet, self.DNA = SeqSet, DNA
        self.sets = {"A": SeqSet(seqs_a), "B": SeqSet.stranded(recs_b, DNA)}
        self.n_b = len(recs_b)
        self.sch = schemes()
        self.seconds = 0.0
        self.score_chunks = {}        # per block of a score pass: the chunks its last run was cut into

    def close(self):
        for s in self.sets.values():
            s.close()

    def replace_a(self, seqs, derived_alive=True):
        """destroys A -- with a pair set derived from it alive, which is destroyed afterwards -- and makes A' from other records"""
        ss = self.sets["A"]
        blk = self.ffi.SeqsetBlock(*upper(0, 8), 0)
        st = C.c_int(0)
        ps = self.lib.aln_pairset_create_from_set(ss.handle, C.byref(blk), 0, 20, C.byref(st)) if derived_alive else None
        assert not derived_alive or (ps and st.value == 0)
        ss.close()
        self.sets["A"] = self.SeqSet(seqs)
        return ps

    def params(self, scheme, outputs=None):
        sem, m, d, e = self.sch[scheme]
        kw = {} if outputs is None else dict(outputs=outputs)
        return self.runtime.make_params(sem, d, e, m, blank=BLANK, **kw)

    def report_params(self, scheme):
        sem, m, _d, _e = self.sch[scheme]
        return self.runtime.make_params(sem, 0.0, 0.0, m, outputs=self.ffi.OUT_SCORE, blank=BLANK)

    def block(self, b):
        return self.ffi.SeqsetBlock(*b, 0)

    def stats(self, ss):
        ms, by = (C.c_double * 4)(), (C.c_uint64 * 2)()
        self.lib.aln_seqset_stats(ss.handle, ms, by)
        return int(by[0]), int(by[1])

    @staticmethod
    def count_out(count):
        """a count word as an output buffer: marker bytes while it holds the value it was given"""
        return _marked(1, np.uint64) if count.value == COUNT_MARK else np.zeros(1, dtype=np.uint64)

    def done(self, status, outs, extra=None):
        """status and outputs; of a refusal, whether every output still holds its marker"""
        got = dict(status=np.asarray(status))
        if status != 0:
            got["_error"] = (self.lib.aln_last_error() or b"").decode("utf-8", "replace")
            touched = [k for k, v in outs.items() if v is not None and v.size and not (v.view(np.uint8) == MARK).all()]
            got["_untouched"], got["_touched"] = not touched, ",".join(touched)
            return got
        got.update(outs)
        got.update(extra or {})
        return got

    def call(self, which, entry, args, step=None):
        import time
        t0 = time.perf_counter()
        try:
            return getattr(self, "do_" + self.ROUTE.get(entry, entry))(self.sets[which], entry, args)
        finally:
            self.seconds += time.perf_counter() - t0

    ROUTE = dict(hits_large="producer", hits_small="producer", best3="producer", hits_global="producer", score_large="score", score_row="score",
                 kmer2="kmer", kmer3="kmer", pf1="prefilter", pf2="prefilter", cigars="cigars", b_scig="cigars", b_pcig="cigars",
                 cluster_components="cluster", cluster_greedy="cluster")

    # ---- producers
    def held_list(self, ss, status, count):
        if status != 0:
            return self.done(status, dict(count=self.count_out(count)))
        n = int(count.value)
        outs = dict(count=np.asarray(n), index=_marked(min(n, 1 << 24), np.uint64), q=_marked(min(n, 1 << 24), np.uint32),
                    t=_marked(min(n, 1 << 24), np.uint32), f=_marked(min(n, 1 << 24), np.float64))
        if 0 < n <= 1 << 24:
            st = self.lib.aln_seqset_held_list(ss.handle, 0, n, outs["index"].ctypes.data, outs["q"].ctypes.data, outs["t"].ctypes.data, outs["f"].ctypes.data)
            if st != 0:
                return self.done(st, {})
        outs["f"] = bits(outs["f"])
        return self.done(0, outs)

    def do_producer(self, ss, entry, args):
        spec = PRODUCERS[entry]
        p, _keep = self.params(spec["scheme"])
        blk = self.block(spec["block"])
        count = C.c_uint64(COUNT_MARK)
        if "k" in spec:
            st = self.lib.aln_seqset_best(ss.handle, C.byref(p), C.byref(blk), spec["k"], float("-inf"), self.ffi.BEST_SKIP_SELF, C.byref(count))
        else:
            st = self.lib.aln_seqset_hits(ss.handle, C.byref(p), C.byref(blk), spec["f_min"], C.byref(count))
        return self.held_list(ss, st, count)

    def do_cand_hits(self, ss, entry, args):
        p, _keep = self.params("local")
        count = C.c_uint64(COUNT_MARK)
        return self.held_list(ss, self.lib.aln_seqset_candidate_hits(ss.handle, C.byref(p), PRODUCERS[entry]["f_min"], C.byref(count)), count)

    def do_b_hits(self, ss, entry, args):
        p, _keep = self.params("dna")
        blk = self.block(rect(0, self.n_b, 0, 2 * self.n_b))
        count = C.c_uint64(COUNT_MARK)
        return self.held_list(ss, self.lib.aln_seqset_hits(ss.handle, C.byref(p), C.byref(blk), strand_cases.F_MIN, C.byref(count)), count)

    def score(self, ss, scheme, block):
        p, _keep = self.params(scheme, self.ffi.OUT_SCORE)
        blk = self.block(block)
        n = len(block_pairs(block))
        f, status = _marked(n, np.float64), _marked(n, np.int32)
        st = self.lib.aln_seqset_score(ss.handle, C.byref(p), C.byref(blk), f.ctypes.data, status.ctypes.data)
        if st != 0:
            return self.done(st, dict(f=f, pair_status=status))
        # (12 bytes per pair and 16 per chunk come down: the chunks the pass ran in)
        self.score_chunks[block] = (self.stats(ss)[1] - 12 * n) // 16
        return self.done(0, dict(f=bits(f), pair_status=status))

    def do_score(self, ss, entry, args):
        return self.score(ss, "local", SCORES[entry])

    def do_b_score_minus(self, ss, entry, args):
        return self.score(ss, "dna", rect(0, self.n_b, self.n_b, self.n_b))

    # ---- indexes and lists
    def do_kmer(self, ss, entry, args):
        n_words = _marked(len(ss), np.uint32)
        return self.done(self.lib.aln_seqset_kmer_index(ss.handle, KMERS[entry], 20, n_words.ctypes.data), dict(n_words=n_words))

    def do_word5(self, ss, entry, args):
        n_words = _marked(len(ss), np.uint32)
        return self.done(self.lib.aln_seqset_word_index(ss.handle, WORD_K, 20, n_words.ctypes.data), dict(n_words=n_words))

    def cand_list(self, ss, status, count):
        if status != 0:
            return self.done(status, dict(count=self.count_out(count)))
        n = min(int(count.value), 1 << 24)
        outs = dict(count=np.asarray(int(count.value)), index=_marked(n, np.uint64), q=_marked(n, np.uint32), t=_marked(n, np.uint32), shared=_marked(n, np.uint32))
        if n:
            st = self.lib.aln_seqset_candidates(ss.handle, 0, n, outs["index"].ctypes.data, outs["q"].ctypes.data, outs["t"].ctypes.data, outs["shared"].ctypes.data)
            if st != 0:
                return self.done(st, {})
        return self.done(0, outs)

    def do_prefilter(self, ss, entry, args):
        p = PREFILTERS[entry]
        spec = self.ffi.PrefilterSpec(p["k"], 20, p["min_shared"], p["per"], 0, 0, 0)
        blk = self.block(p["block"])
        count = C.c_uint64(COUNT_MARK)
        return self.cand_list(ss, self.lib.aln_seqset_prefilter(ss.handle, C.byref(spec), C.byref(blk), C.byref(count)), count)

    def do_word_join(self, ss, entry, args):
        w = WORDJOIN
        spec = self.ffi.WordjoinSpec(w["k"], 20, w["min_shared"], w["per"], 0, 0, 0)
        blk = self.block(w["block"])
        count = C.c_uint64(COUNT_MARK)
        return self.cand_list(ss, self.lib.aln_seqset_word_join(ss.handle, C.byref(spec), C.byref(blk), C.byref(count)), count)

    # ---- consumers
    def do_strings(self, ss, entry, args):
        from aligner_amd.batch import RESULT_DTYPE
        keep, off = np.ascontiguousarray(args["_arg_keep"], dtype=np.uint32), np.ascontiguousarray(args["_arg_off"], dtype=np.uint64)
        # (the offsets are the expected hits': should other hits be held, a string may run past its place, by less than the slack)
        n_tb, slack = len(args["tb"]), 8192
        res, tb = _marked(len(keep), RESULT_DTYPE), _marked(n_tb + slack, np.uint8)
        st = self.lib.aln_seqset_held_strings(ss.handle, keep.ctypes.data, len(keep), res.ctypes.data, tb.ctypes.data, off.ctypes.data)
        if st != 0:
            return self.done(st, dict(res=res, tb=tb))
        out = dict(tb=tb[:n_tb], slack=tb[n_tb:])
        out.update({"res." + name: bits(np.ascontiguousarray(res[name])) for name in FIELDS})
        return self.done(0, out)

    def do_report(self, ss, entry, args):
        from aligner_amd.seqset import REPORT_DTYPE
        n = int(args["_arg_held"])
        keep = np.arange(n, dtype=np.uint32)
        p, _keep = self.report_params("local")     # (a report classes columns under the matrix alone: every protein scheme here is BLOSUM62's)
        rep = _marked(n, REPORT_DTYPE)
        st = self.lib.aln_seqset_held_report(ss.handle, C.byref(p), self.ffi.REPORT_SKIP_SEED, keep.ctypes.data, n, rep.ctypes.data)
        return self.done(st, dict(rep=rep)) if st != 0 else self.done(0, struct_fields("rep", rep))

    def do_filter(self, ss, entry, args):
        from aligner_amd.seqset import REPORT_DTYPE
        cap = int(args["_arg_held"])
        p, _keep = self.report_params("local")
        flt = self.ffi.HitFilter(MIN_IDENTITY, 0.0, 0.0, 0, 0)
        pos, rep, count = _marked(cap, np.uint32), _marked(cap, REPORT_DTYPE), C.c_uint64(COUNT_MARK)
        st = self.lib.aln_seqset_held_filter(ss.handle, C.byref(p), self.ffi.REPORT_SKIP_SEED, C.byref(flt), pos.ctypes.data, rep.ctypes.data, cap, C.byref(count))
        if st != 0:
            return self.done(st, dict(positions=pos, rep=rep))
        n = min(int(count.value), cap)
        out = dict(count=np.asarray(int(count.value)), positions=pos[:n])
        out.update(struct_fields("rep", rep[:n]))
        return self.done(0, out)

    def do_cluster(self, ss, entry, args):
        from aligner_amd import cluster as _cluster
        n = len(ss)
        label, rec, summ = _marked(n, np.uint32), _marked(n, _cluster.RECORD_DTYPE), self.ffi.ClusterSummary()
        mode = self.ffi.CLUSTER_COMPONENTS if entry == "cluster_components" else self.ffi.CLUSTER_GREEDY
        st = self.lib.aln_seqset_held_cluster(ss.handle, None, 0, None, mode, label.ctypes.data, rec.ctypes.data, n, C.byref(summ))
        if st != 0:
            return self.done(st, dict(label=label, records=rec))
        k = min(int(summ.clusters), n)
        out = dict(label=label, records=np.stack([rec[name][:k] for name in ("label", "size", "longest", "edges")], axis=1).reshape(-1, 4))
        out.update({"summary." + key: np.asarray(int(getattr(summ, key))) for key in ("nodes", "clusters", "edges", "self_edges", "singletons")})
        return self.done(0, out)

    def do_profiles(self, ss, entry, args):
        from aligner_amd import profile as _profile
        label, cen = np.ascontiguousarray(args["_arg_label"], dtype=np.uint32), np.ascontiguousarray(args["_arg_centers"], dtype=np.uint32)
        total = int(sum((N_CODES + 2) * int(ss.len[c]) for c in cen))
        out, rec, summ = _marked(total, np.uint32), _marked(len(cen), _profile.RECORD_DTYPE), self.ffi.ProfileSummary()
        st = self.lib.aln_seqset_held_profiles(ss.handle, None, self.ffi.PROFILE_SKIP_SEED, None, label.ctypes.data, _ptr(cen), len(cen), N_CODES, _ptr(out),
                                               len(out), _ptr(rec), C.byref(summ))
        if st != 0:
            return self.done(st, dict(out=out, records=rec))
        got = dict(out=out, records=np.stack([rec[name] for name in ("center", "hits", "matched", "deleted")], axis=1).reshape(-1, 4))
        got.update({"summary." + key: np.asarray(int(getattr(summ, key))) for key in profile_ref.SUMMARY_KEYS})
        return self.done(0, got)

    def do_msa(self, ss, entry, args):
        from aligner_amd import msa as _msa
        label, cen = np.ascontiguousarray(args["_arg_label"], dtype=np.uint32), np.ascontiguousarray(args["_arg_centers"], dtype=np.uint32)
        rec, summ = _marked(len(cen), _msa.RECORD_DTYPE), self.ffi.MsaSummary()
        st = self.lib.aln_seqset_held_msa_plan(ss.handle, None, 0, None, label.ctypes.data, _ptr(cen), len(cen), _ptr(rec), C.byref(summ))
        if st != 0:
            return self.done(st, dict(records=rec))
        out, row_hit = _marked(int(summ.bytes), np.uint8), _marked(int(summ.total_rows), np.uint32)
        st = self.lib.aln_seqset_held_msa_fill(ss.handle, _ptr(out), len(out), _ptr(row_hit), len(row_hit))
        if st != 0:
            return self.done(st, {})
        got = dict(out=out, row_hit=row_hit, records=np.stack([rec[name] for name in ("center", "rows", "width", "inserted")], axis=1).reshape(-1, 4))
        got.update({"summary." + key: np.asarray(int(getattr(summ, key))) for key in msa_ref.SUMMARY_KEYS})
        return self.done(0, got)

    def do_msa_fill(self, ss, entry, args):
        out, row_hit = _marked(int(args["_arg_bytes"]), np.uint8), _marked(int(args["_arg_rows"]), np.uint32)
        st = self.lib.aln_seqset_held_msa_fill(ss.handle, _ptr(out), len(out), _ptr(row_hit), len(row_hit))
        return self.done(st, dict(out=out, row_hit=row_hit))

    def do_cigars(self, ss, entry, args):
        from aligner_amd import cigar as _cigar
        n = int(args["_arg_held"])
        which = np.arange(n, dtype=np.uint32)
        rec, summ = _marked(n, _cigar.RECORD_DTYPE), self.ffi.CigarSummary()
        stranded = entry == "b_scig"
        strands = _marked(n, _cigar.STRAND_DTYPE) if stranded else None
        flags = CIGAR_FLAGS if entry == "cigars" else B_CIGAR_FLAGS
        if stranded:
            st = self.lib.aln_seqset_held_strand_cigar_plan(ss.handle, flags, _ptr(which), n, _ptr(rec), _ptr(strands), C.byref(summ))
        else:
            st = self.lib.aln_seqset_held_cigar_plan(ss.handle, flags, _ptr(which), n, _ptr(rec), C.byref(summ))
        if st != 0:
            return self.done(st, dict(records=rec, strands=strands))
        up, down = self.stats(ss)
        words, offsets = _marked(int(summ.total_ops), np.uint32), _marked(n + 1, np.uint64)
        fill = self.lib.aln_seqset_held_strand_cigar_fill if stranded else self.lib.aln_seqset_held_cigar_fill
        st = fill(ss.handle, _ptr(words), len(words), offsets.ctypes.data, len(offsets))
        if st != 0:
            return self.done(st, {})
        got = dict(records=np.stack([rec[name].astype(np.int64) for name in cigar_ref.RECORD_KEYS], axis=1).reshape(-1, 8), offsets=offsets, words=words,
                   bytes_up=np.asarray(up), bytes_down=np.asarray(down))
        if stranded:
            got["strands"] = np.stack([strands[name].astype(np.uint32) for name in strand_ref.STRAND_KEYS], axis=1).reshape(-1, 5)
        got.update({"summary." + key: np.asarray(int(getattr(summ, key))) for key in cigar_ref.SUMMARY_KEYS})
        return self.done(0, got)

    def fill(self, ss, args, stranded):
        words, offsets = _marked(int(args["_arg_total"]), np.uint32), _marked(int(args["_arg_n"]) + 1, np.uint64)
        fill = self.lib.aln_seqset_held_strand_cigar_fill if stranded else self.lib.aln_seqset_held_cigar_fill
        st = fill(ss.handle, _ptr(words), len(words), offsets.ctypes.data, len(offsets))
        return self.done(st, dict(words=words, offsets=offsets))

    def do_cigar_fill(self, ss, entry, args):
        return self.fill(ss, args, False)

    def do_b_sfill(self, ss, entry, args):
        return self.fill(ss, args, True)

    def do_signif(self, ss, entry, args):
        from aligner_amd.seqset import SIGNIF_RECORD_DTYPE
        keep = np.ascontiguousarray(args["_arg_keep"], dtype=np.uint32)
        scheme = "global" if int(args["_global"]) else "local"
        p, _keep = self.params(scheme, self.ffi.OUT_SCORE)
        spec = self.ffi.ShuffleSpec(SEED, 0, PER_PAIR, MAX_TRIM)
        rec, f, L = _marked(len(keep), SIGNIF_RECORD_DTYPE), _marked((len(keep), PER_PAIR), np.float64), _marked((len(keep), PER_PAIR), np.uint32)
        st = self.lib.aln_seqset_held_significance(ss.handle, C.byref(p), C.byref(spec), _ptr(keep), len(keep), _ptr(rec), _ptr(f), _ptr(L))
        if st != 0:
            return self.done(st, dict(rec=rec, f=f, lengths=L))
        got = dict(f=bits(f), lengths=L, bytes_down=np.asarray(self.stats(ss)[1]))
        got.update(struct_fields("rec", rec))
        return self.done(0, got)

    def fresh(self, entry, pre, refs, args, want):
        """the same call on a fresh handle of A's records after the prerequisites; None if it agrees with the reference"""
        keep = self.sets["A"]
        try:
            self.sets["A"] = self.SeqSet(refs.a)
            m = Model("A")
            for p, _ in pre:
                _w, _k, a = m.step(p)
                self.call("A", p, refs.get(a))
            return check(self.call("A", entry, refs.get(args)), refs.get(want) if want else None)
        except Exception as exc:      # (only ever part of a failure's message)
            return "error: %r" % (exc,)
        finally:
            self.sets["A"].close()
            self.sets["A"] = keep


# ---------------------------------------------------------------- the child process of tests/test_set_history_gpu.py
# python set_history.py expected.npz report.json: the whole walk in a context of its own (under the parent's environment knobs),
# every call held against the expected values the parent computed from the oracle; the parent asserts on the report.
def main(argv):
    import json
    import time
    expected, report = argv
    refs = Refs(set_a(), set_b()).load(expected)
    backend = GpuBackend(refs.a, refs.recs_b)
    t0 = time.perf_counter()
    out = walk(backend, refs)
    out["seconds"] = time.perf_counter() - t0
    out["score_chunks"] = int(backend.score_chunks.get(BIG, 0))
    backend.close()
    with open(report, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1:])
