"""Every exported family called through include/aligner_hip.h from C99 (tests/abi_families.c), on the GPU.

The C program is run ONCE, in a child process, on a case file written here; its printout is parsed once and compared, family by
family and bit for bit, with references that never touch the library: the CPU oracle (summaries, strings, scores of shuffled copies),
tests/seqset_ref.py (pair order), a sort by the stated rule (k best), tests/report_ref.py, tests/shuffle_ref.py, tests/signif_ref.py,
tests/transform_ref.py, numpy on oracle scores (scan selections) and tests/set_loop_cases.py (the loop).  The same calls through the
Python wrappers (ctypes) must give what the C caller got.  Timings and byte counters are checked for call status and sign only.

Sizes: nine protein sequences of 1 .. 513 residues (one with a code outside the matrix), a 3 000-residue DNA string scanned in 600
windows by two 4 x 12 matrices, 65 shuffled copies per pair or hit."""
import collections
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import report_ref  # noqa: E402
import seqset_ref  # noqa: E402
import set_loop_cases  # noqa: E402
import shuffle_ref  # noqa: E402
import signif_ref  # noqa: E402
import transform_ref  # noqa: E402
from aligner_amd import _ffi  # noqa: E402
from aligner_amd.enums import Protein  # noqa: E402

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, CAPACITY = _ffi.OK, _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED, _ffi.ERR_CAPACITY
LOCAL, GLOBAL, REAL = (11.0, 2.0), (4.0, 4.0), (11.3, 2.1)
LENGTHS = (1, 2, 7, 63, 64, 65, 130, 513)
BAD = 8                                              # the sequence with a code outside the matrix
NSEQ = 9
F_MIN = 20.0
BEST_K, BEST_F_MIN = 3, 1.0
FILTER = dict(min_identity=0.5, min_q_cover=0.5, min_t_cover=0.2, min_columns=10)
SHUFFLE = dict(seed=0x5EED0AB1, pair_base=700, per_pair=65, max_trim=6)
SIGNIF = dict(seed=0xAB1F00D, pair_base=1000, per_pair=65, max_trim=6)
SCAN_LEN, SCAN_FIRST, SCAN_STEP, SCAN_WIDTH, SCAN_COLS, SCAN_GAPS, SCAN_Z, SCAN_CAP = 3000, 0, 5, 40, 12, (5.0, 2.0), 2.0, 96
SCAN_TAGS = ("int.fwd", "int.rev", "real.fwd", "real.rev")
BATCH_PAIRS = seqset_ref.generate_pairs(0, NSEQ)
SHUFFLE_PAIRS = [(4, 5), (3, 6), (2, 3)]
PAIRSET_PAIRS = [(4, 5), (3, 6), (2, 3), (6, 7), (BAD, 4), (0, 1)]
PAIRSET_ACTIVE = [5, 0, 2, 4, 1, 3]
PAIRSET_WHICH = [3, 4, 0, 5, 1, 2]
RECT = (2, 4, 3, 6)                                  # q_first q_count t_first t_count: starts at neither 0


def bits(x):
    return np.atleast_1d(np.asarray(x, dtype=np.float64)).view(np.uint64).tolist()


# ---------------------------------------------------------------- the inputs, from fixed seeds
def sequences(S):
    """Eight proteins of LENGTHS -- the longer ones mutated pieces of one 513-residue ancestor whose first seven residues are the four
    with the highest self-score, the three shortest its first 1, 2, 7 residues -- and one of 40 residues holding code 30."""
    rng = np.random.default_rng(20261019)
    top = np.argsort(-np.diag(S)[:20], kind="stable")[:4]
    anc = rng.integers(0, 20, 513).astype(np.uint8)
    anc[:7] = top[[0, 1, 0, 2, 0, 3, 1]]
    seqs = []
    for L in LENGTHS:
        s = anc[:L].copy()
        if 7 < L < 513:
            mut = rng.random(L) < 0.25
            s[mut] = rng.integers(0, 20, int(mut.sum()))
            s[:7] = anc[:7]
        seqs.append(s)
    bad = anc[100:140].copy()
    bad[17] = 30
    seqs.append(bad)
    return seqs


def scan_inputs():
    rng = np.random.default_rng(77)
    seq = rng.integers(0, 4, SCAN_LEN).astype(np.uint8)
    motif = rng.integers(0, 4, SCAN_COLS).astype(np.uint8)
    for at in (103, 611, 1200, 1777, 2402, 2970, 2991):                # the last two lie in truncated windows; 2991 is cut short itself
        m = motif.copy()
        m[int(rng.integers(0, SCAN_COLS))] = rng.integers(0, 4)
        n = min(SCAN_COLS, SCAN_LEN - at)
        seq[at:at + n] = m[:n]
    pwm_int = rng.integers(-3, 1, size=(4, SCAN_COLS)).astype(np.float64)
    pwm_int[motif, np.arange(SCAN_COLS)] = 3.0
    pwm_real = pwm_int * 0.37 + rng.normal(0.0, 0.1, size=(4, SCAN_COLS))
    return seq, pwm_int, pwm_real


def scan_windows():
    starts = np.arange(SCAN_FIRST, SCAN_LEN, SCAN_STEP)
    return starts, np.minimum(starts + SCAN_WIDTH, SCAN_LEN) - starts


def transform_inputs(S):
    rng = np.random.default_rng(5)
    m = np.stack([S, 0.37 * S + 0.013, S + rng.normal(0, 0.5, S.shape), 0.37 * S + 0.013])
    return m, rng.dirichlet(np.ones(24), 4), np.array([-0.5, -1.0, -0.2, -0.5]), np.array([576.0, 576.0, 100.0, 1e-9])     # the last: no root


def pairset_heuristics():
    rng = np.random.default_rng(9)
    n = len(PAIRSET_PAIRS)
    return rng.dirichlet(np.ones(24), n), rng.choice([-0.2, -0.5, -1.0], n), np.full(n, 576.0)


def loop_heuristics(seqs):
    fr, kd, r2 = [], [], []
    for q, t in BATCH_PAIRS:
        c = seqs[t][seqs[t] < 24]
        fr.append(np.bincount(c, minlength=24).astype(np.float64) / max(len(seqs[t]), 1))
        kd.append([-0.2, -0.5, -1.0][(q + 2 * t) % 3])
        r2.append(0.0 if (q + t) % 4 == 0 else 576.0)
    return np.array(fr), np.array(kd), np.array(r2)


class Case:
    """The inputs and the oracle's answers the inputs themselves depend on (scan thresholds, the positions whose significance is asked)."""

    def __init__(self, S, orc):
        self.S, self.R, self.orc = S, 0.37 * S + 0.013, orc
        self.seqs = sequences(S)
        self.len = np.array([len(s) for s in self.seqs], dtype=np.uint64)
        self.scan_seq, self.pwm_int, self.pwm_real = scan_inputs()
        self.memo = {}
        # the scan: oracle f of every window of the four passes; mean and sd of each are the pass's thresholds
        starts, lens = scan_windows()
        self.scan = {}
        for tag in SCAN_TAGS:
            pwm = self.pwm_int if tag.startswith("int") else self.pwm_real
            strand = self.scan_seq[::-1].copy() if tag.endswith("rev") else self.scan_seq
            wins = [orc.align_pwm(strand[int(s):int(s + n)], SCAN_GAPS[0], SCAN_GAPS[1], pwm) for s, n in zip(starts, lens)]
            assert all(w["status"] == 0 for w in wins), tag
            f = np.array([w["f"] for w in wins])
            mean, sd = float(np.mean(f)), float(np.std(f))
            hits = np.flatnonzero((f - mean) / sd >= SCAN_Z)
            assert 3 < len(hits) <= SCAN_CAP, (tag, len(hits))
            assert tag.endswith("rev") or (lens[hits] < SCAN_WIDTH).any(), tag                          # a truncated window is among the hits
            self.scan[tag] = dict(pwm=pwm, wins=wins, f=f, mean=mean, sd=sd, hits=hits, lens=lens)
        self.m_transform, self.fr_transform, self.kd_transform, self.r2_transform = transform_inputs(S)
        self.pairset_matrices = np.stack([self.R + 0.001 * k for k in range(len(PAIRSET_ACTIVE))])
        self.pairset_fr, self.pairset_kd, self.pairset_r2 = pairset_heuristics()
        first = {PAIRSET_ACTIVE[k]: self.align(PAIRSET_PAIRS[PAIRSET_ACTIVE[k]], orc.CORE_LOCAL, REAL, self.pairset_matrices[k]) for k in range(len(PAIRSET_ACTIVE))}
        self.pairset_first = first
        self.pairset_reest = [i for i in PAIRSET_WHICH if first[i]["status"] == 0]
        assert BAD in PAIRSET_PAIRS[4] and first[4]["status"] == orc.ERR_CODE_OUT_OF_RANGE and len(self.pairset_reest) >= 4
        self.loop_fr, self.loop_kd, self.loop_r2 = loop_heuristics(self.seqs)
        # the k best of the whole grid (the oracle's f sorted by the stated rule) and the positions whose significance is asked
        self.best = self.best_list()
        ok = [k for k, (q, t, f) in enumerate(self.best) if len(self.seqs[t]) >= SIGNIF["max_trim"]]
        big = [k for k in ok if len(self.seqs[self.best[k][1]]) == 513][:1]         # one 513-residue target: two strips
        chosen = sorted(set(np.array(ok)[np.linspace(0, len(ok) - 1, 7).astype(int)].tolist() + big))
        self.signif_keep = chosen[::-1] + [chosen[0]]                            # any order, one position twice; at most nine
        assert any(len(self.seqs[self.best[k][1]]) == 513 for k in self.signif_keep)

    def align(self, pair, sem, gaps, matrix, key=None):
        q, t = pair
        k = (q, t, sem, gaps, key)
        if key is None or k not in self.memo:
            r = self.orc.align(sem, self.seqs[q], self.seqs[t], gaps[0], gaps[1], matrix)
            if key is None:
                return r
            self.memo[k] = r
        return self.memo[k]

    def local(self, q, t):
        return self.align((q, t), self.orc.CORE_LOCAL, LOCAL, self.S, "b62")

    def best_list(self):
        out = []
        for q in range(NSEQ):
            cand = [(t, self.local(q, t)["f"]) for t in range(NSEQ) if t != q and self.local(q, t)["status"] == 0]
            cand = [(t, f) for t, f in cand if f == f and f >= BEST_F_MIN]
            cand.sort(key=lambda c: (-c[1], c[0]))                                  # higher f first, equal f by the earlier record
            out += [(q, t, f) for t, f in sorted(cand[:BEST_K])]
        return out

    def write(self, path):
        seq_txt = lambda a: " ".join(str(int(v)) for v in np.asarray(a).ravel())           # noqa: E731
        hex_txt = lambda a: " ".join("%016x" % v for v in bits(np.asarray(a, dtype=np.float64).ravel()))   # noqa: E731
        pairs_txt = lambda ps: seq_txt([v for p in ps for v in p])                      # noqa: E731
        rec = []

        def ints(key, a):
            a = np.atleast_1d(np.asarray(a)).ravel()
            rec.append("%s %d %s" % (key, len(a), seq_txt(a)))

        def f64s(key, a):
            a = np.atleast_1d(np.asarray(a, dtype=np.float64)).ravel()
            rec.append("%s %d %s" % (key, len(a), hex_txt(a)))

        f64s("matrix_b62", self.S); f64s("matrix_real", self.R); f64s("gaps", LOCAL + GLOBAL + REAL)
        ints("refusals", [UNSUPPORTED, UNSUPPORTED, INVALID, CAPACITY])
        ints("set_len", self.len); ints("set_codes", np.concatenate(self.seqs))
        rec.append("batch_pairs %d %s" % (2 * len(BATCH_PAIRS), pairs_txt(BATCH_PAIRS)))
        ints("scan_seq", self.scan_seq); ints("scan_geom", [SCAN_FIRST, SCAN_STEP, SCAN_WIDTH])
        f64s("scan_pwm_int", self.pwm_int); f64s("scan_pwm_real", self.pwm_real); f64s("scan_gaps", SCAN_GAPS)
        f64s("scan_select", [v for tag in SCAN_TAGS for v in (self.scan[tag]["mean"], self.scan[tag]["sd"], SCAN_Z)])
        ints("scan_cap", [SCAN_CAP])
        rec.append("shuffle_pairs %d %s" % (2 * len(SHUFFLE_PAIRS), pairs_txt(SHUFFLE_PAIRS)))
        ints("shuffle_spec", [SHUFFLE["seed"], SHUFFLE["pair_base"], SHUFFLE["per_pair"], SHUFFLE["max_trim"]])
        ints("transform_n", [len(self.m_transform)]); f64s("transform_matrices", self.m_transform); f64s("transform_freq", self.fr_transform)
        f64s("transform_kd", self.kd_transform); f64s("transform_r2", self.r2_transform)
        rec.append("pairset_pairs %d %s" % (2 * len(PAIRSET_PAIRS), pairs_txt(PAIRSET_PAIRS)))
        ints("pairset_active", PAIRSET_ACTIVE); f64s("pairset_matrices", self.pairset_matrices); ints("pairset_which", PAIRSET_WHICH)
        f64s("pairset_freq", self.pairset_fr); f64s("pairset_kd", self.pairset_kd); f64s("pairset_r2", self.pairset_r2)
        ints("pairset_reestimate", self.pairset_reest)
        ints("set_rect", RECT); f64s("set_fmin", [F_MIN])
        f64s("set_filter", [FILTER["min_identity"], FILTER["min_q_cover"], FILTER["min_t_cover"]]); ints("set_filter_columns", [FILTER["min_columns"]])
        ints("best_k", [BEST_K]); f64s("best_fmin", [BEST_F_MIN]); ints("signif_keep", self.signif_keep)
        ints("signif_spec", [SIGNIF["seed"], SIGNIF["pair_base"], SIGNIF["per_pair"], SIGNIF["max_trim"]])
        f64s("loop_freq", self.loop_fr); f64s("loop_kd", self.loop_kd); f64s("loop_r2", self.loop_r2)
        with open(path, "w") as fp:
            fp.write("\n".join(rec) + "\n")


@pytest.fixture(scope="module")
def case(blosum62, orc):
    return Case(blosum62, orc)


# ---------------------------------------------------------------- the one run of the C program, parsed once
class Printout:
    def __init__(self, text):
        self.lines = collections.defaultdict(list)
        for line in text.splitlines():
            w = line.split()
            if w:
                self.lines[w[0]].append(w[1:])

    def one(self, key):
        assert len(self.lines[key]) == 1, key
        return self.lines[key][0]

    def ints(self, key):
        return [int(v) for v in self.one(key)]

    def f64(self, key):
        return [int(v.split("/")[0], 16) for v in self.one(key)]

    def rc(self, label):
        got = [w for w in self.lines["rc"] if w[0] == label]
        assert len(got) == 1, label
        return int(got[0][1])

    def indexed(self, key):
        """the lines `<key> <k> ...`, k = 0, 1, .. in order, without k"""
        rows = self.lines[key]
        assert [int(r[0]) for r in rows] == list(range(len(rows))), key
        return [r[1:] for r in rows]

    def results(self, key):
        """[dict of SUMMARY + passes, flags]; f and score as bits"""
        out = []
        for r in self.indexed(key):
            d = dict(status=int(r[0]), f=int(r[1].split("/")[0], 16), score=int(r[2].split("/")[0], 16))
            d.update(zip(("end_y", "end_x", "start_y", "start_x", "aln_len", "passes", "flags"), (int(v) for v in r[3:])))
            out.append(d)
        return out

    def strings(self, key):
        q, t = self.indexed(key + "_q"), self.indexed(key + "_t")
        return [([int(v) for v in a], [int(v) for v in b]) for a, b in zip(q, t)]


@pytest.fixture(scope="module")
def run(case, tmp_path_factory):
    from aligner_amd import build as native_build
    exe = native_build.build_families_harness()
    path = tmp_path_factory.mktemp("abi_families") / "case.txt"
    case.write(str(path))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    p = Printout(out.stdout)
    p.returncode, p.text, p.stderr = out.returncode, out.stdout, out.stderr
    return p


def summary_of(o):
    """an oracle answer as the summary fields (f and score as bits)"""
    d = dict(status=o["status"])
    if o["status"] == 0:
        d.update(f=bits(o["f"])[0], score=bits(o["score"])[0], end_y=o["end"][0], end_x=o["end"][1], start_y=o["start"][0], start_x=o["start"][1])
        d["aln_len"] = len(o["qa"] if "qa" in o else o["numbered"])
    return d


def same_summaries(got, want):
    """status always; every other field where the reference succeeded (a failed pair's other fields are not specified)"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert {key: g[key] for key in w} == w, k


def same_strings(got, want_orc):
    assert len(got) == len(want_orc)
    for k, (g, o) in enumerate(zip(got, want_orc)):
        if o["status"] == 0:
            assert g == (o["qa"].tolist(), o["ta"].tolist()), k
        else:
            assert g == ([], []), k


def from_dtype(res):
    """RESULT_DTYPE records as the printout's dicts"""
    out = []
    for r in res:
        d = {k: int(r[k]) for k in ("status", "end_y", "end_x", "start_y", "start_x", "aln_len", "flags")}
        d["f"], d["score"] = bits(r["f"])[0], bits(r["score"])[0]
        out.append(d)
    return out


def same_as_wrapper(got, res):
    want = from_dtype(res)
    assert [{k: g[k] for k in w} for g, w in zip(got, want)] == want and len(got) == len(want)


# ---------------------------------------------------------------- the run as a whole
def test_every_call_returned_what_the_case_expects(run):
    assert run.returncode == 0, run.text[-4000:] + run.stderr[-2000:]
    assert run.one("done") == ["bad", "0"]
    assert run.one("guards")[1:] == ["damaged", "0"] and int(run.one("guards")[0]) > 100        # no buffer of the documented size was overrun
    assert all(w[1] == w[2] for w in run.lines["rc"]) and len(run.lines["rc"]) > 70
    assert "unexpected" not in run.lines and "guard_damaged" not in run.lines
    assert run.one("abi_version_header") == run.one("abi_version_library") == ["2"]


def test_refusals(run):
    assert run.rc("refusal.scan_semantics") == UNSUPPORTED and run.one("refusal.scan_semantics.sentinel") == ["1"]
    assert run.rc("refusal.best_upper") == UNSUPPORTED and run.one("refusal.best_upper.sentinel") == ["1"]
    assert run.rc("refusal.strings_before_run") == INVALID and run.one("refusal.strings_before_run.sentinel") == ["1"]
    assert run.rc("refusal.select_capacity") == CAPACITY


def test_select_over_capacity_reports_the_true_count(run, case):
    count, sentinel = run.one("refusal.select_capacity.count")[0], run.one("refusal.select_capacity.count")[2]
    assert int(count) == len(case.scan["int.fwd"]["hits"]) and sentinel == "1"


def test_context(run):
    from aligner_amd import runtime
    info = runtime.device_info()
    d = re.search(r"^device compute_units (\d+) hbm_bytes (\d+) name (.*)$", run.text, flags=re.M)
    assert int(d.group(1)) == info["compute_units"] > 0 and int(d.group(2)) == info["hbm_bytes"] > 0
    # the name's first part is the marketing name the driver looks up per process (it can be empty in one and not in another on the same
    # device); the part in parentheses is the architecture the library appends
    arch = info["name"][info["name"].rindex("("):]
    assert arch.startswith("(gfx") and d.group(3).endswith(arch)
    assert run.one("devices") == ["1", "second", "1"]


def test_plan_chunks(run, case):
    import ctypes as C
    n = len(BATCH_PAIRS)
    k = int(run.one("plan.chunks")[0])
    first, count = run.ints("plan.first"), run.ints("plan.count")
    assert 1 <= k <= n and len(first) == k
    assert first[0] == 0 and all(first[i] + count[i] == (first + [n])[i + 1] for i in range(k))           # ranges of the caller's order
    q_len = np.array([case.len[q] for q, t in BATCH_PAIRS], dtype=np.uint64)
    t_len = np.array([case.len[t] for q, t in BATCH_PAIRS], dtype=np.uint64)
    p, _keep = runtime_params(_ffi.CORE_LOCAL, LOCAL, case.S)
    a, b = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    assert _ffi.load().aln_plan_chunks(C.byref(p), q_len.ctypes.data, t_len.ctypes.data, n, 1, a.ctypes.data, b.ctypes.data, n) == k
    assert a[:k].tolist() == first and b[:k].tolist() == count


def runtime_params(sem, gaps, matrix, **kw):
    from aligner_amd import runtime
    return runtime.make_params(sem, gaps[0], gaps[1], matrix, **kw)


# ---------------------------------------------------------------- staged batch
def test_staged_batch(run, case):
    from aligner_amd.batch import PairBatch, StagedBatch
    want = [case.local(q, t) for q, t in BATCH_PAIRS]
    got = run.results("batch.res")
    same_summaries(got, [summary_of(o) for o in want])
    same_strings(run.strings("batch.str"), want)
    assert {o["status"] for o in want} >= {0, case.orc.ERR_CODE_OUT_OF_RANGE}
    assert run.one("batch.timing_values")[:2] == ["nonnegative", "1"]
    facts = run.one("batch.cells")
    cells, size, dir_bytes, dev = int(facts[0]), int(facts[2]), int(facts[4]), int(facts[6])
    assert size == len(BATCH_PAIRS) and dev == 1
    sb = StagedBatch(PairBatch.from_pairs([(case.seqs[q], case.seqs[t]) for q, t in BATCH_PAIRS]), _ffi.CORE_LOCAL, 11.0, 2.0, case.S,
                     outputs=_ffi.OUT_SCORE | _ffi.OUT_TRACEBACK)
    try:
        sb.run(); sb.sync()
        res = sb.fetch()
        assert (cells, dir_bytes) == (sb.cells, sb.direction_bytes)
        same_as_wrapper(got, res.results)
        for i, o in enumerate(want):
            if o["status"] == 0:
                qa, ta = res.aligned(i)
                assert (qa.tolist(), ta.tolist()) == run.strings("batch.str")[i]
    finally:
        sb.close()
    ok = sum(int(case.len[q] * case.len[t]) for (q, t), o in zip(BATCH_PAIRS, want) if o["status"] == 0)
    assert ok <= cells <= sum(int(case.len[q] * case.len[t]) for q, t in BATCH_PAIRS)


# ---------------------------------------------------------------- window scan
def pwm_counts(wins, cols):
    out = np.zeros((4, cols))
    for w in wins:
        for col, c in zip(w["numbered"].tolist(), w["qal"].tolist()):
            if col != 0 and c != 98:
                out[c, col - 1] += 1.0
    return out


@pytest.mark.parametrize("tag", SCAN_TAGS)
def test_scan(run, case, tag):
    from aligner_amd import repeats as R
    sc = case.scan[tag]
    key = "scan.%s." % tag
    n = len(sc["f"])
    stride = int(run.one(key + "windows")[2])
    assert int(run.one(key + "windows")[0]) == n == 600 and stride >= 5 * (SCAN_COLS + SCAN_WIDTH + 2)
    assert run.f64(key + "f") == bits(sc["f"])
    hits = sc["hits"].tolist()
    # select
    assert run.ints(key + "select_count") == [len(hits)] and run.ints(key + "select_idx") == hits
    want = [sc["wins"][k] for k in hits]
    same_summaries(run.results(key + "select_res"), [summary_of(o) for o in want])
    assert [[int(v) for v in r] for r in run.indexed(key + "select_num")] == [o["numbered"].tolist() for o in want]
    assert [[int(v) for v in r] for r in run.indexed(key + "select_seq")] == [o["qal"].tolist() for o in want]
    # the held pass and its fetches: keep = the list backwards and position 0 again
    keep = list(range(len(hits)))[::-1] + [0]
    assert run.ints(key + "held_count") == [len(hits)] and run.ints(key + "held_idx") == hits
    assert run.f64(key + "held_f") == bits(sc["f"][hits])
    kept = [want[k] for k in keep]
    assert run.f64(key + "held_counts") == bits(pwm_counts(kept, SCAN_COLS).ravel())
    same_summaries(run.results(key + "held_res"), [summary_of(o) for o in kept])
    assert [[int(v) for v in r] for r in run.indexed(key + "held_num")] == [o["numbered"].tolist() for o in kept]
    assert [[int(v) for v in r] for r in run.indexed(key + "held_seq")] == [o["qal"].tolist() for o in kept]
    for s in ("select_stats", "held_stats"):
        assert run.one(key + s)[:2] == ["nonnegative", "1"]
    # the same calls through the Python classes
    reverse = tag.endswith("rev")
    with R.ScanBackend().scan(case.scan_seq) as gs:
        assert run.f64(key + "f") == bits(gs.score(sc["pwm"], SCAN_GAPS[0], SCAN_GAPS[1], SCAN_FIRST, SCAN_STEP, SCAN_WIDTH, reverse=reverse))
        idx, res, tb, count, pstride, st = gs.select_raw(sc["pwm"], SCAN_GAPS[0], SCAN_GAPS[1], SCAN_FIRST, SCAN_STEP, SCAN_WIDTH, sc["mean"], sc["sd"], SCAN_Z,
                                                         reverse=reverse, cap=SCAN_CAP)
        assert (st, count, pstride) == (OK, len(hits), stride) and idx[:count].tolist() == hits
        same_as_wrapper(run.results(key + "select_res"), res[:count])
        held = gs.hits(sc["pwm"], SCAN_GAPS[0], SCAN_GAPS[1], SCAN_FIRST, SCAN_STEP, SCAN_WIDTH, sc["mean"], sc["sd"], SCAN_Z, reverse=reverse)
        assert held.idx.tolist() == hits and bits(held.f) == run.f64(key + "held_f")
        assert bits(held.frequencies(keep).ravel()) == run.f64(key + "held_counts")
        hs = held.strings(keep)
        same_as_wrapper(run.results(key + "held_res"), hs.res)
        alns = hs.alignments()
        assert [a.numbered.tolist() for a in alns] == [[int(v) for v in r] for r in run.indexed(key + "held_num")]


# ---------------------------------------------------------------- shuffled copies
@pytest.fixture(scope="module")
def shuffled(case):
    """[(copies, lengths, oracle answers)] per pair, by tests/shuffle_ref.py and the oracle on those copies"""
    out = []
    for i, (q, t) in enumerate(SHUFFLE_PAIRS):
        copies = [shuffle_ref.copy_of(case.seqs[t], SHUFFLE["seed"], SHUFFLE["pair_base"] + i, s, SHUFFLE["max_trim"])[1] for s in range(SHUFFLE["per_pair"])]
        out.append((copies, [case.orc.align(case.orc.CORE_LOCAL, case.seqs[q], c, LOCAL[0], LOCAL[1], case.S) for c in copies]))
    return out


def test_shuffle(run, case, shuffled):
    from aligner_amd import statistics
    per = SHUFFLE["per_pair"]
    rows = run.lines["shuffle.copies"]
    assert [int(r[0]) for r in rows] == list(range(len(SHUFFLE_PAIRS)))
    f, lengths, status = [], [], []
    for i, (q, t) in enumerate(SHUFFLE_PAIRS):
        L = int(case.len[t])
        got = np.array([int(v) for v in rows[i][2:]], dtype=np.uint8).reshape(per, L)
        assert int(rows[i][1]) == L
        copies, answers = shuffled[i]
        for s in range(per):
            assert got[s].tolist() == copies[s].tolist() + [0] * (L - len(copies[s])), (i, s)
        assert {len(c) for c in copies} == set(range(L - SHUFFLE["max_trim"], L + 1))                   # every trim was drawn
        assert all(o["status"] == 0 for o in answers)
        f += [o["f"] for o in answers]
        lengths += [len(c) for c in copies]
        status.append(0)
    assert run.f64("shuffle.f") == bits(f) and run.ints("shuffle.lengths") == lengths and run.ints("shuffle.status") == status
    pf, pl, ps = statistics.device_shuffled_scores([(case.seqs[q], case.seqs[t]) for q, t in SHUFFLE_PAIRS], LOCAL[0], LOCAL[1], case.S, SHUFFLE["seed"],
                                                   per_pair=per, max_trim=SHUFFLE["max_trim"], pair_base=SHUFFLE["pair_base"])
    assert bits(pf.ravel()) == run.f64("shuffle.f") and pl.ravel().tolist() == lengths and ps.tolist() == status
    pc, _ = statistics.shuffle_targets([case.seqs[t] for q, t in SHUFFLE_PAIRS], SHUFFLE["seed"], per_pair=per, max_trim=SHUFFLE["max_trim"],
                                       pair_base=SHUFFLE["pair_base"])
    for i in range(len(SHUFFLE_PAIRS)):
        assert pc[i].ravel().tolist() == [int(v) for v in rows[i][2:]]


# ---------------------------------------------------------------- transforms
def ref_transform(m, fr, kd, r2):
    st, out, _branch = transform_ref.transform([float(v) for v in np.asarray(m).ravel()], 24, 24, [float(v) for v in fr], float(kd), float(r2))
    return st, out


def test_transforms(run, case):
    from aligner_amd.pairset import transform_matrices, transform_matrices_device
    n = len(case.m_transform)
    want = [ref_transform(case.m_transform[i], case.fr_transform[i], case.kd_transform[i], case.r2_transform[i]) for i in range(n)]
    assert [w[0] for w in want] == [0, 0, 0, transform_ref.NO_ROOT]
    host, hst = transform_matrices(case.m_transform, case.fr_transform, case.kd_transform, case.r2_transform)
    dev, dst = transform_matrices_device(case.m_transform, case.fr_transform, case.kd_transform, case.r2_transform)
    for where, pm, pst in (("host", host, hst), ("device", dev, dst)):
        assert run.ints("transform.%s_status" % where) == [w[0] for w in want] == pst.tolist()
        rows = run.lines["transform.%s_out" % where]
        assert [int(r[0]) for r in rows] == list(range(n))
        for i, (st, out) in enumerate(want):
            got = [int(v.split("/")[0], 16) for v in rows[i][2:]]
            if st == 0:
                assert rows[i][1] == "0" and got == bits(out) == bits(pm[i].ravel()), (where, i)
            else:
                assert rows[i][1] == "1", (where, i)                                    # left as it was: still the sentinel


# ---------------------------------------------------------------- pair set
@pytest.fixture(scope="module")
def pairset_truth(case):
    """the store after both re-estimations and the oracle's answers under it"""
    orc = case.orc
    first = case.pairset_first
    counts = {i: (orc.frequency_matrix(o["qa"], o["ta"], 24) if o["status"] == 0 else np.zeros((24, 24))) for i, o in first.items()}
    store, shared_status, held_status = {}, [], []
    for i in PAIRSET_WHICH:
        st, out = ref_transform(case.R, case.pairset_fr[i], case.pairset_kd[i], case.pairset_r2[i])
        shared_status.append(st)
        store[i] = np.array(out).reshape(24, 24)
    for i in case.pairset_reest:
        st, out = ref_transform(counts[i], case.pairset_fr[i], case.pairset_kd[i], case.pairset_r2[i])
        held_status.append(st)
        if st == 0:
            store[i] = np.array(out).reshape(24, 24)
    assert all(np.isfinite(m).all() for m in store.values())
    second = {i: case.align(PAIRSET_PAIRS[i], orc.CORE_LOCAL, REAL, store[i]) for i in PAIRSET_ACTIVE}
    return dict(first=first, counts=counts, store=store, shared_status=shared_status, held_status=held_status, second=second)


def test_pairset(run, case, pairset_truth):
    from aligner_amd.pairset import PairSet
    T = pairset_truth
    same_summaries(run.results("pairset.run_res"), [summary_of(T["first"][i]) for i in PAIRSET_ACTIVE])
    got_counts = [[int(v) for v in r] for r in run.indexed("pairset.counts")]
    assert got_counts == [T["counts"][i].astype(np.int64).ravel().tolist() for i in PAIRSET_WHICH]
    same_summaries(run.results("pairset.str_res"), [summary_of(T["first"][i]) for i in PAIRSET_WHICH])
    same_strings(run.strings("pairset.str"), [T["first"][i] for i in PAIRSET_WHICH])
    assert run.one("pairset.stats")[:2] == ["nonnegative", "1"]
    assert run.ints("pairset.reestimate_shared_status") == T["shared_status"] == [0] * len(PAIRSET_WHICH)
    assert run.ints("pairset.reestimate_held_status") == T["held_status"]
    got_store = [[int(v.split("/")[0], 16) for v in r] for r in run.indexed("pairset.store")]
    assert got_store == [bits(T["store"][i].ravel()) for i in PAIRSET_WHICH]
    same_summaries(run.results("pairset.stored_res"), [summary_of(T["second"][i]) for i in PAIRSET_ACTIVE])
    same_summaries(run.results("pairset.stored_str_res"), [summary_of(T["second"][i]) for i in PAIRSET_WHICH])
    same_strings(run.strings("pairset.stored_str"), [T["second"][i] for i in PAIRSET_WHICH])
    # the same calls through PairSet
    with PairSet([(case.seqs[q], case.seqs[t]) for q, t in PAIRSET_PAIRS]) as ps:
        same_as_wrapper(run.results("pairset.run_res"), ps.run(_ffi.CORE_LOCAL, REAL[0], REAL[1], case.pairset_matrices, PAIRSET_ACTIVE))
        assert [c.ravel().tolist() for c in ps.frequencies(PAIRSET_WHICH)] == got_counts
        res, strs = ps.strings(PAIRSET_WHICH)
        same_as_wrapper(run.results("pairset.str_res"), res)
        assert [(a.tolist(), b.tolist()) for a, b in strs] == run.strings("pairset.str")
        ps.set_heuristics(24, 24, case.pairset_fr, case.pairset_kd, case.pairset_r2)
        assert ps.reestimate(PAIRSET_WHICH, matrix=case.R).tolist() == T["shared_status"]
        assert ps.reestimate(case.pairset_reest).tolist() == T["held_status"]
        assert [bits(m.ravel()) for m in ps.matrices(PAIRSET_WHICH)] == got_store
        same_as_wrapper(run.results("pairset.stored_res"), ps.run_stored(_ffi.CORE_LOCAL, REAL[0], REAL[1], PAIRSET_ACTIVE))
        res, strs = ps.strings(PAIRSET_WHICH)
        assert [(a.tolist(), b.tolist()) for a, b in strs] == run.strings("pairset.stored_str")


# ---------------------------------------------------------------- sequence set
@pytest.fixture(scope="module")
def seqset(case):
    from aligner_amd.seqset import SeqSet
    with SeqSet(case.seqs) as ss:
        yield ss


def test_seqset_pairs_and_scores(run, case, seqset):
    from aligner_amd.seqset import rectangle, upper
    orc = case.orc
    rect = seqset_ref.rectangle_pairs(*RECT)
    assert run.one("set.pairs") == ["upper", str(len(BATCH_PAIRS)), "rectangle", str(len(rect)), "invalid", "0"]
    assert seqset_ref.block_pairs(NSEQ, 0, NSEQ, 0, NSEQ, 1) == len(BATCH_PAIRS) and seqset_ref.block_pairs(NSEQ, *RECT, 0) == len(rect)
    want = [case.local(q, t) for q, t in BATCH_PAIRS]
    status, f = run.ints("set.upper_status"), run.f64("set.upper_f")
    assert status == [o["status"] for o in want]
    assert [v for v, o in zip(f, want) if o["status"] == 0] == bits([o["f"] for o in want if o["status"] == 0])
    assert {0, orc.ERR_CODE_OUT_OF_RANGE} <= set(status)
    wantg = [case.align(p, orc.CORE_GLOBAL, GLOBAL, case.S, "global") for p in rect]
    statusg, fg = run.ints("set.rect_status"), run.f64("set.rect_f")
    assert statusg == [o["status"] for o in wantg] and {0, orc.ERR_CODE_OUT_OF_RANGE} <= set(statusg)
    assert [v for v, o in zip(fg, wantg) if o["status"] == 0] == bits([o["f"] for o in wantg if o["status"] == 0])
    pf, pst = seqset.score(case.S, LOCAL[0], LOCAL[1], upper(0, NSEQ))
    assert bits(pf) == f and pst.tolist() == status
    pf, pst = seqset.score(case.S, GLOBAL[0], GLOBAL[1], rectangle(*RECT), semantics=_ffi.CORE_GLOBAL)
    assert bits(pf) == fg and pst.tolist() == statusg
    assert run.one("set.stats")[:2] == ["nonnegative", "1"]


@pytest.fixture(scope="module")
def hits_truth(case):
    """[(pair index, q, t, oracle answer)] of the pairs of the upper block with f >= F_MIN, ascending"""
    out = []
    for k, (q, t) in enumerate(BATCH_PAIRS):
        o = case.local(q, t)
        if o["status"] == 0 and o["f"] >= F_MIN:
            out.append((k, q, t, o))
    assert 8 <= len(out) < len(BATCH_PAIRS)
    return out


def test_seqset_hits_report_and_filter(run, case, seqset, hits_truth):
    from aligner_amd.seqset import upper
    H = hits_truth
    n = len(H)
    assert run.ints("set.hits_count") == [n]
    assert (run.ints("set.held_pair"), run.ints("set.held_q"), run.ints("set.held_t")) == ([h[0] for h in H], [h[1] for h in H], [h[2] for h in H])
    assert run.f64("set.held_f") == bits([h[3]["f"] for h in H])
    same_summaries(run.results("set.held_res"), [summary_of(h[3]) for h in H])
    same_strings(run.strings("set.held_str"), [h[3] for h in H])
    rep = report_ref.reports([(h[3]["qa"], h[3]["ta"]) for h in H], case.S, report_ref.SKIP_SEED)
    got = np.array([tuple(int(v) for v in r) for r in run.indexed("set.report")], dtype=report_ref.RECORD)
    assert got.tolist() == rep.tolist()
    keep = np.flatnonzero(report_ref.keep(rep, [case.len[h[1]] for h in H], [case.len[h[2]] for h in H], **FILTER))
    assert 0 < len(keep) < n                                                       # the filter separates these hits
    assert run.ints("set.filter_count") == [len(keep)] and run.ints("set.filter_positions") == keep.tolist()
    gotf = np.array([tuple(int(v) for v in r) for r in run.indexed("set.filter_report")], dtype=report_ref.RECORD)
    assert gotf.tolist() == rep[keep].tolist()
    held = seqset.hits(case.S, LOCAL[0], LOCAL[1], F_MIN, upper(0, NSEQ))
    assert (held.index.tolist(), held.q.tolist(), held.t.tolist(), bits(held.f)) == (run.ints("set.held_pair"), run.ints("set.held_q"), run.ints("set.held_t"),
                                                                                   run.f64("set.held_f"))
    res, strs = held.strings()
    same_as_wrapper(run.results("set.held_res"), res)
    assert [(a.tolist(), b.tolist()) for a, b in strs] == run.strings("set.held_str")
    assert held.report(case.S).tolist() == got.tolist()
    pos, prep = held.filter(case.S, with_reports=True, **FILTER)
    assert pos.tolist() == keep.tolist() and prep.tolist() == gotf.tolist() and held.last_filter_count == len(keep)


@pytest.fixture(scope="module")
def signif_truth(case):
    """per listed position: (f of the copies as bits, lengths, the record) from tests/shuffle_ref.py, the oracle and tests/signif_ref.py"""
    out = []
    memo = {}
    for pos in case.signif_keep:
        if pos not in memo:
            q, t, f_hit = case.best[pos]
            stream = SIGNIF["pair_base"] + q * NSEQ + t
            copies = [shuffle_ref.copy_of(case.seqs[t], SIGNIF["seed"], stream, s, SIGNIF["max_trim"])[1] for s in range(SIGNIF["per_pair"])]
            ans = [case.orc.align(case.orc.CORE_LOCAL, case.seqs[q], c, REAL[0], REAL[1], case.R) for c in copies]
            f = np.array([o["f"] if o["status"] == 0 else 0.0 for o in ans])
            status = np.array([o["status"] for o in ans], dtype=np.int32)
            memo[pos] = (f, status, [len(c) for c in copies], signif_ref.reduce_one(f, status, f_hit))
        out.append(memo[pos])
    return out


def test_seqset_best_and_significance(run, case, seqset, signif_truth):
    B = case.best
    assert run.ints("set.best_count") == [len(B)] and len(B) > 2 * BEST_K
    assert run.ints("set.best_pair") == [q * NSEQ + t for q, t, f in B]
    assert (run.ints("set.best_q"), run.ints("set.best_t")) == ([b[0] for b in B], [b[1] for b in B])
    assert run.f64("set.best_f") == bits([b[2] for b in B])
    per = SIGNIF["per_pair"]
    got_f, got_len = run.f64("set.signif_f"), run.ints("set.signif_lengths")
    rows = run.indexed("set.signif")
    assert len(rows) == len(case.signif_keep) <= 9
    for k, (f, status, lengths, rec) in enumerate(signif_truth):
        r = rows[k]
        got = tuple(int(v.split("/")[0], 16) for v in r[:3]) + tuple(int(v) for v in r[3:])
        want = tuple(bits([rec["sum"], rec["sum_sq"], rec["f_max"]])) + (int(rec["n_ok"]), int(rec["n_ge"]), int(rec["status"]), int(rec["first_bad"]), 0)
        assert got == want, k
        assert got_len[k * per:(k + 1) * per] == lengths, k
        ok = status == 0
        assert np.array(got_f[k * per:(k + 1) * per], dtype=np.uint64)[ok].tolist() == bits(f[ok]), k
    assert any(int(rec["n_ge"]) < int(rec["n_ok"]) for _f, _s, _l, rec in signif_truth)
    best = seqset.best(case.S, LOCAL[0], LOCAL[1], BEST_K, f_min=BEST_F_MIN, skip_self=True)
    assert (best.index.tolist(), best.q.tolist(), best.t.tolist(), bits(best.f)) == (run.ints("set.best_pair"), run.ints("set.best_q"), run.ints("set.best_t"),
                                                                                   run.f64("set.best_f"))
    rec, pf, pl = best.significance_records(case.R, REAL[0], REAL[1], SIGNIF["seed"], per_pair=per, max_trim=SIGNIF["max_trim"], keep=case.signif_keep,
                                            pair_base=SIGNIF["pair_base"], scores=True)
    assert bits(pf.ravel()) == got_f and pl.ravel().tolist() == got_len
    for k, r in enumerate(rows):
        assert bits([rec["sum"][k], rec["sum_sq"][k], rec["f_max"][k]]) == [int(v.split("/")[0], 16) for v in r[:3]]
        assert [int(rec[name][k]) for name in ("n_ok", "n_ge", "status", "first_bad", "reserved")] == [int(v) for v in r[3:]]


# ---------------------------------------------------------------- device loop
def test_device_loop(run, case, seqset):
    from aligner_amd.pairset import PairSet
    from aligner_amd.seqset import upper
    block = types.SimpleNamespace(q_first=0, q_count=NSEQ, t_first=0, t_count=NSEQ, upper=1, reserved=0)
    ref = set_loop_cases.OracleSetLoop(set_loop_cases.FakeSeqSet(case.seqs, Protein), block, 0, len(BATCH_PAIRS))
    ref.set_heuristics(24, 24, case.loop_fr, case.loop_kd, case.loop_r2)
    begin = ref.loop_begin(case.S).tolist()
    assert run.ints("loop.begin_status") == begin and 0 in begin and _ffi.TRANSFORM_NO_ROOT in begin
    with PairSet.from_seqset(seqset, upper(0, NSEQ)) as ps:
        ps.set_heuristics(24, 24, case.loop_fr, case.loop_kd, case.loop_r2)
        assert ps.loop_begin(case.S).tolist() == begin
        step, causes = 0, set()
        while ref.going:
            step += 1
            fin, cause, res, counts = ref.loop_step(case.orc.CORE_LOCAL, LOCAL[0], LOCAL[1])
            key = "loop.step%d." % step
            assert run.ints(key + "counts") == list(counts), step
            assert run.ints(key + "finished") == fin.tolist() and run.ints(key + "cause") == cause.tolist(), step
            want = [dict(status=int(r["status"])) if r["status"] != 0 else
                    dict(status=0, f=bits(r["f"])[0], score=bits(r["score"])[0], end_y=int(r["end_y"]), end_x=int(r["end_x"]), start_y=int(r["start_y"]),
                         start_x=int(r["start_x"]), aln_len=int(r["aln_len"])) for r in res]
            same_summaries(run.results(key + "res") if len(res) else [], want)
            causes |= set(cause.tolist())
            pfin, pcause, pres, pcounts = ps.loop_step(_ffi.CORE_LOCAL, LOCAL[0], LOCAL[1])
            assert (pfin.tolist(), pcause.tolist(), list(pcounts)) == (fin.tolist(), cause.tolist(), list(counts)), step
            same_as_wrapper(run.results(key + "res") if len(res) else [], pres)
            assert step < 64
    assert run.one("loop.steps") == [str(step), "going", "0"] and step >= 2
    assert {set_loop_cases.DONE, set_loop_cases.FAILED} <= causes
    assert run.ints("loop.idle_counts") == [0, 0, 0, 0]
