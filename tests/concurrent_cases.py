"""Helpers of the concurrent-caller tests (tests/test_concurrent_*.py).  Not a test module (no test_ prefix); nothing here touches the
GPU at import.

include/aligner_hip.h calls aln_ctx thread-safe: callers on several threads lease different slots of the pool.  The call-history tests
pin what one call after another may assume; these helpers put calls BESIDE one another, on one shared context:

* jobs(): the catalogue.  A Job makes whatever handle it needs, makes a fixed sequence of calls, destroys the handle and returns its
  results as one flat dict of arrays (the form call_history.compare understands).  Its expectation comes from the CPU oracle and the
  plain references alone (expected(orc)); its route predicates (on flags and passes, as call_history.Entry's) show that running beside
  others did not change the route; `calls` names the library symbols it makes.
  - From call_history.catalogue(): every entry without environment knobs, inputs and expectations reused.  The environment is
    process-wide, so an entry that sets a knob would reroute its neighbours: claim_runs (ALN_CLAIM), single_global (ALN_SINGLE_R) and
    pipelined_four_slots (ALN_CHUNK_CELLS) are left out.
  - Handle jobs, each on a handle of its own: a staged batch, a sequence set with its held post-processors (the hand-built set of
    test_cigar_gpu.py), a pair set walked through the state model of pairset_history.py, the device transform against the host one
    bit for bit, aln_cluster_edges, and two refusals with different status and text that read aln_last_error() on their own thread.
  - The LDS opt-in group: two jobs of a kind differ only in the dynamic LDS they ask of ONE kernel, both above 64 KiB
    (hipFuncAttributeMaxDynamicSharedMemorySize belongs to the kernel, not to the thread that set it: aln_launch.h).
    single_lds_30k / single_lds_45k: the single-pair route, core local, BLOSUM62, 11 / 2, 30 000 and 45 000 columns against 128 rows.
    128 and not fewer: aln_big_pair (aln_plan_rules.h) asks for M >= 128, so that is the smallest target that stays on the route;
    with two strips of one row per lane both take the four-wave kernel aln_fill_single_kernel<core local, 1, 4> at 120 800 and
    150 800 bytes.  shuffle_lds_1100 / shuffle_lds_2048: aln_shuffle_scores of one pair, 128 copies, 64 threads x the 16-aligned
    target length: 70 656 and 131 072 bytes.
    The fast batch kernel is absent: its LDS is S + four profiles of cols x 512 bytes + 1 856 bytes of rings, ALN_FAST_LDS admits at
    most 30 columns, and only 30 columns pass 64 KiB (29: 64 624 bytes; 30: 66 896 at most) -- every reachable size above 64 KiB lies
    within 1 360 bytes of every other, none 16 KiB apart.
* rounds(): rounds of ROUND = 6 jobs -- more threads than the pool has slots (4), so a lease waits in every round -- built by a
  deterministic greedy cover so that every unordered pair of jobs, a job with itself included (two threads, two handles), shares a
  round.  lds_rounds(): one dedicated round per pair of the LDS group.  covered(rounds): the pairs a list of rounds covers.
* run_round(): one thread per job of the round behind a barrier; every thread repeats its job `reps` times, every library call timed
  with perf_counter_ns (TimedLib stands in for the ctypes library while a round runs), EVERY repetition compared with the expectation
  and the route.  A thread that outlives its join timeout, or a job that raises, sets STUCK: every later round refuses to start.
  No round is tried twice.
* overlaps(): from the recorded intervals, the pairs of jobs two of whose library calls overlapped in time.
"""
import ctypes as C
import hashlib
import os
import sys
import threading
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import call_history as CH  # noqa: E402
from aligner_amd import _ffi, runtime  # noqa: E402
from aligner_amd.batch import PairBatch  # noqa: E402
from aligner_amd.matrices import get_blosum62  # noqa: E402

LEFT_OUT = ("claim_runs", "single_global", "pipelined_four_slots")
ROUND = 6                            # threads of a round; ALN_POOL_SLOTS is 4
REPS = 3                             # repetitions per thread in the general rounds
# Repetitions per thread in the dedicated LDS rounds: never fewer than 200; as many as keep a round near two seconds on an MI355X (a
# repetition alone takes 2.3 to 2.9 ms on the single-pair route and 0.6 to 0.9 ms in the shuffle, six threads share four slots)
LDS_REPS = 600
LDS_FLOOR, LDS_APART = 64 * 1024, 16 * 1024
SHUFFLE_THREADS = 64                 # ALN_SHUFFLE_THREADS (tests/test_concurrent_cpu.py holds it against aln_device.h)
# Serial seconds of one repetition of a job alone on an MI355X, its comparison included (measured with serial_seconds(), three
# repetitions after a warming one, rounded up to 0.1 ms); a job not listed counts as DEFAULT_SERIAL_S.  A round's join timeout is
# JOIN_FACTOR times the serial time of all its repetitions, at least JOIN_FLOOR_S: at these sizes the floor decides every round.
SERIAL_S = {"fast_local_long": 0.0014, "fast_local_short": 0.0005, "fast_global": 0.0008, "read_pairs_duo": 0.0010, "legacy_local_batch": 0.0004,
            "single_local": 0.0006, "wg_real": 0.0005, "wg_integer_h_d": 0.0004, "f64_strip_batch": 0.0011, "pwm_fast_windows": 0.0010,
            "pwm_real_windows": 0.0008, "force_serial": 0.0056, "shuffle_scores": 0.0005, "scan_hits_held_list": 0.0090, "staged_batch": 0.0050,
            "seqset_held": 0.0080, "pairset_walk": 0.0065, "transform_device": 0.0005, "cluster_edges": 0.0007, "refusal_scan": 0.0041,
            "refusal_null": 0.0005, "single_lds_30k": 0.0030, "single_lds_45k": 0.0023, "shuffle_lds_1100": 0.0007, "shuffle_lds_2048": 0.0010}
DEFAULT_SERIAL_S = 0.25
JOIN_FACTOR, JOIN_FLOOR_S = 20.0, 30.0

STUCK = []                           # names of the jobs of a round that hung or raised: nothing more is started


# ---------------------------------------------------------------- the job
class Job:
    def __init__(self, name, run, expected, calls, route=(), lds=None):
        self.name, self.run, self.expected, self.calls, self.route, self.lds = name, run, expected, frozenset(calls), tuple(route), lds

    def routed(self, got):
        return all(check(got) for check in self.route)


def flat(prefix, d):
    return {prefix + k: np.asarray(v) for k, v in d.items()}


def digest(want):
    """the bytes of an expectation: every key in order, with dtype and shape"""
    h = hashlib.sha256()
    for k in sorted(want):
        a = np.ascontiguousarray(want[k])
        h.update(("%s|%s|%s|" % (k, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def differences(got, want):
    """every key of `want` in which `got` differs (call_history.compare, one key at a time): [] when all agree"""
    out = []
    for k in want:
        if k.startswith("_"):
            continue
        one = {k: want[k]}
        if k == "strings" and "_idx" in want:
            one["_idx"] = want["_idx"]
        d = CH.compare(got, one)
        if d is not None:
            out.append(d)
    return out


# ---------------------------------------------------------------- jobs from call_history.catalogue()
CATALOGUE_CALLS = {"batch": ("aln_align_batch",), "pair": ("aln_align_pair",), "pwm": ("aln_align_batch",), "shuffle": ("aln_shuffle_scores",),
                   "scan": ("aln_scan_create", "aln_scan_hits", "aln_scan_held_list", "aln_scan_held_strings", "aln_scan_string_stride", "aln_scan_destroy")}


def _catalogue_job(e):
    def run(ctx):
        try:
            return e.run()
        finally:
            if e.shape["kind"] == "scan":
                CH.close_scan()                # the handle is the job's own: made and destroyed on its thread
    return Job(e.name, run, e.expected, CATALOGUE_CALLS[e.shape["kind"]], e.route)


# ---------------------------------------------------------------- handle jobs
def _staged_job():
    """about 40 pairs of 40 to 400 residues: create, run, sync, fetch, run again, fetch"""
    b = CH._pairs(31, CH._shapes(31, 40, (40, 401), (40, 401)))
    S = get_blosum62()

    def run(ctx):
        from aligner_amd.batch import StagedBatch
        sb = StagedBatch(b, _ffi.CORE_LOCAL, 11, 2, S, outputs=_ffi.OUT_SCORE | _ffi.OUT_TRACEBACK)
        try:
            out = {}
            for k in ("first/", "again/"):
                sb.run()
                sb.sync()
                got = CH.batch_got(sb.fetch(True))
                out.update({k + f: got[f] for f in CH.FIELDS})
                # (both strings of every pair up to the aln_len that came back: a wrong length shows in aln_len and in the shape)
                out[k + "aligned"] = got["_tb"][CH.string_index(b.q_len, b.t_len, got["aln_len"])]
                out["_flags"], out["_passes"] = got["_flags"], got["_passes"]
            return out
        finally:
            sb.close()

    def expected(orc):
        w = CH.batch_expected(orc, b, _ffi.CORE_LOCAL, 11, 2, S)
        out = {}
        for k in ("first/", "again/"):
            out.update({k + f: w[f] for f in CH.FIELDS})
            out[k + "aligned"] = w["strings"]
        return out

    return Job("staged_batch", run, expected, ("aln_batch_create", "aln_batch_run", "aln_batch_sync", "aln_batch_fetch", "aln_batch_destroy"),
               [CH._is(_ffi.FLAG_FAST)])


SET_DEL, SET_EXT, SET_F_MIN, BLANK = 4.0, 1.0, 150.0, 98


def _seqset_job():
    """the hand-built set of test_cigar_gpu.py (32 records of at most 330 residues): hits, then report, cigars and strings of the held
    hits; expectations from seqset_ref's order, report_ref and cigar_ref, fed from the oracle"""
    import cigar_ref
    import report_ref
    import seqset_ref
    import set_history as SH
    from test_cigar_gpu import hand_built
    recs = hand_built()
    S = get_blosum62()
    flags = cigar_ref.EXTENDED | cigar_ref.CLIPS

    def run(ctx):
        from aligner_amd.seqset import SeqSet, upper
        with SeqSet(recs) as ss:
            held = ss.hits(S, SET_DEL, SET_EXT, SET_F_MIN, upper(0, len(recs)))
            out = dict(count=len(held), index=held.index, q=held.q, t=held.t, f=SH.bits(held.f))
            out.update(SH.struct_fields("rep", held.report(S)))
            cg = held.cigars(extended=True, clips=True)
            out.update(records=np.array(cg.records.tolist(), dtype=np.int64).reshape(-1, 8), offsets=cg.offsets, words=cg.words)
            out.update({"summary." + k: v for k, v in cg.summary.items()})
            res, strs = held.strings()
            out.update({"res." + f: SH.bits(np.ascontiguousarray(res[f])) for f in SH.FIELDS})
            out["aligned"] = np.concatenate([x for pair in strs for x in pair] + [np.zeros(0, np.uint8)])
            return {k: np.asarray(v) for k, v in out.items()}

    def expected(orc):
        n = len(recs)
        pairs = seqset_ref.generate_pairs(0, n)
        res, strs = SH.align_pairs(orc, recs, pairs, (_ffi.CORE_LOCAL, S, SET_DEL, SET_EXT), threads=8)
        index = np.flatnonzero((res["status"] == 0) & (res["f"] >= SET_F_MIN))
        h = SH.Held(SH.upper(0, n), "local", index, pairs, res, strs)
        assert len(h) > 256, "more than one tile of every selection"
        lens = np.array([len(r) for r in recs], dtype=np.uint64)
        out = dict(count=len(h), index=h.index, q=h.q, t=h.t, f=SH.bits(h.f))
        out.update(SH.struct_fields("rep", report_ref.reports(h.strs, S, report_ref.SKIP_SEED, h.res["status"], BLANK)))
        entries = [(h.strs[i][0], h.strs[i][1], int(h.res["aln_len"][i]), int(h.res["status"][i]), int(h.res["start_x"][i]), int(h.res["start_y"][i]),
                    int(lens[h.q[i]])) for i in range(len(h))]
        crecs, off, words, summ = cigar_ref.listed(entries, list(range(len(h))), len(h), BLANK, flags)
        out.update(records=np.array(crecs, dtype=np.int64).reshape(-1, 8), offsets=np.array(off, dtype=np.uint64), words=np.array(words, dtype=np.uint32))
        out.update({"summary." + k: v for k, v in summ.items()})
        out.update({"res." + f: SH.bits(np.ascontiguousarray(h.res[f])) for f in SH.FIELDS})
        out["aligned"] = np.concatenate([x for pair in h.strs for x in pair])
        return {k: np.asarray(v) for k, v in out.items()}

    return Job("seqset_held", run, expected, ("aln_seqset_create", "aln_seqset_hits", "aln_seqset_held_list", "aln_seqset_held_report",
                                              "aln_seqset_held_cigar_plan", "aln_seqset_held_cigar_fill", "aln_seqset_held_strings", "aln_seqset_stats",
                                              "aln_seqset_pairs", "aln_seqset_destroy"))


PAIRSET_WALK = ("heur_a", "run_all", "frequencies", "reest_shared", "reest_held", "run_stored", "strings")


def _pairset_job():
    """a pair set: parameters, a run of every pair, frequencies, reestimate (from a shared matrix, then from the held run), run_stored and
    the held strings; expectations from the state model of pairset_history.py over the oracle"""
    import pairset_history as PH
    lists = PH._Lists(20261021)

    def plan(refs):
        m, out = PH.Model(refs), []
        for entry in PAIRSET_WALK:
            kind, spec, _facts = m.step(entry)
            assert kind is None, "the walk holds no refusal: %s %s" % (entry, kind)
            out.append((entry, refs.get(PH.name_of(entry, spec), spec)))
        return out

    def expected(orc):
        out = {}
        for i, (entry, want) in enumerate(plan(PH.Refs(orc))):
            out["%d:%s/status" % (i, entry)] = np.asarray(0)
            out.update(flat("%d:%s/" % (i, entry), {k: v for k, v in want.items() if not k.startswith("_")}))
        return out

    def run(ctx):
        backend = PH.GpuBackend(lists, borrowed=False)
        try:
            out = {}
            for i, entry in enumerate(PAIRSET_WALK):
                out.update(flat("%d:%s/" % (i, entry), {k: v for k, v in backend.call(entry, {}).items() if not k.startswith("_")}))
            return out
        finally:
            backend.close()

    return Job("pairset_walk", run, expected, ("aln_pairset_create", "aln_pairset_heuristics", "aln_pairset_run", "aln_pairset_frequencies",
                                               "aln_pairset_reestimate", "aln_pairset_run_stored", "aln_pairset_strings", "aln_pairset_destroy"))


def _transform_job():
    """aln_transform_matrices_device on 24 x 24 and 4 x 4 matrices against aln_transform_matrices (the library's host code), bit for bit"""
    rng = np.random.default_rng(41)
    B62 = get_blosum62()
    big = np.stack([B62 * rng.uniform(0.8, 1.2) + rng.normal(0, 0.1, B62.shape) for _ in range(64)])
    small = rng.integers(-4, 6, (48, 4, 4)).astype(np.float64)
    cases = []
    for m in (big, small):
        n, rows = m.shape[0], m.shape[1]
        r2 = np.full(n, float(rows * rows))
        r2[3] = 1e-9                             # no root: the status, and whatever the rule leaves in the matrix
        cases.append((m, rng.dirichlet(np.ones(rows), n), rng.choice([-0.2, -0.5, -1.0], n), r2))

    def both(device):
        from aligner_amd.pairset import transform_matrices, transform_matrices_device
        out = {}
        for k, (m, fr, kd, r2) in enumerate(cases):
            with np.errstate(all="ignore"):
                got, st = (transform_matrices_device if device else transform_matrices)(m, fr, kd, r2)
            out["%d/out" % k], out["%d/status" % k] = np.ascontiguousarray(got, dtype=np.float64), np.asarray(st)
        return out

    job = Job("transform_device", lambda ctx: both(True), lambda orc: both(False), ("aln_transform_matrices_device",))
    job.bitwise = True
    return job


def _cluster_job():
    """aln_cluster_edges, both modes, over 300 nodes and 420 seeded edges (self edges and repeats among them) against cluster_ref"""
    import cluster_ref
    rng = np.random.default_rng(43)
    n = 300
    a, b = rng.integers(0, n, 420).astype(np.uint32), rng.integers(0, n, 420).astype(np.uint32)
    b[:5] = a[:5]
    lengths = rng.integers(30, 400, n).astype(np.uint32)
    keys = ("nodes", "clusters", "edges", "self_edges", "singletons")

    def run(ctx):
        from aligner_amd.cluster import cluster_edges
        out = {}
        for mode in ("components", "greedy"):
            c = cluster_edges(n, a, b, lengths, mode=mode)
            out[mode + "/label"] = c.label
            out[mode + "/records"] = np.array(c.records.tolist(), dtype=np.uint32).reshape(-1, 4)
            out.update({mode + "/" + k: np.asarray(c.summary[k]) for k in keys})
        return out

    def expected(orc):
        out = {}
        for mode, code in (("components", cluster_ref.COMPONENTS), ("greedy", cluster_ref.GREEDY)):
            lab, recs, summ, _mem = cluster_ref.cluster(code, n, a, b, lengths)
            out[mode + "/label"] = np.array(lab, dtype=np.uint32)
            out[mode + "/records"] = np.array(recs, dtype=np.uint32).reshape(-1, 4)
            out.update({mode + "/" + k: np.asarray(summ[k]) for k in keys})
        return out

    return Job("cluster_edges", run, expected, ("aln_cluster_edges",))


REFUSALS = 64                        # refused calls per repetition, each followed by aln_last_error() on the same thread
SCAN_REFUSAL_TEXT = "a window scan aligns a position-weight matrix (ALN_PWM_LOCAL) only"
NULL_REFUSAL_TEXT = "null argument"


def _refusal_expected(status, text):
    return lambda orc: dict(status=np.full(REFUSALS, status, dtype=np.int32), text=np.frombuffer((text * REFUSALS).encode(), dtype=np.uint8).copy(),
                            f_untouched=np.asarray(True))


def _refusal_scan_job():
    """aln_scan_score with core-local semantics on a scan of its own: ALN_ERR_UNSUPPORTED, its own text, the output untouched"""
    seq = np.random.default_rng(47).integers(0, 4, 5000).astype(np.uint8)
    S = get_blosum62()

    def run(ctx):
        lib = _ffi.load()
        st = C.c_int(0)
        h = lib.aln_scan_create(ctx, seq.ctypes.data, len(seq), C.byref(st))
        assert h and st.value == 0, st.value
        try:
            p, _keep = runtime.make_params(_ffi.CORE_LOCAL, 11, 2, S, outputs=_ffi.OUT_SCORE)
            g = _ffi.ScanGeometry(0, 33, 66, 0, 0)
            f = np.full(int(lib.aln_scan_windows(h, C.byref(g))), -7.0)
            status, text = [], []
            for _ in range(REFUSALS):
                status.append(lib.aln_scan_score(h, C.byref(p), C.byref(g), f.ctypes.data))
                text.append(lib.aln_last_error() or b"")
            return dict(status=np.array(status, dtype=np.int32), text=np.frombuffer(b"".join(text), dtype=np.uint8).copy(),
                        f_untouched=np.asarray(bool((f == -7.0).all())))
        finally:
            lib.aln_scan_destroy(h)

    return Job("refusal_scan", run, _refusal_expected(_ffi.ERR_UNSUPPORTED, SCAN_REFUSAL_TEXT),
               ("aln_scan_create", "aln_scan_windows", "aln_scan_score", "aln_last_error", "aln_scan_destroy"))


def _refusal_null_job():
    """aln_align_batch without parameters: ALN_ERR_INVALID_ARGUMENT, its own text, the results untouched"""
    b = CH._pairs(53, [(50, 60), (70, 40)])

    def run(ctx):
        lib = _ffi.load()
        from aligner_amd.batch import RESULT_DTYPE
        res = np.zeros(len(b), dtype=RESULT_DTYPE)
        res.view(np.uint8)[:] = 0x5A
        status, text = [], []
        for _ in range(REFUSALS):
            status.append(lib.aln_align_batch(ctx, None, b.seqs.ctypes.data, b.q_off.ctypes.data, b.q_len.ctypes.data, b.t_off.ctypes.data,
                                              b.t_len.ctypes.data, len(b), res.ctypes.data, None, None))
            text.append(lib.aln_last_error() or b"")
        return dict(status=np.array(status, dtype=np.int32), text=np.frombuffer(b"".join(text), dtype=np.uint8).copy(),
                    f_untouched=np.asarray(bool((res.view(np.uint8) == 0x5A).all())))

    return Job("refusal_null", run, _refusal_expected(_ffi.ERR_INVALID_ARGUMENT, NULL_REFUSAL_TEXT), ("aln_align_batch", "aln_last_error"))


# ---------------------------------------------------------------- the LDS opt-in group
SINGLE_LDS_ROWS = 128                # the smallest target on the single-pair route (aln_big_pair: M >= 128)


def _single_lds_job(columns):
    rng = np.random.default_rng(columns)
    t = rng.integers(0, 20, SINGLE_LDS_ROWS).astype(np.uint8)
    q = rng.integers(0, 20, columns).astype(np.uint8)
    at = columns - 5000                                              # the related stretch lies far into the query
    q[at:at + 100] = np.where(rng.random(100) < 0.08, rng.integers(0, 20, 100), t[14:114])
    e = CH._pair_entry("single_lds_%dk" % (columns // 1000), q, t, _ffi.CORE_LOCAL, 11, 2, get_blosum62(), [CH._is(_ffi.FLAG_SINGLE)])
    return Job(e.name, lambda ctx: e.run(), e.expected, ("aln_align_pair",), e.route,
               lds=dict(kind="single", rows=24, cols=24, N=columns, M=SINGLE_LDS_ROWS, semantics=_ffi.CORE_LOCAL))


SHUFFLE_LDS_QUERY, SHUFFLE_LDS_COPIES, SHUFFLE_LDS_TRIM, SHUFFLE_LDS_SEED = 60, 128, 6, 0xC0FFEE


def _shuffle_lds_job(t_len):
    import shuffle_ref
    rng = np.random.default_rng(t_len)
    q, t = CH._related_pair(rng, SHUFFLE_LDS_QUERY, t_len)
    b = PairBatch.from_pairs([(q, t)])
    S, per = get_blosum62(), SHUFFLE_LDS_COPIES

    def run(ctx):
        f = np.zeros((1, per)); L = np.zeros((1, per), dtype=np.uint32); st = np.zeros(1, dtype=np.int32)
        p, _keep = runtime.make_params(_ffi.CORE_LOCAL, 11, 2, S, outputs=_ffi.OUT_SCORE)
        spec = _ffi.ShuffleSpec(SHUFFLE_LDS_SEED, 0, per, SHUFFLE_LDS_TRIM)
        r = _ffi.load().aln_shuffle_scores(ctx, C.byref(p), C.byref(spec), b.seqs.ctypes.data, b.q_off.ctypes.data, b.q_len.ctypes.data,
                                           b.t_off.ctypes.data, b.t_len.ctypes.data, 1, f.ctypes.data, L.ctypes.data, st.ctypes.data)
        return dict(call_status=np.asarray(r), f=f, lengths=L, status=st)

    def expected(orc):
        copies = [(q, shuffle_ref.copy_of(t, SHUFFLE_LDS_SEED, 0, s, SHUFFLE_LDS_TRIM)[1]) for s in range(per)]
        tb = PairBatch.from_pairs(copies)
        ref, _, _ = orc.align_batch(_ffi.CORE_LOCAL, tb.seqs, tb.q_off, tb.q_len, tb.t_off, tb.t_len, 11, 2, S, n_threads=8, want_traceback=False)
        r = np.frombuffer(ref, dtype=CH.ORC_DTYPE)
        assert (r["status"] == 0).all()
        return dict(call_status=np.asarray(0), f=r["f"].reshape(1, per).copy(), lengths=tb.t_len.astype(np.uint32).reshape(1, per),
                    status=np.zeros(1, np.int32))

    return Job("shuffle_lds_%d" % t_len, run, expected, ("aln_shuffle_scores",), lds=dict(kind="shuffle", t_len=t_len))


LDS_PAIRS = (("single_lds_30k", "single_lds_45k"), ("shuffle_lds_1100", "shuffle_lds_2048"))

_jobs = []


def jobs():
    """The jobs, in a fixed order (built once per process)."""
    if not _jobs:
        out = [_catalogue_job(e) for e in CH.catalogue() if not e.env]
        assert not {j.name for j in out} & set(LEFT_OUT) and len(out) == len(CH.catalogue()) - len(LEFT_OUT)
        out += [_staged_job(), _seqset_job(), _pairset_job(), _transform_job(), _cluster_job(), _refusal_scan_job(), _refusal_null_job()]
        out += [_single_lds_job(30000), _single_lds_job(45000), _shuffle_lds_job(1100), _shuffle_lds_job(2048)]
        assert len({j.name for j in out}) == len(out)
        _jobs.extend(out)
    return _jobs


def by_name():
    return {j.name: j for j in jobs()}


_wants = {}


def expectations(orc):
    """{job name: expectation}: computed once per process from the oracle and left unchanged"""
    if not _wants:
        for j in jobs():
            _wants[j.name] = {k: np.asarray(v) for k, v in j.expected(orc).items()}
    return _wants


def compare(job, got, want):
    """every difference of one repetition's results: fields, strings and the route"""
    if getattr(job, "bitwise", False):
        from test_pairset_resident_gpu import same_bits
        out = ["%s: not the same bits" % k for k in want if k.endswith("/out") and not same_bits(got[k], want[k])]
        out += differences(got, {k: v for k, v in want.items() if not k.endswith("/out")})
    else:
        out = differences(got, want)
    if not job.routed(got):
        out.append("not the route: flags %s passes %s" % (np.unique(got.get("_flags")).tolist(), np.unique(got.get("_passes")).tolist()))
    return out


# ---------------------------------------------------------------- the schedule
def pair_key(a, b):
    return (a, b) if a <= b else (b, a)


def covered(round_list):
    """the unordered pairs of job names (a job with itself included, where it stands twice) that share a round"""
    out = set()
    for r in round_list:
        for i in range(len(r)):
            for k in range(i + 1, len(r)):
                out.add(pair_key(r[i], r[k]))
    return out


def all_pairs(names):
    return {pair_key(a, b) for i, a in enumerate(names) for b in names[i:]}


def rounds(names=None):
    """Rounds of ROUND job names that cover every unordered pair, self pairs included; deterministic.  First the self pairs: three jobs
    twice each per round, in catalogue order (the last round filled up from the front).  Then rounds of six different jobs, greedy: a
    round starts with the first job that has the most uncovered pairs left and takes, five times, the job that covers the most new
    pairs with the round so far, the first in catalogue order on a tie."""
    names = [j.name for j in jobs()] if names is None else list(names)
    assert len(names) >= ROUND
    out = []
    for i in range(0, len(names), ROUND // 2):
        three = (names[i:i + ROUND // 2] + names)[:ROUND // 2]
        out.append([n for n in three for _ in range(2)])
    todo = all_pairs(names) - covered(out)
    while todo:
        left = {n: sum(1 for p in todo if n in p) for n in names}
        r = [max(names, key=lambda n: (left[n], -names.index(n)))]
        while len(r) < ROUND:
            r.append(max((n for n in names if n not in r), key=lambda n: (len({pair_key(n, m) for m in r} & todo), -names.index(n))))
        todo -= covered([r])
        out.append(r)
    return out


def lds_rounds():
    """one dedicated round per pair of the LDS group: three threads each, alternating"""
    return [[a, b] * (ROUND // 2) for a, b in LDS_PAIRS]


def refusal_round():
    """the two refusals beside four working jobs"""
    return ["refusal_scan", "refusal_null", "fast_local_short", "wg_real", "pwm_fast_windows", "staged_batch"]


def join_timeout(round_names, reps):
    serial = sum(SERIAL_S.get(n, DEFAULT_SERIAL_S) for n in round_names) * reps
    return max(JOIN_FLOOR_S, JOIN_FACTOR * serial)


# ---------------------------------------------------------------- the runner
_tl = threading.local()


class TimedLib:
    """Stands in for the ctypes library while a round runs: every aln_* call made on a runner thread is timed into that thread's list."""

    def __init__(self, lib):
        self._lib, self._wrapped = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("aln_"):
            return fn
        w = self._wrapped.get(name)
        if w is None:
            def w(*args, _fn=fn, _name=name):
                sink = getattr(_tl, "calls", None)
                if sink is None:
                    return _fn(*args)
                t0 = time.perf_counter_ns()
                try:
                    return _fn(*args)
                finally:
                    sink.append((t0, time.perf_counter_ns(), _name))
            self._wrapped[name] = w
        return w


class ThreadRecord:
    def __init__(self, name):
        self.name, self.calls, self.failures, self.error, self.reps_done, self.seconds = name, [], [], None, 0, 0.0


def run_round(round_names, wants, reps, timeout=None):
    """Runs one round: [ThreadRecord] in the round's order.  Raises if an earlier round hung or raised, or if this one does."""
    if STUCK:
        raise RuntimeError("an earlier round hung or raised (%s): nothing more is started on the GPU" % ", ".join(STUCK))
    table = by_name()
    ctx = runtime.context()
    real = _ffi.load()
    if isinstance(real, TimedLib):
        real = real._lib
    records = [ThreadRecord(n) for n in round_names]
    barrier = threading.Barrier(len(round_names))

    def work(rec):
        job = table[rec.name]
        _tl.calls = rec.calls
        try:
            barrier.wait(timeout=60)
            t0 = time.perf_counter()
            for r in range(reps):
                got = job.run(ctx)
                diffs = compare(job, got, wants[job.name])
                if diffs:
                    rec.failures.append((r, diffs))
                rec.reps_done += 1
            rec.seconds = time.perf_counter() - t0
        except BaseException as e:      # noqa: BLE001 (reported by the caller; a job that raised ends the module's GPU work)
            rec.error = "%r\n%s" % (e, traceback.format_exc())
        finally:
            _tl.calls = None

    _ffi._lib = TimedLib(real)
    try:
        threads = [threading.Thread(target=work, args=(rec,), name="round-" + rec.name, daemon=True) for rec in records]
        for t in threads:
            t.start()
        deadline = time.monotonic() + (join_timeout(round_names, reps) if timeout is None else timeout)
        for t in threads:
            t.join(timeout=max(0.0, deadline - time.monotonic()))
        alive = [rec.name for t, rec in zip(threads, records) if t.is_alive()]
        if alive:
            STUCK.extend(alive)
            raise RuntimeError("still running after the join timeout: %s" % ", ".join(alive))
        raised = [rec for rec in records if rec.error]
        if raised:
            STUCK.extend(rec.name for rec in raised)
            raise RuntimeError("raised in round %s:\n%s" % (round_names, "\n".join("%s: %s" % (rec.name, rec.error) for rec in raised)))
    finally:
        if not STUCK:
            _ffi._lib = real
    return records


def failures_of(records):
    return ["%s, repetition %d: %s" % (rec.name, r, "; ".join(d)) for rec in records for r, d in rec.failures] + \
           ["%s: %d repetitions done" % (rec.name, rec.reps_done) for rec in records if rec.error]


def _overlap(a, b):
    """do two sorted lists of (t0, t1, name) intervals hold two that intersect?"""
    i = k = 0
    while i < len(a) and k < len(b):
        if a[i][0] < b[k][1] and b[k][0] < a[i][1]:
            return True
        if a[i][1] <= b[k][1]:
            i += 1
        else:
            k += 1
    return False


def overlaps(records):
    """the pairs of job names of one round two of whose library calls, on two threads, overlapped in time"""
    out = set()
    for i in range(len(records)):
        for k in range(i + 1, len(records)):
            if _overlap(sorted(records[i].calls), sorted(records[k].calls)):
                out.add(pair_key(records[i].name, records[k].name))
    return out


def serial_seconds(names, wants, reps=1):
    """{name: seconds per repetition} of every listed job alone, after one warming repetition; asserts every answer"""
    out = {}
    for n in names:
        rec = run_round([n], wants, 1)
        assert not failures_of(rec), failures_of(rec)
        rec = run_round([n], wants, reps)
        assert not failures_of(rec), failures_of(rec)
        out[n] = rec[0].seconds / reps
    return out
