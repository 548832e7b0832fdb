"""Helpers of the pair-set call-history tests (tests/test_pairset_history_*.py).  Not a test module (no test_ prefix).

A resident pair set keeps the held run and entry_of, the transform parameters, the matrix store and its `written` flags, the loop's
best, going lists and host copy, and some twenty grow-only device buffers from call to call.  These helpers walk ONE
handle through call_history.schedule(k) -- every ordered pair of catalogue entries exactly once -- and hold every answer, bit for bit,
against values that come from the CPU oracle, tests/transform_ref.py and the loop rule restated in tests/set_loop_cases.py alone:

* records() / pair_list(): thirteen seeded records whose block window (BLOCK, FIRST, N_PAIRS) numbers the 13 pairs, so that a handle made
  by aln_pairset_create (COPIED) and one made by aln_pairset_create_from_set (BORROWED) must answer identically.
* CATALOGUE: the calls, each with fixed arguments.
* Refs: the primitives (one pair's alignment under one matrix, one transform) and the expected arrays of a call, memoised.
* Model: the handle's state in pure Python.  step(entry) answers the specification of the expected bytes, or the kind of refusal
  the header prescribes, after which state and outputs must be untouched.
* dry_run(): the plan of a walk (the model over the schedule); walk(): the walker over any backend.  GpuBackend calls the library
  through ctypes on marker-filled buffers; FakeBackend answers from the references and can have one defect switched on.
* planned_chunks(): aln_make_chunks (aligner_amd/csrc/aln_plan_rules.h) under a forced ALN_CHUNK_CELLS, restated.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import call_history as CH  # noqa: E402
import set_history as SH  # noqa: E402
import set_loop_cases as cases  # noqa: E402
import transform_ref  # noqa: E402

INV = SH.INV
MARK = SH.MARK                         # every output buffer starts as bytes of this
COUNT_MARK = SH.COUNT_MARK             # every count word starts as this
FIELDS = SH.FIELDS
RES = SH.RES
CORE_GLOBAL, CORE_LOCAL = 0, 1
ROWS = COLS = 24
KINDS = ("no_heuristics", "never_written", "not_in_last_run", "no_held_run", "other_shape", "no_loop")
# scheme name -> (semantics, del, ext, blank code, rows, cols); G and N write their gaps as 7, so that a stale blank code shows
SCHEMES = {"L": (CORE_LOCAL, 11.0, 2.0, 98, 24, 24), "G": (CORE_GLOBAL, 4.0, 4.0, 7, 24, 24), "N": (CORE_LOCAL, 6.0, 1.0, 7, 4, 4)}
CHUNK_CELLS = 40000                    # ALN_CHUNK_CELLS of run_chunked: three chunks or more (planned_chunks)

# ---------------------------------------------------------------- the records and the pairs
BLOCK = (0, 3, 3, 10, 0)               # queries: records 0 .. 2, targets: records 3 .. 12
FIRST, N_PAIRS = 8, 13                 # the window of the block's numbering that is the pair list: it starts and ends inside a row
PLANTED = {2: 63, 3: 64, 4: 65, 5: 127, 6: 128, 7: 129}          # pair -> the oracle's aln_len under run_all
PAIR_ONE, PAIR_NOPOS, PAIR_STRIPS, PAIR_BAD, PAIR_EMPTY = 0, 1, 8, 9, 12
NO_ROOT_PAIR = 3                       # heur_b: r_squared 1e-9


def records(seed=20261021):
    """[one, A, empty, six prefixes of A, t520, bad, [3], [1, 1, 1, 1]].  A target that is a prefix of the query A (300) ends where
    its alignment ends, so nothing can extend it: its aligned length is the prefix's and one (the duplicated seed pair).  t520 holds mutated pieces of A (A x t520: two
    strips), bad a code outside the matrix; the window's first row is the one-residue query's last two pairs (1 x 1, and no positive
    cell against [1, 1, 1, 1]), its last row the empty query's first pair."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 20, 300).astype(np.uint8)
    t520 = rng.integers(0, 20, 520).astype(np.uint8)
    for at, frm, n in ((15, 40, 90), (200, 150, 120), (400, 10, 100)):
        piece = A[frm:frm + n].copy()
        mut = rng.random(n) < 0.2
        piece[mut] = rng.integers(0, 20, int(mut.sum()))
        t520[at:at + n] = piece
    bad = rng.integers(0, 20, 40).astype(np.uint8)
    bad[17] = 30
    recs = [np.array([3], np.uint8), A, np.zeros(0, np.uint8)] + [A[:n - 1].copy() for n in sorted(PLANTED.values())]     # (the seed pair is counted twice)
    recs += [t520, bad, np.array([3], np.uint8), np.array([1, 1, 1, 1], np.uint8)]
    return recs


def window():
    """[(query record, target record)] of the list's pairs: the block's numbering (pair k: q_first + k / t_count, t_first + k % t_count)"""
    qf, qc, tf, tc, _up = BLOCK
    return [(qf + k // tc, tf + k % tc) for k in range(FIRST, FIRST + N_PAIRS)]


def pair_list(recs):
    return [(recs[q], recs[t]) for q, t in window()]


def params_of(name, seed):
    """(frequencies (n, 24), kd (n,), r_squared (n,)) of parameter set a or b"""
    rng = np.random.default_rng(seed + (0 if name == "a" else 7919))
    fr = rng.dirichlet(np.ones(ROWS), N_PAIRS)
    kd = rng.choice([-0.2, -0.5, -1.0], N_PAIRS)
    r2 = np.full(N_PAIRS, 576.0)
    if name == "b":
        r2[NO_ROOT_PAIR] = 1e-9
    return fr, kd, r2


def pair_matrix(k, pair, seed):
    """per-pair matrix k of a pair: BLOSUM62 rescaled and perturbed"""
    from aligner_amd.matrices import get_blosum62
    rng = np.random.default_rng([seed, k, pair])
    return get_blosum62() * rng.uniform(0.8, 1.2) + rng.normal(0, 0.1, (ROWS, COLS))


# ---------------------------------------------------------------- the catalogue: one call with fixed arguments per entry
ALL = tuple(range(N_PAIRS))
SUBSET = (8, 3, 0, 9, 11, 5)
DNA_SUBSET = (1, 0)                    # the pairs whose codes are all < 4
REEST_SHARED = (4, 8, 3, 10, 12, 9, 5, 0)
REEST_HELD = (5, 8)
RUN_STORED = (10, 5, 8, 4, 0)
# Every kind of fetch has a list inside run_subset's list and one that holds pairs in and out of it: strings_out names pair 6, which
# only a run of every pair holds; freq_dna is the 4 x 4 run's list (pair 1 is not in run_subset's), so that the count layout of the
# other shape is compared; matrices names pairs in and out of it.
WHICH = {"matrices": (8, 4, 10), "frequencies": (5, 0, 8), "strings": (0, 8, 5), "strings_out": (0, 8, 6), "freq_dna": (1, 0)}
FETCH_STRINGS, FETCH_FREQ = ("strings", "strings_out"), ("frequencies", "freq_dna")
RUNS = {"run_all": ("L", 0, ALL), "run_chunked": ("L", 0, ALL), "run_subset": ("G", 1, SUBSET), "run_dna": ("N", "D", DNA_SUBSET),
        "run_none": ("L", 0, ())}
# what the header rules out whatever came before: a fetch after a run that does not hold every listed pair, a 4 x 4 or empty held run
# for reestimate, a cleared store
IMPOSSIBLE = frozenset([(r, f) for r in ("run_subset", "run_dna", "run_none", "run_stored") for f in FETCH_STRINGS + FETCH_FREQ
                        if not set(WHICH[f]) <= set(RUN_STORED if r == "run_stored" else RUNS[r][2])] +
                       [(a, "reest_held") for a in ("run_dna", "run_none")] +
                       [(a, b) for a in ("heur_a", "heur_b") for b in ("matrices", "run_stored", "loop_step")])
SET_PASS = dict(block=(0, 13, 0, 13, 1), f_min=20.0)
# The order decides which state every transition of the schedule meets.  This one was picked (by trying seeded shuffles against the
# model alone, tests/test_pairset_history_cpu.py prints the counts) so that the conditions of the CPU test hold.
CATALOGUE = ("run_stored", "frequencies", "run_subset", "run_all", "heur_a", "loop_step", "matrices", "loop_begin", "heur_b", "run_chunked",
             "set_pass", "run_none", "reest_shared", "run_dna", "reest_held", "strings", "freq_dna", "strings_out")
CHANGERS = ("run_all", "run_subset", "run_dna", "run_none", "run_chunked", "heur_a", "heur_b", "reest_shared", "reest_held", "run_stored",
            "loop_begin", "loop_step")
assert 14 <= len(CATALOGUE) <= 18 and len(set(CATALOGUE)) == len(CATALOGUE)


def name_of(entry, spec):
    return entry + "@" + hashlib.sha1(repr(spec).encode()).hexdigest()[:16]


# ---------------------------------------------------------------- references
def count_columns(qa, ta, rows, cols, blank):
    """counts[t * cols + q]: the columns that put target residue t on query residue q, neither being blank, the duplicated seed pair
    included (every column of the strings counts)"""
    c = [0] * (rows * cols)
    for q, t in zip(qa.tolist(), ta.tolist()):
        if q != blank and t != blank and t < rows and q < cols:
            c[t * cols + q] += 1
    return c


class Refs:
    """The primitives and the expected arrays, computed from the oracle on demand and memoised."""

    def __init__(self, orc, seed=20261021):
        from aligner_amd.matrices import get_blosum62
        self.orc, self.seed = orc, seed
        self.recs = records(seed)
        self.pairs = pair_list(self.recs)
        self.par = {"a": params_of("a", seed), "b": params_of("b", seed)}
        self.b62 = get_blosum62()
        self._mat, self._aln, self.memo = {}, {}, {}
        self.q_len = np.array([len(q) for q, _t in self.pairs], dtype=np.int64)
        self.t_len = np.array([len(t) for _q, t in self.pairs], dtype=np.int64)

    # ---- primitives.  A matrix key: ("P", k) per-pair matrix k; ("D",) the 4 x 4 matrix; ("T", parameter set, "B62") the transform of
    # BLOSUM62; ("T", parameter set, scheme, key, blank) the transform of the counts of the pair's alignment under scheme and key
    def matrix(self, pair, mk):
        """(status, matrix or None)"""
        key = (pair, mk)
        if key not in self._mat:
            if mk[0] == "P":
                out = (0, pair_matrix(mk[1], pair, self.seed))
            elif mk[0] == "D":
                out = (0, np.array(cases.DNA_MATRIX))
            else:
                fr, kd, r2 = self.par[mk[1]]
                if mk[2] == "B62":
                    src = [float(x) for x in self.b62.ravel()]
                else:
                    res, qa, ta = self.aln(pair, mk[2], mk[3])
                    if len(mk) > 5:             # (a planted defect: counted as a run of another shape lays its counts)
                        c = count_columns(qa, ta, mk[5][0], mk[5][1], mk[4])
                        src = [float(x) for x in c + [0] * (ROWS * COLS - len(c))]
                    else:
                        src = [float(x) for x in count_columns(qa, ta, ROWS, COLS, mk[4])]
                st, m, _branch = transform_ref.transform(src, ROWS, COLS, [float(x) for x in fr[pair]], float(kd[pair]), float(r2[pair]))
                out = (st, np.array(m, dtype=np.float64).reshape(ROWS, COLS) if st == 0 else None)
            self._mat[key] = out
        return self._mat[key]

    def aln(self, pair, sch, mk):
        """(RES record, aligned query, aligned target) of one pair under one matrix: the oracle, one pair at a time"""
        key = (pair, sch, mk)
        if key not in self._aln:
            sem, d, e, blank, _r, _c = SCHEMES[sch]
            st, m = self.matrix(pair, mk)
            assert st == 0
            q, t = self.pairs[pair]
            packed = np.concatenate([q, t, np.zeros(0, np.uint8)]).astype(np.uint8)
            off = np.array([0], np.uint64)
            ref, tb, tb_off = self.orc.align_batch(sem, packed, off, np.array([len(q)], np.uint64), np.array([len(q)], np.uint64),
                                                   np.array([len(t)], np.uint64), d, e, m, n_threads=1, blank=blank)
            r = np.frombuffer(ref, dtype=CH.ORC_DTYPE)
            res = np.zeros(1, dtype=RES)
            res["status"] = r["status"]
            n = 0
            if r["status"][0] == 0:                 # (a failed pair's other fields are not specified by the header: zeros here, masked in what comes back)
                for name in FIELDS:
                    res[name] = r[name]
                n = int(res["aln_len"][0])
            a, cap = int(tb_off[0]), len(q) + len(t) + 2
            self._aln[key] = (res[0], tb[a:a + n].copy(), tb[a + cap:a + cap + n].copy())
        return self._aln[key]

    # ---- the expected arrays of a call
    def get(self, name, spec=None):
        if name not in self.memo:
            self.memo[name] = {k: np.asarray(v) for k, v in self.compute(spec).items()}
        return self.memo[name]

    def summaries(self, entries):
        res = np.array([self.aln(p, sch, mk)[0] for p, sch, mk in entries], dtype=RES) if entries else np.zeros(0, dtype=RES)
        return {"res." + f: SH.bits(np.ascontiguousarray(res[f])) for f in FIELDS}

    def compute(self, spec):
        kind = spec[0]
        if kind == "ok":
            return dict(_ok=np.asarray(1))
        if kind == "status":
            return dict(status_out=np.array(spec[1], dtype=np.int32))
        if kind == "run":
            return self.summaries(spec[1])
        if kind == "mats":
            return dict(out=SH.bits(np.array([self.matrix(p, mk)[1] for p, mk in spec[1]], dtype=np.float64).reshape(-1)))
        if kind == "freq":
            _k, rows, cols, blank, entries = spec
            out = []
            for p, sch, mk in entries:
                res, qa, ta = self.aln(p, sch, mk)
                out += count_columns(qa, ta, rows, cols, blank)
            return dict(counts=np.array(out, dtype=np.uint32), behind_untouched=np.asarray(True))
        if kind == "strings":
            entries = spec[1]
            out = self.summaries(entries)
            cap = [int(self.q_len[p] + self.t_len[p] + 2) for p, _s, _m in entries]
            tb = np.zeros(2 * sum(cap), dtype=np.uint8)
            at = 0
            for (p, sch, mk), c in zip(entries, cap):
                _res, qa, ta = self.aln(p, sch, mk)
                tb[at:at + len(qa)] = qa
                tb[at + c:at + c + len(ta)] = ta
                at += 2 * c
            out["tb"] = tb
            return out
        if kind == "step":
            _k, n_run, fin, cause, entries = spec
            room = N_PAIRS
            k = len(fin)
            res = np.zeros(room, dtype=RES)
            res.view(np.uint8).reshape(-1)[:] = MARK
            for i, (p, sch, mk) in enumerate(entries):
                res[i] = self.aln(p, sch, mk)[0]
            done = sum(1 for c in cause if c == cases.DONE)
            out = dict(counts=np.array([n_run, done, k - done, n_run - k], dtype=np.uint32), finished=_marked_with(room, np.uint32, fin),
                       cause=_marked_with(room, np.uint32, cause), n_finished=np.asarray(k))
            out.update({"res." + f: SH.bits(np.ascontiguousarray(res[f])) for f in FIELDS})
            return out
        if kind == "set_pass":
            b, f_min = SET_PASS["block"], SET_PASS["f_min"]
            pairs = SH.block_pairs(b)
            res, _strs = SH.align_pairs(self.orc, self.recs, pairs, (CORE_LOCAL, self.b62, 11.0, 2.0), threads=4)
            index = np.flatnonzero((res["status"] == 0) & (res["f"] >= f_min))
            return dict(count=np.asarray(len(index)), index=index.astype(np.uint64), q=np.array([pairs[i][0] for i in index], dtype=np.uint32),
                        t=np.array([pairs[i][1] for i in index], dtype=np.uint32), f=SH.bits(res["f"][index].copy()))
        raise KeyError(kind)


def _marked(shape, dtype):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8).reshape(-1)[:] = MARK
    return a


def _marked_with(n, dtype, head):
    a = _marked(n, dtype)
    a[:len(head)] = np.array(head, dtype=dtype) if len(head) else a[:0]
    return a


# ---------------------------------------------------------------- the state model
class Model:
    """What a handle must answer.  The rules are the comments of include/aligner_hip.h: a run (run, run_stored, a step with pairs
    going) replaces the held run and touches neither the parameters, the store's other entries, best nor the going list; heuristics
    replaces the parameters, clears the store and ends the loop; reestimate writes the listed entries that have a root; loop_begin
    zeroes best, writes every entry that has a root and makes the going list; a refused call changes nothing."""

    def __init__(self, refs):
        self.r = refs
        self.held = None            # dict(active, sch, mk: {pair: matrix key})
        self.heur = None            # None | "a" | "b"
        self.store = {}             # pair -> matrix key (present: written)
        self.loop = False
        self.best = {}              # pair -> f
        self.going = []
        self.flips = 0              # steps that ran since the last loop_begin (cur = flips & 1)
        self.begun_after_odd = False

    def text(self):
        h = "none" if self.held is None else "%s%s" % (self.held["sch"], list(self.held["active"]))
        return "held=%s heur=%s written=%s loop=%s going=%s cur=%d" % (h, self.heur, sorted(self.store), self.loop, self.going, self.flips & 1)

    def held_entries(self, which):
        return tuple((p, self.held["sch"], self.held["mk"][p]) for p in which)

    def hold(self, sch, active, mk):
        self.held = dict(active=tuple(active), sch=sch, mk=dict(mk))

    def fetch_refusal(self, which):
        if self.held is None:
            return "no_held_run"
        if any(p not in self.held["mk"] for p in which):
            return "not_in_last_run"
        return None

    def step(self, entry):
        """(refusal kind or None, specification of the expected arrays or None, extra facts for the conditions): the state moves on"""
        if entry == "set_pass":
            return None, ("set_pass",), {}
        if entry in RUNS:
            sch, k, active = RUNS[entry]
            mk = {p: (("D",) if k == "D" else ("P", k)) for p in active}
            self.hold(sch, active, mk)
            return None, ("run", self.held_entries(active)), {}
        if entry in ("heur_a", "heur_b"):
            self.heur, self.store, self.loop, self.going = entry[-1], {}, False, []
            return None, ("ok",), {}
        if self.heur is None and entry in ("reest_shared", "reest_held", "run_stored", "matrices", "loop_begin", "loop_step"):
            return "no_heuristics", None, {}
        if entry == "reest_shared":
            st = []
            for p in REEST_SHARED:
                mk = ("T", self.heur, "B62")
                st.append(self.r.matrix(p, mk)[0])
                if st[-1] == 0:
                    self.store[p] = mk
            return None, ("status", tuple(st)), {}
        if entry == "reest_held":
            if self.held is None:
                return "no_held_run", None, {}
            sem, d, e, blank, rows, cols = SCHEMES[self.held["sch"]]
            if (rows, cols) != (ROWS, COLS):
                return "other_shape", None, {}
            if any(p not in self.held["mk"] for p in REEST_HELD):
                return "not_in_last_run", None, {}
            st = []
            for p in REEST_HELD:
                mk = ("T", self.heur, self.held["sch"], self.held["mk"][p], blank)
                st.append(self.r.matrix(p, mk)[0])
                if st[-1] == 0:
                    self.store[p] = mk
            return None, ("status", tuple(st)), {}
        if entry == "run_stored":
            if any(p not in self.store for p in RUN_STORED):
                return "never_written", None, {}
            self.hold("G", RUN_STORED, {p: self.store[p] for p in RUN_STORED})
            return None, ("run", self.held_entries(RUN_STORED)), {}
        if entry == "matrices":
            if any(p not in self.store for p in WHICH[entry]):
                return "never_written", None, {}
            return None, ("mats", tuple((p, self.store[p]) for p in WHICH[entry])), {}
        if entry in FETCH_STRINGS + FETCH_FREQ:
            kind = self.fetch_refusal(WHICH[entry])
            if kind:
                return kind, None, {}
            if entry in FETCH_STRINGS:
                return None, ("strings", self.held_entries(WHICH[entry])), {}
            _sem, _d, _e, blank, rows, cols = SCHEMES[self.held["sch"]]
            return None, ("freq", rows, cols, blank, self.held_entries(WHICH[entry])), {}
        if entry == "loop_begin":
            st = []
            for p in ALL:
                mk = ("T", self.heur, "B62")
                st.append(self.r.matrix(p, mk)[0])
                if st[-1] == 0:
                    self.store[p] = mk
            self.begun_after_odd = bool(self.loop and self.flips & 1)
            self.best = {p: 0.0 for p in ALL}
            self.going = [p for p in ALL if st[p] == 0]
            self.loop, self.flips = True, 0
            return None, ("status", tuple(st)), {}
        if entry == "loop_step":
            if not self.loop:
                return "no_loop", None, {}
            going = list(self.going)
            if not going:
                return None, ("step", 0, (), (), ()), dict(going=0, causes=())
            self.hold("L", going, {p: self.store[p] for p in going})
            blank = SCHEMES["L"][3]
            fin, cause, more = [], [], []
            for p in going:
                res = self.r.aln(p, "L", self.held["mk"][p])[0]
                c = cases.classify(int(res["status"]), float(res["f"]), self.best[p])
                if c == 3:
                    self.best[p] = float(res["f"])
                    mk = ("T", self.heur, "L", self.held["mk"][p], blank)
                    if self.r.matrix(p, mk)[0] == 0:
                        self.store[p] = mk
                        more.append(p)
                        continue
                    c = cases.NO_ROOT
                fin.append(p)
                cause.append(c)
            self.going = more
            self.flips += 1
            return None, ("step", len(going), tuple(fin), tuple(cause), self.held_entries(fin)), dict(going=len(going), causes=tuple(cause),
                                                                                                     begun_after_odd=self.begun_after_odd)
        raise KeyError(entry)

    def observations(self):
        """[(observing entry, specification, arguments)]: the whole held list's strings and every written entry"""
        out = []
        if self.held is not None and self.held["active"]:
            out.append(("obs_strings", ("strings", self.held_entries(self.held["active"])), dict(which=list(self.held["active"]))))
        if self.heur is not None and self.store:
            w = sorted(self.store)
            out.append(("obs_matrices", ("mats", tuple((p, self.store[p]) for p in w)), dict(which=w)))
        elif self.heur is not None:         # a cleared store: a fetch of any entry is refused
            out.append(("obs_matrices", None, dict(which=[WHICH["matrices"][0]])))
        return out


def the_schedule(k=None):
    return CH.schedule(len(CATALOGUE) if k is None else k)


def tail(catalogue=CATALOGUE):
    """What follows the circuit.  A circuit holds every transition once, in whatever state the order brings; the tail holds every
    transition the header allows in a state that accepts both calls: parameters, a loop with every rooted pair going and a held run of
    every pair, then the state-changing entry, then the entry.  Behind that, every entry that may stand between two steps stands
    between the first and the second step of a loop and between the second and the third, and a fourth step follows: best is not zero
    there, cur is 1 and then 0, and some pairs finish at the third step because they no longer improve."""
    out = []
    for c in CHANGERS:
        for e in catalogue:
            if (c, e) not in IMPOSSIBLE:
                out += ["heur_a", "loop_begin", "run_all", c, e]
    for c in catalogue:
        if c not in ("heur_a", "heur_b", "loop_begin"):
            out += ["heur_a", "loop_begin", "loop_step", c, "loop_step", c, "loop_step", "loop_step"]
    return out


def dry_run(refs, calls=None, catalogue=CATALOGUE, compute=True):
    """The plan of a walk: [dict(step, prev, entry, kind, name, args, facts, state, obs=[dict(entry, name, args)])].  With compute the
    expected arrays of every name are computed into refs.memo."""
    m = Model(refs)
    seq = [catalogue[e] for e in the_schedule(len(catalogue))][:calls] + (tail(catalogue) if calls is None else [])
    plan, prev = [], None
    for i, entry in enumerate(seq):
        before = m.text()
        kind, spec, facts = m.step(entry)
        item = dict(step=i, prev=prev, entry=entry, kind=kind, name=None, facts={k: (list(v) if isinstance(v, tuple) else v) for k, v in facts.items()},
                    state=before, obs=[])
        if spec is not None:
            item["name"] = name_of(entry, spec)
            if compute:
                refs.get(item["name"], spec)
        for oentry, ospec, oargs in m.observations():
            oname = name_of(oentry, ospec) if ospec is not None else None
            if compute and ospec is not None:
                refs.get(oname, ospec)
            item["obs"].append(dict(entry=oentry, name=oname, args=oargs))
        plan.append(item)
        prev = entry
    return plan


# ---------------------------------------------------------------- the walker
def check(got, want):
    """None, or what is wrong with one call's answer; want: the expected arrays, or None for a refusal"""
    if want is None:
        if int(got["status"]) != INV:
            return "status %d, want the refusal %d" % (int(got["status"]), INV)
        if not got.get("_untouched", True):
            return "a refused call wrote into %s" % got.get("_touched", "an output")
        return None
    if int(got["status"]) != 0:
        return "status %d (%s), want 0" % (int(got["status"]), got.get("_error", ""))
    return CH.compare(got, want)


def digest(got, want):
    h = hashlib.sha1(str(int(got["status"])).encode())
    for key in sorted(want or {}):
        if not key.startswith("_") and key in got:
            h.update(np.ascontiguousarray(got[key]).tobytes())
    return h.hexdigest()


def walk(backend, plan, wants, stop_at_first=False, skip=()):
    """Runs the plan on the backend's handle and holds every answer, and after every call the observable state, against wants.
    Returns dict(calls, refusals per kind, failures, log): a failure names the step, the transition, the state and the first differing
    field and position; log: one digest per call of the plan (None for a skipped entry)."""
    failures, refusals, n_calls, log = [], dict.fromkeys(KINDS, 0), 0, []
    for item in plan:
        if item["entry"] in skip:
            log.append(None)
            continue
        todo = [(item["entry"], item["name"], {}, True)] + [(o["entry"], o["name"], o["args"], False) for o in item["obs"]]
        digests = []
        for entry, name, args, main in todo:
            want = wants[name] if name else None
            got = backend.call(entry, args, item["step"])
            n_calls += 1
            if main and item["kind"]:
                refusals[item["kind"]] += 1
            diff = check(got, want)
            digests.append(digest(got, want))
            if diff is None:
                continue
            msg = "step %d: %s -> %s%s: %s [%s]" % (item["step"], item["prev"], item["entry"], "" if main else " (then %s)" % entry, diff, item["state"])
            failures.append(dict(step=item["step"], prev=item["prev"], entry=item["entry"], observed=entry, message=msg))
            if int(got["status"]) not in (0, INV):          # an error of the device or the runtime, not an answer: nothing more is started
                failures[-1]["message"] += "; the walk ends here"
                return dict(calls=n_calls, refusals=refusals, failures=failures, log=log)
            if stop_at_first:
                return dict(calls=n_calls, refusals=refusals, failures=failures, log=log)
        log.append("".join(digests))
    return dict(calls=n_calls, refusals=refusals, failures=failures, log=log)


def planned_chunks(q_len, t_len, target):
    """aln_make_chunks under a forced target of `target` cells: the number of chunks of a run over the listed pairs"""
    cells = [float(a) * float(b) for a, b in zip(q_len, t_len)]
    total = float(sum(cells))
    if total <= 1.5 * target:
        return 1
    chunks, acc, open_ = 0, 0.0, 0
    for c in cells:
        acc += c
        open_ += 1
        if acc >= target:
            chunks, acc, open_ = chunks + 1, 0.0, 0
    if open_ and not (chunks and acc < 0.25 * target):
        chunks += 1
    return chunks


# ---------------------------------------------------------------- the fake backend (the CPU test's): answers from the references
DEFECTS = ("run_resets_best", "run_resets_going", "heuristics_keeps_written", "strings_serves_previous_run", "reest_held_counts_run_before_last",
           "loop_begin_keeps_going", "step_uses_earlier_blank", "step_uses_earlier_shape", "refused_call_writes", "chunked_differs")


class FakeBackend:
    """A handle that answers from the references under the model's own rules -- with one defect switched on, wrongly:
    run_resets_best                     a run between two steps zeroes best
    run_resets_going                    a run between two steps empties the going list
    heuristics_keeps_written            heuristics leaves the written flags (and what the entries held) as they were
    strings_serves_previous_run         strings answers from the run before for a pair that is not in the last run
    reest_held_counts_run_before_last   reestimate from held strings counts the strings of the run before the last
    loop_begin_keeps_going              loop_begin keeps the old going list where one is left
    step_uses_earlier_blank             the step's transform counts under the blank code of the run before the step's own
    step_uses_earlier_shape             the step's transform lays its counts in the rows and cols of the run before the step's own
    refused_call_writes                 a refused call writes one byte of an output
    chunked_differs                     run_chunked differs from run_all in one pair
    first_effect: the step at which the defect first changed the state or an answer."""

    def __init__(self, refs, defect=None):
        assert defect is None or defect in DEFECTS
        self.r, self.defect, self.first_effect = refs, defect, None
        self.m = Model(refs)
        self.before_last = None
        self.cache = {}

    def effect(self, step):
        if self.first_effect is None:
            self.first_effect = step

    def answer(self, spec):
        name = name_of("fake", spec)
        if name not in self.cache:
            self.cache[name] = {k: np.asarray(v) for k, v in self.r.compute(spec).items()}
        out = dict(self.cache[name])
        out["status"] = np.asarray(0)
        return out

    def call(self, entry, args, step):
        m, d = self.m, self.defect
        if entry == "obs_strings":
            return self.answer(("strings", m.held_entries(args["which"]))) if m.fetch_refusal(args["which"]) is None else dict(status=np.asarray(INV))
        if entry == "obs_matrices":
            if any(p not in m.store for p in args["which"]):
                return dict(status=np.asarray(INV))
            return self.answer(("mats", tuple((p, m.store[p]) for p in args["which"])))
        held_before, store_before, going_before, loop_before = m.held, dict(m.store), list(m.going), m.loop
        if d in ("step_uses_earlier_blank", "step_uses_earlier_shape") and entry == "loop_step" and m.loop and m.going and m.held is not None:
            blank, shape = SCHEMES[m.held["sch"]][3], SCHEMES[m.held["sch"]][4:]
            if d == "step_uses_earlier_blank" and blank != SCHEMES["L"][3]:
                return self.stale_step(step, blank, None)
            if d == "step_uses_earlier_shape" and shape != (ROWS, COLS):
                return self.stale_step(step, SCHEMES["L"][3], shape)
        if d == "reest_held_counts_run_before_last" and entry == "reest_held" and self.before_last is not None and m.heur and m.held is not None:
            old = self.before_last
            if all(p in old["mk"] for p in REEST_HELD) and SCHEMES[old["sch"]][4] == ROWS and m.fetch_refusal(REEST_HELD) is None and \
                    SCHEMES[m.held["sch"]][4] == ROWS and any((old["sch"], old["mk"][p]) != (m.held["sch"], m.held["mk"][p]) for p in REEST_HELD):
                keep, m.held = m.held, old
                kind, spec, _f = m.step(entry)
                m.held = keep
                self.effect(step)
                return self.answer(spec)
        kind, spec, _facts = m.step(entry)
        if m.held is not held_before and held_before is not None:
            self.before_last = held_before
        if kind:
            if d == "strings_serves_previous_run" and entry in FETCH_STRINGS and kind == "not_in_last_run" and self.before_last is not None and \
                    all(p in self.before_last["mk"] for p in WHICH[entry]):
                self.effect(step)
                old = self.before_last
                return self.answer(("strings", tuple((p, old["sch"], old["mk"][p]) for p in WHICH[entry])))
            if d == "refused_call_writes":
                self.effect(step)
                return dict(status=np.asarray(INV), _untouched=False, _touched="one byte")
            return dict(status=np.asarray(INV), _untouched=True)
        if entry in RUNS or entry == "run_stored":
            if d == "run_resets_best" and loop_before and any(v != 0.0 for v in m.best.values()):
                m.best = {p: 0.0 for p in ALL}
                self.effect(step)
            if d == "run_resets_going" and loop_before and m.going:
                m.going = []
                self.effect(step)
        if d == "heuristics_keeps_written" and entry in ("heur_a", "heur_b") and store_before:
            m.store = store_before
            self.effect(step)
        if d == "loop_begin_keeps_going" and entry == "loop_begin" and loop_before and going_before and going_before != m.going:
            m.going = going_before
            self.effect(step)
        out = self.answer(spec)
        if d == "chunked_differs" and entry == "run_chunked":
            f = out["res.f"].copy()
            f[3] ^= np.uint64(1)
            out["res.f"] = f
            self.effect(step)
        return out

    def stale_step(self, step, blank, shape):
        """loop_step whose transform counts under the blank code, or in the shape, of the run it replaced"""
        m = self.m
        going = list(m.going)
        m.hold("L", going, {p: m.store[p] for p in going})
        fin, cause, more = [], [], []
        for p in going:
            res = self.r.aln(p, "L", m.held["mk"][p])[0]
            c = cases.classify(int(res["status"]), float(res["f"]), m.best[p])
            if c == 3:
                m.best[p] = float(res["f"])
                mk = ("T", m.heur, "L", m.held["mk"][p], blank) + ((tuple(shape),) if shape else ())
                self.effect(step)
                if self.r.matrix(p, mk)[0] == 0:
                    m.store[p] = mk
                    more.append(p)
                    continue
                c = cases.NO_ROOT
            fin.append(p)
            cause.append(c)
        m.going = more
        m.flips += 1
        return self.answer(("step", len(going), tuple(fin), tuple(cause), m.held_entries(fin)))


# ---------------------------------------------------------------- the GPU backend
def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class GpuBackend:
    """One handle, COPIED (aln_pairset_create) or BORROWED (aln_pairset_create_from_set over the owning SeqSet), every call through
    ctypes on buffers that start as MARK bytes."""

    def __init__(self, refs_like, borrowed):
        from aligner_amd import _ffi, runtime
        from aligner_amd.batch import RESULT_DTYPE, PairBatch
        from aligner_amd.seqset import SeqSet
        assert _ffi.ERR_INVALID_ARGUMENT == INV
        self.ffi, self.runtime, self.lib, self.RESULT = _ffi, runtime, _ffi.load(), RESULT_DTYPE
        self.seed, self.pairs, self.par, self.b62 = refs_like.seed, refs_like.pairs, refs_like.par, np.ascontiguousarray(refs_like.b62, dtype=np.float64)
        self.q_len = np.array([len(q) for q, _t in self.pairs], dtype=np.int64)
        self.t_len = np.array([len(t) for _q, t in self.pairs], dtype=np.int64)
        self.set, self.ps, self.seconds, self.shape = None, None, 0.0, (0, 0)
        st = C.c_int(0)
        if borrowed:
            self.set = SeqSet(refs_like.recs)
            blk = _ffi.SeqsetBlock(*BLOCK, 0)
            self.ps = self.lib.aln_pairset_create_from_set(self.set.handle, C.byref(blk), FIRST, N_PAIRS, C.byref(st))
        else:
            b = PairBatch.from_pairs(self.pairs)
            self.ps = self.lib.aln_pairset_create(runtime.context(), b.seqs.ctypes.data, b.q_off.ctypes.data, b.q_len.ctypes.data, b.t_off.ctypes.data,
                                                  b.t_len.ctypes.data, len(b), C.byref(st))
        assert self.ps and st.value == 0, st.value

    def close(self):
        if self.ps:
            self.lib.aln_pairset_destroy(self.ps)
            self.ps = None
        if self.set is not None:
            self.set.close()
            self.set = None

    def params(self, sch):
        sem, d, e, blank, rows, cols = SCHEMES[sch]
        return self.ffi.Params(sem, 0, d, e, None, rows, cols, cols, 0, blank, 0, 0, 0, 0)

    def done(self, status, outs):
        """status and outputs; of a refusal, whether every output still holds its marker"""
        got = dict(status=np.asarray(status))
        if status != 0:
            got["_error"] = (self.lib.aln_last_error() or b"").decode("utf-8", "replace")
            touched = [k for k, v in outs.items() if v is not None and v.size and not (v.view(np.uint8) == MARK).all()]
            got["_untouched"], got["_touched"] = not touched, ",".join(touched)
            return got
        got.update(outs)
        return got

    def summaries(self, res):
        """the compared fields; a failed pair's fields other than its status are not specified by the header: zeros"""
        bad = res["status"] != 0
        out = {}
        for f in FIELDS:
            a = np.ascontiguousarray(res[f]).copy()
            if f != "status":
                a[bad] = 0
            out["res." + f] = SH.bits(a)
        return out

    def call(self, entry, args, step=None):
        import time
        t0 = time.perf_counter()
        try:
            return getattr(self, "do_" + ("run" if entry in RUNS else "heur" if entry.startswith("heur_") else entry))(entry, args)
        finally:
            self.seconds += time.perf_counter() - t0

    def do_run(self, entry, args):
        sch, k, active = RUNS[entry]
        rows, cols = SCHEMES[sch][4:]
        act = np.array(active, dtype=np.uint32)
        mats = np.array([cases.DNA_MATRIX if k == "D" else pair_matrix(k, p, self.seed) for p in active], dtype=np.float64).reshape(len(active), rows, cols)
        p = self.params(sch)
        res = _marked(len(act), self.RESULT)
        with CH.knobs({"ALN_CHUNK_CELLS": str(CHUNK_CELLS)} if entry == "run_chunked" else {}):
            st = self.lib.aln_pairset_run(self.ps, C.byref(p), _ptr(mats), _ptr(act), len(act), _ptr(res))
        if st == 0:
            self.shape = (rows, cols)
        return self.done(st, dict(res=res)) if st != 0 else self.done(0, self.summaries(res))

    def do_heur(self, entry, args):
        fr, kd, r2 = (np.ascontiguousarray(x, dtype=np.float64) for x in self.par[entry[-1]])
        return self.done(self.lib.aln_pairset_heuristics(self.ps, ROWS, COLS, fr.ctypes.data, kd.ctypes.data, r2.ctypes.data), {})

    def reestimate(self, which, shared):
        w = np.array(which, dtype=np.uint32)
        status = _marked(len(w), np.int32)
        st = self.lib.aln_pairset_reestimate(self.ps, self.b62.ctypes.data if shared else None, w.ctypes.data, len(w), status.ctypes.data)
        return self.done(st, dict(status_out=status))

    def do_reest_shared(self, entry, args):
        return self.reestimate(REEST_SHARED, True)

    def do_reest_held(self, entry, args):
        return self.reestimate(REEST_HELD, False)

    def do_run_stored(self, entry, args):
        act = np.array(RUN_STORED, dtype=np.uint32)
        p = self.params("G")
        res = _marked(len(act), self.RESULT)
        st = self.lib.aln_pairset_run_stored(self.ps, C.byref(p), act.ctypes.data, len(act), res.ctypes.data)
        if st == 0:
            self.shape = (ROWS, COLS)
        return self.done(st, dict(res=res)) if st != 0 else self.done(0, self.summaries(res))

    def matrices(self, which):
        w = np.array(which, dtype=np.uint32)
        out = _marked(len(w) * ROWS * COLS, np.float64)
        st = self.lib.aln_pairset_matrices(self.ps, w.ctypes.data, len(w), out.ctypes.data)
        return self.done(st, dict(out=out)) if st != 0 else self.done(0, dict(out=SH.bits(out)))

    def do_matrices(self, entry, args):
        return self.matrices(WHICH["matrices"])

    def do_obs_matrices(self, entry, args):
        return self.matrices(args["which"])

    def do_frequencies(self, entry, args):
        w = np.array(WHICH[entry], dtype=np.uint32)
        counts = _marked(len(w) * ROWS * COLS, np.uint32)               # room for the larger shape: a 4 x 4 run fills its head and no more
        st = self.lib.aln_pairset_frequencies(self.ps, w.ctypes.data, len(w), counts.ctypes.data)
        if st != 0:
            return self.done(st, dict(counts=counts))
        n = len(w) * self.shape[0] * self.shape[1]                      # (the shape of the caller's own last run)
        return self.done(0, dict(counts=counts[:n], behind_untouched=np.asarray(bool((counts[n:].view(np.uint8) == MARK).all()))))

    do_freq_dna = do_frequencies

    def strings(self, which):
        w = np.array(which, dtype=np.uint32)
        cap = (self.q_len[w] + self.t_len[w] + 2).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(2 * cap)[:-1]]).astype(np.uint64)
        res, tb = _marked(len(w), self.RESULT), _marked(int((2 * cap).sum()), np.uint8)
        st = self.lib.aln_pairset_strings(self.ps, w.ctypes.data, len(w), res.ctypes.data, tb.ctypes.data, off.ctypes.data)
        if st != 0:
            return self.done(st, dict(res=res, tb=tb))
        out = self.summaries(res)
        out["tb"] = tb
        return self.done(0, out)

    def do_strings(self, entry, args):
        return self.strings(WHICH[entry])

    do_strings_out = do_strings

    def do_obs_strings(self, entry, args):
        return self.strings(args["which"])

    def do_loop_begin(self, entry, args):
        status = _marked(N_PAIRS, np.int32)
        return self.done(self.lib.aln_pairset_loop_begin(self.ps, self.b62.ctypes.data, status.ctypes.data), dict(status_out=status))

    def do_loop_step(self, entry, args):
        p = self.params("L")
        fin, cause, res, counts = _marked(N_PAIRS, np.uint32), _marked(N_PAIRS, np.uint32), _marked(N_PAIRS, self.RESULT), _marked(4, np.uint32)
        st = self.lib.aln_pairset_loop_step(self.ps, C.byref(p), fin.ctypes.data, cause.ctypes.data, res.ctypes.data, counts.ctypes.data)
        if st != 0:
            return self.done(st, dict(finished=fin, cause=cause, res=res, counts=counts))
        k = int(counts[1]) + int(counts[2])
        if int(counts[0]):
            self.shape = (ROWS, COLS)
        out = dict(counts=counts, finished=fin, cause=cause, n_finished=np.asarray(k))
        if k <= N_PAIRS:                         # the finished entries as summaries; whatever lies behind them as it is (the marker)
            head = self.summaries(res[:k])
            for f in FIELDS:
                out["res." + f] = np.concatenate([head["res." + f], SH.bits(np.ascontiguousarray(res[f][k:]))])
        return self.done(0, out)

    def do_set_pass(self, entry, args):
        ss = self.set
        p, _keep = self.runtime.make_params(CORE_LOCAL, 11.0, 2.0, self.b62, blank=98)
        blk = self.ffi.SeqsetBlock(*SET_PASS["block"], 0)
        count = C.c_uint64(COUNT_MARK)
        st = self.lib.aln_seqset_hits(ss.handle, C.byref(p), C.byref(blk), SET_PASS["f_min"], C.byref(count))
        if st != 0:
            return self.done(st, dict(count=_marked(1, np.uint64) if count.value == COUNT_MARK else np.zeros(1, np.uint64)))
        n = min(int(count.value), 1 << 16)
        outs = dict(count=np.asarray(int(count.value)), index=_marked(n, np.uint64), q=_marked(n, np.uint32), t=_marked(n, np.uint32), f=_marked(n, np.float64))
        if n:
            st = self.lib.aln_seqset_held_list(ss.handle, 0, n, outs["index"].ctypes.data, outs["q"].ctypes.data, outs["t"].ctypes.data, outs["f"].ctypes.data)
            if st != 0:
                return self.done(st, {})
        outs["f"] = SH.bits(outs["f"])
        return self.done(0, outs)


# ---------------------------------------------------------------- the child process of tests/test_pairset_history_gpu.py
# python pairset_history.py MODE job.json report.json: one walk in a context of its own, every call held against the expected values the
# parent computed from the oracle; the parent asserts on the report.  MODE: copied | borrowed | destroy.
class _Lists:
    def __init__(self, seed):
        from aligner_amd.matrices import get_blosum62
        self.seed, self.recs = seed, records(seed)
        self.pairs = pair_list(self.recs)
        self.par = {"a": params_of("a", seed), "b": params_of("b", seed)}
        self.b62 = get_blosum62()


def main(argv):
    import time
    mode, job_path, report = argv
    with open(job_path) as f:
        job = json.load(f)
    out = dict(walks=[])
    backend = None
    for part in job["parts"]:
        wants = CH.load_expected(part["expected"])
        if backend is not None:
            backend.close()                      # (destroy: the first handle goes half-way, the next one lives on the same context)
        backend = GpuBackend(_Lists(part["seed"]), borrowed=(mode == "borrowed"))
        t0 = time.perf_counter()
        w = walk(backend, part["plan"], wants, skip=() if mode == "borrowed" else ("set_pass",))
        w["seconds"], w["library_seconds"] = time.perf_counter() - t0, backend.seconds
        out["walks"].append(w)
        if any("the walk ends here" in x["message"] for x in w["failures"]):
            break
    backend.close()
    with open(report, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1:])
