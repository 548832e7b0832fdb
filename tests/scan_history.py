"""Helpers of the window-scan call-history tests (tests/test_scan_history_*.py).  Not a test module (no test_ prefix).

A window scan (aln_scan_*) keeps from call to call: the reversed strand once a reverse pass has built it (rev_ready), the
held hits of its last aln_scan_hits (host words, and the hits themselves in its private slot, idx and held_f), a dozen grow-only
device buffers that passes of different geometries, widths, PWM kinds and routes share, its slot's salt counter, and -- with every
other scan of the process -- an LRU of 8 plans whose key holds neither the residues nor the strand.  These helpers walk
ONE scan through call_history.schedule(K) -- every ordered pair of catalogue entries exactly once -- and hold every answer, bit for bit
over whole marker-filled arrays, against the CPU oracle window by window:

* chromosome(seed): 3001 seeded codes (a prime: no step divides it); a second seed gives the other scan's, of the same length.
* PASSES / FETCHES / REFUSED / CATALOGUE: the calls, each with fixed arguments; a threshold that is "the pass's own" mean and
  standard deviation is computed from the oracle's f (Refs.args).
* Refs: the oracle's alignment of every window of a (PWM, gaps, geometry, strand, chromosome), memoised, and the expected arrays.
* Model: the ABI's rule in pure Python -- which calls hold hits, which invalidate them, what a fetch may address -- and with it the
  kind of every refusal.
* dry_run(): the plan of a walk; walk(): the walker over any backend.  Backend drives an "abi" object on marker-filled buffers:
  GpuAbi calls the library through ctypes on GpuScan.h, FakeAbi answers from repeats_held_backend.HeldOracleScan and can have one
  fault planted.
* plan_keys(): the shape fields of scan_plan's cache key (aln_host.hip), restated.
* the child program of tests/test_scan_history_gpu.py (walk | destroy | wrap).
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
import repeats_held_backend as HB  # noqa: E402
from aligner_amd.enums import DNA  # noqa: E402
from aligner_amd.pwm import PWMAlignment  # noqa: E402

OK, DEVICE, OOM, INV, UNSUPPORTED, CAPACITY = 0, 5, 6, 7, 8, 10
CORE_LOCAL, PWM_LOCAL = 1, 4
MARK = 0x5A                            # every output buffer starts as bytes of this
COUNT_MARK = 0xABCDEF                  # every count word starts as this
PAD = 3                                # entries of room behind what a call may write: they must keep the marker
RES = np.dtype([("f", "<f8"), ("score", "<f8"), ("end_y", "<u4"), ("end_x", "<u4"), ("start_y", "<u4"), ("start_x", "<u4"),
                ("aln_len", "<u4"), ("status", "<i4"), ("passes", "<u4"), ("flags", "<u4")])
assert RES.itemsize == 48
FIELDS = ("f", "score", "end_y", "end_x", "start_y", "start_x", "aln_len", "status", "flags")      # every field but `passes`
FLAG_INTEGER, FLAG_FAST = 1, 8
LEN, SEED, OTHER_SEED = 3001, 20261021, 977
MIN_SLOTS = 8                          # ALN_SCAN_MIN_SLOTS
# The widest PWM and window of the catalogue: the room of a fetch that must be refused.  A library that answers it all the same then
# writes into the buffers and is reported; with less room it would write past them, into the test's own heap.
MAX_W, MAX_WIDTH = 300, 530
KINDS = ("no_held", "keep_beyond", "not_pwm", "step_zero")
KIND_RET = {"no_held": INV, "keep_beyond": INV, "not_pwm": UNSUPPORTED, "step_zero": INV}

# geometry name -> (PWM columns, seed of the PWMs, del, ext, first, step, width)
GEOMS = {
    "g50": (50, 3, 5.0, 2.0, 3, 7, 40),                     # windows shorter than the PWM, the tail truncated
    "g30": (30, 5, 4.0, 1.0, 0, 10, 70),
    "two_strip": (40, 13, 5.0, 2.0, 0, 257, 530),           # 512 + 18 rows: two strips, another scratch layout; 12 windows
    "few": (300, 9, 30.0, 7.0, LEN - 100, 30, 330),         # 100, 70, 40 and 10 rows: the one-workgroup route and the batch kernel
    "none": (50, 3, 5.0, 2.0, LEN + 5, 7, 40),              # first >= len: no window
}
# pass name -> (call, PWM kind, geometry, reverse, threshold rule, capacity (None: every window))
#   ("own", z): the pass's own mean and standard deviation; ("above",): mean above the maximum; ("sd0",): median, sd = 0, z = 3
PASSES = {
    "score_fwd_int": ("score", "int", "g50", 0, None, None),
    "score_rev_real": ("score", "real", "g50", 1, None, None),
    "select_rev": ("select", "int", "g30", 1, ("own", 1.5), None),
    "select_cap": ("select", "int", "g30", 1, ("own", 0.5), 3),
    "select_none": ("select", "int", "g30", 1, ("above",), None),
    "select_sd0": ("select", "int", "g30", 1, ("sd0",), None),
    "hits_fwd_int": ("hits", "int", "g50", 0, ("own", 1.0), None),
    "hits_rev_real": ("hits", "real", "g30", 1, ("own", 1.0), None),
    "hits_all": ("hits", "int", "g50", 1, ("own", -np.inf), None),
    "hits_none": ("hits", "int", "g30", 0, ("above",), None),
    "hits_two_strip": ("hits", "int", "two_strip", 0, ("fixed", 0.0, 1.0, -np.inf), None),
    "hits_few_fwd": ("hits", "real", "few", 0, ("own", -np.inf), None),
    "hits_few_rev": ("hits", "real", "few", 1, ("own", -np.inf), None),
    "hits_no_window": ("hits", "int", "none", 0, ("fixed", 0.0, 1.0, -np.inf), None),
}
SOME_HITS = ("select_rev", "select_cap", "select_sd0", "hits_fwd_int", "hits_rev_real")       # hits, and fewer than windows
EVERY_HIT = ("hits_all", "hits_two_strip", "hits_few_fwd", "hits_few_rev")
NO_HIT = ("select_none", "hits_none", "hits_no_window")
REFUSED = {"refused_not_pwm": "not_pwm", "refused_step_zero": "step_zero"}
FETCHES = ("list_all", "list_inner", "freq_subset", "freq_empty", "strings_subset", "keep_beyond")
OTHER_PASS = "hits_fwd_int"            # what the other scan runs: a geometry (and so the plans) the first scan uses as well
# The order decides which state every transition of the schedule meets; the CPU test asserts what it is built for.
CATALOGUE = ("hits_fwd_int", "list_all", "score_rev_real", "strings_subset", "hits_two_strip", "select_rev", "freq_subset", "hits_few_rev",
             "refused_not_pwm", "hits_all", "list_inner", "select_cap", "other_hits", "hits_rev_real", "keep_beyond", "score_fwd_int",
             "hits_few_fwd", "freq_empty", "select_sd0", "hits_none", "refused_step_zero", "select_none", "hits_no_window")
assert set(CATALOGUE) == set(PASSES) | set(REFUSED) | set(FETCHES) | {"other_hits"} and len(set(CATALOGUE)) == len(CATALOGUE)


def chromosome(seed, n=LEN):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def pwm(kind, W, seed):
    """as tests/test_repeats_gpu.py::_pwms: "int" holds integers in -3 .. 3, "real" normal(0, 1.3) values"""
    rng = np.random.default_rng(seed)
    ints = rng.integers(-3, 4, size=(4, W)).astype(np.float64)
    real = rng.normal(0.0, 1.3, size=(4, W))
    return ints if kind == "int" else real


def n_windows(length, first, step):
    return (length - 1 - first) // step + 1 if first < length else 0


def window_lengths(length, first, step, width, idx):
    idx = np.asarray(idx, dtype=np.int64)
    return np.clip(np.minimum(width, length - (first + idx * step)), 0, width)


def string_stride(length, W, width):
    """aln_scan_string_stride restated"""
    return (5 * (W + min(width, length) + 2) + 3) & ~3


def flags_of(kind):
    """a hit's summary comes from the re-fill, which has at least 8 slots: the fast integer kernels or the f64 batch kernel"""
    return FLAG_INTEGER | FLAG_FAST if kind == "int" else 0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def marked(n, dtype):
    a = np.empty(n, dtype=dtype)
    a.view(np.uint8).reshape(-1)[:] = MARK
    return a


def marked_with(n, dtype, head):
    a = marked(n, dtype)
    if len(head):
        a[:len(head)] = np.asarray(head, dtype=dtype)
    return a


def untouched(a):
    return a is None or bool((np.ascontiguousarray(a).view(np.uint8) == MARK).all())


def subset(count, salt):
    """a permuted half of the positions 0 .. count - 1, its first listed twice"""
    if count == 0:
        return []
    perm = np.random.default_rng(1000 * salt + count).permutation(count)[:max(1, (count + 1) // 2)].tolist()
    return perm + perm[:1]


def fetch_args(entry, count):
    """the arguments of a fetch over `count` held hits; count None: no hits are held (the call must be refused, on room for one entry)"""
    if count is None:
        return dict(first=0, n=1) if entry.startswith("list") else dict(keep=[] if entry == "freq_empty" else [0])
    if entry == "list_all":
        return dict(first=0, n=count)
    if entry == "list_inner":
        return dict(first=count // 4, n=count // 2)
    if entry == "freq_subset":
        return dict(keep=subset(count, 1))
    if entry == "freq_empty":
        return dict(keep=[])
    if entry == "strings_subset":
        return dict(keep=subset(count, 2))
    if entry == "keep_beyond":
        return dict(keep=([0, count] if count else [0]))
    raise KeyError(entry)


def name_of(entry, spec):
    return entry + "@" + hashlib.sha1(repr(spec).encode()).hexdigest()[:16]


# ---------------------------------------------------------------- references
class Refs:
    """The oracle's answers.  which: 0 the walked scan's chromosome, 1 the other scan's."""

    def __init__(self, orc, seed=SEED, other_seed=OTHER_SEED, length=LEN):
        self.orc, self.seed, self.other_seed, self.length = orc, seed, other_seed, length
        self.chroms = [chromosome(seed, length), chromosome(other_seed, length)]
        self.scans = [HB.MemoOracleScan(c) for c in self.chroms]
        self._aligned, self._args, self.memo = {}, {}, {}

    def geom(self, name):
        W, pseed, d, e, first, step, width = GEOMS[name]
        if name == "few":
            first = self.length - 100
        elif name == "none":
            first = self.length + 5
        return W, pseed, d, e, first, step, width

    def aligned(self, kind, gname, reverse, which):
        """the oracle's result of every window, memoised per (PWM, gaps, geometry, strand, chromosome)"""
        key = (kind, gname, int(reverse), which)
        if key not in self._aligned:
            W, pseed, d, e, first, step, width = self.geom(gname)
            m = pwm(kind, W, pseed)
            sc = self.scans[which]
            self._aligned[key] = [sc._align(w, m, d, e) for _k, w in sc._windows(first, step, width, bool(reverse))]
        return self._aligned[key]

    def f(self, name, which=0):
        _call, kind, gname, reverse, _rule, _cap = PASSES[name]
        return np.array([r["f"] for r in self.aligned(kind, gname, reverse, which)], dtype=np.float64)

    def args(self, name, which=0):
        """every argument of a pass, as plain numbers"""
        if (name, which) not in self._args:
            call, kind, gname, reverse, rule, cap = PASSES[name]
            W, pseed, d, e, first, step, width = self.geom(gname)
            f = self.f(name, which)
            mean = sd = z = 0.0
            if rule is not None:
                if rule[0] == "own":
                    mean, sd, z = float(np.mean(f)), float(np.std(f)), float(rule[1])
                elif rule[0] == "above":
                    mean, sd, z = float(f.max()) + 1.0, 1.0, 0.0
                elif rule[0] == "sd0":
                    mean, sd, z = float(np.median(f)), 0.0, 3.0
                else:
                    mean, sd, z = (float(x) for x in rule[1:])
            n = n_windows(self.length, first, step)
            self._args[(name, which)] = dict(name=name, call=call, kind=kind, W=W, pwm_seed=pseed, d=d, e=e, first=first, step=step, width=width,
                                             reverse=int(reverse), mean=mean, sd=sd, z=z, cap=int(n if cap is None else cap), n=n, which=which,
                                             semantics=PWM_LOCAL, length=self.length)
        return dict(self._args[(name, which)])

    def hit_idx(self, name, which=0):
        """numpy's float64 division under errstate: NaN fails, +inf passes"""
        a, f = self.args(name, which), self.f(name, which)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.flatnonzero((f - np.float64(a["mean"])) / np.float64(a["sd"]) >= np.float64(a["z"])) if len(f) else np.zeros(0, np.int64)

    def hit_records(self, name, which=0):
        _call, kind, gname, reverse, _rule, _cap = PASSES[name]
        al = self.aligned(kind, gname, reverse, which)
        return [al[int(k)] for k in self.hit_idx(name, which)]

    def hit_lengths(self, name, which=0):
        a = self.args(name, which)
        return window_lengths(self.length, a["first"], a["step"], a["width"], self.hit_idx(name, which))

    # ---- the expected arrays of a call
    def get(self, name, spec):
        if name not in self.memo:
            self.memo[name] = {k: np.asarray(v) for k, v in self.compute(spec).items()}
        return self.memo[name]

    @staticmethod
    def summaries(records, room, kind):
        res = marked(room, RES)
        for i, r in enumerate(records):
            res[i] = (r["f"], r["score"], r["end"][0], r["end"][1], r["start"][0], r["start"][1], len(r["numbered"]), r["status"], 0, flags_of(kind))
        return {"res." + f: bits(np.ascontiguousarray(res[f])) for f in FIELDS}

    @staticmethod
    def strings(records):
        return dict(numbered=np.concatenate([np.asarray(r["numbered"], dtype=np.uint32) for r in records] + [np.zeros(0, np.uint32)]),
                    residues=np.concatenate([np.asarray(r["qal"], dtype=np.uint8) for r in records] + [np.zeros(0, np.uint8)]),
                    tb_behind_untouched=np.asarray(True))

    def compute(self, spec):
        what = spec[0]
        if what == "score":
            f = self.f(spec[1], spec[2])
            return dict(ret=np.asarray(OK), f=bits(marked_with(len(f) + PAD, np.float64, f)))
        name, which = spec[1], spec[2]
        a = self.args(name, which)
        idx, recs = self.hit_idx(name, which), self.hit_records(name, which)
        if what == "hits":
            return dict(ret=np.asarray(OK), count=np.asarray(len(idx)))
        if what == "select":
            got = min(len(idx), a["cap"])
            out = dict(ret=np.asarray(CAPACITY if len(idx) > a["cap"] else OK), count=np.asarray(len(idx)),
                       idx=marked_with(a["cap"] + PAD, np.uint32, idx[:got]))
            out.update(self.summaries(recs[:got], a["cap"] + PAD, a["kind"]))
            out.update(self.strings(recs[:got]))
            return out
        if what == "list":
            first, n = spec[3], spec[4]
            f = np.array([r["f"] for r in recs[first:first + n]], dtype=np.float64)
            return dict(ret=np.asarray(OK), idx=marked_with(n + PAD, np.uint32, idx[first:first + n]), f=bits(marked_with(n + PAD, np.float64, f)))
        if what == "freq":
            total = np.zeros((4, a["W"]), dtype=np.float64)
            for k in spec[3]:                     # the sum of get_frequency_matrix over the list as written
                r = recs[k]
                total = total + PWMAlignment(DNA, r["numbered"], r["qal"], a["W"], r["coords"], r["f"]).get_frequency_matrix()
            return dict(ret=np.asarray(OK), counts=bits(marked_with(4 * a["W"] + PAD, np.float64, total.ravel())), behind_untouched=np.asarray(True))
        if what == "strings":
            keep = list(spec[3])
            out = dict(ret=np.asarray(OK))
            out.update(self.summaries([recs[k] for k in keep], len(keep) + PAD, a["kind"]))
            out.update(self.strings([recs[k] for k in keep]))
            return out
        if what == "other":
            f = np.array([r["f"] for r in recs], dtype=np.float64)
            n = len(idx)
            out = dict(ret=np.asarray(OK), count=np.asarray(n), idx=marked_with(n + PAD, np.uint32, idx), f=bits(marked_with(n + PAD, np.float64, f)))
            out.update(self.summaries(recs, n + PAD, a["kind"]))
            out.update(self.strings(recs))
            return out
        raise KeyError(what)


# ---------------------------------------------------------------- the state model
class Model:
    """The rule of include/aligner_hip.h, restated: aln_scan_hits holds its hits (an empty list too, and with no window at all);
    every accepted pass -- score and select included -- replaces or drops them; a refused call (a pass or a fetch) changes nothing;
    a fetch addresses positions 0 .. count - 1 of the held list and is refused without one; the other scan's calls touch nothing here."""

    def __init__(self, refs):
        self.r = refs
        self.held = None               # name of the held pass

    def text(self):
        return "held=%s" % (self.held if self.held is None else "%s(%d)" % (self.held, self.count()))

    def count(self):
        return len(self.r.hit_idx(self.held))

    def lengths(self, keep):
        return [int(self.r.hit_lengths(self.held)[k]) for k in keep]

    def step(self, entry):
        """(refusal kind or None, specification of the expected arrays or None, the call's arguments): the state moves on"""
        if entry in PASSES:
            a = self.r.args(entry)
            self.held = entry if a["call"] == "hits" else None
            return None, (a["call"], entry, 0), a
        if entry in REFUSED:
            a = self.r.args("hits_fwd_int")
            if entry == "refused_not_pwm":
                a["semantics"] = CORE_LOCAL
            else:                          # (as a select pass: every kind of output has room that must stay untouched)
                a["step"], a["reverse"], a["call"] = 0, 1, "select"
            return REFUSED[entry], None, a
        if entry == "other_hits":
            return None, ("other", OTHER_PASS, 1), self.r.args(OTHER_PASS, 1)
        if self.held is None:
            return "no_held", None, fetch_args(entry, None)
        a = fetch_args(entry, self.count())
        pa = self.r.args(self.held)
        a.update(W=pa["W"], width=pa["width"])
        if entry == "keep_beyond":
            return "keep_beyond", None, a
        if entry.startswith("list"):
            return None, ("list", self.held, 0, a["first"], a["n"]), a
        if entry.startswith("freq"):
            return None, ("freq", self.held, 0, tuple(a["keep"])), a
        a["lengths"] = self.lengths(a["keep"])
        return None, ("strings", self.held, 0, tuple(a["keep"])), a

    def observations(self):
        """[(observing entry, specification or None, arguments)]: the whole held list and every hit's strings, or the refusal of
        an empty range"""
        if self.held is None:
            return [("obs_refused", None, dict(first=0, n=0))]
        n, pa = self.count(), self.r.args(self.held)
        every = list(range(n))
        return [("obs_list", ("list", self.held, 0, 0, n), dict(first=0, n=n)),
                ("obs_strings", ("strings", self.held, 0, tuple(every)), dict(keep=every, lengths=self.lengths(every), W=pa["W"], width=pa["width"]))]


def the_schedule(catalogue=CATALOGUE):
    return [catalogue[i] for i in CH.schedule(len(catalogue))]


def dry_run(refs, calls=None, catalogue=CATALOGUE, compute=True):
    """The plan of a walk: [dict(step, prev, entry, kind, name, args, state, obs=[dict(entry, name, args)])].  With compute the expected
    arrays of every name are computed into refs.memo."""
    m = Model(refs)
    plan, prev = [], None
    for i, entry in enumerate(the_schedule(catalogue)[:calls]):
        before = m.text()
        kind, spec, args = m.step(entry)
        item = dict(step=i, prev=prev, entry=entry, kind=kind, name=None, args=args, state=before, obs=[])
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


def expected_calls(plan):
    return sum(1 + len(x["obs"]) for x in plan)


def plan_keys(refs, entry):
    """The shape fields of the keys scan_plan looks up for one pass (aln_host.hip): (len, windows, first, step, width, re-fill slots,
    PWM columns, PWM kind, strings wanted).  The strand and the residues are not part of a key."""
    a = refs.args(entry)
    if a["n"] == 0:
        return []
    fill = (a["length"], a["n"], a["first"], a["step"], a["width"], 0, a["W"], a["kind"], 0)
    hits = len(refs.hit_idx(entry))
    if a["call"] == "select":
        slots = max(min(a["cap"], a["n"]), MIN_SLOTS)
    elif a["call"] == "hits" and hits:
        slots = max(hits, MIN_SLOTS)
    else:
        return [fill]
    return [fill, (a["length"], a["n"], a["first"], a["step"], a["width"], slots, a["W"], a["kind"], 1)]


# ---------------------------------------------------------------- the walker
def check(got, want, kind):
    """None, or what is wrong with one call's answer; want: the expected arrays, or None for a refusal of `kind`"""
    ret = int(got["ret"])
    if want is None:
        if ret != KIND_RET[kind]:
            return "status %d, want the refusal %d (%s)" % (ret, KIND_RET[kind], kind)
        if not got.get("_untouched", True):
            return "a refused call wrote into %s" % got.get("_touched", "an output")
        return None
    if ret != int(want["ret"]):
        return "status %d (%s), want %d" % (ret, got.get("_error", ""), int(want["ret"]))
    return CH.compare(got, want)


def walk(backend, plan, wants, stop_at_first=False):
    """Runs the plan on the backend and holds every answer, and after every call the observable held state, against wants.  Returns
    dict(calls, refusals per kind, failures, entries): a failure names the step, the transition, the state and the first differing
    field and position; entries: the catalogue entries in the order they ran."""
    failures, refusals, n_calls, entries = [], dict.fromkeys(KINDS, 0), 0, []
    for item in plan:
        todo = [(item["entry"], item["name"], item["args"], item["kind"], True)]
        todo += [(o["entry"], o["name"], o["args"], None if o["name"] else "no_held", False) for o in item["obs"]]
        entries.append(item["entry"])
        for entry, name, args, kind, main in todo:
            want = wants[name] if name else None
            got = backend.call(entry, args, item["step"])
            n_calls += 1
            if main and kind:
                refusals[kind] += 1
            diff = check(got, want, kind)
            if diff is None:
                continue
            msg = "step %d: %s -> %s%s: %s [%s]" % (item["step"], item["prev"], item["entry"], "" if main else " (then %s)" % entry, diff, item["state"])
            failures.append(dict(step=item["step"], prev=item["prev"], entry=item["entry"], observed=entry, message=msg))
            if int(got["ret"]) in (DEVICE, OOM):              # an error of the device or the runtime, not an answer: nothing more is started
                failures[-1]["message"] += "; the walk ends here"
                return dict(calls=n_calls, refusals=refusals, failures=failures, entries=entries)
            if stop_at_first:
                return dict(calls=n_calls, refusals=refusals, failures=failures, entries=entries)
    return dict(calls=n_calls, refusals=refusals, failures=failures, entries=entries)


def take_strings(tb, stride, aln_len, lengths, W, n):
    """both strings of entries 0 .. n - 1 up to aln_len, out of the layout of aln_scan_select: entry h at h * stride, its column
    numbers first, its residues at 4 * (W + that window's length + 2)"""
    nums, ress = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint8)]
    for h in range(n):
        c = W + int(lengths[h]) + 2
        L, o = min(int(aln_len[h]), c), h * stride
        nums.append(tb[o:o + 4 * L].copy().view(np.uint32))
        ress.append(tb[o + 4 * c:o + 4 * c + L].copy())
    return np.concatenate(nums), np.concatenate(ress)


class Backend:
    """Every call on buffers that start as marker bytes, with PAD entries of room behind what the call may write.  abi: an object with
    the functions of the window scan's C ABI (GpuAbi, FakeAbi); scan 0 is the walked one, scan 1 the other."""

    def __init__(self, abi):
        self.abi, self.seconds, self.serial = abi, 0.0, 0

    def close(self):
        self.abi.close()

    def call(self, entry, args, step=None):
        import time
        self.serial += 1
        self.abi.mark(self.serial, entry, step)
        t0 = time.perf_counter()
        try:
            if entry in PASSES or entry in REFUSED:
                return getattr(self, "do_" + args["call"])(args)
            if entry == "other_hits":
                return self.do_other(args)
            if "keep" not in args:
                return self.do_list(args)
            if entry.startswith("freq"):
                return self.do_freq(args)
            if entry == "keep_beyond":
                return self.do_beyond(args)
            return self.do_strings(args)
        finally:
            self.seconds += time.perf_counter() - t0

    def done(self, ret, raw, outs=None, count=None):
        """status and outputs; of any status but OK and CAPACITY, whether every output still holds its marker"""
        got = dict(ret=np.asarray(ret))
        if ret not in (OK, CAPACITY):
            got["_error"] = self.abi.last_error()
            touched = [k for k, v in raw.items() if not untouched(v)]
            if count is not None and int(count[0]) != COUNT_MARK:
                touched.append("count")
            got["_untouched"], got["_touched"] = not touched, ",".join(touched)
            return got
        got.update(outs or {})
        return got

    @staticmethod
    def split(res):
        return {"res." + f: bits(np.ascontiguousarray(res[f])) for f in FIELDS}

    def with_strings(self, out, res, tb, stride, lengths, W, n):
        out.update(self.split(res))
        out["numbered"], out["residues"] = take_strings(tb, stride, res["aln_len"], lengths, W, n)
        out["tb_behind_untouched"] = np.asarray(untouched(tb[n * stride:]))
        return out

    def do_score(self, a):
        f = marked(a["n"] + PAD, np.float64)
        ret = self.abi.score(a["which"], a, f)
        return self.done(ret, dict(f=f), dict(f=bits(f)))

    def do_select(self, a):
        cap = a["cap"]
        stride = self.abi.stride(a["which"], a)
        count, idx, res, tb = np.array([COUNT_MARK], np.uint64), marked(cap + PAD, np.uint32), marked(cap + PAD, RES), marked(stride * cap + 64, np.uint8)
        ret = self.abi.select(a["which"], a, cap, count, idx, res, tb)
        if ret not in (OK, CAPACITY):
            return self.done(ret, dict(idx=idx, res=res, tb=tb), count=count)
        if stride != string_stride(a["length"], a["W"], a["width"]):
            return dict(ret=np.asarray(ret), _stride=stride)          # (every expected key is then missing)
        n = min(int(count[0]), cap)
        lengths = window_lengths(a["length"], a["first"], a["step"], a["width"], idx[:n])
        return self.with_strings(dict(ret=np.asarray(ret), count=np.asarray(int(count[0])), idx=idx), res, tb, stride, lengths, a["W"], n)

    def do_hits(self, a):
        count = np.array([COUNT_MARK], np.uint64)
        ret = self.abi.hits(a["which"], a, count)
        return self.done(ret, {}, dict(count=np.asarray(int(count[0]))), count=count)

    def do_list(self, a, which=0):
        idx, f = marked(a["n"] + PAD, np.uint32), marked(a["n"] + PAD, np.float64)
        ret = self.abi.held_list(which, a["first"], a["n"], idx, f)
        return self.done(ret, dict(idx=idx, f=f), dict(idx=idx, f=bits(f)))

    def do_freq(self, a):
        W = a.get("W", MAX_W)
        # (room for the widest PWM whatever the model says is held: the library writes what ITS held pass has columns for)
        counts, keep = marked(4 * max(W, MAX_W) + PAD, np.float64), np.array(a["keep"], dtype=np.uint32)
        ret = self.abi.held_frequencies(0, keep, counts)
        return self.done(ret, dict(counts=counts), dict(counts=bits(counts[:4 * W + PAD]), behind_untouched=np.asarray(untouched(counts[4 * W:]))))

    def do_strings(self, a, which=0):
        keep = np.array(a["keep"], dtype=np.uint32)
        W, width = a.get("W", MAX_W), a.get("width", MAX_WIDTH)
        stride = string_stride(self.abi.length, W, width)
        room = max(stride, string_stride(self.abi.length, MAX_W, MAX_WIDTH))      # (the library strides by what ITS held pass has)
        res, tb = marked(len(keep) + PAD, RES), marked(room * len(keep) + 64, np.uint8)
        ret = self.abi.held_strings(which, keep, res, tb)
        if ret != OK:
            return self.done(ret, dict(res=res, tb=tb))
        return self.with_strings(dict(ret=np.asarray(ret)), res, tb, stride, a.get("lengths", [0] * len(keep)), W, len(keep))

    def do_beyond(self, a):
        """both fetches that take a list: each must refuse it and write nothing"""
        first = self.do_freq(a)
        if int(first["ret"]) != INV or not first.get("_untouched", True):
            return first
        return self.do_strings(a)

    def do_other(self, a):
        """a held pass on the other scan, then its whole list and every hit's strings"""
        count = np.array([COUNT_MARK], np.uint64)
        ret = self.abi.hits(1, a, count)
        if ret != OK:
            return self.done(ret, {}, count=count)
        n = int(count[0])
        if n > a["n"]:
            return dict(ret=np.asarray(ret), count=np.asarray(n))
        lst = self.do_list(dict(first=0, n=n), which=1)
        if int(lst["ret"]) != OK:
            return lst
        lengths = window_lengths(a["length"], a["first"], a["step"], a["width"], lst["idx"][:n])
        out = self.do_strings(dict(keep=list(range(n)), lengths=lengths, W=a["W"], width=a["width"]), which=1)
        out.update(count=np.asarray(n), idx=lst["idx"], f=lst["f"])
        return out


# ---------------------------------------------------------------- the fake scan (the CPU test's): HeldOracleScan behind the ABI's rules
FAULTS = ("score_keeps_held", "select_keeps_held", "refused_pass_drops_held", "strings_ignore_keep_order")


class FakeAbi:
    """The ABI over repeats_held_backend.HeldOracleScan, which is right by construction -- with one fault planted, wrongly:
    score_keeps_held            held hits survive a score pass
    select_keeps_held           held hits survive a select pass (the fetches behind it are answered, from whatever pass is held)
    refused_pass_drops_held     a refused pass drops the held hits
    strings_ignore_keep_order   held_strings answers the listed hits in ascending order
    first_effect: the step at which the fault first changed the state or an answer."""

    def __init__(self, chroms, fault=None):
        assert fault is None or fault in FAULTS
        self.length, self.fault, self.first_effect, self.step = len(chroms[0]), fault, None, None
        self.scans = [HB.HeldOracleScan(c) for c in chroms]
        self.held = [None, None]       # dict(h=FakeHeld, W, kind, stride, lengths)

    def close(self):
        pass

    def mark(self, serial, entry, step):
        self.step = step

    def last_error(self):
        return ""

    def effect(self):
        if self.first_effect is None:
            self.first_effect = self.step

    def stride(self, which, a):
        return string_stride(self.length, a["W"], a["width"])

    def refusal(self, which, a):
        ret = UNSUPPORTED if a["semantics"] != PWM_LOCAL else INV if a["step"] == 0 or a["width"] == 0 else OK
        if ret != OK and self.fault == "refused_pass_drops_held" and self.held[which] is not None:
            self.held[which] = None
            self.effect()
        return ret

    def drop(self, which):
        self.held[which] = None

    @staticmethod
    def record(aln, kind):
        (sx, ex), (sy, ey) = aln.coords
        return (aln.f, aln.f, ey - 1, ex - 1, sy - 1, sx - 1, len(aln.numbered), OK, 1, flags_of(kind))

    @classmethod
    def write(cls, alns, kind, W, lengths, stride, res, tb):
        for h, (aln, wl) in enumerate(zip(alns, lengths)):
            res[h] = cls.record(aln, kind)
            L, o, c = len(aln.numbered), h * stride, W + int(wl) + 2
            tb[o:o + 4 * L] = aln.numbered.astype(np.uint32).view(np.uint8)
            tb[o + 4 * c:o + 4 * c + L] = aln.query

    def score(self, which, a, f):
        ret = self.refusal(which, a)
        if ret != OK:
            return ret
        sc = self.scans[which]
        f[:a["n"]] = sc.score(pwm(a["kind"], a["W"], a["pwm_seed"]), a["d"], a["e"], a["first"], a["step"], a["width"], reverse=bool(a["reverse"]))
        if self.fault == "score_keeps_held" and self.held[which] is not None:
            self.held[which]["h"].generation = sc.generation
            self.effect()
        else:
            self.drop(which)
        return OK

    def select(self, which, a, cap, count, idx, res, tb):
        ret = self.refusal(which, a)
        if ret != OK:
            return ret
        sc = self.scans[which]
        sc.generation += 1
        if self.fault == "select_keeps_held" and self.held[which] is not None:
            self.held[which]["h"].generation = sc.generation
            self.effect()
        else:
            self.drop(which)
        hit, alns = HB.MemoOracleScan.select(sc, pwm(a["kind"], a["W"], a["pwm_seed"]), a["d"], a["e"], a["first"], a["step"], a["width"], a["mean"],
                                             a["sd"], a["z"], reverse=bool(a["reverse"]))
        count[0] = len(hit)
        n = min(len(hit), cap)
        idx[:n] = hit[:n]
        self.write(alns[:n], a["kind"], a["W"], window_lengths(self.length, a["first"], a["step"], a["width"], hit[:n]), self.stride(which, a), res, tb)
        return CAPACITY if len(hit) > cap else OK

    def hits(self, which, a, count):
        ret = self.refusal(which, a)
        if ret != OK:
            return ret
        sc = self.scans[which]
        h = sc.hits(pwm(a["kind"], a["W"], a["pwm_seed"]), a["d"], a["e"], a["first"], a["step"], a["width"], a["mean"], a["sd"], a["z"],
                    reverse=bool(a["reverse"]))
        self.held[which] = dict(h=h, W=a["W"], kind=a["kind"], stride=self.stride(which, a),
                                lengths=window_lengths(self.length, a["first"], a["step"], a["width"], h.idx))
        count[0] = len(h.idx)
        return OK

    def listed(self, which, keep):
        st = self.held[which]
        return None if st is None or any(int(k) >= len(st["h"].idx) for k in keep) else st

    def held_list(self, which, first, n, idx, f):
        st = self.held[which]
        if st is None or first > len(st["h"].idx) or n > len(st["h"].idx) - first:
            return INV
        idx[:n], f[:n] = st["h"].idx[first:first + n], st["h"].f[first:first + n]
        return OK

    def held_frequencies(self, which, keep, counts):
        st = self.listed(which, keep)
        if st is None:
            return INV
        counts[:4 * st["W"]] = st["h"].frequencies(keep).ravel()
        return OK

    def held_strings(self, which, keep, res, tb):
        st = self.listed(which, keep)
        if st is None:
            return INV
        order = [int(k) for k in keep]
        if self.fault == "strings_ignore_keep_order" and sorted(order) != order:
            order = sorted(order)
            self.effect()
        self.write(st["h"].alignments(order), st["kind"], st["W"], [st["lengths"][k] for k in order], st["stride"], res, tb)
        return OK


# ---------------------------------------------------------------- the GPU: the C ABI through ctypes on GpuScan.h
def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class GpuAbi:
    def __init__(self, chroms):
        from aligner_amd import _ffi, runtime
        from aligner_amd.repeats import GpuScan
        assert (_ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED, _ffi.ERR_CAPACITY, _ffi.PWM_LOCAL) == (INV, UNSUPPORTED, CAPACITY, PWM_LOCAL)
        self.ffi, self.runtime, self.lib, self.length = _ffi, runtime, _ffi.load(), len(chroms[0])
        self.scans = [GpuScan(c) for c in chroms]
        self._pwm = {}

    def close(self):
        for sc in self.scans:
            sc.close()                   # aln_scan_destroy

    def mark(self, serial, entry, step):
        """a line of our own on the stream the library traces its plans on ("aln route:"): which call planned what"""
        sys.stderr.write("scan call %d %s\n" % (serial, entry))
        sys.stderr.flush()

    def last_error(self):
        return (self.lib.aln_last_error() or b"").decode("utf-8", "replace")

    def handles(self, which, a):
        key = (a["kind"], a["W"], a["pwm_seed"])
        if key not in self._pwm:
            self._pwm[key] = np.ascontiguousarray(pwm(*key))
        p, keep = self.runtime.make_params(a["semantics"], a["d"], a["e"], self._pwm[key])
        g = self.ffi.ScanGeometry(a["first"], a["step"], a["width"], a["reverse"], 0)
        return self.scans[which].h, p, g, keep

    def stride(self, which, a):
        h, _p, g, _keep = self.handles(which, a)
        return int(self.lib.aln_scan_string_stride(h, a["W"], C.byref(g)))

    def score(self, which, a, f):
        h, p, g, _keep = self.handles(which, a)
        return self.lib.aln_scan_score(h, C.byref(p), C.byref(g), f.ctypes.data)

    def select(self, which, a, cap, count, idx, res, tb):
        h, p, g, _keep = self.handles(which, a)
        return self.lib.aln_scan_select(h, C.byref(p), C.byref(g), a["mean"], a["sd"], a["z"], cap, count.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        idx.ctypes.data, res.ctypes.data, tb.ctypes.data)

    def hits(self, which, a, count):
        h, p, g, _keep = self.handles(which, a)
        return self.lib.aln_scan_hits(h, C.byref(p), C.byref(g), a["mean"], a["sd"], a["z"], count.ctypes.data_as(C.POINTER(C.c_uint64)))

    def held_list(self, which, first, n, idx, f):
        return self.lib.aln_scan_held_list(self.scans[which].h, first, n, idx.ctypes.data, f.ctypes.data)

    def held_frequencies(self, which, keep, counts):
        return self.lib.aln_scan_held_frequencies(self.scans[which].h, _ptr(keep), len(keep), counts.ctypes.data)

    def held_strings(self, which, keep, res, tb):
        return self.lib.aln_scan_held_strings(self.scans[which].h, _ptr(keep), len(keep), res.ctypes.data, tb.ctypes.data)


# ---------------------------------------------------------------- the salt wrap: more than 1024 + 50 launches on one scan's slot
WRAP_LEN, WRAP_GEOM, WRAP_PASSES, WRAP_Z = 1001, (30, 4.0, 1.0, 0, 7, 40), 1100, 1.0
WRAP_PWM_SEEDS = (101, 102, 103)


def wrap_args(orc, seed=SEED):
    """[arguments of the held pass of PWM A, B, C] and the expected arrays of a score and of a held pass with each: three references"""
    chrom = chromosome(seed, WRAP_LEN)
    sc = HB.MemoOracleScan(chrom)
    W, d, e, first, step, width = WRAP_GEOM
    n = n_windows(WRAP_LEN, first, step)
    args, wants = [], {}
    for k, pseed in enumerate(WRAP_PWM_SEEDS):
        m = pwm("int", W, pseed)
        recs = [sc._align(w, m, d, e) for _k, w in sc._windows(first, step, width, False)]
        f = np.array([r["f"] for r in recs], dtype=np.float64)
        a = dict(name="wrap%d" % k, kind="int", W=W, pwm_seed=pseed, d=d, e=e, first=first, step=step, width=width, reverse=0, mean=float(np.mean(f)),
                 sd=float(np.std(f)), z=WRAP_Z, cap=n, n=n, which=0, semantics=PWM_LOCAL, length=WRAP_LEN)
        idx = np.flatnonzero((f - np.float64(a["mean"])) / np.float64(a["sd"]) >= np.float64(WRAP_Z))
        hit = [recs[int(i)] for i in idx]
        a["lengths"] = window_lengths(WRAP_LEN, first, step, width, idx).tolist()
        args.append(a)
        wants["score-%d" % k] = dict(ret=np.asarray(OK), f=bits(marked_with(n + PAD, np.float64, f)))
        held = dict(ret=np.asarray(OK), count=np.asarray(len(idx)), idx=marked_with(len(idx) + PAD, np.uint32, idx),
                    f=bits(marked_with(len(idx) + PAD, np.float64, f[idx])))
        held.update(Refs.summaries(hit, len(idx) + PAD, "int"))
        held.update(Refs.strings(hit))
        wants["hits-%d" % k] = held
    return args, wants


def child_wrap(job, wants):
    """A, B, C, A, .. (1024 is no multiple of 3), score and held pass in turn: all six combinations, every pass against the oracle"""
    import time
    chrom = chromosome(job["seed"], WRAP_LEN)
    b = Backend(GpuAbi([chrom]))
    bad, launches, t0 = [], 0, time.perf_counter()
    for n in range(job["passes"]):
        k, a = n % 3, job["args"][n % 3]
        if n % 2 == 0:
            got, want = b.do_score(a), wants["score-%d" % k]
            launches += 1
        else:
            got, want = b.do_hits(a), wants["hits-%d" % k]
            launches += 2 if int(want["count"]) else 1
            if int(got["ret"]) == OK and int(got["count"]) == int(want["count"]):
                cnt = int(got["count"])
                lst = b.do_list(dict(first=0, n=cnt))
                got.update({key: v for key, v in b.do_strings(dict(keep=list(range(cnt)), lengths=a["lengths"], W=a["W"], width=a["width"])).items()
                            if key != "ret" or int(v) != OK})
                got.update({key: v for key, v in lst.items() if key != "ret" or int(v) != OK})
        diff = check(got, want, None)
        if diff is not None:
            bad.append([n, k, diff])
            if int(got["ret"]) in (DEVICE, OOM):
                break
    b.close()
    return dict(passes=n + 1, launches=launches, bad=len(bad), first_bad=bad[:10], seconds=time.perf_counter() - t0,
                windows=job["args"][0]["n"])


# ---------------------------------------------------------------- the child process of tests/test_scan_history_gpu.py
# python scan_history.py MODE job.json report.json: one mode in a process (and so a context and a plan cache) of its own, every call
# held against the expected values the parent computed from the oracle; the parent asserts on the report.  MODE: walk | destroy | wrap.
def main(argv):
    import time
    mode, job_path, report = argv
    with open(job_path) as f:
        job = json.load(f)
    if mode == "wrap":
        out = child_wrap(job, CH.load_expected(job["expected"]))
    else:
        out = dict(walks=[])
        for part in job["parts"]:
            wants = CH.load_expected(part["expected"])
            backend = Backend(GpuAbi([chromosome(part["seed"], part["length"]), chromosome(part["other_seed"], part["length"])]))
            t0 = time.perf_counter()
            w = walk(backend, part["plan"], wants)
            w["seconds"], w["library_seconds"] = time.perf_counter() - t0, backend.seconds
            backend.close()                      # (destroy: aln_scan_destroy half-way; the next scan lives on the same context)
            out["walks"].append(w)
            if any("the walk ends here" in x["message"] for x in w["failures"]):
                break
    with open(report, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1:])
