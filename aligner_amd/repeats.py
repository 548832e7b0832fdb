"""latent-repeat-search on the GPU: dispersed repeats in chromosomes by an iterated position-weight matrix.

Restatement of aligner-core/src/bin/latent-repeat-search (args.rs, main.rs, engine/{calc,mod,sequences}.rs,
cmd/{testing,exploring,csv}.rs).  Per FASTA record:

  1. a random PWM (lib.rs:92-96), transformed to the record's residue frequencies; the mean and standard deviation of f over
     windows of a SHUFFLED copy of the chromosome (calculate_starting_values)
  2. every window j = 0, qo, 2 qo, ... (rows seq[j .. min(j + rl + qo, len))): z = (f - mean) / std, kept when z >= 3 (calculate_cycle)
  3. overlapping hits dropped (filter)
  4. mean, std (the VARIANCE, calc.rs:198-203) and the PWM re-estimated from the hits' frequency matrices; back to 2, up to
     --repeats times
  5. with --reverse, one cycle on the reversed chromosome with the final PWM (key "<head>-reversed")

The windows are aligned by a scoring backend with two passes over a resident chromosome: `score` (f of every window of a
geometry) and `select` (the windows with z >= z_min, with their alignments).  ScanBackend is the GPU one (aln_scan_*: the
chromosome is uploaded once, windows are expanded on the device, only the hits come back).  A scan that also offers `hits` (the
GPU one by default) keeps a cycle's hits on the device: window numbers and f come back, the overlap filter runs on arrays
(filter_hits), the kept hits' frequency matrices are summed on the device, and alignment strings are fetched for kept hits only.  Randomness comes from a
numpy.random.Generator; sums run left to right in ascending window order (the reference's order with its default of one thread).
`python -m aligner_amd.repeats` is the program.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

from . import _ffi, runtime
from .batch import RESULT_DTYPE
from .enums import DNA
from .errors import ReferencePanic
from .heuristic import HeuristicPWMAligner, WrongMatrixSpecified, transform_matrix
from .pwm import PWMAlignment
from .simple import Heuristics

Z = 3.0                                  # calc.rs:17
TEST_SEQUENCE_LENGTH = 100000            # cmd/testing.rs:10
DESCENDANTS_AMOUNT = 10                  # cmd/testing.rs:11
QUARTER = 4                              # MutationPercent::Quarter (engine/mod.rs:12-15)


# ---------------------------------------------------------------- options (args.rs, cmd/mod.rs:20-88)
class Options:
    def __init__(self, repeat_length=300, query_offset=30, deletions=30.0, extension=7.0, rsquared=100000.0, kd=0.0, threads=1,
                 repeats=10, simple_init=False, reverse=False, fasta_path=None, csv_path=None):
        self.repeat_length, self.query_offset = int(repeat_length), int(query_offset)
        self.deletions, self.extension = float(deletions), float(extension)
        self.rsquared, self.kd = float(rsquared), float(kd)
        self.threads, self.repeats = int(threads), int(repeats)
        self.simple_init, self.reverse = bool(simple_init), bool(reverse)
        self.fasta_path, self.csv_path = fasta_path, csv_path
        self.testing = fasta_path is None
        self.csv = csv_path is not None

    @property
    def width(self):
        return self.repeat_length + self.query_offset


class Task:
    """engine/task.rs: equality compares left_coord only."""
    __slots__ = ("alignment", "left_coord", "right_coord", "z")

    def __init__(self, alignment, left_coord, right_coord, z):
        self.alignment, self.left_coord, self.right_coord, self.z = alignment, int(left_coord), int(right_coord), z

    def __eq__(self, other):
        return self.left_coord == other.left_coord

    def __repr__(self):
        return "Task(z=%r, left_coord=%d, right_coord=%d)" % (self.z, self.left_coord, self.right_coord)


# ---------------------------------------------------------------- engine/mod.rs
def get_random_pwm(length, rng):
    """lib.rs:92-96: 4 x length, every entry drawn from {-1, 0, 1}, row-major."""
    return rng.integers(-1, 2, size=(4, int(length))).astype(np.float64)


def generate_descendants(sequence, amount, percent, rng):
    """engine/mod.rs:17-47: descendant i re-draws every `percent`-th residue from position i on."""
    out = []
    for i in range(amount):
        d = np.array(sequence, dtype=np.uint8, copy=True)
        for k in range(i, len(d), percent):
            d[k] = rng.integers(0, DNA.volume())
        out.append(d)
    return out


def check_intersection(c1, c2):
    """engine/mod.rs:104-119, as written (the fourth test repeats the first)."""
    if c2[0] <= c1[0] <= c2[1]:
        return True
    if c2[0] <= c1[1] <= c2[1]:
        return True
    if c2[0] >= c1[0] and c2[1] <= c1[1]:
        return True
    if c2[0] <= c1[0] <= c2[1]:
        return True
    return False


def filter_tasks(tasks):
    """engine/mod.rs:49-102: stable sort by left_coord; each cluster = the first task and the run of tasks that intersect IT;
    the best z of a cluster is kept (the last of equal ones); the scan then resumes at the last task the inner loop looked at
    (so the last task of a run that overlaps to the end is looked at again); `contains` compares left_coord only."""
    tasks = list(tasks)
    if not tasks:
        return []
    if len(tasks) == 1:
        return tasks[:]
    result = []
    tasks.sort(key=lambda t: t.left_coord)
    lo = 0                                       # tasks[lo:] is the reference's `tasks` (re-sliced there; an offset here)
    while lo < len(tasks):
        if len(tasks) - lo == 1:
            if tasks[lo] not in result:
                result.append(tasks[lo])
            break
        current = tasks[lo]
        batch = [current]
        index = 0
        for i in range(len(tasks) - lo - 1):
            task = tasks[lo + 1 + i]
            index = i
            if check_intersection((current.left_coord, current.right_coord), (task.left_coord, task.right_coord)):
                batch.append(task)
            else:
                break
        if len(batch) == 1:
            result.append(batch[0])
        else:
            best = batch[0]
            for t in batch[1:]:                  # Iterator::max_by: the LAST of equal maxima
                if _partial_cmp(t.z, best.z) >= 0:
                    best = t
            result.append(best)
        lo += index + 1
    return result


def filter_hits(left, right, z):
    """filter_tasks on plain arrays: -> the positions (in the input) of the hits it keeps, in its order.  The same stable sort by
    left_coord, clusters, last of equal maxima, resume-at-the-last-looked-at and ReferencePanic on a NaN comparison."""
    left = np.asarray(left, dtype=np.int64)
    n = len(left)
    if n <= 1:
        return np.arange(n, dtype=np.int64)
    order = np.argsort(left, kind="stable")
    L = left[order].tolist()
    Rt = np.asarray(right, dtype=np.int64)[order].tolist()
    Zs = np.asarray(z, dtype=np.float64)[order].tolist()
    result, seen = [], set()                     # positions in sorted order; the left_coords in `result` (Task equality)
    lo = 0
    while lo < n:
        if n - lo == 1:
            if L[lo] not in seen:
                result.append(lo)
            break
        cur = (L[lo], Rt[lo])
        best, index = lo, 0
        for i in range(n - lo - 1):
            p = lo + 1 + i
            index = i
            if not check_intersection(cur, (L[p], Rt[p])):
                break
            if _partial_cmp(Zs[p], Zs[best]) >= 0:       # Iterator::max_by: the LAST of equal maxima
                best = p
        result.append(best)
        seen.add(L[best])
        lo += index + 1
    return order[np.asarray(result, dtype=np.int64)]


def _partial_cmp(a, b):
    if a != a or b != b:
        raise ReferencePanic(-1, "called `Option::unwrap()` on a `None` value (partial_cmp of NaN, engine/mod.rs:92)")
    return (a > b) - (a < b)


def index_coord(target, indices):
    """engine/mod.rs:121-129: the first index (they are in descending coord) at or below target shifts it by its offset."""
    for index in indices:
        if target >= index.coord:
            return target + index.offset
    return target


def rotate_indices(indices, query_length):
    """engine/mod.rs:131-152."""
    from .enums import Index
    if not indices:
        return []
    ref = indices[0]
    full_length = query_length + ref.offset
    out, offset = [], 0
    for index in indices:
        offset += index.local_offset
        coord = full_length - index.coord - ref.offset
        if coord < 0:
            raise ReferencePanic(-1, "attempt to subtract with overflow (rotate_indices)")
        out.append(Index(coord, offset, index.local_offset))
    out.reverse()
    return out


# ---------------------------------------------------------------- sums in the reference's order
def seq_sum(values):
    """`iter().sum::<f64>()`: one addition after the other, left to right (not numpy's pairwise sum)."""
    v = np.asarray(values, dtype=np.float64)
    return np.float64(np.cumsum(v)[-1]) if len(v) else np.float64(0.0)


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(a) / np.float64(b)


def mean_and_variance(fs):
    """calc.rs:197-202: sum / n and sum((f - mean)^2) / n, both sequential."""
    fs = np.asarray(fs, dtype=np.float64)
    mean = _div(seq_sum(fs), len(fs))
    d = fs - mean
    return mean, _div(seq_sum(d * d), len(fs))


# ---------------------------------------------------------------- window sets
def starting_window_starts(length, opts):
    """calc.rs:37-54: per thread i, range(i * qo, len, step * threads) with step = qo or len / 1000 (--simple-init);
    returned as one ascending list (with repeats, if the threads' ranges meet)."""
    step = length // 1000 if opts.simple_init else opts.query_offset
    parts = []
    for i in range(opts.threads):
        if step * opts.threads == 0:
            raise ReferencePanic(-1, "assertion failed: step != 0 (step_by(0), calc.rs:53)")
        parts.append(np.arange(i * opts.query_offset, length, step * opts.threads, dtype=np.int64))
    if not parts:
        return np.zeros(0, dtype=np.int64), []
    starts = np.concatenate(parts)
    order = np.argsort(starts, kind="stable")
    geoms = [(i * opts.query_offset, step * opts.threads) for i in range(opts.threads)]
    return starts[order], (geoms, order)


def cycle_step(opts):
    """calc.rs:107-114: the threads' ranges together are every multiple of qo below len, whatever --threads is."""
    if opts.query_offset * opts.threads == 0:
        if opts.threads == 0:
            return None
        raise ReferencePanic(-1, "assertion failed: step != 0 (step_by(0), calc.rs:114)")
    return opts.query_offset


# ---------------------------------------------------------------- engine/calc.rs
def calculate_starting_values(query, matrix, opts, rng, backend):
    """calc.rs:19-86: f over windows of a shuffled copy; returns (mean, sqrt(variance))."""
    shuffled = np.array(query, dtype=np.uint8, copy=True)
    rng.shuffle(shuffled)
    length = len(shuffled)
    starts, plan = starting_window_starts(length, opts)
    if len(starts) == 0:
        fs = np.zeros(0)
    else:
        geoms, order = plan
        with backend.scan(shuffled) as sc:
            parts = [sc.score(matrix, opts.deletions, opts.extension, first, step, opts.width) for first, step in geoms]
        fs = np.concatenate(parts)[order]
    mean, var = mean_and_variance(fs)
    return mean, np.sqrt(var)


def calculate_cycle(query, matrix, indices, mean, std, opts, backend, reverse=False, scan=None):
    """calc.rs:88-147: every window j = k * qo; the tasks with z >= 3 in ascending window order.  `reverse`: the windows of the
    reversed query (the scan holds the forward one)."""
    length = len(query)
    step = cycle_step(opts)
    if step is None or length == 0:
        return []
    own = scan is None
    sc = backend.scan(query) if own else scan
    try:
        if hasattr(sc, "hits"):
            return _HeldCycle(sc, query, matrix, indices, mean, std, opts, reverse).tasks()
        idx, alns = sc.select(matrix, opts.deletions, opts.extension, 0, step, opts.width, mean, std, Z, reverse=reverse)
    finally:
        if own:
            sc.close()
    tasks = []
    for k, aln in zip(idx, alns):
        j = int(k) * step
        border = min(j + opts.width, length)
        z = _div(np.float64(aln.f) - np.float64(mean), std)
        tasks.append(Task(aln, index_coord(j, indices), index_coord(border, indices), float(z)))
    return tasks


class _HeldCycle:
    """One cycle on a scan that holds its hits (`hits`): window numbers and f as arrays, z and coordinates from them; alignment
    strings are fetched (`fetch`, raw bytes) for the positions asked for, and Task / PWMAlignment objects are built by `tasks`
    only.  The held state lasts until the scan's next pass: `fetch` what is to outlive it before that."""

    def __init__(self, sc, query, matrix, indices, mean, std, opts, reverse=False):
        length, step = len(query), cycle_step(opts)
        self.held = sc.hits(matrix, opts.deletions, opts.extension, 0, step, opts.width, mean, std, Z, reverse=reverse)
        self.f = self.held.f
        j = self.held.idx * step
        border = np.minimum(j + opts.width, length)
        if indices:
            self.left = np.array([index_coord(int(v), indices) for v in j], dtype=np.int64)
            self.right = np.array([index_coord(int(v), indices) for v in border], dtype=np.int64)
        else:
            self.left, self.right = j.astype(np.int64), border.astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.z = (self.f - np.float64(mean)) / np.float64(std)
        self.kept = np.arange(len(self.f), dtype=np.int64)
        self._alns = None

    def __len__(self):
        return len(self.f)

    def keep(self, positions):
        self.kept = np.asarray(positions, dtype=np.int64)
        self._alns = None

    def fetch(self):
        """The kept hits' summaries and strings off the device (no objects yet)."""
        if self._alns is None:
            strings = getattr(self.held, "strings", None)     # a scan without `strings` hands over the objects at once
            self._alns = strings(self.kept) if strings else _Ready(self.held.alignments(self.kept))

    def tasks(self):
        self.fetch()
        alns = self._alns.alignments()
        return [Task(a, self.left[k], self.right[k], float(self.z[k])) for a, k in zip(alns, self.kept)]


class _Ready:
    def __init__(self, alns):
        self._alns = alns

    def alignments(self):
        return self._alns


def _transform(matrix, opts, freqs):
    try:
        return transform_matrix(matrix, 0.0, opts.deletions * opts.extension, freqs)
    except WrongMatrixSpecified:
        raise ReferencePanic(-1, "called `Result::unwrap()` on an `Err` value: WrongMatrixSpecified") from None


def perform_calculation_per_sequence(opts, raw_seq, head, rng, backend):
    """calc.rs:149-241 -> {"direct": (tasks, matrix)[, "inverse": (tasks, matrix)]}."""
    query, freqs, indices = DNA.from_u8_vec_with_freqs_and_indices(raw_seq)
    matrix = _transform(get_random_pwm(opts.repeat_length, rng), opts, freqs)
    mean, std = calculate_starting_values(query, matrix, opts, rng, backend)
    result = {}
    tasks = []
    with backend.scan(query) as sc:
        if hasattr(sc, "hits"):
            return _held_calculation(opts, query, freqs, indices, matrix, mean, std, sc)
        for i in range(opts.repeats):
            new_tasks = calculate_cycle(query, matrix, indices, mean, std, opts, backend, scan=sc)
            if not new_tasks:
                break
            tasks = filter_tasks(new_tasks)
            if i < opts.repeats - 1:
                mean, std = mean_and_variance([t.alignment.f for t in tasks])     # std is the variance here (calc.rs:198-203)
                m = np.zeros(matrix.shape, dtype=np.float64)
                for t in tasks:
                    m = m + t.alignment.get_frequency_matrix()
                matrix = _transform(m, opts, freqs)
        result["direct"] = (tasks, matrix.copy())
        if opts.reverse:
            rotated = rotate_indices(indices, len(query))
            inv = calculate_cycle(query, matrix, rotated, mean, std, opts, backend, reverse=True, scan=sc)
            result["inverse"] = (filter_tasks(inv), matrix)
    return result


def _held_calculation(opts, query, freqs, indices, matrix, mean, std, sc):
    """The loop of perform_calculation_per_sequence on a scan that holds its hits.  Per cycle: hits -> filter_hits -> mean and
    variance of the kept f -> the kept hits' frequency sum from the device -> the next PWM.  The kept hits' strings are fetched
    before the next pass replaces the held state (also when that pass then finds nothing and these are the tasks returned);
    Task and PWMAlignment objects are built for the cycle that is returned only."""
    def cycle(indices, reverse=False):
        if cycle_step(opts) is None or len(query) == 0:          # calculate_cycle's empty cases
            return None
        return _HeldCycle(sc, query, matrix, indices, mean, std, opts, reverse)

    result = {}
    last = None
    for i in range(opts.repeats):
        cyc = cycle(indices)
        if cyc is None or not len(cyc):
            break
        cyc.keep(filter_hits(cyc.left, cyc.right, cyc.z))
        if i < opts.repeats - 1:
            mean, std = mean_and_variance(cyc.f[cyc.kept])                  # std is the variance here (calc.rs:198-203)
            matrix = _transform(cyc.held.frequencies(cyc.kept), opts, freqs)
        cyc.fetch()
        last = cyc
    result["direct"] = (last.tasks() if last is not None else [], matrix.copy())
    if opts.reverse:
        cyc = cycle(rotate_indices(indices, len(query)), reverse=True)
        inv = []
        if cyc is not None:
            cyc.keep(filter_hits(cyc.left, cyc.right, cyc.z))
            inv = cyc.tasks()
        result["inverse"] = (inv, matrix)
    return result


# ---------------------------------------------------------------- cmd/*.rs
def run_testing(opts, rng, backend):
    """cmd/testing.rs:13-75: a random chromosome with ten mutated copies of a sample planted in it; starting values and
    exactly one cycle, unfiltered, under "test"."""
    sequence_raw = DNA.random_seq(TEST_SEQUENCE_LENGTH, rng)
    query, freqs = DNA.random_seq_with_freqs(opts.repeat_length + opts.query_offset, rng)
    matrix = get_random_pwm(opts.repeat_length, rng)
    result = HeuristicPWMAligner.from_seqs(query, None, DNA).perform_alignment(
        opts.deletions, opts.extension, matrix, Heuristics(opts.kd, opts.rsquared, freqs))
    matrix = np.asarray(result.matrix, dtype=np.float64)
    descendants = generate_descendants(query, DESCENDANTS_AMOUNT, QUARTER, rng)
    offset = len(sequence_raw) // (len(descendants) + 1)
    parts = [sequence_raw[:offset]]
    for i, d in enumerate(descendants):                # testing.rs:51-55: the first chunk appears twice
        parts.append(d)
        parts.append(sequence_raw[offset * i:offset * (i + 1)])
    sequence = np.concatenate(parts).astype(np.uint8)
    mean, std = calculate_starting_values(sequence, matrix, opts, rng, backend)
    return {"test": (calculate_cycle(sequence, matrix, [], mean, std, opts, backend), matrix)}


def read_records_csv(path):
    """aligner-helpers csv::read_csv: name,z_value,left_coord,right_coord -> {name: [(left, right), ...]}."""
    import csv
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            out.setdefault(row["name"], []).append((int(row["left_coord"]), int(row["right_coord"])))
    return out


def prepare_sequence(raw_seq, records):
    """engine/sequences.rs:33-43: [left, right) of every record set to 'N'."""
    b = bytearray(raw_seq)
    for left, right in records:
        if left > right or right > len(b):
            raise ReferencePanic(-1, "slice index out of range (prepare_sequence, sequences.rs:37)")
        b[left:right] = b"N" * (right - left)
    return bytes(b)


def run_fasta(opts, rng, backend):
    """cmd/exploring.rs / cmd/csv.rs: per record, keys "<head>" and "<head>-reversed", in FASTA order."""
    from .fasta import read_fasta
    records = read_fasta(opts.fasta_path)
    if not records:
        raise ValueError("empty fasta file")
    masks = read_records_csv(opts.csv_path) if opts.csv else {}
    result = {}
    for rec in records:
        head = rec.head.decode("utf-8")
        seq = prepare_sequence(rec.seq, masks[head]) if head in masks else rec.seq
        r = perform_calculation_per_sequence(opts, seq, head, rng, backend)
        if "direct" in r:
            result[head] = r["direct"]
        if "inverse" in r:
            result["%s-reversed" % head] = r["inverse"]
    return result


def run(opts, rng, backend):
    """cmd/mod.rs:90-98."""
    if opts.testing:
        return run_testing(opts, rng, backend)
    return run_fasta(opts, rng, backend)


# ---------------------------------------------------------------- output (main.rs)
def output_paths(output, cwd=None):
    cwd = os.getcwd() if cwd is None else cwd
    if output is None:
        return os.path.join(cwd, "output.csv"), os.path.join(cwd, "matrices.json")
    return output, "%s.matrices.json" % output


def write_outputs(result, csv_path, json_path):
    """The CSV (header name,z_value,left_coord,right_coord; z in shortest round-trip form) and the matrices in ndarray's serde
    form {"v":1,"dim":[rows,cols],"data":[...]}."""
    with open(csv_path, "w", newline="") as f:
        f.write("name,z_value,left_coord,right_coord\n")
        for key, (tasks, _m) in result.items():
            for t in tasks:
                f.write("%s,%s,%d,%d\n" % (_csv_field(key), _float_text(t.z), t.left_coord, t.right_coord))
    mats = {key: {"v": 1, "dim": [int(m.shape[0]), int(m.shape[1])], "data": [_json_float(x) for x in np.asarray(m).ravel()]}
            for key, (_t, m) in result.items()}
    with open(json_path, "w") as f:
        f.write(json.dumps(mats, separators=(",", ":"), allow_nan=False))


def _csv_field(s):
    if any(ch in s for ch in ',"\n\r'):
        return '"%s"' % s.replace('"', '""')
    return s


def _float_text(x):
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    return repr(x)


def _json_float(x):
    x = float(x)
    return x if np.isfinite(x) else None       # serde_json writes a non-finite f64 as null


# ---------------------------------------------------------------- the GPU backend: aln_scan_*
class ScanBackend:
    """Scores windows on the GPU through aln_scan_*: `scan(seq)` uploads a chromosome once; its passes send the PWM and a
    geometry and get back f of every window (score) or the hits only (select)."""

    def __init__(self, device=None, cap=4096, held=True):
        self.device, self.cap, self.held = device, int(cap), bool(held)

    def scan(self, seq):
        return (HeldGpuScan if self.held else GpuScan)(seq, self.device, self.cap)


class GpuScan:
    def __init__(self, seq, device=None, cap=4096):
        self.lib = _ffi.load()
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.len = len(self.seq)
        self.cap = max(1, int(cap))
        st = C.c_int(0)
        self.h = self.lib.aln_scan_create(runtime.context(device), self.seq.ctypes.data, self.len, C.byref(st))
        if not self.h:
            runtime.raise_for_status(st.value, "aln_scan_create")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if getattr(self, "h", None):
            self.lib.aln_scan_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @staticmethod
    def _geometry(first, step, width, reverse):
        return _ffi.ScanGeometry(int(first), int(step), int(width), 1 if reverse else 0, 0)

    def windows(self, first, step, width):
        if step == 0:
            raise ValueError("step must be positive")
        return (self.len - 1 - first) // step + 1 if first < self.len else 0

    def score(self, matrix, del_, ext, first, step, width, reverse=False):
        p, keep = runtime.make_params(_ffi.PWM_LOCAL, del_, ext, matrix, outputs=_ffi.OUT_SCORE)
        g = self._geometry(first, step, width, reverse)
        f = np.zeros(self.windows(first, step, width), dtype=np.float64)
        st = self.lib.aln_scan_score(self.h, C.byref(p), C.byref(g), f.ctypes.data)
        runtime.raise_for_status(st, "aln_scan_score")
        return f

    def select(self, matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=False, cap=None):
        """-> (window indices ascending, [PWMAlignment]) of the windows with (f - mean) / sd >= z_min."""
        m = np.asarray(matrix, dtype=np.float64)
        p, keep = runtime.make_params(_ffi.PWM_LOCAL, del_, ext, m)
        g = self._geometry(first, step, width, reverse)
        n = self.windows(first, step, width)
        cap = max(1, min(int(cap or self.cap), max(n, 1)))
        while True:
            idx, res, tb, count, stride = self._select_raw(p, g, mean, sd, z_min, cap)
            if count <= cap:
                break
            cap = count                                    # more hits than room: again, with room for all of them,
            self.cap = max(self.cap, count)                # and that room from now on (the next cycles keep about as many)
        idx = idx[:count].astype(np.int64)
        lengths = np.minimum(width, self.len - (first + idx * step))
        return idx, self._alignments(res[:count], tb, stride, lengths, m.shape[1])

    def select_raw(self, matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=False, cap=1024):
        """One select pass as the C ABI returns it: (indices, results, strings, true count, string stride, status)."""
        p, keep = runtime.make_params(_ffi.PWM_LOCAL, del_, ext, matrix)
        return self._select_raw(p, self._geometry(first, step, width, reverse), mean, sd, z_min, cap, check=False)

    def _select_raw(self, p, g, mean, sd, z_min, cap, check=True):
        W = p.cols
        stride = int(self.lib.aln_scan_string_stride(self.h, W, C.byref(g)))
        idx = np.zeros(cap, dtype=np.uint32)
        res = np.zeros(cap, dtype=RESULT_DTYPE)
        tb = np.zeros(stride * cap + 8, dtype=np.uint8)
        count = C.c_uint64(0)
        st = self.lib.aln_scan_select(self.h, C.byref(p), C.byref(g), float(mean), float(sd), float(z_min), cap, C.byref(count),
                                      idx.ctypes.data, res.ctypes.data, tb.ctypes.data)
        if not check:
            return idx, res, tb, int(count.value), stride, st
        if st != _ffi.ERR_CAPACITY:
            runtime.raise_for_status(st, "aln_scan_select")
        return idx, res, tb, int(count.value), stride

    @staticmethod
    def _alignments(res, tb, stride, lengths, W):
        """PWMAlignment objects out of summaries and strings in the layout of aln_scan_select (entry h at h * stride; its residues
        at 4 * (W + that window's length + 2))."""
        alns = []
        for h in range(len(res)):
            r = res[h]
            L, o, c = int(r["aln_len"]), h * stride, W + int(lengths[h]) + 2
            numbered = tb[o:o + 4 * L].view(np.uint32).copy()
            qal = tb[o + 4 * c:o + 4 * c + L].copy()
            coords = ((int(r["start_x"]) + 1, int(r["end_x"]) + 1), (int(r["start_y"]) + 1, int(r["end_y"]) + 1))
            alns.append(PWMAlignment(DNA, numbered, qal, W, coords, float(r["f"])))
        return alns

    def stats(self):
        """The last pass: kernel ms (fill, selection, hit re-fill + walk), download wall ms, bytes host->device, device->host."""
        ms = (C.c_double * 4)()
        by = (C.c_uint64 * 2)()
        self.lib.aln_scan_stats(self.h, ms, by)
        return dict(fill_ms=ms[0], select_ms=ms[1], refill_ms=ms[2], download_ms=ms[3], h2d_bytes=by[0], d2h_bytes=by[1])


class HeldGpuScan(GpuScan):
    """A GpuScan that also offers `hits`: a select pass whose hits stay on the device (aln_scan_hits)."""

    generation = 0                                   # counts the passes: held hits are those of the last one only

    def score(self, *a, **kw):
        self.generation += 1
        return GpuScan.score(self, *a, **kw)

    def _select_raw(self, *a, **kw):
        self.generation += 1
        return GpuScan._select_raw(self, *a, **kw)

    def hits(self, matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=False):
        """-> HeldHits: the windows with (f - mean) / sd >= z_min, held on the device until this scan's next pass."""
        m = np.asarray(matrix, dtype=np.float64)
        p, keep = runtime.make_params(_ffi.PWM_LOCAL, del_, ext, m)
        g = self._geometry(first, step, width, reverse)
        self.generation += 1
        count = C.c_uint64(0)
        st = self.lib.aln_scan_hits(self.h, C.byref(p), C.byref(g), float(mean), float(sd), float(z_min), C.byref(count))
        runtime.raise_for_status(st, "aln_scan_hits")
        n = int(count.value)
        idx = np.zeros(n, dtype=np.uint32)
        f = np.zeros(n, dtype=np.float64)
        st = self.lib.aln_scan_held_list(self.h, 0, n, idx.ctypes.data, f.ctypes.data)
        runtime.raise_for_status(st, "aln_scan_held_list")
        stride = int(self.lib.aln_scan_string_stride(self.h, m.shape[1], C.byref(g)))
        idx = idx.astype(np.int64)
        lengths = np.minimum(int(width), self.len - (int(first) + idx * int(step)))
        return HeldHits(self, idx, f, m.shape[1], stride, lengths)


class HeldHits:
    """The hits of one held pass: `idx` (window numbers, ascending) and `f`; `frequencies(keep)`, `strings(keep)` and
    `alignments(keep)` take positions in this list and work on what the device holds, until the scan's next pass."""

    def __init__(self, scan, idx, f, W, stride, lengths):
        self.scan, self.idx, self.f, self.W, self.stride, self.lengths = scan, idx, f, int(W), int(stride), lengths
        self.generation = scan.generation

    def __len__(self):
        return len(self.idx)

    def _keep(self, keep):
        if self.generation != self.scan.generation or not self.scan.h:
            raise RuntimeError("the held hits have been replaced by a later pass on this scan")
        keep = np.asarray(keep, dtype=np.int64).ravel()
        if len(keep) and (keep.min() < 0 or keep.max() >= len(self.idx)):
            raise IndexError("position outside the held hits")
        return np.ascontiguousarray(keep, dtype=np.uint32)

    def frequencies(self, keep):
        """The sum of the listed hits' frequency matrices (PWMAlignment.get_frequency_matrix), float64 (4, W)."""
        k = self._keep(keep)
        out = np.zeros((4, self.W), dtype=np.float64)
        st = self.scan.lib.aln_scan_held_frequencies(self.scan.h, k.ctypes.data, len(k), out.ctypes.data)
        runtime.raise_for_status(st, "aln_scan_held_frequencies")
        return out

    def strings(self, keep):
        """The listed hits' summaries and strings as they come off the device -> HeldStrings."""
        k = self._keep(keep)
        res = np.zeros(len(k), dtype=RESULT_DTYPE)
        tb = np.zeros(self.stride * len(k) + 8, dtype=np.uint8)
        st = self.scan.lib.aln_scan_held_strings(self.scan.h, k.ctypes.data, len(k), res.ctypes.data, tb.ctypes.data)
        runtime.raise_for_status(st, "aln_scan_held_strings")
        return HeldStrings(res, tb, self.stride, self.lengths[k.astype(np.int64)], self.W)

    def alignments(self, keep):
        return self.strings(keep).alignments()


class HeldStrings:
    def __init__(self, res, tb, stride, lengths, W):
        self.res, self.tb, self.stride, self.lengths, self.W = res, tb, stride, lengths, W

    def alignments(self):
        return GpuScan._alignments(self.res, self.tb, self.stride, self.lengths, self.W)


# ---------------------------------------------------------------- CLI (args.rs, main.rs)
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="latent-repeat-search")
    ap.add_argument("-i", "--input")
    ap.add_argument("-o", "--output")
    ap.add_argument("--csv")
    ap.add_argument("-d", "--deletions", type=float, default=30.0)
    ap.add_argument("-e", "--extension", type=float, default=7.0)
    ap.add_argument("--rsquared", type=float, default=100000.0)
    ap.add_argument("--kd", type=float, default=0.0)
    ap.add_argument("-q", "--query-offset", type=int, default=30)
    ap.add_argument("-r", "--repeat-length", type=int, default=300)
    ap.add_argument("--threads", type=int, default=1)
    ap.add_argument("--simple-init", action="store_true")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--reverse", action="store_true")
    ap.add_argument("--seed", type=int, default=None, help="seed of the random generator (runs with the same seed are the same)")
    return ap.parse_args(argv)


def options_from_args(a):
    return Options(repeat_length=a.repeat_length, query_offset=a.query_offset, deletions=a.deletions, extension=a.extension,
                   rsquared=a.rsquared, kd=a.kd, threads=a.threads, repeats=a.repeats, simple_init=a.simple_init,
                   reverse=a.reverse, fasta_path=a.input, csv_path=a.csv)


def main(argv=None, backend=None):
    a = parse_args(argv)
    opts = options_from_args(a)
    csv_path, json_path = output_paths(a.output)
    rng = np.random.default_rng(a.seed)
    result = run(opts, rng, backend or ScanBackend())
    write_outputs(result, csv_path, json_path)
    print("\nOutput written to:\n 1. Result: %s\n 2. Matrices: %s" % (csv_path, json_path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
