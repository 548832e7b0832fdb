"""A set of pairs resident in HBM, aligned again and again under per-pair matrices (aln_pairset_*, include/aligner_hip.h).

The device-resident form of the loop of HeuristicAligner (aligner-core/src/heuristic/mod.rs:36-78) for many pairs at once:
`run` aligns the listed pairs, each under a real-valued matrix of its own, and leaves the walked strings on the device;
`frequencies` counts Alignment::get_frequency_matrix (alignment.rs:13-23) there for the pairs that go on, `strings` fetches
the pairs that are done.  heuristic.align_many drives it.

The matrices can stay in HBM as well: `set_heuristics` uploads every pair's transform parameters once, `reestimate` rebuilds the
listed pairs' matrices on the device (from one shared matrix, or from the counts of their held strings) into a resident store,
`run_stored` aligns under the store's entries and `matrices` downloads the entries of the pairs that are done.
"""
import ctypes as C

import numpy as np

from . import _ffi
from . import runtime
from .batch import RESULT_DTYPE, PairBatch


class PairSet:
    def __init__(self, pairs, device=None):
        self.lib = _ffi.load()
        self.batch = pairs if isinstance(pairs, PairBatch) else PairBatch.from_pairs(pairs)
        b = self.batch
        st = C.c_int(0)
        self.handle = self.lib.aln_pairset_create(runtime.context(device), b.seqs.ctypes.data, b.q_off.ctypes.data, b.q_len.ctypes.data,
                                                  b.t_off.ctypes.data, b.t_len.ctypes.data, len(b), C.byref(st))
        if not self.handle:
            runtime.raise_for_status(st.value, "aln_pairset_create")
            raise RuntimeError("aln_pairset_create returned NULL")
        self.shape = None

    @classmethod
    def from_seqset(cls, seqset, block=None, first=0, n=None):
        """Pairs first .. first + n - 1 (default: to the end) of a block of a resident SeqSet as a pair set that reads the set's own
        residues on the device (aln_pairset_create_from_set): nothing is uploaded.  .q / .t are the pairs' sequence numbers."""
        from . import seqset as seqset_module
        self = cls.__new__(cls)
        self.lib = _ffi.load()
        self.handle = None
        self.shape = None
        b = seqset_module._block(block, len(seqset))
        total = int(self.lib.aln_seqset_pairs(seqset.handle, C.byref(b)))
        if n is None:
            n = max(total - int(first), 0)
        st = C.c_int(0)
        self.handle = self.lib.aln_pairset_create_from_set(seqset.handle, C.byref(b), int(first), int(n), C.byref(st))
        if not self.handle:
            runtime.raise_for_status(st.value, "aln_pairset_create_from_set")
            raise RuntimeError("aln_pairset_create_from_set returned NULL")
        self.q, self.t = seqset_module.window(b, first, n)
        self.batch = _Lengths(seqset.len[self.q.astype(np.int64)], seqset.len[self.t.astype(np.int64)])
        return self

    def __len__(self):
        return len(self.batch)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.handle:
            self.lib.aln_pairset_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, semantics, del_, ext, matrices, active, blank=98, force_serial=False, max_passes=0):
        """matrices: (len(active), rows, cols) f64, entry k scores pair active[k].  Returns the summaries (RESULT_DTYPE), entry k
        pair active[k]'s; a failed pair carries its status and leaves the others untouched."""
        m = np.ascontiguousarray(matrices, dtype=np.float64)
        act = np.ascontiguousarray(active, dtype=np.uint32)
        if m.ndim != 3 or m.shape[0] != len(act):
            raise ValueError("matrices: one (rows, cols) matrix per active pair")
        p = _ffi.Params(int(semantics), 0, float(del_), float(ext), None, m.shape[1], m.shape[2], m.shape[2], 0, int(blank), 0,
                        int(bool(force_serial)), 0, int(max_passes))
        res = np.zeros(len(act), dtype=RESULT_DTYPE)
        st = self.lib.aln_pairset_run(self.handle, C.byref(p), m.ctypes.data, act.ctypes.data, len(act), res.ctypes.data)
        runtime.raise_for_status(st, "aln_pairset_run")
        self.shape = (m.shape[1], m.shape[2])
        return res

    def frequencies(self, which):
        """uint32 (len(which), rows, cols): the frequency matrix of every listed pair of the last run."""
        w = np.ascontiguousarray(which, dtype=np.uint32)
        rows, cols = self.shape if self.shape else (0, 0)
        out = np.zeros((len(w), rows, cols), dtype=np.uint32)
        st = self.lib.aln_pairset_frequencies(self.handle, w.ctypes.data, len(w), out.ctypes.data)
        runtime.raise_for_status(st, "aln_pairset_frequencies")
        return out

    def strings(self, which):
        """(summaries, [(aligned query, aligned target)]) of the listed pairs of the last run (empty strings for a failed pair)."""
        w = np.ascontiguousarray(which, dtype=np.uint32)
        b = self.batch
        cap = (b.q_len[w] + b.t_len[w] + np.uint64(2)).astype(np.uint64) if len(w) else np.zeros(0, dtype=np.uint64)
        off = np.zeros(len(w), dtype=np.uint64)
        if len(w) > 1:
            off[1:] = np.cumsum(2 * cap)[:-1]
        tb = np.zeros(int((2 * cap).sum()), dtype=np.uint8)
        res = np.zeros(len(w), dtype=RESULT_DTYPE)
        st = self.lib.aln_pairset_strings(self.handle, w.ctypes.data, len(w), res.ctypes.data, tb.ctypes.data, off.ctypes.data)
        runtime.raise_for_status(st, "aln_pairset_strings")
        out = []
        for k in range(len(w)):
            n = int(res["aln_len"][k]) if res["status"][k] == _ffi.OK else 0
            o, c = int(off[k]), int(cap[k])
            out.append((tb[o:o + n].copy(), tb[o + c:o + c + n].copy()))
        return res, out

    def set_heuristics(self, rows, cols, frequencies, kd, r_squared):
        """Every pair's transform parameters (frequencies (n, rows), kd and r_squared scalars or (n,)), uploaded once; reserves the
        store of one rows x cols matrix per pair and clears it."""
        n = len(self)
        fr = np.ascontiguousarray(frequencies, dtype=np.float64)
        if fr.shape != (n, rows):
            raise ValueError("frequencies: (n_pairs, rows)")
        kd = np.ascontiguousarray(np.broadcast_to(np.asarray(kd, dtype=np.float64), (n,)))
        r2 = np.ascontiguousarray(np.broadcast_to(np.asarray(r_squared, dtype=np.float64), (n,)))
        st = self.lib.aln_pairset_heuristics(self.handle, int(rows), int(cols), fr.ctypes.data, kd.ctypes.data, r2.ctypes.data)
        runtime.raise_for_status(st, "aln_pairset_heuristics")
        self.store_shape = (int(rows), int(cols))

    def reestimate(self, which, matrix=None):
        """store[which[k]] = transform_matrix(source, pair which[k]'s parameters) on the device; the source is `matrix` for every
        listed pair, or (None) the frequency counts of the pair's held strings.  Returns status (len(which),) int32: 0, or
        _ffi.TRANSFORM_NO_ROOT (the store entry is then unchanged)."""
        w = np.ascontiguousarray(which, dtype=np.uint32)
        m = None
        if matrix is not None:
            m = np.ascontiguousarray(matrix, dtype=np.float64)
            if m.shape != getattr(self, "store_shape", None):
                raise ValueError("matrix: the shape given to set_heuristics")
        status = np.zeros(len(w), dtype=np.int32)
        st = self.lib.aln_pairset_reestimate(self.handle, m.ctypes.data if m is not None else None, w.ctypes.data, len(w), status.ctypes.data)
        runtime.raise_for_status(st, "aln_pairset_reestimate")
        return status

    def run_stored(self, semantics, del_, ext, active, blank=98, force_serial=False, max_passes=0):
        """`run` with entry k scored by the store entry of pair active[k]."""
        act = np.ascontiguousarray(active, dtype=np.uint32)
        rows, cols = getattr(self, "store_shape", None) or (0, 0)
        p = _ffi.Params(int(semantics), 0, float(del_), float(ext), None, rows, cols, cols, 0, int(blank), 0, int(bool(force_serial)), 0,
                        int(max_passes))
        res = np.zeros(len(act), dtype=RESULT_DTYPE)
        st = self.lib.aln_pairset_run_stored(self.handle, C.byref(p), act.ctypes.data, len(act), res.ctypes.data)
        runtime.raise_for_status(st, "aln_pairset_run_stored")
        self.shape = (rows, cols)
        return res

    def matrices(self, which):
        """f64 (len(which), rows, cols): the store entries of the listed pairs."""
        w = np.ascontiguousarray(which, dtype=np.uint32)
        rows, cols = getattr(self, "store_shape", None) or (0, 0)
        out = np.zeros((len(w), rows, cols), dtype=np.float64)
        st = self.lib.aln_pairset_matrices(self.handle, w.ctypes.data, len(w), out.ctypes.data)
        runtime.raise_for_status(st, "aln_pairset_matrices")
        return out

    def loop_begin(self, matrix):
        """The loop's start (aln_pairset_loop_begin, after set_heuristics): best f = 0 and store entry i = transform(matrix, pair i's
        parameters) for every pair; the pairs with a root form the going list on the device.  Returns status (n,) int32: 0, or
        _ffi.TRANSFORM_NO_ROOT."""
        m = np.ascontiguousarray(matrix, dtype=np.float64)
        if m.shape != getattr(self, "store_shape", None):
            raise ValueError("matrix: the shape given to set_heuristics")
        status = np.zeros(len(self), dtype=np.int32)
        st = self.lib.aln_pairset_loop_begin(self.handle, m.ctypes.data, status.ctypes.data)
        runtime.raise_for_status(st, "aln_pairset_loop_begin")
        self._going = int((status == 0).sum())
        return status

    def loop_step(self, semantics, del_, ext, blank=98):
        """One iteration for every going pair (aln_pairset_loop_step): the run, the decision, the re-estimation and both lists on the
        device.  Returns (finished pair numbers uint32, causes uint32 -- _ffi.LOOP_CAUSE_*, summaries RESULT_DTYPE, counts (run, done,
        failed, more)); strings / matrices of the finished pairs can be fetched until the next step."""
        rows, cols = getattr(self, "store_shape", None) or (0, 0)
        p = _ffi.Params(int(semantics), 0, float(del_), float(ext), None, rows, cols, cols, 0, int(blank), 0, 0, 0, 0)
        room = max(int(getattr(self, "_going", len(self))), 1)
        fin = np.zeros(room, dtype=np.uint32)
        cause = np.zeros(room, dtype=np.uint32)
        res = np.zeros(room, dtype=RESULT_DTYPE)
        counts = np.zeros(4, dtype=np.uint32)
        st = self.lib.aln_pairset_loop_step(self.handle, C.byref(p), fin.ctypes.data, cause.ctypes.data, res.ctypes.data, counts.ctypes.data)
        runtime.raise_for_status(st, "aln_pairset_loop_step")
        self.shape = (rows, cols)
        self._going = int(counts[3])
        k = int(counts[1]) + int(counts[2])
        return fin[:k], cause[:k], res[:k], tuple(int(c) for c in counts)

    def stats(self):
        ms, by = (C.c_double * 4)(), (C.c_uint64 * 2)()
        runtime.raise_for_status(self.lib.aln_pairset_stats(self.handle, ms, by), "aln_pairset_stats")
        return dict(fill_ms=ms[0], traceback_ms=ms[1], fetch_kernel_ms=ms[2], wall_ms=ms[3], bytes_up=int(by[0]), bytes_down=int(by[1]))


class _Lengths:
    """What PairSet needs of a PairBatch when the residues are a sequence set's: the pairs' lengths."""

    def __init__(self, q_len, t_len):
        self.q_len = np.ascontiguousarray(q_len, dtype=np.uint64)
        self.t_len = np.ascontiguousarray(t_len, dtype=np.uint64)

    def __len__(self):
        return len(self.q_len)


def _transform(context, matrices, frequencies, kd, r_squared):
    lib = _ffi.load()
    m = np.ascontiguousarray(matrices, dtype=np.float64)
    if m.ndim != 3:
        raise ValueError("matrices: (n, rows, cols)")
    n, rows, cols = m.shape
    fr = np.ascontiguousarray(frequencies, dtype=np.float64)
    if fr.shape != (n, rows):
        raise ValueError("frequencies: (n, rows)")
    kd = np.ascontiguousarray(np.broadcast_to(np.asarray(kd, dtype=np.float64), (n,)))
    r2 = np.ascontiguousarray(np.broadcast_to(np.asarray(r_squared, dtype=np.float64), (n,)))
    out = np.zeros_like(m)
    status = np.zeros(n, dtype=np.int32)
    args = (n, rows, cols, m.ctypes.data, fr.ctypes.data, kd.ctypes.data, r2.ctypes.data, out.ctypes.data, status.ctypes.data)
    name = "aln_transform_matrices" if context is None else "aln_transform_matrices_device"
    st = lib.aln_transform_matrices(*args) if context is None else lib.aln_transform_matrices_device(context, *args)
    if st != _ffi.OK:
        raise ValueError("%s: %s" % (name, _ffi.STATUS_NAMES.get(st, st)))
    return out, status


def transform_matrices(matrices, frequencies, kd, r_squared):
    """aln_transform_matrices: transform_matrix (heuristic.py) for n matrices at once, in the library's host code -- the same bits as
    the numpy mirror (aligner_amd/csrc/aln_transform_rules.h).  matrices (n, rows, cols), frequencies (n, rows), kd and r_squared
    scalars or (n,).  Returns (out (n, rows, cols), status (n,) int32: 0, or _ffi.TRANSFORM_NO_ROOT = WrongMatrixSpecified)."""
    return _transform(None, matrices, frequencies, kd, r_squared)


def transform_matrices_device(matrices, frequencies, kd, r_squared, device=None):
    """aln_transform_matrices_device: transform_matrices computed on the GPU by the kernel of PairSet.reestimate (at most 1024 entries
    per matrix): the same arguments, the same results bit for bit."""
    return _transform(runtime.context(device), matrices, frequencies, kd, r_squared)
