"""Shared by tests/test_set_heuristic_*.py (not a test module): the loop of HeuristicAligner replayed on the CPU (oracle + numpy
transform) as (cause, finishing step), an oracle-backed stand-in for a pair set derived from a sequence set, and the tiny DNA set
whose pairs' loops are a table lookup (the way of tests/select_cases.py)."""
import numpy as np

import seqset_ref

from aligner_amd.batch import RESULT_DTYPE
from aligner_amd.heuristic import WrongMatrixSpecified, transform_matrix

DONE, FAILED, NO_ROOT = 0, 1, 2


def classify(status, f, best):
    """aln_loop_rules.h restated: a cause, or 3 (improved)."""
    if status != 0:
        return FAILED
    return 3 if f > best else DONE


def replay(orc, q, t, matrix, kd, r2, freq, del_, ext, volume):
    """One pair's loop: dict(begin=bool no root at the start, cause, step (1-based finishing step), status, f, matrix, best)."""
    with np.errstate(all="ignore"):
        try:
            cur = transform_matrix(matrix, kd, r2, freq)
        except WrongMatrixSpecified:
            return dict(begin=True, cause=NO_ROOT, step=0, status=0, f=0.0, matrix=None, ref=None)
        best, step = 0.0, 0
        while True:
            step += 1
            r = orc.align(orc.CORE_LOCAL, q, t, del_, ext, cur)
            c = classify(r["status"], r["f"] if r["status"] == 0 else 0.0, best)
            if c == FAILED:
                return dict(begin=False, cause=FAILED, step=step, status=r["status"], f=0.0, matrix=cur, ref=r)
            if c == DONE:
                return dict(begin=False, cause=DONE, step=step, status=0, f=r["f"], matrix=cur, ref=r)
            best = r["f"]
            try:
                cur = transform_matrix(orc.frequency_matrix(r["qa"], r["ta"], volume), kd, r2, freq)
            except WrongMatrixSpecified:
                return dict(begin=False, cause=NO_ROOT, step=step, status=0, f=r["f"], matrix=cur, ref=r)
            assert step < 64


def block_list(n_seqs, b):
    """[(q, t)] of a block (q_first, q_count, t_first, t_count, upper) by tests/seqset_ref.py."""
    assert seqset_ref.block_pairs(n_seqs, *b) > 0
    return seqset_ref.generate_pairs(b[0], b[1]) if b[4] else seqset_ref.rectangle_pairs(b[0], b[1], b[2], b[3])


class FakeSeqSet:
    """What heuristic.align_set asks of a SeqSet, without a device."""

    def __init__(self, codes, alphabet):
        self.codes = [np.asarray(c, dtype=np.uint8) for c in codes]
        self.alphabet = alphabet
        self.handle = None

    def __len__(self):
        return len(self.codes)

    def pairs(self, b):
        return seqset_ref.block_pairs(len(self), b.q_first, b.q_count, b.t_first, b.t_count, b.upper, b.reserved)


class OracleSetLoop:
    """PairSet.from_seqset + set_heuristics / loop_begin / loop_step / strings / matrices on the CPU oracle.  made: every instance's
    (first, n, steps)."""
    made = []

    def __init__(self, seqset, b, first, n):
        import oracle
        self.orc = oracle
        allp = block_list(len(seqset), (b.q_first, b.q_count, b.t_first, b.t_count, b.upper))
        self.qt = allp[first:first + n]
        assert len(self.qt) == n
        self.q = np.array([p[0] for p in self.qt], dtype=np.uint64)
        self.t = np.array([p[1] for p in self.qt], dtype=np.uint64)
        self.codes = seqset.codes
        self.first, self.n, self.steps, self.closed = first, n, 0, False
        OracleSetLoop.made.append(self)

    def set_heuristics(self, rows, cols, freq, kd, r2):
        assert np.asarray(freq).shape == (self.n, rows) and len(kd) == self.n and len(r2) == self.n
        self.v, self.freq, self.kd, self.r2 = rows, np.array(freq), np.array(kd), np.array(r2)

    def loop_begin(self, m):
        self.store, self.best, status = [None] * self.n, np.zeros(self.n), np.zeros(self.n, dtype=np.int32)
        with np.errstate(all="ignore"):
            for i in range(self.n):
                try:
                    self.store[i] = transform_matrix(m, self.kd[i], self.r2[i], self.freq[i])
                except WrongMatrixSpecified:
                    status[i] = 1
        self.going = [i for i in range(self.n) if status[i] == 0]
        return status

    def loop_step(self, semantics, del_, ext, blank=98):
        orc = self.orc
        self.steps += 1
        self.held, fin, cause, res, more = {}, [], [], [], []
        for i in self.going:
            r = orc.align(semantics, self.codes[self.qt[i][0]], self.codes[self.qt[i][1]], del_, ext, self.store[i], blank=blank)
            s = np.zeros(1, dtype=RESULT_DTYPE)[0]
            s["status"] = r["status"]
            if r["status"] == 0:
                s["f"], s["score"] = r["f"], r["score"]
                s["end_y"], s["end_x"] = r["end"]
                s["start_y"], s["start_x"] = r["start"]
                s["aln_len"] = len(r["qa"])
            self.held[i] = (s, r.get("qa"), r.get("ta"))
            c = classify(r["status"], s["f"], self.best[i])
            if c == 3:
                self.best[i] = s["f"]
                try:
                    with np.errstate(all="ignore"):
                        self.store[i] = transform_matrix(orc.frequency_matrix(r["qa"], r["ta"], self.v, blank), self.kd[i], self.r2[i], self.freq[i])
                    more.append(i)
                    continue
                except WrongMatrixSpecified:
                    c = NO_ROOT
            fin.append(i); cause.append(c); res.append(s)
        counts = (len(self.going), cause.count(DONE), len(fin) - cause.count(DONE), len(more))
        self.going = more
        return (np.array(fin, dtype=np.uint32), np.array(cause, dtype=np.uint32),
                np.array(res, dtype=RESULT_DTYPE) if res else np.zeros(0, dtype=RESULT_DTYPE), counts)

    def strings(self, which):
        res = np.zeros(len(which), dtype=RESULT_DTYPE)
        strs = []
        for k, i in enumerate(which):
            s, qa, ta = self.held[int(i)]
            res[k] = s
            strs.append((qa.copy(), ta.copy()) if s["status"] == 0 else (np.zeros(0, np.uint8), np.zeros(0, np.uint8)))
        return res, strs

    def matrices(self, which):
        return np.array([self.store[int(i)] for i in which])

    def close(self):
        self.closed = True


# ---------------------------------------------------------------- the tiny DNA set of the compaction test
DNA_MATRIX = np.where(np.eye(4) > 0, 5.0, -4.0) + 0.125
DNA_DEL, DNA_EXT = 6.0, 1.0
# contents 0 .. 11: 1 - 4 residues; 12: empty (the reference panics: cause 1, ALN_ERR_EMPTY_SEQUENCE); 13: a code outside the matrix
DNA_CONTENTS = [[0], [1], [0, 1], [0, 0], [0, 1, 2], [2, 2, 2], [0, 1, 2, 3], [3, 2, 1, 0], [1, 1, 0, 0], [2], [3, 3], [0, 2, 0, 2], [], [9]]
# (kd, r_squared, frequencies); entry 3 has no root under any matrix (r_squared below kd^2 / sum p^2)
DNA_PARAMS = [(-0.5, 16.0, [.25] * 4), (-1.0, 16.0, [.4, .3, .2, .1]), (-0.2, 4.0, [.1, .2, .3, .4]), (-0.5, 1e-9, [.25] * 4),
              (0.5, 16.0, [.25] * 4), (-2.0, 100.0, [.7, .1, .1, .1])]


def dna_content_of(seq):
    return seq % len(DNA_CONTENTS)


def dna_param_of(q, t):
    return (q * 5 + t * 3) % len(DNA_PARAMS)


def dna_table(orc):
    """table[cq][ct][par] = replay(...) for every content pair and parameter entry."""
    out = {}
    for a, qa in enumerate(DNA_CONTENTS):
        for b, tb in enumerate(DNA_CONTENTS):
            for p, (kd, r2, fr) in enumerate(DNA_PARAMS):
                out[a, b, p] = replay(orc, np.array(qa, np.uint8), np.array(tb, np.uint8), DNA_MATRIX, kd, r2, np.array(fr), DNA_DEL, DNA_EXT, 4)
    return out
