"""An oracle-backed stand-in for aligner_amd.pairset.PairSet: the same run / frequencies / strings / close, every alignment by the CPU
oracle (oracle.align), the frequency matrices by oracle.frequency_matrix.  Not a test module: imported by tests/test_pairset_*.py."""
import numpy as np

from aligner_amd.batch import RESULT_DTYPE


class OraclePairSet:
    def __init__(self, pairs, device=None):
        self.pairs = [(np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)) for q, t in pairs]
        self.held = None
        self.runs = []          # the `active` list of every run
        self.closed = False

    def run(self, semantics, del_, ext, matrices, active, blank=98, **_kw):
        import oracle
        m = np.asarray(matrices, dtype=np.float64)
        assert m.ndim == 3 and m.shape[0] == len(active) and len(set(active)) == len(active)
        self.runs.append(list(active))
        self.shape, self.blank = m.shape[1:], blank
        res = np.zeros(len(active), dtype=RESULT_DTYPE)
        self.held = {}
        for k, i in enumerate(active):
            q, t = self.pairs[i]
            r = oracle.align(semantics, q, t, del_, ext, m[k], blank=blank)
            res["status"][k] = r["status"]
            if r["status"] == 0:
                res["f"][k], res["score"][k] = r["f"], r["score"]
                res["end_y"][k], res["end_x"][k] = r["end"]
                res["start_y"][k], res["start_x"][k] = r["start"]
                res["aln_len"][k] = len(r["qa"])
            self.held[i] = (res[k].copy(), r["qa"], r["ta"])
        return res

    def frequencies(self, which):
        import oracle
        assert self.held is not None and self.shape[0] == self.shape[1]
        out = np.zeros((len(which),) + tuple(self.shape), dtype=np.uint32)
        for k, i in enumerate(which):
            r, qa, ta = self.held[i]
            if r["status"] == 0:
                out[k] = oracle.frequency_matrix(qa, ta, self.shape[0], self.blank).astype(np.uint32)
        return out

    def strings(self, which):
        res = np.zeros(len(which), dtype=RESULT_DTYPE)
        strs = []
        for k, i in enumerate(which):
            r, qa, ta = self.held[i]
            res[k] = r
            strs.append((qa.copy(), ta.copy()) if r["status"] == 0 else (np.zeros(0, np.uint8), np.zeros(0, np.uint8)))
        return res, strs

    def close(self):
        self.closed = True
