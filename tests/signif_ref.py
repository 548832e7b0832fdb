"""numpy restatement of the per-hit reduction of aln_seqset_held_significance (aligner_amd/csrc/aln_signif_rules.h), written from the
specification, not from the header: the copies are padded to rows of 64, the 64 column accumulators take row after row (copy
l + 64 r is column l of row r), then the halves are folded onto each other at widths 32, 16, 8, 4, 2, 1.  Every numpy operation
below is one IEEE operation per element, rounded on its own (f * f is formed before it is added)."""
import numpy as np

RECORD = np.dtype([("sum", "<f8"), ("sum_sq", "<f8"), ("f_max", "<f8"), ("n_ok", "<u4"), ("n_ge", "<u4"), ("status", "<i4"),
                   ("first_bad", "<u4"), ("reserved", "<u8")])
LANES = 64
NONE = 0xFFFFFFFF


def reduce_one(f, status, f_hit):
    """The record (a RECORD scalar) of one hit: f float64[per_pair], status int32[per_pair] of its copies, f_hit its held score."""
    f = np.asarray(f, dtype=np.float64)
    status = np.asarray(status, dtype=np.int32)
    n = len(f)
    rows = (n + LANES - 1) // LANES
    v = np.zeros(rows * LANES)
    ok = np.zeros(rows * LANES, dtype=bool)
    v[:n] = f
    ok[:n] = status == 0
    v, ok = v.reshape(rows, LANES), ok.reshape(rows, LANES)
    s = np.zeros(LANES)
    s2 = np.zeros(LANES)
    mx = np.full(LANES, -np.inf)
    n_ok = np.zeros(LANES, dtype=np.uint32)
    n_ge = np.zeros(LANES, dtype=np.uint32)
    with np.errstate(all="ignore"):
        for r in range(rows):
            x, t = v[r], ok[r]
            sq = x * x
            s = np.where(t, s + x, s)
            s2 = np.where(t, s2 + sq, s2)
            mx = np.where(t & (x > mx), x, mx)
            n_ok = n_ok + t.astype(np.uint32)
            n_ge = n_ge + (t & (x >= f_hit)).astype(np.uint32)
        w = LANES // 2
        while w >= 1:
            s = s[:w] + s[w:2 * w]
            s2 = s2[:w] + s2[w:2 * w]
            mx = np.where(mx[w:2 * w] > mx[:w], mx[w:2 * w], mx[:w])
            n_ok = n_ok[:w] + n_ok[w:2 * w]
            n_ge = n_ge[:w] + n_ge[w:2 * w]
            w //= 2
    out = np.zeros((), dtype=RECORD)
    out["sum"], out["sum_sq"], out["f_max"], out["n_ok"], out["n_ge"] = s[0], s2[0], mx[0], n_ok[0], n_ge[0]
    bad = np.flatnonzero(status != 0)
    out["first_bad"] = bad[0] if len(bad) else NONE
    out["status"] = status[bad[0]] if len(bad) else 0
    return out


def reduce_many(f, status, f_hit):
    """Records of hits: f [n, per_pair], status [n, per_pair], f_hit [n]."""
    out = np.zeros(len(f), dtype=RECORD)
    for i in range(len(f)):
        out[i] = reduce_one(f[i], status[i], f_hit[i])
    return out


def sequential(f, status):
    """(sum, sum_sq) of the taken copies as one ascending left-to-right sum: what the rule is NOT (for tests that the order matters)."""
    s = s2 = 0.0
    for x, st in zip(np.asarray(f, dtype=np.float64).tolist(), np.asarray(status).tolist()):
        if st == 0:
            s = s + x
            s2 = s2 + x * x
    return s, s2
