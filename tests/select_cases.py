"""Inputs for the selection tests (test_select_tiles_cpu.py, test_select_tiles_gpu.py) whose kept set is known by construction.

The scan (aln_scan_*) and the sequence set (aln_seqset_*) both end a pass in a count / offsets / compact selection over tiles of
256 threads x 8 items = 2048 items; the offsets kernel takes 256 tiles per trip.  The cases here put hits on thread, tile and
256-tile edges, leave tiles empty, and make the per-tile counts differ.  Nothing in this file needs a GPU.

Scan: a DNA sequence of code 0, a PWM of 8 columns whose row 1 scores +1 everywhere and whose other rows score -1, del 4, ext 1,
windows first = 0, step = width = 8 (no overlap).  A run of L ones at the start of window k gives that window f = L (F_OF_RUN; the
CPU test asks the oracle) and changes no other window.

Set: S = 726 protein sequences.  Background sequences are 'A' repeated 1 + (i mod 3) times, marked sequences are 'WWWW', one
sequence is empty.  Under BLOSUM62, core local, 11 / 2: background x background scores 4 min(a, b), marked x marked 44, marked x
background has no positive cell and the empty sequence fails its pairs (PAIR_F / PAIR_STATUS; the CPU test asks the oracle)."""
import hashlib

import numpy as np

TILE = 2048                   # 256 threads x 8 items
TRIP = 256                    # tiles per trip of the offsets kernel
PER_THREAD = 8

# ---------------------------------------------------------------- scan
W = 8
DEL, EXT = 4.0, 1.0
F_OF_RUN = {L: float(L) for L in range(W + 1)}        # run length at the window's start -> f (0: an unplanted window)


def scan_pwm():
    m = -np.ones((4, W), dtype=np.float64)
    m[1] = 1.0
    return m


def window_content(L):
    w = np.zeros(W, dtype=np.uint8)
    w[:L] = 1
    return w


def scan_sequence(n, planted):
    """The strand whose window k (8 residues) starts with planted[k] ones."""
    runs = np.zeros(n, dtype=np.int64)
    if planted:
        k = np.fromiter(planted.keys(), dtype=np.int64, count=len(planted))
        runs[k] = np.fromiter(planted.values(), dtype=np.int64, count=len(planted))
    return (np.arange(W)[None, :] < runs[:, None]).astype(np.uint8).ravel()


def runs_of(strand):
    """Run length per window, read back from the residues: a window's content must be one of the nine patterns."""
    w = np.asarray(strand, dtype=np.uint8).reshape(-1, W)
    runs = w.sum(axis=1).astype(np.int64)
    assert np.array_equal(w, (np.arange(W)[None, :] < runs[:, None]).astype(np.uint8))
    return runs


class ScanCase:
    def __init__(self, name, n, planted):
        self.name, self.n, self.planted = name, int(n), dict(planted)
        assert all(0 <= k < n and 1 <= L <= W for k, L in self.planted.items())
        self.strand = scan_sequence(self.n, self.planted)
        self.runs = runs_of(self.strand)
        self.first, self.step, self.width = 0, W, W
        self.tiles = (self.n + TILE - 1) // TILE

    def f(self):
        """f of every window, by table lookup."""
        table = np.array([F_OF_RUN[L] for L in range(W + 1)], dtype=np.float64)
        return table[self.runs]

    def kept(self, min_run):
        """The windows whose run is at least min_run, ascending."""
        return np.flatnonzero(self.runs >= min_run)

    def tile_counts(self, min_run):
        return np.bincount(self.kept(min_run) // TILE, minlength=self.tiles)

    def starts(self, idx):
        idx = np.asarray(idx, dtype=np.uint64)
        return idx * np.uint64(W), np.full(len(idx), W, dtype=np.uint64)


# thresholds (mean, sd, z_min) -> the smallest run that passes; None: nothing passes.  One holds exactly:
# (4 - 1) / 2 == 1.5 and (7 - 0.5) / 0.25 == 26 in binary floating point (every operand is dyadic).
SCAN_THRESHOLDS = [
    ((0.0, 1.0, 1.0), 1),                 # every planted window; (1 - 0) / 1 == 1 exactly
    ((1.0, 2.0, 1.5), 4),                 # exact at L = 4
    ((0.5, 0.25, 26.0), 7),               # exact at L = 7
    ((3.0, 0.0, 2.0), 4),                 # sd = 0: +inf passes (f > mean), 0 / 0 at L = 3 does not, -inf does not
    ((0.0, 1.0, float("nan")), None),     # z_min = NaN
    ((float("nan"), 1.0, 1.0), None),     # mean = NaN
]


def numpy_kept(f, mean, sd, z_min):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.flatnonzero((np.asarray(f, dtype=np.float64) - np.float64(mean)) / np.float64(sd) >= np.float64(z_min))


def case_edges():
    """(a) 3 tiles and a ragged tail of 5: hits on thread edges (7, 8), on both sides of every tile edge, on the last window, and a
    sparse 1 %; run lengths 1 .. 8."""
    n = 3 * TILE + 5
    rng = np.random.default_rng(20261)
    named = [0, 7, 8, 2047, 2048, 2049, 4095, 4096, 6143, 6144, n - 1]
    planted = {k: 1 + i % W for i, k in enumerate(named)}
    for k in rng.choice(n, size=n // 100, replace=False):
        planted.setdefault(int(k), int(rng.integers(1, W + 1)))
    planted[2047], planted[2048] = 8, 8          # the tile 0 | tile 1 edge passes every threshold
    return ScanCase("edges", n, planted), named


def case_empty_tiles():
    """(b) hits in tile 2 of 4 only (tiles 0, 1 and the partial tile 3 are empty: the tile offsets repeat a value)."""
    n = 3 * TILE + 17
    rng = np.random.default_rng(20262)
    planted = {2 * TILE: 5, 3 * TILE - 1: 6}
    for k in rng.choice(TILE, size=23, replace=False):
        planted.setdefault(2 * TILE + int(k), int(rng.integers(1, W + 1)))
    return ScanCase("empty_tiles", n, planted)


def case_exact_multiple():
    """(b) n an exact multiple of the tile, a hit on the last window, an empty first tile."""
    n = 2 * TILE
    return ScanCase("exact_multiple", n, {TILE + 3: 2, TILE + 8: 3, n - 9: 1, n - 1: 4})


_big = {}


def case_many_tiles():
    """(c), (e) 257 full tiles and a tail of 5: the offsets kernel's second trip takes tiles 256 and 257.  About 3000 windows with a
    run of 2 .. 8, spread so that a tile holds between none and a few dozen of them, and a run of 1 on every 26th window that has no
    other (about 20 000 more, for the frequency sums).  Built once."""
    if "case" in _big:
        return _big["case"], _big["named"]
    n = (TRIP + 1) * TILE + 5
    rng = np.random.default_rng(20263)
    named = [0, TRIP * TILE - 1, TRIP * TILE, TRIP * TILE + 1, n - 1]
    planted = {k: 2 + i % 7 for i, k in enumerate(named)}
    tiles = (n + TILE - 1) // TILE
    per_tile = rng.choice([0, 0, 2, 5, 12, 24, 40], size=tiles)
    per_tile[3] = 0
    for t in range(tiles):
        size = min(TILE, n - t * TILE)
        c = min(int(per_tile[t]), size)
        for k in rng.choice(size, size=c, replace=False):
            planted.setdefault(t * TILE + int(k), int(rng.integers(2, W + 1)))
    for k in range(0, n, 26):
        planted.setdefault(k, 1)
    _big["case"], _big["named"] = ScanCase("many_tiles", n, planted), named
    return _big["case"], _big["named"]


MANY_TILES_LEN = ((TRIP + 1) * TILE + 5) * W          # 4 210 728 residues


def capacity_cuts(case, min_run=1):
    """(d) capacities around the tile 0 | tile 1 edge and around the total."""
    counts = case.tile_counts(min_run)
    c0, total = int(counts[0]), int(counts.sum())
    return [c0, c0 + 1, c0 - 1, total - 1, total]


def keep_lists(n):
    """(e) every position; reversed; every third position twice."""
    every = np.arange(n, dtype=np.int64)
    doubled = np.sort(np.concatenate([every, every[::3]]), kind="stable")
    return {"every": every, "reversed": every[::-1].copy(), "doubled": doubled}


# ---------------------------------------------------------------- set
S = 726
SET_DEL, SET_EXT = 11.0, 2.0
MARKED = (2, 115, 116, 595, 596, 722, 725)
EMPTY = 723                                    # its row is pairs 524 898 .. 525 623 (tile 256), its column crosses tiles 256 and 257
CONTENTS = ["A", "AA", "AAA", "WWWW", ""]      # content ids 0 .. 4
OK, ERR_EMPTY, ERR_NO_POSITIVE = 0, 2, 4
# f and status per (query content, target content), as assumed; the CPU test asks the oracle
PAIR_F = np.array([[4, 4, 4, 0, 0], [4, 8, 8, 0, 0], [4, 8, 12, 0, 0], [0, 0, 0, 44, 0], [0, 0, 0, 0, 0]], dtype=np.float64)
PAIR_STATUS = np.array([[0, 0, 0, 4, 2], [0, 0, 0, 4, 2], [0, 0, 0, 4, 2], [4, 4, 4, 0, 2], [2, 2, 2, 2, 2]], dtype=np.int32)
F_MARKED = 44.0          # the marked-only threshold
F_BACKGROUND = 12.0      # equals the score of 'AAA' x 'AAA' exactly: >= keeps those pairs
RECT_TAIL = (718, 8, 0, 726)       # rows 718 .. 725 of the grid: 5808 pairs, 2.8 tiles, with the empty sequence's row
RECT_INNER = (590, 136, 110, 490)  # queries 590 .. 725 x targets 110 .. 599: neither range starts at 0; 66 640 pairs, 32.5 tiles


def set_content_ids():
    ids = np.arange(S) % 3
    ids[list(MARKED)] = 3
    ids[EMPTY] = 4
    return ids


def set_strings():
    return [CONTENTS[c] for c in set_content_ids()]


def set_lengths():
    return np.array([len(s) for s in set_strings()], dtype=np.int64)


def block_pairs_qt(block):
    """(q, t) arrays of a block in its pair order, from tests/seqset_ref.py.  block: ("full",), ("upper", first, n) or
    ("rect", q_first, q_count, t_first, t_count)."""
    import seqset_ref
    if block[0] == "full":
        pairs = seqset_ref.rectangle_pairs(0, S, 0, S)
    elif block[0] == "upper":
        pairs = seqset_ref.generate_pairs(block[1], block[2])
    else:
        pairs = seqset_ref.rectangle_pairs(*block[1:])
    a = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    return a[:, 0], a[:, 1]


_blocks = {}


def block_expect(block):
    """-> (q, t, f, status) of every pair of the block, by table lookup over the contents.  Computed once per block."""
    if block not in _blocks:
        ids = set_content_ids()
        q, t = block_pairs_qt(block)
        _blocks[block] = (q, t, PAIR_F[ids[q], ids[t]], PAIR_STATUS[ids[q], ids[t]])
    return _blocks[block]


def expect_hits(f, status, f_min):
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((status == OK) & (f >= f_min))


def chunk_counts(lengths, q, t, target, cap=None):
    """Restatement of the set's chunking with ALN_CHUNK_CELLS = target: consecutive pairs until their cells reach the target, a tail
    of less than a quarter of the target joins the chunk before it.  cap: no chunk holds more pairs than this (None: no limit).
    (All cell sums here are small integers: exact in doubles.)"""
    cells = (lengths[q] * lengths[t]).astype(np.float64)
    total = float(cells.sum())
    pairs = len(cells)
    if total <= 1.5 * target and (cap is None or pairs <= cap):
        return [pairs]
    cum = np.cumsum(cells)
    counts, start, done = [], 0, 0.0
    while start < pairs:
        k = int(np.searchsorted(cum, done + target, side="left"))       # the first pair at which the chunk's cells reach the target
        while k < pairs and not (total - cum[k] >= 0.25 * target or k + 1 == pairs):
            k += 1
        if cap is not None:
            k = min(k, start + cap - 1)                                  # ... or the pair that fills the chunk
        if k >= pairs:
            counts.append(pairs - start)
            break
        counts.append(k + 1 - start)
        start, done = k + 1, float(cum[k])
    return counts


def chunk_cells():
    """ALN_CHUNK_CELLS for the chunked run: a bit more than a fifth of the full block's cells, so that the full block and the upper
    triangle are cut into at least 3 chunks of several tiles each."""
    L = set_lengths()
    return int(L.sum()) ** 2 // 5 + 977


# ---------------------------------------------------------------- set: what a run of the held passes leaves, hashed
FIELDS = ["f", "score", "end_y", "end_x", "start_y", "start_x", "aln_len", "status"]
DIGEST_PASSES = [(("full",), F_MARKED), (("full",), F_BACKGROUND), (("upper", 0, S), F_MARKED), (("rect",) + RECT_INNER, F_MARKED),
                 (("rect",) + RECT_TAIL, float("-inf"))]


def to_block(block):
    from aligner_amd.seqset import rectangle, upper
    if block[0] == "full":
        return rectangle(0, S, 0, S)
    if block[0] == "upper":
        return upper(block[1], block[2])
    return rectangle(*block[1:])


def sample_positions(n, edges=(), count=50, seed=7):
    """Positions of a held list to fetch strings for: the named ones, the first, the last and `count` random ones."""
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    pos = set(int(e) for e in edges) | {0, n - 1} | set(int(v) for v in rng.integers(0, n, size=min(count, n)))
    return np.array(sorted(pos), dtype=np.uint32)


def set_digest(sset, matrix):
    """SHA-256 over the hit lists (pair numbers, q, t, f: whole) and the summaries and strings of sampled hits of DIGEST_PASSES."""
    h = hashlib.sha256()
    for block, f_min in DIGEST_PASSES:
        held = sset.hits(matrix, SET_DEL, SET_EXT, f_min, to_block(block))
        for a in (held.index, held.q, held.t, held.f):
            h.update(np.ascontiguousarray(a).tobytes())
        res, strs = held.strings(sample_positions(len(held)))
        for name in FIELDS:
            h.update(np.ascontiguousarray(res[name]).tobytes())
        for qa, ta in strs:
            h.update(qa.tobytes()); h.update(b"|"); h.update(ta.tobytes()); h.update(b"/")
    return h.hexdigest()
