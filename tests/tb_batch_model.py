"""The batch traceback (tb_walk_pair, tb_walk_pair_wave, aln_traceback_expand_kernel: aln_traceback.hip) and the direction store
they read (aln_device.h), restated on the CPU.  Not a test module.

`pack` turns the ORACLE's direction matrix into the words of a strip region; `lane_walk` and `wave_walk` then take the steps the
two kernels take over those words and `expand` turns the tag string into the two aligned strings in rounds of 128 positions.
tests/test_tb_batch_model_cpu.py holds the three to the oracle's own answer on every constructed pair of tests/tb_batch_cases.py, so
the step records they return -- strip, lane, row within the lane, step k, quad row, word of the quad, m, "the lane's last block",
and for the wave walk the window register and the reason of every fetch round -- say where on the oracle's path an edge of the
kernels' geometry lies.  A GPU test never takes its expectation from here.

`variant=` breaks one rule at a time (VARIANTS); the CPU test shows that every broken rule gives a wrong answer on at least one
case that is aimed at it.

Restated from aln_device.h: aln_spb, aln_pick_r, aln_strip_blocks, aln_dir_word_index, aln_dir_bitpos, aln_strip_bytes,
aln_uniform_strip_bytes, the row-major fallback (row stride (N + 4) / 4 bytes, four cells a byte, Direction discriminants).
Tags: 0 Diagonal, 1 Left, 2 Top, 3 Beginning; the oracle's D holds Direction discriminants (Top 0, Left 1, Diagonal 2, Beginning 3).
"""
import numpy as np

from tb_single_model import path_from_alignment  # noqa: F401  (the path helper fits unchanged)

SKEW, ROWMAJOR, UNIFORM, UBATCH = 0, 1, 2, 3
FULL_R = 8
STRIP_ROWS = 64 * FULL_R
LOCAL, GLOBAL = "local", "global"
TAG = {"D": 0, "L": 1, "T": 2}
UNWRITTEN = 7                           # a tag byte no lane wrote

VARIANTS = ("window2", "no_wrap_recentre", "flush63", "no_lend", "stale_strip", "last_r8", "no_carry", "tag3_moves")
WALK_VARIANTS = ("window2", "no_wrap_recentre", "flush63", "no_lend", "stale_strip", "last_r8")
WAVE_ONLY = ("window2", "no_wrap_recentre", "flush63")
EXPAND_VARIANTS = ("no_carry", "tag3_moves")


def spb(R):
    return 2 if R >= 5 else 4 if R >= 3 else 16 // R


def pick_r(rem):
    return min(max((rem + 63) // 64, 1), FULL_R)


def strip_blocks(nsteps, s):
    return ((nsteps + s - 1) // s + 3) & ~3


def word_index(k, lane, s):
    kb = k // s
    return ((kb >> 2) * 64 + lane) * 4 + (kb & 3)


def bitpos(k, r, lane, N, R):
    s = spb(R)
    bend, lend = (k // s) * s + s - 1, lane + N - 1
    e = np.minimum(bend, lend)
    return 30 - 2 * ((e - k) * R + (R - 1 - r))


def strip_bytes(N):
    return strip_blocks(N + 63, spb(FULL_R)) * 256


def uniform_strip_bytes(N, R):
    return strip_blocks(N + 63, spb(R)) * 256


def num_strips(M):
    return (M + STRIP_ROWS - 1) // STRIP_ROWS


class Store:
    """words: the strip regions (u32), or the row-major bytes.  R: rows per lane of the uniform layouts (0: skewed)."""

    def __init__(self, M, N, layout, R, words):
        self.M, self.N, self.layout, self.R, self.words = M, N, layout, R, words

    def view(self, y, variant=None):
        """strip_view: (strip, y0, R, first word of the strip's region) for row y >= 1."""
        if self.layout in (UNIFORM, UBATCH):
            strip = (y - 1) // (64 * self.R)
            return strip, strip * 64 * self.R, self.R, strip * uniform_strip_bytes(self.N, self.R) // 4
        strip = (y - 1) // STRIP_ROWS
        R = pick_r(self.M - strip * STRIP_ROWS) if strip + 1 == num_strips(self.M) else FULL_R
        if variant == "last_r8":
            R = FULL_R
        return strip, strip * STRIP_ROWS, R, strip * strip_bytes(self.N) // 4

    def dir_at(self, y, x, global_):
        """dir_at: the plain cell-by-cell reader (a Direction discriminant)."""
        if y == 0 or x == 0:
            if not global_ or (y == 0 and x == 0):
                return 3
            return 1 if y == 0 else 0
        if self.layout == ROWMAJOR:
            return (int(self.words[y * ((self.N + 4) // 4) + (x >> 2)]) >> (2 * (x & 3))) & 3
        _, y0, R, base = self.view(y)
        i = y - 1 - y0
        lane, r = i // R, i % R
        k = x - 1 + lane
        tag = (int(self.words[base + word_index(k, lane, spb(R))]) >> int(bitpos(k, r, lane, self.N, R))) & 3
        return 3 if tag == 3 else 2 - tag


def pack(D, M, N, layout=SKEW, R=0):
    """The oracle's (M + 1) x (N + 1) direction matrix as the fill kernels store it.  Skewed layout: 512-row strips with R = 8, the
    last strip with aln_pick_r of what remains; uniform layouts: 64 R rows a strip.  Bits of cells no lane is active for stay 0."""
    D = np.asarray(D)
    assert D.shape == (M + 1, N + 1)
    if layout == ROWMAJOR:
        rb = (N + 4) // 4
        out = np.zeros((M + 1) * rb, dtype=np.uint8)
        ys, xs = np.meshgrid(np.arange(1, M + 1), np.arange(1, N + 1), indexing="ij")
        np.bitwise_or.at(out, (ys * rb + (xs >> 2)).ravel(), (D[1:, 1:].astype(np.uint8) << (2 * (xs & 3)).astype(np.uint8)).ravel())
        return Store(M, N, layout, 0, out)
    uniform = layout in (UNIFORM, UBATCH)
    assert (R >= 1) == uniform
    rows_per = 64 * R if uniform else STRIP_ROWS
    ns = (M + rows_per - 1) // rows_per
    sbytes = uniform_strip_bytes(N, R) if uniform else strip_bytes(N)
    words = np.zeros(ns * sbytes // 4, dtype=np.uint32)
    for s in range(ns):
        y0 = s * rows_per
        rows = min(M - y0, rows_per)
        Rs = R if uniform else (pick_r(M - y0) if s + 1 == ns else FULL_R)
        i, xs = np.meshgrid(np.arange(rows), np.arange(1, N + 1), indexing="ij")
        lane, r = i // Rs, i % Rs
        k = xs - 1 + lane
        d = D[y0 + 1:y0 + rows + 1, 1:].astype(np.int64)
        tag = np.where(d == 3, 3, 2 - d).astype(np.uint32)
        kb = k // spb(Rs)
        idx = s * sbytes // 4 + ((kb >> 2) * 64 + lane) * 4 + (kb & 3)
        np.bitwise_or.at(words, idx.ravel(), (tag << bitpos(k, r, lane, N, Rs).astype(np.uint32)).ravel())
    return Store(M, N, layout, R if uniform else 0, words)


def _consts(R):
    s = spb(R)
    lgS = s.bit_length() - 1
    return (65535 + R) // R, lgS, lgS + 2, s - 1


def _tag(quad, k, r, lane, N, R, lgS, bmask, variant):
    lend = lane + N - 1
    kb = k | bmask
    m = (kb if variant == "no_lend" else min(kb, lend)) - k
    j = (k >> lgS) & 3
    half = (int(quad[3]) << 32 | int(quad[2])) if j & 2 else (int(quad[1]) << 32 | int(quad[0]))
    return (half >> (32 * (j & 1) + 32 - 2 * R * (m + 1) + 2 * r)) & 3, m, j, kb > lend


def _borders(tags, cy, cx, global_):
    if global_:
        if cy == 0 and cx != 0:
            tags += [1] * cx
            cx = 0
        elif cx == 0 and cy != 0:
            tags += [2] * cy
            cy = 0
    return cy, cx


def lane_walk(store, end, mode, legacy=False, variant=None):
    """tb_walk_pair.  Returns (tags in walk order, start cell, steps, records of the interior steps)."""
    global_ = mode == GLOBAL
    cy, cx = end
    if legacy:
        cy, cx = cy - 1, cx - 1
    tags, recs = [], []
    if store.layout == ROWMAJOR:
        while True:
            d = store.dir_at(cy, cx, global_)
            if d == 3:
                break
            tags.append(2 - d)
            cy -= d != 1
            cx -= d != 0
        return tags, (cy, cx), len(tags), recs
    N, W = store.N, store.words
    if cy != 0 and cx != 0:
        strip, y0, R, base = store.view(cy, variant)
        iy, cxm = cy - 1 - y0, cx - 1
        rinv, lgS, qsh, bmask = _consts(R)
        qcur, quad = None, None
        while True:
            if iy < 0 or cxm < 0:
                cy, cx = iy + 1 + y0, cxm + 1
                if cy == 0 or cx == 0:
                    break
                strip, y0, R2, base = store.view(cy, variant)
                iy = cy - 1 - y0
                if variant != "stale_strip":
                    R = R2
                    rinv, lgS, qsh, bmask = _consts(R)
                qcur = None
            lane = (iy * rinv) >> 16
            r = iy - lane * R
            k = cxm + lane
            qi = ((k >> qsh) << 6) + lane
            if qi != qcur:
                quad, qcur = W[base + 4 * qi:base + 4 * qi + 4], qi
            tag, m, j, last = _tag(quad, k, r, lane, N, R, lgS, bmask, variant)
            recs.append(dict(strip=strip, lane=lane, r=r, k=k, qrow=k >> qsh, word=j, m=m, last_block=last, y=iy + 1 + y0, x=cxm + 1,
                             R=R, tag=tag))
            if tag == 3:
                cy, cx = iy + 1 + y0, cxm + 1
                break
            tags.append(tag)
            iy -= tag != 1
            cxm -= tag != 2
            if len(tags) > store.M + N + 2:
                break                                    # a broken variant that no longer ends
    cy, cx = _borders(tags, cy, cx, global_)
    return tags, (cy, cx), len(tags), recs


def wave_walk(store, end, mode, legacy=False, variant=None):
    """tb_walk_pair_wave.  Returns (tags as the 64 lanes wrote them, start cell, steps, records, fetch rounds).  A record carries
    reg: the window register that served the step; a round: strip, step number, lane, reason ("first": first step of a strip,
    "dq": the path left the three quads downwards, dq = 3 and up, "wrap": it is to the right of the prediction and dq wrapped),
    clamp: kj <= 0 on some fetching lane."""
    global_ = mode == GLOBAL
    if store.layout == ROWMAJOR:
        return lane_walk(store, end, mode, legacy, variant) + ([],)
    cy, cx = end
    if legacy:
        cy, cx = cy - 1, cx - 1
    N, W = store.N, store.words
    ops = [UNWRITTEN] * (store.M + N + 2 + 64)
    tagv = [0] * 64
    length, recs, rounds = 0, [], []
    if cy != 0 and cx != 0:
        strip, y0, R, base = store.view(cy, variant)
        iy, cxm = cy - 1 - y0, cx - 1
        rinv, lgS, qsh, bmask = _consts(R)
        nq = ((N + 62) >> qsh) + 1
        zero = (0, 0, 0, 0)
        wa, wb, wc = [zero] * 64, [zero] * 64, [zero] * 64
        qrow = [0] * 64
        have, cur_lane, cur_q, q, reg = False, None, None, zero, None
        while True:
            if iy < 0 or cxm < 0:
                cy, cx = iy + 1 + y0, cxm + 1
                if cy == 0 or cx == 0:
                    break
                strip, y0, R2, base = store.view(cy, variant)
                iy = cy - 1 - y0
                if variant != "stale_strip":
                    R = R2
                    rinv, lgS, qsh, bmask = _consts(R)
                    nq = ((N + 62) >> qsh) + 1
                have, cur_lane = False, None
            lane = (iy * rinv) >> 16
            r = iy - lane * R
            k = cxm + lane
            qr = k >> qsh
            if lane != cur_lane or qr != cur_q:
                dq = (qrow[lane] + 1 - qr) & 0xffffffff
                wrapped = dq >= 1 << 31
                if not have or (dq > 2 and not (wrapped and variant == "no_wrap_recentre")):
                    clamp = False
                    wa, wb, wc = [zero] * 64, [zero] * 64, [zero] * 64
                    for j in range(64):
                        t = iy - (j * R + R - 1)
                        kj = (cxm - max(t, 0)) + j - (R >> 1)
                        qrow[j] = max(kj, 0) >> qsh
                        if j == lane:
                            qrow[j] = qr
                        if j > lane:
                            continue
                        clamp |= kj <= 0
                        g = lambda row: tuple(int(v) for v in W[base + 4 * ((row << 6) + j):base + 4 * ((row << 6) + j) + 4])  # noqa: E731
                        if qrow[j] + 1 < nq:
                            wa[j] = g(qrow[j] + 1)
                        if qrow[j] < nq:
                            wb[j] = g(qrow[j])
                        if qrow[j] >= 1 and variant != "window2":
                            wc[j] = g(qrow[j] - 1)
                    rounds.append(dict(strip=strip, step=length, lane=lane, reason="first" if not have else "wrap" if wrapped else "dq", clamp=clamp))
                    have, dq = True, 1
                reg = "wa" if dq == 0 else "wb" if dq == 1 else "wc"
                q = (wa if dq == 0 else wb if dq == 1 else wc)[lane]
                cur_lane, cur_q = lane, qr
            tag, m, j, last = _tag(q, k, r, lane, N, R, lgS, bmask, variant)
            recs.append(dict(strip=strip, lane=lane, r=r, k=k, qrow=qr, word=j, m=m, last_block=last, y=iy + 1 + y0, x=cxm + 1, R=R,
                             tag=tag, reg=reg))
            if tag == 3:
                cy, cx = iy + 1 + y0, cxm + 1
                break
            tagv = [tag] + tagv[:63]                     # the lane shift register: the new tag enters at lane 0
            length += 1
            if (length & 63) == (63 if variant == "flush63" else 0):
                for lane_id in range(64):
                    if length - 1 - lane_id >= 0:
                        ops[length - 1 - lane_id] = tagv[lane_id]
            iy -= tag != 1
            cxm -= tag != 2
            if length > store.M + N + 2:
                break
    for lane_id in range(length & 63):
        ops[length - 1 - lane_id] = tagv[lane_id]
    tags = ops[:length]
    cy, cx = _borders(tags, cy, cx, global_)
    return tags, (cy, cx), len(tags), recs, rounds


def expand(tags, start, q, t, pwm=False, blank=98, variant=None):
    """aln_traceback_expand_kernel: rounds of 64 G positions (G = 2), the counts of x and y moves carried from group to group in
    base_x / base_y, tag 3 padding the last round.  Returns (query string or column numbers, target string, reads outside a
    sequence): the strings without the duplicated seed pair.  A padding lane never loads a residue in the kernel; with
    variant "tag3_moves" it does, and the only thing that shows is the index of that load."""
    n = len(tags)
    qa, ta = [None] * n, [None] * n
    base_y, base_x = start
    outside = 0
    for j0 in range(0, n, 128):
        for u in range(2):
            tg = [(tags[n - 1 - j] if j < n else 3) for j in range(j0 + 64 * u, j0 + 64 * u + 64)]
            moves3 = variant == "tag3_moves"
            fx = [(g != 2 and (g != 3 or moves3)) for g in tg]
            fy = [(g != 1 and (g != 3 or moves3)) for g in tg]
            cxs, cys = np.cumsum(fx), np.cumsum(fy)
            for lane in range(64):
                j = j0 + 64 * u + lane
                px, py = base_x + int(cxs[lane]), base_y + int(cys[lane])
                g = tg[lane]
                if fx[lane] and not pwm and not 1 <= px <= len(q):
                    outside += 1
                if fy[lane] and not 1 <= py <= len(t):
                    outside += 1
                if j < n:
                    if g not in (0, 1, 2):
                        qa[j], ta[j] = -1, -1           # a byte no lane wrote
                        continue
                    inq, int_ = 1 <= px <= (len(q) if not pwm else px), 1 <= py <= len(t)
                    if pwm:
                        qa[j] = 0 if g == 2 else px
                    else:
                        qa[j] = blank if g == 2 else (int(q[px - 1]) if inq else -1)
                    ta[j] = blank if g == 1 else (int(t[py - 1]) if int_ else -1)
            if variant != "no_carry":
                base_x += int(cxs[-1])
                base_y += int(cys[-1])
    return qa, ta, outside
