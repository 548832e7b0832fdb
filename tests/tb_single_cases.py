"""Constructed pairs for the parallel traceback of one large pair (tests/tb_single_model.py states the rule they are aimed at).

Every pair is a seeded random protein core with blocks inserted or deleted, so the oracle's path is a diagonal with gap runs of
chosen length at chosen rows; each entry names the class (tb_single_model: 1 own strip, 2 map entry, 3 outside the band, 4 the map's
walk gave up) and the offset from the slope-1 line it is built to hit.  tests/test_tb_single_model_cpu.py confirms every aim on
the oracle's path before a GPU test may rely on it; tests/test_tb_single_gpu.py runs this file as a child process (`main`).

Sequences, as lists of blocks read from the start of both sequences:
  ("m", n)   n residues in both (a diagonal run)         ("q", n)  n residues in the query only (a Left run in the walk)
  ("t", n)   n residues in the target only (a Top run)   ("jq", n) / ("jt", n)  a prefix of one repeated residue, W in the query and
                                                                   P in the target (BLOSUM62 W/P = -4: nothing aligns there)
No pair has a suffix, so a local alignment ends in the last cell and the end cell's row is the target's length.
A gap of L residues costs 11 + 2 (L - 1); identical flanks score about 5 a residue, 1.85 with the real-valued matrix, so the
flanks are L / 2 + 100 residues or more (integer route) and 1.2 L + 100 or more (real-valued, local); global paths are forced.
Border runs: the core global border costs `del` a cell and an interior gap `ext`, so the core oracle leaves the border after a
cell or two; the legacy semantics (linear gaps) keep to it when the residue that opens the match (W) occurs nowhere earlier.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tb_single_model as model  # noqa: E402

CORE_GLOBAL, CORE_LOCAL, LEGACY_GLOBAL, LEGACY_LOCAL = 0, 1, 2, 3
W, P, G = 17, 14, 7                     # Protein codes
SEED = 20260419
DIRECTION_CELLS = 1_500_000             # at or under this many cells every direction is compared as well


class Case:
    def __init__(self, name, route, sem, R, blocks, aim, no_w=False):
        self.name, self.route, self.sem, self.R, self.blocks, self.aim, self.no_w = name, route, sem, R, blocks, aim, no_w

    @property
    def id(self):
        return "%s/%s/R%d" % (self.route, self.name, self.R)

    def mode(self):
        return model.GLOBAL if self.sem in (CORE_GLOBAL, LEGACY_GLOBAL) else model.LOCAL

    def legacy(self):
        return self.sem in (LEGACY_GLOBAL, LEGACY_LOCAL)

    def scheme(self):
        """(matrix, del, ext): BLOSUM62 11 / 2 on the integer route, BLOSUM62 x 0.37 with 11.3 / 2.1 on the one-workgroup route."""
        from aligner_amd.matrices import get_blosum62
        if self.route == "wg":
            return get_blosum62() * 0.37, 11.3, 2.1
        return get_blosum62(), 11.0, 2.0

    def seqs(self):
        import zlib
        rng = np.random.default_rng([SEED, zlib.crc32(self.name.encode())])
        q, t = [], []
        for kind, n in self.blocks:
            if kind == "jq":
                q.append(np.full(n, W, np.uint8))
            elif kind == "jt":
                t.append(np.full(n, P, np.uint8))
            elif kind == "w":                           # one W in both: the residue that opens a match on a border
                q.append(np.full(n, W, np.uint8)); t.append(np.full(n, W, np.uint8))
            elif kind == "qW":
                q.append(np.full(n, W, np.uint8))
            elif kind == "tG":
                t.append(np.full(n, G, np.uint8))
            else:
                r = rng.integers(0, 20, n).astype(np.uint8)
                if self.no_w and kind in ("q", "t"):
                    r[(r == W) | (r == 13) | (r == 18)] = 0   # no W, nor F / Y (the only other residues W does not score negative with)
                if kind in ("m", "q"):
                    q.append(r)
                if kind in ("m", "t"):
                    t.append(r)
        return np.concatenate(q), np.concatenate(t)


def _edge(route, sem_name, sem, R, side, L, flank, top=None, count=2):
    """A gap of L above the end cell: L query residues (side -1: the strips above it are entered L columns left of the line) or L
    target residues (side +1: L columns right).  top: the flank above the gap -- on the right side the line itself must stay 512
    columns or more from column 0 where the strips above the gap are entered, or the band is clamped to [0, 1023] and holds the entry."""
    gap = ("q", L) if side < 0 else ("t", L)
    inside = -512 <= side * L <= 511
    return Case("edge_%s_%s%d" % (sem_name, "m" if side < 0 else "p", L), route, sem, R, [("m", top or flank), gap, ("m", flank)],
                dict(cls=2 if inside else 3, delta=side * L, count=count, **(dict(absent=3) if inside else {})))


def cases():
    out = []
    for R in (1, 2):
        rows = 64 * R
        # band edges: strips entered above the gap keep the whole offset
        for sem_name, sem in (("local", CORE_LOCAL), ("global", CORE_GLOBAL)):
            for L in (511, 512, 513):
                out.append(_edge("single", sem_name, sem, R, -1, L, 420))
            for L in (510, 511, 512):
                out.append(_edge("single", sem_name, sem, R, +1, L, 420, top=1300))
        # clamped bands.  ex < 512: the band is [0, 1023], so +600 is inside it
        out.append(Case("clamp_left_p600", "single", CORE_GLOBAL, R, [("m", 300), ("t", 600), ("m", 200)], dict(cls=2, delta=600, count=2)))
        # c_hi = N: Top moves at x = N first; the offset grows with every strip and leaves the band past +511
        out.append(Case("right_edge_top900", "single", CORE_GLOBAL, R, [("m", 1400), ("t", 900)], dict(cls=3, entry_x=1400, count=2, also=2)))
        # the line runs to column 0 together with the path (local: the path ends there; M = 3 N)
        out.append(Case("line_off_left_local", "single", CORE_LOCAL, R, [("t", 1400), ("m", 700)], dict(cls=2, delta=0, count=3)))
        # legacy global, left border: x == 0 Top runs strip after strip, in the band because c_lo == 0
        out.append(Case("left_border_legacy", "single", LEGACY_GLOBAL, R, [("t", 1400), ("w", 1), ("m", 699)],
                        dict(cls=2, entry_x=0, count=12 // R, border=rows), no_w=True))
        out.append(Case("left_border_core", "single", CORE_GLOBAL, R, [("t", 1400), ("w", 1), ("m", 699)], dict(cls=2, count=3), no_w=True))
        # global, top border: y == 0 at x = 1970, the Left run to the origin is written inside strip 0
        out.append(Case("top_border_legacy", "single", LEGACY_GLOBAL, R, [("q", 1970), ("w", 1), ("m", 129)],
                        dict(strip=0, cls=2, border=1970), no_w=True))
        # the core oracle runs Left along row 1 instead (border cells cost del, gap cells ext): 1970 interior steps in strip 0
        out.append(Case("top_border_core", "single", CORE_GLOBAL, R, [("q", 1970), ("w", 1), ("m", 129)],
                        dict(strip=0, cls=4, seg_leaves=True), no_w=True))
        # the give-up cap: rows + G interior steps against 2 rows + 64
        for G_, cls in ((rows + 63, 2), (rows + 64, 2), (rows + 65, 4)):
            out.append(Case("cap_%d" % G_, "single", CORE_LOCAL, R, [("m", 400), ("q", G_), ("m", 400)],
                            dict(cls=cls, delta=0, interior=rows + G_, count=1, only=True)))
        if R == 1:
            out.append(Case("cap_450", "single", CORE_LOCAL, R, [("m", 400), ("q", 450), ("m", 400)], dict(cls=4, delta=0, interior=64 + 450)))
            # the window: 768 wave steps below the segment's start
            out.append(Case("left_700", "single", CORE_LOCAL, R, [("m", 600), ("q", 700), ("m", 600)],
                            dict(cls=4, seg_leaves=True, also=3)))
        out.append(Case("left_900", "single", CORE_LOCAL, R, [("m", 600), ("q", 900), ("m", 600)],
                        dict(cls=4, delta=0, interior=rows + 900, seg_leaves=True, also=3)))
        # start-cell rows: the target's length is the end cell's row
        for sem_name, sem in (("local", CORE_LOCAL), ("legacy", LEGACY_LOCAL)):
            out.append(Case("rows_256_%s" % sem_name, "single", sem, R, [("jq", 800), ("m", 256)], dict(first_cls1_strip=256 // rows - 1)))
            out.append(Case("rows_257_%s" % sem_name, "single", sem, R, [("jq", 800), ("m", 257)],
                            dict(first_cls1_strip=(255 if sem == LEGACY_LOCAL else 256) // rows)))
            out.append(Case("strip0_only_%s" % sem_name, "single", sem, R, [("jq", 1000), ("m", 50), ("qW", 100), ("tG", 210)],
                            dict(classes="1" + "0" * ((260 + rows - 1) // rows - 1))))
        # legacy local, end cell in row 1: the walk starts in row 0 and ends at once (no tags, no strip)
        out.append(Case("legacy_row1", "single", LEGACY_LOCAL, R, [("w", 1), ("qW", 1399), ("tG", 200)],
                        dict(classes="0" * ((201 + rows - 1) // rows), tags=0)))
        # expand: tag counts around 1024 (per thread 1 -> 2) and 2048, and fewer than a wave's
        for tags in (1022, 1023, 1024, 1025, 2049):
            out.append(Case("tags_%d" % tags, "single", CORE_LOCAL, R, [("m", 500), ("q", 10), ("m", tags - 510)],
                            dict(tags=tags)))
        out.append(Case("tags_under_64", "single", CORE_LOCAL, R, [("jq", 1000), ("m", 25), ("q", 2), ("m", 25), ("qW", 100), ("tG", 210)], dict(tags_max=63)))
    # ---- the one-workgroup route (real-valued matrix)
    for sem_name, sem in (("local", CORE_LOCAL), ("global", CORE_GLOBAL)):
        # R = 4: 256 rows, 576 + steps of 1.25 wave steps: the map's walk from the low columns of a block leaves the window
        out.append(Case("left_300_%s" % sem_name, "wg", sem, 4, [("m", 700), ("q", 300), ("m", 700)], dict(cls=2, delta=0, map_leaves=True)))
    for L in (512, 513):
        out.append(_edge("wg", "local", CORE_LOCAL, 4, -1, L, 720))
    for L in (511, 512, 513):       # 2048 rows at most: global (the path is forced), one strip entered above the gap with the band unclamped
        out.append(_edge("wg", "global", CORE_GLOBAL, 4, +1, L, 380, top=1150, count=1))
    out.append(Case("cap_321", "wg", CORE_LOCAL, 4, [("m", 700), ("q", 321), ("m", 700)], dict(cls=4, delta=0, interior=256 + 321)))
    out.append(_edge("wg", "global", CORE_GLOBAL, 1, -1, 512, 500))
    out.append(_edge("wg", "global", CORE_GLOBAL, 1, -1, 513, 500))
    out.append(Case("cap_129", "wg", CORE_LOCAL, 1, [("m", 400), ("q", 129), ("m", 400)], dict(cls=4, delta=0, interior=64 + 129)))
    out.append(_edge("wg", "local", CORE_LOCAL, 2, -1, 512, 720))
    out.append(_edge("wg", "local", CORE_LOCAL, 2, -1, 513, 720))
    out.append(Case("cap_193", "wg", CORE_LOCAL, 2, [("m", 500), ("q", 193), ("m", 500)], dict(cls=4, delta=0, interior=128 + 193)))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


# ---- the PWM window case: a 4 x 400 real-valued PWM against a 1500-residue window that lacks columns 100 .. 299
PWM_DEL, PWM_EXT, PWM_R = 11.3, 2.1, 4


def pwm_case():
    rng = np.random.default_rng([SEED, 400])
    motif = rng.integers(0, 4, 400).astype(np.uint8)
    pwm = np.round(rng.normal(-4.0, 0.5, (4, 400)), 2)
    pwm[motif, np.arange(400)] = np.round(rng.normal(6.0, 0.25, 400), 2)
    seq = np.concatenate([rng.integers(0, 4, 700), motif[:100], motif[300:], rng.integers(0, 4, 600)]).astype(np.uint8)
    return seq, pwm


def pwm_model(ref):
    first, moves = model.path_from_alignment(False, ref["end"], ref["start"], ref["numbered"], ref["qal"], pwm=True)
    strips = model.classify(model.LOCAL, 1500, 400, PWM_R, first, moves)
    return strips, model.class_string(strips, 1500, PWM_R), moves


def run_model(case, ref):
    """The oracle's answer of a case -> (strips, class string, moves)."""
    q, t = case.seqs()
    first, moves = model.path_from_alignment(case.legacy(), ref["end"], ref["start"], ref["qa"], ref["ta"])
    strips = model.classify(case.mode(), len(t), len(q), case.R, first, moves)
    return strips, model.class_string(strips, len(t), case.R), moves


def oracle(orc, case, want_matrices=False):
    q, t = case.seqs()
    S, dele, ext = case.scheme()
    return orc.align(case.sem, q, t, dele, ext, S, want_matrices=want_matrices)


def check_aim(case, strips, classes, moves):
    """What a case is built to hit, on the oracle's path.  Returns the list of misses (empty: the construction holds)."""
    a, miss = case.aim, []
    if "classes" in a and classes != a["classes"]:
        miss.append("classes %s, built for %s" % (classes, a["classes"]))
    if "tags" in a and len(moves) != a["tags"]:
        miss.append("%d tags, built for %d" % (len(moves), a["tags"]))
    if "tags_max" in a and not 0 < len(moves) <= a["tags_max"]:
        miss.append("%d tags, built for 1 .. %d" % (len(moves), a["tags_max"]))
    if "tags" in a and a["tags"] > 64 and not ("L" in moves or "T" in moves):
        miss.append("no gap in the path")
    if "first_cls1_strip" in a and not (strips and strips[0]["cls"] == 1 and strips[0]["strip"] == a["first_cls1_strip"] and len(strips) > 1
                                        or (strips and a["first_cls1_strip"] == 0 and strips[0]["strip"] == 0)):
        miss.append("the walk starts in strip %s, built for %d" % (strips[0]["strip"] if strips else None, a["first_cls1_strip"]))
    if "cls" in a:
        sel = [r for r in strips if r["cls"] == a["cls"]]
        for key, field in (("delta", "delta"), ("strip", "strip"), ("interior", "interior")):
            if key in a:
                sel = [r for r in sel if r[field] == a[key]]
        if "entry_x" in a:
            sel = [r for r in sel if r["entry"][1] == a["entry_x"]]
        if "border" in a:
            sel = [r for r in sel if r["steps"] - r["interior"] == a["border"]]
        if len(sel) < a.get("count", 1):
            miss.append("%d strips as aimed at (%s), built for %d: %s" % (len(sel), a, a.get("count", 1), classes))
        for key, field in (("seg_leaves", "seg_leaves_window"), ("map_leaves", "map_leaves_window")):
            if key in a and any(r[field] for r in sel) != a[key]:
                miss.append("%s is %s over the aimed strips, built for %s" % (field, not a[key], a[key]))
        if a.get("only") and any(r["cls"] in (3, 4) and r not in sel for r in strips):
            miss.append("a class 3 or 4 strip beside the aimed one: %s" % classes)
    if "absent" in a and str(a["absent"]) in classes:
        miss.append("a class %d strip: %s" % (a["absent"], classes))
    if "also" in a and str(a["also"]) not in classes:
        miss.append("no class %d strip: %s" % (a["also"], classes))
    return miss


# ---- child process: run cases on the GPU in the given order on one context, report what came back
def mark(label):
    sys.stderr.flush()
    sys.stderr.write("tb case: %s\n" % label)
    sys.stderr.flush()


def _gpu_case(case, directions):
    import hashlib
    from aligner_amd import runtime
    q, t = case.seqs()
    S, dele, ext = case.scheme()
    want_d = directions and len(q) * len(t) <= DIRECTION_CELLS
    res, qa, ta, D, _ = runtime.align_pair(case.sem, q, t, dele, ext, S, want_directions=want_d)
    return dict(id=case.id, status=int(res.status), score=float(res.score).hex(), f=float(res.f).hex(), end=[int(res.end_y), int(res.end_x)],
                start=[int(res.start_y), int(res.start_x)], aln_len=int(res.aln_len), flags=int(res.flags),
                qa=qa.tobytes().hex(), ta=ta.tobytes().hex(), D=hashlib.sha256(D.tobytes()).hexdigest() if want_d else None)


def main(argv):
    """argv: report path, "pwm" or a comma-separated list of case ids in the order to run them ("+d": with directions)."""
    report, what = argv[0], argv[1]
    out = []
    if what == "pwm":
        from aligner_amd import runtime
        seq, pwm = pwm_case()
        mark("pwm")
        res, numbered, qal, _, _ = runtime.align_pwm(seq, PWM_DEL, PWM_EXT, pwm)
        out.append(dict(id="pwm", status=int(res.status), score=float(res.score).hex(), f=float(res.f).hex(), end=[int(res.end_y), int(res.end_x)],
                        start=[int(res.start_y), int(res.start_x)], aln_len=int(res.aln_len), flags=int(res.flags),
                        qa=numbered.astype("<u4").tobytes().hex(), ta=qal.tobytes().hex(), D=None))
    else:
        directions = what.endswith("+d")
        by_id = {c.id: c for c in cases()}
        for i, cid in enumerate(what.replace("+d", "").split(",")):
            mark("%d %s" % (i, cid))
            out.append(_gpu_case(by_id[cid], directions))
    sys.stderr.flush()
    with open(report, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1:])
