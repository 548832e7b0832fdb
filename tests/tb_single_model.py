"""The parallel traceback of one large pair (aln_tb_single_{maps,chain,segments}_kernel), restated as a rule over the ORACLE's path.

Nothing here walks direction words: the input is the path the CPU oracle took (its two aligned strings and its start cell), and the
rule says, strip by strip, which of the chain kernel's ways must have crossed it and whether a walk had to leave the staged window.
A GPU test then compares the class string of `ALN_TRACE_TB` with this one, so a right answer reached by the wrong way is a failure.

Geometry (DESIGN 4.4 "exit maps", 4.5): strips of rows = 64 R rows, strip s holds rows s*rows + 1 .. (s + 1)*rows; the walk starts
at the end cell (core, PWM) or at its diagonal predecessor (legacy: aligner_core.rs:146-147, :232-233) and moves up and left.

  cls 1   the strip the walk starts in: the chain thread walks it from global memory
  cls 2   a strip entered on its bottom row inside the band: the exit-map entry is used
  cls 3   entered outside the band: the chain thread walks it
  cls 4   entered inside the band, but the map's walk was capped before it left the strip: the chain thread walks it

The band on the row `cy` a strip is entered on: the slope-1 line through the walk's first cell (ey, ex) is at column
ex - (ey - cy), clamped at 0; the band starts BAND/2 columns left of it, clamped at 0, and holds BAND columns, clamped at N.

Constants restated from aligner_amd/csrc/aln_traceback.hip (by the names and lines they have there):
  BAND    1024  `#define TB_BAND 1024u` (l. 414), used by tb_band (l. 415-423)
  cap     2 rows + 64 steps: the last arguments of walk_in_strip in aln_tb_single_maps_kernel (l. 459); the loop's test is
          `n < n_stop` (l. 389), `gave_up` is "still inside after the loop" (l. 391)
  window  min(12 R, 48) quads: tb_window_quads (l. 408); a quad is 4 blocks of 16 / R wave steps (stage_window, l. 332-358:
          the window ends with the quad of wave step k_hi)
  BLOCK   256 columns per workgroup of the maps kernel: `__launch_bounds__(256)` (l. 426), grid TB_BAND / 256 (l. 713)
A wave step is k = x - 1 + lane, lane = (y - 1 - y0) / R (walk_in_strip, l. 378-380).
"""
BAND = 1024
BLOCK = 256
LOCAL, GLOBAL = "local", "global"


def cap_steps(rows):
    return 2 * rows + 64


def window_quads(R):
    return min(12 * R, 48)


def band(ey, ex, cy, N):
    """(c_lo, c_hi) of the band on row cy, or None when the row is below the walk's first cell."""
    if cy > ey:
        return None
    c = max(ex - (ey - cy), 0)
    c_lo = max(c - BAND // 2, 0)
    return c_lo, min(N, c_lo + BAND - 1)


def path_from_alignment(legacy, end, start, a, b, blank=98, pwm=False):
    """The walk's first cell and its moves in walk order ('D', 'L', 'T'), from the forward aligned strings.  a: the query string (PWM:
    the column numbers, 0 = no column); b: the target string.  Except for the PWM aligner the strings end with the duplicated seed
    pair, which is no move."""
    n = len(a) - (0 if pwm else 1)
    moves = []
    for j in range(n - 1, -1, -1):
        if (a[j] == 0) if pwm else (a[j] == blank):
            moves.append("T")
        elif b[j] == blank:
            moves.append("L")
        else:
            moves.append("D")
    cy, cx = (end[0] - 1, end[1] - 1) if legacy else end
    dy = sum(m != "L" for m in moves)
    dx = sum(m != "T" for m in moves)
    assert (cy - dy, cx - dx) == tuple(start), ("the strings do not lead from the start cell to the end cell", end, start, dy, dx)
    return (cy, cx), moves


def _leaves(reads, k_hi, R):
    """Does one of the wave steps read lie below the window that ends with the quad of k_hi?"""
    per_quad = 64 // R
    q_hi = k_hi // per_quad
    q_lo = q_hi + 1 - min(window_quads(R), q_hi + 1)
    return any(k // per_quad < q_lo for k in reads)


def classify(mode, M, N, R, first, moves):
    """mode: LOCAL (the path ends at a Beginning cell) or GLOBAL (it ends at the origin through the borders).  first: the walk's first
    cell.  Returns the visited strips from the bottom up, each a dict(strip, cls, entry, delta, steps, interior, seg_leaves_window,
    map_leaves_window, map_gave_up); delta and the two map fields are None where there is no entry on a bottom row (cls 1)."""
    assert mode in (LOCAL, GLOBAL) and R in (1, 2, 4)
    rows = 64 * R
    ey, ex = first
    y, x = first
    out = []
    if (y == 0 or x == 0) and (mode == LOCAL or (y == 0 and x == 0)):
        assert not moves
        return out
    i = 0                                   # next move
    s = 0 if y == 0 else (y - 1) // rows
    cls1 = True
    while True:
        y0 = s * rows
        sy, sx = y, x
        reads, steps, k_moves = [], 0, 0
        # interior: cells with y > y0 and x != 0, each read through the direction words
        while y > y0 and x != 0:
            reads.append(x - 1 + (y - 1 - y0) // R)
            if i == len(moves):
                break                       # the cell read last said Beginning
            m = moves[i]; i += 1
            y -= m != "L"; x -= m != "T"
            steps += 1; k_moves += 1
        ended = i == len(moves) and y > y0 and x != 0
        if not ended:
            if mode == LOCAL:
                ended = y == 0 or x == 0
                assert not ended or i == len(moves)
            elif y == 0:                    # top border: Left to the origin, written inside strip 0
                assert all(m == "L" for m in moves[i:]) and len(moves) - i == x
                steps += x; i += x; x = 0; ended = True
            elif x == 0:                    # left border: Top until the strip is left
                run = y - y0
                assert all(m == "T" for m in moves[i:i + run])
                steps += run; i += run; y = y0
        rec = dict(strip=s, entry=(sy, sx), steps=steps, interior=k_moves, delta=None, map_leaves_window=None, map_gave_up=None)
        k_hi = (sx - 1 if sx else 0) + ((sy - 1 - y0) // R if sy > y0 else 0)
        rec["seg_leaves_window"] = _leaves(reads, k_hi, R)
        if cls1:
            rec["cls"] = 1
            cls1 = False
        else:
            rec["delta"] = sx - (ex - (ey - sy))
            c_lo, c_hi = band(ey, ex, sy, N)
            if not c_lo <= sx <= c_hi:
                rec["cls"] = 3
            else:
                cap = cap_steps(rows)
                # the map's walk: at most `cap` steps; it gave up if it is still inside the strip then
                gave_up = False
                map_reads = reads
                if k_moves >= cap:
                    map_reads = reads[:cap]
                    # where the path stands after cap interior steps: inside iff a further interior read followed
                    gave_up = len(reads) > cap
                rec["map_gave_up"] = gave_up
                rec["cls"] = 4 if gave_up else 2
                x_hi = min(c_hi, c_lo + (sx - c_lo) // BLOCK * BLOCK + BLOCK - 1)
                rec["map_leaves_window"] = _leaves(map_reads, (x_hi - 1 if x_hi else 0) + (rows - 1) // R, R)
        out.append(rec)
        if ended or s == 0:
            break
        s -= 1
    assert i == len(moves), "the path goes on after the walk ended"
    return out


def class_string(strips, M, R):
    ns = (M + 64 * R - 1) // (64 * R)
    digits = ["0"] * ns
    for r in strips:
        digits[r["strip"]] = str(r["cls"])
    return "".join(digits)
