"""The repeat-search engine's host logic (aligner_amd/repeats.py) without a GPU: filter, coordinates, window sets, the reference's
summation order and statistics, the output formats and the CLI's masking -- with a fake scoring backend."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aligner_amd import repeats as R                      # noqa: E402
from aligner_amd.enums import DNA, Index                  # noqa: E402
from aligner_amd.errors import ReferencePanic             # noqa: E402
from aligner_amd.pwm import PWMAlignment                  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _task(z, left, right, f=0.0):
    return R.Task(PWMAlignment(DNA, [], [], 0, ((0, 0), (0, 0)), f), left, right, z)


def test_filter_reference_vectors():
    kat = json.load(open(os.path.join(GOLDEN, "repeat_filter_kat.json")))
    got = R.filter_tasks([_task(t["z"], t["left_coord"], t["right_coord"]) for t in kat["tasks"]])
    assert [(t.z, t.left_coord, t.right_coord) for t in got] == [(t["z"], t["left_coord"], t["right_coord"]) for t in kat["expected"]]


def test_filter_reexamines_last_task_of_an_overlapping_run():
    # every task overlaps the first: the loop ends on index len-2, so the last task is examined again as a cluster of its own
    tasks = [_task(5.0, 0, 100), _task(4.0, 10, 110), _task(3.5, 20, 120)]
    got = R.filter_tasks(tasks)
    assert [(t.left_coord, t.z) for t in got] == [(0, 5.0), (20, 3.5)]
    # ... unless it is the kept one: `contains` compares left_coord only
    tasks = [_task(3.0, 0, 100), _task(4.0, 10, 110), _task(9.0, 20, 120)]
    assert [(t.left_coord, t.z) for t in R.filter_tasks(tasks)] == [(20, 9.0)]
    # the cluster is tested against its FIRST task only, and equal z keep the last
    tasks = [_task(3.0, 0, 10), _task(3.0, 5, 30), _task(3.0, 20, 40)]
    assert [(t.left_coord, t.z) for t in R.filter_tasks(tasks)] == [(5, 3.0), (20, 3.0)]
    assert R.filter_tasks([]) == [] and len(R.filter_tasks([_task(1.0, 3, 4)])) == 1


def _indices_reference(raw):
    """enums.rs:489-522 as a plain loop."""
    indices, count, local, passing, kept = [], 0, 0, True, 0
    for i, b in enumerate(raw):
        if chr(b) in "ATCG_+":
            if not passing:
                indices.append(Index(i - count, count, local))
                local = 0
                passing = True
            kept += 1
        else:
            passing = False
            count += 1
            local += 1
    return indices[::-1]


@pytest.mark.parametrize("raw", [b"NNNACGTA", b"ACGNNNNTTA", b"ACGTNN", b"NNACNNNNGTNAC", b"nNACGT", b"ACGT", b"NNNN", b""])
def test_from_u8_vec_with_freqs_and_indices(raw):
    codes, freqs, idx = DNA.from_u8_vec_with_freqs_and_indices(raw)
    assert idx == _indices_reference(raw)
    assert codes.tolist() == [("ATCG").index(chr(b)) for b in raw if chr(b) in "ATCG"]
    if len(codes):
        assert freqs.tolist() == (np.bincount(codes, minlength=4) / len(codes)).tolist()


def test_indices_hand_cases():
    _c, _f, idx = DNA.from_u8_vec_with_freqs_and_indices(b"NNACNNNGT")
    assert idx == [Index(2, 5, 3), Index(0, 2, 2)]
    assert DNA.from_u8_vec_with_freqs_and_indices(b"ACNN")[2] == []     # a run at the end leaves nothing


def test_index_coord_and_rotate_indices():
    idx = [Index(2, 5, 3), Index(0, 2, 2)]                 # "NNACNNNGT": kept AC GT
    assert [R.index_coord(j, idx) for j in range(5)] == [2, 3, 7, 8, 9]
    assert R.index_coord(7, []) == 7
    # the reversed kept sequence "TGCA" of the reversed raw "TGNNNCANN": runs end at kept 2 (offset 3)
    rot = R.rotate_indices(idx, 4)
    assert rot == [Index(4, 5, 2), Index(2, 3, 3)]
    assert [R.index_coord(j, rot) for j in range(4)] == [0, 1, 5, 6]
    assert R.rotate_indices([], 10) == []


def test_window_starts():
    o = R.Options(query_offset=30, threads=1)
    s, _ = R.starting_window_starts(1000, o)
    assert s.tolist() == list(range(0, 1000, 30))
    o = R.Options(query_offset=30, threads=3)
    s, _ = R.starting_window_starts(1000, o)
    assert s.tolist() == list(range(0, 1000, 30))           # the threads' ranges together are every multiple of qo
    o = R.Options(query_offset=30, threads=1, simple_init=True)
    s, _ = R.starting_window_starts(5000, o)
    assert s.tolist() == list(range(0, 5000, 5))
    o = R.Options(query_offset=30, threads=3, simple_init=True)   # --threads changes the window set here
    s, _ = R.starting_window_starts(5000, o)
    want = sorted(j for i in range(3) for j in range(i * 30, 5000, 15))
    assert s.tolist() == want and s.tolist() != list(range(0, 5000, 5))
    with pytest.raises(ReferencePanic):
        R.starting_window_starts(999, R.Options(simple_init=True))        # len / 1000 == 0: step_by(0)
    with pytest.raises(ReferencePanic):
        R.starting_window_starts(999, R.Options(query_offset=0))
    with pytest.raises(ReferencePanic):
        R.cycle_step(R.Options(query_offset=0))
    assert R.cycle_step(R.Options(query_offset=30, threads=4)) == 30


def test_sequential_sum():
    x = np.array([1e16, 1.0, -1e16, 1.0] * 3 + [0.1] * 7)
    want = 0.0
    for v in x:
        want += v
    assert R.seq_sum(x) == want
    assert R.seq_sum(x) != np.sum(x) and R.seq_sum(x) != math.fsum(x)     # the vector tells the three orders apart
    mean, var = R.mean_and_variance(x)
    m = want / len(x)
    acc = 0.0
    for v in x:
        acc += (v - m) * (v - m)
    assert mean == m and var == acc / len(x)


class FakeScan:
    """f of window k = table[k]; select = the z test on the host."""

    def __init__(self, owner, seq):
        self.owner, self.len = owner, len(seq)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def close(self):
        pass

    def _f(self, first, step):
        return np.array([self.owner.fvalue(j) for j in range(first, self.len, step)], dtype=np.float64)

    def score(self, matrix, d, e, first, step, width, reverse=False):
        self.owner.log.append(("score", None, None))
        return self._f(first, step)

    def select(self, matrix, d, e, first, step, width, mean, sd, z_min, reverse=False):
        self.owner.log.append(("select", float(mean), float(sd)))
        f = self._f(first, step)
        with np.errstate(divide="ignore", invalid="ignore"):
            idx = np.flatnonzero((f - mean) / sd >= z_min)
        W = np.asarray(matrix).shape[1]
        alns = [PWMAlignment(DNA, np.arange(1, 4), np.zeros(3, np.uint8), W, ((1, 3), (1, 3)), f[k]) for k in idx]
        return idx, alns


class FakeBackend:
    def __init__(self, fvalue):
        self.fvalue, self.log = fvalue, []

    def scan(self, seq):
        return FakeScan(self, seq)


def test_std_after_a_cycle_is_the_variance():
    rng = np.random.default_rng(0)
    hot = {1000: 50.0, 3000: 60.0, 6000: 58.0}
    be = FakeBackend(lambda j: hot.get(j, float(j % 7)))
    raw = rng.choice(np.frombuffer(b"ACGT", np.uint8), 9000).tobytes()
    opts = R.Options(repeat_length=60, query_offset=10, repeats=3)
    r = R.perform_calculation_per_sequence(opts, raw, "x", np.random.default_rng(1), be)
    sel = [e for e in be.log if e[0] == "select"]
    assert len(sel) == 2                                       # cycle 2 finds nothing at z >= 3 against the variance: break
    fs = np.array([50.0, 60.0, 58.0])
    mean = R.seq_sum(fs) / 3
    var = R.seq_sum((fs - mean) * (fs - mean)) / 3
    assert sel[1][1] == mean and sel[1][2] == var and sel[1][2] != np.sqrt(var)
    tasks, m = r["direct"]
    assert [t.left_coord for t in tasks] == [1000, 3000, 6000]


def test_empty_cycle_breaks_and_keeps_previous_state():
    be = FakeBackend(lambda j: 100.0 if j == 500 else 0.0)
    raw = b"ACGT" * 1000
    opts = R.Options(repeat_length=60, query_offset=10, repeats=5, reverse=True)
    r = R.perform_calculation_per_sequence(opts, raw, "x", np.random.default_rng(1), be)
    sel = [e for e in be.log if e[0] == "select"]
    # cycle 1: one hit; cycle 2: std = 0 -> z = 0/0 for the hit itself (NaN fails), others -inf: empty -> break; then reverse
    assert len(sel) == 3
    assert [t.left_coord for t in r["direct"][0]] == [500]
    assert sel[2][1:] == sel[1][1:]                            # the reverse pass gets the final mean and std
    assert set(r) == {"direct", "inverse"}


def test_output_formats_and_default_paths(tmp_path):
    csv_p, json_p = R.output_paths(None, cwd=str(tmp_path))
    assert csv_p == os.path.join(str(tmp_path), "output.csv") and json_p == os.path.join(str(tmp_path), "matrices.json")
    assert R.output_paths("res/x.csv") == ("res/x.csv", "res/x.csv.matrices.json")
    m = np.arange(8, dtype=np.float64).reshape(4, 2) / 3
    result = {"chr1": ([_task(3.25, 10, 40), _task(0.1 + 0.2, 50, 80)], m), "chr1-reversed": ([], m * 2)}
    R.write_outputs(result, csv_p, json_p)
    assert open(csv_p).read().splitlines() == ["name,z_value,left_coord,right_coord", "chr1,3.25,10,40",
                                               "chr1,0.30000000000000004,50,80"]
    js = json.load(open(json_p))
    assert list(js) == ["chr1", "chr1-reversed"]
    assert js["chr1"] == {"v": 1, "dim": [4, 2], "data": m.ravel().tolist()}


def test_csv_masking(tmp_path):
    p = tmp_path / "m.csv"
    p.write_text("name,z_value,left_coord,right_coord\nchrA,4.5,2,5\nchrB,3.0,0,1\nchrA,3.1,7,8\n")
    recs = R.read_records_csv(str(p))
    assert recs == {"chrA": [(2, 5), (7, 8)], "chrB": [(0, 1)]}
    assert R.prepare_sequence(b"ACGTACGTAC", recs["chrA"]) == b"ACNNNCGNAC"


def test_cli_masks_records_named_like_the_head(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">chrA\nACGTACGTACGTACGTACGT\n>chrB\nTTTTGGGGCCCCAAAATTTT\n")
    mask = tmp_path / "m.csv"
    mask.write_text("name,z_value,left_coord,right_coord\nchrA,4.5,4,12\n")
    seen = []

    class Spy(FakeBackend):
        def scan(self, seq):
            seen.append(np.array(seq))
            return FakeScan(self, seq)

    out = tmp_path / "o.csv"
    R.main(["-i", str(fa), "-o", str(out), "--csv", str(mask), "-r", "4", "-q", "2", "--repeats", "1", "--seed", "3"],
           backend=Spy(lambda j: 0.0))
    # chrA lost its masked 8 residues before encoding; chrB is whole (the first scan of each record is the shuffled copy)
    lens = sorted({len(s) for s in seen})
    assert lens == [12, 20]
    assert out.exists() and (tmp_path / "o.csv.matrices.json").exists()
    assert list(json.load(open(str(out) + ".matrices.json"))) == ["chrA", "chrB"]


def test_random_pwm_and_descendants():
    rng = np.random.default_rng(5)
    m = R.get_random_pwm(7, rng)
    assert m.shape == (4, 7) and set(np.unique(m)) <= {-1.0, 0.0, 1.0}
    base = np.zeros(21, np.uint8)
    ds = R.generate_descendants(base, 10, 4, np.random.default_rng(1))
    assert len(ds) == 10
    for i, d in enumerate(ds):
        untouched = [k for k in range(21) if k < i or (k - i) % 4]
        assert (d[untouched] == 0).all()
