"""The held-hits path of the repeat search without a GPU: filter_hits against filter_tasks, and the engine on a scan that
offers `hits` (computed from the CPU oracle) against the engine on the plain select path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aligner_amd import repeats as R                                              # noqa: E402
from aligner_amd.errors import ReferencePanic                                     # noqa: E402
from repeats_oracle_backend import RecordingBackend                               # noqa: E402
import repeats_held_backend as H                                                  # noqa: E402


def _random_hits(rng, case):
    n = int(rng.integers(0, 401))
    step = int(rng.integers(1, 40))
    reach = int(rng.integers(1, 13))                         # how many neighbours a window overlaps
    if case % 2:
        width = np.full(n, step * reach - (1 if rng.random() < 0.5 else 0), dtype=np.int64)
    else:
        width = rng.integers(1, step * reach + 1, n)
    if case % 5 == 0:                                        # repeated left_coords
        left = np.sort(rng.integers(0, max(1, n // 2), n)) * step
    elif case % 7 == 0:                                      # one run that overlaps to the very end
        left = np.arange(n, dtype=np.int64)
        width = np.full(n, 10 * n + 5, dtype=np.int64)
    else:                                                    # gaps now and then: clusters and singletons
        left = np.cumsum(rng.choice([step, step, step, step * (reach + 2)], n)) if n else np.zeros(0, dtype=np.int64)
    left = np.asarray(left, dtype=np.int64)
    z = rng.integers(3, 7, n).astype(np.float64) if case % 3 else rng.normal(5.0, 2.0, n)     # many ties / none
    perm = rng.permutation(n) if case % 4 == 0 else np.arange(n)                              # unsorted input too
    return left[perm], (left + width)[perm], z[perm]


def _both(left, right, z):
    tasks = [R.Task(None, l, r, float(v)) for l, r, v in zip(left, right, z)]
    for p, t in enumerate(tasks):
        t.alignment = p                                      # the position in the input
    try:
        want = [t.alignment for t in R.filter_tasks(tasks)]
    except ReferencePanic:
        want = "panic"
    try:
        got = R.filter_hits(left, right, z).tolist()
    except ReferencePanic:
        got = "panic"
    return want, got


def test_filter_hits_equals_filter_tasks():
    rng = np.random.default_rng(20240)
    kept = dropped = 0
    for case in range(2400):
        left, right, z = _random_hits(rng, case)
        want, got = _both(left, right, z)
        assert want != "panic" and got == want, case
        kept += len(got)
        dropped += len(left) - len(got)
    assert kept > 10000 and dropped > 10000


def test_filter_hits_nan_inside_a_cluster_panics_in_a_singleton_does_not():
    left = np.array([0, 10, 20, 500, 900, 910], dtype=np.int64)
    right = left + 25
    z = np.array([4.0, np.nan, 5.0, np.nan, 3.0, 3.0])
    assert _both(left, right, z) == ("panic", "panic")
    with pytest.raises(ReferencePanic):
        R.filter_hits(left, right, z)
    z = np.array([4.0, 6.0, 5.0, np.nan, 3.0, 3.0])          # the NaN is alone: nothing compares it
    want, got = _both(left, right, z)
    assert got == want == [1, 3, 5]
    rng = np.random.default_rng(5)
    for case in range(200):                                  # a NaN somewhere in random inputs: the same outcome either way
        left, right, z = _random_hits(rng, case)
        if len(z) == 0:
            continue
        z[int(rng.integers(0, len(z)))] = np.nan
        want, got = _both(left, right, z)
        assert got == want, case


def test_filter_hits_small_inputs():
    assert R.filter_hits([], [], []).tolist() == []
    assert R.filter_hits([7], [9], [np.nan]).tolist() == [0]
    assert R.filter_hits([5, 5], [9, 9], [1.0, 1.0]).tolist() == [1]


@pytest.mark.parametrize("case", range(3))
def test_engine_on_held_hits_equals_engine_on_select(case):
    name, raw, opts, seed = H.engine_cases()[case]
    plain, held = RecordingBackend(H.MemoOracleBackend()), H.RecordingHeldBackend(H.HeldOracleBackend())
    a = H.run_engine(raw, opts, seed, held)
    b = H.run_engine(raw, opts, seed, plain)
    H.assert_same_engine(a, b, held.log, plain.log)
    fwd, rev, n_direct, n_inverse = H.case_properties(plain.log, b)
    # the properties the inputs were chosen for
    if name != "flipped":                                                                     # an empty cycle after a non-empty one:
        assert any(k == 0 and fwd[i - 1] > 0 for i, k in enumerate(fwd) if i), (name, fwd)     # the tasks returned are the one's before
    assert n_direct > 0 and any(n_direct < k for k in fwd), (name, fwd, n_direct)             # the filter drops hits
    if name == "flipped":
        assert rev and rev[0] > 0 and 0 < n_inverse < rev[0], (name, rev, n_inverse)           # a reverse pass with hits
    # alignments are asked for kept hits only, never for a whole cycle's hits where the filter dropped some
    for what, n_hits, n_keep in held.kept:
        assert n_keep <= n_hits
    got = [n_keep for what, n_hits, n_keep in held.kept if what == "alignments"]
    assert sum(got) < sum(k for k in fwd + rev), (name, got, fwd, rev)


def test_calculate_cycle_on_held_hits_returns_every_task_with_its_alignment():
    name, raw, opts, seed = H.engine_cases()[0]
    query, freqs, indices = R.DNA.from_u8_vec_with_freqs_and_indices(raw)
    m = R._transform(R.get_random_pwm(opts.repeat_length, np.random.default_rng(1)), opts, freqs)
    a = R.calculate_cycle(query, m, indices, 10.0, 4.0, opts, H.HeldOracleBackend())
    b = R.calculate_cycle(query, m, indices, 10.0, 4.0, opts, H.MemoOracleBackend())
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert (x.left_coord, x.right_coord, x.z) == (y.left_coord, y.right_coord, y.z) and H.same_alignment(x.alignment, y.alignment)
