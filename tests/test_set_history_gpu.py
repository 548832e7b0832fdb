"""No result of a resident sequence set may depend on the handle's call history (helpers, catalogue and state model: tests/set_history.py).

One handle of a 48-protein set runs call_history.schedule(24): 577 calls in which every one of the 24 catalogue entries -- five passes
that replace the held hits, two that hold nothing, the two indexes and three candidate lists, nine consumers of the held hits and the
two fills alone -- directly follows every other one and itself exactly once, so that every grow-only buffer shrinks and grows, every
counter word is written by every family in both orders, and every plan meets every pass.  After each of them one call on a
stranded set's handle on the same context.  Every answer is compared, bit for bit over whole arrays, with values that come from the CPU
oracle and the Python rule restatements; every call the state model refuses must be refused and must leave its marker-filled outputs
untouched.  The same walk runs in a child process under a small ALN_CHUNK_CELLS, and the first 24 calls run again on a new set after
the first was destroyed under a live derived pair set."""
import json
import os
import subprocess
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import set_history as H  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = 2 * (len(H.CATALOGUE) ** 2 + 1)


@pytest.fixture(scope="module")
def refs(orc):
    r = H.Refs(H.set_a(), H.set_b(), orc)
    for name in H.needed():
        r.get(name)
    return r


@pytest.fixture(scope="module")
def walked(refs):
    """the in-process walk, once: (backend with both handles as the walk left them, its report)"""
    backend = H.GpuBackend(refs.a, refs.recs_b)
    t0 = time.perf_counter()
    out = H.walk(backend, refs)
    out["seconds"] = time.perf_counter() - t0
    yield backend, out
    backend.close()


def describe(out):
    return "\n".join(f["message"] for f in out["failures"][:12]) + "\n(%d failures in %d calls)" % (len(out["failures"]), out["calls"])


def test_walk_in_process(walked):
    backend, out = walked
    print("walk: %d calls in %.2f s (%.2f s inside the library's calls), refusals %s" % (out["calls"], out["seconds"], backend.seconds, out["refusals"]))
    assert not out["failures"], describe(out)
    assert out["calls"] == CALLS and all(v >= 3 for v in out["refusals"].values()), out["refusals"]
    assert backend.score_chunks[H.BIG] == 1


def test_walk_in_small_chunks(refs, tmp_path):
    """ALN_CHUNK_CELLS in a child process (the variable is read per call, and the other tests must not see it): the large pass and the
    large score run in three chunks or more -- by the rule and by the bytes the score brought down -- so that per-chunk buffers, plans
    and events are reused inside the calls as well as between them.  The expected values are the parent's, through a file."""
    lens = [len(s) for s in refs.a]
    chunks = H.planned_chunks(lens, H.BIG, H.CHUNK_CELLS)
    assert chunks >= 3
    expected, report = str(tmp_path / "expected.npz"), str(tmp_path / "report.json")
    refs.save(expected)
    env = dict(os.environ, ALN_CHUNK_CELLS=str(H.CHUNK_CELLS))
    t0 = time.perf_counter()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "set_history.py"), expected, report], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with open(report) as f:
        out = json.load(f)
    print("chunked walk: %d calls in %.2f s (child process %.2f s), %d chunks" % (out["calls"], out["seconds"], time.perf_counter() - t0, out["score_chunks"]))
    assert not out["failures"], describe(out)
    assert out["calls"] == CALLS and out["score_chunks"] == chunks


def test_destroy_in_the_middle(walked, orc):
    """After the walk A is destroyed while a pair set derived from it is alive (its residue buffer outlives it); A' holds other records
    of the same shapes.  The first k calls of the schedule on A': nothing of A may show through."""
    backend, _out = walked
    k = len(H.CATALOGUE)
    other = H.set_a(seed=977)
    assert [len(s) for s in other] != [len(s) for s in H.set_a()] or any(a.tobytes() != b.tobytes() for a, b in zip(other, H.set_a()))
    refs2 = H.Refs(other, H.set_b(), orc)
    for name in H.needed(k):
        refs2.get(name)
    assert len(refs2.held("hits_large")) > 512
    t0 = time.perf_counter()
    ps = backend.replace_a(other)
    try:
        out = H.walk(backend, refs2, calls=k)
    finally:
        backend.lib.aln_pairset_destroy(ps)
    print("after the destroy: %d calls in %.2f s" % (out["calls"], time.perf_counter() - t0))
    assert not out["failures"], describe(out)
    assert out["calls"] == 2 * k
