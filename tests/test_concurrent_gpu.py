"""Concurrent callers of every family on ONE context (tests/concurrent_cases.py): rounds of six threads, every repetition of every
thread compared with the CPU oracle's expectation and the route predicate, and the overlap of the library calls read off their time
stamps.  All threads live in this process; no environment knob is set.

Measured on an MI355X: see DESIGN 4.24c."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import concurrent_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu
OVERLAP_CAP = 0.10                   # at most this share of the scheduled pairs may lack an observed overlap


@pytest.fixture(scope="module")
def wants(orc):
    return CC.expectations(orc)


class Results:
    """the records of a list of rounds: run once, left unchanged"""

    def __init__(self, rounds, wants, reps):
        self.rounds, self.records = rounds, []
        for r in rounds:
            self.records.append(CC.run_round(r, wants, reps))        # (raises, and ends the module's GPU work, if a round hangs or raises)

    def failures(self):
        return [f for recs in self.records for f in CC.failures_of(recs)]

    def observed(self):
        return set().union(*(CC.overlaps(recs) for recs in self.records))


@pytest.fixture(scope="module")
def general(wants):
    return Results(CC.rounds(), wants, CC.REPS)


@pytest.fixture(scope="module")
def dedicated(wants):
    return Results(CC.lds_rounds(), wants, CC.LDS_REPS)


def test_every_pair_of_jobs_side_by_side(general):
    assert all(rec.reps_done == CC.REPS for recs in general.records for rec in recs)
    bad = general.failures()
    assert not bad, "%d repetitions differ from the oracle or left their route; first: %s" % (len(bad), bad[:5])


def test_lds_opt_in_sizes_side_by_side(dedicated):
    """Two sizes above 64 KiB asked of one kernel from six threads at once: every repetition is the oracle's."""
    assert all(rec.reps_done == CC.LDS_REPS >= 200 for recs in dedicated.records for rec in recs)
    bad = dedicated.failures()
    assert not bad, "%d repetitions differ from the oracle or left their route; first: %s" % (len(bad), bad[:5])


def test_refusals_keep_their_own_error_text(wants):
    """Two calls the library refuses with different status and text, beside four working jobs: aln_last_error() on a thread is that
    thread's (compared in every repetition: concurrent_cases.REFUSALS refused calls each)."""
    recs = CC.run_round(CC.refusal_round(), wants, CC.REPS)
    bad = CC.failures_of(recs)
    assert not bad, bad[:5]
    assert all(rec.reps_done == CC.REPS for rec in recs)


def test_overlap_was_observed(general, dedicated):
    """A run in which nothing overlapped tested nothing: of the scheduled pairs at most one in ten may lack two library calls that
    overlapped in time, and no pair inside the LDS group may."""
    scheduled = CC.covered(general.rounds)
    seen = general.observed()
    missing = sorted(scheduled - seen)
    share = len(missing) / len(scheduled)
    print("overlap: %d of %d scheduled pairs observed, %.1f %% missing: %s" % (len(scheduled) - len(missing), len(scheduled), 100 * share, missing))
    lds_seen = dedicated.observed()
    lds_missing = [p for r in dedicated.rounds for p in CC.covered([r]) if p not in lds_seen]
    print("LDS rounds: missing %s" % lds_missing)
    assert not lds_missing, lds_missing
    assert share <= OVERLAP_CAP, "%d of %d scheduled pairs never overlapped: %s" % (len(missing), len(scheduled), missing)
