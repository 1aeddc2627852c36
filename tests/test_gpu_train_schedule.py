"""The launch schedule of the three training nodes (fast_train._MCForward / _MCForwardBF16 / _MCForwardLRT) against the recorded
one: every bbb_hip.ops call fast_train makes during one forward + backward, in order, with the stream it lands on (main or one of the
round-robin side streams), the shapes and dtypes of its tensor arguments, and every wait_stream edge.  Stream placement moves no
value, so the value suites (test_*_switches_are_value_neutral) pass whichever stream a launch lands on; this test does not.

tests/golden/train_schedule.json holds the expected traces (its _comment names the commit and the command that produced them);
tests/train_schedule_recorder.py is the recorder and lists the cases: four Bayesian layers on 8 x 8 images at B = 8, a 3-channel
first layer (im2col forked early), a 4-channel one (no fork), a strided second convolution; E = 2 on the three nodes and E = 1 on
the LRT node (the paired g_pair forms); overlap_wgrad / flips_up_front on and off, pair_lrt_backward / fold_lrt_combine off, frozen
parameters with x.requires_grad.  Run with -m gpu."""
import json
import os

import pytest

import train_schedule_recorder as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_schedule.json")
CASES = R.cases()


@pytest.fixture(scope="module")
def expected():
    with open(GOLDEN) as f:
        return json.load(f)["traces"]


def test_golden_lists_exactly_the_cases(expected):
    assert sorted(expected) == sorted(CASES)


@pytest.mark.parametrize("cid", list(CASES))
def test_schedule_matches_recorded(cid, expected, monkeypatch):
    got = R.record(CASES[cid], monkeypatch)
    want = expected[cid]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (f"{cid}: {len(got)} events against {len(want)} recorded; first difference at event {first}: "
                         f"got {got[first] if first < len(got) else None!r}, recorded {want[first] if first < len(want) else None!r}")
