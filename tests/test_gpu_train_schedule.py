"""The launch schedule of the four training nodes (fast_train._MCForward / _MCForwardBF16 / _MCForwardLRT / _MCForwardLRTBF16) against
the recorded one: every bbb_hip.ops call fast_train makes during one forward + backward, in order, with the stream it lands on (main or
one of the round-robin side streams), the shapes and dtypes of its tensor arguments, and every wait_stream edge.  Stream placement moves
no value, so the value suites (test_*_switches_are_value_neutral) pass whichever stream a launch lands on; this test does not.

tests/golden/train_schedule.json holds the expected traces (its _comment names the commit and the command that produced them);
tests/train_schedule_recorder.py is the recorder and lists the cases: four Bayesian layers on 8 x 8 images at B = 8, a 3-channel
first layer (im2col forked early), a 4-channel one (no fork), a strided second convolution; E = 2 on the four nodes and E = 1 on
the two LRT nodes (the paired g_pair forms); overlap_wgrad / flips_up_front on and off, pair_lrt_backward / fold_lrt_combine off, frozen
parameters with x.requires_grad.  The bf16 node with frozen parameters runs under LaunchConfig.bf16_input_grad
(cin3-bf16-e2-frozen_dx, cin4-bf16-e2-frozen_dx) and behind the strided layer under bf16_strided_train (cin3_s2-bf16-e2-default,
cin3_s2-bf16-e2-frozen_dx); the bf16 LRT node, which has input gradients with frozen parameters alone, under bf16_lrt +
bf16_lrt_input_grad ({cin3,cin4,cin3_s2}-lrt_bf16-e{2,1}-frozen_dx).  A side-stream count of 0 must give the schedule of
overlap_wgrad off.  Run with -m gpu."""
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


def _assert_same(cid, got, want):
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (f"{cid}: {len(got)} events against {len(want)} recorded; first difference at event {first}: "
                         f"got {got[first] if first < len(got) else None!r}, recorded {want[first] if first < len(want) else None!r}")


def test_golden_lists_exactly_the_cases(expected):
    assert sorted(expected) == sorted(CASES)


@pytest.mark.parametrize("cid", list(CASES))
def test_schedule_matches_recorded(cid, expected, monkeypatch):
    _assert_same(cid, R.record(CASES[cid], monkeypatch), expected[cid])


@pytest.mark.parametrize("cid, recorded_as", [("cin4-fp32-e2-default", "cin4-fp32-e2-overlap_off"),
                                              ("cin3-lrt-e2-default", "cin3-lrt-e2-overlap_off")])
def test_no_side_streams_is_the_schedule_of_overlap_off(cid, recorded_as, expected, monkeypatch):
    """fast_train.n_side_streams (BBB_TRAIN_SIDE_STREAMS) below 1: no side streams -- every launch on main, no wait -- instead of a
    round robin over none of them (a ZeroDivisionError in the first eager backward)."""
    model, node, draws, variant = CASES[cid]
    got = R.record((model, node, draws, dict(variant, side_streams=0)), monkeypatch)
    _assert_same(f"{cid} without side streams", got, expected[recorded_as])
