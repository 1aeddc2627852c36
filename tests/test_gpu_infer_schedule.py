"""The batch-innermost inference forward (ensemble._mc_logits_chwn) against what was recorded from the commit before it was cut
into partition / plan / operands / walk: per case, every bbb_hip.ops launch in order with its stream, tensor shapes / dtypes, scalar
arguments and wait_stream edges; the (tag, info) list a timers= object sees (bench.py's roofline); the sha256 of the logits' and kl's
bytes -- all three compared with ==.  tests/golden/infer_schedule.json holds them (its _comment names the commit and the command);
tests/infer_schedule_recorder.py is the recorder and lists the cases.  The query ensemble.chwn_plan must name exactly the launches
of the recorded walk, so it cannot drift from it.  Run with -m gpu."""
import json
import os

import pytest

import infer_schedule_recorder as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infer_schedule.json")
CASES = R.cases()
# form -> the bbb_hip.ops function of its launch (a pool / a conversion: by the layout h arrives in)
FORM_OPS = {"s2d_lrt": "lrt_conv2d_c8x3_forward", "s2d_bbb": "conv2d_c8x3_forward", "bf16_bbb": "conv2d_chwn_bf16_forward",
            "c8x3_lrt": "lrt_conv2d_c8x3_forward", "c8x3_bbb": "conv2d_c8x3_forward", "fp32_bbb": "conv2d_chwn_forward",
            "bf16_lrt": "lrt_conv2d_chwn_bf16_forward", "fp32_lrt": "lrt_conv2d_chwn_forward", "to_c8s3": "c8s3_from_f32",
            ("to_f32", "s3"): "s3_to_f32", ("to_f32", "c8s3"): "c8s3_to_f32", ("pool", "c8s3"): "maxpool_c8s3",
            ("pool", "s3"): "maxpool_chwn_s3", ("pool", "bf16"): "maxpool_chwn_bf16", ("pool", "bf16c8"): "maxpool_chwn_bf16",
            ("pool", "f32"): "maxpool_chwn"}
WALK_OPS = set(FORM_OPS.values())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_lists_exactly_the_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    assert all(c["logits"] and c["kl"] for c in golden["cases"].values())


@pytest.mark.parametrize("cid", list(CASES))
def test_forward_matches_recorded(cid, golden, monkeypatch):
    from bbb_hip import ensemble, ops
    case, want = CASES[cid], golden["cases"][cid]
    got = R.record(case, monkeypatch)
    first = next((i for i, (a, b) in enumerate(zip(got["trace"], want["trace"])) if a != b), min(len(got["trace"]), len(want["trace"])))
    assert got["trace"] == want["trace"], (f"{cid}: first difference at event {first}: "
                                           f"got {got['trace'][first:first + 1]}, recorded {want['trace'][first:first + 1]}")
    assert got["brackets"] == want["brackets"]
    assert (got["logits"], got["kl"]) == (want["logits"], want["kl"])
    # the query names exactly the launches of the recorded walk (every stream of a split step runs the same forms)
    with ops.use_config(**case["cfg"]):
        steps = ensemble.chwn_plan(R.build(case["model"], case["kind"]), R.x_shape(case), case["draws"], case["precision"],
                                   **{k: v for k, v in case["kw"].items() if k in ("units", "groups", "share")})
    named = [FORM_OPS.get(st.form) or FORM_OPS[(st.form, "bf16" if (st.form == "pool" and case["precision"] == "bf16") else st.in_layout)]
             for st in steps if st.form not in ("relu", "softplus", "flatten")]
    streams = ("side0", "side1") if case["kw"].get("streams", 1) > 1 else ("main",)
    for tag in streams:
        ran = [ev.split()[1] for ev in want["trace"] if ev.split()[0] == tag and ev.split()[1] in WALK_OPS]
        assert ran == named, (cid, tag)


def test_fallback_by_value_and_path(golden):
    """A flatten whose rows do not divide an image: the forward answers None (now before anything is launched) and mc_logits
    computes on the reference-layout path what it computed before."""
    assert R.fallback() == golden["fallback"]
    from bbb_hip import ensemble
    assert ensemble.chwn_plan(R.build(R.FALLBACK["model"], R.FALLBACK["kind"]), R.x_shape(R.FALLBACK), 2) is None
