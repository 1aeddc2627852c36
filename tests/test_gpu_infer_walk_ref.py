"""The batch-innermost inference forward (ensemble._mc_logits_chwn: partition, plan, operands, walk) held BY VALUE to a float64
forward of the same model on the CPU (tests/infer_ref.py, fed the device's Philox noise), run by run over tests/infer_walk_cases.py:
the 44 recorded cases of tests/infer_schedule_recorder.py (whose golden pins their schedule and bits, not their values), the
fall-back case, and a table of small models with the geometry those lack -- rectangular kernels, strides, dilation, overlapping /
gapped / floor-cut pools, average pools, layers that leave and rejoin the MFMA-ready chain, missing biases, two priors, more than 16
parameter tensors, mixed BBB / LRT models -- each under every precision and configuration it admits, two of them under every partition.

Every run first asserts that ensemble.chwn_plan names exactly the steps tests/golden/infer_walk_plans.json expects of it (a planner
change must fail the run, not move it off its form), then compares every output slab with the reference of the images, noise call and
global image offset tests/infer_ref.slab_sources states for it:

    ratio = max |got - want64| / max |want64|
    fp32, bf16x3   ratio <= max(4 ratio_twin, floor) and ratio <= 2e-5; ratio_twin: the same forward in plain CPU fp32; floor 4e-6,
                   1e-5 for models with an LRT layer (tests/test_gpu_parity_fullsize.py's figures)
    bf16           ratio <= 1e-2 against the reference under the bf16 storage contract's roundings
    kl             |kl - kl64| <= 2e-6 kl64 (unpartitioned runs)

tests/test_infer_ref_cpu.py checks, on the CPU, that wrong answers lie far outside these bounds.  Run with -m gpu (-s for the table
of worst ratios per form set, precision and kind)."""
import re

import pytest
import torch

import infer_ref as IR
import infer_schedule_recorder as R
import infer_walk_cases as C

pytestmark = pytest.mark.gpu

RUNS = C.runs()
WORST = {}                       # (form set, precision, kind) -> [worst ratio, worst twin ratio, runs]


def _note(key, ratio, twin):
    w = WORST.setdefault(key, [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], ratio), max(w[1], twin), w[2] + 1


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        ratio, twin, n = WORST[k]
        print(f"[infer-walk worst] {k[1]:<7s} {k[2]:<6s} {ratio:.3e} twin {twin:.3e} slabs {n:<4d} {k[0]}")


@pytest.fixture(scope="module")
def world():
    """The models and inputs on the device (one per model, kind and batch) and the references per (model, kind, call, block, offset,
    arithmetic), computed once."""
    from bbb_hip import rng
    models, refs = {}, {}

    def model(run):
        key = (run["source"], run["model"], run["kind"], run["B"])
        if key not in models:
            if run["source"] == "recorded":
                models[key] = R._inputs(run)                 # (the recorder's own model and input)
            else:
                net = C.build(run["model"], run["kind"]).cuda()
                rng.assign_stream_ids(net)
                models[key] = (net, C.table_x(run["model"], run["B"]).cuda())
        return models[key]

    def ref(run, slab, mode):
        key = (run["source"], run["model"], run["kind"], run["B"]) + tuple(slab) + (mode,)
        if key not in refs:
            net, x = model(run)
            i0, i1, call, boff = slab
            kw = dict(dtype=torch.float32) if mode == "twin" else dict(rounding="bf16") if mode == "bf16" else {}
            refs[key] = IR.forward64(net, x[i0:i1].cpu(), C.SEED, call, b_offset=boff, **kw).double()
        return refs[key]
    return model, ref


def _ratio(got, want):
    return float((got - want).abs().max()) / float(want.abs().max())


@pytest.mark.parametrize("rid", list(RUNS))
def test_walk_against_float64(rid, world):
    from bbb_hip import ensemble, ops, _lib
    run, (model, ref) = RUNS[rid], world
    net, x = model(run)
    precision, draws, kw = run["precision"], run["draws"], run["kw"]
    expected = C.expected_plans()[rid]
    with torch.no_grad(), ops.use_config(**run["cfg"]):
        assert C.plan_of(run, net) == expected, rid
        if run.get("refusal"):
            who, message = run["refusal"]
            if who == "mc_logits":                           # no plan: the walk returns None before any launch, its caller refuses
                assert expected is None
                assert ensemble._mc_logits_chwn(net, x, draws, C.SEED, C.CALL0, precision=precision, **kw) is None
            with pytest.raises(_lib.BBBHipError, match=re.escape(message)):
                if who == "mc_logits":
                    ensemble.mc_logits(net, x, draws, C.SEED, C.CALL0, precision=precision)
                else:
                    ensemble._mc_logits_chwn(net, x, draws, C.SEED, C.CALL0, precision=precision, **kw)
            return
        if expected is None:                                 # the forward does not apply: its caller falls back
            assert ensemble._mc_logits_chwn(net, x, draws, C.SEED, C.CALL0, precision=precision, **kw) is None
            logits, kl = ensemble.mc_logits(net, x, draws, C.SEED, C.CALL0, precision=precision)
            assert ensemble.stats["path"] == "nchw"
        else:
            out, kl = ensemble._mc_logits_chwn(net, x, draws, C.SEED, C.CALL0, precision=precision, **kw)
            assert ensemble.stats["path"] == ("chwn-bf16-lrt" if precision == "bf16" and C.has_lrt(run) else "chwn")
            logits = out.permute(0, 2, 1)                    # [slabs, rows, classes]
        torch.cuda.synchronize()
    logits, kl = logits.double().cpu(), float(kl)
    slabs = IR.slab_sources(tuple(x.shape), draws, C.CALL0, **{k: v for k, v in kw.items() if k != "streams"})
    assert logits.shape[0] == len(slabs)
    forms = "+".join(sorted({s[0] for s in expected})) if expected else "nchw"
    floor = C.FLOOR_LRT if C.has_lrt(run) else C.FLOOR_BBB
    fails, wants = [], []
    for e, slab in enumerate(slabs):
        want = ref(run, slab, "bf16" if precision == "bf16" else "f64")
        wants.append(want)
        assert logits[e].shape == want.shape, (rid, e, logits[e].shape, want.shape)
        ratio = _ratio(logits[e], want)
        if precision == "bf16":
            twin, bound = 0.0, C.BOUND_BF16
        else:
            twin = _ratio(ref(run, slab, "twin"), want)
            bound = min(C.CAP, max(C.TWIN_FACTOR * twin, floor))
        print(f"[infer-walk] {rid} slab {e}: ratio {ratio:.3e} twin {twin:.3e} bound {bound:.3e}")
        _note((forms, precision, run["kind"]), ratio, twin)
        if not ratio <= bound:
            fails.append((e, slab, ratio, twin, bound))
    # (the slabs of THIS model, as built on this machine, are as far apart as the CPU tests ask of the cases)
    for a in range(len(wants)):
        for b in range(a + 1, len(wants)):
            if wants[a].shape == wants[b].shape:
                assert _ratio(wants[a], wants[b]) >= C.separation(run), (rid, a, b)
    assert not fails, (rid, fails)
    if not any(k in kw for k in ("units", "groups", "share")):
        kl64 = IR.kl64(net)
        assert abs(kl - kl64) <= C.KL_RTOL * kl64, (rid, kl, kl64)
