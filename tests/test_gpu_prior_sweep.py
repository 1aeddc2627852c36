"""Per-weight Gaussian priors in the fused reparameterisation + KL pass (bbb_reparam_kl_tp_fwd / _tp_bwd), launch form by launch form:
the cases of tests/prior_contract.py.  Per forward case: the plan of the launched Segment array is the written rule's (the prior
never enters it); w, sigma and every sentinel are BIT-equal to the scalar entry's launch on the same inputs (the prior must not reach
them); the KL float and double are inside c 2^-23 M of float64; a repeated launch gives the same bits; and the KL is bit-equal to
the plainest launch of the same kernel on the same tensors (fast: one draw, dense, nothing sampled; generic: dense with external
noise) -- offset views, both store flavours, the per-draw split, tap-major blocks, bf16 rows and an own call_dev word change nothing.
Needs an MI355X: -m gpu."""
import dataclasses

import numpy as np
import pytest
import torch

import prior_contract as P
import reparam_contract as C

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def env():
    from bbb_hip import ops, _lib
    _lib.lib()
    return {"ops": ops, "lib": _lib, "slots": 8 * torch.cuda.get_device_properties(0).multi_processor_count}


def _rule_input(segs):
    return [(s.n, s.ext_eps, s.kind == "bf16", (s.cin, s.taps) if s.kind == "tm" else None) for s in segs]


def _noise(env, case, segs):
    out = []
    for i, s in enumerate(segs):
        if not s.want_w:
            out.append(np.zeros((case.draws, s.n), F32))
        elif s.ext_eps:
            out.append(C.external_noise(case, i, s.n, case.draws))
        else:
            out.append(torch.stack([env["ops"].eps_dump(s.n, case.seed, case.call0 + (case.call_dev or 0) + e, case.stream(i), "cuda")
                                    for e in range(case.draws)]).cpu().numpy())
    return out


def _new_launch(case, segs, inputs, eps):
    L = C.Launch(segs, case.draws, inputs, [e if s.ext_eps else None for s, e in zip(segs, eps)])
    L.set_streams(case)
    return L


def _same_outputs(A, B, segs, what):
    for i, s in enumerate(segs):
        if s.want_w:
            C.check_image(A.w_bits(i), B.w_bits(i), "%s w %d" % (what, i))
        if s.want_sigma:
            C.check_image(A.sigma_bits(i), B.sigma_bits(i), "%s sigma %d" % (what, i))


def _plain_kl_bits(env, case, segs, inputs, pb, kernel):
    """KL bits of the plainest launch of `kernel` on the same tensors and prior buffers."""
    plain = dataclasses.replace(case, draws=1, call_dev=None, kl="both", flags=case.flags & C.KL_TEXTBOOK)
    if kernel == "fast":
        psegs = tuple(C.Seg(s.n, want_w=False, want_sigma=False) for s in segs)
        Q = C.Launch(psegs, 1, inputs)
    else:
        psegs = tuple(C.Seg(s.n, ext_eps=True, want_sigma=False) for s in segs)
        Q = C.Launch(psegs, 1, inputs, [np.zeros((1, s.n), F32) for s in segs])
    plan = env["ops"].reparam_plan(Q.arr, 1, nseg=len(segs), priors=pb.arr)
    assert plan["kernel"] == kernel and plan["n_small"] == 0 and plan["tm_blocks"] == 0
    assert P.forward_tp(Q, plain, pb.arr) == 0
    return Q.kl_bits()


RATIOS = {}


@pytest.mark.parametrize("name", list(P.FWD_CASES))
def test_forward_case(env, name):
    case, _, regime = P.FWD_CASES[name]
    segs = case.segments(env["slots"])
    kinds = P.kinds_of(P.FWD_CASES[name], len(segs))
    assert len(kinds) == len(segs)
    inputs = C.case_inputs(case, segs)
    pri = P.prior_inputs(name, regime, inputs)
    eps = _noise(env, case, segs)
    pb = P.PriorBuffers(kinds, pri)
    S = _new_launch(case, segs, inputs, eps)
    T = _new_launch(case, segs, inputs, eps)
    plan = env["ops"].reparam_plan(T.arr, case.draws, nseg=len(segs), priors=pb.arr)
    assert plan == C.plan_rules(_rule_input(segs), case.draws, env["slots"]), (name, plan)
    assert plan == env["ops"].reparam_plan(S.arr, case.draws, nseg=len(segs))
    assert S.forward(case, kl=case.kl) == 0
    assert P.forward_tp(T, case, pb.arr, kl=case.kl) == 0
    _same_outputs(T, S, segs, name)
    k32, k64 = T.kl_bits()
    assert (k32 is None) == (case.kl in ("64", "none")) and (k64 is None) == (case.kl in ("32", "none"))
    eff = [P.effective(k, p, s.n) for k, p, s in zip(kinds, pri, segs)]
    ref = P.kl_reference_tp(inputs, eff, case.flags)
    c = P.FWD_C[plan["kernel"]]
    assert c <= P.FWD_C_MAX
    ratios = [P.kl_ratio(t.item(), ref) for t in (T.kl32, T.kl64) if t is not None]
    same_as_scalar = None
    if regime == "const" and case.kl != "none":
        same_as_scalar = T.kl_bits() == S.kl_bits()              # recorded, not asserted (the textbook form divides differently)
    print("PRIOR-SWEEP fwd %s kernel=%s regime=%s kl=%r ref=%.9g M=%.6g ratios=%s c=%g const_bits_equal_scalar=%s" % (
        name, plan["kernel"], regime, None if T.kl32 is None else T.kl32.item(), ref[0], ref[1],
        ["%.3f" % r for r in ratios], c, same_as_scalar))
    RATIOS.setdefault(plan["kernel"], []).extend(ratios)
    for t in (T.kl32, T.kl64):
        if t is not None:
            P.check_kl_tp(t.item(), ref, c)
    if case.kl == "none":
        return
    first = T.kl_bits()
    assert P.forward_tp(T, case, pb.arr, kl=case.kl) == 0          # again: the same bits, and the slots were re-armed
    assert T.kl_bits() == first
    _same_outputs(T, S, segs, name + " (repeat)")
    plain = _plain_kl_bits(env, case, segs, inputs, pb, plan["kernel"])
    assert first[0] in (None, plain[0]) and first[1] in (None, plain[1]), (name, first, plain)


@pytest.mark.parametrize("name", ["tp-fast16", "tp-flag-generic-squared", "tp-tm-mixed", "tp-bf16-r3x33-philox", "tp-flag-fast-textbook"])
def test_no_prior_pointer_is_the_scalar_launch(env, name):
    """pri == NULL and a PriorSegment array with every pointer NULL: the scalar entry's bits, KL included."""
    case = P.FWD_CASES[name][0]
    segs = case.segments(env["slots"])
    inputs = C.case_inputs(case, segs)
    eps = _noise(env, case, segs)
    S = _new_launch(case, segs, inputs, eps)
    assert S.forward(case) == 0
    for arr in (None, (env["lib"].PriorSegment * len(segs))()):
        T = _new_launch(case, segs, inputs, eps)
        assert P.forward_tp(T, case, arr) == 0
        _same_outputs(T, S, segs, name)
        assert T.kl_bits() == S.kl_bits()


def test_forward_gpt4(env):
    """More than 1024 x 16384 elements: four groups per thread, the prior loaded beside each group's term.  Outputs bit-equal to the
    scalar launch; float64 windows (C.GPT4_WINDOWS) hold the per-window KL of a one-segment launch on the window's elements."""
    case = C.GPT4_CASE
    segs = case.segments()
    inputs = C.case_inputs(case, segs)
    pri = P.prior_inputs("tp-gpt4", "random", inputs)
    pb = P.PriorBuffers(P.GPT4_KINDS, pri)
    S = C.Launch(segs, 1, inputs)
    T = C.Launch(segs, 1, inputs)
    S.set_streams(case)
    T.set_streams(case)
    plan = env["ops"].reparam_plan(T.arr, 1, nseg=3, priors=pb.arr)
    assert all(plan[k] == v for k, v in case.want.items()), plan
    assert S.forward(case) == 0 and P.forward_tp(T, case, pb.arr) == 0
    for i, s in enumerate(segs):
        assert torch.equal(T.w[i].view(torch.int32), S.w[i].view(torch.int32)), "gpt4 w %d" % i
        assert torch.equal(T.sigma[i].view(torch.int32), S.sigma[i].view(torch.int32)), "gpt4 sigma %d" % i
    eff = [P.effective(k, p, s.n) for k, p, s in zip(P.GPT4_KINDS, pri, segs)]
    ref = P.kl_reference_tp(inputs, eff, 0)
    r = [P.check_kl_tp(t.item(), ref, P.FWD_C["fast"]) for t in (T.kl32, T.kl64)]
    print("PRIOR-SWEEP fwd gpt4 ratios=%s" % r)
    RATIOS.setdefault("fast", []).extend(r)
    # the windows of the first segment, each as a launch of its own (gpt 1) against float64: the prior index of group `it` of a
    # four-group thread is the element's own
    (mu, rho), (mu0, s0) = inputs[0], eff[0]
    for a in C.GPT4_WINDOWS:
        b = min(a + 4096, segs[0].n)
        wc = C.Case("gpt4-window-%d" % a, (C.Seg(b - a, want_w=False, want_sigma=False),))
        wi = [(mu[a:b], rho[a:b])]
        wp = P.PriorBuffers(("tt",), [(mu0[a:b], s0[a:b])])
        W = C.Launch(wc.segs, 1, wi)
        assert P.forward_tp(W, wc, wp.arr) == 0
        P.check_kl_tp(W.kl64.item(), P.kl_reference_tp(wi, [(mu0[a:b], s0[a:b])], 0), P.FWD_C["fast"])


@pytest.mark.parametrize("bad", [float("nan"), 0.0, -0.25])
@pytest.mark.parametrize("name", ["tp-fast16", "tp-flag-generic-squared"])
def test_bad_sigma0_element_gives_a_non_finite_kl_and_nothing_else(env, name, bad):
    """Tensor elements are not checked in the launch: a NaN or non-positive sigma0 follows IEEE into the sum."""
    case, kinds, regime = P.FWD_CASES[name]
    segs = case.segments(env["slots"])
    inputs = C.case_inputs(case, segs)
    pri = [(m.copy(), s.copy()) for m, s in P.prior_inputs(name, regime, inputs)]
    k = max(i for i, kd in enumerate(kinds) if kd in ("tt", "-t", "off"))
    pri[k][1][segs[k].n // 2] = bad
    eps = _noise(env, case, segs)
    pb = P.PriorBuffers(kinds, pri)
    S = _new_launch(case, segs, inputs, eps)
    T = _new_launch(case, segs, inputs, eps)
    assert S.forward(case) == 0 and P.forward_tp(T, case, pb.arr) == 0
    _same_outputs(T, S, segs, name)
    assert not np.isfinite(T.kl32.item()) and not np.isfinite(T.kl64.item()), (T.kl32.item(), T.kl64.item())


def test_refusals(env):
    """A prior pointer that is not 4-byte aligned: BBB_EALIGN from the launch and the plan entry alike; the scalar entry's own refusals
    come first."""
    lib = env["lib"]
    case = C.Case("tp-refusal", (C.Seg(8), C.Seg(10)), 2)
    inputs = C.case_inputs(case, case.segs)
    pb = P.PriorBuffers(("tt", "tt"), P.prior_inputs("tp-refusal", "random", inputs))
    out = [None] * 8

    L = C.Launch(case.segs, 2, inputs)
    plan_rc = lambda: lib.lib().bbb_reparam_kl_tp_plan(L.arr, pb.arr, 2, 2, 0, *out)
    assert plan_rc() == 0 and P.forward_tp(L, case, pb.arr) == 0
    pb.arr[1].sigma0 += 2
    assert plan_rc() == C.EALIGN and P.forward_tp(L, case, pb.arr) == C.EALIGN
    pb.arr[1].sigma0 -= 2
    assert lib.lib().bbb_reparam_kl_tp_plan(L.arr, pb.arr, 0, 2, 0, *out) == C.EINVAL
    assert lib.lib().bbb_reparam_kl_tp_plan(L.arr, pb.arr, 17, 2, 0, *out) == C.EINVAL
    assert P.forward_tp(L, case, pb.arr, prior=(0.0, 0.0)) == C.EINVAL       # the scalar fallback is checked even when unused
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", list(P.BWD_CASES))
def test_backward_case(env, name):
    """External noise against float64 of the header's formulas with per-element priors, |error| <= c 2^-23 M per element; the Philox
    launch bit-equal to the external-noise launch fed the noise entry's output."""
    combo, case, kinds, regime = P.BWD_CASES[name]
    segs = case.segments()
    kinds = kinds[:len(segs)]
    data = C.bwd_inputs(case, segs)
    pri = P.prior_inputs(name, regime, [(d["mu"], d["rho"]) for d in data])
    pb = P.PriorBuffers(kinds, pri)
    rc, outs = P.launch_bwd_tp(case, segs, data, [d["eps"] for d in data], pb.arr)
    assert rc == 0
    worst = 0.0
    for s, d, k, p, (gm, gr) in zip(segs, data, kinds, pri, outs):
        mu0, s0 = P.effective(k, p, s.n)
        ref = P.bwd_reference_tp(d["mu"], d["rho"], d["gw"] if s.gw else None, d["eps"], d["gs"] if s.gs else None, case.gkl, case.flags,
                                 mu0, s0)
        worst = max(worst, C.bwd_ratio(C.grads_of(gm, s, "gmu"), C.grads_of(gr, s, "grho"), ref))
    print("PRIOR-SWEEP bwd %s combo=%s regime=%s ratio=%.3f c=%g" % (name, combo, regime, worst, P.BWD_C[combo]))
    assert P.BWD_C[combo] <= C.BWD_C_MAX and worst <= P.BWD_C[combo]
    rc, philox = P.launch_bwd_tp(case, segs, data, None, pb.arr)
    assert rc == 0
    rc, fed = P.launch_bwd_tp(case, segs, data, _noise(env, case, segs), pb.arr)
    assert rc == 0
    for i, (a, b) in enumerate(zip(philox, fed)):
        C.check_image(a[0], b[0], "grad_mu %d" % i)
        C.check_image(a[1], b[1], "grad_rho %d" % i)
    # no pointer set: the scalar entry's bits
    rc, none = P.launch_bwd_tp(case, segs, data, [d["eps"] for d in data], None)
    rc2, scalar = C.launch_bwd(case, segs, data, [d["eps"] for d in data])
    assert rc == 0 and rc2 == 0
    for i, (a, b) in enumerate(zip(none, scalar)):
        C.check_image(a[0], b[0], "scalar grad_mu %d" % i)
        C.check_image(a[1], b[1], "scalar grad_rho %d" % i)


def test_measured_ratios_are_reported(env):
    """Runs last in the file: the worst forward ratio per kernel of this session, for profiles/tensor_prior_notes.md."""
    for k, v in RATIOS.items():
        print("PRIOR-SWEEP worst forward ratio %s = %.3f over %d values (c = %g)" % (k, max(v), len(v), P.FWD_C[k]))
