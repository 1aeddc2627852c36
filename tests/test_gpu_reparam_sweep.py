"""The fused reparameterisation + KL pass (csrc/reparam_kl.hip), launch form by launch form, against float64: the named cases of
tests/reparam_contract.py.  Each case asserts the form ops.reparam_plan reports for the very Segment array it launches, then its
outputs: the noise entry against the float64 stream, the generic kernel with external noise against float64 rounded once (bit
equality), every other form bit-equal to that launch in the layout its header describes, with sentinels around and between the
draws.  The KL float and double are inside 1e-6 of the float64 sum and bit-equal wherever the same kernel computes them: every generic
launch against the canonical one, every fast launch (offset views, both store flavours, the per-draw split, tap-major blocks, an own
call_dev word) against a plain one-draw fast launch of the same tensors.  Between the fast and the generic kernel they are NOT
bit-equal on hardware (measured: the fp32 sum one ulp apart; the packed and the scalar KL term are contracted differently), so that
pair is held to the float64 bound only.  Needs an MI355X: -m gpu."""
import dataclasses

import numpy as np
import pytest
import torch

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


def _noise(env, case, segs, word=None):
    """Per segment [draws][n]: the case's external noise, or what the noise entry gives for the stream the launch draws from."""
    word = (case.call_dev or 0) if word is None else word
    out = []
    for i, s in enumerate(segs):
        if not s.want_w:
            out.append(np.zeros((case.draws, s.n), F32))
        elif s.ext_eps:
            out.append(C.external_noise(case, i, s.n, case.draws))
        else:
            out.append(torch.stack([env["ops"].eps_dump(s.n, case.seed, case.call0 + word + e, case.stream(i), "cuda")
                                    for e in range(case.draws)]).cpu().numpy())
    return out


def _launch(env, case, segs, inputs, eps):
    """Launch `case` on `segs`; assert the plan of the Segment array it launched."""
    L = C.Launch(segs, case.draws, inputs, [e if s.ext_eps else None for s, e in zip(segs, eps)])
    L.set_streams(case)
    plan = env["ops"].reparam_plan(L.arr, case.draws, nseg=len(segs))
    assert plan == C.plan_rules(_rule_input(segs), case.draws, env["slots"]), (case.name, plan)
    assert L.forward(case, kl=case.kl) == 0
    return L, plan


def _canonical(env, case, segs, inputs, eps):
    """The generic kernel on dense aligned fp32 segments with the same noise, held to float64: -> (launch, samples per segment,
    sigma bits per segment, skipped half-way elements)."""
    ccase = dataclasses.replace(case, call_dev=None, kl="both", flags=case.flags & C.KL_TEXTBOOK)
    csegs = tuple(C.Seg(s.n, ext_eps=True, want_w=s.want_w) for s in segs)
    R = C.Launch(csegs, case.draws, inputs, eps)
    assert env["ops"].reparam_plan(R.arr, case.draws, nseg=len(segs))["kernel"] == "generic"
    assert R.forward(ccase) == 0
    ws, sgs, skipped = [], [], 0
    for i, (s, (mu, rho)) in enumerate(zip(csegs, inputs)):
        sg = R.sigma_bits(i)
        C.check_image(sg, C.sigma_image(s, sg[:s.n]), "canonical sigma %d" % i)
        C.check_sigma(sg[:s.n].view(F32), rho, False)
        w = None
        if s.want_w:
            wb = R.w_bits(i)
            w = wb[:-1].view(F32).reshape(case.draws, s.n)
            assert wb[-1] == C.sentinel_bits(s)
            skipped += C.check_exact(w, mu, sg[:s.n].view(F32), eps[i])
        ws.append(w)
        sgs.append(sg[:s.n])
    want = C.kl_reference(inputs, case.flags)
    C.check_kl(R.kl32.item(), want)
    C.check_kl(R.kl64.item(), want)
    return R, ws, sgs, skipped


def _fast_kl_bits(env, case, segs, inputs):
    """KL bits of the plain fast launch: the same tensors dense and aligned, one draw, nothing sampled."""
    plain = dataclasses.replace(case, draws=1, call_dev=None, kl="both", flags=case.flags & C.KL_TEXTBOOK)
    P = C.Launch(tuple(C.Seg(s.n, want_w=False, want_sigma=False) for s in segs), 1, inputs)
    plan = env["ops"].reparam_plan(P.arr, 1, nseg=len(segs))
    assert plan["kernel"] == "fast" and plan["n_small"] == 0 and plan["tm_blocks"] == 0
    assert P.forward(plain) == 0
    return P.kl_bits()


def _check_against(case, segs, inputs, L, ws, sgs, kl_ref_bits):
    for i, s in enumerate(segs):
        if s.want_w:
            C.check_image(L.w_bits(i), C.w_image(s, case.draws, ws[i]), "%s w %d" % (case.name, i))
        if s.want_sigma:
            sg = sgs[i].view(F32)
            want = (sg * sg).view(np.uint32) if case.flags & C.SIGMA_SQUARED else sgs[i]
            C.check_image(L.sigma_bits(i), C.sigma_image(s, want), "%s sigma %d" % (case.name, i))
    k32, k64 = L.kl_bits()
    r32, r64 = kl_ref_bits
    assert k32 in (None, r32) and k64 in (None, r64), (case.name, (k32, k64), (r32, r64))
    want = C.kl_reference(inputs, case.flags)
    if k32 is not None:
        C.check_kl(L.kl32.item(), want)
    if k64 is not None:
        C.check_kl(L.kl64.item(), want)
    assert (k32 is None) == (case.kl in ("64", "none")) and (k64 is None) == (case.kl in ("32", "none"))


def _run(env, case):
    segs = case.segments(env["slots"])
    inputs = C.case_inputs(case, segs)
    eps = _noise(env, case, segs)
    L, plan = _launch(env, case, segs, inputs, eps)
    for k, v in case.want.items():
        if k != "split":
            assert plan[k] == v, (case.name, k, plan)
    R, ws, sgs, skipped = _canonical(env, case, segs, inputs, eps)
    same_kernel = R.kl_bits() if plan["kernel"] == "generic" else _fast_kl_bits(env, case, segs, inputs)
    _check_against(case, segs, inputs, L, ws, sgs, same_kernel)
    print("REPARAM-SWEEP fwd %s kernel=%s gpt=%d nt=%d chunks=%d n_small=%d tm_blocks=%d skipped=%d" % (
        case.name, plan["kernel"], plan["gpt"], plan["nt"], plan["chunks"], plan["n_small"], plan["tm_blocks"], skipped))
    return segs, inputs, eps, L, R, plan


# ------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("start", [0, 4099, 2 ** 34 - 5, 2 ** 34 + 3])
@pytest.mark.parametrize("call,stream", [(7, 13), (2 ** 32 - 1, 13), (7, 2 ** 32 - 1), (2 ** 32 - 1, 2 ** 32 - 1)])
def test_noise_entry_against_float64(env, start, call, stream):
    """Step one of the chain.  The windows at 2^34 - 5 and 2^34 + 3 straddle / follow the first group whose counter uses its second
    word; stream and call take their largest values."""
    seed, n = 0x1234567890ABCDEF, 2051
    got = env["ops"].eps_dump(n, seed, call, stream, "cuda", start=start).cpu().numpy()
    print("REPARAM-SWEEP noise start=%d call=%d stream=%d err=%.3g" % (start, call, stream, C.check_noise(got, seed, call, stream, n, start)))


# ------------------------------------------------------------------------------------------------ forward
SPLIT = [n for n in C.FWD_CASES if n.startswith("split-")]
TM = [n for n in C.FWD_CASES if n.startswith("tm-")]


@pytest.mark.parametrize("name", [n for n in C.FWD_CASES if n not in SPLIT and n not in TM])
def test_forward_case(env, name):
    case = C.FWD_CASES[name]
    segs, inputs, eps, L, R, plan = _run(env, case)
    if case.call_dev is not None:
        # an own device word: bit-equal to the launch at the summed call number
        summed = dataclasses.replace(case, call0=(case.call0 + case.call_dev) & 0xFFFFFFFF, call_dev=None)
        S, _ = _launch(env, summed, segs, inputs, eps)
        for i, s in enumerate(segs):
            C.check_image(S.w_bits(i), L.w_bits(i), "summed call, w %d" % i)
        assert S.kl_bits() == L.kl_bits()


@pytest.mark.parametrize("name", TM)
def test_forward_tap_major_case(env, name):
    """fp32 tap-major blocks; sigma and KL are those of the dense launch, bit for bit."""
    case = C.FWD_CASES[name]
    segs, inputs, eps, L, R, plan = _run(env, case)
    assert plan["tm_blocks"] > 0
    dense = tuple(C.Seg(s.n) for s in segs)
    D, dplan = _launch(env, case, dense, inputs, eps)
    assert dplan["tm_blocks"] == 0 and D.kl_bits() == L.kl_bits()
    for i in range(len(segs)):
        C.check_image(D.sigma_bits(i), L.sigma_bits(i), "dense sigma %d" % i)


@pytest.mark.parametrize("name", SPLIT)
def test_forward_per_draw_split_case(env, name):
    """slots < chunks <= 3 slots: the last chunks % slots chunks run as one block per draw.  KL bit-equal to a one-draw launch (which is
    never split)."""
    case = C.FWD_CASES[name]
    slots = env["slots"]
    segs, inputs, eps, L, R, plan = _run(env, case)
    excess = {89: 89, -1: slots - 1, 0: 0}[case.want["split"]]
    assert plan["n_small"] == excess * case.draws and plan["small_chunk0"] == plan["chunks"] - excess
    one = dataclasses.replace(case, draws=1)
    O1, p1 = _launch(env, one, tuple(C.Seg(s.n, want_w=False) for s in segs), inputs, eps)
    assert p1["n_small"] == 0 and O1.kl_bits() == L.kl_bits()


def test_forward_gpt4(env):
    """More than 1024 x 16384 elements: four groups per thread.  Bulk: bit-equal to the generic <4> kernel fed the noise entry's output;
    float64: windows of 4096 elements at the start, around element 16 777 216 and at the tail (and the two small segments whole)."""
    case = C.GPT4_CASE
    segs = case.segments()
    inputs = C.case_inputs(case, segs)
    eps = _noise(env, case, segs)
    L, plan = _launch(env, case, segs, inputs, eps)
    assert all(plan[k] == v for k, v in case.want.items()), plan
    csegs = C.canonical(segs)
    R = C.Launch(csegs, 1, inputs, eps)
    rplan = env["ops"].reparam_plan(R.arr, 1, nseg=3)
    assert (rplan["kernel"], rplan["gpt"]) == ("generic", 4)
    assert R.forward(dataclasses.replace(case, kl="both")) == 0
    skipped = 0
    for i, (s, (mu, rho)) in enumerate(zip(segs, inputs)):
        wr, sr = R.w_bits(i), R.sigma_bits(i)
        C.check_image(L.w_bits(i), C.w_image(s, 1, wr[:-1].view(F32)[None]), "gpt4 w %d" % i)
        C.check_image(L.sigma_bits(i), sr, "gpt4 sigma %d" % i)
        for a in (C.GPT4_WINDOWS if i == 0 else (0,)):
            b = min(a + 4096, s.n)
            C.check_sigma(sr[a:b].view(F32), rho[a:b], False)
            skipped += C.check_exact(wr[a:b].view(F32)[None], mu[a:b], sr[a:b].view(F32), eps[i][:, a:b])
    want = C.kl_reference(inputs, 0)                      # (fast <4> and generic <4>: different kernels, the float64 bound only)
    C.check_kl(L.kl32.item(), want)
    C.check_kl(L.kl64.item(), want)
    print("REPARAM-SWEEP fwd gpt4 chunks=%d tm_blocks=%d skipped=%d" % (plan["chunks"], plan["tm_blocks"], skipped))


def test_refusals(env):
    """17 segments, and what the tap-major form does not take, come back with the stated code from the launch entry and the plan
    entry alike, before anything is launched."""
    lib = env["lib"]

    def rc_of(segs, draws=2):
        case = C.Case("refusal", segs, draws)
        inputs = C.case_inputs(case, segs)
        L = C.Launch(segs, draws, inputs, [np.zeros((draws, s.n), F32) if s.ext_eps else None for s in segs])
        rc = L.forward(case)
        out = [None] * 8
        assert lib.lib().bbb_reparam_kl_plan(L.arr, len(segs), draws, 0, *out) == rc
        return rc
    assert rc_of(tuple(C.Seg(8) for _ in range(16))) == 0
    assert rc_of(tuple(C.Seg(8) for _ in range(17))) == C.EINVAL
    assert rc_of((C.tm(4, 8, 9),)) == 0
    assert rc_of((C.tm(4, 8, 1),)) == C.EINVAL
    assert rc_of((C.tm(4, 8, 129),)) == C.EINVAL
    assert rc_of((C.tm(4, 12, 9),)) == C.EINVAL
    assert rc_of((C.tm(4, 8, 9, ext_eps=True),)) == C.EINVAL
    assert rc_of((C.tm(4, 8, 9, off=("w",)),)) == C.EALIGN
    assert rc_of((C.tm(4, 8, 9), C.Seg(10, ext_eps=True))) == C.EINVAL      # a tap-major segment on the generic kernel
    torch.cuda.synchronize()


def test_scratch_is_rearmed_between_launches(env):
    """Three launches back to back on ONE scratch buffer with different chunk counts (large, small, large): each KL bit-equal to the
    same launch on a scratch buffer of its own."""
    sizes = (5000 * 1024 - 1, 10, 4097 * 1024 + 5)
    buf = env["ops"]._partials(torch.device("cuda"), 5000)
    got, alone = [], []
    runs = []
    for k, n in enumerate(sizes):
        case = C.Case("rearm-%d" % k, (C.Seg(n, want_w=False, want_sigma=False),))
        runs.append((case, C.Launch(case.segs, 1, C.case_inputs(case, case.segs))))
    for case, L in runs:                                     # back to back: nothing in between
        assert L.forward(case, parts=buf) == 0
        got.append((L.kl32, L.kl64))
    got = [(int(a.view(torch.int32).item()), int(b.view(torch.int64).item())) for a, b in got]
    for case, L in runs:
        fresh = torch.full((5000,), -1, dtype=torch.int64, device="cuda").view(torch.float64)
        assert L.forward(case, parts=fresh) == 0
        alone.append(L.kl_bits())
        C.check_kl(L.kl64.item(), C.kl_reference(C.case_inputs(case, case.segs), 0))
        assert bool((fresh.view(torch.int64) == -1).all())    # every slot it consumed is armed again
    assert got == alone
    assert bool((buf.view(torch.int64) == -1).all())


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", list(C.BWD_CASES))
def test_backward_case(env, name):
    """Arithmetic tier: external noise, float64 of the header's formulas, |error| <= c 2^-23 M per element.  Philox tier: bit-equal to
    the arithmetic tier fed the noise entry's output for the launch's seed, call (call_dev added) and streams."""
    combo, case = C.BWD_CASES[name]
    segs = case.segments()
    data = C.bwd_inputs(case, segs)
    rc, outs = C.launch_bwd(case, segs, data, [d["eps"] for d in data])
    assert rc == 0
    worst = 0.0
    for s, d, (gm, gr) in zip(segs, data, outs):
        ref = C.bwd_reference(d["mu"], d["rho"], d["gw"] if s.gw else None, d["eps"], d["gs"] if s.gs else None, case.gkl, case.flags)
        worst = max(worst, C.bwd_ratio(C.grads_of(gm, s, "gmu"), C.grads_of(gr, s, "grho"), ref))
    print("REPARAM-SWEEP bwd %s combo=%s ratio=%.3f c=%g" % (name, combo, worst, C.BWD_C[combo]))
    assert C.BWD_C[combo] <= C.BWD_C_MAX and worst <= C.BWD_C[combo]
    rc, philox = C.launch_bwd(case, segs, data, None)
    assert rc == 0
    dump = _noise(env, case, segs)
    rc, fed = C.launch_bwd(case, segs, data, dump)
    assert rc == 0
    for i, (a, b) in enumerate(zip(philox, fed)):
        C.check_image(a[0], b[0], "grad_mu %d" % i)
        C.check_image(a[1], b[1], "grad_rho %d" % i)
