"""bf16 training behind strided layers (LaunchConfig.bf16_strided_train): the transposed form of the general bf16 GEMM
(bbb_conv2d_chwn_bf16_dgrad, csrc/pconv_bf16.hip TR) on the MI355X, with the tiers, helpers and bounds of
test_gpu_bf16_train_fuzz.py and the geometries of test_gpu_strided_dgrad.py:

  * kernel sweep: ops.conv2d_chwn_input_grad_bf16(stride=...) against float64 torch.nn.grad.conv2d_input on the SAME bf16 operands
    -- test_gpu_strided_dgrad.DGRAD_CASES with B taken up to a multiple of 8 (strides, kernels, paddings, dilations, gcd(s, d) > 1,
    pixels no tap reaches, floor-dropped rows; per-draw and shared weights; w_flipped passed in and not), plus the smallest shapes
    that reach every form the launcher can select (ops.bf16_dgrad_form says which), both row orders, and an empty contraction
    (K = 0) under the plain, k-group and wave-specialised families.  Pixels no tap reaches must hold the bits of +0;
  * bitwise invariants: two identical calls, w_flipped passed in against computed inside, stride=(1, 1) through the new keyword
    against the call without it;
  * generated BBB models with a stride-2 / stride-3 convolution as layer 2 or 3 under the switch: every parameter gradient of
    train.forward_loss(precision="bf16") against the float64 contract (tests/bf16_train_contract.py) fed the device's Philox
    noise, and against the fp32 path by cosine; graph replay, train_step's self-capture, the value-neutral switches, and what
    the switch still refuses.

EXACT tier: integers in [-3, 3], the result must equal the float64 value rounded once, bit for bit.  GAUSSIAN tier: |err| <=
c(K) * sum |g||w| + half a bf16 ulp, c = 2e-5 * max(1, sqrt(K / 4096)).  No element and no case is excluded.  Run with -m gpu.

Worst err / bound observed on an MI355X (exact tier: bit for bit everywhere): see profiles/bf16_strided_train_notes.md."""
import numpy as np
import pytest
import torch

import bbb_numpy as O
import bf16_train_contract as C
import test_gpu_bf16_train_fuzz as FZ
import test_gpu_strided_dgrad as SD
from test_gpu_bf16_train_fuzz import C_GAUSS, _L, _bf, _check_bf16, _data, _m, _pack_w
from test_gpu_strided_dgrad import _dgrad_ref, _out_hw

pytestmark = pytest.mark.gpu

assert C_GAUSS == 2e-5
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(FZ.WORST):
        if k[0].startswith("strided"):
            print(f"[bf16-strided-train worst, err / bound] {k[0]:<34s} {k[1]:<8s} {FZ.WORST[k]:.3e}")
    for k in sorted(WORST):
        print(f"[bf16-strided-train worst, err / bound] {k[0]:<34s} {k[1]:<8s} {WORST[k]:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# the fixed case list (pure: tests/test_bf16_strided_train_cpu.py checks what it reaches without a GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _dg(B, E, Cin, Cout, H, W, kh, kw, s, p=(0, 0), d=(1, 1), form="perdraw", flip=False):
    return dict(B=B, E=E, Cin=Cin, Cout=Cout, H=H, W=W, kh=kh, kw=kw, s=tuple(s), p=tuple(p), d=tuple(d), form=form, flip=flip)


def _from_fp32_case(c):
    """A case of test_gpu_strided_dgrad: B up to a multiple of 8; the LRT pair form runs as per-draw weights."""
    c = dict(c)
    c["B"] = (c["B"] + 7) & ~7
    if c["form"] == "pair":
        c["form"] = "perdraw"
    return c


CASES = {n: _from_fp32_case(c) for n, c in SD.DGRAD_CASES.items()}
CASES.update({
    # the smallest shapes that reach each form (dx channels = Cin; ops.bf16_dgrad_form confirms each in the CPU file)
    "form_ws_128x128": _dg(128, 1, 128, 16, 6, 5, 3, 3, (2, 2), (1, 1)),                  # 30 items: wave-specialised
    "form_ws_k0": _dg(128, 1, 128, 8, 11, 14, 2, 2, (4, 4), (1, 0), flip=True),          # ... with pixels no tap reaches
    "form_ws_refrows": _dg(128, 2, 128, 12, 7, 6, 3, 3, (2, 2), (1, 1)),                  # ... on reference-order rows
    "form_22_plain": _dg(128, 3, 128, 8, 19, 18, 3, 3, (2, 2), (1, 1), flip=True),       # 1026 items: 128 x 128, not specialised
    "form_14_kg1": _dg(256, 1, 64, 8, 5, 4, 3, 3, (2, 2), (1, 1)),
    "form_14_kg2": _dg(256, 1, 64, 128, 5, 4, 3, 3, (2, 2), (1, 1), flip=True),          # 8 k tiles of the 4 taps a pixel can have
    "form_12_kg1": _dg(128, 2, 64, 8, 7, 5, 3, 3, (2, 2), (1, 1), form="shared"),
    "form_12_kg2": _dg(128, 1, 64, 128, 6, 5, 3, 3, (2, 2), (1, 1)),
    "form_12_kg2_k0": _dg(128, 1, 64, 512, 6, 7, 2, 2, (4, 4), flip=True),                # k-groups with an empty contraction
    "form_12_kg2_refrows": _dg(128, 1, 64, 60, 5, 4, 3, 3, (2, 2), (1, 1)),               # K = 540 over the full row: 9 k tiles
    "form_12_ragged": _dg(136, 2, 70, 16, 7, 6, 3, 3, (3, 2), (1, 1), flip=True),         # ragged image and channel tiles
    "form_14_ragged_k0": _dg(264, 1, 40, 8, 9, 6, 3, 2, (4, 3), (0, 0)),
    "lenet_like_cout6": _dg(16, 3, 6, 6, 14, 12, 5, 5, (2, 2), (2, 2)),                  # Cout % 8 != 0: reference-order rows
})


def case_tags(c):
    """What a case reaches: the launch form (ops.bf16_dgrad_form) and the geometry properties the sweep claims."""
    import math
    from bbb_hip import ops
    shape, kgs, ws, tm = ops.bf16_dgrad_form(c["B"], c["Cin"], c["Cout"], c["kh"], c["kw"], (c["H"], c["W"]), c["s"], c["d"], c["E"])
    fam = "ws" if ws else ("kg>1" if kgs > 1 else "plain")
    tags = {f"shape{shape}-{'ws' if ws else 'kg%d' % kgs}", "tap-major" if tm else "ref-order", fam}
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    rows = [bool(ops.dgrad_tap_plan(ih, ho, c["kh"], c["s"][0], c["p"][0], c["d"][0])) for ih in range(c["H"])]
    cols = [bool(ops.dgrad_tap_plan(iw, wo, c["kw"], c["s"][1], c["p"][1], c["d"][1])) for iw in range(c["W"])]
    if not (all(rows) and all(cols)):
        tags.add("holes")
        if tm:
            tags.add(f"k0-{fam}")                         # tap-major rows: such a pixel's contraction is EMPTY (niter == 0)
    if any(math.gcd(c["s"][i], c["d"][i]) > 1 and c["d"][i] > 1 for i in (0, 1)):
        tags.add("gcd>1")
    if (c["H"] + 2 * c["p"][0] - c["d"][0] * (c["kh"] - 1) - 1) % c["s"][0] or (c["W"] + 2 * c["p"][1] - c["d"][1] * (c["kw"] - 1) - 1) % c["s"][1]:
        tags.add("floor")
    if c["B"] % 128:
        tags.add("ragged-batch")
    if c["Cin"] % (128 if shape == 22 else 64):
        tags.add("ragged-channels")
    tags.add(c["form"])
    tags.add("flip" if c["flip"] else "noflip")
    return tags


def _dead_pixels(ops, c):
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    rows = [bool(ops.dgrad_tap_plan(ih, ho, c["kh"], c["s"][0], c["p"][0], c["d"][0])) for ih in range(c["H"])]
    cols = [bool(ops.dgrad_tap_plan(iw, wo, c["kw"], c["s"][1], c["p"][1], c["d"][1])) for iw in range(c["W"])]
    return ~(torch.tensor(rows)[:, None] & torch.tensor(cols)[None, :])


def _operands(name, tier, salt=0):
    from bbb_hip import ops
    c = CASES[name]
    B, E, Cin, Cout, H, W, kh, kw = (c[k] for k in ("B", "E", "Cin", "Cout", "H", "W", "kh", "kw"))
    ho, wo = _out_hw(H, W, kh, kw, c["s"], c["p"], c["d"])
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact") + salt)
    w = _data(gen, tier, (1 if c["form"] == "shared" else E, Cout, Cin, kh, kw), 0.3)
    g = _data(gen, tier, (E, Cout, ho, wo, B))
    wshape = (Cout, Cin, kh, kw)
    rows = _pack_w(w.cuda(), ops.bf16_tap_major(wshape))
    return c, w, g, wshape, rows, _bf(g.cuda())


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the transposed bf16 launch against float64 conv2d_input on the same bf16 operands
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(CASES))
def test_strided_dgrad_bf16_vs_float64(name, tier):
    from bbb_hip import ops
    c, w, g, wshape, rows, gd = _operands(name, tier)
    want = _dgrad_ref(c, g.double(), w.double())
    mag = _dgrad_ref(c, g.double().abs(), w.double().abs()) if tier == "gauss" else None
    wf = ops.flip_transpose_w_bf16(rows, wshape) if c["flip"] else None
    gx = ops.conv2d_chwn_input_grad_bf16(gd, rows, wshape, (c["H"], c["W"]), c["p"], c["d"], w_flipped=wf, stride=c["s"])
    assert gx.shape == (c["E"], c["Cin"], c["H"], c["W"], c["B"]) and gx.dtype == torch.bfloat16
    _check_bf16(f"strided dgrad {c['form']}", tier, gx, want, mag, c["Cout"] * c["kh"] * c["kw"])
    # pixels that no tap reaches hold the bits of +0.0 (-0.0 would compare equal above)
    dead = _dead_pixels(ops, c)
    if dead.any():
        z = gx.cpu()[:, :, dead, :]
        assert (z.view(torch.int16) == 0).all(), name
        FZ._note(("strided dgrad: +0 without a tap", tier), 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bitwise invariants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s2_d2_gcd", "holes_s4_k2", "e10_shared", "form_ws_k0", "form_14_kg2", "form_12_kg2_k0", "form_22_plain",
                                  "lenet_like_cout6"])
def test_strided_dgrad_bf16_is_repeatable_and_takes_flipped_rows(name):
    from bbb_hip import ops
    c, w, g, wshape, rows, gd = _operands(name, "gauss", salt=5)
    hw = (c["H"], c["W"])
    a = ops.conv2d_chwn_input_grad_bf16(gd, rows, wshape, hw, c["p"], c["d"], stride=c["s"])
    b = ops.conv2d_chwn_input_grad_bf16(gd, rows, wshape, hw, c["p"], c["d"], stride=c["s"])
    wf = ops.flip_transpose_w_bf16(rows, wshape)
    f = ops.conv2d_chwn_input_grad_bf16(gd, rows, wshape, hw, c["p"], c["d"], w_flipped=wf, stride=c["s"])
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), name
    assert torch.equal(a.view(torch.int16), f.view(torch.int16)), name


@pytest.mark.parametrize("name", ["q0", "dil", "c64", "tm"])
def test_stride1_keyword_is_the_forward_launch(name):
    """stride 1 through the new keyword (spelled out either way) stays the call without it: the forward on the flipped rows."""
    from bbb_hip import ops
    B, E, Cin, Cout, H, W, kh, kw, p, d = {
        "q0": (8, 2, 8, 12, 9, 5, 3, 3, (2, 2), (1, 1)), "dil": (16, 3, 4, 6, 11, 8, 3, 2, (1, 2), (2, 3)),
        "c64": (64, 2, 64, 70, 6, 4, 5, 5, (2, 2), (1, 1)), "tm": (8, 1, 16, 16, 7, 5, 3, 3, (1, 1), (1, 1))}[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    ho, wo = _out_hw(H, W, kh, kw, (1, 1), p, d)
    g = _bf(_data(gen, "gauss", (E, Cout, ho, wo, B)).cuda())
    wshape = (Cout, Cin, kh, kw)
    rows = _pack_w(_data(gen, "gauss", (E,) + wshape, 0.3).cuda(), ops.bf16_tap_major(wshape))
    wf = ops.flip_transpose_w_bf16(rows, wshape)
    q = (d[0] * (kh - 1) - p[0], d[1] * (kw - 1) - p[1])
    want = ops.conv2d_chwn_bf16_forward(g, wf, None, (Cout, kh, kw), 1, q, d, tap_major=ops.bf16_tap_major((Cin, Cout, kh, kw)))
    for kwargs in ({}, {"stride": 1}, {"stride": (1, 1)}, {"stride": 1, "w_flipped": wf}):
        got = ops.conv2d_chwn_input_grad_bf16(g, rows, wshape, (H, W), p, d, **kwargs)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (name, kwargs)


def test_strided_dgrad_bf16_refuses_what_the_entry_refuses():
    from bbb_hip import ops, _lib
    g = torch.zeros((1, 8, 3, 3, 8), device="cuda", dtype=torch.bfloat16)
    rows = torch.zeros((1, 8, 8), device="cuda", dtype=torch.bfloat16)
    with pytest.raises(_lib.BBBHipError, match="padding larger than the kernel reach"):
        ops.conv2d_chwn_input_grad_bf16(g, rows, (8, 8, 1, 1), (4, 4), (1, 1), (1, 1), stride=2)
    with pytest.raises(_lib.BBBHipError):                      # x_hw that this layer's forward does not map onto g's 3 x 3
        ops.conv2d_chwn_input_grad_bf16(g, rows, (8, 8, 1, 1), (9, 5), (0, 0), (1, 1), stride=2)
    with pytest.raises(_lib.BBBHipError):                      # B % 8
        ops.conv2d_chwn_input_grad_bf16(g[..., :4].contiguous(), rows, (8, 8, 1, 1), (5, 5), (0, 0), (1, 1), stride=2)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. generated models with strided later layers, switch on
# ---------------------------------------------------------------------------------------------------------------------------
MODELS = {
    # 3 x 3 / 2 second layer, ReLU, no pools (reference-order rows: Cout = 12)
    "l2_s2_relu_e3": _m(3, 8, 3, 17, 14, [_L("conv", 8, 3, 1, 1, act="relu"), _L("conv", 12, 3, 2, 1, act="relu"), _L("fc", 10)]),
    # 5 x 5 / 2 + 3 x 3 / 2 with a pool, Softplus (tap-major rows)
    "l2_l3_s2_pool_softplus": _m(1, 16, 3, 21, 18, [_L("conv", 8, 5, 1, 2, act="softplus"),
                                                     _L("conv", 16, 5, 2, 2, act="softplus", pool=(2, 2)),
                                                     _L("conv", 16, 3, 2, 1, act="softplus"), _L("fc", 10)]),
    # 2 x 2 / 3 third layer, no activation anywhere (floor-dropped rows, pixels no tap reaches; first layer on 4 channels)
    "l3_s3_linear_e3": _m(3, 16, 4, 16, 13, [_L("conv", 8, 3, 1, 1), _L("conv", 8, 3, 1, 1), _L("conv", 8, 2, 3), _L("fc", 16),
                                              _L("fc", 10)]),
    # 1 x 1 / 3 "holes" layer
    "l2_1x1_s3_holes": _m(1, 8, 3, 14, 11, [_L("conv", 8, 3, 1, 1, act="softplus"), _L("conv", 16, 1, 3, act="softplus"), _L("fc", 10)]),
    # a (2, 1) stride behind a pooled first layer, dilated, ReLU
    "l2_s21_dil_pool_relu": _m(3, 8, 3, 20, 17, [_L("conv", 8, 3, 1, 1, act="relu", pool=(3, 2)),
                                                  _L("conv", 8, 3, (2, 1), 2, 2, act="relu"), _L("fc", 12, act="relu"), _L("fc", 10)]),
    # 2 x 2 / 4 on tap-major rows: empty contractions inside a model
    "l2_k2_s4_k0": _m(1, 16, 3, 15, 18, [_L("conv", 8, 3, 1, 1, act="softplus"), _L("conv", 8, 2, 4, 1, act="softplus"), _L("fc", 10)]),
}


def _model_setup(name):
    from bbb_hip import fast_train, ops, rng
    spec = MODELS[name]
    net = FZ._build(spec, sum(map(ord, name))).cuda()
    rng.assign_stream_ids(net)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 1)
    x = torch.rand((spec["B"], spec["Cin"], spec["H"], spec["W"]), generator=gen).cuda()
    y = torch.randint(0, 10, (spec["B"],), generator=gen).cuda()
    assert fast_train._strided_later_conv(net)
    why = fast_train.bf16_train_refusal(net, x)
    assert why is not None and "bf16_strided_train" in why                # the default still refuses, and names the switch
    with ops.use_config(bf16_strided_train=True):
        assert fast_train.bf16_train_refusal(net, x) is None
    return spec, net, x, y


def _bf16_grads(spec, net, x, y, seed_call):
    from bbb_hip import ops
    with ops.use_config(bf16_strided_train=True):
        return FZ._grads(net, x, y, spec["E"], seed_call, "bf16")


def test_models_cover_what_they_claim():
    later = [L for s in MODELS.values() for L in s["layers"][1:] if L["kind"] == "conv"]
    assert {C._pair(L["s"]) for L in later} >= {(2, 2), (3, 3), (2, 1)}
    assert all(any(C._pair(L["s"]) != (1, 1) for L in s["layers"][1:3] if L["kind"] == "conv") for s in MODELS.values())
    assert {L["act"] for s in MODELS.values() for L in s["layers"][:-1]} == {None, "relu", "softplus"}
    assert any(L["pool"] for L in later) and any(all(L["pool"] is None for L in s["layers"]) for s in MODELS.values())
    assert {s["E"] for s in MODELS.values()} == {1, 3} and {s["B"] for s in MODELS.values()} == {8, 16}


@pytest.mark.parametrize("name", list(MODELS))
def test_model_gradients_bf16_vs_contract_and_fp32(name):
    spec, net, x, y = _model_setup(name)
    E, seed, call0, beta, n = spec["E"], 4242, 17, 0.1, 5000.0
    got = _bf16_grads(spec, net, x, y, (seed, call0))
    g32 = FZ._grads(net, x, y, E, (seed, call0), "fp32")
    plan = FZ.model_plan(spec)
    mods = dict(net.named_modules())
    npar = {L["name"]: {k: getattr(mods[L["name"]], k).detach().cpu().numpy() for k in ("W_mu", "W_rho", "bias_mu", "bias_rho")}
            for L in plan}
    npar["_prior_mu"], npar["_prior_sigma"] = mods["l0"].prior_mu, mods["l0"].prior_sigma
    eps = [{L["name"]: {kind: O.normal_eps(seed, call0 + e, mods[L["name"]]._stream_base + off,
                                           int(np.prod(npar[L["name"]][key].shape))).reshape(npar[L["name"]][key].shape)
                        for kind, key, off in (("W", "W_mu", 0), ("bias", "bias_mu", 1))} for L in plan} for e in range(E)]
    _, _, want = C.step_grads(plan, npar, x.cpu().numpy(), y.cpu().numpy(), eps, None, beta, n)
    no_ties = FZ._no_ties(spec)
    bound = 1e-2 if no_ties else 4e-2
    fails = []
    for L in plan:
        for key in ("W_mu", "W_rho", "bias_mu", "bias_rho"):
            pn = f"{L['name']}.{key}"
            g = got[pn].double().cpu().numpy()
            w = np.asarray(want[L["name"]][key]).reshape(g.shape)
            rel = float(np.abs(g - w).max()) / float(np.abs(w).max())
            a, b = got[pn].double().flatten(), g32[pn].double().flatten()
            cos = float(a @ b / (a.norm() * b.norm()))
            print(f"{name} {pn}: err / max {rel:.3e} (bound {bound:.0e}), cosine vs fp32 {cos:.6f}")
            _note((f"model {'no-ties' if no_ties else 'pool/relu'} {key}", "contract"), rel / bound)
            _note(("model 1 - cosine vs fp32", "fp32"), (1.0 - cos) / 0.0005)
            if not rel <= bound:
                fails.append((pn, "contract", rel, bound))
            if not cos >= 0.9995:
                fails.append((pn, "cosine", cos, 0.9995))
    assert not fails, fails


SWITCH_MODELS = ["l2_l3_s2_pool_softplus", "l3_s3_linear_e3"]


@pytest.mark.parametrize("name", SWITCH_MODELS)
def test_bf16_switches_are_value_neutral(name):
    from bbb_hip import fast_train
    spec, net, x, y = _model_setup(name)
    ref = _bf16_grads(spec, net, x, y, (7, 3))
    saved = (fast_train.overlap_wgrad[0], fast_train.flips_up_front[0])
    try:
        for ov, fl in ((False, True), (False, False), (True, False)):
            fast_train.overlap_wgrad[0], fast_train.flips_up_front[0] = ov, fl
            got = _bf16_grads(spec, net, x, y, (7, 3))
            for k in ref:
                assert torch.equal(got[k], ref[k]), (k, ov, fl)
    finally:
        fast_train.overlap_wgrad[0], fast_train.flips_up_front[0] = saved
    _note(("switches overlap / flips", "bitwise"), 0.0)


@pytest.mark.parametrize("name", SWITCH_MODELS)
def test_bf16_graph_replay_equals_eager(name):
    """Six eager train_step calls against three warm-up + three replayed GraphedTrainStep steps, bitwise (capturable Adam on both
    sides); the graphed step is handed the switch as launch_config= and replays outside any use_config."""
    from bbb_hip import ops, rng, train
    spec = MODELS[name]
    E, lr, beta, n = spec["E"], 1e-3, 0.1, 1000.0

    def fresh():
        s, net, x, y = _model_setup(name)
        rng.manual_seed(77, call=0)
        return net, x, y

    net_e, x, y = fresh()
    opt_e = train.FusedAdam(net_e.parameters(), lr=lr, capturable=True)
    with ops.use_config(bf16_strided_train=True):
        eager = [train.train_step(net_e, opt_e, x, y, E, beta, n, precision="bf16", graph=False)[0] for _ in range(6)]
    net_g, _, _ = fresh()
    opt_g = train.FusedAdam(net_g.parameters(), lr=lr, capturable=True)
    g = train.GraphedTrainStep(net_g, opt_g, x, y, E, beta, n, warmup=3, precision="bf16",
                               launch_config=ops.current_config().copy(bf16_strided_train=True))
    assert g.launch_config.bf16_strided_train and not ops.current_config().bf16_strided_train
    graphed = [g.step()[0].clone() for _ in range(3)]
    for a, b in zip(eager[3:], graphed):
        assert torch.equal(a, b)
    for (na, a), (_, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(a, b), na
    assert rng.get_state()[1] == 6 * E
    _note(("graph replay vs eager", "bitwise"), 0.0)


def test_train_step_captures_itself_on_a_strided_model():
    """train_step's self-capture under the switch: calls 1-3 launch by launch, call 4 captures, later calls replay; the same
    call outside the switch is refused again (the switch is part of what a captured step bakes in)."""
    from bbb_hip import _lib, ops, rng, train
    name = "l2_l3_s2_pool_softplus"
    spec, net, x, y = _model_setup(name)
    rng.manual_seed(5, call=0)
    opt = train.FusedAdam(net.parameters(), lr=1e-3)
    E = spec["E"]
    losses, captured = [], []
    with ops.use_config(bf16_strided_train=True):
        for _ in range(6):
            losses.append(train.train_step(net, opt, x, y, E, 0.1, 1000.0, precision="bf16")[0].item())
            st = train._auto.get(net)
            captured.append(bool(st and st["graphed"] is not None))
    assert captured == [False] * 3 + [True] * 3
    assert all(np.isfinite(v) for v in losses) and rng.get_state()[1] == 6 * E
    with pytest.raises(_lib.BBBHipError, match="stride-1 convolutions after the first layer"):
        train.train_step(net, opt, x, y, E, 0.1, 1000.0, precision="bf16")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. what the switch does not admit
# ---------------------------------------------------------------------------------------------------------------------------
def test_switch_on_still_refuses_lrt_and_input_gradients():
    from bbb_hip import _lib, fast_train, ops, rng, train
    spec, net, x, y = _model_setup("l2_s2_relu_e3")
    with ops.use_config(bf16_strided_train=True):
        xg = x.clone().requires_grad_(True)
        with pytest.raises(_lib.BBBHipError, match="inputs that do not require a gradient"):
            train.forward_loss(net, xg, y, spec["E"], 0.1, 1000.0, precision="bf16")
        lspec, lnet, lx, ly = SD._setup("lrt_allconv")
        assert fast_train.train_path_ok(lnet, lx) == "lrt"
        with pytest.raises(_lib.BBBHipError, match="local-reparameterisation layers have no bf16 mode"):
            train.forward_loss(lnet, lx, ly, lspec["E"], 0.1, 1000.0, precision="bf16")
        with pytest.raises(_lib.BBBHipError, match="multiple of 8"):
            train.forward_loss(net, x[:4], y[:4], spec["E"], 0.1, 1000.0, precision="bf16")
