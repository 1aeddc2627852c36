"""Average pooling in the bf16 storage mode (csrc/pool2d_bf16.hip, LaunchConfig.bf16_avgpool) against float64 references on the
CPU, on the nine geometries of test_gpu_avgpool.CASES with batches of 8, 16 or 24 images (one, two, three 16-byte groups per row):

  A. the forward kernel: bit for bit on integer inputs (the fp32 sum of integers in [-64, 64] is exact, ONE IEEE division of it is
     the correctly rounded fp32 quotient, and rounding that to bf16 equals rounding the float64 quotient: a tie of the double
     rounding is 2^-15 away at this range); Gaussian inputs within half a bf16 ulp plus the fp32 sum's own error,
     e32 = (n + 1) * 2^-24 * avgpool(|x|), n the window's tap count; a plane alone equals the plane inside the full launch;
  B. the backward of [activation -> pool] against float64 autograd of the pool times act'(y): within half a bf16 ulp plus
     e32 = (m + 2) * 2^-24 * |act'| * sum |g_out / div| over the m windows that cover the element (m divisions, m adds, the product
     and the fp32 act'); bit for bit where the divisor is a power of two; the fp32 output form at a padded pitch; zeros where no
     window covers an element;
  C. two generated BBB models against the contract helper (bf16_avgpool_contract): inference logits, training gradients, graphs and
     captures; the all-LRT twin of the first in inference; the refusals of the default configuration.
Run with -m gpu."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bbb_numpy as O
import bf16_avgpool_contract as A
import bf16_lrt_contract as L
import ref_port_torch as P
from bf16_train_contract import _act_grad
from test_gpu_avgpool import CASES as F32_CASES, _ref_pool, _route, _spec
from test_gpu_bf16_train import _half_ulp

pytestmark = pytest.mark.gpu

CASES = {n: dict(c, B=(8, 16, 24)[i % 3]) for i, (n, c) in enumerate(F32_CASES.items())}
POW2 = ("1_plain_floor_row", "7_gaps", "9_padded_pitch", "8_adaptive_3x2")      # 2 x 2 and 4 x 4 windows, count_include_pad
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"[bf16 avgpool worst] {k:<44s} {WORST[k]:.3e}")


def _shape(c):
    return (c["E"], c["C"], c["H"], c["W"], c["B"])


def test_cases_are_the_fp32_geometries_at_three_group_counts():
    assert len(CASES) == 9 and sorted({c["B"] for c in CASES.values()}) == [8, 16, 24]
    assert all(c["E"] * c["C"] <= 12 for c in CASES.values())
    for n in POW2:
        spec, _ = _spec(CASES[n])
        assert spec[0] in ((2, 2), (4, 4)) and spec[3] is True


# ---------------------------------------------------------------------------------------------------------------------------
# A. forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_vs_float64(name, tier):
    from bbb_hip import ops
    c = CASES[name]
    spec, _ = _spec(c)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    if tier == "exact":
        x = torch.randint(-64, 65, _shape(c), generator=gen).float().bfloat16()
    else:
        x = (3.0 * torch.randn(_shape(c), generator=gen)).bfloat16()
    want64 = _ref_pool(x.double(), c, spec)
    got = ops.avgpool_chwn_bf16(x.cuda(), *spec)
    assert got.dtype == torch.bfloat16 and got.shape == want64.shape
    ho, wo, _, _ = ops.avgpool_bf16_plan(c["H"], c["W"], c["B"], *spec)
    assert tuple(got.shape[2:4]) == (ho, wo)
    if tier == "exact":
        want = want64.float().bfloat16()
        bad = got.cpu() != want
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result"
        return
    n = spec[0][0] * spec[0][1]
    e32 = (n + 1) * 2.0 ** -24 * _ref_pool(x.double().abs(), c, spec)
    bound = _half_ulp(want64.abs() + e32) * (1 + 1e-6) + e32
    err = (got.cpu().double() - want64).abs()
    ratio = float((err / (bound + 1e-300)).max())
    _note("forward err / bound (gauss)", ratio)
    print(f"[bf16 avgpool] forward {name}: worst err / bound {ratio:.4f}")
    assert bool((err <= bound).all()), f"{name}: err / bound {ratio:.4f} > 1"


def test_forward_does_not_depend_on_the_launch_size():
    """A plane computed alone, or a draw alone, equals the same plane inside the full launch, bit for bit."""
    from bbb_hip import ops
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((10, 5, 9, 7, 24), generator=gen).bfloat16().cuda()
    for spec in (((3, 3), (2, 2), (1, 1), False), ((9, 7), (9, 7), (0, 0), True)):
        full = ops.avgpool_chwn_bf16(x, *spec)
        for j in (0, 3, 9):
            assert torch.equal(ops.avgpool_chwn_bf16(x[j:j + 1].contiguous(), *spec)[0], full[j])
            assert torch.equal(ops.avgpool_chwn_bf16(x[j, 2:3].contiguous(), *spec)[0], full[j, 2])


# ---------------------------------------------------------------------------------------------------------------------------
# B. backward
# ---------------------------------------------------------------------------------------------------------------------------
def _cover_count(c, spec):
    """How many windows cover each element of a plane [H, W]: the backward of sum pooling (divisor 1) on ones."""
    t = torch.zeros((1, 1, c["H"], c["W"]), dtype=torch.float64).requires_grad_(True)
    out = F.avg_pool2d(t, spec[0], spec[1], spec[2], ceil_mode=False, count_include_pad=True, divisor_override=1)
    out.backward(torch.ones_like(out))
    return t.grad[0, 0].round()


def _bwd_inputs(c, spec, act, tier, g_f32, gen):
    from bbb_hip import ops
    E, C, H, W, B = _shape(c)
    Ho, Wo, _, _ = ops.avgpool_bf16_plan(H, W, B, *spec)
    v = torch.randn((E, C, H, W, B), generator=gen)
    y = {"none": v, "relu": F.relu(v), "softplus": F.softplus(v)}[act]
    y = ((y * 4).round() / 4).bfloat16()                                   # coarse values, as the max-pool test draws them
    if tier == "exact":
        g = torch.randint(-3, 4, (E, C, Ho, Wo, B), generator=gen).float()
    else:
        g = torch.randn((E, C, Ho, Wo, B), generator=gen)
    g = g if g_f32 else g.bfloat16()
    return y, g


def _dact(y64, act):
    return torch.ones_like(y64) if act == "none" else _act_grad(y64, act)


BWD_RUNS = [(n, a, "gauss", gf) for n in CASES for a in ("none", "relu", "softplus") for gf in (False, True)] + \
           [(n, a, "exact", gf) for n in POW2 for a in ("none", "relu") for gf in (False, True)]


@pytest.mark.parametrize("name,act,tier,g_f32", BWD_RUNS, ids=[f"{n}-{a}-{t}-{'gf32' if gf else 'gbf16'}" for n, a, t, gf in BWD_RUNS])
def test_act_backward_vs_float64(name, act, tier, g_f32):
    from bbb_hip import ops
    c = CASES[name]
    spec, _ = _spec(c)
    gen = torch.Generator().manual_seed(sum(map(ord, name + act)) * 4 + 2 * (tier == "exact") + g_f32)
    y, g = _bwd_inputs(c, spec, act, tier, g_f32, gen)
    a = None if act == "none" else act
    y64, g64 = y.double(), g.double()
    da = _dact(y64, act)
    want = _route(g64, y, c, spec) * da
    got = ops.avgpool_act_backward_chwn_bf16(g.cuda(), y.cuda(), *spec, a)
    assert got.dtype == torch.bfloat16 and got.shape == y.shape
    count = _cover_count(c, spec)                                          # [H, W]
    if tier == "exact":
        bad = got.cpu() != want.float().bfloat16()
        assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ from the exact result"
    else:
        m = count[None, None, :, :, None]
        e32 = (m + 2) * 2.0 ** -24 * da.abs() * _route(g64.abs(), y, c, spec)
        bound = _half_ulp(want.abs() + e32) * (1 + 1e-6) + e32
        err = (got.cpu().double() - want).abs()
        ratio = float((err / (bound + 1e-300)).max())
        _note(f"backward err / bound ({act})", ratio)
        assert bool((err <= bound).all()), f"err / bound {ratio:.4f} > 1"
    # elements no window covers (the gaps of k < s; rows and columns floor mode drops) receive exactly 0
    uncovered = (count == 0)[None, None, :, :, None].expand_as(want)
    if name in ("7_gaps", "1_plain_floor_row"):
        assert bool(uncovered.any())
    assert bool((got.cpu().float()[uncovered] == 0).all())
    # the fp32 output form holds the values of the bf16 one, at the padded pitch when asked
    f = ops.avgpool_act_backward_chwn_bf16(g.cuda(), y.cuda(), *spec, a, out_f32=True, pad_planes=True)
    assert f.dtype == torch.float32 and torch.equal(f, got.float())


@pytest.mark.parametrize("g_f32", [False, True])
def test_out_f32_at_a_padded_pitch_leaves_the_pad_untouched(g_f32):
    """The entry itself on a buffer of this test's: planes at pitch K + 64, the 64 elements behind every plane keep their fill."""
    import ctypes
    from bbb_hip import _lib, ops
    c = CASES["9_padded_pitch"]
    spec, _ = _spec(c)
    gen = torch.Generator().manual_seed(91 + g_f32)
    y, g = _bwd_inputs(c, spec, "softplus", "gauss", g_f32, gen)
    yd, gd = y.cuda(), g.cuda()
    dense = ops.avgpool_act_backward_chwn_bf16(gd, yd, *spec, "softplus")
    E, C, H, W, B = _shape(c)
    planes, K = E * C, H * W * B
    for out_f32 in (True, False):
        dt = torch.float32 if out_f32 else torch.bfloat16
        buf = torch.full((planes, K + 64), 7.0, dtype=dt, device="cuda")
        d = ops._pool_desc(H, W, B, *spec)
        rc = _lib.lib().bbb_avgpool_act_bwd_chwn_bf16(ctypes.byref(d), gd.data_ptr(), yd.data_ptr(), buf.data_ptr(), planes, 2, K + 64,
                                                      (1 if g_f32 else 0) | (2 if out_f32 else 0), _lib.cur_stream(buf.device))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(buf[:, :K].reshape(dense.shape).float(), dense.float())
        assert bool((buf[:, K:] == 7.0).all())


def test_backward_refuses_a_gradient_of_the_wrong_size():
    from bbb_hip import _lib, ops
    y = torch.zeros((1, 2, 9, 8, 8), dtype=torch.bfloat16, device="cuda")
    spec = ((2, 2), (2, 2), (0, 0), True)
    with pytest.raises(_lib.BBBHipError, match="pooled map"):
        ops.avgpool_act_backward_chwn_bf16(torch.zeros((1, 2, 5, 4, 8), dtype=torch.bfloat16, device="cuda"), y, *spec, None)
    with pytest.raises(_lib.BBBHipError):
        ops.avgpool_act_backward_chwn_bf16(torch.zeros((1, 2, 4, 4, 8), dtype=torch.float16, device="cuda"), y, *spec, None)


# ---------------------------------------------------------------------------------------------------------------------------
# C. models
# ---------------------------------------------------------------------------------------------------------------------------
def _m(E, B, Cin, H, W, act, convs, fcs):
    """convs: (Cout, k, stride, padding, pool module factory or None), each followed by `act`; fcs: hidden widths before the output."""
    return dict(E=E, B=B, Cin=Cin, H=H, W=W, act=act, convs=convs, fcs=fcs)


MODELS = {
    "bbb_gap": _m(2, 8, 3, 12, 10, "softplus", [(8, 3, 1, 1, lambda: nn.AvgPool2d(2)), (16, 3, 1, 1, lambda: nn.AdaptiveAvgPool2d(1))], []),
    "bbb_padavg": _m(3, 16, 3, 13, 11, "relu", [(8, 5, 2, 2, lambda: nn.AvgPool2d(3, 2, 1, count_include_pad=False)), (16, 3, 1, 1, None)],
                     [20]),
}
# (beta small enough that the data term, which is what travels through bf16, carries the gradients: with every rounding of the contract
# switched off the helper's own gradients move by 3e-3 / 1.7e-2 of a tensor's maximum on the two models, so agreement with the helper
# far below that says the device rounds where the contract does)
SEED, CALL0, BETA, N = 4242, 17, 1e-3, 1000.0


def _build(spec, kind="bbb"):
    """-> (the model, the contract helper's plan of it)."""
    from bbb_hip import ops
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    Conv, Linear = (BBB_Conv2d, BBB_Linear) if kind == "bbb" else (BBB_LRT_Conv2d, BBB_LRT_Linear)
    Act = nn.Softplus if spec["act"] == "softplus" else nn.ReLU
    net, plan = ModuleWrapper(), []
    cin, H, W = spec["Cin"], spec["H"], spec["W"]
    for i, (cout, k, st, pd, pool) in enumerate(spec["convs"]):
        net.add_module(f"conv{i}", Conv(cin, cout, k, stride=st, padding=pd, bias=True, priors=P.CONFIG_PRIORS))
        net.add_module(f"act{i}", Act())
        H, W = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
        avg = None
        if pool is not None:
            net.add_module(f"pool{i}", pool())
            avg = ops.avgpool_of(getattr(net, f"pool{i}"), H, W)
            H, W = ops.avgpool_plan(H, W, 8, *avg)[:2]
        plan.append(dict(name=f"conv{i}", kind="conv", stride=st, padding=pd, act=spec["act"], pool=avg))
        cin = cout
    feat = cin * H * W
    net.add_module("flatten", FlattenLayer(feat))
    plan[-1]["flat"] = feat
    for j, n in enumerate(spec["fcs"] + [10]):
        net.add_module(f"fc{j}", Linear(feat, n, bias=True, priors=P.CONFIG_PRIORS))
        hidden = j < len(spec["fcs"])
        if hidden:
            net.add_module(f"fact{j}", Act())
        plan.append(dict(name=f"fc{j}", kind="fc", act=spec["act"] if hidden else None))
        feat = n
    return net, plan


_SETUP = {}


def _setup(name, kind="bbb"):
    """The model on the device, its batch, the helper's plan, parameters and the device's Philox noise as numpy (built once)."""
    from bbb_hip import rng
    key = (name, kind)
    if key not in _SETUP:
        spec = MODELS[name]
        torch.manual_seed(sum(map(ord, name)))
        net, plan = _build(spec, kind)
        net = net.cuda()
        rng.assign_stream_ids(net)
        gen = torch.Generator().manual_seed(sum(map(ord, name)) + 1)
        x = torch.rand((spec["B"], spec["Cin"], spec["H"], spec["W"]), generator=gen).cuda()
        y = torch.randint(0, 10, (spec["B"],), generator=gen).cuda()
        mods = dict(net.named_modules())
        params = {L_["name"]: {k: getattr(mods[L_["name"]], k).detach().cpu().numpy() for k in ("W_mu", "W_rho", "bias_mu", "bias_rho")}
                  for L_ in plan}
        first = mods[plan[0]["name"]]
        params["_prior_mu"], params["_prior_sigma"] = float(first.prior_mu), float(first.prior_sigma)
        _SETUP[key] = (spec, net, x, y, plan, params, mods)
    return _SETUP[key]


def _weight_eps(plan, params, mods, E, call0):
    return [{L_["name"]: {kind: O.normal_eps(SEED, call0 + e, mods[L_["name"]]._stream_base + off,
                                            int(np.prod(params[L_["name"]][key].shape))).reshape(params[L_["name"]][key].shape)
                          for kind, key, off in (("W", "W_mu", 0), ("bias", "bias_mu", 1))} for L_ in plan} for e in range(E)]


_REF = {}


def _reference(name):
    """The contract's training step of the model, computed once, shared, left unchanged."""
    if name not in _REF:
        spec, net, x, y, plan, params, mods = _setup(name)
        eps = _weight_eps(plan, params, mods, spec["E"], CALL0)
        _, logits = A.forward(plan, params, x.cpu().numpy(), eps)
        _REF[name] = (torch.stack(logits), A.step_grads(plan, params, x.cpu().numpy(), y.cpu().numpy(), eps, BETA, N))
    return _REF[name]


@pytest.mark.parametrize("name", list(MODELS))
def test_model_inference_vs_contract(name):
    from bbb_hip import ensemble, ops, rng
    spec, net, x, y, plan, params, mods = _setup(name)
    want, _ = _reference(name)                                              # [E, B, 10]
    E = spec["E"]
    with torch.no_grad():
        _, kl32 = ensemble.mc_logits(net, x, E, SEED, CALL0)
        with ops.use_config(bf16_avgpool=True):
            steps = ensemble.chwn_plan(net, tuple(x.shape), E, precision="bf16")
            assert sum(s.form == "avgpool" and s.in_layout == "bf16" for s in steps) == sum(p is not None for *_, p in spec["convs"])
            logits, kl = ensemble.mc_logits(net, x, E, SEED, CALL0, precision="bf16")
            assert ensemble.stats["path"] == "chwn"
            again, _ = ensemble.mc_logits(net, x, E, SEED, CALL0, precision="bf16")
            three, _ = ensemble.mc_logits(net, x, 3, SEED, CALL0, precision="bf16")
            for j in range(3):
                one, _ = ensemble.mc_logits(net, x, 1, SEED, CALL0 + j, precision="bf16")
                assert torch.equal(one[0], three[j]), f"draw {j} of a 3-draw launch differs from the single-draw launch"
            # the drop-in loop under dropin_precision="bf16" is draw 0
            with ops.use_config(dropin_precision="bf16"):
                rng.manual_seed(SEED, call=CALL0)
                out, _ = net(x)
            assert torch.equal(out, logits[0])
    rng.use_device_generator()
    assert torch.equal(kl, kl32) and torch.equal(logits, again)
    assert logits.shape == (E, spec["B"], 10)
    ratio = float((logits.cpu().double() - want).abs().max()) / float(want.abs().max())
    _note(f"{name} logits vs contract / max|logit|", ratio)
    assert ratio <= 1e-2, ratio


@pytest.mark.parametrize("name", list(MODELS))
def test_model_gradients_vs_contract_and_fp32(name):
    from bbb_hip import fast_train, ops, train as T
    spec, net, x, y, plan, params, mods = _setup(name)
    _, (loss_c, lo_c, want) = _reference(name)
    E = spec["E"]

    def grads(precision):
        net.zero_grad(set_to_none=True)
        loss, lo, kl = T.forward_loss(net, x, y, E, BETA, N, seed_call=(SEED, CALL0), precision=precision)
        loss.backward()
        return kl.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    with ops.use_config(bf16_avgpool=True):
        assert fast_train.bf16_train_refusal(net, x) is None
        kl, got = grads("bf16")
    kl32, g32 = grads("fp32")
    net.zero_grad(set_to_none=True)
    assert torch.equal(kl, kl32)
    worst, cos_min = 0.0, 1.0
    for L_ in plan:
        for key in ("W_mu", "W_rho", "bias_mu", "bias_rho"):
            nm = f"{L_['name']}.{key}"
            g = got[nm].double().cpu().numpy()
            w = np.asarray(want[L_["name"]][key]).reshape(g.shape)
            rel = float(np.abs(g - w).max()) / float(np.abs(w).max())
            worst = max(worst, rel)
            a, b = got[nm].double().flatten(), g32[nm].double().flatten()
            cos = float(a @ b / (a.norm() * b.norm()))
            cos_min = min(cos_min, cos)
            assert rel <= 4e-2, (nm, rel)
            assert cos >= 0.995, (nm, cos)
    _note(f"{name} grad vs contract / max|grad|", worst)
    _note(f"{name} 1 - min cosine vs fp32", 1.0 - cos_min)
    print(f"[bf16 avgpool] {name}: max rel grad err vs contract {worst:.2e}, min cosine vs fp32 {cos_min:.6f}")


def test_graphed_mc_replays_the_eager_step():
    from bbb_hip import _lib, ensemble, ops, rng
    spec, net, *_ = _setup("bbb_gap")
    E = 3
    torch.manual_seed(5)
    batches = [torch.rand(spec["B"], 3, 12, 10, device="cuda") for _ in range(3)]
    with torch.no_grad():
        with ops.use_config(bf16_avgpool=True):
            rng.manual_seed(31, call=0)
            eager = [tuple(t.clone() for t in ensemble.mc_forward(net, xb, E, precision="bf16")) for xb in batches]
            rng.manual_seed(31, call=0)
            g = ensemble.GraphedMC(net, batches[0].clone(), E, precision="bf16")
        assert ops.current_config().bf16_avgpool is False                    # the graph took a snapshot of the configuration
        for i in range(3):
            lo, kl = g.step(batches[i])
            torch.cuda.synchronize()
            assert torch.equal(lo, eager[i][0]) and torch.equal(kl, eager[i][1]), i
        with pytest.raises(_lib.BBBHipError, match="bf16_avgpool"):          # outside the context a NEW graph is refused again
            ensemble.GraphedMC(net, batches[0].clone(), E, precision="bf16")
    rng.use_device_generator()


def _fresh(name, seed=12):
    from bbb_hip import rng
    torch.manual_seed(seed)
    net, _ = _build(MODELS[name])
    net = net.cuda()
    rng.assign_stream_ids(net)
    rng.manual_seed(77, call=0)
    return net


def test_graphed_train_step_equals_eager():
    from bbb_hip import ops, rng, train as T
    spec, _, x, y, *_ = _setup("bbb_padavg")
    E, lr = spec["E"], 1e-3
    net_e = _fresh("bbb_padavg")
    opt_e = T.FusedAdam(net_e.parameters(), lr=lr, capturable=True)
    with ops.use_config(bf16_avgpool=True):
        eager = [T.train_step(net_e, opt_e, x, y, E, BETA, N, precision="bf16", graph=False)[0] for _ in range(6)]
    net_g = _fresh("bbb_padavg")
    opt_g = T.FusedAdam(net_g.parameters(), lr=lr, capturable=True)
    g = T.GraphedTrainStep(net_g, opt_g, x, y, E, BETA, N, warmup=3, precision="bf16", launch_config=ops.LaunchConfig(bf16_avgpool=True))
    assert ops.current_config().bf16_avgpool is False
    graphed = [g.step()[0].clone() for _ in range(3)]
    for a, b in zip(eager[3:], graphed):
        assert torch.equal(a, b)
    for (na, a), (_, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(a, b), na
    rng.use_device_generator()


def test_train_step_captures_itself_with_average_pools():
    """train.train_step(precision="bf16") on bbb_gap under the switch, six identical calls: the self-captured graph gives the losses
    of graph=False; the switch is part of the capture key, so switching it off drops the graph and refuses."""
    from bbb_hip import _lib, ops, rng, train as T
    spec, _, x, y, *_ = _setup("bbb_gap")

    def run(graph):
        net = _fresh("bbb_gap", seed=11)
        opt = T.FusedAdam(net.parameters(), lr=1e-3, capturable=True)
        with ops.use_config(bf16_avgpool=True):
            losses = [T.train_step(net, opt, x, y, spec["E"], BETA, N, graph=graph, precision="bf16")[0].item() for _ in range(6)]
        st = T._auto.get(net)
        return net, opt, losses, bool(st and st["graphed"] is not None)

    net_e, _, eager, cap_e = run(False)
    net_g, opt_g, auto, cap_g = run(None)
    assert not cap_e and cap_g
    np.testing.assert_allclose(auto, eager, rtol=2e-5)
    for (na, a), (nb, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        np.testing.assert_allclose(b.detach().cpu().numpy(), a.detach().cpu().numpy(), rtol=2e-5, atol=1e-7, err_msg=na)
    with pytest.raises(_lib.BBBHipError, match="bf16_avgpool"):              # the default configuration: no replay of that graph
        T.train_step(net_g, opt_g, x, y, spec["E"], BETA, N, precision="bf16")
    rng.use_device_generator()


def test_lrt_twin_inference_vs_contract():
    """The GAP model with all-LRT layers under bf16_lrt + bf16_avgpool: logits against the float64 restatement of
    bf16_lrt_contract (its moments, its rounding points) with the pool's one more rounding, within that contract's bound."""
    from bbb_hip import _lib, ensemble, ops
    spec, net, x, y, plan, params, mods = _setup("bbb_gap", kind="lrt")
    E = 2

    def restated(call):
        h = L._rnd(x.cpu().numpy(), True)
        for li, L_ in enumerate(plan):
            p, m = params[L_["name"]], mods[L_["name"]]
            if L_["kind"] == "fc":
                h = h.reshape(h.shape[0], -1)
            am, av = L.lrt_moments(h, p, L_["kind"], L_.get("stride", 1), L_.get("padding", 0), True)
            eps = O.normal_eps(SEED, call, m._stream_base + 2, int(np.prod(am.shape))).reshape(am.shape)
            yv = O.lrt_output(am, av, eps)
            if li == len(plan) - 1:
                return yv
            h = L._rnd(O.softplus_act(yv), True)
            if L_["pool"] is not None:
                pooled = A.pool_fwd(torch.from_numpy(h).double(), A.normal_plan([L_])[0]["pool"])
                h = L._rnd(pooled.float().numpy(), True)

    with torch.no_grad():
        with ops.use_config(bf16_avgpool=True):
            with pytest.raises(_lib.BBBHipError, match="bf16_lrt"):          # the existing LRT hint
                ensemble.mc_logits(net, x, E, SEED, CALL0, precision="bf16")
        with ops.use_config(bf16_lrt=True):
            with pytest.raises(_lib.BBBHipError, match="bf16_avgpool"):
                ensemble.mc_logits(net, x, E, SEED, CALL0, precision="bf16")
        _, kl32 = ensemble.mc_logits(net, x, E, SEED, CALL0)
        with ops.use_config(bf16_lrt=True, bf16_avgpool=True):
            logits, kl = ensemble.mc_logits(net, x, E, SEED, CALL0, precision="bf16")
            assert ensemble.stats["path"] == "chwn-bf16-lrt"
    assert torch.equal(kl, kl32)
    for e in range(E):
        want = restated(CALL0 + e)
        ratio = float(np.abs(logits[e].cpu().numpy() - want).max()) / float(np.abs(want).max())
        _note("lrt gap logits vs contract / max|logit|", ratio)
        assert ratio <= 1e-2, (e, ratio)


def test_refusals():
    from bbb_hip import _lib, ensemble, ops, train as T
    spec, net, x, y, *_ = _setup("bbb_gap")
    opt = T.FusedAdam(net.parameters(), lr=1e-3)
    with torch.no_grad():
        with pytest.raises(_lib.BBBHipError, match="average pooling") as ei:
            ensemble.mc_logits(net, x, 2, SEED, CALL0, precision="bf16")
        assert "bf16_avgpool" in str(ei.value)
    with pytest.raises(_lib.BBBHipError, match="average pooling") as ei:
        T.train_step(net, opt, x, y, 2, BETA, N, precision="bf16", graph=False)
    assert "bf16_avgpool" in str(ei.value)
    _, lrt, *_ = _setup("bbb_gap", kind="lrt")
    with ops.use_config(bf16_avgpool=True, bf16_lrt=True):
        with pytest.raises(_lib.BBBHipError, match="local-reparameterisation"):
            T.forward_loss(lrt, x, y, 2, BETA, N, precision="bf16")
