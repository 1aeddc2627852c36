"""Average pooling on the batch-innermost paths (csrc/pool2d.hip) against float64 references on the CPU, in the two tiers of
test_gpu_train_fuzz.py (EXACT: integers in [-3, 3]; GAUSS: normal operands):

  A. the forward kernel against F.avg_pool2d / F.adaptive_avg_pool2d in float64: bit for bit in the EXACT tier (a sequential fp32
     sum of small integers is exact and ONE IEEE division of it is the correctly rounded quotient, which is what the float64
     result cast to fp32 is, non-power-of-two divisors included); GAUSS within the derived bound of n - 1 sequential fp32 adds and
     one division, (n + 1) * 2^-24 * avgpool(|x|) with n = kh * kw;
  B. the backward of [activation -> pool], BBB and LRT forms, against float64 autograd of the pool routed through the activated
     output as test_pool_act_backward_vs_float64 does: bit for bit where the divisor is a power of two (cases 1, 7, 9; act none /
     relu), else that test's `close` rule and bounds;
  C. generated models (BBB and LRT) against CPU float64 autograd fed the device's Philox noise, parameter gradients within
     test_gpu_train_fuzz.MODEL_BOUND, once more under bf16x3 for the BBB models, and an input gradient;
  D. inference and the other entry points on the two global-average-pool models.

(The fourth model of the issue, lrt_avg_e1, reads "conv(12, 3) + AvgPool2d((2, 1))" on a 3 x 2 map, which a 3 x 3 kernel does not
fit: the convolution here has padding 1, everything else as stated.)  Run with -m gpu."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bbb_numpy as O
import ref_port_torch as P
from test_gpu_train_fuzz import MODEL_BOUND, MODEL_BOUND_LRT_RHO, _check, _dact, _data

pytestmark = pytest.mark.gpu

WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"[avgpool worst] {k[0]:<28s} {k[1]:<10s} {WORST[k]:.3e}")


# (E, C, H, W, B; kernel; stride; padding; count_include_pad) -- or an adaptive output size, resolved through ops.avgpool_of
def _c(E, C, H, W, B, k=None, s=None, p=0, cip=True, adaptive=None):
    return dict(E=E, C=C, H=H, W=W, B=B, k=k, s=s, p=p, cip=cip, adaptive=adaptive)


CASES = {
    "1_plain_floor_row": _c(2, 3, 9, 8, 4, 2, 2, 0, True),
    "2_overlap_padded": _c(1, 5, 9, 7, 12, 3, 2, 1, True),
    "3_overlap_padded_valid": _c(1, 5, 9, 7, 12, 3, 2, 1, False),
    "4_rect": _c(2, 2, 7, 8, 8, (3, 2), (1, 2), (1, 0), False),
    "5_large_padded": _c(1, 4, 11, 9, 4, 5, 3, 2, False),
    "6_global_adaptive": _c(3, 4, 7, 6, 20, adaptive=1),
    "7_gaps": _c(1, 3, 8, 8, 4, 2, 3, 0, True),
    "8_adaptive_3x2": _c(1, 2, 12, 8, 4, adaptive=(3, 2)),
    "9_padded_pitch": _c(2, 3, 16, 16, 4, 2, 2, 0, True),
}
POW2 = ("1_plain_floor_row", "7_gaps", "9_padded_pitch")          # 2 x 2 taps, count_include_pad: divisions by 4 are exact


def _spec(c):
    """(kernel, stride, padding, count_include_pad) as pairs and a bool, and the torch module of the case."""
    from bbb_hip import ops
    if c["adaptive"] is not None:
        mod = nn.AdaptiveAvgPool2d(c["adaptive"])
    else:
        mod = nn.AvgPool2d(c["k"], c["s"], c["p"], count_include_pad=c["cip"])
    spec = ops.avgpool_of(mod, c["H"], c["W"])
    assert spec is not None
    if c["adaptive"] is None:
        assert spec == (ops._pair(c["k"]), ops._pair(c["s"]), ops._pair(c["p"]), c["cip"])
    return spec, mod


def _ref_pool(x64, c, spec):
    """float64 reference on [E, C, H, W, B]: F.adaptive_avg_pool2d for the adaptive cases, else F.avg_pool2d."""
    E, C, H, W, B = x64.shape
    t = x64.permute(0, 4, 1, 2, 3).reshape(E * B, C, H, W)
    if c["adaptive"] is not None:
        o = F.adaptive_avg_pool2d(t, c["adaptive"])
    else:
        o = F.avg_pool2d(t, spec[0], spec[1], spec[2], ceil_mode=False, count_include_pad=spec[3])
    return o.reshape(E, B, C, *o.shape[2:]).permute(0, 2, 3, 4, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# A. forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(CASES))
def test_avgpool_forward_vs_float64(name, tier):
    from bbb_hip import ops
    c = CASES[name]
    spec, _ = _spec(c)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    x = _data(gen, tier, (c["E"], c["C"], c["H"], c["W"], c["B"]))
    want = _ref_pool(x.double(), c, spec)
    got = ops.avgpool_chwn(x.cuda(), *spec)
    assert got.shape == want.shape
    ho, wo, _, _ = ops.avgpool_plan(c["H"], c["W"], c["B"], *spec)
    assert tuple(got.shape[2:4]) == (ho, wo)
    if tier == "exact":
        _check("avgpool_fwd", "exact", got, want)
        _note(("avgpool_fwd", "exact"), 0.0)
        return
    n = spec[0][0] * spec[0][1]
    bound = (n + 1) * 2.0 ** -24 * _ref_pool(x.double().abs(), c, spec)
    err = (got.cpu().double() - want).abs()
    ratio = float((err / (bound + 1e-300)).max())
    _note(("avgpool_fwd err/bound", "gauss"), ratio)
    print(f"[avgpool] forward {name}: worst err / bound {ratio:.3f}")
    assert (err <= bound).all(), f"{name}: err / bound {ratio:.3f} > 1"


def test_avgpool_forward_does_not_depend_on_the_launch_size():
    """A draw computed alone, or inside a 10-draw launch, is the same bits."""
    from bbb_hip import ops
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((10, 5, 9, 7, 12), generator=gen).cuda()
    for spec in (((3, 3), (2, 2), (1, 1), False), ((9, 7), (9, 7), (0, 0), True)):
        full = ops.avgpool_chwn(x, *spec)
        for j in (0, 3, 9):
            assert torch.equal(ops.avgpool_chwn(x[j:j + 1].contiguous(), *spec)[0], full[j])
            assert torch.equal(ops.avgpool_chwn(x[j, 2:3].contiguous(), *spec)[0], full[j, 2])


# ---------------------------------------------------------------------------------------------------------------------------
# B. backward: BBB and LRT forms
# ---------------------------------------------------------------------------------------------------------------------------
def _route(g_in, y, c, spec):
    """float64 average-pool backward through autograd: [E', C, Ho, Wo, B] -> [E', C, H, W, B] (the pool is linear: y gives the shape)."""
    E, C, H, W, B = g_in.shape[0], *y.shape[1:]
    t = torch.zeros((E, C, H, W, B), dtype=torch.float64).requires_grad_(True)
    out = _ref_pool(t, c, spec)
    out.backward(g_in)
    return t.grad


def _inputs(c, spec, tier, gen, shared):
    from bbb_hip import ops
    E, C, H, W, B = (c[n] for n in ("E", "C", "H", "W", "B"))
    Ho, Wo, _, _ = ops.avgpool_plan(H, W, B, *spec)
    Em = 1 if shared else E
    am = torch.randn((Em, C, H, W, B), generator=gen)
    av = torch.rand((Em, C, H, W, B), generator=gen) * 0.5 + 0.05
    eps = torch.randn((E, C, H, W, B), generator=gen)
    v = am + torch.sqrt(av) * eps
    g = _data(gen, tier, (E, C, Ho, Wo, B))
    g2 = _data(gen, tier, (E, C, Ho, Wo, B))
    xc = _data(gen, tier, (Em, C, Ho, Wo, B))
    return am, av, v, g, g2, xc


BWD_RUNS = [(n, a, "gauss") for n in CASES for a in ("none", "relu", "softplus")] + \
           [(n, a, "exact") for n in POW2 for a in ("none", "relu")]


@pytest.mark.parametrize("name,act,tier", BWD_RUNS, ids=[f"{n}-{a}-{t}" for n, a, t in BWD_RUNS])
def test_avgpool_act_backward_vs_float64(name, act, tier):
    from bbb_hip import ops
    c = CASES[name]
    spec, _ = _spec(c)
    shared = c["E"] == 3                      # case 6: three draws over ONE pair of moments (a first layer); else moment_planes == planes
    gen = torch.Generator().manual_seed(sum(map(ord, name + act)) * 2 + (tier == "exact"))
    am, av, v, g, g2, xc = _inputs(c, spec, tier, gen, shared)
    y = {"none": v, "relu": F.relu(v), "softplus": F.softplus(v)}[act].contiguous()
    a = None if act == "none" else act
    exact = tier == "exact"

    def close(what, got, want, rtol, exact):
        got = got.detach().cpu().double()
        if exact:
            _check(what, "exact", got.float(), want)
            _note((what, "exact"), 0.0)
            return
        scale = float(want.abs().max()) + 1e-30
        rel = (got - want).abs() / (want.abs() + 1e-3 * scale)
        _note((what, tier if act != "softplus" else "softplus"), float(rel.max()))
        assert (rel <= rtol).all(), f"{what}: relative error {float(rel.max()):.3e} > {rtol:.1e}"

    yd = y.cuda()
    K = c["H"] * c["W"] * c["B"]
    if name == "9_padded_pitch":
        assert ops.padded_plane_pitch(K) != K                       # pad_planes=True writes at the padded pitch
    want = _route(g.double(), y, c, spec) * _dact(y, a)
    for pad in (False, True):
        got = ops.avgpool_act_backward_chwn(g.cuda(), yd, *spec, a, pad_planes=pad)
        assert got.shape == y.shape and (not pad or got.is_contiguous() == (ops.padded_plane_pitch(K) == K))
        close("avgpool_act_bwd", got, want, 2e-5, exact)
    # LRT: (g + 2 x g2) formed inside, then d/d act_mu and d/d act_var
    g_in = g.double() + 2.0 * xc.double() * g2.double()
    g_mu = _route(g_in, y, c, spec) * _dact(y, a)
    y64 = y.double()
    vv = torch.where(y64 > 20.0, y64, y64 + torch.log(-torch.expm1(-y64))) if a == "softplus" else y64
    g_var = g_mu * (vv - am.double()) / (2.0 * av.double())
    comb = (xc.cuda(), g2.cuda())
    args = (g.cuda(), yd, am.cuda(), av.cuda(), *spec, a)
    outs = [ops.lrt_avgpool_act_backward_chwn(*args, combine=comb),
            ops.lrt_avgpool_act_backward_chwn(*args, pad_planes=True, combine=comb),
            ops.lrt_avgpool_act_backward_chwn(*args, stacked=True, combine=comb)]
    for gm, gv in outs:
        close("lrt_avgpool_act_bwd g_mu", gm, g_mu, 2e-5, exact)
        close("lrt_avgpool_act_bwd g_var", gv, g_var, 2e-4 if a == "softplus" else 2e-5, False)
    # without the combine: the plain incoming gradient
    gm, gv = ops.lrt_avgpool_act_backward_chwn(*args)
    close("lrt_avgpool_act_bwd g_mu", gm, want, 2e-5, exact)


# ---------------------------------------------------------------------------------------------------------------------------
# C. generated models against CPU float64 autograd fed the device's Philox noise
# ---------------------------------------------------------------------------------------------------------------------------
def _m(kind, E, B, Cin, H, W, convs, fcs):
    """convs: (Cout, k, stride, padding, pool module or None), each followed by Softplus; fcs: hidden widths before the 10-way output."""
    return dict(kind=kind, E=E, B=B, Cin=Cin, H=H, W=W, convs=convs, fcs=fcs)


def _gap(kind):
    return _m(kind, 2, 8, 3, 12, 10, [(8, 3, 1, 1, lambda: nn.AvgPool2d(2)), (12, 3, 1, 1, lambda: nn.AdaptiveAvgPool2d(1))], [])


MODELS = {
    "bbb_gap": _gap("bbb"),
    "bbb_padavg": _m("bbb", 3, 12, 3, 13, 11, [(8, 5, 2, 2, lambda: nn.AvgPool2d(3, 2, 1, count_include_pad=False)), (16, 3, 1, 1, None)], [20]),
    "lrt_gap": _gap("lrt"),
    "lrt_avg_e1": _m("lrt", 1, 4, 4, 14, 11, [(8, 3, 2, 0, lambda: nn.AvgPool2d(2)), (8, 3, 1, 1, None),
                                             (12, 3, 1, 1, lambda: nn.AvgPool2d((2, 1)))], [16]),
}


def _build(spec):
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    Conv, Linear = (BBB_Conv2d, BBB_Linear) if spec["kind"] == "bbb" else (BBB_LRT_Conv2d, BBB_LRT_Linear)
    net = ModuleWrapper()
    cin = spec["Cin"]
    probe = torch.zeros(1, 1, spec["H"], spec["W"])
    for i, (cout, k, st, pd, pool) in enumerate(spec["convs"]):
        net.add_module(f"conv{i}", Conv(cin, cout, k, stride=st, padding=pd, bias=True, priors=P.CONFIG_PRIORS))
        net.add_module(f"act{i}", nn.Softplus())
        probe = F.conv2d(probe, torch.zeros(1, 1, k, k), stride=st, padding=pd)
        if pool is not None:
            net.add_module(f"pool{i}", pool())
            probe = getattr(net, f"pool{i}")(probe)
        cin = cout
    feat = cin * probe.shape[2] * probe.shape[3]
    net.add_module("flatten", FlattenLayer(feat))
    for j, n in enumerate(spec["fcs"] + [10]):
        net.add_module(f"fc{j}", Linear(feat, n, bias=True, priors=P.CONFIG_PRIORS))
        if j < len(spec["fcs"]):
            net.add_module(f"fact{j}", nn.Softplus())
        feat = n
    return net


def _model_ref(net, spec, x, y, seed, call0, beta, N, want_dx=False):
    """test_gpu_train_fuzz._model_ref with F.avg_pool2d / F.adaptive_avg_pool2d in place of the max pool: CPU float64 autograd of the
    same model and loss fed the device's Philox noise -> ({parameter: gradient}, d loss / d x or None, the logits [E, B, 10])."""
    from bbb_hip import ensemble
    from layers.bbb import _BBBLayer
    from layers.lrt import _LRTLayer
    mods = ensemble.flat_children(net)
    leaves = {n: p.detach().cpu().double().requires_grad_(True) for n, p in net.named_parameters()}
    pname = {id(m): n for n, m in net.named_modules()}
    KIND = {"W": 0, "bias": 1, "act": 2}

    def sp(r):
        return torch.log1p(torch.exp(r))

    x64 = x.detach().cpu().double().requires_grad_(want_dx)
    outs, logits = [], []
    for j in range(spec["E"]):
        h = x64
        for m in mods:
            if isinstance(m, (_BBBLayer, _LRTLayer)):
                pre = pname[id(m)]
                Wm, Wr, bm, br = (leaves[f"{pre}.{t}"] for t in ("W_mu", "W_rho", "bias_mu", "bias_rho"))
                sid = m._stream_base

                def eps(kind, shape):
                    return torch.from_numpy(O.normal_eps(seed, call0 + j, sid + KIND[kind], int(np.prod(shape))).reshape(shape)).double()

                conv = hasattr(m, "kernel_size")

                def lin(inp, w, b):
                    return F.conv2d(inp, w, b, m.stride, m.padding, m.dilation) if conv else F.linear(inp, w, b)
                if isinstance(m, _BBBLayer):
                    h = lin(h, Wm + eps("W", tuple(Wm.shape)) * sp(Wr), bm + eps("bias", tuple(bm.shape)) * sp(br))
                else:
                    am = lin(h, Wm, bm)
                    av = 1e-16 + lin(h * h, sp(Wr) ** 2, sp(br) ** 2)
                    h = am + torch.sqrt(av) * eps("act", tuple(am.shape))
            elif isinstance(m, nn.Softplus):
                h = F.softplus(h)
            elif isinstance(m, nn.AvgPool2d):
                h = F.avg_pool2d(h, m.kernel_size, m.stride, m.padding, m.ceil_mode, m.count_include_pad)
            elif isinstance(m, nn.AdaptiveAvgPool2d):
                h = F.adaptive_avg_pool2d(h, m.output_size)
            else:
                h = h.reshape(-1, m.num_features)
        logits.append(h.detach())
        outs.append(F.log_softmax(h, dim=1))
    kl = 0.0
    for m in mods:
        if isinstance(m, (_BBBLayer, _LRTLayer)):
            pre = pname[id(m)]
            for a, b in (("W_mu", "W_rho"), ("bias_mu", "bias_rho")):
                kl = kl + P._kl(m.prior_mu, m.prior_sigma, leaves[f"{pre}.{a}"], sp(leaves[f"{pre}.{b}"]))
    lo = P.logmeanexp(torch.stack(outs, dim=2), 2)
    loss = F.nll_loss(lo, y.cpu()) * N + beta * kl
    loss.backward()
    return {n: t.grad for n, t in leaves.items()}, (x64.grad if want_dx else None), torch.stack(logits)


SEED, CALL0, BETA, N = 4242, 17, 1e-3, 100.0
_REF = {}


def _setup(name, want_dx=False):
    """The model on the device, its batch, and the float64 reference (computed once per model, shared by the tests, left unchanged)."""
    from bbb_hip import rng
    spec = MODELS[name]
    torch.manual_seed(sum(map(ord, name)))
    net = _build(spec).cuda()
    rng.assign_stream_ids(net)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 1)
    x = torch.rand((spec["B"], spec["Cin"], spec["H"], spec["W"]), generator=gen).cuda()
    y = torch.randint(0, 10, (spec["B"],), generator=gen).cuda()
    if name not in _REF:
        _REF[name] = _model_ref(net, spec, x, y, SEED, CALL0, BETA, N, want_dx=True)
    return spec, net, x, y, _REF[name]


def _grad_fails(spec, net, want, mode):
    fails = []
    for n, p in net.named_parameters():
        kind = n.split(".")[-1]
        got, w = p.grad.detach().cpu().double(), want[n]
        ratio = float((got - w).abs().max()) / (float(w.abs().max()) + 1e-30)
        lrt_rho = spec["kind"] == "lrt" and kind.endswith("rho")
        _note((f"model {spec['kind']} {kind}", mode), ratio)
        bound = MODEL_BOUND_LRT_RHO if lrt_rho else MODEL_BOUND[kind]
        if not ratio <= bound:
            fails.append((n, ratio, bound))
    return fails


MODEL_RUNS = [(n, "fp32") for n in MODELS] + [(n, "bf16x3") for n in MODELS if MODELS[n]["kind"] == "bbb"]


@pytest.mark.parametrize("name,mode", MODEL_RUNS, ids=[f"{n}-{m}" for n, m in MODEL_RUNS])
def test_model_gradients_vs_float64_autograd(name, mode):
    from bbb_hip import ensemble, fast_train, ops, rng
    spec, net, x, y, (want, _, _) = _setup(name)
    assert fast_train.train_path_ok(net, x) == spec["kind"]
    cfg = dict(gemm_mode=mode, bf16x3_min_workgroups=0) if mode == "bf16x3" else {}
    with ops.use_config(**cfg):
        rng.manual_seed(SEED, call=CALL0)
        lo, kl = ensemble.mc_forward(net, x, spec["E"], kl_mode="mean")
        assert ensemble.stats["path"] == "chwn-autograd"
        (F.nll_loss(lo, y) * N + BETA * kl).backward()
    fails = _grad_fails(spec, net, want, mode)
    assert not fails, fails


@pytest.mark.parametrize("name", ["bbb_gap", "lrt_gap"])
def test_model_input_gradient_vs_float64_autograd(name):
    from bbb_hip import ensemble, fast_train, rng
    spec, net, x, y, (want, want_dx, _) = _setup(name)
    x = x.clone().requires_grad_()
    assert fast_train.train_path_ok(net, x) == spec["kind"]
    rng.manual_seed(SEED, call=CALL0)
    lo, kl = ensemble.mc_forward(net, x, spec["E"], kl_mode="mean")
    assert ensemble.stats["path"] == "chwn-autograd"
    (F.nll_loss(lo, y) * N + BETA * kl).backward()
    ratio = float((x.grad.cpu().double() - want_dx).abs().max()) / (float(want_dx.abs().max()) + 1e-30)
    _note((f"model {spec['kind']} dx", "fp32"), ratio)
    assert ratio <= MODEL_BOUND["W_mu"], ratio
    assert not _grad_fails(spec, net, want, "fp32+dx")


# ---------------------------------------------------------------------------------------------------------------------------
# D. inference and the other entry points
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bbb_gap", "lrt_gap"])
def test_inference_paths_agree(name, monkeypatch):
    from bbb_hip import _lib, ensemble, rng
    from layers import _fused
    spec, net, x, y, (_, _, want_logits) = _setup(name)
    with torch.no_grad():
        logits3, _ = ensemble.mc_logits(net, x, 3, SEED, CALL0)
        assert ensemble.stats["path"] == "chwn"                                  # what an admitted model reports
        assert logits3.shape == (3, spec["B"], 10)
        for j in range(3):
            one, _ = ensemble.mc_logits(net, x, 1, SEED, CALL0 + j)
            assert ensemble.stats["path"] == "chwn"
            assert torch.equal(one[0], logits3[j]), f"draw {j} of a 3-draw launch differs from the single-draw launch"
        rng.manual_seed(SEED, call=CALL0)
        out, _ = net(x)
        assert torch.equal(out, logits3[0])                                       # the drop-in net(x) is draw 0
        # against the float64 forward with the same noise (the reference holds spec["E"] = 2 draws)
        w = want_logits
        ratio = float((logits3[:w.shape[0]].cpu().double() - w).abs().max()) / float(w.abs().max())
        _note((f"model {spec['kind']} logits", "fp32"), ratio)
        assert ratio <= MODEL_BOUND["W_mu"], ratio

        # a forward hook on the pooling module: hooked_chain serves the model, bit for bit the module-by-module loop
        seen, served = [], []
        hook = net.pool1.register_forward_hook(lambda m, i, o: seen.append((tuple(i[0].shape), tuple(o.shape))))
        real = _fused.hooked_chain

        def spy(wrapper, xx, scope):
            r = real(wrapper, xx, scope)
            served.append(r is not None)
            return r
        monkeypatch.setattr(_fused, "hooked_chain", spy)
        try:
            rng.manual_seed(SEED, call=CALL0)
            chained, _ = net(x)
            assert served == [True] and seen == [((spec["B"], 12, 6, 5), (spec["B"], 12, 1, 1))]
            _fused.hooked_chain_enabled[0] = False
            try:
                rng.manual_seed(SEED, call=CALL0)
                looped, _ = net(x)
            finally:
                _fused.hooked_chain_enabled[0] = True
            assert served == [True, False] and len(seen) == 2 and seen[0] == seen[1]
            assert torch.equal(chained, looped)
        finally:
            hook.remove()
        with pytest.raises(_lib.BBBHipError, match="average pooling"):
            ensemble.mc_logits(net, x, 2, SEED, CALL0, precision="bf16")


def test_train_step_captures_itself_with_average_pools():
    """train.train_step on lrt_gap, six identical calls: the self-captured graph gives the losses of graph=False (compared as
    test_gpu_train.py::test_train_step_captures_itself_and_keeps_the_eager_sequence does, at its tolerance)."""
    from bbb_hip import rng, train as T
    spec = MODELS["lrt_gap"]
    gen = torch.Generator().manual_seed(9)
    x = torch.rand((spec["B"], spec["Cin"], spec["H"], spec["W"]), generator=gen).cuda()
    y = torch.randint(0, 10, (spec["B"],), generator=gen).cuda()

    def run(graph):
        torch.manual_seed(11)
        net = _build(spec).cuda()
        rng.assign_stream_ids(net)
        rng.manual_seed(77, call=0)
        opt = T.FusedAdam(net.parameters(), lr=1e-3)
        losses = [T.train_step(net, opt, x, y, spec["E"], 0.1, 1000.0, graph=graph)[0].item() for _ in range(6)]
        st = T._auto.get(net)
        return net, losses, bool(st and st["graphed"] is not None)

    net_e, eager, cap_e = run(False)
    net_g, auto, cap_g = run(None)
    assert not cap_e and cap_g
    np.testing.assert_allclose(auto, eager, rtol=2e-5)
    for (na, a), (nb, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        np.testing.assert_allclose(b.detach().cpu().numpy(), a.detach().cpu().numpy(), rtol=2e-5, atol=1e-7, err_msg=na)
