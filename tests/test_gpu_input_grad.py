"""Input gradients (d loss / d x) of Monte-Carlo forwards on the batch-innermost path: ops.first_layer_input_grad (the first layer's
contraction on the forward GEMM + bbb_input_grad_col2im), the autograd nodes' `x` output (fast_train._MCForward / _MCForwardLRT,
whose frozen-parameter backward runs no weight side: fast_train._Schedule(weight_side=False)) and the routing of ensemble.mc_forward / mc_logits / train.forward_loss, frozen parameters included.

  * kernel sweep against float64 (torch.nn.grad.conv2d_input summed over draws) over first layers fast_train._train_path_static
    admits -- the zoo's three first layers at full channel counts, strides 2-4 with floor-dropped rows, dilations 2-3, rectangular
    geometries, Cin 1 / 3 / 4 / 6 / 8, a first linear layer, E 1 / 2 / 10, B 4 / 12 / 36, dense and padded-pitch g_pre, the LRT
    combine form -- under gemm_mode fp32 and bf16x3, in the two tiers of test_gpu_train_fuzz.py (EXACT: small-integer operands,
    bit for bit; GAUSSIAN: |err| <= 2e-5 * the same backward on |operands|, widened by sqrt(K / 4096));
  * generated fast-path models (BBB and LRT; BBB also under bf16x3): x.grad against float64 autograd of the same model fed the
    device's own Philox noise, max |got - want| / max |want| <= 2e-4 (BBB) / 1e-3 (LRT);
  * the same gradient through the drop-in `net(x)` loop (reference-layout path) under the same seed and call index;
  * invariants, bitwise: parameter gradients and logits with and without x.requires_grad, x.grad with frozen / trainable
    parameters, two runs, the overlap_wgrad / flips_up_front switches; frozen parameters get no .grad;
  * the bf16 storage mode refuses x.requires_grad.
Run with -m gpu."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.grad import conv2d_input

import bbb_numpy as O
import ref_port_torch as P
from test_gpu_train_fuzz import MODELS, _build

pytestmark = pytest.mark.gpu

CONFIGS = [dict(gemm_mode=m, bf16x3_min_workgroups=0, split_k=sk) for m in ("fp32", "bf16x3") for sk in (False, True)]
C_GAUSS = 2e-5
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"[input-grad worst] {k[0]:<34s} {k[1]:<8s} {WORST[k]:.3e}")


def _out_hw(H, W, kh, kw, s, p, d):
    return (H + 2 * p[0] - d[0] * (kh - 1) - 1) // s[0] + 1, (W + 2 * p[1] - d[1] * (kw - 1) - 1) // s[1] + 1


def _case(B, E, Cin, Cout, H, W, kh, kw, s=(1, 1), p=(0, 0), d=(1, 1)):
    return dict(B=B, E=E, Cin=Cin, Cout=Cout, H=H, W=W, kh=kh, kw=kw, s=tuple(s), p=tuple(p), d=tuple(d))


def _cases(n, seed):
    """First layers as _train_path_static admits them: any stride, padding 0..d*(k-1), any dilation and channel count."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        kh, kw = int(rs.choice([1, 2, 3, 5, 7])), int(rs.choice([1, 2, 3, 5]))
        d = (int(rs.randint(1, 4)), int(rs.randint(1, 4)))
        p = (int(rs.randint(0, d[0] * (kh - 1) + 1)), int(rs.randint(0, d[1] * (kw - 1) + 1)))
        s = (int(rs.randint(1, 5)), int(rs.randint(1, 5)))
        H, W = int(rs.randint(3, 20)), int(rs.randint(3, 20))
        Cin, Cout = int(rs.choice([1, 3, 4, 6, 8])), int(rs.choice([1, 5, 16, 33, 64]))
        B, E = int(rs.choice([4, 12, 36])), int(rs.choice([1, 2, 10]))
        ho, wo = _out_hw(H, W, kh, kw, s, p, d)
        if H == W or ho < 1 or wo < 1 or B * E * Cin * Cout * ho * wo * kh * kw > 8e6:
            continue
        out.append(_case(B, E, Cin, Cout, H, W, kh, kw, s, p, d))
    return out


CASES = {
    "alexnet_conv1": _case(4, 2, 3, 64, 32, 32, 11, 11, s=(4, 4), p=(5, 5)),
    "3conv3fc_conv1": _case(4, 1, 3, 32, 32, 32, 5, 5, p=(2, 2)),
    "lenet_conv1": _case(12, 10, 1, 6, 32, 32, 5, 5),
    "s3_floor_rect_dil2": _case(12, 2, 6, 10, 17, 11, 3, 2, s=(3, 2), p=(2, 1), d=(2, 1)),          # rows dropped by the floor
    "s4_dil3": _case(36, 1, 4, 16, 19, 14, 3, 3, s=(4, 3), p=(6, 3), d=(3, 3)),
    "s2_q0_cin8": _case(4, 10, 8, 5, 9, 12, 5, 3, s=(2, 2), p=(4, 2)),                                 # padding = d*(k-1)
    "linear_first": _case(12, 2, 48, 10, 1, 1, 1, 1),
    "linear_first_e10": _case(36, 10, 12, 33, 1, 1, 1, 1),
}
CASES.update({f"rand{i}": c for i, c in enumerate(_cases(10, 20261016))})


def _data(gen, tier, shape, scale=1.0):
    if tier == "exact":
        return torch.randint(-3, 4, shape, generator=gen).float()
    return torch.randn(shape, generator=gen) * scale


def _ref(c, g, w):
    """float64 sum over draws of conv2d_input: g [E, Cout, Ho, Wo, B], w [E, Cout, Cin, kh, kw] -> [B, Cin, H, W]."""
    geom = dict(stride=c["s"], padding=c["p"], dilation=c["d"])
    return sum(conv2d_input((c["B"], c["Cin"], c["H"], c["W"]), w[e], g[e].permute(3, 0, 1, 2), **geom) for e in range(g.shape[0]))


def _check(name, tier, got, want, mag, K):
    got = got.detach().cpu()
    if tier == "exact":
        bad = got != want.float()
        assert not bad.any(), f"{name}: {int(bad.sum())} of {got.numel()} elements differ from the exact result"
        _note((name, tier), 0.0)
        return
    err = (got.double() - want).abs()
    c = C_GAUSS * max(1.0, math.sqrt(K / 4096.0))
    ratio = float((err / (mag + 1e-30)).max())
    _note((name, tier), ratio)
    assert (err <= c * mag + 1e-30).all(), f"{name}: err / mag {ratio:.3e} > {c:.3e}"


def _padded(g):
    """g [E, C, Ho, Wo, B] as pool_act_backward_chwn(pad_planes=True) leaves a first layer's gradient: rows at a pitch K + 32 whose
    pad columns hold NaN here (they are contracted and never read)."""
    E, C, Ho, Wo, B = g.shape
    K = Ho * Wo * B
    buf = torch.full((E * C, K + 32), float("nan"), device=g.device)
    buf[:, :K] = g.reshape(E * C, K)
    return buf[:, :K].view(E, C, Ho, Wo, B)


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(CASES))
def test_first_layer_input_grad_vs_float64(name, tier):
    from bbb_hip import ops
    c = CASES[name]
    B, E, Cin, Cout, H, W, kh, kw = (c[k] for k in ("B", "E", "Cin", "Cout", "H", "W", "kh", "kw"))
    ho, wo = _out_hw(H, W, kh, kw, c["s"], c["p"], c["d"])
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    g = _data(gen, tier, (E, Cout, ho, wo, B))
    w = _data(gen, tier, (E, Cout, Cin, kh, kw), 0.3)
    want = _ref(c, g.double(), w.double())
    mag = _ref(c, g.double().abs(), w.double().abs()) if tier == "gauss" else None
    K = E * Cout * kh * kw
    gd, wd = g.cuda(), w.cuda()
    for cfg in CONFIGS:
        tag = f"{cfg['gemm_mode']}{'-splitk' if cfg['split_k'] else ''}"
        with ops.use_config(**cfg):
            for form, gg in (("dense", gd), ("padded", _padded(gd))):
                dx = ops.first_layer_input_grad(gg, wd, (H, W), c["s"], c["p"], c["d"])
                assert dx.shape == (B, Cin, H, W)
                _check(f"dx[{tag}]-{form}", tier, dx, want, mag, K)
    # LRT form: the two moment gradients (summed over draws) with W_mu / W_var, combined as T(g_mu, W_mu) + 2 x T(g_var, W_var)
    c1 = dict(c, E=1)
    gp = _data(gen, tier, (2, 1, Cout, ho, wo, B))
    wp = _data(gen, tier, (2, Cout, Cin, kh, kw), 0.3)
    x = _data(gen, tier, (B, Cin, H, W))
    t0, t1 = _ref(c1, gp[0].double(), wp[0:1].double()), _ref(c1, gp[1].double(), wp[1:2].double())
    want = t0 + 2 * x.double() * t1
    mag = None
    if tier == "gauss":
        mag = _ref(c1, gp[0].double().abs(), wp[0:1].double().abs()) + 2 * x.double().abs() * _ref(c1, gp[1].double().abs(), wp[1:2].double().abs())
    gpd, wpd, xd = gp.cuda(), wp.cuda(), x.cuda()
    for cfg in CONFIGS:
        tag = f"{cfg['gemm_mode']}{'-splitk' if cfg['split_k'] else ''}"
        with ops.use_config(**cfg):
            for form, pair in (("pair", (gpd[0], gpd[1])), ("apart", (gpd[0].clone(), gpd[1].clone()))):
                dx = ops.first_layer_input_grad(pair, (wpd[0], wpd[1]), (H, W), c["s"], c["p"], c["d"], x_lrt=xd)
                _check(f"dx-lrt[{tag}]-{form}", tier, dx, want, mag, Cout * kh * kw)


def test_first_layer_input_grad_is_deterministic():
    from bbb_hip import ops
    c = CASES["alexnet_conv1"]
    gen = torch.Generator().manual_seed(3)
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    g = torch.randn((10, 64, ho, wo, 64), generator=gen).cuda()
    w = torch.randn((10, 64, 3, 11, 11), generator=gen).cuda()
    a = ops.first_layer_input_grad(g, w, (32, 32), c["s"], c["p"], c["d"])
    b = ops.first_layer_input_grad(g, w, (32, 32), c["s"], c["p"], c["d"])
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------
def _model_ref_x(net, spec, x, y, seed, call0, beta, N):
    """test_gpu_train_fuzz._model_ref restated with x as a float64 leaf: -> d loss / d x."""
    from bbb_hip import ensemble
    from layers.bbb import _BBBLayer
    from layers.lrt import _LRTLayer
    mods = ensemble.flat_children(net)
    prm = {n: p.detach().cpu().double() for n, p in net.named_parameters()}
    pname = {id(m): n for n, m in net.named_modules()}
    KIND = {"W": 0, "bias": 1, "act": 2}
    sp = lambda r: torch.log1p(torch.exp(r))
    x64 = x.detach().cpu().double().requires_grad_(True)
    outs = []
    for j in range(spec["E"]):
        h = x64
        for m in mods:
            if isinstance(m, (_BBBLayer, _LRTLayer)):
                pre = pname[id(m)]
                Wm, Wr, bm, br = (prm[f"{pre}.{t}"] for t in ("W_mu", "W_rho", "bias_mu", "bias_rho"))
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
            elif isinstance(m, nn.MaxPool2d):
                h = F.max_pool2d(h, m.kernel_size, m.stride)
            else:
                h = h.reshape(-1, m.num_features)
        outs.append(F.log_softmax(h, dim=1))
    lo = P.logmeanexp(torch.stack(outs, dim=2), 2)
    (F.nll_loss(lo, y.cpu()) * N).backward()
    return x64.grad


X_BOUND = {"bbb": 2e-4, "lrt": 1e-3}
MODEL_RUNS = [(n, "fp32") for n in MODELS] + [(n, "bf16x3") for n in MODELS if MODELS[n]["kind"] == "bbb"]


def _setup(name):
    from bbb_hip import fast_train, rng
    spec = MODELS[name]
    torch.manual_seed(sum(map(ord, name)))
    net = _build(spec).cuda()
    rng.assign_stream_ids(net)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 7)
    x = torch.rand((spec["B"], spec["Cin"], spec["H"], spec["W"]), generator=gen).cuda()
    y = torch.randint(0, 10, (spec["B"],), generator=gen).cuda()
    assert fast_train.train_path_ok(net, x) == spec["kind"]
    return spec, net, x, y


def _ratio(got, want):
    return float((got.detach().cpu().double() - want).abs().max()) / (float(want.abs().max()) + 1e-30)


@pytest.mark.parametrize("name,mode", MODEL_RUNS, ids=[f"{n}-{m}" for n, m in MODEL_RUNS])
def test_model_input_gradient_vs_float64_autograd(name, mode):
    from bbb_hip import ensemble, ops, rng
    spec, net, x, y = _setup(name)
    net.requires_grad_(False)                                  # the attack / saliency case: frozen weights
    seed, call0, N = 4242, 17, 100.0
    cfg = dict(gemm_mode=mode, bf16x3_min_workgroups=0) if mode == "bf16x3" else {}
    xg = x.clone().requires_grad_(True)
    with ops.use_config(**cfg):
        rng.manual_seed(seed, call=call0)
        lo, kl = ensemble.mc_forward(net, xg, spec["E"], kl_mode="mean")
        assert ensemble.stats["path"] == "chwn-autograd"
        (F.nll_loss(lo, y) * N).backward()
    want = _model_ref_x(net, spec, x, y, seed, call0, 0.0, N)
    r = _ratio(xg.grad, want)
    _note((f"model {spec['kind']} x.grad", mode), r)
    assert r <= X_BOUND[spec["kind"]], r
    assert all(p.grad is None for p in net.parameters())


@pytest.mark.parametrize("name", list(MODELS))
def test_mc_forward_input_gradient_matches_the_dropin_loop(name):
    """Same seed and call index: the new node's x.grad against the drop-in `net(x)` loop (per-layer reference-layout path)."""
    from bbb_hip import ensemble, rng
    spec, net, x, y = _setup(name)
    net.requires_grad_(False)
    E, N = spec["E"], 100.0
    grads = []
    for fast in (True, False):
        xg = x.clone().requires_grad_(True)
        rng.manual_seed(99, call=5)
        if fast:
            lo, _ = ensemble.mc_forward(net, xg, E, kl_mode="mean")
            assert ensemble.stats["path"] == "chwn-autograd"
        else:
            outs = [F.log_softmax(net(xg)[0], dim=1) for _ in range(E)]
            lo = P.logmeanexp(torch.stack(outs, dim=2), 2)
        (F.nll_loss(lo, y) * N).backward()
        grads.append(xg.grad.detach().double().cpu())
    r = _ratio(grads[0], grads[1])
    _note((f"vs net(x) loop {spec['kind']}", "fp32"), r)
    assert r <= X_BOUND[spec["kind"]], r


def _run(net, x, y, E, want_x, frozen=False, seed=7, call=3):
    from bbb_hip import ensemble, rng
    net.zero_grad(set_to_none=True)
    net.requires_grad_(not frozen)
    xg = x.clone().requires_grad_(want_x)
    rng.manual_seed(seed, call=call)
    lo, kl = ensemble.mc_forward(net, xg, E, kl_mode="mean")
    assert ensemble.stats["path"] == "chwn-autograd"
    loss = F.nll_loss(lo, y) * 100.0 + (0.0 if frozen else 1e-3 * kl)
    loss.backward()
    pg = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in net.named_parameters()}
    return lo.detach().clone(), pg, (xg.grad.detach().clone() if want_x else None)


@pytest.mark.parametrize("name", ["bbb_c3_lenetlike", "bbb_dil_c1_pool23", "lrt_s2_c3_pool32", "lrt_c8_cin6_e1"])
def test_input_gradient_invariants(name):
    from bbb_hip import fast_train
    spec, net, x, y = _setup(name)
    E = spec["E"]
    lo0, pg0, _ = _run(net, x, y, E, False)
    lo1, pg1, gx1 = _run(net, x, y, E, True)
    assert torch.equal(lo0, lo1)
    for n in pg0:
        assert torch.equal(pg0[n], pg1[n]), n                                  # the weight side does not change with d/dx
    _, pgf, gxf = _run(net, x, y, E, True, frozen=True)
    assert all(v is None for v in pgf.values())                                 # frozen: no parameter gets a .grad
    assert torch.equal(gx1, gxf)                                                # x.grad: frozen == trainable
    _, _, gx2 = _run(net, x, y, E, True, frozen=True)
    assert torch.equal(gxf, gx2)                                                # two runs, same bits
    for flag in (fast_train.overlap_wgrad, fast_train.flips_up_front):
        flag[0] = False
        try:
            _, _, gx3 = _run(net, x, y, E, True)
        finally:
            flag[0] = True
        assert torch.equal(gx1, gx3)
    net.requires_grad_(True)


@pytest.mark.parametrize("lt", ["bbb", "lrt"])
def test_zoo_models_route_input_gradients_to_the_node(lt):
    """AlexNet / 3Conv3FC / LeNet from the zoo with frozen weights: mc_forward, forward_loss and mc_logits all take the node."""
    import layers  # noqa: F401
    from bbb_hip import ensemble, rng, train, zoo
    for net_type, cin in (("alexnet", 3), ("3conv3fc", 3), ("lenet", 1)):
        torch.manual_seed(1)
        net = zoo.getModel(net_type, cin, 10, P.CONFIG_PRIORS, lt, "softplus").cuda().requires_grad_(False)
        rng.assign_stream_ids(net)
        x = torch.rand(8, cin, 32, 32, device="cuda").requires_grad_(True)
        y = torch.randint(0, 10, (8,), device="cuda")
        grads = []
        for entry in ("mc_forward", "forward_loss", "mc_logits"):
            x.grad = None
            rng.manual_seed(11, call=2)
            if entry == "mc_forward":
                lo, _ = ensemble.mc_forward(net, x, 2, kl_mode="mean")
                loss = F.nll_loss(lo, y)
            elif entry == "forward_loss":
                loss, lo, _ = train.forward_loss(net, x, y, 2, 0.0, 1.0)
            else:
                logits, _ = ensemble.mc_logits(net, x, 2, 11, 2)
                loss = F.nll_loss(P.logmeanexp(F.log_softmax(logits, dim=2).permute(1, 2, 0), 2), y)
            assert ensemble.stats["path"] == "chwn-autograd", (net_type, entry)
            loss.backward()
            assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0, (net_type, entry)
            grads.append(x.grad.clone())
        for g in grads[1:]:                                  # (the three tails differ in their last bits only)
            assert _ratio(g, grads[0].double().cpu()) <= X_BOUND[lt], net_type


def test_bf16_training_refuses_input_gradients():
    import layers  # noqa: F401
    from bbb_hip import _lib, rng, train, zoo
    torch.manual_seed(1)
    net = zoo.getModel("3conv3fc", 3, 10, P.CONFIG_PRIORS, "bbb", "softplus").cuda()
    rng.assign_stream_ids(net)
    x = torch.rand(16, 3, 32, 32, device="cuda").requires_grad_(True)
    y = torch.randint(0, 10, (16,), device="cuda")
    with pytest.raises(_lib.BBBHipError):
        train.forward_loss(net, x, y, 2, 0.1, 100.0, precision="bf16")
