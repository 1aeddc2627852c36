"""bf16 input gradients of LRT models (LaunchConfig.bf16_lrt + bf16_lrt_input_grad) on the MI355X: the new pass
(ops.lrt_pool_act_backward_chwn_bf16 = bbb_lrt_pool_act_bwd_chwn_bf16) against its float64 restatement on the same operands, the node's
forward against the bf16 LRT inference path bit for bit, whole-model d loss / d x against the restatement of the backward walk evaluated
FROM THE DEVICE TAPE (tests/bf16_lrt_input_grad_contract.py) and against the fp32 LRT node, the exact
properties of the node, the three entry points, and the switch.  Stated tolerances:
  * the pass, per element: one bf16 ulp of the float64 reference plus 4 fp32 ulps of the sum of the absolute values of the terms that
    form it (the combine d1 + 2 x d2 and overlapping windows can cancel: that is not charged to the kernel); where ReLU's stored y is 0
    the result is exactly +-0;
  * whole-model dx against the walk restated from the device tape, max |dx - contract| / max |contract|: DX_BOUND = twice the worst
    value measured over the seven models and three entries on the MI355X (the margin: a rounding that falls the other way on another
    build), never above 4e-2, the project's bf16 bound.  Measured: MEASURED_DX below, worst 3.453e-6 (M5), so DX_BOUND = 6.906e-6;
  * cosine between this dx and the fp32 LRT node's dx for the same noise: COS_BOUND = 1 - 2 * (1 - worst measured).  Measured:
    MEASURED_COS below, worst 0.995485 (M1), so COS_BOUND = 0.99097;
  * logits against the inference path, kl against the fp32 kl, x.grad of two identical calls: bitwise.
Run with -m gpu."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16_lrt_input_grad_contract as CL
import ref_port_torch as P

pytestmark = pytest.mark.gpu

F64 = torch.float64
BOTH = dict(bf16_lrt=True, bf16_lrt_input_grad=True, bf16_strided_train=True)

# max |dx - contract| / max |contract| over the three entries, and the cosine with the fp32 node's dx, as measured on the MI355X
# (E = 2, B = 8, the seeds below)
# (M5 through mc_forward / mc_logits: one bf16 rounding fell the other way -- the logits' gradient there is float64 in the restatement
# and fp32 on the device; everywhere else what is left is the fp32 accumulation of the device against float64)
MEASURED_DX = {"M1": 7.859e-8, "M2": 8.910e-8, "M3": 9.483e-8, "M4": 7.265e-8, "M5": 3.453e-6, "M6": 6.625e-8, "M7": 9.951e-8}
MEASURED_COS = {"M1": 0.995485, "M2": 0.999759, "M3": 0.998504, "M4": 0.999990, "M5": 0.999801, "M6": 0.998787, "M7": 0.995806}
DX_BOUND = min(2 * max(v for v in MEASURED_DX.values()), 4e-2)       # capped at the project's bf16 bound: a larger measurement is a finding
COS_BOUND = 1 - 2 * (1 - min(MEASURED_COS.values()))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _fold(t):
    """device [E, C, H, W, B] -> float64 CPU [E * B, C, H, W]"""
    E, C, H, W, B = t.shape
    return t.detach().cpu().to(F64).permute(0, 4, 1, 2, 3).reshape(E * B, C, H, W)


# ---- the pass alone ----------------------------------------------------------------------------------------------------------------
SEED, SID = 20261019, 9
_ops_cache = {}


def _operands(hw, B, ks, act, E=2, C=8, call0=7, b_offset=0):
    """Random bf16 / fp32 operands of one pass on the device, made once per key: y (ReLU: about half zeros), act_var per draw, the
    bf16 and fp32 incoming gradients, d2 and x_out for the combine, and the noise of every draw from ops.eps_dump."""
    key = (hw, B, ks, act, E, C, call0, b_offset)
    if key in _ops_cache:
        return _ops_cache[key]
    from bbb_hip import ops
    H, W = hw
    k, s = ks
    hp, wp = (H, W) if k == 0 else ((H - k) // s + 1, (W - k) // s + 1)
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, repr(key))))
    r = lambda *sh: torch.randn(*sh, device="cuda", generator=g)
    v = r(E, C, H, W, B)
    y = (v if act is None else F.relu(v) if act == "relu" else F.softplus(v)).to(torch.bfloat16)
    av = 0.02 + torch.rand(E, C, H, W, B, device="cuda", generator=g)
    o = dict(y=y, av=av, g16=r(E, C, hp, wp, B).to(torch.bfloat16), g32=r(E, C, hp, wp, B), d2=r(E, C, hp, wp, B).to(torch.bfloat16),
             xo=r(E, C, hp, wp, B).to(torch.bfloat16), E=E, C=C, call0=call0, b_offset=b_offset, ks=ks, act=act)
    n = B * C * H * W
    o["eps"] = torch.stack([ops.eps_dump(n, SEED, call0 + e, SID, y.device, start=b_offset * C * H * W).cpu().to(F64).reshape(B, C, H, W)
                            for e in range(E)]).reshape(E * B, C, H, W)
    _ops_cache[key] = o
    return o


def _launch(o, gform, combine, shared, **over):
    from bbb_hip import ops
    a = dict(o, **over)
    k, s = o["ks"]
    y = a["y"] if (o["act"] is not None or k) else (a["y"] if gform == "g16" else None)      # (no y: the logits layer's form)
    av = a["av"][:1] if shared else a["av"]
    comb = (a["xo"], a["d2"]) if combine else None
    return ops.lrt_pool_act_backward_chwn_bf16(a[gform], y, av, k, s, o["act"], noise=(SEED, o["call0"], SID), combine=comb,
                                               b_offset=o["b_offset"])


def _check_pass(o, out, gform, combine, shared, what):
    k, s = o["ks"]
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (2,) + tuple(o["y"].shape)
    y64 = _fold(o["y"])
    av = o["av"][:1].expand_as(o["av"]) if shared else o["av"]
    comb = (_fold(o["xo"]), _fold(o["d2"])) if combine else None
    g_mu, g_var, a_mu, a_var = CL.lrt_pass(_fold(o[gform]), y64 if (o["act"] or k) else None, _fold(av), o["eps"], k, s, o["act"], combine=comb)
    worst = 0.0
    for got, want, terms, name in ((out[0], g_mu, a_mu, "g_mu"), (out[1], g_var, a_var, "g_var")):
        got64, want, terms = _fold(got).numpy(), want.numpy(), terms.numpy()
        assert np.isfinite(got64).all(), (what, name)
        ulp32 = np.where(terms > 0, 2.0 ** (np.floor(np.log2(np.maximum(terms, 1e-300))) - 23), 0.0)
        bound = CL.bf16_ulp(want) + 4 * ulp32
        err = np.abs(got64 - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (what, name, float((err / bound).max()))
        assert np.abs(want).max() > 0
        if o["act"] == "relu":                                       # nothing flows where ReLU clipped: exactly +-0
            zero = (y64 == 0).numpy()
            assert zero.any() and (_fold(got.view(torch.int16).to(torch.int32) & 0x7FFF).numpy()[zero] == 0).all(), (what, name)
    return worst


@pytest.mark.parametrize("ks", [(0, 1), (2, 2), (3, 2)])
@pytest.mark.parametrize("B", [8, 24])
@pytest.mark.parametrize("hw", [(6, 5), (8, 8)])
def test_pass_vs_float64(hw, B, ks):
    """Every activation, both gradient formats, with and without the combine, moments per draw and shared: against the restatement on
    the same operands, and two calls give the same bits."""
    worst = 0.0
    for act in (None, "relu", "softplus"):
        o = _operands(hw, B, ks, act)
        for gform, combine in (("g16", False), ("g32", False), ("g16", True)):
            for shared in (False, True):
                what = f"{hw} B={B} ks={ks} act={act} {gform} combine={combine} shared={shared}"
                out = _launch(o, gform, combine, shared)
                worst = max(worst, _check_pass(o, out, gform, combine, shared, what))
                assert torch.equal(_bits(out), _bits(_launch(o, gform, combine, shared))), what
    print(f"{hw} B={B} ks={ks}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("hw", [(6, 5), (8, 8)])
def test_pass_inside_nan_filled_buffers(hw):
    """Every operand as a view inside a larger buffer filled with NaN (a plane before, a plane after): the same bits as the plain
    call -- a NaN that was read would show -- and the buffers' bytes unchanged."""
    o = _operands(hw, 8, (3, 2), "softplus")

    def inside(t):
        planes = t.shape[0] * t.shape[1]
        row = t[0, 0].numel()
        buf = torch.full((planes + 2, row), float("nan"), dtype=t.dtype, device=t.device)
        buf[1:planes + 1] = t.reshape(planes, row)
        view = buf[1:planes + 1].view(t.shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 0 and torch.equal(_bits(view), _bits(t))
        return buf, view

    for gform, combine in (("g16", True), ("g32", False)):
        names = ["y", "av", gform] + (["xo", "d2"] if combine else [])
        bufs = {n: inside(o[n]) for n in names}
        before = {n: _bits(b).clone() for n, (b, _) in bufs.items()}
        out = _launch(o, gform, combine, False, **{n: v for n, (_, v) in bufs.items()})
        assert bool(torch.isfinite(out.float()).all())
        assert torch.equal(_bits(out), _bits(_launch(o, gform, combine, False)))
        for n, (b, _) in bufs.items():
            assert torch.equal(_bits(b), before[n]), n


def test_each_draw_uses_its_own_call():
    """E = 4, call0 = 5: every draw's rows match the restatement fed ops.eps_dump for call0 + draw (the bound of test_pass_vs_float64:
    another call's noise misses it by orders of magnitude), a batch offset moves the canonical index, and a draw computed alone under its
    own call is the same bits as inside the four-draw launch."""
    from bbb_hip import ops
    for hw in ((6, 5), (8, 8)):
        o = _operands(hw, 8, (2, 2), "softplus", E=4, call0=5)
        out = _launch(o, "g16", True, False)
        _check_pass(o, out, "g16", True, False, f"E=4 {hw}")
        for e in range(4):
            alone = ops.lrt_pool_act_backward_chwn_bf16(o["g16"][e:e + 1], o["y"][e:e + 1], o["av"][e:e + 1], 2, 2, "softplus",
                                                        noise=(SEED, 5 + e, SID), combine=(o["xo"][e:e + 1], o["d2"][e:e + 1]))
            assert torch.equal(_bits(alone[:, 0]), _bits(out[:, e])), e
        wrong = ops.lrt_pool_act_backward_chwn_bf16(o["g16"], o["y"], o["av"], 2, 2, "softplus", noise=(SEED, 6, SID), combine=(o["xo"], o["d2"]))
        assert torch.equal(_bits(wrong[0]), _bits(out[0])) and not torch.equal(_bits(wrong[1]), _bits(out[1]))      # g_mu has no noise in it
        ob = _operands(hw, 8, (2, 2), "softplus", E=2, call0=5, b_offset=8)
        _check_pass(ob, _launch(ob, "g16", False, False), "g16", False, False, f"b_offset=8 {hw}")


@pytest.mark.parametrize("hw", [(6, 5), (8, 8)])
def test_padded_plane_pitch_writes_the_same_values(hw):
    """The entry with out_plane_pitch = one plane + 8 elements, into NaN-filled buffers: the planes hold the dense launch's bits and
    the pad columns are left alone."""
    from bbb_hip import _lib, rng
    o = _operands(hw, 8, (2, 2), "relu")
    dense = _launch(o, "g16", True, False)
    E, C, H, W, B = o["y"].shape
    planes, K = E * C, H * W * B
    buf = torch.full((2, planes, K + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    dev = o["y"].device
    rc = _lib.lib().bbb_lrt_pool_act_bwd_chwn_bf16(o["g16"].data_ptr(), o["y"].data_ptr(), o["av"].data_ptr(), buf[0].data_ptr(),
                                                   buf[1].data_ptr(), planes, planes, C, H, W, B, 2, 2, 1, K + 8, o["d2"].data_ptr(),
                                                   o["xo"].data_ptr(), planes, SEED, o["call0"], rng.call_dev_ptr(dev), SID, 0, 0,
                                                   _lib.cur_stream(dev))
    assert rc == 0
    assert torch.equal(_bits(buf[:, :, :K]), _bits(dense.reshape(2, planes, K)))
    assert bool(torch.isnan(buf[:, :, K:].float()).all())


def test_wrapper_refusals():
    from bbb_hip import _lib, ops
    o = _operands((6, 5), 8, (2, 2), "relu")
    n = (SEED, 7, SID)
    with pytest.raises(_lib.BBBHipError, match="needs the stored output y"):
        ops.lrt_pool_act_backward_chwn_bf16(o["g16"], None, o["av"], 2, 2, "relu", noise=n)
    with pytest.raises(_lib.BBBHipError, match="act_var must hold"):
        ops.lrt_pool_act_backward_chwn_bf16(o["g16"], o["y"], o["av"][:, :3], 2, 2, "relu", noise=n)
    with pytest.raises(_lib.BBBHipError, match="g_out must hold"):
        ops.lrt_pool_act_backward_chwn_bf16(o["g16"], o["y"], o["av"], 0, 1, "relu", noise=n)
    with pytest.raises(_lib.BBBHipError, match="two bf16 input gradients"):
        ops.lrt_pool_act_backward_chwn_bf16(o["g32"], o["y"], o["av"], 2, 2, "relu", noise=n, combine=(o["xo"], o["d2"]))
    with pytest.raises(_lib.BBBHipError):
        ops.lrt_pool_act_backward_chwn_bf16(o["g16"].double(), o["y"], o["av"], 2, 2, "relu", noise=n)


# ---- whole models ------------------------------------------------------------------------------------------------------------------
E, B, CALL0, BETA, N = 2, 8, 7, 0.1, 100.0
MSEED = 4242
# name -> (input (C, H, W), layers): ("conv", cout, kernel, stride, padding, dilation, act, pool) / ("fc", out, act); the first layers are the
# six shapes of tests/bf16_input_grad_contract.py, each followed by a second (hidden) Bayesian layer, then the classifier; M7: a
# stride-2 second convolution (LaunchConfig.bf16_strided_train)
MODELS = {
    "M1": ((3, 16, 16), [("conv", 8, 5, 2, 2, 1, "softplus", (2, 2)), ("conv", 8, 3, 1, 1, 1, "relu", None)]),
    "M2": ((3, 16, 16), [("conv", 16, 11, 4, 5, 1, "relu", None), ("conv", 8, 3, 1, 1, 1, "softplus", (2, 2))]),
    "M3": ((8, 8, 8), [("conv", 16, 3, 1, 1, 1, "relu", (2, 2)), ("conv", 8, 3, 1, 1, 1, "relu", (2, 2))]),
    "M4": ((3, 4, 4), [("fc", 24, "softplus"), ("fc", 16, "relu")]),
    "M5": ((3, 9, 13), [("conv", 12, (2, 3), (3, 2), (1, 0), (1, 2), "softplus", None), ("conv", 8, 3, 1, 1, 1, "relu", None)]),
    "M6": ((1, 16, 16), [("conv", 6, 5, 1, 0, 1, "relu", (2, 2)), ("fc", 16, "softplus")]),
    "M7": ((3, 16, 16), [("conv", 8, 3, 1, 1, 1, "softplus", None), ("conv", 8, 3, 2, 1, 1, "relu", (2, 2))]),
}


def build(name):
    from layers import BBB_LRT_Conv2d, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    from bf16_input_grad_contract import _out_hw
    (C, H, W), layers = MODELS[name]
    net = ModuleWrapper()
    flat = False
    for i, L in enumerate(layers):
        if L[0] == "conv":
            _, cout, k, st, pd, dl, act, pool = L
            conv = BBB_LRT_Conv2d(C, cout, k if isinstance(k, int) else k[0], stride=st, padding=pd, dilation=dl, bias=True,
                                  priors=P.CONFIG_PRIORS)
            if not isinstance(k, int):       # the LRT layer's constructor takes an int kernel, like the reference: rectangular taps by hand
                conv.kernel_size = tuple(k)
                conv.W_mu, conv.W_rho = nn.Parameter(torch.empty(cout, C, *k)), nn.Parameter(torch.empty(cout, C, *k))
                conv.reset_parameters()
            net.add_module(f"conv{i}", conv)
            H, W = _out_hw(H, W, k, st, pd, dl)
        else:
            _, cout, act = L
            pool = None
            if not flat:
                net.add_module(f"flatten{i}", FlattenLayer(C * H * W))
                flat = True
            net.add_module(f"fc{i}", BBB_LRT_Linear(C * H * W, cout, bias=True, priors=P.CONFIG_PRIORS))
            H = W = 1
        net.add_module(f"act{i}", nn.Softplus() if act == "softplus" else nn.ReLU())
        if pool is not None:
            net.add_module(f"pool{i}", nn.MaxPool2d(*pool))
            H, W = (H - pool[0]) // pool[1] + 1, (W - pool[0]) // pool[1] + 1
        C = cout
    if not flat:
        net.add_module("flatten", FlattenLayer(C * H * W))
    net.add_module("fc_out", BBB_LRT_Linear(C * H * W, 10, bias=True, priors=P.CONFIG_PRIORS))
    return net, MODELS[name][0]


def _node_forward(net, x, seed, call0):
    """fast_train._lrt_bf16_forward as mc_logits_autograd calls it -> (tape, logits [E, C, B], kl)."""
    from bbb_hip import ensemble, fast_train, ops
    layers = ensemble.bayesian_layers(net)
    mus, rhos, _ = fast_train._param_lists(layers, lambda t: t)
    kl, s2 = ops.kl_only(mus, rhos, layers[0].prior_mu, layers[0].prior_sigma, want_sigma=True, sigma_squared=True)
    params = []
    for li in range(len(layers)):
        params += [mus[2 * li], s2[2 * li], mus[2 * li + 1], s2[2 * li + 1]]
    tape, logits = fast_train._lrt_bf16_forward(dict(net=net, draws=E, seed=seed, call0=call0), x, params)
    return tape, logits, kl


def _g_logits(logits, y, scale):
    """d (scale * nll_loss(logmeanexp over draws of log_softmax)) / d logits in float64: the loss of all three entries."""
    lg = logits.detach().cpu().to(F64).requires_grad_(True)                   # [E, C, B]
    lo = torch.logsumexp(F.log_softmax(lg.permute(0, 2, 1), dim=2), dim=0) - np.log(lg.shape[0])
    (g,) = torch.autograd.grad(F.nll_loss(lo, y.cpu(), reduction="mean") * scale, lg)
    return g


_models = {}


def _model(name):
    """Everything the whole-model tests compare, computed once per model."""
    if name in _models:
        return _models[name]
    import layers  # noqa: F401
    from bbb_hip import ensemble, fast_train, ops, rng, train
    torch.manual_seed(11)
    net, chw = build(name)
    net = net.cuda()
    net.requires_grad_(False)
    rng.assign_stream_ids(net)
    g = torch.Generator().manual_seed(5)
    x = torch.rand((B,) + chw, generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    m = dict(net=net, x=x, y=y)
    with ops.use_config(**BOTH):
        why = fast_train.bf16_train_refusal(net, x.clone().requires_grad_(True))
        assert why is None, (name, why)                                      # (every model is admitted on the MI355X: none is dropped)
        with torch.no_grad():
            tape, logits, kl = _node_forward(net, x, MSEED, CALL0)
            ref, ref_kl = ensemble.mc_logits(net, x, E, MSEED, CALL0, precision="bf16")
        assert ensemble.stats["path"] == "chwn-bf16-lrt"
        m.update(logits=logits, inference_logits=ref.permute(0, 2, 1).contiguous(), kl=kl, inference_kl=ref_kl)
        cpu_tape = CL.tape_to_cpu(tape, MSEED, CALL0, E)
        x_b = x.to(torch.bfloat16).to(F64).cpu()
        m["want"] = {s: CL.walk_dx(cpu_tape, _g_logits(logits, y, s), x_b) for s in (N, 1.0)}

        def forward_loss():
            xg = x.clone().requires_grad_(True)
            loss, lo, kl_ = train.forward_loss(net, xg, y, E, BETA, N, seed_call=(MSEED, CALL0), precision="bf16")
            path = ensemble.stats["path"]
            loss.backward()
            return dict(dx=xg.grad.detach().clone(), kl=kl_.detach().clone(), path=path, lo=lo.detach().clone())

        def mc_forward():
            xg = x.clone().requires_grad_(True)
            rng.manual_seed(MSEED, call=CALL0)
            lo, _ = ensemble.mc_forward(net, xg, E, kl_mode="mean", precision="bf16")
            path = ensemble.stats["path"]
            F.nll_loss(lo, y).backward()
            return dict(dx=xg.grad.detach().clone(), path=path)

        def mc_logits():
            xg = x.clone().requires_grad_(True)
            lg, kl_ = ensemble.mc_logits(net, xg, E, MSEED, CALL0, precision="bf16")
            path = ensemble.stats["path"]
            F.nll_loss(P.logmeanexp(F.log_softmax(lg, dim=2).permute(1, 2, 0), 2), y).backward()
            return dict(dx=xg.grad.detach().clone(), path=path, logits=lg.detach().clone(), kl=kl_.detach().clone())

        m["forward_loss"], m["forward_loss_again"] = forward_loss(), forward_loss()
        m["mc_forward"], m["mc_logits"] = mc_forward(), mc_logits()
    xg = x.clone().requires_grad_(True)                                       # the fp32 LRT node, the same noise
    loss, _, kl32 = train.forward_loss(net, xg, y, E, BETA, N, seed_call=(MSEED, CALL0), precision="fp32")
    m["fp32_path"] = ensemble.stats["path"]
    loss.backward()
    m["fp32"] = dict(dx=xg.grad.detach().clone(), kl=kl32.detach().clone())
    m["param_grads"] = [p.grad for p in net.parameters()]
    _models[name] = m
    return m


@pytest.mark.parametrize("seed", [MSEED, 99])
@pytest.mark.parametrize("name", ["M1", "M6"])
def test_forward_is_the_inference_path_bit_for_bit(name, seed):
    from bbb_hip import ensemble, ops
    m = _model(name)
    with ops.use_config(**BOTH), torch.no_grad():
        tape, logits, kl = _node_forward(m["net"], m["x"], seed, CALL0 + 3)
        ref, ref_kl = ensemble.mc_logits(m["net"], m["x"], E, seed, CALL0 + 3, precision="bf16")
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (E, 10, B)
    assert torch.equal(_bits(logits), _bits(ref.permute(0, 2, 1).contiguous())) and torch.equal(_bits(kl), _bits(ref_kl))
    assert len(tape) == 3 and all(r["av"].dtype == torch.float32 and r["x"].dtype == torch.bfloat16 for r in tape)
    assert tape[0]["av"].shape[0] == 1 and tape[1]["av"].shape[0] == E          # the shared first layer keeps one draw's worth
    assert [r["sid"] for r in tape] == [l._stream_base + 2 for l in ensemble.bayesian_layers(m["net"])]


@pytest.mark.parametrize("name", list(MODELS))
def test_model_dx_vs_contract_and_fp32(name):
    m = _model(name)
    assert torch.equal(_bits(m["logits"]), _bits(m["inference_logits"]))
    worst = 0.0
    for entry, scale in (("forward_loss", N), ("mc_forward", 1.0), ("mc_logits", 1.0)):
        got, want = m[entry]["dx"].double().cpu().numpy(), m["want"][scale]
        assert got.shape == want.shape and np.isfinite(got).all() and np.abs(want).max() > 0
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"{name} {entry}: max |dx - contract| / max |contract| = {rel:.3e}")
        worst = max(worst, rel)
    a, b = m["forward_loss"]["dx"].double().flatten(), m["fp32"]["dx"].double().flatten()
    cos = float(a @ b / (a.norm() * b.norm()))
    print(f"{name}: worst over the entries {worst:.3e} (bound {DX_BOUND:.2e}); cosine with the fp32 LRT node's dx = {cos:.6f} (bound {COS_BOUND:.6f})")
    assert worst <= DX_BOUND, (name, worst)
    assert cos >= COS_BOUND, (name, cos)


@pytest.mark.parametrize("name", list(MODELS))
def test_model_exact_properties(name):
    m = _model(name)
    assert m["forward_loss"]["path"] == m["mc_forward"]["path"] == m["mc_logits"]["path"] == "chwn-autograd-bf16-lrt"
    assert m["fp32_path"] == "chwn-autograd"
    assert torch.equal(_bits(m["forward_loss"]["kl"]), _bits(m["fp32"]["kl"])) and torch.equal(_bits(m["mc_logits"]["kl"]), _bits(m["fp32"]["kl"]))
    assert torch.equal(_bits(m["kl"]), _bits(m["inference_kl"]))
    assert torch.equal(_bits(m["forward_loss"]["dx"]), _bits(m["forward_loss_again"]["dx"]))         # two identical calls: bitwise
    assert torch.equal(_bits(m["mc_logits"]["logits"].permute(0, 2, 1).contiguous()), _bits(m["inference_logits"]))
    assert all(g is None for g in m["param_grads"])                                                  # no parameter has a .grad
    assert m["forward_loss"]["dx"].dtype == torch.float32 and m["forward_loss"]["dx"].shape == m["x"].shape


def test_refusals_and_the_switch_off():
    from bbb_hip import _lib, ensemble, ops, train
    m = _model("M1")
    net, x, y = m["net"], m["x"], m["y"]
    xg = lambda: x.clone().requires_grad_(True)
    # the switch off: exactly what these calls raise today
    for kw in ({}, dict(bf16_lrt=True)):
        with ops.use_config(**kw):
            with pytest.raises(_lib.BBBHipError, match="bf16 training covers inputs that do not require a gradient"):
                train.forward_loss(net, xg(), y, E, BETA, N, precision="bf16")
    with pytest.raises(_lib.BBBHipError, match="LRT models run in bf16 only under LaunchConfig.bf16_lrt"):
        ensemble.mc_logits(net, xg(), E, MSEED, CALL0, precision="bf16")
    with ops.use_config(bf16_lrt_input_grad=True):                            # without bf16_lrt: the message naming bf16_lrt
        with pytest.raises(_lib.BBBHipError, match="LRT models run in bf16 only under LaunchConfig.bf16_lrt"):
            ensemble.mc_logits(net, xg(), E, MSEED, CALL0, precision="bf16")
        with pytest.raises(_lib.BBBHipError, match="LRT models run in bf16 only under LaunchConfig.bf16_lrt"):
            train.forward_loss(net, xg(), y, E, BETA, N, precision="bf16")
    with ops.use_config(**BOTH):
        # trainable parameters, through every entry
        net.requires_grad_(True)
        try:
            for call in (lambda: train.forward_loss(net, xg(), y, E, BETA, N, precision="bf16"),
                         lambda: ensemble.mc_forward(net, xg(), E, precision="bf16"),
                         lambda: ensemble.mc_logits(net, xg(), E, MSEED, CALL0, precision="bf16"),
                         lambda: train.forward_loss(net, x, y, E, BETA, N, precision="bf16")):
                with pytest.raises(_lib.BBBHipError, match=r"input gradients only.*net\.requires_grad_\(False\).*precision='fp32'"):
                    call()
        finally:
            net.requires_grad_(False)
        # what the node does not cover is refused under the new switch's name, never computed some other way
        for kw in (dict(units=(2, 0, 2)), dict(groups=2), dict(b_offset=8), dict(share=(2, 0)), dict(timers={})):
            with pytest.raises(_lib.BBBHipError, match="bf16_lrt_input_grad"):
                ensemble._local_lse(net, xg(), E, MSEED, CALL0, E, precision="bf16", **kw)
        with pytest.raises(_lib.BBBHipError, match="bf16 training covers a batch size that is a multiple of 8"):
            ensemble.mc_forward(net, torch.cat([x, x[:4]]).requires_grad_(True), E, precision="bf16")
