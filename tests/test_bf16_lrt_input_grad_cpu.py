"""CPU-only checks of bf16 input gradients for LRT models (LaunchConfig.bf16_lrt_input_grad): the switch, the gate
(fast_train.bf16_train_refusal: admitted only with bf16_lrt, the switch and frozen parameters; with the switch off, today's strings),
the new entry of the C ABI and its argument validation (it happens before any launch, so the codes come back on a GPU-less host), and
the float64 restatement (tests/bf16_lrt_input_grad_contract.py) against torch autograd: the pass's formulas, and the whole walk."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16_lrt_input_grad_contract as CL
import ref_port_torch as P
from test_bf16_input_grad_cpu import _no_device
from test_strided_train_cpu import _net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
EINVAL, EALIGN, ESHAPE = -1, -2, -3
PTR = 64          # a dummy operand pointer: non-null, 16-byte aligned, never dereferenced (every call below is refused before a launch)
F64 = torch.float64
CONVS = [(8, 3, 1, 1, 1, (2, 2)), (8, 3, 1, 1, 1, None)]
BOTH = dict(bf16_lrt=True, bf16_lrt_input_grad=True)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def _frozen(net):
    net.requires_grad_(False)
    return net


def _xg(B=8):
    return torch.zeros(B, 3, 16, 16, requires_grad=True)


# ---- the switch ----
def test_config_field():
    from bbb_hip import ops
    assert "bf16_lrt_input_grad" in ops.LaunchConfig.FIELDS and ops.LaunchConfig().bf16_lrt_input_grad is False
    on = ops.LaunchConfig(bf16_lrt_input_grad=True)
    assert on.key() != ops.LaunchConfig().key() and len(on.key()) == len(ops.LaunchConfig.FIELDS)
    assert on.copy().bf16_lrt_input_grad is True and on.copy(bf16_lrt_input_grad=False).bf16_lrt_input_grad is False
    assert on.bf16_lrt is False and on.bf16_input_grad is False                  # it sets nothing else
    assert ops.current_config().bf16_lrt_input_grad is False
    with ops.use_config(bf16_lrt_input_grad=True):
        assert ops.current_config().bf16_lrt_input_grad is True
        with ops.use_config(bf16_lrt=True, bf16_avgpool=True):
            cur = ops.current_config()
            assert cur.bf16_lrt_input_grad is True and cur.bf16_lrt is True and cur.bf16_input_grad is False
        assert ops.current_config().bf16_lrt is False
    assert ops.current_config().bf16_lrt_input_grad is False
    assert "bf16_lrt_input_grad" in ops.LaunchConfig.__doc__ and "bf16_lrt_input_grad=True" in repr(on)


# ---- the gate ----
def test_admitted_only_with_both_switches_and_frozen_parameters(monkeypatch):
    from bbb_hip import fast_train, ops
    _no_device(monkeypatch)
    net, xg = _frozen(_net("lrt", CONVS)), _xg()
    with ops.use_config(**BOTH):
        assert fast_train.bf16_train_refusal(net, xg) is None
        with ops.use_config(bf16_input_grad=True, bf16_avgpool=True, bf16_strided_train=True):          # it nests with the other switches
            assert fast_train.bf16_train_refusal(net, xg) is None
    assert fast_train.bf16_train_refusal(net, xg) is not None                                           # ... and only inside it
    with ops.use_config(bf16_lrt_input_grad=True):                   # without bf16_lrt: the message that names bf16_lrt
        why = fast_train.bf16_train_refusal(net, xg)
        assert why is not None and "LaunchConfig.bf16_lrt " in why and "ops.use_config(bf16_lrt=True)" in why
    with ops.use_config(bf16_lrt=True):                              # without the new switch: what it always was
        assert "do not require a gradient" in fast_train.bf16_train_refusal(net, xg)
    with ops.use_config(bf16_lrt=True, bf16_input_grad=True):       # bf16_input_grad does not stand in for it
        assert "local-reparameterisation layers have no bf16 mode" in fast_train.bf16_train_refusal(net, xg)


def test_each_refusal_names_what_it_should(monkeypatch):
    from bbb_hip import fast_train, ops
    from layers import BBB_LRT_Conv2d, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    _no_device(monkeypatch)
    with ops.use_config(**BOTH):
        xg = _xg()
        # trainable parameters: all of them, or one
        why = fast_train.bf16_train_refusal(_net("lrt", CONVS), xg)
        assert "input gradients only" in why and "net.requires_grad_(False)" in why and "precision='fp32'" in why
        one = _frozen(_net("lrt", CONVS))
        next(iter(one.parameters())).requires_grad_(True)
        assert "input gradients only" in fast_train.bf16_train_refusal(one, xg)
        # an average pool, with and without bf16_avgpool: a line of its own
        avg = ModuleWrapper()
        avg.add_module("conv0", BBB_LRT_Conv2d(3, 8, 3, stride=1, padding=1, bias=True, priors=P.CONFIG_PRIORS))
        avg.add_module("act0", nn.Softplus())
        avg.add_module("pool0", nn.AvgPool2d(2, 2))
        avg.add_module("flatten", FlattenLayer(8 * 8 * 8))
        avg.add_module("fc", BBB_LRT_Linear(8 * 8 * 8, 10, bias=True, priors=P.CONFIG_PRIORS))
        _frozen(avg)
        for kw in ({}, dict(bf16_avgpool=True)):
            with ops.use_config(**kw):
                why = fast_train.bf16_train_refusal(avg, xg)
                assert "average" in why and "LRT pooling / activation backward" in why and "bf16 planes" in why
        # a strided later layer: today's line, unchanged, and bf16_strided_train admits it
        strided = _frozen(_net("lrt", [(8, 3, 1, 1, 1, None), (8, 3, 2, 1, 1, None)]))
        why = fast_train.bf16_train_refusal(strided, xg)
        with ops.use_config(bf16_lrt=False, bf16_lrt_input_grad=False):
            assert why == fast_train.bf16_train_refusal(_net("bbb", [(8, 3, 1, 1, 1, None), (8, 3, 2, 1, 1, None)]), torch.zeros(8, 3, 16, 16))
        assert "bf16_strided_train" in why and "stride-1 convolutions after the first layer" in why
        with ops.use_config(bf16_strided_train=True):
            assert fast_train.bf16_train_refusal(strided, xg) is None
        # B = 12, eps replay, mixed models, an input that needs no gradient
        assert "multiple of 8" in fast_train.bf16_train_refusal(_frozen(_net("lrt", CONVS)), _xg(12))
        replay = _frozen(_net("lrt", CONVS))
        next(m for m in replay.modules() if hasattr(m, "eps_source")).eps_source = object()
        assert fast_train.bf16_train_refusal(replay, xg) == "no eps replay"
        assert "ALL local-reparameterisation layers" in fast_train.bf16_train_refusal(_frozen(_net("lrt", CONVS, mixed_last=True)), xg)
        assert "requires a gradient" in fast_train.bf16_train_refusal(_frozen(_net("lrt", CONVS)), torch.zeros(8, 3, 16, 16))
        assert "4-d fp32 CUDA batch" in fast_train.bf16_train_refusal(_frozen(_net("lrt", CONVS)), torch.zeros(8, 3, 16, 16, dtype=torch.float64))
        # BBB models do not see the switch
        assert "LaunchConfig.bf16_input_grad" in fast_train.bf16_train_refusal(_net("bbb", CONVS), xg)
        assert fast_train.bf16_train_refusal(_net("bbb", CONVS), torch.zeros(8, 3, 16, 16)) is None


def test_switch_off_returns_todays_strings(monkeypatch):
    """The substrings the existing tests pin, on LRT nets, under every combination of the OTHER switches."""
    from bbb_hip import fast_train, ops
    _no_device(monkeypatch)
    for kw in ({}, dict(bf16_lrt=True)):
        with ops.use_config(**kw):
            lrt = _net("lrt", CONVS)
            assert "local-reparameterisation layers have no bf16 mode" in fast_train.bf16_train_refusal(lrt, torch.zeros(8, 3, 16, 16))
            why = fast_train.bf16_train_refusal(lrt, _xg())
            assert "do not require a gradient" in why and "LaunchConfig.bf16_input_grad" in why and "ops.use_config(bf16_input_grad=True)" in why
            assert why == fast_train.bf16_train_refusal(_frozen(_net("lrt", CONVS)), _xg())
            with ops.use_config(bf16_input_grad=True):
                assert "local-reparameterisation layers have no bf16 mode" in fast_train.bf16_train_refusal(lrt, _xg())
                replay = _net("lrt", CONVS)
                next(m for m in replay.modules() if hasattr(m, "eps_source")).eps_source = object()
                assert fast_train.bf16_train_refusal(replay, _xg()) == "no eps replay"
            assert "a model and input on the batch-innermost training path" in \
                fast_train.bf16_train_refusal(_net("lrt", CONVS, mixed_last=True), torch.zeros(8, 3, 16, 16))


def test_entry_points_learn_the_condition():
    from bbb_hip import ensemble, ops
    net, xg = _frozen(_net("lrt", CONVS)), _xg()
    assert not ensemble._bf16_x_grad("bf16", xg, net)
    with ops.use_config(**BOTH):
        assert ensemble._bf16_x_grad("bf16", xg, net) and ensemble._bf16_lrt_x_grad("bf16", xg, net)
        assert not ensemble._bf16_x_grad("bf16", xg) and not ensemble._bf16_x_grad("fp32", xg, net)
        assert not ensemble._bf16_x_grad("bf16", torch.zeros(8, 3, 16, 16), net)
        assert not ensemble._bf16_x_grad("bf16", xg, _net("bbb", CONVS))
        with torch.no_grad():
            assert not ensemble._bf16_x_grad("bf16", xg, net)
        # what _BF16_X_GRAD_ONLY excludes is excluded here too, under the new switch's name
        with pytest.raises(Exception, match="LaunchConfig.bf16_lrt_input_grad.*batch-innermost autograd node only"):
            ensemble._bf16_x_grad_logits(net, xg, 2, 1, 0, plain=False, lrt=True)
    with ops.use_config(bf16_lrt_input_grad=True):
        assert not ensemble._bf16_x_grad("bf16", xg, net)            # not without bf16_lrt
    with pytest.raises(Exception, match=r"LaunchConfig.bf16_input_grad\)"):
        ensemble._bf16_x_grad_logits(net, xg, 2, 1, 0, plain=False)


# ---- the C ABI ----
def test_entry_is_exported_and_declared(lib):
    h = lib.lib()
    assert h.bbb_abi_version() == 13 and lib.ABI_VERSION == 13                    # additive: the version stays
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = fh.read()
    name = "bbb_lrt_pool_act_bwd_chwn_bf16"
    assert name in lib.EXPORTS and hasattr(h, name) and f"int {name}(" in header
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        assert name in fh.read()


def _rc(lib, **kw):
    a = dict(g_out=PTR, y=PTR, act_var=PTR, g_mu=PTR, g_var=PTR, planes=16, mom=16, channels=8, h=6, w=5, batch=8, k=2, s=2, act=1, pitch=0,
             g2=None, xo=None, x_planes=0, seed=7, call0=5, call_dev=None, sid=3, b_off=0, flags=0)
    a.update(kw)
    rc = lib.lib().bbb_lrt_pool_act_bwd_chwn_bf16(a["g_out"], a["y"], a["act_var"], a["g_mu"], a["g_var"], a["planes"], a["mom"], a["channels"],
                                                  a["h"], a["w"], a["batch"], a["k"], a["s"], a["act"], a["pitch"], a["g2"], a["xo"],
                                                  a["x_planes"], a["seed"], a["call0"], a["call_dev"], a["sid"], a["b_off"], a["flags"], None)
    assert rc != 0, "this helper is for refusals: an accepted call would launch"
    return rc


def test_every_check_refuses_before_a_launch(lib):
    # BBB_EINVAL: null operands (y only where it is needed), non-positive sizes, the counts, the flags, half a combine
    for kw in (dict(g_out=None), dict(y=None), dict(act_var=None), dict(g_mu=None), dict(g_var=None), dict(y=None, k=0, act=2),
               dict(planes=0), dict(planes=-16), dict(h=0), dict(w=-1), dict(batch=0), dict(batch=-8), dict(k=-1), dict(s=0), dict(channels=0),
               dict(mom=0), dict(mom=-16), dict(channels=3), dict(mom=12), dict(mom=4), dict(act=3), dict(act=-1), dict(flags=2),
               dict(flags=1 << 31), dict(b_off=-1), dict(g2=PTR), dict(xo=PTR), dict(g2=PTR, xo=PTR, x_planes=0),
               dict(g2=PTR, xo=PTR, x_planes=5), dict(g2=PTR, xo=PTR, x_planes=16, flags=1), dict(pitch=6 * 5 * 8 - 8), dict(pitch=6 * 5 * 8 + 4)):
        assert _rc(lib, **kw) == EINVAL, kw
    # BBB_EINVAL wins over BBB_ESHAPE
    assert _rc(lib, batch=12, g_out=None) == EINVAL
    # BBB_ESHAPE: batch % 8 != 0, a window larger than the map
    for kw in (dict(batch=12), dict(batch=4), dict(batch=20, k=0, act=0, y=None), dict(k=7), dict(h=1, w=1, k=3)):
        assert _rc(lib, **kw) == ESHAPE, kw
    # BBB_EALIGN: every operand
    for name in ("g_out", "y", "act_var", "g_mu", "g_var"):
        assert _rc(lib, **{name: 72}) == EALIGN, name
    assert _rc(lib, g2=72, xo=PTR, x_planes=16) == EALIGN and _rc(lib, g2=PTR, xo=68, x_planes=8) == EALIGN


# ---- the restatement: its formulas are torch autograd's ----
@pytest.mark.parametrize("act", [None, "relu", "softplus"])
@pytest.mark.parametrize("ks", [(0, 1), (2, 2), (3, 2)])
def test_pass_without_roundings_is_autograd(act, ks):
    g = torch.Generator().manual_seed(11)
    N, C, H, W = 3, 4, 6, 5
    k, s = ks
    mu = torch.randn(N, C, H, W, dtype=F64, generator=g).requires_grad_(True)           # (random: no ties)
    var = (0.05 + torch.rand(N, C, H, W, dtype=F64, generator=g)).requires_grad_(True)
    eps = torch.randn(N, C, H, W, dtype=F64, generator=g)
    v = mu + torch.sqrt(var) * eps
    y = v if act is None else F.relu(v) if act == "relu" else F.softplus(v)
    out = F.max_pool2d(y, k, s) if k else y
    d1 = torch.randn(out.shape, dtype=F64, generator=g)
    d2, xo = torch.randn(out.shape, dtype=F64, generator=g), out.detach()
    for comb in (None, (xo, d2)):
        gin = d1 if comb is None else d1 + 2.0 * xo * d2
        want_mu, want_var = torch.autograd.grad(out, (mu, var), gin, retain_graph=True)
        g_mu, g_var, a_mu, a_var = CL.lrt_pass(d1, y.detach() if (act or k) else None, var.detach(), eps, k, s, act, combine=comb)
        assert want_mu.abs().max() > 0 and want_var.abs().max() > 0
        assert (g_mu - want_mu).abs().max() <= 1e-12 * want_mu.abs().max()
        assert (g_var - want_var).abs().max() <= 1e-12 * want_var.abs().max()
        assert (a_mu >= g_mu.abs() * (1 - 1e-12)).all() and (a_var >= g_var.abs() * (1 - 1e-12)).all()
        if comb is None and k <= s:                                   # one term per element: nothing can cancel
            assert (a_mu - g_mu.abs()).abs().max() <= 1e-12 * a_mu.max()


def test_bf16_ulp_and_rows():
    assert CL.bf16_ulp(1.0) == 2.0 ** -7 and CL.bf16_ulp(-1.99) == 2.0 ** -7 and CL.bf16_ulp(2.0) == 2.0 ** -6 and CL.bf16_ulp(0.0) == 2.0 ** -133
    w = torch.arange(2 * 8 * 3 * 3, dtype=torch.float32).reshape(2, 8, 3, 3)
    plain = torch.zeros(2, 72)
    plain[:, :72] = w.reshape(2, 72)
    tapm = w.permute(0, 2, 3, 1).reshape(2, 72)
    assert torch.equal(CL.rows_to_weight(plain, (2, 8, 3, 3), False), w.to(F64))
    assert torch.equal(CL.rows_to_weight(tapm, (2, 8, 3, 3), True), w.to(F64))


def _cpu_layers(gen):
    r = lambda *s: torch.randn(*s, dtype=F64, generator=gen)
    v = lambda *s: 0.01 + 0.05 * torch.rand(*s, dtype=F64, generator=gen)
    return [dict(kind="conv", w_mu=0.3 * r(8, 3, 5, 5), w_var=v(8, 3, 5, 5), b_mu=0.1 * r(8), b_var=v(8), geom=(2, 2, 1), act="softplus", pool=(2, 2)),
            dict(kind="conv", w_mu=0.3 * r(8, 8, 3, 3), w_var=v(8, 8, 3, 3), b_mu=0.1 * r(8), b_var=v(8), geom=((2, 1), 1, 1), act="relu", pool=(3, 2)),
            dict(kind="fc", w_mu=0.3 * r(10, 8, 1, 1), w_var=v(10, 8, 1, 1), b_mu=0.1 * r(10), b_var=v(10), geom=(1, 0, 1), act=None, pool=None)]


def test_walk_without_roundings_is_autograd():
    gen = torch.Generator().manual_seed(5)
    layers = _cpu_layers(gen)
    E, B = 2, 4
    x = torch.rand(B, 3, 20, 16, dtype=F64, generator=gen).requires_grad_(True)
    shapes = [(B, 8, 10, 8), (B, 8, 3, 4), (B, 10, 1, 1)]
    eps = [[torch.randn(sh, dtype=F64, generator=gen) for sh in shapes] for _ in range(E)]
    tape, logits = CL.cpu_forward(layers, x, eps)
    assert tuple(logits.shape) == (E, 10, B)
    lo = torch.logsumexp(F.log_softmax(logits.permute(0, 2, 1), dim=2), dim=0) - np.log(E)
    loss = F.nll_loss(lo, torch.tensor([1, 3, 5, 7]), reduction="mean") * 100.0
    g_logits, want = torch.autograd.grad(loss, (logits, x))
    dx = CL.walk_dx(tape, g_logits, x.detach(), rounding=False)
    assert dx.shape == tuple(x.shape) and want.abs().max() > 0
    assert np.abs(dx - want.numpy()).max() <= 1e-11 * want.abs().max().item()
    # ... and with the four rounding points it is another set of numbers close to it (8 significant bits per stored gradient)
    dxr = CL.walk_dx(tape, g_logits, x.detach())
    rel = np.abs(dxr - want.numpy()).max() / want.abs().max().item()
    assert 0 < rel < 4e-2
