"""CPU-only checks of the strided later layers on the training fast path: what fast_train._train_path_static admits and still
refuses, the bf16 refusal's reason, the argument validation of bbb_conv2d_chwn_dgrad (it happens before any launch, so the error
codes come back on a GPU-less host), and the transposed launch's tap plan (ops.dgrad_tap_plan, the host restatement of
csrc/pconv_body.cuh's tr_axis) against torch.nn.grad.conv2d_input in float64."""
import ctypes
import itertools
import os
import subprocess

import pytest
import torch
import torch.nn as nn
from torch.nn.grad import conv2d_input

import ref_port_torch as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def _net(kind, convs, hw=(16, 16), cin=3, act=nn.Softplus, mixed_last=False, bias=True):
    """convs: (cout, k, stride, padding, dilation, pool | None)."""
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    Conv, Linear = (BBB_Conv2d, BBB_Linear) if kind == "bbb" else (BBB_LRT_Conv2d, BBB_LRT_Linear)
    net = ModuleWrapper()
    H, W = hw
    for i, (cout, k, st, pd, dl, pool) in enumerate(convs):
        net.add_module(f"conv{i}", Conv(cin, cout, k, stride=st, padding=pd, dilation=dl, bias=bias, priors=P.CONFIG_PRIORS))
        net.add_module(f"act{i}", act())
        H, W = (H + 2 * pd - dl * (k - 1) - 1) // st + 1, (W + 2 * pd - dl * (k - 1) - 1) // st + 1
        if pool is not None:
            net.add_module(f"pool{i}", nn.MaxPool2d(*pool))
            H, W = (H - pool[0]) // pool[1] + 1, (W - pool[0]) // pool[1] + 1
        cin = cout
    net.add_module("flatten", FlattenLayer(cin * H * W))
    if mixed_last:
        Linear = BBB_LRT_Linear if kind == "bbb" else BBB_Linear
    net.add_module("fc", Linear(cin * H * W, 10, bias=True, priors=P.CONFIG_PRIORS))
    return net


class _X:
    """What _train_path_static reads of the batch: its shape."""
    shape = (8, 3, 16, 16)


STRIDED = {
    "second_s2": [(8, 3, 1, 1, 1, None), (8, 3, 2, 1, 1, None)],
    "third_s2_after_pool": [(8, 3, 1, 1, 1, (2, 2)), (8, 3, 1, 1, 1, None), (12, 3, 2, 0, 1, None)],
    "second_1x1_s2": [(8, 3, 1, 1, 1, None), (16, 1, 2, 0, 1, None)],
    "second_s21": [(8, 3, 1, 1, 1, None), (8, 3, (2, 1), 1, 1, None)],
    "second_s2_dil2": [(8, 3, 2, 1, 1, None), (8, 3, 2, 2, 2, None)],
    "second_s3_pool": [(8, 3, 1, 1, 1, None), (8, 3, 3, 1, 1, (2, 1))],
}


def _net2(kind, convs, **kw):
    # (per-axis strides: _net's size arithmetic takes scalars, so route tuple strides through torch itself)
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    if all(isinstance(c[2], int) for c in convs):
        return _net(kind, convs, **kw)
    Conv, Linear = (BBB_Conv2d, BBB_Linear) if kind == "bbb" else (BBB_LRT_Conv2d, BBB_LRT_Linear)
    net, cin = ModuleWrapper(), 3
    probe = torch.zeros(1, 3, 16, 16)
    for i, (cout, k, st, pd, dl, pool) in enumerate(convs):
        net.add_module(f"conv{i}", Conv(cin, cout, k, stride=st, padding=pd, dilation=dl, bias=True, priors=P.CONFIG_PRIORS))
        net.add_module(f"act{i}", nn.Softplus())
        probe = nn.functional.conv2d(probe, torch.zeros(cout, cin, k, k), None, st, pd, dl)
        cin = cout
    feat = probe.numel()
    net.add_module("flatten", FlattenLayer(feat))
    net.add_module("fc", Linear(feat, 10, bias=True, priors=P.CONFIG_PRIORS))
    return net


@pytest.mark.parametrize("kind", ["bbb", "lrt"])
@pytest.mark.parametrize("name", list(STRIDED))
def test_static_gate_admits_strided_later_convolutions(name, kind):
    from bbb_hip import fast_train
    assert fast_train._train_path_static(_net2(kind, STRIDED[name]), _X) == kind


def test_static_gate_still_refuses():
    from bbb_hip import fast_train
    ok = [(8, 3, 1, 1, 1, None), (8, 3, 2, 1, 1, None)]
    assert fast_train._train_path_static(_net("bbb", ok), _X) == "bbb"
    # padding beyond the kernel reach (p > d (k - 1)), in a strided later layer and in a stride-1 one
    assert fast_train._train_path_static(_net("bbb", [(8, 3, 1, 1, 1, None), (8, 3, 2, 3, 1, None)]), _X) is None
    assert fast_train._train_path_static(_net("lrt", [(8, 3, 1, 1, 1, None), (8, 1, 2, 1, 1, None)]), _X) is None
    assert fast_train._train_path_static(_net("bbb", [(8, 3, 1, 1, 1, None), (8, 3, 1, 3, 1, None)]), _X) is None
    # mixed kinds, a layer without bias, a stand-alone activation, a channel count that is no multiple of 4 behind the first layer
    assert fast_train._train_path_static(_net("bbb", ok, mixed_last=True), _X) is None
    assert fast_train._train_path_static(_net("bbb", ok, bias=False), _X) is None
    net = _net("bbb", ok)
    mods = dict(net.named_children())
    from layers import ModuleWrapper
    twice = ModuleWrapper()
    for n, m in mods.items():
        twice.add_module(n, m)
        if n == "act1":
            twice.add_module("act1b", nn.ReLU())
    assert fast_train._train_path_static(twice, _X) is None
    # a padded pool behind a strided layer
    net = _net("bbb", ok)
    padded = ModuleWrapper()
    for n, m in net.named_children():
        padded.add_module(n, m)
        if n == "act1":
            padded.add_module("pool1", nn.MaxPool2d(2, 2, padding=1))
    assert fast_train._train_path_static(padded, _X) is None


def test_bf16_refusal_names_strided_later_layers(monkeypatch):
    from bbb_hip import fast_train
    net = _net("bbb", STRIDED["second_s2"])
    x = torch.zeros(8, 3, 16, 16)
    # (no device here: stand in for the checks that need one; the reason under test comes from the model alone)
    monkeypatch.setattr(fast_train, "train_path_ok", lambda n, t: fast_train._train_path_static(n, t))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    why = fast_train.bf16_train_refusal(net, x)
    assert why is not None and "stride-1 convolutions after the first layer" in why
    first_only = _net("bbb", [(8, 3, 2, 1, 1, None), (8, 3, 1, 1, 1, None)])
    assert fast_train.bf16_train_refusal(first_only, x) is None          # a strided FIRST layer stays covered
    assert fast_train._strided_later_conv(net) and not fast_train._strided_later_conv(first_only)


def _desc(_lib, **kw):
    # the stride-1 launch of a 3 x 3 / stride 2 / padding 1 layer's gradient: g [8][4 x 4], dx [4][8 x 8] (pad = 2 - 1)
    d = _lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = 4, 8, 4, 4, 4, 3, 3
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = d.draws = 1
    d.pad_h = d.pad_w = 1
    d.x_draw_stride, d.w_draw_stride = 8 * 4 * 4 * 4, 4 * 8 * 9
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_dgrad_entry_is_exported_and_validates_without_a_gpu(lib):
    assert "bbb_conv2d_chwn_dgrad" in lib.EXPORTS
    h = lib.lib()
    f = h.bbb_conv2d_chwn_dgrad
    assert h.bbb_abi_version() == 13
    ok = ctypes.byref(_desc(lib))
    assert f(None, 64, 64, 64, 2, 2, 8, 8, None) == -1                                # no descriptor
    for args in ((None, 64, 64), (64, None, 64), (64, 64, None)):
        assert f(ok, *args, 2, 2, 8, 8, None) == -1                                   # a missing operand
    assert f(ok, 64, 64, 64, 1, 1, 8, 8, None) == -1                                  # stride 1 is the forward launch's job
    assert f(ok, 64, 64, 64, 0, 2, 8, 8, None) == -1
    assert f(ok, 64, 64, 64, 2, 2, 0, 8, None) == -1
    for field, v in (("batch", 0), ("cin", 0), ("h", -1), ("kh", 0), ("stride_w", 2), ("pad_h", -1), ("dil_w", 0), ("draws", 0),
                     ("act", 1), ("pool", 1), ("w_tap_major", 1), ("unit_div", 2), ("x_unit_div", 2), ("w_row_pitch", 80)):
        assert f(ctypes.byref(_desc(lib, **{field: v})), 64, 64, 64, 2, 2, 8, 8, None) == -1, field
    assert f(ok, 66, 64, 64, 2, 2, 8, 8, None) == -2                                  # misaligned pointers
    assert f(ok, 64, 64, 72, 2, 2, 8, 8, None) == -2
    assert f(ok, 64, 66, 64, 2, 2, 8, 8, None) == -2
    assert f(ctypes.byref(_desc(lib, batch=6)), 64, 64, 64, 2, 2, 8, 8, None) == -3   # batch % 4
    assert f(ctypes.byref(_desc(lib, pad_h=3)), 64, 64, 64, 2, 2, 8, 8, None) == -3   # the layer's padding would be negative
    assert f(ok, 64, 64, 64, 2, 2, 9, 8, None) == -3                                  # a 9-row input gives 5 output rows, not 4
    assert f(ok, 64, 64, 64, 2, 2, 6, 8, None) == -3
    assert f(ok, 64, 64, 64, 3, 2, 8, 8, None) == -3                                  # stride 3 on 8 rows gives 3


def _dgrad_by_plan(g, w, H, W, s, p, d):
    """dx from the tap plan alone (float64): g [B, Cout, Ho, Wo], w [Cout, Cin, kh, kw]; also the (pixel, tap) pairs visited."""
    from bbb_hip import ops
    B, Cout, Ho, Wo = g.shape
    Cin, kh, kw = w.shape[1:]
    wf = w.flip(2, 3)                                                                  # wf[co][ci][r'][q'] = w[co][ci][k-1-r'][k-1-q']
    dx = torch.zeros(B, Cin, H, W, dtype=torch.float64)
    pairs = 0
    for ih in range(H):
        rows = ops.dgrad_tap_plan(ih, Ho, kh, s[0], p[0], d[0])
        for iw in range(W):
            cols = ops.dgrad_tap_plan(iw, Wo, kw, s[1], p[1], d[1])
            pairs += len(rows) * len(cols)
            for r, oh in rows:
                for q, ow in cols:
                    dx[:, :, ih, iw] += g[:, :, oh, ow] @ wf[:, :, r, q]
    return dx, pairs


def _plan_geometries():
    rs = torch.Generator().manual_seed(5)
    out = []
    for (sh, sw), (dh, dw), (kh, kw) in itertools.product([(2, 2), (3, 3), (2, 1), (1, 2), (3, 2), (4, 4)], [(1, 1), (2, 2), (3, 2), (2, 3)],
                                                          [(1, 1), (2, 2), (3, 3), (5, 4), (2, 5)]):
        for ph, pw in {(0, 0), (dh * (kh - 1) // 2, dw * (kw - 1) // 2), (dh * (kh - 1), dw * (kw - 1))}:
            H, W = (int(v) for v in torch.randint(3, 14, (2,), generator=rs))
            if H + 2 * ph - dh * (kh - 1) - 1 < 0 or W + 2 * pw - dw * (kw - 1) - 1 < 0:
                continue
            out.append((H, W, kh, kw, (sh, sw), (ph, pw), (dh, dw)))
    return out


def test_tap_plan_matches_conv2d_input_bit_for_bit():
    """Small-integer operands: every sum is exact, so the plan's dx must EQUAL torch's; the pairs it visits must be the forward's
    in-bounds (pixel, tap) pairs (no inserted zero, no padding tap), and pixels no tap reaches stay zero."""
    gen = torch.Generator().manual_seed(11)
    geoms = _plan_geometries()
    assert len(geoms) > 250
    unreached = 0
    for H, W, kh, kw, s, p, d in geoms:
        Ho, Wo = (H + 2 * p[0] - d[0] * (kh - 1) - 1) // s[0] + 1, (W + 2 * p[1] - d[1] * (kw - 1) - 1) // s[1] + 1
        g = torch.randint(-3, 4, (2, 3, Ho, Wo), generator=gen).double()
        w = torch.randint(-3, 4, (3, 2, kh, kw), generator=gen).double()
        want = conv2d_input((2, 2, H, W), w, g, stride=s, padding=p, dilation=d)
        got, pairs = _dgrad_by_plan(g, w, H, W, s, p, d)
        assert torch.equal(got, want), (H, W, kh, kw, s, p, d)
        fwd_pairs = sum(1 for oh in range(Ho) for r in range(kh) if 0 <= oh * s[0] - p[0] + r * d[0] < H) * \
            sum(1 for ow in range(Wo) for q in range(kw) if 0 <= ow * s[1] - p[1] + q * d[1] < W)
        assert pairs == fwd_pairs, (H, W, kh, kw, s, p, d)
        from bbb_hip import ops
        unreached += sum(1 for ih in range(H) if not ops.dgrad_tap_plan(ih, Ho, kh, s[0], p[0], d[0]))
    assert unreached > 0                               # the sweep contains rows that receive nothing
