"""CPU-only checks of bf16 training behind strided layers (LaunchConfig.bf16_strided_train): the gate (fast_train.bf16_train_refusal
with the switch off and on), the configuration field, the argument validation of bbb_conv2d_chwn_bf16_dgrad (it happens before any
launch, so the error codes come back on a GPU-less host), the host restatement of its form selection (ops.bf16_dgrad_form), and what
the fixed case list of tests/test_gpu_bf16_strided_train.py reaches through it."""
import ctypes
import os
import subprocess

import pytest
import torch

from test_strided_train_cpu import STRIDED, _net, _net2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def _no_device(monkeypatch):
    # (no device here: stand in for the checks that need one; the reasons under test come from the model, the batch and the switch)
    from bbb_hip import fast_train
    monkeypatch.setattr(fast_train, "train_path_ok", lambda n, t: fast_train._train_path_static(n, t))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))


def test_config_field():
    from bbb_hip import ops
    cfg = ops.LaunchConfig()
    assert cfg.bf16_strided_train is False and "bf16_strided_train" in ops.LaunchConfig.FIELDS
    on = cfg.copy(bf16_strided_train=True)
    assert on.bf16_strided_train is True and on.key() != cfg.key() and len(on.key()) == len(ops.LaunchConfig.FIELDS)
    with ops.use_config(bf16_strided_train=True) as c:
        assert c.bf16_strided_train and ops.current_config().bf16_strided_train
    assert ops.current_config().bf16_strided_train is False
    assert "bf16_strided_train" in ops.LaunchConfig.__doc__ and "bf16_strided_train" in repr(on)


@pytest.mark.parametrize("name", list(STRIDED))
def test_gate_follows_the_switch(name, monkeypatch):
    from bbb_hip import fast_train, ops
    _no_device(monkeypatch)
    net = _net2("bbb", STRIDED[name])
    x = torch.zeros(8, 3, 16, 16)
    why = fast_train.bf16_train_refusal(net, x)
    assert why is not None and "stride-1 convolutions after the first layer" in why and "bf16_strided_train" in why
    with ops.use_config(bf16_strided_train=True):
        assert fast_train.bf16_train_refusal(net, x) is None
    assert fast_train.bf16_train_refusal(net, x) is not None              # ... and only inside it


def test_switch_on_still_refuses(monkeypatch):
    from bbb_hip import fast_train, ops
    _no_device(monkeypatch)
    convs = STRIDED["second_s2"]
    x = torch.zeros(8, 3, 16, 16)
    with ops.use_config(bf16_strided_train=True):
        assert "local-reparameterisation layers have no bf16 mode" in fast_train.bf16_train_refusal(_net("lrt", convs), x)
        assert "multiple of 8" in fast_train.bf16_train_refusal(_net("bbb", convs), torch.zeros(12, 3, 16, 16))
        xg = torch.zeros(8, 3, 16, 16, requires_grad=True)
        assert "do not require a gradient" in fast_train.bf16_train_refusal(_net("bbb", convs), xg)
        replay = _net("bbb", convs)
        next(m for m in replay.modules() if hasattr(m, "eps_source")).eps_source = object()
        assert fast_train.bf16_train_refusal(replay, x) == "no eps replay"
        # what the training path itself refuses stays refused (padding beyond the kernel reach in the strided layer)
        assert "train_path_ok" in fast_train.bf16_train_refusal(_net("bbb", [(8, 3, 1, 1, 1, None), (8, 3, 2, 3, 1, None)]), x)
        # a model without strided later layers does not care about the switch
        assert fast_train.bf16_train_refusal(_net("bbb", [(8, 3, 2, 1, 1, None), (8, 3, 1, 1, 1, None)]), x) is None


def _desc(_lib, **kw):
    # the stride-1 launch of a 3 x 3 / stride 2 / padding 1 layer's gradient: g [8][4 x 4], dx [8][8 x 8] (pad = 2 - 1), 8 images
    d = _lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = 8, 8, 4, 4, 8, 3, 3
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = d.draws = 1
    d.pad_h = d.pad_w = 1
    d.x_draw_stride, d.w_draw_stride = 8 * 4 * 4 * 8, 8 * 72
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_bf16_dgrad_entry_is_exported_and_validates_without_a_gpu(lib):
    assert "bbb_conv2d_chwn_bf16_dgrad" in lib.EXPORTS
    h = lib.lib()
    f = h.bbb_conv2d_chwn_bf16_dgrad
    assert h.bbb_abi_version() == 13
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        assert "int bbb_conv2d_chwn_bf16_dgrad(" in fh.read()
    ok = ctypes.byref(_desc(lib))
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    assert f(None, 64, 64, 64, 2, 2, 8, 8, 2, None) == EINVAL                               # no descriptor
    for args in ((None, 64, 64), (64, None, 64), (64, 64, None)):
        assert f(ok, *args, 2, 2, 8, 8, 2, None) == EINVAL                                  # a missing operand
    assert f(ok, 64, 64, 64, 1, 1, 8, 8, 2, None) == EINVAL                                 # stride 1 is the forward launch's job
    assert f(ok, 64, 64, 64, 0, 2, 8, 8, 2, None) == EINVAL
    assert f(ok, 64, 64, 64, 2, -1, 8, 8, 2, None) == EINVAL
    assert f(ok, 64, 64, 64, 2, 2, 0, 8, 2, None) == EINVAL
    assert f(ok, 64, 64, 64, 2, 2, 8, 0, 2, None) == EINVAL
    for field, v in (("batch", 0), ("cin", 0), ("h", -1), ("w", 0), ("cout", 0), ("kh", 0), ("kw", 0), ("stride_h", 2), ("stride_w", 2),
                     ("pad_h", -1), ("pad_w", -1), ("dil_h", 0), ("dil_w", 0), ("draws", 0), ("act", 1), ("pool", 1), ("w_tap_major", 1),
                     ("unit_div", 2), ("unit_off", 1), ("x_unit_mod", 2), ("x_unit_div", 2), ("x_unit_off", 1), ("w_row_pitch", 80),
                     ("b_offset", 4), ("x_draw_stride", -8), ("w_draw_stride", -8)):
        assert f(ctypes.byref(_desc(lib, **{field: v})), 64, 64, 64, 2, 2, 8, 8, 2, None) == EINVAL, field
    for flags in (1, 4, 8, 3, 16):                                                            # only BBB_BF16_W_TAP_MAJOR is a flag here
        assert f(ok, 64, 64, 64, 2, 2, 8, 8, flags, None) == EINVAL, flags
    for ptrs in ((72, 64, 64), (64, 72, 64), (64, 64, 72), (66, 64, 64), (64, 64, 66)):     # 16-byte alignment of all three
        assert f(ok, *ptrs, 2, 2, 8, 8, 2, None) == EALIGN, ptrs
    assert f(ctypes.byref(_desc(lib, x_draw_stride=8 * 4 * 4 * 8 + 4)), 64, 64, 64, 2, 2, 8, 8, 2, None) == EALIGN
    assert f(ctypes.byref(_desc(lib, w_draw_stride=8 * 72 + 4)), 64, 64, 64, 2, 2, 8, 8, 2, None) == EALIGN
    assert f(ctypes.byref(_desc(lib, batch=12)), 64, 64, 64, 2, 2, 8, 8, 2, None) == ESHAPE   # batch % 8
    assert f(ctypes.byref(_desc(lib, cin=12)), 64, 64, 64, 2, 2, 8, 8, 2, None) == ESHAPE     # tap-major rows need cin % 8
    assert f(ctypes.byref(_desc(lib, pad_h=3)), 64, 64, 64, 2, 2, 8, 8, 2, None) == ESHAPE    # the layer's padding would be negative
    assert f(ctypes.byref(_desc(lib, pad_w=3)), 64, 64, 64, 2, 2, 8, 8, 2, None) == ESHAPE
    assert f(ok, 64, 64, 64, 2, 2, 9, 8, 2, None) == ESHAPE                                  # a 9-row input gives 5 output rows, not 4
    assert f(ok, 64, 64, 64, 2, 2, 6, 8, 2, None) == ESHAPE
    assert f(ok, 64, 64, 64, 2, 2, 8, 10, 2, None) == ESHAPE
    assert f(ok, 64, 64, 64, 3, 2, 8, 8, 2, None) == ESHAPE                                  # stride 3 on 8 rows gives 3
    # the 32-bit offset limits of the bf16 forward and the exact range of the k decode
    big = dict(x_draw_stride=0, w_draw_stride=0)
    assert f(ctypes.byref(_desc(lib, cin=1 << 21, **big)), 64, 64, 64, 2, 2, 8, 8, 0, None) == ESHAPE          # K = 9 * 2^21 >= 2^24
    assert f(ctypes.byref(_desc(lib, cin=1 << 20, cout=1 << 10, **big)), 64, 64, 64, 2, 2, 8, 8, 2, None) == ESHAPE   # weight slab bytes
    assert f(ctypes.byref(_desc(lib, h=4096, w=4096, cin=64, **big)), 64, 64, 64, 2, 2, 8192, 8192, 2, None) == ESHAPE   # g slab bytes
    assert f(ctypes.byref(_desc(lib, cout=1 << 20, h=64, w=64, **big)), 64, 64, 64, 2, 2, 128, 128, 2, None) == ESHAPE   # dx slab bytes
    assert f(ctypes.byref(_desc(lib, batch=1 << 28, cin=8, h=1, w=1, kh=1, kw=1, pad_h=0, pad_w=0, **big)), 64, 64, 64, 2, 2, 1, 1, 0,
             None) == ESHAPE                                                                                    # one row of images


def test_form_selection_restatement():
    """ops.bf16_dgrad_form on hand-worked launches (the rules of csrc/pconv_bf16.hip)."""
    from bbb_hip import ops
    # dx 128 channels x 128 images: 128 x 128 tiles, wave-specialised up to 1024 items, plain above
    assert ops.bf16_dgrad_form(128, 128, 16, 3, 3, (6, 5), 2, 1, 1) == (22, 1, True, True)
    assert ops.bf16_dgrad_form(128, 128, 16, 3, 3, (32, 32), 2, 1, 1) == (22, 1, True, True)         # 1024 items
    assert ops.bf16_dgrad_form(128, 128, 16, 3, 3, (19, 18), 2, 1, 3) == (22, 1, False, True)        # 1026 items
    # 64 channels x 256 images: 64 x 256 tiles; a second k-group below 512 items once the LONGEST per-pixel contraction has 8 tiles:
    # 3 x 3 / 2 visits at most 2 x 2 taps, so Cout = 128 gives 512 k, Cout = 112 gives 448
    assert ops.bf16_dgrad_form(256, 64, 128, 3, 3, (5, 4), 2, 1, 1) == (14, 2, False, True)
    assert ops.bf16_dgrad_form(256, 64, 112, 3, 3, (5, 4), 2, 1, 1) == (14, 1, False, True)
    assert ops.bf16_dgrad_form(256, 64, 128, 3, 3, (16, 32), 2, 1, 1) == (14, 1, False, True)        # 512 items
    # dilation 2 under stride 2: every tap takes part (tstep = 1), 9 taps
    assert ops.bf16_dgrad_form(128, 64, 64, 3, 3, (6, 5), 2, 2, 1) == (12, 2, False, True)           # 576 k
    assert ops.bf16_dgrad_form(128, 64, 64, 3, 3, (6, 5), 2, 1, 1) == (12, 1, False, True)           # 256 k
    # reference-order rows (Cout % 8 != 0, or one tap): the full row counts
    assert ops.bf16_dgrad_form(128, 64, 60, 3, 3, (5, 4), 2, 1, 1) == (12, 2, False, False)          # 540 k
    assert ops.bf16_dgrad_form(8, 8, 512, 1, 1, (4, 6), 2, 1, 1) == (12, 2, False, False)
    # never four k-groups: what the forward calls "tiny" (>= 16 k tiles, < 256 items) runs with two
    assert ops.bf16_dgrad_form(8, 8, 1024, 3, 3, (4, 4), 2, 1, 1) == (12, 2, False, True)


def test_gpu_case_list_reaches_what_it_claims():
    import test_gpu_bf16_strided_train as T
    tags = {n: T.case_tags(c) for n, c in T.CASES.items()}
    reached = set().union(*tags.values())
    # every form the launcher can select (csrc/pconv_bf16.hip, launch_dgrad_shape) and both row orders
    forms = {"shape22-ws", "shape22-kg1", "shape14-kg1", "shape14-kg2", "shape12-kg1", "shape12-kg2"}
    assert {t for t in reached if t.startswith("shape")} == forms
    for form in forms:
        assert any(form in t and "tap-major" in t for t in tags.values()), form
    assert any("ref-order" in t and "ws" in t for t in tags.values()) and any("ref-order" in t and "kg>1" in t for t in tags.values())
    assert any("ref-order" in t and "plain" in t for t in tags.values())
    # an empty contraction under every form family; holes on reference-order rows too (their image rows read as zero)
    assert {"k0-plain", "k0-kg>1", "k0-ws"} <= reached
    assert any("holes" in t and "ref-order" in t for t in tags.values())
    assert {"gcd>1", "floor", "ragged-batch", "ragged-channels", "perdraw", "shared", "flip", "noflip"} <= reached
    assert any("ragged-batch" in t and "ragged-channels" in t and t & {"shape14-kg1", "shape12-kg1"} for t in tags.values())
    # named form cases are what their names say
    want = {"form_ws_128x128": "shape22-ws", "form_ws_k0": "shape22-ws", "form_ws_refrows": "shape22-ws", "form_22_plain": "shape22-kg1",
            "form_14_kg1": "shape14-kg1", "form_14_kg2": "shape14-kg2", "form_12_kg1": "shape12-kg1", "form_12_kg2": "shape12-kg2",
            "form_12_kg2_k0": "shape12-kg2", "form_12_kg2_refrows": "shape12-kg2"}
    for n, form in want.items():
        assert form in tags[n], (n, tags[n])
    assert "k0-ws" in tags["form_ws_k0"] and "k0-kg>1" in tags["form_12_kg2_k0"] and "k0-plain" in tags["holes_s4_k2"]
    assert "ref-order" in tags["form_ws_refrows"] and "ref-order" in tags["form_12_kg2_refrows"] and "ref-order" in tags["lenet_like_cout6"]
    # sizes stay those of the fp32 sweep plus the form cases: maps of 2-19 pixels a side, every B a multiple of 8
    assert all(c["B"] % 8 == 0 and 2 <= min(c["H"], c["W"]) and max(c["H"], c["W"]) <= 19 for c in T.CASES.values())
    assert all(T.CASES[n]["form"] in ("perdraw", "shared") for n in T.CASES)
    import test_gpu_strided_dgrad as SD
    assert set(SD.DGRAD_CASES) <= set(T.CASES)
    T.test_models_cover_what_they_claim()
