"""CPU-only checks of bf16 input gradients (LaunchConfig.bf16_input_grad): the switch and the gate (fast_train.bf16_train_refusal with
it off and on), the two new entries of the C ABI, the argument validation of bbb_first_layer_dgrad_bf16 in its documented order (it
happens before any launch, so the codes come back on a GPU-less host), its plan (bbb_first_layer_dgrad_bf16_plan =
ops.first_layer_dgrad_bf16_plan) against a Python restatement over a seeded sweep, a host-only walk of the plan header under the
sanitizers, the float64 restatement of the contract with dx (tests/bf16_input_grad_contract.py) against torch autograd, and that
the six models of tests/test_gpu_bf16_input_grad.py are on the training path."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest
import torch

import bf16_input_grad_contract as CX
from test_strided_train_cpu import _net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
EINVAL, EALIGN, ESHAPE = -1, -2, -3
G_F32, TAP_MAJOR = 1, 2
P = 64            # a dummy operand pointer: non-null, 16-byte aligned, never dereferenced (every call below is refused before a launch)


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


# ---- the switch and the gate ----
def test_config_field():
    from bbb_hip import ops
    assert "bf16_input_grad" in ops.LaunchConfig.FIELDS and ops.LaunchConfig().bf16_input_grad is False
    on = ops.LaunchConfig(bf16_input_grad=True)
    assert on.key() != ops.LaunchConfig().key() and on.copy().bf16_input_grad is True and on.copy(bf16_input_grad=False).bf16_input_grad is False
    assert ops.current_config().bf16_input_grad is False
    with ops.use_config(bf16_input_grad=True):
        assert ops.current_config().bf16_input_grad is True
        with ops.use_config(bf16_avgpool=True):
            assert ops.current_config().bf16_input_grad is True
    assert ops.current_config().bf16_input_grad is False
    assert "bf16_input_grad" in ops.LaunchConfig.__doc__ and "bf16_input_grad" in repr(on)


CONVS = [(8, 3, 1, 1, 1, None), (8, 3, 1, 1, 1, None)]


def test_gate_follows_the_switch(monkeypatch):
    from bbb_hip import fast_train, ops
    _no_device(monkeypatch)
    net = _net("bbb", CONVS)
    xg = torch.zeros(8, 3, 16, 16, requires_grad=True)
    why = fast_train.bf16_train_refusal(net, xg)
    assert why is not None and "do not require a gradient" in why
    assert "LaunchConfig.bf16_input_grad" in why and "ops.use_config(bf16_input_grad=True)" in why
    with ops.use_config(bf16_input_grad=True):
        assert fast_train.bf16_train_refusal(net, xg) is None
    assert fast_train.bf16_train_refusal(net, xg) is not None                 # ... and only inside it
    assert fast_train.bf16_train_refusal(net, torch.zeros(8, 3, 16, 16)) is None
    with torch.no_grad():                                                    # nothing is differentiated: nothing to refuse
        assert fast_train.bf16_train_refusal(net, xg) is None


def test_switch_on_still_refuses(monkeypatch):
    from bbb_hip import fast_train, ops
    _no_device(monkeypatch)
    with ops.use_config(bf16_input_grad=True):
        xg = torch.zeros(8, 3, 16, 16, requires_grad=True)
        assert "local-reparameterisation layers have no bf16 mode" in fast_train.bf16_train_refusal(_net("lrt", CONVS), xg)
        assert "multiple of 8" in fast_train.bf16_train_refusal(_net("bbb", CONVS), torch.zeros(12, 3, 16, 16, requires_grad=True))
        replay = _net("bbb", CONVS)
        next(m for m in replay.modules() if hasattr(m, "eps_source")).eps_source = object()
        assert fast_train.bf16_train_refusal(replay, xg) == "no eps replay"
        # the other two switches keep their own lines
        strided = _net("bbb", [(8, 3, 1, 1, 1, None), (8, 3, 2, 1, 1, None)])
        assert "bf16_strided_train" in fast_train.bf16_train_refusal(strided, xg)
        with ops.use_config(bf16_strided_train=True):
            assert fast_train.bf16_train_refusal(strided, xg) is None
        assert "4-d fp32 CUDA batch" in fast_train.bf16_train_refusal(_net("bbb", CONVS), torch.zeros(8, 3, 16, 16, dtype=torch.float64))


def test_the_six_models_are_on_the_training_path():
    from bbb_hip import fast_train

    class X:
        pass

    for name in CX.MODELS:
        net, plan, chw = CX.build(name)
        X.shape = (8,) + chw
        assert fast_train._train_path_static(net, X) == "bbb", name
        assert len(plan) == 2


# ---- the C ABI ----
def test_entries_are_exported_and_declared(lib):
    h = lib.lib()
    assert h.bbb_abi_version() == 13 and lib.ABI_VERSION == 13
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = fh.read()
    for name in ("bbb_first_layer_dgrad_bf16", "bbb_first_layer_dgrad_bf16_plan"):
        assert name in lib.EXPORTS and hasattr(h, name) and f"int {name}(" in header


def _desc(lib, batch=8, cin=3, hw=(9, 13), cout=12, k=(2, 3), stride=(3, 2), pad=(1, 0), dil=(1, 2), draws=2, **kw):
    d = lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = batch, cin, hw[0], hw[1], cout, k[0], k[1]
    d.stride_h, d.stride_w = stride
    d.pad_h, d.pad_w = pad
    d.dil_h, d.dil_w = dil
    d.draws = draws
    d.w_draw_stride = cout * ((cin * k[0] * k[1] + 7) & ~7)
    for name, v in kw.items():
        setattr(d, name, v)
    return d


NCOLS = 4 * 5 * 8          # the default descriptor's output map (4 x 5) times its 8 images


def _rc(lib, d, gp=NCOLS, dp=NCOLS, flags=0, g=P, w=P, dcol=P):
    """The launch entry's code; where no operand pointer is at fault the plan query must return the same, with and without
    out-pointers."""
    h = lib.lib()
    dref = None if d is None else ctypes.byref(d)
    rc = h.bbb_first_layer_dgrad_bf16(dref, g, gp, w, dcol, dp, flags, None)
    assert rc != 0, "this helper is for refusals: an accepted call would launch"
    if (g, w, dcol) == (P, P, P):
        out = [ctypes.c_int32(-1) for _ in range(3)] + [ctypes.c_int64(-1)]
        assert h.bbb_first_layer_dgrad_bf16_plan(dref, gp, dp, flags, *[ctypes.byref(v) for v in out]) == rc
        assert h.bbb_first_layer_dgrad_bf16_plan(dref, gp, dp, flags, None, None, None, None) == rc
    return rc


def test_every_check_refuses_before_a_launch_in_the_documented_order(lib):
    h = lib.lib()
    ok = _desc(lib)
    out = [ctypes.c_int32(-1) for _ in range(3)] + [ctypes.c_int64(-1)]
    assert h.bbb_first_layer_dgrad_bf16_plan(ctypes.byref(ok), NCOLS, NCOLS, 0, *[ctypes.byref(v) for v in out]) == 0
    assert [v.value for v in out] == [32, 128, 1, 8]                      # J = 18 -> 32 rows; M = 24 -> one chunk; 160 columns -> 2 tiles, dealt to 8 XCDs
    # BBB_EINVAL: nulls and unknown flags
    assert _rc(lib, None) == EINVAL
    for kw in (dict(g=None), dict(w=None), dict(dcol=None)):
        assert _rc(lib, ok, **kw) == EINVAL, kw
    for bit in (4, 8, 1 << 31):
        assert _rc(lib, ok, flags=bit) == EINVAL
    # ... the descriptor: sizes, the fields a layer does not have, the rows' pitch, tap-major rows
    for field, v in (("batch", 0), ("cin", 0), ("h", -1), ("w", 0), ("cout", 0), ("kh", 0), ("kw", -2), ("stride_h", 0), ("stride_w", -1),
                     ("pad_h", -1), ("pad_w", -1), ("dil_h", 0), ("dil_w", 0), ("draws", 0), ("x_draw_stride", 8), ("b_draw_stride", 12),
                     ("act", 1), ("w_row_pitch", 24), ("pool", 1), ("w_tap_major", 1), ("unit_div", 2), ("unit_off", 1), ("x_unit_mod", 1),
                     ("x_unit_div", 2), ("x_unit_off", 1), ("b_offset", 8), ("w_draw_stride", 12 * 18), ("w_draw_stride", 0)):
        assert _rc(lib, _desc(lib, **{field: v})) == EINVAL, field
    assert _rc(lib, ok, flags=TAP_MAJOR) == EINVAL                       # cin = 3
    # BBB_EINVAL wins over BBB_EALIGN and BBB_ESHAPE
    assert _rc(lib, _desc(lib, batch=12), flags=4, g=72) == EINVAL
    # BBB_EALIGN: the three pointers, the pitches
    for kw in (dict(g=72), dict(w=72), dict(dcol=72), dict(g=66), dict(dcol=68)):
        assert _rc(lib, ok, **kw) == EALIGN, kw
    assert _rc(lib, ok, gp=NCOLS + 4) == EALIGN and _rc(lib, ok, dp=NCOLS + 2) == EALIGN
    assert _rc(lib, ok, gp=NCOLS + 8, dp=NCOLS + 4, g=72) == EALIGN
    # BBB_EALIGN wins over BBB_ESHAPE
    assert _rc(lib, _desc(lib, batch=12), g=72) == EALIGN and _rc(lib, _desc(lib, batch=12), dp=4 * 5 * 12 + 2) == EALIGN
    # BBB_ESHAPE: pitches below a row, batch % 8, a kernel larger than the padded map, the 32-bit limits, the grid
    assert _rc(lib, ok, gp=NCOLS - 8) == ESHAPE and _rc(lib, ok, dp=NCOLS - 4) == ESHAPE
    assert _rc(lib, _desc(lib, batch=12), gp=4 * 5 * 12 + 8, dp=4 * 5 * 12) == ESHAPE
    assert _rc(lib, _desc(lib, batch=4), gp=80, dp=80) == ESHAPE
    assert _rc(lib, _desc(lib, hw=(2, 2), k=(3, 3), stride=(2, 2), pad=(0, 0), dil=(1, 1)), gp=8, dp=8) == ESHAPE
    assert _rc(lib, _desc(lib, hw=(2, 13), k=(5, 3), pad=(1, 0)), gp=8, dp=8) == ESHAPE
    big = dict(cin=4, hw=(1, 1), k=(1, 1), stride=(1, 1), pad=(0, 0), dil=(1, 1))
    assert _rc(lib, _desc(lib, cout=1 << 10, draws=1 << 10, **big), gp=2048, dp=8) == ESHAPE          # M * g_row_pitch = 2^31
    assert h.bbb_first_layer_dgrad_bf16_plan(ctypes.byref(_desc(lib, cout=1 << 10, draws=1 << 10, **big)), 2040, 8, 0, None, None, None, None) == 0
    assert _rc(lib, _desc(lib, cout=1 << 14, draws=1 << 14, **big), gp=8, dp=8) == ESHAPE             # M * Kp = 2^31
    assert _rc(lib, _desc(lib, cout=1, draws=1, **dict(big, cin=1 << 20)), gp=8, dp=2048) == ESHAPE   # J * d_row_pitch = 2^31
    assert _rc(lib, _desc(lib, cout=0x7fffffff, draws=2, **big), gp=8, dp=8) == ESHAPE                # E * cout past an int
    assert _rc(lib, _desc(lib, cout=1, draws=1, **dict(big, cin=0x7fffffff, k=(2, 1))), gp=8, dp=8) == EINVAL    # (Kp is not representable: the rows' pitch cannot match)


# ---- the plan against a restatement ----
def restated_plan(B, w_shape, hw, stride, pad, dil, draws, gp, dp, g_f32, tap_major):
    """(tile_j, tile_n, k_chunks, workgroups) or None where the entry refuses, from the rule as include/bbb_hip.h words it."""
    cout, cin, kh, kw = w_shape
    if tap_major and cin % 8:
        return None
    if gp % 8 or dp % 4:
        return None
    ho = (hw[0] + 2 * pad[0] - dil[0] * (kh - 1) - 1) // stride[0] + 1
    wo = (hw[1] + 2 * pad[1] - dil[1] * (kw - 1) - 1) // stride[1] + 1
    if ho < 1 or wo < 1 or B % 8:
        return None
    n, J, M = ho * wo * B, cin * kh * kw, draws * cout
    if gp < n or dp < n or max(M * gp, M * ((J + 7) // 8 * 8), J * dp) > 0x7fffffff:
        return None
    tj = 32 if J <= 32 else 64
    return tj, 128, -(-M // 32), 8 * -(-(-(-J // tj) * -(-n // 128)) // 8)          # (the tiles dealt to the 8 XCDs)


def test_plan_equals_the_restatement(lib):
    from bbb_hip import ops
    rng = random.Random(20261019)
    refused, seen = 0, set()
    N = 6000
    for i in range(N):
        linear = rng.random() < 0.2
        B = 8 * rng.choice([1, 1, 2, 3, 5, 15, 16, 17, 64])
        if rng.random() < 0.05:
            B += 4
        # E * cout around the multiples of 16 and 32; J around 32 (and 64); columns around the 128-column tile
        M = rng.choice([16, 32, 48, 64, 96, 320]) + rng.choice([-2, -1, 0, 0, 1, 2])
        draws = rng.choice([d for d in (1, 2, 3, 5, 6, 10) if M % d == 0] or [1])
        cout = M // draws
        if linear:
            cin, kh, kw, hw, stride, pad, dil = rng.choice([28, 32, 36, 48, 60, 64, 68, 200]), 1, 1, (1, 1), (1, 1), (0, 0), (1, 1)
        else:
            cin, kh, kw = rng.choice([(1, 5, 5), (3, 3, 3), (3, 11, 11), (4, 2, 4), (8, 2, 2), (8, 3, 3), (16, 1, 2), (2, 4, 4), (11, 1, 3), (3, 2, 3), (1, 1, 1)])
            stride, dil = (rng.choice([1, 2, 3, 4]), rng.choice([1, 2])), (rng.choice([1, 1, 2]), rng.choice([1, 2]))
            pad = (rng.randint(0, dil[0] * (kh - 1)), rng.randint(0, dil[1] * (kw - 1)))
            hw = (rng.randint(1, 20), rng.randint(1, 20))
        tap_major = cin % 8 == 0 and kh * kw > 1 if rng.random() < 0.9 else rng.random() < 0.5
        g_f32 = rng.random() < 0.5
        ho = (hw[0] + 2 * pad[0] - dil[0] * (kh - 1) - 1) // stride[0] + 1
        wo = (hw[1] + 2 * pad[1] - dil[1] * (kw - 1) - 1) // stride[1] + 1
        n = max(ho, 0) * max(wo, 0) * B
        gp = n + rng.choice([0, 0, 0, 0, 0, 8, 32, -8, 4])
        dp = n + rng.choice([0, 0, 0, 0, 0, 4, 32, -4, 2])
        want = restated_plan(B, (cout, cin, kh, kw), hw, stride, pad, dil, draws, gp, dp, g_f32, tap_major)
        try:
            got = ops.first_layer_dgrad_bf16_plan(B, (cout, cin, kh, kw), hw, stride, pad, dil, draws, g_row_pitch=gp, d_row_pitch=dp,
                                                  g_f32=g_f32, tap_major=tap_major)
        except lib.BBBHipError:
            got = None
        assert got == want, (i, B, cout, cin, kh, kw, hw, stride, pad, dil, draws, gp, dp, tap_major, got, want)
        if want is None:
            refused += 1
        else:
            seen.add((want[0], M % 32 == 0, M % 16 == 0, n % 128 == 0, linear))
    print(f"refused {refused} of {N}; {len(seen)} kinds of plan")
    assert refused < 0.65 * N
    assert {s[0] for s in seen} == {32, 64} and {s[1] for s in seen} == {True, False} and {s[3] for s in seen} == {True, False}
    assert {s[4] for s in seen} == {True, False}
    # hand-worked: AlexNet's conv1 on 32 x 32 at bs 512 x 10, the fp32 g_pre at its padded pitch
    assert ops.first_layer_dgrad_bf16_plan(512, (64, 3, 11, 11), (32, 32), 4, 5, 1, 10, g_row_pitch=32768 + 32, g_f32=True) == (64, 128, 20, 6 * 256)
    # the tile is a function of the layer alone: the number of columns does not enter it
    assert {ops.first_layer_dgrad_bf16_plan(B, (16, 3, 3, 3), (8, 8), 1, 1, 1, 2)[:3] for B in (8, 24, 512)} == {(32, 128, 1)}


def test_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/input_grad_bf16_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: ordinary first layers, every refusal, descriptors and pitches at the integer limits."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "input_grad_bf16_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "input_grad_bf16_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    assert int(got["cases"]) >= 120000 and min(int(got[k]) for k in ("ok", "einval", "ealign", "eshape")) > 1000, got
    assert min(int(got["tile32"]), int(got["tile64"])) > 1000 and len(got["checksum"]) == 16, got


# ---- the restatement of the contract: without roundings it is torch autograd's d loss / d x ----
@pytest.mark.parametrize("name", list(CX.MODELS))
def test_contract_dx_without_roundings_is_autograd(name):
    from bbb_hip import rng
    torch.manual_seed(3)
    net, plan, chw = CX.build(name)
    rng.assign_stream_ids(net)
    npar = CX.numpy_params(net)
    E, B = 2, 8
    eps = CX.device_eps(net, plan, npar, 4242, 7, E)
    g = np.random.default_rng(1)
    x, y = g.random((B,) + chw, dtype=np.float32), g.integers(0, 10, B)
    loss, lo, dx = CX.step_dx(plan, npar, x, y, eps, 0.1, 100.0, rounding=False)
    want = CX.autograd_dx(plan, npar, x, y, eps, 100.0)
    assert dx.shape == x.shape and np.abs(want).max() > 0
    assert np.abs(dx - want).max() <= 1e-12 * np.abs(want).max()
    # ... and with them it is another set of numbers of the same shape (how far off: a rounding can re-route a pooling window, so no
    # bound is stated here; the device is held to this restatement, not to the exact gradient)
    _, _, dxr = CX.step_dx(plan, npar, x, y, eps, 0.1, 100.0)
    assert dxr.shape == want.shape and np.isfinite(dxr).all() and np.abs(dxr - want).max() > 0
