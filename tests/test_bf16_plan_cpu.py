"""CPU-only checks of the bf16 GEMM family's launch plan (csrc/pconv_bf16_plan.h) through its query entries
(bbb_conv2d_chwn_bf16_plan = ops.bf16_fwd_plan, bbb_conv2d_chwn_bf16_dgrad_plan = ops.bf16_dgrad_form): the library's choice against
the independent restatement of the forward rules (test_gpu_bf16_train_fuzz.gemm_form) over a seeded sweep, hand-worked cases of
the forms that restatement does not model (pooled strip / window-resident, strip8) with the launch entry's error codes for their
out-of-range variants, and a host-only walk of the plans under the undefined-behaviour sanitizer."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
EINVAL, EALIGN, ESHAPE = -1, -2, -3
OUT_F32, TAP_MAJOR, X_C8, OUT_C8 = 1, 2, 4, 8


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def test_query_entries_are_exported_and_declared(lib):
    h = lib.lib()
    assert h.bbb_abi_version() == 13
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = fh.read()
    for name in ("bbb_conv2d_chwn_bf16_plan", "bbb_conv2d_chwn_bf16_dgrad_plan", "bbb_lrt_conv2d_chwn_bf16_plan"):
        assert name in lib.EXPORTS and hasattr(h, name) and f"int {name}(" in header
    assert h.bbb_conv2d_chwn_bf16_plan(None, 0, None, None, None, None) == EINVAL
    assert h.bbb_conv2d_chwn_bf16_dgrad_plan(None, 2, 2, 8, 8, 0, None, None, None) == EINVAL
    from bbb_hip import ops
    for i, name in enumerate(("GENERAL", "SMALLK", "SMALLK_POOL", "SMALLK_POOLWIN", "STRIP8", "FEWOUT")):
        assert f"#define BBB_BF16_FORM_{name} {i} " in header and ops.BF16_FORMS[i] == name.lower().replace("_", "-")


def _sweep_case(rng):
    """One geometry of the sweep: B 8..512, cin 1..1040, cout 1..512, taps 1 / 3 / 5 / 11, strides 1 / 2 / 4, dilation 1 / 2, maps of
    1..32 pixels a side, 1..64 draws, both outputs, tap-major rows only where cin % 8 == 0.  Padding from the smallest that gives the
    layer an output pixel, so the library refuses next to nothing; a share of linear layers (the few-output form needs them)."""
    B = rng.choice([8, 16, 24, 64, 128, 136, 200, 256, 264, 512])
    cin = rng.choice([rng.randint(1, 16), rng.randint(1, 128), rng.randint(1, 1040), 8 * rng.randint(1, 130)])
    cout = rng.choice([rng.randint(1, 16), rng.randint(1, 128), rng.randint(1, 512)])
    draws = rng.choice([1, 1, 2, 3, 10, rng.randint(1, 64)])
    out_f32 = rng.random() < 0.5
    if rng.random() < 0.15:
        kh = kw = H = W = 1
        s, p, d = (1, 1), (0, 0), (1, 1)
    else:
        kh = rng.choice([1, 3, 5, 11])
        kw = kh if rng.random() < 0.8 else rng.choice([1, 3, 5, 11])
        s = (rng.choice([1, 1, 2, 4]), rng.choice([1, 1, 2, 4]))
        d = (rng.choice([1, 1, 2]), rng.choice([1, 1, 2]))
        H, W = rng.randint(1, 32), rng.randint(1, 32)
        p = tuple(max(0, -(-(dd * (k - 1) + 1 - n) // 2)) + rng.choice([0, 0, 1, 2]) for dd, k, n in ((d[0], kh, H), (d[1], kw, W)))
    tap_major = cin % 8 == 0 and rng.random() < 0.5
    return B, cin, H, W, cout, kh, kw, s, p, d, draws, out_f32, tap_major


def test_forward_plan_equals_the_independent_restatement(lib):
    """ops.bf16_fwd_plan == gemm_form on everything gemm_form models (no pool, no c8: the general, small-k and few-output forms)."""
    from test_gpu_bf16_train_fuzz import gemm_form
    from bbb_hip import ops
    rng = random.Random(20261018)
    N, skipped, reached = 24000, 0, set()
    for _ in range(N):
        B, cin, H, W, cout, kh, kw, s, p, d, draws, out_f32, tap_major = c = _sweep_case(rng)
        try:
            got = ops.bf16_fwd_plan((draws, cin, H, W, B), cout, (cin, kh, kw), s, p, d, out_f32=out_f32, tap_major=tap_major)
        except lib.BBBHipError:
            skipped += 1
            continue
        tags = gemm_form(*c)
        reached |= tags
        if "general" in tags:
            shape = next(int(t[5:]) for t in tags if t.startswith("shape"))
            kgs = 4 if "tiny" in tags else (1 if "ws" in tags else next(int(t[2:]) for t in tags if t.startswith("kg")))
            want = ("general", shape, kgs, "ws" in tags)
        else:
            (tag,) = tags
            want = ("smallk" if tag == "smallk" else "fewout", 0, 0, False)
            assert tag == "smallk" or tag == ("fewout-f32" if out_f32 else "fewout-bf16")
        assert got == want, (c, got, tags)
    assert N - skipped >= 20000 and skipped < 0.25 * N, skipped
    assert {"smallk", "fewout-f32", "fewout-bf16", "shape12", "shape14", "shape22", "tiny", "ws", "kg1", "kg2"} <= reached, reached


def _desc(lib, batch=256, cin=3, hw=(32, 32), cout=32, k=5, stride=1, pad=2, dil=1, draws=1, pool=0, **kw):
    d = lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = batch, cin, hw[0], hw[1], cout, k, k
    d.stride_h = d.stride_w = stride
    d.pad_h = d.pad_w = pad
    d.dil_h = d.dil_w = dil
    d.draws, d.pool = draws, pool
    d.x_draw_stride = cin * hw[0] * hw[1] * batch
    d.w_draw_stride = cout * ((cin * k * k + 7) & ~7)
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def _form(lib, d, flags):
    """(return code, form name | None) of the query entry; the launch entry must refuse with the same code (a refusal comes back
    before any launch, so this needs no device)."""
    from bbb_hip import ops
    h = lib.lib()
    fm, sh, kg, ws = (ctypes.c_int32(-1) for _ in range(4))
    rc = h.bbb_conv2d_chwn_bf16_plan(ctypes.byref(d), flags, ctypes.byref(fm), ctypes.byref(sh), ctypes.byref(kg), ctypes.byref(ws))
    if rc != 0:
        assert h.bbb_conv2d_chwn_bf16_fwd(ctypes.byref(d), 64, 64, None, 64, flags, None) == rc
        assert h.bbb_conv2d_chwn_bf16_plan(ctypes.byref(d), flags, None, None, None, None) == rc      # null out-pointers
        return rc, None
    name = ops.BF16_FORMS[fm.value]
    assert (name == "general") == (sh.value != 0) and (name == "general" or (sh.value, kg.value, ws.value) == (0, 0, 0))
    return 0, name


POOL22, POOL32 = 1, (3 << 8) | 2


def test_pooled_first_layer_forms(lib):
    """3Conv3FC conv1 (3 -> 32 channels, 5 x 5, padding 2, 32 x 32 images) with the pooling in the launch at bs 256: the window-resident
    form below 70 pooled rows x image tiles of the launch, the strip form from there on and for more than 32 channels."""
    # MaxPool2d(2, 2): 16 pooled rows per step -- one step 16, 4 steps 64, 5 steps 80, 16 steps per launch 256
    assert _form(lib, _desc(lib, pool=POOL22), 0) == (0, "smallk-poolwin")
    assert _form(lib, _desc(lib, pool=POOL22, draws=4), 0) == (0, "smallk-poolwin")
    assert _form(lib, _desc(lib, pool=POOL22, draws=5), 0) == (0, "smallk-pool")
    assert _form(lib, _desc(lib, pool=POOL22, draws=16), 0) == (0, "smallk-pool")
    assert _form(lib, _desc(lib, pool=(2 << 8) | 2), 0) == (0, "smallk-poolwin")                   # the long spelling of (2, 2)
    # the boundary itself: 3 steps of 23 pooled rows = 69, 7 steps of 10 = 70; two image tiles of 256 double the rows
    assert _form(lib, _desc(lib, hw=(46, 32), pool=POOL22, draws=3), 0) == (0, "smallk-poolwin")
    assert _form(lib, _desc(lib, hw=(20, 32), pool=POOL22, draws=7), 0) == (0, "smallk-pool")
    assert _form(lib, _desc(lib, hw=(20, 32), pool=POOL22, draws=6), 0) == (0, "smallk-poolwin")   # 60
    assert _form(lib, _desc(lib, hw=(20, 32), pool=POOL22, draws=6, batch=264), 0) == (0, "smallk-pool")   # 120
    # 64 channels: two 32-channel tiles per workgroup, which the window-resident form does not have
    assert _form(lib, _desc(lib, cout=64, pool=POOL22), 0) == (0, "smallk-pool")
    # the window of a strip (+ the zero row) must fit 13 passes of 16 image rows: 5 channels x 6 x 6 + 1 = 181 rows for one pooled
    # pixel fit, 16 channels x 5 x 5 + 1 = 401 (1 x 1 taps, stride 4) do not fit even one
    assert _form(lib, _desc(lib, cin=5, pool=POOL22), 0) == (0, "smallk-poolwin")
    assert _form(lib, _desc(lib, cin=16, k=1, pad=0, stride=4, hw=(64, 64), pool=POOL22), 0) == (0, "smallk-pool")
    # both forms write the channel-interleaved layout (cout % 8 == 0)
    assert _form(lib, _desc(lib, pool=POOL22), OUT_C8) == (0, "smallk-poolwin")
    assert _form(lib, _desc(lib, pool=POOL22, draws=16), OUT_C8) == (0, "smallk-pool")
    # MaxPool2d(3, 2): 15 pooled rows per step
    assert _form(lib, _desc(lib, pool=POOL32), 0) == (0, "smallk-poolwin")
    assert _form(lib, _desc(lib, pool=POOL32, draws=4), 0) == (0, "smallk-poolwin")                # 60
    assert _form(lib, _desc(lib, pool=POOL32, draws=5), 0) == (0, "smallk-pool")                   # 75
    assert _form(lib, _desc(lib, pool=POOL32, draws=16), 0) == (0, "smallk-pool")
    # what the pooled forms refuse: other windows, maps smaller than the window, tap-major rows, fp32 output, a row pitch > 128,
    # channel-interleaved input, an interleaved output of a channel count that is no multiple of 8
    for bad in ((3 << 8) | 3, (2 << 8) | 1, (4 << 8) | 2, 2, -1):
        assert _form(lib, _desc(lib, pool=bad), 0) == (EINVAL, None), bad
    assert _form(lib, _desc(lib, hw=(1, 32), pool=POOL22), 0) == (EINVAL, None)
    assert _form(lib, _desc(lib, hw=(32, 2), pool=POOL32), 0) == (EINVAL, None)
    assert _form(lib, _desc(lib, cin=8, pool=POOL22), TAP_MAJOR) == (EINVAL, None)
    assert _form(lib, _desc(lib, pool=POOL22), OUT_F32) == (EINVAL, None)
    assert _form(lib, _desc(lib, cin=6, pool=POOL22), 0) == (EINVAL, None)                          # K = 150 -> pitch 152
    assert _form(lib, _desc(lib, cin=5, pool=POOL22), 0)[0] == 0                                    # K = 125 -> pitch 128
    assert _form(lib, _desc(lib, pool=POOL22), X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, cout=30, pool=POOL22), OUT_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, batch=252, pool=POOL22), 0) == (ESHAPE, None)
    assert _form(lib, _desc(lib, pool=POOL22, x_draw_stride=4), 0) == (EALIGN, None)
    # without the pool the same layer is the small-k form
    assert _form(lib, _desc(lib), 0) == (0, "smallk")


def test_strip8_admission(lib):
    """BBB_BF16_X_C8: tap-major rows of 32 input channels, 5 x 5 taps, stride 1, no dilation, padding < 5, bf16 output in either
    layout (3Conv3FC conv2: 32 -> 64 channels on 16 x 16 maps, padding 2); every other request is BBB_EINVAL."""
    conv2 = dict(cin=32, hw=(16, 16), cout=64, k=5, pad=2)
    assert _form(lib, _desc(lib, **conv2), TAP_MAJOR | X_C8) == (0, "strip8")
    assert _form(lib, _desc(lib, **conv2), TAP_MAJOR | X_C8 | OUT_C8) == (0, "strip8")
    assert _form(lib, _desc(lib, **dict(conv2, pad=4, draws=16)), TAP_MAJOR | X_C8) == (0, "strip8")
    assert _form(lib, _desc(lib, **dict(conv2, cout=60)), TAP_MAJOR | X_C8) == (0, "strip8")
    # one condition broken at a time
    assert _form(lib, _desc(lib, **conv2), X_C8) == (EINVAL, None)                                  # reference-order rows
    assert _form(lib, _desc(lib, **conv2), TAP_MAJOR | X_C8 | OUT_F32) == (EINVAL, None)            # fp32 output
    assert _form(lib, _desc(lib, **dict(conv2, cin=64)), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **dict(conv2, cin=24)), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **dict(conv2, k=3, pad=1)), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **conv2, kh=3), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **conv2, kw=3), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **dict(conv2, stride=2)), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **conv2, stride_w=2), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **dict(conv2, dil=2, pad=4)), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **dict(conv2, pad=5)), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **conv2, pad_w=5), TAP_MAJOR | X_C8) == (EINVAL, None)
    assert _form(lib, _desc(lib, **dict(conv2, cout=60)), TAP_MAJOR | X_C8 | OUT_C8) == (EINVAL, None)   # interleaved output: cout % 8
    # without the flag the same layer runs on the general kernel
    assert _form(lib, _desc(lib, **conv2), TAP_MAJOR) == (0, "general")


def test_out_c8_needs_a_form_that_writes_it(lib):
    for d, flags in ((_desc(lib, cin=32, hw=(16, 16), cout=64), TAP_MAJOR | OUT_C8),               # the general kernel
                     (_desc(lib), OUT_C8),                                                          # the small-k form without pool
                     (_desc(lib, batch=136, cin=1040, hw=(1, 1), cout=8, k=1, pad=0), OUT_C8),      # the few-output form
                     (_desc(lib, cin=32, hw=(16, 16), cout=64), OUT_C8 | OUT_F32)):
        assert _form(lib, d, flags) == (EINVAL, None)
        assert _form(lib, d, flags & ~OUT_C8)[0] == 0
    # unknown flags, and the order of the checks: rows of 8 images (ESHAPE) are looked at before the flags (EINVAL)
    assert _form(lib, _desc(lib), 16) == (EINVAL, None)
    assert _form(lib, _desc(lib, batch=12), 16) == (ESHAPE, None)


def test_long_row_classifier_is_the_few_output_form(lib):
    """The case of tests/test_gpu_bf16.py commented as a long-row classifier: 1040 -> 10 at 136 images, two draws."""
    from bbb_hip import ops
    for out_f32 in (False, True):
        assert ops.bf16_fwd_plan((2, 1040, 1, 1, 136), 10, (1040, 1, 1), out_f32=out_f32) == ("fewout", 0, 0, False)
    assert ops.bf16_fwd_plan((2, 1040, 1, 1, 136), 10, (1040, 1, 1), tap_major=True) == ("fewout", 0, 0, False)
    # 17 outputs: the general kernel's "tiny" rule, 64 x 128 tiles with four k-groups
    assert ops.bf16_fwd_plan((2, 1040, 1, 1, 136), 17, (1040, 1, 1)) == ("general", 12, 4, False)


def test_plans_are_free_of_undefined_behaviour(tmp_path):
    """tests/host/bf16_plan_check.cpp (the plan header alone, no device code) under -fsanitize=undefined: ordinary geometries and
    descriptors with dimensions near INT32_MAX / 2."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bf16_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "bf16_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    assert int(got["cases"]) >= 100000 and min(int(got[k]) for k in ("ok", "einval", "eshape")) > 10000 and len(got["checksum"]) == 16
