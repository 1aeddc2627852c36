"""CPU-only checks of the layer under the C ABI: the launch plan of the split-bf16 contraction over MFMA-ready operands
(csrc/pconv_c8x3_plan.h) through its query entry (bbb_conv2d_c8x3_plan = ops.c8x3_fwd_plan) against an independent restatement of
the rule over a seeded sweep and on hand-worked refusals, with the launch entries' own codes; the one descriptor check
(csrc/conv_desc_check.h): a kernel that reaches past the padded input is BBB_ESHAPE from every entry that takes a descriptor; the
fp32 transposed launch's plan (bbb_conv2d_chwn_dgrad_plan = ops.fp32_dgrad_plan) against the forward's; and a host-only walk of the
c8x3 plan under the sanitizers.  A refusal comes back before any launch, so none of this needs a device."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
EINVAL, EALIGN, ESHAPE = -1, -2, -3
OUT_F32, TILE128, TILE256, POOL, NT_SHIFT = 1, 2, 4, 8, 4
P = 64            # a dummy operand pointer: non-null, 16-byte aligned, never dereferenced (every call below is refused before a launch)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def test_query_entries_are_exported_and_declared(lib):
    from bbb_hip import ops
    h = lib.lib()
    assert h.bbb_abi_version() == 13
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = fh.read()
    for name in ("bbb_conv2d_c8x3_plan", "bbb_conv2d_chwn_dgrad_plan"):
        assert name in lib.EXPORTS and hasattr(h, name) and f"int {name}(" in header
    assert h.bbb_conv2d_c8x3_plan(None, 0, 0, None, None, None, None, None) == EINVAL
    assert h.bbb_conv2d_chwn_dgrad_plan(None, 2, 2, 8, 8, None, None, None, None) == EINVAL
    assert len(ops.C8X3_FORMS) == 20 and len(set(ops.C8X3_FORMS)) == 20
    for i, name in enumerate(ops.C8X3_FORMS):
        assert f"#define BBB_C8X3_FORM_{name.upper().replace('-', '_')} {i}\n" in header
    with open(os.path.join(PKG, "csrc", "pconv_c8x3.hip")) as fh:
        assert "getenv" not in fh.read()


# ---- the sweep: ops.c8x3_fwd_plan against a restatement of the launcher's rule ----
def _trunc_div(a, b):
    """C's integer division (towards zero), as the launcher's output-map arithmetic was written."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def restated_plan(B, cin, H, W, cout, kh, kw, s, p, d, draws, out_f32, pool, lrt, tile, nt_force):
    """The launcher's decisions for a launch without work units, restated from the text of c8x3_launch as it stood before the plan
    header existed: None where it refuses, else (form, nt, images per workgroup, items, workgroups, why MT)."""
    if pool and out_f32:
        return None
    if lrt and (pool or nt_force not in (0, 2)):
        return None
    sets = 2 if lrt else 1
    if cin % 16 or B % 4 or (not out_f32 and cout % 8):
        return None
    ho = _trunc_div(H + 2 * p[0] - d[0] * (kh - 1) - 1, s[0]) + 1
    wo = _trunc_div(W + 2 * p[1] - d[1] * (kw - 1) - 1, s[1]) + 1
    if ho <= 0 or wo <= 0:
        return None
    if pool and (p != (0, 0) or ho % 2 or wo % 2):
        return None
    x_ps, y_ps, K = cin * H * W * B, cout * ho * wo * B // (4 if pool else 1), cin * kh * kw
    if 6 * sets * x_ps >= 0x3FFF0000 or 6 * sets * y_ps >= 0x3FFF0000 or (cout + 128) * K * 4 >= 0x3FFF0000:
        return None
    pixels = ho * wo // (4 if pool else 1)
    nt = nt_force or 2
    bm2 = (32 if pool else 128) * 2
    items2 = draws * -(-cout // (32 * nt)) * pixels * -(-B // bm2)
    if tile is not None:
        mt, why = (1 if tile in (128, 32) else 2), "flag"
    elif B <= bm2 // 2:
        mt, why = 1, "images"
    elif items2 < 1024:
        mt, why = 1, "items"
    else:
        mt, why = 2, "neither"
    if lrt:
        mt, why = 1, (why if why == "flag" else "lrt")
    bm = (32 if pool else 128) * mt
    items = -(-cout // (32 * nt)) * draws * pixels * -(-B // bm)
    blocks = 8 * -(-items // 8)
    if blocks > 0x7fffffff:
        return None
    form = ("lrt-f32" if out_f32 else "lrt-s3") if lrt else f"nt{nt}-mt{mt}-{'pool' if pool else 'f32' if out_f32 else 's3'}"
    return form, nt, bm, items, blocks, why


def _sweep_case(rng):
    """B = 4 x {1, 2, 8, 16, 17, 33, 64, 65, 128}, cin = 16 x {1, 1, 2, 3, 4, 16}, cout a multiple of 8 up to 320 (fp32 output:
    anything in 1..300), taps 1 / 2 / 3 / 5, strides 1 / 2, dilation 1 / 2, maps of 1..24 a side, padding from the smallest that
    gives an output pixel (pooled: 0, and most maps chosen so that the conv map is even), a quarter pooled, a fifth LRT, draws
    1 / 2 / 3 / 10 / 40, the image tile forced in half of the cases, NT in three of five."""
    B = 4 * rng.choice([1, 2, 8, 16, 17, 33, 64, 65, 128])
    cin = 16 * rng.choice([1, 1, 2, 3, 4, 16])
    pool, lrt = rng.random() < 0.25, rng.random() < 0.2
    out_f32 = rng.random() < (0.1 if pool else 0.35)
    cout = rng.randint(1, 300) if out_f32 else 8 * rng.randint(1, 40)
    kh = rng.choice([1, 2, 3, 5])
    kw = kh if rng.random() < 0.8 else rng.choice([1, 2, 3, 5])
    s = (rng.choice([1, 1, 2]), rng.choice([1, 1, 2]))
    d = (rng.choice([1, 1, 2]), rng.choice([1, 1, 2]))
    H, W = rng.randint(1, 24), rng.randint(1, 24)
    if pool:
        p = (0, 0)
        if rng.random() < 0.85:         # an even conv map where one fits 24 rows: 2 m pixels need (2 m - 1) s + d (k - 1) + 1 rows
            fit = [[(2 * m - 1) * ss + dd * (k - 1) + 1 for m in range(1, 7) if (2 * m - 1) * ss + dd * (k - 1) + 1 <= 24]
                   for ss, dd, k in ((s[0], d[0], kh), (s[1], d[1], kw))]
            H, W = rng.choice(fit[0]), rng.choice(fit[1])
    else:
        p = tuple(max(0, -(-(dd * (k - 1) + 1 - n) // 2)) + rng.choice([0, 0, 1, 2]) for dd, k, n in ((d[0], kh, H), (d[1], kw, W)))
    draws = rng.choice([1, 2, 3, 10, 40])
    tile = rng.choice([32, 64] if pool else [128, 256]) if rng.random() < 0.5 else None
    nt = rng.choice([2, 3, 4]) if rng.random() < 0.6 else 0
    return B, cin, H, W, cout, kh, kw, s, p, d, draws, out_f32, pool, lrt, tile, nt


def test_plan_equals_the_independent_restatement(lib):
    from bbb_hip import ops
    rng = random.Random(20261019)
    N, refused, forms, reasons = 20000, 0, {}, {}
    for _ in range(N):
        B, cin, H, W, cout, kh, kw, s, p, d, draws, out_f32, pool, lrt, tile, nt = c = _sweep_case(rng)
        want = restated_plan(*c)
        try:
            got = ops.c8x3_fwd_plan((draws, cin, H, W, B), cout, (kh, kw), s, p, d, out_f32=out_f32, tile=tile, nt=nt or None, pool=pool, lrt=lrt)
        except lib.BBBHipError:
            got = None
        assert got == (want and want[:5]), (c, got, want)
        if want is None:
            refused += 1
            continue
        forms[want[0]] = forms.get(want[0], 0) + 1
        reasons[want[5]] = reasons.get(want[5], 0) + 1
    print(f"refused {refused} of {N}; forms {forms}; MT by {reasons}")
    assert refused <= 0.30 * N, refused
    assert set(forms) == set(ops.C8X3_FORMS), set(ops.C8X3_FORMS) - set(forms)
    assert set(reasons) == {"flag", "lrt", "images", "items", "neither"} and min(reasons.values()) >= 500, reasons


# ---- hand-worked refusals, one for each check of the plan, with the launch entries' own codes ----
def _desc(lib, batch=8, cin=16, hw=(6, 6), cout=16, k=3, stride=1, pad=1, dil=1, draws=2, **kw):
    d = lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = batch, cin, hw[0], hw[1], cout, k, k
    d.stride_h = d.stride_w = stride
    d.pad_h = d.pad_w = pad
    d.dil_h = d.dil_w = dil
    d.draws = draws
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def _launch(h, d, flags, lrt, x=P, w=P, bias=None, y=P, w_var=P, b_var=None):
    if lrt:
        return h.bbb_lrt_conv2d_c8x3_fwd(ctypes.byref(d), x, w, w_var, bias, b_var, y, 1, 2, 3, 1, None, flags, None)
    return h.bbb_conv2d_c8x3_fwd(ctypes.byref(d), x, w, bias, y, flags, None)


def _rc(lib, d, flags=0, lrt=False):
    """The query's return code; a refusal must come back from the launch entry with the same code, and with null out-pointers."""
    h = lib.lib()
    out = [ctypes.c_int32(-1) for _ in range(3)] + [ctypes.c_int64(-1) for _ in range(2)]
    rc = h.bbb_conv2d_c8x3_plan(ctypes.byref(d), flags, 1 if lrt else 0, *[ctypes.byref(v) for v in out])
    assert h.bbb_conv2d_c8x3_plan(ctypes.byref(d), flags, 1 if lrt else 0, None, None, None, None, None) == rc
    if rc != 0:
        assert _launch(h, d, flags, lrt) == rc
    return rc


def test_every_check_of_the_plan_refuses_with_the_launch_entrys_code(lib):
    h = lib.lib()
    nt = lambda n: n << NT_SHIFT
    assert _rc(lib, _desc(lib)) == 0 and _rc(lib, _desc(lib), lrt=True) == 0
    # the flag word
    assert _rc(lib, _desc(lib), 1 << 24) == EINVAL                                 # an unknown bit
    assert _rc(lib, _desc(lib), TILE128 | TILE256) == EINVAL
    assert _rc(lib, _desc(lib), nt(1)) == EINVAL and _rc(lib, _desc(lib), nt(5)) == EINVAL and _rc(lib, _desc(lib), nt(7)) == EINVAL
    assert _rc(lib, _desc(lib, hw=(4, 4), pad=0), POOL | OUT_F32) == EINVAL
    assert [_rc(lib, _desc(lib), nt(n)) for n in (2, 3, 4)] == [0, 0, 0]
    # the descriptor's sizes and the fields this family leaves alone
    for field, v in (("batch", 0), ("cin", -16), ("h", 0), ("cout", 0), ("kw", 0), ("stride_h", 0), ("pad_w", -1), ("dil_h", 0), ("draws", 0),
                     ("act", 3), ("act", -1), ("pool", 1), ("w_row_pitch", 144), ("w_tap_major", 1)):
        assert _rc(lib, _desc(lib, **{field: v})) == EINVAL, field
    # the LRT restrictions
    assert _rc(lib, _desc(lib, hw=(4, 4), pad=0), POOL, lrt=True) == EINVAL
    assert _rc(lib, _desc(lib), nt(3), lrt=True) == EINVAL and _rc(lib, _desc(lib), nt(2), lrt=True) == 0
    assert _rc(lib, _desc(lib, w_draw_stride=16 * 9 * 16), lrt=True) == EINVAL
    assert _rc(lib, _desc(lib, b_draw_stride=16), lrt=True) == EINVAL
    # rows of 16 channels, 4 images, 8 output channels unless fp32
    assert _rc(lib, _desc(lib, cin=24)) == ESHAPE and _rc(lib, _desc(lib, batch=6)) == ESHAPE
    assert _rc(lib, _desc(lib, cout=12)) == ESHAPE and _rc(lib, _desc(lib, cout=12), OUT_F32) == 0
    # the output map: none, and a kernel that reaches past the padded input (stride 2 would name one row)
    assert _rc(lib, _desc(lib, hw=(2, 2), k=3, pad=0)) == ESHAPE
    assert _rc(lib, _desc(lib, hw=(2, 2), k=3, pad=0, stride=2)) == ESHAPE
    assert _rc(lib, _desc(lib, hw=(3, 3), k=3, pad=0, stride=2)) == 0
    # the pooled form's geometry
    assert _rc(lib, _desc(lib, hw=(4, 4), pad=0), POOL) == 0
    assert _rc(lib, _desc(lib, hw=(4, 4), pad=1), POOL) == ESHAPE
    assert _rc(lib, _desc(lib, hw=(5, 4), pad=0), POOL) == ESHAPE and _rc(lib, _desc(lib, hw=(4, 5), pad=0), POOL) == ESHAPE
    # operand pointers: only the launch entries see them; alignment comes after the pooled geometry and before the zero border
    ok = _desc(lib)
    for kw in (dict(x=72), dict(y=72), dict(w=72), dict(bias=68)):
        assert _launch(h, ok, 0, False, **kw) == EALIGN, kw
    assert _launch(h, ok, OUT_F32, False, bias=66) == EALIGN
    for kw in (dict(x=None), dict(w=None), dict(y=None)):
        assert _launch(h, ok, 0, False, **kw) == EINVAL, kw
    assert _launch(h, ok, 0, True, w_var=None) == EINVAL and _launch(h, ok, 0, True, bias=P) == EINVAL        # b_mu without b_var
    assert _launch(h, ok, 0, True, w_var=72) == EALIGN and _launch(h, ok, 0, True, bias=P, b_var=72) == EALIGN
    assert _launch(h, _desc(lib, cin=24), 0, True, w_var=72) == EALIGN           # (the LRT pair's alignment is looked at before the rows)
    assert _launch(h, _desc(lib, hw=(4, 4), pad=1), POOL, False, x=72) == ESHAPE
    assert _launch(h, ok, 15 << 8, False, x=72) == EALIGN
    # the zero border must leave a row and a column
    assert _rc(lib, _desc(lib), (3 << 8) | (3 << 16)) == EINVAL and _rc(lib, _desc(lib), (3 << 8) | (2 << 16)) == 0
    assert _rc(lib, _desc(lib), (6 << 12)) == EINVAL and _rc(lib, _desc(lib), (2 << 12) | (4 << 20)) == EINVAL
    # the 32-bit slab limits: 6 (LRT: 12) bytes per element of a plane below 0x3FFF0000, the weights likewise
    assert _rc(lib, _desc(lib, batch=2048, hw=(74, 74), pad=0, k=1)) == ESHAPE      # 16 * 74 * 74 * 2048 * 6 = 1.0002 * 2^30
    assert _rc(lib, _desc(lib, batch=2048, hw=(73, 73), pad=0, k=1)) == 0
    assert _rc(lib, _desc(lib, batch=2048, hw=(73, 73), pad=0, k=1), lrt=True) == ESHAPE
    assert _rc(lib, _desc(lib, cin=16, hw=(1, 1), k=1, pad=0, cout=1 << 24), OUT_F32) == ESHAPE
    assert _rc(lib, _desc(lib, cin=1 << 20, hw=(1, 1), k=1, pad=0, cout=128, batch=4)) == ESHAPE   # (128 + 128) * 2^20 * 4 bytes of weights
    # draw strides
    x_ps = 16 * 6 * 6 * 8
    assert _rc(lib, _desc(lib, x_draw_stride=3 * x_ps - 8)) == EINVAL and _rc(lib, _desc(lib, x_draw_stride=3 * x_ps)) == 0
    assert _rc(lib, _desc(lib, x_draw_stride=3 * x_ps), lrt=True) == EINVAL and _rc(lib, _desc(lib, x_draw_stride=6 * x_ps), lrt=True) == 0
    assert _rc(lib, _desc(lib, x_draw_stride=3 * x_ps + 4)) == EALIGN
    assert _rc(lib, _desc(lib, w_draw_stride=16 * 9 * 16 + 2)) == EALIGN
    assert _rc(lib, _desc(lib, b_draw_stride=18)) == EALIGN and _rc(lib, _desc(lib, b_draw_stride=18), OUT_F32) == 0
    # work units and steps per launch: either, never both, offsets reduced
    assert _rc(lib, _desc(lib, unit_div=2, unit_off=1, x_unit_mod=2)) == 0 and _rc(lib, _desc(lib, x_unit_div=2, x_unit_off=1)) == 0
    for kw in (dict(unit_div=-1), dict(unit_div=2, unit_off=2), dict(unit_div=2, x_unit_mod=3), dict(x_unit_mod=2), dict(x_unit_div=-1),
               dict(x_unit_div=2, x_unit_off=2), dict(x_unit_off=1), dict(unit_div=2, x_unit_div=2)):
        assert _rc(lib, _desc(lib, **kw)) == EINVAL, kw
    # the grid: (draw, channel tile) groups and workgroups fit an int
    assert _rc(lib, _desc(lib, hw=(1, 1), k=1, pad=0, cout=72, draws=0x7fffffff)) == ESHAPE
    assert _rc(lib, _desc(lib, hw=(1, 1), k=1, pad=0, cout=72, draws=0x3ffffffc)) == 0
    assert _rc(lib, _desc(lib, hw=(1, 1), k=1, pad=0, cout=72, draws=0x3fffffff)) == ESHAPE     # 2^31 - 2 items round up to 2^31 workgroups


def test_the_tile_rule_by_hand(lib):
    """NT = 2 unless forced; 32 images per wave when forced, when B <= 128 (pooled: 32), when the 256-image launch has fewer than 1024
    items, and for LRT; else 64."""
    from bbb_hip import ops
    x = (2, 16, 16, 16, 260)
    assert ops.c8x3_fwd_plan(x, 128, 1) == ("nt2-mt2-s3", 2, 256, 2 * 2 * 256 * 2, 2048)          # 2 draws x 2 tiles x 256 px x 2 = 2048
    assert ops.c8x3_fwd_plan(x, 128, 1, draws=1) == ("nt2-mt2-s3", 2, 256, 1024, 1024)            # exactly 1024
    assert ops.c8x3_fwd_plan(x, 64, 1, draws=1) == ("nt2-mt1-s3", 2, 128, 256 * 3, 768)           # 512 items of 256 images -> 128-image tiles
    assert ops.c8x3_fwd_plan(x, 128, 1, tile=128) == ("nt2-mt1-s3", 2, 128, 2 * 2 * 256 * 3, 3072)
    assert ops.c8x3_fwd_plan((2, 16, 16, 16, 128), 128, 1, draws=40)[0] == "nt2-mt1-s3"            # B <= 128, however large the launch
    assert ops.c8x3_fwd_plan((2, 16, 16, 16, 132), 128, 1, draws=40)[0] == "nt2-mt2-s3"
    assert ops.c8x3_fwd_plan((2, 16, 16, 16, 128), 128, 1, draws=40, tile=256)[0] == "nt2-mt2-s3"
    assert ops.c8x3_fwd_plan(x, 200, 1, nt=3, out_f32=True) == ("nt3-mt2-f32", 3, 256, 2 * 3 * 256 * 2, 3072)
    assert ops.c8x3_fwd_plan(x, 200, 1, nt=4, out_f32=True)[:3] == ("nt4-mt2-f32", 4, 256)
    assert ops.c8x3_fwd_plan(x, 128, 1, lrt=True) == ("lrt-s3", 2, 128, 2 * 2 * 256 * 3, 3072)
    assert ops.c8x3_fwd_plan(x, 128, 1, lrt=True, tile=256, out_f32=True)[:3] == ("lrt-f32", 2, 128)
    # pooled: 32 | 64 images per workgroup, a quarter of the pixels
    assert ops.c8x3_fwd_plan((2, 16, 18, 18, 36), 64, 3, pool=True, draws=40) == ("nt2-mt2-pool", 2, 64, 40 * 64, 2560)
    assert ops.c8x3_fwd_plan((2, 16, 18, 18, 32), 64, 3, pool=True, draws=40)[:3] == ("nt2-mt1-pool", 2, 32)
    assert ops.c8x3_fwd_plan((2, 16, 6, 6, 36), 64, 3, pool=True)[:3] == ("nt2-mt1-pool", 2, 32)


# ---- the one descriptor check: a kernel that reaches past the padded input ----
def test_an_over_reaching_kernel_is_eshape_in_every_entry(lib):
    """h = w = 2, k = 3, stride 2, no padding: h + 2 pad - dil (k - 1) - 1 = -1.  C's division rounds -1 / 2 to 0, which names one
    output row; floor division (conv_desc.out_map) names none.  Every entry that reads a map off the descriptor refuses it."""
    from bbb_hip import conv_desc
    h = lib.lib()
    assert conv_desc.out_map(2, 2, 3, 2, 0, 1) == (0, 0)
    d = _desc(lib, hw=(2, 2), k=3, stride=2, pad=0, draws=1)
    dp = ctypes.byref(d)
    i32 = lambda: ctypes.byref(ctypes.c_int32(0))
    calls = {
        "bbb_conv2d_fwd": lambda: h.bbb_conv2d_fwd(dp, P, P, None, P, None),
        "bbb_lrt_conv2d_fwd": lambda: h.bbb_lrt_conv2d_fwd(dp, P, P, P, None, None, P, None, None, None, 1, 2, 3, 1, None, None),
        "bbb_conv2d_chwn_fwd": lambda: h.bbb_conv2d_chwn_fwd(dp, P, P, None, P, None),
        "bbb_conv2d_chwn_splitk_fwd": lambda: h.bbb_conv2d_chwn_splitk_fwd(dp, P, P, None, P, 1, None, 0, None),
        "bbb_lrt_conv2d_chwn_fwd": lambda: h.bbb_lrt_conv2d_chwn_fwd(dp, P, P, P, None, None, P, None, None, None, 1, 2, 3, 1, None, None),
        "bbb_lrt_conv2d_chwn_splitk_fwd": lambda: h.bbb_lrt_conv2d_chwn_splitk_fwd(dp, P, P, P, None, None, P, None, None, None, 1, 2, 3, 1, None,
                                                                                     1, None, 0, None),
        "bbb_conv2d_chwn_bf16x3_fwd": lambda: h.bbb_conv2d_chwn_bf16x3_fwd(dp, P, P, None, P, 0, None),
        "bbb_conv2d_c8x3_fwd": lambda: h.bbb_conv2d_c8x3_fwd(dp, P, P, None, P, 0, None),
        "bbb_lrt_conv2d_c8x3_fwd": lambda: h.bbb_lrt_conv2d_c8x3_fwd(dp, P, P, P, None, None, P, 1, 2, 3, 1, None, 0, None),
        "bbb_conv2d_chwn_bf16_fwd": lambda: h.bbb_conv2d_chwn_bf16_fwd(dp, P, P, None, P, 0, None),
        "bbb_lrt_conv2d_chwn_bf16_fwd": lambda: h.bbb_lrt_conv2d_chwn_bf16_fwd(dp, P, P, P, None, None, P, None, None, 1, 2, 3, 1, None, 0, None),
        "bbb_im2col_pbj": lambda: h.bbb_im2col_pbj(P, P, dp, None),
        "bbb_input_grad_col2im": lambda: h.bbb_input_grad_col2im(P, 64, 0, None, P, dp, None),
        # the plan queries
        "bbb_conv2d_fwd_plan": lambda: h.bbb_conv2d_fwd_plan(dp, 0, None, None, None, None, None),
        "bbb_conv2d_fwd_plan (lrt)": lambda: h.bbb_conv2d_fwd_plan(dp, 1, None, None, None, None, None),
        "bbb_conv2d_chwn_plan": lambda: h.bbb_conv2d_chwn_plan(dp, 0, 1, 0, None, None, None, None, None),
        "bbb_conv2d_chwn_plan (lrt)": lambda: h.bbb_conv2d_chwn_plan(dp, 1, 1, 0, None, None, None, None, None),
        "bbb_conv2d_chwn_bf16_plan": lambda: h.bbb_conv2d_chwn_bf16_plan(dp, 0, i32(), i32(), i32(), i32()),
        "bbb_lrt_conv2d_chwn_bf16_plan": lambda: h.bbb_lrt_conv2d_chwn_bf16_plan(dp, 0, i32(), i32(), i32()),
        "bbb_conv2d_c8x3_plan": lambda: h.bbb_conv2d_c8x3_plan(dp, 0, 0, None, None, None, None, None),
        "bbb_conv2d_c8x3_plan (lrt)": lambda: h.bbb_conv2d_c8x3_plan(dp, 0, 1, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == ESHAPE, name
    assert {n.split(" ")[0] for n in calls} == {n for n, (_, args) in lib._SIGNATURES.items()
                                                if any(a is ctypes.POINTER(lib.ConvDesc) for a in args)} - {
        "bbb_conv2d_chwn_splitk_scratch", "bbb_conv2d_chwn_dgrad", "bbb_conv2d_chwn_dgrad_plan", "bbb_conv2d_chwn_bf16_dgrad",
        "bbb_conv2d_chwn_bf16_dgrad_plan"}
    cs = ctypes.c_int32(7)
    assert h.bbb_conv2d_chwn_splitk_scratch(dp, 0, ctypes.byref(cs)) == 0 and cs.value == 1       # (reports bytes, not a code: none)
    # the transposed launches read (out_h, out_w) instead: their descriptor is the stride-1 launch over g's map, and the same rule
    # holds for the forward of the map they are asked to write -- a 2 x 2 input under 3 x 3 taps, stride 2, no padding
    g = _desc(lib, hw=(1, 1), k=3, stride=1, pad=2, draws=1)
    gp = ctypes.byref(g)
    assert h.bbb_conv2d_chwn_dgrad(gp, P, P, P, 2, 2, 2, 2, None) == ESHAPE
    assert h.bbb_conv2d_chwn_dgrad_plan(gp, 2, 2, 2, 2, None, None, None, None) == ESHAPE
    assert h.bbb_conv2d_chwn_bf16_dgrad(gp, P, P, P, 2, 2, 2, 2, 0, None) == ESHAPE
    assert h.bbb_conv2d_chwn_bf16_dgrad_plan(gp, 2, 2, 2, 2, 0, None, None, None) == ESHAPE
    assert h.bbb_conv2d_chwn_dgrad_plan(gp, 2, 2, 3, 3, None, None, None, None) == 0              # 3 x 3 does give g's one pixel


# ---- the fp32 transposed launch takes the forward's tile and interleave choice ----
def test_fp32_dgrad_plan_is_the_forward_rule(lib):
    """What the launcher's comment has always claimed ("items and tile choice as the forward launcher makes them"): for the equivalent
    stride-1 launch -- the same pixels, output channels, images and draws, never a split contraction -- ops.fp32_fwd_plan and
    ops.fp32_dgrad_plan agree on images per item, interleaved staging, items and workgroups."""
    from bbb_hip import ops
    rng = random.Random(77)
    seen = set()
    for _ in range(400):
        B = 4 * rng.choice([1, 8, 16, 17, 32, 33, 48, 51, 64, 65, 96, 128])
        cin, cout = rng.choice([3, 16, 64, 65, 192, 200]), rng.choice([4, 16, 64, 100])
        k, dl = rng.choice([1, 2, 3, 5]), rng.choice([1, 2])
        s = rng.choice([(2, 2), (2, 1), (1, 2), (3, 3), (3, 2)])
        H, W = rng.randint(1, 24), rng.randint(1, 24)
        E = rng.choice([1, 2, 10, 40])
        bm, ilv, items, blocks = ops.fp32_dgrad_plan(B, cin, cout, k, k, (H, W), s, dl, E)
        form, fbm, filv, fitems, fblocks, _ = ops.fp32_fwd_plan((E, 4, H, W, B), (1, cin, 4, 1, 1), k_split=1)
        assert (bm, ilv, items, blocks) == (fbm, filv, fitems, fblocks), (B, cin, cout, k, dl, s, H, W, E)
        assert form == "bbb-%d%s" % (bm, "-ilv" if ilv else "")
        seen.add((bm, ilv))
        # the layer's padding does not enter the choice
        if k > 1 and min(H, W) > dl * (k - 1):
            assert ops.fp32_dgrad_plan(B, cin, cout, k, k, (H, W), s, dl, E, padding=dl * (k - 1) // 2)[:3] == (bm, ilv, items)
    assert seen == {(64, True), (64, False), (128, True), (128, False)}, seen


def test_fp32_dgrad_plan_refuses_with_the_launch_entrys_codes(lib):
    h = lib.lib()

    def gdesc(**kw):
        # the stride-1 launch of a 3 x 3 / stride 2 / padding 1 layer's gradient: g [8][4 x 4], dx [4][8 x 8] (pad = 2 - 1)
        d = _desc(lib, batch=4, cin=8, hw=(4, 4), cout=4, k=3, pad=1, draws=1)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def rc(d, up=(2, 2), out=(8, 8)):
        r = h.bbb_conv2d_chwn_dgrad_plan(ctypes.byref(d), up[0], up[1], out[0], out[1], None, None, None, None)
        if r != 0:
            assert h.bbb_conv2d_chwn_dgrad(ctypes.byref(d), P, P, P, up[0], up[1], out[0], out[1], None) == r
        return r

    bm, items = ctypes.c_int32(0), ctypes.c_int64(0)
    assert h.bbb_conv2d_chwn_dgrad_plan(ctypes.byref(gdesc()), 2, 2, 8, 8, ctypes.byref(bm), None, ctypes.byref(items), None) == 0
    assert (bm.value, items.value) == (64, 64)
    assert rc(gdesc()) == 0
    assert rc(gdesc(), up=(1, 1)) == EINVAL and rc(gdesc(), up=(0, 2)) == EINVAL and rc(gdesc(), out=(0, 8)) == EINVAL
    for field, v in (("batch", 0), ("cin", 0), ("h", -1), ("kh", 0), ("stride_w", 2), ("pad_h", -1), ("dil_w", 0), ("draws", 0), ("act", 1),
                     ("pool", 1), ("w_tap_major", 1), ("unit_div", 2), ("unit_div", 1), ("unit_off", 1), ("x_unit_mod", 1), ("x_unit_div", 2),
                     ("x_unit_off", 1), ("b_offset", 4), ("w_row_pitch", 80), ("x_draw_stride", -8), ("w_draw_stride", -8)):
        assert rc(gdesc(**{field: v})) == EINVAL, field
    assert rc(gdesc(batch=6)) == ESHAPE                                   # batch % 4
    assert rc(gdesc(pad_h=3)) == ESHAPE                                   # the layer's padding would be negative
    assert rc(gdesc(), out=(9, 8)) == ESHAPE and rc(gdesc(), out=(6, 8)) == ESHAPE and rc(gdesc(), up=(3, 2)) == ESHAPE
    assert rc(gdesc(batch=1 << 20, cout=1 << 10), out=(7, 7)) == ESHAPE   # dx slab past 32-bit offsets
    assert rc(gdesc(draws=0x7fffffff, cout=65)) == ESHAPE                 # draws x channel tiles past 2^31
    # operand pointers come after the slab limits and before the grid
    d = gdesc()
    assert h.bbb_conv2d_chwn_dgrad(ctypes.byref(d), None, P, P, 2, 2, 8, 8, None) == EINVAL
    assert h.bbb_conv2d_chwn_dgrad(ctypes.byref(d), P, P, 72, 2, 2, 8, 8, None) == EALIGN
    assert h.bbb_conv2d_chwn_dgrad(ctypes.byref(gdesc(batch=6)), None, P, P, 2, 2, 8, 8, None) == ESHAPE
    assert h.bbb_conv2d_chwn_dgrad(ctypes.byref(gdesc(draws=0x7fffffff, cout=65)), P, P, 72, 2, 2, 8, 8, None) == EALIGN


def test_c8x3_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/c8x3_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: ordinary layers, launches around the tile rule's two thresholds, descriptors at the integer limits."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "c8x3_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "c8x3_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[:10:2], out[1:10:2]))
    forms, reasons = [int(v) for v in out[11:31]], [int(v) for v in out[32:37]]
    assert out[10] == "forms" and out[31] == "reasons" and out[37] == "checksum" and len(out[38]) == 16
    assert int(got["cases"]) >= 150000 and min(int(got[k]) for k in ("ok", "einval", "ealign", "eshape")) > 1000
    assert len(forms) == 20 and min(forms) > 0 and min(reasons) > 1000, (forms, reasons)
