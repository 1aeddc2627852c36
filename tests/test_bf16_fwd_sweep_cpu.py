"""CPU-only companions of tests/test_gpu_bf16_fwd_sweep.py: the case table reaches every form and edge it claims (the library's
own plan query, host only), the exact tier's checker rejects single-term errors, and the one slab combination the launch entry
refuses.  Needs the built library, no device."""
import ctypes
import os
import random
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")

GENERAL = ["general(12,1)", "general(12,2)", "general(12,4)", "general(14,1)", "general(14,2)", "general(22,1,ws)",
           "general(22,1,plain)"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def test_bf16_fwd_sweep_branch_coverage(lib):
    """CASES of test_gpu_bf16_fwd_sweep.py, by ops.bf16_fwd_plan: every case runs the form it was written for; together they reach
    the general kernel's seven instantiations, each in both row orders x both output types and with ragged last tiles in both
    directions (two or more tiles in one), padding up to and beyond d (k - 1) under tap-major rows on the multi-k-group and wave-
    specialised ones, every small-k (ks, nt) pair and pixel-run edge, both pooled forms' windows / strip counts / layouts, the strip8
    and few-output edges, and the slab-addressing variants on each of the six forms.  And over the seeded sweep of
    test_bf16_plan_cpu._sweep_case the plan picks no general instantiation beyond those seven: if it does, the table needs it."""
    import test_gpu_bf16_fwd_sweep as S
    from test_bf16_plan_cpu import _sweep_case
    from bbb_hip import ops
    for name, c in S.CASES.items():
        assert S.form_name(S._plan(c)) == c["want"], (name, S._plan(c))
    tags = set().union(*(S.case_branches(c) for c in S.CASES.values()))
    want = set(ops.BF16_FORMS) - {"general"}
    for g in GENERAL:
        want |= {g, g + ":ragged-both+multi-tile"} | {f"{g}:{r}:{o}" for r in ("ref", "tm") for o in ("f32", "bf16")}
    for g in ("general(12,2)", "general(12,4)", "general(14,2)", "general(22,1,ws)"):
        want |= {g + ":tm-pad=d(k-1)", g + ":tm-pad>d(k-1)"}
    want |= {"general:tm-cin24", "general:dilation2", "general:stride2-nonsquare", "general:15px-short-row"}
    want |= {f"smallk:ks{ks}:nt{nt}" for ks in (2, 5, 8) for nt in (1, 2)}
    want |= {"smallk:run1", "smallk:run>1", "smallk:run-ragged", "smallk:run16", "smallk:ragged-images", "smallk:16px"}
    want |= {"smallk-pool:" + t for t in ("nt1", "nt2", "pool2/2", "pool3/2", "strips1", "strips>1", "column-unused", "out_c8", "out_chwn")}
    want |= {"smallk-poolwin:" + t for t in ("pool2/2", "pool3/2", "strips1", "strips>1", "stride2", "two-image-tiles-ragged", "out_c8",
                                             "out_chwn", "cout6", "cout20", "cout32")}
    want |= {"strip8:" + t for t in ("width%3", "pad0", "pad2", "pad4", "ragged-images", "ragged-channels", "partial-channel-tile", "out_c8")}
    want |= {"fewout:" + t for t in ("K512", "K520", "K1040", "K4100", "K%slice", "cout1", "cout7", "cout16", "ragged-images", "f32", "bf16")}
    assert want <= tags, sorted(want - tags)
    assert set(S.SLAB_CASES) == set(ops.BF16_FORMS)
    for form, name in S.SLAB_CASES.items():
        assert S.CASES[name]["want"].startswith(form) and S._plan(S.CASES[name])[0] == form
    slabs = S.slab_branches()
    assert {f"slab:{f}:{v}" for f in ops.BF16_FORMS for v in ("xshared", "wshared", "nobias", "units", "units-perslice", "xdiv")} == slabs
    # the variants are the ones asked for: off % S != 0, n_units % S != 0, x_off != 0, draws % D != 0
    assert S.OFF_ % S.S_ and S.NU_ % S.S_ and S.XOFF_ and S.SLAB_VARIANTS["xdiv"]["E"] % S.D_
    rng = random.Random(20261018)
    seen = set()
    for _ in range(24000):
        B, cin, H, W, cout, kh, kw, s, p, d, draws, out_f32, tap_major = _sweep_case(rng)
        try:
            plan = ops.bf16_fwd_plan((draws, cin, H, W, B), cout, (cin, kh, kw), s, p, d, out_f32=out_f32, tap_major=tap_major)
        except lib.BBBHipError:
            continue
        if plan[0] == "general":
            seen.add(S.form_name(plan))
    assert seen == set(GENERAL), seen ^ set(GENERAL)


def test_exact_tier_rejects_single_term_errors():
    """The exact tier on a K = 1600 row with bf16 output: a result that lacks ONE product, takes one product from the neighbouring
    tap, or reads one output slab from the wrong input slab is rejected (by both checkers), and the unperturbed result passes --
    what a bound of 2^-8 |want| lets through on such a row."""
    import test_gpu_bf16_fwd_sweep as S
    c = S._c("-", 8, 2, 64, 8, 4, 4, 5, p=2)
    E, cin, cout, B = 2, 64, 8, 8
    gen = torch.Generator().manual_seed(1600)
    x = S._data(gen, "exact", (E, cin, 4, 4, B)).double()
    w = S._data(gen, "exact", (E, cout, cin, 5, 5)).double()
    b = S._data(gen, "exact", (E, cout)).double()
    pre, _ = S.reference64(c, x, w, b, lambda e: e, lambda e: e, E)
    assert cin * 25 >= 1600 and float(pre.abs().max()) < 2 ** 24

    def verdicts(res):
        """(bf16 checker passes, fp32 checker passes) on `res` as the kernel's result."""
        out = []
        for cc, got in ((c, res.float().to(torch.bfloat16)), (dict(c, f32=True), res.float())):
            try:
                S.check(cc, "selftest", "exact", got, pre, None, None)
                out.append(True)
            except AssertionError:
                out.append(False)
        return tuple(out)

    try:
        assert verdicts(pre) == (True, True)
        # output element (slab 1, channel o, pixel (1, 2), image n); tap (r, q) = (2, 1) reads x[.., 1, 1, n], its neighbour (2, 2)
        # reads x[.., 1, 2, n].  Take an element below 256 (every integer there is a bf16 value: no perturbation can round away)
        # whose product is non-zero and differs from the neighbour's
        e, oh, ow, r, q = 1, 1, 2, 2, 1
        ih, iw = oh - 2 + r, ow - 2 + q
        pick = [(o, ci, n) for o in range(cout) for ci in range(cin) for n in range(B)
                if abs(pre[e, o, oh, ow, n]) < 200 and w[e, o, ci, r, q] * x[e, ci, ih, iw, n] != 0 and x[e, ci, ih, iw + 1, n] != x[e, ci, ih, iw, n]]
        o, ci, n = pick[0]
        dropped = pre.clone()
        dropped[e, o, oh, ow, n] -= w[e, o, ci, r, q] * x[e, ci, ih, iw, n]
        assert verdicts(dropped) == (False, False)
        shifted = pre.clone()
        shifted[e, o, oh, ow, n] += w[e, o, ci, r, q] * (x[e, ci, ih, iw + 1, n] - x[e, ci, ih, iw, n])
        assert verdicts(shifted) == (False, False)
        wrong_slab, _ = S.reference64(c, x, w, b, lambda e: 0, lambda e: e, E)          # output slab 1 from input slab 0
        assert torch.equal(wrong_slab[0], pre[0])
        assert verdicts(wrong_slab) == (False, False)
    finally:
        for k in [k for k in S._T_WORST if k[0] == S.PREFIX + "selftest"]:
            S._T_WORST.pop(k)


def test_work_units_and_grouped_steps_do_not_combine(lib):
    """x_unit_div > 1 with unit_div > 1 is the one slab combination bbb_conv2d_chwn_bf16_fwd refuses (BBB_EINVAL), on every form
    alike: the check sits before the form is chosen (pconv_bf16_plan.h:216).  conv2d_chwn_bf16_forward cannot express it."""
    d = lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = 40, 6, 9, 7, 70, 3, 3
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1
    d.draws, d.x_draw_stride, d.w_draw_stride = 4, 6 * 9 * 7 * 40, 70 * 56
    h = lib.lib()
    assert h.bbb_conv2d_chwn_bf16_plan(ctypes.byref(d), 0, None, None, None, None) == 0
    d.unit_div, d.unit_off, d.x_unit_div, d.x_unit_off = 2, 1, 2, 1
    assert h.bbb_conv2d_chwn_bf16_plan(ctypes.byref(d), 0, None, None, None, None) == -1
    assert h.bbb_conv2d_chwn_bf16_fwd(ctypes.byref(d), 64, 64, None, 64, 0, None) == -1          # refused before any launch
