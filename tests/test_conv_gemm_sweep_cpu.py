"""CPU-only companions of tests/test_gpu_conv_gemm_sweep.py: the plan query (bbb_conv2d_fwd_plan, the launch entries' own plan)
against the launch rules written out in tests/conv_gemm_contract.py over a seeded sweep, every refusal asked of the entries
themselves, the case table's coverage of the eight instantiations of conv_gemm_kernel and of every tag, the exactness precondition
of the exact tier, the float64 reference against torch.nn.functional.conv2d on float64 tensors, each checker rejecting each planted
fault, and which cases of the older GPU modules reach the 128-pixel tile.  Needs the built library, no device.  (The host-only
walk of csrc/conv_gemm_plan.h under the sanitizers is in tests/test_host_cpu.py.)"""
import ctypes
import os
import random
import subprocess
from dataclasses import replace

import numpy as np
import pytest
import torch

import conv_gemm_contract as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
GOOD = C.GOOD
BBB_PTRS = dict(x=4096, w=8192, bias=12288, y=16384)                       # never read: a refusal comes back before any launch
LRT_PTRS = dict(x=4096, w_mu=8192, w_var=12288, b_mu=16384, b_var=20480, y=24576, act_mu=28672, act_var=32768, eps=36864)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def test_plan_entry_is_exported_and_declared(lib):
    h = lib.lib()
    assert h.bbb_abi_version() == 13 and lib.ABI_VERSION == 13                    # additive: the version stays
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = fh.read()
    assert "bbb_conv2d_fwd_plan" in lib.EXPORTS and hasattr(h, "bbb_conv2d_fwd_plan") and "int bbb_conv2d_fwd_plan(" in header
    none = [None] * 5
    assert h.bbb_conv2d_fwd_plan(None, 0, *none) == C.EINVAL
    assert h.bbb_conv2d_fwd_plan(ctypes.byref(C.conv_desc(lib, GOOD)), 0, *none) == 0                        # null out-pointers
    assert C.plan_query(lib, GOOD, False) == dict(bm=64, linear=False, bk=32, k_tiles=1, grid=(6, 1, 2))      # 5 x 9 pixels x 8 images = 360
    assert C.plan_query(lib, GOOD, True) == dict(bm=64, linear=False, bk=16, k_tiles=2, grid=(6, 1, 2))
    assert len(set(C.FORMS)) == 8


def test_refusals_are_the_launch_entries(lib):
    """Every refusal of csrc/conv_gemm_plan.h by name: plan_rules, the query (where the descriptor alone decides) and the launch
    entry return the same code; the order of the checks."""
    seen = set()
    for name, dchange, pchange, lrt_only in C.refusals():
        for lrt in ((True,) if lrt_only else (False, True)):
            base = LRT_PTRS if lrt else BBB_PTRS
            if any(k not in base for k in pchange):
                continue
            desc, ptrs = dict(GOOD, **dchange), C.with_operands(base, pchange)
            want = C.plan_rules(desc, lrt, ptrs)
            assert want in (C.EINVAL, C.EALIGN, C.ESHAPE), (name, lrt, want)
            if not pchange:
                assert C.plan_query(lib, desc, lrt) == want, (name, lrt)
            else:
                assert isinstance(C.plan_query(lib, desc, lrt), dict), (name, lrt)
            assert C.entry_refusal(lib, desc, lrt, ptrs) == want, (name, lrt)
            seen.add((want, lrt))
    assert seen == {(c, l) for c in (C.EINVAL, C.EALIGN, C.ESHAPE) for l in (False, True)}
    assert C.plan_rules(dict(GOOD, w_draw_stride=72, b_draw_stride=12), False) != C.EINVAL                 # BBB weights per draw
    # the order: the descriptor's EINVAL, its ESHAPE, the operands' EINVAL, the LRT strides, alignment
    null_x, odd_y = dict(LRT_PTRS, x=0), dict(LRT_PTRS, y=24578)
    for desc, ptrs, want in ((dict(GOOD, act=3, kh=12), null_x, C.EINVAL), (dict(GOOD, kh=12), null_x, C.ESHAPE), (GOOD, dict(null_x, y=24578), C.EINVAL),
                             (dict(GOOD, w_draw_stride=72), odd_y, C.EINVAL), (GOOD, dict(odd_y, b_var=0), C.EINVAL), (GOOD, odd_y, C.EALIGN)):
        assert C.plan_rules(desc, True, ptrs) == want == C.entry_refusal(lib, desc, True, ptrs), (desc, ptrs)
    # absent optional operands are no refusal (nothing is launched here: the rules alone)
    assert isinstance(C.plan_rules(GOOD, False, dict(BBB_PTRS, bias=0)), dict)
    assert isinstance(C.plan_rules(GOOD, True, dict(LRT_PTRS, b_mu=0, b_var=0, act_mu=0, act_var=0, eps=0)), dict)


def _sweep_descriptor(rng):
    """Ordinary layers (a fifth linear) with the draws next to the tile rule's threshold, then any refusal or an integer limit."""
    linear = rng.random() < 0.2
    if linear:
        desc = dict(B=rng.randint(1, 3000), Cin=rng.randint(1, 600), H=1, W=1, Cout=rng.randint(1, 200), kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1)
    else:
        desc = dict(B=rng.randint(1, 300), Cin=rng.randint(1, 40), H=rng.randint(1, 33), W=rng.randint(1, 33), Cout=rng.randint(1, 200),
                    kh=rng.randint(1, 5), kw=rng.randint(1, 5), sh=rng.randint(1, 3), sw=rng.randint(1, 3), ph=rng.randint(0, 3),
                    pw=rng.randint(0, 3), dh=rng.randint(1, 2), dw=rng.randint(1, 2))
    desc["draws"] = 1
    ok = C.plan_rules(desc, False)
    if isinstance(ok, dict):
        per = ok["grid"][1] * -(-(ok["grid"][0] * ok["bm"]) // 128)
        desc["draws"] = max(1, -(-rng.choice([1, 50, 766, 767, 768, 769, 1536, 3000]) // per) + rng.choice([-1, 0, 0, 1]))
    desc["act"] = rng.randint(0, 2)
    r = rng.random()
    if r < 0.10:
        desc[rng.choice(C.ZERO_FIELDS)] = rng.choice([1, 2, -1])
    elif r < 0.16:
        desc[rng.choice(["w_draw_stride", "b_draw_stride"])] = rng.choice([1, 64, 2 ** 40])
    elif r < 0.22:
        desc["act"] = rng.choice([-1, 3, 7])
    elif r < 0.40:
        for _ in range(rng.randint(1, 3)):
            desc[rng.choice(["B", "Cin", "H", "W", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "draws"])] = rng.choice(
                [0, -1, 1, 2, 64, 127, 128, 0x6fff, 0x7000, 0x7fff, 0x10000, 2 ** 30, 2 ** 31 - 128, 2 ** 31 - 64, 2 ** 31 - 1, -2 ** 31])
    return desc


def test_plan_agrees_with_the_written_rules(lib):
    """30 000 seeded descriptors x (BBB | LRT): the query == C.plan_rules field by field, refusals included, and the sweep reaches
    all eight instantiations and the three descriptor codes."""
    rng = random.Random(20261021)
    reached, codes = {}, {}
    for _ in range(30000):
        desc, lrt = _sweep_descriptor(rng), rng.random() < 0.5
        got, want = C.plan_query(lib, desc, lrt), C.plan_rules(desc, lrt)
        assert got == want, (desc, lrt, got, want)
        if isinstance(got, dict):
            form = "%s-%d%s" % ("lrt" if lrt else "bbb", got["bm"], "-lin" if got["linear"] else "")
            reached[form] = reached.get(form, 0) + 1
            assert got["grid"][0] * got["bm"] >= desc["B"] and got["k_tiles"] * got["bk"] >= desc["Cin"]
        else:
            codes[got] = codes.get(got, 0) + 1
    assert set(reached) == set(C.FORMS) and min(reached.values()) >= 300, reached
    assert set(codes) == {C.EINVAL, C.ESHAPE} and min(codes.values()) > 1000, codes
    # the rule's edges by hand: 16 draws x 3 channel tiles x 16 pixel tiles = 768
    at = dict(B=7, Cin=3, H=17, W=17, Cout=130, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, draws=16)
    for change, bm, grid in ((dict(), 128, (16, 3, 16)), (dict(draws=15), 64, (32, 3, 15)), (dict(Cout=128), 64, (32, 2, 16)),
                             (dict(Cout=129), 128, (16, 3, 16)), (dict(B=6, draws=17), 64, (28, 3, 17)), (dict(B=6, draws=19), 128, (14, 3, 19))):
        for lrt in (False, True):
            got = C.plan_query(lib, dict(at, **change), lrt)
            assert (got["bm"], got["grid"]) == (bm, grid), (change, got)
    big = dict(B=2 ** 31 - 1, Cin=1, H=1, W=1, Cout=2 ** 31 - 1, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1, draws=2 ** 31 - 1)
    assert C.plan_query(lib, big, False) == dict(bm=128, linear=True, bk=32, k_tiles=1, grid=(2 ** 24, 2 ** 25, 2 ** 31 - 1)) == C.plan_rules(big, False)


def test_every_instantiation_and_tag_is_named_by_a_case(lib):
    """The case table by the library's own query: each case takes the instantiation it was written for, and together the cases reach
    the eight instantiations and every tag of C.wanted_tags()."""
    tags, per_form = set(), {}
    for name, c in C.CASES.items():
        plan = C.plan_query(lib, c.desc, c.lrt)
        assert isinstance(plan, dict) and plan == C.plan_rules(c.desc, c.lrt), (name, plan)
        form = "%s-%d%s" % ("lrt" if c.lrt else "bbb", plan["bm"], "-lin" if plan["linear"] else "")
        assert form == c.form, (name, form)
        tags |= C.case_branches(c, plan)
        per_form.setdefault(form, []).append(name)
        assert c.K <= C.K_MAX and max(C.exact_bits(c)) <= 24, name
        ho, wo = c.out_hw
        assert 4 * 4 * c.E * c.B * c.Cout * ho * wo < 96 * 2 ** 20, name                 # y, two moments and eps stay under 96 MB
    want = C.wanted_tags()
    assert len(want) >= 130 and set(C.FORMS) <= want
    assert want <= tags, sorted(want - tags)
    assert set(per_form) == set(C.FORMS), per_form
    # the threshold's two sides, as the issue states them
    assert C.plan_query(lib, C.CASES["bbb-128-c3"].desc, False)["grid"] == (16, 3, 16)
    assert C.plan_query(lib, C.CASES["lrt-128-lin70"].desc, True) == dict(bm=128, linear=True, bk=16, k_tiles=5, grid=(16, 3, 16))
    p = C.plan_query(lib, C.CASES["bbb-767"].desc, False)
    assert p["bm"] == 64 and -(-p["grid"][0] // 2) * p["grid"][1] * p["grid"][2] == 767


def test_exactness_precondition_and_the_kernels_gather():
    """The exact tier's operands are what exact_bits assumes, so the fp32 emulation (numpy's own summation order) equals the float64
    reference bit for bit; and the emulation's gather -- the kernel's (b, oh, ow) x (ci, r, q) addressing -- is the oracle's im2col."""
    for name in ("bbb-rect", "lrt-rect", "lrt-straddle", "bbb-K98", "lrt-K50", "bbb-pad>reach", "lrt-W1", "bbb-K128-lin"):
        c = C.quiet(C.CASES[name])
        o = C.operands(c, "exact")
        assert np.abs(o["x"]).max() == 2 and (o["x"] == np.round(o["x"])).all()
        assert np.abs(o["w"]).max() == 1 and (o["w"] * 8 == np.round(o["w"] * 8)).all()
        if c.lrt:
            assert 1 / 64 <= o["w_var"].min() and o["w_var"].max() == 0.25 and (o["w_var"] * 64 == np.round(o["w_var"] * 64)).all()
        plan = C.plan_rules(c.desc, c.lrt)
        for ix in range(c.x_slabs):
            assert np.array_equal(C.gather(c, o["x"][ix], plan["bm"], plan["bk"]), C.O.im2col(o["x"][ix], *c.k, c.s, c.p, c.d)[0])
        ref, got = C.reference(c, o), C.emulate_f32(c, o)
        assert C.check_exact(c, got, ref) == got["y"].size * (3 if c.lrt else 1)
    c = C.CASES["lrt-straddle"]
    assert C.reference(c, C.operands(c, "exact"))["zero"].tolist() == [False, True, False]


def test_reference_is_torch_conv2d_in_float64():
    """The float64 reference == torch.nn.functional.conv2d on float64 tensors (both contractions, and mag), to float64 rounding."""
    for name in ("bbb-rect", "lrt-rect", "bbb-pad>reach", "lrt-W1", "bbb-K65", "lrt-K33-lin", "bbb-straddle", "lrt-n%4=3"):
        c = C.CASES[name]
        o = C.operands(c, "rounded")
        ref = C.reference(c, o)
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        for e in range(c.E):
            x = t(o["x"][0 if c.x_shared else e])
            w = t(o["w"] if c.lrt else o["w"][0 if c.w_shared else e])
            b = None if o["b"] is None else t(o["b"] if c.lrt else o["b"][0 if c.bias == "shared" else e])
            conv = lambda x_, w_, b_: torch.nn.functional.conv2d(x_, w_, b_, c.s, c.p, c.d).numpy()
            np.testing.assert_allclose(ref["act_mu"][e], conv(x, w, b), rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(ref["mag"][e], conv(x.abs(), w.abs(), None if b is None else b.abs()), rtol=1e-12, atol=1e-13)
            if c.lrt:
                bv = None if o["b_var"] is None else t(o["b_var"])
                np.testing.assert_allclose(ref["act_var"][e], 1e-16 + conv(x * x, t(o["w_var"]), bv), rtol=1e-12, atol=0)
                z = C.O.normal_eps(C.SEED, C.CALL0 + (c.call_dev or 0) + e, C.STREAM, ref["eps"][e].size).reshape(ref["eps"][e].shape)
                assert np.array_equal(ref["eps"][e], z.astype(np.float64))
                np.testing.assert_allclose(ref["pre"][e], ref["act_mu"][e] + np.sqrt(ref["act_var"][e]) * z, rtol=1e-15)


# ------------------------------------------------------------------------------------------------ planted faults
_LONG = C.Case("fault-long", "bbb-64", 3, 8, 5, 5, 10, (3, 3), E=2, act="relu")                       # K = 72: 3 (BBB) or 5 (LRT) k tiles
_RECT = C.Case("fault-rect", "bbb-64", 3, 3, 9, 7, 10, (3, 2), (2, 1), (1, 2), (1, 2), E=2)
_STRADDLE = C.Case("fault-straddle", "bbb-64", 15, 2, 5, 5, 5, (3, 3), E=2)                           # 9 pixels per image
_lrt = lambda c, **kw: replace(c, name=c.name + "-lrt", form="lrt-64", **kw)
PLANTED = [(f, c, ("exact", "rounded")) for f, cs in (
    ("drop-last-k-tile", (_LONG, _lrt(_LONG))), ("rq-swapped", (_RECT, _lrt(_RECT), _LONG)), ("dhdw-swapped", (_RECT, _lrt(_RECT))),
    ("tile-table-t-2", (_LONG, _lrt(_LONG))), ("image-base", (_STRADDLE, _lrt(_STRADDLE))), ("weight-slab-e-1", (_LONG,)),
    ("bias-wrong-draw", (_LONG, _RECT)), ("var-x-not-squared", (_lrt(_LONG), _lrt(_RECT, sample=False)))) for c in cs]
PLANTED += [("noise-neighbour-lane", _lrt(_LONG), ("rounded",)), ("noise-neighbour-lane", _lrt(_RECT, act="softplus", moments=False), ("rounded",))]


@pytest.mark.parametrize("fault,case,tiers", PLANTED, ids=["%s-%s" % (f, c.name) for f, c, _ in PLANTED])
def test_checkers_reject_planted_faults(fault, case, tiers):
    """The launch in numpy fp32 passes both tiers as it is and fails the tier(s) meant to catch it with one fault planted."""
    assert fault in C.FAULTS and set(f for f, _, _ in PLANTED) == set(C.FAULTS)
    for tier in ("exact", "rounded"):
        c = C.quiet(case) if tier == "exact" else case
        check = C.check_exact if tier == "exact" else C.check_rounded
        o = C.operands(c, tier)
        ref = C.reference(c, o)
        check(c, C.emulate_f32(c, o), ref)
        if tier in tiers:
            with pytest.raises(AssertionError):
                check(c, C.emulate_f32(c, o, fault), ref)


def test_one_ulp_one_element_and_an_unwritten_element_are_seen():
    """The exact tier sees one ulp in one element of y or of either moment, and an element that still holds the sentinel; the rounded
    tier an act_var of a zero slab that is off by an ulp, and the sentinel."""
    c = C.quiet(replace(_lrt(_STRADDLE), zero_slab=1, bias=None))
    o = C.operands(c, "exact")
    ref, got = C.reference(c, o), C.emulate_f32(c, o)
    nan = np.array([C.SENTINEL], np.int32).view(np.float32)[0]
    assert np.isnan(nan)
    for k in ("y", "act_mu", "act_var"):
        for v in (None, nan):
            bad = dict(got, **{k: got[k].copy()})
            bad[k][0, 3, 2, 1, 1] = np.nextafter(bad[k][0, 3, 2, 1, 1], np.float32(1e9)) if v is None else v
            with pytest.raises(AssertionError):
                C.check_exact(c, bad, ref)
    c = replace(c, sample=True)
    o = C.operands(c, "rounded")
    ref, got = C.reference(c, o), C.emulate_f32(c, o)
    assert ref["zero"].tolist() == [False, True] and (got["act_var"][1] == np.float32(1e-16)).all()
    C.check_rounded(c, got, ref)
    for k, v in (("act_var", np.nextafter(np.float32(1e-16), np.float32(1))), ("y", nan), ("act_mu", nan)):
        bad = dict(got, **{k: got[k].copy()})
        bad[k][1, 0, 0, 0, 0] = v
        with pytest.raises(AssertionError):
            C.check_rounded(c, bad, ref)


# ------------------------------------------------------------------------------------------------ what the older modules reach
def _older_cases():
    """(module::test[case], descriptor, lrt) of every launch of conv_gemm_kernel that tests/test_gpu_kernels.py and
    tests/test_gpu_fuzz.py make through ops.conv2d_forward / ops.lrt_conv2d_forward with a fixed case list."""
    import test_gpu_fuzz as F
    import test_gpu_kernels as T
    geo = lambda B, Cin, H, W, Cout, kh, kw, s, p, d, E: dict(B=B, Cin=Cin, H=H, W=W, Cout=Cout, kh=kh, kw=kw, sh=s, sw=s, ph=p, pw=p, dh=d, dw=d, draws=E)
    args = lambda f: next(m.args[1] for m in f.pytestmark if m.name == "parametrize")
    out = []
    for name, cases in (("test_conv2d_against_oracle", T.CONV_CASES), ("test_conv2d_chwn_matches_oracle_and_nchw_kernel", T.CHWN_CASES)):
        out += [("test_gpu_kernels::%s[case%d]" % (name, i), geo(*c[:11]), False) for i, c in enumerate(cases)]
    out += [("test_gpu_kernels::test_linear_against_oracle[%d-%d-%d-%d]" % c, geo(c[0], c[1], 1, 1, c[2], 1, 1, 1, 0, 1, c[3]), False)
            for c in args(T.test_linear_against_oracle)]
    out += [("test_gpu_kernels::test_lrt_moments_and_output[case%d]" % i, geo(B, Cin, H, W, Cout, k, k, s, p, 1, E), True)
            for i, (B, Cin, H, W, Cout, k, s, p, E) in enumerate(args(T.test_lrt_moments_and_output))]
    out += [("test_gpu_kernels::test_conv2d_splitk_matches_the_single_launch[case%d]" % i, geo(B, Cin, H, W, Cout, k, k, s, p, 1, E), False)
            for i, (B, Cin, H, W, Cout, k, s, p, E, _) in enumerate(args(T.test_conv2d_splitk_matches_the_single_launch))]
    for i, (B, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, E, _, _) in enumerate(F.CASES):
        d = dict(B=B, Cin=Cin, H=H, W=W, Cout=Cout, kh=kh, kw=kw, sh=sh, sw=sw, ph=ph, pw=pw, dh=dh, dw=dw, draws=E)
        out += [("test_gpu_fuzz::test_random_geometry_all_kernels[case%d]" % i, d, False),
                ("test_gpu_fuzz::test_random_geometry_lrt_kernels[case%d]" % i, d, True)]
    return out


WIDE_BEFORE = ()


def test_which_older_cases_reach_the_wide_tile(lib):
    """A record, by the library's own query: the fixed cases of the two older modules that launch a <128, *, *> instantiation, and the
    bound they are held to there.  Before this sweep these were the only launches of the 128-pixel tile compared by value at small
    size (profiles/conv_gemm_sweep_notes.md)."""
    older = _older_cases()
    assert len(older) >= 8 + 10 + 5 + 4 + 3 + 48
    wide = tuple(sorted(name for name, desc, lrt in older if C.plan_query(lib, desc, lrt)["bm"] == 128))
    print("\nolder cases on the 128-pixel tile:", *wide, sep="\n  ")
    assert wide == WIDE_BEFORE
