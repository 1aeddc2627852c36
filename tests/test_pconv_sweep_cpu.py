"""CPU-only companions of tests/test_gpu_pconv_sweep.py: the plan query (bbb_conv2d_chwn_plan = ops.fp32_fwd_plan, the launch entries'
own plan) against the launch rules written out in tests/pconv_contract.py over a seeded sweep, the case table's coverage of the
fifteen launch forms and of every plan and kernel edge, the exactness precondition of the exact tier, each checker rejecting the
planted faults it is meant to catch, and a host-only walk of csrc/pconv_plan.h under the address and undefined-behaviour sanitizers.
Needs the built library, no device."""
import ctypes
import os
import random
import re
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import pconv_contract as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def test_plan_entry_is_exported_and_declared(lib):
    from bbb_hip import ops
    h = lib.lib()
    assert h.bbb_abi_version() == 13
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = fh.read()
    assert "bbb_conv2d_chwn_plan" in lib.EXPORTS and hasattr(h, "bbb_conv2d_chwn_plan") and "int bbb_conv2d_chwn_plan(" in header
    assert ops.FP32_FORMS == C.FORMS and len(set(C.FORMS)) == 15
    for i, name in enumerate(("64_ILV", "64", "128_ILV", "128", "SEQ64_ILV", "SEQ64", "SEQ128_ILV", "SEQ128", "CROSS", "POOL", "LRT64_ILV",
                              "LRT64", "LRT_SEQ64", "LRT_CROSS", "LRT_POOL")):
        assert re.search(r"#define BBB_FP32_FORM_%s %d\s" % (name, i), header), name
    none = [None] * 5
    assert h.bbb_conv2d_chwn_plan(None, 0, 1, 1, *none) == C.EINVAL
    good = dict(B=8, Cin=512, H=2, W=2, Cout=10, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1, draws=2, pool=0)
    assert h.bbb_conv2d_chwn_plan(ctypes.byref(C.conv_desc(lib, good)), 0, 2, 1, *none) == 0                  # null out-pointers
    assert C.plan_query(lib, good, False, 2, True)["form"] == "bbb-cross" and C.plan_query(lib, good, True, 2, False)["form"] == "lrt-seq64"


def _launch_refusal(lib, d, lrt, k_split):
    """The launch entry on the same descriptor: a refusal comes back before any launch, so it can be asked without a device.  Operand
    pointers are non-null, aligned and never read."""
    h, p = lib.lib(), 4096
    if lrt:
        return h.bbb_lrt_conv2d_chwn_splitk_fwd(ctypes.byref(d), p, p, p, p, p, p, None, None, None, 1, 0, 0, 1, None, k_split, None, 0, None)
    return h.bbb_conv2d_chwn_splitk_fwd(ctypes.byref(d), p, p, p, p, k_split, None, 0, None)


def test_refusals_are_the_launch_entries(lib):
    """Every refusal the query can give, asked of the launch entries with the same descriptor: the same code."""
    h = lib.lib()
    good = dict(B=8, Cin=512, H=2, W=2, Cout=10, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1, draws=2, pool=0)
    seen = set()
    for change, k_split in ((dict(B=0), 1), (dict(B=6), 1), (dict(kh=4), 1), (dict(H=3, pool=1), 1), (dict(pool=1), 2), (dict(pool=2), 1),
                            (dict(), 3), (dict(Cin=480), 2), (dict(draws=0), 1), (dict(sh=0), 1), (dict(ph=-1), 1),
                            (dict(B=2 ** 26, Cin=1, H=1, W=1), 1), (dict(Cin=2 ** 20, kh=64, kw=64, ph=32, pw=32), 1),
                            (dict(H=2 ** 15, W=2 ** 15, Cin=1), 1), (dict(Cout=2 ** 31 - 1, Cin=1), 1)):
        desc = dict(good, **change)
        for lrt in (False, True):
            d = C.conv_desc(lib, desc)
            rc = h.bbb_conv2d_chwn_plan(ctypes.byref(d), int(lrt), k_split, 0, None, None, None, None, None)
            assert rc in (C.EINVAL, C.ESHAPE), (change, rc)
            assert _launch_refusal(lib, d, lrt, k_split) == rc, (change, lrt)
            seen.add(rc)
    for field, value in (("act", 3), ("unit_div", -1), ("unit_off", 5), ("x_unit_mod", 2), ("x_unit_off", 1), ("w_row_pitch", 3), ("b_offset", -1),
                         ("w_tap_major", 2)):
        d = C.conv_desc(lib, good)
        if field == "unit_off":
            d.unit_div = 3
        setattr(d, field, value)
        for lrt in (False, True):
            rc = h.bbb_conv2d_chwn_plan(ctypes.byref(d), int(lrt), 1, 0, None, None, None, None, None)
            assert rc == C.EINVAL == _launch_refusal(lib, d, lrt, 1), field
    d = C.conv_desc(lib, good)
    d.w_draw_stride = 5                                  # LRT weights are shared by the slabs
    assert h.bbb_conv2d_chwn_plan(ctypes.byref(d), 1, 1, 0, None, None, None, None, None) == C.EINVAL == _launch_refusal(lib, d, True, 1)
    assert seen == {C.EINVAL, C.ESHAPE}


def _sweep_descriptor(rng):
    """Layers next to the split's rule (groups 1..18, k tiles around 16 / 24 / 32) and ordinary ones, with launch sizes next to every
    item-count edge of the plan, image counts on both sides of the "128 declined" rule, pooled launches and refusals mixed in."""
    B = rng.choice([4, 8, 60, 64, 68, 128, 132, 192, 204, 208, 256, 260, 304, 308, 324, 408, 412, 512, 6])
    if rng.random() < 0.5:
        tiles = rng.choice([1, 8, 15, 16, 17, 23, 24, 25, 31, 32, 33, 48])
        cin = 32 * tiles - (rng.randrange(32) if rng.random() < 0.3 else 0)
        ph = rng.choice([1, 1, 2, 3, 4, 16, 17, 18])
        desc = dict(B=B, Cin=max(cin, 1), H=ph, W=rng.choice([1, 1, 1, 2]), Cout=rng.choice([1, 10, 64, 65, 128, 130]), kh=1, kw=1, sh=1, sw=1, ph=0,
                    pw=0, dh=1, dw=1)
        if rng.random() < 0.2:
            desc.update(kh=3, ph=1, Cin=max(1, -(-cin // 3)), dh=rng.choice([1, 2]))
    else:
        desc = dict(B=B, Cin=rng.choice([1, 3, 16, 64, 200]), H=rng.randint(1, 24), W=rng.randint(1, 24), Cout=rng.choice([1, 8, 33, 64, 65, 100, 200]),
                    kh=rng.choice([1, 2, 3, 5]), kw=rng.choice([1, 2, 3]), sh=rng.choice([1, 1, 2, 3]), sw=rng.choice([1, 1, 2]), ph=rng.randint(0, 3),
                    pw=rng.randint(0, 3), dh=rng.choice([1, 1, 2]), dw=rng.choice([1, 1, 2]))
    desc["pool"] = int(rng.random() < 0.15)
    ho, wo = C.out_hw(*(desc[k] for k in ("H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw")))
    per = max(1, ho * wo * -(-B // rng.choice([64, 128])) * -(-desc["Cout"] // 64))
    target = rng.choice([383, 384, 385, 511, 512, 513, 766, 767, 768, 769, 11999, 12000, 12001, 12002, 24001, 50])
    desc["draws"] = max(1, -(-target // per) + rng.choice([-1, 0, 0, 1])) if rng.random() < 0.8 else rng.randint(1, 30)
    return desc


def test_plan_agrees_with_the_written_rules(lib):
    """40 000 seeded descriptors x (BBB | LRT) x (the layer's split | none | a wrong one) x (scratch | none): the query ==
    C.plan_rules field by field, refusals included, and the sweep reaches every form."""
    rng = random.Random(20261018)
    reached, refused = {}, 0
    for _ in range(40000):
        desc = _sweep_descriptor(rng)
        lrt, scratch = rng.random() < 0.5, rng.random() < 0.7
        ks = C.layer_ksplit(desc)
        k_split = rng.choice([ks, ks, ks, 1, ks + 1])
        got, want = C.plan_query(lib, desc, lrt, k_split, scratch), C.plan_rules(desc, lrt, k_split, scratch)
        assert got == want, (desc, lrt, k_split, scratch, got, want)
        if isinstance(got, dict):
            reached[got["form"]] = reached.get(got["form"], 0) + 1
        else:
            refused += 1
    assert set(reached) == set(C.FORMS) and min(reached.values()) >= 50, reached
    assert refused > 1000
    # the rule's edges by hand
    one = dict(B=64, Cin=512, H=1, W=1, Cout=4, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1, pool=0)
    for lrt, draws, form in ((False, 384, "bbb-cross"), (False, 385, "bbb-seq64-ilv"), (True, 512, "lrt-cross"), (True, 513, "lrt-seq64"),
                             (False, 767, "bbb-seq64-ilv"), (False, 12000, "bbb-seq64-ilv"), (False, 12001, "bbb-seq64")):
        assert C.plan_query(lib, dict(one, draws=draws), lrt, 2, True)["form"] == form, (lrt, draws)
    wide = dict(one, B=128, Cin=3)
    for draws, form in ((767, "bbb-64-ilv"), (768, "bbb-128-ilv"), (12000, "bbb-128-ilv"), (12001, "bbb-128")):
        assert C.plan_query(lib, dict(wide, draws=draws), False, 1, True)["form"] == form, draws
    for B, bm in ((132, 64), (192, 64), (196, 128), (260, 64), (304, 64), (308, 128), (408, 64), (412, 128), (68, 128), (128, 128), (516, 128)):
        assert C.plan_query(lib, dict(wide, B=B, draws=3000), False, 1, True)["bm"] == bm, B
    for cin, ks in ((479, 1), (480, 1), (481, 2), (736, 2), (737, 3), (992, 3), (993, 4), (4000, 4)):
        assert C.layer_ksplit(dict(one, Cin=cin)) == ks
        assert C.plan_query(lib, dict(one, Cin=cin, draws=2), False, ks, True)["form"] == ("bbb-cross" if ks > 1 else "bbb-64-ilv")
    assert C.layer_ksplit(dict(one, H=16)) == 2 and C.layer_ksplit(dict(one, H=17)) == 1 and C.layer_ksplit(dict(one, H=8, Cout=65)) == 2
    assert C.layer_ksplit(dict(one, H=9, Cout=65)) == 1


def test_every_form_and_edge_is_named_by_a_case(lib):
    """The case table of tests/pconv_contract.py, by ops.fp32_fwd_plan: each case takes the form it was written for, and together the
    cases reach the fifteen forms, every plan edge, every kernel edge on a BBB and on an LRT case, and every LRT feature with each of
    the three sampling epilogues."""
    tags, per_form = set(), {}
    for name, c in C.CASES.items():
        plan = C.case_plan(c)
        assert plan[0] == c.form, (name, plan)
        assert C.plan_rules(c.desc, c.lrt, plan[5], True)["form"] == c.form and plan[5] == C.layer_ksplit(c.desc), name
        tags |= C.case_branches(c, plan)
        per_form.setdefault(c.form, []).append(name)
    want = C.wanted_tags()
    assert len(want) >= 15 + 12 + 2 * 28 + 3 * 6 + 4
    assert want <= tags, sorted(want - tags)
    assert set(per_form) == set(C.FORMS)
    # operands of a case stay under 256 MB, and the pairs across the cross / SEQ boundary are one layer one item apart
    for name, c in C.CASES.items():
        ho, wo = c.out_hw
        floats = c.x_slabs * c.Cin * c.H * c.W * c.B + c.w_sets * c.Cout * c.Cin * c.k[0] * c.k[1] * (2 if c.lrt else 1) + 4 * c.E * c.Cout * ho * wo * c.B
        assert 4 * floats < 256 * 2 ** 20, (name, floats)
    for a, b in C.PAIRS:
        a, b = C.CASES[a], C.CASES[b]
        assert replace(a, name="", form="", E=0, x=()) == replace(b, name="", form="", E=0, x=()) and b.E == a.E + 1
    # slab addressing of the table: what the kernel computes from (unit_div, unit_off, x_unit_mod, x_unit_div, x_unit_off)
    c = C.CASES["lrt-units"]
    assert [c.slab(e) for e in range(c.E)] == [(0, 0, 24 + 16), (1, 1, 24), (2, 1, 24 + 8), (3, 1, 24 + 16), (4, 2, 24)]
    c = C.CASES["lrt-units-x-per-slice"]
    assert [c.slab(e)[0] for e in range(c.E)] == [1, 2, 0, 1] and c.x_slabs == 3
    c = C.CASES["lrt-k257"]
    assert [c.slab(e)[:2] for e in range(c.E)] == [(0, 0), (1, 1), (1, 2)] and c.x_slabs == 2


def test_exactness_precondition_of_every_case():
    """Integer bits of the largest partial sum + fractional bits of the operands' products <= 24 for both contractions, and the
    operands are what the precondition assumes; no case is left out of the exact tier."""
    for name, c in C.CASES.items():
        assert max(C.exact_bits(c)) <= 24, (name, C.exact_bits(c))
    for name in ("bbb-cross-k4", "lrt-cross-k3", "lrt-pool", "bbb-5x2-s2x1-d2"):
        c = C.CASES[name]
        o = C.operands(c, "exact")
        assert np.abs(o["x"]).max() == 2 and (o["x"] == np.round(o["x"])).all()
        assert np.abs(o["w"]).max() == 1 and (o["w"] * 8 == np.round(o["w"] * 8)).all()
        if o["b"] is not None:
            assert np.abs(o["b"]).max() <= 2 and (o["b"] * 8 == np.round(o["b"] * 8)).all()
        if c.lrt:
            assert 1 / 64 <= o["w_var"].min() and o["w_var"].max() == 0.25 and (o["w_var"] * 64 == np.round(o["w_var"] * 64)).all()
            assert o["b_var"] is None or (o["b_var"].max() <= 0.25 and (o["b_var"] * 64 == np.round(o["b_var"] * 64)).all())
        # ... so the fp32 emulation (numpy's own summation order) is exact too
        r, got = C.reference(c, o), C.forward(c, o, np.float32)
        if not (c.lrt and c.sample) and c.act != "softplus":
            assert (got["y"].astype(np.float64) == r["y"]).all()
        if c.lrt:
            assert (got["act_mu"].astype(np.float64) == r["act_mu"]).all() and (got["act_var"] == r["act_var"].astype(np.float32)).all()


# ------------------------------------------------------------------------------------------------ planted faults
# a launch per fault whose geometry the fault can show on: (case, overrides), and the tier(s) meant to catch it
_PAD = C.Case("fault-pad", "lrt-64-ilv", 8, 5, 6, 6, 10, (3, 3), p=(1, 1), E=2, moments=True, b_offset=16, act="relu")
_UNITS = replace(_PAD, name="fault-units", x=("units", 3, 2, False), E=4)
_ZERO = replace(_PAD, name="fault-zero", zero_slab=1, bias=False)
_SPLIT = C.Case("fault-split", "lrt-cross", 8, 100, 2, 2, 10, (3, 3), p=(1, 1), E=2, moments=True)
_POOL = replace(_PAD, name="fault-pool", pool=True, moments=False, act=None)
_LONG = C.Case("fault-long", "lrt-64-ilv", 8, 40, 5, 5, 10, (3, 3), E=2, moments=True)
_BBB_SPLIT = C.Case("fault-bbb-split", "bbb-cross", 8, 100, 2, 2, 10, (3, 3), p=(1, 1), E=2)
_BBB_POOL = C.Case("fault-bbb-pool", "bbb-pool", 8, 5, 6, 6, 10, (3, 3), p=(1, 1), E=2, pool=True, act="relu")
_BBB_LONG = C.Case("fault-bbb-long", "bbb-64-ilv", 8, 40, 5, 5, 10, (3, 3), E=2)
PLANTED = [("var-pad-tap", _PAD, ("exact", "rounded")), ("var-x-not-squared", _PAD, ("exact", "rounded")), ("no-1e-16", _ZERO, ("exact", "rounded")),
           ("noise-shift", _PAD, ("rounded",)), ("noise-call", _PAD, ("rounded",)), ("local-image", _PAD, ("rounded",)),
           ("local-image", _UNITS, ("rounded",)), ("no-bias-var", _PAD, ("exact", "rounded")), ("drop-last-range", _SPLIT, ("exact", "rounded")),
           ("drop-last-range", _BBB_SPLIT, ("exact", "rounded")), ("pool-skip-pixel", _POOL, ("rounded",)),
           ("pool-skip-pixel", replace(_POOL, sample=False), ("exact", "rounded")), ("pool-skip-pixel", _BBB_POOL, ("exact", "rounded")),
           ("tap-table-256", _LONG, ("exact", "rounded")), ("tap-table-256", _BBB_LONG, ("exact", "rounded"))]


@pytest.mark.parametrize("fault,case,tiers", PLANTED, ids=["%s-%s" % (f, c.name) for f, c, _ in PLANTED])
def test_checkers_reject_planted_faults(fault, case, tiers):
    """The launch in numpy fp32 passes both tiers as it is and fails the tier(s) meant to catch it with one fault planted."""
    assert fault in C.FAULTS and set(f for f, _, _ in PLANTED) == set(C.FAULTS)
    for tier in ("exact", "rounded"):
        check = C.check_exact if tier == "exact" else C.check_rounded
        o = C.operands(case, tier)
        ref = C.reference(case, o)
        check(case, C.emulate_f32(case, o), ref)
        if tier in tiers:
            with pytest.raises(AssertionError):
                check(case, C.emulate_f32(case, o, fault), ref)


def test_one_ulp_and_one_element_are_seen():
    """The exact tier sees one ulp in one element of either moment; the rounded tier an act_var of a zero slab that is off by an ulp."""
    o = C.operands(_ZERO, "exact")
    ref, got = C.reference(_ZERO, o), C.emulate_f32(_ZERO, o)
    for k in ("act_mu", "act_var"):
        bad = dict(got, **{k: got[k].copy()})
        bad[k][0, 3, 2, 1, 5] = np.nextafter(bad[k][0, 3, 2, 1, 5], np.float32(1e9))
        with pytest.raises(AssertionError):
            C.check_exact(_ZERO, bad, ref)
    o = C.operands(_ZERO, "rounded")
    ref, got = C.reference(_ZERO, o), C.emulate_f32(_ZERO, o)
    assert ref["zero"].tolist() == [False, True] and (got["act_var"][1] == np.float32(1e-16)).all()
    got["act_var"][1, 0, 0, 0, 0] = np.nextafter(np.float32(1e-16), np.float32(1))
    with pytest.raises(AssertionError):
        C.check_rounded(_ZERO, got, ref)


def test_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/pconv_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: layers and launches around every threshold of the plan, descriptors at the integer limits."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "pconv_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "pconv_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[:10:2], out[1:10:2]))
    forms = [int(v) for v in out[11:26]]
    assert out[10] == "forms" and out[26] == "checksum" and len(out[27]) == 16
    assert int(got["cases"]) >= 200000 and min(int(got[k]) for k in ("ok", "einval", "eshape")) > 1000
    assert len(forms) == 15 and min(forms) > 1000, forms
