"""CPU-only companions of tests/test_gpu_tail_sweep.py: the contract of the Monte-Carlo tail, loss and uncertainty kernels
(tests/tail_contract.py) held against itself.  The max-first fp32 model's worst error per operation over all cases IS the stored
constant (rounded up to one digit) the device bound is built from; the order the kernels had before breaks that bound on the offset
recipes, so the sweep can see a tail that is not shift-invariant; the slab enumeration of units, groups and shares agrees with a
brute-force loop; the case table covers every entry, recipe, shape and form; and the host-only launch plan (csrc/mc_tail_plan.h)
walks its argument space under the address and undefined-behaviour sanitizers.  No device; only the last two tests need the library."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tail_contract as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
ALL = C.ALL_CASES


@pytest.fixture(scope="module")
def ratios():
    """{case name: ({op: ratio} max-first, {op: ratio} previous order)}; computing them also asserts that no reference holds a NaN,
    is all -inf, or has its -inf anywhere but where the model has them."""
    return {c.name: (C.model_ratios(c), C.model_ratios(c, "present") if c.entry != "uncertainty" else {}) for c in ALL}


def test_constants_are_the_measured_model_errors(ratios):
    worst = {}
    for name, (good, _) in ratios.items():
        for op, r in good.items():
            if r > worst.get(op, (0.0, ""))[0]:
                worst[op] = (r, name)
    print("max-first fp32 model, worst |model - float64| / scale:", {k: (round(v, 3), n) for k, (v, n) in worst.items()})
    assert set(worst) == set(C.MODEL_CONSTANT)
    for op, (r, name) in worst.items():
        assert C.MODEL_CONSTANT[op] == C.round_up_1sf(r), (op, r, name)
    assert C.DEVICE_FACTOR == 4 and C.bound("tail") == 4 * C.MODEL_CONSTANT["tail"]
    assert [C.round_up_1sf(x) for x in (7.61, 0.806, 20.0, 14.2, 3.0001)] == [8.0, 0.9, 20.0, 20.0, 4.0]


# The three offset cases of two classes or more whose values stay inside the bound of 32 in the previous order, all at |off| = 100, where
# one rounding of mx + log se is worth at most 64 units: 17 draws average it (17.0), or a single image never meets the worst (24.0, 22.3).
INSIDE_AT_100 = {"mc_tail-offset+100-17x64x64", "mc_tail_units-offset+100-3x100x1-S4o6", "mc_tail_cb-offset-100-2x100x1"}


def test_previous_order_breaks_the_bound_on_offset_logits(ratios):
    """ls = v - (mx + log se) rounds at ulp(|mx|).  Every offset case of two classes or more breaks the tail bound on its own, at every
    |off|, but for the three cases named in INSIDE_AT_100 (which must stay inside: the list cannot grow stale); with one class ls is 0
    in either order.  The worst case of each (operation, |off|) group breaks the gradients' bounds too.  The max-first model stays
    inside the constant everywhere, offset or not."""
    groups = {}
    for c in ALL:
        good, prev = ratios[c.name]
        assert all(r <= C.MODEL_CONSTANT[op] for op, r in good.items()), (c.name, good)
        if not c.recipe.startswith("offset") or c.entry == "uncertainty":
            continue
        mag = abs(float(c.recipe[6:]))
        if c.C >= 2 and "tail" in prev:
            assert (prev["tail"] > C.bound("tail")) == (c.name not in INSIDE_AT_100), (c.name, prev)
        for op in ("tail", "tail_grad", "elbo_grad"):
            if op in prev:
                groups[(op, mag)] = max(groups.get((op, mag), 0.0), prev[op])
    print("previous order, worst ratio per (operation, |off|):", {k: round(v, 1) for k, v in sorted(groups.items())})
    assert set(groups) == {(op, m) for op in ("tail", "tail_grad", "elbo_grad") for m in (100.0, 1000.0, 1e4)}
    for (op, mag), r in groups.items():
        assert r > C.bound(op), (op, mag, r)
    assert groups[("tail", 1e4)] > 100 * C.bound("tail")


def test_slab_enumeration_against_brute_force():
    forms = set()
    for c in ALL:
        blocks = C.blocks_of(c)
        assert blocks == C.blocks_brute_force(c), c.name
        assert sorted(e for b in blocks for e in b) == list(range(c.slabs)) and any(blocks), c.name      # every slab in one block
        forms.add(c.p.get("form", c.entry))
    # the worked examples of the header: 5 units from offset 1 over 4 slices; a share that starts at draw 3 of a 4-draw step
    ex = C.Case("x", "mc_tail_units", "gauss4", 5, 3, 2, 0, (("form", "mc_tail_units"), ("S", 4), ("off", 1)))
    assert C.blocks_of(ex) == [[3], [0, 4], [1], [2]]
    ex = C.Case("x", "mc_tail_share", "gauss4", 5, 3, 2, 0, (("form", "mc_tail_share"), ("steps", 3), ("draws", 4), ("first_off", 3)))
    assert C.blocks_of(ex) == [[0], [1, 2, 3, 4], []]
    ex = C.Case("x", "mc_tail_units", "gauss4", 1, 3, 2, 0, (("form", "mc_tail_units"), ("S", 5), ("off", 2)))
    assert C.blocks_of(ex) == [[], [], [0], [], []]
    assert forms >= {"mc_tail_units", "mc_tail_groups", "mc_tail_share", "mc_tail", "mc_tail_cb"}


def test_case_table_covers_every_entry_recipe_shape_and_form():
    assert len(C.CASES) >= 60 and len({c.name for c in ALL}) == len(ALL)
    seen = {}
    for c in C.CASES:
        assert c.recipe in C.VALID[C.op_key(c)], c.name
        seen.setdefault(C.op_key(c), set()).add(c.recipe)
        assert c.B in C.BATCHES and c.C in (C.CLASSES_CB if c.batch_innermost else C.CLASSES_BC), c.name
    assert set(seen) == set(C.ENTRIES) | {"uncertainty_normalized"}
    for key, recipes in seen.items():
        assert recipes == set(C.VALID[key]), (key, set(C.VALID[key]) - recipes)
    for entry in ("mc_tail", "uncertainty"):
        own = [c for c in C.CASES if c.entry == entry]
        assert {c.C for c in own} == set(C.CLASSES_BC) and {c.B for c in own} == set(C.BATCHES) and {c.slabs for c in own} == set(C.DRAWS), entry
    for entry in ("mc_tail_cb", "mc_tail_cb_autograd", "elbo_cb_autograd"):
        own = [c for c in C.CASES if c.entry == entry]
        assert {c.C for c in own} == set(C.CLASSES_CB) and {c.B for c in own} == set(C.BATCHES) and {c.slabs for c in own} == set(C.DRAWS), entry
    for entry in ("mc_tail_units", "mc_tail_groups", "mc_tail_share", "step_end"):
        own = [c for c in C.CASES if c.entry == entry]
        assert {c.C for c in own} == set(C.CLASSES_CB) and {c.B for c in own} == set(C.BATCHES), entry
    units = {(c.p["S"], c.p["off"], c.slabs) for c in C.CASES if c.entry == "mc_tail_units"}
    groups = {(c.p["G"], c.p["E"]) for c in C.CASES if c.entry == "mc_tail_groups"}
    shares = {(c.p["steps"], c.p["draws"], c.p["first_off"], c.slabs) for c in C.CASES if c.entry == "mc_tail_share"}
    assert units == set(C.UNITS) and groups == set(C.GROUPS) and shares == set(C.SHARES)
    assert {c.p["form"] for c in C.CASES if c.entry == "step_end"} == {"mc_tail_units", "mc_tail_groups", "mc_tail_share"}
    assert any(c.p["counter0"] < 0 for c in C.CASES if c.entry == "step_end") and any(c.p["add"] == 2 ** 32 - 1 for c in C.CASES if c.entry == "step_end")
    elbo = [c for c in C.CASES if c.entry == "elbo_cb_autograd"]
    assert {c.p["beta_dev"] for c in elbo} == {False, True}
    assert any(((t < 0) | (t >= c.C)).any() for c in elbo for t in [C.targets_of(c)])
    assert {(c.mean_over > 0) for c in C.CASES if c.entry in ("mc_tail", "mc_tail_cb", "mc_tail_units", "mc_tail_groups")} == {False, True}
    unc = [c for c in C.CASES if c.entry == "uncertainty"]
    assert {(c.slabs == 1, c.p["normalized"]) for c in unc} >= {(True, False), (True, True), (False, False), (False, True)}
    assert any(c.entry == "mc_tail_cb" and c.slabs == c.C == c.B == 1 for c in C.CASES)                    # ny = 1
    assert [(c.slabs, c.C, c.B) for c in C.LARGE_CASES] == [(257, 3, 4), (512, 3, 4)]
    # both sides of the keep_max rule of the plan; beyond it more classes than the 4 x 16 of one sweep of the kernel's phase 2
    assert [c.slabs for c in C.EDGE_CASES] == [C.MAX_PER_SLICE // 2, C.MAX_PER_SLICE // 2 + 1] and C.EDGE_CASES[1].C > 64


def test_recipes_are_what_they_say():
    by = {c.recipe: c for c in C.CASES if c.entry == "mc_tail_cb_autograd"}
    for r, c in by.items():
        x = C.rows_of(c)
        assert x.dtype == np.float32 and x.shape == (c.slabs, c.B, c.C) and np.isfinite(x).all()
        assert (C.rows_of(c) == x).all() and C.layout(c, x).shape == (c.slabs, c.C, c.B)
        if r.startswith("offset"):
            assert abs(float(x.mean()) - float(r[6:])) < 3.0
        if r == "ties":
            assert (x == x.flat[0]).all()
    big = next(c for c in C.CASES if c.recipe == "dominant" and c.C >= 7 and c.B >= 3)
    x = C.rows_of(big).astype(np.float64)
    top = np.sort(x, axis=2)
    assert (top[..., -1] - top[..., -2] > 30).all() and len({int(k) for k in x[0].argmax(axis=1)}) > 1
    skew = next(c for c in C.CASES if c.recipe == "draw_skew" and c.slabs >= 10 and c.C >= 7)
    ls = C.log_softmax64(C.rows_of(skew))
    k, b = (np.arange(skew.B) * 7) % skew.C, np.arange(skew.B)
    others = np.delete(ls[:, b, k], skew.slabs // 2, axis=0)
    assert skew.slabs // 2 > 0 and (ls[skew.slabs // 2, b, k] - others.max(axis=0) > 40).all()
    sp = C.rows_of(next(c for c in C.CASES if c.recipe == C.SOFTPLUS_RECIPE and c.C >= 10 and c.B >= 3))
    assert (sp > 20).any() and (sp < 20).any() and sp.min() >= -30 and sp.max() <= 40


def test_checkers_reject_planted_faults():
    ref = np.array([[0.0, -1.0], [-np.inf, -np.inf]])
    assert C.tail_ratio(ref.astype(np.float32), ref) == 0.0
    for bad in (np.array([[0.0, -1.0], [-np.inf, -50.0]]), np.array([[0.0, -np.inf], [-np.inf, -np.inf]]),
                np.array([[np.nan, -1.0], [-np.inf, -np.inf]])):
        with pytest.raises(AssertionError):
            C.tail_ratio(bad, ref)
    with pytest.raises(AssertionError):
        C.tail_ratio(np.full((2, 2), -np.inf), np.full((2, 2), -np.inf))                 # a reference that is all -inf checks nothing
    assert abs(C.tail_ratio(np.array([[0.0, -1.0 - 2.0 * C.U * 30]]), ref[:1]) - 30.0) < 1e-6
    assert C.grad_ratio(np.zeros(3), np.zeros(3)) == 0.0
    with pytest.raises(AssertionError):
        C.grad_ratio(np.array([0.0, 1e-30, 0.0]), np.zeros(3))
    assert abs(C.grad_ratio(np.array([2.0, 1e-3 + 2 * C.U]), np.array([2.0, 1e-3])) - 1.0) < 1e-6


def _lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def test_entries_refuse_before_any_launch():
    """What the plan refuses comes back from the C entries before a launch (addresses are only looked at), and ops' own pre-checks and
    constants state the same limits."""
    lib = _lib()
    from bbb_hip import ops
    h = lib.lib()
    assert (ops.MC_TAIL_MAX_PER_SLICE, ops.MC_TAIL_MAX_DRAWS) == (C.MAX_PER_SLICE, C.MAX_CB_DRAWS)
    a, b = 0x1000, 0x2000
    units = lambda U, S, Bs=4: h.bbb_mc_tail_units(a, U, S, 0, Bs, 3, 0, b, None)
    assert units(641, 1) == C.ESHAPE and units(4096, 6) == C.ESHAPE and units(4097, 8) == C.EINVAL and units(0, 1) == C.EINVAL
    assert units(3, 2 ** 31 - 1, 1) == C.ESHAPE and units(3, 2 ** 25, 64) == C.ESHAPE                      # the image index is an int
    assert h.bbb_mc_tail_cb(a, 513, 4, 3, 0, b, None) == C.EINVAL
    none = (None, 0.0, None, None, 0, None)
    assert h.bbb_mc_tail_groups_step(a, 6, 641, 4, 3, 0, b, *none) == C.ESHAPE
    assert h.bbb_mc_tail_groups_step(a, 7, 640, 4, 3, 0, b, *none) == C.EINVAL                            # more than 4096 slabs
    assert h.bbb_mc_tail_share_step(a, 10, 2, 641, 0, 4, 3, b, *none) == C.ESHAPE
    assert h.bbb_mc_tail_share_step(a, 10, 2, 5, 5, 4, 3, b, *none) == C.EINVAL                           # first_off == draws
    assert h.bbb_mc_tail_share_step(a, 10, 2, 5, 1, 4, 3, b, *none) == C.EINVAL                           # 1 + 10 > 2 * 5
    assert h.bbb_mc_tail_share_step(a + 2, 10, 2, 5, 0, 4, 3, b, *none) == C.EALIGN
    assert h.bbb_mc_tail(a, 2, 4, 1025, 0, b, None) == C.EINVAL and h.bbb_uncertainty(a, 2, 4, 1025, 0, b, b, b, None) == C.EINVAL
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = " ".join(fh.read().split())
    for phrase in ("at most 640 such draws", "draws <= 640", "ceil(units / slices) <= 640", "subtracts a row's maximum before"):
        assert phrase in header, phrase


def test_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/mc_tail_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: ordinary units / groups / shares, then arguments at the 32-bit limits."""
    gxx = shutil.which("g++") or shutil.which("clang++")
    assert gxx is not None, "a host C++ compiler is part of the build environment"
    exe = str(tmp_path / "mc_tail_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "mc_tail_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    # the counts per return code and the checksum of every code and every field of every plan: what the plan answers is pinned, a change
    # of any rule has to be made here too
    assert got == {"cases": "240000", "ok": "108366", "einval": "92961", "ealign": "6185", "eshape": "32488", "checksum": "3bb7872481070639"}, got
