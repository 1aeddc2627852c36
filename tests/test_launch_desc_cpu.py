"""What the per-launch wrappers of bbb_hip.ops hand to the C ABI, against tests/golden/launch_desc.json (recorded from the commit the
file names, before the wrappers moved onto bbb_hip.conv_desc; tests/fwd_desc_recorder.py), case by case and for equality -- and
conv_desc.slab_rule / out_map against a few lines of independent arithmetic.  No device."""
import json
import os
import random

import pytest

import fwd_desc_recorder as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_desc.json")
CASES = R.cases()
REFUSED = {"raises": "BBBHipError", "calls": []}
X_DRAW_STRIDE = slice(2 * 56, 2 * 64)       # hex digits of bbb_conv_desc_t::x_draw_stride (14 int32 fields in front of it)

# The inputs on which the wrappers disagreed before they shared one slab rule; no caller in the tree passes them.  The rule takes the
# stricter behaviour; what each case gives now is stated here, not taken from the golden:
#   a slab count of x that fits no form is refused by every wrapper (lrt_conv2d_chwn_forward checked nothing outside x_div,
#   conv2d_chwn_bf16_forward nothing for work units and launched with the strides the arguments implied);
#   one input slab feeding several output slabs has a draw stride of 0 in every wrapper (lrt_conv2d_chwn_forward with n_slabs > 1 on
#   a single slab passed the slab's size: slab e would have read e slabs past the tensor).
CHANGED = {f"{w}/{g}/{name}": REFUSED for g in R.GEOMS
           for w, name in (("lrt-chwn", "bad-slabs"), ("lrt-chwn", "bad-units"), ("lrt-chwn", "bad-units-slice"),
                           ("bf16", "bad-units"), ("bf16", "bad-units-slice"))}
CHANGED.update({f"lrt-chwn/{g}/xshared": "x_draw_stride 0" for g in R.GEOMS})


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_the_table_is_the_recorded_one(golden):
    assert set(golden) == set(CASES)
    assert set(CHANGED) <= set(CASES) and 20 * len(CHANGED) <= len(CASES)         # the restated cases stay a small minority
    kinds = [sum(1 for c in golden.values() if "raises" in c), sum(1 for c in golden.values() if c["calls"])]
    assert min(kinds) > 50, kinds                                                  # refusals and launches are both there


@pytest.mark.parametrize("cid", sorted(CASES))
def test_wrapper_passes_what_the_parent_passed(golden, monkeypatch, cid):
    fn, cfg = CASES[cid]
    got, want = R.record(fn, cfg, monkeypatch), golden[cid]
    if CHANGED.get(cid) is REFUSED:
        assert "raises" not in want and want["calls"], "the parent launched this"
        want = REFUSED
    elif cid in CHANGED:
        strides = {c["desc"][X_DRAW_STRIDE] for c in want["calls"]}
        assert strides == {(16 * 8 * 8 * 8).to_bytes(8, "little").hex()}, "the parent's: one slab's size"
        want = dict(want, calls=[dict(c, desc=c["desc"][:X_DRAW_STRIDE.start] + "0" * 16 + c["desc"][X_DRAW_STRIDE.stop:]) for c in want["calls"]])
    assert got == want


# ---- the slab rule and the output map against independent arithmetic ---------------------------------------------------------
def _reads(d, e):
    """(input slab, weight set) output slab e reads, from the descriptor's fields as include/bbb_hip.h defines them; strides in slabs."""
    if d.unit_div > 1:
        u = d.unit_off + e
        xs, ws = (u % d.x_unit_mod if d.x_unit_mod else e), u // d.unit_div
    elif d.x_unit_div > 1:
        xs, ws = (e + d.x_unit_off) // d.x_unit_div, e
    else:
        xs, ws = e, e
    return xs * (1 if d.x_draw_stride else 0), ws * (1 if d.w_draw_stride else 0)


def _expect(Ex, Ew, units, n_units, x_per_slice, x_div, x_off, n_slabs, lrt):
    """None (refused), or (E, [(input slab, weight set) per output slab])."""
    if units is not None and units[0] > 1:
        S, off = units
        E = n_units
        if Ex != (S if x_per_slice else E):
            return None
        first = off // S                                                   # w holds the sets of the draws the units touch
        return E, [((off + e) % S if x_per_slice else e, 0 if lrt else (off + e) // S - first) for e in range(E)]
    E = (n_slabs if n_slabs is not None else Ex * x_div) if lrt else (Ew if x_div > 1 else max(Ex, Ew))
    if x_div > 1:
        if not 0 <= x_off < x_div or Ex != -(-(E + x_off) // x_div):     # ceil((E + x_off) / x_div) input slabs
            return None
        return E, [((e + x_off) // x_div, 0 if lrt else e) for e in range(E)]
    if Ex not in (1, E) or (not lrt and Ew not in (1, E)):
        return None
    return E, [(e if Ex == E else 0, e if (not lrt and Ew == E) else 0) for e in range(E)]


def test_slab_rule_against_the_arithmetic():
    from bbb_hip import _lib, conv_desc as C
    rnd = random.Random(7)
    seen = {"units": 0, "steps": 0, "plain": 0, "refused": 0}
    for _ in range(6000):
        lrt = rnd.random() < 0.5
        Ex, Ew = rnd.randint(1, 5), (1 if lrt else rnd.randint(1, 5))
        units = rnd.choice([None, None, (1, 0), (2, rnd.randint(0, 5)), (3, rnd.randint(0, 7))])
        n_units, x_per_slice = rnd.randint(1, 5), rnd.random() < 0.4
        x_div, x_off = rnd.choice([1, 1, 2, 3]), rnd.choice([0, 0, 1, 2, 3, -1])
        n_slabs = rnd.choice([None, None, rnd.randint(1, 6)]) if lrt else None
        want = _expect(Ex, Ew, units, n_units, x_per_slice, x_div, x_off, n_slabs, lrt)
        d, _, _ = C.conv_desc(8, 16, (8, 8), 16, (3, 3))
        kw = dict(units=units, n_units=n_units, x_per_slice=x_per_slice, x_div=x_div, x_off=x_off, n_slabs=n_slabs, weights_shared=lrt)
        if want is None:
            with pytest.raises(_lib.BBBHipError):
                C.slab_rule(d, Ex, Ew, **kw)
            seen["refused"] += 1
            continue
        E, xs, ws = C.slab_rule(d, Ex, Ew, **kw)
        assert (E, d.draws) == (want[0], want[0]), kw
        assert [_reads(d, e) for e in range(E)] == want[1], (Ex, Ew, kw)
        assert all(0 <= x < Ex and (d.unit_div or 0 <= w < Ew) for x, w in want[1]), (Ex, Ew, kw)      # inside the operands
        assert xs == (d.x_draw_stride == 0) and ws == (d.w_draw_stride == 0) and (d.b_draw_stride == 0) == ws
        assert not (d.unit_div and d.x_unit_div) and d.unit_off < max(d.unit_div, 1)
        seen["units" if d.unit_div else "steps" if d.x_unit_div else "plain"] += 1
    assert min(seen.values()) > 300, seen


def test_out_map_against_a_count_of_window_positions():
    from bbb_hip import conv_desc as C
    rnd = random.Random(8)
    for _ in range(3000):
        (h, w), (kh, kw), (sh, sw) = [(rnd.randint(1, 12), rnd.randint(1, 12)) for _ in range(3)]
        (ph, pw), (dh, dw) = (rnd.randint(0, 3), rnd.randint(0, 3)), (rnd.randint(1, 3), rnd.randint(1, 3))
        count = lambda n, k, s, p, dl: sum(1 for o in range(0, n + 2 * p, s) if o + dl * (k - 1) < n + 2 * p)   # window starts that fit
        ho, wo = count(h, kh, sh, ph, dh), count(w, kw, sw, pw, dw)
        if ho and wo:
            assert C.out_map(h, w, (kh, kw), (sh, sw), (ph, pw), (dh, dw)) == (ho, wo)
            d, dho, dwo = C.conv_desc(4, 3, (h, w), 5, (kh, kw), (sh, sw), (ph, pw), (dh, dw), draws=2, act="relu")
            assert (dho, dwo) == (ho, wo)
            assert (d.h, d.w, d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w) == (h, w, kh, kw, sh, sw, ph, pw, dh, dw)
            assert (d.x_draw_stride, d.w_draw_stride, d.b_draw_stride, d.draws, d.act) == (3 * h * w * 4, 5 * 3 * kh * kw, 5, 2, 1)
    assert C.out_map(8, 8, 3, 1, 1, 1) == (8, 8) and C.out_map(8, 8, 3, (1, 2), (2, 1), (2, 1)) == (8, 4)


def test_flag_words():
    from bbb_hip import conv_desc as C
    assert C.c8x3_flags(True, 256, (1, 2, 3, 20), nt=3, pool=True) == 1 | 4 | 8 | (3 << 4) | (1 << 8) | (2 << 12) | (3 << 16) | (15 << 20)
    assert C.c8x3_flags(False, 64, (0, 0, 0, 0), pool=False) == 4 and C.c8x3_flags(False, None, (0, 0, 0, 0)) == 0
    with pytest.raises(KeyError):
        C.c8x3_flags(False, 64, (0, 0, 0, 0))                     # an entry without the pooled form has no 64-image tile
    assert C.bf16_flags(True, False, True, True) == 13 and C.bf16_flags() == 0
    assert [C.pool_code(p) for p in (None, (2, 2), (3, 2))] == [0, 1, (3 << 8) | 2] and C.pooled_map(8, 7, (3, 2)) == (3, 3)
