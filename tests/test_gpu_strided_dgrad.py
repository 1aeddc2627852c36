"""Strided convolutions behind the first layer on the training fast path (bbb_hip/fast_train.py), against float64 references on
the CPU -- the tiers, helpers and CONFIGS of test_gpu_train_fuzz.py:

  * kernel sweep: conv2d_chwn_input_grad(stride=...) (the transposed launch bbb_conv2d_chwn_dgrad, csrc/pconv_dgrad.hip) against
    torch.nn.grad.conv2d_input over strides, dilations (gcd(s, d) > 1 included), kernels, paddings 0 / half / full, H != W, maps
    whose floor drops rows and columns, s > d (k - 1) + 1 (input pixels that receive nothing: exact zeros), channel counts up to
    the zoo's 384 / 256, E = 1 / 3 / 10, B = 4 / 8 / 128 / 132, per-draw weights and the LRT shared-weight pair in both of
    fast_train's call forms, w_flipped passed in and not;
  * bitwise invariants: stride-1 calls are the forward launch on the flipped weights; a draw alone equals its slab in an E-draw
    launch (split_k off and on); two identical calls agree;
  * the weight gradient of strided later layers: per-draw x, batch chunks S = 1 / 2 / >= 4, x_squares, wgrad_in_place on / off;
  * generated models (BBB and LRT) with strided later layers: the gate, every parameter gradient and x.grad against float64
    autograd fed the device's Philox noise, six eager train_step calls against three warm-up + three replayed GraphedTrainStep
    steps, bitwise repeatability, the drop-in net(x) loop; and the bf16 refusal.

EXACT tier: small-integer operands, bit for bit against the float64 value.  GAUSSIAN tier: |err| <= _gauss_c(K) * mag per
element, mag = the same gradient of |g|, |w| (|x|).  No element and no case is excluded from either tier.  Run with -m gpu."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import bbb_numpy as O
import ref_port_torch as P

pytestmark = pytest.mark.gpu

CONFIGS = [dict(gemm_mode=m, bf16x3_min_workgroups=0, split_k=sk) for m in ("fp32", "bf16x3") for sk in (False, True)]
C_GAUSS = 2e-5
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"[strided-dgrad worst] {k[0]:<34s} {k[1]:<8s} {WORST[k]:.3e}")


def _gauss_c(K):
    return C_GAUSS * max(1.0, math.sqrt(K / 4096.0))


def _out_hw(H, W, kh, kw, s, p, d):
    return (H + 2 * p[0] - d[0] * (kh - 1) - 1) // s[0] + 1, (W + 2 * p[1] - d[1] * (kw - 1) - 1) // s[1] + 1


def _data(gen, tier, shape, scale=1.0):
    if tier == "exact":
        return torch.randint(-3, 4, shape, generator=gen).float()
    return torch.randn(shape, generator=gen) * scale


def _chwn(t):
    return t.permute(1, 2, 3, 0)


def _check(name, tier, got, want, mag=None, K=None):
    got = got.detach().cpu()
    if tier == "exact":
        w32 = want.float()
        bad = (got != w32)
        assert not bad.any(), f"{name}: {int(bad.sum())} of {got.numel()} elements differ from the exact result; first at " \
                              f"{tuple(int(i) for i in bad.nonzero()[0])}: got {got[bad][0].item()} want {w32[bad][0].item()}"
        _note((name, tier), 0.0)
        return
    err = (got.double() - want).abs()
    c = _gauss_c(K)
    ratio = float((err / (mag + 1e-30)).max())
    _note((name, tier), ratio)
    assert (err <= c * mag + 1e-30).all(), f"{name}: err / mag {ratio:.3e} > {c:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the transposed launch against conv2d_input
# ---------------------------------------------------------------------------------------------------------------------------
def _dg(B, E, Cin, Cout, H, W, kh, kw, s, p=(0, 0), d=(1, 1), form="perdraw", flip=False):
    """form: "perdraw" (w [E, ...]), "shared" (g [E, ...] with ONE weight set: fast_train's two separate LRT launches) or "pair"
    (g [2, ...] = the gradients w.r.t. the mean / variance activations of one draw, weights = the (mean, variance) pair as two
    draws: fast_train's paired LRT launch)."""
    return dict(B=B, E=2 if form == "pair" else E, Cin=Cin, Cout=Cout, H=H, W=W, kh=kh, kw=kw, s=tuple(s), p=tuple(p), d=tuple(d),
                form=form, flip=flip)


STRIDES = [(2, 2), (3, 3), (2, 1), (1, 2), (3, 2), (4, 4)]
KERNELS = [(1, 1), (2, 2), (3, 3), (5, 5), (2, 5)]


def _grid_cases():
    """Every stride x kernel x padding (0, half, full) once, dilations / sizes / forms cycling deterministically."""
    rs = np.random.RandomState(20261016)
    out = {}
    dils = [(1, 1), (2, 2), (3, 3), (2, 1), (1, 3), (3, 2)]
    forms = ["perdraw", "perdraw", "shared", "pair"]
    i = 0
    for s in STRIDES:
        for (kh, kw) in KERNELS:
            for pi, pname in enumerate(("p0", "phalf", "pfull")):
                d = dils[i % len(dils)]
                full = (d[0] * (kh - 1), d[1] * (kw - 1))
                p = ((0, 0), (full[0] // 2, full[1] // 2), full)[pi]
                while True:
                    H, W = int(rs.randint(2, 15)), int(rs.randint(2, 15))
                    ho, wo = _out_hw(H, W, kh, kw, s, p, d)
                    if H != W and ho >= 1 and wo >= 1 and H + 2 * p[0] - d[0] * (kh - 1) - 1 >= 0 and W + 2 * p[1] - d[1] * (kw - 1) - 1 >= 0:
                        break
                form = forms[i % len(forms)]
                E = [1, 3, 2][i % 3]
                Cin, Cout = int(rs.choice([4, 8, 20, 36])), int(rs.choice([4, 5, 12, 33, 70]))
                B = [4, 8, 12, 36][i % 4]
                out[f"s{s[0]}{s[1]}_k{kh}{kw}_d{d[0]}{d[1]}_{pname}"] = _dg(B, E, Cin, Cout, H, W, kh, kw, s, p, d, form, flip=bool(i % 2))
                i += 1
    return out


DGRAD_CASES = {
    # gcd(s, d) > 1: the taps that take part are every tap (s | d) or every second one
    "s2_d2_gcd": _dg(8, 3, 8, 12, 11, 9, 3, 3, (2, 2), (2, 2), (2, 2)),
    "s4_d2_gcd": _dg(4, 1, 4, 8, 13, 10, 3, 5, (4, 4), (1, 3), (2, 2), flip=True),
    "s3_d3_gcd": _dg(8, 2, 8, 8, 12, 14, 2, 3, (3, 3), (0, 2), (3, 3)),
    "s2_d3": _dg(8, 3, 4, 6, 14, 9, 3, 2, (2, 2), (3, 1), (3, 3), flip=True),
    # s > d (k - 1) + 1: input pixels between the taps' reach receive nothing -> exact zeros
    "holes_s3_k1": _dg(8, 3, 8, 16, 10, 7, 1, 1, (3, 3)),
    "holes_s4_k2": _dg(4, 1, 12, 8, 11, 14, 2, 2, (4, 4), (1, 0), form="shared"),
    "holes_s4_k3_floor": _dg(8, 2, 4, 4, 14, 9, 3, 3, (4, 4), (1, 1), flip=True),
    # the forward's floor drops rows and columns (the last input rows receive nothing, or fewer taps)
    "floor_s2_even": _dg(8, 3, 8, 8, 10, 8, 3, 3, (2, 2)),
    "floor_s3_rect": _dg(12, 2, 4, 20, 13, 9, 2, 5, (3, 2), (0, 1)),
    # sizes: the zoo's widest channel counts, many draws, wide and ragged batches
    "c256_to_c384": _dg(4, 1, 256, 384, 5, 4, 3, 3, (2, 2), (1, 1)),
    "c384_to_c256_1x1": _dg(8, 1, 384, 256, 4, 6, 1, 1, (2, 2), flip=True),
    "e10": _dg(8, 10, 8, 16, 9, 7, 3, 3, (2, 2), (1, 1), flip=True),
    "e10_shared": _dg(4, 10, 8, 8, 7, 8, 3, 3, (2, 1), (1, 1), form="shared"),
    "b128": _dg(128, 3, 16, 32, 9, 7, 3, 3, (2, 2), (1, 1)),
    "b132_ragged": _dg(132, 1, 8, 70, 8, 5, 5, 5, (2, 2), (2, 2), flip=True),
    "b128_pair": _dg(128, 1, 32, 64, 6, 8, 3, 3, (2, 2), (1, 1), form="pair"),
    "b132_pair_flip": _dg(132, 1, 8, 12, 7, 5, 2, 2, (2, 2), form="pair", flip=True),
    "bm128_tiles": _dg(256, 3, 8, 64, 12, 10, 3, 3, (2, 2), (1, 1)),          # enough items for the 128-image tile form
    "one_pixel_map": _dg(4, 3, 4, 8, 3, 4, 3, 3, (2, 2), (0, 0)),             # g is one pixel (W = 4: the floor drops a column)
}
DGRAD_CASES.update(_grid_cases())


def _dgrad_ref(c, g, w):
    """float64 per draw: g [E, Cout, Ho, Wo, B], w [Ew, Cout, Cin, kh, kw] (Ew = 1: shared)."""
    geom = dict(stride=c["s"], padding=c["p"], dilation=c["d"])
    return torch.stack([_chwn(conv2d_input((c["B"], c["Cin"], c["H"], c["W"]), w[e if w.shape[0] > 1 else 0], g[e].permute(3, 0, 1, 2), **geom))
                        for e in range(g.shape[0])])


def _dgrad_call(ops, c, gd, wd):
    """The call forms of fast_train: -> [E, Cin, H, W, B]."""
    hw = (c["H"], c["W"])
    if c["form"] == "pair":
        w_t = ops.flip_transpose_w_pair(wd[0:1], wd[1:2]) if c["flip"] else None
        if w_t is None:
            # (fast_train always passes the pair's flipped set; without it the two weight sets are flipped as two draws)
            return ops.conv2d_chwn_input_grad(gd, wd, hw, c["p"], c["d"], stride=c["s"])
        return ops.conv2d_chwn_input_grad(gd, wd[0:1], hw, c["p"], c["d"], w_flipped=w_t, stride=c["s"])
    wf = ops.flip_transpose_w_multi([wd])[0] if c["flip"] else None
    return ops.conv2d_chwn_input_grad(gd, wd, hw, c["p"], c["d"], w_flipped=wf, stride=c["s"])


def test_dgrad_sweep_covers_what_it_claims():
    cs = DGRAD_CASES.values()
    assert {c["s"] for c in cs} >= set(STRIDES)
    assert {(c["kh"], c["kw"]) for c in cs} >= set(KERNELS)
    assert {c["E"] for c in cs} >= {1, 3, 10} and {c["B"] for c in cs} >= {4, 8, 128, 132}
    assert {c["form"] for c in cs} == {"perdraw", "shared", "pair"} and {c["flip"] for c in cs} == {False, True}
    assert any(math.gcd(c["s"][0], c["d"][0]) > 1 and c["d"][0] > 1 for c in cs)
    assert any(c["s"][0] > c["d"][0] * (c["kh"] - 1) + 1 for c in cs)
    assert any((c["H"] + 2 * c["p"][0] - c["d"][0] * (c["kh"] - 1) - 1) % c["s"][0] for c in cs)
    assert any(c["p"] == (c["d"][0] * (c["kh"] - 1), c["d"][1] * (c["kw"] - 1)) and c["kh"] > 1 for c in cs)
    assert all(c["H"] != c["W"] for c in cs)
    assert max(c["Cout"] for c in cs) == 384 and max(c["Cin"] for c in cs) == 384


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(DGRAD_CASES))
def test_strided_dgrad_vs_float64(name, tier):
    from bbb_hip import ops
    c = DGRAD_CASES[name]
    B, E, Cin, Cout, H, W, kh, kw = (c[k] for k in ("B", "E", "Cin", "Cout", "H", "W", "kh", "kw"))
    ho, wo = _out_hw(H, W, kh, kw, c["s"], c["p"], c["d"])
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    w = _data(gen, tier, (1 if c["form"] == "shared" else E, Cout, Cin, kh, kw), 0.3)
    g = _data(gen, tier, (E, Cout, ho, wo, B))
    want = _dgrad_ref(c, g.double(), w.double())
    mag = _dgrad_ref(c, g.double().abs(), w.double().abs()) if tier == "gauss" else None
    gd, wd = g.cuda(), w.cuda()
    for cfg in CONFIGS:
        tag = f"{cfg['gemm_mode']}{'-splitk' if cfg['split_k'] else ''}"
        with ops.use_config(**cfg):
            gx = _dgrad_call(ops, c, gd, wd)
        assert gx.shape == (E, Cin, H, W, B)
        _check(f"strided dgrad[{tag}] {c['form']}", tier, gx, want, mag, Cout * kh * kw)
    # pixels that no tap reaches are exact zeros (+0.0 or -0.0 would both compare equal above: ask for the bits of +0.0)
    rows = [bool(ops.dgrad_tap_plan(ih, ho, kh, c["s"][0], c["p"][0], c["d"][0])) for ih in range(H)]
    cols = [bool(ops.dgrad_tap_plan(iw, wo, kw, c["s"][1], c["p"][1], c["d"][1])) for iw in range(W)]
    dead = ~(torch.tensor(rows)[:, None] & torch.tensor(cols)[None, :])
    if dead.any():
        z = gx.cpu()[:, :, dead, :]
        assert (z.view(torch.int32) == 0).all(), name
        _note(("pixels without a tap: zero bits", tier), 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bitwise invariants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q0", "dil", "c64", "splitk_layer"])
def test_stride1_input_grad_is_the_forward_launch(name):
    """stride 1 (spelled out or defaulted) stays the parent's definition: the forward kernel on the flipped weights."""
    from bbb_hip import ops
    B, E, Cin, Cout, H, W, kh, kw, p, d = {
        "q0": (8, 2, 8, 12, 9, 5, 3, 3, (2, 2), (1, 1)), "dil": (12, 3, 4, 6, 11, 8, 3, 2, (1, 2), (2, 3)),
        "c64": (64, 2, 64, 70, 6, 4, 5, 5, (2, 2), (1, 1)),
        "splitk_layer": (8, 1, 192, 256, 2, 3, 3, 3, (1, 1), (1, 1))}[name]          # few pixels, long contraction: the layer's split
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    ho, wo = _out_hw(H, W, kh, kw, (1, 1), p, d)
    g = torch.randn((E, Cout, ho, wo, B), generator=gen).cuda()
    w = (torch.randn((E, Cout, Cin, kh, kw), generator=gen) * 0.3).cuda()
    q = (d[0] * (kh - 1) - p[0], d[1] * (kw - 1) - p[1])
    for cfg in CONFIGS:
        with ops.use_config(**cfg):
            want = ops.conv2d_chwn_forward(g, ops.flip_transpose_w(w), None, 1, q, d)
            for kwargs in ({}, {"stride": 1}, {"stride": (1, 1)}, {"stride": 1, "w_flipped": ops.flip_transpose_w(w)}):
                got = ops.conv2d_chwn_input_grad(g, w, (H, W), p, d, **kwargs)
                assert torch.equal(got, want), (name, cfg, kwargs)


@pytest.mark.parametrize("name", ["e10", "b128", "c256_to_c384", "s2_d2_gcd", "e10_shared", "holes_s3_k1", "bm128_tiles"])
def test_strided_dgrad_draw_alone_equals_its_slab(name):
    """A draw's gradient does not depend on how many draws share the launch (tile form, item order), with split_k off and on;
    two identical calls agree."""
    from bbb_hip import ops
    c = dict(DGRAD_CASES[name])
    if name == "c256_to_c384":
        c["E"] = 3
    B, E, Cin, Cout, H, W, kh, kw = (c[k] for k in ("B", "E", "Cin", "Cout", "H", "W", "kh", "kw"))
    ho, wo = _out_hw(H, W, kh, kw, c["s"], c["p"], c["d"])
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 5)
    shared = c["form"] == "shared"
    w = (torch.randn((1 if shared else E, Cout, Cin, kh, kw), generator=gen) * 0.3).cuda()
    g = torch.randn((E, Cout, ho, wo, B), generator=gen).cuda()
    outs = []
    for sk in (False, True):
        with ops.use_config(split_k=sk):
            full = ops.conv2d_chwn_input_grad(g, w, (H, W), c["p"], c["d"], stride=c["s"])
            again = ops.conv2d_chwn_input_grad(g, w, (H, W), c["p"], c["d"], stride=c["s"])
            assert torch.equal(full, again), name
            for e in range(E):
                we = w if shared else w[e:e + 1]
                alone = ops.conv2d_chwn_input_grad(g[e:e + 1].contiguous(), we.contiguous(), (H, W), c["p"], c["d"], stride=c["s"])
                assert torch.equal(alone[0], full[e]), (name, sk, e)
        outs.append(full)
    assert torch.equal(outs[0], outs[1]), name                 # the transposed launch is never split


def test_strided_dgrad_refuses_padding_beyond_the_kernel_reach():
    from bbb_hip import ops, _lib
    g = torch.zeros((1, 4, 3, 3, 4), device="cuda")
    w = torch.zeros((1, 4, 4, 1, 1), device="cuda")
    with pytest.raises(_lib.BBBHipError, match="padding larger than the kernel reach"):
        ops.conv2d_chwn_input_grad(g, w, (4, 4), (1, 1), (1, 1), stride=2)
    with pytest.raises(_lib.BBBHipError):                      # x_hw that this layer's forward does not map onto g's 3 x 3
        ops.conv2d_chwn_input_grad(g, w, (9, 5), (0, 0), (1, 1), stride=2)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the weight gradient of strided later layers (per-draw x)
# ---------------------------------------------------------------------------------------------------------------------------
def _wg(B, E, Cin, Cout, H, W, kh, kw, s, p=(0, 0), d=(1, 1), xsq=False):
    return dict(B=B, E=E, Cin=Cin, Cout=Cout, H=H, W=W, kh=kh, kw=kw, s=tuple(s), p=tuple(p), d=tuple(d), xsq=xsq)


WGRAD_CASES = {
    "s22_S1": _wg(8, 3, 64, 70, 9, 7, 3, 3, (2, 2), (1, 1)),
    "s33_S1_inplace_big": _wg(4, 2, 192, 64, 8, 11, 3, 3, (3, 3), (1, 1)),
    "s21_S2": _wg(16, 2, 64, 130, 7, 9, 5, 5, (2, 1), (2, 2)),
    "s12_S4": _wg(64, 1, 8, 12, 9, 6, 3, 3, (1, 2), (1, 1)),
    "s32_S4_ragged": _wg(132, 3, 4, 5, 10, 7, 3, 2, (3, 2), (1, 0)),
    "s44_S8_holes": _wg(128, 1, 8, 8, 13, 10, 2, 2, (4, 4)),
    "s22_dil2_S2": _wg(36, 2, 20, 33, 11, 8, 3, 3, (2, 2), (2, 2), (2, 2)),
    "s22_1x1": _wg(8, 3, 20, 10, 7, 10, 1, 1, (2, 2)),
    "s22_floor_khslice": _wg(8, 2, 8, 16, 10, 8, 3, 3, (2, 2)),             # the role-swapped launch yields kh' > kh rows
    "s25_k25": _wg(12, 1, 8, 10, 9, 14, 2, 5, (2, 2), (1, 2)),
    "xsq_s22_S1": _wg(12, 3, 64, 70, 7, 5, 3, 3, (2, 2), (1, 1), xsq=True),
    "xsq_s33_S2": _wg(20, 2, 20, 33, 10, 8, 3, 3, (3, 3), (1, 2), (1, 2), xsq=True),
    "xsq_s21_S4": _wg(64, 1, 8, 16, 9, 6, 3, 3, (2, 1), (1, 1), xsq=True),
    "xsq_cin6_s22": _wg(8, 1, 6, 16, 9, 7, 3, 3, (2, 2), (1, 1), xsq=True),
}


def test_wgrad_sweep_covers_what_it_claims():
    from bbb_hip import ops
    S = {n: ops.wgrad_batch_chunks(2 * c["E"] if c["xsq"] else c["E"], c["Cout"], (c["Cin"] + 3) & ~3, c["kh"], c["kw"], c["B"])
         for n, c in WGRAD_CASES.items()}
    for xsq in (False, True):
        got = {S[n] for n, c in WGRAD_CASES.items() if c["xsq"] == xsq}
        assert 1 in got and 2 in got and any(s >= 4 for s in got), (xsq, S)
    assert {c["s"] for c in WGRAD_CASES.values()} >= set(STRIDES)


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_strided_later_layer_weight_grad_vs_float64(name, tier):
    from bbb_hip import ops
    c = WGRAD_CASES[name]
    B, E, Cin, Cout, H, W, kh, kw = (c[k] for k in ("B", "E", "Cin", "Cout", "H", "W", "kh", "kw"))
    ho, wo = _out_hw(H, W, kh, kw, c["s"], c["p"], c["d"])
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    Eg = 2 * E if c["xsq"] else E
    x = _data(gen, tier, (E, Cin, H, W, B))
    g = _data(gen, tier, (Eg, Cout, ho, wo, B))
    geom = dict(stride=c["s"], padding=c["p"], dilation=c["d"])

    def ref(g64, x64):
        out = []
        for e in range(Eg):
            xe = x64[e % E].permute(3, 0, 1, 2)
            if c["xsq"] and e >= E:
                xe = xe * xe
            out.append(conv2d_weight(xe, (Cout, Cin, kh, kw), g64[e].permute(3, 0, 1, 2), **geom))
        return torch.stack(out)
    want = ref(g.double(), x.double())
    mag = ref(g.double().abs(), x.double().abs()) if tier == "gauss" else None
    gd, xd = g.cuda(), x.cuda()
    K = B * ho * wo
    for in_place in (False, True):
        for cfg in CONFIGS:
            tag = f"{cfg['gemm_mode']}{'-splitk' if cfg['split_k'] else ''}{'-inplace' if in_place else ''}"
            saved = ops.wgrad_in_place[0]
            ops.wgrad_in_place[0] = in_place
            try:
                with ops.use_config(**cfg):
                    gw = ops.conv2d_chwn_weight_grad(gd, xd, (Eg, Cout, Cin, kh, kw), c["s"], c["p"], c["d"], x_squares=c["xsq"])
            finally:
                ops.wgrad_in_place[0] = saved
            assert gw.shape == (Eg, Cout, Cin, kh, kw)
            _check(f"strided wgrad[{tag}]" + ("-xsq" if c["xsq"] else ""), tier, gw, want, mag, K)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. generated models with strided later layers
# ---------------------------------------------------------------------------------------------------------------------------
def _m(kind, E, B, Cin, H, W, convs, fcs, act="softplus"):
    """convs: (Cout, k, stride, padding, dilation, pool or None); fcs: hidden widths before the 10-way output."""
    return dict(kind=kind, E=E, B=B, Cin=Cin, H=H, W=W, convs=convs, fcs=fcs, act=act)


MODELS = {
    # all-convolutional, two stride-2 layers, no pooling (ReLU: no pool behind it, so no max-pool ties among clipped zeros)
    "bbb_allconv_relu": _m("bbb", 2, 8, 3, 17, 14, [(8, 3, 1, 1, 1, None), (12, 3, 2, 1, 1, None), (16, 3, 2, 0, 1, None)], [20], "relu"),
    "lrt_allconv": _m("lrt", 2, 8, 3, 16, 13, [(8, 3, 1, 1, 1, None), (8, 3, 2, 1, 1, None), (12, 3, 2, 1, 1, None)], []),
    # a stride-2 layer followed by MaxPool2d
    "bbb_s2_pool32": _m("bbb", 3, 8, 3, 20, 17, [(8, 5, 1, 2, 1, None), (12, 3, 2, 1, 1, (3, 2))], [16]),
    "lrt_s2_pool22": _m("lrt", 1, 8, 1, 19, 16, [(8, 3, 1, 0, 1, (2, 2)), (8, 3, 2, 1, 1, (2, 2))], []),
    # a 1x1 / 2 projection and a (2, 1) stride
    "bbb_1x1s2_s21": _m("bbb", 2, 12, 4, 13, 11, [(8, 3, 1, 1, 1, None), (16, 1, 2, 0, 1, None), (8, 3, (2, 1), 1, 1, None)], []),
    "lrt_1x1s2_s21_relu": _m("lrt", 3, 8, 3, 12, 15, [(8, 3, 1, 1, 1, None), (12, 1, 2, 0, 1, None), (8, 3, (2, 1), 1, 1, None)], [12],
                             "relu"),
    # a strided dilated layer; a strided first AND a strided later layer
    "bbb_s2_dil2": _m("bbb", 2, 8, 3, 18, 15, [(8, 3, 1, 1, 1, None), (8, 3, 2, 2, 2, None)], [12]),
    "bbb_first_s2_later_s3": _m("bbb", 3, 8, 3, 23, 20, [(8, 5, 2, 2, 1, None), (12, 3, 3, 1, 1, None)], []),
    "lrt_first_s2_later_s2_dil": _m("lrt", 2, 8, 4, 21, 18, [(8, 3, 2, 1, 1, None), (8, 3, 2, 2, 2, (2, 1))], [16]),
}


def _build(spec):
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    from bbb_hip import ops
    Conv, Linear = (BBB_Conv2d, BBB_Linear) if spec["kind"] == "bbb" else (BBB_LRT_Conv2d, BBB_LRT_Linear)
    Act = nn.ReLU if spec["act"] == "relu" else nn.Softplus
    net = ModuleWrapper()
    cin, H, W = spec["Cin"], spec["H"], spec["W"]
    for i, (cout, k, st, pd, dl, pool) in enumerate(spec["convs"]):
        net.add_module(f"conv{i}", Conv(cin, cout, k, stride=st, padding=pd, dilation=dl, bias=True, priors=P.CONFIG_PRIORS))
        net.add_module(f"act{i}", Act())
        kh, kw = ops._pair(k)
        H, W = _out_hw(H, W, kh, kw, ops._pair(st), ops._pair(pd), ops._pair(dl))
        if pool is not None:
            net.add_module(f"pool{i}", nn.MaxPool2d(pool[0], pool[1]))
            H, W = (H - pool[0]) // pool[1] + 1, (W - pool[0]) // pool[1] + 1
        cin = cout
        assert H >= 1 and W >= 1, spec
    feat = cin * H * W
    net.add_module("flatten", FlattenLayer(feat))
    for j, n in enumerate(spec["fcs"] + [10]):
        net.add_module(f"fc{j}", Linear(feat, n, bias=True, priors=P.CONFIG_PRIORS))
        if j < len(spec["fcs"]):
            net.add_module(f"fact{j}", Act())
        feat = n
    return net


def test_models_cover_what_they_claim():
    from bbb_hip import ops
    later = [(n, c) for n, s in MODELS.items() for c in s["convs"][1:]]
    assert len(MODELS) >= 6 and {s["kind"] for s in MODELS.values()} == {"bbb", "lrt"} and {s["act"] for s in MODELS.values()} == {"relu", "softplus"}
    assert any(sum(ops._pair(c[2]) == (2, 2) for c in s["convs"][1:]) == 2 and all(c[5] is None for c in s["convs"]) for s in MODELS.values())
    assert any(ops._pair(c[2]) == (2, 2) and c[5] is not None for _, c in later)
    assert any(ops._pair(c[1]) == (1, 1) and ops._pair(c[2]) == (2, 2) for _, c in later)
    assert any(ops._pair(c[2]) == (2, 1) for _, c in later)
    assert any(ops._pair(c[2]) != (1, 1) and ops._pair(c[4]) != (1, 1) for _, c in later)
    assert any(ops._pair(s["convs"][0][2]) != (1, 1) and any(ops._pair(c[2]) != (1, 1) for c in s["convs"][1:]) for s in MODELS.values())


def _forward64(net, spec, x64, prm, seed, call0):
    """The model in float64 on the CPU, fed the device's Philox noise (test_gpu_train_fuzz._model_ref's forward; ReLU added):
    prm: name -> float64 tensor (leaves or constants) -> log_outputs [B, 10] of the E-draw logmeanexp."""
    from bbb_hip import ensemble
    from layers.bbb import _BBBLayer
    from layers.lrt import _LRTLayer
    mods = ensemble.flat_children(net)
    pname = {id(m): n for n, m in net.named_modules()}
    KIND = {"W": 0, "bias": 1, "act": 2}
    sp = lambda r: torch.log1p(torch.exp(r))
    outs = []
    for j in range(spec["E"]):
        h = x64
        for m in mods:
            if isinstance(m, (_BBBLayer, _LRTLayer)):
                pre = pname[id(m)]
                Wm, Wr, bm, br = (prm[f"{pre}.{t}"] for t in ("W_mu", "W_rho", "bias_mu", "bias_rho"))
                sid = m._stream_base

                def eps(kind, shape):
                    return torch.from_numpy(O.normal_eps(seed, call0 + j, sid + KIND[kind], int(np.prod(shape))).reshape(shape)).double()

                conv = hasattr(m, "kernel_size")

                def lin(inp, w, b):
                    return F.conv2d(inp, w, b, m.stride, m.padding, m.dilation) if conv else F.linear(inp, w, b)
                if isinstance(m, _BBBLayer):
                    h = lin(h, Wm + eps("W", tuple(Wm.shape)) * sp(Wr), bm + eps("bias", tuple(bm.shape)) * sp(br))
                else:
                    am = lin(h, Wm, bm)
                    av = 1e-16 + lin(h * h, sp(Wr) ** 2, sp(br) ** 2)
                    h = am + torch.sqrt(av) * eps("act", tuple(am.shape))
            elif isinstance(m, nn.Softplus):
                h = F.softplus(h)
            elif isinstance(m, nn.ReLU):
                h = F.relu(h)
            elif isinstance(m, nn.MaxPool2d):
                h = F.max_pool2d(h, m.kernel_size, m.stride)
            else:
                h = h.reshape(-1, m.num_features)
        outs.append(F.log_softmax(h, dim=1))
    return P.logmeanexp(torch.stack(outs, dim=2), 2), mods, pname, sp


def _model_ref(net, spec, x, y, seed, call0, beta, N):
    from layers.bbb import _BBBLayer
    from layers.lrt import _LRTLayer
    leaves = {n: p.detach().cpu().double().requires_grad_(True) for n, p in net.named_parameters()}
    lo, mods, pname, sp = _forward64(net, spec, x.cpu().double(), leaves, seed, call0)
    kl = 0.0
    for m in mods:
        if isinstance(m, (_BBBLayer, _LRTLayer)):
            pre = pname[id(m)]
            for a, b in (("W_mu", "W_rho"), ("bias_mu", "bias_rho")):
                kl = kl + P._kl(m.prior_mu, m.prior_sigma, leaves[f"{pre}.{a}"], sp(leaves[f"{pre}.{b}"]))
    (F.nll_loss(lo, y.cpu()) * N + beta * kl).backward()
    return {n: t.grad for n, t in leaves.items()}


def _model_ref_x(net, spec, x, y, seed, call0, N):
    prm = {n: p.detach().cpu().double() for n, p in net.named_parameters()}
    x64 = x.detach().cpu().double().requires_grad_(True)
    lo = _forward64(net, spec, x64, prm, seed, call0)[0]
    (F.nll_loss(lo, y.cpu()) * N).backward()
    return x64.grad


MODEL_BOUND = {"W_mu": 2e-4, "bias_mu": 2e-4, "W_rho": 2e-4, "bias_rho": 2e-4}
MODEL_BOUND_LRT_RHO = 1e-3
X_BOUND = {"bbb": 2e-4, "lrt": 1e-3}
MODEL_RUNS = [(n, "fp32") for n in MODELS] + [(n, "bf16x3") for n in MODELS if MODELS[n]["kind"] == "bbb"]


def _setup(name, salt=1):
    from bbb_hip import fast_train, rng
    spec = MODELS[name]
    torch.manual_seed(sum(map(ord, name)))
    net = _build(spec).cuda()
    rng.assign_stream_ids(net)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + salt)
    x = torch.rand((spec["B"], spec["Cin"], spec["H"], spec["W"]), generator=gen).cuda()
    y = torch.randint(0, 10, (spec["B"],), generator=gen).cuda()
    assert fast_train.train_path_ok(net, x) == spec["kind"]
    return spec, net, x, y


def _ratio(got, want):
    return float((got.detach().cpu().double() - want).abs().max()) / (float(want.abs().max()) + 1e-30)


@pytest.mark.parametrize("name,mode", MODEL_RUNS, ids=[f"{n}-{m}" for n, m in MODEL_RUNS])
def test_model_gradients_vs_float64_autograd(name, mode):
    from bbb_hip import ensemble, ops, rng
    spec, net, x, y = _setup(name)
    seed, call0, beta, N = 4242, 17, 1e-3, 100.0
    cfg = dict(gemm_mode=mode, bf16x3_min_workgroups=0) if mode == "bf16x3" else {}
    with ops.use_config(**cfg):
        rng.manual_seed(seed, call=call0)
        lo, kl = ensemble.mc_forward(net, x, spec["E"], kl_mode="mean")
        assert ensemble.stats["path"] == "chwn-autograd"
        (F.nll_loss(lo, y) * N + beta * kl).backward()
    want = _model_ref(net, spec, x, y, seed, call0, beta, N)
    fails = []
    for n, p in net.named_parameters():
        kind = n.split(".")[-1]
        ratio = _ratio(p.grad, want[n])
        lrt_rho = spec["kind"] == "lrt" and kind.endswith("rho")
        _note((f"model {spec['kind']} {kind}", mode), ratio)
        bound = MODEL_BOUND_LRT_RHO if lrt_rho else MODEL_BOUND[kind]
        print(f"{name} [{mode}] {n}: {ratio:.3e} (bound {bound:.0e})")
        if not ratio <= bound:
            fails.append((n, ratio, bound))
    assert not fails, fails


@pytest.mark.parametrize("name,mode", MODEL_RUNS, ids=[f"{n}-{m}" for n, m in MODEL_RUNS])
def test_model_input_gradient_vs_float64_autograd(name, mode):
    from bbb_hip import ensemble, ops, rng
    spec, net, x, y = _setup(name, salt=7)
    net.requires_grad_(False)
    seed, call0, N = 4242, 17, 100.0
    cfg = dict(gemm_mode=mode, bf16x3_min_workgroups=0) if mode == "bf16x3" else {}
    xg = x.clone().requires_grad_(True)
    with ops.use_config(**cfg):
        rng.manual_seed(seed, call=call0)
        lo, kl = ensemble.mc_forward(net, xg, spec["E"], kl_mode="mean")
        assert ensemble.stats["path"] == "chwn-autograd"
        (F.nll_loss(lo, y) * N).backward()
    want = _model_ref_x(net, spec, x, y, seed, call0, N)
    r = _ratio(xg.grad, want)
    _note((f"model {spec['kind']} x.grad", mode), r)
    print(f"{name} [{mode}] x.grad: {r:.3e} (bound {X_BOUND[spec['kind']]:.0e})")
    assert r <= X_BOUND[spec["kind"]], r
    assert all(p.grad is None for p in net.parameters())


@pytest.mark.parametrize("name", list(MODELS))
def test_graphed_train_step_equals_eager_steps(name):
    """tests/test_gpu_train.py::test_graphed_train_step_equals_eager_steps on a model with strided later layers: six eager
    train_step calls against three warm-up + three replayed GraphedTrainStep steps (capturable Adam is not bitwise the eager one)."""
    from bbb_hip import rng, train as T
    spec = MODELS[name]
    E, lr, beta, n = spec["E"], 1e-3, 0.1, 1000.0

    def fresh():
        _, net, x, y = _setup(name)
        rng.manual_seed(77, call=0)
        return net, x, y

    net_e, x, y = fresh()
    opt_e = T.FusedAdam(net_e.parameters(), lr=lr)
    eager_losses = [T.train_step(net_e, opt_e, x, y, E, beta, n)[0].item() for _ in range(6)]
    net_g, x, y = fresh()
    opt_g = T.FusedAdam(net_g.parameters(), lr=lr, capturable=True)
    g = T.GraphedTrainStep(net_g, opt_g, x, y, E, beta, n, warmup=3)
    graph_losses = [g.step()[0].item() for _ in range(3)]
    np.testing.assert_allclose(graph_losses, eager_losses[3:], rtol=1e-5)
    for (na, a), (nb, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        np.testing.assert_allclose(b.detach().cpu().numpy(), a.detach().cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=na)
    assert rng.get_state()[1] == 6 * E


@pytest.mark.parametrize("name", list(MODELS))
def test_two_identical_backward_passes_agree_bitwise(name):
    from bbb_hip import ensemble, rng
    spec, net, x, y = _setup(name)
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        rng.manual_seed(7, call=3)
        lo, kl = ensemble.mc_forward(net, xg, spec["E"], kl_mode="mean")
        assert ensemble.stats["path"] == "chwn-autograd"
        (F.nll_loss(lo, y) * 100.0 + 1e-3 * kl).backward()
        runs.append([p.grad.detach().clone() for p in net.parameters()] + [xg.grad.detach().clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("name", list(MODELS))
def test_dropin_loop_takes_the_fast_node_and_matches_it(name):
    """`for j in range(E): net(x)` under autograd is gated on the same function: for these models it now runs the fast node too,
    with the noise calls the per-layer loop used (call0 + j).  Parameter gradients of the loop against mc_forward's, same seed;
    and (as test_gpu_input_grad.py does for its models) mc_forward's x.grad against the loop's -- the drop-in loop does not take
    the fast node for inputs that require a gradient, so that side is the reference-layout path."""
    from bbb_hip import ensemble, rng
    spec, net, x, y = _setup(name, salt=7)
    E, N = spec["E"], 100.0
    grads = []
    for fast in (True, False):
        net.zero_grad(set_to_none=True)
        rng.manual_seed(99, call=5)
        if fast:
            lo, _ = ensemble.mc_forward(net, x, E, kl_mode="mean")
        else:
            outs = [F.log_softmax(net(x)[0], dim=1) for _ in range(E)]
            lo = P.logmeanexp(torch.stack(outs, dim=2), 2)
        (F.nll_loss(lo, y) * N).backward()
        grads.append({n: p.grad.detach().double().cpu() for n, p in net.named_parameters()})
    for n in grads[0]:
        lrt_rho = spec["kind"] == "lrt" and n.endswith("rho")
        r = _ratio(grads[1][n], grads[0][n])
        _note((f"net(x) loop vs mc_forward {spec['kind']}", "fp32"), r)
        assert r <= (MODEL_BOUND_LRT_RHO if lrt_rho else 2e-4), (n, r)
    net.requires_grad_(False)
    xgrads = []
    for fast in (True, False):
        xg = x.clone().requires_grad_(True)
        rng.manual_seed(99, call=5)
        if fast:
            lo, _ = ensemble.mc_forward(net, xg, E, kl_mode="mean")
            assert ensemble.stats["path"] == "chwn-autograd"
        else:
            outs = [F.log_softmax(net(xg)[0], dim=1) for _ in range(E)]
            lo = P.logmeanexp(torch.stack(outs, dim=2), 2)
        (F.nll_loss(lo, y) * N).backward()
        xgrads.append(xg.grad.detach().double().cpu())
    r = _ratio(xgrads[0], xgrads[1])
    _note((f"x.grad vs net(x) loop {spec['kind']}", "fp32"), r)
    assert r <= X_BOUND[spec["kind"]], r


def test_bf16_training_refuses_strided_later_layers():
    from bbb_hip import _lib, train as T
    spec, net, x, y = _setup("bbb_s2_pool32")
    with pytest.raises(_lib.BBBHipError, match="stride-1 convolutions after the first layer"):
        T.forward_loss(net, x, y, spec["E"], 0.1, 1000.0, precision="bf16")
    opt = T.FusedAdam(net.parameters(), lr=1e-3)
    with pytest.raises(_lib.BBBHipError, match="stride-1 convolutions after the first layer"):
        T.train_step(net, opt, x, y, spec["E"], 0.1, 1000.0, precision="bf16")
