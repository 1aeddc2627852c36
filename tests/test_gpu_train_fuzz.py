"""Seeded sweep of the training backward (bbb_hip/fast_train.py) over the geometries the fast path admits
(fast_train._train_path_static), against float64 references on the CPU:

  * kernel level: conv2d_chwn_input_grad (with / without up-front flipped weights), conv2d_chwn_weight_grad (batch chunks,
    strided first layers whose role-swapped launch yields kh' > kh rows, zero-plane channel padding, shared x, the x_squares
    LRT pair), im2col_pbj (bitwise against F.unfold), conv2d_chwn_weight_grad_shared_input (K slices, the three g_pre pitch
    forms), pool_act_backward_chwn and lrt_pool_act_backward_chwn (overlapping, gapped and floor-dropping pools on H != W, the
    folded LRT combine) -- each under fp32 / bf16x3 and split_k off / on;
  * model level: small generated eligible models (BBB and LRT) whose every parameter gradient from ensemble.mc_forward +
    backward is compared with CPU float64 autograd of the same model fed the device's own Philox noise.

Two tiers.  EXACT: small-integer operands make every product and partial sum exact in fp32 (and in the three-piece bf16
split), so a result must equal the float64 reference cast to fp32 bit for bit whatever the summation order: a dropped,
duplicated or misplaced term cannot hide.  GAUSSIAN: normal operands, |got - want| <= c * mag per element with mag the same
backward on |g|, |x|, |w| (as test_gpu_fuzz.py), which catches lost precision.  Run with -m gpu."""
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
WORST = {}                       # (what, tier) -> worst observed err / bound-scale, printed at the end of the module


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"[train-fuzz worst] {k[0]:<28s} {k[1]:<8s} {WORST[k]:.3e}")


def _gauss_c(K):
    # the fp32 accumulation chains of a contraction of K terms: rounding error grows like sqrt(K) past the 4096 the base
    # bound was set for (wgrad contracts over images x output pixels: tens of thousands of terms on full-size first layers)
    return C_GAUSS * max(1.0, math.sqrt(K / 4096.0))


def _out_hw(H, W, kh, kw, s, p, d):
    return (H + 2 * p[0] - d[0] * (kh - 1) - 1) // s[0] + 1, (W + 2 * p[1] - d[1] * (kw - 1) - 1) // s[1] + 1


# ---------------------------------------------------------------------------------------------------------------------------
# case generators: only what _train_path_static admits
# ---------------------------------------------------------------------------------------------------------------------------
def _conv(B, E, Cin, Cout, H, W, kh, kw, s=(1, 1), p=(0, 0), d=(1, 1), xs=False, xsq=False, flip=False):
    return dict(B=B, E=E, Cin=Cin, Cout=Cout, H=H, W=W, kh=kh, kw=kw, s=tuple(s), p=tuple(p), d=tuple(d), xs=xs, xsq=xsq,
                flip=flip)


def _conv_cases(n, seed):
    """Later layers (stride 1, any dilation, padding 0..d*(k-1)) and strided first layers on Cin % 4 == 0 inputs."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        kh, kw = int(rs.choice([1, 2, 3, 5, 7])), int(rs.choice([1, 2, 3, 5]))
        d = (int(rs.randint(1, 4)), int(rs.randint(1, 4)))
        p = (int(rs.randint(0, d[0] * (kh - 1) + 1)), int(rs.randint(0, d[1] * (kw - 1) + 1)))
        H, W = int(rs.randint(1, 17)), int(rs.randint(1, 17))
        first = rs.rand() < 0.25
        s = (int(rs.randint(2, 5)), int(rs.randint(1, 5))) if first else (1, 1)
        Cin = int(rs.choice([4, 8, 20, 64])) if first else int(rs.choice([4, 6, 8, 20, 64, 192]))
        Cout = int(rs.choice([1, 5, 10, 33, 64, 70, 130]))
        B = int(rs.choice([4, 8, 12, 36, 64, 132]))
        E = int(rs.choice([1, 2, 3]))
        ho, wo = _out_hw(H, W, kh, kw, s, p, d)
        if H == W or ho < 1 or wo < 1:
            continue
        xs = first or bool(rs.rand() < 0.3)
        xsq = (not xs) and bool(rs.rand() < 0.4)
        Eg = 2 * E if xsq else E
        if B * Cin * Cout * ho * wo * kh * kw * Eg > 12e6:             # CPU float64 reference work per case
            continue
        out.append(_conv(B, E, Cin, Cout, H, W, kh, kw, s, p, d, xs, xsq, flip=bool(rs.rand() < 0.5)))
    return out


CONV_CASES = {
    # named edges (each reaches a launcher branch the random draw may miss; see test_host_cpu.py::test_train_fuzz_branch_coverage)
    "q0_rect_dil": _conv(8, 2, 6, 10, 9, 5, 5, 3, p=(8, 4), d=(2, 2), flip=True),          # padding = d*(k-1): q = 0
    "chunks4_perdraw": _conv(64, 1, 8, 12, 5, 7, 3, 3, p=(1, 1)),
    "chunks4_shared": _conv(132, 3, 4, 5, 6, 4, 3, 2, p=(1, 0), xs=True),                 # ragged 33-image chunks
    "chunks2_xsq": _conv(36, 2, 20, 33, 4, 6, 3, 3, p=(1, 2), d=(1, 2), xsq=True),
    "nochunk_xsq": _conv(12, 3, 64, 70, 3, 2, 2, 1, xsq=True),
    "cin6_xsq": _conv(8, 1, 6, 16, 7, 5, 3, 3, p=(1, 1), xsq=True),
    "cin192_nochunk": _conv(4, 1, 192, 64, 3, 4, 3, 3, p=(1, 1), flip=True),
    "first_s2_khslice": _conv(8, 2, 4, 16, 16, 11, 3, 3, s=(2, 2), xs=True),              # kh' = 4, kw' = 4 > 3
    "first_s4_khslice_chunks": _conv(64, 1, 8, 8, 15, 13, 3, 2, s=(4, 3), p=(1, 1), xs=True),
    "first_s3_dil2": _conv(12, 3, 4, 10, 14, 9, 2, 3, s=(3, 2), p=(2, 0), d=(2, 1), xs=True),
    "alexnet_conv1_cin4": _conv(8, 1, 4, 64, 32, 32, 11, 11, s=(4, 4), p=(5, 5), xs=True),
    "x1x1": _conv(4, 2, 8, 3, 1, 1, 1, 1, flip=True),
}
CONV_CASES.update({f"rand{i}": c for i, c in enumerate(_conv_cases(28, 20261016))})


def _shared(B, E, Cin, Cout, H, W, kh, kw, s=(1, 1), p=(0, 0), d=(1, 1), form="contig", prebuilt=False):
    return dict(B=B, E=E, Cin=Cin, Cout=Cout, H=H, W=W, kh=kh, kw=kw, s=tuple(s), p=tuple(p), d=tuple(d), form=form,
                prebuilt=prebuilt)


def _shared_cases(n, seed):
    """First layers on 1..7-channel images (the shared-input weight gradient over an im2col)."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        Cin = int(rs.choice([1, 2, 3, 5, 6, 7]))
        kh, kw = int(rs.randint(1, 12)), int(rs.randint(1, 12))
        s = (int(rs.randint(1, 5)), int(rs.randint(1, 5)))
        d = (int(rs.randint(1, 3)), int(rs.randint(1, 3)))
        p = (int(rs.randint(0, d[0] * (kh - 1) + 1)), int(rs.randint(0, d[1] * (kw - 1) + 1)))
        H, W = int(rs.randint(4, 33)), int(rs.randint(4, 33))
        ho, wo = _out_hw(H, W, kh, kw, s, p, d)
        if H == W or ho < 1 or wo < 1:
            continue
        B, E, Cout = int(rs.choice([4, 8, 12, 16, 32])), int(rs.choice([1, 2, 3])), int(rs.choice([6, 8, 16, 32, 64]))
        if E * Cout * Cin * kh * kw * ho * wo * B > 12e6:
            continue
        form = "view" if (ho * wo * B) % 1024 == 0 else str(rs.choice(["contig", "copy"]))
        out.append(_shared(B, E, Cin, Cout, H, W, kh, kw, s, p, d, form, bool(rs.rand() < 0.5)))
    return out


SHARED_CASES = {
    "alexnet_conv1_32": _shared(16, 2, 3, 64, 32, 32, 11, 11, (4, 4), (5, 5), prebuilt=True),
    "alexnet_conv1_224": _shared(4, 1, 3, 64, 224, 224, 11, 11, (4, 4), (5, 5)),
    "lenet_conv1": _shared(16, 3, 1, 6, 32, 32, 5, 5),
    "pitch_view": _shared(16, 2, 3, 8, 10, 8, 3, 1, form="view"),                 # K = 8 * 8 * 16 = 1024: padded pitch
    "pitch_copy_contig": _shared(16, 1, 5, 16, 9, 9, 2, 2, form="contig"),        # K = 1024, contiguous: copied
    "pitch_copy_strided": _shared(12, 2, 2, 8, 7, 11, 3, 5, (2, 1), (1, 2), form="copy", prebuilt=True),
    "one_slice_odd_pixels": _shared(4, 3, 7, 32, 5, 9, 3, 3, (1, 2), (1, 1), (2, 1)),   # K / 2 % 4 != 0: S = 1
    "rect_11x2": _shared(8, 1, 6, 16, 20, 13, 11, 2, (3, 1), (5, 1), (1, 2)),
}
SHARED_CASES.update({f"rand{i}": c for i, c in enumerate(_shared_cases(16, 20261017))})


def _pool(E, C, H, W, B, k, s, act, shared=False):
    return dict(E=E, C=C, H=H, W=W, B=B, k=k, s=s, act=act, shared=shared)


POOL_CASES = {}
for _i, (_k, _s, _H, _W) in enumerate([(3, 2, 10, 8), (2, 3, 11, 8), (3, 1, 7, 5), (1, 2, 7, 10), (2, 2, 7, 9), (3, 3, 10, 8),
                                        (0, 1, 5, 3), (4, 2, 13, 7)]):
    for _act in ("none", "relu", "softplus"):
        if _k == 0 and _act == "none":
            continue                     # (no pool, no activation: the backward is the identity, nothing launches)
        POOL_CASES[f"k{_k}s{_s}_{_H}x{_W}_{_act}"] = _pool(1 + _i % 3, 4 + _i, _H, _W, 4 * (1 + _i % 3), _k, _s, _act,
                                                            shared=bool(_i % 2))


# ---------------------------------------------------------------------------------------------------------------------------
# branch classification (pure: also run without a GPU, test_host_cpu.py::test_train_fuzz_branch_coverage)
# ---------------------------------------------------------------------------------------------------------------------------
def conv_branches(c):
    from bbb_hip import ops
    Cp = (c["Cin"] + 3) & ~3
    Eg = 2 * c["E"] if c["xsq"] else c["E"]
    S = ops.wgrad_batch_chunks(Eg, c["Cout"], Cp, c["kh"], c["kw"], c["B"])
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    # the role-swapped launch: stride <-> dilation, output rows = taps
    khp = (c["H"] + 2 * c["p"][0] - c["s"][0] * (ho - 1) - 1) // c["d"][0] + 1
    kwp = (c["W"] + 2 * c["p"][1] - c["s"][1] * (wo - 1) - 1) // c["d"][1] + 1
    out = {("wgrad-S1" if S == 1 else "wgrad-S2+") + ("-shared" if c["xs"] else "-perdraw")}
    if S >= 4:
        out.add("wgrad-S4+")
    if (khp, kwp) != (c["kh"], c["kw"]):
        out.add("wgrad-khslice" + ("-S2+" if S > 1 else "-S1"))
    if c["Cin"] % 4:
        out.add("wgrad-cinpad")
    if c["xsq"]:
        out.add("wgrad-xsquares")
    if c["s"] == (1, 1):
        out.add("dgrad-flipped" if c["flip"] else "dgrad-plain")
        if c["p"] == (c["d"][0] * (c["kh"] - 1), c["d"][1] * (c["kw"] - 1)):
            out.add("dgrad-q0")
    return out


def shared_branches(c):
    from bbb_hip import ops
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    K, Jp = ho * wo * c["B"], (c["Cin"] * c["kh"] * c["kw"] + 3) // 4 * 4
    S = ops.shared_input_k_slices(c["E"] * c["Cout"], Jp, K)
    padded = ops.padded_plane_pitch(K) != K
    if c["form"] == "contig":
        form = "gpre-copied" if padded else "gpre-contiguous"
    elif c["form"] == "view":
        form = "gpre-padded-view" if padded else "gpre-contiguous"
    else:
        form = "gpre-copied"
    return {"shared-S1" if S == 1 else "shared-S2+", form, "xk-prebuilt" if c["prebuilt"] else "xk-built"}


def pool_branches(c):
    k, s, H, W = c["k"], c["s"], c["H"], c["W"]
    if k == 0:
        return {"act-only"}
    out = set()
    out.add("overlap" if k > s else ("gap" if k < s else "tiled"))
    if (H - k) % s or (s > k and H % s):
        out.add("floor-rows")
    if (W - k) % s or (s > k and W % s):
        out.add("floor-cols")
    if H != W:
        out.add("h!=w")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def _data(gen, tier, shape, scale=1.0):
    if tier == "exact":
        return torch.randint(-3, 4, shape, generator=gen).float()
    return torch.randn(shape, generator=gen) * scale


def _chwn(t):        # [B, C, H, W] (CPU float64 reference layout) -> [C, H, W, B]
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
# 2a. input and weight gradients of the role-swapped launches
# ---------------------------------------------------------------------------------------------------------------------------
def _conv_ref(c, g, x, w):
    """float64 dgrad / wgrad per draw (CPU): g [E', Cout, Ho, Wo, B], x [Ex, Cin, H, W, B], w [E, Cout, Cin, kh, kw]."""
    B, E, Cin = c["B"], c["E"], c["Cin"]
    geom = dict(stride=c["s"], padding=c["p"], dilation=c["d"])
    gx = []
    if c["s"] == (1, 1):
        for e in range(E):
            gx.append(_chwn(conv2d_input((B, Cin, c["H"], c["W"]), w[e], g[e].permute(3, 0, 1, 2), **geom)))
    gw = []
    for e in range(g.shape[0]):
        xe = x[0 if c["xs"] else e % E].permute(3, 0, 1, 2)
        if c["xsq"] and e >= E:
            xe = xe * xe
        gw.append(conv2d_weight(xe, (c["Cout"], Cin, c["kh"], c["kw"]), g[e].permute(3, 0, 1, 2), **geom))
    return (torch.stack(gx) if gx else None), torch.stack(gw)


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_backward_vs_float64(name, tier):
    from bbb_hip import ops
    c = CONV_CASES[name]
    B, E, Cin, Cout, H, W, kh, kw = (c[k] for k in ("B", "E", "Cin", "Cout", "H", "W", "kh", "kw"))
    ho, wo = _out_hw(H, W, kh, kw, c["s"], c["p"], c["d"])
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    Eg = 2 * E if c["xsq"] else E
    x = _data(gen, tier, (1 if c["xs"] else E, Cin, H, W, B))
    w = _data(gen, tier, (E, Cout, Cin, kh, kw), 0.3)
    g = _data(gen, tier, (Eg, Cout, ho, wo, B))
    x64, w64, g64 = x.double(), w.double(), g.double()
    want_x, want_w = _conv_ref(c, g64, x64, w64)
    mag_x = mag_w = None
    if tier == "gauss":
        mag_x, mag_w = _conv_ref(c, g64.abs(), x64.abs(), w64.abs())
    gd, xd, wd = g.cuda(), x.cuda(), w.cuda()
    K_w = B * ho * wo
    K_x = Cout * kh * kw
    for cfg in CONFIGS:
        tag = f"{cfg['gemm_mode']}{'-splitk' if cfg['split_k'] else ''}"
        with ops.use_config(**cfg):
            if c["s"] == (1, 1):
                g_in = gd[:E]
                wf = ops.flip_transpose_w_multi([wd])[0] if c["flip"] else None
                gx = ops.conv2d_chwn_input_grad(g_in, wd, (H, W), c["p"], c["d"], w_flipped=wf)
                assert gx.shape == (E, Cin, H, W, B)
                _check(f"dgrad[{tag}]", tier, gx, want_x[:E], mag_x, K_x)
            gw = ops.conv2d_chwn_weight_grad(gd, xd, (Eg, Cout, Cin, kh, kw), c["s"], c["p"], c["d"], x_squares=c["xsq"])
            assert gw.shape == (Eg, Cout, Cin, kh, kw)
            _check(f"wgrad[{tag}]" + ("-xsq" if c["xsq"] else ""), tier, gw, want_w, mag_w, K_w)
    if Cin % 4 == 0 and not c["xsq"] and ops.wgrad_batch_chunks(E, Cout, Cin, kh, kw, B) == 1:
        # the option that reads the output gradient in place as a tap-major weight operand (unchunked launches only)
        ops.wgrad_in_place[0] = True
        try:
            gw = ops.conv2d_chwn_weight_grad(gd, xd, (E, Cout, Cin, kh, kw), c["s"], c["p"], c["d"])
        finally:
            ops.wgrad_in_place[0] = False
        _check("wgrad[in-place]", tier, gw, want_w, mag_w, K_w)


# ---------------------------------------------------------------------------------------------------------------------------
# 2b. first layers on few channels: im2col + shared-input weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
def _unfold_pbj(x, c):
    """F.unfold rearranged to im2col_pbj's [Ho * Wo, B, Jp] (j = (ci, r, q), zero pad columns)."""
    cols = F.unfold(x, (c["kh"], c["kw"]), dilation=c["d"], padding=c["p"], stride=c["s"])          # [B, J, L]
    J = cols.shape[1]
    Jp = (J + 3) // 4 * 4
    return F.pad(cols.permute(2, 0, 1), (0, Jp - J))


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(SHARED_CASES))
def test_shared_input_weight_grad_vs_float64(name, tier):
    from bbb_hip import ops
    c = SHARED_CASES[name]
    B, E, Cin, Cout, H, W, kh, kw = (c[k] for k in ("B", "E", "Cin", "Cout", "H", "W", "kh", "kw"))
    ho, wo = _out_hw(H, W, kh, kw, c["s"], c["p"], c["d"])
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    x = _data(gen, tier, (B, Cin, H, W))
    g = _data(gen, tier, (E, Cout, ho, wo, B))
    wshape = (E, Cout, Cin, kh, kw)
    geom = (c["s"], c["p"], c["d"])
    xd = x.cuda()
    xk = ops.im2col_pbj(xd, wshape, *geom)
    want_k = _unfold_pbj(x, c)
    assert xk.shape == want_k.shape and torch.equal(xk.cpu(), want_k), f"{name}: im2col_pbj differs from F.unfold"
    _note(("im2col_pbj", "bitwise"), 0.0)

    def ref(gg, xx):
        return torch.stack([conv2d_weight(xx, (Cout, Cin, kh, kw), gg[e].permute(3, 0, 1, 2), stride=c["s"], padding=c["p"],
                                          dilation=c["d"]) for e in range(E)])
    want = ref(g.double(), x.double())
    mag = ref(g.double().abs(), x.double().abs()) if tier == "gauss" else None
    gd = g.cuda()
    K = ho * wo * B
    if c["form"] == "view":
        g_pre = ops.pool_act_backward_chwn(gd, torch.ones_like(gd), 0, 1, "relu", pad_planes=True)    # g itself, padded pitch
        assert torch.equal(g_pre, gd)
    elif c["form"] == "copy":
        big = torch.zeros((E, Cout, ho, wo, B + 4), device="cuda")
        big[..., :B] = gd
        g_pre = big[..., :B]                                                                           # not contiguous
    else:
        g_pre = gd
    for cfg in CONFIGS:
        with ops.use_config(**cfg):
            gw = ops.conv2d_chwn_weight_grad_shared_input(g_pre, None if c["prebuilt"] else xd, wshape, *geom,
                                                          xk=xk if c["prebuilt"] else None)
        assert gw.shape == wshape
        _check("wgrad_shared_input", tier, gw, want, mag, K)


# ---------------------------------------------------------------------------------------------------------------------------
# 2c. pooling / activation backward (and the LRT split with the folded combine)
# ---------------------------------------------------------------------------------------------------------------------------
def _route(g_in, y, k, s):
    """float64 max-pool backward routed by the activated output y: [E, C, Ho, Wo, B] -> [E, C, H, W, B]."""
    if k == 0:
        return g_in
    E, C, H, W, B = y.shape
    yt = y.permute(0, 4, 1, 2, 3).reshape(E * B, C, H, W).double().requires_grad_(True)
    out = F.max_pool2d(yt, k, s)
    out.backward(g_in.permute(0, 4, 1, 2, 3).reshape(out.shape))
    return yt.grad.reshape(E, B, C, H, W).permute(0, 2, 3, 4, 1)


def _dact(y, act):
    y = y.double()
    if act == "relu":
        return (y > 0).double()
    if act == "softplus":
        return -torch.expm1(-y)                  # sigmoid(v) for y = softplus(v)
    return torch.ones_like(y)


def _pool_inputs(c, tier, gen):
    E, C, H, W, B, k, s = (c[n] for n in ("E", "C", "H", "W", "B", "k", "s"))
    Ho, Wo = ((H - k) // s + 1, (W - k) // s + 1) if k else (H, W)
    Em = 1 if c["shared"] else E
    am = torch.randn((Em, C, H, W, B), generator=gen)
    av = torch.rand((Em, C, H, W, B), generator=gen) * 0.5 + 0.05
    eps = torch.randn((E, C, H, W, B), generator=gen)
    v = am + torch.sqrt(av) * eps                                   # continuous: no ties inside a window except ReLU zeros
    y = {"none": v, "relu": F.relu(v), "softplus": F.softplus(v)}[c["act"]].contiguous()
    g = _data(gen, tier, (E, C, Ho, Wo, B))
    g2 = _data(gen, tier, (E, C, Ho, Wo, B))
    xc = _data(gen, tier, (1 if c["shared"] else E, C, Ho, Wo, B))
    return am, av, y, g, g2, xc


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_pool_act_backward_vs_float64(name, tier):
    from bbb_hip import ops
    c = POOL_CASES[name]
    k, s, act = c["k"], c["s"], c["act"]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    am, av, y, g, g2, xc = _pool_inputs(c, tier, gen)
    a = None if act == "none" else act
    exact = tier == "exact" and act != "softplus"       # softplus' derivative is a transcendental: a relative bound instead

    def close(what, got, want, rtol, exact):
        got = got.detach().cpu().double()
        if exact:
            _check(what, "exact", got.float(), want)
            return
        scale = float(want.abs().max()) + 1e-30
        rel = (got - want).abs() / (want.abs() + 1e-3 * scale)
        _note((what, tier if act != "softplus" else "softplus"), float(rel.max()))
        assert (rel <= rtol).all(), f"{what}: relative error {float(rel.max()):.3e} > {rtol:.1e}"

    yd = y.cuda()
    # plain layers: routed by y, times the activation's derivative recovered from y
    want = _route(g.double(), y, k, s) * _dact(y, a)
    for pad in (False, True):
        close("pool_act_bwd", ops.pool_act_backward_chwn(g.cuda(), yd, k, s, a, pad_planes=pad), want, 2e-5, exact)
    # LRT layers: (g + 2 x g2) formed inside, then d/d act_mu and d/d act_var
    g_in = g.double() + 2.0 * xc.double() * g2.double()
    g_mu = _route(g_in, y, k, s) * _dact(y, a)
    y64 = y.double()
    v = torch.where(y64 > 20.0, y64, y64 + torch.log(-torch.expm1(-y64))) if a == "softplus" else y64
    g_var = g_mu * (v - am.double()) / (2.0 * av.double())
    comb = (xc.cuda(), g2.cuda())
    args = (g.cuda(), yd, am.cuda(), av.cuda(), k, s, a)
    outs = [ops.lrt_pool_act_backward_chwn(*args, combine=comb),
            ops.lrt_pool_act_backward_chwn(*args, pad_planes=True, combine=comb),
            ops.lrt_pool_act_backward_chwn(*args, stacked=True, combine=comb)]
    for gm, gv in outs:
        close("lrt_pool_act_bwd g_mu", gm, g_mu, 2e-5, exact)
        # (v - act_mu) / (2 act_var) in fp32 from the recovered v: a few roundings; softplus' inverse v = y + log(-expm1(-y)) in
        # fp32 loses relative accuracy where it saturates towards 0, and v - act_mu cancels (test_gpu_fast_train.py allows 2e-3)
        close("lrt_pool_act_bwd g_var", gv, g_var, 2e-4 if a == "softplus" else 2e-5, False)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. generated eligible models against CPU float64 autograd
# ---------------------------------------------------------------------------------------------------------------------------
def _m(kind, E, B, Cin, H, W, convs, fcs):
    """convs: (Cout, k, stride, padding, dilation, pool or None); fcs: hidden widths before the 10-way output."""
    return dict(kind=kind, E=E, B=B, Cin=Cin, H=H, W=W, convs=convs, fcs=fcs)


MODELS = {
    "bbb_rect_s2_c3_pool32": _m("bbb", 2, 8, 3, 16, 13, [(8, (5, 3), (2, 1), (2, 1), 1, (3, 2)), (12, 3, 1, 2, 2, None)], [20]),
    "bbb_dil_c1_pool23": _m("bbb", 3, 12, 1, 15, 17, [(6, 3, 3, 1, 2, None), (8, (2, 3), 1, (1, 2), (1, 2), (2, 3))], []),
    "bbb_c4_s2_first": _m("bbb", 1, 8, 4, 14, 11, [(8, 3, 2, 0, 1, None), (16, 3, 1, 1, 1, (3, 1))], [12]),
    "bbb_c8_s3_cin6": _m("bbb", 2, 4, 8, 19, 16, [(6, (3, 5), (3, 2), (1, 2), 1, None), (8, 3, 1, 2, 2, (2, 2))], []),
    "bbb_c3_lenetlike": _m("bbb", 3, 16, 3, 20, 18, [(6, 5, 1, 0, 1, (2, 2)), (16, 3, 1, 1, 1, (3, 2))], [24]),
    "lrt_s2_c3_pool32": _m("lrt", 2, 8, 3, 16, 13, [(8, 5, 2, 2, 1, (3, 2)), (12, 3, 1, 2, 2, None)], [20]),
    "lrt_dil_c1_pool31": _m("lrt", 3, 12, 1, 12, 15, [(6, 3, 1, 2, 2, (3, 1)), (8, 3, 1, 1, 1, (2, 3))], []),
    "lrt_c4_s2_first": _m("lrt", 2, 8, 4, 14, 11, [(8, 3, 2, 0, 1, None), (16, 3, 1, 1, 1, (2, 2))], [12]),
    "lrt_c8_cin6_e1": _m("lrt", 1, 4, 8, 13, 16, [(6, 3, 2, 1, 1, None), (8, 3, 1, 2, 2, (2, 2))], []),
    "lrt_c3_e3_deep": _m("lrt", 3, 8, 3, 18, 14, [(8, 3, 1, 1, 1, (2, 2)), (8, 3, 1, 1, 1, None), (12, 3, 1, 0, 1, (2, 3))], [16]),
}


def _build(spec):
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    from bbb_hip import ops
    Conv, Linear = (BBB_Conv2d, BBB_Linear) if spec["kind"] == "bbb" else (BBB_LRT_Conv2d, BBB_LRT_Linear)
    net = ModuleWrapper()
    cin, H, W = spec["Cin"], spec["H"], spec["W"]
    for i, (cout, k, st, pd, dl, pool) in enumerate(spec["convs"]):
        net.add_module(f"conv{i}", Conv(cin, cout, k, stride=st, padding=pd, dilation=dl, bias=True, priors=P.CONFIG_PRIORS))
        net.add_module(f"act{i}", nn.Softplus())
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
            net.add_module(f"fact{j}", nn.Softplus())
        feat = n
    return net


def _model_ref(net, spec, x, y, seed, call0, beta, N):
    """CPU float64 autograd of the same model and loss, fed the device's Philox noise: weight noise (streams base + 0 / + 1) for
    BBB layers, activation noise keyed by the NCHW output index (stream base + 2) for LRT layers; draw j uses call call0 + j."""
    from bbb_hip import ensemble
    from layers.bbb import _BBBLayer
    from layers.lrt import _LRTLayer
    mods = ensemble.flat_children(net)
    leaves = {}
    for n, p in net.named_parameters():
        leaves[n] = p.detach().cpu().double().requires_grad_(True)
    pname = {id(m): n for n, m in net.named_modules()}
    KIND = {"W": 0, "bias": 1, "act": 2}

    def sp(r):
        return torch.log1p(torch.exp(r))

    x64 = x.cpu().double()
    outs = []
    for j in range(spec["E"]):
        h = x64
        for m in mods:
            if isinstance(m, (_BBBLayer, _LRTLayer)):
                pre = pname[id(m)]
                Wm, Wr, bm, br = (leaves[f"{pre}.{t}"] for t in ("W_mu", "W_rho", "bias_mu", "bias_rho"))
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
            elif isinstance(m, nn.MaxPool2d):
                h = F.max_pool2d(h, m.kernel_size, m.stride)
            else:
                h = h.reshape(-1, m.num_features)
        outs.append(F.log_softmax(h, dim=1))
    kl = 0.0
    for m in mods:
        if isinstance(m, (_BBBLayer, _LRTLayer)):
            pre = pname[id(m)]
            for a, b in (("W_mu", "W_rho"), ("bias_mu", "bias_rho")):
                kl = kl + P._kl(m.prior_mu, m.prior_sigma, leaves[f"{pre}.{a}"], sp(leaves[f"{pre}.{b}"]))
    lo = P.logmeanexp(torch.stack(outs, dim=2), 2)
    loss = F.nll_loss(lo, y.cpu()) * N + beta * kl
    loss.backward()
    return {n: t.grad for n, t in leaves.items()}


# max |got - want| / max |want| per parameter tensor (issue targets); the LRT rho gradients pass through the variance
# contraction, whose output gradient is (v - act_mu) / (2 act_var) of the recovered pre-activation (cf. test_gpu_fast_train.py)
MODEL_BOUND = {"W_mu": 2e-4, "bias_mu": 2e-4, "W_rho": 2e-4, "bias_rho": 2e-4}
MODEL_BOUND_LRT_RHO = 1e-3


# BBB models once more under bf16x3 (LRT layers keep their fused fp32 kernel in that mode: LaunchConfig docstring)
MODEL_RUNS = [(n, "fp32") for n in MODELS] + [(n, "bf16x3") for n in MODELS if MODELS[n]["kind"] == "bbb"]


@pytest.mark.parametrize("name,mode", MODEL_RUNS, ids=[f"{n}-{m}" for n, m in MODEL_RUNS])
def test_model_gradients_vs_float64_autograd(name, mode):
    from bbb_hip import ensemble, fast_train, ops, rng
    spec = MODELS[name]
    torch.manual_seed(sum(map(ord, name)))
    net = _build(spec).cuda()
    rng.assign_stream_ids(net)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 1)
    x = torch.rand((spec["B"], spec["Cin"], spec["H"], spec["W"]), generator=gen).cuda()
    y = torch.randint(0, 10, (spec["B"],), generator=gen).cuda()
    assert fast_train.train_path_ok(net, x) == spec["kind"]
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
        got, w = p.grad.detach().cpu().double(), want[n]
        ratio = float((got - w).abs().max()) / (float(w.abs().max()) + 1e-30)
        lrt_rho = spec["kind"] == "lrt" and kind.endswith("rho")
        _note((f"model {spec['kind']} {kind}", mode), ratio)
        bound = MODEL_BOUND_LRT_RHO if lrt_rho else MODEL_BOUND[kind]
        if not ratio <= bound:
            fails.append((n, ratio, bound))
    assert not fails, fails
