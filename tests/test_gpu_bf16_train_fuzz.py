"""Seeded sweep of the bf16 training backward (fast_train._MCForwardBF16 on the shared fast_train._walk / _Schedule,
csrc/train_bf16.hip, the role-swapped launches of the bf16 GEMM) over the geometries bf16_train_refusal admits -- what _train_path_static admits with B % 8 == 0 -- against CPU float64
references computed on the SAME bf16 operands:

  * kernel level: conv2d_chwn_input_grad_bf16 (with / without up-front flipped rows), conv2d_chwn_weight_grad_bf16 (batch chunks on
    and off, S = 1 / 2 / >= 4, shared and per-draw x, strided first layers whose role-swapped launch yields kh' > kh rows, Cin not a
    multiple of 8, 1 x 1 output maps, linear layers), every GEMM form of bbb_conv2d_chwn_bf16_fwd those launches reach,
    pool_act_backward_chwn_bf16 (overlapping, gapped, tiled and floor-dropping pools on H != W, three activations, bf16 / fp32
    incoming gradients, out_f32 + pad_planes), plane_sums_bf16, and the shared-input first layer fed the bf16 mode's fp32 g_pre;
  * data movement, bitwise: flip_transpose_w_bf16 (the four row-order combinations and 1 x 1), chwn_to_bhwc_bf16, batch_chunks_bf16;
  * model level: generated eligible BBB models whose every parameter gradient from train.forward_loss(precision="bf16") is compared
    with the float64 restatement of the contract (tests/bf16_train_contract.py) fed the device's own Philox noise, and with the fp32
    path by cosine; value-neutral switches (overlap_wgrad, flips_up_front, a graph replay) must not move a bit.

Two tiers.  EXACT: small-integer operands, which bf16 holds exactly, and partial sums below 2^24: an fp32 result must equal the
float64 reference cast to fp32 bit for bit, a bf16 result the float64 reference rounded once (nearest-even), whatever the summation
order -- a dropped, duplicated or misplaced term cannot hide.  GAUSSIAN: normal operands, the bounds of test_gpu_bf16_train.py:
contractions 2e-5 of sum |a||b| (widened by sqrt(K / 4096) past K = 4096 terms, as test_gpu_train_fuzz.py) plus half a bf16 ulp where
the output is bf16; pooling / activation backward half a bf16 ulp; bias sums 1e-5 of the sum of magnitudes.  Run with -m gpu."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import bbb_numpy as O
import bf16_train_contract as C
import ref_port_torch as P
from test_gpu_train_fuzz import _out_hw

pytestmark = pytest.mark.gpu

C_GAUSS = 2e-5
WORST = {}                       # (what, tier) -> worst observed err / bound (0 = bit-exact), printed at the end of the module


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"[bf16-train-fuzz worst, err / bound] {k[0]:<34s} {k[1]:<8s} {WORST[k]:.3e}")


def _gauss_c(K):
    return C_GAUSS * max(1.0, math.sqrt(K / 4096.0))


def _bf(t):
    return t.to(torch.bfloat16)


def _rne(t64):
    """float64 -> the bf16 value it rounds to once (nearest-even), as float64 (exact-tier values are fp32-exact)."""
    return t64.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _half_ulp(v):
    """Half a bf16 ulp of each value of a float64 tensor (0 where v == 0)."""
    a = v.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    return torch.where(a > 0, torch.pow(2.0, e - 8), torch.zeros_like(a))


def _pack_w(w, tap_major):
    """[E, Cout, Cin, kh, kw] (values bf16-exact) -> bf16 rows [E, Cout, Kp] (zero pad), (r, q, ci) columns when tap_major."""
    E, Cout = w.shape[:2]
    K = w[0, 0].numel()
    out = torch.zeros(E, Cout, (K + 7) & ~7, dtype=torch.bfloat16, device=w.device)
    src = w.permute(0, 1, 3, 4, 2) if tap_major else w
    out[:, :, :K] = _bf(src.reshape(E, Cout, K))
    return out


def _data(gen, tier, shape, scale=1.0):
    """bf16-exact fp32 values: small integers (exact tier) or normals rounded to bf16."""
    if tier == "exact":
        return torch.randint(-3, 4, shape, generator=gen).float()
    return (torch.randn(shape, generator=gen) * scale).to(torch.bfloat16).float()


def _check_f32(name, tier, got, want, mag=None, K=1):
    """fp32 output: exact = bitwise the float64 reference cast to fp32; gauss = |err| <= c(K) * mag."""
    got = got.detach().cpu()
    if tier == "exact":
        w32 = want.float()
        bad = got != w32
        assert not bad.any(), f"{name}: {int(bad.sum())} of {got.numel()} elements differ from the exact result; first at " \
                              f"{tuple(int(i) for i in bad.nonzero()[0])}: got {got[bad][0].item()} want {w32[bad][0].item()}"
        _note((name, tier), 0.0)
        return
    err = (got.double() - want).abs()
    bound = _gauss_c(K) * mag + 1e-30
    _note((name, tier), float((err / bound).max()))
    assert (err <= bound).all(), f"{name}: err / bound {float((err / bound).max()):.3e} > 1"


def _check_bf16(name, tier, got, want, mag=None, K=1):
    """bf16 output: exact = bitwise the float64 reference rounded once; gauss = |err| <= c(K) * mag + half a bf16 ulp (mag None:
    the half ulp alone -- one rounding of a value the kernel forms to a few fp32 ulps, which may sit on the other side of a
    rounding midpoint: 2^-12 of the half ulp covers that)."""
    assert got.dtype == torch.bfloat16
    got = got.detach().cpu().double()
    if tier == "exact":
        w = _rne(want)
        bad = got != w
        assert not bad.any(), f"{name}: {int(bad.sum())} of {got.numel()} elements differ from the exact result; first at " \
                              f"{tuple(int(i) for i in bad.nonzero()[0])}: got {got[bad][0].item()} want {w[bad][0].item()}"
        _note((name, tier), 0.0)
        return
    err = (got - want).abs()
    if mag is None:
        bound = _half_ulp(want) * (1 + 2.0 ** -12) + 1e-30
    else:
        slack = _gauss_c(K) * mag
        bound = slack + _half_ulp(want.abs() + slack) + 1e-30
    _note((name, tier), float((err / bound).max()))
    assert (err <= bound).all(), f"{name}: err / bound {float((err / bound).max()):.3e} > 1"


# ---------------------------------------------------------------------------------------------------------------------------
# the GEMM forms of bbb_conv2d_chwn_bf16_fwd (pconv_bf16.hip) a backward launch reaches -- pure: also run without a GPU
# (test_host_cpu.py::test_bf16_train_fuzz_branch_coverage)
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_form(B, cin, H, W, cout, kh, kw, s, p, d, draws, out_f32, tap_major):
    """The dispatcher's choice for one launch (no pool, no c8 layouts: what the backward launches), restated independently of
    the library's plan (fwd_plan in csrc/pconv_bf16_plan.h; tests/test_bf16_plan_cpu.py holds ops.bf16_fwd_plan against it).
    Returns a set of tags."""
    ho, wo = _out_hw(H, W, kh, kw, s, p, d)
    K = cin * kh * kw
    Kp = (K + 7) & ~7
    # fwd_plan, BBB_BF16_FORM_SMALLK  if (!tap_major && !out_f32 && Kp <= 128 && (int64_t)ho * wo >= 16)  -> pconv_bf16_smallk_kernel
    if not tap_major and not out_f32 and Kp <= 128 and ho * wo >= 16:
        return {"smallk"}
    # fwd_plan, BBB_BF16_FORM_FEWOUT  cout <= 16, K >= 512, a 1 x 1 layer on a one-pixel map without padding
    if cout <= 16 and K >= 512 and kh == 1 and kw == 1 and H == 1 and W == 1 and p == (0, 0):
        return {"fewout-f32" if out_f32 else "fewout-bf16"}

    def waste(n, t):
        return -(-n // t) * t / n
    # tile_shape: the tile shape by LDS cycles per useful unit
    c22 = 256.0 * waste(cout, 128) * waste(B, 128)
    c14 = 288.0 * waste(cout, 64) * waste(B, 256)
    c12 = 320.0 * waste(cout, 64) * waste(B, 128)
    shape = 22 if (c22 <= c14 and c22 <= c12) else (14 if c14 <= c12 else 12)
    # fwd_tile_rule  tiny: >= 16 k tiles of 64 and < 256 (64 x 128) items -> shape 12 with four k-groups
    t64 = -(-K // 64)
    items12 = draws * ho * wo * -(-cout // 64) * -(-B // 128)
    tiny = t64 >= 16 and items12 < 256
    if tiny:
        shape = 12
    bn, bm = (128 if shape == 22 else 64), (256 if shape == 14 else 128)
    items = draws * ho * wo * -(-cout // bn) * -(-B // bm)
    # small_launch_rule  a second k-group for small launches with long k loops; wave specialisation for 128 x 128 tiles
    kgs = 2 if (items < 512 and t64 >= 8) else 1
    if tiny:
        kgs = 4
    ws = shape == 22 and items <= 1024
    if ws:
        kgs = 1
    return {"general", f"shape{shape}", "tiny" if tiny else ("ws" if ws else f"kg{kgs}"),
            "items<512" if items < 512 else "items>=512", "out-f32" if out_f32 else "out-bf16"}


def wgrad_S(c, chunks=True):
    from bbb_hip import ops
    Cp = (c["Cin"] + 7) & ~7
    return ops.wgrad_batch_chunks_bf16(c["E"], c["Cout"], Cp, c["kh"], c["kw"], c["B"]) if chunks else 1


def wgrad_launch_form(c, chunks=True):
    """The role-swapped weight-gradient launch: batch = Cin padded to 8, contraction channels = B / S images, taps = output
    pixels (stride <-> dilation), E * S draws, fp32 out, tap-major rows unless the output map is one pixel."""
    S = wgrad_S(c, chunks)
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    return gemm_form((c["Cin"] + 7) & ~7, c["B"] // S, c["H"], c["W"], c["Cout"], ho, wo, c["d"], c["p"], c["s"], c["E"] * S,
                     True, ho * wo > 1)


def dgrad_launch_form(c):
    """The input-gradient launch: the forward over the flipped rows, padding d * (k - 1) - p, bf16 out."""
    from bbb_hip import ops
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    q = (c["d"][0] * (c["kh"] - 1) - c["p"][0], c["d"][1] * (c["kw"] - 1) - c["p"][1])
    return gemm_form(c["B"], c["Cout"], ho, wo, c["Cin"], c["kh"], c["kw"], (1, 1), q, c["d"], c["E"], False,
                     ops.bf16_tap_major((c["Cin"], c["Cout"], c["kh"], c["kw"])))


# ---------------------------------------------------------------------------------------------------------------------------
# case generators: only what _train_path_static admits, B % 8 == 0
# ---------------------------------------------------------------------------------------------------------------------------
def _conv(B, E, Cin, Cout, H, W, kh, kw, s=(1, 1), p=(0, 0), d=(1, 1), xs=False, flip=False):
    return dict(B=B, E=E, Cin=Cin, Cout=Cout, H=H, W=W, kh=kh, kw=kw, s=tuple(s), p=tuple(p), d=tuple(d), xs=xs, flip=flip)


def _lin(B, E, Fin, Fout, xs=False, flip=False):
    return _conv(B, E, Fin, Fout, 1, 1, 1, 1, xs=xs, flip=flip)


def _conv_cost(c):
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    return c["B"] * c["Cin"] * c["Cout"] * ho * wo * c["kh"] * c["kw"] * c["E"]


def _conv_cases(n, seed):
    """Later layers (stride 1, any dilation, padding 0..d*(k-1)) and strided first layers on Cin % 4 == 0 inputs (x shared)."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        kh, kw = int(rs.choice([1, 2, 3, 5])), int(rs.choice([1, 2, 3, 5, 7]))
        d = (int(rs.randint(1, 4)), int(rs.randint(1, 4)))
        p = (int(rs.randint(0, d[0] * (kh - 1) + 1)), int(rs.randint(0, d[1] * (kw - 1) + 1)))
        H, W = int(rs.randint(1, 15)), int(rs.randint(1, 15))
        first = rs.rand() < 0.3
        s = (int(rs.randint(1, 5)), int(rs.randint(2, 5))) if first else (1, 1)
        Cin = int(rs.choice([4, 8, 12, 20])) if first else int(rs.choice([4, 6, 8, 12, 20, 64, 128]))
        Cout = int(rs.choice([4, 6, 10, 16, 33, 64, 70, 128]))
        B = int(rs.choice([8, 16, 24, 32, 64, 128, 136]))
        E = int(rs.choice([1, 2, 3]))
        ho, wo = _out_hw(H, W, kh, kw, s, p, d)
        if H == W or ho < 1 or wo < 1:
            continue
        c = _conv(B, E, Cin, Cout, H, W, kh, kw, s, p, d, xs=first or bool(rs.rand() < 0.3), flip=bool(rs.rand() < 0.5))
        if _conv_cost(c) > 12e6:                                        # CPU float64 reference work per case
            continue
        out.append(c)
    return out


CONV_CASES = {
    # named edges: each reaches a branch the random draw may miss (test_host_cpu.py::test_bf16_train_fuzz_branch_coverage)
    "q0_rect_dil": _conv(8, 2, 6, 10, 9, 5, 5, 3, p=(8, 4), d=(2, 2), flip=True),           # padding = d*(k-1): q = 0
    "S2_perdraw_cin12": _conv(32, 1, 12, 20, 5, 7, 3, 3, p=(1, 1)),
    "S4_shared": _conv(64, 3, 20, 6, 6, 4, 3, 2, p=(1, 0), xs=True),
    "S8_perdraw_cout70": _conv(128, 1, 8, 70, 4, 3, 3, 3, p=(1, 1)),
    "S1_b136": _conv(136, 2, 16, 12, 5, 3, 2, 3, p=(1, 2), d=(1, 2)),                     # 136 % 16 != 0: no chunks
    "first_s2_khslice_S1": _conv(8, 2, 4, 16, 16, 11, 3, 3, s=(2, 2), xs=True),           # kh' = 4, kw' = 4 > 3
    "first_s4_khslice_S4": _conv(64, 1, 8, 8, 15, 13, 3, 2, s=(4, 3), p=(1, 1), xs=True),
    "first_s3_dil2_S2": _conv(32, 3, 12, 10, 14, 9, 2, 3, s=(3, 2), p=(2, 0), d=(2, 1), xs=True),
    "first_alexnet_cin4": _conv(8, 1, 4, 48, 32, 32, 11, 11, s=(4, 4), p=(5, 5), xs=True),
    "out1x1_conv": _conv(16, 2, 8, 10, 3, 5, 3, 5, flip=True),                             # Ho * Wo = 1
    "out1x1_dil": _conv(24, 1, 20, 6, 5, 3, 3, 2, d=(2, 2), flip=False),
    "cin8_1x1_not_tapmajor": _conv(16, 2, 8, 16, 6, 5, 1, 1, flip=True),                   # kh * kw == 1: rows not tap-major
    "cin16_cout12_in_tm": _conv(16, 1, 16, 12, 5, 6, 3, 3, p=(1, 1), flip=True),          # in tap-major, out not
    "cin12_cout16_out_tm": _conv(16, 2, 12, 16, 6, 5, 3, 3, p=(1, 1)),                     # out tap-major, in not
    "cin16_cout16_both_tm": _conv(8, 2, 16, 16, 7, 5, 3, 2, p=(2, 1), d=(2, 1), flip=True),
    "dgrad_smallk": _conv(24, 2, 8, 12, 7, 5, 3, 3, p=(1, 1)),                              # Kp = 112, not tap-major, 35 pixels
    "wgrad_tiny_1x1": _conv(8, 1, 64, 32, 12, 11, 1, 1),                                   # K = 1056: 17 k tiles, one item
    "wgrad_kg2": _conv(8, 1, 16, 16, 10, 9, 3, 3, p=(1, 1)),                                # K = 720: 12 k tiles, few items
    "ws_128": _conv(8, 1, 128, 128, 3, 4, 3, 3, p=(1, 0)),                                 # 128 x 128 tiles, wave-specialised
    "dgrad_large_launch": _conv(8, 3, 8, 16, 15, 12, 3, 3, p=(1, 1), flip=True),
    # linear layers: x [E|1, F, 1, 1, B]
    "lin_first_shared_S4": _lin(64, 2, 48, 32, xs=True),                                   # expand + reshape of a shared x
    "lin_first_shared_S1": _lin(8, 3, 20, 12, xs=True),
    "lin_logits_f12": _lin(24, 2, 12, 10),
    "lin_fewout_dgrad_16x512": _lin(16, 1, 16, 512, flip=True),                             # dgrad: 16 outputs, K = 512
    "lin_fewout_f32_512": _lin(512, 1, 84, 10),                                            # wgrad, chunks off: K = 512 images
    "lin_fewout_f32_16out": _lin(512, 2, 20, 16, xs=True),
}
CONV_CASES.update({f"rand{i}": c for i, c in enumerate(_conv_cases(24, 20261016))})


def conv_branches(c, chunks=True):
    from bbb_hip import ops
    S = wgrad_S(c, chunks)
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    khp = (c["H"] + 2 * c["p"][0] - c["s"][0] * (ho - 1) - 1) // c["d"][0] + 1
    kwp = (c["W"] + 2 * c["p"][1] - c["s"][1] * (wo - 1) - 1) // c["d"][1] + 1
    out = {("wgrad-S1" if S == 1 else "wgrad-S2+") + ("-shared" if c["xs"] else "-perdraw")}
    if S == 2:
        out.add("wgrad-S2")
    if S >= 4:
        out.add("wgrad-S4+")
    if (khp, kwp) != (c["kh"], c["kw"]):
        out.add("wgrad-khslice" + ("-S2+" if S > 1 else "-S1"))
    if c["Cin"] % 8:
        out.add("wgrad-cinpad")
    if ho * wo == 1:
        out.add("wgrad-1pixel")
    if c["H"] == c["W"] == c["kh"] == c["kw"] == 1:
        out.add("linear-shared" if c["xs"] else "linear")
        if c["xs"] and S > 1 and c["E"] > 1:
            out.add("linear-shared-expand")
    out |= {"wgrad:" + t for t in wgrad_launch_form(c, chunks)}
    if c["s"] == (1, 1):
        out.add("dgrad-flipped" if c["flip"] else "dgrad-plain")
        if c["p"] == (c["d"][0] * (c["kh"] - 1), c["d"][1] * (c["kw"] - 1)):
            out.add("dgrad-q0")
        out |= {"dgrad:" + t for t in dgrad_launch_form(c)}
        tin, tout = ops.bf16_tap_major((c["Cout"], c["Cin"], c["kh"], c["kw"])), ops.bf16_tap_major((c["Cin"], c["Cout"], c["kh"], c["kw"]))
        out.add(f"flip-in{'TM' if tin else 'CM'}-out{'TM' if tout else 'CM'}")
    return out


def _pool(E, C, H, W, B, k, s, act, g_f32=False):
    return dict(E=E, C=C, H=H, W=W, B=B, k=k, s=s, act=act, g_f32=g_f32)


POOL_CASES = {}
for _i, (_k, _s, _H, _W) in enumerate([(3, 2, 10, 8), (2, 3, 11, 8), (1, 2, 7, 10), (3, 1, 7, 5), (2, 2, 7, 9), (3, 3, 10, 8),
                                        (4, 2, 13, 7), (2, 2, 8, 6), (0, 1, 5, 3)]):
    for _act in (None, "relu", "softplus"):
        if _k == 0 and _act is None:
            continue                     # (no pool, no activation: a rounding only -- the logits layer, covered below)
        POOL_CASES[f"k{_k}s{_s}_{_H}x{_W}_{_act}"] = _pool(1 + _i % 3, 3 + _i, _H, _W, 8 * (1 + _i % 3), _k, _s, _act,
                                                            g_f32=bool(_i % 2))
POOL_CASES["logits_round_only"] = _pool(2, 10, 1, 1, 24, 0, 1, None, g_f32=True)


def pool_branches(c):
    k, s, H, W = c["k"], c["s"], c["H"], c["W"]
    out = {"g-f32" if c["g_f32"] else "g-bf16", f"act-{c['act']}"}
    if k == 0:
        out.add("act-only")
        return out
    out.add("overlap" if k > s else ("gap" if k < s else "tiled"))
    if (H - k) % s or (s > k and H % s):
        out.add("floor-rows")
    if (W - k) % s or (s > k and W % s):
        out.add("floor-cols")
    if H != W:
        out.add("h!=w")
    return out


def _shared(B, E, Cin, Cout, H, W, kh, kw, s=(1, 1), p=(0, 0), d=(1, 1), pool=None, act="softplus"):
    return dict(B=B, E=E, Cin=Cin, Cout=Cout, H=H, W=W, kh=kh, kw=kw, s=tuple(s), p=tuple(p), d=tuple(d), pool=pool, act=act)


SHARED_CASES = {
    "cin1_lenet": _shared(16, 2, 1, 6, 32, 32, 5, 5, pool=(2, 2), act="relu"),
    "cin2_s2_dil2": _shared(8, 3, 2, 8, 17, 13, 3, 3, (2, 2), (2, 1), (2, 1)),
    "cin5_s3_rect": _shared(24, 1, 5, 12, 20, 14, 5, 3, (3, 2), (2, 1), pool=(3, 2)),
    "cin6_s1_dil3": _shared(8, 2, 6, 16, 12, 15, 3, 2, (1, 1), (3, 1), (3, 1), act="relu"),
    "cin7_s4_11x11": _shared(8, 1, 7, 16, 36, 32, 11, 11, (4, 4), (5, 5), pool=(1, 2)),
    "cin3_padded_pitch": _shared(16, 2, 3, 8, 10, 8, 3, 1, act="relu"),                 # K = 8 * 8 * 16 = 1024: padded pitch
    "cin1_s2_slices": _shared(32, 1, 1, 8, 29, 31, 3, 3, (2, 2), (1, 1), pool=(2, 3)),
}


def shared_branches(c):
    from bbb_hip import ops
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    K, Jp = ho * wo * c["B"], (c["Cin"] * c["kh"] * c["kw"] + 3) // 4 * 4
    S = ops.shared_input_k_slices(c["E"] * c["Cout"], Jp, K)
    return {"shared-S1" if S == 1 else "shared-S2+", "gpre-padded-view" if ops.padded_plane_pitch(K) != K else "gpre-contiguous",
            f"cin{c['Cin']}", "strided" if c["s"] != (1, 1) else "stride1", "dilated" if c["d"] != (1, 1) else "undilated"}


# ---------------------------------------------------------------------------------------------------------------------------
# 1. input and weight gradients on the bf16 GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def _conv_ref(c, g, x, w):
    """float64 dgrad / wgrad per draw: g [E, Cout, Ho, Wo, B], x [Ex, Cin, H, W, B], w [E, Cout, Cin, kh, kw]."""
    B, E, Cin = c["B"], c["E"], c["Cin"]
    geom = dict(stride=c["s"], padding=c["p"], dilation=c["d"])
    gx = None
    if c["s"] == (1, 1):
        gx = torch.stack([conv2d_input((B, Cin, c["H"], c["W"]), w[e], g[e].permute(3, 0, 1, 2), **geom).permute(1, 2, 3, 0)
                          for e in range(E)])
    gw = torch.stack([conv2d_weight(x[0 if c["xs"] else e].permute(3, 0, 1, 2), (c["Cout"], Cin, c["kh"], c["kw"]),
                                    g[e].permute(3, 0, 1, 2), **geom) for e in range(E)])
    return gx, gw


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_backward_bf16_vs_float64(name, tier):
    from bbb_hip import ops
    c = CONV_CASES[name]
    B, E, Cin, Cout, H, W, kh, kw = (c[k] for k in ("B", "E", "Cin", "Cout", "H", "W", "kh", "kw"))
    ho, wo = _out_hw(H, W, kh, kw, c["s"], c["p"], c["d"])
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    x = _data(gen, tier, (1 if c["xs"] else E, Cin, H, W, B))
    w = _data(gen, tier, (E, Cout, Cin, kh, kw), 0.3)
    g = _data(gen, tier, (E, Cout, ho, wo, B))
    x64, w64, g64 = x.double(), w.double(), g.double()
    want_x, want_w = _conv_ref(c, g64, x64, w64)
    mag_x = mag_w = None
    if tier == "gauss":
        mag_x, mag_w = _conv_ref(c, g64.abs(), x64.abs(), w64.abs())
    gd, xd = _bf(g.cuda()), _bf(x.cuda())
    wshape = (Cout, Cin, kh, kw)
    if c["s"] == (1, 1):
        rows = _pack_w(w.cuda(), ops.bf16_tap_major(wshape))
        wf = ops.flip_transpose_w_bf16(rows, wshape) if c["flip"] else None
        gx = ops.conv2d_chwn_input_grad_bf16(gd, rows, wshape, (H, W), c["p"], c["d"], w_flipped=wf)
        assert gx.shape == (E, Cin, H, W, B)
        _check_bf16("dgrad", tier, gx, want_x, mag_x, Cout * kh * kw)
    for chunks in (True, False):
        ops.wgrad_chunks_bf16[0] = chunks
        try:
            gw = ops.conv2d_chwn_weight_grad_bf16(gd, xd, (E,) + wshape, c["s"], c["p"], c["d"])
        finally:
            ops.wgrad_chunks_bf16[0] = True
        assert gw.shape == (E,) + wshape and gw.dtype == torch.float32
        S = wgrad_S(c, chunks)
        _check_f32(f"wgrad S{'1' if S == 1 else ('2' if S == 2 else '4+')}", tier, gw, want_w, mag_w, B * ho * wo)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. pooling / activation backward, plane sums
# ---------------------------------------------------------------------------------------------------------------------------
def _route_chwn(g, y, k, s):
    """float64 max-pool backward routed by y (first maximum): g [E, C, Hp, Wp, B], y [E, C, H, W, B] -> [E, C, H, W, B]."""
    if k == 0:
        return g
    E, Cc, H, W, B = y.shape
    yy = y.permute(0, 4, 1, 2, 3).reshape(E * B, Cc, H, W)
    gg = g.permute(0, 4, 1, 2, 3).reshape(E * B, Cc, g.shape[2], g.shape[3])
    return C._route(gg, yy, k, s).reshape(E, B, Cc, H, W).permute(0, 2, 3, 4, 1)


def _pool_ref(g64, y64, k, s, act):
    r = _route_chwn(g64, y64, k, s)
    return r * C._act_grad(y64, act) if act is not None else r


def _coarse_y(gen, shape, act):
    """Stored activated outputs on a coarse grid (ties inside windows are common), bf16-exact; Softplus outputs include values
    around its threshold of 20."""
    v = torch.randn(shape, generator=gen)
    if act == "relu":
        v = v.clamp_min(0)
    elif act == "softplus":
        v = F.softplus(v)
        near = torch.rand(shape, generator=gen) < 0.15
        v = torch.where(near, 20.0 + (torch.randint(-3, 4, shape, generator=gen).float() * 0.125), v)
    return _bf((v * 4).round() / 4 if act != "softplus" else v).float()


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_pool_act_backward_bf16_vs_float64(name, tier):
    from bbb_hip import ops
    c = POOL_CASES[name]
    E, Cc, H, W, B, k, s, act = (c[n] for n in ("E", "C", "H", "W", "B", "k", "s", "act"))
    if tier == "exact" and act == "softplus":
        tier = "gauss"                   # softplus' derivative is a transcendental: no exact tier (the gauss run covers it twice)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    hp, wp = ((H - k) // s + 1, (W - k) // s + 1) if k else (H, W)
    y = _coarse_y(gen, (E, Cc, H, W, B), act)
    g = _data(gen, tier, (E, Cc, hp, wp, B))
    if c["g_f32"] and tier == "gauss":
        g = torch.randn((E, Cc, hp, wp, B), generator=gen)              # the logits' fp32 gradient: not bf16-exact
    want = _pool_ref(g.double(), y.double(), k, s, act)
    gd = g.cuda() if c["g_f32"] else _bf(g.cuda())
    yd = _bf(y.cuda()) if (k or act) else None
    got = ops.pool_act_backward_chwn_bf16(gd, yd, k, s, act)
    assert got.shape == (E, Cc, H, W, B)
    what = f"pool_act_bwd[{act}]" + ("-gf32" if c["g_f32"] else "")
    _check_bf16(what, tier, got, want)
    # the fp32 form holds exactly the values of the bf16 one, at the padded plane pitch when asked
    K = H * W * B
    for pad in (False, True):
        f = ops.pool_act_backward_chwn_bf16(gd, yd, k, s, act, out_f32=True, pad_planes=pad)
        assert f.dtype == torch.float32 and torch.equal(f, got.float())
        assert f.stride(1) == (ops.padded_plane_pitch(K) if pad else K)
    _note(("pool_act_bwd out_f32 / pitch", "bitwise"), 0.0)
    # bias partials of that g_pre: fp32 sums of the bf16 values
    sums = ops.plane_sums_bf16(got)
    g64 = got.double().cpu()
    _check_f32("plane_sums_bf16", tier, sums, g64.sum(dim=(2, 3, 4)), g64.abs().sum(dim=(2, 3, 4)) * (1e-5 / C_GAUSS))


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("shape", [(2, 3, 1, 1, 8), (1, 2, 33, 17, 24), (1, 2, 64, 64, 136), (3, 5, 7, 9, 8), (1, 1, 1, 257, 2048)],
                         ids=lambda s: "x".join(map(str, s)))
def test_plane_sums_bf16_long_and_ragged_rows(shape, tier):
    from bbb_hip import ops
    gen = torch.Generator().manual_seed(sum(shape) * 2 + (tier == "exact"))
    g = _data(gen, tier, shape)
    got = ops.plane_sums_bf16(_bf(g.cuda()))
    g64 = g.double()
    _check_f32("plane_sums_bf16", tier, got, g64.sum(dim=(2, 3, 4)), g64.abs().sum(dim=(2, 3, 4)) * (1e-5 / C_GAUSS))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. data movement, bitwise
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,cin,kh,kw", [(16, 8, 3, 3), (12, 8, 3, 2), (16, 6, 5, 3), (10, 6, 3, 3), (8, 16, 1, 1), (10, 84, 1, 1),
                                            (24, 40, 2, 5), (5, 7, 1, 3)])
def test_flip_transpose_bf16_all_row_orders(cout, cin, kh, kw):
    from bbb_hip import ops
    gen = torch.Generator().manual_seed(cout * 100 + cin * 10 + kh * kw)
    w = torch.randn((3, cout, cin, kh, kw), generator=gen).cuda()
    rows = _pack_w(w, ops.bf16_tap_major((cout, cin, kh, kw)))
    got = ops.flip_transpose_w_bf16(rows, (cout, cin, kh, kw))
    want = _pack_w(w.flip(3, 4).transpose(1, 2).contiguous(), ops.bf16_tap_major((cin, cout, kh, kw)))
    assert got.shape == want.shape and torch.equal(got, want)
    _note(("flip_transpose_w_bf16", "bitwise"), 0.0)


@pytest.mark.parametrize("E,C_,H,W,B,cp", [(2, 70, 3, 2, 72, 72), (1, 4, 5, 3, 136, 8), (3, 12, 2, 5, 200, 24), (1, 130, 1, 1, 64, 136),
                                           (2, 20, 4, 4, 8, 64), (1, 64, 2, 3, 128, 64)])
def test_chwn_to_bhwc_bf16_ragged_tiles(E, C_, H, W, B, cp):
    from bbb_hip import ops
    gen = torch.Generator().manual_seed(C_ * 1000 + B)
    x = _bf(torch.randn((E, C_, H, W, B), generator=gen).cuda())
    got = ops.chwn_to_bhwc_bf16(x, cp)
    want = torch.zeros((E, B, H, W, cp), dtype=torch.bfloat16, device="cuda")
    want[..., :C_] = x.permute(0, 4, 2, 3, 1)
    assert torch.equal(got, want)                       # pad channels C .. Cp - 1 are zero
    if cp == (C_ + 7) & ~7:
        assert torch.equal(ops.chwn_to_bhwc_bf16(x), want)
    _note(("chwn_to_bhwc_bf16", "bitwise"), 0.0)


@pytest.mark.parametrize("shape", [(2, 3, 4, 5, 64), (1, 70, 1, 1, 512), (3, 6, 3, 2, 128), (1, 1, 2, 2, 16)], ids=lambda s: "x".join(map(str, s)))
def test_batch_chunks_bf16(shape):
    from bbb_hip import ops
    gen = torch.Generator().manual_seed(sum(shape))
    g = _bf(torch.randn(shape, generator=gen).cuda())
    B = shape[-1]
    for S in (1, 2, 4, 8, 16, 32, 64):
        if B % (8 * S):
            continue
        ch = ops.batch_chunks_bf16(g, S)
        want = g.reshape(*shape[:-1], S, B // S).permute(0, 4, 1, 2, 3, 5).contiguous()
        assert torch.equal(ch, want), S
    _note(("batch_chunks_bf16", "bitwise"), 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the first layer in bf16 mode: the fp32 shared-input weight gradient over the bf16 mode's fp32, padded-pitch g_pre
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "bf16x3"])
@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(SHARED_CASES))
def test_shared_input_first_layer_bf16_mode(name, tier, mode):
    from bbb_hip import ops
    c = SHARED_CASES[name]
    B, E, Cin, Cout, H, W, kh, kw = (c[k] for k in ("B", "E", "Cin", "Cout", "H", "W", "kh", "kw"))
    act = c["act"]
    ho, wo = _out_hw(H, W, kh, kw, c["s"], c["p"], c["d"])
    k, s = c["pool"] if c["pool"] else (0, 1)
    hp, wp = ((ho - k) // s + 1, (wo - k) // s + 1) if k else (ho, wo)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (tier == "exact"))
    x = _data(gen, tier, (B, Cin, H, W))                                # the bf16-rounded input, as fp32 (ctx.x_nchw)
    y = _coarse_y(gen, (E, Cout, ho, wo, B), "relu" if (tier == "exact" and act == "softplus") else act)
    act_used = "relu" if (tier == "exact" and act == "softplus") else act
    g = _data(gen, tier, (E, Cout, hp, wp, B))
    g_pre = ops.pool_act_backward_chwn_bf16(_bf(g.cuda()), _bf(y.cuda()), k, s, act_used, out_f32=True, pad_planes=True)
    K = ho * wo * B
    assert g_pre.stride(1) == ops.padded_plane_pitch(K)
    _check_bf16("first-layer g_pre", tier, _bf(g_pre), _pool_ref(g.double(), y.double(), k, s, act_used))
    gp64 = g_pre.double().cpu()                                         # the same bf16 operands the kernel contracts

    def ref(gg, xx):
        return torch.stack([conv2d_weight(xx, (Cout, Cin, kh, kw), gg[e].permute(3, 0, 1, 2), stride=c["s"], padding=c["p"],
                                          dilation=c["d"]) for e in range(E)])
    want = ref(gp64, x.double())
    mag = ref(gp64.abs(), x.double().abs()) if tier == "gauss" else None
    cfg = dict(gemm_mode="bf16x3", bf16x3_min_workgroups=0) if mode == "bf16x3" else {}
    with ops.use_config(**cfg):
        gw = ops.conv2d_chwn_weight_grad_shared_input(g_pre, x.cuda(), (E, Cout, Cin, kh, kw), c["s"], c["p"], c["d"])
    _check_f32(f"first-layer wgrad[{mode}]", tier, gw, want, mag, K)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. generated eligible BBB models against the contract and the fp32 path
# ---------------------------------------------------------------------------------------------------------------------------
def _L(kind, out, k=1, s=1, p=0, d=1, act=None, pool=None):
    return dict(kind=kind, out=out, k=k, s=s, p=p, d=d, act=act, pool=pool)


def _m(E, B, Cin, H, W, layers, chunks=True):
    """layers: convs, then linear layers (the last = the 10-way logits, no activation); a FlattenLayer sits before the first
    linear layer (at the very front when the model starts with one)."""
    return dict(E=E, B=B, Cin=Cin, H=H, W=W, layers=layers, chunks=chunks)


MODELS = {
    "c4_s2_relu_gap": _m(2, 8, 4, 17, 14, [_L("conv", 8, 3, 2, 1, act="relu", pool=(2, 3)),
                                             _L("conv", 16, (3, 2), 1, (2, 1), (1, 2), act="softplus"), _L("fc", 10)]),
    "c8_s3_overlap_e3": _m(3, 24, 8, 19, 16, [_L("conv", 16, (3, 5), (3, 2), (1, 2), act="softplus", pool=(3, 1)),
                                                _L("conv", 12, 3, 1, 4, 2, act="softplus"), _L("fc", 24, act="relu"), _L("fc", 10)]),
    "c1_dil_b136_e1": _m(1, 136, 1, 15, 17, [_L("conv", 6, 5, 2, 2, 2, act="softplus"),
                                              _L("conv", 8, (2, 3), 1, (1, 2), (1, 2), act="softplus"), _L("fc", 10)]),
    "c2_relu_pool22": _m(2, 24, 2, 14, 12, [_L("conv", 8, 3, 1, 1, act="relu", pool=(2, 2)),
                                             _L("conv", 8, 3, 1, 2, 2, act="relu", pool=(3, 2)), _L("fc", 10)]),
    "c5_softplus_nopool": _m(3, 8, 5, 13, 10, [_L("conv", 12, (3, 5), (2, 1), (1, 2), act="softplus"),
                                                _L("conv", 16, (5, 1), 1, (4, 0), (2, 1), act="softplus"), _L("fc", 16, act="softplus"),
                                                _L("fc", 10)]),
    "c7_relu_tiled33": _m(1, 24, 7, 16, 13, [_L("conv", 10, 3, (2, 1), 1, act="relu", pool=(3, 3)),
                                              _L("conv", 12, (1, 2), 1, (0, 1), act="softplus"), _L("fc", 10)]),
    "flatten_linear_first": _m(2, 24, 3, 4, 4, [_L("fc", 16, act="softplus"), _L("fc", 512, act="softplus"), _L("fc", 10)]),
    "linear_first_relu_b136": _m(3, 136, 2, 4, 6, [_L("fc", 32, act="relu"), _L("fc", 10)]),
    "c4_b512_fewout_logits": _m(1, 512, 4, 6, 5, [_L("conv", 8, 3, 1, 1, act="softplus"), _L("fc", 10)], chunks=False),
}


def model_plan(spec):
    """The model as a general layer plan (bf16_train_contract.general_plan), layer names = the module names of _build."""
    plan = []
    cin, H, W = spec["Cin"], spec["H"], spec["W"]
    for i, L in enumerate(spec["layers"]):
        ent = dict(name=f"l{i}", kind=L["kind"], stride=L["s"], padding=L["p"], dilation=L["d"], act=L["act"], pool=L["pool"],
                   flat=None)
        if L["kind"] == "conv":
            kh, kw = C._pair(L["k"])
            H, W = _out_hw(H, W, kh, kw, C._pair(L["s"]), C._pair(L["p"]), C._pair(L["d"]))
            if L["pool"]:
                H, W = (H - L["pool"][0]) // L["pool"][1] + 1, (W - L["pool"][0]) // L["pool"][1] + 1
            assert H >= 1 and W >= 1, spec
            cin = L["out"]
            if spec["layers"][i + 1]["kind"] == "fc":
                ent["flat"] = cin * H * W
        plan.append(ent)
    return plan


def _build(spec, model_seed):
    from layers import BBB_Conv2d, BBB_Linear, FlattenLayer, ModuleWrapper
    torch.manual_seed(model_seed)
    net = ModuleWrapper()
    cin, H, W = spec["Cin"], spec["H"], spec["W"]
    feat = cin * H * W
    for i, L in enumerate(spec["layers"]):
        if L["kind"] == "conv":
            net.add_module(f"l{i}", BBB_Conv2d(cin, L["out"], L["k"], stride=L["s"], padding=L["p"], dilation=L["d"], bias=True,
                                               priors=P.CONFIG_PRIORS))
        else:
            if i == 0:
                net.add_module("flatten", FlattenLayer(feat))
            net.add_module(f"l{i}", BBB_Linear(feat, L["out"], bias=True, priors=P.CONFIG_PRIORS))
        if L["act"]:
            net.add_module(f"a{i}", nn.ReLU() if L["act"] == "relu" else nn.Softplus())
        if L["kind"] == "conv":
            kh, kw = C._pair(L["k"])
            H, W = _out_hw(H, W, kh, kw, C._pair(L["s"]), C._pair(L["p"]), C._pair(L["d"]))
        if L["pool"]:
            net.add_module(f"p{i}", nn.MaxPool2d(*L["pool"]))
            H, W = (H - L["pool"][0]) // L["pool"][1] + 1, (W - L["pool"][0]) // L["pool"][1] + 1
        cin = L["out"]
        if L["kind"] == "conv" and spec["layers"][i + 1]["kind"] == "fc":
            net.add_module("flatten", FlattenLayer(cin * H * W))
        feat = cin * H * W if L["kind"] == "conv" else L["out"]
    return net


def _model_setup(name):
    from bbb_hip import fast_train, rng
    spec = MODELS[name]
    net = _build(spec, sum(map(ord, name))).cuda()
    rng.assign_stream_ids(net)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 1)
    x = torch.rand((spec["B"], spec["Cin"], spec["H"], spec["W"]), generator=gen).cuda()
    y = torch.randint(0, 10, (spec["B"],), generator=gen).cuda()
    assert fast_train.bf16_train_refusal(net, x) is None
    return spec, net, x, y


def _grads(net, x, y, E, seed_call, precision, beta=0.1, n=5000.0):
    from bbb_hip import train
    net.zero_grad(set_to_none=True)
    loss, _, _ = train.forward_loss(net, x, y, E, beta, n, seed_call=seed_call, precision=precision)
    loss.backward()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def _bf16_grads(spec, net, x, y, seed_call):
    from bbb_hip import ops
    ops.wgrad_chunks_bf16[0] = spec["chunks"]
    try:
        return _grads(net, x, y, spec["E"], seed_call, "bf16")
    finally:
        ops.wgrad_chunks_bf16[0] = True


def model_branches(spec):
    """What a generated model reaches (pure, for the CPU coverage test)."""
    from bbb_hip import ops
    L0 = spec["layers"][0]
    out = set()
    if L0["kind"] == "fc":
        out.add("first-linear")
    elif spec["Cin"] % 4:
        out.add(f"first-shared-cin{spec['Cin']}")
    else:
        out.add(f"first-bf16-wgrad-cin{spec['Cin']}")
        if C._pair(L0["s"]) != (1, 1):
            out.add("first-bf16-wgrad-strided")
    for L in spec["layers"][1:]:
        if L["kind"] == "conv" and (C._pair(L["d"]) != (1, 1)):
            out.add("later-dilated")
        if L["kind"] == "conv" and C._pair(L["k"])[0] != C._pair(L["k"])[1]:
            out.add("later-nonsquare")
    for L in spec["layers"]:
        if L["pool"]:
            k, s = L["pool"]
            out.add("pool-" + ("overlap" if k > s else ("gap" if k < s else "tiled")))
        if L["act"]:
            out.add("act-" + L["act"])
    out |= {f"E{spec['E']}", f"B{spec['B']}"}
    # the logits layer's weight gradient: >= 512 images in one launch reaches the fewout kernel's fp32 output
    plan = model_plan(spec)
    feat = plan[-2]["flat"] if plan[-2]["flat"] else spec["layers"][-2]["out"]
    lc = _lin(spec["B"], spec["E"], feat, spec["layers"][-1]["out"])
    if "fewout-f32" in wgrad_launch_form(lc, spec["chunks"]):
        out.add("logits-fewout-f32")
    if not spec["chunks"]:
        out.add("chunks-off")
    return out


def _no_ties(spec):
    return all(L["pool"] is None and L["act"] != "relu" for L in spec["layers"])


@pytest.mark.parametrize("name", list(MODELS))
def test_model_gradients_bf16_vs_contract_and_fp32(name):
    spec, net, x, y = _model_setup(name)
    E, seed, call0, beta, n = spec["E"], 4242, 17, 0.1, 5000.0
    got = _bf16_grads(spec, net, x, y, (seed, call0))
    g32 = _grads(net, x, y, E, (seed, call0), "fp32")
    plan = model_plan(spec)
    mods = dict(net.named_modules())
    npar = {L["name"]: {k: getattr(mods[L["name"]], k).detach().cpu().numpy() for k in ("W_mu", "W_rho", "bias_mu", "bias_rho")}
            for L in plan}
    npar["_prior_mu"], npar["_prior_sigma"] = mods["l0"].prior_mu, mods["l0"].prior_sigma
    eps = [{L["name"]: {kind: O.normal_eps(seed, call0 + e, mods[L["name"]]._stream_base + off,
                                           int(np.prod(npar[L["name"]][key].shape))).reshape(npar[L["name"]][key].shape)
                        for kind, key, off in (("W", "W_mu", 0), ("bias", "bias_mu", 1))} for L in plan} for e in range(E)]
    _, _, want = C.step_grads(plan, npar, x.cpu().numpy(), y.cpu().numpy(), eps, None, beta, n)
    bound = 1e-2 if _no_ties(spec) else 4e-2
    fails = []
    for L in plan:
        for key in ("W_mu", "W_rho", "bias_mu", "bias_rho"):
            pn = f"{L['name']}.{key}"
            g = got[pn].double().cpu().numpy()
            w = np.asarray(want[L["name"]][key]).reshape(g.shape)
            rel = float(np.abs(g - w).max()) / float(np.abs(w).max())
            _note((f"model {'no-ties' if _no_ties(spec) else 'pool/relu'} {key}", "contract"), rel / bound)
            a, b = got[pn].double().flatten(), g32[pn].double().flatten()
            cos = float(a @ b / (a.norm() * b.norm()))
            _note(("model 1 - cosine vs fp32", "fp32"), (1.0 - cos) / 0.005)
            if not rel <= bound:
                fails.append((pn, "contract", rel, bound))
            if not cos >= 0.995:
                fails.append((pn, "cosine", cos, 0.995))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------------
# 6. value-neutral switches: bitwise the same gradients
# ---------------------------------------------------------------------------------------------------------------------------
SWITCH_MODELS = ["c8_s3_overlap_e3", "flatten_linear_first"]


@pytest.mark.parametrize("name", SWITCH_MODELS)
def test_bf16_switches_are_value_neutral(name):
    from bbb_hip import fast_train
    spec, net, x, y = _model_setup(name)
    ref = _bf16_grads(spec, net, x, y, (7, 3))
    saved = (fast_train.overlap_wgrad[0], fast_train.flips_up_front[0])
    try:
        for ov, fl in ((False, True), (False, False), (True, False)):
            fast_train.overlap_wgrad[0], fast_train.flips_up_front[0] = ov, fl
            got = _bf16_grads(spec, net, x, y, (7, 3))
            for k in ref:
                assert torch.equal(got[k], ref[k]), (k, ov, fl)
    finally:
        fast_train.overlap_wgrad[0], fast_train.flips_up_front[0] = saved
    _note(("switches overlap / flips", "bitwise"), 0.0)


@pytest.mark.parametrize("name", SWITCH_MODELS)
def test_bf16_graph_replay_equals_eager(name):
    from bbb_hip import rng, train
    spec = MODELS[name]
    E, lr, beta, n = spec["E"], 1e-3, 0.1, 1000.0

    def fresh():
        s, net, x, y = _model_setup(name)
        rng.manual_seed(77, call=0)
        return net, x, y

    net_e, x, y = fresh()
    opt_e = train.FusedAdam(net_e.parameters(), lr=lr, capturable=True)
    eager = [train.train_step(net_e, opt_e, x, y, E, beta, n, precision="bf16", graph=False)[0] for _ in range(5)]
    net_g, _, _ = fresh()
    opt_g = train.FusedAdam(net_g.parameters(), lr=lr, capturable=True)
    g = train.GraphedTrainStep(net_g, opt_g, x, y, E, beta, n, warmup=3, precision="bf16")
    graphed = [g.step()[0].clone() for _ in range(2)]
    for a, b in zip(eager[3:], graphed):
        assert torch.equal(a, b)
    for (na, a), (_, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(a, b), na
    _note(("graph replay vs eager", "bitwise"), 0.0)
