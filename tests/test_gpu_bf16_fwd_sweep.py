"""Named sweep of bbb_conv2d_chwn_bf16_fwd (ops.conv2d_chwn_bf16_forward) over every kernel form its launch plan picks -- the
general kernel's seven instantiations (tile shape, k-groups, wave-specialised), small-k, small-k + pool (strip), window-resident
pool, strip8 and few-output -- each held to a float64 reference computed on the SAME bf16 operands.  The reference is unfold +
matmul in float64, then max_pool2d, bias, activation and one rounding; it goes through no kernel of this library (the
channel-interleaved layouts are torch permutes here too).

Which form a case runs is the library's own answer: case_branches() asks ops.bf16_fwd_plan (bbb_conv2d_chwn_bf16_plan, the launch
entry's plan; host only) and restates from csrc/pconv_bf16_plan.h only what that query does not report, one line each with the
header line cited.  Every case also carries the form it was written for (`want`) and fails when the plan moves it elsewhere;
tests/test_bf16_fwd_sweep_cpu.py::test_bf16_fwd_sweep_branch_coverage asserts the union of the tags without a GPU.

Two tiers, the helpers of test_gpu_bf16_train_fuzz.py.  EXACT: small-integer operands (|v| <= 3, bias included; K * 9 + 3 < 2^24),
activation None and relu: an fp32 output must equal the float64 reference cast to fp32 bit for bit, a bf16 output that reference
rounded once (nearest-even), whatever the summation order -- a dropped, duplicated or misplaced term cannot hide.  GAUSS: bf16-
rounded normals, all three activations (1-Lipschitz), |err| <= 2e-5 * sum |w||x| + 2e-6 (the 2e-5 widened by sqrt(K / 4096) past
4096 terms) plus half a bf16 ulp where the output is bf16; pooled launches take the maximum of sum |w||x| over the window.

Slab addressing (every kernel has its own copy of the slab-index arithmetic): on one case of each of the six forms a shared input
slab, shared weights / bias and no bias, work units with and without a per-slice input, and grouped steps (x_div / x_off), each
against the float64 reference of the mapping written at bbb_conv_desc_t (include/bbb_hip.h), exact tier.  Run with -m gpu."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_bf16_train_fuzz import WORST as _T_WORST
from test_gpu_bf16_train_fuzz import _bf, _check_bf16, _check_f32, _data, _gauss_c, _pack_w
from test_gpu_train_fuzz import _out_hw

pytestmark = pytest.mark.gpu

PREFIX = "fwd "                  # names this file hands to _check_*: its rows of the shared worst-case table


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(k for k in _T_WORST if k[0].startswith(PREFIX)):
        print(f"[bf16-fwd-sweep worst, err / bound] {k[0]:<34s} {k[1]:<8s} {_T_WORST.pop(k):.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
def _c(want, B, E, cin, cout, H, W, k, s=1, p=0, d=1, f32=False, tm=False, pool=None, xc8=False, oc8=False):
    pr = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    kh, kw = pr(k)
    return dict(want=want, B=B, E=E, cin=cin, cout=cout, H=H, W=W, kh=kh, kw=kw, s=pr(s), p=pr(p), d=pr(d), f32=f32, tm=tm,
                pool=pool, xc8=xc8, oc8=oc8)


CASES = {}


def _general(stem, want, B, E, cin, cout, H, W, k, ref_bf16=None, **geom):
    """One geometry of the general kernel in both row orders and both output types.  Reference-order rows with bf16 output of a
    pitch <= 128 on >= 16 pixels are the small-k form: such geometries pass `ref_bf16` = the overrides that keep that combination
    on the general kernel (a longer row or a smaller map)."""
    for tm in (False, True):
        for f32 in (True, False):
            g = dict(B=B, E=E, cin=cin, cout=cout, H=H, W=W, k=k, **geom)
            if not tm and not f32 and ref_bf16:
                g.update(ref_bf16)
            CASES[f"{stem}-{'tm' if tm else 'ref'}-{'f32' if f32 else 'bf16'}"] = _c(want, f32=f32, tm=tm, **g)


# the general kernel.  64 x 128 tiles (shape 12): 40 images = one ragged image tile, 130 channels = three tiles, the last ragged
_general("g12_1", "general(12,1)", 40, 1, 8, 130, 3, 5, 3, p=1)                              # K = 72, 15 pixels
_general("g12_2", "general(12,2)", 40, 1, 64, 130, 3, 5, 3, p=1)                             # K = 576: 9 k tiles, 45 workgroups
_general("g12_4", "general(12,4)", 136, 1, 128, 70, 2, 3, 3, p=1)                            # K = 1152: 18 k tiles, 24 workgroups
# 64 x 256 tiles (shape 14): 392 images = two tiles, the second ragged; 136 = one ragged tile
_general("g14_1", "general(14,1)", 392, 1, 8, 130, 3, 5, 3, p=1)
_general("g14_2", "general(14,2)", 136, 1, 64, 130, 2, 3, 3, p=1)                            # 61 M MACs
# 128 x 128 tiles (shape 22): 136 images x 200 channels = 2 x 2 tiles, both last ones ragged; wave-specialised up to 1024 workgroups
_general("g22_ws", "general(22,1,ws)", 136, 1, 8, 200, 3, 5, 3, p=1)
# ... and plain beyond: 12 x 11 pixels x 2 channel tiles x 4 draws = 1056 workgroups (8 images: one ragged image tile).  With
# reference-order rows and bf16 output the row must be longer than 128 to stay off the small-k form: 15 channels, pitch 136 -- at
# 114 M MACs the largest case of the file (8 images x 193+ channels x 513+ pixels x 129+ k is the least this combination admits)
_general("g22_plain", "general(22,1,plain)", 8, 4, 8, 200, 12, 11, 3, p=1, ref_bf16=dict(cin=15))
# geometry edges on the general kernel
_general("g12_2_cin24", "general(12,2)", 40, 2, 24, 130, 2, 3, 5, p=2)                      # cin = 24: 64-k tiles straddle taps
_general("g14_1_dil2", "general(14,1)", 136, 2, 8, 130, 5, 4, 3, p=2, d=2, ref_bf16=dict(H=4, W=3))    # dilation 2
_general("g22_ws_s2_rect", "general(22,1,ws)", 136, 1, 16, 200, 9, 6, 3, s=2, p=1)       # stride 2, H != W; K = 144
CASES.update({
    # tap-major rows skip the taps in the padding: with padding d (k - 1) border pixels contract a short row, beyond it some
    # contract NO tap and must come out as act(bias) -- on the multi-k-group and wave-specialised instantiations
    "g12_2-tm-padfull": _c("general(12,2)", 40, 1, 64, 40, 2, 2, 3, p=2, tm=True),
    "g12_2-tm-padbeyond": _c("general(12,2)", 40, 1, 64, 40, 2, 2, 3, p=3, tm=True, f32=True),
    "g12_4-tm-padfull": _c("general(12,4)", 8, 1, 128, 70, 2, 2, 3, p=2, tm=True, f32=True),
    "g12_4-tm-padbeyond": _c("general(12,4)", 8, 1, 128, 70, 2, 2, 3, p=3, tm=True),
    "g14_2-tm-padfull": _c("general(14,2)", 136, 1, 64, 10, 2, 1, 3, p=(4, 2), d=(2, 1), tm=True, f32=True),
    "g14_2-tm-padbeyond": _c("general(14,2)", 136, 1, 64, 10, 1, 2, 3, p=(3, 4), tm=True),
    "g22_ws-tm-padfull": _c("general(22,1,ws)", 136, 1, 8, 200, 2, 3, 3, p=2, tm=True),
    "g22_ws-tm-padbeyond": _c("general(22,1,ws)", 136, 1, 8, 200, 2, 1, 3, p=3, tm=True, f32=True),
    # a short reference-order row on a 15-pixel map: one pixel short of the small-k form
    "g_15px_not_smallk": _c("general(12,1)", 8, 1, 3, 33, 5, 3, 3, p=1),
    # small-k: weights in registers, a run of pixels per workgroup
    "sk_16px": _c("smallk", 8, 1, 3, 33, 4, 4, 3, p=1),                                        # the form's lower edge; ks 2, nt 2
    "sk_ks2_nt1": _c("smallk", 8, 2, 1, 6, 12, 12, 5),                                          # LeNet conv1: K = 25
    "sk_ks2_nt2_b264": _c("smallk", 264, 1, 3, 70, 5, 4, 3, p=1),                               # ragged 256-image tile, ragged channel tile
    "sk_ks5_nt1_run2": _c("smallk", 8, 1, 3, 24, 33, 33, 5, p=2),                               # 1089 units: runs of 2, 1089 odd
    "sk_ks5_nt2_s2": _c("smallk", 40, 2, 6, 70, 9, 7, 3, s=2, p=1),                             # K = 54, stride 2
    "sk_ks8_nt1": _c("smallk", 16, 2, 8, 32, 7, 6, 4, p=1),                                     # K = 128: the longest row
    "sk_ks8_nt2": _c("smallk", 16, 1, 12, 40, 6, 5, 3, p=1, d=(1, 2)),                          # K = 108 -> pitch 112
    "sk_run16": _c("smallk", 8, 8, 3, 8, 33, 33, 5, p=2),                                       # 8712 units: runs of 16, 1089 % 16 = 1
    # small-k + pool, strip form: >= 70 pooled rows x image tiles, or more than 32 channels
    "pool_nt1_22_c8": _c("smallk-pool", 8, 12, 3, 24, 12, 11, 5, p=2, pool=(2, 2), oc8=True),   # 72 pooled rows; width 11: a column unused
    "pool_nt1_32_wide": _c("smallk-pool", 8, 10, 3, 16, 16, 33, 3, p=1, pool=(3, 2)),           # 70 pooled rows of 16 pixels: several strips
    "pool_nt2_32": _c("smallk-pool", 40, 2, 6, 70, 9, 8, 3, p=1, pool=(3, 2)),                  # 9 x 8 -> 4 x 3: one strip, a column unused
    "pool_nt2_22_c8": _c("smallk-pool", 264, 1, 8, 40, 7, 12, 4, p=1, pool=(2, 2), oc8=True),   # K = 128; 6 x 11 -> 3 x 5: two strips
    # window-resident pool: <= 32 channels, fewer than 70 pooled rows x image tiles, 128-image tiles
    "pw_c6_22": _c("smallk-poolwin", 64, 3, 1, 6, 32, 32, 5, pool=(2, 2)),                      # LeNet conv1 + pool: one strip of 14 pooled pixels
    "pw_c20_s2_32": _c("smallk-poolwin", 16, 2, 3, 20, 21, 19, 3, s=2, p=1, pool=(3, 2)),       # a stride-2 convolution: four strips of one
    "pw_c32_b136_c8": _c("smallk-poolwin", 136, 1, 3, 32, 8, 8, 5, p=2, pool=(3, 2), oc8=True),  # two image tiles, the second ragged
    "pw_c32_22_1strip": _c("smallk-poolwin", 8, 2, 2, 32, 6, 5, 3, p=1, pool=(2, 2)),           # 6 x 5 -> 3 x 2: one strip per row
    # strip8: channel-interleaved input, tap-major rows of 32 channels, 5 x 5 taps
    "s8_b136_c8": _c("strip8", 136, 1, 32, 8, 3, 4, 5, p=2, tm=True, xc8=True, oc8=True),       # ragged image tile, one partial channel tile
    "s8_pad0_cout72": _c("strip8", 8, 2, 32, 72, 6, 8, 5, p=0, tm=True, xc8=True),              # 2 x 4 map, ragged second channel tile
    "s8_pad4": _c("strip8", 8, 2, 32, 40, 2, 3, 5, p=4, tm=True, xc8=True, oc8=True),           # 6 x 7 map: up to four of five taps outside
    # few-output: <= 16 outputs, rows of >= 512, k slices summed in a fixed order
    "fo_k512_c7": _c("fewout", 8, 1, 512, 7, 1, 1, 1, f32=True),                                # the lower edge
    "fo_k520_b40": _c("fewout", 40, 3, 520, 10, 1, 1, 1, f32=True),                             # ragged 32-image group, 520 % 16 != 0
    "fo_k1040_c16": _c("fewout", 136, 2, 1040, 16, 1, 1, 1),
    "fo_k4100_c1": _c("fewout", 40, 2, 4100, 1, 1, 1, 1),
    "fo_k4100_c16_f32": _c("fewout", 8, 1, 4100, 16, 1, 1, 1, f32=True),
})

SLAB_CASES = {                   # form -> the case whose geometry the slab-addressing variants run on
    "general": "g12_2-tm-bf16", "smallk": "sk_ks5_nt2_s2", "smallk-pool": "pool_nt2_32", "smallk-poolwin": "pw_c20_s2_32",
    "strip8": "s8_pad0_cout72", "fewout": "fo_k520_b40",
}
# variant -> (draws of the launch, keyword arguments of the launch, input slabs, weight sets, bias sets | None,
#             input slab / weight set of output slab e): the mapping of include/bbb_hip.h (bbb_conv_desc_t, unit_div .. x_unit_off)
S_, OFF_, NU_, D_, XOFF_ = 2, 3, 3, 2, 1         # units (S, off): off % S = 1, 3 units; x_div = 2 with x_off = 1 over 3 draws
SLAB_VARIANTS = {
    "xshared": dict(E=3, kw={}, Ex=1, Ew=3, bias="per", ex=lambda e: 0, ew=lambda e: e),
    "wshared": dict(E=3, kw={}, Ex=3, Ew=1, bias="shared", ex=lambda e: e, ew=lambda e: 0),
    "nobias": dict(E=3, kw={}, Ex=3, Ew=3, bias=None, ex=lambda e: e, ew=lambda e: e),
    # unit u = off + e: weight / bias set (off % S + e) / S of those passed in; input slab e, or u % S of an [S] per-slice tensor
    "units": dict(E=NU_, kw=dict(units=(S_, OFF_), n_units=NU_), Ex=NU_, Ew=(OFF_ % S_ + NU_ + S_ - 1) // S_, bias="per",
                  ex=lambda e: e, ew=lambda e: (OFF_ % S_ + e) // S_),
    "units-perslice": dict(E=NU_, kw=dict(units=(S_, OFF_), n_units=NU_, x_per_slice=True), Ex=S_,
                           Ew=(OFF_ % S_ + NU_ + S_ - 1) // S_, bias="per", ex=lambda e: (OFF_ + e) % S_,
                           ew=lambda e: (OFF_ % S_ + e) // S_),
    # x_unit_div = D: output slab e reads input slab (e + x_off) / D; weight / bias set e
    "xdiv": dict(E=3, kw=dict(x_div=D_, x_off=XOFF_), Ex=(3 + XOFF_ + D_ - 1) // D_, Ew=3, bias="per",
                 ex=lambda e: (e + XOFF_) // D_, ew=lambda e: e),
}


# ---------------------------------------------------------------------------------------------------------------------------
# which kernel a case runs: pure (ops.bf16_fwd_plan needs the built library, no device)
# ---------------------------------------------------------------------------------------------------------------------------
def _plan(c, draws=None):
    from bbb_hip import ops
    E = c["E"] if draws is None else draws
    return ops.bf16_fwd_plan((E, c["cin"], c["H"], c["W"], c["B"]), c["cout"], (c["cin"], c["kh"], c["kw"]), c["s"], c["p"], c["d"],
                             draws=E, out_f32=c["f32"], tap_major=c["tm"], x_c8=c["xc8"], out_c8=c["oc8"], pool=c["pool"])


def form_name(plan):
    form, shape, kgs, ws = plan
    if form != "general":
        return form
    return f"general({shape},{kgs}" + ((",ws" if ws else ",plain") if shape == 22 else "") + ")"


def _pool_strips(c, ho, wo, nt):
    """Strips per pooled row of the two pooled forms (the query does not report it): ("win" | "strip", n)."""
    pk, ps = c["pool"]
    hp, wp = (ho - pk) // ps + 1, (wo - pk) // ps + 1
    rows = c["E"] * -(-c["cout"] // (32 * nt)) * -(-c["B"] // 256) * hp                  # pconv_bf16_plan.h:225-227, 273
    if nt == 1 and rows < 70:                                                            # pconv_bf16_plan.h:243
        wrw = (pk - 1) * c["s"][0] + (c["kh"] - 1) * c["d"][0] + 1                       # :244
        win = lambda n: c["cin"] * wrw * ((((n - 1) * ps + pk) - 1) * c["s"][1] + (c["kw"] - 1) * c["d"][1] + 1) + 1   # :245-249
        fit = [n for n in range(1, wp + 1) if win(n) <= 13 * 16 and win(n) * 160 * 2 + 4 * 32 * 40 * 2 <= 72 * 1024]   # :251-255
        if fit:
            return "win", -(-wp // max(fit))                                             # :257
    cost = lambda n: -(-rows * -(-wp // -(-wp // n)) // 512) * (-(-wp // n) * ps + pk - ps)       # :278-283
    return "strip", min(range(1, max(wp // 2, 1) + 1), key=lambda n: (cost(n), n))       # :277, 283: the first cheapest split


def case_branches(c):
    """The tags one case of the table reaches.  Form, tile shape, k-groups and wave specialisation are ops.bf16_fwd_plan's."""
    plan = _plan(c)
    form = plan[0]
    name = form_name(plan)
    B, cin, cout, kh, kw = c["B"], c["cin"], c["cout"], c["kh"], c["kw"]
    ho, wo = _out_hw(c["H"], c["W"], kh, kw, c["s"], c["p"], c["d"])
    Kp = (cin * kh * kw + 7) & ~7
    out = {name}
    if form == "general":
        bn, bm = (128 if plan[1] == 22 else 64), (256 if plan[1] == 14 else 128)         # pconv_bf16_plan.h:111
        out.add(f"{name}:{'tm' if c['tm'] else 'ref'}:{'f32' if c['f32'] else 'bf16'}")
        if B % bm and cout % bn and (B > bm or cout > bn):
            out.add(f"{name}:ragged-both+multi-tile")
        full = (c["d"][0] * (kh - 1), c["d"][1] * (kw - 1))
        if c["tm"] and kh * kw > 1 and c["p"] == full:
            out.add(f"{name}:tm-pad=d(k-1)")
        if c["tm"] and c["p"][0] > full[0] and c["p"][1] > full[1]:
            out.add(f"{name}:tm-pad>d(k-1)")
        if c["tm"] and cin == 24 and kh * kw > 1:
            out.add("general:tm-cin24")
        if c["d"] == (2, 2):
            out.add("general:dilation2")
        if c["s"] == (2, 2) and c["H"] != c["W"]:
            out.add("general:stride2-nonsquare")
        if not c["tm"] and not c["f32"] and Kp <= 128 and ho * wo == 15:
            out.add("general:15px-short-row")                                            # pconv_bf16_plan.h:307: one pixel short
    elif form == "smallk":
        nt = 1 if cout <= 32 else 2                                                      # pconv_bf16_plan.h:223
        ks = 2 if Kp <= 32 else (5 if Kp <= 80 else 8)                                   # pconv_bf16_plan.h:224
        units = c["E"] * -(-cout // (32 * nt)) * -(-B // 256) * ho * wo                  # pconv_bf16_plan.h:225-227, 312
        run = min(16, max(1, units // 512))                                              # pconv_bf16_plan.h:313-314
        out |= {f"smallk:ks{ks}:nt{nt}", "smallk:run1" if run == 1 else "smallk:run>1"}
        if run > 1 and (ho * wo) % run:
            out.add("smallk:run-ragged")
        if run == 16:
            out.add("smallk:run16")
        if B > 256 and B % 256:
            out.add("smallk:ragged-images")
        if ho * wo == 16:
            out.add("smallk:16px")
    elif form in ("smallk-pool", "smallk-poolwin"):
        nt = 1 if cout <= 32 else 2                                                      # pconv_bf16_plan.h:223
        kind, n = _pool_strips(c, ho, wo, nt)
        assert kind == ("win" if form == "smallk-poolwin" else "strip"), (kind, form)
        pk, ps = c["pool"]
        out |= {f"{form}:pool{pk}/{ps}", f"{form}:strips1" if n == 1 else f"{form}:strips>1", f"{form}:out_c8" if c["oc8"] else f"{form}:out_chwn"}
        if (wo - pk) % ps:
            out.add(f"{form}:column-unused")
        if form == "smallk-pool":
            out.add(f"smallk-pool:nt{nt}")
        else:
            out.add(f"smallk-poolwin:cout{cout}")
            if c["s"] == (2, 2):
                out.add("smallk-poolwin:stride2")
            if 128 < B < 256 and B % 128:                                                # pconv_bf16_plan.h:262: 128-image tiles
                out.add("smallk-poolwin:two-image-tiles-ragged")
    elif form == "strip8":
        out.add(f"strip8:pad{c['p'][0]}")
        if wo % 3:                                                                       # pconv_bf16_plan.h:295: three pixels per strip
            out.add("strip8:width%3")
        if B % 128:                                                                      # pconv_bf16_plan.h:301
            out.add("strip8:ragged-images")
        if cout % 64:                                                                    # pconv_bf16_plan.h:297
            out.add("strip8:ragged-channels" if cout > 64 else "strip8:partial-channel-tile")
        if c["oc8"]:
            out.add("strip8:out_c8")
    elif form == "fewout":
        K = cin
        kps = ((Kp + 63) // 64 + 7) // 8 * 8                                             # pconv_bf16_plan.h:321: k per slice
        out |= {f"fewout:K{K}", f"fewout:cout{cout}", "fewout:f32" if c["f32"] else "fewout:bf16"}
        if K % kps:
            out.add("fewout:K%slice")
        if B % 32:                                                                       # pconv_bf16_plan.h:324
            out.add("fewout:ragged-images")
    return out


def slab_branches():
    """slab:<form>:<variant> for every variant whose launch (its own number of draws) the plan still gives the form of its case."""
    out = set()
    for form, name in SLAB_CASES.items():
        for v, spec in SLAB_VARIANTS.items():
            got = _plan(CASES[name], draws=spec["E"])[0]
            if got == form:
                out.add(f"slab:{form}:{v}")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 reference and the launch
# ---------------------------------------------------------------------------------------------------------------------------
def _to_c8(x):
    """[E, C, H, W, B] -> [E, C / 8, H, W, B, 8] (BBB_BF16_X_C8), as a torch permute."""
    E, C, H, W, B = x.shape
    return x.reshape(E, C // 8, 8, H, W, B).permute(0, 1, 3, 4, 5, 2).contiguous()


def _from_c8(y):
    E, C8, H, W, B, _ = y.shape
    return y.permute(0, 1, 5, 2, 3, 4).reshape(E, C8 * 8, H, W, B)


def reference64(c, x64, w64, b64, ex, ew, E):
    """float64 pre-activation values and magnitudes sum |w||x| of output slabs 0 .. E-1, [E, Cout, Hp, Wp, B]: slab e contracts
    input slab ex(e) of x64 [Ex, Cin, H, W, B] with weight set ew(e) of w64 [Ew, Cout, Cin, kh, kw] and adds bias set ew(e) of b64
    [Eb, Cout] (None: no bias).  Pooled launches: MaxPool2d over the biased map -- the kernel takes the maximum of the fp32
    contraction results, then bias, then activation, which is the same because adding the bias and the activation are
    non-decreasing; the activation is applied by the caller, after the pool, for the same reason."""
    ho, wo = _out_hw(c["H"], c["W"], c["kh"], c["kw"], c["s"], c["p"], c["d"])
    pre, mag = [], []
    for e in range(E):
        cols = F.unfold(x64[ex(e)].permute(3, 0, 1, 2), (c["kh"], c["kw"]), dilation=c["d"], padding=c["p"], stride=c["s"])   # [B, K, L]
        rows = w64[ew(e)].reshape(c["cout"], -1)
        y = torch.einsum("ok,bkl->bol", rows, cols)
        m = torch.einsum("ok,bkl->bol", rows.abs(), cols.abs())
        if b64 is not None:
            y = y + b64[ew(e) if b64.shape[0] > 1 else 0][None, :, None]
        y, m = y.reshape(c["B"], c["cout"], ho, wo), m.reshape(c["B"], c["cout"], ho, wo)
        if c["pool"]:
            y, m = F.max_pool2d(y, c["pool"][0], c["pool"][1]), F.max_pool2d(m, c["pool"][0], c["pool"][1])
        pre.append(y.permute(1, 2, 3, 0))
        mag.append(m.permute(1, 2, 3, 0))
    return torch.stack(pre), torch.stack(mag)


def activate64(pre, act):
    return pre if act is None else (pre.clamp_min(0) if act == "relu" else F.softplus(pre))


def launch(c, x, rows, bias, act, **kw):
    """The launch under test on bf16 x [Ex, Cin, H, W, B], packed rows and fp32 bias -> [E, Cout, Hp, Wp, B]."""
    from bbb_hip import ops
    y = ops.conv2d_chwn_bf16_forward(_to_c8(x) if c["xc8"] else x, rows, bias, (c["cin"], c["kh"], c["kw"]), c["s"], c["p"], c["d"],
                                     act=act, out_f32=c["f32"], tap_major=c["tm"], pool=c["pool"], out_c8=c["oc8"], **kw)
    assert y.dtype == (torch.float32 if c["f32"] else torch.bfloat16)
    return _from_c8(y) if c["oc8"] else y


def check(c, what, tier, got, pre, mag, act):
    """One output against the float64 reference under the tier's rule (the training sweep's helpers)."""
    want = activate64(pre, act).cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    K = c["cin"] * c["kh"] * c["kw"]
    m = None if tier == "exact" else mag.cpu() + 2e-6 / _gauss_c(K)           # c(K) * m = c(K) * sum |w||x| + 2e-6
    (_check_f32 if c["f32"] else _check_bf16)(PREFIX + what, tier, got, want, m, K)


def _seed(name, tier):
    return sum(map(ord, name)) * 2 + (tier == "exact")


def _dev():
    return "cuda"


@pytest.mark.parametrize("tier", ["exact", "gauss"])
@pytest.mark.parametrize("name", list(CASES))
def test_form_vs_float64(name, tier):
    c = CASES[name]
    assert form_name(_plan(c)) == c["want"], (name, _plan(c))          # the plan moved the case off the kernel it was written for
    E = c["E"]
    gen = torch.Generator().manual_seed(_seed(name, tier))
    x = _data(gen, tier, (E, c["cin"], c["H"], c["W"], c["B"]))
    w = _data(gen, tier, (E, c["cout"], c["cin"], c["kh"], c["kw"]), 0.3)
    b = _data(gen, tier, (E, c["cout"]))
    xd, wd, bd = x.to(_dev()), w.to(_dev()), b.to(_dev())
    pre, mag = reference64(c, xd.double(), wd.double(), bd.double(), lambda e: e, lambda e: e, E)
    xb, rows = _bf(xd), _pack_w(wd, c["tm"])
    for act in ((None, "relu") if tier == "exact" else (None, "relu", "softplus")):
        got = launch(c, xb, rows, bd, act)
        check(c, c["want"] + (" f32" if c["f32"] else " bf16"), tier, got, pre, mag, act)


@pytest.mark.parametrize("variant", list(SLAB_VARIANTS))
@pytest.mark.parametrize("form", list(SLAB_CASES))
def test_slab_addressing_vs_float64(form, variant):
    """Every form admits every variant (fwd_plan refuses only work units combined with x_unit_div, which conv2d_chwn_bf16_forward
    cannot express): none is left out, and a variant the plan moves to another form is a wrong case (slab_branches)."""
    c, v = CASES[SLAB_CASES[form]], SLAB_VARIANTS[variant]
    E = v["E"]
    assert _plan(c, draws=E)[0] == form, (form, variant, _plan(c, draws=E))
    gen = torch.Generator().manual_seed(_seed(form + variant, "exact"))
    x = _data(gen, "exact", (v["Ex"], c["cin"], c["H"], c["W"], c["B"]))
    w = _data(gen, "exact", (v["Ew"], c["cout"], c["cin"], c["kh"], c["kw"]))
    b = None if v["bias"] is None else _data(gen, "exact", (1 if v["bias"] == "shared" else v["Ew"], c["cout"]))
    xd, wd, bd = x.to(_dev()), w.to(_dev()), None if b is None else b.to(_dev())
    pre, _ = reference64(c, xd.double(), wd.double(), None if bd is None else bd.double(), v["ex"], v["ew"], E)
    for act in (None, "relu"):
        got = launch(c, _bf(xd), _pack_w(wd, c["tm"]), bd, act, **v["kw"])
        check(c, f"slab {form}", "exact", got, pre, None, act)
