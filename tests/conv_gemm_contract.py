"""What tests/test_conv_gemm_sweep_cpu.py and tests/test_gpu_conv_gemm_sweep.py share about the reference-layout implicit GEMM
(csrc/conv_gemm.hip, conv_gemm_kernel<BM, LRT, LINEAR>; bbb_conv2d_fwd = "BBB", bbb_lrt_conv2d_fwd = "LRT"):

  * plan_rules: the launch rules of csrc/conv_gemm_plan.h written out once more, independently, in Python (every refusal of the
    descriptor and of the two entries' operands, the tile rule, the grid);
  * CASES: the table of launches the GPU module runs, each naming the instantiation it was written for, and case_branches(): the
    tags (instantiation, tile edge, k-tile count, loader remainder, geometry, slab addressing, epilogue) a case reaches;
  * reference(): one launch in float64 from oracle/bbb_numpy.py pieces (im2col without any rounding back to fp32, the Philox noise
    keyed by the NCHW element index inside the draw's slab, draw e using call CALL0 + call_dev + e);
  * launch(): the two entries through ctypes, y / act_mu / act_var each between two guard bands that must come back untouched;
  * two checkers: check_exact (dyadic operands: every partial sum of either contraction is an fp32 number in any order, so y,
    act_mu and act_var - float32(1e-16) must EQUAL the reference) and check_rounded (Gaussian operands, per-element bounds);
  * emulate_f32(): the same launch in numpy fp32 with one planted fault, to show on the CPU that the checkers bite.

Tolerances of the rounded tier (every element is checked; tests/pconv_contract.py's):
  act_mu   |got - ref| <= 2e-5 mag + 2e-6, mag = conv(|x|, |W_mu|) + |b_mu|
  act_var  |got - ref| <= 3e-5 ref; == float32(1e-16) + b_var where the input slab is all zero
  pre-activation  tol_mu + |eps| sqrt(ref_var) (3e-5 / 2 + 2^-22): sqrt halves the variance's relative error, and the square root
           and the product add half an ulp each (2^-24 + 2^-24 of the term, rounded up to 2^-22 for the final sum's own rounding)
  output   relu and softplus are 1-Lipschitz: the pre-activation's bound + 2e-5 |ref| for the activation's own rounding.
  BBB launches use the first line (+ the activation's term).  Cases with operand scales (1e-12, 1e6) drop the absolute 2e-6.
Every rounded case keeps K = cin kh kw <= 320, so (K + 2) 2^-24 < 2e-5: the first bound also holds a priori for a chain of K fused
multiply-adds and the bias, in any order; check_rounded returns the worst error / ((K + 2) 2^-24 mag) as "chain"."""
import ctypes
import math
from dataclasses import dataclass, replace

import numpy as np

import bbb_numpy as O

F32, F64 = np.float32, np.float64
EINVAL, EALIGN, ESHAPE = -1, -2, -3
INT_MAX = 2 ** 31 - 1
FORMS = tuple("%s-%d%s" % (k, bm, l) for bm in (64, 128) for k in ("bbb", "lrt") for l in ("", "-lin"))
UNIT_FIELDS = ("unit_div", "unit_off", "x_unit_mod", "x_unit_div", "x_unit_off", "b_offset")
ZERO_FIELDS = UNIT_FIELDS + ("w_row_pitch", "pool", "w_tap_major")
K_MAX = 320


# ------------------------------------------------------------------------------------------------ launch rules
def out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw):
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def plan_rules(desc, lrt, ptrs=None):
    """desc: dict B, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, draws [, act, w_draw_stride, b_draw_stride, any of ZERO_FIELDS]
    -> dict(bm, linear, bk, k_tiles, grid) or the refusal code.  ptrs (the launch entries only): dict of operand addresses, 0 = NULL --
    x, w, y [, bias] for BBB; x, w_mu, w_var, y [, b_mu, b_var, act_mu, act_var, eps] for LRT."""
    g = lambda k: desc.get(k, 0)
    if min(desc[k] for k in ("B", "Cin", "H", "W", "Cout", "kh", "kw", "sh", "sw", "dh", "dw", "draws")) <= 0 or min(desc["ph"], desc["pw"]) < 0:
        return EINVAL
    if not 0 <= g("act") <= 2:
        return EINVAL
    if any(g(k) != 0 for k in ZERO_FIELDS):
        return EINVAL
    out = []
    for n, k, s, p, d in ((desc["H"], desc["kh"], desc["sh"], desc["ph"], desc["dh"]), (desc["W"], desc["kw"], desc["sw"], desc["pw"], desc["dw"])):
        num = n + 2 * p - d * (k - 1) - 1
        if num < 0 or num // s + 1 > INT_MAX:
            return ESHAPE
        out.append(num // s + 1)
    M, K = desc["B"] * out[0] * out[1], desc["Cin"] * desc["kh"] * desc["kw"]
    if M > INT_MAX or K > INT_MAX or desc["Cin"] * desc["H"] * desc["W"] > INT_MAX:
        return ESHAPE
    if desc["H"] + desc["ph"] + desc["dh"] * desc["kh"] >= 0x7000 or desc["W"] + desc["pw"] + desc["dw"] * desc["kw"] >= 0x7000:
        return ESHAPE
    if ptrs is not None and any(ptrs.get(k, 0) == 0 for k in (("x", "w_mu", "w_var", "y") if lrt else ("x", "w", "y"))):
        return EINVAL
    if lrt:
        if ptrs is not None and (ptrs.get("b_mu", 0) == 0) != (ptrs.get("b_var", 0) == 0):
            return EINVAL
        if g("w_draw_stride") != 0 or g("b_draw_stride") != 0:
            return EINVAL
    if ptrs is not None and any(v & 3 for v in ptrs.values()):
        return EALIGN
    linear = all(desc[k] == 1 for k in ("H", "W", "kh", "kw")) and desc["ph"] == 0 and desc["pw"] == 0
    bk = 16 if lrt else 32
    n_tiles = -(-desc["Cout"] // 64)
    bm = 128 if -(-M // 128) * n_tiles * desc["draws"] >= 768 else 64
    return dict(bm=bm, linear=linear, bk=bk, k_tiles=-(-K // bk), grid=(-(-M // bm), n_tiles, desc["draws"]))


def conv_desc(lib, desc):
    d = lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = (desc[k] for k in ("B", "Cin", "H", "W", "Cout", "kh", "kw"))
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = (desc[k] for k in ("sh", "sw", "ph", "pw", "dh", "dw"))
    d.draws = desc["draws"]
    for k in ("act", "x_draw_stride", "w_draw_stride", "b_draw_stride") + ZERO_FIELDS:
        setattr(d, k, desc.get(k, 0))
    return d


def plan_query(lib, desc, lrt):
    """bbb_conv2d_fwd_plan on the same descriptor, in plan_rules' terms."""
    bm, lin, bk, kt, grid = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), (ctypes.c_int32 * 3)()
    rc = lib.lib().bbb_conv2d_fwd_plan(ctypes.byref(conv_desc(lib, desc)), int(lrt), ctypes.byref(bm), ctypes.byref(lin), ctypes.byref(bk),
                                       ctypes.byref(kt), grid)
    if rc != 0:
        assert (bm.value, lin.value, bk.value, kt.value, tuple(grid)) == (0, 0, 0, 0, (0, 0, 0)), "a refusal wrote a plan"
        return rc
    return dict(bm=bm.value, linear=bool(lin.value), bk=bk.value, k_tiles=kt.value, grid=tuple(grid))


def entry_refusal(lib, desc, lrt, ptrs):
    """The launch entry itself on (desc, ptrs): only for arguments plan_rules refuses -- the code comes back before any launch."""
    assert plan_rules(desc, lrt, ptrs) != 0
    p = lambda k: ptrs.get(k, 0) or None
    d = conv_desc(lib, desc)
    if lrt:
        return lib.lib().bbb_lrt_conv2d_fwd(ctypes.byref(d), p("x"), p("w_mu"), p("w_var"), p("b_mu"), p("b_var"), p("y"), p("act_mu"),
                                            p("act_var"), p("eps"), 1, 0, 0, 1, None, None)
    return lib.lib().bbb_conv2d_fwd(ctypes.byref(d), p("x"), p("w"), p("bias"), p("y"), None)


GOOD = dict(B=8, Cin=3, H=9, W=13, Cout=12, kh=2, kw=3, sh=2, sw=1, ph=1, pw=0, dh=1, dw=2, draws=2)        # 5 x 9 pixels, K = 18


def refusals():
    """(name, change of GOOD, change of the operands {name: "null" | "odd"}, LRT only) of every refusal of the two entries."""
    out = [("zero " + k, {k: 0}, {}, False) for k in ("B", "Cin", "H", "W", "Cout", "kh", "kw", "sh", "sw", "dh", "dw", "draws")]
    out += [("negative " + k, {k: -1}, {}, False) for k in ("ph", "pw", "B", "draws")]
    out += [("act 3", dict(act=3), {}, False), ("act -1", dict(act=-1), {}, False)]
    out += [(k, {k: v}, {}, False) for k, v in (("unit_div", 2), ("unit_off", 1), ("x_unit_mod", 2), ("x_unit_div", 2), ("x_unit_off", 1),
                                                ("b_offset", 8), ("w_row_pitch", 64), ("pool", 1), ("w_tap_major", 1))]
    out += [("kernel past the padded rows", dict(kh=12), {}, False), ("kernel past the padded columns", dict(kw=8), {}, False),
            ("rows at 0x7000", dict(H=0x7000 - 1 - 2, Cin=1), {}, False), ("columns at 0x7000", dict(W=0x7000 - 6, Cin=1), {}, False),
            ("dilated taps at 0x7000", dict(H=0x6000, dh=0x800, Cin=1), {}, False),
            ("M past int32", dict(B=2 ** 24, H=40, W=40, Cin=1), {}, False), ("K past int32", dict(Cin=2 ** 29), {}, False),
            ("cin h w past int32", dict(Cin=2 ** 18, H=128, W=128, kh=1, kw=1), {}, False),
            ("output rows past int32", dict(ph=2 ** 30, sh=1), {}, False),
            ("LRT weight draw stride", dict(w_draw_stride=72), {}, True), ("LRT bias draw stride", dict(b_draw_stride=12), {}, True)]
    out += [("NULL " + k, {}, {k: "null"}, False) for k in ("x", "w", "y")] + [("NULL " + k, {}, {k: "null"}, True) for k in ("w_mu", "w_var")]
    out += [("b_mu without b_var", {}, dict(b_var="null"), True), ("b_var without b_mu", {}, dict(b_mu="null"), True)]
    out += [("odd " + k, {}, {k: "odd"}, False) for k in ("x", "w", "bias", "y")]
    out += [("odd " + k, {}, {k: "odd"}, True) for k in ("w_mu", "w_var", "b_mu", "b_var", "act_mu", "act_var", "eps")]
    return out


def with_operands(base, change):
    """base: operand addresses by name; change: {name: "null" | "odd"} -> the addresses an entry is called with."""
    return {k: (0 if change.get(k) == "null" else v + 2 if change.get(k) == "odd" else v) for k, v in base.items()}


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    form: str                         # the instantiation this case was written for (bbb_conv2d_fwd_plan confirms it)
    B: int
    Cin: int
    H: int
    W: int
    Cout: int
    k: tuple = (1, 1)
    s: tuple = (1, 1)
    p: tuple = (0, 0)
    d: tuple = (1, 1)
    E: int = 1                        # draws of the launch
    x_shared: bool = False            # one input slab for every draw (x_draw_stride 0)
    w_shared: bool = False            # BBB: one weight set for every draw (an LRT launch always shares its pair of moments)
    bias: str = "draw"                # "draw" | "shared" | None (LRT: one pair b_mu / b_var, or both NULL)
    act: str = None
    sample: bool = True               # LRT ...
    ext_eps: bool = False
    moments: bool = True
    call_dev: int = None              # value of the device-side call counter during the launch (None: a NULL pointer)
    zero_slab: int = None             # this input slab is all zero
    scale: tuple = None               # (x scale, w scale) of the scale tier: the bounds lose their absolute term
    seed: int = 0
    tags: tuple = ()

    @property
    def lrt(self):
        return self.form.startswith("lrt")

    @property
    def desc(self):
        K = self.Cin * self.k[0] * self.k[1]
        per_draw_w = not self.lrt and not self.w_shared
        return dict(B=self.B, Cin=self.Cin, H=self.H, W=self.W, Cout=self.Cout, kh=self.k[0], kw=self.k[1], sh=self.s[0], sw=self.s[1],
                    ph=self.p[0], pw=self.p[1], dh=self.d[0], dw=self.d[1], draws=self.E, act={None: 0, "relu": 1, "softplus": 2}[self.act],
                    x_draw_stride=0 if self.x_shared else self.B * self.Cin * self.H * self.W,
                    w_draw_stride=self.Cout * K if per_draw_w else 0,
                    b_draw_stride=self.Cout if (not self.lrt and self.bias == "draw") else 0)

    @property
    def out_hw(self):
        return out_hw(self.H, self.W, *self.k, *self.s, *self.p, *self.d)

    @property
    def K(self):
        return self.Cin * self.k[0] * self.k[1]

    @property
    def M(self):
        return self.B * self.out_hw[0] * self.out_hw[1]

    @property
    def x_slabs(self):
        return 1 if self.x_shared else self.E

    @property
    def w_sets(self):
        return 1 if (self.lrt or self.w_shared) else self.E

    @property
    def b_sets(self):
        return 1 if (self.lrt or self.bias == "shared") else self.E


SEED, CALL0, STREAM = 0x1234567887654321, 41, 6          # of the LRT noise
K_EDGES = {32: (1, 2, 3, 31, 32, 33, 64, 65, 98, 128), 16: (1, 2, 3, 15, 16, 17, 32, 33, 50, 64)}     # 1, 2, 3, BK - 1 .. 4 BK
COUT_EDGES = (1, 31, 32, 33, 63, 64, 65)


def case_branches(c, plan):
    """Tags one case reaches; plan = plan_query(...) of the case."""
    kind, bm, lin = ("lrt" if c.lrt else "bbb"), plan["bm"], plan["linear"]
    ho, wo = c.out_hw
    form = "%s-%d%s" % (kind, bm, "-lin" if lin else "")
    t = {form}
    kb = "%s:%d:" % (kind, bm)
    t.add(kb + "kt:%d" % min(plan["k_tiles"], 5))
    if c.M % bm:
        t.add(kb + "ragged-pixel-tile")
    if c.Cout % 64:
        t.add(kb + "ragged-channel-tile")
    if plan["grid"][0] > 1 and plan["grid"][1] > 1:
        t.add(kb + "blocks>1")
    blocks128 = -(-c.M // 128) * -(-c.Cout // 64) * c.E
    if blocks128 in (767, 768):
        t.add("%s:tile:%d" % (kind, blocks128))
    if bm == 64:
        for v, name in ((1, "1"), (63, "BM-1"), (64, "BM"), (65, "BM+1")):
            if c.M == v:
                t.add("%s:M:%s" % (kind, name))
        if not lin and ho * wo == 9 and c.M > 64:
            t.add(kind + ":straddle:HoWo=9")
        if c.Cout in COUT_EDGES:
            t.add("%s:cout:%d" % (kind, c.Cout))
        if c.K in K_EDGES[plan["bk"]]:
            t.add("%s:K:%d" % (kind, c.K))
        t.add("%s:%s:K%%4:%d" % (kind, "lin" if lin else "conv", c.K % 4))
        for name, hit in (("rect", c.k[0] != c.k[1] and c.s[0] != c.s[1] and c.p[0] != c.p[1] and c.d[0] != c.d[1]),
                          ("pad>reach", c.p[0] > c.d[0] * (c.k[0] - 1) and c.p[1] > c.d[1] * (c.k[1] - 1)),
                          ("k=image", (ho, wo) == (1, 1) and c.H > 1 and c.W > 1 and c.p != (0, 0)),
                          ("W=1", c.W == 1 and c.H > 1), ("x:shared", c.x_shared and c.E > 1), ("x:draw", not c.x_shared and c.E > 1),
                          ("b:none", c.bias is None), ("E:1", c.E == 1), ("E:3", c.E == 3), ("act:" + str(c.act), True),
                          ("scale:%g" % c.scale[0] if c.scale else "", c.scale is not None)):
            if hit:
                t.add(kind + ":" + name)
        if not c.lrt:
            for name, hit in (("w:shared", c.w_shared and c.E > 1), ("w:draw", not c.w_shared and c.E > 1), ("b:draw", c.bias == "draw" and c.E > 1),
                              ("b:shared", c.bias == "shared" and c.E > 1)):
                if hit:
                    t.add("bbb:" + name)
        else:
            philox = c.sample and not c.ext_eps
            for name, hit in (("philox:n%%4:%d" % (c.B * c.Cout * ho * wo % 4), philox), ("ext-eps", c.sample and c.ext_eps),
                              ("nosample", not c.sample), ("moments", c.moments), ("no-moments", not c.moments),
                              ("call_dev", philox and bool(c.call_dev)), ("zero-slab", c.zero_slab is not None)):
                if hit:
                    t.add("lrt:" + name)
    return t | set(c.tags)


def wanted_tags():
    """Every instantiation; for the 64-pixel tile every edge on a BBB and on an LRT case; for the 128-pixel tile the k-tile counts and
    the ragged tiles; the tile rule's threshold from both sides."""
    want = set(FORMS)
    for kind, bk in (("bbb", 32), ("lrt", 16)):
        want |= {"%s:%d:kt:%d" % (kind, bm, n) for bm in (64, 128) for n in (1, 2, 3, 4)}
        want |= {"%s:%d:%s" % (kind, bm, n) for bm in (64, 128) for n in ("ragged-pixel-tile", "ragged-channel-tile", "blocks>1")}
        want |= {"%s:tile:767" % kind, "%s:tile:768" % kind}
        want |= {"%s:M:%s" % (kind, n) for n in ("1", "BM-1", "BM", "BM+1")}
        want |= {"%s:cout:%d" % (kind, n) for n in COUT_EDGES} | {"%s:K:%d" % (kind, n) for n in K_EDGES[bk]}
        want |= {"%s:%s:K%%4:%d" % (kind, l, r) for l in ("lin", "conv") for r in range(4)}
        want |= {kind + ":" + n for n in ("straddle:HoWo=9", "rect", "pad>reach", "k=image", "W=1", "x:shared", "x:draw", "b:none", "E:1", "E:3",
                                         "act:None", "act:relu", "act:softplus")}
    want |= {"bbb:w:shared", "bbb:w:draw", "bbb:b:draw", "bbb:b:shared", "bbb:scale:1e-12", "lrt:scale:1e+06"}
    want |= {"lrt:philox:n%4:1", "lrt:philox:n%4:2", "lrt:philox:n%4:3", "lrt:ext-eps", "lrt:nosample", "lrt:moments", "lrt:no-moments",
             "lrt:call_dev", "lrt:zero-slab"}
    return want


def _taps_for(K):
    """K = Cin * kh * kw with the first tap shape that divides it."""
    for kh, kw in ((2, 2), (1, 3), (3, 1), (1, 2), (5, 1)):
        if K % (kh * kw) == 0:
            return K // (kh * kw), (kh, kw)
    return K, (1, 1)


def _cases():
    C = Case
    cs = []
    acts = (None, "relu", "softplus")
    for kind, bk in (("bbb", 32), ("lrt", 16)):
        f, fl = kind + "-64", kind + "-64-lin"
        lrt = kind == "lrt"
        # ---- M around the pixel tile: linear rows for BBB, a kernel as large as the padded image (Ho = Wo = 1) for LRT --------------
        for i, M in enumerate((1, 63, 64, 65)):
            if lrt:
                cs.append(C("%s-M%d" % (kind, M), f, M, 2, 3, 3, 5, (5, 5), p=(1, 1), act=acts[i % 3], call_dev=(7 if i == 1 else None)))
            else:
                cs.append(C("%s-M%d" % (kind, M), fl, M, 6, 1, 1, 5, E=3, x_shared=(i % 2 == 0), act=acts[i % 3]))
        cs.append(C(kind + "-k=image", f, 3, 2, 3, 3, 5, (5, 5), p=(1, 1), E=3, bias=None) if not lrt else
                  C(kind + "-M65-lin", fl, 65, 7, 1, 1, 3, E=3, act="relu", moments=False))
        # ---- a pixel tile across image boundaries: 9 output pixels per image, 15 images in 3 tiles ----------------------------------
        cs.append(C(kind + "-straddle", f, 15, 2, 5, 5, 5, (3, 3), E=3, act="relu", w_shared=True, bias="shared", zero_slab=(1 if lrt else None)))
        # ---- output channels around the 32-row MFMA tile and the 64-row block ------------------------------------------------------
        for i, cout in enumerate(COUT_EDGES):
            cs.append(C("%s-cout%d" % (kind, cout), f, 2, 2, 4, 4, cout, (2, 2), E=(3 if i % 2 else 1), x_shared=(i % 4 == 1), act=acts[i % 3],
                        bias=("draw", "shared", None)[i % 3], sample=(i != 3), ext_eps=(i == 4), moments=(i % 2 == 0),
                        call_dev=(2 ** 32 - 2 if i == 5 else None)))
        # ---- K through 1, 2, 3 and the k-tile edges, on the gather loaders and on the row loaders ----------------------------------
        for i, K in enumerate(K_EDGES[bk]):
            cin, taps = _taps_for(K)
            cs.append(C("%s-K%d" % (kind, K), f, 2, cin, taps[0] + 1, taps[1] + 1, 5, taps, p=(1, 1), act=acts[i % 3], ext_eps=(i % 3 == 1)))
            cs.append(C("%s-K%d-lin" % (kind, K), fl, 9, K, 1, 1, 5, act=acts[(i + 1) % 3], sample=(i % 4 != 2)))
        # ---- more tap shapes for the (ci, r, q) decode: 1 x 3 with padded columns, 1 x 1 on an unpadded map (not LINEAR), 5 x 1 -------
        cs.append(C(kind + "-K6", f, 2, 2, 2, 4, 5, (1, 3), p=(0, 1)))
        cs.append(C(kind + "-K7", f, 2, 7, 2, 3, 5, E=3, x_shared=True))                                      # 1 x 1 taps on a 2 x 3 map
        cs.append(C(kind + "-K35", f, 2, 7, 6, 2, 5, (5, 1), p=(2, 0), act="relu"))
        # ---- geometry --------------------------------------------------------------------------------------------------------------
        cs.append(C(kind + "-rect", f, 3, 3, 9, 7, 33, (3, 2), (2, 1), (1, 2), (1, 2), E=3, act="softplus", moments=False))
        cs.append(C(kind + "-pad>reach", f, 2, 3, 4, 3, 5, (2, 2), p=(3, 3), E=3, act="relu", bias="shared"))   # pixels no tap reaches
        cs.append(C(kind + "-W1", f, 3, 4, 6, 1, 5, (3, 1), (2, 1), (1, 0), E=3, x_shared=True))
        cs.append(C(kind + "-blocks", f, 5, 3, 6, 6, 70, (3, 3), (1, 1), (1, 1), E=3, act="relu"))              # 3 x 2 x 3 workgroups
        # ---- the 128-pixel tile at its threshold: 16 draws x 3 channel tiles x 16 pixel tiles = 768 workgroups; k tiles 1, 2, 3, 4 ----
        # (per-draw operands in one case of each kind; the others share x -- and, BBB, the weights -- so that their float64 reference
        # is three contractions, not 48)
        w = dict(E=16, x_shared=True, sample=False)
        for cin in ((3, 5) if not lrt else (1, 3, 5, 7)):                                                    # K = 9 cin
            own = dict(w, x_shared=False) if cin == 3 else dict(w, w_shared=not lrt)
            cs.append(C("%s-128-c%d" % (kind, cin), kind + "-128", 7, cin, 17, 17, 130, (3, 3), p=(1, 1), act=("relu" if cin == 3 else None), **own))
        w = dict(w, w_shared=not lrt)
        cs.append(C(kind + "-128-lin70", kind + "-128-lin", 2023, 70, 1, 1, 130, **dict(w, sample=True, ext_eps=True)))
        if not lrt:
            cs.append(C(kind + "-128-lin100", kind + "-128-lin", 2023, 100, 1, 1, 130, act="relu", **w))
        else:
            cs.append(C(kind + "-128-lin20", kind + "-128-lin", 2023, 20, 1, 1, 130, E=16, x_shared=True, moments=False))   # Philox on 4.2 M elements
        # ... and its neighbour: 13 draws x 1 x 59 = 767 workgroups of 128 pixels -> the 64-pixel tile
        cs.append(C(kind + "-767", f, 30, 3, 10, 25, 33, (3, 3), p=(1, 1), E=13, x_shared=True, sample=False, bias="shared"))
    # ---- LRT epilogue: Philox quads at output sizes 1, 2, 3 modulo 4 -------------------------------------------------------------------
    cs.append(C("lrt-n%4=1", "lrt-64", 1, 2, 5, 5, 1, (3, 3), E=3, call_dev=5))
    cs.append(C("lrt-n%4=2", "lrt-64", 1, 2, 5, 5, 2, (3, 3), E=3, act="relu", bias=None))
    cs.append(C("lrt-n%4=3", "lrt-64", 1, 2, 5, 5, 3, (3, 3), E=3, act="softplus", x_shared=True, moments=False))
    # ---- scale tier ------------------------------------------------------------------------------------------------------------------
    cs.append(C("bbb-scale-1e-12", "bbb-64", 3, 5, 6, 6, 33, (3, 3), p=(1, 1), E=3, scale=(1e-12, 1e-12)))
    cs.append(C("lrt-scale-1e6", "lrt-64-lin", 20, 50, 1, 1, 33, E=3, scale=(1e6, 1e6)))
    return {c.name: c for c in cs}


CASES = _cases()


def quiet(c):
    """The same launch without noise and without the transcendental: what the exact tier runs."""
    return replace(c, sample=False, moments=True, act=None if c.act == "softplus" else c.act)


# ------------------------------------------------------------------------------------------------ operands
def exact_bits(c):
    """The exactness precondition of the exact tier: x in {-2..2}, W_mu multiples of 1/8 in [-1, 1], sigma^2 multiples of 1/64 in
    [1/64, 1/4], b_mu multiples of 1/8 in [-2, 2], b_var multiples of 1/64 in [1/64, 1/4].  Every partial sum of the mean contraction
    is a multiple of 2^-3 of magnitude <= 2 K + 2, of the variance contraction a multiple of 2^-6 <= K + 1/4: (integer bits +
    fractional bits) of the two; both must be <= 24 for every partial sum to be an fp32 number in ANY order."""
    return math.ceil(math.log2(2 * c.K + 2 + 1)) + 3, math.ceil(math.log2(c.K + 1)) + 6


def _rng(c, kind, i):
    return np.random.default_rng([c.seed, {"x": 1, "w": 2, "s": 3, "b": 4, "v": 5, "e": 6}[kind], i, c.B, c.Cin, c.Cout, c.H])


def operands(c, tier):
    """x [slabs, B, Cin, H, W], w [sets, Cout, Cin, kh, kw] (LRT: [Cout, Cin, kh, kw]), w_var | None, b [sets, Cout] | None (LRT: [Cout]),
    b_var | None, eps [E, B, Cout, Ho, Wo] | None -- float32."""
    ex = tier == "exact"
    xs, ws = (1.0, 1.0) if (ex or c.scale is None) else c.scale
    shp = (c.B, c.Cin, c.H, c.W)
    x = np.stack([(_rng(c, "x", i).integers(-2, 3, shp) if ex else _rng(c, "x", i).standard_normal(shp) * xs).astype(F32) for i in range(c.x_slabs)])
    if c.zero_slab is not None:
        x[c.zero_slab] = 0
    wshape = (c.Cout, c.Cin) + c.k
    w = np.stack([(_rng(c, "w", i).integers(-8, 9, wshape) / 8 if ex else _rng(c, "w", i).standard_normal(wshape) * 0.3 * ws).astype(F32)
                  for i in range(c.w_sets)])
    b = bv = wv = eps = None
    if c.bias:
        b = np.stack([(_rng(c, "b", i).integers(-16, 17, c.Cout) / 8 if ex else _rng(c, "b", i).standard_normal(c.Cout) * xs * ws).astype(F32)
                      for i in range(c.b_sets)])
    if c.lrt:
        wv = (_rng(c, "s", 0).integers(1, 17, wshape) / 64 if ex else (_rng(c, "s", 0).uniform(0.01, 0.3, wshape) * ws) ** 2).astype(F32)
        w, b = w[0], (None if b is None else b[0])
        if c.bias:
            bv = (_rng(c, "v", 0).integers(1, 17, c.Cout) / 64 if ex else (_rng(c, "v", 0).uniform(0.01, 0.3, c.Cout) * xs * ws) ** 2).astype(F32)
        if c.ext_eps and c.sample:
            ho, wo = c.out_hw
            eps = np.stack([_rng(c, "e", e).standard_normal((c.B, c.Cout, ho, wo)).astype(F32) for e in range(c.E)])
    return dict(x=x, w=w, w_var=wv, b=b, b_var=bv, eps=eps)


# ------------------------------------------------------------------------------------------------ the launch in numpy
def _act(v, act):
    if act == "relu":
        return np.maximum(v, v.dtype.type(0))
    if act == "softplus":
        return np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, 20))))
    return v


def noise(c, e, shift_lane=False):
    """[B, Cout, Ho, Wo] of draw e: element ((b Cout + n) Ho Wo + pixel) of the stream (SEED, CALL0 + call_dev + e, STREAM)."""
    ho, wo = c.out_hw
    n = c.B * c.Cout * ho * wo
    z = O.normal_eps(SEED, (CALL0 + (c.call_dev or 0) + e) & 0xFFFFFFFF, STREAM, 4 * -(-n // 4))
    if shift_lane:
        z = z.reshape(-1, 2)[:, ::-1].reshape(-1)                       # element idx ^ 1: the neighbouring lane of its quad
    return z[:n].reshape(c.B, c.Cout, ho, wo)


FAULTS = ("drop-last-k-tile", "rq-swapped", "dhdw-swapped", "tile-table-t-2", "image-base", "weight-slab-e-1", "bias-wrong-draw",
          "noise-neighbour-lane", "var-x-not-squared")


def gather(c, xs, bm, bk, fault=None):
    """The kernel's own im2col of one input slab xs [B, Cin, H, W] -> [M, K]: pixel m = (b, oh, ow) of the launch's pixel tiles, k decoded
    to (ci, r, q) per k tile; with one of the addressing FAULTS planted."""
    ho, wo = c.out_hw
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = c.k, c.s, c.p, c.d
    m = np.arange(c.M)
    b, pix = m // (ho * wo), m % (ho * wo)
    if fault == "image-base":
        b = (m // bm * bm) // (ho * wo)                                 # the tile's first pixel's image for every pixel of the tile
    oh, ow = pix // wo, pix % wo
    k = np.arange(c.K)
    if fault == "tile-table-t-2":
        k = np.where(k >= 2 * bk, k - 2 * bk, k)                        # tile t decoded with the table of tile t - 2
    ci, rq = k // (kh * kw), k % (kh * kw)
    r, q = (rq % kh, rq // kh) if fault == "rq-swapped" else (rq // kw, rq % kw)
    if fault == "dhdw-swapped":
        dh, dw = dw, dh
    ih = (oh * sh - ph)[:, None] + (r * dh)[None, :]
    iw = (ow * sw - pw)[:, None] + (q * dw)[None, :]
    ok = (ih >= 0) & (ih < c.H) & (iw >= 0) & (iw < c.W)
    cols = xs[b[:, None], ci[None, :], np.clip(ih, 0, c.H - 1), np.clip(iw, 0, c.W - 1)] * ok
    if fault == "drop-last-k-tile":
        cols[:, (-(-c.K // bk) - 1) * bk:] = 0
    return cols


def forward(c, ops_, dtype=F64, fault=None, plan=None):
    """One launch of case c on the operands ops_ in `dtype` arithmetic: float64 = the reference (oracle im2col); float32 = the
    emulation (the kernel's gather; plan = its bm and bk), with one of FAULTS planted.  Returns act_mu, var0 (= act_var without the
    1e-16), act_var (LRT), pre, y, eps, mag = conv(|x|, |w|) + |b|, zero = draws whose input is all zero; all [E, B, Cout, Ho, Wo]."""
    ho, wo = c.out_hw
    K = c.K
    cache, res = {}, {}

    def cols(ix, what):
        if (ix, what) not in cache:
            xs = ops_["x"][ix].astype(dtype)
            xs = {"x": xs, "abs": np.abs(xs), "sq": xs if fault == "var-x-not-squared" else xs * xs}[what]
            if dtype == F64 and fault is None:
                cache[ix, what] = O.im2col(xs, *c.k, c.s, c.p, c.d)[0]
            else:
                cache[ix, what] = gather(c, xs, plan["bm"], plan["bk"], fault)
        return cache[ix, what]

    def contract(mat, wmat):
        return (mat @ wmat.reshape(c.Cout, K).astype(dtype).T).reshape(c.B, ho, wo, c.Cout).transpose(0, 3, 1, 2)

    outs = {k: [] for k in ("act_mu", "var0", "act_var", "pre", "y", "eps", "mag")}
    col = lambda v: v.astype(dtype)[None, :, None, None]
    for e in range(c.E):
        ix = 0 if c.x_shared else e
        iw = 0 if (c.lrt or c.w_shared) else (max(e - 1, 0) if fault == "weight-slab-e-1" else e)
        ib = 0 if (c.lrt or c.bias == "shared") else ((e + 1) % c.E if fault == "bias-wrong-draw" else e)
        w = ops_["w"] if c.lrt else ops_["w"][iw]
        b = None if ops_["b"] is None else (ops_["b"] if c.lrt else ops_["b"][ib])
        if (ix, iw) not in res:                                         # draws that share both operands share the contractions
            res[ix, iw] = (contract(cols(ix, "x"), w), contract(cols(ix, "abs"), np.abs(w)),
                           contract(cols(ix, "sq"), ops_["w_var"]) if c.lrt else None)
        mu, mag, var0 = res[ix, iw]
        if b is not None:
            mu, mag = mu + col(b), mag + col(np.abs(b))
        var = z = None
        pre = mu
        if c.lrt:
            if ops_["b_var"] is not None:
                var0 = var0 + col(ops_["b_var"])
            var = dtype(F32(1e-16)) + var0
            if c.sample:
                z = (ops_["eps"][e] if ops_["eps"] is not None else noise(c, e, fault == "noise-neighbour-lane")).astype(dtype)
                with np.errstate(invalid="ignore"):                         # (a planted fault may make the variance negative)
                    pre = mu + np.sqrt(var) * z
        for k, v in (("act_mu", mu), ("var0", var0), ("act_var", var), ("pre", pre), ("y", _act(pre, c.act)), ("eps", z), ("mag", mag)):
            outs[k].append(v)
    r = {k: (np.stack(v) if v[0] is not None else None) for k, v in outs.items()}
    r["b_var"] = ops_["b_var"]
    r["zero"] = np.array([not ops_["x"][0 if c.x_shared else e].any() for e in range(c.E)])
    return r


def reference(c, ops_):
    return forward(c, ops_, F64)


def emulate_f32(c, ops_, fault=None):
    """What a launch with this fault would store: y, and the moments when the case asks for them."""
    plan = plan_rules(c.desc, c.lrt)
    r = forward(c, ops_, F32, fault, plan)
    want = c.lrt and c.moments
    return dict(y=r["y"].astype(F32), act_mu=r["act_mu"].astype(F32) if want else None, act_var=r["act_var"].astype(F32) if want else None)


# ------------------------------------------------------------------------------------------------ the launch on the device
GUARD = 256                                               # floats before and behind every output
SENTINEL = 0x7FC5A5A5                                     # a quiet NaN no kernel computes


class Guarded:
    """A float32 device buffer of n elements between two guard bands of a sentinel pattern; the body starts as the sentinel too, so an
    element a launch never stored shows up as a NaN in every comparison."""

    def __init__(self, torch, n, device="cuda"):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=device)

    @property
    def ptr(self):
        return self.raw.data_ptr() + 4 * GUARD

    def body(self, torch):
        return self.raw[GUARD:GUARD + self.n].view(torch.float32)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == SENTINEL).all().item() and (self.raw[GUARD + self.n:] == SENTINEL).all().item())

    def unwritten(self):
        return bool((self.raw == SENTINEL).all().item())


def launch(lib, torch, c, ops_):
    """Case c on the operands ops_ through bbb_conv2d_fwd / bbb_lrt_conv2d_fwd directly -> dict(y, act_mu, act_var) of numpy arrays
    [E, B, Cout, Ho, Wo]; the guard bands of every output are asserted untouched."""
    sample, moments = c.sample, c.moments
    d = conv_desc(lib, c.desc)
    ho, wo = c.out_hw
    shape = (c.E, c.B, c.Cout, ho, wo)
    n = int(np.prod(shape))
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    x, w, b = dev(ops_["x"]), dev(ops_["w"]), dev(ops_["b"])
    y = Guarded(torch, n)
    am = av = None
    stream = torch.cuda.current_stream().cuda_stream
    if not c.lrt:
        rc = lib.lib().bbb_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), ptr(b), y.ptr, stream)
    else:
        wv, bv = dev(ops_["w_var"]), dev(ops_["b_var"])
        eps = dev(ops_["eps"]) if sample else None
        if moments:
            am, av = Guarded(torch, n), Guarded(torch, n)
        counter = None
        if c.call_dev is not None:
            counter = torch.tensor([c.call_dev - 2 ** 32 if c.call_dev >= 2 ** 31 else c.call_dev], dtype=torch.int32, device="cuda")
        rc = lib.lib().bbb_lrt_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), wv.data_ptr(), ptr(b), ptr(bv), y.ptr,
                                          None if am is None else am.ptr, None if av is None else av.ptr, ptr(eps), SEED, CALL0, STREAM,
                                          1 if sample else 0, ptr(counter), stream)
    assert rc == 0, (c.name, rc)
    torch.cuda.synchronize()
    for name, g in (("y", y), ("act_mu", am), ("act_var", av)):
        assert g is None or g.guards_intact(), "%s: the launch wrote outside %s" % (c.name, name)
    out = lambda g: None if g is None else g.body(torch).cpu().numpy().reshape(shape)
    return dict(y=out(y), act_mu=out(am), act_var=out(av))


# ------------------------------------------------------------------------------------------------ checkers
def _worst(err, tol, what, c):
    assert err.shape == tol.shape, (c.name, what, err.shape, tol.shape)
    assert np.isfinite(err).all(), (c.name, what, "not finite")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max())
    assert worst <= 1.0, "%s %s: error / bound = %.3f at %s" % (c.name, what, worst, np.unravel_index(np.argmax(ratio), err.shape))
    return worst


def check_rounded(c, got, ref):
    """Every element of everything the launch stored, against the float64 reference; returns {output: worst error / bound} and, where
    the stored value is the contraction itself, "chain": the worst error / ((K + 2) 2^-24 mag)."""
    assert c.K <= K_MAX, (c.name, c.K)
    sample, act = c.sample, c.act
    worst = {}
    tol_mu = 2e-5 * ref["mag"] + (0.0 if c.scale else 2e-6)
    chain = (c.K + 2) * 2.0 ** -24 * ref["mag"]
    tol_pre, want = tol_mu, ref["act_mu"]
    if c.lrt:
        if got["act_mu"] is not None:
            err = np.abs(got["act_mu"].astype(F64) - ref["act_mu"])
            worst["act_mu"] = _worst(err, tol_mu, "act_mu", c)
            worst["chain"] = float(np.max(err[chain > 0] / chain[chain > 0])) if (chain > 0).any() else 0.0
            worst["act_var"] = _worst(np.abs(got["act_var"].astype(F64) - ref["act_var"]), 3e-5 * ref["act_var"], "act_var", c)
            for e in np.nonzero(ref["zero"])[0]:
                bv = (np.zeros(c.Cout, F32) if ref["b_var"] is None else ref["b_var"])[None, :, None, None]
                assert (got["act_var"][e] == F32(1e-16) + bv).all(), "%s: act_var of the all-zero slab %d is not float32(1e-16) + b_var" % (c.name, e)
        if sample:
            tol_pre = tol_mu + np.abs(ref["eps"]) * np.sqrt(ref["act_var"]) * (3e-5 / 2 + 2.0 ** -22)
            want = ref["pre"]
    want = _act(want, act)
    tol = tol_pre + (2e-5 * np.abs(want) if act else 0.0)
    assert got["y"].shape == want.shape, (c.name, got["y"].shape, want.shape)
    err = np.abs(got["y"].astype(F64) - want)
    worst["y"] = _worst(err, tol, "y", c)
    if not act and not (c.lrt and sample) and (chain > 0).any():
        worst["chain"] = max(worst.get("chain", 0.0), float(np.max(err[chain > 0] / chain[chain > 0])))
    return worst


def check_exact(c, got, ref):
    """Dyadic operands (exact_bits(c) <= 24) and a launch without noise and without softplus: y, act_mu and act_var - float32(1e-16)
    EQUAL the float64 reference.  Returns how many elements were compared."""
    assert max(exact_bits(c)) <= 24, (c.name, exact_bits(c))
    act = c.act
    assert act != "softplus" and not (c.lrt and c.sample), "the exact tier runs quiet(c)"
    n = 0
    pairs = [("y", got["y"], _act(ref["act_mu"], act))]
    if c.lrt and got["act_mu"] is not None:
        pairs += [("act_mu", got["act_mu"], ref["act_mu"]), ("act_var - 1e-16", got["act_var"] - F32(1e-16), ref["var0"])]
    for name, g, want in pairs:
        assert g.shape == want.shape and g.dtype == F32, (c.name, name, g.shape, g.dtype)
        bad = ~(g.astype(F64) == want)                                   # (a NaN -- an element never stored -- is bad)
        assert not bad.any(), "%s: %d elements of %s differ from the exact value, first at %s" % (
            c.name, int(bad.sum()), name, np.unravel_index(np.argmax(bad), bad.shape))
        n += bad.size
    return n
