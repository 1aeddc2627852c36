"""What tests/test_pconv_sweep_cpu.py and tests/test_gpu_pconv_sweep.py share about the batch-innermost fp32 implicit GEMM
(csrc/pconv_gemm.hip, csrc/pconv_body.cuh; ops.conv2d_chwn_forward = "BBB", ops.lrt_conv2d_chwn_forward = "LRT"):

  * plan_rules: the launch rules of csrc/pconv_plan.h written out once more, independently, in Python;
  * CASES: the table of launches the GPU module runs, each naming the launch form it was written for, and case_branches(): the
    tags (form, plan edge, kernel edge, LRT feature x sampling epilogue) a case reaches;
  * reference(): one launch in float64 from oracle/bbb_numpy.py pieces (im2col without any rounding back to fp32, the Philox
    noise stream, slab / work-unit addressing);
  * two checkers: check_exact (dyadic operands: every partial sum of either contraction is an fp32 number in any order, so the
    moments must EQUAL the reference) and check_rounded (Gaussian operands, per-element bounds taken from the suite's own);
  * emulate_f32(): the same launch in numpy fp32 with one planted fault, to show on the CPU that the checkers bite.

Tolerances of the rounded tier (every element is checked):
  act_mu   |got - ref| <= 2e-5 mag + 2e-6, mag = conv(|x|, |W_mu|) + |b_mu|                          (tests/test_gpu_fuzz.py)
  act_var  |got - ref| <= 3e-5 ref; == float32(1e-16) + b_var where the input slab is all zero       (test_lrt_moments_and_output,
           without its atol)
  pre-activation  tol_mu + |eps| sqrt(ref_var) (3e-5 / 2 + 2^-22): sqrt halves the variance's relative error, and the square root
           and the product add half an ulp each (2^-24 + 2^-24 of the term, rounded up to 2^-22 for the final sum's own rounding)
  output   relu and softplus are 1-Lipschitz: the pre-activation's bound + 2e-5 |ref| for the activation's own rounding;
           max over a 2 x 2 window moves by at most the largest move of its four arguments: the largest of the window's bounds.
  BBB launches use the first line (+ the activation's term)."""
import math
from dataclasses import dataclass

import numpy as np

import bbb_numpy as O

F32, F64 = np.float32, np.float64
EINVAL, EALIGN, ESHAPE = -1, -2, -3
FORMS = ("bbb-64-ilv", "bbb-64", "bbb-128-ilv", "bbb-128", "bbb-seq64-ilv", "bbb-seq64", "bbb-seq128-ilv", "bbb-seq128",
         "bbb-cross", "bbb-pool", "lrt-64-ilv", "lrt-64", "lrt-seq64", "lrt-cross", "lrt-pool")
ILV_MAX, SPLIT_MAX_BBB, SPLIT_MAX_LRT = 12000, 384, 512
INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ launch rules
def out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw):
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def layer_ksplit(desc):
    """The layer's split of its contraction: at most 16 (pixel, 64-channel tile) groups and at least 16 k tiles of 32 -> 2..4
    ranges of at least 8 tiles; a function of the geometry only."""
    ho, wo = out_hw(desc["H"], desc["W"], desc["kh"], desc["kw"], desc["sh"], desc["sw"], desc["ph"], desc["pw"], desc["dh"], desc["dw"])
    if ho * wo * -(-desc["Cout"] // 64) > 16:
        return 1
    nr = min(desc["kh"], (desc["H"] - 1) // desc["dh"] + 1)
    nq = min(desc["kw"], (desc["W"] - 1) // desc["dw"] + 1)
    tiles = -(-desc["Cin"] * nr * nq // 32)
    return 1 if tiles < 16 else min(4, tiles // 8)


def plan_rules(desc, lrt, k_split, has_scratch):
    """desc: dict B, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, draws, pool -> dict(form, bm, ilv, items, blocks) or the refusal
    code.  Only geometries whose slabs fit 32-bit byte offsets (the sweep stays far inside)."""
    if min(desc[k] for k in ("B", "Cin", "H", "W", "Cout", "kh", "kw", "sh", "sw", "dh", "dw", "draws")) <= 0 or min(desc["ph"], desc["pw"]) < 0:
        return EINVAL
    if desc["B"] % 4:
        return ESHAPE
    ho, wo = out_hw(desc["H"], desc["W"], desc["kh"], desc["kw"], desc["sh"], desc["sw"], desc["ph"], desc["pw"], desc["dh"], desc["dw"])
    if ho <= 0 or wo <= 0:
        return ESHAPE
    if desc["pool"] not in (0, 1) or (desc["pool"] and (ho % 2 or wo % 2)):
        return EINVAL
    if k_split > 1 and k_split != layer_ksplit(desc):
        return EINVAL
    split = k_split > 1
    B, pixels, G = desc["B"], ho * wo, -(-desc["Cout"] // 64) * desc["draws"]
    if desc["pool"]:
        if split:
            return EINVAL
        bm = 64 if lrt else 128
        items = G * (pixels // 4) * -(-B // bm)
        if items > INT_MAX - 8:
            return ESHAPE
        return dict(form="lrt-pool" if lrt else "bbb-pool", bm=bm, ilv=False, items=items, blocks=8 * -(-items // 8))
    t128, t64 = -(-B // 128), -(-B // 64)
    wide = not lrt and pixels * t128 * G >= 768 and not (t128 * 128 * 4 >= B * 5 and t64 * 64 < t128 * 128)
    items64 = pixels * t64 * G
    if split and has_scratch and items64 <= (SPLIT_MAX_LRT if lrt else SPLIT_MAX_BBB):
        return dict(form="lrt-cross" if lrt else "bbb-cross", bm=64, ilv=True, items=items64, blocks=8 * -(-items64 * k_split // 8))
    bm = 128 if wide else 64
    items = pixels * -(-B // bm) * G
    blocks = 8 * -(-items // 8)
    if blocks > INT_MAX:
        return ESHAPE
    ilv = items <= ILV_MAX
    if lrt:
        form, ilv = ("lrt-seq64", False) if split else ("lrt-64-ilv" if ilv else "lrt-64", ilv)
    else:
        form = "bbb-" + ("seq" if split else "") + str(bm) + ("-ilv" if ilv else "")
    return dict(form=form, bm=bm, ilv=ilv, items=items, blocks=blocks)


def conv_desc(lib, desc):
    d = lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = (desc[k] for k in ("B", "Cin", "H", "W", "Cout", "kh", "kw"))
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = (desc[k] for k in ("sh", "sw", "ph", "pw", "dh", "dw"))
    d.draws, d.pool = desc["draws"], desc["pool"]
    d.x_draw_stride = desc["Cin"] * desc["H"] * desc["W"] * desc["B"]
    return d


def plan_query(lib, desc, lrt, k_split, has_scratch):
    """bbb_conv2d_chwn_plan on the same descriptor, in plan_rules' terms."""
    import ctypes
    fm, bm, ilv, items, blocks = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib.lib().bbb_conv2d_chwn_plan(ctypes.byref(conv_desc(lib, desc)), int(lrt), k_split, int(has_scratch), ctypes.byref(fm),
                                        ctypes.byref(bm), ctypes.byref(ilv), ctypes.byref(items), ctypes.byref(blocks))
    if rc != 0:
        return rc
    return dict(form=FORMS[fm.value], bm=bm.value, ilv=bool(ilv.value), items=items.value, blocks=blocks.value)


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    form: str                         # the launch form this case was written for (ops.fp32_fwd_plan confirms it)
    B: int
    Cin: int
    H: int
    W: int
    Cout: int
    k: tuple = (1, 1)
    s: tuple = (1, 1)
    p: tuple = (0, 0)
    d: tuple = (1, 1)
    E: int = 1                        # output slabs of the launch
    x: tuple = ("draw",)              # ("draw",) one input slab per output slab | ("shared",) BBB: one slab, x_draw_stride 0 |
                                      # ("div", D, off) slab e reads (e + off) // D | ("units", S, off, per_slice) work units
    w_shared: bool = False            # BBB: one weight set for every slab
    bias: bool = True
    act: str = None
    pool: bool = False
    wtap: bool = False                # BBB: weights given tap-major
    sample: bool = True               # LRT ...
    ext_eps: bool = False
    moments: bool = False
    b_offset: int = 0
    call_dev: int = None              # value of the device-side call counter during the launch (None: no counter, a NULL pointer)
    zero_slab: int = None             # this input slab is all zero
    seed: int = 0                     # of the operands: cases with the same seed and geometry share their slabs
    tags: tuple = ()

    @property
    def lrt(self):
        return self.form.startswith("lrt")

    @property
    def desc(self):
        return dict(B=self.B, Cin=self.Cin, H=self.H, W=self.W, Cout=self.Cout, kh=self.k[0], kw=self.k[1], sh=self.s[0], sw=self.s[1],
                    ph=self.p[0], pw=self.p[1], dh=self.d[0], dw=self.d[1], draws=self.E, pool=int(self.pool))

    @property
    def out_hw(self):
        return out_hw(self.H, self.W, *self.k, *self.s, *self.p, *self.d)

    # slab e -> (input slab, weight set / call increment, global index of local image 0)
    def slab(self, e):
        if self.x[0] == "units":
            S, off = self.x[1], self.x[2] % self.x[1]
            u = off + e
            return (u % S if self.x[3] else e), u // S, self.b_offset + (u % S) * self.B
        if self.x[0] == "div":
            return (e + self.x[2]) // self.x[1], e, self.b_offset
        return (0 if self.x[0] == "shared" else e), e, self.b_offset

    @property
    def x_slabs(self):
        if self.x[0] == "units" and self.x[3]:
            return self.x[1]
        return 1 + max(self.slab(e)[0] for e in range(self.E))

    @property
    def w_sets(self):
        return 1 if (self.lrt or self.w_shared) else 1 + max(self.slab(e)[1] for e in range(self.E))


SEED, CALL0, STREAM = 0x1234567887654321, 41, 6          # of the LRT noise


def keff_set(c):
    """Contraction length Cin * (in-bounds taps) of every output pixel."""
    ho, wo = c.out_hw
    def taps(n_out, size, k, s, p, d):
        return [sum(0 <= o * s - p + r * d < size for r in range(k)) for o in range(n_out)]
    th, tw = taps(ho, c.H, c.k[0], c.s[0], c.p[0], c.d[0]), taps(wo, c.W, c.k[1], c.s[1], c.p[1], c.d[1])
    return {c.Cin * a * b for a in th for b in tw}


def step_major(c, ntiles):
    """pconv_body.cuh, item enumeration: (step, pixel, image tile) major when the draws of a step share their input."""
    if c.x[0] == "shared":
        return True
    return c.x[0] == "div" and c.x[1] > 1 and c.x[2] == 0 and (ntiles * c.E) % (c.x[1] * ntiles) == 0


def epilogue(form):
    return {"lrt-cross": "cross", "lrt-pool": "pool"}.get(form, "plain")


def case_branches(c, plan):
    """Tags one case reaches; plan = ops.fp32_fwd_plan(...) of the case."""
    form, bm, ilv, items, blocks, ks = plan
    kind = "lrt" if c.lrt else "bbb"
    t = {form}
    ke = keff_set(c)
    tiles = -(-max(ke) // 32)
    for name, hit in (("keff:1", 1 in ke), ("keff:<32", any(0 < v < 32 for v in ke)), ("keff:%32", any(v % 32 for v in ke)),
                      ("keff:256", 256 in ke), ("keff:257", 257 in ke), ("keff:>512", max(ke) > 512),
                      ("taps:ragged", len(ke - {0}) > 1), ("taps:none", 0 in ke), ("kh!=kw", c.k[0] != c.k[1]), ("H!=W", c.H != c.W),
                      ("stride:2x1", c.s == (2, 1)), ("stride:3", 3 in c.s), ("dil:2", 2 in c.d), ("nobias", not c.bias),
                      ("act:" + str(c.act), True), ("cout:%d" % c.Cout, c.Cout in (1, 33, 65, 100)), ("B:%d" % c.B, c.B in (4, 68, 132, 260)),
                      ("enum:step-major", step_major(c, -(-c.Cout // 64))), ("enum:draw-major", not step_major(c, -(-c.Cout // 64))),
                      ("x_div+off", c.x[0] == "div" and c.x[1] > 1 and c.x[2] != 0)):
        if hit:
            t.add(kind + ":" + name)
    if ks > 1:
        t.add("ksplit:%d" % ks)
        if tiles % ks:
            t.add("ksplit:ragged-ranges")
    ho, wo = c.out_hw
    if ks == 1 and tiles == 15 and ho * wo * -(-c.Cout // 64) <= 16:
        t.add("ksplit:below:15-tiles")
    if ks == 1 and tiles >= 16 and ho * wo * -(-c.Cout // 64) == 17:
        t.add("ksplit:below:17-groups")
    if form in ("bbb-cross", "lrt-cross", "bbb-seq64-ilv", "lrt-seq64") and items in (384, 385, 512, 513):
        t.add("edge:%s:%d" % (kind, items))
    if not c.lrt and bm == 64 and ho * wo * -(-c.B // 128) * -(-c.Cout // 64) * c.E >= 768:
        t.add("tile:128-declined")
    if c.wtap:
        t.add("bbb:w_tap_major")
    if c.lrt:
        ep = epilogue(form)
        for name, hit in (("nosample", not c.sample), ("ext-eps", c.ext_eps and c.sample), ("moments", c.moments), ("b_offset", c.b_offset != 0),
                          ("units:ragged", c.x[0] == "units" and c.x[2] % c.x[1] != 0 and c.E % c.x[1] != 0),
                          ("pool:ragged", c.pool and c.B % 64 != 0 and c.Cout % 64 != 0), ("zero-slab", c.zero_slab is not None),
                          ("call_dev", c.call_dev is not None and c.sample and not c.ext_eps), ("n_slabs", c.x[0] == "div" and c.E % c.x[1] != 0)):
            if hit:
                t.add("lrt:%s:%s" % (ep, name))
    return t | set(c.tags)


def wanted_tags():
    """Every form, plan edge, kernel edge (on a BBB and on an LRT case) and LRT feature (with each sampling epilogue) of the sweep."""
    want = set(FORMS) | {"ksplit:2", "ksplit:3", "ksplit:4", "ksplit:ragged-ranges", "ksplit:below:15-tiles", "ksplit:below:17-groups",
                         "edge:bbb:384", "edge:bbb:385", "edge:lrt:512", "edge:lrt:513", "tile:128-declined", "bbb:w_tap_major"}
    for kind in ("bbb", "lrt"):
        want |= {kind + ":" + n for n in ("keff:1", "keff:<32", "keff:%32", "keff:256", "keff:257", "keff:>512", "taps:ragged", "taps:none",
                                          "kh!=kw", "H!=W", "stride:2x1", "stride:3", "dil:2", "nobias", "act:None", "act:relu", "act:softplus",
                                          "cout:1", "cout:33", "cout:65", "cout:100", "B:4", "B:68", "B:132", "B:260",
                                          "enum:step-major", "enum:draw-major", "x_div+off")}
    for ep in ("plain", "cross", "pool"):
        want |= {"lrt:%s:%s" % (ep, n) for n in ("nosample", "ext-eps", "b_offset", "units:ragged", "zero-slab", "call_dev")}
    want |= {"lrt:plain:moments", "lrt:cross:moments", "lrt:pool:pool:ragged", "lrt:plain:n_slabs"}        # (a pooled launch keeps no moments)
    return want


def _cases():
    C = Case
    U = lambda S, off, per=False: ("units", S, off, per)
    cs = [
        # ---- BBB, the plain forms ------------------------------------------------------------------------------------------------
        C("bbb-k1", "bbb-64-ilv", 4, 1, 5, 7, 1, E=2, act="relu"),                                         # K_eff 1, one image quad, one channel
        C("bbb-3x3-pad3", "bbb-64-ilv", 68, 3, 6, 5, 33, (3, 3), p=(3, 3), E=2, act="softplus"),           # pixels no tap reaches, K_eff 3..27
        C("bbb-5x2-s2x1-d2", "bbb-64-ilv", 132, 8, 11, 9, 65, (5, 2), (2, 1), (4, 1), (2, 2), E=2, bias=False, wtap=True),
        C("bbb-s3-k256", "bbb-64-ilv", 260, 64, 7, 8, 100, (2, 2), (3, 3), (1, 1), E=1, act="relu", x=("shared",)),   # K_eff 64, 128, 256
        C("bbb-k257", "bbb-64-ilv", 8, 257, 3, 3, 10, x=("div", 2, 1), E=3),                              # a 257th table entry; x_div with an offset
        C("bbb-k>512", "bbb-64-ilv", 8, 65, 5, 4, 10, (3, 3), p=(1, 1), x=("div", 2, 0), E=4, wtap=True),  # K_eff 260, 390, 585 (three table chunks)
        C("bbb-units", "bbb-64-ilv", 8, 5, 6, 6, 70, (3, 3), p=(1, 1), x=U(3, 2), E=5, act="relu"),
        C("bbb-units-x-per-slice", "bbb-64-ilv", 8, 5, 6, 6, 10, (3, 3), p=(1, 1), x=U(3, 1, True), E=4),
        C("bbb-128-ilv", "bbb-128-ilv", 324, 3, 16, 16, 8, x=("shared",), act="relu"),                     # 768 items of 128 images, ragged third tile
        C("bbb-128-ilv-3x3", "bbb-128-ilv", 68, 9, 10, 10, 65, (3, 3), p=(1, 1), E=4, w_shared=True, act="softplus"),
        C("bbb-128", "bbb-128", 128, 3, 16, 16, 8, x=("shared",), E=48, act="relu"),                       # 12288 items: staging up front
        C("bbb-64-declined", "bbb-64", 192, 3, 8, 8, 8, x=("shared",), E=63),                              # 128-image tiles declined, 12096 items
        C("bbb-pool", "bbb-pool", 132, 3, 12, 8, 70, (3, 3), p=(1, 1), E=2, act="relu", pool=True),
        C("bbb-pool-pad", "bbb-pool", 68, 2, 6, 6, 5, (3, 3), p=(3, 3), E=2, x=("shared",), act="softplus", pool=True),
        # ---- BBB, the layer's split --------------------------------------------------------------------------------------------------
        C("bbb-cross-384", "bbb-cross", 64, 512, 1, 1, 4, x=("shared",), E=384, seed=7),                   # k_split 2
        C("bbb-seq-385", "bbb-seq64-ilv", 64, 512, 1, 1, 4, x=("shared",), E=385, seed=7),
        C("bbb-cross-k3", "bbb-cross", 68, 86, 4, 4, 33, (3, 3), (2, 2), (1, 1), E=2, act="relu"),          # 2 x 2 pixels, 25 k tiles in 3 ranges
        C("bbb-cross-k4", "bbb-cross", 8, 260, 2, 2, 100, (3, 3), p=(1, 1), E=2, act="softplus", bias=False),   # 2 x 2 pixels x 2 tiles, 33 k tiles in 4
        C("bbb-15-tiles", "bbb-64-ilv", 8, 480, 2, 2, 10, E=2),                                           # 15 k tiles: no split
        C("bbb-17-groups", "bbb-64-ilv", 8, 512, 17, 1, 10, E=2),                                         # 17 pixels: no split
        C("bbb-seq64", "bbb-seq64", 192, 512, 2, 2, 4, x=("shared",), E=1004),                             # 12048 items of 64 images
        C("bbb-seq128-ilv", "bbb-seq128-ilv", 128, 512, 1, 1, 4, x=("shared",), E=768, act="relu"),
        C("bbb-seq128", "bbb-seq128", 1024, 512, 2, 2, 4, x=("shared",), E=376),                           # 12032 items of 128 images
        # ---- LRT, the plain epilogue -------------------------------------------------------------------------------------------------
        C("lrt-k1", "lrt-64-ilv", 4, 1, 5, 7, 1, E=2, act="relu", moments=True),
        C("lrt-3x3-pad3", "lrt-64-ilv", 68, 3, 6, 5, 33, (3, 3), p=(3, 3), E=2, act="softplus", moments=True, b_offset=12),
        C("lrt-5x2-s2x1-d2", "lrt-64-ilv", 132, 8, 11, 9, 65, (5, 2), (2, 1), (4, 1), (2, 2), E=2, bias=False, sample=False, moments=True),
        C("lrt-s3-k256", "lrt-64-ilv", 260, 64, 7, 8, 100, (2, 2), (3, 3), (1, 1), E=2, x=("div", 2, 0), act="relu", ext_eps=True),
        C("lrt-k257", "lrt-64-ilv", 8, 257, 3, 3, 10, x=("div", 2, 1), E=3, call_dev=5),
        C("lrt-k>512", "lrt-64-ilv", 8, 65, 5, 4, 10, (3, 3), p=(1, 1), x=("div", 3, 0), E=5, call_dev=2 ** 32 - 3),   # n_slabs 5 of 2 x 3
        C("lrt-units", "lrt-64-ilv", 8, 5, 6, 6, 70, (3, 3), p=(1, 1), x=U(3, 2), E=5, act="relu", b_offset=24, zero_slab=1, moments=True),
        C("lrt-units-x-per-slice", "lrt-64-ilv", 8, 5, 6, 6, 10, (3, 3), p=(1, 1), x=U(3, 1, True), E=4, zero_slab=2, bias=False),
        C("lrt-64", "lrt-64", 64, 3, 16, 16, 8, x=("div", 48, 0), E=48, act="relu", moments=True),                       # 12288 items: staging up front
        C("lrt-15-tiles", "lrt-64-ilv", 8, 480, 2, 2, 10, E=2, moments=True),
        C("lrt-17-groups", "lrt-64-ilv", 8, 512, 17, 1, 10, E=2),
        C("lrt-seq-513", "lrt-seq64", 64, 512, 1, 1, 4, x=("div", 513, 0), E=513, seed=9, act="relu"),
        C("lrt-seq-features", "lrt-seq64", 68, 86, 4, 4, 33, (3, 3), (2, 2), (1, 1), x=U(3, 2), E=65, b_offset=8, moments=True, zero_slab=3),
        # ---- LRT, the cross-workgroup epilogue -----------------------------------------------------------------------------------------
        C("lrt-cross-512", "lrt-cross", 64, 512, 1, 1, 4, x=("div", 512, 0), E=512, seed=9, act="relu"),
        C("lrt-cross-k3", "lrt-cross", 68, 86, 4, 4, 33, (3, 3), (2, 2), (1, 1), x=U(3, 2), E=5, b_offset=8, moments=True, zero_slab=3,
          act="softplus", call_dev=5),
        C("lrt-cross-k4", "lrt-cross", 8, 260, 2, 2, 100, (3, 3), p=(1, 1), x=("div", 2, 1), E=3, ext_eps=True, bias=False, moments=True),
        C("lrt-cross-nosample", "lrt-cross", 12, 512, 2, 2, 65, E=2, sample=False, act="relu"),
        # ---- LRT, the pooled epilogue --------------------------------------------------------------------------------------------------
        C("lrt-pool", "lrt-pool", 132, 3, 12, 8, 70, (3, 3), p=(1, 1), x=U(3, 2), E=5, act="relu", pool=True, b_offset=8, zero_slab=1, call_dev=4),
        C("lrt-pool-ext", "lrt-pool", 68, 2, 6, 6, 5, (3, 3), p=(3, 3), E=2, act="softplus", pool=True, ext_eps=True, bias=False),
        C("lrt-pool-nosample", "lrt-pool", 8, 40, 4, 6, 65, (3, 3), p=(1, 1), E=2, x=("div", 2, 0), pool=True, sample=False),
    ]
    return {c.name: c for c in cs}


CASES = _cases()
PAIRS = (("bbb-cross-384", "bbb-seq-385"), ("lrt-cross-512", "lrt-seq-513"))        # same layer across the cross / SEQ boundary: same bits


def case_plan(c):
    from bbb_hip import ops
    return ops.fp32_fwd_plan((c.x_slabs, c.Cin, c.H, c.W, c.B), (1, c.Cout, c.Cin) + c.k, c.s, c.p, c.d, draws=c.E, lrt=c.lrt, pool=c.pool)


# ------------------------------------------------------------------------------------------------ operands
def exact_bits(c):
    """The exactness precondition of the exact tier: operands are x in {-2..2}, W_mu multiples of 1/8 in [-1, 1], sigma^2 multiples
    of 1/64 in [1/64, 1/4], b_mu multiples of 1/8 in [-2, 2], b_var multiples of 1/64 in [1/64, 1/4].  Every partial sum of the mean
    contraction is a multiple of 2^-3 of magnitude <= 2 K + 2, of the variance contraction a multiple of 2^-6 <= K + 1/4 (x^2 <= 4):
    -> (integer bits + fractional bits) of the two; both must be <= 24 for every partial sum to be an fp32 number in ANY order."""
    K = c.Cin * c.k[0] * c.k[1]
    return math.ceil(math.log2(2 * K + 2 + 1)) + 3, math.ceil(math.log2(K + 1)) + 6


def _rng(c, kind, i):
    return np.random.default_rng([c.seed, {"x": 1, "w": 2, "s": 3, "b": 4, "v": 5, "e": 6}[kind], i, c.B, c.Cin, c.Cout])


def operands(c, tier):
    """x [slabs, Cin, H, W, B], w [sets, Cout, Cin, kh, kw] (reference order), w_var | None, b [sets, Cout] | None, b_var | None,
    eps [E, Cout, Ho, Wo, B] | None -- float32, generated per slab so that cases sharing seed and geometry share slabs."""
    ex = tier == "exact"
    shp = (c.Cin, c.H, c.W, c.B)
    x = np.stack([(_rng(c, "x", i).integers(-2, 3, shp) if ex else _rng(c, "x", i).standard_normal(shp)).astype(F32)
                  for i in range(c.x_slabs)])
    if c.zero_slab is not None:
        x[c.zero_slab] = 0
    wshape = (c.Cout, c.Cin) + c.k
    w = np.stack([(_rng(c, "w", i).integers(-8, 9, wshape) / 8 if ex else _rng(c, "w", i).standard_normal(wshape) * 0.3).astype(F32)
                  for i in range(c.w_sets)])
    b = bv = wv = eps = None
    if c.bias:
        b = np.stack([(_rng(c, "b", i).integers(-16, 17, c.Cout) / 8 if ex else _rng(c, "b", i).standard_normal(c.Cout)).astype(F32)
                      for i in range(c.w_sets)])
    if c.lrt:
        wv = (_rng(c, "s", 0).integers(1, 17, wshape) / 64 if ex else _rng(c, "s", 0).uniform(0.01, 0.3, wshape) ** 2).astype(F32)
        w, b = w[0], (None if b is None else b[0])
        if c.bias:
            bv = (_rng(c, "v", 0).integers(1, 17, c.Cout) / 64 if ex else _rng(c, "v", 0).uniform(0.01, 0.3, c.Cout) ** 2).astype(F32)
        if c.ext_eps and c.sample:
            ho, wo = c.out_hw
            eps = np.stack([_rng(c, "e", e).standard_normal((c.Cout, ho, wo, c.B)).astype(F32) for e in range(c.E)])
    return dict(x=x, w=w, w_var=wv, b=b, b_var=bv, eps=eps)


# ------------------------------------------------------------------------------------------------ the launch in numpy
def _act(v, act):
    if act == "relu":
        return np.maximum(v, v.dtype.type(0))
    if act == "softplus":
        return np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, 20))))
    return v


def _pool(v):
    """MaxPool2d(2, 2) of [..., Ho, Wo, B]."""
    return np.maximum(np.maximum(v[..., 0::2, 0::2, :], v[..., 0::2, 1::2, :]), np.maximum(v[..., 1::2, 0::2, :], v[..., 1::2, 1::2, :]))


def _noise(c, call, bglob, ho, wo, shift=0):
    """[Cout, Ho, Wo, B]: element ((b_global Cout + n) Ho Wo + pixel) of the stream (SEED, call, STREAM)."""
    n = c.B * c.Cout * ho * wo
    z = O.normal_eps(SEED, call & 0xFFFFFFFF, STREAM, n, start=bglob * c.Cout * ho * wo + shift)
    return z.reshape(c.B, c.Cout, ho, wo).transpose(1, 2, 3, 0)


FAULTS = ("var-pad-tap", "var-x-not-squared", "no-1e-16", "noise-shift", "noise-call", "local-image", "no-bias-var", "drop-last-range",
          "pool-skip-pixel", "tap-table-256")


def forward(c, ops_, dtype=F64, fault=None):
    """One launch of case c on the operands ops_ in `dtype` arithmetic: float64 = the reference; float32 = the emulation, with one of
    FAULTS planted.  Returns act_mu, act_var (LRT), pre (pre-activation), out (activated, unpooled), y (what the launch stores),
    eps, mag = conv(|x|, |w|) + |b|, zero = slabs whose input is all zero; all [E, Cout, Ho, Wo, B] (y: pooled when c.pool)."""
    ho, wo = c.out_hw
    K = c.Cin * c.k[0] * c.k[1]
    cols_cache, res = {}, {}

    def cols(ix, what):
        key = (ix, what)
        if key not in cols_cache:
            xs = ops_["x"][ix].transpose(3, 0, 1, 2).astype(dtype)                       # [B, Cin, H, W]
            xs = {"x": xs, "abs": np.abs(xs), "sq": xs * xs if fault != "var-x-not-squared" else xs}[what]
            if what == "sq" and fault == "var-pad-tap":
                # the padded corner reads its valid neighbour instead of zero: ONE tap of the corner pixel, variance contraction only
                assert c.p[0] > 0 and c.p[1] > 0 and c.d == (1, 1) and c.s == (1, 1) and c.p[0] < c.k[0] and c.p[1] < c.k[1]
                xp = np.zeros((c.B, c.Cin, c.H + 2 * c.p[0], c.W + 2 * c.p[1]), dtype)
                xp[:, :, c.p[0]:c.p[0] + c.H, c.p[1]:c.p[1] + c.W] = xs
                xp[:, :, c.p[0] - 1, c.p[1] - 1] = xs[:, :, 0, 0]
                cols_cache[key] = O.im2col(xp, *c.k, c.s, 0, c.d)[0]
            else:
                cols_cache[key] = O.im2col(xs, *c.k, c.s, c.p, c.d)[0]                 # [B Ho Wo, K], k = (ci, r, q)
        return cols_cache[key]

    def contract(m, wmat):
        """[B Ho Wo, K] x [Cout, K] -> [Cout, Ho, Wo, B]"""
        wm = wmat.reshape(c.Cout, K).astype(dtype)
        if fault == "tap-table-256" and K > 256:
            wm = wm.copy()
            wm[:, 256:] = wm[:, :K - 256]                                               # entries from 256 on repeat the first chunk's
        if fault == "drop-last-range":
            tiles = -(-K // 32)
            m, wm = m[:, :32 * (tiles * 2 // 3)], wm[:, :32 * (tiles * 2 // 3)]         # the third of three ranges never added
        return (m @ wm.T).reshape(c.B, ho, wo, c.Cout).transpose(3, 1, 2, 0)

    outs = {k: [] for k in ("act_mu", "act_var", "pre", "out", "eps", "mag")}
    for e in range(c.E):
        ix, iw, bglob = c.slab(e)
        ws = 0 if (c.lrt or c.w_shared) else iw
        w = ops_["w"] if c.lrt else ops_["w"][ws]
        b = None if ops_["b"] is None else (ops_["b"] if c.lrt else ops_["b"][ws])
        key = (ix, ws)
        if key not in res:
            mu = contract(cols(ix, "x"), w)
            mag = contract(cols(ix, "abs"), np.abs(w))
            if b is not None:
                mu = mu + b.astype(dtype)[:, None, None, None]
                mag = mag + np.abs(b).astype(dtype)[:, None, None, None]
            var = None
            if c.lrt:
                var = contract(cols(ix, "sq"), ops_["w_var"])
                if ops_["b_var"] is not None and fault != "no-bias-var":
                    var = var + ops_["b_var"].astype(dtype)[:, None, None, None]
                if fault != "no-1e-16":
                    var = dtype(F32(1e-16)) + var
            res[key] = (mu, var, mag)
        mu, var, mag = res[key]
        pre, z = mu, None
        if c.lrt and c.sample:
            if ops_["eps"] is not None:
                z = ops_["eps"][e].astype(dtype)
            else:
                call = CALL0 + (c.call_dev or 0) + iw + (1 if fault == "noise-call" else 0)
                z = _noise(c, call, 0 if fault == "local-image" else bglob, ho, wo, 1 if fault == "noise-shift" else 0).astype(dtype)
            with np.errstate(invalid="ignore"):                                        # (a planted fault may make the variance negative)
                pre = mu + np.sqrt(var) * z
        for k, v in (("act_mu", mu), ("act_var", var), ("pre", pre), ("out", _act(pre, c.act)), ("eps", z), ("mag", mag)):
            outs[k].append(v)
    r = {k: (np.stack(v) if v[0] is not None else None) for k, v in outs.items()}
    r["y"] = r["out"]
    if c.pool:
        o = r["out"]
        if fault == "pool-skip-pixel":
            o = o.copy()
            o[..., 1::2, 1::2, :] = -np.inf                                             # the window's fourth pixel never enters the maximum
        r["y"] = _pool(o)
    r["b_var"] = ops_["b_var"]
    r["zero"] = np.array([not ops_["x"][c.slab(e)[0]].any() for e in range(c.E)])
    return r


def reference(c, ops_):
    return forward(c, ops_, F64)


def emulate_f32(c, ops_, fault=None):
    """What a launch with this fault would store: y, and the moments when the case asks for them."""
    r = forward(c, ops_, F32, fault)
    want = c.lrt and c.moments
    return dict(y=r["y"].astype(F32), act_mu=r["act_mu"].astype(F32) if want else None, act_var=r["act_var"].astype(F32) if want else None)


# ------------------------------------------------------------------------------------------------ checkers
def _worst(err, tol, what, c):
    assert err.shape == tol.shape, (c.name, what, err.shape, tol.shape)
    assert np.isfinite(err).all(), (c.name, what, "not finite")
    ratio = float(np.max(err / tol))
    assert ratio <= 1.0, "%s %s: error / bound = %.3f at %s" % (c.name, what, ratio, np.unravel_index(np.argmax(err / tol), err.shape))
    return ratio


def check_rounded(c, got, ref):
    """Every element of everything the launch stored, against the float64 reference; returns {output: worst error / bound}."""
    worst = {}
    tol_mu = 2e-5 * ref["mag"] + 2e-6
    tol_pre = tol_mu
    if c.lrt:
        if got["act_mu"] is not None:
            worst["act_mu"] = _worst(np.abs(got["act_mu"].astype(F64) - ref["act_mu"]), tol_mu, "act_mu", c)
            worst["act_var"] = _worst(np.abs(got["act_var"].astype(F64) - ref["act_var"]), 3e-5 * ref["act_var"], "act_var", c)
            for e in np.nonzero(ref["zero"])[0]:
                want = F32(1e-16) + (np.zeros(c.Cout, F32) if ref["b_var"] is None else ref["b_var"])[:, None, None, None]
                assert (got["act_var"][e] == want).all(), "%s: act_var of the all-zero slab %d is not float32(1e-16) + b_var" % (c.name, e)
        if c.sample:
            tol_pre = tol_mu + np.abs(ref["eps"]) * np.sqrt(ref["act_var"]) * (3e-5 / 2 + 2.0 ** -22)
    tol = tol_pre + (2e-5 * np.abs(ref["out"]) if c.act else 0.0)
    want = ref["y"]
    if c.pool:
        tol = _pool(tol)
    assert got["y"].shape == want.shape, (c.name, got["y"].shape, want.shape)
    worst["y"] = _worst(np.abs(got["y"].astype(F64) - want), tol, "y", c)
    return worst


def check_exact(c, got, ref):
    """Dyadic operands (exact_bits(c) <= 24): the moments, and y where no noise and no transcendental enters it, EQUAL the float64
    reference; a sampled or softplus output is held to the rounded tier's bound.  Returns how many elements were compared for equality."""
    assert max(exact_bits(c)) <= 24, (c.name, exact_bits(c))
    n = 0
    if c.lrt and got["act_mu"] is not None:
        for k in ("act_mu", "act_var"):
            bad = got[k].astype(F64) != ref[k].astype(F32).astype(F64)
            assert not bad.any(), "%s: %d elements of %s differ from the exact value, first at %s" % (
                c.name, int(bad.sum()), k, np.unravel_index(np.argmax(bad), bad.shape))
            n += bad.size
    if (c.lrt and c.sample) or c.act == "softplus":
        # the sum mu + sd * eps is rounded, and softplus is a transcendental whose tail underflows in fp32: the rounded tier's bound
        check_rounded(c, dict(got, act_mu=None, act_var=None), ref)
    else:
        bad = got["y"].astype(F64) != ref["y"]
        assert not bad.any(), "%s: %d elements of y differ from the exact value, first at %s" % (
            c.name, int(bad.sum()), np.unravel_index(np.argmax(bad), bad.shape))
        n += got["y"].size
    return n
