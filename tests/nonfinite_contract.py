"""What tests/test_nonfinite_cpu.py and tests/test_gpu_nonfinite.py share: the forward's contract on NaN and Inf operands.

A case is (entry, geometry, poison).  Its operands are O(1) Gaussians (nothing overflows on its own in fp32 or bf16) with ONE
element -- of the input, of a weight or of a bias -- replaced by NaN, +Inf or -Inf, or ("pair") two input elements of one receptive
field replaced by +Inf and -Inf.  The reference is the float64 evaluation of the entry on the poisoned operands (torch on the CPU;
the LRT noise is the device's own stream: ops.eps_dump on the GPU, oracle/bbb_numpy.normal_eps -- the same Philox stream -- where
there is no device; relu / softplus are torch's, which tests/test_nonfinite_cpu.py holds to the oracle's relu_act / softplus_act on
non-finite arguments).  Two assertions per case, neither with a tolerance (check()):

  class map   every output element is finite / NaN / +Inf / -Inf, and the device's map equals the reference's ("exact" outputs).
              "mask" outputs only have to agree on finite / non-finite:
                * entries that carry values as three bf16 pieces (gemm_mode "bf16x3", conv2d_c8x3_forward, the S3 and c8 S3 layouts
                  and their pools, their LRT forms): hi = bf16(Inf) = Inf, mid = bf16(Inf - hi) = NaN, so an Inf is (inf, nan, nan)
                  and joins to NaN -- Inf and NaN cannot be told apart.  For these entries the REFERENCE replaces an Inf of an
                  operand that travels in pieces (input, weight; not the fp32 bias) by NaN before it evaluates: behind a ReLU a
                  -Inf would otherwise be a finite 0 in the reference and a NaN on the device;
                * the LRT sampled output y under an Inf poison: mu = +-Inf and sqrt(var) * eps = +-Inf meet with the sign of eps.
              The LRT moments always get the exact class.
  locality    every element the poison does not reach is bitwise what the SAME launch (same seed and call) returns on the clean
              operands: images, channels and draws the poison does not reach must not notice it (LDS staging, wave reductions,
              split-k scratch, the zero images of an odd batch).  "Does not reach" is read off the reference (reach()): the float64
              evaluation with every poisoned element set to NaN is NOT NaN there -- a NaN marks everything that depends on it.  (Finite alone is not enough: relu(-Inf) and
              softplus(-Inf) are a finite 0 that the poison produced, in torch as here, and a softmax row with a +Inf entry holds
              finite zeros.  Such an element is held by the class map and, where the reference's value is an exact zero -- relu or
              softplus of -Inf, outside the fused-pool forms --, to that zero; any other finite value the poison makes is an
              arithmetic result of the remaining operands and has no tolerance-free reference.)  Compared with ==, so the sign of
              a zero is not part of the contract.

Out of scope:
  * padding taps: a NaN weight at a tap that touches only padding for some output pixel poisons that pixel in torch (0 * NaN) and
    not here (padding is never multiplied).  Weight poisons therefore sit at the centre tap of an odd kernel with pad <= (k-1)/2,
    which always reads a real pixel;
  * the backward kernels (first-maximum routing, act' from a NaN output): once the forward propagates, the loss is NaN already;
  * a -Inf that an entry maps to a finite value everywhere (relu(-Inf) = 0, max(-Inf, finite)): such a case poisons nothing and is
    not in the table (non-vacuity, tests/test_nonfinite_cpu.py).

Shapes: B = 8, 16 channels (32 for the c8-input bf16 form, 3 for the pooled bf16 first-layer forms, 512 x 1 x 1 for the layer with a
split contraction), 8 x 8 maps, E = 2 -- the shapes tests/infer_schedule_recorder.py uses to reach every form."""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import bbb_numpy as O

F64 = torch.float64
SEED, CALL0, STREAM = 0x5EED00012345, 17, 6
NAN, PINF, NINF, PAIR = "nan", "+inf", "-inf", "pair"
VALUE = {NAN: float("nan"), PINF: float("inf"), NINF: float("-inf")}
ACTS = (None, "relu", "softplus")
FINITE, IS_NAN, IS_PINF, IS_NINF = 0, 1, 2, 3
SCALAR_OUTPUTS = ("kl", "loss")          # exempt from "at least half of the elements are untouched": one element, poisoned by design


def classes(a):
    """finite 0 / NaN 1 / +Inf 2 / -Inf 3 of every element."""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), IS_NAN, np.where(np.isposinf(a), IS_PINF, np.where(np.isneginf(a), IS_NINF, FINITE))).astype(np.int8)


@dataclass(frozen=True)
class Case:
    id: str
    entry: str            # the bbb_hip.ops / ensemble / train entry the case launches (ENTRIES)
    family: str
    p: tuple              # sorted (key, value) pairs: variant and geometry
    place: str            # which operand holds the poison
    poison: str

    @property
    def params(self):
        return dict(self.p)

    @property
    def group(self):
        """Cases of one group share operands and the clean launch."""
        return (self.family, self.p)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) % (2 ** 31))


def _act64(v, act):
    return v if act is None else (F.relu(v) if act == "relu" else F.softplus(v))


def default_eps(call, n):
    """n elements of the noise stream (SEED, call, STREAM) from the oracle's Philox; the GPU module passes ops.eps_dump instead."""
    return O.normal_eps(SEED, call & 0xFFFFFFFF, STREAM, n)


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


def _pieces_first(t, axis=1):
    """A three- (six-) piece device tensor with its piece axis moved to the front: [P, ...]."""
    return _np(t.movedim(axis, 0).contiguous())


def _c8_to_logical(t):
    """c8 S3 [E, P, C / 8, H, W, B, 8] -> pieces [P, E, C, H, W, B]."""
    E, P, CG, H, W, B, _ = t.shape
    return _np(t.permute(1, 0, 2, 6, 3, 4, 5).reshape(P, E, CG * 8, H, W, B).contiguous())


def _pack_w(w, tap_major):
    """[E, Cout, Cin, kh, kw] fp32 -> the bf16 GEMM's rows [E, Cout, Kp] (zero pad), (r, q, ci) columns when tap_major."""
    E, Cout = w.shape[:2]
    K = w[0, 0].numel()
    out = torch.zeros(E, Cout, (K + 7) & ~7, dtype=torch.bfloat16, device=w.device)
    out[:, :, :K] = (w.permute(0, 1, 3, 4, 2) if tap_major else w).reshape(E, Cout, K).to(torch.bfloat16)
    return out


def _chwn(x):
    """[E, B, C, H, W] -> batch-innermost [E, C, H, W, B]."""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _from_chwn(y):
    return y.permute(0, 4, 1, 2, 3).contiguous()


# =============================================================================================== families
# Each family: make(p) -> clean CPU fp32 operands; spots(p, t, place) -> [(operand, index), (operand, index of the pair's second)];
# pieces(p) -> operands whose Inf the reference reads as NaN; ref(p, t64, eps) -> {output: float64 array}; kinds(p, poison) ->
# {output: "exact" | "mask"}; launch(p, t) -> {output: array, a leading piece axis where the entry stores pieces}.

GEO = dict(B=8, Cin=16, Cout=16, H=8, W=8, k=3, pad=1, E=2)
# variant -> (ops entry, geometry overrides, three-piece operands)
CONV_VARIANTS = {
    "nchw": ("conv2d_forward", {}, False),
    "chwn": ("conv2d_chwn_forward", {}, False),
    "chwn-splitk": ("conv2d_chwn_forward", dict(Cin=512, H=1, W=1, k=1, pad=0), False),
    "chwn-pool": ("conv2d_chwn_forward", {}, False),
    "chwn-x3": ("conv2d_chwn_forward", {}, True),
    "chwn-s3": ("conv2d_chwn_forward", {}, True),
    "c8x3": ("conv2d_c8x3_forward", {}, True),
    "c8x3-pool": ("conv2d_c8x3_forward", dict(pad=0), True),
    "bf16": ("conv2d_chwn_bf16_forward", {}, False),
    "bf16-tm": ("conv2d_chwn_bf16_forward", {}, False),
    "bf16-smallk": ("conv2d_chwn_bf16_forward", dict(Cin=3), False),                   # the first-layer kernel, weights in registers
    # the window-resident fused pool: <= 32 channels and fewer than 70 pooled rows x image tiles
    "bf16-pool22": ("conv2d_chwn_bf16_forward", dict(Cin=3), False),
    "bf16-pool32": ("conv2d_chwn_bf16_forward", dict(Cin=3), False),
    "bf16-pool22-c8": ("conv2d_chwn_bf16_forward", dict(Cin=3), False),
    # the strip-form fused pool: more than 32 channels (two channel tiles per workgroup), or 18 draws x 4 pooled rows = 72 rows
    "bf16-strip22": ("conv2d_chwn_bf16_forward", dict(Cin=3, Cout=64), False),
    "bf16-strip32": ("conv2d_chwn_bf16_forward", dict(Cin=3, Cout=64), False),
    "bf16-strip22-c8": ("conv2d_chwn_bf16_forward", dict(Cin=3, Cout=64), False),
    "bf16-strip32-c8": ("conv2d_chwn_bf16_forward", dict(Cin=3, Cout=64), False),
    "bf16-strip22-nt1": ("conv2d_chwn_bf16_forward", dict(Cin=3, E=18), False),
    # channel-interleaved input (5 x 5 taps on 32 channels), channel-interleaved and batch-innermost output
    "bf16-c8": ("conv2d_chwn_bf16_forward", dict(Cin=32, k=5, pad=2), False),
    "bf16-c8in": ("conv2d_chwn_bf16_forward", dict(Cin=32, k=5, pad=2), False),
}
CONV_POOL = {"chwn-pool": (2, 2), "c8x3-pool": (2, 2), "bf16-pool22": (2, 2), "bf16-pool32": (3, 2), "bf16-pool22-c8": (2, 2),
             "bf16-strip22": (2, 2), "bf16-strip32": (3, 2), "bf16-strip22-c8": (2, 2), "bf16-strip32-c8": (3, 2), "bf16-strip22-nt1": (2, 2)}
# the kernel form ops.bf16_fwd_plan must report for each bf16 variant (tests/test_nonfinite_cpu.py)
BF16_FORMS = {"bf16": "general", "bf16-tm": "general", "bf16-smallk": "smallk", "bf16-pool22": "smallk-poolwin", "bf16-pool32": "smallk-poolwin",
              "bf16-pool22-c8": "smallk-poolwin", "bf16-strip22": "smallk-pool", "bf16-strip32": "smallk-pool", "bf16-strip22-c8": "smallk-pool",
              "bf16-strip32-c8": "smallk-pool", "bf16-strip22-nt1": "smallk-pool", "bf16-c8": "strip8", "bf16-c8in": "strip8"}
BF16_TM, BF16_XC8 = ("bf16-tm", "bf16-c8", "bf16-c8in"), ("bf16-c8", "bf16-c8in")
BF16_OC8 = ("bf16-pool22-c8", "bf16-strip22-c8", "bf16-strip32-c8", "bf16-c8")


def geo_of(p):
    g = dict(GEO)
    g.update(CONV_VARIANTS.get(p.get("variant"), LRT_VARIANTS.get(p.get("variant"), (None, {}, False)))[1])
    return g


class Conv:
    @staticmethod
    def make(p):
        g, gen = geo_of(p), _gen("conv", sorted(geo_of(p).items()))
        return dict(x=torch.randn(g["E"], g["B"], g["Cin"], g["H"], g["W"], generator=gen),
                    w=0.3 * torch.randn(g["E"], g["Cout"], g["Cin"], g["k"], g["k"], generator=gen),
                    b=torch.randn(g["E"], g["Cout"], generator=gen))

    @staticmethod
    def spots(p, t, place):
        g = geo_of(p)
        h, w, c = g["H"] // 2, g["W"] // 2, g["k"] // 2
        if place == "input":        # draw slab 1, image 3, one pixel of channel 5; the pair's second: channel 6 of the same pixel
            return [("x", (1, 3, 5 % g["Cin"], h, w)), ("x", (1, 3, 6 % g["Cin"], h, w))]
        if place == "weight":       # the centre tap
            return [("w", (1, 7, 5 % g["Cin"], c, c))]
        return [("b", (1, 7))]

    @staticmethod
    def pieces(p):
        return ("x", "w") if CONV_VARIANTS[p["variant"]][2] else ()

    @staticmethod
    def ref(p, t, eps):
        g = geo_of(p)
        ys = []
        for e in range(g["E"]):
            y = _act64(F.conv2d(t["x"][e], t["w"][e], t["b"][e], padding=g["pad"]), p["act"])
            if p["variant"] in CONV_POOL:
                y = F.max_pool2d(y, *CONV_POOL[p["variant"]])
            ys.append(y)
        return {"y": torch.stack(ys).numpy()}                                 # [E, B, Cout, Ho, Wo]

    @staticmethod
    def kinds(p, poison):
        return {"y": "mask" if CONV_VARIANTS[p["variant"]][2] else "exact"}

    @staticmethod
    def launch(p, t):
        from bbb_hip import ops
        g, v, act = geo_of(p), p["variant"], p["act"]
        x, w, b = (t[k].cuda() for k in ("x", "w", "b"))
        pad, kk = g["pad"], g["k"]
        if v == "nchw":
            return {"y": _np(ops.conv2d_forward(x, w, b, 1, pad, 1, act=act))}
        xc = _chwn(x)
        if v in ("chwn", "chwn-pool", "chwn-splitk"):
            with ops.use_config(split_k=(v == "chwn-splitk")):
                y = ops.conv2d_chwn_forward(xc, w, b, 1, pad, 1, act=act, bf16x3=False, pool=(v == "chwn-pool"))
            return {"y": _np(_from_chwn(y))}
        if v == "chwn-x3":
            with ops.use_config(gemm_mode="bf16x3", bf16x3_min_workgroups=1):
                y = ops.conv2d_chwn_forward(xc, w, b, 1, pad, 1, act=act)
            return {"y": _np(_from_chwn(y))}
        if v == "chwn-s3":
            y = ops.conv2d_chwn_forward(ops.s3_from_f32(xc), w, b, 1, pad, 1, act=act, x_s3=True, out_s3=True)     # [E, 3, Cout, Ho, Wo, B]
            return {"y": _np(y.permute(1, 0, 5, 2, 3, 4).contiguous())}
        if v in ("c8x3", "c8x3-pool"):
            y = ops.conv2d_c8x3_forward(ops.c8s3_from_f32(xc), ops.w_tap_major(w), b, kk, 1, pad, 1, act=act, pool=(v == "c8x3-pool"))
            return {"y": np.ascontiguousarray(_c8_to_logical(y).transpose(0, 1, 5, 2, 3, 4))}
        tm, oc8, xc8 = v in BF16_TM, v in BF16_OC8, v in BF16_XC8
        xb = xc.to(torch.bfloat16)
        y = ops.conv2d_chwn_bf16_forward(ops.to_c8(xb) if xc8 else xb, _pack_w(w, tm), b, (g["Cin"], kk, kk), 1, pad, 1, act=act,
                                         tap_major=tm, pool=CONV_POOL.get(v), out_c8=oc8)
        return {"y": _np(_from_chwn(ops.from_c8(y) if oc8 else y))}


LRT_VARIANTS = {
    "lrt-nchw": ("lrt_conv2d_forward", {}, False),
    "lrt-chwn": ("lrt_conv2d_chwn_forward", {}, False),
    "lrt-chwn-pool": ("lrt_conv2d_chwn_forward", {}, False),
    "lrt-c8x3": ("lrt_conv2d_c8x3_forward", {}, True),
    "lrt-bf16": ("lrt_conv2d_chwn_bf16_forward", {}, False),
}


class Lrt:
    @staticmethod
    def make(p):
        g, gen = geo_of(p), _gen("lrt", sorted(geo_of(p).items()))
        ws = (g["Cout"], g["Cin"], g["k"], g["k"])
        return dict(x=torch.randn(g["E"], g["B"], g["Cin"], g["H"], g["W"], generator=gen), w_mu=0.3 * torch.randn(ws, generator=gen),
                    w_var=(0.01 + 0.29 * torch.rand(ws, generator=gen)) ** 2, b_mu=torch.randn(g["Cout"], generator=gen),
                    b_var=(0.01 + 0.29 * torch.rand(g["Cout"], generator=gen)) ** 2)

    @staticmethod
    def spots(p, t, place):
        g = geo_of(p)
        h, w, c = g["H"] // 2, g["W"] // 2, g["k"] // 2
        if place == "input":
            return [("x", (1, 3, 5, h, w)), ("x", (1, 3, 6, h, w))]
        if place == "weight":
            return [("w_mu", (7, 5, c, c))]
        return [("b_mu", (7,))]

    @staticmethod
    def pieces(p):
        return ("x", "w_mu") if LRT_VARIANTS[p["variant"]][2] else ()

    @staticmethod
    def ref(p, t, eps):
        g = geo_of(p)
        out = {"y": [], "act_mu": [], "act_var": []}
        for e in range(g["E"]):
            mu = F.conv2d(t["x"][e], t["w_mu"], t["b_mu"], padding=g["pad"])
            var = float(np.float32(1e-16)) + F.conv2d(t["x"][e] * t["x"][e], t["w_var"], t["b_var"], padding=g["pad"])
            z = torch.from_numpy(np.asarray(eps(CALL0 + e, mu.numel()), np.float64)).reshape(mu.shape)     # canonical NCHW index
            y = _act64(mu + torch.sqrt(var) * z, p["act"])
            if p["variant"] == "lrt-chwn-pool":
                y = F.max_pool2d(y, 2, 2)
            for k, v in (("y", y), ("act_mu", mu), ("act_var", var)):
                out[k].append(v)
        keep = ("y",) if p["variant"] in ("lrt-chwn-pool", "lrt-c8x3") else ("y", "act_mu", "act_var")
        return {k: torch.stack(out[k]).numpy() for k in keep}

    @staticmethod
    def kinds(p, poison):
        if LRT_VARIANTS[p["variant"]][2]:
            return {"y": "mask"}
        k = {"y": "exact" if poison == NAN else "mask", "act_mu": "exact", "act_var": "exact"}
        return {"y": k["y"]} if p["variant"] == "lrt-chwn-pool" else k

    @staticmethod
    def launch(p, t):
        from bbb_hip import ops
        g, v, act = geo_of(p), p["variant"], p["act"]
        x, wm, wv, bm, bv = (t[k].cuda() for k in ("x", "w_mu", "w_var", "b_mu", "b_var"))
        pad, kk = g["pad"], g["k"]
        if v == "lrt-nchw":
            y, am, av = ops.lrt_conv2d_forward(x, wm, wv, bm, bv, SEED, CALL0, STREAM, 1, pad, 1, want_moments=True, act=act)
            return {"y": _np(y), "act_mu": _np(am), "act_var": _np(av)}
        xc = _chwn(x)
        if v == "lrt-chwn":
            y, am, av = ops.lrt_conv2d_chwn_forward(xc, wm, wv, bm, bv, SEED, CALL0, STREAM, 1, pad, 1, want_moments=True, act=act)
            return {k: _np(_from_chwn(a)) for k, a in (("y", y), ("act_mu", am), ("act_var", av))}
        if v == "lrt-chwn-pool":
            y, _, _ = ops.lrt_conv2d_chwn_forward(xc, wm, wv, bm, bv, SEED, CALL0, STREAM, 1, pad, 1, act=act, pool=True)
            return {"y": _np(_from_chwn(y))}
        if v == "lrt-c8x3":
            y = ops.lrt_conv2d_c8x3_forward(ops.c8s3_from_f32(xc, squares=True), ops.w_tap_major(wm[None])[0], ops.w_tap_major(wv[None])[0],
                                            bm, bv, kk, SEED, CALL0, STREAM, 1, pad, 1, act=act, out_f32=True)
            return {"y": _np(_from_chwn(y))}
        rm, rv = ops.lrt_weights_bf16([wm, wv])
        y, am, av = ops.lrt_conv2d_chwn_bf16_forward(xc.to(torch.bfloat16), rm, rv, bm, bv, (g["Cin"], kk, kk), SEED, CALL0, STREAM, 1, pad, 1,
                                                     want_moments=True, act=act, tap_major=ops.bf16_tap_major(tuple(wm.shape)))
        return {k: _np(_from_chwn(a)) for k, a in (("y", y), ("act_mu", am), ("act_var", av))}


SAMPLE_ENTRIES = ("lrt_sample_chwn", "lrt_sample_chwn_bf16", "lrt_sample_nchw")


class Sample:
    """E draws from one pair of moments.  chwn entries: moments [1, C, Ho, Wo, B]; nchw: [E, B, C, Ho, Wo], y = mu + sqrt(var) eps."""
    C, HW, B, E = 16, 4, 8, 2

    @staticmethod
    def make(p):
        gen = _gen("sample", p["entry"])
        shape = (Sample.E, Sample.B, Sample.C, Sample.HW, Sample.HW) if p["entry"] == "lrt_sample_nchw" else \
            (1, Sample.C, Sample.HW, Sample.HW, Sample.B)
        return dict(act_mu=torch.randn(shape, generator=gen), act_var=(0.01 + 0.29 * torch.rand(shape, generator=gen)) ** 2)

    @staticmethod
    def spots(p, t, place):
        idx = (1, 3, 5, 2, 3) if p["entry"] == "lrt_sample_nchw" else (0, 5, 2, 3, 3)
        return [("act_mu" if place == "input" else "act_var", idx)]

    @staticmethod
    def pieces(p):
        return ()

    @staticmethod
    def ref(p, t, eps):
        n = Sample.B * Sample.C * Sample.HW * Sample.HW
        ys = []
        for e in range(Sample.E):
            z = torch.from_numpy(np.asarray(eps(CALL0 + e, n), np.float64)).reshape(Sample.B, Sample.C, Sample.HW, Sample.HW)
            if p["entry"] == "lrt_sample_nchw":
                ys.append(t["act_mu"][e] + torch.sqrt(t["act_var"][e]) * z)
            else:
                z = z.permute(1, 2, 3, 0)
                ys.append(_act64(t["act_mu"][0] + torch.sqrt(t["act_var"][0]) * z, p["act"]))
        return {"y": torch.stack(ys).numpy()}

    @staticmethod
    def kinds(p, poison):
        return {"y": "exact"}

    @staticmethod
    def launch(p, t):
        from bbb_hip import ops
        mu, var = t["act_mu"].cuda(), t["act_var"].cuda()
        if p["entry"] == "lrt_sample_nchw":
            return {"y": _np(ops.lrt_sample_nchw(mu, var, SEED, CALL0, STREAM))}
        fn = ops.lrt_sample_chwn if p["entry"] == "lrt_sample_chwn" else ops.lrt_sample_chwn_bf16
        return {"y": _np(fn(mu, var, Sample.E, SEED, CALL0, STREAM, act=p["act"]))}


POOL_ENTRIES = {"maxpool_chwn": False, "maxpool_chwn_bf16": False, "maxpool_chwn_s3": True, "maxpool_c8s3": True,
                "avgpool_chwn": False, "avgpool_chwn_bf16": False}
POOL_TAPS = {(2, 2): {"first": (2, 2), "middle": (2, 3), "last": (3, 3)},          # window (1, 1) of MaxPool2d(2, 2): rows / columns 2..3
             (3, 2): {"first": (2, 2), "middle": (3, 3), "last": (4, 4)}}          # window (1, 1) of MaxPool2d(3, 2): rows / columns 2..4


class Pool:
    """x [E = 2, C = 16, 8, 8, B = 8]; the poison in image 3 of channel 5 of slab 1, at the first / a middle / the last tap of a
    window (torch keeps a NaN wherever it is seen: the order matters for a compare-and-select maximum).  The pair's second element
    is the next tap of the same window."""

    @staticmethod
    def make(p):
        return dict(x=torch.randn(2, 16, 8, 8, 8, generator=_gen("pool")))

    @staticmethod
    def spots(p, t, place):
        r, c = POOL_TAPS[p["win"]][place]
        r2, c2 = {"first": (r, c + 1), "middle": (r + 1, c - 1), "last": (r, c - 1)}[place]
        return [("x", (1, 5, r, c, 3)), ("x", (1, 5, r2, c2, 3))]

    @staticmethod
    def pieces(p):
        return ("x",) if POOL_ENTRIES[p["entry"]] else ()

    @staticmethod
    def ref(p, t, eps):
        x = t["x"]
        E, C, H, W, B = x.shape
        xn = x.permute(0, 4, 1, 2, 3).reshape(E * B, C, H, W)
        y = (F.avg_pool2d if p["entry"].startswith("avg") else F.max_pool2d)(xn, *p["win"])
        return {"y": y.reshape(E, B, C, *y.shape[2:]).permute(0, 2, 3, 4, 1).contiguous().numpy()}

    @staticmethod
    def kinds(p, poison):
        return {"y": "mask" if POOL_ENTRIES[p["entry"]] else "exact"}

    @staticmethod
    def launch(p, t):
        from bbb_hip import ops
        x, (k, s), e = t["x"].cuda(), p["win"], p["entry"]
        if e == "maxpool_chwn_s3":
            return {"y": _pieces_first(ops.maxpool_chwn_s3(ops.s3_from_f32(x), k, s))}
        if e == "maxpool_c8s3":
            return {"y": _c8_to_logical(ops.maxpool_c8s3(ops.c8s3_from_f32(x), k, s))}
        if e.endswith("bf16"):
            x = x.to(torch.bfloat16)
        return {"y": _np(getattr(ops, e)(x, k, s))}


CONVERT_ENTRIES = {"to_batch_innermost": False, "to_batch_innermost_bf16": False, "s3_from_f32": True, "s3_to_f32": True,
                   "c8s3_from_f32": True, "c8s3_to_f32": True, "s2d_c8s3": True}
S2D = dict(N=8, C=3, H=16, W=16, k=11, s=4, p=5)          # AlexNet's first layer in small (tests/infer_schedule_recorder.py "s2d")


class Convert:
    @staticmethod
    def make(p):
        e = p["entry"]
        if e == "s2d_c8s3":
            return dict(x=torch.randn(S2D["N"], S2D["C"], S2D["H"], S2D["W"], generator=_gen("s2d")))
        shape = (8, 16, 8, 8) if e.startswith("to_batch") else (2, 16, 8, 8, 8)
        return dict(x=torch.randn(shape, generator=_gen("convert", len(shape))))

    @staticmethod
    def spots(p, t, place):
        return [("x", (3, 1, 9, 6))] if p["entry"] == "s2d_c8s3" else [("x", (3, 5, 4, 3) if t["x"].dim() == 4 else (1, 5, 4, 3, 3))]

    @staticmethod
    def pieces(p):
        return ("x",) if CONVERT_ENTRIES[p["entry"]] else ()

    @staticmethod
    def ref(p, t, eps):
        x, e = t["x"], p["entry"]
        if e.startswith("to_batch"):
            return {"y": x.permute(1, 2, 3, 0).contiguous().numpy()}
        if e == "s2d_c8s3":
            # the definition of include/bbb_hip.h (bbb_s2d_c8s3): channel (c s + dy) s + dx of block position (i, j) is pixel
            # (s i + dy - p, s j + dx - p) of channel c, zero outside the map and in the padding channels
            from bbb_hip import ops
            N, C, H, W, s, pd = S2D["N"], S2D["C"], S2D["H"], S2D["W"], S2D["s"], S2D["p"]
            m, cp, hb, wb, _, _ = ops.s2d_geometry(C, S2D["k"], s, pd, 1, H, W)
            xpad = torch.zeros(N, C, s * hb + s + pd, s * wb + s + pd, dtype=x.dtype)
            xpad[:, :, pd:pd + H, pd:pd + W] = x
            want = torch.zeros(N, cp, hb, wb, dtype=x.dtype)
            for c in range(C):
                for dy in range(s):
                    for dx in range(s):
                        want[:, (c * s + dy) * s + dx] = xpad[:, c, dy:dy + s * hb:s, dx:dx + s * wb:s]
            return {"y": want.permute(1, 2, 3, 0)[None].contiguous().numpy()}        # [1, C', Hb, Wb, N]
        return {"y": x.numpy()}

    @staticmethod
    def kinds(p, poison):
        return {"y": "mask" if CONVERT_ENTRIES[p["entry"]] else "exact"}

    @staticmethod
    def launch(p, t):
        from bbb_hip import ops
        x, e = t["x"].cuda(), p["entry"]
        if e.startswith("to_batch"):
            return {"y": _np(getattr(ops, e)(x))}
        if e == "s3_from_f32":
            return {"y": _pieces_first(ops.s3_from_f32(x))}
        if e == "s3_to_f32":
            return {"y": _np(ops.s3_to_f32(ops.s3_from_f32(x)))}
        if e == "c8s3_from_f32":
            return {"y": _c8_to_logical(ops.c8s3_from_f32(x))}
        if e == "c8s3_to_f32":
            return {"y": _np(ops.c8s3_to_f32(ops.c8s3_from_f32(x)))}
        return {"y": _c8_to_logical(ops.s2d_c8s3(x, 1, S2D["k"], S2D["s"], S2D["p"]))}


TAIL_ENTRIES = ("mc_tail", "mc_tail_cb", "mc_tail_units", "mc_tail_groups", "mc_tail_share", "uncertainty", "uncertainty_normalized",
                "elbo_cb_autograd")
TAIL = dict(slabs=4, B=8, C=4)
TAIL_BLOCKS = {"mc_tail_units": [[0, 2], [1, 3]],          # slices = 2, unit_off = 0: unit u is batch slice u % 2
               "mc_tail_groups": [[0, 1], [2, 3]],         # groups = 2 x draws = 2
               "mc_tail_share": [[0], [1, 2], [3]]}        # steps = 3, draws = 2, first_off = 1: slab e = draw 1 + e of (step, draw)
ELBO = dict(kl=3.5, beta=0.1, train_size=64.0)


class Tail:
    """logits [slabs = 4, B = 8, C = 4] (rows); a NaN or +Inf logit in row (slab 1, image 3) makes every output of image 3 of that
    slab's block NaN, as torch's log_softmax does; every other image stays bitwise; a NaN image makes the loss NaN."""

    @staticmethod
    def make(p):
        t = dict(rows=2.0 * torch.randn(TAIL["slabs"], TAIL["B"], TAIL["C"], generator=_gen("tail")))
        if p["entry"] == "elbo_cb_autograd":
            t["target"] = torch.randint(0, TAIL["C"], (TAIL["B"],), generator=_gen("target")).double()
        return t

    @staticmethod
    def spots(p, t, place):
        return [("rows", (1, 3, 2))]

    @staticmethod
    def pieces(p):
        return ()

    @staticmethod
    def ref(p, t, eps):
        import tail_contract as TC
        rows, e = t["rows"].numpy(), p["entry"]
        with np.errstate(invalid="ignore", over="ignore"):
            if e.startswith("uncertainty"):
                return dict(zip(("pred", "epistemic", "aleatoric"), TC.uncertainty_ref(rows, e.endswith("normalized"))))
            mean_over = TAIL["slabs"] if e in ("mc_tail", "mc_tail_cb", "elbo_cb_autograd") else 0
            lse = TC.tail_ref(rows, TAIL_BLOCKS.get(e, [list(range(TAIL["slabs"]))]), mean_over)
            if e != "elbo_cb_autograd":
                return {"lse": lse}
            tg = t["target"].numpy().astype(np.int64)
            loss = -(lse[np.arange(TAIL["B"]), tg].sum() / TAIL["B"]) * ELBO["train_size"] + ELBO["beta"] * ELBO["kl"]
            return {"lse": lse, "loss": np.array(loss)}

    @staticmethod
    def kinds(p, poison):
        e = p["entry"]
        if e.startswith("uncertainty"):
            return {"pred": "exact", "epistemic": "exact", "aleatoric": "exact"}
        return {"lse": "exact", "loss": "exact"} if e == "elbo_cb_autograd" else {"lse": "exact"}

    @staticmethod
    def launch(p, t):
        from bbb_hip import ops
        rows, e = t["rows"].cuda(), p["entry"]
        n = TAIL["slabs"]
        if e.startswith("uncertainty"):
            return dict(zip(("pred", "epistemic", "aleatoric"), (_np(o) for o in ops.uncertainty(rows, normalized=e.endswith("normalized")))))
        if e == "mc_tail":
            return {"lse": _np(ops.mc_tail(rows, mean_over=n))}
        cb = rows.permute(0, 2, 1).contiguous()
        if e == "mc_tail_cb":
            return {"lse": _np(ops.mc_tail_cb(cb, mean_over=n))}
        if e == "mc_tail_units":
            return {"lse": _np(ops.mc_tail_units(cb, 2, 0))}
        if e == "mc_tail_groups":
            return {"lse": _np(ops.mc_tail_groups(cb, 2, 2))}
        if e == "mc_tail_share":
            return {"lse": _np(ops.mc_tail_share(cb, 3, 2, 1))}
        with torch.no_grad():
            loss, lse = ops.elbo_cb_autograd(cb, torch.tensor(ELBO["kl"], device="cuda"), t["target"].long().cuda(), ELBO["beta"],
                                             ELBO["train_size"], mean_over=n)
        return {"lse": _np(lse), "loss": _np(loss)}


PARAM_ENTRIES = ("reparam_kl_forward", "sample_weights")
PRIOR_MU, PRIOR_SIGMA, PARAM_DRAWS, PARAM_STREAMS = 0.0, 0.1, 2, (0, 1)


class Param:
    """The fused reparam + KL pass on a conv weight [16, 16, 3, 3] and its bias [16]: a NaN in one mu or one rho is NaN in every
    draw of that element, every other element is bitwise, the KL scalar is non-finite."""

    @staticmethod
    def make(p):
        gen = _gen("param")
        return dict(mu0=0.1 * torch.randn(16, 16, 3, 3, generator=gen), rho0=-5 + 0.1 * torch.randn(16, 16, 3, 3, generator=gen),
                    mu1=0.1 * torch.randn(16, generator=gen), rho1=-5 + 0.1 * torch.randn(16, generator=gen))

    @staticmethod
    def spots(p, t, place):
        return [(place + "0", (7, 5, 1, 1))]

    @staticmethod
    def pieces(p):
        return ()

    @staticmethod
    def ref(p, t, eps):
        out, kl = {}, 0.0
        for i in (0, 1):
            mu, sigma = t["mu%d" % i], F.softplus(t["rho%d" % i])
            ws = []
            for e in range(PARAM_DRAWS):
                z = O.normal_eps(SEED, (CALL0 + e) & 0xFFFFFFFF, PARAM_STREAMS[i], mu.numel())
                ws.append(mu + sigma * torch.from_numpy(np.asarray(z, np.float64)).reshape(mu.shape))
            out["w%d" % i] = torch.stack(ws).numpy()
            kl = kl + (math.log(PRIOR_SIGMA) - torch.log(sigma) - 0.5 + (sigma ** 2 + (mu - PRIOR_MU) ** 2) / (2 * PRIOR_SIGMA ** 2)).sum()
        out["kl"] = np.array(float(kl))
        return out

    @staticmethod
    def kinds(p, poison):
        return {"w0": "exact", "w1": "exact", "kl": "mask"}

    @staticmethod
    def launch(p, t):
        from bbb_hip import ops
        mus, rhos = [t["mu0"].cuda(), t["mu1"].cuda()], [t["rho0"].cuda(), t["rho1"].cuda()]
        if p["entry"] == "reparam_kl_forward":
            ws, _, kl = ops.reparam_kl_forward(mus, rhos, PRIOR_MU, PRIOR_SIGMA, list(PARAM_STREAMS), SEED, CALL0, PARAM_DRAWS)
        else:
            with torch.no_grad():
                kl, ws = ops.sample_weights(mus, rhos, PRIOR_MU, PRIOR_SIGMA, list(PARAM_STREAMS), SEED, CALL0, PARAM_DRAWS)
        return {"w0": _np(ws[0]), "w1": _np(ws[1]), "kl": _np(kl)}


MODELS = (("std", "bbb"), ("std", "lrt"), ("alone", "bbb"), ("quirk", "bbb"))
MODEL_IMAGE, MODEL_DRAWS = 3, 2


@functools.lru_cache(maxsize=None)
def _net(model, kind):
    import infer_schedule_recorder as R
    from bbb_hip import rng
    net = R.build(model, kind)
    rng.assign_stream_ids(net)
    return net


def rows_per_image(model):
    """Output rows of one image: 4 behind the flatten of "quirk", which cuts each image's 256 features into rows of 64."""
    return 4 if model == "quirk" else 1


class Model:
    """ensemble.mc_forward on the models of tests/infer_schedule_recorder.py: one NaN pixel in image 3 makes that image's
    log_outputs rows NaN in every class (through every draw); all other images are bitwise the clean run.  The reference states
    exactly that: the pixel reaches every feature row of its image (a 3 x 3 layer spreads it to every channel of a neighbourhood that
    meets every pooling window row the flatten cuts out), and no other image."""

    @staticmethod
    def make(p):
        import infer_schedule_recorder as R
        cin, side, _ = R.MODELS[p["model"]]
        return dict(x=torch.rand(p["B"], cin, side, side, generator=_gen("model-x")))

    @staticmethod
    def spots(p, t, place):
        return [("x", (MODEL_IMAGE, 1, 4, 4))]

    @staticmethod
    def pieces(p):
        return ()

    @staticmethod
    def ref(p, t, eps):
        import infer_schedule_recorder as R
        r = rows_per_image(p["model"])
        lo = np.zeros((p["B"] * r, R.CLASSES))
        bad = ~np.isfinite(t["x"].numpy()).reshape(p["B"], -1).all(axis=1)
        lo[np.repeat(bad, r)] = np.nan
        out = {"log_outputs": lo}
        if p.get("train"):
            out["loss"] = np.array(np.nan if bad.any() else 0.0)
        return out

    @staticmethod
    def kinds(p, poison):
        return {"log_outputs": "exact", "loss": "exact"} if p.get("train") else {"log_outputs": "exact"}

    @staticmethod
    def launch(p, t):
        import copy
        from bbb_hip import ensemble, ops, rng, train
        x = t["x"].cuda()
        _net(p["model"], p["kind"])                     # (built first: building seeds torch, which un-pins the noise stream)
        rng.manual_seed(SEED, CALL0)
        try:
            if p.get("train"):
                net = copy.deepcopy(_net(p["model"], p["kind"])).cuda()
                rng.assign_stream_ids(net)
                target = torch.randint(0, 4, (p["B"],), generator=_gen("model-target")).cuda()
                loss, lo, _ = train.train_step(net, train.FusedAdam(net.parameters(), lr=1e-3), x, target, MODEL_DRAWS, 1e-7, 64.0, graph=False)
                return {"log_outputs": _np(lo), "loss": _np(loss)}
            net = _net(p["model"], p["kind"]).cuda()
            cfg = dict(bf16_lrt=True) if (p["kind"], p["precision"]) == ("lrt", "bf16") else {}
            with torch.no_grad(), ops.use_config(**cfg):
                lo, _ = ensemble.mc_forward(net, x, MODEL_DRAWS, precision=p["precision"])
            return {"log_outputs": _np(lo)}
        finally:
            rng.use_device_generator()


FAMILIES = {"conv": Conv, "lrt": Lrt, "sample": Sample, "pool": Pool, "convert": Convert, "tail": Tail, "param": Param, "model": Model}

# every forward entry the contract covers -> the family that holds its cases (tests/test_nonfinite_cpu.py: each has a case for every
# poison it can take)
ENTRIES = {**{v[0]: "conv" for v in CONV_VARIANTS.values()}, **{v[0]: "lrt" for v in LRT_VARIANTS.values()},
           **{e: "sample" for e in SAMPLE_ENTRIES}, **{e: "pool" for e in POOL_ENTRIES}, **{e: "convert" for e in CONVERT_ENTRIES},
           **{e: "tail" for e in TAIL_ENTRIES if e != "uncertainty_normalized"}, **{e: "param" for e in PARAM_ENTRIES},
           "mc_forward": "model", "train_step": "model"}


def _poisons(place, act, elementwise=False):
    """The poisons a placement can take without the case going vacuous: a -Inf bias (or a -Inf the entry maps element by element)
    behind relu / softplus is a finite 0 everywhere."""
    if place == "input" and not elementwise:
        return (NAN, PINF, NINF, PAIR)
    if place == "weight":
        return (NAN, PINF, NINF)
    return (NAN, PINF, NINF) if act is None else (NAN, PINF)


def _build():
    cs = []

    def add(entry, family, p, place, poison):
        name = "-".join([family] + [str(v) for k, v in sorted(p.items()) if k != "act" and v is not None]).replace(" ", "")
        name += "-%s-%s-%s" % (p.get("act") or "none", place, poison) if "act" in p else "-%s-%s" % (place, poison)
        cs.append(Case(name, entry, family, tuple(sorted(p.items(), key=lambda kv: kv[0])), place, poison))

    for v, (entry, _, _) in CONV_VARIANTS.items():
        for act in ACTS:
            for place in ("input", "weight", "bias"):
                for poison in _poisons(place, act):
                    add(entry, "conv", dict(variant=v, act=act), place, poison)
    for v, (entry, _, _) in LRT_VARIANTS.items():
        for act in ACTS:
            for place in ("input", "weight", "bias"):
                for poison in _poisons(place, act):
                    add(entry, "lrt", dict(variant=v, act=act), place, poison)
    for entry in SAMPLE_ENTRIES:
        for act in (ACTS if entry != "lrt_sample_nchw" else (None,)):
            for poison in _poisons("input", act, elementwise=True):
                add(entry, "sample", dict(entry=entry, act=act), "input", poison)
            add(entry, "sample", dict(entry=entry, act=act), "var", NAN)
    for entry in POOL_ENTRIES:
        for win in POOL_TAPS:
            for tap in ("first", "middle", "last"):
                # max pools: a -Inf never wins a window; the pair is +Inf there and NaN in an average
                for poison in ((NAN, PINF, NINF, PAIR) if entry.startswith("avg") else (NAN, PINF, PAIR)):
                    add(entry, "pool", dict(entry=entry, win=win), tap, poison)
    for entry in CONVERT_ENTRIES:
        for poison in (NAN, PINF, NINF):
            add(entry, "convert", dict(entry=entry), "input", poison)
    for entry in TAIL_ENTRIES:
        for poison in (NAN, PINF):
            add("uncertainty" if entry.startswith("uncertainty") else entry, "tail", dict(entry=entry), "input", poison)
    for entry in PARAM_ENTRIES:
        for place in ("mu", "rho"):
            add(entry, "param", dict(entry=entry), place, NAN)
    for model, kind in MODELS:
        for precision in ("fp32", "bf16x3", "bf16"):
            for B in (8, 6):
                # bf16 storage takes batches of a multiple of 8 and no flatten that cuts an image into rows: the entry refuses
                if precision == "bf16" and (B % 8 or model == "quirk"):
                    continue
                add("mc_forward", "model", dict(model=model, kind=kind, precision=precision, B=B), "input", NAN)
    add("train_step", "model", dict(model="std", kind="bbb", precision="fp32", B=8, train=True), "input", NAN)
    assert len({c.id for c in cs}) == len(cs)
    return tuple(cs)


CASES = _build()
BY_ID = {c.id: c for c in CASES}


# =============================================================================================== operands, reference, check
@functools.lru_cache(maxsize=None)
def _clean(group):
    family, p = group
    return FAMILIES[family].make(dict(p))


def operands(case, poisoned=True):
    """The case's CPU fp32 operands: clean, or with the poison written."""
    t = {k: v.clone() for k, v in _clean(case.group).items()}
    if poisoned:
        spots = FAMILIES[case.family].spots(case.params, t, case.place)
        if case.poison == PAIR:
            t[spots[0][0]][spots[0][1]] = VALUE[PINF]
            t[spots[1][0]][spots[1][1]] = VALUE[NINF]
        else:
            t[spots[0][0]][spots[0][1]] = VALUE[case.poison]
    return t


def reference(case, eps=default_eps, poisoned=True, as_nan=False):
    """{output: float64 array}: the entry in float64 on the poisoned (or the clean) operands (three-piece operands: Inf read as NaN;
    as_nan: every poisoned element read as NaN, whatever the poison)."""
    fam = FAMILIES[case.family]
    t = {k: v.to(F64) for k, v in operands(case, poisoned).items()}
    if as_nan:
        t = {k: torch.where(torch.isfinite(v), v, torch.full_like(v, float("nan"))) for k, v in t.items()}
    for k in fam.pieces(case.params):
        t[k] = torch.where(torch.isinf(t[k]), torch.full_like(t[k], float("nan")), t[k])
    return fam.ref(case.params, t, eps)


def reach(case, eps=default_eps):
    """{output: bool array}: the elements that depend on a poisoned operand element."""
    return {k: np.isnan(v) for k, v in reference(case, eps, as_nan=True).items()}


def kinds(case):
    return FAMILIES[case.family].kinds(case.params, case.poison)


def launch(case, poisoned=True):
    return FAMILIES[case.family].launch(case.params, operands(case, poisoned))


def _nonfinite(got, ref_shape):
    """Non-finite mask of a device output in the reference's shape: any piece, where the entry stores pieces."""
    bad = ~np.isfinite(np.asarray(got, np.float64))
    return bad.any(axis=0) if bad.ndim == len(ref_shape) + 1 else bad


def check(case, ref, reached, clean, got):
    """The two assertions on the device's outputs `got` (poisoned operands) and `clean` (clean operands), given the float64
    reference and reach(case); returns the list of failures (empty: the case holds)."""
    fails = []
    for name, kind in kinds(case).items():
        r, g, c = np.asarray(ref[name]), np.asarray(got[name]), np.asarray(clean[name])
        pieces = g.ndim == r.ndim + 1
        if (g.shape[1:] if pieces else g.shape) != r.shape or c.shape != g.shape:
            fails.append("%s: shape %s (clean %s) against the reference's %s" % (name, g.shape, c.shape, r.shape))
            continue
        rc = classes(r)
        if kind == "exact" and not pieces:
            bad = classes(g) != rc
            what = "class"
        else:
            bad = _nonfinite(g, r.shape) != (rc != FINITE)
            what = "non-finite mask"
        if bad.any():
            i = np.unravel_index(np.argmax(bad), bad.shape)
            fails.append("%s: %s differs at %d elements, first at %s: device %s, reference %s" % (
                name, what, int(bad.sum()), i, g[(slice(None),) + i] if pieces else g[i], r[i]))
        same = ~np.asarray(reached[name])
        moved = np.broadcast_to(same, g.shape) & ~(g == c)
        # a finite value the poison MADE is exact where it is a zero (relu / softplus of -Inf, a window of them): the device's too
        # (not behind a fused pool: there a reached zero is the maximum over the window's other taps as well, arithmetic results
        # whose sign at a bf16 or fp32 rounding of zero is not the float64 reference's)
        pooled = case.params.get("variant") in CONV_POOL or case.params.get("variant") == "lrt-chwn-pool"
        zero = np.broadcast_to(~same & (r == 0), g.shape) & ~(g == 0)
        if zero.any() and not pooled:
            i = np.unravel_index(np.argmax(zero), zero.shape)
            fails.append("%s: %d elements the poison turns into an exact zero are not zero, first at %s: %s" % (name, int(zero.sum()), i, g[i]))
        if moved.any():
            i = np.unravel_index(np.argmax(moved), moved.shape)
            fails.append("%s: %d elements the poison does not reach differ from the clean launch, first at %s: %s against %s" % (
                name, int(moved.sum()), i, g[i], c[i]))
    return fails
