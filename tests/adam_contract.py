"""The contract of the multi-tensor Adam step (bbb_adam_step, csrc/adam.hip; launch plan csrc/adam_plan.h), shared by
tests/test_gpu_adam_sweep.py (device) and tests/test_adam_sweep_cpu.py (the contract held against itself, no device).

One launch maps (p, g, m, v) to (p', m', v').  Four tiers:

values      against float64.  The reference takes the launch's seven fp32 scalars -- step_size = lr / (1 - beta1^t), sqrt(1 - beta2^t),
            beta1, beta2, 1 - beta1, 1 - beta2, eps, each formed in double and rounded to fp32 ONCE (scalars()) -- and does everything
            else in float64:  m' = m + (g - m) omb1,  v' = v beta2 + omb2 g g.  p' is held to p - step_size (m' / (sqrt(v') / sqrt_bc2 +
            eps)) evaluated in float64 on the launch's OWN m' and v' (a chain of trust: m' and v' have their own bounds, and the
            cancellation inside m' does not leak into the parameter's).  Per element |out - ref| <= c (2^-23 M + 2^-149) with M the sum
            of the absolute terms: M_m = |m| + (|g| + |m|) omb1, M_v = v', M_p = |p| + |update|.  c is NOT taken from the kernel: it is
            4 x the worst ratio of the fp32 reference (torch.optim.Adam(foreach=False) on CPU, one step from loaded state) against the
            same float64 reference over VALUE_CASES, rounded up to a power of two, at most 64 -- test_adam_sweep_cpu.py measures it and
            holds C to it.  Multi-step cases feed each launch the previous launch's outputs, so no error accumulates inside a bound.
geometry    bit for bit.  The update is element-wise, so an element's result may not depend on where it sits: segment count, chunk
            position, alignment, vector or scalar path.  The bit reference is ONE aligned single-segment launch over the same values.
            Every array lives in a flat buffer with GUARD sentinels before, between and behind the segments; after a launch all four
            buffers are compared whole: results at the launched segments, everything else (sentinels, segments not launched, all of
            grad) bitwise as before.
device step bit for bit against the host path (test_gpu_adam_sweep.py), and the scalars themselves bitwise against scalars().
classes     non-finite and out-of-range operands: every output element is finite / NaN / +Inf / -Inf exactly where the CPU fp32
            torch.optim.Adam result on the same operands is, and every element the poison does not reach is bitwise the clean launch's.
"""
import ctypes
import math
import zlib
from collections import namedtuple

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -23                    # one fp32 ulp of 1
TINY = 2.0 ** -149                # the spacing of fp32 below 2^-126
EINVAL, EALIGN, ESHAPE = -1, -2, -3
MAX_SEGMENTS = 16
CHUNK = 1024                      # elements of a block
GUARD = 8                         # sentinel elements before, between and behind the segments of a buffer
SENTINEL = 0x7FA55AA5             # a NaN with a payload no arithmetic produces
KINDS = ("param", "grad", "exp_avg", "exp_avg_sq")

Hyper = namedtuple("Hyper", "lr beta1 beta2 eps")
Scalars = namedtuple("Scalars", "step_size sqrt_bc2 beta1 beta2 omb1 omb2 eps")
DEFAULT = Hyper(1e-3, 0.9, 0.999, 1e-8)

# c of the value bounds: 4 x the fp32 reference's worst ratio over VALUE_CASES, rounded up to a power of two
# (test_adam_sweep_cpu.py::test_constants_follow_from_the_fp32_reference measures 0.84 / 0.98 / 1.35 for m / v / p; profiles/adam_sweep_notes.md)
C = {"m": 4, "v": 4, "p": 8}
DEVICE_FACTOR, C_MAX = 4, 64


def constant_from(ratio):
    """The rule: 4 x the reference's ratio, rounded up to a power of two, never above 64."""
    assert 0.0 < ratio and DEVICE_FACTOR * ratio <= C_MAX, ratio
    return 2 ** max(0, math.ceil(math.log2(DEVICE_FACTOR * ratio)))


# ---- scalars ----

def scalars(h, t, lr=None):
    """The seven fp32 scalars of a host-path launch at step t: formed in double, rounded once."""
    lr = h.lr if lr is None else lr
    bc1 = 1.0 - math.pow(h.beta1, float(t))
    bc2 = 1.0 - math.pow(h.beta2, float(t))
    with np.errstate(over="ignore"):
        return Scalars(F32(lr / bc1), F32(math.sqrt(bc2)), F32(h.beta1), F32(h.beta2), F32(1.0 - h.beta1), F32(1.0 - h.beta2), F32(h.eps))


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def check_scalars(got, h, t, lr=None):
    """got: the seven scalars a plan reports (a mapping or a Scalars) -- bitwise those of scalars()."""
    want = scalars(h, t, lr)
    for k in Scalars._fields:
        g = got[k] if isinstance(got, dict) else getattr(got, k)
        assert bits(F32(g)) == bits(getattr(want, k)), (k, float(g), float(getattr(want, k)), h, t)


# ---- float64 reference, bounds ----

def moments64(g, m, v, sc):
    g, m, v = (np.asarray(a, dtype=F64) for a in (g, m, v))
    return m + (g - m) * F64(sc.omb1), v * F64(sc.beta2) + F64(sc.omb2) * g * g


def param64(p, m1, v1, sc):
    """(p', update) from the launch's own m' and v'."""
    p, m1, v1 = (np.asarray(a, dtype=F64) for a in (p, m1, v1))
    upd = F64(sc.step_size) * (m1 / (np.sqrt(v1) / F64(sc.sqrt_bc2) + F64(sc.eps)))
    return p - upd, upd


def step64(p, g, m, v, h, t):
    """One step in float64 with UNROUNDED scalars: what torch.optim.Adam computes on float64 tensors."""
    bc1, bc2 = 1.0 - h.beta1 ** t, 1.0 - h.beta2 ** t
    m1 = m + (g - m) * (1.0 - h.beta1)
    v1 = v * h.beta2 + (1.0 - h.beta2) * g * g
    return p - (h.lr / bc1) * (m1 / (np.sqrt(v1) / math.sqrt(bc2) + h.eps)), m1, v1


def value_ratios(before, after, sc):
    """{m, v, p: worst |out - float64| / (2^-23 M + 2^-149)} of one launch; before = (p, g, m, v), after = (p', m', v').  Every operand,
    every output and every reference value must be finite: this tier has no holes."""
    p, g, m, v = (np.asarray(a, dtype=F64) for a in before)
    p1, m1, v1 = (np.asarray(a, dtype=F64) for a in after)
    for a in (p, g, m, v, p1, m1, v1):
        assert np.isfinite(a).all(), "non-finite value in the value tier"
    mr, vr = moments64(g, m, v, sc)
    pr, upd = param64(p, m1, v1, sc)
    assert np.isfinite(pr).all() and (vr >= 0).all()
    scale = {"m": np.abs(m) + (np.abs(g) + np.abs(m)) * F64(sc.omb1), "v": vr, "p": np.abs(p) + np.abs(upd)}
    err = {"m": np.abs(m1 - mr), "v": np.abs(v1 - vr), "p": np.abs(p1 - pr)}
    return {k: float((err[k] / (U * scale[k] + TINY)).max()) for k in ("m", "v", "p")}


def check_values(before, after, sc, name=""):
    r = value_ratios(before, after, sc)
    for k, x in r.items():
        assert x <= C[k], (name, k, x, C[k])
    return r


def torch_adam(before, h, t, dtype=None):
    """torch.optim.Adam(foreach=False) on CPU: one step from loaded state, at step t.  Returns (p', m', v') as numpy."""
    import torch
    dtype = dtype or torch.float32
    p, g, m, v = (torch.from_numpy(np.array(a)).to(dtype) for a in before)
    opt = torch.optim.Adam([p], lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m, "exp_avg_sq": v}
    p.grad = g
    opt.step()
    return p.numpy(), m.numpy(), v.numpy()


def model32(before, sc, fault=None):
    """The update in fp32, operation by operation as the kernel's source states it (numpy: no contraction) -- the stand-in for a
    device in test_adam_sweep_cpu.py, with the arithmetic faults a checker must catch."""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in before)
    with np.errstate(all="ignore"):
        m1 = m + (g - m) * sc.omb1
        v1 = v * sc.beta2 + sc.omb2 * g * g
        root = np.sqrt(v1 + sc.eps) if fault == "eps_in_root" else np.sqrt(v1)
        denom = root / sc.sqrt_bc2 + (F32(0) if fault == "eps_in_root" else sc.eps)
        p1 = p - sc.step_size * (m1 / denom)
        if fault == "nan_to_finite":
            p1 = np.where(np.isnan(p1), p, p1)
    return p1.astype(F32), m1.astype(F32), v1.astype(F32)


def faulty_scalars(h, t, fault):
    """Scalars with one planted fault."""
    sc = scalars(h, t)
    if fault == "omb2_in_fp32":
        return sc._replace(omb2=F32(1.0) - F32(h.beta2))
    if fault == "no_bc2":
        return sc._replace(sqrt_bc2=F32(1.0))
    if fault == "bc1_at_t-1":
        return sc._replace(step_size=F32(h.lr / (1.0 - math.pow(h.beta1, float(t - 1)))))
    assert fault == "lr_through_float"
    return sc._replace(step_size=F32(float(F32(h.lr)) / (1.0 - math.pow(h.beta1, float(t)))))


# ---- value cases ----

T_VALUES = (1, 2, 7, 1000, 100000, 2 ** 24 - 1)
G_SCALES = (1e-12, 1e-6, 1e-3, 1.0, 1e3, 1e6)
HYPERS = {"default": DEFAULT, "lr3e-3": Hyper(3e-3, 0.9, 0.999, 1e-8), "beta1=0": Hyper(1e-3, 0.0, 0.999, 1e-8),
          "beta2=0": Hyper(1e-3, 0.9, 0.0, 1e-8), "loose": Hyper(1e-1, 0.5, 0.9, 1e-3), "eps=0": Hyper(1e-3, 0.9, 0.999, 0.0)}
VALUE_N = 1537                    # two chunks, the second ragged, the last thread's quad a single element
ValueCase = namedtuple("ValueCase", "name hyper t gscale moments")       # moments: "zero" | "match"

VALUE_CASES = [ValueCase("%s-t%d-g%g-%s" % (hn, t, gs, mo), hn, t, gs, mo)
               for hn in HYPERS for t in T_VALUES for gs in G_SCALES for mo in (("zero", "match") if t == 1 else ("match",))]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def draw(name, n, gscale=1e-2, moments="match", pscale=1.0):
    """(p, g, m, v) fp32: p ~ pscale N(0, 1); g = gscale z with |z| >= 1e-3 (every g != 0, and g^2 (1 - beta2) stays a normal fp32 at the
    smallest scale); moments zero, or at the gradient's scale: m ~ gscale N(0, 1) / 2, v = (gscale (0.3 + |N(0, 1)|))^2."""
    r = _rng(name)
    z = r.standard_normal(n)
    z = np.where(z < 0, -1.0, 1.0) * np.maximum(np.abs(z), 1e-3)
    p, g = (pscale * r.standard_normal(n)).astype(F32), (gscale * z).astype(F32)
    if moments == "zero":
        return p, g, np.zeros(n, F32), np.zeros(n, F32)
    m = (0.5 * gscale * r.standard_normal(n)).astype(F32)
    v = ((gscale * (0.3 + np.abs(r.standard_normal(n)))) ** 2).astype(F32)
    assert (g != 0).all() and (v > 0).all() and np.isfinite(v).all()
    return p, g, m, v


def values_of(case):
    return draw(case.name, VALUE_N, case.gscale, case.moments)


# the six chained steps of test_gpu_train.py::test_fused_adam_matches_torch_adam: gradients 10^(it - 3) N(0, 1), lr 3e-3, from zero moments
CHAIN_HYPER, CHAIN_STEPS = HYPERS["lr3e-3"], 6
CHAIN_SIZES = (1025, 1, 330)


def chain_grad(it, n):
    return (_rng("chain%d" % it).standard_normal(n) * 10.0 ** (it - 3)).astype(F32)


# ---- buffers with sentinels ----

class Layout:
    """Four flat fp32 buffers (param, grad, exp_avg, exp_avg_sq) holding the segments of a case: segment s of kind k sits at
    start[k][s], `off` elements (0..3) past a 16-byte boundary, with at least GUARD sentinels on either side.  The buffers' own starts
    are 16-byte aligned on the device (an allocation is)."""

    def __init__(self, segments):
        """segments: a list of ((p, g, m, v), (off_p, off_g, off_m, off_v))."""
        self.n = [len(vals[0]) for vals, _ in segments]
        self.off = [tuple(off) for _, off in segments]
        self.start = [[] for _ in KINDS]
        size = []
        for k in range(4):
            pos = GUARD
            for (vals, off), n in zip(segments, self.n):
                assert len(vals[k]) == n and 0 <= off[k] < 4 and pos % 4 == 0
                self.start[k].append(pos + off[k])
                pos = (pos + off[k] + n + GUARD + 3) // 4 * 4
            size.append(pos)
        self.host = []
        for k in range(4):
            buf = np.full(size[k], SENTINEL, dtype=np.uint32)
            for s, (vals, _) in enumerate(segments):
                buf[self.start[k][s]:self.start[k][s] + self.n[s]] = bits(vals[k])
            self.host.append(buf.view(F32))

    def seg(self, bufs, k, s):
        return bufs[k][self.start[k][s]:self.start[k][s] + self.n[s]]

    def values(self, which=None, bufs=None):
        """(p, g, m, v) of the segments `which` (default: all), concatenated in that order."""
        bufs = self.host if bufs is None else bufs
        which = range(len(self.n)) if which is None else which
        return tuple(np.concatenate([self.seg(bufs, k, s) for s in which]) for k in range(4))

    def vec_capable(self, s):
        return all(o == 0 for o in self.off[s]) and self.n[s] >= 4

    def plan_segments(self, which=None, base=4096 * 16):
        """Dicts of AdamSegment fields for ops.adam_plan: the alignment of the device addresses, on made-up aligned bases."""
        which = range(len(self.n)) if which is None else which
        return [dict(n=self.n[s], **{KINDS[k]: base * (k + 1) + 4 * self.start[k][s] for k in range(4)}) for s in which]

    def expected(self, which, result, before=None):
        """The four buffers a correct launch of the segments `which` leaves: `result` = (p', m', v') of their concatenated values (the
        bit reference) at the launched segments, everything else as before."""
        out = [np.array(b) for b in (self.host if before is None else before)]
        at = 0
        for s in which:
            for k, r in ((0, result[0]), (2, result[1]), (3, result[2])):
                self.seg(out, k, s)[:] = bits(r[at:at + self.n[s]]).view(F32)
            at += self.n[s]
        assert at == len(result[0])
        return out

    def where(self, k, i):
        for s, (st, n) in enumerate(zip(self.start[k], self.n)):
            if st <= i < st + n:
                return "element %d of segment %d (n = %d)" % (i - st, s, n)
            if i < st:
                return "sentinel %d before segment %d" % (st - i, s)
        return "sentinel %d behind the last segment" % (i - self.start[k][-1] - self.n[-1] + 1)


def check_geometry(layout, after, which, result, before=None, name=""):
    """All four buffers after a launch, bit for bit: the bit reference at the launched segments; sentinels, segments not launched and
    all of grad as before."""
    check_buffers(layout, after, layout.expected(which, result, before), name)


def check_buffers(layout, after, want, name=""):
    """The four buffers against the four expected ones, bit for bit, naming the first difference."""
    for k in range(4):
        got, exp = bits(after[k]), bits(want[k])
        assert got.shape == exp.shape
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, "%s: %s differs at %s (%d elements in all): got %08x, want %08x" % (
            name, KINDS[k], layout.where(k, int(bad[0])), bad.size, got[bad[0]], exp[bad[0]])


def model_launch(layout, which, sc, fault=None, before=None):
    """A launch on host buffers by model32 (test_adam_sweep_cpu.py): the four buffers afterwards.  Geometry faults: "stale_boundary"
    leaves the last element of the first launched segment as it was, "past_n" writes one element behind it, "writes_grad" stores m'
    over the first gradient."""
    before = layout.host if before is None else before
    out = [np.array(b) for b in before]
    for s in which:
        res = model32(tuple(layout.seg(before, k, s) for k in range(4)), sc, fault)
        for k, r in ((0, res[0]), (2, res[1]), (3, res[2])):
            layout.seg(out, k, s)[:] = r
    s0 = which[0]
    if fault == "stale_boundary":
        layout.seg(out, 2, s0)[-1:] = layout.seg(before, 2, s0)[-1:]
    elif fault == "past_n":
        out[3][layout.start[3][s0] + layout.n[s0]] = layout.seg(out, 3, s0)[-1]
    elif fault == "writes_grad":
        layout.seg(out, 1, s0)[:1] = layout.seg(out, 2, s0)[:1]
    return out


# ---- geometry cases ----

ALIGNED = (0, 0, 0, 0)
SINGLE_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4099)
# 16 segments: n = 1, exact multiples of a chunk, ragged sizes; last chunks of 1, 2 and 3 elements (1025, 2050, 1027)
SIXTEEN_N = (1, 1024, 1025, 7, 2048, 2050, 1, 1027, 1024, 3, 333, 1023, 2, 1024, 5, 1)
SIXTEEN_TAILS = {1: 2, 2: 5, 3: 7}          # elements of the last chunk: the segment that has it
GEOMETRY_T = 7

GeoCase = namedtuple("GeoCase", "name sizes offs launched")      # launched: None = every segment


def _geo_cases():
    cases = [GeoCase("single-n%d" % n, (n,), (ALIGNED,), None) for n in SINGLE_N]
    cases.append(GeoCase("sixteen", SIXTEEN_N, (ALIGNED,) * 16, None))
    for d in (1, 2, 3):
        for k in range(4):
            off = tuple(d if j == k else 0 for j in range(4))
            cases.append(GeoCase("%s+%d" % (KINDS[k], d), (1029, 6), (off, off), None))
        cases.append(GeoCase("all+%d" % d, (1029, 6), ((d,) * 4,) * 2, None))
    cases.append(GeoCase("all+1+2+3+0", (2051,), ((1, 2, 3, 0),), None))
    # aligned and misaligned segments in one launch, a short one (n < 4) among them
    cases.append(GeoCase("mixed", (1030, 9, 2, 2052, 4, 1024), (ALIGNED, (1, 1, 1, 1), ALIGNED, (0, 0, 2, 0), (0, 3, 0, 0), ALIGNED), None))
    # segments that are not launched lie between the launched ones and stay as they are
    cases.append(GeoCase("untouched", (5, 1025, 64, 3, 1024), (ALIGNED, ALIGNED, (1, 0, 0, 0), ALIGNED, ALIGNED), (0, 2, 4)))
    return cases


GEOMETRY_CASES = _geo_cases()


def geo_layout(case, gscale=1e-2):
    return Layout([(draw("%s/%d" % (case.name, s), n, gscale), off) for s, (n, off) in enumerate(zip(case.sizes, case.offs))])


def geo_launched(case):
    return list(range(len(case.sizes))) if case.launched is None else list(case.launched)


# FusedAdam: more than 16 tensors (two and three launches), parameters without a gradient, one group at several step counts
FUSED_SIZES = {17: tuple(1 + (37 * i * i + 11 * i) % 700 for i in range(17)), 33: tuple(1 + (53 * i * i + 7 * i) % 300 for i in range(33))}
# parameters without a gradient: 21 tensors, four of them with grad None, so that the 17 that have one still take two launches
FUSED_NO_GRAD_SIZES = tuple(1 + (29 * i * i + 13 * i) % 500 for i in range(21))
FUSED_NO_GRAD = (1, 4, 5, 20)


def fused_launches(sizes, no_grad=()):
    """Launches FusedAdam.step makes for one group at one step count: parameters without a gradient are dropped BEFORE the split
    into parts of MAX_SEGMENTS."""
    return -(-len([s for s in range(len(sizes)) if s not in no_grad]) // MAX_SEGMENTS)


# a capturable group: 'step' and the rate on the device; t = 7 at lr = 1e-3 is a pair where float(float32(lr)) gives another step_size
FUSED_CAPTURABLE_SIZES, FUSED_CAPTURABLE_T, FUSED_CAPTURABLE_LR = (1029, 5, 2, 515, 1024), 7, 1e-3
FUSED_STEPS = (3, 7, 3, 1000, 1, 7, 3, 100000, 1)                  # 'step' after the update, tensor by tensor


# ---- device step ----

DEVICE_LRS = (1e-3, 3e-3, 0.1)                                    # none of them is a float


def lr_through_float(lr):
    return float(F32(lr))


# ---- classes ----

POISON_N = 2053
POISON_AT = (0, 5, 1023, 1024, 2050, 2052)     # first, inside a quad, either side of a chunk boundary, inside the last quad, the scalar tail
POISONS = [("grad", x) for x in (np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-30)] + \
          [(kind, x) for kind in ("param", "exp_avg", "exp_avg_sq") for x in (np.nan, np.inf, -np.inf)] + [("exp_avg_sq", -1.0)]
POISON_T = (1, 7)


def poisoned(values, kind, x):
    out = [np.array(a) for a in values]
    out[KINDS.index(kind)][list(POISON_AT)] = F32(x)
    return tuple(out)


def classes(a):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def check_classes(got, want, clean, name=""):
    """got / want / clean: (p', m', v') of the poisoned launch, of torch's CPU fp32 Adam on the same operands, of the clean launch."""
    reach = np.zeros(len(got[0]), bool)
    reach[list(POISON_AT)] = True
    for k, (a, w, c) in enumerate(zip(got, want, clean)):
        bad = np.flatnonzero(classes(a) != classes(w))
        assert bad.size == 0, "%s: output %d, element %d is %r where torch has %r" % (name, k, bad[0], a[bad[0]], w[bad[0]])
        assert (classes(w)[~reach] == 0).all()
        bad = np.flatnonzero((bits(a) != bits(c)) & ~reach)
        assert bad.size == 0, "%s: output %d, element %d is not the clean launch's (the poison is at %r)" % (name, k, bad[0], POISON_AT)


# ---- refusals ----

# name -> (code, changes to the arguments of an ordinary three-segment launch).  seg: (segment, field, value); value "+2" / "+1" = the
# address moved by that many BYTES, 0 = a null pointer.  Every one is refused by the plan, before any launch.
REFUSALS = {
    "nseg=0": (EINVAL, dict(nseg=0)),
    "nseg=17": (EINVAL, dict(nseg=17)),
    "n=0": (EINVAL, dict(seg=(1, "n", 0))),
    "n<0": (EINVAL, dict(seg=(2, "n", -4))),
    "null param": (EINVAL, dict(seg=(0, "param", 0))),
    "null grad": (EINVAL, dict(seg=(1, "grad", 0))),
    "null exp_avg": (EINVAL, dict(seg=(2, "exp_avg", 0))),
    "null exp_avg_sq": (EINVAL, dict(seg=(0, "exp_avg_sq", 0))),
    "param+2B": (EALIGN, dict(seg=(0, "param", "+2"))),
    "grad+1B": (EALIGN, dict(seg=(1, "grad", "+1"))),
    "exp_avg+3B": (EALIGN, dict(seg=(2, "exp_avg", "+3"))),
    "exp_avg_sq+2B": (EALIGN, dict(seg=(1, "exp_avg_sq", "+2"))),
    "step=0": (EINVAL, dict(step=0)),
    "step<0": (EINVAL, dict(step=-3)),
    "lr_dev alone": (EINVAL, dict(lr_dev="+0")),
    "step_dev+2B": (EALIGN, dict(step_dev="+2")),
    "lr_dev+1B": (EALIGN, dict(step_dev="+0", lr_dev="+1")),
    "lr<0": (EINVAL, dict(lr=-1e-3)),
    "lr nan": (EINVAL, dict(lr=math.nan)),
    "beta1=1": (EINVAL, dict(beta1=1.0)),
    "beta1<0": (EINVAL, dict(beta1=-0.1)),
    "beta2=1": (EINVAL, dict(beta2=1.0)),
    "beta2 nan": (EINVAL, dict(beta2=math.nan)),
    "eps<0": (EINVAL, dict(eps=-1e-8)),
    "too many chunks": (ESHAPE, dict(seg=(2, "n", 2 ** 31 * CHUNK - 1))),
    "chunks sum": (ESHAPE, dict(seg=(0, "n", (2 ** 31 - 2) * CHUNK))),         # 2^31 - 2 chunks, and two more segments
}
REFUSAL_SIZES = (1025, 6, 300)


def refusal_args(change, seg_addr, step_dev_addr, lr_dev_addr):
    """(segments as dicts of AdamSegment fields, nseg, hyper, step, step_dev, lr_dev) of a refused call.  seg_addr: one dict per
    segment of an ordinary launch (REFUSAL_SIZES)."""
    segs = [dict(s) for s in seg_addr]
    if "seg" in change:
        s, field, val = change["seg"]
        segs[s][field] = segs[s][field] + int(val) if isinstance(val, str) else val
    h = Hyper(change.get("lr", DEFAULT.lr), change.get("beta1", DEFAULT.beta1), change.get("beta2", DEFAULT.beta2), change.get("eps", DEFAULT.eps))
    dev = lambda key, addr: addr + int(change[key]) if key in change else 0
    nseg = change.get("nseg", len(segs))
    while len(segs) < nseg:
        segs.append(dict(segs[-1]))
    return segs, nseg, h, change.get("step", 3), dev("step_dev", step_dev_addr), dev("lr_dev", lr_dev_addr)


# ---- direct launcher ----

def segment_array(lib_mod, segs):
    arr = (lib_mod.AdamSegment * max(len(segs), 1))()
    for a, s in zip(arr, segs):
        for k, v in s.items():
            setattr(a, k, v)
    return arr


def device_segments(layout, dev_bufs, which=None):
    """Dicts of AdamSegment fields: the segments `which` of a layout whose four buffers are the device tensors dev_bufs."""
    which = range(len(layout.n)) if which is None else which
    for b in dev_bufs:
        assert b.data_ptr() % 16 == 0
    return [dict(n=layout.n[s], **{KINDS[k]: dev_bufs[k].data_ptr() + 4 * layout.start[k][s] for k in range(4)}) for s in which]


def launch(lib_mod, segs, h, step, step_dev=0, lr_dev=0, nseg=None):
    """bbb_adam_step through ctypes on caller-made addresses, on the current device and stream.  segs: dicts of AdamSegment fields;
    step_dev / lr_dev: device addresses (0 = none).  Returns the entry's return code."""
    import torch
    arr = segment_array(lib_mod, segs)
    dev = torch.device("cuda", torch.cuda.current_device())
    return lib_mod.lib().bbb_adam_step(arr, len(segs) if nseg is None else nseg, float(h.lr), float(h.beta1), float(h.beta2), float(h.eps),
                                       int(step), ctypes.c_void_p(step_dev or None), ctypes.c_void_p(lr_dev or None), lib_mod.cur_stream(dev))
