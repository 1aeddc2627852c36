"""What the fused reparameterisation + KL pass (csrc/reparam_kl.hip) owes its callers, as code: the named sweep cases, float64
references, the memory images of its output layouts, and a direct launcher over bbb_reparam_kl_fwd / bbb_reparam_kl_bwd that builds
the Segment arrays itself (draw strides beyond n, views one element past a 16-byte boundary, an own call_dev word, kl_out64 -- none of
which the ops wrappers set).  tests/test_gpu_reparam_sweep.py runs the cases on the device; tests/test_reparam_sweep_cpu.py checks the
checkers, the case table and the plan query without one.

Chain of trust on the device: ops.eps_dump against the float64 Philox / Box-Muller stream (2e-5 absolute); the generic kernel with
external fp32 noise against float64 mu + eps * sigma rounded ONCE (bit equality: the product of two fp32 values is exact in float64,
the kernels use one fused multiply-add); every other form bit-equal to that "canonical" launch, laid out as its header describes.
"""
import ctypes
import zlib
from dataclasses import dataclass, field

import numpy as np

import bbb_numpy as O

F32, F64 = np.float32, np.float64
SIGMA_SQUARED, KL_TEXTBOOK, GW_MEAN_ONLY = 1, 2, 4
EINVAL, EALIGN, ESHAPE = -1, -2, -3
CHUNK = 1024
BIG_TOTAL = CHUNK * 16384
SENTINEL = F32(-7776.0)                 # exactly representable in bf16 too: every output buffer is pre-filled with it
PRIOR = (0.0, 0.1)
OFF = 5                                 # elements: a view that starts one fp32 element past a 16-byte boundary


# ------------------------------------------------------------------------------------------------ case descriptions
@dataclass(frozen=True)
class Seg:
    """One segment of a launch.  kind "f32": dense fp32 w.  "tm": fp32 tap-major, the tensor is [rows][cin][taps].  "bf16": bf16 rows
    of row_len elements (taps > 1: written tap-major).  off: the buffers that start OFF elements into their allocation (for a bf16
    w: ONE bf16 element, 2-byte aligned only).  stride_extra: draw_stride - (elements of one draw's output)."""
    n: int
    kind: str = "f32"
    rows: int = 0
    cin: int = 0
    taps: int = 0
    row_len: int = 0
    ext_eps: bool = False
    stride_extra: int = 0
    off: tuple = ()
    want_w: bool = True
    want_sigma: bool = True
    gs: bool = False                    # backward: a gradient w.r.t. the sigma output is given
    gw: bool = True                     # backward: a gradient w.r.t. w is given

    @property
    def pitch(self):
        return (self.row_len + 7) & ~7

    @property
    def extent(self):                   # elements one draw of w occupies
        return self.n // self.row_len * self.pitch if self.kind == "bf16" else self.n

    @property
    def draw_stride(self):
        return self.extent + self.stride_extra


def tm(rows, cin, taps, **kw):
    return Seg(rows * cin * taps, "tm", rows=rows, cin=cin, taps=taps, **kw)


def bf(rows, row_len, taps=0, **kw):
    return Seg(rows * row_len, "bf16", rows=rows, row_len=row_len, taps=taps, **kw)


@dataclass(frozen=True)
class Case:
    name: str
    segs: tuple                         # of Seg, or a callable slots -> tuple of Seg (the per-draw split depends on the device)
    draws: int = 1
    flags: int = 0
    call0: int = 3
    call_dev: object = None             # None | value of an own device word
    kl: str = "both"                    # "both" | "32" | "64" | "none"
    want: dict = field(default_factory=dict)      # plan fields the case was written for
    forms: tuple = ()                   # what the case is in the table for (coverage list of the CPU test)
    gkl: object = 0.37                  # backward: None = NULL

    def segments(self, slots=2048):
        return self.segs(slots) if callable(self.segs) else self.segs

    @property
    def seed(self):
        return zlib.crc32(self.name.encode()) | (0x5EED << 32)

    def stream(self, i):
        return ((zlib.crc32(self.name.encode()) >> 8) + 7 * i) & 0xFFFFFFFF


def case_inputs(case, segs):
    """(mu, rho) per segment, seeded by the case's name: mu ~ 0.1 N(0, 1), rho uniform in [-6, 2] (sigma from 0.0025 to 2.1, so that a
    noise error is not hidden under a small sigma)."""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    return [((rng.standard_normal(s.n) * 0.1).astype(F32), rng.uniform(-6.0, 2.0, s.n).astype(F32)) for s in segs]


def external_noise(case, i, n, draws):
    rng = np.random.default_rng([zlib.crc32(case.name.encode()), i, 99])
    return rng.standard_normal((draws, n)).astype(F32)


# ------------------------------------------------------------------------------------------------ the plan, restated
def plan_rules(segs, draws, slots):
    """The launch rules as the issue and include/bbb_hip.h state them, on (n, ext_eps, bf16, tm (cin, taps)) tuples."""
    total = sum(s[0] for s in segs)
    gpt = 4 if total > BIG_TOTAL else 1
    per = CHUNK * gpt
    chunks = sum(-(-s[0] // per) for s in segs)
    fast = not any(s[1] or s[2] for s in segs)
    tmb = 0
    for n, _, _, t in segs:
        if t is not None:
            rc = n // t[1]
            cg = min((CHUNK // t[1]) & ~7, rc)
            tmb += -(-rc // cg)
    excess = chunks % slots if (fast and gpt == 1 and draws > 1 and slots < chunks <= 3 * slots and tmb == 0) else 0
    return {"kernel": "fast" if fast else "generic", "gpt": gpt, "nt": fast and (gpt == 4 or draws <= 16), "chunks": chunks,
            "n_small": excess * draws, "small_chunk0": chunks - excess, "tm_blocks": tmb,
            "grid": tmb + excess * draws + chunks - excess + 1}


def descriptors(segs):
    """Segment field dicts for ops.reparam_plan: placeholder addresses with the case's alignments (nothing is read)."""
    out = []
    for i, s in enumerate(segs):
        base = 0x100000 * (i + 1)
        a = lambda k, j: base + 0x10000 * j + (4 * OFF if k in s.off else 0)
        d = {"mu": a("mu", 0), "rho": a("rho", 1), "n": s.n, "draw_stride": s.draw_stride,
             "w": (a("w", 2) if s.kind != "bf16" else base + 0x20000 + (2 if "w" in s.off else 0)) if s.want_w else 0,
             "sigma": a("sigma", 3) if s.want_sigma else 0, "eps": a("eps", 4) if s.ext_eps else 0}
        if s.kind == "bf16":
            d.update(w_row_len=s.row_len, w_taps=s.taps)
        if s.kind == "tm":
            d.update(w_tm_cin=s.cin, w_taps=s.taps)
        out.append(d)
    return out


def case_branches(case, slots=2048):
    """The launch forms and in-kernel paths a case reaches, from its description (restating the conditions in reparam_kl.hip)."""
    segs = case.segments(slots)
    p = plan_rules([(s.n, s.ext_eps, s.kind == "bf16", (s.cin, s.taps) if s.kind == "tm" else None) for s in segs], case.draws, slots)
    t = set()
    if p["kernel"] == "fast":
        t.add("fast<%d,%s>" % (p["gpt"], "nt" if p["nt"] else "plain"))
        if p["n_small"]:
            t.add("per-draw-split")
        if p["tm_blocks"]:
            t.add("tap-major-blocks")
        for s in segs:
            if s.kind == "tm":
                continue
            t.add("fast:ld_vec" if not ({"mu", "rho"} & set(s.off)) else "fast:ld_scalar")
            if s.want_w:
                t.add("fast:st_vec" if "w" not in s.off and s.draw_stride % 4 == 0 else "fast:st_scalar")
            if s.want_sigma:
                t.add("fast:sg_vec" if "sigma" not in s.off else "fast:sg_scalar")
            if s.n % 4:
                t.add("fast:tail")
    else:
        t.add("generic<%d>" % p["gpt"])
        for s in segs:
            if s.kind == "bf16":
                t.add("bf16:tap-major" if s.taps > 1 else "bf16:dense")
                packed = s.taps <= 1 and s.row_len % 4 == 0 and "w" not in s.off and s.draw_stride % 4 == 0
                t.add("bf16:packed-store" if packed else "bf16:scalar-store")
                if s.row_len % 8:
                    t.add("bf16:pad")
                t.add("bf16:ext-eps" if s.ext_eps else "bf16:philox")
            else:
                al = not s.off and s.draw_stride % 4 == 0
                t.add("generic:aligned" if al else "generic:unaligned")
                t.add("generic:ext-eps" if s.ext_eps else "generic:philox")
    if case.flags & SIGMA_SQUARED:
        t.add("flag:sigma-squared")
    if case.flags & KL_TEXTBOOK:
        t.add("flag:textbook")
    if not any(s.want_w for s in segs):
        t.add("flag:no-sample")
    t.add("kl:" + case.kl)
    if case.call_dev is not None:
        t.add("call_dev")
    return t | set(case.forms)


# ------------------------------------------------------------------------------------------------ float64 references
def kl_textbook(mu, sigma, prior_mu, prior_sigma):
    """KL(q || p), q = the posterior (mu, sigma), p = the prior: O.kl_elements with the roles as the textbook has them
    (BBB_KL_TEXTBOOK); float32 elementwise like O.kl_elements, float64 sum like O.kl_loss."""
    mu, sigma = np.asarray(mu, F32), np.asarray(sigma, F32)
    sp, mp = F32(prior_sigma), F32(prior_mu)
    t = F32(2.0) * np.log(sp / sigma) - F32(1.0) + (sigma / sp) ** 2 + ((mp - mu) / sp) ** 2
    return float(np.sum(F32(0.5) * t, dtype=F64))


def kl_reference(inputs, flags, prior=PRIOR):
    f = kl_textbook if flags & KL_TEXTBOOK else O.kl_loss
    return sum(f(mu, O.sigma_from_rho(rho), *prior) for mu, rho in inputs)


def exact_sample(mu, sigma, eps):
    """-> (w, skip): float64 mu + eps * sigma rounded once to fp32 (the product of two fp32 values is exact in float64; the sum is
    rounded to 53 bits first), and the elements where that first rounding can decide the second: the float64 sum is INEXACT (the
    two-sum error term is not zero) and sits on the bit pattern half-way between two fp32 values, or lies below the fp32 normal
    range.  An exact float64 sum on that pattern is a true tie, which the fused multiply-add and the conversion both round to
    even.  sigma: [n] fp32, eps: [draws][n] fp32."""
    m = np.broadcast_to(np.asarray(mu, F32).astype(F64)[None], np.shape(eps))
    p = np.asarray(eps, F32).astype(F64) * np.asarray(sigma, F32).astype(F64)[None]
    s = m + p
    t = s - m
    inexact = ((m - (s - t)) + (p - t)) != 0
    bits = s.view(np.uint64)
    skip = (((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & inexact) | ((np.abs(s) < 2.0 ** -126) & (s != 0))
    return s.astype(F32), skip


def check_exact(got, mu, sigma, eps):
    """got [draws][n] fp32 == exact_sample bit for bit -> number of skipped elements (at most 1 in 10^6 may be)."""
    want, skip = exact_sample(mu, sigma, eps)
    bad = (np.asarray(got, F32).view(np.uint32) != want.view(np.uint32)) & ~skip
    assert not bad.any(), "sample differs from float64 rounded once at %d of %d elements, first (draw, i) = %s" % (
        bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))
    assert skip.sum() * 10 ** 6 <= skip.size, "half-way elements skipped: %d of %d" % (skip.sum(), skip.size)
    return int(skip.sum())


def check_sigma(got, rho, squared):
    s = O.sigma_from_rho(rho)
    if squared:
        np.testing.assert_allclose(got, s.astype(F64) ** 2, rtol=1e-6)
    else:
        np.testing.assert_allclose(got, s, rtol=5e-7)


def check_kl(got, want):
    assert abs(float(got) - want) <= 1e-6 * abs(want), (float(got), want)


def check_noise(got, seed, call, stream, n, start=0):
    want = O.normal_eps(seed, call & 0xFFFFFFFF, stream, n, start=start)
    err = float(np.max(np.abs(np.asarray(got, F64) - want)))
    assert err < 2e-5, "noise differs from the float64 stream by %.3g" % err
    return err


# ------------------------------------------------------------------------------------------------ output images
def bf16_bits(a):
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def w_off(seg):
    return 0 if "w" not in seg.off else (1 if seg.kind == "bf16" else OFF)


def draw_image(seg, vals, fault=None):
    """One draw's output elements (bit patterns: uint32, or uint16 for bf16 rows) from the draw's fp32 samples in the tensor's own
    order.  Dense rows have a pitch rounded up to 8 with zero pads; tap-major columns are t * cin + ci; fp32 tap-major is
    [row][tap][ci].  fault: None | "pad" | "tm-swapped" | "pitch" (planted by the CPU self-tests)."""
    vals = np.ascontiguousarray(vals, F32)
    if seg.kind == "f32":
        return vals.view(np.uint32).copy()
    if seg.kind == "tm":
        v = vals.reshape(seg.rows, seg.cin, seg.taps)
        v = v.transpose(0, 2, 1) if fault != "tm-swapped" else v
        return np.ascontiguousarray(v).reshape(-1).view(np.uint32).copy()
    rows, rl = seg.n // seg.row_len, seg.row_len
    pitch = seg.pitch if fault != "pitch" else rl
    b = bf16_bits(vals).reshape(rows, rl)
    if seg.taps > 1:
        b = b.reshape(rows, rl // seg.taps, seg.taps)
        b = (b.transpose(0, 2, 1) if fault != "tm-swapped" else b).reshape(rows, rl)
    img = np.zeros((rows, pitch), np.uint16)
    img[:, :rl] = b
    if fault == "pad" and pitch != rl:
        img[rows // 2, rl] = 0x3F80
    out = np.full(seg.extent, sentinel_bits(seg), np.uint16)
    out[:img.size] = img.reshape(-1)
    return out


def sentinel_bits(seg):
    s = np.array([SENTINEL], F32)
    return bf16_bits(s)[0] if seg.kind == "bf16" else s.view(np.uint32)[0]


def w_image(seg, draws, vals, fault=None):
    """The whole w allocation after a launch: w_off(seg) sentinel elements, `draws` draw images draw_stride apart with the sentinel
    in the gaps, one sentinel element behind the last."""
    dt = np.uint16 if seg.kind == "bf16" else np.uint32
    off = w_off(seg)
    img = np.full(off + (draws - 1) * seg.draw_stride + seg.extent + 1, sentinel_bits(seg), dt)
    for e in range(draws):
        img[off + e * seg.draw_stride: off + e * seg.draw_stride + seg.extent] = draw_image(seg, vals[e], fault)
    return img


def check_image(got, want, what="w"):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: got %#x, want %#x" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


# ------------------------------------------------------------------------------------------------ backward references
def bwd_reference(mu, rho, gw, eps, gs, gkl, flags, prior=PRIOR):
    """Float64 of the header's formulas -> (grad_mu, grad_rho, M_mu, M_rho); M = the sum of the absolute values of the terms that
    enter the gradient (the cancellation in 1 / sigma - (sigma0^2 + d^2) / sigma^3 is then accounted for).  gw, eps: [draws][n] or
    None; gs: [n] or None; gkl: number or None.  The priors are the fp32 values the entry receives."""
    mu, rho = np.asarray(mu, F32).astype(F64), np.asarray(rho, F32).astype(F64)
    mu0, s0 = float(F32(prior[0])), float(F32(prior[1]))
    g = 0.0 if gkl is None else float(F32(gkl))
    sigma = np.log1p(np.exp(rho))
    sgm = 1.0 / (1.0 + np.exp(-rho))
    d = mu - mu0
    gw64 = np.zeros((1, mu.size)) if gw is None else np.asarray(gw, F32).astype(F64)
    if flags & KL_TEXTBOOK:
        kmu = d / s0 ** 2
        ksig_terms = (sigma / s0 ** 2, -1.0 / sigma)
    else:
        kmu = d / sigma ** 2
        ksig_terms = (1.0 / sigma, -(s0 ** 2) / sigma ** 3, -(d ** 2) / sigma ** 3)
    terms_mu = [gw64[e] for e in range(gw64.shape[0])] + [g * kmu]
    terms_rho = [g * t for t in ksig_terms]
    if gw is not None and not flags & GW_MEAN_ONLY:
        e64 = np.asarray(eps, F32).astype(F64)
        terms_rho += [gw64[e] * e64[e] for e in range(gw64.shape[0])]
    if gs is not None:
        terms_rho.append(np.asarray(gs, F32).astype(F64) * (2.0 * sigma if flags & SIGMA_SQUARED else 1.0))
    return (sum(terms_mu), sum(terms_rho) * sgm, sum(np.abs(t) for t in terms_mu), sum(np.abs(t) for t in terms_rho) * sgm)


def bwd_mirror_f32(mu, rho, gw, eps, gs, gkl, flags, prior=PRIOR, fault=None):
    """The backward kernel's expression in numpy fp32 (unfused, libm softplus).  fault: None | "drop-gs" | "drop-2sigma" |
    "mean-only-leak" | "other-kl" (planted by the CPU self-tests)."""
    mu, rho = np.asarray(mu, F32), np.asarray(rho, F32)
    mu0, s0 = F32(prior[0]), F32(prior[1])
    g = F32(0 if gkl is None else gkl)
    textbook = bool(flags & KL_TEXTBOOK) != (fault == "other-kl")
    acc_mu, acc_sig = np.zeros(mu.size, F32), np.zeros(mu.size, F32)
    if gw is not None:
        for e in range(len(gw)):
            acc_mu = acc_mu + gw[e]
            if not flags & GW_MEAN_ONLY or fault == "mean-only-leak":
                acc_sig = acc_sig + gw[e] * eps[e]
    sigma = np.log1p(np.exp(rho)).astype(F32)
    sgm = F32(1) / (F32(1) + np.exp(-rho))
    d = mu - mu0
    i = F32(1) / sigma
    if textbook:
        kmu, ksig = d / (s0 * s0), sigma / (s0 * s0) - i
    else:
        kmu, ksig = d * i * i, i - (s0 * s0 + d * d) * i * i * i
    gsv = np.zeros(mu.size, F32)
    if gs is not None and fault != "drop-gs":
        gsv = np.asarray(gs, F32) * (F32(2) * sigma if flags & SIGMA_SQUARED and fault != "drop-2sigma" else F32(1))
    return (acc_mu + g * kmu).astype(F32), ((acc_sig + g * ksig + gsv) * sgm).astype(F32)


BWD_C_MAX = 64          # softplus is within 4 ulp and enters cubed; roughly ten roundings follow
# c per flag combination: 4 x the worst |error| / (2^-23 M) measured on an MI355X against bwd_reference (external-eps tier, every
# backward case of the combination), rounded up to a power of two.  Measured ratios: see DESIGN.md, "Parameter pass".
# Measured: swapped 7.26, textbook 2.55, gs 7.35, gs-squared 6.45, mean-only 6.05, mean-only+gs 6.47, gw-null 6.64, gkl-null 1.65.
BWD_C = {"swapped": 32, "textbook": 16, "gs": 32, "gs-squared": 32, "mean-only": 32, "mean-only+gs": 32, "gw-null": 32, "gkl-null": 8}


def bwd_ratio(got_mu, got_rho, ref):
    """Worst |got - float64| / (2^-23 M) over both gradients (elements with M == 0 must be exactly zero)."""
    worst = 0.0
    for got, want, M in ((got_mu, ref[0], ref[2]), (got_rho, ref[1], ref[3])):
        err = np.abs(np.asarray(got, F32).astype(F64) - want)
        assert not (err[M == 0] != 0).any()
        nz = M > 0
        if nz.any():
            worst = max(worst, float(np.max(err[nz] / (2.0 ** -23 * M[nz]))))
    return worst


def check_bwd(got_mu, got_rho, ref, c):
    r = bwd_ratio(got_mu, got_rho, ref)
    assert r <= c, "backward error is %.3g x 2^-23 M, bound %g" % (r, c)
    return r


# ------------------------------------------------------------------------------------------------ the case tables
def _split89(slots):
    # slots + 89 chunks over five segments; the last 89 chunks (from chunk `slots` on) hold the end of segment 2 (a ragged tail,
    # n % 4 == 3), a 10-element segment (scalar stores at three draws) and segment 4 (ragged again)
    return (Seg((slots - 11) * CHUNK), Seg(10 * CHUNK), Seg(49 * CHUNK + 3), Seg(10), Seg(38 * CHUNK + 7))


def _edge(mult, plus):
    return lambda slots: (Seg((mult * slots + plus - 4) * CHUNK), Seg(2 * CHUNK + 3), Seg(7))        # mult * slots + plus chunks


def _fwd_cases():
    c = []
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4099):
        for e in (1, 2, 16, 17):
            c.append(Case("fast1-n%d-e%d" % (n, e), (Seg(n),), e, want={"kernel": "fast", "gpt": 1, "nt": e <= 16, "chunks": -(-n // CHUNK)}))
    ragged = (1, 3, 4, 5, 10, 7, 1023, 1024, 1025, 2049, 4099, 363, 33, 72, 2048, 3001)
    c.append(Case("fast16", tuple(Seg(n) for n in ragged), 3, want={"kernel": "fast", "chunks": 26}, forms=("16-segments",)))
    for kern in ("fast", "generic"):
        names = ("mu", "rho", "w", "sigma") + (("eps",) if kern == "generic" else ())
        for which in [(k,) for k in names] + [names]:
            for n in (10, 1028):
                for extra in (0, 1, 4):
                    c.append(Case("off-%s-%s-n%d-s%d" % (kern, "all" if len(which) > 1 else which[0], n, extra),
                                  (Seg(n, ext_eps=kern == "generic", stride_extra=extra, off=which), Seg(9, ext_eps=kern == "generic")), 2,
                                  want={"kernel": kern}))
    c.append(Case("split-89", _split89, 3, want={"kernel": "fast", "split": 89}, forms=("split:segment-boundary+ragged-tail",)))
    c.append(Case("split-3s-1", _edge(3, -1), 2, want={"kernel": "fast", "split": -1}))
    c.append(Case("split-3s", _edge(3, 0), 2, want={"kernel": "fast", "split": 0}, forms=("split:edge-3s",)))
    c.append(Case("split-3s+1", _edge(3, 1), 2, want={"kernel": "fast", "split": 0}, forms=("split:edge-3s+1",)))
    for rows, C, T in ((16, 8, 9), (5, 8, 2), (7, 40, 25), (3, 16, 121), (2, 8, 128), (33, 24, 9), (64, 64, 9)):
        for e in (1, 2, 3, 17):
            c.append(Case("tm-%dx%dx%d-e%d" % (rows, C, T, e), (tm(rows, C, T, stride_extra=4 * (e % 2)),), e,
                          want={"kernel": "fast", "tm_blocks": -(-(rows * C) // min((CHUNK // T) & ~7, rows * C))}))
    c.append(Case("tm-mixed", (Seg(1025), tm(33, 24, 9), Seg(10), tm(5, 8, 2, stride_extra=8), Seg(2049)), 3,
                  want={"kernel": "fast", "tm_blocks": 9}, forms=("tm:mixed-launch",)))
    for rl in (1, 2, 3, 4, 5, 7, 8, 9, 16, 33, 363, 1024, 1030):
        for rows in (1, 3, 10):
            for ext in (False, True):
                c.append(Case("bf16-r%dx%d-%s" % (rows, rl, "ext" if ext else "philox"),
                              (bf(rows, rl, ext_eps=ext, stride_extra=8 * (rows == 3)),), 3, want={"kernel": "generic"}))
    for cin, taps in ((8, 9), (16, 25), (8, 2)):
        for ext in (False, True):
            c.append(Case("bf16-tm-%dx%d-%s" % (cin, taps, "ext" if ext else "philox"),
                          (bf(5, cin * taps, taps, ext_eps=ext), bf(3, cin * taps, taps, ext_eps=ext, stride_extra=8)), 2,
                          want={"kernel": "generic"}))
    c.append(Case("bf16-w-off", (bf(3, 16, off=("w",)), bf(10, 1024, off=("w",), stride_extra=8), bf(3, 33, off=("w",)), bf(4, 64)), 2,
                  want={"kernel": "generic"}, forms=("bf16:2-byte-aligned",)))
    c.append(Case("bf16-stride", (bf(3, 363), bf(3, 363, stride_extra=8), bf(3, 72), bf(3, 72, stride_extra=8), Seg(10), Seg(7)), 3,
                  want={"kernel": "generic"}))
    mixed = (Seg(1025), Seg(10), Seg(2049), Seg(7))
    gen = (bf(10, 33), Seg(10), Seg(2049, ext_eps=True), Seg(7), Seg(1028, ext_eps=True))
    for tag, segs in (("fast", mixed), ("generic", gen)):
        c.append(Case("flag-%s-squared" % tag, segs, 2, flags=SIGMA_SQUARED))
        c.append(Case("flag-%s-textbook" % tag, segs, 2, flags=KL_TEXTBOOK))
        c.append(Case("flag-%s-nosample" % tag, tuple(Seg(s.n, want_w=False, ext_eps=s.ext_eps or s.kind == "bf16") for s in segs), 1))
        c.append(Case("flag-%s-nokl" % tag, segs, 2, kl="none"))
        c.append(Case("flag-%s-kl64" % tag, segs, 2, kl="64"))
        c.append(Case("flag-%s-kl32" % tag, segs, 2, kl="32"))
        c.append(Case("calldev5-%s" % tag, tuple(s for s in segs if not s.ext_eps), 2, call0=3, call_dev=5))
        c.append(Case("calldevwrap-%s" % tag, tuple(s for s in segs if not s.ext_eps), 2, call0=7, call_dev=2 ** 32 - 3))
    c.append(Case("calldev5-tm", (tm(16, 8, 9), Seg(10)), 2, call0=3, call_dev=5))
    return {x.name: x for x in c}


FWD_CASES = _fwd_cases()
GPT4_CASE = Case("gpt4", (Seg(BIG_TOTAL + 4096 + 3), Seg(10), tm(16, 8, 9)), 1,
                 want={"kernel": "fast", "gpt": 4, "nt": True, "chunks": 4097 + 1 + 1 + 1, "tm_blocks": 2})
# (a (16, 8, 3, 3) weight: 9 taps.  Chunks of 4096 elements: 4096 + 2 for the first segment's 4099-element rest, + 1 + 1)
GPT4_WINDOWS = (0, BIG_TOTAL - 2048, BIG_TOTAL + 4096 + 3 - 4096)

BWD_FLAGS = {"swapped": dict(), "textbook": dict(flags=KL_TEXTBOOK), "gs": dict(gs=True), "gs-squared": dict(gs=True, flags=SIGMA_SQUARED),
             "mean-only": dict(flags=GW_MEAN_ONLY), "mean-only+gs": dict(gs=True, flags=GW_MEAN_ONLY | SIGMA_SQUARED),
             "gw-null": dict(gw=False, gs=True), "gkl-null": dict(gkl=None, gs=True)}


def _bwd_cases():
    c = []
    for n in (1, 5, 1023, 1025, 4099):
        for e in (1, 3):
            for extra in (0, 4):
                c.append(("swapped", Case("bwd-n%d-e%d-s%d" % (n, e, extra), (Seg(n, stride_extra=extra),), e)))
    for combo, o in BWD_FLAGS.items():
        gs, gw = o.get("gs", False), o.get("gw", True)
        segs = (Seg(1025, gs=gs, gw=gw), Seg(10, gs=gs, gw=gw), Seg(4099, gs=False, gw=gw, stride_extra=4),
                Seg(1028, gs=gs, gw=gw, off=("mu", "rho", "w", "eps", "sigma", "gmu", "grho")), Seg(5, gs=gs, gw=gw))
        c.append((combo, Case("bwd5-" + combo, segs, 3, flags=o.get("flags", 0), gkl=o.get("gkl", 0.37))))
        c.append((combo, Case("bwd1-" + combo, (Seg(1023, gs=gs, gw=gw),), 1, flags=o.get("flags", 0), gkl=o.get("gkl", 0.37))))
    c.append(("gs", Case("bwd-calldev5", (Seg(1025, gs=True), Seg(10)), 3, call0=3, call_dev=5)))
    c.append(("gs", Case("bwd-calldevwrap", (Seg(1025, gs=True), Seg(10)), 3, call0=7, call_dev=2 ** 32 - 3)))
    return {x.name: (combo, x) for combo, x in c}


BWD_CASES = _bwd_cases()


def bwd_inputs(case, segs):
    """Per segment: mu, rho, gw [draws][n], gs [n], external eps [draws][n] (all fp32, seeded by the case's name)."""
    rng = np.random.default_rng([zlib.crc32(case.name.encode()), 5])
    out = []
    for s in segs:
        out.append(dict(mu=(rng.standard_normal(s.n) * 0.1).astype(F32), rho=rng.uniform(-6.0, 2.0, s.n).astype(F32),
                        gw=rng.standard_normal((case.draws, s.n)).astype(F32), gs=rng.standard_normal(s.n).astype(F32),
                        eps=rng.standard_normal((case.draws, s.n)).astype(F32)))
    return out


# ------------------------------------------------------------------------------------------------ direct launches (device)
class Launch:
    """Device buffers of one launch, built from Seg descriptions; every output allocation is pre-filled with SENTINEL and is one
    element longer than the launch may write."""

    def __init__(self, segs, draws, inputs, eps=None, device="cuda"):
        import torch
        from bbb_hip import _lib
        self.torch, self.lib, self.segs, self.draws, self.dev = torch, _lib, segs, draws, torch.device(device)
        self.arr = (_lib.Segment * max(len(segs), 1))()
        self.keep, self.w, self.sigma = [], [], []
        for i, (s, (mu, rho)) in enumerate(zip(segs, inputs)):
            a = self.arr[i]
            a.mu, a.rho = self._input(mu, "mu" in s.off).data_ptr(), self._input(rho, "rho" in s.off).data_ptr()
            a.n, a.draw_stride = s.n, s.draw_stride
            wt = st = None
            if s.want_w:
                size = w_off(s) + (draws - 1) * s.draw_stride + s.extent + 1
                wt = torch.full((size,), float(SENTINEL), dtype=torch.bfloat16 if s.kind == "bf16" else torch.float32, device=self.dev)
                a.w = wt.data_ptr() + w_off(s) * wt.element_size()
            if s.want_sigma:
                so = OFF if "sigma" in s.off else 0
                st = torch.full((so + s.n + 1,), float(SENTINEL), dtype=torch.float32, device=self.dev)
                a.sigma = st.data_ptr() + 4 * so
            if eps is not None and eps[i] is not None:
                # external noise: [draws][n] with the stride of w (fp32 outputs) or n (bf16 rows)
                stride = s.n if s.kind == "bf16" else s.draw_stride
                buf = np.zeros((draws - 1) * stride + s.n, F32)
                for e in range(draws):
                    buf[e * stride: e * stride + s.n] = eps[i][e]
                a.eps = self._input(buf, "eps" in s.off).data_ptr()
            if s.kind == "bf16":
                a.w_row_len, a.w_taps = s.row_len, s.taps
            if s.kind == "tm":
                a.w_tm_cin, a.w_taps = s.cin, s.taps
            self.w.append(wt)
            self.sigma.append(st)

    def _input(self, a, off):
        t = self.torch.zeros((OFF if off else 0) + len(a), dtype=self.torch.float32, device=self.dev)
        v = t[OFF if off else 0:]
        v.copy_(self.torch.from_numpy(np.ascontiguousarray(a, F32)))
        self.keep.append(t)
        return v

    def set_streams(self, case):
        for i in range(len(self.segs)):
            self.arr[i].stream_id = case.stream(i)

    def forward(self, case, parts=None, kl="both", nseg=None):
        """-> return code; kl32 / kl64 as device tensors (bit patterns are compared)."""
        torch = self.torch
        from bbb_hip import ops
        L = self.lib.lib()
        nseg = len(self.segs) if nseg is None else nseg
        self.kl32 = torch.full((1,), float("nan"), dtype=torch.float32, device=self.dev) if kl in ("both", "32") else None
        self.kl64 = torch.full((1,), float("nan"), dtype=torch.float64, device=self.dev) if kl in ("both", "64") else None
        if parts is None and kl != "none":
            parts = ops._partials(self.dev, L.bbb_reparam_partials(self.arr, nseg))
        self.cd = call_word(torch, case.call_dev, self.dev)
        p = lambda t: 0 if t is None else t.data_ptr()
        return L.bbb_reparam_kl_fwd(self.arr, nseg, self.draws, PRIOR[0], PRIOR[1], case.seed, case.call0, case.flags, p(parts),
                                    p(self.kl32), p(self.kl64), p(self.cd), self.lib.cur_stream(self.dev))

    def w_bits(self, i):
        t = self.w[i]
        return t.view(self.torch.int16 if t.dtype == self.torch.bfloat16 else self.torch.int32).cpu().numpy().view(
            np.uint16 if t.dtype == self.torch.bfloat16 else np.uint32)

    def sigma_bits(self, i):
        return self.sigma[i].view(self.torch.int32).cpu().numpy().view(np.uint32)

    def kl_bits(self):
        return (None if self.kl32 is None else int(self.kl32.view(self.torch.int32).item()),
                None if self.kl64 is None else int(self.kl64.view(self.torch.int64).item()))


def call_word(torch, value, device):
    """An own device uint32 for call_dev (None = NULL)."""
    if value is None:
        return None
    return torch.tensor([value - 2 ** 32 if value >= 2 ** 31 else value], dtype=torch.int32, device=device)


def canonical(segs):
    """The same tensors as dense, aligned fp32 segments with external noise: the launch every other form is compared with."""
    return tuple(Seg(s.n, ext_eps=True) for s in segs)


def sigma_image(seg, sigma_bits):
    """The whole sigma allocation after a launch, from the expected fp32 bit patterns of the n elements."""
    so = OFF if "sigma" in seg.off else 0
    img = np.full(so + seg.n + 1, np.array([SENTINEL], F32).view(np.uint32)[0], np.uint32)
    img[so:so + seg.n] = sigma_bits
    return img


def launch_bwd(case, segs, data, eps, device="cuda"):
    """bbb_reparam_kl_bwd on the case's segments.  eps: per segment [draws][n] external noise, or None = on-chip Philox of the case's
    seed / call0 / call_dev / streams.  -> (return code, [(grad_mu bits, grad_rho bits)] whole allocations: OFF sentinel elements when
    the segment's "gmu" / "grho" is offset, n gradients, one sentinel)."""
    import torch
    from bbb_hip import _lib
    dev = torch.device(device)
    keep, outs = [], []

    def put(a, off):
        t = torch.zeros((OFF if off else 0) + len(a), dtype=torch.float32, device=dev)
        t[OFF if off else 0:].copy_(torch.from_numpy(np.ascontiguousarray(a, F32)))
        keep.append(t)
        return t.data_ptr() + (4 * OFF if off else 0)

    def strided(a, s):
        buf = np.zeros((case.draws - 1) * s.draw_stride + s.n, F32)
        for e in range(case.draws):
            buf[e * s.draw_stride: e * s.draw_stride + s.n] = a[e]
        return buf

    arr = (_lib.Segment * len(segs))()
    pm, pr = (ctypes.c_void_p * len(segs))(), (ctypes.c_void_p * len(segs))()
    for i, (s, d) in enumerate(zip(segs, data)):
        a = arr[i]
        a.mu, a.rho = put(d["mu"], "mu" in s.off), put(d["rho"], "rho" in s.off)
        a.n, a.draw_stride, a.stream_id = s.n, s.draw_stride, case.stream(i)
        if s.gw:
            a.w = put(strided(d["gw"], s), "w" in s.off)
        if s.gs:
            a.sigma = put(d["gs"], "sigma" in s.off)
        if eps is not None:
            a.eps = put(strided(eps[i], s), "eps" in s.off)
        pair = []
        for name, ptrs in (("gmu", pm), ("grho", pr)):
            o = OFF if name in s.off else 0
            t = torch.full((o + s.n + 1,), float(SENTINEL), dtype=torch.float32, device=dev)
            ptrs[i] = t.data_ptr() + 4 * o
            pair.append(t)
        outs.append(pair)
    gkl = None if case.gkl is None else torch.tensor([case.gkl], dtype=torch.float32, device=dev)
    cd = call_word(torch, case.call_dev if eps is None else None, dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    rc = _lib.lib().bbb_reparam_kl_bwd(arr, len(segs), case.draws, PRIOR[0], PRIOR[1], case.seed, case.call0, case.flags, p(gkl), pm, pr,
                                       p(cd), _lib.cur_stream(dev))
    return rc, [tuple(t.view(torch.int32).cpu().numpy().view(np.uint32) for t in pair) for pair in outs]


def grads_of(bits, seg, name):
    """The n gradients of one allocation of launch_bwd, after checking the sentinels around them."""
    o = OFF if name in seg.off else 0
    sent = np.array([SENTINEL], F32).view(np.uint32)[0]
    assert (bits[:o] == sent).all() and bits[o + seg.n] == sent, "%s: an element outside the tensor was written" % name
    return bits[o:o + seg.n].view(F32)
