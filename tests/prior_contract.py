"""What the tensor-prior entries of the fused reparameterisation + KL pass (bbb_reparam_kl_tp_fwd / _tp_bwd / _tp_plan) owe their
callers, as code, on top of tests/reparam_contract.py: the prior input regimes, the per-segment prior kinds, float64 references with
the magnitude M the error bounds are stated in, a numpy fp32 mirror of the kernel's expression (with planted faults), the case table
and direct launchers.  tests/test_gpu_prior_sweep.py runs the cases on the device, tests/test_prior_cpu.py checks the checkers.

The contract: the prior reaches the KL only.  w, sigma and every sentinel are the scalar entry's bits.  The KL float and double are
within c * 2^-23 * M of the float64 sum, M = sum_i 0.5 (|2 ln(sigma_i / sigma0_i)| + 1 + a_i^2 + b_i^2) -- the sum of the absolute
values of the terms, so the bound keeps its meaning where the terms cancel: with mu0 = mu, sigma0 = sigma ("equal") the true KL is 0,
a relative bound says nothing, and the fp32 result may be slightly NEGATIVE.  That is allowed.
"""
import ctypes
import zlib

import numpy as np

import bbb_numpy as O
import reparam_contract as C

F32, F64 = np.float32, np.float64
REGIMES = ("random", "near", "equal", "const")
KINDS = ("tt", "t-", "-t", "--", "off")          # (mean, sigma): tensor or scalar; off = both tensors, views C.OFF elements past a 16-byte boundary

FWD_C_MAX = 64
# c per kernel: 4 x the worst |KL - float64| / (2^-23 M) measured on an MI355X over every forward case of the table below (float and
# double output, the four-groups-per-thread launch included), rounded up to a power of two.
# Measured: fast 3.253 (72 values), generic 2.287 (30 values); see profiles/tensor_prior_notes.md.
FWD_C = {"fast": 16, "generic": 16}
# backward, per flag combination of C.BWD_FLAGS, built like C.BWD_C with the tensor-prior M; the cap is C.BWD_C_MAX.
# Measured: swapped 5.98, textbook 2.39, gs 7.09, gs-squared 7.16, mean-only 6.52, mean-only+gs 6.73, gw-null 7.04, gkl-null 1.65.
BWD_C = {"swapped": 32, "textbook": 16, "gs": 32, "gs-squared": 32, "mean-only": 32, "mean-only+gs": 32, "gw-null": 32, "gkl-null": 8}


# ------------------------------------------------------------------------------------------------ inputs
def prior_inputs(name, regime, inputs):
    """(mu0, sigma0) fp32 per segment for the regime, seeded by the case name."""
    rng = np.random.default_rng([zlib.crc32(name.encode()), 77])
    out = []
    for mu, rho in inputs:
        n = mu.size
        sigma = O.sigma_from_rho(rho)
        if regime == "random":
            mu0 = (0.1 * rng.standard_normal(n)).astype(F32)
            s0 = np.exp(rng.uniform(np.log(0.003), np.log(2.0), n)).astype(F32)
        elif regime == "near":
            mu0 = (mu * (1 + 0.01 * rng.standard_normal(n))).astype(F32)
            s0 = (sigma * np.exp(0.1 * rng.standard_normal(n))).astype(F32)
        elif regime == "equal":
            mu0, s0 = mu.copy(), sigma.astype(F32).copy()
        elif regime == "const":
            mu0, s0 = np.full(n, C.PRIOR[0], F32), np.full(n, C.PRIOR[1], F32)
        else:
            raise KeyError(regime)
        out.append((mu0, s0))
    return out


def effective(kind, pri, n, scalar=C.PRIOR):
    """What a segment of `kind` is held to: the tensors it passes, the launch-wide scalar where it passes none."""
    mu0 = pri[0] if kind in ("tt", "t-", "off") else np.full(n, scalar[0], F32)
    s0 = pri[1] if kind in ("tt", "-t", "off") else np.full(n, scalar[1], F32)
    return mu0, s0


# ------------------------------------------------------------------------------------------------ float64 references
def kl_terms64(mu, sigma, mu0, s0, textbook):
    """Float64 of the header's term on fp32 inputs -> (terms, magnitudes)."""
    mu, sigma, mu0, s0 = (np.asarray(v, F32).astype(F64) for v in (mu, sigma, mu0, s0))
    lr = np.log(sigma / s0)
    if textbook:
        a, b, sgn = sigma / s0, (mu0 - mu) / s0, -1.0
    else:
        a, b, sgn = s0 / sigma, (mu - mu0) / sigma, 1.0
    return 0.5 * (sgn * 2 * lr - 1 + a * a + b * b), 0.5 * (np.abs(2 * lr) + 1 + a * a + b * b)


def kl_reference_tp(inputs, priors, flags):
    """-> (KL, M) over the segments: inputs [(mu, rho)], priors [(mu0, sigma0)] effective arrays; sigma is the oracle's fp32 softplus."""
    kl = m = 0.0
    for (mu, rho), (mu0, s0) in zip(inputs, priors):
        t, mag = kl_terms64(mu, O.sigma_from_rho(rho), mu0, s0, bool(flags & C.KL_TEXTBOOK))
        kl += float(t.sum())
        m += float(mag.sum())
    return kl, m


def kl_mirror_f32(mu, sigma, mu0, s0, textbook, fault=None):
    """The kernels' expression per element in numpy fp32: exact division, libm log2.  fault (planted by the CPU self-tests): "shift"
    (prior index off by one), "swap" (mu0 and sigma0 exchanged), "scalar" (the scalar fallback where a tensor was given)."""
    mu, sigma, mu0, s0 = (np.asarray(v, F32) for v in (mu, sigma, mu0, s0))
    if fault == "shift":
        mu0, s0 = np.roll(mu0, 1), np.roll(s0, 1)
    elif fault == "swap":
        mu0, s0 = s0, np.abs(mu0) + F32(1e-3)
    elif fault == "scalar":
        mu0, s0 = np.full_like(mu0, C.PRIOR[0]), np.full_like(s0, C.PRIOR[1])
    l2 = np.log2(sigma / s0)          # (the log of the exact quotient; the kernels subtract two hardware logs: the device bound covers that)
    k = F64(F32(1.3862943611198906))
    fma = lambda x, y: (x * l2.astype(F64) + y).astype(F32)        # one rounding, as the kernels' fmaf: the fp32 product is exact in float64
    if textbook:
        a, b = sigma / s0, (mu0 - mu) / s0
        t = fma(-k, -1.0) + a * a + b * b
    else:
        a, b = s0 / sigma, (mu - mu0) / sigma
        t = fma(k, -1.0) + a * a + b * b
    return (F32(0.5) * t).astype(F32)


def kl_ratio(got, ref):
    kl, m = ref
    return abs(float(got) - kl) / (2.0 ** -23 * m)


def check_kl_tp(got, ref, c):
    r = kl_ratio(got, ref)
    assert np.isfinite(float(got)) and r <= c, "KL %r, float64 %r: %.3g x 2^-23 M, bound %g" % (float(got), ref[0], r, c)
    return r


def bwd_reference_tp(mu, rho, gw, eps, gs, gkl, flags, mu0, s0):
    """C.bwd_reference with array priors -> (grad_mu, grad_rho, M_mu, M_rho)."""
    mu, rho = np.asarray(mu, F32).astype(F64), np.asarray(rho, F32).astype(F64)
    mu0, s0 = np.asarray(mu0, F32).astype(F64), np.asarray(s0, F32).astype(F64)
    g = 0.0 if gkl is None else float(F32(gkl))
    sigma = np.log1p(np.exp(rho))
    sgm = 1.0 / (1.0 + np.exp(-rho))
    d = mu - mu0
    gw64 = np.zeros((1, mu.size)) if gw is None else np.asarray(gw, F32).astype(F64)
    if flags & C.KL_TEXTBOOK:
        kmu = d / s0 ** 2
        ksig_terms = (sigma / s0 ** 2, -1.0 / sigma)
    else:
        kmu = d / sigma ** 2
        ksig_terms = (1.0 / sigma, -(s0 ** 2) / sigma ** 3, -(d ** 2) / sigma ** 3)
    terms_mu = [gw64[e] for e in range(gw64.shape[0])] + [g * kmu]
    terms_rho = [g * t for t in ksig_terms]
    if gw is not None and not flags & C.GW_MEAN_ONLY:
        e64 = np.asarray(eps, F32).astype(F64)
        terms_rho += [gw64[e] * e64[e] for e in range(gw64.shape[0])]
    if gs is not None:
        terms_rho.append(np.asarray(gs, F32).astype(F64) * (2.0 * sigma if flags & C.SIGMA_SQUARED else 1.0))
    return (sum(terms_mu), sum(terms_rho) * sgm, sum(np.abs(t) for t in terms_mu), sum(np.abs(t) for t in terms_rho) * sgm)


def bwd_mirror_tp_f32(mu, rho, gw, eps, gs, gkl, flags, mu0, s0, fault=None):
    """C.bwd_mirror_f32 with array priors; faults as kl_mirror_f32."""
    mu, rho, mu0, s0 = (np.asarray(v, F32) for v in (mu, rho, mu0, s0))
    if fault == "shift":
        mu0, s0 = np.roll(mu0, 1), np.roll(s0, 1)
    elif fault == "swap":
        mu0, s0 = s0, np.abs(mu0) + F32(1e-3)
    elif fault == "scalar":
        mu0, s0 = np.full_like(mu0, C.PRIOR[0]), np.full_like(s0, C.PRIOR[1])
    g = F32(0 if gkl is None else gkl)
    acc_mu, acc_sig = np.zeros(mu.size, F32), np.zeros(mu.size, F32)
    if gw is not None:
        for e in range(len(gw)):
            acc_mu = acc_mu + gw[e]
            if not flags & C.GW_MEAN_ONLY:
                acc_sig = acc_sig + gw[e] * eps[e]
    sigma = np.log1p(np.exp(rho)).astype(F32)
    sgm = F32(1) / (F32(1) + np.exp(-rho))
    d = mu - mu0
    i = F32(1) / sigma
    if flags & C.KL_TEXTBOOK:
        kmu, ksig = d / (s0 * s0), sigma / (s0 * s0) - i
    else:
        kmu, ksig = d * i * i, i - (s0 * s0 + d * d) * i * i * i
    gsv = np.zeros(mu.size, F32)
    if gs is not None:
        gsv = np.asarray(gs, F32) * (F32(2) * sigma if flags & C.SIGMA_SQUARED else F32(1))
    return (acc_mu + g * kmu).astype(F32), ((acc_sig + g * ksig + gsv) * sgm).astype(F32)


# ------------------------------------------------------------------------------------------------ the case table
def _cycle(kinds, n):
    return tuple(kinds[i % len(kinds)] for i in range(n))


def _fwd_cases():
    """name -> (C.Case, prior kinds per segment | callable(nseg), regime)."""
    t = {}
    F = C.FWD_CASES
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4099):
        for e in (1, 3):
            for k, (kind, regime) in enumerate((("tt", "random"), ("off", "near"))):
                if k == 1 and (n, e) not in ((5, 3), (1025, 1), (4099, 3)):
                    continue
                t["tp-n%d-e%d-%s" % (n, e, kind)] = (C.Case("tp-n%d-e%d" % (n, e), (C.Seg(n),), e), (kind,), regime)
    t["tp-fast16"] = (F["fast16"], _cycle(("tt", "t-", "-t", "--", "off"), 16), "random")
    t["tp-fast16-equal"] = (F["fast16"], _cycle(("tt", "off"), 16), "equal")
    t["tp-fast16-const"] = (F["fast16"], _cycle(("tt", "off", "tt"), 16), "const")
    for kern in ("fast", "generic"):
        for n in (10, 1028):
            t["tp-off-%s-n%d" % (kern, n)] = (F["off-%s-all-n%d-s1" % (kern, n)], ("off", "tt"), "random")
            t["tp-aligned-prior-%s-n%d" % (kern, n)] = (F["off-%s-all-n%d-s0" % (kern, n)], ("tt", "-t"), "near")
    t["tp-split-89"] = (F["split-89"], ("--", "t-", "tt", "off", "-t"), "random")      # the boundary lies inside segment 2 (tt)
    t["tp-tm-mixed"] = (F["tm-mixed"], ("tt", "tt", "off", "-t", "t-"), "random")
    for rows, rl in ((3, 33), (10, 1024)):
        for src in ("philox", "ext"):
            t["tp-bf16-r%dx%d-%s" % (rows, rl, src)] = (F["bf16-r%dx%d-%s" % (rows, rl, src)], ("tt",), "near" if rows == 3 else "random")
    mixed4, gen5 = ("tt", "off", "t-", "-t"), ("tt", "off", "t-", "--", "-t")
    for tag, kinds in (("fast", mixed4), ("generic", gen5)):
        for flag, regime in (("squared", "random"), ("textbook", "random"), ("nosample", "near"), ("nokl", "random"), ("kl64", "random"),
                             ("kl32", "equal")):
            t["tp-flag-%s-%s" % (tag, flag)] = (F["flag-%s-%s" % (tag, flag)], kinds, regime)
        t["tp-flag-%s-textbook-equal" % tag] = (F["flag-%s-textbook" % tag], kinds, "equal")
        t["tp-flag-%s-textbook-const" % tag] = (F["flag-%s-textbook" % tag], _cycle(("tt",), len(kinds)), "const")
        t["tp-calldev5-%s" % tag] = (F["calldev5-%s" % tag], lambda n: _cycle(("tt", "off", "t-"), n), "random")
    return t


FWD_CASES = _fwd_cases()
GPT4_KINDS = ("tt", "off", "t-")
BWD_SEG_KINDS = ("tt", "t-", "-t", "off", "--")


def kinds_of(entry, nseg):
    k = entry[1]
    return k(nseg) if callable(k) else k


def _bwd_cases():
    """name -> (combo, C.Case, kinds, regime): C.BWD_FLAGS' eight combinations on the five-segment launch, plus n in (1, 5, 1023)."""
    t = {}
    for name, (combo, case) in C.BWD_CASES.items():
        if name.startswith("bwd5-"):
            t["tp-" + name] = (combo, case, BWD_SEG_KINDS, "random")
        elif name in ("bwd-n1-e1-s0", "bwd-n5-e3-s4", "bwd-n1023-e3-s0"):
            t["tp-" + name] = (combo, case, ("tt",) if "n5" not in name else ("off",), "near")
    t["tp-bwd5-textbook-equal"] = ("textbook", C.BWD_CASES["bwd5-textbook"][1], BWD_SEG_KINDS, "equal")
    return t


BWD_CASES = _bwd_cases()


# ------------------------------------------------------------------------------------------------ direct launches (device)
class PriorBuffers:
    """Device copies of a launch's prior tensors and the PriorSegment array over them; kind "off" views start C.OFF elements into
    their allocation."""

    def __init__(self, kinds, priors, device="cuda"):
        import torch
        from bbb_hip import _lib
        self.arr = (_lib.PriorSegment * max(len(kinds), 1))()
        self.keep = []
        for i, (k, (mu0, s0)) in enumerate(zip(kinds, priors)):
            for name, a, used in (("mu0", mu0, k in ("tt", "t-", "off")), ("sigma0", s0, k in ("tt", "-t", "off"))):
                if not used:
                    continue
                off = C.OFF if k == "off" else 0
                t = torch.full((off + len(a),), 1.0, dtype=torch.float32, device=device)
                t[off:].copy_(torch.from_numpy(np.ascontiguousarray(a, F32)))
                self.keep.append(t)
                setattr(self.arr[i], name, t.data_ptr() + 4 * off)


def forward_tp(L, case, pri_arr, kl="both", parts=None, prior=C.PRIOR):
    """C.Launch.forward through bbb_reparam_kl_tp_fwd; pri_arr: a PriorSegment array or None (pri == NULL)."""
    torch = L.torch
    from bbb_hip import ops
    lib = L.lib.lib()
    nseg = len(L.segs)
    L.kl32 = torch.full((1,), float("nan"), dtype=torch.float32, device=L.dev) if kl in ("both", "32") else None
    L.kl64 = torch.full((1,), float("nan"), dtype=torch.float64, device=L.dev) if kl in ("both", "64") else None
    if parts is None and kl != "none":
        parts = ops._partials(L.dev, lib.bbb_reparam_partials(L.arr, nseg))
    L.cd = C.call_word(torch, case.call_dev, L.dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    return lib.bbb_reparam_kl_tp_fwd(L.arr, pri_arr, nseg, L.draws, prior[0], prior[1], case.seed, case.call0, case.flags, p(parts),
                                     p(L.kl32), p(L.kl64), p(L.cd), L.lib.cur_stream(L.dev))


def launch_bwd_tp(case, segs, data, eps, pri_arr, device="cuda"):
    """C.launch_bwd through bbb_reparam_kl_tp_bwd (the same buffers, sentinels and return value)."""
    import torch
    from bbb_hip import _lib
    dev = torch.device(device)
    keep, outs = [], []
    OFF = C.OFF

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
            t = torch.full((o + s.n + 1,), float(C.SENTINEL), dtype=torch.float32, device=dev)
            ptrs[i] = t.data_ptr() + 4 * o
            pair.append(t)
        outs.append(pair)
    gkl = None if case.gkl is None else torch.tensor([case.gkl], dtype=torch.float32, device=dev)
    cd = C.call_word(torch, case.call_dev if eps is None else None, dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    rc = _lib.lib().bbb_reparam_kl_tp_bwd(arr, pri_arr, len(segs), case.draws, C.PRIOR[0], C.PRIOR[1], case.seed, case.call0, case.flags,
                                          p(gkl), pm, pr, p(cd), _lib.cur_stream(dev))
    return rc, [tuple(t.view(torch.int32).cpu().numpy().view(np.uint32) for t in pair) for pair in outs]
