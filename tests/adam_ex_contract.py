"""The contract of the clipped / decayed / guarded Adam step (bbb_grad_sumsq, bbb_grad_norm_finish, bbb_adam_step_ex; csrc/grad_norm.hip,
csrc/adam.hip; plans csrc/grad_norm_plan.h, csrc/adam_plan.h), shared by tests/test_gpu_adam_ex.py (device) and
tests/test_adam_ex_cpu.py (the contract held against itself, no device).  It extends tests/adam_contract.py and takes the layouts,
value cases, geometry cases, sentinels and launcher helpers from there.

norm        norm = fp32(sqrt(sum double(g)^2)) over every tensor.  Reference: float64 sqrt(math.fsum(g^2)).  Bound: |norm - ref| <=
            2^-23 ref + 2^-149 -- one rounding to fp32 is 2^-24 relative, the float64 accumulation of n terms adds at most n 2^-53, and the
            bound leaves a factor of two.  Range-free: it holds at gradient scales 1e-30 and 1e30 alike.  NaN if any element is NaN,
            else +Inf if any is +-Inf.  Bit for bit the same whatever the alignment of the tensors and however they are dealt to launches.
coefficient bit for bit coef_ref(norm, max_norm): min(1, max_norm / (double(norm) + 1e-6)) in double on the launch's OWN fp32 norm, rounded
            once; NaN for a NaN norm, 0 for an Inf norm, exactly 1.0 when nothing is clipped.
values      as adam_contract's tier, with  g1 = coef g (one rounding);  L2: g1 = g1 + wd32 p;  decoupled: p0 = p decay, decay = fp32(1 - lr wd)
            formed in double.  The float64 reference takes the launch's fp32 scalars (the seven, wd32, decay, coef) and computes the rest
            in float64; p' is held to the formula on the launch's own m' and v'.  |out - ref| <= c (2^-23 M + 2^-149) with
              M_g = |coef g| + |wd32 p| (L2; |coef g| otherwise),  M_m = |m| + (M_g + |m|) omb1,  M_v = v beta2 + omb2 M_g^2,
              M_p = |p0| + |update|.
            c follows adam_contract's rule from torch's CPU fp32 Adam(foreach=False, weight_decay, decoupled_weight_decay) fed fp32(coef g),
            over VALUE_CASES x WDS x {L2, decoupled} x COEFS (test_adam_ex_cpu.py measures it and holds C_EX to the rule).
neutral     weight_decay 0 and no device scalars -- or coef = ok = 1.0 -- is bbb_adam_step bit for bit, all four buffers whole.
classes     with a NaN or an Inf among the gradients every output element has the class torch's clip_grad_norm_ + Adam (CPU fp32) has.
skip        ok = 0: nothing is stored.
"""
import ctypes
import math

import numpy as np

import adam_contract as A

F32, F64 = np.float32, np.float64
U, TINY = A.U, A.TINY
NORM_CHUNK = 4096                 # elements per block and per float64 partial
NORM_EPS = 1e-6                   # torch.nn.utils.clip_grad_norm_
MODES = ("none", "l2", "decoupled")

# c of the value bounds, by adam_contract's rule (test_adam_ex_cpu.py::test_constants_follow_from_the_fp32_reference re-measures the
# ratios: worst m 1.29, v 2.58, p 1.61 over the grid below; profiles/adam_clip_notes.md)
C_EX = {"m": 8, "v": 16, "p": 8}
WDS = (0.0, 1e-2, 0.3)
COEFS = (1.0, 0.37, 1e-3)
# weight decays at which fp32(1 - lr wd) differs between lr and float(float32(lr)) for some lr of adam_contract.DEVICE_LRS: (0.1, 7), (1e-3, 30)
DECAY_APART_WDS = (1e-2, 0.3, 7.0, 30.0)
DEVICE_DECAY = {1e-3: 30.0, 3e-3: 0.3, 0.1: 7.0}      # the decoupled decay of the device-step test, per rate

ScalarsEx = A.namedtuple("ScalarsEx", "base wd32 decay mode")


def mode_of(wd, decoupled):
    return "none" if wd == 0.0 else ("decoupled" if decoupled else "l2")


def scalars_ex(h, t, wd, decoupled, lr=None):
    """The fp32 scalars of a host-path bbb_adam_step_ex launch: adam_contract.scalars(), wd32 = fp32(wd), decay = fp32(1 - lr wd) in double."""
    lr_ = h.lr if lr is None else lr
    return ScalarsEx(A.scalars(h, t, lr), F32(wd), F32(1.0 - lr_ * wd), mode_of(wd, decoupled))


def check_scalars_ex(plan, h, t, wd, decoupled, lr=None):
    want = scalars_ex(h, t, wd, decoupled, lr)
    A.check_scalars(plan, h, t, lr)
    assert A.bits(F32(plan["wd32"])) == A.bits(want.wd32), (plan["wd32"], want.wd32)
    assert A.bits(F32(plan["decay"])) == A.bits(want.decay), (plan["decay"], want.decay, h, wd)
    assert plan["mode"] == want.mode, (plan["mode"], want.mode)


# ---- norm and coefficient ----

def norm_ref(grads):
    """float64 sqrt(fsum(g^2)) over all tensors (every product of two floats is exact in float64; fsum is exactly rounded)."""
    flat = np.concatenate([np.asarray(g, dtype=F64).ravel() for g in grads])
    if np.isnan(flat).any():
        return math.nan
    if np.isinf(flat).any():
        return math.inf
    return math.sqrt(math.fsum((flat * flat).tolist()))


def check_norm(got, grads, name=""):
    ref = norm_ref(grads)
    got = float(got)
    if math.isnan(ref) or math.isinf(ref):
        assert (math.isnan(got) if math.isnan(ref) else got == math.inf), (name, got, ref)
        return 0.0
    err = abs(got - ref)
    assert err <= U * ref + TINY, (name, got, ref, err / (U * ref + TINY))
    return err / (U * ref + TINY)


def coef_ref(norm32, max_norm):
    """The coefficient for an fp32 norm: the double formula, comparison written out, rounded to fp32 once."""
    nd = float(F32(norm32))
    if math.isnan(nd):
        return F32(np.nan)
    if max_norm == math.inf:
        return F32(1.0)
    c = max_norm / (nd + NORM_EPS)
    return F32(c) if c < 1.0 else F32(1.0)


def check_coef(got, norm32, max_norm, name=""):
    want = coef_ref(norm32, max_norm)
    if np.isnan(want):
        assert np.isnan(F32(got)), (name, got)
    else:
        assert A.bits(F32(got)) == A.bits(want), (name, float(got), float(want), float(norm32), max_norm)


def norm_model(grads, max_norm, fault=None):
    """(norm, coef) as the two launches compute them, in numpy: float64 chunk partials, float64 sum, one rounding -- the stand-in for a
    device in test_adam_ex_cpu.py.  Faults: "fp32_sumsq" accumulates the squares in fp32; "fmin" takes the coefficient with fmin."""
    acc = F32 if fault == "fp32_sumsq" else F64
    with np.errstate(all="ignore"):
        parts = [(np.asarray(g, dtype=acc)[i:i + NORM_CHUNK] ** 2).sum(dtype=acc) for g in grads for i in range(0, len(g), NORM_CHUNK)]
        norm = F32(np.sqrt(np.asarray(parts, dtype=acc).sum(dtype=acc)))
    if fault == "fmin":
        return norm, F32(np.fmin(1.0, max_norm / (float(norm) + NORM_EPS)))
    return norm, coef_ref(norm, max_norm)


NORM_SCALES = (1e-30, 1e-12, 1e-6, 1.0, 1e6, 1e30)
NORM_SINGLE_N = (1, 4095, 4096, 4097)        # one element either side of the chunk


def norm_grad(name, n, scale=1.0):
    return (scale * A._rng("norm/" + name).standard_normal(n)).astype(F32)


# ---- float64 reference, bounds ----

def g1_64(g, p, ex, coef):
    g1 = F64(F32(coef)) * np.asarray(g, dtype=F64)
    return g1 + F64(ex.wd32) * np.asarray(p, dtype=F64) if ex.mode == "l2" else g1


def value_ratios_ex(before, after, ex, coef):
    """{m, v, p: worst |out - float64| / (2^-23 M + 2^-149)} of one bbb_adam_step_ex launch; before = (p, g, m, v), after = (p', m', v')."""
    sc = ex.base
    p, g, m, v = (np.asarray(a, dtype=F64) for a in before)
    p1, m1, v1 = (np.asarray(a, dtype=F64) for a in after)
    for a in (p, g, m, v, p1, m1, v1):
        assert np.isfinite(a).all(), "non-finite value in the value tier"
    g1 = g1_64(g, p, ex, coef)
    mr, vr = A.moments64(g1, m, v, sc)
    p0 = p * F64(ex.decay) if ex.mode == "decoupled" else p
    pr, upd = A.param64(p0, m1, v1, sc)
    assert np.isfinite(pr).all() and (vr >= 0).all()
    mg = np.abs(F64(F32(coef)) * g) + (np.abs(F64(ex.wd32) * p) if ex.mode == "l2" else 0.0)
    scale = {"m": np.abs(m) + (mg + np.abs(m)) * F64(sc.omb1), "v": v * F64(sc.beta2) + F64(sc.omb2) * mg * mg, "p": np.abs(p0) + np.abs(upd)}
    err = {"m": np.abs(m1 - mr), "v": np.abs(v1 - vr), "p": np.abs(p1 - pr)}
    return {k: float((err[k] / (U * scale[k] + TINY)).max()) for k in ("m", "v", "p")}


def check_values_ex(before, after, ex, coef, name=""):
    r = value_ratios_ex(before, after, ex, coef)
    for k, x in r.items():
        assert x <= C_EX[k], (name, k, x, C_EX[k])
    return r


def torch_adam_ex(before, h, t, wd, decoupled, coef=1.0):
    """torch.optim.Adam(foreach=False, weight_decay, decoupled_weight_decay) on CPU fp32, one step from loaded state at step t, fed
    fp32(coef g).  Returns (p', m', v') as numpy."""
    import torch
    p, g, m, v = (torch.from_numpy(np.array(a)) for a in before)
    with np.errstate(all="ignore"):
        g = torch.from_numpy((F32(coef) * np.asarray(before[1], dtype=F32)).astype(F32))
    opt = torch.optim.Adam([p], lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=wd, decoupled_weight_decay=bool(decoupled), foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m, "exp_avg_sq": v}
    p.grad = g
    opt.step()
    return p.numpy(), m.numpy(), v.numpy()


def torch_clipped_adam(tensors, h, t, wd, decoupled, max_norm):
    """clip_grad_norm_ over ALL tensors, then the Adam step, on CPU fp32.  tensors: a list of (p, g, m, v).  Returns a list of (p', m', v')."""
    import torch
    ps, ms, vs = [], [], []
    for p, g, m, v in tensors:
        ps.append(torch.from_numpy(np.array(p)))
        ps[-1].grad = torch.from_numpy(np.array(g))
        ms.append(torch.from_numpy(np.array(m)))
        vs.append(torch.from_numpy(np.array(v)))
    opt = torch.optim.Adam(ps, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=wd, decoupled_weight_decay=bool(decoupled), foreach=False)
    for p, m, v in zip(ps, ms, vs):
        opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m, "exp_avg_sq": v}
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
    opt.step()
    return [(p.numpy(), m.numpy(), v.numpy()) for p, m, v in zip(ps, ms, vs)]


def model32_ex(before, ex, coef=None, fault=None):
    """bbb_adam_step_ex in fp32, operation by operation as the kernel's source states it (numpy: no contraction).  coef None = no
    coef_dev.  Fault "decay_after_update": the decoupled decay multiplies the UPDATED parameter."""
    sc = ex.base
    p, g, m, v = (np.asarray(a, dtype=F32) for a in before)
    with np.errstate(all="ignore"):
        if coef is not None:
            g = F32(coef) * g
        if ex.mode == "l2":
            g = g + ex.wd32 * p
        p0 = p * ex.decay if (ex.mode == "decoupled" and fault != "decay_after_update") else p
        m1 = m + (g - m) * sc.omb1
        v1 = v * sc.beta2 + sc.omb2 * g * g
        p1 = p0 - sc.step_size * (m1 / (np.sqrt(v1) / sc.sqrt_bc2 + sc.eps))
        if ex.mode == "decoupled" and fault == "decay_after_update":
            p1 = p1 * ex.decay
    return p1.astype(F32), m1.astype(F32), v1.astype(F32)


def check_all_classes(got, want, name=""):
    """Every element of (p', m', v') has torch's class (finite / NaN / +Inf / -Inf)."""
    for k, (a, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(A.classes(a) != A.classes(w))
        assert bad.size == 0, "%s: output %d, element %d is %r where torch has %r (%d in all)" % (name, k, bad[0], a[bad[0]], w[bad[0]], bad.size)


# ---- refusals ----

# bbb_adam_step_ex: everything bbb_adam_step refuses, with its code, then the new ones (checked after the old ones)
EX_REFUSALS = dict(A.REFUSALS)
EX_REFUSALS.update({
    "wd<0": (A.EINVAL, dict(wd=-1e-2)),
    "wd nan": (A.EINVAL, dict(wd=math.nan)),
    "coef_dev+2B": (A.EALIGN, dict(coef_dev="+2")),
    "ok_dev+1B": (A.EALIGN, dict(ok_dev="+1")),
    "coef_dev before wd": (A.EALIGN, dict(coef_dev="+3", wd=-1.0)),
    "old checks before new": (A.EINVAL, dict(lr=-1e-3, ok_dev="+2")),
})


def ex_refusal_args(change, seg_addr, step_dev_addr, lr_dev_addr, coef_addr, ok_addr):
    segs, nseg, h, step, step_dev, lr_dev = A.refusal_args({k: v for k, v in change.items() if k not in ("wd", "coef_dev", "ok_dev")},
                                                           seg_addr, step_dev_addr, lr_dev_addr)
    dev = lambda key, addr: addr + int(change[key]) if key in change else 0
    return segs, nseg, h, step, step_dev, lr_dev, change.get("wd", 1e-2), dev("coef_dev", coef_addr), dev("ok_dev", ok_addr)


# bbb_grad_sumsq: name -> (code, changes): seg (segment, field, value) as adam_contract's; partials / first
SUMSQ_REFUSALS = {
    "nseg=0": (A.EINVAL, dict(nseg=0)),
    "nseg=17": (A.EINVAL, dict(nseg=17)),
    "n=0": (A.EINVAL, dict(seg=(1, "n", 0))),
    "n<0": (A.EINVAL, dict(seg=(2, "n", -4))),
    "null grad": (A.EINVAL, dict(seg=(1, "grad", 0))),
    "grad+2B": (A.EALIGN, dict(seg=(0, "grad", "+2"))),
    "null partials": (A.EINVAL, dict(partials=0)),
    "partials+4B": (A.EALIGN, dict(partials="+4")),
    "first<0": (A.EINVAL, dict(first=-1)),
    "too many chunks": (A.ESHAPE, dict(seg=(2, "n", 2 ** 31 * NORM_CHUNK - 1))),
    "first + chunks": (A.ESHAPE, dict(first=2 ** 31 - 3)),                       # three segments of one chunk... and one of two
}
# what bbb_grad_sumsq does NOT look at: the other three pointers
SUMSQ_IGNORED = {"null param": dict(seg=(0, "param", 0)), "exp_avg+1B": dict(seg=(1, "exp_avg", "+1")), "null exp_avg_sq": dict(seg=(2, "exp_avg_sq", 0))}

# bbb_grad_norm_finish: name -> (code, keyword changes of finish_args)
FINISH_REFUSALS = {
    "null partials": (A.EINVAL, dict(partials=0)),
    "partials+4B": (A.EALIGN, dict(partials="+4")),
    "npartials=0": (A.EINVAL, dict(npartials=0)),
    "npartials<0": (A.EINVAL, dict(npartials=-7)),
    "npartials 2^31": (A.ESHAPE, dict(npartials=2 ** 31)),
    "null norm_out": (A.EINVAL, dict(norm=0)),
    "norm_out+2B": (A.EALIGN, dict(norm="+2")),
    "coef_out+1B": (A.EALIGN, dict(coef="+1")),
    "ok_out+3B": (A.EALIGN, dict(ok="+3")),
    "skipped_out+2B": (A.EALIGN, dict(skipped="+2")),
    "max_norm=0": (A.EINVAL, dict(max_norm=0.0)),
    "max_norm<0": (A.EINVAL, dict(max_norm=-1.0)),
    "max_norm nan": (A.EINVAL, dict(max_norm=math.nan)),
}


def moved(change, key, addr):
    v = change.get(key, "+0")
    return addr + int(v) if isinstance(v, str) else v


# ---- direct launchers ----

def _void(addr):
    return ctypes.c_void_p(addr or None)


def launch_ex(lib_mod, segs, h, step, wd=0.0, decoupled=False, step_dev=0, lr_dev=0, coef_dev=0, ok_dev=0, nseg=None):
    """bbb_adam_step_ex through ctypes on caller-made addresses, on the current device and stream."""
    import torch
    arr = A.segment_array(lib_mod, segs)
    dev = torch.device("cuda", torch.cuda.current_device())
    return lib_mod.lib().bbb_adam_step_ex(arr, len(segs) if nseg is None else nseg, float(h.lr), float(h.beta1), float(h.beta2), float(h.eps),
                                          float(wd), int(bool(decoupled)), int(step), _void(step_dev), _void(lr_dev), _void(coef_dev),
                                          _void(ok_dev), lib_mod.cur_stream(dev))


def chunks_of(n):
    return -(-n // NORM_CHUNK)


def launch_norm(lib_mod, segs, partials, scalars, skipped, max_norm=math.inf, skip=False, deal=None):
    """bbb_grad_sumsq over `segs` (dicts with grad and n) dealt to launches as `deal` (a list of counts; default 16, 16, ...), then ONE
    bbb_grad_norm_finish into scalars[0..2] = (norm, coef, ok) and `skipped` (device tensors; partials float64).  Returns the partial count."""
    import torch
    L = lib_mod.lib()
    stream = lib_mod.cur_stream(torch.device("cuda", torch.cuda.current_device()))
    deal = list(deal) if deal is not None else [A.MAX_SEGMENTS] * (-(-len(segs) // A.MAX_SEGMENTS))
    assert sum(deal) >= len(segs)
    at = first = 0
    for count in deal:
        part = segs[at:at + count]
        if not part:
            break
        assert L.bbb_grad_sumsq(A.segment_array(lib_mod, part), len(part), _void(partials.data_ptr()), first, stream) == 0
        first += sum(chunks_of(s["n"]) for s in part)
        at += count
    assert first <= partials.numel()
    assert L.bbb_grad_norm_finish(_void(partials.data_ptr()), first, float(max_norm), int(bool(skip)), _void(scalars.data_ptr()),
                                  _void(scalars.data_ptr() + 4), _void(scalars.data_ptr() + 8), _void(skipped.data_ptr()), stream) == 0
    return first
