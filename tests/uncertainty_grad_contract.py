"""Contract of the backward of the batch-innermost uncertainty reduction (csrc/mc_uncertainty.hip: bbb_mc_uncertainty_cb_bwd,
ops.mc_uncertainty_cb_autograd) for tests/test_uncertainty_grad_cpu.py and tests/test_gpu_uncertainty_grad.py, built on
tests/uncertainty_cb_contract.py: its named cases, seeded logits, probabilities and injections; here the upstream-gradient patterns, a
float64 reference (the closed form of include/bbb_hip.h with its zero conventions), an fp32 numpy model of the kernel's order of
operations, the error scale and the stored model constant.  No device and no library needed; nothing is taken from kernel output.

With L = sum over the seven outputs of (upstream gradient x output), per image:
    G[t,k] = (-(w_ent + w_mi) log p_bar[k] - (w_ee - w_mi) log p[t,k] + w_pm[k] + 2 w_epi[k] (p[t,k] - p_bar[k])
              + w_ale[k] (1 - 2 p[t,k])) / T,        D[t] = sum_k p[t,k] G[t,k],
    d L / d logits[t,c] = J[t,c] (G[t,c] - D[t]) + w_pred[c] / T,     J = p (softmax), sigmoid(v) / z (normalized; 1 / z above 20).
Conventions: a class with p = 0 contributes exactly 0 to D and its probability side J (G - D) is exactly 0, so what it receives is
w_pred / T alone -- an exact 0 under every pattern without w_pred (the -inf classes of the neginf cases; d pred / d logit = 1 / T holds
at any logit, so WITH w_pred the value there is w_pred / T in both references); the log p_bar term is 0 where p_bar = 0; T = 1: log p_bar
is log p; the clamp of mutual_info is not differentiated; the `== 0` tests are false for NaN.  An absent upstream gradient is a zero in
the same arithmetic, so 0 x NaN stays NaN: an image with a NaN or +inf logit is NaN in every element under every pattern.

Error scale of image b: 2^-24 x max over (t, c) of A[t,c,b], A = the same backward on |operands|: the closed form with every added
term replaced by its absolute value, J (|G| + sum_k p |G|) + |w_pred| / T with |G| = ((|w_ent| + |w_mi|) |log p_bar| + (|w_ee| + |w_mi|)
|log p| + |w_pm| + 2 |w_epi| (p + p_bar) + |w_ale| (1 + 2 p)) / T (0 where p = 0, as G) -- the differences p - p_bar and 1 - 2 p are sums
of two terms themselves, so an upstream weight on epistemic keeps a scale where every draw agrees (p = p_bar).  A >= |gradient|, and A
is non-zero wherever a term is; where an image's scale is 0 (all of its upstream weights zero) every element of the image must be
exactly 0.  The device bound of a pattern is DEVICE_FACTOR x MODEL_CONSTANT[pattern], the latter the worst ratio of the fp32 model over
all cases, rounded up to one significant digit (tests/test_uncertainty_grad_cpu.py measures it again).  The constants of the entropy
patterns are the 'dominant' cases': a class 40 below the row maximum has log p = -40 rounded to 40 x 2^-24, so its p -- and all of a
gradient that is made of such classes -- carries |log p| roundings, not one."""
import numpy as np

import uncertainty_cb_contract as K
from tail_contract import DEVICE_FACTOR, F32, U, round_up_1sf  # noqa: F401  (round_up_1sf, DEVICE_FACTOR: for the tests)

CASES, BY_NAME, FIELDS, PER_CLASS, MAX_DRAWS = K.CASES, K.BY_NAME, K.FIELDS, K.PER_CLASS, K.MAX_DRAWS
rows_of, probs64 = K.rows_of, K.probs64
ENTRY = "mc_uncertainty_cb_bwd"
EINVAL, EALIGN, ESHAPE = K.EINVAL, K.EALIGN, K.ESHAPE
PATTERNS = FIELDS + ("all", "all_alternate")       # each field alone with weights of one; all seven Gaussian; the same with every
                                                   # other image's weights zero

# worst |fp32 model - float64 reference| / scale over CASES per pattern, rounded up to one significant digit
MODEL_CONSTANT = {"pred": 0.3, "p_mean": 2.0, "epistemic": 2.0, "aleatoric": 2.0, "entropy": 30.0, "expected_entropy": 30.0,
                  "mutual_info": 3.0, "all": 2.0, "all_alternate": 2.0}


def upstream_of(case, pattern):
    """{field: fp32 upstream gradient [B][C] or [B], or None (absent: a NULL pointer)} of a pattern."""
    B, C = case.B, case.C
    shape = lambda f: (B, C) if f in PER_CLASS else (B,)
    if pattern in FIELDS:
        return {f: np.ones(shape(f), F32) if f == pattern else None for f in FIELDS}
    rng = np.random.default_rng(case.seed + 3)
    w = {f: rng.standard_normal(shape(f)).astype(F32) for f in FIELDS}
    if pattern == "all_alternate":
        for f in FIELDS:
            w[f][1::2] = 0
    else:
        assert pattern == "all"
    return w


def _dense(w, B, C, dtype):
    """The seven upstream gradients with zeros for the absent ones: per-class ones [1][B][C], per-image ones [1][B][1]."""
    out = []
    for i, f in enumerate(FIELDS):
        a = np.zeros((B, C) if i < 4 else (B,), dtype) if w[f] is None else np.asarray(w[f], dtype)
        out.append(a[None] if i < 4 else a[None, :, None])
    return out


# ------------------------------------------------------------------------------------------------ float64 reference
def reference(rows, normalized, w):
    """(gradient, A), each [T][B][C] float64: the closed form and the same form on absolute values."""
    z = np.asarray(rows, np.float64)
    T, B, C = z.shape
    p, lp = probs64(rows, normalized)
    w_pred, w_pm, w_epi, w_ale, w_ent, w_ee, w_mi = _dense(w, B, C, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pbar = p.mean(axis=0)[None]
        lpbar = lp if T == 1 else np.log(pbar)
        terms = [np.where(pbar == 0, 0.0, -(w_ent + w_mi) * lpbar), -(w_ee - w_mi) * lp, w_pm + 0 * p, 2 * w_epi * (p - pbar),
                 w_ale * (1 - 2 * p)]
        a = np.abs
        terms_abs = [np.where(pbar == 0, 0.0, (a(w_ent) + a(w_mi)) * a(lpbar)), (a(w_ee) + a(w_mi)) * a(lp), a(w_pm) + 0 * p,
                     2 * a(w_epi) * (p + pbar), a(w_ale) * (1 + 2 * p)]
        zero = p == 0
        G = np.where(zero, 0.0, sum(terms) / T)
        Ga = np.where(zero, 0.0, sum(terms_abs) / T)
        if normalized:
            sp = np.where(z > 20, z, np.log1p(np.exp(np.minimum(z, 20))))
            J = np.where(z > 20, 1.0, 1.0 / (1.0 + np.exp(-z))) / sp.sum(axis=2, keepdims=True)
        else:
            J = p
        D = np.where(zero, 0.0, p * G).sum(axis=2, keepdims=True)
        Da = np.where(zero, 0.0, p * Ga).sum(axis=2, keepdims=True)
        g = np.where(zero, 0.0, J * (G - D)) + w_pred / T
        A = np.where(zero, 0.0, J * (Ga + Da)) + np.abs(w_pred) / T
    return g, A


# ------------------------------------------------------------------------------------------------ fp32 model of the kernel
def forward_p_mean(rows, normalized):
    """p_mean [B][C] fp32 as mc_uncertainty_cb_kernel forms it (uncertainty_cb_contract.model, its first sweep alone)."""
    v = np.asarray(rows, F32)
    a, lz = _partition(v, normalized)
    _, p = _prob(v, a, lz, normalized)
    s_p = np.zeros(v.shape[1:], F32)
    with np.errstate(invalid="ignore"):
        for t in range(v.shape[0]):
            s_p = s_p + p[t]
        return s_p / F32(v.shape[0])


def _partition(v, normalized):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if normalized:
            a = K._comp_sum(K._softplus32(v))
            return a, np.log(a)
        a = np.fmax.reduce(v, axis=2)
        return a, np.log(K._comp_sum(np.exp(v - a[..., None])))


def _prob(v, a, lz, normalized):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if normalized:
            q = K._softplus32(v)
            return np.log(q) - lz[..., None], q / a[..., None]
        ls = (v - a[..., None]) - lz[..., None]
        return ls, np.exp(ls)


def model(rows, normalized, w, p_mean=None):
    """mc_uncertainty_cb_bwd_kernel in fp32 numpy -> [T][B][C] float32 (every product and sum rounded once; the device contracts some into
    fused multiply-adds, which DEVICE_FACTOR covers)."""
    v = np.asarray(rows, F32)
    T, B, C = v.shape
    pb = (forward_p_mean(rows, normalized) if p_mean is None else np.asarray(p_mean, F32))[None]
    w_pred, w_pm, w_epi, w_ale, w_ent, w_ee, w_mi = _dense(w, B, C, F32)
    fT, one, two = F32(T), F32(1), F32(2)
    a, lz = _partition(v, normalized)
    ls, p = _prob(v, a, lz, normalized)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c_bar, c_t = -(w_ent + w_mi), -(w_ee - w_mi)
        lpb = ls if T == 1 else np.log(pb)
        t_bar = np.where(pb == 0, F32(0), c_bar * lpb)
        t_epi = two * w_epi * (p - pb)
        t_ale = w_ale * (one - two * p)
        G = ((((t_bar + c_t * ls) + w_pm) + t_epi) + t_ale) / fT
        zero = p == 0
        D = K._comp_sum(np.where(zero, F32(0), p * G))[..., None]
        J = np.where(v > 20, one, one / (one + np.exp(-v))) / a[..., None] if normalized else p
        out = np.where(zero, F32(0), J * (G - D)) + w_pred / fT
    assert out.dtype == F32 and out.shape == v.shape
    return out


# ------------------------------------------------------------------------------------------------ error scale and checks
def image_scales(A):
    """[B]: 2^-24 x the largest finite A of the image."""
    return U * np.where(np.isfinite(A), A, 0.0).max(axis=(0, 2))


def ratio(got, g64, A):
    """Worst |got - g64| / scale of its image over the elements where the reference is finite.  NaN and infinities of the reference must
    be met at exactly their positions; an image whose scale is 0 must be exactly 0."""
    got, g64 = np.asarray(got, np.float64), np.asarray(g64, np.float64)
    assert got.shape == g64.shape, (got.shape, g64.shape)
    assert (np.isnan(got) == np.isnan(g64)).all(), "NaN positions differ from the reference's"
    inf = np.isinf(g64)
    assert (np.isinf(got) == inf).all() and (got[inf] == g64[inf]).all(), "infinities differ from the reference's"
    sc = np.broadcast_to(image_scales(A)[None, :, None], g64.shape)
    fin = np.isfinite(g64)
    dead = fin & (sc == 0)
    assert not got[dead].any(), "an image without upstream weight must get exact zeros"
    live = fin & (sc > 0)
    return float((np.abs(got[live] - g64[live]) / sc[live]).max()) if live.any() else 0.0


def bound(pattern):
    return DEVICE_FACTOR * MODEL_CONSTANT[pattern]


def model_ratio(case, pattern):
    rows, norm, w = rows_of(case), case.p["normalized"], upstream_of(case, pattern)
    g, A = reference(rows, norm, w)
    return ratio(model(rows, norm, w), g, A)
