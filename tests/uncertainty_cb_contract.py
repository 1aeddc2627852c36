"""Contract of the batch-innermost uncertainty reduction (csrc/mc_uncertainty.hip: bbb_mc_uncertainty_cb, ops.mc_uncertainty_cb) for
tests/test_uncertainty_cb_cpu.py and tests/test_gpu_uncertainty_cb.py, built the way tests/tail_contract.py is and on its recipes: the
named cases, their seeded fp32 logits, float64 references written from the definitions, an fp32 numpy model of the kernel's order of
operations, the error scales and the stored model constants.  No device and no library needed.

The device bound of an output is DEVICE_FACTOR x its constant; the constant is the worst |fp32 model - float64| / scale over all cases,
rounded up to one significant digit (tests/test_uncertainty_cb_cpu.py measures it again and compares).  Nothing here is taken from
kernel output.

Conventions of the reference (include/bbb_hip.h): a term with p = 0 contributes exactly 0 to an entropy and to the KL sum (entr /
xlogy), so a class at -inf gives finite scores; a NaN or +inf logit makes its whole draw NaN, hence every probability output of the image
and its three scores, while pred is non-finite in that class only."""
import numpy as np

from tail_contract import (BATCHES, CLASSES_CB, DEVICE_FACTOR, DRAWS, F32, RECIPES, SOFTPLUS_RECIPE, U, VALID, Case, round_up_1sf)
from tail_contract import rows_of as _recipe_rows

FIELDS = ("pred", "p_mean", "epistemic", "aleatoric", "entropy", "expected_entropy", "mutual_info")
PER_CLASS = FIELDS[:4]
ENTRY = "mc_uncertainty_cb"
EINVAL, EALIGN, ESHAPE = -1, -2, -3
MAX_DRAWS = 202          # (160 KB - 8 KB of row partials) / (3 floats x 64 images) per draw
ROWS = 16                # rows of a block at most
LDS_PER_DRAW, LDS_REDUCE = 768, 8192
NORMALIZED_RECIPES = VALID["uncertainty_normalized"]
INJECTIONS = ("neginf_some", "neginf_all", "nan", "posinf")

# worst |fp32 model - float64 reference| / scale over CASES, rounded up to one significant digit (scales: ratios() below)
MODEL_CONSTANT = {"pred": 4.0, "p_mean": 3.0, "epistemic": 1.0, "aleatoric": 4.0, "entropy": 3.0, "expected_entropy": 3.0,
                  "mutual_info": 3.0}


def _build_cases():
    cases = []

    def add(recipe, T, C, B, normalized=False, tag="", inject=None):
        if recipe == "draw_skew" and T < 2:
            T = 2
        name = "%s-%s-%dx%dx%d%s%s" % (ENTRY, recipe, T, C, B, "-norm" if normalized else "", tag)
        params = (("normalized", normalized),) + ((("inject", inject),) if inject else ())
        cases.append(Case(name, ENTRY, recipe, T, C, B, 0, params))

    for i, r in enumerate(RECIPES):                      # two passes through the size cycles, out of step with each other
        add(r, DRAWS[i % 4], CLASSES_CB[i % 5], BATCHES[i % 6])
        add(r, DRAWS[(i + 2) % 4], CLASSES_CB[(i + 3) % 5], BATCHES[(i + 3) % 6], tag="-b")
    for i, r in enumerate(NORMALIZED_RECIPES + (SOFTPLUS_RECIPE,) * 3):
        add(r, DRAWS[(i + 1) % 4], CLASSES_CB[(i + 2) % 5], BATCHES[(i * 5 + 1) % 6], True, "-%d" % i)
    # boundaries: one draw, one class, a block of one row, a batch of one block exactly, the largest T the plan admits
    add("dominant", 1, 10, 65, tag="-T1")
    add(SOFTPLUS_RECIPE, 1, 10, 65, True, "-T1")
    add("gauss4", 10, 1, 63, tag="-C1")
    add("gauss4", 17, 1, 3, True, "-C1")
    add("gauss4", 1, 1, 1, tag="-row1")
    add("gauss4", 10, 17, 64, tag="-B64")
    add("gauss4", MAX_DRAWS, 3, 4, tag="-maxT")
    add("gauss4", MAX_DRAWS, 3, 4, True, "-maxT")
    for inj in INJECTIONS:
        add("gauss4", 10, 7, 65, tag="-" + inj, inject=inj)
    add("gauss4", 10, 7, 65, True, "-neginf_some", inject="neginf_some")
    return tuple(cases)


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def rows_of(case):
    """Seeded fp32 logits [T][B][C] of the recipe, then the case's injection:
    neginf_some: class 2 of every other image at -inf in draws 0, 3 and 4;   neginf_all: class b % C of every third image at -inf in
    every draw;   nan / posinf: one logit of images 5 and 64 (the second block), in draws 1 and 2."""
    x = _recipe_rows(case).copy()
    inj = case.p.get("inject")
    b = np.arange(case.B)
    if inj == "neginf_some":
        x[np.ix_([0, 3, 4], b[::2], [2])] = -np.inf
    elif inj == "neginf_all":
        x[:, b[::3], b[::3] % case.C] = -np.inf
    elif inj in ("nan", "posinf"):
        x[1, 5, 3] = x[2, 64, 0] = np.nan if inj == "nan" else np.inf
    else:
        assert inj is None
    return x


# ------------------------------------------------------------------------------------------------ float64 reference
def _xlogy(p, logq):
    """p * logq with the term exactly 0 where p == 0 (NaN p stays NaN)."""
    with np.errstate(invalid="ignore"):
        return np.where(p == 0, 0.0, p * logq)


def probs64(rows, normalized):
    """(p, log p), each [T][B][C] float64."""
    z = np.asarray(rows, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if normalized:
            sp = np.where(z > 20, z, np.log1p(np.exp(np.minimum(z, 20))))
            tot = sp.sum(axis=2, keepdims=True)
            return sp / tot, np.log(sp) - np.log(tot)
        ls = z - z.max(axis=2, keepdims=True)
        ls = ls - np.log(np.exp(ls).sum(axis=2, keepdims=True))
        return np.exp(ls), ls


def reference(rows, normalized):
    """{field: float64 array} from the definitions; mutual_info in its KL form and NOT clamped."""
    z = np.asarray(rows, np.float64)
    p, lp = probs64(rows, normalized)
    with np.errstate(invalid="ignore", divide="ignore"):
        pbar = p.mean(axis=0)
        lpbar = np.log(pbar)
        kl = np.where((p == 0) | (pbar[None] == 0), 0.0, p * (lp - lpbar[None]))
        return {"pred": z.mean(axis=0), "p_mean": pbar, "epistemic": ((p - pbar[None]) ** 2).mean(axis=0),
                "aleatoric": pbar - (p ** 2).mean(axis=0), "entropy": -_xlogy(pbar, lpbar).sum(axis=1),
                "expected_entropy": -_xlogy(p, lp).sum(axis=2).mean(axis=0), "mutual_info": kl.sum(axis=2).mean(axis=0)}


def entropy_difference(ref):
    """entropy - expected_entropy of a reference: equals its mutual_info in exact arithmetic."""
    return ref["entropy"] - ref["expected_entropy"]


# ------------------------------------------------------------------------------------------------ fp32 model of the kernel
def _comp_sum(terms):
    """Compensated running sum over the LAST axis, in fp32, in the kernel's order."""
    s = np.zeros(terms.shape[:-1], F32)
    c = np.zeros(terms.shape[:-1], F32)
    with np.errstate(invalid="ignore"):
        for k in range(terms.shape[-1]):
            y = terms[..., k] - c
            t = s + y
            c = (t - s) - y
            s = t
    return s


def _softplus32(v):
    return np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, F32(20))))).astype(F32)


def model(rows, normalized):
    """mc_uncertainty_cb_kernel in fp32 numpy: {field: float32 array}."""
    v = np.asarray(rows, F32)
    T, B, C = v.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if normalized:
            q = _softplus32(v)
            a = _comp_sum(q)
            lz = np.log(a)
            ls = np.log(q) - lz[..., None]
            p = q / a[..., None]
        else:
            a = np.fmax.reduce(v, axis=2)                                    # fmaxf skips a NaN
            lz = np.log(_comp_sum(np.exp(v - a[..., None])))
            ls = (v - a[..., None]) - lz[..., None]
            p = np.exp(ls)
        assert ls.dtype == F32 and p.dtype == F32
        h = -_comp_sum(np.where(p == 0, F32(0), p * ls))                     # [T][B]
        s_v, s_p, s_p2 = (np.zeros((B, C), F32) for _ in range(3))
        for t in range(T):
            s_v, s_p, s_p2 = s_v + v[t], s_p + p[t], s_p2 + p[t] * p[t]
        fT = F32(T)
        pbar = s_p / fT
        lpbar = np.log(pbar)
        s_d2, s_kl = np.zeros((B, C), F32), np.zeros((B, C), F32)
        for t in range(T):
            d = p[t] - pbar
            s_d2 = s_d2 + d * d
            s_kl = s_kl + np.where((p[t] == 0) | (pbar == 0), F32(0), p[t] * (ls[t] - (ls[t] if T == 1 else lpbar)))
        ent_c = np.where(pbar == 0, F32(0), pbar * lpbar)
        ny = min(ROWS, max(T, C))
        e, m = np.zeros(B, F32), np.zeros(B, F32)
        for r in range(ny):                                                  # a row's classes compensated, the rows in ascending order
            e = e + _comp_sum(ent_c[:, r::ny])
            m = m + _comp_sum(s_kl[:, r::ny])
        eh = np.zeros(B, F32)
        for t in range(T):
            eh = eh + h[t]
        m = m / fT
        out = {"pred": s_v / fT, "p_mean": pbar, "epistemic": s_d2 / fT, "aleatoric": pbar - s_p2 / fT, "entropy": -e,
               "expected_entropy": eh / fT, "mutual_info": np.where(m < 0, F32(0), m)}
    assert all(o.dtype == F32 for o in out.values())
    return out


# ------------------------------------------------------------------------------------------------ error scales
def scales(rows):
    """{field: scale}: pred 2^-24 x the image's largest finite |logit| (uncertainty_ratios), p_mean / epistemic / aleatoric 2^-24,
    the three entropy scores 2^-24 (1 + ln C)."""
    r = np.asarray(rows, np.float64)
    C = r.shape[2]
    row_max = np.where(np.isfinite(r), np.abs(r), 0.0).max(axis=(0, 2))[:, None]
    s = {"pred": U * row_max, "p_mean": U, "epistemic": U, "aleatoric": U}
    s.update({f: U * (1.0 + np.log(C)) for f in FIELDS[4:]})
    return s


def field_ratio(field, got, ref, rows):
    """Worst |got - ref| / scale of one output over the elements where the reference is finite.  Where it is NaN the value must be NaN,
    where it is infinite the same infinity -- at exactly those positions and nowhere else."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (field, got.shape, ref.shape)
    assert (np.isnan(got) == np.isnan(ref)).all(), field + ": NaN positions differ from the reference's"
    inf = np.isinf(ref)
    assert (np.isinf(got) == inf).all() and (got[inf] == ref[inf]).all(), field + ": infinities differ from the reference's"
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    sc = np.broadcast_to(scales(rows)[field], ref.shape)
    return float((np.abs(got[fin] - ref[fin]) / sc[fin]).max())


def ratios(got, ref, rows, fields=FIELDS):
    return {f: field_ratio(f, got[f], ref[f], rows) for f in fields}


def bound(field):
    return DEVICE_FACTOR * MODEL_CONSTANT[field]


def model_ratios(case):
    rows = rows_of(case)
    return ratios(model(rows, case.p["normalized"]), reference(rows, case.p["normalized"]), rows)

