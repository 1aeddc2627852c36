"""Contract of the Monte-Carlo tail, loss and uncertainty kernels (csrc/mc_tail.hip) for tests/test_tail_sweep_cpu.py and
tests/test_gpu_tail_sweep.py: the named cases, their seeded fp32 logits, float64 references written from the definitions, fp32 numpy
models of each operation in the max-first order ls = (v - mx) - log(se) and, for contrast, in the order the kernels had before
(ls = v - (mx + log(se))), the shift-invariant error scales and the stored model constants.  No device and no library needed.

The device bound of an operation is DEVICE_FACTOR x its constant; the constant is the worst |max-first model - float64| / scale over
all cases, rounded up to one significant digit (tests/test_tail_sweep_cpu.py measures it again and compares).  Nothing here is taken
from kernel output."""
import dataclasses
import math
import zlib

import numpy as np

F32 = np.float32
U = 2.0 ** -24
DEVICE_FACTOR = 4        # device expf / logf a few ulp where numpy is close to correctly rounded; another summation order over <= 1024 classes

# worst |max-first fp32 model - float64 reference| / scale over CASES, rounded up to one significant digit (scales: see *_ratio below)
MODEL_CONSTANT = {"tail": 8.0, "tail_grad": 20.0, "elbo_loss": 4.0, "elbo_grad": 30.0, "pred": 4.0, "epi": 0.9, "ale": 3.0}

EINVAL, EALIGN, ESHAPE = -1, -2, -3
MAX_PER_SLICE = 640      # draws one image reduces over: 640 x 64 images x 4 bytes = the 160 KB of LDS of a workgroup
MAX_CB_DRAWS = 512       # ops.mc_tail_cb and the autograd entries
MAX_UNITS = 4096

TAIL_ENTRIES = ("mc_tail", "mc_tail_cb", "mc_tail_units", "mc_tail_groups", "mc_tail_share", "step_end")
ENTRIES = TAIL_ENTRIES + ("mc_tail_cb_autograd", "elbo_cb_autograd", "uncertainty")
OFFSETS = (100.0, -100.0, 1000.0, -1000.0, 1e4)
RECIPES = ("gauss0.01", "gauss4", "gauss30") + tuple("offset%+g" % o for o in OFFSETS) + ("dominant", "ties", "draw_skew")
SOFTPLUS_RECIPE = "softplus_range"
VALID = {e: RECIPES for e in ENTRIES}
# normalized=True: softplus(v) / sum softplus(v) -- a row of very negative logits has no finite float64 value, so only bounded recipes
VALID["uncertainty_normalized"] = (SOFTPLUS_RECIPE, "gauss0.01", "gauss4", "ties")

BATCHES = (1, 3, 63, 64, 65, 130)
DRAWS = (1, 2, 10, 17)
CLASSES_BC = (1, 10, 63, 64, 65, 257, 1024)        # mc_tail, uncertainty: [E][B][C], 64 lanes x 16 classes
CLASSES_CB = (1, 7, 10, 17, 100)                   # batch-innermost entries
UNITS = ((4, 0, 8), (4, 1, 5), (4, 3, 2), (4, 6, 3), (5, 2, 1), (1, 0, 10))      # (slices, unit_off, units)
GROUPS = ((1, 1), (4, 10), (16, 1), (3, 7))                                      # (groups, draws)
SHARES = ((3, 4, 0, 12), (3, 4, 1, 9), (3, 4, 3, 5), (2, 10, 9, 2), (4, 3, 2, 1))  # (steps, draws, first_off, slabs)
LARGE_E = ((257, 3, 4), (512, 3, 4))               # mc_tail_cb (E, C, B): 64.25 KB and 128 KB of LDS
# the rule between the kernel's two ways to the row maxima (csrc/mc_tail_plan.h: kept in LDS up to 320 draws, found again beyond): the
# last launch that keeps them (160 KB) and the first that does not, the latter with more classes than one sweep of phase 2 takes (64)
KEEP_MAX_EDGE = ((320, 3, 4), (321, 100, 3))


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    entry: str
    recipe: str
    slabs: int            # leading dimension of the logits: draws, units or slabs
    C: int
    B: int                # images per slab
    mean_over: int = 0
    params: tuple = ()    # entry-specific (key, value) pairs

    @property
    def p(self):
        return dict(self.params)

    @property
    def seed(self):
        return zlib.crc32(self.name.encode())

    @property
    def batch_innermost(self):
        return self.entry not in ("mc_tail", "uncertainty")


def _form_params(form, i):
    """(params, slabs) of tail form `form`, the i-th of its parameter sets."""
    if form == "mc_tail_units":
        S, off, n = UNITS[i % len(UNITS)]
        return (("form", form), ("S", S), ("off", off)), n
    if form == "mc_tail_groups":
        G, E = GROUPS[i % len(GROUPS)]
        return (("form", form), ("G", G), ("E", E)), G * E
    steps, draws, first_off, n = SHARES[i % len(SHARES)]
    return (("form", form), ("steps", steps), ("draws", draws), ("first_off", first_off)), n


def _form_params_for(form, i, recipe):
    """draw_skew needs two slabs: the next parameter set that has them."""
    while recipe == "draw_skew" and _form_params(form, i)[1] < 2:
        i += 1
    return _form_params(form, i)


def _build_cases():
    cases = []

    def add(entry, recipe, slabs, C, B, mean_over=0, params=(), tag=""):
        if recipe == "draw_skew" and slabs < 2:
            assert not params or params[0][0] != "form"
            slabs = 2
        name = "%s-%s-%dx%dx%d%s" % (entry, recipe, slabs, C, B, tag)
        cases.append(Case(name, entry, recipe, slabs, C, B, mean_over if mean_over >= 0 else slabs, tuple(params)))

    for i, r in enumerate(RECIPES):
        E, B = DRAWS[i % 4], BATCHES[i % 6]
        add("mc_tail", r, E, CLASSES_BC[i % 7], B, -(i % 2))
        add("mc_tail_cb", r, DRAWS[(i + 1) % 4], CLASSES_CB[i % 5], BATCHES[(i + 2) % 6], -((i + 1) % 2))
        prm, n = _form_params_for("mc_tail_units", i, r)
        add("mc_tail_units", r, n, CLASSES_CB[(i + 1) % 5], BATCHES[(i + 3) % 6], (i % 2) * 3, prm, "-S%do%d" % (prm[1][1], prm[2][1]))
        prm, n = _form_params_for("mc_tail_groups", i, r)
        add("mc_tail_groups", r, n, CLASSES_CB[(i + 2) % 5], BATCHES[(i + 4) % 6], (i % 2) * prm[2][1], prm, "-G%d" % prm[1][1])
        prm, n = _form_params_for("mc_tail_share", i, r)
        add("mc_tail_share", r, n, CLASSES_CB[(i + 3) % 5], BATCHES[(i + 5) % 6], 0, prm, "-s%dd%df%d" % tuple(v for _, v in prm[1:]))
        form = ("mc_tail_units", "mc_tail_groups", "mc_tail_share")[i % 3]
        prm, n = _form_params_for(form, i + 2, r)
        step = (("kl", 1234.5 + i), ("scale", float(1 + i % 5)), ("counter0", (0, 7, 2 ** 31 - 3, -5)[i % 4]), ("add", (1, 20, 2 ** 32 - 1)[i % 3]))
        add("step_end", r, n, CLASSES_CB[(i + 4) % 5], BATCHES[i % 6], 0, prm + step, "-" + form[8:] + str(i))
        add("mc_tail_cb_autograd", r, DRAWS[(i + 2) % 4], CLASSES_CB[(i + 2) % 5], BATCHES[(i + 1) % 6], -(i % 2))
        for dev in (False, True):
            k = i + (3 if dev else 0)
            add("elbo_cb_autograd", r, DRAWS[(k + 3) % 4], CLASSES_CB[(k + 3) % 5], BATCHES[(k + 3) % 6], -1,
                (("beta", 0.37 if dev else 0.1), ("beta_dev", dev), ("kl", 4321.0 + i), ("train_size", 50000.0)), "-dev" if dev else "-host")
        add("uncertainty", r, DRAWS[(i + 1) % 4], CLASSES_BC[(i + 3) % 7], BATCHES[(i + 1) % 6], 0, (("normalized", False),))
    for i, r in enumerate(VALID["uncertainty_normalized"] + (SOFTPLUS_RECIPE,) * 3):
        add("uncertainty", r, DRAWS[i % 4], CLASSES_BC[(i * 2) % 7], BATCHES[(i * 5 + 2) % 6], 0, (("normalized", True),), "-norm%d" % i)
    # boundaries no cycle above reaches: ny = 1, a batch of one block exactly with 1024 classes, T = 1 on confident rows
    add("mc_tail_cb", "gauss4", 1, 1, 1, 0, (), "-ny1")
    add("mc_tail", "gauss4", 2, 1024, 64, -1, (), "-lanes")
    add("uncertainty", "dominant", 1, 65, 3, 0, (("normalized", False),), "-T1")
    add("uncertainty", SOFTPLUS_RECIPE, 1, 10, 65, 0, (("normalized", True),), "-T1")
    return tuple(cases)


CASES = _build_cases()
# added only once the launch plan asks for (and checks) the LDS they need: more than the 64 KB a kernel gets unasked
LARGE_CASES = tuple(Case("mc_tail_cb-gauss4-%dx%dx%d-lds" % s, "mc_tail_cb", "gauss4", s[0], s[1], s[2], s[0]) for s in LARGE_E)
EDGE_CASES = tuple(Case("mc_tail_cb-gauss4-%dx%dx%d-keepmax" % s, "mc_tail_cb", "gauss4", s[0], s[1], s[2], s[0]) for s in KEEP_MAX_EDGE)
ALL_CASES = CASES + LARGE_CASES + EDGE_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


def op_key(case):
    """Recipe table the case belongs to."""
    return "uncertainty_normalized" if case.entry == "uncertainty" and case.p["normalized"] else case.entry


# ------------------------------------------------------------------------------------------------ logits
def rows_of(case):
    """Seeded fp32 logits [slabs][B][C] (draw, image, class)."""
    rng = np.random.default_rng(case.seed)
    n, B, C, r = case.slabs, case.B, case.C, case.recipe
    z = rng.standard_normal((n, B, C))
    if r.startswith("gauss"):
        x = float(r[5:]) * z
    elif r.startswith("offset"):
        x = 4.0 * z + float(r[6:])
    elif r == "dominant":                        # one class 40 above the rest in every draw, another class for each image
        x = z.copy()
        x[:, np.arange(B), (np.arange(B) * 3 + 1) % C] += 40.0
    elif r == "ties":
        x = np.full((n, B, C), 1.5)
    elif r == "draw_skew":                       # every draw but one holds class k(b) of image b 80 below: that one draw's
        x = 4.0 * z                              # log-probability there is ~80 above the others', and it is not the first
        k = (np.arange(B) * 7) % C
        low = np.zeros((n, B, C))
        low[:, np.arange(B), k] = -80.0
        low[n // 2] = 0.0
        x = x + low
    elif r == SOFTPLUS_RECIPE:                   # both branches of softplus (v > 20), no row without a finite normaliser
        x = rng.uniform(-30.0, 40.0, (n, B, C))
    else:
        raise KeyError(r)
    return np.ascontiguousarray(x.astype(F32))


def layout(case, rows):
    """The array the entry takes: [slabs][B][C] or batch-innermost [slabs][C][B]."""
    return np.ascontiguousarray(rows.transpose(0, 2, 1)) if case.batch_innermost else rows


def targets_of(case):
    """int64 targets [B]; with three images or more the first and the last lie outside [0, C)."""
    t = np.random.default_rng(case.seed + 1).integers(0, case.C, case.B).astype(np.int64)
    if case.B >= 3:
        t[0], t[-1] = -1, case.C
    return t


def upstream_of(case):
    """fp32 weights [B][C] of the scalar sum(w * lse) whose gradient the tail's backward is asked for."""
    return np.random.default_rng(case.seed + 2).standard_normal((case.B, case.C)).astype(F32)


# ------------------------------------------------------------------------------------------------ which slabs a block reduces over
def blocks_of(case):
    """Per output block of B images: the slab indices it reduces over, from the docstrings of ops.mc_tail_units / _groups / _share."""
    p, n = case.p, case.slabs
    form = p.get("form", case.entry)
    if form == "mc_tail_units":        # unit u = off + e is batch slice u % S
        S, off = p["S"], p["off"]
        return [list(range((s - off) % S, n, S)) for s in range(S)]
    if form == "mc_tail_groups":       # slab g * E + j = draw j of step g
        return [list(range(g * p["E"], (g + 1) * p["E"])) for g in range(p["G"])]
    if form == "mc_tail_share":        # slab e = draw first_off + e of the draw-major (step, draw) enumeration
        d, f = p["draws"], p["first_off"]
        return [list(range(max(k * d - f, 0), min((k + 1) * d - f, n))) for k in range(p["steps"])]
    return [list(range(n))]


def blocks_brute_force(case):
    """The same by visiting every slab and asking which block it belongs to."""
    p, form = case.p, case.p.get("form", case.entry)
    nblk = {"mc_tail_units": p.get("S"), "mc_tail_groups": p.get("G"), "mc_tail_share": p.get("steps")}.get(form, 1)
    out = [[] for _ in range(nblk)]
    for e in range(case.slabs):
        if form == "mc_tail_units":
            out[(p["off"] + e) % p["S"]].append(e)
        elif form == "mc_tail_groups":
            out[e // p["E"]].append(e)
        elif form == "mc_tail_share":
            out[(p["first_off"] + e) // p["draws"]].append(e)
        else:
            out[0].append(e)
    return out


# ------------------------------------------------------------------------------------------------ float64 references
def log_softmax64(rows):
    z = np.asarray(rows, np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


def tail_ref(rows, blocks, mean_over=0):
    """[len(blocks) * B][C] float64: logsumexp over each block's slabs of the per-draw log_softmax, minus log(mean_over); -inf where a
    block holds no slab."""
    ls = log_softmax64(rows)
    out = []
    for idx in blocks:
        if not idx:
            out.append(np.full(ls.shape[1:], -np.inf))
            continue
        a = ls[idx]
        m = a.max(axis=0)
        out.append(m + np.log(np.exp(a - m).sum(axis=0)) - (math.log(mean_over) if mean_over > 0 else 0.0))
    return np.concatenate(out, axis=0)


def _torch_tail(t, mean_over):
    import torch
    return torch.logsumexp(torch.log_softmax(t, dim=2), dim=0) - (math.log(mean_over) if mean_over > 0 else 0.0)


def tail_grad_ref(rows, w, mean_over):
    """float64 autograd: d sum(w * lse) / d logits, [E][B][C]."""
    import torch
    t = torch.from_numpy(np.asarray(rows, np.float64)).requires_grad_(True)
    (_torch_tail(t, mean_over) * torch.from_numpy(np.asarray(w, np.float64))).sum().backward()
    return t.grad.numpy()


def elbo_ref(rows, target, kl, beta, train_size, mean_over):
    """float64 autograd of loss = nll_loss(lse, target) * train_size + beta * kl -> (loss, d loss / d logits [E][B][C], d loss / d kl).
    nll_loss here: -(1 / B) sum over the images whose target lies in [0, C) of lse[b][target[b]] -- the others contribute nothing and
    the mean still divides by B.  (NOT the ignore_index mean of F.nll_loss, which divides by the number of images kept.)"""
    import torch
    t = torch.from_numpy(np.asarray(rows, np.float64)).requires_grad_(True)
    k = torch.tensor(float(kl), dtype=torch.float64, requires_grad=True)
    lse = _torch_tail(t, mean_over)
    B, C = lse.shape
    keep = np.flatnonzero((target >= 0) & (target < C))
    loss = -(lse[keep, target[keep]].sum() / B) * float(train_size) + float(beta) * k
    loss.backward()
    return float(loss.detach()), t.grad.numpy(), float(k.grad)


def uncertainty_ref(rows, normalized):
    """oracle/bbb_numpy.uncertainty without its casts to fp32: (pred, epistemic, aleatoric), each [B][C] float64."""
    z = np.asarray(rows, np.float64)
    if normalized:
        sp = np.where(z > 20, z, np.log1p(np.exp(np.minimum(z, 20))))
        p = sp / sp.sum(axis=2, keepdims=True)
    else:
        e = np.exp(z - z.max(axis=2, keepdims=True))
        p = e / e.sum(axis=2, keepdims=True)
    pbar = p.mean(axis=0)
    return z.mean(axis=0), ((p - pbar[None]) ** 2).mean(axis=0), pbar - (p ** 2).mean(axis=0)


# ------------------------------------------------------------------------------------------------ fp32 models
def log_softmax_model(rows, order):
    """fp32 per-draw log_softmax: "max_first" = (v - mx) - log(se), "present" = v - (mx + log(se)), se = sum exp(v - mx) in both."""
    v = np.asarray(rows, F32)
    mx = v.max(axis=-1, keepdims=True)
    se = np.exp(v - mx).sum(axis=-1, keepdims=True, dtype=F32)
    if order == "max_first":
        return (v - mx) - np.log(se)
    assert order == "present"
    return v - (mx + np.log(se))


def _sub32(mean_over):
    return np.log(F32(mean_over)) if mean_over > 0 else F32(0)


def tail_model(rows, blocks, mean_over=0, order="max_first"):
    """The kernels' online (max, sum) pair carried over the draws, in fp32."""
    ls = log_softmax_model(rows, order)
    out = []
    with np.errstate(invalid="ignore"):
        for idx in blocks:
            if not idx:
                out.append(np.full(ls.shape[1:], -np.inf, F32))
                continue
            m, s = np.full(ls.shape[1:], -np.inf, F32), np.zeros(ls.shape[1:], F32)
            for e in idx:
                nm = np.maximum(m, ls[e])
                s = s * np.where(np.isinf(m), F32(0), np.exp(m - nm)) + np.exp(ls[e] - nm)
                m = nm
            out.append((m + np.log(s)) - _sub32(mean_over))
    res = np.concatenate(out, axis=0)
    assert res.dtype == F32
    return res


def tail_grad_model(rows, w, mean_over, order="max_first"):
    """bbb_mc_tail_cb_bwd in fp32: H = g exp(ls - (lse + log mean_over)), d logits = H - exp(ls) sum_c H."""
    ls = log_softmax_model(rows, order)
    lse = tail_model(rows, [list(range(ls.shape[0]))], mean_over, order)
    h = np.asarray(w, F32)[None] * np.exp(ls - (lse + _sub32(mean_over))[None])
    g = h - np.exp(ls) * h.sum(axis=-1, keepdims=True, dtype=F32)
    assert g.dtype == F32
    return g


def elbo_model(rows, target, kl, beta, train_size, mean_over, order="max_first"):
    """bbb_elbo_cb_fwd / _bwd in fp32 with an upstream gradient of one -> (loss, d logits, d kl)."""
    ls = log_softmax_model(rows, order)
    E, B, C = ls.shape
    lse = tail_model(rows, [list(range(E))], mean_over, order)
    keep = np.flatnonzero((target >= 0) & (target < C))
    acc = lse[keep, target[keep]].sum(dtype=F32)
    loss = (-acc / F32(B)) * F32(train_size) + F32(beta) * F32(kl)
    gscale = F32(train_size) / F32(B)
    g = np.zeros_like(ls)
    h = -gscale * np.exp(ls[:, keep, target[keep]] - (lse[keep, target[keep]] + _sub32(mean_over))[None])       # [E][keep]
    g[:, keep, :] = -np.exp(ls[:, keep, :]) * h[:, :, None]
    g[:, keep, target[keep]] += h
    assert g.dtype == F32
    return F32(loss), g, F32(beta)


def uncertainty_model(rows, normalized):
    """uncertainty_kernel in fp32: two passes over the draws, p_hat = q * (1 / z)."""
    v = np.asarray(rows, F32)
    T = v.shape[0]
    if normalized:
        q = np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, F32(20)))))
    else:
        q = np.exp(v - v.max(axis=2, keepdims=True))
    ph = (q * (F32(1) / q.sum(axis=2, keepdims=True, dtype=F32))).astype(F32)
    s_l, s_p, s_p2, s_d2 = (np.zeros(v.shape[1:], F32) for _ in range(4))
    for t in range(T):
        s_l, s_p, s_p2 = s_l + v[t], s_p + ph[t], s_p2 + ph[t] * ph[t]
    s_p = s_p / F32(T)
    for t in range(T):
        d = ph[t] - s_p
        s_d2 = s_d2 + d * d
    out = s_l / F32(T), s_d2 / F32(T), s_p - s_p2 / F32(T)
    assert all(o.dtype == F32 for o in out)
    return out


# ------------------------------------------------------------------------------------------------ error scales (all shift-invariant)
def tail_ratio(got, ref):
    """Worst |got - ref| / (2^-24 (1 + |ref|)) over EVERY element; where the reference is -inf the value must be -inf, at exactly
    those positions."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    hole = np.isneginf(ref)
    assert not np.isnan(ref).any() and not hole.all() and not np.isposinf(ref).any()
    assert (np.isneginf(got) == hole).all(), "-inf rows differ from the reference's"
    assert np.isfinite(got[~hole]).all(), "non-finite value where the reference is finite"
    return float((np.abs(got[~hole] - ref[~hole]) / (U * (1.0 + np.abs(ref[~hole])))).max())


def grad_ratio(got, g64):
    """Worst |got - g64| / (2^-24 max |g64|) of one case; a reference that is zero everywhere asks for exact zeros."""
    got, g64 = np.asarray(got, np.float64), np.asarray(g64, np.float64)
    assert got.shape == g64.shape and np.isfinite(got).all() and np.isfinite(g64).all()
    scale = float(np.abs(g64).max())
    if scale == 0.0:                     # one class: log_softmax is the constant 0 and every gradient exactly 0
        assert not got.any()
        return 0.0
    return float(np.abs(got - g64).max() / (U * scale))


def loss_ratio(got, ref):
    assert np.isfinite(got) and np.isfinite(ref) and ref != 0
    return abs(float(got) - ref) / (U * abs(ref))


def uncertainty_ratios(got, ref, rows):
    """(pred, epi, ale): pred against 2^-24 x the largest |logit| of the image (over draws and classes), epi and ale against 2^-24."""
    pred, epi, ale = (np.asarray(g, np.float64) for g in got)
    assert all(np.isfinite(g).all() and g.shape == r.shape for g, r in zip((pred, epi, ale), ref))
    row_max = np.abs(np.asarray(rows, np.float64)).max(axis=(0, 2))[:, None]
    return (float((np.abs(pred - ref[0]) / (U * row_max)).max()), float(np.abs(epi - ref[1]).max() / U), float(np.abs(ale - ref[2]).max() / U))


def bound(op):
    return DEVICE_FACTOR * MODEL_CONSTANT[op]


def round_up_1sf(x):
    d = 10.0 ** math.floor(math.log10(x))
    return round(math.ceil(x / d - 1e-12) * d, 12)


def model_ratios(case, order="max_first"):
    """{operation: |fp32 model - float64| / scale} of one case; also asserts the reference holds no NaN."""
    rows = rows_of(case)
    p = case.p
    if case.entry in TAIL_ENTRIES:
        blocks = blocks_of(case)
        return {"tail": tail_ratio(tail_model(rows, blocks, case.mean_over, order), tail_ref(rows, blocks, case.mean_over))}
    if case.entry == "mc_tail_cb_autograd":
        w = upstream_of(case)
        full = [list(range(case.slabs))]
        return {"tail": tail_ratio(tail_model(rows, full, case.mean_over, order), tail_ref(rows, full, case.mean_over)),
                "tail_grad": grad_ratio(tail_grad_model(rows, w, case.mean_over, order), tail_grad_ref(rows, w, case.mean_over))}
    if case.entry == "elbo_cb_autograd":
        args = (rows, targets_of(case), p["kl"], p["beta"], p["train_size"], case.mean_over)
        loss, g, gk = elbo_model(*args, order)
        loss64, g64, gk64 = elbo_ref(*args)
        assert float(gk) == float(F32(gk64))
        return {"elbo_loss": loss_ratio(loss, loss64), "elbo_grad": grad_ratio(g, g64)}
    ref = uncertainty_ref(rows, p["normalized"])
    assert not any(np.isnan(r).any() for r in ref)
    return dict(zip(("pred", "epi", "ale"), uncertainty_ratios(uncertainty_model(rows, p["normalized"]), ref, rows)))
