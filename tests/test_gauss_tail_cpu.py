"""CPU-only companions of tests/test_gpu_gauss_tail.py: the contract of the Gaussian-likelihood tail (tests/gauss_tail_contract.py) held
against itself and against torch.  The float64 reference agrees with torch.nn.functional.gaussian_nll_loss where nothing is clamped and
with float64 autograd of train.gaussian_elbo everywhere; the fp32 model's worst error per operation IS the stored constant the device
bound is built from; the library exports the six new entries under ABI 13; the host-only plans refuse in the documented order and give
the documented grid; the plan header walks its argument space under the address and undefined-behaviour sanitizers (a stand-alone
program, nothing loaded into Python); and forward_loss(likelihood=...) on a CPU model raises the usual device error.  No device; the
library is only loaded, never launched."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import gauss_tail_contract as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
NAMES = ("bbb_gauss_elbo_cb_fwd", "bbb_gauss_elbo_cb_bwd", "bbb_gauss_moments_cb", "bbb_gauss_elbo_cb_fwd_plan",
         "bbb_gauss_elbo_cb_bwd_plan", "bbb_gauss_moments_cb_plan")


@pytest.fixture(scope="module")
def refs():
    """{case name: (logits, y, float64 reference)}, computed once."""
    out = {}
    for c in K.CASES:
        logits, y = K.inputs(c)
        out[c.name] = (logits, y, K.reference(c, logits, y))
    return out


def _lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def _lik(c):
    from bbb_hip import train
    return train.GaussianLikelihood(noise_sigma=c.noise_sigma, log_var_min=c.log_var_min, log_var_max=c.log_var_max, mc=c.mc)


def test_case_table_covers_the_sizes_forms_and_recipes():
    own = [c for c in K.CASES if (c.E, c.D, c.B) != K.LARGE_E]
    assert {c.B for c in own} == set(K.BATCHES) and {c.E for c in own} == set(K.DRAWS) and {c.D for c in own} == set(K.DIMS)
    assert [(c.E, c.D, c.B) for c in K.CASES if c not in own] == [K.LARGE_E]
    assert {c.noise_sigma for c in K.CASES} == set(K.SIGMAS) | {None}
    for r in K.RECIPES:
        mine = [c for c in K.CASES if c.recipe == r]
        assert {c.noise_sigma is None for c in mine} == {True, False} and {c.mc for c in mine} == set(K.MODES), r
        assert {c.mean_over for c in mine} == set(K.MEAN_OVER) and {c.beta_dev for c in mine} == {True, False}, r
    assert any(c.D > K.TILE for c in K.CASES) and any(c.D == K.TILE // 2 for c in K.CASES)       # both ways of staging y
    assert any(c.B > K.THREADS for c in K.CASES)                                                 # more than one block
    for c in K.CASES:
        logits, y = K.inputs(c)
        assert logits.dtype == y.dtype == np.float32 and logits.shape == (c.E, c.C, c.B) and y.shape == (c.B, c.D)
        again = K.inputs(c)
        assert np.array_equal(again[0], logits) and np.array_equal(again[1], y)
    edges = next(c for c in K.CASES if c.recipe == "clamp_edges" and c.noise_sigma is None and c.E * c.D * c.B > 50)
    s = K.inputs(edges)[0][:, edges.D:]
    assert (s == edges.log_var_min).any() and (s == edges.log_var_max).any() and (s < edges.log_var_min).any() and (s > edges.log_var_max).any()


def test_reference_is_torch_gaussian_nll_where_nothing_is_clamped(refs):
    import torch.nn.functional as F
    seen = 0
    for c in K.CASES:
        logits, y, ref = refs[c.name]
        X = torch.from_numpy(logits).double()
        mu = X[:, :c.D]
        s = X[:, c.D:] if c.noise_sigma is None else torch.full_like(mu, 2.0 * math.log(c.noise_sigma))
        if bool(((s < c.log_var_min) | (s > c.log_var_max)).any()):
            continue
        seen += 1
        nll = F.gaussian_nll_loss(mu, torch.from_numpy(y).double().t().expand_as(mu), torch.exp(s), full=True, eps=0.0, reduction="none")
        L = -nll.sum(dim=1).numpy()
        assert (np.abs(L - ref["L"]) <= 1e-13 * (0.5 * (K.LOG_2PI + s.abs().numpy() + ((torch.from_numpy(y).double().t() - mu) ** 2
                                                                                      * torch.exp(-s)).numpy())).sum(axis=1)).all(), c.name
    assert seen >= 30


def test_gaussian_elbo_in_float64_is_the_reference_with_its_gradient(refs):
    _lib()
    from bbb_hip import train
    for c in K.CASES:
        logits, y, ref = refs[c.name]
        X = torch.from_numpy(logits).double().requires_grad_(True)
        kl = torch.tensor(c.kl, dtype=torch.float64, requires_grad=True)
        loss, LL = train.gaussian_elbo(X, torch.from_numpy(y).double(), kl, c.beta, c.train_size, _lik(c), c.mean_over)
        loss.backward(torch.tensor(c.g, dtype=torch.float64))
        sc = ref["scale"]
        assert (np.abs(LL.detach().numpy() - ref["LL"]) <= 1e-13 * sc["LL"]).all(), c.name
        assert abs(loss.item() - float(ref["loss"])) <= 1e-13 * float(sc["loss"]) * max(1, c.B), c.name
        err = np.abs(X.grad.numpy() - ref["g_logits"])
        assert (err <= 1e-12 * sc["g_logits"]).all(), (c.name, float((err / np.maximum(sc["g_logits"], 1e-300)).max()))
        assert abs(kl.grad.item() - float(ref["g_kl"])) <= 1e-15, c.name
        if c.E == 1 and c.mean_over == 0:                # the two mc modes agree bit for bit on one draw
            other = K.dataclasses.replace(c, mc="mean" if c.mc == "logmeanexp" else "logmeanexp")
            assert np.array_equal(K.reference(other, logits, y)["LL"], ref["LL"]) and np.array_equal(K.model(other, logits, y)["LL"],
                                                                                                      K.model(c, logits, y)["LL"])


def test_constants_are_the_measured_model_errors(refs):
    worst = {}
    for c in K.CASES:
        logits, y, ref = refs[c.name]
        for f, r in K.ratios(K.model(c, logits, y), ref).items():
            if r > worst.get(f, (-1.0, ""))[0]:
                worst[f] = (r, c.name)
    print("fp32 model, worst |model - float64| / (U scale):", {k: (round(v, 3), n) for k, (v, n) in worst.items()})
    assert set(worst) == set(K.MODEL_CONSTANT) == set(K.FIELDS)
    for f, (r, name) in worst.items():
        assert K.round_up_1sf(r) <= K.MODEL_CONSTANT[f], (f, r, name)          # (the models may be better than stored, never worse)
        assert K.MODEL_CONSTANT[f] == K.round_up_1sf(K.MODEL_CONSTANT[f])
    assert K.DEVICE_FACTOR == 4 and K.bound("LL") == 4 * K.MODEL_CONSTANT["LL"]


def test_model_and_reference_give_exact_zeros_and_keep_a_nan_local(refs):
    for c in K.CASES:
        logits, y, ref = refs[c.name]
        mod = K.model(c, logits, y)
        if c.noise_sigma is None:
            s = logits[:, c.D:]
            out = (s < c.log_var_min) | (s > c.log_var_max)
            assert not ref["g_logits"][:, c.D:][out].any() and not mod["g_logits"][:, c.D:][out].any(), c.name
        if c.recipe == "far_draw" and c.mc == "logmeanexp" and c.noise_sigma is None:      # (s = -10: L near -1e10)
            assert (ref["L"][-1] - ref["L"].max(axis=0) < -1e4).all()
            assert not ref["w"][-1].any() and not mod["g_logits"][-1].any(), c.name
        if c.recipe == "identical":
            assert not ref["epistemic"].any(), c.name
    c = next(c for c in K.CASES if c.noise_sigma is None and c.mc == "logmeanexp" and c.B >= 63 and c.E > 1)
    logits, y, ref = refs[c.name]
    logits, y = logits.copy(), y.copy()
    logits[1, 0, 5] = np.nan
    y[7, c.D - 1] = np.nan
    bad, mod = K.reference(c, logits, y), K.model(c, logits, y)
    hit = np.zeros(c.B, bool)
    hit[[5, 7]] = True
    for out in (bad, mod):
        assert (np.isnan(out["LL"]) == hit).all() and np.isnan(out["loss"])
        assert (np.isnan(out["g_logits"]).any(axis=(0, 1)) == hit).all()
    assert np.array_equal(bad["g_logits"][:, :, ~hit], ref["g_logits"][:, :, ~hit])
    assert K.ratios(mod, bad)["g_logits"] <= K.MODEL_CONSTANT["g_logits"]


def test_library_exports_the_six_entries_under_abi_13():
    lib = _lib()
    h = lib.lib()
    assert lib.ABI_VERSION == 13 and h.bbb_abi_version() == 13
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = " ".join(fh.read().split())
    for name in NAMES:
        assert name in lib.EXPORTS and hasattr(h, name) and f"int {name}(" in header, name
    for phrase in ("draws <= 512, channels <= 1024, batch <= INT32_MAX - 63", "64 x 17 floats = 4352", "#define BBB_ABI_VERSION 13",
                   "never E[mu^2] - mean^2", "RECOMPUTED from the logits"):
        assert phrase in header, phrase
    from bbb_hip import ops, train, ensemble
    assert (ops.GAUSS_MAX_DRAWS, ops.GAUSS_MAX_CHANNELS) == (K.MAX_DRAWS, K.MAX_CHANNELS) and ops.Moments._fields == K.MOMENTS
    assert tuple(ops.GAUSS_MC_CODE) == K.MODES and ensemble.hip_gauss_tail == [True]
    lik = train.GaussianLikelihood()
    assert (lik.noise_sigma, lik.log_var_min, lik.log_var_max, lik.mc) == (None, -20.0, 20.0, "logmeanexp")
    for kw in (dict(noise_sigma=0.0), dict(noise_sigma=float("inf")), dict(log_var_min=1.0, log_var_max=0.0), dict(mc="median")):
        with pytest.raises(lib.BBBHipError):
            train.GaussianLikelihood(**kw)


def test_plans_refuse_in_the_documented_order_and_give_the_grid():
    """Every refusal code of the three host-only plans, and -- through the library loaded on the CPU -- of the launch entries, which
    return before a launch (addresses are only looked at)."""
    h = _lib().lib()
    i32 = ctypes.c_int32
    A = [0x1000 * (k + 1) for k in range(7)]
    good = dict(E=2, B=4, C=6, D=3, sigma=1.0, lo=-20.0, hi=20.0, mc=0, mo=0)

    def call(entry, p, **kw):
        a = dict(good, **kw)
        t, b, l = i32(-7), i32(-7), i32(-7)
        mid = (a["E"], a["B"], a["C"], a["D"], a["sigma"], a["lo"], a["hi"])
        outp = (ctypes.byref(t), ctypes.byref(b), ctypes.byref(l))
        if entry == "fwd":
            rc = h.bbb_gauss_elbo_cb_fwd_plan(p[0], p[1], p[2], p[3], *mid, a["mc"], a["mo"], p[4], p[5], *outp)
            launch = lambda: h.bbb_gauss_elbo_cb_fwd(p[0], p[1], p[2], 0.1, p[3], 100.0, *mid, a["mc"], a["mo"], p[4], p[5], None)
        elif entry == "bwd":
            rc = h.bbb_gauss_elbo_cb_bwd_plan(p[0], p[1], p[2], p[3], *mid, a["mc"], a["mo"], p[4], p[5], *outp)
            launch = lambda: h.bbb_gauss_elbo_cb_bwd(p[0], p[1], p[2], 0.1, p[3], 100.0, *mid, a["mc"], a["mo"], p[4], p[5], None)
        else:
            rc = h.bbb_gauss_moments_cb_plan(p[0], p[1], *mid, *p[2:7], *outp)
            launch = lambda: h.bbb_gauss_moments_cb(p[0], p[1], *mid, *p[2:7], None)
        if rc != 0:
            assert (t.value, b.value, l.value) == (0, 0, 0)
            assert launch() == rc                                    # refused: nothing is launched
        return rc, (t.value, b.value, l.value)

    def without(p, *ks):
        return [None if k in ks else v for k, v in enumerate(p)]

    def bent(p, k, by=2):
        return [v + by if j == k else v for j, v in enumerate(p)]

    for entry, n, required in (("fwd", 6, (0, 1, 2, 4, 5)), ("bwd", 6, (0, 1, 2, 4)), ("mom", 7, (0,))):
        p = A[:n]
        assert call(entry, p) == (0, (64, 1, K.LDS_BYTES)), entry
        for k in required:
            assert call(entry, without(p, k))[0] == K.EINVAL, (entry, k)
        for kw in (dict(E=0), dict(B=0), dict(C=0, D=0), dict(D=-1), dict(C=5), dict(C=3, D=3, sigma=0.0), dict(C=3, D=3, sigma=-1.0),
                   dict(C=3, D=3, sigma=float("nan")), dict(C=3, D=3, sigma=float("inf")), dict(lo=1.0, hi=0.0), dict(lo=float("nan"))):
            assert call(entry, p, **kw)[0] == K.EINVAL, (entry, kw)
        assert call(entry, p, sigma=float("nan"))[0] == 0                # the heteroscedastic form does not read noise_sigma
        assert call(entry, p, C=3, D=3, sigma=30.0)[0] == 0 and call(entry, p, lo=2.0, hi=2.0)[0] == 0
        if entry != "mom":
            for kw in (dict(mc=2), dict(mc=-1), dict(mo=-1)):
                assert call(entry, p, **kw)[0] == K.EINVAL, (entry, kw)
            assert call(entry, p, mc=1, mo=40)[0] == 0
            assert call(entry, without(p, 3))[0] == 0                    # beta_dev is optional
        for k in range(n):
            assert call(entry, bent(p, k))[0] == K.EALIGN, (entry, k)
        # EINVAL comes before EALIGN, EALIGN before ESHAPE
        assert call(entry, bent(p, 0), E=0)[0] == K.EINVAL and call(entry, bent(without(p, 0), 1))[0] == K.EINVAL
        assert call(entry, bent(p, 1, 1), E=K.MAX_DRAWS + 1)[0] == K.EALIGN
        for kw in (dict(E=K.MAX_DRAWS + 1), dict(C=1026, D=513), dict(C=1025, D=1025), dict(B=2 ** 31 - 63), dict(B=2 ** 31 - 1)):
            assert call(entry, p, **kw)[0] == K.ESHAPE, (entry, kw)
        assert call(entry, p, E=K.MAX_DRAWS, C=1024, D=512, B=2 ** 31 - 64) == (0, (64, 2 ** 25 - 1, K.LDS_BYTES))
        for c in K.CASES:
            assert call(entry, p, E=c.E, B=c.B, C=c.C, D=c.D, sigma=c.noise_sigma or 0.0, lo=c.log_var_min, hi=c.log_var_max,
                        mc=K.MODES.index(c.mc), mo=c.mean_over) == (0, (K.THREADS, -(-c.B // K.THREADS), K.LDS_BYTES)), (entry, c.name)
    assert call("bwd", without(A[:6], 5))[0] == 0                        # g_kl is optional
    mom = A[:7]
    assert call("mom", without(mom, 2, 3, 4, 5, 6))[0] == K.EINVAL       # no output wanted
    assert call("mom", without(mom, 1))[0] == K.EINVAL                   # log_density without y
    assert call("mom", without(mom, 1, 6))[0] == 0 and call("mom", without(mom, 2, 3, 4, 5))[0] == 0
    assert h.bbb_gauss_moments_cb_plan(*mom[:2], 2, 4, 6, 3, 0.0, -20.0, 20.0, *mom[2:], None, None, None) == 0


def test_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/gauss_tail_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: ordinary arguments, then arguments at the 32-bit limits."""
    gxx = shutil.which("g++") or shutil.which("clang++")
    assert gxx is not None, "a host C++ compiler is part of the build environment"
    exe = str(tmp_path / "gauss_tail_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "gauss_tail_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    # the counts per return code and the checksum of every code and every field of every plan: a change of any rule is made here too
    assert got == {"cases": "120000", "ok": "32828", "einval": "44846", "ealign": "2859", "eshape": "39467", "checksum": "9e670bb9cbd83a01"}, got


def test_forward_loss_with_a_likelihood_on_a_cpu_model_raises_the_device_error():
    lib = _lib()
    import ref_port_torch as P
    from bbb_hip import train, uncertainty
    from layers import BBB_Linear, FlattenLayer
    net = nn.Sequential(FlattenLayer(12), BBB_Linear(12, 6, bias=True, priors=P.CONFIG_PRIORS))
    x, y = torch.zeros(4, 3, 2, 2), torch.zeros(4, 3)
    lik = train.GaussianLikelihood()
    with pytest.raises(lib.BBBHipError, match="MI355X only"):
        train.forward_loss(net, x, y, 2, 0.1, 100.0, likelihood=lik)
    opt = torch.optim.Adam(net.parameters())
    with pytest.raises(lib.BBBHipError, match="MI355X only"):
        train.train_step(net, opt, x, y, 2, 0.1, 100.0, likelihood=lik)
    with pytest.raises(lib.BBBHipError, match="GaussianLikelihood"):
        train.forward_loss(net, x, y, 2, 0.1, 100.0, likelihood="gaussian")
    with pytest.raises(lib.BBBHipError):
        uncertainty.mc_regression(net, x, T=2, likelihood=lik)
    with pytest.raises(lib.BBBHipError, match="GaussianLikelihood"):
        uncertainty.mc_regression(net, x, T=2)
