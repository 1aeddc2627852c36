"""CPU-only companions of tests/test_gpu_uncertainty_grad.py: the contract of the uncertainty reduction's backward
(tests/uncertainty_grad_contract.py) held against itself.  The closed-form float64 reference equals float64 torch autograd of the
forward contract's definitions; the fp32 model's worst error over all cases and upstream patterns IS the stored constant the device
bound is built from; the zero and non-finite conventions hold in reference and model; the two C entries refuse, in the documented
order and in agreement with each other, before any launch; the host-only plan walks its argument space under the address and
undefined-behaviour sanitizers; and uncertainty.mc_uncertainty(grad=True) refuses CPU tensors.  No device; the library is only loaded,
never launched."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import uncertainty_cb_contract as K
import uncertainty_grad_contract as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")


@pytest.fixture(scope="module")
def refs():
    """{(case name, pattern): (float64 gradient, A, fp32 model)}, computed once."""
    out = {}
    for c in G.CASES:
        rows, norm = G.rows_of(c), c.p["normalized"]
        pm = G.forward_p_mean(rows, norm)
        for pat in G.PATTERNS:
            w = G.upstream_of(c, pat)
            out[c.name, pat] = G.reference(rows, norm, w) + (G.model(rows, norm, w, pm),)
    return out


def _torch_loss(z, normalized, w):
    """sum of (upstream x output) with the outputs written from uncertainty_cb_contract.reference's definitions in float64 torch:
    mutual_info in its KL form, not clamped."""
    if normalized:
        sp = torch.where(z > 20, z, torch.log1p(torch.exp(torch.clamp(z, max=20))))
        tot = sp.sum(dim=2, keepdim=True)
        p, lp = sp / tot, torch.log(sp) - torch.log(tot)
    else:
        lp = torch.log_softmax(z, dim=2)
        p = torch.exp(lp)
    pbar = p.mean(dim=0)
    lpbar = torch.log(pbar)
    out = {"pred": z.mean(dim=0), "p_mean": pbar, "epistemic": ((p - pbar[None]) ** 2).mean(dim=0),
           "aleatoric": pbar - (p ** 2).mean(dim=0), "entropy": -(pbar * lpbar).sum(dim=1),
           "expected_entropy": -(p * lp).sum(dim=2).mean(dim=0), "mutual_info": (p * (lp - lpbar[None])).sum(dim=2).mean(dim=0)}
    return sum((torch.from_numpy(w[f].astype(np.float64)) * out[f]).sum() for f in G.FIELDS if w[f] is not None)


def test_closed_form_is_float64_autograd_of_the_definitions(refs):
    """On every case without an injection and without a zero probability, every pattern: |closed form - autograd| <= 1e-12 x (the
    case's largest A + its largest upstream weight).  Relative to A, the scale of the sums both sides form (C = 1 and T = 1 have
    gradients that are 0 in exact arithmetic); the weight stands for the absolute error of log p, 2^-53 x the spread of the logits
    however small |log p| is -- in the 'dominant' cases the two sides' log p of the leading class, ~1e-15, agree to one digit."""
    checked = 0
    for c in G.CASES:
        rows, norm = G.rows_of(c), c.p["normalized"]
        p, _ = G.probs64(rows, norm)
        if "inject" in c.p or (p == 0).any():
            continue
        for pat in G.PATTERNS:
            z = torch.from_numpy(rows.astype(np.float64)).requires_grad_(True)
            w = G.upstream_of(c, pat)
            want, = torch.autograd.grad(_torch_loss(z, norm, w), z)
            g, A, _ = refs[c.name, pat]
            w_max = max(float(np.abs(v).max()) for v in w.values() if v is not None)
            assert np.abs(g - want.numpy()).max() <= 1e-12 * (A.max() + w_max), (c.name, pat)
            assert (A >= np.abs(g) * (1 - 1e-12)).all(), (c.name, pat)
        checked += 1
    assert checked >= 30, checked


def test_constant_is_the_measured_model_error(refs):
    worst = {}
    for (name, pat), (g, A, mod) in refs.items():
        r = G.ratio(mod, g, A)
        if r > worst.get(pat, (-1.0, ""))[0]:
            worst[pat] = (r, name)
    print("fp32 model, worst |model - float64| / scale per pattern:", {k: (round(v, 3), n) for k, (v, n) in worst.items()})
    assert set(worst) == set(G.PATTERNS) == set(G.MODEL_CONSTANT)
    for pat, (r, name) in worst.items():
        assert G.MODEL_CONSTANT[pat] == G.round_up_1sf(r), (pat, r, name)
    assert G.DEVICE_FACTOR == 4 and G.bound("entropy") == 4 * G.MODEL_CONSTANT["entropy"]


def test_patterns_and_scales():
    c = G.BY_NAME["mc_uncertainty_cb-gauss4-10x17x64-B64"]
    for f in G.FIELDS:
        w = G.upstream_of(c, f)
        assert [k for k, v in w.items() if v is not None] == [f] and (w[f] == 1).all()
        assert w[f].shape == ((64, 17) if f in G.PER_CLASS else (64,)) and w[f].dtype == np.float32
    full, alt = G.upstream_of(c, "all"), G.upstream_of(c, "all_alternate")
    for f in G.FIELDS:
        assert np.array_equal(full[f][0::2], alt[f][0::2]) and not alt[f][1::2].any() and full[f][1::2].all()
    rows = G.rows_of(c)
    g, A = G.reference(rows, False, alt)
    assert not g[:, 1::2].any() and not A[:, 1::2].any() and (G.image_scales(A)[0::2] > 0).all()
    # an image of the alternate pattern is the image of the full pattern: nothing crosses images
    g_full, _ = G.reference(rows, False, full)
    assert np.array_equal(g[:, 0::2], g_full[:, 0::2])
    # the planted-fault side of the checker
    assert G.ratio(g, g, A) == 0.0
    bad = g.copy()
    bad[0, 1, 0] = 1e-30
    with pytest.raises(AssertionError):
        G.ratio(bad, g, A)                               # an image without weight must be exactly 0
    bad = g.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        G.ratio(bad, g, A)
    off = g.copy()
    off[3, 2, 5] += 3 * G.image_scales(A)[2]
    assert abs(G.ratio(off, g, A) - 3.0) < 1e-6


def test_zero_and_non_finite_conventions(refs):
    for c in G.CASES:
        rows = G.rows_of(c)
        inj = c.p.get("inject")
        for pat in G.PATTERNS:
            g, A, mod = refs[c.name, pat]
            if inj is None and (c.C == 1 or (c.slabs == 1 and pat == "mutual_info")):
                # one class: p = 1 and G = D; mutual information of one draw: log p_bar is log p.  The probability side is an exact 0
                # on both sides whether its scale is 0 (one class under entropy: log p = 0, no term at all) or not: no special case
                w_pred = G.upstream_of(c, pat)["pred"]
                side = 0.0 if w_pred is None else w_pred[None] / np.float32(c.slabs)
                assert np.array_equal(mod, np.broadcast_to(np.float32(side), mod.shape)), (c.name, pat)
                assert np.abs(g - side).max() <= 1e-7 * np.abs(side).max() and (A.max() > 0 or not mod.any()), (c.name, pat)
            if inj in ("neginf_some", "neginf_all"):
                at = np.isneginf(rows)
                assert at.any() and np.isfinite(g).all() and np.isfinite(mod).all(), (c.name, pat)
                w_pred = G.upstream_of(c, pat)["pred"]
                if w_pred is None:
                    assert not g[at].any() and not mod[at].any(), (c.name, pat)
                else:                                                          # d pred / d logit = 1 / T at any logit
                    want = np.broadcast_to((w_pred / np.float32(c.slabs))[None], rows.shape)[at]
                    assert np.array_equal(mod[at], want) and np.allclose(g[at], want, rtol=1e-6, atol=0), (c.name, pat)
            if inj in ("nan", "posinf"):
                hit = np.zeros(c.B, bool)
                hit[[5, 64]] = True
                for arr in (g, mod):
                    bad = np.isnan(arr).transpose(1, 0, 2).reshape(c.B, -1)
                    assert (bad.all(axis=1) == hit).all() and (bad.any(axis=1) == hit).all() and not np.isinf(arr).any(), (c.name, pat)
                clean = K._recipe_rows(c)
                w = G.upstream_of(c, pat)
                g0, _ = G.reference(clean, False, w)
                m0 = G.model(clean, False, w)
                assert np.array_equal(g[:, ~hit], g0[:, ~hit]) and np.array_equal(mod[:, ~hit].view(np.uint32), m0[:, ~hit].view(np.uint32))


def _lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def test_entries_refuse_in_the_documented_order_and_agree():
    lib = _lib()
    from bbb_hip import ops
    h = lib.lib()
    assert lib.ABI_VERSION == 13 and h.bbb_abi_version() == 13 and ops.MC_UNCERTAINTY_MAX_DRAWS == G.MAX_DRAWS
    a, pm, d = 0x1000, 0x9000, 0xA000
    ups = [0x2000 + 0x1000 * i for i in range(7)]
    none = [None] * 7
    only = lambda i, v=0x2000: none[:i] + [v] + none[i + 1:]
    i32 = ctypes.c_int32

    def both(logits, p_mean, T, B, C, w, out):
        r, b, l = i32(-7), i32(-7), i32(-7)
        rc = h.bbb_mc_uncertainty_cb_bwd_plan(logits, p_mean, T, B, C, *w, out, ctypes.byref(r), ctypes.byref(b), ctypes.byref(l))
        if rc != 0:
            assert (r.value, b.value, l.value) == (0, 0, 0)
            for norm in (0, 1):
                assert h.bbb_mc_uncertainty_cb_bwd(logits, p_mean, T, B, C, norm, *w, out, None) == rc      # refused: nothing is launched
        return rc, (r.value, b.value, l.value)

    refused = [
        (G.EINVAL, (None, pm, 2, 4, 3, ups, d)), (G.EINVAL, (a, None, 2, 4, 3, ups, d)), (G.EINVAL, (a, pm, 2, 4, 3, ups, None)),
        (G.EINVAL, (a, pm, 0, 4, 3, ups, d)), (G.EINVAL, (a, pm, 2, 0, 3, ups, d)), (G.EINVAL, (a, pm, 2, 4, -1, ups, d)),
        (G.EINVAL, (a, pm, 2, 4, 3, none, d)),
        (G.EINVAL, (None, pm, 2, 4, 3, only(0, 0x2002), d)),             # EINVAL comes before EALIGN ...
        (G.EINVAL, (a + 1, pm, 0, 4, 3, ups, d)),
        (G.EALIGN, (a + 2, pm, 2, 4, 3, ups, d)), (G.EALIGN, (a, pm + 1, 2, 4, 3, ups, d)), (G.EALIGN, (a, pm, 2, 4, 3, ups, d + 3)),
        (G.EALIGN, (a, pm, 2, 4, 3, only(6, 0x2001), d)), (G.EALIGN, (a, pm, 2, 4, 3, only(1, 0x2003), d)),
        (G.EALIGN, (a + 2, pm, G.MAX_DRAWS + 1, 4, 3, ups, d)),          # ... and EALIGN before ESHAPE
        (G.ESHAPE, (a, pm, G.MAX_DRAWS + 1, 4, 3, ups, d)), (G.ESHAPE, (a, pm, 2 ** 31 - 1, 4, 3, only(4), d)),
        (G.ESHAPE, (a, pm, 2, 2 ** 31 - 63, 3, ups, d)), (G.ESHAPE, (a, pm, 2, 2 ** 31 - 1, 3, only(0), d)),
    ]
    for want, args in refused:
        assert both(*args)[0] == want, (want, args)
    # admitted by the plan (no launch made here): draws of a block, gridDim.x, LDS bytes
    assert both(a, pm, G.MAX_DRAWS, 4, 3, ups, d) == (0, (1, 1, 0))
    assert both(a, pm, 1, 1, 1, only(5), d) == (0, (1, 1, 0))
    assert both(a, pm, 2, 2 ** 31 - 64, 2 ** 31 - 1, only(2), d) == (0, (1, 2 ** 25 - 1, 0))
    assert both(a, pm, 5, 130, 10, ups, d) == (0, (1, 3, 0)) and both(a, pm, 15, 512, 10, only(6), d) == (0, (1, 8, 0))
    assert h.bbb_mc_uncertainty_cb_bwd_plan(a, pm, 5, 130, 10, *ups, d, None, None, None) == 0
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = " ".join(fh.read().split())
    for phrase in ("Backward of bbb_mc_uncertainty_cb in ONE launch", "all seven upstream gradients NULL", "NULL logits, p_mean or d_logits",
                   "contributes exactly 0 to D", "gradient is that of the KL form", "#define BBB_ABI_VERSION 13"):
        assert phrase in header, phrase


def test_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/mc_uncertainty_bwd_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: ordinary arguments, then arguments at the 32-bit limits."""
    gxx = shutil.which("g++") or shutil.which("clang++")
    assert gxx is not None, "a host C++ compiler is part of the build environment"
    exe = str(tmp_path / "mc_uncertainty_bwd_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "mc_uncertainty_bwd_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    # the counts per return code and the checksum of every code and every field of every plan: a change of any rule is made here too
    assert got == {"cases": "120000", "ok": "59932", "einval": "24677", "ealign": "6798", "eshape": "28593", "checksum": "ae00481847c6be84"}, got


def test_grad_true_refuses_cpu_tensors():
    _lib()
    import layers  # noqa: F401
    import ref_port_torch as P
    from bbb_hip import BBBHipError, ops, uncertainty, zoo
    net = zoo.getModel("lenet", 1, 10, P.CONFIG_PRIORS, "bbb", "softplus")
    x = torch.rand(4, 1, 32, 32, requires_grad=True)
    if next(net.parameters()).is_cuda:
        pytest.skip("GPU present")
    with pytest.raises(BBBHipError, match="MI355X only"):
        uncertainty.mc_uncertainty(net, x, T=2, grad=True)
    with pytest.raises(BBBHipError, match="MI355X only"):
        uncertainty.saliency(net, x, T=2)
    with pytest.raises(BBBHipError, match="MI355X only"):
        ops.mc_uncertainty_cb_autograd(torch.zeros(2, 3, 4, requires_grad=True))
    with pytest.raises(BBBHipError, match="score must be one of"):
        uncertainty.saliency(net, x, T=2, score="epistemic")
