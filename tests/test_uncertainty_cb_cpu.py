"""CPU-only companions of tests/test_gpu_uncertainty_cb.py: the contract of the batch-innermost uncertainty reduction
(tests/uncertainty_cb_contract.py) held against itself.  The fp32 model's worst error per output over all cases IS the stored constant
the device bound is built from; the float64 references satisfy entropy - expected_entropy = mutual_info; the boundaries the kernel
promises exact zeros at give exact zeros in the model; the two C entries refuse, in the documented order and in agreement with each
other, before any launch; the host-only plan (csrc/mc_uncertainty_plan.h) walks its argument space under the address and
undefined-behaviour sanitizers; and uncertainty.mc_uncertainty, on a model off the batch-innermost path, transposes once into the one
kernel and consumes T noise calls.  No device; the library is only loaded, never launched."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import tail_contract as TC
import uncertainty_cb_contract as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")


@pytest.fixture(scope="module")
def refs():
    """{case name: (rows, float64 reference, fp32 model)}, computed once."""
    out = {}
    for c in K.CASES:
        rows = K.rows_of(c)
        out[c.name] = (rows, K.reference(rows, c.p["normalized"]), K.model(rows, c.p["normalized"]))
    return out


def test_constants_are_the_measured_model_errors(refs):
    worst = {}
    for c in K.CASES:
        rows, ref, mod = refs[c.name]
        for f, r in K.ratios(mod, ref, rows).items():
            if r > worst.get(f, (-1.0, ""))[0]:
                worst[f] = (r, c.name)
    print("fp32 model, worst |model - float64| / scale:", {k: (round(v, 3), n) for k, (v, n) in worst.items()})
    assert set(worst) == set(K.MODEL_CONSTANT) == set(K.FIELDS)
    for f, (r, name) in worst.items():
        assert K.MODEL_CONSTANT[f] == K.round_up_1sf(r), (f, r, name)
    assert K.DEVICE_FACTOR == 4 and K.bound("entropy") == 4 * K.MODEL_CONSTANT["entropy"]


def test_references_satisfy_the_entropy_identity(refs):
    for c in K.CASES:
        _, ref, _ = refs[c.name]
        d = np.abs(K.entropy_difference(ref) - ref["mutual_info"])
        nan = np.isnan(ref["mutual_info"])
        assert (np.isnan(d) == nan).all() and (d[~nan] <= 1e-12).all(), c.name
        assert (ref["mutual_info"][~nan] >= -1e-12).all(), c.name


def test_case_table_covers_recipes_sizes_and_boundaries():
    plain = [c for c in K.CASES if not c.p["normalized"]]
    norm = [c for c in K.CASES if c.p["normalized"]]
    assert {c.recipe for c in plain} == set(TC.RECIPES) and {c.recipe for c in norm} == set(K.NORMALIZED_RECIPES)
    assert TC.SOFTPLUS_RECIPE in K.NORMALIZED_RECIPES and "offset+10000" in TC.RECIPES
    own = [c for c in K.CASES if "inject" not in c.p and c.slabs != K.MAX_DRAWS]
    assert {c.slabs for c in own} == set(TC.DRAWS) and {c.C for c in own} == set(TC.CLASSES_CB) and {c.B for c in own} == set(TC.BATCHES)
    assert any(c.slabs == 1 and c.C > 1 for c in plain) and any(c.slabs == 1 and c.C > 1 for c in norm)
    assert any(c.C == 1 and c.slabs > 1 for c in plain) and any(c.C == 1 and c.slabs > 1 for c in norm)
    assert any(c.slabs == c.C == c.B == 1 for c in K.CASES) and any(c.B == 64 for c in K.CASES)
    assert [(c.slabs, c.C, c.B) for c in K.CASES if c.name.endswith("-maxT")] == [(K.MAX_DRAWS, 3, 4)] * 2
    assert {c.p["inject"] for c in plain if "inject" in c.p} == set(K.INJECTIONS)
    for c in K.CASES:
        x = K.rows_of(c)
        assert x.dtype == np.float32 and x.shape == (c.slabs, c.B, c.C) and np.array_equal(K.rows_of(c), x, equal_nan=True)
        assert TC.layout(c, x).shape == (c.slabs, c.C, c.B)


def test_boundaries_give_exact_zeros_and_non_finite_logits_stay_local(refs):
    for c in K.CASES:
        rows, ref, mod = refs[c.name]
        if c.slabs == 1:
            assert not mod["epistemic"].any() and not mod["mutual_info"].any(), c.name
            assert not ref["epistemic"].any() and np.abs(ref["mutual_info"]).max() <= 1e-12, c.name     # (log(exp(ls)) is not ls)
        if c.C == 1:
            for f in K.FIELDS[4:]:
                assert not mod[f].any() and not ref[f].any(), (c.name, f)
        inj = c.p.get("inject")
        if inj in ("neginf_some", "neginf_all"):
            assert np.isneginf(rows).any()
            for f in K.FIELDS[1:]:
                assert np.isfinite(ref[f]).all() and np.isfinite(mod[f]).all(), (c.name, f)
            assert (np.isneginf(ref["pred"]) == np.isneginf(rows).any(axis=0)).all()
            if inj == "neginf_all":
                assert (ref["p_mean"][np.isneginf(ref["pred"])] == 0).all() and np.isneginf(ref["pred"]).any()
        if inj in ("nan", "posinf"):
            hit = np.zeros(c.B, bool)
            hit[[5, 64]] = True
            for f in K.FIELDS[1:]:
                bad = np.isnan(ref[f])
                assert (bad.reshape(c.B, -1).all(axis=1) == hit).all() and (bad.reshape(c.B, -1).any(axis=1) == hit).all(), (c.name, f)
            assert (~np.isfinite(ref["pred"])).sum() == 2
    # the planted-fault side of the checker: a NaN or an infinity that is not the reference's is an assertion, not a ratio
    ref = np.array([[0.5, np.nan], [np.inf, 0.25]])
    rows = np.ones((1, 2, 2), np.float32)
    assert K.field_ratio("p_mean", ref, ref, rows) == 0.0
    for bad in (np.array([[0.5, 0.0], [np.inf, 0.25]]), np.array([[np.nan, np.nan], [np.inf, 0.25]]), np.array([[0.5, np.nan], [-np.inf, 0.25]]),
                np.array([[0.5, np.nan], [1.0, 0.25]])):
        with pytest.raises(AssertionError):
            K.field_ratio("p_mean", bad, ref, rows)
    assert abs(K.field_ratio("p_mean", np.array([[0.5 + 3 * K.U, np.nan], [np.inf, 0.25]]), ref, rows) - 3.0) < 1e-6


def _lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def test_entries_refuse_in_the_documented_order_and_agree():
    """Every refusal code of bbb_mc_uncertainty_cb and of its host-only plan, reached through the library loaded on the CPU: the launch
    entry returns before a launch (addresses are only looked at), and the plan entry gives the same code for the same arguments."""
    lib = _lib()
    from bbb_hip import ops
    h = lib.lib()
    assert lib.ABI_VERSION == 13 and h.bbb_abi_version() == 13
    assert ops.MC_UNCERTAINTY_MAX_DRAWS == K.MAX_DRAWS and ops.Uncertainty._fields == K.FIELDS
    a = 0x1000
    outs = [0x2000 + 0x1000 * i for i in range(7)]
    none = [None] * 7
    only = lambda i, v=0x2000: none[:i] + [v] + none[i + 1:]
    i32 = ctypes.c_int32

    def both(logits, T, B, C, o):
        r, b, l = i32(-7), i32(-7), i32(-7)
        rc_plan = h.bbb_mc_uncertainty_cb_plan(logits, T, B, C, *o, ctypes.byref(r), ctypes.byref(b), ctypes.byref(l))
        if rc_plan != 0:
            assert (r.value, b.value, l.value) == (0, 0, 0)
            for norm in (0, 1):
                assert h.bbb_mc_uncertainty_cb(logits, T, B, C, norm, *o, None) == rc_plan      # refused: nothing is launched
        return rc_plan, (r.value, b.value, l.value)

    refused = [
        (K.EINVAL, (None, 2, 4, 3, outs)), (K.EINVAL, (a, 0, 4, 3, outs)), (K.EINVAL, (a, 2, 0, 3, outs)), (K.EINVAL, (a, 2, 4, -1, outs)),
        (K.EINVAL, (a, 2, 4, 3, none)),
        (K.EINVAL, (None, 2, 4, 3, only(0, 0x2002))),                    # EINVAL comes before EALIGN ...
        (K.EINVAL, (a + 1, 0, 4, 3, outs)),
        (K.EALIGN, (a + 2, 2, 4, 3, outs)), (K.EALIGN, (a, 2, 4, 3, only(6, 0x2001))), (K.EALIGN, (a, 2, 4, 3, only(1, 0x2003))),
        (K.EALIGN, (a + 2, K.MAX_DRAWS + 1, 4, 3, outs)),                # ... and EALIGN before ESHAPE
        (K.ESHAPE, (a, K.MAX_DRAWS + 1, 4, 3, outs)), (K.ESHAPE, (a, 2 ** 31 - 1, 4, 3, only(4))),
        (K.ESHAPE, (a, 2, 2 ** 31 - 63, 3, outs)), (K.ESHAPE, (a, 2, 2 ** 31 - 1, 3, only(0))),
    ]
    for want, args in refused:
        assert both(*args)[0] == want, (want, args)
    # admitted by the plan (no launch made here): rows, blocks, LDS bytes
    assert both(a, K.MAX_DRAWS, 4, 3, outs) == (0, (16, 1, K.MAX_DRAWS * K.LDS_PER_DRAW + K.LDS_REDUCE))
    assert K.MAX_DRAWS * K.LDS_PER_DRAW + K.LDS_REDUCE <= 160 * 1024 < (K.MAX_DRAWS + 1) * K.LDS_PER_DRAW + K.LDS_REDUCE
    assert both(a, 1, 1, 1, only(5)) == (0, (1, 1, K.LDS_PER_DRAW + K.LDS_REDUCE))
    assert both(a, 2, 2 ** 31 - 64, 2 ** 31 - 1, only(2)) == (0, (16, 2 ** 25 - 1, 2 * K.LDS_PER_DRAW + K.LDS_REDUCE))
    assert both(a, 5, 130, 10, outs)[1][:2] == (10, 3) and both(a, 15, 64, 10, outs)[1][:2] == (15, 1)
    assert h.bbb_mc_uncertainty_cb_plan(a, 5, 130, 10, *outs, None, None, None) == 0
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = " ".join(fh.read().split())
    for phrase in ("draws <= 202", "batch <= INT32_MAX - 63", "all seven outputs NULL", "draws * 768 + 8192",
                   "A term with p = 0 contributes exactly 0", "clamped below at 0", "#define BBB_ABI_VERSION 13"):
        assert phrase in header, phrase


def test_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/mc_uncertainty_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: ordinary arguments, then arguments at the 32-bit limits."""
    gxx = shutil.which("g++") or shutil.which("clang++")
    assert gxx is not None, "a host C++ compiler is part of the build environment"
    exe = str(tmp_path / "mc_uncertainty_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "mc_uncertainty_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    # the counts per return code and the checksum of every code and every field of every plan: a change of any rule is made here too
    assert got == {"cases": "120000", "ok": "64154", "einval": "22990", "ealign": "3893", "eshape": "28963", "checksum": "22ccca25bac46046"}, got


class _Hidden(nn.Module):
    """A Bayesian layer inside a module with a forward of its own: ensemble.flat_children rejects the model."""

    def __init__(self):
        super().__init__()
        import ref_port_torch as P
        from layers import BBB_Linear
        self.fc = BBB_Linear(12, 5, bias=True, priors=P.CONFIG_PRIORS)

    def forward(self, x):
        return self.fc(x.flatten(1))


def test_mc_uncertainty_off_the_fast_path_transposes_once_into_the_kernel(monkeypatch):
    _lib()
    from bbb_hip import ensemble, ops, rng, uncertainty
    net = nn.Sequential()
    net.add_module("block", _Hidden())
    assert ensemble.flat_children(net) is None and not ensemble._chwn_ok(net, torch.zeros(4, 3, 2, 2))
    T, B, C = 6, 4, 5
    logits = torch.arange(T * B * C, dtype=torch.float32).reshape(T, B, C)
    seen = {}

    def fake_mc_logits(model, x, draws, seed, call0, **kw):
        seen["mc_logits"] = (model, tuple(x.shape), draws, seed, call0, kw)
        return logits, torch.zeros(())

    def fake_kernel(logits_cb, normalized=False, want=None):
        seen["kernel"] = (logits_cb, normalized, want)
        return "scores"

    monkeypatch.setattr(ensemble, "mc_logits", fake_mc_logits)
    monkeypatch.setattr(ops, "mc_uncertainty_cb", fake_kernel)
    saved = dict(rng._state)
    try:
        rng.manual_seed(1234, call=100)
        assert uncertainty.mc_uncertainty(net, torch.zeros(B, 3, 2, 2), T=T, normalized=True, precision="bf16x3") == "scores"
        assert rng.get_state() == (1234, 100 + T)                        # T calls, as get_uncertainty_per_batch
    finally:
        rng._state.clear()
        rng._state.update(saved)
    assert seen["mc_logits"] == (net, (B, 3, 2, 2), T, 1234, 100, {"precision": "bf16x3"})
    got, normalized, want = seen["kernel"]
    assert normalized is True and want is None
    assert tuple(got.shape) == (T, C, B) and got.is_contiguous() and torch.equal(got, logits.permute(0, 2, 1))
