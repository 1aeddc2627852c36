"""CPU-only companions of tests/test_gpu_adam_ex.py: the contract of the clipped / decayed / guarded Adam step
(tests/adam_ex_contract.py) held against itself.  The plans of the three new launch entries (host only) -- chunk walks, every refusal,
the scalars bit for bit; the two plan headers under the address and undefined-behaviour sanitizers in a stand-alone program; the
float64 restatement against torch's clip_grad_norm_ + Adam on float64 tensors; the constants of the value bounds by adam_contract's
rule from torch's CPU fp32 Adam; every checker against the fault planted for it; and FusedAdam's state dict.  No device."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import adam_contract as A
import adam_ex_contract as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
F32 = np.float32


def _lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    _lib.lib()
    return _lib


# ---- 1. plans ----

def test_adam_ex_plan_scalars_and_chunk_walk():
    """bbb_adam_step_ex_plan: bbb_adam_step_plan's answers, plus wd32, decay and the mode, bit for bit the contract's."""
    _lib()
    from bbb_hip import ops
    for h in A.HYPERS.values():
        for t in (1, 7, 2 ** 24 - 1):
            for wd in X.WDS + (1.0, 1e3):
                for decoupled in (False, True):
                    plan = ops.adam_plan_ex([5, 1025], h.lr, (h.beta1, h.beta2), h.eps, wd, decoupled, t)
                    assert plan["status"] == 0
                    X.check_scalars_ex(plan, h, t, wd, decoupled)
    # decay is formed from the double lr, not from the float: DECAY_APART_WDS holds pairs that tell the two apart
    apart = [(lr, wd) for lr in A.DEVICE_LRS for wd in X.DECAY_APART_WDS if F32(1.0 - lr * wd) != F32(1.0 - A.lr_through_float(lr) * wd)]
    print("(lr, wd) at which float(float32(lr)) gives another decay:", apart)
    assert (0.1, 7.0) in apart and (1e-3, 30.0) in apart
    for lr, wd in apart:
        X.check_scalars_ex(ops.adam_plan_ex([7], lr, weight_decay=wd, decoupled=True), A.DEFAULT._replace(lr=lr), 1, wd, True)
        with pytest.raises(AssertionError):
            X.check_scalars_ex(ops.adam_plan_ex([7], A.lr_through_float(lr), weight_decay=wd, decoupled=True), A.DEFAULT._replace(lr=lr), 1, wd, True)
    # the chunk walk and the vector rule are bbb_adam_step's own, geometry case by geometry case
    for c in A.GEOMETRY_CASES:
        lay, which = A.geo_layout(c), A.geo_launched(c)
        old = ops.adam_plan(lay.plan_segments(which), step=A.GEOMETRY_T)
        new = ops.adam_plan_ex(lay.plan_segments(which), weight_decay=1e-2, step=A.GEOMETRY_T, coef_dev=0x900000, ok_dev=0x900004)
        assert new["status"] == 0 and all(new[k] == old[k] for k in old), c.name
        assert new["mode"] == "l2"
    assert ops.adam_plan_ex([7], weight_decay=0.0, decoupled=True)["mode"] == "none"


def test_grad_norm_plan_chunk_walk():
    _lib()
    from bbb_hip import ops
    assert ops.GRAD_NORM_CHUNK == X.NORM_CHUNK == 4096
    for c in A.GEOMETRY_CASES:
        lay, which = A.geo_layout(c), A.geo_launched(c)
        plan = ops.grad_norm_plan(lay.plan_segments(which), first=11)
        assert plan["status"] == 0, c.name
        assert plan["chunk_begin"][:len(which) + 1] == list(np.cumsum([0] + [X.chunks_of(lay.n[s]) for s in which])), c.name
        assert all(b == plan["chunks"] for b in plan["chunk_begin"][len(which):]), c.name
        assert plan["vec"] == [lay.off[s][1] == 0 and lay.n[s] >= 4 for s in which], c.name          # the gradient's alignment alone
    for n, chunks in ((1, 1), (4095, 1), (4096, 1), (4097, 2), (8192, 2), (8193, 3)):
        assert ops.grad_norm_plan([n])["chunks"] == chunks
    sizes = list(A.FUSED_SIZES[33])
    whole = sum(X.chunks_of(n) for n in sizes)
    assert sum(ops.grad_norm_plan(sizes[i:i + 16])["chunks"] for i in (0, 16, 32)) == whole == 33


def test_every_refusal_of_the_new_entries_returns_its_code_before_any_launch():
    """The plan queries and the launch entries themselves: addresses are only looked at, so no device is needed for a refusal."""
    lib = _lib()
    from bbb_hip import ops
    L = lib.lib()
    seg_addr = [dict(n=n, param=0x10000 * (4 * s + 1), grad=0x10000 * (4 * s + 2), exp_avg=0x10000 * (4 * s + 3), exp_avg_sq=0x10000 * (4 * s + 4))
                for s, n in enumerate(A.REFUSAL_SIZES)]
    ok = ops.adam_plan_ex(seg_addr, weight_decay=1e-2, step=3, coef_dev=0x900200, ok_dev=0x900204)
    assert ok["status"] == 0 and ok["chunks"] == 4 and ok["vec"] == [True, True, True]
    assert set(A.REFUSALS) < set(X.EX_REFUSALS) and len(X.EX_REFUSALS) == len(A.REFUSALS) + 6
    for name, (code, change) in X.EX_REFUSALS.items():
        segs, nseg, h, step, step_dev, lr_dev, wd, coef_dev, ok_dev = X.ex_refusal_args(change, seg_addr, 0x900000, 0x900100, 0x900200, 0x900204)
        plan = ops.adam_plan_ex(segs, h.lr, (h.beta1, h.beta2), h.eps, wd, False, step, step_dev, lr_dev, coef_dev, ok_dev, nseg=nseg)
        assert plan["status"] == code, (name, plan["status"])
        assert plan["chunks"] == 0 and not any(plan["chunk_begin"]) and not any(plan["vec"]) and plan["mode"] == "none", name
        assert all(plan[k] == 0.0 for k in ops.ADAM_PLAN_EX_SCALARS), name
        rc = L.bbb_adam_step_ex(A.segment_array(lib, segs), nseg, h.lr, h.beta1, h.beta2, h.eps, wd, 0, step, step_dev or None, lr_dev or None,
                                coef_dev or None, ok_dev or None, None)
        assert rc == code, (name, rc)
    # the sumsq launch
    assert ops.grad_norm_plan(seg_addr, partials=0x800000)["chunks"] == 3
    assert {code for code, _ in X.SUMSQ_REFUSALS.values()} == {A.EINVAL, A.EALIGN, A.ESHAPE}
    for name, (code, change) in X.SUMSQ_REFUSALS.items():
        segs, nseg = A.refusal_args({k: v for k, v in change.items() if k in ("seg", "nseg")}, seg_addr, 0, 0)[:2]
        partials, first = X.moved(change, "partials", 0x800000), change.get("first", 0)
        plan = ops.grad_norm_plan(segs, partials, first, nseg=nseg)
        assert plan["status"] == code, (name, plan["status"])
        assert plan["chunks"] == 0 and not any(plan["chunk_begin"]) and not any(plan["vec"]), name
        assert L.bbb_grad_sumsq(A.segment_array(lib, segs), nseg, partials or None, first, None) == code, name
    assert ops.grad_norm_plan(seg_addr, 0x800000, first=2 ** 31 - 4)["status"] == 0
    for name, change in X.SUMSQ_IGNORED.items():
        segs = A.refusal_args(change, seg_addr, 0, 0)[0]
        assert ops.grad_norm_plan(segs, 0x800000)["status"] == 0, name
    # the finish launch
    assert {code for code, _ in X.FINISH_REFUSALS.values()} == {A.EINVAL, A.EALIGN, A.ESHAPE}
    base = dict(partials=0x800000, norm=0x900300, coef=0x900304, ok=0x900308, skipped=0x90030c)
    for name, (code, change) in X.FINISH_REFUSALS.items():
        addr = {k: X.moved(change, k, v) for k, v in base.items()}
        n, mx = change.get("npartials", 3), change.get("max_norm", 1.0)
        plan = ops.grad_norm_plan(seg_addr, addr["partials"], max_norm=mx, norm=2.0, npartials=n,
                                  outs=(addr["norm"], addr["coef"], addr["ok"], addr["skipped"]))
        assert plan["finish_status"] == code and plan["coef"] == 0.0, (name, plan)
        rc = L.bbb_grad_norm_finish(addr["partials"] or None, n, mx, 1, addr["norm"] or None, addr["coef"] or None, addr["ok"] or None,
                                    addr["skipped"] or None, None)
        assert rc == code, (name, rc)
    plan = ops.grad_norm_plan(seg_addr, 0x800000, max_norm=1.0, norm=2.0)
    assert plan["finish_status"] == 0 and plan["coef"] == float(X.coef_ref(2.0, 1.0)) == float(F32(1.0 / (2.0 + 1e-6)))


def test_finish_plan_coefficient_is_the_contracts_bit_for_bit():
    _lib()
    from bbb_hip import ops
    norms = [0.0, 1e-30, 1e-6, 0.5, 0.999999, 1.0, 1.000001, 2.0, 37.5, 1e6, 1e30, 3.4e38, math.inf, math.nan]
    for norm in norms:
        for mx in (1e-6, 0.1, 1.0, 5.0, 1e6, math.inf):
            got = ops.grad_norm_plan([7], max_norm=mx, norm=norm)["coef"]
            X.check_coef(got, norm, mx, "norm %r max %r" % (norm, mx))
    assert float(X.coef_ref(math.inf, 5.0)) == 0.0 and np.isnan(X.coef_ref(math.nan, 5.0)) and float(X.coef_ref(0.5, 1.0)) == 1.0
    assert np.isnan(X.coef_ref(math.nan, math.inf)) and float(X.coef_ref(math.inf, math.inf)) == 1.0
    # the planted fault: fmin swallows the NaN
    _, c = X.norm_model([np.array([1.0, np.nan, 2.0], F32)], 1.0, fault="fmin")
    assert float(c) == 1.0
    with pytest.raises(AssertionError):
        X.check_coef(c, np.nan, 1.0)


# ---- 2. plan headers under the sanitizers ----

def test_plan_headers_under_the_sanitizers(tmp_path):
    """tests/host/grad_norm_plan_check.cpp (csrc/grad_norm_plan.h and adam_plan::plan_ex alone: no device code, not loaded into Python)
    under -fsanitize=address,undefined: a seeded sweep, every refusal, n and `first` next to their limits and to INT64_MAX."""
    gxx = shutil.which("g++") or shutil.which("clang++")
    assert gxx is not None, "a host C++ compiler is part of the build environment"
    exe = str(tmp_path / "grad_norm_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "grad_norm_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    assert got == {"cases": "60190", "ok": "52657", "einval": "5491", "ealign": "1605", "eshape": "349", "checksum": "e975bfff308deea9"}, got


# ---- the float64 restatement against torch in float64 ----

def test_float64_restatement_is_torchs_clip_and_adam_in_float64():
    """norm, coefficient and the update formulas of the contract, restated in float64 with unrounded scalars, against
    clip_grad_norm_ + torch.optim.Adam(weight_decay, decoupled_weight_decay) on float64 tensors, three tensors, step 3."""
    h, t = A.CHAIN_HYPER, 3
    worst = 0.0
    for decoupled in (False, True):
        for max_norm in (None, 0.05, 1e9):
            tensors = [tuple(np.asarray(a, dtype=np.float64) for a in A.draw("ref64/%d" % i, n)) for i, n in enumerate(A.CHAIN_SIZES)]
            ps = [torch.from_numpy(p.copy()) for p, _, _, _ in tensors]
            opt = torch.optim.Adam(ps, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=0.1, decoupled_weight_decay=decoupled, foreach=False)
            for p, (_, g, m, v) in zip(ps, tensors):
                p.grad = torch.from_numpy(g.copy())
                opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
            norm = X.norm_ref([g for _, g, _, _ in tensors])
            coef = 1.0
            if max_norm is not None:
                tn = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False))
                assert abs(tn - norm) <= 1e-15 * norm
                coef = min(1.0, max_norm / (norm + X.NORM_EPS))
                assert (coef < 1.0) == (max_norm == 0.05)
            opt.step()
            for p, (p0, g, m, v) in zip(ps, tensors):
                g1 = coef * g + (0.0 if decoupled else 0.1 * p0)
                q0 = p0 * (1.0 - h.lr * 0.1) if decoupled else p0
                want = A.step64(q0, g1, m, v, h, t)
                st = opt.state[p]
                for got, w in zip((p.numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), want):
                    worst = max(worst, float(np.abs(got - w).max()))
    print("float64 restatement against torch, worst |diff|: %.3g" % worst)
    assert worst <= 1e-15


# ---- 4. constants ----

@pytest.fixture(scope="module")
def reference_ratios():
    """{(case, wd, decoupled, coef): {m, v, p: ratio}} of torch's CPU fp32 Adam fed fp32(coef g) against the float64 reference."""
    out = {}
    for c in A.VALUE_CASES:
        before, h = A.values_of(c), A.HYPERS[c.hyper]
        for wd in X.WDS:
            for decoupled in ((False,) if wd == 0.0 else (False, True)):
                ex = X.scalars_ex(h, c.t, wd, decoupled)
                for coef in X.COEFS:
                    out[(c.name, wd, decoupled, coef)] = X.value_ratios_ex(before, X.torch_adam_ex(before, h, c.t, wd, decoupled, coef), ex, coef)
    return out


def test_constants_follow_from_the_fp32_reference(reference_ratios):
    worst, neutral = {}, {}
    for key, r in reference_ratios.items():
        for k, x in r.items():
            if x > worst.get(k, (0.0, ""))[0]:
                worst[k] = (x, key)
            if key[1] == 0.0 and key[3] == 1.0:
                neutral[k] = max(neutral.get(k, 0.0), x)
    print("torch CPU fp32 Adam with decay, fed fp32(coef g): worst |out - float64| / (2^-23 M):", {k: (round(x, 3), n) for k, (x, n) in worst.items()})
    print("at wd = 0, coef = 1:", {k: round(x, 3) for k, x in neutral.items()})
    assert len(reference_ratios) == len(A.VALUE_CASES) * (1 + 2 * (len(X.WDS) - 1)) * len(X.COEFS)
    assert set(worst) == set(X.C_EX) == {"m", "v", "p"}
    for k, (x, key) in worst.items():
        assert X.C_EX[k] == A.constant_from(x), (k, x, key)
    # without decay and without clipping the figures are adam_contract's own
    for k, x in neutral.items():
        assert A.C[k] == A.constant_from(x), (k, x)


# ---- 3. the contract against itself ----

def test_value_checker_accepts_the_fp32_model_and_rejects_planted_faults():
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for c in A.VALUE_CASES:
        before, h = A.values_of(c), A.HYPERS[c.hyper]
        for wd, decoupled, coef in ((1e-2, False, 0.37), (1e-2, True, 1.0), (0.3, True, 1e-3), (0.0, False, None)):
            ex = X.scalars_ex(h, c.t, wd, decoupled)
            r = X.check_values_ex(before, X.model32_ex(before, ex, coef), ex, 1.0 if coef is None else coef, c.name)
            worst = {k: max(worst[k], r[k]) for k in r}
    print("fp32 model (numpy, no contraction), worst ratios:", {k: round(x, 3) for k, x in worst.items()})
    # neutral arguments give adam_contract's model bit for bit
    before = A.values_of(A.VALUE_CASES[0])
    ex0 = X.scalars_ex(A.DEFAULT, 7, 0.0, True)
    for coef in (None, 1.0):
        assert all((A.bits(a) == A.bits(b)).all() for a, b in zip(X.model32_ex(before, ex0, coef), A.model32(before, ex0.base)))
    by_name = {c.name: c for c in A.VALUE_CASES}
    c = by_name["loose-t7-g0.001-match"]
    before, h = A.values_of(c), A.HYPERS[c.hyper]
    ex = X.scalars_ex(h, c.t, 0.3, True)
    assert float(ex.decay) == float(F32(1.0 - 0.1 * 0.3))
    with pytest.raises(AssertionError):       # decay applied after the update
        X.check_values_ex(before, X.model32_ex(before, ex, 0.37, fault="decay_after_update"), ex, 0.37, c.name)
    c = by_name["default-t7-g1-match"]
    before, h = A.values_of(c), A.HYPERS[c.hyper]
    for wd, decoupled, wrong in ((1e-2, False, dict(decoupled=True)), (1e-2, True, dict(decoupled=False)), (0.3, False, dict(wd=0.0))):
        ex = X.scalars_ex(h, c.t, wd, decoupled)
        other = X.scalars_ex(h, c.t, wrong.get("wd", wd), wrong.get("decoupled", decoupled))
        with pytest.raises(AssertionError):   # the other form of decay, or none
            X.check_values_ex(before, X.model32_ex(before, other, 0.37), ex, 0.37, c.name)
    ex = X.scalars_ex(h, c.t, 1e-2, False)
    with pytest.raises(AssertionError):       # the coefficient left out
        X.check_values_ex(before, X.model32_ex(before, ex, None), ex, 0.37, c.name)
    with pytest.raises(AssertionError):       # the gradient clipped twice
        X.check_values_ex(before, X.model32_ex(before, ex, 0.37 * 0.37), ex, 0.37, c.name)


# ---- 5. norm reference ----

def test_norm_checker_accepts_the_float64_model_and_rejects_an_fp32_accumulation():
    worst = 0.0
    for scale in X.NORM_SCALES:
        grads = [X.norm_grad("s%g" % scale, A.VALUE_N, scale)]
        norm, coef = X.norm_model(grads, 1.0)
        worst = max(worst, X.check_norm(norm, grads, "scale %g" % scale))
        X.check_coef(coef, norm, 1.0)
        assert 20 * scale < float(norm) < 60 * scale                                # sqrt(1537) = 39.2: the norm has no range of its own
    grads = [X.norm_grad("sixteen/%d" % s, n) for s, n in enumerate(A.SIXTEEN_N)]
    worst = max(worst, X.check_norm(X.norm_model(grads, 1.0)[0], grads, "sixteen"))
    print("float64 model of the two launches, worst |norm - ref| / (2^-23 ref): %.3f" % worst)
    assert worst <= 0.5 + 1e-6                                                       # one rounding: half an ulp
    for scale, wrong in ((1e30, math.inf), (1e-30, 0.0)):
        grads = [X.norm_grad("s%g" % scale, A.VALUE_N, scale)]
        norm, _ = X.norm_model(grads, 1.0, fault="fp32_sumsq")
        assert float(norm) == wrong
        tn = float(torch.nn.utils.clip_grad_norm_([_with_grad(grads[0])], 1.0))
        assert tn == wrong                                                           # torch's fp32 norm does the same
        with pytest.raises(AssertionError):
            X.check_norm(norm, grads)
    # classes
    for x, want in ((np.nan, math.nan), (np.inf, math.inf), (-np.inf, math.inf)):
        g = X.norm_grad("cls", 100)
        g[17] = x
        norm, coef = X.norm_model([g], 1.0)
        X.check_norm(norm, [g])
        assert math.isnan(want) and np.isnan(coef) or float(coef) == 0.0
    g[17], g[18] = np.inf, np.nan
    assert math.isnan(X.norm_ref([g])) and np.isnan(X.norm_model([g], 1.0)[0])
    with pytest.raises(AssertionError):
        X.check_norm(F32(np.inf), [g])


def _with_grad(g):
    p = torch.zeros(len(g), requires_grad=True)
    p.grad = torch.from_numpy(np.array(g))
    return p


def test_class_reference_of_a_clipped_step():
    """What the class tier of the device test is held to: with a NaN gradient element torch's clip_grad_norm_ + Adam turns EVERY output
    into NaN; with an Inf the coefficient is 0 and only the poisoned elements are NaN -- and the fp32 model with the contract's coefficient
    has the same classes, while the fmin coefficient does not."""
    t, h, mx = 7, A.DEFAULT, 5.0
    clean = A.draw("cls-ex", A.POISON_N, 1.0)
    for x in (np.nan, np.inf, -np.inf):
        bad = A.poisoned(clean, "grad", x)
        want = X.torch_clipped_adam([bad], h, t, 1e-2, False, mx)[0]
        norm, coef = X.norm_model([bad[1]], mx)
        ex = X.scalars_ex(h, t, 1e-2, False)
        X.check_all_classes(X.model32_ex(bad, ex, coef), want, repr(x))
        if np.isnan(x):
            assert all(np.isnan(w).all() for w in want)
            _, wrong = X.norm_model([bad[1]], mx, fault="fmin")
            with pytest.raises(AssertionError):
                X.check_all_classes(X.model32_ex(bad, ex, wrong), want)
        else:
            assert float(coef) == 0.0 and all(int(np.isnan(w).sum()) == len(A.POISON_AT) for w in want[1:])


# ---- 6. no new group keys ----

@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (1e-2, False), (1e-2, True)])
@pytest.mark.parametrize("max_norm,skip", [(None, False), (1.0, False), (None, True), (0.5, True)])
def test_state_dict_has_torch_adams_keys_and_round_trips(wd, decoupled, max_norm, skip):
    from bbb_hip import train
    make = lambda: [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.ones(3))]
    opt = train.FusedAdam(make(), lr=2e-3, weight_decay=wd, decoupled_weight_decay=decoupled, max_grad_norm=max_norm, skip_nonfinite=skip)
    ref = torch.optim.Adam(make(), lr=1e-3)
    sd = opt.state_dict()
    assert set(sd["param_groups"][0]) <= set(ref.state_dict()["param_groups"][0])
    assert all(not torch.is_tensor(v) for v in sd["param_groups"][0].values())
    assert "max_grad_norm" not in sd["param_groups"][0] and "skip_nonfinite" not in sd["param_groups"][0] and set(sd) == {"state", "param_groups"}
    assert sd["param_groups"][0]["weight_decay"] == wd and sd["param_groups"][0]["decoupled_weight_decay"] == decoupled
    assert sd["param_groups"][0]["capturable"] == skip                              # the guard needs the step counts on the device
    assert opt.max_grad_norm == max_norm and opt.skip_nonfinite == skip and opt.grad_norm is None and opt.skipped_steps is None
    for cls in (torch.optim.Adam, torch.optim.AdamW):
        other = cls(make(), lr=1e-3)
        other.load_state_dict(sd)
        g = other.param_groups[0]
        assert g["lr"] == 2e-3 and g["weight_decay"] == wd
        assert g["decoupled_weight_decay"] == decoupled or cls is torch.optim.AdamW        # (AdamW keeps its own form)
        back = train.FusedAdam(make(), lr=1.0)
        back.load_state_dict(other.state_dict())
        assert back.param_groups[0]["weight_decay"] == wd and back.param_groups[0]["lr"] == 2e-3 and back.max_grad_norm is None


def test_constructors():
    from bbb_hip import train
    p = lambda: [torch.nn.Parameter(torch.zeros(4))]
    w = train.FusedAdamW(p())
    assert w.param_groups[0]["weight_decay"] == 1e-2 and w.param_groups[0]["decoupled_weight_decay"] is True
    assert train.FusedAdam(p()).param_groups[0]["weight_decay"] == 0.0
    for bad in (dict(weight_decay=-1.0), dict(max_grad_norm=0.0), dict(max_grad_norm=-2.0), dict(max_grad_norm=math.nan)):
        with pytest.raises(ValueError):
            train.FusedAdam(p(), **bad)
    # positional order: torch.optim.Adam's first four, then weight_decay, decoupled_weight_decay, capturable
    o = train.FusedAdam(p(), 1e-3, (0.8, 0.9), 1e-6, 0.5, True, True)
    g = o.param_groups[0]
    assert (g["betas"], g["eps"], g["weight_decay"], g["decoupled_weight_decay"], g["capturable"]) == ((0.8, 0.9), 1e-6, 0.5, True, True)
    assert "p.grad" in train.FusedAdam.__doc__ and "never written" in train.FusedAdam.__doc__
