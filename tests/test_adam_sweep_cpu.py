"""CPU-only companions of tests/test_gpu_adam_sweep.py: the contract of the multi-tensor Adam step (tests/adam_contract.py) held
against itself.  The float64 reference is torch.optim.Adam on float64 tensors; the constants of the value bounds follow from the fp32
reference (torch.optim.Adam(foreach=False) on CPU) by the stated rule; the cases reach the paths they name (bbb_adam_step_plan, host
only); every checker rejects the fault planted for it; every refusal returns its code without a device; and the host-only launch plan
(csrc/adam_plan.h) walks its argument space under the address and undefined-behaviour sanitizers.  No device; the library is needed
from the plan tests on."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import adam_contract as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
F32 = np.float32


def test_float64_reference_is_torch_adam_in_float64():
    """Six steps, gradients 10^(it - 3) N(0, 1), three tensors: step64 (the contract's formula with unrounded scalars) against
    torch.optim.Adam on float64 CPU tensors, per element within 1e-15 of the sum of the absolute terms."""
    h = A.CHAIN_HYPER
    sizes = A.CHAIN_SIZES
    ps = [torch.from_numpy(A.draw("ref%d" % i, n)[0].astype(np.float64)) for i, n in enumerate(sizes)]
    opt = torch.optim.Adam(ps, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, foreach=False)
    mine = [(p.numpy().copy(), np.zeros(n), np.zeros(n)) for p, n in zip(ps, sizes)]
    worst = 0.0
    for it in range(A.CHAIN_STEPS):
        gs = [A.chain_grad(it, n).astype(np.float64) for n in sizes]
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        for i, (p, g) in enumerate(zip(ps, gs)):
            p0, m0, v0 = mine[i]
            mine[i] = A.step64(p0, g, m0, v0, h, it + 1)
            st = opt.state[p]
            upd = np.abs(mine[i][0] - p0)
            scales = (np.abs(p0) + upd, np.abs(m0) + (np.abs(g) + np.abs(m0)) * (1 - h.beta1), mine[i][2])
            for got, want, sc in zip(mine[i], (p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), scales):
                worst = max(worst, float((np.abs(got - want) / sc).max()))
        assert int(opt.state[ps[0]]["step"]) == it + 1
    print("float64 reference against torch.optim.Adam(float64), worst |diff| / scale over six steps: %.3g" % worst)
    assert worst <= 1e-15


@pytest.fixture(scope="module")
def reference_ratios():
    """{case name: {m, v, p: ratio}} of torch's CPU fp32 Adam against the float64 reference, over the sweep's own value cases."""
    out = {}
    for c in A.VALUE_CASES:
        before = A.values_of(c)
        out[c.name] = A.value_ratios(before, A.torch_adam(before, A.HYPERS[c.hyper], c.t), A.scalars(A.HYPERS[c.hyper], c.t))
    return out


def test_constants_follow_from_the_fp32_reference(reference_ratios):
    worst = {}
    for name, r in reference_ratios.items():
        for k, x in r.items():
            if x > worst.get(k, (0.0, ""))[0]:
                worst[k] = (x, name)
    print("torch CPU fp32 Adam, worst |out - float64| / (2^-23 M):", {k: (round(x, 3), n) for k, (x, n) in worst.items()})
    assert set(worst) == set(A.C) == {"m", "v", "p"}
    for k, (x, name) in worst.items():
        assert A.C[k] == A.constant_from(x), (k, x, name)
    assert [A.constant_from(x) for x in (0.87, 0.99, 1.0, 1.46, 2.01, 0.2, 16.0)] == [4, 4, 4, 8, 16, 1, 64]
    with pytest.raises(AssertionError):
        A.constant_from(16.1)


def test_value_cases_are_the_whole_grid_and_nothing_is_left_out():
    cases = A.VALUE_CASES
    assert len({c.name for c in cases}) == len(cases) == len(A.HYPERS) * len(A.G_SCALES) * (len(A.T_VALUES) + 1)
    assert {(c.hyper, c.t, c.gscale) for c in cases} == {(h, t, g) for h in A.HYPERS for t in A.T_VALUES for g in A.G_SCALES}
    assert A.T_VALUES == (1, 2, 7, 1000, 100000, 2 ** 24 - 1) and A.G_SCALES == (1e-12, 1e-6, 1e-3, 1.0, 1e3, 1e6)
    assert {c.moments for c in cases if c.t == 1} == {"zero", "match"} and all(c.moments == "match" for c in cases if c.t > 1)
    hs = set(A.HYPERS.values())
    assert {A.Hyper(1e-3, 0.9, 0.999, 1e-8), A.Hyper(3e-3, 0.9, 0.999, 1e-8), A.Hyper(1e-1, 0.5, 0.9, 1e-3)} <= hs
    assert any(h.beta1 == 0 for h in hs) and any(h.beta2 == 0 for h in hs) and any(h.eps == 0 for h in hs)
    for c in cases:
        p, g, m, v = A.values_of(c)
        assert all(a.dtype == F32 and a.shape == (A.VALUE_N,) for a in (p, g, m, v)) and (g != 0).all()
        assert all((a == b).all() for a, b in zip(A.values_of(c), (p, g, m, v)))                   # the same values every time
        assert 0.1 * c.gscale < np.abs(g).mean() < 10 * c.gscale
        assert ((m == 0).all() and (v == 0).all()) if c.moments == "zero" else (0.01 * c.gscale ** 2 < v.mean() < 100 * c.gscale ** 2)
    # no escape hatches: the device file holds no skip, no expected failure, and the only exclusion from a bound is the class tier's
    with open(os.path.join(ROOT, "tests", "test_gpu_adam_sweep.py")) as fh:
        text = fh.read()
    for word in ("skip", "xfail", "importorskip"):
        assert word not in text, word


ARITHMETIC_FAULTS = {          # fault -> a value case on which the value checker must reject it
    "omb2_in_fp32": "default-t1-g1-zero",
    "eps_in_root": "default-t7-g0.001-match",
    "no_bc2": "default-t1-g1-match",
    "bc1_at_t-1": "default-t2-g1-match",
}


def test_value_checker_accepts_the_fp32_model_and_rejects_planted_faults():
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for c in A.VALUE_CASES:
        before, sc = A.values_of(c), A.scalars(A.HYPERS[c.hyper], c.t)
        r = A.check_values(before, A.model32(before, sc), sc, c.name)
        worst = {k: max(worst[k], r[k]) for k in r}
    print("fp32 model (numpy, no contraction), worst ratios:", {k: round(x, 3) for k, x in worst.items()})
    by_name = {c.name: c for c in A.VALUE_CASES}
    for fault, name in ARITHMETIC_FAULTS.items():
        c = by_name[name]
        h = A.HYPERS[c.hyper]
        before, sc = A.values_of(c), A.scalars(h, c.t)
        after = A.model32(before, sc, fault) if fault == "eps_in_root" else A.model32(before, A.faulty_scalars(h, c.t, fault))
        with pytest.raises(AssertionError):
            A.check_values(before, after, sc, name)
    # the value bound cannot see an lr rounded through float (one ulp of step_size at most): the scalar check and the bitwise
    # device-step tier are held to it instead
    c = by_name["default-t1-g1-match"]
    before = A.values_of(c)
    A.check_values(before, A.model32(before, A.faulty_scalars(A.DEFAULT, 1, "lr_through_float")), A.scalars(A.DEFAULT, 1))
    # a non-finite output has no place in this tier
    bad = [np.array(a) for a in A.model32(before, A.scalars(A.DEFAULT, 1))]
    bad[0][3] = np.nan
    with pytest.raises(AssertionError):
        A.check_values(before, bad, A.scalars(A.DEFAULT, 1))


def _lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    _lib.lib()
    return _lib


def test_plan_scalars_are_the_contracts_bit_for_bit():
    """bbb_adam_step_plan's scalars against scalars() for every (hyper-parameters, t) of the sweep and both forms of every device
    learning rate; an lr rounded through float on the host path is rejected at (lr = 1e-3, t = 1), and for every lr of DEVICE_LRS some t
    of the sweep tells the two roundings apart (so the device-step tier can see which one a launch used)."""
    _lib()
    from bbb_hip import ops
    for h in A.HYPERS.values():
        for t in A.T_VALUES + (2 ** 24, 2 ** 53 + 1):
            plan = ops.adam_plan([5, 1025], h.lr, (h.beta1, h.beta2), h.eps, t)
            assert plan["status"] == 0
            A.check_scalars(plan, h, t)
    for lr in A.DEVICE_LRS:
        through = A.lr_through_float(lr)
        assert through != lr
        for t in A.T_VALUES:
            A.check_scalars(ops.adam_plan([7], through, (0.9, 0.999), 1e-8, t), A.DEFAULT, t, lr=through)
    apart = {lr: [t for t in A.T_VALUES if A.scalars(A.DEFAULT, t, lr).step_size != A.scalars(A.DEFAULT, t, A.lr_through_float(lr)).step_size]
             for lr in A.DEVICE_LRS}
    print("t at which float(float32(lr)) gives another step_size than lr:", apart)
    assert 1 in apart[1e-3] and any(apart.values())
    bad = A.faulty_scalars(A.DEFAULT, 1, "lr_through_float")
    with pytest.raises(AssertionError):
        A.check_scalars(bad, A.DEFAULT, 1)
    A.check_scalars(A.scalars(A.DEFAULT, 1), A.DEFAULT, 1)
    for fault in ("omb2_in_fp32", "no_bc2"):
        with pytest.raises(AssertionError):
            A.check_scalars(A.faulty_scalars(A.DEFAULT, 1, fault), A.DEFAULT, 1)
    with pytest.raises(AssertionError):
        A.check_scalars(A.faulty_scalars(A.DEFAULT, 2, "bc1_at_t-1"), A.DEFAULT, 2)
    # with step_dev and step <= 0 the plan's host scalars are those of step 1
    A.check_scalars(ops.adam_plan([7], step=0, step_dev=4096), A.DEFAULT, 1)


def test_cases_reach_what_they_claim():
    _lib()
    from bbb_hip import ops
    names = [c.name for c in A.GEOMETRY_CASES]
    assert len(set(names)) == len(names)
    assert [c.sizes[0] for c in A.GEOMETRY_CASES if c.name.startswith("single-")] == [1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4099]
    seen_vec = set()
    for c in A.GEOMETRY_CASES:
        lay, which = A.geo_layout(c), A.geo_launched(c)
        plan = ops.adam_plan(lay.plan_segments(which), step=A.GEOMETRY_T)
        assert plan["status"] == 0, c.name
        assert plan["vec"] == [lay.vec_capable(s) for s in which], c.name
        assert plan["chunk_begin"][:len(which) + 1] == list(np.cumsum([0] + [-(-lay.n[s] // A.CHUNK) for s in which])), c.name
        assert all(b == plan["chunks"] for b in plan["chunk_begin"][len(which):]), c.name
        assert sum(lay.n) <= 12000, c.name                                       # a few thousand elements
        seen_vec |= {(c.name.split("+")[0], v) for v in plan["vec"]}
        for k in range(4):                                                       # sentinels before, between and behind
            b = A.bits(lay.host[k])
            edges = [0] + [x for s in range(len(lay.n)) for x in (lay.start[k][s], lay.start[k][s] + lay.n[s])] + [len(b)]
            for lo, hi in zip(edges[::2], edges[1::2]):
                assert hi - lo >= A.GUARD and (b[lo:hi] == A.SENTINEL).all(), (c.name, k)
            assert [(st - off[k]) % 4 for st, off in zip(lay.start[k], lay.off)] == [0] * len(lay.n)
    by = {c.name: c for c in A.GEOMETRY_CASES}
    # misaligned alone: every segment of the launch loses the 16-byte path, whichever of the four arrays is off; n < 4 never has it
    for d in (1, 2, 3):
        for kind in A.KINDS + ("all",):
            c = by["%s+%d" % (kind, d)]
            assert ops.adam_plan(A.geo_layout(c).plan_segments(), step=7)["vec"] == [False, False]
            assert min(c.sizes) >= 4 and max(c.sizes) > A.CHUNK                   # full quads go down the scalar path, in two chunks
    assert ops.adam_plan(A.geo_layout(by["mixed"]).plan_segments(), step=7)["vec"] == [True, False, False, False, False, True]
    assert [ops.adam_plan(A.geo_layout(by["single-n%d" % n]).plan_segments(), step=7)["vec"] for n in (1, 3, 4)] == [[False], [False], [True]]
    # the 16-segment walk: 16 distinct chunk_begin values, last chunks of 1, 2 and 3 elements where the table says
    c = by["sixteen"]
    plan = ops.adam_plan(A.geo_layout(c).plan_segments(), step=7)
    assert len(c.sizes) == A.MAX_SEGMENTS and len(set(plan["chunk_begin"][:16])) == 16 and plan["chunk_begin"][16] == plan["chunks"]
    for tail, s in A.SIXTEEN_TAILS.items():
        assert c.sizes[s] > A.CHUNK and c.sizes[s] % A.CHUNK == tail
    assert {1} <= set(c.sizes) and sum(1 for n in c.sizes if n % A.CHUNK == 0) >= 4 and c.sizes[0] == c.sizes[-1] == 1
    assert by["untouched"].launched == (0, 2, 4)
    # FusedAdam: two and three launches; poisons on both paths; the chained case
    # (FusedAdam drops parameters without a gradient before it splits: the launches are counted over the tensors that have one)
    assert [len(A.FUSED_SIZES[k]) for k in (17, 33)] == [17, 33] and [A.fused_launches(A.FUSED_SIZES[k]) for k in (17, 33)] == [2, 3]
    assert len(A.FUSED_NO_GRAD) == 4 and max(A.FUSED_NO_GRAD) == len(A.FUSED_NO_GRAD_SIZES) - 1 and 0 not in A.FUSED_NO_GRAD
    assert A.fused_launches(A.FUSED_NO_GRAD_SIZES, A.FUSED_NO_GRAD) == 2 and A.fused_launches(A.FUSED_SIZES[17], (1, 4, 5, 16)) == 1
    assert len(set(A.FUSED_STEPS)) == 5
    cap = A.DEFAULT._replace(lr=A.FUSED_CAPTURABLE_LR)
    assert A.scalars(cap, A.FUSED_CAPTURABLE_T).step_size != A.scalars(cap, A.FUSED_CAPTURABLE_T, A.lr_through_float(cap.lr)).step_size
    assert max(A.POISON_AT) == A.POISON_N - 1 and A.POISON_N % 4 == 1 and {1023, 1024} <= set(A.POISON_AT)
    kinds = {(k, "nan" if np.isnan(x) else float(x)) for k, x in A.POISONS}
    assert {("grad", x) for x in ("nan", np.inf, -np.inf, 1e30, 1e-30)} <= kinds and ("exp_avg_sq", -1.0) in kinds
    assert all((k, x) in kinds for k in ("param", "exp_avg", "exp_avg_sq") for x in ("nan", np.inf, -np.inf))
    with np.errstate(all="ignore"):
        assert F32(1e30) * F32(1e30) == np.inf and F32(1e-30) * F32(1e-30) == 0


def test_geometry_checker_rejects_planted_faults():
    by = {c.name: c for c in A.GEOMETRY_CASES}
    sc = A.scalars(A.DEFAULT, A.GEOMETRY_T)
    for name in ("sixteen", "mixed", "untouched", "all+3"):
        c = by[name]
        lay, which = A.geo_layout(c), A.geo_launched(c)
        ref = A.model32(lay.values(which), sc)                     # "one aligned launch over the same values"
        A.check_geometry(lay, A.model_launch(lay, which, sc), which, ref, name=name)
        for fault, where in (("stale_boundary", "exp_avg differs at element %d of segment" % (lay.n[which[0]] - 1)),
                             ("past_n", "exp_avg_sq differs at sentinel"), ("writes_grad", "grad differs at element 0 of segment")):
            with pytest.raises(AssertionError, match=where):
                A.check_geometry(lay, A.model_launch(lay, which, sc, fault), which, ref, name=name)
    # a launch that also updates a segment it was not given
    c = by["untouched"]
    lay = A.geo_layout(c)
    with pytest.raises(AssertionError, match="segment 1"):
        A.check_geometry(lay, A.model_launch(lay, [0, 1, 2, 4], sc), [0, 2, 4], A.model32(lay.values([0, 2, 4]), sc))
    # one wrong bit in a result
    lay = A.geo_layout(by["single-n5"])
    after = A.model_launch(lay, [0], sc)
    after[0].view(np.uint32)[lay.start[0][0] + 4] ^= 1
    with pytest.raises(AssertionError, match="param differs at element 4"):
        A.check_geometry(lay, after, [0], A.model32(lay.values([0]), sc))


def test_class_checker_rejects_a_nan_gradient_turned_into_a_finite_update():
    sc = A.scalars(A.DEFAULT, 7)
    clean_in = A.draw("poison", A.POISON_N, 1.0)
    clean = A.model32(clean_in, sc)
    seen = set()
    for kind, x in A.POISONS:
        bad_in = A.poisoned(clean_in, kind, x)
        want = A.torch_adam(bad_in, A.DEFAULT, 7)
        A.check_classes(A.model32(bad_in, sc), want, clean, "%s=%r" % (kind, x))
        seen |= {tuple(int(A.classes(w)[0]) for w in want)}
    assert len(seen) >= 5, seen                                     # the map is not trivial: several class patterns occur
    bad_in = A.poisoned(clean_in, "grad", np.nan)
    want = A.torch_adam(bad_in, A.DEFAULT, 7)
    with pytest.raises(AssertionError, match=r"output 0, element 0 is .* where torch has .*nan"):
        A.check_classes(A.model32(bad_in, sc, "nan_to_finite"), want, clean)
    spread = [np.array(a) for a in A.model32(bad_in, sc)]
    spread[1][6] = np.nan                                           # a poison that reaches its neighbour
    with pytest.raises(AssertionError):
        A.check_classes(spread, want, clean)
    off = [np.array(a) for a in A.model32(bad_in, sc)]
    off[2].view(np.uint32)[100] ^= 1                                # an untouched element that is not the clean launch's
    with pytest.raises(AssertionError, match="not the clean launch's"):
        A.check_classes(off, want, clean)


def test_every_refusal_returns_its_code_before_any_launch():
    """The plan query and the launch entry itself (addresses are only looked at: no device is needed for a refusal)."""
    lib = _lib()
    from bbb_hip import ops
    seg_addr = [dict(n=n, param=0x10000 * (4 * s + 1), grad=0x10000 * (4 * s + 2), exp_avg=0x10000 * (4 * s + 3), exp_avg_sq=0x10000 * (4 * s + 4))
                for s, n in enumerate(A.REFUSAL_SIZES)]
    ok = ops.adam_plan(seg_addr, step=3)
    assert ok["status"] == 0 and ok["chunks"] == 4 and ok["vec"] == [True, True, True]
    assert {code for code, _ in A.REFUSALS.values()} == {A.EINVAL, A.EALIGN, A.ESHAPE}
    for name, (code, change) in A.REFUSALS.items():
        segs, nseg, h, step, step_dev, lr_dev = A.refusal_args(change, seg_addr, 0x900000, 0x900100)
        plan = ops.adam_plan(segs, h.lr, (h.beta1, h.beta2), h.eps, step, step_dev, lr_dev, nseg=nseg)
        assert plan["status"] == code, (name, plan["status"])
        assert plan["chunks"] == 0 and not any(plan["chunk_begin"]) and not any(plan["vec"]), name
        assert all(plan[k] == 0.0 for k in ops.ADAM_PLAN_SCALARS), name
        arr = A.segment_array(lib, segs)
        rc = lib.lib().bbb_adam_step(arr, nseg, h.lr, h.beta1, h.beta2, h.eps, step, step_dev or None, lr_dev or None, None)
        assert rc == code, (name, rc)


def test_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/adam_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: ordinary segment lists, every refusal, the chunk limits, steps and betas at their ends."""
    gxx = shutil.which("g++") or shutil.which("clang++")
    assert gxx is not None, "a host C++ compiler is part of the build environment"
    exe = str(tmp_path / "adam_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "adam_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    # the counts per return code and the checksum of every code and every field of every plan: what the plan answers is pinned
    assert got == {"cases": "60553", "ok": "45452", "einval": "13426", "ealign": "1663", "eshape": "12", "checksum": "4e60e0139b84bcdd"}, got
