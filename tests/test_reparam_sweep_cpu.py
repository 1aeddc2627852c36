"""CPU-only companions of tests/test_gpu_reparam_sweep.py: the plan query (bbb_reparam_kl_plan = ops.reparam_plan, the launch entry's own
plan) against the launch rules written out in tests/reparam_contract.py over a seeded sweep, the case table's coverage of every
launch form and in-kernel path, each checker rejecting a planted fault, the half-way count of the exact tier, the fp32 mirror of the
backward inside c = 64, and a host-only walk of the plan under the address and undefined-behaviour sanitizers.  Needs the built
library, no device."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import bbb_numpy as O
import reparam_contract as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def test_plan_entry_is_exported_and_declared(lib):
    h = lib.lib()
    assert h.bbb_abi_version() == 13
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = fh.read()
    assert "bbb_reparam_kl_plan" in lib.EXPORTS and hasattr(h, "bbb_reparam_kl_plan") and "int bbb_reparam_kl_plan(" in header
    none = [None] * 8
    assert h.bbb_reparam_kl_plan(None, 1, 1, 2048, *none) == C.EINVAL
    seg = (lib.Segment * 1)()
    seg[0].mu = seg[0].rho = seg[0].w = 64
    seg[0].n = seg[0].draw_stride = 5
    assert h.bbb_reparam_kl_plan(seg, 1, 1, 2048, *none) == 0                       # null out-pointers
    assert h.bbb_reparam_kl_plan(seg, 1, 0, 2048, *none) == C.EINVAL
    seg[0].n = seg[0].draw_stride = 2 ** 41 + 1                                    # more chunks than a grid has blocks
    assert h.bbb_reparam_kl_plan(seg, 1, 1, 2048, *none) == C.ESHAPE
    # the refusal comes back before any launch, so the launch entry can be asked without a device
    assert h.bbb_reparam_kl_fwd(seg, 1, 1, 0.0, 0.1, 0, 0, 0, None, None, None, None, None) == C.ESHAPE
    seg[0].n = seg[0].draw_stride = 3 * 2048 * 1024                                 # n_small * draws beyond int32
    assert h.bbb_reparam_kl_plan(seg, 1, 2 ** 31 - 1, 2049, *none) == C.ESHAPE
    assert h.bbb_reparam_kl_plan(seg, 1, 2 ** 31 - 1, 2048, *none) == 0             # chunks % slots == 0: no split


def _sweep_descriptor(rng):
    """A segment list of the sweep: 1..16 segments; ordinary sizes, launches next to the split rule's edges (slots 2048) and beyond
    1024 x 16384 elements; external noise, bf16 rows and fp32 tap-major segments mixed in."""
    kind = rng.choice(["small", "small", "split", "split", "big", "generic", "generic", "tm"])
    nseg = rng.randint(1, 16)
    segs = []
    for i in range(nseg):
        n = rng.choice([rng.randint(1, 12), rng.randint(1, 5000), rng.randint(1, 300000)])
        segs.append({"n": n})
    if kind == "split":
        target = rng.choice([2048, 2049, 2137, 4095, 4096, 4097, 6143, 6144, 6145, rng.randint(1900, 6300)])
        have = sum(-(-s["n"] // 1024) for s in segs[1:])
        if target > have:
            segs[0]["n"] = (target - have) * 1024 - rng.randint(0, 1023)
    if kind == "big":
        segs[0]["n"] = C.BIG_TOTAL - sum(s["n"] for s in segs[1:]) + rng.randint(-2, 3000000)
        if rng.random() < 0.3:
            segs[-1]["eps"] = 64
    if kind == "generic":
        for s in rng.sample(segs, rng.randint(1, nseg)):
            if rng.random() < 0.5:
                s["eps"] = 64
            else:
                s["w_row_len"] = rl = rng.choice([1, 5, 8, 33, 72, 363, 1024])
                s["n"] = rl * rng.randint(1, 40)
                if rl % 9 == 0 and rng.random() < 0.5:
                    s["w_taps"] = 9
    if (kind == "tm" or (kind in ("small", "split", "big") and rng.random() < 0.1)) and not any("eps" in s for s in segs):
        pool = segs[1:] if nseg > 1 else segs
        for s in rng.sample(pool, rng.randint(1, min(3, len(pool)))):
            s["w_tm_cin"], s["w_taps"] = rng.choice([8, 16, 24, 40, 64]), rng.choice([2, 9, 25, 121, 128])
            s["n"] = s["w_tm_cin"] * s["w_taps"] * rng.randint(1, 70)
    draws = rng.choice([1, 1, 2, 3, 10, 16, 17, 25])
    return segs, draws


def test_plan_agrees_with_the_written_rules(lib):
    """30 000 seeded descriptors, slots = 2048: ops.reparam_plan == C.plan_rules field by field, and the sweep reaches every form."""
    from bbb_hip import ops
    rng = random.Random(20261018)
    reached = set()
    for _ in range(30000):
        segs, draws = _sweep_descriptor(rng)
        if any(s["n"] <= 0 for s in segs):
            continue
        got = ops.reparam_plan(segs, draws, 2048)
        rule = [(s["n"], "eps" in s, "w_row_len" in s, (s["w_tm_cin"], s["w_taps"]) if "w_tm_cin" in s else None) for s in segs]
        if got["kernel"] == "generic" and any(r[3] for r in rule):
            raise AssertionError("a tap-major segment on the generic kernel was not refused")
        want = C.plan_rules(rule, draws, 2048)
        assert got == want, (segs, draws, got, want)
        reached.add((got["kernel"], got["gpt"], got["nt"], got["n_small"] > 0, got["tm_blocks"] > 0))
    for form in (("fast", 1, True, False, False), ("fast", 1, False, False, False), ("fast", 4, True, False, False),
                 ("fast", 1, True, True, False), ("fast", 1, False, True, False), ("fast", 1, True, False, True),
                 ("fast", 4, True, False, True), ("generic", 1, False, False, False), ("generic", 4, False, False, False)):
        assert form in reached, (form, sorted(reached))
    # the rule's edges by hand: slots < chunks <= 3 slots, draws > 1
    for chunks, draws, excess in ((2048, 3, 0), (2049, 3, 1), (2137, 10, 89), (2137, 1, 0), (6143, 2, 2047), (6144, 2, 0), (6145, 2, 0)):
        p = ops.reparam_plan([chunks * 1024], draws, 2048)
        assert (p["n_small"], p["small_chunk0"], p["grid"]) == (excess * draws, chunks - excess, chunks - excess + excess * draws + 1)


def _generic_with_tm_is_refused(lib):
    from bbb_hip import ops
    with pytest.raises(lib.BBBHipError):
        ops.reparam_plan([{"n": 8 * 9 * 4, "w_tm_cin": 8, "w_taps": 9}, {"n": 10, "eps": 64}], 2, 2048)


def test_tap_major_refusals_need_no_device(lib):
    from bbb_hip import ops
    _generic_with_tm_is_refused(lib)
    ok = {"n": 8 * 9 * 4, "w_tm_cin": 8, "w_taps": 9}
    assert ops.reparam_plan([ok], 2, 2048)["tm_blocks"] == 1
    for bad in (dict(ok, w_taps=1, n=32), dict(ok, w_taps=129, n=8 * 129), dict(ok, w_tm_cin=12, n=12 * 9 * 4), dict(ok, eps=64),
                dict(ok, w=20), dict(ok, draw_stride=8 * 9 * 4 + 2)):
        with pytest.raises(lib.BBBHipError):
            ops.reparam_plan([bad], 2, 2048)
    with pytest.raises(lib.BBBHipError):
        ops.reparam_plan([8] * 17, 1, 2048)


def test_every_form_is_named_by_a_case(lib):
    """The case tables of tests/reparam_contract.py, by ops.reparam_plan at slots = 2048: each case takes the form it was written for,
    and together they reach every launch form, every in-kernel alignment path, every flag and every backward variant."""
    from bbb_hip import ops
    tags = set()
    for name, c in list(C.FWD_CASES.items()) + [("gpt4", C.GPT4_CASE)]:
        segs = c.segments(2048)
        p = ops.reparam_plan(C.descriptors(segs), c.draws, 2048)
        for k, v in c.want.items():
            if k == "split":
                v, k = {89: 89, -1: 2047, 0: 0}[v] * c.draws, "n_small"
            assert p[k] == v, (name, k, p)
        tags |= C.case_branches(c)
    want = {"fast<1,nt>", "fast<1,plain>", "fast<4,nt>", "per-draw-split", "tap-major-blocks", "generic<1>",
            "bf16:dense", "bf16:tap-major", "bf16:packed-store", "bf16:scalar-store", "bf16:pad", "bf16:ext-eps", "bf16:philox",
            "bf16:2-byte-aligned", "fast:ld_vec", "fast:ld_scalar", "fast:st_vec", "fast:st_scalar", "fast:sg_vec", "fast:sg_scalar",
            "fast:tail", "generic:aligned", "generic:unaligned", "generic:ext-eps", "generic:philox", "16-segments", "tm:mixed-launch",
            "split:segment-boundary+ragged-tail", "split:edge-3s", "split:edge-3s+1", "flag:sigma-squared", "flag:textbook",
            "flag:no-sample", "kl:none", "kl:64", "kl:32", "kl:both", "call_dev"}
    assert want <= tags, sorted(want - tags)
    # generic <4> is the GPT-4 case's own comparison launch
    big = C.canonical(C.GPT4_CASE.segments())
    assert ops.reparam_plan(C.descriptors(big), 1, 2048)["gpt"] == 4 and ops.reparam_plan(C.descriptors(big), 1, 2048)["kernel"] == "generic"
    # the split case: a segment boundary and a ragged tail inside the last 89 chunks
    segs = C.FWD_CASES["split-89"].segments(2048)
    ends = np.cumsum([-(-s.n // 1024) for s in segs])
    assert ends[-1] == 2048 + 89 and any(2048 < e < ends[-1] and s.n % 4 == 3 for e, s in zip(ends, segs))
    # backward: every flag combination, sizes, draws, strides, a five-segment launch with a 10-element and an offset-view segment
    combos = {combo for combo, _ in C.BWD_CASES.values()}
    assert combos == set(C.BWD_FLAGS) == set(C.BWD_C) and max(C.BWD_C.values()) <= C.BWD_C_MAX
    cases = [c for _, c in C.BWD_CASES.values()]
    assert {s.n for c in cases for s in c.segments()} >= {1, 5, 10, 1023, 1025, 4099}
    assert {c.draws for c in cases} == {1, 3} and {s.stride_extra for c in cases for s in c.segments()} == {0, 4}
    five = [c for c in cases if len(c.segments()) == 5]
    assert len(five) == len(C.BWD_FLAGS) and all(any(s.off for s in c.segments()) and any(s.n == 10 for s in c.segments()) for c in five)
    assert any(any(s.gs for s in c.segments()) and not all(s.gs for s in c.segments()) for c in five)       # one segment's gs NULL
    assert {c.call_dev for c in cases} == {None, 5, 2 ** 32 - 3}
    assert any(c.gkl is None for c in cases) and any(not s.gw for c in cases for s in c.segments())


def _cpu_noise(case, segs):
    return [C.external_noise(case, i, s.n, case.draws) if s.ext_eps else
            np.stack([O.normal_eps(case.seed, (case.call0 + (case.call_dev or 0) + e) & 0xFFFFFFFF, case.stream(i), s.n) for e in range(case.draws)])
            for i, s in enumerate(segs)]


def test_no_case_has_a_half_way_element():
    """The exact tier may skip elements whose ROUNDED float64 sum sits half-way between two fp32 values; with the cases' own seeds
    (sigma from the float32 oracle, Philox noise from the float64 stream) there are none.  The GPT-4 case: its float64 windows."""
    total = 0
    for c in C.FWD_CASES.values():
        segs = c.segments(2048)
        for s, (mu, rho), eps in zip(segs, C.case_inputs(c, segs), _cpu_noise(c, segs)):
            if s.want_w:
                _, skip = C.exact_sample(mu, O.sigma_from_rho(rho), eps)
                assert not skip.any(), (c.name, int(skip.sum()))
                total += skip.size
    c = C.GPT4_CASE
    rng_in = C.case_inputs(c, c.segments())
    for a in C.GPT4_WINDOWS:
        mu, rho = rng_in[0][0][a:a + 4096], rng_in[0][1][a:a + 4096]
        _, skip = C.exact_sample(mu, O.sigma_from_rho(rho), O.normal_eps(c.seed, c.call0, c.stream(0), 4096, start=a)[None])
        assert not skip.any()
    assert total > 10 ** 7


def test_textbook_reference_matches_the_reference_fixture(golden):
    Fn = golden["functions"]
    got = C.kl_textbook(Fn["kl.mu"], Fn["kl.sigma"], 0.0, 0.1)
    assert abs(got - float(Fn["kl.value_textbook"])) <= 2e-6 * float(Fn["kl.value_textbook"])


# ------------------------------------------------------------------------------------------------ planted faults
def _sample(seed=1, n=4099, draws=3):
    rng = np.random.default_rng(seed)
    mu, rho = (rng.standard_normal(n) * 0.1).astype(F32), rng.uniform(-6, 2, n).astype(F32)
    return mu, O.sigma_from_rho(rho), draws


def test_exact_checker_rejects_wrong_noise():
    mu, sigma, draws = _sample()
    eps = np.stack([O.normal_eps(9, 3 + e, 2, mu.size) for e in range(draws)])
    good, _ = C.exact_sample(mu, sigma, eps)
    assert C.check_exact(good, mu, sigma, eps) == 0
    nxt = np.stack([O.normal_eps(9, 4 + e, 2, mu.size) for e in range(draws)])                    # noise of call + 1
    with pytest.raises(AssertionError):
        C.check_exact(C.exact_sample(mu, sigma, nxt)[0], mu, sigma, eps)
    group = np.stack([O.normal_eps(9, 3 + e, 2, mu.size, start=4) for e in range(draws)])         # the neighbouring 4-element group
    with pytest.raises(AssertionError):
        C.check_exact(C.exact_sample(mu, sigma, group)[0], mu, sigma, eps)
    one = good.copy()                                                                             # one element, one ulp
    one[1, 77] = np.nextafter(one[1, 77], F32(1e9))
    with pytest.raises(AssertionError):
        C.check_exact(one, mu, sigma, eps)
    two = (mu[None] + eps * sigma[None]).astype(F32)                                              # two roundings instead of one
    assert (two != good).any()
    with pytest.raises(AssertionError):
        C.check_exact(two, mu, sigma, eps)


@pytest.mark.parametrize("seg,fault", [(C.bf(3, 33), "pad"), (C.bf(3, 33, stride_extra=8), "pitch"), (C.bf(3, 72, 9), "tm-swapped"),
                                       (C.tm(5, 8, 9), "tm-swapped"), (C.tm(3, 16, 2, stride_extra=4), "tm-swapped")])
def test_layout_checker_rejects(seg, fault):
    """A pad left non-zero, a row pitch that is not rounded, a tap-major column computed as ci * T + t."""
    vals = np.random.default_rng(2).standard_normal((2, seg.n)).astype(F32)
    good = C.w_image(seg, 2, vals)
    C.check_image(good.copy(), good)
    with pytest.raises(AssertionError):
        C.check_image(C.w_image(seg, 2, vals, fault), good)
    for hit in (0 if C.w_off(seg) else None, seg.extent if seg.stride_extra else None, good.size - 1):   # a write outside a draw
        if hit is not None:
            bad = good.copy()
            bad[hit] = 0
            with pytest.raises(AssertionError):
                C.check_image(bad, good)


def test_layouts_are_the_headers():
    seg = C.bf(2, 6, 3)                                  # rows of [cin 2][taps 3] -> columns t * 2 + ci, pitch 8
    v = np.arange(12, dtype=F32)
    img = C.draw_image(seg, v)
    assert img.size == 16 and not img[6:8].any() and not img[14:].any()
    assert (img[:6] == C.bf16_bits(v[[0, 3, 1, 4, 2, 5]])).all()
    seg = C.tm(2, 8, 2)                                  # [row][tap][ci]
    v = np.arange(32, dtype=F32)
    assert (C.draw_image(seg, v).view(F32)[:16] == np.concatenate([np.arange(0, 16, 2), np.arange(1, 16, 2)])).all()
    assert C.bf16_bits(np.array([1.00390625, 1.01171875], F32)).tolist() == [0x3F80, 0x3F82]      # ties to even, both ways


def _bwd_data(n=1025, draws=3, seed=4):
    rng = np.random.default_rng(seed)
    return dict(mu=(rng.standard_normal(n) * 0.1).astype(F32), rho=rng.uniform(-6, 2, n).astype(F32),
                gw=rng.standard_normal((draws, n)).astype(F32), gs=rng.standard_normal(n).astype(F32),
                eps=rng.standard_normal((draws, n)).astype(F32))


@pytest.mark.parametrize("fault,flags", [("drop-gs", 0), ("drop-gs", C.SIGMA_SQUARED), ("drop-2sigma", C.SIGMA_SQUARED),
                                         ("mean-only-leak", C.GW_MEAN_ONLY), ("other-kl", 0), ("other-kl", C.KL_TEXTBOOK)])
def test_backward_checker_rejects(fault, flags):
    d = _bwd_data()
    ref = C.bwd_reference(d["mu"], d["rho"], d["gw"], d["eps"], d["gs"], 0.37, flags)
    C.check_bwd(*C.bwd_mirror_f32(d["mu"], d["rho"], d["gw"], d["eps"], d["gs"], 0.37, flags), ref, C.BWD_C_MAX)
    with pytest.raises(AssertionError):
        C.check_bwd(*C.bwd_mirror_f32(d["mu"], d["rho"], d["gw"], d["eps"], d["gs"], 0.37, flags, fault=fault), ref, C.BWD_C_MAX)


def test_backward_mirror_stays_inside_c64():
    """The kernel's expression in numpy fp32 on every backward case's inputs: inside c = 64 of the float64 reference."""
    worst = {}
    for name, (combo, case) in C.BWD_CASES.items():
        segs = case.segments()
        for s, d in zip(segs, C.bwd_inputs(case, segs)):
            args = (d["mu"], d["rho"], d["gw"] if s.gw else None, d["eps"], d["gs"] if s.gs else None, case.gkl, case.flags)
            r = C.check_bwd(*C.bwd_mirror_f32(*args), C.bwd_reference(*args), C.BWD_C_MAX)
            worst[combo] = max(worst.get(combo, 0.0), r)
    print("fp32 mirror, worst |error| / (2^-23 M):", {k: round(v, 3) for k, v in worst.items()})


def test_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/reparam_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: ordinary segment lists, launches around the split rule, sizes / draws / slots at the integer limits."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "reparam_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "reparam_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    assert int(got["cases"]) >= 100000 and min(int(got[k]) for k in ("ok", "einval", "ealign", "eshape")) > 1000 and len(got["checksum"]) == 16
