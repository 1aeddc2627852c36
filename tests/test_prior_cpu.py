"""Per-weight Gaussian priors without a device: the checkers of tests/prior_contract.py have teeth (a numpy fp32 mirror of the
kernels' expression stays inside the bounds, planted faults break them), the case table covers what tests/test_gpu_prior_sweep.py
claims, the plan of the tensor-prior entry is the scalar entry's, the refusals, the prior checks of csrc/reparam_kl_plan.h under the
sanitizers, and the host logic of BayesianLayer.set_prior / bbb_hip.priors on CPU tensors."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import bbb_numpy as O
import prior_contract as P
import reparam_contract as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "pytorch-bayesiancnn_amd", "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the C surface
def test_entries_are_exported_and_declared(lib):
    h = lib.lib()
    assert h.bbb_abi_version() == 13
    with open(os.path.join(ROOT, "include", "bbb_hip.h")) as fh:
        header = fh.read()
    for name in ("bbb_reparam_kl_tp_fwd", "bbb_reparam_kl_tp_bwd", "bbb_reparam_kl_tp_plan"):
        assert name in lib.EXPORTS and hasattr(h, name) and ("int %s(" % name) in header
    assert "typedef struct bbb_prior_segment" in header and "#define BBB_ABI_VERSION 13" in header
    import ctypes
    assert ctypes.sizeof(lib.PriorSegment) == 16


# ------------------------------------------------------------------------------------------------ the mirror inside the bounds
def _data(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 0.1).astype(F32), rng.uniform(-6.0, 2.0, n).astype(F32)


@pytest.mark.parametrize("n", [4099, 2 ** 20])
@pytest.mark.parametrize("textbook", [False, True])
@pytest.mark.parametrize("regime", ["random", "near", "equal"])
def test_mirror_stays_inside_the_bounds(n, textbook, regime):
    """The expression in numpy fp32 (exact division, libm log2) against float64: at most 4.8 x 2^-23 of its magnitude per element,
    at most 0.1 x 2^-23 M on the float64 sum of the fp32 terms -- the reference alone is far inside the cap of 64."""
    mu, rho = _data(n, n + textbook)
    (mu0, s0), = P.prior_inputs("mirror-%s" % regime, regime, [(mu, rho)])
    sigma = O.sigma_from_rho(rho)
    t64, mag = P.kl_terms64(mu, sigma, mu0, s0, textbook)
    t32 = P.kl_mirror_f32(mu, sigma, mu0, s0, textbook)
    per = np.abs(t32.astype(F64) - t64) / (2.0 ** -23 * mag)
    assert per.max() <= 4.8, per.max()
    ratio = P.kl_ratio(t32.sum(dtype=F64), (float(t64.sum()), float(mag.sum())))
    assert ratio <= 0.1, ratio
    if regime == "equal":
        assert abs(float(t64.sum())) <= 1e-9 * mag.sum()          # the true KL is 0: only the bound in M has a meaning


@pytest.mark.parametrize("textbook", [False, True])
@pytest.mark.parametrize("fault", ["shift", "swap", "scalar"])
def test_planted_prior_faults_break_the_forward_check(fault, textbook):
    mu, rho = _data(4099, 5)
    (mu0, s0), = P.prior_inputs("fault", "random", [(mu, rho)])
    sigma = O.sigma_from_rho(rho)
    t64, mag = P.kl_terms64(mu, sigma, mu0, s0, textbook)
    ref = (float(t64.sum()), float(mag.sum()))
    P.check_kl_tp(P.kl_mirror_f32(mu, sigma, mu0, s0, textbook).sum(dtype=F64), ref, P.FWD_C_MAX)
    with pytest.raises(AssertionError):
        P.check_kl_tp(P.kl_mirror_f32(mu, sigma, mu0, s0, textbook, fault=fault).sum(dtype=F64), ref, P.FWD_C_MAX)


def test_bias_priors_taken_from_the_weight_break_the_check():
    """Two segments (weight, bias): the bias held to the head of the weight's prior tensors."""
    inputs = [_data(1025, 1), _data(10, 2)]
    pri = P.prior_inputs("w-for-b", "random", inputs)
    ref = P.kl_reference_tp(inputs, pri, 0)
    term = lambda i, p: P.kl_mirror_f32(inputs[i][0], O.sigma_from_rho(inputs[i][1]), p[0], p[1], False).sum(dtype=F64)
    P.check_kl_tp(term(0, pri[0]) + term(1, pri[1]), ref, P.FWD_C_MAX)
    with pytest.raises(AssertionError):
        P.check_kl_tp(term(0, pri[0]) + term(1, (pri[0][0][:10], pri[0][1][:10])), ref, P.FWD_C_MAX)


@pytest.mark.parametrize("combo", list(C.BWD_FLAGS))
def test_backward_mirror_and_planted_faults(combo):
    o = C.BWD_FLAGS[combo]
    flags, gkl = o.get("flags", 0), o.get("gkl", 0.37)
    rng = np.random.default_rng(11)
    n, E = 1025, 3
    mu, rho = _data(n, 3)
    gw, eps, gs = (rng.standard_normal((E, n)).astype(F32), rng.standard_normal((E, n)).astype(F32), rng.standard_normal(n).astype(F32))
    gw_, gs_ = (gw if o.get("gw", True) else None), (gs if o.get("gs", False) else None)
    for regime in ("random", "near", "equal"):
        (mu0, s0), = P.prior_inputs("bwd-mirror", regime, [(mu, rho)])
        ref = P.bwd_reference_tp(mu, rho, gw_, eps, gs_, gkl, flags, mu0, s0)
        C.check_bwd(*P.bwd_mirror_tp_f32(mu, rho, gw_, eps, gs_, gkl, flags, mu0, s0), ref, C.BWD_C_MAX)
        if gkl is not None and regime == "random":
            for fault in ("shift", "swap", "scalar"):
                with pytest.raises(AssertionError):
                    C.check_bwd(*P.bwd_mirror_tp_f32(mu, rho, gw_, eps, gs_, gkl, flags, mu0, s0, fault=fault), ref, C.BWD_C_MAX)
    # with scalar arrays the tensor-prior reference IS the scalar contract's
    a = P.bwd_reference_tp(mu, rho, gw_, eps, gs_, gkl, flags, np.full(n, C.PRIOR[0], F32), np.full(n, C.PRIOR[1], F32))
    b = C.bwd_reference(mu, rho, gw_, eps, gs_, gkl, flags)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_scalar_arrays_give_the_scalar_contracts_kl():
    inputs = [_data(4099, 8)]
    eff = [P.effective("--", None, 4099)]
    for flags in (0, C.KL_TEXTBOOK):
        kl, m = P.kl_reference_tp(inputs, eff, flags)
        assert abs(kl - C.kl_reference(inputs, flags)) <= 1e-6 * abs(kl) and m >= abs(kl)


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_covers_the_forms():
    names = set(P.FWD_CASES)
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4099):
        for e in (1, 3):
            assert "tp-n%d-e%d-tt" % (n, e) in names
    kinds, regimes, forms = set(), set(), set()
    for name, entry in P.FWD_CASES.items():
        case, _, regime = entry
        segs = case.segments(2048)
        ks = P.kinds_of(entry, len(segs))
        assert len(ks) == len(segs) and set(ks) <= set(P.KINDS) and regime in P.REGIMES, name
        kinds |= set(ks)
        regimes.add(regime)
        forms |= C.case_branches(case)
    assert kinds == set(P.KINDS) and regimes == set(P.REGIMES)
    need = {"fast<1,nt>", "generic<1>", "per-draw-split", "tap-major-blocks", "fast:ld_scalar", "fast:st_scalar", "fast:tail", "bf16:dense",
            "bf16:pad", "bf16:ext-eps", "bf16:philox", "generic:ext-eps", "generic:unaligned", "flag:sigma-squared", "flag:textbook",
            "flag:no-sample", "kl:32", "kl:64", "kl:none", "call_dev", "16-segments", "tm:mixed-launch"}
    assert need <= forms, need - forms
    # the split boundary of split-89 lies inside the segment that carries both prior tensors
    segs = P.FWD_CASES["tp-split-89"][0].segments(2048)
    begin = np.cumsum([0] + [-(-s.n // C.CHUNK) for s in segs])
    k = int(np.searchsorted(begin, 2048, side="right") - 1)
    assert begin[k] < 2048 < begin[k + 1] and P.FWD_CASES["tp-split-89"][1][k] == "tt"
    combos = {v[0] for n, v in P.BWD_CASES.items() if n.startswith("tp-bwd5-")}
    assert combos == set(C.BWD_FLAGS) and set(P.BWD_C) == set(C.BWD_FLAGS)
    assert max(P.FWD_C.values()) <= P.FWD_C_MAX and max(P.BWD_C.values()) <= C.BWD_C_MAX


# ------------------------------------------------------------------------------------------------ plan and refusals
def _fake_priors(kinds, nseg):
    out = []
    for i, k in enumerate(kinds[:nseg]):
        base = 0x4000000 + 0x100000 * i + (4 * C.OFF if k == "off" else 0)
        out.append((base if k in ("tt", "t-", "off") else 0, base + 0x80000 if k in ("tt", "-t", "off") else 0))
    return out


@pytest.mark.parametrize("name", list(P.FWD_CASES))
def test_plan_does_not_depend_on_the_prior(lib, name):
    from bbb_hip import ops
    entry = P.FWD_CASES[name]
    case = entry[0]
    for slots in (2048, 8 * 304):
        segs = case.segments(slots)
        want = C.plan_rules([(s.n, s.ext_eps, s.kind == "bf16", (s.cin, s.taps) if s.kind == "tm" else None) for s in segs], case.draws, slots)
        d = C.descriptors(segs)
        assert ops.reparam_plan(d, case.draws, slots, priors=_fake_priors(P.kinds_of(entry, len(segs)), len(segs))) == want
        assert ops.reparam_plan(d, case.draws, slots, priors=[(0, 0)] * len(segs)) == want
        assert ops.reparam_plan(d, case.draws, slots) == want


def test_refusals(lib):
    import ctypes
    from bbb_hip import ops
    h = lib.lib()
    d = C.descriptors((C.Seg(1025), C.Seg(10)))
    assert ops.reparam_plan(d, 2, 2048, priors=[(0x1000, 0x2004), (0, 0x3000)])["chunks"] == 3
    with pytest.raises(lib.BBBHipError, match="one .* pair per segment"):
        ops.reparam_plan(d, 2, 2048, priors=[(0x1000, 0)])
    for bad in ([(0x1001, 0), (0, 0)], [(0, 0), (0, 0x3002)], [(0x1000, 0x2000), (0x1003, 0)]):
        with pytest.raises(lib.BBBHipError, match="EALIGN"):
            ops.reparam_plan(d, 2, 2048, priors=bad)
    # the scalar entry's own refusals come first, and with the same code
    with pytest.raises(lib.BBBHipError, match="EINVAL"):
        ops.reparam_plan(C.descriptors((C.Seg(8), C.tm(4, 8, 1))), 2, 2048, priors=[(0x1001, 0), (0, 0)])
    out = [None] * 8
    segs = (lib.Segment * 17)()
    pri = (lib.PriorSegment * 17)()
    for s in segs:
        s.mu = s.rho = 16
        s.n = s.draw_stride = 8
    assert h.bbb_reparam_kl_tp_plan(segs, pri, 16, 1, 2048, *out) == 0
    assert h.bbb_reparam_kl_tp_plan(segs, None, 16, 1, 2048, *out) == 0
    for nseg in (0, -1, 17, 2 ** 31 - 1):
        assert h.bbb_reparam_kl_tp_plan(segs, pri, nseg, 1, 2048, *out) == C.EINVAL
    pri[15].sigma0 = 0x1002
    assert h.bbb_reparam_kl_tp_plan(segs, pri, 16, 1, 2048, *out) == C.EALIGN
    assert h.bbb_reparam_kl_tp_plan(segs, pri, 15, 1, 2048, *out) == 0          # entries past nseg are not read
    g = ctypes.c_int32(0)
    assert h.bbb_reparam_kl_tp_plan(segs, pri, 15, 1, 2048, None, None, None, None, None, None, None, ctypes.byref(g)) == 0 and g.value == 16


def test_prior_checks_under_the_sanitizers(tmp_path):
    """tests/host/reparam_tp_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: PriorSegment arrays of exactly nseg entries, nseg at and beyond its limits."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "reparam_tp_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "reparam_tp_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    assert int(got["cases"]) >= 200000 and min(int(got[k]) for k in ("scalar", "tensor", "einval", "ealign")) > 1000 and len(got["checksum"]) == 16


def test_wrapper_refuses_bad_prior_tensors(lib):
    from bbb_hip import ops
    mu = [torch.zeros(4, 3), torch.zeros(4)]
    ok = torch.ones(4, 3)
    assert ops._prior_segments(None, mu) is None
    assert ops._prior_segments([(None, None), None], mu) is None
    arr = ops._prior_segments([(ok, None), (None, torch.ones(4))], mu)
    assert arr[0].mu0 == ok.data_ptr() and not arr[0].sigma0 and not arr[1].mu0 and arr[1].sigma0
    for bad, what in (([(ok, None)], "one .* per tensor"), ([(torch.ones(4, 3, requires_grad=True), None), None], "requires a gradient"),
                      ([(torch.ones(5, 3), None), None], "12 elements"), ([(ok.double(), None), None], "fp32"),
                      ([(torch.ones(3, 4).t(), None), None], "contiguous"), ([(1.0, None), None], "float")):
        with pytest.raises(lib.BBBHipError, match=what):
            ops._prior_segments(bad, mu)


# ------------------------------------------------------------------------------------------------ set_prior / bbb_hip.priors (host logic)
def _net():
    import layers
    from layers.misc import ModuleWrapper, FlattenLayer

    class Net(ModuleWrapper):
        def __init__(self):
            super().__init__()
            self.conv1 = layers.BBB_Conv2d(3, 8, 3, padding=1)
            self.act1 = nn.ReLU()
            self.pool1 = nn.MaxPool2d(2, 2)
            self.flatten = FlattenLayer(128)
            self.fc1 = layers.BBB_Linear(128, 12)
            self.act2 = nn.Softplus()
            self.fc2 = layers.BBB_Linear(12, 10)
    torch.manual_seed(3)
    return Net().cpu()


def test_set_prior_validates_and_names_the_layer(lib):
    from bbb_hip import priors
    net = _net()
    l = net.fc1
    for kw, what in ((dict(mu=torch.zeros(12, 127)), r"fc1: prior mu: shape \(12, 127\)"),
                     (dict(sigma=torch.zeros(12, 128)), "fc1: prior sigma: every element must be > 0"),
                     (dict(sigma=torch.full((12, 128), float("nan"))), "fc1: prior sigma: non-finite"),
                     (dict(mu=torch.zeros(12, 128, dtype=torch.float64)), "fc1: prior mu: dtype"),
                     (dict(bias_sigma=-torch.ones(12)), "fc1: prior bias_sigma: every element"),
                     (dict(sigma=0.0), "fc1: prior sigma = 0.0: must be > 0"),
                     (dict(bias_mu=0.5), "fc1: prior bias_mu = 0.5 differs from the layer's prior_mu")):
        with pytest.raises(ValueError, match=what):
            l.set_prior(name="fc1", **kw)
    assert l._prior_lists() is None and not priors.state_dict(net)
    # through bbb_hip.priors the layer's name in the model is given; on its own a layer is called by its class
    with pytest.raises(ValueError, match=r"fc1: prior mu: shape \(3,\)"):
        priors.load_state_dict(net, {"fc1.W_prior_mu": torch.zeros(3)})
    with pytest.raises(ValueError, match="BBBLinear: prior sigma = -1.0"):
        l.set_prior(sigma=-1.0)
    # every argument is validated before anything is applied: a refused call leaves the layer as it was
    from bbb_hip import ensemble
    e0 = ensemble._epoch[0]
    with pytest.raises(ValueError, match="prior sigma: every element"):
        l.set_prior(mu=torch.zeros(12, 128), sigma=torch.zeros(12, 128), name="fc1")
    with pytest.raises(ValueError, match="prior bias_mu"):
        l.set_prior(mu=0.5, sigma=torch.ones(12, 128), bias_mu=torch.zeros(11), name="fc1")
    assert l._prior_lists() is None and l.prior_mu == 0 and ensemble._epoch[0] == e0
    l.set_prior(mu=0.5, bias_mu=0.5)                                 # a bias number is held to the scalar as this call leaves it
    assert l.prior_mu == 0.5
    import layers
    nobias = layers.BBB_Linear(4, 2, bias=False)
    with pytest.raises(ValueError, match="BBBLinear: prior bias_mu: the layer has no bias"):
        nobias.set_prior(bias_mu=torch.zeros(2))


def test_buffers_kinds_and_epoch(lib):
    from bbb_hip import ensemble, priors
    net = _net()
    l = net.conv1
    keys = set(net.state_dict())
    e0 = ensemble._epoch[0]
    l.set_prior(mu=torch.zeros(8, 3, 3, 3), sigma=torch.full((8, 3, 3, 3), 0.5))
    assert ensemble._epoch[0] > e0                                   # number -> tensor: a change of kind
    assert l._prior_lists() == [(l.W_prior_mu, l.W_prior_sigma), (None, None)]
    assert set(net.state_dict()) == keys                             # non-persistent: checkpoints stay the reference's
    assert {n for n, _ in net.named_buffers()} == {"conv1.W_prior_mu", "conv1.W_prior_sigma"}
    e1, ptr = ensemble._epoch[0], l.W_prior_mu.data_ptr()
    l.set_prior(mu=torch.ones(8, 3, 3, 3))
    assert ensemble._epoch[0] == e1 and l.W_prior_mu.data_ptr() == ptr and float(l.W_prior_mu.min()) == 1.0     # in place
    l.set_prior(bias_sigma=torch.full((8,), 0.25))
    e2 = ensemble._epoch[0]
    assert e2 > e1 and l._prior_lists()[1] == (None, l.bias_prior_sigma)
    l.set_prior(bias_sigma=l.prior_sigma)                            # an equal number clears that bias tensor
    assert l.bias_prior_sigma is None and ensemble._epoch[0] > e2
    l.set_prior(sigma=0.2)                                           # tensor -> number
    assert l.prior_sigma == 0.2 and l.W_prior_sigma is None and l.W_prior_mu is not None
    c = copy.deepcopy(net)
    assert torch.equal(c.conv1.W_prior_mu, l.W_prior_mu) and c.conv1.W_prior_mu.data_ptr() != l.W_prior_mu.data_ptr()
    assert c.conv1.prior_sigma == 0.2
    moved = copy.deepcopy(net).to(torch.float32).to("cpu")
    assert moved.conv1.W_prior_mu is not None
    priors.clear(net)
    assert all(l2._prior_lists() is None for _, l2 in priors.named_layers(net)) and l.prior_sigma == 0.2
    e3 = ensemble._epoch[0]
    priors.clear(net)
    assert ensemble._epoch[0] == e3                                  # nothing changed


def test_from_posterior_state_dict_round_trip(lib):
    from bbb_hip import priors
    net, other = _net(), _net()
    with torch.no_grad():
        for p in other.parameters():
            p.add_(0.01)
    priors.from_posterior(net, other)
    for name, l in priors.named_layers(net):
        s = dict(priors.named_layers(other))[name]
        assert torch.equal(l.W_prior_mu, s.W_mu) and torch.equal(l.bias_prior_sigma, torch.nn.functional.softplus(s.bias_rho))
        assert not l.W_prior_mu.requires_grad and l.W_prior_mu.data_ptr() != s.W_mu.data_ptr()
    sd = priors.state_dict(net)
    assert set(sd) == {"%s.%s" % (n, b) for n in ("conv1", "fc1", "fc2") for b in ("W_prior_mu", "W_prior_sigma", "bias_prior_mu", "bias_prior_sigma")}
    ptr = net.fc1.W_prior_mu.data_ptr()
    priors.from_posterior(net)                                       # its own posterior, in place
    assert net.fc1.W_prior_mu.data_ptr() == ptr and torch.equal(net.fc1.W_prior_mu, net.fc1.W_mu)
    fresh = _net()
    priors.load_state_dict(fresh, sd)
    got = priors.state_dict(fresh)
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    part = {k: v for k, v in sd.items() if k.startswith("fc1.W_prior")}
    priors.load_state_dict(fresh, part)                              # covers tensors only: what is absent goes back to the scalar
    assert set(priors.state_dict(fresh)) == set(part)
    with pytest.raises(KeyError, match="unexpected key"):
        priors.load_state_dict(fresh, {"fc9.W_prior_mu": torch.zeros(1)})


def test_moped(lib):
    from bbb_hip import priors
    net = _net()
    det = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2, 2), nn.Flatten(), nn.Linear(128, 12), nn.Softplus(),
                        nn.Linear(12, 10))
    with torch.no_grad():
        det[0].weight[0, 0, 0, 0] = 0.0                              # a pruned weight: |w| clamped at 1e-6 inside the expm1
    priors.moped(net, det, delta=0.1, prior_sigma=1.0)
    for (name, l), d in zip(priors.named_layers(net), (det[0], det[4], det[6])):
        assert torch.equal(l.W_mu, d.weight) and torch.equal(l.W_prior_mu, d.weight) and torch.equal(l.bias_prior_mu, d.bias)
        assert l.W_prior_sigma is None and l.bias_prior_sigma is None and l.prior_sigma == 1.0
        for rho, w in ((l.W_rho, d.weight), (l.bias_rho, d.bias)):
            want = 0.1 * w.detach().abs().clamp_min(1e-6).double()
            got = torch.log1p(torch.exp(rho.detach().double()))
            # fp32 accuracy: rho is rounded once (|rho| 2^-24 absolute = that much relative in softplus(rho) where it is small)
            # behind a few roundings of the product, expm1 and log
            assert torch.isfinite(rho).all() and float(((got - want).abs() / want).max()) <= (float(rho.abs().max()) + 4) * 2.0 ** -24
    named = {n: (d.weight, d.bias) for n, d in (("conv1", det[0]), ("fc1", det[4]), ("fc2", det[6]))}
    other = _net()
    priors.moped(other, named, delta=0.05)
    assert torch.equal(other.fc2.W_prior_mu, det[6].weight)
    with pytest.raises(ValueError, match="conv / linear layers"):
        priors.moped(_net(), nn.Sequential(nn.Linear(3, 3)))
