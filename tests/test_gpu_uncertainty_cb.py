"""The batch-innermost uncertainty reduction (csrc/mc_uncertainty.hip) on the device: ops.mc_uncertainty_cb against float64 on the named
cases of tests/uncertainty_cb_contract.py, every element of all seven outputs, inside DEVICE_FACTOR x the error of the fp32 model -- a
bound taken from the reference and the model (tests/test_uncertainty_cb_cpu.py), never from a kernel; NaN and infinities at exactly the
reference's positions.  Bitwise where one kernel computes both sides: an output asked for alone against the same output asked for with
the others, an image inside a batch of 130 against the same image alone and inside a batch of 65, a GraphedUncertainty replay against
the eager uncertainty.mc_uncertainty from the same generator state.  Model level: mc_uncertainty against the float64 reference on
ensemble.mc_logits of the same seed and calls, and against get_uncertainty_per_batch within the sum of both routes' bounds.
Needs an MI355X: -m gpu."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import ref_port_torch as P
import tail_contract as TC
import uncertainty_cb_contract as K

pytestmark = pytest.mark.gpu
WORST = {}
_REFS = {}


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import _lib, ensemble, ops, rng, uncertainty, zoo
    _lib.lib()
    saved = dict(rng._state)
    yield {"ops": ops, "lib": _lib, "ens": ensemble, "rng": rng, "unc": uncertainty, "zoo": zoo}
    rng._state.clear()
    rng._state.update(saved)
    print("\ndevice, worst |kernel - float64| / scale per output (bound):",
          {k: "%.2f at %s (%g)" % (v[0], v[1], K.bound(k)) for k, v in sorted(WORST.items())})


def _ref(case):
    """(rows [T][B][C], float64 reference) of a contract case, computed once and left unchanged."""
    if case.name not in _REFS:
        rows = K.rows_of(case)
        _REFS[case.name] = (rows, K.reference(rows, case.p["normalized"]))
    return _REFS[case.name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(out):
    return {f: None if t is None else t.cpu().numpy() for f, t in out._asdict().items()}


def _note(field, ratio, name, limit=None):
    """Print the figure, keep the worst, then hold it to the bound."""
    limit = K.bound(field) if limit is None else limit
    print("%s %s: %.3f (bound %g)" % (name, field, ratio, limit))
    if limit == K.bound(field) and ratio > WORST.get(field, (-1.0, ""))[0]:
        WORST[field] = (ratio, name)
    assert ratio <= limit, (name, field, ratio)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_case_within_bounds_all_outputs_and_each_alone(env, case):
    ops = env["ops"]
    rows, ref = _ref(case)
    norm = case.p["normalized"]
    x = _dev(TC.layout(case, rows))
    got = _np(ops.mc_uncertainty_cb(x, normalized=norm))
    for f in K.FIELDS:
        assert got[f].shape == ((case.B, case.C) if f in K.PER_CLASS else (case.B,)) and got[f].dtype == np.float32
        _note(f, K.field_ratio(f, got[f], ref[f], rows), case.name)
    for f in K.FIELDS:                                   # asked for alone: the same bits, hence inside the same bound
        alone = ops.mc_uncertainty_cb(x, normalized=norm, want=(f,))
        assert [g for g, t in alone._asdict().items() if t is not None] == [f]
        a = getattr(alone, f).cpu().numpy()
        assert _same_bits(a, got[f]), (case.name, f)
        assert K.field_ratio(f, a, ref[f], rows) <= K.bound(f)
    # the device's own entropy identity, and a mutual information that is never negative
    mi, nan = got["mutual_info"], np.isnan(ref["mutual_info"])
    assert (mi[~nan] >= 0).all(), case.name
    slack = (K.bound("entropy") + K.bound("expected_entropy") + K.bound("mutual_info")) * K.U * (1.0 + np.log(case.C))
    d = np.abs(got["entropy"].astype(np.float64) - got["expected_entropy"] - mi)[~nan]
    if d.size:
        print("%s |entropy - expected_entropy - mutual_info|: %.3g (bound %.3g)" % (case.name, d.max(), slack))
        assert d.max() <= slack, case.name
    if case.slabs == 1:
        assert not got["epistemic"].any() and not mi.any(), case.name
    if case.C == 1:
        assert not got["entropy"].any() and not got["expected_entropy"].any() and not mi.any(), case.name


def test_the_plan_limit_is_refused_by_name(env):
    ops, lib = env["ops"], env["lib"]
    x = torch.zeros((K.MAX_DRAWS + 1, 3, 4), device="cuda")
    with pytest.raises(lib.BBBHipError, match="BBB_ESHAPE"):
        ops.mc_uncertainty_cb(x)
    with pytest.raises(lib.BBBHipError, match="want must name"):
        ops.mc_uncertainty_cb(x[:2], want=("variance",))
    with pytest.raises(lib.BBBHipError, match="want must name"):
        ops.mc_uncertainty_cb(x[:2], want=())


@pytest.mark.parametrize("normalized", [False, True], ids=["softmax", "normalized"])
def test_an_image_does_not_depend_on_its_batch(env, normalized):
    """Image b of a launch of 130 = the same image alone = the same image inside a launch of 65, bit for bit, all seven outputs."""
    ops = env["ops"]
    case = TC.Case("identity", K.ENTRY, "gauss4", 10, 17, 130, 0, (("normalized", normalized),))
    x = _dev(TC.layout(case, TC.rows_of(case)))                        # [T][C][B]
    full = _np(ops.mc_uncertainty_cb(x, normalized=normalized))
    for lo, hi in ((0, 65), (65, 130), (0, 1), (63, 64), (64, 65), (129, 130)):
        part = _np(ops.mc_uncertainty_cb(x[:, :, lo:hi].contiguous(), normalized=normalized))
        for f in K.FIELDS:
            assert _same_bits(part[f], full[f][lo:hi]), (f, lo, hi)


# ---------------------------------------------------------------- model level
def _model(env, net_type, lt, cin, B=8):
    torch.manual_seed(3)
    net = env["zoo"].getModel(net_type, cin, 10, P.CONFIG_PRIORS, lt, "softplus").cuda()
    env["rng"].assign_stream_ids(net)
    return net, torch.rand(B, cin, 32, 32, device="cuda")


# (the zoo's LeNet has no padding and flattens 5 x 5 x 16: it takes 32 x 32 images, as everywhere in this suite)
# (B = 6: the forward pads the batch to a multiple of 4 and hands back a view of its buffer, which is compacted before the launch)
MODELS = [("lenet", "bbb", 1, "fp32", False, 8), ("lenet", "lrt", 1, "fp32", True, 8), ("3conv3fc", "bbb", 3, "fp32", False, 8),
          ("3conv3fc", "lrt", 3, "fp32", False, 8), ("3conv3fc", "bbb", 3, "bf16x3", False, 8), ("lenet", "bbb", 1, "fp32", False, 6)]


@pytest.mark.parametrize("net_type,lt,cin,precision,normalized,B", MODELS)
def test_mc_uncertainty_on_models(env, net_type, lt, cin, precision, normalized, B):
    ens, rng, unc = env["ens"], env["rng"], env["unc"]
    net, x = _model(env, net_type, lt, cin, B)
    T = 5
    rng.manual_seed(1234, call=10)
    out = unc.mc_uncertainty(net, x, T=T, normalized=normalized, precision=precision)
    assert isinstance(out, env["ops"].Uncertainty) and all(t.is_cuda for t in out)
    assert ens.stats["path"] == "chwn" and rng.get_state() == (1234, 10 + T)
    got = _np(out)
    with torch.no_grad():
        logits, _ = ens.mc_logits(net, x, T, 1234, 10, precision=precision)                  # [T, B, C], the same seed and calls
    rows = logits.cpu().numpy()
    ref = K.reference(rows, normalized)
    assert got["pred"].shape == (B, 10) and got["entropy"].shape == (B,)
    name = "%s-%s-%s%s-B%d" % (net_type, lt, precision, "-norm" if normalized else "", B)
    for f in K.FIELDS:
        _note(f, K.field_ratio(f, got[f], ref[f], rows), name)
    if precision != "fp32":
        return
    # the reference-mirroring route from the same generator state: another summation order, so the sum of both routes' bounds
    rng.manual_seed(1234, call=10)
    old = dict(zip(("pred", "epistemic", "aleatoric"), unc.get_uncertainty_per_batch(net, x.cpu(), T=T, normalized=normalized)))
    assert rng.get_state() == (1234, 10 + T)
    for f, op in (("pred", "pred"), ("epistemic", "epi"), ("aleatoric", "ale")):
        _note(f, K.field_ratio(f, got[f], old[f].astype(np.float64), rows), name + " vs get_uncertainty_per_batch", K.bound(f) + TC.bound(op))


def test_get_uncertainty_per_batch_keeps_its_bits_around_mc_uncertainty(env):
    rng, unc = env["rng"], env["unc"]
    net, x = _model(env, "lenet", "bbb", 1)
    rng.manual_seed(99, call=7)
    before = unc.get_uncertainty_per_batch(net, x, T=5)
    rng.manual_seed(99, call=7)                                          # the generator state saved above, restored around the new call
    unc.mc_uncertainty(net, x, T=5)
    assert rng.get_state() == (99, 12)
    rng.manual_seed(99, call=7)
    after = unc.get_uncertainty_per_batch(net, x, T=5)
    assert all(isinstance(a, np.ndarray) and _same_bits(a, b) for a, b in zip(after, before)) and len(after) == 3


# ---------------------------------------------------------------- captured form
def _clone(out):
    return type(out)(*[t.clone() for t in out])


def _equal(a, b):
    return all(torch.equal(s.view(torch.int32), t.view(torch.int32)) for s, t in zip(a, b))


@pytest.mark.parametrize("lt,normalized", [("bbb", False), ("lrt", True)])
def test_graphed_uncertainty_replays_are_the_eager_calls(env, lt, normalized):
    rng, unc = env["rng"], env["unc"]
    net, _ = _model(env, "lenet", lt, 1)
    T = 5
    xs = [torch.rand(8, 1, 32, 32, device="cuda") for _ in range(3)]
    rng.manual_seed(77, call=100)
    eager = [_clone(unc.mc_uncertainty(net, xb, T=T, normalized=normalized)) for xb in xs]
    assert not _equal(eager[0], eager[1])
    rng.manual_seed(77, call=100)
    g = unc.GraphedUncertainty(net, xs[0], T, normalized=normalized)
    assert rng.get_state() == (77, 100)                                  # building it consumes no noise call
    for xb, want in zip(xs, eager):
        assert _equal(g.step(xb), want)
    assert rng.get_state() == (77, 100 + 3 * T)
    with torch.no_grad():
        net(xs[0])                                                       # a validation forward moves the noise: one call
    seed_call = rng.get_state()
    assert seed_call == (77, 100 + 3 * T + 1)
    want = _clone(unc.mc_uncertainty(net, xs[1], T=T, normalized=normalized))
    rng.manual_seed(seed_call[0], call=seed_call[1])
    assert _equal(g.step(xs[1]), want) and not _equal(want, eager[1])
    seed_call = rng.get_state()
    want = _clone(unc.mc_uncertainty(net, xs[1], T=T, normalized=normalized))
    rng.manual_seed(seed_call[0], call=seed_call[1])
    assert _equal(g.step(), want)                                        # no batch given: the one it holds
    rng.manual_seed(5, call=0)
    with pytest.raises(env["lib"].BBBHipError, match="noise seed changed"):
        g.step()
    assert rng.get_state() == (5, 0)


def test_two_graphed_uncertainties_with_different_launch_configs_coexist(env):
    ops, rng, unc = env["ops"], env["rng"], env["unc"]
    net, x = _model(env, "3conv3fc", "bbb", 3)
    T = 5
    split = ops.LaunchConfig(gemm_mode="bf16x3", bf16x3_min_workgroups=0)
    rng.manual_seed(31, call=8)
    want32 = _clone(unc.mc_uncertainty(net, x, T=T))
    rng.manual_seed(31, call=8)
    with ops.use_config(split):
        want16 = _clone(unc.mc_uncertainty(net, x, T=T))
    assert not _equal(want32, want16)                                    # the two configurations really are different arithmetic
    rng.manual_seed(31, call=8)
    g32 = unc.GraphedUncertainty(net, x, T)
    g16 = unc.GraphedUncertainty(net, x, T, launch_config=split)
    for _ in range(2):                                                   # replayed alternately, no synchronisation in between
        rng.manual_seed(31, call=8)
        a = _clone(g32.step())
        rng.manual_seed(31, call=8)
        b = _clone(g16.step())
        assert _equal(a, want32) and _equal(b, want16)
    assert ops.current_config().gemm_mode == "fp32"


class _Hidden(nn.Module):
    """A Bayesian layer inside a module with a forward of its own: ensemble.flat_children rejects the model."""

    def __init__(self):
        super().__init__()
        from layers import BBB_Linear
        self.fc = BBB_Linear(12, 5, bias=True, priors=P.CONFIG_PRIORS)

    def forward(self, x):
        return self.fc(x.flatten(1))


def test_off_the_fast_path_eager_runs_and_the_graph_refuses(env):
    ens, rng, unc = env["ens"], env["rng"], env["unc"]
    from layers import ModuleWrapper
    torch.manual_seed(4)
    net = ModuleWrapper()
    net.add_module("block", _Hidden())
    net = net.cuda()
    rng.assign_stream_ids(net)
    x = torch.rand(8, 3, 2, 2, device="cuda")
    with pytest.raises(env["lib"].BBBHipError, match="batch-innermost inference path only"):
        unc.GraphedUncertainty(net, x, 4)
    rng.manual_seed(8, call=2)
    got = _np(unc.mc_uncertainty(net, x, T=4))
    assert ens.stats["path"] == "loop" and rng.get_state() == (8, 6)
    with torch.no_grad():
        logits, _ = ens.mc_logits(net, x, 4, 8, 2)
    rows = logits.cpu().numpy()
    ref = K.reference(rows, False)
    for f in K.FIELDS:
        _note(f, K.field_ratio(f, got[f], ref[f], rows), "hidden-layer model")
