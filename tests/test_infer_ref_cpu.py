"""The reference of tests/test_gpu_infer_walk_ref.py checked on its own, without a device: tests/infer_ref.py against the oracle's zoo
forward, its partition rule against hand-written tables, and the cases of tests/infer_walk_cases.py for the conditions that give the
GPU comparison teeth -- the plans they are to reach (all of them, together: every form of the walk), wrong answers far from right
ones (another slab, the next noise call, the neighbouring batch block, a neighbouring image offset), every logit depending on every
input channel, activations on both sides of 0.  Needs the built library for the host-only plan helpers, as test_infer_plan_cpu.py."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn

import bbb_numpy as O
import bf16_lrt_contract as LC
import infer_ref as IR
import infer_schedule_recorder as R
import infer_walk_cases as C

PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}
LENET = ("conv1", "conv2", "fc1", "fc2", "fc3")


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import ensemble, ops, rng, zoo
    return dict(ens=ensemble, ops=ops, rng=rng, zoo=zoo)


def _ratio(a, b):
    return float((a.double() - b.double()).abs().max()) / float(b.double().abs().max())


# ---- the reference against the oracle ------------------------------------------------------------------------------------------
def _lenet(env, kind):
    torch.manual_seed(3)
    net = env["zoo"].getModel("lenet", 1, 10, PRIORS, kind, "softplus")
    env["rng"].assign_stream_ids(net)
    params = {"_prior_mu": 0, "_prior_sigma": 0.1}
    for name in LENET:
        m = getattr(net, name)
        params[name] = {k: getattr(m, k).detach().numpy() for k in ("W_mu", "W_rho", "bias_mu", "bias_rho")}
    x = torch.rand((4, 1, 32, 32), generator=torch.Generator().manual_seed(4))
    seed, call = 2026, 9

    def eps_fn(name, what, shape):
        sid = getattr(net, name)._stream_base + {"W": 0, "bias": 1, "act": 2}[what]
        return O.normal_eps(seed, call, sid, int(np.prod(shape))).reshape(shape)
    return net, params, x, seed, call, eps_fn


@pytest.mark.parametrize("kind", ["bbb", "lrt"])
def test_forward64_is_the_oracles_zoo_forward(env, kind):
    net, params, x, seed, call, eps_fn = _lenet(env, kind)
    want, kl = O.model_forward("lenet", params, x.numpy(), kind, "softplus", eps_fn)
    want = torch.from_numpy(want)
    # value for value with the oracle's fp32 holds restated ...
    assert _ratio(IR.forward64(net, x, seed, call, rounding="fp32"), want) <= 1e-12
    # ... and, all in float64, within what five layers of fp32 holds can move a logit (a few 2^-24 per hold)
    assert _ratio(IR.forward64(net, x, seed, call), want) <= 2e-6
    assert _ratio(IR.forward64(net, x, seed, call, dtype=torch.float32), want) <= 1e-5
    assert abs(IR.kl64(net) - kl) <= 1e-12 * kl


@pytest.mark.parametrize("kind", ["bbb", "lrt"])
def test_bf16_rounding_is_the_oracles_storage_contract(env, kind):
    net, params, x, seed, call, eps_fn = _lenet(env, kind)
    if kind == "bbb":
        want, _ = O.model_forward_bf16("lenet", params, x.numpy(), "softplus", eps_fn)
    else:
        want = LC.model_forward("lenet", params, x.numpy(), "softplus", eps_fn)
    got = IR.forward64(net, x, seed, call, rounding="bf16")
    assert _ratio(got, torch.from_numpy(want)) <= 1e-12
    assert _ratio(got, IR.forward64(net, x, seed, call)) > 1e-4              # (the roundings are there)


def test_bf16_rounding_of_an_average_pool_is_the_avgpool_contracts(env):
    """tests/bf16_avgpool_contract.py (float64 torch, no fp32 holds; weights sampled in float64, then rounded) on a model with a padded
    average pool and a global-average-pool head: the average pool's result rounds once more.  The two restatements differ by the fp32
    holds (a few 2^-24 per stage) unless one of them flips a bf16 rounding, which none does on this model: 1e-5."""
    import bf16_avgpool_contract as AC
    from layers import BBB_Conv2d, BBB_Linear, FlattenLayer, ModuleWrapper
    torch.manual_seed(11)
    net = ModuleWrapper()
    mods = [("c1", BBB_Conv2d(3, 8, 3, stride=1, padding=1, priors=PRIORS)), ("a1", nn.ReLU()),
            ("p1", nn.AvgPool2d((3, 2), (2, 1), (1, 0), count_include_pad=False)),
            ("c2", BBB_Conv2d(8, 8, 3, stride=1, padding=1, priors=PRIORS)), ("a2", nn.Softplus()), ("p2", nn.AdaptiveAvgPool2d(1)),
            ("fl", FlattenLayer(8)), ("fc", BBB_Linear(8, 10, priors=PRIORS))]
    for name, m in mods:
        net.add_module(name, m)
    env["rng"].assign_stream_ids(net)
    x = torch.rand((4, 3, 10, 9), generator=torch.Generator().manual_seed(12)) * 2 - 1
    seed, call = 77, 3
    plan = [dict(name="c1", kind="conv", stride=1, padding=1, act="relu", pool=((3, 2), (2, 1), (1, 0), False)),
            dict(name="c2", kind="conv", stride=1, padding=1, act="softplus", pool=((5, 8), (5, 8), (0, 0), True), flat=8),
            dict(name="fc", kind="fc")]
    params, eps = {}, {}
    for name in ("c1", "c2", "fc"):
        m = getattr(net, name)
        params[name] = {k: getattr(m, k).detach().numpy() for k in ("W_mu", "W_rho", "bias_mu", "bias_rho")}
        eps[name] = {"W": O.normal_eps(seed, call, m._stream_base, m.W_mu.numel()).reshape(tuple(m.W_mu.shape)),
                     "bias": O.normal_eps(seed, call, m._stream_base + 1, m.bias_mu.numel())}
    _, (want,) = AC.forward(plan, params, x.numpy(), [eps])
    got = IR.forward64(net, x, seed, call, rounding="bf16")
    assert got.shape == want.shape and _ratio(got, want) <= 1e-5
    assert _ratio(got, IR.forward64(net, x, seed, call)) > 1e-4              # (the roundings are there)


def test_lrt_noise_is_keyed_by_the_global_image(env):
    """A block of a batch at its offset is the rows of the whole batch, also behind a flatten that cuts every image into rows."""
    for name in ("chain", "quirk"):
        net, x = C.build(name, "lrt"), C.table_x(name, 8)
        whole = IR.forward64(net, x, 3, 4, b_offset=5)
        r = whole.shape[0] // 8
        part = IR.forward64(net, x[4:], 3, 4, b_offset=9)
        assert torch.equal(part, whole[4 * r:])
        assert _ratio(IR.forward64(net, x[4:], 3, 4, b_offset=5), whole[4 * r:]) > 1e-2


# ---- the partition rule --------------------------------------------------------------------------------------------------------
def test_slab_sources_tables():
    """Hand-written from the chwn_partition docstring for the recorder's four partitions (B = 16 in x, two draws, call0 = 5)."""
    shape, B = (16, 3, 8, 8), 16
    assert IR.slab_sources((8, 3, 8, 8), 2, 5) == [(0, 8, 5, 0), (0, 8, 6, 0)]
    assert IR.slab_sources((8, 3, 8, 8), 2, 5, b_offset=8) == [(0, 8, 5, 8), (0, 8, 6, 8)]
    assert IR.slab_sources((6, 3, 8, 8), 2, 5) == [(0, 6, 5, 0), (0, 6, 6, 0)]
    # units (2, 1, 3): unit 1 = draw 0, slice 1; unit 2 = draw 1, slice 0
    assert IR.slab_sources(shape, 2, 5, **{k: v for k, v in R.PARTS["units"].items() if k != "B"}) == [(8, 16, 5, 8), (0, 8, 6, 0)]
    assert IR.slab_sources(shape, 2, 5, units=(2, 1, 3), b_offset=16) == [(8, 16, 5, 24), (0, 8, 6, 16)]
    # two steps of two draws: calls 5..8, batch 0 twice, then batch 1 twice
    assert IR.slab_sources(shape, 2, 5, groups=R.PARTS["groups"]["groups"]) == [(0, 8, 5, 0), (0, 8, 6, 0), (8, 16, 7, 0), (8, 16, 8, 0)]
    # a share (2, 1): slab 0 = draw 1 of step 0, slab 1 = draw 0 of step 1
    assert IR.slab_sources(shape, 2, 5, share=R.PARTS["share"]["share"]) == [(0, 8, 5, 0), (8, 16, 6, 0)]
    assert IR.slab_sources((24, 3, 8, 8), 4, 5, share=(2, 1), b_offset=3) == [(0, 8, 5, 3), (8, 16, 6, 3), (8, 16, 7, 3), (16, 24, 8, 3)]
    assert IR.slab_sources((8, 3, 8, 8), 2, 5, **{k: v for k, v in R.PARTS["streams2"].items() if k != "streams"}) == \
        IR.slab_sources((8, 3, 8, 8), 2, 5)
    assert B == R.PARTS["units"]["B"] == R.PARTS["groups"]["B"] == R.PARTS["share"]["B"]


# ---- the plans -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(env):
    cache = {}

    def get(run):
        key = (run["source"], run["model"], run["kind"])
        if key not in cache:
            cache[key] = C.run_model(run)[0]
        return cache[key]
    return get


def test_every_run_has_its_expected_plan(env, nets):
    """The planner names today what tests/golden/infer_walk_plans.json expects of every run (the GPU module asserts the same in front
    of every launch): a planner change that moves a run off its form fails here first."""
    runs, want = C.runs(), C.expected_plans()
    assert sorted(runs) == sorted(want) and len(runs) >= 150
    assert sum(r["source"] == "recorded" for r in runs.values()) == 45 and set(R.cases()) <= set(runs)
    for rid, run in runs.items():
        assert C.plan_of(run, nets(run)) == want[rid], rid
    assert want["fallback"] is None
    for rid, run in runs.items():
        if run.get("refusal") and run["refusal"][0] == "mc_logits":
            assert want[rid] is None, rid
    for rid, forms in C.INTENT.items():                      # what the table was written to reach, by hand
        assert [s[0] for s in want[rid]] == forms.split(), rid


def test_the_runs_reach_every_form_of_the_walk(env):
    ens = env["ens"]
    plans = {rid: p for rid, p in C.expected_plans().items() if isinstance(p, list)}
    steps = [tuple(map(lambda v: tuple(map(str, v)) if isinstance(v, list) else v, s)) for p in plans.values() for s in p]
    forms = {s[0] for s in steps}
    assert forms >= set(ens.BAYES_FORMS) | {"pool", "avgpool", "to_f32", "to_c8s3", "flatten", "relu", "softplus"}
    for form in ("fp32_lrt", "bf16_lrt"):                           # (the forms that have a shared_in)
        assert {s[4] for s in steps if s[0] == form} == {False, True}, form
    # a stand-alone max pool with a window other than (2, 2) in every layout the planner can place one in.  "bf16c8" is not among them:
    # the planner chooses the channel-interleaved layout only where a BBB convolution follows the pooled launch directly
    windows = {lay: {s[3] for s in steps if s[0] == "pool" and s[1] == lay} - {("2", "2")} for lay in ("f32", "s3", "c8s3", "bf16")}
    assert all(windows.values()), windows
    assert not any(s[0] == "pool" and s[1] == "bf16c8" for s in steps)
    assert {s[1] for s in steps if s[0] == "avgpool"} == {"f32", "bf16"}
    behind = {p[k - 1][1] for p in plans.values() for k, s in enumerate(p) if s[0] == "avgpool" and k and p[k - 1][0] == "to_f32"}
    assert behind == {"s3", "c8s3"}
    assert {s[1] for s in steps if s[0] == "to_f32"} == {"s3", "c8s3"}
    rows_lrt = [p for p in plans.values() for k, s in enumerate(p) if s[0] == "flatten" and s[5]
                and any(t[0] in ("fp32_lrt", "c8x3_lrt") for t in p[k + 1:k + 3])]
    assert rows_lrt
    fused = {s[0]: set() for s in steps}
    for s in steps:
        if s[0] in ens.BAYES_FORMS and s[3] is not None:
            fused[s[0]].add(s[3])
    assert fused["fp32_bbb"] and fused["s2d_bbb"] and fused["bf16_bbb"] - {("2", "2")}
    assert any(s[0] == "bf16_bbb" and s[2] == "bf16c8" for s in steps)      # out_c8
    # tap-major weight rows for some layers of a run and not for others: the draws of the MFMA-ready chain beside dense ones (a run
    # with a c8x3_bbb convolution and an fp32_bbb layer), and the bf16 rows (ChwnStep.tap_major) in both states in one run
    assert any({"c8x3_bbb", "fp32_bbb"} <= {s[0] for s in p} for p in plans.values())
    for form in ("bf16_bbb", "bf16_lrt"):
        assert any({s[6] for s in p if s[0] == form} == {False, True} for p in plans.values()), form
    # the models that mix BBB and LRT layers
    assert any({"fp32_bbb", "fp32_lrt"} <= {s[0] for s in p} for p in plans.values())


def test_table_models_hold_what_the_issue_lists(env):
    ens, ops = env["ens"], env["ops"]
    mods = {(n, k): ens.flat_children(C.build(n, k)) for n, spec in C.MODELS.items() for k in spec["kinds"]}
    convs = [m for (n, k), ms in mods.items() if k != "lrt" for m in ms if hasattr(m, "kernel_size") and hasattr(m, "W_mu")]
    pair = ops._pair
    assert {(3, 5), (5, 1), (1, 1)} <= {tuple(m.kernel_size) for m in convs}
    assert {2, 3} <= {pair(m.stride)[1] for m in convs} and {2, 3} <= {pair(mods[n, "bbb"][0].stride)[0] for n in ("chain", "stride")}
    assert any(pair(m.dilation) == (2, 2) for m in convs)
    assert any(pair(m.padding)[0] > pair(m.dilation)[0] * (m.kernel_size[0] - 1) for m in convs)
    pools = {(m.kernel_size, m.stride) for ms in mods.values() for m in ms if isinstance(m, nn.MaxPool2d)}
    assert {(3, 2), (3, 1), (2, 3)} <= pools
    trace, cut = [], []                                      # a window that floor mode cuts, rows and columns
    IR.forward64(C.build("rect", "bbb"), C.table_x("rect", 8), C.SEED, C.CALL0, trace=trace)
    for k, (m, out) in enumerate(trace):
        if isinstance(m, nn.MaxPool2d):
            H, W = trace[k - 1][1].shape[2:]
            cut.append(((H - m.kernel_size) % m.stride != 0, (W - m.kernel_size) % m.stride != 0))
    assert (True, True) in cut, cut
    assert any(isinstance(m, nn.AvgPool2d) and not m.count_include_pad for ms in mods.values() for m in ms)
    assert any(isinstance(m, nn.AdaptiveAvgPool2d) for ms in mods.values() for m in ms)
    for kind in ("bbb", "lrt"):
        assert any(not m.use_bias for (n, k), ms in mods.items() if k == kind for m in ms if hasattr(m, "use_bias"))
        assert any(len({m.prior_sigma for m in ms if hasattr(m, "prior_sigma")}) > 1 for (n, k), ms in mods.items() if k == kind)
        assert any(sum(1 + m.use_bias for m in ms if hasattr(m, "use_bias")) > 16 for (n, k), ms in mods.items() if k == kind)
    m0, spec = mods["s2d", "bbb"][0], C.MODELS["s2d"]
    assert ops.s2d_layer_ok(m0.in_channels, m0.out_channels, m0.kernel_size, m0.stride, m0.padding, m0.dilation, spec["H"], spec["W"])
    assert all(spec["H"] != spec["W"] and spec["H"] <= 20 and spec["W"] <= 18 for spec in C.MODELS.values())
    assert {spec["E"] for spec in C.MODELS.values()} == {1, 2, 3} and {spec["B"] for spec in C.MODELS.values()} == {6, 8}


# ---- the conditions that give the bounds teeth -----------------------------------------------------------------------------------
def _combos():
    """The runs by what the reference depends on -> {key: (a run, the widest separation any of its precisions asks for)}."""
    out = {}
    for rid, run in C.runs().items():
        if run.get("refusal"):
            continue                                         # (nothing is compared there)
        key = (run["source"], run["model"], run["kind"], run["draws"], run["B"], tuple(sorted((k, str(v)) for k, v in run["kw"].items())))
        need = C.separation(run)
        out[key] = (run, max(need, out.get(key, (None, 0.0))[1]))
    return out


@pytest.fixture(scope="module")
def refs(env):
    cache = {}

    def ref(run, i0, i1, call, boff):
        key = (run["source"], run["model"], run["kind"], run["B"], i0, i1, call, boff)
        if key not in cache:
            net, x = _model(run)
            cache[key] = IR.forward64(net, x[i0:i1], C.SEED, call, b_offset=boff)
        return cache[key]
    models = {}

    def _model(run):
        key = (run["source"], run["model"], run["kind"], run["B"])
        if key not in models:
            models[key] = C.run_model(run)
        return models[key]
    ref.model = _model
    return ref


@pytest.mark.parametrize("key", list(_combos()), ids=lambda k: "-".join(map(str, k[:5])) + ("-" + "-".join(v for _, v in k[5]) if k[5] else ""))
def test_wrong_slabs_lie_far_from_right_ones(refs, key):
    run, need = _combos()[key]
    kw = {k: v for k, v in run["kw"].items() if k in ("units", "groups", "share", "b_offset")}
    slabs = IR.slab_sources(C.x_shape(run), run["draws"], C.CALL0, **kw)
    want = [refs(run, *s) for s in slabs]
    far = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    worst = []
    for (a, sa), (b, sb) in itertools.combinations(zip(want, slabs), 2):
        assert sa != sb
        worst.append(("slabs", far(a, b)))
    blocks = sorted({s[:2] for s in slabs})
    for w, (i0, i1, call, boff) in zip(want, slabs):
        for other in (call - 1, call + 1):
            worst.append(("call", far(refs(run, i0, i1, other, boff), w)))
        for j0, j1 in blocks:
            if (j0, j1) != (i0, i1):
                worst.append(("block", far(refs(run, j0, j1, call, boff), w)))
        if C.has_lrt(run):                                   # the same images counted from a neighbouring offset
            worst.append(("offset", far(refs(run, i0, i1, call, boff + (i1 - i0)), w)))
    low = min(worst, key=lambda t: t[1])
    print(f"[separation] {key[0]} {key[1]}-{key[2]}: closest wrong answer {low[0]} at {low[1]:.3e}, needed {need:.1e}")
    assert low[1] >= need, (low, need)


def _models():
    return sorted({(k[0], k[1], k[2]) for k in _combos()})


@pytest.mark.parametrize("source,model,kind", _models())
def test_every_logit_lives_on_every_input_channel(refs, source, model, kind):
    run = next(r for k, (r, n) in _combos().items() if k[:3] == (source, model, kind) and not r["kw"])
    net, x, need = *refs.model(run), C.LIVENESS
    want = IR.forward64(net, x, C.SEED, C.CALL0)
    scale = float(want.abs().max())
    for c in range(x.shape[1]):
        xz = x.clone()
        xz[:, c] = 0
        moved = (IR.forward64(net, xz, C.SEED, C.CALL0) - want).abs().max(dim=0).values / scale
        assert float(moved.min()) >= need, (c, moved, need)


@pytest.mark.parametrize("name,kind", [(n, k) for n, spec in C.MODELS.items() for k in spec["kinds"]])
def test_table_models_exercise_their_edges(name, kind):
    """On the reference's intermediate activations: no ReLU plane is dead, every Softplus sees both signs, and every pool that stands
    behind no activation (a max pool mistaken about its window, an average pool about its zero padding) reads negative values."""
    net, x = C.build(name, kind), C.table_x(name, C.MODELS[name]["B"])
    trace = []
    IR.forward64(net, x, C.SEED, C.CALL0, trace=trace)
    assert float(x.min()) < 0 < float(x.max())
    for k, (m, out) in enumerate(trace):
        inp = trace[k - 1][1] if k else x
        if isinstance(m, nn.ReLU):
            alive = (out > 0).flatten(2).any(dim=2).any(dim=0) if out.dim() == 4 else (out > 0).any()
            assert bool(alive.all()), (k, alive)            # (a plane of a map; behind a linear layer: the layer)
        if isinstance(m, nn.Softplus):
            assert float(inp.min()) < 0 < float(inp.max()), k
        if isinstance(m, (nn.MaxPool2d, nn.AvgPool2d)) and not isinstance(trace[k - 1][0], (nn.ReLU, nn.Softplus)):
            assert float(inp.min()) < 0, k
    if name in ("alone", "stride"):
        assert any(isinstance(m, (nn.MaxPool2d, nn.AvgPool2d)) and not isinstance(trace[k - 1][0], (nn.ReLU, nn.Softplus))
                   for k, (m, _) in enumerate(trace))
