"""The pure parts of the batch-innermost inference forward, without a device: ensemble.chwn_partition (how a call is cut into
work units / steps per launch / shares) against a brute-force enumeration, and ensemble.chwn_plan (which launch every layer takes)
against shapes restated with torch.nn.functional on zero CPU tensors."""
import itertools
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import infer_schedule_recorder as R
import test_strided_train_cpu as ST

PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import ensemble, ops, zoo, _lib
    return dict(ens=ensemble, ops=ops, zoo=zoo, err=_lib.BBBHipError)


# ---- the partition ---------------------------------------------------------------------------------------------------------
def _slab_reads(p, e):
    """The input block the first layer's slab e reads, from the record alone."""
    if p.ukw:
        return (p.ukw["units"][1] + e) % p.S
    return (e + p.x_off) // p.x_div if p.x_div > 1 else (e if p.nblk > 1 else 0)


@pytest.mark.parametrize("bf16", [False, True])
def test_units_are_the_draw_major_grid(env, bf16):
    part = env["ens"].chwn_partition
    for draws, S in itertools.product((1, 2, 3), (2, 4)):
        for lo, hi in itertools.combinations(range(draws * S + 1), 2):
            p = part((8 * S, 3, 8, 8), draws, 10, bf16, units=(S, lo, hi), streams=3)
            grid = [(u // S, u % S) for u in range(lo, hi)]                       # unit u is draw u // S, slice u % S
            assert (p.E, p.B, p.S, p.nblk, p.streams, p.pad) == (hi - lo, 8, S, S, 1, 0)
            assert p.call0 == 10 + grid[0][0] and p.n_draws == len({j for j, _ in grid})
            assert p.ukw["n_units"] == hi - lo
            for e, (j, s) in enumerate(grid):
                assert _slab_reads(p, e) == s and (p.ukw["units"][1] + e) // S == j - grid[0][0]


def test_a_share_reads_the_batches_it_touches(env):
    part = env["ens"].chwn_partition
    for D, draws in itertools.product((1, 2, 3), (1, 2, 3, 5)):
        for off in range(D):
            batches = [(e + off) // D for e in range(draws)]                       # slab e of a share reads batch (e + off) // D
            n = batches[-1] + 1
            p = part((4 * n, 3, 8, 8), draws, 10, share=(D, off), streams=2)
            assert (p.E, p.B, p.S, p.n_draws, p.call0, p.nblk, p.streams, p.ukw) == (draws, 4, 1, draws, 10, n, 1, {})
            assert [_slab_reads(p, e) for e in range(draws)] == batches


def test_groups_run_consecutive_steps(env):
    part = env["ens"].chwn_partition
    for G, draws in itertools.product((2, 3), (1, 2, 3)):
        p = part((8 * G, 3, 8, 8), draws, 10, True, groups=G, streams=2)
        assert (p.E, p.B, p.S, p.n_draws, p.call0, p.nblk, p.streams, p.ukw) == (G * draws, 8, 1, G * draws, 10, G, 1, {})
        for g, j in itertools.product(range(G), range(draws)):                     # slab g * draws + j reads batch g (call call0 + slab)
            assert _slab_reads(p, g * draws + j) == g


def test_plain_and_odd_batches(env):
    part = env["ens"].chwn_partition
    p = part((8, 3, 8, 8), 3, 10, streams=2)
    assert tuple(p) == (3, 8, 1, 3, 10, 1, 1, 0, {}, 2, 0)
    assert part((8, 3, 8, 8), 3, 10, units=(1, 0, 3))[:9] == p[:9]
    assert part((6, 3, 8, 8), 3, 10)[:2] == (3, 8) and part((6, 3, 8, 8), 3, 10).pad == 2
    assert part((5, 3, 8, 8), 1, 0).pad == 3 and part((6, 3, 8, 8), 1, 0, True).pad == 0


REFUSALS = [
    (dict(groups=2, units=(2, 0, 2)), "several steps per launch and work units do not combine"),
    (dict(groups=3), "several steps per launch: every batch must hold a multiple of 4 (bf16: 8) images"),
    (dict(groups=2, bf16=True), "several steps per launch: every batch must hold a multiple of 4 (bf16: 8) images"),
    (dict(share=(2, 0), groups=2), "a share of a group of steps combines with neither work units nor whole groups"),
    (dict(share=(2, 0), units=(2, 0, 2)), "a share of a group of steps combines with neither work units nor whole groups"),
    (dict(share=(2, 2)), "share of a group of steps: x must hold the batches it touches, multiples of 4 (bf16: 8) images"),
    (dict(share=(1, 0)), "share of a group of steps: x must hold the batches it touches, multiples of 4 (bf16: 8) images"),
    (dict(units=(4, 0, 2)), "work units: batch slices must hold a multiple of 4 (bf16: 8) images"),
    (dict(units=(2, 0, 2), bf16=True), "work units: batch slices must hold a multiple of 4 (bf16: 8) images"),
]


@pytest.mark.parametrize("kw,message", REFUSALS)
def test_partition_refusals(env, kw, message):
    with pytest.raises(env["err"], match=re.escape(message)):
        env["ens"].chwn_partition((8, 3, 8, 8), 3, 0, **kw)


# ---- the plan --------------------------------------------------------------------------------------------------------------
def _models(env):
    out = {}
    for name, kind in itertools.product(("alexnet", "3conv3fc", "lenet"), ("bbb", "lrt")):
        cin = 1 if name == "lenet" else 3
        out[f"zoo-{name}-{kind}"] = (lambda name=name, kind=kind, cin=cin: env["zoo"].getModel(name, cin, 10, PRIORS, kind, "softplus"),
                                     (8, cin, 32, 32), kind)
    for name, kind in itertools.product(ST.STRIDED, ("bbb", "lrt")):
        out[f"strided-{name}-{kind}"] = (lambda name=name, kind=kind: ST._net2(kind, ST.STRIDED[name]), (8, 3, 16, 16), kind)
    for name, kind in itertools.product(R.MODELS, ("bbb", "lrt")):
        cin, side, _ = R.MODELS[name]
        out[f"case-{name}-{kind}"] = (lambda name=name, kind=kind: R.build(name, kind), (8, cin, side, side), kind)
    return out


MODES = {"fp32": ("fp32", {}), "x3": ("bf16x3", {}), "x3-noc8": ("bf16x3", dict(c8x3=False)), "x3-s3": ("bf16x3", R.S3),
         "x3-nos2d": ("bf16x3", dict(c8x3_s2d=False)), "fp32-fuse": ("fp32", R.FUSE), "bf16": ("bf16", dict(bf16_lrt=True)),
         "bf16-noc8": ("bf16", dict(bf16_lrt=True, bf16_c8=False, pool_fusion=False))}


def _reference_shapes(ens, children, x_shape):
    """(C, H, W, B) behind every module, restated with torch.nn.functional on zero tensors (None from a flatten on that does not
    divide: the reference itself would refuse it)."""
    from layers.misc import FlattenLayer
    h, out = torch.zeros(x_shape), []
    for m in children:
        if isinstance(m, (ens._BBBConv, ens._LRTConv)):
            h = F.conv2d(h, torch.zeros(m.out_channels, m.in_channels, *m.kernel_size), None, m.stride, m.padding, m.dilation)
        elif isinstance(m, (ens._BBBLin, ens._LRTLin)):
            h = F.linear(h.reshape(h.shape[0], -1), torch.zeros(m.out_features, m.in_features))
        elif isinstance(m, nn.MaxPool2d):
            h = F.max_pool2d(h, m.kernel_size, m.stride)
        elif isinstance(m, FlattenLayer):
            h = h.reshape(-1, m.num_features)
        out.append(tuple(h.shape[1:]) + (1,) * (4 - h.dim()) + (h.shape[0],))
    return out


def _plans(env):
    ens, ops = env["ens"], env["ops"]
    for mname, (make, x_shape, kind) in _models(env).items():
        net = make()
        for mode, (precision, cfg) in MODES.items():
            for draws in (1, 2):
                with ops.use_config(**cfg):
                    yield f"{mname}-{mode}-e{draws}", net, x_shape, kind, precision, draws, ens.chwn_plan(net, x_shape, draws, precision)


def test_plan_walks_every_module_once_with_the_reference_shapes(env):
    ens, n_plans = env["ens"], 0
    for cid, net, x_shape, kind, precision, draws, steps in _plans(env):
        children = ens.flat_children(net)
        if steps is None:
            assert cid.startswith("case-none") or (precision == "bf16" and cid.startswith("case-quirk")), cid
            continue
        n_plans += 1
        want = _reference_shapes(ens, children, x_shape)
        at, shape = 0, tuple(x_shape[1:]) + (x_shape[0],)
        for st in steps:
            per_image = lambda s: (s[0] * s[1] * s[2], s[3])
            assert per_image(st.in_shape) == per_image(shape), (cid, st)           # (a linear layer reads its input as 1 x 1 maps)
            assert st.in_layout == (steps[steps.index(st) - 1].layout if st is not steps[0] else ("bf16" if precision == "bf16" else "f32"))
            if st.n_mods == 0:
                assert st.form in ("to_f32", "to_c8s3") and per_image(st.out_shape) == per_image(shape), (cid, st)
                continue
            assert st.i == at and st.mod is children[at], (cid, st)
            at += st.n_mods
            assert st.out_shape == want[at - 1], (cid, st, want[at - 1])
            shape = st.out_shape
            if st.form in ens.BAYES_FORMS:
                follows = [type(m) for m in children[st.i + 1:at]]
                assert follows == [nn.Softplus if st.act == "softplus" else nn.ReLU] * (st.act is not None) + [nn.MaxPool2d] * bool(st.pool)
            else:
                assert st.n_mods == 1 and st.form in ("pool", "relu", "softplus", "flatten"), (cid, st)
        assert at == len(children) and steps[-1].layout == "f32", cid
    assert n_plans > 200


def test_only_the_logits_step_writes_fp32_and_the_buffer(env):
    ens = env["ens"]
    for cid, net, x_shape, kind, precision, draws, steps in _plans(env):
        if steps is None:
            continue
        bayes = [st for st in steps if st.form in ens.BAYES_FORMS]
        for st in bayes[:-1]:
            assert not st.out_f32 and not st.logits, (cid, st)
        last = bayes[-1]
        tail = last.i + last.n_mods == len(ens.flat_children(net))
        assert last.logits == (tail and isinstance(last.mod, (ens._BBBLin, ens._LRTLin))), (cid, last)
        assert last.out_f32 == (tail and last.form not in ("fp32_bbb", "fp32_lrt")), (cid, last)
        assert [st.first for st in bayes] == [True] + [False] * (len(bayes) - 1)


def test_chain_forms_only_where_they_apply(env):
    ens, ops = env["ens"], env["ops"]
    seen = set()
    for cid, net, x_shape, kind, precision, draws, steps in _plans(env):
        for st in steps or ():
            seen.add(st.form)
            mode = cid.rsplit("-e", 1)[0].split(f"-{kind}-", 1)[1]
            if st.form in ("c8x3_bbb", "c8x3_lrt", "s2d_bbb", "s2d_lrt"):
                assert precision == "bf16x3" and MODES[mode][1].get("c8x3", True), (cid, st)
                assert st.form.endswith(kind)
            if st.form.startswith("c8x3"):
                m = st.mod
                cin, cout = (m.in_channels, m.out_channels) if hasattr(m, "in_channels") else (m.in_features, m.out_features)
                assert not st.first and ops.c8x3_layer_ok(cin, cout, is_logits=st.out_f32), (cid, st)
            if st.form.startswith("s2d"):
                m = st.mod
                assert st.i == 0 and MODES[mode][1].get("c8x3_s2d", True) and not (kind == "lrt" and draws > 1), (cid, st)
                assert ops.s2d_layer_ok(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, *x_shape[2:])
                assert st.pool is None or kind == "bbb"
            if precision == "bf16":
                assert st.form not in ("fp32_bbb", "fp32_lrt") and st.layout in ("bf16", "bf16c8", "f32"), (cid, st)
    assert seen >= set(ens.BAYES_FORMS) | {"pool", "relu", "softplus", "flatten", "to_f32", "to_c8s3"}


def test_partitions_keep_every_layers_form(env):
    """Which kernel a layer takes is a property of the layer and the step: work units, several steps per launch and a share of a
    group of steps give every layer the form of the whole step."""
    ens, ops = env["ens"], env["ops"]
    for mname, (make, x_shape, kind) in _models(env).items():
        net, (B, *chw) = make(), x_shape
        for mode, (precision, cfg) in MODES.items():
            if precision == "bf16" and kind == "lrt":
                continue                                                           # (no partitions there: the forward refuses them)
            with ops.use_config(**cfg):
                whole = ens.chwn_plan(net, x_shape, 2, precision)
                parts = [ens.chwn_plan(net, (2 * B, *chw), 2, precision, units=(2, 1, 3)),
                         ens.chwn_plan(net, (2 * B, *chw), 2, precision, groups=2),
                         ens.chwn_plan(net, (2 * B, *chw), 2, precision, share=(2, 1))]
            forms = lambda steps: None if steps is None else [(st.i, st.form) for st in steps if st.form in ens.BAYES_FORMS]
            for p in parts:
                assert forms(p) == forms(whole), (mname, mode)


def test_plan_of_a_model_the_forward_does_not_cover(env):
    ens = env["ens"]
    net = R.build("std", "bbb")
    net.add_module("extra", nn.Tanh())
    assert ens.chwn_plan(net, (8, 3, 8, 8), 2) is None
    assert ens.chwn_plan(R.build("std", "bbb"), (8, 3, 8), 2) is None
