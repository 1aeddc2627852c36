"""CPU-only checks of fast_train.train_plan and fast_train._walk, the layer plan and the forward walk over it that the training nodes
share: over the module lists the other CPU tests build (test_strided_train_cpu.py, the zoo models of test_host_cpu.py) and the seeded
families of the training fuzz suites, with stub callbacks that return CPU tensors of the right shape.  Whenever
fast_train._train_path_static admits a model the plan's blocks carry the maps and weight shape torch's own shape arithmetic gives,
and the walk yields one record per Bayesian layer with the activation, pool, `first`, geometry and out_shape the nodes' backward
relies on (restated here from the module list and torch's shapes); a linear layer receives [*, in_features, 1, 1, B]; a FlattenLayer
reshapes to num_features; a pool that follows no layer is refused by the parser; a geometry changed in place on an analysed model
raises in the walk until ensemble.invalidate."""
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ref_port_torch as P
import test_gpu_bf16_train_fuzz as BF
import test_gpu_train_fuzz as TF
from test_strided_train_cpu import STRIDED, _net2

E = 2


def _models():
    import layers  # noqa: F401
    from bbb_hip import zoo
    out = {}
    for kind in ("bbb", "lrt"):
        for name, convs in STRIDED.items():
            out[f"strided-{name}-{kind}"] = (lambda kind=kind, convs=convs: _net2(kind, convs), (8, 3, 16, 16))
        for net_type, cin in (("alexnet", 3), ("3conv3fc", 3), ("lenet", 1)):
            out[f"zoo-{net_type}-{kind}"] = (lambda t=net_type, c=cin, kind=kind: zoo.getModel(t, c, 10, P.CONFIG_PRIORS, kind, "softplus"),
                                             (8, cin, 32, 32))
    for name, spec in TF.MODELS.items():
        out[f"fuzz-{name}"] = (lambda spec=spec: TF._build(spec), (spec["B"], spec["Cin"], spec["H"], spec["W"]))
    for name, spec in BF.MODELS.items():
        out[f"bf16fuzz-{name}"] = (lambda spec=spec: BF._build(spec, 1), (spec["B"], spec["Cin"], spec["H"], spec["W"]))
    return out


MODELS = _models()


def _chwn(t):                              # [B, C, H, W] -> [1, C, H, W, B]
    return t.permute(1, 2, 3, 0).unsqueeze(0)


def _nchw(t5):                             # [E', C, H, W, B] -> [E' * B, C, H, W]
    return t5.permute(0, 4, 1, 2, 3).reshape(-1, *t5.shape[1:4])


def _stubs(B, seen):
    def run_layer(blk, x_in):                  # (convolves with the LIVE module's geometry, as a node's launch of a mutated model would)
        m, li, is_conv = blk.layer, blk.li, blk.is_conv
        seen.append(dict(li=li, x_shape=tuple(x_in.shape), is_conv=is_conv, act=blk.act, pooled=blk.pool is not None))
        assert is_conv == hasattr(m, "kernel_size")
        cout, cin = (m.out_channels, m.in_channels) if is_conv else (m.out_features, m.in_features)
        k = tuple(m.kernel_size) if is_conv else (1, 1)
        geom = (m.stride, m.padding, m.dilation) if is_conv else (1, 0, 1)
        y = F.conv2d(_nchw(x_in[:1]), torch.zeros(cout, cin, *k), None, *geom)                    # [B, Cout, Ho, Wo]
        return dict(y=y.permute(1, 2, 3, 0).unsqueeze(0).expand(E, -1, -1, -1, -1), mine=li)

    def pool(y, k, s):
        p = F.max_pool2d(_nchw(y), k, s)
        return p.reshape(y.shape[0], B, *p.shape[1:]).permute(0, 2, 3, 4, 1)

    return run_layer, pool


def _expected(mods, x_shape):
    """Per Bayesian layer (act, pool, geom, out_shape; in_chw, conv_chw, out_chw, wshape), from the module list and torch's shapes
    alone."""
    from layers.misc import FlattenLayer
    B = x_shape[0]
    h = torch.zeros(x_shape)
    out = []
    i = 0
    while i < len(mods):
        m = mods[i]
        if hasattr(m, "W_mu"):
            conv = hasattr(m, "kernel_size")
            geom = (m.stride, m.padding, m.dilation) if conv else (1, 0, 1)
            w = torch.zeros(m.W_mu.shape) if conv else torch.zeros(m.out_features, m.in_features, 1, 1)
            x4 = h if conv else h.reshape(B, m.in_features, 1, 1)
            h = F.conv2d(x4, w, None, *geom)
            ent = dict(layer=m, act=None, pool=None, geom=geom, first=not out, in_chw=tuple(x4.shape[1:]), conv_chw=tuple(h.shape[1:]),
                       wshape=tuple(w.shape))
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            if isinstance(nxt, (nn.ReLU, nn.Softplus)):
                ent["act"] = "relu" if isinstance(nxt, nn.ReLU) else "softplus"
                i += 1
                nxt = mods[i + 1] if i + 1 < len(mods) else None
            if isinstance(nxt, nn.MaxPool2d):
                ent["pool"] = (nxt.kernel_size, nxt.stride)
                h = F.max_pool2d(h, nxt.kernel_size, nxt.stride)
                i += 1
            ent["out_chw"] = tuple(h.shape[1:])
            ent["out_shape"] = (E,) + ent["out_chw"] + (B,)
            out.append(ent)
        elif isinstance(m, FlattenLayer):
            h = h.reshape(B, -1)
            assert h.shape[1] == m.num_features
        i += 1
    return out


def _walk(net, x_shape, seen):
    from bbb_hip import ensemble, fast_train
    mods = ensemble.flat_children(net)
    run_layer, pool = _stubs(x_shape[0], seen)
    tape, h = fast_train._walk(fast_train.train_plan(net, x_shape), _chwn(torch.zeros(x_shape)), run_layer, pool)
    return mods, tape, h


def test_the_model_lists_reach_every_form():
    from bbb_hip import fast_train
    admitted = [n for n, (make, xs) in MODELS.items() if fast_train._train_path_static(make(), torch.zeros(xs)) is not None]
    assert len(admitted) >= 30, admitted


@pytest.mark.parametrize("name", list(MODELS))
def test_walk_records_what_the_backward_reads(name):
    from bbb_hip import fast_train
    make, x_shape = MODELS[name]
    net = make()
    if fast_train._train_path_static(net, torch.zeros(x_shape)) is None:
        return                             # (not on the path: nothing is promised about it)
    seen = []
    mods, tape, h = _walk(net, x_shape, seen)
    want = _expected(mods, x_shape)
    assert len(tape) == len(want) == len([m for m in mods if hasattr(m, "W_mu")])
    B = x_shape[0]
    plan = fast_train.train_plan(net, x_shape)
    assert plan.kind == fast_train._train_path_static(net, torch.zeros(x_shape)) and len(plan.blocks) == len(want)
    for li, (blk, w) in enumerate(zip(plan.blocks, want)):                          # the plan against torch's own shapes
        assert blk.layer is w["layer"] and blk.li == li and (blk.first, blk.last) == (li == 0, li == len(want) - 1)
        assert (blk.in_chw, blk.conv_chw, blk.out_chw, blk.wshape) == (w["in_chw"], w["conv_chw"], w["out_chw"], w["wshape"])
    for li, (rec, w, s) in enumerate(zip(tape, want, seen)):
        assert rec["layer"] is w["layer"] and rec["mine"] == li == s["li"]          # the node's own keys stay in the record
        assert (rec["act"], rec["pool"], rec["geom"], rec["first"]) == (w["act"], w["pool"], w["geom"], w["first"])
        assert rec["first"] == (li == 0)
        assert rec["out_shape"] == w["out_shape"]
        assert (s["act"], s["pooled"]) == (w["act"], w["pool"] is not None)
        assert tuple(rec["x"].shape) == s["x_shape"]
        m = rec["layer"]
        if not s["is_conv"]:               # a linear layer reads [*, in_features, 1, 1, B]
            assert s["x_shape"][1:] == (m.in_features, 1, 1, B)
        else:
            assert s["x_shape"][1] == m.in_channels and s["x_shape"][-1] == B
        if li > 0:                         # what a layer reads is what the one before left (a flatten only reshapes it)
            prev = tape[li - 1]["out_shape"]
            assert s["x_shape"][0] == prev[0] and s["x_shape"][-1] == B
            assert s["x_shape"][1] * s["x_shape"][2] * s["x_shape"][3] == prev[1] * prev[2] * prev[3]
    assert tuple(h.shape) == tape[-1]["out_shape"]


def test_flatten_reshapes_to_num_features():
    from layers import BBB_Linear, FlattenLayer, ModuleWrapper
    net = ModuleWrapper()
    net.add_module("flatten", FlattenLayer(3 * 4 * 4))
    net.add_module("fc", BBB_Linear(48, 10, bias=True, priors=P.CONFIG_PRIORS))
    seen = []
    _, tape, h = _walk(net, (8, 3, 4, 4), seen)
    assert seen[0]["x_shape"] == (1, 48, 1, 1, 8) and tape[0]["out_shape"] == (E, 10, 1, 1, 8)


@pytest.mark.parametrize("where", ["leading", "after_pool", "after_flatten"])
def test_a_pool_that_follows_no_layer_raises(where):
    from bbb_hip import _lib, ensemble, fast_train
    from layers import BBB_Conv2d, BBB_Linear, FlattenLayer, ModuleWrapper
    net = ModuleWrapper()
    if where == "leading":
        net.add_module("p0", nn.MaxPool2d(2, 2))
    net.add_module("c1", BBB_Conv2d(3, 8, 3, padding=1, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("a1", nn.ReLU())
    net.add_module("p1", nn.MaxPool2d(2, 2))
    if where == "after_pool":
        net.add_module("p2", nn.MaxPool2d(2, 2))
    net.add_module("fl", FlattenLayer(8 * 8 * 8))
    if where == "after_flatten":
        net.add_module("p3", nn.MaxPool2d(1, 1))
    net.add_module("f1", BBB_Linear(512, 10, bias=True, priors=P.CONFIG_PRIORS))
    assert fast_train.train_plan(net, (8, 3, 16, 16)) is None
    plan, why = fast_train._parse(ensemble.flat_children(net), (8, 3, 16, 16))
    assert plan is None and re.search("pooling must follow a Bayesian layer", why)
    with pytest.raises(_lib.BBBHipError, match="fast_train: pooling must follow a Bayesian layer"):    # what a node's forward raises
        fast_train._node_plan(dict(net=net), torch.zeros(8, 3, 16, 16))


def test_a_geometry_changed_in_place_raises_until_invalidate():
    """The plan is an analysis cached on the model (ensemble._structure).  A stride changed in place afterwards: the walk holds what
    the layer's launch returns (the stubs convolve with the live module's geometry) against the plan and raises, naming
    ensemble.invalidate; after it the plan carries the new geometry and the walk passes."""
    from bbb_hip import _lib, ensemble, fast_train
    from layers import BBB_Conv2d, BBB_Linear, FlattenLayer, ModuleWrapper
    net = ModuleWrapper()
    net.add_module("conv1", BBB_Conv2d(3, 8, 3, padding=1, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("act1", nn.ReLU())
    net.add_module("conv2", BBB_Conv2d(8, 8, 3, padding=1, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("act2", nn.ReLU())
    net.add_module("gap", nn.AdaptiveAvgPool2d(1))                   # (one feature per channel at either stride)
    net.add_module("flatten", FlattenLayer(8))
    net.add_module("fc", BBB_Linear(8, 10, bias=True, priors=P.CONFIG_PRIORS))
    x_shape = (8, 3, 8, 8)
    run_layer, pool = _stubs(x_shape[0], [])

    def avgpool(y, k, s, p, count_include_pad):
        q = F.avg_pool2d(_nchw(y), k, s, p, count_include_pad=count_include_pad)
        return q.reshape(y.shape[0], x_shape[0], *q.shape[1:]).permute(0, 2, 3, 4, 1)

    def walk():
        return fast_train._walk(fast_train.train_plan(net, x_shape), _chwn(torch.zeros(x_shape)), run_layer, pool, avgpool)

    before = fast_train.train_plan(net, x_shape)
    assert before.blocks[1].geom[0] == 1 and (before.blocks[1].conv_chw, before.blocks[1].out_chw) == ((8, 8, 8), (8, 1, 1))
    assert tuple(walk()[1].shape) == (E, 10, 1, 1, 8)
    net.conv2.stride = 2                                              # in place: no hook sees it, the cached plan stays
    assert fast_train.train_plan(net, x_shape) is before
    with pytest.raises(_lib.BBBHipError, match=r"geometry changed since it was analysed.*ensemble\.invalidate\(net\)"):
        walk()
    ensemble.invalidate(net)
    after = fast_train.train_plan(net, x_shape)
    assert after.blocks[1].geom[0] == 2 and (after.blocks[1].conv_chw, after.blocks[1].out_chw) == ((8, 4, 4), (8, 1, 1))
    assert tuple(after.blocks[1].pool[0]) == (4, 4) and tuple(before.blocks[1].pool[0]) == (8, 8)
    assert tuple(walk()[1].shape) == (E, 10, 1, 1, 8)
