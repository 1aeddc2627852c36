"""Recorder for the launch schedule of the training nodes (bbb_hip.fast_train): which bbb_hip.ops function fast_train calls, in
which order, on which stream (`main`, `side0`, `side1`, ...), with tensors of which shape and dtype, and every wait_stream edge
(who waits on whom).  The placement is value-neutral -- no gradient moves when a launch lands on another stream -- so the value
suites cannot see it; tests/test_gpu_train_schedule.py compares these traces with tests/golden/train_schedule.json.
Every case, the frozen bf16 LRT ones included, is driven through train.forward_loss + loss.backward() (the entry
tests/test_gpu_bf16_lrt_input_grad.py calls "forward_loss"), under the case's LaunchConfig fields.

    python tests/train_schedule_recorder.py --write tests/golden/train_schedule.json --commit <the commit that is recorded>

rewrites the expected traces (on a GPU).  They are a record of ONE commit's schedule: regenerate them only from a commit whose
schedule is the intended one, never to make a failing comparison pass."""
import json
import os
import re
import sys

import torch
import torch.nn as nn

DTYPES = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float64: "f64", torch.int32: "i32", torch.int64: "i64",
          torch.uint8: "u8", torch.bool: "b8", torch.float16: "f16"}
CALLER = "bbb_hip.fast_train"


def _describe(a):
    """Tensors -> 'f32[2,8,4,4,8]'; lists / tuples that hold tensors -> the list of their descriptions; anything else -> None."""
    if torch.is_tensor(a):
        return f"{DTYPES.get(a.dtype, str(a.dtype))}[{','.join(str(int(s)) for s in a.shape)}]"
    if isinstance(a, (list, tuple)):
        inner = [_describe(t) for t in a]
        return inner if any(d is not None for d in inner) else None
    return None


def _flat(d):
    return "(" + " ".join(_flat(t) if t is not None else "-" for t in d) + ")" if isinstance(d, list) else d


def _is_scalar(a):
    return a is None or isinstance(a, (bool, int, float, str)) or (isinstance(a, tuple) and all(_is_scalar(t) for t in a))


def _describe_all(a):
    """_describe, and scalar arguments (None, bools, numbers, strings, tuples of those) as their repr; other objects -> None."""
    if _is_scalar(a):
        return repr(a)
    if isinstance(a, (list, tuple)):
        return [_describe_all(t) for t in a]
    return _describe(a)


def _train_sides(device):
    from bbb_hip import fast_train
    sides = fast_train._side_streams.get((device.index, fast_train.n_side_streams[0]))
    return [] if sides is None else sides.streams


class Recorder:
    """with Recorder(monkeypatch, device) as rec: ...; rec.events is the trace, one string per event:
    '<stream> <op> <tensor arguments>' and 'wait <waiting stream> <- <awaited stream>'.
    callers: the modules whose calls are recorded; sides(device) -> their side streams, in order; scalars: the scalar arguments
    (None, bools, numbers, strings, tuples of those) are recorded too; skip: names of bbb_hip.ops that are left alone."""

    def __init__(self, monkeypatch, device, callers=(CALLER,), sides=_train_sides, scalars=False, skip=()):
        from bbb_hip import ops
        self.mp, self.device = monkeypatch, torch.device(device)
        self.callers, self.sides, self.ops = tuple(callers), sides, ops
        self.describe = _describe_all if scalars else _describe
        self.skip = frozenset(skip)
        self.events = []
        self.depth = 0
        self.main = None

    def called_ops(self):
        """Every public callable of bbb_hip.ops that the callers' source names (called there, or handed on as a callback)."""
        import importlib
        import inspect
        src = "".join(inspect.getsource(importlib.import_module(c)) for c in self.callers)
        names = sorted(set(re.findall(r"\bops\.([A-Za-z]\w*)", src)) - self.skip)
        return [n for n in names if callable(getattr(self.ops, n, None))]

    def tag(self, stream):
        if stream == self.main:
            return "main"
        for i, s in enumerate(self.sides(self.device)):
            if stream == s:
                return f"side{i}"
        return "other"

    def _wrap(self, name, fn):
        def wrapper(*args, **kwargs):
            # only what the callers themselves call: not what one ops function asks of another (depth), nor other modules' calls
            mine = self.depth == 0 and sys._getframe(1).f_globals.get("__name__") in self.callers
            if mine:
                descr = [self.describe(a) for a in args] + [(k, self.describe(v)) for k, v in sorted(kwargs.items())]
                parts = [_flat(d) for d in descr if not isinstance(d, tuple) and d is not None]
                parts += [f"{k}={_flat(d)}" for k, d in (d for d in descr if isinstance(d, tuple)) if d is not None]
                self.events.append(" ".join([self.tag(torch.cuda.current_stream(self.device)), name] + parts))
            self.depth += 1
            try:
                return fn(*args, **kwargs)
            finally:
                self.depth -= 1
        wrapper.__name__ = name
        return wrapper

    def __enter__(self):
        self.main = torch.cuda.current_stream(self.device)
        for name in self.called_ops():
            self.mp.setattr(self.ops, name, self._wrap(name, getattr(self.ops, name)))
        orig_wait = torch.cuda.Stream.wait_stream
        rec = self

        def wait_stream(self, other):
            if sys._getframe(1).f_globals.get("__name__") in rec.callers:
                rec.events.append(f"wait {rec.tag(self)} <- {rec.tag(other)}")
            return orig_wait(self, other)
        self.mp.setattr(torch.cuda.Stream, "wait_stream", wait_stream)
        return self

    def __exit__(self, *exc):
        self.mp.undo()
        return False


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: B = 8 (bf16 needs B % 8 == 0), 8 x 8 images, four Bayesian layers (a two-stream round robin wraps)
# ---------------------------------------------------------------------------------------------------------------------------
B, HW, CLASSES = 8, 8, 4
MODELS = {"cin3": dict(cin=3, stride2=1),          # first layer: the shared-input im2col path (forked early under side streams)
          "cin4": dict(cin=4, stride2=1),          # no im2col fork; the first layer on conv2d_chwn_weight_grad
          "cin3_s2": dict(cin=3, stride2=2)}       # the transposed dgrad launch (the bf16 nodes: under bf16_strided_train)
DEFAULT = dict(overlap_wgrad=True, flips_up_front=True, pair_lrt_backward=True, fold_lrt_combine=True)
# node -> (the layers it is built from, the precision it runs at, the ensemble.stats["path"] it must take)
NODES = {"fp32": ("bbb", "fp32", "chwn-autograd"), "bf16": ("bbb", "bf16", "chwn-autograd-bf16"),
         "lrt": ("lrt", "fp32", "chwn-autograd"), "lrt_bf16": ("lrt", "bf16", "chwn-autograd-bf16-lrt")}


def _variants(model, node):
    """{variant: settings}.  Settings: the fast_train switches of DEFAULT; frozen (frozen parameters, x.requires_grad: no weight
    side, no side streams); config (LaunchConfig fields, applied with ops.use_config around the forward and the backward);
    side_streams (fast_train.n_side_streams, 2 unless set)."""
    strided = dict(bf16_strided_train=True) if MODELS[model]["stride2"] != 1 else {}
    if node == "lrt_bf16":                         # input gradients with frozen parameters are all this node has
        return {"frozen_dx": dict(frozen=True, config=dict(bf16_lrt=True, bf16_lrt_input_grad=True, **strided))}
    if node == "bf16" and strided:
        return {"default": dict(config=strided), "frozen_dx": dict(frozen=True, config=dict(bf16_input_grad=True, **strided))}
    out = {"default": {}, "overlap_off": dict(overlap_wgrad=False), "flips_off": dict(flips_up_front=False),
           "overlap_off_flips_off": dict(overlap_wgrad=False, flips_up_front=False)}
    if node == "lrt":
        out["pair_off"] = dict(pair_lrt_backward=False)
        out["fold_off"] = dict(fold_lrt_combine=False)
    out["frozen_dx"] = dict(frozen=True, config=dict(bf16_input_grad=True)) if node == "bf16" else dict(frozen=True)
    return out


def cases():
    """{case id: (model, node, draws, variant settings)}."""
    out = {}
    for model in MODELS:
        for node, draws in (("fp32", 2), ("bf16", 2), ("lrt", 2), ("lrt", 1), ("lrt_bf16", 2), ("lrt_bf16", 1)):
            for vname, v in _variants(model, node).items():
                out[f"{model}-{node}-e{draws}-{vname}"] = (model, node, draws, v)
    return out


def build(model, node):
    import ref_port_torch as P
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    Conv, Linear = (BBB_LRT_Conv2d, BBB_LRT_Linear) if NODES[node][0] == "lrt" else (BBB_Conv2d, BBB_Linear)
    spec = MODELS[model]
    torch.manual_seed(5)
    net = ModuleWrapper()
    net.add_module("conv0", Conv(spec["cin"], 8, 3, padding=1, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("act0", nn.ReLU())
    net.add_module("pool0", nn.MaxPool2d(2, 2))
    net.add_module("conv1", Conv(8, 8, 3, stride=spec["stride2"], padding=1, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("act1", nn.Softplus())
    side = (HW // 2 + 2 - 3) // spec["stride2"] + 1
    feat = 8 * side * side
    net.add_module("flatten", FlattenLayer(feat))
    net.add_module("fc0", Linear(feat, 16, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("fact0", nn.ReLU())
    net.add_module("fc1", Linear(16, CLASSES, bias=True, priors=P.CONFIG_PRIORS))
    return net


def record(case, monkeypatch, grads=None):
    """One forward + backward of the case under the recorder -> the trace.  Every switch is restored.
    grads: a dict that receives the gradients the backward left, "x" and every parameter's by name (None where there is none)."""
    from bbb_hip import ensemble, fast_train, ops, rng, train
    model, node, draws, variant = case
    _, precision, path = NODES[node]
    net = build(model, node).cuda()
    rng.assign_stream_ids(net)
    frozen = variant.get("frozen", False)
    net.requires_grad_(not frozen)
    gen = torch.Generator().manual_seed(6)
    x = torch.rand((B, MODELS[model]["cin"], HW, HW), generator=gen).cuda().requires_grad_(frozen)
    y = torch.randint(0, CLASSES, (B,), generator=gen).cuda()
    device = x.device
    switches = {k: {**DEFAULT, **variant}[k] for k in DEFAULT}
    saved = {k: getattr(fast_train, k)[0] for k in switches}
    saved_n = fast_train.n_side_streams[0]
    try:
        for k, v in switches.items():
            getattr(fast_train, k)[0] = v
        fast_train.n_side_streams[0] = variant.get("side_streams", 2)
        if fast_train.n_side_streams[0] >= 1:
            fast_train._side_stream(device).i = 0             # the round robin starts where a fresh process starts it
        torch.cuda.synchronize()
        with Recorder(monkeypatch, device) as rec, ops.use_config(**variant.get("config", {})):
            loss, _, _ = train.forward_loss(net, x, y, draws, 0.0 if frozen else 0.1, 100.0, seed_call=(7, 3), precision=precision)
            assert ensemble.stats["path"] == path, ensemble.stats["path"]
            loss.backward()
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            getattr(fast_train, k)[0] = v
        fast_train.n_side_streams[0] = saved_n
    if frozen:
        assert x.grad is not None and all(p.grad is None for p in net.parameters())
    else:
        assert all(p.grad is not None for p in net.parameters())
    if grads is not None:
        grads.update({"x": x.grad}, **{n: p.grad for n, p in net.named_parameters()})
    return rec.events


def main(argv):
    import argparse
    import pytest
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "pytorch-bayesiancnn_amd"), os.path.join(root, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True, help="where the expected traces go (tests/golden/train_schedule.json)")
    ap.add_argument("--commit", required=True, help="the commit whose schedule is recorded")
    args = ap.parse_args(argv)
    traces = {}
    for cid, case in cases().items():
        with pytest.MonkeyPatch.context() as mp:
            traces[cid] = record(case, mp)
    doc = {"_comment": ["Launch schedule of the training nodes (bbb_hip.fast_train), recorded by tests/train_schedule_recorder.py.",
                        f"Produced on an MI355X from commit {args.commit} by:",
                        f"  python tests/train_schedule_recorder.py --write tests/golden/train_schedule.json --commit {args.commit}",
                        "One string per event: '<stream> <op> <tensor arguments>' or 'wait <waiting stream> <- <awaited stream>'."],
           "traces": traces}
    with open(args.write, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(traces)} traces, {sum(len(t) for t in traces.values())} events -> {args.write}")


if __name__ == "__main__":
    main(sys.argv[1:])
