"""Recorder for the batch-innermost inference forward (bbb_hip.ensemble._mc_logits_chwn), on the base of
tests/train_schedule_recorder.py: per case (i) every bbb_hip.ops launch the forward makes, in order, with its stream, its tensor
arguments' shapes / dtypes, its scalar arguments and every wait_stream edge, (ii) the (tag, info) list a `timers=` stand-in sees
(what bench.py's roofline consumes) and (iii) the sha256 of the logits' and of kl's bytes.  tests/test_gpu_infer_schedule.py compares
all three with tests/golden/infer_schedule.json.

    python tests/infer_schedule_recorder.py --write tests/golden/infer_schedule.json --commit <the commit that is recorded>

rewrites the golden (on a GPU).  It is a record of ONE commit's launches and bits: regenerate it only from a commit whose forward is
the intended one, never to make a failing comparison pass.  Every case runs twice; a digest that differs between the two runs is not
written (the case is listed in the file's _comment instead).

The cases use the smallest shapes that still reach each form of the walk: B = 8 (16 where a partition halves it), E = 2, 4 classes,
8 x 8 or 16 x 16 images, 16 channels behind the first layer (ops.c8x3_layer_ok holds); the size-gated forms are reached through
LaunchConfig thresholds (ops.use_config), not through size."""
import hashlib
import importlib.util
import json
import os
import sys

import torch
import torch.nn as nn

import train_schedule_recorder as T

CALLERS = ("bbb_hip.ensemble", "bbb_hip.infer_walk")       # (the second exists since the forward was cut into pieces)
# host-side queries of bbb_hip.ops (they launch nothing; how often the forward asks them is not part of its schedule)
HOST_ONLY = ("current_config", "use_config", "overlapped_launches", "LaunchConfig", "c8x3_layer_ok", "s2d_layer_ok", "s2d_geometry",
             "s2d_zero_border", "pool_fusion_ok", "bf16_pool_fusion_ok", "bf16_c8_input_ok", "bf16_tap_major", "is_pool_2x2",
             "bf16_row_pitch", "scratch_scope", "current_scratch_token", "graph_capture", "fp32_fwd_plan", "bf16_fwd_plan",
             "lrt_bf16_plan", "reparam_plan", "elbo_cb_ok")
SEED, CALL0, CLASSES = 11, 5, 4

# (kind, args): conv(cout, k, stride, pad) | relu | softplus | pool(k, s) | flatten(n) | fc(out)
_HEAD = [("flatten", 64), ("fc", 16), ("relu",), ("fc", CLASSES)]
MODELS = {
    # name: (input channels, image side, table)
    "std": (3, 8, [("conv", 16, 3, 1, 1), ("relu",), ("pool", 2, 2), ("conv", 16, 3, 1, 1), ("softplus",), ("pool", 2, 2)] + _HEAD),
    # AlexNet's first layer in small (space-to-depth form); the maps end 1 x 1 (a flatten that moves nothing, in every layout)
    "s2d": (3, 16, [("conv", 16, 11, 4, 5), ("relu",), ("pool", 2, 2), ("conv", 16, 3, 1, 1), ("relu",), ("pool", 2, 2),
                    ("flatten", 16), ("fc", 16), ("relu",), ("fc", CLASSES)]),
    # a pooled first layer in front of a 32-channel 5 x 5 stride-1 layer (ops.bf16_c8_input_ok)
    "c8in": (3, 8, [("conv", 32, 5, 1, 2), ("relu",), ("pool", 2, 2), ("conv", 16, 5, 1, 2), ("relu",), ("pool", 2, 2)] + _HEAD),
    # a flatten that cuts each image into four rows: B' = 4 B
    "quirk": (3, 8, [("conv", 16, 3, 1, 1), ("relu",), ("pool", 2, 2)] + _HEAD),
    # a flatten whose rows do not divide an image: the forward returns None and the caller falls back
    "none": (3, 8, [("conv", 12, 3, 1, 1), ("relu",), ("pool", 2, 2), ("flatten", 128), ("fc", CLASSES)]),
    # a pool right behind a layer, then an activation and a pool behind no layer
    "alone": (3, 8, [("conv", 16, 3, 1, 1), ("relu",), ("conv", 16, 3, 1, 1), ("pool", 2, 2), ("relu",), ("pool", 2, 2), ("softplus",)]
              + _HEAD),
}
FUSE = dict(pool_fuse_min_items=1, pool_fuse_imbalance=1e9)
S3 = dict(c8x3=False, s3_min_images=1, bf16x3_min_workgroups=1)
PARTS = {"units": dict(units=(2, 1, 3), B=16), "groups": dict(groups=2, B=16), "share": dict(share=(2, 1), B=16),
         "streams2": dict(streams=2)}


def _case(model="std", kind="bbb", precision="fp32", draws=2, B=8, cfg=None, **kw):
    return dict(model=model, kind=kind, precision=precision, draws=draws, B=B, cfg=dict(cfg or {}), kw=kw)


def cases():
    """{case id: dict(model, kind, precision, draws, B, cfg = LaunchConfig fields, kw = _mc_logits_chwn's partition arguments)}."""
    c = {"fp32-bbb": _case(), "fp32-bbb-poolfuse": _case(cfg=FUSE), "fp32-bbb-nosplitk": _case(cfg=dict(split_k=False)),
         "fp32-lrt-e2": _case(kind="lrt"), "fp32-lrt-e1": _case(kind="lrt", draws=1), "fp32-lrt-poolfuse": _case(kind="lrt", cfg=FUSE),
         "x3-bbb-c8x3": _case(precision="bf16x3"), "x3-bbb-s3": _case(precision="bf16x3", cfg=S3),
         "x3-bbb-plain": _case(precision="bf16x3", cfg=dict(c8x3=False)), "x3-lrt-c8x3": _case(kind="lrt", precision="bf16x3"),
         "s2d-bbb": _case("s2d", precision="bf16x3"), "s2d-lrt-e1": _case("s2d", "lrt", "bf16x3", draws=1),
         "s2d-lrt-e2": _case("s2d", "lrt", "bf16x3"),
         "bf16-bbb-plain": _case(precision="bf16", cfg=dict(pool_fusion=False)), "bf16-bbb-pooled": _case(precision="bf16"),
         "bf16-bbb-outc8": _case("c8in", precision="bf16"), "bf16-bbb-noc8": _case("c8in", precision="bf16", cfg=dict(bf16_c8=False)),
         "bf16-lrt-e2": _case(kind="lrt", precision="bf16", cfg=dict(bf16_lrt=True)),
         "bf16-lrt-e1": _case(kind="lrt", precision="bf16", draws=1, cfg=dict(bf16_lrt=True)),
         "quirk-streams1": _case("quirk"), "quirk-streams2": _case("quirk", streams=2)}
    for base, kw in (("fp32-bbb", {}), ("fp32-lrt", dict(kind="lrt")), ("x3-bbb-c8x3", dict(precision="bf16x3")),
                     ("bf16-bbb", dict(precision="bf16"))):
        for pname, part in PARTS.items():
            c[f"{base}-{pname}"] = _case(**kw, **part)
    for kind in ("bbb", "lrt"):
        c[f"fp32-{kind}-odd"] = _case(kind=kind, B=6)
    c["fp32-lrt-boffset"] = _case(kind="lrt", b_offset=8)
    for name, kw in (("fp32", {}), ("x3-c8x3", dict(precision="bf16x3")), ("x3-s3", dict(precision="bf16x3", cfg=S3)),
                     ("bf16", dict(precision="bf16"))):
        c[f"alone-{name}"] = _case("alone", **kw)
    return c


FALLBACK = _case("none")              # checked by value and stats["path"] only (golden["fallback"])


def build(model, kind):
    """The case model on the CPU (chwn_plan works there; record() moves it to the GPU)."""
    import ref_port_torch as P
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    Conv, Linear = (BBB_LRT_Conv2d, BBB_LRT_Linear) if kind == "lrt" else (BBB_Conv2d, BBB_Linear)
    cin, _, table = MODELS[model]
    torch.manual_seed(5)
    net, feat = ModuleWrapper(), None
    for i, (what, *a) in enumerate(table):
        if what == "conv":
            mod = Conv(cin, a[0], a[1], stride=a[2], padding=a[3], bias=True, priors=P.CONFIG_PRIORS)
            cin = a[0]
        elif what == "fc":
            mod = Linear(feat, a[0], bias=True, priors=P.CONFIG_PRIORS)
            feat = a[0]
        elif what == "flatten":
            mod, feat = FlattenLayer(a[0]), a[0]
        else:
            mod = nn.ReLU() if what == "relu" else nn.Softplus() if what == "softplus" else nn.MaxPool2d(a[0], a[1])
        net.add_module(f"{what}{i}", mod)
    return net


def x_shape(case):
    cin, side, _ = MODELS[case["model"]]
    return (case["B"], cin, side, side)


class Brackets:
    """Stand-in for ensemble.Timers: records (tag, info) as bench.py's roofline would read them; no events."""

    def __init__(self):
        self.records = []

    def bracket(self, tag, info, fn):
        out = fn()
        self.records.append([tag, info(out) if callable(info) else info])
        return out


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _inputs(case):
    from bbb_hip import rng
    net = build(case["model"], case["kind"]).cuda()
    rng.assign_stream_ids(net)
    x = torch.rand(x_shape(case), generator=torch.Generator().manual_seed(6)).cuda()
    return net, x


def _sides(device):
    from bbb_hip import ensemble
    return [s for (dev, _), pool in sorted(ensemble._stream_pool.items()) if dev == device.index for s in pool]


def record(case, monkeypatch):
    """-> dict(trace, brackets, logits, kl): one recorded forward, then one under the bracket stand-in."""
    from bbb_hip import ensemble, ops
    net, x = _inputs(case)
    args = (net, x, case["draws"], SEED, CALL0)
    with torch.no_grad(), ops.use_config(**case["cfg"]):
        torch.cuda.synchronize()
        callers = [m for m in CALLERS if importlib.util.find_spec(m) is not None]
        with T.Recorder(monkeypatch, x.device, callers=callers, sides=_sides, scalars=True, skip=HOST_ONLY) as rec:
            logits, kl = ensemble._mc_logits_chwn(*args, precision=case["precision"], **case["kw"])
        torch.cuda.synchronize()
        br = Brackets()
        ensemble._mc_logits_chwn(*args, timers=br, precision=case["precision"], **case["kw"])
        torch.cuda.synchronize()
    return dict(trace=rec.events, brackets=json.loads(json.dumps(br.records)), logits=_sha(logits), kl=_sha(kl))


def fallback():
    """The forward that does not fit (-> None before or after some launches): what mc_logits returns, and on which path."""
    from bbb_hip import ensemble
    net, x = _inputs(FALLBACK)
    with torch.no_grad():
        assert ensemble._mc_logits_chwn(net, x, 2, SEED, CALL0) is None
        logits, kl = ensemble.mc_logits(net, x, 2, SEED, CALL0)
    torch.cuda.synchronize()
    return dict(path=ensemble.stats["path"], logits=_sha(logits), kl=_sha(kl))


def main(argv):
    import argparse
    import pytest
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "pytorch-bayesiancnn_amd"), os.path.join(root, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True, help="where the golden goes (tests/golden/infer_schedule.json)")
    ap.add_argument("--commit", required=True, help="the commit whose forward is recorded")
    args = ap.parse_args(argv)
    out, unstable = {}, []
    for cid, case in cases().items():
        runs = []
        for _ in range(2):
            with pytest.MonkeyPatch.context() as mp:
                runs.append(record(case, mp))
        if runs[0] != runs[1]:
            unstable.append(cid)
            print(f"{cid}: two runs differ in {[k for k in runs[0] if runs[0][k] != runs[1][k]]}")
            runs[0]["logits"] = runs[0]["kl"] = None
        out[cid] = runs[0]
        print(cid, len(runs[0]["trace"]), "events", flush=True)
    fb = [fallback(), fallback()]
    assert fb[0] == fb[1], fb
    doc = {"_comment": ["The batch-innermost inference forward (bbb_hip.ensemble._mc_logits_chwn), recorded by tests/infer_schedule_recorder.py.",
                        f"Produced on an MI355X from commit {args.commit} by:",
                        f"  python tests/infer_schedule_recorder.py --write tests/golden/infer_schedule.json --commit {args.commit}",
                        "trace: '<stream> <op> <arguments>' or 'wait <waiting stream> <- <awaited stream>'; brackets: [tag, info] as a "
                        "timers= object sees them; logits / kl: sha256 of the bytes.",
                        "Cases whose digests differed between the two recording runs (digests null): " + (", ".join(unstable) or "none")],
           "cases": out, "fallback": fb[0]}
    with open(args.write, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(out)} cases, {sum(len(c['trace']) for c in out.values())} events -> {args.write}; unstable: {unstable}")


if __name__ == "__main__":
    main(sys.argv[1:])
