"""Strided convolutions behind the first layer on the training path, one MI355X (numbers: strided_dgrad_notes.md).

The model is defined here, not in zoo: Bayesian3Conv3FC with its three MaxPool2d(3, 2) removed and each 5 x 5 convolution given
stride 2 (32 x 32 -> 16 -> 8 -> 3; conv2 and conv3 are strided later layers).  BBB and LRT, bs 256 x 1 draw and bs 512 x 10 draws.

    python profiles/strided_dgrad_timing.py steps [--blocks 3] [--steps 10]
        ms per step from device events, median and spread over blocks, of (eager) train.train_step(graph=False), (captured)
        train.GraphedTrainStep, (xgrad) ensemble.mc_forward + backward to x with frozen weights and (xgrad_loop) the same gradient
        through a `net(x)` loop of num_ens calls -- what serves it where mc_forward has no graph to x; the path each took is printed.
        The script runs against the package next to it, so a copy placed in a checkout of the parent commit measures the parent
        (there the model takes the reference-layout path) -- run both on one box in one session and compare.
    python profiles/strided_dgrad_timing.py layers [--reps 20]
        per strided layer: `reps` forward launches, then `reps` input-gradient launches (device-event times printed); under
        `rocprofv3 --kernel-trace --stats -- python ...` the trace holds them in that order (pconv_gemm_kernel / pconv_dgrad_kernel).
    python profiles/strided_dgrad_timing.py parse <kernel_trace.csv> [--reps 20]
        per-layer mean kernel times and TFLOP/s of in-bounds work from such a trace.
"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))

PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}
CONVS = [(3, 32, 5, 2, 2, 32), (32, 64, 5, 2, 2, 16), (64, 128, 5, 2, 1, 8)]          # cin, cout, k, stride, padding, input map
WORKLOADS = [("bbb", 256, 1), ("bbb", 512, 10), ("lrt", 256, 1), ("lrt", 512, 10)]
VARIANTS = ("eager", "captured", "xgrad", "xgrad_loop")


def build(kind):
    import torch
    import torch.nn as nn
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    from bbb_hip import rng
    Conv, Linear = (BBB_Conv2d, BBB_Linear) if kind == "bbb" else (BBB_LRT_Conv2d, BBB_LRT_Linear)
    torch.manual_seed(0)
    net = ModuleWrapper()
    for i, (cin, cout, k, s, p, _) in enumerate(CONVS):
        net.add_module(f"conv{i + 1}", Conv(cin, cout, k, stride=s, padding=p, bias=True, priors=PRIORS))
        net.add_module(f"act{i + 1}", nn.Softplus())
    net.add_module("flatten", FlattenLayer(3 * 3 * 128))
    for j, (fi, fo) in enumerate([(3 * 3 * 128, 1000), (1000, 1000), (1000, 10)]):
        net.add_module(f"fc{j + 1}", Linear(fi, fo, bias=True, priors=PRIORS))
        if j < 2:
            net.add_module(f"act{j + 4}", nn.Softplus())
    net = net.cuda()
    rng.assign_stream_ids(net)
    return net


def step_fn(variant, kind, B, E):
    import torch
    import torch.nn.functional as F
    from bbb_hip import ensemble, train
    net = build(kind)
    x = torch.rand(B, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (B,), device="cuda")
    if variant == "eager":
        opt = train.FusedAdam(net.parameters(), lr=1e-9)
        return lambda: train.train_step(net, opt, x, y, E, 0.1, 50000.0, graph=False)[0]
    if variant == "captured":
        opt = train.FusedAdam(net.parameters(), lr=1e-9, capturable=True)
        g = train.GraphedTrainStep(net, opt, x, y, E, 0.1, 50000.0, warmup=3)
        return lambda: g.step()[0]
    net.requires_grad_(False)
    xg = x.clone().requires_grad_(True)

    def step():
        xg.grad = None
        if variant == "xgrad":
            lo, _ = ensemble.mc_forward(net, xg, E)
        else:
            outs = torch.stack([F.log_softmax(net(xg)[0], dim=1) for _ in range(E)], dim=2)
            m = outs.max(dim=2, keepdim=True)[0]
            lo = (m + torch.log(torch.mean(torch.exp(outs - m), dim=2, keepdim=True))).squeeze(2)
        loss = F.nll_loss(lo, y)
        loss.backward()
        return loss.detach()
    return step


def measure(variant, kind, B, E, steps, blocks, warm=3):
    import torch
    from bbb_hip import ensemble
    step = step_fn(variant, kind, B, E)
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    path = ensemble.stats.get("path")
    ms = []
    for _ in range(blocks):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            loss = step()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / steps)
    ms.sort()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], loss=float(loss), path=path)


def in_bounds_flop(cin, cout, k, s, p, H, B, E):
    """2 x (pixel, tap) pairs inside the image x channels x images x draws: the forward launch's work and the input gradient's."""
    Ho = (H + 2 * p - (k - 1) - 1) // s + 1
    per_axis = sum(1 for o in range(Ho) for r in range(k) if 0 <= o * s - p + r < H)
    return 2.0 * per_axis * per_axis * cin * cout * B * E


def layers_mode(reps):
    import torch
    from bbb_hip import ops
    for B, E in ((256, 1), (512, 10)):
        for li, (cin, cout, k, s, p, H) in enumerate(CONVS[1:], start=2):
            Ho = (H + 2 * p - (k - 1) - 1) // s + 1
            x = torch.randn(E, cin, H, H, B, device="cuda")
            w = torch.randn(E, cout, cin, k, k, device="cuda") * 0.1
            g = torch.randn(E, cout, Ho, Ho, B, device="cuda")
            wf = ops.flip_transpose_w(w)
            fl = in_bounds_flop(cin, cout, k, s, p, H, B, E)
            for what, fn in (("forward", lambda: ops.conv2d_chwn_forward(x, w, None, s, p, 1)),
                             ("dgrad", lambda: ops.conv2d_chwn_input_grad(g, w, (H, H), p, 1, w_flipped=wf, stride=s))):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(reps):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                us = t0.elapsed_time(t1) * 1e3 / reps
                print(json.dumps(dict(layer=f"conv{li}", B=B, E=E, launch=what, us_events=round(us, 2), gflop=round(fl / 1e9, 3),
                                      tflops_events=round(fl / us / 1e6, 2))), flush=True)


def parse_mode(path, reps):
    """The trace of `layers`: per (B, E, layer) 3 + reps forward launches then 3 + reps input-gradient launches, in order."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            n = r["Kernel_Name"]
            if "pconv_gemm_kernel" in n or "pconv_dgrad_kernel" in n or "pconv_gemm_splitk" in n:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n))
    rows.sort()
    i = 0
    for B, E in ((256, 1), (512, 10)):
        for li, (cin, cout, k, s, p, H) in enumerate(CONVS[1:], start=2):
            fl = in_bounds_flop(cin, cout, k, s, p, H, B, E)
            for what in ("forward", "dgrad"):
                grp = rows[i + 3:i + 3 + reps]
                i += 3 + reps
                us = sum(e - b for b, e, _ in grp) / len(grp) / 1e3
                names = sorted({re.search(r"pconv_\w+<[^>]*>", n).group(0) for _, _, n in grp})
                print(json.dumps(dict(layer=f"conv{li}", B=B, E=E, launch=what, us_kernel=round(us, 2), tflops=round(fl / us / 1e6, 2),
                                      kernel=names)))
    assert i == len(rows), (i, len(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("steps", "layers", "parse"))
    ap.add_argument("trace", nargs="?")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tag", default="")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    a = ap.parse_args()
    if a.mode == "parse":
        return parse_mode(a.trace, a.reps)
    import torch
    import layers  # noqa: F401
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if a.mode == "layers":
        return layers_mode(a.reps)
    for kind, B, E in WORKLOADS:
        for v in a.variants.split(","):
            try:
                m = measure(v, kind, B, E, a.steps, a.blocks)
            except Exception as exc:                       # (recorded, not hidden: a variant a tree cannot run is a finding)
                m = dict(error=f"{type(exc).__name__}: {exc}"[:200])
            print(json.dumps(dict(tag=a.tag, kind=kind, B=B, E=E, variant=v, **m)), flush=True)


if __name__ == "__main__":
    main()
