"""fp32 LRT vs bf16 LRT inference (ensemble precision="bf16" under LaunchConfig.bf16_lrt) on one MI355X.
The two modes alternate block by block inside one process (same box, same clocks); a timed block is `--steps` replays of a
captured step (GraphedPipeline, depth 1) behind a preheat, timed with device events; the report is the median block of each mode
with the spread (min .. max) over the blocks, the speed-up, and each mode's peak memory while its step is warmed up and
captured (torch.cuda.max_memory_allocated).
    python profiles/bf16_lrt_timing.py [--blocks 7] [--steps 30]
    python profiles/bf16_lrt_timing.py --layers          (the AlexNet layers' GEMM launches one by one: us and useful TFLOP/s)
    python profiles/bf16_lrt_timing.py --only bf16 --shape alexnet-e10 --blocks 1     (a short run to trace with rocprofv3)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
import torch  # noqa: E402

import layers  # noqa: E402,F401
from bbb_hip import ensemble, ops, rng, zoo  # noqa: E402

PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}
# name -> (model, classes, batch, draws, steps per launch)
SHAPES = {"alexnet100-e1x16": ("alexnet", 100, 512, 1, 16),      # BASELINE configs[2]: AlexNet CIFAR-100, LRT, bs 512
          "alexnet-e10": ("alexnet", 10, 512, 10, 1),
          "3conv3fc-e1": ("3conv3fc", 10, 256, 1, 1)}


def build(shape, precision):
    net_type, classes, B, E, G = SHAPES[shape]
    torch.manual_seed(0)
    net = zoo.getModel(net_type, 3, classes, PRIORS, "lrt", "softplus").cuda()
    rng.assign_stream_ids(net)
    x = torch.rand(B, 3, 32, 32, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad(), ops.use_config(bf16_lrt=(precision == "bf16")):
        pipe = ensemble.GraphedPipeline(net, x, E, depth=1, steps_per_launch=G, precision=precision)
    torch.cuda.synchronize()
    peak_mb = (torch.cuda.max_memory_allocated() - base) / 2 ** 20      # warm-up + capture: the step's buffers live in the graph's pool
    return pipe, x, G, peak_mb, net


def block(pipe, x, G, steps):
    """ms per STEP over `steps` launches of G steps each."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for _ in range(3 * G):                      # preheat
            pipe.step(x)
        pipe.sync()
        t0.record()
        for _ in range(steps * G):
            pipe.step(x)
        pipe.sync()
        t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / (steps * G)


def layer_times(reps=30):
    """The GEMM launches of AlexNet's layers (bs 512, 10 draws) on the bf16 LRT kernel and on the fp32 LRT kernel, one by one."""
    B, E = 512, 10
    geo = [("conv1", 3, 32, 64, 11, 4, 5), ("conv2", 64, 4, 192, 5, 1, 2), ("conv3", 192, 2, 384, 3, 1, 1),
           ("conv4", 384, 2, 256, 3, 1, 1), ("conv5", 256, 2, 128, 3, 1, 1), ("classifier", 128, 1, 10, 1, 1, 0)]
    for name, cin, hw, cout, k, s, p in geo:
        Ex = 1 if name == "conv1" else E
        x = torch.rand(Ex, cin, hw, hw, B, device="cuda")
        w_mu = torch.randn(cout, cin, k, k, device="cuda") * 0.05
        w_var = torch.rand(cout, cin, k, k, device="cuda") * 1e-3
        b_mu, b_var = torch.zeros(cout, device="cuda"), torch.full((cout,), 1e-4, device="cuda")
        tapm = ops.bf16_tap_major((cout, cin, k, k))
        wm_b, wv_b = ops.lrt_weights_bf16([w_mu if tapm else w_mu.reshape(cout, -1), w_var if tapm else w_var.reshape(cout, -1)])
        xb = x.to(torch.bfloat16)
        mo = name == "conv1"                        # shared first layer: one moments-only launch
        f16 = lambda: ops.lrt_conv2d_chwn_bf16_forward(xb, wm_b, wv_b, b_mu, b_var, (cin, k, k), 1, 0, 2, s, p, 1, act="softplus",
                                                       tap_major=tapm, sample=not mo, moments_only=mo, out_f32=name == "classifier")
        f32 = lambda: ops.lrt_conv2d_chwn_forward(x, w_mu, w_var, b_mu, b_var, 1, 0, 2, s, p, 1, act=None if mo else "softplus",
                                                  sample=not mo, want_moments=mo)
        useful, _ = ensemble.conv_flops(B, cin, hw, hw, cout, k, k, s, p, 1, Ex, 2)
        row = dict(layer=name, plan=ops.lrt_bf16_plan((Ex, cin, hw, hw, B), cout, (cin, k, k), s, p, 1), useful_gflop=useful / 1e9)
        for tag, fn in (("bf16", f16), ("fp32", f32)):
            for _ in range(5):
                fn()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / reps
            row[tag + "_us"] = round(us, 2)
            row[tag + "_tflops"] = round(useful / us / 1e6, 1)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only", choices=("fp32", "bf16"))
    ap.add_argument("--shape", choices=tuple(SHAPES))
    ap.add_argument("--layers", action="store_true")
    a = ap.parse_args()
    if a.layers:
        layer_times()
        return
    precs = (a.only,) if a.only else ("fp32", "bf16")
    for shape in ((a.shape,) if a.shape else tuple(SHAPES)):
        pipes = {p: build(shape, p) for p in precs}
        peak = {p: pipes[p][3] for p in precs}
        ms = {p: [] for p in precs}
        for b in range(a.blocks):
            for p in precs:                          # the modes alternate
                pipe, x, G, _, _ = pipes[p]
                ms[p].append(block(pipe, x, G, a.steps))
        out = dict(shape=shape, steps_per_block=a.steps * SHAPES[shape][4], blocks=a.blocks)
        for p in precs:
            v = sorted(ms[p])
            out[p] = dict(median_ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4), peak_mb=round(peak[p], 1))
        if len(precs) == 2:
            out["speedup"] = round(out["fp32"]["median_ms"] / out["bf16"]["median_ms"], 3)
            spread = (out["fp32"]["max_ms"] - out["fp32"]["min_ms"]) + (out["bf16"]["max_ms"] - out["bf16"]["min_ms"])
            out["faster_by_more_than_the_combined_spread"] = out["fp32"]["median_ms"] - out["bf16"]["median_ms"] > spread
        print(json.dumps(out), flush=True)
        del pipes


if __name__ == "__main__":
    main()
