"""fp32 vs bf16 training behind strided layers (LaunchConfig.bf16_strided_train) on one MI355X (numbers: bf16_strided_train_notes.md).

The model is strided_dgrad_timing.py's: Bayesian3Conv3FC with its three MaxPool2d(3, 2) removed and each 5 x 5 convolution given
stride 2 (32 x 32 -> 16 -> 8 -> 3; conv2 and conv3 are strided later layers), BBB layers, bs 256 x 1 draw and bs 512 x 10 draws.
The baseline is the fp32 step: without the switch precision="bf16" refuses this model.

    python profiles/bf16_strided_train_timing.py steps [--rounds 5] [--steps 30] [--modes eager,captured]
        ms per step from device events.  fp32 and bf16 alternate block by block inside ONE process (a block = `steps` steps after
        a warm-up of every shape; both precisions' steps are built and warmed before the first timed block), median and spread over
        the rounds.  Against the parent commit only the fp32 rows run (`--only fp32`): a copy of this script placed in a checkout
        of the parent measures the parent.
    python profiles/bf16_strided_train_timing.py layers [--rounds 5] [--reps 50]
        per strided layer the input-gradient launch alone: the fp32 transposed launch (ops.conv2d_chwn_input_grad(stride=2)) and the
        bf16 one (ops.conv2d_chwn_input_grad_bf16(stride=2)) of this tree, alternating, `reps` launches per block; us per launch,
        TFLOP/s of in-bounds work, and the form the bf16 launch takes (ops.bf16_dgrad_form).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from strided_dgrad_timing import CONVS, build, in_bounds_flop  # noqa: E402

WORKLOADS = [(256, 1), (512, 10)]


def make_step(B, E, precision, captured):
    import torch
    from bbb_hip import ops, train
    net = build("bbb")
    x = torch.rand(B, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (B,), device="cuda")
    opt = train.FusedAdam(net.parameters(), lr=1e-9, capturable=captured)
    cfg = ops.current_config().copy(bf16_strided_train=True) if (precision == "bf16" and hasattr(ops.LaunchConfig(), "bf16_strided_train")) \
        else ops.current_config().copy()
    if captured:
        g = train.GraphedTrainStep(net, opt, x, y, E, 0.1, 50000.0, warmup=3, launch_config=cfg, precision=precision)
        return lambda: g.step()[0]

    def step():
        with ops.use_config(cfg):
            return train.train_step(net, opt, x, y, E, 0.1, 50000.0, graph=False, precision=precision)[0]
    return step


def timed(fn, n):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n, out


def summary(vals):
    v = sorted(vals)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def steps_mode(a):
    import torch
    precs = (a.only,) if a.only else ("fp32", "bf16")
    for B, E in WORKLOADS:
        for mode in a.modes.split(","):
            fns = {p: make_step(B, E, p, mode == "captured") for p in precs}
            for p in precs:                                          # every shape of the timed window, both precisions
                for _ in range(5):
                    fns[p]()
            torch.cuda.synchronize()
            ms = {p: [] for p in precs}
            loss = {}
            for _ in range(a.rounds):
                for p in precs:
                    t, out = timed(fns[p], a.steps)
                    ms[p].append(t)
                    loss[p] = float(out)
            for p in precs:
                print(json.dumps(dict(tag=a.tag, B=B, E=E, mode=mode, precision=p, ms_per_step=summary(ms[p]), loss=loss[p])), flush=True)
            if len(precs) == 2:
                f, b = summary(ms["fp32"])["median"], summary(ms["bf16"])["median"]
                print(json.dumps(dict(tag=a.tag, B=B, E=E, mode=mode, bf16_over_fp32=round(b / f, 3))), flush=True)


def layers_mode(a):
    import torch
    from bbb_hip import ops
    for B, E in WORKLOADS:
        for li, (cin, cout, k, s, p, H) in enumerate(CONVS[1:], start=2):
            Ho = (H + 2 * p - (k - 1) - 1) // s + 1
            w = torch.randn(E, cout, cin, k, k, device="cuda") * 0.1
            g = torch.randn(E, cout, Ho, Ho, B, device="cuda")
            wf = ops.flip_transpose_w(w)
            wshape = (cout, cin, k, k)
            tm = ops.bf16_tap_major(wshape)
            rows = torch.zeros(E, cout, ops.bf16_row_pitch(cin * k * k), dtype=torch.bfloat16, device="cuda")
            rows[:, :, :cin * k * k] = (w.permute(0, 1, 3, 4, 2) if tm else w).reshape(E, cout, -1).to(torch.bfloat16)
            wfb = ops.flip_transpose_w_bf16(rows, wshape)
            gb = g.to(torch.bfloat16)
            fns = {"fp32": lambda: ops.conv2d_chwn_input_grad(g, w, (H, H), p, 1, w_flipped=wf, stride=s),
                   "bf16": lambda: ops.conv2d_chwn_input_grad_bf16(gb, rows, wshape, (H, H), p, 1, w_flipped=wfb, stride=s)}
            for fn in fns.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            us = {n: [] for n in fns}
            for _ in range(a.rounds):
                for n, fn in fns.items():
                    us[n].append(timed(fn, a.reps)[0] * 1e3)
            fl = in_bounds_flop(cin, cout, k, s, p, H, B, E)
            form = ops.bf16_dgrad_form(B, cin, cout, k, k, (H, H), s, 1, E)
            for n in fns:
                sm = summary(us[n])
                print(json.dumps(dict(tag=a.tag, layer=f"conv{li}", B=B, E=E, launch=f"dgrad-{n}", us=sm, gflop=round(fl / 1e9, 3),
                                      tflops=round(fl / sm["median"] / 1e6, 2), **({"bf16_form": form} if n == "bf16" else {}))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("steps", "layers"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--modes", default="eager,captured")
    ap.add_argument("--only", choices=("fp32", "bf16"))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import torch
    import layers  # noqa: F401
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    (steps_mode if a.mode == "steps" else layers_mode)(a)


if __name__ == "__main__":
    main()
