"""bf16 input gradients of LRT models (LaunchConfig.bf16_lrt + bf16_lrt_input_grad) against the fp32 LRT node on one MI355X (numbers:
bf16_lrt_input_grad_notes.md).  Device events, every shape pre-heated, the two sides alternating block by block inside ONE process,
median and spread over the rounds.

    python profiles/bf16_lrt_input_grad_timing.py steps [--rounds 7] [--steps 50]
        an attack / saliency iteration -- ensemble.mc_forward + F.nll_loss + backward to x, frozen parameters, eager -- on LRT AlexNet at
        bs 512 x 10 draws and LRT 3Conv3FC at bs 256 x 1 draw: precision="bf16" under the two switches (_MCForwardLRTBF16) against
        precision="fp32" (_MCForwardLRT).
    python profiles/bf16_lrt_input_grad_timing.py pass [--rounds 7] [--reps 200]
        the new pass alone at AlexNet conv2's shape (10 draws x 192 channels, 4 x 4 map, 512 images, Softplus, MaxPool2d(2, 2), the
        combine of the layer above's two input gradients): bbb_lrt_pool_act_bwd_chwn_bf16 against fp32 bbb_lrt_pool_act_bwd_chwn.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# name -> (net_type, Cin, H, B, E)
MODELS = {"lrt alexnet 512x10": ("alexnet", 3, 32, 512, 10), "lrt 3conv3fc 256x1": ("3conv3fc", 3, 32, 256, 1)}
BOTH = dict(bf16_lrt=True, bf16_lrt_input_grad=True)


def timed(fn, n):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n, out


def summary(vals, digits=2):
    v = sorted(vals)
    return dict(median=round(v[len(v) // 2], digits), min=round(v[0], digits), max=round(v[-1], digits))


def alternate(fns, rounds, reps, scale, digits=2):
    import torch
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            out[n].append(timed(fn, reps)[0] * scale)
    return {n: summary(v, digits) for n, v in out.items()}


def steps_mode(a):
    import torch
    import torch.nn.functional as F
    import ref_port_torch as P
    from bbb_hip import ensemble, ops, rng, zoo
    for name, (net_type, cin, H, B, E) in MODELS.items():
        torch.manual_seed(1)
        net = zoo.getModel(net_type, cin, 10, P.CONFIG_PRIORS, "lrt", "softplus").cuda().requires_grad_(False)
        rng.assign_stream_ids(net)
        x = torch.rand(B, cin, H, H, device="cuda").requires_grad_(True)
        y = torch.randint(0, 10, (B,), device="cuda")
        paths = {}

        def step(precision):
            x.grad = None
            with ops.use_config(**BOTH):
                lo, _ = ensemble.mc_forward(net, x, E, kl_mode="mean", precision=precision)
                paths[precision] = ensemble.stats["path"]
                F.nll_loss(lo, y).backward()
            return x.grad

        ms = alternate({"fp32": lambda: step("fp32"), "bf16": lambda: step("bf16")}, a.rounds, a.steps, 1.0, digits=4)
        grads = {}
        for precision in ("fp32", "bf16"):                                # the same noise for both: the timed iterations each drew their own
            rng.manual_seed(7, call=3)
            grads[precision] = step(precision).double().flatten().clone()
        rng.use_device_generator()
        a32, a16 = grads["fp32"], grads["bf16"]
        cos = float(a32 @ a16 / (a32.norm() * a16.norm()))
        for n, v in ms.items():
            print(json.dumps(dict(model=name, precision=n, path=paths[n], ms_per_iteration=v)), flush=True)
        print(json.dumps(dict(model=name, bf16_over_fp32=round(ms["bf16"]["median"] / ms["fp32"]["median"], 3), cosine_dx=round(cos, 5))), flush=True)


def pass_mode(a):
    import torch
    import torch.nn.functional as F
    from bbb_hip import ops
    E, C, H, B, k, s = 10, 192, 4, 512, 2, 2
    hp = (H - k) // s + 1
    r = lambda *sh: torch.randn(*sh, device="cuda")
    y32 = F.softplus(r(E, C, H, H, B))
    am, av = r(E, C, H, H, B), 0.02 + torch.rand(E, C, H, H, B, device="cuda")
    d1, d2, xo = r(E, C, hp, hp, B), r(E, C, hp, hp, B), r(E, C, hp, hp, B)
    bf = lambda t: t.to(torch.bfloat16)
    y16, d1b, d2b, xob = bf(y32), bf(d1), bf(d2), bf(xo)
    fns = {"fp32 bbb_lrt_pool_act_bwd_chwn": lambda: ops.lrt_pool_act_backward_chwn(d1, y32, am, av, k, s, "softplus", stacked=True, combine=(xo, d2)),
           "bf16 bbb_lrt_pool_act_bwd_chwn_bf16": lambda: ops.lrt_pool_act_backward_chwn_bf16(d1b, y16, av, k, s, "softplus", noise=(7, 3, 5),
                                                                                              combine=(xob, d2b))}
    us = alternate(fns, a.rounds, a.reps, 1e3)
    n, np_ = E * C * H * H * B, E * C * hp * hp * B
    mbytes = {"fp32 bbb_lrt_pool_act_bwd_chwn": 4 * (5 * n + 3 * np_), "bf16 bbb_lrt_pool_act_bwd_chwn_bf16": 2 * (3 * n + 3 * np_) + 4 * n}
    for name, v in us.items():
        print(json.dumps(dict(shape=[E, C, H, H, B], pool=[k, s], launch=name, us=v, mbytes=round(mbytes[name] / 1e6, 1),
                              tb_per_s=round(mbytes[name] / v["median"] / 1e6, 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("steps", "pass"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    import torch
    import layers  # noqa: F401
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    (steps_mode if a.mode == "steps" else pass_mode)(a)


if __name__ == "__main__":
    main()
