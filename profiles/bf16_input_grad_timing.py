"""bf16 input gradients (LaunchConfig.bf16_input_grad) against the fp32 node on one MI355X (numbers: bf16_input_grad_notes.md).

Two first layers: BayesianAlexNet conv1 (3 -> 64, 11 x 11 / 4, padding 5, 32 x 32 images) at bs 512 x 10 draws and Bayesian3Conv3FC
conv1 (3 -> 32, 5 x 5, padding 2) at bs 256 x 1 draw.  Device events, every shape pre-heated, the two sides alternating block by block
inside ONE process, median and spread over the rounds.

    python profiles/bf16_input_grad_timing.py launch [--rounds 7] [--reps 200]
        the contraction over (draw, channel) alone, on the same numbers: bf16 = ONE launch of bbb_first_layer_dgrad_bf16 on the sampled
        rows and g_pre where they are (g_pre as bf16, and as the fp32 values at the padded pitch a trainable step hands it);
        fp32 = what ops.first_layer_input_grad does before its gather, bbb_transpose2d of the weights + bbb_conv2d_chwn_fwd as a
        1 x 1 convolution over the fp32 values of the same operands.  Then both wrappers whole (contraction + the shared gather).
    python profiles/bf16_input_grad_timing.py steps [--rounds 7] [--steps 50]
        ensemble.mc_forward + F.nll_loss + backward to x with frozen parameters (an attack / saliency iteration), precision="bf16"
        under the switch against precision="fp32", eager.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# name -> (net_type, Cin, Cout, k, stride, padding, H, B, E)
FIRST_LAYERS = {"alexnet conv1 512x10": ("alexnet", 3, 64, 11, 4, 5, 32, 512, 10), "3conv3fc conv1 256x1": ("3conv3fc", 3, 32, 5, 1, 2, 32, 256, 1)}


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


def launch_mode(a):
    import torch
    from bbb_hip import _lib, ops
    L = _lib.lib()
    for name, (_, cin, cout, k, s, p, H, B, E) in FIRST_LAYERS.items():
        Ho = (H + 2 * p - (k - 1) - 1) // s + 1
        J, M, K = cin * k * k, E * cout, Ho * Ho * B
        wshape = (cout, cin, k, k)
        w = (torch.randn(E, cout, cin, k, k, device="cuda") * 0.1).to(torch.bfloat16)
        g = torch.randn(E, cout, Ho, Ho, B, device="cuda").to(torch.bfloat16)
        rows = torch.zeros(E, cout, ops.bf16_row_pitch(J), dtype=torch.bfloat16, device="cuda")
        rows[:, :, :J] = w.reshape(E, cout, J)
        g32 = ops.pool_act_backward_chwn_bf16(g, None, 0, 1, None, out_f32=True, pad_planes=True)      # the fp32 values, padded pitch
        w32 = w.float().contiguous()
        d, _, _ = ops._first_layer_desc(B, cin, cout, k, k, (H, H), s, p, 1, E)
        dcol = torch.empty((J, K), dtype=torch.float32, device="cuda")
        st = lambda: _lib.cur_stream(g.device)

        def bf16_launch(gg, flags):
            _lib.check(L.bbb_first_layer_dgrad_bf16(ctypes.byref(d), gg.data_ptr(), gg.stride(1), rows.data_ptr(), dcol.data_ptr(), K, flags,
                                                    st()), "bbb_first_layer_dgrad_bf16")

        def fp32_contraction():
            xg, P = ops._gemm_rows([g32])
            wt = torch.empty((1, J, M, 1, 1), dtype=torch.float32, device="cuda")
            _lib.check(L.bbb_transpose2d(w32.data_ptr(), wt.data_ptr(), M, J, st()), "bbb_transpose2d")
            return ops.conv2d_chwn_forward(xg, wt, None)

        geom = ((H, H), s, p, 1)
        fns = {"bf16 contraction, g_pre bf16": lambda: bf16_launch(g, 0),
               "bf16 contraction, g_pre fp32 padded": lambda: bf16_launch(g32, 1),
               "fp32 transpose + GEMM": fp32_contraction,
               "first_layer_input_grad_bf16 (g_pre bf16)": lambda: ops.first_layer_input_grad_bf16(g, rows, wshape, *geom),
               "first_layer_input_grad_bf16 (g_pre fp32 padded)": lambda: ops.first_layer_input_grad_bf16(g32, rows, wshape, *geom),
               "first_layer_input_grad (fp32)": lambda: ops.first_layer_input_grad(g32, w32, *geom)}
        us = alternate(fns, a.rounds, a.reps, 1e3)
        plan = ops.first_layer_dgrad_bf16_plan(B, wshape, (H, H), s, p, 1, E)
        for n, v in us.items():
            print(json.dumps(dict(layer=name, M=M, J=J, columns=K, gflop=round(2e-9 * M * J * K, 3), plan=plan, launch=n, us=v)), flush=True)


def steps_mode(a):
    import torch
    import torch.nn.functional as F
    import ref_port_torch as P
    from bbb_hip import ensemble, ops, rng, zoo
    for name, (net_type, cin, _, _, _, _, H, B, E) in FIRST_LAYERS.items():
        torch.manual_seed(1)
        net = zoo.getModel(net_type, cin, 10, P.CONFIG_PRIORS, "bbb", "softplus").cuda().requires_grad_(False)
        rng.assign_stream_ids(net)
        x = torch.rand(B, cin, H, H, device="cuda").requires_grad_(True)
        y = torch.randint(0, 10, (B,), device="cuda")
        paths = {}

        def step(precision):
            x.grad = None
            with ops.use_config(bf16_input_grad=True):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("launch", "steps"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    import torch
    import layers  # noqa: F401
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    (launch_mode if a.mode == "launch" else steps_mode)(a)


if __name__ == "__main__":
    main()
