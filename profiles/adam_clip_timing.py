"""Device time of FusedAdam.step with and without the options of the clipped step, and of the training step that contains it
(profiles/adam_clip_notes.md).  Everything inside ONE process, variants alternated window by window, device events around each window;
per variant the windows' times, their median and their range (the spread of repeats of the same variant: a difference between
variants below it is not a difference).  Nothing is copied to the host inside a window.
    python profiles/adam_clip_timing.py                 optimizer step on the parameters of zoo.BBBAlexNet(10, 3) with gradients present:
                                                        default | max_grad_norm | max_grad_norm + L2 | skip_nonfinite; then the captured
                                                        training step at the reference's defaults (lrt, bs 256, num_ens 1), default
                                                        against clipped, and the launch-by-launch step at bs 512 x 10
    python profiles/adam_clip_timing.py --step-only     the optimizer steps only, 50 per variant, for a kernel trace
                                                        (rocprofv3 --kernel-trace --stats -- python ... --step-only)
    python profiles/adam_clip_timing.py --default-only  the default optimizer's training steps only (bench.py's training_step workloads):
                                                        runs on a tree without the options too, for a comparison with the parent commit
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}


def windows(fns, steps, rounds, torch):
    """{name: [ms per call, one per round]}: the variants take turns, `steps` calls per window."""
    out = {k: [] for k in fns}
    for k, f in fns.items():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / steps)
    return out


def report(what, res, **extra):
    line = {"what": what}
    for k, v in res.items():
        line[k] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}
    line.update(extra)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--default-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
    import torch
    import layers  # noqa: F401
    from bbb_hip import rng, train, zoo
    dev = torch.device("cuda")

    def alexnet(kind):
        torch.manual_seed(0)
        net = zoo.getModel("alexnet", 3, 10, PRIORS, kind, "softplus").to(dev)
        rng.assign_stream_ids(net)
        return net

    if not a.default_only:
        net = alexnet("bbb")
        params = list(net.parameters())
        n = sum(p.numel() for p in params)
        for p in params:
            p.grad = torch.randn_like(p) * 1e-2
        variants = {"default": {}, "max_grad_norm": dict(max_grad_norm=1.0), "max_grad_norm+l2": dict(max_grad_norm=1.0, weight_decay=1e-2),
                    "skip_nonfinite": dict(skip_nonfinite=True)}
        opts = {k: train.FusedAdam(params, lr=1e-5, capturable=True, **kw) for k, kw in variants.items()}
        fns = {k: o.step for k, o in opts.items()}
        if a.step_only:
            for k, f in fns.items():
                for _ in range(50):
                    f()
            torch.cuda.synchronize()
            print(json.dumps({"elements": n, "tensors": len(params), "sumsq_bytes": 4 * n, "adam_bytes": 28 * n}))
            return
        report("FusedAdam.step, BBBAlexNet(10, 3) parameters, capturable, launch by launch", windows(fns, a.steps, a.rounds, torch),
               elements=n, tensors=len(params), sumsq_bytes=4 * n, norm=float(opts["max_grad_norm"].grad_norm))
        graphs = {}
        for k, o in opts.items():                       # the same steps as one hipGraph each: device time without the host's launch cost
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                o.step()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                o.step()
            graphs[k] = g.replay
        report("the same steps, each captured as one hipGraph", windows(graphs, a.steps, a.rounds, torch), elements=n)
        del opts, graphs, fns, net, params
    # the training step at the reference's defaults, captured (train_step's own self-capture), and launch by launch at bs 512 x 10
    for kind, B, E, what in (("lrt", 256, 1, "captured train_step, BBBAlexNet lrt bs 256 num_ens 1"),
                             ("bbb", 512, 10, "train_step launch by launch, BBBAlexNet bbb bs 512 num_ens 10")):
        x = torch.rand(B, 3, 32, 32, device=dev)
        y = torch.randint(0, 10, (B,), device=dev)
        fns = {}
        for name, kw in (("default", {}),) + (() if a.default_only else (("clipped", dict(max_grad_norm=1.0)),)):
            net = alexnet(kind)
            opt = train.FusedAdam(net.parameters(), lr=1e-5, **kw)
            fns[name] = (lambda net=net, opt=opt: train.train_step(net, opt, x, y, E, 0.1, 50000.0))
        res = windows(fns, max(10, a.steps // (1 if E == 1 else 10)), a.rounds, torch)
        report(what, res)


if __name__ == "__main__":
    main()
