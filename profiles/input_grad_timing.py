"""d loss / d x of a Monte-Carlo forward on one MI355X, ms per step from device events, the three variants interleaved in rounds
inside one process (same clocks, same box):
  (a) "node":   ensemble.mc_forward + backward to x with frozen weights -- the batch-innermost autograd node, whose backward ends in
                the first layer's input gradient (ops.first_layer_input_grad) and skips the weight side;
  (b) "loop":   the path that served this gradient before: a `net(x)` loop of num_ens calls with x.requires_grad (the per-layer
                reference-layout path), log_softmax / logmeanexp / nll, backward to x;
  (c) "train":  the fp32 training step, train.train_step(graph=False) (launch by launch, as (a) and (b)).
Workloads: BayesianAlexNet CIFAR-10 bs 512 x 10 draws (BBB), Bayesian3Conv3FC bs 256 x 1 (BBB), the LRT default (AlexNet, bs 256 x 1).
    python profiles/input_grad_timing.py [--rounds 3] [--steps 20]
    python profiles/input_grad_timing.py --only node --config alexnet --rounds 1 --steps 10     (a short run to trace with rocprofv3)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import layers  # noqa: E402,F401
from bbb_hip import ensemble, rng, train, zoo  # noqa: E402

PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}
CONFIGS = {"alexnet": ("alexnet", "bbb", 512, 10), "3conv3fc": ("3conv3fc", "bbb", 256, 1), "alexnet_lrt": ("alexnet", "lrt", 256, 1)}
VARIANTS = ("node", "loop", "train")


def _logmeanexp(t, dim):
    m = t.max(dim=dim, keepdim=True)[0]
    return (m + torch.log(torch.mean(torch.exp(t - m), dim=dim, keepdim=True))).squeeze(dim)


def make(net_type, lt, B):
    torch.manual_seed(0)
    net = zoo.getModel(net_type, 3, 10, PRIORS, lt, "softplus").cuda()
    rng.assign_stream_ids(net)
    x = torch.rand(B, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (B,), device="cuda")
    return net, x, y


def step_fn(variant, net, x, y, E):
    if variant == "train":
        net.requires_grad_(True)
        opt = train.FusedAdam(net.parameters(), lr=1e-9)

        def step():
            return train.train_step(net, opt, x, y, E, 0.1, 50000.0, graph=False)[0]
        return step
    net.requires_grad_(False)
    xg = x.clone().requires_grad_(True)

    def step():
        xg.grad = None
        if variant == "node":
            lo, _ = ensemble.mc_forward(net, xg, E)
            assert ensemble.stats["path"] == "chwn-autograd"
        else:
            outs = [F.log_softmax(net(xg)[0], dim=1) for _ in range(E)]
            lo = _logmeanexp(torch.stack(outs, dim=2), 2)
        loss = F.nll_loss(lo, y)
        loss.backward()
        return loss.detach()
    return step


def measure(cfg, variant, steps, warm=3):
    net_type, lt, B, E = CONFIGS[cfg]
    net, x, y = make(net_type, lt, B)
    step = step_fn(variant, net, x, y, E)
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        loss = step()
    t1.record()
    torch.cuda.synchronize()
    return dict(ms=t0.elapsed_time(t1) / steps, loss=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--config", choices=tuple(CONFIGS))
    a = ap.parse_args()
    variants = (a.only,) if a.only else VARIANTS
    cfgs = (a.config,) if a.config else tuple(CONFIGS)
    res = {}
    for r in range(a.rounds):
        for c in cfgs:
            for v in variants:
                m = measure(c, v, a.steps)
                res.setdefault((c, v), []).append(m)
                print(json.dumps(dict(round=r, config=c, variant=v, **m)), flush=True)
    print("summary (median over rounds): config variant ms/step")
    for (c, v), ms in res.items():
        t = sorted(m["ms"] for m in ms)[len(ms) // 2]
        print(f"  {c:12s} {v:6s} {t:9.3f}")


if __name__ == "__main__":
    main()
