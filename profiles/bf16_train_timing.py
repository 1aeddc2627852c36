"""fp32 vs bf16 training step (train.train_step(precision=...)) on one MI355X: ms per step from device events and the step's peak
memory (torch.cuda.max_memory_allocated), eager (launch by launch, graph=False) and captured (one GraphedTrainStep replay per
step).  The two precisions alternate in rounds inside one process, so clocks and the box are the same for both.
    python profiles/bf16_train_timing.py [--rounds 3] [--steps 40]
    python profiles/bf16_train_timing.py --only bf16 --config alexnet --steps 20     (a short run to trace with rocprofv3)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
import torch  # noqa: E402

import layers  # noqa: E402,F401
from bbb_hip import rng, train, zoo  # noqa: E402

PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}
CONFIGS = {"alexnet": ("alexnet", 512, 10), "3conv3fc": ("3conv3fc", 256, 1)}


def measure(net_type, B, E, precision, captured, steps, warm=5):
    torch.manual_seed(0)
    net = zoo.getModel(net_type, 3, 10, PRIORS, "bbb", "softplus").cuda()
    rng.assign_stream_ids(net)
    x = torch.rand(B, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (B,), device="cuda")
    opt = train.FusedAdam(net.parameters(), lr=1e-3, capturable=captured)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    if captured:
        g = train.GraphedTrainStep(net, opt, x, y, E, 0.1, 50000.0, warmup=2, precision=precision)
        step = lambda: g.step()
    else:
        step = lambda: train.train_step(net, opt, x, y, E, 0.1, 50000.0, graph=False, precision=precision)
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        loss = step()[0]
    t1.record()
    torch.cuda.synchronize()
    return dict(ms=t0.elapsed_time(t1) / steps, peak_mb=(torch.cuda.max_memory_allocated() - base) / 2 ** 20, loss=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--only", choices=("fp32", "bf16"))
    ap.add_argument("--config", choices=tuple(CONFIGS))
    ap.add_argument("--modes", default="eager,captured")
    a = ap.parse_args()
    precs = (a.only,) if a.only else ("fp32", "bf16")
    cfgs = (a.config,) if a.config else tuple(CONFIGS)
    res = {}
    for r in range(a.rounds):
        for c in cfgs:
            for mode in a.modes.split(","):
                for p in precs:
                    m = measure(*CONFIGS[c], p, mode == "captured", a.steps)
                    res.setdefault((c, mode, p), []).append(m)
                    print(json.dumps(dict(round=r, config=c, mode=mode, precision=p, **m)), flush=True)
    print("summary (median over rounds): config mode precision ms/step peak_MB")
    for (c, mode, p), ms in res.items():
        t = sorted(m["ms"] for m in ms)[len(ms) // 2]
        print(f"  {c:9s} {mode:8s} {p:5s} {t:8.3f} {max(m['peak_mb'] for m in ms):9.1f}")


if __name__ == "__main__":
    main()
