"""Device time of one uncertainty-scoring call on a batch, three routes inside ONE process, alternated window by window:
    parent    ensemble.mc_logits -> ops.uncertainty (pred, epistemic, aleatoric), plus predictive entropy, expected entropy and their
              difference as torch expressions on the same [T, B, C] logits -- the only way to those three scores before
              ops.mc_uncertainty_cb existed
    eager     uncertainty.mc_uncertainty: the batch-innermost logits straight into one bbb_mc_uncertainty_cb launch
    graphed   uncertainty.GraphedUncertainty.step: the same as one hipGraph replay
BBB AlexNet on CIFAR-shaped input, bs = 512, T = 15, with 10 and with 100 classes.  Device events around windows of at least
`--seconds` of calls, every route warmed first; per route the windows' ms per call, the median and the range (the spread of repeats of
the same route: a difference between routes below it is not a difference).  Nothing is copied to the host inside a window.
    python profiles/mc_uncertainty_timing.py                  a JSON line per workload
    python profiles/mc_uncertainty_timing.py --tail-only      for a kernel trace (rocprofv3 --kernel-trace --stats -- python ... --tail-only):
                                                              only the reduction launches on seeded logits of both workloads -- the new
                                                              kernel, and the parent's transpose copy + uncertainty_kernel -- 50 each,
                                                              and the bytes the new kernel has to move per launch
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}
BATCH, DRAWS = 512, 15
WORKLOADS = {"alexnet-c10": 10, "alexnet-c100": 100}


def tail_bytes(T, C, B):
    """Bytes one bbb_mc_uncertainty_cb launch must move: every logit read once, the seven outputs written once."""
    return 4 * (T * C * B + 4 * B * C + 3 * B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--tail-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
    import torch
    import layers  # noqa: F401
    from bbb_hip import ensemble, ops, rng, uncertainty, zoo

    if a.tail_only:
        for name, C in WORKLOADS.items():
            g = torch.Generator(device="cuda").manual_seed(1)
            cb = 4.0 * torch.randn((DRAWS, C, BATCH), device="cuda", generator=g)
            for _ in range(50):
                ops.mc_uncertainty_cb(cb)
                ops.uncertainty(cb.permute(0, 2, 1).contiguous())
            torch.cuda.synchronize()
            print(json.dumps(dict(workload=name, T=DRAWS, C=C, B=BATCH, tail_bytes=tail_bytes(DRAWS, C, BATCH), launches_each=50)), flush=True)
        return

    def entropies(logits):                    # [T, B, C] -> predictive entropy, expected entropy, their difference
        lp = torch.log_softmax(logits, dim=2)
        p = lp.exp()
        pbar = p.mean(dim=0)
        ent = -torch.special.xlogy(pbar, pbar).sum(dim=1)
        eent = -(p * lp).sum(dim=2).mean(dim=0)
        return ent, eent, ent - eent

    for name, C in WORKLOADS.items():
        torch.manual_seed(0)
        net = zoo.getModel("alexnet", 3, C, PRIORS, "bbb", "softplus").cuda()
        rng.assign_stream_ids(net)
        x = torch.rand(BATCH, 3, 32, 32, device="cuda")
        rng.manual_seed(7, call=0)
        graphed = uncertainty.GraphedUncertainty(net, x, DRAWS)

        def parent():
            seed, call0 = rng.next_calls(DRAWS)
            logits, _ = ensemble.mc_logits(net, x, DRAWS, seed, call0)
            return ops.uncertainty(logits) + entropies(logits)

        routes = {"parent": parent, "eager": lambda: uncertainty.mc_uncertainty(net, x, T=DRAWS), "graphed": graphed.step}

        def window(fn, calls):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / calls

        with torch.no_grad():
            calls = {}
            for k, fn in routes.items():                              # warm-up, and how many calls fill a window
                window(fn, 5)
                calls[k] = max(5, int(a.seconds * 1e3 / window(fn, 20)) + 1)
            ms = {k: [] for k in routes}
            for _ in range(a.windows):
                for k, fn in routes.items():                          # the routes alternate
                    ms[k].append(window(fn, calls[k]))
        out = dict(workload=name, bs=BATCH, T=DRAWS, classes=C, calls_per_window=calls)
        for k, v in ms.items():
            out[k] = dict(ms_per_call=[round(t, 4) for t in v], median=round(sorted(v)[len(v) // 2], 4), range=round(max(v) - min(v), 4))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
