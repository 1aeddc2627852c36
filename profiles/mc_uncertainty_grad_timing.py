"""Device time of one saliency iteration -- T forwards, the three per-image scores, then backward to the batch -- two routes inside
ONE process, alternated window by window, on the same batch-innermost autograd node (fast_train.mc_logits_autograd, frozen weights):
    parent    the only route before ops.mc_uncertainty_cb_autograd existed: predictive entropy, expected entropy and mutual information
              as torch expressions on the permuted [T, B, C] logits (xlogy forms, so a zero probability gives no NaN forward)
    new       ops.mc_uncertainty_cb_autograd on the node's [T, C, B] output: one reduction launch forward, one backward
Both differentiate (entropy + expected_entropy + mutual_info).sum() with torch.autograd.grad on the input alone.
BBB AlexNet on CIFAR-shaped input, bs = 512, T = 15, with 10 and with 100 classes.  Device events around windows of at least
`--seconds` of iterations, every route warmed first; per route the windows' ms per iteration, the median and the range (the spread of
repeats of the same route: a difference between routes below it is not a difference).  Nothing is copied to the host inside a window.
    python profiles/mc_uncertainty_grad_timing.py               a JSON line per workload
    python profiles/mc_uncertainty_grad_timing.py --tail-only   for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...
                                                                --tail-only): only the score tails on seeded logits of both workloads,
                                                                forward and backward to the logits -- the new entry's two launches and
                                                                the torch expressions' -- 50 each, and the bytes the backward launch
                                                                has to move
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}
BATCH, DRAWS = 512, 15
WORKLOADS = {"alexnet-c10": 10, "alexnet-c100": 100}
SCORES = ("entropy", "expected_entropy", "mutual_info")


def bwd_bytes(T, C, B):
    """Bytes one bbb_mc_uncertainty_cb_bwd launch must move: every logit read once, every gradient written once, p_mean and the three
    per-image upstream gradients read once."""
    return 4 * (2 * T * C * B + B * C + 3 * B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--tail-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
    import torch
    import layers  # noqa: F401
    from bbb_hip import fast_train, ops, rng, zoo

    def torch_scores(logits):                 # [T, B, C] -> the sum of the three scores over the batch
        lp = torch.log_softmax(logits, dim=2)
        p = lp.exp()
        pbar = p.mean(dim=0)
        ent = -torch.special.xlogy(pbar, pbar).sum(dim=1)
        eent = -torch.special.xlogy(p, p).sum(dim=2).mean(dim=0)
        mi = (torch.special.xlogy(p, p) - torch.special.xlogy(p, pbar[None])).sum(dim=2).mean(dim=0)
        return (ent + eent + mi).sum()

    def new_scores(logits_cb):                # [T, C, B]
        out = ops.mc_uncertainty_cb_autograd(logits_cb, want=SCORES)
        return (out.entropy + out.expected_entropy + out.mutual_info).sum()

    if a.tail_only:
        for name, C in WORKLOADS.items():
            g = torch.Generator(device="cuda").manual_seed(1)
            cb = (4.0 * torch.randn((DRAWS, C, BATCH), device="cuda", generator=g)).requires_grad_(True)
            for _ in range(50):
                torch.autograd.grad(new_scores(cb), cb)
                torch.autograd.grad(torch_scores(cb.permute(0, 2, 1)), cb)
            torch.cuda.synchronize()
            print(json.dumps(dict(workload=name, T=DRAWS, C=C, B=BATCH, bwd_bytes=bwd_bytes(DRAWS, C, BATCH), iterations_each=50)),
                  flush=True)
        return

    for name, C in WORKLOADS.items():
        torch.manual_seed(0)
        net = zoo.getModel("alexnet", 3, C, PRIORS, "bbb", "softplus").cuda().requires_grad_(False)
        rng.assign_stream_ids(net)
        x = torch.rand(BATCH, 3, 32, 32, device="cuda").requires_grad_(True)
        rng.manual_seed(7, call=0)
        assert fast_train.train_path_ok(net, x) == "bbb"

        def iteration(scores, permute):
            seed, call0 = rng.next_calls(DRAWS)
            logits_cb, _ = fast_train.mc_logits_autograd(net, x, DRAWS, seed, call0)
            return torch.autograd.grad(scores(logits_cb.permute(0, 2, 1) if permute else logits_cb), x)[0]

        routes = {"parent": lambda: iteration(torch_scores, True), "new": lambda: iteration(new_scores, False)}

        def window(fn, calls):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / calls

        calls = {}
        for k, fn in routes.items():                                  # warm-up, and how many iterations fill a window
            window(fn, 5)
            calls[k] = max(5, int(a.seconds * 1e3 / window(fn, 20)) + 1)
        ms = {k: [] for k in routes}
        for _ in range(a.windows):
            for k, fn in routes.items():                              # the routes alternate
                ms[k].append(window(fn, calls[k]))
        ga, gb = routes["parent"](), routes["new"]()                  # (different noise calls: magnitudes only)
        out = dict(workload=name, bs=BATCH, T=DRAWS, classes=C, calls_per_window=calls,
                   grad_abs_max=dict(parent=float(ga.abs().max()), new=float(gb.abs().max())))
        for k, v in ms.items():
            out[k] = dict(ms_per_call=[round(t, 4) for t in v], median=round(sorted(v)[len(v) // 2], 4), range=round(max(v) - min(v), 4))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
