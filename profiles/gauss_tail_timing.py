"""Device time of the Gaussian-likelihood loss tail (csrc/gauss_tail.hip through ops.gauss_elbo_cb_autograd) against the same tail as the
torch expression train.gaussian_elbo under autograd, on the same tensors, and of one whole train_step each way
(profiles/gauss_tail_notes.md).  Everything inside ONE process, the variants alternated window by window, device events around each
window; per variant the windows' times, their median and their range (the spread of repeats of the same variant: a difference between
variants below it is not a difference).  Nothing is copied to the host inside a window.
    python profiles/gauss_tail_timing.py             the tails, forward + backward, on logits [10, 16, 512] and [1, 16, 256] (D = 8,
                                                     heteroscedastic), with the device launches of one forward + backward each way;
                                                     then train_step on zoo AlexNet with outputs = 16, HIP tail against torch tail
                                                     (bs 512 x 10 launch by launch, bs 256 x 1 self-captured)
    python profiles/gauss_tail_timing.py --errors    worst |device - float64| / (U x scale) per operation over the cases of
                                                     tests/gauss_tail_contract.py, next to its bound
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


def launches(f, torch):
    """Device kernels of one call of f, from torch's own profiler (None where it records none)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        f()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            f()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as e:                       # a measurement aid: the times do not depend on it
        return "profiler unavailable: %s" % type(e).__name__


def errors(torch, ops, train):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gauss_tail_contract as K
    worst = {}
    for c in K.CASES:
        logits, y = K.inputs(c)
        ref = K.reference(c, logits, y)
        lik = train.GaussianLikelihood(noise_sigma=c.noise_sigma, log_var_min=c.log_var_min, log_var_max=c.log_var_max, mc=c.mc)
        lg = torch.from_numpy(logits).cuda().requires_grad_(True)
        yt = torch.from_numpy(y).cuda()
        kl = torch.tensor(c.kl, device="cuda", requires_grad=True)
        beta = torch.tensor(c.beta, device="cuda") if c.beta_dev else c.beta
        loss, LL = ops.gauss_elbo_cb_autograd(lg, kl, yt, beta, c.train_size, lik, c.mean_over)
        loss.backward(torch.tensor(c.g, device="cuda"))
        got = {"LL": LL, "loss": loss.detach(), "g_logits": lg.grad, "g_kl": kl.grad}
        got.update(ops.gauss_moments_cb(lg.detach(), lik, y=yt)._asdict())
        for f, r in K.ratios({k: v.cpu().numpy() for k, v in got.items()}, ref).items():
            if r > worst.get(f, (-1.0, ""))[0]:
                worst[f] = (r, c.name)
    print(json.dumps({"what": "worst |device - float64| / (U x scale) over %d cases" % len(K.CASES),
                      **{f: {"worst": round(r, 3), "bound": K.bound(f), "case": n} for f, (r, n) in worst.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--errors", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
    import torch
    import layers  # noqa: F401
    from bbb_hip import ensemble, ops, rng, train, zoo
    dev = torch.device("cuda")
    if a.errors:
        return errors(torch, ops, train)
    lik = train.GaussianLikelihood()
    D = 8
    for E, B in ((10, 512), (1, 256)):
        torch.manual_seed(E)
        lg = torch.randn(E, 2 * D, B, device=dev, requires_grad=True)
        y = torch.randn(B, D, device=dev)
        kl = torch.tensor(4321.0, device=dev, requires_grad=True)

        def hip():
            loss, _ = ops.gauss_elbo_cb_autograd(lg, kl, y, 0.1, 50000.0, lik, E)
            torch.autograd.grad(loss, (lg, kl))

        def expr():
            loss, _ = train.gaussian_elbo(lg, y, kl, 0.1, 50000.0, lik, E)
            torch.autograd.grad(loss, (lg, kl))

        report("Gaussian tail forward + backward, logits [%d, %d, %d]" % (E, 2 * D, B),
               windows({"hip": hip, "torch": expr}, a.steps, a.rounds, torch),
               launches={"hip": launches(hip, torch), "torch": launches(expr, torch)})
    for kind, B, E, what in (("bbb", 512, 10, "train_step launch by launch, AlexNet bbb outputs 16, bs 512 num_ens 10"),
                             ("lrt", 256, 1, "train_step self-captured, AlexNet lrt outputs 16, bs 256 num_ens 1")):
        x = torch.rand(B, 3, 32, 32, device=dev)
        y = torch.randn(B, D, device=dev)
        fns = {}
        for name, on in (("hip", True), ("torch", False)):
            torch.manual_seed(0)
            net = zoo.getModel("alexnet", 3, 2 * D, PRIORS, kind, "softplus").to(dev)
            rng.assign_stream_ids(net)
            opt = train.FusedAdam(net.parameters(), lr=1e-5)

            def step(net=net, opt=opt, on=on):
                ensemble.hip_gauss_tail[0] = on          # (read while the step runs or is captured; a replay does not read it)
                try:
                    train.train_step(net, opt, x, y, E, 0.1, 50000.0, likelihood=lik)
                finally:
                    ensemble.hip_gauss_tail[0] = True
            fns[name] = step
        report(what, windows(fns, max(10, a.steps // (1 if E == 1 else 10)), a.rounds, torch))


if __name__ == "__main__":
    main()
