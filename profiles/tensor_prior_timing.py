"""Device time of the parameter pass with per-weight Gaussian priors (bbb_reparam_kl_tp_fwd / _tp_bwd) against the scalar entries on the
same tensors, and of whole training steps with tensor priors (profiles/tensor_prior_notes.md).  One process; every launch variant is
captured as a hipGraph of 20 launches (hot, as bench.py measures the pass), the variants take turns window by window, device events
around each window; per variant the windows' median and range.  The scalar launch is captured TWICE ("scalar", "scalar_again"): the
difference between the two is the spread a difference between variants has to exceed.
    python profiles/tensor_prior_timing.py            AlexNet-10's 12 tensors: forward E = 1 and E = 10, KL-only with sigma^2 out,
                                                      backward E = 1; then train_step on LRT AlexNet, bs 256, num_ens 1: captured with
                                                      scalar and with tensor priors, and launch by launch with scalar priors against
                                                      the same step with the tensor KL added as torch expressions
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}
LAUNCHES = 20


def windows(fns, steps, rounds, torch):
    out = {k: [] for k in fns}
    for f in fns.values():
        for _ in range(5):
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


def report(what, res, per=1, **extra):
    line = {"what": what}
    for k, v in res.items():
        line[k] = {"median_us": round(1e3 * statistics.median(v) / per, 3), "min_us": round(1e3 * min(v) / per, 3),
                   "max_us": round(1e3 * max(v) / per, 3)}
    line.update(extra)
    print(json.dumps(line), flush=True)


def graph_of(fn, torch):
    """fn() x LAUNCHES in one hipGraph -> replay callable (outputs stay alive in the graph's pool)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            keep.append(fn())
    g._keep = keep
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    import torch
    import layers  # noqa: F401
    from bbb_hip import ensemble, ops, priors, rng, train, zoo

    torch.manual_seed(0)
    net = zoo.getModel("alexnet", 3, 10, PRIORS, "bbb", "softplus").cuda()
    rng.assign_stream_ids(net)
    mus, rhos, ids = [], [], []
    for l in ensemble.bayesian_layers(net):
        m, r, i = l._param_lists()
        mus += [t.detach() for t in m]
        rhos += [t.detach() for t in r]
        ids += i
    n_el = sum(m.numel() for m in mus)
    pri = [(0.1 * torch.randn_like(m), torch.exp(torch.empty_like(m).uniform_(-3.0, 0.0))) for m in mus]
    print(json.dumps({"what": "tensors", "count": len(mus), "elements": n_el}), flush=True)

    def fwd(E, p, **kw):
        return lambda: ops.reparam_kl_forward(mus, rhos, 0.0, 0.1, ids, 7, 3, draws=E, priors=p, **kw)

    for E in (1, 10):
        fns = {"scalar": graph_of(fwd(E, None), torch), "tensor": graph_of(fwd(E, pri), torch), "scalar_again": graph_of(fwd(E, None), torch)}
        report("forward E=%d" % E, windows(fns, a.steps, a.rounds, torch), per=LAUNCHES, byte_ratio=round((16 + 4 * E) / (8 + 4 * E), 3),
               bytes_scalar=(8 + 4 * E) * n_el, bytes_tensor=(16 + 4 * E) * n_el)
    kw = dict(sample=False, want_sigma=True, sigma_squared=True)
    fns = {"scalar": graph_of(fwd(1, None, **kw), torch), "tensor": graph_of(fwd(1, pri, **kw), torch),
           "scalar_again": graph_of(fwd(1, None, **kw), torch)}
    report("KL only, sigma^2 out", windows(fns, a.steps, a.rounds, torch), per=LAUNCHES, byte_ratio=round(20 / 12, 3))
    gws = [torch.randn((1,) + tuple(m.shape), device="cuda") for m in mus]
    gkl = torch.tensor(0.5, device="cuda")
    bwd = lambda p: (lambda: ops.reparam_kl_backward(mus, rhos, gws, gkl, 0.0, 0.1, ids, 7, 3, 1, priors=p))
    fns = {"scalar": graph_of(bwd(None), torch), "tensor": graph_of(bwd(pri), torch), "scalar_again": graph_of(bwd(None), torch)}
    report("backward E=1", windows(fns, a.steps, a.rounds, torch), per=LAUNCHES, byte_ratio=round(28 / 20, 3))
    if a.skip_train:
        return

    # ---- whole steps: LRT AlexNet, bs 256, num_ens 1 (the reference's default configuration)
    x = torch.rand(256, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (256,), device="cuda")

    def model(tensor):
        torch.manual_seed(1)
        m = zoo.getModel("alexnet", 3, 10, PRIORS, "lrt", "softplus").cuda()
        rng.assign_stream_ids(m)
        if tensor:
            torch.manual_seed(2)
            priors.from_posterior(m, zoo.getModel("alexnet", 3, 10, PRIORS, "lrt", "softplus").cuda())
        return m, train.FusedAdam(m.parameters(), lr=1e-4)

    steps = {}
    for name, tensor in (("captured_scalar", False), ("captured_tensor", True), ("captured_scalar_again", False)):
        m, opt = model(tensor)
        steps[name] = (lambda m=m, opt=opt: train.train_step(m, opt, x, y, 1, 0.1, 50000.0))
    for f in steps.values():
        for _ in range(6):
            f()
    report("train_step LRT AlexNet bs256 E1, self-captured", windows(steps, a.steps, a.rounds, torch))

    m_s, opt_s = model(False)
    m_t, opt_t = model(False)
    other = model(False)[0]
    tp = [(l.W_mu.detach().clone(), torch.nn.functional.softplus(l.W_rho.detach()), l.bias_mu.detach().clone(),
           torch.nn.functional.softplus(l.bias_rho.detach())) for l in ensemble.bayesian_layers(other)]

    def torch_kl(m):
        kl = 0.0
        for l, (wm, ws, bm, bs) in zip(ensemble.bayesian_layers(m), tp):
            for mu, rho, m0, s0 in ((l.W_mu, l.W_rho, wm, ws), (l.bias_mu, l.bias_rho, bm, bs)):
                sg = torch.nn.functional.softplus(rho)
                kl = kl + 0.5 * (2 * torch.log(sg / s0) - 1 + (s0 / sg) ** 2 + ((mu - m0) / sg) ** 2).sum()
        return kl

    def eager_torch_kl():
        opt_t.zero_grad()
        loss, _, _ = train.forward_loss(m_t, x, y, 1, 0.0, 50000.0)      # the scalar KL weighted out, the tensor KL as torch expressions
        (loss + 0.1 * torch_kl(m_t)).backward()
        opt_t.step()

    m_e, opt_e = model(True)
    eager = {"eager_scalar": lambda: train.train_step(m_s, opt_s, x, y, 1, 0.1, 50000.0, graph=False),
             "eager_tensor": lambda: train.train_step(m_e, opt_e, x, y, 1, 0.1, 50000.0, graph=False),
             "eager_scalar_plus_torch_kl": eager_torch_kl}
    report("train_step LRT AlexNet bs256 E1, launch by launch", windows(eager, a.steps, a.rounds, torch))


if __name__ == "__main__":
    main()
