"""The Gaussian-likelihood tail on the device (csrc/gauss_tail.hip through ops.gauss_elbo_cb_autograd and ops.gauss_moments_cb) against
the float64 contract of tests/gauss_tail_contract.py, case by case; the refusals of the three entries before any launch; the smallest
regression model on the training fast path end to end (forward_loss and train_step with likelihood=..., HIP tail against the torch
expression train.gaussian_elbo, launch by launch against the captured step, fp32 and bf16 storage); and uncertainty.mc_regression.
Run with -m gpu.

Measured on an MI355X, worst |device - float64| / (U x scale) over the cases, next to its bound: see profiles/gauss_tail_notes.md."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import gauss_tail_contract as K
import ref_port_torch as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import _lib, ensemble, fast_train, ops, rng, train, uncertainty
    return dict(lib=_lib, ens=ensemble, ft=fast_train, ops=ops, rng=rng, train=train, unc=uncertainty)


@pytest.fixture(scope="module")
def refs():
    """{case name: (logits, y, float64 reference)}, computed once and left unchanged."""
    out = {}
    for c in K.CASES:
        logits, y = K.inputs(c)
        out[c.name] = (logits, y, K.reference(c, logits, y))
    return out


def _lik(env, c):
    return env["train"].GaussianLikelihood(noise_sigma=c.noise_sigma, log_var_min=c.log_var_min, log_var_max=c.log_var_max, mc=c.mc)


def _device_run(env, c, logits, y):
    """Every output of the three entries for one case, as numpy."""
    ops = env["ops"]
    lg = torch.from_numpy(logits).to(DEV).requires_grad_(True)
    yt = torch.from_numpy(y).to(DEV)
    kl = torch.tensor(c.kl, device=DEV, requires_grad=True)
    beta = torch.tensor(c.beta, device=DEV) if c.beta_dev else c.beta
    lik = _lik(env, c)
    loss, LL = ops.gauss_elbo_cb_autograd(lg, kl, yt, beta, c.train_size, lik, c.mean_over)
    assert loss.requires_grad and not LL.requires_grad
    loss.backward(torch.tensor(c.g, device=DEV))
    mom = ops.gauss_moments_cb(lg.detach(), lik, y=yt)
    out = {"LL": LL, "loss": loss.detach(), "g_logits": lg.grad, "g_kl": kl.grad}
    out.update(mom._asdict())
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("c", K.CASES, ids=lambda c: c.name)
def test_case_against_float64(env, refs, c):
    logits, y, ref = refs[c.name]
    got = _device_run(env, c, logits, y)
    r = K.ratios(got, ref)                           # (also: NaN pattern, and exact values where the scale is 0 -- a clamped s)
    print(c.name, {f: round(v, 3) for f, v in r.items()})
    assert set(r) == set(K.FIELDS)
    for f, v in r.items():
        assert v <= K.bound(f), (f, v, K.bound(f))
    if c.noise_sigma is None:
        s = logits[:, c.D:]
        assert not got["g_logits"][:, c.D:][(s < c.log_var_min) | (s > c.log_var_max)].any()
    dead = (ref["L"] - ref["L"].max(axis=0) < -1e4) if c.mc == "logmeanexp" else np.zeros((c.E, c.B), bool)
    assert not got["g_logits"].transpose(0, 2, 1)[dead].any()                  # weight exactly 0
    if c.recipe == "far_draw" and c.mc == "logmeanexp" and c.noise_sigma is None:
        assert dead[-1].all()
    again = _device_run(env, c, logits, y)
    for f in K.FIELDS:
        assert np.array_equal(got[f], again[f], equal_nan=True), f


def test_a_nan_stays_inside_its_image(env, refs):
    c = next(c for c in K.CASES if c.noise_sigma is None and c.mc == "logmeanexp" and c.B >= 63 and c.E > 1)
    logits, y, _ = refs[c.name]
    clean = _device_run(env, c, logits, y)
    logits, y = logits.copy(), y.copy()
    logits[1, 0, 5] = np.nan
    y[7, c.D - 1] = np.nan
    ref = K.reference(c, logits, y)
    got = _device_run(env, c, logits, y)
    hit = np.zeros(c.B, bool)
    hit[[5, 7]] = True
    assert (np.isnan(got["LL"]) == hit).all() and np.isnan(got["loss"]) and (np.isnan(got["log_density"]) == hit).all()
    assert (np.isnan(got["g_logits"]).any(axis=(0, 1)) == hit).all()
    assert np.array_equal(got["g_logits"][:, :, ~hit], clean["g_logits"][:, :, ~hit])          # the other images: what they were
    assert np.array_equal(got["LL"][~hit], clean["LL"][~hit])
    for f, v in K.ratios(got, ref).items():
        assert v <= K.bound(f), (f, v)


def test_entries_return_the_plan_codes_without_launching(env):
    h = env["lib"].lib()
    E, D, B = 2, 3, 4
    lg = torch.randn(E, 2 * D, B, device=DEV)
    y = torch.randn(B, D, device=DEV)
    kl, g = torch.tensor(3.0, device=DEV), torch.tensor(1.0, device=DEV)
    outs = [torch.full((B,), 7.0, device=DEV), torch.full((), 7.0, device=DEV), torch.full((E, 2 * D, B), 7.0, device=DEV),
            torch.full((), 7.0, device=DEV)] + [torch.full((B, D), 7.0, device=DEV) for _ in range(4)] + [torch.full((B,), 7.0, device=DEV)]
    ll, loss, gl, gkl = outs[:4]
    mom = outs[4:]
    p = lambda t: t.data_ptr()

    def fwd(E=E, B=B, C=2 * D, D=D, sigma=0.0, lo=-20.0, hi=20.0, mc=0, mo=0, logits=p(lg)):
        return h.bbb_gauss_elbo_cb_fwd(logits, p(y), p(kl), 0.1, None, 100.0, E, B, C, D, sigma, lo, hi, mc, mo, p(ll), p(loss), None)

    def bwd(E=E, B=B, C=2 * D, D=D, sigma=0.0, lo=-20.0, hi=20.0, mc=0, mo=0, logits=p(lg)):
        return h.bbb_gauss_elbo_cb_bwd(logits, p(y), p(g), 0.1, None, 100.0, E, B, C, D, sigma, lo, hi, mc, mo, p(gl), p(gkl), None)

    def moments(E=E, B=B, C=2 * D, D=D, sigma=0.0, lo=-20.0, hi=20.0, logits=p(lg), yy=p(y), **_):
        return h.bbb_gauss_moments_cb(logits, yy, E, B, C, D, sigma, lo, hi, *[p(t) for t in mom], None)

    for f in (fwd, bwd, moments):
        for want, kw in ((K.EINVAL, dict(E=0)), (K.EINVAL, dict(C=5)), (K.EINVAL, dict(lo=1.0, hi=0.0)), (K.EINVAL, dict(logits=None)),
                         (K.EINVAL, dict(C=D, sigma=-1.0)), (K.EINVAL, dict(C=D, sigma=float("nan"))), (K.EALIGN, dict(logits=p(lg) + 2)),
                         (K.ESHAPE, dict(E=513)), (K.ESHAPE, dict(B=2 ** 31 - 1)), (K.ESHAPE, dict(C=2050, D=1025))):
            assert f(**kw) == want, (f.__name__, kw)
    assert fwd(mc=2) == K.EINVAL and bwd(mo=-1) == K.EINVAL and moments(yy=None) == K.EINVAL
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())                 # nothing was launched
    with pytest.raises(env["lib"].BBBHipError, match="gauss_elbo_cb_ok"):
        env["ops"].gauss_elbo_cb_autograd(lg, kl, y[:, :2].contiguous(), 0.1, 100.0, env["train"].GaussianLikelihood())
    with pytest.raises(env["lib"].BBBHipError, match="log_density needs y"):
        env["ops"].gauss_moments_cb(lg, env["train"].GaussianLikelihood(), want=("log_density",))


# ---- end to end: the smallest model on the training fast path ----
D_OUT, BATCH = 3, 8


def _net(layer_type, seed=5):
    from layers import BBB_Conv2d, BBB_Linear, BBB_LRT_Conv2d, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    conv, lin = (BBB_Conv2d, BBB_Linear) if layer_type == "bbb" else (BBB_LRT_Conv2d, BBB_LRT_Linear)
    torch.manual_seed(seed)
    net = ModuleWrapper()
    net.add_module("c1", conv(3, 8, 3, padding=1, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("a1", nn.ReLU())
    net.add_module("p1", nn.MaxPool2d(2, 2))
    net.add_module("fl", FlattenLayer(8 * 4 * 4))
    net.add_module("f1", lin(8 * 4 * 4, 2 * D_OUT, bias=True, priors=P.CONFIG_PRIORS))
    return net.to(DEV)


def _batch():
    g = torch.Generator().manual_seed(21)
    return torch.rand(BATCH, 3, 8, 8, generator=g).to(DEV), torch.randn(BATCH, D_OUT, generator=g).to(DEV)


def _param_scales(env, net, x, y, num_ens, lik, precision, train_size, beta):
    """Per parameter tensor, sum |terms| of its gradient sum: sum_k |d logit_k / d theta| x S_g[k] -- the Jacobian of the logits row by
    row through the node's own backward, S_g the contract's scale of d loss / d logit_k from the float64 reference on the node's fp32
    logits (the error either tail may make in that cotangent, and what the backward's own rounding scales with) -- plus the KL term."""
    rng, ens = env["rng"], env["ens"]
    params = [p for p in net.parameters() if p.requires_grad]
    seed, call0 = rng.next_calls(0)
    if precision == "bf16":
        logits, kl = env["ft"].mc_logits_autograd(net, x, num_ens, seed, call0, precision="bf16")
    else:
        logits, kl = ens.mc_logits_cb_autograd(net, x, num_ens, seed, call0)
    E, C, B = logits.shape
    c = K.Case("e2e", "unit", E, C // 2, B, None, lik.log_var_min, lik.log_var_max, lik.mc, num_ens, beta, False, float(kl.detach()), train_size, 1.0)
    ref = K.reference(c, logits.detach().cpu().numpy(), y.cpu().numpy())
    S = torch.from_numpy(ref["scale"]["g_logits"]).to(DEV)
    scales = [torch.zeros_like(p, dtype=torch.float64) for p in params]
    flat = logits.reshape(-1)
    for k in range(flat.numel()):
        rows = torch.autograd.grad(flat[k], params, retain_graph=True, allow_unused=True)
        for acc, r in zip(scales, rows):
            if r is not None:
                acc += r.double().abs() * S.reshape(-1)[k]
    gkl = torch.autograd.grad(kl, params, allow_unused=True)
    for acc, r in zip(scales, gkl):
        if r is not None:
            acc += r.double().abs() * abs(beta)
    return scales, ref


def _one_forward_backward(env, net, x, y, num_ens, lik, precision, hip, train_size=1000.0, beta=0.1):
    env["rng"].manual_seed(4242, call=0)
    env["ens"].hip_gauss_tail[0] = hip
    try:
        net.zero_grad(set_to_none=True)
        loss, LL, kl = env["train"].forward_loss(net, x, y, num_ens, beta, train_size, precision=precision, likelihood=lik)
        loss.reshape(()).backward()
    finally:
        env["ens"].hip_gauss_tail[0] = True
    return loss.detach().reshape(()), LL.detach(), kl.detach(), [p.grad.clone() for p in net.parameters() if p.requires_grad]


@pytest.mark.parametrize("layer_type,num_ens,precision", [("bbb", 1, "fp32"), ("bbb", 4, "fp32"), ("lrt", 1, "fp32"), ("lrt", 4, "fp32"),
                                                          ("bbb", 4, "bf16")])
def test_forward_loss_hip_tail_against_the_torch_tail(env, layer_type, num_ens, precision):
    net = _net(layer_type)
    env["rng"].assign_stream_ids(net)
    x, y = _batch()
    lik = env["train"].GaussianLikelihood()
    train_size, beta = 1000.0, 0.1
    assert env["ft"].train_path_ok(net, x) is not None
    seen = []
    real = env["ops"].gauss_elbo_cb_autograd
    env["ops"].gauss_elbo_cb_autograd = lambda *a, **k: (seen.append(1), real(*a, **k))[1]
    try:
        a = _one_forward_backward(env, net, x, y, num_ens, lik, precision, True, train_size, beta)
        assert seen == [1] and env["ens"].stats["path"] == ("chwn-autograd" if precision == "fp32" else "chwn-autograd-bf16")
        b = _one_forward_backward(env, net, x, y, num_ens, lik, precision, False, train_size, beta)
        assert seen == [1]                                                 # the switch forces the torch expression
    finally:
        env["ops"].gauss_elbo_cb_autograd = real
    assert a[1].shape == (BATCH,) and torch.equal(a[2], b[2])
    env["rng"].manual_seed(4242, call=0)
    scales, ref = _param_scales(env, net, x, y, num_ens, lik, precision, train_size, beta)
    tol_loss = 2 * K.bound("loss") * K.U * float(ref["scale"]["loss"])      # each side within the bound of the float64 value
    print("loss", a[0].item(), b[0].item(), "tol", tol_loss)
    assert abs(a[0].item() - float(ref["loss"])) <= tol_loss / 2 and abs(a[0].item() - b[0].item()) <= tol_loss
    assert (np.abs(a[1].cpu().numpy() - ref["LL"]) <= K.bound("LL") * K.U * ref["scale"]["LL"]).all()
    for (name, _), ga, gb, sc in zip([(n, p) for n, p in net.named_parameters() if p.requires_grad], a[3], b[3], scales):
        ratio = ((ga.double() - gb.double()).abs() / (K.U * sc).clamp_min(1e-300)).max().item()
        print(name, "max |hip - torch| / (U sum|terms|) =", round(ratio, 4))
        assert ratio <= 4.0, (name, ratio)


@pytest.mark.parametrize("layer_type", ["bbb", "lrt"])
def test_train_step_launch_by_launch_against_the_captured_step(env, layer_type):
    T = env["train"]
    x, y = _batch()
    lik = T.GaussianLikelihood()
    saved = dict(T.auto_graph)

    def run(graph):
        net = _net(layer_type)
        env["rng"].assign_stream_ids(net)
        env["rng"].manual_seed(99, call=0)
        opt = T.FusedAdam(net.parameters(), lr=1e-2, capturable=True)
        T.auto_graph["after"] = 0 if graph else saved["after"]           # capture at the first call
        try:
            out = [T.train_step(net, opt, x, y, 4, 0.1, 1000.0, graph=graph, likelihood=lik) for _ in range(3)]
        finally:
            T.auto_graph.update(saved)
        st = T._auto.get(net)
        return net, out, st

    net_e, eager, st_e = run(False)
    net_g, graphed, st_g = run(True)
    assert st_e is None and st_g is not None and st_g["graphed"] is not None and st_g["graphed"].replays == 2
    assert st_g["key"][-1] == "fp32" and lik.key() in st_g["key"]
    for (le, lle, kle), (lg_, llg, klg) in zip(eager, graphed):
        print("loss", le.item(), lg_.item())
        assert lle.shape == (BATCH,) and torch.equal(le.reshape(()), lg_.reshape(())) and torch.equal(lle, llg) and torch.equal(kle, klg)
    for (n, a), (_, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(a, b), n


def test_auto_key_tells_the_likelihoods_apart_and_ends_in_precision(env):
    T = env["train"]
    net = _net("bbb")
    opt = T.FusedAdam(net.parameters(), lr=1e-3)
    x, y = _batch()
    target = torch.zeros(BATCH, dtype=torch.int64, device=DEV)
    k0 = T._auto_key(net, opt, x, target, 2, 100.0, "fp32")
    k1 = T._auto_key(net, opt, x, y, 2, 100.0, "fp32", T.GaussianLikelihood())
    k2 = T._auto_key(net, opt, x, y, 2, 100.0, "fp32", T.GaussianLikelihood(mc="mean"))
    k3 = T._auto_key(net, opt, x, y, 2, 100.0, "bf16", T.GaussianLikelihood(noise_sigma=0.5))
    assert k0 is not None and len({k0, k1, k2, k3}) == 4 and len(k0) == len(k1)
    assert k0[-1] == k1[-1] == k2[-1] == "fp32" and k3[-1] == "bf16" and k0[-2] is None and k1[-2] == T.GaussianLikelihood().key()
    with pytest.raises(env["lib"].BBBHipError, match="group= sharding"):
        env["ens"]._local_lse(net, x, 2, 1, 0, 2, units=(2, 0, 2), elbo=[y, 0.1, 100.0, None, T.GaussianLikelihood()])


def test_forward_loss_without_autograd_and_off_the_fast_path(env):
    """Autograd off: the batch-innermost inference path, then the same tail.  B % 4 != 0: the reference-layout path, transposed once."""
    T = env["train"]
    net = _net("bbb")
    env["rng"].assign_stream_ids(net)
    x, y = _batch()
    lik = T.GaussianLikelihood(mc="mean")
    env["rng"].manual_seed(7, call=0)
    with torch.no_grad():
        loss0, LL0, kl0 = T.forward_loss(net, x, y, 3, 0.1, 500.0, likelihood=lik)
    env["rng"].manual_seed(7, call=0)
    loss1, LL1, kl1 = T.forward_loss(net, x, y, 3, 0.1, 500.0, likelihood=lik)
    assert not loss0.requires_grad and loss1.requires_grad and LL0.shape == LL1.shape == (BATCH,)
    np.testing.assert_allclose(LL0.cpu().numpy(), LL1.detach().cpu().numpy(), rtol=2e-4, atol=2e-4)
    env["rng"].manual_seed(7, call=0)
    loss2, LL2, _ = T.forward_loss(net, x[:6], y[:6], 3, 0.1, 500.0, likelihood=lik)
    assert env["ft"].train_path_ok(net, x[:6]) is None and loss2.requires_grad and LL2.shape == (6,)
    loss2.reshape(()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    np.testing.assert_allclose(LL2.detach().cpu().numpy(), LL1.detach().cpu().numpy()[:6], rtol=2e-4, atol=2e-4)


def test_mc_regression_is_the_moments_of_the_same_noise_calls(env):
    net = _net("bbb")
    env["rng"].assign_stream_ids(net)
    x, y = _batch()
    lik = env["train"].GaussianLikelihood()
    T_ = 5
    env["rng"].manual_seed(31, call=10)
    got = env["unc"].mc_regression(net, x, T=T_, likelihood=lik, y=y)
    assert env["rng"].get_state() == (31, 10 + T_)
    env["rng"].manual_seed(31, call=10)
    with torch.no_grad():
        seed, call0 = env["rng"].next_calls(T_)
        logits_cb, _ = env["ens"].mc_logits_cb(net, x, T_, seed, call0)
        want = env["ops"].gauss_moments_cb(logits_cb, lik, y=y)
        part = env["ops"].gauss_moments_cb(logits_cb, lik, want=("total", "mean"))
    assert tuple(logits_cb.shape) == (T_, 2 * D_OUT, BATCH)
    for f in K.MOMENTS:
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    assert torch.equal(part.total, want.total) and torch.equal(part.mean, want.mean) and part.epistemic is None and part.log_density is None
    no_y = env["unc"].mc_regression(net, x, T=T_, likelihood=lik)
    assert no_y.log_density is None and no_y.mean.shape == (BATCH, D_OUT) and env["rng"].get_state() == (31, 10 + 2 * T_)
