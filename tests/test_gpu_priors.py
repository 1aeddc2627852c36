"""Per-weight Gaussian priors end to end on the smallest model (conv 3->8 k3 p1 on 8x8, ReLU, MaxPool2d(2,2), flatten, linear 128->12,
Softplus, linear 12->10; B = 8; BBB and LRT): the drop-in layers, the batched and the hooked forward, cached inference graphs, the
fast training node's gradients, captured training steps across an in-place prior update and a change of kind, bf16 storage, MOPED
and the posterior of one task as the prior of the next.  KL against float64 in the bound of tests/prior_contract.py.  -m gpu."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import prior_contract as P

pytestmark = pytest.mark.gpu
B = 8


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import ops, rng, ensemble, train, fast_train, priors, _lib
    return dict(ops=ops, rng=rng, ens=ensemble, train=train, ft=fast_train, priors=priors, lib=_lib)


def _net(lt, seed=3):
    import layers
    from layers.misc import ModuleWrapper, FlattenLayer
    conv, lin = (layers.BBB_Conv2d, layers.BBB_Linear) if lt == "bbb" else (layers.BBB_LRT_Conv2d, layers.BBB_LRT_Linear)

    class Net(ModuleWrapper):
        def __init__(self):
            super().__init__()
            self.conv1 = conv(3, 8, 3, padding=1)
            self.act1 = nn.ReLU()
            self.pool1 = nn.MaxPool2d(2, 2)
            self.flatten = FlattenLayer(128)
            self.fc1 = lin(128, 12)
            self.act2 = nn.Softplus()
            self.fc2 = lin(12, 10)
    torch.manual_seed(seed)
    from bbb_hip import rng
    net = Net().cuda()
    rng.assign_stream_ids(net)
    return net


def _random_priors(net, seed=5):
    """Different tensor priors per layer, equal scalar fallbacks: conv1 both tensors on weight and bias, fc1 a tensor mean only (MOPED's
    form), fc2 a tensor sigma on the weight and a tensor mean on the bias."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda p: 0.1 * torch.randn(p.shape, device="cuda", generator=g)
    s = lambda p: torch.exp(torch.empty(p.shape, device="cuda").uniform_(-3.0, 0.0, generator=g))
    net.conv1.set_prior(mu=r(net.conv1.W_mu), sigma=s(net.conv1.W_mu), bias_mu=r(net.conv1.bias_mu), bias_sigma=s(net.conv1.bias_mu))
    net.fc1.set_prior(mu=r(net.fc1.W_mu))
    net.fc2.set_prior(sigma=s(net.fc2.W_mu), bias_mu=r(net.fc2.bias_mu))
    return net


def _kl64(env, net, layers=None):
    """Float64 (KL, M) of the model's current posterior against its current priors, by the contract's reference."""
    inputs, eff = [], []
    for l in (env["ens"].bayesian_layers(net) if layers is None else layers):
        mus, rhos, _ = l._param_lists()
        pri = l._prior_lists() or [(None, None)] * len(mus)
        for m, r, (pm, ps) in zip(mus, rhos, pri):
            n = m.numel()
            inputs.append((m.detach().cpu().numpy().reshape(-1), r.detach().cpu().numpy().reshape(-1)))
            eff.append((pm.cpu().numpy().reshape(-1) if pm is not None else np.full(n, l.prior_mu, np.float32),
                        ps.cpu().numpy().reshape(-1) if ps is not None else np.full(n, l.prior_sigma, np.float32)))
    return P.kl_reference_tp(inputs, eff, 0)


def _check_kl(env, net, kl, c=None):
    ref = _kl64(env, net)
    return P.check_kl_tp(float(kl), ref, max(P.FWD_C.values()) if c is None else c)


def _x(seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(B, 3, 8, 8, device="cuda", generator=g), torch.randint(0, 10, (B,), device="cuda", generator=g)


@pytest.mark.parametrize("lt", ["bbb", "lrt"])
def test_drop_in_layers_and_equality_across_paths(env, lt):
    net = _random_priors(_net(lt))
    x, _ = _x()
    # a layer on its own, with and without a forward before kl_loss()
    l = net.conv1
    with torch.no_grad():
        k0 = l.kl_loss()
        l(x)
        k1 = l.kl_loss()
    assert torch.equal(k0, k1)
    P.check_kl_tp(k0.item(), _kl64(env, net, [l]), max(P.FWD_C.values()))
    with torch.no_grad():
        out, kl = net(x)
        assert out.shape == (B, 10) and bool(torch.isfinite(out).all())
        _check_kl(env, net, kl.item())
        env["rng"].manual_seed(9, call=0)
        lo, kl_b = env["ens"].mc_forward(net, x, 3)
        kl_h = 0.0
        h = net.fc1.register_forward_hook(lambda *a: None)               # the hooked loop
        try:
            for _ in range(3):
                kl_h = kl_h + net(x)[1]
        finally:
            h.remove()
    assert float(kl_b) == float(kl_h), (float(kl_b), float(kl_h))
    P.check_kl_tp(float(kl_b) / 3, _kl64(env, net), max(P.FWD_C.values()))
    # a repeated shape is served from the cached graph; an in-place update of the priors is seen by its next replay
    other = _net(lt, seed=4)
    with torch.no_grad():
        env["priors"].from_posterior(net)                                # fc1 / fc2 get new tensors: a change of kind
        for _ in range(5):
            _, kl_c = net(x)
        assert abs(float(kl_c)) <= max(P.FWD_C.values()) * 2.0 ** -23 * _kl64(env, net)[1] + abs(_kl64(env, net)[0])
        ptr = net.fc2.W_prior_sigma.data_ptr()
        env["priors"].from_posterior(net, other)                         # every buffer exists: in place, behind the cached graph
        assert net.fc2.W_prior_sigma.data_ptr() == ptr
        _, kl_after = net(x)
        env["ens"].invalidate(net)                                       # a fresh eager one
        _, kl_fresh = net(x)
    assert float(kl_after) == float(kl_fresh)
    ref = _kl64(env, net)
    P.check_kl_tp(float(kl_after), ref, max(P.FWD_C.values()))
    assert ref[0] > 1e-3 * ref[1]                                        # (far from the stale priors' KL of zero)
    with torch.no_grad():                                                # a direct write into a prior buffer is seen as well
        net.fc2.W_prior_mu.add_(0.05)
        _, kl_w = net(x)
    ref_w = _kl64(env, net)
    P.check_kl_tp(float(kl_w), ref_w, max(P.FWD_C.values()))
    assert ref_w[0] - ref[0] > 100 * max(P.FWD_C.values()) * 2.0 ** -23 * ref[1]


@pytest.mark.parametrize("lt", ["bbb", "lrt"])
def test_gradients_of_the_fast_node(env, lt):
    """train.forward_loss on the fast node against the module-by-module path on the same noise, in the bounds tests/test_gpu_fast_train.py
    uses for scalar priors; beta and train_size are such that the KL part is at least a tenth of every parameter gradient's scale
    (asserted on float64), so a dropped prior tensor cannot hide under the bound."""
    ens, T = env["ens"], env["train"]
    net = _random_priors(_net(lt))
    x, y = _x()
    assert env["ft"].train_path_ok(net, x) == lt
    E, beta, n = 3, 1.0, 8.0
    grads = {}
    for fast in (True, False):
        ens.fast_autograd = fast
        try:
            net.zero_grad(set_to_none=True)
            env["rng"].manual_seed(5, call=7)
            loss, lo, kl = T.forward_loss(net, x, y, E, beta, n)
            assert ens.stats["path"] == ("chwn-autograd" if fast else "nchw")
            loss.backward()
            grads[fast] = ({k: p.grad.detach().clone() for k, p in net.named_parameters()}, float(kl))
        finally:
            ens.fast_autograd = True
    (ga, kla), (gb, klb) = grads[True], grads[False]
    _check_kl(env, net, kla)
    _check_kl(env, net, klb)
    # float64 KL gradient of every parameter (torch autograd on the closed form), weighted as the loss weights it
    kl_share = {}
    for name, l in env["priors"].named_layers(net):
        pri = l._prior_lists()
        for (pn, mu, rho), (pm, ps) in zip((("W", l.W_mu, l.W_rho), ("bias", l.bias_mu, l.bias_rho)), pri):
            m = mu.detach().double().requires_grad_(True)
            r = rho.detach().double().requires_grad_(True)
            m0 = pm.double() if pm is not None else torch.full_like(m, float(l.prior_mu))
            s0 = ps.double() if ps is not None else torch.full_like(m, float(l.prior_sigma))
            sg = F.softplus(r)
            (0.5 * (2 * torch.log(sg / s0) - 1 + (s0 / sg) ** 2 + ((m - m0) / sg) ** 2)).sum().backward()
            kl_share["%s.%s_mu" % (name, pn)] = m.grad
            kl_share["%s.%s_rho" % (name, pn)] = r.grad
    w = beta                                                             # d loss / d kl of train.elbo
    for k in ga:
        scale = float(gb[k].abs().max()) + 1e-12
        assert float((w * kl_share[k]).abs().max()) >= 0.1 * scale, (k, float((w * kl_share[k]).abs().max()), scale)
        err = float((ga[k] - gb[k]).abs().max()) / scale
        assert err <= 2e-3, (k, err)


@pytest.mark.parametrize("lt", ["bbb", "lrt"])
def test_captured_steps_follow_the_priors(env, lt):
    """graph=False against graph=True, bit for bit: loss and kl of every step and the parameters behind it, for five steps (the fourth
    call captures, the fifth replays), then for the step after priors.from_posterior in place -- the captured step is KEPT and sees the
    new values at its replay -- and for the step after set_prior(sigma=0.2), a change of kind, which drops it."""
    T, pri = env["train"], env["priors"]
    x, y = _x()
    E, beta, n = 2, 0.1, 1000.0

    def run(graph):
        net = _random_priors(_net(lt, seed=11))
        pri.from_posterior(net)                                          # every buffer exists from here on
        _random_priors(net)
        env["rng"].manual_seed(77, call=0)
        # (capturable in both runs, as a captured step needs it: train_step would switch the optimizer of the graph=True run over at
        # its capture, and the launch-by-launch step behind the dropped graph would then take Adam's step scalars from the device where
        # the graph=False run computes them on the host -- measured: same loss and kl bits, parameters one ulp, 1.5e-8, apart)
        opt = T.FusedAdam(net.parameters(), lr=1e-3, capturable=True)
        out, snaps = [], []

        def step():
            loss, _, kl = T.train_step(net, opt, x, y, E, beta, n, graph=graph)
            out.append((loss.detach().view(torch.int32).item(), kl.detach().view(torch.int32).item(), float(loss), float(kl)))
            snaps.append({k: p.detach().clone() for k, p in net.named_parameters()})
        for _ in range(5):                                               # (the capture happens at call auto_graph["after"] + 1 = 4)
            step()
        g0 = T._auto[net]["graphed"] if graph else None
        assert (g0 is not None) == bool(graph)
        pri.from_posterior(net)                                          # in place: pointers stable
        step()
        if graph:
            assert T._auto[net]["graphed"] is g0, "an in-place prior update dropped the captured step"
        for l in env["ens"].bayesian_layers(net):
            l.set_prior(sigma=0.2)                                       # tensor -> number
        step()
        if graph:
            assert T._auto[net]["graphed"] is not g0
        return out, snaps

    eager, snaps_e = run(False)
    graphed, snaps_g = run(True)
    for i, (a, b) in enumerate(zip(eager, graphed)):
        worst = max(float((snaps_e[i][k] - snaps_g[i][k]).abs().max()) for k in snaps_e[i])
        print("PRIORS captured-vs-eager %s step %d: loss %r / %r, kl %r / %r, worst |parameter difference| %.3g" % (
            lt, i, a[2], b[2], a[3], b[3], worst))
    for i in range(5):
        assert eager[i][:2] == graphed[i][:2], ("step %d" % i, eager[i], graphed[i])
        assert all(torch.equal(snaps_e[i][k], snaps_g[i][k]) for k in snaps_e[i]), "parameters after step %d" % i
    assert eager[5][:2] == graphed[5][:2], ("the step after from_posterior", eager[5], graphed[5])
    assert all(torch.equal(snaps_e[5][k], snaps_g[5][k]) for k in snaps_e[5]), "parameters after the step behind from_posterior"
    assert eager[6][:2] == graphed[6][:2], ("the step after set_prior(sigma=0.2)", eager[6], graphed[6])
    assert all(torch.equal(snaps_e[6][k], snaps_g[6][k]) for k in snaps_e[6]), "parameters after the step behind the change of kind"
    assert abs(eager[5][3]) < 0.05 * eager[4][3]                         # the KL right after from_posterior: one Adam step away from zero


@pytest.mark.parametrize("lt", ["bbb", "lrt"])
def test_tensor_priors_keep_the_fast_path_and_one_launch(env, lt, monkeypatch):
    """Layers with DIFFERENT tensor priors and equal scalar fallbacks: still the fast training path, still ONE parameter-pass launch
    forward and one backward, through the tensor-prior entries; different scalar fallbacks are refused as before."""
    net = _random_priors(_net(lt))
    x, y = _x()
    assert env["ft"].train_path_ok(net, x) == lt
    h = env["lib"].lib()
    calls = []
    for name in ("bbb_reparam_kl_fwd", "bbb_reparam_kl_bwd", "bbb_reparam_kl_tp_fwd", "bbb_reparam_kl_tp_bwd"):
        fn = getattr(h, name)
        monkeypatch.setattr(h, name, lambda *a, _fn=fn, _n=name: (calls.append((_n, a[2] if "_tp_" in _n else a[1])), _fn(*a))[1])
    loss, _, kl = env["train"].forward_loss(net, x, y, 2, 0.1, 100.0)
    loss.backward()
    assert env["ens"].stats["path"] == "chwn-autograd"
    assert calls == [("bbb_reparam_kl_tp_fwd", 6), ("bbb_reparam_kl_tp_bwd", 6)], calls
    _check_kl(env, net, float(kl))
    del calls[:]
    with torch.no_grad():
        env["ens"].mc_forward(net, x, 3)
    assert calls == [("bbb_reparam_kl_tp_fwd", 6)], calls
    net.fc1.set_prior(sigma=0.3)                                         # another scalar fallback: today's rule
    assert env["ft"].train_path_ok(net, x) is None


def test_bf16_storage_sees_the_same_kl(env):
    """precision="bf16" inference and one BBB train_step(precision="bf16") with tensor priors: the KL has the fp32 path's bits (the KL
    never sees the storage mode)."""
    T = env["train"]
    x, y = _x()
    net = _random_priors(_net("bbb"))
    with torch.no_grad():
        env["rng"].manual_seed(9, call=0)
        _, k32 = env["ens"].mc_forward(net, x, 3)
        env["rng"].manual_seed(9, call=0)
        _, k16 = env["ens"].mc_forward(net, x, 3, precision="bf16")
    assert float(k32) == float(k16)
    out = {}
    for prec in ("fp32", "bf16"):
        net = _random_priors(_net("bbb"))
        env["rng"].manual_seed(9, call=0)
        opt = T.FusedAdam(net.parameters(), lr=1e-3)
        loss, _, kl = T.train_step(net, opt, x, y, 2, 0.1, 100.0, graph=False, precision=prec)
        assert np.isfinite(float(loss))
        out[prec] = float(kl)
    assert out["fp32"] == out["bf16"], out


@pytest.mark.parametrize("lt", ["bbb", "lrt"])
def test_moped_then_a_step(env, lt):
    T = env["train"]
    net = _net(lt)
    torch.manual_seed(2)
    det = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2, 2), nn.Flatten(), nn.Linear(128, 12), nn.Softplus(),
                        nn.Linear(12, 10)).cuda()
    env["priors"].moped(net, det, delta=0.1, prior_sigma=1.0)
    x, y = _x()
    ref = _kl64(env, net)
    opt = T.FusedAdam(net.parameters(), lr=1e-3)
    loss, _, kl = T.train_step(net, opt, x, y, 2, 0.1, 100.0, graph=False)
    assert np.isfinite(float(loss))
    P.check_kl_tp(float(kl), ref, max(P.FWD_C.values()))                 # (the KL of the step's forward: before the update)


@pytest.mark.parametrize("lt", ["bbb", "lrt"])
def test_posterior_as_prior_over_two_tasks(env, lt):
    T = env["train"]
    net = _net(lt)
    xa, ya = _x(1)
    xb, yb = _x(2)
    opt = T.FusedAdam(net.parameters(), lr=1e-2)
    for _ in range(20):
        T.train_step(net, opt, xa, ya, 2, 0.1, 100.0)
    env["priors"].from_posterior(net)
    with torch.no_grad():
        kl0 = float(sum(l.kl_loss() for l in env["ens"].bayesian_layers(net)))
        _, kl_net = net(xa)
    ref = _kl64(env, net)
    c = max(P.FWD_C.values())
    assert abs(ref[0]) <= 4 * 2.0 ** -23 * ref[1]                        # float64 itself: softplus of torch against the oracle's
    bound = c * 2.0 ** -23 * ref[1] + abs(ref[0])                        # the contract's bound around the float64 value (about zero)
    print("PRIORS two tasks %s: sum of kl_loss() %r, net(x) kl %r, float64 %r, bound %.3g" % (lt, kl0, float(kl_net), ref[0], bound))
    assert abs(kl0) <= bound and abs(float(kl_net)) <= bound
    kls = [float(T.train_step(net, opt, xb, yb, 2, 0.1, 100.0)[2]) for _ in range(20)]
    assert kls[-1] > kls[0] and kls[-1] > 100 * c * 2.0 ** -23 * ref[1], kls
