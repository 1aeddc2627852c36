"""bf16 training (train.train_step / forward_loss / GraphedTrainStep with precision="bf16") on the MI355X: the new backward kernels
against float64 torch, whole-model gradients against the test-side restatement of the contract (tests/bf16_train_contract.py,
DESIGN.md section 4.5) and against the fp32 path, training, graphs, determinism, refusals.  Stated tolerances:
  * pooling / activation backward: half a bf16 ulp of the float64 value computed from the same bf16 inputs (one rounding);
  * bias partials: 1e-5 of the sum of magnitudes (fp32 accumulation order only);
  * flips, transposes, batch chunks: bitwise (they move values);
  * dgrad / wgrad on the bf16 GEMM: 2e-5 relative to sum |a||b| of the float64 contraction of the same bf16 operands, plus half a
    bf16 ulp where the output is bf16;
  * whole-model parameter gradients vs the restatement: 4e-2 of each tensor's max |value| -- a rounding that lands within
    accumulation error of a bf16 boundary flips by one ulp, a flipped tie re-routes a whole pooling window's gradient, and the
    flips cascade (measured on the MI355X: 2.6e-2 for AlexNet / ReLU conv4 W_rho, whose 2 x 2 maps pool ReLU outputs; <= 7.8e-3
    for every other model, activation and tensor);
  * against the fp32 path's gradients for the same noise: cosine >= 0.995 per tensor (measured: >= 0.9979, first layers lowest);
  * loss forward: log_outputs within 1e-2 of their largest magnitude of the bf16 inference path (measured: 0), KL bitwise the fp32 KL;
  * 20 training steps: every bf16 loss within 2e-2 relative of the fp32 loss of the same step (measured: <= 4.2e-3).
Run with -m gpu."""
import numpy as np
import pytest
import torch

import bbb_numpy as O
import bf16_train_contract as C
import ref_port_torch as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import _lib, ensemble, ops, rng, train, zoo
    return dict(lib=_lib, ops=ops, rng=rng, ens=ensemble, zoo=zoo, train=train)


def _bf(t):
    return t.to(torch.bfloat16)


def _half_ulp(v):
    """Half a bf16 ulp of each value of a float64 tensor (0 where v == 0)."""
    a = v.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    return torch.where(a > 0, torch.pow(2.0, e - 8), torch.zeros_like(a))


def _pack_w(w, tap_major):
    """[E, Cout, Cin, kh, kw] -> bf16 rows [E, Cout, Kp] (zero pad), (r, q, ci) columns when tap_major."""
    E, Cout = w.shape[:2]
    K = w[0, 0].numel()
    out = torch.zeros(E, Cout, (K + 7) & ~7, dtype=torch.bfloat16, device=w.device)
    src = w.permute(0, 1, 3, 4, 2) if tap_major else w
    out[:, :, :K] = _bf(src.reshape(E, Cout, K))
    return out


# ---- kernels --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,s", [(0, 1), (2, 2), (3, 2)])
@pytest.mark.parametrize("act", [None, "relu", "softplus"])
@pytest.mark.parametrize("g_f32", [False, True])
def test_pool_act_backward_bf16_kernel_vs_torch(env, k, s, act, g_f32):
    ops = env["ops"]
    torch.manual_seed(10 * k + s)
    E, Cc, H, W, B = 2, 3, 9, 11, 16
    y = torch.randn(E, Cc, H, W, B, device="cuda")
    if act == "relu":
        y = y.clamp_min(0)
    elif act == "softplus":
        y = torch.nn.functional.softplus(y)
    y = _bf((y * 4).round() / 4)                   # coarse values: ties inside windows are common
    hp, wp = ((H - k) // s + 1, (W - k) // s + 1) if k else (H, W)
    g = torch.randn(E, Cc, hp, wp, B, device="cuda")
    g = g if g_f32 else _bf(g)
    got = ops.pool_act_backward_chwn_bf16(g, y, k, s, act)
    assert got.dtype == torch.bfloat16
    y64 = y.double().cpu().permute(0, 4, 1, 2, 3).reshape(E * B, Cc, H, W)
    g64 = g.double().cpu().permute(0, 4, 1, 2, 3).reshape(E * B, Cc, hp, wp)
    r = C._route(g64, y64, k, s) if k else g64
    if act is not None:
        r = r * C._act_grad(y64, act)
    want = r.reshape(E, B, Cc, H, W).permute(0, 2, 3, 4, 1)
    err = (got.double().cpu() - want).abs()
    assert bool((err <= _half_ulp(want) * (1 + 1e-6) + 1e-30).all()), float(err.max())
    # the fp32 form holds exactly the values of the bf16 one, at the padded pitch when asked
    f = ops.pool_act_backward_chwn_bf16(g, y, k, s, act, out_f32=True, pad_planes=True)
    assert torch.equal(f, got.float())
    # bias partials of that g_pre
    sums = ops.plane_sums_bf16(got)
    w64 = got.double().sum(dim=(2, 3, 4)).cpu()
    assert float((sums.double().cpu() - w64).abs().max()) <= 1e-5 * float(got.double().abs().sum(dim=(2, 3, 4)).max()) + 1e-30


@pytest.mark.parametrize("cout,cin,kh,kw", [(16, 6, 5, 5), (64, 32, 5, 5), (10, 84, 1, 1), (192, 64, 3, 3), (12, 3, 5, 5)])
def test_flip_transpose_bf16_bitwise(env, cout, cin, kh, kw):
    ops = env["ops"]
    torch.manual_seed(cout + cin)
    w = torch.randn(3, cout, cin, kh, kw, device="cuda")
    rows = _pack_w(w, ops.bf16_tap_major((cout, cin, kh, kw)))
    got = ops.flip_transpose_w_bf16(rows, (cout, cin, kh, kw))
    want = _pack_w(w.flip(3, 4).transpose(1, 2).contiguous(), ops.bf16_tap_major((cin, cout, kh, kw)))
    assert torch.equal(got, want)


@pytest.mark.parametrize("C_,H,W,B,cp", [(6, 14, 14, 32, 8), (64, 5, 5, 72, 64), (120, 1, 1, 256, 120), (3, 4, 4, 8, 16)])
def test_layout_transposes_bf16_bitwise(env, C_, H, W, B, cp):
    ops = env["ops"]
    torch.manual_seed(C_ + B)
    x = _bf(torch.randn(2, C_, H, W, B, device="cuda"))
    got = ops.chwn_to_bhwc_bf16(x, cp)
    want = torch.zeros(2, B, H, W, cp, dtype=torch.bfloat16, device="cuda")
    want[..., :C_] = x.permute(0, 4, 2, 3, 1)
    assert torch.equal(got, want)
    for S in (1, 2, B // 8):
        if B % (8 * S) == 0:
            ch = ops.batch_chunks_bf16(x, S)
            assert torch.equal(ch, x.reshape(2, C_, H, W, S, B // S).permute(0, 4, 1, 2, 3, 5).contiguous())


def _contract_bound(a64, b64, conv):
    """2e-5 of sum |a||b| per output element."""
    return 2e-5 * conv(a64.abs(), b64.abs())


@pytest.mark.parametrize("E,cout,cin,H,W,kh,pad,B", [(2, 16, 6, 10, 10, 5, 0, 32), (1, 64, 32, 15, 15, 5, 2, 64),
                                                     (2, 192, 64, 4, 4, 5, 2, 64), (2, 10, 84, 1, 1, 1, 0, 32),
                                                     (1, 128, 64, 3, 3, 3, 1, 256)])
def test_bf16_dgrad_wgrad_vs_float64(env, E, cout, cin, H, W, kh, pad, B):
    """Input and weight gradients of a stride-1 layer on the bf16 GEMM vs the float64 contraction of the same bf16 operands
    (padding, a 6-channel input, a linear layer, batch-chunked weight gradients)."""
    ops = env["ops"]
    F = torch.nn.functional
    torch.manual_seed(cout * 7 + cin)
    Ho, Wo = H + 2 * pad - kh + 1, W + 2 * pad - kh + 1
    w = _bf(torch.randn(E, cout, cin, kh, kh, device="cuda") * 0.1)
    x = _bf(torch.randn(E, cin, H, W, B, device="cuda"))
    g = _bf(torch.randn(E, cout, Ho, Wo, B, device="cuda"))
    rows = _pack_w(w.float(), ops.bf16_tap_major((cout, cin, kh, kh)))
    gx = ops.conv2d_chwn_input_grad_bf16(g, rows, (cout, cin, kh, kh), (H, W), pad, 1)
    gw = ops.conv2d_chwn_weight_grad_bf16(g, x, (E, cout, cin, kh, kh), 1, pad, 1)
    assert gx.dtype == torch.bfloat16 and gw.dtype == torch.float32
    for e in range(E):
        w64, x64 = w[e].double().cpu(), x[e].double().cpu().permute(3, 0, 1, 2)
        g64 = g[e].double().cpu().permute(3, 0, 1, 2)
        want_x = torch.nn.grad.conv2d_input(tuple(x64.shape), w64, g64, 1, pad)
        bound_x = _contract_bound(w64, g64, lambda a, b: torch.nn.grad.conv2d_input(tuple(x64.shape), a, b, 1, pad))
        got_x = gx[e].double().cpu().permute(3, 0, 1, 2)
        assert bool(((got_x - want_x).abs() <= bound_x + _half_ulp(want_x) * (1 + 1e-6) + 1e-30).all())
        want_w = torch.nn.grad.conv2d_weight(x64, tuple(w64.shape), g64, 1, pad)
        bound_w = _contract_bound(x64, g64, lambda a, b: torch.nn.grad.conv2d_weight(a, tuple(w64.shape), b, 1, pad))
        assert bool(((gw[e].double().cpu() - want_w).abs() <= bound_w + 1e-30).all()), float((gw[e].double().cpu() - want_w).abs().max())


# ---- whole model ----------------------------------------------------------------------------------------------------------------

def _model(env, net_type, cin, activation, seed=11):
    torch.manual_seed(seed)
    params = P.init_params(net_type, cin, 10, P.CONFIG_PRIORS)
    net = env["zoo"].getModel(net_type, cin, 10, P.CONFIG_PRIORS, "bbb", activation)
    net.load_state_dict({f"{n}.{k}": v for n, p in params.items() if not n.startswith("_") for k, v in p.items()}, strict=True)
    net = net.cuda()
    env["rng"].assign_stream_ids(net)
    npar = {n: {k: v.numpy() for k, v in p.items()} if isinstance(p, dict) else p for n, p in params.items()}
    return net, npar


def _grads(env, net, x, y, E, seed_call, precision, beta=0.1, n=50000.0):
    net.zero_grad(set_to_none=True)
    loss, lo, kl = env["train"].forward_loss(net, x, y, E, beta, n, seed_call=seed_call, precision=precision)
    loss.backward()
    return loss.detach(), lo.detach(), kl.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("net_type,B,cin,activation", [("3conv3fc", 256, 3, "softplus"), ("3conv3fc", 256, 3, "relu"),
                                                       ("alexnet", 64, 3, "softplus"), ("alexnet", 64, 3, "relu"),
                                                       ("lenet", 32, 1, "softplus"), ("lenet", 32, 1, "relu")])
def test_model_gradients_vs_contract_and_fp32(env, net_type, B, cin, activation):
    net, npar = _model(env, net_type, cin, activation)
    torch.manual_seed(5)
    x = torch.rand(B, cin, 32, 32, device="cuda")
    y = torch.randint(0, 10, (B,), device="cuda")
    E, seed, call0 = 2, 4242, 7
    loss, lo, kl, got = _grads(env, net, x, y, E, (seed, call0), "bf16")
    _, _, kl32, g32 = _grads(env, net, x, y, E, (seed, call0), "fp32")
    assert torch.equal(kl, kl32)
    mods = dict(net.named_modules())
    names = [op[1] for op in O.TOPOLOGY[net_type] if op[0] in ("conv", "fc")]
    eps = [{nm: {kind: O.normal_eps(seed, call0 + e, mods[nm]._stream_base + off, int(np.prod(npar[nm][key].shape))).reshape(npar[nm][key].shape)
                 for kind, key, off in (("W", "W_mu", 0), ("bias", "bias_mu", 1))} for nm in names} for e in range(E)]
    loss_c, lo_c, want = C.step_grads(net_type, npar, x.cpu().numpy(), y.cpu().numpy(), eps, activation, 0.1, 50000.0)
    worst, cos_min = 0.0, 1.0
    for nm in names:
        for key in ("W_mu", "W_rho", "bias_mu", "bias_rho"):
            g = got[f"{nm}.{key}"].double().cpu().numpy()
            w = np.asarray(want[nm][key]).reshape(g.shape)
            scale = float(np.abs(w).max())
            rel = float(np.abs(g - w).max()) / scale
            worst = max(worst, rel)
            assert rel <= 4e-2, (nm, key, rel)
            a, b = got[f"{nm}.{key}"].double().flatten(), g32[f"{nm}.{key}"].double().flatten()
            cos = float(a @ b / (a.norm() * b.norm()))
            cos_min = min(cos_min, cos)
            assert cos >= 0.995, (nm, key, cos)
    print(f"{net_type} {activation}: max rel grad err vs contract {worst:.2e}, min cosine vs fp32 {cos_min:.6f}")


def test_forward_loss_bf16_matches_the_inference_path(env):
    net, _ = _model(env, "3conv3fc", 3, "softplus")
    torch.manual_seed(6)
    x = torch.rand(256, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (256,), device="cuda")
    E, seed, call0 = 3, 99, 40
    loss, lo, kl = env["train"].forward_loss(net, x, y, E, 0.1, 50000.0, seed_call=(seed, call0), precision="bf16")
    _, _, kl32 = env["train"].forward_loss(net, x, y, E, 0.1, 50000.0, seed_call=(seed, call0))
    assert torch.equal(kl.detach(), kl32.detach())
    with torch.no_grad():
        lo_inf, kl_inf = env["ens"]._local_lse(net, x, E, seed, call0, E, precision="bf16")
    scale = max(1.0, float(lo_inf.abs().max()))
    d = float((lo.detach() - lo_inf).abs().max())
    print(f"forward_loss bf16 vs inference bf16: {d:.3e} (scale {scale:.3e})")
    assert d <= 1e-2 * scale


def test_twenty_bf16_training_steps_track_fp32(env):
    T = env["train"]
    torch.manual_seed(7)
    x = torch.rand(256, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (256,), device="cuda")
    losses = {}
    for prec in ("fp32", "bf16"):
        net, _ = _model(env, "3conv3fc", 3, "softplus", seed=21)
        env["rng"].manual_seed(1234, call=0)
        opt = T.FusedAdam(net.parameters(), lr=1e-3)
        losses[prec] = [T.train_step(net, opt, x, y, 1, 0.1, 50000.0, precision=prec, graph=False)[0].item() for _ in range(20)]
    a, b = np.array(losses["bf16"]), np.array(losses["fp32"])
    rel = np.abs(a - b) / np.abs(b)
    print(f"20 steps: max rel loss distance {rel.max():.2e}; bf16 {a[0]:.4e} -> {a[-1]:.4e}")
    assert rel.max() <= 2e-2, rel
    assert a[-1] < a[0] and np.all(np.isfinite(a))


def test_graphed_bf16_step_equals_eager_and_self_capture_keys_on_precision(env):
    T = env["train"]
    B, E, lr, beta, n = 64, 2, 1e-3, 0.1, 1000.0
    torch.manual_seed(3)
    x = torch.rand(B, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (B,), device="cuda")

    def fresh():
        net, _ = _model(env, "3conv3fc", 3, "softplus", seed=12)
        env["rng"].manual_seed(77, call=0)
        return net

    net_e = fresh()
    opt_e = T.FusedAdam(net_e.parameters(), lr=lr, capturable=True)       # the same Adam arithmetic (device-side step count) as the graph
    eager = [T.train_step(net_e, opt_e, x, y, E, beta, n, precision="bf16", graph=False)[0] for _ in range(6)]
    net_g = fresh()
    opt_g = T.FusedAdam(net_g.parameters(), lr=lr, capturable=True)
    g = T.GraphedTrainStep(net_g, opt_g, x, y, E, beta, n, warmup=3, precision="bf16")
    graphed = [g.step()[0].clone() for _ in range(3)]
    for a, b in zip(eager[3:], graphed):
        assert torch.equal(a, b)
    for (na, a), (_, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(a, b), na
    # train_step's self-capture: the key holds the precision, so a bf16 call never replays the fp32 graph (and back)
    net_a = fresh()
    opt_a = T.FusedAdam(net_a.parameters(), lr=lr)
    for _ in range(T.auto_graph["after"] + 2):
        T.train_step(net_a, opt_a, x, y, E, beta, n)
    st = T._auto.get(net_a)
    assert st is not None and st["graphed"] is not None and st["key"][-1] == "fp32"
    T.train_step(net_a, opt_a, x, y, E, beta, n, precision="bf16")
    st = T._auto.get(net_a)
    assert st["graphed"] is None and st["key"][-1] == "bf16"


def test_bf16_steps_are_deterministic(env):
    torch.manual_seed(8)
    x = torch.rand(64, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (64,), device="cuda")
    net, _ = _model(env, "alexnet", 3, "relu")
    _, _, _, g1 = _grads(env, net, x, y, 4, (5, 100), "bf16")
    _, _, _, g2 = _grads(env, net, x, y, 4, (5, 100), "bf16")
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_bf16_training_refuses_what_it_does_not_cover(env):
    T, err = env["train"], env["lib"].BBBHipError
    x = torch.rand(16, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (16,), device="cuda")
    net, _ = _model(env, "3conv3fc", 3, "softplus")
    opt = T.FusedAdam(net.parameters(), lr=1e-3)
    with pytest.raises(err):
        T.train_step(net, opt, x, y, 1, 0.1, 100.0, precision="fp16")
    with pytest.raises(err):                                    # B % 8 != 0
        T.train_step(net, opt, x[:12], y[:12], 1, 0.1, 100.0, precision="bf16")
    lrt = env["zoo"].getModel("3conv3fc", 3, 10, P.CONFIG_PRIORS, "lrt", "softplus").cuda()
    env["rng"].assign_stream_ids(lrt)
    with pytest.raises(err):
        T.forward_loss(lrt, x, y, 1, 0.1, 100.0, precision="bf16")
    with pytest.raises(err):
        T.GraphedTrainStep(lrt, T.FusedAdam(lrt.parameters(), capturable=True), x, y, 1, 0.1, 100.0, precision="bf16")
    net.conv1.eps_source = lambda shape: torch.zeros(tuple(shape))
    try:
        with pytest.raises(err):
            T.forward_loss(net, x, y, 1, 0.1, 100.0, precision="bf16")
    finally:
        net.conv1.eps_source = None
    off = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3)).cuda()     # not a Bayesian model: off the fast path
    with pytest.raises(err):
        T.forward_loss(off, x, y, 1, 0.1, 100.0, precision="bf16")
