"""bf16 storage path for LRT models (LaunchConfig.bf16_lrt; csrc/pconv_bf16_lrt.hip) on the MI355X against the arithmetic
contract of DESIGN.md section 4.5b (tests/bf16_lrt_contract.py), against float64 on the same bf16 operands, against the fp32 LRT
path's noise, and against the fp32 LRT path itself.  Stated tolerances:
  * moments of one launch, Gaussian operands: 2e-5 * sum|a||b| + 2e-6 (the project's bound for its bf16 kernels: fp32
    accumulation order only); exact-tier operands (small integers x powers of two): bit for bit;
  * sampled output: that bound carried through mu + sqrt(var) * eps -- the mu bound plus the var bound times |eps| / (2 sqrt(var))
    -- plus 2^-8 |want| for bf16 outputs (one rounding);
  * whole model against the contract, same noise: 1e-2 * max|logit| (the BBB bf16 model bound of the same storage model);
  * whole model against the fp32 LRT path, same noise: 2.4e-2 * max|logit| = twice the measured worst (1.21e-2, AlexNet).
Run with -m gpu."""
import numpy as np
import pytest
import torch

import bbb_numpy as O
import ref_port_torch as P
import bf16_lrt_contract as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import ops, rng, ensemble, zoo, train, _lib
    return dict(ops=ops, rng=rng, ens=ensemble, zoo=zoo, train=train, lib=_lib)


# name -> (B, Cin, H, W, Cout, kh, kw, stride, (ph, pw), dil, E)
CASES = {
    "lenet-conv1":      (8, 1, 12, 12, 6, 5, 5, 1, (0, 0), 1, 1),          # one input channel, 6 outputs, 8 images: 64 x 128 tiles
    "nonsquare-s2":     (200, 3, 16, 16, 100, 5, 3, 2, (4, 2), 1, 3),      # 5 x 3 taps, stride 2, padding d (k - 1), ragged 100 / 200
    "dilated-192":      (256, 16, 9, 7, 192, 3, 3, 1, (4, 4), 2, 3),       # dilation 2, padding d (k - 1), 9 x 7 map, 64 x 256 tiles
    "straddling-taps":  (200, 24, 5, 7, 100, 3, 3, 1, (1, 1), 1, 3),       # cin = 24: 64-k tiles straddle taps in the tap-major order
    "large-launch":     (256, 8, 12, 12, 128, 3, 3, 1, (1, 1), 1, 10),     # 2880 workgroups of 128 x 128: no wave specialisation
    "long-rows-22":     (256, 128, 2, 2, 256, 3, 3, 1, (1, 1), 1, 10),     # AlexNet conv4 family: two k-groups, 128 x 128 tiles
    "long-rows-14":     (256, 128, 4, 4, 64, 3, 3, 1, (1, 1), 1, 10),      # two k-groups, 64 x 256 tiles
    "classifier":       (200, 1040, 1, 1, 10, 1, 1, 1, (0, 0), 1, 3),      # linear, long rows, a handful of workgroups: two k-groups
    "lenet-fc2":        (8, 120, 1, 1, 84, 1, 1, 1, (0, 0), 1, 1),         # linear, 84 outputs
    "one-pixel-map":    (8, 16, 3, 5, 10, 3, 5, 1, (0, 0), 1, 3),          # 3 x 5 map and kernel -> one output pixel
    "alexnet-conv1":    (256, 3, 32, 32, 64, 11, 11, 4, (5, 5), 1, 1),     # K = 363 (padded rows), stride 4
    "seven-channels":   (8, 7, 6, 6, 10, 3, 3, 2, (1, 1), 1, 3),           # a first layer on 7 channels, stride 2
}


def out_hw(c):
    B, Cin, H, W, Cout, kh, kw, s, (ph, pw), d, E = c
    return (H + 2 * ph - d * (kh - 1) - 1) // s + 1, (W + 2 * pw - d * (kw - 1) - 1) // s + 1


def tap_major_options(c):
    """Reference-order rows always; tap-major rows too where the layout exists (ops.bf16_tap_major's rule)."""
    return (False, True) if (c[1] % 8 == 0 and c[5] * c[6] > 1) else (False,)


def case_branches(name, plan):
    """What the launcher (ops.lrt_bf16_plan = bbb_lrt_conv2d_chwn_bf16_plan) picks for a case, as tags; every case runs with fp32
    and bf16 output, sampled and moments-only, and in both weight row orders where tap_major_options says so."""
    c = CASES[name]
    sh, kg, ws = plan((c[10], c[1], c[2], c[3], c[0]), c[4], (c[1], c[5], c[6]), c[7], c[8], c[9])
    tags = {f"shape{sh}", f"kg{kg}", "ws" if ws else "no-ws", f"inst:{sh}-kg{kg}-{'ws' if ws else 'plain'}"}
    tags |= {"out-f32", "out-bf16", "moments-only", "rows-reference"}
    if len(tap_major_options(c)) == 2:
        tags.add("rows-tap-major")
    return tags


def exact_operands(c, seed):
    """The exact tier: x = k / 4 with |k| in 1..4 (x^2 = k^2 / 16 is a bf16 value), W_mu = j / 8 with |j| <= 8, sigma^2 = i * 2^-9
    with i in 1..4, biases alike.  Products are multiples of 2^-5 (mean) and 2^-13 (variance) and every partial sum stays far below
    2^24 of those units, so any summation order is exact in fp32."""
    B, Cin, H, W, Cout, kh, kw, s, pad, d, E = c
    g = np.random.default_rng(seed)
    x = (g.integers(1, 5, size=(E, B, Cin, H, W)) * g.choice([-1, 1], size=(E, B, Cin, H, W)) / 4.0).astype(np.float32)
    w_mu = (g.integers(-8, 9, size=(Cout, Cin, kh, kw)) / 8.0).astype(np.float32)
    w_var = (g.integers(1, 5, size=(Cout, Cin, kh, kw)) * 2.0 ** -9).astype(np.float32)
    b_mu = (g.integers(-8, 9, size=(Cout,)) / 8.0).astype(np.float32)
    b_var = (g.integers(1, 5, size=(Cout,)) * 2.0 ** -9).astype(np.float32)
    return x, w_mu, w_var, b_mu, b_var


def gaussian_operands(c, seed):
    """|x| in [0.25, 1] and sigma^2 in [1e-4, 1e-2]: act_var is bounded away from 0, no element needs excluding."""
    B, Cin, H, W, Cout, kh, kw, s, pad, d, E = c
    g = np.random.default_rng(seed)
    K = Cin * kh * kw
    x = (g.uniform(0.25, 1.0, size=(E, B, Cin, H, W)) * g.choice([-1, 1], size=(E, B, Cin, H, W))).astype(np.float32)
    w_mu = (g.standard_normal((Cout, Cin, kh, kw)) / np.sqrt(K)).astype(np.float32)
    w_var = g.uniform(1e-4, 1e-2, size=(Cout, Cin, kh, kw)).astype(np.float32)
    b_mu = (g.standard_normal((Cout,)) * 0.1).astype(np.float32)
    b_var = g.uniform(1e-4, 1e-2, size=(Cout,)).astype(np.float32)
    return x, w_mu, w_var, b_mu, b_var


def _contract64(x, w, b, s, pad, d):
    """float64 conv of float64 tensors on the device (unfold + matmul): [N, Cin, H, W] x [Cout, Cin, kh, kw] -> [N, Cout, L]."""
    cols = torch.nn.functional.unfold(x, w.shape[2:], dilation=d, padding=pad, stride=s)          # [N, K, L]
    y = torch.einsum("ok,nkl->nol", w.reshape(w.shape[0], -1), cols)
    return y if b is None else y + b[None, :, None]


def _launch(env, c, xb, wm_b, wv_b, b_mu, b_var, tapm, **kw):
    B, Cin, H, W, Cout, kh, kw_, s, pad, d, E = c
    return env["ops"].lrt_conv2d_chwn_bf16_forward(xb, wm_b, wv_b, b_mu, b_var, (Cin, kh, kw_), SEED, CALL0, STREAM, s, pad, d,
                                                   tap_major=tapm, **kw)


SEED, CALL0, STREAM = 20240607, 11, 6


def _eps(env, c, e):
    """The fp32 path's noise for draw e: element index = canonical [B][Cout][Ho][Wo] index, stream STREAM, call CALL0 + e."""
    ho, wo = out_hw(c)
    n = c[0] * c[4] * ho * wo
    return env["ops"].eps_dump(n, SEED, CALL0 + e, STREAM, torch.device("cuda")).reshape(c[0], c[4], ho * wo).double()


@pytest.mark.parametrize("tier", ["exact", "gaussian"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_float64_on_the_same_bf16_operands(env, name, tier):
    ops = env["ops"]
    c = CASES[name]
    B, Cin, H, W, Cout, kh, kw, s, pad, d, E = c
    ho, wo = out_hw(c)
    x, w_mu, w_var, b_mu, b_var = (exact_operands if tier == "exact" else gaussian_operands)(c, len(name) * 31 + E)
    bf = lambda t: torch.from_numpy(t).cuda().to(torch.bfloat16)
    xq, wmq, wvq = bf(x), bf(w_mu), bf(w_var)                                   # the stored operands
    if tier == "exact":
        assert torch.equal(xq.float().cpu(), torch.from_numpy(x)) and torch.equal(wvq.float().cpu(), torch.from_numpy(w_var))
    bm, bv = torch.from_numpy(b_mu).cuda(), torch.from_numpy(b_var).cuda()
    xb = xq.permute(0, 2, 3, 4, 1).contiguous()                                 # [E, Cin, H, W, B]
    # float64 on the same operands; x^2 rounded once to bf16 as the contract says
    x64 = xq.double().reshape(E * B, Cin, H, W)
    x2_64 = (xq.float() * xq.float()).to(torch.bfloat16).double().reshape(E * B, Cin, H, W)
    mu64 = _contract64(x64, wmq.double(), bm.double(), s, pad, d).reshape(E, B, Cout, ho * wo)
    var64 = _contract64(x2_64, wvq.double(), bv.double(), s, pad, d).reshape(E, B, Cout, ho * wo) + 1e-16
    mag_mu = _contract64(x64.abs(), wmq.double().abs(), bm.double().abs(), s, pad, d).reshape(E, B, Cout, ho * wo)
    tol_mu = 2e-5 * mag_mu + 2e-6
    tol_var = 2e-5 * var64 + 2e-6                                               # every term of the variance is non-negative
    eps = torch.stack([_eps(env, c, e) for e in range(E)])                      # [E, B, Cout, L]
    to_ebcl = lambda t: t.double().reshape(E, Cout, ho * wo, B).permute(0, 3, 1, 2)
    rows = ops.lrt_weights_bf16([torch.from_numpy(w_mu).cuda(), torch.from_numpy(w_var).cuda()])
    assert rows[0].shape == (Cout, ops.bf16_row_pitch(Cin * kh * kw))
    for tapm in tap_major_options(c):
        if tapm:
            wm_b, wv_b = rows
            assert ops.bf16_tap_major((Cout, Cin, kh, kw))
        else:                                           # reference-order rows: the conversion of the matrices seen as [Cout, K]
            wm_b, wv_b = ops.lrt_weights_bf16([torch.from_numpy(w_mu).cuda().reshape(Cout, -1), torch.from_numpy(w_var).cuda().reshape(Cout, -1)])
            assert torch.equal(wm_b[:, :Cin * kh * kw], wmq.reshape(Cout, -1)) and not wm_b[:, Cin * kh * kw:].any()
        # fp32 output, no activation, with the moments
        y, am, av = _launch(env, c, xb, wm_b, wv_b, bm, bv, tapm, out_f32=True, want_moments=True)
        assert y.dtype == torch.float32 and y.shape == (E, Cout, ho, wo, B)
        am, av, y = to_ebcl(am), to_ebcl(av), to_ebcl(y)
        if tier == "exact":
            assert torch.equal(am, mu64), float((am - mu64).abs().max())
            assert torch.equal(av, var64.float().double()), float((av - var64).abs().max())
        else:
            assert bool(((am - mu64).abs() <= tol_mu).all()), float(((am - mu64).abs() - tol_mu).max())
            assert bool(((av - var64).abs() <= tol_var).all()), float(((av - var64).abs() - tol_var).max())
        # the noise: y = y_mu + sqrt(y_var) * eps of the fp32 path's stream, call and index, to a few fp32 ulps of the terms
        want_y = am + av.sqrt() * eps
        ulps = 4 * 2.0 ** -23 * (am.abs() + av.sqrt() * eps.abs()) + 1e-30
        assert bool(((y - want_y).abs() <= ulps).all()), float((y - want_y).abs().max())
        # ... and against float64 throughout
        tol_y = tol_mu + tol_var * eps.abs() / (2 * var64.sqrt())
        want64 = mu64 + var64.sqrt() * eps
        assert bool(((y - want64).abs() <= tol_y + ulps).all()), float(((y - want64).abs() - tol_y).max())
        # bf16 output behind the activation (1-Lipschitz): one more rounding
        yb, _, _ = _launch(env, c, xb, wm_b, wv_b, bm, bv, tapm, act="softplus")
        assert yb.dtype == torch.bfloat16
        want_sp = torch.nn.functional.softplus(want64)
        err = (to_ebcl(yb) - want_sp).abs()
        assert bool((err <= tol_y + ulps + 2.0 ** -8 * want_sp.abs()).all()), float((err - tol_y - 2.0 ** -8 * want_sp.abs()).max())
        # moments-only launch: no y, the same moments bit for bit; two identical calls are bitwise equal
        none, am2, av2 = _launch(env, c, xb, wm_b, wv_b, bm, bv, tapm, sample=False, moments_only=True)
        assert none is None and torch.equal(to_ebcl(am2), am) and torch.equal(to_ebcl(av2), av)
        yb2, _, _ = _launch(env, c, xb, wm_b, wv_b, bm, bv, tapm, act="softplus")
        assert torch.equal(yb, yb2)
        # a slab computed alone is the slab of the larger launch (the summation order belongs to the layer)
        if E > 1:
            one = env["ops"].lrt_conv2d_chwn_bf16_forward(xb[E - 1:], wm_b, wv_b, bm, bv, (Cin, kh, kw), SEED, CALL0 + E - 1, STREAM, s, pad, d,
                                                          tap_major=tapm, act="softplus")[0]
            assert torch.equal(one[0], yb[E - 1])
        # cross-check: act_mu of the fp32 LRT kernel fed the fp32 values of the same bf16 operands
        _, am32, _ = ops.lrt_conv2d_chwn_forward(xb.float(), wmq.float(), wvq.float(), bm, bv, SEED, CALL0, STREAM, s, pad, d,
                                                 sample=False, want_moments=True)
        d32 = (to_ebcl(am32) - am).abs()
        assert bool((d32 <= tol_mu).all()), float((d32 - tol_mu).max())                  # the same sum|a||b| bound


@pytest.mark.parametrize("name", ["alexnet-conv1", "nonsquare-s2", "lenet-conv1", "one-pixel-map"])
@pytest.mark.parametrize("act", ["softplus", "relu", None])
def test_shared_first_layer_form_equals_sampling_launches(env, name, act):
    """Input and weights shared by the draws: one moments-only launch + lrt_sample_chwn_bf16 is bitwise E sampling launches."""
    ops = env["ops"]
    c = CASES[name]
    B, Cin, H, W, Cout, kh, kw, s, pad, d, _ = c
    E = 5
    x, w_mu, w_var, b_mu, b_var = gaussian_operands(c[:10] + (1,), 77)
    cu = lambda t: torch.from_numpy(t).cuda()
    xb = cu(x).to(torch.bfloat16).permute(0, 2, 3, 4, 1).contiguous()
    wm_b, wv_b = ops.lrt_weights_bf16([cu(w_mu).reshape(Cout, -1), cu(w_var).reshape(Cout, -1)])
    _, am, av = _launch(env, c, xb, wm_b, wv_b, cu(b_mu), cu(b_var), False, sample=False, moments_only=True)
    got = ops.lrt_sample_chwn_bf16(am, av, E, SEED, CALL0, STREAM, act=act)
    assert got.dtype == torch.bfloat16 and got.shape == (E,) + tuple(am.shape[1:])
    for e in range(E):
        one = ops.lrt_conv2d_chwn_bf16_forward(xb, wm_b, wv_b, cu(b_mu), cu(b_var), (Cin, kh, kw), SEED, CALL0 + e, STREAM, s, pad, d, act=act)[0]
        assert torch.equal(one[0], got[e]), (e, float((one[0].float() - got[e].float()).abs().max()))
    assert not torch.equal(got[0], got[1])


# ---- whole models ----

def _model(env, net_type, cin, layer_type="lrt"):
    torch.manual_seed(11)
    params = P.init_params(net_type, cin, 10, P.CONFIG_PRIORS)
    net = env["zoo"].getModel(net_type, cin, 10, P.CONFIG_PRIORS, layer_type, "softplus")
    sd = {f"{n}.{k}": v for n, p in params.items() if not n.startswith("_") for k, v in p.items()}
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    env["rng"].assign_stream_ids(net)
    npar = {n: {k: v.numpy() for k, v in p.items()} for n, p in params.items() if not n.startswith("_")}
    return net, npar


def _device_eps_fn(env, net_type, seed, call):
    names = [op[1] for op in O.TOPOLOGY[net_type] if op[0] in ("conv", "fc")]
    idx = {n: i for i, n in enumerate(names)}

    def fn(name, kind, shape):
        assert kind == "act"
        n = int(np.prod(shape))
        return env["ops"].eps_dump(n, seed, call, 4 * idx[name] + 2, torch.device("cuda")).cpu().numpy().reshape(shape)
    return fn


# Measured on the MI355X, worst over the draws of each model, as a fraction of max|logit|:
#              |bf16 - contract|   |bf16 - fp32 LRT path|
#   lenet          1.5e-3              6.9e-3
#   3conv3fc       3.3e-3              7.3e-3
#   alexnet        5.0e-3              1.21e-2
# The contract bound is the BBB bf16 models' (1e-2: rounding-boundary flips of hidden activations, one bf16 ulp each, spreading
# through the later layers); it holds with a factor of two to spare.  The distance to the fp32 path is the rounding of W_mu, sigma^2,
# x, x^2 and the hidden activations themselves; it is bounded at twice the measured worst.
FP32_DISTANCE_BOUND = 2.4e-2


@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("net_type,B,cin", [("lenet", 32, 1), ("3conv3fc", 64, 3), ("alexnet", 64, 3)])
def test_models_against_contract_and_fp32(env, net_type, B, cin, E):
    ops, ens, rng = env["ops"], env["ens"], env["rng"]
    net, npar = _model(env, net_type, cin)
    x = torch.rand(B, cin, 32, 32)
    seed, call0 = 4242, 7
    with torch.no_grad():
        logits32, kl32 = ens.mc_logits(net, x.cuda(), E, seed, call0)
        with ops.use_config(bf16_lrt=True):
            logits, kl = ens.mc_logits(net, x.cuda(), E, seed, call0, precision="bf16")
            assert ens.stats["path"] == "chwn-bf16-lrt"
            again, _ = ens.mc_logits(net, x.cuda(), E, seed, call0, precision="bf16")
            rng.manual_seed(seed, call=call0)
            lo16, klf16 = ens.mc_forward(net, x.cuda(), E, precision="bf16")
        rng.manual_seed(seed, call=call0)
        lo32, klf32 = ens.mc_forward(net, x.cuda(), E)
    assert torch.equal(kl, kl32) and torch.equal(klf16, klf32)                   # KL never touches bf16
    assert torch.equal(logits, again)                                            # fixed summation orders, no atomics
    assert logits.shape == logits32.shape == (E, B, 10) and not torch.equal(logits, logits32)     # the mode really ran
    worst_c = worst_f = 0.0
    for e in range(E):
        want = C.model_forward(net_type, npar, x.numpy(), "softplus", _device_eps_fn(env, net_type, seed, call0 + e))
        got = logits[e].cpu().numpy()
        scale = float(np.abs(want).max())
        dc = float(np.abs(got - want).max()) / scale
        df = float((logits[e] - logits32[e]).abs().max()) / scale
        print(f"bf16-lrt {net_type} E={E} draw {e}: vs contract {dc:.3e}, vs fp32 {df:.3e} (of max|logit| {scale:.3e})")
        worst_c, worst_f = max(worst_c, dc), max(worst_f, df)
    assert worst_c <= 1e-2, worst_c
    assert worst_f <= FP32_DISTANCE_BOUND, worst_f
    # the whole step (log-probabilities): a perturbation of the fp32 step
    scale = max(1.0, float(lo32.abs().max()))
    assert float((lo16 - lo32).abs().max()) <= FP32_DISTANCE_BOUND * scale
    rng.use_device_generator()


@pytest.mark.parametrize("net_type,B", [("alexnet", 64), ("3conv3fc", 32)])
def test_graphs_replay_the_eager_step(env, net_type, B):
    """GraphedMC and GraphedPipeline (depth 2, 1 and 4 steps per launch) under bf16_lrt: every step is bitwise the eager single
    step for the same batch and noise calls, fresh noise per replay; the pipeline took a snapshot of the configuration, so it
    keeps working after the context that enabled the mode has exited."""
    ops, ens, rng = env["ops"], env["ens"], env["rng"]
    net, _ = _model(env, net_type, 3)
    E = 3
    torch.manual_seed(5)
    batches = [torch.rand(B, 3, 32, 32, device="cuda") for _ in range(8)]
    with torch.no_grad(), ops.use_config(bf16_lrt=True):
        rng.manual_seed(31, call=0)
        eager = [tuple(t.clone() for t in ens.mc_forward(net, xb, E, precision="bf16")) for xb in batches]
        rng.manual_seed(31, call=0)
        g = ens.GraphedMC(net, batches[0].clone(), E, precision="bf16")        # (a single lane uses the tensor it is given as its buffer)
        pipes = {}
        for G in (1, 4):
            rng.manual_seed(31, call=0)
            pipes[G] = ens.GraphedPipeline(net, batches[0].clone(), E, depth=2, steps_per_launch=G, precision="bf16")
    assert ops.current_config().bf16_lrt is False
    with torch.no_grad():
        for i in range(2):                                                   # fresh noise per replay: calls i * E .. (i + 1) * E - 1
            lo, kl = g.step(batches[i])
            torch.cuda.synchronize()
            assert torch.equal(lo, eager[i][0]) and torch.equal(kl, eager[i][1]), i
        assert not torch.equal(eager[0][0], eager[1][0])
        for G, pipe in pipes.items():
            views = []
            for i, xb in enumerate(batches):
                views.append((i, pipe.step(xb)))
                if G == 1 or (i + 1) % (2 * G) == 0:
                    pipe.sync()
                    for j, (lo, kl) in views:
                        assert torch.equal(lo, eager[j][0]), (G, j, float((lo - eager[j][0]).abs().max()))
                        assert torch.equal(kl, eager[j][1]), (G, j, float(kl), float(eager[j][1]))
                    views = []
        with pytest.raises(env["lib"].BBBHipError):                          # outside the context a NEW graph is refused again
            ens.GraphedMC(net, batches[0].clone(), E, precision="bf16")
        cfg = ops.current_config().copy(bf16_lrt=True)                       # ... unless it is handed the configuration
        rng.manual_seed(31, call=0)
        g2 = ens.GraphedMC(net, batches[0].clone(), E, precision="bf16", launch_config=cfg)
        lo, kl = g2.step(batches[0])
        torch.cuda.synchronize()
        assert torch.equal(lo, eager[0][0]) and torch.equal(kl, eager[0][1])
    rng.use_device_generator()


def test_refusals(env):
    ops, ens, rng, T, err = env["ops"], env["ens"], env["rng"], env["train"], env["lib"].BBBHipError
    net, _ = _model(env, "3conv3fc", 3)
    x = torch.rand(16, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (16,), device="cuda")
    with torch.no_grad():
        with pytest.raises(err, match="bf16_lrt"):                           # the default configuration still refuses, and names the switch
            ens.mc_forward(net, x, 2, precision="bf16")
        with pytest.raises(err):
            ens.mc_logits(net, x, 2, 1, 0, precision="bf16")
    with ops.use_config(bf16_lrt=True):
        with torch.no_grad():
            ens.mc_forward(net, x, 2, precision="bf16")                      # what it covers runs
            with pytest.raises(err):                                         # B % 8 != 0
                ens.mc_forward(net, x[:12], 2, precision="bf16")
            # mixed BBB / LRT models
            mixed = env["zoo"].getModel("lenet", 1, 10, P.CONFIG_PRIORS, "lrt", "softplus").cuda()
            bbb = env["zoo"].getModel("lenet", 1, 10, P.CONFIG_PRIORS, "bbb", "softplus").cuda()
            mixed.fc2 = bbb.fc2
            rng.assign_stream_ids(mixed)
            with pytest.raises(err, match="mixes"):
                ens.mc_forward(mixed, torch.rand(16, 1, 32, 32, device="cuda"), 2, precision="bf16")
            # eps replay
            eps = [[torch.zeros(1, device="cuda")]]
            with pytest.raises(err):
                ens.mc_logits(net, x, 1, 1, 0, eps=eps, precision="bf16")
            # the drop-in loop
            with ops.use_config(dropin_precision="bf16"), pytest.raises(err, match="drop-in"):
                net(x)
            # work units / shares of a group of steps / batch offsets
            with pytest.raises(err):
                ens._mc_logits_chwn(net, x, 2, 1, 0, precision="bf16", units=(2, 0, 2))
            with pytest.raises(err):
                ens._mc_logits_chwn(net, torch.cat([x, x]), 2, 1, 0, precision="bf16", share=(2, 1))
            with pytest.raises(err):
                ens._mc_logits_chwn(net, x, 2, 1, 0, precision="bf16", b_offset=16)
        with pytest.raises(err):                                             # autograd on
            ens.mc_forward(net, x, 2, precision="bf16")
        # training in bf16 on LRT models
        with pytest.raises(err):
            T.forward_loss(net, x, y, 1, 0.1, 100.0, precision="bf16")
        with pytest.raises(err):
            T.GraphedTrainStep(net, T.FusedAdam(net.parameters(), capturable=True), x, y, 1, 0.1, 100.0, precision="bf16")
    rng.use_device_generator()


def test_process_groups_are_refused(env, tmp_path, monkeypatch):
    """group= sharding of a bf16 LRT step is refused at its real call sites: GraphedMC with a (one-process gloo) group whose
    multi-rank protocol is forced, and the eager entry points as rank 0 of a group that reports two ranks -- each raises before
    anything is launched or any collective is entered."""
    import torch.distributed as dist
    ops, ens, rng, err = env["ops"], env["ens"], env["rng"], env["lib"].BBBHipError
    net, _ = _model(env, "3conv3fc", 3)
    x = torch.rand(16, 3, 32, 32, device="cuda")
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        group = dist.group.WORLD
        with torch.no_grad(), ops.use_config(bf16_lrt=True):
            monkeypatch.setenv("BBB_FORCE_COMBINE", "1")
            with pytest.raises(err, match="one device"):
                ens.GraphedMC(net, x, 2, precision="bf16", group=group)
            with pytest.raises(err, match="one device"):
                ens.GraphedPipeline(net, x, 2, depth=2, precision="bf16", group=group, steps_per_launch=2)
            monkeypatch.setenv("BBB_FORCE_COMBINE", "0")
            lo, _ = ens.mc_forward(net, x, 2, group=group, precision="bf16")       # one rank, nothing sharded: runs
            assert lo.shape == (16, 10)
            monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
            with pytest.raises(err, match="one device"):
                ens.mc_forward(net, x, 2, group=group, precision="bf16")
            with pytest.raises(err, match="one device"):
                ens.mc_forward_batch_parallel(net, x, 2, group=group, precision="bf16")
            with pytest.raises(err, match="one device"):
                ens.GraphedMC(net, x, 2, precision="bf16", group=group)
    finally:
        monkeypatch.undo()
        dist.destroy_process_group()
    rng.use_device_generator()


def test_kernel_entry_refusals(env):
    ops, err = env["ops"], env["lib"].BBBHipError
    # the kernel entry: no per-draw weights, no sample with a moments-only launch
    xb = torch.zeros(1, 8, 4, 4, 8, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(16, 72, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(err):
        ops.lrt_conv2d_chwn_bf16_forward(xb, w, w[:, :64], None, None, (8, 3, 3), 1, 0, 2)
    with pytest.raises(err):
        ops.lrt_conv2d_chwn_bf16_forward(xb, w, w, None, None, (8, 3, 3), 1, 0, 2, tap_major=False, moments_only=True, sample=True)
