"""The test-side restatement of the bf16 training contract (tests/bf16_train_contract.py) checked against torch autograd before it
judges any kernel: with its rounding switched off, its hand-written backward must be the exact float64 gradient of the step.
CPU only (float64 torch): every topology of the zoo, both activations, overlapping (3 / 2) and plain (2 / 2) pooling, and the
generated layer plans of test_gpu_bf16_train_fuzz.py (dilation, non-square kernels, any (k, s) pool, linear first layers)."""
import numpy as np
import pytest
import torch

import bf16_train_contract as C
import ref_port_torch as P


def _eps(net_type, params, E, rs):
    return [{n: {"W": rs.standard_normal(params[n]["W_mu"].shape), "bias": rs.standard_normal(params[n]["bias_mu"].shape)}
             for n, *_ in C.layer_plan(net_type)} for _ in range(E)]


@pytest.mark.parametrize("net_type,cin,activation", [("lenet", 1, "softplus"), ("lenet", 3, "relu"), ("3conv3fc", 3, "softplus"),
                                                     ("3conv3fc", 3, "relu"), ("alexnet", 3, "softplus")])
def test_manual_backward_equals_autograd_without_rounding(net_type, cin, activation):
    torch.manual_seed(3)
    params = {n: {k: v.numpy() for k, v in p.items()} if isinstance(p, dict) else p
              for n, p in P.init_params(net_type, cin, 10, P.CONFIG_PRIORS).items()}
    rs = np.random.default_rng(5)
    B, E = 3, 2
    x = rs.random((B, cin, 32, 32), dtype=np.float32)
    y = rs.integers(0, 10, B)
    eps = _eps(net_type, params, E, rs)
    loss, _, got = C.step_grads(net_type, params, x, y, eps, activation, 0.1, 500.0, rounding=False)
    loss_ref, want = C.autograd_grads(net_type, params, x, y, eps, activation, 0.1, 500.0)
    assert abs(loss - loss_ref) <= 1e-9 * abs(loss_ref)
    for n in want:
        for k in want[n]:
            scale = float(np.abs(want[n][k]).max())
            err = float(np.abs(got[n][k] - want[n][k]).max())
            assert err <= 1e-9 * scale, (n, k, err, scale)


def test_rounding_points_change_the_result_by_bf16_amounts():
    """With rounding on, the same step moves by bf16-sized (not fp32-sized, not arbitrary) amounts: the switch is live."""
    torch.manual_seed(4)
    params = {n: {k: v.numpy() for k, v in p.items()} if isinstance(p, dict) else p
              for n, p in P.init_params("lenet", 1, 10, P.CONFIG_PRIORS).items()}
    rs = np.random.default_rng(6)
    x = rs.random((4, 1, 32, 32), dtype=np.float32)
    y = rs.integers(0, 10, 4)
    eps = _eps("lenet", params, 2, rs)
    _, _, g64 = C.step_grads("lenet", params, x, y, eps, "softplus", 0.1, 500.0, rounding=False)
    _, _, g16 = C.step_grads("lenet", params, x, y, eps, "softplus", 0.1, 500.0, rounding=True)
    rel = max(float(np.abs(g16[n]["W_mu"] - g64[n]["W_mu"]).max() / np.abs(g64[n]["W_mu"]).max()) for n in g64)
    assert 1e-5 < rel < 5e-2, rel


def _fuzz_models():
    import test_gpu_bf16_train_fuzz as T
    return T


@pytest.mark.parametrize("name", list(_fuzz_models().MODELS))
def test_manual_backward_equals_autograd_on_generated_plans(name):
    """The same check on the generated models of test_gpu_bf16_train_fuzz.py: per-axis stride / padding / dilation, any (k, s)
    pool, an activation per layer, flatten points, linear first layers."""
    T = _fuzz_models()
    spec = T.MODELS[name]
    net = T._build(spec, 11)
    plan = T.model_plan(spec)
    mods = dict(net.named_modules())
    params = {L["name"]: {k: getattr(mods[L["name"]], k).detach().numpy() for k in ("W_mu", "W_rho", "bias_mu", "bias_rho")}
              for L in plan}
    params["_prior_mu"], params["_prior_sigma"] = mods["l0"].prior_mu, mods["l0"].prior_sigma
    rs = np.random.default_rng(7)
    B, E = 3, spec["E"]
    x = rs.random((B, spec["Cin"], spec["H"], spec["W"]), dtype=np.float32)
    y = rs.integers(0, 10, B)
    eps = [{L["name"]: {"W": rs.standard_normal(params[L["name"]]["W_mu"].shape),
                        "bias": rs.standard_normal(params[L["name"]]["bias_mu"].shape)} for L in plan} for _ in range(E)]
    # the plan describes the module: its forward (no noise: eps = 0) is the model's own
    with torch.no_grad():
        from layers.bbb import _BBBLayer
        h = torch.from_numpy(x).double()
        net64 = net.double()
        for m in net64.children():
            if isinstance(m, _BBBLayer):
                h = (torch.nn.functional.conv2d(h, m.W_mu, m.bias_mu, m.stride, m.padding, m.dilation) if hasattr(m, "kernel_size")
                     else torch.nn.functional.linear(h.reshape(h.shape[0], -1), m.W_mu, m.bias_mu))
            else:
                h = m(h)
        want_logits = h
    zero = [{n: {k: np.zeros_like(v) for k, v in d.items()} for n, d in eps[0].items()}]
    _, lo0, _ = C.step_grads(plan, params, x, y, zero, None, 0.1, 500.0, rounding=False)
    assert np.allclose(lo0, torch.log_softmax(want_logits, dim=1).numpy(), rtol=0, atol=1e-9)
    loss, _, got = C.step_grads(plan, params, x, y, eps, None, 0.1, 500.0, rounding=False)
    loss_ref, want = C.autograd_grads(plan, params, x, y, eps, None, 0.1, 500.0)
    assert abs(loss - loss_ref) <= 1e-9 * abs(loss_ref)
    for n in want:
        for k in want[n]:
            scale = float(np.abs(want[n][k]).max())
            err = float(np.abs(got[n][k] - want[n][k]).max())
            assert err <= 1e-9 * scale, (n, k, err, scale)


def test_layer_plan_of_a_net_type_is_unchanged():
    """layer_plan(net_type) keeps its tuples; general_plan reads them with the net's activation and unit dilations."""
    plan = C.layer_plan("lenet")
    assert all(isinstance(t, tuple) and len(t) == 7 for t in plan)
    g = C.general_plan("lenet", "relu")
    assert [L["name"] for L in g] == [t[0] for t in plan]
    for t, L in zip(plan, g):
        assert L["act"] == ("relu" if t[4] else None) and L["dilation"] == (1, 1) and L["pool"] == t[5] and L["flat"] == t[6]
