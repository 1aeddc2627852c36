"""The test-side restatement of the bf16 training contract (tests/bf16_train_contract.py) checked against torch autograd before it
judges any kernel: with its rounding switched off, its hand-written backward must be the exact float64 gradient of the step.
CPU only (float64 torch): every topology of the zoo, both activations, overlapping (3 / 2) and plain (2 / 2) pooling."""
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
