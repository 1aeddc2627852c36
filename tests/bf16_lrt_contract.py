"""Test-side restatement of the bf16 LRT arithmetic contract on the CPU, noise as an INPUT.

For a local-reparameterisation layer with stored bf16 input x (layers/BBB_LRT/BBBConv.py:62-87, BBBLinear.py:56-79):
    act_mu  = sum x * bf16(W_mu) + b_mu
    act_var = 1e-16 + sum bf16(x^2) * bf16(sigma_W^2) + sigma_b^2
    out     = act(act_mu + sqrt(act_var) * eps)
with sigma_W^2 the fp32 value the parameter pass produces (softplus(rho)^2), rounded once; x^2 the exact square of the stored value,
rounded once; biases, the sampling step, the activation and KL unrounded; hidden outputs rounded once when stored (after the
activation; max-pooling commutes with the rounding); the input image rounded once; the logits layer unrounded.

Every contraction is accumulated in float64 (oracle.bbb_numpy.conv2d / linear) from the rounded operands; stage results are held as
fp32 exactly where the oracle's LRT model forward holds them, so that with `rounding=False` (rounding replaced by the identity)
this IS oracle.bbb_numpy.model_forward(layer_type="lrt"), value for value.  Rounding is the oracle's bf16_round."""
import numpy as np

import bbb_numpy as O

F32 = np.float32


def _rnd(a, on):
    return O.bf16_round(a) if on else np.asarray(a, F32)


def lrt_moments(h, p, kind, stride, padding, rounding=True, dilation=1):
    """(act_mu, act_var) of one layer from its stored input h (fp32 array holding bf16 values when rounding is on)."""
    h = np.asarray(h, F32)
    w_sigma = O.sigma_from_rho(p["W_rho"])
    w_mu = _rnd(p["W_mu"], rounding)
    w_var = _rnd(w_sigma * w_sigma, rounding)
    x2 = _rnd(h * h, rounding)                      # exact in fp32 for bf16 h: 8 x 8 significant bits
    b_var = None if p.get("bias_mu") is None else O.sigma_from_rho(p["bias_rho"]) ** 2
    if kind == "conv":
        am = O.conv2d(h, w_mu, p.get("bias_mu"), stride, padding, dilation)
        av = (F32(1e-16) + O.conv2d(x2, w_var, b_var, stride, padding, dilation)).astype(F32)
    else:
        am = O.linear(h, w_mu, p.get("bias_mu"))
        av = (F32(1e-16) + O.linear(x2, w_var, b_var)).astype(F32)
    return am, av


def model_forward(net_type, params, x, activation, eps_fn, rounding=True):
    """One stochastic forward of an all-LRT model under the contract -> logits (fp32).  eps_fn(name, "act", shape) returns the
    activation noise of layer `name` in the canonical [B, Cout, Ho, Wo] / [B, out] order."""
    act = O.softplus_act if activation == "softplus" else O.relu_act
    ops_ = O.TOPOLOGY[net_type]
    last = max(i for i, op in enumerate(ops_) if op[0] in ("conv", "fc"))
    h = _rnd(x, rounding)
    i = 0
    while i < len(ops_):
        op = ops_[i]
        if op[0] == "act":
            h = _rnd(act(h), rounding)
        elif op[0] == "pool":
            h = O.maxpool2d(h, op[1], op[2])
        elif op[0] == "flatten":
            h = h.reshape(-1, op[1])
        else:
            p = params[op[1]]
            if op[0] == "conv":
                am, av = lrt_moments(h, p, "conv", op[4], op[5], rounding)
            else:
                am, av = lrt_moments(h, p, "fc", 1, 0, rounding)
            y = O.lrt_output(am, av, eps_fn(op[1], "act", am.shape))
            if i + 1 < len(ops_) and ops_[i + 1][0] == "act":      # the activation is part of the launch's epilogue, in fp32
                y = act(y)
                i += 1
            h = y if i >= last else _rnd(y, rounding)
        i += 1
    return h
