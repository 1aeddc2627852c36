"""Test-side restatement of the bf16 training contract WITH the input gradient (LaunchConfig.bf16_input_grad)
in float64 torch on the CPU, and the six small models tests/test_gpu_bf16_input_grad.py differentiates.

The step is tests/bf16_train_contract.py's, rounding point for rounding point (its helpers are imported, not restated): sampled
weights, the input and every hidden activated / pooled output rounded once to bf16; the logits' gradient rounded once; every layer's
g_pre = act'(y) * route(g) from the stored y, rounded once; the gradients passed between layers rounded once.  What is added: after
the FIRST layer's g_pre (rounded once) d loss / d x is the float64 transposed convolution of that g_pre with the rounded weights,
summed over the draws, and NOT rounded -- dx is fp32 on the device, like the caller's x.
rounding=False turns every rounding off: the exact float64 d loss / d x of the step (what torch autograd gives)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import bbb_numpy as O
import ref_port_torch as P
from bf16_train_contract import F64, _act, _act_grad, _conv_fwd, _kl, _round, _route, _sample, general_plan


def step_dx(plan, params, x, target, eps, beta, train_size, rounding=True):
    """One step of the contract -> (loss, log_outputs [B, C], dx [B, Cin, H, W]), float64 numpy.  plan: a list of general_plan's dicts;
    params, x, target, eps as bf16_train_contract.step_grads takes them.  The loss's KL term does not depend on x."""
    plan = general_plan(plan)
    E = len(eps)
    R = lambda t: _round(t, rounding)
    pm, ps = float(params["_prior_mu"]), float(params["_prior_sigma"])
    x_shape = tuple(np.asarray(x).shape)
    xin = R(torch.from_numpy(np.asarray(x, np.float32)).to(F64))
    tapes, logits = [], []
    for e in range(E):
        h, tape = xin, []
        for li, L in enumerate(plan):
            name, kind, act, pool, flat = L["name"], L["kind"], L["act"], L["pool"], L["flat"]
            p = params[name]
            w = R(_sample(p["W_mu"], p["W_rho"], eps[e][name]["W"]))
            b = _sample(p["bias_mu"], p["bias_rho"], eps[e][name]["bias"])
            if kind == "fc" and h.dim() != 2:
                h = h.reshape(h.shape[0], -1)
            v = _conv_fwd(h, w, b, L) if kind == "conv" else F.linear(h, w, b)
            y = _act(v, act) if act else v
            if li != len(plan) - 1:
                y = R(y)
            out = F.max_pool2d(y, *pool) if pool else y
            tape.append(dict(x=h, w=w, y=y, out_shape=tuple(out.shape)))
            h = out.reshape(out.shape[0], flat) if flat else out
        tapes.append(tape)
        logits.append(h)
    lg = torch.stack(logits).detach().requires_grad_(True)
    lo = torch.logsumexp(F.log_softmax(lg, dim=2), dim=0) - np.log(E)
    nll = F.nll_loss(lo, torch.from_numpy(np.asarray(target, np.int64)), reduction="mean") * train_size
    kl = sum(_kl(params[L["name"]][k + "_mu"], params[L["name"]][k + "_rho"], pm, ps) for L in plan for k in ("W", "bias"))
    (g_lg,) = torch.autograd.grad(nll, lg)
    dx = torch.zeros(x_shape, dtype=F64)
    for e in range(E):
        g = R(g_lg[e])
        for li in range(len(plan) - 1, -1, -1):
            L = plan[li]
            rec = tapes[e][li]
            g = g.reshape(rec["out_shape"])
            if L["pool"]:
                g = _route(g, rec["y"], *L["pool"])
            if L["act"]:
                g = g * _act_grad(rec["y"], L["act"])
            g_pre = R(g) if (L["pool"] or L["act"]) else g
            if L["kind"] == "conv":
                gx = torch.nn.grad.conv2d_input(tuple(rec["x"].shape), rec["w"], g_pre, stride=L["stride"], padding=L["padding"],
                                                dilation=L["dilation"])
            else:
                gx = g_pre @ rec["w"]
            if li > 0:
                g = R(gx)
            else:
                dx += gx.reshape(x_shape)                    # the first layer: summed over the draws, never rounded
    return float(nll.detach()) + beta * kl, lo.detach().numpy(), dx.numpy()


def autograd_dx(plan, params, x, target, eps, train_size):
    """The same step without roundings, differentiated in x by torch autograd in float64: what step_dx(rounding=False) must equal."""
    plan = general_plan(plan)
    E = len(eps)
    xin = torch.from_numpy(np.asarray(x, np.float32)).to(F64).requires_grad_(True)
    logits = []
    for e in range(E):
        h = xin
        for L in plan:
            p = params[L["name"]]
            w = _sample(p["W_mu"], p["W_rho"], eps[e][L["name"]]["W"])
            b = _sample(p["bias_mu"], p["bias_rho"], eps[e][L["name"]]["bias"])
            if L["kind"] == "fc" and h.dim() != 2:
                h = h.reshape(h.shape[0], -1)
            v = _conv_fwd(h, w, b, L) if L["kind"] == "conv" else F.linear(h, w, b)
            y = _act(v, L["act"]) if L["act"] else v
            h = F.max_pool2d(y, *L["pool"]) if L["pool"] else y
            h = h.reshape(h.shape[0], L["flat"]) if L["flat"] else h
        logits.append(h)
    lo = torch.logsumexp(F.log_softmax(torch.stack(logits), dim=2), dim=0) - np.log(E)
    (F.nll_loss(lo, torch.from_numpy(np.asarray(target, np.int64)), reduction="mean") * train_size).backward()
    return xin.grad.numpy()


# ---- the six models: name -> (input shape (C, H, W), layers) with a layer (kind, cout, kernel, stride, padding, dilation, act, pool) ----
MODELS = {
    "M1": ((3, 16, 16), [("conv", 8, 5, 2, 2, 1, "softplus", (2, 2))]),
    "M2": ((3, 16, 16), [("conv", 16, 11, 4, 5, 1, "relu", None)]),
    "M3": ((8, 8, 8), [("conv", 16, 3, 1, 1, 1, "relu", (2, 2))]),
    "M4": ((3, 4, 4), [("fc", 24, 1, 1, 0, 1, "softplus", None)]),
    "M5": ((3, 9, 13), [("conv", 12, (2, 3), (3, 2), (1, 0), (1, 2), "softplus", None)]),
    "M6": ((1, 16, 16), [("conv", 6, 5, 1, 0, 1, "relu", (2, 2))]),
}
FLAT = {"M1": 128, "M2": 256, "M3": 256, "M4": 24, "M5": 240, "M6": 216}      # what the classifier reads (the issue's numbers)


def build(name):
    """-> (net on the CPU (BBB layers, ModuleWrapper), plan of dicts for step_dx / autograd_dx, input shape (C, H, W))."""
    from layers import BBB_Conv2d, BBB_Linear, FlattenLayer, ModuleWrapper
    (C, H, W), layers = MODELS[name]
    net, plan = ModuleWrapper(), []
    cin = C
    for i, (kind, cout, k, st, pd, dl, act, pool) in enumerate(layers):
        lname = f"{kind}{i}"
        if kind == "conv":
            net.add_module(lname, BBB_Conv2d(cin, cout, k, stride=st, padding=pd, dilation=dl, bias=True, priors=P.CONFIG_PRIORS))
            H, W = _out_hw(H, W, k, st, pd, dl)
        else:
            net.add_module("flatten_in", FlattenLayer(cin * H * W))
            net.add_module(lname, BBB_Linear(cin * H * W, cout, bias=True, priors=P.CONFIG_PRIORS))
            H = W = 1
        net.add_module(f"act{i}", nn.Softplus() if act == "softplus" else nn.ReLU())
        if pool is not None:
            net.add_module(f"pool{i}", nn.MaxPool2d(*pool))
            H, W = (H - pool[0]) // pool[1] + 1, (W - pool[0]) // pool[1] + 1
        cin = cout
        plan.append(dict(name=lname, kind=kind, stride=st, padding=pd, dilation=dl, act=act, pool=pool, flat=None))
    feat = cin * H * W
    assert feat == FLAT[name], (name, feat)
    if layers[-1][0] == "conv":
        net.add_module("flatten", FlattenLayer(feat))
        plan[-1]["flat"] = feat
    net.add_module("fc_out", BBB_Linear(feat, 10, bias=True, priors=P.CONFIG_PRIORS))
    plan.append(dict(name="fc_out", kind="fc", stride=1, padding=0, dilation=1, act=None, pool=None, flat=None))
    return net, plan, MODELS[name][0]


def _out_hw(H, W, k, st, pd, dl):
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(st), pair(pd), pair(dl)
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def numpy_params(net):
    """name -> {W_mu, W_rho, bias_mu, bias_rho} (numpy fp32) + the prior, as step_dx reads them."""
    out = {"_prior_mu": P.CONFIG_PRIORS["prior_mu"], "_prior_sigma": P.CONFIG_PRIORS["prior_sigma"]}
    for n, m in net.named_modules():
        if hasattr(m, "W_mu"):
            out[n] = {k: getattr(m, k).detach().cpu().numpy() for k in ("W_mu", "W_rho", "bias_mu", "bias_rho")}
    return out


def device_eps(net, plan, npar, seed, call0, E):
    """The noise the device draws for calls call0 .. call0 + E - 1 (oracle.normal_eps on the layers' stream ids)."""
    mods = dict(net.named_modules())
    return [{L["name"]: {kind: O.normal_eps(seed, call0 + e, mods[L["name"]]._stream_base + off,
                                            int(np.prod(npar[L["name"]][key].shape))).reshape(npar[L["name"]][key].shape)
                         for kind, key, off in (("W", "W_mu", 0), ("bias", "bias_mu", 1))} for L in plan} for e in range(E)]
