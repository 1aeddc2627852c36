"""Test-side restatement of the bf16 training contract ("bf16 training") in float64 torch on the CPU:
one training step's forward AND its backward, written out layer by layer by hand (no autograd through the layers), with the
contract's rounding points switchable.

Forward (the bf16 inference path's rounding points, oracle.model_forward_bf16): sampled weights rounded once to bf16
(nearest-even); the input image and every hidden activated / pooled output rounded to bf16; accumulation, bias, activation,
logits, KL and the ELBO tail in float64 here (fp32 on the device).
Backward:
  * the logits' gradient (ELBO tail, float64) rounded once to bf16 = the logits layer's output gradient;
  * every layer: g_pre = act'(y) * route(g) from the STORED (rounded) activated output y -- Softplus' = 1 - exp(-y) (1 above 20),
    ReLU' = [y > 0]; max-pool routing to the first maximum among the stored values (torch's max_pool2d order) -- rounded once;
  * weight gradient = the contraction of the rounded g_pre with the rounded layer input, never rounded; bias gradient = the sum of
    the same rounded g_pre; input gradient = the contraction of g_pre with the rounded weights, rounded once;
  * parameter gradients: d/d mu = sum over draws of the weight gradients, d/d rho = sum of (weight gradient * eps) * sigmoid(rho),
    plus beta * the KL's own gradients (the reference's swapped KL form, oracle.bbb_numpy.kl_grads).
rounding=False turns every rounding off: the result is then the exact float64 gradient of the step (what torch autograd gives).
"""
import numpy as np
import torch
import torch.nn.functional as F

import bbb_numpy as O

F64 = torch.float64


def _round(t, on):
    return t.to(torch.float32).to(torch.bfloat16).to(F64) if on else t


def _act(v, kind):
    return F.relu(v) if kind == "relu" else torch.where(v > 20, v, torch.log1p(torch.exp(torch.clamp(v, max=20.0))))


def _act_grad(y, kind):
    """act' written from the activated output alone."""
    if kind == "relu":
        return (y > 0).to(F64)
    return torch.where(y > 20, torch.ones_like(y), -torch.expm1(-y))


def _sample(mu, rho, eps):
    """mu + softplus(rho) * eps in float64 (the device forms it in fp32; the difference is far below a bf16 rounding)."""
    return torch.from_numpy(mu.astype(np.float64)) + torch.from_numpy(np.asarray(eps, np.float64)) * \
        torch.log1p(torch.exp(torch.from_numpy(rho.astype(np.float64))))


def _kl(mu, rho, pm, ps):
    """The reference's KL (swapped form, oracle.bbb_numpy.kl_elements) in float64."""
    mu, s = mu.astype(np.float64), np.log1p(np.exp(rho.astype(np.float64)))
    return float(np.sum(0.5 * (2.0 * np.log(s / ps) - 1.0 + (ps / s) ** 2 + ((mu - pm) / s) ** 2)))


def _route(g, y, k, s):
    """max_pool2d(k, s) backward: g to the first maximum of every window of y (torch's order), overlapping windows summed."""
    yy = y.detach().clone().requires_grad_(True)
    out = F.max_pool2d(yy, k, s)
    (gy,) = torch.autograd.grad(out, yy, g)
    return gy


def layer_plan(net_type):
    """[(name, kind, stride, padding, act_follows, pool or None, flatten_to or None)] from the oracle's topology table."""
    ops_ = O.TOPOLOGY[net_type]
    plan = []
    for i, op in enumerate(ops_):
        if op[0] not in ("conv", "fc"):
            continue
        act = i + 1 < len(ops_) and ops_[i + 1][0] == "act"
        j = i + (2 if act else 1)
        pool = (ops_[j][1], ops_[j][2]) if j < len(ops_) and ops_[j][0] == "pool" else None
        j += 1 if pool else 0
        flat = ops_[j][1] if j < len(ops_) and ops_[j][0] == "flatten" else None
        stride, pad = (op[4], op[5]) if op[0] == "conv" else (1, 0)
        plan.append((op[1], op[0], stride, pad, act, pool, flat))
    return plan


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(t) for t in v)


def general_plan(plan, activation=None):
    """A layer plan in its general form: [dict(name, kind, stride, padding, dilation, act, pool, flat)] with per-axis (h, w)
    stride / padding / dilation, act None / "relu" / "softplus" per layer, pool (k, s) or None, flat = the row length a
    FlattenLayer after the layer (and its pool) keeps, or None.  A linear layer whose input is still 4-d (a first layer behind a
    FlattenLayer) flattens it first.  plan: a net_type (layer_plan, every activation = `activation`), a list of layer_plan's
    tuples (likewise), or a list of such dicts (stride / padding / dilation may be ints; dilation defaults to 1)."""
    if isinstance(plan, str):
        plan = layer_plan(plan)
    out = []
    for ent in plan:
        if isinstance(ent, dict):
            d = dict(ent)
            d.setdefault("dilation", 1)
            d.setdefault("act", None)
            d.setdefault("pool", None)
            d.setdefault("flat", None)
        else:
            name, kind, stride, pad, act, pool, flat = ent
            d = dict(name=name, kind=kind, stride=stride, padding=pad, dilation=1, act=activation if act else None, pool=pool,
                     flat=flat)
        for key in ("stride", "padding", "dilation"):
            d[key] = _pair(d[key])
        d["pool"] = None if d["pool"] is None else (int(d["pool"][0]), int(d["pool"][1]))
        out.append(d)
    return out


def _conv_fwd(h, w, b, L):
    return F.conv2d(h, w, b, L["stride"], L["padding"], L["dilation"])


def step_grads(plan, params, x, target, eps, activation, beta, train_size, rounding=True):
    """One training step of the contract.  plan: a net_type or a layer plan (general_plan); activation: the activation of a
    net_type's / layer_plan tuples' layers (a plan of dicts names its own).  params: name -> {W_mu, W_rho, bias_mu, bias_rho}
    (numpy fp32) + '_prior_mu', '_prior_sigma'; eps: a list over draws of name -> {'W': ..., 'bias': ...} (numpy); x [B, C, H, W],
    target [B] (numpy).  Returns (loss, log_outputs [B, C], {name: {W_mu, W_rho, bias_mu, bias_rho}} gradients), float64 numpy."""
    plan = general_plan(plan, activation)
    E = len(eps)
    R = lambda t: _round(t, rounding)
    pm, ps = float(params["_prior_mu"]), float(params["_prior_sigma"])
    xin = R(torch.from_numpy(np.asarray(x, np.float32)).to(F64))
    tapes, logits = [], []
    for e in range(E):
        h, tape = xin, []
        for li, L in enumerate(plan):
            name, kind, act, pool, flat = L["name"], L["kind"], L["act"], L["pool"], L["flat"]
            p = params[name]
            w = R(_sample(p["W_mu"], p["W_rho"], eps[e][name]["W"]))
            b = _sample(p["bias_mu"], p["bias_rho"], eps[e][name]["bias"])
            last = li == len(plan) - 1
            if kind == "fc" and h.dim() != 2:
                h = h.reshape(h.shape[0], -1)
            v = _conv_fwd(h, w, b, L) if kind == "conv" else F.linear(h, w, b)
            y = _act(v, act) if act else v
            if not last:
                y = R(y)
            out = F.max_pool2d(y, *pool) if pool else y
            tape.append(dict(x=h, w=w, y=y, out_shape=tuple(out.shape)))
            h = out.reshape(out.shape[0], flat) if flat else out
        tapes.append(tape)
        logits.append(h)
    # the ELBO tail: log_softmax per draw, logmeanexp over draws, nll_loss(mean) * train_size + beta * kl
    lg = torch.stack(logits).detach().requires_grad_(True)
    lo = torch.logsumexp(F.log_softmax(lg, dim=2), dim=0) - np.log(E)
    nll = F.nll_loss(lo, torch.from_numpy(np.asarray(target, np.int64)), reduction="mean") * train_size
    kl = sum(_kl(params[L["name"]][k + "_mu"], params[L["name"]][k + "_rho"], pm, ps) for L in plan for k in ("W", "bias"))
    loss = float(nll.detach()) + beta * kl
    (g_lg,) = torch.autograd.grad(nll, lg)
    grads = {L["name"]: dict(W_mu=0.0, W_rho=0.0, bias_mu=0.0, bias_rho=0.0) for L in plan}
    for e in range(E):
        g = R(g_lg[e])
        for li in range(len(plan) - 1, -1, -1):
            L = plan[li]
            name, kind, act, pool = L["name"], L["kind"], L["act"], L["pool"]
            geom = dict(stride=L["stride"], padding=L["padding"], dilation=L["dilation"])
            rec = tapes[e][li]
            g = g.reshape(rec["out_shape"])
            if pool:
                g = _route(g, rec["y"], *pool)
            if act:
                g = g * _act_grad(rec["y"], act)
            g_pre = R(g) if (pool or act) else g
            if kind == "conv":
                gw = torch.nn.grad.conv2d_weight(rec["x"], tuple(rec["w"].shape), g_pre, **geom)
                gb = g_pre.sum(dim=(0, 2, 3))
            else:
                gw = g_pre.t() @ rec["x"]
                gb = g_pre.sum(dim=0)
            p = params[name]
            for key, gg, rho, ek in (("W", gw, p["W_rho"], "W"), ("bias", gb, p["bias_rho"], "bias")):
                ep = torch.from_numpy(eps[e][name][ek].astype(np.float64))
                sgm = torch.sigmoid(torch.from_numpy(rho.astype(np.float64)))
                grads[name][key + "_mu"] = grads[name][key + "_mu"] + gg.numpy()
                grads[name][key + "_rho"] = grads[name][key + "_rho"] + (gg * ep * sgm).numpy()
            if li > 0:
                if kind == "conv":
                    gx = torch.nn.grad.conv2d_input(tuple(rec["x"].shape), rec["w"], g_pre, **geom)
                else:
                    gx = g_pre @ rec["w"]
                g = R(gx)
    for L in plan:
        p = params[L["name"]]
        for key in ("W", "bias"):
            gm, gr = O.kl_grads(p[key + "_mu"], p[key + "_rho"], pm, ps)
            grads[L["name"]][key + "_mu"] = grads[L["name"]][key + "_mu"] + beta * gm
            grads[L["name"]][key + "_rho"] = grads[L["name"]][key + "_rho"] + beta * gr
    return loss, lo.detach().numpy(), grads


def autograd_grads(plan, params, x, target, eps, activation, beta, train_size):
    """The same step (no rounding) differentiated by torch autograd in float64: what step_grads(rounding=False) must equal."""
    plan = general_plan(plan, activation)
    E = len(eps)
    pm, ps = float(params["_prior_mu"]), float(params["_prior_sigma"])
    leaves = {L["name"]: {k: torch.from_numpy(params[L["name"]][k].astype(np.float64)).requires_grad_(True)
                          for k in ("W_mu", "W_rho", "bias_mu", "bias_rho")} for L in plan}
    sp = lambda r: torch.log1p(torch.exp(r))
    xin = torch.from_numpy(np.asarray(x, np.float32)).to(F64)
    logits = []
    for e in range(E):
        h = xin
        for L in plan:
            name, kind, act, pool, flat = L["name"], L["kind"], L["act"], L["pool"], L["flat"]
            Lv = leaves[name]
            w = Lv["W_mu"] + torch.from_numpy(eps[e][name]["W"].astype(np.float64)) * sp(Lv["W_rho"])
            b = Lv["bias_mu"] + torch.from_numpy(eps[e][name]["bias"].astype(np.float64)) * sp(Lv["bias_rho"])
            if kind == "fc" and h.dim() != 2:
                h = h.reshape(h.shape[0], -1)
            v = _conv_fwd(h, w, b, L) if kind == "conv" else F.linear(h, w, b)
            y = _act(v, act) if act else v
            h = F.max_pool2d(y, *pool) if pool else y
            h = h.reshape(h.shape[0], flat) if flat else h
        logits.append(h)
    lo = torch.logsumexp(F.log_softmax(torch.stack(logits), dim=2), dim=0) - np.log(E)
    kl = 0.0
    for n in leaves:
        for key in ("W", "bias"):
            s = sp(leaves[n][key + "_rho"])
            t = 2.0 * torch.log(s / ps) - 1.0 + (ps / s) ** 2 + ((leaves[n][key + "_mu"] - pm) / s) ** 2
            kl = kl + 0.5 * t.sum()
    loss = F.nll_loss(lo, torch.from_numpy(np.asarray(target, np.int64)), reduction="mean") * train_size + beta * kl
    loss.backward()
    return float(loss), {n: {k: v.grad.numpy() for k, v in L.items()} for n, L in leaves.items()}
