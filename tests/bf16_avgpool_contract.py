"""Test-side restatement of the bf16 training contract for models with average pools, in float64 torch on
the CPU: bf16_train_contract.step_grads with one more kind of pool.  A layer's pool is None, a max pool (k, s) or an average pool
(kernel, stride, padding, count_include_pad) -- pairs and a bool, pool_desc.avgpool_of's tuple.

What an average pool adds to the contract:
  * forward: the pool reads the stored (rounded) activated output; its result -- the window's sum over the divisor, float64 here,
    fp32 on the device -- is rounded ONCE to bf16 when stored (a max pool's result needs no rounding: it is one of the stored values);
  * backward: g_pre = act'(y) * route(g) with route = the average pool's own backward (every tap of a window receives the window's
    gradient over its divisor; F.avg_pool2d's autograd in float64), act' from the stored y, rounded once.
Everything else is that file's, whose pieces are imported, not restated.  rounding=False turns every rounding off: the result is
the exact float64 gradient of the step (autograd_grads, torch autograd of the same model, must give the same).
"""
import numpy as np
import torch
import torch.nn.functional as F

import bbb_numpy as O
from bf16_train_contract import F64, _act, _act_grad, _kl, _pair, _round, _route, _sample


def normal_plan(plan):
    """[dict(name, kind, stride, padding, dilation, act, pool, flat)] with per-axis geometry; pool None, (k, s) or the 4-tuple."""
    out = []
    for ent in plan:
        d = dict(ent)
        for key, default in (("stride", 1), ("padding", 0), ("dilation", 1)):
            d[key] = _pair(d.get(key, default))
        d.setdefault("act", None)
        d.setdefault("flat", None)
        p = d.get("pool")
        if p is not None and len(p) == 4:
            p = (_pair(p[0]), _pair(p[1]), _pair(p[2]), bool(p[3]))
        elif p is not None:
            p = (int(p[0]), int(p[1]))
        d["pool"] = p
        out.append(d)
    return out


def is_avg(pool):
    return pool is not None and len(pool) == 4


def pool_fwd(y, pool):
    if is_avg(pool):
        return F.avg_pool2d(y, pool[0], pool[1], pool[2], ceil_mode=False, count_include_pad=pool[3])
    return F.max_pool2d(y, *pool)


def avg_route(g, y, pool):
    """The average pool's backward through autograd (the pool is linear: y gives the shape only)."""
    t = torch.zeros_like(y).requires_grad_(True)
    (gy,) = torch.autograd.grad(pool_fwd(t, pool), t, g)
    return gy


def _lin(h, w, b, L):
    if L["kind"] == "conv":
        return F.conv2d(h, w, b, L["stride"], L["padding"], L["dilation"])
    return F.linear(h, w, b)


def forward(plan, params, x, eps, rounding=True):
    """The forward of every draw -> (tapes, [logits [B, classes]] per draw), float64 torch."""
    plan = normal_plan(plan)
    R = lambda t: _round(t, rounding)
    xin = R(torch.from_numpy(np.asarray(x, np.float32)).to(F64))
    tapes, logits = [], []
    for e in range(len(eps)):
        h, tape = xin, []
        for li, L in enumerate(plan):
            p = params[L["name"]]
            w = R(_sample(p["W_mu"], p["W_rho"], eps[e][L["name"]]["W"]))
            b = _sample(p["bias_mu"], p["bias_rho"], eps[e][L["name"]]["bias"])
            last = li == len(plan) - 1
            if L["kind"] == "fc" and h.dim() != 2:
                h = h.reshape(h.shape[0], -1)
            v = _lin(h, w, b, L)
            y = _act(v, L["act"]) if L["act"] else v
            if not last:
                y = R(y)
            out = y
            if L["pool"]:
                out = pool_fwd(y, L["pool"])
                if is_avg(L["pool"]):
                    out = R(out)                       # the one more rounding point: an average is not one of the stored values
            tape.append(dict(x=h, w=w, y=y, out_shape=tuple(out.shape)))
            h = out.reshape(out.shape[0], L["flat"]) if L["flat"] else out
        tapes.append(tape)
        logits.append(h)
    return tapes, logits


def step_grads(plan, params, x, target, eps, beta, train_size, rounding=True):
    """One training step of the contract (bf16_train_contract.step_grads' structure and return value; a plan of dicts).
    Returns (loss, log_outputs [B, C], {name: {W_mu, W_rho, bias_mu, bias_rho}} gradients), float64 numpy."""
    plan = normal_plan(plan)
    E = len(eps)
    R = lambda t: _round(t, rounding)
    pm, ps = float(params["_prior_mu"]), float(params["_prior_sigma"])
    tapes, logits = forward(plan, params, x, eps, rounding)
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
            if is_avg(pool):
                g = avg_route(g, rec["y"], pool)
            elif pool:
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
            for key, gg, rho in (("W", gw, p["W_rho"]), ("bias", gb, p["bias_rho"])):
                ep = torch.from_numpy(eps[e][name][key].astype(np.float64))
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


def autograd_grads(plan, params, x, target, eps, beta, train_size):
    """The same step (no rounding) differentiated by torch autograd in float64: what step_grads(rounding=False) must equal."""
    plan = normal_plan(plan)
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
            Lv = leaves[L["name"]]
            w = Lv["W_mu"] + torch.from_numpy(eps[e][L["name"]]["W"].astype(np.float64)) * sp(Lv["W_rho"])
            b = Lv["bias_mu"] + torch.from_numpy(eps[e][L["name"]]["bias"].astype(np.float64)) * sp(Lv["bias_rho"])
            if L["kind"] == "fc" and h.dim() != 2:
                h = h.reshape(h.shape[0], -1)
            v = _lin(h, w, b, L)
            y = _act(v, L["act"]) if L["act"] else v
            h = pool_fwd(y, L["pool"]) if L["pool"] else y
            h = h.reshape(h.shape[0], L["flat"]) if L["flat"] else h
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
    return float(loss.detach()), {n: {k: v.grad.numpy() for k, v in L.items()} for n, L in leaves.items()}
