"""Test-side restatement of the bf16 LRT input-gradient contract (LaunchConfig.bf16_lrt_input_grad) in float64
torch on the CPU.  Two things:

  * lrt_pass: the pooling / activation backward of a local-reparameterisation layer on GIVEN operands (the stored output y, act_var,
    the noise eps, the incoming gradient or the two input gradients of the layer above with this layer's output) -- what
    bbb_lrt_pool_act_bwd_chwn_bf16 computes, unrounded, with the sum of the absolute values of the terms that form each element (the
    combine d1 + 2 x d2 can cancel: a test charges the kernel's fp32 arithmetic against that sum, not against the result);
  * walk_dx: the whole backward walk of fast_train._MCForwardLRTBF16 FROM A DEVICE TAPE (tape_to_cpu: every layer's stored y, act_var
    and bf16 weight rows, the noise from ops.eps_dump) and the logits' gradient -- only the backward's arithmetic is restated, so a
    rounding that flips in the forward cannot enter.  Rounding points: g_mu and g_var when stored, d1 and d2 when stored; dx never.

No device forward is restated here: the walk starts from the tape (the forward's contract and its restatement are
tests/bf16_lrt_contract.py's, held to the device by tests/test_gpu_bf16_lrt.py); the routing and act' are
tests/bf16_train_contract.py's.  cpu_forward is a float64 forward of the same layer that records such a tape without a device.
Everything here is NCHW per draw: a device tensor [E, C, H, W, B] is read as [E, B, C, H, W]."""
import numpy as np
import torch
import torch.nn.functional as F

from bf16_train_contract import F64, _act_grad, _round, _route


def lrt_pass(g, y, av, eps, k, s, act, combine=None):
    """-> (g_mu, g_var, a_mu, a_var), float64, unrounded.  g: the gradient w.r.t. the (pooled) output [N, C, Hp, Wp]; combine =
    (x_out, d2): the incoming gradient is g + 2 * x_out * d2.  y: the stored activated output [N, C, H, W] (None: no activation and
    no pool); av, eps [N, C, H, W]; k, s: MaxPool2d(k, s), k = 0 none; act None / "relu" / "softplus".
        g_act = route(incoming) to the first maximum of every window of y;  g_mu = g_act * act'(y);  g_var = g_mu * eps / (2 sqrt(av))
    a_mu / a_var: the same expressions over the absolute values of the incoming gradient's terms (|g| + |2 x_out d2|)."""
    gin, gabs = g, g.abs()
    if combine is not None:
        t = 2.0 * combine[0] * combine[1]
        gin, gabs = g + t, g.abs() + t.abs()
    if k:
        gin, gabs = _route(gin, y, k, s), _route(gabs, y, k, s)
    d = _act_grad(y, act) if act else torch.ones_like(gin)
    scale = eps / (2.0 * torch.sqrt(av))
    g_mu = gin * d
    return g_mu, g_mu * scale, gabs * d.abs(), gabs * d.abs() * scale.abs()


def bf16_ulp(v):
    """One unit in the last place of bf16 at |v| (8 significant bits), float64; the smallest normal binade below that."""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 7)


def rows_to_weight(rows, wshape, tap_major):
    """bf16 GEMM rows [Cout, Kp] (ops.lrt_weights_bf16: (ci, r, q) column order, or tap-major (r, q, ci)) -> float64 [Cout, Cin, kh, kw]."""
    cout, cin, kh, kw = wshape
    w = rows.detach().cpu().to(F64)[:, :cin * kh * kw]
    if tap_major:
        return w.reshape(cout, kh * kw, cin).permute(0, 2, 1).reshape(cout, cin, kh, kw).contiguous()
    return w.reshape(cout, cin, kh, kw)


def _nchw(t):
    """device [E, C, H, W, B] -> float64 CPU [E, B, C, H, W]"""
    return t.detach().cpu().to(F64).permute(0, 4, 1, 2, 3).contiguous()


def tape_to_cpu(tape, seed, call0, E):
    """fast_train._lrt_bf16_forward's tape -> a list of float64 CPU records: x [E|1, B, Cin, H, W], y [E, B, C, H, W] (None for the
    logits layer: fp32 output, no activation, no pool), av [E|1, ...], eps [E, B, C, H, W] (ops.eps_dump: draw e under call0 + e, the
    layer's stream, the canonical NCHW index), w_mu / w_var [Cout, Cin, kh, kw], geom, act, pool (k, s) or None, out_shape (of one
    draw, NCHW)."""
    from bbb_hip import ops
    out = []
    for rec in tape:
        _, C, H, W, B = rec["y"].shape
        tapm = ops.bf16_tap_major(rec["wshape"])
        eps = torch.stack([ops.eps_dump(B * C * H * W, seed, call0 + e, rec["sid"], rec["y"].device).cpu().to(F64).reshape(B, C, H, W)
                           for e in range(E)])
        sh = rec["out_shape"]
        pool = None if rec["pool"] is None else (int(rec["pool"][0]), int(rec["pool"][1]))
        out.append(dict(x=_nchw(rec["x"]), y=_nchw(rec["y"]) if rec["y"].dtype == torch.bfloat16 else None, av=_nchw(rec["av"]), eps=eps,
                        w_mu=rows_to_weight(rec["w_mu"], rec["wshape"], tapm), w_var=rows_to_weight(rec["w_var"], rec["wshape"], tapm),
                        geom=rec["geom"], act=rec["act"], pool=pool, out_shape=(sh[4], sh[1], sh[2], sh[3])))
    return out


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(t) for t in v)


def _dgrad(x_shape, w, g, geom):
    st, pd, dl = (_pair(v) for v in geom)
    return torch.nn.grad.conv2d_input(x_shape, w, g, stride=st, padding=pd, dilation=dl)


def walk_dx(tape, g_logits, x_b, rounding=True):
    """The backward walk -> dx [B, Cin, H, W] float64 (x_b's shape).  tape: tape_to_cpu's records; g_logits [E, C, B] (the gradient
    w.r.t. the node's batch-innermost logits); x_b: the bf16-rounded input the forward multiplied.  Per draw, from the top: lrt_pass
    (the layer above's d1 / d2 combined with this layer's output there), g_mu and g_var rounded once; below the first layer
    d1 = dgrad(g_mu, W_mu), d2 = dgrad(g_var, sigma^2), each rounded once; at the first layer
    dx = sum_e T(g_mu, W_mu) + 2 x_b * sum_e T(g_var, sigma^2), never rounded.  rounding=False: the exact gradient of the recorded
    forward (what torch autograd gives)."""
    R = lambda t: _round(t, rounding)
    g_logits = torch.as_tensor(g_logits).detach().cpu().to(F64)
    x_b = torch.as_tensor(x_b).detach().cpu().to(F64)
    E = g_logits.shape[0]
    t_mu = t_var = None
    for e in range(E):
        g, comb = g_logits[e].t().contiguous(), None
        for li in range(len(tape) - 1, -1, -1):
            rec = tape[li]
            g = g.reshape(rec["out_shape"])
            if comb is not None:
                comb = (comb[0].reshape(rec["out_shape"]), comb[1].reshape(rec["out_shape"]))
            k, s = rec["pool"] if rec["pool"] else (0, 1)
            y = None if rec["y"] is None else rec["y"][e]
            g_mu, g_var, _, _ = lrt_pass(g, y, rec["av"][e % rec["av"].shape[0]], rec["eps"][e], k, s, rec["act"], combine=comb)
            g_mu, g_var = R(g_mu), R(g_var)
            x_in = rec["x"][e % rec["x"].shape[0]]
            if li > 0:
                d1, d2 = R(_dgrad(tuple(x_in.shape), rec["w_mu"], g_mu, rec["geom"])), R(_dgrad(tuple(x_in.shape), rec["w_var"], g_var, rec["geom"]))
                g, comb = d1, (x_in, d2)
            else:
                a, b = _dgrad(tuple(x_in.shape), rec["w_mu"], g_mu, rec["geom"]), _dgrad(tuple(x_in.shape), rec["w_var"], g_var, rec["geom"])
                t_mu, t_var = (a, b) if t_mu is None else (t_mu + a, t_var + b)
    return (t_mu.reshape(x_b.shape) + 2.0 * x_b * t_var.reshape(x_b.shape)).numpy()


# ---- a forward in float64 that records such a tape (no device): what walk_dx(rounding=False) must differentiate exactly ----
def cpu_forward(layers, x, eps, rounding=False):
    """layers: dicts (kind "conv" / "fc", w_mu, w_var [Cout, Cin, kh, kw] float64, b_mu, b_var [Cout], geom, act, pool) -> (tape,
    logits [E, C, B]) with x [B, Cin, H, W] float64 and eps[e][li] of the layer's pre-pool output shape; act(mu + sqrt(var) * eps),
    var = 1e-16 + conv(x^2, w_var) + b_var, max pools, NCHW flattening in front of a linear layer.  Differentiable in x."""
    from bf16_train_contract import _act
    E = len(eps)
    tape = [dict(x=[], y=[], av=[], eps=[], w_mu=L["w_mu"], w_var=L["w_var"], geom=L["geom"], act=L["act"], pool=L["pool"]) for L in layers]
    logits = []
    for e in range(E):
        h = x
        for li, L in enumerate(layers):
            if L["kind"] == "fc":
                h = h.reshape(h.shape[0], -1, 1, 1)
            st, pd, dl = (_pair(v) for v in L["geom"])
            am = F.conv2d(h, L["w_mu"], L["b_mu"], st, pd, dl)
            av = 1e-16 + F.conv2d(h * h, L["w_var"], L["b_var"], st, pd, dl)
            y = am + torch.sqrt(av) * eps[e][li]
            y = _act(y, L["act"]) if L["act"] else y
            out = F.max_pool2d(y, *L["pool"]) if L["pool"] else y
            rec = tape[li]
            rec["x"].append(h.detach()); rec["y"].append(y.detach()); rec["av"].append(av.detach()); rec["eps"].append(eps[e][li])
            rec["out_shape"] = tuple(out.shape)
            h = out
        logits.append(h.reshape(h.shape[0], -1).t())
    for li, rec in enumerate(tape):
        for key in ("x", "y", "av", "eps"):
            rec[key] = torch.stack(rec[key])
        if li == len(tape) - 1:
            rec["y"] = None
    return tape, torch.stack(logits)
