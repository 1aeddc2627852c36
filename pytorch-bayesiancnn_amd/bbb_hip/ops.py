"""Tensor-level entry points over the C ABI + their autograd wiring.

Forward math is entirely in the HIP kernels.  Backward (training extension): the parameter pass
has its own fused HIP kernel (eps regenerated from the counter, never stored); conv / linear weight gradients and input
gradients run on the SAME fp32-MFMA implicit-GEMM kernel as the forward (wgrad = the axis-swapped convolution, dgrad = the
flipped-weight convolution of the stride-upsampled output gradient) -- no ATen / MIOpen / rocBLAS convolution or GEMM
anywhere.  Activations, pooling and the loss tail use torch autograd (element-wise ops) in this mode.
"""
import collections
import contextlib
import ctypes
import math
import os
import itertools
import sys
import threading
import types
import weakref

import torch

from . import _lib, rng
from ._lib import PriorSegment, Segment, check, ptr, require_device, cur_stream, on_device
from .pool_desc import (avgpool_bf16_plan, avgpool_of, avgpool_plan, is_avgpool, is_maxpool, is_pool, pool_of,  # noqa: F401
                        pool_plan, pool_desc as _pool_desc)                                    # (ops.pool_of, ops.avgpool_of, ...)
from .conv_desc import ACT_CODE, _pair, bf16_flags, c8x3_flags, conv_desc, out_map, pool_code, pooled_map, slab_rule  # noqa: F401  (ops.ACT_CODE)

_scratch = {}
_retired = []     # (key, buffer) of outgrown scratch buffers: a captured hipGraph may have their address baked in, so a per-stream
                  # one is NEVER freed (a second pipeline / a larger model captured on the same stream must not pull the first
                  # graph's tickets or KL slots out from under it); a scope's go when its owner dies (_release_scope).  Sizes at
                  # least double, so a key retires < its final size in total.


_scope_tls = threading.local()
_scope_ids = itertools.count(1)


class scratch_scope:
    """Context: launches enqueued inside take their scratch buffers (KL partial slots, split-contraction tickets / partial tiles)
    from a set that belongs to `owner` instead of the per-(device, stream) set.  For captured graphs: the buffers' addresses are
    baked into the recorded launches, and a graph may be replayed on another stream than it was captured on (GraphedLogits) while
    torch's stream pool hands the capture stream's HANDLE to a later capture -- keyed by stream, the two graphs would then share
    tickets while replaying concurrently.  Keyed by owner, every graph has its own; the set is dropped when the owner dies."""

    def __init__(self, owner=None, token=None):
        if owner is None:                            # re-enter a scope by its token (autograd's device thread: fast_train backward)
            self.tok = token
            return
        tok = getattr(owner, "_bbb_scratch_token", None)
        if tok is None:
            tok = next(_scope_ids)
            try:
                owner._bbb_scratch_token = tok
                weakref.finalize(owner, _release_scope, tok)
            except (AttributeError, TypeError):
                # an owner that can carry neither the token nor a finaliser: a fresh token per call would leave a scratch set behind
                # every time and nothing would ever release it -- fall back to the per-(device, stream) set
                tok = None
        self.tok = tok

    def __enter__(self):
        self.prev = getattr(_scope_tls, "tok", None)
        _scope_tls.tok = self.tok
        return self

    def __exit__(self, *a):
        _scope_tls.tok = self.prev
        return False


def current_scratch_token():
    return getattr(_scope_tls, "tok", None)


def _release_scope(tok):
    mine = lambda k: isinstance(k[2], tuple) and k[2][:2] == ("scope", tok)
    for k in [k for k in _scratch if mine(k)]:
        del _scratch[k]
    _retired[:] = [(k, b) for k, b in _retired if not mine(k)]          # the scope's outgrown buffers: its graphs are gone too


def _scratch_key(device, kind):
    # (inside a scope still one set per stream: a captured step may fan its draws out over side streams that run concurrently)
    tok = getattr(_scope_tls, "tok", None)
    st = cur_stream(device)
    return (device.index, kind, ("scope", tok, st) if tok is not None else st)


def _grow(key, need, make):
    buf = _scratch.get(key)
    if buf is None or buf.numel() < need:
        if buf is not None:
            _retired.append((key, buf))
            need = max(int(need), 2 * buf.numel())
        buf = _scratch[key] = make(int(need))
    return buf


def _partials(device, n):
    # one scratch buffer per (device, stream): launches on different streams (graph lanes, a second model) may overlap.
    # every slot starts as "not published yet" (0xFF bytes); each launch re-arms the slots it consumed
    return _grow(_scratch_key(device, "kl"), max(int(n), 4096),
                 lambda m: torch.full((m,), -1, dtype=torch.int64, device=device).view(torch.float64))


def _segments(mus, rhos, ws, sigmas, epss, stream_ids, draws):
    arr = (Segment * len(mus))()
    for i, (mu, rho) in enumerate(zip(mus, rhos)):
        n = mu.numel()
        s = arr[i]
        s.mu, s.rho = mu.data_ptr(), rho.data_ptr()
        s.w = ptr(ws[i]) if ws is not None else 0
        s.sigma = ptr(sigmas[i]) if sigmas is not None else 0
        s.eps = ptr(epss[i]) if epss is not None else 0
        s.n = n
        s.draw_stride = n
        s.stream_id = stream_ids[i]
    return arr


def _prior_segments(priors, mus):
    """Tensor priors of a launch: `priors` is None or one (mu0 | None, sigma0 | None) per tensor of `mus`, each tensor fp32,
    contiguous, on the parameter's device, with the parameter's numel and no gradient (nothing flows to a prior).  Returns a ctypes
    array of PriorSegment -- or None when no tensor is set: the launch is then the scalar entry's, as it always was."""
    if priors is None:
        return None
    priors = list(priors)
    if len(priors) != len(mus):
        raise _lib.BBBHipError(f"priors: one (mu0, sigma0) pair per tensor, got {len(priors)} for {len(mus)} tensors")
    if all(p is None or (p[0] is None and p[1] is None) for p in priors):
        return None
    arr = (PriorSegment * len(mus))()
    for seg, p, m in zip(arr, priors, mus):
        if p is None:
            continue
        for name, t in zip(("mu0", "sigma0"), p):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != m.device or t.numel() != m.numel() or not t.is_contiguous():
                raise _lib.BBBHipError(f"prior {name}: a contiguous fp32 tensor on {m.device} with {m.numel()} elements (the parameter's), "
                                       f"got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}"
                                       + (f" {t.dtype} on {t.device}" if torch.is_tensor(t) else ""))
            if t.requires_grad:
                raise _lib.BBBHipError(f"prior {name} requires a gradient: nothing flows to a prior, pass a detached tensor")
            setattr(seg, name, t.data_ptr())
    return arr


def _reparam_fwd(segs, pri, nseg, *args):
    """bbb_reparam_kl_fwd, or bbb_reparam_kl_tp_fwd when the launch has tensor priors."""
    L = _lib.lib()
    if pri is None:
        check(L.bbb_reparam_kl_fwd(segs, nseg, *args), "bbb_reparam_kl_fwd")
    else:
        check(L.bbb_reparam_kl_tp_fwd(segs, pri, nseg, *args), "bbb_reparam_kl_tp_fwd")


def reparam_kl_forward(mus, rhos, prior_mu, prior_sigma, stream_ids, seed, call0, draws=1, sample=True,
                       want_sigma=False, sigma_squared=False, want_kl=True, eps=None, textbook_kl=False, priors=None):
    """Raw (no autograd) fused pass.  mus/rhos: lists of contiguous fp32 device tensors.  priors: per-weight Gaussian priors, one
    (mu0 | None, sigma0 | None) per tensor (see _prior_segments); None entries fall back to the scalars.
    Returns (ws | None, sigmas | None, kl | None); ws[i] has shape [draws, *mus[i].shape]."""
    if len(mus) == 0 or len(mus) > _lib.MAX_SEGMENTS:
        raise _lib.BBBHipError(f"1..{_lib.MAX_SEGMENTS} tensors per launch, got {len(mus)}")
    require_device(*mus, *rhos)
    dev = mus[0].device
    mus = [m.contiguous() for m in mus]
    rhos = [r.contiguous() for r in rhos]
    ws = [torch.empty((draws,) + tuple(m.shape), dtype=torch.float32, device=dev) for m in mus] if sample else None
    sigmas = [torch.empty_like(m) for m in mus] if want_sigma else None
    if eps is not None:
        eps = [e.contiguous() for e in eps]
        require_device(*eps)
        for e, m in zip(eps, mus):
            if e.numel() != draws * m.numel():
                raise _lib.BBBHipError("external eps must have shape [draws, *param.shape]")
    segs = _segments(mus, rhos, ws, sigmas, eps, stream_ids, draws)
    pri = _prior_segments(priors, mus)
    kl = torch.empty((), dtype=torch.float32, device=dev) if want_kl else None
    L = _lib.lib()
    nparts = L.bbb_reparam_partials(segs, len(mus))
    parts = _partials(dev, nparts) if want_kl else None
    flags = (_lib.SIGMA_SQUARED if sigma_squared else 0) | (_lib.KL_TEXTBOOK if textbook_kl else 0)
    with on_device(dev):
        _reparam_fwd(segs, pri, len(mus), draws, float(prior_mu), float(prior_sigma), seed, call0 & 0xFFFFFFFF,
                     flags, ptr(parts), ptr(kl), 0, rng.call_dev_ptr(dev), cur_stream(dev))
    return ws, sigmas, kl


def reparam_kl_backward(mus, rhos, gws, gkl, prior_mu, prior_sigma, stream_ids, seed, call0, draws, eps=None,
                        textbook_kl=False, gsigmas=None, sigma_squared=False, gws_mean_only=False, priors=None):
    """grad_mu[i], grad_rho[i] for every tensor (see bbb_reparam_kl_bwd; priors as in reparam_kl_forward: bbb_reparam_kl_tp_bwd).  gsigmas: gradients w.r.t. the forward's sigma
    (sigma_squared: sigma^2) outputs, entries may be None.  gws_mean_only: gws are gradients w.r.t. the means themselves
    (BBB_GW_MEAN_ONLY: added into grad_mu, nothing into grad_rho)."""
    require_device(*mus, *rhos)
    dev = mus[0].device
    mus = [m.contiguous() for m in mus]
    rhos = [r.contiguous() for r in rhos]
    gws = [None if g is None else g.contiguous() for g in gws]
    if eps is not None:
        eps = [e.contiguous() for e in eps]
    if gsigmas is not None:
        gsigmas = [None if g is None else g.to(dtype=torch.float32).contiguous() for g in gsigmas]
        require_device(*gsigmas)
    segs = _segments(mus, rhos, gws, gsigmas, eps, stream_ids, draws)
    pri = _prior_segments(priors, mus)
    gmu = [torch.empty_like(m) for m in mus]
    grho = [torch.empty_like(m) for m in mus]
    pm = (ctypes.c_void_p * len(mus))(*[g.data_ptr() for g in gmu])
    pr = (ctypes.c_void_p * len(mus))(*[g.data_ptr() for g in grho])
    if gkl is not None:
        gkl = gkl.to(device=dev, dtype=torch.float32).contiguous()
    flags = (_lib.KL_TEXTBOOK if textbook_kl else 0) | (_lib.SIGMA_SQUARED if (sigma_squared and gsigmas is not None) else 0)
    flags |= _lib.GW_MEAN_ONLY if gws_mean_only else 0
    tail = (draws, float(prior_mu), float(prior_sigma), seed, call0 & 0xFFFFFFFF, flags, ptr(gkl), pm, pr, rng.call_dev_ptr(dev),
            cur_stream(dev))
    with on_device(dev):
        if pri is None:
            check(_lib.lib().bbb_reparam_kl_bwd(segs, len(mus), *tail), "bbb_reparam_kl_bwd")
        else:
            check(_lib.lib().bbb_reparam_kl_tp_bwd(segs, pri, len(mus), *tail), "bbb_reparam_kl_tp_bwd")
    return gmu, grho


REPARAM_PLAN_FIELDS = ("kernel", "gpt", "nt", "chunks", "n_small", "small_chunk0", "tm_blocks", "grid")


def reparam_plan(segs, draws, slots=0, nseg=None, priors=None):
    """What bbb_reparam_kl_fwd launches for `segs` (bbb_reparam_kl_plan: the launch entry's own plan, host only): a dict of
    REPARAM_PLAN_FIELDS with kernel "fast" | "generic" and nt a bool.  segs: a ctypes array of Segment as the launch takes it, or a
    sequence whose items are element counts or dicts of Segment fields (mu, rho and w then get a placeholder address that is never
    read).  slots <= 0: the current device's resident blocks, as the launcher asks.  priors: a ctypes array of PriorSegment, or a
    sequence of (mu0, sigma0) ADDRESSES (0 / None = the scalar), one per segment: the plan of bbb_reparam_kl_tp_fwd
    (bbb_reparam_kl_tp_plan) -- the same launch shape, after the checks of the prior pointers."""
    if isinstance(segs, ctypes.Array):
        arr, nseg = segs, (len(segs) if nseg is None else nseg)
    else:
        nseg = len(segs)
        arr = (Segment * max(nseg, 1))()
        for s, item in zip(arr, segs):
            fields = {"n": item} if isinstance(item, int) else dict(item)
            s.mu = s.rho = s.w = 16
            for k, v in fields.items():
                setattr(s, k, v)
            if "draw_stride" not in fields:
                s.draw_stride = s.n
    out = [ctypes.c_int32(0) for _ in REPARAM_PLAN_FIELDS]
    if priors is None:
        check(_lib.lib().bbb_reparam_kl_plan(arr, nseg, draws, slots, *[ctypes.byref(o) for o in out]), "bbb_reparam_kl_plan")
    else:
        if not isinstance(priors, ctypes.Array):
            pairs = list(priors)
            if len(pairs) != nseg:
                raise _lib.BBBHipError(f"priors: one (mu0, sigma0) pair per segment, got {len(pairs)} for {nseg} segments")
            priors = (PriorSegment * max(len(pairs), 1))()
            for seg, (m0, s0) in zip(priors, pairs):
                seg.mu0, seg.sigma0 = m0 or 0, s0 or 0
        check(_lib.lib().bbb_reparam_kl_tp_plan(arr, priors, nseg, draws, slots, *[ctypes.byref(o) for o in out]),
              "bbb_reparam_kl_tp_plan")
    plan = {k: o.value for k, o in zip(REPARAM_PLAN_FIELDS, out)}
    plan["kernel"] = ("fast", "generic")[plan["kernel"]]
    plan["nt"] = bool(plan["nt"])
    return plan


ADAM_PLAN_SCALARS = ("step_size", "sqrt_bc2", "beta1", "beta2", "omb1", "omb2", "eps")


def adam_plan(segs, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, step=1, step_dev=0, lr_dev=0, nseg=None):
    """What bbb_adam_step launches for these arguments (bbb_adam_step_plan: the launch entry's own plan, csrc/adam_plan.h; host only:
    needs no device).  segs: a ctypes array of AdamSegment as the launch takes it, or a sequence whose items are element counts or
    dicts of AdamSegment fields (absent pointers get a 16-byte aligned placeholder address that is never read).  step_dev / lr_dev:
    addresses (0 = none).  Returns a dict: status (0 or the BBB_E* code the launch entry would return -- a refusal is reported, not
    raised, and leaves every other field zero), chunks, chunk_begin (17 entries), vec (one bool per segment: some thread can move 16
    bytes at a time) and the seven fp32 scalars of ADAM_PLAN_SCALARS as Python floats."""
    if isinstance(segs, ctypes.Array):
        arr, nseg = segs, (len(segs) if nseg is None else nseg)
    else:
        arr = (_lib.AdamSegment * max(len(segs), 1))()
        for s, item in zip(arr, segs):
            s.param = s.grad = s.exp_avg = s.exp_avg_sq = 4096
            for k, v in ({"n": item} if isinstance(item, int) else dict(item)).items():
                setattr(s, k, v)
        nseg = len(segs) if nseg is None else nseg
    chunks, begin = ctypes.c_int32(0), (ctypes.c_int32 * (_lib.MAX_SEGMENTS + 1))()
    sc, vec = (ctypes.c_float * len(ADAM_PLAN_SCALARS))(), (ctypes.c_int32 * _lib.MAX_SEGMENTS)()
    rc = _lib.lib().bbb_adam_step_plan(arr, nseg, float(lr), float(betas[0]), float(betas[1]), float(eps), int(step), step_dev or None,
                                       lr_dev or None, ctypes.byref(chunks), begin, sc, vec)
    plan = {"status": rc, "chunks": chunks.value, "chunk_begin": list(begin), "vec": [bool(v) for v in vec[:max(min(nseg, len(vec)), 0)]]}
    plan.update(zip(ADAM_PLAN_SCALARS, sc))
    return plan


def _adam_segments(segs, nseg):
    """adam_plan's segment forms -> (ctypes array, nseg)."""
    if isinstance(segs, ctypes.Array):
        return segs, (len(segs) if nseg is None else nseg)
    arr = (_lib.AdamSegment * max(len(segs), 1))()
    for s, item in zip(arr, segs):
        s.param = s.grad = s.exp_avg = s.exp_avg_sq = 4096
        for k, v in ({"n": item} if isinstance(item, int) else dict(item)).items():
            setattr(s, k, v)
    return arr, (len(segs) if nseg is None else nseg)


ADAM_PLAN_EX_SCALARS = ADAM_PLAN_SCALARS + ("wd32", "decay")
ADAM_EX_MODES = ("none", "l2", "decoupled")


def adam_plan_ex(segs, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, step=1, step_dev=0, lr_dev=0,
                 coef_dev=0, ok_dev=0, nseg=None):
    """What bbb_adam_step_ex launches (bbb_adam_step_ex_plan; host only).  As adam_plan, plus the fp32 scalars wd32 and decay and
    `mode`: "none" (weight_decay == 0), "l2" or "decoupled".  A refusal is reported in `status` and leaves every other field zero
    (mode "none")."""
    arr, nseg = _adam_segments(segs, nseg)
    chunks, begin = ctypes.c_int32(0), (ctypes.c_int32 * (_lib.MAX_SEGMENTS + 1))()
    sc, vec, mode = (ctypes.c_float * len(ADAM_PLAN_EX_SCALARS))(), (ctypes.c_int32 * _lib.MAX_SEGMENTS)(), ctypes.c_int32(0)
    rc = _lib.lib().bbb_adam_step_ex_plan(arr, nseg, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                          int(bool(decoupled)), int(step), step_dev or None, lr_dev or None, coef_dev or None,
                                          ok_dev or None, ctypes.byref(chunks), begin, sc, vec, ctypes.byref(mode))
    plan = {"status": rc, "chunks": chunks.value, "chunk_begin": list(begin), "vec": [bool(v) for v in vec[:max(min(nseg, len(vec)), 0)]],
            "mode": ADAM_EX_MODES[mode.value]}
    plan.update(zip(ADAM_PLAN_EX_SCALARS, sc))
    return plan


GRAD_NORM_CHUNK = 4096


def grad_norm_plan(segs, partials=4096, first=0, nseg=None, max_norm=None, norm=0.0, outs=(4096, 4096, 4096, 4096), npartials=None):
    """What the gradient-norm launches do for these arguments (bbb_grad_sumsq_plan and bbb_grad_norm_finish_plan; host only, needs no
    device).  segs as adam_plan's (only grad and n matter); partials: the address of the float64 buffer; first: index of this
    launch's first partial.  Returns status, chunks (= partials written), chunk_begin (17), vec (grad 16-byte aligned and n >= 4).
    With max_norm: also finish_status -- the finish launch's code for (partials, npartials or first + chunks, max_norm, outs = the
    addresses of norm / coef / ok / skipped) -- and coef, the coefficient it writes for the fp32 norm `norm`."""
    arr, nseg = _adam_segments(segs, nseg)
    chunks, begin, vec = ctypes.c_int32(0), (ctypes.c_int32 * (_lib.MAX_SEGMENTS + 1))(), (ctypes.c_int32 * _lib.MAX_SEGMENTS)()
    rc = _lib.lib().bbb_grad_sumsq_plan(arr, nseg, partials or None, int(first), ctypes.byref(chunks), begin, vec)
    plan = {"status": rc, "chunks": chunks.value, "chunk_begin": list(begin), "vec": [bool(v) for v in vec[:max(min(nseg, len(vec)), 0)]]}
    if max_norm is not None:
        coef = ctypes.c_float(0.0)
        n = int(first) + chunks.value if npartials is None else int(npartials)
        plan["finish_status"] = _lib.lib().bbb_grad_norm_finish_plan(partials or None, n, float(max_norm), *[o or None for o in outs],
                                                                     float(norm), ctypes.byref(coef))
        plan["coef"] = coef.value
    return plan


def eps_dump(n, seed, call, stream_id, device, start=0):
    out = torch.empty(n, dtype=torch.float32, device=device)
    with on_device(out.device):
        check(_lib.lib().bbb_eps_dump(out.data_ptr(), n, start, seed, call & 0xFFFFFFFF, stream_id, cur_stream(out.device)),
              "bbb_eps_dump")
    return out


def _same_channels(cin, w_cin):
    if cin != w_cin:
        raise _lib.BBBHipError(f"channel mismatch: input has {cin}, weight expects {w_cin}")


def _out_tensor(out, shape, dtype, device):
    """The launch's output: a fresh tensor, or the caller's `out=` viewed as `shape`."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.numel() != math.prod(shape) or not out.is_contiguous() or out.dtype != dtype:
        raise _lib.BBBHipError("out= must be a contiguous tensor of the output's size and dtype")
    return out.view(shape)


def conv2d_forward(x, w, bias, stride=1, padding=0, dilation=1, act=None):
    """Batched-over-draws conv on the fp32 matrix cores (no autograd).
    x: [E, B, Cin, H, W] or [1, B, Cin, H, W] (shared by all draws); w: [E, Cout, Cin, kh, kw] (or [1, ...]
    shared); bias: [E|1, Cout] or None.  Returns y [E, B, Cout, Ho, Wo] with E = max of the leading dims."""
    require_device(x, w, bias)
    x, w = x.contiguous(), w.contiguous()
    bias = None if bias is None else bias.contiguous()
    Ex, B, Cin, H, W = x.shape
    Ew, Cout, w_cin, kh, kw = w.shape
    _same_channels(Cin, w_cin)
    d, ho, wo = conv_desc(B, Cin, (H, W), Cout, (kh, kw), stride, padding, dilation, act=act)
    E, _, _ = slab_rule(d, Ex, Ew)
    y = torch.empty((E, B, Cout, ho, wo), dtype=torch.float32, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), ptr(bias), y.data_ptr(),
                                        cur_stream(x.device)), "bbb_conv2d_fwd")
    return y


def lrt_conv2d_forward(x, w_mu, w_var, b_mu, b_var, seed, call0, stream_id, stride=1, padding=0, dilation=1,
                       sample=True, eps=None, want_moments=False, act=None):
    """LRT layer in one launch.  x: [E, B, Cin, H, W] (E independent sample slabs); weights shared.
    Returns (y, act_mu | None, act_var | None), each [E, B, Cout, Ho, Wo]."""
    require_device(x, w_mu, w_var, b_mu, b_var, eps)
    x = x.contiguous()
    w_mu, w_var = w_mu.contiguous(), w_var.contiguous()
    b_mu = None if b_mu is None else b_mu.contiguous()
    b_var = None if b_var is None else b_var.contiguous()
    E, B, Cin, H, W = x.shape
    Cout, w_cin, kh, kw = w_mu.shape
    _same_channels(Cin, w_cin)
    d, ho, wo = conv_desc(B, Cin, (H, W), Cout, (kh, kw), stride, padding, dilation, act=act)
    slab_rule(d, E, 1, weights_shared=True)
    shape = (E, B, Cout, ho, wo)
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    am = torch.empty(shape, dtype=torch.float32, device=x.device) if want_moments else None
    av = torch.empty(shape, dtype=torch.float32, device=x.device) if want_moments else None
    if eps is not None:
        eps = eps.contiguous()
        if eps.numel() != y.numel():
            raise _lib.BBBHipError("external eps must have the output's shape")
    with on_device(x.device):
        check(_lib.lib().bbb_lrt_conv2d_fwd(ctypes.byref(d), x.data_ptr(), w_mu.data_ptr(), w_var.data_ptr(), ptr(b_mu),
                                            ptr(b_var), y.data_ptr(), ptr(am), ptr(av), ptr(eps), seed,
                                            call0 & 0xFFFFFFFF, stream_id, 1 if sample else 0, rng.call_dev_ptr(x.device),
                                            cur_stream(x.device)),
              "bbb_lrt_conv2d_fwd")
    return y, am, av


@contextlib.contextmanager
def graph_capture(graph, stream=None):
    """torch.cuda.graph(graph, stream, thread-local error mode) with the cyclic garbage collector out of the way: this torch no
    longer collects before a capture, and a dead reference cycle that owns an older hipGraph (or any device memory) may be
    collected at ANY allocation -- inside the capture, where destroying a graph is an illegal HIP call that surfaces as
    `operation not permitted when stream is capturing` from a destructor, i.e. terminate().  Collect first, keep the collector off
    until the capture has ended."""
    import gc
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            yield
    finally:
        if was:
            gc.enable()


class LaunchConfig:
    """The launch-shape / arithmetic-mode choices of the batch-innermost path, as ONE object instead of process-wide switches.

    A `GraphedMC` / `GraphedPipeline` / `GraphedLogits` / `GraphedTrainStep` / `GraphedUncertainty` snapshots the configuration that
    is current when it is built (or takes `launch_config=`) and enqueues every launch under it, so two models -- or two pipelines of one model --
    with different modes coexist in one process and on several threads.  `ops.gemm_mode = ...` and friends still exist: they
    read / write the fields of the process DEFAULT configuration (what applies when nobody asked for anything else).

    gemm_mode   "fp32" | "bf16x3": the batch-innermost BBB GEMM launches (inference AND the role-swapped gradient launches of the
                training path) run their contraction on the 16-bit matrix pipe at fp32 accuracy (bbb_conv2d_chwn_bf16x3_fwd:
                every operand element split into three bf16 pieces while staged, six products, fp32 accumulation).  Range-free
                (bf16 has fp32's exponent range: no operand windows or scales).  Opt-in: results agree with the fp32 kernel
                to rounding, not bit for bit.  LRT layers keep the fused fp32 kernel (one staged x tile feeds both of its
                contractions; a split form would need twelve operand planes in LDS).
                The input gradient of a STRIDED layer (conv2d_chwn_input_grad(stride != 1)) runs on the fp32 transposed
                launch in either mode; it is held to the same bounds.
    bf16x3_min_workgroups   smaller launches stay on the fp32 kernel (and the layer's split contraction): measured faster there
    s3_min_images   split-bf16 mode: steps of at least this many (draw x image) rows keep their activations in the split format S3
                between layers (ensemble._mc_logits_chwn); smaller steps split while staging, per launch
    split_k     layers with few (pixel, channel-tile) groups and a long contraction (AlexNet conv4 / conv5) add their k ranges'
                partial sums in range order (bbb_conv2d_chwn_splitk_fwd): a property of the LAYER, identical for every launch
                size and partition.  False: the plain fmaf chain everywhere (bit-identical to the reference-layout kernel).
                (The strided input gradient is never split: one chain per element whatever this says.)
    pool_fusion a conv layer followed by [activation ->] MaxPool2d(2, 2) may run as ONE launch (bbb_conv_desc_t::pool)
    pool_fuse_min_items / pool_fuse_imbalance   a launch with nothing else in flight: only when it still has this many (pooled pixel,
                64-channel tile, 128-image tile, draw) items and they spread over the 256 CUs to within this factor (4x longer items)
    launches_overlap   the caller enqueues work that runs beside other lanes' kernels: the under-filled tail of a fused launch is
                then filled by them, and fusing pays from ~2 items per CU on (measured, profiles/r04_notes.md section 7: -2 to
                -3 % per step at 10 draws x 3 lanes, +4.5 % with one lane; at 5 draws per launch it no longer does)
    pool_fuse_weight_budget   bytes of weight tiles concurrently live per XCD that a fused launch may have (see pool_fusion_ok)
    c8x3        split-bf16 mode: layers with Cin % 16 == 0 take the MFMA-ready-operand kernel (csrc/pconv_c8x3.hip), whatever the
                launch size (a property of the layer: partitions of a step keep its bits)
    c8x3_s2d    ... and a strided first layer on few channels (s2d_layer_ok: AlexNet conv1) joins them in space-to-depth form
    dropin_precision   "fp32" | "bf16": what a whole-model `net(x)` through the drop-in layers computes in.  "bf16" = the bf16 storage
                path of ensemble.mc_forward(precision="bf16") (sampled weights and activations in bf16, fp32 accumulation, fp32 logits)
                behind the unmodified `for j in range(num_ens): net(x)` loop -- inference only, BBB models the batch-innermost path
                covers; anything else (autograd enabled, LRT layers, hooks, a layer called on its own) raises instead of silently
                computing in fp32
    bf16_lrt    False | True: precision="bf16" admits models whose Bayesian layers are ALL local-reparameterisation layers, on
                lrt_conv2d_chwn_bf16_forward (csrc/pconv_bf16_lrt.hip: both contractions of a layer on the 16-bit matrix pipe from one
                staged bf16 x tile; W_mu and sigma^2 rounded once per step by lrt_weights_bf16, x^2 rounded once to bf16 in the kernel;
                fp32 accumulation, biases, sampling step, KL and tail; the fp32 path's noise elements).  Inference on
                ensemble.mc_logits / mc_forward / GraphedMC / GraphedPipeline, B % 8 == 0.  Opt-in: under the default, bf16 on an LRT
                model raises, as it always did
    bf16_strided_train   False | True: train_step / forward_loss / GraphedTrainStep(precision="bf16") admit BBB models with STRIDED
                convolutions behind the first layer: their input gradient runs on the transposed form of the general bf16 GEMM
                (conv2d_chwn_input_grad_bf16(stride=...), bbb_conv2d_chwn_bf16_dgrad; bf16 in, fp32 accumulation, one rounding).
                Opt-in: under the default such a model is refused, as it always was (precision="fp32" trains it)
    bf16_avgpool   False | True: precision="bf16" admits models with nn.AvgPool2d / a dividing nn.AdaptiveAvgPool2d (pool_desc.avgpool_of)
                on avgpool_chwn_bf16 / avgpool_act_backward_chwn_bf16 (csrc/pool2d_bf16.hip: bf16 planes, fp32 sums in scan order, one
                IEEE division, ONE rounding to bf16; the backward in gather form with act' from the stored bf16 output).  Inference
                (mc_logits / mc_forward / the Graphed* objects / the drop-in loop; LRT models together with bf16_lrt) and BBB
                training (train_step / forward_loss / GraphedTrainStep), B % 8 == 0.  Opt-in: under the default bf16 on a model
                with an average pool raises, naming this switch, as it always did
    bf16_input_grad   False | True: forward_loss / mc_forward / mc_logits(precision="bf16") admit an input that requires a gradient
                (saliency maps, adversarial steps): the bf16 node's backward then ends in first_layer_input_grad_bf16
                (csrc/input_grad_bf16.hip: the first layer's contraction over (draw, channel) on the bf16 MFMA from the sampled rows
                and g_pre where they are, fp32 accumulation, an fp32 dx that is never rounded) and, with frozen parameters, runs no
                weight side at all.  BBB models, B % 8 == 0, eager only.  Opt-in: under the default such an input is refused,
                naming this switch, as it always was (precision="fp32" has input gradients)
    bf16_lrt_input_grad   False | True: together with bf16_lrt, forward_loss / mc_forward / mc_logits(precision="bf16") admit an input
                that requires a gradient on an all-LRT model whose parameters are ALL FROZEN (saliency maps, adversarial steps against
                the reference's default layer type): fast_train._MCForwardLRTBF16 -- the bf16 LRT inference launches with a tape, and
                the activation side of the LRT backward in bf16 storage (lrt_pool_act_backward_chwn_bf16, csrc/pool2d_bf16.hip: the
                noise regenerated from the counter; the two input-gradient contractions on conv2d_chwn_input_grad_bf16; an fp32 dx
                from first_layer_input_grad_bf16_lrt that is never rounded).  No parameter gradient (bf16 LRT training does not
                exist: trainable parameters are refused), no average pools, B % 8 == 0, eager only, one device.  Does not need
                bf16_input_grad; without bf16_lrt it changes nothing.  Opt-in: under the default such a call raises what it always did"""
    FIELDS = ("gemm_mode", "bf16x3_min_workgroups", "s3_min_images", "split_k", "pool_fusion", "pool_fuse_min_items",
              "pool_fuse_imbalance", "launches_overlap", "pool_fuse_min_items_overlapped", "pool_fuse_weight_budget",
              "bf16_pool_fuse_min_rows", "bf16_pool_fuse_min_rows_overlapped", "bf16_c8", "bf16_c8_min_items", "c8x3", "c8x3_s2d",
              "dropin_precision", "bf16_lrt", "bf16_strided_train", "bf16_avgpool", "bf16_input_grad", "bf16_lrt_input_grad")
    __slots__ = FIELDS

    def __init__(self, **kw):
        self.gemm_mode = "fp32"
        self.bf16x3_min_workgroups = 256
        self.s3_min_images = 2048
        self.split_k = True
        self.pool_fusion = True
        self.pool_fuse_min_items = 1536
        self.pool_fuse_imbalance = 1.07
        self.launches_overlap = False
        self.pool_fuse_min_items_overlapped = 400
        self.pool_fuse_weight_budget = 1 << 20
        self.bf16_pool_fuse_min_rows = 0               # (bf16_pool_fusion_ok) pooled rows x image tiles x slabs from which the pooled
        self.bf16_pool_fuse_min_rows_overlapped = 0    # first-layer form of the bf16 path is taken (0: always -- the library's
                                                       # window-resident form wins from one step per launch on); ... beside other lanes
        self.bf16_c8 = True                            # (bf16_c8_input_ok) channel-interleaved activations between a pooled first layer and a
        self.bf16_c8_min_items = 0                     # layer that has the strip form over them, for launches of at least this many strip
                                                       # workgroups (0: always -- measured faster from one step per launch on); False: never
        self.dropin_precision = "fp32"
        self.bf16_lrt = False                          # precision="bf16" on all-LRT models (lrt_conv2d_chwn_bf16_forward); opt-in
        self.bf16_strided_train = False                # bf16 training of models with strided later layers (bbb_conv2d_chwn_bf16_dgrad); opt-in
        self.bf16_avgpool = False                      # precision="bf16" on models with average pools (csrc/pool2d_bf16.hip); opt-in
        self.bf16_input_grad = False                   # precision="bf16" on inputs that require a gradient (csrc/input_grad_bf16.hip); opt-in
        self.bf16_lrt_input_grad = False               # ... on all-LRT models with frozen parameters, together with bf16_lrt (_MCForwardLRTBF16); opt-in
        self.c8x3 = True                               # split-bf16 mode: layers (behind the first) with Cin % 32 == 0 run on the
                                                       # MFMA-ready-operand kernel (conv2d_c8x3_forward: channel-interleaved split
                                                       # activations + tap-major weights from the parameter pass); False: round 4's
                                                       # kernel (split while staging / planar S3) everywhere
        self.c8x3_s2d = True                           # ... and a strided first layer on few channels joins that chain in space-to-depth form
                                                       # (s2d_layer_ok: AlexNet conv1), pooling inside its launch; False: fp32 kernel
        for k, v in kw.items():
            setattr(self, k, v)              # (unknown names raise: __slots__)

    def copy(self, **kw):
        c = LaunchConfig(**{k: getattr(self, k) for k in self.FIELDS})
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def key(self):
        """Hashable value of every field (cache keys: a result / a captured graph depends on all of them)."""
        return tuple(getattr(self, k) for k in self.FIELDS)

    def __repr__(self):
        return "LaunchConfig(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.FIELDS)


_default_config = LaunchConfig()
_tls = threading.local()


def current_config():
    """The configuration launches are enqueued under right now: the innermost `use_config` of THIS thread, else the process default."""
    st = getattr(_tls, "stack", None)
    return st[-1] if st else _default_config


class use_config:
    """Context: enqueue under `cfg` (a LaunchConfig), or under the current configuration with some fields replaced
    (`use_config(gemm_mode="bf16x3")`).  Thread-local, re-entrant."""

    def __init__(self, cfg=None, **fields):
        self.cfg, self.fields = cfg, fields

    def __enter__(self):
        base = self.cfg if self.cfg is not None else current_config()
        cfg = base.copy(**self.fields) if self.fields else base
        st = getattr(_tls, "stack", None)
        if st is None:
            st = _tls.stack = []
        st.append(cfg)
        return cfg

    def __exit__(self, *a):
        _tls.stack.pop()
        return False


_split_plans = {}


def _split_scratch(d, lrt, device):
    """(k_split, scratch tensor | None) for this launch.  k_split is the LAYER's plan (a function of its geometry only:
    bbb_conv2d_chwn_splitk_scratch), applied to every launch of the layer whatever its size, so that a draw computed alone, in
    a 10-draw launch, as a work unit or as one of several steps per launch is the same number bit for bit; the scratch (a
    zero-initialised per-(device, stream) buffer whose arrival tickets stay zero from launch to launch) is only there when
    this launch is small enough for the cross-workgroup form -- larger launches run the same summation order inside one
    workgroup per tile."""
    if not current_config().split_k:
        return 1, None
    pkey = (bytes(d), bool(lrt))
    plan = _split_plans.get(pkey)
    if plan is None:
        ks = ctypes.c_int32(1)
        need = _lib.lib().bbb_conv2d_chwn_splitk_scratch(ctypes.byref(d), 1 if lrt else 0, ctypes.byref(ks))
        plan = _split_plans[pkey] = (ks.value, int(need))
    ks_v, need = plan
    if ks_v <= 1:
        return 1, None
    if need <= 0:
        return ks_v, None
    buf = _grow(_scratch_key(device, "splitk"), max(int(need), 1 << 22),
                lambda m: torch.zeros(m, dtype=torch.uint8, device=device))
    return ks_v, buf


class overlapped_launches(use_config):
    """Context: the launches enqueued inside run concurrently with other streams' kernels (a lane of a GraphedPipeline)."""

    def __init__(self, on=True):
        super().__init__(launches_overlap=bool(on))


def pool_fusion_ok(x_shape, w_shape, stride, padding, dilation, draws, pool_module=None, fp32_kernel=False):
    """Should conv2d_chwn_forward(..., pool=True) replace conv + maxpool_chwn(2, 2) for this launch?  Same bits either way; the
    fused launch saves the pooling launch and 3/4 of the layer's output traffic, but its items are four times fewer and four
    times longer: chosen when other lanes' kernels run beside it (launches_overlap), else only when its items still fill the chip
    evenly (measured: profiles/r04_notes.md section 7).
    x_shape [*, Cin, H, W, B], w_shape [*, Cout, Cin, kh, kw]; pool_module: the nn.MaxPool2d that follows (checked for 2 / 2)."""
    cfg = current_config()
    if not cfg.pool_fusion or (cfg.gemm_mode != "fp32" and not fp32_kernel):       # (fp32_kernel: the caller runs THIS launch on the fp32 kernel)
        return False
    key = (tuple(x_shape[-4:]), tuple(w_shape[-4:]), _pair(stride), _pair(padding), _pair(dilation), int(draws), cfg.launches_overlap,
           cfg.pool_fuse_min_items, cfg.pool_fuse_imbalance, cfg.pool_fuse_min_items_overlapped, cfg.pool_fuse_weight_budget,
           None if pool_module is None else (str(pool_module.kernel_size), str(pool_module.stride), str(pool_module.padding),
                                             str(pool_module.dilation), pool_module.ceil_mode,
                                             getattr(pool_module, "return_indices", False)))
    hit = _pool_rule_cache.get(key)
    if hit is None:
        if len(_pool_rule_cache) > 512:
            _pool_rule_cache.clear()
        hit = _pool_rule_cache[key] = _pool_fusion_rule(x_shape, w_shape, stride, padding, dilation, draws, pool_module)
    return hit


_pool_rule_cache = {}


def is_pool_2x2(pool_module):
    """Is this nn.MaxPool2d the plain 2 x 2 / stride 2 window (what the fused launches implement)?"""
    pr = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    return not (pr(pool_module.kernel_size) != (2, 2) or pr(pool_module.stride if pool_module.stride is not None else 2) != (2, 2) or
                pr(pool_module.padding) != (0, 0) or pr(pool_module.dilation) != (1, 1) or pool_module.ceil_mode or
                getattr(pool_module, "return_indices", False))


def _pool_fusion_rule(x_shape, w_shape, stride, padding, dilation, draws, pool_module):
    cfg = current_config()
    if pool_module is not None and not is_pool_2x2(pool_module):
        return False
    B = x_shape[-1]
    Cin, H, W = x_shape[-4:-1]
    _same_channels(Cin, w_shape[-3])
    d, ho, wo = conv_desc(B, Cin, (H, W), w_shape[-4], tuple(w_shape[-2:]), stride, padding, dilation, int(draws))
    if ho % 2 or wo % 2 or B % 4:
        return False
    ks = ctypes.c_int32(1)
    _lib.lib().bbb_conv2d_chwn_splitk_scratch(ctypes.byref(d), 0, ctypes.byref(ks))
    if ks.value > 1:
        return False
    # the weight tiles live in one XCD's L2 at a time: an XCD runs 128 workgroups = 128 / (pooled pixels x image tiles) groups of
    # items that share a (draw, 64-channel) weight tile -- four times the unfused launch's, whose groups hold four times the items.
    # AlexNet conv2 on CIFAR maps (4 pooled pixels x 4 tiles: 8 tiles of 410 KB) overflowed the 4 MB L2: 404 MB fetched per step for
    # 25 MB of operands, and no time gained (profiles/r04_notes.md section 7)
    per_group = (ho // 2) * (wo // 2) * -(-B // 128)
    if max(1, 128 // per_group) * 64 * w_shape[-3] * w_shape[-2] * w_shape[-1] * 4 > cfg.pool_fuse_weight_budget:
        return False
    items = int(draws) * per_group * -(-w_shape[-4] // 64)
    if cfg.launches_overlap:
        return items >= cfg.pool_fuse_min_items_overlapped
    return items >= cfg.pool_fuse_min_items and -(-items // 256) * 256 <= cfg.pool_fuse_imbalance * items


def conv2d_chwn_forward(x, w, bias, stride=1, padding=0, dilation=1, act=None, out=None, units=None, n_units=None,
                        x_per_slice=False, x_div=1, bf16x3=None, x_s3=False, out_s3=False, x_off=0, pool=False, w_tap_major=False):
    """Batch-innermost conv for the ensemble path.  x: [E|1, Cin, H, W, B] (B % 4 == 0); w: [E|1, Cout, Cin, kh, kw];
    bias [E|1, Cout] or None -> y [E, Cout, Ho, Wo, B].  Padding taps are skipped, not multiplied.
    Work units (ensemble sharding): units = (S, off), n_units = U output slabs; w / bias hold the weight sets of the draws
    the units touch, x is [U, ...] or, for a layer whose input is the same for every draw, the per-slice [S, Cin, H, W, Bs].
    x_div = D > 1 (several Monte-Carlo steps per launch): x holds E / D input slabs and output slab e reads slab e // D
    (bbb_conv_desc_t::x_unit_div) -- the first layer of G steps x D draws, each step on its own batch.  x_off (< D): output slab
    e reads slab (e + x_off) // D -- a rank's share of a group of steps that starts in the middle of a step.
    bf16x3: True / False = run this launch on the split-bf16 kernel or not; None (default) = ops.gemm_mode decides.
    x_s3 / out_s3 (split-bf16 kernel only, B % 8 == 0): the input / output travels in the split activation format S3 -- a bf16
    tensor [E|1, 3, C, H, W, B] holding the hi / mid / lo pieces of the same fp32 values (s3_from_f32 / s3_to_f32).
    pool = True (fp32 kernel, layers without a split contraction, even Ho and Wo): the launch also applies MaxPool2d(2, 2) to the
    activated output -> y [E, Cout, Ho/2, Wo/2, B], bit for bit maxpool_chwn(conv2d_chwn_forward(...), 2, 2) (pool_fusion_ok says
    when that pays).
    w_tap_major = True (fp32 kernel only): w is given as [E|1, Cout, kh, kw, Cin] and the contraction runs tap-major
    (bbb_conv_desc_t::w_tap_major) -- the same products in another summation order."""
    require_device(w, bias)
    require_device(x, dtype=torch.bfloat16 if x_s3 else torch.float32)
    x, w = x.contiguous(), w.contiguous()
    bias = None if bias is None else bias.contiguous()
    if w_tap_major:
        if x_s3 or out_s3 or bf16x3:
            raise _lib.BBBHipError("w_tap_major: fp32 kernel only")
        bf16x3 = False
        Ew, Cout, kh, kw, w_cin = w.shape
    else:
        Ew, Cout, w_cin, kh, kw = w.shape
    if x_s3 and (x.dim() != 6 or x.shape[1] != 3 or x.shape[5] % 8):
        raise _lib.BBBHipError("an S3 input is a bf16 tensor [E|1, 3, C, H, W, B] with B % 8 == 0")
    Ex, Cin, H, W, B = (x.shape[0], *x.shape[2:]) if x_s3 else x.shape
    _same_channels(Cin, w_cin)
    d, ho, wo = conv_desc(B, Cin, (H, W), Cout, (kh, kw), stride, padding, dilation, act=act, x_planes=3 if x_s3 else 1)
    E, _, _ = slab_rule(d, Ex, Ew, units=units, n_units=n_units, x_per_slice=x_per_slice, x_div=x_div, x_off=x_off)
    if w_tap_major:
        d.w_tap_major = 1
    if pool:
        if x_s3 or out_s3 or bf16x3 or ho % 2 or wo % 2:
            raise _lib.BBBHipError("pool=True: fp32 kernel only, even output height and width")
        d.pool = 1
        ho, wo = ho // 2, wo // 2
    if out_s3 and B % 8:
        raise _lib.BBBHipError("an S3 output needs B % 8 == 0")
    y = _out_tensor(out, (E, 3, Cout, ho, wo, B) if out_s3 else (E, Cout, ho, wo, B), torch.bfloat16 if out_s3 else torch.float32, x.device)
    with on_device(x.device):
        if x_s3 or out_s3 or (not pool and (bf16x3 if bf16x3 is not None else current_config().gemm_mode == "bf16x3")
                              and E * ho * wo * -(-Cout // 64) * -(-B // 128) >= current_config().bf16x3_min_workgroups):
            check(_lib.lib().bbb_conv2d_chwn_bf16x3_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), ptr(bias), y.data_ptr(),
                                                        (1 if x_s3 else 0) | (2 if out_s3 else 0), cur_stream(x.device)),
                  "bbb_conv2d_chwn_bf16x3_fwd")
            return y
        ks, scr = _split_scratch(d, False, x.device)
        if ks > 1 and pool:
            raise _lib.BBBHipError("pool=True: this layer's contraction is split (conv + maxpool_chwn instead)")
        if ks > 1:
            check(_lib.lib().bbb_conv2d_chwn_splitk_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), ptr(bias), y.data_ptr(), ks,
                                                        ptr(scr), 0 if scr is None else scr.numel(), cur_stream(x.device)),
                  "bbb_conv2d_chwn_splitk_fwd")
        else:
            check(_lib.lib().bbb_conv2d_chwn_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), ptr(bias), y.data_ptr(),
                                                 cur_stream(x.device)), "bbb_conv2d_chwn_fwd")
    return y


def s3_from_f32(x):
    """fp32 [E, ...] -> its split activation form S3: bf16 [E, 3, ...] (hi, mid, lo pieces; exact).  The trailing dims must hold
    a multiple of 8 elements."""
    require_device(x)
    x = x.contiguous()
    n = x.numel() // x.shape[0]
    y = torch.empty((x.shape[0], 3) + tuple(x.shape[1:]), dtype=torch.bfloat16, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_s3_convert(x.data_ptr(), y.data_ptr(), x.shape[0], n, 1, cur_stream(x.device)), "bbb_s3_convert")
    return y


def s3_to_f32(x):
    """S3 bf16 [E, 3, ...] -> the fp32 tensor [E, ...] it stores (hi + mid + lo, exact)."""
    require_device(x, dtype=torch.bfloat16)
    x = x.contiguous()
    n = x.numel() // (3 * x.shape[0])
    y = torch.empty((x.shape[0],) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_s3_convert(x.data_ptr(), y.data_ptr(), x.shape[0], n, 0, cur_stream(x.device)), "bbb_s3_convert")
    return y


def maxpool_chwn_s3(x, k, s):
    """MaxPool2d(k, s) on an S3 tensor [E, 3, C, H, W, B] (B % 8 == 0) -> [E, 3, C, Ho, Wo, B]."""
    require_device(x, dtype=torch.bfloat16)
    x = x.contiguous()
    E, three, C, H, W, B = x.shape
    ho, wo = pooled_map(H, W, (k, s))
    y = torch.empty((E, 3, C, ho, wo, B), dtype=torch.bfloat16, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_maxpool_chwn_s3(x.data_ptr(), y.data_ptr(), E, C, H, W, B, int(k), int(s), cur_stream(x.device)),
              "bbb_maxpool_chwn_s3")
    return y


# ---- split-bf16 contraction over MFMA-ready operands (csrc/pconv_c8x3.hip): channel-interleaved split activations + tap-major weights
def c8s3_from_f32(x, squares=False):
    """fp32 batch-innermost [E, C, H, W, B] (C % 8 == 0) -> "c8 S3": bf16 [E, 3, C / 8, H, W, B, 8], the hi / mid / lo pieces
    (exact: hi + mid + lo is the fp32 value) of the 8 channels 8g .. 8g + 7 of an image adjacent in memory.
    squares = True: SIX planes [E, 6, ...] -- the pieces of the values, then the pieces of their squares (fp32 products): the slabs
    of the LRT chain (lrt_conv2d_c8x3_forward's second contraction reads the squares)."""
    require_device(x)
    x = x.contiguous()
    E, C, H, W, B = x.shape
    if C % 8:
        raise _lib.BBBHipError("c8 S3 needs a multiple of 8 channels")
    y = torch.empty((E, 6 if squares else 3, C // 8, H, W, B, 8), dtype=torch.bfloat16, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_c8s3_convert(x.data_ptr(), y.data_ptr(), E, C, H * W, B, 2 if squares else 1, cur_stream(x.device)), "bbb_c8s3_convert")
    return y


def c8s3_to_f32(x):
    """c8 S3 [E, 3 | 6, C / 8, H, W, B, 8] -> the fp32 batch-innermost tensor [E, C, H, W, B] it stores (exact; six-plane slabs: their
    values)."""
    require_device(x, dtype=torch.bfloat16)
    x = x.contiguous()
    E, planes, CG, H, W, B, eight = x.shape
    y = torch.empty((E, CG * 8, H, W, B), dtype=torch.float32, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_c8s3_convert(x.data_ptr(), y.data_ptr(), E, CG * 8, H * W, B, 3 if planes == 6 else 0, cur_stream(x.device)),
              "bbb_c8s3_convert")
    return y


def w_tap_major(w):
    """[E, Cout, Cin, kh, kw] -> the tap-major rows [E, Cout, kh * kw, Cin] (what the parameter pass writes directly for a
    segment with w_tm_cin set: sample_weights_tm)."""
    require_device(w)
    w = w.contiguous()
    E, Cout, Cin, kh, kw = w.shape
    y = torch.empty((E, Cout, kh * kw, Cin), dtype=torch.float32, device=w.device)
    with on_device(w.device):
        check(_lib.lib().bbb_w_tap_major(w.data_ptr(), y.data_ptr(), E * Cout, Cin, kh * kw, cur_stream(w.device)), "bbb_w_tap_major")
    return y


def s2d_geometry(cin, kernel_size, stride, padding, dilation, h, w):
    """Space-to-depth form of a strided square layer (bbb_s2d_c8s3 / bbb_w_s2d_tap_major): None, or (m, C', Hb, Wb, Ho, Wo) -- the
    layer as an m x m convolution, stride 1, no padding, over a block image of C' channels and Hb x Wb positions."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
    if kh != kw or sh != sw or ph != pw or (dh, dw) != (1, 1):
        return None
    ho, wo = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    if ho <= 0 or wo <= 0:
        return None
    m = -(-kh // sh)
    cp = -(-(cin * sh * sh) // 16) * 16
    return m, cp, ho + m - 1, wo + m - 1, ho, wo


def s2d_zero_border(cin, kernel_size, stride, padding, h, w):
    """Block rows / columns of the layer's space-to-depth image that lie entirely in the padding: (lead_h, lead_w, trail_h, trail_w)."""
    g = s2d_geometry(cin, kernel_size, stride, padding, 1, h, w)
    s, p = _pair(stride)[0], _pair(padding)[0]
    return (p // s, p // s, max(0, g[2] - -(-(p + h) // s)), max(0, g[3] - -(-(p + w) // s)))


def s2d_layer_ok(cin, cout, kernel_size, stride, padding, dilation, h, w, max_waste=1.5):
    """Should a layer that bbb_conv2d_c8x3_fwd cannot take directly (few input channels) run on it in space-to-depth form?  Yes when
    the block form's contraction (m * m * C' products per output) is at most max_waste times the layer's own (kh * kw * Cin): AlexNet
    conv1 (3 channels, 11 x 11, stride 4: 9 x 48 = 432 against 363, 1.19); not a 5 x 5 stride-1 layer on 3 channels (25 x 16 against
    75)."""
    g = s2d_geometry(cin, kernel_size, stride, padding, dilation, h, w)
    if g is None or cout % 8:
        return False
    kh, kw = _pair(kernel_size)
    return g[0] * g[0] * g[1] <= max_waste * kh * kw * cin


def s2d_c8s3(x, blocks, kernel_size, stride, padding, squares=False):
    """The caller's NCHW fp32 batch [blocks * Bs, C, H, W] -> the c8 S3 block image [blocks, 3, C' / 8, Hb, Wb, Bs, 8] of the layer
    (kernel_size, stride, padding): see s2d_geometry.  squares = True: six planes (the squares' pieces behind: an LRT first layer)."""
    require_device(x)
    x = x.contiguous()
    N, C, H, W = x.shape
    k, st, pd = _pair(kernel_size)[0], _pair(stride)[0], _pair(padding)[0]
    g = s2d_geometry(C, kernel_size, stride, padding, 1, H, W)
    if g is None or N % blocks:
        raise _lib.BBBHipError("space-to-depth form: square kernel / stride / padding, no dilation, the batch a multiple of `blocks`")
    m, cp, hb, wb, _, _ = g
    y = torch.empty((blocks, 6 if squares else 3, cp // 8, hb, wb, N // blocks, 8), dtype=torch.bfloat16, device=x.device)
    with on_device(x.device):
        fn = _lib.lib().bbb_s2d_c8s3sq if squares else _lib.lib().bbb_s2d_c8s3
        check(fn(x.data_ptr(), y.data_ptr(), blocks, N // blocks, C, H, W, k, st, pd, cur_stream(x.device)), "bbb_s2d_c8s3")
    return y


def w_s2d_tap_major(w, stride):
    """[E, Cout, Cin, k, k] -> the tap-major rows [E, Cout, m * m, C'] of the space-to-depth layer (zeros outside the k x k taps and in
    the padding channels)."""
    require_device(w)
    w = w.contiguous()
    E, Cout, Cin, kh, kw = w.shape
    st = _pair(stride)[0]
    m = -(-kh // st)
    cp = -(-(Cin * st * st) // 16) * 16
    y = torch.empty((E, Cout, m * m, cp), dtype=torch.float32, device=w.device)
    with on_device(w.device):
        check(_lib.lib().bbb_w_s2d_tap_major(w.data_ptr(), y.data_ptr(), E * Cout, Cin, kh, st, cur_stream(w.device)), "bbb_w_s2d_tap_major")
    return y


def c8x3_layer_ok(cin, cout, is_logits=False):
    """May a BBB layer with these channel counts run on bbb_conv2d_c8x3_fwd?  (16-channel k steps inside one tap; the output is
    written in groups of 8 channels unless it is the fp32 logits tensor.)"""
    return cin % 16 == 0 and (is_logits or cout % 8 == 0)


def conv2d_c8x3_forward(x, w_tm, bias, kernel_size, stride=1, padding=0, dilation=1, act=None, out_f32=False, out=None, units=None,
                        n_units=None, x_div=1, x_off=0, tile=None, nt=None, pool=False, x_per_slice=False, zero_border=(0, 0, 0, 0)):
    """The split-bf16 contraction over MFMA-ready operands (bbb_conv2d_c8x3_fwd).  x: c8 S3 [E|1, 3, Cin / 8, H, W, B, 8];
    w_tm: fp32 tap-major [E|1, Cout, kh * kw, Cin]; bias [E|1, Cout] | None -> c8 S3 [E, 3, Cout / 8, Ho, Wo, B, 8], or with
    out_f32 the fp32 batch-innermost [E, Cout, Ho, Wo, B] (the logits layer).  Work units / x_div / x_off as conv2d_chwn_forward.
    tile = 128 | 256: images per workgroup, nt = 2 | 3 | 4: 32-channel tiles per workgroup (None: the library picks by layer and
    launch size; same bits whatever the choice).
    pool = True (padding 0, even Ho and Wo, c8 S3 output): the launch also applies MaxPool2d(2, 2) to the activated output ->
    [E, 3, Cout / 8, Ho / 2, Wo / 2, B, 8], bit for bit maxpool_c8s3(conv2d_c8x3_forward(...), 2, 2); tile then means 32 | 64
    images per workgroup (its four waves own the four pixels of a window).
    zero_border = (leading rows, leading columns, trailing rows, trailing columns) of the input map that hold nothing but zeros (a
    space-to-depth block image's materialised padding, s2d_zero_border): their products are skipped -- same result, less work."""
    require_device(w_tm, bias)
    require_device(x, dtype=torch.bfloat16)
    x, w_tm = x.contiguous(), w_tm.contiguous()
    bias = None if bias is None else bias.contiguous()
    if x.dim() != 7 or x.shape[1] != 3 or x.shape[6] != 8 or w_tm.dim() != 4:
        raise _lib.BBBHipError("c8 S3 input [E|1, 3, Cin / 8, H, W, B, 8] and tap-major weights [E|1, Cout, kh * kw, Cin] expected")
    kh, kw = _pair(kernel_size)
    Ex, _, CG, H, W, B, _ = x.shape
    Ew, Cout, T, Cin = w_tm.shape
    if T != kh * kw or Cin != CG * 8:
        raise _lib.BBBHipError(f"weights [{Cout}, {T}, {Cin}] do not match a {kh} x {kw} layer on {CG * 8} channels")
    d, ho, wo = conv_desc(B, Cin, (H, W), Cout, (kh, kw), stride, padding, dilation, act=act, x_planes=3)
    E, _, _ = slab_rule(d, Ex, Ew, units=units, n_units=n_units, x_per_slice=x_per_slice, x_div=x_div, x_off=x_off)
    if pool:
        if out_f32 or ho % 2 or wo % 2 or _pair(padding) != (0, 0):
            raise _lib.BBBHipError("pool=True: c8 S3 output, no padding, even output height and width")
        ho, wo = ho // 2, wo // 2
    if out_f32:
        shape, odt = (E, Cout, ho, wo, B), torch.float32
    else:
        if Cout % 8:
            raise _lib.BBBHipError("a c8 S3 output needs a multiple of 8 output channels")
        shape, odt = (E, 3, Cout // 8, ho, wo, B, 8), torch.bfloat16
    y = _out_tensor(out, shape, odt, x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_conv2d_c8x3_fwd(ctypes.byref(d), x.data_ptr(), w_tm.data_ptr(), ptr(bias), y.data_ptr(),
                                             c8x3_flags(out_f32, tile, zero_border, nt, bool(pool)), cur_stream(x.device)),
              "bbb_conv2d_c8x3_fwd")
    return y


# BBB_C8X3_FORM_* (include/bbb_hip.h): 32-channel tiles per workgroup x 32-image fragments per wave x output, then the LRT pair
C8X3_FORMS = tuple(f"nt{nt}-mt{mt}-{out}" for nt in (2, 3, 4) for mt in (1, 2) for out in ("s3", "f32", "pool")) + ("lrt-s3", "lrt-f32")


def c8x3_fwd_plan(x_shape, cout, kernel_size, stride=1, padding=0, dilation=1, draws=None, out_f32=False, tile=None, nt=None, pool=False,
                  lrt=False, zero_border=(0, 0, 0, 0)):
    """(form, nt, images per workgroup, items, workgroups) of the launch conv2d_c8x3_forward (lrt=False) or lrt_conv2d_c8x3_forward
    (lrt=True) makes for x_shape = [*, Cin, H, W, B] (the logical shape, not the c8 S3 one) and `draws` output slabs: form one of
    C8X3_FORMS (bbb_conv2d_c8x3_plan, the launch entries' own plan, csrc/pconv_c8x3_plan.h; host only: needs no device).  A geometry
    or a flag combination the launch refuses raises the launch's error."""
    E = int(draws) if draws is not None else x_shape[0]
    Cin, H, W, B = x_shape[-4:]
    d, _, _ = conv_desc(B, Cin, (H, W), cout, _pair(kernel_size), stride, padding, dilation, E, x_planes=6 if lrt else 3,
                        w_stride=0 if lrt else None, b_stride=0 if lrt else None)
    flags = c8x3_flags(out_f32, tile, zero_border, nt, bool(pool))
    fm, ntv, ipw, items, blocks = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(_lib.lib().bbb_conv2d_c8x3_plan(ctypes.byref(d), flags, 1 if lrt else 0, ctypes.byref(fm), ctypes.byref(ntv), ctypes.byref(ipw),
                                          ctypes.byref(items), ctypes.byref(blocks)), "bbb_conv2d_c8x3_plan")
    return C8X3_FORMS[fm.value], ntv.value, ipw.value, items.value, blocks.value


def maxpool_c8s3(x, k, s):
    """MaxPool2d(k, s) on a c8 S3 tensor [E, 3, C / 8, H, W, B, 8] (element-wise on the 16-byte channel vectors); six-plane slabs
    (the LRT chain): the maximum of the values, and the squares of the pooled values behind."""
    require_device(x, dtype=torch.bfloat16)
    x = x.contiguous()
    E, planes, CG, H, W, B, eight = x.shape
    if planes == 6:
        ho, wo = pooled_map(H, W, (k, s))
        y = torch.empty((E, 6, CG, ho, wo, B, 8), dtype=torch.bfloat16, device=x.device)
        with on_device(x.device):
            check(_lib.lib().bbb_maxpool_chwn_s3sq(x.data_ptr(), y.data_ptr(), E, CG, H, W, B * 8, int(k), int(s), cur_stream(x.device)),
                  "bbb_maxpool_chwn_s3sq")
        return y
    y = maxpool_chwn_s3(x.view(E, 3, CG, H, W, B * 8), k, s)
    return y.view(E, 3, CG, y.shape[3], y.shape[4], B, 8)


def lrt_conv2d_c8x3_forward(x, w_mu_tm, w_var_tm, b_mu, b_var, kernel_size, seed, call0, stream_id, stride=1, padding=0, dilation=1,
                            sample=True, act=None, out_f32=False, out=None, units=None, n_units=None, b_offset=0, x_per_slice=False,
                            x_div=1, x_off=0, n_slabs=None, tile=None, zero_border=(0, 0, 0, 0)):
    """The LRT layer on the split-bf16 kernel over MFMA-ready operands (bbb_lrt_conv2d_c8x3_fwd): both contractions -- (x, W_mu) and
    (x^2, W_sigma^2) -- on the 16-bit matrix pipe at fp32 accuracy, sampling epilogue as lrt_conv2d_chwn_forward's (same noise
    elements).  x: six-plane c8 S3 [E|1|S, 6, Cin / 8, H, W, B, 8]; w_mu_tm / w_var_tm: fp32 tap-major [Cout, kh * kw, Cin];
    -> six-plane c8 S3 [E, 6, Cout / 8, Ho, Wo, B, 8], or with out_f32 the fp32 [E, Cout, Ho, Wo, B].  Work units / x_div / x_off /
    b_offset / n_slabs as lrt_conv2d_chwn_forward."""
    require_device(w_mu_tm, w_var_tm, b_mu, b_var)
    require_device(x, dtype=torch.bfloat16)
    x, w_mu_tm, w_var_tm = x.contiguous(), w_mu_tm.contiguous(), w_var_tm.contiguous()
    b_mu = None if b_mu is None else b_mu.contiguous()
    b_var = None if b_var is None else b_var.contiguous()
    if x.dim() != 7 or x.shape[1] != 6 or x.shape[6] != 8 or w_mu_tm.dim() != 3 or w_var_tm.shape != w_mu_tm.shape:
        raise _lib.BBBHipError("six-plane c8 S3 input [E|1, 6, Cin / 8, H, W, B, 8] and tap-major weights [Cout, kh * kw, Cin] expected")
    kh, kw = _pair(kernel_size)
    Ex, _, CG, H, W, B, _ = x.shape
    Cout, T, Cin = w_mu_tm.shape
    if T != kh * kw or Cin != CG * 8:
        raise _lib.BBBHipError(f"weights [{Cout}, {T}, {Cin}] do not match a {kh} x {kw} layer on {CG * 8} channels")
    d, ho, wo = conv_desc(B, Cin, (H, W), Cout, (kh, kw), stride, padding, dilation, act=act, x_planes=6)
    E, _, _ = slab_rule(d, Ex, 1, units=units, n_units=n_units, x_per_slice=x_per_slice, x_div=x_div, x_off=x_off, n_slabs=n_slabs,
                        weights_shared=True)
    d.b_offset = int(b_offset)
    if out_f32:
        shape, odt = (E, Cout, ho, wo, B), torch.float32
    else:
        if Cout % 8:
            raise _lib.BBBHipError("a c8 S3 output needs a multiple of 8 output channels")
        shape, odt = (E, 6, Cout // 8, ho, wo, B, 8), torch.bfloat16
    y = _out_tensor(out, shape, odt, x.device)
    flags = c8x3_flags(out_f32, tile, zero_border)
    with on_device(x.device):
        check(_lib.lib().bbb_lrt_conv2d_c8x3_fwd(ctypes.byref(d), x.data_ptr(), w_mu_tm.data_ptr(), w_var_tm.data_ptr(), ptr(b_mu), ptr(b_var),
                                                 y.data_ptr(), seed, call0 & 0xFFFFFFFF, stream_id, 1 if sample else 0,
                                                 rng.call_dev_ptr(x.device), flags, cur_stream(x.device)), "bbb_lrt_conv2d_c8x3_fwd")
    return y


def lrt_conv2d_chwn_forward(x, w_mu, w_var, b_mu, b_var, seed, call0, stream_id, stride=1, padding=0, dilation=1,
                            sample=True, eps=None, want_moments=False, act=None, units=None, n_units=None, b_offset=0,
                            x_per_slice=False, x_div=1, x_off=0, n_slabs=None, pool=False):
    """LRT layer, batch-innermost.  x: [E, Cin, H, W, B] -> (y, act_mu|None, act_var|None) [E, Cout, Ho, Wo, B].
    Work units as in conv2d_chwn_forward (call0 = the call index of the first unit's draw; the noise of unit u is keyed by
    its draw and by the GLOBAL image index slice*B + b).  b_offset: global index of local image 0 (batch-parallel shards)."""
    require_device(x, w_mu, w_var, b_mu, b_var, eps)
    x = x.contiguous()
    w_mu, w_var = w_mu.contiguous(), w_var.contiguous()
    b_mu = None if b_mu is None else b_mu.contiguous()
    b_var = None if b_var is None else b_var.contiguous()
    Ex, Cin, H, W, B = x.shape
    Cout, w_cin, kh, kw = w_mu.shape
    _same_channels(Cin, w_cin)
    d, ho, wo = conv_desc(B, Cin, (H, W), Cout, (kh, kw), stride, padding, dilation, act=act)
    E, _, _ = slab_rule(d, Ex, 1, units=units, n_units=n_units, x_per_slice=x_per_slice, x_div=x_div, x_off=x_off, n_slabs=n_slabs,
                        weights_shared=True)
    d.b_offset = int(b_offset)
    if pool:
        # [activation ->] MaxPool2d(2, 2) inside the launch (pconv_body.cuh, POOL + LRT): the sampling epilogue per window pixel with
        # the CONV output's noise elements, running maximum in registers -- bit for bit maxpool_chwn of the unpooled launch
        if want_moments or ho % 2 or wo % 2:
            raise _lib.BBBHipError("pool=True: even output height / width, and no moment outputs (the unpooled pixels are not kept)")
        d.pool = 1
        ho, wo = ho // 2, wo // 2
    shape = (E, Cout, ho, wo, B)
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    am = torch.empty(shape, dtype=torch.float32, device=x.device) if want_moments else None
    av = torch.empty(shape, dtype=torch.float32, device=x.device) if want_moments else None
    if eps is not None:
        eps = eps.contiguous()
    with on_device(x.device):
        ks, scr = _split_scratch(d, True, x.device)
        if pool and ks > 1:
            raise _lib.BBBHipError("pool=True: this layer's contraction is split (conv + maxpool_chwn instead)")
        check(_lib.lib().bbb_lrt_conv2d_chwn_splitk_fwd(ctypes.byref(d), x.data_ptr(), w_mu.data_ptr(), w_var.data_ptr(), ptr(b_mu),
                                                        ptr(b_var), y.data_ptr(), ptr(am), ptr(av), ptr(eps), seed,
                                                        call0 & 0xFFFFFFFF, stream_id, 1 if sample else 0,
                                                        rng.call_dev_ptr(x.device), ks, ptr(scr), 0 if scr is None else scr.numel(),
                                                        cur_stream(x.device)),
              "bbb_lrt_conv2d_chwn_splitk_fwd")
    return y, am, av


FP32_FORMS = ("bbb-64-ilv", "bbb-64", "bbb-128-ilv", "bbb-128", "bbb-seq64-ilv", "bbb-seq64", "bbb-seq128-ilv", "bbb-seq128",
              "bbb-cross", "bbb-pool", "lrt-64-ilv", "lrt-64", "lrt-seq64", "lrt-cross", "lrt-pool")      # BBB_FP32_FORM_* (include/bbb_hip.h)


def fp32_fwd_plan(x_shape, w_shape, stride=1, padding=0, dilation=1, draws=None, lrt=False, pool=False, k_split=None, scratch=True):
    """(form, images per item, interleaved staging, items, workgroups, k_split) of the launch conv2d_chwn_forward (lrt=False) or
    lrt_conv2d_chwn_forward (lrt=True) makes for x_shape = [*, Cin, H, W, B], w_shape = [*, Cout, Cin, kh, kw] and `draws` output
    slabs: form one of FP32_FORMS (bbb_conv2d_chwn_plan, the launch entries' own plan; host only: needs no device).  k_split: None =
    the layer's own split when ops.current_config().split_k is on (what the two forwards pass), else the value to ask about;
    scratch: the launch gets scratch for its cross-workgroup form, as the two forwards give it.  A geometry or a k_split the launch
    refuses raises the launch's error."""
    E = int(draws) if draws is not None else x_shape[0]
    Cin, H, W, B = x_shape[-4:]
    d, _, _ = conv_desc(B, Cin, (H, W), w_shape[-4], tuple(w_shape[-2:]), stride, padding, dilation, E, w_stride=0, b_stride=0)
    d.pool = 1 if pool else 0
    if k_split is None:
        ks = ctypes.c_int32(1)
        if current_config().split_k:
            _lib.lib().bbb_conv2d_chwn_splitk_scratch(ctypes.byref(d), 1 if lrt else 0, ctypes.byref(ks))
        k_split = ks.value
    fm, bm, ilv, items, blocks = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(_lib.lib().bbb_conv2d_chwn_plan(ctypes.byref(d), 1 if lrt else 0, int(k_split), 1 if scratch else 0, ctypes.byref(fm),
                                          ctypes.byref(bm), ctypes.byref(ilv), ctypes.byref(items), ctypes.byref(blocks)),
          "bbb_conv2d_chwn_plan")
    return FP32_FORMS[fm.value], bm.value, bool(ilv.value), items.value, blocks.value, int(k_split)


def lrt_sample_chwn(act_mu, act_var, draws, seed, call0, stream_id, act=None, b_offset=0):
    """E draws y[e] = act(act_mu + sqrt(act_var) * eps[e]) from one pair of LRT moments [1|-, C, Ho, Wo, B] ->
    [E, C, Ho, Wo, B]; eps as the LRT GEMM epilogue would draw it for draw e."""
    require_device(act_mu, act_var)
    act_mu, act_var = act_mu.contiguous(), act_var.contiguous()
    C, Ho, Wo, B = act_mu.shape[-4:]
    y = torch.empty((draws, C, Ho, Wo, B), dtype=torch.float32, device=act_mu.device)
    with on_device(act_mu.device):
        check(_lib.lib().bbb_lrt_sample_chwn(act_mu.data_ptr(), act_var.data_ptr(), y.data_ptr(), draws, C, Ho * Wo, B, int(b_offset),
                                             ACT_CODE[act], seed, call0 & 0xFFFFFFFF, stream_id,
                                             rng.call_dev_ptr(act_mu.device), cur_stream(act_mu.device)), "bbb_lrt_sample_chwn")
    return y


# ---- pooling (csrc/pool2d.hip, pool2d_bf16.hip; what a launch checks: csrc/pool_plan.h; what is admitted: bbb_hip/pool_desc.py) ----
def _planes_of(shape):
    """(leading dims, H, W, B, planes) of planes [..., H, W, B]: planes = the product of the leading dims."""
    *lead, H, W, B = shape
    planes = 1
    for v in lead:
        planes *= v
    return lead, H, W, B, planes


def _grad_buffers(like, planes, dtype, pad_planes, pair=False):
    """The output of a pooling / activation backward over the `planes` planes [*lead, H, W, B] of the contiguous tensor `like`, in
    `dtype` (None: like's): dense, or (pad_planes) every plane at padded_plane_pitch(H * W * B) -> (buf, out, pitch): what the launch writes, the
    same as a tensor of like's shape, and the entry's out_plane_pitch (0 = dense).  pair (the LRT forms): two of them one allocation
    apart -- buf and out carry a leading 2."""
    shape = like.shape
    K = shape[-3] * shape[-2] * shape[-1]
    pitch = padded_plane_pitch(K) if pad_planes else K
    if pitch == K and not pair:
        buf = torch.empty_like(like) if dtype is None else torch.empty_like(like, dtype=dtype)
        return buf, buf, 0
    dtype = like.dtype if dtype is None else dtype
    if pair:
        shape = (2,) + tuple(shape)
    if pitch == K:
        buf = torch.empty(shape, dtype=dtype, device=like.device)
        return buf, buf, 0
    buf = torch.empty(((2, planes, pitch) if pair else (planes, pitch)), dtype=dtype, device=like.device)
    return buf, buf[..., :K].view(shape), pitch


def _pooled_grad_shape(g_out, planes, H, W, B, avg, bf16=False):
    """The average-pool backward kernels index g_out by the pooled map: refuse a gradient of any other size before the launch."""
    ho, wo, _, _ = pool_plan("avg", H, W, B, *avg, planes=max(planes, 1) if bf16 else planes, bf16=bf16)     # (no planes: the fp32 plan refuses)
    if g_out.numel() != planes * ho * wo * B:
        raise _lib.BBBHipError("average-pool backward: g_out must hold %d planes of the pooled map %d x %d x %d" % (planes, ho, wo, B))


def maxpool_chwn(x, k, s):
    """MaxPool2d(k, s) on [..., H, W, B] (B innermost, B % 4 == 0)."""
    require_device(x)
    x = x.contiguous()
    lead, H, W, B, planes = _planes_of(x.shape)
    y = torch.empty((*lead, *pooled_map(H, W, (k, s)), B), dtype=torch.float32, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_maxpool_chwn(x.data_ptr(), y.data_ptr(), planes, H, W, B, int(k), int(s), cur_stream(x.device)),
              "bbb_maxpool_chwn")
    return y


def avgpool_chwn(x, kernel, stride, padding=0, count_include_pad=True):
    """AvgPool2d(kernel, stride, padding, count_include_pad=) in floor mode on [..., H, W, B] (B innermost, B % 4 == 0): the taps
    inside the map added in scan order, one IEEE division (bbb_avgpool_chwn)."""
    require_device(x)
    x = x.contiguous()
    lead, H, W, B, planes = _planes_of(x.shape)
    d = _pool_desc(H, W, B, kernel, stride, padding, count_include_pad)
    ho, wo, _, _ = avgpool_plan(H, W, B, kernel, stride, padding, count_include_pad, planes=max(planes, 1))
    y = torch.empty((*lead, ho, wo, B), dtype=torch.float32, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_avgpool_chwn(ctypes.byref(d), x.data_ptr(), y.data_ptr(), planes, cur_stream(x.device)), "bbb_avgpool_chwn")
    return y


# ---- bf16 storage path (BASELINE.json configs[1]) -------------------------------------------------------------------

def bf16_row_pitch(k):
    return (int(k) + 7) & ~7


def bf16_tap_major(shape):
    """Conv weights [Cout, Cin, kh, kw] with Cin % 8 == 0 and more than one tap are stored tap-major ((r, q, ci) order
    inside a row): the bf16 GEMM can then skip the taps that fall into the padding."""
    return len(shape) == 4 and shape[1] % 8 == 0 and shape[2] * shape[3] > 1


def sample_weights_bf16(mus, rhos, prior_mu, prior_sigma, stream_ids, seed, call0, draws, eps=None, priors=None):
    """The fused reparam + KL pass with the sampled WEIGHT matrices written as bf16 in the bf16 GEMM's operand layout
    ([draws, rows, pitch], pitch = row length rounded up to 8, pad zero; tap-major column order where bf16_tap_major says
    so) and 1-d tensors (biases) kept fp32.  Inference only.  Returns (kl, [tensors])."""
    if len(mus) == 0 or len(mus) > _lib.MAX_SEGMENTS:
        raise _lib.BBBHipError(f"1..{_lib.MAX_SEGMENTS} tensors per launch, got {len(mus)}")
    require_device(*mus, *rhos)
    dev = mus[0].device
    mus = [m.detach().contiguous() for m in mus]
    rhos = [r.detach().contiguous() for r in rhos]
    outs, row_lens, taps = [], [], []
    for m in mus:
        if m.dim() >= 2:
            rows, k = m.shape[0], m.numel() // m.shape[0]
            outs.append(torch.empty((draws, rows, bf16_row_pitch(k)), dtype=torch.bfloat16, device=dev))   # pad written by the kernel
            row_lens.append(k)
            taps.append(m.shape[2] * m.shape[3] if bf16_tap_major(tuple(m.shape)) else 0)
        else:
            outs.append(torch.empty((draws,) + tuple(m.shape), dtype=torch.float32, device=dev))
            row_lens.append(0)
            taps.append(0)
    if eps is not None:
        eps = [e.contiguous() for e in eps]
        require_device(*eps)
    segs = _segments(mus, rhos, outs, None, eps, stream_ids, draws)
    for i, (o, rl, tp) in enumerate(zip(outs, row_lens, taps)):
        if rl:
            segs[i].w_row_len = rl
            segs[i].w_taps = tp
            segs[i].draw_stride = o.shape[1] * o.shape[2]
    kl = torch.empty((), dtype=torch.float32, device=dev)
    L = _lib.lib()
    parts = _partials(dev, L.bbb_reparam_partials(segs, len(mus)))
    with on_device(dev):
        _reparam_fwd(segs, _prior_segments(priors, mus), len(mus), draws, float(prior_mu), float(prior_sigma), seed, call0 & 0xFFFFFFFF,
                     0, ptr(parts), ptr(kl), 0, rng.call_dev_ptr(dev), cur_stream(dev))
    return kl, outs


def sample_weights_tm(mus, rhos, prior_mu, prior_sigma, stream_ids, seed, call0, draws, tap_major, priors=None):
    """The fused reparam + KL pass with the conv weights flagged in `tap_major` (one bool per tensor) written TAP-MAJOR, fp32
    [draws, Cout, kh * kw, Cin] (bbb_segment_t::w_tm_cin: the weight operand of conv2d_c8x3_forward), every other tensor dense
    [draws, *shape].  Same noise elements, same KL bits as the dense launch (w_tap_major(dense) == this, bit for bit).
    Inference only.  Returns (kl, [tensors])."""
    if len(mus) == 0 or len(mus) > _lib.MAX_SEGMENTS:
        raise _lib.BBBHipError(f"1..{_lib.MAX_SEGMENTS} tensors per launch, got {len(mus)}")
    require_device(*mus, *rhos)
    dev = mus[0].device
    mus = [m.detach().contiguous() for m in mus]
    rhos = [r.detach().contiguous() for r in rhos]
    outs = []
    for m, tm in zip(mus, tap_major):
        if tm:
            if m.dim() != 4 or m.shape[1] % 8 or m.shape[2] * m.shape[3] < 2:
                raise _lib.BBBHipError("tap-major output: conv weights [Cout, Cin, kh, kw] with Cin % 8 == 0 and more than one tap")
            outs.append(torch.empty((draws, m.shape[0], m.shape[2] * m.shape[3], m.shape[1]), dtype=torch.float32, device=dev))
        else:
            outs.append(torch.empty((draws,) + tuple(m.shape), dtype=torch.float32, device=dev))
    segs = _segments(mus, rhos, outs, None, None, stream_ids, draws)
    for i, (m, tm) in enumerate(zip(mus, tap_major)):
        if tm:
            segs[i].w_taps = m.shape[2] * m.shape[3]
            segs[i].w_tm_cin = m.shape[1]
    kl = torch.empty((), dtype=torch.float32, device=dev)
    L = _lib.lib()
    parts = _partials(dev, L.bbb_reparam_partials(segs, len(mus)))
    with on_device(dev):
        _reparam_fwd(segs, _prior_segments(priors, mus), len(mus), draws, float(prior_mu), float(prior_sigma), seed, call0 & 0xFFFFFFFF,
                     0, ptr(parts), ptr(kl), 0, rng.call_dev_ptr(dev), cur_stream(dev))
    return kl, outs


def to_batch_innermost_bf16(x):
    """fp32 [B, C, H, W] -> bf16 [C, H, W, B] (one rounding, nearest-even)."""
    require_device(x)
    x = x.contiguous()
    B = x.shape[0]
    plane = x.numel() // B
    y = torch.empty(tuple(x.shape[1:]) + (B,), dtype=torch.bfloat16, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_nchw_to_chwn_bf16(x.data_ptr(), y.data_ptr(), B, plane, cur_stream(x.device)), "bbb_nchw_to_chwn_bf16")
    return y


def to_batch_innermost_bf16_slices(x, slices):
    """fp32 [S*Bs, C, H, W] -> bf16 [S, C, H, W, Bs] in one launch."""
    require_device(x)
    x = x.contiguous()
    Bs = x.shape[0] // slices
    plane = x.numel() // x.shape[0]
    y = torch.empty((slices,) + tuple(x.shape[1:]) + (Bs,), dtype=torch.bfloat16, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_nchw_to_chwn_bf16_slices(x.data_ptr(), y.data_ptr(), Bs, plane, int(slices), cur_stream(x.device)),
              "bbb_nchw_to_chwn_bf16_slices")
    return y


def bf16_pool_fusion_ok(cin_khkw, tap_major, out_f32, pool_module, x_shape=None, geom=None, draws=1):
    """Should conv2d_chwn_bf16_forward(..., pool=(k, s)) replace conv + maxpool_chwn_bf16(k, s)?  First layers with a short
    contraction (row pitch <= 128: 3Conv3FC conv1, LeNet conv1 -- pconv_bf16_smallk_pool_kernel) followed by [activation ->]
    MaxPool2d(2, 2) or MaxPool2d(3, 2) without padding / dilation / ceil_mode.  Same values as the two launches (the maximum is
    taken before bias, activation and rounding, which are non-decreasing), so the choice never changes a result.
    x_shape [*, Cin, H, W, B] + geom (stride, padding, dilation) + draws: the launch (the thresholds of the current LaunchConfig;
    0 = always: the library picks the window-resident form for small launches and the strip form for large ones, and one of them
    beats the two launches at every size measured -- 3Conv3FC conv1 + pool1 at bs 256, us per launch: 1 step 18.4 -> 16.8, 4 steps
    46.5 -> 37.4, 16 steps 167 -> 125; profiles/r05_notes.md section 3).  Without x_shape: only whether the library HAS the form."""
    if not current_config().pool_fusion or pool_module is None or tap_major or out_f32:
        return False
    cin, kh, kw = cin_khkw
    if bf16_row_pitch(cin * kh * kw) > 128:
        return False
    pr = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    ks = (pr(pool_module.kernel_size), pr(pool_module.stride if pool_module.stride is not None else pool_module.kernel_size))
    if ks not in (((2, 2), (2, 2)), ((3, 3), (2, 2))):
        return False
    if not (pr(pool_module.padding) == (0, 0) and pr(pool_module.dilation) == (1, 1) and not pool_module.ceil_mode and
            not getattr(pool_module, "return_indices", False)):
        return False
    if x_shape is None:
        return True
    H, W, B = x_shape[-3], x_shape[-2], x_shape[-1]
    ho, wo = out_map(H, W, (kh, kw), *geom)
    pk, pst = ks[0][0], ks[1][0]
    if ho < pk or wo < pk:
        return False
    rows = int(draws) * -(-B // 256) * pooled_map(ho, wo, (pk, pst))[0]
    cfg = current_config()
    return rows >= (cfg.bf16_pool_fuse_min_rows_overlapped if cfg.launches_overlap else cfg.bf16_pool_fuse_min_rows)


def conv2d_chwn_bf16_forward(x, w, bias, cin_khkw, stride=1, padding=0, dilation=1, act=None, out_f32=False, out=None,
                             tap_major=False, units=None, n_units=None, x_per_slice=False, x_div=1, x_off=0, pool=None,
                             out_c8=False):
    """bf16 batch-innermost conv.  x: [E|1, Cin, H, W, B] bf16 (B % 8 == 0); w: [E|1, Cout, Kp] bf16 as written by
    sample_weights_bf16 (tap_major = its column order, see bf16_tap_major); cin_khkw = (Cin, kh, kw); bias [E|1, Cout]
    fp32 or None -> y [E, Cout, Ho, Wo, B] bf16 (fp32 when out_f32).
    pool = (k, s): the launch also applies MaxPool2d(k, s) to the activated output -> [E, Cout, Hp, Wp, B] (bf16_pool_fusion_ok
    says when the library has that form).
    Channel-interleaved activations ("c8", see to_c8): a 6-d x [E|1, Cin / 8, H, W, B, 8] is read as such (bf16_c8_input_ok says
    which layers have that form); out_c8=True writes y as [E, Cout / 8, Ho, Wo, B, 8] (bf16_c8_output_ok)."""
    require_device(x, w, dtype=torch.bfloat16)
    require_device(bias)
    x, w = x.contiguous(), w.contiguous()
    x_c8 = x.dim() == 6
    if x_c8:
        if x.shape[5] != 8:
            raise _lib.BBBHipError("a 6-d input is [E, Cin / 8, H, W, B, 8]")
        x = x.view(x.shape[0], x.shape[1] * 8, x.shape[2], x.shape[3], x.shape[4])      # same bytes; only the element order differs
    bias = None if bias is None else bias.contiguous()
    cin, kh, kw = cin_khkw
    Ex, Cin, H, W, B = x.shape
    Ew, Cout, Kp = w.shape
    if Cin != cin or Kp != bf16_row_pitch(cin * kh * kw):
        raise _lib.BBBHipError("weight pitch / channel count do not match the geometry")
    d, ho, wo = conv_desc(B, Cin, (H, W), Cout, (kh, kw), stride, padding, dilation, act=act, w_stride=Cout * Kp)
    E, _, _ = slab_rule(d, Ex, Ew, units=units, n_units=n_units, x_per_slice=x_per_slice, x_div=x_div, x_off=x_off)
    if bias is None or (bias.shape[0] == 1 and E > 1 and not d.unit_div):
        d.b_draw_stride = 0
    if pool is not None:
        d.pool = pool_code(pool)
        ho, wo = pooled_map(ho, wo, pool)
    if out_c8 and (out_f32 or Cout % 8):
        raise _lib.BBBHipError("out_c8: bf16 output with a multiple of 8 channels")
    y = _out_tensor(out, (E, Cout // 8, ho, wo, B, 8) if out_c8 else (E, Cout, ho, wo, B), torch.float32 if out_f32 else torch.bfloat16,
                    x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_conv2d_chwn_bf16_fwd(ctypes.byref(d), x.data_ptr(), w.data_ptr(), ptr(bias), y.data_ptr(),
                                                  bf16_flags(out_f32, tap_major, x_c8, out_c8), cur_stream(x.device)),
              "bbb_conv2d_chwn_bf16_fwd")
    return y


def lrt_weights_bf16(weights):
    """The W_mu / sigma^2 operands of lrt_conv2d_chwn_bf16_forward: fp32 [Cout, Cin, kh, kw] or [Cout, K] tensors -> bf16
    [Cout, Kp] rows (Kp = bf16_row_pitch(K), zero pad; tap-major column order where bf16_tap_major says so -- the layout
    sample_weights_bf16 writes for BBB layers), one rounding each.  Every tensor of the list in one launch per
    _lib.BF16_ROWS_MAX_SEGMENTS of them (both operands of every layer of a model: one launch per step)."""
    require_device(*weights)
    weights = [w.detach().contiguous() for w in weights]
    if not weights:
        return []
    dev = weights[0].device
    outs = []
    for w in weights:
        if w.dim() not in (2, 4):
            raise _lib.BBBHipError("lrt_weights_bf16: [Cout, Cin, kh, kw] or [Cout, K] tensors")
        outs.append(torch.empty((w.shape[0], bf16_row_pitch(w.numel() // w.shape[0])), dtype=torch.bfloat16, device=dev))
    n = _lib.BF16_ROWS_MAX_SEGMENTS
    with on_device(dev):
        for s0 in range(0, len(weights), n):
            ws, os_ = weights[s0:s0 + n], outs[s0:s0 + n]
            segs = (_lib.RowsSegment * len(ws))()
            for sg, w, o in zip(segs, ws, os_):
                sg.src, sg.dst, sg.rows, sg.row_len = w.data_ptr(), o.data_ptr(), w.shape[0], w.numel() // w.shape[0]
                sg.taps = w.shape[2] * w.shape[3] if bf16_tap_major(tuple(w.shape)) else 0
            check(_lib.lib().bbb_lrt_weights_bf16(segs, len(ws), cur_stream(dev)), "bbb_lrt_weights_bf16")
    return outs


def _bf16_plan_desc(x_shape, cout, cin_khkw, stride, padding, dilation, draws, w_stride):
    """The descriptor the bf16 plan queries ask about: `draws` (default x_shape[0]) slabs of x_shape = [E, Cin, H, W, B]."""
    _, Cin, H, W, B = x_shape
    return conv_desc(B, Cin, (H, W), cout, cin_khkw[1:], stride, padding, dilation, int(draws) if draws is not None else x_shape[0],
                     w_stride=w_stride, b_stride=0)[0]


def lrt_bf16_plan(x_shape, cout, cin_khkw, stride=1, padding=0, dilation=1, draws=None):
    """(tile shape 22 | 14 | 12, k-groups, wave-specialised) the library picks for lrt_conv2d_chwn_bf16_forward on this geometry
    (bbb_lrt_conv2d_chwn_bf16_plan; host only: needs no device)."""
    d = _bf16_plan_desc(x_shape, cout, cin_khkw, stride, padding, dilation, draws, 0)
    sh, kg, ws = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    check(_lib.lib().bbb_lrt_conv2d_chwn_bf16_plan(ctypes.byref(d), 0, ctypes.byref(sh), ctypes.byref(kg), ctypes.byref(ws)),
          "bbb_lrt_conv2d_chwn_bf16_plan")
    return sh.value, kg.value, bool(ws.value)


BF16_FORMS = ("general", "smallk", "smallk-pool", "smallk-poolwin", "strip8", "fewout")      # BBB_BF16_FORM_* (include/bbb_hip.h)


def bf16_fwd_plan(x_shape, cout, cin_khkw, stride=1, padding=0, dilation=1, draws=None, out_f32=False, tap_major=False, x_c8=False,
                  out_c8=False, pool=None):
    """(form, tile shape, k-groups, wave-specialised) the library picks for conv2d_chwn_bf16_forward on x_shape = [E, Cin, H, W, B]:
    form one of BF16_FORMS; for "general" the tile shape 22 | 14 | 12, 1 | 2 | 4 k-groups and whether the launch is
    wave-specialised, (0, 0, False) otherwise (bbb_conv2d_chwn_bf16_plan, the launch entry's own plan; host only: needs no device).
    A geometry the launch refuses raises the launch's error."""
    d = _bf16_plan_desc(x_shape, cout, cin_khkw, stride, padding, dilation, draws,
                        cout * bf16_row_pitch(cin_khkw[0] * cin_khkw[1] * cin_khkw[2]))
    d.pool = pool_code(pool)
    flags = bf16_flags(out_f32, tap_major, x_c8, out_c8)
    fm, sh, kg, ws = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    check(_lib.lib().bbb_conv2d_chwn_bf16_plan(ctypes.byref(d), flags, ctypes.byref(fm), ctypes.byref(sh), ctypes.byref(kg),
                                               ctypes.byref(ws)), "bbb_conv2d_chwn_bf16_plan")
    return BF16_FORMS[fm.value], sh.value, kg.value, bool(ws.value)


def lrt_conv2d_chwn_bf16_forward(x, w_mu, w_var, b_mu, b_var, cin_khkw, seed, call0, stream_id, stride=1, padding=0, dilation=1,
                                 sample=True, want_moments=False, moments_only=False, act=None, out_f32=False, out=None,
                                 tap_major=False, b_offset=0, x_div=1, x_off=0, n_slabs=None):
    """LRT layer on bf16 storage, batch-innermost.  x: [E|1, Cin, H, W, B] bf16 (B % 8 == 0); w_mu / w_var: bf16 [Cout, Kp] rows
    from lrt_weights_bf16 (tap_major = their column order), shared by every slab; b_mu / b_var fp32 [Cout] or None ->
    (y, act_mu | None, act_var | None): y [E, Cout, Ho, Wo, B] bf16 (fp32 when out_f32) = act(act_mu + sqrt(act_var) * eps) with
    act_mu = sum x bf16(W_mu) + b_mu, act_var = 1e-16 + sum bf16(x^2) bf16(sigma^2) + b_var and eps the fp32 LRT kernel's element
    (call0 + slab, stream_id, canonical index keyed by b_offset + image); the moments fp32.  moments_only: no y (sample=False).
    x_div / x_off / n_slabs: several steps per launch, as in lrt_conv2d_chwn_forward."""
    require_device(x, w_mu, w_var, dtype=torch.bfloat16)
    require_device(b_mu, b_var)
    x, w_mu, w_var = x.contiguous(), w_mu.contiguous(), w_var.contiguous()
    b_mu = None if b_mu is None else b_mu.contiguous()
    b_var = None if b_var is None else b_var.contiguous()
    cin, kh, kw = cin_khkw
    if x.shape[1] != cin or w_mu.shape != w_var.shape or w_mu.dim() != 2 or w_mu.shape[1] != bf16_row_pitch(cin * kh * kw):
        raise _lib.BBBHipError("weight pitch / channel count do not match the geometry")
    if moments_only and sample:
        raise _lib.BBBHipError("moments_only: sample=False")
    (Ex, _, H, W, B), cout = x.shape, w_mu.shape[0]
    d, ho, wo = conv_desc(B, cin, (H, W), cout, (kh, kw), stride, padding, dilation, act=act)
    E, _, _ = slab_rule(d, Ex, 1, x_div=x_div, x_off=x_off, n_slabs=n_slabs, weights_shared=True)
    d.b_offset = int(b_offset)
    shape = (E, cout, ho, wo, B)
    y = None if moments_only else _out_tensor(out, shape, torch.float32 if out_f32 else torch.bfloat16, x.device)
    moments = want_moments or moments_only
    am = torch.empty(shape, dtype=torch.float32, device=x.device) if moments else None
    av = torch.empty(shape, dtype=torch.float32, device=x.device) if moments else None
    with on_device(x.device):
        check(_lib.lib().bbb_lrt_conv2d_chwn_bf16_fwd(ctypes.byref(d), x.data_ptr(), w_mu.data_ptr(), w_var.data_ptr(), ptr(b_mu),
                                                      ptr(b_var), ptr(y), ptr(am), ptr(av), seed, call0 & 0xFFFFFFFF, stream_id,
                                                      1 if sample else 0, rng.call_dev_ptr(x.device),
                                                      bf16_flags(out_f32, tap_major), cur_stream(x.device)),
              "bbb_lrt_conv2d_chwn_bf16_fwd")
    return y, am, av


def lrt_sample_chwn_bf16(act_mu, act_var, draws, seed, call0, stream_id, act=None, b_offset=0):
    """lrt_sample_chwn with bf16 output: E draws from one pair of fp32 moments [1|-, C, Ho, Wo, B] (B % 8 == 0) -> bf16
    [E, C, Ho, Wo, B]; bit for bit what E sampling launches of lrt_conv2d_chwn_bf16_forward store."""
    require_device(act_mu, act_var)
    act_mu, act_var = act_mu.contiguous(), act_var.contiguous()
    C, Ho, Wo, B = act_mu.shape[-4:]
    y = torch.empty((draws, C, Ho, Wo, B), dtype=torch.bfloat16, device=act_mu.device)
    with on_device(act_mu.device):
        check(_lib.lib().bbb_lrt_sample_chwn_bf16(act_mu.data_ptr(), act_var.data_ptr(), y.data_ptr(), draws, C, Ho * Wo, B,
                                                  int(b_offset), ACT_CODE[act], seed, call0 & 0xFFFFFFFF,
                                                  stream_id, rng.call_dev_ptr(act_mu.device), cur_stream(act_mu.device)),
              "bbb_lrt_sample_chwn_bf16")
    return y


def bf16_c8_input_ok(cin_khkw, geom, tap_major, out_f32, x_shape=None, draws=1):
    """Does conv2d_chwn_bf16_forward have a kernel that reads THIS layer's input channel-interleaved (a 6-d x, see to_c8), and
    should the launch take it?  pconv_bf16_strip8_kernel: tap-major rows of 32 input channels, 5 x 5 taps, stride 1, no dilation,
    padding < 5, bf16 output (3Conv3FC conv2: 131-153 us on the general kernel at bs 256 x 16 steps per launch, 88-100 us here).  The
    producer must then write that layout (out_c8: the pooled first-layer forms and the strip form itself).
    x_shape (H, W, B) + draws: the launch, for LaunchConfig.bf16_c8_min_items (strip workgroups: a strip of three pixels of an output
    row x 64 channels x 128 images).  0 = always: 3Conv3FC conv2 at bs 256, us per launch, general kernel / strip form: 1 step 18.1 /
    15.0, 2 steps 33.7 / 20.8, 4 steps 43.4 / 30.9, 8 steps 71.3 / 47.8, 16 steps 131-153 / 88-100 (profiles/r05_notes.md section 8).
    Values: the strip form always adds a pixel's taps in one fixed order (the general kernel's order with ONE k-group, which is what
    that kernel uses for launches of 512 workgroups and more) -- bit-identical there, rounding-level differences against the
    general kernel's two- / four-group launches."""
    cfg = current_config()
    if not cfg.bf16_c8 or not tap_major or out_f32:
        return False
    cin, kh, kw = cin_khkw
    (sh, sw), (ph, pw), (dh, dw) = _pair(geom[0]), _pair(geom[1]), _pair(geom[2])
    if not (cin == 32 and (kh, kw) == (5, 5) and (sh, sw) == (1, 1) and (dh, dw) == (1, 1) and ph < kh and pw < kw):
        return False
    if x_shape is None:
        return True
    H, W, B = x_shape
    ho, wo = H + 2 * ph - kh + 1, W + 2 * pw - kw + 1
    if ho < 1 or wo < 1:
        return False
    return int(draws) * ho * -(-wo // 3) * -(-B // 128) >= cfg.bf16_c8_min_items


def to_c8(x):
    """[E, C, H, W, B] -> the channel-interleaved layout [E, C / 8, H, W, B, 8] (8 consecutive channels of an image adjacent in
    memory: an MFMA operand of the bf16 kernels is then one 16-byte load).  A torch permute: tests and one-off conversions; inside
    the batched path the producing kernel writes the layout itself (out_c8)."""
    E, C, H, W, B = x.shape
    return x.view(E, C // 8, 8, H, W, B).permute(0, 1, 3, 4, 5, 2).contiguous()


def from_c8(x):
    """The inverse of to_c8: [E, C / 8, H, W, B, 8] -> [E, C, H, W, B]."""
    E, C8, H, W, B, _ = x.shape
    return x.permute(0, 1, 5, 2, 3, 4).reshape(E, C8 * 8, H, W, B).contiguous()


def maxpool_chwn_bf16(x, k, s):
    """MaxPool2d(k, s) on bf16 [..., H, W, B] (B % 8 == 0)."""
    require_device(x, dtype=torch.bfloat16)
    x = x.contiguous()
    lead, H, W, B, planes = _planes_of(x.shape)
    y = torch.empty((*lead, *pooled_map(H, W, (k, s)), B), dtype=torch.bfloat16, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_maxpool_chwn_bf16(x.data_ptr(), y.data_ptr(), planes, H, W, B, int(k), int(s), cur_stream(x.device)),
              "bbb_maxpool_chwn_bf16")
    return y


def avgpool_chwn_bf16(x, kernel, stride, padding=0, count_include_pad=True):
    """avgpool_chwn on bf16 [..., H, W, B] (B % 8 == 0): the taps inside the map added in scan order in fp32, one IEEE division, one
    rounding to bf16 (bbb_avgpool_chwn_bf16)."""
    require_device(x, dtype=torch.bfloat16)
    x = x.contiguous()
    lead, H, W, B, planes = _planes_of(x.shape)
    d = _pool_desc(H, W, B, kernel, stride, padding, count_include_pad)
    ho, wo, _, _ = avgpool_bf16_plan(H, W, B, kernel, stride, padding, count_include_pad, planes=max(planes, 1))
    y = torch.empty((*lead, ho, wo, B), dtype=torch.bfloat16, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_avgpool_chwn_bf16(ctypes.byref(d), x.data_ptr(), y.data_ptr(), planes, cur_stream(x.device)),
              "bbb_avgpool_chwn_bf16")
    return y


# Draws ONE image reduces over in a batch-innermost tail launch, at most (csrc/mc_tail_plan.h): each takes 64 images x 4 bytes of the
# workgroup's 160 KB of LDS.  The plain entry and the autograd entries stay at 512 draws.
MC_TAIL_MAX_PER_SLICE = 640
MC_TAIL_MAX_DRAWS = 512


def mc_tail_cb(logits, mean_over=0, step_end=None):
    """mc_tail for batch-innermost logits [E <= 512, C, B] -> [B, C]."""
    return mc_tail_units(logits, 1, 0, mean_over, step_end)


class _McTailCB(torch.autograd.Function):
    """lse = mc_tail_cb(logits [E, C, B]) with its backward in ONE launch (bbb_mc_tail_cb_bwd): the training step's loss tail
    (log_softmax + logmeanexp, main_bayesian.py:49-53) was ~15 ATen launches forward and backward."""

    @staticmethod
    def forward(ctx, logits, mean_over):
        logits = logits.contiguous()
        lse = mc_tail_cb(logits, mean_over=mean_over)
        ctx.save_for_backward(logits, lse)
        ctx.mean_over = int(mean_over)
        return lse

    @staticmethod
    def backward(ctx, g):
        logits, lse = ctx.saved_tensors
        g = g.contiguous()
        E, C, B = logits.shape
        out = torch.empty_like(logits)
        with on_device(logits.device):
            check(_lib.lib().bbb_mc_tail_cb_bwd(logits.data_ptr(), lse.data_ptr(), g.data_ptr(), out.data_ptr(), E, B, C, ctx.mean_over,
                                                cur_stream(logits.device)), "bbb_mc_tail_cb_bwd")
        return out, None


class _ElboCB(torch.autograd.Function):
    """(loss, lse) = the whole loss tail of a training step: log_softmax + logmeanexp (bbb_mc_tail_cb), then nll_loss(mean) *
    train_size + beta * kl in one block (bbb_elbo_cb_fwd); backward in ONE launch (bbb_elbo_cb_bwd: d loss / d logits and
    d loss / d kl).  main_bayesian.py:49-56 / metrics.py:7-14 upstream -- ~25 ATen launches forward and backward otherwise."""

    @staticmethod
    def forward(ctx, logits, kl, target, beta, train_size, mean_over):
        logits = logits.contiguous()
        E, C, B = logits.shape
        lse = mc_tail_cb(logits, mean_over=mean_over)
        klc = kl.detach().reshape(()).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        beta_t = beta if torch.is_tensor(beta) else None
        with on_device(logits.device):
            check(_lib.lib().bbb_elbo_cb_fwd(lse.data_ptr(), target.data_ptr(), klc.data_ptr(), 0.0 if beta_t is not None else float(beta),
                                             ptr(beta_t), float(train_size), B, C, loss.data_ptr(), cur_stream(logits.device)),
                  "bbb_elbo_cb_fwd")
        ctx.save_for_backward(logits, lse, target)
        ctx.beta, ctx.beta_t, ctx.train_size, ctx.mean_over = (None if beta_t is not None else float(beta)), beta_t, float(train_size), int(mean_over)
        ctx.kl_shape = tuple(kl.shape)
        ctx.mark_non_differentiable(lse)
        return loss, lse

    @staticmethod
    def backward(ctx, g_loss, _g_lse):
        logits, lse, target = ctx.saved_tensors
        E, C, B = logits.shape
        g_loss = g_loss.to(dtype=torch.float32).reshape(()).contiguous()
        out = torch.empty_like(logits)
        g_kl = torch.empty(ctx.kl_shape, dtype=torch.float32, device=logits.device)
        with on_device(logits.device):
            check(_lib.lib().bbb_elbo_cb_bwd(logits.data_ptr(), lse.data_ptr(), target.data_ptr(), g_loss.data_ptr(),
                                             0.0 if ctx.beta_t is not None else ctx.beta, ptr(ctx.beta_t), ctx.train_size, out.data_ptr(),
                                             g_kl.data_ptr(), E, B, C, ctx.mean_over, cur_stream(logits.device)), "bbb_elbo_cb_bwd")
        return out, g_kl, None, None, None, None


def elbo_cb_ok(logits, kl, target, beta):
    """The fused loss tail takes: logits [E <= 512, C, B] fp32 on the device, a one-element fp32 kl there too, int64 targets [B] there too,
    beta a Python number or a one-element fp32 device tensor."""
    return (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3 and logits.shape[0] <= 512
            and torch.is_tensor(kl) and kl.device == logits.device and kl.dtype == torch.float32 and kl.numel() == 1
            and torch.is_tensor(target) and target.device == logits.device and target.dtype == torch.int64
            and target.dim() == 1 and target.shape[0] == logits.shape[2] and target.is_contiguous()
            and (not torch.is_tensor(beta) or (beta.device == logits.device and beta.dtype == torch.float32 and beta.numel() == 1
                                               and not beta.requires_grad)))


def elbo_cb_autograd(logits, kl, target, beta, train_size, mean_over=0):
    """Differentiable (loss, lse [B, C]) of one Monte-Carlo training step from its logits [E, C, B] and the KL of one forward."""
    require_device(logits)
    if not elbo_cb_ok(logits, kl, target, beta):
        raise _lib.BBBHipError("elbo_cb_autograd: see elbo_cb_ok for the accepted operands")
    return _ElboCB.apply(logits, kl, target, beta, float(train_size), int(mean_over))


def mc_tail_cb_autograd(logits, mean_over=0):
    """Differentiable mc_tail_cb: logits [E, C, B] (requires grad) -> lse [B, C]."""
    require_device(logits)
    if logits.shape[0] > MC_TAIL_MAX_DRAWS:
        raise _lib.BBBHipError("too many draws for one tail launch")
    return _McTailCB.apply(logits, int(mean_over))


def mc_tail_units(logits, slices, unit_off, mean_over=0, step_end=None):
    """mc_tail_cb for a rank's work units: logits [U, C, Bs] (unit u = unit_off + e is draw u // slices, batch slice
    u % slices) -> [slices * Bs, C]; -inf rows for slices the rank holds no unit of.  U <= 4096 (512 with one slice) and at most
    640 units per slice (ceil(U / slices): the launch keeps one float per local unit and image in LDS).
    step_end = (kl_one_forward, scale, counter | None, counter_add): the end of a captured Monte-Carlo step in the same launch
    (bbb_mc_tail_units_step) -> returns (lse, kl_one_forward * scale) and adds counter_add to the int32 device counter."""
    require_device(logits)
    logits = logits.contiguous()
    U, C, Bs = logits.shape
    if int(slices) <= 0 or U > (MC_TAIL_MAX_DRAWS if int(slices) == 1 else 4096) or -(-U // int(slices)) > MC_TAIL_MAX_PER_SLICE:
        raise _lib.BBBHipError("too many draws / units for one tail launch")
    out = torch.empty((int(slices) * Bs, C), dtype=torch.float32, device=logits.device)
    L = _lib.lib()
    with on_device(logits.device):
        if step_end is None:
            check(L.bbb_mc_tail_units(logits.data_ptr(), U, int(slices), int(unit_off) % int(slices), Bs, C, int(mean_over),
                                      out.data_ptr(), cur_stream(logits.device)), "bbb_mc_tail_units")
            return out
        kl_in, scale, counter, add = step_end
        require_device(kl_in)
        kl_out = torch.empty((), dtype=torch.float32, device=logits.device)
        if counter is not None and (counter.dtype != torch.int32 or not counter.is_cuda):
            raise _lib.BBBHipError("the call counter must be an int32 device tensor")
        check(L.bbb_mc_tail_units_step(logits.data_ptr(), U, int(slices), int(unit_off) % int(slices), Bs, C, int(mean_over),
                                       out.data_ptr(), kl_in.data_ptr(), float(scale), kl_out.data_ptr(), ptr(counter),
                                       int(add) & 0xFFFFFFFF, cur_stream(logits.device)), "bbb_mc_tail_units_step")
    return out, kl_out


def mc_tail_groups(logits, groups, draws, mean_over=0, step_end=None):
    """Tail of `groups` Monte-Carlo steps that share one set of launches: logits [groups * draws, C, B] (slab g * draws + j =
    draw j of step g) -> [groups * B, C], block g = log-sum-exp over step g's draws of the per-draw log_softmax, minus
    log(mean_over) when > 0.  groups * draws <= 4096 and draws <= 640 (the LDS of the launch).  step_end as in mc_tail_units."""
    require_device(logits)
    logits = logits.contiguous()
    U, C, B = logits.shape
    if U != int(groups) * int(draws) or U > 4096 or int(draws) > MC_TAIL_MAX_PER_SLICE:
        raise _lib.BBBHipError("mc_tail_groups: logits must hold groups * draws <= 4096 slabs of at most 640 draws per step")
    out = torch.empty((int(groups) * B, C), dtype=torch.float32, device=logits.device)
    kl_in, scale, counter, add = step_end if step_end is not None else (None, 0.0, None, 0)
    require_device(kl_in)
    kl_out = torch.empty((), dtype=torch.float32, device=logits.device) if step_end is not None else None
    if counter is not None and (counter.dtype != torch.int32 or not counter.is_cuda):
        raise _lib.BBBHipError("the call counter must be an int32 device tensor")
    with on_device(logits.device):
        check(_lib.lib().bbb_mc_tail_groups_step(logits.data_ptr(), int(groups), int(draws), B, C, int(mean_over), out.data_ptr(),
                                                 ptr(kl_in), float(scale), ptr(kl_out), ptr(counter), int(add) & 0xFFFFFFFF,
                                                 cur_stream(logits.device)), "bbb_mc_tail_groups_step")
    return out if step_end is None else (out, kl_out)


def mc_tail_share(logits, steps, draws, first_off, step_end=None):
    """Tail of one rank's share of a GROUP of steps: logits [slabs, C, B], slab e = draw (first_off + e) of the draw-major (step,
    draw) enumeration of `steps` local steps with `draws` draws each -> [steps * B, C], block k = log-sum-exp over the LOCAL draws
    of local step k of the per-draw log_softmax (no mean: the ranks' blocks are combined by one more log-sum-exp; -inf where the
    share holds no draw of the step).  0 <= first_off < draws <= 640, slabs <= 4096 and first_off + slabs <= steps * draws.  step_end
    as in mc_tail_units."""
    require_device(logits)
    logits = logits.contiguous()
    U, C, B = logits.shape
    if (U > 4096 or not 0 <= int(first_off) < int(draws) or int(steps) * int(draws) < U + int(first_off)
            or int(draws) > MC_TAIL_MAX_PER_SLICE):
        raise _lib.BBBHipError("mc_tail_share: the slabs must fit the steps * draws grid, <= 4096 slabs of at most 640 draws per step")
    out = torch.empty((int(steps) * B, C), dtype=torch.float32, device=logits.device)
    kl_in, scale, counter, add = step_end if step_end is not None else (None, 0.0, None, 0)
    require_device(kl_in)
    kl_out = torch.empty((), dtype=torch.float32, device=logits.device) if step_end is not None else None
    if counter is not None and (counter.dtype != torch.int32 or not counter.is_cuda):
        raise _lib.BBBHipError("the call counter must be an int32 device tensor")
    with on_device(logits.device):
        check(_lib.lib().bbb_mc_tail_share_step(logits.data_ptr(), U, int(steps), int(draws), int(first_off), B, C, out.data_ptr(),
                                                ptr(kl_in), float(scale), ptr(kl_out), ptr(counter), int(add) & 0xFFFFFFFF,
                                                cur_stream(logits.device)), "bbb_mc_tail_share_step")
    return out if step_end is None else (out, kl_out)


def uncertainty(logits, normalized=False):
    """logits [T, B, C] -> (pred, epistemic, aleatoric), each [B, C] (see bbb_uncertainty)."""
    require_device(logits)
    logits = logits.contiguous()
    T, B, C = logits.shape
    outs = [torch.empty((B, C), dtype=torch.float32, device=logits.device) for _ in range(3)]
    with on_device(logits.device):
        check(_lib.lib().bbb_uncertainty(logits.data_ptr(), T, B, C, 1 if normalized else 0, outs[0].data_ptr(),
                                         outs[1].data_ptr(), outs[2].data_ptr(), cur_stream(logits.device)), "bbb_uncertainty")
    return tuple(outs)


# Draws one bbb_mc_uncertainty_cb launch takes (csrc/mc_uncertainty_plan.h): three floats per (draw, image) and 8 KB of row partials
# in the workgroup's 160 KB of LDS.
MC_UNCERTAINTY_MAX_DRAWS = 202
Uncertainty = collections.namedtuple("Uncertainty", "pred p_mean epistemic aleatoric entropy expected_entropy mutual_info")


def mc_uncertainty_cb(logits_cb, normalized=False, want=None):
    """Batch-innermost logits [T <= 202, C, B] -> ops.Uncertainty in one launch (bbb_mc_uncertainty_cb): pred, p_mean, epistemic,
    aleatoric [B, C] and entropy, expected_entropy, mutual_info [B], device tensors.  want: the field names to compute (None: all
    seven); the other fields are None, and a field's bits do not depend on what else was asked for."""
    require_device(logits_cb)
    want = Uncertainty._fields if want is None else tuple(want)
    unknown = [w for w in want if w not in Uncertainty._fields]
    if unknown or not want:
        raise _lib.BBBHipError(f"want must name at least one of {Uncertainty._fields}, got {want!r}")
    logits_cb = logits_cb.contiguous()
    T, C, B = logits_cb.shape
    outs = [torch.empty((B, C) if i < 4 else (B,), dtype=torch.float32, device=logits_cb.device) if f in want else None
            for i, f in enumerate(Uncertainty._fields)]
    with on_device(logits_cb.device):
        check(_lib.lib().bbb_mc_uncertainty_cb(logits_cb.data_ptr(), T, B, C, 1 if normalized else 0, *[ptr(t) for t in outs],
                                               cur_stream(logits_cb.device)), "bbb_mc_uncertainty_cb")
    return Uncertainty(*outs)


class _McUncertaintyCB(torch.autograd.Function):
    """The wanted fields of mc_uncertainty_cb(logits [T, C, B]) with their backward in ONE launch (bbb_mc_uncertainty_cb_bwd): the
    scores written as torch expressions on permuted logits are dozens of ATen launches forward and backward, and p * log p gives NaN
    gradients where a probability is 0.  The forward launch also writes p_mean for the backward when it was not asked for (a field's
    bits do not depend on what else is computed); fields that receive no gradient go down as NULL."""

    @staticmethod
    def forward(ctx, logits, normalized, want):
        logits = logits.contiguous()
        full = mc_uncertainty_cb(logits, normalized=normalized, want=want if "p_mean" in want else want + ("p_mean",))
        ctx.save_for_backward(logits, full.p_mean)
        ctx.normalized, ctx.want = bool(normalized), want
        ctx.set_materialize_grads(False)
        return tuple(getattr(full, f) for f in want)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        logits, p_mean = ctx.saved_tensors
        T, C, B = logits.shape
        ups = dict.fromkeys(Uncertainty._fields)
        for f, g in zip(ctx.want, grads):
            if g is not None:
                ups[f] = g.to(dtype=torch.float32).contiguous()
        if all(g is None for g in ups.values()):
            return None, None, None
        out = torch.empty_like(logits)
        with on_device(logits.device):
            check(_lib.lib().bbb_mc_uncertainty_cb_bwd(logits.data_ptr(), p_mean.data_ptr(), T, B, C, 1 if ctx.normalized else 0,
                                                       *[ptr(ups[f]) for f in Uncertainty._fields], out.data_ptr(),
                                                       cur_stream(logits.device)), "bbb_mc_uncertainty_cb_bwd")
        return out, None, None


def mc_uncertainty_cb_autograd(logits_cb, normalized=False, want=None):
    """Differentiable mc_uncertainty_cb: logits [T <= 202, C, B] (requires grad) -> ops.Uncertainty whose fields carry a gradient
    back to the logits; the values are bit for bit mc_uncertainty_cb's, fields not in `want` are None.  The gradient of
    mutual_info is that of its KL form (the clamp at 0 only repairs rounding); a class with probability 0 gets an exact 0 from the
    probability side, where torch expressions give NaN."""
    require_device(logits_cb)
    want = Uncertainty._fields if want is None else tuple(want)
    unknown = [w for w in want if w not in Uncertainty._fields]
    if unknown or not want:
        raise _lib.BBBHipError(f"want must name at least one of {Uncertainty._fields}, got {want!r}")
    if logits_cb.dim() != 3 or logits_cb.dtype != torch.float32:
        raise _lib.BBBHipError("mc_uncertainty_cb_autograd takes fp32 logits [T, C, B]")
    if logits_cb.shape[0] > MC_UNCERTAINTY_MAX_DRAWS:
        raise _lib.BBBHipError(f"too many draws for one uncertainty launch: {logits_cb.shape[0]} > {MC_UNCERTAINTY_MAX_DRAWS}")
    want = tuple(f for f in Uncertainty._fields if f in want)
    outs = dict(zip(want, _McUncertaintyCB.apply(logits_cb, bool(normalized), want)))
    return Uncertainty(*[outs.get(f) for f in Uncertainty._fields])


# ---- regression with a Gaussian likelihood (csrc/gauss_tail.hip; the likelihood object: likelihood.GaussianLikelihood) ----
GAUSS_MAX_DRAWS = 512
GAUSS_MAX_CHANNELS = 1024
GAUSS_MC_CODE = {"logmeanexp": 0, "mean": 1}
Moments = collections.namedtuple("Moments", "mean epistemic aleatoric total log_density")


def _gauss_shape(logits, y_dims, lik):
    """The shared middle of the six C entries: draws, batch, channels, dims, noise_sigma, log_var_min, log_var_max."""
    E, C, B = logits.shape
    return (E, B, C, int(y_dims), 0.0 if lik.noise_sigma is None else float(lik.noise_sigma), float(lik.log_var_min),
            float(lik.log_var_max))


class _GaussElboCB(torch.autograd.Function):
    """(loss, LL) = the whole loss tail of a regression step: LL [B] in one launch and the loss in a one-block launch behind it
    (bbb_gauss_elbo_cb_fwd); backward in ONE launch (bbb_gauss_elbo_cb_bwd: d loss / d logits and d loss / d kl), which recomputes
    the per-draw log-likelihoods from the logits -- about 30 ATen launches forward and backward as torch ops."""

    @staticmethod
    def forward(ctx, logits, kl, y, beta, train_size, lik, mean_over):
        logits = logits.contiguous()
        E, C, B = logits.shape
        klc = kl.detach().reshape(()).contiguous()
        ll = torch.empty((B,), dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        beta_t = beta if torch.is_tensor(beta) else None
        with on_device(logits.device):
            check(_lib.lib().bbb_gauss_elbo_cb_fwd(logits.data_ptr(), y.data_ptr(), klc.data_ptr(),
                                                   0.0 if beta_t is not None else float(beta), ptr(beta_t), float(train_size),
                                                   *_gauss_shape(logits, y.shape[1], lik), GAUSS_MC_CODE[lik.mc], int(mean_over),
                                                   ll.data_ptr(), loss.data_ptr(), cur_stream(logits.device)), "bbb_gauss_elbo_cb_fwd")
        ctx.save_for_backward(logits, y)
        ctx.beta, ctx.beta_t, ctx.train_size, ctx.mean_over = (None if beta_t is not None else float(beta)), beta_t, float(train_size), int(mean_over)
        ctx.lik, ctx.kl_shape = lik, tuple(kl.shape)
        ctx.mark_non_differentiable(ll)
        return loss, ll

    @staticmethod
    def backward(ctx, g_loss, _g_ll):
        logits, y = ctx.saved_tensors
        g_loss = g_loss.to(dtype=torch.float32).reshape(()).contiguous()
        out = torch.empty_like(logits)
        g_kl = torch.empty(ctx.kl_shape, dtype=torch.float32, device=logits.device)
        with on_device(logits.device):
            check(_lib.lib().bbb_gauss_elbo_cb_bwd(logits.data_ptr(), y.data_ptr(), g_loss.data_ptr(),
                                                   0.0 if ctx.beta_t is not None else ctx.beta, ptr(ctx.beta_t), ctx.train_size,
                                                   *_gauss_shape(logits, y.shape[1], ctx.lik), GAUSS_MC_CODE[ctx.lik.mc], ctx.mean_over,
                                                   out.data_ptr(), g_kl.data_ptr(), cur_stream(logits.device)), "bbb_gauss_elbo_cb_bwd")
        return out, g_kl, None, None, None, None, None


def gauss_elbo_cb_ok(logits, kl, y, beta, lik):
    """The fused Gaussian loss tail takes: logits [E <= 512, C <= 1024, B] fp32 on the device, a one-element fp32 kl there too, fp32
    contiguous targets y [B, D] there too with C == 2 D (lik.noise_sigma None) or C == D, beta a Python number or a one-element fp32
    device tensor."""
    return (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3
            and logits.shape[0] <= GAUSS_MAX_DRAWS and logits.shape[1] <= GAUSS_MAX_CHANNELS
            and torch.is_tensor(kl) and kl.device == logits.device and kl.dtype == torch.float32 and kl.numel() == 1
            and torch.is_tensor(y) and y.device == logits.device and y.dtype == torch.float32 and y.dim() == 2
            and y.shape[0] == logits.shape[2] and y.shape[1] > 0 and y.is_contiguous() and not y.requires_grad
            and logits.shape[1] == y.shape[1] * (2 if lik.noise_sigma is None else 1) and lik.mc in GAUSS_MC_CODE
            and (not torch.is_tensor(beta) or (beta.device == logits.device and beta.dtype == torch.float32 and beta.numel() == 1
                                               and not beta.requires_grad)))


def gauss_elbo_cb_autograd(logits, kl, y, beta, train_size, lik, mean_over=0):
    """Differentiable (loss, LL [B]) of one Monte-Carlo regression step from its logits [E, C, B], its targets y [B, D] and the KL of
    one forward under a likelihood.GaussianLikelihood; LL carries no gradient.  The arithmetic: train.gaussian_elbo's."""
    require_device(logits)
    if not gauss_elbo_cb_ok(logits, kl, y, beta, lik):
        raise _lib.BBBHipError("gauss_elbo_cb_autograd: see gauss_elbo_cb_ok for the accepted operands")
    return _GaussElboCB.apply(logits, kl, y, beta, float(train_size), lik, int(mean_over))


def gauss_moments_cb(logits, lik, y=None, want=None):
    """Batch-innermost logits [T <= 512, C, B] of a regression model -> ops.Moments in one launch (bbb_gauss_moments_cb): mean,
    epistemic, aleatoric, total [B, D] and, with targets y [B, D], log_density [B] (the log of the mixture predictive density at y),
    device tensors.  want: the field names to compute (None: all that the arguments allow); the other fields are None, and a field's
    bits do not depend on what else was asked for."""
    require_device(logits, y)
    fields = Moments._fields if y is not None else Moments._fields[:4]
    want = fields if want is None else tuple(want)
    unknown = [w for w in want if w not in fields]
    if unknown or not want:
        raise _lib.BBBHipError(f"want must name at least one of {fields}" + ("" if y is not None else " (log_density needs y)")
                               + f", got {want!r}")
    logits = logits.contiguous()
    T, C, B = logits.shape
    per = 2 if lik.noise_sigma is None else 1
    if C % per != 0 or (y is not None and (y.dim() != 2 or tuple(y.shape) != (B, C // per))):
        raise _lib.BBBHipError(f"gauss_moments_cb: logits {tuple(logits.shape)} do not fit this likelihood / y")
    D = C // per
    y = y.contiguous() if y is not None else None
    outs = [torch.empty((B, D) if i < 4 else (B,), dtype=torch.float32, device=logits.device) if f in want else None
            for i, f in enumerate(Moments._fields)]
    with on_device(logits.device):
        check(_lib.lib().bbb_gauss_moments_cb(logits.data_ptr(), ptr(y), *_gauss_shape(logits, D, lik), *[ptr(t) for t in outs],
                                              cur_stream(logits.device)), "bbb_gauss_moments_cb")
    return Moments(*outs)


def to_batch_innermost(x):
    """[B, C, H, W] -> [C, H, W, B] (LDS-tiled transpose)."""
    require_device(x)
    x = x.contiguous()
    B = x.shape[0]
    out = torch.empty(tuple(x.shape[1:]) + (B,), dtype=torch.float32, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_transpose2d(x.data_ptr(), out.data_ptr(), B, x.numel() // B, cur_stream(x.device)), "bbb_transpose2d")
    return out


def from_batch_innermost(y):
    """[C, H, W, B] -> [B, C, H, W] (the same LDS-tiled transpose, the other way round)."""
    require_device(y)
    y = y.contiguous()
    B = y.shape[-1]
    out = torch.empty((B,) + tuple(y.shape[:-1]), dtype=torch.float32, device=y.device)
    with on_device(y.device):
        check(_lib.lib().bbb_transpose2d(y.data_ptr(), out.data_ptr(), y.numel() // B, B, cur_stream(y.device)), "bbb_transpose2d")
    return out


def _layer_on_fast_kernels(x4, *operands):
    """The per-layer path of the drop-in layers (a model with forward hooks, modules the whole-model path does not know, ...):
    may THIS layer's convolution run on the batch-innermost kernel between two layout transposes?  Inference only (the
    reference-layout kernels carry the autograd wiring), a 4-d fp32 GPU batch with B % 4 == 0."""
    if not (torch.is_tensor(x4) and x4.is_cuda and x4.dim() == 4 and x4.dtype == torch.float32 and x4.shape[0] % 4 == 0 and x4.shape[0] > 0):
        return False
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x4,) + operands):
        return False
    return True


def conv2d_layer(x4, w, b, stride, padding, dilation):
    """BBB conv layer of the per-layer path: x4 [B, Cin, H, W], w [1, Cout, Cin, kh, kw], b [1, Cout] | None -> [B, Cout, Ho, Wo].
    Inference takes the pixel-major batch-innermost kernel (padding taps skipped, the layer's split contraction: the kernel of
    the whole-model path) between two transposes -- 3-5x faster than the reference-layout kernel at bs 512; everything else the
    reference-layout autograd function."""
    if _layer_on_fast_kernels(x4, w, b):
        # (the plain fmaf chain, not the layer's split contraction: bit for bit the reference-layout kernel's result, which is what
        # this path promises -- tests/test_gpu_models.py::test_batched_ensemble_equals_loop)
        with use_config(split_k=False):
            y = conv2d_chwn_forward(to_batch_innermost(x4).unsqueeze(0), w, b, stride, padding, dilation, bf16x3=False)
        return from_batch_innermost(y[0])
    return conv2d(x4.unsqueeze(0), w, b, stride, padding, dilation).squeeze(0)


def lrt_conv2d_layer(x4, w_mu, w_var, b_mu, b_var, seed, call, stream_id, stride, padding, dilation, sample, eps):
    """LRT conv layer of the per-layer path (same noise elements on either kernel: the canonical NCHW index keys them)."""
    if eps is None and _layer_on_fast_kernels(x4, w_mu, w_var, b_mu, b_var):
        with use_config(split_k=False):
            y = lrt_conv2d_chwn_forward(to_batch_innermost(x4).unsqueeze(0), w_mu, w_var, b_mu, b_var, seed, call, stream_id, stride,
                                        padding, dilation, sample=sample)[0]
        return from_batch_innermost(y[0])
    return lrt_conv2d(x4.unsqueeze(0), w_mu, w_var, b_mu, b_var, seed, call, stream_id, stride, padding, dilation, sample=sample,
                      eps=eps).squeeze(0)


def to_batch_innermost_slices(x, slices):
    """[S*Bs, C, H, W] -> [S, C, H, W, Bs]: one batch-innermost block per batch slice (the input of a rank's work units), as ONE
    batched transpose launch."""
    require_device(x)
    x = x.contiguous()
    Bs = x.shape[0] // slices
    plane = x.numel() // x.shape[0]
    out = torch.empty((slices,) + tuple(x.shape[1:]) + (Bs,), dtype=torch.float32, device=x.device)
    if not _transpose_batched(x, out, Bs, plane, slices, 1, Bs * plane, 0, plane, plane * Bs, 0, Bs):
        raise _lib.BBBHipError("to_batch_innermost_slices: too many slices")
    return out


def mc_tail(logits, mean_over=0):
    """logits [E, B, C] -> [B, C]: log-sum-exp over draws of the per-draw log_softmax, minus log(mean_over)
    when mean_over > 0 (== utils.logmeanexp of the stacked log_softmax when mean_over == E)."""
    require_device(logits)
    logits = logits.contiguous()
    E, B, C = logits.shape
    out = torch.empty((B, C), dtype=torch.float32, device=logits.device)
    with on_device(logits.device):
        check(_lib.lib().bbb_mc_tail(logits.data_ptr(), E, B, C, int(mean_over), out.data_ptr(), cur_stream(logits.device)),
              "bbb_mc_tail")
    return out


# ------------------------------------------------------------------------------------------------
# autograd wiring
# ------------------------------------------------------------------------------------------------
class _SampleWeights(torch.autograd.Function):
    """(mu_0, rho_0, mu_1, rho_1, ...) -> (kl, w_0, w_1, ...), one fused launch; w_i: [draws, *shape]."""

    @staticmethod
    def forward(ctx, cfg, *params):
        mus, rhos = list(params[0::2]), list(params[1::2])
        ws, _, kl = reparam_kl_forward(mus, rhos, cfg["prior_mu"], cfg["prior_sigma"], cfg["stream_ids"], cfg["seed"],
                                       cfg["call0"], cfg["draws"], sample=True, eps=cfg.get("eps"),
                                       textbook_kl=cfg.get("textbook_kl", False), priors=cfg.get("priors"))
        ctx.cfg = cfg
        ctx.save_for_backward(*params)
        return (kl, *ws)

    @staticmethod
    def backward(ctx, gkl, *gws):
        params = ctx.saved_tensors
        cfg = ctx.cfg
        mus, rhos = list(params[0::2]), list(params[1::2])
        gmu, grho = reparam_kl_backward(mus, rhos, list(gws), gkl, cfg["prior_mu"], cfg["prior_sigma"], cfg["stream_ids"],
                                        cfg["seed"], cfg["call0"], cfg["draws"], eps=cfg.get("eps"),
                                        textbook_kl=cfg.get("textbook_kl", False), priors=cfg.get("priors"))
        out = [None]
        for a, b in zip(gmu, grho):
            out += [a, b]
        return tuple(out)


class _KLOnly(torch.autograd.Function):
    """KL (and optionally sigma / sigma^2 as a differentiable output) without sampling."""

    @staticmethod
    def forward(ctx, cfg, *params):
        mus, rhos = list(params[0::2]), list(params[1::2])
        _, sig, kl = reparam_kl_forward(mus, rhos, cfg["prior_mu"], cfg["prior_sigma"], cfg["stream_ids"], 0, 0, 1,
                                        sample=False, want_sigma=cfg.get("want_sigma", False),
                                        sigma_squared=cfg.get("sigma_squared", False),
                                        textbook_kl=cfg.get("textbook_kl", False), priors=cfg.get("priors"))
        ctx.cfg = cfg
        ctx.save_for_backward(*params)
        ctx.n_sig = 0 if sig is None else len(sig)
        out = (kl,) if sig is None else (kl, *sig)
        if cfg.get("mu_through", False):
            # the means again, as outputs of THIS node: what consumes them (the LRT forward node) hands its gradients back here,
            # where the backward kernel adds them to d KL / d mu -- instead of one accumulation launch per tensor in the engine
            out = out + tuple(m.view_as(m) for m in mus)
        return out

    @staticmethod
    def backward(ctx, gkl, *gout):
        params = ctx.saved_tensors
        cfg = ctx.cfg
        mus, rhos = list(params[0::2]), list(params[1::2])
        gsig, gthru = gout[:ctx.n_sig], gout[ctx.n_sig:]
        # d sigma / d rho = sigmoid(rho), d sigma^2 / d rho = 2 sigma sigmoid(rho): folded into the backward kernel (the LRT
        # training step spent ~70 ATen launches per step on these twelve small tensors)
        gs = None
        if gsig and any(g is not None for g in gsig):
            gs = [gsig[i] if i < len(gsig) else None for i in range(len(mus))]
        gws = [None] * len(mus)
        if gthru and any(g is not None for g in gthru):
            gws = [gthru[i] if i < len(gthru) else None for i in range(len(mus))]
        gmu, grho = reparam_kl_backward(mus, rhos, gws, gkl, cfg["prior_mu"], cfg["prior_sigma"],
                                        cfg["stream_ids"], 0, 0, 1, textbook_kl=cfg.get("textbook_kl", False), gsigmas=gs,
                                        sigma_squared=cfg.get("sigma_squared", False), gws_mean_only=True, priors=cfg.get("priors"))
        out = [None]
        for a, b in zip(gmu, grho):
            out += [a, b]
        return tuple(out)


def conv2d_splitk(x, w, bias, stride=1, padding=0, dilation=1):
    """conv2d_forward for the training path, where launches are small (one draw, a few hundred images): when the GEMM
    would occupy fewer than ~512 workgroups, the input channels are split into S chunks that run as extra "draws" of one
    launch and are summed afterwards in a fixed order (deterministic).  Same result up to fp32 summation order -- which is
    why the inference paths, whose loop / batched forms must agree bit for bit, never come through here."""
    Ex, B, Cin, H, W = x.shape
    Ew, Cout, _, kh, kw = w.shape
    E = max(Ex, Ew)
    ho, wo = out_map(H, W, (kh, kw), stride, padding, dilation)
    tiles = E * -(-B * ho * wo // 64) * -(-Cout // 64)
    S = 1
    while tiles * S < 512 and Cin % (2 * S) == 0 and (Cin // (2 * S)) * kh * kw >= 64:
        S *= 2
    if S == 1:
        return conv2d_forward(x, w, bias, stride, padding, dilation)
    c = Cin // S
    xs = x.reshape(Ex, B, S, c, H, W).permute(0, 2, 1, 3, 4, 5)                      # [Ex, S, B, c, H, W]
    ws = w.reshape(Ew, Cout, S, c, kh, kw).permute(0, 2, 1, 3, 4, 5)                 # [Ew, S, Cout, c, kh, kw]
    xs = xs.expand(E, S, B, c, H, W).reshape(E * S, B, c, H, W)
    ws = ws.expand(E, S, Cout, c, kh, kw).reshape(E * S, Cout, c, kh, kw)
    y = conv2d_forward(xs, ws, None, stride, padding, dilation)                      # [E*S, B, Cout, ho, wo]
    y = y.reshape(E, S, B, Cout, ho, wo).sum(1)
    if bias is not None:
        y = y + bias.reshape(bias.shape[0], 1, Cout, 1, 1)
    return y


def _small_launch(x, w, stride, padding, dilation):
    """True when a conv of x [E,B,Cin,H,W] with w [*,Cout,Cin,kh,kw] would occupy fewer than 512 64x64 output tiles and its
    channels can be split (the conv2d_splitk criterion)."""
    E, B, Cin, H, W = x.shape
    Cout, kh, kw = w.shape[1], w.shape[3], w.shape[4]
    ho, wo = out_map(H, W, (kh, kw), stride, padding, dilation)
    tiles = E * -(-B * ho * wo // 64) * -(-Cout // 64)
    return tiles < 512 and Cin % 2 == 0 and (Cin // 2) * kh * kw >= 64


def lrt_sample_nchw(act_mu, act_var, seed, call0, stream_id):
    """y = act_mu + sqrt(act_var) * eps for [E, ...] moments; eps = the LRT kernels' noise stream (draw e = call0 + e)."""
    require_device(act_mu, act_var)
    act_mu, act_var = act_mu.contiguous(), act_var.contiguous()
    E = act_mu.shape[0]
    n = act_mu.numel() // E
    y = torch.empty_like(act_mu)
    with on_device(act_mu.device):
        check(_lib.lib().bbb_lrt_sample_nchw(act_mu.data_ptr(), act_var.data_ptr(), y.data_ptr(), n, E, seed, call0 & 0xFFFFFFFF,
                                             stream_id, rng.call_dev_ptr(act_mu.device), cur_stream(act_mu.device)),
              "bbb_lrt_sample_nchw")
    return y


def conv2d_input_grad(gy, w, x_shape, stride, padding, dilation):
    """d loss / d x of y = conv2d(x, w) on the same fp32-MFMA kernel: a stride-1 convolution of gy -- zero-upsampled by the
    layer's stride -- with the spatially flipped, channel-transposed weights, the layer's dilation and padding
    d*(k-1) - p; rows / columns of x that no output touched get zero.  gy [E,B,Cout,Ho,Wo], w [E|1,Cout,Cin,kh,kw].
    (Stride s multiplies s*s - 1 inserted zeros: fine for the rare strided layer that is not a model's first layer -- on the
    batch-innermost path a first layer's input gradient is first_layer_input_grad, which multiplies no inserted zero.)"""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    kh, kw = w.shape[3], w.shape[4]
    H, W = x_shape[-2], x_shape[-1]
    E, B, Cout, Ho, Wo = gy.shape
    # upsampled extent, extended so that the stride-1 transposed convolution yields exactly H x W: input rows past
    # (Ho-1)*s + d*(k-1) - p still receive gradient from the last outputs only if they exist, i.e. zeros are appended
    Uh, Uw = H + 2 * ph - dh * (kh - 1), W + 2 * pw - dw * (kw - 1)
    if (sh, sw) != (1, 1) or (Uh, Uw) != (Ho, Wo):
        up = gy.new_zeros((E, B, Cout, Uh, Uw))
        up[:, :, :, :(Ho - 1) * sh + 1:sh, :(Wo - 1) * sw + 1:sw] = gy
        gy = up
    qh, qw = dh * (kh - 1) - ph, dw * (kw - 1) - pw                      # padding of the transposed convolution
    w_t = w.flip(3, 4).transpose(1, 2).contiguous()                     # [E|1, Cin, Cout, kh, kw]
    gx = conv2d_splitk(gy, w_t, None, 1, (max(qh, 0), max(qw, 0)), (dh, dw))
    if qh < 0 or qw < 0:                                                 # padding larger than the kernel reach: crop
        gx = gx[:, :, :, max(-qh, 0):gx.shape[3] - max(-qh, 0), max(-qw, 0):gx.shape[4] - max(-qw, 0)]
    if gx.shape[3] != H or gx.shape[4] != W:
        raise _lib.BBBHipError("conv2d_input_grad: geometry mismatch")
    return gx.contiguous()


def conv2d_weight_grad(gy, x, w_shape, stride, padding, dilation):
    """d loss / d w on the same kernel: with batch and channel axes swapped, wgrad is itself a convolution --
    input x^T [Cin as batch, B as channels, H, W], "weights" gy^T [Cout, B, Ho, Wo], stride = the layer's dilation,
    dilation = the layer's stride -> [Cin, Cout, kh(+), kw(+)], cropped and transposed back.  One GEMM per draw, batched
    over draws; when the weights are shared by all draws (LRT) the draw axis is folded into the batch."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    Ew, Cout, Cin, kh, kw = w_shape
    E = gy.shape[0]
    if x.shape[0] == 1 and E > 1:
        x = x.expand(E, *x.shape[1:])
    if Ew == 1 and E > 1:                                                # shared weights: sum over draws = bigger batch
        x = x.reshape(1, E * x.shape[1], *x.shape[2:])
        gy = gy.reshape(1, E * gy.shape[1], *gy.shape[2:])
    # split-K: the reduction runs over batch x output pixels while the result is only Cin*kh*kw x Cout, so a layer
    # with a large feature map would occupy a handful of workgroups.  Batch chunks become extra "draws", summed after.
    E1, Bt = x.shape[0], x.shape[1]
    tiles = E1 * -(-Cin * kh * kw // 64) * -(-Cout // 64)
    split = 1
    while Bt % (2 * split) == 0 and Bt // (2 * split) >= 4 and tiles * 2 * split <= 1024:
        split *= 2
    if split > 1:
        x = x.reshape(E1 * split, Bt // split, *x.shape[2:])
        gy = gy.reshape(E1 * split, Bt // split, *gy.shape[2:])
    x_t = x.transpose(1, 2).contiguous()                                 # [E, Cin, B, H, W]
    gy_t = gy.transpose(1, 2).contiguous()                               # [E, Cout, B, Ho, Wo]
    g = conv2d_forward(x_t, gy_t, None, (dh, dw), (ph, pw), (sh, sw))    # [E, Cin, Cout, kh', kw'], kh' >= kh
    g = g[:, :, :, :kh, :kw]
    if split > 1:
        g = g.reshape(E1, split, *g.shape[1:]).sum(1)
    return g.transpose(1, 2).contiguous()


class _Conv2d(torch.autograd.Function):
    """y = conv2d(x, w, bias) batched over draws.  Backward runs on the same HIP GEMM (dgrad as a flipped-weight conv of the
    stride-upsampled gradient, wgrad as the axis-swapped conv)."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, padding, dilation):
        y = conv2d_splitk(x, w, bias, stride, padding, dilation)
        ctx.save_for_backward(x, w)
        ctx.geom = (_pair(stride), _pair(padding), _pair(dilation), bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, padding, dilation, has_bias = ctx.geom
        gy = gy.contiguous()
        E = gy.shape[0]
        gx = gw = gb = None
        if has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum(dim=(1, 3, 4))
            if w.shape[0] == 1 and E > 1:
                gb = gb.sum(0, keepdim=True)
        if ctx.needs_input_grad[1]:
            gw = conv2d_weight_grad(gy, x, tuple(w.shape), stride, padding, dilation)
        if ctx.needs_input_grad[0]:
            gx = conv2d_input_grad(gy, w, (E,) + tuple(x.shape[1:]), stride, padding, dilation)
            if x.shape[0] == 1 and E > 1:
                gx = gx.sum(0, keepdim=True)
        return gx, gw, gb, None, None, None


class _LrtConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_mu, w_var, b_mu, b_var, cfg):
        geom = (cfg["stride"], cfg["padding"], cfg["dilation"])
        if _small_launch(x, w_mu.unsqueeze(0), *geom):
            # training-sized launch: the fused kernel would run a few dozen workgroups with long k loops; compute the two
            # moments with split-K launches and sample separately (same noise stream, same result up to summation order)
            am = conv2d_splitk(x, w_mu.unsqueeze(0), None if b_mu is None else b_mu.unsqueeze(0), *geom)
            av = conv2d_splitk(x * x, w_var.unsqueeze(0), None if b_var is None else b_var.unsqueeze(0), *geom) + 1e-16
            if not cfg["sample"]:
                y = am
            elif cfg.get("eps") is not None:
                y = am + av.sqrt() * cfg["eps"].reshape(am.shape)
            else:
                y = lrt_sample_nchw(am, av, cfg["seed"], cfg["call0"], cfg["stream_id"])
        else:
            y, am, av = lrt_conv2d_forward(x, w_mu, w_var, b_mu, b_var, cfg["seed"], cfg["call0"], cfg["stream_id"], *geom,
                                           sample=cfg["sample"], eps=cfg.get("eps"), want_moments=True)
        ctx.cfg = cfg
        ctx.save_for_backward(x, w_mu, w_var, y, am, av)
        ctx.has_bias = b_mu is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w_mu, w_var, y, am, av = ctx.saved_tensors
        cfg = ctx.cfg
        geom = (cfg["stride"], cfg["padding"], cfg["dilation"])
        gy = gy.contiguous()
        # out = am + sqrt(av) * eps  ->  d/d am = g ;  d/d av = g * eps / (2 sqrt(av)) = g * (y - am) / (2 av)
        gv = gy * (y - am) / (2.0 * av) if cfg["sample"] else torch.zeros_like(gy)
        x2 = x * x
        wm5, wv5 = w_mu.unsqueeze(0), w_var.unsqueeze(0)
        gwm = conv2d_weight_grad(gy, x, tuple(wm5.shape), *geom)[0]
        gwv = conv2d_weight_grad(gv, x2, tuple(wv5.shape), *geom)[0]
        gx = None
        if ctx.needs_input_grad[0]:
            g1 = conv2d_input_grad(gy, wm5, tuple(x.shape), *geom)
            g2 = conv2d_input_grad(gv, wv5, tuple(x.shape), *geom)
            gx = g1 + g2 * 2.0 * x
        gbm = gy.sum(dim=(0, 1, 3, 4)) if ctx.has_bias else None
        gbv = gv.sum(dim=(0, 1, 3, 4)) if ctx.has_bias else None
        return gx, gwm, gwv, gbm, gbv, None


def _no_grad_needed(tensors):
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


def sample_weights(mus, rhos, prior_mu, prior_sigma, stream_ids, seed, call0, draws=1, eps=None, textbook_kl=False, priors=None):
    if _no_grad_needed(list(mus) + list(rhos)):
        # inference: the launch itself -- autograd.Function.apply on 24 tensors costs ~80 us of host time per call
        ws, _, kl = reparam_kl_forward([m.detach() for m in mus], [r.detach() for r in rhos], prior_mu, prior_sigma, list(stream_ids), seed,
                                       call0, draws, sample=True, eps=eps, textbook_kl=textbook_kl, priors=priors)
        return kl, ws
    cfg = dict(prior_mu=prior_mu, prior_sigma=prior_sigma, stream_ids=list(stream_ids), seed=seed, call0=call0,
               draws=draws, eps=eps, textbook_kl=textbook_kl, priors=priors)
    flat = []
    for m, r in zip(mus, rhos):
        flat += [m, r]
    out = _SampleWeights.apply(cfg, *flat)
    return out[0], list(out[1:])


def kl_only(mus, rhos, prior_mu, prior_sigma, want_sigma=False, sigma_squared=False, textbook_kl=False, mu_through=False, priors=None):
    """-> (kl, [sigma ...]) -- with mu_through (and want_sigma) -> (kl, [sigma ...], [mu ...]): the means as outputs of the same
    autograd node, so that gradients w.r.t. them are added to d KL / d mu inside its one backward launch."""
    if _no_grad_needed(list(mus) + list(rhos)):
        _, sig, kl = reparam_kl_forward([m.detach() for m in mus], [r.detach() for r in rhos], prior_mu, prior_sigma, [0] * len(mus), 0, 0, 1,
                                        sample=False, want_sigma=want_sigma, sigma_squared=sigma_squared, textbook_kl=textbook_kl,
                                        priors=priors)
        sig = list(sig) if sig is not None else []
        return (kl, sig, list(mus)) if mu_through else (kl, sig)
    cfg = dict(prior_mu=prior_mu, prior_sigma=prior_sigma, stream_ids=[0] * len(mus), want_sigma=want_sigma,
               sigma_squared=sigma_squared, textbook_kl=textbook_kl, mu_through=mu_through, priors=priors)
    flat = []
    for m, r in zip(mus, rhos):
        flat += [m, r]
    out = _KLOnly.apply(cfg, *flat)
    if mu_through:
        n_sig = len(out) - 1 - len(mus)
        return out[0], list(out[1:1 + n_sig]), list(out[1 + n_sig:])
    return out[0], list(out[1:])


def conv2d(x, w, bias, stride=1, padding=0, dilation=1):
    """Differentiable conv2d batched over draws.  Without autograd (inference through the drop-in layers) this is the
    plain kernel launch, whose results the batched ensemble path reproduces bit for bit; with autograd the split-K
    variant may be used (training launches are small)."""
    if not (torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (bias is not None and bias.requires_grad))):
        return conv2d_forward(x, w, bias, stride, padding, dilation)
    return _Conv2d.apply(x, w, bias, stride, padding, dilation)


def lrt_conv2d(x, w_mu, w_var, b_mu, b_var, seed, call0, stream_id, stride=1, padding=0, dilation=1, sample=True, eps=None):
    cfg = dict(seed=seed, call0=call0, stream_id=stream_id, stride=stride, padding=padding, dilation=dilation,
               sample=sample, eps=eps)
    needs_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w_mu, w_var, b_mu, b_var))
    if not needs_grad:          # inference through the drop-in layers: the fused kernel, bitwise what the ensemble path runs
        return lrt_conv2d_forward(x, w_mu, w_var, b_mu, b_var, seed, call0, stream_id, stride, padding, dilation,
                                  sample=sample, eps=eps)[0]
    return _LrtConv2d.apply(x, w_mu, w_var, b_mu, b_var, cfg)


# ------------------------------------------------------------------------------------------------
# batch-innermost backward helpers (training on the fast path: called from the nodes' _backward in bbb_hip/fast_train.py, on the
# stream fast_train._Schedule puts them on)
# ------------------------------------------------------------------------------------------------
def padded_plane_pitch(K):
    """Row pitch for a [planes, K] matrix that a GEMM reads row-wise: K itself unless rows of K floats are a multiple of 4 KiB
    apart (then every row of a 64-row tile would start in the same memory channel: measured 10x slower), else K + 32."""
    return K + 32 if K % 1024 == 0 else K


def pool_act_backward_chwn(g_out, y, k, s, act, pad_planes=False, avg=None):
    """Backward of [fused activation -> MaxPool2d(k, s)] (k = 0: activation only) on [..., H, W, B] planes: gradient w.r.t.
    the layer's pre-activation from the gradient w.r.t. the (pooled) output and the ACTIVATED output y (bbb_pool_act_bwd_chwn).
    pad_planes: return a view of y's shape into a [planes, padded_plane_pitch(H*W*B)] buffer (see there).
    avg = (kernel, stride, padding, count_include_pad): the pool is that average pool instead (avgpool_act_backward_chwn)."""
    require_device(g_out, y)
    g_out, y = g_out.contiguous(), y.contiguous()
    _, H, W, B, planes = _planes_of(y.shape)
    buf, g_pre, pitch = _grad_buffers(y, planes, None, pad_planes)
    if avg is not None:
        _pooled_grad_shape(g_out, planes, H, W, B, avg)
    with on_device(y.device):
        if avg is not None:
            check(_lib.lib().bbb_avgpool_act_bwd_chwn(ctypes.byref(_pool_desc(H, W, B, *avg)), g_out.data_ptr(), y.data_ptr(), buf.data_ptr(),
                                                      planes, ACT_CODE[act], pitch, cur_stream(y.device)), "bbb_avgpool_act_bwd_chwn")
        else:
            check(_lib.lib().bbb_pool_act_bwd_chwn(g_out.data_ptr(), y.data_ptr(), buf.data_ptr(), planes, H, W, B, int(k), int(s),
                                                   ACT_CODE[act], pitch, cur_stream(y.device)), "bbb_pool_act_bwd_chwn")
    return g_pre


def avgpool_act_backward_chwn(g_out, y, kernel, stride, padding, count_include_pad, act, pad_planes=False):
    """Backward of [fused activation -> AvgPool2d(kernel, stride, padding, count_include_pad=)] on [..., H, W, B] planes
    (bbb_avgpool_act_bwd_chwn): pool_act_backward_chwn with every tap of a window receiving that window's gradient over its divisor."""
    return pool_act_backward_chwn(g_out, y, 0, 1, act, pad_planes=pad_planes, avg=(kernel, stride, padding, count_include_pad))


def plane_sums(g, over_draws=False):
    """Bias gradient from the gradient w.r.t. a layer's pre-activation g [E, C, H, W, B] (possibly a padded-pitch view as
    pool_act_backward_chwn returns it): -> [E, C] (sum over pixels and images), or [C] with over_draws (bbb_plane_sum)."""
    require_device(g)
    E, C, H, W, B = g.shape
    cols = H * W * B
    if g.stride(4) != 1 or g.stride(3) != B or g.stride(2) != W * B or g.stride(0) != C * g.stride(1):
        g = g.contiguous()
    pitch = g.stride(1)
    out = torch.empty((C,) if over_draws else (E, C), dtype=torch.float32, device=g.device)
    with on_device(g.device):
        if over_draws:
            check(_lib.lib().bbb_plane_sum(g.data_ptr(), out.data_ptr(), E, C, cols, pitch, C * pitch, cur_stream(g.device)), "bbb_plane_sum")
        else:
            check(_lib.lib().bbb_plane_sum(g.data_ptr(), out.data_ptr(), 1, E * C, cols, pitch, 0, cur_stream(g.device)), "bbb_plane_sum")
    return out


def sum_over_draws(x, keepdim=False, out=None):
    """x [E, ...] -> the sum over the leading (draw) axis, added in draw order (bbb_sum_leading); trailing size % 4 == 0.
    out: a contiguous fp32 tensor of one draw's element count to write into (returned in the result's shape)."""
    require_device(x)
    x = x.contiguous()
    E = x.shape[0]
    if E == 1 and out is None:
        return x if keepdim else x[0]
    n = x.numel() // E
    shape = ((1,) if keepdim else ()) + tuple(x.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif not out.is_contiguous() or out.numel() != n or out.dtype != torch.float32:
        raise _lib.BBBHipError("sum_over_draws: out must be a contiguous fp32 tensor of one draw's size")
    with on_device(x.device):
        check(_lib.lib().bbb_sum_leading(x.data_ptr(), out.data_ptr(), E, n, cur_stream(x.device)), "bbb_sum_leading")
    return out.view(shape)


def square(x, out=None):
    """x * x (bbb_lrt_glue mode 0): the operand of the LRT variance contraction's weight gradient.  out: a contiguous tensor of
    x's element count to write into."""
    require_device(x)
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    elif not out.is_contiguous() or out.numel() != x.numel() or out.dtype != torch.float32:
        raise _lib.BBBHipError("square: out must be a contiguous fp32 tensor of x's size")
    with on_device(x.device):
        check(_lib.lib().bbb_lrt_glue(0, x.data_ptr(), 0, out.data_ptr(), x.numel(), 0, 0, cur_stream(x.device)), "bbb_lrt_glue")
    return out


def lrt_input_grad_combine(g1, x, g2):
    """g1 + 2 * x * g2 with x [1|E, ...] broadcast over the draws of g1 / g2 [E, ...] (bbb_lrt_glue mode 1)."""
    require_device(g1, x, g2)
    g1, x, g2 = g1.contiguous(), x.contiguous(), g2.contiguous()
    out = torch.empty_like(g1)
    with on_device(g1.device):
        check(_lib.lib().bbb_lrt_glue(g1.data_ptr(), x.data_ptr(), g2.data_ptr(), out.data_ptr(), g1.numel(), x.numel(), 1,
                                      cur_stream(g1.device)), "bbb_lrt_glue")
    return out


def lrt_pool_act_backward_chwn(g_out, y, act_mu, act_var, k, s, act, pad_planes=False, stacked=False, combine=None, avg=None):
    """pool_act_backward_chwn for a local-reparameterisation layer: -> (g_mu, g_var), the gradients w.r.t. act_mu and act_var
    (bbb_lrt_pool_act_bwd_chwn).  act_mu / act_var: y's shape, or one draw's worth ([1, C, H, W, B]) when every draw was sampled
    from the same pair of moments.  stacked (without pad_planes): the two land in ONE buffer [2, *y.shape], returned as such --
    the weight-side and input-side contractions of the pair then run as the draws of one launch.
    combine = (x_out, g_out2): the incoming gradient is g_out + 2 * x_out * g_out2 (lrt_input_grad_combine of the layer above,
    formed on the fly: g_out / g_out2 = its two input gradients, x_out = this layer's output, [E|1, ...] of g_out's trailing shape).
    avg = (kernel, stride, padding, count_include_pad): the pool is that average pool instead (lrt_avgpool_act_backward_chwn)."""
    require_device(g_out, y, act_mu, act_var)
    g_out, y, act_mu, act_var = g_out.contiguous(), y.contiguous(), act_mu.contiguous(), act_var.contiguous()
    g2p, xcp, x_planes = 0, 0, 0
    if combine is not None:
        xc, g2 = combine[0].contiguous(), combine[1].contiguous()
        require_device(xc, g2)
        if g2.numel() != g_out.numel() or g_out.numel() % xc.numel() != 0:
            raise _lib.BBBHipError("lrt_pool_act_backward_chwn: combine = (x_out, g_out2) of g_out's shape (x_out may hold one draw)")
        g2p, xcp = g2.data_ptr(), xc.data_ptr()
    _, H, W, B, planes = _planes_of(y.shape)
    mom_planes = act_mu.numel() // (H * W * B)
    if act_mu.shape != act_var.shape or act_mu.numel() != mom_planes * H * W * B or planes % max(mom_planes, 1) != 0:
        raise _lib.BBBHipError("lrt_pool_act_backward_chwn: act_mu / act_var must hold y's planes, or one draw's worth of them")
    # the two outputs one allocation apart in every form: a first layer's input gradient reads them as the two draws of one launch
    bufs, outs, pitch = _grad_buffers(y, planes, None, pad_planes, pair=True)
    x_planes = (planes * xc.numel() // g_out.numel()) if combine is not None else 0
    if avg is not None:
        _pooled_grad_shape(g_out, planes, H, W, B, avg)
    with on_device(y.device):
        if avg is not None:
            check(_lib.lib().bbb_lrt_avgpool_act_bwd_chwn(ctypes.byref(_pool_desc(H, W, B, *avg)), g_out.data_ptr(), y.data_ptr(),
                                                          act_mu.data_ptr(), act_var.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                                                          planes, mom_planes, ACT_CODE[act], pitch, g2p, xcp,
                                                          x_planes, cur_stream(y.device)),
                  "bbb_lrt_avgpool_act_bwd_chwn")
        else:
            check(_lib.lib().bbb_lrt_pool_act_bwd_chwn(g_out.data_ptr(), y.data_ptr(), act_mu.data_ptr(), act_var.data_ptr(),
                                                       bufs[0].data_ptr(), bufs[1].data_ptr(), planes, mom_planes, H, W, B, int(k), int(s),
                                                       ACT_CODE[act], pitch, g2p, xcp, x_planes,
                                                       cur_stream(y.device)),
                  "bbb_lrt_pool_act_bwd_chwn")
    if stacked and pitch == 0:
        return outs
    return outs[0], outs[1]


def lrt_avgpool_act_backward_chwn(g_out, y, act_mu, act_var, kernel, stride, padding, count_include_pad, act, pad_planes=False,
                                  stacked=False, combine=None):
    """lrt_pool_act_backward_chwn behind an AvgPool2d(kernel, stride, padding, count_include_pad=) (bbb_lrt_avgpool_act_bwd_chwn):
    the same arguments and results, the average pool's routing."""
    return lrt_pool_act_backward_chwn(g_out, y, act_mu, act_var, 0, 1, act, pad_planes=pad_planes, stacked=stacked, combine=combine,
                                      avg=(kernel, stride, padding, count_include_pad))


def flip_transpose_w(w):
    """[E, Cout, Cin, kh, kw] -> [E, Cin, Cout, kh, kw] with the taps spatially flipped: the weight operand of the input gradient."""
    w = w.contiguous()
    E, Cout, Cin, kh, kw = w.shape
    w_t = torch.empty((E, Cin, Cout, kh, kw), dtype=torch.float32, device=w.device)
    with on_device(w.device):
        check(_lib.lib().bbb_flip_transpose_w(w.data_ptr(), w_t.data_ptr(), E, Cout, Cin, kh * kw, cur_stream(w.device)),
              "bbb_flip_transpose_w")
    return w_t


def flip_transpose_w_pair(w0, w1):
    """flip_transpose_w of two weight sets of one shape as ONE operand: [E, Cout, Cin, kh, kw] x 2 -> [2E, Cin, Cout, kh, kw], w0's
    draws first (bbb_flip_transpose_w_pair: an LRT layer's mean and variance weights for both input gradients in one launch)."""
    require_device(w0, w1)
    w0, w1 = w0.contiguous(), w1.contiguous()
    if w0.shape != w1.shape or w0.dim() != 5:
        raise _lib.BBBHipError("flip_transpose_w_pair: two [E, Cout, Cin, kh, kw] tensors of one shape")
    E, Cout, Cin, kh, kw = w0.shape
    w_t = torch.empty((2 * E, Cin, Cout, kh, kw), dtype=torch.float32, device=w0.device)
    with on_device(w0.device):
        check(_lib.lib().bbb_flip_transpose_w_pair(w0.data_ptr(), w1.data_ptr(), w_t.data_ptr(), E, Cout, Cin, kh * kw,
                                                   cur_stream(w0.device)), "bbb_flip_transpose_w_pair")
    return w_t


def flip_transpose_w_multi(sets):
    """flip_transpose_w / flip_transpose_w_pair for several layers in ONE launch (bbb_flip_transpose_w_multi): `sets` = a list of
    w [E, Cout, Cin, kh, kw] or (w0, w1) pairs of one shape -> the list of [E | 2E, Cin, Cout, kh, kw] results."""
    if not sets:
        return []
    if len(sets) > 16:
        return flip_transpose_w_multi(sets[:16]) + flip_transpose_w_multi(sets[16:])
    segs = (_lib.FlipSeg * len(sets))()
    outs, hold = [], []
    for i, s_ in enumerate(sets):
        w0, w1 = s_ if isinstance(s_, (tuple, list)) else (s_, None)
        require_device(w0) if w1 is None else require_device(w0, w1)
        w0 = w0.contiguous()
        E, Cout, Cin, kh, kw = w0.shape
        if w1 is not None:
            w1 = w1.contiguous()
            if w1.shape != w0.shape:
                raise _lib.BBBHipError("flip_transpose_w_multi: the two sources of a pair must have one shape")
        n = E if w1 is None else 2 * E
        o = torch.empty((n, Cin, Cout, kh, kw), dtype=torch.float32, device=w0.device)
        segs[i].w0, segs[i].w1, segs[i].out = w0.data_ptr(), (0 if w1 is None else w1.data_ptr()), o.data_ptr()
        segs[i].draws, segs[i].cout, segs[i].cin, segs[i].khkw = n, Cout, Cin, kh * kw
        outs.append(o)
        hold += [w0, w1]
    dev = outs[0].device
    with on_device(dev):
        check(_lib.lib().bbb_flip_transpose_w_multi(segs, len(sets), cur_stream(dev)), "bbb_flip_transpose_w_multi")
    return outs


def dgrad_tap_plan(ih, ho, k, s, p, d):
    """Host restatement of the transposed launch's per-axis tap enumeration (csrc/pconv_args.h, tr_axis): the flipped-weight taps
    r' that take part in input row `ih` of a layer with `ho` output rows, kernel k, stride s, padding p, dilation d, and the output
    row each reads -> [(r', oh)].  t = ih - (d (k - 1) - p) + r' d must be >= 0, divisible by s and t / s < ho; those taps are an
    arithmetic progression with step s / gcd(s, d) whose first member is among the first `step` taps."""
    base, step = ih - (d * (k - 1) - p), s // math.gcd(s, d)
    first = next((r for r in range(min(step, k)) if (base + r * d) % s == 0), None)
    if first is None:
        return []
    t0, sd = base + first * d, step * d
    r0 = first + ((-t0 + sd - 1) // sd if t0 < 0 else 0) * step
    lim = (ho - 1) * s - base
    if lim < 0:
        return []
    r1 = min(lim // d, k - 1)
    return [(r, (base + r * d) // s) for r in range(r0, r1 + 1, step)]


def conv2d_chwn_input_grad(g_pre, w, x_hw, padding, dilation, w_flipped=None, stride=1):
    """d loss / d x of y = conv(x, w) in the batch-innermost layout.  g_pre [E, Cout, Ho, Wo, B], w [E|1, Cout, Cin, kh, kw] ->
    [E, Cin, H, W, B] for x_hw = (H, W).  w_flipped: flip_transpose_w(w) computed ahead (off the gradient chain).
    stride 1 (the default): the forward kernel itself -- the convolution of g_pre with the spatially flipped, channel-transposed
    weights, padding d*(k-1) - p.
    Any other stride: the transposed form of that launch (bbb_conv2d_chwn_dgrad, csrc/pconv_dgrad.hip), which visits exactly the
    forward's in-bounds (pixel, tap) pairs -- no zero-upsampled gradient, no product with an inserted zero; input pixels that no
    tap reaches come back as zeros.  Always the fp32 kernel and never a split contraction (LaunchConfig: gemm_mode, split_k)."""
    (ph, pw), (dh, dw), (sh, sw) = _pair(padding), _pair(dilation), _pair(stride)
    kh, kw = w.shape[3], w.shape[4]
    qh, qw = dh * (kh - 1) - ph, dw * (kw - 1) - pw
    if qh < 0 or qw < 0:
        raise _lib.BBBHipError("conv2d_chwn_input_grad: padding larger than the kernel reach")
    w_t = w_flipped if w_flipped is not None else flip_transpose_w(w)
    if (sh, sw) == (1, 1):
        gx = conv2d_chwn_forward(g_pre, w_t, None, 1, (qh, qw), (dh, dw))
        if gx.shape[2] != x_hw[0] or gx.shape[3] != x_hw[1]:
            raise _lib.BBBHipError("conv2d_chwn_input_grad: geometry mismatch (x_hw is not this stride-1 layer's input map)")
        return gx
    if sh < 1 or sw < 1:
        raise _lib.BBBHipError("conv2d_chwn_input_grad: strides are positive")
    require_device(g_pre, w_t)
    g_pre, w_t = g_pre.contiguous(), w_t.contiguous()
    if g_pre.dim() != 5 or w_t.dim() != 5:
        raise _lib.BBBHipError("g_pre [E|1, Cout, Ho, Wo, B] and flipped weights [E|1, Cin, Cout, kh, kw] expected")
    H, W = int(x_hw[0]), int(x_hw[1])
    Eg, Cout, Ho, Wo, B = g_pre.shape
    _same_channels(Cout, w_t.shape[2])
    d, _, _ = conv_desc(B, Cout, (Ho, Wo), w_t.shape[1], (kh, kw), 1, (qh, qw), (dh, dw))        # the stride-1 launch on the flipped weights
    E, _, _ = slab_rule(d, Eg, w_t.shape[0])
    gx = torch.empty((E, w_t.shape[1], H, W, B), dtype=torch.float32, device=g_pre.device)
    with on_device(g_pre.device):
        check(_lib.lib().bbb_conv2d_chwn_dgrad(ctypes.byref(d), g_pre.data_ptr(), w_t.data_ptr(), gx.data_ptr(), sh, sw, H, W,
                                               cur_stream(g_pre.device)), "bbb_conv2d_chwn_dgrad")
    return gx


def fp32_dgrad_plan(B, cin, cout, kh, kw, x_hw, stride, dilation, draws, padding=None):
    """(images per item 64 | 128, interleaved staging, items, workgroups) of the launch bbb_conv2d_chwn_dgrad makes for the input
    gradient of a strided layer with weights (cout, cin, kh, kw), input map x_hw = (H, W), `draws` draws of B images: the launch
    entry's own plan (bbb_conv2d_chwn_dgrad_plan, csrc/pconv_plan.h: dgrad_plan -- the forward's tile rule; host only).  padding:
    the layer's (default dilation * (k - 1), whose output map exists for every input map; the choice does not depend on it)."""
    (sh, sw), (dh, dw) = _pair(stride), _pair(dilation)
    H, W = int(x_hw[0]), int(x_hw[1])
    ph, pw = (dh * (kh - 1), dw * (kw - 1)) if padding is None else _pair(padding)
    g_hw = out_map(H, W, (kh, kw), (sh, sw), (ph, pw), (dh, dw))
    d, _, _ = conv_desc(B, cout, g_hw, cin, (kh, kw), 1, (dh * (kh - 1) - ph, dw * (kw - 1) - pw), (dh, dw), int(draws))
    bm, ilv, items, blocks = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(_lib.lib().bbb_conv2d_chwn_dgrad_plan(ctypes.byref(d), sh, sw, H, W, ctypes.byref(bm), ctypes.byref(ilv), ctypes.byref(items),
                                                ctypes.byref(blocks)), "bbb_conv2d_chwn_dgrad_plan")
    return bm.value, bool(ilv.value), items.value, blocks.value


def _transpose_batched(src, out, rows, cols, nb1, nb2, ib1, ib2, ir, ob1, ob2, oc):
    nb = nb1 * nb2
    if nb > 65535 or (rows + 31) // 32 > 65535:
        return False
    with on_device(src.device):
        check(_lib.lib().bbb_transpose_batched(src.data_ptr(), out.data_ptr(), rows, cols, nb1, nb2, ib1, ib2, ir, ob1, ob2, oc,
                                               cur_stream(src.device)), "bbb_transpose_batched")
    return True


def _transpose_sum_batched(src, out, rows, cols, nb, ib, ob, ir, oc, nsum=1, in_sum=0, square_off=0):
    """bbb_transpose_sum_batched: three batch dimensions `nb` with strides `ib` / `ob`, `nsum` slices `in_sum` apart summed in
    ascending order; square_off != 0: the squares land square_off elements behind the outputs.  False (nothing launched) when the
    batch does not fit one grid."""
    if nb[0] * nb[1] * nb[2] > 65535 or (rows + 31) // 32 > 65535:
        return False
    with on_device(src.device):
        check(_lib.lib().bbb_transpose_sum_batched(src.data_ptr(), out.data_ptr(), rows, cols, (ctypes.c_int32 * 3)(*nb),
                                                   (ctypes.c_int64 * 3)(*ib), (ctypes.c_int64 * 3)(*ob), ir, oc, nsum, in_sum,
                                                   int(square_off), cur_stream(src.device)), "bbb_transpose_sum_batched")
    return True


def chwn_to_bhwc(x, out=None):
    """[E, C, H, W, B] -> [E, B, H, W, C] (the batch becomes the contraction channels, C the innermost axis).  out: a contiguous
    [E, B, H, W, C] tensor to write into."""
    E, C, H, W, B = x.shape
    x = x.contiguous()
    if out is None:
        out = torch.empty((E, B, H, W, C), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (E, B, H, W, C) or not out.is_contiguous():
        raise _lib.BBBHipError("chwn_to_bhwc: out must be a contiguous [E, B, H, W, C] tensor")
    HW = H * W
    if not _transpose_batched(x, out, C, B, E, HW, C * HW * B, B, HW * B, B * HW * C, C, HW * C):
        out.copy_(x.permute(0, 4, 2, 3, 1))
    return out


def chwn_grad_as_weights(g, chunks=1):
    """[E, Cout, Ho, Wo, B] -> [E, Cout, B, Ho, Wo] (the output gradient in the layout of a weight operand); with `chunks` = S
    the batch splits into S slices that become extra draws: [E*S, Cout, B/S, Ho, Wo], slice s of draw e at index e*S + s."""
    E, Co, Ho, Wo, B = g.shape
    g = g.contiguous()
    P_ = Ho * Wo
    S = int(chunks)
    if S > 1:
        Bs = B // S
        out = torch.empty((E * S, Co, Bs, Ho, Wo), dtype=g.dtype, device=g.device)
        if _transpose_sum_batched(g, out, P_, Bs, (E, S, Co), (Co * P_ * B, Bs, P_ * B), (S * Co * Bs * P_, Co * Bs * P_, Bs * P_),
                                  B, P_):
            return out
        return (chwn_grad_as_weights(g).reshape(E, Co, S, Bs, Ho, Wo).permute(0, 2, 1, 3, 4, 5)
                .reshape(E * S, Co, Bs, Ho, Wo))
    out = torch.empty((E, Co, B, Ho, Wo), dtype=g.dtype, device=g.device)
    if not _transpose_batched(g, out, P_, B, E * Co, 1, P_ * B, 0, B, B * P_, 0, P_):
        out = g.permute(0, 1, 4, 2, 3).contiguous()
    return out


# conv2d_chwn_weight_grad may read a large launch's output gradient in place as a tap-major weight operand (no transposed copy, 250 MB
# per 512 x 10 step).  Measured slower, so off: 2.54 against 2.47 ms per step (profiles/experiments/ab_wgrad_inplace.py) -- with the
# images innermost in k, consecutive rows of the role-swapped input are a whole image apart instead of adjacent.
wgrad_in_place = [False]


def wgrad_batch_chunks(E, Cout, Cin, kh, kw, B):
    """The number S of batch chunks conv2d_chwn_weight_grad runs as extra draws: doubled while the role-swapped launch (E draws,
    Cin already a multiple of 4) would occupy fewer than 512 workgroups and every chunk keeps an even share of >= 8 images."""
    wgs = E * kh * kw * -(-Cout // 64) * -(-Cin // 64)
    S = 1
    while wgs * S < 512 and B % (2 * S) == 0 and B // (2 * S) >= 8:
        S *= 2
    return S


def shared_input_k_slices(M, Jp, K):
    """The number S of K slices conv2d_chwn_weight_grad_shared_input runs as the launch's draws (M = E * Cout rows, Jp im2col
    columns, K = Ho * Wo * B): slices sized for the launcher's 128-wide tiles (>= 768 of them; 64-wide: 2.50 -> 2.48 ms per
    512 x 10 step), each a multiple of 4 and >= 256 long."""
    wgs = -(-M // 64) * -(-Jp // 128)
    S = 1
    while wgs * S < 768 and K % (2 * S) == 0 and (K // (2 * S)) % 4 == 0 and K // (2 * S) >= 256:
        S *= 2
    return S


def conv2d_chwn_weight_grad(g_pre, x, w_shape, stride, padding, dilation, x_squares=False):
    """d loss / d w in the batch-innermost layout, again on the forward kernel with the roles swapped: the batch becomes the
    contraction channels, the layer's input channels the innermost ("image") axis, the output pixels the kernel taps:
        gw[e][n][tap][ci] = sum_{b, opix} g_pre'[e][n][b][opix] * x'[e][b][ipix(tap, opix)][ci]
    with x' = x as [E|1, B, H, W, Cin], g_pre' = g_pre as [E, Cout, B, Ho, Wo], stride <-> dilation swapped.  Padding taps
    are skipped as in the forward.  The innermost axis moves as 16-byte vectors: an input with Cin % 4 != 0 is padded with zero
    planes first.  x may be shared by all draws ([1, ...]).  A launch that would occupy fewer than 512 workgroups (one draw of a small model) splits the batch into
    S chunks that run as extra draws and are summed in a fixed order.  g_pre [E, Cout, Ho, Wo, B], x [E|1, Cin, H, W, B] ->
    [E, Cout, Cin, kh, kw].
    x_squares (the two weight gradients of a local-reparameterisation layer as one launch): g_pre holds 2E' draws -- the gradients
    w.r.t. the E' mean activations, then the E' variance activations -- and x [E', ...] pairs with the first half, its squares with
    the second; -> [2E', Cout, Cin, kh, kw]."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    Ew, Cout, Cin, kh, kw = w_shape
    if Cin % 4 != 0:
        # the innermost axis of the role-swapped launch moves as 16-byte vectors: pad the input channels with zero planes
        # (BayesianLeNet's 6-channel second conv) and drop their -- all-zero -- gradient columns
        Cp = (Cin + 3) & ~3
        xp = x.new_zeros((x.shape[0], Cp) + tuple(x.shape[2:]))
        xp[:, :Cin] = x
        return conv2d_chwn_weight_grad(g_pre, xp, (Ew, Cout, Cp, kh, kw), stride, padding, dilation,
                                       x_squares=x_squares)[:, :, :Cin].contiguous()
    E, B = g_pre.shape[0], g_pre.shape[4]
    if x_squares:
        Ex = x.shape[0]
        if E != 2 * Ex:
            raise _lib.BBBHipError("conv2d_chwn_weight_grad(x_squares): g_pre must hold two draws per draw of x")
        xr = torch.empty((2 * Ex, B, x.shape[2], x.shape[3], Cin), dtype=torch.float32, device=x.device)
        H_, W_ = x.shape[2], x.shape[3]
        HW_ = H_ * W_
        xc = x.contiguous()
        # the transposed x and, behind it, its squares (x^2 transposed = the transposed x, squared) in ONE pass
        if not _transpose_sum_batched(xc, xr, Cin, B, (Ex, HW_, 1), (Cin * HW_ * B, B, 0), (B * HW_ * Cin, Cin, 0), HW_ * B, HW_ * Cin,
                                      square_off=Ex * B * HW_ * Cin):
            chwn_to_bhwc(xc, out=xr[:Ex])
            square(xr[:Ex], out=xr[Ex:])
    else:
        xr = chwn_to_bhwc(x)                                            # [E|1, B, H, W, Cin]
    S = wgrad_batch_chunks(E, Cout, Cin, kh, kw, B)
    if S == 1 and wgrad_in_place[0] and current_config().gemm_mode != "bf16x3":
        # the output gradient [E, Cout, Ho, Wo, B] IS a tap-major weight operand (taps = output pixels, channels = images): read in
        # place, the contraction running (pixel, image) instead of (image, pixel) -- no transposed copy (250 MB per 512 x 10 step)
        y = conv2d_chwn_forward(xr, g_pre.contiguous(), None, (dh, dw), (ph, pw), (sh, sw), w_tap_major=True)
    else:
        gr = chwn_grad_as_weights(g_pre, S)                             # [E*S, Cout, B/S, Ho, Wo]
        if S > 1:
            if xr.shape[0] == 1 and E > 1:
                xr = xr.expand(E, *xr.shape[1:])
            xr = xr.reshape(xr.shape[0] * S, B // S, *xr.shape[2:])
        y = conv2d_chwn_forward(xr, gr, None, (dh, dw), (ph, pw), (sh, sw))  # [E*S, Cout, kh', kw', Cin], kh' >= kh
    if y.shape[2] == kh and y.shape[3] == kw:                           # sum_s [E, S, Cout, kh*kw, Cin] -> [E, Cout, Cin, kh*kw]
        gw = torch.empty((E, Cout, Cin, kh, kw), dtype=torch.float32, device=y.device)
        T = kh * kw
        if _transpose_sum_batched(y, gw, T, Cin, (E, Cout, 1), (S * Cout * T * Cin, T * Cin, 0), (Cout * Cin * T, Cin * T, 0), Cin, T,
                                  S, Cout * T * Cin):
            return gw
    if S > 1:
        y = y.reshape(E, S, *y.shape[1:]).sum(1)
    return y[:, :, :kh, :kw, :].permute(0, 1, 4, 2, 3).contiguous()


def im2col_pbj(x_nchw, w_shape, stride, padding, dilation):
    """The im2col of a shared first-layer input for conv2d_chwn_weight_grad_shared_input (bbb_im2col_pbj): x [B, Cin, H, W] ->
    [Ho * Wo, B, Jp] with j = (ci, r, q), Jp = Cin * kh * kw rounded up to 4 (zero columns).  It depends on the batch alone: a
    training step may build it off the gradient chain; its elementwise square is the im2col of x^2 (the LRT variance side)."""
    _, Cout, Cin, kh, kw = w_shape
    x_nchw = x_nchw.contiguous()
    B, x_cin, H, W = x_nchw.shape
    _same_channels(x_cin, Cin)
    dd, ho, wo = conv_desc(B, Cin, (H, W), Cout, (kh, kw), stride, padding, dilation)
    Jp = (Cin * kh * kw + 3) // 4 * 4
    xk = torch.empty((ho * wo, B, Jp), dtype=torch.float32, device=x_nchw.device)
    with on_device(x_nchw.device):
        check(_lib.lib().bbb_im2col_pbj(x_nchw.data_ptr(), xk.data_ptr(), ctypes.byref(dd), cur_stream(x_nchw.device)), "bbb_im2col_pbj")
    return xk


def conv2d_chwn_weight_grad_shared_input(g_pre, x_nchw, w_shape, stride, padding, dilation, xk=None):
    """Weight gradient of a layer whose INPUT is the same for every draw (a model's first layer; 3-channel images do not fit
    the role-swapped launch, whose innermost axis would be Cin).  The draws stack into the row dimension instead:
        GW[(e, n)][j] = sum_k G[(e, n)][k] * Xcol[k][j],   k = (output pixel, image), j = (ci, r, q)
    -- g_pre's own memory IS the [E*Cout, K] matrix G, Xcol is the im2col of the shared input (built once: F.unfold + one
    permute), and the product runs on the forward kernel as a 1x1 "convolution" with K as the contraction channels and j as
    the innermost axis, K split into S slices that run as the launch's draws (w_row_pitch lets a slice of G's rows be read in
    place) and are summed in a fixed order.  g_pre [E, Cout, Ho, Wo, B], x_nchw [B, Cin, H, W] -> [E, Cout, Cin, kh, kw].
    xk: im2col_pbj(x_nchw, ...) built ahead (x_nchw is then only checked for its batch size and may be None)."""
    E, Cout, Ho, Wo, B = g_pre.shape
    _, _, Cin, kh, kw = w_shape
    J, P_ = Cin * kh * kw, Ho * Wo
    Jp = (J + 3) // 4 * 4
    K = P_ * B
    if xk is None:
        xk = im2col_pbj(x_nchw, w_shape, stride, padding, dilation)
    if tuple(xk.shape) != (P_, B, Jp) or not xk.is_contiguous():
        raise _lib.BBBHipError("conv2d_chwn_weight_grad_shared_input: geometry mismatch")
    M = E * Cout
    S = shared_input_k_slices(M, Jp, K)
    Ks = K // S
    # the 1x1 "layer": Jp "images" of Ks channels, M filters; its S draws are the K slices, Ks columns apart inside G's rows
    d, _, _ = conv_desc(Jp, Ks, (1, 1), M, (1, 1), draws=S, w_stride=Ks, b_stride=0)
    # G's rows must not be a multiple of 4 KiB apart (128 KiB for 64 pixels x 512 images: the 64 rows of a weight tile would
    # all sit in the same memory channel).  pool_act_backward_chwn(pad_planes=True) already wrote g_pre at the padded pitch;
    # anything else is copied once.
    pitch = padded_plane_pitch(K)
    if g_pre.is_contiguous() and pitch == K:
        gp = g_pre
    elif g_pre.stride(1) == pitch and g_pre.stride(0) == Cout * pitch and g_pre[0, 0].is_contiguous():
        gp = g_pre                                                     # a view into the padded [M, pitch] buffer
    else:
        gp = torch.empty((M, pitch), dtype=torch.float32, device=g_pre.device)
        gp[:, :K] = g_pre.reshape(M, K)
    d.w_row_pitch = pitch
    y = torch.empty((S, M, Jp), dtype=torch.float32, device=g_pre.device)
    with on_device(g_pre.device):
        check(_lib.lib().bbb_conv2d_chwn_fwd(ctypes.byref(d), xk.data_ptr(), gp.data_ptr(), 0, y.data_ptr(),
                                             cur_stream(g_pre.device)), "bbb_conv2d_chwn_fwd")
    gw = y.sum(0) if S > 1 else y[0]
    return gw[:, :J].reshape(E, Cout, Cin, kh, kw)


def _gemm_rows(gs):
    """gs: tensors [E, C, Ho, Wo, B] of one shape -> (operand [len(gs), E*C, 1, 1, P], P): their (draw, channel) rows as the input of
    a 1x1 launch whose draws are the tensors.  Read in place when every row sits at one pitch P >= Ho*Wo*B and the tensors one set
    apart in one allocation -- a first layer's gradient as pool_act_backward_chwn(pad_planes=True) writes it: the pad columns are
    contracted too, their results are never read -- else copied once into a dense buffer."""
    g0 = gs[0]
    E, C, Ho, Wo, B = g0.shape
    K, M, P = Ho * Wo * B, E * C, g0.stride(1)
    st = g0.untyped_storage()
    ok = (g0.stride(4) == 1 and g0.stride(3) == B and g0.stride(2) == Wo * B and P >= K and P % 4 == 0 and (E == 1 or g0.stride(0) == C * P)
          and (g0.storage_offset() + len(gs) * M * P) * 4 <= st.nbytes()
          and all(g.shape == g0.shape and g.stride() == g0.stride() and g.untyped_storage().data_ptr() == st.data_ptr()
                  and g.data_ptr() - g0.data_ptr() == i * M * P * 4 for i, g in enumerate(gs)))
    if ok:
        return g0.as_strided((len(gs), M, 1, 1, P), (M * P, P, P, P, 1)), P
    out = torch.empty((len(gs), M, 1, 1, K), dtype=torch.float32, device=g0.device)
    for i, g in enumerate(gs):
        out[i].view(E, C, Ho, Wo, B).copy_(g)
    return out, K


def first_layer_input_grad(g_pre, w, x_hw, stride, padding, dilation, x_lrt=None):
    """d loss / d x of a model's FIRST layer, whose input (the caller's batch) every draw shares -- the sum over draws is part of the
    contraction:
        dx[b, ci, h, w] = sum_e sum_co sum_(r, q) g_pre[e, co, ho, wo, b] * w[e, co, ci, r, q],  h = ho*sh - ph + r*dh, w = wo*sw - pw + q*dw
    Two launches: D[j, ho, wo, b] = sum_(e, co) W[(e, co), j] G[(e, co), ho, wo, b], j = (ci, r, q), on the forward kernel as a 1x1
    "convolution" (g_pre's own memory is its input with E*Cout channels -- as conv2d_chwn_weight_grad_shared_input reads it the other
    way round --, the sampled weights transposed to [J, E*Cout] its weights; follows gemm_mode like every gradient GEMM), then
    bbb_input_grad_col2im folds D onto the input pixels in NCHW (no stride upsampling: no product lands on an inserted zero).
    g_pre [E, Cout, Ho, Wo, B] (the padded-pitch view of pool_act_backward_chwn(pad_planes=True) is read in place), w [E, Cout, Cin,
    kh, kw], x_hw = (H, W) -> dx [B, Cin, H, W].  A first linear layer behind a flatten: kh = kw = 1, H = W = 1, Cin = in_features.
    x_lrt = the layer's input x (a local-reparameterisation layer): g_pre = (g_mu, g_var), each [1, Cout, Ho, Wo, B] (summed over
    draws), w = (W_mu, W_var) [Cout, Cin, kh, kw] -> T(g_mu, W_mu) + 2 x * T(g_var, W_var); the pair runs as the two draws of one GEMM
    launch (in place when g_var sits one set behind g_mu in one buffer)."""
    lrt = x_lrt is not None
    gs = list(g_pre) if lrt else [g_pre]
    ws = [t.contiguous() for t in (w if lrt else [w])]
    require_device(*gs, *ws, x_lrt)
    E, Cout, Ho, Wo, B = gs[0].shape
    Cin, kh, kw = ws[0].shape[-3:]
    H, W = int(x_hw[0]), int(x_hw[1])
    J, M = Cin * kh * kw, E * Cout
    # (the layer itself, for bbb_input_grad_col2im: one slab, no operand of its own)
    d, ho, wo = conv_desc(B, Cin, (H, W), 1, (kh, kw), stride, padding, dilation, w_stride=0, b_stride=0)
    d.x_draw_stride = 0
    if ((ho, wo) != (Ho, Wo)
            or any(t.numel() != M * J for t in ws) or (lrt and (len(gs) != 2 or x_lrt.numel() != B * Cin * H * W))):
        raise _lib.BBBHipError("first_layer_input_grad: geometry mismatch")
    xg, P = _gemm_rows(gs)
    wt = torch.empty((len(gs), J, M, 1, 1), dtype=torch.float32, device=xg.device)
    with on_device(xg.device):
        for i, t in enumerate(ws):
            check(_lib.lib().bbb_transpose2d(t.data_ptr(), wt[i].data_ptr(), M, J, cur_stream(xg.device)), "bbb_transpose2d")
    dcol = conv2d_chwn_forward(xg, wt, None)                          # [len(gs), J, 1, 1, P]
    xc = x_lrt.contiguous() if lrt else None
    dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=xg.device)
    with on_device(dx.device):
        check(_lib.lib().bbb_input_grad_col2im(dcol.data_ptr(), P, J * P, ptr(xc), dx.data_ptr(), ctypes.byref(d), cur_stream(dx.device)),
              "bbb_input_grad_col2im")
    return dx


# ---- bf16 training backward (fast_train._MCForwardBF16._backward on fast_train._Schedule) ---------------

def pool_act_backward_chwn_bf16(g_out, y, k, s, act, out_f32=False, pad_planes=False, avg=None):
    """pool_act_backward_chwn on bf16 storage (bbb_pool_act_bwd_chwn_bf16): y = the stored bf16 activated output [..., H, W, B],
    g_out the bf16 (or, the logits layer's, fp32) gradient w.r.t. the (pooled) output -> g_pre = act'(y) * route(g_out) in fp32,
    rounded once to bf16.  out_f32: the rounded values as fp32 (the first layer's fp32 weight gradient), pad_planes as there.
    y = None (k = 0, no activation): the rounding of g_out alone (the logits layer, whose output is fp32).
    avg = (kernel, stride, padding, count_include_pad): the pool is that average pool instead (avgpool_act_backward_chwn_bf16)."""
    name = "pool_act_backward_chwn_bf16" if avg is None else "avgpool_act_backward_chwn_bf16"
    if g_out.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.BBBHipError(name + ": g_out must be bf16 or fp32")
    require_device(g_out, dtype=g_out.dtype)
    if y is None and avg is None:
        if int(k) != 0 or act is not None:
            raise _lib.BBBHipError("pool_act_backward_chwn_bf16: pooling / activation backward needs the stored output y")
    else:
        require_device(y, dtype=torch.bfloat16)
        y = y.contiguous()
    g_out = g_out.contiguous()
    shape = tuple(g_out.shape) if y is None else tuple(y.shape)
    _, H, W, B, planes = _planes_of(shape)
    if avg is not None:
        _pooled_grad_shape(g_out, planes, H, W, B, avg, bf16=True)
    buf, g_pre, pitch = _grad_buffers(g_out if y is None else y, planes, torch.float32 if out_f32 else torch.bfloat16, pad_planes)
    flags = (1 if g_out.dtype == torch.float32 else 0) | (2 if out_f32 else 0)
    with on_device(g_out.device):
        if avg is not None:
            check(_lib.lib().bbb_avgpool_act_bwd_chwn_bf16(ctypes.byref(_pool_desc(H, W, B, *avg)), g_out.data_ptr(), y.data_ptr(),
                                                           buf.data_ptr(), planes, ACT_CODE[act], pitch, flags, cur_stream(g_out.device)),
                  "bbb_avgpool_act_bwd_chwn_bf16")
        else:
            check(_lib.lib().bbb_pool_act_bwd_chwn_bf16(g_out.data_ptr(), ptr(y), buf.data_ptr(), planes, H, W, B, int(k), int(s),
                                                        ACT_CODE[act], pitch, flags, cur_stream(g_out.device)),
                  "bbb_pool_act_bwd_chwn_bf16")
    return g_pre


def avgpool_act_backward_chwn_bf16(g_out, y, kernel, stride, padding, count_include_pad, act, out_f32=False, pad_planes=False):
    """pool_act_backward_chwn_bf16 behind an AvgPool2d(kernel, stride, padding, count_include_pad=) (bbb_avgpool_act_bwd_chwn_bf16):
    every tap of a window receives that window's gradient over its divisor (fp32, windows in ascending order), times act'(y) from the
    stored bf16 y [..., H, W, B], rounded once to bf16.  g_out bf16 or fp32, of the pooled size; out_f32 / pad_planes as there."""
    return pool_act_backward_chwn_bf16(g_out, y, 0, 1, act, out_f32=out_f32, pad_planes=pad_planes,
                                       avg=(kernel, stride, padding, count_include_pad))


def lrt_pool_act_backward_chwn_bf16(g_out, y, act_var, k, s, act, noise, combine=None, b_offset=0):
    """lrt_pool_act_backward_chwn(stacked=True) on bf16 storage (bbb_lrt_pool_act_bwd_chwn_bf16; LaunchConfig.bf16_lrt_input_grad):
    the activation side of a local-reparameterisation layer's backward -> [2, *y.shape] bf16, [0] = g_mu = act'(y) * route(g), the
    gradient w.r.t. act_mu, [1] = g_var = g_mu * eps / (2 sqrt(act_var)), the gradient w.r.t. act_var, each rounded once.
    y: the layer's stored bf16 activated output [E, C, H, W, B] (None: k = 0 and no activation -- the logits layer, whose output is
    fp32; the shape is then g_out's); act_var fp32, y's shape or one draw's worth [1, C, H, W, B]; g_out bf16 or fp32, of the
    (pooled) output's shape.  noise = (seed, call0, stream_id): eps is the forward's element, regenerated from the counter (draw e of
    the launch under call0 + e; b_offset: the global index of the first image).  combine = (x_out, g_out2): the incoming gradient is
    g_out + 2 * x_out * g_out2 in fp32 -- g_out / g_out2 the layer above's two bf16 input gradients, x_out this layer's (pooled) bf16
    output.  Max pools only: there is no average-pool form."""
    if g_out.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.BBBHipError("lrt_pool_act_backward_chwn_bf16: g_out must be bf16 or fp32")
    require_device(g_out, dtype=g_out.dtype)
    require_device(act_var)
    if y is None:
        if int(k) != 0 or act is not None:
            raise _lib.BBBHipError("lrt_pool_act_backward_chwn_bf16: pooling / activation backward needs the stored output y")
    else:
        require_device(y, dtype=torch.bfloat16)
        y = y.contiguous()
    g_out, act_var = g_out.contiguous(), act_var.contiguous()
    shape = tuple(g_out.shape) if y is None else tuple(y.shape)
    if len(shape) < 4:
        raise _lib.BBBHipError("lrt_pool_act_backward_chwn_bf16: planes [..., C, H, W, B] expected")
    _, H, W, B, planes = _planes_of(shape)
    C = shape[-4]
    mom_planes = act_var.numel() // (H * W * B)
    if act_var.numel() != mom_planes * H * W * B or mom_planes == 0 or planes % mom_planes != 0 or mom_planes % C != 0:
        raise _lib.BBBHipError("lrt_pool_act_backward_chwn_bf16: act_var must hold y's planes, or one draw's worth of them")
    g2p, xcp, x_planes = 0, 0, 0
    if combine is not None:
        if g_out.dtype != torch.bfloat16:
            raise _lib.BBBHipError("lrt_pool_act_backward_chwn_bf16: the combine is of two bf16 input gradients")
        xc, g2 = combine[0].contiguous(), combine[1].contiguous()
        require_device(xc, g2, dtype=torch.bfloat16)
        if g2.numel() != g_out.numel() or xc.numel() == 0 or g_out.numel() % xc.numel() != 0:
            raise _lib.BBBHipError("lrt_pool_act_backward_chwn_bf16: combine = (x_out, g_out2) of g_out's shape (x_out may hold one draw)")
        g2p, xcp, x_planes = g2.data_ptr(), xc.data_ptr(), planes * xc.numel() // g_out.numel()
    ho, wo = (H, W) if int(k) == 0 else pooled_map(H, W, (k, s))
    if g_out.numel() != planes * ho * wo * B:
        raise _lib.BBBHipError("lrt_pool_act_backward_chwn_bf16: g_out must hold %d planes of the map %d x %d x %d" % (planes, ho, wo, B))
    seed, call0, stream_id = noise
    out = torch.empty((2,) + shape, dtype=torch.bfloat16, device=g_out.device)
    with on_device(g_out.device):
        check(_lib.lib().bbb_lrt_pool_act_bwd_chwn_bf16(g_out.data_ptr(), ptr(y), act_var.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                        planes, mom_planes, C, H, W, B, int(k), int(s), ACT_CODE[act], 0, g2p, xcp,
                                                        x_planes, seed, call0 & 0xFFFFFFFF, rng.call_dev_ptr(g_out.device), stream_id,
                                                        int(b_offset), 1 if g_out.dtype == torch.float32 else 0,
                                                        cur_stream(g_out.device)), "bbb_lrt_pool_act_bwd_chwn_bf16")
    return out


def first_layer_input_grad_bf16_lrt(g_pair, w_mu, w_var, w_shape, x_hw, stride, padding, dilation, x_b):
    """first_layer_input_grad(x_lrt=) on the bf16 LRT node's operands: d loss / d x of a local-reparameterisation FIRST layer,
        dx = T(g_mu, W_mu) + 2 x_b * T(g_var, sigma^2),   T(g, w)[b, ci, h, w] = sum_e sum_co sum_(r, q) g[e, co, ho, wo, b] * w[co, ci, r, q]
    g_pair [2, E, Cout, Ho, Wo, B] bf16 (lrt_pool_act_backward_chwn_bf16: the per-draw g_mu / g_var as they are -- the sum over
    draws is part of the fp32 accumulation); w_mu / w_var: the bf16 rows [Cout, Kp] of lrt_weights_bf16 for weights w_shape = (Cout, Cin,
    kh, kw), shared by every draw (one small copy per draw: the contraction reads one weight set per draw); x_b [B, Cin, H, W] fp32, the
    bf16-rounded input the forward multiplied.  Two launches of bbb_first_layer_dgrad_bf16 into the two sets of one buffer, then
    bbb_input_grad_col2im in its LRT form (fmaf(2 x, set 1, set 0)); nothing is rounded -> dx [B, Cin, H, W] fp32."""
    require_device(g_pair, w_mu, w_var, dtype=torch.bfloat16)
    require_device(x_b)
    Cout, Cin, kh, kw = (int(v) for v in w_shape)
    if g_pair.dim() != 6 or g_pair.shape[0] != 2 or w_mu.dim() != 2 or w_mu.shape != w_var.shape:
        raise _lib.BBBHipError("first_layer_input_grad_bf16_lrt: g_pair [2, E, Cout, Ho, Wo, B] and rows [Cout, Kp] expected")
    _, E, _, Ho, Wo, B = g_pair.shape
    H, W = int(x_hw[0]), int(x_hw[1])
    J = Cin * kh * kw
    d, ho, wo = _first_layer_desc(B, Cin, Cout, kh, kw, (H, W), stride, padding, dilation, E)
    if ((ho, wo) != (Ho, Wo) or g_pair.shape[2] != Cout or tuple(w_mu.shape) != (Cout, bf16_row_pitch(J))
            or x_b.numel() != B * Cin * H * W):
        raise _lib.BBBHipError("first_layer_input_grad_bf16_lrt: geometry mismatch")
    g_pair, x_b = g_pair.contiguous(), x_b.contiguous()
    K = Ho * Wo * B
    flags = 2 if bf16_tap_major((Cout, Cin, kh, kw)) else 0
    dcol = torch.empty((2, J, K), dtype=torch.float32, device=g_pair.device)
    dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=g_pair.device)
    with on_device(g_pair.device):
        st = cur_stream(g_pair.device)
        for i, w in enumerate((w_mu, w_var)):
            rows = w.unsqueeze(0).expand(E, -1, -1).contiguous()
            check(_lib.lib().bbb_first_layer_dgrad_bf16(ctypes.byref(d), g_pair[i].data_ptr(), K, rows.data_ptr(), dcol[i].data_ptr(), K,
                                                        flags, st), "bbb_first_layer_dgrad_bf16")
        check(_lib.lib().bbb_input_grad_col2im(dcol.data_ptr(), K, J * K, x_b.data_ptr(), dx.data_ptr(), ctypes.byref(d), st),
              "bbb_input_grad_col2im")
    return dx


def plane_sums_bf16(g):
    """plane_sums of a bf16 g [E, C, H, W, B]: -> fp32 [E, C] (bbb_plane_sum_bf16, fp32 accumulation in a fixed order)."""
    require_device(g, dtype=torch.bfloat16)
    g = g.contiguous()
    E, C, H, W, B = g.shape
    out = torch.empty((E, C), dtype=torch.float32, device=g.device)
    with on_device(g.device):
        check(_lib.lib().bbb_plane_sum_bf16(g.data_ptr(), out.data_ptr(), E * C, H * W * B, H * W * B, cur_stream(g.device)),
              "bbb_plane_sum_bf16")
    return out


def flip_transpose_w_bf16(w, w_shape):
    """The input gradient's weight operand from sampled bf16 rows: w [E, Cout, Kp] (sample_weights_bf16's layout and column order,
    bf16_tap_major(w_shape)) of a layer with weights w_shape = (Cout, Cin, kh, kw) -> [E, Cin, Kp'] with the taps flipped and the
    channels transposed, Kp' = Cout * kh * kw rounded up to 8, tap-major where bf16_tap_major((Cin, Cout, kh, kw))."""
    require_device(w, dtype=torch.bfloat16)
    w = w.contiguous()
    Cout, Cin, kh, kw = w_shape
    E = w.shape[0]
    if w.shape[1] != Cout or w.shape[2] != bf16_row_pitch(Cin * kh * kw):
        raise _lib.BBBHipError("flip_transpose_w_bf16: rows do not match the weight shape")
    flags = (1 if bf16_tap_major((Cout, Cin, kh, kw)) else 0) | (2 if bf16_tap_major((Cin, Cout, kh, kw)) else 0)
    out = torch.empty((E, Cin, bf16_row_pitch(Cout * kh * kw)), dtype=torch.bfloat16, device=w.device)
    with on_device(w.device):
        check(_lib.lib().bbb_flip_transpose_w_bf16(w.data_ptr(), out.data_ptr(), E, Cout, Cin, kh * kw, flags, cur_stream(w.device)),
              "bbb_flip_transpose_w_bf16")
    return out


def _bf16_dgrad_launch(B, cin, cout, kh, kw, g_hw, pad, dilation, draws):
    """The descriptor of bbb_conv2d_chwn_bf16_dgrad: the stride-1 launch on the flipped rows [cin, Kp'] of a layer with weights (cout,
    cin, kh, kw) over g's map g_hw, pad = dilation * (k - 1) - the layer's padding."""
    return conv_desc(B, cout, g_hw, cin, (kh, kw), 1, pad, dilation, draws, w_stride=cin * bf16_row_pitch(cout * kh * kw), b_stride=0)[0]


def bf16_dgrad_form(B, cin, cout, kh, kw, x_hw, stride, dilation, draws):
    """(tile shape 22 | 14 | 12, k-groups 1 | 2, wave-specialised, tap-major rows) bbb_conv2d_chwn_bf16_dgrad picks for the input
    gradient of a strided layer with weights (cout, cin, kh, kw), input map x_hw = (H, W), `draws` draws of B images: the launch
    entry's own plan (bbb_conv2d_chwn_bf16_dgrad_plan, csrc/pconv_bf16_plan.h: dgrad_tile_rule; host only).  The selection does
    not depend on the layer's padding; the descriptor asked about is the layer with padding dilation * (k - 1), whose output map
    exists for every input map."""
    (sh, sw), (dh, dw) = _pair(stride), _pair(dilation)
    H, W = int(x_hw[0]), int(x_hw[1])
    tap_major = bf16_tap_major((cin, cout, kh, kw))
    g_hw = out_map(H, W, (kh, kw), (sh, sw), (dh * (kh - 1), dw * (kw - 1)), (dh, dw))
    d = _bf16_dgrad_launch(B, cin, cout, kh, kw, g_hw, 0, (dh, dw), int(draws))
    shape, kg, ws = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    check(_lib.lib().bbb_conv2d_chwn_bf16_dgrad_plan(ctypes.byref(d), sh, sw, H, W, 2 if tap_major else 0, ctypes.byref(shape),
                                                     ctypes.byref(kg), ctypes.byref(ws)), "bbb_conv2d_chwn_bf16_dgrad_plan")
    return shape.value, kg.value, bool(ws.value), tap_major


def conv2d_chwn_input_grad_bf16(g_pre, w, w_shape, x_hw, padding, dilation, w_flipped=None, stride=1):
    """conv2d_chwn_input_grad on bf16 storage: g_pre [E, Cout, Ho, Wo, B] bf16, w [E, Cout, Kp] sampled bf16 rows of a layer with
    weights w_shape = (Cout, Cin, kh, kw) -> bf16 [E, Cin, H, W, B] for x_hw = (H, W); fp32 accumulation, one rounding.
    w_flipped: flip_transpose_w_bf16(w, w_shape) computed ahead.
    stride 1 (the default): conv2d_chwn_bf16_forward on the flipped rows, padding d*(k-1) - p.
    Any other stride: the transposed form of the general bf16 GEMM (bbb_conv2d_chwn_bf16_dgrad, csrc/pconv_bf16.hip) on the same
    flipped rows -- with tap-major rows (Cout % 8 == 0) exactly the forward's in-bounds (pixel, tap) pairs, with reference-order rows
    the full row against image rows read as zero; input pixels no tap reaches come back as +0 (bf16_dgrad_form: the launch form)."""
    Cout, Cin, kh, kw = w_shape
    (ph, pw), (dh, dw), (sh, sw) = _pair(padding), _pair(dilation), _pair(stride)
    qh, qw = dh * (kh - 1) - ph, dw * (kw - 1) - pw
    if qh < 0 or qw < 0:
        raise _lib.BBBHipError("conv2d_chwn_input_grad_bf16: padding larger than the kernel reach")
    w_t = w_flipped if w_flipped is not None else flip_transpose_w_bf16(w, w_shape)
    tap_major = bf16_tap_major((Cin, Cout, kh, kw))
    if (sh, sw) == (1, 1):
        gx = conv2d_chwn_bf16_forward(g_pre, w_t, None, (Cout, kh, kw), 1, (qh, qw), (dh, dw), tap_major=tap_major)
        if gx.shape[2] != x_hw[0] or gx.shape[3] != x_hw[1]:
            raise _lib.BBBHipError("conv2d_chwn_input_grad_bf16: geometry mismatch (x_hw is not this stride-1 layer's input map)")
        return gx
    if sh < 1 or sw < 1:
        raise _lib.BBBHipError("conv2d_chwn_input_grad_bf16: strides are positive")
    require_device(g_pre, w_t, dtype=torch.bfloat16)
    g_pre, w_t = g_pre.contiguous(), w_t.contiguous()
    if g_pre.dim() != 5 or w_t.dim() != 3:
        raise _lib.BBBHipError("g_pre [E|1, Cout, Ho, Wo, B] and flipped rows [E|1, Cin, Kp] expected")
    if g_pre.shape[1] != Cout or w_t.shape[1] != Cin or w_t.shape[2] != bf16_row_pitch(Cout * kh * kw):
        raise _lib.BBBHipError("conv2d_chwn_input_grad_bf16: rows do not match the weight shape")
    H, W, B = int(x_hw[0]), int(x_hw[1]), g_pre.shape[4]
    d = _bf16_dgrad_launch(B, Cin, Cout, kh, kw, (g_pre.shape[2], g_pre.shape[3]), (qh, qw), (dh, dw), 1)
    E, _, _ = slab_rule(d, g_pre.shape[0], w_t.shape[0])
    gx = torch.empty((E, Cin, H, W, B), dtype=torch.bfloat16, device=g_pre.device)
    with on_device(g_pre.device):
        check(_lib.lib().bbb_conv2d_chwn_bf16_dgrad(ctypes.byref(d), g_pre.data_ptr(), w_t.data_ptr(), gx.data_ptr(), sh, sw, H, W,
                                                    2 if tap_major else 0, cur_stream(g_pre.device)), "bbb_conv2d_chwn_bf16_dgrad")
    return gx


def _first_layer_desc(B, cin, cout, kh, kw, x_hw, stride, padding, dilation, draws):
    """The descriptor of bbb_first_layer_dgrad_bf16 (and of the gather behind it): the LAYER, its weight sets one set of bf16 rows apart."""
    d, ho, wo = conv_desc(B, cin, (int(x_hw[0]), int(x_hw[1])), cout, (kh, kw), stride, padding, dilation, int(draws),
                          w_stride=cout * bf16_row_pitch(cin * kh * kw), b_stride=0)
    d.x_draw_stride = 0
    return d, ho, wo


def first_layer_dgrad_bf16_plan(B, w_shape, x_hw, stride=1, padding=0, dilation=1, draws=1, g_row_pitch=None, d_row_pitch=None,
                                g_f32=False, tap_major=None):
    """(rows of D per workgroup 32 | 64, columns per workgroup, steps of the contraction, workgroups) of the launch
    first_layer_input_grad_bf16 makes for a layer with weights w_shape = (Cout, Cin, kh, kw) over `draws` draws of B images on the map
    x_hw: the launch entry's own plan (bbb_first_layer_dgrad_bf16_plan, csrc/input_grad_bf16_plan.h; host only).  The pitches default
    to a dense row, tap_major to bf16_tap_major(w_shape).  What the entry refuses raises BBBHipError with its code."""
    Cout, Cin, kh, kw = (int(v) for v in w_shape)
    d, ho, wo = _first_layer_desc(B, Cin, Cout, kh, kw, x_hw, stride, padding, dilation, draws)
    K = max(ho, 0) * max(wo, 0) * B
    tm = bf16_tap_major((Cout, Cin, kh, kw)) if tap_major is None else bool(tap_major)
    tj, tn, kc, blocks = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    check(_lib.lib().bbb_first_layer_dgrad_bf16_plan(ctypes.byref(d), K if g_row_pitch is None else int(g_row_pitch),
                                                     K if d_row_pitch is None else int(d_row_pitch), (1 if g_f32 else 0) | (2 if tm else 0),
                                                     ctypes.byref(tj), ctypes.byref(tn), ctypes.byref(kc), ctypes.byref(blocks)),
          "bbb_first_layer_dgrad_bf16_plan")
    return tj.value, tn.value, kc.value, blocks.value


def first_layer_input_grad_bf16(g_pre, w, w_shape, x_hw, stride, padding, dilation):
    """first_layer_input_grad on the bf16 node's operands: d loss / d x of a model's FIRST layer, summed over the draws,
        dx[b, ci, h, w] = sum_e sum_co sum_(r, q) g_pre[e, co, ho, wo, b] * w[e, co, ci, r, q],  h = ho*sh - ph + r*dh, w = wo*sw - pw + q*dw
    in two launches: bbb_first_layer_dgrad_bf16 (csrc/input_grad_bf16.hip: D[(ci, r, q)] = the contraction over (e, co) on the bf16
    MFMA, fp32 accumulation, both operands read where they are) and bbb_input_grad_col2im, the fp32 path's gather.  Nothing is
    rounded: dx is fp32 like the caller's x.
    g_pre [E, Cout, Ho, Wo, B]: bf16, or fp32 holding bf16 values (pool_act_backward_chwn_bf16(out_f32=True)); a view whose (draw,
    channel) planes sit at one pitch (% 8 == 0: pad_planes=True) is read in place, anything else is made contiguous first.
    w: the sampled bf16 rows [E, Cout, Kp] of a layer with weights w_shape = (Cout, Cin, kh, kw) (sample_weights_bf16's layout and
    column order, bf16_tap_major(w_shape)); x_hw = (H, W) -> dx [B, Cin, H, W] fp32.  A first linear layer behind a flatten:
    kh = kw = 1, H = W = 1, Cin = in_features."""
    if g_pre.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.BBBHipError("first_layer_input_grad_bf16: g_pre must be bf16, or fp32 holding bf16 values")
    require_device(g_pre, dtype=g_pre.dtype)
    require_device(w, dtype=torch.bfloat16)
    Cout, Cin, kh, kw = (int(v) for v in w_shape)
    if g_pre.dim() != 5 or w.dim() != 3:
        raise _lib.BBBHipError("first_layer_input_grad_bf16: g_pre [E, Cout, Ho, Wo, B] and rows [E, Cout, Kp] expected")
    E, _, Ho, Wo, B = g_pre.shape
    H, W = int(x_hw[0]), int(x_hw[1])
    J = Cin * kh * kw
    d, ho, wo = _first_layer_desc(B, Cin, Cout, kh, kw, (H, W), stride, padding, dilation, E)
    if (ho, wo) != (Ho, Wo) or g_pre.shape[1] != Cout or tuple(w.shape) != (E, Cout, bf16_row_pitch(J)):
        raise _lib.BBBHipError("first_layer_input_grad_bf16: geometry mismatch")
    w = w.contiguous()
    K, P = Ho * Wo * B, g_pre.stride(1)
    if not (g_pre.stride(4) == 1 and g_pre.stride(3) == B and g_pre.stride(2) == Wo * B and P >= K and P % 8 == 0
            and (E == 1 or g_pre.stride(0) == Cout * P)):
        g_pre, P = g_pre.contiguous(), K
    flags = (1 if g_pre.dtype == torch.float32 else 0) | (2 if bf16_tap_major((Cout, Cin, kh, kw)) else 0)
    dcol = torch.empty((J, K), dtype=torch.float32, device=g_pre.device)
    dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=g_pre.device)
    with on_device(g_pre.device):
        st = cur_stream(g_pre.device)
        check(_lib.lib().bbb_first_layer_dgrad_bf16(ctypes.byref(d), g_pre.data_ptr(), P, w.data_ptr(), dcol.data_ptr(), K, flags, st),
              "bbb_first_layer_dgrad_bf16")
        check(_lib.lib().bbb_input_grad_col2im(dcol.data_ptr(), K, 0, 0, dx.data_ptr(), ctypes.byref(d), st), "bbb_input_grad_col2im")
    return dx


def chwn_to_bhwc_bf16(x, c_pad=None):
    """bf16 [E, C, H, W, B] -> [E, B, H, W, Cp] (bbb_chwn_to_bhwc_bf16), Cp = c_pad (default C rounded up to 8), pad channels zero."""
    require_device(x, dtype=torch.bfloat16)
    x = x.contiguous()
    E, C, H, W, B = x.shape
    Cp = ((C + 7) & ~7) if c_pad is None else int(c_pad)
    out = torch.empty((E, B, H, W, Cp), dtype=torch.bfloat16, device=x.device)
    with on_device(x.device):
        check(_lib.lib().bbb_chwn_to_bhwc_bf16(x.data_ptr(), out.data_ptr(), E, C, H * W, B, Cp, cur_stream(x.device)), "bbb_chwn_to_bhwc_bf16")
    return out


def batch_chunks_bf16(g, chunks):
    """bf16 [E, *R, B] -> [E, S, *R, B / S] (bbb_batch_chunks_bf16): S batch chunks of each row, chunk-major."""
    require_device(g, dtype=torch.bfloat16)
    g = g.contiguous()
    E, B = g.shape[0], g.shape[-1]
    S = int(chunks)
    R = g.numel() // (E * B)
    out = torch.empty((E, S) + tuple(g.shape[1:-1]) + (B // S,), dtype=torch.bfloat16, device=g.device)
    with on_device(g.device):
        check(_lib.lib().bbb_batch_chunks_bf16(g.data_ptr(), out.data_ptr(), E, R, B, S, cur_stream(g.device)), "bbb_batch_chunks_bf16")
    return out


def wgrad_batch_chunks_bf16(E, Cout, Cp, kh, kw, B):
    """The number S of batch chunks conv2d_chwn_weight_grad_bf16 runs as extra draws (a K split): doubled while the role-swapped
    launch (workgroups of one output pixel x 64 channels x 128 images) would occupy fewer than 512 workgroups and every chunk
    keeps >= 16 images, a multiple of 8."""
    wgs = E * kh * kw * -(-Cout // 64) * -(-Cp // 128)
    S = 1
    while wgs * S < 512 and B % (16 * S) == 0 and B // (2 * S) >= 16:
        S *= 2
    return S


wgrad_chunks_bf16 = [True]      # False: one role-swapped launch reading the output gradient in place, whatever its size


def conv2d_chwn_weight_grad_bf16(g_pre, x, w_shape, stride, padding, dilation):
    """conv2d_chwn_weight_grad on bf16 storage, on the bf16 forward kernel with the roles swapped: the batch becomes the contraction
    channels, the layer's input channels (padded with zero planes to a multiple of 8) the 16-byte "image" axis, the output pixels
    the kernel taps.  g_pre [E, Cout, Ho, Wo, B] bf16 IS a tap-major weight operand (taps = output pixels, channels = images, row
    length Ho*Wo*B): read in place, or -- when the launch would leave the chip short of workgroups -- as S batch chunks
    (batch_chunks_bf16) that run as extra draws and are summed in a fixed order.  x [E|1, Cin, H, W, B] bf16 ->
    fp32 [E, Cout, Cin, kh, kw] (fp32 accumulation, never rounded)."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    Ew, Cout, Cin, kh, kw = w_shape
    E, B = g_pre.shape[0], g_pre.shape[4]
    Ho, Wo = g_pre.shape[2], g_pre.shape[3]
    Cp = (Cin + 7) & ~7
    S = wgrad_batch_chunks_bf16(E, Cout, Cp, kh, kw, B) if wgrad_chunks_bf16[0] else 1
    xr = chwn_to_bhwc_bf16(x, Cp)                                      # [E|1, B, H, W, Cp]
    if S > 1:
        gr = batch_chunks_bf16(g_pre, S).reshape(E * S, Cout, Ho * Wo * (B // S))
        if xr.shape[0] == 1 and E > 1:
            xr = xr.expand(E, *xr.shape[1:])
        xr = xr.reshape(xr.shape[0] * S, B // S, *xr.shape[2:])
    else:
        gr = g_pre.contiguous().reshape(E, Cout, Ho * Wo * B)
    Bs = B // S
    y = conv2d_chwn_bf16_forward(xr, gr, None, (Bs, Ho, Wo), (dh, dw), (ph, pw), (sh, sw), out_f32=True,
                                 tap_major=Ho * Wo > 1)               # [E*S, Cout, kh', kw', Cp] fp32, kh' >= kh
    T = kh * kw
    if y.shape[2] == kh and y.shape[3] == kw:
        gw = torch.empty((E, Cout, Cin, kh, kw), dtype=torch.float32, device=y.device)
        if _transpose_sum_batched(y, gw, T, Cin, (E, Cout, 1), (S * Cout * T * Cp, T * Cp, 0), (Cout * Cin * T, Cin * T, 0), Cp, T,
                                  S, Cout * T * Cp):
            return gw
    if S > 1:
        y = y.reshape(E, S, *y.shape[1:]).sum(1)
    return y[:, :, :kh, :kw, :Cin].permute(0, 1, 4, 2, 3).contiguous()


class _OpsModule(types.ModuleType):
    """`ops.gemm_mode`, `ops.split_k`, ... read and write the fields of the process-default LaunchConfig (compatibility with the
    round-1..4 switches; prefer `use_config` / `launch_config=`)."""

    def __getattr__(self, name):                     # only reached when the module dict has no such name
        if name in LaunchConfig.FIELDS:
            return getattr(_default_config, name)
        raise AttributeError(f"module {self.__name__!r} has no attribute {name!r}")

    def __setattr__(self, name, value):
        if name in LaunchConfig.FIELDS:
            setattr(_default_config, name, value)
        else:
            super().__setattr__(name, value)


sys.modules[__name__].__class__ = _OpsModule
