"""The reference of the inference forward, on the CPU: one stochastic forward of a model, module by module in NCHW, written from the
reference's layer definitions (layers/BBB/*.py, layers/BBB_LRT/*.py, layers/misc.py) and fed the device's Philox noise restated by
oracle/bbb_numpy.normal_eps.  Nothing here launches anything or reads bbb_hip.infer_walk: tests/test_gpu_infer_walk_ref.py holds the
batch-innermost walk (ensemble._mc_logits_chwn) to it by value, tests/test_infer_ref_cpu.py holds it to the oracle's zoo forward.

    forward64     logits [rows, classes] of one draw on a block of images
    kl64          the closed-form KL of every Bayesian layer
    slab_sources  which images, which noise call and which global image offset every output slab of a partitioned call has:
                  restated from the DOCSTRING of infer_walk.chwn_partition, not from its code
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import bbb_numpy as O

F32 = np.float32


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


class _Arith:
    """The three ways the forward is stated.  rounding=None: every operation in `dtype` (float64: the reference; float32: its fp32
    twin, plain CPU fp32).  rounding="fp32": float64 contractions on operands and results HELD as fp32 exactly where
    oracle.bbb_numpy.model_forward holds them (its elementwise float32 functions are used for those steps), so that the result is the
    oracle's value for value.  rounding="bf16": the holds of "fp32" and the storage roundings of the bf16 contract
    (bbb_numpy.model_forward_bf16, tests/bf16_lrt_contract.py, tests/bf16_avgpool_contract.py)."""

    def __init__(self, dtype, rounding):
        assert rounding in (None, "fp32", "bf16") and (rounding is None or dtype == torch.float64)
        self.dtype, self.hold, self.bf16 = dtype, rounding is not None, rounding == "bf16"

    def held(self, t):
        return t.float().to(self.dtype) if self.hold else t

    def stored(self, t):                                 # an activation (or the input) as the bf16 path stores it
        return _t(O.bf16_round(t.float().numpy()), self.dtype) if self.bf16 else t

    def operand(self, t):                                # a weight operand of a contraction as the bf16 path stores it
        return self.stored(t)

    def sigma(self, rho):
        if self.hold:
            return _t(O.sigma_from_rho(rho.float().numpy()), self.dtype)
        return torch.log1p(torch.exp(rho.to(self.dtype)))

    def reparam(self, mu, sigma, eps):
        if self.hold:
            return _t(O.reparam(mu.float().numpy(), sigma.float().numpy(), eps), self.dtype)
        return mu.to(self.dtype) + _t(eps, self.dtype) * sigma

    def square(self, t):
        return self.held(t.float() * t.float()) if self.hold else t * t

    def lrt_out(self, am, av, eps):
        if self.hold:
            return _t(O.lrt_output(am.float().numpy(), av.float().numpy(), eps), self.dtype)
        return am + torch.sqrt(av) * _t(eps, self.dtype)

    def var_floor(self, v):
        if self.hold:
            return _t((F32(1e-16) + v.float().numpy()).astype(F32), self.dtype)
        return 1e-16 + v

    def softplus(self, t):
        return _t(O.softplus_act(t.float().numpy()), self.dtype) if self.hold else F.softplus(t)


def _kinds():
    from layers.bbb import _BBBLayer
    from layers.lrt import _LRTLayer
    from layers.misc import FlattenLayer
    return _BBBLayer, _LRTLayer, FlattenLayer


def _param(p, dtype):
    return None if p is None else p.detach().cpu().to(dtype)


def forward64(net, x, seed, call, b_offset=0, dtype=torch.float64, rounding=None, trace=None):
    """One stochastic forward of `net` on the images x [n, C, H, W] under noise call `call` -> logits [rows, classes] in `dtype`.
    b_offset: the global index of x's first image (LRT activation noise is keyed by the NCHW output index of the GLOBAL image; behind
    a flatten that cuts every image into r rows the "image" index is (b_offset + b) * r + row).  dtype / rounding: _Arith.
    trace: a list that receives (module, its output) for every module (the CPU tests look at the intermediate activations)."""
    from bbb_hip import ensemble
    BBB, LRT, Flatten = _kinds()
    A = _Arith(dtype, rounding)
    mods = ensemble.flat_children(net)
    last = max(i for i, m in enumerate(mods) if isinstance(m, (BBB, LRT)))
    h = A.stored(A.held(x.detach().cpu().to(dtype)))
    boff = int(b_offset)

    def eps(stream, shape, start=0):
        n = int(np.prod(shape))
        return O.normal_eps(seed, call, stream, n, start=start).reshape(shape)

    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, (BBB, LRT)):
            conv = hasattr(m, "kernel_size")
            if not conv and h.dim() != 2:
                h = h.reshape(h.shape[0], -1)

            def lin(inp, w, b):
                y = F.conv2d(inp, w, b, m.stride, m.padding, m.dilation) if conv else F.linear(inp, w, b)
                return A.held(y)
            W_mu, W_rho, b_mu, b_rho = (_param(getattr(m, n), dtype) for n in ("W_mu", "W_rho", "bias_mu", "bias_rho"))
            sid = m._stream_base
            if isinstance(m, BBB):
                w = A.operand(A.reparam(W_mu, A.sigma(W_rho), eps(sid, tuple(W_mu.shape))))
                b = None if b_mu is None else A.reparam(b_mu, A.sigma(b_rho), eps(sid + 1, tuple(b_mu.shape)))
                y = lin(h, w, b)
            else:
                s_w = A.sigma(W_rho)
                b_var = None if b_mu is None else A.held(A.sigma(b_rho) ** 2)
                am = lin(h, A.operand(W_mu), b_mu)
                av = A.var_floor(lin(A.stored(A.square(h)), A.operand(A.held(s_w * s_w)), b_var))
                per_image = int(np.prod(am.shape[1:]))
                y = A.lrt_out(am, av, eps(sid + 2, tuple(am.shape), start=boff * per_image))
            fused = i + 1 < len(mods) and isinstance(mods[i + 1], (nn.ReLU, nn.Softplus))
            if trace is not None:
                trace.append((m, y))
            if fused:                                    # (the bf16 contract: one rounding, behind the activation)
                i += 1
                y = torch.relu(y) if isinstance(mods[i], nn.ReLU) else A.softplus(y)
            h = y if i >= last else A.stored(y)
        elif isinstance(m, nn.ReLU):
            h = A.stored(torch.relu(h))
        elif isinstance(m, nn.Softplus):
            h = A.stored(A.softplus(h))
        elif isinstance(m, nn.MaxPool2d):
            h = F.max_pool2d(h, m.kernel_size, m.stride, m.padding, m.dilation, m.ceil_mode)
        elif isinstance(m, nn.AvgPool2d):
            h = A.stored(A.held(F.avg_pool2d(h, m.kernel_size, m.stride, m.padding, m.ceil_mode, m.count_include_pad, m.divisor_override)))
        elif isinstance(m, nn.AdaptiveAvgPool2d):
            h = A.stored(A.held(F.adaptive_avg_pool2d(h, m.output_size)))
        elif isinstance(m, Flatten):
            rows = h.shape[0]
            h = h.reshape(-1, m.num_features)            # the reference's view(-1, num_features), layers/misc.py
            boff = boff * (h.shape[0] // rows)
        else:
            raise TypeError(f"no reference for {type(m).__name__}")
        if trace is not None:
            trace.append((mods[i], h))
        i += 1
    return h


def kl64(net):
    """The closed-form KL of all Bayesian layers, float64 sum of the oracle's per-element terms (bbb_numpy.kl_loss)."""
    from bbb_hip import ensemble
    kl = 0.0
    for m in ensemble.bayesian_layers(net):
        for mu, rho in ((m.W_mu, m.W_rho), (m.bias_mu, m.bias_rho)):
            if mu is not None:
                kl += O.kl_loss(mu.detach().cpu().numpy(), O.sigma_from_rho(rho.detach().cpu().numpy()), m.prior_mu, m.prior_sigma)
    return kl


def slab_sources(x_shape, draws, call0, units=None, groups=1, share=None, b_offset=0):
    """[(image range (i0, i1) of x, noise call, global index of image i0)] per output slab of a call, as the chwn_partition docstring
    states it (and _mc_logits_chwn's for b_offset):
      unpartitioned         slab j: every image, call call0 + j, images counted from b_offset
      units = (S, lo, hi)   the units lo..hi-1 of the draw-major grid u = j * S + s: slab u - lo is slice s = images
                            [s B / S, (s + 1) B / S) of draw j under call0 + j; its images keep their global indices
      groups = G            x holds G batches back to back: slab g * draws + j is batch g under call0 + g * draws + j; every batch is
                            a step of its own, its images counted from b_offset
      share = (D, off)      slab e is batch (e + off) // D of the ceil((draws + off) / D) batches in x, under call0 + e
    An odd batch is padded inside the call and the padding dropped again: the real images only, which is what this returns anyway."""
    B = int(x_shape[0])
    if units is not None and units[0] > 1:
        S, lo, hi = units
        n = B // S
        return [((u % S) * n, (u % S + 1) * n, call0 + u // S, b_offset + (u % S) * n) for u in range(lo, hi)]
    if groups > 1:
        n = B // groups
        return [(g * n, (g + 1) * n, call0 + g * draws + j, b_offset) for g in range(groups) for j in range(draws)]
    if share is not None:
        D, off = share
        n = B // -(-(draws + off) // D)
        return [(((e + off) // D) * n, ((e + off) // D + 1) * n, call0 + e, b_offset) for e in range(draws)]
    return [(0, B, call0 + j, b_offset) for j in range(draws)]
