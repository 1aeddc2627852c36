"""Average pooling on the batch-innermost paths, host side: the descriptor of a launch (bbb_pool_desc_t), the launches' own plan
(bbb_avgpool_plan, csrc/pool_plan.h) and THE statement of which modules are admitted (avgpool_of).  No tensors, no device.  bbb_hip.ops
re-exports all of it (ops.avgpool_of, ...); the walks (ensemble, infer_walk, fast_train) ask here directly: these are queries, not
launches, and how often a walk asks them is not part of its schedule."""
import ctypes

import torch

from . import _lib
from ._lib import check
from .conv_desc import _pair


def pool_desc(H, W, B, kernel, stride, padding, count_include_pad):
    d = _lib.PoolDesc()
    d.kind, d.h, d.w, d.batch = _lib.POOL_AVG, int(H), int(W), int(B)
    (d.kh, d.kw), (d.stride_h, d.stride_w), (d.pad_h, d.pad_w) = _pair(kernel), _pair(stride), _pair(padding)
    d.count_include_pad = 1 if count_include_pad else 0
    return d


def avgpool_plan(H, W, B, kernel, stride, padding=0, count_include_pad=True, planes=1, out_plane_pitch=0):
    """(ho, wo, forward workgroups, backward workgroups) of the average-pool launches on `planes` planes [H, W, B]
    (bbb_avgpool_plan, the launch entries' own plan; host only: needs no device).  A geometry the launches refuse raises their error."""
    return _plan("bbb_avgpool_plan", pool_desc(H, W, B, kernel, stride, padding, count_include_pad), planes, out_plane_pitch)


def avgpool_bf16_plan(H, W, B, kernel, stride, padding=0, count_include_pad=True, planes=1, out_plane_pitch=0):
    """avgpool_plan of the launches on bf16 planes (bbb_avgpool_bf16_plan: 16-byte groups of 8 images, so B % 8 == 0 and a pitch
    that is a multiple of 8; every other check shared with avgpool_plan).  Host only."""
    return _plan("bbb_avgpool_bf16_plan", pool_desc(H, W, B, kernel, stride, padding, count_include_pad), planes, out_plane_pitch)


def _plan(entry, d, planes, out_plane_pitch):
    ho, wo, fb, bb = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(getattr(_lib.lib(), entry)(ctypes.byref(d), int(planes), int(out_plane_pitch), ctypes.byref(ho), ctypes.byref(wo),
                                     ctypes.byref(fb), ctypes.byref(bb)), entry)
    return ho.value, wo.value, fb.value, bb.value


def _int_pair(v):
    """(a, b) for an int or a pair of ints (bools are not sizes), else None."""
    if isinstance(v, int) and not isinstance(v, bool):
        return (v, v)
    if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(a, int) and not isinstance(a, bool) for a in v):
        return (v[0], v[1])
    return None


def is_avgpool(module):
    """An average-pooling module of a kind avgpool_of may admit (which it does depends on the map it meets)."""
    return isinstance(module, (torch.nn.AvgPool2d, torch.nn.AdaptiveAvgPool2d))


def avgpool_of(module, H, W):
    """THE statement of which average-pooling modules the batch-innermost paths admit: (kernel, stride, padding, count_include_pad)
    -- pairs and a bool, what avgpool_chwn and the backward wrappers take -- for such a module on an H x W map, else None.
    nn.AvgPool2d: int or pair arguments, stride=None meaning the kernel, ceil_mode=False, divisor_override=None, and a geometry the
    launches take (pool_plan.h: 2 * pad <= k, a window within the padded map, ...).  nn.AdaptiveAvgPool2d: an output size (an int or a
    pair of ints) that divides H and W -- it is then the window (H / oh, W / ow) at the same stride, no padding."""
    if isinstance(module, torch.nn.AdaptiveAvgPool2d):
        o = _int_pair(module.output_size)
        if o is None or min(o) < 1 or H % o[0] != 0 or W % o[1] != 0:
            return None
        spec = ((H // o[0], W // o[1]),) * 2 + ((0, 0), True)
    elif isinstance(module, torch.nn.AvgPool2d):
        k, p = _int_pair(module.kernel_size), _int_pair(module.padding)
        s = k if module.stride is None else _int_pair(module.stride)
        if k is None or s is None or p is None or module.ceil_mode or module.divisor_override is not None:
            return None
        spec = (k, s, p, bool(module.count_include_pad))
    else:
        return None
    try:
        avgpool_plan(H, W, 4, *spec)
    except _lib.BBBHipError:
        return None
    return spec
