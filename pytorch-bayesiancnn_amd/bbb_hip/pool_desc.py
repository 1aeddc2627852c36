"""Pooling on the batch-innermost paths, host side, maximum and average: the descriptor of a launch (bbb_pool_desc_t), the launches'
own plan (bbb_avgpool_plan / bbb_avgpool_bf16_plan, csrc/pool_plan.h: one plan for both kinds) and THE statement of which modules are
admitted (pool_of; avgpool_of is its average-only view).  No tensors, no device.  bbb_hip.ops re-exports all of it (ops.pool_of,
ops.avgpool_of, ...); the walks (ensemble, infer_walk, fast_train) ask here directly: these are queries, not launches, and how often
a walk asks them is not part of its schedule."""
import ctypes

import torch

from . import _lib
from ._lib import check
from .conv_desc import _pair, pooled_map

_KIND = {"avg": _lib.POOL_AVG, "max": _lib.POOL_MAX}


class PoolSpec(tuple):
    """What pool_of states about an admitted module on its map.  The tuple itself is what the kind's ops wrappers take behind the
    tensors -- (k, s), the module's ints, for kind "max" (maxpool_chwn(x, k, s), pool_act_backward_chwn(g, y, k, s, ...)); (kernel,
    stride, padding, count_include_pad), pairs and a bool, for kind "avg" (avgpool_chwn and the avg= of the backward wrappers) -- so a
    walk unpacks it into the launch, and a record compares (and hashes) as those arguments alone.  kind: "max" | "avg"; out: the
    output map (ho, wo).  Immutable; copies and pickles like any value."""

    def __new__(cls, kind, args, out):
        self = super().__new__(cls, args)
        self.__dict__.update(kind=kind, out=tuple(out))
        return self

    def __setattr__(self, name, value):
        raise AttributeError("PoolSpec is immutable")

    def __reduce__(self):
        return (PoolSpec, (self.kind, tuple(self), self.out))


def pool_desc(H, W, B, kernel, stride, padding, count_include_pad, kind="avg"):
    d = _lib.PoolDesc()
    d.kind, d.h, d.w, d.batch = _KIND[kind], int(H), int(W), int(B)
    (d.kh, d.kw), (d.stride_h, d.stride_w), (d.pad_h, d.pad_w) = _pair(kernel), _pair(stride), _pair(padding)
    d.count_include_pad = 1 if count_include_pad else 0
    return d


def pool_plan(kind, H, W, B, kernel, stride, padding=0, count_include_pad=False, planes=1, out_plane_pitch=0, bf16=False):
    """(ho, wo, forward workgroups, backward workgroups) of the launches of `kind` ("max" | "avg") on `planes` planes [H, W, B], fp32
    or (bf16: 16-byte groups of 8 images, so B % 8 == 0 and a pitch that is a multiple of 8) bf16 -- the launch entries' own plan
    (bbb_avgpool_plan / bbb_avgpool_bf16_plan answer for both kinds; host only: needs no device).  A geometry the launches refuse
    raises their error."""
    entry = "bbb_avgpool_bf16_plan" if bf16 else "bbb_avgpool_plan"
    d = pool_desc(H, W, B, kernel, stride, padding, count_include_pad, kind)
    ho, wo, fb, bb = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(getattr(_lib.lib(), entry)(ctypes.byref(d), int(planes), int(out_plane_pitch), ctypes.byref(ho), ctypes.byref(wo),
                                     ctypes.byref(fb), ctypes.byref(bb)), entry)
    return ho.value, wo.value, fb.value, bb.value


def avgpool_plan(H, W, B, kernel, stride, padding=0, count_include_pad=True, planes=1, out_plane_pitch=0):
    """pool_plan of the average-pool launches on fp32 planes."""
    return pool_plan("avg", H, W, B, kernel, stride, padding, count_include_pad, planes, out_plane_pitch)


def avgpool_bf16_plan(H, W, B, kernel, stride, padding=0, count_include_pad=True, planes=1, out_plane_pitch=0):
    """pool_plan of the average-pool launches on bf16 planes."""
    return pool_plan("avg", H, W, B, kernel, stride, padding, count_include_pad, planes, out_plane_pitch, bf16=True)


def _int_pair(v):
    """(a, b) for an int or a pair of ints (bools are not sizes), else None."""
    if isinstance(v, int) and not isinstance(v, bool):
        return (v, v)
    if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(a, int) and not isinstance(a, bool) for a in v):
        return (v[0], v[1])
    return None


def is_pool(module):
    """A pooling module of a kind pool_of may admit (whether it does depends on its arguments and, for the average kinds, on the map)."""
    return is_maxpool(module) or is_avgpool(module)


def is_maxpool(module):
    """A max-pooling module of the kind pool_of may admit."""
    return isinstance(module, torch.nn.MaxPool2d)


def is_avgpool(module):
    """An average-pooling module of a kind pool_of may admit."""
    return isinstance(module, (torch.nn.AvgPool2d, torch.nn.AdaptiveAvgPool2d))


def max_args_of(module):
    """(k, s) of an nn.MaxPool2d the paths admit -- an int kernel, an int stride, padding 0, dilation 1, ceil_mode=False -- else None.
    The rule needs no map: the checks that see only a module list (ensemble._chwn_mods_ok) ask it, pool_of states it with the map."""
    k, s = module.kernel_size, module.stride
    if isinstance(k, int) and isinstance(s, int) and module.padding == 0 and module.dilation == 1 and not module.ceil_mode:
        return (k, s)
    return None


def pool_of(module, H, W):
    """THE statement of which pooling modules the batch-innermost paths admit: the PoolSpec of such a module on an H x W map, else None.
    nn.MaxPool2d: an int kernel, an int stride, padding 0, dilation 1, ceil_mode=False -- by its arguments alone, whatever the map (a
    window larger than the map is refused by the launch).  nn.AvgPool2d: int or pair arguments, stride=None meaning the kernel,
    ceil_mode=False, divisor_override=None, and a geometry the launches take (pool_plan.h: 2 * pad <= k, a window within the padded
    map, ...).  nn.AdaptiveAvgPool2d: an output size (an int or a pair of ints) that divides H and W -- it is then the window
    (H / oh, W / ow) at the same stride, no padding."""
    if is_maxpool(module):
        # (the map is conv_desc.pooled_map's, not the plan's: where the window fits they agree -- tests/host/pool_plan_check.cpp holds
        # the two together -- and where it does not the plan refuses, while the walks need the empty map to reach the refusing entry)
        ks = max_args_of(module)
        return None if ks is None else PoolSpec("max", ks, pooled_map(H, W, ks))
    if isinstance(module, torch.nn.AdaptiveAvgPool2d):
        o = _int_pair(module.output_size)
        if o is None or min(o) < 1 or H % o[0] != 0 or W % o[1] != 0:
            return None
        args = ((H // o[0], W // o[1]),) * 2 + ((0, 0), True)
    elif isinstance(module, torch.nn.AvgPool2d):
        k, p = _int_pair(module.kernel_size), _int_pair(module.padding)
        s = k if module.stride is None else _int_pair(module.stride)
        if k is None or s is None or p is None or module.ceil_mode or module.divisor_override is not None:
            return None
        args = (k, s, p, bool(module.count_include_pad))
    else:
        return None
    try:
        out = avgpool_plan(H, W, 4, *args)[:2]
    except _lib.BBBHipError:
        return None
    return PoolSpec("avg", args, out)


def avgpool_of(module, H, W):
    """pool_of for the average modules alone: (kernel, stride, padding, count_include_pad) -- pairs and a bool, what avgpool_chwn and
    the backward wrappers take -- or None (also for a max pool)."""
    return pool_of(module, H, W) if is_avgpool(module) else None
