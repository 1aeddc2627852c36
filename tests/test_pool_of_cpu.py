"""CPU-only check of pool_desc.pool_of, THE statement of which pooling modules the batch-innermost paths admit: over a seeded sweep
of modules x maps it answers as the rules did that it replaced -- the MaxPool2d predicate ensemble._chwn_mods_ok and
fast_train.train_path_ok each wrote out (copied here literally) with the map both computed by hand, and avgpool_of's rules (copied
here, the plan's refusals restated) -- and an admitted module's map is the shape torch's own pooling returns on the CPU.  Then the
source text of the consumers: the rule and the map arithmetic live in pool_desc alone."""
import os
import random
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")


# ---- the rules as they stood, literally ----
def old_max_rule(m, H, W):
    """(reason, None) or (None, map): the predicate of _chwn_mods_ok / train_path_ok and the map output_rows / train_path_ok computed."""
    k, s = m.kernel_size, m.stride
    if not (isinstance(k, int) and isinstance(s, int) and m.padding == 0 and m.dilation == 1 and not m.ceil_mode):
        why = ("max: kernel not an int" if not isinstance(k, int) else "max: stride not an int" if not isinstance(s, int) else
               "max: padding" if m.padding != 0 else "max: dilation" if m.dilation != 1 else "max: ceil_mode")
        return why, None
    return None, ((H - k) // s + 1, (W - k) // s + 1)


def _int_pair(v):
    if isinstance(v, int) and not isinstance(v, bool):
        return (v, v)
    if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(a, int) and not isinstance(a, bool) for a in v):
        return (v[0], v[1])
    return None


def old_avg_rule(m, H, W):
    """avgpool_of's rules; where it asked the launches' plan (avgpool_plan(H, W, 4, *spec)), that plan's refusals restated."""
    if isinstance(m, nn.AdaptiveAvgPool2d):
        o = _int_pair(m.output_size)
        if o is None or min(o) < 1:
            return "adaptive: output size not ints", None
        if H % o[0] != 0 or W % o[1] != 0:
            return "adaptive: output size does not divide the map", None
        k = s = (H // o[0], W // o[1])
        p = (0, 0)
    else:
        k, p = _int_pair(m.kernel_size), _int_pair(m.padding)
        s = k if m.stride is None else _int_pair(m.stride)
        if k is None or s is None or p is None:
            return "avg: an argument that is no int or pair of ints", None
        if m.ceil_mode:
            return "avg: ceil_mode", None
        if m.divisor_override is not None:
            return "avg: divisor_override", None
    if min(k + s) <= 0 or min(p) < 0:
        return "avg: a non-positive size", None
    if 2 * p[0] > k[0] or 2 * p[1] > k[1]:
        return "avg: 2 * pad > k", None
    if k[0] > H + 2 * p[0] or k[1] > W + 2 * p[1]:
        return "avg: window larger than the padded map", None
    return None, ((H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1)


def modules(rng):
    """The seeded module list: about half plain, every refusal reason several times."""
    out = []
    for _ in range(26):                                       # plain max pools: int arguments, stride=None, return_indices
        k = rng.randint(1, 4)
        out.append(nn.MaxPool2d(k, rng.choice([None, 1, 2, 3]), return_indices=rng.random() < 0.2))
    for _ in range(4):
        out.append(nn.MaxPool2d((rng.randint(1, 3),) * 2))                                  # tuple kernel (and so tuple stride)
        out.append(nn.MaxPool2d(rng.randint(2, 3), (rng.randint(1, 2),) * 2))               # tuple stride
        out.append(nn.MaxPool2d(rng.randint(2, 4), rng.randint(1, 2), padding=1))
        out.append(nn.MaxPool2d(rng.randint(2, 3), rng.randint(1, 2), padding=(0, 0)))      # (a pair of zeros is not 0 to the rule)
        out.append(nn.MaxPool2d(rng.randint(1, 3), rng.randint(1, 2), dilation=2))
        out.append(nn.MaxPool2d(rng.randint(1, 3), rng.randint(1, 2), ceil_mode=True))
    for _ in range(22):                                       # plain average pools: ints and pairs, stride=None, both divisor rules
        k = rng.choice([rng.randint(1, 4), (rng.randint(1, 4), rng.randint(1, 4))])
        s = rng.choice([None, rng.randint(1, 3), (rng.randint(1, 3), rng.randint(1, 3))])
        kmin = k if isinstance(k, int) else min(k)
        out.append(nn.AvgPool2d(k, s, padding=rng.randint(0, kmin // 2), count_include_pad=rng.random() < 0.5))
    for _ in range(3):
        out.append(nn.AvgPool2d(rng.randint(1, 3), ceil_mode=True))
        out.append(nn.AvgPool2d(rng.randint(1, 3), divisor_override=rng.randint(1, 4)))
        out.append(nn.AvgPool2d(float(rng.randint(1, 3))))
        out.append(nn.AvgPool2d(rng.randint(1, 3), rng.randint(1, 2), padding=2))           # 2 * pad > k
        out.append(nn.AdaptiveAvgPool2d((None, rng.randint(1, 2))))
    out.append(nn.AvgPool2d(0, 1))                                                          # a window of no size: it constructs
    for o in (1, 2, 3, (1, 2), (3, 1), (2, 4), 4, (1, 1)):
        out.append(nn.AdaptiveAvgPool2d(o))
    return out


def torch_map(m, H, W):
    """The map torch's own pooling returns for the module on a CPU tensor, or None where torch refuses the geometry."""
    x = torch.zeros(1, 1, H, W)
    try:
        if isinstance(m, nn.MaxPool2d):
            y = F.max_pool2d(x, m.kernel_size, m.stride, m.padding, m.dilation, m.ceil_mode)
        else:
            y = m(x)
    except RuntimeError:
        return None
    return tuple(y.shape[2:])


def test_pool_of_answers_as_the_rules_it_replaced():
    from bbb_hip import pool_desc
    rng = random.Random(20261019)
    mods = modules(rng)
    admitted, reasons, n, small = 0, {}, 0, 0
    for m in mods:
        for H in range(1, 10):
            for W in range(1, 10):
                n += 1
                why, want = old_max_rule(m, H, W) if isinstance(m, nn.MaxPool2d) else old_avg_rule(m, H, W)
                spec = pool_desc.pool_of(m, H, W)
                assert pool_desc.is_pool(m)
                if why is not None:
                    reasons[why] = reasons.get(why, 0) + 1
                    assert spec is None, (m, H, W, why)
                    continue
                admitted += 1
                assert spec is not None and tuple(spec.out) == want, (m, H, W, spec, want)
                assert spec.kind == ("max" if isinstance(m, nn.MaxPool2d) else "avg")
                got = torch_map(m, H, W)
                if min(want) >= 1:
                    assert got == want, (m, H, W, got, want)
                else:                                          # a max pool on a map smaller than its window: admitted by its
                    small += 1                                 # arguments (the launch refuses it), and torch refuses it too
                    assert isinstance(m, nn.MaxPool2d) and got is None, (m, H, W, got)
                if spec.kind == "max":
                    assert tuple(spec) == (m.kernel_size, m.stride) and spec == pool_desc.max_args_of(m)
                else:
                    assert spec == pool_desc.avgpool_of(m, H, W) and len(spec) == 4
                    assert pool_desc.avgpool_plan(H, W, 4, *spec)[:2] == want
                if spec.kind == "max" and min(want) >= 1:       # where the window fits, the plan states the same map
                    assert pool_desc.pool_plan("max", H, W, 4, *spec)[:2] == want
    print("cases %d admitted %d (maps smaller than a max window: %d) refused %s" % (n, admitted, small, sorted(reasons.items())))
    assert 3 * admitted >= n, (admitted, n)
    assert len(reasons) == 13 and min(reasons.values()) >= 50, reasons
    assert small >= 50
    # the average-only views answer for the average modules alone
    assert pool_desc.avgpool_of(nn.MaxPool2d(2), 8, 8) is None and pool_desc.pool_of(nn.ReLU(), 8, 8) is None
    assert not pool_desc.is_avgpool(nn.MaxPool2d(2)) and pool_desc.is_maxpool(nn.MaxPool2d(2)) and not pool_desc.is_pool(nn.ReLU())


def test_a_max_window_larger_than_the_map_is_refused_by_the_plan_not_by_pool_of():
    from bbb_hip import _lib, pool_desc
    spec = pool_desc.pool_of(nn.MaxPool2d(3, 2), 2, 5)
    assert spec is not None and spec.out == (0, 2)
    with pytest.raises(_lib.BBBHipError):
        pool_desc.pool_plan("max", 2, 5, 4, *spec)
    for bad in (dict(kernel=(3, 2), stride=2), dict(kernel=3, stride=(2, 1)), dict(kernel=3, stride=2, padding=1),
                dict(kernel=3, stride=2, count_include_pad=True)):
        with pytest.raises(_lib.BBBHipError):                  # what the maximum kernels do not implement is no maximum descriptor
            pool_desc.pool_plan("max", 9, 9, 4, **bad)
    assert pool_desc.pool_plan("max", 9, 7, 8, 3, 2, planes=6) == (4, 3, 1, 3)
    assert pool_desc.pool_plan("max", 9, 7, 8, 3, 2, planes=6, bf16=True) == (4, 3, 1, 2)


CONSUMERS = ("bbb_hip/ensemble.py", "bbb_hip/fast_train.py", "bbb_hip/infer_walk.py", "bbb_hip/ops.py", "layers/_fused.py")


@pytest.mark.parametrize("path", CONSUMERS)
def test_the_rule_and_the_map_live_in_pool_desc_alone(path):
    src = open(os.path.join(PKG, path)).read()
    assert not re.search(r"isinstance\([^()]*\bMaxPool2d\b", src), path
    # (n - k) // s + 1 in any spelling of its three names, subscripts and calls included
    name = r"[\w.]+(?:\([^()]*\)|\[[^\[\]]*\])*"
    assert not re.search(r"\(\s*%s\s*-\s*%s\s*\)\s*//\s*%s\s*\+\s*1" % (name, name, name), src), path
    assert "pool_desc" in src or "ops.pool_of" in src, path


def test_a_spec_is_a_value():
    """Compares and hashes as the wrappers' arguments; immutable; survives copy and pickle (tape records and plan steps hold specs)."""
    import copy
    import pickle
    from bbb_hip import pool_desc
    for spec in (pool_desc.pool_of(nn.MaxPool2d(3, 2), 9, 7), pool_desc.pool_of(nn.AvgPool2d((3, 2), 2, (1, 0)), 9, 7)):
        for twin in (copy.copy(spec), copy.deepcopy(spec), pickle.loads(pickle.dumps(spec))):
            assert twin == spec and (twin.kind, twin.out) == (spec.kind, spec.out) and type(twin) is type(spec)
        assert spec == tuple(spec) and hash(spec) == hash(tuple(spec))
        with pytest.raises(AttributeError):
            spec.kind = "other"


def test_a_max_pool_outside_the_rule_fails_the_module_list_check():
    """What sees only the module list (chwn_plan's and _chwn_ok's first gate) refuses such a max pool itself, before any partition."""
    from bbb_hip import ensemble
    assert ensemble._chwn_mods_ok([nn.MaxPool2d(2), nn.MaxPool2d(3, 2), nn.AvgPool2d(2, ceil_mode=True)])    # (average: the map decides)
    for bad in (nn.MaxPool2d(3, 2, 1), nn.MaxPool2d((2, 2)), nn.MaxPool2d(2, dilation=2), nn.MaxPool2d(2, ceil_mode=True)):
        assert not ensemble._chwn_mods_ok([bad])
