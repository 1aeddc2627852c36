"""CPU-only checks of average pooling on the batch-innermost paths: the C ABI (four entries, bbb_pool_desc_t), the launches' plan
(csrc/pool_plan.h through bbb_avgpool_plan = ops.avgpool_plan) against an independent restatement over a seeded sweep and on
hand-worked refusals with the launch entries' own codes, what ops.avgpool_of admits, the inference plan (ensemble.chwn_plan) and
the training gate (fast_train._train_path_static) of models with nn.AvgPool2d / nn.AdaptiveAvgPool2d, the bf16 refusals by name,
and a host-only walk of the plan header under the sanitizers.  A refusal comes back before any launch: none of this needs a device."""
import ctypes
import os
import random
import re
import shutil
import subprocess
import tempfile

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ref_port_torch as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")
HEADER = os.path.join(ROOT, "include", "bbb_hip.h")
EINVAL, EALIGN, ESHAPE = -1, -2, -3
PTR = 64          # a dummy operand pointer: non-null, 16-byte aligned, never dereferenced (every call below is refused before a launch)
ENTRIES = ("bbb_avgpool_chwn", "bbb_avgpool_act_bwd_chwn", "bbb_lrt_avgpool_act_bwd_chwn", "bbb_avgpool_plan")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


# ---- 1. the C ABI ----
def test_entries_are_exported_declared_and_bound(lib):
    h = lib.lib()
    assert h.bbb_abi_version() == 13 and lib.ABI_VERSION == 13
    header = open(HEADER).read()
    decl = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(bbb_\w+)\s*\(", header, flags=re.M))
    for name in ENTRIES:
        assert name in lib.EXPORTS and hasattr(h, name) and name in decl, name
    assert re.search(r"^#define BBB_POOL_AVG 1\b", header, flags=re.M) and lib.POOL_AVG == 1
    assert re.search(r"^#define BBB_POOL_MAX 2\b", header, flags=re.M) and lib.POOL_MAX == 2
    assert h.bbb_avgpool_plan(None, 1, 0, None, None, None, None) == EINVAL


def test_pool_desc_layout_matches_the_header(lib):
    fields = [n for n, _ in lib.PoolDesc._fields_]
    assert fields == ["kind", "h", "w", "batch", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w", "count_include_pad"]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"bbb_hip.h\"\nint main(void) {\n  printf(\"%zu\", sizeof(bbb_pool_desc_t));\n" + \
        "".join("  printf(\" %%zu\", offsetof(bbb_pool_desc_t, %s));\n" % f for f in fields) + "  return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    D = lib.PoolDesc
    assert got == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]


# ---- 2. the plan against an independent restatement ----
def restated_plan(h, w, B, kh, kw, sh, sw, ph, pw, cip, planes=1, pitch=0, kind=1):
    """What the launches do, restated from torch's documentation of AvgPool2d (floor mode) and the kernels' thread layout: the
    refusal code, or (ho, wo, forward workgroups, backward workgroups)."""
    if kind != 1 or min(planes, h, w, B, kh, kw, sh, sw) <= 0 or min(ph, pw) < 0 or cip not in (0, 1):
        return EINVAL
    if B % 4 or 2 * ph > kh or 2 * pw > kw or kh > h + 2 * ph or kw > w + 2 * pw:
        return ESHAPE
    if max(h + 2 * ph + kh, w + 2 * pw + kw) > 2 ** 31 - 1:
        return ESHAPE
    ho, wo = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    fwd, bwd = -(-planes * ho * wo * (B // 4) // 256), -(-planes * h * w * (B // 4) // 256)
    if max(fwd, bwd) > 2 ** 31 - 1:
        return ESHAPE
    if pitch != 0 and (pitch < h * w * B or pitch % 4):
        return EINVAL
    return ho, wo, fwd, bwd


def _desc(lib, h, w, B, kh, kw, sh, sw, ph, pw, cip, kind=1):
    d = lib.PoolDesc()
    d.kind, d.h, d.w, d.batch, d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.count_include_pad = kind, h, w, B, kh, kw, sh, sw, ph, pw, cip
    return d


def _entry_codes(lib, d, planes, pitch):
    """What each launch entry returns with dummy aligned pointers.  Only ever asked for what the plan refuses, so nothing is
    launched: the forward, which has no output pitch, is not asked about a pitch (it would take the descriptor)."""
    h, r = lib.lib(), ctypes.byref(d)
    assert h.bbb_avgpool_plan(r, planes, pitch, None, None, None, None) != 0
    return (h.bbb_avgpool_chwn(r, PTR, PTR, planes, None) if pitch == 0 else None,
            h.bbb_avgpool_act_bwd_chwn(r, PTR, PTR, PTR, planes, 0, pitch, None),
            h.bbb_lrt_avgpool_act_bwd_chwn(r, PTR, PTR, PTR, PTR, PTR, PTR, planes, planes, 2, pitch, None, None, 0, None))


def test_plan_matches_the_restatement_over_a_sweep(lib):
    from bbb_hip import ops
    rng = random.Random(20261019)
    n_ok = n_bad = 0
    for _ in range(400):
        h, w, B = rng.randint(1, 40), rng.randint(1, 40), 4 * rng.randint(1, 64)
        kh = rng.randint(1, 7)
        kw = kh if rng.random() < 0.6 else rng.randint(1, 7)
        sh = rng.randint(1, 5)
        sw = sh if rng.random() < 0.6 else rng.randint(1, 5)
        ph, pw = rng.randint(0, kh // 2 + (rng.random() < 0.1)), rng.randint(0, kw // 2 + (rng.random() < 0.1))
        cip, planes = rng.random() < 0.5, rng.randint(1, 3000)
        if rng.random() < 0.05:
            B += rng.randint(1, 3)
        want = restated_plan(h, w, B, kh, kw, sh, sw, ph, pw, int(cip), planes)
        if isinstance(want, tuple):
            assert ops.avgpool_plan(h, w, B, (kh, kw), (sh, sw), (ph, pw), cip, planes=planes) == want
            x = torch.zeros(1, 1, h, w)
            assert tuple(F.avg_pool2d(x, (kh, kw), (sh, sw), (ph, pw), count_include_pad=cip).shape[2:]) == want[:2]
            n_ok += 1
        else:
            with pytest.raises(lib.BBBHipError):
                ops.avgpool_plan(h, w, B, (kh, kw), (sh, sw), (ph, pw), cip, planes=planes)
            d = _desc(lib, h, w, B, kh, kw, sh, sw, ph, pw, int(cip))
            assert lib.lib().bbb_avgpool_plan(ctypes.byref(d), planes, 0, None, None, None, None) == want
            assert _entry_codes(lib, d, planes, 0) == (want,) * 3
            n_bad += 1
    assert n_ok > 200 and n_bad > 20, (n_ok, n_bad)


def test_every_refusal_by_its_code(lib):
    h = lib.lib()
    good = dict(h=9, w=7, B=8, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, cip=1)

    def rc(planes=6, pitch=0, kind=1, **kw):
        g = dict(good, **kw)
        d = _desc(lib, g["h"], g["w"], g["B"], g["kh"], g["kw"], g["sh"], g["sw"], g["ph"], g["pw"], g["cip"], kind)
        r = h.bbb_avgpool_plan(ctypes.byref(d), planes, pitch, None, None, None, None)
        assert r == restated_plan(planes=planes, pitch=pitch, kind=kind, **g) if r != 0 else True
        if r != 0:
            fwd, bwd, lrt = _entry_codes(lib, d, planes, pitch)
            assert bwd == r and lrt == r and fwd == (r if pitch == 0 else None), (kw, fwd, bwd, lrt)
        return r

    ho, wo, fb, bb = (ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0))
    d = _desc(lib, 9, 7, 8, 3, 3, 2, 2, 1, 1, 1)
    assert h.bbb_avgpool_plan(ctypes.byref(d), 6, 0, ctypes.byref(ho), ctypes.byref(wo), ctypes.byref(fb), ctypes.byref(bb)) == 0
    assert (ho.value, wo.value, fb.value, bb.value) == (5, 4, 1, 3)          # 6 * 5 * 4 * 2 = 240 and 6 * 9 * 7 * 2 = 756 threads
    assert rc() == 0
    # a null descriptor, null pointers, an unknown kind
    assert h.bbb_avgpool_plan(None, 6, 0, None, None, None, None) == EINVAL
    assert h.bbb_avgpool_chwn(None, PTR, PTR, 6, None) == EINVAL
    r = ctypes.byref(d)
    assert h.bbb_avgpool_chwn(r, None, PTR, 6, None) == EINVAL and h.bbb_avgpool_chwn(r, PTR, None, 6, None) == EINVAL
    assert h.bbb_avgpool_act_bwd_chwn(r, None, PTR, PTR, 6, 0, 0, None) == EINVAL
    assert h.bbb_avgpool_act_bwd_chwn(r, PTR, PTR, None, 6, 0, 0, None) == EINVAL
    assert h.bbb_avgpool_act_bwd_chwn(r, PTR, PTR, PTR, 6, 3, 0, None) == EINVAL                       # an unknown activation
    assert h.bbb_lrt_avgpool_act_bwd_chwn(r, PTR, PTR, None, PTR, PTR, PTR, 6, 6, 0, 0, None, None, 0, None) == EINVAL
    assert h.bbb_lrt_avgpool_act_bwd_chwn(r, PTR, PTR, PTR, PTR, PTR, PTR, 6, 4, 0, 0, None, None, 0, None) == EINVAL      # 6 % 4 planes
    assert rc(kind=0) == EINVAL and rc(kind=2) == EINVAL
    # non-positive sizes, a negative padding, a divisor rule that is neither
    for f in ("h", "w", "B", "kh", "kw", "sh", "sw"):
        assert rc(**{f: 0}) == EINVAL and rc(**{f: -4}) == EINVAL, f
    assert rc(planes=0) == EINVAL and rc(ph=-1) == EINVAL and rc(pw=-1) == EINVAL and rc(cip=2) == EINVAL
    # batch % 4
    assert rc(B=6) == ESHAPE
    # 2 * pad > k on an axis (k = 3: pad 1 is the most)
    assert rc(ph=2) == ESHAPE and rc(pw=2) == ESHAPE and rc(kh=2, ph=1) == 0 and rc(kh=1, ph=1) == ESHAPE
    # a window larger than the padded map (9 + 2: 11 fits, 12 does not)
    assert rc(kh=11) == 0 and rc(kh=12) == ESHAPE and rc(w=1, kw=4, pw=1) == ESHAPE
    # a grid that does not fit an int: planes * 9 * 7 * 2 threads in workgroups of 256
    edge = (2 ** 31 - 1) * 256 // 126
    assert rc(planes=edge) == 0 and rc(planes=edge + 3) == ESHAPE and rc(planes=2 ** 62) == ESHAPE
    assert rc(h=2 ** 31 - 1, w=1, kh=2) == ESHAPE
    # an output pitch that is not a multiple of 4, or below a plane (9 * 7 * 8 = 504)
    assert rc(pitch=504) == 0 and rc(pitch=536) == 0 and rc(pitch=506) == EINVAL and rc(pitch=500) == EINVAL
    # pointers are looked at after the plan: alignment last
    assert h.bbb_avgpool_chwn(r, PTR + 4, PTR, 6, None) == EALIGN
    assert h.bbb_avgpool_act_bwd_chwn(r, PTR, PTR, PTR + 8, 6, 0, 0, None) == EALIGN
    assert h.bbb_lrt_avgpool_act_bwd_chwn(r, PTR, PTR, PTR, PTR + 4, PTR, PTR, 6, 6, 0, 0, None, None, 0, None) == EALIGN
    assert h.bbb_lrt_avgpool_act_bwd_chwn(r, PTR, PTR, PTR, PTR, PTR, PTR, 6, 6, 0, 0, PTR, None, 0, None) == EINVAL       # g_out2 without x_out
    assert h.bbb_lrt_avgpool_act_bwd_chwn(r, PTR, PTR, PTR, PTR, PTR, PTR, 6, 6, 0, 0, PTR, PTR, 4, None) == EINVAL        # 6 % 4 x planes


# ---- 3. what is admitted ----
def test_avgpool_of(lib):
    from bbb_hip.ops import avgpool_of
    assert avgpool_of(nn.AvgPool2d(2), 9, 8) == ((2, 2), (2, 2), (0, 0), True)                                   # stride=None: the kernel
    assert avgpool_of(nn.AvgPool2d(3, 2, 1), 9, 7) == ((3, 3), (2, 2), (1, 1), True)
    assert avgpool_of(nn.AvgPool2d((3, 2), (1, 2), (1, 0), count_include_pad=False), 7, 8) == ((3, 2), (1, 2), (1, 0), False)
    assert avgpool_of(nn.AvgPool2d((2, 1)), 5, 5) == ((2, 1), (2, 1), (0, 0), True)
    assert avgpool_of(nn.AvgPool2d(2, 3), 8, 8) == ((2, 2), (3, 3), (0, 0), True)                                # gaps are fine
    assert avgpool_of(nn.AvgPool2d(2, ceil_mode=True), 9, 8) is None
    assert avgpool_of(nn.AvgPool2d(2, divisor_override=3), 9, 8) is None
    assert avgpool_of(nn.AvgPool2d(3, 2, 2), 9, 8) is None                                                       # 2 * pad > k
    assert avgpool_of(nn.AvgPool2d(5), 4, 8) is None                                                             # a window larger than the map
    assert avgpool_of(nn.AvgPool2d(2.0), 8, 8) is None
    assert avgpool_of(nn.AdaptiveAvgPool2d(1), 7, 6) == ((7, 6), (7, 6), (0, 0), True)
    assert avgpool_of(nn.AdaptiveAvgPool2d((1, 1)), 7, 6) == ((7, 6), (7, 6), (0, 0), True)
    assert avgpool_of(nn.AdaptiveAvgPool2d((3, 2)), 12, 8) == ((4, 4), (4, 4), (0, 0), True)
    assert avgpool_of(nn.AdaptiveAvgPool2d(4), 12, 8) == ((3, 2), (3, 2), (0, 0), True)
    assert avgpool_of(nn.AdaptiveAvgPool2d((5, 2)), 12, 8) is None                                               # 12 % 5
    assert avgpool_of(nn.AdaptiveAvgPool2d((None, 2)), 12, 8) is None
    assert avgpool_of(nn.MaxPool2d(2), 8, 8) is None and avgpool_of(nn.ReLU(), 8, 8) is None


# ---- 4. the inference plan and the training gate ----
def _gap_net(kind, mid=8, c2=12, pool1=None, head=None, lead=None, extra=None, hw=(12, 10)):
    """conv(mid, 3, p1) + Softplus + pool1, conv(c2, 3, p1) + Softplus + head, flatten, fc 10 (defaults: AvgPool2d(2) and a global
    AdaptiveAvgPool2d(1)); lead: a module in front of everything; extra: one more behind pool1."""
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    Conv, Linear = (BBB_Conv2d, BBB_Linear) if kind == "bbb" else (BBB_LRT_Conv2d, BBB_LRT_Linear)
    pool1 = nn.AvgPool2d(2) if pool1 is None else pool1
    head = nn.AdaptiveAvgPool2d(1) if head is None else head
    net = ModuleWrapper()
    if lead is not None:
        net.add_module("lead", lead)
    net.add_module("conv0", Conv(3, mid, 3, padding=1, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("act0", nn.Softplus())
    net.add_module("pool0", pool1)
    if extra is not None:
        net.add_module("extra", extra)
    net.add_module("conv1", Conv(mid, c2, 3, padding=1, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("act1", nn.Softplus())
    net.add_module("head", head)
    x = torch.zeros(1, 1, *hw)                                                 # (the convolutions keep the map)
    for m in ([lead] if lead is not None else []) + [pool1] + ([extra] if extra is not None else []) + [head]:
        x = m(x)
    feat = c2 * x.shape[2] * x.shape[3]
    net.add_module("flatten", FlattenLayer(feat))
    net.add_module("fc", Linear(feat, 10, bias=True, priors=P.CONFIG_PRIORS))
    return net


class _X:
    """What _train_path_static reads of the batch: its shape."""
    shape = (8, 3, 12, 10)


@pytest.mark.parametrize("draws", [1, 2])
@pytest.mark.parametrize("kind", ["bbb", "lrt"])
def test_chwn_plan_walks_average_pools(lib, kind, draws):
    from bbb_hip import ensemble, fast_train
    net = _gap_net(kind)
    steps = ensemble.chwn_plan(net, _X.shape, draws)
    assert steps is not None
    children = ensemble.flat_children(net)
    assert sum(s.n_mods for s in steps) == len(children)                       # every module is walked once
    walked = [s.i for s in steps if s.n_mods]
    assert walked == sorted(set(walked))
    avg = [s for s in steps if s.form == "avgpool"]
    assert [s.mod for s in avg] == [net.pool0, net.head]
    assert [s.pool for s in avg] == [((2, 2), (2, 2), (0, 0), True), ((6, 5), (6, 5), (0, 0), True)]
    for s, ref in zip(avg, (F.avg_pool2d(torch.zeros(8, 8, 12, 10), 2), F.adaptive_avg_pool2d(torch.zeros(8, 12, 6, 5), 1))):
        assert s.out_shape == tuple(ref.shape[1:]) + (8,) and s.in_layout == s.layout == "f32" and s.n_mods == 1
    assert steps[-1].out_shape == (10, 1, 1, 8)
    assert not any(s.pool for s in steps if s.form != "avgpool")               # never fused into a conv launch
    assert ensemble.output_rows(net, _X.shape) == 8
    assert fast_train._train_path_static(net, _X) == kind


@pytest.mark.parametrize("kind", ["bbb", "lrt"])
def test_split_layouts_convert_in_front_of_an_average_pool(lib, kind):
    from bbb_hip import ensemble
    net = _gap_net(kind, mid=16, c2=16)                                        # conv1 and fc read 16 channels: the MFMA-ready-operand chain
    steps = ensemble.chwn_plan(net, _X.shape, 2, precision="bf16x3")
    forms = [s.form for s in steps]
    avg = [j for j, s in enumerate(steps) if s.form == "avgpool"]
    assert len(avg) == 2 and any(s.layout == "c8s3" for s in steps), forms
    split_in = 0
    for j in avg:
        assert steps[j].in_layout == "f32"
        if steps[j - 1].form == "to_f32":
            assert steps[j - 1].in_layout in ("s3", "c8s3") and steps[j - 1].mod is steps[j].mod
            split_in += 1
        else:
            assert steps[j - 1].layout == "f32"
    assert split_in >= 1, forms                                                # conv1 hands its output on split: converted for the head
    # the chain layer behind the first pool gets its conversion as for any fp32 input
    k = forms.index("to_c8s3")
    assert steps[k].mod is net.conv1 and steps[k - 1].form == "avgpool"
    assert sum(s.n_mods for s in steps) == len(ensemble.flat_children(net))


def test_what_the_paths_do_not_take(lib):
    from bbb_hip import ensemble, fast_train
    for kind in ("bbb", "lrt"):
        # an adaptive pool whose output does not divide the map (6 x 5): no plan, off the training path
        net = _gap_net(kind, head=nn.AdaptiveAvgPool2d((4, 5)))
        assert ensemble.chwn_plan(net, _X.shape, 2) is None
        assert fast_train._train_path_static(net, _X) is None
        assert ensemble.chwn_plan(_gap_net(kind, pool1=nn.AvgPool2d(2, ceil_mode=True)), _X.shape, 1) is None
        # inference takes an average pool anywhere; training pairs it with a Bayesian layer
        lead = _gap_net(kind, lead=nn.AvgPool2d(1))
        assert ensemble.chwn_plan(lead, _X.shape, 2) is not None and fast_train._train_path_static(lead, _X) is None
        twice = _gap_net(kind, extra=nn.AvgPool2d(1))
        assert ensemble.chwn_plan(twice, _X.shape, 2) is not None and fast_train._train_path_static(twice, _X) is None
        after_max = _gap_net(kind, pool1=nn.MaxPool2d(2, 2), extra=nn.AvgPool2d(1))
        assert fast_train._train_path_static(after_max, _X) is None
        # a dividing adaptive pool and a padded average pool are on both
        ok = _gap_net(kind, pool1=nn.AvgPool2d(3, 2, 1, count_include_pad=False), head=nn.AdaptiveAvgPool2d((3, 1)))
        assert ensemble.chwn_plan(ok, _X.shape, 2) is not None and fast_train._train_path_static(ok, _X) == kind
        assert ensemble.output_rows(ok, _X.shape) == 8
    # MaxPool2d's rules are what they were
    assert fast_train._train_path_static(_gap_net("bbb", pool1=nn.MaxPool2d(3, 2, 1)), _X) is None


# ---- 5. bf16 storage has no average pooling, and says so ----
def test_bf16_refusals_name_average_pooling(lib, monkeypatch):
    from bbb_hip import ensemble, fast_train
    net = _gap_net("bbb")
    x = torch.zeros(8, 3, 12, 10)
    with pytest.raises(lib.BBBHipError, match="average pooling"):
        ensemble._check_precision("bf16", net, x, True)
    with pytest.raises(lib.BBBHipError, match="average pooling"):
        ensemble._check_precision("bf16", net, x, True, dropin=True)
    ensemble._check_precision("bf16x3", net, x, True)
    assert ensemble.chwn_plan(net, (8, 3, 12, 10), 2, precision="bf16") is None
    # (no device here: stand in for the checks that need one; the reason under test comes from the model alone)
    monkeypatch.setattr(fast_train, "train_path_ok", lambda n, t: fast_train._train_path_static(n, t))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    why = fast_train.bf16_train_refusal(net, x)
    assert why is not None and "average pooling" in why
    assert fast_train.bf16_train_refusal(_gap_net("bbb", pool1=nn.MaxPool2d(2, 2), head=nn.MaxPool2d(5, 5)), x) is None


# ---- 6. the plan header alone under the sanitizers ----
def test_pool_plan_walk_under_the_sanitizers(tmp_path):
    """tests/host/pool_plan_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: ordinary geometries with every refusal mixed in, descriptors at the integer limits; then the
    maximum kind against the program's restatement of the scalar entries' former checks (the same code for any single violation, the
    same map and grids wherever the plan succeeds: the program exits non-zero otherwise) and the maximum descriptors the plan refuses;
    and the dump mode, one line per average-kind descriptor."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "pool_plan_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "pool_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[:10:2], out[1:10:2]))
    assert out[10] == "checksum" and len(out[11]) == 16
    assert int(got["cases"]) >= 120000 and min(int(got[k]) for k in ("ok", "einval", "eshape")) > 10000 and int(got["ealign"]) == 0
    mx = dict(zip(out[12::2], out[13::2]))
    print("pool_plan_check:", " ".join(out))
    assert int(mx["max_cases"]) >= 80000 and min(int(mx[k]) for k in ("max_ok", "max_single", "max_multi")) > 5000, mx
    assert int(mx["max_cases"]) == int(mx["max_ok"]) + int(mx["max_single"]) + int(mx["max_multi"])
    dump = subprocess.run([exe, "dump"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(dump) > 100000 and all(" f32 " in ln and " bf16 " in ln for ln in dump[:50])
