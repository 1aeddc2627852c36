"""CPU-only checks of average pooling in the bf16 storage mode (LaunchConfig.bf16_avgpool, csrc/pool2d_bf16.hip): the C ABI (three
entries, additive to ABI 13), the switch, the launches' plan (csrc/pool_plan.h plan_bf16 through bbb_avgpool_bf16_plan =
ops.avgpool_bf16_plan) against an independent restatement over a seeded sweep and on hand-worked refusals with the launch entries'
own codes, the inference plan and the precision check with and without the switch, the LRT rule, the training gate, and a
host-only walk of the plan header (both group widths side by side) under the sanitizers.  A refusal comes back before any launch:
none of this needs a device."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_avgpool_cpu import EALIGN, EINVAL, ESHAPE, HEADER, PKG, PTR, ROOT, _desc, _gap_net

ENTRIES = ("bbb_avgpool_bf16_plan", "bbb_avgpool_chwn_bf16", "bbb_avgpool_act_bwd_chwn_bf16")
X_SHAPE = (8, 3, 12, 10)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def _gap(kind):
    """conv 8 -> Softplus -> AvgPool2d(2) -> conv 16 -> Softplus -> AdaptiveAvgPool2d(1) -> Flatten -> linear 10."""
    return _gap_net(kind, mid=8, c2=16)


# ---- 1. the C ABI and the switch ----
def test_entries_are_exported_declared_and_bound(lib):
    h = lib.lib()
    assert h.bbb_abi_version() == 13 and lib.ABI_VERSION == 13
    header = open(HEADER).read()
    decl = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(bbb_\w+)\s*\(", header, flags=re.M))
    for name in ENTRIES:
        assert name in lib.EXPORTS and hasattr(h, name) and name in decl, name
    assert h.bbb_avgpool_bf16_plan(None, 1, 0, None, None, None, None) == EINVAL
    from bbb_hip import ops
    for fn in ("avgpool_chwn_bf16", "avgpool_act_backward_chwn_bf16", "avgpool_bf16_plan"):
        assert callable(getattr(ops, fn)), fn


def test_the_switch_is_a_launch_config_field(lib):
    from bbb_hip import ops
    assert "bf16_avgpool" in ops.LaunchConfig.FIELDS
    c = ops.LaunchConfig()
    assert c.bf16_avgpool is False and ops.current_config().bf16_avgpool is False
    on = c.copy(bf16_avgpool=True)
    assert on.bf16_avgpool is True and on.key() != c.key() and on.copy().key() == on.key()
    assert "bf16_avgpool=True" in repr(on) and "bf16_avgpool" in ops.LaunchConfig.__doc__
    with ops.use_config(bf16_avgpool=True):
        assert ops.current_config().bf16_avgpool is True and ops.current_config().bf16_lrt is False
    assert ops.current_config().bf16_avgpool is False


# ---- 2. the plan against an independent restatement ----
def restated_plan(h, w, B, kh, kw, sh, sw, ph, pw, cip, planes=1, pitch=0, kind=1):
    """What the launches on bf16 planes do, restated from torch's documentation of AvgPool2d (floor mode) and the kernels' thread
    layout (one thread per 8 images): the refusal code, or (ho, wo, forward workgroups, backward workgroups)."""
    if kind != 1 or min(planes, h, w, B, kh, kw, sh, sw) <= 0 or min(ph, pw) < 0 or cip not in (0, 1):
        return EINVAL
    if B % 8 or 2 * ph > kh or 2 * pw > kw or kh > h + 2 * ph or kw > w + 2 * pw:
        return ESHAPE
    if max(h + 2 * ph + kh, w + 2 * pw + kw) > 2 ** 31 - 1:
        return ESHAPE
    ho, wo = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    fwd, bwd = -(-planes * ho * wo * (B // 8) // 256), -(-planes * h * w * (B // 8) // 256)
    if max(fwd, bwd) > 2 ** 31 - 1:
        return ESHAPE
    if pitch != 0 and (pitch < h * w * B or pitch % 8):
        return EINVAL
    return ho, wo, fwd, bwd


def _entry_codes(lib, d, planes, pitch):
    """What each launch entry returns with dummy aligned pointers.  Only ever asked for what the plan refuses, so nothing is
    launched: the forward, which has no output pitch, is not asked about a pitch (it would take the descriptor)."""
    h, r = lib.lib(), ctypes.byref(d)
    assert h.bbb_avgpool_bf16_plan(r, planes, pitch, None, None, None, None) != 0
    return (h.bbb_avgpool_chwn_bf16(r, PTR, PTR, planes, None) if pitch == 0 else None,
            h.bbb_avgpool_act_bwd_chwn_bf16(r, PTR, PTR, PTR, planes, 0, pitch, 0, None))


def test_plan_matches_the_restatement_over_a_sweep(lib):
    from bbb_hip import ops
    rng = random.Random(20261020)
    n_ok = n_bad = n_b = 0
    for _ in range(400):
        h, w, B = rng.randint(1, 40), rng.randint(1, 40), 8 * rng.randint(1, 32)
        kh = rng.randint(1, 7)
        kw = kh if rng.random() < 0.6 else rng.randint(1, 7)
        sh = rng.randint(1, 5)
        sw = sh if rng.random() < 0.6 else rng.randint(1, 5)
        ph, pw = rng.randint(0, kh // 2 + (rng.random() < 0.1)), rng.randint(0, kw // 2 + (rng.random() < 0.1))
        cip, planes = rng.random() < 0.5, rng.randint(1, 3000)
        if rng.random() < 0.08:
            B += rng.choice((1, 2, 3, 4, 5, 6, 7, 4, 4))             # (a multiple of 4 that is no multiple of 8 among them)
        pitch = 0
        if rng.random() < 0.3:
            pitch = h * w * B + rng.choice((0, 8, 64, 4, 12, -8))
        want = restated_plan(h, w, B, kh, kw, sh, sw, ph, pw, int(cip), planes, pitch)
        if isinstance(want, tuple):
            assert ops.avgpool_bf16_plan(h, w, B, (kh, kw), (sh, sw), (ph, pw), cip, planes=planes, out_plane_pitch=pitch) == want
            # the 4-wide plan of the same descriptor: the same map, twice the threads
            ho, wo, f4, b4 = ops.avgpool_plan(h, w, B, (kh, kw), (sh, sw), (ph, pw), cip, planes=planes, out_plane_pitch=pitch)
            assert (ho, wo) == want[:2] and f4 == -(-planes * ho * wo * (B // 4) // 256)
            x = torch.zeros(1, 1, h, w)
            assert tuple(F.avg_pool2d(x, (kh, kw), (sh, sw), (ph, pw), count_include_pad=cip).shape[2:]) == want[:2]
            n_ok += 1
        else:
            with pytest.raises(lib.BBBHipError):
                ops.avgpool_bf16_plan(h, w, B, (kh, kw), (sh, sw), (ph, pw), cip, planes=planes, out_plane_pitch=pitch)
            d = _desc(lib, h, w, B, kh, kw, sh, sw, ph, pw, int(cip))
            assert lib.lib().bbb_avgpool_bf16_plan(ctypes.byref(d), planes, pitch, None, None, None, None) == want
            fwd, bwd = _entry_codes(lib, d, planes, pitch)
            assert bwd == want and fwd == (want if pitch == 0 else None)
            n_bad += 1
            n_b += B % 8 != 0
    assert n_ok > 200 and n_bad > 40 and n_b > 10, (n_ok, n_bad, n_b)


def test_every_refusal_by_its_code(lib):
    h = lib.lib()
    d = _desc(lib, 9, 7, 8, 3, 3, 2, 2, 1, 1, 1)
    r = ctypes.byref(d)
    ho, wo, fb, bb = (ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0))
    assert h.bbb_avgpool_bf16_plan(r, 6, 0, ctypes.byref(ho), ctypes.byref(wo), ctypes.byref(fb), ctypes.byref(bb)) == 0
    assert (ho.value, wo.value, fb.value, bb.value) == (5, 4, 1, 2)            # 6 * 5 * 4 * 1 = 120 and 6 * 9 * 7 * 1 = 378 threads

    def codes(dd, planes=6, pitch=0):
        rr = ctypes.byref(dd)
        rc = h.bbb_avgpool_bf16_plan(rr, planes, pitch, None, None, None, None)
        assert rc != 0
        fwd, bwd = _entry_codes(lib, dd, planes, pitch)
        assert bwd == rc and fwd in (rc, None)
        return rc

    # B = 12: a multiple of 4 (the fp32 plan takes it) that is no multiple of 8
    d12 = _desc(lib, 9, 7, 12, 3, 3, 2, 2, 1, 1, 1)
    assert codes(d12) == ESHAPE and h.bbb_avgpool_plan(ctypes.byref(d12), 6, 0, None, None, None, None) == 0
    # an output pitch of 12: below a plane (504), and no multiple of 8; 508: above a plane, a multiple of 4 only; 512 is taken
    assert codes(d, pitch=12) == EINVAL and codes(d, pitch=508) == EINVAL and codes(d, pitch=496) == EINVAL
    assert h.bbb_avgpool_bf16_plan(r, 6, 512, None, None, None, None) == 0 and h.bbb_avgpool_bf16_plan(r, 6, 504, None, None, None, None) == 0
    assert h.bbb_avgpool_plan(r, 6, 508, None, None, None, None) == 0
    # 2 * pad > k on an axis
    assert codes(_desc(lib, 9, 7, 8, 3, 3, 2, 2, 2, 1, 1)) == ESHAPE and codes(_desc(lib, 9, 7, 8, 3, 1, 2, 2, 1, 1, 1)) == ESHAPE
    # a null descriptor, null pointers
    assert h.bbb_avgpool_bf16_plan(None, 6, 0, None, None, None, None) == EINVAL
    assert h.bbb_avgpool_chwn_bf16(None, PTR, PTR, 6, None) == EINVAL
    assert h.bbb_avgpool_act_bwd_chwn_bf16(None, PTR, PTR, PTR, 6, 0, 0, 0, None) == EINVAL
    assert h.bbb_avgpool_chwn_bf16(r, None, PTR, 6, None) == EINVAL and h.bbb_avgpool_chwn_bf16(r, PTR, None, 6, None) == EINVAL
    for args in ((None, PTR, PTR), (PTR, None, PTR), (PTR, PTR, None)):
        assert h.bbb_avgpool_act_bwd_chwn_bf16(r, *args, 6, 0, 0, 0, None) == EINVAL
    # null pointers come before the plan, the plan before the alignment, the alignment before act and the flags
    assert h.bbb_avgpool_chwn_bf16(ctypes.byref(d12), None, PTR, 6, None) == EINVAL
    assert h.bbb_avgpool_chwn_bf16(ctypes.byref(d12), PTR + 8, PTR, 6, None) == ESHAPE
    assert h.bbb_avgpool_chwn_bf16(r, PTR + 8, PTR, 6, None) == EALIGN and h.bbb_avgpool_chwn_bf16(r, PTR, PTR + 2, 6, None) == EALIGN
    for args in ((PTR + 8, PTR, PTR), (PTR, PTR + 4, PTR), (PTR, PTR, PTR + 2)):
        assert h.bbb_avgpool_act_bwd_chwn_bf16(r, *args, 6, 0, 0, 0, None) == EALIGN
        assert h.bbb_avgpool_act_bwd_chwn_bf16(r, *args, 6, 3, 0, 4, None) == EALIGN
        assert h.bbb_avgpool_act_bwd_chwn_bf16(ctypes.byref(d12), *args, 6, 3, 0, 4, None) == ESHAPE
    # an unknown activation, an unknown flag bit (1 = fp32 g_out and 2 = fp32 output are the known ones)
    assert h.bbb_avgpool_act_bwd_chwn_bf16(r, PTR, PTR, PTR, 6, 3, 0, 0, None) == EINVAL
    assert h.bbb_avgpool_act_bwd_chwn_bf16(r, PTR, PTR, PTR, 6, -1, 0, 0, None) == EINVAL
    for flags in (4, 8, 1 << 31, 7):
        assert h.bbb_avgpool_act_bwd_chwn_bf16(r, PTR, PTR, PTR, 6, 0, 0, flags, None) == EINVAL


# ---- 3. the inference plan and the precision check, with and without the switch ----
def test_plan_and_precision_check_follow_the_switch(lib):
    from bbb_hip import ensemble, ops
    net = _gap("bbb")
    x = torch.zeros(X_SHAPE)
    with torch.no_grad():
        assert ensemble.chwn_plan(net, X_SHAPE, 2, precision="bf16") is None
        for dropin in (False, True):
            with pytest.raises(lib.BBBHipError, match="average pooling") as ei:
                ensemble._check_precision("bf16", net, x, True, dropin=dropin)
            assert "bf16_avgpool" in str(ei.value) and "use_config(bf16_avgpool=True)" in str(ei.value)
        fp32_steps = ensemble.chwn_plan(net, X_SHAPE, 2)
        with ops.use_config(bf16_avgpool=True):
            steps = ensemble.chwn_plan(net, X_SHAPE, 2, precision="bf16")
            assert steps is not None
            avg = [s for s in steps if s.form == "avgpool"]
            assert [s.mod for s in avg] == [net.pool0, net.head]
            assert [s.pool for s in avg] == [((2, 2), (2, 2), (0, 0), True), ((6, 5), (6, 5), (0, 0), True)]
            assert [s.out_shape for s in avg] == [(8, 6, 5, 8), (16, 1, 1, 8)]
            for s in avg:
                assert s.in_layout == s.layout == "bf16" and s.n_mods == 1
            assert sum(s.n_mods for s in steps) == len(ensemble.flat_children(net))
            assert [s.form for s in steps] == ["bf16_bbb", "avgpool", "bf16_bbb", "avgpool", "flatten", "bf16_bbb"]
            assert steps[-1].out_shape == (10, 1, 1, 8) and steps[-1].layout == "f32"
            ensemble._check_precision("bf16", net, x, True)
            ensemble._check_precision("bf16", net, x, True, dropin=True)
            # the remaining bf16 checks decide: the batch-innermost path (B % 4 here; B % 8 is the walk's own refusal) ...
            with pytest.raises(lib.BBBHipError, match="batch-innermost"):
                ensemble._check_precision("bf16", net, torch.zeros(6, 3, 12, 10), True)
            with pytest.raises(lib.BBBHipError, match="batch-innermost"):
                ensemble._check_precision("bf16", net, x, False)
            # ... and an average pool the paths do not admit on its map is no plan, as in fp32
            odd = _gap_net("bbb", c2=16, head=nn.AdaptiveAvgPool2d((4, 5)))
            assert ensemble.chwn_plan(odd, X_SHAPE, 2, precision="bf16") is None
            # B = 12: the 8-wide plan refuses the map rule's question -> no plan
            assert ensemble.chwn_plan(net, (12, 3, 12, 10), 2, precision="bf16") is None
            # an average pool in front of everything pools the bf16 input planes
            lead = ensemble.chwn_plan(_gap_net("bbb", c2=16, lead=nn.AvgPool2d(1)), X_SHAPE, 2, precision="bf16")
            assert lead[0].form == "avgpool" and lead[0].in_layout == lead[0].layout == "bf16" and lead[0].out_shape == (3, 12, 10, 8)
            # the fp32 plan does not depend on the switch
            again = ensemble.chwn_plan(net, X_SHAPE, 2)
            assert [(s.form, s.in_layout, s.layout, s.out_shape, s.pool) for s in again] == \
                [(s.form, s.in_layout, s.layout, s.out_shape, s.pool) for s in fp32_steps]
        assert ensemble.chwn_plan(net, X_SHAPE, 2, precision="bf16") is None       # and off again behind the context


def test_lrt_models_need_both_switches(lib):
    from bbb_hip import ensemble, ops
    net = _gap("lrt")
    x = torch.zeros(X_SHAPE)
    with torch.no_grad():
        with ops.use_config(bf16_lrt=True):
            with pytest.raises(lib.BBBHipError, match="bf16_avgpool"):
                ensemble._check_precision("bf16", net, x, True)
            assert ensemble.chwn_plan(net, X_SHAPE, 2, precision="bf16") is None
        with ops.use_config(bf16_avgpool=True):
            with pytest.raises(lib.BBBHipError, match="bf16_lrt"):                # the existing LRT hint
                ensemble._check_precision("bf16", net, x, True, dropin=True)
            assert ensemble._BF16_LRT_HINT.startswith("LRT models run in bf16 only under LaunchConfig.bf16_lrt")
        with ops.use_config(bf16_avgpool=True, bf16_lrt=True):
            ensemble._check_precision("bf16", net, x, True)
            steps = ensemble.chwn_plan(net, X_SHAPE, 2, precision="bf16")
            assert [s.form for s in steps] == ["bf16_lrt", "avgpool", "bf16_lrt", "avgpool", "flatten", "bf16_lrt"]
            assert all(s.in_layout == s.layout == "bf16" for s in steps if s.form == "avgpool")


# ---- 4. the training gate ----
def test_training_gate_follows_the_switch(lib, monkeypatch):
    from bbb_hip import fast_train, ops
    net = _gap("bbb")
    x = torch.zeros(X_SHAPE)
    # (no device here: stand in for the checks that need one; the reason under test comes from the model alone)
    monkeypatch.setattr(fast_train, "train_path_ok", lambda n, t: fast_train._train_path_static(n, t))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    why = fast_train.bf16_train_refusal(net, x)
    assert why is not None and "average pooling" in why and "bf16_avgpool" in why
    with ops.use_config(bf16_avgpool=True):
        assert fast_train.bf16_train_refusal(net, x) is None
        why = fast_train.bf16_train_refusal(net, torch.zeros(12, 3, 12, 10))
        assert why is not None and "multiple of 8" in why
        why = fast_train.bf16_train_refusal(_gap("lrt"), x)
        assert why is not None and "local-reparameterisation" in why
        # an average pool the training path does not pair with a layer stays off it
        assert fast_train.bf16_train_refusal(_gap_net("bbb", lead=nn.AvgPool2d(1)), x) is not None
    assert fast_train.bf16_train_refusal(net, x) is not None


# ---- 5. the contract helper: without roundings it is the exact gradient ----
def test_contract_helper_without_rounding_is_autograd():
    import bf16_avgpool_contract as A
    gen = np.random.default_rng(3)
    plan = [dict(name="c0", kind="conv", stride=2, padding=2, act="relu", pool=((3, 3), (2, 2), (1, 1), False)),
            dict(name="c1", kind="conv", padding=1, act="softplus", pool=((2, 1), (2, 1), (0, 0), True)),
            dict(name="c2", kind="conv", padding=1, act="softplus", pool=(2, 1), flat=8 * 1 * 2),
            dict(name="f0", kind="fc", act="relu"), dict(name="f1", kind="fc")]
    shapes = {"c0": (6, 3, 5, 5), "c1": (8, 6, 3, 3), "c2": (8, 8, 3, 3), "f0": (12, 16), "f1": (10, 12)}
    params = {"_prior_mu": 0.0, "_prior_sigma": 0.1}
    for n, s in shapes.items():
        fan = int(np.prod(s[1:]))
        params[n] = dict(W_mu=(gen.standard_normal(s) / np.sqrt(fan)).astype(np.float32), W_rho=np.full(s, -4.0, np.float32),
                         bias_mu=(0.1 * gen.standard_normal(s[0])).astype(np.float32), bias_rho=np.full(s[0], -4.0, np.float32))
    x = gen.random((4, 3, 13, 11)).astype(np.float32)
    t = gen.integers(0, 10, 4)
    eps = [{n: dict(W=gen.standard_normal(s), bias=gen.standard_normal(s[0])) for n, s in shapes.items()} for _ in range(2)]
    # the map: 13 x 11 -> 7 x 6 -> (3, 2, 1) 4 x 3 -> conv 4 x 3 -> (2, 1) 2 x 3 -> conv 2 x 3 -> max(2, 1) 1 x 2: 8 * 1 * 2 features
    loss, lo, got = A.step_grads(plan, params, x, t, eps, 0.1, 100.0, rounding=False)
    loss_a, want = A.autograd_grads(plan, params, x, t, eps, 0.1, 100.0)
    assert abs(loss - loss_a) <= 1e-9 * abs(loss_a)
    for n in shapes:
        for k in ("W_mu", "W_rho", "bias_mu", "bias_rho"):
            w = want[n][k]
            assert np.abs(np.asarray(got[n][k]).reshape(w.shape) - w).max() <= 1e-10 * (np.abs(w).max() + 1e-30), (n, k)
    # ... and with them it is a perturbation of it: the roundings are on (the gradients differ) and small
    _, _, rnd = A.step_grads(plan, params, x, t, eps, 0.1, 100.0)
    w = want["c0"]["W_mu"]
    d = np.abs(np.asarray(rnd["c0"]["W_mu"]).reshape(w.shape) - w).max() / np.abs(w).max()
    assert 0 < d < 0.1, d


# ---- 6. the plan header alone, both widths, under the sanitizers ----
def test_pool_plan_bf16_walk_under_the_sanitizers(tmp_path):
    """tests/host/pool_plan_bf16_check.cpp (the plan header alone, no device code, not loaded into Python) under
    -fsanitize=address,undefined: plan_bf16 and plan side by side over ordinary geometries with every refusal mixed in and over
    descriptors at the integer limits."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "pool_plan_bf16_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "pool_plan_bf16_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[:14:2], out[1:14:2]))
    assert out[14] == "checksum" and len(out[15]) == 16
    assert int(got["cases"]) >= 120000 and min(int(got[k]) for k in ("ok", "einval", "eshape")) > 10000 and int(got["ealign"]) == 0
    assert int(got["both"]) > 10000 and int(got["only4"]) > 1000
