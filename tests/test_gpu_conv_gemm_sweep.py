"""The reference-layout implicit GEMM (csrc/conv_gemm.hip, conv_gemm_kernel<BM, LRT, LINEAR>) and everything that runs on it,
against float64: bbb_conv2d_fwd and bbb_lrt_conv2d_fwd through ctypes on every case of conv_gemm_contract.CASES, each in two tiers;
every refusal on the device build; the backward helpers of bbb_hip.ops (conv2d_input_grad, conv2d_weight_grad, conv2d_splitk) and
ops.conv2d(...).backward(); ops.lrt_conv2d forward on both sides of ops._small_launch, and its backward.

  exact    dyadic operands, every partial sum of either contraction an fp32 number in any summation order: y, act_mu and
           act_var - float32(1e-16) of the case's launch without noise and without softplus (conv_gemm_contract.quiet) EQUAL the
           reference.  One dropped, duplicated or mis-addressed tap fails this.
  rounded  Gaussian operands, the case as it is; every element inside the per-element bounds of conv_gemm_contract's docstring.

Every output of a launch lies between two guard bands of a NaN pattern that must come back untouched, and starts as that pattern,
so an element the kernel never stored fails both tiers.  Which instantiation a case runs is the library's answer
(bbb_conv2d_fwd_plan, the launch entries' own plan), asserted per case; tests/test_conv_gemm_sweep_cpu.py holds the table's coverage
of the eight instantiations and of every edge.  Measured figures: profiles/conv_gemm_sweep_notes.md."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

import conv_gemm_contract as C

pytestmark = pytest.mark.gpu
F64 = np.float64


@pytest.fixture(scope="module")
def lib():
    from bbb_hip import _lib
    _lib.lib()
    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", list(C.CASES))
def test_instantiation_by_instantiation_against_float64(lib, name):
    c = C.CASES[name]
    plan = C.plan_query(lib, c.desc, c.lrt)
    assert "%s-%d%s" % ("lrt" if c.lrt else "bbb", plan["bm"], "-lin" if plan["linear"] else "") == c.form, (name, plan)
    # exact tier
    q = C.quiet(c)
    o = C.operands(q, "exact")
    n = C.check_exact(q, C.launch(lib, torch, q, o), C.reference(q, o))
    assert n == c.E * c.M * c.Cout * (3 if c.lrt else 1)
    # rounded tier
    o = C.operands(c, "rounded")
    worst = C.check_rounded(c, C.launch(lib, torch, c, o), C.reference(c, o))
    print("\nworst error / bound  %-12s %-18s %s  exact: %d elements equal" % (c.form, name, "  ".join("%s %.3f" % kv for kv in worst.items()), n))


def test_every_refusal_on_the_device_build_leaves_the_output_unwritten(lib):
    """Each refusal of conv_gemm_contract.refusals() asked of the launch entries with real device operands: the code, and not one
    element of y, act_mu or act_var written (nor anything around them)."""
    c = C.Case("good", "lrt-64", C.GOOD["B"], C.GOOD["Cin"], C.GOOD["H"], C.GOOD["W"], C.GOOD["Cout"], (2, 3), (2, 1), (1, 0), (1, 2), E=2, ext_eps=True)
    o = C.operands(c, "rounded")
    n = c.E * c.M * c.Cout
    t = {k: dev(o[k]) for k in ("x", "w", "w_var", "b", "b_var", "eps")}
    outs = {k: C.Guarded(torch, n) for k in ("y", "act_mu", "act_var")}
    lrt_ptrs = dict(x=t["x"].data_ptr(), w_mu=t["w"].data_ptr(), w_var=t["w_var"].data_ptr(), b_mu=t["b"].data_ptr(), b_var=t["b_var"].data_ptr(),
                    eps=t["eps"].data_ptr(), **{k: g.ptr for k, g in outs.items()})
    bbb_ptrs = dict(x=lrt_ptrs["x"], w=lrt_ptrs["w_mu"], bias=lrt_ptrs["b_mu"], y=lrt_ptrs["y"])
    seen = set()
    for name, dchange, pchange, lrt_only in C.refusals():
        for lrt in ((True,) if lrt_only else (False, True)):
            base = lrt_ptrs if lrt else bbb_ptrs
            if any(k not in base for k in pchange):
                continue
            desc, ptrs = dict(c.desc, **dchange), C.with_operands(base, pchange)
            want = C.plan_rules(desc, lrt, ptrs)
            assert want in (C.EINVAL, C.EALIGN, C.ESHAPE), (name, lrt)
            assert C.entry_refusal(lib, desc, lrt, ptrs) == want, (name, lrt)
            seen.add((want, lrt))
    torch.cuda.synchronize()
    assert seen == {(code, l) for code in (C.EINVAL, C.EALIGN, C.ESHAPE) for l in (False, True)}
    assert all(g.unwritten() for g in outs.values())


# ------------------------------------------------------------------------------------------------ the backward helpers
# B, Cin, H, W, Cout, k, s, p, d, E, weights shared by the draws, x shared by the draws -- the contraction of either gradient stays
# <= 320 long (dgrad: Cout kh kw [x E when x is shared]; wgrad: B Ho Wo [x E when the weights are shared])
BWD_CASES = {
    "s1": (4, 3, 7, 6, 5, (3, 3), (1, 1), (1, 1), (1, 1), 2, False, False),
    "s2-ragged": (8, 3, 8, 8, 5, (3, 3), (2, 2), (0, 0), (1, 1), 2, False, False),              # (H + 2p - k) % s = 1: a last row no output reads; wgrad splits its 8 images
    "s3-ragged": (6, 2, 9, 8, 4, (2, 2), (3, 3), (1, 1), (1, 1), 1, False, False),              # W: (8 + 2 - 2) % 3 = 2
    "d2": (3, 3, 8, 7, 5, (3, 3), (1, 1), (2, 2), (2, 2), 2, False, False),
    "s2-d2": (5, 2, 9, 9, 6, (3, 3), (2, 2), (1, 1), (2, 2), 1, False, False),
    "crop": (3, 2, 5, 4, 5, (2, 2), (1, 1), (3, 3), (1, 1), 2, False, False),                   # p > d (k - 1): the crop branch
    "rect": (4, 3, 9, 7, 5, (3, 2), (2, 1), (1, 0), (1, 2), 2, False, False),
    "linear": (8, 20, 1, 1, 7, (1, 1), (1, 1), (0, 0), (1, 1), 3, False, False),                # ... whose batch of 8 splits the wgrad in two
    "w-shared": (2, 3, 6, 6, 5, (3, 3), (1, 1), (1, 1), (1, 1), 3, True, False),                # wgrad folds the draws into the batch: 6 images, no split
    "x-shared": (6, 3, 6, 5, 5, (3, 3), (1, 1), (1, 1), (1, 1), 3, False, True),                # gx is summed; a batch of 6 does not split
    "dgrad-splitk": (2, 4, 5, 5, 16, (3, 3), (1, 1), (1, 1), (1, 1), 1, False, False),          # Cout = 16: the dgrad launch splits its channels in two
}


def _t64(a):
    return torch.from_numpy(np.asarray(a, F64))


def _bwd_operands(name):
    B, Cin, H, W, Cout, k, s, p, d, E, w_shared, x_shared = BWD_CASES[name]
    rng = np.random.default_rng([7, B, Cin, H, W, Cout, E])
    ho, wo = C.out_hw(H, W, *k, *s, *p, *d)
    x = rng.standard_normal((1 if x_shared else E, B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((1 if w_shared else E, Cout, Cin) + k) * 0.3).astype(np.float32)
    b = rng.standard_normal((w.shape[0], Cout)).astype(np.float32)
    gy = rng.standard_normal((E, B, Cout, ho, wo)).astype(np.float32)
    return x, w, b, gy


@functools.lru_cache(maxsize=None)
def _bwd_reference(name):
    """Per draw, float64 on the CPU from the same fp32 operands: gx, gw and their magnitudes from the absolute operands."""
    B, Cin, H, W, Cout, k, s, p, d, E, w_shared, x_shared = BWD_CASES[name]
    x, w, b, gy = _bwd_operands(name)
    r = {key: [] for key in ("gx", "gx_mag", "gw", "gw_mag")}
    for e in range(E):
        xe, we, ge = _t64(x[0 if x_shared else e]), _t64(w[0 if w_shared else e]), _t64(gy[e])
        for key, a, bb, cc in (("", xe, we, ge), ("_mag", xe.abs(), we.abs(), ge.abs())):
            r["gx" + key].append(torch.nn.grad.conv2d_input(a.shape, bb, cc, s, p, d).numpy())
            r["gw" + key].append(torch.nn.grad.conv2d_weight(a, bb.shape, cc, s, p, d).numpy())
    return {key: np.stack(v) for key, v in r.items()}


def _inside(got, ref, mag, what):
    got = got.detach().cpu().numpy().astype(F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = np.abs(got - ref) / (2e-5 * mag + 2e-6)
    assert np.isfinite(ratio).all() and ratio.max() <= 1.0, "%s: error / bound = %.3f at %s" % (what, ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
    return float(ratio.max())


@pytest.mark.parametrize("name", list(BWD_CASES))
def test_backward_helpers_against_float64(name):
    """conv2d_input_grad and conv2d_weight_grad -- the same kernel on a zero-upsampled gy with flipped weights, and with the axes
    swapped and stride and dilation exchanged -- every element inside 2e-5 mag + 2e-6 of float64 conv2d_input / conv2d_weight."""
    from bbb_hip import ops
    B, Cin, H, W, Cout, k, s, p, d, E, w_shared, x_shared = BWD_CASES[name]
    x, w, b, gy = _bwd_operands(name)
    ref = _bwd_reference(name)
    gx = ops.conv2d_input_grad(dev(gy), dev(w), (E, B, Cin, H, W), s, p, d)
    gw = ops.conv2d_weight_grad(dev(gy), dev(x), tuple(w.shape), s, p, d)
    torch.cuda.synchronize()
    fold = (lambda a: a.sum(0, keepdims=True)) if w_shared else (lambda a: a)
    worst = (_inside(gx, ref["gx"], ref["gx_mag"], name + " gx"), _inside(gw, fold(ref["gw"]), fold(ref["gw_mag"]), name + " gw"))
    # the branches this case was written for
    Bt = B * (E if w_shared else 1)
    assert (Bt % 2 == 0 and Bt // 2 >= 4) == (name in ("s2-ragged", "linear")), Bt                  # conv2d_weight_grad's batch split
    ho, wo = C.out_hw(H, W, *k, *s, *p, *d)
    assert Bt * ho * wo <= C.K_MAX and Cout * k[0] * k[1] * (E if x_shared else 1) <= C.K_MAX
    print("\nworst error / bound  %-12s gx %.3f  gw %.3f" % (name, *worst))


@pytest.mark.parametrize("name", list(BWD_CASES))
def test_conv2d_autograd_against_float64(name):
    """ops.conv2d(x, w, bias).backward() over the same geometries: gx (summed over the draws that share x), gw, gb."""
    from bbb_hip import ops
    B, Cin, H, W, Cout, k, s, p, d, E, w_shared, x_shared = BWD_CASES[name]
    x, w, b, gy = _bwd_operands(name)
    ref = _bwd_reference(name)
    xd, wd, bd = (dev(a).requires_grad_() for a in (x, w, b))
    y = ops.conv2d(xd, wd, bd, s, p, d)
    y.backward(dev(gy))
    torch.cuda.synchronize()
    fx = (lambda a: a.sum(0, keepdims=True)) if x_shared else (lambda a: a)
    fw = (lambda a: a.sum(0, keepdims=True)) if w_shared else (lambda a: a)
    _inside(xd.grad, fx(ref["gx"]), fx(ref["gx_mag"]), name + " x.grad")
    _inside(wd.grad, fw(ref["gw"]), fw(ref["gw_mag"]), name + " w.grad")
    g64 = gy.astype(F64)
    _inside(bd.grad, fw(g64.sum((1, 3, 4))), fw(np.abs(g64).sum((1, 3, 4))), name + " b.grad")
    # ... and the forward of the node, which may split its channels
    ys, mags = [], []
    for e in range(E):
        xe, we, be = _t64(x[0 if x_shared else e]), _t64(w[0 if w_shared else e]), _t64(b[0 if w_shared else e])
        ys.append(torch.nn.functional.conv2d(xe, we, be, s, p, d).numpy())
        mags.append(torch.nn.functional.conv2d(xe.abs(), we.abs(), be.abs(), s, p, d).numpy())
    _inside(y, np.stack(ys), np.stack(mags), name + " y")


@pytest.mark.parametrize("cin,S", [(16, 2), (32, 4), (3, 1)])
def test_conv2d_splitk_against_float64(cin, S):
    """conv2d_splitk with its channels in S chunks run as extra draws and summed (S = 1: the fall-through), against float64 -- not
    against the kernel itself."""
    from bbb_hip import ops
    E, B, H, W, Cout, k = 2, 3, 5, 5, 6, (3, 3)
    assert cin * 9 <= C.K_MAX
    s_rule = 1
    while E * -(-B * H * W // 64) * -(-Cout // 64) * s_rule < 512 and cin % (2 * s_rule) == 0 and (cin // (2 * s_rule)) * 9 >= 64:
        s_rule *= 2
    assert s_rule == S and ops._small_launch(torch.empty(E, B, cin, H, W), torch.empty(1, Cout, cin, *k), 1, 1, 1) == (S > 1)
    rng = np.random.default_rng([11, cin])
    x = rng.standard_normal((E, B, cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((E, Cout, cin) + k) * 0.3).astype(np.float32)
    b = rng.standard_normal((E, Cout)).astype(np.float32)
    y = ops.conv2d_splitk(dev(x), dev(w), dev(b), 1, 1, 1)
    torch.cuda.synchronize()
    conv = lambda e, f: torch.nn.functional.conv2d(f(_t64(x[e])), f(_t64(w[e])), f(_t64(b[e])), 1, 1, 1).numpy()
    ref, mag = (np.stack([conv(e, f) for e in range(E)]) for f in (lambda a: a, torch.abs))
    print("\nworst error / bound  splitk S=%d  y %.3f" % (S, _inside(y, ref, mag, "splitk S=%d" % S)))


# ------------------------------------------------------------------------------------------------ the LRT node
LRT_NODE = {"fused": C.Case("node-fused", "lrt-64", 4, 3, 6, 6, 5, (3, 3), p=(1, 1), E=2),               # _small_launch: False
            "split": C.Case("node-split", "lrt-64", 3, 16, 5, 5, 6, (3, 3), p=(1, 1), E=2)}              # 16 channels split in two: True


# c of the backward's bound c 2^-23 M = 4 x (CPU fp32 ratio), rounded up to a power of two.  torch's CPU convolutions sum in an order
# that depends on the thread count, so the ratio is the worse of the run with 1 and with 16 threads (x86, torch 2):
#   fused  gx 1.639  gw_mu 0.497  gw_var 1.167  gb_mu 0.064  gb_var 0.213        split  gx 1.415  gw_mu 1.341  gw_var 2.178  gb_mu 0.087  gb_var 0.481
# device (MI355X):
#   fused  gx 1.283  gw_mu 0.497  gw_var 1.236  gb_mu 0.082  gb_var 0.176        split  gx 1.392  gw_mu 1.661  gw_var 2.015  gb_mu 0.149  gb_var 0.228
LRT_BWD_C = {"fused": dict(x=8, w_mu=2, w_var=8, b_mu=0.5, b_var=1), "split": dict(x=8, w_mu=8, w_var=16, b_mu=0.5, b_var=2)}


def _lrt_node_args(c, o, grad):
    t = [dev(o[k]) for k in ("x", "w", "w_var", "b", "b_var")]
    if grad:
        t = [a.requires_grad_() for a in t]
    return t


@pytest.mark.parametrize("branch", list(LRT_NODE))
def test_lrt_node_forward_against_float64(branch):
    """ops.lrt_conv2d under autograd, on both sides of ops._small_launch (one fused launch | two split-k launches and
    lrt_sample_nchw): y inside the rounded tier's bound of act_mu + sqrt(act_var) eps with the oracle's Philox eps; an external eps;
    sample=False."""
    from bbb_hip import ops, rng
    c = LRT_NODE[branch]
    o = C.operands(c, "rounded")
    assert ops._small_launch(torch.empty(o["x"].shape), torch.empty((1,) + o["w"].shape), c.s, c.p, c.d) == (branch == "split")
    assert rng.call_dev_ptr(torch.device("cuda", torch.cuda.current_device())) == 0
    ext = np.random.default_rng(5).standard_normal((c.E, c.B, c.Cout) + c.out_hw).astype(np.float32)
    for kw, case, eps in ((dict(), c, None), (dict(eps=dev(ext)), replace(c, ext_eps=True), ext), (dict(sample=False), replace(c, sample=False), None)):
        ref = C.reference(case, dict(o, eps=eps))
        y = ops.lrt_conv2d(*_lrt_node_args(c, o, True), C.SEED, C.CALL0, C.STREAM, c.s, c.p, c.d, **kw)
        torch.cuda.synchronize()
        assert y.requires_grad
        worst = C.check_rounded(case, dict(y=y.detach().cpu().numpy(), act_mu=None, act_var=None), ref)
        print("\nworst error / bound  lrt node %-6s %-14s y %.3f" % (branch, ",".join(kw) or "philox", worst["y"]))


@pytest.mark.parametrize("branch", list(LRT_NODE))
def test_lrt_node_backward_against_float64(branch):
    """_LrtConv2d.backward: gx, gw_mu, gw_var, gb_mu, gb_var against float64 of the analytic gradient, d / d act_var = g eps /
    (2 sqrt(act_var)) with the same eps.  The node computes (y - act_mu) / (2 act_var), which cancels: no bound can be derived, so
    one is measured -- the node's own formula in fp32 with torch on the CPU, its worst error / (2^-23 x the sum of the absolute
    terms), times 4, rounded up to a power of two (the rule of the Adam and parameter-pass sweeps): LRT_BWD_C, from the CPU ratios
    recorded beside it.  The CPU run is held to the same bound, so a torch build whose fp32 convolutions round worse shows up here."""
    from bbb_hip import ops
    c = LRT_NODE[branch]
    o = C.operands(c, "rounded")
    ref = C.reference(c, o)
    assert ref["act_var"].min() >= 1e-6
    gy = np.random.default_rng(9).standard_normal(ref["y"].shape).astype(np.float32)
    geom = (c.s, c.p, c.d)
    ci, cw = torch.nn.grad.conv2d_input, torch.nn.grad.conv2d_weight

    def grads(x, wm, wv, gm, gv):
        """The five gradients from d / d act_mu = gm and d / d act_var = gv [E, B, Cout, Ho, Wo], in the tensors' dtype."""
        gx = torch.stack([ci(x[e].shape, wm, gm[e], *geom) + 2 * x[e] * ci(x[e].shape, wv, gv[e], *geom) for e in range(c.E)])
        gwm = sum(cw(x[e], wm.shape, gm[e], *geom) for e in range(c.E))
        gwv = sum(cw(x[e] * x[e], wv.shape, gv[e], *geom) for e in range(c.E))
        return dict(x=gx, w_mu=gwm, w_var=gwv, b_mu=gm.sum((0, 1, 3, 4)), b_var=gv.sum((0, 1, 3, 4)))

    x64, wm64, wv64, g64 = _t64(o["x"]), _t64(o["w"]), _t64(o["w_var"]), _t64(gy)
    gv64 = g64 * _t64(ref["eps"]) / (2 * _t64(ref["act_var"]).sqrt())
    want = grads(x64, wm64, wv64, g64, gv64)
    mag = grads(x64.abs(), wm64.abs(), wv64.abs(), g64.abs(), gv64.abs())
    # the node's own formula, fp32 on the CPU
    x32, wm32, wv32, g32 = (torch.from_numpy(a) for a in (o["x"], o["w"], o["w_var"], gy))
    f32conv = lambda x_, w_, b_: torch.stack([torch.nn.functional.conv2d(x_[e], w_, torch.from_numpy(b_), *geom) for e in range(c.E)])
    am32, av32 = f32conv(x32, wm32, o["b"]), f32conv(x32 * x32, wv32, o["b_var"]) + 1e-16
    y32 = am32 + av32.sqrt() * torch.from_numpy(ref["eps"].astype(np.float32))
    cpu = grads(x32, wm32, wv32, g32, g32 * (y32 - am32) / (2.0 * av32))
    # the device
    args = _lrt_node_args(c, o, True)
    y = ops.lrt_conv2d(*args, C.SEED, C.CALL0, C.STREAM, *geom)
    y.backward(dev(gy))
    torch.cuda.synchronize()
    for key, t in zip(("x", "w_mu", "w_var", "b_mu", "b_var"), args):
        unit = 2.0 ** -23 * mag[key].numpy()
        assert (unit > 0).all()
        r_cpu = float((np.abs(cpu[key].numpy().astype(F64) - want[key].numpy()) / unit).max())
        bound = LRT_BWD_C[branch][key]
        got = t.grad.cpu().numpy().astype(F64)
        assert got.shape == unit.shape
        r_dev = float((np.abs(got - want[key].numpy()) / unit).max())
        print("\nerror / (2^-23 sum|terms|)  lrt node %-6s g%-6s cpu fp32 %.3f  device %.3f  bound %g" % (branch, key, r_cpu, r_dev, bound))
        assert r_cpu <= bound, (branch, key, r_cpu, bound)
        assert np.isfinite(r_dev) and r_dev <= bound, (branch, key, r_cpu, r_dev, bound)
