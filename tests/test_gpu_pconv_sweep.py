"""The batch-innermost fp32 implicit GEMM (csrc/pconv_gemm.hip, csrc/pconv_body.cuh), launch form by launch form, against the
float64 reference of tests/pconv_contract.py: ops.conv2d_chwn_forward (BBB) and ops.lrt_conv2d_chwn_forward (LRT) on every case of
pconv_contract.CASES, each in two tiers.

  exact    dyadic operands, every partial sum of either contraction an fp32 number in any summation order: act_mu and act_var
           (LRT, unpooled: the launch is asked for its moments), and y wherever no noise and no transcendental enters it (BBB and
           sample=False launches with act none / relu -- a case that samples or ends in softplus is launched once more without
           the noise and without the softplus; its own y is held to the rounded tier's bound), EQUAL the reference.  One
           dropped, duplicated or mis-addressed tap fails this.  No case is outside the precondition (pconv_contract.exact_bits
           is at most 18 of the 24 bits).
  rounded  Gaussian operands, every element inside the per-element bounds listed in pconv_contract's docstring.

Which form a case runs is the library's answer (ops.fp32_fwd_plan = bbb_conv2d_chwn_plan, the launch entries' own plan), asserted
per case; tests/test_pconv_sweep_cpu.py holds the table's coverage of the fifteen forms and of every plan / kernel edge.  The
device-side call counter (rng.call_dev_ptr) is NULL during a case unless the case sets it to a value of its own.

Measured on an MI355X: 43 cases + 2 pairs, 45 tests in 6.7 s (slowest 0.9 s); every exact-tier comparison equal; worst
error / bound of the rounded tier per form (moments where a case of the form asks for them; a pooled launch keeps none):

  form            cases  act_mu  act_var  y       compared for equality
  bbb-64-ilv      10     -       -        0.018    1 689 080
  bbb-64           1     -       -        0.007    6 193 152
  bbb-128-ilv      2     -       -        0.011    2 431 552
  bbb-128          1     -       -        0.004   12 582 912
  bbb-seq64-ilv    1     -       -        0.009       98 560
  bbb-seq64        1     -       -        0.010    3 084 288
  bbb-seq128-ilv   1     -       -        0.010      393 216
  bbb-seq128       1     -       -        0.011    6 160 384
  bbb-cross        3     -       -        0.009      122 656
  bbb-pool         2     -       -        0.008      460 520
  lrt-64-ilv      10     0.014   0.034    0.014    7 770 120
  lrt-64           1     0.005   0.006    0.009   31 457 280
  lrt-seq64        2     0.006   0.020    0.011    3 573 840
  lrt-cross        4     0.005   0.018    0.008      946 480
  lrt-pool         3     -       -        0.012    1 132 040

The same bounds hold for the 24 geometries of tests/test_gpu_fuzz.py through both LRT kernels (test_random_geometry_lrt_kernels)."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

import pconv_contract as C

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=4)
def _operands_and_reference(name, tier):
    c = C.CASES[name]
    o = C.operands(c, tier)
    return o, C.reference(c, o)


def launch(c, o, sample=None, moments=None):
    """Case c on the operands o -> dict(y, act_mu, act_var) of numpy arrays [E, Cout, Ho(/2), Wo(/2), B]."""
    from bbb_hip import ops, rng
    sample = c.sample if sample is None else sample
    moments = c.moments if moments is None else moments
    kw = dict(act=c.act, pool=c.pool)
    if c.x[0] == "units":
        kw.update(units=(c.x[1], c.x[2]), n_units=c.E, x_per_slice=c.x[3])
    elif c.x[0] == "div":
        kw.update(x_div=c.x[1], x_off=c.x[2])
    x = dev(o["x"])
    if not c.lrt:
        w = o["w"].transpose(0, 1, 3, 4, 2) if c.wtap else o["w"]
        y = ops.conv2d_chwn_forward(x, dev(w), dev(o["b"]), c.s, c.p, c.d, bf16x3=False, w_tap_major=c.wtap, **kw)
        am = av = None
    else:
        if c.x[0] == "div":
            kw["n_slabs"] = c.E
        args = (x, dev(o["w"]), dev(o["w_var"]), dev(o["b"]), dev(o["b_var"]), C.SEED, C.CALL0, C.STREAM, c.s, c.p, c.d)
        kw.update(sample=sample, eps=dev(o["eps"]) if sample else None, want_moments=moments, b_offset=c.b_offset)
        if c.call_dev is None:
            assert rng.call_dev_ptr(x.device) == 0
            y, am, av = ops.lrt_conv2d_chwn_forward(*args, **kw)
        else:
            counter = torch.tensor([c.call_dev - 2 ** 32 if c.call_dev >= 2 ** 31 else c.call_dev], dtype=torch.int32, device=x.device)
            with rng.device_call_offset(counter):
                assert rng.call_dev_ptr(x.device) == counter.data_ptr()
                y, am, av = ops.lrt_conv2d_chwn_forward(*args, **kw)
            assert int(counter.item()) & 0xFFFFFFFF == c.call_dev                      # a launch reads the counter, never moves it
    torch.cuda.synchronize()
    return dict(y=y.cpu().numpy(), act_mu=None if am is None else am.cpu().numpy(), act_var=None if av is None else av.cpu().numpy())


@pytest.mark.parametrize("name", list(C.CASES))
def test_form_by_form_against_float64(name):
    c = C.CASES[name]
    plan = C.case_plan(c)
    assert plan[0] == c.form, (name, plan)
    # exact tier
    assert max(C.exact_bits(c)) <= 24
    o, ref = _operands_and_reference(name, "exact")
    got = launch(c, o, moments=c.lrt and not c.pool)
    n = C.check_exact(c, got, ref)
    if (c.lrt and c.sample) or c.act == "softplus":
        # the same launch without noise and without the transcendental: its y must equal the reference too
        quiet = replace(c, sample=False, act=None if c.act == "softplus" else c.act)
        n += C.check_exact(quiet, launch(quiet, o, moments=c.lrt and not c.pool), C.reference(quiet, o))
    assert n >= got["y"].size
    # rounded tier
    o, ref = _operands_and_reference(name, "rounded")
    worst = C.check_rounded(c, launch(c, o), ref)
    print("\nworst error / bound  %-12s %-24s %s  exact: %d elements equal" % (
        c.form, name, "  ".join("%s %.3f" % kv for kv in worst.items()), n))


@pytest.mark.parametrize("small,large", C.PAIRS)
def test_cross_and_seq_forms_of_one_layer_agree_bitwise(small, large):
    """The same layer one item below and one item above the cross-workgroup form's limit: the slabs both launches compute are the
    same bits (the split is the layer's: same partial sums, added in the same order)."""
    a, b = C.CASES[small], C.CASES[large]
    assert C.case_plan(a)[0].endswith("cross") and "seq" in C.case_plan(b)[0] and b.E == a.E + 1
    oa, ob = C.operands(a, "rounded"), C.operands(b, "rounded")
    assert all(np.array_equal(oa[k], ob[k][:len(oa[k])] if k == "w" and not a.lrt else ob[k]) for k in ("x", "w", "w_var") if oa[k] is not None)
    ya, yb = launch(a, oa, moments=a.lrt), launch(b, ob, moments=a.lrt)
    for k in ("y", "act_mu", "act_var"):
        if ya[k] is not None:
            assert np.array_equal(ya[k], yb[k][:a.E]), (small, large, k)
