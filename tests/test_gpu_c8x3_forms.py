"""Every kernel instantiation bbb_conv2d_c8x3_fwd / bbb_lrt_conv2d_c8x3_fwd can start (the 20 BBB_C8X3_FORM_* of include/bbb_hip.h),
each on the smallest launch that takes it: ops.c8x3_fwd_plan (the launch entries' own plan, csrc/pconv_c8x3_plan.h) names the form,
the output is bit for bit the NT = 2 / 128-image launch of the same operands (the MFMA sequence per output element does not depend
on the workgroup tile), and one form per output kind is held to the float64 oracle at the bound of tests/test_gpu_c8x3.py.
Shapes are ragged against every tile: 200 channels against 64 / 96 / 128, 132 images against 128, 260 against 256, 40 and 72 against
the pooled form's 32 / 64.  Run with -m gpu."""
import numpy as np
import pytest
import torch

import bbb_numpy as O

pytestmark = pytest.mark.gpu
TOL = 4e-6

# B, Cin, H, W, Cout, k, pad, E
PLAIN = (132, 16, 3, 3, 200, 3, 1, 2)
LARGE = (260, 16, 16, 16, 128, 1, 0, 2)          # 2 048 items of 256 images: the 256-image tile without a flag
POOLED = {40: (40, 16, 6, 6, 200, 3, 0, 2), 72: (72, 16, 6, 6, 200, 3, 0, 2)}


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import ops
    cache = {}

    def operands(shape):
        """(x fp32, w fp32, bias, x c8 S3, w tap-major) of a shape, made once"""
        if shape not in cache:
            B, Cin, H, W, Cout, k, _, E = shape
            torch.manual_seed(B + Cout + H)
            x = torch.randn(E, Cin, H, W, B, device="cuda")
            w = torch.randn(E, Cout, Cin, k, k, device="cuda") * 0.1
            bias = torch.randn(E, Cout, device="cuda") * 0.1
            cache[shape] = (x, w, bias, ops.c8s3_from_f32(x), ops.w_tap_major(w))
        return cache[shape]
    return dict(ops=ops, operands=operands)


def _plan(ops, shape, **kw):
    B, Cin, H, W, Cout, k, p, E = shape
    return ops.c8x3_fwd_plan((E, Cin, H, W, B), Cout, k, 1, p, 1, **kw)


BBB_FORMS = [(nt, mt, out) for nt in (2, 3, 4) for mt in (1, 2) for out in ("s3", "f32")]


@pytest.mark.parametrize("nt,mt,out", BBB_FORMS)
def test_plain_forms_by_flag(env, nt, mt, out):
    ops = env["ops"]
    x, w, bias, xc, wt = env["operands"](PLAIN)
    B, Cin, H, W, Cout, k, p, E = PLAIN
    of32, tile = out == "f32", 128 * mt
    assert _plan(ops, PLAIN, out_f32=of32, nt=nt, tile=tile)[:3] == (f"nt{nt}-mt{mt}-{out}", nt, tile)
    assert _plan(ops, PLAIN, out_f32=of32)[0] == f"nt2-mt1-{out}"                         # what the library picks here: 132 images, 24 items
    ref = ops.conv2d_c8x3_forward(xc, wt, bias, k, 1, p, 1, act="softplus", out_f32=of32, nt=2, tile=128)
    got = ops.conv2d_c8x3_forward(xc, wt, bias, k, 1, p, 1, act="softplus", out_f32=of32, nt=nt, tile=tile)
    assert got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.parametrize("out", ["s3", "f32"])
def test_the_256_image_tile_by_launch_size(env, out):
    ops = env["ops"]
    x, w, bias, xc, wt = env["operands"](LARGE)
    B, Cin, H, W, Cout, k, p, E = LARGE
    of32 = out == "f32"
    assert _plan(ops, LARGE, out_f32=of32) == (f"nt2-mt2-{out}", 2, 256, 2048, 2048)
    assert _plan(ops, LARGE, out_f32=of32, draws=1)[:3] == (f"nt2-mt2-{out}", 2, 256)       # 1 024 items: still 256
    assert _plan(ops, LARGE, out_f32=of32, tile=128)[:3] == (f"nt2-mt1-{out}", 2, 128)
    ref = ops.conv2d_c8x3_forward(xc, wt, bias, k, 1, p, 1, act="softplus", out_f32=of32, nt=2, tile=128)
    got = ops.conv2d_c8x3_forward(xc, wt, bias, k, 1, p, 1, act="softplus", out_f32=of32)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("B", [40, 72])
@pytest.mark.parametrize("nt,mt", [(nt, mt) for nt in (2, 3, 4) for mt in (1, 2)])
def test_pooled_forms_by_flag(env, B, nt, mt):
    ops = env["ops"]
    shape = POOLED[B]
    x, w, bias, xc, wt = env["operands"](shape)
    _, Cin, H, W, Cout, k, p, E = shape
    tile = 32 * mt
    assert _plan(ops, shape, pool=True, nt=nt, tile=tile)[:3] == (f"nt{nt}-mt{mt}-pool", nt, tile)
    assert _plan(ops, shape, pool=True)[0] == "nt2-mt1-pool"                                # 32 items of 64 images: the 32-image tile
    ref = ops.conv2d_c8x3_forward(xc, wt, bias, k, 1, p, 1, act="softplus", pool=True, nt=2, tile=32)
    got = ops.conv2d_c8x3_forward(xc, wt, bias, k, 1, p, 1, act="softplus", pool=True, nt=nt, tile=tile)
    assert got.shape == (E, 3, Cout // 8, 2, 2, B, 8) and torch.equal(got, ref)


@pytest.mark.parametrize("out", ["s3", "f32"])
def test_lrt_forms(env, out):
    """One instantiation per output kind whatever the tile flag says; the same noise key gives the same bits."""
    ops = env["ops"]
    x, w, bias, xc, wt = env["operands"](PLAIN)
    B, Cin, H, W, Cout, k, p, E = PLAIN
    of32 = out == "f32"
    for tile in (None, 128, 256):
        assert _plan(ops, PLAIN, out_f32=of32, lrt=True, tile=tile)[:3] == (f"lrt-{out}", 2, 128)
    x6 = ops.c8s3_from_f32(x, squares=True)
    torch.manual_seed(9)
    w_var = ops.w_tap_major(torch.rand(1, Cout, Cin, k, k, device="cuda") * 0.01)[0]
    b_var = torch.rand(Cout, device="cuda") * 0.01
    run = lambda tile: ops.lrt_conv2d_c8x3_forward(x6, wt[0], w_var, bias[0], b_var, k, 77, 5, 6, 1, p, 1, act="softplus", out_f32=of32, tile=tile)
    ref = run(128)
    assert torch.equal(run(None), ref) and torch.equal(run(256), ref)
    assert not torch.equal(ref, ops.lrt_conv2d_c8x3_forward(x6, wt[0], w_var, bias[0], b_var, k, 77, 6, 6, 1, p, 1, act="softplus", out_f32=of32,
                                                            tile=128))                     # (another noise key: other samples)


def _oracle(x, w, bias, p):
    """float64 conv and the magnitude sum |w||x| + |b| per output element, [E][B, Cout, Ho, Wo]"""
    want, mag = [], []
    for e in range(w.shape[0]):
        xe = x[e].permute(3, 0, 1, 2).double().cpu().numpy()
        we, be = w[e].double().cpu().numpy(), bias[e].double().cpu().numpy()
        want.append(O.conv2d(xe, we, be, 1, p, 1))
        mag.append(O.conv2d(np.abs(xe), np.abs(we), np.abs(be), 1, p, 1))
    return np.stack(want), np.stack(mag)


def test_one_form_per_output_kind_against_float64(env):
    ops = env["ops"]
    x, w, bias, xc, wt = env["operands"](PLAIN)
    B, Cin, H, W, Cout, k, p, E = PLAIN
    want, mag = _oracle(x, w, bias, p)
    assert _plan(ops, PLAIN, nt=3, tile=256)[0] == "nt3-mt2-s3" and _plan(ops, PLAIN, nt=4, tile=128, out_f32=True)[0] == "nt4-mt1-f32"
    got = ops.c8s3_to_f32(ops.conv2d_c8x3_forward(xc, wt, bias, k, 1, p, 1, nt=3, tile=256)).permute(0, 4, 1, 2, 3).double().cpu().numpy()
    worst = float((np.abs(got - want) / mag).max())
    print(f"nt3-mt2-s3: {worst:.2e} of sum|w||x|")
    assert worst <= TOL
    got = ops.conv2d_c8x3_forward(xc, wt, bias, k, 1, p, 1, nt=4, tile=128, out_f32=True).permute(0, 4, 1, 2, 3).double().cpu().numpy()
    worst = float((np.abs(got - want) / mag).max())
    print(f"nt4-mt1-f32: {worst:.2e} of sum|w||x|")
    assert worst <= TOL
    # pooled: the maximum of a window moves by at most the largest error among its four pixels
    shape = POOLED[72]
    x, w, bias, xc, wt = env["operands"](shape)
    B, Cin, H, W, Cout, k, p, E = shape
    want, mag = _oracle(x, w, bias, p)                                                      # [E, B, Cout, 4, 4]
    win = lambda a: a.reshape(E, B, Cout, 2, 2, 2, 2).max(axis=(4, 6))
    assert _plan(ops, shape, pool=True, nt=3, tile=64)[0] == "nt3-mt2-pool"
    got = ops.c8s3_to_f32(ops.conv2d_c8x3_forward(xc, wt, bias, k, 1, p, 1, pool=True, nt=3, tile=64)).permute(0, 4, 1, 2, 3).double().cpu().numpy()
    worst = float((np.abs(got - win(want)) / win(mag)).max())
    print(f"nt3-mt2-pool: {worst:.2e} of the window's largest sum|w||x|")
    assert worst <= TOL
