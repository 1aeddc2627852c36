"""CPU checks of the bf16 LRT work (LaunchConfig.bf16_lrt): the contract restatement (tests/bf16_lrt_contract.py) against the
oracle, the exact-tier operand sets of tests/test_gpu_bf16_lrt.py, the configuration field, the library's new entry points, and
that the GPU file's fixed cases reach every instantiation the launcher can select.  Run with -m "not gpu"."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bbb_numpy as O
import ref_port_torch as P
import bf16_lrt_contract as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")


@pytest.fixture(scope="module")
def built():
    so = os.path.join(PKG, "bbb_hip", "libbbb_hip.so")
    if not os.path.exists(so):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    return so


def _params(net_type, cin):
    import torch
    torch.manual_seed(3)
    params = P.init_params(net_type, cin, 10, P.CONFIG_PRIORS)
    npar = {n: {k: v.numpy() for k, v in p.items()} for n, p in params.items() if not n.startswith("_")}
    npar["_prior_mu"], npar["_prior_sigma"] = params["_prior_mu"], params["_prior_sigma"]
    return npar


def _eps_fn(net_type, seed, call):
    names = [op[1] for op in O.TOPOLOGY[net_type] if op[0] in ("conv", "fc")]
    idx = {n: i for i, n in enumerate(names)}

    def fn(name, kind, shape):
        stream = 4 * idx[name] + {"W": 0, "bias": 1, "act": 2}[kind]
        return O.normal_eps(seed, call, stream, int(np.prod(shape))).reshape(shape)
    return fn


@pytest.mark.parametrize("net_type,cin", [("lenet", 1), ("alexnet", 3), ("3conv3fc", 3)])
def test_identity_rounding_is_the_oracles_lrt_forward(net_type, cin):
    """With rounding replaced by the identity the restatement is oracle.bbb_numpy.model_forward(layer_type="lrt") on the same eps
    (same operations on the same fp32 stage values, float64 accumulation): equal to float64 rounding -- here, value for value."""
    npar = _params(net_type, cin)
    x = np.random.default_rng(5).random((4, cin, 32, 32), dtype=np.float32)
    want, _ = O.model_forward(net_type, npar, x, "lrt", "softplus", _eps_fn(net_type, 99, 3))
    got = C.model_forward(net_type, npar, x, "softplus", _eps_fn(net_type, 99, 3), rounding=False)
    assert got.shape == want.shape == (4, 10)
    np.testing.assert_allclose(got.astype(np.float64), want.astype(np.float64), rtol=1e-12, atol=0)
    # ... and with the rounding on it is a perturbation of that forward of bf16 size, not the same numbers
    rounded = C.model_forward(net_type, npar, x, "softplus", _eps_fn(net_type, 99, 3))
    d = float(np.abs(rounded - want).max())
    assert 0.0 < d <= 5e-2 * float(np.abs(want).max())


def test_exact_tier_operands_are_exact():
    """Every product and partial sum of the exact tier is representable in fp32 (so any summation order gives the float64 value),
    x, x^2, W_mu and sigma^2 are bf16 values, and the float64 moments survive an fp32 round trip."""
    import test_gpu_bf16_lrt as T
    for name, c in T.CASES.items():
        B, Cin, H, W, Cout, kh, kw, s, pad, d, E = c
        x, w_mu, w_var, b_mu, b_var = T.exact_operands(c, len(name) * 31 + E)
        for a in (x, x * x, w_mu, w_var):
            assert np.array_equal(O.bf16_round(a), a), name
        # products are multiples of 2^-5 (mean) / 2^-13 (variance); the sum of their magnitudes, in those units, stays below 2^24:
        # every partial sum of every order is an integer of at most 24 bits times the unit
        K = Cin * kh * kw
        assert np.array_equal(np.round(x * 4), x * 4) and np.array_equal(np.round(w_mu * 8), w_mu * 8)
        assert np.array_equal(np.round(w_var * 2 ** 9), w_var * 2 ** 9) and np.array_equal(np.round(b_var * 2 ** 9), b_var * 2 ** 9)
        assert (K * np.abs(x).max() * np.abs(w_mu).max() + np.abs(b_mu).max()) * 2 ** 5 < 2 ** 24
        assert (K * (x * x).max() * w_var.max() + b_var.max()) * 2 ** 13 < 2 ** 24
        # the float64 moments of a few images survive the fp32 round trip (and so does 1e-16 + var: it rounds to var)
        xs = x[0, :2].astype(np.float64)
        cols, ho, wo = O.im2col(xs, kh, kw, s, pad, d)
        mu = cols @ w_mu.reshape(Cout, -1).astype(np.float64).T + b_mu.astype(np.float64)
        cols2, _, _ = O.im2col(xs * xs, kh, kw, s, pad, d)
        var = cols2 @ w_var.reshape(Cout, -1).astype(np.float64).T + b_var.astype(np.float64)
        assert np.array_equal(mu.astype(np.float32).astype(np.float64), mu), name
        assert np.array_equal(var.astype(np.float32).astype(np.float64), var), name
        assert np.array_equal((np.float32(1e-16) + var.astype(np.float32)), var.astype(np.float32)), name
        assert (ho, wo) == T.out_hw(c)


def test_launch_config_field():
    from bbb_hip import ops
    cfg = ops.LaunchConfig()
    assert cfg.bf16_lrt is False and "bf16_lrt" in ops.LaunchConfig.FIELDS
    on = cfg.copy(bf16_lrt=True)
    assert on.bf16_lrt is True and on.key() != cfg.key() and len(on.key()) == len(ops.LaunchConfig.FIELDS)
    with ops.use_config(bf16_lrt=True) as c:
        assert c.bf16_lrt and ops.current_config().bf16_lrt
    assert ops.current_config().bf16_lrt is False
    assert "bf16_lrt" in ops.LaunchConfig.__doc__


def test_library_exports_the_new_entry_points(built):
    from bbb_hip import _lib
    h = _lib.lib()
    for name in ("bbb_lrt_conv2d_chwn_bf16_fwd", "bbb_lrt_conv2d_chwn_bf16_plan", "bbb_lrt_sample_chwn_bf16", "bbb_lrt_weights_bf16"):
        assert name in _lib.EXPORTS and hasattr(h, name)
    assert h.bbb_abi_version() == 13
    # argument checks come back without a device
    d = _lib.ConvDesc()
    assert h.bbb_lrt_conv2d_chwn_bf16_fwd(ctypes.byref(d), None, None, None, None, None, None, None, None, 0, 0, 0, 1, None, 0, None) == -1
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = 12, 3, 8, 8, 4, 3, 3
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = d.draws = 1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    assert h.bbb_lrt_conv2d_chwn_bf16_fwd(ctypes.byref(d), p, p, p, None, None, p, None, None, 0, 0, 0, 1, None, 0, None) == -3   # B % 8
    d.batch = 16
    d.w_draw_stride = 4 * 32
    assert h.bbb_lrt_conv2d_chwn_bf16_fwd(ctypes.byref(d), p, p, p, None, None, p, None, None, 0, 0, 0, 1, None, 0, None) == -1   # per-draw weights
    d.w_draw_stride = 0
    d.unit_div = 2
    assert h.bbb_lrt_conv2d_chwn_bf16_fwd(ctypes.byref(d), p, p, p, None, None, p, None, None, 0, 0, 0, 1, None, 0, None) == -1   # work units
    assert h.bbb_lrt_sample_chwn_bf16(None, None, None, 1, 1, 1, 8, 0, 0, 0, 0, 0, None, None) == -1
    assert h.bbb_lrt_weights_bf16(None, 1, None) == -1
    seg = (_lib.RowsSegment * 1)()
    assert h.bbb_lrt_weights_bf16(seg, _lib.BF16_ROWS_MAX_SEGMENTS + 1, None) == -1
    assert ctypes.sizeof(_lib.RowsSegment) == 32


def test_gpu_cases_reach_every_instantiation(built):
    """The fixed cases of tests/test_gpu_bf16_lrt.py reach every instantiation bbb_lrt_conv2d_chwn_bf16_fwd can select -- the three
    tile shapes, one and two k-groups for each, the wave-specialised form of the 128 x 128 shape -- each with fp32 and bf16 output,
    with tap-major and reference-order rows, and as a moments-only launch.  The choices are the library's own
    (bbb_lrt_conv2d_chwn_bf16_plan), the ones the launcher makes."""
    import test_gpu_bf16_lrt as T
    from bbb_hip import ops
    per_case = {n: T.case_branches(n, ops.lrt_bf16_plan) for n in T.CASES}
    tags = set().union(*per_case.values())
    assert {"inst:22-kg1-ws", "inst:22-kg1-plain", "inst:22-kg2-plain", "inst:14-kg1-plain", "inst:14-kg2-plain",
            "inst:12-kg1-plain", "inst:12-kg2-plain"} <= tags, tags
    assert {"out-f32", "out-bf16", "moments-only", "rows-reference", "rows-tap-major"} <= tags
    # tap-major rows on every tile shape and on both k-group counts
    tm = set().union(*(t for t in per_case.values() if "rows-tap-major" in t))
    assert {"shape22", "shape14", "shape12", "kg1", "kg2", "ws", "no-ws"} <= tm, tm
    # the geometries the sweep promises
    cs = T.CASES.values()
    assert {c[0] for c in cs} >= {8, 200, 256} and {c[10] for c in cs} >= {1, 3, 10} and {c[4] for c in cs} >= {6, 10, 84, 100, 192}
    assert any(c[7] == 2 for c in cs) and any(c[9] == 2 for c in cs) and any(c[5] != c[6] for c in cs) and any(c[2] != c[3] for c in cs)
    assert any(c[8] == (c[9] * (c[5] - 1), c[9] * (c[6] - 1)) and c[8] != (0, 0) for c in cs)          # padding d (k - 1)
    assert any(c[2] == c[3] == 1 and c[1] >= 1000 for c in cs) and any(T.out_hw(c) == (1, 1) and c[5] > 1 for c in cs)
    assert any(c[1] in range(1, 8) and c[5] > 1 for c in cs)                                             # first layers on 1..7 channels
    # the number of k-groups belongs to the layer: the launch size (draws, batch) never changes it
    for c in cs:
        kgs = {ops.lrt_bf16_plan((E, c[1], c[2], c[3], B), c[4], (c[1], c[5], c[6]), c[7], c[8], c[9])[1] for E in (1, 3, 10, 64) for B in (8, 200, 512)}
        assert len(kgs) == 1, c
