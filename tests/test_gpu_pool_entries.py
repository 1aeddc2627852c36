"""The pooling entries through their wrappers, bit for bit: the max pools of csrc/pool2d.hip and csrc/pool2d_bf16.hip against torch's
own max pooling and its autograd on the CPU, and each average wrapper under its own name against the same launch reached through avg=.

Everything compared is exact, so there is no tolerance: inputs are small integers (windows hold ties, and torch's rule -- the FIRST
maximum in scan order receives the gradient -- decides), incoming gradients are small integers (sums over overlapping windows are
exact in any order, in fp32 and in bf16), and ReLU's derivative is 0 or 1.  Softplus and the LRT variance gradient stay with the
tolerance tests (test_gpu_kernels, test_gpu_train_fuzz, test_gpu_bf16_train).

Maps: 7 x 6 (not square; floor mode drops a row) and 8 x 8 with B = 16, where H * W * B = 1024 and pad_planes really pads.  Batches:
8 (two fp32 groups of images, one bf16 group) and 16.  Leading shapes [3] and [2, 3].  Windows (k, s): (2, 2), (3, 2) overlapping,
(3, 1), (2, 3) with gaps, and k = 0, the activation alone.  Run with -m gpu."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAPS = [(7, 6, 8), (7, 6, 16), (8, 8, 16)]
LEADS = [(3,), (2, 3)]
WINDOWS = [(2, 2), (3, 2), (3, 1), (2, 3), (0, 1)]


def _nchw(t):
    """[*lead, H, W, B] -> [B, planes, H, W] on the CPU, fp32."""
    *lead, H, W, B = t.shape
    return t.detach().float().cpu().reshape(-1, H, W, B).permute(3, 0, 1, 2).contiguous()


def _chwn(t, lead):
    """[B, planes, H, W] -> [*lead, H, W, B]."""
    B, _, H, W = t.shape
    return t.permute(1, 2, 3, 0).reshape(*lead, H, W, B).contiguous()


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _reference(v, g, k, s, act):
    """(pooled activated output, gradient w.r.t. the pre-activation v) by torch on the CPU; v, g in NCHW."""
    v = v.clone().requires_grad_(True)
    y = torch.relu(v) if act == "relu" else v
    p = F.max_pool2d(y, k, s) if k else y
    p.backward(g)
    return p.detach(), v.grad


@pytest.fixture(scope="module")
def cases():
    """Per (map, leading shape): the pre-activation v, its ReLU, and per window the incoming gradient with the references --
    computed once, shared by the tests below, never written to."""
    gen = torch.Generator().manual_seed(20261019)
    out = {}
    for H, W, B in MAPS:
        for lead in LEADS:
            v = _ints(gen, (*lead, H, W, B), -2, 2)                         # five values: ties in every window; ReLU clips two of them
            ent = dict(v=v, wins={})
            for k, s in WINDOWS:
                ho, wo = ((H - k) // s + 1, (W - k) // s + 1) if k else (H, W)
                g = _ints(gen, (*lead, ho, wo, B), -3, 3)
                ref = {act: _reference(_nchw(v), _nchw(g), k, s, act) for act in (None, "relu")}
                ent["wins"][(k, s)] = dict(g=g, ref=ref)
            out[(H, W, B, lead)] = ent
    return out


def _eq(got, want_nchw, lead, what):
    want = _chwn(want_nchw, lead)
    got = got.detach().float().cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert torch.equal(got, want), (what, int((got != want).sum()))


@pytest.mark.parametrize("lead", LEADS, ids=["lead3", "lead2x3"])
@pytest.mark.parametrize("hwb", MAPS, ids=["7x6x8", "7x6x16", "8x8x16"])
def test_max_forward_is_torchs(cases, hwb, lead):
    from bbb_hip import ops
    ent = cases[hwb + (lead,)]
    for act in (None, "relu"):
        y = (torch.relu(ent["v"]) if act else ent["v"]).to(DEV)
        for (k, s), w in ent["wins"].items():
            if k == 0:
                continue
            _eq(ops.maxpool_chwn(y, k, s), w["ref"][act][0], lead, ("fp32", k, s, act))
            _eq(ops.maxpool_chwn_bf16(y.to(torch.bfloat16), k, s), w["ref"][act][0], lead, ("bf16", k, s, act))
    torch.cuda.synchronize()


@pytest.mark.parametrize("lead", LEADS, ids=["lead3", "lead2x3"])
@pytest.mark.parametrize("hwb", MAPS, ids=["7x6x8", "7x6x16", "8x8x16"])
def test_max_backward_is_torch_autograd(cases, hwb, lead):
    from bbb_hip import ops
    H, W, B = hwb
    ent = cases[hwb + (lead,)]
    padded = ops.padded_plane_pitch(H * W * B) != H * W * B
    assert padded == (H * W * B == 1024)                                   # the 8 x 8 x 16 map is the one whose planes get a pad
    for act in (None, "relu"):
        y = (torch.relu(ent["v"]) if act else ent["v"]).to(DEV)
        yb = y.to(torch.bfloat16)
        # one draw's worth of moments where there are draws ([2, 3]: [1, 3, H, W, B]); positive variances; their values do not reach g_mu
        mom = (1,) + tuple(y.shape[1:]) if len(lead) == 2 else tuple(y.shape)
        am, av = torch.zeros(mom, device=DEV), torch.full(mom, 0.5, device=DEV)
        for (k, s), w in ent["wins"].items():
            g, want = w["g"].to(DEV), w["ref"][act][1]
            tag = (k, s, act)
            # fp32 planes: dense, at the padded pitch, and the LRT form's g_mu
            dense = ops.pool_act_backward_chwn(g, y, k, s, act)
            _eq(dense, want, lead, ("fp32",) + tag)
            pad = ops.pool_act_backward_chwn(g, y, k, s, act, pad_planes=True)
            assert torch.equal(pad, dense) and pad.is_contiguous() != padded, ("fp32 pad_planes",) + tag
            g_mu, g_var = ops.lrt_pool_act_backward_chwn(g, y, am, av, k, s, act)
            assert torch.equal(g_mu, dense) and g_var.shape == dense.shape, ("lrt g_mu",) + tag
            g_mu_p, _ = ops.lrt_pool_act_backward_chwn(g, y, am, av, k, s, act, pad_planes=True)
            assert torch.equal(g_mu_p, dense), ("lrt g_mu pad_planes",) + tag
            both = ops.lrt_pool_act_backward_chwn(g, y, am, av, k, s, act, stacked=True)
            assert both.shape == (2,) + tuple(dense.shape) and torch.equal(both[0], dense), ("lrt stacked",) + tag
            # bf16 storage: bf16 and fp32 incoming gradients, bf16 and fp32 outputs, dense and padded
            for gin in (g.to(torch.bfloat16), g):
                for out_f32 in (False, True):
                    r = ops.pool_act_backward_chwn_bf16(gin, yb, k, s, act, out_f32=out_f32)
                    assert r.dtype == (torch.float32 if out_f32 else torch.bfloat16)
                    _eq(r, want, lead, ("bf16", str(gin.dtype), out_f32) + tag)
                    rp = ops.pool_act_backward_chwn_bf16(gin, yb, k, s, act, out_f32=out_f32, pad_planes=True)
                    assert torch.equal(rp, r) and rp.is_contiguous() != padded, ("bf16 pad_planes", str(gin.dtype), out_f32) + tag
            if k == 0 and act is None:                                      # without y: the rounding alone
                _eq(ops.pool_act_backward_chwn_bf16(g, None, 0, 1, None), want, lead, ("bf16 rounding only",) + tag)
    torch.cuda.synchronize()


AVG = ((3, 2), (2, 1), (1, 0), False)                                     # a rectangular, overlapping, padded window; valid-tap divisors


@pytest.mark.parametrize("pad_planes", [False, True], ids=["dense", "padded"])
def test_average_wrappers_are_the_avg_form_of_the_max_wrappers(pad_planes):
    """Each average backward wrapper, called by its own name and through avg= of its max twin: the same launch, the same bits."""
    from bbb_hip import ops
    gen = torch.Generator().manual_seed(7)
    H, W, B, lead = 8, 8, 16, (2, 3)
    y = torch.randn((*lead, H, W, B), generator=gen).abs().to(DEV)
    ho, wo = ops.avgpool_plan(H, W, B, *AVG)[:2]
    g = torch.randn((*lead, ho, wo, B), generator=gen).to(DEV)
    am, av = torch.randn((1, 3, H, W, B), generator=gen).to(DEV), (torch.rand((1, 3, H, W, B), generator=gen) + 0.5).to(DEV)
    for act in (None, "relu", "softplus"):
        a = ops.avgpool_act_backward_chwn(g, y, *AVG, act, pad_planes=pad_planes)
        b = ops.pool_act_backward_chwn(g, y, 0, 1, act, pad_planes=pad_planes, avg=AVG)
        assert torch.equal(a, b), ("fp32", act)
        a = ops.lrt_avgpool_act_backward_chwn(g, y, am, av, *AVG, act, pad_planes=pad_planes)
        b = ops.lrt_pool_act_backward_chwn(g, y, am, av, 0, 1, act, pad_planes=pad_planes, avg=AVG)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), ("lrt", act)
        yb = y.to(torch.bfloat16)
        for gin in (g.to(torch.bfloat16), g):
            for out_f32 in (False, True):
                a = ops.avgpool_act_backward_chwn_bf16(gin, yb, *AVG, act, out_f32=out_f32, pad_planes=pad_planes)
                b = ops.pool_act_backward_chwn_bf16(gin, yb, 0, 1, act, out_f32=out_f32, pad_planes=pad_planes, avg=AVG)
                assert a.dtype == b.dtype and torch.equal(a, b), ("bf16", act, str(gin.dtype), out_f32)
    torch.cuda.synchronize()
