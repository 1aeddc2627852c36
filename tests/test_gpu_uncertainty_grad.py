"""The backward of the batch-innermost uncertainty reduction (csrc/mc_uncertainty.hip: bbb_mc_uncertainty_cb_bwd) on the device, through
ops.mc_uncertainty_cb_autograd: every named case of tests/uncertainty_cb_contract.py under every upstream pattern of
tests/uncertainty_grad_contract.py against float64, inside DEVICE_FACTOR x the error of the fp32 model -- a bound taken from the
reference and the model (tests/test_uncertainty_grad_cpu.py), never from a kernel; NaN at exactly the reference's positions, exact
zeros at classes of probability 0.  Bitwise where one kernel computes both sides: two runs, an image inside a batch of 130 against the
same image in a batch of 66, a field left out against the same field with a zero upstream gradient, the forward outputs against
ops.mc_uncertainty_cb.  Model level: uncertainty.saliency against the manual composition (bitwise) and against the float64 gradient of
the scores fed through the same autograd node, trainable and bf16 routes, a model off the fast path, and the refusals.
Needs an MI355X: -m gpu."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import ref_port_torch as P
import tail_contract as TC
import uncertainty_cb_contract as K
import uncertainty_grad_contract as G

pytestmark = pytest.mark.gpu
WORST = {}
SCORES = ("entropy", "expected_entropy", "mutual_info")


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import _lib, ensemble, fast_train, ops, rng, uncertainty, zoo
    _lib.lib()
    saved = dict(rng._state)
    yield {"ops": ops, "lib": _lib, "ens": ensemble, "rng": rng, "unc": uncertainty, "zoo": zoo, "ft": fast_train}
    rng._state.clear()
    rng._state.update(saved)
    for k in sorted(WORST):
        print("[uncertainty-grad worst] %-18s %.3f at %s (bound %g)" % (k, WORST[k][0], WORST[k][1], G.bound(k)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _grad(ops, x, normalized, w):
    """d sum(w x outputs) / d logits through the autograd entry: x [T][C][B] device leaf, w {field: numpy or None} -> (device
    tensor [T][C][B], the forward outputs).  Only the fields with a weight are asked for."""
    want = tuple(f for f in G.FIELDS if w[f] is not None)
    out = ops.mc_uncertainty_cb_autograd(x, normalized=normalized, want=want)
    g, = torch.autograd.grad([getattr(out, f) for f in want], x, grad_outputs=[_dev(w[f]) for f in want])
    return g, out


def _as_rows(g):
    return g.detach().permute(0, 2, 1).cpu().numpy()                   # [T][B][C], as the contract's arrays


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_case_within_bounds_every_pattern(env, case):
    ops = env["ops"]
    rows, norm, inj = G.rows_of(case), case.p["normalized"], case.p.get("inject")
    x = _dev(TC.layout(case, rows)).requires_grad_(True)
    clean = _dev(TC.layout(case, K._recipe_rows(case))).requires_grad_(True) if inj in ("nan", "posinf") else None
    for pat in G.PATTERNS:
        w = G.upstream_of(case, pat)
        g64, A = G.reference(rows, norm, w)
        g, out = _grad(ops, x, norm, w)
        assert g.shape == x.shape and g.dtype == torch.float32
        got = _as_rows(g)
        r = G.ratio(got, g64, A)                                        # (asserts the NaN / infinity positions and the exact zeros)
        print("%s %s: %.3f (bound %g)" % (case.name, pat, r, G.bound(pat)))
        if r > WORST.get(pat, (-1.0, ""))[0]:
            WORST[pat] = (r, case.name)
        assert r <= G.bound(pat), (case.name, pat, r)
        if inj in ("neginf_some", "neginf_all"):
            at = np.isneginf(rows)
            assert np.isfinite(got).all(), (case.name, pat)
            if w["pred"] is None:
                assert not got[at].any(), (case.name, pat)             # probability 0: an exact 0, not 0 x -inf
            else:
                assert np.array_equal(got[at], np.broadcast_to((w["pred"] / np.float32(case.slabs))[None], rows.shape)[at])
        if clean is not None:                                           # a NaN / +inf stays inside its image
            hit = np.zeros(case.B, bool)
            hit[[5, 64]] = True
            g0, _ = _grad(ops, clean, norm, w)
            assert torch.equal(_bits(g[:, :, ~hit]), _bits(g0[:, :, ~hit])), (case.name, pat)
            assert np.isnan(got[:, hit]).all() and not np.isinf(got).any(), (case.name, pat)


@pytest.mark.parametrize("normalized", [False, True], ids=["softmax", "normalized"])
def test_bitwise_runs_batches_forward_and_absent_fields(env, normalized):
    ops = env["ops"]
    case = TC.Case("identity", K.ENTRY, "gauss4", 10, 17, 130, 0, (("normalized", normalized),))
    x = _dev(TC.layout(case, TC.rows_of(case))).requires_grad_(True)    # [T][C][B]
    w = G.upstream_of(case, "all")
    g, out = _grad(ops, x, normalized, w)
    g2, _ = _grad(ops, x, normalized, w)
    assert torch.equal(_bits(g), _bits(g2))                             # two runs
    # images 64..129 as a batch of their own: another grid, other neighbours, the same bits
    part = x.detach()[:, :, 64:].contiguous().requires_grad_(True)
    gp, _ = _grad(ops, part, normalized, {f: v[64:] for f, v in w.items()})
    assert gp.shape == (10, 17, 66) and torch.equal(_bits(gp), _bits(g[:, :, 64:]))
    # the forward outputs are those of the plain entry, whatever is asked for
    plain = ops.mc_uncertainty_cb(x.detach(), normalized=normalized)
    for f in G.FIELDS:
        assert getattr(out, f).grad_fn is not None and torch.equal(_bits(getattr(out, f)), _bits(getattr(plain, f))), f
    some = ops.mc_uncertainty_cb_autograd(x, normalized=normalized, want=("mutual_info", "pred"))
    assert [f for f, t in some._asdict().items() if t is not None] == ["pred", "mutual_info"]
    assert torch.equal(_bits(some.mutual_info), _bits(plain.mutual_info)) and torch.equal(_bits(some.pred), _bits(plain.pred))
    # a field left out = the field with a zero upstream gradient; every other image's zero weights change no bit of an image
    for f in ("epistemic", "entropy"):
        without = dict(w, **{f: None})
        zeroed = dict(w, **{f: np.zeros_like(w[f])})
        ga, _ = _grad(ops, x, normalized, without)
        gb, _ = _grad(ops, x, normalized, zeroed)
        assert torch.equal(_bits(ga), _bits(gb)) and not torch.equal(_bits(ga), _bits(g)), f
    galt, _ = _grad(ops, x, normalized, G.upstream_of(case, "all_alternate"))
    assert torch.equal(_bits(galt[:, :, 0::2]), _bits(g[:, :, 0::2])) and not galt[:, :, 1::2].any()
    # an output that received no gradient goes down as a null pointer: the same bits as asking for the others alone
    o7 = ops.mc_uncertainty_cb_autograd(x, normalized=normalized)
    g7, = torch.autograd.grad(o7.mutual_info.sum(), x)
    g1, _ = _grad(ops, x, normalized, G.upstream_of(case, "mutual_info"))
    assert torch.equal(_bits(g7), _bits(g1))


def test_limits_and_arguments_are_refused_by_name(env):
    ops, lib = env["ops"], env["lib"]
    x = torch.zeros((K.MAX_DRAWS + 1, 3, 4), device="cuda", requires_grad=True)
    with pytest.raises(lib.BBBHipError, match="too many draws"):
        ops.mc_uncertainty_cb_autograd(x)
    with pytest.raises(lib.BBBHipError, match="want must name"):
        ops.mc_uncertainty_cb_autograd(x[:2], want=("variance",))
    with pytest.raises(lib.BBBHipError, match="want must name"):
        ops.mc_uncertainty_cb_autograd(x[:2], want=())
    out = ops.mc_uncertainty_cb_autograd(x.detach()[:2])                # nothing requires a gradient: plain tensors
    assert all(t.grad_fn is None for t in out)


# ---------------------------------------------------------------- model level
X_BOUND = {"bbb": 2e-4, "lrt": 1e-3}             # what tests/test_gpu_input_grad.py holds the node's x.grad to


def _model(env, net_type, lt, cin, B=8, frozen=True):
    torch.manual_seed(3)
    net = env["zoo"].getModel(net_type, cin, 10, P.CONFIG_PRIORS, lt, "softplus").cuda().requires_grad_(not frozen)
    env["rng"].assign_stream_ids(net)
    return net, torch.rand(B, cin, 32, 32, device="cuda")


def _manual(env, net, x, T, seed, call0, score, normalized=False):
    """fast_train.mc_logits_autograd -> ops.mc_uncertainty_cb_autograd -> autograd.grad, on a fresh leaf."""
    xg = x.detach().clone().requires_grad_(True)
    logits_cb, _ = env["ft"].mc_logits_autograd(net, xg, T, seed, call0)
    s = getattr(env["ops"].mc_uncertainty_cb_autograd(logits_cb, normalized=normalized, want=(score,)), score)
    g, = torch.autograd.grad(s.sum(), xg)
    return s.detach(), g, logits_cb.detach()


@pytest.mark.parametrize("net_type,lt,cin,score,normalized", [("lenet", "bbb", 1, "mutual_info", False), ("lenet", "lrt", 1, "entropy", True),
                                                              ("3conv3fc", "bbb", 3, "expected_entropy", False),
                                                              ("3conv3fc", "lrt", 3, "mutual_info", False)])
def test_saliency_is_the_manual_composition_and_close_to_float64(env, net_type, lt, cin, score, normalized):
    ens, rng, unc, ft = env["ens"], env["rng"], env["unc"], env["ft"]
    net, x = _model(env, net_type, lt, cin)
    T, B = 5, 8
    x.requires_grad_(True)                                             # the caller's own leaf: its .grad stays untouched
    rng.manual_seed(1234, call=10)
    s, g = unc.saliency(net, x, T=T, score=score, normalized=normalized)
    assert ens.stats["path"] == "chwn-autograd" and rng.get_state() == (1234, 10 + T)
    assert s.shape == (B,) and g.shape == x.shape and s.grad_fn is None and g.grad_fn is None
    assert x.grad is None and all(p.grad is None for p in net.parameters())
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    s2, g2, logits_cb = _manual(env, net, x, T, 1234, 10, score, normalized)
    assert torch.equal(_bits(s), _bits(s2)) and torch.equal(_bits(g), _bits(g2))
    # float64: d score / d logits of the node's own logits from the contract's reference, fed through the same node
    rows = logits_cb.permute(0, 2, 1).cpu().numpy()
    w = {f: np.ones(B, np.float32) if f == score else None for f in G.FIELDS}
    g64, _ = G.reference(rows, normalized, w)
    xg = x.detach().clone().requires_grad_(True)
    logits2, _ = ft.mc_logits_autograd(net, xg, T, 1234, 10)
    assert torch.equal(_bits(logits2), _bits(logits_cb))
    want, = torch.autograd.grad(logits2, xg, grad_outputs=_dev(g64.transpose(0, 2, 1).astype(np.float32)))
    r = float((g.double() - want.double()).abs().max()) / float(want.double().abs().max())
    print("%s-%s %s%s: |saliency - node(float64 d score / d logits)| / max |want| = %.3e (bound %g)"
          % (net_type, lt, score, "-norm" if normalized else "", r, X_BOUND[lt]))
    assert r <= X_BOUND[lt], r


def test_trainable_weights_get_gradients_and_x_grad_keeps_its_bits(env):
    ens, rng, unc = env["ens"], env["rng"], env["unc"]
    net, x = _model(env, "lenet", "bbb", 1)
    rng.manual_seed(77, call=3)
    _, frozen = unc.saliency(net, x, T=5)
    net.requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    rng.manual_seed(77, call=3)
    out = unc.mc_uncertainty(net, xg, T=5, grad=True, want=("mutual_info",))
    assert ens.stats["path"] == "chwn-autograd" and rng.get_state() == (77, 8)
    assert out.mutual_info.grad_fn is not None and out.entropy is None and out.pred is None
    out.mutual_info.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert torch.equal(_bits(xg.grad), _bits(frozen))


def test_bf16_storage_route(env):
    ens, ops, rng, unc = env["ens"], env["ops"], env["rng"], env["unc"]
    net, x = _model(env, "3conv3fc", "bbb", 3, B=8)
    rng.manual_seed(5, call=1)
    with ops.use_config(bf16_input_grad=True):
        s, g = unc.saliency(net, x, T=5, precision="bf16")
    assert ens.stats["path"] == "chwn-autograd-bf16" and rng.get_state() == (5, 6)
    assert g.shape == x.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and bool(torch.isfinite(s).all())


class _Hidden(nn.Module):
    """A Bayesian layer inside a module with a forward of its own: ensemble.flat_children rejects the model."""

    def __init__(self):
        super().__init__()
        from layers import BBB_Linear
        self.fc = BBB_Linear(12, 5, bias=True, priors=P.CONFIG_PRIORS)

    def forward(self, x):
        return self.fc(x.flatten(1))


def test_off_the_fast_path_the_transposed_route_differentiates(env):
    ens, rng, unc = env["ens"], env["rng"], env["unc"]
    from layers import ModuleWrapper
    torch.manual_seed(4)
    net = ModuleWrapper()
    net.add_module("block", _Hidden())
    net = net.cuda().requires_grad_(False)
    rng.assign_stream_ids(net)
    x = torch.rand(8, 3, 2, 2, device="cuda")
    rng.manual_seed(8, call=2)
    s, g = unc.saliency(net, x, T=4, score="entropy")
    assert ens.stats["path"] == "loop" and rng.get_state() == (8, 6)
    assert g.shape == x.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    rng.manual_seed(8, call=2)
    plain = unc.mc_uncertainty(net, x, T=4)
    assert torch.allclose(s, plain.entropy, rtol=0, atol=1e-5)          # (the layers' autograd and inference launches: last bits)


def test_refusals_and_the_unchanged_inference_call(env):
    ens, lib, rng, unc = env["ens"], env["lib"], env["rng"], env["unc"]
    net, x = _model(env, "lenet", "bbb", 1)
    xg = x.clone().requires_grad_(True)
    with pytest.raises(lib.BBBHipError, match='gemm_mode="bf16x3"'):
        unc.mc_uncertainty(net, xg, T=3, precision="bf16x3", grad=True)
    with pytest.raises(lib.BBBHipError, match="do not require a gradient"):
        unc.mc_uncertainty(net, x, T=3, grad=True)                     # frozen weights, a batch without requires_grad
    with pytest.raises(lib.BBBHipError, match="score must be one of"):
        unc.saliency(net, x, score="epistemic")
    # grad=False: today's call, whatever requires a gradient -- and the same bits as before around the new calls
    rng.manual_seed(9, call=4)
    a = unc.mc_uncertainty(net, xg, T=3)
    assert ens.stats["path"] == "chwn" and all(t.grad_fn is None and not t.requires_grad for t in a)
    rng.manual_seed(9, call=4)
    b = unc.mc_uncertainty(net, x, T=3, grad=False, want=("entropy", "p_mean"))
    assert torch.equal(_bits(b.entropy), _bits(a.entropy)) and torch.equal(_bits(b.p_mean), _bits(a.p_mean)) and b.pred is None
    rng.manual_seed(9, call=4)
    c = unc.mc_uncertainty(net, xg, T=3, grad=True)
    assert ens.stats["path"] == "chwn-autograd" and all(t.grad_fn is not None for t in c)
