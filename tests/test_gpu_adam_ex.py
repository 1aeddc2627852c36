"""The clipped / decayed / guarded Adam step on the device (bbb_grad_sumsq, bbb_grad_norm_finish, bbb_adam_step_ex; FusedAdam's
weight_decay, max_grad_norm and skip_nonfinite), on the tiers of tests/adam_ex_contract.py: neutral arguments bit for bit against
bbb_adam_step over every geometry case; values against float64 inside bounds taken from the fp32 reference
(tests/test_adam_ex_cpu.py), never from the kernel; the device-step path bit for bit against the host path, eager and captured; the
norm against float64 at six gradient scales and bitwise the same whatever the alignment and the dealing of tensors to launches;
non-finite gradients against the class map of torch's clip_grad_norm_ + Adam; the skipped step; FusedAdam bit for bit against the
direct launches in the documented order; and the captured training step.  Needs an MI355X: -m gpu."""
import math

import numpy as np
import pytest
import torch

import adam_contract as A
import adam_ex_contract as X
import ref_port_torch as P

pytestmark = pytest.mark.gpu
F32 = np.float32
WORST = {}


@pytest.fixture(scope="module")
def env():
    import layers  # noqa: F401
    from bbb_hip import ops, _lib, train, rng, fast_train
    _lib.lib()
    yield {"ops": ops, "lib": _lib, "train": train, "rng": rng, "fast_train": fast_train}
    print("\ndevice, worst |out - float64| / (2^-23 M) per output (bound):",
          {k: "%.3f at %s (%d)" % (v[0], v[1], X.C_EX.get(k, 1)) for k, v in sorted(WORST.items())})


def _note(ratios, name):
    print("%s: %s" % (name, " ".join("%s %.3f" % kv for kv in ratios.items())))
    for k, x in ratios.items():
        if x > WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (x, name)


def _up(bufs):
    return [torch.from_numpy(np.array(b)).cuda() for b in bufs]


def _down(dev):
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in dev]


def _scalar(x):
    return torch.full((1,), float(x), dtype=torch.float32, device="cuda")


def _run_ex(env, lay, which, h, t, before=None, **kw):
    dev = _up(lay.host if before is None else before)
    assert X.launch_ex(env["lib"], A.device_segments(lay, dev, which), h, t, **kw) == 0
    return _down(dev)


def _results(lay, after, which):
    vals = lay.values(which, after)
    return vals[0], vals[2], vals[3]


# ---- 7. neutral = old, bit for bit ----

@pytest.mark.parametrize("case", A.GEOMETRY_CASES, ids=lambda c: c.name)
def test_neutral_arguments_are_the_old_entry_bit_for_bit(env, case):
    lay, which = A.geo_layout(case), A.geo_launched(case)
    dev = _up(lay.host)
    assert A.launch(env["lib"], A.device_segments(lay, dev, which), A.DEFAULT, A.GEOMETRY_T) == 0
    old = _down(dev)
    assert (A.bits(old[0]) != A.bits(lay.host[0])).any()
    A.check_buffers(lay, _run_ex(env, lay, which, A.DEFAULT, A.GEOMETRY_T), old, case.name + ": wd 0, no device scalars")
    one = _scalar(1.0)
    for kw in (dict(coef_dev=one.data_ptr(), ok_dev=one.data_ptr()), dict(coef_dev=one.data_ptr()), dict(ok_dev=one.data_ptr()),
               dict(decoupled=True, coef_dev=one.data_ptr(), ok_dev=one.data_ptr())):
        A.check_buffers(lay, _run_ex(env, lay, which, A.DEFAULT, A.GEOMETRY_T, **kw), old, case.name + ": %s" % sorted(kw))
    assert float(one) == 1.0


# ---- 8. values ----

@pytest.mark.parametrize("hyper", list(A.HYPERS))
def test_values_against_float64(env, hyper):
    h = A.HYPERS[hyper]
    coefs = {c: _scalar(c) for c in (1.0, 0.37)}
    for c in (c for c in A.VALUE_CASES if c.hyper == hyper):
        before = A.values_of(c)
        lay = A.Layout([(before, A.ALIGNED)])
        for decoupled in (False, True):
            ex = X.scalars_ex(h, c.t, 1e-2, decoupled)
            for coef, coef_dev in coefs.items():
                after = _run_ex(env, lay, [0], h, c.t, wd=1e-2, decoupled=decoupled, coef_dev=coef_dev.data_ptr())
                res = _results(lay, after, [0])
                A.check_geometry(lay, after, [0], res, name=c.name)          # sentinels and grad
                name = "%s-%s-coef%g" % (c.name, ex.mode, coef)
                _note(X.check_values_ex(before, res, ex, float(F32(coef)), name), name)


def test_six_chained_steps_with_clipping_engaged(env):
    """adam_contract's chain (gradients 10^(it - 3) N(0, 1), lr 3e-3, from zero moments), every step clipped to max_norm 1e-3 by the
    norm launches and decayed (L2, 1e-2); every launch is fed the device's previous outputs and held to the bound on its own."""
    h, mx = A.CHAIN_HYPER, 1e-3
    lay = A.Layout([(A.draw("chain-ex/%d" % s, n, moments="zero"), (s, 0, 0, s)) for s, n in enumerate(A.CHAIN_SIZES)])
    cur = [np.array(b) for b in lay.host]
    which = list(range(len(A.CHAIN_SIZES)))
    ex_of = lambda t: X.scalars_ex(h, t, 1e-2, False)
    for it in range(A.CHAIN_STEPS):
        grads = [A.chain_grad(it, n) for n in A.CHAIN_SIZES]
        for s, g in enumerate(grads):
            lay.seg(cur, 1, s)[:] = g
        dev = _up(cur)
        segs = A.device_segments(lay, dev, which)
        partials, scalars, skipped = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(3, device="cuda"), torch.zeros((), dtype=torch.int32, device="cuda")
        assert X.launch_norm(env["lib"], segs, partials, scalars, skipped, mx) == len(which)
        assert X.launch_ex(env["lib"], segs, h, it + 1, wd=1e-2, coef_dev=scalars.data_ptr() + 4) == 0
        after = _down(dev)
        norm, coef, ok = scalars.cpu().numpy()
        X.check_norm(norm, grads, "chain%d" % it)
        X.check_coef(coef, norm, mx)
        assert norm > mx and 0.0 < coef < 1.0 and ok == 1.0 and int(skipped) == 0
        before, res = lay.values(which, cur), _results(lay, after, which)
        A.check_geometry(lay, after, which, res, before=cur, name="chain%d" % it)
        _note(X.check_values_ex(before, res, ex_of(it + 1), float(coef), "chain%d" % it), "chain-step%d" % (it + 1))
        cur = after


# ---- 9. device path ----

@pytest.mark.parametrize("t", (1, 7, 100000))
def test_device_step_with_decoupled_decay_is_the_host_step_bit_for_bit(env, t):
    """step_dev holding t: the host launch at step t.  lr_dev holding float32(lr): the host launch given float(float32(lr)) -- step_size AND
    decay formed on the device from the device rate.  adam_ex_contract.DEVICE_DECAY pairs each rate with a decay at which the two
    roundings of lr give another fp32 decay where such a pair exists."""
    lay = A.Layout([(A.draw("dstep-ex", A.VALUE_N, 1e-2, pscale=1e-2), A.ALIGNED)])
    step_dev, coef = _scalar(t), _scalar(0.37)
    for lr in A.DEVICE_LRS:
        wd = X.DEVICE_DECAY[lr]
        h = A.DEFAULT._replace(lr=lr)
        through = A.lr_through_float(lr)
        kw = dict(wd=wd, decoupled=True, coef_dev=coef.data_ptr())
        host = _results(lay, _run_ex(env, lay, [0], h, t, **kw), [0])
        dev_step = _results(lay, _run_ex(env, lay, [0], h, 0, step_dev=step_dev.data_ptr(), **kw), [0])
        host_f = _results(lay, _run_ex(env, lay, [0], h._replace(lr=through), t, **kw), [0])
        lr_dev = _scalar(lr)
        dev_lr = _results(lay, _run_ex(env, lay, [0], h._replace(lr=12345.0), 0, step_dev=step_dev.data_ptr(), lr_dev=lr_dev.data_ptr(), **kw), [0])
        for what, pair in (("step_dev", (host, dev_step)), ("lr_dev", (host_f, dev_lr))):
            for k, (a, b) in enumerate(zip(*pair)):
                bad = np.flatnonzero(A.bits(a) != A.bits(b))
                assert bad.size == 0, (what, lr, t, k, bad[:4], a[bad[:4]], b[bad[:4]])
        _note(X.check_values_ex(lay.values([0]), host, X.scalars_ex(h, t, wd, True), 0.37, "dstep"), "dstep-lr%g-t%d" % (lr, t))
        same = X.scalars_ex(h, t, wd, True).decay == X.scalars_ex(h, t, wd, True, through).decay and \
            A.scalars(h, t).step_size == A.scalars(h, t, through).step_size
        assert (A.bits(host[0]) == A.bits(host_f[0])).all() == bool(same), (lr, t)


def test_captured_ex_step_replays_as_three_host_launches(env):
    """One bbb_adam_step_ex with step_dev, lr_dev, coef_dev and ok_dev in a captured graph, replayed at steps 5, 6, 7 with the rate changed
    before the third replay: bitwise the three host launches with float(float32(lr))."""
    lay = A.Layout([(A.draw("graph-ex/%d" % s, n, 1e-2, pscale=1e-2), off) for s, (n, off) in enumerate(((1029, A.ALIGNED), (3, A.ALIGNED), (515, (1, 0, 0, 0))))])
    which = [0, 1, 2]
    lrs = (1e-3, 1e-3, 0.1)
    dev = _up(lay.host)
    step_dev, lr_dev, coef, ok = _scalar(1), _scalar(lrs[0]), _scalar(0.37), _scalar(1.0)
    segs = A.device_segments(lay, dev, which)
    h = A.DEFAULT._replace(lr=777.0)                                  # the host rate of a launch with lr_dev is not read
    kw = dict(wd=7.0, decoupled=True, coef_dev=coef.data_ptr(), ok_dev=ok.data_ptr())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                     # warm-up on the side stream, on buffers of its own
        warm = _up(lay.host)
        assert X.launch_ex(env["lib"], A.device_segments(lay, warm, which), h, 0, step_dev=step_dev.data_ptr(), lr_dev=lr_dev.data_ptr(), **kw) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with env["ops"].graph_capture(g, side):
        assert X.launch_ex(env["lib"], segs, h, 0, step_dev=step_dev.data_ptr(), lr_dev=lr_dev.data_ptr(), **kw) == 0
    torch.cuda.synchronize()
    A.check_buffers(lay, _down(dev), lay.host, "capture runs nothing")
    cur = [np.array(b) for b in lay.host]
    for i, lr in enumerate(lrs):
        step_dev.fill_(5 + i)
        lr_dev.fill_(lr)
        g.replay()
        got = _down(dev)
        want = _run_ex(env, lay, which, A.DEFAULT._replace(lr=A.lr_through_float(lr)), 5 + i, before=cur, wd=7.0, decoupled=True, coef_dev=coef.data_ptr())
        A.check_buffers(lay, got, want, "replay %d" % (i + 1))
        assert (A.bits(got[0]) != A.bits(cur[0])).any()
        cur = got
    ok.fill_(0.0)                                                     # and a replay with ok = 0 stores nothing
    g.replay()
    A.check_buffers(lay, _down(dev), cur, "replay with ok = 0")


# ---- 10. norm ----

SENT = -7.0            # sentinel of the partials buffer


def _norm_run(env, grads, offs=None, deal=None, first=0, max_norm=math.inf, skip=False):
    """The norm launches over `grads` laid out with sentinels (gradient s `offs[s]` elements past a 16-byte boundary): (norm, coef, ok,
    skipped) as numpy scalars and the partials written.  Holds the gradient buffer and every sentinel -- the layout's and the
    partials' -- to be untouched."""
    offs = [0] * len(grads) if offs is None else offs
    z = lambda n: np.zeros(n, F32)
    lay = A.Layout([((z(len(g)), g, z(len(g)), z(len(g))), (0, o, 0, 0)) for g, o in zip(grads, offs)])
    dev = _up(lay.host)
    segs = [dict(n=s["n"], grad=s["grad"]) for s in A.device_segments(lay, dev)]
    count = sum(X.chunks_of(len(g)) for g in grads)
    partials = torch.full((first + count + 4,), SENT, dtype=torch.float64, device="cuda")
    scalars, skipped = torch.full((4,), SENT, device="cuda"), torch.zeros((2,), dtype=torch.int32, device="cuda")
    L = env["lib"].lib()
    stream = env["lib"].cur_stream(torch.device("cuda", torch.cuda.current_device()))
    at, f = 0, first
    for c in (deal or [A.MAX_SEGMENTS] * (-(-len(segs) // A.MAX_SEGMENTS))):
        part = segs[at:at + c]
        assert L.bbb_grad_sumsq(A.segment_array(env["lib"], part), len(part), partials.data_ptr(), f, stream) == 0
        f += sum(X.chunks_of(s["n"]) for s in part)
        at += len(part)
    assert at == len(segs) and f == first + count
    assert L.bbb_grad_norm_finish(partials.data_ptr() + 8 * first, count, float(max_norm), int(skip), scalars.data_ptr(), scalars.data_ptr() + 4,
                                  scalars.data_ptr() + 8, skipped.data_ptr(), stream) == 0
    A.check_buffers(lay, _down(dev), lay.host, "the norm launches write no segment array")
    parts, sc, sk = partials.cpu().numpy(), scalars.cpu().numpy(), skipped.cpu().numpy()
    assert (parts[:first] == SENT).all() and (parts[first + count:] == SENT).all() and sc[3] == SENT and sk[1] == 0
    return sc[0], sc[1], sc[2], int(sk[0]), parts[first:first + count]


def _same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("scale", X.NORM_SCALES)
def test_norm_is_range_free(env, scale):
    for name, sizes in (("n1537", (A.VALUE_N,)), ("sixteen", A.SIXTEEN_N)):
        grads = [X.norm_grad("%s/%g/%d" % (name, scale, s), n, scale) for s, n in enumerate(sizes)]
        norm, coef, ok, skipped, _ = _norm_run(env, grads, max_norm=1.0)
        r = X.check_norm(norm, grads, "%s at %g" % (name, scale))
        X.check_coef(coef, norm, 1.0)
        assert np.isfinite(norm) and norm > 0 and ok == 1.0 and skipped == 0
        _note({"norm": r}, "%s at %g" % (name, scale))


def test_norm_does_not_depend_on_alignment_dealing_or_the_run(env):
    grads = [X.norm_grad("align/%d" % s, n) for s, n in enumerate((4097, 6, 1029, 8200))]
    ref = _norm_run(env, grads)
    X.check_norm(ref[0], grads, "aligned")
    assert ref[1] == 1.0                                                      # max_norm = +inf: norm only
    for d in (1, 2, 3):
        got = _norm_run(env, grads, offs=[d] * 4)
        assert _same_bits(got[0], ref[0]) and _same_bits(got[4], ref[4]), d
    assert _same_bits(_norm_run(env, grads, offs=[0, 3, 1, 2], first=5)[4], ref[4])
    for count, deals in ((17, ([16, 1], [1, 16], [5, 5, 7])), (33, ([16, 16, 1], [1, 16, 16], [16, 1, 16]))):
        grads = [X.norm_grad("deal%d/%d" % (count, s), n) for s, n in enumerate(A.FUSED_SIZES[count])]
        runs = [_norm_run(env, grads, deal=d, max_norm=0.5) for d in deals] + [_norm_run(env, grads, deal=deals[0], max_norm=0.5)]
        X.check_norm(runs[0][0], grads, "fused%d" % count)
        X.check_coef(runs[0][1], runs[0][0], 0.5)
        assert runs[0][1] < 1.0
        for r in runs[1:]:
            assert _same_bits(r[0], runs[0][0]) and _same_bits(r[1], runs[0][1]) and _same_bits(r[4], runs[0][4])


@pytest.mark.parametrize("n", X.NORM_SINGLE_N)
def test_norm_of_a_single_tensor_around_the_chunk(env, n):
    g = X.norm_grad("single%d" % n, n)
    for off in (0, 1):
        norm, _, _, _, parts = _norm_run(env, [g], offs=[off])
        X.check_norm(norm, [g], "n = %d" % n)
        assert len(parts) == X.chunks_of(n)
        want = [math.fsum((g[i:i + X.NORM_CHUNK].astype(np.float64) ** 2).tolist()) for i in range(0, n, X.NORM_CHUNK)]
        np.testing.assert_allclose(parts, want, rtol=4096 * 2.0 ** -53, atol=0)


# ---- 11. classes ----

def _clipped_launch(env, bad, h, t, wd, mx):
    lay = A.Layout([(bad, A.ALIGNED)])
    dev = _up(lay.host)
    segs = A.device_segments(lay, dev)
    partials, scalars, skipped = torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(3, device="cuda"), torch.zeros((), dtype=torch.int32, device="cuda")
    X.launch_norm(env["lib"], segs, partials, scalars, skipped, mx)
    assert X.launch_ex(env["lib"], segs, h, t, wd=wd, coef_dev=scalars.data_ptr() + 4) == 0
    after = _down(dev)
    res = _results(lay, after, [0])
    A.check_geometry(lay, after, [0], res, name="classes")                    # sentinels and grad
    return res, scalars.cpu().numpy()


@pytest.mark.parametrize("at", A.POISON_AT)
def test_a_nan_gradient_gives_a_nan_norm_and_torchs_outputs(env, at):
    t, h, mx = 7, A.DEFAULT, 5.0
    bad = [np.array(a) for a in A.draw("cls-ex", A.POISON_N, 1.0)]
    bad[1][at] = np.nan
    got, (norm, coef, ok) = _clipped_launch(env, bad, h, t, 1e-2, mx)
    assert np.isnan(norm) and np.isnan(coef) and ok == 1.0                    # (no skip asked for)
    want = X.torch_clipped_adam([bad], h, t, 1e-2, False, mx)[0]
    X.check_all_classes(got, want, "NaN at %d" % at)
    assert np.isnan(got[0]).all()


@pytest.mark.parametrize("x", [np.inf, -np.inf])
def test_an_inf_gradient_gives_an_inf_norm_a_zero_coefficient_and_torchs_classes(env, x):
    t, h, mx = 7, A.DEFAULT, 5.0
    clean = A.draw("cls-ex", A.POISON_N, 1.0)
    assert np.abs(clean[1]).max() <= 1e3
    bad = A.poisoned(clean, "grad", x)
    got, (norm, coef, ok) = _clipped_launch(env, bad, h, t, 1e-2, mx)
    assert norm == np.inf and coef == 0.0 and ok == 1.0
    want = X.torch_clipped_adam([bad], h, t, 1e-2, False, mx)[0]
    X.check_all_classes(got, want, "%r" % x)
    assert int(np.isnan(got[1]).sum()) == len(A.POISON_AT)


# ---- 12, 13. FusedAdam ----

def _fused_layout(name, sizes):
    return A.Layout([(A.draw("%s/%d" % (name, s), n), (int(s % 5 == 3), 0, int(s % 7 == 2), 0)) for s, n in enumerate(sizes)])


GROUP0 = 5            # tensors of the first group
GROUP_DECAY = ((1e-2, False), (0.3, True))


def _fused(env, lay, dev, t_before, grads, h, capturable=False, **kw):
    """A FusedAdam of two groups (the first GROUP0 tensors L2 1e-2, the others decoupled 0.3) over views of the layout's device buffers,
    with loaded state."""
    view = lambda k, s: dev[k][lay.start[k][s]:lay.start[k][s] + lay.n[s]]
    params = [view(0, s) for s in range(len(lay.n))]
    groups = [dict(params=params[:GROUP0], weight_decay=GROUP_DECAY[0][0], decoupled_weight_decay=GROUP_DECAY[0][1]),
              dict(params=params[GROUP0:], weight_decay=GROUP_DECAY[1][0], decoupled_weight_decay=GROUP_DECAY[1][1])]
    opt = env["train"].FusedAdam(groups, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, capturable=capturable, **kw)
    cap = opt.param_groups[0]["capturable"]
    for s, p in enumerate(params):
        opt.state[p] = {"step": torch.tensor(float(t_before), device="cuda" if cap else "cpu"), "exp_avg": view(2, s), "exp_avg_sq": view(3, s)}
        p.grad = view(1, s) if s in grads else None
    return opt, params


def _direct(env, lay, dev, which, h, t, max_norm):
    """The documented launch order on caller-made views: sumsq over every gradient in param_groups order in launches of 16, ONE finish,
    then per group the Adam launches of 16.  Returns (norm, coef)."""
    segs = A.device_segments(lay, dev, which)
    partials = torch.zeros(sum(X.chunks_of(s["n"]) for s in segs), dtype=torch.float64, device="cuda")
    scalars, skipped = torch.zeros(3, device="cuda"), torch.zeros((), dtype=torch.int32, device="cuda")
    X.launch_norm(env["lib"], segs, partials, scalars, skipped, max_norm)
    for (wd, decoupled), members in zip(GROUP_DECAY, ([s for s in which if s < GROUP0], [s for s in which if s >= GROUP0])):
        for i in range(0, len(members), A.MAX_SEGMENTS):
            assert X.launch_ex(env["lib"], A.device_segments(lay, dev, members[i:i + A.MAX_SEGMENTS]), h, t, wd=wd, decoupled=decoupled,
                               coef_dev=scalars.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    return scalars.cpu().numpy()[:2]


@pytest.mark.parametrize("max_norm,clipped", [(0.05, True), (1e9, False)])
@pytest.mark.parametrize("name", ["17", "33", "nograd"])
def test_fused_adam_is_the_direct_launches_in_the_documented_order(env, name, max_norm, clipped):
    sizes, none = {"17": (A.FUSED_SIZES[17], ()), "33": (A.FUSED_SIZES[33], ()), "nograd": (A.FUSED_NO_GRAD_SIZES, A.FUSED_NO_GRAD)}[name]
    lay = _fused_layout("fused-ex" + name, sizes)
    which = [s for s in range(len(sizes)) if s not in none]
    assert len(which) > A.MAX_SEGMENTS and any(s < GROUP0 for s in none) == bool(none)
    h = A.HYPERS["lr3e-3"]
    dev = _up(lay.host)
    opt, params = _fused(env, lay, dev, 6, set(which), h, max_grad_norm=max_norm)
    assert opt.grad_norm is None
    opt.step()
    after = _down(dev)
    ref = _up(lay.host)
    norm, coef = _direct(env, lay, ref, which, h, 7, max_norm)
    A.check_buffers(lay, after, _down(ref), "fused-ex" + name)                 # all four buffers whole: p.grad bitwise as before, too
    assert (A.bits(after[1]) == A.bits(lay.host[1])).all() and (A.bits(after[0]) != A.bits(lay.host[0])).any()
    assert _same_bits(opt.grad_norm.cpu().numpy(), norm) and _same_bits(opt.clip_coef.cpu().numpy(), coef)
    grads = [lay.seg(lay.host, 1, s) for s in which]
    X.check_norm(norm, grads, name)
    X.check_coef(coef, norm, max_norm)
    assert _same_bits(env["train"].grad_norm([p for p in params if p.grad is not None]).cpu().numpy(), norm)
    assert _same_bits(env["train"].grad_norm([p.grad for p in params if p.grad is not None]).cpu().numpy(), norm)
    if clipped:
        assert float(opt.grad_norm) > opt.max_grad_norm and float(opt.clip_coef) < 1.0
    else:
        assert float(opt.clip_coef) == 1.0
    assert [int(opt.state[p]["step"]) for p in params] == [7 if s in which else 6 for s in range(len(sizes))]
    assert int(opt.skipped_steps) == 0
    # and each tensor is inside the value bound of its group
    for s in which[:3] + which[-3:]:
        wd, decoupled = GROUP_DECAY[s >= GROUP0]
        before = tuple(lay.seg(lay.host, k, s) for k in range(4))
        res = tuple(lay.seg(after, k, s) for k in (0, 2, 3))
        _note(X.check_values_ex(before, res, X.scalars_ex(h, 7, wd, decoupled), float(coef), "fused"), "fused-ex%s/%d" % (name, s))


def test_weight_decay_alone_launches_no_norm(env):
    """weight_decay without max_grad_norm / skip_nonfinite: the extended entry with no device scalar, no norm buffers."""
    sizes = A.FUSED_SIZES[17]
    lay = _fused_layout("wd-only", sizes)
    which = list(range(len(sizes)))
    h = A.HYPERS["lr3e-3"]
    dev = _up(lay.host)
    opt, params = _fused(env, lay, dev, 6, set(which), h)
    opt.step()
    after = _down(dev)
    assert opt.grad_norm is None and opt._norm is None
    ref = _up(lay.host)
    for (wd, decoupled), members in zip(GROUP_DECAY, (which[:GROUP0], which[GROUP0:])):
        assert X.launch_ex(env["lib"], A.device_segments(lay, ref, members), h, 7, wd=wd, decoupled=decoupled) == 0
    A.check_buffers(lay, after, _down(ref), "wd-only")


def test_a_nonfinite_step_is_skipped_and_the_next_one_is_clean(env):
    """17 tensors, one NaN in the last one's gradient, skip_nonfinite: parameters, moments and device step counts stay bit for bit and
    skipped_steps is 1; the next clean step equals the step a never-poisoned optimizer takes at the same count."""
    sizes = A.FUSED_SIZES[17]
    lay = _fused_layout("skip", sizes)
    which = list(range(len(sizes)))
    h = A.HYPERS["lr3e-3"]
    dev = _up(lay.host)
    opt, params = _fused(env, lay, dev, 6, set(which), h, max_grad_norm=0.05, skip_nonfinite=True)
    assert all(g["capturable"] for g in opt.param_groups) and all(opt.state[p]["step"].is_cuda for p in params)
    at = lay.start[1][16] + lay.n[16] - 1
    clean = dev[1][at].clone()
    dev[1][at] = float("nan")
    poisoned = _down(dev)
    opt.step()
    A.check_buffers(lay, _down(dev), poisoned, "skipped step")
    assert [float(opt.state[p]["step"]) for p in params] == [6.0] * len(sizes)
    assert int(opt.skipped_steps) == 1 and np.isnan(float(opt.grad_norm)) and np.isnan(float(opt.clip_coef))
    dev[1][at] = clean
    opt.step()
    after = _down(dev)
    assert [float(opt.state[p]["step"]) for p in params] == [7.0] * len(sizes) and int(opt.skipped_steps) == 1
    ref = _up(lay.host)
    twin, twin_params = _fused(env, lay, ref, 6, set(which), h, max_grad_norm=0.05, skip_nonfinite=True)
    twin.step()
    A.check_buffers(lay, after, _down(ref), "the step after a skipped one")
    assert int(twin.skipped_steps) == 0 and _same_bits(twin.grad_norm.cpu().numpy(), opt.grad_norm.cpu().numpy())
    assert (A.bits(after[0]) != A.bits(lay.host[0])).any()
    # +Inf is skipped too
    dev[1][at] = float("inf")
    before = _down(dev)
    opt.step()
    A.check_buffers(lay, _down(dev), before, "skipped step (Inf)")
    assert int(opt.skipped_steps) == 2 and float(opt.grad_norm) == math.inf


# ---- 14. captured training ----

def _small_net():
    from layers import BBB_Conv2d, BBB_Linear, FlattenLayer, ModuleWrapper
    net = ModuleWrapper()
    net.add_module("c1", BBB_Conv2d(3, 8, 3, padding=1, bias=True, priors=P.CONFIG_PRIORS))
    net.add_module("a1", torch.nn.ReLU())
    net.add_module("p1", torch.nn.MaxPool2d(2, 2))
    net.add_module("fl", FlattenLayer(8 * 4 * 4))
    net.add_module("f1", BBB_Linear(8 * 4 * 4, 10, bias=True, priors=P.CONFIG_PRIORS))
    return net.cuda()


def test_captured_training_step_clips_like_the_eager_one(env):
    T = env["train"]
    B, E, lr, beta, n = 8, 2, 1e-3, 0.1, 1000.0
    torch.manual_seed(3)
    x = torch.rand(B, 3, 8, 8, device="cuda")
    y = torch.randint(0, 10, (B,), device="cuda")

    def fresh(**kw):
        torch.manual_seed(11)
        net = _small_net()
        env["rng"].assign_stream_ids(net)
        env["rng"].manual_seed(77, call=0)
        return net, T.FusedAdam(net.parameters(), lr=lr, weight_decay=1e-2, **kw)

    net0, opt0 = fresh(max_grad_norm=1e30)
    assert env["fast_train"].train_path_ok(net0, x) == "bbb"
    T.train_step(net0, opt0, x, y, E, beta, n, graph=False)
    first_norm = float(opt0.grad_norm)
    mx = 0.25 * first_norm                                                    # below the first step's measured norm
    assert np.isfinite(first_norm) and first_norm > 0

    def run(graph):
        net, opt = fresh(max_grad_norm=mx, skip_nonfinite=True)
        losses, norms, captured = [], [], []
        for it in range(6):
            losses.append(T.train_step(net, opt, x, y, E, beta, n, graph=graph)[0].item())
            norms.append(float(opt.grad_norm))
            st = T._auto.get(net)
            captured.append(bool(st and st["graphed"] is not None))
        return net, opt, losses, norms, captured

    net_e, opt_e, eager, norms_e, cap_e = run(False)
    net_g, opt_g, auto, norms_g, cap_g = run(None)
    assert not any(cap_e) and cap_g == [False] * 3 + [True] * 3
    np.testing.assert_allclose(norms_e[0], first_norm, rtol=1e-6)
    assert all(v > mx for v in norms_e) and float(opt_e.clip_coef) < 1.0      # the clip is engaged at every step
    np.testing.assert_allclose(auto, eager, rtol=2e-5)
    np.testing.assert_allclose(norms_g, norms_e, rtol=2e-5)                   # the replays follow opt.grad_norm step by step
    for (na, a), (nb, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        np.testing.assert_allclose(b.detach().cpu().numpy(), a.detach().cpu().numpy(), rtol=2e-5, atol=1e-7, err_msg=na)
    assert float(opt_g.state[next(iter(net_g.parameters()))]["step"].item()) == 6.0 and int(opt_g.skipped_steps) == 0
    # an explicit GraphedTrainStep: every replay leaves that step's norm in opt.grad_norm
    net_s, opt_s = fresh(max_grad_norm=mx, skip_nonfinite=True)
    g = T.GraphedTrainStep(net_s, opt_s, x, y, E, beta, n, warmup=3)
    seen = []
    for _ in range(3):
        g.step()
        seen.append(float(opt_s.grad_norm))
    np.testing.assert_allclose(seen, norms_e[3:], rtol=2e-5)
    assert len(set(seen)) == 3
    # changing max_grad_norm after the capture drops the graph; the next result is the eager one
    opt_g.max_grad_norm = opt_e.max_grad_norm = 4.0 * mx
    env["rng"].manual_seed(77, call=6 * E)                                    # both take their seventh step on the same noise
    le = T.train_step(net_e, opt_e, x, y, E, beta, n, graph=False)[0].item()
    env["rng"].manual_seed(77, call=6 * E)
    lg = T.train_step(net_g, opt_g, x, y, E, beta, n)[0].item()
    assert T._auto[net_g]["graphed"] is None
    np.testing.assert_allclose(lg, le, rtol=2e-5)
    np.testing.assert_allclose(float(opt_g.clip_coef), float(opt_e.clip_coef), rtol=2e-5)
    for (na, a), (nb, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        np.testing.assert_allclose(b.detach().cpu().numpy(), a.detach().cpu().numpy(), rtol=2e-5, atol=1e-7, err_msg=na)
