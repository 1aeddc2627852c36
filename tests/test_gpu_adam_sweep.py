"""The multi-tensor Adam step (bbb_adam_step, csrc/adam.hip) launch by launch, on the tiers of tests/adam_contract.py: geometry bit for
bit against one aligned single-segment launch over the same values, with sentinels around all four arrays; values against float64
inside bounds taken from the fp32 reference (tests/test_adam_sweep_cpu.py), never from the kernel; the device-step path bit for bit
against the host path, eager and in a captured graph; non-finite and overflowing operands against the class map of torch's CPU fp32
Adam, with every element the poison does not reach bitwise the clean launch's; and every refusal.  The launches go through ctypes on
caller-made views (adam_contract.launch), or through FusedAdam where its grouping is the subject.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest
import torch

import adam_contract as A

pytestmark = pytest.mark.gpu
F32 = np.float32
WORST = {}


@pytest.fixture(scope="module")
def env():
    from bbb_hip import ops, _lib, train
    _lib.lib()
    yield {"ops": ops, "lib": _lib, "train": train}
    print("\ndevice, worst |out - float64| / (2^-23 M) per output (bound):",
          {k: "%.3f at %s (%d)" % (v[0], v[1], A.C[k]) for k, v in sorted(WORST.items())})


def _note(ratios, name):
    """Print the figures, keep the worst; check_values has held them to the bound."""
    print("%s: m %.3f v %.3f p %.3f" % (name, ratios["m"], ratios["v"], ratios["p"]))
    for k, x in ratios.items():
        if x > WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (x, name)


def _up(bufs):
    return [torch.from_numpy(np.array(b)).cuda() for b in bufs]


def _down(dev):
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in dev]


def _run(env, lay, which, h, t, before=None, **kw):
    """Upload the layout's buffers, one launch of the segments `which`, download: the four buffers afterwards."""
    dev = _up(lay.host if before is None else before)
    assert A.launch(env["lib"], A.device_segments(lay, dev, which), h, t, **kw) == 0
    return _down(dev)


def _results(lay, after, which):
    vals = lay.values(which, after)
    return vals[0], vals[2], vals[3]


def _bit_reference(env, values, h, t, name):
    """(p', m', v') of ONE aligned single-segment launch over `values`: sentinels and grad intact, and itself inside the value bound."""
    one = A.Layout([(values, A.ALIGNED)])
    after = _run(env, one, [0], h, t)
    res = _results(one, after, [0])
    A.check_geometry(one, after, [0], res, name=name + " (bit reference)")
    if all(np.isfinite(a).all() for a in values):
        _note(A.check_values(values, res, A.scalars(h, t), name), name + " (bit reference)")
    return res


# ---- geometry ----

@pytest.mark.parametrize("case", A.GEOMETRY_CASES, ids=lambda c: c.name)
def test_geometry(env, case):
    lay, which = A.geo_layout(case), A.geo_launched(case)
    after = _run(env, lay, which, A.DEFAULT, A.GEOMETRY_T)
    ref = _bit_reference(env, lay.values(which), A.DEFAULT, A.GEOMETRY_T, case.name)
    A.check_geometry(lay, after, which, ref, name=case.name)


def _fused(env, lay, dev, steps_before, grads, h, capturable=False):
    """A FusedAdam over views of the layout's device buffers, with loaded state ('step' = steps_before[s], on the device for a
    capturable group); grads: the segments that have a gradient."""
    params = [dev[0][lay.start[0][s]:lay.start[0][s] + n] for s, n in enumerate(lay.n)]
    opt = env["train"].FusedAdam(params, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, capturable=capturable)
    for s, p in enumerate(params):
        opt.state[p] = {"step": torch.tensor(float(steps_before[s]), device="cuda" if capturable else "cpu"),
                        "exp_avg": dev[2][lay.start[2][s]:lay.start[2][s] + lay.n[s]],
                        "exp_avg_sq": dev[3][lay.start[3][s]:lay.start[3][s] + lay.n[s]]}
        p.grad = dev[1][lay.start[1][s]:lay.start[1][s] + lay.n[s]] if s in grads else None
    return opt, params


def _fused_layout(name, sizes):
    return A.Layout([(A.draw("%s/%d" % (name, s), n), (int(s % 5 == 3), 0, int(s % 7 == 2), 0)) for s, n in enumerate(sizes)])


@pytest.mark.parametrize("count", [17, 33])
def test_fused_adam_splits_more_than_16_tensors_into_launches(env, count):
    """Every tensor has a gradient: two and three launches (16 + 1, 16 + 16 + 1)."""
    sizes = A.FUSED_SIZES[count]
    assert A.fused_launches(sizes) == {17: 2, 33: 3}[count]
    lay = _fused_layout("fused%d" % count, sizes)
    which = list(range(count))
    dev = _up(lay.host)
    opt, params = _fused(env, lay, dev, [6] * count, set(which), A.HYPERS["lr3e-3"])
    opt.step()
    after = _down(dev)
    ref = _bit_reference(env, lay.values(which), A.HYPERS["lr3e-3"], 7, "fused%d" % count)
    A.check_geometry(lay, after, which, ref, name="fused%d" % count)
    assert [int(opt.state[p]["step"]) for p in params] == [7] * count


def test_fused_adam_leaves_parameters_without_a_gradient(env):
    """21 tensors, four of them with grad None: they, their moments and their 'step' stay untouched; the 17 others still take two
    launches, the second starting behind a tensor that was dropped."""
    sizes, none = A.FUSED_NO_GRAD_SIZES, A.FUSED_NO_GRAD
    assert A.fused_launches(sizes, none) == 2
    lay = _fused_layout("nograd", sizes)
    which = [s for s in range(len(sizes)) if s not in none]
    dev = _up(lay.host)
    opt, params = _fused(env, lay, dev, [6] * len(sizes), set(which), A.HYPERS["lr3e-3"])
    opt.step()
    after = _down(dev)
    ref = _bit_reference(env, lay.values(which), A.HYPERS["lr3e-3"], 7, "nograd")
    A.check_geometry(lay, after, which, ref, name="nograd")
    assert [int(opt.state[p]["step"]) for p in params] == [7 if s in which else 6 for s in range(len(sizes))]


def test_capturable_fused_adam_is_the_host_launch_given_the_rate_as_a_float(env):
    """A capturable group keeps 'step' and the rate on the device: its step is bitwise the host launch at that step given
    float(float32(lr)) -- at (lr = 1e-3, t = 7) one ulp of step_size away from the launch given lr, which a non-capturable group makes."""
    h = A.DEFAULT._replace(lr=A.FUSED_CAPTURABLE_LR)
    t = A.FUSED_CAPTURABLE_T
    lay = A.Layout([(A.draw("capturable/%d" % s, n, 1e-2, pscale=1e-2), A.ALIGNED) for s, n in enumerate(A.FUSED_CAPTURABLE_SIZES)])
    which = list(range(len(lay.n)))
    dev = _up(lay.host)
    opt, params = _fused(env, lay, dev, [t - 1] * len(which), set(which), h, capturable=True)
    opt.step()
    after = _down(dev)
    assert [float(opt.state[p]["step"]) for p in params] == [float(t)] * len(which) and all(opt.state[p]["step"].is_cuda for p in params)
    through = _bit_reference(env, lay.values(which), h._replace(lr=A.lr_through_float(h.lr)), t, "capturable")
    A.check_geometry(lay, after, which, through, name="capturable")
    plain = _bit_reference(env, lay.values(which), h, t, "capturable, host rate")
    assert (A.bits(plain[0]) != A.bits(through[0])).any() and all((A.bits(a) == A.bits(b)).all() for a, b in zip(plain[1:], through[1:]))
    # and the non-capturable group on the same values is the launch given lr itself
    dev = _up(lay.host)
    opt, params = _fused(env, lay, dev, [t - 1] * len(which), set(which), h)
    opt.step()
    A.check_geometry(lay, _down(dev), which, plain, name="non-capturable")


def test_fused_adam_gives_each_step_count_its_own_bias_correction(env):
    """One non-capturable group whose tensors sit at different 'step' values: one launch per step count, each tensor bitwise what a
    single launch at ITS step gives."""
    steps = A.FUSED_STEPS
    lay = A.Layout([(A.draw("bystep/%d" % s, 300 + 41 * s), A.ALIGNED) for s in range(len(steps))])
    dev = _up(lay.host)
    opt, params = _fused(env, lay, dev, [t - 1 for t in steps], set(range(len(steps))), A.DEFAULT)
    opt.step()
    after = _down(dev)
    want = None
    for t in sorted(set(steps)):
        which = [s for s, x in enumerate(steps) if x == t]
        want = lay.expected(which, _bit_reference(env, lay.values(which), A.DEFAULT, t, "bystep-t%d" % t), want)
    A.check_buffers(lay, after, want, "bystep")
    assert [int(opt.state[p]["step"]) for p in params] == list(steps)
    # (the corrections do differ: the tensors at step 1 and at step 1000 would not survive each other's)
    one = A.scalars(A.DEFAULT, 1)
    assert one.step_size != A.scalars(A.DEFAULT, 1000).step_size and one.sqrt_bc2 != A.scalars(A.DEFAULT, 1000).sqrt_bc2


# ---- values ----

@pytest.mark.parametrize("hyper", list(A.HYPERS))
def test_values_against_float64(env, hyper):
    h = A.HYPERS[hyper]
    for c in (c for c in A.VALUE_CASES if c.hyper == hyper):
        before = A.values_of(c)
        lay = A.Layout([(before, A.ALIGNED)])
        after = _run(env, lay, [0], h, c.t)
        res = _results(lay, after, [0])
        A.check_geometry(lay, after, [0], res, name=c.name)          # sentinels and grad
        _note(A.check_values(before, res, A.scalars(h, c.t), c.name), c.name)


def test_lr_zero_moves_the_moments_only(env):
    before = A.draw("lr0", 1029)
    h = A.DEFAULT._replace(lr=0.0)
    lay = A.Layout([(before, A.ALIGNED)])
    p1, m1, v1 = _results(lay, _run(env, lay, [0], h, 7), [0])
    assert (A.bits(p1) == A.bits(before[0])).all()
    assert (m1 != before[2]).mean() > 0.99 and (v1 != before[3]).mean() > 0.99
    _note(A.check_values(before, (p1, m1, v1), A.scalars(h, 7), "lr=0"), "lr=0")


@pytest.mark.parametrize("t", [1, 1000])
def test_all_zero_gradient_and_moments_leave_the_parameter(env, t):
    n = 1029
    p = A.draw("zeros", n)[0]
    p[:3] = (0.0, -0.0, 1e-38)
    before = (p, np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32))
    lay = A.Layout([(before, A.ALIGNED)])
    p1, m1, v1 = _results(lay, _run(env, lay, [0], A.DEFAULT, t), [0])
    assert (A.bits(p1) == A.bits(p)).all()
    assert (A.bits(m1) == 0).all() and (A.bits(v1) == 0).all()


def test_six_chained_steps_launch_by_launch(env):
    """The scales of test_fused_adam_matches_torch_adam (gradients 10^(it - 3) N(0, 1), lr 3e-3, from zero moments); every launch is
    fed the device's previous outputs and held to the bound on its own."""
    h = A.CHAIN_HYPER
    lay = A.Layout([(A.draw("chain/%d" % s, n, moments="zero"), (s, 0, 0, s)) for s, n in enumerate(A.CHAIN_SIZES)])
    cur = [np.array(b) for b in lay.host]
    which = list(range(len(A.CHAIN_SIZES)))
    for it in range(A.CHAIN_STEPS):
        for s, n in enumerate(A.CHAIN_SIZES):
            lay.seg(cur, 1, s)[:] = A.chain_grad(it, n)
        after = _run(env, lay, which, h, it + 1, before=cur)
        before, res = lay.values(which, cur), _results(lay, after, which)
        A.check_geometry(lay, after, which, res, before=cur, name="chain%d" % it)
        _note(A.check_values(before, res, A.scalars(h, it + 1), "chain%d" % it), "chain-step%d" % (it + 1))
        cur = after


# ---- device step ----

def _scalar(x):
    return torch.full((1,), float(x), dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("t", A.T_VALUES)
def test_device_step_is_the_host_step_bit_for_bit(env, t):
    """step_dev holding t: the host launch with step = t.  lr_dev holding float32(lr): the host launch given float(float32(lr)) -- what a
    captured step is held to.  Where that is another fp32 step_size than lr's own (adam_contract.scalars), the two host launches differ."""
    lay = A.Layout([(A.draw("dstep", A.VALUE_N, 1e-2, pscale=1e-2), A.ALIGNED)])
    step_dev = _scalar(t)
    assert float(step_dev) == t
    for lr in A.DEVICE_LRS:
        h = A.DEFAULT._replace(lr=lr)
        through = A.lr_through_float(lr)
        host = _results(lay, _run(env, lay, [0], h, t), [0])
        dev_step = _results(lay, _run(env, lay, [0], h, 0, step_dev=step_dev.data_ptr()), [0])
        for k, (a, b) in enumerate(zip(host, dev_step)):
            bad = np.flatnonzero(A.bits(a) != A.bits(b))
            assert bad.size == 0, ("step_dev", lr, t, k, bad[:4], a[bad[:4]], b[bad[:4]])
        host_f = _results(lay, _run(env, lay, [0], h._replace(lr=through), t), [0])
        lr_dev = _scalar(lr)
        assert float(lr_dev) == through
        dev_lr = _results(lay, _run(env, lay, [0], h._replace(lr=12345.0), 0, step_dev=step_dev.data_ptr(), lr_dev=lr_dev.data_ptr()), [0])
        for k, (a, b) in enumerate(zip(host_f, dev_lr)):
            bad = np.flatnonzero(A.bits(a) != A.bits(b))
            assert bad.size == 0, ("lr_dev", lr, t, k, bad[:4], a[bad[:4]], b[bad[:4]])
        same = A.scalars(h, t).step_size == A.scalars(h, t, through).step_size
        print("t %d lr %g: step_size of lr %r, of float(float32(lr)) %r" % (t, lr, float(A.scalars(h, t).step_size), float(A.scalars(h, t, through).step_size)))
        assert (A.bits(host[0]) == A.bits(host_f[0])).all() == bool(same), (lr, t)
        for k in (1, 2):
            assert (A.bits(host[k]) == A.bits(host_f[k])).all()


def test_captured_step_replays_as_three_host_launches(env):
    """One bbb_adam_step with step_dev and lr_dev in a captured graph, replayed three times with the counter advanced and the rate
    changed before the third replay: bitwise the three host launches at steps 5, 6, 7 with float(float32(lr))."""
    lay = A.Layout([(A.draw("graph/%d" % s, n, 1e-2, pscale=1e-2), off) for s, (n, off) in enumerate(((1029, A.ALIGNED), (3, A.ALIGNED), (515, (1, 0, 0, 0))))])
    which = [0, 1, 2]
    lrs = (1e-3, 1e-3, 0.1)
    dev = _up(lay.host)
    step_dev, lr_dev = _scalar(1), _scalar(lrs[0])
    segs = A.device_segments(lay, dev, which)
    h = A.DEFAULT._replace(lr=777.0)                                  # the host rate of a launch with lr_dev is not read
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                     # warm-up on the side stream, on buffers of its own
        warm = _up(lay.host)
        assert A.launch(env["lib"], A.device_segments(lay, warm, which), h, 0, step_dev=step_dev.data_ptr(), lr_dev=lr_dev.data_ptr()) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with env["ops"].graph_capture(g, side):
        assert A.launch(env["lib"], segs, h, 0, step_dev=step_dev.data_ptr(), lr_dev=lr_dev.data_ptr()) == 0
    torch.cuda.synchronize()
    A.check_buffers(lay, _down(dev), lay.host, "capture runs nothing")
    cur = [np.array(b) for b in lay.host]
    for i, lr in enumerate(lrs):
        step_dev.fill_(5 + i)
        lr_dev.fill_(lr)
        g.replay()
        got = _down(dev)
        want = _run(env, lay, which, A.DEFAULT._replace(lr=A.lr_through_float(lr)), 5 + i, before=cur)
        A.check_buffers(lay, got, want, "replay %d" % (i + 1))
        assert (A.bits(got[0]) != A.bits(cur[0])).any()
        cur = got


# ---- classes ----

_CLEAN = {}


def _clean(env, t):
    if t not in _CLEAN:
        values = A.draw("poison-t%d" % t, A.POISON_N, 1.0, "zero" if t == 1 else "match")
        lay = A.Layout([(values, A.ALIGNED)])
        _CLEAN[t] = (values, _results(lay, _run(env, lay, [0], A.DEFAULT, t), [0]))
    return _CLEAN[t]


@pytest.mark.parametrize("kind,x", A.POISONS, ids=["%s=%r" % (k, float(x)) for k, x in A.POISONS])
def test_poisoned_operands_follow_torchs_class_map_and_stay_local(env, kind, x):
    for t in A.POISON_T:
        values, clean = _clean(env, t)
        bad = A.poisoned(values, kind, x)
        lay = A.Layout([(bad, A.ALIGNED)])
        after = _run(env, lay, [0], A.DEFAULT, t)
        got = _results(lay, after, [0])
        A.check_geometry(lay, after, [0], got, name="%s=%r" % (kind, x))           # sentinels and grad
        want = A.torch_adam(bad, A.DEFAULT, t)
        print("t %d %s=%r: classes (p', m', v') at the poison: device %r torch %r" % (
            t, kind, x, [int(A.classes(a)[5]) for a in got], [int(A.classes(a)[5]) for a in want]))
        A.check_classes(got, want, clean, "t%d %s=%r" % (t, kind, x))


# ---- refusals ----

def test_every_refusal_returns_its_code_and_writes_nothing(env):
    lay = A.Layout([(A.draw("refuse/%d" % s, n), A.ALIGNED) for s, n in enumerate(A.REFUSAL_SIZES)])
    dev = _up(lay.host)
    step_dev, lr_dev = _scalar(3), _scalar(1e-3)
    seg_addr = A.device_segments(lay, dev)
    for name, (code, change) in A.REFUSALS.items():
        segs, nseg, h, step, sd, ld = A.refusal_args(change, seg_addr, step_dev.data_ptr(), lr_dev.data_ptr())
        plan = env["ops"].adam_plan(segs, h.lr, (h.beta1, h.beta2), h.eps, step, sd, ld, nseg=nseg)
        assert plan["status"] == code, (name, plan)                  # refused by the plan: the entry below launches nothing
        assert A.launch(env["lib"], segs, h, step, step_dev=sd, lr_dev=ld, nseg=nseg) == code, name
        A.check_buffers(lay, _down(dev), lay.host, name)
    assert float(step_dev) == 3 and float(lr_dev) == F32(1e-3)
    assert A.launch(env["lib"], seg_addr, A.DEFAULT, 3) == 0         # and the ordinary launch is taken
    after = _down(dev)
    assert (A.bits(after[0]) != A.bits(lay.host[0])).any()
