"""The Monte-Carlo tail, loss and uncertainty kernels (csrc/mc_tail.hip), entry by entry, against float64: the named cases of
tests/tail_contract.py.  Every element of every output is compared (-inf rows must be -inf at exactly the reference's positions) on
shift-invariant scales, inside DEVICE_FACTOR x the error of the max-first fp32 model -- a bound taken from the reference and the model
(tests/test_tail_sweep_cpu.py), never from a kernel.  Where one kernel computes both sides the comparison is bitwise: a group's block
against mc_tail_cb of its slabs, a full share against mc_tail_groups, one slice of units against mc_tail_cb, a launch with the step
epilogue against the launch without.  mc_tail and mc_tail_cb are different kernels and are held to the bound only.
Needs an MI355X: -m gpu."""
import math

import numpy as np
import pytest
import torch

import tail_contract as C

pytestmark = pytest.mark.gpu
F32 = np.float32
WORST = {}


@pytest.fixture(scope="module")
def env():
    from bbb_hip import ops, _lib
    _lib.lib()
    yield {"ops": ops, "lib": _lib}
    print("\ndevice, worst |kernel - float64| / scale per operation (bound):",
          {k: "%.2f at %s (%g)" % (v[0], v[1], C.bound(k.split(":")[0])) for k, v in sorted(WORST.items())})


def _note(op, ratio, case, limit=None):
    """Print the figure, keep the worst, then hold it to the bound."""
    print("%s %s: %.3f (bound %g)" % (case.name, op, ratio, C.bound(op.split(":")[0]) if limit is None else limit))
    if ratio > WORST.get(op, (-1.0, ""))[0]:
        WORST[op] = (ratio, case.name)
    assert ratio <= (C.bound(op.split(":")[0]) if limit is None else limit), (case.name, op, ratio)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(a, b, ref):
    """Worst |a - b| / (2^-24 (1 + |ref|)) over the finite positions of ref; a and b -inf exactly where ref is."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    hole = np.isneginf(ref)
    assert (np.isneginf(a) == hole).all() and (np.isneginf(b) == hole).all()
    return float((np.abs(a[~hole] - b[~hole]) / (C.U * (1.0 + np.abs(ref[~hole])))).max())


def _run_form(ops, case, x, mean_over, step_end=None):
    """The tail entry of `case` (for step_end cases: of its form) on device logits x."""
    p = case.p
    form = p.get("form", case.entry)
    if form == "mc_tail":
        return ops.mc_tail(x, mean_over)
    if form == "mc_tail_cb":
        return ops.mc_tail_cb(x, mean_over, step_end)
    if form == "mc_tail_units":
        return ops.mc_tail_units(x, p["S"], p["off"], mean_over, step_end)
    if form == "mc_tail_groups":
        return ops.mc_tail_groups(x, p["G"], p["E"], mean_over, step_end)
    assert form == "mc_tail_share" and mean_over == 0
    return ops.mc_tail_share(x, p["steps"], p["draws"], p["first_off"], step_end)


TAIL_CASES = [c for c in C.ALL_CASES if c.entry in C.TAIL_ENTRIES]


@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: c.name)
def test_tail(env, case):
    ops, lib = env["ops"], env["lib"]
    p = case.p
    form = p.get("form", case.entry)
    rows = C.rows_of(case)
    blocks = C.blocks_of(case)
    x = _dev(C.layout(case, rows))
    ref = C.tail_ref(rows, blocks, case.mean_over)
    got_t = _run_form(ops, case, x, case.mean_over)
    got = got_t.cpu().numpy()
    assert got.shape == (len(blocks) * case.B, case.C) and got.dtype == F32
    _note("tail", C.tail_ratio(got, ref), case)

    if form != "mc_tail_share":                    # mean_over = M is mean_over = 0 minus log M
        M = case.mean_over or max(case.slabs, 2)
        ref0 = C.tail_ref(rows, blocks, 0)
        with_m, without = _run_form(ops, case, x, M).cpu().numpy(), _run_form(ops, case, x, 0).cpu().numpy()
        _note("tail", C.tail_ratio(with_m, C.tail_ref(rows, blocks, M)), case)
        _note("tail", C.tail_ratio(without, ref0), case)
        hole = np.isneginf(ref0)
        shifted = np.where(hole, -np.inf, without.astype(np.float64) - math.log(M))
        _note("tail:mean_over", _rel(with_m, shifted, ref0 - math.log(M)), case)
    if form in ("mc_tail", "mc_tail_cb"):          # the other layout's kernel on the transposed logits: the bound, not the bits
        xt = x.permute(0, 2, 1).contiguous()
        other = (ops.mc_tail_cb if form == "mc_tail" else ops.mc_tail)(xt, case.mean_over).cpu().numpy()
        _note("tail", C.tail_ratio(other, ref), case)
        _note("tail:other-layout", _rel(got, other, ref), case)

    # one kernel on both sides: bit for bit
    if form == "mc_tail_groups":
        for g, idx in enumerate(blocks):
            assert torch.equal(got_t[g * case.B:(g + 1) * case.B], ops.mc_tail_cb(x[idx[0]:idx[-1] + 1], case.mean_over)), (case.name, g)
    if form == "mc_tail_share" and p["first_off"] == 0 and case.slabs == p["steps"] * p["draws"]:
        assert torch.equal(got_t, ops.mc_tail_groups(x, p["steps"], p["draws"], 0)), case.name
    if form == "mc_tail_share":                    # every block that holds a slab is mc_tail_cb of its slabs
        for k, idx in enumerate(blocks):
            if idx:
                assert torch.equal(got_t[k * case.B:(k + 1) * case.B], ops.mc_tail_cb(x[idx[0]:idx[-1] + 1], 0)), (case.name, k)
    if form == "mc_tail_units":
        if p["S"] == 1:
            assert torch.equal(got_t, ops.mc_tail_cb(x, case.mean_over)), case.name
        for s, idx in enumerate(blocks):            # a slice's units, gathered, through mc_tail_cb
            if idx:
                assert torch.equal(got_t[s * case.B:(s + 1) * case.B], ops.mc_tail_cb(x[idx].contiguous(), case.mean_over)), (case.name, s)
        if p["off"] >= p["S"]:                      # the entry itself takes unit_off modulo the slices (ops reduces it first)
            raw = torch.full_like(got_t, 7.0)
            rc = lib.lib().bbb_mc_tail_units(x.data_ptr(), case.slabs, p["S"], p["off"], case.B, case.C, case.mean_over, raw.data_ptr(),
                                             ops.cur_stream(x.device))
            assert rc == 0 and torch.equal(raw, got_t), case.name

    if case.entry == "step_end":
        kl_in = torch.tensor(p["kl"], dtype=torch.float32, device="cuda")
        counter = torch.tensor(p["counter0"], dtype=torch.int32, device="cuda")
        lse, kl_out = _run_form(ops, case, x, case.mean_over, (kl_in, p["scale"], counter, p["add"]))
        assert torch.equal(lse, got_t), case.name
        assert kl_out.cpu().numpy() == F32(p["kl"]) * F32(p["scale"]) and float(kl_in) == float(F32(p["kl"]))
        assert (int(counter) - p["counter0"] - p["add"]) % 2 ** 32 == 0, (case.name, int(counter))       # once, whatever the blocks
        lse2, kl2 = _run_form(ops, case, x, case.mean_over, (kl_in, p["scale"], None, 0))                # no counter: nothing else moves
        assert torch.equal(lse2, got_t) and torch.equal(kl2, kl_out)
        assert (int(counter) - p["counter0"] - p["add"]) % 2 ** 32 == 0


@pytest.mark.parametrize("case", [c for c in C.CASES if c.entry == "mc_tail_cb_autograd"], ids=lambda c: c.name)
def test_tail_backward(env, case):
    ops = env["ops"]
    rows, w = C.rows_of(case), C.upstream_of(case)
    x = _dev(C.layout(case, rows)).requires_grad_(True)
    lse = ops.mc_tail_cb_autograd(x, case.mean_over)
    _note("tail", C.tail_ratio(lse.detach().cpu().numpy(), C.tail_ref(rows, C.blocks_of(case), case.mean_over)), case)
    assert torch.equal(lse.detach(), ops.mc_tail_cb(x.detach(), case.mean_over))
    (lse * _dev(w)).sum().backward()
    got = x.grad.cpu().numpy().transpose(0, 2, 1)
    _note("tail_grad", C.grad_ratio(got, C.tail_grad_ref(rows, w, case.mean_over)), case)


@pytest.mark.parametrize("case", [c for c in C.CASES if c.entry == "elbo_cb_autograd"], ids=lambda c: c.name)
def test_elbo(env, case):
    """loss = nll_loss(lse, target) * train_size + beta * kl with targets outside [0, C) contributing nothing while the mean still
    divides by B (include/bbb_hip.h, elbo_cb_kernel's comment).  This is NOT the ignore_index mean of F.nll_loss, which divides by the
    number of images kept; the float64 reference (tail_contract.elbo_ref) is written from the header's definition."""
    ops = env["ops"]
    p = case.p
    rows, target = C.rows_of(case), C.targets_of(case)
    x = _dev(C.layout(case, rows)).requires_grad_(True)
    kl = torch.tensor(p["kl"], dtype=torch.float32, device="cuda", requires_grad=True)
    beta = torch.tensor(p["beta"], dtype=torch.float32, device="cuda") if p["beta_dev"] else p["beta"]
    loss, lse = ops.elbo_cb_autograd(x, kl, _dev(target), beta, p["train_size"], case.mean_over)
    loss.backward()
    beta32 = float(F32(p["beta"]))
    loss64, g64, gk64 = C.elbo_ref(rows, target, float(F32(p["kl"])), beta32, p["train_size"], case.mean_over)
    _note("tail", C.tail_ratio(lse.cpu().numpy(), C.tail_ref(rows, C.blocks_of(case), case.mean_over)), case)
    _note("elbo_loss", C.loss_ratio(float(loss), loss64), case)
    _note("elbo_grad", C.grad_ratio(x.grad.cpu().numpy().transpose(0, 2, 1), g64), case)
    assert float(kl.grad) == beta32 == gk64, (case.name, float(kl.grad))
    if case.B >= 3:                     # the images whose target lies outside [0, C) get no gradient at all
        out = np.flatnonzero((target < 0) | (target >= case.C))
        assert out.size >= 2 and not x.grad[:, :, _dev(out)].any()


@pytest.mark.parametrize("case", [c for c in C.CASES if c.entry == "uncertainty"], ids=lambda c: c.name)
def test_uncertainty(env, case):
    ops = env["ops"]
    rows, normalized = C.rows_of(case), case.p["normalized"]
    got = [t.cpu().numpy() for t in ops.uncertainty(_dev(rows), normalized)]
    ref = C.uncertainty_ref(rows, normalized)
    assert all(g.shape == (case.B, case.C) for g in got)
    for op, r in zip(("pred", "epi", "ale"), C.uncertainty_ratios(got, ref, rows)):
        _note(op, r, case)
    # in exact arithmetic epi >= 0 and ale >= 0
    assert got[1].min() >= -C.bound("epi") * C.U and got[2].min() >= -C.bound("ale") * C.U, (case.name, got[1].min(), got[2].min())
    if case.slabs == 1:
        assert not got[1].any() and (got[0] == rows[0]).all()


def test_refusals(env):
    """Each raises BBBHipError from the argument checks: the outputs, where one was allocated at all, are never written."""
    ops, E = env["ops"], env["lib"].BBBHipError
    z = lambda *s: torch.zeros(*s, device="cuda")
    for call in (lambda: ops.mc_tail(z(2, 3, 1025)), lambda: ops.uncertainty(z(2, 3, 1025)), lambda: ops.uncertainty(z(2, 3, 1025), True),
                 lambda: ops.mc_tail_cb(z(513, 2, 3)), lambda: ops.mc_tail_cb_autograd(z(513, 2, 3).requires_grad_(True)),
                 lambda: ops.mc_tail_share(z(9, 2, 3), 3, 4, 4), lambda: ops.mc_tail_share(z(9, 2, 3), 3, 4, -1),
                 lambda: ops.mc_tail_share(z(9, 2, 3), 2, 4, 0), lambda: ops.mc_tail_share(z(12, 2, 3), 3, 4, 1),
                 lambda: ops.mc_tail_groups(z(12, 2, 3), 3, 5), lambda: ops.mc_tail_groups(z(1282, 1, 1), 2, 641),
                 lambda: ops.mc_tail_share(z(700, 1, 1), 2, 641, 0), lambda: ops.mc_tail_units(z(1300, 1, 1), 2, 0)):
        with pytest.raises(E):
            call()
    torch.cuda.synchronize()


def test_admitted_maximum_launches(env):
    """640 draws per image, the most the plan admits (160 KB of LDS, with the per-kernel attribute set): equal logits of one class make
    every log_softmax 0, so block g is log(640) - log(mean_over); held to the tail bound against float64."""
    ops = env["ops"]
    got = ops.mc_tail_groups(torch.full((2 * C.MAX_PER_SLICE, 1, 3), 2.5, device="cuda"), 2, C.MAX_PER_SLICE, mean_over=10).cpu().numpy()
    ref = np.full((6, 1), math.log(C.MAX_PER_SLICE) - math.log(10))
    case = C.Case("groups-2x640", "mc_tail_groups", "ties", 2 * C.MAX_PER_SLICE, 1, 3, 10)
    _note("tail", C.tail_ratio(got, ref), case)
