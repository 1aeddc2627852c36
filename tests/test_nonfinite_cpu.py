"""The non-finite contract (tests/nonfinite_contract.py) without a device: its table covers every forward entry, its reference
follows torch's rules on NaN and Inf, and no case is vacuous."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bbb_numpy as O
import nonfinite_contract as NC

# the forward entries of bbb_hip/ops.py (and the two model-level entries) the contract covers -> the poisons each can take.  A -Inf
# that the entry maps to a finite value everywhere is not a poison of that entry (max pools); the tail takes NaN and +Inf (a -Inf
# logit is a finite log-probability of zero weight); the parameter pass and the models take a NaN.
ALL4, NO_PAIR, MAXPOOL, TAIL, ONLY_NAN = (NC.NAN, NC.PINF, NC.NINF, NC.PAIR), (NC.NAN, NC.PINF, NC.NINF), (NC.NAN, NC.PINF, NC.PAIR), \
    (NC.NAN, NC.PINF), (NC.NAN,)
FORWARD_ENTRIES = {
    "conv2d_forward": ALL4, "conv2d_chwn_forward": ALL4, "conv2d_c8x3_forward": ALL4, "conv2d_chwn_bf16_forward": ALL4,
    "lrt_conv2d_forward": ALL4, "lrt_conv2d_chwn_forward": ALL4, "lrt_conv2d_c8x3_forward": ALL4, "lrt_conv2d_chwn_bf16_forward": ALL4,
    "lrt_sample_chwn": NO_PAIR, "lrt_sample_chwn_bf16": NO_PAIR, "lrt_sample_nchw": NO_PAIR,
    "maxpool_chwn": MAXPOOL, "maxpool_chwn_bf16": MAXPOOL, "maxpool_chwn_s3": MAXPOOL, "maxpool_c8s3": MAXPOOL,
    "avgpool_chwn": ALL4, "avgpool_chwn_bf16": ALL4,
    "to_batch_innermost": NO_PAIR, "to_batch_innermost_bf16": NO_PAIR, "s3_from_f32": NO_PAIR, "s3_to_f32": NO_PAIR,
    "c8s3_from_f32": NO_PAIR, "c8s3_to_f32": NO_PAIR, "s2d_c8s3": NO_PAIR,
    "mc_tail": TAIL, "mc_tail_cb": TAIL, "mc_tail_units": TAIL, "mc_tail_groups": TAIL, "mc_tail_share": TAIL, "uncertainty": TAIL,
    "elbo_cb_autograd": TAIL,
    "reparam_kl_forward": ONLY_NAN, "sample_weights": ONLY_NAN, "mc_forward": ONLY_NAN, "train_step": ONLY_NAN,
}
# what the issue lists per entry beyond the poisons: every activation / form / window / tap / operand must have its cases
REQUIRED = {
    "conv": {"variant": set(NC.CONV_VARIANTS), "act": set(NC.ACTS), "place": {"input", "weight", "bias"}},
    "lrt": {"variant": set(NC.LRT_VARIANTS), "act": set(NC.ACTS), "place": {"input", "weight", "bias"}},
    "pool": {"entry": set(NC.POOL_ENTRIES), "win": {(2, 2), (3, 2)}, "place": {"first", "middle", "last"}},
    "param": {"entry": set(NC.PARAM_ENTRIES), "place": {"mu", "rho"}},
    "model": {"model": {"std", "alone", "quirk"}, "kind": {"bbb", "lrt"}, "precision": {"fp32", "bf16x3", "bf16"}, "B": {8, 6}},
}


def test_every_forward_entry_has_a_case_for_every_poison_it_takes():
    from bbb_hip import ensemble, ops, train
    have = collections.defaultdict(set)
    for c in NC.CASES:
        have[c.entry].add(c.poison)
    assert set(have) == set(FORWARD_ENTRIES) == set(NC.ENTRIES)
    for entry, poisons in FORWARD_ENTRIES.items():
        assert have[entry] == set(poisons), (entry, have[entry])
        assert hasattr({"mc_forward": ensemble, "train_step": train}.get(entry, ops), entry), entry


def test_every_form_activation_and_placement_is_crossed():
    for family, axes in REQUIRED.items():
        cs = [c for c in NC.CASES if c.family == family]
        for axis, want in axes.items():
            got = {c.place if axis == "place" else c.params.get(axis) for c in cs}
            assert got >= want, (family, axis, want - got)
    # every conv / LRT form meets every activation with a NaN at every placement; uncertainty runs both normalisations
    for family in ("conv", "lrt"):
        seen = {(c.params["variant"], c.params["act"], c.place) for c in NC.CASES if c.family == family and c.poison == NC.NAN}
        variants = NC.CONV_VARIANTS if family == "conv" else NC.LRT_VARIANTS
        assert seen == {(v, a, pl) for v in variants for a in NC.ACTS for pl in ("input", "weight", "bias")}
    assert {c.params["entry"] for c in NC.CASES if c.entry == "uncertainty"} == {"uncertainty", "uncertainty_normalized"}
    assert any(c.params.get("train") for c in NC.CASES if c.entry == "train_step")


def test_the_case_geometries_reach_the_forms_they_name():
    """Host-side plans only: the split layer splits, the pooled bf16 forms are the first-layer kernels, the c8 form is the strip."""
    from bbb_hip import ops
    g = NC.geo_of(dict(variant="chwn-splitk"))
    with ops.use_config(split_k=True):
        plan = ops.fp32_fwd_plan((g["E"], g["Cin"], g["H"], g["W"], g["B"]), (g["E"], g["Cout"], g["Cin"], g["k"], g["k"]), 1, g["pad"], 1, draws=g["E"])
    assert plan[5] > 1 and plan[0] in ("bbb-cross", "bbb-seq64-ilv"), plan
    g = NC.geo_of(dict(variant="chwn-pool"))
    assert ops.fp32_fwd_plan((g["E"], g["Cin"], g["H"], g["W"], g["B"]), (g["E"], g["Cout"], g["Cin"], g["k"], g["k"]), 1, g["pad"], 1, draws=g["E"],
                             pool=True)[0] == "bbb-pool"
    assert ops.fp32_fwd_plan((g["E"], g["Cin"], g["H"], g["W"], g["B"]), (1, g["Cout"], g["Cin"], g["k"], g["k"]), 1, g["pad"], 1, draws=g["E"],
                             lrt=True, pool=True)[0] == "lrt-pool"
    assert set(NC.BF16_FORMS) == {v for v in NC.CONV_VARIANTS if v.startswith("bf16")}
    assert {"general", "smallk", "smallk-pool", "smallk-poolwin", "strip8"} == set(NC.BF16_FORMS.values())      # both fused pools
    seen = set()
    for v, form in NC.BF16_FORMS.items():
        g = NC.geo_of(dict(variant=v))
        got = ops.bf16_fwd_plan((g["E"], g["Cin"], g["H"], g["W"], g["B"]), g["Cout"], (g["Cin"], g["k"], g["k"]), 1, g["pad"], 1, draws=g["E"],
                                tap_major=v in NC.BF16_TM, x_c8=v in NC.BF16_XC8, out_c8=v in NC.BF16_OC8, pool=NC.CONV_POOL.get(v))[0]
        assert got == form, (v, got)
        seen.add((form, NC.CONV_POOL.get(v), v in NC.BF16_OC8, g["Cout"] > 32))
    # each fused pool with both windows and both outputs; the strip form with one and with two channel tiles; strip8 with both outputs
    for form in ("smallk-pool", "smallk-poolwin"):
        assert {(w, c8) for f, w, c8, _ in seen if f == form} >= {((2, 2), False), ((3, 2), False), ((2, 2), True)}, form
    assert {wide for f, _, _, wide in seen if f == "smallk-pool"} == {False, True}
    assert {c8 for f, _, c8, _ in seen if f == "strip8"} == {False, True}
    for v, pool in (("c8x3", False), ("c8x3-pool", True)):
        g = NC.geo_of(dict(variant=v))
        form = ops.c8x3_fwd_plan((g["E"], g["Cin"], g["H"], g["W"], g["B"]), g["Cout"], g["k"], 1, g["pad"], 1, draws=g["E"], pool=pool)[0]
        assert form.endswith("pool" if pool else "s3"), (v, form)


# ------------------------------------------------------------------------------------------------ the reference's rules
NONFINITE = (float("nan"), float("inf"), float("-inf"))


def test_torch_activations_propagate_nan_and_agree_with_float64_and_the_oracle():
    v = torch.tensor([float("nan"), float("inf"), float("-inf"), -1.5, 0.0, 25.0])
    for f32, f64, oracle in ((F.relu, F.relu, O.relu_act), (F.softplus, F.softplus, O.softplus_act)):
        a, b = f32(v).numpy(), f64(v.double()).numpy()
        assert (NC.classes(a) == NC.classes(b)).all() and (NC.classes(a) == NC.classes(oracle(v.numpy()))).all()
        assert NC.classes(a).tolist() == [NC.IS_NAN, NC.IS_PINF, NC.FINITE, NC.FINITE, NC.FINITE, NC.FINITE]


@pytest.mark.parametrize("k,s", [(2, 2), (3, 2)])
def test_torch_max_pool_keeps_a_nan_at_any_position_of_the_window(k, s):
    for dtype in (torch.float32, torch.float64):
        for r in range(k):
            for c in range(k):
                x = torch.randn(1, 1, 8, 8, generator=torch.Generator().manual_seed(3)).to(dtype)
                x[0, 0, 2 + r, 2 + c] = float("nan")
                y = F.max_pool2d(x, k, s)
                assert torch.isnan(y[0, 0, 1, 1]), (dtype, r, c)
                clean = F.max_pool2d(torch.nan_to_num(x, nan=-1e9), k, s)
                assert torch.equal(y[~torch.isnan(y)], clean[~torch.isnan(y)])
    x = torch.randn(1, 1, 8, 8)
    x[0, 0, 2, 2], x[0, 0, 2, 3] = float("inf"), float("-inf")
    assert F.max_pool2d(x, k, s)[0, 0, 1, 1] == float("inf")                    # a -Inf never wins: not a poison of a max pool


def test_torch_avg_pool_and_log_softmax_behave_as_the_contract_says():
    for dtype in (torch.float32, torch.float64):
        for v, want in zip(NONFINITE, (NC.IS_NAN, NC.IS_PINF, NC.IS_NINF)):
            x = torch.randn(1, 1, 4, 4).to(dtype)
            x[0, 0, 1, 1] = v
            y = F.avg_pool2d(x, 2, 2)
            assert NC.classes(y.numpy())[0, 0].tolist() == [[want, NC.FINITE], [NC.FINITE, NC.FINITE]]
        x = torch.randn(1, 1, 4, 4).to(dtype)
        x[0, 0, 0, 0], x[0, 0, 0, 1] = float("inf"), float("-inf")
        assert torch.isnan(F.avg_pool2d(x, 2, 2)[0, 0, 0, 0])
        z = torch.randn(3, 5).to(dtype)
        for v in (float("nan"), float("inf")):                                  # the whole row is NaN, the other rows do not notice
            p = z.clone()
            p[1, 2] = v
            ls = torch.log_softmax(p, dim=1)
            assert torch.isnan(ls[1]).all() and torch.equal(ls[[0, 2]], torch.log_softmax(z, dim=1)[[0, 2]])
        p = z.clone()
        p[1, 2] = float("-inf")                                                 # a class of probability zero: nothing is poisoned
        assert torch.isfinite(torch.log_softmax(p, dim=1)[1, [0, 1, 3, 4]]).all()


def test_an_inf_splits_into_inf_nan_nan():
    """The three-piece exception, from the number format alone: hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid)."""
    for v in (float("inf"), float("-inf")):
        x = torch.tensor([v])
        hi = x.to(torch.bfloat16).float()
        mid = (x - hi).to(torch.bfloat16).float()
        lo = (x - hi - mid).to(torch.bfloat16).float()
        assert torch.isinf(hi).all() and torch.isnan(mid).all() and torch.isnan(lo).all() and torch.isnan(hi + mid + lo).all()


# ------------------------------------------------------------------------------------------------ non-vacuity, on the reference alone
def test_every_case_poisons_something_and_leaves_at_least_half():
    """Both assertions bite in every case: at least one output element is non-finite in the reference, and at least half of every
    output's elements are out of the poison's reach (what the locality assertion compares), and finite there."""
    clean = {}
    for c in NC.CASES:
        ref, kinds = NC.reference(c), NC.kinds(c)
        if c.group not in clean:
            clean[c.group] = NC.reference(c, poisoned=False)
        assert set(ref) == set(kinds) == set(clean[c.group]), (c.id, set(ref), set(kinds))
        poisoned = 0
        for name, r in ref.items():
            assert np.isfinite(clean[c.group][name]).all(), (c.id, name)
            bad = NC.classes(r) != NC.FINITE
            same = ~NC.reach(c)[name]
            assert (r[same] == clean[c.group][name][same]).all() and not (bad & same).any(), (c.id, name)      # reach() covers every change
            poisoned += int(bad.sum())
            if name not in NC.SCALAR_OUTPUTS:
                assert 2 * int(same.sum()) >= same.size and 2 * int(bad.sum()) <= bad.size, (c.id, name, int(same.sum()), int(bad.sum()), bad.size)
            else:
                assert r.size == 1 and bad.all(), (c.id, name)                  # a scalar output is listed because it must be poisoned
        assert poisoned > 0, c.id


def test_the_clean_reference_is_finite_and_the_poison_is_the_only_difference():
    for c in NC.CASES:
        clean, bad = NC.operands(c, poisoned=False), NC.operands(c)
        n = 0
        for k in clean:
            assert torch.isfinite(clean[k]).all(), (c.id, k)
            assert float(clean[k].abs().max()) < 16.0, (c.id, k)                # O(1): nothing overflows on its own in fp32 or bf16
            diff = ~(clean[k] == bad[k])
            n += int(diff.sum())
            assert torch.isfinite(bad[k][~diff]).all()
        assert n == (2 if c.poison == NC.PAIR else 1), (c.id, n)


def test_the_checker_bites():
    """check() on fabricated device outputs: the reference itself passes; a dropped NaN, an Inf reported as NaN and a leak into a
    clean element each fail."""
    c = NC.BY_ID["pool-maxpool_chwn-(2,2)-middle-nan"]
    ref = NC.reference(c)["y"]
    clean = np.where(np.isfinite(ref), ref, 0.25).astype(np.float32)
    good = np.where(np.isfinite(ref), clean, ref).astype(np.float32)
    refc = NC.reach(c)
    assert NC.check(c, {"y": ref}, refc, {"y": clean}, {"y": good}) == []
    assert any("class" in f for f in NC.check(c, {"y": ref}, refc, {"y": clean}, {"y": clean}))                # the NaN dropped (fmaxf)
    leak = good.copy()
    leak[np.unravel_index(np.argmax(np.isfinite(ref)), ref.shape)] += 1.0
    assert any("does not reach" in f for f in NC.check(c, {"y": ref}, refc, {"y": clean}, {"y": leak}))
    ci = NC.BY_ID["pool-maxpool_chwn-(2,2)-middle-+inf"]
    refi = NC.reference(ci)["y"]
    assert np.isposinf(refi).any()
    asnan = np.where(np.isfinite(refi), clean, np.nan).astype(np.float32)
    assert any("class" in f for f in NC.check(ci, {"y": refi}, NC.reach(ci), {"y": clean}, {"y": asnan}))              # exact entries: Inf is not NaN
    cs = NC.BY_ID["pool-maxpool_chwn_s3-(2,2)-middle-+inf"]
    refs = NC.reference(cs)["y"]
    pieces = np.stack([asnan, asnan, asnan])
    assert NC.check(cs, {"y": refs}, NC.reach(cs), {"y": np.stack([clean] * 3)}, {"y": pieces}) == []                  # three pieces: the mask is enough
    # a finite value the poison makes: relu(-Inf) is an exact zero, and any other number there fails
    cz = NC.BY_ID["conv-chwn-relu-input--inf"]
    rz, rzc = NC.reference(cz)["y"], NC.reference(cz, poisoned=False)["y"]
    rch = NC.reach(cz)
    made = rch["y"] & (rz == 0)
    assert made.any() and (rzc[made] != 0).any()
    cl = rzc.astype(np.float32)
    ok = np.where(rch["y"], rz, cl).astype(np.float32)
    assert NC.check(cz, {"y": rz}, rch, {"y": cl}, {"y": ok}) == []
    wrong = ok.copy()
    wrong[np.unravel_index(np.argmax(made), made.shape)] = 0.5
    assert any("exact zero" in f for f in NC.check(cz, {"y": rz}, rch, {"y": cl}, {"y": wrong}))
