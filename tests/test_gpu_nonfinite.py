"""The forward against torch's NaN / Inf semantics, entry by entry (tests/nonfinite_contract.py): per case the device's class map
(finite / NaN / +Inf / -Inf) against the float64 reference on the poisoned operands, and every element the poison does not reach
bitwise against the same launch on the clean operands.  No tolerance in either.

On the library before bbb::max_nan (fmaxf / med3(a, b, +inf) maxima, a `v > 20 ? v : sp` softplus select) 375 of the 933 cases fail:
every ReLU / Softplus epilogue and every max pool under a NaN, and with them every model-level case.  The per-entry counts are
printed at the end of a run (-s) and stand in profiles/nonfinite_notes.md."""
import collections

import numpy as np
import pytest
import torch

import nonfinite_contract as NC

pytestmark = pytest.mark.gpu

_clean = {}
_tally = collections.defaultdict(lambda: [0, 0])


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module's last case: failing cases per entry (visible with -s)."""
    yield
    print("\nnon-finite contract, failing cases per entry (failed / run):")
    for entry in sorted(_tally):
        print("  %-32s %3d / %3d" % (entry, _tally[entry][0], _tally[entry][1]))
    print("  %-32s %3d / %3d" % ("total", sum(v[0] for v in _tally.values()), sum(v[1] for v in _tally.values())))


def device_eps(call, n):
    """The device's own noise stream (the same elements the LRT launches draw)."""
    from bbb_hip import ops
    return ops.eps_dump(n, NC.SEED, call, NC.STREAM, torch.device("cuda")).cpu().numpy()


def _clean_launch(case):
    """One clean launch per group of cases: same operands, same seed and call, poison removed."""
    if case.group not in _clean:
        _clean[case.group] = NC.launch(case, poisoned=False)
    return _clean[case.group]


@pytest.mark.parametrize("cid", [c.id for c in NC.CASES])
def test_nonfinite(cid):
    case = NC.BY_ID[cid]
    _tally[case.entry][1] += 1
    try:
        ref = NC.reference(case, eps=device_eps)
        clean = _clean_launch(case)
        for name, a in clean.items():
            assert np.isfinite(a).all(), "%s: the clean launch's %s is not finite" % (cid, name)
        got = NC.launch(case)
        torch.cuda.synchronize()
        fails = NC.check(case, ref, NC.reach(case, device_eps), clean, got)
        assert not fails, "%s:\n  %s" % (cid, "\n  ".join(fails))
    except BaseException:
        _tally[case.entry][0] += 1
        raise
