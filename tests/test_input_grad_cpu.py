"""CPU-only checks of the first-layer input-gradient entry point (bbb_input_grad_col2im): it validates its arguments before it
touches the device, so the error codes come back on a GPU-less host."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-bayesiancnn_amd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "bbb_hip", "libbbb_hip.so")):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh")], check=True)
    from bbb_hip import _lib
    return _lib


def _desc(_lib, **kw):
    d = _lib.ConvDesc()
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = 4, 3, 8, 8, 1, 3, 3
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = d.draws = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_col2im_argument_errors_without_a_gpu(lib):
    h = lib.lib()
    f = h.bbb_input_grad_col2im
    P = 6 * 6 * 4                                                # ho * wo * batch of the default geometry (8 x 8 map, 3 x 3 taps)
    J = 3 * 3 * 3
    ok = ctypes.byref(_desc(lib))
    assert f(None, P, 0, None, 64, ok, None) == -1                                    # no D
    assert f(64, P, 0, None, None, ok, None) == -1                                    # no dx
    assert f(64, P, 0, None, 64, None, None) == -1                                    # no descriptor
    for field, v in (("batch", 0), ("cin", 0), ("h", -1), ("kh", 0), ("stride_w", 0), ("pad_h", -1), ("dil_w", 0)):
        assert f(64, P, 0, None, 64, ctypes.byref(_desc(lib, **{field: v})), None) == -1, field
    assert f(66, P, 0, None, 64, ok, None) == -2                                      # misaligned pointers
    assert f(64, P, 0, 64, 66, ok, None) == -2
    assert f(64, P, 0, None, 64, ctypes.byref(_desc(lib, kh=11, kw=11)), None) == -3   # kernel larger than the padded map
    assert f(64, P - 4, 0, None, 64, ok, None) == -3                                  # rows shorter than ho * wo * batch
    assert f(64, P, J * P - 1, 64, 64, ok, None) == -3                                # LRT: the two sets overlap
