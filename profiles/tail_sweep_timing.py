"""Kernel time of the batch-innermost Monte-Carlo tail (bbb_mc_tail_cb / _groups_step) and of the ELBO backward, for
profiles/tail_sweep_notes.md.  The launches are 5-500 us, shorter than a Python call, so K of them are captured into one hipGraph (a
serial chain) and the graph is replayed until the timed window is at least 0.2 s; device events around the window; best of five windows.
BBB_HIP_LIB picks the library (one process per library, alternated by the caller)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pytorch-bayesiancnn_amd"))
from bbb_hip import ops, _lib  # noqa: E402

_lib.lib()
print("library:", os.path.relpath(_lib.LIB_PATH))
K = 50


def us_per_launch(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(K):
                fn()
    torch.cuda.synchronize()
    reps, best = 4, float("inf")
    for _ in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 200.0:
            best = min(best, ms * 1e3 / (reps * K))
        else:
            reps = int(reps * max(2.0, 260.0 / max(ms, 1e-3)))
            best = float("inf")
    return best


gen = torch.Generator(device="cuda").manual_seed(7)
for E, C, B in ((10, 10, 512), (25, 10, 512), (10, 100, 512), (10, 1000, 512), (320, 10, 512), (321, 10, 512), (320, 100, 512), (321, 100, 512)):
    x = torch.randn(E, C, B, device="cuda", generator=gen) * 4
    print("mc_tail_cb E %d C %d B %d: %.2f us" % (E, C, B, us_per_launch(lambda: ops.mc_tail_cb(x, E))))
x = torch.randn(40, 10, 512, device="cuda", generator=gen) * 4
print("mc_tail_groups 4 x 10 draws C 10 B 512 (the benchmark's launch): %.2f us" % us_per_launch(lambda: ops.mc_tail_groups(x, 4, 10, 10)))
L = _lib.lib()
for E, C, B in ((10, 10, 512), (1, 100, 256)):
    x = torch.randn(E, C, B, device="cuda", generator=gen) * 4
    lse = ops.mc_tail_cb(x, E)
    y = torch.randint(0, C, (B,), device="cuda")
    one, out, gk = torch.ones((), device="cuda"), torch.empty_like(x), torch.empty((), device="cuda")
    bwd = lambda: _lib.check(L.bbb_elbo_cb_bwd(x.data_ptr(), lse.data_ptr(), y.data_ptr(), one.data_ptr(), 0.1, None, 50000.0, out.data_ptr(),
                                               gk.data_ptr(), E, B, C, E, ops.cur_stream(x.device)), "bbb_elbo_cb_bwd")
    print("elbo_cb_bwd E %d C %d B %d: %.2f us" % (E, C, B, us_per_launch(bwd)))
