"""The forward kernel alone on [10 x 128 planes][8 x 8][512]: the global window (a GAP head) and a 2 x 2 / 2 window, 50 launches
each after warm-up; run under rocprofv3 --kernel-trace --stats."""
import sys
sys.path.insert(0, "pytorch-bayesiancnn_amd")
import torch
from bbb_hip import ops
x = torch.randn((10, 128, 8, 8, 512), device="cuda")
for spec in (((8, 8), (8, 8), (0, 0), True), ((2, 2), (2, 2), (0, 0), True)):
    for _ in range(55):
        y = ops.avgpool_chwn(x, *spec)
    torch.cuda.synchronize()
g = torch.randn((10, 128, 1, 1, 512), device="cuda")
for _ in range(55):
    ops.avgpool_act_backward_chwn(g, x, (8, 8), (8, 8), (0, 0), True, "softplus")
torch.cuda.synchronize()
print("bytes global fwd", x.numel() * 4 + g.numel() * 4, "2x2 fwd", x.numel() * 4 + x.numel(), "global bwd", 2 * x.numel() * 4 + g.numel() * 4)
