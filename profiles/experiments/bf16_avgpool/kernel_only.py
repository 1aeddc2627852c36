"""The bf16 average-pool kernels alone beside their fp32 counterparts on [10 x 128 planes][8 x 8][512]: the global window (a GAP
head) and a 2 x 2 / 2 window forward, the global window's backward with softplus; 50 launches each after warm-up.  Run under
rocprofv3 --kernel-trace --stats (a run of its own)."""
import sys
sys.path.insert(0, "pytorch-bayesiancnn_amd")
import torch
from bbb_hip import ops
x = torch.randn((10, 128, 8, 8, 512), device="cuda")
xb = x.bfloat16()
for spec in (((8, 8), (8, 8), (0, 0), True), ((2, 2), (2, 2), (0, 0), True)):
    for _ in range(55):
        ops.avgpool_chwn(x, *spec)
    torch.cuda.synchronize()
    for _ in range(55):
        ops.avgpool_chwn_bf16(xb, *spec)
    torch.cuda.synchronize()
g = torch.randn((10, 128, 1, 1, 512), device="cuda")
gb = g.bfloat16()
y, yb = torch.nn.functional.softplus(x), torch.nn.functional.softplus(x).bfloat16()
for _ in range(55):
    ops.avgpool_act_backward_chwn(g, y, (8, 8), (8, 8), (0, 0), True, "softplus")
torch.cuda.synchronize()
for _ in range(55):
    ops.avgpool_act_backward_chwn_bf16(gb, yb, (8, 8), (8, 8), (0, 0), True, "softplus")
torch.cuda.synchronize()
n, m = x.numel(), g.numel()
print("fp32 bytes: global fwd", 4 * (n + m), "2x2 fwd", 4 * n + n, "global bwd", 4 * (2 * n + m))
print("bf16 bytes: global fwd", 2 * (n + m), "2x2 fwd", 2 * n + n // 2, "global bwd", 2 * (2 * n + m))
