"""The bf16 pooling / activation backward kernels alone, every <G_F32, OUT_F32> instantiation of the max pass
(pool_act_bwd_bf16_kernel: MaxPool2d(3, 2) behind ReLU, Bayesian3Conv3FC's window) and of the average pass
(avgpool_act_bwd_bf16_kernel: AvgPool2d(2, 2)) on [10 x 64 planes][16 x 16][512]; 35 launches each, the first of them the warm-up.  Run from the
root of a built tree under rocprofv3 --kernel-trace --stats (a run of its own); profiles/pool_home_notes.md compares two trees."""
import sys
sys.path.insert(0, "pytorch-bayesiancnn_amd")
import torch
from bbb_hip import ops
torch.manual_seed(0)
y = torch.relu(torch.randn((10, 64, 16, 16, 512), device="cuda")).bfloat16()
g_max = torch.randn((10, 64, 7, 7, 512), device="cuda")
g_avg = torch.randn((10, 64, 8, 8, 512), device="cuda")
for g_f32 in (False, True):
    for out_f32 in (False, True):
        gm, ga = (g_max, g_avg) if g_f32 else (g_max.bfloat16(), g_avg.bfloat16())
        for _ in range(35):
            ops.pool_act_backward_chwn_bf16(gm, y, 3, 2, "relu", out_f32=out_f32)
        torch.cuda.synchronize()
        for _ in range(35):
            ops.avgpool_act_backward_chwn_bf16(ga, y, (2, 2), (2, 2), (0, 0), True, "relu", out_f32=out_f32)
        torch.cuda.synchronize()
n = y.numel()
print("bytes per launch, max pass: y", 2 * n, "+ g_out", g_max.numel(), "x 2|4 + g_pre", n, "x 2|4")
