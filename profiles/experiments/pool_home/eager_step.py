"""The eager (launch by launch) fp32 training step of the metric shape, what bench.py reports as split_bf16.training_step_ms.fp32,
timed over a longer window: BayesianAlexNet bs=512 num_ens=10, forward + backward + Adam, 20 warm-up steps, then 300 timed steps
ending in a synchronise.  Run from the root of a built tree, one process per figure; profiles/pool_home_notes.md alternates two trees."""
import sys
import time
sys.path.insert(0, ".")
sys.path.insert(0, "pytorch-bayesiancnn_amd")
import torch
import bench
from bbb_hip import ops, train
dev = torch.device("cuda:0")
cfg = bench.CONFIGS["metric"]
net, x = bench.build_net(cfg, dev)
y = torch.randint(0, cfg["classes"], (cfg["B"],), device=dev)
opt = train.FusedAdam(net.parameters(), lr=1e-3)
ops.gemm_mode = "fp32"
for _ in range(20):
    train.train_step(net, opt, x, y, cfg["E"], 0.1, 50000.0, graph=False)
torch.cuda.synchronize(dev)
n = 300
t0 = time.perf_counter()
for _ in range(n):
    train.train_step(net, opt, x, y, cfg["E"], 0.1, 50000.0, graph=False)
torch.cuda.synchronize(dev)
print("eager fp32 training step: %.4f ms per step over %d steps" % (1e3 * (time.perf_counter() - t0) / n, n))
