"""ONE figure per process on the GAP AlexNet (AlexNet's conv stack at CIFAR size, AdaptiveAvgPool2d(1) -> FlattenLayer ->
BBBLinear head), bs 512, 10 draws: argv = what (bbb_infer | bbb_train | lrt_infer), precision (fp32 | bf16).  bf16 runs under
LaunchConfig.bf16_avgpool (and bf16_lrt for the LRT model).  Device events, warm-up, windows of at least a second.  Prints one
JSON line."""
import json
import sys
import time

sys.path.insert(0, "pytorch-bayesiancnn_amd")
what, precision = sys.argv[1], sys.argv[2]
import torch
import torch.nn as nn
from bbb_hip import ensemble, ops, rng, train, zoo

PRIORS = {"prior_mu": 0.0, "prior_sigma": 0.1, "posterior_mu_initial": (0.0, 0.1), "posterior_rho_initial": (-5.0, 0.1)}


def build(kind):
    torch.manual_seed(0)
    net = zoo.BBBAlexNet(10, 3, PRIORS, kind, "softplus")
    net.pool3 = nn.AdaptiveAvgPool2d(1)
    net = net.cuda()
    rng.assign_stream_ids(net)
    return net


def timed(fn, min_s=1.0, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    n, chunks = 0, []
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < min_s or n < 20:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(10):
            fn()
        e.record()
        e.synchronize()
        chunks.append(s.elapsed_time(e) / 10)
        n += 10
    chunks.sort()
    return dict(ms_median=chunks[len(chunks) // 2], ms_min=chunks[0], ms_max=chunks[-1], calls=n)


gen = torch.Generator().manual_seed(1)
x = torch.rand((512, 3, 32, 32), generator=gen).cuda()
y = torch.randint(0, 10, (512,), generator=gen).cuda()
kind, mode = what.split("_")
net = build(kind)
out = {"what": what, "precision": precision}
with ops.use_config(bf16_avgpool=True, bf16_lrt=True):
    rng.manual_seed(5, call=0)
    if mode == "infer":
        with torch.no_grad():
            lo, _ = ensemble.mc_forward(net, x, 10, precision=precision)
            out["path"] = ensemble.stats.get("path")
            out["checksum"] = float(lo.double().sum())
            out.update(timed(lambda: ensemble.mc_forward(net, x, 10, precision=precision)))
    else:
        opt = train.FusedAdam(net.parameters(), lr=1e-3)
        loss = train.train_step(net, opt, x, y, 10, 0.1, 50000.0, graph=False, precision=precision)[0]
        out["path"] = ensemble.stats.get("path")
        out["loss0"] = float(loss)
        out.update(timed(lambda: train.train_step(net, opt, x, y, 10, 0.1, 50000.0, graph=False, precision=precision)))
print(json.dumps(out))
