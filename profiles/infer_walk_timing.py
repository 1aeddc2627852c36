"""Host wall time of one EAGER batch-innermost inference forward (ensemble._mc_logits_chwn, ending in a device synchronise): the
path of mc_logits and of the drop-in loop before its graph is built, which is bound by the host (the layer walk), not by the device.
3Conv3FC and AlexNet (BBB, softplus) at the bench's batch and draws, fp32 and bf16; after a warm-up, `--seconds` of calls per block.
    python profiles/infer_walk_timing.py                            one tree (this one): a JSON line per shape with the blocks' us per call
    python profiles/infer_walk_timing.py --against OTHER_TREE       this tree and another checkout (built), alternating block by block,
                                                                    each block a fresh process; the other tree's own run-to-run range is
                                                                    the measure: this tree's median may not be slower by more than it
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-5, 0.1)}
# name -> (model, batch, draws, precision)
SHAPES = {"3conv3fc-fp32": ("3conv3fc", 256, 10, "fp32"), "3conv3fc-bf16": ("3conv3fc", 256, 10, "bf16"),
          "alexnet-fp32": ("alexnet", 512, 10, "fp32"), "alexnet-bf16": ("alexnet", 512, 10, "bf16")}


def block(shape, seconds):
    """us per call over about `seconds` of calls (after a warm-up of a fifth of that)."""
    sys.path.insert(0, os.path.join(ROOT, "pytorch-bayesiancnn_amd"))
    import torch
    import layers  # noqa: F401
    from bbb_hip import ensemble, rng, zoo
    net_type, B, E, precision = SHAPES[shape]
    torch.manual_seed(0)
    net = zoo.getModel(net_type, 3, 10, PRIORS, "bbb", "softplus").cuda()
    rng.assign_stream_ids(net)
    x = torch.rand(B, 3, 32, 32, device="cuda")

    def calls(budget):
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget:
            ensemble._mc_logits_chwn(net, x, E, 7, n, precision=precision)
            torch.cuda.synchronize()
            n += 1
        return (time.perf_counter() - t0) / n * 1e6

    with torch.no_grad():
        calls(seconds / 5)
        return calls(seconds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--shape", choices=tuple(SHAPES))
    ap.add_argument("--against", metavar="TREE", help="another built checkout of this repository")
    ap.add_argument("--one-block", action="store_true", help="(the child processes of --against) one block of --shape, its us per call")
    a = ap.parse_args()
    if a.one_block:
        print(json.dumps(block(a.shape, a.seconds)), flush=True)
        return
    shapes = (a.shape,) if a.shape else tuple(SHAPES)
    if not a.against:
        for shape in shapes:
            v = [block(shape, a.seconds) for _ in range(a.blocks)]
            print(json.dumps(dict(shape=shape, us_per_call=[round(t, 1) for t in v])), flush=True)
        return
    trees = {"other": os.path.abspath(a.against), "this": ROOT}
    for shape in shapes:
        us = {k: [] for k in trees}
        for _ in range(a.blocks):
            for k, tree in trees.items():                       # the trees alternate; every block is a fresh process
                r = subprocess.run([sys.executable, os.path.join(tree, "profiles", "infer_walk_timing.py"), "--one-block", "--shape", shape,
                                    "--seconds", str(a.seconds)], capture_output=True, text=True, timeout=300, check=True)
                us[k].append(float(r.stdout.strip().splitlines()[-1]))
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        spread = max(us["other"]) - min(us["other"])
        print(json.dumps(dict(shape=shape, other_us=[round(t, 1) for t in us["other"]], this_us=[round(t, 1) for t in us["this"]],
                              other_median=round(med["other"], 1), this_median=round(med["this"], 1), other_range=round(spread, 1),
                              not_slower=med["this"] <= med["other"] + spread)), flush=True)


if __name__ == "__main__":
    main()
