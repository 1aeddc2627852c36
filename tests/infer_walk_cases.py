"""The cases of tests/test_gpu_infer_walk_ref.py, shared with tests/test_infer_ref_cpu.py (which checks on the CPU that the cases
have teeth and that together they reach every form of the walk): the 44 recorded cases of tests/infer_schedule_recorder.py and a table
of small models with the geometry those lack.  No device.

    python tests/infer_walk_cases.py --write tests/golden/infer_walk_plans.json

rewrites the expected plans: per run the (form, in_layout, layout, pool, shared_in, rows > 1, tap_major) of every step ensemble.chwn_plan names (a
host-only query; no GPU needed), null where the walk does not apply.  Regenerate it only for an intended change of the planner and
read the diff: a run that silently moves off its form is what the file is there to catch."""
import functools
import json
import os
import sys

import torch
import torch.nn as nn

import infer_schedule_recorder as R

SEED, CALL0, CLASSES = R.SEED, R.CALL0, 10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infer_walk_plans.json")

# the bounds of the issue (tests/test_gpu_parity_fullsize.py's figures): ratio = max |got - want64| / max |want64| per slab
CAP, FLOOR_BBB, FLOOR_LRT, TWIN_FACTOR, BOUND_BF16, KL_RTOL = 2e-5, 4e-6, 1e-5, 4.0, 1e-2, 2e-6
# how far a wrong answer (another slab, the next call, the neighbouring batch block, a neighbouring image offset) must lie from the right
# one, in units of the run's bound: 100 bounds.  In bf16 that is one whole max |logit|: the table models meet it through their
# posterior (rho per model, below: noise as large as the weight means, so that two draws are unrelated answers).  The recorded cases
# cannot: the recorder builds them with rho = -5, which puts a wrong answer 7 % of max |logit| away at the closest (std-bbb, the
# neighbouring block), so for the recorded bf16 cases alone a wrong answer must lie 5 bounds away
SEPARATION, SEPARATION_RECORDED_BF16 = 100.0, 5.0


def separation(run):
    """How far a wrong answer must lie from the right one in this run, relative to max |want64|."""
    if run["precision"] == "bf16" and run["source"] == "recorded":
        return SEPARATION_RECORDED_BF16 * BOUND_BF16
    return SEPARATION * bound_of(run["precision"])


# an input channel set to zero must move every class logit by 100 fp32 bounds, in every model (a property of the model, which runs in
# every precision: one of three channels cannot move a logit by 100 bf16 bounds, a whole max |logit|)
LIVENESS = 100.0 * CAP


def bound_of(precision):
    return BOUND_BF16 if precision == "bf16" else CAP


# ---- the table -----------------------------------------------------------------------------------------------------------------
# (kind, args..., {options}): conv(cout, kernel, stride, padding, dilation) | fc(out) | relu | softplus | pool(k, s) |
# avg(kernel, stride, padding, count_include_pad) | gap | flatten(n).  Options of a layer: bias=False, prior_sigma=..., lrt=True / False
# (the mixed model: which kind this layer is, whatever the run's), lrt_k=(kernel, padding): what an LRT layer takes in place of a
# rectangular kernel (LRT convolutions take int kernels only, like the reference's; the map stays the same).  mu: the scale of the
# weight means (the deep model needs more for an input channel to reach the logits); rho: the mean of the posterior's rho -- the models
# that run in bf16 carry noise about as large as their weight means, so that two draws are unrelated answers, a whole max |logit|
# apart (100 bf16 bounds); seed (one, or one per kind): of the parameters, one at which that separation holds and no ReLU plane of the
# model is dead.  tests/test_infer_ref_cpu.py checks what these choices are for
def _m(B, E, cin, H, W, table, E_lrt=None, parts=False, kinds=("bbb", "lrt"), mu=0.1, seed=0, rho=-3.0):
    return dict(mu=mu, seed=seed, rho=rho, B=B, E=E, E_lrt=E if E_lrt is None else E_lrt, cin=cin, H=H, W=W, table=table, parts=parts,
                kinds=kinds)


_QUIRK = [("conv", 16, 3, 1, 1, 1), ("relu",), ("pool", 2, 2), ("flatten", 96), ("fc", 16), ("relu",), ("fc", CLASSES)]
MODELS = {
    # rectangular kernels, an overlapping pool that floor mode cuts, a 24-channel layer between 16-channel ones (c8s3 -> to_f32 ->
    # fp32 -> to_c8s3), dilation 2, a gapped pool, a 1 x 1 convolution
    "rect": _m(8, 2, 3, 20, 18, [("conv", 16, (3, 5), 1, (1, 2), 1, dict(lrt_k=(5, 2))), ("relu",), ("pool", 3, 2),
                                 ("conv", 24, (5, 1), 1, (2, 0), 1, dict(lrt_k=(5, 2))), ("softplus",),
                                 ("conv", 16, 3, 1, 2, 2), ("relu",), ("pool", 2, 3),
                                 ("conv", 16, 1, 1, 0, 1), ("softplus",), ("flatten", 144), ("fc", CLASSES)], rho=-1.5),
    # a stride-2 first layer, pools (3, 1) and (3, 2) between layers of the MFMA-ready chain (and of the S3 chain)
    "chain": _m(8, 2, 3, 18, 16, [("conv", 16, 3, 2, 1, 1), ("relu",), ("conv", 32, 3, 1, 1, 1), ("softplus",), ("pool", 3, 1),
                                  ("conv", 16, (3, 5), 1, (1, 2), 1, dict(lrt_k=(5, 2))), ("relu",), ("pool", 3, 2), ("flatten", 96), ("fc", 32), ("relu",),
                                  ("fc", CLASSES)], parts=True, seed=2, rho=-2.0),
    # stride 3 in the first layer, stride (2, 3) and padding beyond the kernel's reach in a later one, an average pool with padding
    # that reads negative values, a global-average-pool head
    "stride": _m(8, 2, 3, 19, 17, [("conv", 16, 5, 3, 2, 1), ("relu",), ("conv", 16, 3, (2, 3), 3, 1),
                                   ("avg", (3, 2), (2, 1), (1, 0), False), ("relu",), ("conv", 16, 3, 1, 1, 1), ("softplus",), ("gap",),
                                   ("flatten", 16), ("fc", CLASSES)], rho=-2.0),
    # a strided few-channel first layer in space-to-depth form (ops.s2d_layer_ok: square kernels, strides and paddings only) with its
    # fused pool; LRT with one draw (with more, an LRT first layer stays on the fp32 kernel)
    "s2d": _m(8, 2, 3, 20, 18, [("conv", 16, 7, 4, 5, 1), ("relu",), ("pool", 2, 2), ("conv", 16, 3, 1, 1, 1), ("relu",), ("pool", 3, 1),
                                ("flatten", 16), ("fc", CLASSES)], E_lrt=1, rho=-1.5, seed=9),
    # a pool right behind a layer, a stand-alone Softplus, a pool behind no layer; three draws
    "alone": _m(8, 3, 3, 16, 14, [("conv", 16, 3, 1, 1, 1), ("relu",), ("conv", 16, 3, 1, 1, 1), ("pool", 3, 2), ("softplus",),
                                  ("pool", 2, 3), ("flatten", 64), ("fc", 16), ("relu",), ("fc", CLASSES)], rho=-1.0, seed=dict(bbb=3, lrt=2)),
    # a flatten that cuts every image into five rows, layers behind it
    "quirk": _m(8, 2, 3, 12, 10, _QUIRK, parts=True),
    # ... and on an odd batch (the padding's rows come last and are dropped)
    "odd": _m(6, 2, 3, 12, 10, _QUIRK),
    # linear layers only, the first without bias; one draw
    "linear": _m(8, 1, 3, 4, 3, [("flatten", 36), ("fc", 32, dict(bias=False)), ("softplus",), ("fc", 24), ("relu",), ("fc", CLASSES)], rho=-2.0),
    # a layer without bias, two priors (one launch per layer in the parameter pass)
    "priors": _m(8, 2, 3, 10, 9, [("conv", 16, 3, 1, 1, 1, dict(bias=False)), ("relu",), ("pool", 2, 2),
                                  ("conv", 16, 3, 1, 1, 1, dict(prior_sigma=0.3)), ("softplus",), ("flatten", 320), ("fc", CLASSES)], rho=-2.0),
    # nine tiny layers: 18 parameter tensors, more than one chunk of the parameter pass
    "nine": _m(8, 2, 3, 8, 6, [("conv", 16, 3, 1, 1, 1), ("relu",)] + [("conv", 16, 1, 1, 0, 1), ("relu",)] * 4 + [("pool", 2, 2)] +
               [("conv", 16, (1, 3), 1, (0, 1), 1, dict(lrt_k=(3, 1))), ("relu",), ("flatten", 192), ("fc", 16), ("relu",), ("fc", 16), ("relu",),
                ("fc", CLASSES)], mu=0.3, rho=-0.5, seed=dict(bbb=8, lrt=7)),
    # a pooled first layer with a short contraction in front of a 32-channel 5 x 5 layer: the bf16 launch with MaxPool2d(3, 2) inside
    "pool32": _m(8, 2, 3, 14, 12, [("conv", 32, 5, 1, 2, 1), ("relu",), ("pool", 3, 2), ("conv", 16, 5, 1, 2, 1), ("relu",),
                                   ("pool", 3, 2), ("flatten", 64), ("fc", CLASSES)], rho=-0.5, seed=3),
    # BBB and LRT layers in one model (fp32 and bf16x3 only)
    "mixed": _m(8, 2, 3, 10, 8, [("conv", 16, 3, 1, 1, 1, dict(lrt=False)), ("relu",), ("pool", 3, 2),
                                 ("conv", 16, 3, 1, 1, 1, dict(lrt=True)), ("softplus",), ("flatten", 192), ("fc", 32, dict(lrt=False)),
                                 ("relu",), ("fc", CLASSES, dict(lrt=True))], kinds=("mixed",)),
}
PRIORS = {"prior_mu": 0, "prior_sigma": 0.1, "posterior_mu_initial": (0, 0.1), "posterior_rho_initial": (-3, 0.1)}
PARTS_B_OFFSET = 16                    # the partitioned table runs sit at a batch offset (a later shard of a batch-parallel job)


def build(name, kind):
    """The table model, parameters from a seeded CPU generator (the layers' own initialisation rule under PRIORS, redrawn here: the
    layers draw on whatever device they are built on, and the CPU tests must see the values the GPU runs use)."""
    from layers import BBB_Conv2d, BBB_LRT_Conv2d, BBB_Linear, BBB_LRT_Linear, FlattenLayer, ModuleWrapper
    from bbb_hip import rng
    spec = MODELS[name]
    seed = spec["seed"][kind] if isinstance(spec["seed"], dict) else spec["seed"]
    gen = torch.Generator().manual_seed(100 * seed + sorted(MODELS).index(name))
    net, cin, feat = ModuleWrapper(), spec["cin"], None
    for i, (what, *a) in enumerate(spec["table"]):
        opt = a.pop() if a and isinstance(a[-1], dict) else {}
        lrt = opt.get("lrt", kind == "lrt")
        pri = dict(PRIORS, prior_sigma=opt.get("prior_sigma", PRIORS["prior_sigma"]), posterior_mu_initial=(0, spec["mu"]),
                   posterior_rho_initial=(spec["rho"], 0.1))
        if what == "conv":
            if lrt and "lrt_k" in opt:
                a[1], a[3] = opt["lrt_k"]
            mod = (BBB_LRT_Conv2d if lrt else BBB_Conv2d)(cin, a[0], a[1], stride=a[2], padding=a[3], dilation=a[4],
                                                          bias=opt.get("bias", True), priors=pri)
            cin = a[0]
        elif what == "fc":
            mod = (BBB_LRT_Linear if lrt else BBB_Linear)(feat, a[0], bias=opt.get("bias", True), priors=pri)
            feat = a[0]
        elif what == "flatten":
            mod, feat = FlattenLayer(a[0]), a[0]
        else:
            mod = {"relu": nn.ReLU, "softplus": nn.Softplus, "pool": lambda: nn.MaxPool2d(a[0], a[1]),
                   "avg": lambda: nn.AvgPool2d(a[0], a[1], a[2], count_include_pad=a[3]), "gap": lambda: nn.AdaptiveAvgPool2d(1)}[what]()
        if what in ("conv", "fc"):
            for pname, (mean, std) in (("W_mu", pri["posterior_mu_initial"]), ("W_rho", pri["posterior_rho_initial"]),
                                       ("bias_mu", pri["posterior_mu_initial"]), ("bias_rho", pri["posterior_rho_initial"])):
                p = getattr(mod, pname)
                if p is not None:
                    p.data.copy_(torch.empty(tuple(p.shape)).normal_(mean, std, generator=gen))
            if mod.use_bias:
                mod.bias_mu.data.abs_()                  # (biases that keep ReLU planes alive)
        net.add_module(f"{what}{i}", mod)
    rng.assign_stream_ids(net)
    return net


def table_x(name, B):
    """Images in (-1, 1): both signs in front of the first layer."""
    spec = MODELS[name]
    g = torch.Generator().manual_seed(7 + sorted(MODELS).index(name))
    return torch.rand((B, spec["cin"], spec["H"], spec["W"]), generator=g) * 2.0 - 1.0


def recorded_x(case):
    return torch.rand(R.x_shape(case), generator=torch.Generator().manual_seed(6))         # (the recorder's _inputs, on the CPU)


def _has(spec, what):
    return any(t[0] == what for t in spec["table"])


def _configs(spec, kind):
    """{config name: (precision, LaunchConfig fields)}: every precision and configuration of the issue that can give the kind a plan
    of its own.  Pool fusion and the S3 chain exist for BBB models only (an all-LRT model under R.S3 is the x3-noc8 run, under R.FUSE
    the fp32 run), and a mixed model takes neither chain (its bf16x3 plan is its fp32 plan: one run says so)."""
    out = {"fp32": ("fp32", {}), "x3": ("bf16x3", {})}
    if kind == "bbb":
        out.update({"fp32-fuse": ("fp32", R.FUSE), "x3-s3": ("bf16x3", R.S3)})
    if kind != "mixed":
        out["x3-noc8"] = ("bf16x3", dict(c8x3=False))
    cfg = {}
    if kind in ("lrt", "mixed"):
        cfg["bf16_lrt"] = True
    if _has(spec, "avg") or _has(spec, "gap"):
        cfg["bf16_avgpool"] = True
    out["bf16"] = ("bf16", cfg)
    return out


# what the product refuses: run id -> (who refuses, its message).  "walk": _mc_logits_chwn raises; "mc_logits": the walk has no plan
# (it returns None before any launch) and its caller, which has no other bf16 path, raises.  The run asserts its plan first
_NO_BF16_PATH = ("mc_logits", "this model / input does not fit the batch-innermost path, which is the only bf16 path")
_BF16_BATCH = ("walk", "the bf16 path covers BBB (non-LRT) layers and batch sizes that are multiples of 8")
REFUSALS = {"priors-bbb-bf16": ("walk", "bf16 path: all layers must share one prior"),
            "mixed-mixed-bf16": ("walk", "bf16: a model mixes BBB and LRT layers (all one kind or the other)"),
            # a flatten that cuts images into rows has no bf16 form; an odd batch has no bf16 form either
            "quirk-bbb-bf16": _NO_BF16_PATH, "quirk-lrt-bf16": _NO_BF16_PATH, "odd-bbb-bf16": _BF16_BATCH, "odd-lrt-bf16": _BF16_BATCH}


def runs():
    """{run id: dict(source = "recorded" | "table", model, kind, precision, draws, B, cfg, kw[, refusal])}: the recorded cases under their own
    ids, the fall-back case, the table models as <model>-<kind>-<config>[-<partition>]."""
    out = {}
    for cid, case in R.cases().items():
        out[cid] = dict(case, source="recorded")
    out["fallback"] = dict(R.FALLBACK, source="recorded")
    for name, spec in MODELS.items():
        for kind in spec["kinds"]:
            draws = spec["E_lrt"] if kind == "lrt" else spec["E"]
            for cname, (precision, cfg) in _configs(spec, kind).items():
                out[f"{name}-{kind}-{cname}"] = dict(source="table", model=name, kind=kind, precision=precision, draws=draws, B=spec["B"],
                                                     cfg=dict(cfg), kw={}, refusal=REFUSALS.get(f"{name}-{kind}-{cname}"))
            if spec["parts"]:
                for cname in ("fp32", "x3"):
                    precision, cfg = _configs(spec, kind)[cname]
                    for pname, part in R.PARTS.items():
                        kw = {k: v for k, v in part.items() if k != "B"}
                        if pname != "streams2":
                            kw["b_offset"] = PARTS_B_OFFSET
                        out[f"{name}-{kind}-{cname}-{pname}"] = dict(source="table", model=name, kind=kind, precision=precision, draws=draws,
                                                                     B=part.get("B", spec["B"]), cfg=dict(cfg), kw=kw)
    return out


def run_model(run):
    """(net on the CPU with its stream ids, x on the CPU) of a run."""
    from bbb_hip import rng
    if run["source"] == "recorded":
        net = R.build(run["model"], run["kind"])
        rng.assign_stream_ids(net)
        return net, recorded_x(run)
    return build(run["model"], run["kind"]), table_x(run["model"], run["B"])


def has_lrt(run):
    return run["kind"] in ("lrt", "mixed")


def x_shape(run):
    if run["source"] == "recorded":
        return R.x_shape(run)
    spec = MODELS[run["model"]]
    return (run["B"], spec["cin"], spec["H"], spec["W"])


# ---- the plans -----------------------------------------------------------------------------------------------------------------
def _plain(v):
    if v is None or isinstance(v, (bool, int, str)):
        return v
    return [_plain(a) for a in v]


def plan_tuples(steps):
    """[(form, in_layout, layout, pool, shared_in, rows > 1, tap_major)] of a plan, JSON-plain.  pool: the window of a stand-alone pool [k, s],
    an average pool's [kernel, stride, padding, count_include_pad], the MaxPool2d inside a layer's launch ([2, 2] where the launch
    has only that one), else null."""
    out = []
    for st in steps:
        pool = st.pool
        if st.form == "pool":
            pool = [st.mod.kernel_size, st.mod.stride]
        elif pool is True:
            pool = [2, 2]
        out.append([st.form, st.in_layout, st.layout, _plain(pool), bool(st.shared_in), st.rows > 1, bool(st.tap_major)])
    return out


def plan_of(run, net):
    """What the planner says about a run under its configuration: plan_tuples, None (the walk does not apply), or
    {"refused": message} for a partition it refuses."""
    from bbb_hip import ensemble, ops, _lib
    kw = {k: v for k, v in run["kw"].items() if k in ("units", "groups", "share")}
    with ops.use_config(**run["cfg"]):
        try:
            steps = ensemble.chwn_plan(net, x_shape(run), run["draws"], run["precision"], **kw)
        except _lib.BBBHipError as e:
            return {"refused": str(e)}
    return None if steps is None else plan_tuples(steps)


# what the table is built to reach, written by hand from the models' tables: the forms, in order, of the runs that carry a model's
# purpose (tests/test_infer_ref_cpu.py holds the expected plans to it; the golden file has every run and every field)
INTENT = {
    # the 24-channel layer leaves the MFMA-ready chain and the next one rejoins it; the linear head joins it behind the flatten
    "rect-bbb-x3": "fp32_bbb pool to_c8s3 c8x3_bbb to_f32 fp32_bbb pool to_c8s3 c8x3_bbb to_f32 flatten to_c8s3 c8x3_bbb",
    # pools (3, 1) and (3, 2) inside the chain, in c8s3 and in s3
    "chain-bbb-x3": "fp32_bbb to_c8s3 c8x3_bbb pool c8x3_bbb pool to_f32 flatten to_c8s3 c8x3_bbb c8x3_bbb",
    "chain-bbb-x3-s3": "fp32_bbb fp32_bbb pool fp32_bbb pool flatten fp32_bbb fp32_bbb",
    # average pools behind both split layouts, a stand-alone ReLU behind the first
    "stride-bbb-x3": "fp32_bbb to_c8s3 c8x3_bbb to_f32 avgpool relu to_c8s3 c8x3_bbb to_f32 avgpool flatten to_c8s3 c8x3_bbb",
    "stride-bbb-x3-s3": "fp32_bbb fp32_bbb to_f32 avgpool relu fp32_bbb to_f32 avgpool flatten fp32_bbb",
    "stride-lrt-bf16": "bf16_lrt bf16_lrt avgpool relu bf16_lrt avgpool flatten bf16_lrt",
    # the space-to-depth first layer: BBB with its pool inside, LRT (one draw) with the pool behind it
    "s2d-bbb-x3": "s2d_bbb c8x3_bbb pool flatten c8x3_bbb",
    "s2d-lrt-x3": "s2d_lrt pool c8x3_lrt pool flatten c8x3_lrt",
    # a pool right behind a chain layer (c8s3), a stand-alone Softplus and a pool behind no layer (fp32)
    "alone-bbb-x3": "fp32_bbb to_c8s3 c8x3_bbb pool to_f32 softplus pool flatten to_c8s3 c8x3_bbb c8x3_bbb",
    # LRT chain layers behind a flatten that cuts images into rows
    "quirk-lrt-x3": "fp32_lrt pool flatten to_c8s3 c8x3_lrt c8x3_lrt",
    "linear-bbb-x3": "flatten fp32_bbb to_c8s3 c8x3_bbb to_f32 fp32_bbb",
    # the fp32 launch with MaxPool2d(2, 2) inside (the fifth layer), the bf16 launch with MaxPool2d(3, 2) inside (the first)
    "nine-bbb-fp32-fuse": "fp32_bbb fp32_bbb fp32_bbb fp32_bbb fp32_bbb fp32_bbb flatten fp32_bbb fp32_bbb fp32_bbb",
    "pool32-bbb-bf16": "bf16_bbb bf16_bbb pool flatten bf16_bbb",
    "mixed-mixed-fp32": "fp32_bbb pool fp32_lrt flatten fp32_bbb fp32_lrt",
}


@functools.lru_cache(maxsize=None)
def expected_plans():
    with open(GOLDEN) as f:
        return json.load(f)["plans"]


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "pytorch-bayesiancnn_amd"), os.path.join(root, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True, help="where the expected plans go (tests/golden/infer_walk_plans.json)")
    args = ap.parse_args(argv)
    plans, nets = {}, {}
    for rid, run in runs().items():
        key = (run["source"], run["model"], run["kind"])
        if key not in nets:
            nets[key] = run_model(run)[0]
        plans[rid] = plan_of(run, nets[key])
    doc = {"_comment": ["ensemble.chwn_plan of every run of tests/infer_walk_cases.py under the run's LaunchConfig:",
                        "[form, in_layout, layout, pool, shared_in, rows > 1, tap_major] per step; null: the walk does not apply.",
                        "Written by: python tests/infer_walk_cases.py --write tests/golden/infer_walk_plans.json"],
           "plans": plans}
    with open(args.write, "w") as f:
        f.write("{\n\"_comment\": " + json.dumps(doc["_comment"]) + ",\n\"plans\": {\n")
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in plans.items()))
        f.write("\n}\n}\n")
    print(f"{len(plans)} runs -> {args.write}")


if __name__ == "__main__":
    main(sys.argv[1:])
