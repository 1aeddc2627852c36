"""Recorder for what the per-launch wrappers of bbb_hip.ops hand to the C ABI, without a device: per case (i) every library entry the
wrapper calls, in order, with its bbb_conv_desc_t as hex bytes, every non-pointer scalar argument and which pointer arguments are
null, and (ii) the result's shapes and dtypes (for a plan query: its value), or the type of the exception it raises.
tests/test_launch_desc_cpu.py compares both with tests/golden/launch_desc.json.

    python tests/fwd_desc_recorder.py --write tests/golden/launch_desc.json --commit <the commit that is recorded>

rewrites the golden.  It is a record of ONE commit's descriptors: regenerate it only from a commit whose wrappers are the intended
ones, never to make a failing comparison pass.

The library is replaced by a stand-in that records every launch entry and returns 0; the host-only queries (*_plan,
bbb_conv2d_chwn_splitk_scratch) are recorded and then answered by the built library.  ops.require_device / cur_stream / on_device
and rng.call_dev_ptr are no-ops, the tensors are zero CPU tensors: pointer values are not recorded.

The cases use the smallest shapes that separate the branches: B = 8, 3 or 16 channels, 8 x 8 maps, 3 x 3 kernels, 2 or 3 slabs; every
wrapper also runs on a geometry whose stride, padding and dilation are unequal pairs (a swapped h / w shows in the bytes)."""
import ctypes
import json
import os
import sys

import torch

B, H, CO, K = 8, 8, 16, 3
SQ = dict(stride=1, padding=1, dilation=1)                          # 8 x 8 -> 8 x 8
RECT = dict(stride=(1, 2), padding=(2, 1), dilation=(2, 1))        # 8 x 8 -> 8 x 4
NOPAD = dict(stride=1, padding=0, dilation=1)                       # 8 x 8 -> 6 x 6 (the c8x3 pooled form takes no padding)
GEOMS = {"sq": SQ, "rect": RECT}
FORWARDED = ("bbb_conv2d_chwn_splitk_scratch",)


def f32(*s):
    return torch.zeros(s, dtype=torch.float32)


def bf(*s):
    return torch.zeros(s, dtype=torch.bfloat16)


def pitch(k):
    return (k + 7) & ~7


# ---- the slab forms: (name, Ex, Ew, keyword arguments); E is the number of output slabs ------------------------------------
BBB_SLABS = [("plain", 2, 2, {}), ("e1", 1, 1, {}), ("xshared", 1, 2, {}), ("wshared", 2, 1, {}),
             ("units", 3, 2, dict(units=(2, 1), n_units=3)), ("units-slice", 2, 2, dict(units=(2, 1), n_units=3, x_per_slice=True)),
             ("units-s1", 2, 2, dict(units=(1, 0), n_units=2)),
             ("xdiv", 2, 3, dict(x_div=2)), ("xdiv-off", 2, 3, dict(x_div=2, x_off=1)), ("xdiv-even", 2, 4, dict(x_div=2)),
             # refusals
             ("bad-lead", 3, 2, {}), ("bad-units", 2, 2, dict(units=(2, 1), n_units=3)),
             ("bad-units-slice", 3, 2, dict(units=(2, 1), n_units=3, x_per_slice=True)),
             ("bad-xdiv", 3, 3, dict(x_div=2)), ("bad-xoff", 2, 3, dict(x_div=2, x_off=2)), ("neg-xoff", 2, 3, dict(x_div=2, x_off=-1))]
LRT_SLABS = [("plain", 2, {}), ("e1", 1, {}), ("slabs-same", 2, dict(n_slabs=2)), ("xshared", 1, dict(n_slabs=3)),
             ("units", 3, dict(units=(2, 1), n_units=3)), ("units-slice", 2, dict(units=(2, 1), n_units=3, x_per_slice=True)),
             ("units-s1", 2, dict(units=(1, 0), n_units=2)),
             ("xdiv", 2, dict(x_div=2)), ("xdiv-off", 2, dict(x_div=2, x_off=1, n_slabs=3)), ("xdiv-slabs", 2, dict(x_div=2, n_slabs=3)),
             ("bad-slabs", 2, dict(n_slabs=3)), ("bad-units", 2, dict(units=(2, 1), n_units=3)),
             ("bad-units-slice", 3, dict(units=(2, 1), n_units=3, x_per_slice=True)),
             ("bad-xdiv", 3, dict(x_div=2, n_slabs=3)), ("bad-xoff", 2, dict(x_div=2, x_off=2, n_slabs=2))]
NO_UNITS = lambda slabs: [s for s in slabs if "units" not in s[-1]]


def _cases():
    """Yield (id, function(ops) -> result, LaunchConfig fields)."""
    seed, call0, sid = 11, 5, 7

    def case(cid, fn, **cfg):
        return cid, fn, cfg

    # ---- conv2d_chwn_forward ---------------------------------------------------------------------------------------------
    def chwn(Ex=2, Ew=2, cin=16, geom=SQ, b=B, bias=True, x=None, w=None, **kw):
        return lambda ops: ops.conv2d_chwn_forward(f32(Ex, cin, H, H, b) if x is None else x, f32(Ew, CO, cin, K, K) if w is None else w,
                                                   f32(Ew, CO) if bias else None, act="relu", **geom, **kw)
    for g, geom in GEOMS.items():
        for name, Ex, Ew, kw in BBB_SLABS:
            yield case(f"chwn/{g}/{name}", chwn(Ex, Ew, geom=geom, **kw))
        yield case(f"chwn/{g}/cin3", chwn(cin=3, geom=geom))
        yield case(f"chwn/{g}/nobias", chwn(geom=geom, bias=False))
        yield case(f"chwn/{g}/pool", chwn(geom=geom, pool=True))
        yield case(f"chwn/{g}/out", chwn(geom=geom, out=f32(2 * CO * 8 * (8 if g == "sq" else 4) * B)))
        yield case(f"chwn/{g}/tapmajor", chwn(geom=geom, w=f32(2, CO, K, K, 16), w_tap_major=True))
        yield case(f"chwn/{g}/s3-in", chwn(geom=geom, x=bf(2, 3, 16, H, H, B), x_s3=True))
        yield case(f"chwn/{g}/s3-in-shared", chwn(geom=geom, x=bf(1, 3, 16, H, H, B), x_s3=True))
        yield case(f"chwn/{g}/s3-in-xdiv", chwn(Ew=3, geom=geom, x=bf(2, 3, 16, H, H, B), x_s3=True, x_div=2, x_off=1))
        yield case(f"chwn/{g}/s3-out", chwn(geom=geom, out_s3=True))
        yield case(f"chwn/{g}/s3-both", chwn(geom=geom, x=bf(2, 3, 16, H, H, B), x_s3=True, out_s3=True))
        yield case(f"chwn/{g}/x3-on", chwn(geom=geom, bf16x3=True), bf16x3_min_workgroups=1)
        yield case(f"chwn/{g}/x3-small", chwn(geom=geom, bf16x3=True))
        yield case(f"chwn/{g}/x3-mode", chwn(geom=geom), gemm_mode="bf16x3", bf16x3_min_workgroups=1)
        yield case(f"chwn/{g}/x3-off", chwn(geom=geom, bf16x3=False), gemm_mode="bf16x3", bf16x3_min_workgroups=1)
        yield case(f"chwn/{g}/nosplitk", chwn(geom=geom), split_k=False)
    deep = lambda **kw: (lambda ops: ops.conv2d_chwn_forward(f32(2, 512, 2, 2, B), f32(2, CO, 512, K, K), f32(2, CO), padding=1, **kw))
    yield case("chwn/deep/splitk", deep())                              # a long contraction on a small map: the layer's split
    yield case("chwn/deep/nosplitk", deep(), split_k=False)
    yield case("chwn/deep/pool", deep(pool=True))                       # refused when the contraction is split
    yield case("chwn/act-none", lambda ops: ops.conv2d_chwn_forward(f32(2, 16, H, H, B), f32(2, CO, 16, K, K), None))
    yield case("chwn/act-softplus", lambda ops: ops.conv2d_chwn_forward(f32(2, 16, H, H, B), f32(2, CO, 16, K, K), None, act="softplus"))
    yield case("chwn/bad-cin", lambda ops: ops.conv2d_chwn_forward(f32(2, 16, H, H, B), f32(2, CO, 8, K, K), None))
    yield case("chwn/bad-tapmajor-s3", chwn(x=bf(2, 3, 16, H, H, B), x_s3=True, w=f32(2, CO, K, K, 16), w_tap_major=True))
    yield case("chwn/bad-tapmajor-x3", chwn(w=f32(2, CO, K, K, 16), w_tap_major=True, bf16x3=True))
    yield case("chwn/bad-s3-shape", chwn(x=bf(2, 16, H, H, B), x_s3=True))
    yield case("chwn/bad-s3-batch", chwn(x=bf(2, 3, 16, H, H, 4), x_s3=True))
    yield case("chwn/bad-s3-out-batch", chwn(b=4, out_s3=True))
    yield case("chwn/bad-pool-odd", chwn(geom=dict(stride=(1, 2), padding=0, dilation=1), pool=True))
    yield case("chwn/bad-pool-s3", chwn(out_s3=True, pool=True))
    yield case("chwn/bad-out-size", chwn(out=f32(7)))
    yield case("chwn/bad-out-dtype", chwn(out=bf(2 * CO * 8 * 8 * B)))
    yield case("chwn/bad-act", lambda ops: ops.conv2d_chwn_forward(f32(2, 16, H, H, B), f32(2, CO, 16, K, K), None, act="tanh"))

    # ---- conv2d_c8x3_forward ---------------------------------------------------------------------------------------------
    def c8x3(Ex=2, Ew=2, geom=SQ, cout=CO, x=None, w=None, **kw):
        return lambda ops: ops.conv2d_c8x3_forward(bf(Ex, 3, 2, H, H, B, 8) if x is None else x, f32(Ew, cout, K * K, 16) if w is None else w,
                                                   f32(Ew, cout), K, act="relu", **geom, **kw)
    for g, geom in GEOMS.items():
        for name, Ex, Ew, kw in BBB_SLABS:
            yield case(f"c8x3/{g}/{name}", c8x3(Ex, Ew, geom=geom, **kw))
        wo = 8 if g == "sq" else 4
        yield case(f"c8x3/{g}/out-f32", c8x3(geom=geom, out_f32=True))
        yield case(f"c8x3/{g}/out", c8x3(geom=geom, out=bf(2, 3, CO // 8, 8, wo, B, 8)))
        yield case(f"c8x3/{g}/out-f32-out", c8x3(geom=geom, out_f32=True, out=f32(2 * CO * 8 * wo * B)))
        yield case(f"c8x3/{g}/border", c8x3(geom=geom, zero_border=(1, 2, 3, 20)))
        for tile in (128, 256):
            yield case(f"c8x3/{g}/tile{tile}", c8x3(geom=geom, tile=tile))
        for nt in (2, 3, 4):
            yield case(f"c8x3/{g}/nt{nt}", c8x3(geom=geom, nt=nt, tile=128))
    yield case("c8x3/nopad/pool", c8x3(geom=NOPAD, pool=True))
    yield case("c8x3/nopad/pool-tile32", c8x3(geom=NOPAD, pool=True, tile=32, zero_border=(1, 0, 0, 1)))
    yield case("c8x3/nopad/pool-tile64-units", c8x3(3, 2, geom=NOPAD, pool=True, tile=64, units=(2, 1), n_units=3))
    yield case("c8x3/cout12-f32", c8x3(cout=12, out_f32=True))
    yield case("c8x3/bad-shape", c8x3(x=bf(2, 6, 2, H, H, B, 8)))
    yield case("c8x3/bad-weights", c8x3(w=f32(2, CO, K * K, 8)))
    yield case("c8x3/bad-taps", c8x3(w=f32(2, CO, 4, 16)))
    yield case("c8x3/bad-pool-pad", c8x3(pool=True))
    yield case("c8x3/bad-pool-f32", c8x3(geom=NOPAD, pool=True, out_f32=True))
    yield case("c8x3/bad-pool-odd", c8x3(geom=dict(stride=(1, 2), padding=0, dilation=1), pool=True))
    yield case("c8x3/bad-cout", c8x3(cout=12))
    yield case("c8x3/bad-out", c8x3(out=bf(5)))
    yield case("c8x3/bad-tile", c8x3(tile=100))
    yield case("c8x3/bad-nt", c8x3(nt=5))

    # ---- lrt_conv2d_c8x3_forward -----------------------------------------------------------------------------------------
    def lrt_c8x3(Ex=2, geom=SQ, cout=CO, x=None, w=None, **kw):
        w = f32(cout, K * K, 16) if w is None else w
        return lambda ops: ops.lrt_conv2d_c8x3_forward(bf(Ex, 6, 2, H, H, B, 8) if x is None else x, w, w.clone(), f32(cout), f32(cout), K,
                                                       seed, call0, sid, act="relu", **geom, **kw)
    for g, geom in GEOMS.items():
        for name, Ex, kw in LRT_SLABS:
            yield case(f"lrt-c8x3/{g}/{name}", lrt_c8x3(Ex, geom=geom, **kw))
        wo = 8 if g == "sq" else 4
        yield case(f"lrt-c8x3/{g}/out-f32", lrt_c8x3(geom=geom, out_f32=True, sample=False))
        yield case(f"lrt-c8x3/{g}/out", lrt_c8x3(geom=geom, out=bf(2, 6, CO // 8, 8, wo, B, 8)))
        yield case(f"lrt-c8x3/{g}/boffset", lrt_c8x3(geom=geom, b_offset=24))
        yield case(f"lrt-c8x3/{g}/border-tile", lrt_c8x3(geom=geom, zero_border=(1, 2, 3, 20), tile=256))
        yield case(f"lrt-c8x3/{g}/tile128", lrt_c8x3(geom=geom, tile=128))
    yield case("lrt-c8x3/bad-shape", lrt_c8x3(x=bf(2, 3, 2, H, H, B, 8)))
    yield case("lrt-c8x3/bad-weights", lrt_c8x3(w=f32(CO, K * K, 8)))
    yield case("lrt-c8x3/bad-cout", lrt_c8x3(cout=12))
    yield case("lrt-c8x3/bad-out", lrt_c8x3(out=bf(5)))
    yield case("lrt-c8x3/bad-tile", lrt_c8x3(tile=32))

    # ---- lrt_conv2d_chwn_forward -----------------------------------------------------------------------------------------
    def lrt_chwn(Ex=2, cin=16, geom=SQ, w=None, x=None, **kw):
        w = f32(CO, cin, K, K) if w is None else w
        return lambda ops: ops.lrt_conv2d_chwn_forward(f32(Ex, cin, H, H, B) if x is None else x, w, w.clone(), f32(CO), f32(CO), seed, call0, sid,
                                                       act="softplus", **geom, **kw)
    for g, geom in GEOMS.items():
        for name, Ex, kw in LRT_SLABS:
            yield case(f"lrt-chwn/{g}/{name}", lrt_chwn(Ex, geom=geom, **kw))
        wo = 8 if g == "sq" else 4
        yield case(f"lrt-chwn/{g}/cin3", lrt_chwn(cin=3, geom=geom))
        yield case(f"lrt-chwn/{g}/pool", lrt_chwn(geom=geom, pool=True))
        yield case(f"lrt-chwn/{g}/moments", lrt_chwn(geom=geom, want_moments=True, sample=False))
        yield case(f"lrt-chwn/{g}/eps", lrt_chwn(geom=geom, eps=f32(2, CO, 8, wo, B)))
        yield case(f"lrt-chwn/{g}/boffset", lrt_chwn(geom=geom, b_offset=24))
        yield case(f"lrt-chwn/{g}/nosplitk", lrt_chwn(geom=geom), split_k=False)
    lrt_deep = lambda **kw: lrt_chwn(x=f32(2, 512, 2, 2, B), w=f32(CO, 512, K, K), geom=SQ, **kw)
    yield case("lrt-chwn/deep/splitk", lrt_deep())
    yield case("lrt-chwn/deep/nosplitk", lrt_deep(), split_k=False)
    yield case("lrt-chwn/deep/pool", lrt_deep(pool=True))
    yield case("lrt-chwn/bad-cin", lrt_chwn(w=f32(CO, 8, K, K)))
    yield case("lrt-chwn/bad-pool-moments", lrt_chwn(pool=True, want_moments=True))
    yield case("lrt-chwn/bad-pool-odd", lrt_chwn(geom=dict(stride=(1, 2), padding=0, dilation=1), pool=True))

    # ---- conv2d_chwn_bf16_forward ----------------------------------------------------------------------------------------
    def bf16(Ex=2, Ew=2, cin=16, geom=SQ, cout=CO, bias=True, x=None, w=None, act="relu", **kw):
        return lambda ops: ops.conv2d_chwn_bf16_forward(bf(Ex, cin, H, H, B) if x is None else x,
                                                        bf(Ew, cout, pitch(cin * K * K)) if w is None else w,
                                                        f32(Ew, cout) if bias else None, (cin, K, K), act=act, **geom, **kw)
    for g, geom in GEOMS.items():
        for name, Ex, Ew, kw in BBB_SLABS:
            yield case(f"bf16/{g}/{name}", bf16(Ex, Ew, geom=geom, **kw))
        wo = 8 if g == "sq" else 4
        yield case(f"bf16/{g}/cin3", bf16(cin=3, geom=geom))
        yield case(f"bf16/{g}/nobias", bf16(geom=geom, bias=False))
        yield case(f"bf16/{g}/nobias-wshared", bf16(2, 1, geom=geom, bias=False))
        yield case(f"bf16/{g}/out-f32", bf16(geom=geom, out_f32=True))
        yield case(f"bf16/{g}/out", bf16(geom=geom, out=bf(2 * CO * 8 * wo * B)))
        yield case(f"bf16/{g}/tapmajor", bf16(geom=geom, tap_major=True))
        yield case(f"bf16/{g}/pool22", bf16(cin=3, geom=geom, pool=(2, 2)))
        yield case(f"bf16/{g}/pool32", bf16(cin=3, geom=geom, pool=(3, 2)))
        yield case(f"bf16/{g}/pool22-outc8-units", bf16(3, 2, cin=3, geom=geom, pool=(2, 2), out_c8=True, units=(2, 1), n_units=3))
        yield case(f"bf16/{g}/c8-in", bf16(geom=geom, x=bf(2, 2, H, H, B, 8), tap_major=True))
        yield case(f"bf16/{g}/c8-in-shared", bf16(geom=geom, x=bf(1, 2, H, H, B, 8), tap_major=True))
        yield case(f"bf16/{g}/c8-out", bf16(geom=geom, out_c8=True))
        yield case(f"bf16/{g}/c8-both-out", bf16(geom=geom, x=bf(2, 2, H, H, B, 8), tap_major=True, out_c8=True, out=bf(2, CO // 8, 8, wo, B, 8)))
    yield case("bf16/act-none", bf16(act=None))
    yield case("bf16/bad-c8-in", bf16(x=bf(2, 2, H, H, B, 4)))
    yield case("bf16/bad-pitch", bf16(w=bf(2, CO, 100)))
    yield case("bf16/bad-cin", bf16(x=bf(2, 8, H, H, B)))
    yield case("bf16/bad-outc8-f32", bf16(out_c8=True, out_f32=True))
    yield case("bf16/bad-outc8-cout", bf16(cout=12, out_c8=True))
    yield case("bf16/bad-out", bf16(out=bf(5)))
    yield case("bf16/bad-out-dtype", bf16(out=f32(2 * CO * 8 * 8 * B)))
    yield case("bf16/bad-act", bf16(act="tanh"))

    # ---- lrt_conv2d_chwn_bf16_forward ------------------------------------------------------------------------------------
    def lrt_bf16(Ex=2, cin=16, geom=SQ, x=None, w=None, **kw):
        w = bf(CO, pitch(cin * K * K)) if w is None else w
        return lambda ops: ops.lrt_conv2d_chwn_bf16_forward(bf(Ex, cin, H, H, B) if x is None else x, w, w.clone(), f32(CO), f32(CO), (cin, K, K),
                                                            seed, call0, sid, act="relu", **geom, **kw)
    for g, geom in GEOMS.items():
        for name, Ex, kw in NO_UNITS(LRT_SLABS):
            yield case(f"lrt-bf16/{g}/{name}", lrt_bf16(Ex, geom=geom, **kw))
        wo = 8 if g == "sq" else 4
        yield case(f"lrt-bf16/{g}/cin3", lrt_bf16(cin=3, geom=geom))
        yield case(f"lrt-bf16/{g}/moments", lrt_bf16(geom=geom, want_moments=True))
        yield case(f"lrt-bf16/{g}/moments-only", lrt_bf16(geom=geom, moments_only=True, sample=False))
        yield case(f"lrt-bf16/{g}/out-f32", lrt_bf16(geom=geom, out_f32=True))
        yield case(f"lrt-bf16/{g}/out", lrt_bf16(geom=geom, out=bf(2 * CO * 8 * wo * B)))
        yield case(f"lrt-bf16/{g}/tapmajor-boffset", lrt_bf16(geom=geom, tap_major=True, b_offset=24))
    yield case("lrt-bf16/bad-pitch", lrt_bf16(w=bf(CO, 100)))
    yield case("lrt-bf16/bad-cin", lrt_bf16(x=bf(2, 8, H, H, B)))
    yield case("lrt-bf16/bad-moments-only", lrt_bf16(moments_only=True))
    yield case("lrt-bf16/bad-out", lrt_bf16(out=bf(5)))

    # ---- the reference-layout wrappers -----------------------------------------------------------------------------------
    for g, geom in GEOMS.items():
        for name, Ex, Ew in (("plain", 2, 2), ("xshared", 1, 2), ("wshared", 2, 1), ("e1", 1, 1), ("bad-lead", 3, 2)):
            yield case(f"nchw/{g}/{name}", lambda ops, Ex=Ex, Ew=Ew, geom=geom: ops.conv2d_forward(f32(Ex, B, 16, H, H), f32(Ew, CO, 16, K, K), f32(Ew, CO),
                                                                                                   act="relu", **geom))
        yield case(f"nchw/{g}/nobias-cin3", lambda ops, geom=geom: ops.conv2d_forward(f32(2, B, 3, H, H), f32(2, CO, 3, K, K), None, **geom))
        wo = 8 if g == "sq" else 4
        for name, kw in (("plain", {}), ("moments", dict(want_moments=True, sample=False)), ("eps", dict(eps=f32(2, B, CO, 8, wo))),
                         ("bad-eps", dict(eps=f32(5)))):
            yield case(f"lrt-nchw/{g}/{name}", lambda ops, kw=kw, geom=geom: ops.lrt_conv2d_forward(f32(2, B, 16, H, H), f32(CO, 16, K, K), f32(CO, 16, K, K),
                                                                                                    f32(CO), f32(CO), seed, call0, sid, act="relu", **geom, **kw))
    yield case("nchw/bad-cin", lambda ops: ops.conv2d_forward(f32(2, B, 16, H, H), f32(2, CO, 8, K, K), None))
    yield case("lrt-nchw/bad-cin", lambda ops: ops.lrt_conv2d_forward(f32(2, B, 16, H, H), f32(CO, 8, K, K), f32(CO, 8, K, K), None, None, seed, call0, sid))

    # ---- the gradient wrappers -------------------------------------------------------------------------------------------
    # (layer: 16 -> CO channels, 3 x 3 on an 8 x 8 map; "s2": stride 2, padding 1 -> 4 x 4; "rect": RECT -> 8 x 4)
    GRAD = {"sq": (SQ, 8, 8), "s2": (dict(stride=2, padding=1, dilation=1), 4, 4), "rect": (RECT, 8, 4)}
    for g, (geom, ho, wo) in GRAD.items():
        s, p, dl = geom["stride"], geom["padding"], geom["dilation"]
        for name, Eg, Ew in (("plain", 2, 2), ("wshared", 2, 1), ("gshared", 1, 2)):
            yield case(f"dgrad/{g}/{name}", lambda ops, Eg=Eg, Ew=Ew, ho=ho, wo=wo, s=s, p=p, dl=dl: ops.conv2d_chwn_input_grad(
                f32(Eg, CO, ho, wo, B), f32(Ew, CO, 16, K, K), (H, H), p, dl, stride=s))
            yield case(f"dgrad-bf16/{g}/{name}", lambda ops, Eg=Eg, Ew=Ew, ho=ho, wo=wo, s=s, p=p, dl=dl: ops.conv2d_chwn_input_grad_bf16(
                bf(Eg, CO, ho, wo, B), bf(Ew, CO, pitch(16 * K * K)), (CO, 16, K, K), (H, H), p, dl, stride=s))
        yield case(f"dgrad/{g}/flipped", lambda ops, ho=ho, wo=wo, s=s, p=p, dl=dl: ops.conv2d_chwn_input_grad(
            f32(2, CO, ho, wo, B), f32(2, CO, 16, K, K), (H, H), p, dl, w_flipped=f32(2, 16, CO, K, K), stride=s))
        yield case(f"dgrad/{g}/bad-pad", lambda ops, ho=ho, wo=wo, s=s, dl=dl: ops.conv2d_chwn_input_grad(
            f32(2, CO, ho, wo, B), f32(2, CO, 16, K, K), (H, H), 9, dl, stride=s))
        yield case(f"dgrad-bf16/{g}/bad-pad", lambda ops, ho=ho, wo=wo, s=s, dl=dl: ops.conv2d_chwn_input_grad_bf16(
            bf(2, CO, ho, wo, B), bf(2, CO, pitch(16 * K * K)), (CO, 16, K, K), (H, H), 9, dl, stride=s))
        yield case(f"wgrad/{g}", lambda ops, ho=ho, wo=wo, geom=geom: ops.conv2d_chwn_weight_grad(
            f32(2, CO, ho, wo, B), f32(2, 16, H, H, B), (2, CO, 16, K, K), **geom))
        yield case(f"wgrad/{g}/squares", lambda ops, ho=ho, wo=wo, geom=geom: ops.conv2d_chwn_weight_grad(
            f32(2, CO, ho, wo, B), f32(1, 16, H, H, B), (1, CO, 16, K, K), x_squares=True, **geom))
        yield case(f"wgrad-bf16/{g}", lambda ops, ho=ho, wo=wo, geom=geom: ops.conv2d_chwn_weight_grad_bf16(
            bf(2, CO, ho, wo, B), bf(2, 16, H, H, B), (2, CO, 16, K, K), **geom))
        yield case(f"im2col/{g}", lambda ops, geom=geom: ops.im2col_pbj(f32(B, 3, H, H), (1, CO, 3, K, K), **geom))
        yield case(f"wgrad-shared/{g}", lambda ops, ho=ho, wo=wo, geom=geom: ops.conv2d_chwn_weight_grad_shared_input(
            f32(2, CO, ho, wo, B), f32(B, 3, H, H), (2, CO, 3, K, K), **geom))
        yield case(f"first-dgrad/{g}", lambda ops, ho=ho, wo=wo, geom=geom: ops.first_layer_input_grad(
            f32(2, CO, ho, wo, B), f32(2, CO, 3, K, K), (H, H), **geom))
        yield case(f"first-dgrad/{g}/lrt", lambda ops, ho=ho, wo=wo, geom=geom: ops.first_layer_input_grad(
            (f32(1, CO, ho, wo, B), f32(1, CO, ho, wo, B)), (f32(CO, 3, K, K), f32(CO, 3, K, K)), (H, H), x_lrt=f32(B, 3, H, H), **geom))
    yield case("dgrad/s2/bad-lead", lambda ops: ops.conv2d_chwn_input_grad(f32(3, CO, 4, 4, B), f32(2, CO, 16, K, K), (H, H), 1, 1, stride=2))
    yield case("dgrad/s2/bad-stride", lambda ops: ops.conv2d_chwn_input_grad(f32(2, CO, 4, 4, B), f32(2, CO, 16, K, K), (H, H), 1, 1, stride=(2, 0)))
    yield case("dgrad/sq/bad-map", lambda ops: ops.conv2d_chwn_input_grad(f32(2, CO, 8, 8, B), f32(2, CO, 16, K, K), (9, 8), 1, 1))
    yield case("dgrad-bf16/s2/bad-lead", lambda ops: ops.conv2d_chwn_input_grad_bf16(bf(3, CO, 4, 4, B), bf(2, CO, pitch(16 * K * K)), (CO, 16, K, K), (H, H), 1, 1,
                                                                                       stride=2))
    yield case("dgrad-bf16/s2/bad-rows", lambda ops: ops.conv2d_chwn_input_grad_bf16(bf(2, 8, 4, 4, B), bf(2, CO, pitch(16 * K * K)), (CO, 16, K, K), (H, H), 1, 1,
                                                                                       stride=2))
    yield case("wgrad-shared/bad-xk", lambda ops: ops.conv2d_chwn_weight_grad_shared_input(f32(2, CO, 8, 8, B), None, (2, CO, 3, K, K), **SQ, xk=f32(5, B, 28)))
    yield case("first-dgrad/bad-map", lambda ops: ops.first_layer_input_grad(f32(2, CO, 8, 8, B), f32(2, CO, 3, K, K), (9, 8), **SQ))

    # ---- the plan queries ------------------------------------------------------------------------------------------------
    for g, geom in GEOMS.items():
        for name, kw in (("bbb", {}), ("lrt", dict(lrt=True)), ("pool", dict(pool=True)), ("lrt-pool", dict(lrt=True, pool=True)),
                         ("draws", dict(draws=5)), ("ksplit", dict(k_split=2)), ("noscratch", dict(scratch=False))):
            yield case(f"fp32-plan/{g}/{name}", lambda ops, kw=kw, geom=geom: ops.fp32_fwd_plan((2, 16, H, H, B), (2, CO, 16, K, K), **geom, **kw))
        yield case(f"fp32-plan/{g}/nosplitk", lambda ops, geom=geom: ops.fp32_fwd_plan((2, 16, H, H, B), (2, CO, 16, K, K), **geom), split_k=False)
        for name, cin, kw in (("plain", 16, {}), ("flags", 16, dict(out_f32=True, tap_major=True)), ("c8", 16, dict(tap_major=True, x_c8=True, out_c8=True)),
                              ("pool22", 3, dict(pool=(2, 2))), ("pool32", 3, dict(pool=(3, 2))), ("draws", 16, dict(draws=5))):
            yield case(f"bf16-plan/{g}/{name}", lambda ops, cin=cin, kw=kw, geom=geom: ops.bf16_fwd_plan((2, cin, H, H, B), CO, (cin, K, K), **geom, **kw))
        yield case(f"lrt-bf16-plan/{g}", lambda ops, geom=geom: ops.lrt_bf16_plan((2, 16, H, H, B), CO, (16, K, K), **geom))
        yield case(f"lrt-bf16-plan/{g}/draws", lambda ops, geom=geom: ops.lrt_bf16_plan((2, 16, H, H, B), CO, (16, K, K), draws=5, **geom))
        yield case(f"pool-rule/{g}", lambda ops, geom=geom: ops._pool_fusion_rule((2, 16, H, H, B), (2, CO, 16, K, K), geom["stride"], geom["padding"],
                                                                                   geom["dilation"], 2, torch.nn.MaxPool2d(2, 2)),
                   pool_fuse_min_items=1, pool_fuse_imbalance=1e9)
        yield case(f"pool-rule/{g}/default", lambda ops, geom=geom: ops._pool_fusion_rule((16, H, H, B), (CO, 16, K, K), geom["stride"], geom["padding"],
                                                                                           geom["dilation"], 2, None))
    yield case("fp32-plan/deep", lambda ops: ops.fp32_fwd_plan((2, 512, 2, 2, B), (2, CO, 512, K, K), padding=1))
    yield case("fp32-plan/bad-ksplit", lambda ops: ops.fp32_fwd_plan((2, 16, H, H, B), (2, CO, 16, K, K), k_split=3, pool=True))
    yield case("pool-rule/odd", lambda ops: ops._pool_fusion_rule((2, 16, 7, 7, B), (2, CO, 16, K, K), 1, 0, 1, 2, None),
               pool_fuse_min_items=1, pool_fuse_imbalance=1e9)
    yield case("pool-rule/pool3", lambda ops: ops._pool_fusion_rule((2, 16, H, H, B), (2, CO, 16, K, K), 1, 1, 1, 2, torch.nn.MaxPool2d(3, 2)))
    yield case("pool-rule/deep", lambda ops: ops._pool_fusion_rule((2, 512, 2, 2, B), (2, CO, 512, K, K), 1, 1, 1, 2, None),
               pool_fuse_min_items=1, pool_fuse_imbalance=1e9)
    for name, stride, dl in (("s2", 2, 1), ("rect", (1, 2), (2, 1))):
        yield case(f"bf16-dgrad-form/{name}", lambda ops, stride=stride, dl=dl: ops.bf16_dgrad_form(B, 16, CO, K, K, (H, H), stride, dl, 2))
    yield case("bf16-dgrad-form/cout12", lambda ops: ops.bf16_dgrad_form(B, 16, 12, K, K, (H, H), 2, 1, 3))


def cases():
    """{case id: (function(ops) -> result, LaunchConfig fields)}."""
    out = {}
    for cid, fn, cfg in _cases():
        assert cid not in out, cid
        out[cid] = (fn, cfg)
    return out


# ---- the stand-in library ----------------------------------------------------------------------------------------------------
class Lib:
    """Stand-in for the ctypes handle: every entry is recorded into `log`; launches return 0, host-only queries the built library's
    answer."""

    def __init__(self, _lib, real):
        self._sig, self._real, self.log = _lib._SIGNATURES, real, []
        self._desc = ctypes.POINTER(_lib.ConvDesc)

    def __getattr__(self, name):
        argtypes = self._sig[name][1]                  # (an entry the binding does not declare: KeyError)
        host = name.endswith("_plan") or name in FORWARDED

        def entry(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            rec = {"entry": name, "args": []}
            for t, a in zip(argtypes, args):
                if t is self._desc:
                    rec["desc"] = bytes(a._obj).hex()
                elif t is ctypes.c_void_p:
                    rec["args"].append("null" if not a else "ptr")
                elif isinstance(t, type) and issubclass(t, ctypes._Pointer):
                    rec["args"].append("ref")
                else:
                    rec["args"].append(a)
            self.log.append(rec)
            return getattr(self._real, name)(*args) if host else 0
        return entry


def _shape(v):
    if torch.is_tensor(v):
        return [list(v.shape), str(v.dtype)]
    if isinstance(v, (tuple, list)):
        return [_shape(u) for u in v]
    return v


def record(fn, cfg, monkeypatch):
    """-> dict(calls, out | raises): one case under the stand-in library."""
    from bbb_hip import _lib, ops, rng
    lib = Lib(_lib, _lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    monkeypatch.setattr(ops, "require_device", lambda *a, **k: None)
    monkeypatch.setattr(ops, "cur_stream", lambda device: 0)
    monkeypatch.setattr(ops, "on_device", lambda device: _lib._NO_GUARD)
    monkeypatch.setattr(rng, "call_dev_ptr", lambda device: 0)
    for cache in (ops._scratch, ops._split_plans, ops._pool_rule_cache):     # (per-process caches: a case must not depend on the ones before it)
        cache.clear()
    res = {}
    with torch.no_grad(), ops.use_config(ops.LaunchConfig(**cfg)):
        try:
            res["out"] = _shape(fn(ops))
        except Exception as e:                                               # noqa: BLE001  (the type is the record)
            res["raises"] = type(e).__name__
    res["calls"] = lib.log
    return json.loads(json.dumps(res))


def record_all():
    import pytest
    out = {}
    for cid, (fn, cfg) in cases().items():
        with pytest.MonkeyPatch.context() as mp:
            out[cid] = record(fn, cfg, mp)
    return out


def main(argv):
    import argparse
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "pytorch-bayesiancnn_amd"), os.path.join(root, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True, help="where the golden goes (tests/golden/launch_desc.json)")
    ap.add_argument("--commit", required=True, help="the commit whose wrappers are recorded")
    args = ap.parse_args(argv)
    out = record_all()
    assert out == record_all(), "two recordings differ"
    doc = {"_comment": ["What the per-launch wrappers of bbb_hip.ops hand to the C ABI, recorded by tests/fwd_desc_recorder.py (no device needed).",
                        f"Produced from commit {args.commit} by:",
                        f"  python tests/fwd_desc_recorder.py --write tests/golden/launch_desc.json --commit {args.commit}",
                        "calls: the library entries in order -- desc: bbb_conv_desc_t as hex, args: the other arguments (scalars by value, "
                        "pointers as null / ptr, by-reference outputs and arrays as ref); out: the result's [shape, dtype] (a plan query's value); "
                        "raises: the exception type."],
           "cases": out}
    with open(args.write, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    n = sum(1 for c in out.values() if "raises" in c)
    print(f"{len(out)} cases ({n} refusals), {sum(len(c['calls']) for c in out.values())} calls -> {args.write}")


if __name__ == "__main__":
    main(sys.argv[1:])
