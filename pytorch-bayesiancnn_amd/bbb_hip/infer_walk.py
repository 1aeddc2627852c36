"""The batch-innermost inference forward behind ensemble._mc_logits_chwn, in pieces that can be read and tested one by one:

    chwn_partition   how a call is cut up (work units, several steps per launch, a share of a group of steps, an odd batch): pure
    _chwn_steps      which launch every layer takes, as a list of ChwnStep: pure (module list, shapes, partition, LaunchConfig);
                     ensemble.chwn_plan asks it for a CPU model
    _chwn_walk       one loop over the steps: one prologue per Bayesian layer, one short launch function per form

The launches in front of the walk (ensemble._chwn_operands) and the entry stay in ensemble."""
import collections
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, pool_desc, _lib
from .conv_desc import out_map, pooled_map  # (queries, not launches: asked directly, as pool_desc is)
from layers.bbb import _BBBLayer, BBBConv2d as _BBBConv
from layers.lrt import _LRTLayer, BBBConv2d as _LRTConv
from layers.misc import FlattenLayer


def _run(timers, tag, info, fn):
    return timers.bracket(tag, info, fn) if timers is not None else fn()


def _act_name(mod):
    if isinstance(mod, nn.ReLU):
        return "relu"
    if isinstance(mod, nn.Softplus) and mod.beta == 1 and mod.threshold == 20:
        return "softplus"
    return None


def conv_flops(B, Cin, H, W, Cout, kh, kw, stride, padding, dilation, draws, contractions=1):
    """(useful, im2col) FLOPs of a conv layer: useful counts only kernel taps that land inside the image."""
    sh, sw = ops._pair(stride)
    ph, pw = ops._pair(padding)
    dh, dw = ops._pair(dilation)
    ho = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    wo = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    vr = sum(1 for o in range(ho) for r in range(kh) if 0 <= o * sh - ph + r * dh < H)
    vq = sum(1 for o in range(wo) for q in range(kw) if 0 <= o * sw - pw + q * dw < W)
    base = 2.0 * contractions * draws * B * Cout * Cin
    return base * vr * vq, base * ho * wo * kh * kw


ChwnPartition = collections.namedtuple("ChwnPartition", "E B S n_draws call0 nblk x_div x_off ukw streams pad")


def chwn_partition(x_shape, draws, call0, bf16=False, units=None, groups=1, share=None, streams=1):
    """How one call of _mc_logits_chwn is cut up (no tensors, no device) -> ChwnPartition:
    E output slabs of B images each; S batch slices per draw; n_draws weight sets, the first under noise call `call0`; the input as
    nblk batch-innermost blocks; the first layer's slab e reads block (e + x_off) // x_div; ukw = the launches' work-unit arguments;
    streams (1 for every partition); pad = zero images that fill an odd batch up to a multiple of 4.
    units = (S, lo, hi): the work units lo..hi-1 of the draw-major (draw, batch slice) grid, u = draw * S + slice (call0 = the call
    index of draw 0).  groups = G > 1: x holds G batches back to back, slab g * draws + j = draw j of step g on batch g under call
    call0 + g * draws + j.  share = (D, off): `draws` consecutive slabs of the draw-major (step, draw) enumeration with D draws per
    step, the first being draw `off` of its step: slab e reads batch (e + off) // D of the ceil((draws + off) / D) batches in x."""
    E, B, G, ukw, pad = draws, x_shape[0], int(groups), {}, 0
    mult = 8 if bf16 else 4
    if B % 4 != 0 and not bf16 and G == 1 and share is None and (units is None or units[0] <= 1):
        # an odd batch stays on the batch-innermost kernels: zero images fill it up to the next multiple of 4 (every image is
        # its own GEMM column -- BBB weights are shared, LRT noise is keyed by the global image index -- so the real images'
        # results are those of an unpadded run), and their output rows (they come last, also behind a flatten that cuts images
        # into several rows) are dropped again.  One small copy instead of the ~2x slower reference-layout kernels.
        pad = -B % 4
        B += pad
    if G > 1:
        if units is not None and units[0] > 1:
            raise _lib.BBBHipError("several steps per launch and work units do not combine")
        if B % G or (B // G) % mult:
            raise _lib.BBBHipError("several steps per launch: every batch must hold a multiple of 4 (bf16: 8) images")
        B, E, streams = B // G, G * draws, 1
    x_div, x_off, nb = (draws if (G > 1 and draws > 1) else 1), 0, G
    if share is not None:
        if G > 1 or (units is not None and units[0] > 1):
            raise _lib.BBBHipError("a share of a group of steps combines with neither work units nor whole groups")
        D, off = int(share[0]), int(share[1])
        nb = -(-(draws + off) // D)
        if not 0 <= off < D or B % nb or (B // nb) % mult:
            raise _lib.BBBHipError("share of a group of steps: x must hold the batches it touches, multiples of 4 (bf16: 8) images")
        B = B // nb
        x_div, x_off = (D, off) if D > 1 else (1, 0)
        streams = 1
    if units is not None and units[0] > 1:
        S, lo, hi = units
        if B % S or (B // S) % mult:
            raise _lib.BBBHipError("work units: batch slices must hold a multiple of 4 (bf16: 8) images")
        E, B = hi - lo, B // S
        j_lo = lo // S
        n_draws = (hi - 1) // S - j_lo + 1                     # weight sets this rank needs
        call0 = call0 + j_lo
        ukw = dict(units=(S, lo % S), n_units=E)
        streams = 1
    else:
        S, n_draws = 1, E
    nblk = (S if S > 1 else nb) if (S > 1 or G > 1 or share is not None) else 1
    return ChwnPartition(E, B, S, n_draws, call0, nblk, x_div, x_off, ukw, streams, pad)


BAYES_FORMS = ("s2d_lrt", "s2d_bbb", "bf16_bbb", "c8x3_lrt", "c8x3_bbb", "fp32_bbb", "bf16_lrt", "fp32_lrt")


class ChwnStep:
    """One step of the walk: a launch (one of BAYES_FORMS, "pool", "avgpool", "to_c8s3"), a torch op ("relu", "softplus", "to_f32") or
    a view ("flatten").  i / mod: the module (a conversion: the module it prepares for, None at the end); act: the activation fused into
    the launch; pool: the MaxPool2d fused into it (True, or (k, s) where the launch takes any window) -- an "avgpool" step: its
    (kernel, stride, padding, count_include_pad), pool_desc.avgpool_of; logits: the launch writes the
    logits buffer; first: the first Bayesian layer (it reads the caller's input blocks); rows: a flatten that cuts every image
    into that many rows; in_layout / layout: how h enters / leaves (f32 | s3 | c8s3 | bf16 | bf16c8); in_shape / out_shape:
    (C, H, W, B); n_mods: modules consumed; a Bayesian layer's is_conv, geom = (stride, padding, dilation), ckk = (Cin, kh, kw) and
    tap_major (its bf16 weight rows, ops.bf16_tap_major)."""
    __slots__ = ("form", "i", "mod", "act", "pool", "out_f32", "logits", "out_c8", "out_s3", "shared_in", "first", "rows", "in_layout",
                 "layout", "in_shape", "out_shape", "n_mods", "is_conv", "geom", "ckk", "tap_major")

    def __init__(self, form, i, mod, in_layout, layout, in_shape, out_shape, n_mods, **kw):
        self.form, self.i, self.mod, self.in_layout, self.layout = form, i, mod, in_layout, layout
        self.in_shape, self.out_shape, self.n_mods = in_shape, out_shape, n_mods
        self.act = self.pool = None
        self.out_f32 = self.logits = self.out_c8 = self.out_s3 = self.shared_in = self.first = self.is_conv = self.tap_major = False
        self.geom = self.ckk = None
        self.rows = 1
        for k, v in kw.items():
            setattr(self, k, v)

    def __repr__(self):
        return "ChwnStep(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__ if k != "mod")


ChwnPlan = collections.namedtuple("ChwnPlan", "steps tm s2d_first lrt_mode bf16_lrt n_out")


def _is_conv(mod):
    return isinstance(mod, (_BBBConv, _LRTConv))


def _geom(mod):
    return (mod.stride, mod.padding, mod.dilation) if _is_conv(mod) else (1, 0, 1)


def _ckk(mod):
    return (mod.in_channels, *mod.kernel_size) if _is_conv(mod) else (mod.in_features, 1, 1)


def _chwn_modes(children, x_shape, draws, precision, cfg):
    """Which kernel family every Bayesian layer takes -> (layers on the MFMA-ready-operand kernel, the space-to-depth first layer or
    None, lrt_mode, split_mode).
    split-bf16 mode: layers with Cin % 16 == 0 (never the first one: its input is the caller's fp32 batch) run on the
    MFMA-ready-operand kernel (ops.conv2d_c8x3_forward) -- their input travels channel-interleaved and already split ("c8 S3"),
    their weights come tap-major from the parameter pass.  Which kernel a layer takes is a property of the LAYER (not of the
    launch size), so that a work unit, a share of a group of steps and the whole step are the same bits.
    LRT models (every Bayesian layer local-reparameterisation) the same way, on the kernel's LRT form: six-plane slabs (values +
    squares), W_mu / W_sigma^2 tap-major (rearranged once per launch: LRT weights do not depend on the draw)."""
    bayes = [m for m in children if isinstance(m, (_BBBLayer, _LRTLayer))]
    bbb = [l for l in bayes if isinstance(l, _BBBLayer)]
    lrt = [l for l in bayes if isinstance(l, _LRTLayer)]
    last = bayes[-1] if bayes else None
    tail_is_last = bool(children) and children[-1] is last
    split_any = (precision == "bf16x3" or cfg.gemm_mode == "bf16x3") and precision != "bf16" and tail_is_last
    split_mode = split_any and not lrt and bool(bbb)
    lrt_mode = split_any and bool(lrt) and not bbb and cfg.c8x3
    tm = set()
    if lrt_mode or (split_mode and cfg.c8x3):
        for l in bayes[1:]:
            cin, cout = (l.in_channels, l.out_channels) if _is_conv(l) else (l.in_features, l.out_features)
            if ops.c8x3_layer_ok(cin, cout, is_logits=(l is last)):
                tm.add(l)
    # a strided first layer on few channels (AlexNet conv1) joins the chain in space-to-depth form (ops.s2d_layer_ok): its block
    # image is cut from the caller's NCHW batch in c8 S3 directly, its dense weight draws are rearranged by one small launch
    s2d_first = None
    l0 = bayes[0] if (split_mode or lrt_mode) else None
    if l0 is not None and cfg.c8x3 and cfg.c8x3_s2d and children[0] is l0 and _is_conv(l0) and l0 not in tm and len(x_shape) == 4 \
            and l0 is not last:
        # (an LRT first layer whose input AND weights are the same for all E > 1 draws stays on the fp32 kernel: it runs its two
        # contractions ONCE and samples E times -- the block form would run them E times: 6.1 against 5.1 M samples/s at bs 512 x 10)
        # -- for EVERY partition of such a step (work units, shares of a group): which kernel a layer takes is a property of the step)
        lrt_shared_first = lrt_mode and int(draws) > 1
        if not lrt_shared_first and \
                ops.s2d_layer_ok(l0.in_channels, l0.out_channels, l0.kernel_size, l0.stride, l0.padding, l0.dilation, x_shape[2], x_shape[3]):
            s2d_first = l0
    return tm, s2d_first, lrt_mode, split_mode


class _NoPlan(Exception):
    """The batch-innermost walk does not apply to this model / shape: the plan is None and the caller falls back."""


class _Planner:
    """The state of the shape walk of _chwn_steps: the steps so far and how h looks behind them -- its layout tag, (C, H, W), B, its
    slabs (`lead`: the input blocks until the first Bayesian layer, then one per output slab) and the x_div of the partition (until
    the first Bayesian layer: its slab e reads block (e + x_off) // x_div)."""

    def __init__(self, children, x_shape, part, precision, cfg, draws, Es):
        self.children, self.Es, self.bf16, self.cfg = children, Es, precision == "bf16", cfg
        self.tm, self.s2d_first, self.lrt_mode, split_mode = _chwn_modes(children, x_shape, draws, precision, cfg)
        self.bayes = [i for i, m in enumerate(children) if isinstance(m, (_BBBLayer, _LRTLayer))]
        self.last_bayes = self.bayes[-1] if self.bayes else -1
        self.tail_is_last = self.last_bayes == len(children) - 1
        self.n_out = getattr(children[self.last_bayes], "out_features", None) if self.tail_is_last else None
        # split-bf16 mode, steps large enough that every conv launch takes that kernel: the activations between the layers travel in
        # the split format S3 (three bf16 planes holding the exact fp32 values; ops.conv2d_chwn_forward x_s3 / out_s3) -- each
        # element is cut into its pieces ONCE, by the launch that produces it, instead of by every workgroup that stages it
        self.s3_chain = split_mode and not self.tm and part.B % 8 == 0 and part.E * part.B >= cfg.s3_min_images
        self.bf16x3 = True if precision == "bf16x3" else None
        self.steps = []
        self.lay, self.chw, self.B = ("bf16" if self.bf16 else "f32"), tuple(x_shape[1:]), part.B
        self.lead, self.x_div = part.nblk, part.x_div

    def emit(self, form, i, mod, layout, out, n_mods, **kw):
        self.steps.append(ChwnStep(form, i, mod, self.lay, layout, self.chw + (self.B,), out, n_mods, **kw))
        self.lay, self.chw, self.B = layout, tuple(out[:3]), out[3]
        return n_mods

    def to_f32(self, i, mod):
        self.emit("to_f32", i, mod, "f32", self.chw + (self.B,), 0)

    def pool_behind(self, i, act):
        at = i + (2 if act is not None else 1)
        return at, (self.children[at] if at < len(self.children) and pool_desc.is_maxpool(self.children[at]) else None)

    def layer(self, i, mod, act):
        """A Bayesian layer with what its launch fuses -> modules consumed."""
        is_conv, geom, ckk = _is_conv(mod), _geom(mod), _ckk(mod)
        last, Es = i == self.last_bayes, self.Es
        cout = mod.out_channels if is_conv else mod.out_features
        kw = dict(act=act, first=i == self.bayes[0], logits=self.n_out is not None and last and not is_conv, is_conv=is_conv, geom=geom,
                  ckk=ckk, tap_major=self.bf16 and is_conv and ops.bf16_tap_major(tuple(mod.W_mu.shape)))
        if mod is self.s2d_first and i == 0:
            # the first layer in space-to-depth form: an m x m layer, stride 1, no padding, on the block image.  BBB: [activation
            # ->] MaxPool2d(2, 2) inside the launch (every window walks the same taps: the parallel-window form); LRT: values and
            # squares of the block image, no pooled form (the pool follows)
            g = ops.s2d_geometry(mod.in_channels, mod.kernel_size, mod.stride, mod.padding, mod.dilation, *self.chw[1:])
            _, pm = self.pool_behind(i, act)
            fuse = not self.lrt_mode and pm is not None and g[4] % 2 == 0 and g[5] % 2 == 0 and ops.is_pool_2x2(pm)
            return self.emit("s2d_lrt" if self.lrt_mode else "s2d_bbb", i, mod, "c8s3",
                             (cout, g[4] // (2 if fuse else 1), g[5] // (2 if fuse else 1), self.B), 1 + (act is not None) + fuse,
                             pool=fuse or None, **kw)
        use_c8 = mod in self.tm
        if self.lay == "c8s3" and not use_c8:
            self.to_f32(i, mod)
        C, H, W = self.chw
        if not is_conv and C * H * W != mod.in_features:
            raise _NoPlan                                        # a linear layer on something else than whole images
        if not is_conv:
            C, H, W = self.chw = (mod.in_features, 1, 1)
        if use_c8 and (self.lay not in ("f32", "c8s3") or (is_conv and C != mod.in_channels)):
            raise _NoPlan
        if use_c8 and self.lay != "c8s3":
            self.emit("to_c8s3", i, mod, "c8s3", (C, H, W, self.B), 0)
        ho, wo = out_map(H, W, ckk[1:], *geom)
        kw["out_f32"] = last if use_c8 else (last and self.tail_is_last and self.bf16)
        if isinstance(mod, _BBBLayer) and self.bf16:
            kw.update(self.bf16_bbb(i, mod, act, kw))
            form, out_lay = "bf16_bbb", ("bf16c8" if kw["out_c8"] else "f32" if kw["out_f32"] else "bf16")
            if kw["pool"]:
                ho, wo = pooled_map(ho, wo, kw["pool"])
        elif use_c8:
            form, out_lay = ("c8x3_lrt" if self.lrt_mode else "c8x3_bbb"), ("f32" if last else "c8s3")
        elif isinstance(mod, _BBBLayer):
            o_s3 = self.s3_chain and not last                    # intermediate layers hand their output on already split
            # [activation ->] MaxPool2d(2, 2) after a conv layer: one launch with it when the launch is large enough
            # (ops.pool_fusion_ok; same bits as the separate pooling launch).  (A chain over MFMA-ready operands: the layers
            # outside it -- the first one -- take the fp32 kernel, pooled form included)
            _, pm = self.pool_behind(i, act)
            fuse = (pm is not None and is_conv and self.lay != "s3" and not o_s3 and (self.bf16x3 is None or bool(self.tm)) and
                    ops.pool_fusion_ok((self.lead, C, H, W, self.B), (1, cout) + ckk, *geom, Es, pm, fp32_kernel=bool(self.tm)))
            kw.update(out_s3=o_s3, pool=fuse or None)
            form, out_lay = "fp32_bbb", ("s3" if o_s3 else "f32")
            if fuse:
                ho, wo = ho // 2, wo // 2
        elif self.bf16:
            # (shared_in: same input AND same weights for every draw -- the two contractions run once, moments only, and the E
            # draws differ only in the noise: bitwise the same result as E full launches.  h has ONE slab only in front of the
            # first layer of a step that is not partitioned)
            form, out_lay = "bf16_lrt", ("f32" if kw["out_f32"] else "bf16")
            kw["shared_in"] = self.lead == 1 and Es > 1 and not kw["out_f32"]
        else:
            # (... and on the fp32 kernel a share of a group of steps that lies inside ONE step -- one input slab, but x_div > 1 --
            # takes the full launch)
            form, out_lay = "fp32_lrt", "f32"
            kw["shared_in"] = self.lead == 1 and Es > 1 and self.x_div == 1
        return self.emit(form, i, mod, out_lay, (cout, ho, wo, self.B), 1 + (act is not None) + bool(kw.get("pool")), **kw)

    def bf16_bbb(self, i, mod, act, kw):
        """The bf16 BBB launch of layer i -> dict(pool = (k, s) | None, out_c8).
        [activation ->] MaxPool2d after a first layer with a short contraction: one launch (ops.bf16_pool_fusion_ok).  The pooled
        first layer writes its output channel-interleaved when the layer that reads it has the strip form over that layout
        (3Conv3FC conv1 + pool1 -> conv2; ops.bf16_c8_input_ok): same values, 8 channels of an image adjacent."""
        is_conv, geom, ckk, tapm, (C, H, W), B = kw["is_conv"], kw["geom"], kw["ckk"], kw["tap_major"], self.chw, self.B
        at, pm = self.pool_behind(i, act)
        x_shape = (self.lead, C // 8, H, W, B, 8) if self.lay == "bf16c8" else (self.lead, C, H, W, B)
        fuse = is_conv and ops.bf16_pool_fusion_ok(ckk, tapm, kw["out_f32"], pm, x_shape, geom, self.Es)
        pool_ks = (pm.kernel_size, pm.stride if pm.stride is not None else pm.kernel_size) if fuse else None
        out_c8 = False
        nb = self.children[at + 1] if (fuse and at + 1 < len(self.children)) else None
        if isinstance(nb, _BBBConv) and (mod.out_channels if is_conv else mod.out_features) % 8 == 0 and not kw["logits"]:
            hw = pooled_map(*out_map(H, W, ckk[1:], *geom), pool_ks)
            out_c8 = ops.bf16_c8_input_ok((nb.in_channels, *nb.kernel_size), (nb.stride, nb.padding, nb.dilation),
                                          ops.bf16_tap_major(tuple(nb.W_mu.shape)), at + 1 == self.last_bayes and self.tail_is_last,
                                          (hw[0], hw[1], B), self.Es)
        return dict(pool=pool_ks, out_c8=out_c8)

    def pool(self, i, mod):
        """A pooling module as a launch of its own -> a "pool" step (nn.MaxPool2d: the launch reads kernel and stride off the module)
        or an "avgpool" step (its `pool`: pool_desc.pool_of's spec, the wrappers' arguments), on the map pool_of states.  No plan
        where pool_of does not admit the module on this map.  A max pool runs in whatever layout it meets
        (ops.maxpool_chwn / _bf16 / _s3 / maxpool_c8s3).  An average pool (nn.AvgPool2d / nn.AdaptiveAvgPool2d; ops.avgpool_chwn, never
        fused into a conv launch) runs on fp32 planes: the split layouts are converted in front of it, as in front of a stand-alone
        activation.  bf16 storage, under LaunchConfig.bf16_avgpool: the same step on planar bf16 planes (ops.avgpool_chwn_bf16, the map
        asked of the 8-wide plan); no plan on bf16 storage without the switch, or in any layout but "bf16" (the planner chooses the
        channel-interleaved one only in front of a conv; the logits are fp32)."""
        C, H, W = self.chw
        spec = pool_desc.pool_of(mod, H, W)
        if spec is None:
            raise _NoPlan
        if spec.kind == "max":
            return self.emit("pool", i, mod, self.lay, (C, *spec.out, self.B), 1)
        if self.bf16 and not (self.cfg.bf16_avgpool and self.lay == "bf16"):
            raise _NoPlan
        if self.lay in ("s3", "c8s3"):
            self.to_f32(i, mod)
        try:
            ho, wo = pool_desc.pool_plan("avg", H, W, self.B if self.bf16 else 4, *spec, bf16=self.bf16)[:2]
        except _lib.BBBHipError:
            raise _NoPlan from None                              # (B % 8 != 0: bf16 storage does not take this batch at all)
        return self.emit("avgpool", i, mod, self.lay, (C, ho, wo, self.B), 1, pool=spec)

    def flatten(self, i, mod):
        F_, (C, H, W) = mod.num_features, self.chw
        if self.lay == "c8s3" and not (H * W == 1 and C == F_):  # ([E, 3, F / 8, 1, 1, B, 8] already is the flattened feature order)
            self.to_f32(i, mod)
        if self.lay == "s3" and C * H * W != F_:
            self.to_f32(i, mod)                                  # the flatten quirk below works on the fp32 tensor
        if self.lay == "bf16c8":
            raise _NoPlan
        chw, rows = C * H * W, 1
        if chw != F_:
            # the reference's view(-1, num_features) on a larger map (AlexNet on 224x224: [B,128,7,7] -> [B*49,128]) cuts each
            # image's NCHW memory into rows of num_features: continue batch-innermost with B' = B*chw/num_features "images"
            if chw % F_ != 0 or self.bf16 or (self.B * chw // F_) % 4 != 0:
                raise _NoPlan
            rows = chw // F_
        return self.emit("flatten", i, mod, self.lay, (F_, 1, 1, self.B * rows), 1, rows=rows)


def _chwn_steps(children, x_shape, part, precision, cfg, draws, n_slabs=None):
    """The walk as a list of ChwnStep, decided from shapes alone (integer arithmetic; the rules are the host-only helpers of
    bbb_hip.ops, asked under the LaunchConfig `cfg`) -> ChwnPlan, or None where the batch-innermost walk does not apply (a flatten
    whose rows do not divide an image, a linear layer on something else than whole images, ...: the caller falls back).
    n_slabs: the output slabs of the launches (default part.E; a stream of a split step runs fewer)."""
    try:
        with ops.use_config(cfg):                                # (the helpers read the current configuration)
            p = _Planner(children, x_shape, part, precision, cfg, draws, part.E if n_slabs is None else n_slabs)
            i = 0
            while i < len(children):
                mod = children[i]
                if isinstance(mod, (_BBBLayer, _LRTLayer)):
                    i += p.layer(i, mod, _act_name(children[i + 1]) if i + 1 < len(children) else None)
                    p.lead, p.x_div = p.Es, 1
                elif isinstance(mod, FlattenLayer):
                    i += p.flatten(i, mod)
                elif pool_desc.is_pool(mod):
                    i += p.pool(i, mod)
                else:
                    if p.lay in ("s3", "c8s3"):
                        p.to_f32(i, mod)
                    i += p.emit("relu" if isinstance(mod, nn.ReLU) else "softplus", i, mod, p.lay, p.chw + (p.B,), 1)
    except _NoPlan:
        return None
    if p.lay in ("s3", "c8s3"):
        p.to_f32(len(children), None)
    return ChwnPlan(p.steps, p.tm, p.s2d_first, p.lrt_mode, p.bf16 and any(isinstance(m, _LRTLayer) for m in children), p.n_out)


def _to_f32(h, layout):
    """h back in fp32 [E, C, H, W, B] from the split formats (the same values)."""
    return ops.s3_to_f32(h) if layout == "s3" else ops.c8s3_to_f32(h) if layout == "c8s3" else h


# ---- one launch function per form: (c = the call's context, st = the step, a = the layer's prologue) -> y.  Each runs in its own
# frame, so bench.py's LaunchRecorder can replay the closures after the walk has moved on
def _launch_s2d_lrt(c, st, a):
    mod, (wm_, wv_), x = st.mod, c.w_s2d, c.x
    m_ = int(round(wm_.shape[1] ** 0.5))
    zb = ops.s2d_zero_border(mod.in_channels, mod.kernel_size, mod.stride, mod.padding, x.shape[2], x.shape[3])
    kw = a.ukw2 if c.part.ukw else dict(a.ukw2, n_slabs=a.Es)
    return _run(c.timers, "lrt_gemm", a.fl, lambda: ops.lrt_conv2d_c8x3_forward(
        c.xs2d, wm_, wv_, mod.bias_mu if mod.use_bias else None, c.variances[mod][1], (m_, m_), c.seed, c.part.call0 + a.e0,
        mod._stream_base + 2, 1, 0, 1, act=st.act, b_offset=a.boff, zero_border=zb, **kw))


def _launch_s2d_bbb(c, st, a):
    mod, x = st.mod, c.x
    m_ = int(round(a.w.shape[2] ** 0.5))
    zb = ops.s2d_zero_border(mod.in_channels, mod.kernel_size, mod.stride, mod.padding, x.shape[2], x.shape[3])
    return _run(c.timers, "conv_gemm", a.fl, lambda: ops.conv2d_c8x3_forward(c.xs2d, a.w, a.b, (m_, m_), 1, 0, 1, act=st.act, pool=bool(st.pool),
                                                                            zero_border=zb, **a.ukw2))


def _launch_bf16_bbb(c, st, a):
    return _run(c.timers, "conv_gemm", a.fl, lambda: ops.conv2d_chwn_bf16_forward(
        a.h5, a.w, a.b, st.ckk, *st.geom, act=st.act, out_f32=st.out_f32, out=a.dst, tap_major=st.tap_major, pool=st.pool, out_c8=st.out_c8,
        **a.ukw2))


def _c8_kwargs(c, a, n_slabs):
    kw = {k: v for k, v in a.ukw2.items() if k != "x_per_slice"}
    if n_slabs and not c.part.ukw:
        kw["n_slabs"] = a.Es
    return kw


def _launch_c8x3_lrt(c, st, a):
    mod, (wm_, wv_), kw = st.mod, c.lrt_tm[st.mod], _c8_kwargs(c, a, True)
    ks = mod.kernel_size if st.is_conv else (1, 1)
    return _run(c.timers, "lrt_gemm", a.fl, lambda: ops.lrt_conv2d_c8x3_forward(
        a.h5, wm_, wv_, mod.bias_mu if mod.use_bias else None, c.variances[mod][1], ks, c.seed, c.part.call0 + a.e0, mod._stream_base + 2,
        *a.geom, act=st.act, out_f32=st.out_f32, out=a.dst, b_offset=a.boff, **kw))


def _launch_c8x3_bbb(c, st, a):
    ks, kw = (st.mod.kernel_size if st.is_conv else (1, 1)), _c8_kwargs(c, a, False)
    w = a.w.reshape(a.w.shape[0], a.w.shape[1], ks[0] * ks[1], -1)      # tap-major rows (a linear layer's rows as they are)
    return _run(c.timers, "conv_gemm", a.fl, lambda: ops.conv2d_c8x3_forward(a.h5, w, a.b, ks, *a.geom, act=st.act, out_f32=st.out_f32,
                                                                            out=a.dst, **kw))


def _launch_fp32_bbb(c, st, a):
    mod, w = st.mod, a.w
    if not st.is_conv:
        w = w.reshape(w.shape[0], mod.out_features, mod.in_features, 1, 1)
    bx3 = False if c.plan.tm else c.bf16x3
    return _run(c.timers, "conv_gemm", a.fl, lambda: ops.conv2d_chwn_forward(
        a.h5, w, a.b, *a.geom, act=st.act, out=a.dst, bf16x3=bx3, x_s3=st.in_layout == "s3", out_s3=st.out_s3, pool=bool(st.pool), **a.ukw2))


def _launch_bf16_lrt(c, st, a):
    """An LRT layer on bf16 storage (LaunchConfig.bf16_lrt): both contractions in one launch of the dual-accumulator bf16 GEMM,
    weights shared by every slab, the fp32 path's noise elements."""
    mod, (wm_b, wv_b), b_var, ckk, tapm = st.mod, c.lrt_b16[st.mod], c.variances[st.mod][1], st.ckk, st.tap_major
    args = (a.h5, wm_b, wv_b, mod.bias_mu if mod.use_bias else None, b_var, ckk, c.seed, c.part.call0 + a.e0, mod._stream_base + 2, *a.geom)
    if st.shared_in:
        _, am, av = _run(c.timers, "lrt_gemm", a.fl, lambda: ops.lrt_conv2d_chwn_bf16_forward(*args, sample=False, moments_only=True,
                                                                                             tap_major=tapm))
        return _run(c.timers, "lrt_sample", None, lambda: ops.lrt_sample_chwn_bf16(am, av, a.Es, c.seed, c.part.call0 + a.e0,
                                                                                  mod._stream_base + 2, act=st.act))
    return _run(c.timers, "lrt_gemm", a.fl, lambda: ops.lrt_conv2d_chwn_bf16_forward(
        *args, sample=True, act=st.act, out_f32=st.out_f32, out=a.dst, tap_major=tapm, n_slabs=a.Es, **a.ukw2)[0])


def _launch_fp32_lrt(c, st, a):
    mod, (w_var, b_var), w_mu = st.mod, c.variances[st.mod], st.mod.W_mu
    if not st.is_conv:
        shp = (mod.out_features, mod.in_features, 1, 1)
        w_mu, w_var = w_mu.reshape(shp), w_var.reshape(shp)
    args = (a.h5, w_mu, w_var, mod.bias_mu if mod.use_bias else None, b_var, c.seed, c.part.call0 + a.e0, mod._stream_base + 2, *a.geom)
    if st.shared_in:
        _, am, av = _run(c.timers, "lrt_gemm", a.fl, lambda: ops.lrt_conv2d_chwn_forward(*args, sample=False, want_moments=True, act=None))
        return _run(c.timers, "lrt_sample", None, lambda: ops.lrt_sample_chwn(am, av, a.Es, c.seed, c.part.call0 + a.e0, mod._stream_base + 2,
                                                                             act=st.act, b_offset=a.boff))
    return _run(c.timers, "lrt_gemm", a.fl, lambda: ops.lrt_conv2d_chwn_forward(
        *args, sample=True, act=st.act, b_offset=a.boff, **a.ukw2, **({"n_slabs": a.Es} if "x_div" in a.ukw2 else {}))[0])


_LAUNCH = {"s2d_lrt": _launch_s2d_lrt, "s2d_bbb": _launch_s2d_bbb, "bf16_bbb": _launch_bf16_bbb, "c8x3_lrt": _launch_c8x3_lrt,
           "c8x3_bbb": _launch_c8x3_bbb, "fp32_bbb": _launch_fp32_bbb, "bf16_lrt": _launch_bf16_lrt, "fp32_lrt": _launch_fp32_lrt}


def _layer_prologue(c, st, h, e0, e1, boff):
    """What every Bayesian layer's launch needs: the layer's view h5 of h (a linear layer reads 1 x 1 maps), the partition
    arguments of the launch (the caller's input blocks are read by the FIRST layer only), this run's slice of the weight draws,
    the destination where the layer writes the logits buffer, and the FLOP figure for the timers."""
    mod, part = st.mod, c.part
    a = types.SimpleNamespace(e0=e0, Es=e1 - e0, boff=boff, geom=st.geom, w=None, b=None)
    if st.is_conv:
        a.h5 = h
    elif st.in_layout == "c8s3":
        a.h5 = h.reshape(h.shape[0], h.shape[1], mod.in_features // 8, 1, 1, h.shape[5], 8)
    elif st.in_layout == "s3":
        a.h5 = h.reshape(h.shape[0], 3, mod.in_features, 1, 1, -1)
    else:
        a.h5 = h.reshape(h.shape[0], mod.in_features, 1, 1, -1)
    if part.ukw:
        a.ukw2 = dict(part.ukw, x_per_slice=st.first)             # work units: until the first layer, h is one block per batch slice
    else:                                                         # several steps per launch: its slab e reads batch (e + x_off) // x_div
        a.ukw2 = {"x_div": part.x_div, "x_off": part.x_off} if (st.first and part.x_div > 1) else {}
    if isinstance(mod, _BBBLayer):
        a.w, a.b = c.sampled[mod]
        if st.form == "s2d_bbb":
            a.w = c.w_s2d
        if not part.ukw:
            a.w = a.w[e0:e1]
            a.b = None if a.b is None else a.b[e0:e1]
    a.dst = c.logits_buf[e0:e1] if st.logits else None
    a.fl = None
    if c.timers is not None:
        ckk, (C, H, W, B) = st.ckk, st.in_shape
        a.fl = conv_flops(B, C, H, W, st.out_shape[0], ckk[1], ckk[2], *a.geom, 1 if st.shared_in else a.Es, 2 if isinstance(mod, _LRTLayer) else 1)
    return a


def _chwn_walk(c, steps, e0, e1):
    """The layers for slabs [e0, e1) on the current stream, one loop over the plan's steps -> logits [e1-e0, C, B]."""
    Es, timers = e1 - e0, c.timers
    h = c.xt
    B = c.part.B
    boff = int(c.b_offset)         # global index of the first local "image" (rows multiply at a flatten that cuts images up)
    for st in steps:
        form, mod = st.form, st.mod
        if form in _LAUNCH:
            h = _LAUNCH[form](c, st, _layer_prologue(c, st, h, e0, e1, boff))
        elif form == "to_f32":
            h = _to_f32(h, st.in_layout)
        elif form == "to_c8s3":
            hf = h if _is_conv(mod) else h.reshape(h.shape[0], mod.in_features, 1, 1, -1)
            h = _run(timers, "layout", None, lambda hf=hf: ops.c8s3_from_f32(hf, squares=c.plan.lrt_mode))
        elif form == "pool":
            pool = ops.maxpool_c8s3 if st.in_layout == "c8s3" else ops.maxpool_chwn_s3 if st.in_layout == "s3" else \
                (ops.maxpool_chwn_bf16 if c.bf16 else ops.maxpool_chwn)
            h = _run(timers, "maxpool", None, lambda h=h, mod=mod, pool=pool: pool(h, mod.kernel_size, mod.stride))
        elif form == "avgpool":
            avg = ops.avgpool_chwn_bf16 if st.in_layout == "bf16" else ops.avgpool_chwn
            h = _run(timers, "avgpool", None, lambda h=h, st=st, avg=avg: avg(h, *st.pool))
        elif form == "relu":
            h = torch.relu(h)
        elif form == "softplus":
            h = F.softplus(h)
        # ... a flatten:
        elif st.rows > 1:
            # the reference's view(-1, num_features) cuts each image's NCHW memory into rows of num_features: go through the NCHW
            # order once, on this small tensor, and continue batch-innermost with B' = B * rows "images"
            rows = h.permute(0, 4, 1, 2, 3).reshape(h.shape[0], -1, mod.num_features)     # [E|1, B', F]
            boff *= st.rows
            B = rows.shape[1]
            h = rows.permute(0, 2, 1).contiguous().reshape(h.shape[0], mod.num_features, 1, 1, B)
            if c.logits_buf is not None and c.logits_buf.shape[2] != B:
                c.logits_buf = torch.empty((c.part.E, c.plan.n_out, B), dtype=torch.float32, device=c.x.device)
        elif st.in_layout != "c8s3":                             # ([E, 3, F / 8, 1, 1, B, 8] already is the flattened feature order)
            h = h.reshape(h.shape[0], *((3,) if st.in_layout == "s3" else ()), mod.num_features, 1, 1, B)
    if h.shape[0] == 1 and Es > 1:
        h = h.expand(Es, *h.shape[1:])
    h = h.reshape(Es, -1, B)
    if c.logits_buf is not None and h.shape[1] == c.logits_buf.shape[1]:
        dst = c.logits_buf[e0:e1]
        if h.data_ptr() != dst.data_ptr():
            dst.copy_(h)
        return dst
    return h
