"""Autograd for the batch-innermost ensemble path (training extension).

`mc_logits_autograd(net, x, draws, seed, call0)` is the differentiable counterpart of ensemble._mc_logits_chwn for models made of
BBB (weight-space) layers: ONE autograd node for the whole batched forward.  Forward = the inference kernels (fused reparam+KL,
pixel-major GEMMs that skip padding taps with the activation in the epilogue, HIP pooling) recording each layer's input and
activated output; backward walks the layers in reverse with
  * `bbb_pool_act_bwd_chwn`            pooling + activation backward from the activated output alone,
  * `ops.conv2d_chwn_input_grad`       dgrad = the forward kernel on flipped, channel-transposed weights (a strided layer: the
                                       transposed form of that launch, csrc/pconv_dgrad.hip),
  * `ops.conv2d_chwn_weight_grad`      wgrad = the forward kernel with batch <-> channel roles swapped (padding taps skipped),
  * `ops.conv2d_chwn_weight_grad_shared_input`  the first layer (3-channel images): draws stacked into the GEMM rows over an
                                       im2col of the shared input, K split over the launch's draws,
  * `ops.reparam_kl_backward`          gradients of (mu, rho) from the gradients of the sampled weights + d loss / d KL (eps
                                       regenerated from the counter),
  * `ops.first_layer_input_grad`       d loss / d x when x requires a gradient (saliency maps, adversarial steps): the first
                                       layer's contraction over (draw, channel) on the forward kernel + the bbb_input_grad_col2im
                                       gather; with frozen parameters the weight side above is skipped altogether
                                       (the bf16 node, under LaunchConfig.bf16_input_grad: ops.first_layer_input_grad_bf16),
so no activation, pooling or convolution of the step runs through torch autograd.  What main_bayesian.py:43-58 does per batch:
E forwards, KL, log_softmax / logmeanexp, ELBO, backward -- on the training path the tail after the logits is HIP too
(ops.elbo_cb_autograd: bbb_elbo_cb_fwd / bbb_elbo_cb_bwd); the entry points that return log-probabilities keep it in torch.

Four nodes -- _MCForward (fp32), _MCForwardBF16 (bf16 storage), _MCForwardLRT (local reparameterisation), _MCForwardLRTBF16 (its
activation side in bf16 storage: input gradients with frozen parameters, no weight side) -- over one layer plan (train_plan: _parse
states the layer / activation / pool pairing, geometry and maps once per model and input shape; admission is that a plan exists), one
forward walk over it (_walk: the tape, every launch's map held against the plan), one backward walk down that tape (_walk_back: the
incoming gradient shaped to each record, the node's passes in their order, the first layer's dx, the join) and one backward schedule
(_Schedule: which stream a layer's weight side runs on, the early fork, the join); _carry / _run_backward take the launch
configuration and scratch scope to the backward.  A node keeps its arithmetic: how it runs a layer, its g_pre, its weight side, its
input gradient, its flips up front -- the backward walk gets them as callables and knows no node.
"""
import collections
import os

import torch

from . import _lib, ops, pool_desc
from .conv_desc import out_map as _out_map


def train_path_ok(net, x):
    """The fast autograd path covers: a 4-d CUDA fp32 batch with B % 4 == 0; a flat model (ensemble.flat_children) of Bayesian
    conv / linear layers of ONE kind (all BBB or all BBB_LRT) sharing one prior, each optionally followed by ReLU /
    Softplus(1, 20) and then a pool pool_desc.pool_of admits (MaxPool2d without padding in floor mode, nn.AvgPool2d, a dividing
    nn.AdaptiveAvgPool2d), and a FlattenLayer that keeps one row per image; convolutions of any
    positive stride in any layer (a strided layer behind the first takes its input gradient on the transposed launch,
    ops.conv2d_chwn_input_grad(stride=)), padding within the kernel reach (p <= d (k - 1)) and channel counts that are multiples
    of 4 everywhere except the first layer; the model ends in a Bayesian linear layer; no eps replay.  Returns "bbb", "lrt" or
    None."""
    from . import ensemble
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 4 or x.dtype != torch.float32 or x.shape[0] % 4 != 0:
        return None
    # what never changes for a given model and input shape is analysed once (train_plan); what can change between calls (eps
    # replay switched on, a layer moved off the device) is re-checked every time
    plan = train_plan(net, x.shape)
    if plan is None or any(m.eps_source is not None or not m.W_mu.is_cuda for m in ensemble.bayesian_layers(net)):
        return None
    return plan.kind


def _train_path_static(net, x):
    return getattr(train_plan(net, x.shape), "kind", None)


# One Bayesian layer with what follows it.  wshape: (Cout, Cin, kh, kw), a linear layer's (out, in, 1, 1); geom: (stride, padding,
# dilation), a linear layer's (1, 0, 1); act: "relu" | "softplus" | None, fused into the layer's launch; pool: the PoolSpec of the
# pool behind that, or None; in_chw: what the layer reads (a linear layer: (in_features, 1, 1) -- a flatten in front of a layer is
# this reshape); conv_chw: what its launch writes; out_chw: behind the pool, what the next block meets.
TrainBlock = collections.namedtuple("TrainBlock", "layer li is_conv wshape geom act pool in_chw conv_chw out_chw first last")
TrainPlan = collections.namedtuple("TrainPlan", "kind blocks")              # kind: "bbb" | "lrt"; blocks: TrainBlocks, forward order


def _parse(mods, x_shape):
    """THE grammar of a model on the training path (train_path_ok states it in words): a flat module list (ensemble.flat_children)
    and an input shape -> (TrainPlan, None), or (None, why it is not on the path).  No tensors, no device; the map is followed with
    conv_desc.out_map and pool_desc.pool_of alone."""
    from . import ensemble
    from layers.bbb import _BBBLayer, BBBConv2d, BBBLinear
    from layers.lrt import _LRTLayer, BBBConv2d as LRTConv2d, BBBLinear as LRTLinear
    from layers.misc import FlattenLayer
    if not mods or not isinstance(mods[-1], (BBBLinear, LRTLinear)):
        return None, "the model must be flat (ensemble.flat_children) and end in a Bayesian linear layer"
    blocks, pri, kinds = [], set(), set()
    chw = tuple(int(v) for v in x_shape[1:])                             # what the next module meets
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, (_BBBLayer, _LRTLayer)):
            kinds.add("lrt" if isinstance(m, _LRTLayer) else "bbb")
            if not m.use_bias:
                return None, "every Bayesian layer needs a bias"
            pri.add((m.prior_mu, m.prior_sigma))
            is_conv = isinstance(m, (BBBConv2d, LRTConv2d))
            if is_conv:
                if min(ops._pair(m.stride)) < 1:
                    return None, "a convolution's stride must be at least 1"
                (ph, pw), (dh, dw) = ops._pair(m.padding), ops._pair(m.dilation)
                if dh * (m.kernel_size[0] - 1) < ph or dw * (m.kernel_size[1] - 1) < pw:
                    return None, "a convolution's padding must stay within the kernel reach (p <= d (k - 1))"
                wshape, geom, in_chw = tuple(m.W_mu.shape), (m.stride, m.padding, m.dilation), chw
                chw = (m.out_channels, *_out_map(chw[1], chw[2], m.kernel_size, *geom))
            elif m.in_features % 4 != 0:         # (a first linear layer too: its weight gradient takes the 4-aligned channel path)
                return None, "a linear layer's in_features must be a multiple of 4"
            else:
                wshape, geom, in_chw = (m.out_features, m.in_features, 1, 1), (1, 0, 1), (m.in_features, 1, 1)
                chw = (m.out_features, 1, 1)
            pool, conv_chw, last = None, chw, i == len(mods) - 1
            act = ensemble._act_name(mods[i + 1]) if not last else None
            i += act is not None
            if i + 1 < len(mods) and pool_desc.is_pool(mods[i + 1]):
                i += 1
                pool = pool_desc.pool_of(mods[i], chw[1], chw[2])
                if pool is None:
                    return None, "a pool this path does not take on the map it meets (pool_desc.pool_of)"
                chw = (chw[0], *pool.out)
            blocks.append(TrainBlock(m, len(blocks), is_conv, wshape, geom, act, pool, in_chw, conv_chw, chw, not blocks, last))
        elif pool_desc.is_pool(m):
            # a leading pool, or a pool after a pool / flatten: the node's backward pairs pools with layers
            return None, "pooling must follow a Bayesian layer (and its activation) directly"
        elif isinstance(m, FlattenLayer):
            chw = (m.num_features, 1, 1)
        else:
            return None, "a stand-alone activation or a module this path does not know: " + type(m).__name__
        i += 1
    if len(pri) != 1 or len(kinds) != 1 or len(blocks) * 2 > _lib.MAX_SEGMENTS:
        return None, f"at most {_lib.MAX_SEGMENTS // 2} Bayesian layers, of one kind (all BBB or all LRT) and sharing one prior"
    return TrainPlan(next(iter(kinds)), tuple(blocks)), None


def _analysis(net, x_shape):
    """(plan, why) of _parse for (net, x_shape), cached on the module with the rest of its analysis (ensemble._structure: dropped by
    the registration hooks and ensemble.invalidate).  One rule is asked of ensemble, which owns it, not of the module list: the
    model yields one output row per image (ensemble.output_rows)."""
    from . import ensemble
    cache = ensemble._structure(net)["train"]
    if x_shape not in cache:
        plan, why = _parse(ensemble.flat_children(net), x_shape)
        if plan is not None and ensemble.output_rows(net, x_shape) != x_shape[0]:
            plan, why = None, "a FlattenLayer that keeps one row per image"
        cache[x_shape] = (plan, why)
    return cache[x_shape]


def train_plan(net, x_shape):
    """The TrainPlan of `net` on an input of shape x_shape (what the nodes' forward walks), or None where the model is not on the
    training path.  The plan is cached: after changing a layer's or a pool's geometry in place, call ensemble.invalidate(net)."""
    return _analysis(net, tuple(x_shape))[0]


def ws_shape(rec):
    """[E, *the layer's W_mu.shape]: the record's wshape, a linear layer's without its two unit taps."""
    return (rec["w"].shape[0],) + rec["wshape"][:rec["layer"].W_mu.dim()]


fold_lrt_combine = [True]       # an LRT layer's g1 + 2 x g2 is formed inside the pooling / activation backward of the layer below
flips_up_front = [True]         # every layer's flipped input-gradient weights in one launch at the start of the backward
pair_lrt_backward = [True]      # an LRT layer's (mean, variance) gradient pairs as the two draws of one launch (see _MCForwardLRT._backward)
overlap_wgrad = [True]
_side_streams = {}


n_side_streams = [int(os.environ.get("BBB_TRAIN_SIDE_STREAMS", "2"))]      # (measured 1 / 2 / 3: 2.895 / 2.75 / 2.78 ms per bs 512 x 10 step)


class _Sides:
    """The side streams of a device, handed out round robin (layer by layer); waits / joins address all of them."""

    def __init__(self, device, n):
        self.streams = [torch.cuda.Stream(device=device) for _ in range(n)]
        self.i = 0

    def wait_stream(self, main):
        self.i = (self.i + 1) % len(self.streams)
        self.streams[self.i].wait_stream(main)

    @property
    def current(self):
        return self.streams[self.i]


def _side_stream(device):
    key = (torch.device(device).index, n_side_streams[0])
    if key not in _side_streams:
        _side_streams[key] = _Sides(device, n_side_streams[0])
    return _side_streams[key]


def _check_versions(versions):
    """What autograd's saved-tensor check would raise: a parameter (or sigma^2 operand) changed in place between the forward
    that recorded this node and its backward, which re-reads the live storage."""
    for p, v in versions:
        if p._version != v:
            raise RuntimeError("one of the variables needed for gradient computation has been modified by an inplace operation: "
                               "a Bayesian layer's parameter changed between the forward and this backward (optimizer.step() "
                               "before a delayed backward?)")


# ---------------------------------------------------------------------------------------------------------------------------
# what the four nodes share: the parameter lists, the forward walk, the context they carry to the backward, the backward schedule,
# the backward walk, how the outputs are packed
# ---------------------------------------------------------------------------------------------------------------------------
def _prior_lists(layers):
    """The tensor priors of the nodes' one parameter pass (ensemble._prior_lists: None when no layer has any)."""
    from . import ensemble
    return ensemble._prior_lists(layers)


def _prior_kw(tp):
    from . import ensemble
    return ensemble._prior_kw(tp)


def _param_lists(layers, leaf):
    """(mus, rhos, stream ids) of the layers in forward order -- per layer (W, bias) -- each parameter passed through `leaf`
    (a node's forward: detach; mc_logits_autograd: the alias that roots the graph)."""
    mus, rhos, ids = [], [], []
    for l in layers:
        m, r, i = l._param_lists()
        mus += [leaf(t) for t in m]
        rhos += [leaf(t) for t in r]
        ids += i
    return mus, rhos, ids


def _node_plan(cfg, x):
    """A node's forward: the plan it walks; a model that is not on the path raises with the parser's reason."""
    plan, why = _analysis(cfg["net"], tuple(x.shape))
    if plan is None:
        raise _lib.BBBHipError("fast_train: " + why)
    return plan


def _held(h, li, chw):                                                     # the walk's check of what a launch returned against the plan
    if tuple(h.shape[1:4]) != chw:
        raise _lib.BBBHipError(f"fast_train: layer {li} left a {tuple(h.shape[1:4])} map where the analysed model has {chw}: the "
                               "model's geometry changed since it was analysed -- call ensemble.invalidate(net) after changing a "
                               "stride, a padding or a pool in place")


def _walk(plan, h, run_layer, pool, avgpool=None):
    """The forward walk over a TrainPlan (train_plan), one copy for the four nodes: -> (tape, final h).
    h: the batch-innermost input [1, C, H, W, B].  run_layer(blk, x_in) -> a record holding at least `y`, the activated output
    [E', *blk.conv_chw, B], of the block's layer on x_in = h as [*, *blk.in_chw, B], with blk.geom and blk.act (fused).
    pool(y, kernel, stride): the node's max pooling; avgpool(y, kernel, stride, padding, count_include_pad): its average pooling --
    each called with blk.pool, the spec of the pool behind the layer, unpacked.
    The walk completes the record from the block -- layer, x, act, geom, wshape, pool (that spec: its kind, and as a tuple the
    arguments above; None without a pool), first, out_shape (of what the next layer reads) -- and appends it to the tape.  The plan is
    an analysis cached on the model: what a launch returns is held against it, so a geometry changed in place since then raises
    instead of running unadmitted."""
    tape = []                                                              # per Bayesian layer, in forward order
    for blk in plan.blocks:
        x_in = h.reshape(h.shape[0], *blk.in_chw, h.shape[-1])
        rec = run_layer(blk, x_in)
        rec.update(layer=blk.layer, x=x_in, act=blk.act, geom=blk.geom, wshape=blk.wshape, pool=blk.pool, first=blk.first)
        h = rec["y"]
        _held(h, blk.li, blk.conv_chw)
        if blk.pool is not None:
            h = (pool if blk.pool.kind == "max" else avgpool)(h, *blk.pool)
            _held(h, blk.li, blk.out_chw)
        rec["out_shape"] = tuple(h.shape)
        tape.append(rec)
    return tape, h


def _pool_pass(rec, max_pass, avg_pass, *tensors, **kw):
    """The pooling / activation backward of a record, one place for the four nodes: the node's wrapper of the record's pool on
    `tensors` -- max_pass(*tensors, k, s, act, **kw) behind a max pool or, as k = 0, behind the activation alone;
    avg_pass(*tensors, kernel, stride, padding, count_include_pad, act, **kw) behind an average pool."""
    spec = rec["pool"]
    if spec is None:
        return max_pass(*tensors, 0, 1, rec["act"], **kw)
    return (max_pass if spec.kind == "max" else avg_pass)(*tensors, *spec, rec["act"], **kw)


def _carry(ctx, cfg, params):
    """forward: what every node's backward needs beside its tape."""
    ctx.cfg = cfg
    ctx.launch_config = ops.current_config()              # backward runs on autograd's device thread: carry the modes along
    ctx.scratch_token = ops.current_scratch_token()
    ctx.versions = [(p, p._version) for p in params]      # backward re-reads the live (mu, rho): they must not have moved


def _run_backward(ctx, node_backward, *grads):
    """backward: the node's _backward under the forward's launch configuration and scratch scope."""
    with ops.use_config(ctx.launch_config), ops.scratch_scope(token=ctx.scratch_token):
        _check_versions(ctx.versions)
        ctx.cfg["spent"] = True                            # layers/_fused.py: no further draws are served from this graph
        return node_backward(ctx, *grads)


class _Schedule:
    """Where the launches of one backward go.  A layer's weight / bias gradients and its input gradient are independent: the former
    run on a side stream beside the latter (both are launches that leave the chip partly idle on their own), the streams taken
    round robin, last layer first; the first layer's weight side runs on the main stream (nothing is left to run beside it); all
    are joined before the parameter pass's backward.  Eager launches only: inside a captured step the forks cost more than the
    overlap gains -- 4.8 against 3.05 ms per step.  A side-stream count below 1 (n_side_streams, BBB_TRAIN_SIDE_STREAMS) means no side
    streams: the schedule of overlap_wgrad off.
    The invariant the code rests on, and why no tensor needs a record_stream (which would change what the allocator does):
      * every launch on a side stream is preceded by that stream's wait_stream(main), so it sees what main has written;
      * every tensor a side stream reads is referenced in `keep` until join() (the allocator, which knows main as their stream, must
        not hand them out again while a side stream still reads them);
      * every tensor a side stream allocates is consumed on main only after main has waited for that stream -- the weight gradients
        gws after join(), the early im2col xk_first after the first layer's wait on fork_early's stream, and held in `keep` until
        join() -- and a side stream that is handed the block again waits for main (the first point) before it writes there.
    g: the incoming gradient (None: nothing to schedule); weight_side: the node runs weight sides at all."""

    def __init__(self, g, weight_side):
        self.run_weights = weight_side
        forks = (g is not None and weight_side and overlap_wgrad[0] and n_side_streams[0] >= 1
                 and not torch.cuda.is_current_stream_capturing())
        self.side = _side_stream(g.device) if forks else None
        self.main = torch.cuda.current_stream(g.device) if forks else None
        self.keep = []
        self.early = None                                  # the stream of fork_early's launch

    def fork_early(self, launch):
        """launch() on a side stream NOW (one turn of the round robin) -> its result, kept until the join; the first layer's
        weight side waits for it."""
        self.side.wait_stream(self.main)
        self.early = self.side.current
        with torch.cuda.stream(self.early):
            out = launch()
        self.keep.append(out)
        return out

    def weight_side(self, first, launch, reads):
        """A layer's weight side: on the next side stream (which keeps `reads` alive) unless it is the first layer's or there are
        no side streams; then on the main stream; not at all when the node runs no weight sides."""
        if self.side is not None and not first:
            self.keep += reads
            self.side.wait_stream(self.main)
            with torch.cuda.stream(self.side.current):
                launch()
        elif self.run_weights:
            if first and self.early is not None:
                self.main.wait_stream(self.early)
            launch()

    def join(self):
        if self.side is not None:
            for st_ in self.side.streams:
                self.main.wait_stream(st_)
        self.keep = []


def _walk_back(tape, g, sched, g_pre_of, weight_side, input_grad, first_dx):
    """The backward walk down a tape (_walk's), one copy for the four nodes, mirror of _walk: -> dx, or None.
    g: the gradient of the last record's output (None: nothing to walk); sched: the node's _Schedule.  What passes from layer to layer
    is a tuple of tensors, each of which the walk shapes to the record's out_shape: one tensor, or what an LRT layer hands down
    (_lrt_incoming).  The node's arithmetic, per record from the last one:
      g_pre_of(rec, *gs) -> (g_pre, reads)    its pooling / activation pass: g_pre in whatever form the other three take it, and the
                                              tensors of it the weight side reads (a side stream keeps them alive);
      weight_side(li, rec, g_pre)             the layer's parameter gradients, run where and if the schedule says (a node that
                                              runs none: its _Schedule has weight_side False, and this is None);
      input_grad(li, rec, g_pre) -> gs        below the first layer: what the layer underneath receives;
      first_dx(rec, g_pre) -> dx              the first layer, when x takes a gradient (None when it does not).
    The streams are joined at the end."""
    dx = None
    gs = () if g is None else (g,)
    for li in range(len(tape) - 1, -1, -1):
        if not gs:
            break
        rec = tape[li]
        g_pre, reads = g_pre_of(rec, *(t.reshape(rec["out_shape"]) for t in gs))
        sched.weight_side(rec["first"], lambda: weight_side(li, rec, g_pre), reads=reads)
        if not rec["first"]:
            gs = input_grad(li, rec, g_pre)
        else:
            if first_dx is not None:
                dx = first_dx(rec, g_pre)
            gs = ()
    sched.join()
    return dx


def _pack(dx, grads):
    """What a node's backward returns: a gradient per forward argument -- cfg (none), x, the parameters."""
    return (None, dx, *grads)


def _pack_bbb(ctx, dx, gws, g_kl):
    """_pack for the two BBB nodes: the gradients of the sampled weights gws (per layer W, bias) + d loss / d KL through the parameter
    pass's backward -> per layer W_mu, W_rho, bias_mu, bias_rho; frozen parameters: no pass, no gradients."""
    mus, rhos, ids, pm, ps, _, tp = ctx.meta
    if not any(ctx.needs_input_grad[2:]):
        return _pack(dx, [None] * (2 * len(mus)))
    gmu, grho = ops.reparam_kl_backward(mus, rhos, gws, g_kl, pm, ps, ids, ctx.cfg["seed"], ctx.cfg["call0"], ctx.cfg["draws"],
                                        **_prior_kw(tp))
    grads = []
    for a, b in zip(gmu, grho):
        grads += [a, b]
    return _pack(dx, grads)


def _lrt_incoming(g, x_out=None, g2=None):
    """What an LRT layer receives from _walk_back -> (g, combine=) of its pooling / activation pass: the logits' gradient alone, or
    the triple (g1, x_out, g2) the layer above hands down under fold_lrt_combine -- its two input gradients and its input, this
    layer's output -- which that pass combines (g1 + 2 x_out g2) instead of a launch of its own.  (All three arrive shaped to this
    record's out_shape: x_out is the output behind the pool as the layer above read it, draws included -- only a first layer's input
    has a single draw, and a first layer hands nothing down.)"""
    return g, (None if g2 is None else (x_out, g2))


class _MCForward(torch.autograd.Function):
    """(x, W_mu0, W_rho0, b_mu0, b_rho0, W_mu1, ...) -> (logits [E, C, B] batch-innermost, kl of one forward)."""

    @staticmethod
    def forward(ctx, cfg, x, *params):
        plan = _node_plan(cfg, x)
        E, seed, call0 = cfg["draws"], cfg["seed"], cfg["call0"]
        layers = [b.layer for b in plan.blocks]
        mus, rhos, ids = _param_lists(layers, torch.Tensor.detach)
        pm, ps = layers[0].prior_mu, layers[0].prior_sigma         # (the scalar fallbacks agree: _parse) + per-weight tensor priors
        tp = _prior_lists(layers)
        ws, _, kl = ops.reparam_kl_forward(mus, rhos, pm, ps, ids, seed, call0, draws=E, **_prior_kw(tp))

        def run_layer(blk, x_in):
            w, b = ws[2 * blk.li], ws[2 * blk.li + 1]
            w5 = w if blk.is_conv else w.reshape(E, *blk.wshape)
            return dict(w=w5, y=ops.conv2d_chwn_forward(x_in, w5, b, *blk.geom, act=blk.act))

        h = ops.to_batch_innermost(x.detach()).unsqueeze(0)               # [1, C, H, W, B]
        tape, h = _walk(plan, h, run_layer, ops.maxpool_chwn, ops.avgpool_chwn)
        _carry(ctx, cfg, params)
        ctx.tape, ctx.meta = tape, (mus, rhos, ids, pm, ps, tuple(x.shape), tp)
        ctx.x_nchw = x.detach()
        return h.reshape(E, -1, x.shape[0]), kl

    @staticmethod
    def backward(ctx, g_logits, g_kl):
        return _run_backward(ctx, _MCForward._backward, g_logits, g_kl)

    @staticmethod
    def _backward(ctx, g_logits, g_kl):
        tape, x_shape = ctx.tape, ctx.meta[5]
        # need_w False (frozen parameters: saliency maps, adversarial steps): no weight side at all -- no bias sums, weight gradients,
        # im2col, parameter pass or side-stream forks; need_x: the first layer's input gradient (first_layer_input_grad) at the end
        need_x, need_w = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
        gws = [None] * (2 * len(tape))
        g = g_logits.contiguous() if g_logits is not None else None
        sched = _Schedule(g, weight_side=need_w)
        # the first layer's im2col depends on the batch alone: on a side stream NOW, beside the small last layers' launches, instead of
        # in the tail of the chain where nothing else is left to run beside it (without side streams
        # conv2d_chwn_weight_grad_shared_input builds it itself: xk None)
        r0 = tape[0]
        xk_first = None
        if sched.side is not None and r0["x"].shape[1] % 4 != 0:
            xk_first = sched.fork_early(lambda: ops.im2col_pbj(ctx.x_nchw, tuple(r0["w"].shape), *r0["geom"]))
        # every layer's input-gradient weights (flipped, channel-transposed: they depend on the sampled weights alone) in ONE launch up
        # front instead of one launch per layer on the chain -- for launch-bound steps (no side streams: captured, small).  A
        # many-draw step keeps them on the chain: up front, even on the side stream, they cost it 40 us (2.45 -> 2.49 ms at 512 x 10,
        # profiles/experiments/ab_flips_up_front.py)
        w_flipped = {}
        if flips_up_front[0] and sched.side is None and g is not None and len(tape) > 1:
            outs = ops.flip_transpose_w_multi([tape[li]["w"] for li in range(1, len(tape))])
            w_flipped = {li: o for li, o in zip(range(1, len(tape)), outs)}

        def g_pre_of(rec, g):
            pad = rec["first"] and rec["x"].shape[1] % 4 != 0            # feeds conv2d_chwn_weight_grad_shared_input
            if rec["pool"] is None and rec["act"] is None:
                g_pre = g
            else:
                g_pre = _pool_pass(rec, ops.pool_act_backward_chwn, ops.avgpool_act_backward_chwn, g, rec["y"], pad_planes=pad)
            return g_pre, [g_pre]

        def weight_side(li, rec, g_pre):
            x_in, wsh = rec["x"], tuple(rec["w"].shape)
            gws[2 * li + 1] = ops.plane_sums(g_pre)                       # bias gradient [E, Cout]
            if x_in.shape[1] % 4 == 0 or not rec["first"]:               # (6-channel inputs etc.: padded to 8 inside)
                gw = ops.conv2d_chwn_weight_grad(g_pre, x_in, wsh, *rec["geom"])
            else:
                # 3-channel first layer: its input is shared by all draws, so the draws stack into the GEMM's row dimension
                gw = ops.conv2d_chwn_weight_grad_shared_input(g_pre, ctx.x_nchw, wsh, *rec["geom"], xk=xk_first)
            gws[2 * li] = gw.reshape(ws_shape(rec))

        def input_grad(li, rec, g_pre):
            stride, padding, dilation = rec["geom"]
            return (ops.conv2d_chwn_input_grad(g_pre, rec["w"], tuple(rec["x"].shape[2:4]), padding, dilation, w_flipped=w_flipped.get(li),
                                               stride=stride),)

        def first_dx(rec, g_pre):
            return ops.first_layer_input_grad(g_pre, rec["w"], tuple(rec["x"].shape[2:4]), *rec["geom"]).view(x_shape)

        dx = _walk_back(tape, g, sched, g_pre_of, weight_side, input_grad, first_dx if need_x else None)
        return _pack_bbb(ctx, dx, gws, g_kl)


class _MCForwardBF16(torch.autograd.Function):
    """_MCForward in the bf16 storage mode (train.train_step(precision="bf16"); the arithmetic contract is DESIGN.md section 4.5):
    (x, W_mu0, W_rho0, b_mu0, b_rho0, W_mu1, ...) -> (fp32 logits [E, C, B] batch-innermost, fp32 kl of one forward).
    Forward = the bf16 inference kernels with the pooling left unfused (the tape keeps every layer's pre-pool output): sampled
    weights, the input and every hidden activated / pooled output stored as bf16, fp32 accumulation, fp32 logits and KL.  Tape:
    each layer's bf16 input, bf16 activated output and bf16 weight rows.  Backward: _walk_back on a _Schedule as _MCForward's, with
      * ops.pool_act_backward_chwn_bf16   g_pre = act'(y) * route(g) in fp32, rounded once to bf16 (the logits' fp32 gradient too),
      * ops.avgpool_act_backward_chwn_bf16   the same behind an average pool (LaunchConfig.bf16_avgpool): every window's gradient over
        its divisor to each of its taps,
      * ops.plane_sums_bf16               bias gradients, the fp32 sum of that bf16 g_pre,
      * ops.conv2d_chwn_input_grad_bf16   dgrad on the bf16 GEMM over the flipped bf16 weight rows -> bf16 (a strided layer, admitted
        under LaunchConfig.bf16_strided_train: the transposed launch on the same rows),
      * ops.conv2d_chwn_weight_grad_bf16  wgrad on the bf16 GEMM with the roles swapped -> fp32,
      * the first layer (3-channel input shared by every draw): ops.conv2d_chwn_weight_grad_shared_input on the fp32 kernel over
        the fp32 values of the bf16 operands (a bf16 x bf16 product is exact in fp32: the same contraction),
      * ops.reparam_kl_backward           unchanged (fp32),
      * ops.first_layer_input_grad_bf16   d loss / d x when x requires a gradient (LaunchConfig.bf16_input_grad): the first layer's
        contraction over (draw, channel) on the bf16 MFMA from the sampled rows and g_pre where they are -> fp32, never rounded, + the
        bbb_input_grad_col2im gather; with frozen parameters the weight side above is skipped altogether and the first layer's g_pre
        stays bf16."""

    @staticmethod
    def forward(ctx, cfg, x, *params):
        plan = _node_plan(cfg, x)
        E, seed, call0 = cfg["draws"], cfg["seed"], cfg["call0"]
        layers = [b.layer for b in plan.blocks]
        mus, rhos, ids = _param_lists(layers, torch.Tensor.detach)
        pm, ps = layers[0].prior_mu, layers[0].prior_sigma
        tp = _prior_lists(layers)
        kl, ws = ops.sample_weights_bf16(mus, rhos, pm, ps, ids, seed, call0, E, **_prior_kw(tp))

        def run_layer(blk, x_in):                          # (the logits layer, fp32 output: the plan ends in it, bare)
            w, b = ws[2 * blk.li], ws[2 * blk.li + 1]
            y = ops.conv2d_chwn_bf16_forward(x_in, w, b, blk.wshape[1:], *blk.geom, act=blk.act, out_f32=blk.last,
                                             tap_major=blk.is_conv and ops.bf16_tap_major(blk.wshape))
            return dict(w=w, y=y)

        h = ops.to_batch_innermost_bf16(x.detach()).unsqueeze(0)          # [1, C, H, W, B] bf16
        tape, h = _walk(plan, h, run_layer, ops.maxpool_chwn_bf16, ops.avgpool_chwn_bf16)
        _carry(ctx, cfg, params)
        ctx.tape, ctx.meta = tape, (mus, rhos, ids, pm, ps, tuple(x.shape), tp)
        # the first layer's fp32 weight gradient reads the input's bf16 values (what the forward contracted); frozen parameters
        # (a backward to x alone, LaunchConfig.bf16_input_grad): there is none
        ctx.x_nchw = (x.detach().to(torch.bfloat16).to(torch.float32)
                      if tape[0]["x"].shape[1] % 4 != 0 and any(ctx.needs_input_grad[2:]) else None)
        return h.reshape(E, -1, x.shape[0]), kl

    @staticmethod
    def backward(ctx, g_logits, g_kl):
        return _run_backward(ctx, _MCForwardBF16._backward, g_logits, g_kl)

    @staticmethod
    def _backward(ctx, g_logits, g_kl):
        tape, E, x_shape = ctx.tape, ctx.cfg["draws"], ctx.meta[5]
        # need_w False -- frozen parameters, reached under LaunchConfig.bf16_input_grad alone: no weight side at all; need_x: the first
        # layer's input gradient (first_layer_input_grad_bf16) at the end.  Without the switch this mode refuses x.requires_grad
        # (bf16_train_refusal): every backward is then one for the parameters alone, enqueued as it always was
        need_x, need_w = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
        gws = [None] * (2 * len(tape))
        g = g_logits.contiguous() if g_logits is not None else None
        sched = _Schedule(g, weight_side=need_w)
        r0 = tape[0]
        shared0 = need_w and r0["x"].shape[1] % 4 != 0                    # (no weight side: the first layer's g_pre stays bf16)
        xk_first = None                                                   # the first layer's im2col, forked up front beside the last layers
        if sched.side is not None and shared0:
            xk_first = sched.fork_early(lambda: ops.im2col_pbj(ctx.x_nchw, (E,) + r0["wshape"], *r0["geom"]))
        # every layer's flipped input-gradient weight rows up front, for captured / launch-bound steps (no side streams); one launch
        # per layer: the rows have no multi-layer form
        w_flipped = {}
        if flips_up_front[0] and sched.side is None and g is not None:
            w_flipped = {li: ops.flip_transpose_w_bf16(tape[li]["w"], tape[li]["wshape"]) for li in range(1, len(tape))}

        def g_pre_of(rec, g):
            y = rec["y"]
            shared = rec["first"] and shared0                             # feeds conv2d_chwn_weight_grad_shared_input (fp32)
            if rec["pool"] is None and rec["act"] is None and g.dtype == torch.bfloat16 and not shared:
                g_pre = g                                                 # already the bf16 output gradient
            else:                                                         # (the logits layer's fp32 y: no pool, no activation -- a rounding)
                g_pre = _pool_pass(rec, ops.pool_act_backward_chwn_bf16, ops.avgpool_act_backward_chwn_bf16,
                                   g, y if y.dtype == torch.bfloat16 else None, out_f32=shared, pad_planes=shared)
            return g_pre, [g_pre]

        def weight_side(li, rec, g_pre):
            wsh = (E,) + rec["wshape"]
            if rec["first"] and shared0:
                gws[2 * li + 1] = ops.plane_sums(g_pre)
                gw = ops.conv2d_chwn_weight_grad_shared_input(g_pre, ctx.x_nchw, wsh, *rec["geom"], xk=xk_first)
            else:
                gws[2 * li + 1] = ops.plane_sums_bf16(g_pre)
                gw = ops.conv2d_chwn_weight_grad_bf16(g_pre, rec["x"], wsh, *rec["geom"])
            gws[2 * li] = gw.reshape(ws_shape(rec))

        def input_grad(li, rec, g_pre):
            stride, padding, dilation = rec["geom"]
            return (ops.conv2d_chwn_input_grad_bf16(g_pre, rec["w"], rec["wshape"], tuple(rec["x"].shape[2:4]), padding, dilation,
                                                    w_flipped=w_flipped.get(li), stride=stride),)

        def first_dx(rec, g_pre):                          # on the sampled rows and g_pre where they are: bf16, or the fp32 form the weight side reads
            return ops.first_layer_input_grad_bf16(g_pre, rec["w"], rec["wshape"], tuple(rec["x"].shape[2:4]), *rec["geom"]).view(x_shape)

        dx = _walk_back(tape, g, sched, g_pre_of, weight_side, input_grad, first_dx if need_x else None)
        return _pack_bbb(ctx, dx, gws, g_kl)


def _inverse_act(y, act):
    """Pre-activation from the activated output (what the LRT backward needs to recover sqrt(act_var) * eps = v - act_mu)."""
    if act == "softplus":
        return torch.where(y > 20.0, y, y + torch.log(-torch.expm1(-y)))
    return y                                  # ReLU: exact where y > 0; elsewhere the incoming gradient is zero anyway


class _MCForwardLRT(torch.autograd.Function):
    """Local-reparameterisation layers (layers/BBB_LRT/BBBConv.py:62-81): (x, W_mu0, W_var0, b_mu0, b_var0, ...) -> logits
    [E, C, B] batch-innermost.  Forward = the dual-accumulator LRT GEMM (act_mu, act_var, sample + activation in the epilogue);
    for the first layer, whose input and weights are the same for every draw, the two contractions run once and
    bbb_lrt_sample_chwn draws the E outputs.  Backward: out = act_mu + sqrt(act_var) * eps gives d/d act_mu = g and
    d/d act_var = g * (v - act_mu) / (2 act_var) with v recovered from the stored activated output; then two weight gradients
    (g_mu with x, g_var with x^2) and, below the first layer, g_x = dgrad(g_mu, W_mu) + 2 x * dgrad(g_var, W_var), all on the
    forward GEMM kernel (fast_train module docstring)."""

    @staticmethod
    def forward(ctx, cfg, x, *params):
        plan = _node_plan(cfg, x)
        E, seed, call0 = cfg["draws"], cfg["seed"], cfg["call0"]

        def run_layer(blk, x_in):
            geom, act = blk.geom, blk.act
            w_mu, w_var, b_mu, b_var = (t.detach() for t in params[4 * blk.li:4 * blk.li + 4])
            if not blk.is_conv:
                w_mu, w_var = w_mu.reshape(blk.wshape), w_var.reshape(blk.wshape)
            sid = blk.layer._stream_base + 2
            if x_in.shape[0] == 1 and E > 1:              # the shared first layer: one pair of moments, E samples of it
                _, am, av = ops.lrt_conv2d_chwn_forward(x_in, w_mu, w_var, b_mu, b_var, seed, call0, sid, *geom, sample=False,
                                                        want_moments=True, act=None)
                y = ops.lrt_sample_chwn(am, av, E, seed, call0, sid, act=act)
            else:
                y, am, av = ops.lrt_conv2d_chwn_forward(x_in, w_mu, w_var, b_mu, b_var, seed, call0, sid, *geom, sample=True,
                                                        want_moments=True, act=act)
            return dict(w_mu=w_mu, w_var=w_var, y=y, am=am, av=av)

        h = ops.to_batch_innermost(x.detach()).unsqueeze(0)
        tape, h = _walk(plan, h, run_layer, ops.maxpool_chwn, ops.avgpool_chwn)
        _carry(ctx, cfg, params)
        ctx.tape = tape
        ctx.x_nchw = x.detach()
        return h.reshape(h.shape[0], -1, x.shape[0])

    @staticmethod
    def backward(ctx, g_logits):
        return _run_backward(ctx, _MCForwardLRT._backward, g_logits)

    @staticmethod
    def _backward(ctx, g_logits):
        tape = ctx.tape
        need_x, need_w = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])         # (frozen parameters: no weight side at all)
        grads = [None] * (4 * len(tape))
        g = g_logits.contiguous()
        sched = _Schedule(g, weight_side=need_w)
        # the flipped input-gradient weights of every layer -- mean and variance sets -- in one launch up front, whether or not there are
        # side streams (the BBB nodes: without them only)
        w_flipped = {}
        if flips_up_front[0] and len(tape) > 1:
            pairs = [(tape[li]["w_mu"].unsqueeze(0), tape[li]["w_var"].unsqueeze(0)) for li in range(1, len(tape))]
            outs = ops.flip_transpose_w_multi(pairs)                     # [2, Cin, Cout, kh, kw] each: the mean set, then the variance set
            w_flipped = {li: o for li, o in zip(range(1, len(tape)), outs)}

        def g_pre_of(rec, *incoming):                      # -> ((g_mu, g_var, g_pair | None), what the weight side reads)
            g, comb = _lrt_incoming(*incoming)
            am = rec["am"]
            # one pass: pooling / activation backward AND the split into d/d act_mu, d/d act_var (was ~10 ATen kernels per layer)
            pad = rec["first"] and rec["x"].shape[1] % 4 != 0            # feeds conv2d_chwn_weight_grad_shared_input
            # below the first layer the pair (d/d act_mu, d/d act_var) stays ONE buffer: its two weight gradients (with x, x^2) and,
            # for a single draw, its two input gradients (with W_mu, W_var) run as the draws of one launch each
            g_pair = None
            def pool_pass(**kw):
                return _pool_pass(rec, ops.lrt_pool_act_backward_chwn, ops.lrt_avgpool_act_backward_chwn, g, rec["y"], am, rec["av"], **kw)
            if pair_lrt_backward[0] and not rec["first"]:
                g_pair = pool_pass(stacked=True, combine=comb)                                 # [2, E, Cout, Ho, Wo, B]
                g_mu, g_var = g_pair[0], g_pair[1]
            else:
                g_mu, g_var = pool_pass(pad_planes=pad, combine=comb)
            if am.shape[0] == 1 and g_mu.shape[0] > 1:      # first layer: one pair of moments feeds every draw
                # (the two sums one set apart in one buffer: the input gradient reads them as the two draws of one launch)
                both = torch.empty((2, 1) + tuple(g_mu.shape[1:]), dtype=torch.float32, device=g_mu.device)
                g_mu, g_var = ops.sum_over_draws(g_mu, keepdim=True, out=both[0]), ops.sum_over_draws(g_var, keepdim=True, out=both[1])
            return (g_mu, g_var, g_pair), [g_mu, g_var]

        def weight_side(li, rec, g_pre):
            g_mu, g_var, g_pair = g_pre
            x_in, w_mu = rec["x"], rec["w_mu"]
            stride, padding, dilation = rec["geom"]
            wshape = (1,) + tuple(w_mu.shape)
            Ed = g_mu.shape[0]
            if g_pair is not None and Ed == 1:
                gb = ops.plane_sums(g_pair.reshape((2,) + tuple(g_mu.shape[1:])))               # [2, Cout]
                grads[4 * li + 2], grads[4 * li + 3] = gb[0], gb[1]
            else:
                grads[4 * li + 2] = ops.plane_sums(g_mu, over_draws=True)
                grads[4 * li + 3] = ops.plane_sums(g_var, over_draws=True)
            if g_pair is not None and x_in.shape[0] == Ed:
                gw = ops.conv2d_chwn_weight_grad(g_pair.reshape((2 * Ed,) + tuple(g_mu.shape[1:])), x_in,
                                                 (2 * Ed,) + tuple(w_mu.shape), stride, padding, dilation, x_squares=True)
                gw_mu, gw_var = ops.sum_over_draws(gw[:Ed]), ops.sum_over_draws(gw[Ed:])
            elif x_in.shape[1] % 4 == 0 or not rec["first"]:
                gw_mu = ops.conv2d_chwn_weight_grad(g_mu, x_in, wshape, stride, padding, dilation)
                gw_var = ops.conv2d_chwn_weight_grad(g_var, ops.square(x_in), wshape, stride, padding, dilation)
                gw_mu, gw_var = ops.sum_over_draws(gw_mu), ops.sum_over_draws(gw_var)
            else:
                # (built inside the weight side, on the main stream: this node forks no early im2col, _MCForward does)
                xk = ops.im2col_pbj(ctx.x_nchw, wshape, stride, padding, dilation)      # (its square = the im2col of x^2)
                gw_mu = ops.conv2d_chwn_weight_grad_shared_input(g_mu, None, wshape, stride, padding, dilation, xk=xk)[0]
                gw_var = ops.conv2d_chwn_weight_grad_shared_input(g_var, None, wshape, stride, padding, dilation, xk=ops.square(xk))[0]
            m = rec["layer"]
            grads[4 * li] = gw_mu.reshape(m.W_mu.shape)
            grads[4 * li + 1] = gw_var.reshape(m.W_mu.shape)

        def input_grad(li, rec, g_pre):
            g_mu, g_var, g_pair = g_pre
            x_in, w_mu, w_var = rec["x"], rec["w_mu"], rec["w_var"]
            stride, padding, dilation = rec["geom"]
            hw = (x_in.shape[2], x_in.shape[3])
            w_t = w_flipped.get(li)
            if g_pair is not None and g_mu.shape[0] == 1:
                if w_t is None:
                    w_t = ops.flip_transpose_w_pair(w_mu.unsqueeze(0), w_var.unsqueeze(0))
                gx = ops.conv2d_chwn_input_grad(g_pair.reshape((2,) + tuple(g_mu.shape[1:])), w_mu.unsqueeze(0), hw, padding, dilation,
                                                w_flipped=w_t, stride=stride)
                g1, g2 = gx[0:1], gx[1:2]
            else:
                t_mu, t_var = (w_t[0:1], w_t[1:2]) if w_t is not None else (None, None)
                g1 = ops.conv2d_chwn_input_grad(g_mu, w_mu.unsqueeze(0), hw, padding, dilation, w_flipped=t_mu, stride=stride)
                g2 = ops.conv2d_chwn_input_grad(g_var, w_var.unsqueeze(0), hw, padding, dilation, w_flipped=t_var, stride=stride)
            # (g1 + 2 x g2 is formed by the layer below's pooling / activation pass: _lrt_incoming)
            return (g1, x_in, g2) if fold_lrt_combine[0] else (ops.lrt_input_grad_combine(g1, x_in, g2),)

        def first_dx(rec, g_pre):
            x_in = rec["x"]
            return ops.first_layer_input_grad(g_pre[:2], (rec["w_mu"], rec["w_var"]), (x_in.shape[2], x_in.shape[3]), *rec["geom"],
                                              x_lrt=ctx.x_nchw).view(ctx.x_nchw.shape)

        dx = _walk_back(tape, g, sched, g_pre_of, weight_side, input_grad, first_dx if need_x else None)
        return _pack(dx, grads)


def _lrt_bf16_forward(cfg, x, params):
    """The forward of _MCForwardLRTBF16 -> (tape, fp32 logits [E, C, B] batch-innermost): the launches of the bf16 LRT inference path
    (ensemble._mc_logits_chwn under LaunchConfig.bf16_lrt: ops.lrt_weights_bf16 once for every layer; per layer
    ops.lrt_conv2d_chwn_bf16_forward -- the shared first layer of a many-draw step as moments only + ops.lrt_sample_chwn_bf16 --;
    ops.maxpool_chwn_bf16 unfused), so the logits are that path's bit for bit, with the fp32 act_var of every layer kept beside them.
    params: per layer W_mu, sigma_W^2, bias_mu, sigma_b^2 (fp32).  A record of the tape: x (the bf16 input), y (the stored bf16
    activated output before the pool; the logits layer's is fp32), av (act_var: y's shape, or one draw's worth for the shared first
    layer), w_mu / w_var (the bf16 rows), sid (the noise stream), and what _walk adds (geom, act, wshape, pool, first, out_shape)."""
    plan = _node_plan(cfg, x)
    E, seed, call0 = cfg["draws"], cfg["seed"], cfg["call0"]
    params = [t.detach() for t in params]
    rows = ops.lrt_weights_bf16([params[4 * li + j] for li in range(len(plan.blocks)) for j in (0, 1)])

    def run_layer(blk, x_in):                              # (the logits layer, fp32 output: the plan ends in it, bare)
        li, act, last = blk.li, blk.act, blk.last
        w_mu, w_var, b_mu, b_var = rows[2 * li], rows[2 * li + 1], params[4 * li + 2], params[4 * li + 3]
        sid = blk.layer._stream_base + 2
        tapm = blk.is_conv and ops.bf16_tap_major(blk.wshape)
        args = (x_in, w_mu, w_var, b_mu, b_var, blk.wshape[1:], seed, call0, sid, *blk.geom)
        if x_in.shape[0] == 1 and E > 1 and not last:        # the shared first layer: one pair of moments, E samples of it
            _, am, av = ops.lrt_conv2d_chwn_bf16_forward(*args, sample=False, moments_only=True, tap_major=tapm)
            y = ops.lrt_sample_chwn_bf16(am, av, E, seed, call0, sid, act=act)
        else:
            y, _, av = ops.lrt_conv2d_chwn_bf16_forward(*args, sample=True, want_moments=True, act=act, out_f32=last, tap_major=tapm,
                                                        n_slabs=E)
        return dict(w_mu=w_mu, w_var=w_var, y=y, av=av, sid=sid)

    def no_avgpool(*a):
        raise _lib.BBBHipError("bf16 LRT input gradients: no average pools (bf16_train_refusal refuses them)")

    h = ops.to_batch_innermost_bf16(x.detach()).unsqueeze(0)              # [1, C, H, W, B] bf16
    tape, h = _walk(plan, h, run_layer, ops.maxpool_chwn_bf16, no_avgpool)
    return tape, h.reshape(E, -1, x.shape[0])


class _MCForwardLRTBF16(torch.autograd.Function):
    """Input gradients of all-LRT models in bf16 storage, frozen parameters (LaunchConfig.bf16_lrt + bf16_lrt_input_grad; the arithmetic
    contract is DESIGN.md section 4.5b): (x, W_mu0, sigma_W0^2, b_mu0, sigma_b0^2, ...) -> fp32 logits [E, C, B] batch-innermost.
    Forward = _lrt_bf16_forward.  Backward = _walk_back as _MCForwardLRT runs it, without a weight side -- a _Schedule that forks
    nothing and waits on nothing, no parameter gradient -- on bf16 storage, per layer from the top:
      * ops.lrt_pool_act_backward_chwn_bf16   pooling / activation backward and the split into (g_mu, g_var) in one pass, eps
        regenerated from the counter (the stored y is rounded: the fp32 kernel's y - act_mu would cancel rounded values), the layer
        above's g1 + 2 x g2 combined on the fly; each of the pair rounded once to bf16,
      * ops.conv2d_chwn_input_grad_bf16       below the first layer d1 = dgrad(g_mu, W_mu), d2 = dgrad(g_var, sigma^2) on the bf16 GEMM
        over the flipped rows (a strided layer, under LaunchConfig.bf16_strided_train: the transposed launch), each rounded once,
      * ops.first_layer_input_grad_bf16_lrt   the first layer: dx = T(g_mu, W_mu) + 2 x_b * T(g_var, sigma^2), the sum over draws part
        of the fp32 accumulation, x_b the bf16-rounded input; fp32, never rounded."""

    @staticmethod
    def forward(ctx, cfg, x, *params):
        tape, logits = _lrt_bf16_forward(cfg, x, params)
        _carry(ctx, cfg, params)
        ctx.tape = tape
        ctx.x_b = x.detach().to(torch.bfloat16).to(torch.float32)         # what the forward multiplied, widened
        return logits

    @staticmethod
    def backward(ctx, g_logits):
        return _run_backward(ctx, _MCForwardLRTBF16._backward, g_logits)

    @staticmethod
    def _backward(ctx, g_logits):
        cfg, tape = ctx.cfg, ctx.tape
        if any(ctx.needs_input_grad[2:]):
            raise _lib.BBBHipError("bf16 LRT has input gradients only: no parameter gradient (bf16_train_refusal refuses trainable parameters)")
        seed, call0 = cfg["seed"], cfg["call0"]
        g = g_logits.contiguous()
        sched = _Schedule(g, weight_side=False)            # no weight side: nothing forks, nothing waits

        def g_pre_of(rec, *incoming):                      # the logits' fp32 gradient, or the layer above's bf16 (d1, x_out, d2)
            g, comb = _lrt_incoming(*incoming)
            y = rec["y"]
            g_pair = _pool_pass(rec, ops.lrt_pool_act_backward_chwn_bf16, None, g, y if y.dtype == torch.bfloat16 else None, rec["av"],
                                noise=(seed, call0, rec["sid"]), combine=comb)            # [2, E, Cout, Ho, Wo, B] bf16
            return g_pair, []

        def input_grad(li, rec, g_pair):
            x_in, wshape = rec["x"], rec["wshape"]
            stride, padding, dilation = rec["geom"]
            hw = (x_in.shape[2], x_in.shape[3])
            d1 = ops.conv2d_chwn_input_grad_bf16(g_pair[0], rec["w_mu"].unsqueeze(0), wshape, hw, padding, dilation, stride=stride)
            d2 = ops.conv2d_chwn_input_grad_bf16(g_pair[1], rec["w_var"].unsqueeze(0), wshape, hw, padding, dilation, stride=stride)
            return (d1, x_in, d2)                          # (d1 + 2 x d2 is formed by the layer below's pass)

        def first_dx(rec, g_pair):
            x_in = rec["x"]
            return ops.first_layer_input_grad_bf16_lrt(g_pair, rec["w_mu"], rec["w_var"], rec["wshape"], (x_in.shape[2], x_in.shape[3]),
                                                       *rec["geom"], ctx.x_b).view(ctx.x_b.shape)

        dx = _walk_back(tape, g, sched, g_pre_of, None, input_grad, first_dx if ctx.needs_input_grad[1] else None)
        return _pack(dx, [None] * (4 * len(tape)))


def _strided_later_conv(net):
    """A convolution behind the first Bayesian layer has a stride other than 1."""
    from . import ensemble
    return any(hasattr(m, "stride") and ops._pair(m.stride) != (1, 1) for m in ensemble.bayesian_layers(net)[1:])


_BF16_STRIDED_REFUSAL = ("stride-1 convolutions after the first layer (the strided input gradient has an fp32 kernel only; "
                         "precision='fp32' trains such a model) unless LaunchConfig.bf16_strided_train is set "
                         "(ops.use_config(bf16_strided_train=True) or launch_config= on GraphedTrainStep: the transposed bf16 launch, opt-in)")


def _bf16_lrt_input_grad_refusal(net, x):
    """bf16_train_refusal for a model with LRT layers under LaunchConfig.bf16_lrt_input_grad: why the bf16 LRT input-gradient node
    (_MCForwardLRTBF16) does not cover (net, x), or None when it does -- an all-LRT model on the training path (train_path_ok "lrt") with
    EVERY parameter frozen, an input that requires a gradient, B % 8 == 0, no eps replay, max pools only, stride-1 convolutions behind
    the first layer (any stride under LaunchConfig.bf16_strided_train), under LaunchConfig.bf16_lrt."""
    from . import ensemble
    cfg = ops.current_config()
    if not cfg.bf16_lrt:
        return ("BBB (weight-space) layers; LaunchConfig.bf16_lrt_input_grad takes effect only together with LaunchConfig.bf16_lrt: "
                + ensemble._BF16_LRT_HINT)
    if any(m.eps_source is not None for m in ensemble.bayesian_layers(net)):
        return "no eps replay"
    if ensemble.any_requires_grad(net):
        return ("frozen parameters on LRT models: bf16 LRT has input gradients only (LaunchConfig.bf16_lrt_input_grad; there is no bf16 "
                "LRT training) -- freeze them with net.requires_grad_(False), or use precision='fp32', which trains LRT models")
    if not (x.requires_grad and torch.is_grad_enabled()):
        return ("an input that requires a gradient: bf16 LRT has input gradients only (LaunchConfig.bf16_lrt_input_grad); without one, "
                "ensemble.mc_logits / mc_forward under torch.no_grad() run the bf16 LRT inference path")
    kind = train_path_ok(net, x)
    if kind != "lrt":
        return ("a model whose Bayesian layers are ALL local-reparameterisation layers, and an input, on the batch-innermost training "
                "path (fast_train.train_path_ok): no mixed BBB / LRT models")
    if ensemble._has_avgpool(net):
        return ("LRT models without average pooling: the LRT pooling / activation backward has no average-pool form on bf16 planes "
                "(lrt_pool_act_backward_chwn_bf16 routes max pools only), with or without LaunchConfig.bf16_avgpool; precision='fp32' "
                "has it")
    if _strided_later_conv(net) and not cfg.bf16_strided_train:
        return _BF16_STRIDED_REFUSAL
    if x.shape[0] % 8 != 0:
        return "a batch size that is a multiple of 8"
    return None


def bf16_train_refusal(net, x):
    """Why the bf16 training mode does not cover (net, x), or None when it does: what train_path_ok calls "bbb" with B % 8 == 0 --
    with stride-1 convolutions behind the first layer, or any stride there under LaunchConfig.bf16_strided_train, and without average
    pools, or with them under LaunchConfig.bf16_avgpool, and with an input that does not require a gradient, or one that does under
    LaunchConfig.bf16_input_grad (all read from the configuration that is current: the caller's use_config, or what GraphedTrainStep
    snapshotted).  Under LaunchConfig.bf16_lrt_input_grad a model with LRT layers is asked of _bf16_lrt_input_grad_refusal instead: input
    gradients of all-LRT models with frozen parameters."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32):
        return "a 4-d fp32 CUDA batch"
    from . import ensemble
    if ensemble._bf16_lrt_input_grad_asked(net):             # (evaluated under that switch alone: off, nothing below moves)
        return _bf16_lrt_input_grad_refusal(net, x)
    if x.requires_grad and torch.is_grad_enabled() and not ops.current_config().bf16_input_grad:
        return ("inputs that do not require a gradient (precision='fp32' has input gradients) unless LaunchConfig.bf16_input_grad is "
                "set (ops.use_config(bf16_input_grad=True): the first layer's input gradient on the bf16 operands, opt-in)")
    if any(m.eps_source is not None for m in ensemble.bayesian_layers(net)):
        return "no eps replay"
    kind = train_path_ok(net, x)
    if kind is not None and ensemble._has_avgpool(net) and not ops.current_config().bf16_avgpool:
        return ("models without average pooling (precision='fp32' trains such a model) unless LaunchConfig.bf16_avgpool is set "
                "(ops.use_config(bf16_avgpool=True) or launch_config= on GraphedTrainStep: the average pool on bf16 planes, opt-in)")
    if kind == "lrt":
        return "BBB (weight-space) layers; local-reparameterisation layers have no bf16 mode"
    if kind is None:
        return "a model and input on the batch-innermost training path (fast_train.train_path_ok)"
    if _strided_later_conv(net) and not ops.current_config().bf16_strided_train:
        return _BF16_STRIDED_REFUSAL
    if x.shape[0] % 8 != 0:
        return "a batch size that is a multiple of 8"
    return None


def mc_logits_autograd(net, x, draws, seed, call0, alias=None, precision="fp32"):
    """Differentiable batched forward: -> (logits [E, C, B] batch-innermost, kl of one forward), gradients flow to every
    layer's W_mu, W_rho, bias_mu, bias_rho.  Call only when train_path_ok(net, x).
    alias: {id(parameter): leaf tensor sharing its storage} -- the autograd graph is then rooted at those leaves instead of the
    parameters (train.GraphedTrainStep: fresh leaves have no gradient accumulator bound to another stream).
    precision="bf16": the bf16 storage mode (_MCForwardBF16); what it does not cover raises BBBHipError (bf16_train_refusal)."""
    def A(t):
        return t if alias is None else alias.get(id(t), t)

    from . import ensemble
    _lib.require_device(x)
    if precision not in ("fp32", "bf16"):
        raise _lib.BBBHipError(f"training precision must be 'fp32' or 'bf16', got {precision!r}")
    if precision == "bf16":
        why = bf16_train_refusal(net, x)
        if why is not None:
            raise _lib.BBBHipError("bf16 training covers " + why)
        node = _MCForwardLRTBF16 if train_path_ok(net, x) == "lrt" else _MCForwardBF16       # (an LRT model passes the refusal under
    else:                                                                                     #  LaunchConfig.bf16_lrt_input_grad alone)
        node = _MCForwardLRT if train_path_ok(net, x) == "lrt" else _MCForward
    layers = ensemble.bayesian_layers(net)
    mus, rhos, _ = _param_lists(layers, A)
    if node is _MCForwardLRT:                # its leaves are (mu, sigma^2) from the KL pass, which carries the gradients to (mu, rho)
        kl, rhos, mus = ops.kl_only(mus, rhos, layers[0].prior_mu, layers[0].prior_sigma, want_sigma=True, sigma_squared=True,
                                    mu_through=True, **_prior_kw(ensemble._prior_lists(layers)))
    elif node is _MCForwardLRTBF16:          # frozen parameters: the inference path's KL pass (fp32), sigma^2 beside it
        kl, rhos = ops.kl_only(mus, rhos, layers[0].prior_mu, layers[0].prior_sigma, want_sigma=True, sigma_squared=True,
                               **_prior_kw(ensemble._prior_lists(layers)))
    params = []
    for li in range(len(layers)):            # per layer: W_mu, W_rho (LRT: W_var), bias_mu, bias_rho (LRT: bias_var)
        params += [mus[2 * li], rhos[2 * li], mus[2 * li + 1], rhos[2 * li + 1]]
    cfg = dict(net=net, draws=int(draws), seed=seed, call0=call0)
    out = node.apply(cfg, x, *params)
    logits, kl = (out, kl) if node in (_MCForwardLRT, _MCForwardLRTBF16) else out
    logits.bbb_cfg = cfg
    return logits, kl
