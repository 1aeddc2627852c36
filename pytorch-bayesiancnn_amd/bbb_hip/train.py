"""Training extension: the inner loop of the reference's train_model
(main_bayesian.py:36-62) on the MI355X path -- Monte-Carlo forward with autograd through the HIP kernels
(bbb_hip.ops), the ELBO of metrics.py:12-24, one multi-tensor Adam launch, and, for data-parallel jobs (one process
per GPU, each with its own shard of the batch), ONE all-reduce of the flattened gradients per step.

Not part of the forward metric; forward-only inference is `bbb_hip.ensemble`.
"""
import weakref

import torch
import torch.nn.functional as F

from . import _lib, ensemble, ops, rng
from ._lib import AdamSegment, check, cur_stream
from .likelihood import GaussianLikelihood, gaussian_elbo  # noqa: F401  (train.GaussianLikelihood, train.gaussian_elbo)


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay, decoupled_weight_decay) semantics (amsgrad off) with the update of up
    to 16 parameter tensors per HIP launch (`bbb_adam_step`; `bbb_adam_step_ex` as soon as an option below is in use).  State layout
    matches torch's ('step', 'exp_avg', 'exp_avg_sq') and param_groups hold torch.optim.Adam's keys only, so state_dicts are
    interchangeable with torch.optim.Adam / AdamW.
    capturable=True keeps 'step' on the device (torch's capturable convention) and lets the kernel derive the bias
    corrections from it, so the step can be part of a captured hipGraph (GraphedTrainStep).  The learning rate of a
    capturable group also lives on the device (a private per-group scalar, kept OUT of param_groups so that state_dict() holds
    exactly what torch.optim.Adam's does): `sync_lr()` copies group['lr'] there, which is how a scheduler's change reaches a
    step that was captured earlier.
    weight_decay / decoupled_weight_decay (per group): Adam's L2 form g + wd p, or AdamW's p (1 - lr wd) before the update.
    max_grad_norm (an attribute of the optimizer, global over ALL groups, not part of state_dict()): clip by the global L2 norm as
    torch.nn.utils.clip_grad_norm_(all parameters, max_grad_norm) would before the step -- coef = min(1, max / (norm + 1e-6)) -- with
    ONE deliberate difference: `p.grad` is never written.  The coefficient scales the gradient on its way into the update, inside the
    Adam launch; the tensors in .grad stay as backward left them.  The norm is accumulated in float64 (`bbb_grad_sumsq`, then
    `bbb_grad_norm_finish`), so it does not overflow or vanish where torch's fp32 norm does.
    skip_nonfinite (attribute; implies capturable=True): a step whose gradient norm is NaN or Inf stores nothing -- parameters,
    moments and step counts stay bit for bit -- and `skipped_steps` goes up by one.  Without it a non-finite norm does what torch does.
    `grad_norm`, `clip_coef`, `skipped_steps`: device scalars of the last step, read without a synchronisation (None before the first
    step with max_grad_norm or skip_nonfinite).  With neither option and no weight decay, step() launches exactly what it always did."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False, capturable=False, *,
                 max_grad_norm=None, skip_nonfinite=False):
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or not 0.0 <= weight_decay:
            raise ValueError("invalid Adam hyper-parameters")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (None: no clipping)")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=float(weight_decay),
                                      decoupled_weight_decay=bool(decoupled_weight_decay),
                                      capturable=bool(capturable) or bool(skip_nonfinite)))
        self._lr_dev = {}          # group index -> [device scalar, last value pushed]
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._norm = None          # {"partials": float64 [chunks], "scalars": fp32 [norm, coef, ok], "skipped": int32 []}

    def __setstate__(self, state):
        super().__setstate__(state)
        for k, v in (("max_grad_norm", None), ("skip_nonfinite", False), ("_norm", None)):      # pickled before the options existed
            self.__dict__.setdefault(k, v)

    @property
    def grad_norm(self):
        return None if self._norm is None else self._norm["scalars"][0]

    @property
    def clip_coef(self):
        return None if self._norm is None else self._norm["scalars"][1]

    @property
    def skipped_steps(self):
        return None if self._norm is None else self._norm["skipped"]

    def _norm_launches(self, grads):
        """sumsq over `grads` (every gradient of every group, in param_groups order), then the finish launch into our scalars."""
        dev = grads[0].device
        chunks = sum(_norm_chunks(g) for g in grads)
        if self._norm is None or self._norm["partials"].numel() < chunks or self._norm["partials"].device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.BBBHipError("FusedAdam's gradient-norm buffers must exist before a capture: run one step eagerly first")
            skipped = self._norm["skipped"] if self._norm is not None and self._norm["skipped"].device == dev else \
                torch.zeros((), dtype=torch.int32, device=dev)
            if self._norm is not None:               # a step captured earlier reads the buffers this replaces: drop it (train._auto_key)
                self._state_generation = getattr(self, "_state_generation", 0) + 1
            self._norm = {"partials": torch.zeros(chunks, dtype=torch.float64, device=dev),
                          "scalars": torch.tensor([0.0, 1.0, 1.0], dtype=torch.float32, device=dev), "skipped": skipped}
        sc = self._norm["scalars"]
        _grad_norm_into(grads, self._norm["partials"], self.max_grad_norm, self.skip_nonfinite, sc.data_ptr(), sc.data_ptr() + 4,
                        sc.data_ptr() + 8, self._norm["skipped"].data_ptr())

    def make_capturable(self):
        """Switch every group to the capturable convention in place: 'step' counts move to the device (same values)."""
        for group in self.param_groups:
            if group.get("capturable", False):
                continue
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st and not st["step"].is_cuda:
                    st["step"] = st["step"].to(device=p.device, dtype=torch.float32)
            group["capturable"] = True

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # new 'step' / 'exp_avg' / 'exp_avg_sq' tensors replaced the ones an earlier capture (train_step's self-capture,
        # GraphedTrainStep) baked in: the generation is part of train_step's capture key, so such a graph is dropped
        self._state_generation = getattr(self, "_state_generation", 0) + 1
        for rec in self._lr_dev.values():     # the captured step keeps reading OUR scalars: refresh them from the loaded lr
            rec[1] = None
        if self._lr_dev and not torch.cuda.is_current_stream_capturing():
            self.sync_lr()

    def sync_lr(self):
        """Push every capturable group's current lr to its device scalar (call outside a graph capture, e.g. after
        scheduler.step(); GraphedTrainStep.step does it before each replay)."""
        for gi, group in enumerate(self.param_groups):
            rec = self._lr_dev.get(gi)
            if rec is not None and rec[1] != float(group["lr"]):
                rec[0].fill_(float(group["lr"]))
                rec[1] = float(group["lr"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.lib()
        touched = []
        guarded = self.max_grad_norm is not None or self.skip_nonfinite
        coef_dev = ok_dev = 0
        if guarded:
            if self.skip_nonfinite and any(not g.get("capturable", False) for g in self.param_groups):
                self.make_capturable()
            grads = [p.grad for group in self.param_groups for p in group["params"] if p.grad is not None]
            if grads:
                for g in grads:
                    _lib.require_device(g)
                    if not g.is_contiguous() or g.device != grads[0].device:
                        raise _lib.BBBHipError("FusedAdam needs contiguous gradients on one device")
                self._norm_launches(grads)
                sc = self._norm["scalars"]
                coef_dev = sc.data_ptr() + 4 if self.max_grad_norm is not None else 0
                ok_dev = sc.data_ptr() + 8 if self.skip_nonfinite else 0
        for gi, group in enumerate(self.param_groups):
            cap = group.get("capturable", False)
            wd, decoupled = float(group.get("weight_decay", 0.0)), bool(group.get("decoupled_weight_decay", False))
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                _lib.require_device(p, p.grad)
                if not p.is_contiguous() or not p.grad.is_contiguous():
                    raise _lib.BBBHipError("FusedAdam needs contiguous parameters and gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if cap else torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if cap:
                    by_step.setdefault(0, []).append((p, st))
                else:
                    st["step"] += 1
                    by_step.setdefault(int(st["step"].item()), []).append((p, st))
            lr_dev = 0
            if cap and by_step:
                steps = [st["step"] for _, st in by_step[0]]
                if any(not t.is_cuda for t in steps):
                    raise _lib.BBBHipError("capturable FusedAdam needs its 'step' state on the device")
                # one launch; all tensors of a group step together (a guarded step adds `ok`: 0 when it is skipped)
                # (the tensor-LIST overload: a tensor given as the scalar would be read on the host, which a capture forbids)
                if ok_dev:
                    torch._foreach_add_(steps, [self._norm["scalars"][2]] * len(steps))
                else:
                    torch._foreach_add_(steps, 1.0)
                # the device-side learning rate lives in a private dict keyed by group index, NOT in param_groups: state_dict()
                # stays interchangeable with torch.optim.Adam's, and load_state_dict / map_location cannot swap or move the
                # scalar a captured step reads
                if gi not in self._lr_dev:
                    self._lr_dev[gi] = [torch.full((), float(group["lr"]), dtype=torch.float32, device=steps[0].device), float(group["lr"])]
                elif not torch.cuda.is_current_stream_capturing():
                    self.sync_lr()
                lr_dev = self._lr_dev[gi][0].data_ptr()
            ex = wd != 0.0 or coef_dev != 0 or ok_dev != 0
            for step, items in by_step.items():
                for s0 in range(0, len(items), _lib.MAX_SEGMENTS):
                    part = items[s0:s0 + _lib.MAX_SEGMENTS]
                    segs = (AdamSegment * len(part))()
                    for i, (p, st) in enumerate(part):
                        segs[i].param, segs[i].grad = p.data_ptr(), p.grad.data_ptr()
                        segs[i].exp_avg, segs[i].exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                        segs[i].n = p.numel()
                    dev = part[0][0].device
                    step_dev = part[0][1]["step"].data_ptr() if cap else 0
                    with torch.cuda.device(dev):
                        if ex:
                            check(L.bbb_adam_step_ex(segs, len(part), float(group["lr"]), float(group["betas"][0]),
                                                     float(group["betas"][1]), float(group["eps"]), wd, int(decoupled), step, step_dev,
                                                     lr_dev, coef_dev, ok_dev, cur_stream(dev)), "bbb_adam_step_ex")
                        else:
                            check(L.bbb_adam_step(segs, len(part), float(group["lr"]), float(group["betas"][0]),
                                                  float(group["betas"][1]), float(group["eps"]), step, step_dev, lr_dev, cur_stream(dev)),
                                  "bbb_adam_step")
                    touched += [p for p, _ in part]
        _bump_versions(touched)
        return loss


class FusedAdamW(FusedAdam):
    """FusedAdam with decoupled weight decay: torch.optim.AdamW's defaults (weight_decay 1e-2)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, capturable=False, *, max_grad_norm=None,
                 skip_nonfinite=False):
        super().__init__(params, lr, betas, eps, weight_decay, True, capturable, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)


def _norm_chunks(t):
    return (t.numel() - 1) // ops.GRAD_NORM_CHUNK + 1


def _grad_norm_into(grads, partials, max_norm, skip, norm_ptr, coef_ptr, ok_ptr, skipped_ptr):
    """bbb_grad_sumsq over `grads` in launches of 16, then ONE bbb_grad_norm_finish: the documented launch order."""
    L = _lib.lib()
    dev = grads[0].device
    first = 0
    with torch.cuda.device(dev):
        stream = cur_stream(dev)
        for s0 in range(0, len(grads), _lib.MAX_SEGMENTS):
            part = grads[s0:s0 + _lib.MAX_SEGMENTS]
            segs = (AdamSegment * len(part))()
            for i, g in enumerate(part):
                segs[i].grad, segs[i].n = g.data_ptr(), g.numel()
            check(L.bbb_grad_sumsq(segs, len(part), partials.data_ptr(), first, stream), "bbb_grad_sumsq")
            first += sum(_norm_chunks(g) for g in part)
        check(L.bbb_grad_norm_finish(partials.data_ptr(), first, float("inf") if max_norm is None else float(max_norm), int(bool(skip)),
                                     norm_ptr, coef_ptr, ok_ptr, skipped_ptr, stream), "bbb_grad_norm_finish")


def grad_norm(params):
    """The global L2 norm of gradients as FusedAdam(max_grad_norm=...) takes it -- float64 accumulation, one rounding to fp32 -- without
    an optimizer, for logging: a 0-d device tensor, no synchronisation.  params: tensors whose .grad is taken (one that requires a
    gradient and has none is left out), or gradient tensors themselves (no .grad, no requires_grad)."""
    grads = [g for g in ((t.grad if (t.grad is not None or t.requires_grad) else t) for t in params) if g is not None]
    if not grads:
        raise _lib.BBBHipError("grad_norm: no gradients")
    for g in grads:
        _lib.require_device(g)
        if not g.is_contiguous() or g.device != grads[0].device:
            raise _lib.BBBHipError("grad_norm needs contiguous gradients on one device")
    partials = torch.empty(sum(_norm_chunks(g) for g in grads), dtype=torch.float64, device=grads[0].device)
    out = torch.empty((), dtype=torch.float32, device=grads[0].device)
    _grad_norm_into(grads, partials, None, False, out.data_ptr(), 0, 0, 0)
    return out


def _bump_versions(params):
    """The HIP kernels write parameters through raw pointers: tell torch (Tensor._version) so that version-keyed caches --
    the split-fp16 weight bound, the speculation cache of layers/_fused.py, fast_train's stale-parameter check -- see the
    update.  Host-side bookkeeping only (legal inside a capture; replays are bumped by GraphedTrainStep.step)."""
    if params:
        torch.autograd.graph.increment_version(params)


def allreduce_gradients(params, group=None, bucket_bytes=64 << 20):
    """Data-parallel gradient averaging: gradients are packed into flat fp32 buckets (one for a BayesianAlexNet: 20 MB)
    and each bucket is ONE all_reduce (RCCL on GPUs); sum / world, written back in place.  Every rank must call this
    with the same parameter order.  Returns the number of collectives issued."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    grads = [p.grad for p in params if p.grad is not None]
    if world == 1 or not grads:
        return 0
    n_coll, i = 0, 0
    while i < len(grads):
        j, size = i, 0
        while j < len(grads) and (j == i or size + grads[j].numel() * 4 <= bucket_bytes):
            size += grads[j].numel() * 4
            j += 1
        flat = torch.cat([g.reshape(-1) for g in grads[i:j]])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        flat.div_(world)
        off = 0
        for g in grads[i:j]:
            g.copy_(flat[off:off + g.numel()].view_as(g))
            off += g.numel()
        n_coll += 1
        i = j
    return n_coll


def elbo(log_outputs, target, kl, beta, train_size):
    """metrics.ELBO.forward (metrics.py:7-14): nll_loss(mean) * train_size + beta * kl."""
    return F.nll_loss(log_outputs, target, reduction="mean") * train_size + beta * kl


def _check_train_precision(precision):
    if precision not in ("fp32", "bf16"):
        raise _lib.BBBHipError(f"training precision must be 'fp32' or 'bf16', got {precision!r}")


def _check_likelihood(likelihood, x, target):
    if not isinstance(likelihood, GaussianLikelihood):
        raise _lib.BBBHipError(f"likelihood must be a train.GaussianLikelihood or None, got {type(likelihood).__name__}")
    _lib.require_device(x)
    if not torch.is_tensor(target) or target.dim() != 2 or target.shape[0] != x.shape[0] or target.dtype != torch.float32:
        raise _lib.BBBHipError("with a Gaussian likelihood the target is y [B, D], fp32")
    _lib.require_device(target)


def forward_loss(net, x, target, num_ens, beta, train_size, seed_call=None, param_alias=None, precision="fp32", likelihood=None):
    """The forward half of a training iteration (main_bayesian.py:43-56): num_ens stochastic forwards batched over the draws,
    kl of one forward (= the reference's kl / num_ens), logmeanexp, ELBO -> (loss, log_outputs, kl).  On the batch-innermost
    autograd path the loss tail is two HIP launches forward and one backward (ops.elbo_cb_autograd); elsewhere torch ops.
    seed_call: (seed, call0) reserved by the caller (a captured step); default: num_ens fresh call indices.
    precision: "fp32" (the reference's arithmetic) or "bf16" -- sampled weights, activations and the gradients passed between
    layers stored as bf16, parameters, their gradients, KL and the loss fp32; BBB models on the
    batch-innermost training path with B % 8 == 0 only, anything else raises BBBHipError.
    likelihood: None (the categorical path above) or a GaussianLikelihood -- regression: target is y [B, D] fp32, the model's last
    Bayesian linear layer has 2 D (heteroscedastic) or D outputs, and the return is (loss, LL [B], kl) with LL the per-image
    log-likelihood of gaussian_elbo.  The logits come from the same forward (the same autograd nodes, in either precision); the tail
    is two HIP launches forward and one backward (ops.gauss_elbo_cb_autograd), or gaussian_elbo for what it refuses."""
    _check_train_precision(precision)
    if likelihood is not None:
        _check_likelihood(likelihood, x, target)
    if precision == "bf16" and torch.is_grad_enabled():
        from . import fast_train
        why = fast_train.bf16_train_refusal(net, x) if ensemble.fast_autograd else "the batch-innermost autograd path"
        if why is not None:
            raise _lib.BBBHipError("bf16 training covers " + why)
    if seed_call is None:
        rng.assign_stream_ids(net)
        seed_call = rng.next_calls(int(num_ens))
    req = [target, beta, float(train_size), None] + ([likelihood] if likelihood is not None else [])
    log_outputs, kl = ensemble._local_lse(net, x, int(num_ens), seed_call[0], seed_call[1], int(num_ens), param_alias=param_alias, elbo=req,
                                          precision=precision)
    if likelihood is not None:
        return req[3], log_outputs, kl                # (ensemble._autograd_tail: a Gaussian request always leaves with its loss)
    loss = req[3] if req[3] is not None else elbo(log_outputs, target, kl, beta, train_size)
    return loss, log_outputs, kl


auto_graph = {"enabled": True, "after": 3,       # train_step captures itself once this many identical calls in a row were seen,
              "max_rows": 2048}                  # for steps of fewer than this many (image x draw) rows: larger steps are GPU-bound, and launch by
                                                 # launch their weight gradients overlap the input gradients on a second stream, which a
                                                 # captured step cannot do profitably (bs 512 x 10: 2.83 ms eager, 3.04 captured)



class _AutoState(dict):
    """Per-net self-capture state; copies and pickles of the net do not take it along (a captured graph belongs to one module)."""

    def __deepcopy__(self, memo):
        return _AutoState()

    def __reduce__(self):
        return (_AutoState, ())


class _AutoStates:
    """net -> {"key", "streak", "graphed"}, kept ON the module (net.__dict__): the captured step references its net, so a
    WeakKeyDictionary entry would keep its own key alive for ever; a net -> state -> step -> net cycle is ordinary garbage."""

    @staticmethod
    def get(net, default=None):
        return net.__dict__.get("_bbb_train_auto") or default        # (an empty state = a copied net's placeholder)

    def __getitem__(self, net):
        return net.__dict__["_bbb_train_auto"]

    def __setitem__(self, net, st):
        net.__dict__["_bbb_train_auto"] = _AutoState(st)

    @staticmethod
    def pop(net, default=None):
        return net.__dict__.pop("_bbb_train_auto", default)


_auto = _AutoStates()


def _python_hooks(net, optimizer):
    """Anything a graph replay would silently skip: module / tensor / optimizer hooks."""
    import torch.nn.modules.module as _m
    if (_m._global_forward_hooks or _m._global_forward_pre_hooks or _m._global_backward_hooks or _m._global_backward_pre_hooks
            or optimizer._optimizer_step_pre_hooks or optimizer._optimizer_step_post_hooks):
        return True
    for m in net.modules():
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks:
            return True
    return any(getattr(p, "_backward_hooks", None) for p in net.parameters())


def _auto_key(net, optimizer, x, target, num_ens, train_size, precision="fp32", likelihood=None):
    """What a captured step bakes in; None = this call cannot be a graph replay (-> eager)."""
    if not (auto_graph["enabled"] and isinstance(optimizer, FusedAdam) and torch.is_tensor(x) and x.is_cuda and target.is_cuda
            and torch.is_grad_enabled() and not x.requires_grad and not torch.cuda.is_current_stream_capturing()):
        return None
    # parameter STORAGE and optimizer-state identity are baked into a captured step too: net.to(...), `p.data = ...` or
    # optimizer.load_state_dict(...) after the capture must drop it (the replay would read and write freed buffers)
    groups = tuple((tuple(g["betas"]), float(g["eps"]), float(g.get("weight_decay", 0.0)), bool(g.get("decoupled_weight_decay", False)),
                    tuple((id(p), p.requires_grad, p.data_ptr()) for p in g["params"]))
                   for g in optimizer.param_groups)
    from . import rng
    return (id(optimizer), getattr(optimizer, "_state_generation", 0), tuple(x.shape), x.dtype, tuple(target.shape), target.dtype,
            int(num_ens), float(train_size), net.training,
            ensemble._epoch[0], groups, rng.next_calls(0)[0],               # the noise seed is a constant of the captured kernels
            ops.current_config().bf16_strided_train,                        # (what bf16_train_refusal admits: switched off, it must refuse again)
            ops.current_config().bf16_avgpool,                              # (likewise)
            getattr(optimizer, "max_grad_norm", None), getattr(optimizer, "skip_nonfinite", False),   # constants of the captured norm and Adam launches
            likelihood.key() if likelihood is not None else None,           # (a categorical and a Gaussian step never replay each other)
            precision)                                                      # (the precision stays the LAST field: callers read key[-1])


def train_step(net, optimizer, x, target, num_ens, beta, train_size, dp_group=None, graph=None, precision="fp32", likelihood=None):
    """One iteration of train_model's batch loop (main_bayesian.py:40-58): zero_grad, num_ens stochastic forwards
    (batched over draws), kl / num_ens, logmeanexp, ELBO, backward, [gradient all-reduce], optimizer.step.
    dp_group: data-parallel process group whose ranks hold different shards of the batch (parameters replicated).
    Returns (loss, log_outputs, kl) detached.

    A fixed-shape loop is host-bound when run launch by launch (~40 launches + autograd bookkeeping per iteration), so by default
    (graph=None) the step captures ITSELF: once the same (optimizer, shapes, num_ens, train_size, parameter set) was seen
    auto_graph["after"] times in a row, single-process, with a FusedAdam and no Python hooks on the model, the call runs one more
    eager iteration on a capture stream, records it as a GraphedTrainStep and replays that from then on (beta and the learning
    rate stay run-time values; a non-capturable FusedAdam is switched to capturable in place).  Any change of the key drops the
    graph and returns to launch-by-launch steps.  graph=False: never capture.  Same noise calls, same results as the eager
    sequence (tests/test_gpu_train.py).
    precision: "fp32" or "bf16" (forward_loss); part of the self-capture key, so fp32 and bf16 calls never replay each other's graph.
    likelihood: None or a GaussianLikelihood (forward_loss): target is then y [B, D] and the return (loss, LL [B], kl); its fields are
    part of the self-capture key too.  dp_group works as for the categorical loss (the loss is local)."""
    _check_train_precision(precision)
    if likelihood is not None:
        _check_likelihood(likelihood, x, target)
    small = graph is True or x.shape[0] * int(num_ens) < int(auto_graph.get("max_rows", 1 << 62))     # (graph=True: capture whatever the size)
    key = _auto_key(net, optimizer, x, target, num_ens, train_size, precision, likelihood) if (graph is not False and dp_group is None and small) else None
    st = _auto.get(net)
    if key is None or st is None or st["key"] != key:
        if key is not None:
            _auto[net] = {"key": key, "streak": 0, "graphed": None}
            st = _auto[net]
        else:
            _auto.pop(net, None)
    if key is not None:
        if st["graphed"] is not None:
            loss, log_outputs, kl = st["graphed"].step(x, target, beta)
            return loss.clone(), log_outputs.clone(), kl.clone()          # the graph's outputs are overwritten by the next replay
        st["streak"] += 1
        if st["streak"] > int(auto_graph["after"]) and not _python_hooks(net, optimizer):
            optimizer.make_capturable()
            g = GraphedTrainStep(net, optimizer, x, target, num_ens, beta, train_size, warmup=1, weak_net=True,   # the warm-up IS this iteration
                                 precision=precision, likelihood=likelihood)
            if g.graph is not None:
                st["graphed"] = g
            else:
                st["streak"] = -(1 << 60)            # capture refused (stale gradient accumulators): launch by launch from here on
            return g.warm_loss.clone(), g.warm_log_outputs.clone(), g.warm_kl.clone()
    optimizer.zero_grad()
    loss, log_outputs, kl = forward_loss(net, x, target, num_ens, beta, train_size, precision=precision, likelihood=likelihood)
    loss.backward()
    if dp_group is not None:
        allreduce_gradients([p for g in optimizer.param_groups for p in g["params"]], dp_group)
    optimizer.step()
    return loss.detach(), log_outputs.detach(), kl.detach()


class GraphedTrainStep:
    """train_step captured as ONE hipGraph: Monte-Carlo forward with autograd, ELBO, backward, noise-counter increment
    and the Adam update replay as a single graph launch (the eager step is host-bound: ~40 kernel launches plus autograd
    bookkeeping per iteration).  Fresh noise per replay through the same device-side call counter as GraphedMC (the
    backward kernel reads it too, so it regenerates the forward's eps); the Adam step count lives on the device.
    Fixed shapes: copy each batch into `self.x` / `self.target` (or pass them to step()).  train_size is a constant of the
    captured graph; the KL weight `beta` (a per-batch schedule in the reference: metrics.get_beta, main_bayesian.py:55) and
    the learning rate (ReduceLROnPlateau, main_bayesian.py:118) are DEVICE scalars the graph reads at run time:
    step(beta=...) sets the former, optimizer.param_groups[i]['lr'] is pushed before every replay.
    `warmup` real training iterations run eagerly on the capture stream first.
    The optimizer must be FusedAdam(capturable=True) (or another capturable optimizer that keeps lr on the device).
    precision: "fp32" or "bf16" (forward_loss), a constant of the captured graph; likelihood: None or a GaussianLikelihood
    (forward_loss), a constant of the captured graph too -- step() then takes y [B, D] as its target and returns (loss, LL [B], kl)."""

    def __init__(self, net, optimizer, x, target, num_ens, beta, train_size, warmup=3, weak_net=False, launch_config=None,
                 precision="fp32", likelihood=None):
        from . import rng
        _lib.require_device(x)
        _check_train_precision(precision)
        self.precision = precision
        if likelihood is not None:
            _check_likelihood(likelihood, x, target)
        self.likelihood = likelihood
        self.launch_config = (launch_config if launch_config is not None else ops.current_config()).copy()
        # weak_net (train_step's self-capture keeps this object ON the net): no net -> state -> step -> net cycle, so dropping the
        # net frees the graph then and there instead of whenever the cyclic collector runs (possibly inside another capture)
        self._net = weakref.ref(net) if weak_net else (lambda n=net: n)
        self.opt, self.num_ens = optimizer, int(num_ens)
        self.train_size = float(train_size)
        self.x, self.target = x.clone(), target.clone()
        dev = x.device
        self.beta = torch.full((), float(beta), dtype=torch.float32, device=dev)
        self.counter = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.seed, self.call0 = rng.next_calls(0)
        self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        import warnings
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            with torch.cuda.stream(self.stream), rng.device_call_offset(self.counter):
                for _ in range(max(1, int(warmup))):
                    self.opt.zero_grad(set_to_none=True)
                    self.warm_loss, self.warm_log_outputs, self.warm_kl = self._body()      # results of the last eager iteration
                    rng.next_calls(self.num_ens)
        self._next_call = rng.next_calls(0)[1]
        torch.cuda.current_stream(dev).wait_stream(self.stream)
        torch.cuda.synchronize(dev)
        # A parameter's gradient accumulator from an earlier backward on ANOTHER stream, kept alive by a still-referenced
        # non-detached output of that forward, makes autograd synchronise with that stream -- fine in the warm-up iterations above
        # (torch warns), fatal inside a capture (observed: a segmentation fault in capture_end).  Refuse to capture instead.
        self.capture_refused = next((str(w.message).split(".")[0] for w in seen if "AccumulateGrad node's stream" in str(w.message)), None)
        for w in seen:
            if "AccumulateGrad node's stream" not in str(w.message):
                warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
        self.graph = None
        self.replays = 0
        if self.capture_refused:
            return
        self.graph = torch.cuda.CUDAGraph()
        self.opt.zero_grad(set_to_none=True)
        with rng.device_call_offset(self.counter), ops.graph_capture(self.graph, self.stream):
            self.loss, self.log_outputs, self.kl = self._body()

    @property
    def net(self):
        return self._net()

    def _body(self):
        with ops.use_config(self.launch_config), ops.scratch_scope(self):
            return self._body_inner()

    def _body_inner(self):
        from . import fast_train
        params = [p for g in self.opt.param_groups for p in g["params"] if p.requires_grad]
        # The autograd graph of a captured step is rooted at FRESH leaves that share the parameters' storage, and differentiated
        # with torch.autograd.grad: the parameters' own gradient accumulators never take part.  (One that an earlier backward
        # created on another stream -- kept alive by a still-referenced, non-detached output of that forward -- makes autograd
        # synchronise with that stream: harmless eagerly, a segmentation fault inside a capture.)  The batch-innermost training
        # path takes the leaves as arguments; on the reference-layout path the layers read their own parameters, and the
        # warm-up iteration's stream-mismatch warning is the (best-effort) signal to refuse the capture.
        alias = None
        if ensemble.fast_autograd and fast_train.train_path_ok(self.net, self.x):
            alias = {id(p): p.detach().requires_grad_(True) for p in params}
        loss, log_outputs, kl = forward_loss(self.net, self.x, self.target, self.num_ens, self.beta, self.train_size,   # kl of one forward
                                             seed_call=(self.seed, self.call0), param_alias=alias,           # = kl / num_ens of the sum
                                             precision=self.precision, likelihood=self.likelihood)
        leaves = params if alias is None else [alias[id(p)] for p in params]
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
        for p, g in zip(params, grads):
            p.grad = g                               # (captured: the tensor lives in the graph's pool; replays rewrite it in place)
        self.counter.add_(self.num_ens)              # after backward: it regenerates eps from the same counter value
        self.opt.step()
        return loss.detach(), log_outputs.detach(), kl.detach()

    def step(self, x=None, target=None, beta=None):
        from . import rng
        if self.graph is None:
            raise _lib.BBBHipError("this step was not captured: " + str(self.capture_refused) + " (drop the references to the "
                                   "outputs of earlier non-detached forwards, then build the GraphedTrainStep again)")
        if x is not None:
            self.x.copy_(x, non_blocking=True)
        if target is not None:
            self.target.copy_(target, non_blocking=True)
        if beta is not None:
            self.beta.fill_(float(beta))
        if hasattr(self.opt, "sync_lr"):
            self.opt.sync_lr()
        seed, call = rng.next_calls(0)
        if call != self._next_call:                  # someone else drew noise in between (a validation pass): follow the host counter
            d = (call - self.call0) & 0xFFFFFFFF
            self.counter.fill_(d - (1 << 32) if d >= (1 << 31) else d)     # the kernels add it modulo 2^32
        self.graph.replay()
        self.replays += 1
        _bump_versions([p for g in self.opt.param_groups for p in g["params"] if p.requires_grad])   # the replay rewrote them
        rng.next_calls(self.num_ens)                 # keep the host-side noise counter in step with the device's
        self._next_call = call + self.num_ens
        return self.loss, self.log_outputs, self.kl
