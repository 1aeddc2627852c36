"""Uncertainty estimation as a second consumer of the Monte-Carlo forwards.

Mirrors uncertainty_estimation.get_uncertainty_per_image / get_uncertainty_per_batch upstream (lines 37-58, 61-102):
same arguments, same (pred, epistemic, aleatoric) numpy results, but the T forwards run as one batched ensemble
launch and the softmax / moment reduction is one HIP kernel instead of a Python loop over samples with numpy dot/diag.

Beyond the reference: mc_uncertainty returns those moments together with predictive entropy, expected entropy and mutual information
(BALD) as device tensors, from one reduction launch on the batch-innermost logits; GraphedUncertainty is its captured form.
mc_uncertainty(grad=True) carries a gradient through the scores (one backward launch), and saliency returns d score / d input.
"""
import torch

from . import _lib, ensemble, ops, rng


def get_uncertainty_per_image(model, input_image, T=15, normalized=False):
    """The reference repeats the image T times in ONE batch and calls model() once (so with 'bbb' layers all T rows share
    a single weight draw and the epistemic part is ~0; 'lrt' layers decorrelate the rows).  Same semantics here."""
    images = input_image.unsqueeze(0).repeat(T, 1, 1, 1)
    with torch.no_grad():
        net_out, _ = model(images)
        pred, epi, ale = ops.uncertainty(net_out.unsqueeze(1), normalized=normalized)      # T rows = T "draws", B = 1
    return pred[0].cpu().numpy(), epi[0].cpu().numpy(), ale[0].cpu().numpy()


def get_uncertainty_per_batch(model, batch, T=15, normalized=False):
    """T stochastic forwards of the whole batch (fresh weight draws each), reduced per sample: -> [B, C] arrays."""
    with torch.no_grad():
        seed, call0 = rng.next_calls(T)
        logits, _ = ensemble.mc_logits(model, batch.to(next(model.parameters()).device), T, seed, call0)
        pred, epi, ale = ops.uncertainty(logits, normalized=normalized)
    return pred.cpu().numpy(), epi.cpu().numpy(), ale.cpu().numpy()


def mc_uncertainty(net, batch, T=15, normalized=False, precision="fp32", grad=False, want=None):
    """T stochastic forwards of the batch -> ops.Uncertainty (pred, p_mean, epistemic, aleatoric [B, C]; entropy, expected_entropy,
    mutual_info [B]), all on the device and without a synchronisation: the scores active learning, out-of-distribution detection
    and selective prediction rank by.  The logits stay batch-innermost from the forward into ONE reduction launch
    (ops.mc_uncertainty_cb); a model off the batch-innermost path runs ensemble.mc_logits as always and is transposed once, so every
    model gets the same kernel and numerics.  Consumes T noise calls, as get_uncertainty_per_batch does.  precision: as mc_logits.
    grad=True: the same scores WITH a gradient to whatever requires one (the batch, the parameters), autograd left on: the forwards on
    ensemble.mc_logits_cb_autograd, the reduction and its one-launch backward on ops.mc_uncertainty_cb_autograd; want: the fields to
    compute (None: all seven), the others are None.  grad=False ignores requires_grad, as it always did."""
    if not grad:
        with torch.no_grad():
            seed, call0 = rng.next_calls(T)
            logits_cb, _ = ensemble.mc_logits_cb(net, batch.to(next(net.parameters()).device), T, seed, call0, precision=precision)
            return ops.mc_uncertainty_cb(logits_cb, normalized=normalized, want=want)
    _lib.require_device(batch)
    seed, call0 = rng.next_calls(T)
    logits_cb, _ = ensemble.mc_logits_cb_autograd(net, batch, T, seed, call0, precision=precision)
    return ops.mc_uncertainty_cb_autograd(logits_cb, normalized=normalized, want=want)


def mc_regression(net, batch, T=15, likelihood=None, y=None, precision="fp32", want=None):
    """The regression counterpart of mc_uncertainty: T stochastic forwards of the batch under a train.GaussianLikelihood ->
    ops.Moments (mean, epistemic, aleatoric, total [B, D]; with targets y [B, D] also log_density [B], the log of the mixture
    predictive density at y), all on the device and without a synchronisation.  The forwards run on ensemble.mc_logits_cb under
    no_grad, the reduction is ONE launch on the batch-innermost logits (ops.gauss_moments_cb).  Consumes T noise calls, as
    mc_uncertainty does.  precision: as mc_logits.  want: the fields to compute (None: all that y allows).
    Out of scope: a captured class (as GraphedUncertainty) and a differentiable form (as mc_uncertainty(grad=True))."""
    from .likelihood import GaussianLikelihood
    if not isinstance(likelihood, GaussianLikelihood):
        raise _lib.BBBHipError(f"mc_regression needs likelihood=train.GaussianLikelihood(...), got {type(likelihood).__name__}")
    with torch.no_grad():
        seed, call0 = rng.next_calls(T)
        dev = next(net.parameters()).device
        logits_cb, _ = ensemble.mc_logits_cb(net, batch.to(dev), T, seed, call0, precision=precision)
        return ops.gauss_moments_cb(logits_cb, likelihood, y=None if y is None else y.to(dev), want=want)


SCORES = ("entropy", "expected_entropy", "mutual_info")


def saliency(net, x, T=15, score="mutual_info", normalized=False, precision="fp32"):
    """(scores [B], d scores.sum() / d x with the shape of x) of one of the three per-image scores under the next T noise calls:
    epistemic (mutual_info) or total (entropy) saliency maps, the step direction of attacks and defences on BALD.  Works on a
    detached copy of x -- x.grad and every parameter's .grad stay as they are (torch.autograd.grad on the input alone)."""
    if score not in SCORES:
        raise _lib.BBBHipError(f"score must be one of {SCORES}, got {score!r}")
    _lib.require_device(x)
    xg = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        s = getattr(mc_uncertainty(net, xg, T=T, normalized=normalized, precision=precision, grad=True, want=(score,)), score)
        g, = torch.autograd.grad(s.sum(), xg)
    return s.detach(), g


class GraphedUncertainty:
    """mc_uncertainty as one captured hipGraph for a scoring loop over fixed-shape batches: the T forwards of the batch-innermost
    path plus the reduction, built the way ensemble.GraphedLogits is.  step(x) is bit for bit mc_uncertainty(net, x, T, ...) from
    the same generator state and consumes the same T noise calls.  The returned tensors belong to the graph and are overwritten by
    the next step(): clone what is kept.  A model / input off the batch-innermost path raises BBBHipError at construction."""

    def __init__(self, net, x, T, normalized=False, precision="fp32", launch_config=None):
        _lib.require_device(x)
        self.T, self.normalized, self.precision = int(T), bool(normalized), precision
        self.launch_config = (launch_config if launch_config is not None else ops.current_config()).copy()
        self.x = x.detach().clone()
        self.seed, self.call0 = rng.next_calls(0)
        dev = x.device
        with torch.no_grad():
            ensemble._check_precision(precision, net, self.x, True)
            if not ensemble._chwn_ok(net, self.x):
                raise _lib.BBBHipError(_OFF_PATH + ": the model is not made of Bayesian layers, ReLU / Softplus, pooling and "
                                       "FlattenLayer as direct or Sequential-nested children, or the input is not a 4-d batch")
        self.counter = torch.zeros((1,), dtype=torch.int32, device=dev)
        # captured on a throw-away stream, replayed on the caller's current stream, with scratch of its own (see GraphedLogits)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad(), torch.cuda.stream(side), rng.device_call_offset(self.counter), ops.scratch_scope(self):
            for _ in range(2):                       # warm-up on a side stream (allocator, lazy module state, scratch growth)
                self._body(net)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), rng.device_call_offset(self.counter), ops.graph_capture(g, side), ops.scratch_scope(self):
            self.out = self._body(net)
        self.graph = g

    def _body(self, net):
        with ops.use_config(self.launch_config):
            out = ensemble._mc_logits_chwn(net, self.x, self.T, self.seed, self.call0, precision=self.precision)
            if out is None:
                raise _lib.BBBHipError(_OFF_PATH + ": the path has no launch for one of its layers on this input under this "
                                       "launch configuration")
            return ops.mc_uncertainty_cb(out[0], normalized=self.normalized)

    def step(self, x=None):
        """Score batch x (None: the batch already held) under the next T noise calls of the host generator -> ops.Uncertainty."""
        if x is not None and x.data_ptr() != self.x.data_ptr():
            self.x.copy_(x, non_blocking=True)
        seed, call = rng.next_calls(self.T)
        if seed != self.seed:
            rng.rewind((seed, call))
            raise _lib.BBBHipError("the noise seed changed since this GraphedUncertainty was captured: build a new one")
        d = (call - self.call0) & 0xFFFFFFFF
        self.counter.fill_(d - (1 << 32) if d >= (1 << 31) else d)     # the kernels add it modulo 2^32
        self.graph.replay()
        return self.out


_OFF_PATH = ("GraphedUncertainty captures the batch-innermost inference path only, which this model / input does not fit "
             "(mc_uncertainty runs it uncaptured)")
