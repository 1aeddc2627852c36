"""Per-weight Gaussian priors for whole models (layers/_base.py: BayesianLayer.set_prior holds one layer's).

  from_posterior(net, source=None)   the current posterior becomes the prior: variational continual learning, task k -> task k + 1
  moped(net, weights, delta, sigma)  empirical-Bayes prior and posterior initialisation from a trained deterministic network (MOPED)
  clear(net)                         back to the layers' scalar pairs
  state_dict(net) / load_state_dict(net, sd)
                                     the prior TENSORS, keyed "<layer name>.<buffer name>": what a checkpoint needs beside the model's
                                     own state_dict(), which stays interchangeable with the reference's (the buffers are non-persistent)

The KL against these tensors is the parameter pass's own (bbb_reparam_kl_tp_fwd / _bwd: same launch, same plan, closed form).
Tensors are copied into existing buffers of the same shape, so a captured training step or a cached inference graph keeps running
and sees the new values at its next replay; only a change of kind (number <-> tensor, new shape) drops them.
"""
import collections
import collections.abc

import torch
import torch.nn as nn
import torch.nn.functional as F

_BUFFERS = ("W_prior_mu", "W_prior_sigma", "bias_prior_mu", "bias_prior_sigma")


def _is_bayesian(m):
    return hasattr(m, "set_prior") and hasattr(m, "W_mu") and hasattr(m, "W_rho")


def named_layers(net):
    """[(name, layer)] of every Bayesian layer of `net`, in module order."""
    return [(name, m) for name, m in net.named_modules() if _is_bayesian(m)]


def from_posterior(net, source=None):
    """Every Bayesian layer's prior becomes the current posterior of the same-named layer of `source` (default: net itself):
    mu0 = W_mu, sigma0 = softplus(W_rho), likewise the bias.  Detached copies; in place where buffers of that shape exist."""
    src = dict(named_layers(net if source is None else source))
    for name, layer in named_layers(net):
        if name not in src:
            raise KeyError(f"from_posterior: the source has no Bayesian layer named {name!r}")
        s = src[name]
        if s.use_bias != layer.use_bias:
            raise ValueError(f"{name}: the source layer {'has' if s.use_bias else 'has no'} bias, this one {'has' if layer.use_bias else 'has none'}")
        with torch.no_grad():
            kw = dict(mu=s.W_mu.detach().to(layer.W_mu.device), sigma=F.softplus(s.W_rho.detach()).to(layer.W_mu.device))
            if layer.use_bias:
                kw.update(bias_mu=s.bias_mu.detach().to(layer.W_mu.device), bias_sigma=F.softplus(s.bias_rho.detach()).to(layer.W_mu.device))
        layer.set_prior(name=name, **kw)
    return net


def _moped_pairs(net, weights):
    layers = named_layers(net)
    if isinstance(weights, nn.Module):
        det = [m for m in weights.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
        if len(det) != len(layers):
            raise ValueError(f"moped: {len(layers)} Bayesian layers, but the deterministic model has {len(det)} conv / linear layers")
        return [(name, l, d.weight, d.bias) for (name, l), d in zip(layers, det)]
    if isinstance(weights, collections.abc.Mapping):
        out = []
        for name, l in layers:
            if name not in weights:
                raise KeyError(f"moped: no weights for layer {name!r}")
            w, b = weights[name]
            out.append((name, l, w, b))
        return out
    raise TypeError("moped: weights must be an nn.Module or a mapping from layer name to (weight, bias)")


def _rho_of(w, delta):
    # softplus(rho) = delta |w|, |w| clamped below at 1e-6 (a pruned weight must not start with sigma = 0: rho = -inf)
    return torch.log(torch.expm1(delta * w.abs().clamp_min(1e-6)))


def moped(net, weights, delta=0.1, prior_sigma=1.0):
    """MOPED (Krishnan et al., AAAI 2020): per layer the prior mean is the pretrained weight, mu0 = w, with the scalar
    sigma = prior_sigma, and the posterior starts at W_mu = w, softplus(W_rho) = delta |w|; likewise the bias.  weights: an nn.Module
    with conv / linear layers in the same order, or a mapping from layer name to (weight, bias)."""
    if not delta > 0:
        raise ValueError("moped: delta must be > 0")
    for name, layer, w, b in _moped_pairs(net, weights):
        if tuple(w.shape) != tuple(layer.W_mu.shape):
            raise ValueError(f"{name}: pretrained weight has shape {tuple(w.shape)}, the layer {tuple(layer.W_mu.shape)}")
        if layer.use_bias and (b is None or tuple(b.shape) != tuple(layer.bias_mu.shape)):
            raise ValueError(f"{name}: the layer has a bias of shape {tuple(layer.bias_mu.shape)}, the pretrained layer "
                             + ("none" if b is None else str(tuple(b.shape))))
        dev = layer.W_mu.device
        with torch.no_grad():
            w = w.detach().to(device=dev, dtype=torch.float32)
            kw = dict(mu=w, sigma=prior_sigma)
            if layer.use_bias:
                b = b.detach().to(device=dev, dtype=torch.float32)
                kw.update(bias_mu=b)
            layer.set_prior(name=name, **kw)
            layer.W_mu.copy_(w)
            layer.W_rho.copy_(_rho_of(w, delta))
            if layer.use_bias:
                layer.bias_mu.copy_(b)
                layer.bias_rho.copy_(_rho_of(b, delta))
    return net


def clear(net):
    """Back to the scalars: every layer keeps prior_mu / prior_sigma and drops its prior tensors."""
    for name, layer in named_layers(net):
        layer.set_prior(mu=layer.prior_mu, sigma=layer.prior_sigma, name=name)
    return net


def state_dict(net):
    """{"<layer name>.<buffer name>": tensor} of every prior tensor that is set (detached clones)."""
    out = collections.OrderedDict()
    for name, layer in named_layers(net):
        for b in _BUFFERS:
            t = layer._buffers.get(b)
            if t is not None:
                out[f"{name}.{b}" if name else b] = t.detach().clone()
    return out


def load_state_dict(net, sd):
    """Inverse of state_dict: sets the tensors it holds (in place where buffers exist) and clears every other prior tensor."""
    layers = dict(named_layers(net))
    todo = {name: {} for name in layers}
    for key, t in sd.items():
        name, _, b = key.rpartition(".")
        if name not in layers or b not in _BUFFERS:
            raise KeyError(f"priors.load_state_dict: unexpected key {key!r}")
        todo[name][b] = t
    for name, layer in layers.items():
        got = todo[name]
        dev = layer.W_mu.device
        arg = lambda b, scalar: got[b].to(dev) if b in got else scalar
        kw = dict(mu=arg("W_prior_mu", layer.prior_mu), sigma=arg("W_prior_sigma", layer.prior_sigma))
        layer.set_prior(name=name, **kw)                        # (a scalar here clears the bias tensor too: set below if present)
        if layer.use_bias:                                      # (an equal number clears that bias tensor)
            layer.set_prior(bias_mu=arg("bias_prior_mu", layer.prior_mu), bias_sigma=arg("bias_prior_sigma", layer.prior_sigma), name=name)
        elif "bias_prior_mu" in got or "bias_prior_sigma" in got:
            raise KeyError(f"priors.load_state_dict: {name} has no bias")
    return net
