"""Gaussian likelihood for regression models (train.GaussianLikelihood, train.gaussian_elbo): the choices the loss tail and the
predictive moments share, and the plain torch expression of their contract -- what the HIP tail (csrc/gauss_tail.hip through
ops.gauss_elbo_cb_autograd) is compared with and what runs where ops.gauss_elbo_cb_ok refuses."""
import math

import torch

from . import _lib

LOG_2PI = math.log(2.0 * math.pi)
MC_MODES = ("logmeanexp", "mean")


class GaussianLikelihood:
    """y [B, D] ~ N(mu, exp(s)) per output, on the C channels of the model's last Bayesian linear layer.
    noise_sigma=None: heteroscedastic, C == 2 D, channel d is the mean and channel D + d the log-variance s.
    noise_sigma > 0 (a Python float, no gradient): homoscedastic, C == D, s = 2 log(noise_sigma).
    s is clamped into [log_var_min, log_var_max] with torch.clamp's gradient.  mc: how the draws of a Monte-Carlo step combine per
    image -- "logmeanexp" (the log of the mixture predictive density, utils.logmeanexp's convention, as the categorical tail) or "mean"
    (the ELBO's expected log-likelihood)."""

    __slots__ = ("noise_sigma", "log_var_min", "log_var_max", "mc")

    def __init__(self, noise_sigma=None, log_var_min=-20.0, log_var_max=20.0, mc="logmeanexp"):
        if noise_sigma is not None:
            noise_sigma = float(noise_sigma)
            if not (noise_sigma > 0.0 and math.isfinite(noise_sigma)):
                raise _lib.BBBHipError(f"noise_sigma must be a finite positive number or None, got {noise_sigma!r}")
        log_var_min, log_var_max = float(log_var_min), float(log_var_max)
        if not log_var_min <= log_var_max:
            raise _lib.BBBHipError(f"log_var_min must not exceed log_var_max, got [{log_var_min}, {log_var_max}]")
        if mc not in MC_MODES:
            raise _lib.BBBHipError(f"mc must be one of {MC_MODES}, got {mc!r}")
        self.noise_sigma, self.log_var_min, self.log_var_max, self.mc = noise_sigma, log_var_min, log_var_max, mc

    def key(self):
        """The fields as a tuple (train._auto_key)."""
        return ("gaussian", self.noise_sigma, self.log_var_min, self.log_var_max, self.mc)

    def channels(self, dims):
        return int(dims) * (2 if self.noise_sigma is None else 1)

    def __repr__(self):
        return "GaussianLikelihood(noise_sigma=%r, log_var_min=%r, log_var_max=%r, mc=%r)" % (self.noise_sigma, self.log_var_min,
                                                                                             self.log_var_max, self.mc)


def check_target(logits_cb, y, lik, what):
    """logits [E, C, B] against targets [B, D] under `lik`; raises BBBHipError by name."""
    if not isinstance(lik, GaussianLikelihood):
        raise _lib.BBBHipError(f"{what}: likelihood must be a train.GaussianLikelihood or None, got {type(lik).__name__}")
    if not torch.is_tensor(y) or y.dim() != 2 or not y.is_floating_point():
        raise _lib.BBBHipError(f"{what}: with a Gaussian likelihood the target is a floating-point y [B, D]")
    if logits_cb.dim() != 3 or logits_cb.shape[2] != y.shape[0] or logits_cb.shape[1] != lik.channels(y.shape[1]):
        form = "2 * D (heteroscedastic)" if lik.noise_sigma is None else "D (homoscedastic)"
        raise _lib.BBBHipError(f"{what}: logits {tuple(logits_cb.shape)} do not fit y {tuple(y.shape)}: [E, C, B] with C == {form}")


def gaussian_elbo(logits_cb, y, kl, beta, train_size, lik, mean_over=0):
    """(loss, LL [B]) of one Monte-Carlo regression step from batch-innermost logits [E, C, B], targets y [B, D] and the KL of one
    forward, as plain torch ops (the counterpart of train.elbo):
      ll = -0.5 (log 2 pi + s_c + (y - mu)^2 exp(-s_c)),  L[e, b] = sum_d ll,
      LL = logsumexp_e L - log(mean_over or E)  (lik.mc == "logmeanexp")  or  mean_e L  ("mean"),
      loss = -(train_size / B) sum_b LL + beta * kl.
    Any floating dtype (the float64 contract tests run it as it is)."""
    check_target(logits_cb, y, lik, "gaussian_elbo")
    E, C, B = logits_cb.shape
    D = y.shape[1]
    mu = logits_cb[:, :D, :]
    if lik.noise_sigma is None:
        s = logits_cb[:, D:, :]
    else:
        s = torch.full((), 2.0 * math.log(lik.noise_sigma), dtype=logits_cb.dtype, device=logits_cb.device)
    sc = torch.clamp(s, lik.log_var_min, lik.log_var_max)
    r = y.t().unsqueeze(0) - mu
    L = (-0.5 * ((LOG_2PI + sc) + r * r * torch.exp(-sc))).sum(dim=1)
    if lik.mc == "logmeanexp":
        LL = torch.logsumexp(L, dim=0) - math.log(mean_over if mean_over > 0 else E)
    else:
        LL = L.sum(dim=0) / E
    return -(train_size / B) * LL.sum() + beta * kl, LL
