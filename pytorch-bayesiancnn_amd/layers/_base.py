"""Shared plumbing of the four Bayesian layers: priors, parameters, noise-stream ids, KL cache."""
import torch
from torch.nn import Parameter

from bbb_hip import ops, rng
from .misc import ModuleWrapper

_DEFAULT_PRIORS = {
    "prior_mu": 0,
    "prior_sigma": 0.1,
    "posterior_mu_initial": (0, 0.1),
    "posterior_rho_initial": (-3, 0.1),
}


# Per-weight Gaussian priors (set_prior): non-persistent buffers, None = the scalar prior_mu / prior_sigma for that quantity.
_PRIOR_BUFFERS = ("W_prior_mu", "W_prior_sigma", "bias_prior_mu", "bias_prior_sigma")


def default_device():
    # the reference pins cuda:0 (layers/BBB/BBBConv.py:27); parameters may later be moved with .to()
    return torch.device("cuda:0" if torch.cuda.is_available() else "cpu")


class BayesianLayer(ModuleWrapper):
    """State common to BBB and BBB_LRT layers.

    Parameters W_mu, W_rho, bias_mu, bias_rho (bias pair registered as None without bias) -> the same
    state_dict keys as the reference.  Departures, both deliberate: eps comes from the on-chip Philox
    stream (rng.py) instead of torch's CPU generator, and every tensor follows the parameters' device
    rather than a hard-coded cuda:0 (needed for one-process-per-GPU jobs).
    """

    def _init_bayes(self, weight_shape, n_out, bias, priors):
        self.use_bias = bias
        self.device = default_device()
        priors = dict(_DEFAULT_PRIORS) if priors is None else priors
        self.prior_mu = priors["prior_mu"]
        self.prior_sigma = priors["prior_sigma"]
        self.posterior_mu_initial = priors["posterior_mu_initial"]
        self.posterior_rho_initial = priors["posterior_rho_initial"]
        self.W_mu = Parameter(torch.empty(weight_shape, device=self.device))
        self.W_rho = Parameter(torch.empty(weight_shape, device=self.device))
        if bias:
            self.bias_mu = Parameter(torch.empty(n_out, device=self.device))
            self.bias_rho = Parameter(torch.empty(n_out, device=self.device))
        else:
            self.register_parameter("bias_mu", None)
            self.register_parameter("bias_rho", None)
        for name in _PRIOR_BUFFERS:      # follow .to() / .cuda() / deepcopy, stay out of state_dict(): checkpoints remain the reference's
            self.register_buffer(name, None, persistent=False)
        self._stream_base = rng.new_stream_base()
        self._kl = None
        self._presampled = None      # (w, bias) handed over by a fused whole-model launch
        self.eps_source = None       # None: on-chip Philox.  callable(shape) -> tensor: external noise (replay tests)
        self.reset_parameters()

    def reset_parameters(self):
        # same draw order as the reference: W_mu, W_rho, bias_mu, bias_rho
        self.W_mu.data.normal_(*self.posterior_mu_initial)
        self.W_rho.data.normal_(*self.posterior_rho_initial)
        if self.use_bias:
            self.bias_mu.data.normal_(*self.posterior_mu_initial)
            self.bias_rho.data.normal_(*self.posterior_rho_initial)

    # -- compat: the reference caches W_sigma / bias_sigma as plain attributes during forward -----------
    # (layers/BBB/BBBConv.py:64,69).  Here they are read-only views of the parameters, computed on every read (nothing in this
    # package reads them; upstream recomputes them every forward too): without autograd the sigma of the fused parameter pass
    # (bbb_reparam_kl_fwd's sigma output: the value every sampled weight of a forward is built from) -- NOT cached: writes
    # through `.data` (reset_parameters, a user's p.data.copy_) do not bump the version counter a cache could be keyed on --
    # with autograd enabled on a trainable rho the differentiable torch expression, as upstream.
    def _sigma_of(self, mu, rho, slot):
        if rho is None:
            return None
        if not rho.is_cuda or (torch.is_grad_enabled() and rho.requires_grad):
            return torch.log1p(torch.exp(rho))
        _, sig, _ = ops.reparam_kl_forward([mu.detach()], [rho.detach()], self.prior_mu, self.prior_sigma, [0], 0, 0, draws=1,
                                           sample=False, want_sigma=True, want_kl=False)
        return sig[0]

    @property
    def W_sigma(self):
        return self._sigma_of(self.W_mu, self.W_rho, "_w_sigma_view")

    @property
    def bias_sigma(self):
        return self._sigma_of(self.bias_mu, self.bias_rho, "_b_sigma_view") if self.use_bias else None

    def __getstate__(self):
        st = super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__.copy()
        st = dict(st)
        st.pop("_w_sigma_view", None)
        st.pop("_b_sigma_view", None)
        return st

    def _param_lists(self):
        mus, rhos = [self.W_mu], [self.W_rho]
        ids = [self._stream_base]
        if self.use_bias:
            mus.append(self.bias_mu)
            rhos.append(self.bias_rho)
            ids.append(self._stream_base + 1)
        return mus, rhos, ids

    def _prior_lists(self):
        """Sibling of _param_lists(): [(W_prior_mu, W_prior_sigma), (bias_prior_mu, bias_prior_sigma)] -- entries None where the
        scalar holds -- or None when this layer has no prior tensor at all."""
        b = self._buffers
        wm, ws, bm, bs = (b.get(n) for n in _PRIOR_BUFFERS)
        if wm is None and ws is None and bm is None and bs is None:
            return None
        return [(wm, ws), (bm, bs)] if self.use_bias else [(wm, ws)]

    def _check_prior_tensor(self, who, t, like, positive):
        if like is None:
            raise ValueError(f"{who}: the layer has no bias")
        if tuple(t.shape) != tuple(like.shape):
            raise ValueError(f"{who}: shape {tuple(t.shape)}, the parameter has {tuple(like.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: dtype {t.dtype}, expected torch.float32")
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{who}: non-finite elements")
        if positive and not bool((t > 0).all()):
            raise ValueError(f"{who}: every element must be > 0")

    def _set_prior_tensor(self, name, t, like):
        """Copy into the existing buffer when the shape matches (stable pointer: a captured step sees the new values at its next
        replay); otherwise a new buffer, which is a change of kind.  -> True when the kind changed."""
        cur = self._buffers.get(name)
        src = t.detach()
        if cur is not None and cur.shape == src.shape:
            with torch.no_grad():
                cur.copy_(src)
            return False
        setattr(self, name, src.to(device=like.device, dtype=torch.float32, copy=True).contiguous())
        return True

    def _clear_prior_tensor(self, name):
        if self._buffers.get(name) is None:
            return False
        setattr(self, name, None)
        return True

    def set_prior(self, mu=None, sigma=None, bias_mu=None, bias_sigma=None, name=None):
        """Set the Gaussian prior of this layer.  Every argument: None (leave as it is), a Python number, or a tensor of the
        parameter's shape (fp32, finite, sigma > 0: validated here, once, on the host).
        mu / sigma: a number sets prior_mu / prior_sigma (the reference's attributes) and drops that quantity's tensors, weight and
        bias; a tensor becomes the weight's per-element prior.  bias_mu / bias_sigma: a tensor for the bias; a number must equal
        prior_mu / prior_sigma (the reference has one scalar pair per layer) and drops that bias tensor.
        A tensor given where a buffer of its shape exists is copied into it; any change of kind (number <-> tensor, new shape)
        invalidates captured steps and cached structures.  Every argument is validated before anything is applied: a refused call
        leaves the layer as it was.  name: what the messages call the layer (bbb_hip.priors passes its name in the model; default:
        the class name)."""
        who = name or type(self).__name__
        scalars = {"prior_mu": self.prior_mu, "prior_sigma": self.prior_sigma}           # as they will be after this call
        todo = []                                                                        # (buffer, tensor | None = clear, like)
        for what, val, attr, wname, bname, positive in (("mu", mu, "prior_mu", "W_prior_mu", "bias_prior_mu", False),
                                                        ("sigma", sigma, "prior_sigma", "W_prior_sigma", "bias_prior_sigma", True)):
            if val is None:
                continue
            if torch.is_tensor(val):
                self._check_prior_tensor(f"{who}: prior {what}", val, self.W_mu, positive)
                todo.append((wname, val, self.W_mu))
            else:
                val = float(val) if not isinstance(val, int) else val
                if not (val == val and abs(val) != float("inf")) or (positive and not val > 0):
                    raise ValueError(f"{who}: prior {what} = {val!r}" + (": must be > 0" if positive else ": not finite"))
                scalars[attr] = val
                todo += [(wname, None, None), (bname, None, None)]
        for what, val, attr, bname, positive in (("bias_mu", bias_mu, "prior_mu", "bias_prior_mu", False),
                                                 ("bias_sigma", bias_sigma, "prior_sigma", "bias_prior_sigma", True)):
            if val is None:
                continue
            if torch.is_tensor(val):
                self._check_prior_tensor(f"{who}: prior {what}", val, self.bias_mu if self.use_bias else None, positive)
                todo.append((bname, val, self.bias_mu))
            else:
                if float(val) != float(scalars[attr]):
                    raise ValueError(f"{who}: prior {what} = {val!r} differs from the layer's {attr} = {scalars[attr]!r}: "
                                     "a layer has one scalar pair; pass a tensor for a bias prior of its own")
                todo.append((bname, None, None))
        changed = False
        for attr, val in scalars.items():
            if getattr(self, attr) != val:
                setattr(self, attr, val)
                changed = True
        for bname, t, like in todo:
            changed |= self._clear_prior_tensor(bname) if t is None else self._set_prior_tensor(bname, t, like)
        self.__dict__["_kl"] = None
        if changed:
            from bbb_hip import ensemble
            ensemble._bump_epoch()
        return self

    def kl_loss(self):
        """KL of this layer in the reference's (swapped-argument) form; computed by the fused kernel during
        forward and cached, or on demand if no forward ran since the parameters changed."""
        if self._kl is None:
            mus, rhos, _ = self._param_lists()
            kl, _ = ops.kl_only(mus, rhos, self.prior_mu, self.prior_sigma, priors=self._prior_lists())
            return kl
        return self._kl

    def _take_kl(self, kl):
        self.__dict__["_kl"] = kl                # (a plain attribute: nn.Module.__setattr__ would spend ~2.5 us on its checks)
