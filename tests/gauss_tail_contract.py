"""Contract of the Gaussian-likelihood tail (csrc/gauss_tail.hip: bbb_gauss_elbo_cb_fwd / _bwd, bbb_gauss_moments_cb) for
tests/test_gauss_tail_cpu.py and tests/test_gpu_gauss_tail.py: the named cases, their seeded fp32 inputs, the float64 reference
written from the definitions, an fp32 numpy model of each operation in the kernel's stated order, the error scale of each operation
and the stored model constants.  No device and no library needed.

The device bound of an operation is DEVICE_FACTOR x its constant x U x its scale; the constant is the worst |fp32 model - float64| /
(U x scale) over all cases, rounded up to one significant digit (tests/test_gauss_tail_cpu.py measures it again and compares).
Nothing here is taken from kernel output.

The scales (all from the float64 reference; q = r^2 exp(-s_c)):
  S_L[e, b]   = 0.5 sum_d (log 2 pi + |s_c| + q): the sum of the absolute terms of L.
  S_LL[b]     logmeanexp: sum_e w S_L[e] + S_L[argmax_e L] + |log n| + 1 -- the rounding of each L reaches LL with its weight, every
              L - max inherits the rounding of the maximum, log n is rounded once and log z with z in [1, E] adds the rest;
              mean: (1 / E) sum_e S_L.
  S_loss      = (train_size / B) sum_b S_LL + |beta kl|.
  S_g[e,c,b]  = |c| A (w (1 + S_L[e, b] + S_LL[b]) + TINY) + TINY, c = -(train_size / B) g, A = |r| exp(-s_c) for a mean channel and
              0.5 (q + 1) for a log-variance channel inside the clamp: the product's own rounding plus the error of the weight
              w = exp(L - lse), which is w x the absolute error of L - lse; TINY = 2^-126 / U is where fp32 flushes (a weight
              below 2^-126 is 0 on the device, and in float64 it is not).  Outside the clamp the scale is 0: the gradient is exactly 0.
  mean: (1 / E) sum_e |mu|.   aleatoric: (1 / E) sum_e exp(s_c).   total: the sum of the two variance scales.
  epistemic: (1 / E) sum_e (mu - mean)^2 + U ((1 / E) sum_e |mu|)^2 -- the sum of its terms, not mean^2: in the two-pass form the
              rounding of the mean, delta <= U mean|mu|, cancels to first order (sum_e (mu - mean) = 0) and leaves delta^2, which
              after the division by U is the second summand; with all draws identical it is the whole error.
  log_density: S_LL in the logmeanexp form with n = E."""
import dataclasses
import math
import zlib

import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126 / U
DEVICE_FACTOR = 4        # device expf / logf a few ulp where numpy is close to correctly rounded; another summation order
LOG_2PI = math.log(2.0 * math.pi)

EINVAL, EALIGN, ESHAPE = -1, -2, -3
MAX_DRAWS, MAX_CHANNELS = 512, 1024
THREADS, TILE, LDS_BYTES, LOSS_THREADS = 64, 16, 64 * 17 * 4, 256

FIELDS = ("LL", "loss", "g_logits", "g_kl", "mean", "epistemic", "aleatoric", "total", "log_density")
MOMENTS = FIELDS[4:]
# worst |fp32 model - float64 reference| / (U x scale) over CASES, rounded up to one significant digit
MODEL_CONSTANT = {"LL": 6.0, "loss": 4.0, "g_logits": 3.0, "g_kl": 0.3, "mean": 5.0, "epistemic": 30.0, "aleatoric": 20.0,
                  "total": 9.0, "log_density": 2.0}

BATCHES = (1, 3, 63, 64, 65, 130)
DRAWS = (1, 2, 10, 17)
DIMS = (1, 3, 8, 17)
SIGMAS = (0.1, 1.0, 30.0)
MODES = ("logmeanexp", "mean")
MEAN_OVER = (0, 40)
RECIPES = ("unit", "clamp_edges", "far_draw", "dominant", "identical", "far_targets")
LARGE_E = (512, 1, 4)


def round_up_1sf(x):
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x))
    return float("%de%d" % (math.ceil(x / 10.0 ** e - 1e-9), e))


def bound(field):
    return DEVICE_FACTOR * MODEL_CONSTANT[field]


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    recipe: str
    E: int
    D: int
    B: int
    noise_sigma: object       # None: heteroscedastic
    log_var_min: float
    log_var_max: float
    mc: str
    mean_over: int
    beta: float
    beta_dev: bool
    kl: float
    train_size: float
    g: float                  # upstream gradient of the loss

    @property
    def C(self):
        return self.D * (2 if self.noise_sigma is None else 1)

    @property
    def seed(self):
        return zlib.crc32(self.name.encode())

    @property
    def n(self):
        return self.mean_over if self.mean_over > 0 else self.E


def _build_cases():
    cases = []
    i = 0
    for r in RECIPES:
        for hetero in (True, False):
            for _ in range(4):
                E, D, B = DRAWS[i % 4], DIMS[(i + i // 4) % 4], BATCHES[i % 6]
                if r in ("far_draw", "dominant") and E < 2:
                    E = 2
                sigma = None if hetero else SIGMAS[i % 3]
                lo, hi = ((-3.0, 2.0) if hetero else (-2.0, 2.0)) if r == "clamp_edges" else (-20.0, 20.0)
                mc, mo, dev = MODES[(i // 2) % 2], MEAN_OVER[(i // 3) % 2], bool((i // 4) % 2)
                name = "%s-%s-%dx%dx%d-%s-mo%d-%s" % (r, "het" if hetero else "sig%g" % sigma, E, D, B, mc, mo, "dev" if dev else "host")
                cases.append(Case(name, r, E, D, B, sigma, lo, hi, mc, mo, 0.37 if dev else 0.1, dev, 4321.0 + i, 50000.0,
                                  (1.0, 0.25)[i % 2]))
                i += 1
    E, D, B = LARGE_E
    cases.append(Case("unit-het-%dx%dx%d-logmeanexp-mo0-host" % LARGE_E, "unit", E, D, B, None, -20.0, 20.0, "logmeanexp", 0, 0.1, False,
                      4321.0, 50000.0, 1.0))
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


CASES = _build_cases()


def inputs(c):
    """(logits [E, C, B], y [B, D]) fp32, from the case's own seed."""
    g = np.random.default_rng(c.seed)
    E, D, B = c.E, c.D, c.B
    mu = g.standard_normal((E, D, B))
    s = g.standard_normal((E, D, B))
    y = g.standard_normal((B, D))
    if c.recipe == "clamp_edges":                      # straddles both edges; a quarter exactly at each
        s = g.uniform(c.log_var_min - 5.0, c.log_var_max + 5.0, (E, D, B))
        pick = g.integers(0, 4, (E, D, B))
        s[pick == 0] = c.log_var_min
        s[pick == 1] = c.log_var_max
    elif c.recipe == "far_draw":                       # residuals of 1e3 with s = -10 on the last draw: L near -1e10, weight 0
        mu[E - 1] = y.T + 1e3
        s[E - 1] = -10.0
    elif c.recipe == "dominant":                       # draw 0 fits, the others miss by ~5 standard deviations
        mu[0] = y.T + 0.01 * g.standard_normal((D, B))
        s[0] = -2.0
        mu[1:] += 5.0
        s[1:] = -1.0 + 0.1 * s[1:]
    elif c.recipe == "identical":
        mu[:] = mu[0]
        s[:] = s[0]
    elif c.recipe == "far_targets":
        y = y + 50.0
    logits = np.concatenate([mu, s], axis=1) if c.noise_sigma is None else mu
    return np.ascontiguousarray(logits, F32), np.ascontiguousarray(y, F32)


def reference(c, logits, y):
    """float64, from the definitions.  -> dict of FIELDS plus the intermediates the scales need."""
    X, Y = logits.astype(F64), y.astype(F64)
    E, D, B = c.E, c.D, c.B
    mu = X[:, :D]
    s = X[:, D:] if c.noise_sigma is None else np.full((E, D, B), 2.0 * math.log(c.noise_sigma))
    with np.errstate(all="ignore"):
        sc = np.where(s < c.log_var_min, c.log_var_min, np.where(s > c.log_var_max, c.log_var_max, s))      # (keeps a NaN)
        inside = (s >= c.log_var_min) & (s <= c.log_var_max)
        r = Y.T[None] - mu
        ei = np.exp(-sc)
        q = r * r * ei
        L = (-0.5 * (LOG_2PI + sc + q)).sum(axis=1)
        S_L = (0.5 * (LOG_2PI + np.abs(sc) + q)).sum(axis=1)
        m = L.max(axis=0)

        def lme(n):
            lse = m + np.log(np.exp(L - m).sum(axis=0))
            w = np.exp(L - lse)
            top = np.take_along_axis(S_L, np.argmax(np.where(np.isnan(L), -np.inf, L), axis=0)[None], axis=0)[0]
            return lse - math.log(n), w, (w * S_L).sum(axis=0) + top + abs(math.log(n)) + 1.0

        if c.mc == "logmeanexp":
            LL, w, S_LL = lme(c.n)
        else:
            LL, w, S_LL = L.sum(axis=0) / E, np.full((E, B), 1.0 / E), S_L.sum(axis=0) / E
        gs = c.train_size / B
        loss = -gs * LL.sum() + c.beta * c.kl
        cc = -gs * c.g
        g_mu = cc * w[:, None] * (r * ei)
        A = np.abs(r) * ei
        out = {"LL": LL, "loss": np.array(loss), "g_kl": np.array(c.beta * c.g), "w": w, "L": L}
        sw = w[:, None] * (1.0 + S_L[:, None] + S_LL[None, None]) + TINY
        if c.noise_sigma is None:
            g_s = np.where(inside, cc * w[:, None] * (0.5 * (q - 1.0)), 0.0)
            out["g_logits"] = np.concatenate([g_mu, g_s], axis=1)
            As = np.where(inside, 0.5 * (q + 1.0), 0.0)
            S_g = np.concatenate([abs(cc) * A * sw + TINY, np.where(inside, abs(cc) * As * sw + TINY, 0.0)], axis=1)
        else:
            out["g_logits"], S_g = g_mu, abs(cc) * A * sw + TINY
        mean = mu.sum(axis=0) / E
        epi = ((mu - mean[None]) ** 2).sum(axis=0) / E
        ale = np.exp(sc).sum(axis=0) / E
        abs_mean = np.abs(mu).sum(axis=0) / E
        out.update(mean=mean.T, epistemic=epi.T, aleatoric=ale.T, total=(epi + ale).T)
        ld, _, S_ld = lme(E)
        out["log_density"] = ld
        out["scale"] = {"LL": S_LL, "loss": np.array(gs * S_LL.sum() + abs(c.beta * c.kl)), "g_logits": S_g,
                        "g_kl": np.array(abs(c.beta * c.g)), "mean": abs_mean.T, "epistemic": (epi + U * abs_mean ** 2).T,
                        "aleatoric": ale.T, "total": (epi + U * abs_mean ** 2 + ale).T, "log_density": S_ld}
    return out


def _draw_ll32(c, mu, s, y, e):
    """L[e, :] of the kernel: d ascending, ll = -0.5 * ((log 2 pi + s_c) + (r * r) * exp(-s_c)), all fp32."""
    lo, hi = F32(c.log_var_min), F32(c.log_var_max)
    L = np.zeros(c.B, F32)
    for d in range(c.D):
        sd = s[e, d]
        sc = np.where(sd < lo, lo, np.where(sd > hi, hi, sd)).astype(F32)
        r = y[:, d] - mu[e, d]
        L = L + F32(-0.5) * ((F32(LOG_2PI) + sc) + (r * r) * np.exp(-sc))
    return L


def _reduce32(c, mu, s, y, mc):
    Ls = [_draw_ll32(c, mu, s, y, e) for e in range(c.E)]
    m, z = Ls[0].copy(), np.ones(c.B, F32)
    for L in Ls[1:]:
        if mc == "mean":
            m = m + L
        else:
            up = L > m
            z = np.where(up, z * np.exp(np.where(up, m - L, F32(0))) + F32(1), z + np.exp(np.where(up, F32(0), L - m))).astype(F32)
            m = np.where(up, L, m)
    return Ls, m, z


def model(c, logits, y):
    """fp32 numpy, operation by operation in the kernel's order (csrc/gauss_tail.hip's header comment)."""
    E, D, B = c.E, c.D, c.B
    mu = logits[:, :D]
    s = logits[:, D:] if c.noise_sigma is None else np.full((E, D, B), F32(2.0 * math.log(c.noise_sigma)), F32)
    lo, hi = F32(c.log_var_min), F32(c.log_var_max)
    with np.errstate(all="ignore"):
        Ls, m, z = _reduce32(c, mu, s, y, c.mc)
        LL = m / F32(E) if c.mc == "mean" else (m + np.log(z)) - F32(math.log(c.n))
        part = np.zeros(LOSS_THREADS, F32)
        for b in range(B):
            part[b % LOSS_THREADS] += LL[b]
        k = LOSS_THREADS // 2
        while k > 0:
            part[:k] = part[:k] + part[k:2 * k]
            k //= 2
        gs = F32(c.train_size) / F32(B)
        loss = -(gs * part[0]) + F32(c.beta) * F32(c.kl)
        cc = -gs * F32(c.g)
        lse = m + np.log(z)
        g = np.zeros_like(logits)
        for e in range(E):
            w = np.full(B, F32(1) / F32(E), F32) if c.mc == "mean" else np.exp(Ls[e] - lse)
            cw = cc * w
            for d in range(D):
                sd = s[e, d]
                sc = np.where(sd < lo, lo, np.where(sd > hi, hi, sd)).astype(F32)
                r = y[:, d] - mu[e, d]
                ei = np.exp(-sc)
                g[e, d] = cw * (r * ei)
                if c.noise_sigma is None:
                    g[e, D + d] = np.where((sd >= lo) & (sd <= hi), cw * (F32(0.5) * ((r * r) * ei - F32(1))), F32(0))
        out = {"LL": LL, "loss": np.array(loss), "g_logits": g, "g_kl": np.array(F32(c.beta) * F32(c.g))}
        mean, epi, ale = (np.zeros((B, D), F32) for _ in range(3))
        for d in range(D):
            s_mu, s_ale = np.zeros(B, F32), np.zeros(B, F32)
            for e in range(E):
                s_mu = s_mu + mu[e, d]
                sd = s[e, d]
                s_ale = s_ale + np.exp(np.where(sd < lo, lo, np.where(sd > hi, hi, sd)).astype(F32))
            mn = s_mu / F32(E)
            s_d2 = np.zeros(B, F32)
            for e in range(E):
                dv = mu[e, d] - mn
                s_d2 = s_d2 + dv * dv
            mean[:, d], epi[:, d], ale[:, d] = mn, s_d2 / F32(E), s_ale / F32(E)
        _, m2, z2 = (Ls, m, z) if c.mc == "logmeanexp" else _reduce32(c, mu, s, y, "logmeanexp")
        out.update(mean=mean, epistemic=epi, aleatoric=ale, total=epi + ale, log_density=(m2 + np.log(z2)) - F32(math.log(E)))
    for k, v in out.items():
        assert v.dtype == F32, (k, v.dtype)
    return out


def field_ratio(got, ref, scale):
    """max |got - ref| / (U x scale).  A NaN must be the reference's NaN; where the scale is 0 the value must be the reference's."""
    got, ref, scale = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(scale, F64)
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), "NaN pattern differs from the reference's"
    live = ~nan & ~np.isnan(scale)
    exact = live & (scale == 0)
    assert (got[exact] == ref[exact]).all(), "a value with scale 0 is not the reference's"
    live &= scale > 0
    if not live.any():
        return 0.0
    return float((np.abs(got[live] - ref[live]) / (U * scale[live])).max())


def ratios(got, ref):
    return {f: field_ratio(got[f], ref[f], ref["scale"][f]) for f in FIELDS if f in got and got[f] is not None}
