"""The one place a bbb_conv_desc_t is built (include/bbb_hip.h), and the one rule by which a launch's output slab finds its input
slab and weight set.  Pure: shapes come in as tuples, no tensor and no device is touched; the per-launch wrappers of bbb_hip.ops and
their plan queries all describe their launch through here."""
from ._lib import BBBHipError, ConvDesc

ACT_CODE = {None: 0, "none": 0, "relu": 1, "softplus": 2}


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _out(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def out_map(h, w, kernel, stride, padding, dilation):
    """(Ho, Wo) of a convolution over an h x w map."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(kernel), _pair(stride), _pair(padding), _pair(dilation)
    return _out(h, kh, sh, ph, dh), _out(w, kw, sw, pw, dw)


def conv_desc(batch, cin, hw, cout, khkw, stride=1, padding=0, dilation=1, draws=1, act=None, *, x_planes=1, w_stride=None, b_stride=None):
    """-> (descriptor, Ho, Wo) of `draws` slabs of a layer: batch images of cin channels on an hw map, cout filters of khkw taps.
    Every slab has its own operands: the input slabs are x_planes * cin * h * w * batch elements apart (x_planes: 3 for the split
    format S3, 6 for six-plane c8 S3), the weight sets w_stride (default: dense fp32 [cout, cin, kh, kw]) and the biases b_stride
    (default cout); slab_rule then says which of them a launch shares."""
    d = ConvDesc()
    (h, w), (kh, kw), (sh, sw), (ph, pw), (dh, dw) = hw, khkw, _pair(stride), _pair(padding), _pair(dilation)
    d.batch, d.cin, d.h, d.w, d.cout, d.kh, d.kw = batch, cin, h, w, cout, kh, kw
    d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = sh, sw, ph, pw, dh, dw
    d.draws = draws
    d.x_draw_stride = x_planes * cin * h * w * batch
    d.w_draw_stride = cout * cin * kh * kw if w_stride is None else w_stride
    d.b_draw_stride = cout if b_stride is None else b_stride
    d.act = ACT_CODE[act]
    return d, _out(h, kh, sh, ph, dh), _out(w, kw, sw, pw, dw)


def slab_rule(d, Ex, Ew, *, units=None, n_units=None, x_per_slice=False, x_div=1, x_off=0, n_slabs=None, weights_shared=False):
    """Which input slab and which weight set output slab e of a launch reads, written into d; -> (E, x is shared, w is shared).
    x holds Ex slabs, w Ew sets (weights_shared: the local-reparameterisation layers' one pair, whatever Ew says).  One of three forms:
      work units   units = (S, off), S > 1: the E = n_units slabs are units u = off + e of the draw-major (draw, batch slice) grid; x
                   holds one slab per unit, or with x_per_slice the S per-slice slabs every draw shares (slab u % S)
      steps        x_div = D > 1 (several steps per launch): slab e reads input slab (e + x_off) // D, 0 <= x_off < D, so x holds
                   ceil((E + x_off) / D) slabs
      plain        x and w each hold E slabs, or one that every slab shares (its draw stride is then 0)
    E is Ew in the last two forms; with weights_shared n_slabs, else Ex * D.  Anything else is refused."""
    S, off = (int(units[0]), int(units[1])) if units is not None else (1, 0)
    D, x_off = int(x_div), int(x_off)
    x_shared = w_shared = False
    if S > 1:
        E = int(n_units)
        if Ex != (S if x_per_slice else E):
            raise BBBHipError("work units: x must hold one slab per unit, or one per batch slice with x_per_slice")
        d.unit_div, d.unit_off, d.x_unit_mod = S, off % S, S if x_per_slice else 0
    else:
        E = Ew if not weights_shared else int(n_slabs) if n_slabs is not None else Ex * D
        if D > 1:
            if not 0 <= x_off < D or Ex != -(-(E + x_off) // D):
                raise BBBHipError("x_div: x must hold ceil((E + x_off) / x_div) input slabs for the E %s" %
                                  ("output slabs" if weights_shared else "weight sets"))
            d.x_unit_div, d.x_unit_off = D, x_off
        else:
            if not weights_shared:
                E = max(Ex, Ew)
            if Ex not in (1, E) or (not weights_shared and Ew not in (1, E)):
                raise BBBHipError("leading (draw) dims of x and w must be 1 or equal" if not weights_shared else
                                  "x must hold one slab, or one per output slab")
            x_shared, w_shared = Ex == 1 and E > 1, Ew == 1 and E > 1
    d.draws = E
    if x_shared:
        d.x_draw_stride = 0
    if w_shared or weights_shared:
        d.w_draw_stride = d.b_draw_stride = 0
    return E, x_shared, w_shared or weights_shared


_C8X3_TILE = {None: 0, 128: 2, 256: 4}
_C8X3_POOL_TILE = {None: 0, 128: 2, 256: 4, 32: 2, 64: 4}       # (a pooled launch: 32 | 64 images per workgroup)


def c8x3_flags(out_f32, tile, zero_border, nt=None, pool=None):
    """The flags word of bbb_conv2d_c8x3_fwd / bbb_lrt_conv2d_c8x3_fwd: bit 0 fp32 output, bits 1-2 the image tile, bit 3 pooled,
    bits 4-7 nt, then the four zero_border counts as nibbles.  pool = None: an entry without the pooled form (and its tiles)."""
    zb = [min(15, int(v)) for v in zero_border]
    return ((1 if out_f32 else 0) | (_C8X3_TILE if pool is None else _C8X3_POOL_TILE)[tile] | (8 if pool else 0) |
            ({None: 0, 2: 2, 3: 3, 4: 4}[nt] << 4) | (zb[0] << 8) | (zb[1] << 12) | (zb[2] << 16) | (zb[3] << 20))


def bf16_flags(out_f32=False, tap_major=False, x_c8=False, out_c8=False):
    """The flags word of the bf16 forward entries and their plan queries."""
    return (1 if out_f32 else 0) | (2 if tap_major else 0) | (4 if x_c8 else 0) | (8 if out_c8 else 0)


def pool_code(pool):
    """bbb_conv_desc_t::pool of the bf16 forward for pool = (k, s) | None: 0 none, 1 the 2 x 2 / 2 window, else k << 8 | s."""
    if pool is None:
        return 0
    k, s = int(pool[0]), int(pool[1])
    return 1 if (k, s) == (2, 2) else (k << 8) | s


def pooled_map(ho, wo, pool):
    """The map behind MaxPool2d(*pool) without padding in floor mode, pool = (k, s), ints or pairs: THE statement of that arithmetic
    for every max pool of the batch-innermost paths (a pooled conv form, a launch of its own).  Stated for any map: where the window
    does not fit, the result is empty or negative and the launch entry is what refuses it."""
    k, s = pool
    if isinstance(k, int) and isinstance(s, int):
        return (ho - k) // s + 1, (wo - k) // s + 1
    (kh, kw), (sh, sw) = (_pair(v) if isinstance(v, (tuple, list)) else (int(v), int(v)) for v in pool)
    return (ho - kh) // sh + 1, (wo - kw) // sw + 1
