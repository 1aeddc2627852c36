// Host-side launch plan of the bf16 pixel-major GEMM family (pconv_bf16.hip, pconv_bf16_lrt.hip): the operand checks the launchers
// share, and the ONE statement of which kernel, tile shape, k-group count and wave specialisation a (descriptor, flags) pair gets.
// The launch entries and their query entries (bbb_conv2d_chwn_bf16_plan, bbb_conv2d_chwn_bf16_dgrad_plan,
// bbb_lrt_conv2d_chwn_bf16_plan) call the same functions here.  Plain C++17: no HIP headers, no device code, so it also compiles
// into a host-only program (tests/host/bf16_plan_check.cpp).
#pragma once
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "conv_desc_check.h"

namespace bf16_plan {

constexpr int BK = 64;                   // k per tile of the tiled kernels
constexpr int LDWB = BK + 8;             // weight row pitch (elements): 144 B
constexpr int KCH = 256;                 // k entries per decode chunk and k-group
constexpr int kWinPasses = 13;           // 16-row passes of the window loader: windows of up to 13 * 16 - 1 = 207 image rows (+ the zero row)

using conv_desc_check::mul_cap;
using conv_desc_check::out_map;
using conv_desc_check::positive_geometry;
inline int64_t cdiv(int64_t n, int64_t t) { return (n + t - 1) / t; }

inline int gcd_i(int a, int b) {
    while (b != 0) { const int t = a % b; a = b; b = t; }
    return a;
}

// ---- operand checks and derived geometry shared by the three launchers ----
struct Geom {
    int32_t ho, wo;      // the output map
    int64_t K, Kp;       // contraction length and the bf16 weight row pitch (K rounded up to 8)
    uint32_t x_inv;      // PConvArgs::x_inv
};

// what differs between the launchers in the 32-bit offset limits: bytes per output element and the bound on an output slab (the LRT
// kernel addresses three outputs through signed offsets), and the rows a weight tile may read past the last channel (LRT: two tiles)
struct Limits { int y_esize; int64_t y_bound; int w_pad_rows; };
constexpr Limits kFwdLimits = {4, 0xFFFE0000LL, 64}, kDgradLimits = {2, 0xFFFE0000LL, 64}, kLrtLimits = {4, 0x7FFE0000LL, 128};

inline int vector_rows(const bbb_conv_desc_t* d, bool tap_major) {
    if (d->batch % 8 != 0) return BBB_ESHAPE;               // rows of 16-byte vectors of 8 bf16 images
    if (tap_major && d->cin % 8 != 0) return BBB_ESHAPE;    // a 16-byte weight vector must not straddle two taps
    return 0;
}

// K, Kp, x_inv and the limits of 32-bit buffer offsets into one draw's slabs, for a launch that writes an ho x wo map
inline int slab_limits(const bbb_conv_desc_t* d, int32_t ho, int32_t wo, const Limits& lim, Geom* g) {
    if ((int64_t)d->cin * d->kh >= (1 << 24)) return BBB_ESHAPE;
    const int64_t K = (int64_t)d->cin * d->kh * d->kw;
    const int64_t Kp = (K + 7) & ~(int64_t)7;
    if (K >= (1 << 24)) return BBB_ESHAPE;           // float-reciprocal k decode is exact below 2^24
    const int64_t x_bytes = mul_cap(mul_cap(mul_cap(d->cin, d->h), d->w), (int64_t)d->batch * 2);
    const int64_t y_bytes = mul_cap(mul_cap(mul_cap(d->cout, ho), wo), (int64_t)d->batch * lim.y_esize);
    if (x_bytes > 0xFFFE0000LL || y_bytes > lim.y_bound || ((int64_t)d->cout + lim.w_pad_rows) * Kp * 2 > 0x7FFFFFFFLL ||
        (int64_t)d->batch * 2 > 0x0FFFFFFFLL)
        return BBB_ESHAPE;
    const uint32_t x_inv = (0xFFFFFFF0u - ((uint32_t)d->batch + 512u) * 2u) & ~15u;   // a ragged last tile reaches < 512 columns past the row
    if (x_bytes > (int64_t)x_inv) return BBB_ESHAPE;
    g->ho = ho; g->wo = wo; g->K = K; g->Kp = Kp; g->x_inv = x_inv;
    return 0;
}

// the geometry part of the kernel-argument block (Args = PConvArgs): the same for every launcher
template <class Args>
inline void fill_geometry(Args& a, const bbb_conv_desc_t* d, const Geom& g, bool tap_major) {
    a.B = d->batch; a.Cin = d->cin; a.H = d->h; a.W = d->w; a.Cout = d->cout; a.kh = d->kh; a.kw = d->kw;
    a.sh = d->stride_h; a.sw = d->stride_w; a.ph = d->pad_h; a.pw = d->pad_w; a.dh = d->dil_h; a.dw = d->dil_w;
    a.Ho = g.ho; a.Wo = g.wo; a.K = (int32_t)g.K; a.Kp = (int32_t)g.Kp; a.khkw = d->kh * d->kw; a.act = d->act;
    a.x_ds = d->x_draw_stride;
    a.y_ds = (int64_t)d->cout * g.ho * g.wo * d->batch;
    a.x_inv = g.x_inv;
    a.wtap = tap_major ? 1 : 0;
}

// ---- the general path: pconv_bf16_kernel / pconv_bf16_lrt_kernel tiles ----
struct TileWork {
    int cout, batch, draws;
    int64_t pixels;
    int64_t items(int shape) const {      // workgroups of the launch under a tile shape
        const int bn = shape == 22 ? 128 : 64, bm = shape == 14 ? 256 : 128;
        return mul_cap(mul_cap(mul_cap(draws, cdiv(cout, bn)), pixels), cdiv(batch, bm));
    }
};
struct TileChoice { int shape, kgs; bool ws; };
struct TileGrid { int32_t Ntiles, G, nbt, Mtiles, per_xcd; int64_t blocks; };

// tile shape: LDS-pipe cycles per unit of useful work (see the kernel comment), including the waste of ragged
// channel / image tiles: 128x128 -> 256, 64x256 -> 288, 64x128 (two waves) -> 320
inline int tile_shape(int cout, int batch) {
    auto waste = [](int n, int t) { return (double)(cdiv(n, t) * t) / (double)n; };
    const double c22 = 256.0 * waste(cout, 128) * waste(batch, 128);
    const double c14 = 288.0 * waste(cout, 64) * waste(batch, 256);
    const double c12 = 320.0 * waste(cout, 64) * waste(batch, 128);
    return (c22 <= c14 && c22 <= c12) ? 22 : (c14 <= c12 ? 14 : 12);
}

inline int tile_grid(int shape, const TileWork& w, TileGrid* t) {
    const int bn = shape == 22 ? 128 : 64, bm = shape == 14 ? 256 : 128;
    t->Ntiles = (int32_t)cdiv(w.cout, bn);
    const int64_t G = (int64_t)t->Ntiles * w.draws;
    if (G > 0x7fffffffLL) return BBB_ESHAPE;
    t->G = (int32_t)G;
    t->nbt = (int32_t)cdiv(w.batch, bm);
    const int64_t mt = mul_cap(w.pixels, t->nbt);
    if (mt > 0x7fffffffLL) return BBB_ESHAPE;
    t->Mtiles = (int32_t)mt;
    return conv_desc_check::xcd_grid(G * mt, &t->per_xcd, &t->blocks);
}

// A second k-group (its own stage, its own loads in flight, deterministic LDS reduction) when the launch cannot fill the chip with
// workgroups and the k loop is long: then per-tile latency, not LDS throughput, sets the pace.
// Wave specialisation pays when few workgroups are resident per CU (nothing else hides the staging phases); measured on AlexNet
// bs=512 E=10: conv3 31.7 -> 23.2 us, conv4 46.5 -> 33.3, conv5 18.2 -> 16.8, but conv1 / conv2 (1280+ workgroups, or the 64x256
// shape whose two stages leave one workgroup per CU) 20-30 % slower.  It replaces the second k-group.
inline TileChoice small_launch_rule(int shape, int t64, const TileWork& w) {
    const int64_t items = w.items(shape);
    const bool ws = shape == 22 && items <= 1024;
    return {shape, (!ws && items < 512 && t64 >= 8) ? 2 : 1, ws};
}

// The forward.  Few workgroups with long rows (a 1000 -> 10 classifier: ONE 64 x 256 tile per draw, 16 tiles of k; AlexNet's
// conv3-5 at one draw) are nothing but their serial k loops ("tiny"): take the two-wave 64 x 128 shape, whose small stage leaves
// room for FOUR k-groups per workgroup, each with its own stage and loads in flight (measured, profiles/r03_notes.md section 10:
// fc3 of 3Conv3FC 20.7 -> 16.5 us, fc2 15.7 -> 14.6, AlexNet one draw conv2 19.0 -> 15.6, conv4 20.3 -> 18.4, conv5 15.4 -> 14.2).
inline TileChoice fwd_tile_rule(int shape, int t64, const TileWork& w) {
    if (t64 >= 16 && w.items(12) < 256) return {12, 4, false};
    return small_launch_rule(shape, t64, w);
}

// The transposed form (the strided input gradient): the forward's rule with the k-tile count of the LONGEST contraction a pixel
// can have -- tap-major rows visit at most ceil(k / tstep) taps per axis (counting the full row would hand k-groups nothing),
// reference-order rows run over the full row -- and without the four-k-group form (launch_dgrad_shape, pconv_bf16.hip).
inline TileChoice dgrad_tile_rule(int shape, const bbb_conv_desc_t* d, bool tap_major, int tstep_h, int tstep_w, int64_t K,
                                  const TileWork& w) {
    const int64_t kmax = tap_major ? (int64_t)d->cin * ((d->kh + tstep_h - 1) / tstep_h) * ((d->kw + tstep_w - 1) / tstep_w) : K;
    return small_launch_rule(shape, (int)((kmax + BK - 1) / BK), w);
}

// LRT.  Two k-groups (each with its own stage and loads in flight, summed in group order) for layers that are few workgroups with
// long rows whatever the launch: at most 16 (pixel, 64-channel tile) groups and at least 16 tiles of 64 k.  A property of the
// LAYER's geometry, because the number of groups is the one launch choice that changes the summation order.  Wave specialisation
// (same bits as one group) as measured on the parent kernel, only with one group.
inline TileChoice lrt_tile_rule(int shape, int t64, const TileWork& w) {
    const int kgs = (t64 >= 16 && mul_cap(w.pixels, cdiv(w.cout, 64)) <= 16) ? 2 : 1;
    if (kgs == 2 && w.items(12) < 256) shape = 12;                // nothing but serial k loops: the small tile gives more of them
    return {shape, kgs, shape == 22 && kgs == 1 && w.items(shape) <= 1024};
}

// ---- bbb_conv2d_chwn_bf16_fwd ----
// the PConvArgs fields a form sets beyond the geometry (zero where the form leaves them alone)
struct LaunchFields { int32_t Ntiles, G, nbt, Mtiles, per_xcd, px_run, pool, y_c8, y_f32; };
struct FwdPlan {
    int form;                  // BBB_BF16_FORM_*
    Geom g;
    int64_t y_ds;              // elements per output slab (pooled forms: of the pooled map)
    LaunchFields f;
    int nt, ks;                // small-k forms: 32-channel tiles per workgroup (1 | 2), 16-k steps (2 | 5 | 8)
    TileChoice tile;           // general form (zero otherwise)
    int64_t blocks;
    int smem_bytes;            // window-resident form: its dynamic LDS
};

inline int xcd_blocks(int64_t items, FwdPlan* p) { return conv_desc_check::xcd_grid(items, &p->f.per_xcd, &p->blocks); }

// ptr_rc: what the entry's pointer-alignment check found (0 | BBB_EALIGN), returned at its place in the order of checks
inline int fwd_plan(const bbb_conv_desc_t* d, uint32_t flags, int ptr_rc, FwdPlan* p) {
    *p = FwdPlan{};
    const bool out_f32 = (flags & BBB_BF16_OUT_F32) != 0, tap_major = (flags & BBB_BF16_W_TAP_MAJOR) != 0;
    if (d == nullptr) return BBB_EINVAL;
    if (!positive_geometry(d) || d->act < 0 || d->act > 2) return BBB_EINVAL;
    if (const int rc = vector_rows(d, tap_major)) return rc;
    if ((flags & ~(BBB_BF16_OUT_F32 | BBB_BF16_W_TAP_MAJOR | BBB_BF16_X_C8 | BBB_BF16_OUT_C8)) != 0) return BBB_EINVAL;
    const bool x_c8 = (flags & BBB_BF16_X_C8) != 0, out_c8 = (flags & BBB_BF16_OUT_C8) != 0;
    int32_t ho = 0, wo = 0;
    if (const int rc = out_map(d, &ho, &wo)) return rc;
    if (const int rc = slab_limits(d, ho, wo, kFwdLimits, &p->g)) return rc;
    if (ptr_rc) return ptr_rc;
    if ((d->x_draw_stride & 7) != 0 || (d->w_draw_stride & 7) != 0) return BBB_EALIGN;
    const int64_t K = p->g.K, Kp = p->g.Kp;
    // (the checks from here to the end of the pooled form's admission all return BBB_EINVAL)
    if (conv_desc_check::unit_fields(d, conv_desc_check::kUnitsAndSteps) != 0 || d->w_row_pitch != 0 || d->w_tap_major != 0) return BBB_EINVAL;
    // pooling in the launch (bbb_conv_desc_t::pool): first layers with a short contraction only (pconv_bf16_smallk_pool_kernel);
    // 1 = MaxPool2d(2, 2), (k << 8) | s otherwise; admitted: 2 / 2 and 3 / 2 (at most one window closes per conv column)
    int pool_k = 0, pool_s = 0;
    if (d->pool != 0) {
        pool_k = d->pool == 1 ? 2 : (d->pool >> 8);
        pool_s = d->pool == 1 ? 2 : (d->pool & 255);
        if (!((pool_k == 2 && pool_s == 2) || (pool_k == 3 && pool_s == 2)) || ho < pool_k || wo < pool_k) return BBB_EINVAL;
        if (tap_major || out_f32 || Kp > 128) return BBB_EINVAL;
        if (x_c8 || (out_c8 && d->cout % 8 != 0)) return BBB_EINVAL;
    }
    LaunchFields& f = p->f;
    p->y_ds = (int64_t)d->cout * ho * wo * d->batch;
    // the small-k forms' tiles: weights in registers, 32 * nt channels x 256 images
    auto smallk_tiles = [&]() {
        p->nt = d->cout <= 32 ? 1 : 2;
        p->ks = Kp <= 32 ? 2 : (Kp <= 80 ? 5 : 8);
        f.Ntiles = (d->cout + 32 * p->nt - 1) / (32 * p->nt);
        f.nbt = (d->batch + 255) / 256;
        return (int64_t)f.Ntiles * d->draws;
    };
    if (pool_k != 0) {
        const int64_t G = smallk_tiles();
        if (G > 0x7fffffffLL) return BBB_ESHAPE;
        f.G = (int32_t)G;
        f.y_c8 = out_c8 ? 1 : 0;
        f.pool = (pool_k << 8) | pool_s;
        const int hp = (ho - pool_k) / pool_s + 1, wp = (wo - pool_k) / pool_s + 1;
        p->y_ds = (int64_t)d->cout * hp * wp * d->batch;
        // the window-resident form (pconv_bf16_smallk_poolwin_kernel): <= 32 channels, 128-image tiles, the widest strip whose input
        // window (+ one zero row) and epilogue staging fit 72 KB of LDS (two workgroups per CU).  Its workgroups are short (one
        // memory round trip for the window, 15 pixels, two pooled outputs: ~8 us each), so it wins where the strip form is a
        // latency chain -- small launches -- and loses once the strip form fills the chip (3Conv3FC conv1 + pool1, bs 256, us per
        // launch, window / strip / conv + pool launches: 1 step 15.8 / 38.8 / 18.4, 4 steps 34.8 / 52.8 / 46.5, 5-6 steps 45.8 / 44.2 /
        // 82, 16 steps 128 / 101 / 167; profiles/r05_notes.md section 3): below 70 pooled rows x image tiles
        if (p->nt == 1 && G * f.nbt * hp < 70) {
            const int64_t WRw = (int64_t)(pool_k - 1) * d->stride_h + (int64_t)(d->kh - 1) * d->dil_h + 1;
            auto window_rows = [&](int n) {          // image rows (channel x window row x window column) + the zero row of an n-pixel strip
                const int64_t cols = (int64_t)(n - 1) * pool_s + pool_k;
                const int64_t WCw = (cols - 1) * d->stride_w + (int64_t)(d->kw - 1) * d->dil_w + 1;
                return mul_cap(mul_cap(d->cin, WRw), WCw) + 1;
            };
            int best_n = 0;
            for (int n = 1; n <= wp; ++n) {
                const int64_t rows = window_rows(n);
                if (rows > kWinPasses * 16 || rows * (128 + 32) * 2 + 4 * 32 * 40 * 2 > 72 * 1024) break;   // (rows grow with n)
                best_n = n;
            }
            if (best_n >= 1) {
                const int nstr = (wp + best_n - 1) / best_n;
                const int wpc = (wp + nstr - 1) / nstr;               // what the kernel derives from nstr
                const int rows = (int)window_rows(wpc);
                f.Mtiles = rows;
                f.px_run = nstr;
                f.nbt = (d->batch + 127) / 128;
                p->smem_bytes = rows * (128 + 32) * 2 + 4 * 32 * 40 * 2;
                p->form = BBB_BF16_FORM_SMALLK_POOLWIN;
                return xcd_blocks(G * f.nbt * hp * nstr, p);
            }
        }
        // workgroups per pooled row.  A strip of n pooled pixels walks n * ps + pk - ps conv columns, so narrow strips compute
        // shared columns twice, wide strips leave the chip short of workgroups: take the split whose launch costs least in
        // (rounds of resident workgroups: 2 per CU at this kernel's register footprint) x (columns of its widest strip).
        // 3Conv3FC conv1, 16 steps per launch (240 pooled rows): 2 strips of 8 / 7 pooled pixels = 480 workgroups, one round, 17
        // columns (3 strips = 720 workgroups = two rounds of 11: measured 128 us against 1xx, profiles/r05_notes.md section 3)
        const int64_t rows = G * f.nbt * hp;
        const int64_t slots = 512;
        int csplit = 1;
        int64_t best = -1;
        const int max_split = wp >= 2 ? wp / 2 : 1;
        for (int c = 1; c <= max_split; ++c) {
            const int wpc = (wp + c - 1) / c;
            const int used = (wp + wpc - 1) / wpc;                // strips that actually hold pixels
            const int64_t rounds = (rows * used + slots - 1) / slots;
            const int64_t cost = rounds * ((int64_t)wpc * pool_s + pool_k - pool_s);
            if (best < 0 || cost < best) { best = cost; csplit = c; }
        }
        f.px_run = csplit;
        p->form = BBB_BF16_FORM_SMALLK_POOL;
        return xcd_blocks(rows * csplit, p);
    }
    if (x_c8) {
        // channel-interleaved input: the strip form that reads its MFMA operands straight from memory (pconv_bf16_strip8_kernel).
        // Tap-major rows of 32 input channels, 5 x 5 taps, stride 1, no dilation (3Conv3FC conv2); bf16 output in either layout.
        if (!(tap_major && !out_f32 && (!out_c8 || d->cout % 8 == 0) && d->cin == 32 && d->kh == 5 && d->kw == 5 && d->stride_h == 1 &&
              d->stride_w == 1 && d->dil_h == 1 && d->dil_w == 1 && d->pad_w < d->kw && d->pad_h < d->kh))
            return BBB_EINVAL;
        constexpr int P8 = 3;                                     // pixels per strip (launch_strip8's instantiation)
        f.y_c8 = out_c8 ? 1 : 0;
        f.Ntiles = (d->cout + 63) / 64;
        const int64_t G = (int64_t)f.Ntiles * d->draws;
        if (G > 0x7fffffffLL) return BBB_ESHAPE;
        f.G = (int32_t)G;
        f.nbt = (d->batch + 127) / 128;
        f.px_run = (wo + P8 - 1) / P8;
        p->form = BBB_BF16_FORM_STRIP8;
        return xcd_blocks(G * ho * f.px_run * f.nbt, p);
    }
    if (out_c8) return BBB_EINVAL;                    // only the pooled first-layer forms and the strip form write that layout
    if (!tap_major && !out_f32 && Kp <= 128 && (int64_t)ho * wo >= 16) {
        // a first layer with a short contraction: weights in registers, a run of pixels per workgroup (pconv_bf16_smallk_kernel)
        const int64_t G = smallk_tiles();
        if (G > 0x7fffffffLL) return BBB_ESHAPE;
        f.G = (int32_t)G;
        const int64_t npix = G * f.nbt * ho * wo;                 // (pixel, channel tile, image tile) units of the launch
        int run = (int)(npix / 512 > 16 ? 16 : npix / 512);       // >= 512 workgroups (2 per CU) before runs get longer
        run = run < 1 ? 1 : run;
        f.px_run = run;
        p->form = BBB_BF16_FORM_SMALLK;
        return xcd_blocks(G * f.nbt * (((int64_t)ho * wo + run - 1) / run), p);
    }
    if (d->cout <= 16 && K >= 512 && d->kh == 1 && d->kw == 1 && d->h == 1 && d->w == 1 && d->pad_h == 0 && d->pad_w == 0) {
        // a classifier with a handful of outputs and a long row: plain FMAs, k slices summed in a fixed order (pconv_bf16_fewout_kernel)
        const int kps = (int)(((Kp + 63) / 64 + 7) / 8) * 8;
        f.px_run = kps;
        f.G = (int)((Kp + kps - 1) / kps);                // slices that hold any k (<= 64)
        f.nbt = (d->batch + 31) / 32;
        f.y_f32 = out_f32 ? 1 : 0;
        p->blocks = (int64_t)d->draws * f.nbt;
        if (p->blocks > 0x7fffffffLL) return BBB_ESHAPE;
        p->form = BBB_BF16_FORM_FEWOUT;
        return 0;
    }
    const TileWork work = {d->cout, d->batch, d->draws, (int64_t)ho * wo};
    p->tile = fwd_tile_rule(tile_shape(d->cout, d->batch), (int)((K + BK - 1) / BK), work);
    TileGrid t = {};
    if (const int rc = tile_grid(p->tile.shape, work, &t)) return rc;
    f.Ntiles = t.Ntiles; f.G = t.G; f.nbt = t.nbt; f.Mtiles = t.Mtiles; f.per_xcd = t.per_xcd;
    p->blocks = t.blocks;
    p->form = BBB_BF16_FORM_GENERAL;
    return 0;
}

// ---- bbb_conv2d_chwn_bf16_dgrad ----
struct DgradPlan {
    Geom g;                    // (ho, wo) = the map of dx
    int tstep_h, tstep_w;      // step between the taps that take part (pconv_args.h, tr_axis)
    TileChoice tile;
    TileGrid grid;
};

// ptr_rc: what the entry's operand-pointer checks found (0 | BBB_EINVAL | BBB_EALIGN), returned at their place in the order of checks
inline int dgrad_plan(const bbb_conv_desc_t* d, int up_h, int up_w, int out_h, int out_w, uint32_t flags, int ptr_rc, DgradPlan* p) {
    *p = DgradPlan{};
    if (d == nullptr) return BBB_EINVAL;
    if (!positive_geometry(d) || up_h <= 0 || up_w <= 0 || out_h <= 0 || out_w <= 0) return BBB_EINVAL;
    // d describes the stride-1 launch on the flipped rows; the layer's stride travels as the upsampling factors
    if (d->stride_h != 1 || d->stride_w != 1) return BBB_EINVAL;
    if (up_h == 1 && up_w == 1) return BBB_EINVAL;          // a stride-1 layer's gradient is bbb_conv2d_chwn_bf16_fwd: one way to compute it
    if (d->act != 0 || d->pool != 0 || d->w_tap_major != 0 || d->w_row_pitch != 0 ||
        conv_desc_check::unit_fields(d, conv_desc_check::kNothing) != 0)
        return BBB_EINVAL;
    if (d->x_draw_stride < 0 || d->w_draw_stride < 0) return BBB_EINVAL;
    if ((flags & ~BBB_BF16_W_TAP_MAJOR) != 0) return BBB_EINVAL;
    const bool tap_major = (flags & BBB_BF16_W_TAP_MAJOR) != 0;
    if (const int rc = vector_rows(d, tap_major)) return rc;
    // (out_h, out_w) must be a map whose forward (padding p = d (k - 1) - q >= 0, stride up) gives exactly the g map of d
    const int64_t rh = (int64_t)d->dil_h * (d->kh - 1), rw = (int64_t)d->dil_w * (d->kw - 1);
    const int64_t fph = rh - d->pad_h, fpw = rw - d->pad_w;
    if (fph < 0 || fpw < 0) return BBB_ESHAPE;
    int32_t gh = 0, gw = 0;
    if (conv_desc_check::out_axis(out_h, fph, d->dil_h, d->kh, up_h, &gh) != 0 ||
        conv_desc_check::out_axis(out_w, fpw, d->dil_w, d->kw, up_w, &gw) != 0 || gh != d->h || gw != d->w)
        return BBB_ESHAPE;
    // per-draw slabs are addressed through 32-bit buffer offsets (as in the forward's checks)
    if (const int rc = slab_limits(d, out_h, out_w, kDgradLimits, &p->g)) return rc;
    if (ptr_rc) return ptr_rc;
    if ((d->x_draw_stride & 7) != 0 || (d->w_draw_stride & 7) != 0) return BBB_EALIGN;
    p->tstep_h = up_h / gcd_i(up_h, d->dil_h); p->tstep_w = up_w / gcd_i(up_w, d->dil_w);
    // never the small-k, few-output, strip or pooled kernels
    const TileWork work = {d->cout, d->batch, d->draws, (int64_t)out_h * out_w};
    p->tile = dgrad_tile_rule(tile_shape(d->cout, d->batch), d, tap_major, p->tstep_h, p->tstep_w, p->g.K, work);
    return tile_grid(p->tile.shape, work, &p->grid);
}

// ---- bbb_lrt_conv2d_chwn_bf16_fwd ----
// what bbb_lrt_conv2d_chwn_bf16_plan reports: the descriptor's geometry alone decides it (the entry's operand checks follow)
struct LrtPlan { int32_t ho, wo; TileWork work; TileChoice tile; };

inline int lrt_plan(const bbb_conv_desc_t* d, LrtPlan* p) {
    *p = LrtPlan{};
    if (d == nullptr || !positive_geometry(d)) return BBB_EINVAL;
    if (const int rc = out_map(d, &p->ho, &p->wo)) return rc;
    p->work = {d->cout, d->batch, d->draws, (int64_t)p->ho * p->wo};
    const int64_t t64 = cdiv(mul_cap(mul_cap(d->cin, d->kh), d->kw), BK);
    p->tile = lrt_tile_rule(tile_shape(d->cout, d->batch), (int)(t64 > 0x7fffffffLL ? 0x7fffffffLL : t64), p->work);
    return 0;
}

}  // namespace bf16_plan
