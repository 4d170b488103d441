// conv_wgrad.hip -- weight gradients of the encoder's 3x3 / 1x1 convolutions (part of what autograd + cuDNN do for the reference's loss.backward(),
// train/train_synthetic_otf_rendering.py:232): the plan of a call (conv_wgrad_plan.h; ONE function of the geometry and the operand form, below), the
// kernels (conv_wgrad_kernels.h) and the entry points, which fill kernel parameters from the plan and launch through one switch.  The fp32-operand 1x1
// kernel and its entry point are in conv_wgrad_x3f.hip; they take their plan and their reduction from here.
#include "conv_wgrad_kernels.h"

namespace {

constexpr int F_TAP_F32 = STRAPS_WG_FAMILY_TAP_F32, F_HALO_F32 = STRAPS_WG_FAMILY_HALO_F32, F_TAP_X3 = STRAPS_WG_FAMILY_TAP_X3,
              F_HALO_X3 = STRAPS_WG_FAMILY_HALO_X3, F_TAP_X3F = STRAPS_WG_FAMILY_TAP_X3F;
constexpr int HALO_NG = 2;      // 4-wave groups per workgroup of both halo kernels

// split count: `target` workgroups per launch over the tiles, at most max_s, at least one
inline int splits_for(int target, int tiles, long long max_s) {
    long long s = (target + tiles - 1) / tiles;
    if (s > max_s) s = max_s;
    return s < 1 ? 1 : (int)s;
}

// plan of a halo-patch kernel with cp-pixel chunks (32; the bf16x3 kernel also 64); false, and *pl untouched, when the layer must use a per-tap kernel
bool halo_plan(int family, int cp, int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, WgradPlan* pl) {
    if (!(kh == 3 && kw == 3 && stride == 1 && pad == 1)) return false;
    if (w < 8 || (w & (w - 1)) != 0) return false;              // chunk columns must tile the row exactly
    const int cw = w < 32 ? w : 32, rpc = cp / cw;
    if (h % rpc != 0) return false;
    int lg = 0;
    while ((1 << lg) < cw) ++lg;
    WgradHaloGeom& g = pl->halo;
    g = {h, w, cin, cout, cw, lg, rpc, w / cw, h / rpc, batch * (h / rpc) * (w / cw), 0, cin / 64};
    const int tiles = (cout / 64) * (cin / 64);
    // one 8-wave workgroup per CU (two 4-wave groups that share one partial); at least 4 chunks (576 MFMAs per wave) per workgroup
    const int s = splits_for(WGRAD_CUS, tiles, (g.nchunks + 3) / 4);
    g.chunks_per_split = (g.nchunks + s - 1) / s;
    // two stages: fp32 rows per group | three bf16 planes of the dy tile and the patch slots (128 / 136), shared by the groups
    const int lds = family == F_HALO_F32 ? HALO_NG * 2 * W3PX * 64 * 4 : 2 * 3 * (cp + (cp == 32 ? 128 : 136)) * 64 * 2;
    pl->q = {family, 64, 64, cp, tiles, (g.nchunks + g.chunks_per_split - 1) / g.chunks_per_split, g.chunks_per_split, g.nchunks, 9, lds, 0};
    return true;
}

// two LDS stages of 32 pixels: fp32 rows | three bf16 planes
inline int tap_lds(int family, int bco, int bci) { return 2 * 32 * (bco + bci) * (family == F_TAP_F32 ? 4 : 3 * 2); }

// plan of a per-tap family (pl->tap holds the layer) with channel block bco x bci: splits for `target` workgroups, whole 32-pixel steps per split
void tap_plan(int family, int bco, int bci, int target, long long max_s, WgradPlan* pl) {
    WgradTapGeom& g = pl->tap;
    g.ct = g.Cout / bco; g.it = g.Cin / bci;
    const int taps = g.R * g.S, tiles = taps * g.ct * g.it, splits = splits_for(target, tiles, max_s);
    g.rows_per_split = (int)((((long long)g.M + splits - 1) / splits + 31) / 32 * 32);
    pl->q = {family, bco, bci, 0, tiles, splits, g.rows_per_split, g.M, taps, tap_lds(family, bco, bci), 0};
}

// 128x128 tiles (32 flop per operand byte instead of 16) for the big 1x1 layers (resnet50): +10 % there; the 3x3 / strided layers
// and small pixel counts do better with 64x64 (more workgroups per tap)
inline bool wgrad_big_tile(const WgradTapGeom& g) { return g.Cin % 128 == 0 && g.Cout % 128 == 0 && g.R * g.S == 1 && g.M >= 8192; }

// the fp32 per-tap plan: square blocks; 128 (64 KB of LDS, two workgroups resident per CU) runs 2 workgroups per CU, 64 runs 6; at least 4 K-steps of
// 32 pixels per split.  Its partials are the advertised workspace size, which every plan on the planes must fit.
void tap_f32_plan(WgradPlan* pl) {
    const bool big = wgrad_big_tile(pl->tap);
    tap_plan(F_TAP_F32, big ? 128 : 64, big ? 128 : 64, (big ? 2 : 6) * WGRAD_CUS, ((long long)pl->tap.M + 127) / 128, pl);
}

// channel block (BCO x BCI) of the per-tap kernel on the planes: square by default (128 x 128 where wgrad_big_tile, else 64 x 64), RECTANGULAR (round 4)
// where that cuts the operand stream.  Every operand is re-read once per block of the OTHER channel dimension (bytes per pixel = 6 (Cout Cin / BCI +
// Cin Cout / BCO)), every block costs split-K partials, and a block's LDS decides how many workgroups a CU holds: measured cold (operands from HBM, as
// inside a step) over the resnet50 / resnet18 layers by tools/sweep_wgrad_tiles.py (profiles/r04_wgrad_tile_sweep.txt), the rectangular blocks beat
// the square ones of round 3 by 8-20 % where the rule below picks them:
//   1x1, >= 32 768 pixels, Cout % 256 == 0           256 x 128   (l2 shortcut 256>512: 140 -> 112 us, l3.0 512>256: 114 -> 96)
//   1x1, <= 8 192 pixels                             64 x 128 when Cout > Cin at stride 1, else 128 x 64   (l4 2048>512: 52 -> 43, l4 shortcut: 94 -> 77)
//   3x3 / stride 2                                   256 x 128 where the channels allow, else 128 x 64   (l4: 113 -> 104, r18 l4.0: 115 -> 106)
void tap_x3_block(const WgradTapGeom& g, int* bco, int* bci) {
    const int cin = g.Cin, cout = g.Cout;
    *bco = *bci = wgrad_big_tile(g) ? 128 : 64;
    if (g.R * g.S == 1) {
        if (g.M >= 32768 && cout % 256 == 0 && cin % 128 == 0) { *bco = 256; *bci = 128; }
        else if (g.M <= 8192 && cout % 128 == 0 && cin % 128 == 0) {
            if (g.stride == 1 && cout > cin) { *bco = 64; *bci = 128; }
            else { *bco = 128; *bci = 64; }
        }
    } else if (cout % 256 == 0 && cin % 128 == 0) { *bco = 256; *bci = 128; }
    else if (cout % 128 == 0 && cin % 64 == 0) { *bco = 128; *bci = 64; }
}

// the per-tap plan on the planes for a given block.  Square: the 128x128 tile takes 96 KB of LDS, one workgroup per CU is resident, so 256 workgroups =
// one round; 512 cost 10-18 % on resnet50's 1x1 layers -- tools/sweep_wgrad_x3.py, round 3 (the fp32 kernel, 64 KB, two resident, keeps 512).
// Rectangular: as many workgroups as the block's LDS lets a CU hold, and never more splits than the fp32 plan -- the `cap`: the workspace both routes
// share is sized by the fp32 plan (the square targets are at most the fp32 plan's; 256 x 128 under a 3x3 filter is the block that reaches the cap).
void tap_x3_plan(int bco, int bci, WgradPlan* pl) {
    const long long max_s = ((long long)pl->tap.M + 127) / 128;
    if (bco == bci) {
        tap_plan(F_TAP_X3, bco, bci, (bco == 128 ? 1 : 6) * WGRAD_CUS, max_s, pl);
        return;
    }
    WgradPlan f32 = *pl;
    tap_f32_plan(&f32);
    const int per_cu = (160 * 1024) / tap_lds(F_TAP_X3, bco, bci);
    tap_plan(F_TAP_X3, bco, bci, WGRAD_CUS * (per_cu < 1 ? 1 : per_cu), max_s < f32.q.splits ? max_s : f32.q.splits, pl);
}

// channel block of the fp32-operand 1x1 kernel (conv_wgrad_x3f.hip): the smaller channel dimension whole where it fits beside 256 of the other (every
// element read once), else 256 x 128 / 128 x 256 (the wide operand once, the narrow one twice), 64 x 64 for the 64 <-> 64 layer
void tap_x3f_block(int cin, int cout, int* bco, int* bci) {
    if (cout % 256 == 0 && cin == 64) { *bco = 256; *bci = 64; }
    else if (cin % 256 == 0 && cout == 64) { *bco = 64; *bci = 256; }
    else if (cout % 256 == 0 && cin % 128 == 0 && cout >= cin) { *bco = 256; *bci = 128; }
    else if (cin % 256 == 0 && cout % 128 == 0) { *bco = 128; *bci = 256; }
    else if (cout % 128 == 0 && cin % 128 == 0) { *bco = 128; *bci = 128; }
    else { *bco = 64; *bci = 64; }
}

inline bool reads_planes(const WgradPlan& pl) { return pl.q.family == F_TAP_X3 || pl.q.family == F_HALO_X3; }

}  // namespace

int straps_internal_wgrad_plan(const char* who, int form, int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, WgradPlan* pl) {
    *pl = WgradPlan{};
    const bool planes = form == STRAPS_WG_ROUTE_PLANES, x3f = form == STRAPS_WG_ROUTE_F32_1X1;
    STRAPS_REQUIRE(cin % 64 == 0 && cout % 64 == 0, "%s: need cin%%64==0 and cout%%64==0 (cin=%d cout=%d)", who, cin, cout);
    STRAPS_REQUIRE(!x3f || (kh == 1 && kw == 1 && pad == 0 && stride >= 1), "%s: 1x1 filters without padding only", who);
    WgradTapGeom& g = pl->tap;
    g = {batch, h, w, cin, cout, kh, kw, stride, pad, (h + 2 * pad - kh) / stride + 1, (w + 2 * pad - kw) / stride + 1};
    if (!x3f && halo_plan(planes ? F_HALO_X3 : F_HALO_F32, 32, batch, h, w, cin, cout, kh, kw, stride, pad, pl)) {
        // on the planes: 64-pixel chunks where the rows allow it.  Half the chunks never need more splits than the 32-pixel plan, whose count (the fp32
        // halo kernel's) sizes the shared workspace; the condition states it.
        WgradPlan p64 = *pl;
        if (planes && halo_plan(F_HALO_X3, 64, batch, h, w, cin, cout, kh, kw, stride, pad, &p64) && p64.q.splits <= pl->q.splits) *pl = p64;
    } else {
        const long long M = (long long)batch * g.Ho * g.Wo;
        STRAPS_REQUIRE(M < (1LL << 31) && (!x3f || M > 0), "%s: problem too large (or empty)", who);
        g.M = (int)M;
        int bco, bci;
        if (x3f) {
            // one eight-wave workgroup per CU (two four-wave ones of the 64 x 64 block); at least two steps per split
            tap_x3f_block(cin, cout, &bco, &bci);
            tap_plan(F_TAP_X3F, bco, bci, (bco == 64 && bci == 64 ? 2 : 1) * WGRAD_CUS, (M + 63) / 64, pl);
        } else if (planes && (kh * kw > 1 || (cin >= 128 && cout >= 128))) {
            // per-tap kernel on the planes where it beats the fp32 one (tools/sweep_wgrad_x3.py: 3x3 / stride 2: 87-93 vs 115-125 us; 1x1 with at least
            // 128 channels on both sides: +0..29 %; with a 64-channel side the fp32 kernel's 4-byte rows win: 52 vs 60 us).  Both stream their operands
            // from memory once per tile of the other channel dimension: bytes, not the matrix pipe, set their rate.
            tap_x3_block(g, &bco, &bci);
            tap_x3_plan(bco, bci, pl);
        } else {
            tap_f32_plan(pl);
        }
    }
#ifdef STRAPS_TOOLS      // measurement overrides of the tools build
    if (pl->q.family == F_TAP_X3) {
        // tools/sweep_wgrad_tiles.py: STRAPS_WGRAD_TILE = 1000 * BCO + BCI, read at every call; a block the layer cannot take gives the square default
        if (const int v = STRAPS_TOOL_ENV_INT("STRAPS_WGRAD_TILE", 0)) {
            const int o = v / 1000, i = v % 1000, sq = wgrad_big_tile(pl->tap) ? 128 : 64;
            const bool ok = (o == 64 || o == 128 || o == 256) && (i == 64 || i == 128 || i == 256) && !(o == 256 && i == 256) && cout % o == 0 && cin % i == 0 &&
                            !(o == 128 && i == 128 && sq != 128);
            tap_x3_plan(ok ? o : sq, ok ? i : sq, pl);
        }
    }
    static const int abl = STRAPS_TOOL_ENV_INT("STRAPS_WGRAD3_ABL", 0);      // (tools/wgrad3_ablate.py; ablations compute wrong results)
    if (pl->q.family == F_HALO_X3 && pl->q.chunk_px == 64) pl->abl = abl;
#endif
    pl->q.part_bytes = (int64_t)pl->q.splits * cout * pl->q.taps * cin * (int64_t)sizeof(float);
    return STRAPS_OK;
}

// ------------------------------------------------------------------------------------------ C ABI
// (library-internal, not part of the C ABI: conv_wgrad_x3f.hip reduces its split-K partials with the same fixed-order kernel)
int straps_internal_wgrad_reduce(const float* part, float* dw_oihw, int splits, int cout, int cin, int taps, int accumulate, hipStream_t st) {
    const long long n = (long long)cout * taps * cin;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(n / 256)), dim3(256), 0, st, part, dw_oihw, splits, cout, cin, taps, accumulate);
    STRAPS_CHECK_LAUNCH("wgrad_reduce_kernel");
    return STRAPS_OK;
}

extern "C" int straps_conv_wgrad_plan(int route, int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, straps_wgrad_plan_t* out) {
    STRAPS_REQUIRE(out && route >= STRAPS_WG_ROUTE_F32 && route <= STRAPS_WG_ROUTE_F32_1X1, "straps_conv_wgrad_plan: null pointer or unknown route %d", route);
    WgradPlan pl;
    const int rc = straps_internal_wgrad_plan("straps_conv_wgrad_plan", route, batch, h, w, cin, cout, kh, kw, stride, pad, &pl);
    if (rc == STRAPS_OK) *out = pl.q;
    return rc;
}

extern "C" size_t straps_conv_wgrad_workspace_bytes(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad) {
    WgradPlan pl;
    const int rc = straps_internal_wgrad_plan("straps_conv_wgrad_workspace_bytes", STRAPS_WG_ROUTE_F32, batch, h, w, cin, cout, kh, kw, stride, pad, &pl);
    return rc == STRAPS_OK ? (size_t)pl.q.part_bytes : 0;
}

extern "C" int straps_conv_wgrad_x3_on_planes(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad) {
    WgradPlan pl;
    return straps_internal_wgrad_plan("straps_conv_wgrad_x3_on_planes", STRAPS_WG_ROUTE_PLANES, batch, h, w, cin, cout, kh, kw, stride, pad, &pl) == STRAPS_OK && reads_planes(pl);
}

namespace {

// the one launch switch: (family, chunk pixels, block) -> kernel instantiation; then the fixed-order reduce of the partials into dW
constexpr int wkey(int family, int chunk_px, int bco, int bci) { return (family << 24) | (chunk_px << 18) | (bco << 9) | bci; }

int wgrad_launch(const WgradPlan& pl, const float* x, const float* dy, const u16* x3, long long xps, const u16* dy3, long long dps, float* dw_oihw,
                 void* workspace, int accumulate, void* stream) {
    const straps_wgrad_plan_t& q = pl.q;
    float* part = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(q.tiles, q.splits);
    const size_t lds = (size_t)q.lds_bytes;
    WgradP tf{x, dy, part, pl.tap};
    Wgrad3P hf{x, dy, part, pl.halo};
    WgradXP tx{x3, dy3, xps, dps, part, pl.tap};
    Wgrad3XP hx{x3, dy3, xps, dps, part, pl.halo, (long long)pl.tap.B * pl.tap.H * pl.tap.W};
#define WGRAD_LAUNCH(KERN, THREADS, P)                                       \
    do {                                                                     \
        if (lds >= 64 * 1024) STRAPS_RAISE_LDS((KERN), lds, #KERN);          \
        hipLaunchKernelGGL((KERN), grid, dim3(THREADS), lds, st, P);         \
        STRAPS_CHECK_LAUNCH(#KERN);                                          \
    } while (0)
    switch (wkey(q.family, q.chunk_px, q.bco, q.bci)) {
    case wkey(F_TAP_F32, 0, 64, 64): WGRAD_LAUNCH((conv_wgrad_kernel<64, 64>), 256, tf); break;
    case wkey(F_TAP_F32, 0, 128, 128): WGRAD_LAUNCH((conv_wgrad_kernel<128, 128>), 256, tf); break;
    case wkey(F_HALO_F32, 32, 64, 64): WGRAD_LAUNCH((conv_wgrad3x3_kernel<HALO_NG>), 256 * HALO_NG, hf); break;
    case wkey(F_HALO_X3, 32, 64, 64): WGRAD_LAUNCH((conv_wgrad3x3_x3_kernel<HALO_NG, 32>), 256 * HALO_NG, hx); break;
    case wkey(F_HALO_X3, 64, 64, 64):
#ifdef STRAPS_TOOLS
        if (pl.abl) {      // the ablated kernel alone, without its reduce: that is what tools/wgrad3_ablate.py times
            auto kern = pl.abl == 1 ? conv_wgrad3x3_x3_kernel<HALO_NG, 64, 1> : pl.abl == 2 ? conv_wgrad3x3_x3_kernel<HALO_NG, 64, 2>
                      : pl.abl == 3 ? conv_wgrad3x3_x3_kernel<HALO_NG, 64, 3> : pl.abl == 4 ? conv_wgrad3x3_x3_kernel<HALO_NG, 64, 4> : conv_wgrad3x3_x3_kernel<HALO_NG, 64, 5>;
            (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, grid, dim3(256 * HALO_NG), lds, st, hx);
            STRAPS_CHECK_LAUNCH("conv_wgrad3x3_x3_kernel (ablation)");
            return STRAPS_OK;
        }
#endif
        WGRAD_LAUNCH((conv_wgrad3x3_x3_kernel<HALO_NG, 64>), 256 * HALO_NG, hx);
        break;
    case wkey(F_TAP_X3, 0, 64, 64): WGRAD_LAUNCH((conv_wgrad_x3_kernel<64, 64>), 256, tx); break;
    case wkey(F_TAP_X3, 0, 128, 128): WGRAD_LAUNCH((conv_wgrad_x3_kernel<128, 128>), 256, tx); break;
    case wkey(F_TAP_X3, 0, 256, 128): WGRAD_LAUNCH((conv_wgrad_x3_kernel<256, 128>), 256, tx); break;
    case wkey(F_TAP_X3, 0, 128, 64): WGRAD_LAUNCH((conv_wgrad_x3_kernel<128, 64>), 256, tx); break;
    case wkey(F_TAP_X3, 0, 64, 128): WGRAD_LAUNCH((conv_wgrad_x3_kernel<64, 128>), 256, tx); break;
#ifdef STRAPS_TOOLS      // blocks only the tile switch of the tools build can select
    case wkey(F_TAP_X3, 0, 256, 64): WGRAD_LAUNCH((conv_wgrad_x3_kernel<256, 64>), 256, tx); break;
    case wkey(F_TAP_X3, 0, 64, 256): WGRAD_LAUNCH((conv_wgrad_x3_kernel<64, 256>), 256, tx); break;
    case wkey(F_TAP_X3, 0, 128, 256): WGRAD_LAUNCH((conv_wgrad_x3_kernel<128, 256>), 256, tx); break;
#endif
    default: STRAPS_REQUIRE(false, "conv weight gradient: no kernel for family %d, block %d x %d", q.family, q.bco, q.bci);
    }
#undef WGRAD_LAUNCH
    return straps_internal_wgrad_reduce(part, dw_oihw, q.splits, pl.tap.Cout, pl.tap.Cin, q.taps, accumulate, st);
}

}  // namespace

// weight gradient on the bf16x3 route: with planes (x3, dy3: [3][plane stride] bf16, see straps_split3_bf16) the plan picks the halo-patch or the per-tap
// kernel on them, or -- like a call without planes -- the fp32 kernels of straps_conv_wgrad on (x, dy)
extern "C" int straps_conv_wgrad_x3(const float* x, const float* dy, const unsigned short* x3, long long x_plane_stride, const unsigned short* dy3,
                                    long long dy_plane_stride, float* dw_oihw, void* workspace, int batch, int h, int w, int cin, int cout, int kh,
                                    int kw, int stride, int pad, int accumulate, void* stream) {
    STRAPS_REQUIRE(dw_oihw && workspace, "straps_conv_wgrad_x3: null pointer");
    WgradPlan pl;
    const int rc = straps_internal_wgrad_plan("straps_conv_wgrad_x3", (x3 && dy3) ? STRAPS_WG_ROUTE_PLANES : STRAPS_WG_ROUTE_F32, batch, h, w, cin, cout, kh, kw, stride, pad, &pl);
    if (rc != STRAPS_OK) return rc;
    if (reads_planes(pl)) {
        STRAPS_REQUIRE(x_plane_stride % 8 == 0 && dy_plane_stride % 8 == 0, "straps_conv_wgrad_x3: plane strides must be multiples of 8 elements");
        // the workspace contract: callers size the workspace with straps_conv_wgrad_workspace_bytes (the fp32 plan), whatever this plan writes must fit
        const size_t adv = straps_conv_wgrad_workspace_bytes(batch, h, w, cin, cout, kh, kw, stride, pad);
        STRAPS_REQUIRE((size_t)pl.q.part_bytes <= adv, "straps_conv_wgrad_x3: the plan's partials (%lld bytes) exceed the advertised workspace (%zu)", (long long)pl.q.part_bytes, adv);
    } else {
        STRAPS_REQUIRE(x && dy, "straps_conv_wgrad_x3: this shape runs on the fp32 tensors, which are NULL (see straps_conv_wgrad_x3_on_planes)");
    }
    return wgrad_launch(pl, x, dy, x3, x_plane_stride, dy3, dy_plane_stride, dw_oihw, workspace, accumulate, stream);
}

extern "C" int straps_conv_wgrad(const float* x, const float* dy, float* dw_oihw, void* workspace, int batch, int h, int w, int cin,
                                 int cout, int kh, int kw, int stride, int pad, int accumulate, void* stream) {
    STRAPS_REQUIRE(x && dy && dw_oihw && workspace, "straps_conv_wgrad: null pointer");
    return straps_conv_wgrad_x3(x, dy, nullptr, 0, nullptr, 0, dw_oihw, workspace, batch, h, w, cin, cout, kh, kw, stride, pad, accumulate, stream);
}
