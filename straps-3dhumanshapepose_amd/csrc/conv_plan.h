// conv_plan.h -- the launch plan of a forward / data-gradient convolution: which kernel, which tile, its M tiles, partial blocks, grid and LDS.
// ONE function per route fills it from the problem's class structure (ConvShape), the tile_cfg and the operand mask of the launch (STRAPS_CONV_OP_*;
// conv_igemm.h reads both off a ConvP).  The dispatchers pick their instantiation by its fields, conv_launch copies NT / MT / partial bases / grid / LDS
// out of it, the block-count queries and straps_conv_plan return its fields; nothing else derives them.  tests/conv_cases.py restates it.  Plain C++.
#pragma once
#include "../../include/straps_hip.h"
#include "tool_env.h"

void straps_set_error(const char* fmt, ...);      // (abi.hip)

// compute units and LDS bytes per unit of the MI355X: constants, never read from the device -- the plan is a pure function of its inputs
constexpr int CONV_CUS = 256;
constexpr int CONV_LDS = 160 * 1024;

// what the rules read of a problem
struct ConvShape {
    int ncls, M[4], ntaps[4];      // classes (blockIdx.y), their output pixels and taps
    int cin, cout;                 // the GEMM's reduction channels per tap and its columns
    bool remap;                    // class 0 does not enumerate the output tensor in order (a parity class, a strided placement)
    int halo_slots;                // patch slots of a 128-row tile of the halo-patch kernel, 0 = the kernel does not cover the problem
};

struct ConvPlan {
    straps_conv_plan_t q;          // what straps_conv_plan shows
    int ns, trace;                 // fp32 route: operand staging (2 = LDS-DMA, 0 = registers: tile_cfg bit 4), the traced build (bit 5)
    int abl;                       // tools build only: ablation selector of the plane kernels (tile_cfg bits 6 / 7) or STRAPS_X3F_ABL; 0 in the product
};

// a tile of the plane kernels (conv_x3_kernels.h): block, wave grid, ring stages, software-pipelined loop; ps / pbuf: the halo-patch kernel's patch
// slots and buffers; pl: the bf16 route's K chunks per stage (0 = three planes per stage).  The dispatchers instantiate FROM these tables.
struct ConvTile { int bm, bn, wgm, wgn, nst; bool pipe; int ps, pbuf, pl; };
// tile_cfg & 15 of the plane route: 1 = 128x128 (8 waves, 3 stages), 2 = 128x64 (4 waves, 2 stages, two workgroups per CU), 3 = 64x64 (4 waves, 3 stages),
// 4 = 256x128 (8 waves, 2 stages), 5 = 128x128 (4 waves, 3 stages), 6 = alias of 4 (a four-wave 256x128 tile until round 5: it spilled registers
// and no rule ever chose it), 7 = 128x64 (4 waves, 3 stages; also what 13..15 run); software-pipelined loop (PIPE): 8 = as 5, 9 = as 1, 10 = as 7, 11 = as 2, 12 = as 4
constexpr ConvTile kX3Tile[13] = {{}, {128, 128, 4, 2, 3}, {128, 64, 2, 2, 2}, {64, 64, 2, 2, 3}, {256, 128, 4, 2, 2}, {128, 128, 2, 2, 3}, {}, {128, 64, 2, 2, 3},
                                  {128, 128, 2, 2, 3, true}, {128, 128, 4, 2, 3, true}, {128, 64, 2, 2, 3, true}, {128, 64, 2, 2, 2, true}, {256, 128, 4, 2, 2, true}};
// halo-patch forms: 1 = 128x128, two patch buffers, 2 = 128x64, two buffers (140 KB of LDS, one workgroup per CU), 3 = 128x64 with ONE patch buffer and a
// two-stage weight ring (76 KB, two workgroups per CU)
constexpr ConvTile kX3Halo[4] = {{}, {128, 128, 2, 2, 3, false, 208, 2}, {128, 64, 2, 2, 3, false, 272, 2}, {128, 64, 2, 2, 2, false, 272, 1}};
// tile_cfg of the bf16 route (0 = its rule).  All PL = 2 unless noted.
//   1 = 128x128 (4 waves, 3 stages)      2 = 128x64 (4 waves, 3 stages)      3 = 64x64 (4 waves, 3 stages)
//   4 = 256x128 (8 waves, 2 stages)      5 = 256x128 (8 waves, 2 stages, software-pipelined loop)
//   6 = 128x128 (4 waves, 2 stages, PL = 4: cin % 128 == 0)                7 = 128x128 (4 waves, 3 stages, software-pipelined loop)
//   8 = 128x64 (4 waves, 3 stages, PL = 1: one chunk per stage -- the bf16x3 loop with the planes deleted; A/B reference)
//   9 = halo patch 128x128 (3 stages, two patch buffers)                  10 = halo patch 128x64 (2 stages, one patch buffer)
constexpr int kBf16Cfgs = 10;
constexpr ConvTile kBf16Tile[kBf16Cfgs + 1] = {{}, {128, 128, 2, 2, 3, false, 0, 0, 2}, {128, 64, 2, 2, 3, false, 0, 0, 2}, {64, 64, 2, 2, 3, false, 0, 0, 2},
                                               {256, 128, 4, 2, 2, false, 0, 0, 2}, {256, 128, 4, 2, 2, true, 0, 0, 2}, {128, 128, 2, 2, 2, false, 0, 0, 4},
                                               {128, 128, 2, 2, 3, true, 0, 0, 2}, {128, 64, 2, 2, 3, false, 0, 0, 1}, {128, 128, 2, 2, 3, false, 208, 2, 2},
                                               {128, 64, 2, 2, 2, false, 272, 1, 2}};

// M tiles, partial bases, grid of a tile kernel: one grid row per class, as wide as the largest class; the partials of the classes one after the other
inline void conv_plan_fill(ConvPlan& pl, const ConvShape& s, int family, int tile, int bm, int bn, int epilogue, int threads, long long lds) {
    straps_conv_plan_t& q = pl.q;
    q.family = family; q.tile = tile; q.bm = bm; q.bn = bn; q.epilogue = epilogue; q.abn = 0;
    q.ncls = s.ncls; q.nt = s.cout / bn; q.blocks = 0; q.grid_x = 0;
    for (int i = 0; i < 4; ++i) {
        q.mt[i] = i < s.ncls ? (s.M[i] + bm - 1) / bm : 0;
        q.part_base[i] = q.blocks;
        q.blocks += q.mt[i];
        if (q.mt[i] * q.nt > q.grid_x) q.grid_x = q.mt[i] * q.nt;
    }
    q.grid_y = s.ncls; q.threads = threads; q.lds_bytes = (int)lds;
    pl.ns = pl.trace = pl.abl = 0;
}
inline void conv_plan_fill(ConvPlan& pl, const ConvShape& s, int family, int tile, const ConvTile& t, int epilogue) {
    const int slots = t.pl ? t.pl : 3;      // operand slots of a stage: three planes, or PL chunks of one; 32 bf16 per row
    conv_plan_fill(pl, s, family, tile, t.bm, t.bn, epilogue, 64 * t.wgm * t.wgn,
                   (long long)(t.ps ? t.pbuf * slots * t.ps + t.nst * slots * t.bn : t.nst * slots * (t.bm + t.bn)) * 32 * 2);
}

inline long long conv_shape_m(const ConvShape& s) {
    long long M = 0;
    for (int i = 0; i < s.ncls; ++i) M += s.M[i];
    return M;
}

// ---- fp32 implicit GEMM (conv.hip) --------------------------------------------------------------------------------------------------------
// tile choice from the per-layer sweeps (tools/sweep_conv.py, tools/sweep_igemm_staging.py, B=64): the larger the tile the fewer
// operand bytes per flop go through L2 -> LDS, but a size only pays while it still yields >= 2 workgroups per CU and the
// reduction is long enough (K >= 512 / 1024) to amortise its heavier prologue / epilogue: 128x128 first (layer2: 124 vs 111 TFLOP/s),
// then 128x64 (layer3: 122 vs 113; layer1's 64-channel 3x3 layers: 98 vs 90), otherwise 64x64 whose 5 resident workgroups per CU hide
// each other's barrier / refill bubbles (layer4's 4096 pixels, the 1x1 down-sampling layers' short K).
// All classes of one launch share the tile (chosen for their total size).  tile_cfg & 15: 0 = the rule, 1 = 128x128, 2 = 128x64, 3 = 64x64,
// 4 = 256x64; bit 4 = the register-staged operand path (A/B tools only; it has no 256-row tile: 64x64 then), bit 5 = the traced build
inline int conv_plan_f32(const ConvShape& s, int tile_cfg, ConvPlan& pl) {
    static constexpr int kBm[5] = {0, 128, 128, 64, 256}, kBn[5] = {0, 128, 64, 64, 64};
    const long long M = conv_shape_m(s);
    int kdim = 0;
    for (int i = 0; i < s.ncls; ++i)
        if (s.ntaps[i] * s.cin > kdim) kdim = s.ntaps[i] * s.cin;
    const long long mt128 = (M + 127) / 128;
    const int cout = s.cout;
    int tile = tile_cfg & 15;
    if (tile < 1 || tile > 4) {
        if (cout % 128 == 0 && kdim >= 512 && mt128 * (cout / 128) >= 512) tile = 1;      // (>= 256 would give layer3 128x128 tiles: +3.5 % in isolation, -0.3 % inside the step)
        else if (kdim >= 1024 && mt128 * (cout / 64) >= 512) tile = 2;
        else if (cout == 64 && kdim >= 512 && mt128 >= 1024) tile = 2;      // layer1: only 64 output channels but 262 144 rows (round 2: 98 vs 90 TFLOP/s forward, 98 vs 94 data gradient, step -0.6 %)
        else tile = 3;
    }
    if (tile == 1 && cout % 128 != 0) tile = 2;
    const int trace = (tile_cfg & 32) != 0, ns = (trace || !(tile_cfg & 16)) ? 2 : 0;
    if (ns == 0 && tile == 4) tile = 3;
    const int bm = kBm[tile], bn = kBn[tile];
    conv_plan_fill(pl, s, STRAPS_CONV_FAMILY_IGEMM_F32, tile, bm, bn, 0, 256,
                   ns ? (long long)ns * (bm + bn) * 32 * 4 : (long long)2 * (bm + bn) * 36 * 4);      // (register staging: rows padded to 36 floats, two buffers)
    pl.ns = ns; pl.trace = trace;
    return STRAPS_OK;
}

// ---- the lean epilogues (conv_igemm.h) -------------------------------------------------------------------------------------------------
// which epilogue an operand set takes: 1 = the lean forward form (raw result + statistics: a training step's forward; one class, no remap), 2 = the lean
// data-gradient form (addend with optional ReLU bits, BatchNorm sums with bits or the re-derived mask; any class structure), 0 = the shared epilogue
inline int lean_epilogue_choice(const ConvShape& s, unsigned ops) {
    if ((ops & (STRAPS_CONV_OP_YPLANES | STRAPS_CONV_OP_BNR_OUT | STRAPS_CONV_OP_SCALE | STRAPS_CONV_OP_RELU)) || !(ops & STRAPS_CONV_OP_Y)) return 0;
    const bool res = ops & STRAPS_CONV_OP_RES, bnr = ops & STRAPS_CONV_OP_BNR_RAW, bits = ops & STRAPS_CONV_OP_RES_BITS;
    if (!res && !bnr && !bits) return (s.ncls == 1 && !s.remap) ? 1 : 0;
    if (!(ops & STRAPS_CONV_OP_STATS) && (res || bnr) && (!bits || res)) {
        for (int i = 0; i < s.ncls; ++i)
            if (s.ntaps[i] == 0) return 0;      // (the dead parity classes of a 1x1 / stride-2 gradient: dx = addend there -- the shared epilogue's row form)
        return 2;
    }
    return 0;
}

// ---- bf16x3 plane kernels (conv_x3.hip, conv_x3_lean.hip) -------------------------------------------------------------------------------
// auto rule from tools/sweep_conv_x3.py (resnet18 shapes, B = 64): 64-channel outputs take 128x64 tiles, two workgroups per CU; otherwise
// the largest tile that still gives every CU a workgroup: 256x128 from 512 128x128-tiles on (layer2: 63 vs 68 us), 128x128 from 256
// (layer3: 97 vs 108), else 128x64 with the three-stage ring (layer4's 4096 pixels: 113 vs 150).
// Stride-2 data gradients (ncls = 4 output-parity classes, each a quarter of the pixels with 1-4 of the taps -- a 1x1 filter has ONE live
// class) are sized by the tiles of a class, not of the launch (round 3, tools/sweep_conv_x3.py on the resnet18 and resnet50 shapes):
// resnet50's 1024 -> 2048 shortcut 124 -> 54 us, 256 -> 256 3x3 77 -> 59, 512 -> 1024 shortcut 71 -> 59; resnet18's 128 -> 256 74 -> 58,
// 256 -> 512 75 -> 64.
inline int pick_tile_x3(int cfg, const ConvShape& s) {
    const int cout = s.cout, ncls = s.ncls;
    cfg &= 15;
    if (cfg == 6) cfg = 4;
    if (cfg == 0) {
        const long long t128 = ((conv_shape_m(s) + 127) / 128) * (cout / 128);
        int taps = 0;
        for (int i = 0; i < ncls; ++i) taps = s.ntaps[i] > taps ? s.ntaps[i] : taps;
        const bool one_tap = taps == 1;
        if (cout % 128 != 0) cfg = 11;
        // fewer than 128 128x128-tile equivalents per class: 128x64 tiles would leave half the CUs without a workgroup -- 64x64 (round 4, from the
        // COLD sweep tools/sweep_conv_x3_cold.py: resnet50's layer4 at 32 bodies, 2 048 pixels x 512 channels: 3x3 96 -> 74 us, 1x1 2048 -> 512
        // 55 -> 41 us; resnet18's 256 -> 512 stride-2 data gradient 80 -> 66 us)
        else if (t128 / ncls < STRAPS_TOOL_ENV_INT("STRAPS_X3_SMALL_T128", 128)) cfg = 3;      // (tools: the threshold of the 64x64 rule, for A/B runs)
        else if (ncls > 1) cfg = t128 / ncls >= 512 ? 12 : t128 / ncls >= 256 ? (one_tap ? 9 : 12) : 11;
        else cfg = t128 >= 512 ? 12 : t128 >= 256 ? 5 : 7;       // (11 / 12: the pipelined loop pays with two-stage rings: -7 %)
        // (tools: one configuration for every class the three size rules above decide -- A/B runs of the rule itself with the lean epilogues in place ...
        if (const int f = STRAPS_TOOL_ENV_INT("STRAPS_X3_RULE_CFG", 0); f > 0 && cout % 128 == 0 && t128 / ncls >= 128) cfg = f;
        // ... and for the smallest of the three buckets alone: 128 <= tiles < 256)
        if (const int lo = STRAPS_TOOL_ENV_INT("STRAPS_X3_LOW_CFG", 0); lo > 0 && ncls == 1 && cout % 128 == 0 && t128 >= 128 && t128 < 256) cfg = lo;
    }
    if (cout % 128 != 0 && cfg != 3 && cfg != 7 && cfg != 10 && cfg != 11) cfg = 2;
    return (cfg < 1 || cfg > 12 || cfg == 6) ? 7 : cfg;
}

// auto tile choice only (tile_cfg & 15 == 0; bit 8 = im2col kernel only, bit 9 = halo kernel wherever it applies: A/B tools; bit 10 = the
// single-patch-buffer halo kernel for 64-channel outputs, explicit only) -> form of kX3Halo, 0 = no.  Measured (tools/sweep_conv_x3.py, B = 64): halving the L2 -> LDS bytes
// buys only 4-5 % where the grid still fills the chip with 128x128 tiles (layer2: 104 vs 108 us -- 98 with the pipelined 256x128 tile,
// which is what layer2 uses --, layer3: 96 vs 101) and loses against the smaller / two-per-CU tiles of layer4 (157 vs 111) and, in
// its two-buffer form, of layer1 (154 vs 135).  With ONE patch buffer the 64-channel layers do gain: 123 vs 137 us -- that form is the rule for them.
inline int halo_choice(const ConvShape& s, int tile_cfg) {
    if ((tile_cfg & 15) != 0 || (tile_cfg & 256) || s.halo_slots <= 0) return 0;
    const bool all = (tile_cfg & 512) != 0, wide = s.cout % 128 == 0;
    const long long t128 = (long long)(s.M[0] / 128) * (s.cout / 128);
    if (!wide && s.halo_slots <= kX3Halo[3].ps && (!all || (tile_cfg & 1024))) return 3;
    if (wide && s.halo_slots <= kX3Halo[1].ps && (all || (t128 >= 256 && t128 < 512))) return 1;
    if (!wide && s.halo_slots <= kX3Halo[2].ps && all) return 2;
    return 0;
}

// The lean epilogues on the automatic tiles: a training step's forward -- raw result + statistics: +3.2 % / +2.8 % on the resnet18 / resnet50 step --
// and its data gradients (LeanDgradEpilogue: the same look-ahead as the shared epilogue -- two units' operands requested under the last chunk's matrix
// work -- with the lean arithmetic, per-value double sums in the shared epilogue's order: bit-identical results, +0.2 ... +1 % on the steps; without the
// look-ahead the lean form was a wash behind these kernels' long reductions: profiles/r06_lean_epilogue_ab.txt).  They exist on halo forms 1 and 3 and on
// the tiles the rule picks; tile_cfg bits 6 / 7 (ablation instantiations in the tools build, ignored by the product library) keep the shared epilogue.
inline int conv_plan_x3(const ConvShape& s, int tile_cfg, unsigned ops, ConvPlan& pl) {
    const int halo = halo_choice(s, tile_cfg);
    const int tile = halo ? halo : pick_tile_x3(tile_cfg, s);
    int epi = 0;
    if ((tile_cfg & 15) == 0 && !(tile_cfg & (64 | 128)) && STRAPS_TOOL_ENV_INT("STRAPS_X3_LEAN", 1)) {
        epi = lean_epilogue_choice(s, ops);
        if (epi == 2 && !STRAPS_TOOL_ENV_INT("STRAPS_X3_LEAN_DGRAD", 1)) epi = 0;      // (tools: A/B of the data-gradient form alone)
        if (halo ? halo == 2 : !(tile == 3 || tile == 5 || tile == 7 || tile == 9 || tile == 11 || tile == 12)) epi = 0;
    }
    conv_plan_fill(pl, s, halo ? STRAPS_CONV_FAMILY_PLANE_HALO : STRAPS_CONV_FAMILY_PLANE_IM2COL, tile, halo ? kX3Halo[halo] : kX3Tile[tile], epi);
#ifdef STRAPS_TOOLS
    if (!halo) pl.abl = (tile_cfg >> 6) & 3;      // (wrong results by design: tools/x3_ablate.py)
#endif
    return STRAPS_OK;
}

// ---- fp32-operand 1x1 route (conv_x3f.hip) ------------------------------------------------------------------------------------------------
// the lean forms serve the single-tap classes only; the tools build can switch them off for the A/B
inline int x3f_epilogue(const ConvShape& s, unsigned ops) {
    if (STRAPS_TOOL_ENV_INT("STRAPS_X3F_LEAN", 1) == 0 || s.ntaps[0] != 1) return 0;
    return lean_epilogue_choice(s, ops);
}
// width of the streaming kernel's output-channel tile, 0 = not eligible (several classes, a reduction extent that is not a multiple of 64, the
// shared epilogue).  256 wide with resident weights where all of K fits beside it (K = 64), else 128 / 64 wide with the weight ring.
inline int stream_bn(const ConvShape& s, int epi) {
    if (s.ncls != 1 || s.ntaps[0] != 1 || s.cin % 64 != 0 || epi == 0) return 0;
    if (s.cout % 256 == 0 && s.cin <= 64) return 256;
    return s.cout % 128 == 0 && s.cin < s.cout ? 128 : 64;
}
// tile_cfg & 15: 0 = auto, 1 = 128x64 (4 waves, 2 stages: 72 KB of LDS, two workgroups per CU), 2 = 64x64 (4 waves, 2 stages: 48 KB, three per CU),
// 5 = the streaming kernel (persistent workgroups, 128-row tiles -- 64-row with the resident 256-wide weight tile) where the problem is eligible, else as 0.
// The 1x1 layers this route exists for are byte-bound: what counts is that a CU always has a workgroup in its load phase beside one in its
// store phase, i.e. SEVERAL workgroups per CU, not a large tile (rule from tools/sweep_conv_x3f_cold.py, profiles/r06_x3f_cold_sweep.txt)
inline int conv_plan_x3f(const char* who, const ConvShape& s, int tile_cfg, unsigned ops, ConvPlan& pl) {
    const int epi = x3f_epilogue(s, ops), sbn = stream_bn(s, epi), cout = s.cout;
    const long long M = conv_shape_m(s);
    int cfg = tile_cfg & 15;
    // the streaming kernel: explicitly (5), or by rule for long problems -- at least four 128-row tiles per workgroup
    if (sbn && (cfg == 5 || (cfg == 0 && M >= 4 * 128 * (CONV_CUS / (cout / sbn))))) {
        const int bm = sbn == 256 ? 64 : 128, wgn = sbn == 64 ? 2 : 4, kc = sbn == 256 ? s.cin / 32 : 2;      // (256 wide: ALL of K resident; else a two-stage ring)
        // A image of two stages + the weights + the epilogue's cross-wave sums + the operand-path BatchNorm's scale | shift
        const long long lds = (long long)2 * 3 * bm * 32 * 2 + (long long)3 * kc * sbn * 32 * 2 + 2 * sbn * 4 * 4 + (long long)2 * s.cin * 4;
        if (lds > CONV_LDS) {
            straps_set_error("%s: conv1x1_stream_kernel: the operand images do not fit the LDS (cin=%d, BN=%d)", who, s.cin, sbn);
            return STRAPS_EINVAL;
        }
        conv_plan_fill(pl, s, STRAPS_CONV_FAMILY_F32OP_STREAM, 5, bm, sbn, epi, 64 * 2 * wgn, lds);
        // as many workgroups as stay resident (LDS decides), at most one per M tile; a multiple of the N tiles (a workgroup keeps ONE weight tile)
        const int per_cu = CONV_LDS / lds > 2 ? 2 : (int)(CONV_LDS / lds);
        int wgs = CONV_CUS * per_cu / pl.q.nt;
        if (const int f = STRAPS_TOOL_ENV_INT("STRAPS_X3F_STREAM_WGS", 0); f > 0) wgs = f;      // (tools: workgroups per N tile; a large number = one tile per workgroup, nothing persistent)
        if (wgs > pl.q.mt[0]) wgs = pl.q.mt[0];
        if (wgs < 1) wgs = 1;
        pl.q.grid_x = wgs * pl.q.nt;
    } else {
        if (cfg == 0 || cfg == 5) cfg = ((M / s.ncls + 127) / 128) * (cout / 64) < 512 ? 2 : 1;      // fewer than 512 128x64 tiles of a class: 64x64
        else if (cfg != 2) cfg = 1;
        const int bm = cfg == 2 ? 64 : 128;
        conv_plan_fill(pl, s, STRAPS_CONV_FAMILY_F32OP_TILE, cfg, bm, 64, epi, 256, (long long)2 * 3 * (bm + 64) * 32 * 2);
    }
    pl.q.abn = (ops & STRAPS_CONV_OP_A_SCALE) && epi != 2;
    pl.abl = STRAPS_TOOL_ENV_INT("STRAPS_X3F_ABL", 0);      // tools build: 1 no result stores, 2 no A loads (constants instead), 4 no MFMAs, 8 no statistics partials (wrong results)
    return STRAPS_OK;
}

// ---- single-product bf16 route (conv_bf16.hip) --------------------------------------------------------------------------------------------
// the automatic rule, from the MI355X sweep over the 33 resnet18 / resnet50 eval shapes at B = 1, 64, 256 (tools/sweep_conv_bf16.py,
// profiles/sweep_conv_bf16.json; t128 = 128x128-tile equivalents of the launch).  Summed over the shapes it is within 0.0 / 1.5 / 1.0 % of the
// per-shape best at B = 1 / 64 / 256 (the bf16x3 route: 1.57 / 2.22 / 2.44x the time):
//   * 64 output channels, or fewer than 256 tiles: 64x64 -- the grid must fill 256 CUs.  The halo-patch tiles lose here (layer1's 3x3 at
//     B = 64: 60 against 58 us) and everywhere else: with one plane the im2col ring's nine-fold reuse of the L2 is cheap enough.
//   * 256 ... 511 tiles: 128x128 / four waves (resnet50's 256-channel layers at B = 64: 27-42 us; the 256x128 tile leaves CUs idle, 34-53 us).
//   * from 512 tiles on: 256x128 / eight waves, software-pipelined (2-12 % ahead of the plain loop of the same tile on most shapes).
// A forced configuration the problem does not admit is refused, never silently replaced.
inline int conv_plan_bf16(const char* who, const ConvShape& s, int tile_cfg, ConvPlan& pl) {
    if (tile_cfg < 0 || tile_cfg > kBf16Cfgs) { straps_set_error("%s: tile_cfg must be in [0, %d] (got %d)", who, kBf16Cfgs, tile_cfg); return STRAPS_EINVAL; }
    if (s.M[0] <= 0) { straps_set_error("%s: empty output", who); return STRAPS_EINVAL; }
    int cfg = tile_cfg;
    if (cfg == 0) {
        const long long t128 = (((long long)s.M[0] + 127) / 128) * (s.cout / 128);
        cfg = (s.cout % 128 != 0 || t128 < 256) ? 3 : t128 < 512 ? 1 : 5;
    }
    const ConvTile& t = kBf16Tile[cfg];
    const char* why = nullptr;
    if (s.cout % t.bn != 0) why = "cout is not a multiple of the tile's N extent";
    else if (t.pl == 4 && s.cin % 128 != 0) why = "the four-chunk stage needs cin % 128 == 0";
    else if (t.ps && !(s.halo_slots > 0 && s.halo_slots <= t.ps))
        why = t.ps == 208 ? "the halo-patch tile needs a 3x3 / stride-1 layer whose patch fits 208 slots" : "the halo-patch tile needs a 3x3 / stride-1 layer whose patch fits 272 slots";
    if (why) { straps_set_error("%s: tile_cfg %d: %s", who, cfg, why); return STRAPS_EINVAL; }
    conv_plan_fill(pl, s, t.ps ? STRAPS_CONV_FAMILY_BF16_HALO : STRAPS_CONV_FAMILY_BF16_IM2COL, cfg, t, 3);
    return STRAPS_OK;
}

// ---- the geometries the entry points of a route accept (who: the entry point's name in the error text) ----------------------------------
#define CONV_PLAN_REQUIRE(cond, ...) do { if (!(cond)) { straps_set_error(__VA_ARGS__); return STRAPS_EINVAL; } } while (0)
inline int conv_geometry_check(const char* who, int route, int kind, int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad) {
    const bool one = route == STRAPS_CONV_ROUTE_F32_1X1 && !(kh == 1 && kw == 1 && pad == 0);      // single-tap geometry only: a 1x1 filter without padding
    if (kind == STRAPS_CONV_KIND_FWD) {
        CONV_PLAN_REQUIRE(batch > 0 && h > 0 && w > 0, "%s: empty input %dx%dx%d", who, batch, h, w);
        CONV_PLAN_REQUIRE(!one && (route != STRAPS_CONV_ROUTE_F32_1X1 || stride >= 1), "%s: 1x1 filters without padding only (kh=%d kw=%d pad=%d)", who, kh, kw, pad);
        if (route == STRAPS_CONV_ROUTE_BF16) CONV_PLAN_REQUIRE(cin % 64 == 0 && cout % 64 == 0, "%s: need cin%%64==0 and cout%%64==0 (cin=%d cout=%d)", who, cin, cout);
        CONV_PLAN_REQUIRE(cin % 32 == 0 && cout % 64 == 0, "%s: need cin%%32==0 and cout%%64==0 (cin=%d cout=%d)", who, cin, cout);
        CONV_PLAN_REQUIRE(kh >= 1 && kw >= 1 && kh * kw <= 9 && stride >= 1 && pad >= 0, "%s: bad filter geometry", who);
    } else {
        CONV_PLAN_REQUIRE(kind == STRAPS_CONV_KIND_DGRAD && route != STRAPS_CONV_ROUTE_BF16, "%s: the bf16 route is forward only; kind is 0 (forward) or 1 (data gradient)", who);
        CONV_PLAN_REQUIRE(!one && (route != STRAPS_CONV_ROUTE_F32_1X1 || stride == 1 || stride == 2), "%s: 1x1 filters without padding, stride 1 or 2 only", who);
        CONV_PLAN_REQUIRE(cout % 32 == 0 && cin % 64 == 0, "%s: need cout%%32==0 and cin%%64==0 (cin=%d cout=%d)", who, cin, cout);
        CONV_PLAN_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2", who);
        CONV_PLAN_REQUIRE(kh * kw <= 9 && kh - 1 - pad >= 0 && kw - 1 - pad >= 0, "%s: unsupported filter geometry", who);
    }
    return STRAPS_OK;
}

inline int conv_plan_route(const char* who, int route, const ConvShape& s, int tile_cfg, unsigned ops, ConvPlan& pl) {
    switch (route) {
        case STRAPS_CONV_ROUTE_F32: return conv_plan_f32(s, tile_cfg, pl);
        case STRAPS_CONV_ROUTE_PLANES: return conv_plan_x3(s, tile_cfg, ops, pl);
        case STRAPS_CONV_ROUTE_F32_1X1: return conv_plan_x3f(who, s, tile_cfg, ops, pl);
        case STRAPS_CONV_ROUTE_BF16: return conv_plan_bf16(who, s, tile_cfg, pl);
        default: straps_set_error("%s: unknown route %d", who, route); return STRAPS_EINVAL;
    }
}
