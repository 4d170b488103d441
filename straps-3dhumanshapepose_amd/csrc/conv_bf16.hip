// conv_bf16.hip -- the single-product bf16 route of the 3x3 / 1x1 convolutions: eval-mode forward only (inference).
//
//   Every fp32 operand value is rounded to the nearest-even bf16 (the leading plane b1 of common.h's split3) and a term a*b is ONE
//   v_mfma_f32_32x32x16_bf16 product of the two roundings, exact in the fp32 accumulator.  Against the bf16x3 route (conv_x3.hip: three
//   planes, six products per term) this is 1/6 of the matrix work and 1/3 of the operand bytes; the price is the rounding of both operands
//   (relative 2^-9 each), i.e. the accuracy of a bf16 network, not of an fp32 one ("Single-product bf16 inference").
//
//   Layouts: the activation is ONE chunk-major bf16 plane (common.h cm_index: 64 bytes per pixel x 32-channel chunk -- plane 0 of the bf16x3
//   route's tensors), the weights one chunk-major plane in the forward layout (elementwise.hip wk_index).  The kernels are those of
//   conv_x3_kernels.h instantiated with PL = 2 (or 4): the stage slots that held the three planes of one K chunk hold PL consecutive K chunks of
//   the one plane -- the plane strides handed to the kernels are the chunk strides -- so that a barrier, a copy wait and the LDS-DMA issue cover
//   PL chunks of matrix work.  With one product per term a chunk of 32 channels is only 2 x MI x NI MFMAs against (BM + BN) / RPP copies: a
//   loop tuned for six products per fragment becomes bound by copy issue and barriers (MI355X_MICROARCH.md: ~60 cycles per LDS-DMA piece among
//   MFMAs).  Epilogue: the shared EPI = 0 one of conv_igemm.h (folded BatchNorm, fp32 residual, ReLU) writing the optional fp32 output and the
//   result as ONE bf16 plane (rn_bf16 of the fp32 value) for the next convolution (X3Epilogue<..., 3>).
#include "conv_x3_kernels.h"

namespace {

// tile_cfg & 15 (tools; 0 = the automatic rule below).  All PL = 2 unless noted.
//   1 = 128x128 (4 waves, 3 stages)      2 = 128x64 (4 waves, 3 stages)      3 = 64x64 (4 waves, 3 stages)
//   4 = 256x128 (8 waves, 2 stages)      5 = 256x128 (8 waves, 2 stages, software-pipelined loop)
//   6 = 128x128 (4 waves, 2 stages, PL = 4: cin % 128 == 0)                7 = 128x128 (4 waves, 3 stages, software-pipelined loop)
//   8 = 128x64 (4 waves, 3 stages, PL = 1: one chunk per stage -- the bf16x3 loop with the planes deleted; A/B reference)
//   9 = halo patch 128x128 (3 stages, two patch buffers)                  10 = halo patch 128x64 (2 stages, one patch buffer)
constexpr int kBf16Cfgs = 10;

int cfg_bm(int cfg) { return (cfg == 4 || cfg == 5) ? 256 : cfg == 3 ? 64 : 128; }
int cfg_bn(int cfg) { return (cfg == 2 || cfg == 3 || cfg == 8 || cfg == 10) ? 64 : 128; }

// the automatic rule, from the MI355X sweep over the 33 resnet18 / resnet50 eval shapes at B = 1, 64, 256 (tools/sweep_conv_bf16.py,
// profiles/sweep_conv_bf16.json; t128 = 128x128-tile equivalents of the launch).  Summed over the shapes it is within 0.0 / 1.5 / 1.0 % of the
// per-shape best at B = 1 / 64 / 256 (the bf16x3 route: 1.57 / 2.22 / 2.44x the time):
//   * 64 output channels, or fewer than 256 tiles: 64x64 -- the grid must fill 256 CUs.  The halo-patch tiles lose here (layer1's 3x3 at
//     B = 64: 60 against 58 us) and everywhere else: with one plane the im2col ring's nine-fold reuse of the L2 is cheap enough.
//   * 256 ... 511 tiles: 128x128 / four waves (resnet50's 256-channel layers at B = 64: 27-42 us; the 256x128 tile leaves CUs idle, 34-53 us).
//   * from 512 tiles on: 256x128 / eight waves, software-pipelined (2-12 % ahead of the plain loop of the same tile on most shapes).
int pick_tile_bf16(const ConvP& p) {
    const long long M = p.cls[0].M;
    const long long t128 = ((M + 127) / 128) * (p.Cout / 128);
    if (p.Cout % 128 != 0 || t128 < 256) return 3;
    return t128 < 512 ? 1 : 5;
}

// which configurations a problem admits (forced ones are checked, never silently replaced)
const char* cfg_refusal(const ConvP& p, int cfg) {
    if (cfg < 1 || cfg > kBf16Cfgs) return "unknown tile configuration";
    if (p.Cout % cfg_bn(cfg) != 0) return "cout is not a multiple of the tile's N extent";
    if (cfg == 6 && p.Cin % 128 != 0) return "the four-chunk stage needs cin % 128 == 0";
    if (cfg == 9 && !(halo_patch_slots(p) > 0 && halo_patch_slots(p) <= 208)) return "the halo-patch tile needs a 3x3 / stride-1 layer whose patch fits 208 slots";
    if (cfg == 10 && !(halo_patch_slots(p) > 0 && halo_patch_slots(p) <= 272)) return "the halo-patch tile needs a 3x3 / stride-1 layer whose patch fits 272 slots";
    return nullptr;
}

int dispatch_bf16(ConvP p, int cfg, hipStream_t st) {
    // slot s of a stage = K chunk q * PL + s: the "plane strides" are the strides of one 32-channel chunk
    p.xps = (long long)p.xrows * 32;
    p.wps = (long long)p.Cout * 32;
    switch (cfg) {
        case 1: return launch_x3<128, 128, 2, 2, 3, 0, false, 3, 2>(p, st);
        case 2: return launch_x3<128, 64, 2, 2, 3, 0, false, 3, 2>(p, st);
        case 3: return launch_x3<64, 64, 2, 2, 3, 0, false, 3, 2>(p, st);
        case 4: return launch_x3<256, 128, 4, 2, 2, 0, false, 3, 2>(p, st);
        case 5: return launch_x3<256, 128, 4, 2, 2, 0, true, 3, 2>(p, st);
        case 6: return launch_x3<128, 128, 2, 2, 2, 0, false, 3, 4>(p, st);
        case 7: return launch_x3<128, 128, 2, 2, 3, 0, true, 3, 2>(p, st);
        case 8: return launch_x3<128, 64, 2, 2, 3, 0, false, 3, 1>(p, st);
        case 9: return launch_x3h<128, 128, 2, 2, 3, 208, 2, 3, 2>(p, st);
        case 10: return launch_x3h<128, 64, 2, 2, 2, 272, 1, 3, 2>(p, st);
        default: break;
    }
    straps_set_error("straps_conv_fwd_bf16: tile configuration %d does not exist", cfg);
    return STRAPS_EUNSUPPORTED;
}

// x [rows][C] fp32 -> rn_bf16(x) as one chunk-major plane; four channels per thread (one 8-byte store)
__global__ __launch_bounds__(256) void split1_cm_kernel(const float* __restrict__ x, u16* __restrict__ o, long long rows, int C) {
    const int C4 = C >> 2;
    const long long n4 = rows * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const long long r = i / C4;
        const int c = (int)(i - r * C4) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
        u16x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = bf16_rn(v[e]);
        *reinterpret_cast<u16x4*>(o + cm_index(r, c, rows)) = q;
    }
}

// OIHW fp32 weights -> rn_bf16 as one chunk-major plane of the forward layout: element (o, tap, c) at ((tap * (C / 32) + c / 32) * O + o) * 32 + c % 32
// (elementwise.hip wk_index).  One thread per destination element: the stores are contiguous, the (small) weight tensor is gathered.
__global__ __launch_bounds__(256) void pack_w_bf16_kernel(const float* __restrict__ w, u16* __restrict__ o, int O, int C, int RS) {
    const long long n = (long long)O * C * RS;
    const int CC = C >> 5;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int kl = (int)(e & 31);
        long long q = e >> 5;
        const int oo = (int)(q % O);
        q /= O;
        const int cc = (int)(q % CC);
        const int tap = (int)(q / CC);
        const int c = cc * 32 + kl;
        o[e] = bf16_rn(w[((long long)oo * C + c) * RS + tap]);
    }
}

unsigned grid_capped(long long n) {
    const long long g = (n + 255) / 256;
    return (unsigned)(g > 16384 ? 16384 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int straps_split_bf16_cm(const float* x, unsigned short* plane, long long rows, int c, void* stream) {
    STRAPS_REQUIRE(x && plane, "straps_split_bf16_cm: null pointer");
    STRAPS_REQUIRE(rows > 0 && c > 0 && c % 32 == 0, "straps_split_bf16_cm: need rows > 0 and c %% 32 == 0 (rows=%lld c=%d)", rows, c);
    STRAPS_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(plane) & 7) == 0,
                   "straps_split_bf16_cm: x must be 16-byte and plane 8-byte aligned");
    hipLaunchKernelGGL(split1_cm_kernel, dim3(grid_capped(rows * (c >> 2))), dim3(256), 0, (hipStream_t)stream, x, plane, rows, c);
    STRAPS_CHECK_LAUNCH("split1_cm_kernel");
    return STRAPS_OK;
}

extern "C" int straps_pack_conv_weight_bf16(const float* w_oihw, unsigned short* w_plane, int cout, int cin, int kh, int kw, void* stream) {
    STRAPS_REQUIRE(w_oihw && w_plane, "straps_pack_conv_weight_bf16: null pointer");
    STRAPS_REQUIRE(cout > 0 && cin > 0 && cin % 32 == 0, "straps_pack_conv_weight_bf16: need cout > 0 and cin %% 32 == 0 (cout=%d cin=%d)", cout, cin);
    STRAPS_REQUIRE(kh >= 1 && kw >= 1 && kh * kw <= 9, "straps_pack_conv_weight_bf16: bad filter geometry %dx%d", kh, kw);
    hipLaunchKernelGGL(pack_w_bf16_kernel, dim3(grid_capped((long long)cout * cin * kh * kw)), dim3(256), 0, (hipStream_t)stream, w_oihw, w_plane, cout, cin,
                       kh * kw);
    STRAPS_CHECK_LAUNCH("pack_w_bf16_kernel");
    return STRAPS_OK;
}

// the tile configuration straps_conv_fwd_bf16 takes for tile_cfg = 0 (1..10, see above); -1 for a geometry it does not cover
extern "C" int straps_conv_bf16_tile_choice(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad) {
    if (batch <= 0 || h <= 0 || w <= 0 || cin % 64 != 0 || cout % 64 != 0 || kh < 1 || kw < 1 || kh * kw > 9 || stride < 1 || pad < 0) return -1;
    ConvP p;
    p.x = nullptr; p.w = nullptr; p.xps = p.wps = 0;
    if (conv_fwd_problem(p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, batch, h, w, cin, cout, kh, kw, stride, pad) != STRAPS_OK) return -1;
    if (p.cls[0].M <= 0) return -1;
    return pick_tile_bf16(p);
}

extern "C" int straps_conv_fwd_bf16(const unsigned short* x1, const unsigned short* w1_krsc, const float* scale, const float* shift, const float* residual,
                                    int relu, float* y, unsigned short* y_plane, int batch, int h, int wdt, int cin, int cout, int kh, int kw, int stride,
                                    int pad, int tile_cfg, void* stream) {
    STRAPS_REQUIRE(x1 && w1_krsc, "straps_conv_fwd_bf16: null pointer");
    STRAPS_REQUIRE(y || y_plane, "straps_conv_fwd_bf16: no output (y and y_plane are both NULL)");
    STRAPS_REQUIRE(batch > 0 && h > 0 && wdt > 0, "straps_conv_fwd_bf16: empty input %dx%dx%d", batch, h, wdt);
    STRAPS_REQUIRE(cin % 64 == 0 && cout % 64 == 0, "straps_conv_fwd_bf16: need cin%%64==0 and cout%%64==0 (cin=%d cout=%d)", cin, cout);
    STRAPS_REQUIRE(kh >= 1 && kw >= 1 && kh * kw <= 9 && stride >= 1 && pad >= 0, "straps_conv_fwd_bf16: bad filter geometry");
    STRAPS_REQUIRE((scale == nullptr) == (shift == nullptr), "straps_conv_fwd_bf16: scale and shift must be given together");
    STRAPS_REQUIRE((reinterpret_cast<uintptr_t>(x1) & 15) == 0 && (reinterpret_cast<uintptr_t>(w1_krsc) & 15) == 0,
                   "straps_conv_fwd_bf16: x1 and w1_krsc must be 16-byte aligned");
    STRAPS_REQUIRE(tile_cfg >= 0 && tile_cfg <= kBf16Cfgs, "straps_conv_fwd_bf16: tile_cfg must be in [0, %d] (got %d)", kBf16Cfgs, tile_cfg);
    ConvP p;
    p.x = reinterpret_cast<const float*>(x1); p.w = reinterpret_cast<const float*>(w1_krsc);
    p.xps = p.wps = 0;
    const int rc = conv_fwd_problem(p, scale, shift, residual, relu, y, nullptr, batch, h, wdt, cin, cout, kh, kw, stride, pad);
    if (rc != STRAPS_OK) return rc;
    STRAPS_REQUIRE(p.cls[0].M > 0, "straps_conv_fwd_bf16: empty output");
    const int cfg = tile_cfg ? tile_cfg : pick_tile_bf16(p);
    const char* why = cfg_refusal(p, cfg);
    STRAPS_REQUIRE(!why, "straps_conv_fwd_bf16: tile_cfg %d: %s", cfg, why);
    p.yplanes = y_plane;
    p.yps = 0;
    return dispatch_bf16(p, cfg, (hipStream_t)stream);
}
