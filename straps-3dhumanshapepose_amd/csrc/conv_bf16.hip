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

int dispatch_bf16(ConvP p, const ConvPlan& pl, hipStream_t st) {
    // slot s of a stage = K chunk q * PL + s: the "plane strides" are the strides of one 32-channel chunk
    p.xps = (long long)p.xrows * 32;
    p.wps = (long long)p.Cout * 32;
    return launch_x3_tiles<kBf16Tile, 3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10>(p, pl, st);
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

// the tile configuration straps_conv_fwd_bf16 takes for tile_cfg = 0 (1..10, conv_plan.h); -1 for a geometry it does not cover
extern "C" int straps_conv_bf16_tile_choice(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad) {
    if (batch <= 0 || h <= 0 || w <= 0 || cin % 64 != 0 || cout % 64 != 0 || kh < 1 || kw < 1 || kh * kw > 9 || stride < 1 || pad < 0) return -1;
    ConvPlan pl;
    return conv_plan_for("straps_conv_bf16_tile_choice", STRAPS_CONV_ROUTE_BF16, STRAPS_CONV_KIND_FWD, STRAPS_CONV_OP_Y | STRAPS_CONV_OP_YPLANES, batch, h, w, cin, cout,
                         kh, kw, stride, pad, 0, pl) == STRAPS_OK ? pl.q.tile : -1;
}

extern "C" int straps_conv_fwd_bf16(const unsigned short* x1, const unsigned short* w1_krsc, const float* scale, const float* shift, const float* residual,
                                    int relu, float* y, unsigned short* y_plane, int batch, int h, int wdt, int cin, int cout, int kh, int kw, int stride,
                                    int pad, int tile_cfg, void* stream) {
    STRAPS_REQUIRE(x1 && w1_krsc, "straps_conv_fwd_bf16: null pointer");
    STRAPS_REQUIRE(y || y_plane, "straps_conv_fwd_bf16: no output (y and y_plane are both NULL)");
    const int ok = conv_geometry_check("straps_conv_fwd_bf16", STRAPS_CONV_ROUTE_BF16, STRAPS_CONV_KIND_FWD, batch, h, wdt, cin, cout, kh, kw, stride, pad);
    if (ok != STRAPS_OK) return ok;
    STRAPS_REQUIRE((scale == nullptr) == (shift == nullptr), "straps_conv_fwd_bf16: scale and shift must be given together");
    STRAPS_REQUIRE((reinterpret_cast<uintptr_t>(x1) & 15) == 0 && (reinterpret_cast<uintptr_t>(w1_krsc) & 15) == 0,
                   "straps_conv_fwd_bf16: x1 and w1_krsc must be 16-byte aligned");
    ConvP p;
    p.x = reinterpret_cast<const float*>(x1); p.w = reinterpret_cast<const float*>(w1_krsc);
    p.xps = p.wps = 0;
    const int rc = conv_fwd_problem(p, scale, shift, residual, relu, y, nullptr, batch, h, wdt, cin, cout, kh, kw, stride, pad);
    if (rc != STRAPS_OK) return rc;
    p.yplanes = y_plane;
    p.yps = 0;
    ConvPlan pl;
    const int rp = conv_plan_bf16("straps_conv_fwd_bf16", conv_shape(p), tile_cfg, pl);      // (a forced configuration is checked, never silently replaced)
    return rp != STRAPS_OK ? rp : dispatch_bf16(p, pl, (hipStream_t)stream);
}
