// conv_x3.hip -- the implicit-GEMM convolution of conv.hip on the bf16 matrix pipe at fp32 accuracy.
//
//   Every fp32 operand value is carried as three bf16 planes  x = x1 + x2 + x3  (round-to-nearest splits: the sum is EXACT, 3 x 8
//   significand bits cover fp32's 24; bf16 has fp32's exponent, so no scaling and no range analysis is needed; only below 2^-110 do
//   the last bits fall under bf16's smallest subnormal: absolute error <= 2^-133 there; above bf16's largest finite value, 3.39e38,
//   the leading plane rounds to infinity and the value is lost: an fp32 activation that close to overflow is already a failed run), and a product
//   a*b is evaluated as the six bf16 products of weight >= 2^-16
//        a1*b1 + a1*b2 + a2*b1 + a1*b3 + a3*b1 + a2*b2          (dropped: a2*b3 + a3*b2 + a3*b3 <= 2^-23 |a*b|)
//   each exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16.  Six 32-cycle instructions do the work of eight 64-cycle
//   v_mfma_f32_32x32x2_f32: 2.67x the exact-fp32 pipe at the same accuracy class (measured error vs float64: tests/test_gpu_conv_x3.py).
//   The planes are separate [pixels][C] bf16 tensors (straps_split3_bf16 writes them; 6 bytes per element instead of 4).
//
//   Same structure as conv.hip: tap table, LDS-DMA operand copies (a 32-channel K chunk of one plane is 64 contiguous bytes of one
//   pixel -> 4 lanes x 16 bytes), two stages, one barrier per chunk, XOR-swizzled 64-byte rows read back as one ds_read_b128 per
//   (32-row block, plane, 16-wide k step), the shared epilogue of conv_igemm.h.  The copies of chunk q+1 are issued between the
//   MFMAs of chunk q (a chunk's matrix work is only 6 x 2 x MI x NI x 32 cycles: issued in front of it they would cost as much
//   as the burst itself).
#include "conv_x3_kernels.h"

// conv_x3_lean.hip: the same kernels with the lean epilogues (p: a ConvP of this translation unit -- the header gives both the same layout)
int straps_internal_dispatch_x3_lean(const void* p, const ConvPlan& pl, hipStream_t st);

namespace {

int dispatch_x3(const ConvP& p, int tile_cfg, hipStream_t st) {
    ConvPlan pl;
    const int rc = conv_plan_x3(conv_shape(p), tile_cfg, conv_ops(p), pl);
    if (rc != STRAPS_OK) return rc;
    if (pl.q.epilogue) return straps_internal_dispatch_x3_lean(&p, pl, st);
    if (pl.q.family == STRAPS_CONV_FAMILY_PLANE_HALO) return launch_x3_tiles<kX3Halo, 0, 0, 1, 2, 3>(p, pl, st);
#ifdef STRAPS_TOOLS
    // ablation instantiations (wrong results by design: tools/x3_ablate.py) exist only in the tools build; the product library ignores the bits
    if (pl.abl == 3) return launch_x3_tiles<kX3Tile, 0, 3, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12>(p, pl, st);
    if (pl.abl == 1) return launch_x3_tiles<kX3Tile, 0, 1, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12>(p, pl, st);
    if (pl.abl == 2) return launch_x3_tiles<kX3Tile, 0, 2, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12>(p, pl, st);
#endif
    return launch_x3_tiles<kX3Tile, 0, 0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12>(p, pl, st);
}

__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ x, u16* __restrict__ o, long long n, long long ps) {
    const long long i4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 + 3 < n) {
        store_planes4(o, ps, i4, *reinterpret_cast<const f32x4*>(x + i4));
    } else {
        for (long long i = i4; i < n; ++i) {
            u16 b1, b2, b3;
            split3(x[i], b1, b2, b3);
            o[i] = b1; o[ps + i] = b2; o[2 * ps + i] = b3;
        }
    }
}

// the same split into the chunk-major layout the convolution kernels read (common.h: cm_index): x is a [rows][C] fp32 tensor
__global__ __launch_bounds__(256) void split3_cm_kernel(const float* __restrict__ x, u16* __restrict__ o, long long rows, int C, long long ps) {
    const int C4 = C >> 2;
    const long long n4 = rows * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const long long r = i / C4;
        const int c4 = (int)(i - r * C4);
        store_planes4_cm(o, ps, r, c4 * 4, rows, *reinterpret_cast<const f32x4*>(x + i * 4));
    }
}

}  // namespace

extern "C" int straps_split3_bf16_cm(const float* x, unsigned short* planes, long long rows, int c, long long plane_stride, void* stream) {
    STRAPS_REQUIRE(x && planes, "straps_split3_bf16_cm: null pointer");
    STRAPS_REQUIRE(rows > 0 && c > 0 && c % 32 == 0, "straps_split3_bf16_cm: need rows > 0 and c %% 32 == 0 (rows=%lld c=%d)", rows, c);
    STRAPS_REQUIRE(plane_stride >= rows * c && plane_stride % 8 == 0, "straps_split3_bf16_cm: plane_stride must be >= rows*c and a multiple of 8");
    STRAPS_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(planes) & 15) == 0, "straps_split3_bf16_cm: pointers must be 16-byte aligned");
    const long long n4 = rows * (c >> 2);
    const long long g = (n4 + 255) / 256;
    hipLaunchKernelGGL(split3_cm_kernel, dim3((unsigned)(g > 16384 ? 16384 : g)), dim3(256), 0, (hipStream_t)stream, x, planes, rows, c, plane_stride);
    STRAPS_CHECK_LAUNCH("split3_cm_kernel");
    return STRAPS_OK;
}

extern "C" int straps_split3_bf16(const float* x, unsigned short* planes, long long n, long long plane_stride, void* stream) {
    STRAPS_REQUIRE(x && planes, "straps_split3_bf16: null pointer");
    STRAPS_REQUIRE(n >= 0 && plane_stride >= n && plane_stride % 8 == 0, "straps_split3_bf16: plane_stride must be >= n and a multiple of 8");
    if (n == 0) return STRAPS_OK;
    STRAPS_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(planes) & 15) == 0, "straps_split3_bf16: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(split3_kernel, dim3(cdiv(n, 1024)), dim3(256), 0, (hipStream_t)stream, x, planes, n, plane_stride);
    STRAPS_CHECK_LAUNCH("split3_kernel");
    return STRAPS_OK;
}

// straps_conv_fwd_x3 (y_planes == NULL, `stats_partial` optional) and straps_conv_fwd_x3p (no statistics) in one body
static int conv_fwd_x3_impl(const char* who, const unsigned short* x3, long long x_plane_stride, const unsigned short* w3, long long w_plane_stride,
                            const float* scale, const float* shift, const float* residual, int relu, float* y, float* stats_partial, unsigned short* y_planes,
                            long long y_plane_stride, int batch, int h, int wdt, int cin, int cout, int kh, int kw, int stride, int pad, int tile_cfg, void* stream) {
    STRAPS_REQUIRE(x3 && w3 && (y_planes || y), "%s: null pointer", who);
    const int ok = conv_geometry_check(who, STRAPS_CONV_ROUTE_PLANES, STRAPS_CONV_KIND_FWD, batch, h, wdt, cin, cout, kh, kw, stride, pad);
    if (ok != STRAPS_OK) return ok;
    STRAPS_REQUIRE((scale == nullptr) == (shift == nullptr), "%s: scale and shift must be given together", who);
    STRAPS_REQUIRE(x_plane_stride % 8 == 0 && w_plane_stride % 8 == 0 && y_plane_stride % 8 == 0, "%s: plane strides must be multiples of 8 elements", who);
    ConvP p;
    p.x = reinterpret_cast<const float*>(x3); p.w = reinterpret_cast<const float*>(w3);
    p.xps = x_plane_stride; p.wps = w_plane_stride;
    const int rc = conv_fwd_problem(p, scale, shift, residual, relu, y, stats_partial, batch, h, wdt, cin, cout, kh, kw, stride, pad);
    if (rc != STRAPS_OK) return rc;
    STRAPS_REQUIRE(!y_planes || y_plane_stride >= (long long)p.cls[0].M * cout, "%s: y_plane_stride smaller than the output", who);
    p.yplanes = y_planes; p.yps = y_plane_stride;
    return dispatch_x3(p, tile_cfg, (hipStream_t)stream);
}

extern "C" int straps_conv_fwd_x3(const unsigned short* x3, long long x_plane_stride, const unsigned short* w3, long long w_plane_stride,
                                  const float* scale, const float* shift, const float* residual, int relu, float* y, float* stats_partial,
                                  int batch, int h, int wdt, int cin, int cout, int kh, int kw, int stride, int pad, int tile_cfg, void* stream) {
    STRAPS_REQUIRE(y, "straps_conv_fwd_x3: null pointer");
    return conv_fwd_x3_impl("straps_conv_fwd_x3", x3, x_plane_stride, w3, w_plane_stride, scale, shift, residual, relu, y, stats_partial, nullptr, 0, batch, h, wdt,
                            cin, cout, kh, kw, stride, pad, tile_cfg, stream);
}

// straps_conv_fwd_x3 whose epilogue also writes the result's three bf16 planes (eval-mode chains: the next convolution's operand without
// a split pass); y may be NULL when only the planes are consumed.
extern "C" int straps_conv_fwd_x3p(const unsigned short* x3, long long x_plane_stride, const unsigned short* w3, long long w_plane_stride,
                                   const float* scale, const float* shift, const float* residual, int relu, float* y, unsigned short* y_planes,
                                   long long y_plane_stride, int batch, int h, int wdt, int cin, int cout, int kh, int kw, int stride, int pad,
                                   int tile_cfg, void* stream) {
    STRAPS_REQUIRE(y_planes, "straps_conv_fwd_x3p: null pointer");
    return conv_fwd_x3_impl("straps_conv_fwd_x3p", x3, x_plane_stride, w3, w_plane_stride, scale, shift, residual, relu, y, nullptr, y_planes, y_plane_stride, batch,
                            h, wdt, cin, cout, kh, kw, stride, pad, tile_cfg, stream);
}

// every data gradient of the plane route: addend (+ addend_bits), and with bn_raw the fused BatchNorm-backward sums (mask: bn_out, its bits, or scale / shift)
static int conv_dgrad_x3_impl(const unsigned short* dy3, long long dy_plane_stride, const unsigned short* w3_crsk, long long w_plane_stride,
                              const float* addend, const unsigned* addend_bits, float* dx, int batch, int h, int wdt, int cin, int cout, int kh, int kw,
                              int stride, int pad, int tile_cfg, bool bn, const float* bn_raw, const float* bn_out, const unsigned* bn_out_bits,
                              const float* bn_mask_scale, const float* bn_mask_shift, const float* bn_mean, const float* bn_invstd,
                              double* bn_partials, void* stream) {
    const char* who = bn ? "straps_conv_dgrad_x3_bn" : "straps_conv_dgrad_x3";
    STRAPS_REQUIRE(dy3 && w3_crsk && dx, "%s: null pointer", who);
    STRAPS_REQUIRE(!bn || (bn_raw && bn_mean && bn_invstd && bn_partials && (bn_out || bn_out_bits || (bn_mask_scale && bn_mask_shift))),
                   "%s: the BatchNorm tensors (raw, mean, invstd, partials, and out / its bits or mask scale / shift) are required", who);
    STRAPS_REQUIRE(!addend_bits || addend, "%s_bits: the ReLU bits mask an addend", who);
    STRAPS_REQUIRE(!(addend_bits || bn_out_bits) || cin % 32 == 0, "%s_bits: bit masks need cin %% 32 == 0 (cin=%d)", who, cin);
    const int ok = conv_geometry_check(who, STRAPS_CONV_ROUTE_PLANES, STRAPS_CONV_KIND_DGRAD, batch, h, wdt, cin, cout, kh, kw, stride, pad);
    if (ok != STRAPS_OK) return ok;
    STRAPS_REQUIRE(dy_plane_stride % 8 == 0 && w_plane_stride % 8 == 0, "%s: plane strides must be multiples of 8 elements", who);
    ConvP p;
    p.x = reinterpret_cast<const float*>(dy3); p.w = reinterpret_cast<const float*>(w3_crsk);
    p.xps = dy_plane_stride; p.wps = w_plane_stride;
    const int rc = conv_dgrad_problem(p, addend, dx, batch, h, wdt, cin, cout, kh, kw, stride, pad);
    if (rc != STRAPS_OK) return rc;
    p.bnr_raw = bn_raw; p.bnr_out = bn_out; p.bnr_sc = bn_mask_scale; p.bnr_sh = bn_mask_shift; p.bnr_mean = bn_mean; p.bnr_invstd = bn_invstd;
    p.bnr_part = bn_partials;
    p.bnr_bits = bn_out_bits; p.res_bits = addend_bits;
    return p.ncls ? dispatch_x3(p, tile_cfg, (hipStream_t)stream) : STRAPS_OK;
}

extern "C" int straps_conv_dgrad_x3(const unsigned short* dy3, long long dy_plane_stride, const unsigned short* w3_crsk, long long w_plane_stride,
                                    const float* addend, float* dx, int batch, int h, int wdt, int cin, int cout, int kh, int kw, int stride,
                                    int pad, int tile_cfg, void* stream) {
    return conv_dgrad_x3_impl(dy3, dy_plane_stride, w3_crsk, w_plane_stride, addend, nullptr, dx, batch, h, wdt, cin, cout, kh, kw, stride, pad, tile_cfg,
                              false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

// straps_conv_dgrad_x3 whose addend is the UNMASKED gradient of a residual unit's output: dx = dgrad + (bit ? addend : 0), with the unit's ReLU
// decisions as bits (straps_bn_apply_bits_x3: word [pixel][cin / 32], bit c & 31) -- the masked copy `dz` of that gradient is never written
extern "C" int straps_conv_dgrad_x3_bits(const unsigned short* dy3, long long dy_plane_stride, const unsigned short* w3_crsk, long long w_plane_stride,
                                         const float* addend, float* dx, int batch, int h, int wdt, int cin, int cout, int kh, int kw, int stride,
                                         int pad, int tile_cfg, const unsigned* addend_bits, void* stream) {
    STRAPS_REQUIRE(addend_bits, "straps_conv_dgrad_x3_bits: null bit mask");
    return conv_dgrad_x3_impl(dy3, dy_plane_stride, w3_crsk, w_plane_stride, addend, addend_bits, dx, batch, h, wdt, cin, cout, kh, kw, stride, pad,
                              tile_cfg, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int straps_conv_dgrad_x3_bn(const unsigned short* dy3, long long dy_plane_stride, const unsigned short* w3_crsk, long long w_plane_stride,
                                       const float* addend, float* dx, int batch, int h, int wdt, int cin, int cout, int kh, int kw, int stride,
                                       int pad, int tile_cfg, const float* bn_raw, const float* bn_out, const float* bn_mask_scale,
                                       const float* bn_mask_shift, const float* bn_mean, const float* bn_invstd, double* bn_partials, void* stream) {
    return conv_dgrad_x3_impl(dy3, dy_plane_stride, w3_crsk, w_plane_stride, addend, nullptr, dx, batch, h, wdt, cin, cout, kh, kw, stride, pad, tile_cfg,
                              true, bn_raw, bn_out, nullptr, bn_mask_scale, bn_mask_shift, bn_mean, bn_invstd, bn_partials, stream);
}

// straps_conv_dgrad_x3_bn with ReLU decisions as bits (word [pixel][cin / 32], bit c & 31; straps_bn_apply_bits_x3) wherever the fp32 form reads
// a whole activation tensor for its sign: bn_out_bits replaces bn_out as the mask of the BatchNorm sums (4 B per element less), addend_bits
// masks the addend, which is then the unmasked gradient of the later unit's output (either may be NULL: that operand is used as before)
extern "C" int straps_conv_dgrad_x3_bn_bits(const unsigned short* dy3, long long dy_plane_stride, const unsigned short* w3_crsk, long long w_plane_stride,
                                            const float* addend, float* dx, int batch, int h, int wdt, int cin, int cout, int kh, int kw, int stride,
                                            int pad, int tile_cfg, const float* bn_raw, const float* bn_out, const float* bn_mask_scale,
                                            const float* bn_mask_shift, const float* bn_mean, const float* bn_invstd, double* bn_partials,
                                            const unsigned* addend_bits, const unsigned* bn_out_bits, void* stream) {
    return conv_dgrad_x3_impl(dy3, dy_plane_stride, w3_crsk, w_plane_stride, addend, addend_bits, dx, batch, h, wdt, cin, cout, kh, kw, stride, pad,
                              tile_cfg, true, bn_raw, bn_out, bn_out_bits, bn_mask_scale, bn_mask_shift, bn_mean, bn_invstd, bn_partials, stream);
}

// number of [cout][2] statistics partials straps_conv_fwd_x3 writes for this geometry (= its M tiles): the plan of a training forward
extern "C" int straps_conv_x3_stat_blocks(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int tile_cfg) {
    ConvPlan pl;
    return conv_plan_for("straps_conv_x3_stat_blocks", STRAPS_CONV_ROUTE_PLANES, STRAPS_CONV_KIND_FWD, STRAPS_CONV_OP_Y | STRAPS_CONV_OP_STATS, batch, h, w, cin, cout,
                         kh, kw, stride, pad, tile_cfg, pl) == STRAPS_OK ? pl.q.blocks : -1;
}

// M tiles (= BatchNorm-backward partial blocks) of straps_conv_dgrad_x3_bn[_bits] for this geometry, all parity classes
extern "C" int straps_conv_dgrad_x3_bn_blocks(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int tile_cfg) {
    ConvPlan pl;
    if (!(stride == 1 || stride == 2) || kh * kw > 9 || kh - 1 - pad < 0 || kw - 1 - pad < 0) return -1;
    return conv_plan_for("straps_conv_dgrad_x3_bn_blocks", STRAPS_CONV_ROUTE_PLANES, STRAPS_CONV_KIND_DGRAD, STRAPS_CONV_OP_Y | STRAPS_CONV_OP_RES | STRAPS_CONV_OP_BNR_RAW,
                         batch, h, w, cin, cout, kh, kw, stride, pad, tile_cfg, pl) == STRAPS_OK ? pl.q.blocks : -1;
}
