// stem_dgrad.hip -- data gradient of the stem conv 7x7 / stride 2 / pad 3 (models/resnet.py:145) w.r.t. its NCHW input
//
// dx[b][c][hi][wi] = sum_{o,r,s} dy[b][ho][wo][o] * w[o][c][r][s],  hi = 2 ho - 3 + r,  wi = 2 wo - 3 + s.
//
// SPACE-TO-DEPTH mapping: the 2 x 2 input block (Y, X) = rows 2Y + py, columns 2X + px receives taps from the 4 x 4 window of
// dy pixels (Y - 1 + d, X - 1 + e), d, e = 0..3, with r = py + 5 - 2d and s = px + 5 - 2e (a tap outside 0..6 is a zero
// weight: 49 of the 64 (d, e, py, px) combinations are real).  The block grid is exactly the dy grid (Ho = ceil(H / 2)), so the
// whole gradient is ONE dense GEMM per image:
//   M = Ho * Wo blocks,  K = 16 window taps x 64 dy channels = 1024,  N = 4 parities x cin,
// with the weight repacked (straps_pack_stem_dgrad_weight) into a [K][N] matrix that holds the zero taps.  N is cut into chunks of
// 20 channels x 4 parities = 80 columns = 5 tiles of v_mfma_f32_16x16x4_f32 (cin = 18: 72 of 80 columns used; useful MACs
// 49/64 x 72/80 = 69 %).  Exact fp32 products, fp32 accumulation -- the arithmetic class of stem_kernel.
//
// Workgroup: 4 block rows x 32 block columns of one image and one channel chunk; wave w owns block row w (2 M tiles of 16 blocks
// x NT N tiles).  The dy halo patch (7 rows x 35 pixels x 64 channels, 68-float pixel stride) is loaded once into LDS with
// float4 reads; A fragments are ds_read_b128 of four consecutive channels (element s = K step s of a 16-channel group, the pack
// uses the same order); B fragments stream from L2 as coalesced float4 in fragment order.  The epilogue interleaves the two
// column parities of each input row in LDS and writes dx as contiguous NCHW rows (256 bytes per wave store), no transpose pass.
#include "common.h"

namespace {

constexpr int TYB = 4, TXB = 32;                  // blocks per workgroup: one block row per wave
constexpr int PR = TYB + 3, PC = TXB + 3;          // dy patch rows / pixels per row
constexpr int PS = 68;                             // floats per patch pixel (64 + 4: the 16 lanes of a ds_read_b128 hit distinct banks)
constexpr int CCH = 20;                            // input channels per N chunk (x 4 parities = 80 columns = 5 MFMA tiles)
constexpr int NTMAX = 5;
constexpr int KG = 64;                             // K groups of 16: 16 window taps x 4 groups of 16 dy channels
constexpr size_t LDS_BYTES = (size_t)PR * PC * PS * sizeof(float);
static_assert(TYB * CCH * 2 * 2 * TXB <= PR * PC * PS, "the epilogue staging must fit in the patch");

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <int NT>
__global__ __launch_bounds__(256, 2) STRAPS_NO_PACKED_FP32 void stem_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ wpk,
                                                                                 float* __restrict__ dx, int C, int H, int W, int Ho, int Wo,
                                                                                 int tiles_x, int tiles_y, int nch, int ch0, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float smem[];      // [PR][PC][PS] dy patch; then [4 waves][CCH][2][64] staging
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bid = blockIdx.x;
    const int b = bid / (tiles_x * tiles_y);
    bid -= b * tiles_x * tiles_y;
    const int ty = bid / tiles_x, tx = bid - ty * tiles_x;
    const int Y0 = ty * TYB, X0 = tx * TXB;
    const int ch = ch0 + blockIdx.y;
    const int c0 = ch * CCH, ncc = min(CCH, C - c0);

    // ---- dy patch: rows Y0-1 .. Y0+5, pixels X0-1 .. X0+33, zero outside the image; 16 float4 per pixel ----
    constexpr int NV = PR * PC * 16;                   // 3920 float4
    const float* dyb = dy + (long long)b * Ho * Wo * 64;
#pragma unroll
    for (int u0 = 0; u0 < 16; u0 += 8) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = (u0 + u) * 256 + tid;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (idx < NV) {
                const int q = idx & 15, pix = idx >> 4;
                const int pr = pix / PC, pc = pix - pr * PC;
                const int yy = Y0 - 1 + pr, xx = X0 - 1 + pc;
                if ((unsigned)yy < (unsigned)Ho && (unsigned)xx < (unsigned)Wo)
                    v[u] = *reinterpret_cast<const f32x4*>(dyb + ((long long)yy * Wo + xx) * 64 + 4 * q);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = (u0 + u) * 256 + tid;
            if (idx < NV) *reinterpret_cast<f32x4*>(smem + (idx >> 4) * PS + 4 * (idx & 15)) = v[u];
        }
    }
    __syncthreads();

    // ---- K loop: kg = tap (d, e) x 4 + channel group g; lane (i = block, kq) reads dy channels 16 g + 4 kq .. + 3 of its pixel ----
    const int i = lane & 15, kq = lane >> 4;
    const float* arow = smem + (wave * PC + i) * PS + 4 * kq;
    const f32x4* __restrict__ wb = reinterpret_cast<const f32x4*>(wpk) + (long long)ch * NTMAX * 64 + lane;
    const long long kstride = (long long)nch * NTMAX * 64;       // f32x4 between consecutive K groups
    f32x4 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[m][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto aoff = [&](int kg) { const int t = kg >> 2; return ((t >> 2) * PC + (t & 3)) * PS + 16 * (kg & 3); };
    f32x4 bn[NT], a0 = *reinterpret_cast<const f32x4*>(arow + aoff(0)), a1 = *reinterpret_cast<const f32x4*>(arow + aoff(0) + 16 * PS);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bn[nt] = wb[nt * 64];
    for (int kg = 0; kg < KG; ++kg) {
        f32x4 bc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bc[nt] = bn[nt];
        const f32x4 ac0 = a0, ac1 = a1;
        if (kg + 1 < KG) {          // next group's fragments in flight while this one's MFMAs issue
            const int o = aoff(kg + 1);
            a0 = *reinterpret_cast<const f32x4*>(arow + o);
            a1 = *reinterpret_cast<const f32x4*>(arow + o + 16 * PS);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bn[nt] = wb[(kg + 1) * kstride + nt * 64];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[0][nt] = mfma16(ac0[s], bc[nt][s], acc[0][nt]);
                acc[1][nt] = mfma16(ac1[s], bc[nt][s], acc[1][nt]);
            }
    }

    // ---- epilogue: stage [wave][channel][py][64 columns] (parities interleaved), then contiguous NCHW row stores ----
    __syncthreads();                                   // every wave is done with the patch
    float* st = smem + wave * (CCH * 2 * 2 * TXB);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = nt * 16 + i;                  // C/D: column = lane & 15, row = 4 (lane >> 4) + reg
            const int cl = n >> 2, py = (n >> 1) & 1, px = n & 1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int xi = m * 16 + 4 * kq + r;
                st[(cl * 2 + py) * (2 * TXB) + 2 * xi + px] = acc[m][nt][r];
            }
        }
    __syncthreads();
    const int Y = Y0 + wave, wi = 2 * X0 + lane;
    if (wi < W) {
        float* dxb = dx + ((long long)b * C + c0) * H * W + wi;
        for (int rr = 0; rr < 2 * ncc; ++rr) {
            const int hi = 2 * Y + (rr & 1);
            if (hi >= H) continue;
            float v = st[rr * (2 * TXB) + lane];
            float* p = dxb + ((long long)(rr >> 1) * H + hi) * W;
            if (accumulate) v += *p;
            *p = v;
        }
    }
}

// [KG][nch][NTMAX][64 lanes][4]: lane = kq * 16 + j, element s -> K index (tap t = kg >> 2, dy channel o = 16 (kg & 3) + 4 kq + s),
// N index n = nt * 16 + j of chunk ch -> channel ch * CCH + (n >> 2), parity (py, px) = ((n >> 1) & 1, n & 1)
__global__ __launch_bounds__(256) void pack_stem_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wp, int C, int nch) {
    const long long total = (long long)KG * nch * NTMAX * 256;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int s = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    long long t = idx >> 8;
    const int nt = (int)(t % NTMAX);
    t /= NTMAX;
    const int ch = (int)(t % nch);
    const int kg = (int)(t / nch);
    const int tap = kg >> 2, d = tap >> 2, e = tap & 3;
    const int o = 16 * (kg & 3) + 4 * (lane >> 4) + s;
    const int n = nt * 16 + (lane & 15);
    const int cl = n >> 2, py = (n >> 1) & 1, px = n & 1;
    const int c = ch * CCH + cl;
    const int r = py + 5 - 2 * d, q = px + 5 - 2 * e;
    float v = 0.f;
    if (cl < CCH && c < C && r >= 0 && r < 7 && q >= 0 && q < 7) v = w[(((long long)o * C + c) * 7 + r) * 7 + q];
    wp[idx] = v;
}

}  // namespace

extern "C" size_t straps_stem_dgrad_weight_floats(int cin) {
    if (cin < 1 || cin > STRAPS_STEM_DGRAD_MAX_CIN) return 0;
    return (size_t)KG * ((cin + CCH - 1) / CCH) * NTMAX * 256;
}

extern "C" int straps_pack_stem_dgrad_weight(const float* w_oihw, float* w_pk, int cin, void* stream) {
    STRAPS_REQUIRE(w_oihw && w_pk, "straps_pack_stem_dgrad_weight: null pointer");
    STRAPS_REQUIRE(cin >= 1 && cin <= STRAPS_STEM_DGRAD_MAX_CIN, "straps_pack_stem_dgrad_weight: cin=%d outside 1..%d", cin, STRAPS_STEM_DGRAD_MAX_CIN);
    const int nch = (cin + CCH - 1) / CCH;
    const long long n = (long long)KG * nch * NTMAX * 256;
    hipLaunchKernelGGL(pack_stem_dgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_oihw, w_pk, cin, nch);
    STRAPS_CHECK_LAUNCH("pack_stem_dgrad_kernel");
    return STRAPS_OK;
}

template <int NT>
static int launch_stem_dgrad(dim3 grid, hipStream_t st, const float* dy, const float* wpk, float* dx, int C, int H, int W, int Ho, int Wo, int tiles_x,
                             int tiles_y, int nch, int ch0, int accumulate) {
    STRAPS_RAISE_LDS(stem_dgrad_kernel<NT>, LDS_BYTES, "stem_dgrad_kernel");
    hipLaunchKernelGGL(stem_dgrad_kernel<NT>, grid, dim3(256), LDS_BYTES, st, dy, wpk, dx, C, H, W, Ho, Wo, tiles_x, tiles_y, nch, ch0, accumulate);
    STRAPS_CHECK_LAUNCH("stem_dgrad_kernel");
    return STRAPS_OK;
}

extern "C" int straps_stem_dgrad(const float* dy_nhwc, const float* w_pk, float* dx_nchw, int batch, int cin, int h, int w, int accumulate,
                                 void* stream) {
    STRAPS_REQUIRE(dy_nhwc && w_pk && dx_nchw, "straps_stem_dgrad: null pointer");
    STRAPS_REQUIRE(batch > 0 && cin > 0 && h >= 7 && w >= 7, "straps_stem_dgrad: bad shape B=%d C=%d H=%d W=%d (B, C >= 1, H, W >= 7)", batch, cin, h, w);
    STRAPS_REQUIRE(cin <= STRAPS_STEM_DGRAD_MAX_CIN, "straps_stem_dgrad: cin=%d above the supported %d input channels", cin, STRAPS_STEM_DGRAD_MAX_CIN);
    STRAPS_REQUIRE(accumulate == 0 || accumulate == 1, "straps_stem_dgrad: accumulate must be 0 or 1 (got %d)", accumulate);
    const int Ho = (h - 1) / 2 + 1, Wo = (w - 1) / 2 + 1;
    const int tiles_x = (Wo + TXB - 1) / TXB, tiles_y = (Ho + TYB - 1) / TYB;
    const long long nblk = (long long)batch * tiles_x * tiles_y;
    STRAPS_REQUIRE(nblk < (1LL << 31), "straps_stem_dgrad: grid too large");
    const int nch = (cin + CCH - 1) / CCH, full = cin / CCH, rest = cin - full * CCH;
    hipStream_t st = (hipStream_t)stream;
    if (full > 0) {
        const int rc = launch_stem_dgrad<NTMAX>(dim3((unsigned)nblk, (unsigned)full), st, dy_nhwc, w_pk, dx_nchw, cin, h, w, Ho, Wo, tiles_x, tiles_y, nch, 0,
                                                accumulate);
        if (rc != STRAPS_OK) return rc;
    }
    if (rest > 0) {      // the last, partial chunk: only the N tiles its channels occupy
        const dim3 g((unsigned)nblk, 1);
        switch ((rest * 4 + 15) / 16) {
            case 1: return launch_stem_dgrad<1>(g, st, dy_nhwc, w_pk, dx_nchw, cin, h, w, Ho, Wo, tiles_x, tiles_y, nch, full, accumulate);
            case 2: return launch_stem_dgrad<2>(g, st, dy_nhwc, w_pk, dx_nchw, cin, h, w, Ho, Wo, tiles_x, tiles_y, nch, full, accumulate);
            case 3: return launch_stem_dgrad<3>(g, st, dy_nhwc, w_pk, dx_nchw, cin, h, w, Ho, Wo, tiles_x, tiles_y, nch, full, accumulate);
            case 4: return launch_stem_dgrad<4>(g, st, dy_nhwc, w_pk, dx_nchw, cin, h, w, Ho, Wo, tiles_x, tiles_y, nch, full, accumulate);
            default: return launch_stem_dgrad<5>(g, st, dy_nhwc, w_pk, dx_nchw, cin, h, w, Ho, Wo, tiles_x, tiles_y, nch, full, accumulate);
        }
    }
    return STRAPS_OK;
}
