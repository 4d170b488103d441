// backward.hip -- gradient kernels of the encoder / IEF / rot6d (what autograd + cuDNN/cuBLAS do for the
// reference's loss.backward(), train/train_synthetic_otf_rendering.py:232).  The convolution weight gradients are in conv_wgrad.hip.
//
//   stem_wgrad_kernel      dW of the 7x7/s2 stem straight from the NCHW input (LDS halo patch, like stem.hip; deterministic
//                          partials + fixed-order reduce)
//   bn_bwd_*               training-mode BatchNorm backward with the ReLU mask fused (two passes: reduce, apply)
//   maxpool / gap backward, masked_copy
//   rot6d_bwd_kernel       Gram-Schmidt backward
#include "common.h"
#include <stdlib.h>

namespace {


// =====================================================================================================
// stem weight gradient (no data gradient is needed: the network input does not require grad)
// =====================================================================================================
// The network input is the proxy representation: a silhouette + 17 truncated joint heat-maps, ~98 % exact zeros.  The
// kernel is organised around that: a workgroup owns ONE GROUP OF 4 INPUT CHANNELS (grid.y) and walks 2-row x 32-column
// output tiles; a pre-pass over the non-zero bit map of the input (straps_stem_nzmask -> stem_tileact_kernel) tells it --
// before touching LDS, x or dy -- which of its channels hold anything inside the tile's 9 x 72 input patch: most (tile,
// group) pairs are skipped outright (a workgroup fetches the activity of 64 tiles with one load), and inside an active
// pair only the active channels are loaded.
// A skipped contribution is 0 * dy = 0, so the result equals the dense one bit for bit; a dense input skips nothing.
// Per group the accumulator is dW[64][4*49 = 196 taps] = 14 MFMA tiles of 32x32 over the 4 waves (64 accumulator
// registers), so 4-5 workgroups are resident per CU and cover each other's load latency (the all-channel variant needed
// 472 registers: one wave per SIMD).
constexpr int TY = 2, TX = 32, PH = 2 * TY + 5, PW = 72, TPIX = TY * TX;
constexpr int CG = 4, GK = CG * 49, GNB = (GK + 31) / 32, GUNITS = 2 * GNB, UPW = (GUNITS + 3) / 4;   // 196 taps, 7 column blocks, 14 units, 4 per wave

// per (channel group, tile): which of the group's channels have a non-zero inside the tile's 9 x 72 input patch (bit cl)
__global__ __launch_bounds__(256) void stem_tileact_kernel(const unsigned* __restrict__ nzmask, uint8_t* __restrict__ tact, int C, int H, int W,
                                                           int tiles_x, int tiles_y, int ntiles, int groups) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= ntiles * groups) return;
    const int grp = idx / ntiles, tile = idx - grp * ntiles;
    int bid = tile;
    const int b = bid / (tiles_x * tiles_y);
    bid -= b * tiles_x * tiles_y;
    const int ty = bid / tiles_x, tx = bid - ty * tiles_x;
    const int hi0 = 2 * (ty * TY) - 3, wi0 = 2 * (tx * TX) - 3;
    const int HC = (H + 3) >> 2, WW = (W + 255) >> 8;
    const int rc0 = max(hi0, 0) >> 2, rc1 = min(hi0 + PH - 1, H - 1) >> 2;
    const int wa = max(wi0 - 1, 0), wb = min(wi0 - 2 + PW, W - 1);
    const int c0 = grp * CG, nc = min(CG, C - c0);
    unsigned chact = 0;
    for (int cl = 0; cl < nc; ++cl) {
        unsigned any = 0;
        for (int rcell = rc0; rcell <= rc1; ++rcell)
            for (int word = wa >> 8; word <= (wb >> 8); ++word) {
                const int lo = max(wa, word << 8), hi = min(wb, (word << 8) + 255);
                const int b0 = (lo >> 3) & 31, b1 = (hi >> 3) & 31;
                const unsigned bits = (b1 == 31 ? 0xffffffffu : ((1u << (b1 + 1)) - 1u)) & ~((1u << b0) - 1u);
                any |= nzmask[(((long long)b * C + c0 + cl) * HC + rcell) * WW + word] & bits;
            }
        if (any) chact |= 1u << cl;
    }
    tact[idx] = (uint8_t)chact;
}

// per tile: does ANY input channel hold a non-zero inside the tile's input patch (= is the tile of dy read by stem_wgrad_kernel at all).
// 32 lanes per tile, one channel each (a few independent word loads per lane), combined with a ballot.
__global__ __launch_bounds__(256) void stem_tileany_kernel(const unsigned* __restrict__ nzmask, uint8_t* __restrict__ tany, int C, int H, int W,
                                                           int tiles_x, int tiles_y, int ntiles) {
    const int lane = threadIdx.x & 63, sub = lane & 31;
    const int tile = (blockIdx.x * 256 + threadIdx.x) >> 5;
    unsigned any = 0;
    if (tile < ntiles) {
        int bid = tile;
        const int b = bid / (tiles_x * tiles_y);
        bid -= b * tiles_x * tiles_y;
        const int ty = bid / tiles_x, tx = bid - ty * tiles_x;
        const int hi0 = 2 * (ty * TY) - 3, wi0 = 2 * (tx * TX) - 3;
        const int HC = (H + 3) >> 2, WW = (W + 255) >> 8;
        const int rc0 = max(hi0, 0) >> 2, rc1 = min(hi0 + PH - 1, H - 1) >> 2;
        const int wa = max(wi0 - 1, 0), wb = min(wi0 - 2 + PW, W - 1);
        for (int c = sub; c < C; c += 32)
            for (int rcell = rc0; rcell <= rc1; ++rcell)
                for (int word = wa >> 8; word <= (wb >> 8); ++word) {
                    const int lo = max(wa, word << 8), hi = min(wb, (word << 8) + 255);
                    const int b0 = (lo >> 3) & 31, b1 = (hi >> 3) & 31;
                    const unsigned bits = (b1 == 31 ? 0xffffffffu : ((1u << (b1 + 1)) - 1u)) & ~((1u << b0) - 1u);
                    any |= nzmask[(((long long)b * C + c) * HC + rcell) * WW + word] & bits;
                }
    }
    const unsigned long long bal = __ballot(any != 0u);
    const unsigned mine = (unsigned)(bal >> (lane & 32));            // the 32 lanes of this tile
    if (sub == 0 && tile < ntiles) tany[tile] = mine ? 1 : 0;
}

__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         float* __restrict__ part, const uint8_t* __restrict__ tact, int B, int C, int H,
                                                         int W, int Ho, int Wo,
                                                         int tiles_x, int tiles_y, int Kp, int ntiles, int rot) {
    __shared__ __attribute__((aligned(16))) float patch[2 * CG * PH * PW]; // [buffer][cl][PH][PW]
    __shared__ __attribute__((aligned(16))) float dys[2 * TPIX * 68];      // [buffer][pixel][64 + 4]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int c0 = blockIdx.y * CG;
    const int nc = min(CG, C - c0);
    const int gk = nc * 49;                                                // valid taps of this group

    // this wave's units u = wave + 4*j = 2*nb + a: (tap column block nb, co half a); patch offset of this lane's tap; channel span
    int u_a[UPW], u_nb[UPW], u_ko[UPW];
    unsigned u_span[UPW];
#pragma unroll
    for (int j = 0; j < UPW; ++j) {
        const int u = wave + 4 * j;
        u_a[j] = u & 1;                     // consecutive column blocks x both co halves land on 4 different waves: the
        u_nb[j] = u >> 1;                   // 4 units of one active channel (49 taps ~ 1.5 column blocks) run in parallel
        const int k = u_nb[j] * 32 + i;
        int o = 0;
        if (u < GUNITS && k < gk) {
            const int cl = k / 49, rs = k - cl * 49;
            const int r = rs / 7, s_ = rs - r * 7;
            o = (cl * PH + r) * PW + s_ + 1;                               // +1: patch origin one column left of the receptive field
        }
        u_ko[j] = o;
        const int k0 = u_nb[j] * 32;
        u_span[j] = 0;
        if (u < GUNITS && k0 < gk) {
            const int cl0 = k0 / 49, cl1 = min(k0 + 31, gk - 1) / 49;
            u_span[j] = (1u << cl0) | (1u << cl1);
        }
    }
    f32x16 acc[UPW];
#pragma unroll
    for (int j = 0; j < UPW; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;

    // Rotated strided tile assignment (evens out body vs background tiles, see the walk below).  The activity bytes of 64 tiles are fetched with one
    // load and only the active tiles are visited -- in ascending order, so the accumulation order is fixed.  The visit is
    // software-pipelined over a double-buffered LDS: while the MFMAs of tile t run, the global loads of the next active
    // tile are already in flight (registers), and one barrier per tile is enough (a buffer is rewritten two tiles later,
    // after every wave has passed the barrier in between).
    constexpr int PIT = (CG * PH * (PW / 4) + 255) / 256;                  // 3 float4 of the patch per thread
    constexpr int DIT = TPIX * 16 / 256;                                   // 4 float4 of the dy tile per thread
    const bool vec = (W & 3) == 0;
    f32x4 pv[PIT], dv[DIT];
    auto tile_origin = [&](int tile, int& b, int& y0, int& x0) {
        b = tile / (tiles_x * tiles_y);
        const int bid = tile - b * tiles_x * tiles_y;
        const int ty = bid / tiles_x;
        y0 = ty * TY;
        x0 = (bid - ty * tiles_x) * TX;
    };
    auto issue_loads = [&](int tile, unsigned chact) {                     // global -> registers, nothing waits here
        int b, y0, x0;
        tile_origin(tile, b, y0, x0);
        const int hi0 = 2 * y0 - 3, wi0 = 2 * x0 - 3;
#pragma unroll
        for (int it = 0; it < PIT; ++it) {
            const int idx = tid + it * 256;
            const int q = idx % (PW / 4);
            const int rc = idx / (PW / 4);
            const int row = rc % PH, cl = rc / PH;
            const int hi = hi0 + row, wi = wi0 - 1 + 4 * q;                // patch column p holds input column wi0 - 1 + p
            pv[it] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (vec && cl < nc && ((chact >> cl) & 1u) && (unsigned)hi < (unsigned)H && wi >= 0 && wi < W)
                pv[it] = *reinterpret_cast<const f32x4*>(x + (((long long)b * C + c0 + cl) * H + hi) * W + wi);
        }
#pragma unroll
        for (int it = 0; it < DIT; ++it) {
            const int idx = tid + it * 256;
            const int pix = idx >> 4, c4 = idx & 15;
            const int yo = y0 + (pix >> 5), xo = x0 + (pix & 31);
            dv[it] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (yo < Ho && xo < Wo) dv[it] = *reinterpret_cast<const f32x4*>(dy + (((long long)b * Ho + yo) * Wo + xo) * 64 + c4 * 4);
        }
    };
    auto store_tile = [&](int tile, unsigned chact, float* pb, float* db) {        // registers -> LDS buffer
        if (vec) {
#pragma unroll
            for (int it = 0; it < PIT; ++it) {
                const int idx = tid + it * 256;
                if (idx < nc * PH * (PW / 4)) *reinterpret_cast<f32x4*>(pb + (idx / (PW / 4)) * PW + 4 * (idx % (PW / 4))) = pv[it];
            }
        } else {                                                           // odd widths: scalar fill, not pipelined
            int b, y0, x0;
            tile_origin(tile, b, y0, x0);
            const int hi0 = 2 * y0 - 3, wi0 = 2 * x0 - 3;
            for (int idx = tid; idx < nc * PH * PW; idx += 256) {
                const int col = idx % PW;
                const int rc = idx / PW;
                const int row = rc % PH, cl = rc / PH;
                const int hi = hi0 + row, wi = wi0 - 1 + col;
                float v = 0.f;
                if (((chact >> cl) & 1u) && (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W) v = x[(((long long)b * C + c0 + cl) * H + hi) * W + wi];
                pb[idx] = v;
            }
        }
#pragma unroll
        for (int it = 0; it < DIT; ++it) {
            const int idx = tid + it * 256;
            *reinterpret_cast<f32x4*>(db + (idx >> 4) * 68 + (idx & 15) * 4) = dv[it];
        }
    };

    const uint8_t* myact = tact + (long long)blockIdx.y * ntiles;
    int buf = 0;
    // tile walk: "row" m of the tile list holds tiles m*G .. m*G + G - 1 (G = gridDim.x); this workgroup takes element (bx + 97 m) mod G of
    // every row.  With G = tiles per image (the B = 64, 256 x 256 case) a plain bx + m*G would pin a workgroup to ONE image position in all
    // images -- the body sits in the middle of every proxy image, so a quarter of the workgroups would do all the work; the rotation walks
    // each workgroup through the whole image instead.  Any G: a bijection per row, ascending tile order (fixed accumulation order).
    const int G = gridDim.x;
    for (int m0 = 0; (long long)m0 * G < ntiles; m0 += 64) {
        const int m = m0 + lane;
        const long long mine_l = (long long)m * G + (blockIdx.x + (long long)rot * m) % G;
        const int mine = mine_l < ntiles ? (int)mine_l : -1;
        const unsigned act = mine >= 0 ? myact[mine] : 0u;
        unsigned long long todo = __ballot(act != 0u);
        if (todo) {
            const int l0 = __ffsll((long long)todo) - 1;
            issue_loads(__shfl(mine, l0, 64), (unsigned)__shfl((int)act, l0, 64));
        }
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int tile = __shfl(mine, l, 64);
            const unsigned chact = (unsigned)__shfl((int)act, l, 64);
            float* pb = patch + buf * (CG * PH * PW);
            float* db = dys + buf * (TPIX * 68);
            store_tile(tile, chact, pb, db);
            __syncthreads();
            if (todo) {                                                    // next active tile of this chunk: loads fly during the MFMAs
                const int ln = __ffsll((long long)todo) - 1;
                issue_loads(__shfl(mine, ln, 64), (unsigned)__shfl((int)act, ln, 64));
            }
            // contraction over the tile's 64 pixels: A[co][pix] = dys[pix][co], B[pix][k] = patch[koff[k] + 2*py*PW + 2*px].
            // Unit-outer / pixel-inner and fully unrolled: every LDS operand is base + immediate offset (a unit is skipped
            // when its taps read only all-zero channels of this tile -- wave-uniform).
#pragma unroll
            for (int j = 0; j < UPW; ++j) {
                if (!(u_span[j] & chact)) continue;
                const float* ap = db + (h * 4) * 68 + u_a[j] * 32 + i;
                const float* bp = pb + u_ko[j] + 8 * h;
                // all 64 operands of the unit are fetched first (the scheduling barrier keeps the compiler from re-serialising
                // read -> wait -> MFMA pairs through two registers), then the 32-MFMA chain runs without LDS waits
                float av[32], bv[32];
#pragma unroll
                for (int g = 0; g < TPIX / 8; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        av[g * 4 + e] = ap[(g * 8 + e) * 68];
                        bv[g * 4 + e] = bp[(g >> 2) * 2 * PW + (g & 3) * 16 + 2 * e];
                    }
                __builtin_amdgcn_sched_barrier(0);
                f32x16 c = acc[j];
#pragma unroll
                for (int t = 0; t < 32; ++t) c = mfma32(av[t], bv[t], c);
                acc[j] = c;
                __builtin_amdgcn_sched_barrier(0);
            }
            buf ^= 1;
        }
        __syncthreads();          // chunk boundary: the next chunk's first store may target the buffer still being read
    }
    // partial[block][co][k], k = (c0 + cl)*49 + rs: the group's taps are a contiguous column range
    float* o = part + (long long)blockIdx.x * 64 * Kp + c0 * 49;
#pragma unroll
    for (int j = 0; j < UPW; ++j) {
        const int kcol = u_nb[j] * 32 + i;
        if (wave + 4 * j < GUNITS && kcol < gk) {
#pragma unroll
            for (int q = 0; q < 16; ++q) o[(long long)(u_a[j] * 32 + mfma_row(q, lane)) * Kp + kcol] = acc[j][q];
        }
    }
}

// fixed-order sum of the per-block partials: 64 consecutive outputs per workgroup, the four waves take the blocks b = wave, wave + 4, ...
// (independent loads, eight in flight per lane), their four sums are added in wave order -- the same order on every launch.
__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int nblocks,
                                                                int K, int Kp, int accumulate) {
    __shared__ float red[4][64];
    const int o = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int idx = blockIdx.x * 64 + o;              // over [64][K]
    const bool live = idx < 64 * K;
    const int co = live ? idx / K : 0, k = live ? idx - co * K : 0;
    const float* src = part + (long long)co * Kp + k;
    const long long bstride = (long long)64 * Kp;
    float s = 0.f;
    if (live) {
#pragma unroll 8
        for (int b = g; b < nblocks; b += 4) s += src[b * bstride];
    }
    red[g][o] = s;
    __syncthreads();
    if (g == 0 && live) {
        const float t = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
        dw[idx] = accumulate ? dw[idx] + t : t;       // OIHW row co is (c,r,s)-ordered == k
    }
}

// =====================================================================================================
// BatchNorm (training) backward with fused ReLU mask
// =====================================================================================================
// pass 1: per-block partial sums of dz and dz*xhat, dz = dy * (y > 0 if masked).  Block (bx, by) owns rows
// [bx*rows_per_block, ...) x the 64 channels [64*by, 64*by+64): 16 float4 column lanes x 16 row lanes, so a deep layer
// (few rows, many channels) still fills the chip, and every wave load is 4 full 256-byte row segments.
// ReLU mask: (yact > 0), or -- when the activation is exactly relu(raw*msc + msh), no residual -- recomputed from raw
// with the forward's own fmaf (bit-identical to reading yact, one tensor read less).
//
// POOL variants (the stem's BatchNorm, whose output only feeds the 3x3/s2 max-pool): the incoming gradient is never materialised --
// each element gathers it from the <= 4 pooling windows that cover it, in the order straps_maxpool_bwd uses (bit-identical).
struct PoolSrc {
    const float* dyp;       // [B][Ho][Wo][C] gradient of the pooled tensor
    const uint8_t* idx;     // [B][Ho][Wo][C] arg-max tap of every window
    int H, W, Ho, Wo;
    // optional (the stem): tany[(b * tiles_y + h / 2) * tiles_x + w / 32] == 0 marks a 2-row x 32-column tile of the un-pooled grid whose
    // gradient nobody reads (the stem weight gradient skips it: no non-zero input under it) -- the apply pass leaves it unwritten
    const uint8_t* tany;
    int tiles_x, tiles_y;
};

__device__ __forceinline__ f32x4 pool_grad(const PoolSrc& ps, long long row, int c4, int C) {
    const int wi = (int)(row % ps.W);
    const long long t = row / ps.W;
    const int hi = (int)(t % ps.H);
    const long long b = t / ps.H;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    const int ho_lo = hi >> 1, ho_hi = (hi + 1) >> 1;        // windows (ho,wo) with 2*ho-1 <= hi <= 2*ho+1
    const int wo_lo = wi >> 1, wo_hi = (wi + 1) >> 1;
    for (int ho = ho_lo; ho <= ho_hi; ++ho) {
        if (ho >= ps.Ho) continue;
        const int r = hi - (2 * ho - 1);
        for (int wo = wo_lo; wo <= wo_hi; ++wo) {
            if (wo >= ps.Wo) continue;
            const int want = r * 3 + wi - (2 * wo - 1);
            const long long o = ((b * ps.Ho + ho) * ps.Wo + wo) * C + c4 * 4;
            const uchar4 k = *reinterpret_cast<const uchar4*>(ps.idx + o);
            const f32x4 d = *reinterpret_cast<const f32x4*>(ps.dyp + o);
            if (k.x == want) g[0] += d[0];
            if (k.y == want) g[1] += d[1];
            if (k.z == want) g[2] += d[2];
            if (k.w == want) g[3] += d[3];
        }
    }
    return g;
}

// The three BatchNorm-backward kernels accumulate and subtract in DOUBLE: in the last stage the gradient that reaches a BatchNorm
// is almost constant per channel (global average pooling broadcasts one value to the 64 positions), so dz - mean(dz) cancels to
// rounding noise of fp32 sums -- measured 4e-4..2e-3 relative on the layer4 gradients against 2e-6 for the reference's CPU path,
// whose BatchNorm backward accumulates in double (ATen acc_type<float, cpu>).  The passes are HBM-bound; the fp64 VALU work is free.
template <bool POOL>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ yact,
                                                            const float* __restrict__ raw, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ msc,
                                                            const float* __restrict__ msh, double* __restrict__ part, long long rows,
                                                            int C, int rows_per_block, PoolSrc ps, const unsigned* __restrict__ bits) {
    // (bits: the ReLU decisions of yact as one word per (row, 32 channels) -- straps_bn_apply_bits_x3 -- read instead of yact itself)
    __shared__ double red[256][8];
    constexpr int TR = 16;
    const int tc = threadIdx.x & 15, tr = threadIdx.x >> 4;
    const int c4 = blockIdx.y * 16 + tc;
    const bool active = c4 * 4 < C;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};       // s2 = sum g * (x - mean); invstd is applied once at the end
    f32x4 is = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c4 * 4);
        is = *reinterpret_cast<const f32x4*>(invstd + c4 * 4);
        f32x4 ksc = {0.f, 0.f, 0.f, 0.f}, ksh = ksc;
        if (msc) { ksc = *reinterpret_cast<const f32x4*>(msc + c4 * 4); ksh = *reinterpret_cast<const f32x4*>(msh + c4 * 4); }
        // 4 rows per trip: 8-12 independent float4 loads in flight per lane before the first use
        long long r = r0 + tr;
        for (; r + 3 * TR < r1; r += 4 * TR) {
            f32x4 g[4], ya[4], xr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long o = (r + (long long)u * TR) * C + c4 * 4;
                if constexpr (POOL) g[u] = pool_grad(ps, r + (long long)u * TR, c4, C);
                else g[u] = *reinterpret_cast<const f32x4*>(dy + o);
                xr[u] = *reinterpret_cast<const f32x4*>(raw + o);
                if (bits) ya[u][0] = __uint_as_float(bits[(r + (long long)u * TR) * (C >> 5) + (c4 >> 3)]);
                else if (yact) ya[u] = *reinterpret_cast<const f32x4*>(yact + o);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (bits) {
                    const unsigned nib = __float_as_uint(ya[u][0]) >> ((c4 & 7) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[u][e] = ((nib >> e) & 1u) ? g[u][e] : 0.f;
                } else if (yact) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[u][e] = ya[u][e] > 0.f ? g[u][e] : 0.f;
                } else if (msc) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[u][e] = fmaf(xr[u][e], ksc[e], ksh[e]) > 0.f ? g[u][e] : 0.f;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s1[e] += (double)g[u][e];
                    s2[e] += (double)g[u][e] * ((double)xr[u][e] - (double)mu[e]);
                }
            }
        }
        for (; r < r1; r += TR) {
            const long long o = r * C + c4 * 4;
            f32x4 g;
            if constexpr (POOL) g = pool_grad(ps, r, c4, C);
            else g = *reinterpret_cast<const f32x4*>(dy + o);
            const f32x4 xr = *reinterpret_cast<const f32x4*>(raw + o);
            if (bits) {
                const unsigned nib = bits[r * (C >> 5) + (c4 >> 3)] >> ((c4 & 7) * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = ((nib >> e) & 1u) ? g[e] : 0.f;
            } else if (yact) {
                const f32x4 ya = *reinterpret_cast<const f32x4*>(yact + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = ya[e] > 0.f ? g[e] : 0.f;
            } else if (msc) {
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = fmaf(xr[e], ksc[e], ksh[e]) > 0.f ? g[e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s1[e] += (double)g[e];
                s2[e] += (double)g[e] * ((double)xr[e] - (double)mu[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[threadIdx.x][e] = s1[e]; red[threadIdx.x][4 + e] = s2[e] * (double)is[e]; }
    __syncthreads();
    if (tr == 0 && active) {
        double t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = red[tc][e];
        for (int q = 1; q < TR; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) t[e] += red[q * 16 + tc][e];
        double* o = part + ((long long)blockIdx.x * C + c4 * 4) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e * 2 + 0] = t[e]; o[e * 2 + 1] = t[4 + e]; }
    }
}

// The same sums for the fused stem tail (bn1 + ReLU + max-pool), taken over the POOLED grid: every pooled element routes its gradient to
// exactly one un-pooled position (its arg-max tap), so  S1 = sum_q mask * dy_q,  S2 = sum_q mask * dy_q * (x[argmax(q)] - mean) --
// a quarter of the elements of the un-pooled sweep, one gathered raw value each, no four-window search per element.
// (mask = the ReLU derivative at the arg-max position, re-derived from raw like everywhere else.)
__global__ __launch_bounds__(256) void bn_bwd_reduce_pooled_kernel(const float* __restrict__ raw, const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd, const float* __restrict__ msc,
                                                                   const float* __restrict__ msh, double* __restrict__ part, long long prows,
                                                                   int C, int rows_per_block, PoolSrc ps) {
    __shared__ double red[256][8];
    constexpr int TR = 16;
    const int tc = threadIdx.x & 15, tr = threadIdx.x >> 4;
    const int c4 = blockIdx.y * 16 + tc;
    const bool active = c4 * 4 < C;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < prows ? r0 + rows_per_block : prows;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    f32x4 is = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c4 * 4);
        is = *reinterpret_cast<const f32x4*>(invstd + c4 * 4);
        const f32x4 ksc = *reinterpret_cast<const f32x4*>(msc + c4 * 4), ksh = *reinterpret_cast<const f32x4*>(msh + c4 * 4);
        for (long long r = r0 + tr; r < r1; r += TR) {
            const int wo = (int)(r % ps.Wo);
            const long long t = r / ps.Wo;
            const int ho = (int)(t % ps.Ho);
            const long long b = t / ps.Ho;
            const long long o = r * C + c4 * 4;
            const f32x4 d = *reinterpret_cast<const f32x4*>(ps.dyp + o);
            const uchar4 k4 = *reinterpret_cast<const uchar4*>(ps.idx + o);
            const int k[4] = {k4.x, k4.y, k4.z, k4.w};
            float xr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int hi = 2 * ho - 1 + k[e] / 3, wi = 2 * wo - 1 + k[e] % 3;          // (the recorded tap lies inside the image)
                xr[e] = raw[((b * ps.H + hi) * ps.W + wi) * C + c4 * 4 + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = fmaf(xr[e], ksc[e], ksh[e]) > 0.f ? d[e] : 0.f;
                s1[e] += (double)g;
                s2[e] += (double)g * ((double)xr[e] - (double)mu[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[threadIdx.x][e] = s1[e]; red[threadIdx.x][4 + e] = s2[e] * (double)is[e]; }
    __syncthreads();
    if (tr == 0 && active) {
        double t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = red[tc][e];
        for (int q = 1; q < TR; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) t[e] += red[q * 16 + tc][e];
        double* o = part + ((long long)blockIdx.x * C + c4 * 4) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e * 2 + 0] = t[e]; o[e * 2 + 1] = t[4 + e]; }
    }
}

// per channel: dbeta = S1, dgamma = S2; coefficients for the apply pass: k1 = gamma*invstd (float), m1 = S1/N, m2 = S2/N (double)
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ part, int nblocks, int C, double count,
                                                             const float* __restrict__ gamma, const float* __restrict__ invstd,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                             double* __restrict__ coefd, float* __restrict__ k1, int accumulate) {
    int c;
    double s1, s2;
    if (bn_partials_sum4(part, nblocks, C, s1, s2, c)) {
        dbeta[c] = accumulate ? dbeta[c] + (float)s1 : (float)s1;
        dgamma[c] = accumulate ? dgamma[c] + (float)s2 : (float)s2;
        k1[c] = gamma[c] * invstd[c];
        coefd[c] = s1 / count;
        coefd[C + c] = s2 / count;
    }
}

// pass 2: draw = k1 * (dz - m1 - xhat*m2), evaluated in double and rounded once;  optionally also writes dz (the gradient the
// skip connection receives)
constexpr int POOL_CHUNK = 1024;        // float4 elements per workgroup of the pooled apply pass (64 pixels of a 64-channel tensor)
template <bool POOL>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ yact,
                                                           const float* __restrict__ raw, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const double* __restrict__ coefd,
                                                           const float* __restrict__ k1p, const float* __restrict__ msc,
                                                           const float* __restrict__ msh, float* __restrict__ draw, float* dz_out,
                                                           u16* __restrict__ planes, long long pstride, long long n4, int C, PoolSrc ps,
                                                           const unsigned* __restrict__ bits, int tiled) {
    const int C4 = C >> 2;
    // POOL: a workgroup owns POOL_CHUNK consecutive elements (with the tile map most workgroups of an empty region exit at once and the
    // dispatcher hands out the rest: a grid-stride loop would pin every workgroup to one image position -- all work or none)
    const long long first = POOL ? (long long)blockIdx.x * POOL_CHUNK + threadIdx.x : (long long)blockIdx.x * 256 + threadIdx.x;
    const long long last = POOL ? (n4 < ((long long)blockIdx.x + 1) * POOL_CHUNK ? n4 : ((long long)blockIdx.x + 1) * POOL_CHUNK) : n4;
    const long long step = POOL ? 256 : (long long)gridDim.x * 256;
    const long long rows = n4 / C4;
    // per-channel constants of four channels: 5 float4 + 8 doubles.  Round 4: when the loop stride is a multiple of the row length (the host
    // sizes the grid so; always for the pooled form's 256-element stride on 64 channels) a thread keeps its four channels for the whole loop
    // and loads them ONCE -- they were 144 bytes of L1 traffic per 48-64 bytes of payload -- and the row index advances by a constant
    // instead of a 64-bit division per element.  Same arithmetic either way.
    struct Consts { f32x4 ksc, ksh, mu, is, k1; double m1[4], m2[4]; };
    auto load_consts = [&](int c4) {
        Consts k;
        if (!yact && !bits && msc) { k.ksc = *reinterpret_cast<const f32x4*>(msc + c4 * 4); k.ksh = *reinterpret_cast<const f32x4*>(msh + c4 * 4); }
        k.mu = *reinterpret_cast<const f32x4*>(mean + c4 * 4);
        k.is = *reinterpret_cast<const f32x4*>(invstd + c4 * 4);
        k.k1 = *reinterpret_cast<const f32x4*>(k1p + c4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { k.m1[e] = coefd[c4 * 4 + e]; k.m2[e] = coefd[C + c4 * 4 + e]; }
        return k;
    };
    auto body = [&](long long idx, long long row, int c4, const Consts& k) {
        f32x4 g;
        if constexpr (POOL) {
            if (ps.tany) {
                const int wi = (int)(row % ps.W);
                const long long t = row / ps.W;
                const int hi = (int)(t % ps.H);
                const long long b = t / ps.H;
                if (!ps.tany[(b * ps.tiles_y + (hi >> 1)) * ps.tiles_x + (wi >> 5)]) return;
            }
            g = pool_grad(ps, row, c4, C);
        } else {
            g = *reinterpret_cast<const f32x4*>(dy + idx * 4);
        }
        const f32x4 xr = *reinterpret_cast<const f32x4*>(raw + idx * 4);
        if (bits) {      // (ReLU decisions of yact as bits: word [row][C / 32], bit c & 31 -- straps_bn_apply_bits_x3)
            const unsigned nib = bits[row * (C >> 5) + (c4 >> 3)] >> ((c4 & 7) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = ((nib >> e) & 1u) ? g[e] : 0.f;
        } else if (yact) {
            const f32x4 ya = *reinterpret_cast<const f32x4*>(yact + idx * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = ya[e] > 0.f ? g[e] : 0.f;
        } else if (msc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = fmaf(xr[e], k.ksc[e], k.ksh[e]) > 0.f ? g[e] : 0.f;
        }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double xh = ((double)xr[e] - (double)k.mu[e]) * (double)k.is[e];
            o[e] = (float)((double)k.k1[e] * (((double)g[e] - k.m1[e]) - xh * k.m2[e]));
        }
        if (dz_out) *reinterpret_cast<f32x4*>(dz_out + idx * 4) = g;
        if (draw) *reinterpret_cast<f32x4*>(draw + idx * 4) = o;      // (NULL: only the planes are consumed, see straps_bn_bwd_x3)
        if (planes) store_planes4_cm(planes, pstride, row, c4 * 4, rows, o);      // bf16x3 route: the data-gradient kernel's operand (chunk-major planes)
    };
    if (!POOL && tiled) {
        // a wave = 4 rows x 2 chunks of 32 channels: whole 256-byte runs of every chunk-major plane per wave store; `tiled` = the column
        // groups of 64 channels the workgroup's waves sit on side by side (bn_apply_kernel's tiled form, csrc/elementwise.hip; the host
        // passes it only for row / channel counts that tile exactly, with a grid that is a multiple of the column blocks)
        const int l = threadIdx.x & 63, w = threadIdx.x >> 6, wcg = tiled, ncb = (C4 >> 4) / wcg, trows = 16 / wcg;
        const int c4 = ((int)(blockIdx.x % ncb) * wcg + w % wcg) * 16 + (l >> 5) * 8 + (l & 7);
        const Consts k = load_consts(c4);
        const long long rstep = (long long)(gridDim.x / ncb) * trows;
        for (long long row = (long long)(blockIdx.x / ncb) * trows + (w / wcg) * 4 + ((l >> 3) & 3); row < rows; row += rstep) body(row * C4 + c4, row, c4, k);
    } else if (step % C4 == 0) {
        if (first >= last) return;
        const int c4 = (int)(first % C4);
        const Consts k = load_consts(c4);
        const long long rstep = step / C4;
        long long row = first / C4;
        for (long long idx = first; idx < last; idx += step, row += rstep) body(idx, row, c4, k);
    } else {
        for (long long idx = first; idx < last; idx += step) {
            const int c4 = (int)(idx % C4);
            body(idx, idx / C4, c4, load_consts(c4));
        }
    }
}

// =====================================================================================================
// pooling backward
// =====================================================================================================
// training-mode max-pool: also records the arg-max tap (first maximum in row-major scan order, like ATen)
__global__ __launch_bounds__(256) void maxpool_idx_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ idx,
                                                          int B, int H, int W, int C, int Ho, int Wo) {
    const int C4 = C >> 2;
    const long long n = (long long)B * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        long long t = i / C4;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho);
        const int b = (int)(t / Ho);
        f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int am[4] = {0, 0, 0, 0};
        bool first = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int hi = 2 * ho - 1 + r;
            if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int wi = 2 * wo - 1 + s;
                if ((unsigned)wi >= (unsigned)W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((long long)b * H + hi) * W + wi) * C + c4 * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (first || v[e] > m[e] || v[e] != v[e]) { m[e] = v[e]; am[e] = r * 3 + s; }
                first = false;
            }
        }
        *reinterpret_cast<f32x4*>(y + i * 4) = m;
        *reinterpret_cast<uchar4*>(idx + i * 4) = make_uchar4((unsigned char)am[0], (unsigned char)am[1], (unsigned char)am[2], (unsigned char)am[3]);
    }
}

// training-mode stem tail: max-pool 3x3/s2/p1 of y = relu(raw*scale + shift) straight from raw -- y itself is never written (the
// backward re-derives the ReLU mask from raw and gathers the pooled gradient, straps_bn_bwd_pooled).  Same fmaf / fmaxf / compare
// sequence as straps_bn_apply followed by straps_maxpool_fwd_idx: bit-identical outputs and arg-max taps.
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const float* __restrict__ raw, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, float* __restrict__ y, uint8_t* __restrict__ idx,
                                                              u16* __restrict__ planes, long long pstride, int B, int H, int W, int C, int Ho, int Wo) {
    const int C4 = C >> 2;
    const long long n = (long long)B * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        long long t = i / C4;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho);
        const int b = (int)(t / Ho);
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c4 * 4);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + c4 * 4);
        f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int am[4] = {0, 0, 0, 0};
        bool first = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int hi = 2 * ho - 1 + r;
            if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int wi = 2 * wo - 1 + s;
                if ((unsigned)wi >= (unsigned)W) continue;
                f32x4 v = *reinterpret_cast<const f32x4*>(raw + (((long long)b * H + hi) * W + wi) * C + c4 * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f);
                    if (first || v[e] > m[e] || v[e] != v[e]) { m[e] = v[e]; am[e] = r * 3 + s; }
                }
                first = false;
            }
        }
        *reinterpret_cast<f32x4*>(y + i * 4) = m;
        *reinterpret_cast<uchar4*>(idx + i * 4) = make_uchar4((unsigned char)am[0], (unsigned char)am[1], (unsigned char)am[2], (unsigned char)am[3]);
        if (planes) store_planes4_cm(planes, pstride, i / C4, c4 * 4, (long long)B * Ho * Wo, m);
    }
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                          float* __restrict__ dx, int B, int H, int W, int C, int Ho, int Wo) {
    const int C4 = C >> 2;
    const long long n = (long long)B * H * W * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        long long t = i / C4;
        const int wi = (int)(t % W); t /= W;
        const int hi = (int)(t % H);
        const int b = (int)(t / H);
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        // windows (ho,wo) with 2*ho-1 <= hi <= 2*ho+1
        const int ho_lo = hi >> 1, ho_hi = (hi + 1) >> 1;
        const int wo_lo = wi >> 1, wo_hi = (wi + 1) >> 1;
        for (int ho = ho_lo; ho <= ho_hi; ++ho) {
            if (ho >= Ho) continue;
            const int r = hi - (2 * ho - 1);
            for (int wo = wo_lo; wo <= wo_hi; ++wo) {
                if (wo >= Wo) continue;
                const int s = wi - (2 * wo - 1);
                const long long o = (((long long)b * Ho + ho) * Wo + wo) * C + c4 * 4;
                const uchar4 k = *reinterpret_cast<const uchar4*>(idx + o);
                const f32x4 d = *reinterpret_cast<const f32x4*>(dy + o);
                const int want = r * 3 + s;
                if (k.x == want) g[0] += d[0];
                if (k.y == want) g[1] += d[1];
                if (k.z == want) g[2] += d[2];
                if (k.w == want) g[3] += d[3];
            }
        }
        *reinterpret_cast<f32x4*>(dx + i * 4) = g;
    }
}

__global__ __launch_bounds__(256) void gap_bwd_kernel(const float* __restrict__ dfeat, float* __restrict__ dx, int B, int HW, int C) {
    const long long n = (long long)B * HW * C;
    const float inv = 1.0f / (float)HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long b = i / ((long long)HW * C);
        dx[i] = dfeat[b * C + c] * inv;
    }
}

// elementwise: y = x * (mask > 0) (+ y)
__global__ __launch_bounds__(256) void masked_copy_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ mask, int ldm,
                                                          float* y, int ldy, int M, int N, int accumulate) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)M * N) return;
    const int m = (int)(i / N), n = (int)(i - (long long)m * N);
    float v = x[(long long)m * ldx + n];
    if (mask) v = mask[(long long)m * ldm + n] > 0.f ? v : 0.f;
    float* o = y + (long long)m * ldy + n;
    *o = accumulate ? *o + v : v;
}

// =====================================================================================================
// rot6d backward (utils/rigid_transform_utils.py:27-41 differentiated by hand)
// =====================================================================================================
__global__ __launch_bounds__(256) void rot6d_bwd_kernel(const float* __restrict__ x6, long long ld, int per_row,
                                                        const float* __restrict__ dR, float* __restrict__ dx6, long long ldd,
                                                        long long n) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const long long row = idx / per_row;
    const int j = (int)(idx - row * per_row);
    const float* x = x6 + row * ld + j * 6;
    const float a1[3] = {x[0], x[2], x[4]}, a2[3] = {x[1], x[3], x[5]};
    const float* g = dR + idx * 9;                 // dL/dR, R columns = (b1,b2,b3)
    float gb1[3] = {g[0], g[3], g[6]}, gb2[3] = {g[1], g[4], g[7]};
    const float gb3[3] = {g[2], g[5], g[8]};
    const float n1r = sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
    const float n1 = fmaxf(n1r, 1e-12f);
    const float b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
    const float d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    const float u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    const float n2r = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const float n2 = fmaxf(n2r, 1e-12f);
    const float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    // b3 = b1 x b2:  gb1 += b2 x gb3, gb2 += gb3 x b1
    gb1[0] += b2[1] * gb3[2] - b2[2] * gb3[1];
    gb1[1] += b2[2] * gb3[0] - b2[0] * gb3[2];
    gb1[2] += b2[0] * gb3[1] - b2[1] * gb3[0];
    gb2[0] += gb3[1] * b1[2] - gb3[2] * b1[1];
    gb2[1] += gb3[2] * b1[0] - gb3[0] * b1[2];
    gb2[2] += gb3[0] * b1[1] - gb3[1] * b1[0];
    // b2 = u / max(|u|, eps)
    float gu[3];
    if (n2r > 1e-12f) {
        const float t = b2[0] * gb2[0] + b2[1] * gb2[1] + b2[2] * gb2[2];
#pragma unroll
        for (int e = 0; e < 3; ++e) gu[e] = (gb2[e] - b2[e] * t) / n2;
    } else {
#pragma unroll
        for (int e = 0; e < 3; ++e) gu[e] = gb2[e] / n2;
    }
    // u = a2 - d*b1, d = b1.a2
    const float gd = -(gu[0] * b1[0] + gu[1] * b1[1] + gu[2] * b1[2]);
    float ga2[3], ga1[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        ga2[e] = gu[e] + gd * b1[e];
        gb1[e] += -d * gu[e] + gd * a2[e];
    }
    // b1 = a1 / max(|a1|, eps)
    if (n1r > 1e-12f) {
        const float t = b1[0] * gb1[0] + b1[1] * gb1[1] + b1[2] * gb1[2];
#pragma unroll
        for (int e = 0; e < 3; ++e) ga1[e] = (gb1[e] - b1[e] * t) / n1;
    } else {
#pragma unroll
        for (int e = 0; e < 3; ++e) ga1[e] = gb1[e] / n1;
    }
    float* o = dx6 + row * ldd + j * 6;
    o[0] = ga1[0]; o[1] = ga2[0]; o[2] = ga1[1]; o[3] = ga2[1]; o[4] = ga1[2]; o[5] = ga2[2];
}

inline unsigned capped_grid(long long n) {
    long long g = (n + 255) / 256;
    return (unsigned)(g > 256 * 16 ? 256 * 16 : (g < 1 ? 1 : g));
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
// row blocks of tiles (grid.x): enough for 4-5 resident workgroups per CU across the channel groups, few enough that the
// per-block partials stay small
static int stem_wgrad_blocks(int ntiles) {
    static const int cap = STRAPS_TOOL_ENV_INT("STRAPS_STEM_WGRAD_BLOCKS", 256);      // (A/B switch for tools)
    return ntiles < cap ? ntiles : cap;
}

extern "C" size_t straps_stem_wgrad_workspace_bytes(int batch, int cin, int h, int w) {
    const int Ho = (h - 1) / 2 + 1, Wo = (w - 1) / 2 + 1;
    const int ntiles = batch * ((Ho + TY - 1) / TY) * ((Wo + TX - 1) / TX);
    const int Kp = (cin * 49 + 31) / 32 * 32;
    // partials + room for an internally computed non-zero map (used when the caller passes none)
    const size_t groups = (cin + CG - 1) / CG;
    return (size_t)stem_wgrad_blocks(ntiles) * 64 * Kp * sizeof(float) + straps_stem_nzmask_words(batch, cin, h, w) * sizeof(uint32_t) +
           ((groups * ntiles + 3) & ~(size_t)3);
}

extern "C" int straps_stem_wgrad(const float* x_nchw, const float* dy_nhwc, float* dw_oihw, void* workspace, const uint32_t* nzmask,
                                 int batch, int cin, int h, int w, int accumulate, void* stream) {
    STRAPS_REQUIRE(x_nchw && dy_nhwc && dw_oihw && workspace, "straps_stem_wgrad: null pointer");
    STRAPS_REQUIRE(batch > 0 && cin > 0 && h >= 7 && w >= 7, "straps_stem_wgrad: bad shape B=%d C=%d H=%d W=%d", batch, cin, h, w);
    const int K = cin * 49, Kp = (K + 31) / 32 * 32;
    const int Ho = (h - 1) / 2 + 1, Wo = (w - 1) / 2 + 1;
    const int tiles_x = (Wo + TX - 1) / TX, tiles_y = (Ho + TY - 1) / TY;
    const int ntiles = batch * tiles_x * tiles_y;
    const int nblk = stem_wgrad_blocks(ntiles);
    const int groups = (cin + CG - 1) / CG;
    STRAPS_REQUIRE(groups <= 65535, "straps_stem_wgrad: too many input channels (%d)", cin);
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    uint32_t* own = (uint32_t*)(part + (size_t)nblk * 64 * Kp);
    uint8_t* tact = (uint8_t*)(own + straps_stem_nzmask_words(batch, cin, h, w));
    if (!nzmask) {
        const int rc = straps_stem_nzmask(x_nchw, own, batch, cin, h, w, stream);
        if (rc != STRAPS_OK) return rc;
        nzmask = own;
    }
    // (every (block, group) writes its whole column slice at the end, skipped tiles or not; padded columns are never read)
    hipLaunchKernelGGL(stem_tileact_kernel, dim3((ntiles * groups + 255) / 256), dim3(256), 0, st, nzmask, tact, cin, h, w, tiles_x, tiles_y, ntiles,
                       groups);
    STRAPS_CHECK_LAUNCH("stem_tileact_kernel");
    static const int rot = STRAPS_TOOL_ENV_INT("STRAPS_STEM_WGRAD_ROT", 97);      // (A/B switch for tools: 0 = plain strided walk)
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3(nblk, groups), dim3(256), 0, st, x_nchw, dy_nhwc, part, tact, batch, cin, h, w, Ho, Wo,
                       tiles_x, tiles_y, Kp, ntiles, rot);
    STRAPS_CHECK_LAUNCH("stem_wgrad_kernel");
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3((64 * K + 63) / 64), dim3(256), 0, st, (const float*)workspace, dw_oihw, nblk, K, Kp, accumulate);
    STRAPS_CHECK_LAUNCH("stem_wgrad_reduce_kernel");
    return STRAPS_OK;
}

// `accumulate` of the BatchNorm-backward entry points is a flag word: bit 0 = add to dgamma / dbeta instead of overwriting them, bit 1 =
// FROZEN statistics (eval-mode BatchNorm: mean / invstd are the running statistics, constants of the graph -- the two mean terms of
// the training-mode formula vanish: draw = gamma * invstd * dz).  Implemented as an infinite element count: m1 = S1 / N = 0, m2 = S2 / N = 0,
// dgamma = S2 and dbeta = S1 unchanged.
static double bn_bwd_count(long long rows, int flags) { return (flags & 2) ? (double)INFINITY : (double)rows; }

// row blocks of the reduction pass: ~2048 blocks in total over (row blocks x 64-channel column blocks), >= 64 rows each
extern "C" int straps_bn_bwd_blocks(long long rows, int c) {
    const int colblocks = (c + 63) / 64;
    long long b = 2048 / colblocks;
    const long long cap = (rows + 63) / 64;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}

static int bn_bwd_x3_impl(const float* dy, const float* yact, const unsigned* relu_bits, const float* raw, const float* save_mean, const float* save_invstd,
                          const float* gamma, const float* mask_scale, const float* mask_shift, float* dgamma, float* dbeta, float* draw,
                          float* dz_out, unsigned short* draw_planes, long long plane_stride, void* workspace, long long rows, int c,
                          int accumulate, void* stream) {
    STRAPS_REQUIRE(!relu_bits || (!yact && (c & 31) == 0), "straps_bn_bwd_bits_x3: the bits replace yact (and need c %% 32 == 0; c=%d)", c);
    STRAPS_REQUIRE(!draw_planes || (plane_stride >= rows * c && plane_stride % 8 == 0), "straps_bn_bwd_x3: plane_stride must be >= rows*c and a multiple of 8");
    STRAPS_REQUIRE(!draw_planes || (c & 31) == 0, "straps_bn_bwd_x3: chunk-major planes need c %% 32 == 0 (c=%d)", c);
    STRAPS_REQUIRE(dy && raw && save_mean && save_invstd && gamma && dgamma && dbeta && (draw || draw_planes) && workspace, "straps_bn_bwd: null pointer");
    STRAPS_REQUIRE(rows > 0 && c > 0 && (c & 3) == 0, "straps_bn_bwd: bad shape rows=%lld c=%d", rows, c);
    const int C4 = c >> 2;
    STRAPS_REQUIRE(C4 <= 256 ? (256 % C4 == 0) : (C4 % 256 == 0), "straps_bn_bwd: channel count %d not supported", c);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = straps_bn_bwd_blocks(rows, c);
    const int rpb = (int)((rows + nblk - 1) / nblk);
    double* part = (double*)workspace;               // [nblk][c][2]
    double* coefd = part + (size_t)nblk * c * 2;     // [2][c]  m1, m2
    float* k1 = (float*)(coefd + 2 * (size_t)c);     // [c]
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, dim3(nblk, (c + 63) / 64), dim3(256), 0, st, dy, yact, raw, save_mean, save_invstd, mask_scale, mask_shift, part, rows, c, rpb, PoolSrc{}, relu_bits);
    STRAPS_CHECK_LAUNCH("bn_bwd_reduce_kernel");
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((c + 3) / 4), dim3(256), 0, st, part, nblk, c, bn_bwd_count(rows, accumulate), gamma, save_invstd, dgamma, dbeta, coefd, k1, accumulate & 1);
    STRAPS_CHECK_LAUNCH("bn_bwd_finalize_kernel");
    const long long n4 = rows * C4;
    const int tiled = straps_bn_tiled(rows, c >> 2);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(tiled ? straps_bn_tiled_grid(rows, c >> 2, tiled) : straps_grid256_rows(n4, c >> 2)), dim3(256), 0, st, dy, yact, raw, save_mean, save_invstd, coefd, k1, mask_scale, mask_shift, draw, dz_out, draw_planes, plane_stride, n4, c, PoolSrc{}, relu_bits, tiled);
    STRAPS_CHECK_LAUNCH("bn_bwd_apply_kernel");
    return STRAPS_OK;
}

// straps_bn_bwd_x3 when the two sums already exist as per-tile partials [nblk][c][2] (S1, invstd * S2) -- written by
// straps_conv_dgrad_x3_bn, the data-gradient launch that produced dy: finalize + apply only, no pass over (dy, raw) for the sums.
// workspace: (2 c) doubles + c floats.
extern "C" int straps_bn_bwd_x3(const float* dy, const float* yact, const float* raw, const float* save_mean, const float* save_invstd,
                                const float* gamma, const float* mask_scale, const float* mask_shift, float* dgamma, float* dbeta, float* draw,
                                float* dz_out, unsigned short* draw_planes, long long plane_stride, void* workspace, long long rows, int c,
                                int accumulate, void* stream) {
    return bn_bwd_x3_impl(dy, yact, nullptr, raw, save_mean, save_invstd, gamma, mask_scale, mask_shift, dgamma, dbeta, draw, dz_out, draw_planes,
                          plane_stride, workspace, rows, c, accumulate, stream);
}

// straps_bn_bwd_x3 with the ReLU mask as bits: relu_bits [rows][c / 32] (bit ch & 31 of word [row][ch / 32] = activation > 0, written by
// straps_bn_apply_bits_x3) takes the place of the fp32 activation `yact` -- 4 bytes per element less in each of the two passes.  There is no
// dz_out: the consumers of the masked gradient apply the same bits to dy themselves (straps_conv_dgrad_x3_bits / _bn_bits: addend_bits).
extern "C" int straps_bn_bwd_bits_x3(const float* dy, const unsigned* relu_bits, const float* raw, const float* save_mean, const float* save_invstd,
                                     const float* gamma, float* dgamma, float* dbeta, float* draw, unsigned short* draw_planes, long long plane_stride,
                                     void* workspace, long long rows, int c, int accumulate, void* stream) {
    STRAPS_REQUIRE(relu_bits, "straps_bn_bwd_bits_x3: null bit mask");
    return bn_bwd_x3_impl(dy, nullptr, relu_bits, raw, save_mean, save_invstd, gamma, nullptr, nullptr, dgamma, dbeta, draw, nullptr, draw_planes,
                          plane_stride, workspace, rows, c, accumulate, stream);
}

static int bn_bwd_finish_x3_impl(const float* dy, const float* yact, const unsigned* relu_bits, const float* raw, const float* save_mean,
                                 const float* save_invstd, const float* gamma, const float* mask_scale, const float* mask_shift, float* dgamma,
                                 float* dbeta, float* draw, float* dz_out, unsigned short* draw_planes, long long plane_stride, const double* partials,
                                 int nblk, void* workspace, long long rows, int c, int accumulate, void* stream) {
    STRAPS_REQUIRE(!relu_bits || (!yact && (c & 31) == 0), "straps_bn_bwd_finish_bits_x3: the bits replace yact (and need c %% 32 == 0; c=%d)", c);
    STRAPS_REQUIRE(!draw_planes || (plane_stride >= rows * c && plane_stride % 8 == 0), "straps_bn_bwd_finish_x3: plane_stride must be >= rows*c and a multiple of 8");
    STRAPS_REQUIRE(!draw_planes || (c & 31) == 0, "straps_bn_bwd_finish_x3: chunk-major planes need c %% 32 == 0 (c=%d)", c);
    STRAPS_REQUIRE(dy && raw && save_mean && save_invstd && gamma && dgamma && dbeta && (draw || draw_planes) && workspace && partials && nblk > 0,
                   "straps_bn_bwd_finish_x3: null pointer");
    STRAPS_REQUIRE(rows > 0 && c > 0 && (c & 3) == 0, "straps_bn_bwd_finish_x3: bad shape rows=%lld c=%d", rows, c);
    const int C4 = c >> 2;
    STRAPS_REQUIRE(C4 <= 256 ? (256 % C4 == 0) : (C4 % 256 == 0), "straps_bn_bwd_finish_x3: channel count %d not supported", c);
    hipStream_t st = (hipStream_t)stream;
    double* coefd = (double*)workspace;              // [2][c]  m1, m2
    float* k1 = (float*)(coefd + 2 * (size_t)c);     // [c]
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((c + 3) / 4), dim3(256), 0, st, partials, nblk, c, bn_bwd_count(rows, accumulate), gamma, save_invstd, dgamma, dbeta, coefd, k1, accumulate & 1);
    STRAPS_CHECK_LAUNCH("bn_bwd_finalize_kernel");
    const long long n4 = rows * C4;
    const int tiled = straps_bn_tiled(rows, c >> 2);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(tiled ? straps_bn_tiled_grid(rows, c >> 2, tiled) : straps_grid256_rows(n4, c >> 2)), dim3(256), 0, st, dy, yact, raw, save_mean, save_invstd, coefd, k1, mask_scale, mask_shift, draw, dz_out, draw_planes, plane_stride, n4, c, PoolSrc{}, relu_bits, tiled);
    STRAPS_CHECK_LAUNCH("bn_bwd_apply_kernel");
    return STRAPS_OK;
}

extern "C" int straps_bn_bwd_finish_x3(const float* dy, const float* yact, const float* raw, const float* save_mean, const float* save_invstd,
                                       const float* gamma, const float* mask_scale, const float* mask_shift, float* dgamma, float* dbeta,
                                       float* draw, float* dz_out, unsigned short* draw_planes, long long plane_stride, const double* partials,
                                       int nblk, void* workspace, long long rows, int c, int accumulate, void* stream) {
    return bn_bwd_finish_x3_impl(dy, yact, nullptr, raw, save_mean, save_invstd, gamma, mask_scale, mask_shift, dgamma, dbeta, draw, dz_out, draw_planes,
                                 plane_stride, partials, nblk, workspace, rows, c, accumulate, stream);
}

// straps_bn_bwd_finish_x3 with the ReLU mask as bits (see straps_bn_bwd_bits_x3; the partials come from straps_conv_dgrad_x3_bn_bits, which read
// the same bits)
extern "C" int straps_bn_bwd_finish_bits_x3(const float* dy, const unsigned* relu_bits, const float* raw, const float* save_mean,
                                            const float* save_invstd, const float* gamma, float* dgamma, float* dbeta, float* draw,
                                            unsigned short* draw_planes, long long plane_stride, const double* partials, int nblk, void* workspace,
                                            long long rows, int c, int accumulate, void* stream) {
    STRAPS_REQUIRE(relu_bits, "straps_bn_bwd_finish_bits_x3: null bit mask");
    return bn_bwd_finish_x3_impl(dy, nullptr, relu_bits, raw, save_mean, save_invstd, gamma, nullptr, nullptr, dgamma, dbeta, draw, nullptr, draw_planes,
                                 plane_stride, partials, nblk, workspace, rows, c, accumulate, stream);
}

extern "C" int straps_bn_bwd(const float* dy, const float* yact, const float* raw, const float* save_mean, const float* save_invstd,
                             const float* gamma, const float* mask_scale, const float* mask_shift, float* dgamma, float* dbeta, float* draw,
                             float* dz_out, void* workspace, long long rows, int c, int accumulate, void* stream) {
    return straps_bn_bwd_x3(dy, yact, raw, save_mean, save_invstd, gamma, mask_scale, mask_shift, dgamma, dbeta, draw, dz_out, nullptr, 0, workspace,
                            rows, c, accumulate, stream);
}

extern "C" size_t straps_stem_tiles(int batch, int h, int w) {
    const int Ho = (h - 1) / 2 + 1, Wo = (w - 1) / 2 + 1;
    return (size_t)batch * ((Wo + TX - 1) / TX) * ((Ho + TY - 1) / TY);
}

extern "C" int straps_stem_tile_activity(const uint32_t* nzmask, uint8_t* tile_active, int batch, int cin, int h, int w, void* stream) {
    STRAPS_REQUIRE(nzmask && tile_active, "straps_stem_tile_activity: null pointer");
    STRAPS_REQUIRE(batch > 0 && cin > 0 && h >= 7 && w >= 7, "straps_stem_tile_activity: bad shape B=%d C=%d H=%d W=%d", batch, cin, h, w);
    const int Ho = (h - 1) / 2 + 1, Wo = (w - 1) / 2 + 1;
    const int tiles_x = (Wo + TX - 1) / TX, tiles_y = (Ho + TY - 1) / TY;
    const int ntiles = batch * tiles_x * tiles_y;
    hipLaunchKernelGGL(stem_tileany_kernel, dim3((unsigned)(((long long)ntiles * 32 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nzmask, tile_active, cin, h, w, tiles_x, tiles_y,
                       ntiles);
    STRAPS_CHECK_LAUNCH("stem_tileany_kernel");
    return STRAPS_OK;
}

extern "C" int straps_bn_bwd_pooled(const float* dy_pool, const uint8_t* idx, const float* raw, const float* save_mean, const float* save_invstd,
                                    const float* gamma, const float* mask_scale, const float* mask_shift, float* dgamma, float* dbeta,
                                    float* draw, void* workspace, int batch, int h, int w, int c, int accumulate, void* stream) {
    return straps_bn_bwd_pooled_sparse(dy_pool, idx, raw, save_mean, save_invstd, gamma, mask_scale, mask_shift, dgamma, dbeta, draw, workspace, batch, h, w,
                                       c, accumulate, nullptr, stream);
}

extern "C" int straps_bn_bwd_pooled_sparse(const float* dy_pool, const uint8_t* idx, const float* raw, const float* save_mean, const float* save_invstd,
                                           const float* gamma, const float* mask_scale, const float* mask_shift, float* dgamma, float* dbeta,
                                           float* draw, void* workspace, int batch, int h, int w, int c, int accumulate,
                                           const uint8_t* tile_active, void* stream) {
    STRAPS_REQUIRE(dy_pool && idx && raw && save_mean && save_invstd && gamma && mask_scale && mask_shift && dgamma && dbeta && draw && workspace,
                   "straps_bn_bwd_pooled: null pointer");
    STRAPS_REQUIRE(batch > 0 && h > 0 && w > 0 && c > 0 && (c & 3) == 0, "straps_bn_bwd_pooled: bad shape %dx%dx%dx%d", batch, h, w, c);
    const int C4 = c >> 2;
    STRAPS_REQUIRE(C4 <= 256 ? (256 % C4 == 0) : (C4 % 256 == 0), "straps_bn_bwd_pooled: channel count %d not supported", c);
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)batch * h * w;
    const int nblk = straps_bn_bwd_blocks(rows, c);
    const int rpb = (int)((rows + nblk - 1) / nblk);
    double* part = (double*)workspace;               // [nblk][c][2]  (straps_bn_bwd_workspace_bytes(rows, c))
    double* coefd = part + (size_t)nblk * c * 2;     // [2][c]  m1, m2
    float* k1 = (float*)(coefd + 2 * (size_t)c);     // [c]
    const PoolSrc ps{dy_pool, idx, h, w, (h - 1) / 2 + 1, (w - 1) / 2 + 1, tile_active, (w + TX - 1) / TX, (h + TY - 1) / TY};
    const long long prows = (long long)batch * ps.Ho * ps.Wo;
    const int prpb = (int)((prows + nblk - 1) / nblk);
    (void)rpb;
    hipLaunchKernelGGL(bn_bwd_reduce_pooled_kernel, dim3(nblk, (c + 63) / 64), dim3(256), 0, st, raw, save_mean, save_invstd, mask_scale, mask_shift, part, prows, c, prpb, ps);
    STRAPS_CHECK_LAUNCH("bn_bwd_reduce_pooled_kernel");
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((c + 3) / 4), dim3(256), 0, st, part, nblk, c, bn_bwd_count(rows, accumulate), gamma, save_invstd, dgamma, dbeta, coefd, k1, accumulate & 1);
    STRAPS_CHECK_LAUNCH("bn_bwd_finalize_kernel");
    const long long n4 = rows * C4;
    hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3((unsigned)((n4 + POOL_CHUNK - 1) / POOL_CHUNK)), dim3(256), 0, st, nullptr, nullptr, raw, save_mean, save_invstd, coefd, k1, mask_scale, mask_shift, draw, nullptr, (u16*)nullptr, 0LL, n4, c, ps, (const unsigned*)nullptr, 0);
    STRAPS_CHECK_LAUNCH("bn_bwd_apply_kernel<pool>");
    return STRAPS_OK;
}

extern "C" int straps_bn_relu_maxpool_fwd_x3(const float* raw, const float* scale, const float* shift, float* y_pool, uint8_t* idx,
                                             unsigned short* y_planes, long long plane_stride, int batch, int h, int w, int c, void* stream) {
    STRAPS_REQUIRE(raw && scale && shift && y_pool && idx && batch > 0 && h > 0 && w > 0 && c > 0 && (c & 3) == 0, "straps_bn_relu_maxpool_fwd: bad arguments");
    const int Ho = (h - 1) / 2 + 1, Wo = (w - 1) / 2 + 1;
    const long long n = (long long)batch * Ho * Wo * (c >> 2);
    STRAPS_REQUIRE(!y_planes || (plane_stride >= n * 4 && plane_stride % 8 == 0), "straps_bn_relu_maxpool_fwd_x3: plane_stride must be >= the output size and a multiple of 8");
    STRAPS_REQUIRE(!y_planes || (c & 31) == 0, "straps_bn_relu_maxpool_fwd_x3: chunk-major planes need c %% 32 == 0 (c=%d)", c);
    hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(capped_grid(n)), dim3(256), 0, (hipStream_t)stream, raw, scale, shift, y_pool, idx, y_planes, plane_stride, batch, h, w, c, Ho, Wo);
    STRAPS_CHECK_LAUNCH("bn_relu_maxpool_kernel");
    return STRAPS_OK;
}

extern "C" int straps_bn_relu_maxpool_fwd(const float* raw, const float* scale, const float* shift, float* y_pool, uint8_t* idx, int batch, int h,
                                          int w, int c, void* stream) {
    return straps_bn_relu_maxpool_fwd_x3(raw, scale, shift, y_pool, idx, nullptr, 0, batch, h, w, c, stream);
}

extern "C" size_t straps_bn_bwd_workspace_bytes(long long rows, int c) {
    return ((size_t)straps_bn_bwd_blocks(rows, c) * c * 2 + 2 * (size_t)c) * sizeof(double) + (size_t)c * sizeof(float);
}

extern "C" int straps_maxpool_fwd_idx(const float* x, float* y, uint8_t* idx, int batch, int h, int w, int c, void* stream) {
    STRAPS_REQUIRE(x && y && idx, "straps_maxpool_fwd_idx: null pointer");
    // (h = 0 would give Ho = (0 - 1) / 2 + 1 = 1 by C division: one row of -inf written into a zero-sized output)
    STRAPS_REQUIRE(batch > 0, "straps_maxpool_fwd_idx: batch must be positive (batch=%d)", batch);
    STRAPS_REQUIRE(h > 0, "straps_maxpool_fwd_idx: h must be positive (h=%d)", h);
    STRAPS_REQUIRE(w > 0, "straps_maxpool_fwd_idx: w must be positive (w=%d)", w);
    STRAPS_REQUIRE(c > 0 && (c & 3) == 0, "straps_maxpool_fwd_idx: c must be a positive multiple of 4 (c=%d)", c);
    const int Ho = (h - 1) / 2 + 1, Wo = (w - 1) / 2 + 1;
    const long long n = (long long)batch * Ho * Wo * (c >> 2);
    hipLaunchKernelGGL(maxpool_idx_kernel, dim3(capped_grid(n)), dim3(256), 0, (hipStream_t)stream, x, y, idx, batch, h, w, c, Ho, Wo);
    STRAPS_CHECK_LAUNCH("maxpool_idx_kernel");
    return STRAPS_OK;
}

extern "C" int straps_maxpool_bwd(const float* dy, const uint8_t* idx, float* dx, int batch, int h, int w, int c, void* stream) {
    STRAPS_REQUIRE(dy && idx && dx, "straps_maxpool_bwd: null pointer");
    STRAPS_REQUIRE(batch > 0, "straps_maxpool_bwd: batch must be positive (batch=%d)", batch);
    STRAPS_REQUIRE(h > 0, "straps_maxpool_bwd: h must be positive (h=%d)", h);
    STRAPS_REQUIRE(w > 0, "straps_maxpool_bwd: w must be positive (w=%d)", w);
    STRAPS_REQUIRE(c > 0 && (c & 3) == 0, "straps_maxpool_bwd: c must be a positive multiple of 4 (c=%d)", c);
    const int Ho = (h - 1) / 2 + 1, Wo = (w - 1) / 2 + 1;
    const long long n = (long long)batch * h * w * (c >> 2);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(capped_grid(n)), dim3(256), 0, (hipStream_t)stream, dy, idx, dx, batch, h, w, c, Ho, Wo);
    STRAPS_CHECK_LAUNCH("maxpool_bwd_kernel");
    return STRAPS_OK;
}

extern "C" int straps_gap_bwd(const float* dfeat, float* dx, int batch, int hw, int c, void* stream) {
    STRAPS_REQUIRE(dfeat && dx && batch > 0 && hw > 0 && c > 0, "straps_gap_bwd: bad arguments");
    const long long n = (long long)batch * hw * c;
    hipLaunchKernelGGL(gap_bwd_kernel, dim3(capped_grid(n)), dim3(256), 0, (hipStream_t)stream, dfeat, dx, batch, hw, c);
    STRAPS_CHECK_LAUNCH("gap_bwd_kernel");
    return STRAPS_OK;
}

extern "C" int straps_masked_copy(const float* x, int ldx, const float* mask, int ldmask, float* y, int ldy, int m, int n, int accumulate,
                                  void* stream) {
    STRAPS_REQUIRE(x && y && m > 0 && n > 0, "straps_masked_copy: bad arguments");
    const long long t = (long long)m * n;
    hipLaunchKernelGGL(masked_copy_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, mask, ldmask, y, ldy, m, n, accumulate);
    STRAPS_CHECK_LAUNCH("masked_copy_kernel");
    return STRAPS_OK;
}

extern "C" int straps_rot6d_bwd(const float* x6, long long ld, int per_row, const float* drot, float* dx6, long long ldd, long long rows,
                                void* stream) {
    STRAPS_REQUIRE(x6 && drot && dx6 && rows > 0 && per_row > 0, "straps_rot6d_bwd: bad arguments");
    const long long n = rows * per_row;
    hipLaunchKernelGGL(rot6d_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x6, ld, per_row, drot, dx6, ldd, n);
    STRAPS_CHECK_LAUNCH("rot6d_bwd_kernel");
    return STRAPS_OK;
}
