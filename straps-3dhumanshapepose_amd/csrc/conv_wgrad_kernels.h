// conv_wgrad_kernels.h -- the kernels of conv_wgrad.hip: dW[co][r][s][ci] = sum_m dy[m][co] * x[m@(r,s)][ci] -- fp32 or bf16x3 MFMA, contraction over
// the B*Ho*Wo pixels, split over many workgroups (deterministic partials + a fixed-order reduce that also transposes KRSC -> OIHW, the layout of the
// parameter's .grad).  A parameter struct is pointers and strides first, then the geometry the plan fills (conv_wgrad_plan.h), member `g`.
#pragma once
#include "common.h"
#include "conv_wgrad_plan.h"

namespace {

struct WgradP {
    const float* x;    // [B][H][W][Cin]
    const float* dy;   // [B][Ho][Wo][Cout]
    float* part;       // [splits][Cout][R*S][Cin]
    WgradTapGeom g;
};

__device__ __attribute__((aligned(16))) float k_zero16w[4] = {0.f, 0.f, 0.f, 0.f};   // source of padding / out-of-range pixels

// One workgroup = one filter tap x a BCO(co) x BCI(ci) block x one split of the B*Ho*Wo pixels, 32 pixels per step.  Both operand
// tiles ([32 px][BCO | BCI channels], unpadded rows) go global -> LDS through the LDS-DMA (one wave-instruction = 1 KiB = 4 or 2
// pixels), two stages, one barrier per step; the fragment reads are ds_read_b32 over 32 consecutive channels (conflict-free without
// padding).  The pixel coordinates of a thread's copy slots advance incrementally (no division in the loop).
// The operands of this contraction stream from HBM (every pixel row is read once per tile of the OTHER channel dimension), so the
// tile sets the roofline: 64x64 = 16 flop/B (~80 TFLOP/s at 5 TB/s), 128x128 = 32 flop/B.
template <int BCO, int BCI>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradP p) {
    constexpr int STG = 32 * (BCO + BCI);                         // floats per stage: [32 px][BCO] then [32 px][BCI]
    constexpr int LPD = BCO / 4, PWD = 64 / LPD, RDD = 8 / PWD;   // dy: lanes per pixel, pixels per wave-copy, copy rounds per wave
    constexpr int LPX = BCI / 4, PWX = 64 / LPX, RDX = 8 / PWX;
    constexpr int MI = BCO / 64, NI = BCI / 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][STG]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wm = wave >> 1, wn = wave & 1;
    int t = blockIdx.x;
    const int itile = t % p.g.it; t /= p.g.it;
    const int ctile = t % p.g.ct; t /= p.g.ct;
    const int tap = t;
    const int r = tap / p.g.S, s = tap - r * p.g.S;
    const int split = blockIdx.y;
    const int co0 = ctile * BCO, ci0 = itile * BCI;
    const int mbeg = split * p.g.rows_per_split;
    const int mend = min(mbeg + p.g.rows_per_split, p.g.M);
    const int nsteps = (mend - mbeg + 31) >> 5;
    const bool pointwise = p.g.R == 1 && p.g.S == 1 && p.g.stride == 1 && p.g.pad == 0;
    const float* zsrc = k_zero16w;
    asm volatile("" : "+s"(zsrc));          // the constant's address stays in SGPRs (else: a GOT load + wait per copy, inside the loop)

    // copy slots at step 0: round q of this wave copies pixels (q*4 + wave) * PW .. of the tile
    int md[RDD];                                                  // dy rows need only the linear pixel index
    int mx[RDX], wo_[RDX], ho_[RDX], b_[RDX];
    const int cd = (lane % LPD) * 4, cx = (lane % LPX) * 4;
#pragma unroll
    for (int q = 0; q < RDD; ++q) md[q] = mbeg + (q * 4 + wave) * PWD + lane / LPD;
#pragma unroll
    for (int q = 0; q < RDX; ++q) {
        const int m = mbeg + (q * 4 + wave) * PWX + lane / LPX;
        mx[q] = m;
        const int HoWo = p.g.Ho * p.g.Wo;
        b_[q] = m / HoWo;
        const int rem = m - b_[q] * HoWo;
        ho_[q] = rem / p.g.Wo;
        wo_[q] = rem - ho_[q] * p.g.Wo;
    }
    const int adv_h = 32 / p.g.Wo, adv_w = 32 - adv_h * p.g.Wo;      // a step moves every slot 32 pixels on
    auto dma_step = [&](int stage) {
        float* D = smem + stage * STG;
        float* X = D + 32 * BCO;
#pragma unroll
        for (int q = 0; q < RDD; ++q) {
            const float* src = md[q] < mend ? p.dy + (long long)md[q] * p.g.Cout + co0 + cd : zsrc;
            md[q] += 32;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(D + (q * 4 + wave_u) * PWD * BCO), 16, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < RDX; ++q) {
            const bool in = mx[q] < mend;
            const float* src = zsrc;
            if (pointwise) {
                if (in) src = p.x + (long long)mx[q] * p.g.Cin + ci0 + cx;
            } else {
                const int hi = ho_[q] * p.g.stride - p.g.pad + r, wi = wo_[q] * p.g.stride - p.g.pad + s;
                if (in && (unsigned)hi < (unsigned)p.g.H && (unsigned)wi < (unsigned)p.g.W)
                    src = p.x + (((long long)b_[q] * p.g.H + hi) * p.g.W + wi) * p.g.Cin + ci0 + cx;
                wo_[q] += adv_w; ho_[q] += adv_h;
                if (wo_[q] >= p.g.Wo) { wo_[q] -= p.g.Wo; ++ho_[q]; }
                if (ho_[q] >= p.g.Ho) { const int k = ho_[q] / p.g.Ho; ho_[q] -= k * p.g.Ho; b_[q] += k; }
            }
            mx[q] += 32;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(X + (q * 4 + wave_u) * PWX * BCI), 16, 0, 0);
        }
    };
    f32x16 acc[MI][NI];
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
        for (int c = 0; c < NI; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[a][c][q] = 0.f;
    if (nsteps > 0) dma_step(0);
    const int i = lane & 31, h = lane >> 5;
    const int fa = h * 4 * BCO + wm * (BCO / 2) + i, fb = 32 * BCO + h * 4 * BCI + wn * (BCI / 2) + i;
    for (int st = 0; st < nsteps; ++st) {
        const int stage = st & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // my copies of step st have landed ...
        __builtin_amdgcn_s_barrier();                         // ... everybody's have, and the other stage is no longer being read
        asm volatile("" ::: "memory");
        if (st + 1 < nsteps) dma_step(stage ^ 1);
        const float* S = smem + stage * STG;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = kk * 8 + e;
                float av[MI], bv[NI];
#pragma unroll
                for (int a = 0; a < MI; ++a) av[a] = S[fa + k * BCO + a * 32];
#pragma unroll
                for (int c = 0; c < NI; ++c) bv[c] = S[fb + k * BCI + c * 32];
#pragma unroll
                for (int a = 0; a < MI; ++a)
#pragma unroll
                    for (int c = 0; c < NI; ++c) acc[a][c] = mfma32(av[a], bv[c], acc[a][c]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    }
    // C layout: lane -> ci (col), reg -> co (row).  partial[split][co][tap][ci]
    const long long RS = (long long)p.g.R * p.g.S;
    float* o = p.part + (long long)split * p.g.Cout * RS * p.g.Cin;
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
        for (int c = 0; c < NI; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int co = co0 + wm * (BCO / 2) + a * 32 + mfma_row(q, lane);
                o[((long long)co * RS + tap) * p.g.Cin + ci0 + wn * (BCI / 2) + c * 32 + i] = acc[a][c][q];
            }
}

// ---- 3x3 / stride 1 / pad 1 weight gradient with an LDS-staged input halo patch ----------------------------------
// All nine taps of a 64(co) x 64(ci) block are accumulated by ONE workgroup: per 32-pixel chunk (rpc output rows x cw
// columns, cw = min(Wo,32)) it stages the dy tile [32][64] and the (rpc+2) x (cw+2) x 64 input patch once, then runs
// 9 taps x 16 = 144 MFMAs per wave between barriers; the nine shifted views are just LDS addresses.  Versus the
// per-tap kernel above: 1/9 of the dy traffic, ~1/3 of the x traffic, 9x fewer barriers per MFMA.
struct Wgrad3P {
    const float* x;
    const float* dy;
    float* part;
    WgradHaloGeom g;
};

// Staging: both operands go global -> LDS through the LDS-DMA (global_load_lds_dwordx4; one wave-instruction = 4 pixels x 256 B,
// rows unpadded: the fragment reads are ds_read_b32 over 32 consecutive channels, conflict-free as they are), two stages, one
// barrier per chunk.  Operands: the four pixels a lane half handles per 8-pixel group sit side by side in one row, so their
// nine-tap windows overlap: 3 x 6 patch values + 4 dy values feed 36 MFMAs (instead of 36 + 4), and the next group's 22 values
// are read while the current 36 MFMAs issue.
// NG = 2: two 4-wave groups per workgroup take alternate chunks of the split into their own LDS stages and add their accumulators
// through LDS at the end -- one partial per CU instead of two: half the partial-sum traffic (write here, read in the reduce pass).
template <int NG>
__global__ __launch_bounds__(256 * NG) void conv_wgrad3x3_kernel(Wgrad3P p) {
    extern __shared__ __attribute__((aligned(16))) float smem_all[];
    const int pw = p.g.cw + 2;
    const int npatch = (p.g.rpc + 2) * pw;                 // <= 102 pixels
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;              // position inside the 4-wave group
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int grp = NG > 1 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8) : 0;
    float* smem = smem_all + grp * (2 * W3PX * 64);
    const int wm = wave >> 1, wn = wave & 1;
    const int itile = blockIdx.x % p.g.it, ctile = blockIdx.x / p.g.it;
    const int co0 = ctile * 64, ci0 = itile * 64;
    const int cbeg = blockIdx.y * p.g.chunks_per_split;
    const int cend = min(cbeg + p.g.chunks_per_split, p.g.nchunks);
    const int lp = tid >> 4, lc = tid & 15;              // staging: pixel slot, float4 column
    const float* zsrc = k_zero16w;
    asm volatile("" : "+s"(zsrc));          // the constant's address stays in SGPRs (else: a GOT load + wait per copy, inside the loop)

    // chunk-independent part of the copy addresses: dy pixel (row, col) inside the chunk, patch pixel (row, col) inside the patch
    int d_off[2], x_pr[7], x_pc[7];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int px = lp + 16 * q;
        d_off[q] = ((px >> p.g.cw_log2) * p.g.W + (px & (p.g.cw - 1))) * p.g.Cout + co0 + lc * 4;
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const int pp = lp + 16 * q;
        x_pr[q] = pp / pw - 1;
        x_pc[q] = pp - (x_pr[q] + 1) * pw - 1;
    }
    auto dma_chunk = [&](int c, int stage) {
        const int per_img = p.g.chunk_rows_per_img * p.g.chunks_per_row;
        const int b = c / per_img;
        const int rem = c - b * per_img;
        const int cr = rem / p.g.chunks_per_row, cc = rem - cr * p.g.chunks_per_row;
        const int ho0 = cr * p.g.rpc, wo0 = cc * p.g.cw;
        float* D = smem + stage * (W3PX * 64);
        float* X = D + 32 * 64;
        const float* dsrc = p.dy + ((long long)(b * p.g.H + ho0) * p.g.W + wo0) * p.g.Cout;
        const float* xsrc = p.x + ((long long)(b * p.g.H + ho0) * p.g.W + wo0) * p.g.Cin + ci0 + lc * 4;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(dsrc + d_off[q]),
                                             (__attribute__((address_space(3))) void*)(D + (4 * wave_u + 16 * q) * 64), 16, 0, 0);
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            if (q * 16 >= npatch) break;                 // wave-uniform
            const int hi = ho0 + x_pr[q], wi = wo0 + x_pc[q];
            const bool ok = (unsigned)hi < (unsigned)p.g.H && (unsigned)wi < (unsigned)p.g.W;     // (slots past the patch read anything)
            const float* src = ok ? xsrc + (x_pr[q] * p.g.W + x_pc[q]) * p.g.Cin : zsrc;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(X + (4 * wave_u + 16 * q) * 64), 16, 0, 0);
        }
    };
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
    if (cbeg + grp < cend) dma_chunk(cbeg + grp, 0);
    const int i = lane & 31, h = lane >> 5;
    // LDS float offsets of the lane's four 4-pixel groups (group kk = pixels kk*8 + h*4 .. +3 of the chunk)
    int g_d[4], g_x[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int px = kk * 8 + h * 4;
        g_d[kk] = px * 64 + wm * 32 + i;
        g_x[kk] = 32 * 64 + ((px >> p.g.cw_log2) * pw + (px & (p.g.cw - 1))) * 64 + wn * 32 + i;
    }
    const int pw64 = pw * 64;
    const int nj = (cend - cbeg + NG - 1) / NG;               // both groups run the same number of rounds (the barrier is shared)
    for (int j = 0; j < nj; ++j) {
        const int c = cbeg + grp + NG * j;
        const int stage = j & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // my copies of chunk c have landed ...
        __builtin_amdgcn_s_barrier();                         // ... everybody's have, and the other stage is no longer being read
        asm volatile("" ::: "memory");
        if (c + NG < cend) dma_chunk(c + NG, stage ^ 1);
        if (NG > 1 && c >= cend) continue;                    // (odd chunk count: the second group idles in the last round)
        const float* S = smem + stage * (W3PX * 64);
        float a[2][4], w[2][18];
        auto read_group = [&](int kk, float* av, float* wv) {
            const float* D = S + g_d[kk];
            const float* X = S + g_x[kk];
#pragma unroll
            for (int e = 0; e < 4; ++e) av[e] = D[e * 64];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cidx = 0; cidx < 6; ++cidx) wv[r * 6 + cidx] = X[r * pw64 + cidx * 64];
        };
        read_group(0, a[0], w[0]);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kk + 1 < 4) read_group(kk + 1, a[(kk + 1) & 1], w[(kk + 1) & 1]);
            const float* av = a[kk & 1];
            const float* wv = w[kk & 1];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int s2 = 0; s2 < 3; ++s2) acc[r * 3 + s2] = mfma32(av[e], wv[r * 6 + e + s2], acc[r * 3 + s2]);
        }
        __builtin_amdgcn_s_setprio(0);
    }
    if constexpr (NG > 1) {
        // group 1 -> LDS -> group 0, three taps per round (48 KB), fixed order: acc(group 0) + acc(group 1)
        float* R = smem_all + ((wave * 3) * 16) * 64 + lane;
#pragma unroll
        for (int rd = 0; rd < 3; ++rd) {
            __syncthreads();                                  // the stages (round 0) / the previous round's values are no longer needed
            if (grp == 1) {
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int q = 0; q < 16; ++q) R[(t * 16 + q) * 64] = acc[rd * 3 + t][q];
            }
            __syncthreads();
            if (grp == 0) {
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[rd * 3 + t][q] += R[(t * 16 + q) * 64];
            }
        }
        if (grp != 0) return;
    }
    float* o = p.part + (long long)blockIdx.y * p.g.Cout * 9 * p.g.Cin;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = co0 + wm * 32 + mfma_row(q, lane);
            o[((long long)co * 9 + t) * p.g.Cin + ci0 + wn * 32 + i] = acc[t][q];
        }
}

// ---- the same weight gradient on the bf16 matrix pipe (bf16x3 route, see conv_x3.hip) -------------------------------------------
// Operands are the three bf16 planes of x and dy (x = x1 + x2 + x3 exactly); a term dy * x is the six bf16 products of weight >= 2^-16
// in the fp32 accumulator of v_mfma_f32_32x32x16_bf16.  The reduction index of this GEMM is the PIXEL, but both operands are stored
// pixel-major / channel-minor, so a lane's eight consecutive k values are eight different LDS rows: they are gathered by the
// hardware transpose read ds_read_b64_tr_b16 -- in a 16-lane group, lanes 4j .. 4j+3 each name 4 contiguous channels of pixel j
// and lane t receives channel t of pixels 0..3 (tools/tr_probe.hip prints the lane map) -- two reads per plane and operand.
// LDS image per stage and plane: dy tile [32 pixels][64 channels] and input patch [128 pixel slots][64 channels], rows of 128 bytes
// copied by the LDS-DMA; the two 64-byte halves of a row are swapped when bit 1 of the pixel (slot) number is set, so four
// consecutive rows -- whatever the tap shift -- touch all 64 banks once per 32-lane read group.
struct Wgrad3XP {
    const u16* x3;
    const u16* dy3;
    long long xps, dps;
    float* part;
    WgradHaloGeom g;
    long long rows;                 // B * H * W: pixels of x and of dy (stride 1), the chunk stride of their chunk-major planes
};

typedef __bf16 bf16x8w __attribute__((ext_vector_type(8)));
typedef short short4w __attribute__((ext_vector_type(4)));
typedef short short8w __attribute__((ext_vector_type(8)));

__device__ __attribute__((aligned(16))) float k_zero16x[4] = {0.f, 0.f, 0.f, 0.f};

constexpr int W3X_TG = 2;          // taps whose MFMA chains are interleaved

// eight k values (pixels) of one channel: two transpose reads of four pixels each
__device__ __forceinline__ bf16x8w tr_frag(const u16* lo, const u16* hi) {
    const short4w a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4w*)lo);
    const short4w b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4w*)hi);
    const short8w v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8w, v);
}

// per-tap weight gradient (stride-2 / 1x1 / any shape the halo plan does not take) on the planes: conv_wgrad_kernel's structure -- one tap
// x a BCO x BCI channel block x one split of the pixels per workgroup, 32 pixels per step, LDS-DMA copies, two stages -- with the
// operand gathers of the kernel below (ds_read_b64_tr_b16).  Rows are BCO (BCI) bf16 channels; their 64-byte segments are permuted
// by the pixel number so four consecutive pixel rows cover all 64 banks (2 segments per row: swap on bit 1; 4 or more: xor with
// the low two bits).
struct WgradXP {
    const u16* x3;
    const u16* dy3;
    long long xps, dps;
    float* part;
    WgradTapGeom g;
};

template <int BC>
__device__ __forceinline__ int seg_swz(int px) { return BC == 64 ? ((px >> 1) & 1) : (px & 3); }

// NST stages: two in production.  Round 3 tried three and four (copies of NST - 1 steps in flight, s_waitcnt vmcnt(DPS * (NST - 2))), on
// the reasoning that a 32-pixel step is only 0.1-0.4 us of matrix work: no gain on any resnet18 / resnet50 shape and 10-60 % slower on
// the 3x3 / stride-2 layers (tools/sweep_wgrad_x3.py with STRAPS_WGRAD_TAP_NST=3|4: the LDS the extra stages take costs a resident
// workgroup) -- the kernel is bound by the operand bytes it streams from L2, not by their latency.
template <int BCO, int BCI, int NST = 2>
__global__ __launch_bounds__(256) void conv_wgrad_x3_kernel(WgradXP p) {
    constexpr int PLD = 32 * BCO, PLX = 32 * BCI;                 // u16 elements per plane of a stage: [32 px][BCO], [32 px][BCI]
    constexpr int STG = 3 * (PLD + PLX);
    constexpr int LPD = BCO / 8, PWD = 64 / LPD, RDD = 8 / PWD;   // dy: lanes per pixel, pixels per wave-copy, copy rounds per wave
    constexpr int LPX = BCI / 8, PWX = 64 / LPX, RDX = 8 / PWX;
    constexpr int MI = BCO / 64, NI = BCI / 64;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    u16* smem = reinterpret_cast<u16*>(smem_f);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wm = wave >> 1, wn = wave & 1;
    int t = blockIdx.x;
    const int itile = t % p.g.it; t /= p.g.it;
    const int ctile = t % p.g.ct; t /= p.g.ct;
    const int tap = t;
    const int r = tap / p.g.S, s = tap - r * p.g.S;
    const int split = blockIdx.y;
    const int co0 = ctile * BCO, ci0 = itile * BCI;
    const int mbeg = split * p.g.rows_per_split;
    const int mend = min(mbeg + p.g.rows_per_split, p.g.M);
    const int nsteps = (mend - mbeg + 31) >> 5;
    const bool pointwise = p.g.R == 1 && p.g.S == 1 && p.g.stride == 1 && p.g.pad == 0;
    const u16* zsrc = reinterpret_cast<const u16*>(k_zero16w);
    asm volatile("" : "+s"(zsrc));

    // copy slots at step 0: round q of this wave copies pixels (q*4 + wave) * PW .. of the tile; a lane's 16-byte slot j = lane % LP
    // of pixel row px receives channel group ((j >> 2) ^ swz(px)) * 4 + (j & 3)
    // (chunk-major planes, common.h: channel c of pixel row m sits at ((c >> 5) * rows + m) * 32 + (c & 31); gd / gx = the chunk's
    //  base + the 16-byte piece inside it, fixed per lane)
    int md[RDD];
    long long gd[RDD], gx[RDX];
    int mx[RDX], wo_[RDX], ho_[RDX], b_[RDX];
    const long long xrows = (long long)p.g.B * p.g.H * p.g.W;
#pragma unroll
    for (int q = 0; q < RDD; ++q) {
        const int px = (q * 4 + wave) * PWD + lane / LPD, j = lane % LPD;
        md[q] = mbeg + px;
        const int c = co0 + ((((j >> 2) ^ seg_swz<BCO>(px)) << 2) | (j & 3)) * 8;
        gd[q] = (long long)(c >> 5) * p.g.M * 32 + (c & 31);
    }
#pragma unroll
    for (int q = 0; q < RDX; ++q) {
        const int px = (q * 4 + wave) * PWX + lane / LPX, j = lane % LPX;
        const int m = mbeg + px;
        mx[q] = m;
        const int c = ci0 + ((((j >> 2) ^ seg_swz<BCI>(px)) << 2) | (j & 3)) * 8;
        gx[q] = (long long)(c >> 5) * xrows * 32 + (c & 31);
        const int HoWo = p.g.Ho * p.g.Wo;
        b_[q] = m / HoWo;
        const int rem = m - b_[q] * HoWo;
        ho_[q] = rem / p.g.Wo;
        wo_[q] = rem - ho_[q] * p.g.Wo;
    }
    const int adv_h = 32 / p.g.Wo, adv_w = 32 - adv_h * p.g.Wo;      // a step moves every slot 32 pixels on
    auto dma_step = [&](int stage) {
        u16* D = smem + stage * STG;
        u16* X = D + 3 * PLD;
#pragma unroll
        for (int q = 0; q < RDD; ++q) {
            const bool in = md[q] < mend;
            const u16* src = in ? p.dy3 + (long long)md[q] * 32 + gd[q] : zsrc;
            const long long ps = in ? p.dps : 0;
            md[q] += 32;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + pl * ps),
                                                 (__attribute__((address_space(3))) void*)(D + pl * PLD + (q * 4 + wave_u) * PWD * BCO), 16, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < RDX; ++q) {
            bool in = mx[q] < mend;
            const u16* src = zsrc;
            if (pointwise) {
                if (in) src = p.x3 + (long long)mx[q] * 32 + gx[q];
            } else {
                const int hi = ho_[q] * p.g.stride - p.g.pad + r, wi = wo_[q] * p.g.stride - p.g.pad + s;
                in = in && (unsigned)hi < (unsigned)p.g.H && (unsigned)wi < (unsigned)p.g.W;
                if (in) src = p.x3 + (((long long)b_[q] * p.g.H + hi) * p.g.W + wi) * 32 + gx[q];
                wo_[q] += adv_w; ho_[q] += adv_h;
                if (wo_[q] >= p.g.Wo) { wo_[q] -= p.g.Wo; ++ho_[q]; }
                if (ho_[q] >= p.g.Ho) { const int k = ho_[q] / p.g.Ho; ho_[q] -= k * p.g.Ho; b_[q] += k; }
            }
            const long long ps = in ? p.xps : 0;
            mx[q] += 32;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + pl * ps),
                                                 (__attribute__((address_space(3))) void*)(X + pl * PLX + (q * 4 + wave_u) * PWX * BCI), 16, 0, 0);
        }
    };
    f32x16 acc[MI][NI];
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
        for (int c = 0; c < NI; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[a][c][q] = 0.f;
#pragma unroll
    for (int s0 = 0; s0 < NST - 1; ++s0)
        if (s0 < nsteps) dma_step(s0);
    // fragment addresses: lane t = lane & 15 names row t >> 2 of a 4-pixel group and channel quad t & 3 of its 16-channel half
    const int tt = lane & 15, ch16 = (lane >> 4) & 1, kh = lane >> 5;
    int fd[2][2][MI], fx[2][2][NI];                               // [k step][read][32-channel block]
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
            const int px = ks * 16 + kh * 8 + rd * 4 + (tt >> 2);
#pragma unroll
            for (int a = 0; a < MI; ++a) {
                const int c4 = wm * (BCO / 2) + a * 32 + ch16 * 16 + (tt & 3) * 4;
                fd[ks][rd][a] = px * BCO + (((c4 >> 5) ^ seg_swz<BCO>(px)) << 5) + (c4 & 31);
            }
#pragma unroll
            for (int c = 0; c < NI; ++c) {
                const int c4 = wn * (BCI / 2) + c * 32 + ch16 * 16 + (tt & 3) * 4;
                fx[ks][rd][c] = px * BCI + (((c4 >> 5) ^ seg_swz<BCI>(px)) << 5) + (c4 & 31);
            }
        }
    constexpr int TA[6] = {1, 0, 2, 0, 1, 0};
    constexpr int TB[6] = {1, 2, 0, 1, 0, 0};
    constexpr int DPS = 3 * (RDD + RDX);                      // LDS-DMA instructions per step and wave
    static_assert(DPS * (NST - 2) <= 63, "vmcnt range");
    int stage = 0;
    for (int st = 0; st < nsteps; ++st) {
        // my copies of step st have landed (the younger steps' may still be in flight) ...
        const int ahead = nsteps - 1 - st;
        if (NST >= 4 && ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DPS * (NST >= 4 ? 2 : 0)) : "memory");
        else if (NST >= 3 && ahead >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DPS * (NST >= 3 ? 1 : 0)) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // ... everybody's have, and the stage about to be refilled is no longer being read
        asm volatile("" ::: "memory");
        if (st + NST - 1 < nsteps) dma_step(stage == 0 ? NST - 1 : stage - 1);
        const u16* D = smem + stage * STG;
        const u16* X = D + 3 * PLD;
        stage = stage + 1 == NST ? 0 : stage + 1;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8w av[MI][3], bv[NI][3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
                for (int a = 0; a < MI; ++a) av[a][pl] = tr_frag(D + pl * PLD + fd[ks][0][a], D + pl * PLD + fd[ks][1][a]);
#pragma unroll
                for (int c = 0; c < NI; ++c) bv[c][pl] = tr_frag(X + pl * PLX + fx[ks][0][c], X + pl * PLX + fx[ks][1][c]);
            }
#pragma unroll
            for (int e = 0; e < 6; ++e)
#pragma unroll
                for (int a = 0; a < MI; ++a)
#pragma unroll
                    for (int c = 0; c < NI; ++c)
                        acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[a][TA[e]], bv[c][TB[e]], acc[a][c], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
    }
    // C layout: lane -> ci (col), reg -> co (row).  partial[split][co][tap][ci]
    const int i = lane & 31;
    const long long RS = (long long)p.g.R * p.g.S;
    float* o = p.part + (long long)split * p.g.Cout * RS * p.g.Cin;
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
        for (int c = 0; c < NI; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int co = co0 + wm * (BCO / 2) + a * 32 + mfma_row(q, lane);
                o[((long long)co * RS + tap) * p.g.Cin + ci0 + wn * (BCI / 2) + c * 32 + i] = acc[a][c][q];
            }
}

// NG = 2: two 4-wave groups share every stage; group g takes the k steps g, g + 2, .. (16 pixels each) of each chunk and the two accumulator
// sets are added through LDS at the end (fixed order) -- two waves per SIMD cover each other's LDS latency and barrier waits.
// CP = pixels per chunk (32 or 64; the plan's cw x rpc): 64 halves the barriers per MFMA and the halo overhead of the patch
// ((rpc + 2) x (cw + 2) slots per chunk: 3.2 -> 2.1 per pixel at cw = 32); a group then runs two k steps per chunk.
// ABL: compile-time measurement switches (tools, STRAPS_WGRAD3_ABL; 0 in production): 1 = no operand copies after the first chunk,
// 2 = no MFMAs (the fragments are folded into one accumulator on the VALU), 4 = a tenth of the fragment reads (every tap uses tap 0's)
template <int NG, int CP, int ABL = 0>
__global__ __launch_bounds__(256 * NG) void conv_wgrad3x3_x3_kernel(Wgrad3XP p) {
    constexpr int DPX = CP, XPX = CP == 32 ? 128 : 136;          // pixel rows per stage and plane: dy tile, input patch slots
    constexpr int STAGE = 3 * (DPX + XPX) * 64;                   // u16 elements per stage
    constexpr int DR = CP / 32, XR = (XPX + 31) / 32;             // copy rounds of 32 pixel slots: dy tile, patch
    constexpr int KSG = CP / 16 / NG;                             // k steps per group and chunk
    static_assert(CP % (16 * NG) == 0, "chunk / group mismatch");
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    u16* smem = reinterpret_cast<u16*>(smem_f);
    const int pw = p.g.cw + 2;
    const int npatch = (p.g.rpc + 2) * pw;                 // <= 102 (CP = 32) / 136 (CP = 64) pixels
    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3;           // wave inside its 4-wave group
    const int grp = NG > 1 ? __builtin_amdgcn_readfirstlane(tid >> 8) : 0;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wm = wave >> 1, wn = wave & 1;
    const int itile = blockIdx.x % p.g.it, ctile = blockIdx.x / p.g.it;
    const int co0 = ctile * 64, ci0 = itile * 64;
    const int cbeg = blockIdx.y * p.g.chunks_per_split;
    const int cend = min(cbeg + p.g.chunks_per_split, p.g.nchunks);
    const u16* zsrc = reinterpret_cast<const u16*>(k_zero16x);
    asm volatile("" : "+s"(zsrc));

    // ---- copies: thread -> (pixel slot of a 32-slot round, 16-byte slot tid & 7 of its row); it fetches channel group slot ^ swap.
    // The five rounds of a chunk (dy tile, four patch rounds) alternate between the groups when NG = 2.
    const int lp = (tid & 255) >> 3, ls = tid & 7;
    const int d_g = ls ^ (((lp >> 1) & 1) << 2);           // (bit 1 of lp + 32 q is bit 1 of lp)
    // (chunk-major planes, common.h: a 64-channel row is two 64-byte pieces, one in each of two 32-channel chunks)
    long long d_off[DR];
#pragma unroll
    for (int q = 0; q < DR; ++q) {
        const int px = lp + 32 * q;
        d_off[q] = ((long long)((co0 >> 5) + (d_g >> 2)) * p.rows + (px >> p.g.cw_log2) * p.g.W + (px & (p.g.cw - 1))) * 32 + (d_g & 3) * 8;
    }
    int x_pr[XR], x_pc[XR];
    long long x_g[XR];
#pragma unroll
    for (int q = 0; q < XR; ++q) {
        const int pp = lp + 32 * q;
        x_pr[q] = pp / pw - 1;
        x_pc[q] = pp - (x_pr[q] + 1) * pw - 1;
        const int g = ls ^ (((pp >> 1) & 1) << 2);
        x_g[q] = (long long)((ci0 >> 5) + (g >> 2)) * p.rows * 32 + (g & 3) * 8;
    }
    auto dma_chunk = [&](int c, int stage) {
        const int per_img = p.g.chunk_rows_per_img * p.g.chunks_per_row;
        const int b = c / per_img;
        const int rem = c - b * per_img;
        const int cr = rem / p.g.chunks_per_row, cc = rem - cr * p.g.chunks_per_row;
        const int ho0 = cr * p.g.rpc, wo0 = cc * p.g.cw;
        u16* D = smem + stage * STAGE;
        u16* X = D + 3 * DPX * 64;
        const u16* dbase = p.dy3 + ((long long)(b * p.g.H + ho0) * p.g.W + wo0) * 32;
        const u16* xsrc = p.x3 + ((long long)(b * p.g.H + ho0) * p.g.W + wo0) * 32;
#pragma unroll
        for (int q = 0; q < DR; ++q) {
            if (NG > 1 && (q & 1) != grp) continue;          // the copy rounds of a chunk (dy rounds, then patch rounds) alternate between the groups
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(dbase + d_off[q] + pl * p.dps),
                                                 (__attribute__((address_space(3))) void*)(D + (pl * DPX + 32 * q + 8 * wave_u) * 64), 16, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < XR; ++q) {
            if (q * 32 + 8 * wave_u >= npatch || q * 32 + 8 * wave_u >= XPX) break;     // wave-uniform: nothing of this round lies inside the patch
            if (NG > 1 && ((q + DR) & 1) != grp) continue;
            const int hi = ho0 + x_pr[q], wi = wo0 + x_pc[q];
            const bool ok = (unsigned)hi < (unsigned)p.g.H && (unsigned)wi < (unsigned)p.g.W;     // (slots past the patch read anything)
            const u16* src = ok ? xsrc + (x_pr[q] * p.g.W + x_pc[q]) * 32 + x_g[q] : zsrc;
            const long long ps = ok ? p.xps : 0;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + pl * ps),
                                                 (__attribute__((address_space(3))) void*)(X + (pl * XPX + 32 * q + 8 * wave_u) * 64), 16, 0, 0);
        }
    };

    // ---- fragment addresses (u16 element offsets inside a stage, plane 0), fixed for the whole kernel.
    // lane: t = lane & 15 (row j = t >> 2 of the 4-pixel group, channel quad t & 3), 16-channel half (lane >> 4) & 1, k half lane >> 5.
    const int t = lane & 15, ch16 = (lane >> 4) & 1, kh = lane >> 5;
    auto row_off = [&](int slot_px, int c4) {            // element offset of 4 contiguous channels c4 .. c4+3 (of 64) in pixel slot slot_px
        const int g = (c4 >> 3) ^ (((slot_px >> 1) & 1) << 2);
        return slot_px * 64 + g * 8 + (c4 & 4);
    };
    int d_fo[KSG][2], x_fo[KSG][2];     // [this group's k step][read]; group g takes k steps g, g + NG, ...
#pragma unroll
    for (int ks = 0; ks < KSG; ++ks)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int px = (grp + NG * ks) * 16 + kh * 8 + r * 4 + (t >> 2);
            d_fo[ks][r] = row_off(px, wm * 32 + ch16 * 16 + (t & 3) * 4);
            x_fo[ks][r] = (px >> p.g.cw_log2) * pw + (px & (p.g.cw - 1));          // patch slot of tap (0,0); the channel part is added per tap
        }
    const int x_c4 = wn * 32 + ch16 * 16 + (t & 3) * 4;

    f32x16 acc[9];
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[tp][q] = 0.f;
    if (cbeg < cend) dma_chunk(cbeg, 0);
    constexpr int TA[6] = {1, 0, 2, 0, 1, 0};            // plane pairs (dy, x) of the six products, smallest terms first
    constexpr int TB[6] = {1, 2, 0, 1, 0, 0};
    for (int c = cbeg; c < cend; ++c) {
        const int stage = (c - cbeg) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // my copies of chunk c have landed ...
        __builtin_amdgcn_s_barrier();                         // ... everybody's have, and the other stage is no longer being read
        asm volatile("" ::: "memory");
        if (c + 1 < cend && !(ABL & 1)) dma_chunk(c + 1, stage ^ 1);
        const u16* D = smem + ((ABL & 1) ? 0 : stage) * STAGE;
        const u16* X = D + 3 * DPX * 64;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < KSG; ++ks) {
            bf16x8w a[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) a[pl] = tr_frag(D + pl * DPX * 64 + d_fo[ks][0], D + pl * DPX * 64 + d_fo[ks][1]);
            // taps in pairs: the six products of a tap accumulate into one tile, so two taps' chains are interleaved (a dependent
            // MFMA issued back to back waits for its predecessor's last pass)
#pragma unroll
            for (int tp0 = 0; tp0 < 9; tp0 += W3X_TG) {
                bf16x8w b[W3X_TG][3];
#pragma unroll
                for (int u = 0; u < W3X_TG; ++u) {
                    const int tp = tp0 + u;
                    if (tp >= 9) break;
                    const int sh = (ABL & 4) ? 0 : (tp / 3) * pw + (tp % 3);      // (ablation 4: every tap reads tap 0's fragments -- the compiler merges the reads)
                    const int o0 = row_off(x_fo[ks][0] + sh, x_c4), o1 = row_off(x_fo[ks][1] + sh, x_c4);
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) b[u][pl] = tr_frag(X + pl * XPX * 64 + o0, X + pl * XPX * 64 + o1);
                }
                if (ABL & 2) {
#pragma unroll
                    for (int u = 0; u < W3X_TG; ++u)
                        if (tp0 + u < 9)
#pragma unroll
                            for (int pl = 0; pl < 3; ++pl) acc[0][pl] += (float)b[u][pl][0] + (float)a[pl][1];
                    continue;
                }
#pragma unroll
                for (int e = 0; e < 6; ++e)
#pragma unroll
                    for (int u = 0; u < W3X_TG; ++u)
                        if (tp0 + u < 9) acc[tp0 + u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[TA[e]], b[u][TB[e]], acc[tp0 + u], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    }
    if constexpr (NG > 1) {
        // group 1 -> LDS -> group 0, three taps per round (48 KB), fixed order: acc(group 0) + acc(group 1)
        float* R = smem_f + ((wave * 3) * 16) * 64 + lane;
#pragma unroll
        for (int rd = 0; rd < 3; ++rd) {
            __syncthreads();                                  // the stages (round 0) / the previous round's values are no longer needed
            if (grp == 1) {
#pragma unroll
                for (int tp = 0; tp < 3; ++tp)
#pragma unroll
                    for (int q = 0; q < 16; ++q) R[(tp * 16 + q) * 64] = acc[rd * 3 + tp][q];
            }
            __syncthreads();
            if (grp == 0) {
#pragma unroll
                for (int tp = 0; tp < 3; ++tp)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[rd * 3 + tp][q] += R[(tp * 16 + q) * 64];
            }
        }
        if (grp != 0) return;
    }
    const int i = lane & 31;
    float* o = p.part + (long long)blockIdx.y * p.g.Cout * 9 * p.g.Cin;
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = co0 + wm * 32 + mfma_row(q, lane);
            o[((long long)co * 9 + tp) * p.g.Cin + ci0 + wn * 32 + i] = acc[tp][q];
        }
}

// dW_oihw[co][ci][r][s] = sum_split part[split][co][tap][ci]   (fixed order)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int splits,
                                                           int Cout, int Cin, int RS, int accumulate) {
    // 256 consecutive KRSC outputs per workgroup (float4 per lane: 1 KiB per wave-load); the 4 waves take interleaved
    // splits, 4 independent loads in flight per lane; fixed summation order; combined through LDS.
    // n is a multiple of 256 (Cin % 64 == 0, Cout % 64 == 0).
    __shared__ f32x4 red[4][64];
    const long long n = (long long)Cout * RS * Cin;
    const int lane = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const long long idx = ((long long)blockIdx.x * 64 + lane) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int k = sg;
    for (; k + 12 < splits; k += 16) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(part + (long long)k * n + idx);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(part + (long long)(k + 4) * n + idx);
        const f32x4 v2 = *reinterpret_cast<const f32x4*>(part + (long long)(k + 8) * n + idx);
        const f32x4 v3 = *reinterpret_cast<const f32x4*>(part + (long long)(k + 12) * n + idx);
        s += (v0 + v1) + (v2 + v3);
    }
    for (; k < splits; k += 4) s += *reinterpret_cast<const f32x4*>(part + (long long)k * n + idx);
    red[sg][lane] = s;
    __syncthreads();
    if (sg != 0) return;
    s = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    const int ci = (int)(idx % Cin);           // 4 consecutive ci of one (co, tap)
    long long t = idx / Cin;
    const int tap = (int)(t % RS);
    const int co = (int)(t / RS);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long long o = ((long long)co * Cin + ci + e) * RS + tap;
        dw[o] = accumulate ? dw[o] + s[e] : s[e];
    }
}

}  // namespace
