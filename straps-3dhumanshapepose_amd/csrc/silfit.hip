// silfit.hip -- the silhouette term of test-time fitting: straps_distance_field, straps_silhouette_energy, straps_fit_adam
// (include/straps_hip.h states the objective).
//
// straps_distance_field: exact squared Euclidean distance transform, two launches.
//   df_columns_kernel  one lane per (frame, column): a sweep down and a sweep up leave the distance to the nearest foreground ROW of the column;
//   df_rows_kernel     one workgroup per (frame, row): the row's squared column distances in LDS, every lane minimises (c - c')^2 + g^2(c') over
//                      c'.  All values are integers below 2^24, so the arithmetic runs in fp32 (fma + min, full rate) and is exact.
// straps_silhouette_energy: four launches, every sum in a fixed order, no float atomics.
//   sil_project_kernel one lane per vertex: projection to grid coordinates, the inside term (bilinear sample of sqrt(d2)) and its derivative,
//                      one partial sum of rho^2 per 256 vertices;
//   sil_nearest_kernel one lane per lattice point, the body's projected vertices in LDS (6912 x 2 floats = 54 KiB per tile), ascending scan with
//                      a strict compare: the lowest index wins among equal squared distances;
//   sil_gather_kernel  one lane per vertex walks the nearest list in index order (the list in LDS, 2048 entries per tile) and adds the points that
//                      chose it: the scatter as a gather, hence deterministic; dverts and one partial of dcam per 256 vertices (the number of
//                      valid points is counted once, by the search: one integer per workgroup of it);
//   sil_finish_kernel  one workgroup per body: energy2 and dcam from the partials, strided sums and a fixed tree.
// straps_fit_adam: one wave per body, element lane + 64 q as in fit_keypoints_kernel; the update is that kernel's, with its fused operations written out.
#include "common.h"

namespace {

constexpr int NE = 157;
constexpr int BLK = 256;
constexpr int VTILE = 6912;               // projected vertices of a body held in LDS by the search (27 x 256)
constexpr int PTILE = 2048;               // entries of the nearest list held in LDS by the gather
constexpr int ADAM_WPB = 4;
constexpr int MAX_NBP = 32;              // workgroups per body of the search, each of which leaves one count of valid lattice points

// fixed-order sum over the 256 threads of a workgroup; every thread gets the result.  `s` is reusable after the call.
__device__ __forceinline__ float block_sum(float v, float* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = BLK / 2; o > 0; o >>= 1) {
        if (tid < o) s[tid] += s[tid + o];
        __syncthreads();
    }
    return s[0];
}

// ------------------------------------------------------------------ distance transform
__global__ __launch_bounds__(64) void df_columns_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ d2, long long batch, int wh) {
    const long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
    const int cb = (wh + 63) / 64 * 64;                  // columns per frame, padded to whole waves
    const long long b = gid / cb;
    const int c = (int)(gid - b * cb);
    if (b >= batch || c >= wh) return;
    const uint8_t* m = mask + (size_t)b * wh * wh + c;
    int32_t* d = d2 + (size_t)b * wh * wh + c;
    const int far = 2 * wh;                               // "no foreground above": larger than any row distance
    int run = far;
    for (int r = 0; r < wh; ++r) {
        run = m[(size_t)r * wh] ? 0 : min(run + 1, far);
        d[(size_t)r * wh] = run;
    }
    run = far;
    for (int r = wh - 1; r >= 0; --r) {
        const int down = d[(size_t)r * wh];
        run = down == 0 ? 0 : min(run + 1, far);
        d[(size_t)r * wh] = min(down, run);
    }
}

__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void df_rows_kernel(int32_t* __restrict__ d2, int wh) {
    __shared__ float g2[1024];
    int32_t* row = d2 + (size_t)blockIdx.x * wh;          // blockIdx.x = frame * wh + r
    const float big = 2.f * (float)wh * (float)wh;
    for (int c = threadIdx.x; c < wh; c += BLK) {
        const int g = row[c];
        g2[c] = g >= 2 * wh ? big : (float)(g * g);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < wh; c += BLK) {
        float best = big;
        float d = (float)c;                               // c - c'
#pragma unroll 8
        for (int cc = 0; cc < wh; ++cc) {
            best = fminf(best, fmaf(d, d, g2[cc]));
            d -= 1.f;
        }
        row[c] = (int32_t)best;
    }
}

// ------------------------------------------------------------------ silhouette energy
struct SilWs {
    float2* gv;        // [B][nverts] grid coordinates of the projected vertices
    float2* gin;       // [B][nverts] d(sum rho^2)/dg of a vertex
    float* pin;        // [B][nbv] partial sums of rho^2
    int32_t* nearest;  // [B][np] (the caller's buffer when given)
    float2* pc;        // [B][np] d(h^2)/dg of the point's nearest vertex
    float* ph2;        // [B][np] h^2, -1 at an invalid point
    float* pcam;       // [B][nbv][3] partials of dcam
    int32_t* pcnt;     // [B][MAX_NBP] valid lattice points seen by each workgroup of the search
};

__device__ __forceinline__ bool body_empty(const int32_t* __restrict__ d2, long long b, int wh) { return d2[(size_t)b * wh * wh] >= 2 * wh * wh; }

__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void sil_project_kernel(const float* __restrict__ verts, const float* __restrict__ cam, int ld_cam,
                                                                               const int32_t* __restrict__ d2, SilWs w, int nverts, int nbv, int wh) {
    __shared__ float red[BLK];
    const long long b = blockIdx.x / nbv;
    const int blk = blockIdx.x - (int)(b * nbv), v = blk * BLK + threadIdx.x;
    float rho2 = 0.f;
    if (v < nverts) {
        const size_t a = (size_t)b * nverts + v;
        const float s = cam[b * ld_cam], tx = cam[b * ld_cam + 1], ty = cam[b * ld_cam + 2];
        const float hw = 0.5f * (float)wh, top = (float)(wh - 1), unit = 2.f / (float)wh;
        const float px = s * (verts[a * 3] + tx), py = s * (verts[a * 3 + 1] + ty);
        const float gx = fmaf(px + 1.f, hw, -0.5f), gy = fmaf(py + 1.f, hw, -0.5f);
        w.gv[a] = make_float2(gx, gy);
        float2 gi = make_float2(0.f, 0.f);
        if (!body_empty(d2, b, wh)) {
            const float qx = fminf(fmaxf(gx, 0.f), top), qy = fminf(fmaxf(gy, 0.f), top);
            const float ox = gx - qx, oy = gy - qy;
            const float o = sqrtf(fmaf(oy, oy, ox * ox));
            const int ix = min((int)floorf(qx), wh - 2), iy = min((int)floorf(qy), wh - 2);
            const float fx = qx - (float)ix, fy = qy - (float)iy;
            const int32_t* cell = d2 + ((size_t)b * wh + iy) * wh + ix;
            const float d00 = sqrtf((float)cell[0]), d01 = sqrtf((float)cell[1]), d10 = sqrtf((float)cell[wh]), d11 = sqrtf((float)cell[wh + 1]);
            const float top_row = fmaf(fx, d01 - d00, d00), bot_row = fmaf(fx, d11 - d10, d10);
            const float D = fmaf(fy, bot_row - top_row, top_row);
            const float rho = (D + o) * unit;
            rho2 = rho * rho;
            // on a clamped axis D does not move and o does; on a free axis o is zero and D moves
            const float ddx = ox != 0.f ? ox / o : fmaf(fy, (d11 - d10) - (d01 - d00), d01 - d00);
            const float ddy = oy != 0.f ? oy / o : fmaf(fx, (d11 - d01) - (d10 - d00), d10 - d00);
            const float k = 2.f * rho * unit;
            gi = make_float2(k * ddx, k * ddy);
        }
        w.gin[a] = gi;
    }
    const float sum = block_sum(rho2, red);
    if (threadIdx.x == 0) w.pin[b * nbv + blk] = sum;
}

__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void sil_nearest_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ d2, SilWs w, int nverts,
                                                                               int wh, int lattice, int nl, int nbp, float tau) {
    __shared__ float2 sv[VTILE];
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    int mine = 0;                                          // valid points of this lane (integer: any order gives the same count)
    const long long b = blockIdx.x / nbp;
    const int blk = blockIdx.x - (int)(b * nbp);
    const int np = nl * nl, nchunks = (np + BLK - 1) / BLK;
    const bool empty = body_empty(d2, b, wh), single = nverts <= VTILE;
    const float2* gv = w.gv + (size_t)b * nverts;
    const float unit = 2.f / (float)wh;
    if (single && !empty) {
        for (int i = threadIdx.x; i < nverts; i += BLK) sv[i] = gv[i];
        __syncthreads();
    }
    for (int chunk = blk; chunk < nchunks; chunk += nbp) {            // (uniform over the workgroup: the barriers below are reached by all)
        const int a = chunk * BLK + threadIdx.x;
        const int i = a / nl, j = a - i * nl;
        const bool valid = a < np && !empty && mask[((size_t)b * wh + (size_t)lattice * i) * wh + (size_t)lattice * j] != 0;
        const float ax = (float)(lattice * j), ay = (float)(lattice * i);
        float bd = INFINITY;
        int bi = -1;
        mine += valid ? 1 : 0;
        for (int t0 = 0; t0 < nverts && !empty; t0 += VTILE) {
            const int n = min(VTILE, nverts - t0);
            if (!single) {
                __syncthreads();
                for (int q = threadIdx.x; q < n; q += BLK) sv[q] = gv[t0 + q];
                __syncthreads();
            }
            if (valid) {
#pragma unroll 4
                for (int q = 0; q < n; ++q) {
                    const float2 g = sv[q];
                    const float dx = g.x - ax, dy = g.y - ay;
                    const float d = fmaf(dy, dy, dx * dx);
                    if (d < bd) { bd = d; bi = t0 + q; }
                }
            }
        }
        if (a < np) {
            float2 c = make_float2(0.f, 0.f);
            float h2 = valid ? 0.f : -1.f;
            if (valid && bi >= 0) {
                const float r = sqrtf(bd);
                const float h = fmaxf(0.f, r - tau) * unit;
                h2 = h * h;
                if (h > 0.f) {
                    const float2 g = gv[bi];
                    const float k = 2.f * h * unit / r;
                    c = make_float2(k * (g.x - ax), k * (g.y - ay));
                }
            }
            const size_t o = (size_t)b * np + a;
            w.nearest[o] = valid ? bi : -1;
            w.pc[o] = c;
            w.ph2[o] = h2;
        }
    }
    __syncthreads();
    atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) w.pcnt[b * MAX_NBP + blk] = cnt;
}

__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void sil_gather_kernel(const float* __restrict__ verts, const float* __restrict__ cam, int ld_cam, SilWs w,
                                                                              float* __restrict__ dverts, int nverts, int nbv, int nbp, int wh, int np, float w_in, float w_out) {
    __shared__ int32_t sn[PTILE];
    __shared__ float red[BLK];
    const long long b = blockIdx.x / nbv;
    const int blk = blockIdx.x - (int)(b * nbv), v = blk * BLK + threadIdx.x;
    const int32_t* near_b = w.nearest + (size_t)b * np;
    const float2* pc = w.pc + (size_t)b * np;
    float ax = 0.f, ay = 0.f;
    for (int p0 = 0; p0 < np; p0 += PTILE) {
        const int n = min(PTILE, np - p0);
        __syncthreads();
        for (int q = threadIdx.x; q < n; q += BLK) sn[q] = near_b[p0 + q];
        __syncthreads();
        for (int q = 0; q < n; ++q) {
            if (sn[q] == v) {
                const float2 c = pc[p0 + q];
                ax += c.x;
                ay += c.y;
            }
        }
    }
    int n_valid = 0;                                       // counted once, by the search
    for (int k = 0; k < nbp; ++k) n_valid += w.pcnt[b * MAX_NBP + k];
    float part[3] = {0.f, 0.f, 0.f};
    if (v < nverts) {
        const size_t a = (size_t)b * nverts + v;
        const float s = cam[b * ld_cam], tx = cam[b * ld_cam + 1], ty = cam[b * ld_cam + 2];
        const float hw = 0.5f * (float)wh;
        const float cin = w_in / (float)nverts, cout = w_out / (float)max(1, n_valid);
        const float2 gi = w.gin[a];
        const float Gx = fmaf(cin, gi.x, cout * ax), Gy = fmaf(cin, gi.y, cout * ay);      // dE/dg of this vertex
        const float sx = s * hw * Gx, sy = s * hw * Gy;
        if (dverts) {
            dverts[a * 3] = sx;
            dverts[a * 3 + 1] = sy;
            dverts[a * 3 + 2] = 0.f;
        }
        part[0] = hw * fmaf(Gy, verts[a * 3 + 1] + ty, Gx * (verts[a * 3] + tx));
        part[1] = sx;
        part[2] = sy;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float sum = block_sum(part[q], red);
        if (threadIdx.x == 0) w.pcam[((size_t)b * nbv + blk) * 3 + q] = sum;
    }
}

__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void sil_finish_kernel(SilWs w, float* __restrict__ energy2, float* __restrict__ dcam, int nverts, int nbv, int np) {
    __shared__ float red[BLK];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    float e_in = 0.f, e_out = 0.f, nv = 0.f, c[3] = {0.f, 0.f, 0.f};
    for (int q = tid; q < nbv; q += BLK) {
        e_in += w.pin[b * nbv + q];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += w.pcam[((size_t)b * nbv + q) * 3 + k];
    }
    for (int q = tid; q < np; q += BLK) {
        const float h2 = w.ph2[(size_t)b * np + q];
        if (h2 >= 0.f) { e_out += h2; nv += 1.f; }        // (a count below 2^24: exact in fp32)
    }
    e_in = block_sum(e_in, red);
    e_out = block_sum(e_out, red);
    nv = block_sum(nv, red);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = block_sum(c[k], red);
    if (tid == 0) {
        if (energy2) {
            energy2[b * 2] = e_in / (float)nverts;
            energy2[b * 2 + 1] = e_out / fmaxf(1.f, nv);
        }
        if (dcam) {
            dcam[b * 3] = c[0];
            dcam[b * 3 + 1] = c[1];
            dcam[b * 3 + 2] = c[2];
        }
    }
}

// ------------------------------------------------------------------ the update step
__device__ __forceinline__ double ipow(double b, int t) {      // as csrc/fit.hip
    double r = 1.0;
    for (int n = 0; n < 32 && t > 0; ++n) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

__global__ __launch_bounds__(ADAM_WPB * 64) STRAPS_NO_PACKED_FP32 void fit_adam_kernel(
        straps_fit_opts_t o, float* __restrict__ est, const float* __restrict__ g_kp, const float* __restrict__ dcam, const float* __restrict__ dx6,
        const float* __restrict__ dbetas, const float* __restrict__ e_kp, const float* __restrict__ energy2, float w_in, float w_out,
        float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, float* __restrict__ energy, long long ld_energy, long long col,
        float* __restrict__ grad, float* __restrict__ best_est, float* __restrict__ best_energy, int step, int first, int update, long long B) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long body = (long long)blockIdx.x * ADAM_WPB + wv;
    if (body >= B) return;
    float E = e_kp ? e_kp[body] : 0.f;
    if (energy2) E = fmaf(w_out, energy2[body * 2 + 1], fmaf(w_in, energy2[body * 2], E));
    // every lane reads the held energy before lane 0 replaces it (one wave: program order)
    const float held = (best_energy && !first) ? best_energy[body] : 0.f;
    const bool better = first || E < held;      // the first minimum wins; a NaN never replaces what is held
    float e[3], g[3];
    bool ve[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int idx = lane + 64 * q;
        ve[q] = idx < NE;
        const int i = ve[q] ? idx : 0;
        e[q] = est[body * NE + i];
        float s = 0.f;
        bool have = false;
        if (i < 3) { if (dcam) { s = dcam[body * 3 + i]; have = true; } }
        else if (i < 147) { if (dx6) { s = dx6[body * 144 + i - 3]; have = true; } }
        else if (dbetas) { s = dbetas[body * 10 + i - 147]; have = true; }
        g[q] = g_kp ? (have ? g_kp[body * NE + i] + s : g_kp[body * NE + i]) : s;
        if (ve[q]) {
            if (grad) grad[body * NE + idx] = g[q];
            if (best_est && better) best_est[body * NE + idx] = e[q];
        }
    }
    if (lane == 0) {
        if (energy) energy[body * ld_energy + col] = E;
        if (best_energy && better) best_energy[body] = E;
    }
    if (!update) return;
    const int t = step + 1;
    const double bc1 = 1.0 - ipow((double)o.beta1, t);
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - ipow((double)o.beta2, t)));
    const float ss_cam = (float)((double)o.lr_cam / bc1), ss_pose = (float)((double)o.lr_pose / bc1), ss_shape = (float)((double)o.lr_shape / bc1);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int idx = lane + 64 * q;
        if (!ve[q]) continue;
        const long long a = body * NE + idx;
        const float mo = exp_avg[a], vo = exp_avg_sq[a];
        const float step_size = idx < 3 ? ss_cam : (idx < 147 ? ss_pose : ss_shape);
        // the fused forms the compiler gives the update of fit_keypoints_kernel, written out (and nothing else fused) so that the two stay bit-identical
        {
#pragma clang fp contract(off)
        const float gm = (1.f - o.beta1) * g[q], gv = (1.f - o.beta2) * g[q];
        const float gv2 = g[q] * gv;
        const float mi = fmaf(o.beta1, mo, gm);
        const float vi = fmaf(o.beta2, vo, gv2);
        const float num = mi * step_size;
        exp_avg[a] = mi;
        exp_avg_sq[a] = vi;
        est[a] = e[q] - num / fmaf(sqrtf(vi), inv_sqrt_bc2, o.eps);
        }
    }
}

inline long long sil_points(int wh, int lattice) {
    const long long nl = ((long long)wh + lattice - 1) / lattice;
    return nl * nl;
}

}  // namespace

extern "C" int straps_distance_field(const uint8_t* mask, int32_t* d2, long long batch, int wh, void* stream) {
    STRAPS_REQUIRE(mask && d2, "straps_distance_field: null pointer (mask, d2)");
    STRAPS_REQUIRE(wh >= 1 && wh <= 1024, "straps_distance_field: wh must be in 1..1024 (got %d)", wh);
    STRAPS_REQUIRE(batch > 0 && batch * wh <= (1LL << 31) - 1, "straps_distance_field: batch must be positive and batch * wh below 2^31 (got %lld)", batch);
    const long long cols = batch * ((wh + 63) / 64 * 64);
    hipLaunchKernelGGL(df_columns_kernel, dim3((unsigned)(cols / 64)), dim3(64), 0, (hipStream_t)stream, mask, d2, batch, wh);
    STRAPS_CHECK_LAUNCH("df_columns_kernel");
    hipLaunchKernelGGL(df_rows_kernel, dim3((unsigned)(batch * wh)), dim3(BLK), 0, (hipStream_t)stream, d2, wh);
    STRAPS_CHECK_LAUNCH("df_rows_kernel");
    return STRAPS_OK;
}

extern "C" size_t straps_silhouette_energy_workspace_bytes(long long batch, int nverts, int wh, int lattice) {
    if (batch <= 0 || nverts < 1 || wh < 2 || wh > 1024 || lattice < 1) return 0;
    const long long np = sil_points(wh, lattice), nbv = (nverts + BLK - 1) / BLK;
    return (size_t)batch * (size_t)(4 * (long long)nverts + 4 * np + 4 * nbv + MAX_NBP) * sizeof(float);
}

extern "C" int straps_silhouette_energy(const float* verts, const float* cam, int ld_cam, const uint8_t* mask, const int32_t* d2,
                                        const straps_silfit_opts_t* opts, float* energy2, float* dverts, float* dcam, int32_t* nearest,
                                        void* workspace, long long batch, int nverts, void* stream) {
    STRAPS_REQUIRE(opts, "straps_silhouette_energy: null opts");
    STRAPS_REQUIRE(verts && cam, "straps_silhouette_energy: null pointer (verts, cam)");
    STRAPS_REQUIRE(mask, "straps_silhouette_energy: null mask");
    STRAPS_REQUIRE(d2, "straps_silhouette_energy: null d2");
    STRAPS_REQUIRE(workspace, "straps_silhouette_energy: null workspace");
    STRAPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "straps_silhouette_energy: workspace must be 8-byte aligned");
    STRAPS_REQUIRE(energy2 || dverts || dcam || nearest, "straps_silhouette_energy: all outputs are null (energy2, dverts, dcam, nearest): give at least one");
    STRAPS_REQUIRE(opts->wh >= 2 && opts->wh <= 1024, "straps_silhouette_energy: wh must be in 2..1024 (got %d)", opts->wh);
    STRAPS_REQUIRE(opts->lattice >= 1, "straps_silhouette_energy: lattice must be at least 1 (got %d)", opts->lattice);
    STRAPS_REQUIRE(nverts >= 1 && nverts <= (1 << 20), "straps_silhouette_energy: nverts must be in 1..2^20 (got %d)", nverts);
    STRAPS_REQUIRE(ld_cam >= 3, "straps_silhouette_energy: ld_cam must be at least 3 (got %d)", ld_cam);
    STRAPS_REQUIRE(opts->tau >= 0.f, "straps_silhouette_energy: tau must not be negative");      // (a NaN fails as well)
    const int wh = opts->wh, lattice = opts->lattice > wh ? wh : opts->lattice;      // (any lattice above wh - 1 leaves the single point (0, 0))
    const long long np = sil_points(wh, lattice);
    const int nl = (wh + lattice - 1) / lattice, nbv = (nverts + BLK - 1) / BLK;
    const int nbp = (int)((np + BLK - 1) / BLK < MAX_NBP ? (np + BLK - 1) / BLK : MAX_NBP);
    STRAPS_REQUIRE(batch > 0 && batch * (long long)(nbv > nbp ? nbv : nbp) <= (1LL << 31) - 1 && batch * (long long)ld_cam <= (1LL << 31) - 1,
                   "straps_silhouette_energy: batch must be positive and batch x workgroups per body below 2^31 (got %lld)", batch);
    // the workspace, in the order of straps_silhouette_energy_workspace_bytes: 8-byte entries first
    SilWs w;
    char* p = static_cast<char*>(workspace);
    w.gv = reinterpret_cast<float2*>(p);        p += (size_t)batch * nverts * sizeof(float2);
    w.gin = reinterpret_cast<float2*>(p);       p += (size_t)batch * nverts * sizeof(float2);
    w.pc = reinterpret_cast<float2*>(p);        p += (size_t)batch * np * sizeof(float2);
    w.ph2 = reinterpret_cast<float*>(p);        p += (size_t)batch * np * sizeof(float);
    int32_t* near_ws = reinterpret_cast<int32_t*>(p); p += (size_t)batch * np * sizeof(int32_t);
    w.pin = reinterpret_cast<float*>(p);        p += (size_t)batch * nbv * sizeof(float);
    w.pcam = reinterpret_cast<float*>(p);       p += (size_t)batch * nbv * 3 * sizeof(float);
    w.pcnt = reinterpret_cast<int32_t*>(p);
    w.nearest = nearest ? nearest : near_ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sil_project_kernel, dim3((unsigned)(batch * nbv)), dim3(BLK), 0, st, verts, cam, ld_cam, d2, w, nverts, nbv, wh);
    STRAPS_CHECK_LAUNCH("sil_project_kernel");
    hipLaunchKernelGGL(sil_nearest_kernel, dim3((unsigned)(batch * nbp)), dim3(BLK), 0, st, mask, d2, w, nverts, wh, lattice, nl, nbp, opts->tau);
    STRAPS_CHECK_LAUNCH("sil_nearest_kernel");
    if (energy2 || dverts || dcam) {
        hipLaunchKernelGGL(sil_gather_kernel, dim3((unsigned)(batch * nbv)), dim3(BLK), 0, st, verts, cam, ld_cam, w, dverts, nverts, nbv, nbp, wh, (int)np,
                           opts->w_in, opts->w_out);
        STRAPS_CHECK_LAUNCH("sil_gather_kernel");
        if (energy2 || dcam) {
            hipLaunchKernelGGL(sil_finish_kernel, dim3((unsigned)batch), dim3(BLK), 0, st, w, energy2, dcam, nverts, nbv, (int)np);
            STRAPS_CHECK_LAUNCH("sil_finish_kernel");
        }
    }
    return STRAPS_OK;
}

extern "C" int straps_fit_adam(const straps_fit_opts_t* opts, float* est, const float* g_kp, const float* dcam, const float* dx6, const float* dbetas,
                               const float* e_kp, const float* energy2, float w_in, float w_out, float* exp_avg, float* exp_avg_sq,
                               float* energy, long long ld_energy, long long col, float* grad, float* best_est, float* best_energy,
                               int step, int first, int update, long long batch, void* stream) {
    STRAPS_REQUIRE(opts, "straps_fit_adam: null opts");
    STRAPS_REQUIRE(est, "straps_fit_adam: null est");
    STRAPS_REQUIRE(batch > 0 && batch <= (1LL << 31) - 4, "straps_fit_adam: batch must be in 1..2^31-4 (got %lld)", batch);
    STRAPS_REQUIRE(step >= 0 && step <= (1 << 30), "straps_fit_adam: step must be in 0..2^30 (got %d)", step);
    STRAPS_REQUIRE((best_est == nullptr) == (best_energy == nullptr), "straps_fit_adam: best_est and best_energy must be given together");
    STRAPS_REQUIRE(!update || (exp_avg && exp_avg_sq), "straps_fit_adam: update needs exp_avg and exp_avg_sq");
    STRAPS_REQUIRE(!energy || (ld_energy >= 1 && col >= 0 && col < ld_energy), "straps_fit_adam: col must be in 0..ld_energy-1 (got %lld of %lld)", col, ld_energy);
    STRAPS_REQUIRE(opts->beta1 >= 0.f && opts->beta1 < 1.f && opts->beta2 >= 0.f && opts->beta2 < 1.f && opts->eps > 0.f,
                   "straps_fit_adam: eps must be positive, beta1 and beta2 in [0, 1)");
    const unsigned blocks = (unsigned)((batch + ADAM_WPB - 1) / ADAM_WPB);
    hipLaunchKernelGGL(fit_adam_kernel, dim3(blocks), dim3(ADAM_WPB * 64), 0, (hipStream_t)stream, *opts, est, g_kp, dcam, dx6, dbetas, e_kp, energy2, w_in, w_out,
                       exp_avg, exp_avg_sq, energy, ld_energy, col, grad, best_est, best_energy, step, first, update, batch);
    STRAPS_CHECK_LAUNCH("fit_adam_kernel");
    return STRAPS_OK;
}
