// fit.hip -- test-time fitting of (cam, 6-D pose, shape) to 2-D keypoints: straps_fit_keypoints (include/straps_hip.h states the objective).
//
// One kernel, one launch, all iterations inside it.  One wave64 per body, FIT_WPB bodies per workgroup:
//   * the tables (tracked-vertex blend directions, dense skinning rows, rest joints) go to LDS once per workgroup with 16-byte loads;
//   * lane e (+64, +128) keeps element e of est / exp_avg / exp_avg_sq / the prior centre / the best iterate in registers for the whole call;
//   * lane j < 24 is joint j: Gram-Schmidt, the kinematic chain by tree depth with wave shuffles (as smpl_pose_kernel) and its transpose;
//   * lane k < n_kp is keypoint k: projection, residual, robust weight;
//   * the K = 218 blend of a tracked vertex is split over the 64 lanes (lane l: columns l, l+64, l+128, l+192) and summed by an xor butterfly;
//     its transpose (the gradient of the blend coefficients) needs no reduction in that layout.
// Waves never talk to each other after the table load, every cross-lane sum is an xor butterfly (the same bits in every lane, fixed order), there
// are no atomics: a body's result depends on nothing but that body.  Inside the loop global memory is touched only by the energy trace.
// All products of the forward chain are explicit fmaf chains: the arithmetic order is in the source, not the optimiser's choice.
#include "common.h"

namespace {

constexpr int NE = 157;                   // cam 3 | x6 144 | beta 10
constexpr int KP = STRAPS_SMPL_KP;        // 224 blend columns (218 used)
constexpr int FIT_WPB = 4;                // bodies (waves) per workgroup
// per-wave LDS slice (floats)
constexpr int W_EST = 0;                  // [160] the current estimate
constexpr int W_F = W_EST + 160;          // [224] blend coefficients
constexpr int W_GT = W_F + KP;            // [24][3] posed joints
constexpr int W_VP = W_GT + 72;           // [16][3] blended (unposed) tracked vertices
constexpr int W_XV = W_VP + 48;           // [16][3] skinned tracked vertices
constexpr int W_GX = W_XV + 48;           // [32][2] dE/dX of a keypoint (z is 0)
constexpr int W_GXV = W_GX + 64;          // [16][2] the same summed per tracked vertex
constexpr int W_GF = W_GXV + 32;          // [224] dE/dF
constexpr int W_GE = W_GF + KP;           // [160] dE/dest without the priors
constexpr int WAVE_FLOATS = W_GE + 160;   // 1032
constexpr int TABLE_TAIL = 72 + 720 + 24 + 24 + 32 + 8;      // j_template, j_shapedirs, parents, depth, kp_src, misc

__host__ __device__ inline size_t fit_lds_floats(int n_verts) { return (size_t)n_verts * (3 * KP + 24) + TABLE_TAIL + (size_t)FIT_WPB * WAVE_FLOATS; }

__device__ __forceinline__ void wave_sync() {      // LDS written by some lanes of this wave, read by others
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over the 64 lanes of N values at once: xor butterfly, every lane ends with the same bits
template <int N>
__device__ __forceinline__ void wave_sum(float (&v)[N]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float t[N];
#pragma unroll
        for (int n = 0; n < N; ++n) t[n] = __shfl_xor(v[n], o, 64);
#pragma unroll
        for (int n = 0; n < N; ++n) v[n] += t[n];
    }
}

__device__ __forceinline__ float lane_bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// b^t by squaring, in double: a function of (b, t) alone, so a call split in two computes the same corrections as the whole
__device__ __forceinline__ double ipow(double b, int t) {
    double r = 1.0;
    for (int n = 0; n < 32 && t > 0; ++n) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

__device__ __forceinline__ void copy16(float* __restrict__ dst, const float* __restrict__ src, int n4, int tid) {
    for (int i = tid; i < n4; i += FIT_WPB * 64) reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
}

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(FIT_WPB * 64) STRAPS_NO_PACKED_FP32 void fit_keypoints_kernel(
        straps_fit_model_t m, straps_fit_opts_t o, float* __restrict__ est, const float* __restrict__ est0, const float* __restrict__ targets,
        const float* __restrict__ conf, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, float* __restrict__ energy,
        float* __restrict__ grad, float* __restrict__ best_est, float* __restrict__ best_energy, float* __restrict__ kp2d, long long B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nv = m.n_verts, nk = m.n_kp;
    float* sD = lds;                               // [nv][3][224]
    float* sW = sD + nv * 3 * KP;                  // [nv][24]
    float* sJT = sW + nv * 24;                     // [24][3]
    float* sJS = sJT + 72;                         // [24][3][10]
    int* sPar = reinterpret_cast<int*>(sJS + 720);
    int* sDep = sPar + 24;
    int* sSrc = sDep + 24;
    int* sMisc = sSrc + 32;
    float* ws = reinterpret_cast<float*>(sMisc + 8) + wv * WAVE_FLOATS;

    // ---- tables, once per workgroup.  Indices are clamped into range: a damaged table gives wrong numbers, never a wild address.
    copy16(sD, m.vert_dirs, nv * (3 * KP / 4), tid);
    copy16(sW, m.vert_w, nv * 6, tid);
    copy16(sJT, m.j_template, 18, tid);
    copy16(sJS, m.j_shapedirs, 180, tid);
    if (tid < 24) {
        const int p = m.parents[tid];
        sPar[tid] = tid == 0 ? -1 : min(max(p, 0), tid - 1);
    }
    if (tid < nk) sSrc[tid] = min(max(m.kp_src[tid], 0), 23 + nv);
    __syncthreads();
    if (tid < 24) {
        int d = 0, p = sPar[tid];
        for (int n = 0; n < 24 && p >= 0; ++n) { ++d; p = sPar[p]; }
        sDep[tid] = d;
    }
    __syncthreads();
    if (tid == 0) {
        int md = 0;
        for (int j = 0; j < 24; ++j) md = max(md, sDep[j]);
        sMisc[0] = md;
    }
    __syncthreads();
    const long long body = (long long)blockIdx.x * FIT_WPB + wv;
    if (body >= B) return;                      // (no workgroup barrier below this line)
    const int max_depth = sMisc[0];

    // ---- this body's state: element lane + 64 q
    float e[3], e0[3], mo[3], vo[3], be[3], lam[3];
    bool ve[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int idx = lane + 64 * q;
        ve[q] = idx < NE;
        const long long a = body * NE + (ve[q] ? idx : 0);
        e[q] = est[a];
        e0[q] = est0 ? est0[a] : e[q];      // (the priors do not hold the camera: what is loaded for the cam columns and the padding is never used)
        mo[q] = exp_avg ? exp_avg[a] : 0.f;
        vo[q] = exp_avg_sq ? exp_avg_sq[a] : 0.f;
        be[q] = e[q];
        lam[q] = (idx < 3 || !ve[q]) ? 0.f : (idx < 147 ? o.lambda_pose : o.lambda_shape);
    }
    float best_e = 0.f;

    // ---- this body's targets: keypoint lane k
    const bool vk = lane < nk;
    float that_x = 0.f, that_y = 0.f, wk = 0.f;
    int src = 0;
    if (vk) {
        const long long a = body * nk + lane;
        const float t0 = targets[a * 2], t1 = targets[a * 2 + 1];
        const float c = conf ? conf[a] : 1.f;
        if (c > 0.f && finite_f(c) && finite_f(t0) && finite_f(t1)) {
            wk = c * c;
            that_x = 2.f * t0 / o.img_wh - 1.f;
            that_y = 2.f * t1 / o.img_wh - 1.f;
        }
        src = sSrc[lane];
    }

    // ---- joint lane j (lanes 24..63 shadow joint 0; nothing of theirs is used)
    const bool vj = lane < 24;
    const int jj = vj ? lane : 0;
    const int par = sPar[jj], dep = sDep[jj];
    const int plane = par < 0 ? 0 : par;
    const float sig2 = o.robust_sigma * o.robust_sigma;
    const bool robust = o.robust_sigma > 0.f;

    for (int it = 0;; ++it) {
        // ================================ evaluation at e ================================
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (ve[q]) ws[W_EST + lane + 64 * q] = e[q];
        wave_sync();
        const float cs = ws[W_EST + 0], ctx = ws[W_EST + 1], cty = ws[W_EST + 2];
        float beta[10];
#pragma unroll
        for (int l = 0; l < 10; ++l) beta[l] = ws[W_EST + 147 + l];
        // Gram-Schmidt (interleaved layout, 1e-12 clamps: straps_rot6d_fwd)
        const float* x6 = ws + W_EST + 3 + 6 * jj;
        const float a1x = x6[0], a2x = x6[1], a1y = x6[2], a2y = x6[3], a1z = x6[4], a2z = x6[5];
        const float s1 = sqrtf(fmaf(a1z, a1z, fmaf(a1y, a1y, a1x * a1x)));
        const float n1 = fmaxf(s1, 1e-12f);
        const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
        const float dd = fmaf(b1z, a2z, fmaf(b1y, a2y, b1x * a2x));
        const float ux = fmaf(-dd, b1x, a2x), uy = fmaf(-dd, b1y, a2y), uz = fmaf(-dd, b1z, a2z);
        const float s2 = sqrtf(fmaf(uz, uz, fmaf(uy, uy, ux * ux)));
        const float n2 = fmaxf(s2, 1e-12f);
        const float b2x = ux / n2, b2y = uy / n2, b2z = uz / n2;
        const float b3x = fmaf(b1y, b2z, -(b1z * b2y)), b3y = fmaf(b1z, b2x, -(b1x * b2z)), b3z = fmaf(b1x, b2y, -(b1y * b2x));
        const float R[9] = {b1x, b2x, b3x, b1y, b2y, b3y, b1z, b2z, b3z};
        // rest joint from the shape, relative to the parent's
        float J[3], rel[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float s = sJT[jj * 3 + c];
#pragma unroll
            for (int l = 0; l < 10; ++l) s = fmaf(sJS[(jj * 3 + c) * 10 + l], beta[l], s);
            J[c] = s;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float jp = __shfl(J[c], plane, 64);
            rel[c] = par >= 0 ? J[c] - jp : J[c];
        }
        // chain by tree depth: G = [GR | Gt], PR = the parent's rotation it was composed with
        float GR[9], Gt[3], PR[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) { GR[q] = R[q]; PR[q] = (q == 0 || q == 4 || q == 8) ? 1.f : 0.f; }
#pragma unroll
        for (int c = 0; c < 3; ++c) Gt[c] = rel[c];
        for (int d = 1; d <= max_depth; ++d) {
            float P[12];
#pragma unroll
            for (int q = 0; q < 9; ++q) P[q] = __shfl(GR[q], plane, 64);
#pragma unroll
            for (int c = 0; c < 3; ++c) P[9 + c] = __shfl(Gt[c], plane, 64);
            if (dep == d) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float p0 = P[r * 3 + 0], p1 = P[r * 3 + 1], p2 = P[r * 3 + 2];
                    PR[r * 3 + 0] = p0; PR[r * 3 + 1] = p1; PR[r * 3 + 2] = p2;
                    GR[r * 3 + 0] = fmaf(p2, R[6], fmaf(p1, R[3], p0 * R[0]));
                    GR[r * 3 + 1] = fmaf(p2, R[7], fmaf(p1, R[4], p0 * R[1]));
                    GR[r * 3 + 2] = fmaf(p2, R[8], fmaf(p1, R[5], p0 * R[2]));
                    Gt[r] = fmaf(p2, rel[2], fmaf(p1, rel[1], fmaf(p0, rel[0], P[9 + r])));
                }
            }
        }
        if (vj) {
#pragma unroll
            for (int c = 0; c < 3; ++c) ws[W_GT + lane * 3 + c] = Gt[c];
            if (lane >= 1) {
#pragma unroll
                for (int q = 0; q < 9; ++q) ws[W_F + 11 + (lane - 1) * 9 + q] = R[q] - ((q == 0 || q == 4 || q == 8) ? 1.f : 0.f);
            } else {
                ws[W_F] = 1.f;
#pragma unroll
                for (int l = 0; l < 10; ++l) ws[W_F + 1 + l] = beta[l];
#pragma unroll
                for (int q = 218; q < KP; ++q) ws[W_F + q] = 0.f;
            }
        }
        wave_sync();
        // tracked vertices: blend (K split over the lanes), then dense skinning (joints over the lanes)
        float Fk[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) Fk[s] = (s < 3 || lane < 32) ? ws[W_F + lane + 64 * s] : 0.f;
        for (int i = 0; i < nv; ++i) {
            float vp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* Drow = sD + (i * 3 + c) * KP + lane;
                float s = Fk[0] * Drow[0];
                s = fmaf(Fk[1], Drow[64], s);
                s = fmaf(Fk[2], Drow[128], s);
                if (lane < 32) s = fmaf(Fk[3], Drow[192], s);
                vp[c] = s;
            }
            wave_sum(vp);
            const float w = vj ? sW[i * 24 + jj] : 0.f;
            const float d0 = vp[0] - J[0], d1 = vp[1] - J[1], d2 = vp[2] - J[2];
            float X[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) X[r] = w * fmaf(GR[r * 3 + 2], d2, fmaf(GR[r * 3 + 1], d1, fmaf(GR[r * 3 + 0], d0, Gt[r])));
            wave_sum(X);
            if (lane < 3) {
                ws[W_VP + i * 3 + lane] = lane == 0 ? vp[0] : (lane == 1 ? vp[1] : vp[2]);
                ws[W_XV + i * 3 + lane] = lane == 0 ? X[0] : (lane == 1 ? X[1] : X[2]);
            }
        }
        wave_sync();
        // keypoints: projection, residual, robust weight; the priors; the energy
        const float* Xs = src < 24 ? ws + W_GT + src * 3 : ws + W_XV + (src - 24) * 3;
        const float qx = vk ? Xs[0] + ctx : 0.f, qy = vk ? Xs[1] + cty : 0.f;
        const float px = cs * qx, py = cs * qy;
        float part[4] = {0.f, 0.f, 0.f, 0.f};      // energy, dE/ds, sum gx, sum gy
        float gx = 0.f, gy = 0.f;
        if (wk > 0.f) {
            const float rx = px - that_x, ry = py - that_y;
            const float r2 = fmaf(ry, ry, rx * rx);
            float rho = r2, drho = 1.f;
            if (robust) {
                const float den = sig2 + r2;
                rho = sig2 * r2 / den;
                drho = (sig2 / den) * (sig2 / den);
            }
            part[0] = wk * rho;
            const float g2 = 2.f * wk * drho;
            gx = g2 * rx;
            gy = g2 * ry;
            part[1] = fmaf(gy, qy, gx * qx);
            part[2] = gx;
            part[3] = gy;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float dp = (lane + 64 * q >= 3 && lane + 64 * q < NE) ? e[q] - e0[q] : 0.f;      // (cam and padding lanes: no prior term at all)
            part[0] = fmaf(lam[q] * dp, dp, part[0]);
        }
        wave_sum(part);
        const float E = part[0];
        if (vk) {
            ws[W_GX + lane * 2] = cs * gx;
            ws[W_GX + lane * 2 + 1] = cs * gy;
        }
        wave_sync();

        // ================================ gradient ================================
        // keypoints -> joints (kinematic) and -> tracked vertices, in keypoint order
        float gGR[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gGt[2] = {0.f, 0.f}, gJ[3] = {0.f, 0.f, 0.f};      // rows 0, 1 only: dE/dX has no z
        float gxv0 = 0.f, gxv1 = 0.f;
        for (int k = 0; k < nk; ++k) {
            const int s = sSrc[k];
            const float g0 = ws[W_GX + k * 2], g1 = ws[W_GX + k * 2 + 1];
            if (s < 24 && s == lane) { gGt[0] += g0; gGt[1] += g1; }     // joint lane s: a kinematic keypoint
            if (s - 24 == lane) { gxv0 += g0; gxv1 += g1; }             // lane i < 16: tracked vertex i
        }
        if (lane < 16) { ws[W_GXV + lane * 2] = gxv0; ws[W_GXV + lane * 2 + 1] = gxv1; }
        wave_sync();
        float gF[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < nv; ++i) {
            const float g0 = ws[W_GXV + i * 2], g1 = ws[W_GXV + i * 2 + 1];
            const float w = vj ? sW[i * 24 + jj] : 0.f;
            const float wg0 = w * g0, wg1 = w * g1;
            const float d[3] = {ws[W_VP + i * 3] - J[0], ws[W_VP + i * 3 + 1] - J[1], ws[W_VP + i * 3 + 2] - J[2]};
            gGt[0] += wg0;
            gGt[1] += wg1;
            float u[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gGR[c] = fmaf(wg0, d[c], gGR[c]);
                gGR[3 + c] = fmaf(wg1, d[c], gGR[3 + c]);
                u[c] = fmaf(GR[3 + c], wg1, GR[c] * wg0);        // w GR^T gX
                gJ[c] -= u[c];
            }
            wave_sum(u);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* Drow = sD + (i * 3 + c) * KP + lane;
                gF[0] = fmaf(u[c], Drow[0], gF[0]);
                gF[1] = fmaf(u[c], Drow[64], gF[1]);
                gF[2] = fmaf(u[c], Drow[128], gF[2]);
                if (lane < 32) gF[3] = fmaf(u[c], Drow[192], gF[3]);
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < 3 || lane < 32) ws[W_GF + lane + 64 * s] = gF[s];
        wave_sync();
        float gR[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) gR[q] = (vj && lane >= 1) ? ws[W_GF + 11 + (jj - (jj > 0 ? 1 : 0)) * 9 + q] : 0.f;
        // the chain's transpose, children before parents (a child's index is above its parent's): joint j's (gGR, gGt) is final when its turn comes
#pragma unroll
        for (int j = 23; j >= 1; --j) {
            float c[11];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc)
                    c[r * 3 + cc] = fmaf(gGt[r], rel[cc], fmaf(gGR[r * 3 + 2], R[cc * 3 + 2], fmaf(gGR[r * 3 + 1], R[cc * 3 + 1], gGR[r * 3] * R[cc * 3])));
            c[6] = gGt[0];
            c[7] = gGt[1];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) c[8 + cc] = fmaf(PR[3 + cc], gGt[1], PR[cc] * gGt[0]);      // d/d rel_j = PR^T gGt
#pragma unroll
            for (int q = 0; q < 11; ++q) c[q] = lane_bcast(c[q], j);
            if (lane == sPar[j]) {
#pragma unroll
                for (int q = 0; q < 6; ++q) gGR[q] += c[q];
                gGt[0] += c[6];
                gGt[1] += c[7];
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) gJ[cc] -= c[8 + cc];
            }
        }
        if (par >= 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) gR[a * 3 + b] += fmaf(PR[3 + a], gGR[3 + b], PR[a] * gGR[b]);
                gJ[a] += fmaf(PR[3 + a], gGt[1], PR[a] * gGt[0]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 6; ++q) gR[q] += gGR[q];
            gJ[0] += gGt[0];
            gJ[1] += gGt[1];
        }
        // Gram-Schmidt's transpose
        {
            float g1x = gR[0], g1y = gR[3], g1z = gR[6], g2x = gR[1], g2y = gR[4], g2z = gR[7];
            const float g3x = gR[2], g3y = gR[5], g3z = gR[8];
            // b3 = b1 x b2
            g1x += fmaf(b2y, g3z, -(b2z * g3y)); g1y += fmaf(b2z, g3x, -(b2x * g3z)); g1z += fmaf(b2x, g3y, -(b2y * g3x));
            g2x += fmaf(g3y, b1z, -(g3z * b1y)); g2y += fmaf(g3z, b1x, -(g3x * b1z)); g2z += fmaf(g3x, b1y, -(g3y * b1x));
            // b2 = u / n2
            const float t2 = s2 < 1e-12f ? 0.f : fmaf(b2z, g2z, fmaf(b2y, g2y, b2x * g2x));
            const float gux = fmaf(-t2, b2x, g2x) / n2, guy = fmaf(-t2, b2y, g2y) / n2, guz = fmaf(-t2, b2z, g2z) / n2;
            // u = a2 - d b1, d = b1 . a2
            const float gd = -fmaf(guz, b1z, fmaf(guy, b1y, gux * b1x));
            g1x += fmaf(gd, a2x, -(dd * gux)); g1y += fmaf(gd, a2y, -(dd * guy)); g1z += fmaf(gd, a2z, -(dd * guz));
            const float ga2x = fmaf(gd, b1x, gux), ga2y = fmaf(gd, b1y, guy), ga2z = fmaf(gd, b1z, guz);
            // b1 = a1 / n1
            const float t1 = s1 < 1e-12f ? 0.f : fmaf(b1z, g1z, fmaf(b1y, g1y, b1x * g1x));
            const float ga1x = fmaf(-t1, b1x, g1x) / n1, ga1y = fmaf(-t1, b1y, g1y) / n1, ga1z = fmaf(-t1, b1z, g1z) / n1;
            if (vj) {
                float* ge = ws + W_GE + 3 + 6 * lane;
                ge[0] = ga1x; ge[1] = ga2x; ge[2] = ga1y; ge[3] = ga2y; ge[4] = ga1z; ge[5] = ga2z;
            }
        }
        // shape: through the rest joints and through the blend
        float gb[10];
#pragma unroll
        for (int l = 0; l < 10; ++l)
            gb[l] = vj ? fmaf(gJ[2], sJS[(jj * 3 + 2) * 10 + l], fmaf(gJ[1], sJS[(jj * 3 + 1) * 10 + l], gJ[0] * sJS[(jj * 3) * 10 + l])) : 0.f;
        wave_sum(gb);
        if (lane < 10) {
            float t = gb[0];
#pragma unroll
            for (int l = 1; l < 10; ++l) t = lane == l ? gb[l] : t;
            ws[W_GE + 147 + lane] = t + ws[W_GF + 1 + lane];
        }
        if (lane == 0) {
            ws[W_GE + 0] = part[1];
            ws[W_GE + 1] = cs * part[2];
            ws[W_GE + 2] = cs * part[3];
        }
        wave_sync();
        float g[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) g[q] = !ve[q] ? 0.f : (lane + 64 * q >= 3 ? fmaf(2.f * lam[q], e[q] - e0[q], ws[W_GE + lane + 64 * q]) : ws[W_GE + lane + 64 * q]);

        // ================================ bookkeeping, then the update ================================
        if (energy && lane == 0) energy[body * (long long)(o.iters + 1) + it] = E;
        if (it == 0 || E < best_e) {        // the first minimum wins; a NaN never replaces what is held
            best_e = E;
#pragma unroll
            for (int q = 0; q < 3; ++q) be[q] = e[q];
        }
        if (it >= o.iters) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (ve[q] && grad) grad[body * NE + lane + 64 * q] = g[q];
            if (vk && kp2d) {
                kp2d[(body * nk + lane) * 2] = px;
                kp2d[(body * nk + lane) * 2 + 1] = py;
            }
            break;
        }
        const int t = o.step0 + it + 1;
        // the formula of adam_kernel (csrc/train.hip): bias corrections in double (b^t by squaring here, pow() there: the step sizes may differ
        // in the last bit), the element update in float
        const double bc1 = 1.0 - ipow((double)o.beta1, t);
        const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - ipow((double)o.beta2, t)));
        const float ss_cam = (float)((double)o.lr_cam / bc1), ss_pose = (float)((double)o.lr_pose / bc1), ss_shape = (float)((double)o.lr_shape / bc1);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int idx = lane + 64 * q;
            const float step_size = idx < 3 ? ss_cam : (idx < 147 ? ss_pose : ss_shape);
            const float mi = o.beta1 * mo[q] + (1.f - o.beta1) * g[q];
            const float vi = o.beta2 * vo[q] + (1.f - o.beta2) * g[q] * g[q];
            mo[q] = mi;
            vo[q] = vi;
            e[q] -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + o.eps);
        }
    }

#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (!ve[q]) continue;
        const long long a = body * NE + lane + 64 * q;
        est[a] = e[q];
        if (exp_avg) { exp_avg[a] = mo[q]; exp_avg_sq[a] = vo[q]; }
        if (best_est) best_est[a] = be[q];
    }
    if (best_energy && lane == 0) best_energy[body] = best_e;
}

}  // namespace

extern "C" int straps_fit_keypoints(const straps_fit_model_t* model, const straps_fit_opts_t* opts, float* est, const float* est0,
                                    const float* targets, const float* conf, float* exp_avg, float* exp_avg_sq, float* energy, float* grad,
                                    float* best_est, float* best_energy, float* kp2d, long long batch, void* stream) {
    STRAPS_REQUIRE(model && opts, "straps_fit_keypoints: null model or opts");
    STRAPS_REQUIRE(est && targets, "straps_fit_keypoints: null pointer (est, targets)");
    STRAPS_REQUIRE(batch > 0 && batch <= (1LL << 31) - 4, "straps_fit_keypoints: batch must be in 1..2^31-4 (got %lld)", batch);
    STRAPS_REQUIRE(opts->iters >= 0 && opts->iters <= 10000, "straps_fit_keypoints: iters must be in 0..10000 (got %d)", opts->iters);
    STRAPS_REQUIRE(opts->step0 >= 0 && opts->step0 <= (1 << 30), "straps_fit_keypoints: step0 must be in 0..2^30 (got %d)", opts->step0);
    STRAPS_REQUIRE(model->n_kp >= 1 && model->n_kp <= 32, "straps_fit_keypoints: n_kp must be in 1..32 (got %d)", model->n_kp);
    STRAPS_REQUIRE(model->n_verts >= 0 && model->n_verts <= 16, "straps_fit_keypoints: n_verts must be in 0..16 (got %d)", model->n_verts);
    STRAPS_REQUIRE(model->j_template && model->j_shapedirs && model->parents && model->kp_src, "straps_fit_keypoints: null table (j_template, j_shapedirs, parents, kp_src)");
    STRAPS_REQUIRE(model->n_verts == 0 || (model->vert_dirs && model->vert_w), "straps_fit_keypoints: null vert_dirs / vert_w with n_verts = %d", model->n_verts);
    STRAPS_REQUIRE((((uintptr_t)model->j_template | (uintptr_t)model->j_shapedirs | (uintptr_t)model->vert_dirs | (uintptr_t)model->vert_w) & 15) == 0,
                   "straps_fit_keypoints: j_template, j_shapedirs, vert_dirs and vert_w must be 16-byte aligned");
    STRAPS_REQUIRE((exp_avg == nullptr) == (exp_avg_sq == nullptr), "straps_fit_keypoints: exp_avg and exp_avg_sq must be given together");
    STRAPS_REQUIRE(opts->img_wh > 0.f && opts->beta1 >= 0.f && opts->beta1 < 1.f && opts->beta2 >= 0.f && opts->beta2 < 1.f && opts->eps > 0.f,
                   "straps_fit_keypoints: img_wh and eps must be positive, beta1 and beta2 in [0, 1)");
    STRAPS_REQUIRE(opts->lambda_pose >= 0.f && opts->lambda_shape >= 0.f && opts->robust_sigma >= 0.f, "straps_fit_keypoints: lambda_pose, lambda_shape and robust_sigma must not be negative");
    static_assert(((size_t)16 * (3 * KP + 24) + TABLE_TAIL + (size_t)FIT_WPB * WAVE_FLOATS) * sizeof(float) <= (64u << 10), "the largest table set must fit the default dynamic LDS limit");
    const size_t lds_bytes = fit_lds_floats(model->n_verts) * sizeof(float);
    const unsigned blocks = (unsigned)((batch + FIT_WPB - 1) / FIT_WPB);
    hipLaunchKernelGGL(fit_keypoints_kernel, dim3(blocks), dim3(FIT_WPB * 64), lds_bytes, (hipStream_t)stream, *model, *opts, est, est0, targets, conf,
                       exp_avg, exp_avg_sq, energy, grad, best_est, best_energy, kp2d, batch);
    STRAPS_CHECK_LAUNCH("fit_keypoints_kernel");
    return STRAPS_OK;
}
