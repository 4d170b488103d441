// measure_bwd.hip -- the gradient of straps_measure_mesh (csrc/measure.hip) w.r.t. the vertices and the anchor points, and the energy head of a
// shape fit to known measurements (include/straps_hip.h states both).  The vertices are read as fp32; every product, sum, division and square
// root of the gradient is done in double; each output element is rounded to float once, after all its terms are added.  A GATHER: no
// floating-point atomics, no allocation, no synchronisation, nothing read that the call has not written.
//
// Two launches per straps_measure_mesh_bwd call, both on the caller's stream:
//   1. partial kernel : shaped like the forward's.  FACE blocks (512 faces of one body, launched only when a GIRTH or a VOLUME with a centre is
//                       asked for) write, per such measurement, the block's sum of the faces' gradients w.r.t. the ANCHOR (three doubles, the
//                       forward's fixed shuffle tree per component).  VERTEX blocks (2048 vertices, launched only for an EXTENT) write
//                       (max, min, lowest index of the max, lowest index of the min) of dir . p.
//   2. gather kernel  : workgroup (body, 256 vertices), one thread per vertex.  n_meas threads first stage dout, the first anchors and the
//                       EXTENT extremes of the body (vertex partials combined in index order) in LDS.  A thread then walks its vertex's
//                       incident faces through the CSR table, four faces' indices and corners in flight, adds per face -- in table order --
//                       the terms of all measurements in measurement order, then the terms the vertex gets as an anchor or an extent extreme
//                       in measurement order (anchor partials summed in index order, eight loads in flight), and stores three floats.  One
//                       more workgroup per body finishes the points: thread j owns row j of dpoints.
// The order of the terms of an output element depends on the topology and the measurement list alone; a workgroup touches one body.
#include "common.h"

#include <string.h>

namespace {

constexpr int MB_THREADS = 256;
constexpr int MB_FACES_PER_BLOCK = 512;       // == the forward's (hipabi.MEASURE_FACES_PER_BLOCK)
constexpr int MB_VERTS_PER_BLOCK = 2048;      // == the forward's (hipabi.MEASURE_VERTS_PER_BLOCK)
constexpr int MB_FPT = MB_FACES_PER_BLOCK / MB_THREADS;
constexpr int MB_VPT = MB_VERTS_PER_BLOCK / MB_THREADS;
constexpr int MB_MAX_MEAS = 32;
constexpr int MB_MAX_POINTS = 64;
constexpr int MB_MAX_VERTS = 1 << 20;
constexpr int MB_FACE_SLOT = 3;               // doubles per (face block, measurement): the anchor gradient
constexpr int MB_VERT_SLOT = 4;               // doubles per (vertex block, measurement): max, min, index of the max, index of the min
constexpr int MB_INFLIGHT = 4;                // incident faces whose indices and corners a gather thread loads before it computes
constexpr int MB_NO_INDEX = 0x7fffffff;

struct MeasPackB {
    straps_measure_t m[MB_MAX_MEAS];
};

__device__ __forceinline__ bool is_face_kind(int kind) { return kind == STRAPS_MEASURE_VOLUME || kind == STRAPS_MEASURE_AREA || kind == STRAPS_MEASURE_GIRTH; }
// the measurements whose anchor receives a gradient from every selected face (the host has set anchor[0] = -1 for a VOLUME about the origin)
__device__ __forceinline__ bool has_face_anchor(const straps_measure_t& q) {
    return q.kind == STRAPS_MEASURE_GIRTH || (q.kind == STRAPS_MEASURE_VOLUME && q.anchor[0] >= 0);
}

__device__ __forceinline__ const float* anchor_ptr(const float* __restrict__ vb, const float* __restrict__ pb, int a, int nverts) {
    return a < nverts ? vb + (long long)a * 3 : pb + (long long)(a - nverts) * 3;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// (value, index) extremes: a NaN wins and stays (the forward's max / min propagate it); among equal values the lower index wins
__device__ __forceinline__ void take_max(double& a, int& ia, double b, int ib) {
    if (b > a || (b != b && a == a) || (b == a && ib < ia)) { a = b; ia = ib; }
}
__device__ __forceinline__ void take_min(double& a, int& ia, double b, int ib) {
    if (b < a || (b != b && a == a) || (b == a && ib < ia)) { a = b; ia = ib; }
}

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// The gradients of one selected face's term of measurement q (as the forward's face_term scales it: VOLUME / 6, AREA / 2 included):
// g[i] w.r.t. corner i, go w.r.t. the anchor `o` (zero for an AREA).  false: the face contributes nothing (an AREA face with |n|^2 == 0, a
// GIRTH face that is not cut or whose section length is exactly 0); g and go are then not to be used.
__device__ __forceinline__ bool face_grads(const straps_measure_t& q, const double (&P)[3][3], const double (&o)[3], double (&g)[3][3], double (&go)[3]) {
    if (q.kind == STRAPS_MEASURE_VOLUME) {
        double r[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) r[i][c] = P[i][c] - o[c];
        cross3(r[1], r[2], g[0]);
        cross3(r[2], r[0], g[1]);
        cross3(r[0], r[1], g[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g[0][c] *= 1.0 / 6.0;
            g[1][c] *= 1.0 / 6.0;
            g[2][c] *= 1.0 / 6.0;
            go[c] = -((g[0][c] + g[1][c]) + g[2][c]);
        }
        return true;
    }
    if (q.kind == STRAPS_MEASURE_AREA) {
        double e1[3], e2[3], n[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            e1[c] = P[1][c] - P[0][c];
            e2[c] = P[2][c] - P[0][c];
        }
        cross3(e1, e2, n);
        const double n2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
        if (n2 == 0.0) return false;
        const double inv = 0.5 / sqrt(n2);
        double h[3], w[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            h[c] = n[c] * inv;                    // n / (2 |n|)
            w[0][c] = P[2][c] - P[1][c];
            w[1][c] = P[0][c] - P[2][c];
            w[2][c] = e1[c];
            go[c] = 0.0;
        }
        cross3(h, w[0], g[0]);
        cross3(h, w[1], g[1]);
        cross3(h, w[2], g[2]);
        return true;
    }
    // GIRTH: the forward's side tests and lone vertex
    const double n[3] = {(double)q.dir[0], (double)q.dir[1], (double)q.dir[2]};
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = (n[0] * (P[i][0] - o[0]) + n[1] * (P[i][1] - o[1])) + n[2] * (P[i][2] - o[2]);
    const bool s0 = d[0] >= 0.0, s1 = d[1] >= 0.0, s2 = d[2] >= 0.0;
    if (s0 == s1 && s1 == s2) return false;
    const int a = (s1 == s2) ? 0 : ((s0 == s2) ? 1 : 2);
    double A[3], B[3], C[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A[c] = a == 0 ? P[0][c] : (a == 1 ? P[1][c] : P[2][c]);
        B[c] = a == 0 ? P[1][c] : (a == 1 ? P[2][c] : P[0][c]);
        C[c] = a == 0 ? P[2][c] : (a == 1 ? P[0][c] : P[1][c]);
    }
    const double da = a == 0 ? d[0] : (a == 1 ? d[1] : d[2]);
    const double db = a == 0 ? d[1] : (a == 1 ? d[2] : d[0]);
    const double dc = a == 0 ? d[2] : (a == 1 ? d[0] : d[1]);
    // (two reciprocals serve t, s / D and s / D^2: the divisions are what a wave with one cut face among its lanes waits for)
    const double rb = 1.0 / (da - db), rc = 1.0 / (da - dc);
    const double tb = da * rb, tc = da * rc;
    double e[3], len2 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double xb = A[c] + tb * (B[c] - A[c]);
        const double xc = A[c] + tc * (C[c] - A[c]);
        e[c] = xb - xc;
        len2 += e[c] * e[c];
    }
    if (len2 == 0.0) return false;
    // L = |x_b - x_c| with u = (x_b - x_c) / L, s_b = u . (B - A), s_c = u . (C - A), t_b = d_a / D_b, t_c = d_a / D_c:
    //   dL/dA = u (t_c - t_b) + n (s_c d_c / D_c^2 - s_b d_b / D_b^2)      dL/dB = u t_b + n s_b d_a / D_b^2
    //   dL/dC = -u t_c - n s_c d_a / D_c^2                                   dL/do = -n (s_b / D_b - s_c / D_c)
    const double invl = 1.0 / sqrt(len2);
    double u[3], sb = 0.0, sc = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        u[c] = e[c] * invl;
        sb += u[c] * (B[c] - A[c]);
        sc += u[c] * (C[c] - A[c]);
    }
    const double qb = sb * rb, qc = sc * rc;      // s / D
    const double kb = qb * rb, kc = qc * rc;      // s / D^2
    const double na = kc * dc - kb * db, nb = kb * da, nc = -(kc * da), no = qc - qb;
    double GA[3], GB[3], GC[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        GA[c] = u[c] * (tc - tb) + n[c] * na;
        GB[c] = u[c] * tb + n[c] * nb;
        GC[c] = n[c] * nc - u[c] * tc;
        go[c] = n[c] * no;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g[0][c] = a == 0 ? GA[c] : (a == 1 ? GC[c] : GB[c]);      // corner i has the role (i - a) mod 3 of (A, B, C)
        g[1][c] = a == 0 ? GB[c] : (a == 1 ? GA[c] : GC[c]);
        g[2][c] = a == 0 ? GC[c] : (a == 1 ? GB[c] : GA[c]);
    }
    return true;
}

__global__ __launch_bounds__(MB_THREADS) STRAPS_NO_PACKED_FP32 void measure_bwd_partial_kernel(const float* __restrict__ verts, const float* __restrict__ points,
                                                                                              const int32_t* __restrict__ faces,
                                                                                              const uint8_t* __restrict__ face_parts, const MeasPackB mp,
                                                                                              double* __restrict__ ws, int nverts, int n_points, int nfaces,
                                                                                              int n_meas, int nfb, int nvb, int fb_run, int vb_run) {
    __shared__ double red[MB_MAX_MEAS][4][MB_THREADS / 64];
    __shared__ int redi[MB_MAX_MEAS][2][MB_THREADS / 64];
    __shared__ float anc[MB_MAX_MEAS][3];
    const int per_body = fb_run + vb_run;
    const long long b = blockIdx.x / per_body;
    const int k = (int)(blockIdx.x - b * per_body);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* vb = verts + b * nverts * 3;
    const float* pb = points ? points + b * n_points * 3 : nullptr;
    double* wb = ws + b * (long long)n_meas * (MB_FACE_SLOT * nfb + MB_VERT_SLOT * nvb);      // [nfb][n_meas][3], then [nvb][n_meas][4]
    if (tid < n_meas) {
        float x = 0.f, y = 0.f, z = 0.f;
        if (has_face_anchor(mp.m[tid])) {
            const float* ap = anchor_ptr(vb, pb, mp.m[tid].anchor[0], nverts);
            x = ap[0]; y = ap[1]; z = ap[2];
        }
        anc[tid][0] = x; anc[tid][1] = y; anc[tid][2] = z;
    }
    __syncthreads();

    if (k < fb_run) {
        // ---- a face block: corners once, then the anchor gradient of every GIRTH and centred VOLUME
        double P[MB_FPT][3][3];
        bool ok[MB_FPT];
        unsigned part_bit[MB_FPT];
#pragma unroll
        for (int j = 0; j < MB_FPT; ++j) {
            const int f = k * MB_FACES_PER_BLOCK + j * MB_THREADS + tid;      // < nfaces + 512 <= 2^31 / 3 + 512
            ok[j] = false;
            part_bit[j] = 0u;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) P[j][i][c] = 0.0;
            if (f < nfaces) {
                const int i0 = faces[(long long)f * 3 + 0], i1 = faces[(long long)f * 3 + 1], i2 = faces[(long long)f * 3 + 2];
                if ((unsigned)i0 < (unsigned)nverts && (unsigned)i1 < (unsigned)nverts && (unsigned)i2 < (unsigned)nverts) {
                    ok[j] = true;
                    const int idx[3] = {i0, i1, i2};
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int c = 0; c < 3; ++c) P[j][i][c] = (double)vb[(long long)idx[i] * 3 + c];
                    if (face_parts) {
                        const unsigned lab = face_parts[f];
                        part_bit[j] = lab < 32u ? (1u << lab) : 0u;
                    }
                }
            }
        }
        for (int m = 0; m < n_meas; ++m) {
            const straps_measure_t& q = mp.m[m];
            if (!has_face_anchor(q)) continue;                 // (uniform over the workgroup)
            const double o[3] = {(double)anc[m][0], (double)anc[m][1], (double)anc[m][2]};
            double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < MB_FPT; ++j) {
                const bool sel = ok[j] && (q.part_mask == 0u || (part_bit[j] & q.part_mask) != 0u);
                double g[3][3], go[3];
                if (sel && face_grads(q, P[j], o, g, go)) {
                    acc[0] += go[0];
                    acc[1] += go[1];
                    acc[2] += go[2];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double s = wave_sum(acc[c]);
                if (lane == 0) red[m][c][wave] = s;
            }
        }
        __syncthreads();
        if (tid < n_meas && has_face_anchor(mp.m[tid])) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double s = red[tid][c][0];
#pragma unroll
                for (int w = 1; w < MB_THREADS / 64; ++w) s += red[tid][c][w];
                wb[((long long)k * n_meas + tid) * MB_FACE_SLOT + c] = s;
            }
        }
        return;
    }

    // ---- a vertex block: (max, min) of dir . p per EXTENT, each with the lowest vertex index that attains it
    const int kv = k - fb_run;
    double V[MB_VPT][3];
    int vid[MB_VPT];
#pragma unroll
    for (int j = 0; j < MB_VPT; ++j) {
        const int v = kv * MB_VERTS_PER_BLOCK + j * MB_THREADS + tid;      // < 2^20 + 2048
        vid[j] = v < nverts ? v : -1;
#pragma unroll
        for (int c = 0; c < 3; ++c) V[j][c] = v < nverts ? (double)vb[(long long)v * 3 + c] : 0.0;
    }
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    for (int m = 0; m < n_meas; ++m) {
        const straps_measure_t& q = mp.m[m];
        if (q.kind != STRAPS_MEASURE_EXTENT) continue;
        const double nx = (double)q.dir[0], ny = (double)q.dir[1], nz = (double)q.dir[2];
        double mx = -inf, mn = inf;
        int imx = MB_NO_INDEX, imn = MB_NO_INDEX;
#pragma unroll
        for (int j = 0; j < MB_VPT; ++j) {
            if (vid[j] >= 0) {
                const double h = (nx * V[j][0] + ny * V[j][1]) + nz * V[j][2];
                take_max(mx, imx, h, vid[j]);
                take_min(mn, imn, h, vid[j]);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double omx = __shfl_down(mx, off, 64), omn = __shfl_down(mn, off, 64);
            const int oimx = __shfl_down(imx, off, 64), oimn = __shfl_down(imn, off, 64);
            take_max(mx, imx, omx, oimx);
            take_min(mn, imn, omn, oimn);
        }
        if (lane == 0) {
            red[m][0][wave] = mx;
            red[m][1][wave] = mn;
            redi[m][0][wave] = imx;
            redi[m][1][wave] = imn;
        }
    }
    __syncthreads();
    if (tid < n_meas && mp.m[tid].kind == STRAPS_MEASURE_EXTENT) {
        double mx = red[tid][0][0], mn = red[tid][1][0];
        int imx = redi[tid][0][0], imn = redi[tid][1][0];
#pragma unroll
        for (int w = 1; w < MB_THREADS / 64; ++w) {
            take_max(mx, imx, red[tid][0][w], redi[tid][0][w]);
            take_min(mn, imn, red[tid][1][w], redi[tid][1][w]);
        }
        double* e = wb + (long long)nfb * n_meas * MB_FACE_SLOT + ((long long)kv * n_meas + tid) * MB_VERT_SLOT;
        e[0] = mx;
        e[1] = mn;
        e[2] = (double)imx;      // (< 2^31: exact)
        e[3] = (double)imn;
    }
}

// partials of one (body, measurement, component), `stride` doubles apart, added in index order; eight loads in flight per trip, as the
// forward's sum_in_order (one after the other they cost a round trip to memory each)
__device__ __forceinline__ double sum_in_order(const double* __restrict__ p, int count, long long stride) {
    double r = 0.0;
    for (int k = 0; k < count; k += 8) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = k + u < count ? p[(long long)(k + u) * stride] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k + u < count) r += t[u];
    }
    return r;
}

// what anchor `a` (a vertex id, or nverts + j for point j) receives beyond its face terms, added in measurement order: the anchor gradient
// of a centred VOLUME or a GIRTH, the EXTENT terms of an extreme vertex, the unit segment vectors of a PATH
__device__ __forceinline__ void add_anchor_terms(double (&acc)[3], int a, const MeasPackB& mp, const double* __restrict__ s_dout, const int* __restrict__ ext_hi,
                                                 const int* __restrict__ ext_lo, const double* __restrict__ wb, const float* __restrict__ vb,
                                                 const float* __restrict__ pb, int nverts, int n_meas, int nfb) {
    for (int m = 0; m < n_meas; ++m) {
        const straps_measure_t& q = mp.m[m];
        const double d = s_dout[m];
        if (has_face_anchor(q)) {
            if (q.anchor[0] != a) continue;
            const double* p = wb + (long long)m * MB_FACE_SLOT;
            const long long stride = (long long)n_meas * MB_FACE_SLOT;
            const double gx = sum_in_order(p, nfb, stride), gy = sum_in_order(p + 1, nfb, stride), gz = sum_in_order(p + 2, nfb, stride);
            acc[0] += d * gx;
            acc[1] += d * gy;
            acc[2] += d * gz;
        } else if (q.kind == STRAPS_MEASURE_EXTENT) {
            if (a == ext_hi[m]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += (double)q.dir[c] * d;
            }
            if (a == ext_lo[m]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] -= (double)q.dir[c] * d;
            }
        } else if (q.kind == STRAPS_MEASURE_PATH) {
            // position j of the polyline: +unit(A_j - A_(j-1)) from the segment that ends there, -unit(A_(j+1) - A_j) from the one that starts there
            for (int j = 0; j < 4 && q.anchor[j] >= 0; ++j) {
                if (q.anchor[j] != a) continue;
                const float* me = anchor_ptr(vb, pb, a, nverts);
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    const int jo = side == 0 ? j - 1 : j + 1;
                    if (jo < 0 || jo > 3 || q.anchor[jo] < 0) continue;
                    const float* ot = anchor_ptr(vb, pb, q.anchor[jo], nverts);
                    const double dx = (double)me[0] - (double)ot[0], dy = (double)me[1] - (double)ot[1], dz = (double)me[2] - (double)ot[2];
                    const double l2 = (dx * dx + dy * dy) + dz * dz;
                    if (l2 == 0.0) continue;
                    const double s = d / sqrt(l2);
                    acc[0] += dx * s;
                    acc[1] += dy * s;
                    acc[2] += dz * s;
                }
            }
        }
    }
}

__global__ __launch_bounds__(MB_THREADS) STRAPS_NO_PACKED_FP32 void measure_bwd_gather_kernel(const float* __restrict__ verts, const float* __restrict__ points,
                                                                                             const int32_t* __restrict__ faces,
                                                                                             const uint8_t* __restrict__ face_parts,
                                                                                             const int32_t* __restrict__ vf_offsets,
                                                                                             const int32_t* __restrict__ vf_faces, const MeasPackB mp,
                                                                                             const float* __restrict__ dout, const double* __restrict__ ws,
                                                                                             float* __restrict__ dverts, float* __restrict__ dpoints, int nverts,
                                                                                             int n_points, int dpoints_rows, int nfaces, int n_meas, int nfb,
                                                                                             int nvb, int nvc, int per_body, int any_face) {
    __shared__ double s_dout[MB_MAX_MEAS];
    __shared__ float anc[MB_MAX_MEAS][3];
    __shared__ int ext_hi[MB_MAX_MEAS], ext_lo[MB_MAX_MEAS];
    const long long b = blockIdx.x / per_body;
    const int k = (int)(blockIdx.x - b * per_body);
    const int tid = threadIdx.x;
    const float* vb = verts + b * nverts * 3;
    const float* pb = points ? points + b * n_points * 3 : nullptr;
    const double* wb = ws + b * (long long)n_meas * (MB_FACE_SLOT * nfb + MB_VERT_SLOT * nvb);
    if (tid < n_meas) {
        const straps_measure_t& q = mp.m[tid];
        s_dout[tid] = (double)dout[b * n_meas + tid];
        float x = 0.f, y = 0.f, z = 0.f;
        if (has_face_anchor(q)) {
            const float* ap = anchor_ptr(vb, pb, q.anchor[0], nverts);
            x = ap[0]; y = ap[1]; z = ap[2];
        }
        anc[tid][0] = x; anc[tid][1] = y; anc[tid][2] = z;
        int hi = -1, lo = -1;
        if (q.kind == STRAPS_MEASURE_EXTENT) {
            // the vertex blocks' extremes combined in index order; a NaN extreme compares equal to no vertex
            const double* e = wb + (long long)nfb * n_meas * MB_FACE_SLOT + (long long)tid * MB_VERT_SLOT;
            const long long stride = (long long)n_meas * MB_VERT_SLOT;
            double mx = e[0], mn = e[1];
            int imx = (int)e[2], imn = (int)e[3];
            for (int kk = 1; kk < nvb; ++kk) {
                take_max(mx, imx, e[kk * stride], (int)e[kk * stride + 2]);
                take_min(mn, imn, e[kk * stride + 1], (int)e[kk * stride + 3]);
            }
            hi = mx == mx ? imx : -1;
            lo = mn == mn ? imn : -1;
        }
        ext_hi[tid] = hi;
        ext_lo[tid] = lo;
    }
    __syncthreads();

    if (k == nvc) {
        // ---- the points of the body: thread j owns row j
        if (tid < n_points) {
            double acc[3] = {0.0, 0.0, 0.0};
            add_anchor_terms(acc, nverts + tid, mp, s_dout, ext_hi, ext_lo, wb, vb, pb, nverts, n_meas, nfb);
            float* dp = dpoints + (b * dpoints_rows + tid) * 3;
            dp[0] = (float)acc[0];
            dp[1] = (float)acc[1];
            dp[2] = (float)acc[2];
        }
        return;
    }

    const int v = k * MB_THREADS + tid;
    if (v >= nverts) return;
    double acc[3] = {0.0, 0.0, 0.0};
    if (any_face) {
        const int beg = vf_offsets[v], end = vf_offsets[v + 1];
        for (int e0 = beg; e0 < end; e0 += MB_INFLIGHT) {
            // the dependent chain table -> face -> indices -> corners, MB_INFLIGHT faces wide at every stage
            int f[MB_INFLIGHT], idx[MB_INFLIGHT][3];
            float C[MB_INFLIGHT][3][3];
            unsigned part_bit[MB_INFLIGHT];
            bool ok[MB_INFLIGHT];
#pragma unroll
            for (int u = 0; u < MB_INFLIGHT; ++u) f[u] = e0 + u < end ? vf_faces[e0 + u] : -1;
#pragma unroll
            for (int u = 0; u < MB_INFLIGHT; ++u) {
                const bool in = (unsigned)f[u] < (unsigned)nfaces;
#pragma unroll
                for (int i = 0; i < 3; ++i) idx[u][i] = in ? faces[(long long)f[u] * 3 + i] : -1;
                part_bit[u] = 0u;
                if (in && face_parts) {
                    const unsigned lab = face_parts[f[u]];
                    part_bit[u] = lab < 32u ? (1u << lab) : 0u;
                }
            }
#pragma unroll
            for (int u = 0; u < MB_INFLIGHT; ++u) {
                ok[u] = (unsigned)idx[u][0] < (unsigned)nverts && (unsigned)idx[u][1] < (unsigned)nverts && (unsigned)idx[u][2] < (unsigned)nverts;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) C[u][i][c] = ok[u] ? vb[(long long)idx[u][i] * 3 + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < MB_INFLIGHT; ++u) {
                if (!ok[u]) continue;
                double P[3][3];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) P[i][c] = (double)C[u][i][c];
                for (int m = 0; m < n_meas; ++m) {
                    const straps_measure_t& q = mp.m[m];
                    if (!is_face_kind(q.kind)) continue;
                    if (!(q.part_mask == 0u || (part_bit[u] & q.part_mask) != 0u)) continue;
                    const double o[3] = {(double)anc[m][0], (double)anc[m][1], (double)anc[m][2]};
                    double g[3][3], go[3];
                    if (!face_grads(q, P, o, g, go)) continue;
                    const double d = s_dout[m];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        if (idx[u][i] == v) {      // every corner that names the vertex adds its gradient
                            acc[0] += d * g[i][0];
                            acc[1] += d * g[i][1];
                            acc[2] += d * g[i][2];
                        }
                    }
                }
            }
        }
    }
    add_anchor_terms(acc, v, mp, s_dout, ext_hi, ext_lo, wb, vb, pb, nverts, n_meas, nfb);
    float* dv = dverts + (b * nverts + v) * 3;
    dv[0] = (float)acc[0];
    dv[1] = (float)acc[1];
    dv[2] = (float)acc[2];
}

constexpr int MR_NE = 157, MR_SHAPE0 = 147;

__global__ __launch_bounds__(MB_THREADS) STRAPS_NO_PACKED_FP32 void measure_residual_kernel(const float* __restrict__ values, const float* __restrict__ targets,
                                                                                           const float* __restrict__ weights, const float* __restrict__ est,
                                                                                           const float* __restrict__ est0, float lambda_shape,
                                                                                           float* __restrict__ energy, float* __restrict__ dvalues,
                                                                                           float* __restrict__ g, long long batch, int n_meas) {
    const long long b = (long long)blockIdx.x * MB_THREADS + threadIdx.x;
    if (b >= batch) return;
    float e = 0.f;
    for (int m = 0; m < n_meas; ++m) {
        const float t = targets[b * n_meas + m];
        const float w = weights ? weights[b * n_meas + m] : 1.f;
        float dv = 0.f;
        if (isfinite(t) && t != 0.f && isfinite(w) && w > 0.f) {
            const float r = values[b * n_meas + m] / t - 1.f;
            const float wr = w * r;
            e = fmaf(wr, r, e);
            dv = (2.f * wr) / t;
        }
        dvalues[b * n_meas + m] = dv;
    }
    float p = 0.f;
    float* gb = g + b * MR_NE;
    for (int c = 0; c < MR_SHAPE0; ++c) gb[c] = 0.f;
#pragma unroll
    for (int i = 0; i < MR_NE - MR_SHAPE0; ++i) {
        const float d = est[b * MR_NE + MR_SHAPE0 + i] - est0[b * MR_NE + MR_SHAPE0 + i];
        p = fmaf(d, d, p);
        gb[MR_SHAPE0 + i] = (2.f * lambda_shape) * d;
    }
    energy[b] = fmaf(lambda_shape, p, e);
}

}  // namespace

extern "C" size_t straps_measure_bwd_workspace_bytes(long long batch, int nverts, int nfaces, int n_meas) {
    if (batch <= 0 || batch >= (1LL << 31) || nverts < 1 || nverts > MB_MAX_VERTS || nfaces < 0 || nfaces > 0x7fffffff / 3 || n_meas < 1 || n_meas > MB_MAX_MEAS) return 0;
    const size_t nfb = ((size_t)nfaces + MB_FACES_PER_BLOCK - 1) / MB_FACES_PER_BLOCK, nvb = ((size_t)nverts + MB_VERTS_PER_BLOCK - 1) / MB_VERTS_PER_BLOCK;
    return (size_t)batch * (size_t)n_meas * (MB_FACE_SLOT * nfb + MB_VERT_SLOT * nvb) * sizeof(double);
}

extern "C" int straps_measure_mesh_bwd(const float* verts, const float* points, const int32_t* faces, const uint8_t* face_parts, const int32_t* vf_offsets,
                                       const int32_t* vf_faces, const straps_measure_t* meas, const float* dout, float* dverts, float* dpoints, void* workspace,
                                       long long batch, int nverts, int n_points, int dpoints_rows, int nfaces, int n_meas, void* stream) {
    STRAPS_REQUIRE(verts, "straps_measure_mesh_bwd: `verts` is a null pointer");
    STRAPS_REQUIRE(meas, "straps_measure_mesh_bwd: `meas` is a null pointer");
    STRAPS_REQUIRE(dout, "straps_measure_mesh_bwd: `dout` is a null pointer");
    STRAPS_REQUIRE(dverts, "straps_measure_mesh_bwd: `dverts` is a null pointer");
    STRAPS_REQUIRE(workspace, "straps_measure_mesh_bwd: `workspace` is a null pointer");
    STRAPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "straps_measure_mesh_bwd: `workspace` must be 8-byte aligned");
    STRAPS_REQUIRE(batch >= 1 && batch < (1LL << 31), "straps_measure_mesh_bwd: `batch` must be in 1..2^31-1 (got %lld)", batch);
    STRAPS_REQUIRE(nverts >= 1 && nverts <= MB_MAX_VERTS, "straps_measure_mesh_bwd: `nverts` must be in 1..1048576 (got %d)", nverts);
    STRAPS_REQUIRE(n_points >= 0 && n_points <= MB_MAX_POINTS, "straps_measure_mesh_bwd: `n_points` must be in 0..64 (got %d)", n_points);
    STRAPS_REQUIRE(dpoints_rows >= n_points, "straps_measure_mesh_bwd: `dpoints_rows` = %d is below n_points = %d", dpoints_rows, n_points);
    STRAPS_REQUIRE(nfaces >= 0 && nfaces <= 0x7fffffff / 3, "straps_measure_mesh_bwd: `nfaces` must be in 0..715827882 (got %d)", nfaces);
    STRAPS_REQUIRE(n_meas >= 1 && n_meas <= MB_MAX_MEAS, "straps_measure_mesh_bwd: `n_meas` must be in 1..32 (got %d)", n_meas);
    STRAPS_REQUIRE(points || n_points == 0, "straps_measure_mesh_bwd: `points` is a null pointer with n_points = %d", n_points);
    STRAPS_REQUIRE(faces || nfaces == 0, "straps_measure_mesh_bwd: `faces` is a null pointer with nfaces = %d", nfaces);
    MeasPackB mp;
    memset(&mp, 0, sizeof(mp));
    bool any_face = false, any_face_anchor = false, any_extent = false, any_point = false;
    const int n_anchor = nverts + n_points;
    for (int m = 0; m < n_meas; ++m) {
        const straps_measure_t& q = meas[m];
        int used = 0;      // leading anchors this kind reads
        switch (q.kind) {
            case STRAPS_MEASURE_VOLUME:
                used = q.anchor[0] == -1 ? 0 : 1;
                break;
            case STRAPS_MEASURE_AREA:
            case STRAPS_MEASURE_EXTENT:
                break;
            case STRAPS_MEASURE_GIRTH:
                STRAPS_REQUIRE(q.anchor[0] != -1, "straps_measure_mesh_bwd: `meas[%d]` is a GIRTH without an anchor: `anchor[0]` is required", m);
                used = 1;
                break;
            case STRAPS_MEASURE_PATH:
                while (used < 4 && q.anchor[used] != -1) ++used;
                STRAPS_REQUIRE(used >= 2, "straps_measure_mesh_bwd: `meas[%d]` is a PATH with %d leading `anchor` entries: 2 to 4 are required", m, used);
                break;
            default:
                STRAPS_REQUIRE(false, "straps_measure_mesh_bwd: `meas[%d].kind` is unknown (got %d)", m, q.kind);
        }
        for (int j = 0; j < used; ++j) {
            STRAPS_REQUIRE(q.anchor[j] >= 0 && q.anchor[j] < n_anchor, "straps_measure_mesh_bwd: `meas[%d].anchor[%d]` = %d is outside 0..nverts + n_points - 1 = %d",
                           m, j, q.anchor[j], n_anchor - 1);
            any_point |= q.anchor[j] >= nverts;
        }
        const bool face_kind = q.kind == STRAPS_MEASURE_VOLUME || q.kind == STRAPS_MEASURE_AREA || q.kind == STRAPS_MEASURE_GIRTH;
        if (face_kind) {
            STRAPS_REQUIRE(nfaces > 0, "straps_measure_mesh_bwd: `meas[%d]` reads faces but `nfaces` is 0", m);
            STRAPS_REQUIRE(q.part_mask == 0u || face_parts, "straps_measure_mesh_bwd: `meas[%d].part_mask` is set but `face_parts` is a null pointer", m);
            STRAPS_REQUIRE(vf_offsets, "straps_measure_mesh_bwd: `meas[%d]` reads faces but `vf_offsets` is a null pointer", m);
            STRAPS_REQUIRE(vf_faces, "straps_measure_mesh_bwd: `meas[%d]` reads faces but `vf_faces` is a null pointer", m);
        }
        any_face |= face_kind;
        any_face_anchor |= face_kind && used == 1;
        any_extent |= q.kind == STRAPS_MEASURE_EXTENT;
        mp.m[m].kind = q.kind;
        for (int j = 0; j < 4; ++j) mp.m[m].anchor[j] = j < used ? q.anchor[j] : -1;
        for (int c = 0; c < 3; ++c) mp.m[m].dir[c] = q.dir[c];
        mp.m[m].part_mask = face_kind ? q.part_mask : 0u;
    }
    STRAPS_REQUIRE(dpoints || !any_point, "straps_measure_mesh_bwd: `dpoints` is a null pointer but a measurement is anchored at a point");
    const int nfb = (nfaces + MB_FACES_PER_BLOCK - 1) / MB_FACES_PER_BLOCK, nvb = (nverts + MB_VERTS_PER_BLOCK - 1) / MB_VERTS_PER_BLOCK;
    const int nvc = (nverts + MB_THREADS - 1) / MB_THREADS;
    const int fb_run = any_face_anchor ? nfb : 0, vb_run = any_extent ? nvb : 0;
    const int per_body = nvc + ((dpoints && n_points > 0) ? 1 : 0);
    const long long blocks = batch * (long long)(fb_run + vb_run), gather_blocks = batch * (long long)per_body;
    STRAPS_REQUIRE(blocks < (1LL << 31) && gather_blocks < (1LL << 31), "straps_measure_mesh_bwd: `batch` too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    if (blocks > 0) {
        hipLaunchKernelGGL(measure_bwd_partial_kernel, dim3((unsigned)blocks), dim3(MB_THREADS), 0, st, verts, points, faces, face_parts, mp, ws, nverts, n_points,
                           nfaces, n_meas, nfb, nvb, fb_run, vb_run);
        STRAPS_CHECK_LAUNCH("measure_bwd_partial_kernel");
    }
    hipLaunchKernelGGL(measure_bwd_gather_kernel, dim3((unsigned)gather_blocks), dim3(MB_THREADS), 0, st, verts, points, faces, face_parts, vf_offsets, vf_faces, mp,
                       dout, ws, dverts, dpoints, nverts, n_points, dpoints_rows, nfaces, n_meas, nfb, nvb, nvc, per_body, any_face ? 1 : 0);
    STRAPS_CHECK_LAUNCH("measure_bwd_gather_kernel");
    return STRAPS_OK;
}

extern "C" int straps_measure_residual(const float* values, const float* targets, const float* weights, const float* est, const float* est0, float lambda_shape,
                                       float* energy, float* dvalues, float* g, long long batch, int n_meas, void* stream) {
    STRAPS_REQUIRE(values, "straps_measure_residual: `values` is a null pointer");
    STRAPS_REQUIRE(targets, "straps_measure_residual: `targets` is a null pointer");
    STRAPS_REQUIRE(est, "straps_measure_residual: `est` is a null pointer");
    STRAPS_REQUIRE(est0, "straps_measure_residual: `est0` is a null pointer");
    STRAPS_REQUIRE(energy, "straps_measure_residual: `energy` is a null pointer");
    STRAPS_REQUIRE(dvalues, "straps_measure_residual: `dvalues` is a null pointer");
    STRAPS_REQUIRE(g, "straps_measure_residual: `g` is a null pointer");
    STRAPS_REQUIRE(batch >= 1 && batch < (1LL << 31), "straps_measure_residual: `batch` must be in 1..2^31-1 (got %lld)", batch);
    STRAPS_REQUIRE(n_meas >= 1 && n_meas <= MB_MAX_MEAS, "straps_measure_residual: `n_meas` must be in 1..32 (got %d)", n_meas);
    STRAPS_REQUIRE(lambda_shape >= 0.f, "straps_measure_residual: `lambda_shape` must not be negative or NaN (got %g)", (double)lambda_shape);
    const long long blocks = (batch + MB_THREADS - 1) / MB_THREADS;
    hipLaunchKernelGGL(measure_residual_kernel, dim3((unsigned)blocks), dim3(MB_THREADS), 0, (hipStream_t)stream, values, targets, weights, est, est0, lambda_shape,
                       energy, dvalues, g, batch, n_meas);
    STRAPS_CHECK_LAUNCH("measure_residual_kernel");
    return STRAPS_OK;
}
