// measure.hip -- body measurements of a batch of meshes on the device: volume, surface area, extent along a direction, planar girths and
// lengths along anchor points (include/straps_hip.h states the definitions).  The vertices are read as fp32; every product, sum, division
// and square root is done in double; each result is rounded to float once.  Gather- and latency-bound work, no MFMA.
//
// Two launches per call, both on the caller's stream, no synchronisation, no allocation, no floating-point atomics:
//   1. partial kernel : workgroup (body, k).  The first ceil(nfaces / 512) workgroups of a body are FACE blocks: thread t owns faces
//                       512 k + t and 512 k + 256 + t, loads their corners ONCE and walks the measurements (kinds and first anchors of all
//                       of them staged in LDS by n_meas threads at once); per face-based measurement it adds its two terms, the wave adds
//                       its 64 lanes in a fixed shuffle tree (32, 16, .. 1), the four wave sums are added in wave order, and the block's
//                       double lands in workspace[body][k][m].  The following ceil(nverts / 2048) workgroups are VERTEX
//                       blocks (launched only when an EXTENT is asked for): thread t owns vertices 2048 k + t + 256 i, i < 8, and per EXTENT
//                       reduces (max, min) of dir . p the same way.  Face blocks are not launched when no measurement reads faces.
//   2. finish kernel  : workgroup (measurement, 256 bodies), one thread per body: adds the body's partials in index order (eight loads in
//                       flight), scales, rounds to float once.  PATH is computed here from its anchors alone.
// A workgroup touches one body, every reduction has a fixed shape: a body's row is the same bits alone or in any batch, from run to run, and
// a NaN in one body stays there.  max / min PROPAGATE a NaN (an EXTENT of a body with a NaN coordinate on a non-zero axis is NaN).
// Only slots that the first kernel wrote are read by the second: face slots of face-based measurements, vertex slots of EXTENTs.
#include "common.h"

#include <string.h>

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_FACES_PER_BLOCK = 512;       // == hipabi.MEASURE_FACES_PER_BLOCK
constexpr int MS_VERTS_PER_BLOCK = 2048;      // == hipabi.MEASURE_VERTS_PER_BLOCK
constexpr int MS_FPT = MS_FACES_PER_BLOCK / MS_THREADS;
constexpr int MS_VPT = MS_VERTS_PER_BLOCK / MS_THREADS;
constexpr int MS_MAX_MEAS = 32;
constexpr int MS_MAX_POINTS = 64;
constexpr int MS_MAX_VERTS = 1 << 20;

struct MeasPack {
    straps_measure_t m[MS_MAX_MEAS];
};

__device__ __forceinline__ bool is_face_kind(int kind) { return kind == STRAPS_MEASURE_VOLUME || kind == STRAPS_MEASURE_AREA || kind == STRAPS_MEASURE_GIRTH; }

// anchor a of body b (0 <= a < nverts + n_points, checked on the host): a vertex, or one of the extra points
__device__ __forceinline__ const float* anchor_ptr(const float* __restrict__ vb, const float* __restrict__ pb, int a, int nverts) {
    return a < nverts ? vb + (long long)a * 3 : pb + (long long)(a - nverts) * 3;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
// NaN-propagating: a NaN on either side stays
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }

// the term of one selected face (corners P[corner][xyz]) for measurement q; `o` is its anchor (VOLUME: the centre, zero without one)
__device__ __forceinline__ double face_term(const straps_measure_t& q, const double (&P)[3][3], const double (&o)[3]) {
    if (q.kind == STRAPS_MEASURE_VOLUME) {
        double r[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) r[i][c] = P[i][c] - o[c];
        const double cx = r[1][1] * r[2][2] - r[1][2] * r[2][1];
        const double cy = r[1][2] * r[2][0] - r[1][0] * r[2][2];
        const double cz = r[1][0] * r[2][1] - r[1][1] * r[2][0];
        return (r[0][0] * cx + r[0][1] * cy) + r[0][2] * cz;
    }
    if (q.kind == STRAPS_MEASURE_AREA) {
        const double ax = P[1][0] - P[0][0], ay = P[1][1] - P[0][1], az = P[1][2] - P[0][2];
        const double bx = P[2][0] - P[0][0], by = P[2][1] - P[0][1], bz = P[2][2] - P[0][2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        return sqrt((cx * cx + cy * cy) + cz * cz);
    }
    // GIRTH: signed distances (times |dir|) to the plane; the vertex alone on its side is `a` of both crossing edges
    const double nx = (double)q.dir[0], ny = (double)q.dir[1], nz = (double)q.dir[2];
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = (nx * (P[i][0] - o[0]) + ny * (P[i][1] - o[1])) + nz * (P[i][2] - o[2]);
    const bool s0 = d[0] >= 0.0, s1 = d[1] >= 0.0, s2 = d[2] >= 0.0;
    if (s0 == s1 && s1 == s2) return 0.0;
    const int a = (s1 == s2) ? 0 : ((s0 == s2) ? 1 : 2);
    double A[3], B[3], C[3], da, db, dc;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A[c] = a == 0 ? P[0][c] : (a == 1 ? P[1][c] : P[2][c]);
        B[c] = a == 0 ? P[1][c] : (a == 1 ? P[2][c] : P[0][c]);
        C[c] = a == 0 ? P[2][c] : (a == 1 ? P[0][c] : P[1][c]);
    }
    da = a == 0 ? d[0] : (a == 1 ? d[1] : d[2]);
    db = a == 0 ? d[1] : (a == 1 ? d[2] : d[0]);
    dc = a == 0 ? d[2] : (a == 1 ? d[0] : d[1]);
    const double tb = da / (da - db), tc = da / (da - dc);
    double len2 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double xb = A[c] + tb * (B[c] - A[c]);
        const double xc = A[c] + tc * (C[c] - A[c]);
        const double e = xb - xc;
        len2 += e * e;
    }
    return sqrt(len2);
}

__global__ __launch_bounds__(MS_THREADS) STRAPS_NO_PACKED_FP32 void measure_partial_kernel(const float* __restrict__ verts, const float* __restrict__ points,
                                                                                          const int32_t* __restrict__ faces,
                                                                                          const uint8_t* __restrict__ face_parts, const MeasPack mp,
                                                                                          double* __restrict__ ws, int nverts, int n_points, int nfaces,
                                                                                          int n_meas, int nfb, int nvb, int fb_run, int vb_run) {
    __shared__ double red[MS_MAX_MEAS][2][MS_THREADS / 64];
    __shared__ int kinds[MS_MAX_MEAS];
    __shared__ float anc[MS_MAX_MEAS][3];
    const int per_body = fb_run + vb_run;                       // workgroups launched per body
    const long long b = blockIdx.x / per_body;
    const int k = (int)(blockIdx.x - b * per_body);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* vb = verts + b * nverts * 3;
    const float* pb = points ? points + b * n_points * 3 : nullptr;
    double* wb = ws + b * (long long)n_meas * (nfb + 2 * nvb);      // [nfb][n_meas] face partials, then [nvb][n_meas][2] (max, min)
    // kinds and first anchors of all measurements, fetched by n_meas threads at once: the loops below would otherwise wait for one
    // dependent global load per measurement
    if (tid < n_meas) {
        const int kind = mp.m[tid].kind, a = mp.m[tid].anchor[0];
        kinds[tid] = kind;
        float x = 0.f, y = 0.f, z = 0.f;
        if (is_face_kind(kind) && a >= 0) {
            const float* ap = anchor_ptr(vb, pb, a, nverts);
            x = ap[0]; y = ap[1]; z = ap[2];
        }
        anc[tid][0] = x; anc[tid][1] = y; anc[tid][2] = z;
    }
    __syncthreads();

    if (k < fb_run) {
        // ---- a face block: corners once, then every face-based measurement
        double P[MS_FPT][3][3];
        bool ok[MS_FPT];
        unsigned part_bit[MS_FPT];
#pragma unroll
        for (int j = 0; j < MS_FPT; ++j) {
            const int f = k * MS_FACES_PER_BLOCK + j * MS_THREADS + tid;      // < nfaces + 512 <= 2^31 / 3 + 512
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
            if (!is_face_kind(q.kind)) continue;                 // (uniform over the workgroup)
            const double o[3] = {(double)anc[m][0], (double)anc[m][1], (double)anc[m][2]};      // (zero without an anchor)
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < MS_FPT; ++j) {
                const bool sel = ok[j] && (q.part_mask == 0u || (part_bit[j] & q.part_mask) != 0u);
                if (sel) acc += face_term(q, P[j], o);
            }
            acc = wave_sum(acc);
            if (lane == 0) red[m][0][wave] = acc;
        }
        __syncthreads();
        if (tid < n_meas && is_face_kind(kinds[tid])) {
            double s = red[tid][0][0];
#pragma unroll
            for (int w = 1; w < MS_THREADS / 64; ++w) s += red[tid][0][w];
            wb[(long long)k * n_meas + tid] = s;
        }
        return;
    }

    // ---- a vertex block: (max, min) of dir . p per EXTENT
    const int kv = k - fb_run;
    double V[MS_VPT][3];
    bool have[MS_VPT];
#pragma unroll
    for (int j = 0; j < MS_VPT; ++j) {
        const int v = kv * MS_VERTS_PER_BLOCK + j * MS_THREADS + tid;      // < 2^20 + 2048
        have[j] = v < nverts;
#pragma unroll
        for (int c = 0; c < 3; ++c) V[j][c] = have[j] ? (double)vb[(long long)v * 3 + c] : 0.0;
    }
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    for (int m = 0; m < n_meas; ++m) {
        const straps_measure_t& q = mp.m[m];
        if (q.kind != STRAPS_MEASURE_EXTENT) continue;
        const double nx = (double)q.dir[0], ny = (double)q.dir[1], nz = (double)q.dir[2];
        double mx = -inf, mn = inf;
#pragma unroll
        for (int j = 0; j < MS_VPT; ++j) {
            if (have[j]) {
                const double h = (nx * V[j][0] + ny * V[j][1]) + nz * V[j][2];
                mx = nan_max(mx, h);
                mn = nan_min(mn, h);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            mx = nan_max(mx, __shfl_down(mx, off, 64));
            mn = nan_min(mn, __shfl_down(mn, off, 64));
        }
        if (lane == 0) {
            red[m][0][wave] = mx;
            red[m][1][wave] = mn;
        }
    }
    __syncthreads();
    if (tid < n_meas && kinds[tid] == STRAPS_MEASURE_EXTENT) {
        double mx = red[tid][0][0], mn = red[tid][1][0];
#pragma unroll
        for (int w = 1; w < MS_THREADS / 64; ++w) {
            mx = nan_max(mx, red[tid][0][w]);
            mn = nan_min(mn, red[tid][1][w]);
        }
        double* e = wb + (long long)nfb * n_meas + ((long long)kv * n_meas + tid) * 2;
        e[0] = mx;
        e[1] = mn;
    }
}

// partials of one (body, measurement), `stride` doubles apart, added in index order; eight loads in flight per trip (one after the other they
// cost a round trip to memory each)
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

__global__ __launch_bounds__(MS_THREADS) STRAPS_NO_PACKED_FP32 void measure_finish_kernel(const float* __restrict__ verts, const float* __restrict__ points,
                                                                                         const MeasPack mp, const double* __restrict__ ws,
                                                                                         float* __restrict__ out, long long batch, int nverts, int n_points,
                                                                                         int n_meas, int nfb, int nvb) {
    const int m = blockIdx.x % n_meas;                            // uniform: the measurement comes from scalar registers
    const long long b = (long long)(blockIdx.x / n_meas) * MS_THREADS + threadIdx.x;
    if (b >= batch) return;
    const straps_measure_t& q = mp.m[m];
    const double* wb = ws + b * (long long)n_meas * (nfb + 2 * nvb);
    double r = 0.0;
    if (is_face_kind(q.kind)) {
        r = sum_in_order(wb + m, nfb, n_meas);
        if (q.kind == STRAPS_MEASURE_VOLUME) r = r / 6.0;
        if (q.kind == STRAPS_MEASURE_AREA) r = r * 0.5;
    } else if (q.kind == STRAPS_MEASURE_EXTENT) {
        const double* e = wb + (long long)nfb * n_meas;
        double mx = e[(long long)m * 2], mn = e[(long long)m * 2 + 1];
        for (int k = 1; k < nvb; ++k) {
            mx = nan_max(mx, e[((long long)k * n_meas + m) * 2]);
            mn = nan_min(mn, e[((long long)k * n_meas + m) * 2 + 1]);
        }
        r = mx - mn;
    } else {      // PATH
        const float* vb = verts + b * nverts * 3;
        const float* pb = points ? points + b * n_points * 3 : nullptr;
        const float* prev = anchor_ptr(vb, pb, q.anchor[0], nverts);
        for (int j = 1; j < 4 && q.anchor[j] >= 0; ++j) {
            const float* cur = anchor_ptr(vb, pb, q.anchor[j], nverts);
            const double dx = (double)cur[0] - (double)prev[0], dy = (double)cur[1] - (double)prev[1], dz = (double)cur[2] - (double)prev[2];
            r += sqrt((dx * dx + dy * dy) + dz * dz);
            prev = cur;
        }
    }
    out[b * n_meas + m] = (float)r;
}

}  // namespace

extern "C" size_t straps_measure_workspace_bytes(long long batch, int nverts, int nfaces, int n_meas) {
    if (batch <= 0 || batch >= (1LL << 31) || nverts < 1 || nverts > MS_MAX_VERTS || nfaces < 0 || nfaces > 0x7fffffff / 3 || n_meas < 1 || n_meas > MS_MAX_MEAS) return 0;
    const size_t nfb = ((size_t)nfaces + MS_FACES_PER_BLOCK - 1) / MS_FACES_PER_BLOCK, nvb = ((size_t)nverts + MS_VERTS_PER_BLOCK - 1) / MS_VERTS_PER_BLOCK;
    return (size_t)batch * (size_t)n_meas * (nfb + 2 * nvb) * sizeof(double);
}

extern "C" int straps_measure_mesh(const float* verts, const float* points, const int32_t* faces, const uint8_t* face_parts, const straps_measure_t* meas,
                                   float* out, void* workspace, long long batch, int nverts, int n_points, int nfaces, int n_meas, void* stream) {
    STRAPS_REQUIRE(verts, "straps_measure_mesh: `verts` is a null pointer");
    STRAPS_REQUIRE(meas, "straps_measure_mesh: `meas` is a null pointer");
    STRAPS_REQUIRE(out, "straps_measure_mesh: `out` is a null pointer");
    STRAPS_REQUIRE(workspace, "straps_measure_mesh: `workspace` is a null pointer");
    STRAPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "straps_measure_mesh: `workspace` must be 8-byte aligned");
    STRAPS_REQUIRE(batch >= 1 && batch < (1LL << 31), "straps_measure_mesh: `batch` must be in 1..2^31-1 (got %lld)", batch);
    STRAPS_REQUIRE(nverts >= 1 && nverts <= MS_MAX_VERTS, "straps_measure_mesh: `nverts` must be in 1..1048576 (got %d)", nverts);
    STRAPS_REQUIRE(n_points >= 0 && n_points <= MS_MAX_POINTS, "straps_measure_mesh: `n_points` must be in 0..64 (got %d)", n_points);
    STRAPS_REQUIRE(nfaces >= 0 && nfaces <= 0x7fffffff / 3, "straps_measure_mesh: `nfaces` must be in 0..715827882 (got %d)", nfaces);
    STRAPS_REQUIRE(n_meas >= 1 && n_meas <= MS_MAX_MEAS, "straps_measure_mesh: `n_meas` must be in 1..32 (got %d)", n_meas);
    STRAPS_REQUIRE(points || n_points == 0, "straps_measure_mesh: `points` is a null pointer with n_points = %d", n_points);
    STRAPS_REQUIRE(faces || nfaces == 0, "straps_measure_mesh: `faces` is a null pointer with nfaces = %d", nfaces);
    MeasPack mp;
    memset(&mp, 0, sizeof(mp));
    bool any_face = false, any_extent = false;
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
                STRAPS_REQUIRE(q.anchor[0] != -1, "straps_measure_mesh: `meas[%d]` is a GIRTH without an anchor: `anchor[0]` is required", m);
                used = 1;
                break;
            case STRAPS_MEASURE_PATH:
                while (used < 4 && q.anchor[used] != -1) ++used;
                STRAPS_REQUIRE(used >= 2, "straps_measure_mesh: `meas[%d]` is a PATH with %d leading `anchor` entries: 2 to 4 are required", m, used);
                break;
            default:
                STRAPS_REQUIRE(false, "straps_measure_mesh: `meas[%d].kind` is unknown (got %d)", m, q.kind);
        }
        for (int j = 0; j < used; ++j)
            STRAPS_REQUIRE(q.anchor[j] >= 0 && q.anchor[j] < n_anchor, "straps_measure_mesh: `meas[%d].anchor[%d]` = %d is outside 0..nverts + n_points - 1 = %d", m,
                           j, q.anchor[j], n_anchor - 1);
        const bool face_kind = q.kind == STRAPS_MEASURE_VOLUME || q.kind == STRAPS_MEASURE_AREA || q.kind == STRAPS_MEASURE_GIRTH;
        if (face_kind) {
            STRAPS_REQUIRE(nfaces > 0, "straps_measure_mesh: `meas[%d]` reads faces but `nfaces` is 0", m);
            STRAPS_REQUIRE(q.part_mask == 0u || face_parts, "straps_measure_mesh: `meas[%d].part_mask` is set but `face_parts` is a null pointer", m);
        }
        any_face |= face_kind;
        any_extent |= q.kind == STRAPS_MEASURE_EXTENT;
        // what the kernels see: the kind, the anchors it reads (-1 behind them), dir, and a part mask only where faces are read
        mp.m[m].kind = q.kind;
        for (int j = 0; j < 4; ++j) mp.m[m].anchor[j] = j < used ? q.anchor[j] : -1;
        for (int c = 0; c < 3; ++c) mp.m[m].dir[c] = q.dir[c];
        mp.m[m].part_mask = face_kind ? q.part_mask : 0u;
    }
    const int nfb = (nfaces + MS_FACES_PER_BLOCK - 1) / MS_FACES_PER_BLOCK, nvb = (nverts + MS_VERTS_PER_BLOCK - 1) / MS_VERTS_PER_BLOCK;
    const int fb_run = any_face ? nfb : 0, vb_run = any_extent ? nvb : 0;
    const long long blocks = batch * (long long)(fb_run + vb_run), fin_blocks = (batch + MS_THREADS - 1) / MS_THREADS * n_meas;
    STRAPS_REQUIRE(blocks < (1LL << 31) && fin_blocks < (1LL << 31), "straps_measure_mesh: `batch` too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    if (blocks > 0) {
        hipLaunchKernelGGL(measure_partial_kernel, dim3((unsigned)blocks), dim3(MS_THREADS), 0, st, verts, points, faces, face_parts, mp, ws, nverts, n_points,
                           nfaces, n_meas, nfb, nvb, fb_run, vb_run);
        STRAPS_CHECK_LAUNCH("measure_partial_kernel");
    }
    hipLaunchKernelGGL(measure_finish_kernel, dim3((unsigned)fin_blocks), dim3(MS_THREADS), 0, st, verts, points, mp, ws, out, batch, nverts, n_points, n_meas, nfb,
                       nvb);
    STRAPS_CHECK_LAUNCH("measure_finish_kernel");
    return STRAPS_OK;
}
