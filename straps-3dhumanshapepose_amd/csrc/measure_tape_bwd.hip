// measure_tape_bwd.hip -- the gradient of straps_measure_tape (csrc/measure_tape.hip) w.r.t. the vertices and the anchor points: tape girths
// (the perimeter of the convex hull of a plane section) and section lengths, with the plane's normal given once or taken per body from two
// anchors (include/straps_hip.h states the definition).  The vertices are read as fp32; every product, sum, division and square root is done
// in double; each output element is rounded to float once, after all its terms are added.  A GATHER: no floating-point atomics, no
// allocation, no synchronisation, nothing read that the call has not written.
//
// Three launches per call (two without a HULL), all on the caller's stream:
//   1. collect kernel : the forward's collect kernel, statement for statement, so that the section points, their slots and the section length
//                       are the same bits; a HULL also stores the face index of every cut slot (ascending: slot order is face order).  A SECTION
//                       adds, per thread in trip order and then in the forward's fixed tree, the gradient of its length w.r.t. the plane's
//                       anchor and normal (six doubles in the row's header).
//   2. hull kernel    : workgroup (body, measurement), only for a HULL.  The forward's march with a candidate that carries its point index:
//                       among equal coordinates the lower index wins, every other choice is the forward's, so the perimeter is the same bits.
//                       Every step gives the unit vector of a hull edge; a corner's upstream vector (g_u, g_v) is the edge that arrives minus
//                       the edge that leaves, stored at the corner's point (all other points hold zero).  Then the workgroup walks the slots,
//                       a slot per thread, recomputes the face of every slot with a non-zero vector and adds the gradient w.r.t. the anchor
//                       and the normal in slot order and a fixed tree (six doubles in the header).
//   3. gather kernel  : workgroup (body, 256 vertices), one thread per vertex, as measure_bwd_gather_kernel: the vertex's incident faces in
//                       table order, per face the measurements in index order (a HULL finds the face's slot by binary search in the row's
//                       face-index list), point 0 then point 1; then what the vertex receives as an anchor, in measurement order; three
//                       floats stored, or added to what is there.  One more workgroup per body finishes the points: thread j owns row j.
// A workgroup touches one body, every reduction has a fixed shape and the order of an element's terms depends on the topology, the
// measurement list and that body's own chain alone.
#include "common.h"

#include <string.h>

namespace {

constexpr int TB_THREADS = 256;
constexpr int TB_FACES_PER_BLOCK = 256;       // == the forward's MT_FACES_PER_BLOCK (hipabi.MEASURE_TAPE_FACES_PER_BLOCK)
constexpr int TB_WAVES = TB_THREADS / 64;
constexpr int TB_MAX_MEAS = 32;
constexpr int TB_MAX_POINTS = 64;
constexpr int TB_MAX_VERTS = 1 << 20;
constexpr int TB_MAX_FACES = 0x7fffffff / 3;
constexpr int TB_HEADER = 10;                 // doubles in front of a row: count, section length, status, d/d anchor (3), d/d normal (3), spare
constexpr int TB_STATUS = 2, TB_DO = 3, TB_DN = 6;
constexpr int TB_INFLIGHT = 4;                // incident faces whose indices and corners a gather thread loads before it computes

struct TapePackB {
    straps_tape_t m[TB_MAX_MEAS];
};

// a row of the workspace, in doubles: header | cap (u, v) pairs | cap (g_u, g_v) pairs | ceil(cap / 2) face indices (int32, padded to a double)
__host__ __device__ __forceinline__ long long tb_row_doubles(long long cap) { return TB_HEADER + 4 * cap + ((cap + 1) / 2 + 1) / 2; }

__device__ __forceinline__ const float* tape_anchor_ptr(const float* __restrict__ vb, const float* __restrict__ pb, int a, int nverts) {
    return a < nverts ? vb + (long long)a * 3 : pb + (long long)(a - nverts) * 3;
}

__device__ __forceinline__ double tape_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000LL); }      // (false for a NaN)

// the plane of (body, measurement) as the forward builds it: anchor o, normal n, basis (u, v); false when the normal cuts nothing
__device__ __forceinline__ bool tape_plane(const straps_tape_t& q, const float* __restrict__ vb, const float* __restrict__ pb, int nverts, double (&o)[3],
                                           double (&n)[3], double (&u)[3], double (&v)[3]) {
    const float* a0 = tape_anchor_ptr(vb, pb, q.anchor[0], nverts);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (double)a0[c];
    if (q.anchor[1] >= 0) {
        const float* a1 = tape_anchor_ptr(vb, pb, q.anchor[1], nverts);
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] = (double)a1[c] - o[c];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] = (double)q.dir[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = v[c] = 0.0;
    if (!(finite_d(n[0]) && finite_d(n[1]) && finite_d(n[2])) || (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0)) return false;
    const double m0 = fabs(n[0]), m1 = fabs(n[1]), m2 = fabs(n[2]);
    const int k = (m0 <= m1 && m0 <= m2) ? 0 : (m1 <= m2 ? 1 : 2);
    double a[3];
    a[0] = k == 0 ? 0.0 : (k == 1 ? n[2] : -n[1]);
    a[1] = k == 0 ? -n[2] : (k == 1 ? 0.0 : n[0]);
    a[2] = k == 0 ? n[1] : (k == 1 ? -n[0] : 0.0);
    const double la = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = a[c] / la;
    double w[3];
    w[0] = n[1] * u[2] - n[2] * u[1];
    w[1] = n[2] * u[0] - n[0] * u[2];
    w[2] = n[0] * u[1] - n[1] * u[0];
    const double lw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = w[c] / lw;
    return true;
}

// The section of one face by the plane (o, n), on the forward's branch: the side tests, the lone corner a, t = d_a / (d_a - d_b).  false: not
// cut.  EB = p_b - p_a and EC = p_c - p_a are the two cut edges, X their section points, Db = d_b - d_a = n . EB and Dc likewise (the two
// distances have opposite sides, so the difference does not cancel).
struct FaceCut {
    int a;
    double tb, tc, Db, Dc, EB[3], EC[3], X[2][3];
};

__device__ __forceinline__ bool face_cut(const double (&P)[3][3], const double (&o)[3], const double (&n)[3], FaceCut& k) {
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = (n[0] * (P[i][0] - o[0]) + n[1] * (P[i][1] - o[1])) + n[2] * (P[i][2] - o[2]);
    const bool s0 = d[0] >= 0.0, s1 = d[1] >= 0.0, s2 = d[2] >= 0.0;
    if (s0 == s1 && s1 == s2) return false;
    const int a = (s1 == s2) ? 0 : ((s0 == s2) ? 1 : 2);
    const double da = a == 0 ? d[0] : (a == 1 ? d[1] : d[2]);
    const double db = a == 0 ? d[1] : (a == 1 ? d[2] : d[0]);
    const double dc = a == 0 ? d[2] : (a == 1 ? d[0] : d[1]);
    k.a = a;
    k.tb = da / (da - db);
    k.tc = da / (da - dc);
    k.Db = db - da;
    k.Dc = dc - da;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double A = a == 0 ? P[0][c] : (a == 1 ? P[1][c] : P[2][c]);
        const double B = a == 0 ? P[1][c] : (a == 1 ? P[2][c] : P[0][c]);
        const double C = a == 0 ? P[2][c] : (a == 1 ? P[0][c] : P[1][c]);
        k.EB[c] = B - A;
        k.EC[c] = C - A;
        k.X[0][c] = A + k.tb * k.EB[c];
        k.X[1][c] = A + k.tc * k.EC[c];
    }
    return true;
}

// With the upstream vectors g0, g1 of the two section points: s = (g . e) / D per point, and what the plane receives:
// d/do += s n, d/dn += -s (x - o).  h0 = g0 - s0 n and h1 = g1 - s1 n are what the corners share out: a gets (1 - t) h, b (or c) gets t h.
__device__ __forceinline__ void cut_terms(const FaceCut& k, const double (&g0)[3], const double (&g1)[3], const double (&o)[3], const double (&n)[3], double (&h0)[3],
                                          double (&h1)[3], double (&go)[3], double (&gn)[3]) {
    const double s0 = ((g0[0] * k.EB[0] + g0[1] * k.EB[1]) + g0[2] * k.EB[2]) / k.Db;
    const double s1 = ((g1[0] * k.EC[0] + g1[1] * k.EC[1]) + g1[2] * k.EC[2]) / k.Dc;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        h0[c] = g0[c] - s0 * n[c];
        h1[c] = g1[c] - s1 * n[c];
        go[c] = s0 * n[c] + s1 * n[c];
        gn[c] = -(s0 * (k.X[0][c] - o[c])) - s1 * (k.X[1][c] - o[c]);
    }
}

// six per-thread sums -> the workgroup's, in the forward's shape: the wave's 64 lanes in a shuffle tree, the four waves in wave order.
// Thread 0 returns the sums.  (The barrier in front keeps a second call from overwriting what a slow wave still reads.)
__device__ __forceinline__ void block_sum6(double (&a)[6], double (*red)[TB_WAVES]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const double s = tape_wave_sum(a[c]);
        if (lane == 0) red[c][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double s = red[c][0];
#pragma unroll
        for (int w = 1; w < TB_WAVES; ++w) s += red[c][w];
        a[c] = s;
    }
}

__global__ __launch_bounds__(TB_THREADS) STRAPS_NO_PACKED_FP32 void tape_bwd_collect_kernel(const float* __restrict__ verts, const float* __restrict__ points,
                                                                                           const int32_t* __restrict__ faces,
                                                                                           const uint8_t* __restrict__ face_parts, const TapePackB mp,
                                                                                           const float* __restrict__ dout, float* __restrict__ values,
                                                                                           int32_t* __restrict__ counts, double* __restrict__ ws, int nverts,
                                                                                           int n_points, int nfaces, int n_meas, int cap) {
    __shared__ int wave_cut[2][TB_WAVES];
    __shared__ double wave_len[TB_WAVES];
    __shared__ double red6[6][TB_WAVES];
    const long long row = blockIdx.x;                              // body * n_meas + measurement
    const long long b = row / n_meas;
    const int m = (int)(row - b * n_meas);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const straps_tape_t& q = mp.m[m];
    const bool active = dout[row] != 0.f;                          // (a NaN is active)
    if (!active && !values && !counts) return;                     // (uniform) nothing of this row is asked for
    const float* vb = verts + b * nverts * 3;
    const float* pb = points ? points + b * n_points * 3 : nullptr;
    double* wr = ws + row * tb_row_doubles(cap);
    double* pts = wr + TB_HEADER;
    int32_t* slot_face = (int32_t*)(wr + TB_HEADER + 4LL * cap);
    double o[3], n[3], u[3], v[3];
    const bool plane_ok = tape_plane(q, vb, pb, nverts, o, n, u, v);      // (uniform over the workgroup)
    const bool store = q.kind == STRAPS_TAPE_HULL;
    const bool plane_grad = !store && active;                     // a SECTION adds its gradient w.r.t. the plane here
    int base = 0;                                                  // cut faces of the trips before this one
    double acc = 0.0;
    double pg[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (plane_ok) {
        int parity = 0;
        for (int f0 = 0; f0 < nfaces; f0 += TB_FACES_PER_BLOCK, parity ^= 1) {      // (f0 <= nfaces - 1 < 2^31 / 3: f0 + 256 does not overflow)
            const int f = f0 + tid;
            bool cut = false;
            double X[2][3];
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int c = 0; c < 3; ++c) X[e][c] = 0.0;
            if (f < nfaces) {
                const int i0 = faces[(long long)f * 3 + 0], i1 = faces[(long long)f * 3 + 1], i2 = faces[(long long)f * 3 + 2];
                bool sel = (unsigned)i0 < (unsigned)nverts && (unsigned)i1 < (unsigned)nverts && (unsigned)i2 < (unsigned)nverts;
                if (sel && q.part_mask != 0u) {
                    const unsigned lab = face_parts[f];
                    sel = lab < 32u && ((q.part_mask >> lab) & 1u) != 0u;
                }
                if (sel) {
                    const int idx[3] = {i0, i1, i2};
                    double P[3][3], d[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) P[i][c] = (double)vb[(long long)idx[i] * 3 + c];
                        d[i] = (n[0] * (P[i][0] - o[0]) + n[1] * (P[i][1] - o[1])) + n[2] * (P[i][2] - o[2]);
                    }
                    const bool s0 = d[0] >= 0.0, s1 = d[1] >= 0.0, s2 = d[2] >= 0.0;
                    cut = !(s0 == s1 && s1 == s2);
                    if (cut) {
                        const int a = (s1 == s2) ? 0 : ((s0 == s2) ? 1 : 2);
                        double A[3], Bc[3], Cc[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            A[c] = a == 0 ? P[0][c] : (a == 1 ? P[1][c] : P[2][c]);
                            Bc[c] = a == 0 ? P[1][c] : (a == 1 ? P[2][c] : P[0][c]);
                            Cc[c] = a == 0 ? P[2][c] : (a == 1 ? P[0][c] : P[1][c]);
                        }
                        const double da = a == 0 ? d[0] : (a == 1 ? d[1] : d[2]);
                        const double db = a == 0 ? d[1] : (a == 1 ? d[2] : d[0]);
                        const double dc = a == 0 ? d[2] : (a == 1 ? d[0] : d[1]);
                        const double tb = da / (da - db), tc = da / (da - dc);
                        double len2 = 0.0;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            X[0][c] = A[c] + tb * (Bc[c] - A[c]);
                            X[1][c] = A[c] + tc * (Cc[c] - A[c]);
                            const double e = X[0][c] - X[1][c];
                            len2 += e * e;
                        }
                        acc += sqrt(len2);
                        if (plane_grad && len2 != 0.0) {           // g = +-(x - x') / |x - x'|; a face of length exactly 0 adds nothing
                            FaceCut k;
                            k.a = a;
                            k.tb = tb;
                            k.tc = tc;
                            k.Db = db - da;
                            k.Dc = dc - da;
                            const double invl = 1.0 / sqrt(len2);
                            double g0[3], g1[3], h0[3], h1[3], go[3], gn[3];
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                k.EB[c] = Bc[c] - A[c];
                                k.EC[c] = Cc[c] - A[c];
                                k.X[0][c] = X[0][c];
                                k.X[1][c] = X[1][c];
                                g0[c] = (X[0][c] - X[1][c]) * invl;
                                g1[c] = -g0[c];
                            }
                            cut_terms(k, g0, g1, o, n, h0, h1, go, gn);
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                pg[c] += go[c];
                                pg[3 + c] += gn[c];
                            }
                        }
                    }
                }
            }
            const unsigned long long mask = __ballot(cut);          // wave64: one bit per lane
            if (lane == 0) wave_cut[parity][wave] = __popcll(mask);
            __syncthreads();      // (one barrier per trip: the next trip writes the other half of wave_cut, the one after it comes behind the next barrier)
            int before = base, total = 0;
#pragma unroll
            for (int w = 0; w < TB_WAVES; ++w) {
                const int cw = wave_cut[parity][w];
                before += w < wave ? cw : 0;
                total += cw;
            }
            if (cut && store) {
                const long long slot = before + __popcll(mask & ((1ull << lane) - 1ull));      // < nfaces
                if (2 * slot < cap) slot_face[slot] = f;            // (slot < ceil(cap / 2): inside the row's face-index list)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const long long pi = 2 * slot + e;
                    if (pi < cap) {
                        const double dx = X[e][0] - o[0], dy = X[e][1] - o[1], dz = X[e][2] - o[2];
                        pts[2 * pi + 0] = (u[0] * dx + u[1] * dy) + u[2] * dz;
                        pts[2 * pi + 1] = (v[0] * dx + v[1] * dy) + v[2] * dz;
                    }
                }
            }
            base += total;
        }
    }
    acc = tape_wave_sum(acc);
    if (lane == 0) wave_len[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = wave_len[0];
#pragma unroll
        for (int w = 1; w < TB_WAVES; ++w) s += wave_len[w];
        wr[0] = (double)(2 * (long long)base);
        wr[1] = s;
        if (counts) counts[row] = 2 * base;                        // (2 * nfaces < 2^31)
        if (!store && values) values[row] = (float)s;
    }
    if (plane_grad) {                                              // (uniform)
        block_sum6(pg, red6);
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < 6; ++c) wr[TB_DO + c] = pg[c];
        }
    }
}

// ---- the hull kernel's reductions: a candidate is a point (x, y) with its index, idx < 0: nothing (passed by value, as in the forward)
struct CandI {
    double x, y;
    int idx;
};

__device__ __forceinline__ bool lex_less(double ax, double ay, double bx, double by) { return ax < bx || (ax == bx && ay < by); }

// of two candidates the lexicographically smaller; of equal ones the lower index
__device__ __forceinline__ CandI pick_min(CandI a, CandI b) {
    if (b.idx < 0) return a;
    if (a.idx < 0) return b;
    if (lex_less(b.x, b.y, a.x, a.y)) return b;
    if (lex_less(a.x, a.y, b.x, b.y)) return a;
    return b.idx < a.idx ? b : a;
}
// the forward's pick_cw -- the more clockwise seen from (cx, cy), of collinear ones the farther, products rounded one by one -- and of equal
// points the lower index
__device__ __forceinline__ CandI pick_cw(CandI a, CandI b, double cx, double cy) {
    if (b.idx < 0) return a;
    if (a.idx < 0) return b;
    const double cross = __dsub_rn(__dmul_rn(a.x - cx, b.y - cy), __dmul_rn(a.y - cy, b.x - cx));
    if (cross < 0.0) return b;
    if (cross > 0.0) return a;
    if (lex_less(a.x, a.y, b.x, b.y)) return b;
    if (lex_less(b.x, b.y, a.x, a.y)) return a;
    return b.idx < a.idx ? b : a;
}

template <bool MARCH>
__device__ __forceinline__ CandI pick(CandI a, CandI b, double cx, double cy) {
    return MARCH ? pick_cw(a, b, cx, cy) : pick_min(a, b);
}

// the forward's hull_reduce with indices: thread t folds i = t, t + 256, .. in that order, the wave folds its lanes in a shuffle tree, every
// thread folds the four wave results in wave order
template <bool MARCH>
__device__ __forceinline__ CandI hull_reduce(const double* __restrict__ pts, int n, double sg, double cx, double cy, CandI* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    CandI best = {0.0, 0.0, -1};
    for (int i = tid; i < n; i += TB_THREADS) {
        CandI c = {sg * pts[2 * (long long)i], sg * pts[2 * (long long)i + 1], i};
        if (MARCH && !lex_less(cx, cy, c.x, c.y)) c.idx = -1;
        best = pick<MARCH>(best, c, cx, cy);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        CandI c;
        c.x = __shfl_down(best.x, off, 64);
        c.y = __shfl_down(best.y, off, 64);
        c.idx = __shfl_down(best.idx, off, 64);
        best = pick<MARCH>(best, c, cx, cy);
    }
    if (lane == 0) red[wave] = best;
    __syncthreads();
    CandI r = red[0];
#pragma unroll
    for (int w = 1; w < TB_WAVES; ++w) r = pick<MARCH>(r, red[w], cx, cy);
    return r;
}

__global__ __launch_bounds__(TB_THREADS) STRAPS_NO_PACKED_FP32 void tape_bwd_hull_kernel(const float* __restrict__ verts, const float* __restrict__ points,
                                                                                        const int32_t* __restrict__ faces, const TapePackB mp,
                                                                                        const float* __restrict__ dout, float* __restrict__ values,
                                                                                        double* __restrict__ ws, int nverts, int n_points, int n_meas, int cap) {
    __shared__ CandI red[2][TB_WAVES];
    __shared__ double red6[6][TB_WAVES];
    const long long row = blockIdx.x;
    const long long b = row / n_meas;
    const int m = (int)(row - b * n_meas);
    const straps_tape_t& q = mp.m[m];
    if (q.kind != STRAPS_TAPE_HULL) return;                        // (uniform)
    const bool active = dout[row] != 0.f;
    if (!active && !values) return;                                // (uniform) neither the value nor a gradient of this row is asked for
    const int tid = threadIdx.x;
    double* wr = ws + row * tb_row_doubles(cap);
    const double* pts = wr + TB_HEADER;
    double* g = wr + TB_HEADER + 2LL * cap;
    const int32_t* slot_face = (const int32_t*)(wr + TB_HEADER + 4LL * cap);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double countd = wr[0];                                   // (an integer below 2^31, exact)
    if (!(countd <= (double)cap)) {                               // more points than the row holds: NaN, as the forward
        if (tid == 0) {
            wr[TB_STATUS] = 1.0;
            if (values) values[row] = (float)nan;
        }
        return;
    }
    const int n = (int)countd;
    int bad = 0;
    for (int i = tid; i < n; i += TB_THREADS) bad |= !(finite_d(pts[2 * (long long)i]) && finite_d(pts[2 * (long long)i + 1]));
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            wr[TB_STATUS] = 1.0;
            if (values) values[row] = (float)nan;
        }
        return;
    }
    for (long long i = tid; i < 2LL * n; i += TB_THREADS) g[i] = 0.0;      // every point that is no corner: zero (the first reduction's barrier orders these stores before thread 0's)
    double perimeter = 0.0;
    if (n > 0) {
        int parity = 0;
        const CandI lo = hull_reduce<false>(pts, n, 1.0, 0.0, 0.0, red[parity]);
        parity ^= 1;
        const CandI hi = hull_reduce<false>(pts, n, -1.0, 0.0, 0.0, red[parity]);      // (minus the lexicographic maximum)
        parity ^= 1;
        // the corner the march stands on has received the unit vector of the edge that arrived (in_x, in_y); the first corner's comes last
        const int first = lo.idx;
        int cur = lo.idx, steps = 0;
        double in_x = 0.0, in_y = 0.0, first_x = 0.0, first_y = 0.0;
#pragma unroll 1
        for (int chain = 0; chain < 2; ++chain) {
            // the lower chain on the points as they are, from lo to the maximum; the upper chain on the negated points, from hi to minus lo
            const double sg = chain == 0 ? 1.0 : -1.0;
            double cx = chain == 0 ? lo.x : hi.x, cy = chain == 0 ? lo.y : hi.y;
            const double ex = chain == 0 ? -hi.x : -lo.x, ey = chain == 0 ? -hi.y : -lo.y;
            for (int step = 0; step < n && !(cx == ex && cy == ey); ++step) {
                const CandI nx = hull_reduce<true>(pts, n, sg, cx, cy, red[parity]);
                parity ^= 1;
                if (nx.idx < 0) break;                             // (cannot happen before the end point is reached: it is a candidate)
                const double dx = nx.x - cx, dy = nx.y - cy;
                const double len = sqrt(dx * dx + dy * dy);
                perimeter += len;
                // the edge's unit vector in the frame of the stored points
                const double wx = len > 0.0 ? (sg * dx) / len : 0.0, wy = len > 0.0 ? (sg * dy) / len : 0.0;
                if (steps == 0) {
                    first_x = -wx;
                    first_y = -wy;
                } else if (tid == 0) {
                    g[2 * (long long)cur] = in_x - wx;
                    g[2 * (long long)cur + 1] = in_y - wy;
                }
                in_x = wx;
                in_y = wy;
                cur = nx.idx;
                cx = nx.x;
                cy = nx.y;
                ++steps;
            }
        }
        if (steps > 0 && tid == 0) {
            if (cur == first) {                                    // the chain has closed
                g[2 * (long long)first] = in_x + first_x;
                g[2 * (long long)first + 1] = in_y + first_y;
            } else {
                g[2 * (long long)cur] = in_x;
                g[2 * (long long)cur + 1] = in_y;
                g[2 * (long long)first] = first_x;
                g[2 * (long long)first + 1] = first_y;
            }
        }
    }
    if (tid == 0) {
        wr[TB_STATUS] = 0.0;
        if (values) values[row] = (float)perimeter;
    }
    if (!active) return;                                           // (uniform)
    // ---- the gradient w.r.t. the plane's anchor and normal: the slots whose points hold a vector, a slot per thread in slot order
    __syncthreads();                                               // thread 0's stores to g
    const float* vb = verts + b * nverts * 3;
    const float* pb = points ? points + b * n_points * 3 : nullptr;
    double o[3], nn[3], u[3], v[3];
    tape_plane(q, vb, pb, nverts, o, nn, u, v);                    // (n > 0 only with a plane that cuts)
    double pg[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = tid; s < n / 2; s += TB_THREADS) {
        const double gu0 = g[4 * (long long)s], gv0 = g[4 * (long long)s + 1], gu1 = g[4 * (long long)s + 2], gv1 = g[4 * (long long)s + 3];
        if (gu0 == 0.0 && gv0 == 0.0 && gu1 == 0.0 && gv1 == 0.0) continue;
        const int f = slot_face[s];                                // a selected face: its indices are in range
        double P[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int vi = faces[(long long)f * 3 + i];
#pragma unroll
            for (int c = 0; c < 3; ++c) P[i][c] = (double)vb[(long long)vi * 3 + c];
        }
        FaceCut k;
        if (!face_cut(P, o, nn, k)) continue;                      // (it was cut when it took the slot)
        double g0[3], g1[3], h0[3], h1[3], go[3], gn[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g0[c] = gu0 * u[c] + gv0 * v[c];
            g1[c] = gu1 * u[c] + gv1 * v[c];
        }
        cut_terms(k, g0, g1, o, nn, h0, h1, go, gn);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            pg[c] += go[c];
            pg[3 + c] += gn[c];
        }
    }
    block_sum6(pg, red6);
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) wr[TB_DO + c] = pg[c];
    }
}

// what anchor `a` (a vertex id, or nverts + j for point j) receives from the planes, in measurement order: d/do - d/dn (or d/do with a
// fixed direction) as anchor[0], d/dn as anchor[1]; both are staged in LDS, scaled by dout
__device__ __forceinline__ void add_plane_terms(double (&acc)[3], int a, const TapePackB& mp, const int* __restrict__ s_mode, const double (*s_a0)[3],
                                                const double (*s_a1)[3], int n_meas) {
    for (int m = 0; m < n_meas; ++m) {
        if (s_mode[m] < 0) continue;                               // dout == 0
        const straps_tape_t& q = mp.m[m];
        if (q.anchor[0] == a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += s_a0[m][c];
        }
        if (q.anchor[1] == a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += s_a1[m][c];
        }
    }
}

__device__ __forceinline__ void store3(float* __restrict__ p, const double (&acc)[3], int accumulate) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = accumulate ? (float)((double)p[c] + acc[c]) : (float)acc[c];
}

__global__ __launch_bounds__(TB_THREADS) STRAPS_NO_PACKED_FP32 void tape_bwd_gather_kernel(const float* __restrict__ verts, const float* __restrict__ points,
                                                                                          const int32_t* __restrict__ faces,
                                                                                          const uint8_t* __restrict__ face_parts,
                                                                                          const int32_t* __restrict__ vf_offsets,
                                                                                          const int32_t* __restrict__ vf_faces, const TapePackB mp,
                                                                                          const float* __restrict__ dout, const double* __restrict__ ws,
                                                                                          float* __restrict__ dverts, float* __restrict__ dpoints, int nverts,
                                                                                          int n_points, int dpoints_rows, int nfaces, int n_meas, int cap, int nvc,
                                                                                          int per_body, int accumulate) {
    // per measurement: mode -1: dout == 0, nothing; 0: anchor terms only (a NaN row, a plane that cuts nothing); 1: SECTION faces; 2: HULL faces
    __shared__ int s_mode[TB_MAX_MEAS], s_slots[TB_MAX_MEAS];
    __shared__ double s_d[TB_MAX_MEAS], s_o[TB_MAX_MEAS][3], s_n[TB_MAX_MEAS][3], s_u[TB_MAX_MEAS][3], s_v[TB_MAX_MEAS][3], s_a0[TB_MAX_MEAS][3],
        s_a1[TB_MAX_MEAS][3];
    const long long b = blockIdx.x / per_body;
    const int k = (int)(blockIdx.x - b * per_body);
    const int tid = threadIdx.x;
    const float* vb = verts + b * nverts * 3;
    const float* pb = points ? points + b * n_points * 3 : nullptr;
    const long long row_doubles = tb_row_doubles(cap);
    const double* wb = ws + b * n_meas * row_doubles;
    if (tid < n_meas) {
        const straps_tape_t& q = mp.m[tid];
        const double d = (double)dout[b * n_meas + tid];
        const double* wr = wb + tid * row_doubles;
        int mode = -1, slots = 0;
        double o[3], n[3], u[3], v[3], a0[3] = {0.0, 0.0, 0.0}, a1[3] = {0.0, 0.0, 0.0};
        const bool plane_ok = tape_plane(q, vb, pb, nverts, o, n, u, v);
        if (d != 0.0) {                                            // (a NaN is not zero)
            const bool hull = q.kind == STRAPS_TAPE_HULL;
            if (hull && wr[TB_STATUS] != 0.0) {                    // the forward's NaN row: NaN to anchor[0], nothing else
                mode = 0;
                a0[0] = a0[1] = a0[2] = __longlong_as_double(0x7ff8000000000000LL);
            } else {
                mode = plane_ok ? (hull ? 2 : 1) : 0;
                slots = (int)(wr[0] * 0.5);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double go = wr[TB_DO + c], gn = wr[TB_DN + c];
                    a0[c] = q.anchor[1] >= 0 ? d * (go - gn) : d * go;
                    a1[c] = d * gn;
                }
            }
        }
        s_mode[tid] = mode;
        s_slots[tid] = slots;
        s_d[tid] = d;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s_o[tid][c] = o[c];
            s_n[tid][c] = n[c];
            s_u[tid][c] = u[c];
            s_v[tid][c] = v[c];
            s_a0[tid][c] = a0[c];
            s_a1[tid][c] = a1[c];
        }
    }
    __syncthreads();

    if (k == nvc) {
        // ---- the points of the body: thread j owns row j
        if (tid < n_points) {
            double acc[3] = {0.0, 0.0, 0.0};
            add_plane_terms(acc, nverts + tid, mp, s_mode, s_a0, s_a1, n_meas);
            store3(dpoints + (b * dpoints_rows + tid) * 3, acc, accumulate);
        }
        return;
    }

    const int vtx = k * TB_THREADS + tid;
    if (vtx >= nverts) return;
    double acc[3] = {0.0, 0.0, 0.0};
    const int beg = vf_offsets[vtx], end = vf_offsets[vtx + 1];
    for (int e0 = beg; e0 < end; e0 += TB_INFLIGHT) {
        // the dependent chain table -> face -> indices -> corners, TB_INFLIGHT faces wide at every stage
        int f[TB_INFLIGHT], idx[TB_INFLIGHT][3];
        float C[TB_INFLIGHT][3][3];
        unsigned part_bit[TB_INFLIGHT];
        bool ok[TB_INFLIGHT];
#pragma unroll
        for (int j = 0; j < TB_INFLIGHT; ++j) f[j] = e0 + j < end ? vf_faces[e0 + j] : -1;
#pragma unroll
        for (int j = 0; j < TB_INFLIGHT; ++j) {
            const bool in = (unsigned)f[j] < (unsigned)nfaces;
#pragma unroll
            for (int i = 0; i < 3; ++i) idx[j][i] = in ? faces[(long long)f[j] * 3 + i] : -1;
            part_bit[j] = 0u;
            if (in && face_parts) {
                const unsigned lab = face_parts[f[j]];
                part_bit[j] = lab < 32u ? (1u << lab) : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < TB_INFLIGHT; ++j) {
            ok[j] = (unsigned)idx[j][0] < (unsigned)nverts && (unsigned)idx[j][1] < (unsigned)nverts && (unsigned)idx[j][2] < (unsigned)nverts;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) C[j][i][c] = ok[j] ? vb[(long long)idx[j][i] * 3 + c] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < TB_INFLIGHT; ++j) {
            if (!ok[j]) continue;
            double P[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) P[i][c] = (double)C[j][i][c];
            for (int m = 0; m < n_meas; ++m) {
                const int mode = s_mode[m];
                if (mode <= 0) continue;
                const straps_tape_t& q = mp.m[m];
                if (!(q.part_mask == 0u || (part_bit[j] & q.part_mask) != 0u)) continue;
                const double o[3] = {s_o[m][0], s_o[m][1], s_o[m][2]}, n[3] = {s_n[m][0], s_n[m][1], s_n[m][2]};
                FaceCut kc;
                if (!face_cut(P, o, n, kc)) continue;
                const double d = s_d[m];
                double g0[3], g1[3];
                if (mode == 1) {
                    double e[3], len2 = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        e[c] = kc.X[0][c] - kc.X[1][c];
                        len2 += e[c] * e[c];
                    }
                    if (len2 == 0.0) continue;
                    const double sc = d / sqrt(len2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        g0[c] = e[c] * sc;
                        g1[c] = -g0[c];
                    }
                } else {
                    const double* wr = wb + m * row_doubles;
                    const int32_t* slot_face = (const int32_t*)(wr + TB_HEADER + 4LL * cap);
                    int lo = 0, hi = s_slots[m];                   // the row's ascending face indices: the first slot whose face is not below f
                    while (lo < hi) {
                        const int mid = lo + ((hi - lo) >> 1);
                        if (slot_face[mid] < f[j]) lo = mid + 1;
                        else hi = mid;
                    }
                    if (lo >= s_slots[m] || slot_face[lo] != f[j]) continue;      // (a cut face has a slot)
                    const double* gp = wr + TB_HEADER + 2LL * cap + 4LL * lo;
                    const double gu0 = gp[0], gv0 = gp[1], gu1 = gp[2], gv1 = gp[3];
                    if (gu0 == 0.0 && gv0 == 0.0 && gu1 == 0.0 && gv1 == 0.0) continue;      // neither point is a hull corner
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        g0[c] = d * (gu0 * s_u[m][c] + gv0 * s_v[m][c]);
                        g1[c] = d * (gu1 * s_u[m][c] + gv1 * s_v[m][c]);
                    }
                }
                double h0[3], h1[3], go[3], gn[3];
                cut_terms(kc, g0, g1, o, n, h0, h1, go, gn);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (idx[j][i] != vtx) continue;                // every corner that names the vertex adds its terms, point 0 then point 1
                    const int role = i >= kc.a ? i - kc.a : i - kc.a + 3;      // 0: the lone corner a, 1: b, 2: c
                    if (role == 0) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[c] += (1.0 - kc.tb) * h0[c];
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[c] += (1.0 - kc.tc) * h1[c];
                    } else if (role == 1) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[c] += kc.tb * h0[c];
                    } else {
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[c] += kc.tc * h1[c];
                    }
                }
            }
        }
    }
    add_plane_terms(acc, vtx, mp, s_mode, s_a0, s_a1, n_meas);
    store3(dverts + (b * nverts + vtx) * 3, acc, accumulate);
}

// bytes of the workspace, 0 outside the limits (the header states the formula)
size_t tb_workspace_bytes(long long batch, int nverts, int nfaces, int n_meas, int capacity) {
    if (batch <= 0 || batch >= (1LL << 31) || nverts < 1 || nverts > TB_MAX_VERTS || nfaces < 1 || nfaces > TB_MAX_FACES || n_meas < 1 || n_meas > TB_MAX_MEAS) return 0;
    if (batch * n_meas >= (1LL << 31)) return 0;
    if (capacity != 0 && (capacity < 2 || (long long)capacity > 2LL * nfaces)) return 0;
    const long long cap = capacity ? (long long)capacity : 2LL * nfaces;
    const unsigned long long per_row = 8ULL * (unsigned long long)tb_row_doubles(cap);      // < 2^37
    const unsigned long long rows = (unsigned long long)batch * (unsigned long long)n_meas;      // < 2^31
    if (per_row > (1ULL << 62) / rows) return 0;
    const unsigned long long bytes = rows * per_row;
    return bytes >= (1ULL << 62) ? 0 : (size_t)bytes;
}

}  // namespace

extern "C" size_t straps_measure_tape_bwd_workspace_bytes(long long batch, int nverts, int nfaces, int n_meas, int capacity) {
    return tb_workspace_bytes(batch, nverts, nfaces, n_meas, capacity);
}

extern "C" int straps_measure_tape_bwd(const float* verts, const float* points, const int32_t* faces, const uint8_t* face_parts, const int32_t* vf_offsets,
                                       const int32_t* vf_faces, const straps_tape_t* meas, const float* dout, float* dverts, float* dpoints, float* values,
                                       int32_t* counts, void* workspace, long long batch, int nverts, int n_points, int dpoints_rows, int nfaces, int n_meas,
                                       int capacity, int accumulate, void* stream) {
    STRAPS_REQUIRE(verts, "straps_measure_tape_bwd: `verts` is a null pointer");
    STRAPS_REQUIRE(faces, "straps_measure_tape_bwd: `faces` is a null pointer");
    STRAPS_REQUIRE(vf_offsets, "straps_measure_tape_bwd: `vf_offsets` is a null pointer");
    STRAPS_REQUIRE(vf_faces, "straps_measure_tape_bwd: `vf_faces` is a null pointer");
    STRAPS_REQUIRE(meas, "straps_measure_tape_bwd: `meas` is a null pointer");
    STRAPS_REQUIRE(dout, "straps_measure_tape_bwd: `dout` is a null pointer");
    STRAPS_REQUIRE(dverts, "straps_measure_tape_bwd: `dverts` is a null pointer");
    STRAPS_REQUIRE(workspace, "straps_measure_tape_bwd: `workspace` is a null pointer");
    STRAPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "straps_measure_tape_bwd: `workspace` must be 8-byte aligned");
    STRAPS_REQUIRE(batch >= 1 && batch < (1LL << 31), "straps_measure_tape_bwd: `batch` must be in 1..2^31-1 (got %lld)", batch);
    STRAPS_REQUIRE(nverts >= 1 && nverts <= TB_MAX_VERTS, "straps_measure_tape_bwd: `nverts` must be in 1..1048576 (got %d)", nverts);
    STRAPS_REQUIRE(n_points >= 0 && n_points <= TB_MAX_POINTS, "straps_measure_tape_bwd: `n_points` must be in 0..64 (got %d)", n_points);
    STRAPS_REQUIRE(dpoints_rows >= n_points, "straps_measure_tape_bwd: `dpoints_rows` = %d is below n_points = %d", dpoints_rows, n_points);
    STRAPS_REQUIRE(nfaces >= 1 && nfaces <= TB_MAX_FACES, "straps_measure_tape_bwd: `nfaces` must be in 1..715827882 (got %d)", nfaces);
    STRAPS_REQUIRE(n_meas >= 1 && n_meas <= TB_MAX_MEAS, "straps_measure_tape_bwd: `n_meas` must be in 1..32 (got %d)", n_meas);
    STRAPS_REQUIRE(capacity == 0 || (capacity >= 2 && (long long)capacity <= 2LL * nfaces),
                   "straps_measure_tape_bwd: `capacity` must be 0 (the worst case) or in 2..2 * nfaces = %lld (got %d)", 2LL * nfaces, capacity);
    STRAPS_REQUIRE(accumulate == 0 || accumulate == 1, "straps_measure_tape_bwd: `accumulate` must be 0 or 1 (got %d)", accumulate);
    STRAPS_REQUIRE(points || n_points == 0, "straps_measure_tape_bwd: `points` is a null pointer with n_points = %d", n_points);
    TapePackB mp;
    memset(&mp, 0, sizeof(mp));
    bool any_hull = false, any_point = false;
    const int n_anchor = nverts + n_points;
    for (int m = 0; m < n_meas; ++m) {
        const straps_tape_t& q = meas[m];
        STRAPS_REQUIRE(q.kind == STRAPS_TAPE_HULL || q.kind == STRAPS_TAPE_SECTION, "straps_measure_tape_bwd: `meas[%d].kind` is unknown (got %d)", m, q.kind);
        STRAPS_REQUIRE(q.anchor[0] != -1, "straps_measure_tape_bwd: `meas[%d]` has no plane anchor: `anchor[0]` is required", m);
        STRAPS_REQUIRE(q.anchor[0] >= 0 && q.anchor[0] < n_anchor, "straps_measure_tape_bwd: `meas[%d].anchor[0]` = %d is outside 0..nverts + n_points - 1 = %d", m,
                       q.anchor[0], n_anchor - 1);
        STRAPS_REQUIRE(q.anchor[1] == -1 || (q.anchor[1] >= 0 && q.anchor[1] < n_anchor),
                       "straps_measure_tape_bwd: `meas[%d].anchor[1]` = %d is neither -1 nor inside 0..nverts + n_points - 1 = %d", m, q.anchor[1], n_anchor - 1);
        STRAPS_REQUIRE(q.part_mask == 0u || face_parts, "straps_measure_tape_bwd: `meas[%d].part_mask` is set but `face_parts` is a null pointer", m);
        any_hull |= q.kind == STRAPS_TAPE_HULL;
        any_point |= q.anchor[0] >= nverts || q.anchor[1] >= nverts;
        mp.m[m] = q;
        if (q.anchor[1] != -1)      // (dir is not read)
            for (int c = 0; c < 3; ++c) mp.m[m].dir[c] = 0.f;
    }
    STRAPS_REQUIRE(dpoints || !any_point, "straps_measure_tape_bwd: `dpoints` is a null pointer but a measurement is anchored at a point");
    const long long rows = batch * (long long)n_meas;
    STRAPS_REQUIRE(rows < (1LL << 31), "straps_measure_tape_bwd: `batch` * `n_meas` too large for one launch (got %lld)", rows);
    const int nvc = (nverts + TB_THREADS - 1) / TB_THREADS;
    const int per_body = nvc + ((dpoints && n_points > 0) ? 1 : 0);
    const long long gather_blocks = batch * (long long)per_body;
    STRAPS_REQUIRE(gather_blocks < (1LL << 31), "straps_measure_tape_bwd: `batch` too large for one launch");
    const int cap = capacity ? capacity : 2 * nfaces;
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    hipLaunchKernelGGL(tape_bwd_collect_kernel, dim3((unsigned)rows), dim3(TB_THREADS), 0, st, verts, points, faces, face_parts, mp, dout, values, counts, ws, nverts,
                       n_points, nfaces, n_meas, cap);
    STRAPS_CHECK_LAUNCH("tape_bwd_collect_kernel");
    if (any_hull) {
        hipLaunchKernelGGL(tape_bwd_hull_kernel, dim3((unsigned)rows), dim3(TB_THREADS), 0, st, verts, points, faces, mp, dout, values, ws, nverts, n_points, n_meas,
                           cap);
        STRAPS_CHECK_LAUNCH("tape_bwd_hull_kernel");
    }
    hipLaunchKernelGGL(tape_bwd_gather_kernel, dim3((unsigned)gather_blocks), dim3(TB_THREADS), 0, st, verts, points, faces, face_parts, vf_offsets, vf_faces, mp, dout,
                       (const double*)ws, dverts, dpoints, nverts, n_points, dpoints_rows, nfaces, n_meas, cap, nvc, per_body, accumulate);
    STRAPS_CHECK_LAUNCH("tape_bwd_gather_kernel");
    return STRAPS_OK;
}
