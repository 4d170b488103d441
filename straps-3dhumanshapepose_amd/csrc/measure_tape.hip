// measure_tape.hip -- tape-measure girths of a batch of meshes on the device: the perimeter of the convex hull of a plane section, and the
// section's length, with the plane's normal given once or taken per body from two anchors (include/straps_hip.h states the definitions).
// The vertices are read as fp32; every product, sum, division and square root is done in double; each result is rounded to float once.
// Gather- and latency-bound work, no MFMA.
//
// Two launches per call, both on the caller's stream, no synchronisation, no allocation, no atomics:
//   1. collect kernel : workgroup (body, measurement).  The faces are walked in index order, 256 per trip, a face per thread: corners loaded
//                       once, the cut decided, and a cut face takes its slot from the ballot of its wave (the cut lanes below it), the cut
//                       counts of the waves below it (LDS, one barrier per trip) and the running count of the trips before -- slot order is
//                       face order.  A HULL stores the (u, v) of the face's two points as doubles while their index is below the capacity.
//                       The section length is added per thread in trip order, the wave adds its 64 lanes in a fixed shuffle tree, the four
//                       wave sums are added in wave order.  The workgroup writes the count and the length into the row's workspace header,
//                       `counts`, and -- for a SECTION -- the value.
//   2. hull kernel    : workgroup (body, measurement), launched only when a HULL is asked for.  A monotone march over the stored points: from
//                       the lexicographic minimum of (u, v), among the points lexicographically GREATER than the current one the most
//                       clockwise (of collinear ones the farther) until the lexicographic maximum is reached; then the same on the negated
//                       points, which is the upper chain back.  Every choice is a workgroup reduction of fixed shape over COORDINATES (no
//                       slot index takes part: equal points are interchangeable).  A step moves strictly forward in lexicographic order, so
//                       a chain ends after at most `count` steps whatever rounding does to the orientation test; the loops carry that cap.
// A workgroup touches one (body, measurement) and every reduction has a fixed shape: a row is the same bits alone or in any batch and from
// run to run, and a NaN in one body stays there.  The hull kernel reads the header and the first min(count, capacity) points: what the first
// kernel wrote.
#include "common.h"

#include <string.h>

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_FACES_PER_BLOCK = 256;       // == hipabi.MEASURE_TAPE_FACES_PER_BLOCK: faces of one trip of a collect workgroup
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_MAX_MEAS = 32;
constexpr int MT_MAX_POINTS = 64;
constexpr int MT_MAX_VERTS = 1 << 20;
constexpr int MT_MAX_FACES = 0x7fffffff / 3;
constexpr int MT_HEADER = 2;                  // doubles in front of a row's points: count, section length

struct TapePack {
    straps_tape_t m[MT_MAX_MEAS];
};

__device__ __forceinline__ const float* tape_anchor_ptr(const float* __restrict__ vb, const float* __restrict__ pb, int a, int nverts) {
    return a < nverts ? vb + (long long)a * 3 : pb + (long long)(a - nverts) * 3;
}

__device__ __forceinline__ double tape_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000LL); }      // (false for a NaN)

// the plane of (body, measurement): anchor o, normal n, and the basis (u, v) of the header; false when the normal cuts nothing
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

__global__ __launch_bounds__(MT_THREADS) STRAPS_NO_PACKED_FP32 void tape_collect_kernel(const float* __restrict__ verts, const float* __restrict__ points,
                                                                                       const int32_t* __restrict__ faces,
                                                                                       const uint8_t* __restrict__ face_parts, const TapePack mp,
                                                                                       float* __restrict__ out, int32_t* __restrict__ counts,
                                                                                       double* __restrict__ ws, int nverts, int n_points, int nfaces,
                                                                                       int n_meas, int cap) {
    __shared__ int wave_cut[2][MT_WAVES];
    __shared__ double wave_len[MT_WAVES];
    const long long row = blockIdx.x;                              // body * n_meas + measurement
    const long long b = row / n_meas;
    const int m = (int)(row - b * n_meas);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const straps_tape_t& q = mp.m[m];
    const float* vb = verts + b * nverts * 3;
    const float* pb = points ? points + b * n_points * 3 : nullptr;
    double* wr = ws + row * (MT_HEADER + 2LL * cap);
    double* pts = wr + MT_HEADER;
    double o[3], n[3], u[3], v[3];
    const bool plane_ok = tape_plane(q, vb, pb, nverts, o, n, u, v);      // (uniform over the workgroup)
    const bool store = q.kind == STRAPS_TAPE_HULL;
    int base = 0;                                                  // cut faces of the trips before this one
    double acc = 0.0;
    if (plane_ok) {
        int parity = 0;
        for (int f0 = 0; f0 < nfaces; f0 += MT_FACES_PER_BLOCK, parity ^= 1) {      // (f0 <= nfaces - 1 < 2^31 / 3: f0 + 256 does not overflow)
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
                    }
                }
            }
            const unsigned long long mask = __ballot(cut);          // wave64: one bit per lane
            if (lane == 0) wave_cut[parity][wave] = __popcll(mask);
            __syncthreads();      // (one barrier per trip: the next trip writes the other half of wave_cut, the one after it comes behind the next barrier)
            int before = base, total = 0;
#pragma unroll
            for (int w = 0; w < MT_WAVES; ++w) {
                const int cw = wave_cut[parity][w];
                before += w < wave ? cw : 0;
                total += cw;
            }
            if (cut && store) {
                const long long slot = before + __popcll(mask & ((1ull << lane) - 1ull));      // < nfaces
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
        for (int w = 1; w < MT_WAVES; ++w) s += wave_len[w];
        wr[0] = (double)(2 * (long long)base);
        wr[1] = s;
        if (counts) counts[row] = 2 * base;                        // (2 * nfaces < 2^31)
        if (!store) out[row] = (float)s;
    }
}

// ---- the hull kernel's reductions: a candidate is a point (x, y) or nothing (passed by value: by reference the fold's candidates went to
// scratch memory, 96 bytes per lane)
struct Cand {
    double x, y;
    int have;
};

__device__ __forceinline__ bool lex_less(double ax, double ay, double bx, double by) { return ax < bx || (ax == bx && ay < by); }

// of two candidates the lexicographically smaller
__device__ __forceinline__ Cand pick_min(Cand a, Cand b) {
    if (!b.have) return a;
    if (!a.have) return b;
    return lex_less(b.x, b.y, a.x, a.y) ? b : a;
}
// of two candidates, both lexicographically greater than (cx, cy), the more clockwise seen from there; of collinear ones the farther, which
// on a ray into that half-plane is the lexicographically greater.  The products are rounded one by one (no fused multiply-add): the test is
// antisymmetric in (a, b), and exactly 0 for equal points
__device__ __forceinline__ Cand pick_cw(Cand a, Cand b, double cx, double cy) {
    if (!b.have) return a;
    if (!a.have) return b;
    const double cross = __dsub_rn(__dmul_rn(a.x - cx, b.y - cy), __dmul_rn(a.y - cy, b.x - cx));
    if (cross < 0.0) return b;
    if (cross > 0.0) return a;
    return lex_less(a.x, a.y, b.x, b.y) ? b : a;
}

template <bool MARCH>
__device__ __forceinline__ Cand pick(Cand a, Cand b, double cx, double cy) {
    return MARCH ? pick_cw(a, b, cx, cy) : pick_min(a, b);
}

// one workgroup reduction over the points sg * pts[i], i < n: MARCH: the most clockwise of those lexicographically greater than (cx, cy);
// otherwise the lexicographic minimum.  Thread t folds i = t, t + 256, .. in that order, the wave folds its lanes in a shuffle tree, every
// thread folds the four wave results in wave order: all threads return the same candidate.  `red` is the half of the LDS buffer of this call's
// parity (one barrier per call, as in the collect kernel).
template <bool MARCH>
__device__ __forceinline__ Cand hull_reduce(const double* __restrict__ pts, int n, double sg, double cx, double cy, Cand* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Cand best = {0.0, 0.0, 0};
    for (int i = tid; i < n; i += MT_THREADS) {
        Cand c = {sg * pts[2 * (long long)i], sg * pts[2 * (long long)i + 1], 1};
        if (MARCH) c.have = lex_less(cx, cy, c.x, c.y) ? 1 : 0;
        best = pick<MARCH>(best, c, cx, cy);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Cand c;
        c.x = __shfl_down(best.x, off, 64);
        c.y = __shfl_down(best.y, off, 64);
        c.have = __shfl_down(best.have, off, 64);
        best = pick<MARCH>(best, c, cx, cy);
    }
    if (lane == 0) red[wave] = best;
    __syncthreads();
    Cand r = red[0];
#pragma unroll
    for (int w = 1; w < MT_WAVES; ++w) r = pick<MARCH>(r, red[w], cx, cy);
    return r;
}

__global__ __launch_bounds__(MT_THREADS) STRAPS_NO_PACKED_FP32 void tape_hull_kernel(const TapePack mp, const double* __restrict__ ws, float* __restrict__ out,
                                                                                    int n_meas, int cap) {
    __shared__ Cand red[2][MT_WAVES];
    const long long row = blockIdx.x;
    const int m = (int)(row % n_meas);
    if (mp.m[m].kind != STRAPS_TAPE_HULL) return;                  // (uniform)
    const double* wr = ws + row * (MT_HEADER + 2LL * cap);
    const double* pts = wr + MT_HEADER;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double countd = wr[0];                                   // (an integer below 2^31, exact)
    if (!(countd <= (double)cap)) {                               // more points than the row holds: NaN, as the header says
        if (threadIdx.x == 0) out[row] = (float)nan;
        return;
    }
    const int n = (int)countd;
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += MT_THREADS) bad |= !(finite_d(pts[2 * (long long)i]) && finite_d(pts[2 * (long long)i + 1]));
    if (__syncthreads_or(bad)) {
        if (threadIdx.x == 0) out[row] = (float)nan;
        return;
    }
    double perimeter = 0.0;
    if (n > 0) {
        int parity = 0;
        const Cand lo = hull_reduce<false>(pts, n, 1.0, 0.0, 0.0, red[parity]);
        parity ^= 1;
        const Cand hi = hull_reduce<false>(pts, n, -1.0, 0.0, 0.0, red[parity]);      // (minus the lexicographic maximum)
        parity ^= 1;
#pragma unroll 1
        for (int chain = 0; chain < 2; ++chain) {
            // the lower chain on the points as they are, from lo to the maximum; the upper chain on the negated points, from hi to minus lo
            const double sg = chain == 0 ? 1.0 : -1.0;
            double cx = chain == 0 ? lo.x : hi.x, cy = chain == 0 ? lo.y : hi.y;
            const double ex = chain == 0 ? -hi.x : -lo.x, ey = chain == 0 ? -hi.y : -lo.y;
            for (int step = 0; step < n && !(cx == ex && cy == ey); ++step) {
                const Cand nx = hull_reduce<true>(pts, n, sg, cx, cy, red[parity]);
                parity ^= 1;
                if (!nx.have) break;                               // (cannot happen before the end point is reached: it is a candidate)
                const double dx = nx.x - cx, dy = nx.y - cy;
                perimeter += sqrt(dx * dx + dy * dy);
                cx = nx.x;
                cy = nx.y;
            }
        }
    }
    if (threadIdx.x == 0) out[row] = (float)perimeter;
}

}  // namespace

extern "C" size_t straps_measure_tape_workspace_bytes(long long batch, int nfaces, int n_meas, int capacity) {
    if (batch <= 0 || batch >= (1LL << 31) || nfaces < 1 || nfaces > MT_MAX_FACES || n_meas < 1 || n_meas > MT_MAX_MEAS) return 0;
    if (batch * n_meas >= (1LL << 31)) return 0;
    if (capacity != 0 && (capacity < 2 || (long long)capacity > 2LL * nfaces)) return 0;
    const unsigned long long cap = capacity ? (unsigned long long)capacity : 2ULL * (unsigned long long)nfaces;
    const unsigned long long per_row = 8ULL * (MT_HEADER + 2ULL * cap);                  // < 2^36
    const unsigned long long rows = (unsigned long long)batch * (unsigned long long)n_meas;      // < 2^31
    if (per_row > (1ULL << 62) / rows) return 0;
    const unsigned long long bytes = rows * per_row;
    return bytes >= (1ULL << 62) ? 0 : (size_t)bytes;
}

extern "C" int straps_measure_tape(const float* verts, const float* points, const int32_t* faces, const uint8_t* face_parts, const straps_tape_t* meas, float* out,
                                   int32_t* counts, void* workspace, long long batch, int nverts, int n_points, int nfaces, int n_meas, int capacity,
                                   void* stream) {
    STRAPS_REQUIRE(verts, "straps_measure_tape: `verts` is a null pointer");
    STRAPS_REQUIRE(faces, "straps_measure_tape: `faces` is a null pointer");
    STRAPS_REQUIRE(meas, "straps_measure_tape: `meas` is a null pointer");
    STRAPS_REQUIRE(out, "straps_measure_tape: `out` is a null pointer");
    STRAPS_REQUIRE(workspace, "straps_measure_tape: `workspace` is a null pointer");
    STRAPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "straps_measure_tape: `workspace` must be 8-byte aligned");
    STRAPS_REQUIRE(batch >= 1 && batch < (1LL << 31), "straps_measure_tape: `batch` must be in 1..2^31-1 (got %lld)", batch);
    STRAPS_REQUIRE(nverts >= 1 && nverts <= MT_MAX_VERTS, "straps_measure_tape: `nverts` must be in 1..1048576 (got %d)", nverts);
    STRAPS_REQUIRE(n_points >= 0 && n_points <= MT_MAX_POINTS, "straps_measure_tape: `n_points` must be in 0..64 (got %d)", n_points);
    STRAPS_REQUIRE(nfaces >= 1 && nfaces <= MT_MAX_FACES, "straps_measure_tape: `nfaces` must be in 1..715827882 (got %d)", nfaces);
    STRAPS_REQUIRE(n_meas >= 1 && n_meas <= MT_MAX_MEAS, "straps_measure_tape: `n_meas` must be in 1..32 (got %d)", n_meas);
    STRAPS_REQUIRE(capacity == 0 || (capacity >= 2 && (long long)capacity <= 2LL * nfaces),
                   "straps_measure_tape: `capacity` must be 0 (the worst case) or in 2..2 * nfaces = %lld (got %d)", 2LL * nfaces, capacity);
    STRAPS_REQUIRE(points || n_points == 0, "straps_measure_tape: `points` is a null pointer with n_points = %d", n_points);
    TapePack mp;
    memset(&mp, 0, sizeof(mp));
    bool any_hull = false;
    const int n_anchor = nverts + n_points;
    for (int m = 0; m < n_meas; ++m) {
        const straps_tape_t& q = meas[m];
        STRAPS_REQUIRE(q.kind == STRAPS_TAPE_HULL || q.kind == STRAPS_TAPE_SECTION, "straps_measure_tape: `meas[%d].kind` is unknown (got %d)", m, q.kind);
        STRAPS_REQUIRE(q.anchor[0] != -1, "straps_measure_tape: `meas[%d]` has no plane anchor: `anchor[0]` is required", m);
        STRAPS_REQUIRE(q.anchor[0] >= 0 && q.anchor[0] < n_anchor, "straps_measure_tape: `meas[%d].anchor[0]` = %d is outside 0..nverts + n_points - 1 = %d", m,
                       q.anchor[0], n_anchor - 1);
        STRAPS_REQUIRE(q.anchor[1] == -1 || (q.anchor[1] >= 0 && q.anchor[1] < n_anchor),
                       "straps_measure_tape: `meas[%d].anchor[1]` = %d is neither -1 nor inside 0..nverts + n_points - 1 = %d", m, q.anchor[1], n_anchor - 1);
        STRAPS_REQUIRE(q.part_mask == 0u || face_parts, "straps_measure_tape: `meas[%d].part_mask` is set but `face_parts` is a null pointer", m);
        any_hull |= q.kind == STRAPS_TAPE_HULL;
        mp.m[m] = q;
        if (q.anchor[1] != -1)      // (dir is not read)
            for (int c = 0; c < 3; ++c) mp.m[m].dir[c] = 0.f;
    }
    const long long rows = batch * (long long)n_meas;
    STRAPS_REQUIRE(rows < (1LL << 31), "straps_measure_tape: `batch` * `n_meas` too large for one launch (got %lld)", rows);
    const int cap = capacity ? capacity : 2 * nfaces;
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    hipLaunchKernelGGL(tape_collect_kernel, dim3((unsigned)rows), dim3(MT_THREADS), 0, st, verts, points, faces, face_parts, mp, out, counts, ws, nverts, n_points,
                       nfaces, n_meas, cap);
    STRAPS_CHECK_LAUNCH("tape_collect_kernel");
    if (any_hull) {
        hipLaunchKernelGGL(tape_hull_kernel, dim3((unsigned)rows), dim3(MT_THREADS), 0, st, mp, (const double*)ws, out, n_meas, cap);
        STRAPS_CHECK_LAUNCH("tape_hull_kernel");
    }
    return STRAPS_OK;
}
