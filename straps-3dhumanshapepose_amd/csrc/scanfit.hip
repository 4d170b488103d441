// scanfit.hip -- the 3-D scan term of test-time fitting: straps_scan_energy (include/straps_hip.h states the objective).
//
// The two-sided nearest-point energy between a body's translated vertices X and a cloud of 3-D points, and its gradient.  Six launches, every
// float sum in a fixed order, no float atomics:
//   scan_prep_kernel    one lane per vertex / point: X = verts + t as float4 into the workspace, both key lists set to "no partner", the
//                       body's count of valid points zeroed;
//   scan_search_kernel  the distance matrix, once per direction (<true>: every point looks for its vertex; <false>: every vertex for its point).
//                       A work item is QCHUNK = 256 lanes x PPL = 4 queries against one LDS tile of 1024 candidates (float4, 16 KiB): a lane
//                       holds its four queries in registers, so that one broadcast LDS read of a candidate serves four distances.  A body's
//                       items (query chunks x candidate tiles) are walked by at most WPB workgroups.  A lane scans its tile in ascending
//                       order with a strict compare and merges its result into the query's 64-bit key, (bits of d2) << 32 | index, with an
//                       integer atomicMin: squared distances are not negative, so their bit patterns order as they do, and among equal
//                       distances the lowest index wins -- whatever the tiling and whichever workgroup comes first;
//   scan_point_kernel   one lane per point: key -> nearest_vertex, rho and the point's pull on its vertex (unscaled), one partial sum of rho
//                       per 256 points, the valid points counted with an integer atomicAdd;
//   scan_gather_kernel  the scatter as a gather, with one summation order per vertex (ascending point index).  A workgroup owns 256 vertices.
//                       Per tile of 4096 entries of the nearest list, each of its four waves sifts a quarter for the points that chose one
//                       of those vertices and compacts them, by ballot and hence in point order, into its list in LDS; then every lane
//                       walks the four short lists for its own vertex (a lane of sil_gather_kernel walks the whole nearest list: here the
//                       workgroup reads it once).  Then the vertex's own mesh-to-scan term from its key, dverts, nearest_point and one
//                       partial of (dtrans, rho) per 256 vertices;
//   scan_finish_kernel  one workgroup per body: energy2 and dtrans from the partials, strided sums and a fixed tree.
#include "common.h"

namespace {

constexpr int BLK = 256;                  // lanes of a workgroup
constexpr int PPL = 4;                    // queries a lane of the search holds in registers
constexpr int QCHUNK = BLK * PPL;         // queries of a work item
constexpr int VTILE = 1024;               // vertices per LDS tile when the points search (float4: 16 KiB)
constexpr int PTILE = 1024;               // points per LDS tile when the vertices search
constexpr int WPB = 512;                  // workgroups per body of a search
constexpr int GTILE = 4096;               // points of the nearest list a workgroup of the gather sifts between two barriers
constexpr int GWAVE = GTILE / (BLK / 64); // of which every wave takes a quarter: the most entries its list can get
constexpr unsigned long long NO_KEY = ~0ull;

// fixed-order sum over the 256 threads of a workgroup; every thread gets the result.  `s` is reusable after the call.  (as csrc/silfit.hip)
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

struct ScanWs {
    float4* X;                   // [B][nverts] verts + t (w = 0)
    float4* pc;                  // [B][np] xyz: d rho / d X of the point's nearest vertex, w: rho (zeros at a point without a partner)
    float4* pv;                  // [B][nbv] partials per 256 vertices: dtrans xyz, sum of the mesh-to-scan rho
    unsigned long long* keyv;    // [B][nverts] (bits of d2) << 32 | nearest point; NO_KEY = none
    unsigned long long* keyp;    // [B][np] (bits of d2) << 32 | nearest vertex
    int32_t* cnt;                // [B][4] valid points of the body (one word used)
    int32_t* nearv;              // [B][np] nearest vertex of every point (the caller's buffer when given)
    float* pe;                   // [B][nbp] partial sums of the scan-to-mesh rho per 256 points
};

__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }

// rho(r2) and its derivative
__device__ __forceinline__ void robust(float r2, float sigma, float& rho, float& drho) {
    if (sigma > 0.f) {
        const float s2 = sigma * sigma, q = s2 / (s2 + r2);
        rho = q * r2;
        drho = q * q;
    } else {
        rho = r2;
        drho = 1.f;
    }
}

__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void scan_prep_kernel(const float* __restrict__ verts, const float* __restrict__ trans, int ld_trans, ScanWs w,
                                                                             int nverts, int npoints, int nb) {
    const long long b = blockIdx.x / nb;
    const int blk = blockIdx.x - (int)(b * nb), e = blk * BLK + threadIdx.x;
    if (e < nverts) {
        const size_t a = (size_t)b * nverts + e;
        const float tx = trans[b * ld_trans], ty = trans[b * ld_trans + 1], tz = trans[b * ld_trans + 2];
        w.X[a] = make_float4(verts[a * 3] + tx, verts[a * 3 + 1] + ty, verts[a * 3 + 2] + tz, 0.f);
        w.keyv[a] = NO_KEY;
    }
    if (e < npoints) w.keyp[(size_t)b * npoints + e] = NO_KEY;
    if (e == 0) w.cnt[b * 4] = 0;
}

// S2M: the queries are the points, the candidates the vertices; else the other way round.  An invalid point has a NaN or an infinity among
// its coordinates: as a query every distance of it is NaN or +inf and never below the running minimum (+inf), so it stays without a key; as a
// candidate it is stored as (+inf, +inf, +inf), whose distance to a finite query is +inf.
template <bool S2M>
__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void scan_search_kernel(ScanWs w, const float* __restrict__ points, int nverts, int npoints, int nwg) {
    constexpr int TILE = S2M ? VTILE : PTILE;
    __shared__ float4 sc[TILE];
    const long long b = blockIdx.x / nwg;
    const int blk = blockIdx.x - (int)(b * nwg), tid = threadIdx.x;
    const int nq = S2M ? npoints : nverts, nc = S2M ? nverts : npoints;
    const int ctiles = (nc + TILE - 1) / TILE, items = ((nq + QCHUNK - 1) / QCHUNK) * ctiles;
    const float4* X = w.X + (size_t)b * nverts;
    const float* P = points + (size_t)b * npoints * 3;
    unsigned long long* key = S2M ? w.keyp + (size_t)b * npoints : w.keyv + (size_t)b * nverts;
    for (int item = blk; item < items; item += nwg) {                     // (uniform over the workgroup: the barriers below are reached by all)
        const int qc = item / ctiles, c0 = (item - qc * ctiles) * TILE, n = min(TILE, nc - c0);
        float qx[PPL], qy[PPL], qz[PPL], bd[PPL];
        int bi[PPL];
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
            const int q = qc * QCHUNK + k * BLK + tid;
            qx[k] = qy[k] = qz[k] = NAN;                                  // (a lane past the end: a query that finds nothing)
            if (q < nq) {
                if (S2M) { qx[k] = P[(size_t)q * 3]; qy[k] = P[(size_t)q * 3 + 1]; qz[k] = P[(size_t)q * 3 + 2]; }
                else { const float4 x = X[q]; qx[k] = x.x; qy[k] = x.y; qz[k] = x.z; }
            }
            bd[k] = INFINITY;
            bi[k] = -1;
        }
        __syncthreads();                                                  // the tile of the item before is no longer read
        for (int i = tid; i < n; i += BLK) {
            float4 c;
            if (S2M) c = X[c0 + i];
            else {
                const float* p = P + (size_t)(c0 + i) * 3;
                c = make_float4(p[0], p[1], p[2], 0.f);
                if (!finite3(c.x, c.y, c.z)) c = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
            }
            sc[i] = c;
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const float4 c = sc[i];                                       // one broadcast read, PPL distances
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
                const float dx = c.x - qx[k], dy = c.y - qy[k], dz = c.z - qz[k];      // (+-(X - p): the squares are the same)
                const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                if (d < bd[k]) { bd[k] = d; bi[k] = c0 + i; }
            }
        }
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
            const int q = qc * QCHUNK + k * BLK + tid;
            if (q < nq && bi[k] >= 0) atomicMin(&key[q], ((unsigned long long)__float_as_uint(bd[k]) << 32) | (unsigned)bi[k]);
        }
    }
}

__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void scan_point_kernel(ScanWs w, const float* __restrict__ points, int nverts, int npoints, int nbp, float sigma) {
    __shared__ float red[BLK];
    __shared__ int cnt;
    const long long b = blockIdx.x / nbp;
    const int blk = blockIdx.x - (int)(b * nbp), i = blk * BLK + threadIdx.x;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    float rho = 0.f;
    if (i < npoints) {
        const size_t a = (size_t)b * npoints + i;
        const float px = points[a * 3], py = points[a * 3 + 1], pz = points[a * 3 + 2];
        const bool valid = finite3(px, py, pz);
        const unsigned long long key = w.keyp[a];
        const int n = valid && key != NO_KEY ? (int)(unsigned)(key & 0xffffffffu) : -1;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n >= 0 && n < nverts) {
            const float4 x = w.X[(size_t)b * nverts + n];
            float drho;
            robust(__uint_as_float((unsigned)(key >> 32)), sigma, rho, drho);
            const float k = 2.f * drho;
            c = make_float4(k * (x.x - px), k * (x.y - py), k * (x.z - pz), rho);
        }
        w.nearv[a] = n;
        w.pc[a] = c;
        if (valid) atomicAdd(&cnt, 1);                                   // (integers: any order gives the same count)
    }
    const float sum = block_sum(rho, red);                               // (its barriers also order the count)
    if (threadIdx.x == 0) {
        w.pe[b * nbp + blk] = sum;
        if (cnt) atomicAdd(&w.cnt[b * 4], cnt);
    }
}

__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void scan_gather_kernel(ScanWs w, const float* __restrict__ points, float* __restrict__ dverts,
                                                                               int32_t* __restrict__ nearest_point, int nverts, int npoints, int nbv, float sigma,
                                                                               float w_s2m, float w_m2s) {
    __shared__ uint32_t list[BLK / 64][GWAVE];      // per wave: (vertex - first vertex of the workgroup) << 20 | point, in point order
    __shared__ int lcnt[BLK / 64];
    __shared__ float red[BLK];
    const long long b = blockIdx.x / nbv;
    const int blk = blockIdx.x - (int)(b * nbv), v = blk * BLK + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int32_t* near_b = w.nearv + (size_t)b * npoints;
    const float4* pc = w.pc + (size_t)b * npoints;
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (w_s2m != 0.f) {
        for (int p0 = 0; p0 < npoints; p0 += GTILE) {                     // (uniform over the workgroup: the barriers below are reached by all)
            // every wave sifts its quarter of the tile for the points that chose one of the workgroup's 256 vertices; a ballot keeps them in point order
            int cnt = 0;
            const int q0 = p0 + wv * GWAVE;
            for (int i = 0; i < GWAVE; i += 64) {
                const int q = q0 + i + lane;
                const int n = q < npoints ? near_b[q] : -1;
                const bool mine = (unsigned)(n - blk * BLK) < (unsigned)BLK;      // (-1 and every other workgroup's vertices fail)
                const unsigned long long m = __ballot(mine);
                if (mine) list[wv][cnt + __popcll(m & ((1ull << lane) - 1ull))] = ((unsigned)(n - blk * BLK) << 20) | (unsigned)q;
                cnt += __popcll(m);
            }
            if (lane == 0) lcnt[wv] = cnt;
            __syncthreads();
            // a vertex walks the four lists in wave order, which is point order, and adds the points that chose it
#pragma unroll
            for (int k = 0; k < BLK / 64; ++k) {
                const int nk = lcnt[k];
                for (int j = 0; j < nk; ++j) {
                    const unsigned e = list[k][j];
                    if ((e >> 20) == threadIdx.x) {
                        const float4 c = pc[e & 0xfffffu];
                        ax += c.x;
                        ay += c.y;
                        az += c.z;
                    }
                }
            }
            __syncthreads();                                              // the lists are rewritten by the next tile
        }
    }
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    if (v < nverts) {
        const size_t a = (size_t)b * nverts + v;
        const float cs = w_s2m / (float)max(1, w.cnt[b * 4]), cm = w_m2s / (float)nverts;
        const unsigned long long key = w.keyv[a];
        const int m = key != NO_KEY ? (int)(unsigned)(key & 0xffffffffu) : -1;
        float mx = 0.f, my = 0.f, mz = 0.f;
        if (m >= 0 && m < npoints) {
            const float* p = points + ((size_t)b * npoints + m) * 3;
            const float4 x = w.X[a];
            float rho, drho;
            robust(__uint_as_float((unsigned)(key >> 32)), sigma, rho, drho);
            const float k = 2.f * drho;
            mx = k * (x.x - p[0]);
            my = k * (x.y - p[1]);
            mz = k * (x.z - p[2]);
            part[3] = rho;
        }
        part[0] = fmaf(cs, ax, cm * mx);
        part[1] = fmaf(cs, ay, cm * my);
        part[2] = fmaf(cs, az, cm * mz);
        if (dverts) {
            dverts[a * 3] = part[0];
            dverts[a * 3 + 1] = part[1];
            dverts[a * 3 + 2] = part[2];
        }
        if (nearest_point) nearest_point[a] = m;
    }
    float sums[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) sums[q] = block_sum(part[q], red);
    if (threadIdx.x == 0) w.pv[b * nbv + blk] = make_float4(sums[0], sums[1], sums[2], sums[3]);
}

__global__ __launch_bounds__(BLK) STRAPS_NO_PACKED_FP32 void scan_finish_kernel(ScanWs w, float* __restrict__ energy2, float* __restrict__ dtrans, int nverts, int nbv, int nbp) {
    __shared__ float red[BLK];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    float e_s = 0.f, c[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = tid; q < nbp; q += BLK) e_s += w.pe[b * nbp + q];
    for (int q = tid; q < nbv; q += BLK) {
        const float4 p = w.pv[b * nbv + q];
        c[0] += p.x;
        c[1] += p.y;
        c[2] += p.z;
        c[3] += p.w;
    }
    e_s = block_sum(e_s, red);
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = block_sum(c[k], red);
    if (tid == 0) {
        if (energy2) {
            energy2[b * 2] = e_s / (float)max(1, w.cnt[b * 4]);
            energy2[b * 2 + 1] = c[3] / (float)nverts;
        }
        if (dtrans) {
            dtrans[b * 3] = c[0];
            dtrans[b * 3 + 1] = c[1];
            dtrans[b * 3 + 2] = c[2];
        }
    }
}

inline bool finite_nonneg(float x) { return x >= 0.f && x < INFINITY; }      // (a NaN fails)

}  // namespace

extern "C" size_t straps_scan_energy_workspace_bytes(long long batch, int nverts, int npoints) {
    if (batch <= 0 || batch >= (1LL << 19) || nverts < 1 || nverts > (1 << 20) || npoints < 1 || npoints > (1 << 20)) return 0;
    const long long nbv = (nverts + BLK - 1) / BLK, nbp = (npoints + BLK - 1) / BLK;
    return (size_t)batch * (size_t)(24LL * nverts + 28LL * npoints + 16 * nbv + 4 * nbp + 16);
}

extern "C" int straps_scan_energy(const float* verts, const float* trans, int ld_trans, const float* points, const straps_scan_opts_t* opts,
                                  float* energy2, float* dverts, float* dtrans, int32_t* nearest_vertex, int32_t* nearest_point,
                                  void* workspace, long long batch, int nverts, int npoints, void* stream) {
    STRAPS_REQUIRE(opts, "straps_scan_energy: null opts");
    STRAPS_REQUIRE(verts, "straps_scan_energy: null verts");
    STRAPS_REQUIRE(trans, "straps_scan_energy: null trans");
    STRAPS_REQUIRE(points, "straps_scan_energy: null points");
    STRAPS_REQUIRE(workspace, "straps_scan_energy: null workspace");
    STRAPS_REQUIRE(((uintptr_t)workspace & 15) == 0, "straps_scan_energy: workspace must be 16-byte aligned");
    STRAPS_REQUIRE(energy2 || dverts || dtrans || nearest_vertex || nearest_point,
                   "straps_scan_energy: all outputs are null (energy2, dverts, dtrans, nearest_vertex, nearest_point): give at least one");
    STRAPS_REQUIRE(nverts >= 1 && nverts <= (1 << 20), "straps_scan_energy: nverts must be in 1..2^20 (got %d)", nverts);
    STRAPS_REQUIRE(npoints >= 1 && npoints <= (1 << 20), "straps_scan_energy: npoints must be in 1..2^20 (got %d)", npoints);
    STRAPS_REQUIRE(ld_trans >= 3, "straps_scan_energy: ld_trans must be at least 3 (got %d)", ld_trans);
    STRAPS_REQUIRE(finite_nonneg(opts->sigma), "straps_scan_energy: sigma must be finite and not negative");
    STRAPS_REQUIRE(finite_nonneg(opts->w_s2m), "straps_scan_energy: w_s2m must be finite and not negative");
    STRAPS_REQUIRE(finite_nonneg(opts->w_m2s), "straps_scan_energy: w_m2s must be finite and not negative");
    STRAPS_REQUIRE(batch > 0 && batch < (1LL << 19), "straps_scan_energy: batch must be in 1..2^19-1 (got %lld)", batch);
    const int nbv = (nverts + BLK - 1) / BLK, nbp = (npoints + BLK - 1) / BLK, nb = nbv > nbp ? nbv : nbp;
    // the workspace, in the order of straps_scan_energy_workspace_bytes: 16-byte entries first, then 8-byte ones, then words
    ScanWs w;
    char* p = static_cast<char*>(workspace);
    w.X = reinterpret_cast<float4*>(p);                  p += (size_t)batch * nverts * sizeof(float4);
    w.pc = reinterpret_cast<float4*>(p);                 p += (size_t)batch * npoints * sizeof(float4);
    w.pv = reinterpret_cast<float4*>(p);                 p += (size_t)batch * nbv * sizeof(float4);
    w.cnt = reinterpret_cast<int32_t*>(p);               p += (size_t)batch * 16;
    w.keyv = reinterpret_cast<unsigned long long*>(p);   p += (size_t)batch * nverts * 8;
    w.keyp = reinterpret_cast<unsigned long long*>(p);   p += (size_t)batch * npoints * 8;
    int32_t* near_ws = reinterpret_cast<int32_t*>(p);    p += (size_t)batch * npoints * sizeof(int32_t);
    w.pe = reinterpret_cast<float*>(p);
    w.nearv = nearest_vertex ? nearest_vertex : near_ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(scan_prep_kernel, dim3((unsigned)(batch * nb)), dim3(BLK), 0, st, verts, trans, ld_trans, w, nverts, npoints, nb);
    STRAPS_CHECK_LAUNCH("scan_prep_kernel");
    const long long items_s = (long long)((npoints + QCHUNK - 1) / QCHUNK) * ((nverts + VTILE - 1) / VTILE);
    const long long items_m = (long long)((nverts + QCHUNK - 1) / QCHUNK) * ((npoints + PTILE - 1) / PTILE);
    if (opts->w_s2m != 0.f) {
        const int nwg = (int)(items_s < WPB ? items_s : WPB);
        hipLaunchKernelGGL(scan_search_kernel<true>, dim3((unsigned)(batch * nwg)), dim3(BLK), 0, st, w, points, nverts, npoints, nwg);
        STRAPS_CHECK_LAUNCH("scan_search_kernel<s2m>");
    }
    if (opts->w_m2s != 0.f) {
        const int nwg = (int)(items_m < WPB ? items_m : WPB);
        hipLaunchKernelGGL(scan_search_kernel<false>, dim3((unsigned)(batch * nwg)), dim3(BLK), 0, st, w, points, nverts, npoints, nwg);
        STRAPS_CHECK_LAUNCH("scan_search_kernel<m2s>");
    }
    hipLaunchKernelGGL(scan_point_kernel, dim3((unsigned)(batch * nbp)), dim3(BLK), 0, st, w, points, nverts, npoints, nbp, opts->sigma);
    STRAPS_CHECK_LAUNCH("scan_point_kernel");
    if (energy2 || dverts || dtrans || nearest_point) {
        hipLaunchKernelGGL(scan_gather_kernel, dim3((unsigned)(batch * nbv)), dim3(BLK), 0, st, w, points, dverts, nearest_point, nverts, npoints, nbv, opts->sigma,
                           opts->w_s2m, opts->w_m2s);
        STRAPS_CHECK_LAUNCH("scan_gather_kernel");
        if (energy2 || dtrans) {
            hipLaunchKernelGGL(scan_finish_kernel, dim3((unsigned)batch), dim3(BLK), 0, st, w, energy2, dtrans, nverts, nbv, nbp);
            STRAPS_CHECK_LAUNCH("scan_finish_kernel");
        }
    }
    return STRAPS_OK;
}
