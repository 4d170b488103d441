// smpl_bwd.hip -- gradient of the SMPL forward w.r.t. (betas, rotmats) given dL/dvertices, dL/djoints
// (what autograd does through smplx.lbs for pred_smpl_output, train/train_synthetic_otf_rendering.py:196-232).
//
//   smpl_verts_bwd_kernel : same tiling as the forward (32 bodies x vertex chunk per workgroup, one 32-vertex tile
//       per wave per round).  Per tile: (1) recompute v_posed with the K=218 MFMA contraction, (2) gather the vertex
//       gradient (dverts + sparse J-regressor / picked-vertex contributions of djoints) through an LDS-staged tile,
//       (3) per-vertex skinning backward on the VALU: g_vposed = T_R^T g; v_posed is staged next to g and, after a
//       barrier, dA_j += w_j * g (x) [v_posed;1] is accumulated BY JOINT OWNER: lane (body, h) of wave w owns joints
//       w + 4*(2i + h), i = 0..2, walks the round's (tile, vertex, weight) entries of those joints in a fixed order and
//       keeps the 3 x 12 sums in registers -- no atomics, bit-reproducible, (4) second MFMA contraction dF[b][k] += sum_{v,c} D[k][v][c] * g_vposed[b][v][c] with the transposed
//       blend fragments; per-chunk partials of dF and dA are written out.
//   smpl_pose_bwd_kernel  : lane = (body, joint): sums the chunk partials, back-propagates through rest-pose removal
//       and the kinematic chain (children -> parents by depth with wave shuffles), the joint regression and the pose
//       feature, and emits dbetas [B,10] and drotmats [B,24,3,3].  Its AA = true instantiation (straps_smpl_bwd_aa) also reads the axis-angle
//       pose the rotations were made from and writes d axis-angle [B,72] through the derivative of rodrigues.h (the one rodrigues_bwd_kernel uses):
//       the same bits as straps_smpl_bwd followed by straps_rodrigues_bwd, without the drotmats round trip.
#include "common.h"
#include "rodrigues.h"

namespace {

constexpr int KP = STRAPS_SMPL_KP, KG = KP / 8, NT = STRAPS_SMPL_TILES, NV = STRAPS_SMPL_V, NROUNDS = NT / 4;
constexpr int BT = 32, AS = 292, SS = 193;        // SS: stage row = 32 vertices x (g[3], v_posed[3]) + 1
constexpr int NJS = STRAPS_SMPL_NPICK + STRAPS_SMPL_NEXTRA;   // 66 joint-gradient sources (joints 24..89)
// look-ahead of smpl_verts_bwd_kernel: RD fragment groups (3 + 1 f32x4 per lane each) in phase 1, RT = 4 RD transposed fragments in phase 4;
// SKP skinning entries per vertex row are fetched ahead of phase 3 (SMPL has 4 weights per vertex; a wider model's further entries are read in phase 3);
// phase 3b reads its table entries EB at a time
constexpr int RD = 4, RT = 4 * RD, SKP = 4, EB = 8;
// chunk partials per batch of smpl_pose_bwd_kernel
constexpr int PU = 9;
static_assert(RD >= 1 && RT <= 84, "the rings are filled before their loops");

// workgroup barrier that orders the LDS traffic only.  __syncthreads() also waits for every global load of the wave (here: as a call, the kernel's
// target attribute keeps it from being inlined), which would end the look-ahead of the round loop at each of its four barriers
__device__ __forceinline__ STRAPS_NO_PACKED_FP32 void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__global__ __launch_bounds__(256, 1) STRAPS_NO_PACKED_FP32 void smpl_verts_bwd_kernel(straps_smpl_model_t m, const float* __restrict__ F,
                                                                const float* __restrict__ Amat, const float* __restrict__ dverts,
                                                                const float* __restrict__ djoints, float* __restrict__ dFp,
                                                                float* __restrict__ dAp, long long B, int rounds_per_chunk) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As_ = smem;                     // [32][AS]
    float* stage = As_ + BT * AS;          // [4][32][SS]   (the F rows are read straight from global / L1: 16 B per lane per step)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, bl = lane & 31;
    const int chunk = blockIdx.x;
    const long long b0 = (long long)blockIdx.y * BT;
    const int nb = (int)((B - b0) < BT ? (B - b0) : BT);

    for (int i = tid; i < BT * 72; i += 256) {
        const int b = i / 72, q = i % 72;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (b < nb) v = *reinterpret_cast<const f32x4*>(Amat + (b0 + b) * 288 + q * 4);
        *reinterpret_cast<f32x4*>(As_ + b * AS + q * 4) = v;
    }
    __syncthreads();

    const int round0 = chunk * rounds_per_chunk;
    const int round1 = min(round0 + rounds_per_chunk, NROUNDS);
    const f32x4* __restrict__ blend = reinterpret_cast<const f32x4*>(m.blend_frag);
    const f32x4* __restrict__ blend_t = reinterpret_cast<const f32x4*>(m.blend_frag_t);
    float* mystage = stage + wave * BT * SS;
    const int KW = m.skin_k;
    const bool vbody = bl < nb;

    float dacc[3][12];                     // dA of this lane's three joints
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 12; ++e) dacc[i][e] = 0.f;
    f32x16 accF[7];
#pragma unroll
    for (int f = 0; f < 7; ++f)
#pragma unroll
        for (int q = 0; q < 16; ++q) accF[f][q] = 0.f;

    for (int rd = round0; rd < round1; ++rd) {
        const int tile = rd * 4 + wave;
        // ---- loads of the round, issued ahead of their phases (a wave alone on its SIMD has nothing else to hide a round trip behind) ----
        // phase 1's ring: the first RD fragment groups and F steps
        const f32x4* px = blend + ((long long)(tile * 3 + 0) * KG) * 64 + lane;
        const f32x4* py = px + KG * 64;
        const f32x4* pz = py + KG * 64;
        int fo = (vbody ? bl : 0) * KP + 4 * h;
        asm volatile("" : "+v"(fo));         // (the F row is the same in every round: left alone, its 28 steps are hoisted out of the round loop and spilled)
        const float* frow = F + b0 * KP + fo;
        f32x4 rx[RD], ry[RD], rz[RD], rf[RD];
#pragma unroll
        for (int s = 0; s < RD; ++s) {
            if (s < KG) {
                rx[s] = px[s * 64]; ry[s] = py[s * 64]; rz[s] = pz[s * 64];
                rf[s] = *reinterpret_cast<const f32x4*>(frow + 8 * s);
            }
        }
        // phase 2's dL/dverts elements of this lane and the table ranges of phases 2 and 3b: none depends on phase 1, all land while its MFMAs run.
        // Element i = lane + 64 t of the [32 bodies][96] tile, t = 3 q + u: body 2 q + bu, column i0 - 96 bu; the bodies of the batch are
        // q < dvn[u] (0 without dverts or for a column past the last vertex).  Past them a lane reads its last element again, or F[0] if it has
        // none, and stages a zero: no branch around a load
        const int ncol = min(96, (NV - tile * 32) * 3);
        const float* dvp[3];
        int dvn[3], dvq[3], dvs[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int i0 = lane + 64 * u, bu = i0 >= 96, c = i0 - 96 * bu;
            dvn[u] = (dverts && c < ncol) ? (nb - bu + 1) / 2 : 0;
            dvp[u] = dvn[u] > 0 ? dverts + (b0 + bu) * (long long)(NV * 3) + tile * 96 + c : F;
            dvq[u] = dvn[u] > 0 ? 2 * NV * 3 : 0;
            dvs[u] = bu * SS + (c / 3) * 6 + (c % 3);
        }
        float dvr[48];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
#pragma unroll
            for (int u = 0; u < 3; ++u) dvr[3 * q + u] = dvp[u][min(q, max(dvn[u] - 1, 0)) * dvq[u]];
        }
        const int jr0 = m.jrt_ptr[tile], jr1 = m.jrt_ptr[tile + 1];
        int de0[3], de1[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int j = wave + 4 * (2 * i + h);
            de0[i] = m.dj_ptr[rd * 24 + j]; de1[i] = m.dj_ptr[rd * 24 + j + 1];
        }
        // ---- (1) recompute v_posed for this tile: group g's fragments were loaded RD groups ahead ----
        f32x16 ax, ay, az;
#pragma unroll
        for (int r = 0; r < 16; ++r) { ax[r] = 0.f; ay[r] = 0.f; az[r] = 0.f; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            const int s = g % RD;
            const f32x4 f0 = vbody ? rf[s] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ax = mfma32(rx[s][e], f0[e], ax);
                ay = mfma32(ry[s][e], f0[e], ay);
                az = mfma32(rz[s][e], f0[e], az);
            }
            if (g + RD < KG) {                     // refill the slot (the last RD groups load nothing: no read past the tile's fragments or the F row)
                rx[s] = px[(g + RD) * 64]; ry[s] = py[(g + RD) * 64]; rz[s] = pz[(g + RD) * 64];
                rf[s] = *reinterpret_cast<const f32x4*>(frow + 8 * (g + RD));
            }
            if (g == (RD < KG ? RD : KG) - 1) {    // phase 2's staging: the elements were requested before the refills, so the next group's wait covers them
#pragma unroll
                for (int t = 0; t < 48; ++t)
                    mystage[(t / 3) * 2 * SS + dvs[t % 3]] = t / 3 < dvn[t % 3] ? dvr[t] : 0.f;
            }
            __builtin_amdgcn_sched_barrier(0);     // (left alone, the scheduler sinks every refill to the MFMA that reads it: one round trip per group)
        }
        float skw[16][SKP];
        int skj[16][SKP];
#pragma unroll
        for (int k = 0; k < SKP; ++k) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int v = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int at = k < KW ? v * KW + k : 0;           // (an entry the model does not have: element 0, not used below)
                skw[r][k] = m.skin_w[at]; skj[r][k] = m.skin_j[at];
            }
        }
        // ---- (2) dL/dverts of this tile is staged (inside the loop above); add the joint-gradient contributions ----
        lds_barrier();
        if (djoints && h == 0 && vbody) {
            const float* dj = djoints + (b0 + bl) * (STRAPS_SMPL_NJOINTS_OUT * 3) + 72;   // joints 24..89
            for (int e = jr0; e < jr1; ++e) {
                const int code = m.jrt_code[e];
                const float w = m.jrt_w[e];
                float* sv = mystage + bl * SS + (code >> 8) * 6;
                const float* g = dj + (code & 255) * 3;
                sv[0] = fmaf(w, g[0], sv[0]); sv[1] = fmaf(w, g[1], sv[1]); sv[2] = fmaf(w, g[2], sv[2]);
            }
        }
        lds_barrier();
        // ---- (3) skinning backward per (body, vertex) ----
        {
            const float* Ab = As_ + bl * AS;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int vrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int v = tile * 32 + vrow;
                float* sv = mystage + bl * SS + vrow * 6;
                const float gx = sv[0], gy = sv[1], gz = sv[2];
                sv[3] = ax[r]; sv[4] = ay[r]; sv[5] = az[r];              // v_posed, for the joint owners below
                float t00 = 0.f, t01 = 0.f, t02 = 0.f, t10 = 0.f, t11 = 0.f, t12 = 0.f, t20 = 0.f, t21 = 0.f, t22 = 0.f;
#pragma unroll
                for (int k = 0; k < SKP; ++k) {
                    if (k < KW) {
                        const float w = skw[r][k];
                        const int jo = skj[r][k] * 12;
                        const f32x4 a0 = *reinterpret_cast<const f32x4*>(Ab + jo);
                        const f32x4 a1 = *reinterpret_cast<const f32x4*>(Ab + jo + 4);
                        const f32x4 a2 = *reinterpret_cast<const f32x4*>(Ab + jo + 8);
                        t00 += w * a0[0]; t01 += w * a0[1]; t02 += w * a0[2];
                        t10 += w * a1[0]; t11 += w * a1[1]; t12 += w * a1[2];
                        t20 += w * a2[0]; t21 += w * a2[1]; t22 += w * a2[2];
                    }
                }
                for (int k = SKP; k < KW; ++k) {                          // (a model with more than SKP weights per vertex: the rest as they come)
                    const float w = m.skin_w[v * KW + k];
                    const int jo = m.skin_j[v * KW + k] * 12;
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(Ab + jo);
                    const f32x4 a1 = *reinterpret_cast<const f32x4*>(Ab + jo + 4);
                    const f32x4 a2 = *reinterpret_cast<const f32x4*>(Ab + jo + 8);
                    t00 += w * a0[0]; t01 += w * a0[1]; t02 += w * a0[2];
                    t10 += w * a1[0]; t11 += w * a1[1]; t12 += w * a1[2];
                    t20 += w * a2[0]; t21 += w * a2[1]; t22 += w * a2[2];
                }
                // g_vposed = T_R^T g.  The fusion is written out: left as t00 * gx + t10 * gy + t20 * gz, WHICH product the compiler rounds on its own
                // changes with the code around the expression, and with it the last bits of dF.  This is the form of the kernel before the look-ahead
                // (its disassembly rounds t1c * gy alone in all 48 expressions); tools/smpl_bwd_latency_ab.py compares the bits with that library
                ax[r] = fmaf(t20, gz, fmaf(t00, gx, t10 * gy));
                ay[r] = fmaf(t21, gz, fmaf(t01, gx, t11 * gy));
                az[r] = fmaf(t22, gz, fmaf(t02, gx, t12 * gy));
            }
        }
        // phase 4's ring: its first RT transposed fragments are on their way while phase 3b walks the joint tables
        const f32x4* pt = blend_t + ((long long)tile * 3 * 7 * 4) * 64 + lane;
        f32x4 rt[RT];
#pragma unroll
        for (int s = 0; s < RT; ++s) rt[s] = pt[s * 64];
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();   // all four tiles of the round are staged (g and v_posed)
        // ---- (3b) dA_j += w * g (x) [v_posed; 1], by joint owner, entries in table order ----
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            for (int e = de0[i]; e < de1[i]; e += EB) {
                int code[EB];                                             // tile_in_round << 5 | vertex row
                float w[EB];
#pragma unroll
                for (int u = 0; u < EB; ++u) {                            // (past the joint's last entry: that entry again, not used)
                    const int at = min(e + u, de1[i] - 1);
                    code[u] = m.dj_code[at]; w[u] = m.dj_w[at];
                }
#pragma unroll
                for (int u = 0; u < EB; ++u) {
                    if (e + u < de1[i]) {
                        const float* sv = stage + ((code[u] >> 5) * BT + bl) * SS + (code[u] & 31) * 6;
                        const float wx = w[u] * sv[0], wy = w[u] * sv[1], wz = w[u] * sv[2];
                        const float x = sv[3], y = sv[4], z = sv[5];
                        dacc[i][0] = fmaf(wx, x, dacc[i][0]); dacc[i][1] = fmaf(wx, y, dacc[i][1]); dacc[i][2] = fmaf(wx, z, dacc[i][2]); dacc[i][3] += wx;
                        dacc[i][4] = fmaf(wy, x, dacc[i][4]); dacc[i][5] = fmaf(wy, y, dacc[i][5]); dacc[i][6] = fmaf(wy, z, dacc[i][6]); dacc[i][7] += wy;
                        dacc[i][8] = fmaf(wz, x, dacc[i][8]); dacc[i][9] = fmaf(wz, y, dacc[i][9]); dacc[i][10] = fmaf(wz, z, dacc[i][10]); dacc[i][11] += wz;
                    }
                }
            }
        }
        // ---- (4) dF^T[k][b] += sum_v D[k][v][c] * g_vposed[v][b][c]: fragment n = (c * 7 + f) * 4 + rq was loaded RT fragments ahead ----
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 84; ++n) {
            const int c = n / 28, f = (n / 4) % 7, rq = n % 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = c == 0 ? ax[rq * 4 + e] : (c == 1 ? ay[rq * 4 + e] : az[rq * 4 + e]);
                accF[f] = mfma32(rt[n % RT][e], g, accF[f]);
            }
            if (n + RT < 84) rt[n % RT] = pt[(n + RT) * 64];              // refill the slot (nothing past the tile's 84 fragments)
            __builtin_amdgcn_sched_barrier(0);
        }
        lds_barrier();
    }
    // ---- per-chunk partials ----
    // each wave holds dF sums over ITS tiles: fixed-order tree reduction over the 4 waves through the (now free)
    // F/A staging area: (0 += 2, 1 += 3) then (0 += 1)
    {
        __syncthreads();
        float* red = smem;                                   // 2 x 7168 floats fit in As_ + stage (34048 floats)
        if (wave >= 2) {
#pragma unroll
            for (int f = 0; f < 7; ++f)
#pragma unroll
                for (int q = 0; q < 16; ++q) red[(wave - 2) * 7168 + (f * 16 + q) * 64 + lane] = accF[f][q];
        }
        __syncthreads();
        if (wave < 2) {
#pragma unroll
            for (int f = 0; f < 7; ++f)
#pragma unroll
                for (int q = 0; q < 16; ++q) accF[f][q] += red[wave * 7168 + (f * 16 + q) * 64 + lane];
        }
        __syncthreads();
        if (wave == 1) {
#pragma unroll
            for (int f = 0; f < 7; ++f)
#pragma unroll
                for (int q = 0; q < 16; ++q) red[(f * 16 + q) * 64 + lane] = accF[f][q];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int f = 0; f < 7; ++f)
#pragma unroll
                for (int q = 0; q < 16; ++q) accF[f][q] += red[(f * 16 + q) * 64 + lane];
        }
    }
    if (vbody && wave == 0) {
        float* o = dFp + ((long long)chunk * B + b0 + bl) * KP;
#pragma unroll
        for (int f = 0; f < 7; ++f)
#pragma unroll
            for (int q = 0; q < 16; ++q) o[f * 32 + mfma_row(q, lane)] = accF[f][q];
    }
    if (vbody) {
        float* o = dAp + ((long long)chunk * B + b0 + bl) * 288;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int j = wave + 4 * (2 * i + h);
#pragma unroll
            for (int e = 0; e < 12; ++e) o[j * 12 + e] = dacc[i][e];
        }
    }
}

// ------------------------------------------------------------------------------------------
// smpl_pose_bwd_kernel is compiled WITHOUT packed fp32 instructions (common.h, STRAPS_NO_PACKED_FP32): round 5 traced its irreproducible results beside a
// bf16x3 convolution workgroup to ONE instruction the compiler had formed in it, v_pk_fma_f32 ... op_sel:[0,1,0].  The instrumented forms
// of the kernel that found it -- checked lane exchanges, value dumps, the instruction written out next to a plain v_fma_f32 -- were removed in round 6: the
// stand-alone reproducer tools/packed_fp32_hazard_repro.hip carries the finding, profiles/r05_packed_fp32_* the measurements, and the kernel below is the
// product's only form (the removal left its instruction stream alone: same opcode counts but for two integer instructions, registers renumbered --
// compared on the disassembly).
// (a lane exchange of the kernel below: ds_bpermute_b32, several in flight, waits placed by the compiler)
__device__ __forceinline__ float lane_get(float value, int src) { return __shfl(value, src, 64); }
// The chunk partials are read PU chunks at a time: every load of a batch is issued before the first add, the next batch (two register sets, taking
// turns) before the adds of this one; the adds stay one chunk after the other, as in a plain loop over the chunks.
__device__ __forceinline__ STRAPS_NO_PACKED_FP32 void pose_load_dA(float (&t)[PU][12], const float* p, long long stride) {
#pragma unroll
    for (int u = 0; u < PU; ++u)
#pragma unroll
        for (int e = 0; e < 12; ++e) t[u][e] = p[u * stride + e];
}
__device__ __forceinline__ STRAPS_NO_PACKED_FP32 void pose_add_dA(float (&gA)[12], const float (&t)[PU][12]) {
#pragma unroll
    for (int u = 0; u < PU; ++u)
#pragma unroll
        for (int e = 0; e < 12; ++e) gA[e] += t[u][e];
}
// (dF: nine pose-feature columns from fR on, and the shape column fB)
__device__ __forceinline__ STRAPS_NO_PACKED_FP32 void pose_load_dF(float (&t)[PU][10], const float* p, long long stride, int fR, int fB) {
#pragma unroll
    for (int u = 0; u < PU; ++u) {
#pragma unroll
        for (int e = 0; e < 9; ++e) t[u][e] = p[u * stride + fR + e];
        t[u][9] = p[u * stride + fB];
    }
}
__device__ __forceinline__ STRAPS_NO_PACKED_FP32 void pose_add_dF(float (&gR)[9], float& gbeta, const float (&t)[PU][10], bool rot, bool shape) {
#pragma unroll
    for (int u = 0; u < PU; ++u) {
        if (rot) {
#pragma unroll
            for (int e = 0; e < 9; ++e) gR[e] += t[u][e];
        }
        if (shape) gbeta += t[u][9];
    }
}
// (AA: compile-time flag of the fused axis-angle epilogue, no runtime branch added.  AA = false is straps_smpl_bwd's kernel: the same arithmetic, bit-identical
//  results; as a template instantiation the compiler unrolls the dbeta shuffle loop, same speed -- DESIGN, "Axis-angle gradients")
template <bool AA>
__global__ __launch_bounds__(256) STRAPS_NO_PACKED_FP32 void smpl_pose_bwd_kernel(straps_smpl_model_t m, const float* __restrict__ betas,
                                                            const float* __restrict__ rotmats, const float* __restrict__ dFp,
                                                            const float* __restrict__ dAp, const float* __restrict__ djoints,
                                                            float* __restrict__ dbetas, float* __restrict__ drot, long long B,
                                                            int chunks, const float* __restrict__ aa, float* __restrict__ daa) {
    const int lane = threadIdx.x & 63;
    const int j = lane & 31;
    const int base = lane & 32;
    const long long body = ((long long)blockIdx.x * 256 + threadIdx.x) >> 5;
    const bool vb = body < B;
    const bool vj = j < 24;
    const long long bb = vb ? body : 0;
    const int jj = vj ? j : 0;
    const bool act = vb && vj;

    float beta[10];
#pragma unroll
    for (int l = 0; l < 10; ++l) beta[l] = betas[bb * 10 + l];
    float R[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = rotmats[(bb * 24 + jj) * 9 + e];
    float J[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = m.j_template[jj * 3 + c];
#pragma unroll
        for (int l = 0; l < 10; ++l) s = fmaf(m.j_shapedirs[(jj * 3 + c) * 10 + l], beta[l], s);
        J[c] = s;
    }
    const int par = m.parents[jj];
    const int dep = vj ? m.depth[jj] : -1;
    const int src = base + (par < 0 ? 0 : par);
    float rel[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float jp = lane_get(J[c], src);
        rel[c] = (jj > 0) ? J[c] - jp : J[c];
    }
    // dA partials: the first batch is requested here, behind every load the forward chain needs -- the chain itself needs none of it and hides it.
    // A lane without a (body, joint) sums the partials of (0, 0) in the batches; nothing of such a lane reaches an output.
    const float* pA = dAp + (bb * 24 + jj) * 12;
    const long long sA = B * 288;
    const int nbat = chunks / PU;
    float tA[PU][12], tB[PU][12];
    if (nbat > 0) pose_load_dA(tA, pA, sA);
    // forward chain: G (own global transform) and P (parent's rotation), recomputed
    float G[12], PR[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[r * 4 + 0] = R[r * 3 + 0]; G[r * 4 + 1] = R[r * 3 + 1]; G[r * 4 + 2] = R[r * 3 + 2]; G[r * 4 + 3] = rel[r];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) PR[e] = (e == 0 || e == 4 || e == 8) ? 1.f : 0.f;
    for (int d = 1; d <= m.max_depth; ++d) {
        float P[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) P[e] = lane_get(G[e], src);
        if (dep == d) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float p0 = P[r * 4 + 0], p1 = P[r * 4 + 1], p2 = P[r * 4 + 2];
                PR[r * 3 + 0] = p0; PR[r * 3 + 1] = p1; PR[r * 3 + 2] = p2;
                G[r * 4 + 0] = p0 * R[0] + p1 * R[3] + p2 * R[6];
                G[r * 4 + 1] = p0 * R[1] + p1 * R[4] + p2 * R[7];
                G[r * 4 + 2] = p0 * R[2] + p1 * R[5] + p2 * R[8];
                G[r * 4 + 3] = p0 * rel[0] + p1 * rel[1] + p2 * rel[2] + P[r * 4 + 3];
            }
        }
    }
    // gradient arriving at A_j (sum of chunk partials) and at the posed joint
    float gA[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) gA[e] = 0.f;
#pragma unroll
    for (int b = 0; b < NROUNDS / PU; ++b) {             // (no launch has more than NROUNDS chunks: resolve_rpc)
        if (b < nbat) {
            const int bn = b + 1 < nbat ? b + 1 : b;     // (behind the last batch: that batch again, not used -- a branch around the loads would
            pose_load_dA(b & 1 ? tA : tB, pA + bn * PU * sA, sA);      //  make the compiler wait for them before the adds, at the join)
            pose_add_dA(gA, b & 1 ? tB : tA);
        }
    }
    if (act)
        for (int c = nbat * PU; c < chunks; ++c) {
            const float* p = pA + c * sA;
#pragma unroll
            for (int e = 0; e < 12; ++e) gA[e] += p[e];
        }
    float gGR[9], gGt[3], gJ[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float gat = gA[r * 4 + 3];
        gGR[r * 3 + 0] = gA[r * 4 + 0] - gat * J[0];
        gGR[r * 3 + 1] = gA[r * 4 + 1] - gat * J[1];
        gGR[r * 3 + 2] = gA[r * 4 + 2] - gat * J[2];
        gGt[r] = gat + ((vb && vj && djoints) ? djoints[(body * STRAPS_SMPL_NJOINTS_OUT + j) * 3 + r] : 0.f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) gJ[c] = -(G[0 * 4 + c] * gA[3] + G[1 * 4 + c] * gA[7] + G[2 * 4 + c] * gA[11]);

    int child[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) child[c] = m.children[jj * 3 + c];
    // dF partials (this lane's nine pose-feature columns and its shape column): the first batch travels during the walk over the tree below
    const float* pF = dFp + bb * KP;
    const long long sF = B * KP;
    const int fR = 11 + (j >= 1 && vj ? j - 1 : 0) * 9, fB = 1 + (j < 10 ? j : 0);
    float tF[PU][10], tG[PU][10];
    if (nbat > 0) pose_load_dF(tF, pF, sF, fR, fB);
    float gR[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) gR[e] = 0.f;
    for (int d = m.max_depth; d >= 1; --d) {
        // message of a depth-d joint to its parent: gP_R (9), gP_t (3), -grel (3)
        float M[15];
        const bool mine = (dep == d);
        float grel[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) grel[c] = PR[0 * 3 + c] * gGt[0] + PR[1 * 3 + c] * gGt[1] + PR[2 * 3 + c] * gGt[2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                M[r * 3 + c] = mine ? (gGR[r * 3 + 0] * R[c * 3 + 0] + gGR[r * 3 + 1] * R[c * 3 + 1] + gGR[r * 3 + 2] * R[c * 3 + 2] + gGt[r] * rel[c]) : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { M[9 + c] = mine ? gGt[c] : 0.f; M[12 + c] = mine ? -grel[c] : 0.f; }
        if (mine) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    gR[r * 3 + c] = PR[0 * 3 + r] * gGR[0 * 3 + c] + PR[1 * 3 + r] * gGR[1 * 3 + c] + PR[2 * 3 + r] * gGR[2 * 3 + c];
#pragma unroll
            for (int c = 0; c < 3; ++c) gJ[c] += grel[c];
        }
        // parents gather from their (up to 3) children
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            const int ch = child[cc];
            const int cs = base + (ch < 0 ? 0 : ch);
            float in[15];
#pragma unroll
            for (int e = 0; e < 15; ++e) in[e] = lane_get(M[e], cs);
            if (vj && ch >= 0) {       // in[] is zero unless that child is at depth d
#pragma unroll
                for (int e = 0; e < 9; ++e) gGR[e] += in[e];
#pragma unroll
                for (int c = 0; c < 3; ++c) { gGt[c] += in[9 + c]; gJ[c] += in[12 + c]; }
            }
        }
    }
    if (j == 0) {   // root: G = [R | J]
#pragma unroll
        for (int e = 0; e < 9; ++e) gR[e] = gGR[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) gJ[c] += gGt[c];
    }
    // pose-feature and direct beta gradients from dF (sum of chunk partials)
    float gbeta_direct = 0.f;
#pragma unroll
    for (int b = 0; b < NROUNDS / PU; ++b) {
        if (b < nbat) {
            const int bn = b + 1 < nbat ? b + 1 : b;
            pose_load_dF(b & 1 ? tF : tG, pF + bn * PU * sF, sF, fR, fB);
            pose_add_dF(gR, gbeta_direct, b & 1 ? tG : tF, j >= 1, j < 10);
        }
    }
    if (vb && vj) {
        for (int c = nbat * PU; c < chunks; ++c) {
            const float* p = dFp + ((long long)c * B + body) * KP;
            if (j >= 1) {
#pragma unroll
                for (int e = 0; e < 9; ++e) gR[e] += p[11 + (j - 1) * 9 + e];
            }
            if (j < 10) gbeta_direct += p[1 + j];
        }
        if (!AA || drot) {      // (straps_smpl_bwd_aa: drotmats may be NULL)
#pragma unroll
            for (int e = 0; e < 9; ++e) drot[(body * 24 + j) * 9 + e] = gR[e];
        }
        if constexpr (AA) {      // d axis-angle of this (body, joint): full_pose_aa / dfull_pose_aa [B][24][3]
            float ox, oy, oz;
            const float* r = aa + (body * 24 + j) * 3;
            straps_rodrigues_bwd_one(r[0], r[1], r[2], gR, ox, oy, oz);
            float* o = daa + (body * 24 + j) * 3;
            o[0] = ox; o[1] = oy; o[2] = oz;
        }
    }
    // dbeta[l] = dF[1+l] + sum_j sum_c Js[j][c][l] * gJ_j[c]
#pragma unroll
    for (int l = 0; l < 10; ++l) {
        float s = vj ? (m.j_shapedirs[(jj * 3 + 0) * 10 + l] * gJ[0] + m.j_shapedirs[(jj * 3 + 1) * 10 + l] * gJ[1] +
                        m.j_shapedirs[(jj * 3 + 2) * 10 + l] * gJ[2]) : 0.f;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float direct = lane_get(gbeta_direct, base + l);
        if (vb && j == l) dbetas[body * 10 + l] = s + direct;
    }
}

inline int resolve_rpc(long long batch, int chunks) {
    if (chunks <= 0) chunks = (batch >= 1024) ? 8 : 54;
    if (chunks > NROUNDS) chunks = NROUNDS;
    return (NROUNDS + chunks - 1) / chunks;
}

}  // namespace

// forward pose kernel is shared with smpl.hip (recomputes F and A for the backward)
int straps_smpl_launch_pose(const straps_smpl_model_t* model, const float* betas, const float* rotmats, float* F, float* Amat,
                            float* joints, long long batch, hipStream_t st);

extern "C" size_t straps_smpl_bwd_workspace_bytes(long long batch, int chunks) {
    const int rpc = resolve_rpc(batch, chunks);
    const int nch = (NROUNDS + rpc - 1) / rpc;
    return (size_t)batch * (size_t)(KP + 288 + nch * (KP + 288)) * sizeof(float);
}

namespace {
// both entry points: the vertex pass, then the pose pass (AA: with the axis-angle epilogue).  Arguments checked by the callers.
template <bool AA>
int smpl_bwd_launch(const straps_smpl_model_t* model, const float* betas, const float* rotmats, const float* aa, const float* dverts,
                    const float* djoints, float* dbetas, float* drotmats, float* daa, void* workspace, long long batch, int chunks,
                    void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int rpc = resolve_rpc(batch, chunks);
    const int nch = (NROUNDS + rpc - 1) / rpc;
    float* F = (float*)workspace;
    float* Amat = F + batch * KP;
    float* dFp = Amat + batch * 288;
    float* dAp = dFp + (long long)nch * batch * KP;
    int rc = straps_smpl_launch_pose(model, betas, rotmats, F, Amat, nullptr, batch, st);
    if (rc != STRAPS_OK) return rc;
    const size_t lds = (size_t)(BT * AS + 4 * BT * SS) * sizeof(float);
    STRAPS_RAISE_LDS((smpl_verts_bwd_kernel), lds, "smpl_verts_bwd_kernel");
    const long long btiles = (batch + BT - 1) / BT;
    if (btiles > 65535) { straps_set_error("straps_smpl_bwd: batch %lld exceeds one launch; split it", batch); return STRAPS_EUNSUPPORTED; }
    hipLaunchKernelGGL(smpl_verts_bwd_kernel, dim3(nch, (unsigned)btiles), dim3(256), lds, st, *model, F, Amat, dverts, djoints, dFp, dAp, batch, rpc);
    STRAPS_CHECK_LAUNCH("smpl_verts_bwd_kernel");
    // (Round 5, DESIGN section 1: this kernel was the one whose results differed between two processes on one GPU.  Cause: a packed fp32 instruction with a
    //  low-half operand select the compiler had formed in it -- the kernel is compiled without packed fp32 instructions, STRAPS_NO_PACKED_FP32.)
    hipLaunchKernelGGL(smpl_pose_bwd_kernel<AA>, dim3((unsigned)((batch * 32 + 255) / 256)), dim3(256), 0, st, *model, betas, rotmats, dFp, dAp,
                       djoints, dbetas, drotmats, batch, nch, aa, daa);
    STRAPS_CHECK_LAUNCH("smpl_pose_bwd_kernel");
    return STRAPS_OK;
}
}  // namespace

extern "C" int straps_smpl_bwd(const straps_smpl_model_t* model, const float* betas, const float* rotmats, const float* dverts,
                               const float* djoints, float* dbetas, float* drotmats, void* workspace, long long batch, int chunks,
                               void* stream) {
    STRAPS_REQUIRE(model && betas && rotmats && dbetas && drotmats && workspace, "straps_smpl_bwd: null pointer");
    STRAPS_REQUIRE(model->blend_frag_t && model->children && model->jrt_ptr && model->dj_ptr && model->dj_code && model->dj_w,
                   "straps_smpl_bwd: model lacks the backward tables");
    STRAPS_REQUIRE(batch > 0, "straps_smpl_bwd: batch must be positive");
    return smpl_bwd_launch<false>(model, betas, rotmats, nullptr, dverts, djoints, dbetas, drotmats, nullptr, workspace, batch, chunks, stream);
}

extern "C" int straps_smpl_bwd_aa(const straps_smpl_model_t* model, const float* betas, const float* rotmats, const float* full_pose_aa,
                                  const float* dverts, const float* djoints, float* dbetas, float* dfull_pose_aa, float* drotmats,
                                  void* workspace, long long batch, int chunks, void* stream) {
    STRAPS_REQUIRE(model && betas && rotmats && full_pose_aa && dbetas && dfull_pose_aa && workspace, "straps_smpl_bwd_aa: null pointer");
    STRAPS_REQUIRE(model->blend_frag_t && model->children && model->jrt_ptr && model->dj_ptr && model->dj_code && model->dj_w,
                   "straps_smpl_bwd_aa: model lacks the backward tables");
    STRAPS_REQUIRE(batch > 0, "straps_smpl_bwd_aa: batch must be positive");
    return smpl_bwd_launch<true>(model, betas, rotmats, full_pose_aa, dverts, djoints, dbetas, drotmats, dfull_pose_aa, workspace, batch, chunks,
                                 stream);
}
