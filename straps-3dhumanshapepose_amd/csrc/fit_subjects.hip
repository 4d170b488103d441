// fit_subjects.hip -- one body shape per subject across frames: straps_fit_adam_subjects, straps_subject_mean_rows
// (include/straps_hip.h states the semantics).
//
// straps_fit_adam_subjects is straps_fit_adam (csrc/silfit.hip) with the ten shape coefficients tied across the frames of a subject: the update
// step of a fit loop composed of entry points, one launch, no workspace.
//   fit_adam_subjects_kernel  one 1024-thread workgroup per subject, its sixteen waves stride over the subject's frames (frame j of the
//                             subject belongs to wave j % 16, so the order of every sum depends on the subject's frame count and mask alone).
//     pass 1   per frame E_f (every lane) and the ten shape terms t_f (lanes 0..9); a wave adds its counting frames in frame order, starting
//              FROM its first term, not from +0 (a -0 stays a -0); the loads of four frames are issued before the first is consumed (a
//              subject of 256 frames is four such rounds per wave and pass).
//              Everything another wave overwrites in pass 2 -- the held energy, the shape of the first row, the shape moments -- is read here.
//     barrier  one; every thread reaches it (no thread leaves before it, idle waves included).  Wave partials are added in wave order.
//     pass 2   best iterate, gradient, the per-frame Adam of columns 0..146 (fit_adam_kernel's, bit for bit) and the subject's shape step,
//              which every wave computes alike and writes into its own frames' rows; four frames in flight as well.
// straps_subject_mean_rows: the same reduction on `cols` columns of arbitrary rows, divided by the count.
#include "common.h"

namespace {

constexpr int NE = 157;
constexpr int NSHAPE = 10;
constexpr int SHAPE0 = 147;               // first shape column of a row
constexpr int SUBJ_WAVES = 16;             // a 1024-thread workgroup: four waves per SIMD, 128 VGPRs each
constexpr int SUBJ_THREADS = SUBJ_WAVES * 64;
constexpr int FIF = 4;                    // frames whose loads a wave has in flight

__device__ __forceinline__ double ipow(double b, int t) {      // as csrc/fit.hip
    double r = 1.0;
    for (int n = 0; n < 32 && t > 0; ++n) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(SUBJ_THREADS) STRAPS_NO_PACKED_FP32 void fit_adam_subjects_kernel(
        straps_fit_opts_t o, float* __restrict__ est, const int32_t* __restrict__ offsets, const uint8_t* __restrict__ frame_mask,
        const float* __restrict__ g_kp, const float* __restrict__ dcam, const float* __restrict__ dx6, const float* __restrict__ dbetas,
        const float* __restrict__ e_kp, const float* __restrict__ energy2, float w_in, float w_out, float* __restrict__ exp_avg,
        float* __restrict__ exp_avg_sq, float* __restrict__ shape_avg, float* __restrict__ shape_avg_sq, float* __restrict__ energy, long long ld_energy,
        long long col, float* __restrict__ subject_energy, long long ld_subject, float* __restrict__ grad, float* __restrict__ best_est,
        float* __restrict__ best_energy, int step, int first, int update, long long B) {
    __shared__ float part[SUBJ_WAVES][NSHAPE + 2];      // per wave: the ten shape sums, the energy sum
    __shared__ int part_have[SUBJ_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long s = blockIdx.x;
    const long long lo = clampll(offsets[s], 0, B), hi = clampll(offsets[s + 1], lo, B), nf = hi - lo;
    // the shape column this lane holds in pass 2 (element lane + 128 of a row: lanes 19..28), and what pass 2 overwrites of it
    const int sc = lane + 128 - SHAPE0;
    const bool shape_lane = sc >= 0 && sc < NSHAPE;
    const int scc = shape_lane ? sc : 0;
    const float held = (best_energy && !first && nf > 0) ? best_energy[s] : 0.f;
    float shape0 = 0.f, sm = 0.f, sv = 0.f;
    if (nf > 0 && shape_lane) {
        shape0 = est[lo * NE + SHAPE0 + scc];
        if (update) { sm = shape_avg[s * NSHAPE + scc]; sv = shape_avg_sq[s * NSHAPE + scc]; }
    }
    // ---- pass 1: E_f and the shape terms of this wave's frames
    const int tl = lane < NSHAPE ? lane : 0;
    float acc_t = 0.f, acc_e = 0.f;
    bool have = false;
    for (long long j0 = wv; j0 < nf; j0 += SUBJ_WAVES * FIF) {
        float E[FIF], t[FIF];
        bool in[FIF], cnt[FIF];
#pragma unroll
        for (int u = 0; u < FIF; ++u) {
            const long long j = j0 + (long long)u * SUBJ_WAVES;
            in[u] = j < nf;
            const long long f = lo + (in[u] ? j : j0);      // (a slot past the subject's end reads a frame of the subject again and is dropped)
            cnt[u] = in[u] && (frame_mask ? frame_mask[f] != 0 : true);
            E[u] = e_kp ? e_kp[f] : 0.f;
            if (energy2) E[u] = fmaf(w_out, energy2[f * 2 + 1], fmaf(w_in, energy2[f * 2], E[u]));
            const float db = dbetas ? dbetas[f * NSHAPE + tl] : 0.f;
            t[u] = g_kp ? (dbetas ? g_kp[f * NE + SHAPE0 + tl] + db : g_kp[f * NE + SHAPE0 + tl]) : db;
        }
#pragma unroll
        for (int u = 0; u < FIF; ++u) {
            if (in[u] && lane == 0 && energy) energy[(lo + j0 + (long long)u * SUBJ_WAVES) * ld_energy + col] = E[u];
            if (cnt[u]) {      // only real terms are added: the first one starts the sum
                acc_e = have ? acc_e + E[u] : E[u];
                acc_t = have ? acc_t + t[u] : t[u];
                have = true;
            }
        }
    }
    if (lane < NSHAPE) part[wv][lane] = acc_t;
    if (lane == NSHAPE) part[wv][NSHAPE] = acc_e;
    if (lane == 0) part_have[wv] = have ? 1 : 0;
    __syncthreads();      // the only barrier: every thread of the workgroup is here
    float gs = 0.f, Es = 0.f;
    bool counted = false;
#pragma unroll
    for (int w = 0; w < SUBJ_WAVES; ++w) {
        if (part_have[w]) {
            gs = counted ? gs + part[w][scc] : part[w][scc];
            Es = counted ? Es + part[w][NSHAPE] : part[w][NSHAPE];
            counted = true;
        }
    }
    const bool better = nf > 0 && (first || Es < held);      // the first minimum wins; a NaN never replaces what is held
    if (threadIdx.x == 0) {
        if (subject_energy) subject_energy[s * ld_subject + col] = Es;
        if (best_energy && better) best_energy[s] = Es;
    }
    // ---- pass 2
    const int t_ = step + 1;
    const double bc1 = 1.0 - ipow((double)o.beta1, t_);
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - ipow((double)o.beta2, t_)));
    const float ss_cam = (float)((double)o.lr_cam / bc1), ss_pose = (float)((double)o.lr_pose / bc1), ss_shape = (float)((double)o.lr_shape / bc1);
    // the subject's shape step: every wave computes the same bits; a subject without a counting frame keeps shape and moments as they are
    const bool shape_step = update && counted;
    float shape1 = shape0;
    if (shape_step && shape_lane) {
#pragma clang fp contract(off)
        const float gm = (1.f - o.beta1) * gs, gv = (1.f - o.beta2) * gs;
        const float gv2 = gs * gv;
        const float mi = fmaf(o.beta1, sm, gm);
        const float vi = fmaf(o.beta2, sv, gv2);
        const float num = mi * ss_shape;
        shape1 = shape0 - num / fmaf(sqrtf(vi), inv_sqrt_bc2, o.eps);
        if (wv == 0) {
            shape_avg[s * NSHAPE + scc] = mi;
            shape_avg_sq[s * NSHAPE + scc] = vi;
        }
    }
    for (long long j0 = wv; j0 < nf; j0 += SUBJ_WAVES * FIF) {
        float e[FIF][3], g[FIF][3], mo[FIF][3], vo[FIF][3];
        bool in[FIF];
#pragma unroll
        for (int u = 0; u < FIF; ++u) {
            const long long j = j0 + (long long)u * SUBJ_WAVES;
            in[u] = j < nf;
            const long long f = lo + (in[u] ? j : j0);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int idx = lane + 64 * q;
                const int i = idx < NE ? idx : 0;
                e[u][q] = est[f * NE + i];
                if (i < SHAPE0) {
                    float a = 0.f;
                    bool got = false;
                    if (i < 3) { if (dcam) { a = dcam[f * 3 + i]; got = true; } }
                    else if (dx6) { a = dx6[f * 144 + i - 3]; got = true; }
                    g[u][q] = g_kp ? (got ? g_kp[f * NE + i] + a : g_kp[f * NE + i]) : a;
                    mo[u][q] = update ? exp_avg[f * NE + i] : 0.f;
                    vo[u][q] = update ? exp_avg_sq[f * NE + i] : 0.f;
                } else {
                    g[u][q] = gs;
                    mo[u][q] = vo[u][q] = 0.f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < FIF; ++u) {
            if (!in[u]) continue;
            const long long f = lo + j0 + (long long)u * SUBJ_WAVES;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int idx = lane + 64 * q;
                if (idx >= NE) continue;
                const long long a = f * NE + idx;
                if (grad) grad[a] = g[u][q];
                if (best_est && better) best_est[a] = e[u][q];
                if (!update) continue;
                if (idx >= SHAPE0) {
                    if (shape_step) est[a] = shape1;
                    continue;
                }
                const float step_size = idx < 3 ? ss_cam : ss_pose;
                // fit_adam_kernel's update, written out in the same way
                {
#pragma clang fp contract(off)
                const float gm = (1.f - o.beta1) * g[u][q], gv = (1.f - o.beta2) * g[u][q];
                const float gv2 = g[u][q] * gv;
                const float mi = fmaf(o.beta1, mo[u][q], gm);
                const float vi = fmaf(o.beta2, vo[u][q], gv2);
                const float num = mi * step_size;
                exp_avg[a] = mi;
                exp_avg_sq[a] = vi;
                est[a] = e[u][q] - num / fmaf(sqrtf(vi), inv_sqrt_bc2, o.eps);
                }
            }
        }
    }
}

__global__ __launch_bounds__(SUBJ_THREADS) STRAPS_NO_PACKED_FP32 void subject_mean_rows_kernel(
        const float* __restrict__ rows, long long ld, int cols, const int32_t* __restrict__ offsets, const uint8_t* __restrict__ frame_mask,
        float* __restrict__ out, long long B) {
    __shared__ float part[2][SUBJ_WAVES][64];      // [counting rows | all rows]
    __shared__ int part_n[2][SUBJ_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long s = blockIdx.x;
    const long long lo = clampll(offsets[s], 0, B), hi = clampll(offsets[s + 1], lo, B), nf = hi - lo;
    const int c = lane < cols ? lane : 0;
    float acc_c = 0.f, acc_a = 0.f;
    int n_c = 0, n_a = 0;
    for (long long j0 = wv; j0 < nf; j0 += SUBJ_WAVES * FIF) {
        float v[FIF];
        bool in[FIF], cnt[FIF];
#pragma unroll
        for (int u = 0; u < FIF; ++u) {
            const long long j = j0 + (long long)u * SUBJ_WAVES;
            in[u] = j < nf;
            const long long f = lo + (in[u] ? j : j0);
            cnt[u] = in[u] && (frame_mask ? frame_mask[f] != 0 : true);
            v[u] = rows[f * ld + c];
        }
#pragma unroll
        for (int u = 0; u < FIF; ++u) {
            if (in[u]) { acc_a = n_a ? acc_a + v[u] : v[u]; ++n_a; }
            if (cnt[u]) { acc_c = n_c ? acc_c + v[u] : v[u]; ++n_c; }
        }
    }
    part[0][wv][lane] = acc_c;
    part[1][wv][lane] = acc_a;
    if (lane == 0) { part_n[0][wv] = n_c; part_n[1][wv] = n_a; }
    __syncthreads();
    if (wv != 0 || lane >= cols) return;      // (after the only barrier)
    int total_c = 0;
#pragma unroll
    for (int w = 0; w < SUBJ_WAVES; ++w) total_c += part_n[0][w];
    const int k = total_c > 0 ? 0 : 1;        // no counting row: the plain mean over all rows
    float sum = 0.f;
    int n = 0;
#pragma unroll
    for (int w = 0; w < SUBJ_WAVES; ++w) {
        if (part_n[k][w]) {
            sum = n ? sum + part[k][w][lane] : part[k][w][lane];
            n += part_n[k][w];
        }
    }
    out[s * cols + lane] = n ? sum / (float)n : 0.f;
}

}  // namespace

extern "C" int straps_fit_adam_subjects(const straps_fit_opts_t* opts, float* est, const int32_t* offsets, const uint8_t* frame_mask, const float* g_kp,
                                        const float* dcam, const float* dx6, const float* dbetas, const float* e_kp, const float* energy2, float w_in,
                                        float w_out, float* exp_avg, float* exp_avg_sq, float* shape_avg, float* shape_avg_sq, float* energy,
                                        long long ld_energy, long long col, float* subject_energy, long long ld_subject, float* grad, float* best_est,
                                        float* best_energy, int step, int first, int update, long long batch, long long n_subjects, void* stream) {
    STRAPS_REQUIRE(opts, "straps_fit_adam_subjects: null opts");
    STRAPS_REQUIRE(est, "straps_fit_adam_subjects: null est");
    STRAPS_REQUIRE(offsets, "straps_fit_adam_subjects: null offsets");
    STRAPS_REQUIRE(batch > 0 && batch <= (1LL << 31) - 4, "straps_fit_adam_subjects: batch must be in 1..2^31-4 (got %lld)", batch);
    STRAPS_REQUIRE(n_subjects >= 1 && n_subjects <= batch, "straps_fit_adam_subjects: n_subjects must be in 1..batch (got %lld of %lld)", n_subjects, batch);
    STRAPS_REQUIRE(step >= 0 && step <= (1 << 30), "straps_fit_adam_subjects: step must be in 0..2^30 (got %d)", step);
    STRAPS_REQUIRE((best_est == nullptr) == (best_energy == nullptr), "straps_fit_adam_subjects: best_est and best_energy must be given together");
    STRAPS_REQUIRE(!update || (exp_avg && exp_avg_sq), "straps_fit_adam_subjects: update needs exp_avg and exp_avg_sq");
    STRAPS_REQUIRE(!update || (shape_avg && shape_avg_sq), "straps_fit_adam_subjects: update needs shape_avg and shape_avg_sq");
    STRAPS_REQUIRE(!energy || (ld_energy >= 1 && col >= 0 && col < ld_energy), "straps_fit_adam_subjects: col must be in 0..ld_energy-1 (got %lld of %lld)", col,
                   ld_energy);
    STRAPS_REQUIRE(!subject_energy || (ld_subject >= 1 && col >= 0 && col < ld_subject),
                   "straps_fit_adam_subjects: col must be in 0..ld_subject-1 (got %lld of %lld)", col, ld_subject);
    STRAPS_REQUIRE(opts->beta1 >= 0.f && opts->beta1 < 1.f && opts->beta2 >= 0.f && opts->beta2 < 1.f && opts->eps > 0.f,
                   "straps_fit_adam_subjects: eps must be positive, beta1 and beta2 in [0, 1)");
    hipLaunchKernelGGL(fit_adam_subjects_kernel, dim3((unsigned)n_subjects), dim3(SUBJ_THREADS), 0, (hipStream_t)stream, *opts, est, offsets, frame_mask, g_kp,
                       dcam, dx6, dbetas, e_kp, energy2, w_in, w_out, exp_avg, exp_avg_sq, shape_avg, shape_avg_sq, energy, ld_energy, col, subject_energy,
                       ld_subject, grad, best_est, best_energy, step, first, update, batch);
    STRAPS_CHECK_LAUNCH("fit_adam_subjects_kernel");
    return STRAPS_OK;
}

extern "C" int straps_subject_mean_rows(const float* rows, long long ld, int cols, const int32_t* offsets, const uint8_t* frame_mask, float* out,
                                        long long batch, long long n_subjects, void* stream) {
    STRAPS_REQUIRE(rows, "straps_subject_mean_rows: null rows");
    STRAPS_REQUIRE(out, "straps_subject_mean_rows: null out");
    STRAPS_REQUIRE(offsets, "straps_subject_mean_rows: null offsets");
    STRAPS_REQUIRE(cols >= 1 && cols <= 64, "straps_subject_mean_rows: cols must be in 1..64 (got %d)", cols);
    STRAPS_REQUIRE(ld >= cols, "straps_subject_mean_rows: ld must be at least cols (got %lld for %d)", ld, cols);
    STRAPS_REQUIRE(batch > 0 && batch <= (1LL << 31) - 4, "straps_subject_mean_rows: batch must be in 1..2^31-4 (got %lld)", batch);
    STRAPS_REQUIRE(n_subjects >= 1 && n_subjects <= batch, "straps_subject_mean_rows: n_subjects must be in 1..batch (got %lld of %lld)", n_subjects, batch);
    hipLaunchKernelGGL(subject_mean_rows_kernel, dim3((unsigned)n_subjects), dim3(SUBJ_THREADS), 0, (hipStream_t)stream, rows, ld, cols, offsets, frame_mask, out,
                       batch);
    STRAPS_CHECK_LAUNCH("subject_mean_rows_kernel");
    return STRAPS_OK;
}
