// val.hip -- the forward-only head of a validation step (train/train_synthetic_otf_rendering.py:313-348 +
// metrics/train_loss_and_metrics_tracker.py:118-213): prediction heads, the five task losses of losses/multi_task_loss.py (reduction
// 'mean') and the tracker's eleven metric sums of a batch, no gradient, added to a device-resident accumulator.
//
// val_points_kernel, grid (B, 3): one workgroup per (sample, point set) -- vertices, reposed vertices, the 14 H36M-LSP joints read through
// the index map out of the 90-joint array.  The mathematics of point_metrics_kernel (csrc/metrics.hip), copied: pass 1 the fp64 moment
// sums, one thread solves the Procrustes problem, pass 2 the three error sums -- and, from the same differences, the sum of squared
// errors that the 'verts' / 'joints3D' MSE needs: the points are read once for the loss and the metrics together.  Four doubles per
// workgroup go to the workspace.
// val_finalize_kernel, one workgroup: a thread per sample does the 2-D / shape / pose heads in fp64 and rounds the sample's eleven
// metric sums to fp32 (per_sample); then one thread per column adds the samples in ascending order, and thread 0 forms the MSEs, applies
// the log-variances, writes batch_out and adds to the accumulator -- one double addition per slot.  No atomics: nothing depends on
// scheduling, and a sample's row depends on nothing but that sample.
#include <math.h>

#include "common.h"

namespace {

// COCO / H36M-LSP joint selections out of the 90-joint superset (reference config.py:27-32)
__constant__ int c_val_coco[17] = {24, 26, 25, 28, 27, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8};
__constant__ int c_val_h36m14[14] = {73 + 6, 73 + 5, 73 + 4, 73 + 1, 73 + 2, 73 + 3, 73 + 16, 73 + 15, 73 + 14, 73 + 11, 73 + 12, 73 + 13, 73 + 8, 73 + 10};

constexpr int PT_D = 4;       // doubles per (sample, point set): the three error sums, the sum of squared errors
constexpr int HD_D = 4;       // doubles per sample from the heads: joints2D squared error over the visible joints, their number, shape and rotation squared error
constexpr int ROW = 11;       // metric sums per sample (metrics.BatchMetrics.KEYS)
constexpr int WS_D = 3 * PT_D + HD_D;      // doubles per sample in the workspace; ROW floats per sample follow the doubles of all samples

__device__ void val_jacobi_eig3(double A[3][3], double V[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        if (off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

__device__ __forceinline__ double val_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// blockIdx.y: 0 = vertices (P0, T0, nverts points), 1 = reposed vertices (P1, T1; both null: four zeros), 2 = the 14 joints c_val_h36m14 of
// J [B][90][3] against T2 [B][14][3]
__global__ __launch_bounds__(256) void val_points_kernel(const float* __restrict__ P0, const float* __restrict__ T0, const float* __restrict__ P1,
                                                         const float* __restrict__ T1, const float* __restrict__ J, const float* __restrict__ T2,
                                                         double* __restrict__ ws, int nverts) {
    __shared__ double red[4][17];
    __shared__ double sol[20];          // mu1[3] mu2[3] R[9] scale t[3] sc_ratio
    const int b = blockIdx.x, set = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* o = ws + (long long)b * WS_D + set * PT_D;      // (a sample's WS_D doubles: three point sets, then the heads' four)
    const bool mapped = set == 2;
    const int N = mapped ? 14 : nverts;
    const float* P = set == 0 ? P0 : set == 1 ? P1 : J;
    const float* T = set == 0 ? T0 : set == 1 ? T1 : T2;
    if (!P) {                           // (the whole workgroup: no reposed vertices)
        if (tid < PT_D) o[tid] = 0.0;
        return;
    }
    const float* p0 = P + (long long)b * (mapped ? 270 : (long long)N * 3);
    const float* t0 = T + (long long)b * N * 3;
    double a[17];
#pragma unroll
    for (int i = 0; i < 17; ++i) a[i] = 0.0;
    for (int n = tid; n < N; n += 256) {
        const float* pp = p0 + (mapped ? c_val_h36m14[n] : n) * 3;
        const double x[3] = {pp[0], pp[1], pp[2]};
        const double y[3] = {t0[n * 3], t0[n * 3 + 1], t0[n * 3 + 2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a[i] += x[i];
            a[3 + i] += y[i];
            a[6] += x[i] * x[i];
            a[7] += y[i] * y[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) a[8 + i * 3 + j] += x[i] * y[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 17; ++i) {
        const double s = val_wave_sum(a[i]);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double s[17];
        for (int i = 0; i < 17; ++i) s[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
        const double n = (double)N;
        double mu1[3], mu2[3], K[3][3];
        for (int i = 0; i < 3; ++i) { mu1[i] = s[i] / n; mu2[i] = s[3 + i] / n; }
        const double var1 = s[6] - n * (mu1[0] * mu1[0] + mu1[1] * mu1[1] + mu1[2] * mu1[2]);
        const double var2 = s[7] - n * (mu2[0] * mu2[0] + mu2[1] * mu2[1] + mu2[2] * mu2[2]);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) K[i][j] = s[8 + i * 3 + j] - n * mu1[i] * mu2[j];
        // K = U S V^T  ->  K^T K = V S^2 V^T
        double A[3][3], V[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) A[i][j] = K[0][i] * K[0][j] + K[1][i] * K[1][j] + K[2][i] * K[2][j];
        val_jacobi_eig3(A, V);
        int o0 = 0, o1 = 1, o2 = 2;   // order eigenvalues descending
        if (A[o0][o0] < A[o1][o1]) { int t = o0; o0 = o1; o1 = t; }
        if (A[o0][o0] < A[o2][o2]) { int t = o0; o0 = o2; o2 = t; }
        if (A[o1][o1] < A[o2][o2]) { int t = o1; o1 = o2; o2 = t; }
        double v1[3] = {V[0][o0], V[1][o0], V[2][o0]}, v2[3] = {V[0][o1], V[1][o1], V[2][o1]};
        double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
        double u1[3], u2[3];
        for (int i = 0; i < 3; ++i) {
            u1[i] = K[i][0] * v1[0] + K[i][1] * v1[1] + K[i][2] * v1[2];
            u2[i] = K[i][0] * v2[0] + K[i][1] * v2[1] + K[i][2] * v2[2];
        }
        double l1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
        for (int i = 0; i < 3; ++i) u1[i] /= (l1 > 0 ? l1 : 1.0);
        const double d12 = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
        for (int i = 0; i < 3; ++i) u2[i] -= d12 * u1[i];
        double l2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
        for (int i = 0; i < 3; ++i) u2[i] /= (l2 > 0 ? l2 : 1.0);
        const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
        // R = V' U'^T with U' = [u1 u2 u1xu2], V' = [v1 v2 v1xv2]  (== V Z U^T of utils/eval_utils.py:38-42)
        double R[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] = v1[i] * u1[j] + v2[i] * u2[j] + v3[i] * u3[j];
        double trRK = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) trRK += R[i][j] * K[j][i];
        const double scale = trRK / var1;
        for (int i = 0; i < 3; ++i) {
            sol[i] = mu1[i];
            sol[3 + i] = mu2[i];
            sol[16 + i] = mu2[i] - scale * (R[i][0] * mu1[0] + R[i][1] * mu1[1] + R[i][2] * mu1[2]);
            for (int j = 0; j < 3; ++j) sol[6 + i * 3 + j] = R[i][j];
        }
        sol[15] = scale;
        sol[19] = sqrt(var2 / n) / sqrt(var1 / n);       // T_scale / P_scale  (utils/eval_utils.py:75-83)
    }
    __syncthreads();
    double e0 = 0.0, e1 = 0.0, e2 = 0.0, sq = 0.0;
    const double sc = sol[19], s = sol[15];
    for (int n = tid; n < N; n += 256) {
        const float* pp = p0 + (mapped ? c_val_h36m14[n] : n) * 3;
        const double x[3] = {pp[0], pp[1], pp[2]};
        const double y[3] = {t0[n * 3], t0[n * 3 + 1], t0[n * 3 + 2]};
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double r0 = x[i] - y[i];
            const double q1 = (x[i] - sol[i]) * sc + sol[3 + i];
            const double q2 = s * (sol[6 + i * 3] * x[0] + sol[7 + i * 3] * x[1] + sol[8 + i * 3] * x[2]) + sol[16 + i];
            const double r1 = q1 - y[i];
            const double r2 = q2 - y[i];
            d0 += r0 * r0; d1 += r1 * r1; d2 += r2 * r2;
        }
        e0 += sqrt(d0); e1 += sqrt(d1); e2 += sqrt(d2);
        sq += d0;
    }
    e0 = val_wave_sum(e0); e1 = val_wave_sum(e1); e2 = val_wave_sum(e2); sq = val_wave_sum(sq);
    __syncthreads();
    if (lane == 0) { red[wave][0] = e0; red[wave][1] = e1; red[wave][2] = e2; red[wave][3] = sq; }
    __syncthreads();
    if (tid < PT_D) o[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

__device__ __forceinline__ bool val_joint_visible(float x, float y, float wh) { return !(x > wh || y > wh || x < 0.f || y < 0.f); }

// wsd [B][WS_D] doubles: the point sums of val_points_kernel, then this kernel's head sums; wsf [B][ROW] floats: the rounded rows (what
// per_sample receives when it is given).  Neither is `restrict`: both are written and read back across a barrier.
__global__ __launch_bounds__(256) void val_finalize_kernel(const float* __restrict__ joints, const float* __restrict__ est, int ld_est,
                                                           const float* __restrict__ prot, const float* __restrict__ tj2d,
                                                           const float* __restrict__ tshape, const float* __restrict__ trot,
                                                           const float* __restrict__ log_vars, double* wsd, float* wsf,
                                                           float* __restrict__ batch_out, float* __restrict__ per_sample, double* __restrict__ acc,
                                                           long long B, int nverts, float whf) {
    __shared__ double tot[ROW + 6];
    const int tid = threadIdx.x;
    const double wh = (double)whf;
    for (long long b = tid; b < B; b += 256) {
        const float* Jb = joints + b * 270;
        const float* e = est + b * ld_est;
        const double s = e[0], tx = e[1], ty = e[2];
        double sq2 = 0.0, nvis = 0.0, l2 = 0.0, sqs = 0.0, sqr = 0.0;
        for (int k = 0; k < 17; ++k) {
            const float lxf = tj2d[(b * 17 + k) * 2 + 0], lyf = tj2d[(b * 17 + k) * 2 + 1];
            const double lx = lxf, ly = lyf;
            const float* pj = Jb + c_val_coco[k] * 3;
            const double u = s * ((double)pj[0] + tx), v = s * ((double)pj[1] + ty);      // orthographic projection (utils/cam_utils.py:21-22)
            if (val_joint_visible(lxf, lyf, whf)) {
                const double du = u - ((2.0 * lx) / wh - 1.0), dv = v - ((2.0 * ly) / wh - 1.0);
                sq2 += du * du + dv * dv;
                nvis += 1.0;
            }
            const double px = (u + 1.0) * (wh / 2.0) - lx, py = (v + 1.0) * (wh / 2.0) - ly;      // undo_keypoint_normalisation (utils/joints2d_utils.py:5-10)
            l2 += sqrt(px * px + py * py);
        }
        for (int l = 0; l < 10; ++l) { const double d = (double)e[147 + l] - (double)tshape[b * 10 + l]; sqs += d * d; }
        for (int q = 0; q < 216; ++q) { const double d = (double)prot[b * 216 + q] - (double)trot[b * 216 + q]; sqr += d * d; }
        double* w = wsd + b * WS_D;
        w[3 * PT_D + 0] = sq2; w[3 * PT_D + 1] = nvis; w[3 * PT_D + 2] = sqs; w[3 * PT_D + 3] = sqr;
        const float row[ROW] = {(float)w[0], (float)w[1], (float)w[2], (float)w[PT_D], (float)w[PT_D + 1], (float)w[2 * PT_D], (float)w[2 * PT_D + 1],
                                (float)w[2 * PT_D + 2], (float)sqs, (float)sqr, (float)l2};
#pragma unroll
        for (int k = 0; k < ROW; ++k) {
            wsf[b * ROW + k] = row[k];
            if (per_sample) per_sample[b * ROW + k] = row[k];
        }
    }
    __syncthreads();
    // the samples in ascending order, one thread per column: ROW metric columns (the rounded rows), six loss sums (doubles)
    if (tid < ROW) {
        double t = 0.0;
        for (long long b = 0; b < B; ++b) t += (double)wsf[b * ROW + tid];
        tot[tid] = t;
    } else if (tid >= 64 && tid < 70) {
        // sum of squares of: vertices, visible 2-D joints; their number; sum of squares of: 3-D joints, shape, rotations
        const int q = tid - 64;
        const int off = q == 0 ? 3 : q == 1 ? 3 * PT_D : q == 2 ? 3 * PT_D + 1 : q == 3 ? 2 * PT_D + 3 : q == 4 ? 3 * PT_D + 2 : 3 * PT_D + 3;
        double t = 0.0;
        for (long long b = 0; b < B; ++b) t += wsd[b * WS_D + off];
        tot[ROW + q] = t;
    }
    __syncthreads();
    if (tid == 0) {
        const double nvis = tot[ROW + 2];
        // element counts of the 'mean' reductions: verts B*nverts*3, joints2D nvis*2, joints3D B*14*3, shape B*10, pose B*216
        const double cnt[5] = {(double)B * (double)nverts * 3.0, nvis * 2.0, (double)B * 42.0, (double)B * 10.0, (double)B * 216.0};
        const double sq[5] = {tot[ROW + 0], tot[ROW + 1], tot[ROW + 3], tot[ROW + 4], tot[ROW + 5]};
        float out[12];
        double total = 0.0;
        for (int k = 0; k < 5; ++k) {
            const double mse = sq[k] / cnt[k];            // 0/0 = NaN for no visible joint, like nn.MSELoss on an empty tensor
            const double lv = (double)log_vars[k];
            const double w = exp(-lv);
            out[1 + k] = (float)(mse * w);
            out[6 + k] = (float)mse;
            total += mse * w + lv;
        }
        out[0] = (float)total;
        out[11] = (float)nvis;
        if (batch_out)
            for (int k = 0; k < 12; ++k) batch_out[k] = out[k];
        if (acc) {
            for (int k = 0; k < 11; ++k) acc[k] += (double)B * (double)out[k];      // loss.item() * num_inputs of the tracker (:119-124)
            acc[11] += (double)out[11];
            for (int k = 0; k < ROW; ++k) acc[12 + k] += tot[k];
            acc[23] += (double)B;
        }
    }
}

}  // namespace

extern "C" size_t straps_val_head_workspace_bytes(long long batch) {
    return batch > 0 ? (size_t)batch * (WS_D * sizeof(double) + ROW * sizeof(float)) : 0;
}

extern "C" int straps_val_head(const float* pred_verts, const float* pred_reposed, const float* pred_joints, const float* est, int ld_est,
                               const float* pred_rot, const float* tgt_verts, const float* tgt_reposed, const float* tgt_joints2d,
                               const float* tgt_joints3d, const float* tgt_shape, const float* tgt_rot, const float* log_vars, float* batch_out,
                               float* per_sample, double* acc, void* workspace, long long batch, int nverts, int img_wh, void* stream) {
    STRAPS_REQUIRE(pred_verts, "straps_val_head: `pred_verts` is a null pointer");
    STRAPS_REQUIRE(pred_joints, "straps_val_head: `pred_joints` is a null pointer");
    STRAPS_REQUIRE(est, "straps_val_head: `est` is a null pointer");
    STRAPS_REQUIRE(pred_rot, "straps_val_head: `pred_rot` is a null pointer");
    STRAPS_REQUIRE(tgt_verts, "straps_val_head: `tgt_verts` is a null pointer");
    STRAPS_REQUIRE(tgt_joints2d, "straps_val_head: `tgt_joints2d` is a null pointer");
    STRAPS_REQUIRE(tgt_joints3d, "straps_val_head: `tgt_joints3d` is a null pointer");
    STRAPS_REQUIRE(tgt_shape, "straps_val_head: `tgt_shape` is a null pointer");
    STRAPS_REQUIRE(tgt_rot, "straps_val_head: `tgt_rot` is a null pointer");
    STRAPS_REQUIRE(log_vars, "straps_val_head: `log_vars` is a null pointer");
    STRAPS_REQUIRE((pred_reposed == nullptr) == (tgt_reposed == nullptr),
                   "straps_val_head: `pred_reposed` and `tgt_reposed` must both be given or both be null pointers (got %s only)",
                   pred_reposed ? "pred_reposed" : "tgt_reposed");
    STRAPS_REQUIRE(batch_out || per_sample || acc, "straps_val_head: `batch_out`, `per_sample` and `acc` are all null pointers: nothing to compute");
    STRAPS_REQUIRE(workspace, "straps_val_head: `workspace` is a null pointer");
    STRAPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "straps_val_head: `workspace` must be 8-byte aligned");
    STRAPS_REQUIRE(!acc || ((uintptr_t)acc & 7) == 0, "straps_val_head: `acc` must be 8-byte aligned");
    STRAPS_REQUIRE(batch > 0 && batch < (1LL << 31), "straps_val_head: `batch` must be in 1..2^31-1 (got %lld)", batch);
    STRAPS_REQUIRE(nverts >= 3 && nverts <= 0x7fffffff / 3, "straps_val_head: `nverts` must be in 3..715827882 (got %d)", nverts);
    STRAPS_REQUIRE(ld_est >= 157, "straps_val_head: `ld_est` must be at least 157 (got %d)", ld_est);
    STRAPS_REQUIRE(img_wh > 0, "straps_val_head: `img_wh` must be positive (got %d)", img_wh);
    hipStream_t st = (hipStream_t)stream;
    double* wsd = (double*)workspace;
    float* wsf = (float*)(wsd + batch * WS_D);
    hipLaunchKernelGGL(val_points_kernel, dim3((unsigned)batch, 3), dim3(256), 0, st, pred_verts, tgt_verts, pred_reposed, tgt_reposed, pred_joints,
                       tgt_joints3d, wsd, nverts);
    STRAPS_CHECK_LAUNCH("val_points_kernel");
    hipLaunchKernelGGL(val_finalize_kernel, dim3(1), dim3(256), 0, st, pred_joints, est, ld_est, pred_rot, tgt_joints2d, tgt_shape, tgt_rot, log_vars,
                       wsd, wsf, batch_out, per_sample, acc, batch, nverts, (float)img_wh);
    STRAPS_CHECK_LAUNCH("val_finalize_kernel");
    return STRAPS_OK;
}
