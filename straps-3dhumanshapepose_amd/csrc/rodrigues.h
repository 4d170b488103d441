// rodrigues.h -- gradient of one axis-angle -> rotation matrix conversion (straps_rodrigues_fwd, pose.hip), shared by
// rodrigues_bwd_kernel (pose.hip) and the fused axis-angle epilogue of smpl_pose_bwd_kernel (smpl_bwd.hip): the two give the same bits.
#pragma once
#include "common.h"

// The forward evaluates smplx's batch_rodrigues, and this is the exact derivative of THAT formula (what autograd gives through it),
// not the textbook derivative of the exponential map:
//   e = r + eps (eps = 1e-8 in every component),  theta = |e|,  d = r / theta,  K = skew(d),  R = I + sin(theta) K + (1 - cos(theta)) K^2
// With G = dL/dR (row-major 3x3), term by term:
//   gK     = sin G + (1 - cos) (G K^T + K^T G)                         (d<G, K K>/dK = G K^T + K^T G; K^T = -K)
//   gtheta = cos <G, K> + sin <G, K^2>                                   (d sin = cos, d (1 - cos) = sin)
//   gd     = (gK21 - gK12, gK02 - gK20, gK10 - gK01)                     (K01 = -d_z, K02 = d_y, K10 = d_z, K12 = -d_x, K20 = -d_y, K21 = d_x)
//   dr     = gd / theta + (gtheta - <gd, r> / theta^2) e / theta        (d d_i / d r_j = delta_ij / theta - r_i e_j / theta^3, d theta / d r = e / theta)
// A zero row (r = 0): theta = sqrt(3) 1e-8 (a normal fp32 number), d = K = 0, gtheta = 0 and dr = vee(sin(theta) G) / theta ~ vee(G): finite, and
// what autograd of the formula gives.  theta is computed exactly as the forward kernel computes it.  Accuracy: within 1e-5 of max |dr| of float64
// autograd over zero, tiny (1e-7 .. 1e-3), moderate, near-pi and 3 pi angles (tests/test_gpu_pose_grad.py).
// Contraction is off and every fused multiply-add is written out: the result does not depend on the code the function is inlined into.
__device__ __forceinline__ STRAPS_NO_PACKED_FP32 void straps_rodrigues_bwd_one(float rx, float ry, float rz, const float (&g)[9],
                                                                               float& dx_out, float& dy_out, float& dz_out) {
#pragma clang fp contract(off)
    const float ex = rx + 1e-8f, ey = ry + 1e-8f, ez = rz + 1e-8f;
    const float theta = sqrtf(ex * ex + ey * ey + ez * ez);
    const float dx = rx / theta, dy = ry / theta, dz = rz / theta;
    // 1 - cos as 2 sin^2(theta / 2): the same function without the cancellation of 1.0f - cosf(theta), whose absolute error (~6e-8) the
    // gd / theta term would amplify to ~1e-5 of |dr| around theta = 1e-3
    const float s = sinf(theta), c = cosf(theta), h = sinf(0.5f * theta), c1 = 2.0f * (h * h);
    float K[9];
    K[0] = 0.f; K[1] = -dz; K[2] = dy;
    K[3] = dz;  K[4] = 0.f; K[5] = -dx;
    K[6] = -dy; K[7] = dx;  K[8] = 0.f;
    // K^2 with the forward's products (only its inner product with G is needed)
    float GK = 0.f, GK2 = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float q = fmaf(K[a * 3 + 0], K[0 * 3 + b], fmaf(K[a * 3 + 1], K[1 * 3 + b], K[a * 3 + 2] * K[2 * 3 + b]));
            GK = fmaf(g[a * 3 + b], K[a * 3 + b], GK);
            GK2 = fmaf(g[a * 3 + b], q, GK2);
        }
    const float gtheta = fmaf(c, GK, s * GK2);
    // gK_ab = s G_ab + c1 M_ab,  M = G K^T + K^T G:  M_ab = sum_k G_ak K_bk + K_ka G_kb
    float gK[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            float m = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) m = fmaf(g[a * 3 + k], K[b * 3 + k], fmaf(K[k * 3 + a], g[k * 3 + b], m));
            gK[a * 3 + b] = fmaf(s, g[a * 3 + b], c1 * m);
        }
    const float gdx = gK[7] - gK[5], gdy = gK[2] - gK[6], gdz = gK[3] - gK[1];
    const float gdr = fmaf(gdx, rx, fmaf(gdy, ry, gdz * rz));
    const float w = (gtheta - gdr / (theta * theta)) / theta;
    dx_out = fmaf(w, ex, gdx / theta);
    dy_out = fmaf(w, ey, gdy / theta);
    dz_out = fmaf(w, ez, gdz / theta);
}
