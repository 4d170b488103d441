// eval.hip -- silhouette of a mesh under the weak-perspective camera the regressor predicts: the predicted mask that
// metrics/eval_metrics_tracker.py:158-178 compares with the labelled one (silhouette IoU).  The reference renders it with the
// third-party `neural_renderer`; here it is the coverage half of csrc/raster.hip without a z-buffer.
//
// Byte-bound and latency-bound work, no MFMA.  Three launches per call:
//   1. fill kernel     : mask = 0 (straps_fill_bytes: a kernel, not a memset node).
//   2. project kernel  : one thread per (body, vertex): u = s * (x + tx), v = s * (y + ty) -- the order of
//                        utils/cam_utils.py:21-22 and of cam_utils.orthographic_project_torch -- into the workspace [B][nverts][2].
//   3. face kernel     : 16 lanes per (body, face) share the pixel-centre samples inside the face's clipped, conservative bounding box;
//                        two-sided, edge-inclusive inside test (all three edge functions >= 0, or all three <= 0); a covered sample gets a
//                        plain byte store of 1.  Every writer of a byte writes the same value, so the mask does not depend on any order.
// Pixel convention: mask[b][r][c] samples ((2c + 1 - wh) / wh, (2r + 1 - wh) / wh); rows run with +v, no flip -- the pixel grid of
// undo_keypoint_normalisation (utils/joints2d_utils.py:5-10), so the mask lines up with Predictor's `vertices2D`.
// Every arithmetic step is written unfused (fp contract off) in the order tests/eval_cases.py::wp_silhouette uses, so the masks agree
// bit for bit.
#include "common.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) STRAPS_NO_PACKED_FP32 void wp_project_kernel(const float* __restrict__ verts, const float* __restrict__ cam,
                                                                              float* __restrict__ uv, long long n, int nverts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long b = i / nverts;
    const float s = cam[b * 3 + 0], tx = cam[b * 3 + 1], ty = cam[b * 3 + 2];
    const float x = verts[i * 3 + 0], y = verts[i * 3 + 1];
    uv[i * 2 + 0] = s * (x + tx);
    uv[i * 2 + 1] = s * (y + ty);
}

__device__ __forceinline__ float edge_fn(float ax, float ay, float bx, float by, float px, float py) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

constexpr int WP_LANES = 16;      // lanes per face, as raster_face_kernel (a face of the 13 776-face mesh at 256 x 256 has a box of four to nine samples)

__global__ __launch_bounds__(256) STRAPS_NO_PACKED_FP32 void wp_face_kernel(const float* __restrict__ uv, const int32_t* __restrict__ faces,
                                                                           uint8_t* __restrict__ mask, long long n, int nverts, int nfaces, int wh) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long i = gid / WP_LANES;                   // (body, face)
    const int sub = (int)(gid & (WP_LANES - 1));          // lane within the face's group
    if (i >= n) return;
    const long long b = i / nfaces;
    const int f = (int)(i - b * nfaces);
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)nverts || (unsigned)i1 >= (unsigned)nverts || (unsigned)i2 >= (unsigned)nverts) return;
    const float* p0 = uv + (b * nverts + i0) * 2;
    const float* p1 = uv + (b * nverts + i1) * 2;
    const float* p2 = uv + (b * nverts + i2) * 2;
    const float x0 = p0[0], y0 = p0[1];
    const float x1 = p1[0], y1 = p1[1];
    const float x2 = p2[0], y2 = p2[1];
    const float area = edge_fn(x0, y0, x1, y1, x2, y2);
    if (!(fabsf(area) > 1e-12f)) return;                       // degenerate (or NaN) face
    // pixel-centre sample k sits at (2k + 1 - wh) / wh; conservative bounding box of sample indices, clipped to the image
    const float fw = (float)wh;
    const float xmin = fminf(x0, fminf(x1, x2)), xmax = fmaxf(x0, fmaxf(x1, x2));
    const float ymin = fminf(y0, fminf(y1, y2)), ymax = fmaxf(y0, fmaxf(y1, y2));
    if (!(xmax >= -1.f && xmin <= 1.f && ymax >= -1.f && ymin <= 1.f)) return;
    int xa = (int)floorf((fmaxf(xmin, -1.f) * fw + fw - 1.f) * 0.5f), xb = (int)ceilf((fminf(xmax, 1.f) * fw + fw - 1.f) * 0.5f);
    int ya = (int)floorf((fmaxf(ymin, -1.f) * fw + fw - 1.f) * 0.5f), yb = (int)ceilf((fminf(ymax, 1.f) * fw + fw - 1.f) * 0.5f);
    xa = xa < 0 ? 0 : xa; ya = ya < 0 ? 0 : ya;
    xb = xb > wh - 1 ? wh - 1 : xb; yb = yb > wh - 1 ? wh - 1 : yb;
    if (xb < xa || yb < ya) return;
    uint8_t* mb = mask + b * (long long)wh * wh;
    const int bw = xb - xa + 1;
    // the group's lanes take the box samples round-robin in row-major order: 0 <= xa <= xi <= xb < wh and 0 <= ya <= yi <= yb < wh at every store
    int xi = xa + sub, yi = ya;
    while (xi > xb) { xi -= bw; ++yi; }
    while (yi <= yb) {
        const float yp = (float)(2 * yi + 1 - wh) / fw;
        const float xp = (float)(2 * xi + 1 - wh) / fw;
        const float e0 = edge_fn(x1, y1, x2, y2, xp, yp);
        const float e1 = edge_fn(x2, y2, x0, y0, xp, yp);
        const float e2 = edge_fn(x0, y0, x1, y1, xp, yp);
        if ((e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f)) mb[(long long)yi * wh + xi] = 1;
        xi += WP_LANES;
        while (xi > xb) { xi -= bw; ++yi; }
    }
}

}  // namespace

int straps_fill_bytes(void* ptr, size_t bytes, unsigned char value, hipStream_t st);      // csrc/augment.hip

extern "C" size_t straps_wp_silhouette_workspace_bytes(long long batch, int nverts) {
    if (batch <= 0 || nverts <= 0) return 0;
    return (size_t)batch * (size_t)nverts * 2 * sizeof(float);
}

extern "C" int straps_wp_silhouette(const float* verts, const int32_t* faces, const float* cam_wp, uint8_t* mask, void* workspace, long long batch,
                                    int nverts, int nfaces, int wh, void* stream) {
    STRAPS_REQUIRE(verts, "straps_wp_silhouette: `verts` is a null pointer");
    STRAPS_REQUIRE(faces, "straps_wp_silhouette: `faces` is a null pointer");
    STRAPS_REQUIRE(cam_wp, "straps_wp_silhouette: `cam_wp` is a null pointer");
    STRAPS_REQUIRE(mask, "straps_wp_silhouette: `mask` is a null pointer");
    STRAPS_REQUIRE(workspace, "straps_wp_silhouette: `workspace` is a null pointer");
    STRAPS_REQUIRE(((uintptr_t)workspace & 3) == 0, "straps_wp_silhouette: `workspace` must be 4-byte aligned");
    STRAPS_REQUIRE(batch > 0 && nverts > 0 && nfaces > 0, "straps_wp_silhouette: `batch`, `nverts` and `nfaces` must be positive (got %lld, %d, %d)", batch,
                   nverts, nfaces);
    STRAPS_REQUIRE(nfaces <= 0x7fffffff / 3, "straps_wp_silhouette: `nfaces` must be at most 715827882 (got %d)", nfaces);      // faces[f * 3 + k] in int
    STRAPS_REQUIRE(wh >= 1 && wh <= 4096, "straps_wp_silhouette: `wh` must be in 1..4096 (got %d)", wh);
    const long long nv = batch * nverts, nf = batch * nfaces;
    STRAPS_REQUIRE((nv + 255) / 256 < (1LL << 31) && (nf * WP_LANES + 255) / 256 < (1LL << 31) && (batch * (long long)wh * wh + 255) / 256 < (1LL << 31),
                   "straps_wp_silhouette: `batch` too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    float* uv = (float*)workspace;
    {
        const int rc = straps_fill_bytes(mask, (size_t)batch * wh * wh, 0, st);
        if (rc != STRAPS_OK) return rc;
    }
    hipLaunchKernelGGL(wp_project_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, verts, cam_wp, uv, nv, nverts);
    STRAPS_CHECK_LAUNCH("wp_project_kernel");
    hipLaunchKernelGGL(wp_face_kernel, dim3((unsigned)((nf * WP_LANES + 255) / 256)), dim3(256), 0, st, uv, faces, mask, nf, nverts, nfaces, wh);
    STRAPS_CHECK_LAUNCH("wp_face_kernel");
    return STRAPS_OK;
}
