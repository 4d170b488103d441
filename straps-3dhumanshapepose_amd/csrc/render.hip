// render.hip -- shaded picture of a mesh under the weak-perspective camera the regressor predicts: what predict/predict_3D.py:169-178
// draws with renderers/weak_perspective_pyrender_renderer.py (pyrender + trimesh + OpenGL there).  Geometry is csrc/eval.hip's coverage
// test with csrc/raster.hip's deterministic z-buffer and an orthographic depth; shading is Lambert with an ambient term (NOT pyrender's
// metallic-roughness material: pixel parity with the reference's pictures is not claimed, which face a pixel shows is pinned).
//
// Byte-bound and latency-bound work, no MFMA.  Five launches per call, all on the caller's stream, no synchronisation, no allocation:
//   1. fill kernel     : z-buffer = all bytes 0xFF, the empty key (straps_fill_bytes: a kernel, not a memset node).
//   2. vertex kernel   : one thread per (body, vertex): p' = R p (optional row-major rotation, one matrix or one per body; none: no
//                        multiply at all), u = s * (x' + tx), v = s * (y' + ty) -- wp_project_kernel's expressions -- into the workspace.
//   3. normal kernel   : one thread per (body, vertex): sum of the un-normalised face normals cross(p1' - p0', p2' - p0') of the incident
//                        faces in the order of the host's CSR vertex-to-face table (by vertex, then ascending face id).  A gather: no
//                        floating-point atomics, the sum is reproducible bit for bit.
//   4. face kernel     : wp_face_kernel's 16 lanes per (body, face), box, samples, two-sided edge-inclusive inside test and degenerate
//                        skip; per covered sample w_k = e_k / area, z = (w0 z0' + w1 z1') + w2 z2', a monotone unsigned key of z (the mesh
//                        straddles z = 0: sign bit flipped for non-negative floats, all bits for negative ones), 64-bit atomicMin of
//                        (key << 32 | face id).  Nearer = smaller z'; ties go to the lower face id; no dependence on the visiting order.
//   5. resolve kernel  : one thread per pixel.  Empty: background pixel (image or constant colour), mask 0, depth +inf, face id -1.
//                        Covered: the winning face's barycentric weights again (same expressions), interpolated vertex normal normalised
//                        once ((0,0,-1) when its squared length is below 1e-24 or NaN), flipped iff the winning face's own geometric
//                        normal has positive z' (a per-face decision), c = colour * min(1, ambient + sum_l intensity_l * max(0, n . d_l)),
//                        byte = floor(255 * clamp(c, 0, 1) + 0.5).
// Pixel convention: csrc/eval.hip's -- pixel (r, c) samples ((2c + 1 - wh) / wh, (2r + 1 - wh) / wh), rows run with +v, no flip.
// Every arithmetic step is written unfused (fp contract off) in the order tests/render_cases.py repeats in numpy float32, so face ids,
// mask and depth agree bit for bit; colours are held to one level of a float64 restatement.
#include "common.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) STRAPS_NO_PACKED_FP32 void render_vertex_kernel(const float* __restrict__ verts, const float* __restrict__ cam, int ld_cam,
                                                                                 const float* __restrict__ rot, int rot_per_body, float* __restrict__ pt,
                                                                                 float* __restrict__ uv, long long n, int nverts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long b = i / nverts;
    const float s = cam[b * ld_cam + 0], tx = cam[b * ld_cam + 1], ty = cam[b * ld_cam + 2];
    float x = verts[i * 3 + 0], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
    if (rot) {
        const float* R = rot + (rot_per_body ? b * 9 : 0);
        const float xr = (R[0] * x + R[1] * y) + R[2] * z;
        const float yr = (R[3] * x + R[4] * y) + R[5] * z;
        const float zr = (R[6] * x + R[7] * y) + R[8] * z;
        x = xr; y = yr; z = zr;
    }
    pt[i * 3 + 0] = x;
    pt[i * 3 + 1] = y;
    pt[i * 3 + 2] = z;
    uv[i * 2 + 0] = s * (x + tx);
    uv[i * 2 + 1] = s * (y + ty);
}

__global__ __launch_bounds__(256) STRAPS_NO_PACKED_FP32 void render_normal_kernel(const float* __restrict__ pt, const int32_t* __restrict__ faces,
                                                                                 const int32_t* __restrict__ vf_offsets, const int32_t* __restrict__ vf_faces,
                                                                                 float* __restrict__ nrm, long long n, int nverts, int nfaces) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long b = i / nverts;
    const int v = (int)(i - b * nverts);
    const float* pb = pt + b * nverts * 3;
    // the table holds at most one entry per face corner: 0 <= k0 <= k < k1 <= 3 nfaces whatever the table says
    int k0 = vf_offsets[v], k1 = vf_offsets[v + 1];
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > 3 * nfaces ? 3 * nfaces : k1;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int k = k0; k < k1; ++k) {
        const int f = vf_faces[k];
        if ((unsigned)f >= (unsigned)nfaces) continue;
        const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        if ((unsigned)i0 >= (unsigned)nverts || (unsigned)i1 >= (unsigned)nverts || (unsigned)i2 >= (unsigned)nverts) continue;
        const float* p0 = pb + (long long)i0 * 3;
        const float* p1 = pb + (long long)i1 * 3;
        const float* p2 = pb + (long long)i2 * 3;
        const float ax1 = p1[0] - p0[0], ay1 = p1[1] - p0[1], az1 = p1[2] - p0[2];
        const float ax2 = p2[0] - p0[0], ay2 = p2[1] - p0[1], az2 = p2[2] - p0[2];
        ax = ax + (ay1 * az2 - az1 * ay2);
        ay = ay + (az1 * ax2 - ax1 * az2);
        az = az + (ax1 * ay2 - ay1 * ax2);
    }
    nrm[i * 3 + 0] = ax;
    nrm[i * 3 + 1] = ay;
    nrm[i * 3 + 2] = az;
}

__device__ __forceinline__ float edge_fn(float ax, float ay, float bx, float by, float px, float py) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// monotone unsigned key of a float: smaller float <=> smaller key (the sign bit flipped for non-negative values, all bits for negative ones)
__device__ __forceinline__ unsigned depth_key(float z) {
    const unsigned u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_depth(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

constexpr int RD_LANES = 16;      // lanes per face, as wp_face_kernel

__global__ __launch_bounds__(256) STRAPS_NO_PACKED_FP32 void render_face_kernel(const float* __restrict__ uv, const float* __restrict__ pt,
                                                                               const int32_t* __restrict__ faces, unsigned long long* __restrict__ zbuf,
                                                                               long long n, int nverts, int nfaces, int wh) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long i = gid / RD_LANES;                   // (body, face)
    const int sub = (int)(gid & (RD_LANES - 1));          // lane within the face's group
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
    const float z0 = pt[(b * nverts + i0) * 3 + 2], z1 = pt[(b * nverts + i1) * 3 + 2], z2 = pt[(b * nverts + i2) * 3 + 2];
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
    unsigned long long* zb = zbuf + b * (long long)wh * wh;
    const int bw = xb - xa + 1;
    // the group's lanes take the box samples round-robin in row-major order: 0 <= xa <= xi <= xb < wh and 0 <= ya <= yi <= yb < wh at every atomic
    int xi = xa + sub, yi = ya;
    while (xi > xb) { xi -= bw; ++yi; }
    while (yi <= yb) {
        const float yp = (float)(2 * yi + 1 - wh) / fw;
        const float xp = (float)(2 * xi + 1 - wh) / fw;
        const float e0 = edge_fn(x1, y1, x2, y2, xp, yp);
        const float e1 = edge_fn(x2, y2, x0, y0, xp, yp);
        const float e2 = edge_fn(x0, y0, x1, y1, xp, yp);
        if ((e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f)) {
            const float w0 = e0 / area, w1 = e1 / area, w2 = e2 / area;
            const float z = (w0 * z0 + w1 * z1) + w2 * z2;
            const unsigned long long key = ((unsigned long long)depth_key(z) << 32) | (unsigned)f;
            atomicMin(zb + (long long)yi * wh + xi, key);
        }
        xi += RD_LANES;
        while (xi > xb) { xi -= bw; ++yi; }
    }
}

__device__ __forceinline__ uint8_t quantise(float c) { return (uint8_t)floorf(255.f * fminf(fmaxf(c, 0.f), 1.f) + 0.5f); }

__global__ __launch_bounds__(256) STRAPS_NO_PACKED_FP32 void render_resolve_kernel(const unsigned long long* __restrict__ zbuf, const float* __restrict__ uv,
                                                                                  const float* __restrict__ pt, const float* __restrict__ nrm,
                                                                                  const int32_t* __restrict__ faces, straps_render_opts_t o,
                                                                                  const uint8_t* __restrict__ bg, uint8_t* __restrict__ rgb,
                                                                                  uint8_t* __restrict__ mask, float* __restrict__ depth,
                                                                                  int32_t* __restrict__ face_ids, long long n, int nverts, int wh) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = zbuf[i];
    if (key == ~0ULL) {
        for (int k = 0; k < 3; ++k) rgb[i * 3 + k] = bg ? bg[i * 3 + k] : quantise(o.background[k]);
        if (mask) mask[i] = 0;
        if (depth) depth[i] = __uint_as_float(0x7f800000u);
        if (face_ids) face_ids[i] = -1;
        return;
    }
    const long long npix = (long long)wh * wh;
    const long long b = i / npix;
    const int rem = (int)(i - b * npix);
    const int yi = rem / wh, xi = rem - yi * wh;
    const int f = (int)(unsigned)(key & 0xffffffffULL);      // a key's face passed render_face_kernel's index checks: 0 <= f < nfaces, 0 <= i_k < nverts
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    const long long v0 = b * nverts + i0, v1 = b * nverts + i1, v2 = b * nverts + i2;
    const float x0 = uv[v0 * 2], y0 = uv[v0 * 2 + 1];
    const float x1 = uv[v1 * 2], y1 = uv[v1 * 2 + 1];
    const float x2 = uv[v2 * 2], y2 = uv[v2 * 2 + 1];
    const float area = edge_fn(x0, y0, x1, y1, x2, y2);
    const float fw = (float)wh;
    const float yp = (float)(2 * yi + 1 - wh) / fw;
    const float xp = (float)(2 * xi + 1 - wh) / fw;
    const float w0 = edge_fn(x1, y1, x2, y2, xp, yp) / area;
    const float w1 = edge_fn(x2, y2, x0, y0, xp, yp) / area;
    const float w2 = edge_fn(x0, y0, x1, y1, xp, yp) / area;
    float nx = (w0 * nrm[v0 * 3 + 0] + w1 * nrm[v1 * 3 + 0]) + w2 * nrm[v2 * 3 + 0];
    float ny = (w0 * nrm[v0 * 3 + 1] + w1 * nrm[v1 * 3 + 1]) + w2 * nrm[v2 * 3 + 1];
    float nz = (w0 * nrm[v0 * 3 + 2] + w1 * nrm[v1 * 3 + 2]) + w2 * nrm[v2 * 3 + 2];
    const float len2 = (nx * nx + ny * ny) + nz * nz;
    if (!(len2 >= 1e-24f)) {       // no usable normal (or NaN): towards the camera
        nx = 0.f; ny = 0.f; nz = -1.f;
    } else {
        const float len = sqrtf(len2);
        nx = nx / len; ny = ny / len; nz = nz / len;
    }
    // the winning face's own geometric normal, z component, as render_normal_kernel forms it: one decision per face
    const float gz = (pt[v1 * 3 + 0] - pt[v0 * 3 + 0]) * (pt[v2 * 3 + 1] - pt[v0 * 3 + 1]) - (pt[v1 * 3 + 1] - pt[v0 * 3 + 1]) * (pt[v2 * 3 + 0] - pt[v0 * 3 + 0]);
    if (gz > 0.f) { nx = -nx; ny = -ny; nz = -nz; }
    float lam = o.ambient;
    for (int l = 0; l < o.n_lights; ++l) {
        const float d = (nx * o.light_dir[l * 3 + 0] + ny * o.light_dir[l * 3 + 1]) + nz * o.light_dir[l * 3 + 2];
        lam = lam + o.light_intensity[l] * fmaxf(d, 0.f);
    }
    lam = fminf(lam, 1.f);
    for (int k = 0; k < 3; ++k) rgb[i * 3 + k] = quantise(o.colour[k] * lam);
    if (mask) mask[i] = 1;
    if (depth) depth[i] = key_depth((unsigned)(key >> 32));
    if (face_ids) face_ids[i] = f;
}

}  // namespace

int straps_fill_bytes(void* ptr, size_t bytes, unsigned char value, hipStream_t st);      // csrc/augment.hip

extern "C" size_t straps_render_mesh_workspace_bytes(long long batch, int nverts, int wh) {
    if (batch <= 0 || nverts <= 0 || wh <= 0 || wh > 4096) return 0;
    return (size_t)batch * ((size_t)wh * wh * sizeof(unsigned long long) + (size_t)nverts * 8 * sizeof(float));
}

extern "C" int straps_render_mesh(const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_faces, const float* cam_wp,
                                  int ld_cam, const float* rotation, int rotation_per_body, const straps_render_opts_t* opts, const uint8_t* background,
                                  uint8_t* rgb, uint8_t* mask, float* depth, int32_t* face_ids, void* workspace, long long batch, int nverts, int nfaces,
                                  int wh, void* stream) {
    STRAPS_REQUIRE(verts, "straps_render_mesh: `verts` is a null pointer");
    STRAPS_REQUIRE(faces, "straps_render_mesh: `faces` is a null pointer");
    STRAPS_REQUIRE(vf_offsets, "straps_render_mesh: `vf_offsets` is a null pointer");
    STRAPS_REQUIRE(vf_faces, "straps_render_mesh: `vf_faces` is a null pointer");
    STRAPS_REQUIRE(cam_wp, "straps_render_mesh: `cam_wp` is a null pointer");
    STRAPS_REQUIRE(opts, "straps_render_mesh: `opts` is a null pointer");
    STRAPS_REQUIRE(rgb, "straps_render_mesh: `rgb` is a null pointer");
    STRAPS_REQUIRE(workspace, "straps_render_mesh: `workspace` is a null pointer");
    STRAPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "straps_render_mesh: `workspace` must be 8-byte aligned");
    STRAPS_REQUIRE(ld_cam >= 3, "straps_render_mesh: `ld_cam` must be at least 3 (got %d)", ld_cam);
    STRAPS_REQUIRE(batch > 0 && nverts > 0 && nfaces > 0, "straps_render_mesh: `batch`, `nverts` and `nfaces` must be positive (got %lld, %d, %d)", batch,
                   nverts, nfaces);
    STRAPS_REQUIRE(nfaces <= 0x7fffffff / 3, "straps_render_mesh: `nfaces` must be at most 715827882 (got %d)", nfaces);      // faces[f * 3 + k], table entries in int
    STRAPS_REQUIRE(wh >= 1 && wh <= 4096, "straps_render_mesh: `wh` must be in 1..4096 (got %d)", wh);
    STRAPS_REQUIRE(opts->n_lights >= 0 && opts->n_lights <= 4, "straps_render_mesh: `n_lights` must be in 0..4 (got %d)", opts->n_lights);
    STRAPS_REQUIRE(opts->ambient >= 0.f && opts->ambient <= 3.4e38f, "straps_render_mesh: `ambient` must be finite and not negative (got %g)", (double)opts->ambient);
    const long long nv = batch * nverts, nf = batch * nfaces, np = batch * (long long)wh * wh;
    STRAPS_REQUIRE(batch < (1LL << 31) && (nv + 255) / 256 < (1LL << 31) && (nf * RD_LANES + 255) / 256 < (1LL << 31) && (np + 255) / 256 < (1LL << 31),
                   "straps_render_mesh: `batch` too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* zbuf = (unsigned long long*)workspace;
    float* pt = (float*)(zbuf + np);
    float* uv = pt + nv * 3;
    float* nrm = uv + nv * 2;
    {
        const int rc = straps_fill_bytes(zbuf, (size_t)np * sizeof(unsigned long long), 0xff, st);
        if (rc != STRAPS_OK) return rc;
    }
    hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, verts, cam_wp, ld_cam, rotation, rotation_per_body, pt, uv, nv,
                       nverts);
    STRAPS_CHECK_LAUNCH("render_vertex_kernel");
    hipLaunchKernelGGL(render_normal_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, pt, faces, vf_offsets, vf_faces, nrm, nv, nverts, nfaces);
    STRAPS_CHECK_LAUNCH("render_normal_kernel");
    hipLaunchKernelGGL(render_face_kernel, dim3((unsigned)((nf * RD_LANES + 255) / 256)), dim3(256), 0, st, uv, pt, faces, zbuf, nf, nverts, nfaces, wh);
    STRAPS_CHECK_LAUNCH("render_face_kernel");
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, zbuf, uv, pt, nrm, faces, *opts, background, rgb, mask, depth,
                       face_ids, np, nverts, wh);
    STRAPS_CHECK_LAUNCH("render_resolve_kernel");
    return STRAPS_OK;
}
