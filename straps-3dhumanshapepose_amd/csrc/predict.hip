// predict.hip -- the predict-side front end on the device: detector silhouette + 2-D keypoints -> the regressor's proxy input
// (predict/predict_3D.py:116-126: utils/image_utils.py:108-163 crop_and_resize_silhouette_joints, predict_3D.py:67-76
// create_proxy_representation, utils/label_conversions.py:58-87 the numpy heat maps), for a batch, without a host hop.
//
//   predict_bbox_kernel  : one workgroup per sample: min/max row/col of the non-zero bytes (16-byte loads), then the reference's double
//                          box arithmetic: centre, side = max(h, w) * scale, int16 truncation of the four corners.  NOT clamped (the
//                          training-side crop_bbox_kernel of image.hip clamps): the part of the window outside the frame reads as zero,
//                          which is what the reference's crop + copyMakeBorder produce.  boxes[b] = {wr0, wc0, wr1, wc1, valid, 0}.
//   predict_write_kernel : grid over (sample, channel, 16-row tile); every element of out_nchw is stored exactly once, as float4.
//                          Channel 0: nearest resize of the virtual window (OpenCV's resizeNN index rule, as crop_resize_kernel).
//                          Channel 1 + j: the Gaussian patch around the int16-truncated joint; outside the patch zeros, the table untouched.
//                          The (channel 1 + j, tile 0) workgroup also writes out_joints2d[b][j].
#include "common.h"

// the box and joint arithmetic is the reference's double arithmetic, unfused, so that the int16 truncations agree with numpy's
#pragma clang fp contract(off)

namespace {

constexpr int TILE_ROWS = 16;

__device__ __forceinline__ void bbox_take(int r, int c, int& rmin, int& rmax, int& cmin, int& cmax) {
    rmin = min(rmin, r); rmax = max(rmax, r); cmin = min(cmin, c); cmax = max(cmax, c);
}

// bit 7 of every non-zero byte of x
__device__ __forceinline__ unsigned nonzero_bytes(unsigned x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

// sixteen bytes (not all zero) that start at byte p of the frame
__device__ __forceinline__ void bbox_vector(const uint4& v, int p, int w, int& rmin, int& rmax, int& cmin, int& cmax) {
    int r = p / w, c = p - r * w;
    if (c + 16 <= w) {      // inside one row: its first and last non-zero byte
        const unsigned m0 = nonzero_bytes(v.x), m1 = nonzero_bytes(v.y), m2 = nonzero_bytes(v.z), m3 = nonzero_bytes(v.w);
        const int first = m0 ? (__ffs((int)m0) - 1) >> 3 : m1 ? 4 + ((__ffs((int)m1) - 1) >> 3) : m2 ? 8 + ((__ffs((int)m2) - 1) >> 3) : 12 + ((__ffs((int)m3) - 1) >> 3);
        const int last = m3 ? 12 + ((31 - __clz((int)m3)) >> 3) : m2 ? 8 + ((31 - __clz((int)m2)) >> 3) : m1 ? 4 + ((31 - __clz((int)m1)) >> 3) : (31 - __clz((int)m0)) >> 3;
        bbox_take(r, c + first, rmin, rmax, cmin, cmax);
        cmax = max(cmax, c + last);
        return;
    }
    const unsigned q0 = v.x, q1 = v.y, q2 = v.z, q3 = v.w;      // crosses a row end: byte by byte
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const unsigned word = e < 4 ? q0 : e < 8 ? q1 : e < 12 ? q2 : q3;
        if ((word >> ((e & 3) * 8)) & 0xffu) bbox_take(r, c, rmin, rmax, cmin, cmax);
        if (++c == w) { c = 0; ++r; }
    }
}

__global__ __launch_bounds__(1024) STRAPS_NO_PACKED_FP32 void predict_bbox_kernel(const uint8_t* __restrict__ sil, double scale,
                                                                               int32_t* __restrict__ boxes, int h, int w) {
    __shared__ int red[16][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = h * w;                                          // h, w < 32768: below 2^30
    const uint8_t* s = sil + (long long)b * n;
    int rmin = 1 << 30, rmax = -1, cmin = 1 << 30, cmax = -1;
    // [0, lead) and [lead + 16 * nvec, n) byte by byte, the 16-byte aligned middle as uint4
    int lead = (int)((16 - ((uintptr_t)s & 15)) & 15);
    if (lead > n) lead = n;
    const int nvec = (n - lead) >> 4, tail = lead + (nvec << 4);
    for (int i = tid; i < lead + (n - tail); i += 1024) {
        const int p = i < lead ? i : tail + (i - lead);
        if (s[p] != 0) bbox_take(p / w, p % w, rmin, rmax, cmin, cmax);
    }
    // eight independent 16-byte loads per thread and trip (128 KiB in flight per workgroup: one workgroup has a whole frame to read),
    // then the non-zero vectors only
    const uint4* sv = reinterpret_cast<const uint4*>(s + lead);
    for (int base = 0; base < nvec; base += 8 * 1024) {
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = sv[min(base + k * 1024 + tid, nvec - 1)];      // (unconditional: behind the end, the last vector again)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = min(base + k * 1024 + tid, nvec - 1);
            if ((v[k].x | v[k].y | v[k].z | v[k].w) != 0u) bbox_vector(v[k], lead + (i << 4), w, rmin, rmax, cmin, cmax);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rmin = min(rmin, __shfl_xor(rmin, o, 64)); cmin = min(cmin, __shfl_xor(cmin, o, 64));
        rmax = max(rmax, __shfl_xor(rmax, o, 64)); cmax = max(cmax, __shfl_xor(cmax, o, 64));
    }
    if (lane == 0) { red[wave][0] = rmin; red[wave][1] = rmax; red[wave][2] = cmin; red[wave][3] = cmax; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 16; ++k) {
            rmin = min(rmin, red[k][0]); rmax = max(rmax, red[k][1]); cmin = min(cmin, red[k][2]); cmax = max(cmax, red[k][3]);
        }
        int wr0 = 0, wc0 = 0, wr1 = 0, wc1 = 0, valid = 0;
        if (rmax >= 0) {
            // utils/image_utils.py:23-41,115-121 in double, like numpy; no clamp: the window may leave the frame
            const double cr = (rmin + rmax) / 2.0, cc = (cmin + cmax) / 2.0;
            const double height = rmax - rmin, width = cmax - cmin;
            const double side = (height > width ? height : width) * scale;
            wr0 = (int)(short)(int)(cr - side / 2.0); wc0 = (int)(short)(int)(cc - side / 2.0);      // .astype(np.int16): truncation toward zero
            wr1 = (int)(short)(int)(cr + side / 2.0); wc1 = (int)(short)(int)(cc + side / 2.0);
            valid = wr1 - wr0 > 0 && wc1 - wc0 > 0;             // (the reference raises on an empty silhouette and on an empty crop)
        }
        int32_t* o = boxes + (long long)b * 6;
        o[0] = wr0; o[1] = wc0; o[2] = wr1; o[3] = wc1; o[4] = valid; o[5] = 0;
    }
}

__global__ __launch_bounds__(256) STRAPS_NO_PACKED_FP32 void predict_write_kernel(const uint8_t* __restrict__ sil, const float* __restrict__ joints,
                                                                                int ld_joint, const float* __restrict__ patch, int std,
                                                                                const int32_t* __restrict__ boxes, float* __restrict__ out,
                                                                                float* __restrict__ jout, int h, int w, int nj, int owh, int tiles) {
    const int nch = 1 + nj;
    const int tile = blockIdx.x % tiles;
    const int c = (blockIdx.x / tiles) % nch;
    const int b = blockIdx.x / (tiles * nch);
    const int tid = threadIdx.x;
    const int* bx = boxes + (long long)b * 6;
    const int wr0 = bx[0], wc0 = bx[1], ch = bx[2] - bx[0], cw = bx[3] - bx[1], valid = bx[4];
    const int n4 = owh >> 2;                                     // float4 per row
    const int y0 = tile * TILE_ROWS, rows = min(TILE_ROWS, owh - y0);
    f32x4* o = reinterpret_cast<f32x4*>(out + (((long long)b * nch + c) * owh + y0) * owh);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    if (c == 0) {
        if (!valid) {
            for (int i = tid; i < rows * n4; i += 256) o[i] = zero;
            return;
        }
        // OpenCV resizeNN: ifx = 1 / inv_scale_x with inv_scale_x = (double)dst / src; sx = min(cvFloor(x * ifx), src - 1)
        const double ify = 1.0 / ((double)owh / (double)ch), ifx = 1.0 / ((double)owh / (double)cw);
        const uint8_t* s = sil + (long long)b * h * w;
        for (int i = tid; i < rows * n4; i += 256) {
            const int yl = i / n4, x0 = (i - yl * n4) << 2;
            int sy = (int)floor((double)(y0 + yl) * ify);
            sy = wr0 + (sy < ch - 1 ? sy : ch - 1);
            f32x4 v = zero;
            if (sy >= 0 && sy < h) {
                const uint8_t* row = s + (long long)sy * w;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int sx = (int)floor((double)(x0 + e) * ifx);
                    sx = wc0 + (sx < cw - 1 ? sx : cw - 1);
                    if (sx >= 0 && sx < w) v[e] = (float)row[sx];
                }
            }
            o[i] = v;
        }
        return;
    }

    // heat-map channel of joint j (utils/label_conversions.py:58-87 on joints.astype(np.int16))
    const int j = c - 1, size = 2 * std, psz = 2 * size;
    int jx = 0, jy = 0, visible = 0;
    float fx = 0.f, fy = 0.f;
    if (valid) {
        const float* jp = joints + ((long long)b * nj + j) * ld_joint;
        // numpy: float32 joints - int16 corner in float32, then times the float64 scale
        const double dx = (double)(jp[0] - (float)wc0) * ((double)owh / (double)cw);
        const double dy = (double)(jp[1] - (float)wr0) * ((double)owh / (double)ch);
        fx = (float)dx; fy = (float)dy;
        jx = (int)(short)(int)dx; jy = (int)(short)(int)dy;
        visible = jx > -size && jy > -size && jx < owh - 1 + size && jy < owh - 1 + size;
    }
    if (tile == 0 && tid == 0) {
        float* jo = jout + ((long long)b * nj + j) * 2;
        jo[0] = fx; jo[1] = fy;
    }
    // rows [ys, ye) x cols [xs, xe) receive patch[y - jy + size][x - jx + size]; the end is exclusive at owh - 1, as in the reference
    const int ys = max(0, jy - size), ye = min(owh - 1, jy + size), xs = max(0, jx - size), xe = min(owh - 1, jx + size);
    if (!visible || ys >= y0 + rows || ye <= y0 || xs >= xe) {
        for (int i = tid; i < rows * n4; i += 256) o[i] = zero;
        return;
    }
    for (int i = tid; i < rows * n4; i += 256) {
        const int yl = i / n4, x0 = (i - yl * n4) << 2, y = y0 + yl;
        f32x4 v = zero;
        if (y >= ys && y < ye && x0 + 4 > xs && x0 < xe) {
            const float* prow = patch + (y - jy + size) * psz + (size - jx);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x0 + e >= xs && x0 + e < xe) v[e] = prow[x0 + e];
        }
        o[i] = v;
    }
}

}  // namespace

extern "C" int straps_predict_proxy_input(const uint8_t* sil, const float* joints2d, int ld_joint, const float* gauss_patch, int std,
                                          double bbox_scale_factor, float* out_nchw, float* out_joints2d, int32_t* boxes,
                                          int batch, int h, int w, int nj, int out_wh, void* stream) {
    STRAPS_REQUIRE(sil, "straps_predict_proxy_input: `sil` is a null pointer");
    STRAPS_REQUIRE(joints2d, "straps_predict_proxy_input: `joints2d` is a null pointer");
    STRAPS_REQUIRE(gauss_patch, "straps_predict_proxy_input: `gauss_patch` is a null pointer");
    STRAPS_REQUIRE(out_nchw, "straps_predict_proxy_input: `out_nchw` is a null pointer");
    STRAPS_REQUIRE(out_joints2d, "straps_predict_proxy_input: `out_joints2d` is a null pointer");
    STRAPS_REQUIRE(boxes, "straps_predict_proxy_input: `boxes` is a null pointer");
    STRAPS_REQUIRE(batch > 0 && nj > 0, "straps_predict_proxy_input: `batch` and `nj` must be positive (got %d, %d)", batch, nj);
    STRAPS_REQUIRE(h > 0 && w > 0 && h < 32768 && w < 32768,
                   "straps_predict_proxy_input: `h` and `w` must be in 1..32767, like the reference's int16 box arithmetic (got %d, %d)", h, w);
    STRAPS_REQUIRE(ld_joint >= 2, "straps_predict_proxy_input: `ld_joint` must be at least 2 (x, y, ...), got %d", ld_joint);
    STRAPS_REQUIRE(std > 0 && std < 4096, "straps_predict_proxy_input: `std` must be in 1..4095 (got %d)", std);
    STRAPS_REQUIRE(out_wh > 0 && out_wh < 32768 && out_wh % 4 == 0,
                   "straps_predict_proxy_input: `out_wh` must be a positive multiple of 4 below 32768 (got %d)", out_wh);
    STRAPS_REQUIRE(((uintptr_t)out_nchw & 15) == 0, "straps_predict_proxy_input: `out_nchw` must be 16-byte aligned");
    const int tiles = (out_wh + TILE_ROWS - 1) / TILE_ROWS;
    const long long blocks = (long long)batch * (1 + nj) * tiles;
    STRAPS_REQUIRE(blocks <= 0x7fffffffLL, "straps_predict_proxy_input: `batch` x (1 + `nj`) x row tiles = %lld workgroups exceed the grid limit", blocks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(predict_bbox_kernel, dim3(batch), dim3(1024), 0, st, sil, bbox_scale_factor, boxes, h, w);
    STRAPS_CHECK_LAUNCH("predict_bbox_kernel");
    hipLaunchKernelGGL(predict_write_kernel, dim3((unsigned)blocks), dim3(256), 0, st, sil, joints2d, ld_joint, gauss_patch, std, boxes, out_nchw,
                       out_joints2d, h, w, nj, out_wh, tiles);
    STRAPS_CHECK_LAUNCH("predict_write_kernel");
    return STRAPS_OK;
}
