/* straps_hip.h -- C ABI of the MI355X-native STRAPS hot path (libstraps_hip.so, gfx950 only).
 *
 * The reference has no FFI of its own: its operator boundary is the Python nn.Module surface
 * (SURVEY.md 8b).  These entry points are what a ctypes binding placed under that surface calls;
 * each one names the reference code it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); nothing synchronises;
 *   - no hidden allocation: outputs and workspaces are caller-owned, sizes given by *_bytes();
 *   - return value: 0 = STRAPS_OK, otherwise an error code; straps_last_error() gives the text;
 *   - every tensor at the boundary is fp32.  Arithmetic: fp32 everywhere, except where an entry point
 *     says otherwise -- the bf16x3 convolutions (operands split into three exact bf16 planes, six
 *     products per term on the bf16 matrix pipe, fp32 accumulate: the fp32 chain's accuracy class), the
 *     opt-in single-product bf16 inference route (operands rounded to bf16, one product per term, fp32
 *     accumulate: bf16 accuracy; straps_conv_fwd_bf16, regressor precision 3) and the fp16x3 SMPL modes.
 *     The fp32 routes use fp32-input MFMA (exact fmaf chains);
 *   - activations inside the encoder are NHWC fp32; the boundary tensor (network input) is NCHW
 *     exactly as the reference passes it (models/regressor.py:43).
 */
#ifndef STRAPS_HIP_H
#define STRAPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STRAPS_ABI_VERSION 12

#define STRAPS_OK 0
#define STRAPS_EINVAL 1       /* bad argument (shape, alignment, null pointer) */
#define STRAPS_EHIP 2         /* a HIP runtime call / kernel launch failed */
#define STRAPS_EUNSUPPORTED 3 /* valid request this build does not cover */

int straps_abi_version(void);
/* calibration: `blocks` x 4 waves each issue 4*iters register-resident fp32 MFMAs (32x32x2);
 * seed512 = 512 floats, out = blocks*256 floats.  Time it to get the board's sustained MFMA rate. */
int straps_selftest_mfma_peak(const float* seed512, float* out, int blocks, int iters, void* stream);
/* calibration of the bf16 matrix pipe: `blocks` x 4 waves each issue iters x 48 register-resident v_mfma_f32_32x32x16_bf16 on
 * operand-like data (out = blocks*256 floats; clk2 optional: shader / wall ticks of workgroup 0).  Timed, it gives the rate the pipe
 * SUSTAINS under the board's power budget -- the ceiling of the bf16x3 convolution kernels (bench.py: roofline.sustained_*). */
int straps_selftest_mfma_bf16(float* out, unsigned long long* clk2, int blocks, int iters, void* stream);
/* the same with a DENSE issue stream (round 6): eight independent accumulators per wave, two waves per SIMD at blocks = 512; `blocks` x 4 waves each
 * issue iters x 96 MFMAs; data = 0: all-zero operands (no power limit on the pipe's data path), 1: operand-like bit patterns as above.  bench.py
 * reports both (`roofline.sustained_mfma`), with MfmaUtil from its counter pass. */
int straps_selftest_mfma_bf16_dense(float* out, unsigned long long* clk2, int blocks, int iters, int data, void* stream);
const char* straps_last_error(void);
/* number of visible HIP devices (0 => the product path must refuse to run) */
int straps_device_count(void);
/* measurement aid (bench.py `sclk_mhz`; no reference counterpart): with acc2 != NULL (a zeroed device pair of 64-bit counters),
 * workgroup 0 of every implicit-GEMM convolution (and matrix-pipe SMPL vertex kernel) launched AFTERWARDS (incl. launches captured into a hipGraph afterwards) adds the
 * shader-clock ticks and the constant-rate wall ticks of its lifetime to acc2[0] / acc2[1]; sustained shader clock in MHz =
 * acc2[0] / acc2[1] * straps_wall_clock_khz() / 1000.  NULL switches it off (the default: library use pays nothing).  The setting is
 * PER DEVICE (the current one); clear it before freeing the buffer, and do not replay hipGraphs captured with it afterwards.           */
int straps_wall_clock_khz(void);
int straps_set_clock_accumulator(unsigned long long* acc2);

/* ------------------------------------------------------------------------------------------
 * Encoder -- replaces nn.Conv2d / nn.BatchNorm2d / nn.ReLU / nn.MaxPool2d / AdaptiveAvgPool2d as
 * used by models/resnet.py:145-157 (stem), :61-77 (BasicBlock), :101-121 (Bottleneck), :201-216.
 * ------------------------------------------------------------------------------------------ */

/* OIHW [cout][cin][kh][kw] (PyTorch layout, models/resnet.py:30,36) -> KRSC [cout][kh][kw][cin]. */
int straps_pack_conv_weight(const float* w_oihw, float* w_krsc, int cout, int cin, int kh, int kw,
                            void* stream);
/* transposed copy for the data-gradient pass: OIHW -> [cin][kh][kw][cout] with the taps flipped
 * (dgrad of a conv is a conv with rotated filters).                                           */
int straps_pack_conv_weight_dgrad(const float* w_oihw, float* w_crsk, int cout, int cin, int kh,
                                  int kw, void* stream);
/* both packings of MANY conv layers in one launch (a training step repacks every layer after the
 * optimiser update: 2 x 19 / 2 x 52 tiny launches otherwise).  descs: DEVICE array of n entries sorted by
 * `first` (prefix sum of cout*cin*kh*kw); dst_crsk may be NULL (forward only); total = sum of elements. */
typedef struct {
    const float* src;          /* OIHW */
    float* dst_krsc;
    float* dst_crsk;
    int32_t o, c, r, s;
    long long first;
} straps_pack_desc_t;
int straps_pack_conv_weights_batched(const straps_pack_desc_t* descs, int n, long long total,
                                     void* stream);
/* the same launch for the bf16x3 route: the three bf16 planes [3][plane_stride] of the two packed layouts are written in the same
 * pass -- no split pass over the packed weights.  Planes are CHUNK-MAJOR (what straps_conv_fwd_x3 / straps_conv_dgrad_x3 read):
 * inside a layer's slot (element `first` ..) the weight of GEMM row `row`, tap `tap`, reduction index k sits at
 *     ((tap * (K / 32) + k / 32) * rows + row) * 32 + k % 32
 * with (row, k, rows, K) = (cout, cin, Cout, Cin) for the forward planes and (cin, cout, Cin, Cout) with flipped taps for the
 * data-gradient planes: the 64 bytes of one 32-wide K chunk of one row lie next to the neighbouring rows' (whole 128-byte lines
 * per LDS-DMA fetch).  A layer's planes are written only if its K is a multiple of 32 (others cannot run on this route).
 * Either plane buffer may be NULL; dst_krsc / dst_crsk of a descriptor may be NULL when only the planes are consumed.       */
int straps_pack_conv_weights_batched_x3(const straps_pack_desc_t* descs, int n, long long total,
                                        unsigned short* krsc_planes, unsigned short* crsk_planes,
                                        long long plane_stride, void* stream);

/* stem weights OIHW [64][cin][7][7] (models/resnet.py:145) -> MFMA fragment order
 * [ceil(cin*49/8)][2][64][4]; straps_stem_weight_floats gives the element count.              */
size_t straps_stem_weight_floats(int cin);
int straps_pack_stem_weight(const float* w_oihw, float* w_frag, int cin, void* stream);

/* BatchNorm eval-mode fold (models/resnet.py:147 in .eval()): scale = gamma/sqrt(var+eps),
 * shift = beta - mean*scale.                                                                  */
int straps_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
                   float eps, float* scale, float* shift, int c, void* stream);
/* the same fold plus the statistics as the training-mode kernels take them (save_mean = mean, save_invstd = 1/sqrt(var+eps)):
 * an eval-mode BatchNorm that must back-propagate (nn.BatchNorm2d in .eval() with requires_grad parameters -- fine-tuning with
 * frozen statistics) runs the training-mode kernels on these vectors, with bit 1 of the backward entry points' `accumulate`. */
int straps_bn_fold_stats(const float* gamma, const float* beta, const float* mean, const float* var,
                         float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                         int c, void* stream);

/* diagnostics: with tile_cfg bit 5 set, straps_conv_fwd / straps_conv_dgrad run a build of the implicit-GEMM kernel whose
 * wave 0 of every workgroup writes 8 shader-clock sums (copy wait, barrier, copy issue, MFMA burst, chunks, total, prologue,
 * epilogue) to trace[workgroup][8] (device int64; NULL switches the writes off).  tools/igemm_trace.py.                 */
int straps_conv_trace_buffer(long long* trace);

/* conv7x7/s2/p3 over the NCHW network input, fused y = relu?(conv*scale+shift) -> NHWC.
 * scale/shift may be NULL (raw conv output, used in training mode).  If stats_partial != NULL it
 * receives per-block per-channel (sum, sum of squares) of the RAW conv output:
 * [straps_stem_stat_blocks()][64][2] floats (training-mode BatchNorm statistics).
 * ZERO SKIPPING (exact): the proxy input is a silhouette + truncated joint heat-maps, ~98 % exact
 * zeros.  The kernel contracts only the K groups whose input strips hold a non-zero (a skipped
 * group adds 0*w = 0), so the result equals the dense one bit for bit for finite weights; a dense
 * input skips nothing.  nzmask (optional, from straps_stem_nzmask; NULL = probe by loading) lets it
 * skip even the loads of all-zero 4x8 cells.                                                    */
int straps_stem_stat_blocks(int batch, int h, int w);
size_t straps_stem_nzmask_words(int batch, int cin, int h, int w);
/* one bit per 4-row x 8-column cell of x: mask[B][cin][ceil(h/4)][ceil(w/256)] uint32            */
int straps_stem_nzmask(const float* x_nchw, uint32_t* mask, int batch, int cin, int h, int w,
                       void* stream);
int straps_stem_fwd(const float* x_nchw, const float* w_frag, const float* scale,
                    const float* shift, int relu, float* y_nhwc, float* stats_partial,
                    const uint32_t* nzmask, int batch, int cin, int h, int w, void* stream);

/* generic implicit-GEMM convolution over NHWC fp32 (3x3 pad 1 stride 1|2, 1x1 stride 1|2):
 *   y[m][co] = epilogue( sum_{r,s,ci} x[b][ho*stride+r-pad][wo*stride+s-pad][ci] * w[co][r][s][ci] )
 * epilogue: *scale[co] + shift[co] (if scale), + residual[m][co] (if residual), relu (if relu).
 * cin % 32 == 0 and cout % 64 == 0 required.  stats_partial as for the stem:
 * [straps_conv_stat_blocks(...)][cout][2].  tile_cfg: 0 = auto, 1 = 128x128, 2 = 128x64,
 * 3 = 64x64 block tile.                                                                       */
int straps_conv_stat_blocks(int batch, int ho, int wo, int cout, int kdim /* kh*kw*cin */, int tile_cfg);
int straps_conv_fwd(const float* x_nhwc, const float* w_krsc, const float* scale,
                    const float* shift, const float* residual, int relu, float* y_nhwc,
                    float* stats_partial, int batch, int h, int w, int cin, int cout, int kh,
                    int kw, int stride, int pad, int tile_cfg, void* stream);

/* MaxPool2d(3, stride 2, pad 1) over NHWC (models/resnet.py:149); c % 4 == 0.                  */
int straps_maxpool_fwd(const float* x_nhwc, float* y_nhwc, int batch, int h, int w, int c,
                       void* stream);
/* AdaptiveAvgPool2d(1) + flatten over NHWC (models/resnet.py:157,213-214): [B,hw,c] -> [B,c].  */
int straps_gap_fwd(const float* x_nhwc, float* y, int batch, int hw, int c, void* stream);

/* training-mode BatchNorm (models/resnet.py:47 in .train()): reduce the per-block partials to
 * batch mean / biased variance, emit scale/shift for the apply pass and mean/invstd for backward,
 * and update running_mean / running_var (unbiased, momentum) in place.                         */
int straps_bn_stats_finalize(const float* stats_partial, int nblocks, int c, long long count,
                             const float* gamma, const float* beta, float eps, float momentum,
                             float* running_mean, float* running_var, float* scale, float* shift,
                             float* save_mean, float* save_invstd, void* stream);
/* y = relu?(x*scale[c] + shift[c] (+ residual)) elementwise over NHWC; n = B*H*W rows.          */
int straps_bn_apply(const float* x, const float* scale, const float* shift, const float* residual,
                    int relu, float* y, long long rows, int c, void* stream);

/* ------------------------------------------------------------------------------------------
 * IEF regressor -- replaces nn.Linear x3 x iterations (models/ief_module.py:16-18,48-64).
 * ------------------------------------------------------------------------------------------ */
/* out[m][n] = act( addend[m][n]? + bias[n]? + sum_k x[m][k] * w[n][k] ), fp32 MFMA.
 * x: [m][ldx] (k < kdim valid, ldx % 4 == 0, kdim % 8 == 0, padding columns must be zero),
 * w: [n_pad][ldw] rows n >= n are zero-padded up to a multiple of 32, out/addend: [m][ldo].
 * out may alias addend (in-place residual update of the estimate, models/ief_module.py:57).     */
int straps_linear_fwd(const float* x, int ldx, const float* w, int ldw, const float* bias,
                      const float* addend, float* out, int ldo, int m, int n, int kdim, int relu,
                      void* stream);
/* broadcast the initial estimate (models/ief_module.py:50-52): est[m][0..157) = init, pad = 0  */
int straps_broadcast_rows(const float* row, int cols, float* dst, int ld_dst, int m, void* stream);
/* the three repacked weight views the IEF kernels read, one launch per parameter update:
 * fc1.weight [h1][f + p] -> w1f [h1][f] (feature columns) and w1e [h1][ld_e] (estimate columns, zero padded to ld_e >= p);
 * fc3.weight [p][h2] -> w3 [p rounded up to 32][h2] (zero rows).  models/ief_module.py:16-18,54.                             */
int straps_ief_pack(const float* fc1_w, const float* fc3_w, float* w1f, float* w1e, float* w3, int f, int p,
                    int h1, int h2, int ld_e, void* stream);
/* up to STRAPS_GEMM_MULTI_MAX small strided fp32-MFMA GEMMs in ONE launch (backward of the IEF's nn.Linear layers,
 * models/ief_module.py:55-58 differentiated): per problem
 *     v[m][n] = sum_k a[m*sam + k*sak] * b[k*sbk + n*sbn]  (+ addend[m*ldadd + n])  (then 0 where mask[m*ldmask + n] <= 0)
 *     c[m*ldc + n] (+)= v ;  c2[m*ldc2 + n] (+)= v   (c2 optional)
 * The descriptors are HOST memory (copied into the kernel arguments).  With the three iterations' activations stacked
 * row-wise, a weight gradient is ONE problem with k = 3 x batch, a bias gradient the same with a = a single 1.0f (sam = sak = 0). */
#define STRAPS_GEMM_MULTI_MAX 8
typedef struct {
    const float* a; long long sam, sak;
    const float* b; long long sbk, sbn;
    float* c; int32_t ldc, accumulate;
    const float* addend; int32_t ldadd, reserved0;
    const float* mask; int32_t ldmask, reserved1;
    float* c2; int32_t ldc2, accumulate2;
    int32_t m, n, k, reserved2;
} straps_gemm_desc_t;
int straps_gemm_multi(const straps_gemm_desc_t* descs_host, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pose representation -- utils/rigid_transform_utils.py:27-41 and smplx.lbs.batch_rodrigues.
 * ------------------------------------------------------------------------------------------ */
/* x6 [rows][ld]: each row holds `per_row` 6-D rotations (interleaved a1x,a2x,a1y,a2y,a1z,a2z)
 * starting at column 0 -> R [rows*per_row][3][3] row-major (columns b1,b2,b3).                  */
int straps_rot6d_fwd(const float* x6, long long ld, int per_row, float* rotmats, long long rows,
                     void* stream);
/* axis-angle [n][3] -> R [n][3][3] (angle = ||r + 1e-8||).                                      */
int straps_rodrigues_fwd(const float* aa, float* rotmats, long long n, void* stream);
/* gradient of straps_rodrigues_fwd: aa [n][3], drotmats = dL/dR [n][3][3] -> daa [n][3].  The exact derivative of the
 * formula the forward evaluates (autograd of angle = ||r + 1e-8||, d = r / angle, R = I + sin K + (1 - cos) K^2,
 * K = skew(d)), the +1e-8 included: a zero row gives the finite vee(antisymmetric part of dR) autograd gives there.
 * One lane per rotation, fp32.                                                                  */
int straps_rodrigues_bwd(const float* aa, const float* drotmats, float* daa, long long n, void* stream);
/* utils/cam_utils.py:5-26 orthographic_project_torch: points [batch][n][3], cam rows [s, tx, ty] (row stride ld_cam)
 * -> out [batch][n][2] = s * (x + tx, y + ty); and its gradient (dpoints [batch][n][3] and / or dcam [batch][3]; per-body
 * sums in a fixed order).                                                                          */
int straps_orthographic_project(const float* points, const float* cam, int ld_cam, float* out,
                                long long batch, int n, void* stream);
int straps_orthographic_project_bwd(const float* points, const float* cam, int ld_cam, const float* dout,
                                    float* dpoints, float* dcam, long long batch, int n, void* stream);
/* utils/cam_utils.py:40-71 perspective_project_torch: p = R x + t, p /= p_z, out = (K p)[:2]; rotation [batch][3][3],
 * translation [batch][3], cam_k one [3][3] (k_per_body = 0) or [batch][3][3] (k_per_body = 1) -> out [batch][n][2].           */
int straps_perspective_project(const float* points, const float* rotation, const float* translation,
                               const float* cam_k, int k_per_body, float* out, long long batch, int n,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * SMPL forward -- models/smpl_official.py:27-41 -> smplx.SMPL.forward -> smplx.lbs.lbs.
 * The model constants are packed ON THE HOST by the Python side (layout documented at
 * straps_smpl_model_t) and uploaded once.
 * ------------------------------------------------------------------------------------------ */
#define STRAPS_SMPL_V 6890
#define STRAPS_SMPL_VPAD 6912   /* 216 tiles of 32 vertices */
#define STRAPS_SMPL_TILES 216
#define STRAPS_SMPL_KP 224      /* 1 (template) + 10 (betas) + 207 (pose feats) + 6 zero pad */
#define STRAPS_SMPL_NJ 24
#define STRAPS_SMPL_NEXTRA 45   /* 9 extra + 19 cocoplus + 17 h36m regressed joints */
#define STRAPS_SMPL_NPICK 21    /* vertices appended by the vertex-joint selector */
#define STRAPS_SMPL_NJOINTS_OUT 90

typedef struct {
    /* blend directions in MFMA A-fragment order: [tile n_tiles][coord 3][kgroup 28][lane 64][4],
     * element = D[k = 8*g + 4*(lane>>5) + e][vertex = 32*tile + (lane&31)][coord], where D row 0
     * is v_template, rows 1..10 shapedirs[..., l], rows 11..217 posedirs, rest zero.
     * Tiles 0..215 are the 6890 mesh vertices; tiles 216..n_tiles-1 hold the VIRTUAL vertices that
     * carry the 45 sparse-regressed joints (see vj_ptr), zero padded to a multiple of 8 tiles.    */
    const float* blend_frag;
    const float* j_template;   /* [24][3]  J_regressor @ v_template (host fp64)              */
    const float* j_shapedirs;  /* [24][3][10] J_regressor @ shapedirs                          */
    const int32_t* parents;    /* [24] */
    const int32_t* depth;      /* [24] depth of each joint in the kinematic tree               */
    int32_t max_depth;
    int32_t skin_k;            /* non-zeros kept per vertex (4 for the real model)              */
    const float* skin_w;       /* [32*n_tiles][skin_k] */
    const int32_t* skin_j;     /* [32*n_tiles][skin_k] joint index of each weight               */
    /* Extra joints (J_regressor_extra | cocoplus | h36m, 45 rows) without a gather: regrouping
     *   joint_j = sum_v R[j,v] sum_k w[v,k] A_k.[v_posed_v;1]  by bone k gives one rigidly skinned
     * virtual vertex per (joint, bone) pair: blend directions sum_v R[j,v] w[v,k] D[:,v] / s and
     * skinning weight s = sum_v R[j,v] w[v,k] on bone k.  They ride through the same contraction
     * as extra tiles; joint j is the sum of virtual vertices [vj_ptr[j], vj_ptr[j+1]).           */
    const int32_t* vj_ptr;     /* [45 + 1] */
    int32_t n_tiles;           /* 216 + virtual tiles, multiple of 8, at most 256 (straps_smpl_fwd refuses more) */
    int32_t reserved0;
    const int32_t* pick_ids;   /* [21] vertex ids appended as joints 24..44                    */
    /* ---- tables used only by straps_smpl_bwd (may be NULL for forward-only use) ---- */
    /* transposed blend fragments [tile 216][coord 3][kblock 7][rq 4][lane 64][4]:
     * element = D[k = 32*kblock + (lane&31)][vertex = 32*tile + row(4*rq+e, lane>>5)][coord],
     * row(r,h) = (r&3) + 8*(r>>2) + 4*h (the MFMA C-layout row of accumulator register r).    */
    const float* blend_frag_t;
    const int32_t* children;   /* [24][3] child joints, -1 padded                              */
    /* joint-gradient sources per vertex tile: entries of tile t in [jrt_ptr[t], jrt_ptr[t+1]);
     * jrt_code = (v_local << 8) | src, src 0..20 = picked-vertex joints 24..44 (weight 1),
     * src 21..65 = regressed joints 45..89.                                                   */
    const int32_t* jrt_ptr;    /* [216 + 1] */
    const int32_t* jrt_code;
    const float* jrt_w;
    /* skinning weights regrouped for the joint-transform gradient: the non-zero weights of round rd (= 4 tiles of 32
     * vertices) on joint j live in [dj_ptr[rd*24 + j], dj_ptr[rd*24 + j + 1]), ascending vertex;
     * dj_code = (tile_in_round << 5) | vertex_in_tile.                                                           */
    const int32_t* dj_ptr;     /* [54*24 + 1] */
    const int32_t* dj_code;
    const float* dj_w;
    /* ---- split-precision forward (mode STRAPS_SMPL_SPLIT_F16; may be NULL / 0 otherwise) ----
     * fp16 two-term split of the blend directions scaled by a power of two S_D: [tile][kstep 14][coord 3][hi|lo][lane 64][8],
     * element = split(S_D * D[k = 16*kstep + 8*(lane>>5) + j][vertex = 32*tile + (lane&31)][coord]), hi = fp16(x),
     * lo = fp16(x - hi); blend_h_unscale = 1 / (S_D * 64) (the kernel scales the features by 64).               */
    const void* blend_frag_h;
    float blend_h_unscale;
    int32_t reserved1;
    /* ---- skinning on the matrix pipe (modes STRAPS_SMPL_SPLIT_F16_LBS*; may be NULL otherwise) ----
     * fp16 two-term split (hi, lo) of 2^14 * W, W = dense skinning weights [32*n_tiles][24] (the virtual vertices carry their single
     * weight), with the three products of the split packed along K:
     *   T = Ah.Wh + Al.Wh + Ah.Wl = [Ah | Al | Ah | -] . [Wh | Wh | Wl | 0]  over 24 + 24 + 24 + 8 = 80 columns = 5 k-steps of 16
     * (instead of 3 products x 2 k-steps of the 24 joints padded to 32): [tile][kstep 5][lane 64][8], element =
     * P[vertex = 32*tile + (lane&31)][col = 16*kstep + 8*(lane>>5) + j],  P = [hi[0:24] | hi[0:24] | lo[0:24] | 0 x 8].               */
    const void* skin_frag_p;
} straps_smpl_model_t;

/* kernel choice of the STRAPS_SMPL_SPLIT_F16_LBS* modes, OR-ed into `mode` (default 0 = by batch size): _WIDE = 64 bodies per workgroup,
 * one wave per SIMD with the whole 512-entry register file (every fetched direction fragment feeds two body groups, skinning
 * products K-packed; the large-batch kernel), _NARROW = 32 bodies per workgroup, two waves per SIMD (small batches).               */
#define STRAPS_SMPL_KERNEL_WIDE 0x100
#define STRAPS_SMPL_KERNEL_NARROW 0x200
/* _WIDE_BUILTIN (with _WIDE; round 6): the 64-body kernel with its skinning chains issued through the compiler's MFMA builtin (AGPR results, every
 * hazard resolved by the compiler) instead of the hand-placed VGPR-result assembly statements of the product form -- the reference instantiation the
 * product form is compared with bit for bit (tests/test_gpu_forward.py): same arithmetic, ~5 % slower.  Plain-fp16x3_lbs mode only.            */
#define STRAPS_SMPL_KERNEL_WIDE_BUILTIN 0x400
/* arithmetic of the blend contraction (v_template + shapedirs + posedirs, K = 218) in straps_smpl_fwd */
#define STRAPS_SMPL_EXACT_F32 0 /* fp32-input MFMA: exact fmaf chains (the reference's fp32 arithmetic)                  */
/* three fp16-MFMA products of two-term splits, fp32 accumulate: ~7e-7 relative per product at 16x the matrix rate;
 * features must satisfy |f| < 1023 (betas and R - I always do)                                                  */
#define STRAPS_SMPL_SPLIT_F16 1
/* as above, and the skinning transforms T[v][b] = sum_j W[v][j] A[b][j] as the same kind of split product on the matrix
 * pipe (any number of weights per vertex); |A| < 63 (metres)                                                     */
#define STRAPS_SMPL_SPLIT_F16_LBS 2
/* as STRAPS_SMPL_SPLIT_F16_LBS with the pose-corrective directions from column 16 on as plain fp16 (two products per term,
 * their low halves are not fetched): ~2^-12 of the pose-corrective displacement (measured: tests/test_gpu_forward.py),
 * inside north_star's 1e-4 m; template and shape directions keep the three-product split                          */
#define STRAPS_SMPL_SPLIT_F16_LBS_PD16 3
/* and the pose features of those columns as plain fp16 too (one product per term)                                  */
#define STRAPS_SMPL_SPLIT_F16_LBS_P16 4

/* bytes of caller-owned scratch for `batch` bodies (depends on the model's virtual-tile count)  */
size_t straps_smpl_workspace_bytes(const straps_smpl_model_t* model, long long batch);
/* verts [B][6890][3], joints [B][90][3] (may be NULL: vertices only).  betas [B][10],
 * rotmats [B][24][3][3] row-major.  chunks: split of the n_tiles/8 tile rounds over blocks, 0 = auto.
 * mode: STRAPS_SMPL_EXACT_F32 or STRAPS_SMPL_SPLIT_F16 (skinning and the joint chain are exact fp32 in both).   */
int straps_smpl_fwd(const straps_smpl_model_t* model, const float* betas, const float* rotmats,
                    float* verts, float* joints, void* workspace, long long batch, int chunks, int mode,
                    void* stream);

/* gradient of straps_smpl_fwd w.r.t. betas [B,10] and rotmats [B,24,3,3] given dverts [B,6890,3]
 * and/or djoints [B,90,3] (either may be NULL = zero) -- what autograd does through smplx.lbs for
 * pred_smpl_output in loss.backward() (train loop :196,:232).
 * chunks: split of the 54 rounds of 4 vertex tiles over workgroups; 0 (or negative) = 8 from 1024 bodies on, 54 below; values above
 * 54 are 54.  A chunk takes ceil(54 / chunks) rounds, so used = ceil(54 / ceil(54 / chunks)) chunks run (5 -> 5 chunks of 11, 11, 11,
 * 11, 10 rounds; 20 -> 18 chunks of 3).  Workspace: batch * (1 + used) * (224 + 288) * 4 bytes -- the recomputed pose features and joint
 * transforms of every body, and one partial of their gradients per chunk.  Results for different `chunks` differ by summation order
 * only; for one value they are bit-reproducible and a body's result does not depend on the rest of the batch.                    */
size_t straps_smpl_bwd_workspace_bytes(long long batch, int chunks);
int straps_smpl_bwd(const straps_smpl_model_t* model, const float* betas, const float* rotmats,
                    const float* dverts, const float* djoints, float* dbetas, float* drotmats,
                    void* workspace, long long batch, int chunks, void* stream);
/* the same gradient for an axis-angle pose (smplx's pose2rot=True): rotmats [B,24,3,3] = straps_rodrigues_fwd of
 * full_pose_aa [B,72] (global orientation first) -> dbetas [B,10] and dfull_pose_aa [B,72], the Rodrigues derivative
 * applied in the epilogue of the pose pass (bit-identical to straps_smpl_bwd followed by straps_rodrigues_bwd).
 * drotmats [B,24,3,3] may be NULL; when given it receives what straps_smpl_bwd writes there.  Workspace size:
 * straps_smpl_bwd_workspace_bytes(batch, chunks).                                                 */
int straps_smpl_bwd_aa(const straps_smpl_model_t* model, const float* betas, const float* rotmats,
                       const float* full_pose_aa, const float* dverts, const float* djoints, float* dbetas,
                       float* dfull_pose_aa, float* drotmats, void* workspace, long long batch, int chunks,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the encoder / IEF / rot6d -- the work of loss.backward() (train loop :232) that
 * cuDNN / cuBLAS / ATen kernels do for the reference.
 * ------------------------------------------------------------------------------------------ */
/* data gradient of straps_conv_fwd (same geometry arguments as the forward; h,w = forward INPUT
 * size): dx = conv_transpose(dy, w) (+ addend, e.g. the skip-connection gradient).
 * w_crsk from straps_pack_conv_weight_dgrad.  cout % 32 == 0, cin % 64 == 0, stride 1 or 2.      */
int straps_conv_dgrad(const float* dy_nhwc, const float* w_crsk, const float* addend,
                      float* dx_nhwc, int batch, int h, int w, int cin, int cout, int kh, int kw,
                      int stride, int pad, int tile_cfg, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same implicit-GEMM convolution on the bf16 matrix pipe at fp32 accuracy (csrc/conv_x3.hip):
 * every fp32 operand is carried as three bf16 planes x = x1 + x2 + x3 (exact, round-to-nearest
 * splits) and a product is the six bf16 products of weight >= 2^-16, accumulated in fp32 --
 * relative error <= ~2^-23 per product, the accuracy class of the fp32 chain, at 2.67x its
 * matrix-pipe rate.  planes: [3][plane_stride] bf16 bit patterns (uint16), plane_stride >= n,
 * a multiple of 8.  Geometry / epilogue arguments exactly as straps_conv_fwd /
 * straps_conv_dgrad; x3 / dy3 are the CHUNK-MAJOR planes of the NHWC tensor [rows = B*H*W][C]:
 * element (row, c) at ((c / 32) * rows + row) * 32 + c % 32 -- 32-channel chunks outermost, so the 64 bytes
 * one K chunk of a pixel contributes lie next to the neighbouring pixels' and an LDS-DMA fetch of a chunk
 * for 16 rows reads 1 KiB of whole 128-byte lines (plain NHWC planes made the same fetch touch half of each
 * of 16 lines: 16-18 vs 31-36 TB/s of useful L2 -> LDS bytes, tools/l2_line_probe.hip); written by
 * straps_split3_bf16_cm and the fused producers below.  w3: the chunk-major weight planes of
 * straps_pack_conv_weights_batched_x3.
 * tile_cfg: 0 = auto (incl. the halo-patch kernel for 3x3 / stride-1 layers: the tile's input patch is
 * copied once per channel chunk and the nine taps are shifted LDS addresses), 1..12 = explicit tiles
 * of the im2col kernel (8..12: software-pipelined loop; csrc/conv_x3.hip), + 256 = auto without the
 * halo-patch kernel, + 512 = the two-buffer halo-patch kernel wherever it applies, + 1024 = the single-buffer one (the rule for
 * 64-channel outputs); bits 6 / 7 select
 * measurement builds with wrong results (no MFMAs / no operand copies; tools/pmc_x3.sh).
 * ------------------------------------------------------------------------------------------ */
/* plain split of n values, planes in the order of x (any fp32 array; the exactness tests)                  */
int straps_split3_bf16(const float* x, unsigned short* planes, long long n, long long plane_stride,
                       void* stream);
/* split of an NHWC tensor [rows][c] (c % 32 == 0) into the chunk-major planes the convolutions read       */
int straps_split3_bf16_cm(const float* x, unsigned short* planes, long long rows, int c,
                          long long plane_stride, void* stream);
/* statistics partials of straps_conv_fwd_x3 for this geometry: [blocks][cout][2]                          */
int straps_conv_x3_stat_blocks(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride,
                               int pad, int tile_cfg);

/* ---- 1x1 convolutions with the A operand read from the fp32 tensor (round 6; csrc/conv_x3f.hip) -------------------------------------
 * models/resnet.py:34-36 (conv1x1) as used by the bottleneck units :80-121 and the shortcut convolutions :172-177.  Same arithmetic as
 * the plane entry points above (three bf16 parts per fp32 value, six products per term, fp32 accumulate -- the two routes give the same
 * bits on the same values), but the kernel splits the activation / gradient itself: the producer writes (and this reads) 4 bytes per
 * element instead of 6-10, and the BatchNorm + ReLU in front of the convolution can ride in the operand path (a_scale / a_shift).       */
/* 1 if straps_conv_fwd_x3f / straps_conv_dgrad_x3f / straps_conv_wgrad_x3f cover the geometry (1x1, pad 0, stride 1 | 2, channels % 64) */
int straps_conv_x3f_supported(int cin, int cout, int kh, int kw, int stride, int pad);
/* y = conv1x1(act(x)) [* scale + shift] [+ residual] [relu]; x: fp32 NHWC [batch][h][w][cin].  a_scale / a_shift ([cin], 16-byte aligned;
 * both or neither): act(x) = x * a_scale + a_shift per channel, then ReLU if a_relu -- x is then the RAW output of the previous
 * convolution and the normalised activation is never materialised; NULL: act(x) = x.  w3: the weights' planes as for
 * straps_conv_fwd_x3.  stats_partial (training): [straps_conv_x3f_stat_blocks][cout][2] partial (sum, sum of squares) of y.            */
int straps_conv_fwd_x3f(const float* x, const float* a_scale, const float* a_shift, int a_relu, const unsigned short* w3,
                        long long w_plane_stride, const float* scale, const float* shift, const float* residual, int relu,
                        float* y, float* stats_partial, int batch, int h, int w, int cin, int cout, int kh, int kw, int stride,
                        int pad, int tile_cfg, void* stream);
int straps_conv_x3f_stat_blocks(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int tile_cfg);
/* dx = dgrad1x1(dy) [+ addend, masked by addend_bits]; dy: fp32 [batch][ho][wo][cout] (no planes of it need exist).  Optional, as in
 * straps_conv_dgrad_x3_bn_bits: the two BatchNorm-backward sums of the BatchNorm (+ ReLU) whose output the convolution read (bn_raw !=
 * NULL; mask = bn_out_bits, else relu'(bn_raw * bn_mask_scale + bn_mask_shift)) into bn_partials [straps_conv_dgrad_x3f_bn_blocks][cin][2]. */
int straps_conv_dgrad_x3f(const float* dy, const unsigned short* w3_crsk, long long w_plane_stride, const float* addend,
                          const unsigned* addend_bits, float* dx, int batch, int h, int w, int cin, int cout, int kh, int kw,
                          int stride, int pad, int tile_cfg, const float* bn_raw, const unsigned* bn_out_bits,
                          const float* bn_mask_scale, const float* bn_mask_shift, const float* bn_mean, const float* bn_invstd,
                          double* bn_partials, void* stream);
int straps_conv_dgrad_x3f_bn_blocks(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int tile_cfg);
/* dW (OIHW [cout][cin][1][1]) of a 1x1 convolution with BOTH operands read from the fp32 tensors (csrc/conv_wgrad_x3f.hip): x [batch][h][w][cin]
 * -- with a_scale / a_shift / a_relu as in straps_conv_fwd_x3f: x is then the RAW output of the previous convolution, the producer's
 * BatchNorm (+ ReLU) is applied in the operand path -- and dy [batch][ho][wo][cout].  workspace: straps_conv_wgrad_x3f_workspace_bytes
 * (split-K partials); accumulate: dW += instead of =.  Same six-product bf16 arithmetic as straps_conv_wgrad_x3.                        */
size_t straps_conv_wgrad_x3f_workspace_bytes(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad);
int straps_conv_wgrad_x3f(const float* x, const float* a_scale, const float* a_shift, int a_relu, const float* dy, float* dw_oihw,
                          void* workspace, int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad,
                          int accumulate, void* stream);
int straps_conv_fwd_x3(const unsigned short* x3, long long x_plane_stride,
                       const unsigned short* w3_krsc, long long w_plane_stride, const float* scale,
                       const float* shift, const float* residual, int relu, float* y_nhwc,
                       float* stats_partial, int batch, int h, int w, int cin, int cout, int kh,
                       int kw, int stride, int pad, int tile_cfg, void* stream);
/* straps_conv_fwd_x3 (no statistics) that also writes its result as planes -- y_nhwc may be NULL when only they are consumed   */
int straps_conv_fwd_x3p(const unsigned short* x3, long long x_plane_stride,
                        const unsigned short* w3_krsc, long long w_plane_stride, const float* scale,
                        const float* shift, const float* residual, int relu, float* y_nhwc,
                        unsigned short* y_planes, long long y_plane_stride, int batch, int h, int w,
                        int cin, int cout, int kh, int kw, int stride, int pad, int tile_cfg, void* stream);
/* ---- single-product bf16 route (csrc/conv_bf16.hip): eval-mode forward only, no gradients ----
 * Every fp32 operand is rounded to the nearest-even bf16 and each term is ONE bf16 product, accumulated in fp32: 1/6 of the bf16x3
 * route's matrix work and 1/3 of its operand bytes, at the accuracy of bf16 operands (relative 2^-9 per operand), not fp32's.
 * straps_split_bf16_cm: x [rows][c] fp32 (c % 32 == 0) -> rn_bf16(x) as ONE chunk-major plane [rows * c] (the layout of plane 0 of
 *   straps_split3_bf16_cm).
 * straps_pack_conv_weight_bf16: OIHW fp32 weights -> rn_bf16 as one chunk-major plane of the forward layout (the layout of plane 0 of
 *   straps_pack_conv_weights_batched_x3's krsc_planes for a single layer at first = 0); cin % 32 == 0.
 * straps_conv_fwd_bf16: y = act(conv(x1, w1) * scale + shift + residual) on one bf16 plane per operand (cin % 64 == 0, cout % 64 == 0);
 *   writes y (fp32 NHWC, may be NULL) and/or y_plane (rn_bf16(y) as one chunk-major plane, may be NULL; not both NULL) -- the next
 *   convolution's operand.  scale / shift / residual may be NULL.  tile_cfg: 0 = automatic; 1..10 force a tile configuration (tools
 *   and tests; a configuration the geometry does not admit is refused, never replaced).
 * straps_conv_bf16_tile_choice: the configuration tile_cfg = 0 takes for this geometry (1..10), -1 if not covered.               */
int straps_split_bf16_cm(const float* x, unsigned short* plane, long long rows, int c, void* stream);
int straps_pack_conv_weight_bf16(const float* w_oihw, unsigned short* w_plane, int cout, int cin, int kh, int kw, void* stream);
int straps_conv_bf16_tile_choice(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad);
int straps_conv_fwd_bf16(const unsigned short* x1, const unsigned short* w1_krsc, const float* scale, const float* shift,
                         const float* residual, int relu, float* y_nhwc, unsigned short* y_plane, int batch, int h, int w,
                         int cin, int cout, int kh, int kw, int stride, int pad, int tile_cfg, void* stream);
int straps_conv_dgrad_x3(const unsigned short* dy3, long long dy_plane_stride,
                         const unsigned short* w3_crsk, long long w_plane_stride,
                         const float* addend, float* dx_nhwc, int batch, int h, int w, int cin,
                         int cout, int kh, int kw, int stride, int pad, int tile_cfg, void* stream);
/* producers of the bf16x3 route that write their fp32 output AND its three planes in one pass (instead of a
 * straps_split3_bf16 pass over the output): straps_bn_apply / straps_bn_relu_maxpool_fwd / straps_bn_bwd with
 * two more arguments (planes [3][plane_stride], plane_stride >= element count, a multiple of 8; draw_planes
 * may be NULL).  The fp32 output of straps_bn_apply_x3 (y) and of straps_bn_bwd_x3 (draw) may be NULL when only
 * bf16x3 kernels consume it: 4 of the 10 bytes per element are then not written.                            */
int straps_bn_apply_x3(const float* raw, const float* scale, const float* shift, const float* residual,
                       int relu, float* y, unsigned short* y_planes, long long plane_stride,
                       long long rows, int c, void* stream);
int straps_bn_relu_maxpool_fwd_x3(const float* raw, const float* scale, const float* shift,
                                  float* y_pool, uint8_t* idx, unsigned short* y_planes,
                                  long long plane_stride, int batch, int h, int w, int c, void* stream);
int straps_bn_bwd_x3(const float* dy, const float* yact, const float* raw, const float* save_mean,
                     const float* save_invstd, const float* gamma, const float* mask_scale,
                     const float* mask_shift, float* dgamma, float* dbeta, float* draw, float* dz_out,
                     unsigned short* draw_planes, long long plane_stride, void* workspace,
                     long long rows, int c, int accumulate, void* stream);
/* The data gradient with the sums of the NEXT BatchNorm backward fused into its epilogue: dx (= the gradient dy entering the
 * BatchNorm + ReLU that produced this convolution's input) is written as by straps_conv_dgrad_x3, and per M tile one partial
 * bn_partials[block][cin][2] = (S1, invstd * S2) of  S1 = sum mask*dy,  S2 = sum mask*dy*(raw - mean)  (double; mask = bn_out > 0
 * if bn_out, else fma(raw, bn_mask_scale, bn_mask_shift) > 0) -- the reduction pass of straps_bn_bwd_x3 over (dy, raw) is not
 * needed: straps_bn_bwd_finish_x3 takes the partials (blocks from straps_conv_dgrad_x3_bn_blocks; workspace: 2 c doubles + c floats). */
int straps_conv_dgrad_x3_bn_blocks(int batch, int h, int w, int cin, int cout, int kh, int kw, int stride,
                                   int pad, int tile_cfg);
int straps_conv_dgrad_x3_bn(const unsigned short* dy3, long long dy_plane_stride,
                            const unsigned short* w3_crsk, long long w_plane_stride, const float* addend,
                            float* dx_nhwc, int batch, int h, int w, int cin, int cout, int kh, int kw,
                            int stride, int pad, int tile_cfg, const float* bn_raw, const float* bn_out,
                            const float* bn_mask_scale, const float* bn_mask_shift, const float* bn_mean,
                            const float* bn_invstd, double* bn_partials, void* stream);
int straps_bn_bwd_finish_x3(const float* dy, const float* yact, const float* raw, const float* save_mean,
                            const float* save_invstd, const float* gamma, const float* mask_scale,
                            const float* mask_shift, float* dgamma, float* dbeta, float* draw, float* dz_out,
                            unsigned short* draw_planes, long long plane_stride, const double* partials,
                            int nblk, void* workspace, long long rows, int c, int accumulate, void* stream);
/* ReLU decisions as BITS (ABI 8).  The backward pass of a residual unit needs the unit's fp32 activation only for its sign:
 * as the ReLU mask of the last BatchNorm's two passes, of the sums fused into the data gradient that produces dy, and of the gradient
 * the skip connection receives (which the fp32 form materialises as dz_out).  straps_bn_apply_bits_x3 (= straps_bn_apply_x3 with
 * relu = 1) also writes  relu_bits[rows][c / 32]:  bit (ch & 31) of word [row][ch / 32] = (y[row][ch] > 0);  the *_bits forms below
 * read those words where the plain forms read an fp32 tensor:
 *   straps_bn_bwd_bits_x3 / straps_bn_bwd_finish_bits_x3   relu_bits instead of yact; no dz_out (consumers mask dy themselves);
 *   straps_conv_dgrad_x3_bits / _bn_bits                   addend_bits: dx = dgrad + (bit ? addend : 0), the addend being the UNMASKED
 *                                                          gradient of the later unit's output;  bn_out_bits instead of bn_out
 *                                                          (either may be NULL: that operand is then used as in the plain form).
 * Results are bit-identical to the fp32-mask forms (models/resnet.py:72-74,115-117: out += identity; out = relu(out)).
 * c (cin for the data gradients) must be a multiple of 32. */
int straps_bn_apply_bits_x3(const float* raw, const float* scale, const float* shift, const float* residual, float* y,
                            unsigned short* y_planes, long long plane_stride, unsigned* relu_bits, long long rows,
                            int c, void* stream);
int straps_bn_bwd_bits_x3(const float* dy, const unsigned* relu_bits, const float* raw, const float* save_mean,
                          const float* save_invstd, const float* gamma, float* dgamma, float* dbeta, float* draw,
                          unsigned short* draw_planes, long long plane_stride, void* workspace, long long rows, int c,
                          int accumulate, void* stream);
int straps_bn_bwd_finish_bits_x3(const float* dy, const unsigned* relu_bits, const float* raw, const float* save_mean,
                                 const float* save_invstd, const float* gamma, float* dgamma, float* dbeta, float* draw,
                                 unsigned short* draw_planes, long long plane_stride, const double* partials, int nblk,
                                 void* workspace, long long rows, int c, int accumulate, void* stream);
int straps_conv_dgrad_x3_bits(const unsigned short* dy3, long long dy_plane_stride, const unsigned short* w3_crsk,
                              long long w_plane_stride, const float* addend, float* dx_nhwc, int batch, int h, int w,
                              int cin, int cout, int kh, int kw, int stride, int pad, int tile_cfg,
                              const unsigned* addend_bits, void* stream);
int straps_conv_dgrad_x3_bn_bits(const unsigned short* dy3, long long dy_plane_stride,
                                 const unsigned short* w3_crsk, long long w_plane_stride, const float* addend,
                                 float* dx_nhwc, int batch, int h, int w, int cin, int cout, int kh, int kw,
                                 int stride, int pad, int tile_cfg, const float* bn_raw, const float* bn_out,
                                 const float* bn_mask_scale, const float* bn_mask_shift, const float* bn_mean,
                                 const float* bn_invstd, double* bn_partials, const unsigned* addend_bits,
                                 const unsigned* bn_out_bits, void* stream);
/* weight gradient on the bf16x3 route: straps_conv_wgrad's arguments plus the planes of x and dy.  3x3 / stride 1 / pad 1
 * layers (power-of-two width >= 8) run the halo-patch kernel on the planes (ds_read_b64_tr_b16 operand gathers); the other
 * 3x3 layers and the 1x1 layers whose channel counts are both >= 128 run the per-tap kernel on the planes; what is left
 * (1x1 with a 64-channel side) -- or NULL planes -- uses the fp32 kernels on (x, dy).  Workspace as for straps_conv_wgrad.   */
/* 1 if straps_conv_wgrad_x3 handles this geometry on the planes alone (x_nhwc / dy_nhwc may then be NULL, and the producers
 * -- straps_bn_apply_x3's y, straps_bn_bwd_x3's draw -- need not write their fp32 copies), 0 if it needs the fp32 tensors.      */
int straps_conv_wgrad_x3_on_planes(int batch, int h, int w, int cin, int cout, int kh, int kw,
                                   int stride, int pad);
int straps_conv_wgrad_x3(const float* x_nhwc, const float* dy_nhwc, const unsigned short* x3,
                         long long x_plane_stride, const unsigned short* dy3, long long dy_plane_stride,
                         float* dw_oihw, void* workspace, int batch, int h, int w, int cin, int cout,
                         int kh, int kw, int stride, int pad, int accumulate, void* stream);


/* weight gradient in the parameter's own OIHW layout: dw (+)= sum_pixels dy (x) x.                */
size_t straps_conv_wgrad_workspace_bytes(int batch, int h, int w, int cin, int cout, int kh,
                                         int kw, int stride, int pad);
int straps_conv_wgrad(const float* x_nhwc, const float* dy_nhwc, float* dw_oihw, void* workspace,
                      int batch, int h, int w, int cin, int cout, int kh, int kw, int stride,
                      int pad, int accumulate, void* stream);
/* The plan of a weight-gradient call: which kernel the library launches for a geometry, with which grid and split-K extent (host
 * arithmetic only, like straps_conv_x3_stat_blocks; added without a version change).  route: the operand form -- what
 * straps_conv_wgrad, straps_conv_wgrad_x3 with planes, straps_conv_wgrad_x3f run.  Returns STRAPS_EINVAL for a geometry the route
 * refuses.  The kernel's grid is tiles x splits; split k covers units [k * unit, min((k + 1) * unit, units)).                   */
#define STRAPS_WG_ROUTE_F32 0     /* fp32 tensors */
#define STRAPS_WG_ROUTE_PLANES 1  /* bf16 planes (falls back to the fp32 tensors where straps_conv_wgrad_x3_on_planes is 0) */
#define STRAPS_WG_ROUTE_F32_1X1 2 /* fp32-operand 1x1 */
#define STRAPS_WG_FAMILY_TAP_F32 0  /* conv_wgrad_kernel<bco, bci> */
#define STRAPS_WG_FAMILY_HALO_F32 1 /* conv_wgrad3x3_kernel */
#define STRAPS_WG_FAMILY_TAP_X3 2   /* conv_wgrad_x3_kernel<bco, bci> */
#define STRAPS_WG_FAMILY_HALO_X3 3  /* conv_wgrad3x3_x3_kernel<chunk_px> */
#define STRAPS_WG_FAMILY_TAP_X3F 4  /* conv_wgrad_x3f_kernel<bco, bci> */
typedef struct straps_wgrad_plan_t {
    int32_t family;
    int32_t bco, bci;   /* channel block of a workgroup (halo families: 64 x 64, all nine taps) */
    int32_t chunk_px;   /* halo families: pixels per chunk, 32 or 64; per-tap families: 0 */
    int32_t tiles;      /* grid.x: taps x channel blocks (halo families: channel blocks) */
    int32_t splits;     /* grid.y = split-K partials */
    int32_t unit;       /* extent of a split: pixel rows (a multiple of 32), halo families: chunks */
    int32_t units;      /* total extent: output pixels M, halo families: chunks */
    int32_t taps;
    int32_t lds_bytes;  /* dynamic LDS of the launch */
    int64_t part_bytes; /* splits x cout x taps x cin floats of the workspace */
} straps_wgrad_plan_t;
int straps_conv_wgrad_plan(int route, int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad,
                           straps_wgrad_plan_t* out);
/* The plan of a forward / data-gradient convolution call: which kernel the library launches for a geometry, a tile_cfg and an operand
 * set, with which tiles, partial blocks, grid and LDS (host arithmetic only; added without a version change).  The compute entry points
 * launch from this plan, and the block-count queries are fields of it for a fixed operand set:
 *   straps_conv_stat_blocks          FP32 route, forward: `blocks` (the fp32 rule reads no operand)
 *   straps_conv_x3_stat_blocks       PLANES, forward, ops = Y | STATS (a training forward): `blocks`
 *   straps_conv_dgrad_x3_bn_blocks   PLANES, data gradient, ops = Y | RES | BNR_RAW: `blocks` (the plane rules' TILE reads no operand either)
 *   straps_conv_x3f_stat_blocks      F32_1X1, forward, ops = Y | STATS: `blocks`
 *   straps_conv_dgrad_x3f_bn_blocks  F32_1X1, data gradient, ops = Y | BNR_RAW: `blocks`.  On this route the tile DOES depend on the operand
 *                                    set (the lean epilogues decide whether the streaming kernel applies): a caller whose launch has another
 *                                    epilogue form than these two sizes its partials with straps_conv_plan.
 *   straps_conv_bf16_tile_choice     BF16, forward, tile_cfg 0: `tile`
 * route / kind: what straps_conv_fwd | _dgrad, ..._x3 (and _x3p, _x3_bits, _x3_bn, _x3_bn_bits), ..._x3f, straps_conv_fwd_bf16 run.
 * ops: the operands of the launch, STRAPS_CONV_OP_* or-ed.  Returns STRAPS_EINVAL (text in straps_last_error) for a geometry or a
 * configuration the route refuses.                                                                                              */
#define STRAPS_CONV_ROUTE_F32 0
#define STRAPS_CONV_ROUTE_PLANES 1
#define STRAPS_CONV_ROUTE_F32_1X1 2
#define STRAPS_CONV_ROUTE_BF16 3
#define STRAPS_CONV_KIND_FWD 0
#define STRAPS_CONV_KIND_DGRAD 1
#define STRAPS_CONV_FAMILY_IGEMM_F32 0   /* conv_igemm_kernel<bm, bn> */
#define STRAPS_CONV_FAMILY_PLANE_IM2COL 1 /* conv_igemm_x3_kernel, tile 1..12 of csrc/conv_plan.h */
#define STRAPS_CONV_FAMILY_PLANE_HALO 2  /* conv_igemm_x3h_kernel, tile = form 1..3 */
#define STRAPS_CONV_FAMILY_F32OP_TILE 3  /* conv_igemm_x3f_kernel, tile 1 | 2 */
#define STRAPS_CONV_FAMILY_F32OP_STREAM 4 /* conv1x1_stream_kernel, tile 5, bn = 256 | 128 | 64 */
#define STRAPS_CONV_FAMILY_BF16_IM2COL 5 /* conv_igemm_x3_kernel with PL chunks per stage, tile 1..8 */
#define STRAPS_CONV_FAMILY_BF16_HALO 6   /* conv_igemm_x3h_kernel with PL chunks per stage, tile 9 | 10 */
#define STRAPS_CONV_OP_Y 1         /* fp32 result / dx */
#define STRAPS_CONV_OP_STATS 2     /* statistics partials */
#define STRAPS_CONV_OP_SCALE 4     /* folded BatchNorm scale / shift */
#define STRAPS_CONV_OP_RELU 8
#define STRAPS_CONV_OP_RES 16      /* residual / addend */
#define STRAPS_CONV_OP_RES_BITS 32 /* ReLU bits masking the addend */
#define STRAPS_CONV_OP_BNR_RAW 64  /* fused BatchNorm-backward sums */
#define STRAPS_CONV_OP_BNR_OUT 128 /* ... with their mask as an fp32 tensor */
#define STRAPS_CONV_OP_YPLANES 256 /* the result as bf16 plane(s) */
#define STRAPS_CONV_OP_A_SCALE 512 /* BatchNorm in the operand path (F32_1X1) */
typedef struct straps_conv_plan_t {
    int32_t family;
    int32_t tile;         /* the route's tile number after its rule (tile_cfg & 15 numbering; halo families: the form) */
    int32_t bm, bn;       /* rows (output pixels) x output channels of a workgroup's tile */
    int32_t epilogue;     /* 0 shared, 1 lean forward, 2 lean data gradient, 3 bf16 plane */
    int32_t abn;          /* BatchNorm in the operand path */
    int32_t ncls;         /* sub-problems of the launch: 1, or the output-parity classes of a stride-2 data gradient */
    int32_t mt[4];        /* M tiles per class */
    int32_t nt;           /* N tiles */
    int32_t part_base[4]; /* first partial block (statistics / BatchNorm-backward sums) of each class */
    int32_t blocks;       /* partial blocks = sum of mt */
    int32_t grid_x, grid_y, threads;
    int32_t lds_bytes;    /* dynamic LDS of the launch */
} straps_conv_plan_t;
int straps_conv_plan(int route, int kind, int ops, int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad,
                     int tile_cfg, straps_conv_plan_t* out);
/* stem weight gradient straight from the NCHW input (its data gradient: straps_stem_dgrad below). */
size_t straps_stem_wgrad_workspace_bytes(int batch, int cin, int h, int w);
int straps_stem_wgrad(const float* x_nchw, const float* dy_nhwc, float* dw_oihw, void* workspace,
                      const uint32_t* nzmask /* optional, see straps_stem_fwd */, int batch, int cin,
                      int h, int w, int accumulate, void* stream);
/* stem data gradient (gradient w.r.t. the network input): dx_nchw [batch][cin][h][w] (+)= the gradient of the 7x7 / stride 2 /
 * pad 3 convolution given dy_nhwc [batch][Ho][Wo][64] (Ho = (h-1)/2 + 1, the raw-output gradient the BatchNorm backward writes)
 * and the weight packed by straps_pack_stem_dgrad_weight (straps_stem_dgrad_weight_floats(cin) floats) from OIHW [64][cin][7][7].
 * Dense (no zero skipping); exact fp32 products with fp32 accumulation on the fp32 matrix pipe.  h, w >= 7 (odd sizes allowed),
 * 1 <= cin <= STRAPS_STEM_DGRAD_MAX_CIN, accumulate = 0 (overwrite) or 1 (add).  weight_floats returns 0 for an unsupported cin. */
#define STRAPS_STEM_DGRAD_MAX_CIN 64
size_t straps_stem_dgrad_weight_floats(int cin);
int straps_pack_stem_dgrad_weight(const float* w_oihw, float* w_pk, int cin, void* stream);
int straps_stem_dgrad(const float* dy_nhwc, const float* w_pk, float* dx_nchw, int batch, int cin, int h, int w,
                      int accumulate, void* stream);
/* training-mode BatchNorm backward with the ReLU mask fused: dz = dy * (yact > 0) (yact NULL = no
 * ReLU), dgamma/dbeta, draw = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)); dz_out (optional,
 * may alias dy) receives dz for the skip connection.  When the activation was exactly
 * relu(raw*scale + shift) (no residual), pass yact = NULL and the forward's scale/shift as
 * mask_scale/mask_shift: the mask is then recomputed from raw with the forward's fmaf (bit-identical,
 * one tensor read less); both NULL with yact NULL = no ReLU.
 * `accumulate` (here and in straps_bn_bwd_x3 / _finish_x3 / _pooled[_sparse]) is a flag word: bit 0 = add to dgamma / dbeta,
 * bit 1 = FROZEN statistics (eval-mode BatchNorm, models/resnet.py:47 under .eval(): save_mean / save_invstd are constants, the
 * two mean terms vanish: draw = gamma*invstd*dz; dgamma = sum dz*xhat and dbeta = sum dz as before).                          */
int straps_bn_bwd_blocks(long long rows, int c);
size_t straps_bn_bwd_workspace_bytes(long long rows, int c);
int straps_bn_bwd(const float* dy, const float* yact, const float* raw, const float* save_mean,
                  const float* save_invstd, const float* gamma, const float* mask_scale,
                  const float* mask_shift, float* dgamma, float* dbeta, float* draw, float* dz_out,
                  void* workspace, long long rows, int c, int accumulate, void* stream);
/* The stem's training-mode tail fused (models/resnet.py:146-149 bn1 -> relu -> maxpool, whose activation feeds nothing but
 * the pool): straps_bn_relu_maxpool_fwd = straps_bn_apply(relu, no residual) + straps_maxpool_fwd_idx without ever writing
 * the activation; straps_bn_bwd_pooled = straps_maxpool_bwd + straps_bn_bwd(mask from raw) without ever writing the
 * un-pooled gradient (each element gathers it from the <= 4 windows covering it).  Same arithmetic in the same order as the
 * unfused calls: bit-identical results, 1.3 GB less HBM traffic per B=64 step.  workspace: straps_bn_bwd_workspace_bytes(
 * batch*h*w, c).                                                                                   */
int straps_bn_relu_maxpool_fwd(const float* raw_nhwc, const float* scale, const float* shift,
                               float* y_pool_nhwc, uint8_t* idx, int batch, int h, int w, int c,
                               void* stream);
int straps_bn_bwd_pooled(const float* dy_pool_nhwc, const uint8_t* idx, const float* raw,
                         const float* save_mean, const float* save_invstd, const float* gamma,
                         const float* mask_scale, const float* mask_shift, float* dgamma, float* dbeta,
                         float* draw, void* workspace, int batch, int h, int w, int c, int accumulate,
                         void* stream);
/* straps_bn_bwd_pooled that leaves unwritten what nobody reads: the only consumer of `draw` is straps_stem_wgrad, which visits a
 * 2-row x 32-column tile of it only if some input channel has a non-zero under the tile (its 9 x 72 input patch).
 * straps_stem_tile_activity derives that map (straps_stem_tiles(batch, in_h, in_w) bytes, 1 = read) from the input's non-zero
 * bit map (straps_stem_nzmask); tile_active == NULL writes everything.  dgamma / dbeta are sums over the whole tensor either way;
 * on the proxy representation ~40 % of the tiles are never read (tools/stem_tile_activity.py).                                  */
size_t straps_stem_tiles(int batch, int in_h, int in_w);
int straps_stem_tile_activity(const uint32_t* nzmask, uint8_t* tile_active, int batch, int cin, int in_h,
                              int in_w, void* stream);
int straps_bn_bwd_pooled_sparse(const float* dy_pool_nhwc, const uint8_t* idx, const float* raw,
                                const float* save_mean, const float* save_invstd, const float* gamma,
                                const float* mask_scale, const float* mask_shift, float* dgamma,
                                float* dbeta, float* draw, void* workspace, int batch, int h, int w, int c,
                                int accumulate, const uint8_t* tile_active, void* stream);
/* max-pool forward that also records the arg-max tap (uint8 per element), and its backward.      */
int straps_maxpool_fwd_idx(const float* x_nhwc, float* y_nhwc, uint8_t* idx, int batch, int h,
                           int w, int c, void* stream);
int straps_maxpool_bwd(const float* dy_nhwc, const uint8_t* idx, float* dx_nhwc, int batch, int h,
                       int w, int c, void* stream);
int straps_gap_bwd(const float* dfeat, float* dx_nhwc, int batch, int hw, int c, void* stream);
/* y[m][n] (+)= x[m][n] * (mask[m][n] > 0)        (ReLU backward on small matrices)                */
int straps_masked_copy(const float* x, int ldx, const float* mask, int ldmask, float* y, int ldy,
                       int m, int n, int accumulate, void* stream);
/* gradient of straps_rot6d_fwd: drot [rows*per_row][3][3] -> dx6 [rows][ldd].                    */
int straps_rot6d_bwd(const float* x6, long long ld, int per_row, const float* drot, float* dx6,
                     long long ldd, long long rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Train-step glue: input construction, prediction heads + multi-task loss, Adam.
 * ------------------------------------------------------------------------------------------ */
/* utils/label_conversions.py:48-55 + :90-127 + train loop :178-182 in ONE pass: seg [B,H,W] part
 * ids -> channel 0 = (seg != 0), channels 1..nj = 16x16 truncated Gaussian heat-maps of the
 * (int-truncated) joints2d [B,nj,2]; writes the NCHW network input [B,1+nj,wh,wh].                */
int straps_build_proxy_input(const float* seg, const float* joints2d, float* out_nchw, int batch,
                             int nj, int wh, void* stream);
/* the same with the heat-maps' standard deviation as an argument (utils/label_conversions.py:90: `std`, an integer; the patch is
 * 4 std x 4 std samples of torch.linspace(-2 std, 2 std, 4 std)); straps_build_proxy_input is std = 4, the value of every call site. */
int straps_build_proxy_input_std(const float* seg, const float* joints2d, float* out_nchw, int batch,
                                 int nj, int wh, int std, void* stream);
/* the same, and in the same pass the non-zero bit map of the planes it writes: nzmask[straps_stem_nzmask_words(batch, nj + 1, wh, wh)] ==
 * what straps_stem_nzmask(out_nchw, ...) would read back from them (the 302 MB read of that pass at 64 bodies is not made; cells that cannot
 * intersect a joint's window are written as zeros without evaluating the Gaussian).  wh % 8 == 0. */
int straps_build_proxy_input_nz(const float* seg, const float* joints2d, float* out_nchw, uint32_t* nzmask,
                                int batch, int nj, int wh, int std, void* stream);
/* prediction heads + HomoscedasticUncertaintyWeightedMultiTaskLoss (losses/multi_task_loss.py:76-119,
 * reduction 'mean') fused with its own backward.  From pred joints [B,90,3], cam [B,3] (row
 * stride ld_est) it forms joints2D = orthographic projection of the 17 COCO joints
 * (utils/cam_utils.py:5-26, config.py:27) and joints3D = 14 H36M-LSP joints (config.py:28-32);
 * visibility of the target 2D joints per utils/joints2d_utils.py:23-32.
 * loss_out[0] = total, [1..5] = weighted task losses (verts, joints2D, joints3D, shape, pose),
 * [6..10] = raw MSEs, [11] = number of visible joints.  Gradients: dverts [B,6890,3],
 * djoints [B,90,3], dest [B,ld_est] (cam cols 0..2, shape cols 147..156, rest zero),
 * drot [B,24,3,3], dlogvar[5] (order verts, joints2D, joints3D, shape_params, pose_params).        */
size_t straps_loss_workspace_bytes(long long batch);
int straps_loss_fwd_bwd(const float* pred_verts, const float* pred_joints, const float* est,
                        int ld_est, const float* pred_rot, const float* tgt_verts,
                        const float* tgt_joints2d, const float* tgt_joints3d,
                        const float* tgt_shape, const float* tgt_rot, const float* log_vars,
                        float* loss_out, float* dverts, float* djoints, float* dest, float* drot,
                        float* dlogvar, void* workspace, long long batch, int img_wh, void* stream);
/* data parallel with the GLOBAL visibility-masked mean: the joints2D task's denominator becomes
 * 2 * j2d_count_global[0] * count_scale (device scalar = the job's visible-joint count, count_scale = 1 / world size) instead of
 * this rank's own count -- the average over ranks of loss_out and of every gradient (what the sum all-reduce + 1/world of the
 * step computes) is then the masked mean over the global batch, whatever the split of visible joints between ranks.
 * j2d_count_global = NULL: straps_loss_fwd_bwd.  straps_count_visible gives a rank's own count (as a float, to be sum all-reduced). */
int straps_loss_fwd_bwd_gm(const float* pred_verts, const float* pred_joints, const float* est, int ld_est,
                           const float* pred_rot, const float* tgt_verts, const float* tgt_joints2d,
                           const float* tgt_joints3d, const float* tgt_shape, const float* tgt_rot,
                           const float* log_vars, float* loss_out, float* dverts, float* djoints, float* dest,
                           float* drot, float* dlogvar, void* workspace, long long batch, int img_wh,
                           const float* j2d_count_global, float count_scale, void* stream);
int straps_count_visible(const float* tgt_joints2d, float* out_count, long long batch, int nj, int img_wh,
                         void* stream);
/* row-masked mean-squared error used by the drop-in criterion module (losses/multi_task_loss.py:78-112):
 * out3 = {sum of squares, kept element count, mean}; the target is read as tgt*tgt_scale + tgt_shift
 * (the 2x/256-1 normalisation of :92); row_mask (uint8 per row, may be NULL) is labels['vis'].
 * workspace: 512 floats.  straps_mse_bwd: grad = coef[0] * (pred - target) on kept rows.             */
int straps_mse_fwd(const float* pred, const float* tgt, const uint8_t* row_mask, long long rows,
                   int cols, float tgt_scale, float tgt_shift, float* out3, void* workspace,
                   void* stream);
int straps_mse_bwd(const float* pred, const float* tgt, const uint8_t* row_mask, long long rows,
                   int cols, float tgt_scale, float tgt_shift, const float* coef, float* grad,
                   void* stream);
/* random_remove_bodyparts + random_occlude (augmentation/proxy_rep_augmentation.py:52-101) in one
 * pass over the part-id segmentation [B,wh,wh]: uniforms [B][9] in [0,1) (6 part-removal draws,
 * 1 occlusion draw, 2 box-centre draws), remove_prob[6] device array.                              */
int straps_augment_seg(const float* seg, const float* uniforms, const float* remove_prob,
                       float occlude_prob, int box_dim, float* out, int batch, int wh, void* stream);
/* ------------------------------------------------------------------------------------------
 * Random draws + the augmentations that consume them (train loop :121-129,146-151,173-175).  The reference mixes
 * torch's device generator and numpy's host generator; here ONE counter-based generator (Philox4x32-10, 10 rounds,
 * key = seed, counter = {index/4, step, sub-stream}) fills draw buffers on the device.  `step_dev` (optional device
 * int64) overrides step_host so a replayed hipGraph advances the sequence with straps_counter_add.
 * Range / scale parameters of the augmentations are doubles -- the reference's Python scalars: (h - l) is formed in double
 * and rounded once to the fp32 scalar its tensor expression uses, so results are bit-identical given the draws.
 * kind 0: uniform [0,1) = (x >> 8) * 2^-24;  kind 1: standard normal (Box-Muller on consecutive pairs).
 * ------------------------------------------------------------------------------------------ */
int straps_philox_fill(unsigned long long seed, const long long* step_dev, long long step_host,
                       unsigned substream, float* out, long long n, int kind, void* stream);
/* counters[i] += delta for i < n (device int64: the generator's step, Adam's step, the BatchNorm num_batches_tracked row) */
int straps_counter_add(long long* counters, int n, long long delta, void* stream);
/* dst[i] = src[index[i]], i < n (device index array): the step keeps the five loss log-variances in the kernel's task
 * order while the parameters sit in the criterion's registration order (losses/multi_task_loss.py:46-55).            */
int straps_gather_f32(const float* src, const int* index, float* dst, int n, void* stream);
/* hipMemsetAsync(ptr, 0, bytes) on `stream` (the step zeroes its flat gradient buffer with it) */
int straps_memset_zero(void* ptr, size_t bytes, void* stream);
/* augment_smpl (augmentation/smpl_augmentation.py:27-61) + the dataset gather in front of it:
 * body b takes pose_rows[b] ([n_rows][72] axis-angle, global orientation first), or with u_index [B] in [0,1) the
 * row floor(u * n_rows) of a resident pose pool (stand-in for data/synthetic_training_dataset.py);
 * out_rotmats [B][24][3][3] = batch_rodrigues of it (joint 0 = glob_rotmats, 1..23 = pose_rotmats);
 * out_shape [B][10]: shape_mode 0 = orig_shape, 1 = shape_draws * std_vector + mean_shape (normal_sample_shape :18-25,
 * shape_draws ~ N(0,1)), 2 = (range_hi - range_lo) * shape_draws + range_lo + mean_shape (uniform_sample_shape :6-15,
 * shape_draws ~ U[0,1)).  out_pose (optional [B][72]) receives the gathered axis-angle rows.                   */
int straps_augment_smpl(const float* pose_rows, long long n_rows, const float* u_index,
                        const float* orig_shape, const float* mean_shape, const float* shape_draws,
                        int shape_mode, const float* std_vector, double range_lo, double range_hi,
                        float* out_shape, float* out_rotmats, float* out_pose, long long batch,
                        void* stream);
/* augment_cam_t (augmentation/cam_augmentation.py:4-14): out[:, :2] = mean[:, :2] + normals_xy [B][2] * xy_std,
 * out[:, 2] = mean[:, 2] + (z_hi - z_lo) * uniform_z [B] + z_lo.                                               */
int straps_augment_cam_t(const float* mean_cam_t, const float* normals_xy, const float* uniform_z,
                         double xy_std, double z_lo, double z_hi, float* out_cam_t, long long batch,
                         void* stream);
/* random_joints2D_deviation (augmentation/proxy_rep_augmentation.py:25-49) on [B][17][2] COCO joints:
 * out = joints + (hi - lo) * u + lo, the hip joints 11 and 12 with their own range; uniforms [B][17][2].        */
int straps_deviate_joints2d(const float* joints2d, const float* uniforms, double lo, double hi,
                            double hip_lo, double hip_hi, float* out, long long batch, void* stream);
/* random_verts2D_deviation (augmentation/proxy_rep_augmentation.py:5-22) as a materialised copy: out [n][3] = verts with
 * x,y += (hi - lo) * u + lo, uniforms [n][2].  (The training step does not call this: straps_rasterize_parts applies the
 * same noise inside its projection kernel.)                                                                     */
int straps_deviate_verts2d(const float* verts, const float* uniforms, double lo, double hi, float* out,
                           long long nverts_total, void* stream);
/* target-side heads of the train step (train loop :138-143): joints3d [B,14,3] = H36M-LSP subset of
 * joints [B,90,3]; joints2d [B,17,2] = perspective projection of the COCO subset with identity
 * rotation, translation cam_t [B,3] and intrinsics fx,fy,cx,cy (utils/cam_utils.py:40-71).         */
int straps_project_targets(const float* joints, const float* cam_t, float fx, float fy, float cx,
                           float cy, float* joints2d, float* joints3d, long long batch, void* stream);
/* renderers/nmr_renderer.py:84-100 (NMRRenderer.forward, rend_parts_seg=True; train loop :155): body-part id per pixel.
 * neural_renderer's 'projection' camera (x_cam = R v + t, pin-hole K, NDC, flipped v axis), pixel-centre sampling,
 * two-sided faces, nearest depth in (near, far), lower face id on ties, final vertical flip; the texture + cube_parts
 * decode of get_parts is the per-face table face_parts (0..255).  verts [B][nverts][3], faces [nfaces][3],
 * cam_K / cam_R [3][3] shared (cam_per_body = 0) or [B][3][3], cam_t [B][3].  parts [B][wh][wh] float part ids
 * (0 = background) and/or depth [B][wh][wh] (`far` where empty); either may be NULL.  Deterministic.             */
size_t straps_rasterize_workspace_bytes(long long batch, int nverts, int wh);
int straps_rasterize_parts(const float* verts, const int32_t* faces, const uint8_t* face_parts,
                           const float* cam_K, const float* cam_R, const float* cam_t, float* parts,
                           float* depth, void* workspace, long long batch, int nverts, int nfaces, int wh,
                           int cam_per_body, float near, float far, const float* vert_noise_u, double noise_lo,
                           double noise_hi, void* stream);
/* (vert_noise_u: NULL, or uniforms [B][nverts][2] in [0,1): the rendered copy of the mesh gets x,y += (hi-lo)*u + lo --
 *  random_verts2D_deviation, augmentation/proxy_rep_augmentation.py:5-22, train loop :146-151 -- inside the projection
 *  kernel; the caller's vertices, i.e. the loss targets, are not touched.)                                        */
/* On-device bounding-box crop + nearest-neighbour resize (utils/image_utils.py:44-105,
 * train loop :161-170): per sample, box of the non-zero pixels of seg [B,wh,wh] -> centre / max(h,w) * scale
 * (scale = orig_scale_factor + U(delta_scale), centre += U(delta_centre); uniforms [B][3] in [0,1), NULL = no
 * jitter) -> int16-truncated corners -> crop -> resize to out_wh with cv2.INTER_NEAREST index rule; joints are
 * shifted by the top-left corner and scaled by out_wh / crop size.  boxes [B][6] receives {r0,c0,r1,c1,shift_r,shift_c}.
 * The scale / range parameters are doubles: the box arithmetic is the reference's float64 arithmetic on the given draws.  */
int straps_crop_resize(const float* seg, const float* joints2d, const float* uniforms,
                       double orig_scale_factor, double delta_scale_lo, double delta_scale_hi,
                       double delta_centre_lo, double delta_centre_hi, float* out_seg,
                       float* out_joints2d, int* boxes, int batch, int wh, int out_wh, int nj,
                       void* stream);
/* The predict-side front end (csrc/predict.hip; predict/predict_3D.py:116-126 for a batch): detector silhouettes and 2-D keypoints ->
 * the regressor's proxy input, as crop_and_resize_silhouette_joints (utils/image_utils.py:108-163) + create_proxy_representation
 * (predict_3D.py:67-76) + the numpy convert_2Djoints_to_gaussian_heatmaps (utils/label_conversions.py:58-87) compute it per image.
 *   sil [B][h][w] uint8 (0 = background), joints2d [B][nj][ld_joint] fp32 with columns (x, y, ...): ld_joint >= 2, later columns (a
 *   confidence) are skipped; gauss_patch [4*std][4*std] fp32, the reference's truncated Gaussian, supplied by the caller (predict.py
 *   heatmap_patch builds it with the reference's own float64 numpy expressions, which makes the heat maps bit-identical; the library
 *   evaluates no exp);  out_nchw [B][1+nj][out_wh][out_wh], out_joints2d [B][nj][2], boxes [B][6] = {wr0, wc0, wr1, wc1, valid, 0}.
 * Per sample, box arithmetic in double, unfused:
 *   window: (rmin, rmax, cmin, cmax) over sil != 0; centre ((rmin+rmax)/2.0, (cmin+cmax)/2.0); side = max(rmax-rmin, cmax-cmin) *
 *     bbox_scale_factor; (wr0, wc0, wr1, wc1) = int16 truncation toward zero of (cr - side/2, cc - side/2, cr + side/2, cc + side/2),
 *     NOT clamped (straps_crop_resize clamps); ch = wr1 - wr0, cw = wc1 - wc0.  Rows [wr0, wr1) x cols [wc0, wc1) are read with zeros
 *     outside the frame: the reference's crop of the clamped box followed by copyMakeBorder.
 *   channel 0: out[y][x] = (float)sil[wr0 + sy][wc0 + sx] or 0 outside the frame, sy = min(floor(y * (1.0 / ((double)out_wh / ch))),
 *     ch - 1), sx likewise with cw (cv2.INTER_NEAREST as OpenCV computes it); the value passes through.
 *   joints: x' = (double)((float)x - (float)wc0) * ((double)out_wh / cw), y' with wr0 and ch; out_joints2d = (float)(x', y').
 *   channel 1 + j: the reference's heat map around (int16 truncation of x', of y'): nothing unless both exceed -2 std and stay below
 *     out_wh - 1 + 2 std; rows [max(0, jy - 2 std), min(out_wh - 1, jy + 2 std)) and the same columns receive
 *     gauss_patch[y - jy + 2 std][x - jx + 2 std]; zero elsewhere.
 *   invalid sample (empty silhouette, or ch <= 0 or cw <= 0: the reference raises): valid = 0 and every output element of the sample,
 *     its joints included, is written as 0.
 *   Window or scaled joint values beyond int16 are outside the contract.
 * Every output element is stored exactly once (no memset, no scatter); nothing is allocated or synchronised, so the call can be captured
 * into a hipGraph.  Checked before any HIP call (STRAPS_EINVAL, straps_last_error() names the argument): non-null pointers; batch, h, w,
 * nj, std > 0; h, w < 32768; ld_joint >= 2; out_wh % 4 == 0; out_nchw 16-byte aligned.                                                */
int straps_predict_proxy_input(const uint8_t* sil, const float* joints2d, int ld_joint,
                               const float* gauss_patch, int std, double bbox_scale_factor,
                               float* out_nchw, float* out_joints2d, int32_t* boxes,
                               int batch, int h, int w, int nj, int out_wh, void* stream);
/* On-device evaluation metrics (metrics/train_loss_and_metrics_tracker.py:127-197 +
 * utils/eval_utils.py:7-85): for each sample b, out3[b] = { sum_n |p-t|,
 * sum_n |scale_and_translation_transform(p) - t|, sum_n |procrustes(p) - t| } over npoints 3-D points
 * (6890 vertices -> PVE / PVE-SC / PVE-PA sums, 14 joints -> MPJPE / -SC / -PA sums).                */
int straps_point_metrics(const float* pred, const float* target, float* out3, long long batch,
                         int npoints, void* stream);
/* ---- on-device evaluation (metrics/eval_metrics_tracker.py; csrc/metrics.hip, csrc/eval.hip; added without a version change) ----
 * Every entry below checks its arguments before any HIP call (STRAPS_EINVAL, straps_last_error() names the argument), launches on
 * `stream`, allocates nothing and never synchronises, so it can be captured into a hipGraph.
 *
 * straps_point_align: straps_point_metrics (same kernel, out3 bit-identical) that also writes the transformed predictions, the
 * `return_transformed_points` arrays of update_per_batch: pred_sc [B][npoints][3] = (x - mu1) * (rms2 / rms1) + mu2
 * (scale_and_translation_transform_batch, utils/eval_utils.py:66-85) and pred_pa [B][npoints][3] = s R x + t
 * (compute_similarity_transform, :7-55, det R = +1), each coordinate computed in fp64 and rounded once to fp32.  Each of out3,
 * pred_sc, pred_pa may be NULL (not computed / not written); at least one must be non-NULL.  npoints >= 3.
 * The rotation is built from the two leading singular pairs of the 3x3 cross-covariance K (eigenvectors of K^T K in fp64) and their
 * cross products.  The eigenvectors lose about (sigma1 / sigma2)^2 of fp64's precision, so the result stays within one fp32 ulp of
 * the reference's SVD route while sigma2 / sigma1 >= 5e-5 (asserted on a numpy emulation of the kernel, tests/test_eval_cases_cpu.py)
 * and degrades quadratically below that; towards collinear points (sigma2 -> 0) the reference's answer becomes arbitrary as well.
 * npoints = 3 is no special case: three
 * centred points give a rank-2 K (sigma3 = 0), and the construction never uses sigma3 (tests/test_eval_cases_cpu.py).             */
int straps_point_align(const float* pred, const float* target, float* out3, float* pred_sc,
                       float* pred_pa, long long batch, int npoints, void* stream);
/* Confusion counts of two byte masks per frame (eval_metrics_tracker.py:158-178): pred, target [B][npix] uint8, any non-zero byte
 * is foreground; counts4 [B][4] int32 = { true positives, false positives, true negatives, false negatives }.  Integer arithmetic
 * only: the result is exact and independent of any order, and of what counts4 held before the call.  1 <= npix < 2^31.            */
int straps_silhouette_counts(const uint8_t* pred, const uint8_t* target, int32_t* counts4,
                             long long batch, long long npix, void* stream);
/* Silhouette of a mesh under the weak-perspective camera cam_wp [B][3] = (s, tx, ty) the regressor predicts.
 *   projection, per vertex, fp32, unfused: u = s * (x + tx), v = s * (y + ty)   (utils/cam_utils.py:21-22)
 *   mask [B][wh][wh] uint8: mask[b][r][c] = 1 iff the pixel-centre sample ((2c + 1 - wh) / wh, (2r + 1 - wh) / wh) lies inside the
 *   projection of some face, else 0.  Rows run with +v, no flip: the pixel grid of undo_keypoint_normalisation
 *   (utils/joints2d_utils.py:5-10), on which (u + 1) * wh / 2 is a pixel coordinate.
 *   coverage rule of straps_rasterize_parts: with the edge function e(a, b, p) = (px - ax) * (by - ay) - (py - ay) * (bx - ax), a
 *   sample is inside when e(v1,v2,p), e(v2,v0,p), e(v0,v1,p) are all >= 0 or all <= 0 (two-sided, edges included); faces with
 *   |e(v0,v1,v2)| <= 1e-12 (or NaN) and faces with a vertex index outside [0, nverts) are skipped.  No depth test.
 * verts [B][nverts][3], faces [nfaces][3]; workspace: straps_wp_silhouette_workspace_bytes(batch, nverts) =
 * batch * nverts * 2 * sizeof(float) bytes (the projected vertices), 4-byte aligned.  1 <= wh <= 4096.  Deterministic.             */
size_t straps_wp_silhouette_workspace_bytes(long long batch, int nverts);
int straps_wp_silhouette(const float* verts, const int32_t* faces, const float* cam_wp, uint8_t* mask,
                         void* workspace, long long batch, int nverts, int nfaces, int wh, void* stream);
/* ---- the head of a validation step (train/train_synthetic_otf_rendering.py:313-348 + metrics/train_loss_and_metrics_tracker.py:118-213;
 * csrc/val.hip; added without a version change) ----
 * Forward only: the prediction heads, the five task losses of losses/multi_task_loss.py (reduction 'mean') and the tracker's eleven
 * metric sums of one batch, added to a device-resident accumulator -- a whole validation pass costs one device-to-host copy at its end.
 * Inputs as straps_loss_fwd_bwd's: pred_verts / tgt_verts [B][nverts][3], pred_joints [B][90][3] (the 17 COCO and the 14 H36M-LSP joints
 * are read through the index maps), est [B][ld_est] = (cam s, tx, ty | 144 pose | 10 shape | padding), pred_rot / tgt_rot [B][24][3][3],
 * tgt_joints2d [B][17][2] in pixels, tgt_joints3d [B][14][3], tgt_shape [B][10], log_vars [5] in the kernel's task order (verts, joints2D,
 * joints3D, shape_params, pose_params).  pred_reposed / tgt_reposed [B][nverts][3] may BOTH be NULL.
 * Every sum is taken in fp64 from the fp32 inputs; every stored fp32 value is rounded once.
 *   batch_out [12]     : the layout of straps_loss_fwd_bwd's loss_out -- total, five weighted task losses, five raw MSEs, visible-joint
 *                        count; the joints2D entries (and the total) are NaN when no target joint is visible, as nn.MSELoss on nothing.
 *   per_sample [B][11] : per sample, in the order of metrics.BatchMetrics.KEYS: the three error sums of straps_point_metrics (raw,
 *                        scale-and-translation corrected, Procrustes aligned) for the vertices, the first two for the reposed vertices
 *                        (0 without them), the three for the 14 joints; the sum of squares of the shape difference; of the rotation
 *                        difference; the sum over the 17 joints of the pixel distance after undo_keypoint_normalisation, visible or not.
 *                        A row depends on its own sample only.
 *   acc [24] (doubles) : exactly one addition per slot and call: acc[0..10] += batch * (double)batch_out[0..10] (the tracker's
 *                        loss.item() * num_inputs), acc[11] += batch_out[11], acc[12 + k] += sum over b ascending of
 *                        (double)per_sample[b][k], acc[23] += batch.  The caller zeroes it once.
 * Each of the three may be NULL; at least one must not be.  The values written do not depend on which of the others are given.
 * workspace: straps_val_head_workspace_bytes(batch) bytes, 8-byte aligned.  nverts >= 3, ld_est >= 157, img_wh > 0.
 * Two launches on `stream`; no atomics, so the result does not depend on scheduling.  Arguments are checked before any HIP call
 * (STRAPS_EINVAL, straps_last_error() names the argument); nothing is allocated or synchronised: the call can be captured into a hipGraph. */
size_t straps_val_head_workspace_bytes(long long batch);
int straps_val_head(const float* pred_verts, const float* pred_reposed, const float* pred_joints,
                    const float* est, int ld_est, const float* pred_rot, const float* tgt_verts,
                    const float* tgt_reposed, const float* tgt_joints2d, const float* tgt_joints3d,
                    const float* tgt_shape, const float* tgt_rot, const float* log_vars,
                    float* batch_out, float* per_sample, double* acc, void* workspace,
                    long long batch, int nverts, int img_wh, void* stream);
/* torch.optim.Adam defaults (run_train.py:200-201) over one flat fp32 buffer:
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps);
 * grad_scale multiplies g first (1/world_size after a sum all-reduce).  step_dev (optional device
 * int64) overrides `step` so that the step count can live on the device (straps_counter_add).       */
int straps_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                     long long n, int step, float lr, float beta1, float beta2, float eps,
                     float grad_scale, const long long* step_dev, void* stream);

/* ---- the whole eval-mode regressor in one call (ABI 11; csrc/regressor.hip) -----------------------------------------------------
 * proxy representation -> (camera, pose, shape), models/regressor.py:43-47 under .eval(): the encoder with BatchNorm on its running
 * statistics, then the IEF iterations.  Inference only (no gradients).  The launches are those SingleInputRegressor.eval() makes, with
 * the same arguments (same convolution routes, tile_cfg 0), so the results are bit-identical to the module's.
 *
 * desc: layers 18 | 50; in_channels 1..256; ief_iters 1..64; precision 0 = bf16x3 (ResNet's default conv_precision) | 1 = fp32 |
 *   3 = bf16 (single-product bf16 convolutions, straps_conv_fwd_bf16: inference only -- every train-mode entry point below rejects it;
 *   its prepared buffer holds one weight plane, smaller than precision 0's three).  2 is unassigned and invalid.
 *
 * params: ONE flat fp32 device buffer of straps_regressor_param_floats() floats: every tensor of the regressor's state_dict(), in
 *   its order, flattened row-major, WITHOUT the `num_batches_tracked` entries and WITHOUT the `ief_module.ief_layers.*` aliases of
 *   fc1/fc2/fc3; then the IEF's initial estimate (157 floats: 0.9, 0, 0, mean 6-D pose, mean shape), which is an attribute, not a
 *   state-dict entry.  That is, for resnet18:
 *     image_encoder.conv1.weight [64][in_channels][7][7], image_encoder.bn1.{weight, bias, running_mean, running_var} [64],
 *     per unit (layer1.0, layer1.1, ..., layer4.last): conv1.weight, bn1.{4}, conv2.weight, bn2.{4}, (resnet50: conv3.weight, bn3.{4}),
 *       then downsample.0.weight, downsample.1.{4} where the unit has a projection,
 *     ief_module.fc1.weight [h][f + 157], fc1.bias [h], fc2.weight [h][h], fc2.bias [h], fc3.weight [157][h], fc3.bias [157],
 *     initial estimate [157]                                      (f, h = 512, 512 for resnet18; 2048, 1024 for resnet50).
 *   BatchNorm eps is 1e-5 (nn.BatchNorm2d's default).
 * straps_regressor_prepare: params -> the prepared buffer (straps_regressor_prepared_bytes, 256-byte aligned): folded BatchNorm,
 *   the stem's fragment-order weights, the convolution weights packed for `precision` (bf16x3 planes / KRSC fp32), the IEF packing and
 *   copies of the IEF's other tensors.  It synchronises `stream` before returning; afterwards neither `params` nor host memory is
 *   read.  The prepared buffer does not depend on the batch or the image size.
 * straps_regressor_workspace_bytes: scratch of straps_regressor_fwd_infer for this (batch, h, w) -- a fixed set of slots reused by
 *   every layer, not a sum over layers; 0 for an invalid request.
 * straps_regressor_fwd_infer: x NCHW [batch][in_channels][h][w] -> est [batch][ld_est] (ld_est >= 157: cam 3 | pose 144 | shape 10)
 *   and, if rotmats != NULL, rotmats [batch][24][3][3] = straps_rot6d_fwd of the pose columns.  Everything is enqueued on `stream`:
 *   nothing synchronises or allocates, so the call can be captured into a hipGraph.  workspace (256-byte aligned) of at least
 *   straps_regressor_workspace_bytes(desc, batch, h, w) bytes, checked before any launch; its content on entry does not matter. */
typedef struct {
    int layers;        /* 18 | 50 */
    int in_channels;   /* >= 1 (reference: 1 or 18) */
    int ief_iters;     /* >= 1 (reference: 3) */
    int precision;     /* 0 = bf16x3, 1 = fp32, 3 = bf16 (inference only); 2 is unassigned */
} straps_regressor_desc_t;
size_t straps_regressor_param_floats(const straps_regressor_desc_t* desc);
size_t straps_regressor_prepared_bytes(const straps_regressor_desc_t* desc);
int straps_regressor_prepare(const straps_regressor_desc_t* desc, const float* params, void* prepared, void* stream);
size_t straps_regressor_workspace_bytes(const straps_regressor_desc_t* desc, int batch, int h, int w);
int straps_regressor_fwd_infer(const straps_regressor_desc_t* desc, const void* prepared, const float* x, int batch, int h, int w,
                               float* est, int ld_est, float* rotmats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the train-mode regressor forward and backward (added without a version change; csrc/regressor_train.hip) ---------------------
 * models/regressor.py:43-47 under .train(), differentiated: what SingleInputRegressor's autograd path computes for reg.train(); reg(x);
 * torch.autograd.backward(...), with the module's defaults.  The launches are those the module makes, with the same arguments (same
 * convolution routes, ReLU bits, fused stem tail, tile_cfg 0, weight-gradient splits, batched IEF backward), so the estimate, every
 * gradient and the running statistics are bit-identical to the module's.  desc as above.
 *
 * params: straps_regressor_train_param_floats() floats, exactly torch.cat([p.reshape(-1) for p in regressor.parameters()]):
 *   image_encoder.conv1.weight, bn1.{weight, bias}, per unit conv1.weight, bn1.{weight, bias}, conv2 ..., (resnet50: conv3 ...), then
 *   downsample.0.weight, downsample.1.{weight, bias} where the unit has a projection, then ief_module.fc1.{weight, bias}, fc2.{...},
 *   fc3.{...}.  The library never writes it; it is the first part of a training step's flat parameter buffer, so straps_adam_step
 *   runs over it unchanged.
 * bn_state: straps_regressor_bn_state_floats() floats, running_mean then running_var of every BatchNorm in module order (bn1, then
 *   per unit bn1, bn2, (bn3), downsample.1).  fwd_train updates it in place as nn.BatchNorm2d does in train mode (momentum 0.1,
 *   eps 1e-5, the unbiased batch variance in the running value).  num_batches_tracked belongs to the host.
 * init_est: the IEF's initial estimate, 157 floats.
 * straps_regressor_train_workspace_bytes: the tape (every layer's raw output, statistics, the activations the backward reads, the
 *   IEF's per-iteration activations, the packed weights) plus the backward's scratch, for this (batch, h, w); 0 if invalid.
 * straps_regressor_fwd_train: train-mode forward with batch statistics: x NCHW [batch][in_channels][h][w] -> est [batch][ld_est]
 *   (ld_est >= 157).  It packs the weights for the forward and the data gradient into the workspace (one batched launch) and
 *   records the tape there; the workspace's content on entry does not matter.
 * straps_regressor_bwd: consumes the tape of the immediately preceding fwd_train on the same workspace; `params` and `x` must be
 *   unchanged in between (the caller's contract: it cannot be checked).  dest [batch][ld_dest] (ld_dest >= 157; columns 157 and
 *   above are not read) is the gradient w.r.t. est.  grads (layout of `params`) is OVERWRITTEN, not accumulated; grads == NULL runs
 *   no weight-gradient kernel.  dx != NULL receives the NCHW input gradient (straps_stem_dgrad: in_channels <= 64); asking for it
 *   makes the stem tail's gradient dense, so the stem weight gradient reads every tile.
 * straps_regressor_export_infer_params: params + bn_state + init_est -> the straps_regressor_param_floats() layout of
 *   straps_regressor_prepare (device-to-device copies on `stream`).
 * None of them synchronises or allocates: a fwd_train + bwd pair can be captured into one hipGraph.  Every argument is checked
 * before any HIP call (STRAPS_EINVAL, straps_last_error() names the field).                                                        */
size_t straps_regressor_train_param_floats(const straps_regressor_desc_t* desc);
size_t straps_regressor_bn_state_floats(const straps_regressor_desc_t* desc);
size_t straps_regressor_train_workspace_bytes(const straps_regressor_desc_t* desc, int batch, int h, int w);
int straps_regressor_fwd_train(const straps_regressor_desc_t* desc, const float* params, float* bn_state, const float* init_est,
                               const float* x, int batch, int h, int w, float* est, int ld_est,
                               void* workspace, size_t workspace_bytes, void* stream);
int straps_regressor_bwd(const straps_regressor_desc_t* desc, const float* params, const float* x, int batch, int h, int w,
                         const float* dest, int ld_dest, float* grads, float* dx,
                         void* workspace, size_t workspace_bytes, void* stream);
int straps_regressor_export_infer_params(const straps_regressor_desc_t* desc, const float* params, const float* bn_state,
                                         const float* init_est, float* infer_params, void* stream);

/* ---- gradient exchange of data-parallel training -----------------------------------------------
 * The reference trains on one GPU (run_train.py:23-26) and so has no counterpart; north_star asks for "a single RCCL all-reduce of
 * grads over xGMI per step".  These entry points give a host WITHOUT torch that exchange: the flat fp32 gradient buffer every
 * backward kernel of this library writes into (one buffer, straps_adam_step's `grads`) is summed over the ranks in place.
 * RCCL is resolved at run time: the copy already loaded in the process (a torch host's) is preferred so that communicator handles
 * created by the host are valid here; otherwise librccl.so.1 is loaded.  STRAPS_EUNSUPPORTED when no RCCL can be found.
 *   straps_comm_unique_id : rank 0 generates the 128-byte rendezvous id (ncclGetUniqueId); the host ships it to the other ranks.
 *   straps_comm_init_rank : every rank joins (ncclCommInitRank; collective, blocks until all `nranks` have called it).  One
 *                           communicator per process per GPU; the current HIP device is the one it binds to.
 *   straps_allreduce_grads: in-place sum all-reduce of n floats, enqueued on `stream` (asynchronous like every kernel launch here;
 *                           calls on one communicator must be issued in the same order on every rank).  `comm` may equally be
 *                           an ncclComm_t the host created itself with the same RCCL library.
 *   straps_comm_size      : number of ranks of the communicator (0 on error);  straps_comm_library: which librccl is in use.  */
#define STRAPS_COMM_ID_BYTES 128
int straps_comm_unique_id(void* id128);
int straps_comm_init_rank(const void* id128, int nranks, int rank, void** comm);
int straps_comm_destroy(void* comm);
int straps_comm_size(void* comm);
const char* straps_comm_library(void);
int straps_allreduce_grads(float* flat_g, long long n, void* comm, void* stream);

/* ---- test-time fitting of cam, 6-D pose and shape to 2-D keypoints (csrc/fit.hip; added without a version change) ----------------
 * The reference stops at the regressor's answer (predict/predict_3D.py:116-149); this is the optimisation users of an HMR-family
 * regressor run after it, as ONE kernel launch that holds all iterations: one wave per body, parameters and Adam moments in registers.
 *
 * A body's row est[157] is the regressor's: cam = [s, tx, ty] | x6[144] | beta[10].  With a prior centre est0[157]:
 *   R_j  = Gram-Schmidt of x6[6j..6j+5], exactly straps_rot6d_fwd (interleaved layout, 1e-12 clamps);
 *   X_k  = kinematic posed joint kp_src[k] (0..23), or tracked mesh vertex kp_src[k] - 24 after the full LBS (template, shape
 *          directions, pose correctives, dense skinning): the values straps_smpl_fwd writes to joints rows 0..23 / to its vertex rows;
 *   p_k  = s (X_k.x + tx, X_k.y + ty);   that_k = 2 t_k / img_wh - 1 (t_k the pixel target);   r2_k = |p_k - that_k|^2;
 *   w_k  = conf_k^2 when conf_k is finite and > 0 and t_k is finite, else 0 (the residual is then not evaluated); conf == NULL: all ones;
 *   rho(r2) = sigma^2 r2 / (sigma^2 + r2) for robust_sigma > 0, else r2;
 *   E    = sum_k w_k rho(r2_k) + lambda_pose |x6 - x6_0|^2 + lambda_shape |beta - beta_0|^2      (per body; no batch mean).
 * g = dE/dest exactly.  Adam per element, the formula of straps_adam_step (bias corrections in double, b^t by squaring) with t = step0 + i + 1 and the learning rate of the
 * element's block (lr_cam, lr_pose, lr_shape).  iters = n: evaluate (E_i, g_i) at est_i and update, i = 0..n-1, then evaluate once more
 * at est_n (n + 1 evaluations, n updates; iters = 0 is a pure evaluation and leaves est and the moments bit-identical).  No early stop.
 *   est         in: the start; out: est_n.                 est0: the prior centre; NULL = est as given; its cam columns are never used.
 *   exp_avg(_sq) Adam moments, in/out; both NULL = start at zero, not stored.  A call split in two with the moments and step0 carried
 *               over is bit-identical to the whole.
 *   energy      [batch][iters + 1]: E_i of every evaluation, or NULL.      grad: g at the last evaluation, or NULL.
 *   best_est / best_energy: the iterate of the smallest E_i (the first one; a NaN never replaces what is held), or NULL.
 *   kp2d        [batch][n_kp][2]: p_k at the last evaluation, or NULL.
 * vert_dirs rows are the blend directions of a tracked vertex in the column order of STRAPS_SMPL_KP (0 template, 1..10 shape,
 * 11..217 pose correctives, 218..223 zero).  j_template, j_shapedirs, vert_dirs and vert_w must be 16-byte aligned.  Out-of-range
 * entries of parents / kp_src are clamped into range on the device.  Results are bit-reproducible and a body's result depends on
 * nothing but that body's inputs.  Arguments are checked before any HIP call; no workspace, no allocation, never synchronises.  */
typedef struct {
    const float* j_template;    /* [24][3], as straps_smpl_model_t                          */
    const float* j_shapedirs;   /* [24][3][10]                                               */
    const int32_t* parents;     /* [24]                                                      */
    const float* vert_dirs;     /* [n_verts][3][224]: D[k] of the tracked vertex, k as STRAPS_SMPL_KP
                                   (0 template, 1..10 shape, 11..217 pose, 218..223 zero)    */
    const float* vert_w;        /* [n_verts][24] dense skinning weights                      */
    const int32_t* kp_src;      /* [n_kp]: 0..23 kinematic joint, 24+i tracked vertex i      */
    int32_t n_verts;            /* 0..16 */
    int32_t n_kp;               /* 1..32 */
} straps_fit_model_t;
typedef struct {
    int32_t iters, step0;       /* 0 <= iters <= 10000 */
    float lr_cam, lr_pose, lr_shape, beta1, beta2, eps;
    float robust_sigma, lambda_pose, lambda_shape, img_wh;
} straps_fit_opts_t;
int straps_fit_keypoints(const straps_fit_model_t* model, const straps_fit_opts_t* opts,
        float* est /*[B][157] in/out*/, const float* est0 /*[B][157]; NULL = est as given*/,
        const float* targets /*[B][n_kp][2] px*/, const float* conf /*[B][n_kp] or NULL*/,
        float* exp_avg, float* exp_avg_sq /*[B][157] in/out; both NULL = start at zero, not stored*/,
        float* energy /*[B][iters+1] or NULL*/, float* grad /*[B][157] at the last evaluation, or NULL*/,
        float* best_est /*[B][157] or NULL*/, float* best_energy /*[B] or NULL*/,
        float* kp2d /*[B][n_kp][2] normalised projection at the last evaluation, or NULL*/,
        long long batch, void* stream);

/* ---- the silhouette term of test-time fitting (csrc/silfit.hip; added without a version change) -----------------------------------
 * The two-sided point-to-silhouette distance of SMPLify-style fitters: the projected vertices are pulled inside the target mask
 * through a distance field, and the mask's foreground pixels pull their nearest projected vertex towards them.  No rasteriser.
 *
 * Conventions.  Masks are [B][wh][wh] uint8, any non-zero byte is foreground.  The pixel grid is that of straps_wp_silhouette and
 * undo_keypoint_normalisation: a projected point p = (s (x + tx), s (y + ty)) (fp32, unfused) has the grid coordinate
 * g = (p + 1) * wh / 2 - 0.5, so that pixel (r, c) sits at g = (c, r).  Residuals are scaled by 2 / wh: the normalised units of the
 * keypoint term of straps_fit_keypoints.
 *
 * straps_distance_field: d2 [B][wh][wh] int32, d2[b][r][c] = min over the foreground (r', c') of frame b of (r - r')^2 + (c - c')^2
 *   (exact; 0 on the foreground); a frame without foreground gets 2 * wh * wh everywhere, more than any real value.  1 <= wh <= 1024.
 *   No workspace: the column pass writes its result into d2, the row pass finishes it in place.
 *
 * straps_silhouette_energy, per body, fp32, with nl = ceil(wh / lattice):
 *   inside term   q = clamp(g_v, 0, wh - 1) per axis; o = |g_v - q|; cell i = min(floor(q), wh - 2), f = q - i per axis;
 *                 D = bilinear interpolation of sqrtf((float)d2) at the four corners of the cell; rho_v = (D + o) * 2 / wh;
 *                 E_in = (1 / nverts) sum_v rho_v^2.  On a clamped axis the derivative of D is zero and that of o is (g - q) / o; on a free
 *                 axis it is the bilinear derivative of D.
 *   outside term  lattice points a = (lattice * j, lattice * i), i, j = 0 .. nl - 1, valid iff mask[lattice * i][lattice * j] != 0;
 *                 r_a = min_v |g_v - a| over the unclamped g_v, on fp32 squared distances fmaf(dy, dy, dx * dx): the lowest vertex index
 *                 wins among equal ones; h_a = max(0, r_a - tau) * 2 / wh; E_out = (1 / max(1, n_valid)) sum_a h_a^2, whose gradient goes
 *                 to the nearest vertex alone.
 *   empty target  a body with d2[b][0][0] == 2 * wh * wh gets both energies 0, all gradients 0 and nearest -1.
 *   outputs (each may be NULL, at least one must be given): energy2 [B][2] = { E_in, E_out } unweighted; dverts [B][nverts][3] = gradient
 *   of w_in E_in + w_out E_out (the z column is written as 0); dcam [B][3] the same energy's gradient w.r.t. (s, tx, ty); nearest
 *   [B][nl][nl] int32 = the nearest vertex of every lattice point, -1 at invalid points.  cam rows have the stride ld_cam >= 3.
 *   workspace (8-byte aligned): straps_silhouette_energy_workspace_bytes = batch * (16 * (nverts + nl * nl + ceil(nverts / 256)) + 128) bytes, 0
 *   for an invalid request.  2 <= wh <= 1024, lattice >= 1 (above wh - 1: the single point (0, 0)), 1 <= nverts <= 2^20, tau >= 0.
 *
 * straps_fit_adam: the update step of a fit loop composed of entry points.  Per body
 *   g = g_kp [157] + (dcam [3] | dx6 [144] | dbetas [10])   (each of the four may be NULL = zero; nothing is added for a NULL),
 *   E = fmaf(w_out, E_out, fmaf(w_in, E_in, e_kp))          (e_kp [B] NULL = 0; energy2 [B][2] NULL: E = e_kp),
 *   then Adam per element with the learning rate of the element's block and exactly the formula of straps_fit_keypoints (bias
 *   corrections in double, b^t by squaring, t = step + 1); of opts only lr_*, beta1, beta2 and eps are read.  energy[b * ld_energy + col]
 *   = E and grad [B][157] = g when given.  (best_est, best_energy), given together, hold the best iterate as straps_fit_keypoints keeps
 *   it: with first != 0 they are set, otherwise replaced iff E < best_energy (the first minimum wins, a NaN never replaces what is held).
 *   update == 0 only evaluates: est and the moments stay bit-identical (the final evaluation of a loop).
 *
 * All three check their arguments before any HIP call, launch on `stream`, allocate nothing, never synchronise, use no float atomics
 * and are bit-reproducible; a body's result depends on nothing but that body's inputs.                                              */
typedef struct {
    int32_t wh, lattice;
    float tau, w_in, w_out;     /* tau in pixels */
} straps_silfit_opts_t;
int straps_distance_field(const uint8_t* mask, int32_t* d2, long long batch, int wh, void* stream);
size_t straps_silhouette_energy_workspace_bytes(long long batch, int nverts, int wh, int lattice);
int straps_silhouette_energy(const float* verts, const float* cam, int ld_cam, const uint8_t* mask, const int32_t* d2,
        const straps_silfit_opts_t* opts, float* energy2, float* dverts, float* dcam, int32_t* nearest,
        void* workspace, long long batch, int nverts, void* stream);
int straps_fit_adam(const straps_fit_opts_t* opts, float* est /*[B][157] in/out*/, const float* g_kp, const float* dcam,
        const float* dx6, const float* dbetas, const float* e_kp, const float* energy2, float w_in, float w_out,
        float* exp_avg, float* exp_avg_sq, float* energy, long long ld_energy, long long col, float* grad,
        float* best_est, float* best_energy, int step, int first, int update, long long batch, void* stream);

/* ---- the 3-D scan term of test-time fitting (csrc/scanfit.hip; added without a version change) ------------------------------------
 * The two-sided nearest-point distance between a body and a cloud of 3-D points (a depth camera's or a scanner's): every point pulls
 * its nearest vertex towards it, every vertex is pulled towards its nearest point.  Point to point; no normals, no landmarks, no grid.
 *
 * straps_scan_energy, per body, fp32:
 *   inputs        verts [B][nverts][3]; trans: the body's translation t in the first three floats of a row of stride ld_trans >= 3 (a
 *                 row of est in the scan fit, where t takes the place of the camera); points [B][npoints][3], a point is VALID iff its
 *                 three coordinates are finite -- NaN padding is how a ragged batch is passed.
 *   definitions   X_v = verts_v + t, one rounding per component;  d2(i, v) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with d = X_v - p_i;
 *                 rho(r2) = sigma^2 r2 / (sigma^2 + r2) for sigma > 0, else r2 (the robust kernel of straps_fit_keypoints; sigma in
 *                 metres).  Coordinates are taken to be small enough for every d2 between valid partners to be finite: a partner at an
 *                 infinite d2 does not count as one.
 *   scan to mesh  for every valid point, n_i = the lowest v among the minima of d2(i, .);  E_s2m = (1 / max(1, n_valid)) sum_i
 *                 rho(d2(i, n_i)), whose gradient goes to X_{n_i} alone.
 *   mesh to scan  for every vertex, m_v = the lowest valid i among the minima of d2(., v);  E_m2s = (1 / nverts) sum_v rho(d2(m_v, v)).
 *   partial scans w_m2s == 0 skips the mesh-to-scan search: E_m2s is reported as 0 and nearest_point as -1 (half the time); likewise
 *                 w_s2m == 0 (E_s2m 0, nearest_vertex -1).
 *   empty scan    a body without a valid point gets both energies 0, all gradients 0 and both index lists -1.
 *   outputs (each may be NULL, at least one must be given): energy2 [B][2] = { E_s2m, E_m2s } unweighted; dverts [B][nverts][3] = the
 *   gradient of w_s2m E_s2m + w_m2s E_m2s; dtrans [B][3] = the sum of the dverts rows in a fixed order; nearest_vertex [B][npoints]
 *   int32 = n_i, -1 at invalid points; nearest_point [B][nverts] int32 = m_v.
 *   workspace (16-byte aligned): straps_scan_energy_workspace_bytes = batch * (24 * nverts + 28 * npoints + 16 * ceil(nverts / 256)
 *   + 4 * ceil(npoints / 256) + 16) bytes, 0 for an invalid request.  1 <= nverts <= 2^20, 1 <= npoints <= 2^20, 1 <= batch < 2^19,
 *   sigma >= 0 and both weights >= 0, all three finite.
 *
 * Arguments are checked before any HIP call.  It launches on `stream`, allocates nothing, never synchronises and is capturable; it uses
 * no float atomics (the minima over the tiles of the distance matrix are merged with integer minimum atomics, which no order changes)
 * and is bit-reproducible; a body's result depends on nothing but that body's inputs.                                               */
typedef struct {
    float sigma, w_s2m, w_m2s;  /* sigma in metres */
} straps_scan_opts_t;
size_t straps_scan_energy_workspace_bytes(long long batch, int nverts, int npoints);
int straps_scan_energy(const float* verts, const float* trans, int ld_trans, const float* points, const straps_scan_opts_t* opts,
        float* energy2, float* dverts, float* dtrans, int32_t* nearest_vertex, int32_t* nearest_point,
        void* workspace, long long batch, int nverts, int npoints, void* stream);

/* ---- one body shape per subject across frames (csrc/fit_subjects.hip; added without a version change) ----------------------------
 * straps_fit_adam_subjects: straps_fit_adam with the ten shape coefficients tied across the frames of a subject -- the update step of
 * a fit loop in which several frames show one person.  The arguments it shares with straps_fit_adam mean what they mean there.
 *
 * Subjects and masks.  offsets [G + 1] int32 in DEVICE memory, non-decreasing (the caller's duty; the kernel only clamps): subject s
 *   owns the contiguous rows lo .. hi - 1 with lo = clamp(offsets[s], 0, B), hi = clamp(offsets[s + 1], lo, B).  Rows that no subject
 *   owns are not touched.  frame_mask [B] bytes or NULL: a frame whose byte is 0 does not COUNT towards its subject (NULL: all count).
 * Per frame f (masked frames included): E_f, the gradient columns 0..146 (cam and pose), their moments in exp_avg / exp_avg_sq and
 *   their update are exactly straps_fit_adam's, bit for bit; energy[f * ld_energy + col] = E_f.
 * Shape, per subject: g_s[i] = the sum over the subject's counting frames of t_f[i], where t_f[i] is what straps_fit_adam forms for
 *   column 147 + i (g_kp[f][147 + i] + dbetas[f][i], nothing added for a NULL), and E_s = the sum of the counting frames' E_f;
 *   subject_energy[s * ld_subject + col] = E_s.  Both are fp32 sums in a fixed order: frame j of the subject belongs to partial j % 16,
 *   a partial adds its counting frames in frame order, the partials are added in the order 0..15.  Only real terms are summed (a
 *   partial starts from its first term, not from +0: a -0 stays a -0), so the order depends on the subject's frame count and mask
 *   alone -- not on B, the subject's position or other subjects.  The current shape is read from the subject's FIRST row of est
 *   (precondition: all rows of a subject hold the same shape columns).  With update != 0 the shape gets one Adam step from g_s, the
 *   moments shape_avg[s] / shape_avg_sq[s] [G][10], lr_shape and t = step + 1, by the formula of straps_fit_adam; the ten new values
 *   are written into EVERY row of the subject, masked ones included.  The shape columns of exp_avg / exp_avg_sq are neither read nor
 *   written.  grad [B][157], when given: per-frame values in columns 0..146, g_s in columns 147..156 of every row of the subject.
 * Best iterate, per subject: with first != 0, or when E_s < best_energy[s] (the first minimum wins, a NaN never replaces what is
 *   held), all the subject's best_est rows receive the est rows as they were before the update, and best_energy[s] [G] = E_s.
 * Edge cases.  update == 0 leaves est and all moments bit-identical.  A subject without a counting frame has E_s = 0 and g_s = 0,
 *   and its shape and shape moments are left as they are, bit for bit (its frames' cam and pose are updated as ever).  An empty
 *   subject (lo == hi) writes subject_energy 0 and nothing else.
 * Consequence: if every subject has one frame and shape_avg / shape_avg_sq equal the shape columns of exp_avg / exp_avg_sq, then est,
 *   energy, best_est, best_energy, grad and the cam / pose moments equal straps_fit_adam's bit for bit, and the shape moments equal
 *   that call's shape-column moments.
 * Arguments: as straps_fit_adam, and offsets must not be NULL, 1 <= n_subjects <= batch, update needs shape_avg and shape_avg_sq,
 *   ld_subject >= 1 and 0 <= col < ld_subject when subject_energy is given.
 *
 * straps_subject_mean_rows: out[s][c] = the sum, in the same fixed order, of rows[f * ld + c] over the subject's counting rows,
 *   divided by their number (fp32); with no counting row the plain mean over all rows of the subject; zeros for an empty subject.
 *   1 <= cols <= 64, ld >= cols.
 *
 * Both check their arguments before any HIP call, launch one kernel on `stream` (one workgroup per subject; subjects of hundreds of
 * frames are fine), use no workspace, allocate nothing, never synchronise, use no float atomics, are capturable and bit-reproducible;
 * a subject's result depends on nothing but that subject's inputs.                                                                  */
int straps_fit_adam_subjects(const straps_fit_opts_t* opts, float* est /*[B][157] in/out*/,
        const int32_t* offsets /*DEVICE [G+1]*/, const uint8_t* frame_mask /*[B] or NULL = all count*/,
        const float* g_kp, const float* dcam, const float* dx6, const float* dbetas,
        const float* e_kp, const float* energy2, float w_in, float w_out,
        float* exp_avg, float* exp_avg_sq /*[B][157]*/, float* shape_avg, float* shape_avg_sq /*[G][10]*/,
        float* energy /*[B][ld_energy] per frame, or NULL*/, long long ld_energy, long long col,
        float* subject_energy /*[G][ld_subject] or NULL*/, long long ld_subject,
        float* grad /*[B][157] or NULL*/, float* best_est /*[B][157]*/, float* best_energy /*[G]*/,
        int step, int first, int update, long long batch, long long n_subjects, void* stream);
int straps_subject_mean_rows(const float* rows, long long ld, int cols /*1..64*/, const int32_t* offsets,
        const uint8_t* frame_mask, float* out /*[G][cols]*/, long long batch, long long n_subjects, void* stream);

/* ---- shaded picture of a mesh under the weak-perspective camera (csrc/render.hip; added without a version change) -----------------
 * What predict/predict_3D.py:169-178 draws through renderers/weak_perspective_pyrender_renderer.py, for a batch, on the device.  The
 * shading model is Lambert with an ambient term, NOT pyrender's metallic-roughness material: which face a pixel shows is defined
 * exactly below, the colours are this model's, and parity with the reference's pixels is not claimed.
 *
 * Frame and pixel grid: those of straps_wp_silhouette.  Pixel (r, c) samples ((2c + 1 - wh) / wh, (2r + 1 - wh) / wh); rows run with
 * +v, no flip.  The viewer looks along +z: NEARER means SMALLER z (the reference turns the mesh by 180 degrees about x and looks down
 * -z, which is the same picture).  All arithmetic is fp32, unfused, in the order written here.
 *   vertices     p' = R p, each row (R[3r] x + R[3r+1] y) + R[3r+2] z; rotation NULL: p' = p, no multiply; rotation_per_body == 0: one
 *                row-major [3][3] matrix, otherwise [B][3][3].  u = s (x' + tx), v = s (y' + ty) with (s, tx, ty) = cam_wp[b * ld_cam ..].
 *   normals      vertex normal = sum over the incident faces, in the order of the table, of cross(p1' - p0', p2' - p0') (not normalised).
 *                The table is CSR: vf_offsets [nverts + 1] int32, non-decreasing from 0; vf_faces [vf_offsets[nverts]] int32 lists, per
 *                vertex, the faces that hold it, ascending (a face that names a vertex twice is listed once); a face with an index
 *                outside [0, nverts) is not listed.  Built once on the host from `faces`.  A gather: no atomics, bit-reproducible.
 *   coverage     exactly straps_wp_silhouette's rule (two-sided, edges included, |e(v0,v1,v2)| <= 1e-12 or NaN and out-of-range faces
 *                skipped).  Per covered sample w_k = e_k / e(v0,v1,v2), z = (w0 z0' + w1 z1') + w2 z2'; the sample goes to the face with
 *                the smallest z, among equal z to the lowest face id (a 64-bit minimum over (order-preserving key of z, face id): no
 *                dependence on any order).
 *   shading      n = (w0 n0 + w1 n1) + w2 n2 per component with the winning face's weights, divided by sqrtf of its squared length
 *                (nx nx + ny ny) + nz nz; a squared length below 1e-24 (or NaN) gives n = (0, 0, -1).  n is negated iff the z component
 *                (x1' - x0') (y2' - y0') - (y1' - y0') (x2' - x0') of the winning face's own normal is positive -- one decision per
 *                face, after the fallback.  lam = ambient, then lam = lam + intensity_l * max(0, (nx dx + ny dy) + nz dz) for l = 0 ..
 *                n_lights - 1; c_k = colour[k] * min(lam, 1); byte = floor(255 * clamp(c_k, 0, 1) + 0.5).
 *   outputs      rgb [B][wh][wh][3] uint8; mask [B][wh][wh] uint8 (1 covered, 0 not); depth [B][wh][wh] float (z of the winning face,
 *                +inf where nothing covers); face_ids [B][wh][wh] int32 (-1 where nothing covers).  mask, depth and face_ids may be
 *                NULL.  An uncovered pixel takes background[b][r][c][:] (uint8 [B][wh][wh][3]) or, when background is NULL, the
 *                quantised opts->background.
 * light_dir holds unit vectors from the surface towards the light, in this frame (not normalised here).  0 <= n_lights <= 4; ambient
 * finite and >= 0.  workspace (8-byte aligned): straps_render_mesh_workspace_bytes = batch * (8 * wh * wh + 32 * nverts) bytes -- the
 * z-buffer first, then p', (u, v) and the normals -- 0 for a non-positive argument or wh > 4096.  1 <= wh <= 4096, nfaces <= 715827882.
 * Arguments are checked before any HIP call; five launches on `stream`, no allocation, no synchronisation, no floating-point atomics,
 * nothing read that the call has not written: bit-reproducible.                                                                     */
typedef struct {
    float colour[3];
    float ambient;
    float background[3];
    int32_t n_lights;
    float light_dir[12];
    float light_intensity[4];
} straps_render_opts_t;
size_t straps_render_mesh_workspace_bytes(long long batch, int nverts, int wh);
int straps_render_mesh(const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_faces,
        const float* cam_wp, int ld_cam, const float* rotation, int rotation_per_body, const straps_render_opts_t* opts,
        const uint8_t* background, uint8_t* rgb, uint8_t* mask, float* depth, int32_t* face_ids, void* workspace,
        long long batch, int nverts, int nfaces, int wh, void* stream);

/* ---- body measurements of a batch of meshes (csrc/measure.hip; added without a version change) -------------------------------------
 * Volume, surface area, extent along a direction, planar girths and lengths along anchor points, n_meas of them per body, in one call.
 * Vertices and points are read as fp32; every product, sum, division and square root is done in double; each result is rounded to float
 * once.  out [B][n_meas].  Gradients: straps_measure_mesh_bwd below.  A GIRTH is the length of the plane section, and planes and directions are the same for
 * every body of the batch; tape-measure (convex hull) girths and per-body plane normals: straps_measure_tape below.
 *   anchor       a names vertex a of the body when 0 <= a < nverts, points[b][a - nverts] when nverts <= a < nverts + n_points
 *                (points [B][n_points][3], may be NULL when n_points == 0); -1 means "none".
 *   selected     face f is selected iff its three indices lie in [0, nverts) and (part_mask == 0, or face_parts[f] < 32 and bit
 *                face_parts[f] of part_mask is set).  A face with an index out of range is skipped, as straps_render_mesh skips it.
 *                part_mask != 0 with face_parts == NULL is an argument error.  face_parts [nfaces] uint8.
 *   VOLUME       (1/6) * sum over the selected faces of q0 . (q1 x q2), q_i = p_i - c, c = anchor[0] or the origin when it is -1.
 *                Signed: negative for inward-facing winding.
 *   AREA         (1/2) * sum over the selected faces of |(p1 - p0) x (p2 - p0)|.
 *   EXTENT       max_v (dir . p_v) - min_v (dir . p_v) over all nverts vertices; anchors, points and part_mask are not read.  A NaN
 *                among the products makes the result NaN (max and min propagate it).
 *   GIRTH        the plane through o = anchor[0] (required) with normal dir (not normalised here).  d_i = dir . (p_i - o); vertex i is on
 *                the positive side iff d_i >= 0 (a NaN is not).  A selected face contributes iff its three sides are not all equal; then
 *                one vertex a stands alone on its side, and each of the two edges (a, b) from it gives x = p_a + t (p_b - p_a) with
 *                t = d_a / (d_a - d_b); the face adds |x - x'|.  The result is the sum over the faces: 0 (not NaN) when the plane misses
 *                every selected face.  The length per face is continuous in the vertex positions: a vertex at d near 0 is no tie case,
 *                and the anchor vertex itself (d == 0 exactly) counts as positive.
 *   PATH         sum_i |A_(i+1) - A_i| over anchor[0 .. k-1], the leading entries that are not -1, 2 <= k <= 4.
 * Anchors a kind does not read are ignored (VOLUME, GIRTH: anchor[0]; PATH: the leading entries; AREA, EXTENT: none).
 * Limits: 1 <= n_meas <= 32, 1 <= nverts <= 2^20, 0 <= n_points <= 64, 0 <= nfaces <= 715827882; nfaces == 0 (faces may then be NULL)
 * only when no measurement is a VOLUME, AREA or GIRTH.  `meas` is a HOST array, copied by value into the launches.
 * workspace (8-byte aligned): straps_measure_workspace_bytes
 *     = batch * n_meas * 8 * (ceil(nfaces / 512) + 2 * ceil(nverts / 2048)) bytes
 * -- per body one double per measurement and block of 512 faces, then (max, min) per measurement and block of 2048 vertices -- and 0 for
 * an argument outside the limits above.  Two launches on `stream`: workgroups of 512 faces (the corners of a face are loaded once for all
 * measurements) or 2048 vertices of ONE body write partial sums in double, then one thread per (body, measurement) adds them in index
 * order.  Arguments are checked before any HIP call; no allocation, no synchronisation, no floating-point atomics, nothing read that the
 * call has not written: bit-reproducible, and a body's row depends on that body's inputs alone (same bits alone or in a batch; a NaN in
 * one body leaves the others untouched).                                                                                             */
enum { STRAPS_MEASURE_VOLUME = 0, STRAPS_MEASURE_AREA = 1, STRAPS_MEASURE_EXTENT = 2, STRAPS_MEASURE_GIRTH = 3, STRAPS_MEASURE_PATH = 4 };
typedef struct {
    int32_t kind;
    int32_t anchor[4];
    float dir[3];
    uint32_t part_mask;
} straps_measure_t;
size_t straps_measure_workspace_bytes(long long batch, int nverts, int nfaces, int n_meas);
int straps_measure_mesh(const float* verts, const float* points, const int32_t* faces, const uint8_t* face_parts,
        const straps_measure_t* meas, float* out, void* workspace, long long batch, int nverts, int n_points, int nfaces,
        int n_meas, void* stream);

/* ---- tape-measure girths, per-body planes (csrc/measure_tape.hip; added without a version change) -----------------------------------
 * What a tape laid round the body in a plane reads: the perimeter of the CONVEX HULL of the plane section (a tape spans the spine groove
 * and the gap between two thighs; the section length follows them), n_meas of them per body in one call; and the plane's normal may be
 * taken per body from two of its anchors, which is what a posed mesh needs.  out [B][n_meas] float.
 *   anchors, selected faces   exactly as straps_measure_mesh states them above: anchor a is vertex a or points[b][a - nverts]; a face is
 *                selected iff its three indices lie in [0, nverts) and (part_mask == 0, or face_parts[f] < 32 and that bit is set).
 *   arithmetic   vertices and points are read as fp32; every product, sum, division and square root is double; each result is rounded
 *                to float once.
 *   plane        through o = anchor[0] (required).  Normal n = dir (as double) when anchor[1] == -1; otherwise n = A1 - A0, the
 *                difference of THAT body's anchors anchor[1] and anchor[0], each component subtracted in double (dir is not read).
 *                n is not normalised for the side test.  A normal that is zero or has a non-finite component cuts nothing: value 0,
 *                count 0.
 *   section points   GIRTH's: d_i = (n_x (p_i - o)_x + n_y (p_i - o)_y) + n_z (p_i - o)_z; vertex i is positive iff d_i >= 0 (a NaN is
 *                not).  A selected face is CUT iff its three sides are not all equal; then one vertex a stands alone on its side and the
 *                two edges (a, b), (a, c) to the following corners in the face's cyclic order give the face's two section points
 *                x = p_a + t (p_b - p_a), t = d_a / (d_a - d_b), and x' likewise with c.
 *   SECTION      the sum over the cut faces of |x - x'|: GIRTH's value, now with a per-body plane.  0 when nothing is cut.
 *   HULL         Q is the multiset of all section points, two per cut face (a mesh edge that two selected faces share is crossed twice
 *                and appears twice: expected).  Q is expressed in an orthonormal basis (u, v) of the plane built in double from n:
 *                    k = the index of the component of n with the smallest magnitude (the first such on a tie);
 *                    a = e_k x n, i.e. k = 0: (0, -n_z, n_y), k = 1: (n_z, 0, -n_x), k = 2: (-n_y, n_x, 0);   u = a / sqrt(a . a);
 *                    w = n x u;   v = w / sqrt(w . w);      q = (u . (x - o), v . (x - o)), dots summed as (x + y) + z.
 *                The value is the perimeter of the convex hull of Q (invariant under the choice of basis up to rounding): 0 when Q is
 *                empty or all its points coincide; twice the segment's length when Q is collinear (the tape goes there and back); NaN
 *                iff some section point of that (body, measurement) is non-finite, or its count exceeds `capacity` (below).
 *   counts       [B][n_meas] int32 or NULL: the number of section points, 2 x the cut faces, for either kind; always the full count,
 *                whatever `capacity` is.
 *   capacity     the number of section points per (body, measurement) that the workspace holds: 0 means the worst case 2 * nfaces,
 *                otherwise 2 <= capacity <= 2 * nfaces.  A HULL row whose count exceeds it is NaN; SECTION stores nothing and is
 *                unaffected; `counts` tells the caller what happened.
 * Limits, as straps_measure_mesh's: 1 <= n_meas <= 32, 1 <= nverts <= 2^20, 0 <= n_points <= 64, 1 <= batch, batch * n_meas < 2^31,
 * part_mask != 0 needs face_parts; here 1 <= nfaces <= 715827882 and kind is STRAPS_TAPE_HULL or STRAPS_TAPE_SECTION.  anchor[0], and
 * anchor[1] unless it is -1, lie in [0, nverts + n_points).  Every failure is STRAPS_EINVAL before any HIP call and names the argument.
 * `meas` is a HOST array, copied by value into the launches.
 * workspace (8-byte aligned), with cap = capacity, or 2 * nfaces when capacity == 0:
 *     straps_measure_tape_workspace_bytes = batch * n_meas * 8 * (2 + 2 * cap) bytes
 * -- per (body, measurement) two doubles (count, section length) and cap (u, v) pairs -- and 0 for an argument outside the limits above
 * (nverts is not an argument of the size) or a size of 2^62 bytes or more.
 * Two launches on `stream`.  collect: a workgroup per (body, measurement) walks the faces in index order, 256 per trip; a cut face takes
 * its slot from a ballot / popcount prefix in its wave plus the counts of the waves and trips before it, so slot order is face order,
 * without atomics; the SECTION length is added per thread in face order, then in a fixed tree.  hull (launched only when a HULL is
 * asked for): a workgroup per (body, measurement) marches the two monotone chains -- from the lexicographic minimum of (u, v), among the
 * points lexicographically greater than the current one the most clockwise, the farther of collinear ones, by a fixed-tree reduction
 * on coordinates alone, to the lexicographic maximum; the same way back -- and adds the edge lengths in chain order.  Every step moves
 * strictly forward in lexicographic order, so a chain ends after at most `count` steps whatever rounding does to an orientation test.
 * No allocation, no synchronisation, no floating-point atomics, nothing read that the call has not written; capturable;
 * bit-reproducible; a row depends on that body's inputs alone (same bits alone or in a batch; a NaN body leaves the others untouched).
 * Gradients: straps_measure_tape_bwd below. */
enum { STRAPS_TAPE_HULL = 0, STRAPS_TAPE_SECTION = 1 };
typedef struct {
    int32_t kind;
    int32_t anchor[2];
    float dir[3];
    uint32_t part_mask;
} straps_tape_t;
size_t straps_measure_tape_workspace_bytes(long long batch, int nfaces, int n_meas, int capacity);
int straps_measure_tape(const float* verts, const float* points, const int32_t* faces, const uint8_t* face_parts,
        const straps_tape_t* meas, float* out, int32_t* counts, void* workspace, long long batch, int nverts, int n_points,
        int nfaces, int n_meas, int capacity, void* stream);

/* ---- gradients of the body measurements and the energy head of a fit to known measurements (csrc/measure_bwd.hip; added without a
 * version change) ------------------------------------------------------------------------------------------------------------------
 * straps_measure_mesh_bwd: given dout [B][n_meas], the gradient of sum_m dout[b][m] * value_m of straps_measure_mesh w.r.t. the vertices,
 *   dverts [B][nverts][3], and w.r.t. the anchor points, dpoints [B][dpoints_rows][3].  Tape girths (straps_measure_tape): straps_measure_tape_bwd below.
 *   Anchors, selected faces, limits and argument checks are exactly straps_measure_mesh's.  In addition: dout and dverts must not be NULL;
 *   vf_offsets / vf_faces -- the CSR vertex-to-face table of straps_render_mesh above (faces ascending, a face that names a vertex twice
 *   listed once for it, out-of-range faces not listed) -- are required when any measurement reads faces; dpoints_rows >= n_points; dpoints
 *   is required when any anchor that is read is a point (it may be NULL otherwise).  Every failure is STRAPS_EINVAL before any HIP call
 *   and names the argument.
 *   definition   the derivative of the exact-arithmetic function on the branch the forward took at these fp32 inputs: the same side tests
 *                d_i >= 0, the same lone vertex, the same selected faces.  Per selected face and measurement:
 *     VOLUME     d/dq_0 = (q_1 x q_2) / 6, cyclic over the corners; the centre c = anchor[0] receives minus the sum of the three.
 *     AREA       with n = (p1 - p0) x (p2 - p0): d/dp_0 = (n / |n|) x (p2 - p1) / 2, cyclic.  A face with |n|^2 == 0 adds nothing.
 *     GIRTH      the derivative of |x - x'| through t = d_a / (d_a - d_b) w.r.t. the three corners and the anchor o, which enters every
 *                d_i.  A face that is not cut, or whose section length is exactly 0, adds nothing.
 *     EXTENT     +dir * dout to the lowest-index vertex whose dir . p equals the maximum, -dir * dout to the lowest-index vertex that
 *                equals the minimum (one vertex may be both).  A NaN maximum or minimum equals no vertex: nothing is added for it.
 *     PATH       unit segment vectors to the anchors: +(A_j - A_(j-1)) / |.| and -(A_(j+1) - A_j) / |.| at position j, for every position
 *                that names the anchor.  A zero-length segment adds nothing.
 *     A face that names vertex v in several corners adds every one of those corners' gradients to v.  An anchor that is a vertex adds
 *     into that vertex's dverts row; several measurements may share an anchor.
 *   arithmetic   double throughout; each output element is rounded to float once, after all its terms -- anchor terms included -- are
 *                added.  Order of the terms of dverts[b][v]: the incident faces in table order, per face the measurements in index order
 *                (per measurement the corners 0, 1, 2 that name v); then the measurements in index order once more for what v receives
 *                as an anchor or an extreme -- the anchor gradient of a GIRTH or centred VOLUME is the sum over blocks of 512 faces in
 *                block order, each block a fixed tree.  dpoints[b][j]: the measurements in index order.  The order depends on the
 *                topology and the measurement list alone: never on the batch size, the body's position in it, or timing.
 *   outputs      dverts is written whole (+0 for a vertex without a term).  Rows 0 .. n_points - 1 of every body's dpoints are written
 *                whole; rows n_points .. dpoints_rows - 1 are not touched -- a zeroed [B][90][3] buffer can go on to straps_smpl_bwd as
 *                djoints.  dout == 0 is multiplied like any other value (0 * NaN is NaN).
 *   workspace (8-byte aligned): straps_measure_bwd_workspace_bytes
 *       = batch * n_meas * 8 * (3 * ceil(nfaces / 512) + 4 * ceil(nverts / 2048)) bytes, 0 for an argument outside the limits.
 *   Two launches on `stream`.  Blocks of 512 faces (only for a GIRTH or centred VOLUME) and 2048 vertices (only for an EXTENT) of ONE body
 *   write the anchor-gradient partials and (max, min, their lowest indices) in double; then one thread per (body, vertex) gathers: it
 *   walks the vertex's incident faces, loads each face's corners once (four faces in flight) and adds the terms of all measurements, then
 *   its anchor and extreme terms, and stores three floats; one more workgroup per body finishes the points, a thread per row.
 * straps_measure_residual: the energy head of a shape fit to known measurements, one thread per body, fp32, in this order:
 *   per column m = 0 .. n_meas - 1:  w = weights[b][m] (1 when weights is NULL); the column is KNOWN iff the target t is finite and non-zero
 *     and w is finite and > 0.  Known: r = values / t - 1; wr = w * r; e = fmaf(wr, r, e) (e starts at +0); dvalues[b][m] = (2 wr) / t.
 *     Unknown: the value is not read into any result (a NaN there is harmless) and dvalues[b][m] = +0.
 *   prior:  d_i = est[b][147 + i] - est0[b][147 + i], p = fmaf(d_i, d_i, p) for i = 0 .. 9 (p starts at +0);
 *     energy[b] = fmaf(lambda_shape, p, e);  g[b][147 + i] = (2 lambda_shape) * d_i;  g[b][0 .. 146] = +0.
 *   values, targets, dvalues [B][n_meas]; est, est0, g [B][157]; energy [B]; 1 <= n_meas <= 32; lambda_shape >= 0.  energy and g are what
 *   straps_fit_adam takes as e_kp and g_kp.  One launch.
 * Both use no floating-point atomics, no allocation and no synchronisation, read nothing that the call has not written, are capturable
 * and bit-reproducible; a body's rows are the same bits alone or in any batch, and a NaN body leaves the others untouched.            */
size_t straps_measure_bwd_workspace_bytes(long long batch, int nverts, int nfaces, int n_meas);
int straps_measure_mesh_bwd(const float* verts, const float* points, const int32_t* faces, const uint8_t* face_parts,
        const int32_t* vf_offsets, const int32_t* vf_faces, const straps_measure_t* meas,
        const float* dout /*[B][n_meas]*/, float* dverts /*[B][nverts][3]*/,
        float* dpoints /*[B][dpoints_rows][3] or NULL*/, void* workspace,
        long long batch, int nverts, int n_points, int dpoints_rows, int nfaces, int n_meas, void* stream);
int straps_measure_residual(const float* values, const float* targets, const float* weights /*or NULL*/,
        const float* est, const float* est0, float lambda_shape, float* energy, float* dvalues, float* g,
        long long batch, int n_meas, void* stream);

/* ---- gradients of the tape-measure girths (csrc/measure_tape_bwd.hip; added without a version change) ----------------------------------
 * straps_measure_tape_bwd: given dout [B][n_meas], the gradient of sum_m dout[b][m] * value_m of straps_measure_tape w.r.t. the vertices,
 *   dverts [B][nverts][3], and w.r.t. the anchor points, dpoints [B][dpoints_rows][3].  `meas`, `capacity`, anchors, selected faces, limits
 *   and argument checks are exactly straps_measure_tape's (without `out`).  In addition: dout and dverts must not be NULL; vf_offsets /
 *   vf_faces -- the CSR vertex-to-face table of straps_render_mesh, as for straps_measure_mesh_bwd -- are required; dpoints_rows >= n_points;
 *   dpoints is required when anchor[0] or anchor[1] of any measurement is a point (it may be NULL otherwise); accumulate is 0 or 1.
 *   Every failure is STRAPS_EINVAL before any HIP call and names the argument.
 *   definition   the derivative of the exact-arithmetic function on the branch the forward took at these fp32 inputs: the same side tests
 *                d_i >= 0, the same lone vertex, the same selected faces, the same chain of hull corners.
 *     section point   x = p_a + t (p_b - p_a), t = d_a / (d_a - d_b), d_i = n . (p_i - o).  With g the upstream gradient w.r.t. x,
 *                e = p_b - p_a, D = n . e (= d_b - d_a) and s = (g . e) / D:
 *                    dp_a += (1 - t)(g - s n)     dp_b += t (g - s n)     do += s n     dn += -s (x - o)
 *                With a per-body normal (anchor[1] != -1: n = A1 - A0, o = A0): dA1 += dn and dA0 += do - dn.  With a fixed dir, dn is
 *                dropped: there is no gradient w.r.t. dir.
 *     SECTION    a cut face adds |x - x'|: g = +(x - x') / |x - x'| at x and the opposite at x'.  A face whose length is exactly 0 adds
 *                nothing (GIRTH's rule).
 *     HULL       the perimeter is sum_i |h_(i+1) - h_i| over the corners the march took, cyclic, in chain order: the lower chain from the
 *                lexicographic minimum, then the upper chain.  Corner i receives (h_i - h_(i-1)) / |.| + (h_i - h_(i+1)) / |.|, taken in
 *                the plane's basis: g = g_u u + g_v v.  The basis (u, v) is a constant: the perimeter does not depend on it.  Two corners
 *                (a collinear set) give twice the unit vector, by the same formula; no point, or one distinct point, gives nothing.  The
 *                march knows a corner by its coordinates: among the stored section points whose (u, v) equal the corner's (bit for bit,
 *                but -0 equals +0), the one with the LOWEST slot index receives the gradient -- slot order is face order, as in the
 *                forward, point 2 s of slot s on the edge (a, b), point 2 s + 1 on (a, c).
 *     special rows    Unlike straps_measure_mesh_bwd, a (body, measurement) row with dout == +-0 adds NOTHING and is not marched: a fit has
 *                unknown columns, and a NaN value there stays harmless.  A HULL row that is NaN in the forward (a non-finite section point,
 *                or a count above `capacity`) puts, with a non-zero dout, NaN into the three components of the gradient row of its
 *                anchor[0] and adds nothing else.  A normal that cuts nothing (zero, or non-finite) adds nothing.
 *   arithmetic   double throughout; each output element is rounded to float once, after all its terms -- anchor terms included -- are
 *                added.  Order of the terms of dverts[b][v]: the incident faces in table order, per face the measurements in index order,
 *                per measurement the corners 0, 1, 2 that name v, per corner point 0 (the edge (a, b)) then point 1; then the measurements
 *                in index order once more for what v receives as anchor[0] (do - dn, or do), then as anchor[1] (dn).  do and dn of a row are
 *                sums over its cut faces: a SECTION's per thread over the trips of 256 faces in face order, a HULL's per thread over the
 *                slots s = t, t + 256, .. in slot order; then the 64 lanes of a wave in a fixed tree, then the four waves in order.
 *                dpoints[b][j]: the measurements in index order.  The order depends on the topology, the measurement list and that body's
 *                own chain alone: never on the batch size, the body's position in it, or timing.
 *   outputs      accumulate == 0: dverts is written whole (+0 for a vertex without a term); rows 0 .. n_points - 1 of every body's dpoints
 *                are written whole; rows n_points .. dpoints_rows - 1 are not touched.  accumulate == 1: an element becomes
 *                (float)((double)old + sum) -- the tape terms go onto straps_measure_mesh_bwd's output without another pass.
 *   values, counts   [B][n_meas] or NULL: what straps_measure_tape writes to `out` and `counts` at the same arguments, BIT FOR BIT -- how a
 *                caller sees that the same branch was taken.  The call is self-contained: it reads no forward call's workspace.
 *   workspace (8-byte aligned), with cap = capacity, or 2 * nfaces when capacity == 0:
 *       straps_measure_tape_bwd_workspace_bytes = batch * n_meas * 8 * (10 + 4 * cap + ceil(ceil(cap / 2) / 2)) bytes
 *   -- per (body, measurement) ten doubles (count, section length, status, do, dn, one spare), cap (u, v) pairs, cap (g_u, g_v) pairs and
 *   ceil(cap / 2) int32 face indices of the cut slots, padded to a double -- and 0 for an argument outside the limits (nverts included)
 *   or a size of 2^62 bytes or more.  The kernels touch only the slots they fill.
 *   Three launches on `stream` (two without a HULL).  collect: the forward's collect kernel, statement for statement, which also stores
 *   the face index of every cut slot and adds a SECTION's do and dn.  hull: the forward's march with candidates that carry their index
 *   (among equal coordinates the lower index wins); it writes (g_u, g_v) per stored point, zero for a point that is no corner, and adds a
 *   HULL's do and dn over the slots whose points hold a vector.  gather: one thread per (body, vertex) walks the vertex's incident faces
 *   (four in flight), per HULL finds the face's slot by binary search in the row's ascending face-index list, recomputes t, e, D and adds
 *   its terms, then its anchor terms, and stores three floats; one more workgroup per body finishes the points, a thread per row.
 *   No allocation, no synchronisation, no floating-point atomics, nothing read that the call has not written (with accumulate == 1:
 *   besides dverts and dpoints); capturable; bit-reproducible; a body's rows are the same bits alone or in any batch, and a NaN body
 *   leaves the others untouched.                                                                                                      */
size_t straps_measure_tape_bwd_workspace_bytes(long long batch, int nverts, int nfaces, int n_meas, int capacity);
int straps_measure_tape_bwd(const float* verts, const float* points, const int32_t* faces, const uint8_t* face_parts,
        const int32_t* vf_offsets, const int32_t* vf_faces, const straps_tape_t* meas,
        const float* dout /*[B][n_meas]*/, float* dverts /*[B][nverts][3]*/,
        float* dpoints /*[B][dpoints_rows][3] or NULL*/, float* values /*[B][n_meas] or NULL*/, int32_t* counts /*or NULL*/,
        void* workspace, long long batch, int nverts, int n_points, int dpoints_rows, int nfaces, int n_meas, int capacity,
        int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STRAPS_HIP_H */
