// conv_wgrad_plan.h -- the launch plan of a convolution weight gradient: which kernel, its block, grid, split-K extent, LDS and partials.
// ONE function of the geometry and the operand form fills it; the workspace queries, the route query, straps_conv_wgrad_plan and the three compute
// entry points (conv_wgrad.hip, conv_wgrad_x3f.hip) read it and derive nothing themselves.  tests/conv_cases.py wgrad_plan / wgrad_x3f_plan restate it
// (same field meanings as its WPlan) and tests/test_conv_cases_cpu.py holds the two together.  Plain C++: no HIP types.
#pragma once
#include "../../include/straps_hip.h"

// Compute units of the MI355X.  A constant on purpose, never read from the device: the plan is a pure function of the geometry, which is what lets a
// CPU test and the Python restatement pin it.  The workgroup targets of the split rules are multiples of it.
constexpr int WGRAD_CUS = 256;

constexpr int W3PX = 32 + 112;   // conv_wgrad3x3_kernel, pixels per LDS stage: dy tile + input patch rounded up to whole 16-pixel copy rounds

// geometry member of the kernels' parameter structs (conv_wgrad_kernels.h): per-tap kernels ...
struct WgradTapGeom {
    int B, H, W, Cin, Cout, R, S, stride, pad, Ho, Wo;
    int M, rows_per_split, ct, it;   // ct = Cout/BCO tiles, it = Cin/BCI tiles
};
// ... and halo-patch kernels (3x3, stride 1, pad 1: Ho = H, Wo = W)
struct WgradHaloGeom {
    int H, W, Cin, Cout;
    int cw, cw_log2, rpc;      // chunk geometry: cw columns x rpc rows = 32 (or 64) pixels
    int chunks_per_row, chunk_rows_per_img, nchunks, chunks_per_split, it;
};

struct WgradPlan {
    straps_wgrad_plan_t q;     // what straps_conv_wgrad_plan shows: family, block, tiles, splits, unit, units, taps, LDS and partial bytes
    WgradTapGeom tap;          // the layer (B .. Wo) for every family; M, rows_per_split, ct, it for the per-tap families
    WgradHaloGeom halo;        // halo families only
    int abl;                   // tools build only (STRAPS_WGRAD3_ABL): ablation instantiation of the 64-pixel halo kernel; 0 in the product
};

// form: STRAPS_WG_ROUTE_F32 / _PLANES / _F32_1X1 = what straps_conv_wgrad / straps_conv_wgrad_x3 with planes / straps_conv_wgrad_x3f run.
// STRAPS_OK, or STRAPS_EINVAL (error text set, prefixed by `who`) for a geometry the form refuses.
int straps_internal_wgrad_plan(const char* who, int form, int batch, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, WgradPlan* pl);
