// conv_x3_lean.hip -- the bf16x3 implicit-GEMM kernels of conv_x3_kernels.h instantiated with the LEAN epilogues of conv_igemm.h (round 6): EPI = 1, a
// training step's forward (raw result + statistics partials), EPI = 2, its data gradients (LeanDgradEpilogue: addend with optional ReLU bits, fused
// BatchNorm-backward sums, parity classes of a stride-2 gradient; look-ahead under the last chunk) -- both bit-identical to the shared epilogue's results,
// on the tiles the automatic rule of conv_x3.hip picks.  A translation unit of its own so that the two sets of
// instantiations compile in parallel; the plan decides (conv_plan.h: conv_plan_x3) and conv_x3.hip's dispatch_x3 calls in here.
#include "conv_x3_kernels.h"

namespace {

template <int EPI>
int dispatch_lean(const ConvP& p, const ConvPlan& pl, hipStream_t st) {
    if (pl.q.family == STRAPS_CONV_FAMILY_PLANE_HALO) return launch_x3_tiles<kX3Halo, EPI, 0, 1, 3>(p, pl, st);
    return launch_x3_tiles<kX3Tile, EPI, 0, 3, 5, 7, 9, 11, 12>(p, pl, st);
}

}  // namespace

int straps_internal_dispatch_x3_lean(const void* pv, const ConvPlan& pl, hipStream_t st) {
    const ConvP& p = *static_cast<const ConvP*>(pv);
    return pl.q.epilogue == 1 ? dispatch_lean<1>(p, pl, st) : dispatch_lean<2>(p, pl, st);
}
