// dfn_render_f16x3_aux.hip - the aux render kernels (opacity + expected depth next to the RGB: TIER_AUX) of the f16x3 tier
// (templates: dfn_render_kernels.h)
#include "dfn_render_kernels.h"

namespace dfn {
hipError_t launch_render_f16x3_aux(const RenderArgs& A, hipStream_t st) { return launch_render_tier_aux<TIER_F16X3>(A, st); }
}  // namespace dfn
