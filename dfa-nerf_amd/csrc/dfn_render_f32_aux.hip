// dfn_render_f32_aux.hip - the aux render kernels (opacity + expected depth next to the RGB: TIER_AUX) of the f32 tier
// (templates: dfn_render_kernels.h)
#include "dfn_render_kernels.h"

namespace dfn {
hipError_t launch_render_f32_aux(const RenderArgs& A, hipStream_t st) { return launch_render_tier_aux<TIER_F32>(A, st); }
}  // namespace dfn
