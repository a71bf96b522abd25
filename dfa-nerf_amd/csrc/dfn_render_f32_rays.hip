// dfn_render_f32_rays.hip - the render kernels for caller-supplied rays (origins, directions, per-ray bounds: TIER_RAYS) of the f32 tier
// (templates: dfn_render_kernels.h)
#include "dfn_render_kernels.h"

namespace dfn {
hipError_t launch_render_f32_rays(const RenderArgs& A, hipStream_t st) { return launch_render_tier_rays<TIER_F32>(A, st); }
}  // namespace dfn
