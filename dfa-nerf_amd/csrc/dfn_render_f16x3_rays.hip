// dfn_render_f16x3_rays.hip - the render kernels for caller-supplied rays (origins, directions, per-ray bounds: TIER_RAYS) of the f16x3 tier
// (templates: dfn_render_kernels.h)
#include "dfn_render_kernels.h"

namespace dfn {
hipError_t launch_render_f16x3_rays(const RenderArgs& A, hipStream_t st) { return launch_render_tier_rays<TIER_F16X3>(A, st); }
}  // namespace dfn
