// dfn_render_f32_w128_rays.hip - the render kernels for caller-supplied rays (TIER_RAYS) of the 128-wide inference program (DFN_WIDTH_128) of the f32 tier
// (templates: dfn_render_kernels.h, HT = 4)
#include "dfn_render_kernels.h"

namespace dfn {
hipError_t launch_render_f32_w128_rays(const RenderArgs& A, hipStream_t st) { return launch_render_tier_rays<TIER_F32, TIER_W128>(A, st); }
}  // namespace dfn
