// dfn_render_f16_w128.hip - the 128-wide inference program (DFN_WIDTH_128) of the f16 tier: render / decoder kernels
// (templates: dfn_render_kernels.h, HT = 4)
#include "dfn_render_kernels.h"

namespace dfn {
hipError_t launch_render_f16_w128(const RenderArgs& A, hipStream_t st) { return launch_render_tier_w128<TIER_F16>(A, st); }
hipError_t launch_decoder_f16_w128(const DecoderArgs& A, hipStream_t st) { return launch_decoder_tier_w128<TIER_F16>(A, st); }
}  // namespace dfn
