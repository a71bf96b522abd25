// dfn_render_variant.hip - the render / decoder kernels of ONE render variant (templates: dfn_render_kernels.h).
//
// A variant is a precision tier plus a set of flags, and it is one object of the library: the kernels are large, so every variant
// compiles on its own, next to the others.  This file is never compiled as it stands.  For each line of the variant list
// (dfn_render_variants.h: name, tier, flags - and what the flags mean) build.sh writes a stub into the build directory -
//     #define DFN_VARIANT_TIER  <tier>
//     #define DFN_VARIANT_FLAGS (<flags>)
//     #include "dfn_render_variant.hip"
// - named dfn_render_<name>.hip, so that the object and the ISA file kept for the build's checks carry the variant's name.
// The dispatch table of dfn_render.hip is generated from the same list and names each variant's two launchers by <tier, flags>.
#include "dfn_render_kernels.h"

#if !defined(DFN_VARIANT_TIER) || !defined(DFN_VARIANT_FLAGS)
#error "dfn_render_variant.hip is compiled through a stub that defines DFN_VARIANT_TIER and DFN_VARIANT_FLAGS (build.sh)"
#endif

namespace dfn {
template hipError_t launch_render_tier<DFN_VARIANT_TIER, DFN_VARIANT_FLAGS>(const RenderArgs&, hipStream_t);
template hipError_t launch_decoder_tier<DFN_VARIANT_TIER, DFN_VARIANT_FLAGS>(const DecoderArgs&, hipStream_t);
}  // namespace dfn
