// dfn_render_variant.hip - the render / decoder kernels of ONE render variant (templates: dfn_render_kernels.h).
//
// A variant is a precision tier plus a set of flags, and it is one object of the library: the kernels are large, so every variant
// compiles on its own, next to the others.  This file is never compiled as it stands.  For each line of the variant list
// (dfa-nerf_amd/render_variants.sh: name, tier, flags) build.sh writes a stub into the build directory -
//     #define DFN_VARIANT_TIER  <tier>
//     #define DFN_VARIANT_FLAGS (<flags>)
//     #include "dfn_render_variant.hip"
// - named dfn_render_<name>.hip, so that the object and the ISA file kept for the build's checks carry the variant's name.
//
// What a variant holds follows from its flags (launch_render_tier / launch_decoder_tier, dfn_render_kernels.h):
//   0                      render for one and two fields, decoder for head and torso - and, in a trainable tier (f32, bf16), the
//                          training forwards: render_kernel<.., TRAIN = 1, 2>, decoder_kernel<.., REC>
//   TIER_W128              the 128-wide inference program (DFN_WIDTH_128; Prog<TIER, HT = 4>): render and decoder, inference only
//   [TIER_W128 |] TIER_AUX   the render kernels that also write opacity and expected depth (RenderArgs.aux): render only
//   [TIER_W128 |] TIER_RAYS  the render kernels for caller-supplied rays (RenderArgs.use_rays): render only
//   [TIER_W128 |] TIER_ZVALS the render kernels for caller-supplied sample depths (RenderArgs.zvals; coarse-only, 32 ... 192 samples): render only
//   TIER_E4M3              bf16 only: the two training forwards whose recorder writes act_T as MX-fp8 e4m3
//   TIER_RAYS | TIER_TRAIN [| TIER_E4M3]   f32 and bf16: the two training forwards on caller-supplied rays (RenderArgs.use_rays == 2:
//                          render_kernel<TIER | TIER_RAYS, true, TRAIN = 1, 2>); with TIER_E4M3 (bf16) the e4m3 recorder's.  Nothing else
// The other flagged variants exist for the inference tiers (f32, f16, f16x3); bf16 is the training tier.
//
// The library's own list of variants is the dispatch table of dfn_render.hip, which names each variant's two launchers by
// <tier, flags>.  The two lists cannot disagree silently: an entry of the table without an object of exactly that tier and
// those flags is an undefined symbol when the library is linked.
#include "dfn_render_kernels.h"

#if !defined(DFN_VARIANT_TIER) || !defined(DFN_VARIANT_FLAGS)
#error "dfn_render_variant.hip is compiled through a stub that defines DFN_VARIANT_TIER and DFN_VARIANT_FLAGS (build.sh)"
#endif

namespace dfn {
template hipError_t launch_render_tier<DFN_VARIANT_TIER, DFN_VARIANT_FLAGS>(const RenderArgs&, hipStream_t);
template hipError_t launch_decoder_tier<DFN_VARIANT_TIER, DFN_VARIANT_FLAGS>(const DecoderArgs&, hipStream_t);
}  // namespace dfn
