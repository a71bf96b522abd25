// dfn_render.hip - dispatch of the fused frame renderer and the fused decoder by variant key (tier, flags).
// The kernels are templates in dfn_render_kernels.h; each render variant is an object of its own, compiled from
// dfn_render_variant.hip.  The list of them is dfn_render_variants.h; this file turns it into the lookup table.
#include <hip/hip_runtime.h>
#include "dfn_layout.h"
#include "dfn_mlp.h"
#include "dfn_params.h"

namespace dfn {

// ---- the variant table: one entry per line of dfn_render_variants.h, keyed by (tier, flags) ----
struct Variant {
    int tier, flags;
    hipError_t (*render)(const RenderArgs&, hipStream_t);
    hipError_t (*decoder)(const DecoderArgs&, hipStream_t);
};
static constexpr Variant VARIANTS[] = {
#define DFN_VARIANT(name, tier, flags) {tier, (flags), launch_render_tier<tier, (flags)>, launch_decoder_tier<tier, (flags)>},
#include "dfn_render_variants.h"
#undef DFN_VARIANT
};
static constexpr const Variant* variant(int tier, int flags) {
    for (const Variant& v : VARIANTS)
        if (v.tier == tier && v.flags == flags) return &v;
    return nullptr;
}
static constexpr bool keys_unique() {       // every entry is what the lookup finds for its key: no two entries share one
    for (const Variant& v : VARIANTS)
        if (variant(v.tier, v.flags) != &v) return false;
    return true;
}
static_assert(keys_unique(), "dfn_render_variants.h: two variants with the same (tier, flags)");
// keys that must not exist (the API refuses them before; a launch with one is hipErrorInvalidValue): bf16 is the training tier -
// no aux, rays, z or 128-wide form; the f16 tiers are inference only
static_assert(!variant(TIER_BF16, TIER_AUX) && !variant(TIER_BF16, TIER_RAYS) && !variant(TIER_BF16, TIER_ZVALS) && !variant(TIER_BF16, TIER_W128),
              "bf16: training tier");
static_assert(!variant(TIER_F16, TIER_RAYS | TIER_TRAIN) && !variant(TIER_F16X3, TIER_RAYS | TIER_TRAIN) && !variant(TIER_F16, TIER_E4M3),
              "f16 / f16x3: inference only");

hipError_t launch_render(int tier, int flags, const RenderArgs& A, hipStream_t st) {
    const Variant* v = variant(tier, flags);
    return v ? v->render(A, st) : hipErrorInvalidValue;
}
hipError_t launch_decoder(int tier, int flags, const DecoderArgs& A, hipStream_t st) {
    const Variant* v = variant(tier, flags);
    return v ? v->decoder(A, st) : hipErrorInvalidValue;
}

// the 16-bit tiers share one program (same fragment counts and bias blob)
template <class P> static ProgramInfo info_of(int field) {
    return field == FIELD_TORSO ? ProgramInfo{P::T_FRAGS, P::T_SLABS, P::T_NBIAS} : ProgramInfo{P::H_FRAGS, P::H_SLABS, P::H_NBIAS};
}
void program_info(int tier, int field, ProgramInfo* out, int width) {
    if (width == 128) {             // the 128-wide inference program: fewer fragments, the SAME bias blob
        static_assert(Prog<TIER_F16, 4>::H_FRAGS == 314 && Prog<TIER_F16, 4>::T_FRAGS == 450, "128-wide 16-bit stream");
        static_assert(Prog<TIER_F16X3, 4>::H_FRAGS == 2 * 314 && Prog<TIER_F16X3, 4>::T_FRAGS == 2 * 450, "128-wide f16x3 stream");
        static_assert(Prog<TIER_F32, 4>::H_NBIAS == Prog<TIER_F32>::H_NBIAS && Prog<TIER_F16, 4>::T_NBIAS == Prog<TIER_F16>::T_NBIAS, "bias blob");
        *out = tier == TIER_F16X3 ? info_of<Prog<TIER_F16X3, 4>>(field)
               : tier == TIER_F32 ? info_of<Prog<TIER_F32, 4>>(field) : info_of<Prog<TIER_F16, 4>>(field);
        return;
    }
    // f16x3: the f16 program with two fragments (hi, lo') per k-unit and tile; the same bias blob
    static_assert(Prog<TIER_F16X3>::H_FRAGS == 2 * Prog<TIER_F16>::H_FRAGS && Prog<TIER_F16X3>::T_FRAGS == 2 * Prog<TIER_F16>::T_FRAGS, "f16x3 stream");
    static_assert(Prog<TIER_F16X3>::H_NBIAS == Prog<TIER_F16>::H_NBIAS && Prog<TIER_F16X3>::T_NBIAS == Prog<TIER_F16>::T_NBIAS, "f16x3 bias blob");
    static_assert(Prog<TIER_F16>::H_FRAGS == Prog<TIER_BF16>::H_FRAGS && Prog<TIER_F16>::T_FRAGS == Prog<TIER_BF16>::T_FRAGS, "16-bit tiers");
    *out = tier == TIER_F16X3 ? info_of<Prog<TIER_F16X3>>(field)
           : tier == TIER_F32 ? info_of<Prog<TIER_F32>>(field) : info_of<Prog<TIER_BF16>>(field);
}

}  // namespace dfn
