// dfn_render.hip - tier, width and mode dispatch of the fused frame renderer and the fused decoder.
// The kernels are templates in dfn_render_kernels.h; each render variant (a tier and a set of flags) is an object of its own,
// compiled from dfn_render_variant.hip (its header describes the scheme).  This file holds the library's list of them.
#include <hip/hip_runtime.h>
#include "dfn_layout.h"
#include "dfn_mlp.h"
#include "dfn_params.h"

namespace dfn {

// ---- the variant list: X(tier, flags), one object each (the build's side of it: render_variants.sh) ----
#define DFN_INFERENCE_VARIANTS(X, T) \
    X(T, 0) X(T, TIER_W128) X(T, TIER_AUX) X(T, TIER_W128 | TIER_AUX) X(T, TIER_RAYS) X(T, TIER_W128 | TIER_RAYS) \
    X(T, TIER_ZVALS) X(T, TIER_W128 | TIER_ZVALS)
#define DFN_RENDER_VARIANTS(X) \
    DFN_INFERENCE_VARIANTS(X, TIER_F32) DFN_INFERENCE_VARIANTS(X, TIER_F16) DFN_INFERENCE_VARIANTS(X, TIER_F16X3) \
    X(TIER_BF16, 0) X(TIER_BF16, TIER_E4M3) \
    X(TIER_F32, TIER_RAYS | TIER_TRAIN) X(TIER_BF16, TIER_RAYS | TIER_TRAIN) X(TIER_BF16, TIER_RAYS | TIER_TRAIN | TIER_E4M3)

struct Variant {
    hipError_t (*render)(const RenderArgs&, hipStream_t);
    hipError_t (*decoder)(const DecoderArgs&, hipStream_t);
};
enum Mode { MODE_PLAIN, MODE_AUX, MODE_RAYS, MODE_E4M3, MODE_ZVALS, MODE_RAYS_TRAIN, MODE_RAYS_TRAIN_E4M3, N_MODES };
constexpr int N_TIERS = TIER_F16X3 + 1;
struct VariantTable { Variant at[N_TIERS][2][N_MODES]; };         // [tier][width == 128][mode]; no such variant: null
static constexpr VariantTable make_table() {
    VariantTable t{};
#define X(T, F) \
    t.at[T][((F) & TIER_W128) != 0][(F) & TIER_TRAIN ? ((F) & TIER_E4M3 ? MODE_RAYS_TRAIN_E4M3 : MODE_RAYS_TRAIN) : (F) & TIER_RAYS ? MODE_RAYS : (F) & TIER_ZVALS ? MODE_ZVALS : (F) & TIER_AUX ? MODE_AUX : (F) & TIER_E4M3 ? MODE_E4M3 : MODE_PLAIN] = \
        {launch_render_tier<T, (F)>, launch_decoder_tier<T, (F)>};
    DFN_RENDER_VARIANTS(X)
#undef X
    return t;
}
static constexpr VariantTable TABLE = make_table();
static const Variant* variant(int tier, int width, int mode) {
    if (tier < 0 || tier >= N_TIERS) return nullptr;
    return &TABLE.at[tier][width == 128][mode];
}

hipError_t launch_render(int tier, const RenderArgs& A, hipStream_t st, int width) {
    // rays first: a rays launch carries `bounds` in the recorder's samples_out slot (bf16: refused by the API); then aux (bf16 has no
    // aux kernels; the API refuses it before); then the width (bf16: the training tier stays padded; the API refuses it before).
    // The 16-bit training step with the e4m3 opt-out for act_T: those two kernels are a variant of their own.  A z launch: `zvals` shares
    // the argument slot of the recorder's ranks_out and of the aux route's depth16_com - it is one when neither of those is on.
    // use_rays == 2: the training forward on caller-supplied rays (recorder on, bounds in the w_head slot): variants of their own
    const int mode = A.use_rays == 2 ? (tier == TIER_BF16 && A.act_e4m3 ? MODE_RAYS_TRAIN_E4M3 : MODE_RAYS_TRAIN) : A.use_rays ? MODE_RAYS : A.aux ? MODE_AUX : (!A.samples_out && A.zvals) ? MODE_ZVALS : (tier == TIER_BF16 && A.samples_out && A.act_e4m3) ? MODE_E4M3 : MODE_PLAIN;
    const Variant* v = variant(tier, width, mode);
    return v && v->render ? v->render(A, st) : hipErrorInvalidValue;
}
hipError_t launch_decoder(int tier, const DecoderArgs& A, hipStream_t st, int width) {
    const Variant* v = variant(tier, width, MODE_PLAIN);
    return v && v->decoder ? v->decoder(A, st) : hipErrorInvalidValue;
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
