// dfn_render.hip - tier and width dispatch of the fused frame renderer and the fused decoder.
// The kernels are templates in dfn_render_kernels.h, instantiated per precision tier in dfn_render_{f32,bf16,f16,f16x3}.hip
// and, for the 128-wide inference program (DFN_WIDTH_128), in dfn_render_{f32,f16,f16x3}_w128.hip; the aux instantiations
// (RenderArgs.aux: opacity and expected depth next to the RGB) in dfn_render_{f32,f16,f16x3}[_w128]_aux.hip; the instantiations for
// caller-supplied rays (RenderArgs.use_rays) in dfn_render_{f32,f16,f16x3}[_w128]_rays.hip.
#include <hip/hip_runtime.h>
#include "dfn_layout.h"
#include "dfn_mlp.h"
#include "dfn_params.h"

namespace dfn {

hipError_t launch_render_f32(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_bf16(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16x3(const RenderArgs& A, hipStream_t st);
hipError_t launch_decoder_f32(const DecoderArgs& A, hipStream_t st);
hipError_t launch_decoder_bf16(const DecoderArgs& A, hipStream_t st);
hipError_t launch_decoder_f16(const DecoderArgs& A, hipStream_t st);
hipError_t launch_decoder_f16x3(const DecoderArgs& A, hipStream_t st);
hipError_t launch_render_f32_w128(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16_w128(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16x3_w128(const RenderArgs& A, hipStream_t st);
hipError_t launch_decoder_f32_w128(const DecoderArgs& A, hipStream_t st);
hipError_t launch_decoder_f16_w128(const DecoderArgs& A, hipStream_t st);
hipError_t launch_decoder_f16x3_w128(const DecoderArgs& A, hipStream_t st);
hipError_t launch_render_f32_aux(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16_aux(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16x3_aux(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f32_w128_aux(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16_w128_aux(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16x3_w128_aux(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f32_rays(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16_rays(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16x3_rays(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f32_w128_rays(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16_w128_rays(const RenderArgs& A, hipStream_t st);
hipError_t launch_render_f16x3_w128_rays(const RenderArgs& A, hipStream_t st);

hipError_t launch_render(int tier, const RenderArgs& A, hipStream_t st, int width) {
    if (A.use_rays) {               // first: a rays launch carries `bounds` in the recorder's samples_out slot (bf16: refused by the API)
        switch (tier) {
        case TIER_F32: return width == 128 ? launch_render_f32_w128_rays(A, st) : launch_render_f32_rays(A, st);
        case TIER_F16: return width == 128 ? launch_render_f16_w128_rays(A, st) : launch_render_f16_rays(A, st);
        case TIER_F16X3: return width == 128 ? launch_render_f16x3_w128_rays(A, st) : launch_render_f16x3_rays(A, st);
        default: return hipErrorInvalidValue;
        }
    }
    if (A.aux) {                    // (bf16 has no aux kernels; the API refuses it before)
        switch (tier) {
        case TIER_F32: return width == 128 ? launch_render_f32_w128_aux(A, st) : launch_render_f32_aux(A, st);
        case TIER_F16: return width == 128 ? launch_render_f16_w128_aux(A, st) : launch_render_f16_aux(A, st);
        case TIER_F16X3: return width == 128 ? launch_render_f16x3_w128_aux(A, st) : launch_render_f16x3_aux(A, st);
        default: return hipErrorInvalidValue;
        }
    }
    if (width == 128) {
        switch (tier) {
        case TIER_F32: return launch_render_f32_w128(A, st);
        case TIER_F16: return launch_render_f16_w128(A, st);
        case TIER_F16X3: return launch_render_f16x3_w128(A, st);
        default: return hipErrorInvalidValue;      // (bf16: the training tier stays padded; the API refuses it before)
        }
    }
    switch (tier) {
    case TIER_BF16: return launch_render_bf16(A, st);
    case TIER_F16: return launch_render_f16(A, st);
    case TIER_F16X3: return launch_render_f16x3(A, st);
    default: return launch_render_f32(A, st);
    }
}
hipError_t launch_decoder(int tier, const DecoderArgs& A, hipStream_t st, int width) {
    if (width == 128) {
        switch (tier) {
        case TIER_F32: return launch_decoder_f32_w128(A, st);
        case TIER_F16: return launch_decoder_f16_w128(A, st);
        case TIER_F16X3: return launch_decoder_f16x3_w128(A, st);
        default: return hipErrorInvalidValue;
        }
    }
    switch (tier) {
    case TIER_BF16: return launch_decoder_bf16(A, st);
    case TIER_F16: return launch_decoder_f16(A, st);
    case TIER_F16X3: return launch_decoder_f16x3(A, st);
    default: return launch_decoder_f32(A, st);
    }
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
    if (tier == TIER_F16X3) {       // the f16 program with two fragments (hi, lo') per k-unit and tile; the same bias blob
        using P = Prog<TIER_F16X3>;
        static_assert(P::H_FRAGS == 2 * Prog<TIER_F16>::H_FRAGS && P::T_FRAGS == 2 * Prog<TIER_F16>::T_FRAGS, "f16x3 stream");
        static_assert(P::H_NBIAS == Prog<TIER_F16>::H_NBIAS && P::T_NBIAS == Prog<TIER_F16>::T_NBIAS, "f16x3 bias blob");
        *out = field == FIELD_TORSO ? ProgramInfo{P::T_FRAGS, P::T_SLABS, P::T_NBIAS}
                                    : ProgramInfo{P::H_FRAGS, P::H_SLABS, P::H_NBIAS};
    } else if (tier != TIER_F32) {
        using P = Prog<TIER_BF16>;
        static_assert(Prog<TIER_F16>::H_FRAGS == P::H_FRAGS && Prog<TIER_F16>::T_FRAGS == P::T_FRAGS, "16-bit tiers");
        *out = field == FIELD_TORSO ? ProgramInfo{P::T_FRAGS, P::T_SLABS, P::T_NBIAS}
                                    : ProgramInfo{P::H_FRAGS, P::H_SLABS, P::H_NBIAS};
    } else {
        using P = Prog<TIER_F32>;
        *out = field == FIELD_TORSO ? ProgramInfo{P::T_FRAGS, P::T_SLABS, P::T_NBIAS}
                                    : ProgramInfo{P::H_FRAGS, P::H_SLABS, P::H_NBIAS};
    }
}

}  // namespace dfn
