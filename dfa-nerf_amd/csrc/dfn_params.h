// dfn_params.h - kernel argument blocks (internal; the public structs live in include/dfanerf.h)
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>
#include "dfanerf.h"
#include "dfn_layout.h"

namespace dfn {

struct RenderArgs {
    DfnFrame frame;
    const char* wblob[2];       // packed weight streams: head, torso
    int nslab[2];
    const float* bias;          // [head blob | torso blob], global
    const float* bg_f32;
    const unsigned char* bg_u8;
    // pixel ids of the rays - or, in a rays launch (`use_rays` below: the kernel generates no ray and reads no pixel id), the rays
    // themselves in the same slot: f32 [ray_count, 6 * fields] = o_head[3], d_head[3][, o_torso[3], d_torso[3]]
    union { const int* pix_index; const float* rays; };
    float* rgb_head;
    float* rgb_com;
    // the optional per-sample outputs - or, in an aux launch (`aux` below; the two are never combined, and the aux kernels write no
    // per-sample output), the per-ray aux outputs in the same slots: the argument block, hence the kernel argument segment of every
    // kernel, keeps its size and offsets
    // (training launch on caller-supplied rays, `use_rays` == 2: the recorder needs samples_out, so the per-ray `train_bounds` - optional
    // f32 [ray_count,2] = (near, far), NULL = frame.z_near / z_far - ride in the w_head slot, which every training launch leaves null;
    // those kernels write no per-sample weights of the head image)
    union { float* w_head; float* aux_head; unsigned char* alpha8_head; const float* train_bounds; };      // aux: f32 [ray_count,2] {acc, depth}; u8 route: [ray_count]
    union { float* w_com; float* aux_com; unsigned char* alpha8_com; };
    union { float* z_out; unsigned short* depth16_head; };                      // aux, u8 route: [ray_count]
    int out_u8;                 // rgb_head / rgb_com point at uint8 [ray_count,3]: to8b in the epilogue (HELP:17)
    int aux;                    // 1: launch the aux instantiation (render_kernel<TW | TIER_AUX>; inference only) - host-side dispatch only
    // training recorder (all null for inference): per-sample raw outputs and per-field activations / ReLU masks
    // (rays launch - inference, so the recorder is off: `bounds`, optional f32 [ray_count,2] = (near, far) per ray; NULL = frame.z_near / z_far)
    union { float* samples_out; const float* bounds; };         // [ray_count][n_coarse + n_fine][8], evaluation order (coarse points, then the fine ones)
    // hierarchical training: [ray_count][n_coarse + n_fine] merged rank of every evaluated point (aux launch, u8 route: depth16_com)
    // (z launch - inference without a fine pass, so no ranks, and never aux: `zvals`, f32 [ray_count][n_coarse], the sample depths of ray r
    // in the launch's ray order, non-decreasing.  Non-null in a launch that records nothing and is not aux = the z instantiation,
    // render_kernel<TW | TIER_ZVALS>: host-side dispatch reads the pointer, dfn_render.hip)
    union { unsigned char* ranks_out; unsigned short* depth16_com; const float* zvals; };
    void* act_T[2];
    unsigned* masks[2];
    long NP;
    int act_e4m3;               // 16-bit training forward: act_T as MX-fp8 e4m3 instead of MX-fp4 (DFN_TRAIN_ACT_E4M3)
    int use_rays;               // 1: launch the rays instantiation (render_kernel<TW | TIER_RAYS>; inference) - host-side dispatch only
                                // 2: the TRAINING forward on caller-supplied rays (render_kernel<TIER | TIER_RAYS, true, TRAIN>: recorder
                                // on, `train_bounds` above, no loss epilogue - its targets are gathered by pixel id)
                                // (sits in the padding in front of `loss`: the argument block keeps its size and offsets)
    // training forward with the loss in its epilogue (dfn_train_fwd_loss; losses == null: off)
    DfnTrainLoss loss;
    // debug (dfn_debug_clock_probe): the workgroup in the middle of the grid writes {shader cycles, 100 MHz ticks} of its
    // own lifetime -> the effective shader clock UNDER LOAD of this launch.  Null = off.
    unsigned long long* clock_probe;
};

static_assert(offsetof(RenderArgs, loss) == offsetof(RenderArgs, act_e4m3) + 8, "use_rays must sit in the padding in front of loss");
// every render kernel's argument segment is this block: a new variant reuses a slot (the unions above), it moves nothing
static_assert(sizeof(RenderArgs) == 376 && offsetof(RenderArgs, loss) == 320 && offsetof(RenderArgs, clock_probe) == 368, "RenderArgs layout");

struct DecoderArgs {
    const char* wblob;
    int nslab;
    int field;                  // FIELD_HEAD (also listener weights) or FIELD_TORSO
    const float* bias;
    int n_bias;
    const float* points;
    const float* dirs;
    long n_points;
    float* feat;
    float* sigma;
    // training recorder (all null for inference): dfn_decoder_train_fwd
    float* samples;             // [ceil32(n)][8]: (sigma, rgb) in floats 0..3 (head) or 4..7 (torso)
    void* act_T;
    unsigned* masks;
};

// width: 256 = the padded program of every tier; 128 = the 128-wide inference program (DFN_WIDTH_128: f32 / f16 / f16x3)
hipError_t launch_render(int tier, const RenderArgs& A, hipStream_t st, int width = 256);
hipError_t launch_decoder(int tier, const DecoderArgs& A, hipStream_t st, int width = 256);
void program_info(int tier, int field, ProgramInfo* out, int width = 256);
// the launchers of one render variant (dfn_render_kernels.h; instantiated by the variant's object, dfn_render_variant.hip)
template <int TIER, int FLAGS> hipError_t launch_render_tier(const RenderArgs& A, hipStream_t st);
template <int TIER, int FLAGS> hipError_t launch_decoder_tier(const DecoderArgs& A, hipStream_t st);

}  // namespace dfn
