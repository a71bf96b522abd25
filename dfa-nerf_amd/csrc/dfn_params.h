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
    // Shared slots.  The launch's variant key (tier, flags: dfn_render_variants.h) says what each union carries; the first member is
    // the meaning under flags 0 / TIER_W128 / TIER_E4M3, and a kernel only reads the members of its own variant.  The block, hence
    // the kernel argument segment of every kernel, keeps its size and offsets: a new variant reuses a slot, it moves nothing.
    // pixel ids of the rays (NULL: ray_begin ... of the frame).  TIER_RAYS, with or without TIER_TRAIN: `rays`, f32
    // [ray_count, 6 * fields] = o_head[3], d_head[3][, o_torso[3], d_torso[3]] (the kernel generates no ray and reads no pixel id)
    union { const int* pix_index; const float* rays; };
    float* rgb_head;
    float* rgb_com;
    // the optional per-sample outputs.  TIER_AUX (writes none): the per-ray aux outputs - f32 form aux_* = [ray_count,2] {acc, depth};
    // u8 route alpha8_* = [ray_count].  TIER_RAYS | TIER_TRAIN (a training launch leaves w_head null and writes no per-sample weights
    // of the head image): `train_bounds`, optional f32 [ray_count,2] = (near, far), NULL = frame.z_near / z_far
    union { float* w_head; float* aux_head; unsigned char* alpha8_head; const float* train_bounds; };
    union { float* w_com; float* aux_com; unsigned char* alpha8_com; };
    union { float* z_out; unsigned short* depth16_head; };                      // TIER_AUX, u8 route: [ray_count]
    int out_u8;                 // rgb_head / rgb_com point at uint8 [ray_count,3]: to8b in the epilogue (HELP:17)
    int reserved0;              // (no kernel reads it; never written)
    // training recorder (all null for inference): per-sample raw outputs and per-field activations / ReLU masks
    // [ray_count][n_coarse + n_fine][8], evaluation order (coarse points, then the fine ones).  TIER_RAYS without TIER_TRAIN (inference:
    // the recorder is off): `bounds`, optional f32 [ray_count,2] = (near, far) per ray; NULL = frame.z_near / z_far
    union { float* samples_out; const float* bounds; };
    // hierarchical training: [ray_count][n_coarse + n_fine] merged rank of every evaluated point.  TIER_AUX, u8 route: depth16_com.
    // TIER_ZVALS (no fine pass, so no ranks): `zvals`, f32 [ray_count][n_coarse], the sample depths of ray r in the launch's ray
    // order, non-decreasing
    union { unsigned char* ranks_out; unsigned short* depth16_com; const float* zvals; };
    void* act_T[2];
    unsigned* masks[2];
    long NP;
    int act_e4m3;               // 16-bit training forward: act_T as MX-fp8 e4m3 instead of MX-fp4 (DFN_TRAIN_ACT_E4M3; the TIER_E4M3 variants)
    int reserved1;              // (no kernel reads it; never written.  Sits in the padding in front of `loss`)
    // training forward with the loss in its epilogue (dfn_train_fwd_loss; losses == null: off)
    DfnTrainLoss loss;
    // debug (dfn_debug_clock_probe): the workgroup in the middle of the grid writes {shader cycles, 100 MHz ticks} of its
    // own lifetime -> the effective shader clock UNDER LOAD of this launch.  Null = off.
    unsigned long long* clock_probe;
};

static_assert(offsetof(RenderArgs, loss) == offsetof(RenderArgs, act_e4m3) + 8, "reserved1 must sit in the padding in front of loss");
// every render kernel's argument segment is this block
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

// (tier, flags): the variant key, one line of dfn_render_variants.h (launch_decoder: flags 0 or TIER_W128).  A key that is not in the
// list is hipErrorInvalidValue
hipError_t launch_render(int tier, int flags, const RenderArgs& A, hipStream_t st);
hipError_t launch_decoder(int tier, int flags, const DecoderArgs& A, hipStream_t st);
// width: 256 = the padded program of every tier; 128 = the 128-wide inference program (DFN_WIDTH_128: f32 / f16 / f16x3)
void program_info(int tier, int field, ProgramInfo* out, int width = 256);
// the launchers of one render variant (dfn_render_kernels.h; instantiated by the variant's object, dfn_render_variant.hip)
template <int TIER, int FLAGS> hipError_t launch_render_tier(const RenderArgs& A, hipStream_t st);
template <int TIER, int FLAGS> hipError_t launch_decoder_tier(const DecoderArgs& A, hipStream_t st);

}  // namespace dfn
