// dfn_train.h - argument blocks and launchers of the training kernels (dfn_train.hip)
#pragma once
#include <hip/hip_runtime.h>
#include "dfanerf.h"
#include "dfn_layout.h"
#include "dfn_plan.h"      // WOp, WItem, WNItem: the tables the weight-gradient launches read

namespace dfn {

struct MlpBwdArgs {
    const char* wblob_T;        // transposed packed stream of the field
    int nslab;
    const float* samples;       // [NP][8] forward outputs (sigma_h, rgb_h, sigma_t, rgb_t)
    const float* dsamples;      // [NP][8] gradients w.r.t. them
    const unsigned* masks;      // forward ReLU bits of the field
    void* dy_T;                 // out: tile-major [NP/32][rows][32] pre-activation gradients
    long NP;
};

// composite_bwd_kernel: one block for every form.  Which pointers are given says which form is launched (launch_composite_bwd)
struct CompositeBwdArgs {
    DfnFrame frame;
    const int* pix_index;       // pixel-id forms: [rays], or null = ray_begin + ray
    const float* bg_f32;
    const unsigned char* bg_u8;
    const float* samples;       // [rays][S][8], S = n_coarse + n_fine, evaluation order
    const float* d_rgb_head;    // [rays][3]
    const float* d_rgb_com;     // [rays][3] or null
    float* dsamples;            // out [rays][S][8]
    // hierarchical step (n_fine > 0): what the forward left about the merge
    const float* z_all;         // [rays][S] merged, sorted depths
    const unsigned char* ranks; // [rays][S] merged rank of evaluated point i
    float* zero_buf;            // optional: a buffer this launch also fills with zeros ...
    long zero_floats;           // ... and its length
    // the step on caller-supplied rays (pix_index is not read: bg row r is ray r's), what the forward read
    const float* rays;          // [rays][12] = o_head, d_head, o_torso, d_torso (the ray norms come from the directions)
    const float* bounds;        // [rays][2] = (near, far) or null = frame.z_near / z_far (the coarse step's depths)
    float* d_norm;              // rays forms, optional: out [rays][2] = dL/d|d_head| (through the head image's dist = dz |d_head|), dL/d|d_torso|
    const float* d_stats;       // optional: [rays][4] = dL/d(acc_head, depth_head, acc_com, depth_com) of a loss that reads the stats
};
// composite_stats_kernel (opacity and expected depth of the training step; their gradient is d_stats above): one block for all four
// forms (pixel ids | rays + bounds, coarse | hierarchical).  The background is not read
struct CompositeStatsArgs {
    DfnFrame frame;
    const int* pix_index;       // pixel-id form: [rays]
    const float* rays;          // rays form: [rays][12] ...
    const float* bounds;        // ... and [rays][2] or null
    const float* samples;       // [rays][S][8], evaluation order
    const float* z_all;         // hierarchical step: [rays][S] merged depths ...
    const unsigned char* ranks; // ... and [rays][S] ranks
    float* stats;               // out [rays][4] = acc_head, depth_head, acc_com, depth_com
};

// points_grad_kernel (f32 tier): dL/d(point) and dL/d(unit view direction) of every evaluated point of one field, from the arrays a
// backward leaves behind (dy_T: the pre-activation gradients, act_T: the recorded positional encodings) and the flat parameters
struct PointsGradArgs {
    const float* params;        // flat decoder parameters (f32, state_dict order)
    const float* act_T;         // [NP/32][RecMap rows][32]
    const float* dy_T;          // [NP/32][GradMap rows][32]
    float* g_x;                 // out [NP][3]
    float* g_dhat;              // out [NP][3]
    long n_tiles;               // NP / 32
    int w_in, ld_in;            // head / listener: offset and row length of the input layer's weight in `params` (the first 60 columns are used)
    int w_skip, ld_skip;        // ... and of the skip layer's
};
// rays_grad_kernel: the per-ray sums of those (one wave per ray) -> d_rays [rays][12] in the layout of `rays`
struct RaysGradArgs {
    DfnFrame frame;             // ray_count, n_coarse, n_fine, z_near / z_far (bounds == null)
    const float* rays;          // [rays][12]
    const float* bounds;        // [rays][2] or null
    const float* z_all;         // hierarchical step: [rays][S] merged depths ...
    const unsigned char* ranks; // ... and the merged rank of evaluated point j
    const float* g_x[2];        // per field [NP][3], evaluation order
    const float* g_dhat[2];
    const float* d_norm;        // [rays][2]
    float* d_rays;              // out [rays][12]
};

hipError_t launch_mlp_bwd(int tier, int field, const MlpBwdArgs& A, hipStream_t st);
hipError_t launch_mlp_bwd_bf16(bool torso, const MlpBwdArgs& A, hipStream_t st);     // dfn_bwd_bf16.hip
void bwd_program_info(int tier, int field, ProgramInfo* out);
// the compositing family: 32 / 64 / 128 coarse samples and no fine ones, or 64 coarse + 64 / 128 fine ones; fields == 2 wherever rays or
// stats are involved (launch_composite_stats: always).  Anything else: hipErrorInvalidValue
hipError_t launch_composite_bwd(const CompositeBwdArgs& A, hipStream_t st);
hipError_t launch_composite_stats(const CompositeStatsArgs& A, hipStream_t st);
hipError_t launch_points_grad(int field, const PointsGradArgs& A, hipStream_t st);                 // f32 tier; field 0 head, 1 torso, 2 listener
hipError_t launch_rays_grad(const RaysGradArgs& A, hipStream_t st);
// Split-K partials: C [ksplit][c_stride] and dbias [ksplit][n_bias], one writer per element and slice (no atomics);
// launch_reduce_scatter / launch_reduce_bias add the slices in index order (bit-reproducible gradients).
// f32 tier: wgrad_full_kernel + wgrad_narrow_kernel (dfn_plan.h: WNItem)
hipError_t launch_wgrad(int tier, int field, const WOp* ops_dev, const int* full_ops_dev, int n_full, const WNItem* nitems_dev,
                        int n_nitems, const void* dy_T, const void* act_T, long NP, int ksplit, float* C, long c_stride,
                        const int* e_of, float* dbias, int n_bias, hipStream_t st);
// bf16 tier: one workgroup per (GEMM, slice of the points), operands through LDS (dfn_wgrad_bf16.hip); order = GEMMs by
// decreasing size
// act_fp4: act_T is MX-fp4 (recorded by the fused training step) / MX-fp8 e4m3 (by the decoder-on-points recorder)
hipError_t launch_wgrad_bf16(int field, bool act_fp4, const WOp* ops_dev, const WItem* items_dev, int n_items, const void* dy_T,
                             const void* act_T, long NP, float* C, long c_stride, const int* e_of, float* dbias, int n_bias,
                             hipStream_t st);
// grad_flat[map[i]] += sum over the first `slices` slices of parts[.][i]   (i < n; map[i] < 0: structural padding)
hipError_t launch_reduce_scatter(const int* map, const float* parts, long n, long stride, int slices, float* grad_flat,
                                 hipStream_t st);
// launch_reduce_bias + launch_reduce_scatter in one launch (same sums, same order)
// blk_n / bias_n (may be NULL: `slices` everywhere): slices the GEMM owning a 256-element block of C / a bias element was
// split into; `units` = tile pairs of the call - a GEMM split n ways over them fills ceil(units / ceil(units / n)) slices
hipError_t launch_reduce_both(const int* map, const float* parts, long n, long stride, int slices, float* grad_flat,
                              const int* rows, const float* bparts, int n_bias, float* dbias, const unsigned char* blk_n,
                              const unsigned char* bias_n, long units, hipStream_t st);
// dbias[e] = sum over slices of parts[.][e] for the elements that have a gradient row (rows[e] >= 0), 0 otherwise
hipError_t launch_reduce_bias(const int* rows, const float* parts, int n_bias, int slices, float* dbias, hipStream_t st);
constexpr int SAMPLE_PIXELS_CANDIDATES = 8192;
hipError_t launch_sample_pixels(int H, int W, int n, int rect_num, const int* rect, unsigned long long seed,
                                unsigned long long counter, int* out, int* status, hipStream_t st);
hipError_t launch_mse_loss(const float* rgb_head, const float* rgb_com, const unsigned char* img_head,
                           const unsigned char* img_com, const int* pix, int n, float* losses, float* d_head, float* d_com,
                           hipStream_t st);
constexpr int BIAS_GRAD_SLICES = 128;      // slices of the points in the streaming bias_grad_kernel
// streaming row sums: parts [BIAS_GRAD_SLICES][n] (workspace), then launch_reduce_bias
hipError_t launch_bias_grad(int tier, int field, const int* e_of, const int* rows, int n, const void* dy_T, long NP,
                            float* parts, float* dbias, hipStream_t st);

// row sums of the dy_T rows behind d(signal) only (dfn_signal_grad): parts [SIG_ROW_SLICES][n_sig], dbias[elem_of[i]] = sum
constexpr int SIG_ROW_SLICES = 128;
hipError_t launch_signal_rows(int tier, int field, const int* row_of, const int* elem_of, int n_sig, const void* dy_T, long NP,
                              float* parts, float* dbias, hipStream_t st);

}  // namespace dfn
