// dfn_plan.h - host-side planner (see dfn_plan.cpp): pack plans of the weight streams, and everything the weight-gradient
// launches are planned from.  Plain C++ (compiled with g++, included by the .hip units for the table types): no HIP, no
// environment - developer overrides arrive as arguments.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "dfn_layout.h"

namespace dfn {
// Fills `plan` (one int32 per packed element, padded to whole slabs) and returns the number of
// fragments one pass consumes.  field: 0 head, 1 torso, 2 listener (head program, listener weights).
// width: 256, or 128 = the 128-wide inference program (4 output tiles per trunk layer, half-length K over the hidden vector):
// the same flat-parameter entries, rows and columns below 128 of every hidden-sized tensor only.
long build_pack_plan(int tier, int field, std::vector<int32_t>& plan, int width = 256);
// Transposed (backward) stream of the same field, op order of dfn_bwd.h.  field: 0 head, 1 torso.
long build_bwd_plan(int tier, int field, std::vector<int32_t>& plan);

struct WOp {                    // one weight-gradient GEMM: C[M x N] = dy_T[a_row.., :] * act_T[b_row.., :]^T
    int a_row, M, b_row, N, c_off;
    int bias_owner;             // 1: the first GEMM that reads dy_T rows [a_row, a_row + M): it also accumulates their row sums (bias gradients)
};
// Weight-gradient GEMM list of a field, the map dense-C element -> flat parameter index (or -1), and for every
// element of the field's bias blob the row of dy_T whose sum over the sample points is its gradient.
void build_wgrad_plan(int field, std::vector<WOp>& ops, std::vector<int32_t>& map, std::vector<int32_t>& bias_rows);

// f32 tier: two launches per field, both with the operands through LDS (dfn_train.hip) -
//   wgrad_full_kernel    the 256 x 256 GEMMs (`full_ops`: their indices into ops), one workgroup per (GEMM, slice);
//   wgrad_narrow_kernel  every other GEMM, one workgroup per WNItem (below), all shapes side by side in ONE launch.
struct WNItem {                 // slice `ks` of row tiles [m_tile0, m_tile0 + the shape's MT) of GEMM `op` (f32 tier, narrow shapes)
    int op, ks, m_tile0, shape; // shape: WN_* (dfn_train.hip: the (MT, NT) instantiations of wgrad_lds_part)
};
enum WNShape : int { WN_4x4 = 0, WN_4x2, WN_1x8, WN_4x1, WN_2x2, WN_ROWS, WN_COUNT };
// classification of a GEMM M x N (dy_T rows x act_T rows) for the f32 tier: WN_* and the number of row parts it is cut into
// (-1: the 256 x 256 shape of wgrad_full_kernel; -2: a shape no kernel is instantiated for)
DFN_HD constexpr int wn_shape_of(int M, int N) {
    return (M == 256 && N == 256) ? -1 : (M == 256 && N == 128) ? WN_4x4 : (M == 256 && N == 64) ? WN_4x2 : (M == 32 && N == 256) ? WN_1x8
         : (M == 256 && N == 32) ? WN_4x1 : (M == 64 && N == 64) ? WN_2x2 : (N == 0 && M > 0 && M % 32 == 0) ? WN_ROWS : -2;
}
DFN_HD constexpr int wn_shape_mt(int shape) { return shape == WN_1x8 ? 1 : (shape == WN_2x2 || shape == WN_ROWS) ? 2 : 4; }
// The f32 tier's plan: every GEMM cut into `ksplit` slices of the points.  Returns "" or the error of a GEMM shape the f32
// kernels are not instantiated for.
std::string wgrad_f32_plan(const std::vector<WOp>& ops, int ksplit, std::vector<int>& full_ops, std::vector<WNItem>& nitems);

struct WItem {                  // one workgroup of the 16-bit tier's weight-gradient launch: slice `ks` of `n` of GEMM `op`
    int op, ks, n, pad;
};
// The 16-bit tier's split: `items` in launch order and the slice count of every GEMM, for a launch of about `target_wgs`
// workgroups.  uniform > 0: that many slices for every GEMM instead of the balanced split.
void wgrad_split(const std::vector<WOp>& ops, int uniform, int target_wgs, std::vector<WItem>& items, std::vector<int>& n_of);
// What the 16-bit tier's reduction needs of a split: the slices of the GEMM that owns each 256-element block of the dense C
// array (`c_elems` elements) and of the GEMM that produces each bias element's row sum.  Returns null, or an error message.
const char* wgrad_slice_tables(const std::vector<WOp>& ops, const std::vector<int>& n_of, size_t c_elems,
                               const std::vector<int32_t>& bias_rows, std::vector<unsigned char>& blk_n,
                               std::vector<unsigned char>& bias_n);
// Inverse of the bias row table: dy_T row (of `rows`) -> bias element, -1 for a row that feeds none.  Null, or an error message.
const char* bias_row_inverse(const std::vector<int32_t>& bias_rows, int rows, std::vector<int32_t>& e_of);
// dfn_signal_grad: the dy_T rows behind the `n` bias elements `elems` whose fold carries a signal term.  Null, or an error message.
const char* signal_row_table(const std::vector<int32_t>& bias_rows, const int* elems, int n, std::vector<int32_t>& rows);
}  // namespace dfn
