// dfn_layout.h - register/LDS/HBM layout shared by the host-side pack planner and the gfx950 kernels.
//
// Everything in the fused decoder is organised around the C/D fragment map of the CDNA4 32x32 MFMA
// (v_mfma_f32_32x32x16_bf16 and v_mfma_f32_32x32x2_f32 share it):
//     lane l, accumulator register r  ->  row (r&3) + 8*(r>>2) + 4*(l>>5),  column l&31.
// We compute OUT^T[feature][point] = W[feature][k] * ACT^T[k][point], so rows are output features and
// columns are sample points: lane (n = l&31, h = l>>5) ends a layer holding, for ITS point n, the 16
// features {(r&3)+8*(r>>2)+4h} of every 32-feature tile.  The contraction index of an MFMA is free to
// permute as long as A and B agree, so the NEXT layer consumes those registers directly as its B
// operand (k-slot (h, e) of k-unit u  <->  accumulator register r = (u % UPT)*E + e) and the weights
// (A operand) are pre-permuted to match when they are packed.  No LDS transpose, no cross-lane moves:
// a wave carries its 32 points through the whole MLP in registers.
#pragma once
#include <stdint.h>
#include "dfn_devguard.h"

#if defined(__HIPCC__)
#define DFN_HD __host__ __device__ inline
#else
#define DFN_HD inline
#endif

namespace dfn {

// ---- precision tiers ---------------------------------------------------------------------------
enum Tier : int { TIER_F32 = 0, TIER_BF16 = 1, TIER_F16 = 2, TIER_F16X3 = 3 };
// k-slots per half-wave per k-unit: one k-unit = what one 16-byte A-fragment read feeds.
//   bf16: 8 bf16 per lane  = one v_mfma_f32_32x32x16_bf16  (K=16)
//   f16 : 8 f16 per lane   = one v_mfma_f32_32x32x16_f16   (K=16; same rate and fragment map as bf16, 10 mantissa
//                            bits instead of 7: the throughput tier whose rendered RGB stays within the accuracy clause;
//                            inference only - gradients would underflow f16's 5-bit exponent)
//   f32 : 4 f32 per lane   = four v_mfma_f32_32x32x2_f32   (K=2 each)
//   f16x3: the f16 fragment map with split operands: x ~ hi + 2^-11 lo', hi = f16(x), lo' = f16((x - hi) 2^11); a k-unit is a
//          hi fragment followed by a lo' fragment, and three v_mfma_f32_32x32x16_f16 (hi.hi, hi.lo', lo'.hi; lo'.lo' dropped):
//          ~22-bit products, f32 accumulation.  16-bit in its fragment map (tier_frag16), f32 in everything else (tier_is16 is
//          false: positional encoding, epilogue arithmetic, one wave per SIMD like the f32 tier).  Inference only.
// the width flag of the C ABI (include/dfanerf.h: DFN_WIDTH_128), or'ed into a tier where one argument carries both (the kernels'
// first template argument): the 128-wide inference program
constexpr int TIER_W128 = 0x200, TIER_MASK = 0xff;
// internal (no ABI flag: dfn_render_fwd_aux / dfn_render_fwd_u8_aux are entry points of their own), or'ed into the render kernel's
// first template argument the same way: the instantiation that also writes the opacity and the expected depth of every image
constexpr int TIER_AUX = 0x400;
// internal, the same way (dfn_render_rays_fwd / dfn_render_rays_fwd_u8 are entry points of their own): the instantiation that reads
// its rays - origins, directions, optionally per-ray (near, far) - from memory instead of generating pinhole rays.  Never with TIER_AUX
constexpr int TIER_RAYS = 0x800;
// internal, the same way (dfn_render_z_fwd / dfn_render_z_fwd_u8 are entry points of their own): the instantiation that reads its
// sample depths from memory instead of spacing them between near and far; coarse-only launches of 32 ... 192 samples.  Never with
// TIER_AUX or TIER_RAYS
constexpr int TIER_ZVALS = 0x1000;
// a flag of the render variants (dfn_render_variants.h) only - it never reaches a kernel's first template argument: the 16-bit
// training forwards whose recorder writes e4m3 (render_kernel<.., ACT4 = false>)
constexpr int TIER_E4M3 = 0x100;
// a flag of the render variants only, the same way: the training forwards on caller-supplied rays (dfn_train_rays_fwd / _hier;
// render_kernel<TIER | TIER_RAYS, true, TRAIN = 1, 2>).  Always with TIER_RAYS; with TIER_E4M3 in the bf16 tier
// for the e4m3 recorder
constexpr int TIER_TRAIN = 0x2000;
DFN_HD constexpr bool tier_trainable(int tier) { return tier == TIER_F32 || tier == TIER_BF16; }    // has training kernels (recorder on)
DFN_HD constexpr bool tier_is16(int tier) { return tier == TIER_BF16 || tier == TIER_F16; }     // 16-bit operand arithmetic
DFN_HD constexpr bool tier_frag16(int tier) { return tier != TIER_F32; }                       // 16-bit fragment map (E = 8)
DFN_HD constexpr int tier_split(int tier) { return tier == TIER_F16X3 ? 2 : 1; }                // fragments per k-unit and tile
DFN_HD int tier_E(int tier) { return tier_frag16(tier) ? 8 : 4; }
DFN_HD int tier_UPT(int tier) { return tier_frag16(tier) ? 2 : 4; }        // k-units per 32-feature tile
DFN_HD int tier_elem_bytes(int tier) { return tier_frag16(tier) ? 2 : 4; }
// the split of the f16x3 tier: lo' carries the residual scaled by 2^11 (a normal f16 where the residual itself would be
// subnormal); a product term with one lo' factor is folded back with SPLIT_INV
constexpr float SPLIT_SCALE = 2048.0f, SPLIT_INV = 1.0f / 2048.0f;

constexpr int FRAG_BYTES = 1024;            // one A fragment: 64 lanes x 16 B, lane-linear
constexpr int SLAB_FRAGS = 32;              // ring slot = 32 fragments = 32 KiB
constexpr int SLAB_BYTES = SLAB_FRAGS * FRAG_BYTES;

// feature (within a 32-tile) held by half h, accumulator register r
DFN_HD int tile_feat(int h, int r) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// inverse: feature f in [0,32) -> (h, r)
DFN_HD void tile_feat_inv(int f, int* h, int* r) {
    *h = (f >> 2) & 1;
    *r = (f & 3) + 4 * (f >> 3);
}
// slot index of a vector stored tile-wise: slot = 32*t + tile_feat(h, r)
// k-slot (unit u, half h, element e) of a vector consumed as B operand:
DFN_HD int kslot_to_slot(int tier, int u, int h, int e) {
    const int E = tier_E(tier), UPT = tier_UPT(tier);
    const int t = u / UPT, r = (u % UPT) * E + e;
    return 32 * t + tile_feat(h, r);
}

// ---- 16x16x32: the f16 tier's MFMA shape on the same stream ----------------------------------------------------------------
// The f16 tier (inference only) runs v_mfma_f32_16x16x32_f16: half the accumulator registers moved per multiply-accumulate of
// the 32x32x16 shape.  C/D map: lane l, register j -> row 4 * (l >> 4) + j, column l & 15; A / B: lane l holds row / column
// l & 15, k = 8 * (l >> 4) + e.  Lane l = (i = l & 15, k-group g = l >> 4).  A wave still owns 32 points: point group P0 = points
// 0..15, P1 = points 16..31, two MFMAs per A operand.  Every 32-row tile of the stream is computed as two 16-row halves:
//     T0 = rows with bit 3 clear, T1 = rows with bit 3 set: MFMA row i of half T = tile row m16_row(i, T).
// After a layer, k-group g holds, per tile and point, rows 4 m .. 4 m + 3 for m = (0, 1, 4, 5)[g] (from T0) then m = (2, 3, 6, 7)[g]
// (from T1): m16_feat(g, e).  Those eight rows, in that order, are exactly what k-slot (k-unit g >> 1 of the tile, half g & 1)
// of the 32x32x16 map carries (kslot_to_slot): the A operand of (tile, T, K = 32 step v) is, per lane, ONE whole 16-byte slot of
// the packed stream - slot (half g & 1, row m16_row(i, T)) of fragment 2 v + (g >> 1) of the tile - one ds_read_b128, and the
// stream, its plan and its byte counts are those of the bf16 tier.
// The LDS-DMA lanes of this tier swap bits 3 and 4 of the slot they fetch (m16_dma_off), which puts the 16 slots a k-group reads
// for one T next to each other in LDS: 256 contiguous bytes per 16 lanes, where the stream's own order gives two runs of 128
// bytes, 256 bytes apart (the unpermuted image, measured: LABNOTES.md "Permuted against unpermuted LDS image", profiles/mfma16_ab.txt).
DFN_HD constexpr bool tier_m16(int tier) { return tier == TIER_F16; }
DFN_HD constexpr int m16_row(int i, int T) { return (i & 7) + 16 * (i >> 3) + 8 * T; }
// row (feature) within a 32-tile of element e of k-group g's operand / accumulator octet (e = 4 T + j)
DFN_HD constexpr int m16_feat(int g, int e) { return (e & 3) + 8 * (e >> 2) + 4 * (g & 1) + 16 * (g >> 1); }
// bytes from the slot of T0 to the slot of T1 in the LDS image of a fragment
constexpr int M16_T_BYTES = 256;
// byte offset inside a stream fragment that LDS-DMA lane `lane` fetches (it lands at LDS byte lane * 16 of the fragment's image)
DFN_HD constexpr unsigned m16_dma_off(int lane) {
    const unsigned x = (((unsigned)lane >> 3) ^ ((unsigned)lane >> 4)) & 1u;
    return ((unsigned)lane ^ (x * 0x18u)) * 16u;
}
// this lane's LDS byte offset, from the image of the first fragment of a quad (G = 2 tiles per k-unit: fragments [k-unit][tile]) or
// pair (G = 1) of stream fragments, of its T0 slot of tile 0; tile 1: + FRAG_BYTES, T1: + M16_T_BYTES
DFN_HD constexpr unsigned m16_lane_off(int lane, int G) {
    const unsigned i = lane & 15, g = (unsigned)lane >> 4;
    return (g >> 1) * (unsigned)(G * FRAG_BYTES) + (g & 1) * 512u + i * 16u;
}
// Read `pos` (= fragment index within the 32-fragment slab: one read per stream fragment, in stream order) of a G-tile group: the
// byte offset, from the slab's image + m16_lane_off(lane, G), of the slot the lane reads.  G = 2: reads 4 q .. 4 q + 3 are (tile 0, T0),
// (tile 0, T1), (tile 1, T0), (tile 1, T1) of the K = 32 step whose fragments are 4 q .. 4 q + 3; G = 1: reads 2 q, 2 q + 1 are T0, T1 of
// fragments 2 q, 2 q + 1.  Every k-unit count of the programs is even and the G = 1 groups close a pass, so no quad or pair
// straddles a slab.
DFN_HD constexpr int m16_read_off(int pos, int G) {
    return (G == 2 ? (pos & ~3) + ((pos >> 1) & 1) : (pos & ~1)) * FRAG_BYTES + (pos & 1) * M16_T_BYTES;
}
// the lane's eight bias values of a tile (T0's four rows, then T1's) inside a bias vector ([tile][half][16] floats), in units of 8
DFN_HD constexpr int m16_bias_oct(int lane) { return 2 * ((lane >> 4) & 1) + (lane >> 5); }

// ---- architecture (scripts/test_obama.sh: hidden 256, z 256, dim_signal 96, deform on) -----------
constexpr int HID = 256, ZDIM = 256, NPE = 60, NPEV = 24, NSIG = 96, NET = 42, DH = 64;

// Flat parameter buffer = decoder.state_dict() values concatenated in registration order
// (/root/reference/NeRFs/DFANeRF/decoder.py:207-251; tests/golden/g9_manifest.txt).
enum ParamId : int {
    P_DE0_W, P_DE0_B, P_DE1_W, P_DE1_B, P_DE2_W, P_DE2_B, P_DE3_W, P_DE3_B, P_DE4_W, P_DE4_B,
    P_DEO_W, P_DEO_B,
    P_DS0_W, P_DS0_B, P_DS1_W, P_DS1_B, P_DS2_W, P_DS2_B, P_DS3_W, P_DS3_B, P_DS4_W, P_DS4_B,
    P_DSO_W, P_DSO_B,
    P_DESK_W, P_DESK_B, P_DSSK_W, P_DSSK_B,
    P_FCIN_W, P_FCIN_B, P_FCINL_W, P_FCINL_B, P_FCINT_W, P_FCINT_B,
    P_FCZ_W, P_FCZ_B,
    P_BLK0_W, P_BLK0_B, P_BLK1_W, P_BLK1_B, P_BLK2_W, P_BLK2_B, P_BLK3_W, P_BLK3_B,
    P_BLK4_W, P_BLK4_B, P_BLK5_W, P_BLK5_B, P_BLK6_W, P_BLK6_B,
    P_FCZSK_W, P_FCZSK_B, P_FCPSK_W, P_FCPSK_B, P_FCPSKL_W, P_FCPSKL_B, P_FCPSKT_W, P_FCPSKT_B,
    P_SIGMA_W, P_SIGMA_B, P_FCZV_W, P_FCZV_B, P_FEATV_W, P_FEATV_B, P_FCV_W, P_FCV_B,
    P_FEATO_W, P_FEATO_B,
    P_COUNT
};

struct ParamShape { int rows, cols; };   // bias: rows = n, cols = 1

DFN_HD constexpr ParamShape param_shape(int id) {
    switch (id) {
    case P_DE0_W: case P_DS0_W: return {DH, NPE + NET};
    case P_DE1_W: case P_DE2_W: case P_DE3_W: case P_DE4_W:
    case P_DS1_W: case P_DS2_W: case P_DS3_W: case P_DS4_W: return {DH, DH};
    case P_DE0_B: case P_DE1_B: case P_DE2_B: case P_DE3_B: case P_DE4_B:
    case P_DS0_B: case P_DS1_B: case P_DS2_B: case P_DS3_B: case P_DS4_B:
    case P_DESK_B: case P_DSSK_B: return {DH, 1};
    case P_DEO_W: return {NPE, DH};
    case P_DEO_B: return {NPE, 1};
    case P_DSO_W: return {NET, DH};
    case P_DSO_B: return {NET, 1};
    case P_DESK_W: return {DH, NPE};
    case P_DSSK_W: return {DH, NET};
    case P_FCIN_W: case P_FCPSK_W: return {HID, NPE + NSIG};
    case P_FCINL_W: case P_FCPSKL_W: return {HID, NPE};
    case P_FCINT_W: case P_FCPSKT_W: return {HID, NPE + NET};
    case P_FCZ_W: case P_FCZSK_W: case P_FCZV_W: return {HID, ZDIM};
    case P_BLK0_W: case P_BLK1_W: case P_BLK2_W: case P_BLK3_W: case P_BLK4_W: case P_BLK5_W:
    case P_BLK6_W: case P_FEATV_W: return {HID, HID};
    case P_SIGMA_W: return {1, HID};
    case P_SIGMA_B: return {1, 1};
    case P_FCV_W: return {HID, NPEV};
    case P_FEATO_W: return {3, HID};
    case P_FEATO_B: return {3, 1};
    default: return {HID, 1};   // every remaining id is a 256-wide bias
    }
}

DFN_HD constexpr int param_numel(int id) { return param_shape(id).rows * param_shape(id).cols; }
// offsets of the tensors in the flat parameter vector: a compile-time table (a runtime id costs one load, not a
// 60-iteration loop over the shapes - the fold kernels index it with computed ids)
struct ParamOffsets { int v[P_COUNT + 1]; };
DFN_HD constexpr ParamOffsets make_param_offsets() {
    ParamOffsets t = {};
    int off = 0;
    for (int i = 0; i < P_COUNT; ++i) {
        t.v[i] = off;
        off += param_numel(i);
    }
    t.v[P_COUNT] = off;
    return t;
}
DFN_HD constexpr int param_offset(int id) {
    constexpr ParamOffsets T = make_param_offsets();
    return T.v[id];
}
static_assert(make_param_offsets().v[P_COUNT] == 955242, "flat decoder parameter count");
constexpr int N_DECODER_PARAMS = 955242;     // checked against param_offset(P_COUNT) at load time

// ---- input-vector slot maps -------------------------------------------------------------------------
// PE64:   slot s <-> reference PE column s (decoder.py:271-274: 6*octave + 3*is_cos + axis), s < 60;
//         slots 60..63 are zero padding.  The identity map puts PE column f in exactly the register
//         where a 64-wide GEMM leaves output feature f, so the torso's residual `deform(p) + p`
//         (decoder.py:299) is a lane-local register add.
// VIEW32: slot s <-> view-direction PE column s, s < 24; slots 24..31 zero.
// DPE64 / DSIG64 (torso, after the deformation field): slot s <-> column s (s < 60 resp. s < 42).
DFN_HD int pe_slot_to_ref(int slot) { return slot < NPE ? slot : -1; }
DFN_HD int view_slot_to_ref(int slot) { return slot < NPEV ? slot : -1; }

// ---- programs ---------------------------------------------------------------------------------------
enum Field : int { FIELD_HEAD = 0, FIELD_TORSO = 1 };

// fragment / bias-blob sizes of each field's program, per tier (filled by the planner, checked by the
// kernels with static constants)
struct ProgramInfo {
    int n_frags;        // A fragments in the packed weight stream of one MLP pass
    int n_slabs;        // ring slots consumed by one pass
    int n_bias;         // floats in the per-frame bias blob
};

}  // namespace dfn
