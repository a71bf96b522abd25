// dfn_render_variants.h - THE list of render variants of libdfanerf.so: DFN_VARIANT(name, tier, flags), one line each.
//
// A variant is a precision tier plus a set of flags (dfn_layout.h), and it is one object of the library: dfn_render_<name>.o is
// csrc/dfn_render_variant.hip compiled for <tier, flags>.  (tier, flags) is also the variant's KEY: launch_render(tier, flags, ..)
// and launch_decoder(tier, flags, ..) look it up in the table that dfn_render.hip generates from this file, and the caller - the
// entry point in dfn_api.hip, which knows what it was asked for - states the flags.  Nothing is guessed from the argument block.
// The build reads the same lines (render_variants.sh parses them), and tests/test_variant_list_host.py holds the two together.
// An X-macro file: no include guard, no includes; the includer defines DFN_VARIANT.  One variant per line, nothing else on it.
//
// What the flags mean - which kernels the variant holds, and what the shared slots of RenderArgs (dfn_params.h) carry in it:
//   0             render for one and two fields, decoder for head and torso.  In a trainable tier (f32, bf16) also the training
//                 forwards, chosen at run time by the recorder being on (samples_out / act_T non-null): render_kernel<.., TRAIN = 1, 2>
//                 with or without the loss epilogue, decoder_kernel<.., REC>
//   TIER_W128     the 128-wide inference program (DFN_WIDTH_128; Prog<TIER, HT = 4>): render and decoder, inference only
//   TIER_AUX      the render kernels that also write opacity and expected depth (dfn_render_fwd_aux / _u8_aux).  The per-sample
//                 output slots w_head / w_com / z_out / ranks_out carry aux_head | alpha8_head, aux_com | alpha8_com, depth16_head,
//                 depth16_com.  Render only
//   TIER_RAYS     the render kernels for caller-supplied rays (dfn_render_rays_fwd[_u8]).  The pix_index slot carries `rays`, the
//                 recorder's samples_out slot carries `bounds`.  Render only
//   TIER_ZVALS    the render kernels for caller-supplied sample depths (dfn_render_z_fwd[_u8]; coarse only, 32 ... 192 samples).
//                 The recorder's ranks_out slot carries `zvals`.  Render only
//                 (TIER_AUX, TIER_RAYS and TIER_ZVALS exclude one another; each exists with and without TIER_W128, in the
//                 inference tiers f32 / f16 / f16x3 - bf16 is the training tier)
//   TIER_E4M3     bf16 only: the two training forwards (coarse, hierarchical) whose recorder writes act_T as MX-fp8 e4m3 instead
//                 of MX-fp4 (DFN_TRAIN_ACT_E4M3).  Nothing else
//   TIER_RAYS | TIER_TRAIN [| TIER_E4M3]
//                 f32 and bf16: the two training forwards on caller-supplied rays (dfn_train_rays_fwd / _hier:
//                 render_kernel<TIER | TIER_RAYS, true, TRAIN = 1, 2>; no loss epilogue).  The pix_index slot carries `rays`; the
//                 recorder owns samples_out, so the w_head slot carries `train_bounds`.  With TIER_E4M3 (bf16) the e4m3 recorder's
// Within one variant the launcher (launch_render_tier, dfn_render_kernels.h) still chooses at run time: one or two fields,
// n_fine > 0, and in the flags-0 unit of a trainable tier whether the recorder is on.
DFN_VARIANT(f32,              TIER_F32,   0)
DFN_VARIANT(bf16,             TIER_BF16,  0)
DFN_VARIANT(bf16e,            TIER_BF16,  TIER_E4M3)
DFN_VARIANT(f16,              TIER_F16,   0)
DFN_VARIANT(f16x3,            TIER_F16X3, 0)
DFN_VARIANT(f32_w128,         TIER_F32,   TIER_W128)
DFN_VARIANT(f16_w128,         TIER_F16,   TIER_W128)
DFN_VARIANT(f16x3_w128,       TIER_F16X3, TIER_W128)
DFN_VARIANT(f32_aux,          TIER_F32,   TIER_AUX)
DFN_VARIANT(f16_aux,          TIER_F16,   TIER_AUX)
DFN_VARIANT(f16x3_aux,        TIER_F16X3, TIER_AUX)
DFN_VARIANT(f32_w128_aux,     TIER_F32,   TIER_W128|TIER_AUX)
DFN_VARIANT(f16_w128_aux,     TIER_F16,   TIER_W128|TIER_AUX)
DFN_VARIANT(f16x3_w128_aux,   TIER_F16X3, TIER_W128|TIER_AUX)
DFN_VARIANT(f32_rays,         TIER_F32,   TIER_RAYS)
DFN_VARIANT(f16_rays,         TIER_F16,   TIER_RAYS)
DFN_VARIANT(f16x3_rays,       TIER_F16X3, TIER_RAYS)
DFN_VARIANT(f32_w128_rays,    TIER_F32,   TIER_W128|TIER_RAYS)
DFN_VARIANT(f16_w128_rays,    TIER_F16,   TIER_W128|TIER_RAYS)
DFN_VARIANT(f16x3_w128_rays,  TIER_F16X3, TIER_W128|TIER_RAYS)
DFN_VARIANT(f32_z,            TIER_F32,   TIER_ZVALS)
DFN_VARIANT(f16_z,            TIER_F16,   TIER_ZVALS)
DFN_VARIANT(f16x3_z,          TIER_F16X3, TIER_ZVALS)
DFN_VARIANT(f32_w128_z,       TIER_F32,   TIER_W128|TIER_ZVALS)
DFN_VARIANT(f16_w128_z,       TIER_F16,   TIER_W128|TIER_ZVALS)
DFN_VARIANT(f16x3_w128_z,     TIER_F16X3, TIER_W128|TIER_ZVALS)
DFN_VARIANT(f32_rays_train,   TIER_F32,   TIER_RAYS|TIER_TRAIN)
DFN_VARIANT(bf16_rays_train,  TIER_BF16,  TIER_RAYS|TIER_TRAIN)
DFN_VARIANT(bf16e_rays_train, TIER_BF16,  TIER_RAYS|TIER_TRAIN|TIER_E4M3)
