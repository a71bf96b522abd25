# render_variants.sh - the render variants of libdfanerf.so, for the build: sourced by build.sh and tools/build_variant.sh.
# One line per variant: the object dfn_render_<name>.o is csrc/dfn_render_variant.hip (its header describes the scheme) compiled
# with DFN_VARIANT_TIER = <tier> and DFN_VARIANT_FLAGS = <flags>.  The library's side of the list is the dispatch table of
# csrc/dfn_render.hip; an entry there without a line here does not link.
RENDER_VARIANTS="
f32             TIER_F32    0
bf16            TIER_BF16   0
bf16e           TIER_BF16   TIER_E4M3
f16             TIER_F16    0
f16x3           TIER_F16X3  0
f32_w128        TIER_F32    TIER_W128
f16_w128        TIER_F16    TIER_W128
f16x3_w128      TIER_F16X3  TIER_W128
f32_aux         TIER_F32    TIER_AUX
f16_aux         TIER_F16    TIER_AUX
f16x3_aux       TIER_F16X3  TIER_AUX
f32_w128_aux    TIER_F32    TIER_W128|TIER_AUX
f16_w128_aux    TIER_F16    TIER_W128|TIER_AUX
f16x3_w128_aux  TIER_F16X3  TIER_W128|TIER_AUX
f32_rays        TIER_F32    TIER_RAYS
f16_rays        TIER_F16    TIER_RAYS
f16x3_rays      TIER_F16X3  TIER_RAYS
f32_w128_rays   TIER_F32    TIER_W128|TIER_RAYS
f16_w128_rays   TIER_F16    TIER_W128|TIER_RAYS
f16x3_w128_rays TIER_F16X3  TIER_W128|TIER_RAYS
f32_z           TIER_F32    TIER_ZVALS
f16_z           TIER_F16    TIER_ZVALS
f16x3_z         TIER_F16X3  TIER_ZVALS
f32_w128_z      TIER_F32    TIER_W128|TIER_ZVALS
f16_w128_z      TIER_F16    TIER_W128|TIER_ZVALS
f16x3_w128_z    TIER_F16X3  TIER_W128|TIER_ZVALS
f32_rays_train  TIER_F32    TIER_RAYS|TIER_TRAIN
bf16_rays_train TIER_BF16   TIER_RAYS|TIER_TRAIN
bf16e_rays_train TIER_BF16  TIER_RAYS|TIER_TRAIN|TIER_E4M3
"
# variant_units [tier ...]: the unit names (dfn_render_<name>) of the variants of these tiers, or of all of them
variant_units() {
  local n t f
  while read -r n t f; do
    [ -n "$n" ] || continue
    case " $* " in "  "|*" $t "*) echo "dfn_render_$n";; esac
  done <<< "$RENDER_VARIANTS"
}
# variant_stub <unit> <dir>: if <unit> is a render variant, write its source <dir>/<unit>.hip (three lines: the compiler names the
# ISA file it keeps after the SOURCE, so every variant needs a source of its own name); otherwise fail and write nothing
variant_stub() {
  local n t f
  while read -r n t f; do
    [ "dfn_render_$n" = "$1" ] || continue
    printf '#define DFN_VARIANT_TIER %s\n#define DFN_VARIANT_FLAGS (%s)\n#include "dfn_render_variant.hip"\n' "$t" "$f" > "$2/$1.hip"
    return 0
  done <<< "$RENDER_VARIANTS"
  return 1
}
