# render_variants.sh - the render variants of libdfanerf.so, for the build: sourced by build.sh and tools/build_variant.sh.
# The list is csrc/dfn_render_variants.h (DFN_VARIANT(name, tier, flags), one per line; that file says what the flags mean) and is
# read from there: the object dfn_render_<name>.o is csrc/dfn_render_variant.hip compiled with DFN_VARIANT_TIER = <tier> and
# DFN_VARIANT_FLAGS = <flags>.  The library's dispatch table (csrc/dfn_render.hip) is generated from the same lines.
VARIANT_LIST="$(dirname "${BASH_SOURCE[0]}")/csrc/dfn_render_variants.h"
RENDER_VARIANTS="$(sed -n 's/^DFN_VARIANT(\([a-z0-9_]*\), *\(TIER_[A-Z0-9]*\), *\([A-Z0-9_| ]*\))$/\1 \2 \3/p' "$VARIANT_LIST" | sed 's/ *| */|/g')"
# a list line this pattern does not take (upper case in the name, something behind the closing bracket) must not drop out of the build
if [ "$(grep -c '^DFN_VARIANT' "$VARIANT_LIST")" != "$(grep -c . <<< "$RENDER_VARIANTS")" ]; then
  echo "render_variants.sh: a DFN_VARIANT line of $VARIANT_LIST is not of the form DFN_VARIANT(name, TIER_X, FLAGS)" >&2
  return 1 2>/dev/null || exit 1
fi
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
