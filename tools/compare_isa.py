#!/usr/bin/env python3
"""Compare the device ISA that two builds kept: tools/compare_isa.py <build dir A> <build dir B>

build.sh keeps the gfx950 assembly of the MLP kernels' units (dfn_render_<variant>, dfn_train, dfn_bwd_bf16) in its build
directory as <unit>-hip-amdgcn-amd-amdhsa-gfx950.s.  A change that is meant to leave every kernel alone is checked by building
the parent commit and the changed tree from scratch (build.sh --clean) into two directories and comparing those files.  Two
things differ between any two builds of the same source and are dropped before the comparison: comment lines (they carry
paths and compiler remarks) and every line that names the __hip_cuid_<hash> symbol (a hash of the source file's path and
contents).  Any other .s file of that suffix found in the directories (a unit compiled device-only to assembly by hand:
hipcc --cuda-device-only -S -o <dir>/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s) is compared the same way.

Prints one line per unit and the differing ones again at the end; exit status 0 when every unit is identical, 1 otherwise."""
import difflib
import glob
import os
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


def kept_isa(path):
    lines = []
    for line in open(path, errors="replace"):
        s = line.strip()
        if not s or s.startswith(";") or s.startswith("//") or "__hip_cuid" in s:
            continue
        lines.append(s)
    return lines


def units(d):
    return {os.path.basename(p)[:-len(SUFFIX)]: p for p in glob.glob(os.path.join(d, "*" + SUFFIX))}


def main(a, b):
    ua, ub = units(a), units(b)
    if not ua or not ub:
        print("no *%s under %s" % (SUFFIX, a if not ua else b))
        return 1
    differing = []
    for u in sorted(set(ua) | set(ub)):
        if u not in ua or u not in ub:
            print("%-32s only in %s" % (u, a if u in ua else b))
            differing.append(u)
            continue
        la, lb = kept_isa(ua[u]), kept_isa(ub[u])
        if la == lb:
            print("%-32s identical (%d lines)" % (u, len(la)))
        else:
            n = sum(1 for d in difflib.unified_diff(la, lb, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
            print("%-32s DIFFERS (%d lines)" % (u, n))
            differing.append(u)
    print("%d units compared, %d differ%s" % (len(set(ua) | set(ub)), len(differing), ": " + " ".join(differing) if differing else ""))
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
