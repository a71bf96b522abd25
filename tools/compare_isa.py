#!/usr/bin/env python3
"""Compare the device ISA that two builds kept: tools/compare_isa.py <build dir A> <build dir B>

build.sh keeps the gfx950 assembly of the MLP kernels' units (dfn_render_<variant>, dfn_train, dfn_bwd_bf16) in its build
directory as <unit>-hip-amdgcn-amd-amdhsa-gfx950.s.  A change that is meant to leave every kernel alone is checked by building
the parent commit and the changed tree from scratch (build.sh --clean) into two directories and comparing those files.  Two
things differ between any two builds of the same source and are dropped before the comparison: comment lines (they carry
paths and compiler remarks) and every line that names the __hip_cuid_<hash> symbol (a hash of the source file's path and
contents).  Any other .s file of that suffix found in the directories (a unit compiled device-only to assembly by hand:
hipcc --cuda-device-only -S -o <dir>/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s) is compared the same way.

Prints one line per unit and the differing ones again at the end; exit status 0 when every unit is identical, 1 otherwise.

    tools/compare_isa.py --per-kernel <build dir A> <build dir B>

For a change that ADDS kernels to a unit (the unit's file then differs by construction) or gives a kernel template one more
argument (the mangled names change): every kernel of A must have a kernel with the same instruction stream in B.  A kernel's body is
the text between its label and its .Lfunc_end; mangled names, the numbers of local labels (they count the unit's functions) and
trailing comments are dropped before the comparison.  Exit status 0 when every kernel of every unit of A is found in B."""
import difflib
import glob
import os
import re
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


def kernel_bodies(path):
    """label -> normalised lines of every function of an assembly file"""
    out, cur, closed = {}, None, set()
    for line in open(path, errors="replace"):
        s = line.split(";")[0].strip()
        if not s or s.startswith("//") or "__hip_cuid" in s:
            continue
        m = re.match(r"^(_Z\w+):", s)
        if m and cur is None:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None:
            if s.startswith(".Lfunc_end"):
                closed.add(cur)
                cur = None
            else:
                out[cur].append(re.sub(r"\.L(BB|tmp|func_begin|JTI)\d+", r".L\1", re.sub(r"_Z\w+", "SYM", s)))
    return {k: v for k, v in out.items() if k in closed}          # (a data symbol has a label and no .Lfunc_end)


def per_kernel(a, b):
    ua, ub = units(a), units(b)
    missing = 0
    for u in sorted(ua):
        if u not in ub:
            print("%-32s only in %s" % (u, a))
            missing += 1
            continue
        ka, kb = kernel_bodies(ua[u]), kernel_bodies(ub[u])
        have = {}
        for name, body in kb.items():
            have.setdefault("\n".join(body), []).append(name)
        lost = [name for name, body in ka.items() if "\n".join(body) not in have]
        renamed = sum(1 for name, body in ka.items() if "\n".join(body) in have and name not in have["\n".join(body)])
        print("%-32s %d kernels, %d with an identical body in B (%d under another name), %d more kernels in B%s" %
              (u, len(ka), len(ka) - len(lost), renamed, len(kb) - len(ka), "; DIFFERENT: " + " ".join(lost) if lost else ""))
        missing += len(lost)
    print("%d units, %d kernels of A without an identical body in B" % (len(ua), missing))
    return 1 if missing else 0


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
    if len(sys.argv) == 4 and sys.argv[1] == "--per-kernel":
        sys.exit(per_kernel(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
