#!/usr/bin/env python3
"""Build-time check: the 16-bit inference render / decoder kernels must not touch scratch memory.

A stack object or a spilled VGPR in render_kernel<tier, *, TRAIN=false> turns into scratch_load / scratch_store traffic
on every MLP pass (round 1: the Stream struct indexed by a runtime field bit cost the two-field kernel 3.3 GB of HBM
traffic per frame).  Reads the kernel metadata hipcc leaves in the device ISA (--save-temps) and fails if any of those
kernels has a private segment or a `scratch_` instruction in its body.

--agpr-spill-ok: the kernels run one wave per SIMD with the whole 512-register file (the f16x3 tier): VGPRs the allocator parks
in accumulator registers (vgpr_spill_count > 0 with no private segment and no scratch instruction) move no memory and pass.

usage: check_scratch.py [--agpr-spill-ok] <file.s> [...]"""
import re
import sys


def kernels(text):
    """name -> (private_segment_fixed_size, vgpr_spill_count, body)"""
    out = {}
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)",
                         text):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    for name, (priv, spill) in meta.items():
        i = text.find("\n" + name + ":")
        j = text.find(".Lfunc_end", i) if i >= 0 else -1
        out[name] = (priv, spill, text[i:j] if i >= 0 else "")
    return out


def main(paths):
    agpr_ok = "--agpr-spill-ok" in paths
    paths = [p for p in paths if p != "--agpr-spill-ok"]
    bad = seen = 0
    for p in paths:
        for name, (priv, spill, body) in kernels(open(p).read()).items():
            # render_kernel<TIER, TWO, TRAIN (int), ACT4>: TRAIN != 0 are training kernels; decoder_kernel<TIER, TORSO, REC>: REC
            # likewise - not checked here.  (Until round 5 the render_kernel test looked for a BOOL last argument and, since
            # TRAIN had become an int, silently matched nothing: only the decoder kernels were checked.)
            m = re.search(r"render_kernelILi\d+ELb[01]ELi(\d+)E(?:Lb[01]E)?E", name)
            infer = (m is not None and m.group(1) == "0") or \
                    ("decoder_kernel" in name and name.endswith("ELb0EEEvNS_11DecoderArgsE"))
            if not infer:
                continue
            seen += 1
            n_scr = len(re.findall(r"^\s+scratch_", body, re.M))
            ok = priv == 0 and (spill == 0 or agpr_ok) and n_scr == 0
            print(f"{name}: private segment {priv} B, {spill} spilled VGPRs, {n_scr} scratch instructions"
                  + ("" if ok else "   <-- FAIL"))
            bad += not ok
    # (an _aux unit - dfn_render_<tier>[_w128]_aux.hip, the kernels that also write opacity and depth - holds two render kernels only;
    # so does a _rays unit - dfn_render_<tier>[_w128]_rays.hip, the kernels for caller-supplied rays - and a _z unit -
    # dfn_render_<tier>[_w128]_z.hip, the kernels for caller-supplied depths)
    want = 2 if all("_aux-hip-" in p or "_rays-hip-" in p or "_z-hip-" in p for p in paths) else 4
    if any("dfn_render_f16" in p or p.endswith("dfn_render_bf16-hip-amdgcn-amd-amdhsa-gfx950.s") for p in paths) and seen < want:
        print(f"check_scratch: only {seen} inference kernels recognised (expected 2 render + 2 decoder per 16-bit unit, 2 render per "
              "_aux / _rays / _z unit): the name patterns are out of date   <-- FAIL")
        return 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
