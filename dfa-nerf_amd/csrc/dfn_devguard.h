// dfn_devguard.h - the developer switches of the kernels cannot reach a product build by accident.
//
// Two instrumentation switches are left in the sources: DFN_TIMING (per-wave cycle counters in the render and dX kernels, read
// by tools/kernel_timing.py and tools/time_dx.py) and DFN_WL_TRACE (per-workgroup start / end times of the MX weight-gradient
// kernel, read by tools/wl_trace.py).  Defining either without DFN_DEV_BUILD is a compile error; DFN_DEV_BUILD marks the library
// (dfn_version() ends in " DEV"), and dfanerf._lib refuses to load a marked library from the in-tree path (only through
// DFN_LIB=..., the developer override tools/build_variant.sh builds for).  dfa-nerf_amd/build.sh refuses DFN_EXTRA_FLAGS without
// DFN_DEV_BUILD=1 and then passes -DDFN_DEV_BUILD itself; tests/test_pack_plan.py checks all three, and that every DFN_* macro
// a preprocessor conditional of csrc/ tests is either listed here or a named product setting.
// The ablation switches of the tuning rounds (they priced one piece of a kernel by removing it and rendered WRONG results at
// full speed) are retired: LABNOTES.md "Retired switches"; tools/exp_ablations.patch puts them, and their entries here, back.
#pragma once
#if defined(DFN_TIMING) || defined(DFN_WL_TRACE)
#ifndef DFN_DEV_BUILD
#error "a developer switch (DFN_TIMING, DFN_WL_TRACE) is defined without DFN_DEV_BUILD: such a build carries instrumentation - build it with DFN_DEV_BUILD=1 (build.sh) or tools/build_variant.sh, never as the product library"
#endif
#endif
