// dfn_api.hip - the C ABI of libdfanerf.so (declared in include/dfanerf.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "dfanerf.h"
#include "dfn_layout.h"
#include "dfn_misc.h"
#include "dfn_mlp.h"
#include "dfn_params.h"
#include "dfn_plan.h"
#include "dfn_signal.h"
#include "dfn_train.h"

using namespace dfn;

namespace {

thread_local std::string g_err;
unsigned long long* g_clock_probe = nullptr;      // dfn_debug_clock_probe (debug only)

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    return fail(DFN_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

bool tier_ok(int tier) {
    return tier == DFN_TIER_F32 || tier == DFN_TIER_BF16 || tier == DFN_TIER_F16 || tier == DFN_TIER_F16X3;
}
constexpr int N_TIERS = 4;          // size of the tier-indexed tables
static_assert(DFN_TIER_F16X3 == TIER_F16X3 && DFN_TIER_F16X3 + 1 == N_TIERS, "tier ids");
static_assert(DFN_WIDTH_128 == TIER_W128 && (DFN_WIDTH_128 & TIER_MASK) == 0 && DFN_WIDTH_128 != DFN_TRAIN_ACT_E4M3, "flags in the tier argument");
// the training entry points: the f16 and f16x3 tiers are inference only (gradients underflow f16's 5-bit exponent)
bool train_tier_ok(int tier) { return tier == DFN_TIER_F32 || tier == DFN_TIER_BF16; }
// DFN_WIDTH_128 (include/dfanerf.h) rides in the tier argument.  The inference entry points take it off with take_width(): tiers
// f32 / f16 / f16x3 only (bf16 is the training tier and stays padded).  Every other entry point that takes a tier refuses it
// with no_width(), before any HIP call.
bool has_width(int tier) { return tier >= 0 && (tier & DFN_WIDTH_128) != 0; }
int no_width(int tier, const char* who) {
    if (!has_width(tier)) return DFN_OK;
    return fail(DFN_E_ARG, std::string(who) + ": DFN_WIDTH_128 selects the 128-wide INFERENCE program (dfn_packed_bytes, dfn_pack_weights, "
                           "dfn_pack_plan, dfn_bias_floats, dfn_fold_bias, dfn_render_fwd, dfn_render_fwd_u8, dfn_decoder_fwd); training "
                           "and everything else stay on the padded 256-wide layout");
}
int take_width(int& tier, int& width, const char* who) {
    width = 256;
    if (!has_width(tier)) return DFN_OK;
    tier &= ~DFN_WIDTH_128;
    width = 128;
    if (tier == DFN_TIER_BF16)
        return fail(DFN_E_ARG, std::string(who) + ": DFN_WIDTH_128 applies to DFN_TIER_F32 / DFN_TIER_F16 / DFN_TIER_F16X3 (bf16 is the "
                               "training tier and stays padded)");
    return DFN_OK;
}
bool field_ok(int field) { return field >= 0 && field <= 2; }
int prog_field(int field) { return field == DFN_FIELD_TORSO ? FIELD_TORSO : FIELD_HEAD; }
// training entry points: head, torso and (round 6) the listener, i.e. the head's program on fc_in_listener / fc_p_skips_listener
// (decoder.py:306-307, 322-323: `signal is None`).  Its dX chain IS the head's: the head's backward stream holds no input layer
// (the positional encoding gets no gradient), so the transposed weight stream and the kernel are shared (bwd_field).
bool train_field_ok(int field) { return field == DFN_FIELD_HEAD || field == DFN_FIELD_TORSO || field == DFN_FIELD_LISTENER; }
int bwd_field(int field) { return field == DFN_FIELD_TORSO ? 1 : 0; }

template <typename T> hipError_t upload(T** dev, const T* host, size_t n) {
    T* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, n * sizeof(T));
    if (e != hipSuccess) return e;
    e = hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) {          // never publish a table that was not filled
        (void)hipFree(d);
        return e;
    }
    *dev = d;
    return hipSuccess;
}
// A table the kernels read: the host vector plus its device copy, uploaded on first use.  The copy is one per PROCESS, on the
// device the first caller uses: this project runs one process per device (dfanerf/parallel.py).  Tables are built and
// published under g_plan_mu, and publish() is the only place that sets `mem`.
template <typename T> struct DevTable {
    std::vector<T> host;
    void* mem = nullptr;
    const T* dev() const { return (const T*)mem; }
    int n() const { return (int)host.size(); }
};
std::mutex g_plan_mu;
struct Staged {
    void** slot;
    void* mem;
};
template <typename T> hipError_t stage(DevTable<T>& t, std::vector<Staged>& staged) {
    if (t.mem || t.host.empty()) return hipSuccess;
    T* d = nullptr;
    const hipError_t e = upload(&d, t.host.data(), t.host.size());
    if (e == hipSuccess) staged.push_back(Staged{&t.mem, d});
    return e;
}
// Uploads those tables of a group that have no device copy yet - all or nothing: the pointers are published only after EVERY
// copy succeeded (a later call must never launch with one table of its group still null); otherwise the copies made are freed.
template <typename... Ts> hipError_t publish(DevTable<Ts>&... tables) {
    std::vector<Staged> staged;
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? stage(tables, staged) : e), ...);
    for (const Staged& s : staged) {
        if (e == hipSuccess) *s.slot = s.mem;
        else (void)hipFree(s.mem);
    }
    return e;
}

// cached pack plans: one flat-parameter index per packed element
using Plan = DevTable<int32_t>;
Plan g_plans[2][N_TIERS][3];          // [width 256 / 128][tier][field]
Plan g_bwd_plans[2][2];               // [tier][bwd_field]
// Host side of a cached plan, built on first use (g_plan_mu held).  A plan whose fragment count disagrees with the kernel's
// is not kept: the error repeats on every call.
template <typename Build> int plan_host(Plan& e, Build build, long kernel_frags, const char* who) {
    if (!e.host.empty()) return DFN_OK;
    std::vector<int32_t> plan;
    const long n_frags = build(plan);
    if (n_frags != kernel_frags)
        return fail(DFN_E_ARG, std::string(who) + " and kernel disagree on the fragment count (" + std::to_string(n_frags) + " vs " +
                                   std::to_string(kernel_frags) + ")");
    e.host = std::move(plan);
    return DFN_OK;
}

// developer overrides: the field's own variable, else the general one; `fallback` when neither is set or the value is
// outside [lo, hi]
int env_int(const char* field_name, const char* name, int lo, int hi, int fallback) {
    const char* e = getenv(field_name);
    if (!e) e = getenv(name);
    if (!e) return fallback;
    const int k = atoi(e);
    return k >= lo && k <= hi ? k : fallback;
}

struct WgradEntry {
    bool built = false;
    DevTable<WOp> ops;
    DevTable<int32_t> map, bias_rows;    // (bias_rows on the device: the `rows` of the reductions)
    DevTable<int32_t> e_of;              // dy_T row -> bias element
    // f32 tier: the 256 x 256 GEMMs (wgrad_full_kernel) and the work items of every other GEMM (wgrad_narrow_kernel)
    DevTable<int> full_ops;
    DevTable<WNItem> nitems;
    std::string plan_error;              // a GEMM shape the f32 kernels are not instantiated for
    // 16-bit tier: one workgroup per (GEMM, slice of the points), the slice count PER GEMM (balanced split, dfn_plan.cpp: wgrad_split)
    // Two splits: [0] the reference's step (<= WGRAD_SMALL_NP points), [1] larger calls (the hierarchical step)
    DevTable<WItem> items[2];
    DevTable<unsigned char> blk_n[2];    // slices of the GEMM that owns each 256-element block of the dense C array
    DevTable<unsigned char> bias_n[2];   // slices of the GEMM that produces each bias element's row sum
    DevTable<int32_t> sig_rows, sig_elems;   // dfn_signal_grad: dy_T rows / bias elements behind d(signal)
};
WgradEntry g_wgrad[3];               // head, torso, listener
#ifndef DFN_WGRAD_KSPLIT_F32
#define DFN_WGRAD_KSPLIT_F32 32
#endif
constexpr int WGRAD_KSPLIT = DFN_WGRAD_KSPLIT_F32;
constexpr long WGRAD_SMALL_NP = 196608;  // 16-bit tier: calls up to this many points use the split with more spare compute units

#ifndef DFN_WS_KSPLIT_MAX
#define DFN_WS_KSPLIT_MAX 32
#endif
constexpr int WS_KSPLIT_MAX = DFN_WS_KSPLIT_MAX;       // slices the workspace is sized for (>= every tier's split)
static_assert(DFN_WGRAD_KSPLIT_F32 <= DFN_WS_KSPLIT_MAX, "the f32 tier's split fits the workspace");
int wgrad_ksplit_bf16(int field) {     // slices of the points per GEMM, bf16 tier (DFN_WGRAD_KSPLIT[_H|_T]: developer overrides)
    static const int v[2] = {env_int("DFN_WGRAD_KSPLIT_H", "DFN_WGRAD_KSPLIT", 1, WS_KSPLIT_MAX, 16),
                             env_int("DFN_WGRAD_KSPLIT_T", "DFN_WGRAD_KSPLIT", 1, WS_KSPLIT_MAX, 18)};
    return v[field == FIELD_TORSO ? 1 : 0];
}

WgradEntry& wgrad_of(int field) {
    std::lock_guard<std::mutex> lk(g_plan_mu);
    WgradEntry& w = g_wgrad[field];
    if (!w.built) {
        build_wgrad_plan(field, w.ops.host, w.map.host, w.bias_rows.host);
        w.plan_error = wgrad_f32_plan(w.ops.host, WGRAD_KSPLIT, w.full_ops.host, w.nitems.host);
        w.built = true;
    }
    return w;
}
// The 16-bit tier's two splits and their slice tables, built on first use (g_plan_mu held) for the compute units of the
// visible device - 256 (MI355X) when there is none.
int wgrad_splits(WgradEntry& w, int field) {
    if (!w.items[0].host.empty()) return DFN_OK;
    int cus = 256;
    {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            cus = prop.multiProcessorCount;
    }
    // some compute units are left to what runs NEXT to the GEMMs - the torso's dX chain next to the head's GEMMs, the
    // single-workgroup kernels of the conditioning networks' chains (their backward, Adam, the next step's encoders) next to
    // both: a launch of exactly one workgroup per compute unit, 144 KiB of LDS and 2 x 236 registers per SIMD each, leaves
    // them no slot until it ends.  Measured, whole step, interleaved on three boxes: the reference's step (131,072 points)
    // with 8 / 16 / 24 spare 0.99-1.02 ms, with 32 / 40 / 48 / 64: 0.95-0.97 (the GEMMs alone: 301 -> 307 us for both
    // fields with 32, 318 with 64); the hierarchical step (393,216 points: its GEMMs are three times as long, what runs next to
    // them is not) 2.756 with 8, 2.80 with 24, 2.788 with 40.  Hence two splits, by the size of the call: 32 / 8 spare.  (The
    // split only changes the ORDER of the sums; the 200-step bf16-vs-f32 curve of tests/test_gpu_train.py, two chaotic
    // trajectories, moves with it: worst step 1.95 % (32) ... 3.3 % (8) ... 5.2 % (40), final loss 0.014-1.0 %.)
    // DFN_WGRAD_SPARE_CUS[_HEAD | _TORSO]: developer override (both splits); DFN_WGRAD_KSPLIT[_H|_T]: a uniform split (the
    // listener reads _T here and _H in wgrad_ksplit_bf16, as it always has)
    const int uniform = env_int(field ? "DFN_WGRAD_KSPLIT_T" : "DFN_WGRAD_KSPLIT_H", "DFN_WGRAD_KSPLIT", 1, 32, 0);
    std::vector<WItem> items[2];
    std::vector<unsigned char> blk_n[2], bias_n[2];
    for (int c = 0; c < 2; ++c) {
        const int spare = env_int(field == FIELD_TORSO ? "DFN_WGRAD_SPARE_CUS_TORSO" : "DFN_WGRAD_SPARE_CUS_HEAD", "DFN_WGRAD_SPARE_CUS",
                                  INT_MIN, INT_MAX, c == 0 ? 32 : 8);
        const int cus_c = (spare >= 0 && spare < cus / 2) ? cus - spare : cus;
        std::vector<int> n_of;
        wgrad_split(w.ops.host, uniform, cus_c, items[c], n_of);
        if (const char* msg = wgrad_slice_tables(w.ops.host, n_of, w.map.host.size(), w.bias_rows.host, blk_n[c], bias_n[c]))
            return fail(DFN_E_ARG, msg);
    }
    for (int c = 0; c < 2; ++c) {
        w.items[c].host = std::move(items[c]);
        w.blk_n[c].host = std::move(blk_n[c]);
        w.bias_n[c].host = std::move(bias_n[c]);
    }
    return DFN_OK;
}

// the small rules of the entry points, stated once
bool coarse_ok(int n) { return n == 32 || n == 64 || n == 128; }     // --N_samples (MAIN:612-619): 32, 64 or 128 coarse samples
// the sample counts of a FORWARD launch (render_kernel): n_fine = 0, 32, 64 or 128; with a fine pass the sampler is a 64-lane wave
// program with one coarse sample per lane, so n_coarse = 32 or 64, and n_fine <= 2 n_coarse (128 fine samples need 64 coarse ones).
// The hierarchical BACKWARD (dfn_composite_bwd_hier) keeps 64 + 64 | 128: its own check.
int counts_ok(int n_coarse, int n_fine, const char* who) {
    if (!coarse_ok(n_coarse)) return fail(DFN_E_ARG, std::string(who) + ": n_coarse must be 32, 64 or 128");
    if (n_fine != 0 && n_fine != 32 && n_fine != 64 && n_fine != 128)
        return fail(DFN_E_ARG, std::string(who) + ": n_fine must be 0, 32, 64 or 128");
    // (128 fine samples first: with them the one coarse count is 64, whatever else was asked for)
    if (n_fine == 128 && n_coarse != 64) return fail(DFN_E_ARG, std::string(who) + ": n_fine = 128 needs n_coarse = 64 (n_fine <= 2 n_coarse <= 128)");
    if (n_fine != 0 && n_coarse != 32 && n_coarse != 64)
        return fail(DFN_E_ARG, std::string(who) + ": the hierarchical mode (n_fine > 0) needs n_coarse = 32 or 64");
    return DFN_OK;
}
// the sample counts of a z launch (dfn_render_z_fwd[_u8]): the depths come from memory, there is no fine pass, and the kernel's LDS
// holds 192 of them per ray
int z_counts_ok(int n_coarse, int n_fine, const char* who) {
    if (n_fine != 0 || n_coarse < 32 || n_coarse > 192 || n_coarse % 32)
        return fail(DFN_E_ARG, std::string(who) + ": caller-supplied depths need n_fine == 0 and n_coarse (the depths per ray) a multiple of 32 "
                                                  "in 32 ... 192");
    return DFN_OK;
}
int smo_ok(int smo_size, const char* who) {
    if (smo_size < 0 || smo_size > 8 || (smo_size & 1)) return fail(DFN_E_ARG, std::string(who) + ": smo_size must be 0, 2, 4, 6 or 8");
    return DFN_OK;
}
int launched(hipError_t e, const char* what) { return e == hipSuccess ? DFN_OK : hip_fail(e, what); }
}  // namespace

extern "C" {

const char* dfn_last_error(void) { return g_err.c_str(); }
#ifdef DFN_DEV_BUILD      // (dfn_devguard.h: a library built with developer switches says so, and dfanerf._lib refuses it in-tree)
const char* dfn_version(void) { return "dfanerf 0.4 gfx950 DEV"; }
#else
const char* dfn_version(void) { return "dfanerf 0.4 gfx950"; }
#endif

long dfn_packed_bytes(int tier, int field) {
    int width;
    if (take_width(tier, width, "dfn_packed_bytes") != DFN_OK) return DFN_E_ARG;
    if (!tier_ok(tier) || !field_ok(field)) return fail(DFN_E_ARG, "dfn_packed_bytes: bad tier/field");
    ProgramInfo pi;
    program_info(tier, prog_field(field), &pi, width);
    return (long)pi.n_slabs * SLAB_BYTES;
}

// the forward pack plan of (tier, field, width), built on first use; dev: with its device copy
static int fwd_plan(int tier, int width, int field, bool dev, const Plan** out) {
    if (!tier_ok(tier) || !field_ok(field)) return fail(DFN_E_ARG, "dfn_pack_plan: bad tier/field");
    ProgramInfo pi;
    program_info(tier, prog_field(field), &pi, width);
    std::lock_guard<std::mutex> lk(g_plan_mu);
    Plan& e = g_plans[width == 128 ? 1 : 0][tier][field];
    const int rc = plan_host(e, [&](std::vector<int32_t>& v) { return build_pack_plan(tier, field, v, width); }, pi.n_frags,
                             "dfn_pack_plan: planner");
    if (rc != DFN_OK) return rc;
    if (dev) {
        const hipError_t err = publish(e);
        if (err != hipSuccess) return hip_fail(err, "upload(plan)");
    }
    *out = &e;
    return DFN_OK;
}
long dfn_pack_plan(int tier, int field, int32_t* plan_host, long capacity) {
    int width;
    if (take_width(tier, width, "dfn_pack_plan") != DFN_OK) return DFN_E_ARG;
    const Plan* e;
    const int rc = fwd_plan(tier, width, field, false, &e);
    if (rc != DFN_OK) return rc;
    if (plan_host) {
        if (capacity < e->n()) return fail(DFN_E_SIZE, "dfn_pack_plan: capacity too small");
        std::memcpy(plan_host, e->host.data(), e->host.size() * sizeof(int32_t));
    }
    return e->n();
}
static int fwd_plan_dev(int tier, int field, const int32_t** dev, long* n_out, int width = 256) {
    const Plan* e;
    const int rc = fwd_plan(tier, width, field, true, &e);
    if (rc != DFN_OK) return rc;
    *dev = e->dev();
    *n_out = e->n();
    return DFN_OK;
}

int dfn_pack_weights(int tier, int field, const float* params, void* packed, void* stream) {
    int width;
    if (take_width(tier, width, "dfn_pack_weights") != DFN_OK) return DFN_E_ARG;
    if (!tier_ok(tier) || !field_ok(field) || !params || !packed)
        return fail(DFN_E_ARG, "dfn_pack_weights: bad argument");
    if (param_offset(P_COUNT) != N_DECODER_PARAMS) return fail(DFN_E_ARG, "internal: parameter table size");
    const int32_t* plan;
    long n;
    const int rc = fwd_plan_dev(tier, field, &plan, &n, width);
    if (rc != DFN_OK) return rc;
    return launched(launch_pack(plan, params, packed, n, tier, (hipStream_t)stream), "pack_kernel");
}

long dfn_bias_floats(int tier, int field) {
    int width;      // (accepted and ignored: the 128-wide program reads the same blob)
    if (take_width(tier, width, "dfn_bias_floats") != DFN_OK) return DFN_E_ARG;
    if (!tier_ok(tier) || !field_ok(field)) return fail(DFN_E_ARG, "dfn_bias_floats: bad tier/field");
    ProgramInfo pi;
    program_info(tier, prog_field(field), &pi);
    return pi.n_bias;
}

int dfn_fold_bias(int tier, int field, const float* params, const float* signal, const float* z_shape,
                  const float* z_app, float* bias, void* stream) {
    int width;      // (accepted and ignored: the blob keeps its layout, the narrow kernels read the first 128 entries of each vector)
    if (take_width(tier, width, "dfn_fold_bias") != DFN_OK) return DFN_E_ARG;
    if (!tier_ok(tier) || !field_ok(field) || !params || !z_shape || !z_app || !bias)
        return fail(DFN_E_ARG, "dfn_fold_bias: bad argument");
    if (field != DFN_FIELD_LISTENER && !signal) return fail(DFN_E_ARG, "dfn_fold_bias: signal is NULL");
    const int n = (int)dfn_bias_floats(tier, field);
    return launched(launch_fold(field, params, signal, z_shape, z_app, bias, n, (hipStream_t)stream), "fold_kernel");
}

int dfn_fold_bias_bwd(int tier, int field, const float* params, const float* signal, const float* z_shape,
                      const float* z_app, const float* dbias, float* grad_flat, float* d_signal, void* stream) {
    if (no_width(tier, "dfn_fold_bias_bwd") != DFN_OK) return DFN_E_ARG;
    if (!tier_ok(tier) || !field_ok(field) || !params || !z_shape || !z_app || !dbias || !grad_flat)
        return fail(DFN_E_ARG, "dfn_fold_bias_bwd: bad argument");
    if (field != DFN_FIELD_LISTENER && !signal) return fail(DFN_E_ARG, "dfn_fold_bias_bwd: signal is NULL");
    const int n = (int)dfn_bias_floats(tier, field);
    return launched(launch_fold_bwd(field, params, signal, z_shape, z_app, dbias, grad_flat, d_signal, n,
                                    (hipStream_t)stream), "fold_bwd_kernel");
}

int dfn_adam_multi(const DfnAdamItem* items_dev, const int32_t* chunks_dev, int n_chunks, float lr, double beta1,
                   double beta2, float eps, float bias_c1, float bias_c2_sqrt, void* stream) {
    if (n_chunks < 0 || (n_chunks > 0 && (!items_dev || !chunks_dev)) || !(bias_c1 > 0.f) || !(bias_c2_sqrt > 0.f))
        return fail(DFN_E_ARG, "dfn_adam_multi: bad argument");
    return launched(launch_adam_multi(items_dev, chunks_dev, n_chunks, lr, beta1, beta2, eps, bias_c1, bias_c2_sqrt,
                                      (hipStream_t)stream), "adam_multi_kernel");
}

long dfn_grad_stats_floats(long n_chunks) {
    if (n_chunks <= 0 || n_chunks > INT_MAX) return fail(DFN_E_ARG, "dfn_grad_stats_floats: n_chunks must be in 1 .. 2^31 - 1");
    return 2 * n_chunks;
}

int dfn_grad_stats(const DfnAdamItem* items_dev, const int32_t* chunks_dev, int n_chunks, long chunk_base, int finish,
                   float max_norm, int skip_nonfinite, float* workspace, DfnGradStats* stats_dev, void* stream) {
    if (!items_dev || !chunks_dev) return fail(DFN_E_ARG, "dfn_grad_stats: items / chunks table is NULL");
    if (n_chunks <= 0) return fail(DFN_E_ARG, "dfn_grad_stats: n_chunks must be positive");
    if (chunk_base < 0 || chunk_base > INT_MAX - n_chunks) return fail(DFN_E_ARG, "dfn_grad_stats: bad chunk_base");
    if (!stats_dev) return fail(DFN_E_ARG, "dfn_grad_stats: the stats record is NULL");
    if (!workspace) return fail(DFN_E_ARG, "dfn_grad_stats: the workspace is NULL (dfn_grad_stats_floats)");
    if (max_norm != max_norm) return fail(DFN_E_ARG, "dfn_grad_stats: max_norm is NaN");
    return launched(launch_grad_stats(items_dev, chunks_dev, n_chunks, chunk_base, finish != 0, max_norm, skip_nonfinite,
                                      workspace, stats_dev, (hipStream_t)stream), "grad_stats_kernel");
}

int dfn_adam_multi_guarded(const DfnAdamItem* items_dev, const int32_t* chunks_dev, int n_chunks, float lr, double beta1,
                           double beta2, float eps, float bias_c1, float bias_c2_sqrt, long t_host,
                           const DfnGradStats* stats_dev, void* stream) {
    if (!items_dev || !chunks_dev) return fail(DFN_E_ARG, "dfn_adam_multi_guarded: items / chunks table is NULL");
    if (n_chunks <= 0) return fail(DFN_E_ARG, "dfn_adam_multi_guarded: n_chunks must be positive");
    if (!stats_dev) return fail(DFN_E_ARG, "dfn_adam_multi_guarded: the stats record is NULL (dfn_grad_stats fills it)");
    if (!(bias_c1 > 0.f) || !(bias_c2_sqrt > 0.f) || t_host < 1)
        return fail(DFN_E_ARG, "dfn_adam_multi_guarded: bias corrections must be positive and t_host >= 1");
    return launched(launch_adam_multi_guarded(items_dev, chunks_dev, n_chunks, lr, beta1, beta2, eps, bias_c1, bias_c2_sqrt,
                                              t_host, stats_dev, (hipStream_t)stream), "adam_multi_guarded_kernel");
}

// The host-side requests of the fused launches: what an entry point was asked for, by name.  Each entry point fills one (value-
// initialised: every member it does not name is null / 0 = off) and states the variant flags of its form (dfn_render_variants.h).
// `who`: the name the shared checks report under - the texts callers match on.
struct RenderReq {
    const char* who;            // dfn_render_z_fwd for the z forms, dfn_render_fwd for every other one
    int flags;                  // 0, TIER_AUX, TIER_RAYS or TIER_ZVALS (DFN_WIDTH_128 arrives in `tier`)
    int tier;                   // the ABI's tier argument, its flags (DFN_WIDTH_128 / DFN_TRAIN_ACT_E4M3) still in it
    const DfnFrame* frame;
    const void *packed_head, *packed_torso;
    const float *bias_head, *bias_torso, *bg_f32;
    const uint8_t* bg_u8;
    const int32_t* pix_index;
    const float *rays, *bounds, *zvals;     // TIER_RAYS: f32 [ray_count, 6 * fields], [ray_count,2] or NULL; TIER_ZVALS: f32 [ray_count, n_coarse]
    void *rgb_head, *rgb_com;   // f32, or uint8 with out_u8
    int out_u8;
    float *weights_head, *weights_com, *z_vals;
    void *aux_head, *aux_com;   // TIER_AUX: f32 [ray_count,2], or alpha8 with out_u8
    uint16_t *depth16_head, *depth16_com;
    void* stream;
};

// What the inference and the training launch both set of a RenderArgs (value-initialised by the caller: all-zero is the "off"
// state of every optional member): frame, blobs and slab counts, bias, backgrounds, pixel ids, rgb outputs.
// (a generic lambda: N is a RenderReq or a TrainReq, and a function template cannot stand inside extern "C")
static const auto render_args = [](RenderArgs& A, const std::string& who, int tier, int width, const DfnFrame& F, const auto& N) -> int {
    // the kernel reads [head | torso] biases from one LDS image: they must be adjacent in memory
    ProgramInfo ph, pt;
    program_info(tier, FIELD_HEAD, &ph, width);
    program_info(tier, FIELD_TORSO, &pt, width);
    if (F.fields == 2 && N.bias_torso != N.bias_head + ph.n_bias)
        return fail(DFN_E_ARG, who + ": bias_torso must directly follow bias_head in memory");
    A.frame = F;
    A.wblob[0] = (const char*)N.packed_head;
    A.wblob[1] = (const char*)(F.fields == 2 ? N.packed_torso : N.packed_head);
    A.nslab[0] = ph.n_slabs;
    A.nslab[1] = F.fields == 2 ? pt.n_slabs : ph.n_slabs;
    A.bias = N.bias_head;
    A.bg_f32 = N.bg_f32;
    A.bg_u8 = N.bg_u8;
    A.pix_index = N.pix_index;
    A.rgb_head = (float*)N.rgb_head;
    A.rgb_com = (float*)N.rgb_com;
    return DFN_OK;
};

static int render_fwd_impl(const RenderReq& q) {
    const bool aux = q.flags == TIER_AUX, rin = q.flags == TIER_RAYS, zin = q.flags == TIER_ZVALS;
    const std::string who = q.who;
    int tier = q.tier, width;
    if (take_width(tier, width, q.who) != DFN_OK) return DFN_E_ARG;
    // caller-supplied depths: the kernels exist in the inference tiers only
    if (zin && tier == DFN_TIER_BF16)
        return fail(DFN_E_ARG, "dfn_render_z_fwd: caller-supplied depths exist in DFN_TIER_F32 / DFN_TIER_F16 / DFN_TIER_F16X3 only "
                               "(bf16 is the training tier)");
    if (zin && !q.zvals) return fail(DFN_E_ARG, "dfn_render_z_fwd: zvals is NULL (dfn_render_fwd renders the frame's own linspace depths)");
    // caller-supplied rays: the kernels exist in the inference tiers only
    if (rin && tier == DFN_TIER_BF16)
        return fail(DFN_E_ARG, "dfn_render_rays_fwd: caller-supplied rays exist in DFN_TIER_F32 / DFN_TIER_F16 / DFN_TIER_F16X3 only "
                               "(bf16 is the training tier)");
    if (rin && !q.rays) return fail(DFN_E_ARG, "dfn_render_rays_fwd: rays is NULL (dfn_render_fwd renders the frame's own pinhole rays)");
    // the aux kernels exist in the inference tiers only (bf16 is the training tier)
    if (aux && tier == DFN_TIER_BF16)
        return fail(DFN_E_ARG, "dfn_render_fwd_aux: opacity / depth outputs exist in DFN_TIER_F32 / DFN_TIER_F16 / DFN_TIER_F16X3 only "
                               "(bf16 is the training tier)");
    if (!tier_ok(tier) || !q.frame || !q.packed_head || !q.bias_head || !q.rgb_head) return fail(DFN_E_ARG, who + ": bad argument");
    const DfnFrame& F = *q.frame;
    if ((zin ? z_counts_ok(F.n_coarse, F.n_fine, "dfn_render_z_fwd") : counts_ok(F.n_coarse, F.n_fine, "dfn_render_fwd")) != DFN_OK)
        return DFN_E_ARG;
    if (F.fields != 1 && F.fields != 2) return fail(DFN_E_ARG, who + ": fields must be 1 or 2");
    if (F.fields == 2 && (!q.packed_torso || !q.bias_torso || !q.rgb_com))
        return fail(DFN_E_ARG, who + ": torso inputs / rgb_com missing for fields == 2");
    if (!q.bg_f32 && !q.bg_u8) return fail(DFN_E_ARG, who + ": no background given");
    if (F.ray_count <= 0) return DFN_OK;
    // (the z kernels address their per-sample arrays by 32-bit byte offsets)
    if (zin && (long)F.ray_count * F.n_coarse >= (1L << 30)) return fail(DFN_E_ARG, "dfn_render_z_fwd: too many rays per call (ray_count * n_coarse must stay under 2^30)");
    // (supplied rays: H, W, ray_begin, the intrinsics and the poses are ignored)
    if (!rin && (F.H <= 0 || F.W <= 0 || (!q.pix_index && (F.ray_begin < 0 || F.ray_begin + F.ray_count > F.H * F.W))))
        return fail(DFN_E_ARG, who + ": ray range outside the image");
    RenderArgs A{};
    const int rc = render_args(A, who, tier, width, F, q);
    if (rc != DFN_OK) return rc;
    A.out_u8 = q.out_u8;
    // the shared slots, by the variant's flags (dfn_params.h)
    if (aux) {
        A.alpha8_head = (unsigned char*)q.aux_head;          // (= aux_head in the f32 form)
        A.alpha8_com = (unsigned char*)q.aux_com;
        A.depth16_head = q.depth16_head;
        A.depth16_com = q.depth16_com;
    } else {
        A.w_head = q.weights_head;
        A.w_com = q.weights_com;
        A.z_out = q.z_vals;
    }
    if (rin) {
        A.rays = q.rays;
        A.bounds = q.bounds;
    }
    if (zin) A.zvals = q.zvals;
    A.clock_probe = g_clock_probe;
    return launched(launch_render(tier, q.flags | (width == 128 ? TIER_W128 : 0), A, (hipStream_t)q.stream), "render_kernel");
}

int dfn_render_fwd(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                   const float* bias_head, const float* bias_torso, const float* bg_f32,
                   const uint8_t* bg_u8, const int32_t* pix_index, float* rgb_head, float* rgb_com,
                   float* weights_head, float* weights_com, float* z_vals, void* stream) {
    return render_fwd_impl({.who = "dfn_render_fwd", .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                            .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .pix_index = pix_index, .rgb_head = rgb_head,
                            .rgb_com = rgb_com, .weights_head = weights_head, .weights_com = weights_com, .z_vals = z_vals, .stream = stream});
}

int dfn_render_fwd_u8(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                      const float* bias_head, const float* bias_torso, const float* bg_f32, const uint8_t* bg_u8,
                      const int32_t* pix_index, uint8_t* rgb8_head, uint8_t* rgb8_com, void* stream) {
    return render_fwd_impl({.who = "dfn_render_fwd", .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                            .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .pix_index = pix_index, .rgb_head = rgb8_head,
                            .rgb_com = rgb8_com, .out_u8 = 1, .stream = stream});
}

int dfn_render_fwd_aux(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                       const float* bias_head, const float* bias_torso, const float* bg_f32, const uint8_t* bg_u8,
                       const int32_t* pix_index, float* rgb_head, float* rgb_com, float* aux_head, float* aux_com, void* stream) {
    if (!aux_head) return fail(DFN_E_ARG, "dfn_render_fwd_aux: aux_head is NULL");
    if (frame && frame->fields == 2 && rgb_com && !aux_com)
        return fail(DFN_E_ARG, "dfn_render_fwd_aux: aux_com missing for fields == 2");
    return render_fwd_impl({.who = "dfn_render_fwd", .flags = TIER_AUX, .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                            .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .pix_index = pix_index, .rgb_head = rgb_head,
                            .rgb_com = rgb_com, .aux_head = aux_head, .aux_com = aux_com, .stream = stream});
}

int dfn_render_fwd_u8_aux(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                          const float* bias_head, const float* bias_torso, const float* bg_f32, const uint8_t* bg_u8,
                          const int32_t* pix_index, uint8_t* rgb8_head, uint8_t* rgb8_com, uint8_t* alpha8_head,
                          uint8_t* alpha8_com, uint16_t* depth16_head, uint16_t* depth16_com, void* stream) {
    if (!alpha8_head && !depth16_head)
        return fail(DFN_E_ARG, "dfn_render_fwd_u8_aux: neither alpha8_head nor depth16_head given (dfn_render_fwd_u8 is the call without aux outputs)");
    if ((!alpha8_head && alpha8_com) || (!depth16_head && depth16_com))
        return fail(DFN_E_ARG, "dfn_render_fwd_u8_aux: an output pair is selected by its _head pointer");
    if (frame && frame->fields == 2 && rgb8_com && ((alpha8_head && !alpha8_com) || (depth16_head && !depth16_com)))
        return fail(DFN_E_ARG, "dfn_render_fwd_u8_aux: alpha8_com / depth16_com missing for fields == 2");
    return render_fwd_impl({.who = "dfn_render_fwd", .flags = TIER_AUX, .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                            .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .pix_index = pix_index, .rgb_head = rgb8_head,
                            .rgb_com = rgb8_com, .out_u8 = 1, .aux_head = alpha8_head, .aux_com = alpha8_com, .depth16_head = depth16_head,
                            .depth16_com = depth16_com, .stream = stream});
}

int dfn_render_rays_fwd(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                        const float* bias_head, const float* bias_torso, const float* rays, const float* bounds,
                        const float* bg_f32, const uint8_t* bg_u8, float* rgb_head, float* rgb_com, float* weights_head,
                        float* weights_com, float* z_vals, void* stream) {
    return render_fwd_impl({.who = "dfn_render_fwd", .flags = TIER_RAYS, .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                            .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .rays = rays, .bounds = bounds,
                            .rgb_head = rgb_head, .rgb_com = rgb_com, .weights_head = weights_head, .weights_com = weights_com, .z_vals = z_vals,
                            .stream = stream});
}

int dfn_render_rays_fwd_u8(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                           const float* bias_head, const float* bias_torso, const float* rays, const float* bounds,
                           const float* bg_f32, const uint8_t* bg_u8, uint8_t* rgb8_head, uint8_t* rgb8_com, void* stream) {
    return render_fwd_impl({.who = "dfn_render_fwd", .flags = TIER_RAYS, .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                            .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .rays = rays, .bounds = bounds,
                            .rgb_head = rgb8_head, .rgb_com = rgb8_com, .out_u8 = 1, .stream = stream});
}

int dfn_render_z_fwd(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                     const float* bias_head, const float* bias_torso, const float* bg_f32, const uint8_t* bg_u8,
                     const int32_t* pix_index, float* rgb_head, float* rgb_com, float* weights_head, float* weights_com,
                     float* z_vals, const float* zvals, void* stream) {
    return render_fwd_impl({.who = "dfn_render_z_fwd", .flags = TIER_ZVALS, .tier = tier, .frame = frame, .packed_head = packed_head,
                            .packed_torso = packed_torso, .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8,
                            .pix_index = pix_index, .zvals = zvals, .rgb_head = rgb_head, .rgb_com = rgb_com, .weights_head = weights_head,
                            .weights_com = weights_com, .z_vals = z_vals, .stream = stream});
}

int dfn_render_z_fwd_u8(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                        const float* bias_head, const float* bias_torso, const float* bg_f32, const uint8_t* bg_u8,
                        const int32_t* pix_index, uint8_t* rgb8_head, uint8_t* rgb8_com, const float* zvals, void* stream) {
    return render_fwd_impl({.who = "dfn_render_z_fwd", .flags = TIER_ZVALS, .tier = tier, .frame = frame, .packed_head = packed_head,
                            .packed_torso = packed_torso, .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8,
                            .pix_index = pix_index, .zvals = zvals, .rgb_head = rgb8_head, .rgb_com = rgb8_com, .out_u8 = 1, .stream = stream});
}

int dfn_fine_depths(const DfnFrame* frame, const float* weights, float* z_all, void* stream) {
    if (!frame || !weights || !z_all) return fail(DFN_E_ARG, "dfn_fine_depths: bad argument");
    const DfnFrame& F = *frame;
    if (counts_ok(F.n_coarse, F.n_fine, "dfn_fine_depths") != DFN_OK) return DFN_E_ARG;
    if (F.n_fine == 0) return fail(DFN_E_ARG, "dfn_fine_depths: the frame has no fine pass (n_fine > 0 selects the pair)");
    if (F.ray_count <= 0) return DFN_OK;
    return launched(launch_fine_depths(weights, F.ray_count, F.n_coarse, F.n_fine, F.z_near, F.z_far, z_all, (hipStream_t)stream),
                    "fine_depths_kernel");
}

// ---- training ---------------------------------------------------------------------------------------------------
long dfn_train_rows(int field, int what) {
    if (!train_field_ok(field)) return fail(DFN_E_ARG, "dfn_train_rows: bad field");
    const bool t = field == DFN_FIELD_TORSO;
    switch (what) {
    case 0: return t ? 64 + 640 + 128 + 9 * 256 + 32 : 64 + 9 * 256 + 32;          // activation rows (RecMap)
    case 1: return t ? 896 + 10 * 256 + 64 : 10 * 256 + 64;                          // gradient rows (GradMap)
    case 2: return t ? 10 + 36 : 36;                                                  // mask dwords per pass
    case 3: {        // workspace floats: split-K partials of the weight gradients + of the bias gradients
        const long W = (long)wgrad_of(field).map.host.size(), nb = dfn_bias_floats(DFN_TIER_BF16, field);
        return WS_KSPLIT_MAX * W + std::max(WS_KSPLIT_MAX, BIAS_GRAD_SLICES) * nb;
    }
    case 4: return (long)BIAS_GRAD_SLICES * dfn_bias_floats(DFN_TIER_BF16, field);   // dfn_bias_grad workspace floats
    case 5: return (long)SIG_ROW_SLICES * 512 + dfn_bias_floats(DFN_TIER_BF16, field);   // dfn_signal_grad workspace floats
    // 16-bit tier: bytes per 32-point tile of the MX-fp8 arrays act_T / dy_T (rows x 32 e4m3 bytes + the scale block)
    case 6: return act_tile_bytes(t ? 64 + 640 + 128 + 9 * 256 + 32 : 64 + 9 * 256 + 32, true);      // act_T of the FUSED step in its default format (MX-fp4: 16 bytes per row)
    case 7: return rec8_tile_bytes(t ? 896 + 10 * 256 + 64 : 10 * 256 + 64);
    // act_T in e4m3 (rows x 32 bytes + the scale block): dfn_decoder_train_fwd (Decoder.forward on explicit points under autograd)
    // and the fused step with DFN_TRAIN_ACT_E4M3
    case 8: return act_tile_bytes(t ? 64 + 640 + 128 + 9 * 256 + 32 : 64 + 9 * 256 + 32, false);
    default: return fail(DFN_E_ARG, "dfn_train_rows: bad selector");
    }
}

long dfn_packed_bwd_bytes(int tier, int field) {
    if (no_width(tier, "dfn_packed_bwd_bytes") != DFN_OK) return DFN_E_ARG;
    if (!train_tier_ok(tier) || !train_field_ok(field)) return fail(DFN_E_ARG, "dfn_packed_bwd_bytes: bad tier/field");
    ProgramInfo pi;
    bwd_program_info(tier, bwd_field(field), &pi);
    return (long)pi.n_slabs * SLAB_BYTES;
}

// device copy of the transposed (backward) pack plan of (tier, field), built and uploaded on first use
static int bwd_plan_dev(int tier, int field, const int32_t** dev, long* n_out) {
    ProgramInfo pi;
    bwd_program_info(tier, field, &pi);
    std::lock_guard<std::mutex> lk(g_plan_mu);
    Plan& e = g_bwd_plans[tier][field];
    const int rc = plan_host(e, [&](std::vector<int32_t>& v) { return build_bwd_plan(tier, field, v); }, pi.n_frags, "backward planner");
    if (rc != DFN_OK) return rc;
    const hipError_t err = publish(e);
    if (err != hipSuccess) return hip_fail(err, "upload(bwd plan)");
    *dev = e.dev();
    *n_out = e.n();
    return DFN_OK;
}

int dfn_pack_weights_bwd(int tier, int field, const float* params, void* packed_T, void* stream) {
    if (no_width(tier, "dfn_pack_weights_bwd") != DFN_OK) return DFN_E_ARG;
    if (!train_tier_ok(tier) || !train_field_ok(field) || !params || !packed_T)
        return fail(DFN_E_ARG, "dfn_pack_weights_bwd: bad argument");
    const int32_t* plan;
    long n;
    const int rc = bwd_plan_dev(tier, bwd_field(field), &plan, &n);
    if (rc != DFN_OK) return rc;
    return launched(launch_pack(plan, params, packed_T, n, tier, (hipStream_t)stream), "pack_kernel(bwd)");
}

int dfn_train_prepare(int tier, const float* params, const float* signal_head, const float* signal_torso,
                      const float* z_shape, const float* z_app, void* packed_head, void* packed_torso, void* packed_T_head,
                      void* packed_T_torso, float* bias_head, float* bias_torso, void* stream) {
    if (no_width(tier, "dfn_train_prepare") != DFN_OK) return DFN_E_ARG;
    if (!train_tier_ok(tier) || !params || !signal_head || !signal_torso || !z_shape || !z_app || !packed_head ||
        !packed_torso || !packed_T_head || !packed_T_torso || !bias_head || !bias_torso)
        return fail(DFN_E_ARG, "dfn_train_prepare: bad argument");
    if (param_offset(P_COUNT) != N_DECODER_PARAMS) return fail(DFN_E_ARG, "internal: parameter table size");
    PrepareJobs J{};
    J.params = params;
    J.tier = tier;
    void* outs[4] = {packed_head, packed_torso, packed_T_head, packed_T_torso};
    for (int k = 0; k < 4; ++k) {
        const int32_t* plan;
        const int rc = k < 2 ? fwd_plan_dev(tier, k, &plan, &J.n[k]) : bwd_plan_dev(tier, k - 2, &plan, &J.n[k]);
        if (rc != DFN_OK) return rc;
        J.plan[k] = plan;
        J.out[k] = outs[k];
    }
    J.sig[0] = signal_head;  J.sig[1] = signal_torso;
    J.bias[0] = bias_head;   J.bias[1] = bias_torso;
    for (int f = 0; f < 2; ++f) {
        J.zs[f] = z_shape + 256 * f;
        J.za[f] = z_app + 256 * f;
        J.nb[f] = (int)dfn_bias_floats(tier, f);
    }
    return launched(launch_prepare(J, (hipStream_t)stream), "prepare_kernel");
}

struct TrainReq {
    const char* who;            // dfn_train[_rays]_fwd[_hier]; a _loss form reports under the name without _loss
    int flags;                  // 0, or TIER_RAYS | TIER_TRAIN (DFN_TRAIN_ACT_E4M3 arrives in `tier`)
    bool hier;
    int tier;                   // the ABI's tier argument, its flags (DFN_WIDTH_128 / DFN_TRAIN_ACT_E4M3) still in it
    const DfnFrame* frame;
    const void *packed_head, *packed_torso;
    const float *bias_head, *bias_torso, *bg_f32;
    const uint8_t* bg_u8;
    const int32_t* pix_index;
    const float *rays, *bounds; // TIER_RAYS | TIER_TRAIN
    float *rgb_head, *rgb_com;
    float* samples;             // the recorder
    void *act_head, *act_torso;
    uint32_t *masks_head, *masks_torso;
    float* z_all;               // hier
    uint8_t* ranks;
    bool with_loss;             // the _loss forms (no rays form)
    const DfnTrainLoss* loss;
    void* stream;
};
static int train_fwd_impl(const TrainReq& q) {
    const bool rin = (q.flags & TIER_RAYS) != 0, hier = q.hier;
    const std::string who = q.who;
    const DfnFrame* frame = q.frame;
    // the format flag rides in the tier argument (include/dfanerf.h: DFN_TRAIN_ACT_E4M3); 16-bit tier only
    int tier = q.tier;
    if (no_width(tier, q.who) != DFN_OK) return DFN_E_ARG;
    const int act_e4m3 = (tier & DFN_TRAIN_ACT_E4M3) != 0;
    if (tier >= 0) tier &= ~DFN_TRAIN_ACT_E4M3;
    if (act_e4m3 && tier != DFN_TIER_BF16) return fail(DFN_E_ARG, who + ": DFN_TRAIN_ACT_E4M3 applies to DFN_TIER_BF16 only");
    if (rin) {
        if (!q.rays)
            return fail(DFN_E_ARG, who + ": rays is NULL (" + (hier ? "dfn_train_fwd_hier" : "dfn_train_fwd") + " renders the frame's own pinhole rays)");
        if (tier == DFN_TIER_F16 || tier == DFN_TIER_F16X3)
            return fail(DFN_E_ARG, who + ": DFN_TIER_F16 / DFN_TIER_F16X3 are inference only; the training step runs in "
                                         "DFN_TIER_F32 / DFN_TIER_BF16");
        if (frame && frame->fields != 2)
            return fail(DFN_E_ARG, who + ": the training step renders two fields (fields == 2; a rays row is o_head, d_head, "
                                         "o_torso, d_torso)");
        if (frame && !hier && (!coarse_ok(frame->n_coarse) || frame->n_fine != 0))
            return fail(DFN_E_ARG, who + ": 32, 64 or 128 coarse samples, no fine ones (dfn_train_rays_fwd_hier is the "
                                         "hierarchical variant)");
        if (frame && hier && frame->n_fine == 0)
            return fail(DFN_E_ARG, who + ": n_fine > 0 (dfn_train_rays_fwd is the coarse-only step)");
    }
    const DfnTrainLoss* loss = q.loss;
    if (q.with_loss && (!loss || !loss->img_head || !loss->img_com || !loss->d_rgb_head || !loss->d_rgb_com || !loss->losses ||
                        !loss->workspace))
        return fail(DFN_E_ARG, who + "_loss: bad loss argument");
    if (!train_tier_ok(tier) || !frame || !q.packed_head || !q.packed_torso || !q.bias_head || !q.bias_torso || !q.rgb_head ||
        !q.rgb_com || !q.samples || !q.act_head || !q.masks_head || !q.act_torso || !q.masks_torso || (hier && (!q.z_all || !q.ranks)))
        return fail(DFN_E_ARG, who + ": bad argument");
    const DfnFrame& F = *frame;
    if (!hier && (!coarse_ok(F.n_coarse) || F.n_fine != 0 || F.fields != 2))
        return fail(DFN_E_ARG, "dfn_train_fwd: the training step is coarse-only (64 samples), two fields (MAIN:855-899); "
                               "dfn_train_fwd_hier is the hierarchical variant");
    // (the forward records at every pair the renderer takes - the f16 guards calibrate through it; the backward is 64 + 64 | 128)
    if (hier && (F.n_fine == 0 || F.fields != 2))
        return fail(DFN_E_ARG, "dfn_train_fwd_hier: n_fine > 0 (dfn_train_fwd is the coarse-only step), two fields");
    if (hier && counts_ok(F.n_coarse, F.n_fine, q.who) != DFN_OK) return DFN_E_ARG;
    if (!q.bg_f32 && !q.bg_u8) return fail(DFN_E_ARG, who + ": no background given");
    if (F.ray_count <= 0) return DFN_OK;
    const long NP = (long)F.ray_count * (F.n_coarse + F.n_fine);
    if (dfn_train_rows(1, 0) * NP >= (1L << 32)) return fail(DFN_E_ARG, who + ": too many rays per call");
    RenderArgs A{};
    const int rc = render_args(A, who, tier, 256, F, q);
    if (rc != DFN_OK) return rc;
    if (hier) {
        A.z_out = q.z_all;
        A.ranks_out = q.ranks;
    }
    A.samples_out = q.samples;
    A.act_T[0] = q.act_head;
    A.act_T[1] = q.act_torso;
    A.masks[0] = q.masks_head;
    A.masks[1] = q.masks_torso;
    A.NP = NP;
    A.act_e4m3 = act_e4m3;
    if (q.with_loss) A.loss = *loss;
    if (rin) {       // the shared slots of TIER_RAYS | TIER_TRAIN (dfn_params.h)
        A.rays = q.rays;
        A.train_bounds = q.bounds;
    }
    return launched(launch_render(tier, q.flags | (act_e4m3 ? TIER_E4M3 : 0), A, (hipStream_t)q.stream), "render_kernel(train)");
}

// per-workgroup partial sums [2][workgroups] + the ticket; a workgroup renders at least 4 rays in every tier
long dfn_train_loss_floats(int ray_count) { return ray_count <= 0 ? 4 : 2L * ((ray_count + 3) / 4) + 4; }
int dfn_train_fwd_loss(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                       const float* bias_head, const float* bias_torso, const float* bg_f32, const uint8_t* bg_u8,
                       const int32_t* pix_index, float* rgb_head, float* rgb_com, float* samples, void* act_head,
                       uint32_t* masks_head, void* act_torso, uint32_t* masks_torso, const DfnTrainLoss* loss, void* stream) {
    return train_fwd_impl({.who = "dfn_train_fwd", .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                           .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .pix_index = pix_index, .rgb_head = rgb_head,
                           .rgb_com = rgb_com, .samples = samples, .act_head = act_head, .act_torso = act_torso, .masks_head = masks_head,
                           .masks_torso = masks_torso, .with_loss = true, .loss = loss, .stream = stream});
}
int dfn_train_fwd_hier_loss(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                            const float* bias_head, const float* bias_torso, const float* bg_f32, const uint8_t* bg_u8,
                            const int32_t* pix_index, float* rgb_head, float* rgb_com, float* samples, void* act_head,
                            uint32_t* masks_head, void* act_torso, uint32_t* masks_torso, float* z_all, uint8_t* ranks,
                            const DfnTrainLoss* loss, void* stream) {
    return train_fwd_impl({.who = "dfn_train_fwd_hier", .hier = true, .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                           .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .pix_index = pix_index, .rgb_head = rgb_head,
                           .rgb_com = rgb_com, .samples = samples, .act_head = act_head, .act_torso = act_torso, .masks_head = masks_head,
                           .masks_torso = masks_torso, .z_all = z_all, .ranks = ranks, .with_loss = true, .loss = loss, .stream = stream});
}

int dfn_train_fwd(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                  const float* bias_head, const float* bias_torso, const float* bg_f32, const uint8_t* bg_u8,
                  const int32_t* pix_index, float* rgb_head, float* rgb_com, float* samples, void* act_head,
                  uint32_t* masks_head, void* act_torso, uint32_t* masks_torso, void* stream) {
    return train_fwd_impl({.who = "dfn_train_fwd", .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                           .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .pix_index = pix_index, .rgb_head = rgb_head,
                           .rgb_com = rgb_com, .samples = samples, .act_head = act_head, .act_torso = act_torso, .masks_head = masks_head,
                           .masks_torso = masks_torso, .stream = stream});
}

int dfn_train_fwd_hier(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                       const float* bias_head, const float* bias_torso, const float* bg_f32, const uint8_t* bg_u8,
                       const int32_t* pix_index, float* rgb_head, float* rgb_com, float* samples, void* act_head,
                       uint32_t* masks_head, void* act_torso, uint32_t* masks_torso, float* z_all, uint8_t* ranks,
                       void* stream) {
    return train_fwd_impl({.who = "dfn_train_fwd_hier", .hier = true, .tier = tier, .frame = frame, .packed_head = packed_head, .packed_torso = packed_torso,
                           .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .pix_index = pix_index, .rgb_head = rgb_head,
                           .rgb_com = rgb_com, .samples = samples, .act_head = act_head, .act_torso = act_torso, .masks_head = masks_head,
                           .masks_torso = masks_torso, .z_all = z_all, .ranks = ranks, .stream = stream});
}

int dfn_train_rays_fwd(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                       const float* bias_head, const float* bias_torso, const float* rays, const float* bounds,
                       const float* bg_f32, const uint8_t* bg_u8, float* rgb_head, float* rgb_com, float* samples, void* act_head,
                       uint32_t* masks_head, void* act_torso, uint32_t* masks_torso, void* stream) {
    return train_fwd_impl({.who = "dfn_train_rays_fwd", .flags = TIER_RAYS | TIER_TRAIN, .tier = tier, .frame = frame, .packed_head = packed_head,
                           .packed_torso = packed_torso, .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .rays = rays,
                           .bounds = bounds, .rgb_head = rgb_head, .rgb_com = rgb_com, .samples = samples, .act_head = act_head, .act_torso = act_torso,
                           .masks_head = masks_head, .masks_torso = masks_torso, .stream = stream});
}

int dfn_train_rays_fwd_hier(int tier, const DfnFrame* frame, const void* packed_head, const void* packed_torso,
                            const float* bias_head, const float* bias_torso, const float* rays, const float* bounds,
                            const float* bg_f32, const uint8_t* bg_u8, float* rgb_head, float* rgb_com, float* samples,
                            void* act_head, uint32_t* masks_head, void* act_torso, uint32_t* masks_torso, float* z_all,
                            uint8_t* ranks, void* stream) {
    return train_fwd_impl({.who = "dfn_train_rays_fwd_hier", .flags = TIER_RAYS | TIER_TRAIN, .hier = true, .tier = tier, .frame = frame,
                           .packed_head = packed_head, .packed_torso = packed_torso, .bias_head = bias_head, .bias_torso = bias_torso, .bg_f32 = bg_f32,
                           .bg_u8 = bg_u8, .rays = rays, .bounds = bounds, .rgb_head = rgb_head, .rgb_com = rgb_com, .samples = samples, .act_head = act_head,
                           .act_torso = act_torso, .masks_head = masks_head, .masks_torso = masks_torso, .z_all = z_all, .ranks = ranks, .stream = stream});
}

int dfn_sample_pixels(int H, int W, int n, int rect_num, const int32_t* rect, uint64_t seed, uint64_t counter,
                      int32_t* pix_index, int32_t* status, void* stream) {
    if (H <= 0 || W <= 0 || n <= 0 || rect_num < 0 || rect_num > n || !pix_index || (rect_num > 0 && !rect))
        return fail(DFN_E_ARG, "dfn_sample_pixels: bad argument");
    if ((long)H * W > 0x7fffffffL || n > SAMPLE_PIXELS_CANDIDATES / 2)
        return fail(DFN_E_ARG, "dfn_sample_pixels: at most 2^31 - 1 pixels and 4096 rays per call");
    return launched(launch_sample_pixels(H, W, n, rect_num, rect, seed, counter, pix_index, status, (hipStream_t)stream), "sample_pixels_kernel");
}

int dfn_mse_loss_u8(const float* rgb_head, const float* rgb_com, const uint8_t* img_head, const uint8_t* img_com,
                    const int32_t* pix_index, int n, float* losses, float* d_rgb_head, float* d_rgb_com, void* stream) {
    if (!rgb_head || !rgb_com || !img_head || !img_com || !pix_index || !losses || !d_rgb_head || !d_rgb_com || n <= 0)
        return fail(DFN_E_ARG, "dfn_mse_loss_u8: bad argument");
    return launched(launch_mse_loss(rgb_head, rgb_com, img_head, img_com, pix_index, n, losses, d_rgb_head, d_rgb_com,
                                    (hipStream_t)stream), "mse_loss_kernel");
}

// ---- the compositing backward of the fused step, its opacity / expected depth, and the backward of a loss that reads them -------
// the checks of the two entry points that name their ray source by which pointer is given: the source, two fields, the counts, the
// hierarchical extras
static int stats_source_checks(const std::string& who, const DfnFrame* frame, const int32_t* pix_index, const float* rays, const float* bounds,
                               const float* z_all, const uint8_t* ranks) {
    if (!pix_index == !rays)
        return fail(DFN_E_ARG, who + ": exactly one of pix_index / rays selects the ray source (" + (rays ? "both" : "neither") + " given)");
    if (bounds && !rays) return fail(DFN_E_ARG, who + ": bounds are the per-ray (near, far) of caller-supplied rays (rays is NULL)");
    if (frame->fields != 2)
        return fail(DFN_E_ARG, who + ": the training step renders two fields (fields == 2: stats holds the head image's and the composite's pair)");
    const bool hier = frame->n_fine > 0;
    if (hier ? (frame->n_coarse != 64 || (frame->n_fine != 64 && frame->n_fine != 128)) : (!coarse_ok(frame->n_coarse) || frame->n_fine != 0))
        return fail(DFN_E_ARG, who + ": 32, 64 or 128 coarse samples, or 64 coarse + 64 or 128 fine samples");
    if (hier && (!z_all || !ranks)) return fail(DFN_E_ARG, who + ": the hierarchical step (n_fine > 0) needs z_all and ranks");
    return DFN_OK;
}
// one request of the compositing backward, whichever entry point it came through
enum BwdForm { BY_PIXEL, ON_RAYS, ON_RAYS_G, WITH_STATS };      // pixel ids | caller-supplied rays | ... + d_norm | dfn_composite_bwd_stats
struct BwdReq {
    const char* who;            // the name refusals are reported under (the _z forms of the pixel-id step: the name without _z) ...
    const char* who_z;          // ... but for a misaligned zero_buf, when this is given
    BwdForm form;
    bool hier;                  // (WITH_STATS: frame->n_fine > 0 instead)
    const DfnFrame* frame;
    const int32_t* pix_index;
    const float *rays, *bounds, *bg_f32;
    const uint8_t* bg_u8;
    const float *samples, *z_all;
    const uint8_t* ranks;
    const float *d_rgb_head, *d_rgb_com, *d_stats;
    float *dsamples, *zero_buf;
    long zero_floats;
    float* d_norm;
    void* stream;
};
// Validates, then fills the one launch block; nothing touches the device before every check has passed, and an empty request
// (ray_count <= 0) is DFN_OK after them.  Order of the refusals (the first that applies is reported), per form:
//   BY_PIXEL     zero_buf alignment (under the _z name) > bad argument > hierarchical counts > coarse counts
//   ON_RAYS      rays NULL > zero_buf alignment > fields > bad argument > hierarchical counts > coarse counts
//   ON_RAYS_G    d_norm NULL > rays NULL > zero_buf alignment > fields > bad argument > hierarchical counts > coarse counts
//   WITH_STATS   a NULL pointer > no background > ray source > bounds without rays > fields > counts > z_all / ranks > d_norm without
//                rays > zero_buf alignment
static int composite_bwd_request(const BwdReq& q) {
    const std::string who = q.who;
    const DfnFrame* frame = q.frame;
    const bool R = q.form == ON_RAYS, G = q.form == ON_RAYS_G, S = q.form == WITH_STATS;
    if (S) {
        if (!frame || !q.samples || !q.d_rgb_head || !q.d_rgb_com || !q.d_stats || !q.dsamples)
            return fail(DFN_E_ARG, who + ": a NULL pointer (frame, samples, d_rgb_head, d_rgb_com, d_stats, dsamples)");
        if (!q.bg_f32 && !q.bg_u8) return fail(DFN_E_ARG, who + ": no background given");
        if (stats_source_checks(who, frame, q.pix_index, q.rays, q.bounds, q.z_all, q.ranks) != DFN_OK) return DFN_E_ARG;
        if (q.d_norm && !q.rays) return fail(DFN_E_ARG, who + ": d_norm is the gradient of the norms of caller-supplied rays (rays is NULL)");
    }
    const bool hier = S ? frame->n_fine > 0 : q.hier;
    if (G && !q.d_norm)
        return fail(DFN_E_ARG, who + ": d_norm is NULL (" + (hier ? "dfn_composite_bwd_hier_rays_z" : "dfn_composite_bwd_rays_z") +
                                   " is the form without the norm gradients)");
    if (R && !q.rays)
        return fail(DFN_E_ARG, who + ": rays is NULL (" + (hier ? "dfn_composite_bwd_hier_z" : "dfn_composite_bwd_z") +
                                   " rebuilds the frame's own pinhole rays)");
    if (G && !q.rays) return fail(DFN_E_ARG, who + ": rays is NULL");
    if (q.zero_buf && (((unsigned long)q.zero_buf & 15) || q.zero_floats < 0))
        return fail(DFN_E_ARG, std::string(q.who_z ? q.who_z : q.who) + ": zero_buf must be 16-byte aligned");
    if (!S) {
        if ((R || G) && frame && frame->fields != 2)
            return fail(DFN_E_ARG, who + ": the training step renders two fields (fields == 2; a rays row is o_head, d_head, o_torso, d_torso)");
        if (!frame || !q.samples || (hier && (!q.z_all || !q.ranks)) || !q.d_rgb_head || !q.dsamples || (!q.bg_f32 && !q.bg_u8))
            return fail(DFN_E_ARG, who + ": bad argument");
        if (hier && (frame->n_coarse != 64 || (frame->n_fine != 64 && frame->n_fine != 128)))
            return fail(DFN_E_ARG, who + ": 64 coarse + 64 or 128 fine samples");
        if (!hier && (!coarse_ok(frame->n_coarse) || frame->n_fine != 0))
            return fail(DFN_E_ARG, who + ": 32, 64 or 128 coarse samples, no fine ones (" +
                                       (G ? "dfn_composite_bwd_hier_rays_zg" : "dfn_composite_bwd_hier") + ")");
    }
    if (frame->ray_count <= 0) return DFN_OK;
    CompositeBwdArgs A{};
    A.frame = *frame;
    A.pix_index = q.pix_index;
    A.bg_f32 = q.bg_f32;
    A.bg_u8 = q.bg_u8;
    A.samples = q.samples;
    A.d_rgb_head = q.d_rgb_head;
    A.d_rgb_com = q.d_rgb_com;
    A.dsamples = q.dsamples;
    A.z_all = q.z_all;            // (hierarchical step only)
    A.ranks = q.ranks;
    A.zero_buf = q.zero_buf;
    A.zero_floats = q.zero_buf ? q.zero_floats : 0;
    A.rays = q.rays;
    A.bounds = q.bounds;
    A.d_norm = q.d_norm;
    A.d_stats = q.d_stats;
    static const char* const of_form[] = {"", "(rays)", "(rays, d_norm)", "(stats)"};
    const std::string kernel = std::string(hier ? "composite_bwd_hier_kernel" : "composite_bwd_kernel") + of_form[q.form];
    return launched(launch_composite_bwd(A, (hipStream_t)q.stream), kernel.c_str());
}
int dfn_composite_bwd(const DfnFrame* frame, const int32_t* pix_index, const float* bg_f32, const uint8_t* bg_u8,
                      const float* samples, const float* d_rgb_head, const float* d_rgb_com, float* dsamples,
                      void* stream) {
    return composite_bwd_request({.who = "dfn_composite_bwd", .frame = frame, .pix_index = pix_index, .bg_f32 = bg_f32, .bg_u8 = bg_u8,
                                  .samples = samples, .d_rgb_head = d_rgb_head, .d_rgb_com = d_rgb_com, .dsamples = dsamples, .stream = stream});
}
int dfn_composite_bwd_z(const DfnFrame* frame, const int32_t* pix_index, const float* bg_f32, const uint8_t* bg_u8,
                        const float* samples, const float* d_rgb_head, const float* d_rgb_com, float* dsamples,
                        float* zero_buf, long zero_floats, void* stream) {
    return composite_bwd_request({.who = "dfn_composite_bwd", .who_z = "dfn_composite_bwd_z", .frame = frame, .pix_index = pix_index, .bg_f32 = bg_f32,
                                  .bg_u8 = bg_u8, .samples = samples, .d_rgb_head = d_rgb_head, .d_rgb_com = d_rgb_com, .dsamples = dsamples,
                                  .zero_buf = zero_buf, .zero_floats = zero_floats, .stream = stream});
}
int dfn_composite_bwd_hier(const DfnFrame* frame, const int32_t* pix_index, const float* bg_f32, const uint8_t* bg_u8,
                           const float* samples, const float* z_all, const uint8_t* ranks, const float* d_rgb_head,
                           const float* d_rgb_com, float* dsamples, void* stream) {
    return composite_bwd_request({.who = "dfn_composite_bwd_hier", .hier = true, .frame = frame, .pix_index = pix_index, .bg_f32 = bg_f32,
                                  .bg_u8 = bg_u8, .samples = samples, .z_all = z_all, .ranks = ranks, .d_rgb_head = d_rgb_head,
                                  .d_rgb_com = d_rgb_com, .dsamples = dsamples, .stream = stream});
}
int dfn_composite_bwd_hier_z(const DfnFrame* frame, const int32_t* pix_index, const float* bg_f32, const uint8_t* bg_u8,
                             const float* samples, const float* z_all, const uint8_t* ranks, const float* d_rgb_head,
                             const float* d_rgb_com, float* dsamples, float* zero_buf, long zero_floats, void* stream) {
    return composite_bwd_request({.who = "dfn_composite_bwd_hier", .who_z = "dfn_composite_bwd_hier_z", .hier = true, .frame = frame,
                                  .pix_index = pix_index, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .samples = samples, .z_all = z_all, .ranks = ranks,
                                  .d_rgb_head = d_rgb_head, .d_rgb_com = d_rgb_com, .dsamples = dsamples, .zero_buf = zero_buf,
                                  .zero_floats = zero_floats, .stream = stream});
}
int dfn_composite_bwd_rays_z(const DfnFrame* frame, const float* rays, const float* bounds, const float* bg_f32, const uint8_t* bg_u8,
                             const float* samples, const float* d_rgb_head, const float* d_rgb_com, float* dsamples, float* zero_buf,
                             long zero_floats, void* stream) {
    return composite_bwd_request({.who = "dfn_composite_bwd_rays_z", .form = ON_RAYS, .frame = frame, .rays = rays, .bounds = bounds,
                                  .bg_f32 = bg_f32, .bg_u8 = bg_u8, .samples = samples, .d_rgb_head = d_rgb_head, .d_rgb_com = d_rgb_com,
                                  .dsamples = dsamples, .zero_buf = zero_buf, .zero_floats = zero_floats, .stream = stream});
}
int dfn_composite_bwd_hier_rays_z(const DfnFrame* frame, const float* rays, const float* bounds, const float* bg_f32,
                                  const uint8_t* bg_u8, const float* samples, const float* z_all, const uint8_t* ranks,
                                  const float* d_rgb_head, const float* d_rgb_com, float* dsamples, float* zero_buf, long zero_floats,
                                  void* stream) {
    return composite_bwd_request({.who = "dfn_composite_bwd_hier_rays_z", .form = ON_RAYS, .hier = true, .frame = frame, .rays = rays,
                                  .bounds = bounds, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .samples = samples, .z_all = z_all, .ranks = ranks,
                                  .d_rgb_head = d_rgb_head, .d_rgb_com = d_rgb_com, .dsamples = dsamples, .zero_buf = zero_buf,
                                  .zero_floats = zero_floats, .stream = stream});
}
// ... + d_norm: the ray gradients of the fused step (f32 tier)
int dfn_composite_bwd_rays_zg(const DfnFrame* frame, const float* rays, const float* bounds, const float* bg_f32, const uint8_t* bg_u8,
                              const float* samples, const float* d_rgb_head, const float* d_rgb_com, float* dsamples, float* zero_buf,
                              long zero_floats, float* d_norm, void* stream) {
    return composite_bwd_request({.who = "dfn_composite_bwd_rays_zg", .form = ON_RAYS_G, .frame = frame, .rays = rays, .bounds = bounds,
                                  .bg_f32 = bg_f32, .bg_u8 = bg_u8, .samples = samples, .d_rgb_head = d_rgb_head, .d_rgb_com = d_rgb_com,
                                  .dsamples = dsamples, .zero_buf = zero_buf, .zero_floats = zero_floats, .d_norm = d_norm, .stream = stream});
}
int dfn_composite_bwd_hier_rays_zg(const DfnFrame* frame, const float* rays, const float* bounds, const float* bg_f32,
                                   const uint8_t* bg_u8, const float* samples, const float* z_all, const uint8_t* ranks,
                                   const float* d_rgb_head, const float* d_rgb_com, float* dsamples, float* zero_buf, long zero_floats,
                                   float* d_norm, void* stream) {
    return composite_bwd_request({.who = "dfn_composite_bwd_hier_rays_zg", .form = ON_RAYS_G, .hier = true, .frame = frame, .rays = rays,
                                  .bounds = bounds, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .samples = samples, .z_all = z_all, .ranks = ranks,
                                  .d_rgb_head = d_rgb_head, .d_rgb_com = d_rgb_com, .dsamples = dsamples, .zero_buf = zero_buf,
                                  .zero_floats = zero_floats, .d_norm = d_norm, .stream = stream});
}
int dfn_composite_bwd_stats(const DfnFrame* frame, const int32_t* pix_index, const float* rays, const float* bounds, const float* bg_f32,
                            const uint8_t* bg_u8, const float* samples, const float* z_all, const uint8_t* ranks, const float* d_rgb_head,
                            const float* d_rgb_com, const float* d_stats, float* dsamples, float* zero_buf, long zero_floats, float* d_norm,
                            void* stream) {
    return composite_bwd_request({.who = "dfn_composite_bwd_stats", .form = WITH_STATS, .frame = frame, .pix_index = pix_index, .rays = rays,
                                  .bounds = bounds, .bg_f32 = bg_f32, .bg_u8 = bg_u8, .samples = samples, .z_all = z_all, .ranks = ranks,
                                  .d_rgb_head = d_rgb_head, .d_rgb_com = d_rgb_com, .d_stats = d_stats, .dsamples = dsamples,
                                  .zero_buf = zero_buf, .zero_floats = zero_floats, .d_norm = d_norm, .stream = stream});
}
int dfn_composite_stats(const DfnFrame* frame, const int32_t* pix_index, const float* rays, const float* bounds, const float* samples,
                        const float* z_all, const uint8_t* ranks, float* stats, void* stream) {
    const std::string who = "dfn_composite_stats";
    if (!frame || !samples || !stats) return fail(DFN_E_ARG, who + ": a NULL pointer (frame, samples, stats)");
    if (stats_source_checks(who, frame, pix_index, rays, bounds, z_all, ranks) != DFN_OK) return DFN_E_ARG;
    if (frame->ray_count <= 0) return DFN_OK;
    CompositeStatsArgs A{};
    A.frame = *frame;
    A.pix_index = pix_index;
    A.rays = rays;
    A.bounds = bounds;
    A.samples = samples;
    A.z_all = z_all;
    A.ranks = ranks;
    A.stats = stats;
    return launched(launch_composite_stats(A, (hipStream_t)stream), "composite_stats_kernel");
}
// ---- ray gradients of the fused step (f32 tier) ---------------------------------------------------------------------------------
// the tier argument of the two ray-gradient entry points: f32 only
static int ray_grad_tier(int tier, const char* who) {
    if (no_width(tier, who) != DFN_OK) return DFN_E_ARG;
    if (tier != DFN_TIER_F32)
        return fail(DFN_E_ARG, std::string(who) + ": ray gradients run in the f32 tier (DFN_TIER_F32: the recorded arrays of the 16-bit tier are "
                               "MX-fp8 / MX-fp4 blocks, and pose gradients are small and precision-sensitive)");
    return DFN_OK;
}
int dfn_points_grad(int tier, int field, long NP, const float* params, const void* act_T, const void* dy_T, float* g_x, float* g_dhat,
                    void* stream) {
    if (ray_grad_tier(tier, "dfn_points_grad") != DFN_OK) return DFN_E_ARG;
    if (!train_field_ok(field)) return fail(DFN_E_ARG, "dfn_points_grad: bad field");
    if (!params || !act_T || !dy_T || !g_x || !g_dhat) return fail(DFN_E_ARG, "dfn_points_grad: NULL pointer (params, act_T, dy_T, g_x, g_dhat)");
    if (NP <= 0 || NP % 32) return fail(DFN_E_ARG, "dfn_points_grad: bad argument (NP must be a positive multiple of 32)");
    PointsGradArgs A{};
    A.params = params;
    A.act_T = (const float*)act_T;
    A.dy_T = (const float*)dy_T;
    A.g_x = g_x;
    A.g_dhat = g_dhat;
    A.n_tiles = NP / 32;
    const bool lis = field == DFN_FIELD_LISTENER;
    A.w_in = param_offset(lis ? P_FCINL_W : P_FCIN_W);
    A.ld_in = param_shape(lis ? P_FCINL_W : P_FCIN_W).cols;
    A.w_skip = param_offset(lis ? P_FCPSKL_W : P_FCPSK_W);
    A.ld_skip = param_shape(lis ? P_FCPSKL_W : P_FCPSK_W).cols;
    return launched(launch_points_grad(bwd_field(field), A, (hipStream_t)stream), "points_grad_kernel");
}
int dfn_rays_grad(int tier, const DfnFrame* frame, const float* rays, const float* bounds, const float* z_all, const uint8_t* ranks,
                  const float* g_x_head, const float* g_dhat_head, const float* g_x_torso, const float* g_dhat_torso, const float* d_norm,
                  float* d_rays, void* stream) {
    if (ray_grad_tier(tier, "dfn_rays_grad") != DFN_OK) return DFN_E_ARG;
    if (!frame || !rays || !g_x_head || !g_dhat_head || !g_x_torso || !g_dhat_torso || !d_norm || !d_rays)
        return fail(DFN_E_ARG, "dfn_rays_grad: NULL pointer (frame, rays, g_x_*, g_dhat_*, d_norm, d_rays)");
    const bool hier = frame->n_fine != 0;
    if (hier && (frame->n_coarse != 64 || (frame->n_fine != 64 && frame->n_fine != 128)))
        return fail(DFN_E_ARG, "dfn_rays_grad: 64 coarse + 64 or 128 fine samples");
    if (!hier && !coarse_ok(frame->n_coarse)) return fail(DFN_E_ARG, "dfn_rays_grad: 32, 64 or 128 coarse samples");
    if (hier && (!z_all || !ranks)) return fail(DFN_E_ARG, "dfn_rays_grad: the hierarchical step needs z_all and ranks");
    if (frame->ray_count <= 0) return DFN_OK;
    RaysGradArgs A{};
    A.frame = *frame;
    A.rays = rays;
    A.bounds = bounds;
    A.z_all = z_all;
    A.ranks = ranks;
    A.g_x[0] = g_x_head;
    A.g_dhat[0] = g_dhat_head;
    A.g_x[1] = g_x_torso;
    A.g_dhat[1] = g_dhat_torso;
    A.d_norm = d_norm;
    A.d_rays = d_rays;
    return launched(launch_rays_grad(A, (hipStream_t)stream), "rays_grad_kernel");
}

int dfn_mlp_bwd(int tier, int field, const void* packed_T, const float* samples, const float* dsamples,
                const uint32_t* masks, long NP, void* dy_T, void* stream) {
    if (no_width(tier, "dfn_mlp_bwd") != DFN_OK) return DFN_E_ARG;
    if (!train_tier_ok(tier) || !train_field_ok(field) || !packed_T || !samples || !dsamples || !masks || !dy_T ||
        NP <= 0 || NP % 32)
        return fail(DFN_E_ARG, "dfn_mlp_bwd: bad argument");
    field = bwd_field(field);
    ProgramInfo pi;
    bwd_program_info(tier, field, &pi);
    MlpBwdArgs A{};
    A.wblob_T = (const char*)packed_T;
    A.nslab = pi.n_slabs;
    A.samples = samples;
    A.dsamples = dsamples;
    A.masks = masks;
    A.dy_T = dy_T;
    A.NP = NP;
    return launched(launch_mlp_bwd(tier, field, A, (hipStream_t)stream), "mlp_bwd_kernel");
}

// the tables behind a bias gradient: e_of (dfn_plan.cpp: bias_row_inverse) and the bias rows themselves
static int ensure_eof(WgradEntry& w, int tier, int field) {
    if ((long)w.bias_rows.host.size() != dfn_bias_floats(tier, field)) return fail(DFN_E_ARG, "internal: bias row table size");
    std::lock_guard<std::mutex> lk(g_plan_mu);
    if (w.e_of.host.empty()) {
        std::vector<int32_t> e_of;
        if (const char* msg = bias_row_inverse(w.bias_rows.host, (int)dfn_train_rows(field, 1), e_of)) return fail(DFN_E_ARG, msg);
        w.e_of.host = std::move(e_of);
    }
    const hipError_t e = publish(w.e_of, w.bias_rows);
    if (e != hipSuccess) return hip_fail(e, "upload(bias rows)");
    return DFN_OK;
}

// stages: 1 = the GEMMs (partial sums into the workspace), 2 = the reduction of the slices, 3 = both
static int weight_grad_impl(int tier, int field, int act_format, const void* dy_T, const void* act_T, long NP, float* workspace,
                            float* grad_flat, float* dbias, void* stream, const char* who, int stages = 3, int which = 3) {
    if (no_width(tier, who) != DFN_OK) return DFN_E_ARG;
    const bool gemm = stages & 1, red = stages & 2;
    if (which < 1 || which > 3 || (which != 3 && (tier != DFN_TIER_F32 || red)))
        return fail(DFN_E_ARG, std::string(who) + ": `which` selects the f32 tier's two GEMM launches (1: 256 x 256, 2: the others, 3: both)");
    if (act_format != DFN_ACT_E4M3 && act_format != DFN_ACT_E2M1)
        return fail(DFN_E_ARG, std::string(who) + ": act_format must be DFN_ACT_E4M3 or DFN_ACT_E2M1");
    if (!train_tier_ok(tier) || !train_field_ok(field) || (gemm && (!dy_T || !act_T)) || !workspace || (red && !grad_flat) ||
        NP <= 0 || NP % 32)
        return fail(DFN_E_ARG, std::string(who) + ": bad argument (NP must be a multiple of 32)");
    WgradEntry& w = wgrad_of(field);
    if (tier == DFN_TIER_F32 && !w.plan_error.empty()) return fail(DFN_E_ARG, std::string(who) + ": " + w.plan_error);
    hipStream_t st = (hipStream_t)stream;
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        if (!w.ops.mem) {       // (one group: ops is published with everything else a launch reads)
            const int rc = wgrad_splits(w, field);
            if (rc != DFN_OK) return rc;
            const hipError_t e = publish(w.ops, w.map, w.full_ops, w.nitems, w.bias_rows, w.items[0], w.blk_n[0], w.bias_n[0], w.items[1],
                                         w.blk_n[1], w.bias_n[1]);
            if (e != hipSuccess) return hip_fail(e, "upload(wgrad plan)");
        }
    }
    // Split-K without atomics: every (GEMM, slice of the points) writes its own slice of the partial arrays in the
    // workspace, the reduce kernels add the slices in index order -> bit-reproducible gradients.
    const long W = (long)w.map.host.size(), n_tiles = NP / 32;
    const int sc = NP > WGRAD_SMALL_NP ? 1 : 0;                    // which of the two splits (wgrad_splits)
    const int nb = w.bias_rows.n();
    const int ks = tier == DFN_TIER_BF16 ? wgrad_ksplit_bf16(field) : WGRAD_KSPLIT;
    if (tier == DFN_TIER_BF16 && (n_tiles & 1))
        return fail(DFN_E_ARG, std::string(who) + ": the 16-bit tier contracts pairs of 32-point tiles: NP must be a multiple of 64");
    const long units = tier == DFN_TIER_BF16 ? n_tiles / 2 : n_tiles;      // what a slice is made of: tile pairs / tiles
    const long per = (units + ks - 1) / ks;
    const int valid = (int)((units + per - 1) / per);             // slices that hold points (the others write nothing)
    float* c_parts = workspace;
    float* b_parts = workspace + (long)WS_KSPLIT_MAX * W;
    hipError_t err = hipSuccess;
    if (dbias) {
        const int rc = ensure_eof(w, tier, field);
        if (rc != DFN_OK) return rc;
    }
    // The row sums (bias gradients) ride along in the GEMMs, partial per slice like the products: bf16 tier two cheap MFMAs
    // per step; f32 tier on the vector ALU from the operand registers (round 5: a streaming row-sum kernel of its own read
    // dy_T a second time, 0.27 ms per field).
    const bool fuse = dbias && tier == DFN_TIER_BF16;
    const bool ride = dbias && tier == DFN_TIER_F32;
    if (!gemm) {
    } else if (tier == DFN_TIER_BF16)
        err = launch_wgrad_bf16(field, act_format == DFN_ACT_E2M1, w.ops.dev(), w.items[sc].dev(), w.items[sc].n(), dy_T, act_T, NP, c_parts,
                                W, fuse ? w.e_of.dev() : nullptr, fuse ? b_parts : nullptr, nb, st);
    else
        err = launch_wgrad(tier, field, w.ops.dev(), w.full_ops.dev(), (which & 1) ? w.full_ops.n() : 0, w.nitems.dev(),
                           (which & 2) ? w.nitems.n() : 0, dy_T, act_T, NP, ks, c_parts, W, ride ? w.e_of.dev() : nullptr,
                           ride ? b_parts : nullptr, nb, st);
    if (err != hipSuccess) return hip_fail(err, "wgrad_kernel");
    if (!red) return DFN_OK;
    if (ride) {
        err = launch_reduce_bias(w.bias_rows.dev(), b_parts, nb, valid, dbias, st);
        if (err != hipSuccess) return hip_fail(err, "reduce_bias_kernel");
    }
    if (tier == DFN_TIER_BF16)          // the per-GEMM slice counts of the balanced split; without dbias: weights only
        return launched(launch_reduce_both(w.map.dev(), c_parts, W, W, valid, grad_flat, fuse ? w.bias_rows.dev() : nullptr,
                                           fuse ? b_parts : nullptr, fuse ? nb : 0, fuse ? dbias : nullptr, w.blk_n[sc].dev(),
                                           fuse ? w.bias_n[sc].dev() : nullptr, units, st),
                        "reduce_both_kernel");
    return launched(launch_reduce_scatter(w.map.dev(), c_parts, W, W, valid, grad_flat, st), "reduce_scatter_kernel");
}

long dfn_wgrad_plan(int field, int what, int32_t* out, long capacity) {
    if (!train_field_ok(field) || what < 0 || what > 4) return fail(DFN_E_ARG, "dfn_wgrad_plan: bad field / selector");
    WgradEntry& w = wgrad_of(field);
    std::vector<int32_t> made;
    if (what == 0)
        for (const WOp& o : w.ops.host) made.insert(made.end(), {o.a_row, o.M, o.b_row, o.N, o.c_off, o.bias_owner});
    if (what >= 3) {        // the 16-bit tier's split of small (3) / large (4) calls: what weight_grad_impl launches
        std::lock_guard<std::mutex> lk(g_plan_mu);
        const int rc = wgrad_splits(w, field);
        if (rc != DFN_OK) return rc;
        for (const WItem& it : w.items[what - 3].host) made.insert(made.end(), {it.op, it.ks, it.n});
    }
    const std::vector<int32_t>& v = what == 1 ? w.map.host : what == 2 ? w.bias_rows.host : made;
    if (out) {
        if (capacity < (long)v.size()) return fail(DFN_E_SIZE, "dfn_wgrad_plan: capacity too small");
        std::memcpy(out, v.data(), v.size() * sizeof(int32_t));
    }
    return (long)v.size();
}

// (the two entry points without a format argument consume what the FUSED step records: dfn_train_fwd / dfn_train_fwd_hier)
int dfn_weight_grad(int tier, int field, const void* dy_T, const void* act_T, long NP, float* workspace,
                    float* grad_flat, void* stream) {
    return weight_grad_impl(tier, field, DFN_ACT_E2M1, dy_T, act_T, NP, workspace, grad_flat, nullptr, stream,
                            "dfn_weight_grad");
}

int dfn_weight_bias_grad(int tier, int field, const void* dy_T, const void* act_T, long NP, float* workspace,
                         float* grad_flat, float* dbias, void* stream) {
    if (!dbias) return fail(DFN_E_ARG, "dfn_weight_bias_grad: dbias is NULL");
    return weight_grad_impl(tier, field, DFN_ACT_E2M1, dy_T, act_T, NP, workspace, grad_flat, dbias, stream,
                            "dfn_weight_bias_grad");
}

int dfn_weight_bias_grad_fmt(int tier, int field, int act_format, const void* dy_T, const void* act_T, long NP, float* workspace,
                             float* grad_flat, float* dbias, void* stream) {
    if (!dbias) return fail(DFN_E_ARG, "dfn_weight_bias_grad_fmt: dbias is NULL");
    return weight_grad_impl(tier, field, act_format, dy_T, act_T, NP, workspace, grad_flat, dbias, stream, "dfn_weight_bias_grad_fmt");
}

int dfn_weight_bias_grad_partials(int tier, int field, int act_format, const void* dy_T, const void* act_T, long NP,
                                  float* workspace, float* dbias, void* stream) {
    if (!dbias) return fail(DFN_E_ARG, "dfn_weight_bias_grad_partials: dbias is NULL");
    return weight_grad_impl(tier, field, act_format, dy_T, act_T, NP, workspace, nullptr, dbias, stream,
                            "dfn_weight_bias_grad_partials", 1);
}
int dfn_weight_bias_grad_partials_part(int tier, int field, int act_format, const void* dy_T, const void* act_T, long NP,
                                       float* workspace, float* dbias, int which, void* stream) {
    if (!dbias) return fail(DFN_E_ARG, "dfn_weight_bias_grad_partials_part: dbias is NULL");
    return weight_grad_impl(tier, field, act_format, dy_T, act_T, NP, workspace, nullptr, dbias, stream,
                            "dfn_weight_bias_grad_partials_part", 1, which);
}
int dfn_weight_bias_grad_reduce(int tier, int field, long NP, float* workspace, float* grad_flat, float* dbias, void* stream) {
    if (!dbias) return fail(DFN_E_ARG, "dfn_weight_bias_grad_reduce: dbias is NULL");
    return weight_grad_impl(tier, field, DFN_ACT_E4M3, nullptr, nullptr, NP, workspace, grad_flat, dbias, stream,
                            "dfn_weight_bias_grad_reduce", 2);
}

int dfn_bias_grad(int tier, int field, const void* dy_T, long NP, float* workspace, float* dbias, void* stream) {
    if (no_width(tier, "dfn_bias_grad") != DFN_OK) return DFN_E_ARG;
    if (!train_tier_ok(tier) || !train_field_ok(field) || !dy_T || !workspace || !dbias || NP <= 0)
        return fail(DFN_E_ARG, "dfn_bias_grad: bad argument");
    WgradEntry& w = wgrad_of(field);
    const int rc = ensure_eof(w, tier, field);
    if (rc != DFN_OK) return rc;
    return launched(launch_bias_grad(tier, field, w.e_of.dev(), w.bias_rows.dev(), w.bias_rows.n(), dy_T, NP, workspace, dbias,
                                     (hipStream_t)stream),
                    "bias_grad_kernel");
}

int dfn_zero_async(void* p, long bytes, void* stream) {
    if (!p || bytes < 0) return fail(DFN_E_ARG, "dfn_zero_async: bad argument");
    if (bytes == 0) return DFN_OK;
    // dword-aligned buffers (the gradient buffers): ONE launch (hipMemsetAsync of a 3.8-MB buffer is two fill kernels, 12 us
    // between the compositing backward and the dX chain of a 1.1-ms step)
    if (((unsigned long)p & 15) == 0 && (bytes & 3) == 0) {
        return launched(launch_zero_words((unsigned*)p, bytes / 4, (hipStream_t)stream), "zero_words_kernel");
    }
    return launched(hipMemsetAsync(p, 0, (size_t)bytes, (hipStream_t)stream), "hipMemsetAsync");
}

int dfn_signal_grad(int tier, int field, const float* params, const void* dy_T, long NP, float* workspace, float* d_signal,
                    void* stream) {
    if (no_width(tier, "dfn_signal_grad") != DFN_OK) return DFN_E_ARG;
    if (!train_tier_ok(tier) || (field != 0 && field != 1) || !params || !dy_T || !workspace || !d_signal || NP <= 0 ||
        NP % 32)
        return fail(DFN_E_ARG, "dfn_signal_grad: bad argument (NP must be a multiple of 32)");
    WgradEntry& w = wgrad_of(field);
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        if (w.sig_rows.host.empty()) {
            int elems[512];
            const int n = sig_term_elements(field, elems);
            std::vector<int32_t> rows;
            if (const char* msg = signal_row_table(w.bias_rows.host, elems, n, rows)) return fail(DFN_E_ARG, msg);
            w.sig_elems.host.assign(elems, elems + n);
            w.sig_rows.host = std::move(rows);
        }
        const hipError_t e = publish(w.sig_rows, w.sig_elems);
        if (e != hipSuccess) return hip_fail(e, "upload(signal rows)");
    }
    float* parts = workspace;
    float* dbias = workspace + (long)SIG_ROW_SLICES * 512;      // behind the partial sums' whole area (launch_signal_rows sizes the split)
    hipError_t err = launch_signal_rows(tier, field, w.sig_rows.dev(), w.sig_elems.dev(), w.sig_rows.n(), dy_T, NP, parts, dbias,
                                        (hipStream_t)stream);
    if (err != hipSuccess) return hip_fail(err, "sig_rows_kernel");
    return launched(launch_fold_bwd_sig(field, params, dbias, d_signal, true, (hipStream_t)stream), "fold_bwd_sig_kernel");
}

static int encode_signal_impl(const float* aud_params, const float* exp_params, const float* att_params, const float* auds,
                              const float* exps, int n_total, const int32_t* frame_ids, int n_frames, int smo_size, float* out,
                              float* keep, void* stream) {
    if (!aud_params || !exp_params || !auds || !exps || !frame_ids || !out || n_total <= 0 || n_frames < 0)
        return fail(DFN_E_ARG, "dfn_encode_signal: bad argument");
    if (keep && n_frames != 1) return fail(DFN_E_ARG, "dfn_encode_signal_keep: one frame (the training step's)");
    if (smo_ok(smo_size, "dfn_encode_signal") != DFN_OK) return DFN_E_ARG;
    if (smo_size > 0 && !att_params) return fail(DFN_E_ARG, "dfn_encode_signal: attention parameters missing");
    if (n_frames == 0) return DFN_OK;
    return launched(launch_encode_signal(aud_params, exp_params, att_params, auds, exps, n_total, frame_ids, n_frames,
                                         smo_size, out, keep, (hipStream_t)stream), "encode_signal_kernel");
}
int dfn_encode_signal(const float* aud_params, const float* exp_params, const float* att_params, const float* auds,
                      const float* exps, int n_total, const int32_t* frame_ids, int n_frames, int smo_size, float* out,
                      void* stream) {
    return encode_signal_impl(aud_params, exp_params, att_params, auds, exps, n_total, frame_ids, n_frames, smo_size, out, nullptr,
                              stream);
}
int dfn_encode_signal_keep(const float* aud_params, const float* exp_params, const float* att_params, const float* auds,
                           const float* exps, int n_total, const int32_t* frame_id, int smo_size, float* out, float* keep,
                           void* stream) {
    if (!keep) return fail(DFN_E_ARG, "dfn_encode_signal_keep: keep is NULL");
    return encode_signal_impl(aud_params, exp_params, att_params, auds, exps, n_total, frame_id, 1, smo_size, out, keep, stream);
}
long dfn_encode_signal_keep_floats(void) { return SigKeep::TOTAL; }

int dfn_encode_signal_torso(const float* att_params, const float* poses, int pose_stride, int n_total,
                            const int32_t* frame_ids, int n_frames, int smo_size, float* out, void* stream) {
    if (!poses || !frame_ids || !out || n_total <= 0 || n_frames < 0 || (pose_stride != 12 && pose_stride != 16))
        return fail(DFN_E_ARG, "dfn_encode_signal_torso: bad argument");
    if (smo_ok(smo_size, "dfn_encode_signal_torso") != DFN_OK) return DFN_E_ARG;
    if (smo_size > 0 && !att_params) return fail(DFN_E_ARG, "dfn_encode_signal_torso: attention parameters missing");
    if (n_frames == 0) return DFN_OK;
    return launched(launch_encode_signal_torso(att_params, poses, pose_stride, n_total, frame_ids, n_frames, smo_size, out,
                                               (hipStream_t)stream), "encode_signal_torso_kernel");
}

static int encode_signal_bwd_impl(const float* aud_params, const float* exp_params, const float* att_params, const float* auds,
                                  const float* exps, int n_total, int frame, int smo_size, const float* d_out, float* g_aud,
                                  float* g_exp, float* g_att, bool set, void* stream, const float* kept = nullptr) {
    if (!aud_params || !exp_params || !auds || !exps || !d_out || !g_aud || !g_exp || n_total <= 0)
        return fail(DFN_E_ARG, "dfn_encode_signal_bwd: bad argument");
    if (smo_ok(smo_size, "dfn_encode_signal_bwd") != DFN_OK) return DFN_E_ARG;
    if (smo_size > 0 && (!att_params || !g_att)) return fail(DFN_E_ARG, "dfn_encode_signal_bwd: attention buffers missing");
    return launched(launch_encode_signal_bwd(aud_params, exp_params, att_params, auds, exps, n_total, frame, smo_size,
                                             d_out, g_aud, g_exp, g_att, set, kept, (hipStream_t)stream), "encode_signal_bwd_kernel");
}
int dfn_encode_signal_bwd(const float* aud_params, const float* exp_params, const float* att_params, const float* auds,
                          const float* exps, int n_total, int frame, int smo_size, const float* d_out, float* g_aud,
                          float* g_exp, float* g_att, void* stream) {
    return encode_signal_bwd_impl(aud_params, exp_params, att_params, auds, exps, n_total, frame, smo_size, d_out, g_aud, g_exp,
                                  g_att, false, stream);
}
int dfn_encode_signal_bwd_kept(const float* aud_params, const float* exp_params, const float* att_params, const float* auds,
                               const float* exps, int n_total, int frame, int smo_size, const float* d_out, const float* kept,
                               float* g_aud, float* g_exp, float* g_att, void* stream) {
    if (!kept) return fail(DFN_E_ARG, "dfn_encode_signal_bwd_kept: kept is NULL");
    return encode_signal_bwd_impl(aud_params, exp_params, att_params, auds, exps, n_total, frame, smo_size, d_out, g_aud, g_exp,
                                  g_att, false, stream, kept);
}
int dfn_encode_signal_bwd_set(const float* aud_params, const float* exp_params, const float* att_params, const float* auds,
                              const float* exps, int n_total, int frame, int smo_size, const float* d_out, float* g_aud,
                              float* g_exp, float* g_att, void* stream) {
    return encode_signal_bwd_impl(aud_params, exp_params, att_params, auds, exps, n_total, frame, smo_size, d_out, g_aud, g_exp,
                                  g_att, true, stream);
}

static int encode_signal_torso_bwd_impl(const float* att_params, const float* poses, int pose_stride, int n_total, int frame,
                                        int smo_size, const float* d_out, float* g_att, bool set, void* stream) {
    if (!poses || !d_out || n_total <= 0 || (pose_stride != 12 && pose_stride != 16))
        return fail(DFN_E_ARG, "dfn_encode_signal_torso_bwd: bad argument");
    if (smo_ok(smo_size, "dfn_encode_signal_torso_bwd") != DFN_OK) return DFN_E_ARG;
    if (smo_size == 0) return DFN_OK;          // no parameter takes part before --nosmo_iters
    if (!att_params || !g_att) return fail(DFN_E_ARG, "dfn_encode_signal_torso_bwd: attention buffers missing");
    return launched(launch_encode_signal_torso_bwd(att_params, poses, pose_stride, n_total, frame, smo_size, d_out, g_att, set,
                                                   (hipStream_t)stream), "encode_signal_torso_bwd_kernel");
}
int dfn_encode_signal_torso_bwd(const float* att_params, const float* poses, int pose_stride, int n_total, int frame,
                                int smo_size, const float* d_out, float* g_att, void* stream) {
    return encode_signal_torso_bwd_impl(att_params, poses, pose_stride, n_total, frame, smo_size, d_out, g_att, false, stream);
}
int dfn_encode_signal_torso_bwd_set(const float* att_params, const float* poses, int pose_stride, int n_total, int frame,
                                    int smo_size, const float* d_out, float* g_att, void* stream) {
    return encode_signal_torso_bwd_impl(att_params, poses, pose_stride, n_total, frame, smo_size, d_out, g_att, true, stream);
}

// the decoder on explicit points; samples / act_T / masks: the training recorder (all null for inference)
static int decoder_impl(int tier, int width, int field, const void* packed, const float* bias, const float* points, const float* dirs,
                        long n, float* feat, float* sigma, float* samples, void* act_T, uint32_t* masks, const char* what, void* stream) {
    ProgramInfo pi;
    program_info(tier, prog_field(field), &pi, width);
    DecoderArgs A{};
    A.wblob = (const char*)packed;
    A.nslab = pi.n_slabs;
    A.field = prog_field(field);
    A.bias = bias;
    A.n_bias = pi.n_bias;
    A.points = points;
    A.dirs = dirs;
    A.n_points = n;
    A.feat = feat;
    A.sigma = sigma;
    A.samples = samples;
    A.act_T = act_T;
    A.masks = masks;
    return launched(launch_decoder(tier, width == 128 ? TIER_W128 : 0, A, (hipStream_t)stream), what);
}

int dfn_decoder_fwd(int tier, int field, const void* packed, const float* bias, const float* points,
                    const float* dirs, long n, float* feat, float* sigma, void* stream) {
    int width;
    if (take_width(tier, width, "dfn_decoder_fwd") != DFN_OK) return DFN_E_ARG;
    if (!tier_ok(tier) || !field_ok(field) || !packed || !bias || !points || !dirs || !feat || !sigma)
        return fail(DFN_E_ARG, "dfn_decoder_fwd: bad argument");
    if (n <= 0) return DFN_OK;
    return decoder_impl(tier, width, field, packed, bias, points, dirs, n, feat, sigma, nullptr, nullptr, nullptr, "decoder_kernel", stream);
}

int dfn_decoder_train_fwd(int tier, int field, const void* packed, const float* bias, const float* points,
                          const float* dirs, long n, float* feat, float* sigma, float* samples, void* act_T,
                          uint32_t* masks, void* stream) {
    if (no_width(tier, "dfn_decoder_train_fwd") != DFN_OK) return DFN_E_ARG;
    if (!train_tier_ok(tier) || !train_field_ok(field) || !packed || !bias || !points ||
        !dirs || !feat || !sigma || !samples || !act_T || !masks)
        return fail(DFN_E_ARG, "dfn_decoder_train_fwd: bad argument (tiers f32 / bf16, fields head / torso / listener)");
    if (n <= 0) return DFN_OK;
    const long NP = (n + 31) / 32 * 32;
    if (dfn_train_rows(1, 0) * NP >= (1L << 32)) return fail(DFN_E_ARG, "dfn_decoder_train_fwd: too many points per call");
    return decoder_impl(tier, 256, field, packed, bias, points, dirs, n, feat, sigma, samples, act_T, masks, "decoder_kernel(train)", stream);
}

int dfn_get_rays(int H, int W, float focal, float cx, float cy, const float* c2w_host, float* rays_o,
                 float* rays_d, void* stream) {
    return dfn_get_rays_strided(H, W, 1, focal, cx, cy, c2w_host, rays_o, rays_d, stream);
}

int dfn_get_rays_strided(int H, int W, int stride, float focal, float cx, float cy, const float* c2w_host, float* rays_o,
                         float* rays_d, void* stream) {
    if (H <= 0 || W <= 0 || stride <= 0 || H / stride <= 0 || W / stride <= 0 || !c2w_host || !rays_o || !rays_d)
        return fail(DFN_E_ARG, "dfn_get_rays: bad argument");
    return launched(launch_get_rays(H, W, stride, focal, cx, cy, c2w_host, rays_o, rays_d, (hipStream_t)stream), "get_rays_kernel");
}

int dfn_ndc_rays(int H, int W, float focal, float z_near, const float* rays_o, const float* rays_d, long n,
                 float* out_o, float* out_d, void* stream) {
    if (!rays_o || !rays_d || !out_o || !out_d || n < 0) return fail(DFN_E_ARG, "dfn_ndc_rays: bad argument");
    if (n == 0) return DFN_OK;
    return launched(launch_ndc_rays(H, W, focal, z_near, rays_o, rays_d, n, out_o, out_d, (hipStream_t)stream), "ndc_rays_kernel");
}

int dfn_sample_pdf(const float* bins, const float* weights, long R, int nb, int ns, const float* u, float* samples,
                   void* stream) {
    if (!bins || !weights || !samples || R < 0 || ns <= 0) return fail(DFN_E_ARG, "dfn_sample_pdf: bad argument");
    if (nb < 2 || nb > 256) return fail(DFN_E_ARG, "dfn_sample_pdf: need 2 <= nb <= 256");
    if (R == 0) return DFN_OK;
    return launched(launch_sample_pdf(bins, weights, R, nb, ns, u, samples, (hipStream_t)stream), "sample_pdf_kernel");
}

int dfn_composite(const float* sigma, const float* feat, int K, long N, float* sigma_sum, float* feat_w,
                  void* stream) {
    if (!sigma || !feat || !sigma_sum || !feat_w || K < 1 || N < 0) return fail(DFN_E_ARG, "dfn_composite: bad argument");
    if (N == 0) return DFN_OK;
    return launched(launch_composite(sigma, feat, K, N, sigma_sum, feat_w, (hipStream_t)stream), "composite_kernel");
}

int dfn_volume_weights(const float* z, const float* ray, const float* sigma, long R, int S, float last_dist,
                       float* weights, void* stream) {
    if (!z || !ray || !sigma || !weights || R < 0) return fail(DFN_E_ARG, "dfn_volume_weights: bad argument");
    if (S < 1 || S > 1024) return fail(DFN_E_ARG, "dfn_volume_weights: need 1 <= S <= 1024");
    if (R == 0) return DFN_OK;
    return launched(launch_volume_weights(z, ray, sigma, R, S, last_dist, weights, (hipStream_t)stream), "volume_weights_kernel");
}

int dfn_composite_grad(const float* sigma, const float* feat, int K, long N, const float* d_sigma_sum, const float* d_feat_w,
                       float* d_sigma, float* d_feat, void* stream) {
    if (!sigma || !feat || !d_sigma || !d_feat || K < 1 || N < 0) return fail(DFN_E_ARG, "dfn_composite_grad: bad argument");
    if (N == 0) return DFN_OK;
    return launched(launch_composite_grad(sigma, feat, K, N, d_sigma_sum, d_feat_w, d_sigma, d_feat, (hipStream_t)stream), "composite_grad_kernel");
}

int dfn_volume_weights_grad(const float* z, const float* ray, const float* sigma, long R, int S, float last_dist,
                            const float* d_weights, float* d_sigma, void* stream) {
    if (!z || !ray || !sigma || !d_weights || !d_sigma || R < 0)
        return fail(DFN_E_ARG, "dfn_volume_weights_grad: bad argument");
    if (S < 1 || S > 1024) return fail(DFN_E_ARG, "dfn_volume_weights_grad: need 1 <= S <= 1024");
    if (R == 0) return DFN_OK;
    return launched(launch_volume_weights_grad(z, ray, sigma, R, S, last_dist, d_weights, d_sigma, (hipStream_t)stream), "volume_weights_grad_kernel");
}

int dfn_to8b(const float* x, long n, uint8_t* out, void* stream) {
    if (!x || !out || n < 0) return fail(DFN_E_ARG, "dfn_to8b: bad argument");
    if (n == 0) return DFN_OK;
    return launched(launch_to8b(x, n, out, (hipStream_t)stream), "to8b_kernel");
}

int dfn_debug_mfma_chain(int tier, int lds_reads_per_2, int valu_per_2, const void* fragments, const void* operands_b, int iters,
                         int blocks, float* out, uint64_t* clock, void* stream) {
    if (no_width(tier, "dfn_debug_mfma_chain") != DFN_OK) return DFN_E_ARG;
    if ((tier != DFN_TIER_BF16 && tier != DFN_TIER_F16) || !fragments || !operands_b || !out || !clock || iters <= 0 || blocks <= 0)
        return fail(DFN_E_ARG, "dfn_debug_mfma_chain: bad argument");
    return launched(launch_mfma_chain(tier == DFN_TIER_F16, lds_reads_per_2, valu_per_2, fragments, operands_b, iters, blocks, out,
                                      (unsigned long long*)clock, (hipStream_t)stream),
                    "mfma_chain_kernel (variants: (0, 0) and (2, 4))");
}

int dfn_debug_clock_probe(uint64_t* probe) {
    g_clock_probe = (unsigned long long*)probe;
    return DFN_OK;
}

long dfn_mfma16_map(int32_t* out, long capacity) {
    constexpr long N = 1024;
    if (out) {
        if (capacity < N) return fail(DFN_E_SIZE, "dfn_mfma16_map: capacity too small");
        for (int lane = 0; lane < 64; ++lane) {
            out[lane] = (int32_t)m16_dma_off(lane);
            for (int j = 0; j < 4; ++j) out[64 + 64 * j + lane] = (int32_t)m16_lane_off(lane, 2) + m16_read_off(j, 2);
            for (int T = 0; T < 2; ++T) out[320 + 64 * T + lane] = (int32_t)m16_lane_off(lane, 1) + m16_read_off(T, 1);
            for (int e = 0; e < 8; ++e) out[448 + 8 * lane + e] = m16_feat(lane >> 4, e);
            out[960 + lane] = 8 * m16_bias_oct(lane);
        }
    }
    return N;
}
int dfn_debug_mfma16_layout(float* out, void* stream) {
    if (!out) return fail(DFN_E_ARG, "dfn_debug_mfma16_layout: bad argument");
    return launched(launch_mfma16_probe(out, (hipStream_t)stream), "mfma16_probe_kernel");
}
int dfn_debug_mfma_layout(float* out, void* stream) {
    if (!out) return fail(DFN_E_ARG, "dfn_debug_mfma_layout: bad argument");
    return launched(launch_mfma_probe(out, (hipStream_t)stream), "mfma_probe_kernel");
}

}  // extern "C"
