// dfn_signal.h - launchers of the conditioning-signal kernels (dfn_signal.hip)
#pragma once
#include <hip/hip_runtime.h>
namespace dfn {
constexpr int SIG_MAX_WIN = 8;       // largest attention window (smo_size / smo_torse_size)
// dfn_encode_signal_keep's buffer, float offsets (rows of SIG_MAX_WIN whatever the window): the activations the forward leaves
// (h1 | h2 | e1 | feat), then the backward's scratch for signal_dw12_kernel (the pre-activation gradients d h1 | d h2)
struct SigKeep {
    static constexpr int H1 = 0;                              // [S][256]
    static constexpr int H2 = H1 + SIG_MAX_WIN * 256;         // [S][128]
    static constexpr int E1 = H2 + SIG_MAX_WIN * 128;         // [S][32]
    static constexpr int FT = E1 + SIG_MAX_WIN * 32;          // [S][96]
    static constexpr int DH1 = FT + SIG_MAX_WIN * 96;         // [S][256]
    static constexpr int DH2 = DH1 + SIG_MAX_WIN * 256;       // [S][128]
    static constexpr int TOTAL = DH2 + SIG_MAX_WIN * 128;
};
hipError_t launch_encode_signal(const float* aud_params, const float* exp_params, const float* att_params,
                                const float* auds, const float* exps, int N, const int* frame_ids, int n_frames, int smo,
                                float* out, float* keep, hipStream_t st);
hipError_t launch_encode_signal_torso(const float* att_params, const float* poses, int pose_stride, int N,
                                      const int* frame_ids, int n_frames, int smo, float* out, hipStream_t st);
hipError_t launch_encode_signal_bwd(const float* aud_params, const float* exp_params, const float* att_params,
                                    const float* auds, const float* exps, int N, int frame, int smo, const float* d_out,
                                    float* g_aud, float* g_exp, float* g_att, bool set, const float* kept, hipStream_t st);
hipError_t launch_encode_signal_torso_bwd(const float* att_params, const float* poses, int pose_stride, int N, int frame,
                                          int smo, const float* d_out, float* g_att, bool set, hipStream_t st);
}  // namespace dfn
