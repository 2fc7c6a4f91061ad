// mlp_f16_train.hip -- OPT-IN training forward on the split-f16 MFMA path (args.mfma_split = "f16x2" with grad enabled): the
// inference kernel of mlp_f16_impl.h with SAVE = true -- it also writes the f32 activations (pe, de, h_0..h_7, g1, g2) and the
// 1-bit ReLU masks into the SaveLayout workspace that the backward kernels consume (the f32 ones of mlp_bwd.hip / wgrad.hip as
// well as their split twins).  The stores and the mask packing ride in the MFMA gaps with the rest of the epilogue (four gaps
// per element pair); this translation unit is built with -DDMN_STORE_AUX=2 (csrc/Makefile): the 7.8 GB of row stores per fine launch
// are `nt`, which took the kernel from 2.75 to 2.36 ms (docs/EXPERIMENTS.md section 8).  The forward is the fused-heads function, i.e. exactly the form the re-associated backward
// differentiates; values are f32-class (2e-7 against float64) but not the bitwise fmaf chain of the default path.
#include "mlp_f16_impl.h"

namespace {
template <int OBX>
struct Family { static constexpr auto kernel = mlp_f16_kernel<OBX, true>; };
}  // namespace

#ifdef DMN_F16_TRACE
static long long* g_f16_train_trace = nullptr;
extern "C" void dmnerf_f16_train_set_trace(long long* d_trace) { g_f16_train_trace = d_trace; }
#endif

extern "C" int dmnerf_mlp_fwd_rays_train_f16(const float* d_blob_f16, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                             const float* d_z, int64_t N, int S, float* d_raw, float* d_save, void* stream) {
    const char* who = "mlp_fwd_rays_train_f16";
    int rc;
    if (!dmn_rays_given(&rc, who, ins_num, N, S, false, {d_blob_f16, d_rays_o, d_rays_d, d_z, d_raw, d_save})) return rc;
    F16Args a{};
    a.blob = d_blob_f16; a.S = make_f16_layout(ins_num);
    a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z; a.raw = d_raw; a.save = d_save; a.M = N * S; a.Sr = S;
#ifdef DMN_F16_TRACE
    a.trace = g_f16_train_trace;
#endif
    if (a.M > DMNERF_MAX_TRAIN_SAMPLES)
        return dmn_fail(DMNERF_E_ARG, "%s: %lld samples per launch exceed %lld; split the batch", who, (long long)a.M, (long long)DMNERF_MAX_TRAIN_SAMPLES);
    constexpr int LDS = F16_LDS_FLOATS * sizeof(float);
    return dmn_launch_mlp_obx<Family, LDS, false>(who, who, false, a.S.OBX, a.S.C, a, (hipStream_t)stream);
}
