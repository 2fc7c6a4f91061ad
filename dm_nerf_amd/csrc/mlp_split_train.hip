// mlp_split_train.hip -- OPT-IN training forward on the split-bf16 MFMA path (args.mfma_split with grad enabled): the
// inference kernel of mlp_split_impl.h with SAVE = true -- it writes the f32 activations (pe, de, h_0..h_7, g1, g2) and the
// 1-bit ReLU masks into the SaveLayout workspace that the f32 backward kernels (mlp_bwd.hip, wgrad.hip, heads.hip) consume.
// The forward is the fused-heads function (no rgb_feature / ins_feature stage), which is exactly the form the re-associated
// backward differentiates; values are f32-class (1e-7 against float64) but not the bitwise fmaf chain of the default path.
#include "mlp_split_impl.h"

namespace {
template <int OBX>
struct Family { static constexpr auto kernel = mlp_split_kernel<OBX, true>; };
}  // namespace

extern "C" int dmnerf_mlp_fwd_rays_train_split(const float* d_blob_split, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                               const float* d_z, int64_t N, int S, float* d_raw, float* d_save, void* stream) {
    const char* who = "mlp_fwd_rays_train_split";
    int rc;
    if (!dmn_rays_given(&rc, who, ins_num, N, S, false, {d_blob_split, d_rays_o, d_rays_d, d_z, d_raw, d_save})) return rc;
    SplitArgs a{};
    a.blob = d_blob_split; a.L = make_layout(ins_num, true); a.S = make_split_layout(ins_num);
    a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z; a.raw = d_raw; a.save = d_save; a.M = N * S; a.Sr = S;
    if (a.M > DMNERF_MAX_TRAIN_SAMPLES)
        return dmn_fail(DMNERF_E_ARG, "%s: %lld samples per launch exceed %lld; split the batch", who, (long long)a.M, (long long)DMNERF_MAX_TRAIN_SAMPLES);
    constexpr int LDS = SP_LDS_FLOATS * sizeof(float);
    return dmn_launch_mlp_obx<Family, LDS, false>(who, who, false, a.S.OBX, a.S.C, a, (hipStream_t)stream);
}
