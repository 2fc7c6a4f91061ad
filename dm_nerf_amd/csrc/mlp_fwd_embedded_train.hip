// mlp_fwd_embedded_train.hip -- DM_NeRF.forward on pre-embedded rows [M, 90] WITH saved activations: the training-mode
// forward of callers that embed the points themselves (networks/dm_nerf.py:80-106 is differentiable; mesh / third-party
// code calls the model directly).  Same kernel template (mlp_fwd_impl.h); the workspace it fills is the one
// dmnerf_mlp_bwd_data / dmnerf_mlp_bwd_weights consume.
#include "mlp_fwd_impl.h"

extern "C" int dmnerf_mlp_fwd_embedded_train(const float* d_blob, int ins_num, const float* d_x, int64_t M,
                                             float* d_raw, float* d_save, void* stream) {
    const char* who = "mlp_fwd_embedded_train";
    int rc = dmn_check_ins_num(who, ins_num);
    if (rc) return rc;
    if (M < 0) return dmn_fail(DMNERF_E_ARG, "%s: M < 0", who);
    if (!dmn_batch_given(&rc, who, M, {d_blob, d_x, d_raw, d_save})) return rc;
    MlpArgs a{};
    a.blob = d_blob; a.L = make_layout(ins_num); a.x = d_x; a.raw = d_raw; a.save = d_save; a.M = M; a.S = 1;
    return launch<true, true>(a, (hipStream_t)stream);
}
