// mlp_fwd_fused.hip -- inference on rays with the fused-heads blob (opt-in; kernel: mlp_fwd_impl.h)
// (one translation unit per entry point: the 4 logit-block instantiations of a variant compile in parallel with the others)
#include "mlp_fwd_impl.h"

extern "C" int dmnerf_mlp_fwd_rays_fused(const float* d_blob_fused, int ins_num, const float* d_rays_o,
                                         const float* d_rays_d, const float* d_z, int64_t N, int S,
                                         float* d_raw, void* stream) {
    int rc;
    if (!dmn_rays_given(&rc, "mlp_fwd_rays_fused", ins_num, N, S, false, {d_blob_fused, d_rays_o, d_rays_d, d_z, d_raw})) return rc;
    MlpArgs a{};
    a.blob = d_blob_fused; a.L = make_layout(ins_num, true); a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z;
    a.raw = d_raw; a.M = N * S; a.S = S;
    return launch<false, false, true>(a, (hipStream_t)stream);
}
