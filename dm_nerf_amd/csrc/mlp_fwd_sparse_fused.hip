// mlp_fwd_sparse_fused.hip -- the full network over a selection with the fused-heads blob (called by dmnerf_mlp_fwd_rays_sel,
// mlp_fwd_sparse.hip, which has validated the arguments; kernel: mlp_fwd_sel_impl.h)
#include "mlp_fwd_sel_impl.h"

int dmn_mlp_fwd_rays_sel_fused(const float* d_blob, int ins_num, const float* d_rays_o, const float* d_rays_d, const float* d_z,
                                int64_t N, int S, const int* d_sel, const int* d_count, float* d_raw, hipStream_t stream) {
    MlpSelArgs a{};
    a.blob = d_blob; a.L = make_layout(ins_num, true); a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z;
    a.raw = d_raw; a.M = N * S; a.S = S; a.sel = d_sel; a.count = d_count;
    return launch_sel<true>(a, stream);
}
