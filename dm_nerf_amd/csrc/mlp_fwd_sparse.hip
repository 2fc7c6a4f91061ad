// mlp_fwd_sparse.hip -- the fused PE + DM-NeRF MLP forward on rays over a SELECTION of the samples (csrc/skip.hip makes one).
//
// A render that skips empty space (dmnerf_render_rays_fwd_fine_skip, api.hip) evaluates the networks only at the samples whose
// cell of the occupancy bit grid is set.  The two kernels here are the bodies of mlp_fwd_kernel (mlp_fwd_impl.h) and
// mlp_fwd_density_kernel (mlp_fwd_density_impl.h) instantiated with SEL: the same gemm_quarter calls on the same operands in the
// same order, so a selected row is bit-identical to the same row of dmnerf_mlp_fwd_rays / dmnerf_mlp_fwd_rays_density.
//   sample index   a lane's sample is sel[blk * 32 + lane % 32]; its ray is sel[..] / S; it writes row sel[..].  Tail lanes and
//                  tail waves duplicate the last selected sample.  Rows that are not selected are never touched.
//   batch size     read from *d_count on the device.  The launch is sized for the worst case N * S; a workgroup beyond
//                  ceil(count / 32) / 4 leaves as a whole before the DMA ring and the first barrier.  Nothing reaches the host,
//                  so the chain select -> network can be captured in a graph and replayed on another grid.
// sel [count] is read at indices < count only and d_count is one int32.
#include "mlp_fwd_density_impl.h"
#include "mlp_fwd_sel_impl.h"

int dmn_mlp_fwd_rays_sel_fused(const float* d_blob, int ins_num, const float* d_rays_o, const float* d_rays_d, const float* d_z,
                                int64_t N, int S, const int* d_sel, const int* d_count, float* d_raw, hipStream_t stream);   // mlp_fwd_sparse_fused.hip

namespace {

struct DensitySelArgs {
    const float* blob;
    BlobLayout L;
    const float* rays_o;
    const float* rays_d;
    const float* z;
    float* sigma;          // [M]; entries sel[0 .. count) are written
    int64_t M;             // worst-case batch (sizes the launch)
    int S;
    const int* sel;
    const int* count;
};

__global__ __launch_bounds__(256) void mlp_fwd_density_sel_kernel(const DensitySelArgs a) {
    mlp_fwd_density_body<true>(a);
}

}  // namespace

extern "C" int dmnerf_mlp_fwd_rays_sel(const float* d_blob, int ins_num, int fused_heads, const float* d_rays_o,
                                       const float* d_rays_d, const float* d_z, int64_t N, int S,
                                       const int* d_sel, const int* d_count, float* d_raw, void* stream) {
    const char* who = "mlp_fwd_rays_sel";
    int rc = dmn_check_rays(who, ins_num, N, S, true);
    if (rc) return rc;
    if (fused_heads != 0 && fused_heads != 1) return dmn_fail(DMNERF_E_ARG, "%s: fused_heads %d unsupported", who, fused_heads);
    if (!dmn_batch_given(&rc, who, N, {d_blob, d_rays_o, d_rays_d, d_z, d_sel, d_count, d_raw})) return rc;
    if (fused_heads) return dmn_mlp_fwd_rays_sel_fused(d_blob, ins_num, d_rays_o, d_rays_d, d_z, N, S, d_sel, d_count, d_raw, (hipStream_t)stream);
    MlpSelArgs a{};
    a.blob = d_blob; a.L = make_layout(ins_num); a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z;
    a.raw = d_raw; a.M = N * S; a.S = S; a.sel = d_sel; a.count = d_count;
    return launch_sel<false>(a, (hipStream_t)stream);
}

extern "C" int dmnerf_mlp_fwd_rays_density_sel(const float* d_blob, int ins_num, const float* d_rays_o,
                                               const float* d_rays_d, const float* d_z, int64_t N, int S,
                                               const int* d_sel, const int* d_count, float* d_sigma, void* stream) {
    const char* who = "mlp_fwd_rays_density_sel";
    int rc;
    if (!dmn_rays_given(&rc, who, ins_num, N, S, true, {d_blob, d_rays_o, d_rays_d, d_z, d_sel, d_count, d_sigma})) return rc;
    DensitySelArgs a{};
    a.blob = d_blob; a.L = make_layout(ins_num); a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z;
    a.sigma = d_sigma; a.M = N * S; a.S = S; a.sel = d_sel; a.count = d_count;
    constexpr int LDS = LDS_FLOATS * sizeof(float);
    return dmn_launch_mlp<mlp_fwd_density_sel_kernel, LDS>(who, false, a, (hipStream_t)stream);
}
