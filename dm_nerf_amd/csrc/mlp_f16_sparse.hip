// mlp_f16_sparse.hip -- the opt-in split-f16 ("f16x2") network over a SELECTION of the samples (csrc/skip.hip makes one).
//
// The body of mlp_f16_kernel (mlp_f16_body.inc) with SEL: the same f16_pass calls on the same tiles in the same order,
// and a sample is one B-operand column of every MFMA, so a selected row is bit-identical to the same row of
// dmnerf_mlp_fwd_rays_f16 whichever other samples share its wave.  Sample index, batch size and early exit are those of
// dmnerf_mlp_fwd_rays_sel (mlp_fwd_sparse.hip): sel [count] is read at indices < count only, *d_count on the device.
#include "mlp_f16_impl.h"

namespace {

template <int OBX>
__global__ __launch_bounds__(256) void mlp_f16_sel_kernel(const F16Args a) {
    constexpr bool SAVE = false, SEL = true, DENS = false;
#include "mlp_f16_body.inc"
}

template <int OBX>
struct Family { static constexpr auto kernel = mlp_f16_sel_kernel<OBX>; };

}  // namespace

extern "C" int dmnerf_mlp_fwd_rays_f16_sel(const float* d_blob_f16, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                           const float* d_z, int64_t N, int S, const int* d_sel, const int* d_count, float* d_raw,
                                           void* stream) {
    const char* who = "mlp_fwd_rays_f16_sel";
    int rc;
    if (!dmn_rays_given(&rc, who, ins_num, N, S, true, {d_blob_f16, d_rays_o, d_rays_d, d_z, d_sel, d_count, d_raw})) return rc;
    F16Args a{};
    a.blob = d_blob_f16; a.S = make_f16_layout(ins_num);
    a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z; a.raw = d_raw; a.M = N * S; a.Sr = S;
    a.sel = d_sel; a.count = d_count;
    constexpr int LDS = F16_LDS_FLOATS * sizeof(float);                    // (the grid: the worst case count == N * S < 2^31 samples, fits)
    return dmn_launch_mlp_obx<Family, LDS, false>(who, who, false, a.S.OBX, a.S.C, a, (hipStream_t)stream);
}
