// mlp_fwd_density.hip -- density-only forward of the fused PE + DM-NeRF MLP kernel on rays: sigma [N*S], nothing else.
//
// The coarse level of an inference render feeds the fine level through its compositing WEIGHTS alone (networks/render.py:66-70,
// sample_pdf(z_mid, weights[..., 1:-1])), and the weights depend on the density channel alone (render.py:6-20).  When the caller
// keeps only the fine outputs (render_test, networks/tester.py:71-77) the two heads of the coarse network are work for nothing.
// This kernel is mlp_fwd_kernel (mlp_fwd_impl.h) cut off behind density_linear: positional encoding of the points, mlps.0, the
// seven trunk stages with the skip at stage 4, the VALU dot product -- the same gemm_quarter calls on the same operands in the
// same order, so sigma is bit-identical to raw[..., 3] of dmnerf_mlp_fwd_rays.  7680 MFMAs per 32 samples instead of 10880 (C = 14).
//
// It reads the ordinary forward blob: the trunk is the first 30 quarters of the weight stream and the table offsets it uses
// (b0, b_stage, w_den, b_den) do not depend on the heads' form, so the fused-heads blob (layout.h::make_layout(.., true)) serves
// as well.  No direction encoding, no park area, no logit-block template parameter: one instantiation.
//
// End of the stream: the trunk loop is the full kernel's, unpeeled.  Its last quarter (stage 6, quarter 29) fetches quarter 30
// (rgb_feature's first; the rgb hidden layer's in a fused blob -- it exists in both) and hands over into it like any other; the
// kernel then simply ends.  That costs one unused 64 KiB L2 read and 8 unused ds_read_b128 per workgroup, and keeps one code body.
#include "mlp_fwd_density_impl.h"

namespace {

struct DensityArgs {
    const float* blob;
    BlobLayout L;
    const float* rays_o;
    const float* rays_d;
    const float* z;
    float* sigma;          // [M]
    int64_t M;             // total samples
    int S;                 // samples per ray
};

__global__ __launch_bounds__(256) void mlp_fwd_density_kernel(const DensityArgs a) {
    mlp_fwd_density_body<false>(a);
}

}  // namespace

extern "C" int dmnerf_mlp_fwd_rays_density(const float* d_blob, int ins_num, const float* d_rays_o,
                                           const float* d_rays_d, const float* d_z, int64_t N, int S,
                                           float* d_sigma, void* stream) {
    const char* who = "mlp_fwd_rays_density";
    int rc;
    if (!dmn_rays_given(&rc, who, ins_num, N, S, false, {d_blob, d_rays_o, d_rays_d, d_z, d_sigma})) return rc;
    DensityArgs a{};
    a.blob = d_blob; a.L = make_layout(ins_num); a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z;
    a.sigma = d_sigma; a.M = N * S; a.S = S;
    constexpr int LDS = LDS_FLOATS * sizeof(float);                      // 147 456 B: one workgroup per CU, as the full kernel
    return dmn_launch_mlp<mlp_fwd_density_kernel, LDS>(who, false, a, (hipStream_t)stream);
}
