// mlp_f16_density.hip -- the opt-in split-f16 ("f16x2") network cut off behind density_linear, dense and over a selection.
//
// A frame render that keeps only the fine level needs of the coarse network nothing but sigma (api.hip:
// dmnerf_render_rays_fwd_fine, .._fine_skip).  The kernels are the body of mlp_f16_kernel (mlp_f16_body.inc) with
// DENS: encoding, mlps.0 .. mlps.7 and density_linear, 122 weight groups instead of 140 + OBX and no rgb / ins passes; sigma is
// raw[..., 3] of dmnerf_mlp_fwd_rays_f16 bit for bit.  The weight stream is consumed linearly, so they read a blob of their
// own, the f16 DENSITY blob (layout.h::make_f16_density_layout), which dmnerf_blob_f16_density_from_f16 copies out of the f16 blob
// on the device: no second packer, no change to the fetch schedule.
#include "mlp_f16_impl.h"

namespace {

template <bool SEL>
__global__ __launch_bounds__(256) void mlp_f16_density_kernel(const F16Args a) {
    constexpr int OBX = 1;                                               // (unused: no ins_linear)
    constexpr bool SAVE = false, DENS = true;
#include "mlp_f16_body.inc"
}

void fill_args(F16Args& a, const float* d_blob, int ins_num, const float* d_rays_o, const float* d_rays_d, const float* d_z, int64_t N, int S,
               float* d_sigma) {
    a.blob = d_blob; a.S = make_f16_density_layout(ins_num);
    a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z; a.raw = d_sigma; a.M = N * S; a.Sr = S;
}

constexpr int LDS_BYTES = F16_LDS_FLOATS * sizeof(float);

}  // namespace

extern "C" int64_t dmnerf_blob_f16_density_words(int ins_num) {
    return dmn_ins_num_ok(ins_num) ? make_f16_density_layout(ins_num).total : -1;
}

// table + trunk groups | density groups | zeroed landing groups, all on `stream`
extern "C" int dmnerf_blob_f16_density_from_f16(const float* d_blob_f16, int ins_num, float* d_blob_density, void* stream) {
    if (int rc = dmn_check_ins_num("blob_f16_density_from_f16", ins_num)) return rc;
    if (!d_blob_f16 || !d_blob_density) return dmn_fail(DMNERF_E_ARG, "blob_f16_density_from_f16: null pointer");
    const F16Layout F = make_f16_layout(ins_num), D = make_f16_density_layout(ins_num);
    static_assert(F16_DENSITY_GROUP0 + F16_DENSITY_GROUPS <= 4 + 4 * 16 + 20 + 2 * 16 + 9 + 8 + 2 + 1, "density groups inside the forward stream");
    const int64_t head = F.stream + (int64_t)F16_TRUNK_GROUPS * F16_GROUP_WORDS, den = (int64_t)F16_DENSITY_GROUPS * F16_GROUP_WORDS;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(d_blob_density, d_blob_f16, sizeof(float) * head, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_blob_density + head, d_blob_f16 + F.stream + (int64_t)F16_DENSITY_GROUP0 * F16_GROUP_WORDS, sizeof(float) * den,
                           hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_blob_density + head + den, 0, sizeof(float) * (D.total - head - den), st);
    if (e != hipSuccess) return dmn_fail_hip(e, "blob_f16_density_from_f16");
    return DMNERF_OK;
}

extern "C" int dmnerf_mlp_fwd_rays_density_f16(const float* d_blob_f16_density, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                               const float* d_z, int64_t N, int S, float* d_sigma, void* stream) {
    const char* who = "mlp_fwd_rays_density_f16";
    int rc;
    if (!dmn_rays_given(&rc, who, ins_num, N, S, false, {d_blob_f16_density, d_rays_o, d_rays_d, d_z, d_sigma})) return rc;
    F16Args a{};
    fill_args(a, d_blob_f16_density, ins_num, d_rays_o, d_rays_d, d_z, N, S, d_sigma);
    return dmn_launch_mlp<mlp_f16_density_kernel<false>, LDS_BYTES>(who, true, a, (hipStream_t)stream);
}

extern "C" int dmnerf_mlp_fwd_rays_density_f16_sel(const float* d_blob_f16_density, int ins_num, const float* d_rays_o,
                                                   const float* d_rays_d, const float* d_z, int64_t N, int S, const int* d_sel,
                                                   const int* d_count, float* d_sigma, void* stream) {
    const char* who = "mlp_fwd_rays_density_f16_sel";
    int rc;
    if (!dmn_rays_given(&rc, who, ins_num, N, S, true, {d_blob_f16_density, d_rays_o, d_rays_d, d_z, d_sel, d_count, d_sigma})) return rc;
    F16Args a{};
    fill_args(a, d_blob_f16_density, ins_num, d_rays_o, d_rays_d, d_z, N, S, d_sigma);
    a.sel = d_sel; a.count = d_count;
    return dmn_launch_mlp<mlp_f16_density_kernel<true>, LDS_BYTES>(who, false, a, (hipStream_t)stream);   // (the grid: the worst case count == N * S)
}
