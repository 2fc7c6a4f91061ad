// mlp_split.hip -- opt-in split-bf16 inference entry point + the split-plane weight packer (kernel: mlp_split_impl.h)
#include "mlp_split_impl.h"

namespace {

// ---- split packer: stream words from the flat f32 parameters ------------------------------------------------
__device__ __forceinline__ unsigned plane_bits(float x, int plane) {
    unsigned u = __float_as_uint(x);
    if (plane == 0) return u >> 16;
    const float r = x - __uint_as_float(u & 0xffff0000u);
    u = __float_as_uint(r);
    if (plane == 1) return u >> 16;
    const float s = r - __uint_as_float(u & 0xffff0000u);
    return __float_as_uint(s) >> 16;
}

__global__ void pack_split_kernel(const float* __restrict__ flat, const int* __restrict__ idx, unsigned* __restrict__ words, int64_t n_words) {
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * blockDim.x) {
        unsigned out = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int id = idx[2 * w + e];
            if (id >= 0) out |= plane_bits(flat[id & 0x0fffffff], id >> 28) << (16 * e);
        }
        words[w] = out;
    }
}

template <int OBX>
struct Family { static constexpr auto kernel = mlp_split_kernel<OBX>; };

}  // namespace

extern "C" int dmnerf_pack_split(const float* d_flat, const int32_t* d_idx, float* d_stream_words, int64_t n_words, void* stream) {
    if (!d_flat || !d_idx || !d_stream_words || n_words <= 0) return dmn_fail(DMNERF_E_ARG, "pack_split: bad argument");
    const unsigned blocks = (unsigned)((n_words + 255) / 256 < 8192 ? (n_words + 255) / 256 : 8192);
    hipLaunchKernelGGL(pack_split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_flat, (const int*)d_idx, (unsigned*)d_stream_words, n_words);
    return dmn_check_launch("pack_split");
}

extern "C" int dmnerf_mlp_fwd_rays_split(const float* d_blob_split, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                         const float* d_z, int64_t N, int S, float* d_raw, void* stream) {
    const char* who = "mlp_fwd_rays_split";
    int rc;
    if (!dmn_rays_given(&rc, who, ins_num, N, S, false, {d_blob_split, d_rays_o, d_rays_d, d_z, d_raw})) return rc;
    SplitArgs a{};
    a.blob = d_blob_split; a.L = make_layout(ins_num, true); a.S = make_split_layout(ins_num);
    a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z; a.raw = d_raw; a.M = N * S; a.Sr = S;
    constexpr int LDS = SP_LDS_FLOATS * sizeof(float);
    return dmn_launch_mlp_obx<Family, LDS, false>(who, who, true, a.S.OBX, a.S.C, a, (hipStream_t)stream);
}
