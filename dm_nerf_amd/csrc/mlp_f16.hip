// mlp_f16.hip -- opt-in split-f16 ("f16x2") inference entry point + the two-plane weight packer (kernel: mlp_f16_impl.h)
#include "mlp_f16_impl.h"

namespace {

// ---- packer: stream words (two f16 each) from the flat f32 parameters; planes by round-to-nearest (offline: free)
__device__ __forceinline__ unsigned plane_bits_f16(float x, int plane) {
    const _Float16 hi = (_Float16)x;
    if (plane == 0) return (unsigned)__builtin_bit_cast(unsigned short, hi);
    const _Float16 lo = (_Float16)(x - (float)hi);
    return (unsigned)__builtin_bit_cast(unsigned short, lo);
}

__global__ void pack_f16_kernel(const float* __restrict__ flat, const int* __restrict__ idx, unsigned* __restrict__ words, int64_t n_words) {
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * blockDim.x) {
        unsigned out = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int id = idx[2 * w + e];
            if (id >= 0) out |= plane_bits_f16(flat[id & 0x0fffffff], id >> 28) << (16 * e);
        }
        words[w] = out;
    }
}

template <int OBX>
struct Family { static constexpr auto kernel = mlp_f16_kernel<OBX>; };

}  // namespace

extern "C" int dmnerf_pack_f16(const float* d_flat, const int32_t* d_idx, float* d_stream_words, int64_t n_words, void* stream) {
    if (!d_flat || !d_idx || !d_stream_words || n_words <= 0) return dmn_fail(DMNERF_E_ARG, "pack_f16: bad argument");
    const unsigned blocks = (unsigned)((n_words + 255) / 256 < 8192 ? (n_words + 255) / 256 : 8192);
    hipLaunchKernelGGL(pack_f16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_flat, (const int*)d_idx, (unsigned*)d_stream_words, n_words);
    return dmn_check_launch("pack_f16");
}

#ifdef DMN_F16_TRACE
static long long* g_f16_trace = nullptr;
extern "C" void dmnerf_f16_set_trace(long long* d_trace) { g_f16_trace = d_trace; }
#endif

extern "C" int dmnerf_mlp_fwd_rays_f16(const float* d_blob_f16, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                       const float* d_z, int64_t N, int S, float* d_raw, void* stream) {
    const char* who = "mlp_fwd_rays_f16";
    int rc;
    if (!dmn_rays_given(&rc, who, ins_num, N, S, false, {d_blob_f16, d_rays_o, d_rays_d, d_z, d_raw})) return rc;
    F16Args a{};
    a.blob = d_blob_f16; a.S = make_f16_layout(ins_num);
    a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z; a.raw = d_raw; a.M = N * S; a.Sr = S;
#ifdef DMN_F16_TRACE
    a.trace = g_f16_trace;
#endif
    constexpr int LDS = F16_LDS_FLOATS * sizeof(float);
    return dmn_launch_mlp_obx<Family, LDS, false>(who, who, true, a.S.OBX, a.S.C, a, (hipStream_t)stream);
}
