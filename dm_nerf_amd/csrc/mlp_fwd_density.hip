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
#include <hip/hip_runtime.h>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "layout.h"
#include "mlp_common.h"

using namespace dmn;

namespace {

constexpr int DENSITY_QUARTERS = 1 + 5 * 4 + 1 + 2 * 4 + 1;      // w0 | st0..st4 | w5pe | st5 st6 | the look-ahead quarter = 31
static_assert(DENSITY_QUARTERS <= N_QUARTERS - 2 * 4, "the look-ahead quarter must exist in the fused-heads blob as well");

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
    extern __shared__ __attribute__((aligned(16))) float lds[];          // [ring 2 x 64 KiB][table 16 KiB]
    float* const tab = lds + RING_FLOATS;
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (waves beyond the end of the batch and tail lanes: exact duplicates, as in mlp_fwd_kernel)
    const int64_t nblk = (a.M + 31) / 32;
    const int64_t blk_raw = (int64_t)blockIdx.x * 4 + wave;
    const int64_t blk = blk_raw < nblk ? blk_raw : nblk - 1;
    auto fresh = [](int x) -> int { asm volatile("" : "+v"(x)); return x; };
    const int64_t m_in = blk * 32 + (lane & 31);
    const int64_t m = m_in < a.M ? m_in : a.M - 1;

    const float* __restrict__ blob = a.blob;
    const BlobLayout& L = a.L;

    float pt[3];
    {
        const int64_t n = m / a.S;
        const float ox = a.rays_o[n * 3 + 0], oy = a.rays_o[n * 3 + 1], oz = a.rays_o[n * 3 + 2];
        const float dx = a.rays_d[n * 3 + 0], dy = a.rays_d[n * 3 + 1], dz = a.rays_d[n * 3 + 2];
        const float zv = a.z[m];
        // pts = rays_o + rays_d * z   (render.py:49: separate multiply and add, no fma)
        pt[0] = ox + dx * zv; pt[1] = oy + dy * zv; pt[2] = oz + dz * zv;
    }
    f32x16 pe[2];
    // the whole table travels (16 KiB, once per workgroup): w_den / b_den sit behind the heads' biases, in its last 4 KiB
    f32x4 tabv[TAB_FLOATS / 1024];
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(blob) + threadIdx.x;
#pragma unroll
        for (int k = 0; k < TAB_FLOATS / 1024; ++k) tabv[k] = src[k * 256];
    }
    WStream ws;
    // (descriptor bound = what this kernel touches, not L.total: the caller's blob may be the shorter fused-heads one)
    ws_init(ws, blob, L.stream + (int64_t)DENSITY_QUARTERS * QUARTER_FLOATS, lds, lane, wave, L.stream);
    ws_fetch_first(ws);                                                   // quarter 0: mlps.0
    encode<POS_L, 2>(pt, pe, half);                                       // full-range sin/cos under the DMA flight
    {
        f32x4* dst = reinterpret_cast<f32x4*>(tab) + threadIdx.x;
#pragma unroll
        for (int k = 0; k < TAB_FLOATS / 1024; ++k) dst[k * 256] = tabv[k];
    }

    f32x16 h[8], acc[8];
    // ---- mlps.0 : 63 -> 256 (quarter 0)
    ws_prime<8>(ws, lane);
    init_bias_lds<8>(tab + L.b0, acc, half);
    gemm_quarter<0, 8, 8, 8>(ws, pe, acc, lane);
#pragma unroll
    for (int b = 0; b < 8; ++b) h[b] = relu16(acc[b]);

    // ---- trunk: mlps.1 .. mlps.7
#pragma nounroll
    for (int st = 0; st < 7; ++st) {
        init_bias_lds<8>(tab + L.b_stage + st * (int)bias_floats(8), acc, half);
        gemm_quarter<0, 8, 8, 8>(ws, h, acc, lane);
        gemm_quarter<8, 8, 8, 8>(ws, h, acc, lane);
        gemm_quarter<16, 8, 8, 8>(ws, h, acc, lane);
        gemm_quarter<24, 8, 8, 8>(ws, h, acc, lane);
        if (st == 4) {                                                    // skip: cat[h, pts] (dm_nerf.py:87)
            gemm_quarter<0, 8, 8, 8>(ws, pe, acc, lane);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) h[b] = relu16(acc[b]);
    }
    // ---- density_linear(h) (dm_nerf.py:101) on the VALU: 128 features per lane + the other half
    const f32x4* wd = reinterpret_cast<const f32x4*>(tab + L.w_den + fresh(half) * 128);
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const f32x4 w = wd[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = 4 * i + j;
            part = fmaf(h[p >> 4][p & 15], w[j], part);
        }
    }
    const float sigma = part + __shfl_xor(part, 32) + tab[L.b_den];
    const int64_t ms = blk * 32 + (fresh(lane) & 31);
    if (ms < a.M && fresh(half) == 0) a.sigma[ms] = sigma;
}

}  // namespace

extern "C" int dmnerf_mlp_fwd_rays_density(const float* d_blob, int ins_num, const float* d_rays_o,
                                           const float* d_rays_d, const float* d_z, int64_t N, int S,
                                           float* d_sigma, void* stream) {
    if (ins_num < 1 || ins_num + 1 > DMNERF_MAX_LOGITS) return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_density: ins_num %d unsupported", ins_num);
    if (N < 0 || S < 1) return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_density: bad N=%lld S=%d", (long long)N, S);
    if (N == 0) return DMNERF_OK;
    if (!d_blob || !d_rays_o || !d_rays_d || !d_z || !d_sigma) return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_density: null pointer");
    DensityArgs a{};
    a.blob = d_blob; a.L = make_layout(ins_num); a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z;
    a.sigma = d_sigma; a.M = N * S; a.S = S;
    const int64_t nblk = (a.M + 31) / 32;
    const int64_t grid = (nblk + 3) / 4;
    if (grid > 0x7fffffffLL) return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_density: %lld samples is too many for one launch", (long long)a.M);
    constexpr size_t lds_bytes = (size_t)LDS_FLOATS * sizeof(float);     // 147 456 B: one workgroup per CU, as the full kernel
    static DmnOncePerDevice once;
    if (hipError_t e = once.run([] { return hipFuncSetAttribute((const void*)mlp_fwd_density_kernel,
                                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); }); e != hipSuccess)
        return dmn_fail_hip(e, "mlp_fwd_rays_density: hipFuncSetAttribute");
    hipLaunchKernelGGL(mlp_fwd_density_kernel, dim3((unsigned)grid), dim3(256), lds_bytes, (hipStream_t)stream, a);
    return dmn_check_launch("mlp_fwd_rays_density");
}
