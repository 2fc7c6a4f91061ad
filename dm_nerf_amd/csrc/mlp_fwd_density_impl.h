// mlp_fwd_density_impl.h -- body of the density-only forward on rays (entry points: mlp_fwd_density.hip, mlp_fwd_sparse.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "layout.h"
#include "mlp_common.h"

using namespace dmn;

namespace {

constexpr int DENSITY_QUARTERS = 1 + 5 * 4 + 1 + 2 * 4 + 1;      // w0 | st0..st4 | w5pe | st5 st6 | the look-ahead quarter = 31
static_assert(DENSITY_QUARTERS <= N_QUARTERS - 2 * 4, "the look-ahead quarter must exist in the fused-heads blob as well");

// The kernel body, shared by mlp_fwd_density_kernel (mlp_fwd_density.hip) and the kernel over a selection (mlp_fwd_sparse.hip).
// SEL: the batch is a.sel[0 .. *a.count), exactly as in mlp_fwd_impl.h::mlp_fwd_body; without it M is a.M and nothing changes.
template <bool SEL, class Args>
__device__ __forceinline__ void mlp_fwd_density_body(const Args& a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];          // [ring 2 x 64 KiB][table 16 KiB]
    float* const tab = lds + RING_FLOATS;
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (waves beyond the end of the batch and tail lanes: exact duplicates, as in mlp_fwd_kernel)
    int64_t M = a.M;
    if constexpr (SEL) M = *a.count;                                      // wave-uniform: one scalar load
    const int64_t nblk = (M + 31) / 32;
    if constexpr (SEL) {
        if ((int64_t)blockIdx.x * 4 >= nblk) return;                      // the whole workgroup, before the ring and any barrier
    }
    const int64_t blk_raw = (int64_t)blockIdx.x * 4 + wave;
    const int64_t blk = blk_raw < nblk ? blk_raw : nblk - 1;
    auto fresh = [](int x) -> int { asm volatile("" : "+v"(x)); return x; };
    const int64_t m_in = blk * 32 + (lane & 31);
    int64_t m = m_in < M ? m_in : M - 1;
    if constexpr (SEL) m = a.sel[m];                                      // (sel is never read at or beyond count)

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
    if (ms < M && fresh(half) == 0) {
        if constexpr (SEL) a.sigma[a.sel[ms]] = sigma;
        else a.sigma[ms] = sigma;
    }
}

}  // namespace
