// mlp_fwd_points.hip -- the density of the field at free points and on a regular grid: sigma [M], or the occupancy of it.
//
// mesh_main (tools/mesh_generator.py:27-63) asks the fine network for the density on a 256^3 grid.  It builds the grid points on
// the host, embeds every chunk into [n, 90] (63 position columns + the encoding of a zero direction), runs all three heads and
// keeps column 3.  The density depends on neither the direction nor the heads, so this is mlp_fwd_density_kernel
// (mlp_fwd_density.hip) with another front and another back: the same body (density_of_point below -- encoding, mlps.0, seven
// trunk stages, density_linear), 7680 MFMAs per 32 samples instead of 10880 (C = 14), no [n, 90] tensor.
//
// density_of_point repeats mlp_fwd_density_kernel's statements instead of sharing a header with it: lifted into a function, that
// kernel came out of the compiler with the same instructions but other register numbers and one branch inverted, and its emitted
// code is what the frame benchmark runs.  tests/test_gpu_occupancy.py holds the two bodies together bit for bit.
//
//   prologue P (points):  sample m reads pts[m, 0..2].
//   prologue G (grid):    sample m of the slab [m0, m0 + M) of a dim^3 grid computes its own point -- make_3D_grid +
//                         grid_within_bound (tools/visualizer.py:111-155) and the axis swap of mesh_generator.py:28-29, in the
//                         reference's own order of f32 roundings; no point tensor exists.
//   epilogue S:           sigma[m].
//   epilogue O:           occ[m] = 1 - exp(-relu(sigma) * voxel)   (mesh_generator.py:54-60), full-precision expf.
#include <hip/hip_runtime.h>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "layout.h"
#include "mlp_common.h"

using namespace dmn;

namespace {

constexpr int DENSITY_QUARTERS = 1 + 5 * 4 + 1 + 2 * 4 + 1;      // w0 | st0..st4 | w5pe | st5 st6 | the look-ahead quarter = 31
static_assert(DENSITY_QUARTERS <= N_QUARTERS - 2 * 4, "the look-ahead quarter must exist in the fused-heads blob as well");

// the compiler may not assume that two uses of x are the same value (keeps an index out of a register across the MFMA stream)
__device__ __forceinline__ int density_fresh(int x) { asm volatile("" : "+v"(x)); return x; }

// Sigma of one point per lane pair.  The weight stream is read as mlp_fwd_density_kernel reads it: the ordinary forward blob or the
// fused-heads blob, the trunk's 30 quarters and the look-ahead quarter behind them.
// lds: [ring 2 x 64 KiB][table 16 KiB] of the workgroup (256 threads, all of them call).  Returns sigma of this lane's point in
// both halves (lanes l and l + 32 hold the same sample).
__device__ __forceinline__ float density_of_point(const float* __restrict__ blob, const BlobLayout& L, float* lds, float px, float py, float pz,
                                                  int lane, int half, int wave) {
    const float pt[3] = {px, py, pz};
    float* const tab = lds + RING_FLOATS;
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
    const f32x4* wd = reinterpret_cast<const f32x4*>(tab + L.w_den + density_fresh(half) * 128);
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
    return part + __shfl_xor(part, 32) + tab[L.b_den];
}

constexpr int GRID_DIM_MAX = 1024;            // dim^3 <= 2^30: the grid index is 32-bit arithmetic

struct PointsArgs {
    const float* blob;
    BlobLayout L;
    const float* pts;      // P: [M, 3]
    const float* t;        // G: [dim] = linspace(lo, hi, dim)
    float s[3];            // G: extents / (hi - lo)
    float R[12];           // G: rows 0..2 of the 4 x 4 transform, row-major
    unsigned dim;          // G
    unsigned m0;           // G: first grid index of the slab
    float* out;            // [M]
    int64_t M;
    float voxel;           // O
};

template <bool GRID, bool OCC>
__global__ __launch_bounds__(256) void mlp_fwd_points_kernel(const PointsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];          // [ring 2 x 64 KiB][table 16 KiB]
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (waves beyond the end of the batch and tail lanes: exact duplicates, as in mlp_fwd_kernel)
    const int64_t nblk = (a.M + 31) / 32;
    const int64_t blk_raw = (int64_t)blockIdx.x * 4 + wave;
    const int64_t blk = blk_raw < nblk ? blk_raw : nblk - 1;
    const int64_t m_in = blk * 32 + (lane & 31);
    const int64_t m = m_in < a.M ? m_in : a.M - 1;

    float pt[3];
    if constexpr (GRID) {
        const unsigned g = a.m0 + (unsigned)m;                            // < dim^3 <= 2^30 (checked by the caller)
        const unsigned gj = g / a.dim, k = g - gj * a.dim;
        const unsigned i = gj / a.dim, j = gj - i * a.dim;
        // grid_3d = grid_3d_norm * scale (visualizer.py:121)
        const float x = __fmul_rn(a.t[i], a.s[0]), y = __fmul_rn(a.t[j], a.s[1]), z = __fmul_rn(a.t[k], a.s[2]);
        // (R_r * grid_3d).sum(-1) + trans (:127-133): three products, summed left to right, each rounded to f32 -- no fma
        float q[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            q[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a.R[4 * r + 0], x), __fmul_rn(a.R[4 * r + 1], y)), __fmul_rn(a.R[4 * r + 2], z)),
                             a.R[4 * r + 3]);
        // [:, :, [0, 2, 1]], column 1 negated (mesh_generator.py:28-29)
        pt[0] = q[0]; pt[1] = -q[2]; pt[2] = q[1];
    } else {
        pt[0] = a.pts[m * 3 + 0]; pt[1] = a.pts[m * 3 + 1]; pt[2] = a.pts[m * 3 + 2];
    }
    const float sigma = density_of_point(a.blob, a.L, lds, pt[0], pt[1], pt[2], lane, half, wave);
    float v = sigma;
    if constexpr (OCC) {
        const float r = sigma < 0.f ? 0.f : sigma;                        // F.relu: a NaN stays one
        v = __fsub_rn(1.0f, expf(__fmul_rn(-r, a.voxel)));                // sigma <= 0: exp(-0 * voxel) = 1, occ = 0 exactly
    }
    const int64_t ms = blk * 32 + (density_fresh(lane) & 31);
    if (ms < a.M && density_fresh(half) == 0) a.out[ms] = v;
}

template <bool GRID, bool OCC>
int launch(const PointsArgs& a, const char* what, void* stream) {
    unsigned grid;
    if (int rc = dmn_mlp_grid(what, a.M, &grid)) return rc;
    constexpr int LDS = LDS_FLOATS * sizeof(float);                      // 147 456 B: one workgroup per CU, as the full kernel
    if (int rc = dmn_allow_lds<mlp_fwd_points_kernel<GRID, OCC>, LDS>(what, "")) return rc;
    hipLaunchKernelGGL((mlp_fwd_points_kernel<GRID, OCC>), dim3(grid), dim3(256), LDS, (hipStream_t)stream, a);
    return dmn_check_launch(what);
}

}  // namespace

extern "C" int dmnerf_mlp_fwd_points_density(const float* d_blob, int ins_num, const float* d_pts, int64_t M, float* d_out,
                                             float voxel, void* stream) {
    const char* what = "mlp_fwd_points_density";
    int rc = dmn_check_ins_num(what, ins_num);
    if (rc) return rc;
    if (M < 0 || voxel != voxel) return dmn_fail(DMNERF_E_ARG, "%s: bad M=%lld voxel=%g", what, (long long)M, (double)voxel);
    if (!dmn_batch_given(&rc, what, M, {d_blob, d_pts, d_out})) return rc;
    PointsArgs a{};
    a.blob = d_blob; a.L = make_layout(ins_num); a.pts = d_pts; a.out = d_out; a.M = M; a.voxel = voxel;
    return voxel < 0.f ? launch<false, false>(a, what, stream) : launch<false, true>(a, what, stream);
}

extern "C" int dmnerf_occupancy_slab(const float* d_blob, int ins_num, const float* d_t, int dim, const float* scale,
                                     const float* transform, int64_t m0, int64_t M, float* d_out, float voxel, void* stream) {
    const char* what = "occupancy_slab";
    int rc = dmn_check_ins_num(what, ins_num);
    if (rc) return rc;
    if (dim < 1 || dim > GRID_DIM_MAX) return dmn_fail(DMNERF_E_ARG, "%s: dim %d outside 1 .. %d", what, dim, GRID_DIM_MAX);
    const int64_t total = (int64_t)dim * dim * dim;
    if (m0 < 0 || M < 0 || m0 > total || M > total - m0)
        return dmn_fail(DMNERF_E_ARG, "%s: slab [%lld, %lld + %lld) leaves the %d^3 grid", what, (long long)m0, (long long)m0, (long long)M, dim);
    if (voxel != voxel) return dmn_fail(DMNERF_E_ARG, "%s: voxel is NaN", what);
    if (!scale || !transform) return dmn_fail(DMNERF_E_ARG, "%s: null scale / transform", what);
    if (!dmn_batch_given(&rc, what, M, {d_blob, d_t, d_out})) return rc;
    PointsArgs a{};
    a.blob = d_blob; a.L = make_layout(ins_num); a.t = d_t; a.dim = (unsigned)dim; a.m0 = (unsigned)m0; a.out = d_out; a.M = M; a.voxel = voxel;
    for (int i = 0; i < 3; ++i) a.s[i] = scale[i];
    for (int i = 0; i < 12; ++i) a.R[i] = transform[i];
    return voxel < 0.f ? launch<true, false>(a, what, stream) : launch<true, true>(a, what, stream);
}
