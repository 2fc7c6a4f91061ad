// train_skip.hip -- the data movement of a TRAINING step that skips empty space (autograd.run_network_train_skip): the samples the
// select pass of skip.hip flagged are gathered into a compact batch of one-sample rays, the unchanged training kernels (forward with
// saved activations, data gradient, weight gradient) run on that batch, and rows travel between the compact batch and the dense
// [N*S, width] tensors.
//
//   dmnerf_skip_gather_samples  compact row i = the ray (o, d) and the depth z of sample sel[i], copied bit for bit; rows
//                               n_sel <= i < n_pad repeat row n_sel - 1, so a launch over the padded batch reads finite, in-range data.
//   dmnerf_rows_scatter         dst[sel[i]] = src[i] for i < n_sel; no other row of dst is touched (the select pass filled them).
//   dmnerf_rows_gather          dst[i] = src[sel[i]] for i < n_sel, exact zeros for n_sel <= i < n_pad: the transpose of the scatter,
//                               and a zero cotangent for every padded row.
//
// The addressing of the two row kernels is skip_flag_fill_kernel's (skip.hip): width = 4 + C is rarely a multiple of 4
// and a row is not 16-byte aligned, so a block owns the contiguous run of its 256 compact rows and lane t takes floats t, t + 256, ...
// of it (a wave moves 256 consecutive bytes on the compact side); (row, column) advance by (256 / width, 256 % width) per step: no
// division in the loop.  The dense side is addressed through the block's 256 selection entries (LDS).  No atomics: sel is strictly
// ascending, so every dense row has at most one writer.  Nothing allocates or synchronises.  A selection entry outside [0, n_rows)
// is a caller's bug; such a row is not scattered and gathers as zeros (gather_samples: takes the last sample), so that no launch
// reads or writes out of bounds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_WIDTH = 1 << 16;

// One compact row per lane: 7 floats in, 7 floats out.  The one division (sample -> ray) is per lane, outside any loop.
__global__ __launch_bounds__(BLOCK) void gather_samples_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                               const float* __restrict__ z, int64_t M, int S, const int* __restrict__ sel,
                                                               int64_t n_sel, int64_t n_pad, float* __restrict__ o_c,
                                                               float* __restrict__ d_c, float* __restrict__ z_c) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_pad) return;
    int64_t m = sel[i < n_sel ? i : n_sel - 1];
    if (m < 0 || m >= M) m = M - 1;
    const int64_t n = m / S;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o_c[i * 3 + a] = rays_o[n * 3 + a];
        d_c[i * 3 + a] = rays_d[n * 3 + a];
    }
    z_c[i] = z[m];
}

// The block's rows are compact rows [r0, r0 + 256): floats [r0 * width, ...) of the compact tensor, one contiguous run.
// TO_DENSE: dense[sel[r]] = compact[r] for r < n_sel.  Otherwise: compact[r] = r < n_sel ? dense[sel[r]] : 0 for r < n_pad.
template <bool TO_DENSE>
__global__ __launch_bounds__(BLOCK) void rows_move_kernel(float* __restrict__ dense, float* __restrict__ compact, const int* __restrict__ sel,
                                                          int64_t n_sel, int64_t n_pad, int64_t n_rows, int width) {
    __shared__ int64_t block_row[BLOCK];                              // first float of the dense row, or -1: no such row
    const int64_t r0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t last = TO_DENSE ? n_sel : n_pad;                    // compact rows this launch walks
    {
        const int64_t r = r0 + threadIdx.x;
        int64_t row = -1;
        if (r < n_sel) {
            const int64_t m = sel[r];
            if (m >= 0 && m < n_rows) row = m * width;
        }
        block_row[threadIdx.x] = row;
    }
    __syncthreads();
    const int nrows = (int)(last - r0 < BLOCK ? last - r0 : BLOCK);
    const int run = nrows * width;                                    // <= 256 * 65536 floats
    float* __restrict__ c_run = compact + r0 * width;
    const int dr = BLOCK / width, dc = BLOCK - dr * width;
    int r = threadIdx.x / width, c = threadIdx.x - r * width;
    for (int i = threadIdx.x; i < run; i += BLOCK) {
        const int64_t row = block_row[r];
        if (TO_DENSE) {
            if (row >= 0) dense[row + c] = c_run[i];
        } else {
            c_run[i] = row >= 0 ? dense[row + c] : 0.f;
        }
        r += dr; c += dc;
        if (c >= width) { c -= width; ++r; }
    }
}

// the checks the three entries share: sizes, then M' <= Mp and M' <= the dense rows, which fit the int32 selection
int check_sizes(const char* who, int64_t n_sel, int64_t n_pad, int64_t n_rows) {
    if (n_sel < 0 || n_pad < 0 || n_rows < 0)
        return dmn_fail(DMNERF_E_ARG, "%s: bad sizes n_sel=%lld n_pad=%lld rows=%lld", who, (long long)n_sel, (long long)n_pad, (long long)n_rows);
    if (n_rows >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "%s: %lld samples do not fit the int32 selection", who, (long long)n_rows);
    if (n_sel > n_pad) return dmn_fail(DMNERF_E_ARG, "%s: n_sel %lld exceeds the padded length %lld", who, (long long)n_sel, (long long)n_pad);
    if (n_sel > n_rows) return dmn_fail(DMNERF_E_ARG, "%s: n_sel %lld exceeds the %lld samples", who, (long long)n_sel, (long long)n_rows);
    if (n_pad >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "%s: padded length %lld does not fit int32", who, (long long)n_pad);
    return DMNERF_OK;
}

}  // namespace

extern "C" int dmnerf_skip_gather_samples(const float* d_rays_o, const float* d_rays_d, const float* d_z, int64_t N, int S, const int* d_sel,
                                          int64_t n_sel, int64_t n_pad, float* d_o, float* d_d, float* d_zc, void* stream) {
    if (int rc = dmn_check_rays("skip_gather_samples", 1, N, S, true)) return rc;     // (no network here: ins_num 1 always passes)
    if (int rc = check_sizes("skip_gather_samples", n_sel, n_pad, N * S)) return rc;
    if (n_pad == 0) return DMNERF_OK;
    if (n_sel == 0) return dmn_fail(DMNERF_E_ARG, "skip_gather_samples: %lld padded rows but no selected sample to repeat", (long long)n_pad);
    if (!d_rays_o || !d_rays_d || !d_z || !d_sel || !d_o || !d_d || !d_zc) return dmn_fail(DMNERF_E_ARG, "skip_gather_samples: null pointer");
    hipLaunchKernelGGL(gather_samples_kernel, dim3((unsigned)((n_pad + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, d_rays_o,
                       d_rays_d, d_z, N * S, S, d_sel, n_sel, n_pad, d_o, d_d, d_zc);
    return dmn_check_launch("skip_gather_samples");
}

extern "C" int dmnerf_rows_scatter(const float* d_src, int64_t n_pad, const int* d_sel, int64_t n_sel, float* d_dst, int64_t n_rows, int width,
                                   void* stream) {
    if (int rc = check_sizes("rows_scatter", n_sel, n_pad, n_rows)) return rc;
    if (width < 1 || width > MAX_WIDTH) return dmn_fail(DMNERF_E_ARG, "rows_scatter: bad width %d", width);
    if (n_sel == 0) return DMNERF_OK;
    if (!d_src || !d_sel || !d_dst) return dmn_fail(DMNERF_E_ARG, "rows_scatter: null pointer");
    hipLaunchKernelGGL(rows_move_kernel<true>, dim3((unsigned)((n_sel + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, d_dst,
                       const_cast<float*>(d_src), d_sel, n_sel, n_pad, n_rows, width);
    return dmn_check_launch("rows_scatter");
}

extern "C" int dmnerf_rows_gather(const float* d_src, int64_t n_rows, const int* d_sel, int64_t n_sel, float* d_dst, int64_t n_pad, int width,
                                  void* stream) {
    if (int rc = check_sizes("rows_gather", n_sel, n_pad, n_rows)) return rc;
    if (width < 1 || width > MAX_WIDTH) return dmn_fail(DMNERF_E_ARG, "rows_gather: bad width %d", width);
    if (n_pad == 0) return DMNERF_OK;
    if (!d_dst || (n_sel > 0 && (!d_src || !d_sel))) return dmn_fail(DMNERF_E_ARG, "rows_gather: null pointer");
    hipLaunchKernelGGL(rows_move_kernel<false>, dim3((unsigned)((n_pad + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                       const_cast<float*>(d_src), d_dst, d_sel, n_sel, n_pad, n_rows, width);
    return dmn_check_launch("rows_gather");
}
