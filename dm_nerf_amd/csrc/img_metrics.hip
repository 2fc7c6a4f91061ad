// img_metrics.hip -- SSIM and PSNR of rendered frames against their ground truth, on the device: the two image scores of
// render_test (networks/tester.py:89-90) and manipulator_eval (networks/manipulator.py:277-278),
//     peak_signal_noise_ratio(rgb, gt, data_range=1)   and   structural_similarity(rgb, gt, multichannel=True, data_range=1).
//
// The definition implemented here is the documented algorithm of scikit-image 0.18 (the version the reference pins), WRITTEN DOWN
// WITHOUT THE LIBRARY AT HAND (it is not installed where this was developed; tests/test_img_metrics_restate.py compares against
// it wherever `import skimage` succeeds).  Per channel, in float64:
//     ux, uy, uxx, uyy, uxy = 7x7 box means of x, y, x x, y y, x y                      (x = pred, y = gt, converted to f64)
//     vx = 49/48 (uxx - ux ux),  vy = 49/48 (uyy - uy uy),  vxy = 49/48 (uxy - ux uy)   (use_sample_covariance=True)
//     S  = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  C1 = 1e-4, C2 = 9e-4 (data_range 1)
// and the map is cropped by 3 on every side before its mean: only the (H-6)(W-6) windows that lie wholly inside the image count,
// so no border rule exists.  Frame SSIM = mean over the channels of the per-channel means.  PSNR: difference and square in f32,
// summed in f64 (np.mean(..., dtype=float64) of an f32 array), 10 log10(1 / mse) in f64, +inf for mse == 0.
//
//   im_tile_kernel    a workgroup owns IM_TH x IM_TW windows of one frame: it stages the pixels under them (a 6-pixel apron on
//                     two sides, all channels, both images) through LDS once, adds the squared error of the pixels it owns, and
//                     per channel forms the five horizontal 7-tap sums (LDS, f64), then the vertical ones, evaluates S and
//                     reduces (lanes in a fixed order, then the waves in index order) to one f64 partial per channel plus one for the
//                     squared error: d_work [P][C + 1][workgroups of a frame], plain stores
//   im_finish_kernel  one workgroup per frame sums the partials of each quantity in index order and writes the results
// Every window sum adds its 7 taps directly (no running add-new / subtract-old sum, whose rounding error grows along a row), and
// there is no floating-point atomic: a result does not depend on which workgroup finishes first, nor on P (the tiles of a frame
// are the same whatever the batch), so it is bit-identical from run to run.  No allocation, no synchronisation: capturable.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"

namespace {

constexpr int IM_WIN = 7;                       // win_size of structural_similarity's default
constexpr int IM_PAD = IM_WIN - 1;
constexpr int IM_TH = 16, IM_TW = 32;           // windows per workgroup: 480 x 640 -> 30 x 20 = 600 workgroups per frame
constexpr int IM_RH = IM_TH + IM_PAD, IM_RW = IM_TW + IM_PAD;      // staged pixels: 22 x 38
constexpr int IM_MAXC = 4;
constexpr int IM_THREADS = 256, IM_WAVES = IM_THREADS / 64;
constexpr int IM_MAX_DIM = 1 << 15;             // H, W (offsets inside a frame stay far below 2^31 floats x channels in int64)
constexpr int IM_CHUNK = 512;                   // partials per quantity staged per step of the finish kernel

struct ImTiles { int nty, ntx; int64_t per_frame; };
__host__ __device__ inline ImTiles im_tiles(int H, int W) {
    ImTiles t;
    t.nty = (H - IM_PAD + IM_TH - 1) / IM_TH;
    t.ntx = (W - IM_PAD + IM_TW - 1) / IM_TW;
    t.per_frame = (int64_t)t.nty * t.ntx;
    return t;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                   // lane 0 holds the sum (a fixed tree: the same bits every run)
}

__global__ __launch_bounds__(IM_THREADS) void im_tile_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W,
                                                              int C, double* __restrict__ work) {
    __shared__ float s_x[IM_RH * IM_RW * IM_MAXC];              // pred, [row][column][channel] as in memory
    __shared__ float s_y[IM_RH * IM_RW * IM_MAXC];              // gt
    __shared__ double s_h[5][IM_RH][IM_TW];                     // horizontal 7-tap sums of x, y, xx, yy, xy for one channel
    __shared__ double s_red[IM_MAXC + 1][IM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ImTiles t = im_tiles(H, W);
    const int64_t p = blockIdx.x / t.per_frame;
    const int tile = (int)(blockIdx.x - p * t.per_frame);
    const int ty0 = (tile / t.ntx) * IM_TH, tx0 = (tile % t.ntx) * IM_TW;
    const int OH = H - IM_PAD, OW = W - IM_PAD;
    const int rows = min(IM_RH, H - ty0), cols = min(IM_RW, W - tx0);          // staged pixels that exist (>= 7 each)
    // the pixels whose squared error this workgroup adds: its IM_TH x IM_TW corner, up to the image edge for a last tile
    const int own_rows = ty0 + IM_TH >= OH ? rows : IM_TH, own_cols = tx0 + IM_TW >= OW ? cols : IM_TW;
    const int span = cols * C, row_ld = IM_RW * C;
    const int64_t frame = p * H * (int64_t)W * C;

    double sq = 0.0;
    for (int i = tid; i < IM_RH * row_ld; i += IM_THREADS) {
        const int r = i / row_ld, e = i - r * row_ld;
        float a = 0.f, b = 0.f;
        if (r < rows && e < span) {
            const int64_t g = frame + ((int64_t)(ty0 + r) * W + tx0) * C + e;
            a = pred[g];
            b = gt[g];
            if (r < own_rows && e < own_cols * C) {
                const float d = a - b;
                sq += (double)(d * d);                                         // (a - b) ** 2 in f32, summed in f64
            }
        }
        s_x[i] = a;
        s_y[i] = b;
    }
    sq = wave_sum(sq);
    if (lane == 0) s_red[C][wave] = sq;

    constexpr double C1 = 1e-4, C2 = 9e-4, NP = (double)(IM_WIN * IM_WIN), COV = NP / (NP - 1.0);
    for (int c = 0; c < C; ++c) {
        __syncthreads();                                                       // staging done / s_h of the last channel consumed
        for (int i = tid; i < IM_RH * IM_TW; i += IM_THREADS) {
            const int r = i / IM_TW, j = i - r * IM_TW;
            const float* px = s_x + r * row_ld + j * C + c;
            const float* py = s_y + r * row_ld + j * C + c;
            double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
            for (int k = 0; k < IM_WIN; ++k) {
                const double x = (double)px[k * C], y = (double)py[k * C];
                hx += x; hy += y; hxx += x * x; hyy += y * y; hxy += x * y;
            }
            s_h[0][r][j] = hx; s_h[1][r][j] = hy; s_h[2][r][j] = hxx; s_h[3][r][j] = hyy; s_h[4][r][j] = hxy;
        }
        __syncthreads();
        double acc = 0.0;
        for (int i = tid; i < IM_TH * IM_TW; i += IM_THREADS) {
            const int r = i / IM_TW, j = i - r * IM_TW;
            double m[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < IM_WIN; ++k) v += s_h[q][r + k][j];
                m[q] = v / NP;
            }
            const double ux = m[0], uy = m[1];
            const double vx = COV * (m[2] - ux * ux), vy = COV * (m[3] - uy * uy), vxy = COV * (m[4] - ux * uy);
            const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
            const double S = (A1 * A2) / (B1 * B2);
            acc += (ty0 + r < OH && tx0 + j < OW) ? S : 0.0;                   // windows that leave the image count nowhere
        }
        acc = wave_sum(acc);
        if (lane == 0) s_red[c][wave] = acc;
    }
    __syncthreads();
    if (tid <= C) {
        double v = s_red[tid][0];
#pragma unroll
        for (int w = 1; w < IM_WAVES; ++w) v += s_red[tid][w];
        work[(p * (C + 1) + tid) * t.per_frame + tile] = v;
    }
}

// One workgroup per frame.  The partials come through LDS in chunks (coalesced loads by the whole workgroup); thread q (q <= C)
// owns quantity q and adds its partials one by one in index order.
__global__ __launch_bounds__(IM_THREADS) void im_finish_kernel(const double* __restrict__ work, int H, int W, int C,
                                                                double* __restrict__ ssim, double* __restrict__ ssim_ch,
                                                                double* __restrict__ mse_out, double* __restrict__ psnr) {
    __shared__ double s_part[IM_MAXC + 1][IM_CHUNK + 1];        // (+1: the five rows start on different banks)
    __shared__ double s_tot[IM_MAXC + 1];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x, n = im_tiles(H, W).per_frame;
    const double* src = work + p * (C + 1) * n;
    double v = 0.0;
    for (int64_t base = 0; base < n; base += IM_CHUNK) {
        const int m = (int)(n - base < IM_CHUNK ? n - base : IM_CHUNK);
        __syncthreads();
        for (int q = 0; q <= C; ++q)
            for (int i = tid; i < m; i += IM_THREADS) s_part[q][i] = src[q * n + base + i];
        __syncthreads();
        if (tid <= C) {
#pragma unroll 8
            for (int i = 0; i < m; ++i) v += s_part[tid][i];
        }
    }
    if (tid <= C) s_tot[tid] = v;
    __syncthreads();
    if (tid == 0) {
        const double windows = (double)(H - IM_PAD) * (double)(W - IM_PAD);
        double s = 0.0;
        for (int c = 0; c < C; ++c) {
            const double sc = s_tot[c] / windows;
            if (ssim_ch) ssim_ch[p * C + c] = sc;
            s += sc;
        }
        ssim[p] = s / (double)C;
        const double mse = s_tot[C] / ((double)H * (double)W * (double)C);
        mse_out[p] = mse;
        psnr[p] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(1.0 / mse);
    }
}

// 0 when the sizes are supported (with the number of workgroups of the tile pass), else the reason
const char* im_sizes(int P, int H, int W, int C, int64_t* blocks) {
    if (P < 0) return "P < 0";
    if (H < IM_WIN || W < IM_WIN) return "H and W must be at least the 7-pixel window";
    if (H > IM_MAX_DIM || W > IM_MAX_DIM) return "H or W above 32768";
    if (C < 1 || C > IM_MAXC) return "C must lie in 1..4";
    const int64_t b = (int64_t)P * im_tiles(H, W).per_frame;
    if (b > 0x7fffffffll) return "more than 2^31 - 1 tiles";
    *blocks = b;
    return nullptr;
}

}  // namespace

extern "C" int64_t dmnerf_img_metrics_work_bytes(int P, int H, int W, int C) {
    int64_t blocks = 0;
    if (im_sizes(P, H, W, C, &blocks)) return -1;
    return blocks * (C + 1) * (int64_t)sizeof(double);
}

extern "C" int dmnerf_img_metrics(const float* d_pred, const float* d_gt, int P, int H, int W, int C, void* d_work, int64_t work_bytes,
                                  double* d_ssim, double* d_ssim_ch, double* d_mse, double* d_psnr, void* stream) {
    int64_t blocks = 0;
    if (const char* why = im_sizes(P, H, W, C, &blocks))
        return dmn_fail(DMNERF_E_ARG, "img_metrics: bad P=%d H=%d W=%d C=%d (%s)", P, H, W, C, why);
    if (P == 0) return DMNERF_OK;
    if (!d_pred || !d_gt || !d_work || !d_ssim || !d_mse || !d_psnr) return dmn_fail(DMNERF_E_ARG, "img_metrics: null pointer");
    const int64_t need = blocks * (C + 1) * (int64_t)sizeof(double);
    if (work_bytes < need)
        return dmn_fail(DMNERF_E_ARG, "img_metrics: work buffer too small (%lld < %lld bytes)", (long long)work_bytes, (long long)need);
    hipLaunchKernelGGL(im_tile_kernel, dim3((unsigned)blocks), dim3(IM_THREADS), 0, (hipStream_t)stream, d_pred, d_gt, H, W, C,
                       (double*)d_work);
    if (int rc = dmn_check_launch("img_metrics: tiles")) return rc;
    hipLaunchKernelGGL(im_finish_kernel, dim3((unsigned)P), dim3(IM_THREADS), 0, (hipStream_t)stream, (const double*)d_work, H, W, C,
                       d_ssim, d_ssim_ch, d_mse, d_psnr);
    return dmn_check_launch("img_metrics: finish");
}
