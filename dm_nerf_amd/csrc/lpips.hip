// lpips.hip -- what LPIPS needs around its thirteen convolutions (conv3x3.hip): the perceptual score the reference reports next to
// PSNR and SSIM, lpips.LPIPS(net="vgg")(rgb, gt) (networks/tester.py:43,91, networks/manipulator.py:216,280).
//
// The definition implemented here is that of lpips 0.1.4 for net='vgg', version='0.1', spatial=False, WRITTEN DOWN WITHOUT THE
// LIBRARY AT HAND (it is not installed where this was developed, and its constructor fetches weights; tests/_lpips_restate.py is the
// same definition in plain torch, the referee of the tests):
//     x        = (in - shift) / scale per RGB channel, shift (-.030, -.088, -.188), scale (.458, .448, .450); `in` as given
//                (normalize: 2 in - 1 first)
//     features = VGG16 `features`: 3x3 convolutions of widths 64, 64 | 128, 128 | 256 x 3 | 512 x 3 | 512 x 3, ReLU after each, a
//                2x2 / stride 2 max-pool (floor) before each group but the first; tapped after the last ReLU of each group
//     score    = sum over the five taps of  mean over the pixels of  sum_c w_c (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2,
//                n = sqrt(sum_c f_c^2), w = the tap's `lin` weights (no bias; dropout is the identity in eval)
//
//   lpips_prologue_kernel   scaling layer + the 27 taps (3 x 3 x RGB, zero padding of the SCALED image) of every pixel of both frames
//                           into rows of 32 floats (columns 27 .. 31 and the border rows zero): the first convolution's K range, so
//                           that it is a case of conv3x3 with one run (taps = 1).  The frames of a batch: pred 0 .. P-1, gt P .. 2P-1.
//   maxpool2_kernel         padded-flat -> padded-flat, borders and guard rows written zero; a NaN wins the maximum, as in torch
//   lpips_tail_kernel       a wave per pixel: channel sums by a fixed butterfly in f32, the pixel's value added in f64 to the wave's
//                           running sum in pixel order; the four waves of a workgroup are added in index order: one f64 partial per
//                           workgroup.  The workgroups of a frame are the same whatever the batch.
//   lpips_reduce_kernel     per frame: the partials in index order, / pixels, set (first tap) or added to (later taps) the score
// No floating-point atomics: bit-identical from run to run and independent of P.  No allocation, no synchronisation: capturable.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int LP_MIN_DIM = 16, LP_MAX_DIM = 4096;
constexpr int LP_TAIL_PIX = 256;                // pixels per workgroup of the tail: 64 per wave

__global__ __launch_bounds__(256) void lpips_prologue_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int P, int H, int W,
                                                             int normalize, float* __restrict__ out, int64_t M) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * 32) return;
    const int64_t m = e >> 5;
    const int k = (int)(e & 31);
    const int Wp = W + 2;
    const int64_t per = (int64_t)(H + 2) * Wp;
    const int n = (int)(m / per);
    const int p = (int)(m - n * per);
    const int y = p / Wp, x = p - y * Wp;
    float v = 0.f;
    if (k < 27 && y >= 1 && y <= H && x >= 1 && x <= W) {
        const int tap = k / 3, c = k - 3 * tap;
        const int yy = y - 2 + tap / 3, xx = x - 2 + tap % 3;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const float* src = n < P ? pred + (int64_t)n * H * W * 3 : gt + (int64_t)(n - P) * H * W * 3;
            float t = src[((int64_t)yy * W + xx) * 3 + c];
            if (normalize) t = 2.f * t - 1.f;
            const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
            const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
            v = (t - shift) / scale;
        }
    }
    out[e] = v;
}

__device__ __forceinline__ float nanmax(float a, float b) { return (b > a || b != b) ? b : a; }

// one thread per (output row, guards included; 4 channels)
__global__ __launch_bounds__(256) void maxpool2_kernel(const float* __restrict__ in, float* __restrict__ out, int N, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2;
    const int c4 = C >> 2;
    const int64_t Go = Wo + 3, per_o = (int64_t)(Ho + 2) * (Wo + 2);
    const int64_t rows = N * per_o + 2 * Go;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * c4) return;
    const int64_t r = e / c4;
    const int q = (int)(e - r * c4);
    f4 v = (f4)(0.f);
    const int64_t m = r - Go;
    if (m >= 0 && m < N * per_o) {
        const int n = (int)(m / per_o);
        const int p = (int)(m - n * per_o);
        const int y = p / (Wo + 2), x = p - y * (Wo + 2);
        if (y >= 1 && y <= Ho && x >= 1 && x <= Wo) {
            const int64_t Wp = W + 2;
            const int64_t r00 = (W + 3) + (int64_t)n * (H + 2) * Wp + (int64_t)(2 * y - 1) * Wp + (2 * x - 1);
            const f4* s = reinterpret_cast<const f4*>(in) + q;
            const f4 a = s[r00 * c4], b = s[(r00 + 1) * c4], c = s[(r00 + Wp) * c4], d = s[(r00 + Wp + 1) * c4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = nanmax(nanmax(a[i], b[i]), nanmax(c[i], d[i]));
        }
    }
    reinterpret_cast<f4*>(out)[e] = v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid (workgroups of a frame, P); feat: padded-flat [2P images], frame p = images p and P + p
__global__ __launch_bounds__(256) void lpips_tail_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int P, int H, int W, int C,
                                                         double* __restrict__ partials) {
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int frame = blockIdx.y;
    const int Wp = W + 2;
    const int64_t per = (int64_t)(H + 2) * Wp;
    const float* f0 = feat + ((W + 3) + (int64_t)frame * per) * C;
    const float* f1 = feat + ((W + 3) + (int64_t)(P + frame) * per) * C;
    const int npix = H * W;
    const int first = blockIdx.x * LP_TAIL_PIX + wv * 64;
    double acc = 0.0;
    for (int i = 0; i < 64; ++i) {
        const int px = first + i;
        if (px >= npix) break;                                       // (uniform per wave)
        const int y = px / W, x = px - y * W;
        const int64_t row = (int64_t)(y + 1) * Wp + (x + 1);
        const float* a = f0 + row * C;
        const float* b = f1 + row * C;
        float s0 = 0.f, s1 = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float u = a[c], v = b[c];
            s0 += u * u;
            s1 += v * v;
        }
        const float n0 = sqrtf(wave_sum(s0)) + 1e-10f, n1 = sqrtf(wave_sum(s1)) + 1e-10f;
        float d = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float t = a[c] / n0 - b[c] / n1;
            d += lin[c] * (t * t);
        }
        acc += (double)wave_sum(d);
    }
    if (lane == 0) wsum[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(int64_t)frame * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ void lpips_reduce_kernel(const double* __restrict__ partials, int P, int nwg, double npix, int first, double* __restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    for (int g = 0; g < nwg; ++g) s += partials[(int64_t)p * nwg + g];
    const double v = s / npix;
    out[p] = first ? v : out[p] + v;
}

int64_t lp_align(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" int64_t dmnerf_lpips_work_bytes(int P, int H, int W) {
    if (P < 0 || H < LP_MIN_DIM || W < LP_MIN_DIM || H > LP_MAX_DIM || W > LP_MAX_DIM) return -1;
    if (P == 0) return 0;
    const int64_t N = 2 * (int64_t)P;
    const int64_t M = N * (H + 2) * (W + 2);
    if (M > 0x7fffff00LL) return -1;
    const int64_t act = lp_align((M + 2 * (W + 3)) * 64 * 4);       // the widest activation: the first group's (64 channels at full size)
    const int64_t taps = lp_align(M * 32 * 4);
    const int64_t part = lp_align((int64_t)P * (((int64_t)H * W + LP_TAIL_PIX - 1) / LP_TAIL_PIX) * 8);
    return taps + 2 * act + part;
}

extern "C" int dmnerf_lpips_prologue(const float* d_pred, const float* d_gt, int P, int H, int W, int normalize, float* d_taps, int64_t taps_floats,
                                     void* stream) {
    if (P < 0 || H < 1 || W < 1 || H > 32768 || W > 32768) return dmn_fail(DMNERF_E_ARG, "lpips_prologue: bad sizes P=%d H=%d W=%d", P, H, W);
    const int64_t M = 2 * (int64_t)P * (H + 2) * (W + 2);
    if (M > 0x7fffff00LL) return dmn_fail(DMNERF_E_ARG, "lpips_prologue: too many pixels (P=%d H=%d W=%d)", P, H, W);
    if (P == 0) return DMNERF_OK;
    if (!d_pred || !d_gt || !d_taps) return dmn_fail(DMNERF_E_ARG, "lpips_prologue: null pointer");
    if (taps_floats < M * 32) return dmn_fail(DMNERF_E_ARG, "lpips_prologue: d_taps holds %lld floats, %lld needed", (long long)taps_floats, (long long)(M * 32));
    const int64_t blocks = (M * 32 + 255) / 256;
    hipLaunchKernelGGL(lpips_prologue_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_pred, d_gt, P, H, W, normalize, d_taps, M);
    return dmn_check_launch("lpips_prologue");
}

extern "C" int dmnerf_maxpool2(const float* d_in, int64_t in_floats, float* d_out, int64_t out_floats, int N, int H, int W, int C, void* stream) {
    if (N < 0 || H < 2 || W < 2 || H > 32768 || W > 32768 || C < 4 || C % 4 || C > 4096)
        return dmn_fail(DMNERF_E_ARG, "maxpool2: bad sizes N=%d H=%d W=%d C=%d", N, H, W, C);
    const int64_t rows_in = (int64_t)N * (H + 2) * (W + 2) + 2 * (W + 3);
    const int64_t rows_out = (int64_t)N * (H / 2 + 2) * (W / 2 + 2) + 2 * (W / 2 + 3);
    if (rows_in > 0x7fffff00LL) return dmn_fail(DMNERF_E_ARG, "maxpool2: too many rows (N=%d H=%d W=%d)", N, H, W);
    if (N == 0) return DMNERF_OK;
    if (!d_in || !d_out) return dmn_fail(DMNERF_E_ARG, "maxpool2: null pointer");
    if (((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15)) return dmn_fail(DMNERF_E_ARG, "maxpool2: pointers must be 16-byte aligned");
    if (in_floats < rows_in * C || out_floats < rows_out * C)
        return dmn_fail(DMNERF_E_ARG, "maxpool2: buffers hold %lld / %lld floats, %lld / %lld needed", (long long)in_floats, (long long)out_floats,
                        (long long)(rows_in * C), (long long)(rows_out * C));
    const int64_t blocks = (rows_out * (C / 4) + 255) / 256;
    if (blocks > 0x7fffffffLL) return dmn_fail(DMNERF_E_ARG, "maxpool2: too many elements");
    hipLaunchKernelGGL(maxpool2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_in, d_out, N, H, W, C);
    return dmn_check_launch("maxpool2");
}

extern "C" int dmnerf_lpips_tail(const float* d_feat, int64_t feat_floats, const float* d_lin, int P, int H, int W, int C, int first, double* d_partials,
                                 int64_t partials_count, double* d_out, void* stream) {
    if (P < 0 || P > 65535 || H < 1 || W < 1 || H > 32768 || W > 32768 || C < 32 || C % 32 || C > 4096)
        return dmn_fail(DMNERF_E_ARG, "lpips_tail: bad sizes P=%d H=%d W=%d C=%d", P, H, W, C);
    const int64_t rows = 2 * (int64_t)P * (H + 2) * (W + 2) + 2 * (W + 3);
    if (rows > 0x7fffff00LL) return dmn_fail(DMNERF_E_ARG, "lpips_tail: too many rows (P=%d H=%d W=%d)", P, H, W);
    if (P == 0) return DMNERF_OK;
    if (!d_feat || !d_lin || !d_partials || !d_out) return dmn_fail(DMNERF_E_ARG, "lpips_tail: null pointer");
    const int64_t nwg = ((int64_t)H * W + LP_TAIL_PIX - 1) / LP_TAIL_PIX;
    if (feat_floats < rows * C || partials_count < nwg * P)
        return dmn_fail(DMNERF_E_ARG, "lpips_tail: buffers hold %lld floats / %lld partials, %lld / %lld needed", (long long)feat_floats,
                        (long long)partials_count, (long long)(rows * C), (long long)(nwg * P));
    hipLaunchKernelGGL(lpips_tail_kernel, dim3((unsigned)nwg, (unsigned)P), dim3(256), 0, (hipStream_t)stream, d_feat, d_lin, P, H, W, C, d_partials);
    if (int rc = dmn_check_launch("lpips_tail"); rc != DMNERF_OK) return rc;
    hipLaunchKernelGGL(lpips_reduce_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, (hipStream_t)stream, d_partials, P, (int)nwg, (double)H * (double)W,
                       first, d_out);
    return dmn_check_launch("lpips_reduce");
}
