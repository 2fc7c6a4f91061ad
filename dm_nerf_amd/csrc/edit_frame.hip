// edit_frame.hip -- the two non-network stages around the manipulation render of an edited frame, for gfx950:
//   dmnerf_edit_rays      the target rays of T edited objects of a row band in ONE launch, written straight into [T, 2, n, 3]:
//                         a rigid object's rays are get_rays_k of its pose (the device function of raygen.h, shared with
//                         dmnerf_raygen: bit-identical rows), a deformed object's are the given pose's rays with the origin's x
//                         shifted by a per-image-row float64 offset (manipulator_demo, networks/manipulator.py:397-429);
//   dmnerf_edit_products  what the drivers write out per pixel (networks/manipulator.py:472-488): the 8-bit colour (to8b,
//                         evaluator.py:13), the argmax label over ALL object channels, its uint8 mask, its colour from a table.
// Both are bandwidth-trivial (a 640 x 480 frame at C = 95: 121 MB read, 6 MB written); what matters is that the strided rows of
// the packed band are read coalesced and that every lane has work at C = 8 as at C = 95.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "raygen.h"

namespace {

constexpr int WAVE = 64;
constexpr int BLOCK = 256;

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

struct EditRaysArgs {
    RaygenCam cam[DMNERF_EDIT_MAX_OBJECTS];
    int kind[DMNERF_EDIT_MAX_OBJECTS];     // 0 rigid, 1 deform
    int H, W, row0;
    int64_t n;                             // rays of the band
    const double* off;                     // [T, H]
    float* rays;                           // [T, 2, n, 3]
};

// grid.y = object (uniform per workgroup: the camera is read from the kernel arguments with scalar loads)
__global__ void edit_rays_kernel(const EditRaysArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n) return;
    const int t = blockIdx.y;
    const int col = (int)(idx % a.W);
    const int row = a.row0 + (int)(idx / a.W);            // the ABSOLUTE image row: bands of any world size agree
    float o[3], d[3];
    dmn_raygen_ray(a.cam[t], col, row, o, d);
    if (a.kind[t] == 1)                                   // f32 column + f64 tensor: summed in f64, rounded once on assignment (:428)
        o[0] = (float)((double)o[0] + a.off[(int64_t)t * a.H + row]);
    float* po = a.rays + ((int64_t)t * 2 * a.n + idx) * 3;
    float* pd = po + a.n * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        po[r] = o[r];
        pd[r] = d[r];
    }
}

// One pixel per group of G lanes (G = 4 .. 64, a power of two >= min(C, 64)): the lanes of a group read consecutive channels of
// the pixel's row -- consecutive addresses -- and a wave covers 64 / G pixels.  The argmax is reduced over the group with the rule
// of label_conf_kernel (strict >, so the FIRST maximum wins): between two candidates of equal value the lower channel is kept.
__global__ void edit_products_kernel(const float* __restrict__ rgb, int64_t rgb_stride, const float* __restrict__ ins, int64_t ins_stride,
                                     int C, const uint8_t* __restrict__ lut, int64_t n, int G, uint8_t* __restrict__ rgb8,
                                     int64_t* __restrict__ label, uint8_t* __restrict__ mask, uint8_t* __restrict__ ins_img) {
    const int per_block = BLOCK / G;
    const int g = threadIdx.x / G, l = threadIdx.x % G;
    const int64_t p = (int64_t)blockIdx.x * per_block + g;
    const bool live = p < n;                               // (no early return: every lane of the wave takes part in the shuffles)
    if (live && rgb8 && l < 3) {
        const float x = rgb[p * rgb_stride + l];
        const float c = fminf(fmaxf(x, 0.f), 1.f);
        rgb8[p * 3 + l] = (uint8_t)(int)(255.f * c);       // f32 product, truncated
    }
    if (!ins) return;                                      // (uniform)
    float bv = -INFINITY;
    int best = 0x7fffffff;
    if (live) {
        const float* x = ins + p * ins_stride;
        for (int c = l; c < C; c += G) {
            const float v = x[c];
            if (best == 0x7fffffff || v > bv) { bv = v; best = c; }
        }
    }
    for (int m = G >> 1; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(bv, m, WAVE);
        const int ob = __shfl_xor(best, m, WAVE);
        if (ob != 0x7fffffff && (best == 0x7fffffff || ov > bv || (ov == bv && ob < best))) { bv = ov; best = ob; }
    }
    if (!live) return;
    if (l == 0) {
        if (label) label[p] = best;
        if (mask) mask[p] = (uint8_t)best;
    }
    if (ins_img && lut && l < 3) ins_img[p * 3 + l] = lut[best * 3 + l];
}

}  // namespace

extern "C" int dmnerf_edit_rays(int H, int W, const float* h_intr, const float* h_poses, const int* h_kind, int T,
                                const double* d_off, int row0, int nrows, float* d_rays, void* stream) {
    if (H < 1 || W < 1 || row0 < 0 || nrows < 0 || row0 + nrows > H)
        return dmn_fail(DMNERF_E_ARG, "edit_rays: rows [%d,%d) outside image %dx%d", row0, row0 + nrows, H, W);
    if (T < 1 || T > DMNERF_EDIT_MAX_OBJECTS) return dmn_fail(DMNERF_E_ARG, "edit_rays: T=%d outside 1..%d", T, DMNERF_EDIT_MAX_OBJECTS);
    if (!h_intr || !h_poses || !h_kind) return dmn_fail(DMNERF_E_ARG, "edit_rays: null pointer");
    bool deform = false;
    for (int t = 0; t < T; ++t) {
        if (h_kind[t] != 0 && h_kind[t] != 1) return dmn_fail(DMNERF_E_ARG, "edit_rays: kind[%d]=%d (0 rigid, 1 deform)", t, h_kind[t]);
        deform = deform || h_kind[t] == 1;
    }
    if (nrows == 0) return DMNERF_OK;
    if (!d_rays || (deform && !d_off)) return dmn_fail(DMNERF_E_ARG, "edit_rays: null pointer");
    EditRaysArgs a;
    for (int t = 0; t < DMNERF_EDIT_MAX_OBJECTS; ++t) {
        a.cam[t] = dmn_raygen_cam(h_intr, h_poses + 12 * (t < T ? t : 0));
        a.kind[t] = t < T ? h_kind[t] : 0;
    }
    a.H = H; a.W = W; a.row0 = row0; a.n = (int64_t)nrows * W; a.off = d_off; a.rays = d_rays;
    hipLaunchKernelGGL(edit_rays_kernel, dim3(blocks_for(a.n, BLOCK), T), dim3(BLOCK), 0, (hipStream_t)stream, a);
    return dmn_check_launch("edit_rays");
}

extern "C" int dmnerf_edit_products(const float* d_rgb, int64_t rgb_stride, const float* d_ins, int64_t ins_stride, int C,
                                    const uint8_t* d_lut, int64_t n, uint8_t* d_rgb8, int64_t* d_label, uint8_t* d_mask,
                                    uint8_t* d_ins_img, void* stream) {
    if (n < 0 || rgb_stride < 3) return dmn_fail(DMNERF_E_ARG, "edit_products: bad n=%lld rgb_stride=%lld", (long long)n, (long long)rgb_stride);
    if (d_ins && (C < 1 || C > DMNERF_EDIT_MAX_CHANNELS || ins_stride < C))
        return dmn_fail(DMNERF_E_ARG, "edit_products: bad C=%d (1..%d) ins_stride=%lld", C, DMNERF_EDIT_MAX_CHANNELS, (long long)ins_stride);
    if (n > 0 && !d_rgb) return dmn_fail(DMNERF_E_ARG, "edit_products: null pointer");
    if (n == 0) return DMNERF_OK;
    int G = 4;
    if (d_ins)
        while (G < C && G < WAVE) G <<= 1;
    const int64_t blocks = (n + BLOCK / G - 1) / (BLOCK / G);
    if (blocks > 0x7fffffffLL) return dmn_fail(DMNERF_E_ARG, "edit_products: n=%lld too large", (long long)n);
    hipLaunchKernelGGL(edit_products_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, d_rgb, rgb_stride, d_ins,
                       ins_stride, C, d_lut, n, G, d_rgb8, d_label, d_mask, d_ins_img);
    return dmn_check_launch("edit_products");
}
