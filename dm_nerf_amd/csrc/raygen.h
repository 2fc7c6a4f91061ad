// raygen.h -- one camera ray of get_rays_k (networks/helpers.py:50-61), shared by the ray generators of render_kernels.hip and
// the edited-frame target rays of edit_frame.hip: every caller gets the same float32 operations in the same order
// (-ffp-contract=off: each a*b+c is two roundings, like ATen's eager ops), so their rays are bit-identical.
#pragma once
#include <hip/hip_runtime.h>

struct RaygenCam {
    float fx, fy, cx, cy, k22;
    float r[9];      // c2w[:3,:3] row-major
    float t[3];      // c2w[:3,3]
};

// h_intr = {K00, K11, K02, K12, K22}; h_c2w = first 3 rows of c2w, row-major [3][4]
inline RaygenCam dmn_raygen_cam(const float* h_intr, const float* h_c2w) {
    RaygenCam c;
    c.fx = h_intr[0]; c.fy = h_intr[1]; c.cx = h_intr[2]; c.cy = h_intr[3]; c.k22 = h_intr[4];
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) c.r[3 * r + k] = h_c2w[4 * r + k];
        c.t[r] = h_c2w[4 * r + 3];
    }
    return c;
}

// origin and direction of pixel (row, col) -> o[0..2], d[0..2]
__device__ __forceinline__ void dmn_raygen_ray(const RaygenCam& c, int col, int row, float* __restrict__ o, float* __restrict__ d) {
    const float i = (float)col, j = (float)row;          // linspace(0, W-1, W) is exactly 0,1,2,...
    const float d0 = (i - c.cx) / c.fx;
    const float d1 = (j - c.cy) / c.fy;
    const float d2 = c.k22 * 1.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        // torch.sum(dirs[..., None, :] * c2w[:3,:3], -1): sequential over the 3 products
        d[r] = (d0 * c.r[3 * r + 0] + d1 * c.r[3 * r + 1]) + d2 * c.r[3 * r + 2];
        o[r] = c.t[r];
    }
}
