// baked.hip -- the baked field volume seen along rays: colour and transmittance for edit previews, without the networks.
//
//   dmnerf_baked_render   R <= 4 ray sets rays [R, 2, N, 3] against labels [dx, dy, dz] (uint8) and cells [dx, dy, dz, 4] (f32: three
//                         colour logits and sigma per cell, what dmnerf_bake_cells kept of the fine network's row) over the box of a
//                         LabelGrid; set r counts the cells whose label is < C and in its own 128-bit mask.  Per pixel n the counted
//                         cells of all sets are volume-rendered front to back: rgb, depth, acc, the label and set of the heaviest
//                         segment, and the number of segments.
//
// One lane per pixel.  Every set walks the volume exactly as label_trace_kernel does (the same clip, start cell, cell sequence and t
// values: the walk of grid_volume.h, f32 operations rounded one by one), but does not stop at its first counted cell:
//
//   segment    a counted cell of set r gives t_in = the walk's current t, t_out = the next plane crossing tmax_a if tmax_a < t_exit,
//              else t_exit, and len = (t_out - t_in) * |d_r| with |d| = sqrtf(d0 d0 + d1 d1 + d2 d2), summed in that order.  The
//              16-byte cells entry is read for a counted cell only.
//   merge      a pixel's rays share the ray parameter (a target ray is the original one under an affine map), so the pending
//              segments of the R sets are composited in ascending t_in, the lowest set first on equal t_in; a set without a further
//              counted cell drops out.  Within a set the walk's order stands.
//   composite  alpha = 1 - expf(-max(sigma, 0) * len), w = T * alpha, T <- T * (1 - alpha) from T = 1; rgb += w / (1 + expf(-logit)),
//              depth += w * t_in, acc += w; label / source are those of the segment with the largest w so far (a strict > from
//              best_w = 0: the first wins ties, a pixel without positive weight keeps 255 / 255).  max(sigma, 0) is
//              sigma > 0 ? sigma : 0, so a NaN sigma contributes nothing.  After a segment the pixel stops if T < stop.
//
// The walk state of every set lives in registers: the kernel is a template on R, every loop over the sets is unrolled and a set is
// only ever named by a compile-time index (the set whose segment was taken advances under `if (taken == r)`), so there is no
// dynamically indexed per-lane array and no scratch.  The loops are counted: a set visits at most dx + dy + dz + 1 cells, a pixel
// composites at most R times as many segments; no input can make a lane spin.  The cell index is in range before every load.  No
// allocation, no synchronisation, no atomics, no reductions across lanes.  Workgroups are single waves, as in label_trace.hip and for
// its reason: nothing is shared between waves, and a wave lasts as long as its longest lane.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "grid_volume.h"

namespace {

constexpr int BLOCK = 64;
constexpr int MAX_SETS = 4;
constexpr int UNLABELLED = 255;

struct BakedMasks {
    uint32_t w[MAX_SETS * 4];
};

// One set's walk: the ray, where it is, and the counted cell it has found but the pixel has not composited yet.  `it` counts the
// cells visited and is set to the bound when the walk ends; `label` is UNLABELLED while nothing is pending.  (Integers in vector
// registers, not flags: a flag per set and lane is a pair of scalar registers, and four sets of them do not fit.)
struct Walk {
    WalkRay ray;
    float t_exit, t, norm;
    int c0, c1, c2, it;
    float t_in, t_out;
    int g, label;
};

// the trace's clip and start cell (grid_volume.h)
__device__ __forceinline__ void walk_init(Walk& S, const GridBox& G, const float* __restrict__ o, const float* __restrict__ d,
                                          float t_near, float t_far, int max_cells) {
    const float inf = __builtin_huge_valf();
    WalkRay& r = S.ray;
    r.o0 = o[0]; r.o1 = o[1]; r.o2 = o[2];
    r.d0 = d[0]; r.d1 = d[1]; r.d2 = d[2];
    S.norm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(r.d0, r.d0), __fmul_rn(r.d1, r.d1)), __fmul_rn(r.d2, r.d2)));
    const float hi0 = plane_of(G.lo[0], G.cell[0], G.dims[0]), hi1 = plane_of(G.lo[1], G.cell[1], G.dims[1]),
                hi2 = plane_of(G.lo[2], G.cell[2], G.dims[2]);
    float t_enter = t_near;
    bool miss = false;
    S.t_exit = t_far;
    r.inv0 = inf; r.inv1 = inf; r.inv2 = inf;
    walk_clip_axis(G.lo[0], hi0, r.o0, r.d0, r.inv0, t_enter, S.t_exit, miss);
    walk_clip_axis(G.lo[1], hi1, r.o1, r.d1, r.inv1, t_enter, S.t_exit, miss);
    walk_clip_axis(G.lo[2], hi2, r.o2, r.d2, r.inv2, t_enter, S.t_exit, miss);
    S.c0 = walk_start_cell(r.o0, r.d0, t_enter, G.lo[0], G.inv_cell[0], G.dims[0]);
    S.c1 = walk_start_cell(r.o1, r.d1, t_enter, G.lo[1], G.inv_cell[1], G.dims[1]);
    S.c2 = walk_start_cell(r.o2, r.d2, t_enter, G.lo[2], G.inv_cell[2], G.dims[2]);
    S.t = t_enter;
    S.it = (miss || !(t_enter < S.t_exit)) ? max_cells : 0;
    S.t_in = 0.f; S.t_out = 0.f;
    S.g = 0; S.label = UNLABELLED;
}

// The trace's walk from where the set stands to its next counted cell, which becomes the pending segment; the set is then already
// one step further.  Without a further counted cell the set ends with nothing pending.
__device__ __forceinline__ void walk_advance(Walk& S, const GridBox& G, const uint8_t* __restrict__ labels, int C, uint32_t m0, uint32_t m1,
                                             uint32_t m2, uint32_t m3, int max_cells) {
    S.label = UNLABELLED;
    while (S.it < max_cells) {
        ++S.it;
        const int g = (S.c0 * G.dims[1] + S.c1) * G.dims[2] + S.c2;             // 0 <= c_a < dims_a: always inside the volume
        const uint32_t l = labels[g];
        const bool in_set = mask_bit(m0, m1, m2, m3, l);
        const bool counted = l < (uint32_t)C && in_set;
        int axis;
        float tm;
        const bool on = walk_step(G, S.ray, S.c0, S.c1, S.c2, S.t_exit, &axis, &tm);
        if (counted) {
            S.t_in = S.t;
            S.t_out = on ? tm : S.t_exit;
            S.g = g;
            S.label = (int)l;
        }
        if (!on || walk_apply(G, S.ray, axis, tm, S.c0, S.c1, S.c2, S.t)) S.it = max_cells;
        if (counted) break;
    }
}

__device__ __forceinline__ float sigmoid_of(float x) { return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-x))); }

template <int R>
__global__ __launch_bounds__(BLOCK) void baked_render_kernel(const uint8_t* __restrict__ labels, const float4* __restrict__ cells, GridBox G,
                                                             int C, const float* __restrict__ rays, int64_t N, BakedMasks M, float t_near,
                                                             float t_far, float stop, float* __restrict__ out_rgb,
                                                             float* __restrict__ out_depth, float* __restrict__ out_acc,
                                                             uint8_t* __restrict__ out_label, uint8_t* __restrict__ out_source,
                                                             int32_t* __restrict__ out_nseg) {
    const int64_t n = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    const int max_cells = G.dims[0] + G.dims[1] + G.dims[2] + 1;
    Walk S[R];
#pragma unroll
    for (int r = 0; r < R; ++r) walk_init(S[r], G, rays + ((int64_t)(2 * r) * N + n) * 3, rays + ((int64_t)(2 * r + 1) * N + n) * 3, t_near, t_far, max_cells);
    float T = 1.f, rgb0 = 0.f, rgb1 = 0.f, rgb2 = 0.f, depth = 0.f, acc = 0.f, best_w = 0.f;
    int best_label = UNLABELLED, best_source = UNLABELLED, nseg = 0;
    int taken = -1;                                                               // -1: every set looks for its first counted cell
    for (int seg = 0; seg < R * max_cells; ++seg) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            // (r is a constant after unrolling: the four words are scalar loads from the kernel's argument block)
            if (taken < 0 || taken == r) walk_advance(S[r], G, labels, C, M.w[r * 4 + 0], M.w[r * 4 + 1], M.w[r * 4 + 2], M.w[r * 4 + 3], max_cells);
        }
        taken = -1;
        float t_in = 0.f, t_out = 0.f, norm = 0.f;
        int g = 0, label = UNLABELLED;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (S[r].label != UNLABELLED && (taken < 0 || S[r].t_in < t_in)) {
                taken = r; t_in = S[r].t_in; t_out = S[r].t_out; norm = S[r].norm; g = S[r].g; label = S[r].label;
            }
        }
        if (taken < 0) break;
        const float4 c = cells[g];
        const float len = __fmul_rn(__fsub_rn(t_out, t_in), norm);
        const float sigma = c.w > 0.f ? c.w : 0.f;                                // (a NaN: 0)
        const float alpha = __fsub_rn(1.f, expf(-__fmul_rn(sigma, len)));
        const float w = __fmul_rn(T, alpha);
        T = __fmul_rn(T, __fsub_rn(1.f, alpha));
        rgb0 = __fadd_rn(rgb0, __fmul_rn(w, sigmoid_of(c.x)));
        rgb1 = __fadd_rn(rgb1, __fmul_rn(w, sigmoid_of(c.y)));
        rgb2 = __fadd_rn(rgb2, __fmul_rn(w, sigmoid_of(c.z)));
        depth = __fadd_rn(depth, __fmul_rn(w, t_in));
        acc = __fadd_rn(acc, w);
        ++nseg;
        if (w > best_w) { best_w = w; best_label = label; best_source = taken; }
        if (T < stop) break;
    }
    out_rgb[n * 3 + 0] = rgb0;
    out_rgb[n * 3 + 1] = rgb1;
    out_rgb[n * 3 + 2] = rgb2;
    out_depth[n] = depth;
    out_acc[n] = acc;
    out_label[n] = (uint8_t)best_label;
    out_source[n] = (uint8_t)best_source;
    out_nseg[n] = nseg;
}

}  // namespace

extern "C" int dmnerf_baked_render(const uint8_t* d_labels, const float* d_cells, const float lo[3], const float cell[3],
                                   const float inv_cell[3], const int dims[3], int C, const float* d_rays, int R, int64_t N,
                                   const uint32_t* masks, float t_near, float t_far, float stop, float* d_rgb, float* d_depth, float* d_acc,
                                   uint8_t* d_label, uint8_t* d_source, int32_t* d_nseg, void* stream) {
    if (!lo || !cell || !inv_cell || !dims || !masks) return dmn_fail(DMNERF_E_ARG, "baked_render: null pointer");     // (the host arrays: before N, as ever)
    if (N < 0) return dmn_fail(DMNERF_E_ARG, "baked_render: bad N=%lld", (long long)N);
    if (R < 1 || R > MAX_SETS) return dmn_fail(DMNERF_E_ARG, "baked_render: R=%d outside 1..%d", R, MAX_SETS);
    if (int rc = dmn_check_labels("baked_render", C)) return rc;
    if (!(stop >= 0.f)) return dmn_fail(DMNERF_E_ARG, "baked_render: stop %g must be >= 0", (double)stop);
    GridBox G;
    int64_t total;
    if (int rc = dmn_grid_given("baked_render", lo, cell, inv_cell, dims, &G, &total)) return rc;
    const int64_t nb = (N + BLOCK - 1) / BLOCK;
    if (nb > 0x7fffffffLL) return dmn_fail(DMNERF_E_ARG, "baked_render: %lld rays is too many for one launch", (long long)N);
    if (N == 0) return DMNERF_OK;
    if (!d_labels || !d_cells || !d_rays || !d_rgb || !d_depth || !d_acc || !d_label || !d_source || !d_nseg)
        return dmn_fail(DMNERF_E_ARG, "baked_render: null pointer");
    if ((uintptr_t)d_cells & 15) return dmn_fail(DMNERF_E_ARG, "baked_render: d_cells must be 16-byte aligned");
    BakedMasks M;
    for (int q = 0; q < MAX_SETS * 4; ++q) M.w[q] = q < R * 4 ? masks[q] : 0u;
    const float4* cells4 = reinterpret_cast<const float4*>(d_cells);
    const dim3 grid((unsigned)nb), block(BLOCK);
    hipStream_t s = (hipStream_t)stream;
#define DMN_BAKED_LAUNCH(RR)                                                                                                           \
    hipLaunchKernelGGL(baked_render_kernel<RR>, grid, block, 0, s, d_labels, cells4, G, C, d_rays, N, M, t_near, t_far, stop, d_rgb,   \
                       d_depth, d_acc, d_label, d_source, d_nseg)
    switch (R) {
        case 1: DMN_BAKED_LAUNCH(1); break;
        case 2: DMN_BAKED_LAUNCH(2); break;
        case 3: DMN_BAKED_LAUNCH(3); break;
        default: DMN_BAKED_LAUNCH(4); break;
    }
#undef DMN_BAKED_LAUNCH
    return dmn_check_launch("baked_render");
}
