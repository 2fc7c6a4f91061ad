// label_trace.hip -- rays through the label volume: the first cell along a ray whose label belongs to a set (picking an object from a
// pixel, previewing an edit without the networks).
//
//   dmnerf_label_trace   R ray sets rays [R, 2, N, 3] against labels [dx, dy, dz] (uint8, cell (i, j, k) at (i * dy + j) * dz + k) over
//                        the box of a LabelGrid; set r accepts the labels of its own 128-bit mask.  Per pixel n the hit with the
//                        smallest t over the sets, the lowest set on equal t: label, t, cell index, set.
//
// One lane per pixel, exact cell-by-cell traversal (Amanatides-Woo).  Every f32 operation is rounded on its own, as in skip.hip, and
// minimum / maximum are written out as comparisons, so tests/_label_trace_restate.py states the kernel in numpy bit for bit:
//
//   planes   plane_a(b) = lo_a + float(b) * cell_a for b = 0 .. dims_a; the upper face of the box is plane_a(dims_a).
//   clip     per axis with d_a != 0: inv_d_a = 1 / d_a, t0 = (plane_a(0) - o_a) * inv_d_a, t1 = (plane_a(dims_a) - o_a) * inv_d_a;
//            t_enter = max(t_near, max_a min(t0, t1)), t_exit = min(t_far, min_a max(t0, t1)), with a minimum and a maximum that pass
//            a NaN operand on.  An axis with d_a == 0 bounds nothing if lo_a <= o_a < plane_a(dims_a) and makes the ray miss otherwise.
//            The ray misses unless t_enter < t_exit: written this way round a NaN anywhere (origin, direction, bounds) is a miss.
//   start    SkipGrid's cell arithmetic on p = o + d * t_enter, clamped per axis into [0, dims_a - 1] (a NaN goes to 0).
//   walk     at most dx + dy + dz + 1 cells, a counted loop: no input can make a lane spin.  A cell whose label is < C and in the
//            mask is the hit, at the current t.  Otherwise tmax_a = (plane_a(c_a + (d_a > 0)) - o_a) * inv_d_a (+inf where
//            d_a == 0) -- recomputed from the integer index in every cell, never accumulated, so the crossing of plane b is one
//            value however the ray got there -- the axis of the smallest tmax steps (the lowest axis on ties); the ray misses
//            unless tmax_a < t_exit, or where the step leaves the index range; t = max(t, tmax_a).
//
// Label 255 and every label >= C are never accepted, whatever the mask.  The cell index is range-checked before every load, so the
// volume is never read out of bounds.  No allocation, no synchronisation, no atomics, no float reductions.
//
// What the kernel is: latency- and divergence-bound.  A step is one dependent byte load and about thirty VALU operations; the lanes
// of a wave are 64 consecutive pixels, which walk nearly the same cells, and a 128^3 volume is 2 MB: it sits in L2.  The walk of a
// wave lasts as long as its longest lane.  Workgroups are single waves (64 lanes): nothing is shared between waves, so a finished
// wave frees its slot at once instead of waiting for the slowest of four.  Not MFMA work, no roofline claim.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "grid_volume.h"                      // GridBox, mask_bit, the walk

namespace {

constexpr int BLOCK = 64;
constexpr int MAX_SETS = 16;
constexpr int UNLABELLED = 255;

struct TraceMasks {
    uint32_t w[MAX_SETS * 4];
};

__global__ __launch_bounds__(BLOCK) void label_trace_kernel(const uint8_t* __restrict__ labels, GridBox G, int C,
                                                            const float* __restrict__ rays, int R, int64_t N, TraceMasks M,
                                                            float t_near, float t_far, uint8_t* __restrict__ out_label,
                                                            float* __restrict__ out_t, int32_t* __restrict__ out_cell,
                                                            uint8_t* __restrict__ out_source) {
    const int64_t n = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    const int dx = G.dims[0], dy = G.dims[1], dz = G.dims[2];
    const int max_cells = dx + dy + dz + 1;
    const float hi0 = plane_of(G.lo[0], G.cell[0], dx), hi1 = plane_of(G.lo[1], G.cell[1], dy), hi2 = plane_of(G.lo[2], G.cell[2], dz);
    const float inf = __builtin_huge_valf();
    int best_label = UNLABELLED, best_cell = -1, best_source = UNLABELLED;
    float best_t = inf;
    for (int r = 0; r < R; ++r) {
        // (r is the same in every lane: the four words are scalar loads from the kernel's argument block, no scratch)
        const uint32_t m0 = M.w[r * 4 + 0], m1 = M.w[r * 4 + 1], m2 = M.w[r * 4 + 2], m3 = M.w[r * 4 + 3];
        const float* o = rays + ((int64_t)(2 * r) * N + n) * 3;
        const float* d = rays + ((int64_t)(2 * r + 1) * N + n) * 3;
        WalkRay ray = {o[0], o[1], o[2], d[0], d[1], d[2], inf, inf, inf};
        // ---- clip
        float t_enter = t_near, t_exit = t_far;
        bool miss = false;
        walk_clip_axis(G.lo[0], hi0, ray.o0, ray.d0, ray.inv0, t_enter, t_exit, miss);
        walk_clip_axis(G.lo[1], hi1, ray.o1, ray.d1, ray.inv1, t_enter, t_exit, miss);
        walk_clip_axis(G.lo[2], hi2, ray.o2, ray.d2, ray.inv2, t_enter, t_exit, miss);
        if (miss || !(t_enter < t_exit)) continue;
        // ---- start cell
        int c0 = walk_start_cell(ray.o0, ray.d0, t_enter, G.lo[0], G.inv_cell[0], dx);
        int c1 = walk_start_cell(ray.o1, ray.d1, t_enter, G.lo[1], G.inv_cell[1], dy);
        int c2 = walk_start_cell(ray.o2, ray.d2, t_enter, G.lo[2], G.inv_cell[2], dz);
        // ---- walk
        float t = t_enter;
        for (int it = 0; it < max_cells; ++it) {
            const int g = (c0 * dy + c1) * dz + c2;                               // 0 <= c_a < dims_a: always inside the volume
            const uint32_t l = labels[g];
            const bool in_set = mask_bit(m0, m1, m2, m3, l);
            if (l < (uint32_t)C && in_set) {
                if (t < best_t) { best_t = t; best_label = (int)l; best_cell = g; best_source = r; }
                break;
            }
            int axis;
            float tm;
            if (!walk_step(G, ray, c0, c1, c2, t_exit, &axis, &tm)) break;
            if (walk_apply(G, ray, axis, tm, c0, c1, c2, t)) break;
        }
    }
    out_label[n] = (uint8_t)best_label;
    out_t[n] = best_t;
    out_cell[n] = best_cell;
    out_source[n] = (uint8_t)best_source;
}

}  // namespace

extern "C" int dmnerf_label_trace(const uint8_t* d_labels, const float lo[3], const float cell[3], const float inv_cell[3],
                                  const int dims[3], int C, const float* d_rays, int R, int64_t N, const uint32_t* masks, float t_near,
                                  float t_far, uint8_t* d_label, float* d_t, int32_t* d_cell, uint8_t* d_source, void* stream) {
    if (!lo || !cell || !inv_cell || !dims || !masks) return dmn_fail(DMNERF_E_ARG, "label_trace: null pointer");      // (the host arrays: before N, as ever)
    if (N < 0) return dmn_fail(DMNERF_E_ARG, "label_trace: bad N=%lld", (long long)N);
    if (R < 1 || R > MAX_SETS) return dmn_fail(DMNERF_E_ARG, "label_trace: R=%d outside 1..%d", R, MAX_SETS);
    if (int rc = dmn_check_labels("label_trace", C)) return rc;
    GridBox G;
    int64_t total;
    if (int rc = dmn_grid_given("label_trace", lo, cell, inv_cell, dims, &G, &total)) return rc;
    const int64_t nb = (N + BLOCK - 1) / BLOCK;
    if (nb > 0x7fffffffLL) return dmn_fail(DMNERF_E_ARG, "label_trace: %lld rays is too many for one launch", (long long)N);
    if (N == 0) return DMNERF_OK;
    if (!d_labels || !d_rays || !d_label || !d_t || !d_cell || !d_source) return dmn_fail(DMNERF_E_ARG, "label_trace: null pointer");
    TraceMasks M;
    for (int q = 0; q < MAX_SETS * 4; ++q) M.w[q] = q < R * 4 ? masks[q] : 0u;
    hipLaunchKernelGGL(label_trace_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, d_labels, G, C, d_rays, R, N, M, t_near,
                       t_far, d_label, d_t, d_cell, d_source);
    return dmn_check_launch("label_trace");
}
