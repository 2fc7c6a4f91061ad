// grid_volume.h -- what everything that reads a grid volume shares.  A grid volume is an axis-aligned box in world coordinates of
// dims = (dx, dy, dz) cells, cell (i, j, k) at index g = (i * dy + j) * dz + k, holding bits (skip.hip), labels (label_grid.hip,
// label_trace.hip), baked colour (baked.hip) or an owner byte (volume_edit.hip, field_edit.hip).  Four rules, each stated once:
//
//   the cell of a point      grid_cell_of / grid_cell_of_sample
//   the bit of a label mask  LabelMask128 / mask_bit
//   the walk along a ray     walk_clip_axis / walk_start_cell / walk_step / walk_apply (Amanatides-Woo)
//   the selection            block_count_and_rank / fill_block_rows (the scan and the scatter behind them: skip.hip, dmn_select_finish)
//
// Every f32 operation is rounded on its own and minimum / maximum are written out as comparisons, so tests/_grid_restate.py and the
// per-feature restatements state them in numpy bit for bit.  All helpers are forced inline: a box that is a kernel argument stays in
// scalar registers, and nothing here may put a kernel into scratch (scripts/check_no_scratch.py fails the build on it).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct GridBox {
    float lo[3], cell[3], inv_cell[3];         // (cell is 0 for a box whose reader takes none: the bit grid)
    int dims[3];
};

// ---- the cell of a point p: c_a = floor of (p_a - lo_a) * inv_cell_a, subtract, multiply and floor each rounded on its own; the inside
// test is on the float, so a NaN point is outside; the index is accumulated per axis.  -> inside; *g_out = the cell's index where inside.
__device__ __forceinline__ bool grid_cell_of(const GridBox& B, float p0, float p1, float p2, int64_t* g_out) {
    const float p[3] = {p0, p1, p2};
    bool inside = true;
    int64_t g = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float c = floorf(__fmul_rn(__fsub_rn(p[a], B.lo[a]), B.inv_cell[a]));
        inside = inside && (c >= 0.f) && (c < (float)B.dims[a]);
        g = g * B.dims[a] + (inside ? (int)c : 0);
    }
    *g_out = g;
    return inside;
}

// ... of sample (ray n, depth zv): p = o + d z with a separate multiply and add, as the MLP prologue computes it (render.py:49), so a
// sample that is marked or selected here is the sample the network evaluates.
__device__ __forceinline__ bool grid_cell_of_sample(const GridBox& B, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                    int64_t n, float zv, int64_t* g_out) {
    return grid_cell_of(B, __fadd_rn(rays_o[n * 3 + 0], __fmul_rn(rays_d[n * 3 + 0], zv)),
                        __fadd_rn(rays_o[n * 3 + 1], __fmul_rn(rays_d[n * 3 + 1], zv)),
                        __fadd_rn(rays_o[n * 3 + 2], __fmul_rn(rays_d[n * 3 + 2], zv)), g_out);
}

// ---- a set of labels 0 .. 127 as a kernel argument: label l is bit l & 31 of word l >> 5; a label >= 128 (255, unlabelled) is in no set
struct LabelMask128 {
    uint32_t w[4];
};

// (a select chain and not m.w[l >> 5]: a per-lane index into a kernel argument would put the mask into scratch)
__device__ __forceinline__ bool mask_bit(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t l) {
    const uint32_t q = l >> 5;
    const uint32_t word = q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : q == 3 ? w3 : 0u;
    return ((word >> (l & 31)) & 1u) != 0;
}
__device__ __forceinline__ bool mask_bit(const LabelMask128& m, uint32_t l) { return mask_bit(m.w[0], m.w[1], m.w[2], m.w[3], l); }

// ---- the walk of a ray through the cells (label_trace.hip's header has the whole statement).  minimum and maximum that hand a NaN
// operand on (fminf / fmaxf drop it); plane b of an axis.
__device__ __forceinline__ float nan_min(float x, float y) { return (x < y || x != x) ? x : y; }
__device__ __forceinline__ float nan_max(float x, float y) { return (x > y || x != x) ? x : y; }
__device__ __forceinline__ float plane_of(float lo, float cell, int b) { return __fadd_rn(lo, __fmul_rn((float)b, cell)); }

struct WalkRay {
    float o0, o1, o2, d0, d1, d2;
    float inv0, inv1, inv2;                    // 1 / d_a; +inf where d_a == 0 (walk_clip_axis leaves the caller's +inf)
};

// clip against the slab [lo, hi) of one axis: an axis with d == 0 bounds nothing if lo <= o < hi and makes the ray miss otherwise
__device__ __forceinline__ void walk_clip_axis(float lo, float hi, float o, float d, float& inv, float& t_enter, float& t_exit, bool& miss) {
    if (d == 0.f) {
        miss = miss || !(lo <= o && o < hi);
    } else {
        inv = __fdiv_rn(1.f, d);
        const float t0 = __fmul_rn(__fsub_rn(lo, o), inv), t1 = __fmul_rn(__fsub_rn(hi, o), inv);
        t_enter = nan_max(t_enter, nan_min(t0, t1));
        t_exit = nan_min(t_exit, nan_max(t0, t1));
    }
}

// the cell rule on p = o + d * t_enter, clamped into [0, dim - 1]
__device__ __forceinline__ int walk_start_cell(float o, float d, float t_enter, float lo, float inv_cell, int dim) {
    const float f = floorf(__fmul_rn(__fsub_rn(__fadd_rn(o, __fmul_rn(d, t_enter)), lo), inv_cell));
    return f >= 0.f ? (f < (float)dim ? (int)f : dim - 1) : 0;                       // (a NaN: 0)
}

// From cell (c0, c1, c2): tmax_a = (plane_a(c_a + (d_a > 0)) - o_a) * inv_a (+inf where d_a == 0), from the integer index and never
// accumulated; the axis of the smallest steps, the lowest on ties.  -> tmax < t_exit: the ray goes on into the next cell.
__device__ __forceinline__ bool walk_step(const GridBox& G, const WalkRay& r, int c0, int c1, int c2, float t_exit, int* axis_out, float* tm_out) {
    const float inf = __builtin_huge_valf();
    const int up0 = r.d0 > 0.f, up1 = r.d1 > 0.f, up2 = r.d2 > 0.f;
    const float tm0 = r.d0 == 0.f ? inf : __fmul_rn(__fsub_rn(plane_of(G.lo[0], G.cell[0], c0 + up0), r.o0), r.inv0);
    const float tm1 = r.d1 == 0.f ? inf : __fmul_rn(__fsub_rn(plane_of(G.lo[1], G.cell[1], c1 + up1), r.o1), r.inv1);
    const float tm2 = r.d2 == 0.f ? inf : __fmul_rn(__fsub_rn(plane_of(G.lo[2], G.cell[2], c2 + up2), r.o2), r.inv2);
    int axis = 0;
    float tm = tm0;
    if (tm1 < tm) { axis = 1; tm = tm1; }
    if (tm2 < tm) { axis = 2; tm = tm2; }
    *axis_out = axis;
    *tm_out = tm;
    return tm < t_exit;
}

// The step: t = max(t, tmax), one cell along `axis`.  -> the step left the index range.
__device__ __forceinline__ bool walk_apply(const GridBox& G, const WalkRay& r, int axis, float tm, int& c0, int& c1, int& c2, float& t) {
    t = tm > t ? tm : t;
    c0 += axis == 0 ? (r.d0 > 0.f ? 1 : -1) : 0;
    c1 += axis == 1 ? (r.d1 > 0.f ? 1 : -1) : 0;
    c2 += axis == 2 ? (r.d2 > 0.f ? 1 : -1) : 0;
    return c0 < 0 || c0 >= G.dims[0] || c1 < 0 || c1 >= G.dims[1] || c2 < 0 || c2 >= G.dims[2];
}

// ---- selection: the ascending list of the flagged samples in three passes (per-block counts, one scan of the counts, scatter by
// prefix sums), so the list is the same every run.  -> the block's total; *rank_out = number of flagged threads before this one.
template <int BLOCK>
__device__ __forceinline__ int block_count_and_rank(bool f, int* rank_out) {
    __shared__ int wave_n[BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    if (lane == 0) wave_n[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
        if (w < wave) before += wave_n[w];
        total += wave_n[w];
    }
    *rank_out = before + __popcll(b & ((1ull << lane) - 1ull));
    return total;
}

// The block's run of rows [m0, m0 + nrows) of `rows`, one contiguous run of nrows * width floats: fill_row[column] into the rows whose
// byte of `fill` (LDS, published by the caller's barrier) is set.  width = 4 + C is rarely a multiple of 4 and a row is not 16-byte
// aligned, so the run is written one float per lane and step (a wave stores 256 consecutive bytes); (row, column) advance by
// (BLOCK / width, BLOCK % width) per step: no division in the loop.
template <int BLOCK>
__device__ __forceinline__ void fill_block_rows(const uint8_t* fill, float* __restrict__ rows, const float* __restrict__ fill_row, int64_t m0,
                                                int64_t M, int width) {
    const int nrows = (int)(M - m0 < BLOCK ? M - m0 : BLOCK);
    const int run = nrows * width;
    float* out = rows + m0 * width;
    const int dr = BLOCK / width, dc = BLOCK - dr * width;
    int r = threadIdx.x / width, c = threadIdx.x - r * width;
    for (int i = threadIdx.x; i < run; i += BLOCK) {
        if (fill[r]) out[i] = fill_row[c];
        r += dr; c += dc;
        if (c >= width) { c -= width; ++r; }
    }
}
