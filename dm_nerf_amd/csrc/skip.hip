// skip.hip -- the occupancy bit grid that lets a render skip samples in empty space: build it, and mark + compact the samples of a
// chunk of rays against it (the networks over the compacted list: mlp_fwd_sparse.hip; the render: api.hip).
//
// The grid is an axis-aligned box in world coordinates, dims = (dx, dy, dz) cells, one bit per cell in uint32 words: cell
// g = (i * dy + j) * dz + k sits in word g >> 5 at bit g & 31; the unused high bits of the last word are 0.
//
//   dmnerf_skip_grid_build   bit(g) = any sigma in the (2 dilate + 1)^3 neighbourhood of g, clipped at the faces, is > threshold;
//                            NaN counts as occupied (the test is !(sigma <= threshold)).
//   dmnerf_skip_select       flag [N,S], the ascending list sel of the flagged samples, and its length, which stays on the device.
//   dmnerf_skip_select_fill  the same, and in the same pass every row of rows [N*S, width] whose flag is 0 becomes a copy of
//                            fill_row [width]; flagged rows are left for the sparse network.  The manipulation render passes
//                            the EMPTY ROW (0, 0, 0, 0 | 0, .., 0, 1): sigma 0 is exactly neutral to the compositing, and the
//                            argmax over its C logits is C - 1, the label of empty space, never the label of a moved object
//                            ("The empty row").
//
//   dmnerf_skip_grid_mark    the grid from rendered views: the cell of every sample whose compositing weight is > threshold (NaN
//                            counts) gets its bit OR-ed in; bits are only ever set.
//   dmnerf_skip_grid_dilate  out(g) = OR of in over the (2 dilate + 1)^3 neighbourhood of g, clipped at the faces: the build's
//                            dilation with a set bit as the predicate.
//
// No atomics, with one exception: in build and dilate a word of the grid is written by the one lane that holds its ballot, and the
// select's compaction is three passes (per-block counts, one scan of the counts, scatter by prefix sums), so the list is in ascending
// order and the same every run.  The exception is skip_mark_kernel: samples of many rays fall into one word, so a lane ORs its bit in
// with atomicOr -- after reading the word, and only where the bit still reads clear, so once the bits have saturated the kernel
// only loads.  OR is commutative and associative: whatever the order of the lanes, the words are the same every run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "grid_volume.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_DILATE = 4;

// ---- build.  A block owns 256 consecutive cells [g0, g0 + 256) = 8 whole words.  The neighbour (i + di, j + dj, k + dk) of cell g,
// where it exists, is cell g + (di * dy + dj) * dz + dk: for every (di, dj) the neighbours of the block's cells are again one
// contiguous run of 256 + 2 dilate cells.  The LDS tile holds the occupancy predicate of these (2 dilate + 1)^2 runs (halo included);
// whether a neighbour exists is decided per cell from its coordinates (the clipping at the faces), so a run's entries that belong
// to a neighbouring row are never used by mistake.
__global__ __launch_bounds__(BLOCK) void skip_grid_build_kernel(const float* __restrict__ sigma, int dx, int dy, int dz, float threshold,
                                                                int d, uint32_t* __restrict__ bits) {
    extern __shared__ unsigned char tile[];                    // [(2d+1)^2][256 + 2d]
    const int D = 2 * d + 1, SEG = BLOCK + 2 * d;
    const int64_t total = (int64_t)dx * dy * dz;
    const int64_t g0 = (int64_t)blockIdx.x * BLOCK;
    for (int idx = threadIdx.x; idx < D * D * SEG; idx += BLOCK) {
        const int seg = idx / SEG, t = idx - seg * SEG;
        const int di = seg / D - d, dj = seg % D - d;
        const int64_t gl = g0 - d + t + ((int64_t)di * dy + dj) * dz;
        unsigned char v = 0;
        if (gl >= 0 && gl < total) v = !(sigma[gl] <= threshold);          // NaN: occupied
        tile[idx] = v;
    }
    __syncthreads();
    const int64_t g = g0 + threadIdx.x;
    bool occ = false;
    if (g < total) {
        const int k = (int)(g % dz);
        const int64_t r = g / dz;
        const int j = (int)(r % dy), i = (int)(r / dy);
        for (int di = -d; di <= d; ++di) {
            if (i + di < 0 || i + di >= dx) continue;
            for (int dj = -d; dj <= d; ++dj) {
                if (j + dj < 0 || j + dj >= dy) continue;
                const unsigned char* run = tile + ((di + d) * D + (dj + d)) * SEG + threadIdx.x + d;
                for (int dk = -d; dk <= d; ++dk)
                    if (k + dk >= 0 && k + dk < dz) occ |= run[dk] != 0;
            }
        }
    }
    const unsigned long long ballot = __ballot(occ);           // 64 cells = 2 words; lanes 0 and 32 each own one
    const int lane = threadIdx.x & 63;
    if ((lane & 31) == 0) {
        const int64_t w = (g0 + (threadIdx.x & ~63)) / 32 + (lane >> 5);
        if (w < (total + 31) / 32) bits[w] = (uint32_t)(ballot >> (lane & 32));
    }
}

// ---- select, pass 1: the flag of every sample and the number of flagged samples of every block.  The cell of a sample is
// grid_cell_of_sample (grid_volume.h): what this flags is what the sparse network evaluates and what skip_mark_kernel marks.
struct GridDev {
    GridBox box;
    int outside_flag;          // the flag of a sample outside the box: 1 ("evaluate") or 0 ("empty")
    const uint32_t* bits;
};

__device__ __forceinline__ bool skip_flag_of(const GridDev& G, const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n,
                                             float zv) {
    int64_t g;
    const bool inside = grid_cell_of_sample(G.box, rays_o, rays_d, n, zv, &g);
    return inside ? ((G.bits[g >> 5] >> (g & 31)) & 1u) != 0 : G.outside_flag != 0;
}

__global__ __launch_bounds__(BLOCK) void skip_flag_kernel(GridDev G, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                          const float* __restrict__ z, int64_t M, int S, uint8_t* __restrict__ flag,
                                                          int* __restrict__ block_n) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool f = false;
    if (m < M) {
        f = skip_flag_of(G, rays_o, rays_d, m / S, z[m]);
        flag[m] = f ? 1 : 0;
    }
    int rank;
    const int total = block_count_and_rank<BLOCK>(f, &rank);
    if (threadIdx.x == 0) block_n[blockIdx.x] = total;
}

// ---- select-and-fill, pass 1: skip_flag_kernel that also writes fill_row into the rows of the samples it does not flag: the block's
// samples are rows [m0, m0 + 256) of `rows` (fill_block_rows, grid_volume.h).
__global__ __launch_bounds__(BLOCK) void skip_flag_fill_kernel(GridDev G, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                               const float* __restrict__ z, int64_t M, int S, uint8_t* __restrict__ flag,
                                                               int* __restrict__ block_n, float* __restrict__ rows,
                                                               const float* __restrict__ fill_row, int width) {
    __shared__ uint8_t block_fill[BLOCK];
    const int64_t m0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t m = m0 + threadIdx.x;
    bool f = false;
    if (m < M) {
        f = skip_flag_of(G, rays_o, rays_d, m / S, z[m]);
        flag[m] = f ? 1 : 0;
    }
    block_fill[threadIdx.x] = f ? 0 : 1;
    int rank;
    const int total = block_count_and_rank<BLOCK>(f, &rank);     // (its barrier also publishes block_fill)
    if (threadIdx.x == 0) block_n[blockIdx.x] = total;
    fill_block_rows<BLOCK>(block_fill, rows, fill_row, m0, M, width);
}

// ---- mark.  This kernel keeps its own statement of the cell rule and its own argument (the box without `cell`), as it always had
// them: through grid_cell_of_sample and a GridBox the two mark passes measured 4 to 8 % (empty grid) and 17 to 19 % (saturated grid)
// slower in two sessions (profiles/grid_refactor/README.md); like this its instruction text is the parent's.  The statements are
// grid_cell_of_sample's, operation for operation, and tests/_mark_restate.py holds them to the one numpy cell rule.
struct CellDev {
    float lo[3], inv_cell[3];
    int dims[3];
};

__device__ __forceinline__ bool skip_cell_of(const CellDev& G, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                             int64_t n, float zv, int64_t* g_out) {
    bool inside = true;
    int64_t g = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = __fadd_rn(rays_o[n * 3 + a], __fmul_rn(rays_d[n * 3 + a], zv));
        const float c = floorf(__fmul_rn(__fsub_rn(p, G.lo[a]), G.inv_cell[a]));
        inside = inside && (c >= 0.f) && (c < (float)G.dims[a]);
        g = g * G.dims[a] + (inside ? (int)c : 0);
    }
    *g_out = g;
    return inside;
}

// One sample per lane: consecutive lanes read consecutive z and w.  A sample marks iff it is inside the box and !(w <= threshold)
// (NaN marks).  The word is read first (a relaxed atomic load: other lanes may be OR-ing into it) and the atomicOr is issued only
// where the bit reads clear; a stale read costs one redundant OR, never a lost bit.  inside => 0 <= g < cells, so the word exists
// and the unused bits of the last word are never touched.
__global__ __launch_bounds__(BLOCK) void skip_mark_kernel(CellDev G, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                          const float* __restrict__ z, const float* __restrict__ w, int64_t M, int S,
                                                          float threshold, uint32_t* bits) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (m >= M) return;
    const float wv = w[m], zv = z[m];
    if (wv <= threshold) return;
    int64_t g;
    if (!skip_cell_of(G, rays_o, rays_d, m / S, zv, &g)) return;
    uint32_t* word = bits + (g >> 5);
    const uint32_t bit = 1u << (g & 31);
    if ((__atomic_load_n(word, __ATOMIC_RELAXED) & bit) == 0) atomicOr(word, bit);
}

// ---- dilate.  skip_grid_build_kernel's tiling (a block owns 256 consecutive cells = 8 whole words; the LDS tile holds the predicate of
// the (2 d + 1)^2 runs of 256 + 2 d cells; the clipping at the faces is decided per cell from its coordinates) with bit gl of `in`
// as the predicate instead of sigma[gl] > threshold.  A kernel of its own: the build kernel is left as it is.
__global__ __launch_bounds__(BLOCK) void skip_grid_dilate_kernel(const uint32_t* __restrict__ in, int dx, int dy, int dz, int d,
                                                                 uint32_t* __restrict__ bits) {
    extern __shared__ unsigned char tile[];                    // [(2d+1)^2][256 + 2d]
    const int D = 2 * d + 1, SEG = BLOCK + 2 * d;
    const int64_t total = (int64_t)dx * dy * dz;
    const int64_t g0 = (int64_t)blockIdx.x * BLOCK;
    for (int idx = threadIdx.x; idx < D * D * SEG; idx += BLOCK) {
        const int seg = idx / SEG, t = idx - seg * SEG;
        const int di = seg / D - d, dj = seg % D - d;
        const int64_t gl = g0 - d + t + ((int64_t)di * dy + dj) * dz;
        unsigned char v = 0;
        if (gl >= 0 && gl < total) v = (in[gl >> 5] >> (gl & 31)) & 1u;
        tile[idx] = v;
    }
    __syncthreads();
    const int64_t g = g0 + threadIdx.x;
    bool occ = false;
    if (g < total) {
        const int k = (int)(g % dz);
        const int64_t r = g / dz;
        const int j = (int)(r % dy), i = (int)(r / dy);
        for (int di = -d; di <= d; ++di) {
            if (i + di < 0 || i + di >= dx) continue;
            for (int dj = -d; dj <= d; ++dj) {
                if (j + dj < 0 || j + dj >= dy) continue;
                const unsigned char* run = tile + ((di + d) * D + (dj + d)) * SEG + threadIdx.x + d;
                for (int dk = -d; dk <= d; ++dk)
                    if (k + dk >= 0 && k + dk < dz) occ |= run[dk] != 0;
            }
        }
    }
    const unsigned long long ballot = __ballot(occ);           // 64 cells = 2 words; lanes 0 and 32 each own one
    const int lane = threadIdx.x & 63;
    if ((lane & 31) == 0) {
        const int64_t w = (g0 + (threadIdx.x & ~63)) / 32 + (lane >> 5);
        if (w < (total + 31) / 32) bits[w] = (uint32_t)(ballot >> (lane & 32));
    }
}

// ---- pass 2: exclusive scan of the block counts in place (one workgroup walks them, 1024 at a time) and the grand total
__global__ __launch_bounds__(1024) void skip_scan_kernel(int* __restrict__ block_n, int64_t nb, int* __restrict__ count) {
    __shared__ int buf[1024];
    const int tid = threadIdx.x;
    int carry = 0;                                             // the same in every thread
    for (int64_t base = 0; base < nb; base += 1024) {
        const int64_t i = base + tid;
        const int v = i < nb ? block_n[i] : 0;
        buf[tid] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int t = tid >= off ? buf[tid - off] : 0;
            __syncthreads();
            buf[tid] += t;
            __syncthreads();
        }
        if (i < nb) block_n[i] = carry + buf[tid] - v;
        carry += buf[1023];
        __syncthreads();
    }
    if (tid == 0) *count = carry;
}

// ---- pass 3: sample m goes to sel[block offset + rank within the block]; a sample is selected iff its byte is not `none`
// (0 for the select's flags, 255 for the field edit's owners)
__global__ __launch_bounds__(BLOCK) void skip_scatter_kernel(const uint8_t* __restrict__ flag, int none, const int* __restrict__ block_off,
                                                             int64_t M, int* __restrict__ sel) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool f = m < M && flag[m] != none;
    int rank;
    (void)block_count_and_rank<BLOCK>(f, &rank);
    if (f) sel[block_off[blockIdx.x] + rank] = (int)m;
}

__global__ void skip_set_int_kernel(int* p, int v) { *p = v; }

// (the running sums += (selected, M); one thread, a plain read-modify-write ordered by the stream)
__global__ void skip_add_totals_kernel(const int* __restrict__ count, int64_t M, int64_t* __restrict__ totals) {
    totals[0] += *count;
    totals[1] += M;
}

}  // namespace

// (api.hip: the sample count of a level that is rendered dense)
int dmn_skip_set_int(int* d_p, int v, hipStream_t stream) {
    hipLaunchKernelGGL(skip_set_int_kernel, dim3(1), dim3(1), 0, stream, d_p, v);
    return dmn_check_launch("skip: set count");
}

// Passes 2 and 3 of a selection whose pass 1 left one byte per sample and the per-block counts (blocks of 256 samples) in d_work: the
// scan, the scatter of the samples whose byte is not `none` into d_sel, *d_count, and (d_totals, may be NULL) the running sums.  The
// caller checks the launches (dmn_check_launch).  Declared in common.h: field_edit.hip selects by owner with it.
void dmn_select_finish(const uint8_t* d_byte, int none, int64_t M, int* d_work, int* d_sel, int* d_count, int64_t* d_totals, hipStream_t st) {
    const int64_t nb = (M + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(skip_scan_kernel, dim3(1), dim3(1024), 0, st, d_work, nb, d_count);
    hipLaunchKernelGGL(skip_scatter_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, d_byte, none, d_work, M, d_sel);
    if (d_totals) hipLaunchKernelGGL(skip_add_totals_kernel, dim3(1), dim3(1), 0, st, d_count, M, d_totals);
}

extern "C" int dmnerf_skip_grid_build(const float* d_sigma, int dx, int dy, int dz, float threshold, int dilate, uint32_t* d_bits,
                                      void* stream) {
    const int dims[3] = {dx, dy, dz};
    int64_t total;
    if (int rc = dmn_grid_dims("skip_grid_build", dims)) return rc;
    if (dilate < 0 || dilate > MAX_DILATE) return dmn_fail(DMNERF_E_ARG, "skip_grid_build: dilate %d outside 0..%d", dilate, MAX_DILATE);
    if (int rc = dmn_grid_cells("skip_grid_build", dims, &total)) return rc;
    if (!d_sigma || !d_bits) return dmn_fail(DMNERF_E_ARG, "skip_grid_build: null pointer");
    const int D = 2 * dilate + 1;
    const size_t lds = (size_t)D * D * (BLOCK + 2 * dilate);   // <= 81 * 264 B
    hipLaunchKernelGGL(skip_grid_build_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), lds, (hipStream_t)stream,
                       d_sigma, dx, dy, dz, threshold, dilate, d_bits);
    return dmn_check_launch("skip_grid_build");
}

extern "C" int64_t dmnerf_skip_select_work_ints(int64_t M) {
    if (M < 0 || M >= (1LL << 31)) return -1;
    return (M + BLOCK - 1) / BLOCK + 1;
}

static int skip_select_impl(const char* who, const dmnerf_skip_grid* grid, const float* d_rays_o, const float* d_rays_d, const float* d_z,
                            int64_t N, int S, uint8_t* d_flag, int* d_sel, int* d_count, int* d_work, float* d_rows,
                            const float* d_fill_row, int width, int64_t* d_totals, hipStream_t st) {
    if (!grid) return dmn_fail(DMNERF_E_ARG, "%s: null grid", who);
    if (N < 0 || S < 1) return dmn_fail(DMNERF_E_ARG, "%s: bad N=%lld S=%d", who, (long long)N, S);
    const int64_t M = N * S;
    if (M >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "%s: %lld samples do not fit the int32 selection", who, (long long)M);
    if (grid->outside != DMNERF_SKIP_OUTSIDE_EVALUATE && grid->outside != DMNERF_SKIP_OUTSIDE_EMPTY)
        return dmn_fail(DMNERF_E_ARG, "%s: outside policy %d unknown", who, grid->outside);
    GridDev G;
    int64_t cells;
    if (int rc = dmn_grid_given(who, grid->lo, nullptr, grid->inv_cell, grid->dims, &G.box, &cells)) return rc;
    G.outside_flag = grid->outside == DMNERF_SKIP_OUTSIDE_EVALUATE ? 1 : 0;
    G.bits = grid->d_bits;
    if (!d_count) return dmn_fail(DMNERF_E_ARG, "%s: null pointer", who);
    if (d_rows && (!d_fill_row || width < 1 || width > (1 << 16)))
        return dmn_fail(DMNERF_E_ARG, "%s: rows without a fill row, or bad width %d", who, width);
    if (M == 0) return dmn_skip_set_int(d_count, 0, st);
    if (!grid->d_bits || !d_rays_o || !d_rays_d || !d_z || !d_flag || !d_sel || !d_work) return dmn_fail(DMNERF_E_ARG, "%s: null pointer", who);
    const int64_t nb = (M + BLOCK - 1) / BLOCK;
    if (d_rows)
        hipLaunchKernelGGL(skip_flag_fill_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, G, d_rays_o, d_rays_d, d_z, M, S, d_flag, d_work,
                           d_rows, d_fill_row, width);
    else                                                           // (dmnerf_skip_select: the three kernels it always launched)
        hipLaunchKernelGGL(skip_flag_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, G, d_rays_o, d_rays_d, d_z, M, S, d_flag, d_work);
    dmn_select_finish(d_flag, 0, M, d_work, d_sel, d_count, d_totals, st);
    return dmn_check_launch(who);
}

extern "C" int dmnerf_skip_select(const dmnerf_skip_grid* grid, const float* d_rays_o, const float* d_rays_d, const float* d_z,
                                  int64_t N, int S, uint8_t* d_flag, int* d_sel, int* d_count, int* d_work, void* stream) {
    return skip_select_impl("skip_select", grid, d_rays_o, d_rays_d, d_z, N, S, d_flag, d_sel, d_count, d_work, nullptr, nullptr, 0, nullptr,
                            (hipStream_t)stream);
}

// dmnerf_skip_select with one more duty in its first pass: row m of d_rows [N*S, width] becomes d_fill_row [width] where flag m is 0
// (flagged rows are left untouched: the sparse network writes them afterwards).  The manipulation render's fill row is the empty
// row E = (0, 0, 0, 0 | 0, .., 0, 1): neutral to manipulator_render and labelled C - 1 by the exchanger.  d_rows == NULL: exactly
// dmnerf_skip_select.  d_totals (may be NULL): [2] int64 on the device, += (*d_count, N * S) by a one-thread kernel behind the select:
// a plain read-modify-write, so all calls that share one d_totals must be on one stream; N * S == 0 adds nothing.  Nothing reaches
// the host.
extern "C" int dmnerf_skip_select_fill(const dmnerf_skip_grid* grid, const float* d_rays_o, const float* d_rays_d, const float* d_z,
                                       int64_t N, int S, uint8_t* d_flag, int* d_sel, int* d_count, int* d_work, float* d_rows,
                                       const float* d_fill_row, int width, int64_t* d_totals, void* stream) {
    return skip_select_impl("skip_select_fill", grid, d_rays_o, d_rays_d, d_z, N, S, d_flag, d_sel, d_count, d_work, d_rows, d_fill_row,
                            width, d_totals, (hipStream_t)stream);
}

// The grid from rendered views: OR the bit of every sample's cell whose weight is > threshold (NaN counts) into d_bits.  Reads lo /
// inv_cell / dims of `grid` only.  No allocation, no synchronisation.
extern "C" int dmnerf_skip_grid_mark(const dmnerf_skip_grid* grid, uint32_t* d_bits, const float* d_rays_o, const float* d_rays_d,
                                     const float* d_z, const float* d_weights, int64_t N, int S, float threshold, void* stream) {
    if (!grid) return dmn_fail(DMNERF_E_ARG, "skip_grid_mark: null grid");
    if (int rc = dmn_check_rays("skip_grid_mark", 1, N, S, true)) return rc;          // (no network here: ins_num 1 always passes)
    if (!(threshold >= 0.f)) return dmn_fail(DMNERF_E_ARG, "skip_grid_mark: threshold %g must be >= 0", (double)threshold);
    GridBox box;
    int64_t cells;
    if (int rc = dmn_grid_given("skip_grid_mark", grid->lo, nullptr, grid->inv_cell, grid->dims, &box, &cells)) return rc;
    CellDev G;
    for (int a = 0; a < 3; ++a) { G.lo[a] = box.lo[a]; G.inv_cell[a] = box.inv_cell[a]; G.dims[a] = box.dims[a]; }
    if (!d_bits || !d_rays_o || !d_rays_d || !d_z || !d_weights) return dmn_fail(DMNERF_E_ARG, "skip_grid_mark: null pointer");
    if (N == 0) return DMNERF_OK;
    const int64_t M = N * S;
    hipLaunchKernelGGL(skip_mark_kernel, dim3((unsigned)((M + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, G, d_rays_o,
                       d_rays_d, d_z, d_weights, M, S, threshold, d_bits);
    return dmn_check_launch("skip_grid_mark");
}

extern "C" int dmnerf_skip_grid_dilate(const uint32_t* d_bits_in, int dx, int dy, int dz, int dilate, uint32_t* d_bits_out,
                                       void* stream) {
    const int dims[3] = {dx, dy, dz};
    int64_t total;
    if (int rc = dmn_grid_dims("skip_grid_dilate", dims)) return rc;
    if (dilate < 0 || dilate > MAX_DILATE) return dmn_fail(DMNERF_E_ARG, "skip_grid_dilate: dilate %d outside 0..%d", dilate, MAX_DILATE);
    if (int rc = dmn_grid_cells("skip_grid_dilate", dims, &total)) return rc;
    if (!d_bits_in || !d_bits_out) return dmn_fail(DMNERF_E_ARG, "skip_grid_dilate: null pointer");
    if (d_bits_in == d_bits_out) return dmn_fail(DMNERF_E_ARG, "skip_grid_dilate: in and out must be different buffers");
    const int D = 2 * dilate + 1;
    const size_t lds = (size_t)D * D * (BLOCK + 2 * dilate);   // <= 81 * 264 B
    hipLaunchKernelGGL(skip_grid_dilate_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), lds, (hipStream_t)stream,
                       d_bits_in, dx, dy, dz, dilate, d_bits_out);
    return dmn_check_launch("skip_grid_dilate");
}
