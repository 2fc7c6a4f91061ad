// label_grid.hip -- the occupancy volume labelled by object: which object owns a cell, what each object covers, and the bit grid of a
// set of objects.  The device work BEHIND the network: render.run_network_skip evaluates the fine network at one point per cell
// (field.label_grid), and the three kernels here turn its rows into labels, the labels into per-object sums, and labels into bits.
//
//   dmnerf_label_cells            row m of raw [M, 4 + C] -> labels[m]: the first index of the maximum of the C logits raw[m, 4:] if
//                                 raw[m, 3] > sigma_threshold, else 255 (UNLABELLED).  The comparison is exactly that one, so a NaN
//                                 sigma is unlabelled, and so is the empty row (sigma 0) for every threshold >= 0.  The argmax is
//                                 label_conf_kernel's (render_kernels.hip): best = 0, then channel c > 0 replaces it iff
//                                 x[c] > x[best].  Hence ties go to the first channel, a NaN logit in a channel c > 0 is never
//                                 chosen, and a NaN in channel 0 is never replaced: the label is 0.  The exchanger's rule is this
//                                 walk over ALL C logits behind a sigmoid (argmax_sigmoid, render_kernels.hip), which is monotone:
//                                 a cell labelled k is a cell whose centre sample the manipulation render treats as object k
//                                 (they can differ only where two unequal logits round to one f32 sigmoid, both above ~17).
//   dmnerf_bake_cells             dmnerf_label_cells, and cells[m, 0:4] = raw[m, 0:4] bit for bit for a labelled row, four zeros for an
//                                 unlabelled one: the colour logits and the density that csrc/baked.hip composites along rays.
//   dmnerf_label_stats            per label l < C over labels [dx, dy, dz]: the number of cells, the sums of their i, j and k, the
//                                 smallest index and the largest index + 1 per axis.  Labels >= C (255 included) are ignored.
//   dmnerf_skip_grid_from_labels  bit g = labels[g] < 128 and bit labels[g] of a 128-bit mask: SkipGrid's words (skip.hip).
//
// The stats are integers throughout.  A lane walks 16 consecutive cells and adds a run of equal labels to the workgroup's LDS table in
// one go (objects are blobs: a run is usually the whole 16 cells); the table is flushed with integer atomicAdd / atomicMin /
// atomicMax, which commute, so the result is the same every run.  No float atomics.  The bit grid is one cell per lane and one word
// per 32-lane half of a ballot, as in skip.hip: no atomics, every word written once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "grid_volume.h"

namespace {

constexpr int BLOCK = 256;
constexpr int UNLABELLED = 255;
constexpr int RUN = 16;                       // cells per lane and step of the stats kernel: one 16-byte load
constexpr int STATS_MAX_BLOCKS = 2048;        // the stats grid; beyond it a workgroup strides

// ---- labels.  One sample per lane; a row is 4 + C <= 132 floats.
__device__ __forceinline__ int label_of_row(const float* __restrict__ x, int C, float sigma_threshold) {
    int best = UNLABELLED;
    if (x[3] > sigma_threshold) {             // (false for NaN)
        best = 0;
        float bv = x[4];
        for (int c = 1; c < C; ++c) {
            const float v = x[4 + c];
            if (v > bv) { bv = v; best = c; }
        }
    }
    return best;
}

__global__ __launch_bounds__(BLOCK) void label_cells_kernel(const float* __restrict__ raw, int64_t M, int C, float sigma_threshold,
                                                            uint8_t* __restrict__ labels) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (m >= M) return;
    labels[m] = (uint8_t)label_of_row(raw + m * (4 + C), C, sigma_threshold);
}

// The same rule, and what the row says about colour and density kept next to the label: the row's first four words (three colour
// logits, sigma) as they are for a labelled cell, zeros for an unlabelled one; one 16-byte store per row.  (The words travel as
// integers: a NaN keeps its payload.)
__global__ __launch_bounds__(BLOCK) void bake_cells_kernel(const float* __restrict__ raw, int64_t M, int C, float sigma_threshold,
                                                           uint8_t* __restrict__ labels, uint4* __restrict__ cells) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (m >= M) return;
    const float* x = raw + m * (4 + C);
    const int best = label_of_row(x, C, sigma_threshold);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (best != UNLABELLED) {
        const uint32_t* u = reinterpret_cast<const uint32_t*>(x);
        v = make_uint4(u[0], u[1], u[2], u[3]);
    }
    labels[m] = (uint8_t)best;
    cells[m] = v;
}

// ---- stats
struct StatsTable {                           // one workgroup's sums, per label
    unsigned long long sum[DMNERF_MAX_LOGITS][3];
    unsigned int count[DMNERF_MAX_LOGITS];
    int lo[DMNERF_MAX_LOGITS][3], hi[DMNERF_MAX_LOGITS][3];     // inclusive minimum, inclusive maximum
};

struct StatsRun {                             // a lane's current run of equal labels
    int label;
    unsigned int count;
    unsigned long long sum[3];
    int lo[3], hi[3];
};

__device__ __forceinline__ void stats_flush_run(StatsTable& T, const StatsRun& r) {
    if (r.count == 0) return;
    atomicAdd(&T.count[r.label], r.count);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicAdd(&T.sum[r.label][a], r.sum[a]);
        atomicMin(&T.lo[r.label][a], r.lo[a]);
        atomicMax(&T.hi[r.label][a], r.hi[a]);
    }
}

__global__ void label_stats_init_kernel(int dx, int dy, int dz, int C, int64_t* __restrict__ count, int64_t* __restrict__ index_sum,
                                        int* __restrict__ lo, int* __restrict__ hi) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= C) return;
    const int dims[3] = {dx, dy, dz};
    count[l] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        index_sum[l * 3 + a] = 0;
        lo[l * 3 + a] = dims[a];
        hi[l * 3 + a] = 0;
    }
}

// Lane t of a workgroup takes cells [g, g + 16) with g = (step * 256 + t) * 16: one 16-byte load where the pointer allows it and the
// 16 cells exist, single bytes otherwise (cells past the end read as UNLABELLED).  (i, j, k) of the first cell by division, of the
// next ones by carry.
__global__ __launch_bounds__(BLOCK) void label_stats_kernel(const uint8_t* __restrict__ labels, int dx, int dy, int dz, int C,
                                                            int aligned16, unsigned long long* __restrict__ count,
                                                            unsigned long long* __restrict__ index_sum, int* __restrict__ lo,
                                                            int* __restrict__ hi) {
    __shared__ StatsTable T;
    for (int l = threadIdx.x; l < C; l += BLOCK) {
        T.count[l] = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            T.sum[l][a] = 0;
            T.lo[l][a] = 0x7fffffff;
            T.hi[l][a] = -1;
        }
    }
    __syncthreads();
    const int64_t total = (int64_t)dx * dy * dz;
    const int64_t stride = (int64_t)gridDim.x * BLOCK * RUN;
    for (int64_t g0 = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * RUN; g0 < total; g0 += stride) {
        uint32_t w[RUN / 4];
        if (aligned16 && g0 + RUN <= total) {
            const uint4 v = *reinterpret_cast<const uint4*>(labels + g0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < RUN / 4; ++q) {
                w[q] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int64_t g = g0 + q * 4 + b;
                    const uint32_t v = g < total ? labels[g] : (uint32_t)UNLABELLED;
                    w[q] |= v << (8 * b);
                }
            }
        }
        int idx[3];
        idx[2] = (int)(g0 % dz);
        const int64_t r = g0 / dz;
        idx[1] = (int)(r % dy);
        idx[0] = (int)(r / dy);
        StatsRun run;
        run.label = -1;
        run.count = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) { run.sum[a] = 0; run.lo[a] = 0; run.hi[a] = 0; }
#pragma unroll
        for (int e = 0; e < RUN; ++e) {
            const int l = (int)((w[e >> 2] >> (8 * (e & 3))) & 0xffu);
            if (l != run.label) {
                stats_flush_run(T, run);
                run.label = l;
                run.count = 0;
            }
            if (l < C) {                                           // (a cell past the end is UNLABELLED >= C)
                if (run.count == 0) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) { run.sum[a] = 0; run.lo[a] = idx[a]; run.hi[a] = idx[a]; }
                }
                ++run.count;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    run.sum[a] += (unsigned long long)idx[a];
                    run.lo[a] = min(run.lo[a], idx[a]);
                    run.hi[a] = max(run.hi[a], idx[a]);
                }
            }
            if (++idx[2] == dz) {
                idx[2] = 0;
                if (++idx[1] == dy) { idx[1] = 0; ++idx[0]; }
            }
        }
        stats_flush_run(T, run);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < C; l += BLOCK) {
        if (T.count[l] == 0) continue;
        atomicAdd(&count[l], (unsigned long long)T.count[l]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicAdd(&index_sum[l * 3 + a], T.sum[l][a]);
            atomicMin(&lo[l * 3 + a], T.lo[l][a]);
            atomicMax(&hi[l * 3 + a], T.hi[l][a] + 1);             // exclusive
        }
    }
}

// ---- bits.  skip.hip's packing: a block owns 256 consecutive cells = 8 whole words; 64 cells = one ballot = 2 words, written by lanes
// 0 and 32.  A cell past the end contributes 0, so the unused bits of the last word are 0.
__global__ __launch_bounds__(BLOCK) void skip_grid_from_labels_kernel(const uint8_t* __restrict__ labels, int64_t n_cells, LabelMask128 mask,
                                                                      uint32_t* __restrict__ bits) {
    const int64_t g0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t g = g0 + threadIdx.x;
    bool set = false;
    if (g < n_cells) {
        set = mask_bit(mask, labels[g]);
    }
    const unsigned long long ballot = __ballot(set);
    const int lane = threadIdx.x & 63;
    if ((lane & 31) == 0) {
        const int64_t w = (g0 + (threadIdx.x & ~63)) / 32 + (lane >> 5);
        if (w < (n_cells + 31) / 32) bits[w] = (uint32_t)(ballot >> (lane & 32));
    }
}

}  // namespace

extern "C" int dmnerf_label_cells(const float* d_raw, int64_t M, int C, float sigma_threshold, uint8_t* d_labels, void* stream) {
    if (int rc = dmn_check_labels("label_cells", C)) return rc;
    if (M < 0) return dmn_fail(DMNERF_E_ARG, "label_cells: bad M=%lld", (long long)M);
    if (!(sigma_threshold >= 0.f)) return dmn_fail(DMNERF_E_ARG, "label_cells: sigma_threshold %g must be >= 0", (double)sigma_threshold);
    const int64_t nb = (M + BLOCK - 1) / BLOCK;
    if (nb > 0x7fffffffLL) return dmn_fail(DMNERF_E_ARG, "label_cells: %lld samples is too many for one launch", (long long)M);
    if (M == 0) return DMNERF_OK;
    if (!d_raw || !d_labels) return dmn_fail(DMNERF_E_ARG, "label_cells: null pointer");
    hipLaunchKernelGGL(label_cells_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, d_raw, M, C, sigma_threshold, d_labels);
    return dmn_check_launch("label_cells");
}

extern "C" int dmnerf_bake_cells(const float* d_raw, int64_t M, int C, float sigma_threshold, uint8_t* d_labels, float* d_cells,
                                 void* stream) {
    if (int rc = dmn_check_labels("bake_cells", C)) return rc;
    if (M < 0) return dmn_fail(DMNERF_E_ARG, "bake_cells: bad M=%lld", (long long)M);
    if (!(sigma_threshold >= 0.f)) return dmn_fail(DMNERF_E_ARG, "bake_cells: sigma_threshold %g must be >= 0", (double)sigma_threshold);
    const int64_t nb = (M + BLOCK - 1) / BLOCK;
    if (nb > 0x7fffffffLL) return dmn_fail(DMNERF_E_ARG, "bake_cells: %lld samples is too many for one launch", (long long)M);
    if (M == 0) return DMNERF_OK;
    if (!d_raw || !d_labels || !d_cells) return dmn_fail(DMNERF_E_ARG, "bake_cells: null pointer");
    if ((uintptr_t)d_cells & 15) return dmn_fail(DMNERF_E_ARG, "bake_cells: d_cells must be 16-byte aligned");
    hipLaunchKernelGGL(bake_cells_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, d_raw, M, C, sigma_threshold, d_labels,
                       reinterpret_cast<uint4*>(d_cells));
    return dmn_check_launch("bake_cells");
}

extern "C" int dmnerf_label_stats(const uint8_t* d_labels, int dx, int dy, int dz, int C, int64_t* d_count, int64_t* d_index_sum,
                                  int32_t* d_lo, int32_t* d_hi, void* stream) {
    const int dims[3] = {dx, dy, dz};
    int64_t total;
    if (int rc = dmn_grid_dims("label_stats", dims)) return rc;
    if (int rc = dmn_grid_cells("label_stats", dims, &total)) return rc;
    if (int rc = dmn_check_labels("label_stats", C)) return rc;
    if (!d_labels || !d_count || !d_index_sum || !d_lo || !d_hi) return dmn_fail(DMNERF_E_ARG, "label_stats: null pointer");
    hipLaunchKernelGGL(label_stats_init_kernel, dim3(1), dim3(DMNERF_MAX_LOGITS), 0, (hipStream_t)stream, dx, dy, dz, C, d_count,
                       d_index_sum, d_lo, d_hi);
    const int64_t per_block = (int64_t)BLOCK * RUN;
    const int64_t nb = (total + per_block - 1) / per_block;
    hipLaunchKernelGGL(label_stats_kernel, dim3((unsigned)(nb < STATS_MAX_BLOCKS ? nb : STATS_MAX_BLOCKS)), dim3(BLOCK), 0,
                       (hipStream_t)stream, d_labels, dx, dy, dz, C, (int)(((uintptr_t)d_labels & 15) == 0),
                       reinterpret_cast<unsigned long long*>(d_count), reinterpret_cast<unsigned long long*>(d_index_sum), d_lo, d_hi);
    return dmn_check_launch("label_stats");
}

extern "C" int dmnerf_skip_grid_from_labels(const uint8_t* d_labels, int64_t n_cells, const uint32_t mask[4], uint32_t* d_bits,
                                            void* stream) {
    if (n_cells < 1 || n_cells >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "skip_grid_from_labels: bad n_cells=%lld", (long long)n_cells);
    if (!d_labels || !mask || !d_bits) return dmn_fail(DMNERF_E_ARG, "skip_grid_from_labels: null pointer");
    LabelMask128 m;
    for (int q = 0; q < 4; ++q) m.w[q] = mask[q];
    hipLaunchKernelGGL(skip_grid_from_labels_kernel, dim3((unsigned)((n_cells + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                       d_labels, n_cells, m, d_bits);
    return dmn_check_launch("skip_grid_from_labels");
}
