// components.hip -- what is CONNECTED in a label volume: 3-D connected-component labelling of labels [dx, dy, dz] on the device, and the
// filters built on it (drop components below a size, keep the largest component of a label).  tests/_components_restate.py states
// all of it in numpy; the outputs are canonical, so the kernels reproduce it exactly whatever the execution order.
//
// Contract.  Cell (i, j, k) has the index g = (i dy + j) dz + k.  A cell is labelled iff labels[g] < C.  Two labelled cells are adjacent
// iff they carry the SAME label and differ by exactly one in one axis (connectivity 6), or by at most one in every axis without being
// the same cell (26); nothing wraps round the box.  Components are the classes of that adjacency.  root[g] = the smallest index of
// the cell's component (-1 for an unlabelled cell), size[g] = the number of its cells (0).
//
//   cc_tile_kernel<CONN>  a workgroup owns CC_TI x CC_TJ x CC_TK cells, stages their labels in LDS and runs union-find on LDS parents
//                         (local indices; the local order is the global one, so the local root is the smallest cell of the piece):
//                         every cell joins its PREDECESSORS, the adjacent cells with a smaller index (3 at connectivity 6, 13 at 26),
//                         where they lie in the tile.  Then parent[g] = the global index of the local root, and size[g] = the number
//                         of cells of the piece at the piece's root, 0 everywhere else.
//   cc_seam_kernel<CONN>  every cell with a predecessor in ANOTHER tile joins it in the global parent array
//   cc_flatten_kernel     root[g] = the root above g, written over the parent (a store replaces a link by the root it leads to, so a
//                         walk that meets it still ends at the same root); a piece's root that is not the component's adds the
//                         piece's count to the component's root: one integer atomic per piece, not per cell
//   cc_size_kernel        size[g] = size[root[g]]
//   cc_largest_kernel     root cells only: best[l] = max over the components of label l of (size << 32 | 0x7fffffff - root) by
//                         atomicMax (the workgroup's LDS table, then one atomic per label), so the largest component wins and,
//                         on equal sizes, the one with the smallest root; the filter runs it in mode "largest" only
//   cc_filter_kernel      every cell: a cell of a label in the mask keeps its label iff size >= min_cells and (mode "largest")
//                         root == best root of its label, else it becomes 255 and its baked words four zeros; removed / kept per
//                         label from ballots and popcounts into the workgroup's LDS table, one flush with integer atomics
//
// Termination of the union-find (cc_find / cc_union, surface.hip's scheme).  parent[x] <= x always: a cell starts as its own parent,
// and the only writes are atomicMin with a smaller index (a hook of the larger root under the smaller, or path halving with an
// ancestor, which is smaller still).  atomicMin only lowers a parent, so a link, once below x, stays below x.  find walks from x to
// parent[x] < x: strictly decreasing indices, at most x steps.  A hook atomicMin(parent[a], b) with b < a that finds a no longer a
// root returns old < a, and the union goes on from (old, b): a strictly smaller index, so it retries at most a times.  No loop waits
// for another lane or workgroup: every loop ends by what the lane itself has read.  The root of a finished tree is the smallest cell
// of the component because a root is only ever hooked under a smaller cell of the same component.
//
// Integers throughout: no floating point, no inline assembly, no scratch (the neighbourhoods are template parameters: every offset is
// an immediate).  Nothing is allocated: root and size are the only workspace.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "grid_volume.h"

namespace {

constexpr int CC_TI = 8, CC_TJ = 8, CC_TK = 32;                       // cells per workgroup (field.COMPONENTS_TILE; powers of two)
constexpr int CC_TILE = CC_TI * CC_TJ * CC_TK;                        // 2048
constexpr int CC_THREADS = CC_TJ * CC_TK;                             // 256: one (j, k) column per thread, CC_TI cells each
constexpr int CC_BLOCK = 256;
constexpr int CC_STRIDE_MAX_BLOCKS = 2048;                            // the grid of the largest and filter passes; beyond it a workgroup strides
constexpr int UNLABELLED = 255;
constexpr uint32_t ROOT_FLIP = 0x7fffffffu;                           // key = size << 32 | ROOT_FLIP - root

struct Dims { int dx, dy, dz; };

// Is (di, dj, dk) the offset to a predecessor: an adjacent cell with a smaller index?
template <int CONN>
__device__ __forceinline__ constexpr bool cc_pred(int di, int dj, int dk) {
    const bool before = di < 0 || (di == 0 && (dj < 0 || (dj == 0 && dk < 0)));
    const int moved = (di != 0) + (dj != 0) + (dk != 0);
    return before && (CONN == 26 || moved == 1);
}

// ---- union-find with parent[x] <= x (the termination argument is the file header's).  SCOPE: workgroup for LDS parents, agent for global.
template <int SCOPE>
__device__ __forceinline__ int32_t cc_find(int32_t* parent, int32_t x) {
    int32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, SCOPE);
    while (p != x) {
        const int32_t g = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, SCOPE);
        if (g != p) atomicMin(&parent[x], g);                           // path halving; monotone, so it can never undo a hook
        x = p;
        p = g;
    }
    return x;
}

template <int SCOPE>
__device__ __forceinline__ void cc_union(int32_t* parent, int32_t a, int32_t b) {
    while (true) {
        a = cc_find<SCOPE>(parent, a);
        b = cc_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }               // hook the larger root a under the smaller b
        const int32_t old = atomicMin(&parent[a], b);
        if (old == a) return;                                           // a was still a root: joined
        a = old;                                                        // somebody hooked a first: join its new tree with b's
    }
}

// ---- the tile pass.  Local index x = (ti CC_TJ + tj) CC_TK + tk: ascending in x is ascending in g.
template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const uint8_t* __restrict__ labels, Dims d, int C, int nbj, int nbk,
                                                              int32_t* __restrict__ parent, int32_t* __restrict__ size) {
    __shared__ uint8_t s_lab[CC_TILE];
    __shared__ int32_t s_par[CC_TILE];
    __shared__ int32_t s_cnt[CC_TILE];
    const int b = blockIdx.x;
    const int i0 = (b / (nbj * nbk)) * CC_TI, j0 = ((b / nbk) % nbj) * CC_TJ, k0 = (b % nbk) * CC_TK;
    const int tj = threadIdx.x / CC_TK, tk = threadIdx.x % CC_TK;
    const int j = j0 + tj, k = k0 + tk;
    const bool column = j < d.dy && k < d.dz;
#pragma unroll
    for (int ti = 0; ti < CC_TI; ++ti) {
        const int x = (ti * CC_TJ + tj) * CC_TK + tk;
        int l = UNLABELLED;                                             // a cell outside the volume, or a label >= C
        if (column && i0 + ti < d.dx) {
            const int v = labels[((int64_t)(i0 + ti) * d.dy + j) * d.dz + k];
            l = v < C ? v : UNLABELLED;
        }
        s_lab[x] = (uint8_t)l;
        s_par[x] = x;
        s_cnt[x] = 0;
    }
    __syncthreads();
#pragma unroll 1
    for (int ti = 0; ti < CC_TI; ++ti) {
        const int x = (ti * CC_TJ + tj) * CC_TK + tk;
        const int l = s_lab[x];
        if (l == UNLABELLED) continue;
#pragma unroll
        for (int di = -1; di <= 0; ++di) {
#pragma unroll
            for (int dj = -1; dj <= 1; ++dj) {
#pragma unroll
                for (int dk = -1; dk <= 1; ++dk) {
                    if (!cc_pred<CONN>(di, dj, dk)) continue;
                    const int a = ti + di, bb = tj + dj, c = tk + dk;
                    if (a < 0 || bb < 0 || bb >= CC_TJ || c < 0 || c >= CC_TK) continue;   // another tile's cell: the seam pass
                    const int y = x + (di * CC_TJ + dj) * CC_TK + dk;
                    if (s_lab[y] == l) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, x, y);
                }
            }
        }
    }
    __syncthreads();
    int32_t r[CC_TI];
#pragma unroll
    for (int ti = 0; ti < CC_TI; ++ti) {
        int32_t x = (ti * CC_TJ + tj) * CC_TK + tk;
        r[ti] = -1;
        if (s_lab[x] == UNLABELLED) continue;
        for (int32_t p = s_par[x]; p != x; p = s_par[x]) x = p;       // the links are final: plain loads
        r[ti] = x;
        atomicAdd(&s_cnt[x], 1);
    }
    __syncthreads();
    if (!column) return;
#pragma unroll
    for (int ti = 0; ti < CC_TI; ++ti) {
        if (i0 + ti >= d.dx) break;
        const int x = (ti * CC_TJ + tj) * CC_TK + tk;
        const int64_t g = ((int64_t)(i0 + ti) * d.dy + j) * d.dz + k;
        int32_t p = -1, n = 0;
        if (r[ti] >= 0) {
            const int ra = r[ti] / (CC_TJ * CC_TK), rb = (r[ti] / CC_TK) % CC_TJ, rc = r[ti] % CC_TK;
            p = (int32_t)(((int64_t)(i0 + ra) * d.dy + (j0 + rb)) * d.dz + (k0 + rc));
            n = r[ti] == x ? s_cnt[x] : 0;
        }
        parent[g] = p;
        size[g] = n;
    }
}

// ---- the seam pass: one cell per lane; a cell joins its predecessors that lie in the volume but not in its tile
template <int CONN>
__global__ __launch_bounds__(CC_BLOCK) void cc_seam_kernel(const uint8_t* __restrict__ labels, Dims d, int C, int32_t* parent) {
    const int64_t n = (int64_t)d.dx * d.dy * d.dz;
    const int64_t g = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (g >= n) return;
    const int k = (int)(g % d.dz), j = (int)((g / d.dz) % d.dy), i = (int)(g / ((int64_t)d.dz * d.dy));
    const int a = i % CC_TI, b = j % CC_TJ, c = k % CC_TK;
    // (an offset leaves the tile only from its faces)
    if (a != 0 && b != 0 && c != 0 && (CONN == 6 || (b != CC_TJ - 1 && c != CC_TK - 1))) return;
    const int l = labels[g];
    if (l >= C) return;
#pragma unroll
    for (int di = -1; di <= 0; ++di) {
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) {
#pragma unroll
            for (int dk = -1; dk <= 1; ++dk) {
                if (!cc_pred<CONN>(di, dj, dk)) continue;
                const int ii = i + di, jj = j + dj, kk = k + dk;
                if (ii < 0 || jj < 0 || jj >= d.dy || kk < 0 || kk >= d.dz) continue;        // no wrap-around at the box
                const int ta = a + di, tb = b + dj, tc = c + dk;
                if (ta >= 0 && tb >= 0 && tb < CC_TJ && tc >= 0 && tc < CC_TK) continue;     // the tile pass joined these
                const int64_t h = ((int64_t)ii * d.dy + jj) * d.dz + kk;
                if (labels[h] == l) cc_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int32_t)g, (int32_t)h);
            }
        }
    }
}

// ---- flatten: root over parent.  The only concurrent writes replace parent[x] by the root above x, so a walk through x ends where it
// would have ended; the words are read and written whole (relaxed atomics).  size[x] of a piece's root x is read by its own lane only,
// and atomics go to component roots only, which add nothing themselves.
__global__ __launch_bounds__(CC_BLOCK) void cc_flatten_kernel(int64_t n, int32_t* root, int32_t* size) {
    const int64_t g = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (g >= n) return;
    int32_t x = (int32_t)g;
    int32_t p = __hip_atomic_load(&root[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p < 0 || p == x) return;                                        // unlabelled (-1 stands), or a root
    while (p != x) {
        x = p;
        p = __hip_atomic_load(&root[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __hip_atomic_store(&root[g], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t piece = size[g];
    if (piece > 0) atomicAdd(&size[x], piece);
}

__global__ __launch_bounds__(CC_BLOCK) void cc_size_kernel(int64_t n, const int32_t* __restrict__ root, int32_t* size) {
    const int64_t g = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (g >= n) return;
    const int32_t r = root[g];
    if (r >= 0 && r != g) size[g] = size[r];                            // (roots are only read here)
}

// ---- the largest component of every label
__global__ void cc_best_init_kernel(int C, unsigned long long* __restrict__ best) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l < C) best[l] = 0ull;                                          // no component: size 0
}

// (noise has a root in every few cells and few labels: the maximum is taken in the workgroup's LDS table first, then once per label)
__global__ __launch_bounds__(CC_BLOCK) void cc_largest_kernel(const uint8_t* __restrict__ labels, uint32_t total, int C,
                                                               const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                               unsigned long long* best) {
    __shared__ unsigned long long s_best[DMNERF_MAX_LOGITS];
    for (int l = threadIdx.x; l < C; l += CC_BLOCK) s_best[l] = 0ull;
    __syncthreads();
    for (uint32_t g0 = blockIdx.x * CC_BLOCK; g0 < total; g0 += gridDim.x * CC_BLOCK) {
        const uint32_t g = g0 + threadIdx.x;
        if (g >= total || root[g] != (int32_t)g) continue;
        const int l = labels[g];
        if (l < C) atomicMax(&s_best[l], ((unsigned long long)(uint32_t)size[g] << 32) | (unsigned long long)(ROOT_FLIP - g));
    }
    __syncthreads();
    for (int l = threadIdx.x; l < C; l += CC_BLOCK) {
        if (s_best[l]) atomicMax(&best[l], s_best[l]);
    }
}

// ---- the filter.  (the trip count is the workgroup's: every lane stays in the loop, so the ballots see whole waves; total < 2^31
// and the grid's stride is at most 2^19 cells: 32-bit indices do not wrap, and a workgroup counts fewer than 2^32 cells)
template <bool BAKED>
__global__ __launch_bounds__(CC_BLOCK) void cc_filter_kernel(const uint8_t* __restrict__ labels, const uint4* __restrict__ cells, uint32_t total,
                                                              int C, LabelMask128 mask, const int32_t* __restrict__ root,
                                                              const int32_t* __restrict__ size, int min_cells, int largest,
                                                              const unsigned long long* __restrict__ best, uint8_t* __restrict__ out_labels,
                                                              uint4* __restrict__ out_cells, unsigned long long* __restrict__ removed,
                                                              unsigned long long* __restrict__ kept) {
    __shared__ unsigned int s_removed[DMNERF_MAX_LOGITS], s_kept[DMNERF_MAX_LOGITS];
    for (int l = threadIdx.x; l < C; l += CC_BLOCK) { s_removed[l] = 0; s_kept[l] = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint32_t g0 = blockIdx.x * CC_BLOCK; g0 < total; g0 += gridDim.x * CC_BLOCK) {
        const uint32_t g = g0 + threadIdx.x;
        const bool in = g < total;
        const int l = in ? labels[g] : UNLABELLED;
        const bool counted = l < C;
        bool keep = true;
        if (counted && mask_bit(mask, (uint32_t)l)) {
            keep = size[g] >= min_cells;
            if (keep && largest) keep = (uint32_t)root[g] == ROOT_FLIP - (uint32_t)(best[l] & 0xffffffffull);
        }
        if (in) {
            out_labels[g] = (uint8_t)(keep ? l : UNLABELLED);
            if (BAKED) {
                uint4 v = cells[g];                                     // (the words travel as integers: a NaN keeps its payload)
                if (!keep) v = make_uint4(0u, 0u, 0u, 0u);
                out_cells[g] = v;
            }
        }
        const unsigned long long b_kept = __ballot(counted && keep), b_removed = __ballot(counted && !keep);
        unsigned long long todo = b_kept | b_removed;
        while (todo != 0) {                                             // one turn per label of the wave: wave-uniform, at most 64
            const int l0 = __shfl(l, __ffsll((long long)todo) - 1);
            const unsigned long long m = __ballot(l == l0);
            if (lane == 0) {
                const int nk = __popcll(m & b_kept), nr = __popcll(m & b_removed);
                if (nk) atomicAdd(&s_kept[l0], (unsigned int)nk);
                if (nr) atomicAdd(&s_removed[l0], (unsigned int)nr);
            }
            todo &= ~m;
        }
    }
    __syncthreads();
    for (int l = threadIdx.x; l < C; l += CC_BLOCK) {
        if (s_removed[l]) atomicAdd(&removed[l], (unsigned long long)s_removed[l]);
        if (s_kept[l]) atomicAdd(&kept[l], (unsigned long long)s_kept[l]);
    }
}

__global__ void cc_counts_init_kernel(int C, unsigned long long* __restrict__ removed, unsigned long long* __restrict__ kept) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l < C) { removed[l] = 0ull; kept[l] = 0ull; }
}

inline unsigned cc_blocks(int64_t n) { return (unsigned)((n + CC_BLOCK - 1) / CC_BLOCK); }
inline unsigned cc_stride_blocks(int64_t n) { return cc_blocks(n) < (unsigned)CC_STRIDE_MAX_BLOCKS ? cc_blocks(n) : (unsigned)CC_STRIDE_MAX_BLOCKS; }

// What the three entries check of the volume, in one order: dims, cells, C.
int cc_check_volume(const char* who, int dx, int dy, int dz, int C, int64_t* total) {
    const int dims[3] = {dx, dy, dz};
    if (int rc = dmn_grid_dims(who, dims)) return rc;
    if (int rc = dmn_grid_cells(who, dims, total)) return rc;
    return dmn_check_labels(who, C);
}

void cc_launch_largest(const uint8_t* d_labels, int64_t total, int C, const int32_t* d_root, const int32_t* d_size, int64_t* d_best,
                       hipStream_t st) {
    unsigned long long* best = reinterpret_cast<unsigned long long*>(d_best);
    hipLaunchKernelGGL(cc_best_init_kernel, dim3(1), dim3(DMNERF_MAX_LOGITS), 0, st, C, best);
    hipLaunchKernelGGL(cc_largest_kernel, dim3(cc_stride_blocks(total)), dim3(CC_BLOCK), 0, st, d_labels, (uint32_t)total, C, d_root, d_size, best);
}

}  // namespace

extern "C" int32_t dmnerf_label_components(const uint8_t* d_labels, int dx, int dy, int dz, int C, int connectivity, int32_t* d_root,
                                       int32_t* d_size, void* stream) {
    int64_t total;
    if (int rc = cc_check_volume("label_components", dx, dy, dz, C, &total)) return rc;
    if (connectivity != 6 && connectivity != 26) return dmn_fail(DMNERF_E_ARG, "label_components: connectivity %d is neither 6 nor 26", connectivity);
    if (!d_labels || !d_root || !d_size) return dmn_fail(DMNERF_E_ARG, "label_components: null pointer");
    const Dims d = {dx, dy, dz};
    const int nbi = (dx + CC_TI - 1) / CC_TI, nbj = (dy + CC_TJ - 1) / CC_TJ, nbk = (dz + CC_TK - 1) / CC_TK;
    const unsigned tiles = (unsigned)((int64_t)nbi * nbj * nbk);        // (< 2^31: every tile holds a cell)
    hipStream_t st = (hipStream_t)stream;
    if (connectivity == 6) {
        hipLaunchKernelGGL(cc_tile_kernel<6>, dim3(tiles), dim3(CC_THREADS), 0, st, d_labels, d, C, nbj, nbk, d_root, d_size);
        hipLaunchKernelGGL(cc_seam_kernel<6>, dim3(cc_blocks(total)), dim3(CC_BLOCK), 0, st, d_labels, d, C, d_root);
    } else {
        hipLaunchKernelGGL(cc_tile_kernel<26>, dim3(tiles), dim3(CC_THREADS), 0, st, d_labels, d, C, nbj, nbk, d_root, d_size);
        hipLaunchKernelGGL(cc_seam_kernel<26>, dim3(cc_blocks(total)), dim3(CC_BLOCK), 0, st, d_labels, d, C, d_root);
    }
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_blocks(total)), dim3(CC_BLOCK), 0, st, total, d_root, d_size);
    hipLaunchKernelGGL(cc_size_kernel, dim3(cc_blocks(total)), dim3(CC_BLOCK), 0, st, total, d_root, d_size);
    return dmn_check_launch("label_components");
}

extern "C" int32_t dmnerf_label_components_largest(const uint8_t* d_labels, int dx, int dy, int dz, int C, const int32_t* d_root,
                                               const int32_t* d_size, int64_t* d_best, void* stream) {
    int64_t total;
    if (int rc = cc_check_volume("label_components_largest", dx, dy, dz, C, &total)) return rc;
    if (!d_labels || !d_root || !d_size || !d_best) return dmn_fail(DMNERF_E_ARG, "label_components_largest: null pointer");
    cc_launch_largest(d_labels, total, C, d_root, d_size, d_best, (hipStream_t)stream);
    return dmn_check_launch("label_components_largest");
}

extern "C" int32_t dmnerf_label_components_filter(const uint8_t* d_labels, const float* d_cells, int dx, int dy, int dz, int C,
                                              const uint32_t mask[4], const int32_t* d_root, const int32_t* d_size, int min_cells,
                                              int mode, int64_t* d_best, uint8_t* d_out_labels, float* d_out_cells, int64_t* d_removed,
                                              int64_t* d_kept, void* stream) {
    const char* who = "label_components_filter";
    int64_t total;
    if (int rc = cc_check_volume(who, dx, dy, dz, C, &total)) return rc;
    if (min_cells < 1) return dmn_fail(DMNERF_E_ARG, "%s: min_cells %d must be >= 1", who, min_cells);
    if (mode != DMNERF_COMPONENTS_KEEP_ALL && mode != DMNERF_COMPONENTS_KEEP_LARGEST)
        return dmn_fail(DMNERF_E_ARG, "%s: mode %d (0 all, 1 largest)", who, mode);
    if (!mask) return dmn_fail(DMNERF_E_ARG, "%s: null mask", who);
    if (!d_labels || !d_root || !d_size || !d_best || !d_out_labels || !d_removed || !d_kept) return dmn_fail(DMNERF_E_ARG, "%s: null pointer", who);
    if ((d_cells == nullptr) != (d_out_cells == nullptr)) return dmn_fail(DMNERF_E_ARG, "%s: d_cells and d_out_cells go together", who);
    if (((uintptr_t)d_cells | (uintptr_t)d_out_cells) & 15) return dmn_fail(DMNERF_E_ARG, "%s: cells must be 16-byte aligned", who);
    LabelMask128 m;
    for (int q = 0; q < 4; ++q) m.w[q] = mask[q];
    hipStream_t st = (hipStream_t)stream;
    const int largest = mode == DMNERF_COMPONENTS_KEEP_LARGEST;
    if (largest) cc_launch_largest(d_labels, total, C, d_root, d_size, d_best, st);   // (mode "all" never reads d_best)
    unsigned long long* removed = reinterpret_cast<unsigned long long*>(d_removed);
    unsigned long long* kept = reinterpret_cast<unsigned long long*>(d_kept);
    const unsigned long long* best = reinterpret_cast<const unsigned long long*>(d_best);
    hipLaunchKernelGGL(cc_counts_init_kernel, dim3(1), dim3(DMNERF_MAX_LOGITS), 0, st, C, removed, kept);
    const unsigned nb = cc_stride_blocks(total);
    if (d_cells) {
        hipLaunchKernelGGL(cc_filter_kernel<true>, dim3(nb), dim3(CC_BLOCK), 0, st, d_labels, reinterpret_cast<const uint4*>(d_cells),
                           (uint32_t)total, C, m, d_root, d_size, min_cells, largest, best, d_out_labels, reinterpret_cast<uint4*>(d_out_cells),
                           removed, kept);
    } else {
        hipLaunchKernelGGL(cc_filter_kernel<false>, dim3(nb), dim3(CC_BLOCK), 0, st, d_labels, (const uint4*)nullptr, (uint32_t)total, C, m,
                           d_root, d_size, min_cells, largest, best, d_out_labels, (uint4*)nullptr, removed, kept);
    }
    return dmn_check_launch(who);
}
