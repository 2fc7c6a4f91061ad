// surface.hip -- the iso-surface of the occupancy grid on the device: the middle of the reference's mesh_main
// (tools/mesh_generator.py:68-104) between dmnerf_occupancy_slab and dmnerf_ins_label_conf -- marching cubes at a level, the vertex
// normals of trimesh_to_open3d -> compute_vertex_normals(), clean_mesh (cluster_connected_triangles + remove_triangles_by_mask) and
// remove_unreferenced_vertices.  tests/_surface_restate.py states every stage in numpy; the kernels reproduce it bit for bit.
//
// Conventions: occ [dx, dy, dz] f32 row-major, linear index p = (i dy + j) dz + k.  A point is inside iff v > level (NaN: outside).
// Corner c of the cell at p sets bit c of the case; MC_CORNER / MC_EDGE (mc_tables.h) give the corner offsets and, per cell edge, the grid point
// that owns it (its lower end) and its axis.  Vertices are ordered by (owning point, axis), triangles by (cell, position in the
// table row): both orders come from inclusive prefix sums of the per-point counts (the caller scans; the counts are bytes).
//
//   sf_count_kernel     a workgroup owns SF_TI x SF_TJ x SF_TK points and stages them with a one-point halo on the upper sides
//                       through LDS, so a value is read once per tile (and the halo mostly from L2); per point the number of
//                       crossing owned edges (0..3) and, where the point is the lowest corner of a cell, its triangle count (0..5)
//   sf_vertices_kernel  per point with a nonzero count: t = (level - a) / (b - a), position i + t on the axis, all in f32
//   sf_faces_kernel     per cell with triangles: the id of the vertex on a cell edge = the owner's scan - its count + the rank of
//                       the axis among the owner's crossing edges, recomputed from the grid (no index map is kept)
//   sf_normals_kernel   per vertex: the f32 sum of (p1 - p0) x (p2 - p0) over its triangles in ascending triangle index -- the
//                       triangles of the <= 4 cells round its grid edge in ascending cell index and table order -- read from the
//                       stably sorted (vertex, corner slot) incidence list; then normalised; a zero sum stays zero.  No atomics.
//   sf_link / sf_flatten  union-find over the triangles: two triangles that are neighbours in the sorted list of packed
//                       undirected edge keys are joined by hooking the larger root under the smaller with atomicMin, so a parent
//                       is never above its child and the root of a finished tree is the smallest triangle of the cluster, whatever
//                       the order; cluster sizes are integer atomic counts
//   sf_mark / sf_compact  clean_mesh's mask and the two order-preserving compactions with re-indexing
// Memory-bound throughout: no MFMA, no inline assembly, no floating-point atomic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "mc_tables.h"

namespace {

constexpr int SF_TI = 8, SF_TJ = 8, SF_TK = 32;                       // points per workgroup (the test shapes use T = SF_TK)
constexpr int SF_HI = SF_TI + 1, SF_HJ = SF_TJ + 1, SF_HK = SF_TK + 1;
constexpr int SF_THREADS = SF_TJ * SF_TK;                             // 256: one (j, k) column per thread, SF_TI points each
constexpr int SF_BLOCK = 256;

struct Dims { int dx, dy, dz; };

__global__ __launch_bounds__(SF_THREADS) void sf_count_kernel(const float* __restrict__ occ, Dims d, float level, int nbj, int nbk,
                                                               uint8_t* __restrict__ vcnt, uint8_t* __restrict__ tcnt) {
    __shared__ float s[SF_HI * SF_HJ * SF_HK];
    const int b = blockIdx.x;
    const int i0 = (b / (nbj * nbk)) * SF_TI, j0 = ((b / nbk) % nbj) * SF_TJ, k0 = (b % nbk) * SF_TK;
    for (int x = threadIdx.x; x < SF_HI * SF_HJ * SF_HK; x += SF_THREADS) {
        const int c = x % SF_HK, bb = (x / SF_HK) % SF_HJ, a = x / (SF_HK * SF_HJ);
        const int i = i0 + a, j = j0 + bb, k = k0 + c;
        float v = 0.f;                                                  // outside the grid: never used (the edge does not exist)
        if (i < d.dx && j < d.dy && k < d.dz) v = occ[((int64_t)i * d.dy + j) * d.dz + k];
        s[x] = v;
    }
    __syncthreads();
    const int tj = threadIdx.x / SF_TK, tk = threadIdx.x % SF_TK;
    const int j = j0 + tj, k = k0 + tk;
    if (j >= d.dy || k >= d.dz) return;
    const bool hj = j + 1 < d.dy, hk = k + 1 < d.dz;
#pragma unroll
    for (int ti = 0; ti < SF_TI; ++ti) {
        const int i = i0 + ti;
        if (i >= d.dx) break;
        const bool hi = i + 1 < d.dx;
        const float* c = s + (ti * SF_HJ + tj) * SF_HK + tk;
        bool in[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) in[q] = c[(MC_CORNER[q][0] * SF_HJ + MC_CORNER[q][1]) * SF_HK + MC_CORNER[q][2]] > level;
        const int nv = (int)(hi && in[0] != in[4]) + (int)(hj && in[0] != in[3]) + (int)(hk && in[0] != in[1]);
        int nt = 0;
        if (hi && hj && hk) {
            int mc_case = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) mc_case |= (int)in[q] << q;
            nt = mc_triangles(mc_case);
        }
        const int64_t p = ((int64_t)i * d.dy + j) * d.dz + k;
        vcnt[p] = (uint8_t)nv;
        tcnt[p] = (uint8_t)nt;
    }
}

__global__ __launch_bounds__(SF_BLOCK) void sf_vertices_kernel(const float* __restrict__ occ, Dims d, float level,
                                                                const uint8_t* __restrict__ vcnt, const int64_t* __restrict__ vscan,
                                                                int64_t V, float* __restrict__ vertices) {
    const int64_t n = (int64_t)d.dx * d.dy * d.dz;
    const int64_t p = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int nv = vcnt[p];
    if (nv == 0) return;
    const int k = (int)(p % d.dz), j = (int)((p / d.dz) % d.dy), i = (int)(p / ((int64_t)d.dz * d.dy));
    const int64_t stride[3] = {(int64_t)d.dy * d.dz, d.dz, 1};
    const bool has[3] = {i + 1 < d.dx, j + 1 < d.dy, k + 1 < d.dz};
    const float a = occ[p];
    int64_t o = vscan[p] - nv;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!has[ax]) continue;
        const float bv = occ[p + stride[ax]];
        if ((a > level) == (bv > level)) continue;
        if (o < 0 || o >= V) return;                                    // inconsistent scans: write nothing out of bounds
        const float t = (level - a) / (bv - a);
        float pos[3] = {(float)i, (float)j, (float)k};
        pos[ax] = pos[ax] + t;
        vertices[3 * o + 0] = pos[0];
        vertices[3 * o + 1] = pos[1];
        vertices[3 * o + 2] = pos[2];
        ++o;
    }
}

// Does the edge from q = (i, j, k) along `ax` exist and cross?
__device__ __forceinline__ bool sf_crosses(const float* __restrict__ occ, Dims d, float level, int i, int j, int k, int64_t q, int ax) {
    if (ax == 0) return i + 1 < d.dx && (occ[q] > level) != (occ[q + (int64_t)d.dy * d.dz] > level);
    if (ax == 1) return j + 1 < d.dy && (occ[q] > level) != (occ[q + d.dz] > level);
    return k + 1 < d.dz && (occ[q] > level) != (occ[q + 1] > level);
}

__global__ __launch_bounds__(SF_BLOCK) void sf_faces_kernel(const float* __restrict__ occ, Dims d, float level,
                                                             const uint8_t* __restrict__ vcnt, const uint8_t* __restrict__ tcnt,
                                                             const int64_t* __restrict__ vscan, const int64_t* __restrict__ tscan,
                                                             int64_t V, int64_t F, int32_t* __restrict__ faces) {
    const int64_t n = (int64_t)d.dx * d.dy * d.dz;
    const int64_t p = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int nt = tcnt[p];
    if (nt == 0) return;
    const int k = (int)(p % d.dz), j = (int)((p / d.dz) % d.dy), i = (int)(p / ((int64_t)d.dz * d.dy));
    if (i + 1 >= d.dx || j + 1 >= d.dy || k + 1 >= d.dz) return;       // not a cell (the count kernel wrote 0 here)
    int mc_case = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int64_t c = ((int64_t)(i + MC_CORNER[q][0]) * d.dy + (j + MC_CORNER[q][1])) * d.dz + (k + MC_CORNER[q][2]);
        mc_case |= (int)(occ[c] > level) << q;
    }
    const int64_t first = tscan[p] - nt;
    if (first < 0 || first + nt > F || mc_triangles(mc_case) != nt) return;
    for (int s = 0; s < 3 * nt; ++s) {
        const int e = MC_TRI[mc_case][s];
        const int qi = i + MC_EDGE[e][0], qj = j + MC_EDGE[e][1], qk = k + MC_EDGE[e][2], ax = MC_EDGE[e][3];
        const int64_t q = ((int64_t)qi * d.dy + qj) * d.dz + qk;
        int rank = 0;
        if (ax >= 1) rank += (int)sf_crosses(occ, d, level, qi, qj, qk, q, 0);
        if (ax >= 2) rank += (int)sf_crosses(occ, d, level, qi, qj, qk, q, 1);
        const int64_t id = vscan[q] - vcnt[q] + rank;
        faces[3 * first + s] = (int32_t)(id >= 0 && id < V ? id : 0);
    }
}

__global__ __launch_bounds__(SF_BLOCK) void sf_normals_kernel(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ faces,
                                                               int64_t F, const int32_t* __restrict__ inc_vertex,
                                                               const int64_t* __restrict__ inc_slot, float* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (v >= V) return;
    int64_t lo = 0, hi = 3 * F;                                         // first incidence of vertex v in the sorted list
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (inc_vertex[mid] < v) lo = mid + 1; else hi = mid;
    }
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int64_t x = lo; x < 3 * F && inc_vertex[x] == v; ++x) {
        const int64_t f = inc_slot[x] / 3;
        if (f < 0 || f >= F) continue;
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) continue;
        const float ux = vertices[3 * b] - vertices[3 * a], uy = vertices[3 * b + 1] - vertices[3 * a + 1], uz = vertices[3 * b + 2] - vertices[3 * a + 2];
        const float wx = vertices[3 * c] - vertices[3 * a], wy = vertices[3 * c + 1] - vertices[3 * a + 1], wz = vertices[3 * c + 2] - vertices[3 * a + 2];
        sx = sx + (uy * wz - uz * wy);
        sy = sy + (uz * wx - ux * wz);
        sz = sz + (ux * wy - uy * wx);
    }
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
    const bool ok = len > 0.f;
    normals[3 * v + 0] = ok ? sx / len : 0.f;
    normals[3 * v + 1] = ok ? sy / len : 0.f;
    normals[3 * v + 2] = ok ? sz / len : 0.f;
}

// ---- clusters: union-find with parent[x] <= x
__device__ __forceinline__ int32_t sf_find(int32_t* parent, int32_t x) {
    int32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        const int32_t g = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g != p) atomicMin(&parent[x], g);                           // path halving; monotone, so it can never undo a hook
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void sf_union(int32_t* parent, int32_t a, int32_t b) {
    while (true) {
        a = sf_find(parent, a);
        b = sf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }               // hook the larger root a under the smaller b
        const int32_t old = atomicMin(&parent[a], b);
        if (old == a) return;                                           // a was still a root: joined
        a = old;                                                        // somebody hooked a first: join its new tree with b's
    }
}

__global__ __launch_bounds__(SF_BLOCK) void sf_link_kernel(const int64_t* __restrict__ key, const int64_t* __restrict__ slot, int64_t F,
                                                            int32_t* parent) {
    const int64_t x = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (x + 1 >= 3 * F || key[x] != key[x + 1]) return;
    const int64_t a = slot[x] / 3, b = slot[x + 1] / 3;
    if (a < 0 || a >= F || b < 0 || b >= F || a == b) return;
    sf_union(parent, (int32_t)a, (int32_t)b);
}

__global__ __launch_bounds__(SF_BLOCK) void sf_flatten_kernel(int64_t F, const int32_t* __restrict__ parent, int32_t* __restrict__ rep,
                                                               int32_t* __restrict__ count) {
    const int64_t f = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (f >= F) return;
    int32_t x = (int32_t)f;
    for (int32_t p = parent[x]; p != x; p = parent[x]) x = p;          // the links are final: plain loads
    rep[f] = x;
    atomicAdd(&count[x], 1);
}

__global__ __launch_bounds__(SF_BLOCK) void sf_mark_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ rep,
                                                            const int32_t* __restrict__ count, int min_triangles,
                                                            const int64_t* __restrict__ single, uint8_t* __restrict__ keep,
                                                            uint8_t* __restrict__ used) {
    const int64_t f = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int32_t r = rep[f];
    bool k = false;
    if (r >= 0 && r < F) k = single ? r == *single : count[r] >= min_triangles;
    keep[f] = (uint8_t)k;
    if (!k) return;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int64_t v = faces[3 * f + s];
        if (v >= 0 && v < V) used[v] = 1;                               // every writer stores the same value
    }
}

__global__ __launch_bounds__(SF_BLOCK) void sf_compact_faces_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V,
                                                                     const uint8_t* __restrict__ keep, const int32_t* __restrict__ fscan,
                                                                     const int32_t* __restrict__ vscan, int64_t Fk, int32_t* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (f >= F || !keep[f]) return;
    const int64_t o = (int64_t)fscan[f] - 1;
    if (o < 0 || o >= Fk) return;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int64_t v = faces[3 * f + s];
        out[3 * o + s] = v >= 0 && v < V ? vscan[v] - 1 : 0;
    }
}

__global__ __launch_bounds__(SF_BLOCK) void sf_compact_vertices_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                        int64_t V, const uint8_t* __restrict__ used,
                                                                        const int32_t* __restrict__ vscan, int64_t Vk, float* __restrict__ out_v,
                                                                        float* __restrict__ out_n, int64_t* __restrict__ out_kept) {
    const int64_t v = (int64_t)blockIdx.x * SF_BLOCK + threadIdx.x;
    if (v >= V || !used[v]) return;
    const int64_t o = (int64_t)vscan[v] - 1;
    if (o < 0 || o >= Vk) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out_v[3 * o + c] = vertices[3 * v + c];
        out_n[3 * o + c] = normals[3 * v + c];
    }
    out_kept[o] = v;
}

const char* sf_dims(int dx, int dy, int dz) {
    if (dx < 2 || dy < 2 || dz < 2) return "every dimension must be >= 2";
    if ((int64_t)dx * dy * dz >= ((int64_t)1 << 31)) return "dx * dy * dz must be < 2^31";
    return nullptr;
}

inline unsigned sf_blocks(int64_t n) { return (unsigned)((n + SF_BLOCK - 1) / SF_BLOCK); }
constexpr int64_t SF_MAX = ((int64_t)1 << 31) - 1;                      // vertex and triangle ids are int32

}  // namespace

extern "C" int dmnerf_surface_count(const float* d_occ, int dx, int dy, int dz, float level, uint8_t* d_vcount, uint8_t* d_tcount,
                                    void* stream) {
    if (const char* why = sf_dims(dx, dy, dz)) return dmn_fail(DMNERF_E_ARG, "surface_count: bad grid %d x %d x %d (%s)", dx, dy, dz, why);
    if (!d_occ || !d_vcount || !d_tcount) return dmn_fail(DMNERF_E_ARG, "surface_count: null pointer");
    const int nbi = (dx + SF_TI - 1) / SF_TI, nbj = (dy + SF_TJ - 1) / SF_TJ, nbk = (dz + SF_TK - 1) / SF_TK;
    const int64_t blocks = (int64_t)nbi * nbj * nbk;                    // < 2^31 / 2048 + the ragged tiles
    if (blocks >= ((int64_t)1 << 31)) return dmn_fail(DMNERF_E_ARG, "surface_count: too many tiles");
    hipLaunchKernelGGL(sf_count_kernel, dim3((unsigned)blocks), dim3(SF_THREADS), 0, (hipStream_t)stream, d_occ, Dims{dx, dy, dz}, level,
                       nbj, nbk, d_vcount, d_tcount);
    return dmn_check_launch("surface_count");
}

extern "C" int dmnerf_surface_emit(const float* d_occ, int dx, int dy, int dz, float level, const uint8_t* d_vcount,
                                   const uint8_t* d_tcount, const int64_t* d_vscan, const int64_t* d_tscan, int64_t V, int64_t F,
                                   float* d_vertices, int32_t* d_faces, void* stream) {
    if (const char* why = sf_dims(dx, dy, dz)) return dmn_fail(DMNERF_E_ARG, "surface_emit: bad grid %d x %d x %d (%s)", dx, dy, dz, why);
    if (V < 0 || F < 0 || V > SF_MAX || F > SF_MAX)
        return dmn_fail(DMNERF_E_ARG, "surface_emit: V=%lld F=%lld do not fit int32 ids", (long long)V, (long long)F);
    if (!d_occ || !d_vcount || !d_tcount || !d_vscan || !d_tscan || (V && !d_vertices) || (F && !d_faces))
        return dmn_fail(DMNERF_E_ARG, "surface_emit: null pointer");
    const int64_t n = (int64_t)dx * dy * dz;
    if (V) {
        hipLaunchKernelGGL(sf_vertices_kernel, dim3(sf_blocks(n)), dim3(SF_BLOCK), 0, (hipStream_t)stream, d_occ, Dims{dx, dy, dz}, level,
                           d_vcount, d_vscan, V, d_vertices);
        if (int rc = dmn_check_launch("surface_emit: vertices")) return rc;
    }
    if (F) {
        hipLaunchKernelGGL(sf_faces_kernel, dim3(sf_blocks(n)), dim3(SF_BLOCK), 0, (hipStream_t)stream, d_occ, Dims{dx, dy, dz}, level,
                           d_vcount, d_tcount, d_vscan, d_tscan, V, F, d_faces);
        if (int rc = dmn_check_launch("surface_emit: faces")) return rc;
    }
    return DMNERF_OK;
}

extern "C" int dmnerf_surface_normals(const float* d_vertices, int64_t V, const int32_t* d_faces, int64_t F, const int32_t* d_inc_vertex,
                                      const int64_t* d_inc_slot, float* d_normals, void* stream) {
    if (V < 0 || F < 0 || V > SF_MAX || F > SF_MAX) return dmn_fail(DMNERF_E_ARG, "surface_normals: bad V=%lld F=%lld", (long long)V, (long long)F);
    if (V == 0) return DMNERF_OK;
    if (!d_vertices || !d_normals || (F && (!d_faces || !d_inc_vertex || !d_inc_slot)))
        return dmn_fail(DMNERF_E_ARG, "surface_normals: null pointer");
    hipLaunchKernelGGL(sf_normals_kernel, dim3(sf_blocks(V)), dim3(SF_BLOCK), 0, (hipStream_t)stream, d_vertices, V, d_faces, F,
                       d_inc_vertex, d_inc_slot, d_normals);
    return dmn_check_launch("surface_normals");
}

extern "C" int dmnerf_surface_clusters(const int64_t* d_edge_key, const int64_t* d_edge_slot, int64_t F, int32_t* d_parent, int32_t* d_rep,
                                       int32_t* d_count, void* stream) {
    if (F < 0 || F > SF_MAX) return dmn_fail(DMNERF_E_ARG, "surface_clusters: bad F=%lld", (long long)F);
    if (F == 0) return DMNERF_OK;
    if (!d_edge_key || !d_edge_slot || !d_parent || !d_rep || !d_count) return dmn_fail(DMNERF_E_ARG, "surface_clusters: null pointer");
    hipLaunchKernelGGL(sf_link_kernel, dim3(sf_blocks(3 * F)), dim3(SF_BLOCK), 0, (hipStream_t)stream, d_edge_key, d_edge_slot, F, d_parent);
    if (int rc = dmn_check_launch("surface_clusters: link")) return rc;
    hipLaunchKernelGGL(sf_flatten_kernel, dim3(sf_blocks(F)), dim3(SF_BLOCK), 0, (hipStream_t)stream, F, (const int32_t*)d_parent, d_rep,
                       d_count);
    return dmn_check_launch("surface_clusters: flatten");
}

extern "C" int dmnerf_surface_clean_mark(const int32_t* d_faces, int64_t F, int64_t V, const int32_t* d_rep, const int32_t* d_count,
                                         int min_triangles, const int64_t* d_single, uint8_t* d_keep, uint8_t* d_used, void* stream) {
    if (V < 0 || F < 0 || V > SF_MAX || F > SF_MAX) return dmn_fail(DMNERF_E_ARG, "surface_clean_mark: bad V=%lld F=%lld", (long long)V, (long long)F);
    if (F == 0) return DMNERF_OK;
    if (!d_faces || !d_rep || !d_count || !d_keep || !d_used) return dmn_fail(DMNERF_E_ARG, "surface_clean_mark: null pointer");
    hipLaunchKernelGGL(sf_mark_kernel, dim3(sf_blocks(F)), dim3(SF_BLOCK), 0, (hipStream_t)stream, d_faces, F, V, d_rep, d_count,
                       min_triangles, d_single, d_keep, d_used);
    return dmn_check_launch("surface_clean_mark");
}

extern "C" int dmnerf_surface_clean_compact(const float* d_vertices, const float* d_normals, const int32_t* d_faces, int64_t V, int64_t F,
                                            const uint8_t* d_keep, const uint8_t* d_used, const int32_t* d_fscan, const int32_t* d_vscan,
                                            int64_t Vk, int64_t Fk, float* d_out_vertices, float* d_out_normals, int32_t* d_out_faces,
                                            int64_t* d_out_kept, void* stream) {
    if (V < 0 || F < 0 || V > SF_MAX || F > SF_MAX || Vk < 0 || Vk > V || Fk < 0 || Fk > F)
        return dmn_fail(DMNERF_E_ARG, "surface_clean_compact: bad V=%lld F=%lld Vk=%lld Fk=%lld", (long long)V, (long long)F, (long long)Vk,
                        (long long)Fk);
    if (Fk && (!d_faces || !d_keep || !d_fscan || !d_vscan || !d_out_faces)) return dmn_fail(DMNERF_E_ARG, "surface_clean_compact: null pointer");
    if (Vk && (!d_vertices || !d_normals || !d_used || !d_vscan || !d_out_vertices || !d_out_normals || !d_out_kept))
        return dmn_fail(DMNERF_E_ARG, "surface_clean_compact: null pointer");
    if (Fk) {
        hipLaunchKernelGGL(sf_compact_faces_kernel, dim3(sf_blocks(F)), dim3(SF_BLOCK), 0, (hipStream_t)stream, d_faces, F, V, d_keep, d_fscan,
                           d_vscan, Fk, d_out_faces);
        if (int rc = dmn_check_launch("surface_clean_compact: faces")) return rc;
    }
    if (Vk) {
        hipLaunchKernelGGL(sf_compact_vertices_kernel, dim3(sf_blocks(V)), dim3(SF_BLOCK), 0, (hipStream_t)stream, d_vertices, d_normals, V,
                           d_used, d_vscan, Vk, d_out_vertices, d_out_normals, d_out_kept);
        if (int rc = dmn_check_launch("surface_clean_compact: vertices")) return rc;
    }
    return DMNERF_OK;
}
