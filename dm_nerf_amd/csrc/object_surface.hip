// object_surface.hip -- one closed iso-surface per object of a label volume, all objects in one pass over the grid: what a loop
// over the labels k round surface.hip's extract (tools/mesh_generator.py:68 on the masked field M_k = value where labels == k, else
// fill = 0) gives, bit for bit and in its order.  tests/_object_surface_restate.py states that loop in numpy.
//
// Conventions: value [dx, dy, dz] f32 and labels [dx, dy, dz] uint8, row-major.  A label >= C, 255 included, or one whose bit is
// clear in the mask owns nothing: the kernels read it as 255.  Point p is inside object k iff labels[p] == k and value[p] > level
// (NaN: outside); level > 0, so a fill point is outside every object.  With `closed` the kernels walk the EXTENDED grid of
// (dx + 2) (dy + 2) (dz + 2) points whose outer layer is fill, owned by nobody, and subtract 1 from every coordinate after the
// vertex formula (as the loop does on a padded copy); no padded copy is made.  Everything below indexes the extended grid:
// linear index p = (i Dy + j) Dz + k, D = d + 2 pad.
//
//   os_count_kernel     a workgroup owns OS_TI x OS_TJ x OS_TK points and stages the INSIDE LABEL (the label where the point is
//                       inside its object, else 255) of each with the upper halo through LDS, one byte per point, reading value
//                       and labels once per tile.  An edge between two different inside labels carries a vertex per non-255 end
//                       (0..6 per point); a cell carries, per distinct inside label among its corners, the triangles of that
//                       object's case (0..40 per cell over all objects)
//   os_vertices_kernel  per point with a nonzero count and per crossing edge and object: t = (level - a) / (b - a) on the masked
//                       operands -- the far end contributes its real value iff it carries the same label -- the position, the
//                       linear index in the REAL grid of the end that is inside, and the key (label << 40) | (3 p + axis)
//   os_faces_kernel     per cell with triangles and per object of the cell: the key (label << 40) | (5 p + t) of every triangle
//                       and, per corner, the key of the vertex on that cell edge for that object
// The caller sorts the (unique) vertex and triangle keys: that is the order (object, owning point, axis) / (object, cell, table
// position), and a corner's vertex id is the rank of its key among the sorted vertex keys.  The up to 8 labels of a cell stay in
// registers: every loop over them is unrolled with constant indices, duplicates are found by compares in that fixed order.
//
//   os_measures_kernel  one workgroup per object: the float64 area and signed volume of its triangles, summed per thread in
//                       ascending triangle index with stride OS_BLOCK and then over the threads by a fixed LDS tree.  No atomics.
// Memory-bound throughout: no MFMA, no inline assembly, no floating-point atomic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "mc_tables.h"

namespace {

constexpr int OS_TI = 8, OS_TJ = 8, OS_TK = 32;                       // points per workgroup (tests/test_gpu_object_surface.py reads these)
constexpr int OS_HI = OS_TI + 1, OS_HJ = OS_TJ + 1, OS_HK = OS_TK + 1;
constexpr int OS_THREADS = OS_TJ * OS_TK;                             // 256: one (j, k) column per thread, OS_TI points each
constexpr int OS_BLOCK = 256;
constexpr int OS_NONE = 255;
constexpr int OS_KEY_SHIFT = 40;                                      // 3 p + axis and 5 p + t are < 2^34 for p < 2^31

struct ObjGrid {
    int dx, dy, dz;                                                   // the real grid
    int Dx, Dy, Dz;                                                   // the extended grid: d + 2 pad
    int pad, C;
    uint32_t m0, m1, m2, m3;                                          // the selected labels, bit l of the 128
    float level;
};

struct ObjPoint {
    float v;                                                          // the value (0 outside the real grid)
    int l;                                                            // the label, OS_NONE where nobody (selected) owns the point
    int il;                                                           // l where the point is inside its object, else OS_NONE
    int64_t real;                                                     // the linear index in the real grid (0 outside it)
};

__device__ __forceinline__ ObjPoint os_point(const float* __restrict__ value, const uint8_t* __restrict__ labels, const ObjGrid& g, int i,
                                             int j, int k) {
    ObjPoint p{0.f, OS_NONE, OS_NONE, 0};
    i -= g.pad, j -= g.pad, k -= g.pad;
    if ((unsigned)i >= (unsigned)g.dx || (unsigned)j >= (unsigned)g.dy || (unsigned)k >= (unsigned)g.dz) return p;
    p.real = ((int64_t)i * g.dy + j) * g.dz + k;
    p.v = value[p.real];
    const int l = labels[p.real];
    if (l >= g.C) return p;                                           // C <= 128, so the mask has a bit for l
    const uint32_t w = l < 64 ? (l < 32 ? g.m0 : g.m1) : (l < 96 ? g.m2 : g.m3);
    if (!((w >> (l & 31)) & 1u)) return p;
    p.l = l;
    p.il = p.v > g.level ? l : OS_NONE;
    return p;
}

// The triangles of a cell over all its objects, from the inside labels c[0..8) of its corners (constant indices only).
__device__ __forceinline__ int os_cell_triangles(const int (&c)[8]) {
    int nt = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        bool first = c[q] != OS_NONE;
#pragma unroll
        for (int r = 0; r < q; ++r) first = first && c[r] != c[q];
        if (!first) continue;
        int mc_case = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) mc_case |= (int)(c[r] == c[q]) << r;
        nt += mc_triangles(mc_case);
    }
    return nt;
}

__global__ __launch_bounds__(OS_THREADS) void os_count_kernel(const float* __restrict__ value, const uint8_t* __restrict__ labels, ObjGrid g,
                                                               int nbj, int nbk, uint8_t* __restrict__ vcnt, uint8_t* __restrict__ tcnt) {
    __shared__ uint8_t s[OS_HI * OS_HJ * OS_HK];
    const int b = blockIdx.x;
    const int i0 = (b / (nbj * nbk)) * OS_TI, j0 = ((b / nbk) % nbj) * OS_TJ, k0 = (b % nbk) * OS_TK;
    for (int x = threadIdx.x; x < OS_HI * OS_HJ * OS_HK; x += OS_THREADS) {
        const int c = x % OS_HK, bb = (x / OS_HK) % OS_HJ, a = x / (OS_HK * OS_HJ);
        const int i = i0 + a, j = j0 + bb, k = k0 + c;
        int il = OS_NONE;                                               // beyond the extended grid: never used (the edge does not exist)
        if (i < g.Dx && j < g.Dy && k < g.Dz) il = os_point(value, labels, g, i, j, k).il;
        s[x] = (uint8_t)il;
    }
    __syncthreads();
    const int tj = threadIdx.x / OS_TK, tk = threadIdx.x % OS_TK;
    const int j = j0 + tj, k = k0 + tk;
    if (j >= g.Dy || k >= g.Dz) return;
    const bool hj = j + 1 < g.Dy, hk = k + 1 < g.Dz;
#pragma unroll
    for (int ti = 0; ti < OS_TI; ++ti) {
        const int i = i0 + ti;
        if (i >= g.Dx) break;
        const bool hi = i + 1 < g.Dx;
        const uint8_t* t = s + (ti * OS_HJ + tj) * OS_HK + tk;
        int c[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) c[q] = t[(MC_CORNER[q][0] * OS_HJ + MC_CORNER[q][1]) * OS_HK + MC_CORNER[q][2]];
        int nv = 0;
        if (hi && c[0] != c[4]) nv += (int)(c[0] != OS_NONE) + (int)(c[4] != OS_NONE);
        if (hj && c[0] != c[3]) nv += (int)(c[0] != OS_NONE) + (int)(c[3] != OS_NONE);
        if (hk && c[0] != c[1]) nv += (int)(c[0] != OS_NONE) + (int)(c[1] != OS_NONE);
        const int nt = hi && hj && hk ? os_cell_triangles(c) : 0;
        const int64_t p = ((int64_t)i * g.Dy + j) * g.Dz + k;
        vcnt[p] = (uint8_t)nv;
        tcnt[p] = (uint8_t)nt;
    }
}

__global__ __launch_bounds__(OS_BLOCK) void os_vertices_kernel(const float* __restrict__ value, const uint8_t* __restrict__ labels, ObjGrid g,
                                                                const uint8_t* __restrict__ vcnt, const int64_t* __restrict__ vscan, int64_t V,
                                                                int64_t* __restrict__ vkey, float* __restrict__ vpos, int32_t* __restrict__ vcell) {
    const int64_t n = (int64_t)g.Dx * g.Dy * g.Dz;
    const int64_t p = (int64_t)blockIdx.x * OS_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int nv = vcnt[p];
    if (nv == 0) return;
    const int k = (int)(p % g.Dz), j = (int)((p / g.Dz) % g.Dy), i = (int)(p / ((int64_t)g.Dz * g.Dy));
    const ObjPoint P = os_point(value, labels, g, i, j, k);
    const float shift = (float)g.pad;
    int64_t o = vscan[p] - nv;
    const int64_t end = o + nv;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int qi = i + (ax == 0), qj = j + (ax == 1), qk = k + (ax == 2);
        if (qi >= g.Dx || qj >= g.Dy || qk >= g.Dz) continue;
        const ObjPoint Q = os_point(value, labels, g, qi, qj, qk);
        if (P.il == Q.il) continue;
#pragma unroll
        for (int side = 0; side < 2; ++side) {                          // the object of the lower end, then that of the upper end
            const int l = side == 0 ? P.il : Q.il;
            if (l == OS_NONE) continue;
            if (o < 0 || o >= V || o >= end) return;                    // inconsistent scans: write nothing out of bounds
            const float a = side == 0 ? P.v : (P.l == l ? P.v : 0.f);   // the masked field of object l at the two ends
            const float bv = side == 0 ? (Q.l == l ? Q.v : 0.f) : Q.v;
            const float t = (g.level - a) / (bv - a);
            float pos[3] = {(float)i, (float)j, (float)k};
            pos[ax] = pos[ax] + t;
            vpos[3 * o + 0] = pos[0] - shift;
            vpos[3 * o + 1] = pos[1] - shift;
            vpos[3 * o + 2] = pos[2] - shift;
            vcell[o] = (int32_t)(side == 0 ? P.real : Q.real);
            vkey[o] = ((int64_t)l << OS_KEY_SHIFT) | (3 * p + ax);
            ++o;
        }
    }
}

__global__ __launch_bounds__(OS_BLOCK) void os_faces_kernel(const float* __restrict__ value, const uint8_t* __restrict__ labels, ObjGrid g,
                                                             const uint8_t* __restrict__ tcnt, const int64_t* __restrict__ tscan, int64_t F,
                                                             int64_t* __restrict__ tkey, int64_t* __restrict__ ckey) {
    const int64_t n = (int64_t)g.Dx * g.Dy * g.Dz;
    const int64_t p = (int64_t)blockIdx.x * OS_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int nt = tcnt[p];
    if (nt == 0) return;
    const int k = (int)(p % g.Dz), j = (int)((p / g.Dz) % g.Dy), i = (int)(p / ((int64_t)g.Dz * g.Dy));
    if (i + 1 >= g.Dx || j + 1 >= g.Dy || k + 1 >= g.Dz) return;       // not a cell (the count kernel wrote 0 here)
    int c[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) c[q] = os_point(value, labels, g, i + MC_CORNER[q][0], j + MC_CORNER[q][1], k + MC_CORNER[q][2]).il;
    int64_t o = tscan[p] - nt;
    const int64_t end = o + nt;
    if (o < 0 || end > F) return;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        bool first = c[q] != OS_NONE;
#pragma unroll
        for (int r = 0; r < q; ++r) first = first && c[r] != c[q];
        if (!first) continue;
        int mc_case = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) mc_case |= (int)(c[r] == c[q]) << r;
        const int m = mc_triangles(mc_case);
        if (o + m > end) return;                                        // the counts are of another volume: write nothing out of bounds
        const int64_t object = (int64_t)c[q] << OS_KEY_SHIFT;
        for (int t = 0; t < m; ++t) {
            tkey[o + t] = object | (5 * p + t);
            for (int s = 0; s < 3; ++s) {
                const int e = MC_TRI[mc_case][3 * t + s];
                const int64_t owner = ((int64_t)(i + MC_EDGE[e][0]) * g.Dy + (j + MC_EDGE[e][1])) * g.Dz + (k + MC_EDGE[e][2]);
                ckey[3 * (o + t) + s] = object | (3 * owner + MC_EDGE[e][3]);
            }
        }
        o += m;
    }
}

struct Scale3 { double x, y, z; };

__global__ __launch_bounds__(OS_BLOCK) void os_measures_kernel(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ faces,
                                                                int64_t F, const int64_t* __restrict__ face_offset, Scale3 cell,
                                                                double* __restrict__ area, double* __restrict__ volume) {
    __shared__ double sa[OS_BLOCK], sw[OS_BLOCK];
    const int obj = blockIdx.x;
    int64_t f0 = face_offset[obj], f1 = face_offset[obj + 1];
    if (f0 < 0) f0 = 0;
    if (f1 > F) f1 = F;
    double a = 0.0, w = 0.0;
    for (int64_t f = f0 + threadIdx.x; f < f1; f += OS_BLOCK) {
        double q[3][3];
        bool ok = true;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int64_t v = faces[3 * f + s];
            ok = ok && v >= 0 && v < V;
            const int64_t u = ok ? v : 0;
            q[s][0] = (double)vertices[3 * u + 0] * cell.x;
            q[s][1] = (double)vertices[3 * u + 1] * cell.y;
            q[s][2] = (double)vertices[3 * u + 2] * cell.z;
        }
        if (!ok) continue;
        const double ux = q[1][0] - q[0][0], uy = q[1][1] - q[0][1], uz = q[1][2] - q[0][2];
        const double wx = q[2][0] - q[0][0], wy = q[2][1] - q[0][1], wz = q[2][2] - q[0][2];
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        a = a + sqrt((nx * nx + ny * ny) + nz * nz);
        const double cx = q[1][1] * q[2][2] - q[1][2] * q[2][1], cy = q[1][2] * q[2][0] - q[1][0] * q[2][2],
                     cz = q[1][0] * q[2][1] - q[1][1] * q[2][0];
        w = w + ((q[0][0] * cx + q[0][1] * cy) + q[0][2] * cz);
    }
    sa[threadIdx.x] = a;
    sw[threadIdx.x] = w;
    __syncthreads();
    for (int st = OS_BLOCK / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            sa[threadIdx.x] = sa[threadIdx.x] + sa[threadIdx.x + st];
            sw[threadIdx.x] = sw[threadIdx.x] + sw[threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        area[obj] = sa[0] / 2.0;
        volume[obj] = sw[0] / 6.0;
    }
}

inline unsigned os_blocks(int64_t n) { return (unsigned)((n + OS_BLOCK - 1) / OS_BLOCK); }
constexpr int64_t OS_MAX = ((int64_t)1 << 31) - 1;                      // vertex and triangle ids are int32

// The checks the two grid entries share -> the kernel argument and the number of extended points.
int os_grid(const char* who, const float* d_value, const uint8_t* d_labels, int dx, int dy, int dz, int C, const uint32_t* label_mask,
            float level, int closed, ObjGrid* g, int64_t* n) {
    const int dims[3] = {dx, dy, dz};
    if (int rc = dmn_grid_dims(who, dims)) return rc;
    if (int rc = dmn_check_labels(who, C)) return rc;
    if (!(level > 0.f) || !std::isfinite(level)) return dmn_fail(DMNERF_E_ARG, "%s: level must be > 0 and finite, got %g", who, (double)level);
    if (closed != 0 && closed != 1) return dmn_fail(DMNERF_E_ARG, "%s: closed must be 0 or 1, got %d", who, closed);
    if (!d_value || !d_labels || !label_mask) return dmn_fail(DMNERF_E_ARG, "%s: null pointer", who);
    const int pad = closed;
    *n = ((int64_t)dx + 2 * pad) * ((int64_t)dy + 2 * pad) * ((int64_t)dz + 2 * pad);
    if (*n >= ((int64_t)1 << 31)) return dmn_fail(DMNERF_E_ARG, "%s: %lld points (with the border) do not fit int32", who, (long long)*n);
    *g = ObjGrid{dx, dy, dz, dx + 2 * pad, dy + 2 * pad, dz + 2 * pad, pad, C, label_mask[0], label_mask[1], label_mask[2], label_mask[3], level};
    return DMNERF_OK;
}

}  // namespace

extern "C" int32_t dmnerf_object_surface_count(const float* d_value, const uint8_t* d_labels, int dx, int dy, int dz, int C,
                                           const uint32_t* label_mask, float level, int closed, uint8_t* d_vcount, uint8_t* d_tcount,
                                           void* stream) {
    ObjGrid g;
    int64_t n;
    if (int rc = os_grid("object_surface_count", d_value, d_labels, dx, dy, dz, C, label_mask, level, closed, &g, &n)) return rc;
    if (!d_vcount || !d_tcount) return dmn_fail(DMNERF_E_ARG, "object_surface_count: null pointer");
    const int nbi = (g.Dx + OS_TI - 1) / OS_TI, nbj = (g.Dy + OS_TJ - 1) / OS_TJ, nbk = (g.Dz + OS_TK - 1) / OS_TK;
    const int64_t blocks = (int64_t)nbi * nbj * nbk;
    if (blocks >= ((int64_t)1 << 31)) return dmn_fail(DMNERF_E_ARG, "object_surface_count: too many tiles");
    hipLaunchKernelGGL(os_count_kernel, dim3((unsigned)blocks), dim3(OS_THREADS), 0, (hipStream_t)stream, d_value, d_labels, g, nbj, nbk,
                       d_vcount, d_tcount);
    return dmn_check_launch("object_surface_count");
}

extern "C" int32_t dmnerf_object_surface_emit(const float* d_value, const uint8_t* d_labels, int dx, int dy, int dz, int C,
                                          const uint32_t* label_mask, float level, int closed, const uint8_t* d_vcount,
                                          const uint8_t* d_tcount, const int64_t* d_vscan, const int64_t* d_tscan, int64_t V, int64_t F,
                                          int64_t* d_vkey, float* d_vpos, int32_t* d_vcell, int64_t* d_tkey, int64_t* d_ckey, void* stream) {
    ObjGrid g;
    int64_t n;
    if (int rc = os_grid("object_surface_emit", d_value, d_labels, dx, dy, dz, C, label_mask, level, closed, &g, &n)) return rc;
    if (V < 0 || F < 0 || V > OS_MAX || F > OS_MAX)
        return dmn_fail(DMNERF_E_ARG, "object_surface_emit: V=%lld F=%lld do not fit int32 ids", (long long)V, (long long)F);
    if (!d_vcount || !d_tcount || !d_vscan || !d_tscan || (V && (!d_vkey || !d_vpos || !d_vcell)) || (F && (!d_tkey || !d_ckey)))
        return dmn_fail(DMNERF_E_ARG, "object_surface_emit: null pointer");
    if (V) {
        hipLaunchKernelGGL(os_vertices_kernel, dim3(os_blocks(n)), dim3(OS_BLOCK), 0, (hipStream_t)stream, d_value, d_labels, g, d_vcount,
                           d_vscan, V, d_vkey, d_vpos, d_vcell);
        if (int rc = dmn_check_launch("object_surface_emit: vertices")) return rc;
    }
    if (F) {
        hipLaunchKernelGGL(os_faces_kernel, dim3(os_blocks(n)), dim3(OS_BLOCK), 0, (hipStream_t)stream, d_value, d_labels, g, d_tcount, d_tscan,
                           F, d_tkey, d_ckey);
        if (int rc = dmn_check_launch("object_surface_emit: faces")) return rc;
    }
    return DMNERF_OK;
}

extern "C" int32_t dmnerf_object_surface_measures(const float* d_vertices, int64_t V, const int32_t* d_faces, int64_t F,
                                              const int64_t* d_face_offset, int C, const double* cell, double* d_area, double* d_volume,
                                              void* stream) {
    if (int rc = dmn_check_labels("object_surface_measures", C)) return rc;
    if (V < 0 || F < 0 || V > OS_MAX || F > OS_MAX)
        return dmn_fail(DMNERF_E_ARG, "object_surface_measures: bad V=%lld F=%lld", (long long)V, (long long)F);
    if (!cell || !d_face_offset || !d_area || !d_volume || (F && (!d_vertices || !d_faces)))
        return dmn_fail(DMNERF_E_ARG, "object_surface_measures: null pointer");
    hipLaunchKernelGGL(os_measures_kernel, dim3((unsigned)C), dim3(OS_BLOCK), 0, (hipStream_t)stream, d_vertices, V, d_faces, F, d_face_offset,
                       Scale3{cell[0], cell[1], cell[2]}, d_area, d_volume);
    return dmn_check_launch("object_surface_measures");
}
