// field_edit.hip -- the trained field rendered through an edited volume, one network evaluation per sample: who owns the cell a
// sample falls into decides WHERE the network is asked (networks/render.py run_network_edited; DESIGN.md 8a, "The field-edit route").
//
//   dmnerf_field_edit_select   dmnerf_skip_select_fill with the byte volume `source` of dmnerf_volume_edit in place of the bit grid.
//                              Sample m = n S + s has the point p = o + d z and the cell of grid_cell_of_sample (grid_volume.h): the
//                              select's cell, one function.  Its OWNER is source[cell] inside the box (a byte that names a
//                              REMOVE entry or is > E reads as 255), the `outside` policy outside it and the `unowned` policy where
//                              the byte is 255: EVALUATE gives owner 0, EMPTY gives 255.  Owner 255: not evaluated, the row of
//                              `rows` becomes fill_row.  Owner 0: evaluated on its own ray, (o, d) copied bit for bit.  Owner 1 + e:
//                              evaluated on the ray carried back into the trained scene by entry e's matrix,
//                                  o_w_a = ((m_a0 o_x + m_a1 o_y) + m_a2 o_z) + m_a3,   d_w_a = (m_a0 d_x + m_a1 d_y) + m_a2 d_z,
//                              every operation rounded on its own (dmnerf_volume_edit's product).  o + d z is affine in (o, d), so
//                              the network, called with S = 1 on (o_w[m], d_w[m], z[m]), lands on M_e p.
//   dmnerf_field_edit_filter   the exchanger's per-sample rule behind the network: the label of an evaluated row is the first maximum
//                              of its C logits (dmnerf_label_cells' argmax, no sigma threshold); a row whose label is not in its
//                              owner's accept mask becomes fill_row.
//
// The entry that owns a sample differs from lane to lane.  The table is a kernel argument and is walked with a wave-uniform counter
// (scalar loads); a lane takes the entry whose number equals its owner, and a wave skips the entries none of its lanes has: no
// per-lane index into the argument, no register array, no scratch.  The accept masks are walked the same way.  The selection is
// the select's three passes (per-block counts here, then skip.hip's scan and scatter by prefix sums): ascending, the same list every
// run.  The kept counts are ballots and popcounts into the workgroup's LDS table and one flush with integer atomics.  No float
// atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "grid_volume.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NOBODY = 255;
constexpr int MAX_E = DMNERF_VOLUME_EDIT_MAX;
constexpr int KIND_REMOVE = 2;

struct FieldEntries {
    dmnerf_volume_edit_entry e[MAX_E];
};

struct FieldBox {
    GridBox box;
    int outside_owner, unowned_owner;          // 0 ("evaluate") or 255 ("empty")
    unsigned long long evaluable;              // bit b: a source byte b <= E is an owner (bit 0; bit 1 + e for a MOVE / COPY entry e)
};

struct FieldMasks {
    LabelMask128 m[1 + MAX_E];
};

// ---- select, pass 1: owner, the ray of every evaluated sample, the block's count, the fill of the rows nobody evaluates
__global__ __launch_bounds__(BLOCK) void field_edit_owner_kernel(FieldBox G, const uint8_t* __restrict__ source, FieldEntries ent, int E,
                                                                 const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                                 const float* __restrict__ z, int64_t M, int S,
                                                                 uint8_t* __restrict__ owner, float* __restrict__ o_w,
                                                                 float* __restrict__ d_w, int* __restrict__ block_n,
                                                                 float* __restrict__ rows, const float* __restrict__ fill_row, int width) {
    __shared__ uint8_t block_fill[BLOCK];
    const int64_t m0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t m = m0 + threadIdx.x;
    int own = NOBODY;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (m < M) {
        const int64_t n = m / S;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o[a] = rays_o[n * 3 + a];
            d[a] = rays_d[n * 3 + a];
        }
        int64_t g;
        if (grid_cell_of_sample(G.box, rays_o, rays_d, n, z[m], &g)) {        // (the select's cell rule)
            int b = source[g];
            if (b > E || ((G.evaluable >> b) & 1ull) == 0) b = NOBODY;          // (b <= E <= 32: the shift is defined)
            own = b == NOBODY ? G.unowned_owner : b;
        } else {
            own = G.outside_owner;
        }
        owner[m] = (uint8_t)own;
    }
    // (the trip count and the counter are the wave's: every lane stays in the loop, so the ballot sees the whole wave)
    float ow[3] = {o[0], o[1], o[2]}, dw[3] = {d[0], d[1], d[2]};
    for (int e = 0; e < E; ++e) {
        const bool mine = own == 1 + e;
        if (__ballot(mine) == 0) continue;
        const float* q = ent.e[e].m;
        if (mine) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float m0_ = q[4 * a], m1_ = q[4 * a + 1], m2_ = q[4 * a + 2], m3_ = q[4 * a + 3];
                ow[a] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m0_, o[0]), __fmul_rn(m1_, o[1])), __fmul_rn(m2_, o[2])), m3_);
                dw[a] = __fadd_rn(__fadd_rn(__fmul_rn(m0_, d[0]), __fmul_rn(m1_, d[1])), __fmul_rn(m2_, d[2]));
            }
        }
    }
    const bool f = own != NOBODY;                                  // (m >= M: NOBODY)
    if (f) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o_w[m * 3 + a] = ow[a];
            d_w[m * 3 + a] = dw[a];
        }
    }
    block_fill[threadIdx.x] = f ? 0 : 1;
    int rank;
    const int total = block_count_and_rank<BLOCK>(f, &rank);       // (its barrier also publishes block_fill)
    if (threadIdx.x == 0) block_n[blockIdx.x] = total;
    if (rows) fill_block_rows<BLOCK>(block_fill, rows, fill_row, m0, M, width);
}

// (passes 2 and 3, with owner != 255 as the flag: dmn_select_finish, skip.hip)

// ---- filter.  One sample per lane; a row is 4 + C <= 132 floats.
__global__ void field_edit_kept_init_kernel(int E, unsigned long long* __restrict__ kept) {
    if ((int)threadIdx.x <= E) kept[threadIdx.x] = 0;
}

__global__ __launch_bounds__(BLOCK) void field_edit_filter_kernel(float* __restrict__ raw, const uint8_t* __restrict__ owner, int64_t M, int C,
                                                                  FieldMasks masks, int E, const float* __restrict__ fill_row,
                                                                  unsigned long long* __restrict__ kept) {
    __shared__ uint8_t block_fill[BLOCK];
    __shared__ unsigned int s_kept[1 + MAX_E];
    if ((int)threadIdx.x <= E) s_kept[threadIdx.x] = 0;
    __syncthreads();
    const int64_t m0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t m = m0 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int own = m < M ? (int)owner[m] : NOBODY;
    const bool active = own <= E;                                  // (255, and any byte the select cannot have written, is left alone)
    uint32_t label = 0;
    if (active) {                                                  // dmnerf_label_cells' argmax: the first maximum, NaN rules included
        const float* x = raw + m * (4 + C);
        float bv = x[4];
        for (int c = 1; c < C; ++c) {
            const float v = x[4 + c];
            if (v > bv) { bv = v; label = (uint32_t)c; }
        }
    }
    bool keep = false;
    for (int w = 0; w <= E; ++w) {                                 // (wave-uniform: scalar loads of the mask words)
        const bool in_w = active && own == w;
        if (__ballot(in_w) == 0) continue;
        const bool ok = in_w && mask_bit(masks.m[w], label);
        const int n = __popcll(__ballot(ok));
        if (n && lane == 0) atomicAdd(&s_kept[w], (unsigned int)n);
        keep = keep || ok;
    }
    block_fill[threadIdx.x] = (active && !keep) ? 1 : 0;
    __syncthreads();
    fill_block_rows<BLOCK>(block_fill, raw, fill_row, m0, M, 4 + C);
    if (kept && (int)threadIdx.x <= E && s_kept[threadIdx.x]) atomicAdd(&kept[threadIdx.x], (unsigned long long)s_kept[threadIdx.x]);
}

}  // namespace

extern "C" int32_t dmnerf_field_edit_select(const uint8_t* d_source, const float lo[3], const float inv_cell[3], const int dims[3], int outside,
                                        int unowned, const dmnerf_volume_edit_entry* entries, int E, int C, const float* d_rays_o,
                                        const float* d_rays_d, const float* d_z, int64_t N, int S, uint8_t* d_owner, float* d_o_w,
                                        float* d_d_w, int* d_sel, int* d_count, int* d_work, float* d_rows, const float* d_fill_row,
                                        int64_t* d_totals, void* stream) {
    const char* who = "field_edit_select";
    hipStream_t st = (hipStream_t)stream;
    if (!lo || !inv_cell || !dims) return dmn_fail(DMNERF_E_ARG, "%s: null host array", who);      // (before N and S, as ever)
    if (N < 0 || S < 1) return dmn_fail(DMNERF_E_ARG, "%s: bad N=%lld S=%d", who, (long long)N, S);
    const int64_t M = N * S;
    if (M >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "%s: %lld samples do not fit the int32 selection", who, (long long)M);
    FieldBox G;
    int64_t cells;
    if (int rc = dmn_grid_given(who, lo, nullptr, inv_cell, dims, &G.box, &cells)) return rc;
    for (int policy : {outside, unowned})
        if (policy != DMNERF_SKIP_OUTSIDE_EVALUATE && policy != DMNERF_SKIP_OUTSIDE_EMPTY)
            return dmn_fail(DMNERF_E_ARG, "%s: policy %d unknown (outside %d, unowned %d)", who, policy, outside, unowned);
    if (int rc = dmn_check_labels(who, C)) return rc;
    if (int rc = dmn_edit_count_given(who, E, entries)) return rc;
    FieldEntries ent = {};
    if (int rc = dmn_edit_entries_given(who, entries, E, C, ent.e)) return rc;
    G.evaluable = 1ull;
    for (int e = 0; e < E; ++e)
        if (ent.e[e].kind != KIND_REMOVE) G.evaluable |= 1ull << (1 + e);
    G.outside_owner = outside == DMNERF_SKIP_OUTSIDE_EVALUATE ? 0 : NOBODY;
    G.unowned_owner = unowned == DMNERF_SKIP_OUTSIDE_EVALUATE ? 0 : NOBODY;
    if (!d_count) return dmn_fail(DMNERF_E_ARG, "%s: null pointer", who);
    if (d_rows && !d_fill_row) return dmn_fail(DMNERF_E_ARG, "%s: rows without a fill row", who);
    if (M == 0) return DMNERF_OK;                                  // (no launch: *d_count is not written)
    if (!d_source || !d_rays_o || !d_rays_d || !d_z || !d_owner || !d_o_w || !d_d_w || !d_sel || !d_work)
        return dmn_fail(DMNERF_E_ARG, "%s: null pointer", who);
    const int64_t nb = (M + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(field_edit_owner_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, st, G, d_source, ent, E, d_rays_o, d_rays_d, d_z, M, S,
                       d_owner, d_o_w, d_d_w, d_work, d_rows, d_fill_row, 4 + C);
    dmn_select_finish(d_owner, NOBODY, M, d_work, d_sel, d_count, d_totals, st);
    return dmn_check_launch(who);
}

extern "C" int32_t dmnerf_field_edit_filter(float* d_raw, const uint8_t* d_owner, int64_t M, int C, const uint32_t* masks, int E,
                                        const float* d_fill_row, int64_t* d_kept, void* stream) {
    const char* who = "field_edit_filter";
    if (M < 0 || M >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "%s: bad M=%lld (0 <= M < 2^31)", who, (long long)M);
    if (int rc = dmn_check_labels(who, C)) return rc;
    if (int rc = dmn_edit_count_given(who, E, nullptr, false)) return rc;
    if (!masks) return dmn_fail(DMNERF_E_ARG, "%s: null masks", who);
    if (M == 0) return DMNERF_OK;
    if (!d_raw || !d_owner || !d_fill_row) return dmn_fail(DMNERF_E_ARG, "%s: null pointer", who);
    FieldMasks k = {};
    for (int w = 0; w <= E; ++w)
        for (int q = 0; q < 4; ++q) k.m[w].w[q] = masks[4 * w + q];
    unsigned long long* kept = reinterpret_cast<unsigned long long*>(d_kept);
    if (kept) hipLaunchKernelGGL(field_edit_kept_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, E, kept);
    const int64_t nb = (M + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(field_edit_filter_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, d_raw, d_owner, M, C, k, E, d_fill_row,
                       kept);
    return dmn_check_launch(who);
}
