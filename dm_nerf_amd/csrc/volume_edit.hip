// volume_edit.hip -- an edit applied to the label / baked volume itself: the volume resampled under a list of moves, copies and
// removals, and what the edit covers and collides with.  The result is a volume of the same kind over the same box, so everything
// that reads a volume (stats, bit grids, the trace, the baked render, a second edit) reads an edited one.
//
//   dmnerf_volume_edit   one lane per DESTINATION cell g = (i * dy + j) * dz + k (k fastest: coalesced stores).  The target pose of
//                        an entry is trans @ pose, so a point x of a pixel's original ray corresponds to trans x on its target ray:
//                        the edited volume at x is the source volume at trans x.  The matrix maps the destination point to its
//                        source point; no inverse is taken.
//
// Per cell, in f32 with every operation rounded on its own (the Makefile's -ffp-contract=off): the centre p_a = (idx_a + 0.5) cell_a +
// lo_a; candidate 0 is the cell's own content (label < C, kept, not the label of a MOVE / REMOVE entry); candidate 1 + e, for a MOVE or
// COPY entry e, is the source cell c_a = floor((q_a - lo_a) inv_cell_a) of q = M_e p, if it lies in the box and carries the entry's
// (kept) label.  Nearest-cell resampling: no interpolation.  The winner is the lowest candidate (rule 0) or the one with the largest
// source sigma, the lowest on ties, a NaN never beating a number (rule 1).  tests/_volume_edit_restate.py states all of it in numpy.
//
// The entry loop runs over kernel arguments with a wave-uniform counter: scalar loads, no register indexing, no scratch.  The counts
// are integers: ballots and popcounts per wave into the workgroup's LDS table, one flush with global integer atomics, which commute:
// the same numbers every run.  The pair loop behind `hits` runs only in waves that hold a cell with two or more candidates.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "grid_volume.h"

namespace {

constexpr int BLOCK = 256;
constexpr int UNLABELLED = 255;
constexpr int MAX_E = DMNERF_VOLUME_EDIT_MAX;
constexpr int MAX_BLOCKS = 4096;              // the grid; beyond it a workgroup strides (an LDS counter then stays below 2^25)
constexpr int KIND_COPY = 1, KIND_REMOVE = 2;

struct EditEntries {
    dmnerf_volume_edit_entry e[MAX_E];
};

__global__ void volume_edit_init_kernel(int E, int C, unsigned long long* __restrict__ won, unsigned long long* __restrict__ claimed,
                                        unsigned long long* __restrict__ hits) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= E) won[t] = 0;
    if (t < E) claimed[t] = 0;
    if (t < E * C) hits[t] = 0;
}

template <bool BAKED>
__global__ __launch_bounds__(BLOCK) void volume_edit_kernel(const uint8_t* __restrict__ labels, const uint4* __restrict__ cells, GridBox box,
                                                            int C, LabelMask128 keep, LabelMask128 gone, EditEntries ent, int E, int rule,
                                                            uint8_t* __restrict__ out_labels, uint4* __restrict__ out_cells,
                                                            uint8_t* __restrict__ out_source, unsigned long long* __restrict__ won,
                                                            unsigned long long* __restrict__ claimed,
                                                            unsigned long long* __restrict__ hits) {
    __shared__ unsigned int s_won[1 + MAX_E], s_claimed[MAX_E], s_hits[MAX_E * DMNERF_MAX_LOGITS];
    for (int t = threadIdx.x; t < E * C; t += BLOCK) s_hits[t] = 0;
    if (threadIdx.x <= E) s_won[threadIdx.x] = 0;
    if (threadIdx.x < E) s_claimed[threadIdx.x] = 0;
    __syncthreads();

    const int dy = box.dims[1], dz = box.dims[2];
    const uint32_t total = (uint32_t)box.dims[0] * (uint32_t)dy * (uint32_t)dz;
    const int lane = threadIdx.x & 63;
    const float* sigma_of = reinterpret_cast<const float*>(cells);
    const bool densest = BAKED && rule == 1;

    // (the trip count is the workgroup's: every lane stays in the loop, so the ballots below see whole waves)
    // (total < 2^31 and the grid's stride is at most 2^20 cells: 32-bit indices do not wrap)
    for (uint32_t g0 = blockIdx.x * BLOCK; g0 < total; g0 += gridDim.x * BLOCK) {
        const uint32_t g = g0 + threadIdx.x;
        const bool valid = g < total;
        const uint32_t gi = valid ? g : 0u;
        const int k = (int)(gi % (uint32_t)dz);
        const uint32_t r = gi / (uint32_t)dz;
        const int j = (int)(r % (uint32_t)dy);
        const int i = (int)(r / (uint32_t)dy);
        const float px = ((float)i + 0.5f) * box.cell[0] + box.lo[0];
        const float py = ((float)j + 0.5f) * box.cell[1] + box.lo[1];
        const float pz = ((float)k + 0.5f) * box.cell[2] + box.lo[2];

        const uint32_t l0 = valid ? labels[g] : (uint32_t)UNLABELLED;
        const bool own = valid && l0 < (uint32_t)C && mask_bit(keep, l0) && !mask_bit(gone, l0);
        unsigned long long cand = own ? 1ull : 0ull;                // bit 0: the cell's own content, bit 1 + e: entry e
        int win = own ? 0 : -1;
        uint32_t win_label = own ? l0 : (uint32_t)UNLABELLED;
        int64_t win_src = gi;
        float win_sigma = 0.f;
        if (densest && own) win_sigma = sigma_of[(int64_t)g * 4 + 3];

        for (int e = 0; e < E; ++e) {
            const int kind = ent.e[e].kind;
            const uint32_t lab = (uint32_t)ent.e[e].label;
            if (kind == KIND_REMOVE || !mask_bit(keep, lab)) continue;              // (uniform)
            const float* m = ent.e[e].m;
            const float q[3] = {((m[0] * px + m[1] * py) + m[2] * pz) + m[3], ((m[4] * px + m[5] * py) + m[6] * pz) + m[7],
                                ((m[8] * px + m[9] * py) + m[10] * pz) + m[11]};
            bool ok = valid;
            int c[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                // (not grid_cell_of: f < 2^31 and then the INTEGER against the dim is another predicate where a dim above 2^24 is no f32)
                const float f = floorf((q[a] - box.lo[a]) * box.inv_cell[a]);
                const bool in = f >= 0.f && f < 2147483648.f;                       // (false for NaN)
                c[a] = in ? (int)f : 0;
                ok = ok && in && c[a] < box.dims[a];
            }
            int64_t src = 0;
            if (ok) {
                src = ((int64_t)c[0] * dy + c[1]) * dz + c[2];
                ok = labels[src] == lab;
            }
            const int n = __popcll(__ballot(ok));
            if (n && lane == 0) atomicAdd(&s_claimed[e], (unsigned int)n);
            if (ok) {
                cand |= 1ull << (1 + e);
                bool take = win < 0;
                if (densest) {
                    const float s = sigma_of[src * 4 + 3];
                    take = take || s > win_sigma || (win_sigma != win_sigma && s == s);
                    if (take) win_sigma = s;
                }
                if (take) {
                    win = 1 + e;
                    win_label = lab;
                    win_src = src;
                }
            }
        }

        if (valid) {
            out_labels[g] = (uint8_t)win_label;
            out_source[g] = (uint8_t)(win < 0 ? UNLABELLED : win);
            if (BAKED) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (win >= 0) v = cells[win_src];
                out_cells[g] = v;
            }
        }

        for (int w = 0; w <= E; ++w) {
            const int n = __popcll(__ballot(win == w));
            if (n && lane == 0) atomicAdd(&s_won[w], (unsigned int)n);
        }

        const bool multi = __popcll(cand) >= 2;
        if (__ballot(multi) != 0) {                                                 // (uniform per wave)
            for (int e = 0; e < E; ++e) {
                const bool in_e = multi && ((cand >> (1 + e)) & 1ull) != 0;
                if (__ballot(in_e) == 0) continue;
                if (in_e && (cand & 1ull)) atomicAdd(&s_hits[e * C + (int)l0], 1u);
                for (int b = 0; b < E; ++b) {
                    if (b == e) continue;
                    const int n = __popcll(__ballot(in_e && ((cand >> (1 + b)) & 1ull) != 0));
                    if (n && lane == 0) atomicAdd(&s_hits[e * C + ent.e[b].label], (unsigned int)n);
                }
            }
        }
    }

    __syncthreads();
    for (int t = threadIdx.x; t < E * C; t += BLOCK)
        if (s_hits[t]) atomicAdd(&hits[t], (unsigned long long)s_hits[t]);
    if (threadIdx.x <= E && s_won[threadIdx.x]) atomicAdd(&won[threadIdx.x], (unsigned long long)s_won[threadIdx.x]);
    if (threadIdx.x < E && s_claimed[threadIdx.x]) atomicAdd(&claimed[threadIdx.x], (unsigned long long)s_claimed[threadIdx.x]);
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int32_t dmnerf_volume_edit(const uint8_t* d_labels, const float* d_cells, const float lo[3], const float cell[3],
                                  const float inv_cell[3], const int dims[3], int C, const uint32_t keep[4],
                                  const dmnerf_volume_edit_entry* entries, int E, int rule, uint8_t* d_out_labels, float* d_out_cells,
                                  uint8_t* d_out_source, int64_t* d_won, int64_t* d_claimed, int64_t* d_hits, void* stream) {
    if (!cell || !keep) return dmn_fail(DMNERF_E_ARG, "volume_edit: null host array");
    GridBox box;
    int64_t total;
    if (int rc = dmn_grid_given("volume_edit", lo, cell, inv_cell, dims, &box, &total)) return rc;
    if (int rc = dmn_check_labels("volume_edit", C)) return rc;
    if (int rc = dmn_edit_count_given("volume_edit", E, entries)) return rc;
    if (rule != 0 && rule != 1) return dmn_fail(DMNERF_E_ARG, "volume_edit: rule %d is neither 0 (first) nor 1 (densest)", rule);
    if (rule == 1 && !d_cells) return dmn_fail(DMNERF_E_ARG, "volume_edit: rule 1 (densest) needs d_cells");
    if (!d_labels || !d_out_labels || !d_out_source || !d_won || (E > 0 && (!d_claimed || !d_hits)))      // (E == 0: two empty outputs)
        return dmn_fail(DMNERF_E_ARG, "volume_edit: null pointer");
    if ((d_cells == nullptr) != (d_out_cells == nullptr))
        return dmn_fail(DMNERF_E_ARG, "volume_edit: d_cells and d_out_cells go together");
    if (((uintptr_t)d_cells | (uintptr_t)d_out_cells) & 15) return dmn_fail(DMNERF_E_ARG, "volume_edit: cells must be 16-byte aligned");
    // no destination may overlap a source or another destination (a cell reads other cells than its own; the counts are atomics)
    const struct { const void* p; size_t n; bool written; } region[8] = {
        {d_labels, (size_t)total, false}, {d_cells, d_cells ? (size_t)total * 16 : 0, false}, {d_out_labels, (size_t)total, true},
        {d_out_cells, d_out_cells ? (size_t)total * 16 : 0, true}, {d_out_source, (size_t)total, true},
        {d_won, (size_t)(1 + E) * 8, true}, {d_claimed, (size_t)E * 8, true}, {d_hits, (size_t)E * C * 8, true}};
    for (int a = 0; a < 8; ++a)
        for (int b = a + 1; b < 8; ++b)
            if ((region[a].written || region[b].written) && region[a].n && region[b].n &&
                overlap(region[a].p, region[a].n, region[b].p, region[b].n))
                return dmn_fail(DMNERF_E_ARG, "volume_edit: a destination overlaps a source or another destination (arguments %d and %d)", a, b);
    EditEntries ent = {};
    if (int rc = dmn_edit_entries_given("volume_edit", entries, E, C, ent.e)) return rc;
    LabelMask128 k, gone = {{0u, 0u, 0u, 0u}};
    for (int q = 0; q < 4; ++q) k.w[q] = keep[q];
    for (int e = 0; e < E; ++e)
        if (ent.e[e].kind != KIND_COPY) gone.w[ent.e[e].label >> 5] |= 1u << (ent.e[e].label & 31);
    const int n_init = E * C > E + 1 ? E * C : E + 1;
    hipLaunchKernelGGL(volume_edit_init_kernel, dim3((unsigned)((n_init + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, E, C,
                       reinterpret_cast<unsigned long long*>(d_won), reinterpret_cast<unsigned long long*>(d_claimed),
                       reinterpret_cast<unsigned long long*>(d_hits));
    const int64_t nb = (total + BLOCK - 1) / BLOCK;
    const dim3 grid((unsigned)(nb < MAX_BLOCKS ? nb : MAX_BLOCKS));
    unsigned long long* w = reinterpret_cast<unsigned long long*>(d_won);
    unsigned long long* cl = reinterpret_cast<unsigned long long*>(d_claimed);
    unsigned long long* h = reinterpret_cast<unsigned long long*>(d_hits);
    if (d_cells)
        hipLaunchKernelGGL(volume_edit_kernel<true>, grid, dim3(BLOCK), 0, (hipStream_t)stream, d_labels,
                           reinterpret_cast<const uint4*>(d_cells), box, C, k, gone, ent, E, rule, d_out_labels,
                           reinterpret_cast<uint4*>(d_out_cells), d_out_source, w, cl, h);
    else
        hipLaunchKernelGGL(volume_edit_kernel<false>, grid, dim3(BLOCK), 0, (hipStream_t)stream, d_labels,
                           static_cast<const uint4*>(nullptr), box, C, k, gone, ent, E, rule, d_out_labels, static_cast<uint4*>(nullptr),
                           d_out_source, w, cl, h);
    return dmn_check_launch("volume_edit");
}
