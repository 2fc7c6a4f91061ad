// common.h -- what the host side of every translation unit shares: error plumbing, the launch of kernels with large dynamic
// LDS, the checks of a grid volume and of an edit list, and the two ends of a ray / sample MLP entry: its preamble (range
// checks, the empty batch, the null-pointer test) and its tail (the grid of the MLP kernels and the launch of the kernel
// instantiation that the network's logit count selects).  An entry is: preamble, fill the kernel's argument struct, tail.
#pragma once
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "../../include/dmnerf_hip.h"
#include "grid_volume.h"

// Records a printf-style message for dmnerf_last_error() and returns `code`.
int dmn_fail(int code, const char* fmt, ...);
// After a kernel launch: 0, or DMNERF_E_LAUNCH with hipGetErrorString recorded.
int dmn_check_launch(const char* what);
// A HIP runtime call that FAILED with `e` (hipFuncSetAttribute, hipMemsetAsync ...): always an error return.
// (dmn_check_launch() is the wrong tool there: it reports hipGetLastError(), which may have nothing to say, and the
// caller would return DMNERF_OK without having launched anything.)
int dmn_fail_hip(hipError_t e, const char* what);

// hipFuncSetAttribute (large dynamic LDS) is per function AND per device: one bit per device ordinal in a mask,
// so a process that drives several GPUs configures each of them, and two host threads racing here both succeed.
struct DmnOncePerDevice {
    std::atomic<unsigned long long> mask{0};
    template <class F>
    hipError_t run(F&& f) {
        int dev = 0;
        if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
        const unsigned long long bit = 1ull << (dev & 63);
        if (mask.load(std::memory_order_acquire) & bit) return hipSuccess;
        if (hipError_t e = f(); e != hipSuccess) return e;
        mask.fetch_or(bit, std::memory_order_release);
        return hipSuccess;
    }
};

// ---- launching a kernel whose dynamic LDS exceeds the 64 KiB default -----------------------------------------------
// Raises Kernel's limit to MaxLdsBytes, once per device.  The flag belongs to the pair (kernel, limit) and not to a call
// site: entries that launch the same kernel share it, whichever of them runs first, and one kernel configured with two
// limits gets two flags.  A failure is reported as "<what><step>: <HIP's text>".
template <auto Kernel, int MaxLdsBytes>
int dmn_allow_lds(const char* what, const char* step = ": hipFuncSetAttribute") {
    static DmnOncePerDevice once;
    if (hipError_t e = once.run([] { return hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MaxLdsBytes); });
        e != hipSuccess) {
        char text[160];
        snprintf(text, sizeof(text), "%s%s", what, step);
        return dmn_fail_hip(e, text);
    }
    return DMNERF_OK;
}
// ... and launches it with lds_bytes <= MaxLdsBytes of them: 0, or the error of either step under the entry's name `what`.
template <auto Kernel, int MaxLdsBytes, class... Args>
int dmn_launch_lds(const char* what, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args&... args) {
    if (int rc = dmn_allow_lds<Kernel, MaxLdsBytes>(what)) return rc;
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, stream, args...);
    return dmn_check_launch(what);
}

// ---- argument checks of the entries that take a network (ins_num) and a batch of rays or samples --------------------
inline bool dmn_ins_num_ok(int ins_num) { return ins_num >= 1 && ins_num + 1 <= DMNERF_MAX_LOGITS; }
inline int dmn_check_ins_num(const char* who, int ins_num) {
    return dmn_ins_num_ok(ins_num) ? DMNERF_OK : dmn_fail(DMNERF_E_ARG, "%s: ins_num %d unsupported", who, ins_num);
}
// ins_num, then N rays of S samples, then (sel: the entries over an int32 sample selection) N * S < 2^31.
inline int dmn_check_rays(const char* who, int ins_num, int64_t N, int S, bool sel = false) {
    if (int rc = dmn_check_ins_num(who, ins_num)) return rc;
    if (N < 0 || S < 1) return dmn_fail(DMNERF_E_ARG, "%s: bad N=%lld S=%d", who, (long long)N, S);
    if (sel && N * S >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "%s: %lld samples do not fit the int32 selection", who, (long long)(N * S));
    return DMNERF_OK;
}
// What follows an entry's range check: an empty batch (n == 0) is legal and its pointers are not looked at; otherwise every
// pointer of `ptrs` is required.  False: the entry returns *rc (DMNERF_OK, or "<who>: null pointer").  True: it goes on.
inline bool dmn_batch_given(int* rc, const char* who, int64_t n, std::initializer_list<const void*> ptrs) {
    *rc = DMNERF_OK;
    if (n == 0) return false;
    for (const void* p : ptrs)
        if (!p) return *rc = dmn_fail(DMNERF_E_ARG, "%s: null pointer", who), false;
    return true;
}
// The whole preamble of an entry on N rays of S samples: dmn_check_rays, then dmn_batch_given.
inline bool dmn_rays_given(int* rc, const char* who, int ins_num, int64_t N, int S, bool sel, std::initializer_list<const void*> ptrs) {
    return !(*rc = dmn_check_rays(who, ins_num, N, S, sel)) && dmn_batch_given(rc, who, N, ptrs);
}
// ---- argument checks of the entries that take a grid volume (grid_volume.h) or a list of volume edits ----------------
// Every refusal is "<who>: ..." in the entry's name.  The label count of a volume: 1 .. DMNERF_MAX_LOGITS.
inline int dmn_check_labels(const char* who, int C) {
    return C >= 1 && C <= DMNERF_MAX_LOGITS ? DMNERF_OK : dmn_fail(DMNERF_E_ARG, "%s: C=%d outside 1..%d", who, C, DMNERF_MAX_LOGITS);
}
// The two checks of dims, apart for the entries that check something else in between: every dim >= 1 ...
inline int dmn_grid_dims(const char* who, const int dims[3]) {
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return dmn_fail(DMNERF_E_ARG, "%s: bad dims %d x %d x %d", who, dims[0], dims[1], dims[2]);
    return DMNERF_OK;
}
// ... and fewer than 2^31 cells (a cell index is an int32 on the device); -> *total.
inline int dmn_grid_cells(const char* who, const int dims[3], int64_t* total) {
    *total = (int64_t)dims[0] * dims[1] * dims[2];
    if (*total >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "%s: %lld cells do not fit int32", who, (long long)*total);
    return DMNERF_OK;
}
// A box given as host arrays: none of them null (cell may be, for an entry that takes none: the box then carries 0), dims, cells, and
// the kernel argument filled in.
inline int dmn_grid_given(const char* who, const float* lo, const float* cell, const float* inv_cell, const int* dims, GridBox* box, int64_t* total) {
    if (!lo || !inv_cell || !dims) return dmn_fail(DMNERF_E_ARG, "%s: null host array", who);
    if (int rc = dmn_grid_dims(who, dims)) return rc;
    if (int rc = dmn_grid_cells(who, dims, total)) return rc;
    for (int a = 0; a < 3; ++a) {
        box->lo[a] = lo[a];
        box->cell[a] = cell ? cell[a] : 0.f;
        box->inv_cell[a] = inv_cell[a];
        box->dims[a] = dims[a];
    }
    return DMNERF_OK;
}
// A list of E volume edits: its length (entries == NULL with E > 0 is refused where need_entries) ...
inline int dmn_edit_count_given(const char* who, int E, const dmnerf_volume_edit_entry* entries, bool need_entries = true) {
    if (E < 0 || E > DMNERF_VOLUME_EDIT_MAX) return dmn_fail(DMNERF_E_ARG, "%s: E=%d outside 0..%d", who, E, DMNERF_VOLUME_EDIT_MAX);
    if (need_entries && E > 0 && !entries) return dmn_fail(DMNERF_E_ARG, "%s: null entries", who);
    return DMNERF_OK;
}
// ... and, entry by entry, kind 0..2 and label in [0, C); out[0 .. E) = the entries (the kernel argument).
inline int dmn_edit_entries_given(const char* who, const dmnerf_volume_edit_entry* entries, int E, int C, dmnerf_volume_edit_entry* out) {
    for (int e = 0; e < E; ++e) {
        const dmnerf_volume_edit_entry& s = entries[e];
        if (s.kind < 0 || s.kind > 2) return dmn_fail(DMNERF_E_ARG, "%s: entry %d has kind %d (0 move, 1 copy, 2 remove)", who, e, s.kind);
        if (s.label < 0 || s.label >= C) return dmn_fail(DMNERF_E_ARG, "%s: entry %d has label %d outside [0, %d)", who, e, s.label, C);
        out[e] = s;
    }
    return DMNERF_OK;
}
// skip.hip: passes 2 and 3 of a selection by byte (the scan of the per-block counts, the scatter, *d_count, the running sums)
void dmn_select_finish(const uint8_t* d_byte, int none, int64_t M, int* d_work, int* d_sel, int* d_count, int64_t* d_totals, hipStream_t st);

// Grid of the MLP kernels: workgroups of 4 waves x 32 samples for M samples, refused beyond one launch's 2^31 - 1
// (brief: the wording of the split-operand entries).
inline int dmn_mlp_grid(const char* who, int64_t M, unsigned* grid, bool brief = false) {
    const int64_t g = ((M + 31) / 32 + 3) / 4;
    if (g > 0x7fffffffLL)
        return brief ? dmn_fail(DMNERF_E_ARG, "%s: too many samples", who)
                     : dmn_fail(DMNERF_E_ARG, "%s: %lld samples is too many for one launch", who, (long long)M);
    *grid = (unsigned)g;
    return DMNERF_OK;
}
// The tail of an MLP entry: the grid for a.M samples, then the launch of Kernel with LdsBytes of dynamic LDS, both under the
// entry's name `what`.
template <auto Kernel, int LdsBytes, class Args>
int dmn_launch_mlp(const char* what, bool brief, const Args& a, hipStream_t stream) {
    unsigned grid;
    if (int rc = dmn_mlp_grid(what, a.M, &grid, brief)) return rc;
    return dmn_launch_lds<Kernel, LdsBytes>(what, grid, 256, LdsBytes, stream, a);
}
// The same for a kernel template with one instantiation per count obx of 32-logit blocks: Family<obx>::kernel, obx = 1, 2, 4
// and (WITH3) 3.  The grid is refused under the name `grid_who`, which several entries share; C, the logit count, is for the
// refusal of any other obx.
template <template <int> class Family, int LdsBytes, bool WITH3, class Args>
int dmn_launch_mlp_obx(const char* what, const char* grid_who, bool brief, int obx, int C, const Args& a, hipStream_t stream) {
    unsigned grid;
    if (int rc = dmn_mlp_grid(grid_who, a.M, &grid, brief)) return rc;
    switch (obx) {
        case 1: return dmn_launch_lds<Family<1>::kernel, LdsBytes>(what, grid, 256, LdsBytes, stream, a);
        case 2: return dmn_launch_lds<Family<2>::kernel, LdsBytes>(what, grid, 256, LdsBytes, stream, a);
        case 3: if constexpr (WITH3) return dmn_launch_lds<Family<3>::kernel, LdsBytes>(what, grid, 256, LdsBytes, stream, a); else break;
        case 4: return dmn_launch_lds<Family<4>::kernel, LdsBytes>(what, grid, 256, LdsBytes, stream, a);
    }
    return dmn_fail(DMNERF_E_ARG, "%s: unsupported logit count C=%d", what, C);
}
