// common.h -- what the host side of every translation unit shares: error plumbing, the launch of kernels with large dynamic
// LDS, and the two ends of a ray / sample MLP entry: its preamble (range checks, the empty batch, the null-pointer test) and its
// tail (the grid of the MLP kernels and the launch of the kernel instantiation that the network's logit count selects).  An
// entry is: preamble, fill the kernel's argument struct, tail.
#pragma once
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "../../include/dmnerf_hip.h"

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
