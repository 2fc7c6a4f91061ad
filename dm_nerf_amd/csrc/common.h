// common.h -- what the host side of every translation unit shares: error plumbing, the launch of kernels with large dynamic
// LDS, the argument checks of the ray / sample entries and the grid of the MLP kernels.
#pragma once
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

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
// ins_num, then N rays of S samples, then (sel: the entries over an int32 sample selection) N * S < 2^31.  The entry goes
// on with `if (N == 0) return DMNERF_OK;` and its own null-pointer test.
inline int dmn_check_rays(const char* who, int ins_num, int64_t N, int S, bool sel = false) {
    if (int rc = dmn_check_ins_num(who, ins_num)) return rc;
    if (N < 0 || S < 1) return dmn_fail(DMNERF_E_ARG, "%s: bad N=%lld S=%d", who, (long long)N, S);
    if (sel && N * S >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "%s: %lld samples do not fit the int32 selection", who, (long long)(N * S));
    return DMNERF_OK;
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
