// mlp_fwd_sel_impl.h -- the full network over a selection of the samples: kernel and launch (see mlp_fwd_sparse.hip).
// One translation unit per blob form, as for the dense kernels: the plain and the fused-heads instantiation want different register
// classes for the inline-asm tile reads (Makefile: RC_*).
#pragma once
#include "mlp_fwd_impl.h"

namespace {

struct MlpSelArgs : MlpArgs {
    const int* sel;        // [count] sample indices m = n * S + s, any order
    const int* count;      // device scalar, 0 <= count <= M
};

template <int OBI, bool FUSED>
__global__ __launch_bounds__(256) void mlp_fwd_sel_kernel(const MlpSelArgs a) {
    mlp_fwd_body<OBI, false, false, FUSED, true>(a);
}

template <bool FUSED>
int launch_sel(const MlpSelArgs& a, hipStream_t stream) {
    const int64_t grid = ((a.M + 31) / 32 + 3) / 4;
    dim3 g((unsigned)grid), b(256);
    constexpr size_t lds_bytes = (size_t)(LDS_FLOATS + PARK_FLOATS) * sizeof(float);
#define DMN_LAUNCH_SEL(OBI_)                                                                                                     \
    {                                                                                                                            \
        static DmnOncePerDevice once;                                                                                            \
        if (hipError_t e_ = once.run([] { return hipFuncSetAttribute((const void*)(mlp_fwd_sel_kernel<OBI_, FUSED>),             \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); }); e_ != hipSuccess) \
            return dmn_fail_hip(e_, "mlp_fwd_rays_sel: hipFuncSetAttribute");                                                    \
        hipLaunchKernelGGL((mlp_fwd_sel_kernel<OBI_, FUSED>), g, b, lds_bytes, stream, a);                                       \
    }
    switch (a.L.OBI) {
        case 1: DMN_LAUNCH_SEL(1) break;
        case 2: DMN_LAUNCH_SEL(2) break;
        case 3: DMN_LAUNCH_SEL(3) break;
        case 4: DMN_LAUNCH_SEL(4) break;
        default: return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_sel: unsupported logit count C=%d", a.L.C);
    }
#undef DMN_LAUNCH_SEL
    return dmn_check_launch("mlp_fwd_rays_sel");
}

}  // namespace
