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
struct MlpFwdSel {
    template <int OBI>
    struct Family { static constexpr auto kernel = mlp_fwd_sel_kernel<OBI, FUSED>; };
};

template <bool FUSED>
int launch_sel(const MlpSelArgs& a, hipStream_t stream) {
    constexpr int LDS = (LDS_FLOATS + PARK_FLOATS) * sizeof(float);
    const char* what = "mlp_fwd_rays_sel";                               // (the grid is sized for the worst case count == M < 2^31 samples: fits)
    return dmn_launch_mlp_obx<MlpFwdSel<FUSED>::template Family, LDS, true>(what, what, false, a.L.OBI, a.L.C, a, stream);
}

}  // namespace
