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
    unsigned grid;                                                       // the worst case count == M (< 2^31 samples: fits)
    if (int rc = dmn_mlp_grid("mlp_fwd_rays_sel", a.M, &grid)) return rc;
    constexpr int LDS = (LDS_FLOATS + PARK_FLOATS) * sizeof(float);
    const char* what = "mlp_fwd_rays_sel";
    switch (a.L.OBI) {
        case 1: return dmn_launch_lds<mlp_fwd_sel_kernel<1, FUSED>, LDS>(what, grid, 256, LDS, stream, a);
        case 2: return dmn_launch_lds<mlp_fwd_sel_kernel<2, FUSED>, LDS>(what, grid, 256, LDS, stream, a);
        case 3: return dmn_launch_lds<mlp_fwd_sel_kernel<3, FUSED>, LDS>(what, grid, 256, LDS, stream, a);
        case 4: return dmn_launch_lds<mlp_fwd_sel_kernel<4, FUSED>, LDS>(what, grid, 256, LDS, stream, a);
        default: return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_sel: unsupported logit count C=%d", a.L.C);
    }
}

}  // namespace
