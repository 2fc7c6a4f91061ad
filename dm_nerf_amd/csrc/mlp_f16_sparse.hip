// mlp_f16_sparse.hip -- the opt-in split-f16 ("f16x2") network over a SELECTION of the samples (csrc/skip.hip makes one).
//
// The body of mlp_f16_kernel (mlp_f16_body.inc) with SEL: the same f16_pass calls on the same tiles in the same order,
// and a sample is one B-operand column of every MFMA, so a selected row is bit-identical to the same row of
// dmnerf_mlp_fwd_rays_f16 whichever other samples share its wave.  Sample index, batch size and early exit are those of
// dmnerf_mlp_fwd_rays_sel (mlp_fwd_sparse.hip): sel [count] is read at indices < count only, *d_count on the device.
#include "mlp_f16_impl.h"

namespace {

template <int OBX>
__global__ __launch_bounds__(256) void mlp_f16_sel_kernel(const F16Args a) {
    constexpr bool SAVE = false, SEL = true, DENS = false;
#include "mlp_f16_body.inc"
}

}  // namespace

extern "C" int dmnerf_mlp_fwd_rays_f16_sel(const float* d_blob_f16, int ins_num, const float* d_rays_o, const float* d_rays_d,
                                           const float* d_z, int64_t N, int S, const int* d_sel, const int* d_count, float* d_raw,
                                           void* stream) {
    if (ins_num < 1 || ins_num + 1 > DMNERF_MAX_LOGITS) return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_f16_sel: ins_num %d unsupported", ins_num);
    if (N < 0 || S < 1) return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_f16_sel: bad N=%lld S=%d", (long long)N, S);
    if (N * S >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_f16_sel: %lld samples do not fit the int32 selection", (long long)(N * S));
    if (N == 0) return DMNERF_OK;
    if (!d_blob_f16 || !d_rays_o || !d_rays_d || !d_z || !d_sel || !d_count || !d_raw) return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_f16_sel: null pointer");
    F16Args a{};
    a.blob = d_blob_f16; a.S = make_f16_layout(ins_num);
    a.rays_o = d_rays_o; a.rays_d = d_rays_d; a.z = d_z; a.raw = d_raw; a.M = N * S; a.Sr = S;
    a.sel = d_sel; a.count = d_count;
#ifdef DMN_F16_TRACE
    a.trace = nullptr;
#endif
    const int64_t grid = ((a.M + 31) / 32 + 3) / 4;                        // the worst case count == N * S (< 2^31 samples: fits)
    constexpr size_t lds_bytes = (size_t)F16_LDS_FLOATS * sizeof(float);
#define DMN_LAUNCH(OBX_)                                                                                                   \
    {                                                                                                                     \
        static DmnOncePerDevice once;                                                                                 \
        if (hipError_t e_ = once.run([] { return hipFuncSetAttribute((const void*)mlp_f16_sel_kernel<OBX_>,          \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); }); e_ != hipSuccess) \
            return dmn_fail_hip(e_, "mlp_fwd_rays_f16_sel: hipFuncSetAttribute");                                   \
        hipLaunchKernelGGL(mlp_f16_sel_kernel<OBX_>, dim3((unsigned)grid), dim3(256), lds_bytes, (hipStream_t)stream, a); \
    }
    switch (a.S.OBX) {
        case 1: DMN_LAUNCH(1) break;
        case 2: DMN_LAUNCH(2) break;
        case 4: DMN_LAUNCH(4) break;
        default: return dmn_fail(DMNERF_E_ARG, "mlp_fwd_rays_f16_sel: unsupported logit count C=%d", a.S.C);
    }
#undef DMN_LAUNCH
    return dmn_check_launch("mlp_fwd_rays_f16_sel");
}
