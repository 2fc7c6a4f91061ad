// api.hip -- error plumbing and the whole-path entry point of the C ABI.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/dmnerf_hip.h"
#include "common.h"

namespace {
thread_local char g_err[512] = "";
}

int dmn_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int dmn_check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return DMNERF_OK;
    return dmn_fail(DMNERF_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

int dmn_fail_hip(hipError_t e, const char* what) {
    (void)hipGetLastError();                                 // clear the sticky error: it is being reported here
    return dmn_fail(DMNERF_E_LAUNCH, "%s: %s", what, hipGetErrorString(e != hipSuccess ? e : hipErrorUnknown));
}

extern "C" int dmnerf_abi_version(void) { return DMNERF_ABI_VERSION; }
extern "C" const char* dmnerf_last_error(void) { return g_err; }

extern "C" int dmnerf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int dmn_skip_set_int(int* d_p, int v, hipStream_t stream);      // skip.hip

// ---- the stages that the three inference chains below share, each written once and enqueued on `stream`, no sync ----------------
// (A: dmnerf_render_args or dmnerf_render_fine_args, which name their common fields alike)
namespace {

typedef int (*RaysNet)(const float*, int, const float*, const float*, const float*, int64_t, int, float*, void*);
typedef int (*RaysSelNet)(const float*, int, const float*, const float*, const float*, int64_t, int, const int*, const int*, float*, void*);

// fused_heads -> the network on rays: 3 the f16x2 blob, 2 the split-bf16 blob, any other non-zero the fused-heads blob, 0 the plain one
RaysNet raw_net(int fused_heads) {
    return fused_heads == 3 ? dmnerf_mlp_fwd_rays_f16 : fused_heads == 2 ? dmnerf_mlp_fwd_rays_split : fused_heads ? dmnerf_mlp_fwd_rays_fused : dmnerf_mlp_fwd_rays;
}
// ... as far as the density (fused_heads 3, f16x2: of the f16 DENSITY blob, another format than the f16 blob), dense and over a selection
RaysNet density_net(int fused_heads) { return fused_heads == 3 ? dmnerf_mlp_fwd_rays_density_f16 : dmnerf_mlp_fwd_rays_density; }
RaysSelNet density_sel_net(int fused_heads) { return fused_heads == 3 ? dmnerf_mlp_fwd_rays_density_f16_sel : dmnerf_mlp_fwd_rays_density_sel; }
// ... and the whole network over a selection (fused_heads 0, 1 or 3)
int raw_sel_net(int fused_heads, const float* d_blob, int ins_num, const float* d_rays_o, const float* d_rays_d, const float* d_z, int64_t N, int S,
                const int* d_sel, const int* d_count, float* d_raw, void* stream) {
    return fused_heads == 3 ? dmnerf_mlp_fwd_rays_f16_sel(d_blob, ins_num, d_rays_o, d_rays_d, d_z, N, S, d_sel, d_count, d_raw, stream)
                            : dmnerf_mlp_fwd_rays_sel(d_blob, ins_num, fused_heads, d_rays_o, d_rays_d, d_z, N, S, d_sel, d_count, d_raw, stream);
}

// stratified jitter (render.py:40-47) or pass-through copy of the coarse grid; copy_what: "<entry>: z copy"
template <class A>
int z_coarse(const A* a, const char* copy_what, void* stream) {
    if (a->d_t_rand) return dmnerf_stratify(a->d_z_in, a->d_t_rand, a->N, a->S, a->d_z_coarse, stream);
    if (a->d_z_coarse != a->d_z_in)
        if (hipError_t e = hipMemcpyAsync(a->d_z_coarse, a->d_z_in, sizeof(float) * a->N * a->S, hipMemcpyDeviceToDevice, (hipStream_t)stream); e != hipSuccess)
            return dmn_fail_hip(e, copy_what);
    return DMNERF_OK;
}

// hierarchical resampling + merge (render.py:66-70) from the coarse weights in d_weights_ws
template <class A>
int resample(const A* a, void* stream) {
    return dmnerf_importance_resample(a->d_z_coarse, a->d_weights_ws, a->d_u, a->u_row_stride, a->N, a->S, a->n_imp, a->d_z_fine, nullptr, stream);
}

// fine network, between the caller's two events, + compositing (render.py:71-86); d_sel: over that selection of *d_count samples
template <class A>
int fine_level(const A* a, const int* d_sel, const int* d_count, void* stream) {
    const int SF = a->S + a->n_imp;
    if (a->ev_fine_mlp_begin) (void)hipEventRecord((hipEvent_t)a->ev_fine_mlp_begin, (hipStream_t)stream);
    const int rc = d_sel ? raw_sel_net(a->fused_heads, a->d_blob_fine, a->ins_num, a->d_rays_o, a->d_rays_d, a->d_z_fine, a->N, SF, d_sel, d_count, a->d_raw_fine, stream)
                         : raw_net(a->fused_heads)(a->d_blob_fine, a->ins_num, a->d_rays_o, a->d_rays_d, a->d_z_fine, a->N, SF, a->d_raw_fine, stream);
    if (rc) return rc;
    if (a->ev_fine_mlp_end) (void)hipEventRecord((hipEvent_t)a->ev_fine_mlp_end, (hipStream_t)stream);
    return dmnerf_composite_fwd(a->d_raw_fine, a->d_z_fine, a->d_rays_d, a->N, SF, a->ins_num + 1, a->d_rgb_fine, a->d_weights_ws,
                                a->d_depth_fine, a->d_ins_fine, stream);
}

}  // namespace

// dm_nerf inference (networks/render.py:31-96): every stage enqueued on one stream, no sync.
// (fused_heads is not validated: see raw_net)
extern "C" int dmnerf_render_rays_fwd(const dmnerf_render_args* a, void* stream) {
    if (!a) return dmn_fail(DMNERF_E_ARG, "render_rays_fwd: null args");
    if (a->N == 0 && a->S >= 3 && a->n_imp >= 1) return DMNERF_OK;      // an empty chunk: its buffers may be null
    if (!a->d_blob_coarse || !a->d_blob_fine || !a->d_rays_o || !a->d_rays_d || !a->d_z_in || !a->d_u ||
        !a->d_z_coarse || !a->d_raw_coarse || !a->d_rgb_coarse || !a->d_depth_coarse || !a->d_ins_coarse ||
        !a->d_z_fine || !a->d_raw_fine || !a->d_rgb_fine || !a->d_depth_fine || !a->d_ins_fine || !a->d_weights_ws)
        return dmn_fail(DMNERF_E_ARG, "render_rays_fwd: null pointer in args");
    const int64_t N = a->N;
    const int S = a->S;
    if (N < 0 || S < 3 || a->n_imp < 1) return dmn_fail(DMNERF_E_ARG, "render_rays_fwd: bad N=%lld S=%d n_imp=%d", (long long)N, S, a->n_imp);
    int rc;
    if ((rc = z_coarse(a, "render_rays_fwd: z copy", stream))) return rc;
    // coarse network + compositing (render.py:49-63)
    if ((rc = raw_net(a->fused_heads)(a->d_blob_coarse, a->ins_num, a->d_rays_o, a->d_rays_d, a->d_z_coarse, N, S, a->d_raw_coarse, stream))) return rc;
    if ((rc = dmnerf_composite_fwd(a->d_raw_coarse, a->d_z_coarse, a->d_rays_d, N, S, a->ins_num + 1, a->d_rgb_coarse, a->d_weights_ws,
                                   a->d_depth_coarse, a->d_ins_coarse, stream))) return rc;
    if ((rc = resample(a, stream))) return rc;
    return fine_level(a, nullptr, nullptr, stream);
}

// The same render for a caller that keeps the FINE outputs only (render_test, networks/tester.py:71-77): the coarse level is
// evaluated as far as its compositing weights -- the trunk and density_linear of the coarse network, no heads, no raw_coarse, no
// coarse maps.  Everything the fine level sees (the weights, hence z_vals_fine) is bit-identical to dmnerf_render_rays_fwd.
extern "C" int dmnerf_render_rays_fwd_fine(const dmnerf_render_fine_args* a, void* stream) {
    if (!a) return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine: null args");
    if (a->fused_heads != 0 && a->fused_heads != 1 && a->fused_heads != 3)
        return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine: fused_heads %d unsupported (the split-operand blobs go through dmnerf_render_rays_fwd)", a->fused_heads);
    if (a->N == 0 && a->S >= 3 && a->n_imp >= 1) return DMNERF_OK;      // an empty chunk: its buffers may be null
    if (!a->d_blob_coarse || !a->d_blob_fine || !a->d_rays_o || !a->d_rays_d || !a->d_z_in || !a->d_u || !a->d_z_coarse ||
        !a->d_sigma_ws || !a->d_weights_ws || !a->d_z_fine || !a->d_raw_fine || !a->d_rgb_fine || !a->d_depth_fine || !a->d_ins_fine)
        return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine: null pointer in args");
    const int64_t N = a->N;
    const int S = a->S;
    if (N < 0 || S < 3 || a->n_imp < 1) return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine: bad N=%lld S=%d n_imp=%d", (long long)N, S, a->n_imp);
    // f16x2: the coarse blob is the f16 DENSITY blob, another format than the fine one -- one buffer cannot be both (a caller that
    // passes the model's f16 blob twice would get the density of the wrong weight groups, silently)
    if (a->fused_heads == 3 && a->d_blob_coarse == a->d_blob_fine)
        return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine: fused_heads 3 wants the f16 density blob as d_blob_coarse, got d_blob_fine twice");
    int rc;
    if ((rc = z_coarse(a, "render_rays_fwd_fine: z copy", stream))) return rc;
    // coarse network as far as the density (render.py:49-61), its weights (:6-20)
    if ((rc = density_net(a->fused_heads)(a->d_blob_coarse, a->ins_num, a->d_rays_o, a->d_rays_d, a->d_z_coarse, N, S, a->d_sigma_ws, stream))) return rc;
    if ((rc = dmnerf_weights_from_sigma(a->d_sigma_ws, a->d_z_coarse, a->d_rays_d, N, S, a->d_weights_ws, stream))) return rc;
    if ((rc = resample(a, stream))) return rc;
    return fine_level(a, nullptr, nullptr, stream);
}

// dmnerf_render_rays_fwd_fine through an occupancy bit grid (csrc/skip.hip): the networks run on the marked samples only, the other
// rows of sigma / raw_fine are zero.  A zero row is exactly neutral downstream -- alpha = 1 - exp(-0) = 0, weight 0, every term
// 0 * x -- so the result is the dense render with those rows masked.  The sample counts never leave the device.
extern "C" int dmnerf_render_rays_fwd_fine_skip(const dmnerf_render_fine_skip_args* k, void* stream) {
    if (!k) return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine_skip: null args");
    const dmnerf_render_fine_args* a = &k->fine;
    if (a->fused_heads != 0 && a->fused_heads != 1 && a->fused_heads != 3)
        return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine_skip: fused_heads %d unsupported (no split-operand kernels over a selection)", a->fused_heads);
    if (k->levels & ~(DMNERF_SKIP_LEVEL_COARSE | DMNERF_SKIP_LEVEL_FINE)) return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine_skip: bad levels mask %d", k->levels);
    const int64_t N = a->N;
    const int S = a->S, SF = a->S + a->n_imp, C = a->ins_num + 1;
    if (N < 0 || S < 3 || a->n_imp < 1) return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine_skip: bad N=%lld S=%d n_imp=%d", (long long)N, S, a->n_imp);
    if (N * SF >= (1LL << 31)) return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine_skip: %lld samples do not fit the int32 selection", (long long)(N * SF));
    if (!k->d_n_eval) return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine_skip: null pointer in args");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (N == 0) {                                                        // an empty chunk: its buffers may be null
        if ((rc = dmn_skip_set_int(k->d_n_eval, 0, st))) return rc;
        return dmn_skip_set_int(k->d_n_eval + 1, 0, st);
    }
    if (!a->d_blob_coarse || !a->d_blob_fine || !a->d_rays_o || !a->d_rays_d || !a->d_z_in || !a->d_u || !a->d_z_coarse ||
        !a->d_sigma_ws || !a->d_weights_ws || !a->d_z_fine || !a->d_raw_fine || !a->d_rgb_fine || !a->d_depth_fine || !a->d_ins_fine ||
        !k->d_sel || !k->d_flag || !k->d_select_ws || !k->grid.d_bits)
        return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine_skip: null pointer in args");
    if (a->fused_heads == 3 && a->d_blob_coarse == a->d_blob_fine)       // (as in dmnerf_render_rays_fwd_fine: two formats, one buffer)
        return dmn_fail(DMNERF_E_ARG, "render_rays_fwd_fine_skip: fused_heads 3 wants the f16 density blob as d_blob_coarse, got d_blob_fine twice");
    if ((rc = z_coarse(a, "render_rays_fwd_fine_skip: z copy", stream))) return rc;
    // coarse level: the density at the marked samples, 0 elsewhere (render.py:49-61), its weights (:6-20)
    if (k->levels & DMNERF_SKIP_LEVEL_COARSE) {
        if ((rc = dmnerf_skip_select(&k->grid, a->d_rays_o, a->d_rays_d, a->d_z_coarse, N, S, k->d_flag, k->d_sel, k->d_n_eval, k->d_select_ws, stream))) return rc;
        if (hipError_t e = hipMemsetAsync(a->d_sigma_ws, 0, sizeof(float) * N * S, st); e != hipSuccess) return dmn_fail_hip(e, "render_rays_fwd_fine_skip: sigma fill");
        if ((rc = density_sel_net(a->fused_heads)(a->d_blob_coarse, a->ins_num, a->d_rays_o, a->d_rays_d, a->d_z_coarse, N, S, k->d_sel, k->d_n_eval, a->d_sigma_ws, stream))) return rc;
    } else {
        if ((rc = dmn_skip_set_int(k->d_n_eval, (int)(N * S), st))) return rc;
        if ((rc = density_net(a->fused_heads)(a->d_blob_coarse, a->ins_num, a->d_rays_o, a->d_rays_d, a->d_z_coarse, N, S, a->d_sigma_ws, stream))) return rc;
    }
    if ((rc = dmnerf_weights_from_sigma(a->d_sigma_ws, a->d_z_coarse, a->d_rays_d, N, S, a->d_weights_ws, stream))) return rc;
    if ((rc = resample(a, stream))) return rc;
    // fine level: the network at the marked samples, zero rows elsewhere
    if (k->levels & DMNERF_SKIP_LEVEL_FINE) {
        if ((rc = dmnerf_skip_select(&k->grid, a->d_rays_o, a->d_rays_d, a->d_z_fine, N, SF, k->d_flag, k->d_sel, k->d_n_eval + 1, k->d_select_ws, stream))) return rc;
        if (hipError_t e = hipMemsetAsync(a->d_raw_fine, 0, sizeof(float) * N * SF * (4 + C), st); e != hipSuccess) return dmn_fail_hip(e, "render_rays_fwd_fine_skip: raw fill");
        return fine_level(a, k->d_sel, k->d_n_eval + 1, stream);
    }
    if ((rc = dmn_skip_set_int(k->d_n_eval + 1, (int)(N * SF), st))) return rc;
    return fine_level(a, nullptr, nullptr, stream);
}
