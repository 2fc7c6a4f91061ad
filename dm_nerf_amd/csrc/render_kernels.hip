// render_kernels.hip -- the non-GEMM stages of the DM-NeRF render path for gfx950:
//   ray generation, depth grids + stratified jitter, inverse-CDF resampling + sorted merge,
//   positional encoding (stand-alone), and front-to-back compositing.
// All of them are tiny next to the MLP (< 0.5 % of the path's work); they are
// written for exact parity with the reference's float32 op order first:
//   * compiled with -ffp-contract=off: every a*b+c below is two roundings, like ATen's eager ops;
//   * prefix sums / products accumulate in double and round per element, which is what ATen's
//     CPU cumsum / cumprod do for float tensors;
//   * one 64-lane wave per ray; scans use wave shuffles, no atomics.
#include <hip/hip_runtime.h>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "mlp_common.h"
#include "raygen.h"

namespace {

constexpr int WAVE = 64;
constexpr int RAYS_PER_BLOCK = 4;          // one wave per ray, 256-thread blocks
// samples per ray supported by the per-ray LDS staging: the manipulation render composites 64 + 128 + 128 T samples
// for T moved objects (manipulator.py:187-189), and the exchanger takes T <= MAX_MOVE = 8 -> 1216
constexpr int MAX_S = 1280;

__device__ __forceinline__ double shfl_up_d(double v, int delta) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_up(lo, delta, WAVE);
    hi = __shfl_up(hi, delta, WAVE);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_d(double v, int src) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl(lo, src, WAVE);
    hi = __shfl(hi, src, WAVE);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_xor_d(double v, int mask) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, mask, WAVE);
    hi = __shfl_xor(hi, mask, WAVE);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_d(v, m);
    return v;
}
// inclusive scans over the 64 lanes of a wave
__device__ __forceinline__ double wave_scan_add_d(double v, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        double t = shfl_up_d(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ double wave_scan_mul_d(double v, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        double t = shfl_up_d(v, d);
        if (lane >= d) v *= t;
    }
    return v;
}

__device__ __forceinline__ void lds_sync_wave() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float sigmoidf_ref(float x) { return 1.f / (1.f + expf(-x)); }

// exp(x) of the compositing pass, rounded to float once (through double).  The device expf is good to 1 ulp; ATen's is almost
// always the correctly rounded float.  One factor (1 - alpha) hardly shows the difference, but the transmittance is a product of up
// to MAX_S of them: at S = 1280 the weights of a thin ray came out 47 ulp of the ray's largest weight from their float64 values,
// where the reference's own float32 arithmetic stays within 8 (tests/test_gpu_ray_edges.py).  The forward, the weights-only pass
// and both passes of the backward call this one function: they must form the same floats.
__device__ __forceinline__ float expf_rn(float x) { return (float)exp((double)x); }

// ------------------------------------------------------------------------------------------
// get_rays_k  (networks/helpers.py:50-61)
// ------------------------------------------------------------------------------------------
struct RaygenArgs {
    RaygenCam cam;   // raygen.h
    int W, row0;
    int64_t n;       // rays to generate
    float* rays_o;
    float* rays_d;
};

__global__ void raygen_kernel(const RaygenArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n) return;
    dmn_raygen_ray(a.cam, (int)(idx % a.W), a.row0 + (int)(idx / a.W), a.rays_o + idx * 3, a.rays_d + idx * 3);
}

// rays of selected pixels only (get_select_full, helpers.py:99-111: flat index k -> row k / W, col k % W)
__global__ void raygen_select_kernel(const RaygenArgs a, const int64_t* __restrict__ idx) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n) return;
    const int64_t k = idx[t];
    dmn_raygen_ray(a.cam, (int)(k % a.W), (int)(k / a.W), a.rays_o + t * 3, a.rays_d + t * 3);
}

// ------------------------------------------------------------------------------------------
// z_val_sample (helpers.py:114-119) and the stratified jitter (render.py:42-47)
// ------------------------------------------------------------------------------------------
__global__ void zvals_kernel(const float* __restrict__ t, float near_, float far_, int64_t total, int S,
                             float* __restrict__ z) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    z[idx] = near_ + t[idx % S] * (far_ - near_);
}

__global__ void stratify_kernel(const float* __restrict__ zin, const float* __restrict__ t_rand,
                                int64_t total, int S, float* __restrict__ zout) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int s = (int)(idx % S);
    const float zc = zin[idx];
    const float lower = s == 0 ? zc : .5f * (zc + zin[idx - 1]);        // .5 * (z[1:] + z[:-1])
    const float upper = s == S - 1 ? zc : .5f * (zin[idx + 1] + zc);
    zout[idx] = lower + (upper - lower) * t_rand[idx];
}

// ------------------------------------------------------------------------------------------
// Embedder.embed (dm_nerf.py:37-38), stand-alone
// ------------------------------------------------------------------------------------------
__global__ void embed_kernel(const float* __restrict__ x, int64_t M, int L, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (row, component)
    if (idx >= M * 3) return;
    const int64_t m = idx / 3;
    const int c = (int)(idx % 3);
    const int od = 3 + 6 * L;
    const float v = x[idx];
    float* o = out + m * od;
    o[c] = v;
    const double t = dmn::rev_of(v);                 // same shared range reduction as the fused kernel
    for (int k = 0; k < L; ++k) {
        o[3 + 6 * k + c] = dmn::sin_rev(t, k, 0);
        o[3 + 6 * k + 3 + c] = dmn::sin_rev(t, k, 1);
    }
}

// ------------------------------------------------------------------------------------------
// render_train  (networks/render.py:6-28): one wave per ray
// ------------------------------------------------------------------------------------------
// Per-ray LDS rows of the wave-per-ray kernels: dynamic shared memory, `rows` arrays of RAYS_PER_BLOCK rows of row_len(S, C)
// floats -- sized for the launch's S instead of MAX_S (at S = 192 a block of the fused backward needs 16 KiB instead of 80 KiB:
// 8 blocks per CU instead of 1; these kernels are latency-bound and live on occupancy).
__host__ __device__ inline int ray_row_len(int S, int C) {
    const int need = S > 4 + C ? S : 4 + C;              // (the backward reuses a row for its 4 + C channel coefficients)
    return (need + 63) & ~63;
}
__device__ __forceinline__ float* ray_row(float* base, int k, int wv, int SP) { return base + ((size_t)k * RAYS_PER_BLOCK + wv) * SP; }
inline size_t ray_lds_bytes(int rows, int S, int C) { return (size_t)rows * RAYS_PER_BLOCK * ray_row_len(S, C) * sizeof(float); }
constexpr int RAY_LDS_MAX = 4 * RAYS_PER_BLOCK * MAX_S * sizeof(float);                 // 80 KiB: four rows at MAX_S

// The compositing weights of one ray (render.py:6-20), one wave per ray: alpha from the density channel, the exclusive product
// scan in double, w = alpha T.  sig[s * sig_stride] = the density of sample s (raw rows: stride 4 + C; a compact sigma row: 1).
// Writes weights_row[s] and, when wl is non-null, the same value to the wave's LDS row.  Returns this lane's partial of
// sum_s w_s z_s (double), for the depth map.
__device__ __forceinline__ double ray_weights(const float* __restrict__ sig, int sig_stride, const float* __restrict__ zr, float nrm,
                                              int lane, int S, float* __restrict__ weights_row, float* wl) {
    double carry = 1.0;            // prod of (1 - alpha + 1e-10) over all earlier samples
    double depth_acc = 0.0;
    for (int base = 0; base < S; base += WAVE) {
        const int s = base + lane;
        const bool ok = s < S;
        float f = 1.f, alpha = 0.f, zc = 0.f;
        if (ok) {
            zc = zr[s];
            float dist = (s == S - 1) ? 1e10f : zr[s + 1] - zc;
            dist = dist * nrm;
            const float sg = fmaxf(sig[(int64_t)s * sig_stride], 0.f);    // F.relu
            alpha = 1.f - expf_rn(-sg * dist);
            f = (1.f - alpha) + 1e-10f;
        }
        // exclusive cumprod; ATen's CPU cumprod accumulates in double and rounds each element
        const double incl = wave_scan_mul_d((double)f, lane);
        double excl = shfl_up_d(incl, 1);
        if (lane == 0) excl = 1.0;
        const float T = (float)(carry * excl);
        const float w = alpha * T;
        if (ok) {
            if (wl) wl[s] = w;
            weights_row[s] = w;
            depth_acc += (double)(w * zc);
        }
        carry = carry * shfl_d(incl, WAVE - 1);
    }
    return depth_acc;
}

__device__ __forceinline__ float ray_dir_norm(const float* __restrict__ rays_d, int64_t n) {
    const float dx = rays_d[n * 3 + 0], dy = rays_d[n * 3 + 1], dz = rays_d[n * 3 + 2];
    return sqrtf(dx * dx + dy * dy + dz * dz);                       // torch.norm(rays_d[..., None, :], dim=-1)
}

// (one ray = one wave; returns the ray's depth, the same float in every lane)
__device__ __forceinline__ float composite_ray(
    const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rays_d, int64_t n, int lane,
    int S, int C, int n_ins, float* __restrict__ rgb_map, float* __restrict__ weights, float* __restrict__ depth_map,
    float* __restrict__ ins_map, float* wl) {
    const int ch = 4 + C;
    const float* __restrict__ rr = raw + n * (int64_t)S * ch;
    const float* __restrict__ zr = z + n * (int64_t)S;

    double depth_acc = ray_weights(rr + 3, ch, zr, ray_dir_norm(rays_d, n), lane, S, weights + n * (int64_t)S, wl);
    depth_acc = wave_sum_d(depth_acc);
    const float depth_f = (float)depth_acc;
    if (lane == 0) depth_map[n] = depth_f;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // LDS writes above are read below by other lanes
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // channel sums: products in f32 (as the reference forms weights[..., None] * rgb), accumulated in double.
    // lane = (sample group g, channel c): NG = 64 / ch groups take the samples s = g, g + NG, ... of their
    // channel, and the NG partial sums are added in group order (the double accumulator makes the result
    // independent of the order to far below one f32 ulp).
    if (ch <= 32) {
        const int NG = WAVE / ch;
        const int g = lane / ch, c = lane - g * ch;
        const bool act = g < NG && c != 3 && (c < 3 || c - 4 < n_ins);
        double acc = 0.0;
        if (act) {
            // 4 samples per trip: the four loads are issued together (the loop is latency-bound otherwise)
            for (int s = g; s < S; s += 4 * NG) {
                float v[4], wv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int su = s + u * NG;
                    const bool in = su < S;
                    v[u] = in ? rr[(int64_t)su * ch + c] : 0.f;
                    wv[u] = in ? wl[su] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc += (double)(wv[u] * (c < 3 ? sigmoidf_ref(v[u]) : v[u]));
            }
        }
        double tot = 0.0;
        for (int q = 0; q < NG; ++q) tot += shfl_d(acc, q * ch + (lane < ch ? lane : 0));
        if (lane < ch && lane != 3) {
            if (lane < 3) rgb_map[n * 3 + lane] = (float)tot;
            // sigmoid after the sum; n_ins = C-1 drops the last channel (render.py:24-26), n_ins = C keeps it (manipulator.py:101-102)
            else if (lane - 4 < n_ins) ins_map[n * (int64_t)n_ins + (lane - 4)] = sigmoidf_ref((float)tot);
        }
        return depth_f;
    }
    for (int c = lane; c < ch; c += WAVE) {
        if (c == 3) continue;
        double acc = 0.0;
        if (c < 3) {
            for (int s = 0; s < S; ++s) acc += (double)(wl[s] * sigmoidf_ref(rr[(int64_t)s * ch + c]));
            rgb_map[n * 3 + c] = (float)acc;
        } else if (c - 4 < n_ins) {
            for (int s = 0; s < S; ++s) acc += (double)(wl[s] * rr[(int64_t)s * ch + c]);
            // sigmoid after the sum; n_ins = C-1 drops the last channel (render.py:24-26), n_ins = C keeps it (manipulator.py:101-102)
            ins_map[n * (int64_t)n_ins + (c - 4)] = sigmoidf_ref((float)acc);
        }
    }
    return depth_f;
}

__global__ __launch_bounds__(WAVE* RAYS_PER_BLOCK) void composite_kernel(
    const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rays_d, int64_t N,
    int S, int C, int n_ins, float* __restrict__ rgb_map, float* __restrict__ weights, float* __restrict__ depth_map,
    float* __restrict__ ins_map) {
    extern __shared__ float ray_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (n >= N) return;
    composite_ray(raw, z, rays_d, n, lane, S, C, n_ins, rgb_map, weights, depth_map, ins_map, ray_row(ray_lds, 0, wv, ray_row_len(S, C)));
}

// The weights alone, from a compact density row: what the coarse level of an inference render hands to the resampling step
// (render.py:66-70) when nobody reads its maps.  sigma [N,S] (dmnerf_mlp_fwd_rays_density) -> weights [N,S], the floats
// composite_kernel writes for raw[..., 3] = sigma.
__global__ __launch_bounds__(WAVE* RAYS_PER_BLOCK) void weights_kernel(
    const float* __restrict__ sigma, const float* __restrict__ z, const float* __restrict__ rays_d, int64_t N, int S,
    float* __restrict__ weights) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (n >= N) return;
    (void)ray_weights(sigma + n * (int64_t)S, 1, z + n * (int64_t)S, ray_dir_norm(rays_d, n), lane, S, weights + n * (int64_t)S, nullptr);
}

// ------------------------------------------------------------------------------------------
// backward of render_train (autograd of networks/render.py:6-28): one wave per ray.
//   G_s   = dL/dw_s = sum_c g_rgb_c sigmoid(raw_sc) + g_depth z_s + g_w_s      (ins path uses detached weights, :22-23)
//   dL/da_s = G_s T_s - (sum_{t>s} G_t w_t) / (1 - a_s + 1e-10)                 (cumprod backward)
//   d raw_s3 = [raw_s3 > 0] dL/da_s dist_s exp(-relu(raw_s3) dist_s)
//   d raw_sc = g_rgb_c w_s s(1-s), c < 3;   d raw_s(4+k) = g_ins_k m_k (1 - m_k) w_s, k < C-1;  0 for the dropped channel
// ------------------------------------------------------------------------------------------
// PEN (extension, dmnerf_composite_pen_bwd): the emptiness penalizer's gradient w.r.t. raw[..., 4:] (penalizer_kernel<1> below,
// same arithmetic) is ADDED to the compositing gradient in the same pass over the ray: one kernel and one write of d raw instead
// of two kernels, two writes and an elementwise add.
struct PenBwd {
    const float* depth;          // [N] the forward's depth map (the penalizer's detached argument)
    const double* g_part;        // [>= 4] d loss / d (the ray's four partial sums): {scale_b, -, scale_m, -}, the same for every ray
    float tol, k2w, kh;
};

template <bool PEN>
__global__ __launch_bounds__(WAVE* RAYS_PER_BLOCK) void composite_bwd_kernel(
    const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rays_d,
    const float* __restrict__ ins_map, const float* __restrict__ g_rgb, const float* __restrict__ g_ins,
    const float* __restrict__ g_depth, const float* __restrict__ g_w, int64_t N, int S, int C, float* __restrict__ d_raw,
    const PenBwd pen) {
    extern __shared__ float ray_lds[];                     // 3 rows per ray (+ 1 with PEN): w, t, G (, G m_m)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (n >= N) return;
    const int SP = ray_row_len(S, C);
    const int ch = 4 + C;
    const float* __restrict__ rr = raw + n * (int64_t)S * ch;
    const float* __restrict__ zr = z + n * (int64_t)S;
    float* __restrict__ dr = d_raw + n * (int64_t)S * ch;
    float* wl = ray_row(ray_lds, 0, wv, SP);
    float* tl = ray_row(ray_lds, 1, wv, SP);
    float* gl = ray_row(ray_lds, 2, wv, SP);
    float* wml = PEN ? ray_row(ray_lds, 3, wv, SP) : nullptr;
    const float dx = rays_d[n * 3 + 0], dy = rays_d[n * 3 + 1], dz = rays_d[n * 3 + 2];
    const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float gr0 = g_rgb[n * 3 + 0], gr1 = g_rgb[n * 3 + 1], gr2 = g_rgb[n * 3 + 2];
    const float gd = g_depth ? g_depth[n] : 0.f;

    // pass 1 (front to back): recompute alpha, T, w; G_s
    double carry = 1.0;
    for (int base = 0; base < S; base += WAVE) {
        const int s = base + lane;
        const bool ok = s < S;
        float f = 1.f, alpha = 0.f, zc = 0.f;
        if (ok) {
            zc = zr[s];
            float dist = (s == S - 1) ? 1e10f : zr[s + 1] - zc;
            dist = dist * nrm;
            const float sig = fmaxf(rr[(int64_t)s * ch + 3], 0.f);
            alpha = 1.f - expf_rn(-sig * dist);
            f = (1.f - alpha) + 1e-10f;
        }
        const double incl = wave_scan_mul_d((double)f, lane);
        double excl = shfl_up_d(incl, 1);
        if (lane == 0) excl = 1.0;
        const float T = (float)(carry * excl);
        if (ok) {
            const float* r3 = rr + (int64_t)s * ch;
            float G = gr0 * sigmoidf_ref(r3[0]) + gr1 * sigmoidf_ref(r3[1]) + gr2 * sigmoidf_ref(r3[2]) + gd * zc;
            if (g_w) G += g_w[n * (int64_t)S + s];
            wl[s] = alpha * T;
            tl[s] = T;
            gl[s] = G;
        }
        carry = carry * shfl_d(incl, WAVE - 1);
    }
    lds_sync_wave();

    // pass 2 (back to front): suffix sums of G_t w_t, then d raw[..., 3]
    double after = 0.0;                                   // sum over all later chunks
    const int nchunk = (S + WAVE - 1) / WAVE;
    for (int cidx = nchunk - 1; cidx >= 0; --cidx) {
        const int s = cidx * WAVE + lane;
        const bool ok = s < S;
        const double P = ok ? (double)(gl[s] * wl[s]) : 0.0;
        const double incl = wave_scan_add_d(P, lane);
        const double total = shfl_d(incl, WAVE - 1);
        const double R = (total - incl) + after;          // sum_{t > s} G_t w_t
        if (ok) {
            const float zc = zr[s];
            float dist = (s == S - 1) ? 1e10f : zr[s + 1] - zc;
            dist = dist * nrm;
            const float rawsig = rr[(int64_t)s * ch + 3];
            const float sig = fmaxf(rawsig, 0.f);
            const float e = expf_rn(-sig * dist);         // = 1 - alpha
            const float f = ((1.f - (1.f - e))) + 1e-10f; // the forward's (1 - alpha) + 1e-10, bit for bit
            const float dLda = gl[s] * tl[s] - (float)R / f;
            dr[(int64_t)s * ch + 3] = rawsig > 0.f ? dLda * (dist * e) : 0.f;
        }
        after += total;
    }

    // (PEN) the penalizer's per-sample weights: A m_b -> the G row (dead after pass 2), G m_m -> its own row
    float sc_b = 0.f, sc_m = 0.f;
    if constexpr (PEN) {
        sc_b = (float)pen.g_part[0];
        sc_m = (float)pen.g_part[2];
        lds_sync_wave();
        float* wb = gl;
        float* wm = wml;
        const float dep = pen.depth[n];
        const float d_before = (dep - pen.tol) * nrm, d_after = (dep + pen.tol) * nrm, d_depth = dep * nrm;
        for (int s2 = lane; s2 < S; s2 += WAVE) {
            const float p = zr[s2] * nrm;
            const float dd = d_depth - p;
            const float G = expf(-(dd * dd) / pen.k2w) / pen.kh + 1e-8f;
            const float mb = p < d_before ? 1.f : 0.f;
            const float ma = p > d_after ? 1.f : 0.f;
            const float mm = 1.f - (ma + mb);
            wb[s2] = (1.f - G) * mb;
            wm[s2] = G * mm;
        }
    }
    // pass 3: channel gradients.  Per-channel coefficients once (the sample weights' LDS row is reused: t is dead), then
    // the ray's S x (4 + C) block as ONE contiguous stream, lane <-> element (coalesced 256-byte stores, every lane busy)
    lds_sync_wave();
    float* cl = tl;                                       // MAX_S >= 4 + MAX_LOGITS
    for (int c = lane; c < ch; c += WAVE) {
        float coef = 0.f;
        if (c < 3) coef = c == 0 ? gr0 : (c == 1 ? gr1 : gr2);
        else if (c >= 4 && c - 4 < C - 1) {
            const float mk = ins_map[n * (int64_t)(C - 1) + (c - 4)];
            coef = g_ins[n * (int64_t)(C - 1) + (c - 4)] * ((1.f - mk) * mk);
        }
        cl[c] = coef;
    }
    lds_sync_wave();
    int s = lane / ch, c = lane - s * ch;
    const int ds = WAVE / ch, dc = WAVE - ds * ch;
    const int total = S * ch;
    // four trips per iteration: their loads are issued together (one wave per ray: nothing else hides the memory latency)
    for (int e0 = lane; e0 < total; e0 += 4 * WAVE) {
        float x[4];
        int ss[4], cc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * WAVE;
            ss[u] = s; cc[u] = c;
            const bool need = e < total && (c < 3 || (PEN && c > 3));
            x[u] = need ? rr[e] : 0.f;
            s += ds; c += dc;
            if (c >= ch) { c -= ch; ++s; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * WAVE;
            if (e >= total || cc[u] == 3) continue;
            if (cc[u] < 3) {
                const float sg = sigmoidf_ref(x[u]);
                dr[e] = (cl[cc[u]] * wl[ss[u]]) * ((1.f - sg) * sg);
            } else {
                float v = cl[cc[u]] * wl[ss[u]];
                if constexpr (PEN) {                      // + penalizer_kernel<1>'s value for this element (autograd's add, in place)
                    const float P = sigmoidf_ref(x[u]);
                    const float q = (1.f - P) + 1e-8f;
                    const float sp = P * (1.f - P);
                    const bool last = cc[u] == ch - 1;
                    float g = (last ? -(sp / (P + 1e-8f)) : sp / q) * gl[ss[u]] * sc_b;
                    if (last) g += (sp / q) * wml[ss[u]] * sc_m;
                    v = v + g;
                }
                dr[e] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// emptiness_penalizer (networks/penalizer.py:5-55), forward partial sums and backward: one wave per ray.
//   p = z |d|;  G = exp(-(depth|d| - p)^2 / (2 deta_w^2)) / (0.4 sqrt(2 pi)) + 1e-8;  A = 1 - G
//   m_b = [p < (depth - tol)|d|], m_a = [p > (depth + tol)|d|], m_m = 1 - (m_a + m_b)
//   P = sigmoid(raw[..., 4:]);  before: BCE(P, e_last) A m_b summed / (C max(sum m_b, 1e-8))
//                              middle: -log(1 - P_last + 1e-8) G m_m summed / max(sum m_m, 1e-8)
// mode 0: out4[n] = {sum lb*w_b, sum m_b, sum lm*w_m, sum m_m} (double);  mode 1: d raw (zeros in channels 0..3)
// ------------------------------------------------------------------------------------------
struct PenArgs {
    const float* raw; const float* z; const float* depth; const float* rays_d;
    int64_t N; int S, C;
    float tol, k2w, kh;          // tolerance, 2*deta_w^2, 0.4*sqrt(2 pi) -- float32 values computed as the reference does
    double* out4;                // mode 0
    const float* scales;         // mode 1: {up / (C * max(sum m_b,1e-8)), up / max(sum m_m,1e-8)}
    float* d_raw;                // mode 1
};

template <int MODE>
__device__ __forceinline__ void penalizer_ray(const PenArgs& a, int64_t n, int lane, float dep, float* wb, float* wm) {
    const int S = a.S, C = a.C, ch = 4 + C;
    const float* __restrict__ rr = a.raw + n * (int64_t)S * ch;
    const float* __restrict__ zr = a.z + n * (int64_t)S;
    const float dx = a.rays_d[n * 3 + 0], dy = a.rays_d[n * 3 + 1], dz = a.rays_d[n * 3 + 2];
    const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float d_before = (dep - a.tol) * nrm, d_after = (dep + a.tol) * nrm, d_depth = dep * nrm;
    double n_b = 0.0, n_m = 0.0;
    for (int s = lane; s < S; s += WAVE) {
        const float p = zr[s] * nrm;
        const float dd = d_depth - p;
        const float G = expf(-(dd * dd) / a.k2w) / a.kh + 1e-8f;
        const float mb = p < d_before ? 1.f : 0.f;
        const float ma = p > d_after ? 1.f : 0.f;
        const float mm = 1.f - (ma + mb);
        wb[s] = (1.f - G) * mb;
        wm[s] = G * mm;
        n_b += mb;
        n_m += mm;
    }
    lds_sync_wave();
    float sc_b = 0.f, sc_m = 0.f;
    if (MODE == 1) { sc_b = a.scales[0]; sc_m = a.scales[1]; }
    double s_b = 0.0, s_m = 0.0;
    const unsigned total = (unsigned)S * (unsigned)ch;
    float* __restrict__ dr = MODE == 1 ? a.d_raw + n * (int64_t)S * ch : nullptr;
    // four trips per iteration, loads first (latency-bound otherwise); elements are visited in the same order as before
    for (unsigned e0 = lane; e0 < total; e0 += 4 * WAVE) {
        float x[4];
        unsigned ss[4];
        int cc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned e = e0 + u * WAVE;
            const unsigned sq = e / (unsigned)ch;
            ss[u] = sq;
            cc[u] = (int)(e - sq * (unsigned)ch) - 4;
            x[u] = (e < total && cc[u] >= 0) ? rr[e] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned e = e0 + u * WAVE;
            if (e >= total) continue;
            const int c = cc[u];
            const unsigned s = ss[u];
            if (c < 0) {
                if (MODE == 1) dr[e] = 0.f;
                continue;
            }
            const float P = sigmoidf_ref(x[u]);
            const float q = (1.f - P) + 1e-8f;                   // 1 - pred_ins + 1e-8
            const bool last = c == C - 1;
            if (MODE == 0) {
                const float lb = last ? -logf(P + 1e-8f) : -logf(q);
                s_b += (double)(lb * wb[s]);
                if (last) s_m += (double)(-logf(q) * wm[s]);
            } else {
                const float sp = P * (1.f - P);                  // sigmoid backward
                float g = (last ? -(sp / (P + 1e-8f)) : sp / q) * wb[s] * sc_b;
                if (last) g += (sp / q) * wm[s] * sc_m;
                dr[e] = g;
            }
        }
    }
    if (MODE == 0) {
        s_b = wave_sum_d(s_b); s_m = wave_sum_d(s_m); n_b = wave_sum_d(n_b); n_m = wave_sum_d(n_m);
        if (lane == 0) {
            a.out4[n * 4 + 0] = s_b; a.out4[n * 4 + 1] = n_b; a.out4[n * 4 + 2] = s_m; a.out4[n * 4 + 3] = n_m;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(WAVE* RAYS_PER_BLOCK) void penalizer_kernel(const PenArgs a) {
    extern __shared__ float ray_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (n >= a.N) return;
    const int SP = ray_row_len(a.S, a.C);
    penalizer_ray<MODE>(a, n, lane, a.depth[n], ray_row(ray_lds, 0, wv, SP), ray_row(ray_lds, 1, wv, SP));
}

// render_train + the penalizer's per-ray partial sums in ONE pass over the ray (extension, dmnerf_composite_pen_fwd): the
// penalizer's only extra input is the ray's own depth, which the compositing pass has just produced; the second walk over
// raw[..., 4:] hits the cache lines the first one loaded.
__global__ __launch_bounds__(WAVE* RAYS_PER_BLOCK) void composite_pen_kernel(
    const PenArgs a, float* __restrict__ rgb_map, float* __restrict__ weights, float* __restrict__ depth_map, float* __restrict__ ins_map) {
    extern __shared__ float ray_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (n >= a.N) return;
    const int SP = ray_row_len(a.S, a.C);
    const float dep = composite_ray(a.raw, a.z, a.rays_d, n, lane, a.S, a.C, a.C - 1, rgb_map, weights, depth_map, ins_map,
                                    ray_row(ray_lds, 0, wv, SP));
    penalizer_ray<0>(a, n, lane, dep, ray_row(ray_lds, 1, wv, SP), ray_row(ray_lds, 2, wv, SP));
}

// ------------------------------------------------------------------------------------------
// sample_pdf (helpers.py:123-155) [+ z_mid / sort-merge of render.py:66-70]: one wave per ray
// ------------------------------------------------------------------------------------------
constexpr int MAX_NB = 512;      // bins per ray
constexpr int MAX_MERGE = 1024;  // S + n_imp per ray

__device__ __forceinline__ int upper_bound_lds(const float* cdf, int nb, float u) {
    // torch.searchsorted(cdf, u, right=True): number of entries <= u
    int lo = 0, hi = nb;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float invert_cdf(const float* cdf, const float* bins, int nb, float u, int* ind_out) {
    const int ind = upper_bound_lds(cdf, nb, u);
    const int below = max(0, ind - 1);
    const int above = min(nb - 1, ind);
    const float c0 = cdf[below], c1 = cdf[above];
    const float b0 = bins[below], b1 = bins[above];
    float denom = c1 - c0;
    if (denom < 1e-5f) denom = 1.f;
    const float t = (u - c0) / denom;
    *ind_out = ind;
    return b0 + t * (b1 - b0);
}

// Builds cdf[0..nb) in LDS from weights w[0..nb-1) (w = weights + 1e-5, pdf = w / sum, cumsum).
__device__ __forceinline__ void build_cdf(const float* __restrict__ w_in, int nw, float* cdf, int lane) {
    double part = 0.0;
    for (int j = lane; j < nw; j += WAVE) part += (double)(w_in[j] + 1e-5f);
    const float total = (float)wave_sum_d(part);                 // torch.sum(weights, -1) (f32 result)
    double carry = 0.0;
    if (lane == 0) cdf[0] = 0.f;
    for (int base = 0; base < nw; base += WAVE) {
        const int j = base + lane;
        float pdf = 0.f;
        if (j < nw) pdf = (w_in[j] + 1e-5f) / total;
        const double incl = wave_scan_add_d((double)pdf, lane);
        if (j < nw) cdf[j + 1] = (float)(carry + incl);          // ATen CPU cumsum: double accumulate, round per element
        carry += shfl_d(incl, WAVE - 1);
    }
}

struct SampleArgs {
    const float* bins;      // [N, nb]            (sample_pdf / sample_from_cdf)
    const float* weights;   // [N, nb-1]          (sample_pdf)
    const float* cdf_in;    // [N, nb]            (sample_from_cdf)
    const float* z_coarse;  // [N, S]             (importance_resample)
    const float* w_coarse;  // [N, S]             (importance_resample)
    const float* u;
    int64_t u_row_stride;
    int64_t N;
    int nb, n_samples, S;
    float* samples;         // [N, n_samples] nullable for resample
    float* cdf_out;         // nullable
    int64_t* inds_out;      // nullable
    float* z_fine;          // [N, S + n_samples] (importance_resample)
};

// MODE 0: sample_pdf, 1: sample_from_cdf, 2: importance_resample (z_mid + sample_pdf + sorted merge)
template <int MODE>
__global__ __launch_bounds__(WAVE* RAYS_PER_BLOCK) void sample_kernel(const SampleArgs a) {
    __shared__ float s_cdf[RAYS_PER_BLOCK][MAX_NB];
    __shared__ float s_bins[RAYS_PER_BLOCK][MAX_NB];
    __shared__ float s_all[MODE == 2 ? RAYS_PER_BLOCK : 1][MODE == 2 ? MAX_MERGE : 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (n >= a.N) return;
    float* cdf = s_cdf[wv];
    float* bins = s_bins[wv];
    const int nb = a.nb;

    if (MODE == 2) {
        const float* zc = a.z_coarse + n * (int64_t)a.S;
        for (int j = lane; j < nb; j += WAVE) bins[j] = .5f * (zc[j + 1] + zc[j]);     // z_vals_mid (render.py:66)
        for (int j = lane; j < a.S; j += WAVE) s_all[wv][j] = zc[j];
        build_cdf(a.w_coarse + n * (int64_t)a.S + 1, nb - 1, cdf, lane);              // weights[..., 1:-1]
    } else {
        for (int j = lane; j < nb; j += WAVE) bins[j] = a.bins[n * (int64_t)nb + j];
        if (MODE == 0) build_cdf(a.weights + n * (int64_t)(nb - 1), nb - 1, cdf, lane);
        else for (int j = lane; j < nb; j += WAVE) cdf[j] = a.cdf_in[n * (int64_t)nb + j];
    }
    lds_sync_wave();
    if (a.cdf_out) for (int j = lane; j < nb; j += WAVE) a.cdf_out[n * (int64_t)nb + j] = cdf[j];

    const float* ur = a.u + n * a.u_row_stride;
    for (int i = lane; i < a.n_samples; i += WAVE) {
        int ind;
        const float smp = invert_cdf(cdf, bins, nb, ur[i], &ind);
        if (a.samples) a.samples[n * (int64_t)a.n_samples + i] = smp;
        if (a.inds_out) a.inds_out[n * (int64_t)a.n_samples + i] = ind;
        if (MODE == 2) s_all[wv][a.S + i] = smp;
    }
    if (MODE == 2) {
        lds_sync_wave();
        // torch.sort(cat([z_coarse, z_samples])) values: rank sort (pure permutation => exact).
        const int tot = a.S + a.n_samples;
        const float* all = s_all[wv];
        float* zf = a.z_fine + n * (int64_t)tot;
        for (int e = lane; e < tot; e += WAVE) {
            const float v = all[e];
            int rank = 0;
            for (int j = 0; j < tot; ++j) {
                const float o = all[j];
                rank += (o < v) || (o == v && j < e);
            }
            zf[rank] = v;
        }
    }
}

// manipulator z grid (networks/manipulator.py:117-119): near (1 - t) + far t
__global__ void zlerp_kernel(const float* __restrict__ t, float near_, float far_, int64_t total, int S, float* __restrict__ z) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const float tv = t[idx % S];
    z[idx] = near_ * (1.f - tv) + far_ * tv;
}

// torch.sort(x, -1) values of each row (manipulator.py:191,195): rank sort, one wave per row
constexpr int MAX_SORT = 2048;
__global__ __launch_bounds__(WAVE* RAYS_PER_BLOCK) void sort_rows_kernel(const float* __restrict__ in, int64_t N, int K, float* __restrict__ out) {
    __shared__ float v_lds[RAYS_PER_BLOCK][MAX_SORT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * RAYS_PER_BLOCK + wv;
    if (n >= N) return;
    float* all = v_lds[wv];
    for (int j = lane; j < K; j += WAVE) all[j] = in[n * (int64_t)K + j];
    lds_sync_wave();
    for (int e = lane; e < K; e += WAVE) {
        const float v = all[e];
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            const float o = all[j];
            rank += (o < v) || (o == v && j < e);
        }
        out[n * (int64_t)K + rank] = v;
    }
}

// exchanger (networks/manipulator.py:18-83): per (ray, sample) label logic + masked swaps of the raw rows
constexpr int MAX_MOVE = 8;
static_assert(64 + 128 + 128 * MAX_MOVE <= MAX_S, "a manipulation with MAX_MOVE objects must composite");
static_assert(3 * RAYS_PER_BLOCK * MAX_S * 4 <= 65536, "composite_bwd stages three rows per ray in static LDS");
struct ExchArgs {
    float* ori_raw;                       // [N,S,4+C], modified in place
    const float* tar_raw[MAX_MOVE];       // T x [N,S,4+C]
    const float* ori_acc;                 // [N,C] accumulated object map of the original rays
    const float* tar_acc[MAX_MOVE];       // T x [N,C]
    int labels[MAX_MOVE];
    int T, S, C;
    int64_t N;
    int64_t* ori_label;                   // [N,S] out (nullable)
    int64_t* tar_label;                   // [N,S] out: labels of the LAST target (nullable)
};

__device__ __forceinline__ int argmax_sigmoid(const float* x, int n) {
    int best = 0;
    float bv = sigmoidf_ref(x[0]);
    for (int c = 1; c < n; ++c) {
        const float v = sigmoidf_ref(x[c]);
        if (v > bv) { bv = v; best = c; }          // first maximum wins, like torch.argmax on CPU
    }
    return best;
}

__global__ void exchanger_kernel(const ExchArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N * a.S) return;
    const int64_t n = idx / a.S;
    const int ch = 4 + a.C;
    float* orow = a.ori_raw + idx * ch;
    int ori_lab = argmax_sigmoid(orow + 4, a.C);
    const int ori_acc_lab = argmax_sigmoid(a.ori_acc + n * a.C, a.C - 1);
    int tar_lab_last = 0;
    for (int t = 0; t < a.T; ++t) {
        const int L = a.labels[t];
        const float* trow = a.tar_raw[t] + idx * ch;
        if (ori_acc_lab != L && ori_lab == L) ori_lab = ori_acc_lab;                 // occluded: take the ray's label
        const bool fill = ori_acc_lab == L && ori_lab != L;
        int tar_lab = argmax_sigmoid(trow + 4, a.C);
        const int tar_acc_lab = argmax_sigmoid(a.tar_acc[t] + n * a.C, a.C - 1);
        if (tar_acc_lab != L && tar_lab == L) tar_lab = tar_acc_lab;
        const int reduced = (tar_lab == L ? 1 : 0) + (ori_lab == L ? 2 : 0);          // tar_move_mask - ori_move_mask
        const int op = reduced == 0 ? -1 : (reduced == 2 ? 0 : 1);                    // -1 keep, 0 eliminate, 1 exchange
        if (fill || op == 1) {
            for (int c = 0; c < ch; ++c) orow[c] = trow[c];
        } else if (op == 0) {
            for (int c = 0; c < ch; ++c) orow[c] = orow[c] * 0.f;
        }
        tar_lab_last = tar_lab;
    }
    if (a.ori_label) a.ori_label[idx] = ori_lab;
    if (a.tar_label) a.tar_label[idx] = tar_lab_last;
}

// edit_exchange: the exchanger's per-sample decision generalised to three kinds of edit plus a keep mask.  A MOVE is the loop
// body above; a COPY takes the target's rows but never gives up the original's; a REMOVE is the "eliminate" branch without a
// target (no target rays, no target rows read).  The keep mask tests the sample's OWN label l0 (before any occlusion
// correction), so what it zeroes does not depend on the order of the edits.
constexpr int EDIT_MOVE = 0, EDIT_COPY = 1, EDIT_REMOVE = 2;
constexpr int EDIT_MAX_C = 128;           // two 64-bit words of keep bits
struct EditExchArgs {
    float* ori_raw;                       // [N,S,4+C], modified in place
    const float* tar_raw[MAX_MOVE];       // E x [N,S,4+C]; null for a REMOVE
    const float* ori_acc;                 // [N,C]
    const float* tar_acc[MAX_MOVE];       // E x [N,C]; null for a REMOVE
    int labels[MAX_MOVE];
    int kinds[MAX_MOVE];
    uint64_t keep[2];
    int has_keep;
    int E, S, C;
    int64_t N;
    int64_t* ori_label;                   // [N,S] out (nullable): the original's label after the corrections
};

__global__ void edit_exchange_kernel(const EditExchArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N * a.S) return;
    const int64_t n = idx / a.S;
    const int ch = 4 + a.C;
    float* orow = a.ori_raw + idx * ch;
    const int l0 = argmax_sigmoid(orow + 4, a.C);
    int ori_lab = l0;
    const int ori_acc_lab = a.E > 0 ? argmax_sigmoid(a.ori_acc + n * a.C, a.C - 1) : 0;
    for (int e = 0; e < a.E; ++e) {
        const int L = a.labels[e];
        const int kind = a.kinds[e];
        if (ori_acc_lab != L && ori_lab == L) ori_lab = ori_acc_lab;                 // occluded: take the ray's label
        if (kind == EDIT_REMOVE) {
            if (ori_lab == L)
                for (int c = 0; c < ch; ++c) orow[c] = orow[c] * 0.f;                // ori_raw[...] * 0: -0, NaN of inf as there
            continue;
        }
        const float* trow = a.tar_raw[e] + idx * ch;
        int tar_lab = argmax_sigmoid(trow + 4, a.C);
        const int tar_acc_lab = argmax_sigmoid(a.tar_acc[e] + n * a.C, a.C - 1);
        if (tar_acc_lab != L && tar_lab == L) tar_lab = tar_acc_lab;
        const int reduced = (tar_lab == L ? 1 : 0) + (ori_lab == L ? 2 : 0);
        if (kind == EDIT_MOVE) {
            const bool fill = ori_acc_lab == L && ori_lab != L;
            if (fill || reduced == 1 || reduced == 3) {
                for (int c = 0; c < ch; ++c) orow[c] = trow[c];
            } else if (reduced == 2) {
                for (int c = 0; c < ch; ++c) orow[c] = orow[c] * 0.f;
            }
        } else if (reduced == 1) {                                                   // COPY: only where the original is not L
            for (int c = 0; c < ch; ++c) orow[c] = trow[c];
        }
    }
    if (a.has_keep) {
        const uint64_t word = l0 < 64 ? a.keep[0] : a.keep[1];                       // (a select, not a per-lane index into the arguments)
        if (!((word >> (l0 & 63)) & 1))
            for (int c = 0; c < ch; ++c) orow[c] = orow[c] * 0.f;
    }
    if (a.ori_label) a.ori_label[idx] = ori_lab;
}

__global__ void gather_kernel(const float* __restrict__ flat, const int32_t* __restrict__ idx,
                              float* __restrict__ blob, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t s = idx[i];
    blob[i] = s >= 0 ? flat[s] : 0.f;
}

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// One wave per ray.  The rows' dynamic LDS may exceed the 64 KiB default at large S: every launch allows RAY_LDS_MAX (common.h).
template <auto Kernel, class... Args>
int ray_launch(const char* what, int64_t N, size_t lds_bytes, void* stream, const Args&... args) {
    return dmn_launch_lds<Kernel, RAY_LDS_MAX>(what, blocks_for(N, RAYS_PER_BLOCK), WAVE * RAYS_PER_BLOCK, lds_bytes, (hipStream_t)stream, args...);
}

}  // namespace

// ==========================================================================================
// C ABI
// ==========================================================================================
extern "C" int dmnerf_pack_weights(const float* d_flat, const int32_t* d_idx, float* d_blob,
                                   int64_t n_blob, void* stream) {
    if (!d_flat || !d_idx || !d_blob || n_blob <= 0) return dmn_fail(DMNERF_E_ARG, "pack_weights: bad argument");
    hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(n_blob, 256)), dim3(256), 0, (hipStream_t)stream, d_flat, d_idx, d_blob, n_blob);
    return dmn_check_launch("pack_weights");
}

extern "C" int dmnerf_raygen(int H, int W, const float* h_intr, const float* h_c2w, int row0, int nrows,
                             float* d_rays_o, float* d_rays_d, void* stream) {
    if (!h_intr || !h_c2w || !d_rays_o || !d_rays_d) return dmn_fail(DMNERF_E_ARG, "raygen: null pointer");
    if (H < 1 || W < 1 || row0 < 0 || nrows < 0 || row0 + nrows > H)
        return dmn_fail(DMNERF_E_ARG, "raygen: rows [%d,%d) outside image %dx%d", row0, row0 + nrows, H, W);
    if (nrows == 0) return DMNERF_OK;
    RaygenArgs a;
    a.cam = dmn_raygen_cam(h_intr, h_c2w);
    a.W = W; a.row0 = row0; a.n = (int64_t)nrows * W; a.rays_o = d_rays_o; a.rays_d = d_rays_d;
    hipLaunchKernelGGL(raygen_kernel, dim3(blocks_for(a.n, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return dmn_check_launch("raygen");
}

extern "C" int dmnerf_z_val_sample(const float* d_t, float near_, float far_, int64_t N, int S, float* d_z, void* stream) {
    if (N < 0 || S < 1) return dmn_fail(DMNERF_E_ARG, "z_val_sample: bad N=%lld S=%d", (long long)N, S);
    if (N == 0) return DMNERF_OK;                        // an empty batch is legal and has null data pointers
    if (!d_t || !d_z) return dmn_fail(DMNERF_E_ARG, "z_val_sample: null pointer");
    hipLaunchKernelGGL(zvals_kernel, dim3(blocks_for(N * S, 256)), dim3(256), 0, (hipStream_t)stream, d_t, near_, far_, N * S, S, d_z);
    return dmn_check_launch("z_val_sample");
}

extern "C" int dmnerf_stratify(const float* d_z_in, const float* d_t_rand, int64_t N, int S, float* d_z_out, void* stream) {
    if (N < 0 || S < 1) return dmn_fail(DMNERF_E_ARG, "stratify: bad N=%lld S=%d", (long long)N, S);
    if (N == 0) return DMNERF_OK;
    if (!d_z_in || !d_t_rand || !d_z_out) return dmn_fail(DMNERF_E_ARG, "stratify: null pointer");
    if (d_z_in == d_z_out) return dmn_fail(DMNERF_E_ARG, "stratify: in-place not supported (reads neighbours)");
    hipLaunchKernelGGL(stratify_kernel, dim3(blocks_for(N * S, 256)), dim3(256), 0, (hipStream_t)stream, d_z_in, d_t_rand, N * S, S, d_z_out);
    return dmn_check_launch("stratify");
}

extern "C" int dmnerf_embed(const float* d_x, int64_t M, int L, float* d_out, void* stream) {
    if (M < 0 || L < 0 || L > 30) return dmn_fail(DMNERF_E_ARG, "embed: bad M=%lld L=%d", (long long)M, L);
    if (M == 0) return DMNERF_OK;
    if (!d_x || !d_out) return dmn_fail(DMNERF_E_ARG, "embed: null pointer");
    hipLaunchKernelGGL(embed_kernel, dim3(blocks_for(M * 3, 256)), dim3(256), 0, (hipStream_t)stream, d_x, M, L, d_out);
    return dmn_check_launch("embed");
}

extern "C" int dmnerf_composite_fwd(const float* d_raw, const float* d_z, const float* d_rays_d, int64_t N,
                                    int S, int C, float* d_rgb_map, float* d_weights, float* d_depth_map,
                                    float* d_ins_map, void* stream) {
    if (N < 0 || S < 1 || S > MAX_S || C < 1) return dmn_fail(DMNERF_E_ARG, "composite_fwd: bad N=%lld S=%d (max %d) C=%d", (long long)N, S, MAX_S, C);
    if (N == 0) return DMNERF_OK;
    // (C = 1: the object-code map has C - 1 = 0 columns, and an empty tensor has no storage; the kernel never touches it)
    if (!d_raw || !d_z || !d_rays_d || !d_rgb_map || !d_weights || !d_depth_map || (C > 1 && !d_ins_map))
        return dmn_fail(DMNERF_E_ARG, "composite_fwd: null pointer");
    return ray_launch<composite_kernel>("composite_fwd", N, ray_lds_bytes(1, S, C), stream,
                                        d_raw, d_z, d_rays_d, N, S, C, C - 1, d_rgb_map, d_weights, d_depth_map, d_ins_map);
}

extern "C" int dmnerf_weights_from_sigma(const float* d_sigma, const float* d_z, const float* d_rays_d, int64_t N, int S,
                                         float* d_weights, void* stream) {
    if (N < 0 || S < 1 || S > MAX_S) return dmn_fail(DMNERF_E_ARG, "weights_from_sigma: bad N=%lld S=%d (max %d)", (long long)N, S, MAX_S);
    if (N == 0) return DMNERF_OK;
    if (!d_sigma || !d_z || !d_rays_d || !d_weights) return dmn_fail(DMNERF_E_ARG, "weights_from_sigma: null pointer");
    hipLaunchKernelGGL(weights_kernel, dim3(blocks_for(N, RAYS_PER_BLOCK)), dim3(WAVE * RAYS_PER_BLOCK), 0, (hipStream_t)stream,
                       d_sigma, d_z, d_rays_d, N, S, d_weights);
    return dmn_check_launch("weights_from_sigma");
}

extern "C" int dmnerf_manipulator_render(const float* d_raw, const float* d_z, const float* d_rays_d, int64_t N,
                                         int S, int C, float* d_rgb_map, float* d_weights, float* d_depth_map,
                                         float* d_ins_map, void* stream) {
    if (N < 0 || S < 1 || S > MAX_S || C < 1) return dmn_fail(DMNERF_E_ARG, "manipulator_render: bad N=%lld S=%d (max %d) C=%d", (long long)N, S, MAX_S, C);
    if (N == 0) return DMNERF_OK;
    if (!d_raw || !d_z || !d_rays_d || !d_rgb_map || !d_weights || !d_depth_map || !d_ins_map)
        return dmn_fail(DMNERF_E_ARG, "manipulator_render: null pointer");
    return ray_launch<composite_kernel>("manipulator_render", N, ray_lds_bytes(1, S, C), stream,
                                        d_raw, d_z, d_rays_d, N, S, C, C, d_rgb_map, d_weights, d_depth_map, d_ins_map);
}

extern "C" int dmnerf_sample_pdf(const float* d_bins, const float* d_weights, const float* d_u, int64_t u_row_stride,
                                 int64_t N, int nb, int n_samples, float* d_samples, float* d_cdf, int64_t* d_inds,
                                 void* stream) {
    if (N < 0 || nb < 2 || nb > MAX_NB || n_samples < 1) return dmn_fail(DMNERF_E_ARG, "sample_pdf: bad N=%lld nb=%d n_samples=%d", (long long)N, nb, n_samples);
    if (N == 0) return DMNERF_OK;
    if (!d_bins || !d_weights || !d_u || !d_samples) return dmn_fail(DMNERF_E_ARG, "sample_pdf: null pointer");
    SampleArgs a{};
    a.bins = d_bins; a.weights = d_weights; a.u = d_u; a.u_row_stride = u_row_stride; a.N = N; a.nb = nb;
    a.n_samples = n_samples; a.samples = d_samples; a.cdf_out = d_cdf; a.inds_out = d_inds;
    hipLaunchKernelGGL(sample_kernel<0>, dim3(blocks_for(N, RAYS_PER_BLOCK)), dim3(WAVE * RAYS_PER_BLOCK), 0, (hipStream_t)stream, a);
    return dmn_check_launch("sample_pdf");
}

extern "C" int dmnerf_sample_from_cdf(const float* d_bins, const float* d_cdf, const float* d_u, int64_t u_row_stride,
                                      int64_t N, int nb, int n_samples, float* d_samples, int64_t* d_inds, void* stream) {
    if (N < 0 || nb < 2 || nb > MAX_NB || n_samples < 1) return dmn_fail(DMNERF_E_ARG, "sample_from_cdf: bad sizes");
    if (N == 0) return DMNERF_OK;
    if (!d_bins || !d_cdf || !d_u || !d_samples) return dmn_fail(DMNERF_E_ARG, "sample_from_cdf: null pointer");
    SampleArgs a{};
    a.bins = d_bins; a.cdf_in = d_cdf; a.u = d_u; a.u_row_stride = u_row_stride; a.N = N; a.nb = nb;
    a.n_samples = n_samples; a.samples = d_samples; a.inds_out = d_inds;
    hipLaunchKernelGGL(sample_kernel<1>, dim3(blocks_for(N, RAYS_PER_BLOCK)), dim3(WAVE * RAYS_PER_BLOCK), 0, (hipStream_t)stream, a);
    return dmn_check_launch("sample_from_cdf");
}

extern "C" int dmnerf_importance_resample(const float* d_z_coarse, const float* d_weights_coarse, const float* d_u,
                                          int64_t u_row_stride, int64_t N, int S, int n_imp, float* d_z_fine,
                                          float* d_z_samples, void* stream) {
    if (N < 0 || S < 3 || S - 1 > MAX_NB || n_imp < 1 || S + n_imp > MAX_MERGE)
        return dmn_fail(DMNERF_E_ARG, "importance_resample: bad N=%lld S=%d n_imp=%d", (long long)N, S, n_imp);
    if (N == 0) return DMNERF_OK;
    if (!d_z_coarse || !d_weights_coarse || !d_u || !d_z_fine) return dmn_fail(DMNERF_E_ARG, "importance_resample: null pointer");
    SampleArgs a{};
    a.z_coarse = d_z_coarse; a.w_coarse = d_weights_coarse; a.u = d_u; a.u_row_stride = u_row_stride; a.N = N;
    a.nb = S - 1; a.n_samples = n_imp; a.S = S; a.samples = d_z_samples; a.z_fine = d_z_fine;
    hipLaunchKernelGGL(sample_kernel<2>, dim3(blocks_for(N, RAYS_PER_BLOCK)), dim3(WAVE * RAYS_PER_BLOCK), 0, (hipStream_t)stream, a);
    return dmn_check_launch("importance_resample");
}

extern "C" int dmnerf_composite_bwd(const float* d_raw, const float* d_z, const float* d_rays_d, const float* d_ins_map,
                                    const float* d_g_rgb, const float* d_g_ins, const float* d_g_depth,
                                    const float* d_g_weights, int64_t N, int S, int C, float* d_grad_raw, void* stream) {
    if (N < 0 || S < 1 || S > MAX_S || C < 1) return dmn_fail(DMNERF_E_ARG, "composite_bwd: bad N=%lld S=%d (max %d) C=%d", (long long)N, S, MAX_S, C);
    if (N == 0) return DMNERF_OK;
    if (!d_raw || !d_z || !d_rays_d || !d_g_rgb || !d_grad_raw || (C > 1 && (!d_ins_map || !d_g_ins)))      // (C = 1: see composite_fwd)
        return dmn_fail(DMNERF_E_ARG, "composite_bwd: null pointer");
    return ray_launch<composite_bwd_kernel<false>>("composite_bwd", N, ray_lds_bytes(3, S, C), stream,
                                                   d_raw, d_z, d_rays_d, d_ins_map, d_g_rgb, d_g_ins, d_g_depth, d_g_weights, N, S, C, d_grad_raw, PenBwd{});
}

extern "C" int dmnerf_composite_pen_fwd(const float* d_raw, const float* d_z, const float* d_rays_d, int64_t N, int S, int C,
                                        float tolerance, float two_deta_w_sq, float gauss_norm, float* d_rgb_map, float* d_weights,
                                        float* d_depth_map, float* d_ins_map, double* d_partials, void* stream) {
    if (N < 0 || S < 1 || S > MAX_S || C < 1) return dmn_fail(DMNERF_E_ARG, "composite_pen_fwd: bad N=%lld S=%d (max %d) C=%d", (long long)N, S, MAX_S, C);
    if (N == 0) return DMNERF_OK;
    if (!d_raw || !d_z || !d_rays_d || !d_rgb_map || !d_weights || !d_depth_map || (C > 1 && !d_ins_map) || !d_partials)   // (C = 1: see composite_fwd)
        return dmn_fail(DMNERF_E_ARG, "composite_pen_fwd: null pointer");
    PenArgs a{};
    a.raw = d_raw; a.z = d_z; a.depth = d_depth_map; a.rays_d = d_rays_d; a.N = N; a.S = S; a.C = C;
    a.tol = tolerance; a.k2w = two_deta_w_sq; a.kh = gauss_norm; a.out4 = d_partials;
    return ray_launch<composite_pen_kernel>("composite_pen_fwd", N, ray_lds_bytes(3, S, C), stream,
                                            a, d_rgb_map, d_weights, d_depth_map, d_ins_map);
}

extern "C" int dmnerf_composite_pen_bwd(const float* d_raw, const float* d_z, const float* d_rays_d, const float* d_ins_map,
                                        const float* d_depth_map, const float* d_g_rgb, const float* d_g_ins, const float* d_g_depth,
                                        const float* d_g_weights, const double* d_g_partials, int64_t N, int S, int C, float tolerance,
                                        float two_deta_w_sq, float gauss_norm, float* d_grad_raw, void* stream) {
    if (N < 0 || S < 1 || S > MAX_S || C < 1) return dmn_fail(DMNERF_E_ARG, "composite_pen_bwd: bad N=%lld S=%d (max %d) C=%d", (long long)N, S, MAX_S, C);
    if (N == 0) return DMNERF_OK;
    if (!d_raw || !d_z || !d_rays_d || !d_depth_map || !d_g_rgb || !d_g_partials || !d_grad_raw || (C > 1 && (!d_ins_map || !d_g_ins)))
        return dmn_fail(DMNERF_E_ARG, "composite_pen_bwd: null pointer");
    PenBwd pen{};
    pen.depth = d_depth_map; pen.g_part = d_g_partials; pen.tol = tolerance; pen.k2w = two_deta_w_sq; pen.kh = gauss_norm;
    return ray_launch<composite_bwd_kernel<true>>("composite_pen_bwd", N, ray_lds_bytes(4, S, C), stream,
                                                  d_raw, d_z, d_rays_d, d_ins_map, d_g_rgb, d_g_ins, d_g_depth, d_g_weights, N, S, C, d_grad_raw, pen);
}

extern "C" int dmnerf_penalizer_fwd(const float* d_raw, const float* d_z, const float* d_depth, const float* d_rays_d,
                                    int64_t N, int S, int C, float tolerance, float two_deta_w_sq, float gauss_norm,
                                    double* d_partials, void* stream) {
    if (N < 0 || S < 1 || S > MAX_S || C < 1) return dmn_fail(DMNERF_E_ARG, "penalizer_fwd: bad N=%lld S=%d C=%d", (long long)N, S, C);
    if (N == 0) return DMNERF_OK;
    if (!d_raw || !d_z || !d_depth || !d_rays_d || !d_partials) return dmn_fail(DMNERF_E_ARG, "penalizer_fwd: null pointer");
    PenArgs a{};
    a.raw = d_raw; a.z = d_z; a.depth = d_depth; a.rays_d = d_rays_d; a.N = N; a.S = S; a.C = C;
    a.tol = tolerance; a.k2w = two_deta_w_sq; a.kh = gauss_norm; a.out4 = d_partials;
    return ray_launch<penalizer_kernel<0>>("penalizer_fwd", N, ray_lds_bytes(2, S, C), stream, a);
}

extern "C" int dmnerf_penalizer_bwd(const float* d_raw, const float* d_z, const float* d_depth, const float* d_rays_d,
                                    int64_t N, int S, int C, float tolerance, float two_deta_w_sq, float gauss_norm,
                                    const float* d_scales, float* d_grad_raw, void* stream) {
    if (N < 0 || S < 1 || S > MAX_S || C < 1) return dmn_fail(DMNERF_E_ARG, "penalizer_bwd: bad N=%lld S=%d C=%d", (long long)N, S, C);
    if (N == 0) return DMNERF_OK;
    if (!d_raw || !d_z || !d_depth || !d_rays_d || !d_scales || !d_grad_raw) return dmn_fail(DMNERF_E_ARG, "penalizer_bwd: null pointer");
    PenArgs a{};
    a.raw = d_raw; a.z = d_z; a.depth = d_depth; a.rays_d = d_rays_d; a.N = N; a.S = S; a.C = C;
    a.tol = tolerance; a.k2w = two_deta_w_sq; a.kh = gauss_norm; a.scales = d_scales; a.d_raw = d_grad_raw;
    return ray_launch<penalizer_kernel<1>>("penalizer_bwd", N, ray_lds_bytes(2, S, C), stream, a);
}

// The scalar tail of emptiness_penalizer (penalizer.py:44-55) on the device: the per-ray partials -> 4 sums (one block, fixed
// order: deterministic), then loss = S0 / (C max(S1, 1e-8)) + S2 / max(S3, 1e-8) and the two factors the backward multiplies by.
// Two launches instead of the ~14 scalar tensor operations of the same formulas (sum, clamp, mul, div, add, casts).
struct PenSumsArgs { const double* part[2]; int64_t N[2]; double* sums4[2]; };     // one block per problem (two levels per launch)
__global__ __launch_bounds__(1024) void penalizer_sums_kernel(const PenSumsArgs a) {
    const double* __restrict__ part = a.part[blockIdx.x];
    const int64_t N = a.N[blockIdx.x];
    double* __restrict__ sums4 = a.sums4[blockIdx.x];
    __shared__ double red[1024][4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < N; i += 1024)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += part[4 * i + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) red[threadIdx.x][k] = s[k];
    __syncthreads();
    for (int o = 512; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[threadIdx.x][k] += red[threadIdx.x + o][k];
        __syncthreads();
    }
    if (threadIdx.x < 4) sums4[threadIdx.x] = red[0][threadIdx.x];
}
__global__ void penalizer_finish_kernel(const double* __restrict__ sums4, int C, float* __restrict__ loss1, float* __restrict__ inv2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double nb = sums4[1] > 1e-8 ? sums4[1] : 1e-8, nm = sums4[3] > 1e-8 ? sums4[3] : 1e-8;
    loss1[0] = (float)(sums4[0] / ((double)C * nb) + sums4[2] / nm);
    inv2[0] = (float)(1.0 / ((double)C * nb));
    inv2[1] = (float)(1.0 / nm);
}

extern "C" int dmnerf_penalizer_sums(const double* d_partials, int64_t N, double* d_sums4, void* stream) {
    if (N < 0 || !d_sums4 || (N > 0 && !d_partials)) return dmn_fail(DMNERF_E_ARG, "penalizer_sums: bad argument");
    PenSumsArgs a{};
    a.part[0] = d_partials; a.N[0] = N; a.sums4[0] = d_sums4;
    hipLaunchKernelGGL(penalizer_sums_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    return dmn_check_launch("penalizer_sums");
}

extern "C" int dmnerf_penalizer_sums2(const double* d_partials_a, int64_t N_a, const double* d_partials_b, int64_t N_b, double* d_sums8,
                                      void* stream) {
    if (N_a < 0 || N_b < 0 || !d_sums8 || (N_a > 0 && !d_partials_a) || (N_b > 0 && !d_partials_b))
        return dmn_fail(DMNERF_E_ARG, "penalizer_sums2: bad argument");
    PenSumsArgs a{};
    a.part[0] = d_partials_a; a.N[0] = N_a; a.sums4[0] = d_sums8;
    a.part[1] = d_partials_b; a.N[1] = N_b; a.sums4[1] = d_sums8 + 4;
    hipLaunchKernelGGL(penalizer_sums_kernel, dim3(2), dim3(1024), 0, (hipStream_t)stream, a);
    return dmn_check_launch("penalizer_sums2");
}

extern "C" int dmnerf_penalizer_finish(const double* d_sums4, int C, float* d_loss1, float* d_inv2, void* stream) {
    if (!d_sums4 || !d_loss1 || !d_inv2 || C < 1) return dmn_fail(DMNERF_E_ARG, "penalizer_finish: bad argument");
    hipLaunchKernelGGL(penalizer_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_sums4, C, d_loss1, d_inv2);
    return dmn_check_launch("penalizer_finish");
}

extern "C" int dmnerf_raygen_select(int H, int W, const float* h_intr, const float* h_c2w, const int64_t* d_idx, int64_t n,
                                    float* d_rays_o, float* d_rays_d, void* stream) {
    if (H < 1 || W < 1 || n < 0) return dmn_fail(DMNERF_E_ARG, "raygen_select: bad size");
    if (n == 0) return DMNERF_OK;
    if (!h_intr || !h_c2w || !d_idx || !d_rays_o || !d_rays_d) return dmn_fail(DMNERF_E_ARG, "raygen_select: null pointer");
    RaygenArgs a;
    a.cam = dmn_raygen_cam(h_intr, h_c2w);
    a.W = W; a.row0 = 0; a.n = n; a.rays_o = d_rays_o; a.rays_d = d_rays_d;
    hipLaunchKernelGGL(raygen_select_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, a, d_idx);
    return dmn_check_launch("raygen_select");
}

extern "C" int dmnerf_z_val_lerp(const float* d_t, float near_, float far_, int64_t N, int S, float* d_z, void* stream) {
    if (N < 0 || S < 1) return dmn_fail(DMNERF_E_ARG, "z_val_lerp: bad N=%lld S=%d", (long long)N, S);
    if (N == 0) return DMNERF_OK;
    if (!d_t || !d_z) return dmn_fail(DMNERF_E_ARG, "z_val_lerp: null pointer");
    hipLaunchKernelGGL(zlerp_kernel, dim3(blocks_for(N * S, 256)), dim3(256), 0, (hipStream_t)stream, d_t, near_, far_, N * S, S, d_z);
    return dmn_check_launch("z_val_lerp");
}

extern "C" int dmnerf_sort_rows(const float* d_in, int64_t N, int K, float* d_out, void* stream) {
    if (N < 0 || K < 1 || K > MAX_SORT) return dmn_fail(DMNERF_E_ARG, "sort_rows: bad N=%lld K=%d (max %d)", (long long)N, K, MAX_SORT);
    if (N == 0) return DMNERF_OK;
    if (!d_in || !d_out || d_in == d_out) return dmn_fail(DMNERF_E_ARG, "sort_rows: null or aliased pointers");
    hipLaunchKernelGGL(sort_rows_kernel, dim3(blocks_for(N, RAYS_PER_BLOCK)), dim3(WAVE * RAYS_PER_BLOCK), 0, (hipStream_t)stream, d_in, N, K, d_out);
    return dmn_check_launch("sort_rows");
}

// ins_eval's per-pixel label and confidence (networks/evaluator.py:127-137): label = argmax over the object channels
// (first maximum wins, like torch.argmax on CPU), conf = that maximum.  One thread per ray; a row is <= 94 floats.
__global__ void label_conf_kernel(const float* __restrict__ ins, int64_t N, int C, int64_t* __restrict__ label, float* __restrict__ conf) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* x = ins + n * C;
    int best = 0;
    float bv = x[0];
    for (int c = 1; c < C; ++c) {
        const float v = x[c];
        if (v > bv) { bv = v; best = c; }
    }
    label[n] = best;
    if (conf) conf[n] = bv;
}

extern "C" int dmnerf_ins_label_conf(const float* d_ins, int64_t N, int C, int64_t* d_label, float* d_conf, void* stream) {
    if (N < 0 || C < 1) return dmn_fail(DMNERF_E_ARG, "ins_label_conf: bad N=%lld C=%d", (long long)N, C);
    if (N == 0) return DMNERF_OK;
    if (!d_ins || !d_label) return dmn_fail(DMNERF_E_ARG, "ins_label_conf: null pointer");
    hipLaunchKernelGGL(label_conf_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, d_ins, N, C, d_label, d_conf);
    return dmn_check_launch("ins_label_conf");
}

extern "C" int dmnerf_exchanger(float* d_ori_raw, const float* const* h_tar_raws, const float* d_ori_acc,
                                const float* const* h_tar_accs, const int* h_labels, int T, int64_t N, int S, int C,
                                int64_t* d_ori_label, int64_t* d_tar_label, void* stream) {
    if (T < 1 || T > MAX_MOVE || N < 0 || S < 1 || C < 2) return dmn_fail(DMNERF_E_ARG, "exchanger: bad T=%d (max %d) N=%lld S=%d C=%d", T, MAX_MOVE, (long long)N, S, C);
    if (N == 0) return DMNERF_OK;
    if (!d_ori_raw || !h_tar_raws || !d_ori_acc || !h_tar_accs || !h_labels) return dmn_fail(DMNERF_E_ARG, "exchanger: null pointer");
    ExchArgs a{};
    a.ori_raw = d_ori_raw; a.ori_acc = d_ori_acc; a.T = T; a.S = S; a.C = C; a.N = N; a.ori_label = d_ori_label; a.tar_label = d_tar_label;
    for (int t = 0; t < T; ++t) {
        if (!h_tar_raws[t] || !h_tar_accs[t]) return dmn_fail(DMNERF_E_ARG, "exchanger: null target pointer %d", t);
        a.tar_raw[t] = h_tar_raws[t]; a.tar_acc[t] = h_tar_accs[t]; a.labels[t] = h_labels[t];
    }
    hipLaunchKernelGGL(exchanger_kernel, dim3(blocks_for(N * S, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return dmn_check_launch("exchanger");
}

extern "C" int dmnerf_edit_exchange(float* d_ori_raw, const float* const* h_tar_raws, const float* d_ori_acc,
                                    const float* const* h_tar_accs, const int* h_labels, const int* h_kinds, int E,
                                    const uint64_t* h_keep, int64_t N, int S, int C, int64_t* d_ori_label, void* stream) {
    if (E < 0 || E > MAX_MOVE || (E == 0 && !h_keep))
        return dmn_fail(DMNERF_E_ARG, "edit_exchange: bad E=%d (1..%d, or 0 with a keep mask)", E, MAX_MOVE);
    if (N < 0 || S < 1 || C < 2 || C > EDIT_MAX_C)
        return dmn_fail(DMNERF_E_ARG, "edit_exchange: bad N=%lld S=%d C=%d (C in 2..%d)", (long long)N, S, C, EDIT_MAX_C);
    if (E > 0 && (!h_labels || !h_kinds)) return dmn_fail(DMNERF_E_ARG, "edit_exchange: null pointer (labels / kinds)");
    EditExchArgs a{};
    for (int e = 0; e < E; ++e) {
        const int kind = h_kinds[e], L = h_labels[e];
        if (kind != EDIT_MOVE && kind != EDIT_COPY && kind != EDIT_REMOVE)
            return dmn_fail(DMNERF_E_ARG, "edit_exchange: kind[%d]=%d (0 move, 1 copy, 2 remove)", e, kind);
        if (L < 0 || L >= C) return dmn_fail(DMNERF_E_ARG, "edit_exchange: label[%d]=%d outside [0, %d)", e, L, C);
        const float* raw = h_tar_raws ? h_tar_raws[e] : nullptr;
        const float* acc = h_tar_accs ? h_tar_accs[e] : nullptr;
        if (kind == EDIT_REMOVE) {
            if (raw || acc) return dmn_fail(DMNERF_E_ARG, "edit_exchange: edit %d is a removal: its target pointers must be null", e);
        } else if (!raw || !acc) {
            return dmn_fail(DMNERF_E_ARG, "edit_exchange: null target pointer %d (kind %d)", e, kind);
        }
        a.tar_raw[e] = raw; a.tar_acc[e] = acc; a.labels[e] = L; a.kinds[e] = kind;
    }
    if (N == 0) return DMNERF_OK;
    if (!d_ori_raw || (E > 0 && !d_ori_acc)) return dmn_fail(DMNERF_E_ARG, "edit_exchange: null pointer");
    if (N > 0x7fffffffLL * 256 / S) return dmn_fail(DMNERF_E_ARG, "edit_exchange: N=%lld S=%d too large", (long long)N, S);
    a.ori_raw = d_ori_raw; a.ori_acc = d_ori_acc; a.E = E; a.S = S; a.C = C; a.N = N; a.ori_label = d_ori_label;
    if (h_keep) { a.has_keep = 1; a.keep[0] = h_keep[0]; a.keep[1] = h_keep[1]; }
    hipLaunchKernelGGL(edit_exchange_kernel, dim3(blocks_for(N * S, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return dmn_check_launch("edit_exchange");
}
