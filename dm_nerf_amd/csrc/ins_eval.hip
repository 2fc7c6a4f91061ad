// ins_eval.hip -- instance AP of one rendered frame, `ins_eval` + `calculate_ap` (networks/evaluator.py:77-175), on the device.
//
// The reference turns the argmax labels into one-hot channels, broadcasts them against the one-hot ground truth into
// [ins_num, ins_num, H W] tensors for the two cost matrices (:55-70), matches with scipy on the host, and sorts the per-row
// confidences for the AP integral.  With 0/1 inputs every entry of those matrices is a function of three integer counts
// (row pixels, channel pixels, overlap), so here the frame is reduced to counts once and everything after works on them:
//   ie_prep_kernel    one pass over the pixels: label (argmax of pred_ins, or a given label) with the mask rule (:130-133),
//                     the order-preserving key of the confidence, the ground-truth row; per-label counts and the joint
//                     [gt row, label] table as LDS-private int32 histograms, one global atomic per non-zero bin per workgroup
//   ie_hist_kernel    \  exact per-label median (np.median, :141-145) by radix select on the 32-bit keys, all labels at once:
//   ie_select_kernel  /  IE_DIGIT-bit digits, per (label, target rank) histograms (two targets when the count is even);
//                     IE_PASSES pairs of launches
//   ie_solve_kernel   one workgroup: valid labels -> channels (:134-150), cost matrices from the counts (:152-154 -> :55-70),
//                     the assignment of the gt rows (lsa_wave.h, the criterion's solver), confidences (:159-165), the six APs
//                     (calculate_ap 'integral', :77-122) and the matched labels (:169-173)
// Integer counts are exact in any order; no host synchronisation, no allocation, kernels only (no memset node), so the sequence
// is capturable in a HIP graph.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "lsa_wave.h"

namespace {

constexpr int IE_MAXC = LSA_MAXC;      // ins_num <= 128, as for the criterion
constexpr int IE_DIGIT = 6;            // radix digit: [2 targets x 128 labels x 64 bins] int32 = 64 KiB of LDS per workgroup
constexpr int IE_BINS = 1 << IE_DIGIT;
constexpr int IE_PASSES = (32 + IE_DIGIT - 1) / IE_DIGIT;       // 6 (the last one 2 bits wide)
constexpr int IE_THREADS = 256;
constexpr int IE_MAX_BLOCKS = 256;     // workgroups of the pixel passes (each zeroes and flushes its private histograms)
constexpr unsigned char IE_SKIP = 255; // lab8 of a pixel whose label lies outside [0, ins_num) (flagged, counted nowhere)
// cost_ce's unit: -log(f32(1e-8)) as torch evaluates it in f32 (0x41935d8e = 18.420681); every term of the reference's mean is
// 0 or this value when both inputs are one-hot (1 + 1e-8 rounds to 1 in f32)
constexpr float IE_CE_UNIT = 18.420680999755859375f;

// Work buffer layout (byte offsets, 8-byte aligned).  [0, zero_bytes) is cleared by dmnerf_ins_eval_prep (ie_zero_kernel).
struct IeLayout {
    int64_t flags;      // int [4]: DMNERF_IE_* conditions
    int64_t cnt;        // int [C + 1]: pixels per label (label C = masked)
    int64_t joint;      // int [C][C + 1]: pixels per (gt row, label)
    int64_t hist;       // int [IE_PASSES][2][C][IE_BINS]: radix histograms per (target, label)
    int64_t zero_bytes;
    int64_t sel;        // uint [2][C] key prefix, int [2][C] residual rank, int [2][C] active
    int64_t med;        // float [C]: median confidence per label
    int64_t siou;       // float [C][C]: 1 - soft IoU, rows g < gt_num
    int64_t cost;       // float [C][C]: cost_ce + cost_siou
    int64_t lab8;       // uchar [N]: label of the pixel (C = masked, IE_SKIP)
    int64_t keys;       // uint [N]: order-preserving key of the confidence
    int64_t total;
};

__host__ __device__ inline IeLayout ie_layout(int64_t N, int C) {
    IeLayout w{};
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += (bytes + 7) & ~(int64_t)7; return at; };
    w.flags = take(16);
    w.cnt = take((int64_t)(C + 1) * 4);
    w.joint = take((int64_t)C * (C + 1) * 4);
    w.hist = take((int64_t)IE_PASSES * 2 * C * IE_BINS * 4);
    w.zero_bytes = o;
    w.sel = take((int64_t)3 * 2 * C * 4);
    w.med = take((int64_t)C * 4);
    w.siou = take((int64_t)C * C * 4);
    w.cost = take((int64_t)C * C * 4);
    w.lab8 = take(N);
    w.keys = take(N * 4);
    w.total = o;
    return w;
}

__device__ __forceinline__ unsigned f32_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ int pass_width(int p) { return (32 - IE_DIGIT * p) < IE_DIGIT ? 32 - IE_DIGIT * p : IE_DIGIT; }
__device__ __forceinline__ int pass_shift(int p) { return 32 - IE_DIGIT * p - pass_width(p); }

struct IePrep {
    const float* pred;          // [N] rows of pred_stride floats, C channels used; or null
    int64_t pred_stride;
    const int64_t* label_in;    // [N] (when pred is null)
    const float* conf;          // [N] (when pred is null)
    int64_t* label_out;         // [N]
    const float* mask;          // [N] or null
    const float* gt_ins;        // [N] rows of gt_stride floats, columns < gt_num one-hot; or null
    int64_t gt_stride;
    const int64_t* gt_label;    // [N] (when gt_ins is null)
    const int64_t* gt_rows;     // [gt_num] ascending
    int gt_num;
    int64_t N;
    int C;
    char* work;
};

// ---- the counters and histograms start at zero (a kernel, not a memset: one node in stream order when captured) ----------
__global__ __launch_bounds__(IE_THREADS) void ie_zero_kernel(int* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0;
}

// ---- pass 1: labels, keys, gt rows, counts ---------------------------------------------------------------------------
__global__ __launch_bounds__(IE_THREADS) void ie_prep_kernel(const IePrep a) {
    extern __shared__ int lds_i[];                     // [C + 1] label counts | [C][C + 1] joint
    __shared__ int64_t s_rows[IE_MAXC];
    __shared__ int s_flags;
    const int C = a.C, L = C + 1, tid = threadIdx.x;
    const IeLayout w = ie_layout(a.N, C);
    int* s_cnt = lds_i;
    int* s_joint = lds_i + L;
    for (int i = tid; i < L + C * L; i += blockDim.x) lds_i[i] = 0;
    if (a.gt_rows)
        for (int i = tid; i < a.gt_num; i += blockDim.x) s_rows[i] = a.gt_rows[i];
    if (tid == 0) s_flags = 0;
    __syncthreads();
    unsigned char* lab8 = reinterpret_cast<unsigned char*>(a.work + w.lab8);
    unsigned* keys = reinterpret_cast<unsigned*>(a.work + w.keys);
    int flags = 0;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + tid; n < a.N; n += (int64_t)gridDim.x * blockDim.x) {
        int l;
        float cf;
        if (a.pred) {                                   // argmax (first maximum) and max over all C channels (:127-137)
            const float* x = a.pred + n * a.pred_stride;
            l = 0;
            cf = x[0];
            for (int c = 1; c < C; ++c) {
                const float v = x[c];
                if (v > cf) { cf = v; l = c; }
            }
        } else {
            const int64_t l64 = a.label_in[n];
            cf = a.conf[n];
            l = (l64 >= 0 && l64 < C) ? (int)l64 : -1;
            if (l < 0) flags |= DMNERF_IE_LABEL_RANGE;
        }
        if (a.mask && a.mask[n] == 0.f) l = C;          // pred_label[mask == 0] = ins_num (:132)
        if (l >= 0) a.label_out[n] = l;
        else if (a.label_out != a.label_in) a.label_out[n] = a.label_in[n];
        lab8[n] = l >= 0 ? (unsigned char)l : IE_SKIP;
        keys[n] = f32_key(cf);
        int row = -1;
        if (a.gt_ins) {
            const float* g = a.gt_ins + n * a.gt_stride;
            for (int j = 0; j < a.gt_num; ++j) {
                const float v = g[j];
                if (v == 1.f) {
                    if (row >= 0) flags |= DMNERF_IE_GT_NOT_ONEHOT;
                    else row = j;
                } else if (v != 0.f) {
                    flags |= DMNERF_IE_GT_NOT_ONEHOT;
                }
            }
        } else {                                        // binary search of the pixel's label among the ascending rows
            const int64_t v = a.gt_label[n];
            int lo = 0, hi = a.gt_num;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_rows[mid] < v) lo = mid + 1; else hi = mid;
            }
            if (lo < a.gt_num && s_rows[lo] == v) row = lo;
        }
        if (l >= 0) {
            atomicAdd(&s_cnt[l], 1);
            if (row >= 0) atomicAdd(&s_joint[row * L + l], 1);
        }
    }
    if (flags) atomicOr(&s_flags, flags);
    __syncthreads();
    int* g_cnt = reinterpret_cast<int*>(a.work + w.cnt);
    int* g_joint = reinterpret_cast<int*>(a.work + w.joint);
    for (int i = tid; i < L; i += blockDim.x)
        if (s_cnt[i]) atomicAdd(&g_cnt[i], s_cnt[i]);
    const int nj = a.gt_num * L;
    for (int i = tid; i < nj; i += blockDim.x)
        if (s_joint[i]) atomicAdd(&g_joint[i], s_joint[i]);
    if (tid == 0 && s_flags) atomicOr(reinterpret_cast<int*>(a.work + w.flags), s_flags);
}

// ---- radix select, histogram of pass p: the digit of every key whose higher digits equal its (label, target)'s prefix -----
__global__ __launch_bounds__(IE_THREADS) void ie_hist_kernel(int64_t N, int C, char* __restrict__ work, int p) {
    extern __shared__ int lds_h[];                     // [2][C][IE_BINS]
    __shared__ unsigned s_prefix[2 * IE_MAXC];
    __shared__ int s_act[2 * IE_MAXC];
    const int tid = threadIdx.x;
    const IeLayout w = ie_layout(N, C);
    const int nb = 2 * C * IE_BINS;
    for (int i = tid; i < nb; i += blockDim.x) lds_h[i] = 0;
    const unsigned* g_prefix = reinterpret_cast<const unsigned*>(work + w.sel);
    const int* g_act = reinterpret_cast<const int*>(work + w.sel) + 4 * C;
    for (int i = tid; i < 2 * C; i += blockDim.x) {
        s_prefix[i] = p > 0 ? g_prefix[i] : 0u;
        s_act[i] = p > 0 ? g_act[i] : (i < C);         // pass 0: one histogram per label (both targets read it)
    }
    __syncthreads();
    const unsigned char* lab8 = reinterpret_cast<const unsigned char*>(work + w.lab8);
    const unsigned* keys = reinterpret_cast<const unsigned*>(work + w.keys);
    const int shift = pass_shift(p), width = pass_width(p), hi = shift + width;
    const unsigned dmask = (1u << width) - 1u;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + tid; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        const int l = lab8[n];
        if (l >= C) continue;                           // masked or skipped: in no channel
        const unsigned k = keys[n];
        const unsigned d = (k >> shift) & dmask;
        const unsigned top = p > 0 ? (k >> hi) : 0u;    // (hi = 32 only in pass 0)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int s = t * C + l;
            if (s_act[s] && top == s_prefix[s]) atomicAdd(&lds_h[s * IE_BINS + d], 1);
        }
    }
    __syncthreads();
    int* g_hist = reinterpret_cast<int*>(work + w.hist) + (int64_t)p * nb;
    for (int i = tid; i < nb; i += blockDim.x)
        if (lds_h[i]) atomicAdd(&g_hist[i], lds_h[i]);
}

// ---- radix select, pass p: the digit holding each target rank; after the last pass the medians ----------------------------
__global__ __launch_bounds__(IE_THREADS) void ie_select_kernel(int64_t N, int C, char* __restrict__ work, int p) {
    __shared__ unsigned s_key[2 * IE_MAXC];
    const IeLayout w = ie_layout(N, C);
    const int tid = threadIdx.x;
    unsigned* g_prefix = reinterpret_cast<unsigned*>(work + w.sel);
    int* g_rank = reinterpret_cast<int*>(work + w.sel) + 2 * C;
    int* g_act = reinterpret_cast<int*>(work + w.sel) + 4 * C;
    const int* cnt = reinterpret_cast<const int*>(work + w.cnt);
    const int* hist = reinterpret_cast<const int*>(work + w.hist) + (int64_t)p * 2 * C * IE_BINS;
    const int width = pass_width(p);
    for (int s = tid; s < 2 * C; s += blockDim.x) {
        const int t = s >= C, l = s - t * C;
        unsigned prefix;
        int rank, act;
        if (p == 0) {                                   // ranks (n - 1) / 2 and, for an even count, n / 2 (np.median)
            const int n = cnt[l];
            act = n > 0 && (t == 0 || (n & 1) == 0);
            rank = t == 0 ? (n - 1) / 2 : n / 2;
            prefix = 0u;
        } else {
            act = g_act[s];
            rank = g_rank[s];
            prefix = g_prefix[s];
        }
        if (act) {
            const int* h = hist + (int64_t)(p == 0 ? l : s) * IE_BINS;
            int d = 0;
            for (; d < (1 << width) - 1; ++d) {
                const int c = h[d];
                if (rank < c) break;
                rank -= c;
            }
            prefix = (prefix << width) | (unsigned)d;
        }
        g_prefix[s] = prefix;
        g_rank[s] = rank;
        g_act[s] = act;
        s_key[s] = act ? prefix : 0u;
    }
    if (p != IE_PASSES - 1) return;
    __syncthreads();
    float* med = reinterpret_cast<float*>(work + w.med);
    for (int l = tid; l < C; l += blockDim.x) {
        const int n = cnt[l];
        float m = 0.f;
        if (n > 0) {
            m = key_f32(s_key[l]);
            if ((n & 1) == 0) m = (m + key_f32(s_key[C + l])) / 2.0f;    // numpy: mean of the two middle values, in f32
        }
        med[l] = m;
    }
}

// torch.sum of a short f32 vector on the CPU, in ATen's order (what `ap = torch.sum(...)` of the integral method does, :97):
// below 8 elements four scalar accumulators (stride 4, the tail into the first); otherwise 8-lane vectors summed by four vector
// accumulators the same way, then the scalar tail, then lanes 0..7.  x: LDS, n <= 130.
__device__ float aten_sum_f32(const float* x, int n) {
    if (n < 8) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        const int q = n / 4;
        for (int i = 0; i < q; ++i) { a0 += x[4 * i]; a1 += x[4 * i + 1]; a2 += x[4 * i + 2]; a3 += x[4 * i + 3]; }
        for (int i = 4 * q; i < n; ++i) a0 += x[i];
        a0 += a1; a0 += a2; a0 += a3;
        return a0;
    }
    const int nv = n / 8, q = nv / 4;
    float s = 0.f;
    for (int k = nv * 8; k < n; ++k) s += x[k];
    for (int lane = 0; lane < 8; ++lane) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int i = 0; i < q; ++i) {
            a0 += x[8 * (4 * i) + lane]; a1 += x[8 * (4 * i + 1) + lane];
            a2 += x[8 * (4 * i + 2) + lane]; a3 += x[8 * (4 * i + 3) + lane];
        }
        for (int v = 4 * q; v < nv; ++v) a0 += x[8 * v + lane];
        a0 += a1; a0 += a2; a0 += a3;
        s += a0;
    }
    return s;
}

// ---- channels, cost matrices, assignment, confidences, APs, matched labels: one workgroup ------------------------------
__global__ __launch_bounds__(IE_THREADS) void ie_solve_kernel(int64_t N, int C, int gt_num, int masked, char* __restrict__ work,
                                                              float* __restrict__ ap6, int64_t* __restrict__ matched) {
    const IeLayout w = ie_layout(N, C);
    const int L = C + 1, tid = threadIdx.x;
    __shared__ int s_cnt[IE_MAXC + 1], s_lab[IE_MAXC + 1], s_ng[IE_MAXC], s_V;
    __shared__ LsaShared s_lsa;
    __shared__ float s_iou[IE_MAXC], s_conf[IE_MAXC], s_sorted[IE_MAXC];
    __shared__ float s_mrec[6][IE_MAXC + 2], s_mprec[6][IE_MAXC + 2];
    const int* cnt = reinterpret_cast<const int*>(work + w.cnt);
    const int* joint = reinterpret_cast<const int*>(work + w.joint);
    const float* med = reinterpret_cast<const float*>(work + w.med);
    float* siou = reinterpret_cast<float*>(work + w.siou);
    float* cost = reinterpret_cast<float*>(work + w.cost);
    for (int l = tid; l < L; l += blockDim.x) s_cnt[l] = cnt[l];
    for (int g = tid; g < gt_num; g += blockDim.x) {
        int s = 0;
        for (int l = 0; l < L; ++l) s += joint[g * L + l];
        s_ng[g] = s;
    }
    __syncthreads();
    // 1. valid labels, ascending = channels (unique, :129 / :133 -- with a mask the LARGEST present value is dropped)
    if (tid == 0) {
        int v = 0, last = -1;                           // (label C occurs only under a mask, and is then the one dropped)
        for (int l = 0; l < L; ++l)
            if (s_cnt[l] > 0) { s_lab[v++] = l; last = l; }
        if (masked && last >= 0) --v;
        s_V = v;
    }
    __syncthreads();
    const int V = s_V;
    // 2. cost matrices of the gt rows (:152-154 -> hungarian :55-70) from the counts
    for (int e = tid; e < gt_num * C; e += blockDim.x) {
        const int g = e / C, p = e - g * C;
        const int tp = p < V ? joint[g * L + s_lab[p]] : 0;
        const int np_ = p < V ? s_cnt[s_lab[p]] : 0;
        const int ng = s_ng[g];
        // cost_ce = mean over the pixels of 0 / IE_CE_UNIT terms: exact count of differing pixels, rounded once
        const float ce = (float)(((double)IE_CE_UNIT * (double)(ng + np_ - 2 * tp)) / (double)N);
        const float TP = (float)tp;
        const float FP = (float)np_ - TP;
        const float FN = (float)ng - TP;
        const float si = 1.0f - TP / (TP + FP + FN + 1e-6f);
        siou[e] = si;
        cost[e] = ce + si;                              // `cost_ce + cost_siou` in f32 (:70)
    }
    __syncthreads();
    // 3. assignment of the gt rows (reorder, :43-47 -> scipy linear_sum_assignment)
    if (tid < 64)
        lsa_solve_wave(s_lsa, gt_num, C, tid, [&](int i, int j) { return (double)cost[i * C + j]; });
    __syncthreads();
    // 4. IoU and confidence per row (:157-165), matched labels (:169-173)
    for (int g = tid; g < C; g += blockDim.x) {
        int64_t lab = -1;
        if (g < gt_num) {
            const int col = s_lsa.col4row[g];
            s_iou[g] = 1.0f - siou[g * C + col];
            s_conf[g] = col < V ? med[s_lab[col]] : 0.f;
            if (col < V) lab = s_lab[col];
        }
        matched[g] = lab;
    }
    __syncthreads();
    // 5. argsort(confidence, descending), ties in index order (torch's CPU order up to 16 entries)
    for (int g = tid; g < gt_num; g += blockDim.x) {
        const float c = s_conf[g];
        int pos = 0;
        for (int h = 0; h < gt_num; ++h) {
            const float ch = s_conf[h];
            pos += (ch > c) || (ch == c && h < g);
        }
        s_sorted[pos] = s_iou[g];
    }
    __syncthreads();
    // 6. calculate_ap, 'integral' (:77-122): one thread per threshold
    if (tid < 6) {
        const float thre[6] = {0.5f, 0.75f, 0.8f, 0.85f, 0.9f, 0.95f};
        const float th = thre[tid];
        float* mrec = s_mrec[tid];
        float* mprec = s_mprec[tid];
        const int n = gt_num;
        mrec[0] = 0.f; mprec[0] = 0.f;
        int cum = 0;
        for (int k = 0; k < n; ++k) {
            cum += s_sorted[k] > th;
            mprec[k + 1] = (float)cum / (float)(k + 1);
            mrec[k + 1] = (float)cum / (float)n;
        }
        mrec[n + 1] = 1.f; mprec[n + 1] = 0.f;
        for (int i = n + 1; i > 0; --i) mprec[i - 1] = fmaxf(mprec[i - 1], mprec[i]);
        // the terms where recall changes, compacted in place over mprec (term m is written at m <= i, after mprec[i + 1] is read)
        int m = 0;
        for (int i = 0; i <= n; ++i)
            if (mrec[i + 1] != mrec[i]) mprec[m++] = (mrec[i + 1] - mrec[i]) * mprec[i + 1];
        ap6[tid] = aten_sum_f32(mprec, m);
    }
}

}  // namespace

extern "C" int64_t dmnerf_ins_eval_work_bytes(int64_t N, int ins_num) {
    if (N < 1 || ins_num < 1 || ins_num > IE_MAXC) return -1;
    return ie_layout(N, ins_num).total;
}

extern "C" int64_t dmnerf_ins_eval_flags_offset(int64_t N, int ins_num) {
    if (N < 1 || ins_num < 1 || ins_num > IE_MAXC) return -1;
    return ie_layout(N, ins_num).flags;
}

extern "C" int64_t dmnerf_ins_eval_median_offset(int64_t N, int ins_num) {
    if (N < 1 || ins_num < 1 || ins_num > IE_MAXC) return -1;
    return ie_layout(N, ins_num).med;
}

static int ie_blocks(int64_t N) {
    const int64_t b = (N + IE_THREADS - 1) / IE_THREADS;
    return (int)(b < IE_MAX_BLOCKS ? b : IE_MAX_BLOCKS);
}

extern "C" int dmnerf_ins_eval_prep(const float* d_pred_ins, int64_t pred_row_stride, const int64_t* d_label_in, const float* d_conf,
                                    int64_t* d_label_out, const float* d_mask, const float* d_gt_ins, int64_t gt_row_stride,
                                    const int64_t* d_gt_label, const int64_t* d_gt_rows, int gt_num, int64_t N, int ins_num,
                                    void* d_work, int64_t work_bytes, void* stream) {
    if (N < 1 || ins_num < 1 || ins_num > IE_MAXC)
        return dmn_fail(DMNERF_E_ARG, "ins_eval_prep: bad N=%lld ins_num=%d (max %d)", (long long)N, ins_num, IE_MAXC);
    if (gt_num < 0 || gt_num > ins_num) return dmn_fail(DMNERF_E_ARG, "ins_eval_prep: bad gt_num=%d (0..ins_num=%d)", gt_num, ins_num);
    if (!d_label_out || !d_work) return dmn_fail(DMNERF_E_ARG, "ins_eval_prep: null pointer");
    if (d_pred_ins ? pred_row_stride < ins_num : (!d_label_in || !d_conf))
        return dmn_fail(DMNERF_E_ARG, "ins_eval_prep: give pred_ins with a row stride >= ins_num, or a label and a confidence");
    if (d_gt_ins ? gt_row_stride < gt_num : (!d_gt_label || (gt_num > 0 && !d_gt_rows)))
        return dmn_fail(DMNERF_E_ARG, "ins_eval_prep: give gt_ins with a row stride >= gt_num, or gt labels and the gt rows");
    const IeLayout w = ie_layout(N, ins_num);
    if (work_bytes < w.total)
        return dmn_fail(DMNERF_E_ARG, "ins_eval_prep: work buffer too small (%lld < %lld bytes)", (long long)work_bytes, (long long)w.total);
    // (ie_hist_kernel too: dmnerf_ins_eval, which launches it, works on what this entry prepared and so follows it)
    if (int rc = dmn_allow_lds<ie_prep_kernel, (IE_MAXC + 1) * (IE_MAXC + 1) * 4>("ins_eval_prep")) return rc;
    if (int rc = dmn_allow_lds<ie_hist_kernel, 2 * IE_MAXC * IE_BINS * 4>("ins_eval_prep")) return rc;
    const int64_t nz = w.zero_bytes / 4;
    hipLaunchKernelGGL(ie_zero_kernel, dim3((unsigned)((nz + IE_THREADS - 1) / IE_THREADS < 512 ? (nz + IE_THREADS - 1) / IE_THREADS : 512)),
                       dim3(IE_THREADS), 0, (hipStream_t)stream, (int*)d_work, nz);
    if (int rc = dmn_check_launch("ins_eval_prep: clear")) return rc;
    IePrep a{};
    a.pred = d_pred_ins; a.pred_stride = pred_row_stride; a.label_in = d_label_in; a.conf = d_conf; a.label_out = d_label_out;
    a.mask = d_mask; a.gt_ins = d_gt_ins; a.gt_stride = gt_row_stride; a.gt_label = d_gt_label; a.gt_rows = d_gt_rows;
    a.gt_num = gt_num; a.N = N; a.C = ins_num; a.work = (char*)d_work;
    const size_t lds = (size_t)(ins_num + 1) * (ins_num + 1) * 4;
    hipLaunchKernelGGL(ie_prep_kernel, dim3((unsigned)ie_blocks(N)), dim3(IE_THREADS), lds, (hipStream_t)stream, a);
    return dmn_check_launch("ins_eval_prep");
}

extern "C" int dmnerf_ins_eval(int64_t N, int ins_num, int gt_num, int masked, void* d_work, int64_t work_bytes, float* d_ap6,
                               int64_t* d_matched, void* stream) {
    if (N < 1 || ins_num < 1 || ins_num > IE_MAXC)
        return dmn_fail(DMNERF_E_ARG, "ins_eval: bad N=%lld ins_num=%d (max %d)", (long long)N, ins_num, IE_MAXC);
    if (gt_num < 0 || gt_num > ins_num) return dmn_fail(DMNERF_E_ARG, "ins_eval: bad gt_num=%d (0..ins_num=%d)", gt_num, ins_num);
    if (!d_work || !d_ap6 || !d_matched) return dmn_fail(DMNERF_E_ARG, "ins_eval: null pointer");
    const IeLayout w = ie_layout(N, ins_num);
    if (work_bytes < w.total)
        return dmn_fail(DMNERF_E_ARG, "ins_eval: work buffer too small (%lld < %lld bytes)", (long long)work_bytes, (long long)w.total);
    const size_t lds = (size_t)2 * ins_num * IE_BINS * 4;
    for (int p = 0; p < IE_PASSES; ++p) {
        hipLaunchKernelGGL(ie_hist_kernel, dim3((unsigned)ie_blocks(N)), dim3(IE_THREADS), lds, (hipStream_t)stream, N, ins_num,
                           (char*)d_work, p);
        if (int rc = dmn_check_launch("ins_eval: radix histogram")) return rc;
        hipLaunchKernelGGL(ie_select_kernel, dim3(1), dim3(IE_THREADS), 0, (hipStream_t)stream, N, ins_num, (char*)d_work, p);
        if (int rc = dmn_check_launch("ins_eval: radix select")) return rc;
    }
    hipLaunchKernelGGL(ie_solve_kernel, dim3(1), dim3(IE_THREADS), 0, (hipStream_t)stream, N, ins_num, gt_num, masked ? 1 : 0,
                       (char*)d_work, d_ap6, d_matched);
    return dmn_check_launch("ins_eval: solve");
}
