// conv3x3.hip -- 3x3 convolution, stride 1, zero padding 1, bias, ReLU, exact f32: the thirteen convolutions of the VGG16 under LPIPS
// (lpips.LPIPS(net="vgg") at networks/tester.py:43,91 and networks/manipulator.py:216,280 of the reference) as an implicit GEMM on
// gemm_nt.hip's engine: operands global -> LDS by LDS-DMA into a swizzled ring, ds_read_b128 operand reads, a hand-scheduled stream of
// v_mfma_f32_32x32x2_f32, one workgroup = 128 rows x all (up to 320) outputs of an out-tile, persistent over the row tiles.
//
// Layout ("padded-flat", NHWC): per image (H+2)(W+2) rows of C floats with a zero border, the images of a batch stacked, W+3 zeroed
// guard rows before the first and after the last image.  Output row m (0 .. P (H+2)(W+2) - 1, borders included) then needs, for tap
// (dy, dx), buffer row m + dy (W+2) + dx: a CONSTANT row offset.  Since a row is exactly Cin floats, the three taps of one dy are 3 Cin
// CONTIGUOUS floats, and the whole K range is three runs of 3 Cin floats, (W+2) rows apart:
//
//   out[m][n] = relu( bias[n] + sum_{dy} sum_{k < 3 Cin} in[(m + dy (W+2)) Cin + k] Wp[n][dy 3 Cin + k] )        Wp: [Cout][9 Cin], tap-major
//
// The fetch stream walks 32-float chunks with a byte offset that grows by 128 per chunk and jumps by (W+2-3) rows after every third of
// the K range; everything else (ring, hand-over, read geometry, MFMA order: an fmaf chain in k order with the bias as the initial
// value) is gemm_nt's.  `taps == 1` is the one-run form (K = Cin = 32, no neighbours): the first VGG layer, whose 27 taps the LPIPS
// prologue (lpips.hip) has laid out per pixel.
//
// The epilogue writes the output in the same layout, so it is the next layer's input as it stands: rows that are border positions
// are written as exact zeros BY SELECT (whatever was accumulated there -- the sums of a border row are meaningless, and may be NaN
// -- never reaches a neighbour), the guard rows are zeroed by the entry point.  ReLU keeps a NaN (v < 0 ? 0 : v), as torch does.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dmnerf_hip.h"
#include "common.h"
#include "mlp_common.h"

using namespace dmn;

namespace {

constexpr int CV_STAGE_BYTES = 16384;     // the epilogue's transposition area: 4 KiB per wave (one 32 x 32 block)
constexpr int CV_MAX_DEPTH = 4;
constexpr int CV_MAX_NBB = 10;            // 320 outputs per workgroup (gemm_nt's budget)

// Up to 4 out-blocks two workgroups share a CU (ring at depth >= 2 plus staging in 80 KiB); wider tiles keep the CU.
constexpr int cv_occupancy(int nbb) { return nbb <= 4 ? 2 : 1; }

struct CvArgs {
    const float* A;                       // padded-flat input, from its first guard row (taps 9) / the [M][32] tap rows (taps 1)
    int64_t a_floats;                     // floats from A to the end of its allocation
    int lda;                              // = Cin
    int run_chunks;                       // 32-k chunks of one contiguous run: 3 Cin / 32 (taps 9), Cin / 32 (taps 1)
    int nchunk;                           // chunks of the whole K range: 3 runs (taps 9) or 1
    int run_step;                         // bytes added to the A offset after a run: (W+2-3) rows
    int span_rows;                        // rows beyond a tile's own that its taps reach: 2 (W+2) + 2 (taps 9), 0
    const float* B; int64_t b_floats;     // packed weights [Cout][ldb]
    int ldb;
    const float* bias;                    // [n_out] or null
    int n_out;
    float* C; int ldc;                    // output rows from the first IMAGE row (behind the guard); ldc = Cout
    int64_t M;                            // P (H+2)(W+2)
    int Hp, Wp;                           // H+2, W+2
    int relu;
};

template <int NBB>
struct CvRing {
    static constexpr int NL = 4 + NBB;                                   // DMA pieces per wave per chunk (1 KiB each)
    static constexpr int BUF = NL * 4096;                                // bytes per chunk
    static constexpr int BUDGET = (cv_occupancy(NBB) == 2 ? 81920 : 147456) - CV_STAGE_BYTES;
    static constexpr int D = BUDGET / BUF < CV_MAX_DEPTH ? BUDGET / BUF : CV_MAX_DEPTH;
    static_assert(D >= 2, "ring needs two slots");
    static_assert((D - 1) * NL <= 63, "vmcnt range");
};

template <int NBB>
__global__ __launch_bounds__(256, cv_occupancy(NBB)) void conv3x3_kernel(const CvArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)     // (the host pass only needs the launch stub, as in gemm_nt.hip)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    typedef CvRing<NBB> RG;
    constexpr int NL = RG::NL, D = RG::D, BUF = RG::BUF;
    constexpr int NR = 1 + NBB;                     // operand reads per round
    constexpr int NGAP = 4 * NBB;                   // MFMAs per round
    const int tid = threadIdx.x;
    const int lane = tid & 63, half = lane >> 5, li = lane & 31;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lds0 = lds_addr(lds);
    const int j0 = blockIdx.y * (NBB * 32);         // first output of this workgroup
    const int nchunk = a.nchunk;
    // PERSISTENT: a workgroup walks the row tiles blockIdx.x, + gridDim.x, ... (32-bit tile counters; the host bounds M)
    const int ntiles = (int)((a.M + 127) / 128);
    int tile = blockIdx.x;

    // ---- DMA geometry (gemm_nt.hip): wave w owns the 1-KiB piece w of every 32-row block; lane l lands at LDS row 8 w + (l >> 3),
    // unit l & 7, so it fetches unit (l & 7) ^ ((row >> 1) & 7) of that row
    const int drow = 8 * w + (lane >> 3);
    const int dunit = ((lane & 7) ^ ((drow >> 1) & 7)) << 4;
    const int voA = drow * a.lda * 4 + dunit;
    const int voB = drow * a.ldb * 4 + dunit;
    auto bound = [](int64_t want, int64_t have) { const int64_t b = want < have ? want : have; return b < 0 ? (int64_t)0 : (b < 0x1fffffff ? b : (int64_t)0x1fffffff); };
    const rsrc_t rsB = uniform_rsrc(a.B + (int64_t)j0 * a.ldb, bound((int64_t)NBB * 32 * a.ldb, a.b_floats - (int64_t)j0 * a.ldb));
    const int blkA = 32 * a.lda * 4, blkB = 32 * a.ldb * 4;               // bytes per 32-row block
    typedef const CvArgs __attribute__((address_space(4))) KArgs;         // (the kernel's one argument sits at the start of the segment)
    auto args = [&]() -> KArgs* { KArgs* p = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr(); asm volatile("" : "+s"(p)); return p; };
    // per-tile state.  The descriptor of a tile covers its own rows and the span its taps reach, cut at the end of the allocation:
    // what lies beyond reads as 0 and feeds only rows beyond M, which the epilogue never stores
    int64_t i0 = 0;
    rsrc_t rsA;
    auto set_tile = [&](int t) __attribute__((always_inline)) {
        KArgs* q = args();
        i0 = (int64_t)t * 128;
        const int64_t rows_valid = q->M - i0 < 128 ? q->M - i0 : 128;
        rsA = uniform_rsrc(q->A + i0 * q->lda, bound((rows_valid + q->span_rows) * q->lda, q->a_floats - i0 * q->lda));
    };

    auto fresh_s = [](int x) -> int { asm volatile("" : "+s"(x)); return x; };
    int fa = 0;                                         // byte offset of the next request's chunk inside an A row run (uniform)
    auto dma_chunk_piece = [&](int cc, unsigned slot_byte, int i) __attribute__((always_inline)) {      // piece i of NL of chunk cc (< nchunk) into a ring slot
        float* dst = lds + (slot_byte + i * 4096 + fresh_s(w) * 1024) / 4;
        if (i < 4) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (DMN_LAS void*)dst, 16, voA, i * fresh_s(blkA) + fa, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (DMN_LAS void*)dst, 16, voB, (i - 4) * fresh_s(blkB) + cc * 128, 0, 0);
    };
    // ---- read geometry: lane (li, half) reads row 32 blk + li, unit (2 t + half) ^ ((li >> 1) & 7) in round t
    unsigned offA[4], offB[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const unsigned o = lds0 + li * 128 + ((((2 * t + half) ^ ((li >> 1) & 7))) << 4);
        offA[t] = o + w * 4096;
        offB[t] = o + 4 * 4096;
    }

    // ---- the bias (column n = j0 + 32 b + li is this lane's in every register of block b), once for all tiles
    float bias_v[NBB];
#pragma unroll
    for (int b = 0; b < NBB; ++b) {
        bias_v[b] = (a.bias && j0 + 32 * b + li < a.n_out) ? a.bias[j0 + 32 * b + li] : 0.f;
        if constexpr (NBB > 6) asm volatile("" : "+a"(bias_v[b]));          // (parked in the AGPR half next to the accumulators)
    }
    asm volatile("" ::: "memory");

    f32x4 av[2][1], bv[2][NBB];
    auto read_ops_one = [&](auto gc, int buf, unsigned addrA, unsigned addrB) {     // operand g of a round
        constexpr int g = decltype(gc)::value;
        if constexpr (g == 0) lds_read16_async<0>(av[buf][0], addrA);
        else lds_read16_async<(g - 1) * 4096>(bv[buf][g - 1], addrB);
    };

    // ---- ONE chunk stream across the tiles (gemm_nt.hip): the ring does not drain at a tile boundary
    int fc = 0;                                         // chunk (inside the fetch tile) of the next request
    int fr = 0;                                         // ... and its position inside the current run
    int ahead = 0;                                      // chunks requested beyond the one being consumed
    int ftile = tile;
    bool fvalid = true;
    set_tile(ftile);
    const int64_t i0_first = i0;
    auto advance_fetch = [&]() __attribute__((always_inline)) {           // after the NL pieces of (ftile, fc) have been issued
        fa += 128;
        if (++fr == a.run_chunks) { fr = 0; fa += a.run_step; }           // the next dy: (W+2) rows on, less the three rows just walked
        if (++fc == nchunk) {
            fc = 0; fr = 0; fa = 0;
            ftile += (int)gridDim.x;
            fvalid = ftile < ntiles;
            if (fvalid) set_tile(ftile);
        }
    };
#pragma unroll
    for (int sl = 0; sl < D; ++sl)
        if (fvalid) {
#pragma unroll
            for (int i = 0; i < NL; ++i) dma_chunk_piece(fc, sl * BUF, i);
            advance_fetch();
            ++ahead;
        }
    --ahead;                                            // (chunk 0 is the one being consumed)
    if (ahead == D - 1) __builtin_amdgcn_s_waitcnt(0x0F70 | (((D - 1) * NL) & 15) | ((((D - 1) * NL) >> 4) << 14));     // vmcnt((D-1) NL) only
    else __builtin_amdgcn_s_waitcnt(0x0F70);                                                                           // a short stream: everything
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    static_for<NR>([&](auto gc) { read_ops_one(gc, 0, offA[0], offB[0]); });

    f32x16 acc[NBB];
    unsigned sb = 0;                                    // byte offset of the ring slot of the chunk being consumed (uniform)
    int64_t i0c = i0_first;                             // the tile being COMPUTED
#pragma nounroll
    for (;;) {
#pragma unroll
        for (int b = 0; b < NBB; ++b) {                 // accumulators start from the bias
            float bb = bias_v[b];
            asm volatile("" : "+v"(bb));
            acc[b] = (f32x16)(bb);
            if constexpr (NBB > 6) asm volatile("" : "+a"(acc[b]));
        }

#pragma nounroll
        for (int c = 0; c < nchunk; ++c) {
            const unsigned nb = sb + BUF == (unsigned)(D * BUF) ? 0u : sb + BUF;
            unsigned cA[4], cB[4];
#pragma unroll
            for (int t = 1; t < 4; ++t) { cA[t] = offA[t] + sb; cB[t] = offB[t] + sb; }
            cA[0] = offA[0] + nb; cB[0] = offB[0] + nb; // round 0 of the NEXT chunk of the stream (read in this chunk's round 3)
            static_for<4>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                lds_wait<0>(av[r & 1]);
#pragma unroll
                for (int k = 0; k < NBB; ++k) asm volatile("" : "+" DMN_TILE_RC(bv[r & 1][k]));
                if constexpr (r == 3) {
                    // ring hand-over: the next chunk of the stream has landed in every wave's view, and this chunk's slot is released
                    if (ahead == D - 1) __builtin_amdgcn_s_waitcnt(0x0F70 | (((D - 2) * NL) & 15) | ((((D - 2) * NL) >> 4) << 14));
                    else __builtin_amdgcn_s_waitcnt(0x0F70);
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                static_for<NGAP>([&](auto gc) {
                    constexpr int g = decltype(gc)::value;
                    constexpr int u = g / NBB, ib = g % NBB;
                    if constexpr (g < NR) read_ops_one(gc, (r + 1) & 1, cA[(r + 1) & 3], cB[(r + 1) & 3]);
                    if constexpr (r == 3) {                             // refill the released slot with the stream's next chunk (if any)
                        constexpr int G0 = NR < NGAP ? NR : NGAP - 1;
                        constexpr int PD = (NGAP - G0) / NL > 0 ? (NGAP - G0) / NL : 1;
                        static_for<NL>([&](auto ic) {
                            constexpr int i = decltype(ic)::value;
                            constexpr int at = G0 + i * PD < NGAP ? G0 + i * PD : NGAP - 1;
                            if constexpr (at == g) {
                                if (fvalid) dma_chunk_piece(fc, sb, i);
                            }
                        });
                    }
                    acc[ib] = mfma32(av[r & 1][0][u], bv[r & 1][ib][u], acc[ib]);
                    __builtin_amdgcn_sched_barrier(0);
                });
            });
            if (fvalid) advance_fetch();
            else --ahead;
            sb = nb;
        }
        lds_wait<0>(av[0]);
#pragma unroll
        for (int k = 0; k < NBB; ++k) asm volatile("" : "+" DMN_TILE_RC(bv[0][k]));

        const int64_t i0_done = i0c;
        const int64_t rows_done = args()->M - i0_done < 128 ? args()->M - i0_done : 128;
        const int next = tile + (int)gridDim.x;
        const bool more = next < ntiles;
        i0c = (int64_t)next * 128;

        // ---- epilogue: each 32 x 32 block goes through this wave's 4 KiB of LDS (lane (li, half) writes column li of its 16 rows;
        // lane l reads 4 consecutive columns of row 8 j + (l >> 3)) and leaves as four 1-KiB stores: 8 rows x 128 bytes.
        auto fresh_v = [](int x) -> int { asm volatile("" : "+v"(x)); return x; };
        KArgs* q = args();
        const int ncols = q->n_out - j0 < NBB * 32 ? q->n_out - j0 : NBB * 32;         // columns of this workgroup that exist (a multiple of 32)
        float* const Ct = q->C + i0_done * q->ldc + j0;
        const rsrc_t rsC = uniform_rsrc(Ct, (rows_done - 1) * q->ldc + ncols);          // rows beyond M fall outside: dropped by the hardware
        const int lane_e = fresh_v(lane);
        const int half_e = lane_e >> 5, li_e = lane_e & 31;
        const int rowB = fresh_v(q->ldc * 4);
        float* const st = lds + (D * BUF) / 4 + w * 1024;
        const int row_l = lane_e >> 3, col_l = 4 * (lane_e & 7);
        const int voC4 = ((32 * w + row_l) * q->ldc + col_l) * 4;
        const int rowB8 = 8 * rowB;
        // which of this lane's four rows (32 w + 8 j + row_l of the tile) are pixels: 1 <= y <= H, 1 <= x <= W inside their image
        bool interior[4];
        {
            const unsigned per = (unsigned)(q->Hp * q->Wp), wp = (unsigned)q->Wp;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned m = (unsigned)(i0_done + 32 * w + 8 * j + row_l);       // (M < 2^31: the host checked)
                const unsigned p = m % per;
                const unsigned y = p / wp, x = p - y * wp;
                interior[j] = y >= 1u && y + 2u <= (unsigned)q->Hp && x >= 1u && x + 2u <= wp;
            }
        }
        const bool do_relu = q->relu != 0;
#pragma unroll
        for (int b = 0; b < NBB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[((r & 3) + 8 * (r >> 2) + 4 * half_e) * 32 + li_e] = acc[b][r];
            const int col0 = 32 * b + col_l;
            const bool in_c = col0 < ncols;
            const int vo = in_c ? voC4 + b * 128 : 0x7ffffff0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(st + (8 * j + row_l) * 32 + col_l);
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = (do_relu && v[e] < 0.f) ? 0.f : v[e];               // keeps a NaN
                    o[e] = interior[j] ? f2u(t) : 0u;                                   // border rows: exact zeros by select
                }
                __builtin_amdgcn_raw_buffer_store_b128(o, rsC, vo + j * rowB8, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!more) break;
        tile = next;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#else
    (void)a;
#endif
}

// Packed weights: out[n][k], k = (3 dy + dx) Cin + c  <-  w[n][c][dy][dx] (torch's [Cout][Cin][3][3]); k >= 9 Cin (only for Cin = 3,
// ldb = 32) zero.
__global__ void conv3x3_pack_kernel(const float* __restrict__ w, int cout, int cin, float* __restrict__ out, int ldb) {
    const int64_t total = (int64_t)cout * ldb;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(e / ldb), k = (int)(e % ldb);
        float v = 0.f;
        if (k < 9 * cin) {
            const int tap = k / cin, c = k - tap * cin;
            v = w[((int64_t)n * cin + c) * 9 + tap];
        }
        out[e] = v;
    }
}

template <int NBB>
int launch_cv(const CvArgs& a, int tiles_n, hipStream_t stream) {
    constexpr int lds_bytes = CvRing<NBB>::D * CvRing<NBB>::BUF + CV_STAGE_BYTES;
    if (int rc = dmn_allow_lds<conv3x3_kernel<NBB>, lds_bytes>("conv3x3")) return rc;
    int dev = 0, cus = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return dmn_fail_hip(e, "conv3x3: hipGetDevice");
    if (hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev); e != hipSuccess || cus < 1)
        return dmn_fail_hip(e, "conv3x3: hipDeviceGetAttribute");
    const int64_t ti = (a.M + 127) / 128;
    const int64_t slots = (int64_t)cus * cv_occupancy(NBB) / tiles_n > 0 ? (int64_t)cus * cv_occupancy(NBB) / tiles_n : 1;
    const int64_t gx = ti < slots ? ti : slots;
    hipLaunchKernelGGL(conv3x3_kernel<NBB>, dim3((unsigned)gx, (unsigned)tiles_n), dim3(256), lds_bytes, stream, a);
    return dmn_check_launch("conv3x3");
}

int cv_blocks(int n_out) {                      // out-blocks per workgroup: all of them up to CV_MAX_NBB, else even tiles (512 = 2 x 8)
    const int nb = n_out / 32;
    if (nb <= CV_MAX_NBB) return nb;
    const int tiles = (nb + CV_MAX_NBB - 1) / CV_MAX_NBB;
    return (nb + tiles - 1) / tiles;
}

}  // namespace

extern "C" int dmnerf_conv3x3_pack(const float* d_w, int Cout, int Cin, float* d_out, int ldb, void* stream) {
    if (Cout < 1 || !(Cin == 3 || (Cin >= 32 && Cin % 32 == 0)) || Cin > 4096 || Cout > 65536)
        return dmn_fail(DMNERF_E_ARG, "conv3x3_pack: bad sizes Cout=%d Cin=%d (Cin = 3 or a multiple of 32)", Cout, Cin);
    if (ldb != (9 * Cin + 31) / 32 * 32) return dmn_fail(DMNERF_E_ARG, "conv3x3_pack: ldb=%d, %d expected", ldb, (9 * Cin + 31) / 32 * 32);
    if (!d_w || !d_out) return dmn_fail(DMNERF_E_ARG, "conv3x3_pack: null pointer");
    const int64_t total = (int64_t)Cout * ldb;
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(conv3x3_pack_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, d_w, Cout, Cin, d_out, ldb);
    return dmn_check_launch("conv3x3_pack");
}

extern "C" int dmnerf_conv3x3(const float* d_in, int64_t in_floats, const float* d_wp, int64_t w_floats, const float* d_bias, float* d_out,
                              int64_t out_floats, int P, int H, int W, int Cin, int Cout, int taps, int relu, void* stream) {
    if (P < 0 || H < 1 || W < 1 || H > 32768 || W > 32768 || Cin < 32 || Cin % 32 || Cout < 32 || Cout % 32 || Cin > 4096 || Cout > 4096 ||
        !(taps == 9 || (taps == 1 && Cin == 32)))
        return dmn_fail(DMNERF_E_ARG, "conv3x3: bad sizes P=%d H=%d W=%d Cin=%d Cout=%d taps=%d", P, H, W, Cin, Cout, taps);
    const int64_t Hp = H + 2, Wp = W + 2, G = W + 3;
    const int64_t M = (int64_t)P * Hp * Wp;
    if (M > 0x7fffff00LL || (2 * Wp + 3 + 128) * (int64_t)Cin * 4 > 0x3fffffffLL || (int64_t)Cout * 4 * 128 > 0x3fffffffLL)
        return dmn_fail(DMNERF_E_ARG, "conv3x3: too many rows for 32-bit tile offsets (P=%d H=%d W=%d)", P, H, W);
    if (P == 0) return DMNERF_OK;
    if (!d_in || !d_wp || !d_out) return dmn_fail(DMNERF_E_ARG, "conv3x3: null pointer");
    if (((uintptr_t)d_in & 15) || ((uintptr_t)d_wp & 15) || ((uintptr_t)d_out & 15)) return dmn_fail(DMNERF_E_ARG, "conv3x3: pointers must be 16-byte aligned");
    const int64_t rows_pf = M + 2 * G;
    const int64_t need_in = (taps == 9 ? rows_pf : M) * Cin;
    if (in_floats < need_in) return dmn_fail(DMNERF_E_ARG, "conv3x3: input holds %lld floats, %lld needed", (long long)in_floats, (long long)need_in);
    if (out_floats < rows_pf * Cout) return dmn_fail(DMNERF_E_ARG, "conv3x3: output holds %lld floats, %lld needed", (long long)out_floats, (long long)(rows_pf * Cout));
    const int ldb = taps * Cin;
    if (w_floats < (int64_t)Cout * ldb) return dmn_fail(DMNERF_E_ARG, "conv3x3: packed weights hold %lld floats, %lld needed", (long long)w_floats, (long long)Cout * ldb);
    hipStream_t s = (hipStream_t)stream;
    // the guard rows of the output
    if (hipError_t e = hipMemsetAsync(d_out, 0, (size_t)(G * Cout * 4), s); e != hipSuccess) return dmn_fail_hip(e, "conv3x3: hipMemsetAsync");
    if (hipError_t e = hipMemsetAsync(d_out + (G + M) * Cout, 0, (size_t)(G * Cout * 4), s); e != hipSuccess) return dmn_fail_hip(e, "conv3x3: hipMemsetAsync");
    CvArgs a{};
    a.A = d_in; a.a_floats = need_in; a.lda = Cin;
    a.run_chunks = (taps == 9 ? 3 : 1) * (Cin / 32);
    a.nchunk = taps * (Cin / 32);
    a.run_step = taps == 9 ? (int)((Wp - 3) * Cin * 4) : 0;
    a.span_rows = taps == 9 ? (int)(2 * Wp + 2) : 0;
    a.B = d_wp; a.b_floats = (int64_t)Cout * ldb; a.ldb = ldb; a.bias = d_bias; a.n_out = Cout;
    a.C = d_out + G * Cout; a.ldc = Cout; a.M = M; a.Hp = (int)Hp; a.Wp = (int)Wp; a.relu = relu;
    const int nbb = cv_blocks(Cout);
    const int tiles = (Cout / 32 + nbb - 1) / nbb;
    switch (nbb) {
        case 1: return launch_cv<1>(a, tiles, s);
        case 2: return launch_cv<2>(a, tiles, s);
        case 3: return launch_cv<3>(a, tiles, s);
        case 4: return launch_cv<4>(a, tiles, s);
        case 5: return launch_cv<5>(a, tiles, s);
        case 6: return launch_cv<6>(a, tiles, s);
        case 7: return launch_cv<7>(a, tiles, s);
        case 8: return launch_cv<8>(a, tiles, s);
        case 9: return launch_cv<9>(a, tiles, s);
        case 10: return launch_cv<10>(a, tiles, s);
        default: return dmn_fail(DMNERF_E_ARG, "conv3x3: unsupported block count %d", nbb);
    }
}
