// mlp_f16_body.inc -- the body of the split-f16 forward kernels, included INSIDE each kernel definition (mlp_f16_impl.h,
// mlp_f16_sparse.hip, mlp_f16_density.hip), which provides: `a` (F16Args), OBX, and the constexpr bools SAVE, SEL, DENS.
// Textual inclusion, not a device function: behind a function wrapper the register allocation of the dense kernels changed
// (a few dozen accumulator copies and s_nops per kernel); this way their code is the parent's.
// SEL: the batch is the sample list a.sel[0 .. *a.count) -- a lane's sample is sel[blk * 32 + lane % 32], its ray sel[..] / Sr, its
// output row sel[..]; the batch size is read on the device and a workgroup beyond it leaves as a whole, before the DMA prologue
// and the first barrier (a.M only sizes the launch).  Tail lanes and tail waves of a live workgroup recompute the last selected
// sample and store nothing, so all four waves reach every barrier.
// DENS: the network cut off behind density_linear -- encoding, mlps.0 .. mlps.7 and density_linear through the SAME f16_pass calls
// on the same tiles in the same order as the full kernel, so the value is raw[..., 3] of the full kernel bit for bit; a.raw is then
// sigma [M].  It reads the f16 density blob (layout.h::make_f16_density_layout): the trunk groups followed by the density groups.
// Without SEL and DENS every `if constexpr` on them drops out: the dense kernels' code is what it was.
    static_assert(!(SAVE && (SEL || DENS)), "the selection and density-only variants are inference kernels");
    extern __shared__ __attribute__((aligned(16))) float lds[];          // [ring 8 x 16 KiB][table 16 KiB]
    float* const tab = lds + F16_RING_FLOATS;
    const int lane = threadIdx.x & 63, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t M = a.M;
    if constexpr (SEL) M = *a.count;                                     // wave-uniform: one scalar load
    const int64_t nblk = (M + 31) / 32;
    if constexpr (SEL) {
        // blockIdx and the count are the same for all four waves, so the workgroup leaves as one: nobody is left waiting in the
        // ring protocol.  count == 0: nblk == 0 and every workgroup leaves here.
        if ((int64_t)blockIdx.x * 4 >= nblk) return;
    }
    const int64_t blk_raw = (int64_t)blockIdx.x * 4 + wave;
    const int64_t blk = blk_raw < nblk ? blk_raw : nblk - 1;             // (a wave beyond the batch duplicates the last block)
    const int64_t m_raw = blk * 32 + (lane & 31);
    const bool valid = m_raw < M;
    int64_t m = valid ? m_raw : M - 1;
    if constexpr (SEL) m = a.sel[m];                                     // (sel is never read at or beyond count)
    const int C = a.S.C;

    DMN_F16_STAMP(0);
    float pt[3], vd[3];
    {
        const int64_t n = m / a.Sr;
        const float ox = a.rays_o[n * 3 + 0], oy = a.rays_o[n * 3 + 1], oz = a.rays_o[n * 3 + 2];
        const float dx = a.rays_d[n * 3 + 0], dy = a.rays_d[n * 3 + 1], dz = a.rays_d[n * 3 + 2];
        const float zv = a.z[m];
        pt[0] = ox + dx * zv; pt[1] = oy + dy * zv; pt[2] = oz + dz * zv;          // render.py:49
        const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
        vd[0] = dx / nrm; vd[1] = dy / nrm; vd[2] = dz / nrm;                       // render.py:37
    }
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(a.blob) + threadIdx.x;
        f32x4* dst = reinterpret_cast<f32x4*>(tab) + threadIdx.x;
#pragma unroll
        for (int k = 0; k < TAB_FLOATS / 1024; ++k) dst[k * 256] = src[k * 256];
    }
    GStream ws;
    ws.rs = uniform_rsrc(a.blob, a.S.total);
    ws.wave = wave;
    ws.voff = (unsigned)(lane * 16 + wave * 1024);
    ws.ring = lds;
    ws.off = __builtin_amdgcn_readfirstlane((unsigned)(a.S.stream * 4));
    ws.gidx = 0;
    ws.lane16 = lds_addr(lds) + lane * 16;
    // prologue: groups 0 .. F16_LA - 1 into ring slots 0 .. F16_LA - 1
#pragma unroll
    for (int g = 0; g < F16_LA; ++g) {
#pragma unroll
        for (int i = 0; i < 4; ++i) gs_fetch_piece(ws, g, i);
        ws.off += F16_GROUP_BYTES;
    }                                                                    // from now on `off` = group gidx + F16_LA

    // SAVE (opt-in training forward): the f32 workspace of layout.h::SaveLayout that the backward kernels consume -- pe, de,
    // the ReLU outputs h_0 .. h_7, g1, g2 as block-major rows (TID-addressed stores, mlp_common.h::RowIO) and the 1-bit masks
    const SaveLayout SL = make_save_layout(a.M);
    const int64_t MP = save_row_len(a.M);
    rsrc_t bits_rs = uniform_rsrc(SAVE ? a.save + SL.bits : a.blob, SAVE ? (int64_t)(BITS_WORDS_PER_BLOCK / 32) * MP : 0);
    auto save_ctx = [&](int64_t tensor_off, int rows, int words_per_lane, int word0) -> SaveCtx {
        SaveCtx c;
        c.io.rs = bits_rs; c.io.soff = 0u; c.bits_rs = bits_rs; c.bits_voff = 0;      // (inference: never used)
        if constexpr (SAVE) {
            c.io = make_rowio(a.save + tensor_off, rows, MP, blk, lane);
            c.bits_rs = bits_rs;
            c.bits_voff = (int)((blk * BITS_WORDS_PER_BLOCK + word0 + lane * words_per_lane) * 4);
        }
        return c;
    };

    // encodings as planes.  The pad slot of the position encoding (k-pair 1, upper half) carries 1.0: the stream holds the bias
    // of mlps.0 in that column (pack.cpp), so the first layer needs no bias table
    unsigned Ppe[2][16], Pde[2][8];
    {
        f32x16 pe[2], de[1];
        encode<POS_L, 2>(pt, pe, half);
        if constexpr (!DENS) encode<DIR_L, 1>(vd, de, half);
        if constexpr (SAVE) {
            store_encoded_rows<POS_L, 2>(a.save + SL.pe, MP, blk, lane, pe);
            store_encoded_rows<DIR_L, 1>(a.save + SL.de, MP, blk, lane, de);
        }
        pe[0][1] = half ? 1.f : pe[0][1];
        split_blocks_f16<2>(pe, Ppe[0], Ppe[1]);
        if constexpr (!DENS) split_blocks_f16<1>(de, Pde[0], Pde[1]);
    }

    // groups 0 and 1 landed (the pieces of groups 2 .. 5 -- and, SAVE, the 90 younger encoding stores -- may still fly), table
    // visible; hi tiles of group 0
    if constexpr (SAVE) wait_vm<63>(); else wait_vm<4 * (F16_LA - 2)>();
    wait_lgkm<0>();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    ws.cur = ws.lane16;
    ws.nxt = ws.lane16 + F16_GROUP_BYTES;
    static_for<8>([&](auto ic) { constexpr int i = decltype(ic)::value; lds_read16_async<i * 1024>(ws.H[i], ws.cur); });

    DMN_F16_STAMP(1);
    f32x16 acc0[2], acc1[2];                   // the two accumulator sets of the trunk passes (even / odd pass)
    unsigned PA[2][64], PB[2][64];             // the two plane sets: 256 features as (hi, lo) words of f16 pairs
    f32x4 bq[16];                              // bias quads: trunk pass p reads ITS OWN 8 into half p & 1 (used one pass later)
    // bias table walk (this lane's half): mlps.1's first pass, then pass by pass
    unsigned baddr = lds_addr(tab) + half * 64 + 256 * 4;
    // activation stores guaranteed younger than the awaited weight pieces at a trunk hand-over: the window back to their issue is
    // 98 gaps, a pass issues 33 stores in gaps 3..66 of its 96 (mlps.5: 120) -- at least 20 fall into any window
    constexpr int VMT = SAVE ? 16 : 0;
    constexpr int NU0 = SAVE ? 4 : 3;          // mlps.0's one-group passes carry their predecessor's epilogue NU0 pairs at a time

    // ---- mlps.0 : 63 -> 256, four passes of one group; the epilogue of pass p - 1 rides in pass p
    const SaveCtx sv0 = save_ctx(SL.h, 256, 4, 0);
    f16_pass<2, 1, 0, 0, 0, 0, true, 0>(ws, Ppe[0], Ppe[1], acc0, bq, baddr, NoSideC{});
    f16_pass<2, 1, 0, 0, 0, 0, true, 0>(ws, Ppe[0], Ppe[1], acc1, bq, baddr, EpiFwd<SAVE, 2, 0, 0, false, true, 3, NU0, 64, 16>{acc0, bq, PA[0], PA[1], &sv0, 0});
    f16_pass<2, 1, 0, 0, 0, 0, true, 0>(ws, Ppe[0], Ppe[1], acc0, bq, baddr, EpiFwd<SAVE, 2, 2, 0, false, true, 3, NU0, 64, 16>{acc1, bq, PA[0], PA[1], &sv0, 4});
    f16_pass<2, 1, 0, 0, 0, 0, true, 0>(ws, Ppe[0], Ppe[1], acc1, bq, baddr, EpiFwd<SAVE, 2, 4, 0, false, true, 3, NU0, 64, 16>{acc0, bq, PA[0], PA[1], &sv0, 8});

    DMN_F16_STAMP(2);
    // ---- mlps.1 .. mlps.7: layer X reads A and writes B, layer Y reads B and writes A; pass p accumulates out-blocks 2p, 2p+1
    // in set p & 1 and reads its own bias quads, while the other set (pass p - 1, or the previous layer's pass 3) is
    // post-processed into its plane words (and, SAVE, stored as h_l).  LAYER = index of the layer that is being accumulated.
    auto layer = [&](auto lc, unsigned (&Pin)[2][64], unsigned (&Pout)[2][64], auto hasq_prev) __attribute__((always_inline)) {
        constexpr int LAYER = decltype(lc)::value;
        constexpr bool PE_ON = LAYER == 5;                               // skip concat [h, pts] (dm_nerf.py:87)
        constexpr bool HQP = decltype(hasq_prev)::value;                 // (mlps.0 has no table bias)
        const SaveCtx svp = save_ctx(SL.h + (int64_t)(LAYER - 1) * 256 * MP, 256, 4, 0);      // the previous layer's outputs
        const SaveCtx svl = save_ctx(SL.h + (int64_t)LAYER * 256 * MP, 256, 4, 0);
        f16_pass<2, 4, 0, 8, 0, 0, true, VMT>(ws, Pin[0], Pin[1], acc0, bq, baddr,
                                              EpiFwd<SAVE, 2, 6, 8, HQP, true, 3, 1, 64, 16>{acc1, bq, Pin[0], Pin[1], &svp, (LAYER - 1) * 1024 + 12});
        baddr += 256;
        if constexpr (PE_ON) f16_pass<2, 1, 0, 0, 0, 96, false, VMT>(ws, Ppe[0], Ppe[1], acc0, bq, baddr, NoSideC{});
        f16_pass<2, 4, 0, 8, 8, 0, true, VMT>(ws, Pin[0], Pin[1], acc1, bq, baddr,
                                              EpiFwd<SAVE, 2, 0, 0, true, true, 3, 1, 64, 16>{acc0, bq, Pout[0], Pout[1], &svl, LAYER * 1024 + 0});
        baddr += 256;
        if constexpr (PE_ON) f16_pass<2, 1, 0, 0, 0, 96, false, VMT>(ws, Ppe[0], Ppe[1], acc1, bq, baddr, NoSideC{});
        f16_pass<2, 4, 0, 8, 0, 0, true, VMT>(ws, Pin[0], Pin[1], acc0, bq, baddr,
                                              EpiFwd<SAVE, 2, 2, 8, true, true, 3, 1, 64, 16>{acc1, bq, Pout[0], Pout[1], &svl, LAYER * 1024 + 4});
        baddr += 256;
        if constexpr (PE_ON) f16_pass<2, 1, 0, 0, 0, 96, false, VMT>(ws, Ppe[0], Ppe[1], acc0, bq, baddr, NoSideC{});
        f16_pass<2, 4, 0, 8, 8, 0, true, VMT>(ws, Pin[0], Pin[1], acc1, bq, baddr,
                                              EpiFwd<SAVE, 2, 4, 0, true, true, 3, 1, 64, 16>{acc0, bq, Pout[0], Pout[1], &svl, LAYER * 1024 + 8});
        baddr += 256;
        if constexpr (PE_ON) f16_pass<2, 1, 0, 0, 0, 96, false, VMT>(ws, Ppe[0], Ppe[1], acc1, bq, baddr, NoSideC{});
    };
    // straight-line: the group index, hence the ring slot and the hand-over parity, are compile-time constants and the whole
    // network is one basic block -- no control-flow merge at which the register allocator could copy a tile in flight
    typedef std::true_type T_;
    layer(std::integral_constant<int, 1>{}, PA, PB, std::false_type{});
    layer(std::integral_constant<int, 2>{}, PB, PA, T_{});
    layer(std::integral_constant<int, 3>{}, PA, PB, T_{});
    layer(std::integral_constant<int, 4>{}, PB, PA, T_{});
    layer(std::integral_constant<int, 5>{}, PA, PB, T_{});
    layer(std::integral_constant<int, 6>{}, PB, PA, T_{});
    layer(std::integral_constant<int, 7>{}, PA, PB, T_{});

    DMN_F16_STAMP(3);
    if constexpr (DENS) {
        // ---- density_linear (dm_nerf.py:101) on h_7 = planes B.  Its first group reads k-blocks 0..7 only, so the epilogue of
        // mlps.7's last pass (out-blocks 6 and 7 = k-blocks 12..15, which the full kernel carries in the rgb hidden pass) rides
        // in that group's gaps 3..20, three pairs per burst.  The plane words do not depend on where they are computed and the
        // two groups' MFMAs are those of the full kernel, so the accumulator is the full kernel's bit for bit.
        f32x16 accD[1];
        const SaveCtx sv7 = save_ctx(SL.h + (int64_t)7 * 256 * MP, 256, 4, 0);
        f16_pass<1, 2, 0, 0, 0, 0, true, 0>(ws, PB[0], PB[1], accD, bq, baddr,
                                            EpiFwd<false, 2, 6, 8, true, true, 3, 3, 64, 16>{acc1, bq, PB[0], PB[1], &sv7, 0});
        DMN_F16_STAMP(4);
        if (valid && half == 0) a.raw[m] = accD[0][0] + tab[F16_TAB_DEN];
    } else {
        // ---- heads on h_7 = planes B (its last two out-blocks arrive under the first groups of the rgb hidden layer)
        f32x16 accR[4], accI[4], accO[1], accD[1], accL[OBX];
        unsigned G1[2][32], G2[2][32];
        const SaveCtx sv7 = save_ctx(SL.h + (int64_t)7 * 256 * MP, 256, 4, 0);
        const SaveCtx svg1 = save_ctx(SL.g1, 128, 2, 2048), svg2 = save_ctx(SL.g2, 128, 2, 2176);
        // rgb hidden' = relu(W' h + W_dirs dirs + b')   (rgb_feature_linear folded in)
        f16_pass<4, 8, 0, 0, 0, 0, true, 0>(ws, PB[0], PB[1], accR, bq, baddr,
                                            EpiFwd<SAVE, 2, 6, 8, true, true, 3, 1, 64, 16>{acc1, bq, PB[0], PB[1], &sv7, 7 * 1024 + 12});
        f16_pass<4, 1, 0, 0, 0, 192, false, 0>(ws, Pde[0], Pde[1], accR, bq, baddr, NoSideC{});
        // ins hidden' = relu(W'' h + b''); reads the rgb hidden layer's bias quads and carries its epilogue (g1)
        f16_pass<4, 8, 0, 16, 0, 0, true, 0>(ws, PB[0], PB[1], accI, bq, baddr,
                                             EpiFwd<SAVE, 4, 0, 0, true, true, 24, 1, 32, 16>{accR, bq, G1[0], G1[1], &svg1, 0});
        baddr += 512;
        // rgb_linear (dm_nerf.py:102) on the rgb hidden planes, then density_linear (:101) on h_7: together they carry the ins
        // hidden layer's epilogue (g2), whose bias quads the first of them reads
        f16_pass<1, 1, 0, 16, 0, 0, true, 0>(ws, G1[0], G1[1], accO, bq, baddr, NoSideC{});
        f16_pass<1, 2, 0, 0, 0, 24, true, 0>(ws, PB[0], PB[1], accD, bq, baddr,
                                             EpiFwd<SAVE, 4, 0, 0, true, true, 24, (SAVE ? 3 : 2), 32, 16>{accI, bq, G2[0], G2[1], &svg2, 0});
        // ins_linear (:103)
        f16_pass<OBX, OBX, 0, 0, 0, 0, true, 0>(ws, G2[0], G2[1], accL, bq, baddr, NoSideC{});

        DMN_F16_STAMP(4);
        // ---- outputs: cat[rgb, density, ins] (dm_nerf.py:105); biases of the three output layers from the table
        float* __restrict__ out_row = a.raw + m * (4 + C);
        if (valid) {
            const float* bt = tab + half * 16;
            if (half == 0) {
                out_row[0] = accO[0][0] + bt[F16_TAB_RGBO + 0];
                out_row[1] = accO[0][1] + bt[F16_TAB_RGBO + 1];
                out_row[2] = accO[0][2] + bt[F16_TAB_RGBO + 2];
                out_row[3] = accD[0][0] + bt[F16_TAB_DEN];
            }
#pragma unroll
            for (int b = 0; b < OBX; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = 32 * b + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (ch < C) out_row[4 + ch] = accL[b][r] + bt[F16_TAB_INSO + b * 32 + r];
                }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the last (landing-zone) fetches
    DMN_F16_STAMP(5);
