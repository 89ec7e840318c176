// Text of the staggered "w80s" GEMM kernel (see gemm_tiled.hip, which includes this file twice).  Set by the including file:
//   MOCA_W80S_NAME    name of the __global__ template <int AMODE, int SHAPE> defined here
//   MOCA_W80S_CAUSAL  true: the MOCA_EP_TATTN epilogue (SHAPE 3) masks key frame > query frame (moca_gemm_params.tattn_causal)
template <int AMODE, int SHAPE>
__global__ __launch_bounds__(512, 2) void MOCA_W80S_NAME(const moca_gemm_params p) {
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass only needs the launch stub; __amdgpu_buffer_rsrc_t is a device-only type)
    constexpr bool CAUSAL = MOCA_W80S_CAUSAL;
    static_assert(!CAUSAL || SHAPE == 3, "the causal mask belongs to the MOCA_EP_TATTN epilogue");
    constexpr bool WIDE = SHAPE == 1, SQ = SHAPE == 2, TQ = SHAPE == 3;
    constexpr int MT = SQ ? 4 : 5, NT = SQ ? 8 : (TQ ? 6 : 5), KS = 32, RB = 64;
    constexpr int WTM = 16 * MT, WTN = 16 * NT;          // wave tile: 80 x 80, 64 x 128, or 80 x 96
    constexpr int TM = SQ ? 256 : (WIDE ? 160 : 320), BN = SQ ? 256 : (WIDE ? 320 : (TQ ? 192 : 160));
    constexpr int A_BYTES = TM * RB, STAGE = A_BYTES + BN * RB;     // 30 KiB per k-tile (32 KiB for 256 x 256 and 320 x 192)
    constexpr int NS = 5;
    constexpr int PPW = 4;                               // DMA instructions per wave per k-tile (30 pieces + 2 repeats; 32 pieces)
    constexpr int NAP = SQ ? 2 : (WIDE ? 2 : 3);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    MOCA_STAMP(0);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = WIDE ? wave >> 2 : wave >> 1, wave_n = WIDE ? wave & 3 : wave & 1;
    const bool late = wave >= 4;                         // the half of the workgroup that runs one barrier behind

    const int tiles_m = (p.M + TM - 1) / TM;
    const int tiles_n = p.N / BN;
    const int nblk = tiles_m * tiles_n * p.splits;
    if (prefetch_block(p, nblk, 512)) return;
    int split = 0, tile_m, tile_n;
    const int xcd_n = p.reserved4_ >> 8;                 // > 1: 2-D XCD partition (host: splits == 1, both tile counts divide)
    if (xcd_n > 1) {
        remap_tile_2d(tiles_m, tiles_n, xcd_n, tile_m, tile_n);
    } else {
        int logical;
        remap_block<BN>(nblk, logical);
        split = logical % p.splits;
        const int tile = logical / p.splits;
        tile_m = tile / tiles_n; tile_n = tile % tiles_n;
    }
    const int m0 = tile_m * TM, n0 = tile_n * BN;

    const int nk_total = 2 * ((p.K + 63) / 64);
    const int kts = 2 * (((p.K + 63) / 64 + p.splits - 1) / p.splits);
    const int kt_begin = split * kts;
    const int nk = min(kt_begin + kts, nk_total) - kt_begin;

    // DMA pieces (16 rows x 64 B each; lane -> row lane >> 2, physical chunk lane & 3).  The operand with 20 pieces ("big": A of
    // the tall tile, W of the wide one) and the one with 10 ("small") are spread over the 8 waves as in w80 / w80b:
    //   j = 0: big piece w      j = 1: big piece 8 + w      j = 2: big piece 16 + w (w < 4)  or  small piece w - 4 (w >= 4)
    //   j = 3: small piece 4 + w (w < 6)  or  small piece 2 + w (w = 6, 7: a repeat, so that every wave issues 4 per k-tile)
    const int lrow = lane >> 2, pch = lane & 3;
    const int lch = pch ^ swz64(lrow);
    const bool flex_is_big = wave < 4;
    const int kt_last_pair = kt_begin + nk - 2;
    BGather<AMODE, NAP, KS> ga(p, lch, kt_begin, kt_last_pair);
    const int small1 = TQ ? 4 + wave : (wave < 6 ? 4 + wave : 2 + wave);    // j = 3 (320 x 192: 12 W pieces, no repeats)
    // SHAPE 3 ("tq", MOCA_EP_TATTN): the rows of an M tile are the 16 frames of 20 neighbouring pixels of one video, gathered by
    // row index -- tile row r = 16 * (pixel - pix0) + frame -- so that the block holds q, k, v of one head for whole temporal
    // sequences and finishes the temporal attention (attention.py:331-352) in its epilogue.  A DMA piece (16 tile rows) = the 16
    // frames of one pixel.
    const int tq_tpv = TQ ? p.HW / 20 : 1;                                   // row tiles per video
    const int tq_b = tile_m / tq_tpv, tq_pb = tile_m - tq_b * tq_tpv;
    auto grow = [&](int tr) -> int { return TQ ? (tq_b * 16 + (tr & 15)) * p.HW + tq_pb * 20 + (tr >> 4) : m0 + tr; };
    // MOCA per-row-group weights (moca_gemm_params.wgroup_rows: GroupNorm folded into the linear that consumes it): the rows of
    // a tile lie inside one group (host-checked), whose W / bias start wg x stride further -- an offset, nothing in the main loop
    const int wg = (AMODE == MOCA_A_LINEAR && p.wgroup_rows > 0) ? m0 / p.wgroup_rows : 0;
    const unsigned wgo = (unsigned)((int64_t)wg * p.wgroup_stride * 2);
    unsigned w_off[3];
    if constexpr (SQ) {                                  // A pieces w and 8 + w, W pieces w and 8 + w
        ga.init_row(0, m0 + wave * 16 + lrow);
        ga.init_row(1, m0 + (8 + wave) * 16 + lrow);
        w_off[0] = (unsigned)(((int64_t)(n0 + wave * 16 + lrow) * p.ldw + lch * 8) * 2);
        w_off[1] = (unsigned)(((int64_t)(n0 + (8 + wave) * 16 + lrow) * p.ldw + lch * 8) * 2);
        w_off[2] = 0;
    } else if constexpr (!WIDE) {
#pragma unroll
        for (int g = 0; g < NAP; ++g) ga.init_row(g, grow((g < 2 ? g * 8 + wave : 16 + (wave & 3)) * 16 + lrow));
        w_off[0] = (unsigned)(((int64_t)(n0 + (wave & 3) * 16 + lrow) * p.ldw + lch * 8) * 2);      // j = 2 (waves 4..7)
        w_off[1] = (unsigned)(((int64_t)(n0 + small1 * 16 + lrow) * p.ldw + lch * 8) * 2);           // j = 3
        w_off[2] = 0;
    } else {
        ga.init_row(0, m0 + (wave & 3) * 16 + lrow);                                                   // j = 2 (waves 4..7)
        ga.init_row(1, m0 + small1 * 16 + lrow);                                                       // j = 3
        w_off[0] = (unsigned)(((int64_t)(n0 + wave * 16 + lrow) * p.ldw + lch * 8) * 2);             // j = 0
        w_off[1] = (unsigned)(((int64_t)(n0 + (8 + wave) * 16 + lrow) * p.ldw + lch * 8) * 2);       // j = 1
        w_off[2] = (unsigned)(((int64_t)(n0 + (16 + (wave & 3)) * 16 + lrow) * p.ldw + lch * 8) * 2); // j = 2 (waves 0..3)
    }
    if (wgo) { w_off[0] += wgo; w_off[1] += wgo; w_off[2] += wgo; }
    // (two-source A, MOCA_A_LINEAR2: the A descriptor follows the gather's block-uniform source index -- `sync_src()` behind every
    //  ga.seek() / ga.advance(); one scalar compare per k-tile pair, the other modes compile to the constant descriptors)
    __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, OOB_OFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, OOB_OFF, 0x00020000);
    __amdgpu_buffer_rsrc_t rsrc_f = (flex_is_big != WIDE) ? rsrc_a : rsrc_w;            // descriptor of this wave's j = 2 piece
    auto sync_src = [&]() {
        if constexpr (AMODE == MOCA_A_LINEAR2) {
            if (ga.tap == 1) {
                rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a2), 0, OOB_OFF, 0x00020000);
                if (flex_is_big != WIDE) rsrc_f = rsrc_a;
            }
        }
    };

    auto dma_piece = [&](int slot, int j, auto odd_tag) {
        constexpr int odd = decltype(odd_tag)::value;
        const lds_ptr sa = (lds_ptr)smem + slot * STAGE;
        const unsigned a_s = ga.a_soff() + odd * KS * 2, w_s = ga.w_soff() + odd * KS * 2;
        if constexpr (SQ) {
            if (j < 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, sa + (j * 8 + wave) * 1024, 16, ga.a_off[j], a_s, 0, 0);
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, sa + A_BYTES + ((j - 2) * 8 + wave) * 1024, 16, w_off[j - 2], w_s, 0, 0);
        } else if constexpr (!WIDE) {
            if (j < 2) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, sa + (j * 8 + wave) * 1024, 16, ga.a_off[j], a_s, 0, 0);
            } else if (j == 2) {
                const lds_ptr dst = flex_is_big ? sa + (16 + (wave & 3)) * 1024 : sa + A_BYTES + (wave & 3) * 1024;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_f, dst, 16, flex_is_big ? ga.a_off[2] : w_off[0], flex_is_big ? a_s : w_s, 0, 0);
            } else {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, sa + A_BYTES + small1 * 1024, 16, w_off[1], w_s, 0, 0);
            }
        } else {
            if (j < 2) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, sa + A_BYTES + (j * 8 + wave) * 1024, 16, w_off[j], w_s, 0, 0);
            } else if (j == 2) {
                const lds_ptr dst = flex_is_big ? sa + A_BYTES + (16 + (wave & 3)) * 1024 : sa + (wave & 3) * 1024;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_f, dst, 16, flex_is_big ? w_off[2] : ga.a_off[0], flex_is_big ? w_s : a_s, 0, 0);
            } else {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, sa + small1 * 1024, 16, ga.a_off[1], a_s, 0, 0);
            }
        }
    };
    auto issue_pair = [&](int slot_even, int slot_odd) {
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            dma_piece(slot_even, j, int_c<0>{});
            dma_piece(slot_odd, j, int_c<1>{});
        }
    };

    const int fr = lane & 15, fg = lane >> 4;
    f32x4 acc[MT][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (p.bias && p.splits == 1 && !(p.flags & MOCA_EP_LNFOLD)) bv = *reinterpret_cast<const f32x4*>(p.bias + (int64_t)wg * p.N + n0 + wave_n * WTN + nt * 16 + 4 * fg);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = bv;
    }

    // (swz64(fr), written out: through the helper the SHAPE 3 kernels leave their encodings, the causal one two instructions longer)
    const int swz = (fg ^ ((0x78 >> (2 * ((fr >> 2) & 3))) & 3)) << 4;
    const int a_off0 = (wave_m * WTM + fr) * RB + swz;
    const int b_off0 = A_BYTES + (wave_n * WTN + fr) * RB + swz;

    half8v af[2][MT], bf[2][NT];
    auto read_tile = [&](auto set_tag, int slot) {
        constexpr int S = decltype(set_tag)::value;
        const char* cur = smem + slot * STAGE;
#pragma unroll
        for (int r = 0; r < NT; ++r) bf[S][r] = *reinterpret_cast<const half8v*>(cur + b_off0 + r * 1024);
#pragma unroll
        for (int r = 0; r < MT; ++r) af[S][r] = *reinterpret_cast<const half8v*>(cur + a_off0 + r * 1024);
    };
    auto mfma_tile = [&](auto set_tag) {
        constexpr int S = decltype(set_tag)::value;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[S][nt], af[S][mt], acc[mt][nt], 0, 0, 0);   // D^T: lane = row m
        __builtin_amdgcn_s_setprio(0);
    };

    // ---- prologue: pairs (0,1) and (2,3) in flight, pair (0,1) landed everywhere ----
    LnFoldRaw lraw = {float2{0.f, 0.f}, float2{0.f, 0.f}, 0.f, 0.f};
    if (p.flags & MOCA_EP_LNFOLD) lraw = lnfold_issue<TM, BN>(p, grow(tid), n0 + tid, tid);
    ga.seek(kt_begin);
    sync_src();
    issue_pair(0, 1);
    ga.advance();
    sync_src();
    issue_pair(2, 3);
    LnFoldRegs lf = {0.f, 0.f, 0.f, 0.f};
    if (p.flags & MOCA_EP_LNFOLD) lf = lnfold_finish<TM, BN>(p, lraw, grow(tid), tid);
    MOCA_STAMP(1);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPW) : "memory");
    __builtin_amdgcn_s_barrier();
    MOCA_STAMP(2);
    if (late) __builtin_amdgcn_s_barrier();            // from here on waves 4..7 run one barrier behind waves 0..3

    int s0 = 0;                                          // ring slot of tile i
    for (int i = 0; i < nk; i += 2) {
        const int s1 = s0 + 1 == NS ? 0 : s0 + 1;        // tile i+1
        const int sp = s0 == 0 ? NS - 1 : s0 - 1;        // tile i-1 (consumed) -> tile i+4
#if defined(W80S_VARIANT) && W80S_VARIANT == 0    // (A/B build: both fragment sets read in LOADe, MFMAe pure; 1-3 % slower)
        // ---- LOADe ----
        read_tile(int_c<0>{}, s0);
        read_tile(int_c<1>{}, s1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        // ---- MFMAe ----
        mfma_tile(int_c<0>{});
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
#else
#if defined(W80S_GN_DIAG)
        // DIAGNOSTIC build only (results wrong by construction; `make gndiag`, profiles/r04_ab_gn_in_consumer.txt): what a GroupNorm
        // apply + SiLU fused into this consumer would cost as a pass over the LANDED A k-tiles -- each wave rewrites its eighth of the
        // A rows of tiles i and i+1 (affine + SiLU per element, as gn_apply does) before anyone reads fragments, one more barrier.
        if constexpr (AMODE != MOCA_A_LINEAR && !SQ && !TQ) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                char* base = smem + (t == 0 ? s0 : s1) * STAGE;
                for (int c = tid; c < A_BYTES / 16; c += 512) {
                    half8v v = *reinterpret_cast<half8v*>(base + c * 16);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (half_t)moca_silu((float)v[j] * 1.0009765625f + 0.0009765625f);
                    *reinterpret_cast<half8v*>(base + c * 16) = v;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
#endif
        // ---- LOADe: tile i only ----
#ifdef MOCA_STAMPS
        const bool seg = i == SEG_ITER;
        if (seg) MOCA_STAMP_W(8, SEG_WAVE);
#endif
        read_tile(int_c<0>{}, s0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#ifdef MOCA_STAMPS
        if (seg) MOCA_STAMP_W(9, SEG_WAVE);
#endif
        __builtin_amdgcn_s_barrier();
#ifdef MOCA_STAMPS
        if (seg) MOCA_STAMP_W(10, SEG_WAVE);
#endif
        // ---- MFMAe with the reads of tile i+1 in the gaps ----
        {
            const char* nx = smem + s1 * STAGE;
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int j = 0; j < MT * NT; ++j) {
                const int mt = j / NT, nt = j % NT;
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[0][nt], af[0][mt], acc[mt][nt], 0, 0, 0);
                if (j % 2 == 0 && j / 2 < MT + NT) {
                    const int r = j / 2;
                    __builtin_amdgcn_sched_barrier(0);
                    if (r < NT) bf[1][r] = *reinterpret_cast<const half8v*>(nx + b_off0 + r * 1024);
                    else af[1][r - NT] = *reinterpret_cast<const half8v*>(nx + a_off0 + (r - NT) * 1024);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#ifdef MOCA_STAMPS
        if (seg) MOCA_STAMP_W(11, SEG_WAVE);
#endif
        __builtin_amdgcn_s_barrier();
#ifdef MOCA_STAMPS
        if (seg) MOCA_STAMP_W(12, SEG_WAVE);
#endif
#endif
        // ---- LOADo ----
        ga.advance();
        sync_src();
        issue_pair(sp, s0);
#ifdef MOCA_STAMPS
        if (seg) MOCA_STAMP_W(13, SEG_WAVE);
#endif
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPW) : "memory");
        __builtin_amdgcn_sched_barrier(0);
#ifdef MOCA_STAMPS
        if (seg) MOCA_STAMP_W(14, SEG_WAVE);
#endif
        __builtin_amdgcn_s_barrier();
#ifdef MOCA_STAMPS
        if (seg) MOCA_STAMP_W(15, SEG_WAVE);
#endif
        // ---- MFMAo ----
        mfma_tile(int_c<1>{});
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        s0 = s1 + 1 == NS ? 0 : s1 + 1;
    }
    if (!late) __builtin_amdgcn_s_barrier();           // the halves meet again
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                      // every DMA (incl. the repeats) is done: the ring is free for the epilogue
    MOCA_STAMP(3);

    // ---- epilogue (as w80): lane owns 4 consecutive columns n = wave_n*80 + nt*16 + 4*fg + r of row m = wave_m*80 + mt*16 + fr ----
    if (p.splits > 1) {
        float* ws = p.splitk_ws + (int64_t)split * p.M * p.N;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int row = m0 + wave_m * WTM + mt * 16 + fr;
            if (row < p.M) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int col = n0 + wave_n * WTN + nt * 16 + 4 * fg;
                    *reinterpret_cast<f32x4*>(ws + (int64_t)row * p.N + col) = acc[mt][nt];
                }
            }
        }
        return;
    }
    const bool fold = (p.flags & MOCA_EP_LNFOLD) != 0;
    if constexpr (SQ) {
        if (p.flags & MOCA_EP_GEGLU) {                   // per 64-column group: value tiles +0, +1 and their gate tiles +2, +3 (bias is in the accumulators)
            constexpr int gpitch = (BN / 2) * 2 + 16;
            float* rst = reinterpret_cast<float*>(smem + TM * gpitch);
            if (fold) lnfold_publish<TM, BN>(lf, rst, tid);
#pragma unroll
            for (int grp = 0; grp < 2; ++grp)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int lcol = wave_n * WTN + grp * 64 + nt * 16 + 4 * fg;
                    f32x4 wv = {0.f, 0.f, 0.f, 0.f}, wg = wv, bv = wv, bg = wv;
                    if (fold) {
                        wv = *reinterpret_cast<const f32x4*>(rst + 2 * TM + lcol); wg = *reinterpret_cast<const f32x4*>(rst + 2 * TM + lcol + 32);
                        bv = *reinterpret_cast<const f32x4*>(rst + 2 * TM + BN + lcol); bg = *reinterpret_cast<const f32x4*>(rst + 2 * TM + BN + lcol + 32);
                    }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const int row = wave_m * WTM + mt * 16 + fr;
                        f32x4 va = acc[mt][4 * grp + nt], gt = acc[mt][4 * grp + nt + 2];
                        if (fold) {
                            const float2 st = *reinterpret_cast<const float2*>(rst + 2 * row);
                            va = lnfold_apply(va, st, wv, bv); gt = lnfold_apply(gt, st, wg, bg);
                        }
                        const f32x2 lo = moca_geglu2(f32x2{va[0], va[1]}, f32x2{gt[0], gt[1]});
                        const f32x2 hi = moca_geglu2(f32x2{va[2], va[3]}, f32x2{gt[2], gt[3]});
                        half4v h;
                        h[0] = (half_t)lo[0]; h[1] = (half_t)lo[1]; h[2] = (half_t)hi[0]; h[3] = (half_t)hi[1];
                        *reinterpret_cast<half4v*>(smem + row * gpitch + (wave_n * 64 + grp * 32 + nt * 16 + 4 * fg) * 2) = h;
                    }
                }
            __syncthreads();
            MOCA_STAMP(4);
            store_fp16_tile<512>(p, smem, gpitch, TM, BN / 2, m0, n0 / 2, tid);
            MOCA_STAMP(5);
            MOCA_STAMP_HW();
            return;
        }
    }
    constexpr int pitch = BN * 2 + 16;
    if (fold) {                                          // Linear(LayerNorm(x)) from x: row statistics -> LDS behind the staged tile
        float* rst = reinterpret_cast<float*>(smem + TM * pitch);
        lnfold_publish<TM, BN>(lf, rst, tid);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = wave_n * WTN + nt * 16 + 4 * fg;
            const f32x4 ws4 = *reinterpret_cast<const f32x4*>(rst + 2 * TM + col);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(rst + 2 * TM + BN + col);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int row = wave_m * WTM + mt * 16 + fr;
                const float2 st = *reinterpret_cast<const float2*>(rst + 2 * row);
                *reinterpret_cast<half4v*>(smem + row * pitch + col * 2) = __builtin_convertvector(lnfold_apply(acc[mt][nt], st, ws4, b4), half4v);
            }
        }
    } else {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = wave_n * WTN + nt * 16 + 4 * fg;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int row = wave_m * WTM + mt * 16 + fr;
                *reinterpret_cast<half4v*>(smem + row * pitch + col * 2) = __builtin_convertvector(acc[mt][nt], half4v);
            }
        }
    }
    __syncthreads();
    MOCA_STAMP(4);
    if constexpr (TQ) {
        // temporal attention of the 20 pixels of this tile for head tile_n: q | k | v = columns [0,64) | [64,128) | [128,192) of the
        // staged fp16 rows, 16 frames per pixel.  One wavefront per pixel (pixels w, w + 8, w + 16); the arithmetic is that of
        // temporal_attention_kernel (attention.hip): S^T = K.Q^T by v_mfma_f32_16x16x32_f16, softmax over the 16 keys in-lane
        // + two cross-lane steps, O^T = V^T.P^T by v_mfma_f32_16x16x16_f16.  Only O (64 of the 192 columns) goes to memory.
        const float sl2e = p.tattn_scale * 1.4426950408889634f;
        half_t* outp = reinterpret_cast<half_t*>(p.out);
        // Round 5 (profiles/r05_ab_tattn_epilogue.txt): this epilogue was 5.0 k of a tile's 30 k cycles -- a wave ran its 2-3 pixels one
        // after the other, each a chain of LDS reads -> MFMA -> cross-lane maximum -> exp -> cross-lane sum -> 64 two-byte LDS reads of V ->
        // MFMA.  Now (a) the wave's three pixel slots are computed side by side (uniform control flow: slot 2 of waves 4..7 repeats pixel
        // 19 and only skips its stores), so the chains overlap; (b) the cross-lane steps are v_permlane16/32_swap (VALU) instead of
        // ds_bpermute; (c) V^T fragments come from ONE ds_read_b64_tr_b16 per 16 columns instead of 16 two-byte reads.  Same values, same
        // order of additions.
        constexpr int NPX = 3;
        int pixs[NPX];
        half8v kf[NPX][2], qf[NPX][2];
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            pixs[i] = min(wave + 8 * i, 19);
            const char* base = smem + (pixs[i] * 16) * pitch;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                qf[i][ks] = *reinterpret_cast<const half8v*>(base + fr * pitch + (ks * 32 + fg * 8) * 2);
                kf[i][ks] = *reinterpret_cast<const half8v*>(base + fr * pitch + (64 + ks * 32 + fg * 8) * 2);
            }
        }
        half4v vfr[NPX][4];                                   // V^T fragments: lane (d = fr, keys 4 fg .. 4 fg + 3) of column block dt
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            const char* base = smem + (pixs[i] * 16) * pitch;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                vfr[i][dt] = lds_tr_read_b64(base + (4 * fg + (fr >> 2)) * pitch + (128 + dt * 16 + 4 * (fr & 3)) * 2);
        }
        f32x4 sc[NPX];
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            sc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            sc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[i][0], qf[i][0], sc[i], 0, 0, 0);
            sc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[i][1], qf[i][1], sc[i], 0, 0, 0);
        }
        if constexpr (CAUSAL) {
            // attention.py:342-346 -> :101-105: frame fr attends to frames <= fr.  A key above the query is -inf before the row maximum
            // (the diagonal is never masked: the maximum is finite, exp2f(-inf) = 0 exactly, as masked_fill_(-finfo.max) + softmax gives)
#pragma unroll
            for (int i = 0; i < NPX; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * fg + r > fr) sc[i][r] = -INFINITY;
        }
        half4v pf[NPX];
        float inv[NPX];
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            float mx = fmaxf(fmaxf(sc[i][0], sc[i][1]), fmaxf(sc[i][2], sc[i][3]));       // lane: S^T[key = 4 fg + r][query = fr]
            mx = xlane16_max(mx);
            mx = xlane32_max(mx);
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = exp2f((sc[i][r] - mx) * sl2e);
                sum += pv;
                pf[i][r] = (half_t)pv;
            }
            sum = xlane16_sum(sum);
            sum = xlane32_sum(sum);
            inv[i] = 1.0f / sum;
        }
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            half_t* ob = outp + (int64_t)grow(pixs[i] * 16 + fr) * p.ldo + tile_n * 64;
            const bool live = wave + 8 * i < 20;               // (wave-uniform)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                f32x4 o4 = {0.f, 0.f, 0.f, 0.f};
                o4 = __builtin_amdgcn_mfma_f32_16x16x16f16(vfr[i][dt], pf[i], o4, 0, 0, 0);     // lane: O^T[d = 16 dt + 4 fg + r][query = fr]
                half4v h4;
#pragma unroll
                for (int r = 0; r < 4; ++r) h4[r] = (half_t)(o4[r] * inv[i]);
                if (live) *reinterpret_cast<half4v*>(ob + dt * 16 + 4 * fg) = h4;
            }
        }
    } else if constexpr (SQ) {
        store_fp16_tile<512>(p, smem, pitch, TM, BN, m0, n0, tid);
    } else if constexpr (WIDE) {
        if (p.flags & MOCA_EP_LN) store_fp16_tile_ln(p, smem, reinterpret_cast<float*>(smem + TM * pitch), pitch, m0, tid);
        else if (p.flags & (MOCA_EP_COLSUM | MOCA_EP_GSTAT)) store_fp16_tile_colsum<TM, BN>(p, smem, reinterpret_cast<float*>(smem + TM * pitch), pitch, m0, n0, tile_m, tid);
        else if (p.flags & MOCA_EP_ROWSUM) store_fp16_tile_rowsum<512, BN, 8>(p, smem, pitch, TM, m0, n0, tid);
        else store_fp16_tile<512>(p, smem, pitch, TM, BN, m0, n0, tid);
    } else {
        if (p.flags & (MOCA_EP_COLSUM | MOCA_EP_GSTAT)) store_fp16_tile_colsum<TM, BN>(p, smem, reinterpret_cast<float*>(smem + TM * pitch), pitch, m0, n0, tile_m, tid);
        else if (p.flags & MOCA_EP_ROWSUM) store_fp16_tile_rowsum<512, BN, 4>(p, smem, pitch, TM, m0, n0, tid);
        else store_fp16_tile<512>(p, smem, pitch, TM, BN, m0, n0, tid);
    }
    MOCA_STAMP(5);
    MOCA_STAMP_HW();
#endif
}
