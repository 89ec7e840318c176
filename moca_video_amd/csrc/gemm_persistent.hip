// The persistent GEMM kernels of the linears: a fixed grid (G4P_BLOCKS / SQP_BLOCKS, gemm_launch.h) walks the tiles, the DMA stream
// never stops between tiles and the epilogue goes from registers to memory:
//   gemm_g4p_kernel / gemm_g4q_kernel<GEGLU>  the persistent form of g4 (gemm_tiled.hip): ONE body (g4p_body), instantiated on either
//                                             MFMA shape (G4pMma16 / G4pMma32: what a wave holds of the tile and where it goes)
//   gemm_sqp_kernel<GEGLU>                     the persistent form of the 256 x 256 staggered kernel (gemm_tiled.hip)
// Which calls they run: persistent_ok() / route_of() in gemm.hip.  What they share with each other and with the tiled kernels --
// swz64, xcd_range, the LayerNorm-fold statistics (lnfold_*), the plain store store8_rowadd_res -- is in gemm_device.h.
#include "gemm_launch.h"

namespace {

// =====================================================================================
// "g4p" kernel: the two-blocks-per-CU 256 x 128 x 32 structure of g4 as a PERSISTENT kernel for the linears (A mode LINEAR).
// Phase stamps of g4 / the 256 x 256 staggered kernel on the GEGLU projection of the 320-channel level
// (profiles/r05_g4_phase_stamps.txt): of a tile's ~30 k cycles the main loop is 42-44 %; 10-16 % go to the prologue (row set-up,
// first DMA round trip), 30-35 % to the accumulator -> LDS staging pass with the erf-GELU, 8-10 % to the store loop.  Here
//   * a block walks its tiles (XCD-local order: the blocks of an XCD work on consecutive tiles of the tile_m-major raster, so an A
//     row tile is fetched from beyond L2 once and then hit by the blocks that own its other column tiles);
//   * the DMA stream never stops: the last even phase of a tile issues the first k-tile pair of the NEXT tile (per-lane offsets
//     switched just before), so there is no prologue except the block's first;
//   * the ring is never used for staging: W rows are fetched into the LDS tile in a PERMUTED order (free -- the source address of
//     an LDS-DMA is per lane) chosen so that the 4 + 4 accumulator columns a lane holds in two neighbouring 16-column MFMA tiles are
//     8 CONSECUTIVE output columns: the epilogue goes from registers to memory as 16-byte stores (16 rows x 64 B per instruction),
//     no LDS pass, no barrier, and it runs while the next tile's first pair is in flight;
//   * LayerNorm-fold statistics of a tile (row: rstd, -mean rstd; column: wsum, bias) are fetched at the tile's start and
//     published in 3 KiB of LDS behind the ring.
// Buffer-addressed DMA (SGPR descriptors, 32-bit per-lane offsets, out-of-range = zero fill) as in the staggered kernels.
// "g4q" is the same kernel on v_mfma_f32_32x32x16_f16 (MOCA_TUNE_GEMM_MF32; slower in the A/B, profiles/r05_ab_g4p_mfma_shape.txt).
// =====================================================================================
// LDS row rho (0..127) of the W tile <- packed W row n0 + g4p_perm(rho): MFMA tile nt = (rho >> 4) & 3, column j = rho & 15 of wave
// column wn = rho >> 6 holds output column  wn * 64 + (nt >> 1) * 32 + 8 (j >> 2) + 4 (nt & 1) + (j & 3)  of the tile
__device__ __forceinline__ int g4p_perm(int rho) {
    const int wn = rho >> 6, nt = (rho >> 4) & 3, j = rho & 15;
    return wn * 64 + (nt >> 1) * 32 + 8 * (j >> 2) + 4 * (nt & 1) + (j & 3);
}
// W-row permutation for the 32x32x16 operand map (g4q): LDS row rho -> tile nt = (rho >> 5) & 1 of wave column wn = rho >> 6, MFMA row i = rho & 31 =
// 8 g + 4 h + r (g = accumulator register group, h = lane >> 5) holds column 16 (g >> 1) + 8 h + 4 (g & 1) + r of the tile's 32.
__device__ __forceinline__ int g4q_perm(int rho) {
    const int wn = rho >> 6, nt = (rho >> 5) & 1, i = rho & 31;
    const int g = i >> 3, h = (i >> 2) & 1, r = i & 3;
    return wn * 64 + nt * 32 + 16 * (g >> 1) + 8 * h + 4 * (g & 1) + r;
}
#if defined(__HIP_DEVICE_COMPILE__)
// value tiles (lo, hi = columns 0..3, 4..7) and their gate tiles -> eight GEGLU outputs
__device__ __forceinline__ half8v g4p_geglu8(const f32x4 vlo, const f32x4 vhi, const f32x4 glo, const f32x4 ghi) {
    const f32x4 v[2] = {vlo, vhi}, g[2] = {glo, ghi};
    half8v h;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x2 lo = moca_geglu2(f32x2{v[i][0], v[i][1]}, f32x2{g[i][0], g[i][1]});
        const f32x2 hi = moca_geglu2(f32x2{v[i][2], v[i][3]}, f32x2{g[i][2], g[i][3]});
        h[4 * i + 0] = (half_t)lo[0]; h[4 * i + 1] = (half_t)lo[1]; h[4 * i + 2] = (half_t)hi[0]; h[4 * i + 3] = (half_t)hi[1];
    }
    return h;
}
// eight consecutive plain columns (lo, hi) of row m from `col`: + row add, + residual, store
__device__ __forceinline__ void g4p_store8(const moca_gemm_params& p, int m, int col, const f32x4 lo, const f32x4 hi, const half_t* rowadd,
                                           const half_t* resid, bool nt_out) {
    float o[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) { o[r] = lo[r]; o[4 + r] = hi[r]; }
    store8_rowadd_res(p, m, col, o, rowadd, resid, nt_out);
}

// What a wave holds of the 256 x 128 tile (wave tile 128 x 64 = MT x NT MFMA tiles of ROWS rows, KF fragment k-steps per 32-deep k-tile)
// and where it goes: the body below is written on these.  A lane's place in the operand map: fr = its row of an MFMA tile, fk = its
// 16-byte k chunk within a k-step; lst / lws / lbi = the published statistics (lnfold_publish's layout).
struct G4pLane { int fr, fk, wave_m, wave_n; const float *lst, *lws, *lbi; };

// v_mfma_f32_16x16x32_f16: 8 x 4 tiles, one k-step per k-tile (32 MFMAs per phase)
struct G4pMma16 {
    static constexpr int MT = 8, NT = 4, ROWS = 16, KF = 1;
    typedef f32x4 acc_t;
    static __device__ __forceinline__ int perm(int rho) { return g4p_perm(rho); }
    static __device__ __forceinline__ acc_t mfma(half8v b, half8v a, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(b, a, c, 0, 0, 0); }   // D^T: lane = row m
    static __device__ __forceinline__ int dma_after(int j) { return (j % 5 == 2 && j / 5 < 6) ? j / 5 : -1; }      // DMA piece issued behind MFMA j
    static __device__ __forceinline__ void read(const char* cur, const int (&fa_off)[MT][KF], const int (&fb_off)[NT][KF], half8v (&af)[MT][KF], half8v (&bf)[NT][KF]) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt][0] = *reinterpret_cast<const half8v*>(cur + fa_off[mt][0]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bf[nt][0] = *reinterpret_cast<const half8v*>(cur + fb_off[nt][0]);
    }
    // lane = row m0 + wave_m * 128 + mt * 16 + fr, 8 consecutive columns per tile pair
    template <bool GEGLU>
    static __device__ __forceinline__ void epilogue(const moca_gemm_params& p, const acc_t (&acc)[MT][NT], const G4pLane& l, int m0, int n0,
                                                    const half_t* rowadd, const half_t* resid, bool nt_out) {
        const int fr = l.fr, fg = l.fk, wave_m = l.wave_m, wave_n = l.wave_n;
        f32x4 cw[NT], cb[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            cw[nt] = *reinterpret_cast<const f32x4*>(l.lws + wave_n * 64 + nt * 16 + 4 * fg);
            cb[nt] = *reinterpret_cast<const f32x4*>(l.lbi + wave_n * 64 + nt * 16 + 4 * fg);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int rl = wave_m * 128 + mt * 16 + fr;
            const int m = m0 + rl;
            const float2 st = *reinterpret_cast<const float2*>(l.lst + 2 * rl);
            f32x4 v[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) v[nt] = lnfold_apply(acc[mt][nt], st, cw[nt], cb[nt]);
            if constexpr (GEGLU) {
                // value tiles 0, 1 and their gate tiles 2, 3 -> output columns on0 + wave_n * 32 + 8 fg + (0..7)
                const half8v h = g4p_geglu8(v[0], v[1], v[2], v[3]);
                if (m < p.M) st_out8(reinterpret_cast<half_t*>(p.out) + (int64_t)m * p.ldo + (n0 >> 1) + wave_n * 32 + 8 * fg, h, nt_out);
            } else {
#pragma unroll
                for (int hh = 0; hh < 2; ++hh)
                    g4p_store8(p, m, n0 + wave_n * 64 + hh * 32 + 8 * fg, v[2 * hh], v[2 * hh + 1], rowadd, resid, nt_out);
            }
        }
    }
};

// v_mfma_f32_32x32x16_f16 ("g4q"): 4 x 2 tiles, two k-steps per k-tile (16 MFMAs per phase).  The kernel is bound by the SIMDs' issue
// port (an MFMA of either shape holds it for 8 cycles): half as many MFMA instructions for the same matrix cycles, the same fragment bytes.
struct G4pMma32 {
    static constexpr int MT = 4, NT = 2, ROWS = 32, KF = 2;
    typedef f32x16 acc_t;
    static __device__ __forceinline__ int perm(int rho) { return g4q_perm(rho); }
    static __device__ __forceinline__ acc_t mfma(half8v b, half8v a, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(b, a, c, 0, 0, 0); }   // D^T: lane & 31 = row m
    static __device__ __forceinline__ int dma_after(int j) { return ((j & 1) && j / 2 < 6) ? j / 2 : -1; }
    static __device__ __forceinline__ void read(const char* cur, const int (&fa_off)[MT][KF], const int (&fb_off)[NT][KF], half8v (&af)[MT][KF], half8v (&bf)[NT][KF]) {
#pragma unroll
        for (int ks = 0; ks < KF; ++ks) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bf[nt][ks] = *reinterpret_cast<const half8v*>(cur + fb_off[nt][ks]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) af[mt][ks] = *reinterpret_cast<const half8v*>(cur + fa_off[mt][ks]);
        }
    }
    // lane = row m0 + wave_m * 128 + mt * 32 + (lane & 31); accumulator registers 4 g + r of a tile are (permuted W rows) columns
    // 16 (g >> 1) + 8 (lane >> 5) + 4 (g & 1) + r of the tile's 32
    // (the 16 column constants of a lane stay in registers for the GEGLU form; the plain form, which also holds row add / residual
    //  operands, re-reads them from LDS per use)
    template <bool GEGLU>
    static __device__ __forceinline__ void epilogue(const moca_gemm_params& p, const acc_t (&acc)[MT][NT], const G4pLane& l, int m0, int n0,
                                                    const half_t* rowadd, const half_t* resid, bool nt_out) {
        const int fr = l.fr, fh = l.fk, wave_m = l.wave_m, wave_n = l.wave_n;
        f32x4 cw[NT][4], cb[NT][4];
        auto constants = [&](int nt, int g) {
            cw[nt][g] = *reinterpret_cast<const f32x4*>(l.lws + wave_n * 64 + nt * 32 + 8 * g + 4 * fh);
            cb[nt][g] = *reinterpret_cast<const f32x4*>(l.lbi + wave_n * 64 + nt * 32 + 8 * g + 4 * fh);
        };
        if constexpr (GEGLU) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) constants(nt, g);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int rl = wave_m * 128 + mt * 32 + fr;
            const int m = m0 + rl;
            const float2 st = *reinterpret_cast<const float2*>(l.lst + 2 * rl);
#pragma unroll
            for (int s = 0; s < 2; ++s) {                        // store s: registers g = 2 s, 2 s + 1 -> 8 consecutive columns 16 s + 8 fh
                f32x4 v[NT][2];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int gg = 0; gg < 2; ++gg) {
                        const int g = 2 * s + gg;
                        const f32x4 a4 = {acc[mt][nt][4 * g], acc[mt][nt][4 * g + 1], acc[mt][nt][4 * g + 2], acc[mt][nt][4 * g + 3]};
                        if constexpr (!GEGLU) constants(nt, g);
                        v[nt][gg] = lnfold_apply(a4, st, cw[nt][g], cb[nt][g]);
                    }
                if constexpr (GEGLU) {                           // value tile 0, gate tile 1
                    const half8v h = g4p_geglu8(v[0][0], v[0][1], v[1][0], v[1][1]);
                    if (m < p.M) st_out8(reinterpret_cast<half_t*>(p.out) + (int64_t)m * p.ldo + (n0 >> 1) + wave_n * 32 + 16 * s + 8 * fh, h, nt_out);
                } else {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        g4p_store8(p, m, n0 + wave_n * 64 + nt * 32 + 16 * s + 8 * fh, v[nt][0], v[nt][1], rowadd, resid, nt_out);
                }
            }
        }
    }
};

template <bool GEGLU, typename MMA>
__device__ __forceinline__ void g4p_body(const moca_gemm_params& p) {
    constexpr int TM = 256, BN = 128, KS = 32, RB = 64, MT = MMA::MT, NT = MMA::NT, KF = MMA::KF;
    constexpr int A_BYTES = TM * RB, STAGE = A_BYTES + BN * RB, RING = 3 * STAGE;     // 24 KiB per k-tile, 72 KiB ring
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lst = reinterpret_cast<float*>(smem + RING);          // lnfold_publish's layout: [TM] float2 (rstd, -mean rstd), [BN] wsum, [BN] bias  (MFMA column order)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1;
    const int nper = p.reserved2_;                               // persistent blocks (multiple of 8); the rest of the grid prefetches
    if (prefetch_block(p, nper, 256)) return;

    const int tiles_n = p.N / BN;
    // tiles of this block: XCD x = b & 7 owns a contiguous range of the raster, its J = nper / 8 blocks walk it with stride J
    int t_cur, t_end;
    const int J = nper >> 3;
    xcd_range(((p.M + TM - 1) / TM) * tiles_n, blockIdx.x & 7, t_cur, t_end);
    t_end += t_cur;
    t_cur += blockIdx.x >> 3;
    if (t_cur >= t_end) return;                                  // (block-uniform)
    const int nk = 2 * (p.K / 64);                               // K % 64 == 0 (host-checked)

    // ---- DMA addressing: piece = 16 rows x 64 B, lane -> row lane >> 2, physical chunk lane & 3 ----
    const int lrow = lane >> 2, pch = lane & 3;
    const int lch = pch ^ swz64(lrow);
    const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, OOB_OFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, OOB_OFF, 0x00020000);
    unsigned a_off[4], w_off[2];
    int w_perm[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) w_perm[g] = MMA::perm((g * 4 + wave) * 16 + lrow);
    auto set_dma_tile = [&](int t) {                             // t < 0: no tile (every lane out of range: zero fill, no traffic)
        const int tm = t / tiles_n, tn = t - tm * tiles_n;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = tm * TM + (g * 4 + wave) * 16 + lrow;
            a_off[g] = (t >= 0 && row < p.M) ? (unsigned)(((int64_t)row * p.lda + lch * 8) * 2) : OOB_OFF;
        }
#pragma unroll
        for (int g = 0; g < 2; ++g)
            w_off[g] = t >= 0 ? (unsigned)(((int64_t)(tn * BN + w_perm[g]) * p.ldw + lch * 8) * 2) : OOB_OFF;
    };
    auto dma_piece = [&](int kt, int slot, int j) {              // piece j (0..3: A, 4..5: W) of k-tile kt of the DMA tile
        const lds_ptr sa = (lds_ptr)smem + slot * STAGE;
        const unsigned soff = (unsigned)(kt * KS * 2);
        if (j < 4) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, sa + (j * 4 + wave) * 1024, 16, a_off[j], soff, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, sa + A_BYTES + ((j - 4) * 4 + wave) * 1024, 16, w_off[j - 4], soff, 0, 0);
    };

    // ---- fragments: operand row lane % ROWS of an MFMA tile, 16-byte chunk (4 / KF) ks + lane / ROWS of the k-tile's four ----
    const G4pLane l = {lane & (MMA::ROWS - 1), lane / MMA::ROWS, wave_m, wave_n, lst, lst + 2 * TM, lst + 2 * TM + BN};
    int fa_off[MT][KF], fb_off[NT][KF];
#pragma unroll
    for (int ks = 0; ks < KF; ++ks) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int row = wave_m * 128 + mt * MMA::ROWS + l.fr;
            fa_off[mt][ks] = row * RB + ((((4 / KF) * ks + l.fk) ^ swz64(row)) << 4);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int row = wave_n * 64 + nt * MMA::ROWS + l.fr;
            fb_off[nt][ks] = A_BYTES + row * RB + ((((4 / KF) * ks + l.fk) ^ swz64(row)) << 4);
        }
    }

    typename MMA::acc_t acc[MT][NT];
    half8v af[MT][KF], bf[NT][KF];
    int s0 = 0, s1 = 1, s2 = 2;                                  // ring slots of k-tiles i, i+1, i+2 of the running stream
    // one phase = one k-tile: fragments -> registers, its MFMAs; EVEN phases issue the pair (kt2, kt2 + 1) of the DMA tile: kt2 into the
    // slot of k-tile i - 1, kt2 + 1 into k-tile i's own slot (hence the barrier behind the fragment reads)
    auto phase = [&](auto even_tag, int kt2) {
        constexpr bool even = decltype(even_tag)::value;
        MMA::read(smem + s0 * STAGE, fa_off, fb_off, af, bf);
        if constexpr (even) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < KF * MT * NT; ++j) {
            const int ks = j / (MT * NT), mt = (j / NT) % MT, nt = j % NT;
            acc[mt][nt] = MMA::mfma(bf[nt][ks], af[mt][ks], acc[mt][nt]);
            if constexpr (even) {
                if (MMA::dma_after(j) >= 0) {
                    dma_piece(kt2, s2, MMA::dma_after(j));
                    dma_piece(kt2 + 1, s0, MMA::dma_after(j));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        { const int t = s0; s0 = s1; s1 = s2; s2 = t; }
    };

    // statistics of tile t: raw values -> registers (issued early), finished and published behind the tile's main loop
    const bool fold = (p.flags & MOCA_EP_LNFOLD) != 0;
    LnFoldRaw raw;
    auto stat_issue = [&](int t) {
        const int tm = t / tiles_n, tn = t - tm * tiles_n;
        raw = lnfold_issue<TM, BN>(p, tm * TM + tid, tn * BN + MMA::perm(tid), tid, fold);
    };

    // ---- prologue: first pair of the first tile ----
    stat_issue(t_cur);
    set_dma_tile(t_cur);
#pragma unroll
    for (int j = 0; j < 6; ++j) { dma_piece(0, 0, j); dma_piece(1, 1, j); }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const bool nt_out = out_streams(p);
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
#ifdef MOCA_STAMPS
    int tile_no = 0;
#endif
    while (true) {
        const int t_next = t_cur + J < t_end ? t_cur + J : -1;
        const int tm = t_cur / tiles_n, tn = t_cur - tm * tiles_n;
        const int m0 = tm * TM, n0 = tn * BN;
#ifdef MOCA_STAMPS
        const bool stamp_it = tile_no == 2;
        if (stamp_it) MOCA_STAMP(0);
        if (stamp_it) MOCA_STAMP(1);
        if (stamp_it) MOCA_STAMP(2);
#endif
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = typename MMA::acc_t(0.f);
        for (int i = 0; i < nk; i += 2) {
            const bool last = i + 2 >= nk;
            if (last) set_dma_tile(t_next);                      // the stream moves on to the next tile's first pair
            phase(yes_t{}, last ? 0 : i + 2);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            phase(no_t{}, 0);
            if (!last) {
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // pair (i+2, i+3) complete
                __builtin_amdgcn_s_barrier();
            }
        }
#ifdef MOCA_STAMPS
        if (stamp_it) MOCA_STAMP(3);
#endif
        lnfold_publish<TM, BN, false>(lnfold_finish<TM, BN>(p, raw, m0 + tid, tid, fold), lst, tid);
        if (t_next >= 0) stat_issue(t_next);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#ifdef MOCA_STAMPS
        if (stamp_it) MOCA_STAMP(4);
#endif
        MMA::template epilogue<GEGLU>(p, acc, l, m0, n0, rowadd, resid, nt_out);      // from registers
#ifdef MOCA_STAMPS
        if (stamp_it) { MOCA_STAMP(5); MOCA_STAMP_HW(); }
        ++tile_no;
#endif
        if (t_next < 0) break;
        t_cur = t_next;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");           // the next tile's first pair has landed (and the stores have left)
        __builtin_amdgcn_s_barrier();
    }
}
#endif

template <bool GEGLU>
__global__ __launch_bounds__(256, 2) void gemm_g4p_kernel(const moca_gemm_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
    g4p_body<GEGLU, G4pMma16>(p);
#endif
}
template <bool GEGLU>
__global__ __launch_bounds__(256, 2) void gemm_g4q_kernel(const moca_gemm_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
    g4p_body<GEGLU, G4pMma32>(p);
#endif
}

// =====================================================================================
// "sqp" kernel: the 256 x 256 staggered kernel (SHAPE 2 above: 8 waves as 4 x 2, wave tile 64 x 128, 5-slot ring of 32 KiB k-tiles, the
// two waves of a SIMD half an iteration apart) as a PERSISTENT kernel with a REGISTER epilogue, for the wide linears (GEGLU
// projections first).  Per 256 x 256 tile of the 320-channel GEGLU the round-4 kernel spent 31.5 k cycles: 5.0 k in the prologue, 14.0 k in
// the main loop, 9.5 k in the accumulator -> LDS staging pass with the erf-GELU, 2.5 k in the store loop
// (profiles/r05_g4_phase_stamps.txt).  Here
//   * one block per CU walks its tiles; the DMA stream is CONTINUOUS: the pair issued in an iteration's LOADo segment simply moves on to
//     the next tile's k-tiles when the current tile's are exhausted, so a tile's first two pairs are landing while the previous tile's
//     last iterations and epilogue run -- no prologue, no drain, no repeated pieces;
//   * W rows are fetched into the LDS tile in the permuted order of g4p_perm, so a lane's accumulators in two neighbouring MFMA tiles
//     are 8 consecutive output columns and the epilogue stores 16 bytes per lane straight from registers (16 rows x 64 B per
//     instruction): the ring is never used for staging, nothing waits for it to drain;
//   * tile statistics (LayerNorm fold: rstd, -mean rstd per row; wsum, bias per column) travel in four registers through the main
//     loop, as in the staggered kernel, and are published in the ONE ring slot that is free during an epilogue (the slot of the tile's
//     last k-tile: the stream refills it in the next tile's first LOADo, two barriers after the late half's epilogue has ended).
// =====================================================================================
// LDS accesses the compiler must not see: a read / write of ring memory that it cannot prove disjoint from an LDS-DMA in flight is
// given an `s_waitcnt vmcnt(0)` of its own (eight per epilogue here, each behind a global store).  Addresses are LDS byte offsets;
// lds_wait() = lgkmcnt(0) + the scheduling fence that keeps consumers below it (cdna_hip_programming.md rule 18).
__device__ __forceinline__ void lds_wr_f2(unsigned a, f32x2 v) { asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_wr_f1(unsigned a, float v) { asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ __forceinline__ f32x2 lds_rd_f2(unsigned a) { f32x2 v; asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(a) : "memory"); return v; }
__device__ __forceinline__ f32x4 lds_rd_f4(unsigned a) { f32x4 v; asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a) : "memory"); return v; }
__device__ __forceinline__ float lds_rd_f1(unsigned a) { float v; asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(a) : "memory"); return v; }
__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); }

__device__ __forceinline__ int sqp_perm(int rho) {              // LDS row of the 256-row W tile -> packed W row of the tile (64-column groups as g4p_perm)
    return (rho & ~63) + (g4p_perm(rho & 127) & 63);
}

template <bool GEGLU>
__global__ __launch_bounds__(512, 2) void gemm_sqp_kernel(const moca_gemm_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int MT = 4, NT = 8, KS = 32, RB = 64, WTM = 64, WTN = 128, TM = 256, BN = 256;
    constexpr int A_BYTES = TM * RB, STAGE = A_BYTES + BN * RB, NS = 5, PPW = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1;
    const bool late = wave >= 4;
    const int nper = p.reserved2_;                               // persistent blocks (multiple of 8); the rest of the grid prefetches
    if (prefetch_block(p, nper, 512)) return;

    // ---- this block's tiles: XCD x = b & 7 owns either a contiguous range of the tile_m-major raster or (xcd_n > 1) an xm x xn sub-grid,
    //      its J = nper / 8 blocks walk it with stride J ----
    const int tiles_n = p.N / BN, tiles_m = (p.M + TM - 1) / TM;
    const int xcd_n = p.reserved4_ >> 8;
    const int J = nper >> 3;
    int q_base, q_cnt, sub_n, tm_base, tn_base;
    {
        const int x = blockIdx.x & 7;
        if (xcd_n > 1) {
            const int xm = 8 / xcd_n, sm = tiles_m / xm;
            sub_n = tiles_n / xcd_n;
            const int xi = x / xcd_n, xj = x - xi * xcd_n;
            tm_base = xi * sm; tn_base = xj * sub_n;
            q_base = 0; q_cnt = sm * sub_n;
        } else {
            xcd_range(tiles_m * tiles_n, x, q_base, q_cnt);
            sub_n = tiles_n; tm_base = 0; tn_base = 0;
        }
    }
    auto tile_of = [&](int q, int& tm, int& tn) {                // q-th tile of this XCD's set
        const int l = q_base + q;
        const int a = l / sub_n;
        tm = tm_base + a; tn = tn_base + (l - a * sub_n);
    };
    // walk of the XCD's set (p.reserved4_ bit 1): STRIDED -- block j takes tiles j, j + J, ...: at any time the XCD's J blocks hold J
    // consecutive tiles of the raster (3.2 rows of 10 column tiles), every A row tile is shared by ~10 blocks that all request it at the
    // same moment, i.e. all of them wait out the same HBM miss; or CONTIGUOUS -- block j takes tiles [j cnt / J, (j + 1) cnt / J): it walks
    // a row's column tiles one after the other, so its A row tile misses to HBM once and is then re-read from L2 / the Infinity Cache,
    // while the J blocks of the XCD, in step, share ONE W panel at a time.
    int q_cur, q_step, q_end;
    {
        const int j = blockIdx.x >> 3;
        if (p.reserved4_ & 2) {
            q_cur = (int)((int64_t)q_cnt * j / J);
            q_end = (int)((int64_t)q_cnt * (j + 1) / J);
            q_step = 1;
        } else {
            q_cur = j; q_end = q_cnt; q_step = J;
        }
    }
    if (q_cur >= q_end) return;                                  // (block-uniform)
    const int nk = p.K / 32;                                     // K % 64 == 0 (host-checked): an even number of k-tiles

    // ---- DMA stream: piece = 16 rows x 64 B; A pieces w and 8 + w, W pieces w and 8 + w of every k-tile (4 per wave) ----
    const int lrow = lane >> 2, pch = lane & 3;
    const int lch = pch ^ swz64(lrow);
    const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, OOB_OFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, OOB_OFF, 0x00020000);
    unsigned a_off[2], w_off[2];
    int d_q = q_cur, d_k = 0;                                    // tile / even k-tile of the next pair the stream issues
    auto set_dma_tile = [&](int q) {                             // q >= q_end: no tile (every lane out of range: zero fill, no traffic)
        int tm, tn;
        tile_of(q, tm, tn);
        const bool any = q < q_end;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int row = tm * TM + (g * 8 + wave) * 16 + lrow;
            a_off[g] = (any && row < p.M) ? (unsigned)(((int64_t)row * p.lda + lch * 8) * 2) : OOB_OFF;
            w_off[g] = any ? (unsigned)(((int64_t)(tn * BN + sqp_perm((g * 8 + wave) * 16 + lrow)) * p.ldw + lch * 8) * 2) : OOB_OFF;
        }
    };
    auto issue_pair = [&](int slot_even, int slot_odd) {
        const unsigned soff = (unsigned)(d_k * KS * 2);
        const lds_ptr se = (lds_ptr)smem + slot_even * STAGE, so = (lds_ptr)smem + slot_odd * STAGE;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, se + (g * 8 + wave) * 1024, 16, a_off[g], soff, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, so + (g * 8 + wave) * 1024, 16, a_off[g], soff + KS * 2, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, se + A_BYTES + (g * 8 + wave) * 1024, 16, w_off[g], soff, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, so + A_BYTES + (g * 8 + wave) * 1024, 16, w_off[g], soff + KS * 2, 0, 0);
        }
        d_k += 2;
        if (d_k >= nk) { d_k = 0; d_q += q_step; set_dma_tile(d_q); }
    };

    const int fr = lane & 15, fg = lane >> 4;
    const int swz = (fg ^ swz64(fr)) << 4;
    const int a_off0 = (wave_m * WTM + fr) * RB + swz;
    const int b_off0 = A_BYTES + (wave_n * WTN + fr) * RB + swz;
    f32x4 acc[MT][NT];
    half8v af[2][MT], bf[2][NT];
    auto read_tile = [&](auto set_tag, int slot) {
        constexpr int S = decltype(set_tag)::value;
        const char* cur = smem + slot * STAGE;
#pragma unroll
        for (int r = 0; r < NT; ++r) bf[S][r] = *reinterpret_cast<const half8v*>(cur + b_off0 + r * 1024);
#pragma unroll
        for (int r = 0; r < MT; ++r) af[S][r] = *reinterpret_cast<const half8v*>(cur + a_off0 + r * 1024);
    };

    // (asm volatile: recomputed where it is used -- as a loop invariant it is hoisted, kept across the main loop and spilled)
    auto tid_now = [&]() -> int {
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return wave * 64 + l;
    };
    // ---- tile statistics: thread t < 256 (the early half) owns row t and LDS column t of the tile.  The values of tile q + 1 are
    //      fetched at the head of tile q's epilogue and finished behind its stores; they travel through the main loop as four registers
    //      (rstd, -mean rstd, wsum, bias).  The fetch is LDS-DMA (4 bytes per lane, into 22 KiB of the free slot behind the published
    //      statistics, one private area per wavefront), read back with inline-asm ds_reads behind a counted wait -- no VGPR is the
    //      destination of a load: a VGPR load the compiler knows about makes it guard every later write of those registers (the fragment
    //      reads of the main loop) with `s_waitcnt vmcnt(0)`, draining the DMA stream once per iteration; an inline-asm VGPR load is
    //      copied by the register allocator BEFORE the asm wait that retires it (`v_mov` of the load destinations in front of the
    //      `s_waitcnt` statement that names them "+v": seen in the ISA of the first form of this path -- stale statistics whenever a load
    //      is slower than the epilogue's arithmetic). ----
    const bool fold = (p.flags & MOCA_EP_LNFOLD) != 0;
    const float* const dummy = reinterpret_cast<const float*>(p.w);
    constexpr unsigned STAT_SCRATCH = 8192;                      // offset of the raw-value areas inside the free slot
    auto stat_dma = [&](int q, unsigned slot_off) {              // waves 0..3 only
        int tm, tn;
        tile_of(q < q_end ? q : 0, tm, tn);
        const int t = tid_now();
        const int n = tn * BN + sqp_perm(t);
        const int m = min(tm * TM + t, p.M - 1);
        const lds_ptr area = (lds_ptr)smem + slot_off + STAT_SCRATCH + wave * (22 * 256);
        __builtin_amdgcn_global_load_lds((glb_ptr)(fold ? p.lnf_wsum + n : dummy), area, 4, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_ptr)(p.bias ? p.bias + n : dummy), area + 256, 4, 0, 0);
        if (fold) {
            for (int i = 0; i < p.lnf_nparts; ++i) {             // (block-uniform; <= 10)
                const float* src = p.lnf_part + ((int64_t)i * p.M + m) * 2;
                __builtin_amdgcn_global_load_lds((glb_ptr)src, area + (2 + 2 * i) * 256, 4, 0, 0);
                __builtin_amdgcn_global_load_lds((glb_ptr)(src + 1), area + (3 + 2 * i) * 256, 4, 0, 0);
            }
        }
    };
    // (`after` = vector-memory instructions this wave has issued behind the DMAs, at least: the wait leaves that many outstanding)
    auto stat_read = [&](unsigned slot_off, auto after_tag) -> LnFoldRegs {
        constexpr int after = decltype(after_tag)::value;
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(after) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        int lane_;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_));
        const unsigned area = (unsigned)(size_t)((lds_ptr)smem + slot_off + STAT_SCRATCH + wave * (22 * 256)) + 4 * lane_;
        const float ws = lds_rd_f1(area), b = lds_rd_f1(area + 256);
        float s = 0.f, qq = 0.f;
        LnFoldRegs f = {1.f, 0.f, 0.f, 0.f};
        if (fold) {
            for (int i = 0; i < p.lnf_nparts; ++i) {
                const float x = lds_rd_f1(area + (2 + 2 * i) * 256), y = lds_rd_f1(area + (3 + 2 * i) * 256);
                lds_wait();
                s += x; qq += y;
            }
        }
        lds_wait();
        f.ws = fold ? ws : 0.f;
        f.b = p.bias ? b : 0.f;
        if (fold) {
            const float2 st = lnfold_stats(s, qq, p.K, p.ln_eps);
            f.rs = st.x;
            f.rb = st.y;
        }
        return f;
    };

    // ---- prologue (once per block): two pairs in flight, the first landed everywhere ----
    LnFoldRegs lf = {1.f, 0.f, 0.f, 0.f};
    if (!late) {                                                 // (slot 4 is not part of the prologue's four k-tiles)
        stat_dma(q_cur, (NS - 1) * STAGE);
        lf = stat_read((NS - 1) * STAGE, int_c<0>{});
    }
    __builtin_amdgcn_s_barrier();                                // (every read of slot 4 done before the stream reaches it)
    set_dma_tile(q_cur);
    issue_pair(0, 1);
    issue_pair(2, 3);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPW) : "memory");
    __builtin_amdgcn_s_barrier();
    if (late) __builtin_amdgcn_s_barrier();                      // from here on waves 4..7 run one barrier behind waves 0..3

    const bool nt_out = out_streams(p);
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
    int s0 = 0;                                                  // ring slot of the running stream's current k-tile
#ifdef MOCA_STAMPS
    int tile_no = 0;
#endif
    while (true) {
        int tm, tn;
        tile_of(q_cur, tm, tn);
        const int m0 = tm * TM, n0 = tn * BN;
#ifdef MOCA_STAMPS
        const bool stamp_it = tile_no == 3;          // (phases: [0, 0, main loop, publish + barrier, epilogue arithmetic + stores] + the statistics wait)
        if (stamp_it) { MOCA_STAMP(0); }
#endif
        // (plain zeros, default unrolling: the compiler peels the first iteration -- literal C operand -- and reconciles the peeled copy's
        //  result registers with ~100 v_mov per steady-state iteration; opaque zeros and / or `unroll(disable)` remove the moves and
        //  measure 1-8 % SLOWER on every GEGLU shape, same box, profiles/r05_ab_sqp_loop_shape.txt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < nk; i += 2) {
            const int s1 = s0 + 1 == NS ? 0 : s0 + 1;
            const int sp = s0 == 0 ? NS - 1 : s0 - 1;
            // ---- LOADe: k-tile i ----
#ifdef MOCA_STAMPS
            const bool seg = stamp_it && i == SEG_ITER;
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
            // ---- MFMAe with the reads of k-tile i + 1 in the gaps ----
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
            // ---- LOADo: the stream's next pair into the slots of k-tiles i - 1 and i; the pair before it has landed ----
            issue_pair(sp, s0);
#ifdef MOCA_STAMPS
            if (seg) MOCA_STAMP_W(13, SEG_WAVE);
#endif
            // (behind an epilogue this also waits for the epilogue's stores, which are older than the pair just issued: leaving them
            //  outstanding -- vmcnt(8 + stores) in a tile's first LOADo -- measured no different, profiles/r05_ab_sqp_store_wait.txt)
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
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[1][nt], af[1][mt], acc[mt][nt], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
#ifdef MOCA_STAMPS
            if (seg) MOCA_STAMP_W(1, SEG_WAVE);
#endif
            __builtin_amdgcn_s_barrier();
#ifdef MOCA_STAMPS
            if (seg) MOCA_STAMP_W(2, SEG_WAVE);
#endif
            s0 = s1 + 1 == NS ? 0 : s1 + 1;
        }
#ifdef MOCA_STAMPS
        if (stamp_it) MOCA_STAMP(3);
#endif
        // ---- epilogue: statistics -> the free slot (that of the tile's last k-tile), then registers -> memory.  The halves MEET first
        //      (waves 0..3 wait for waves 4..7's last MFMAo) and part again behind it: one barrier apart, with no barrier inside, the
        //      two epilogues would run one after the other -- each half's 6 k cycles of arithmetic inside the other's barrier wait ----
        if (!late) __builtin_amdgcn_s_barrier();
        const unsigned lst = (unsigned)(size_t)((lds_ptr)smem + (s0 == 0 ? NS - 1 : s0 - 1) * STAGE);   // [TM] float2, [BN] wsum, [BN] bias
        const unsigned lws = lst + 8 * TM, lbi = lws + 4 * BN;
        if (!late) {
            const int t = tid_now();                              // (recomputed: a thread id kept across the main loop is the one value it spills)
            lds_wr_f2(lst + 8 * t, f32x2{lf.rs, lf.rb});
            lds_wr_f1(lws + 4 * t, lf.ws);
            lds_wr_f1(lbi + 4 * t, lf.b);
        }
        lds_wait();
        __builtin_amdgcn_s_barrier();
#ifdef MOCA_STAMPS
        if (stamp_it) MOCA_STAMP(4);
#endif
        f32x2 st[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) st[mt] = lds_rd_f2(lst + 8 * (wave_m * WTM + mt * 16 + fr));
        const int q_next = q_cur + q_step;
        const unsigned stat_slot = (unsigned)((s0 == 0 ? NS - 1 : s0 - 1) * STAGE);
        if (!late) stat_dma(q_next, stat_slot);                   // (in flight under the epilogue's arithmetic; read back behind its stores)
#pragma unroll
        for (int grp = 0; grp < 2; ++grp) {
            f32x4 cw[4], cb[4];                                   // (per 64-column group: 32 registers instead of 64)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                cw[t] = lds_rd_f4(lws + 4 * (wave_n * WTN + (grp * 4 + t) * 16 + 4 * fg));
                cb[t] = lds_rd_f4(lbi + 4 * (wave_n * WTN + (grp * 4 + t) * 16 + 4 * fg));
            }
            lds_wait();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int m = m0 + wave_m * WTM + mt * 16 + fr;
                f32x4 v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = st[mt][0] * acc[mt][grp * 4 + t] + (st[mt][1] * cw[t] + cb[t]);
                if constexpr (GEGLU) {
                    half8v h;
#pragma unroll
                    for (int nv = 0; nv < 2; ++nv) {
                        const f32x4 r4 = moca_geglu4(v[nv], v[nv + 2]);        // (4-wide: 7 instead of 133 s_nop per epilogue, -1 % at K = 320)
                        h[4 * nv + 0] = (half_t)r4[0]; h[4 * nv + 1] = (half_t)r4[1]; h[4 * nv + 2] = (half_t)r4[2]; h[4 * nv + 3] = (half_t)r4[3];
                    }
                    if (m < p.M) st_out8(reinterpret_cast<half_t*>(p.out) + (int64_t)m * p.ldo + (n0 >> 1) + wave_n * 64 + grp * 32 + 8 * fg, h, nt_out);
                } else {
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const int col = n0 + wave_n * WTN + grp * 64 + hh * 32 + 8 * fg;
                        float o[8];
#pragma unroll
                        for (int r = 0; r < 4; ++r) { o[r] = v[2 * hh][r]; o[4 + r] = v[2 * hh + 1][r]; }
                        store8_rowadd_res(p, m, col, o, rowadd, resid, nt_out);
                    }
                }
            }
        }
        // the next tile's statistics: complete once at most the stores issued behind their loads are outstanding (GEGLU: 8 per lane, plain
        // 16; a tile with rows past M may have skipped stores: full drain there)
#ifdef MOCA_STAMPS
        if (stamp_it) { MOCA_STAMP(5); MOCA_STAMP_HW(); }
        ++tile_no;
#endif
        if (!late) {
            if (m0 + TM > p.M) lf = stat_read(stat_slot, int_c<0>{});
            else lf = stat_read(stat_slot, int_c<(GEGLU ? 8 : 16)>{});
        }
        if (q_next >= q_end) break;
        q_cur = q_next;
        if (late) __builtin_amdgcn_s_barrier();                  // waves 4..7 fall one barrier behind again
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // (the stream's last pairs were zero fill; the halves are together here)
#endif
}

template <bool GEGLU>
int launch_gemm_g4p(const moca_gemm_params& p, hipStream_t st) {
    constexpr int lds = 3 * (256 + 128) * 64 + (2 * 256 + 2 * 128) * 4;      // 72 KiB ring + 3 KiB of tile statistics
    if (!dyn_lds_once<&gemm_g4p_kernel<GEGLU>>(lds)) return MOCA_E_LAUNCH;
    moca_gemm_params pl = p;
    pl.reserved2_ = G4P_BLOCKS;
    if (moca_tuning_get(MOCA_TUNE_GEMM_MF32)) {
        if (!dyn_lds_once<&gemm_g4q_kernel<GEGLU>>(lds)) return MOCA_E_LAUNCH;
        hipLaunchKernelGGL((gemm_g4q_kernel<GEGLU>), dim3(G4P_BLOCKS + 2 * prefetch_blocks(pl)), dim3(256), lds, st, pl);
    } else {
        hipLaunchKernelGGL((gemm_g4p_kernel<GEGLU>), dim3(G4P_BLOCKS + 2 * prefetch_blocks(pl)), dim3(256), lds, st, pl);
    }
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

template <bool GEGLU>
int launch_gemm_sqp(const moca_gemm_params& p, hipStream_t st) {
    constexpr int lds = 5 * (256 + 256) * 64;                    // the whole 160 KiB: the ring; tile statistics live in its one free slot
    if (!dyn_lds_once<&gemm_sqp_kernel<GEGLU>>(lds)) return MOCA_E_LAUNCH;
    moca_gemm_params pl = p;
    pl.reserved2_ = SQP_BLOCKS;
    pl.reserved4_ = (pl.reserved4_ & 0xfd) | (choose_xcd_n(p, (p.M + 255) / 256, p.N / 256, 256) << 8) |
                    (moca_tuning_get(MOCA_TUNE_SQP_WALK) ? 2 : 0);
    hipLaunchKernelGGL((gemm_sqp_kernel<GEGLU>), dim3(SQP_BLOCKS + prefetch_blocks(pl)), dim3(512), lds, st, pl);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

}  // namespace

int moca_gemm_g4p_launch(const moca_gemm_params& p, hipStream_t st) {
    return (p.flags & MOCA_EP_GEGLU) ? launch_gemm_g4p<true>(p, st) : launch_gemm_g4p<false>(p, st);
}
int moca_gemm_sqp_launch(const moca_gemm_params& p, hipStream_t st) {
    return (p.flags & MOCA_EP_GEGLU) ? launch_gemm_sqp<true>(p, st) : launch_gemm_sqp<false>(p, st);
}
