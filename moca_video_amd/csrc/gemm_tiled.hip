// The GEMM kernels that compute one tile per block and send it through the store loops of the staged fp16 tile (gemm_device.h):
//   gemm_glds_kernel<BN, AMODE, FAST>  256 x BN (128 or 160), 8 waves, direct-to-LDS 3-slot ring; column / row statistics,
//                                      LayerNorm fold, fp32 output, split-K slabs (fp32 or fp16)
//   gemm_g4_kernel<AMODE, FAST>        256 x 128, 4 waves, two blocks per CU: one block's epilogue under the other's MFMAs
//   gemm_w80s_kernel<AMODE, SHAPE>     (gemm_w80s_kernel.inc, compiled twice below) the staggered, buffer-addressed 8-wave kernel
// Which calls they run: route_of() in gemm.hip.
// Why one translation unit: the code hipcc generates for a shared store loop follows what ALL its callers in the unit pass.  The
// 256 x 160 kernel and the 320 x 160 staggered kernel share store_fp16_tile_rowsum<512, 160, 4>, one with 256 rows and one with 320:
// apart, each unit's copy is specialised for its row count and the ten kernels that call it change (5 to 7 instructions each).
// glds and g4 share AGather and its one zero page.
#include "gemm_launch.h"

namespace {

// zeros: long enough that `zero + per-tile k offset` of the fast gather path stays inside it
constexpr int ZERO_PAGE_HALVES = 8192 + 64;
__device__ __attribute__((aligned(16))) half_t g_zero_page[ZERO_PAGE_HALVES];

// ---- A-operand gather addressing shared by the direct-to-LDS kernels (glds, g4, w80) -----------------------------------
// A lane owns NAP rows of the block tile (one per DMA instruction it issues) and a 16-byte chunk `lch` of the KS-wide k-tile.
// Fast path (every layer of the UNet except the 4-channel input conv): a k-tile lies inside ONE tap (C % 64 == 0) resp. inside
// K (K % 64 == 0), so per tile every lane just adds a block-uniform element offset to a per-row base pointer.  Rows that must
// read zeros (conv halo, t-1/t+1 outside the clip, M tail) have the zero page as base; the zero page is longer than any
// per-tile offset, so no per-tile select is needed.  Bases are recomputed only when the tap changes (every C/KS tiles).
// Slow path (input conv with C = 8, odd K): the source of every (row, tile) is computed from scratch.
template <int AMODE, bool FAST, int NAP, int KS>
struct AGather {
    const moca_gemm_params& p;
    const half_t* Aptr;
    const half_t* zero;
    int lch;
    int64_t row_off[NAP];
    int row_y[NAP], row_x[NAP];
    bool row_ok[NAP];
    const half_t* a_base[NAP];
    int tap_cur = -1, a_koff = 0, tiles_per_tap;

    __device__ __forceinline__ AGather(const moca_gemm_params& p_, int lch_)
        : p(p_), Aptr(reinterpret_cast<const half_t*>(p_.a)), zero(g_zero_page), lch(lch_),
          tiles_per_tap((AMODE == MOCA_A_LINEAR || !FAST) ? (1 << 30) : p_.C / KS) {}

    // row slot g of this lane is output row m (pixel m of the [frame][y][x] raster for the conv modes)
    __device__ __forceinline__ void init_row(int g, int m) {
        row_ok[g] = m < p.M;
        const int mm = row_ok[g] ? m : 0;
        if (AMODE == MOCA_A_LINEAR) {
            row_off[g] = (int64_t)mm * p.lda;
            row_y[g] = row_x[g] = 0;
        } else if (AMODE == MOCA_A_CONV3X3) {
            const int ohw = p.outH * p.outW;
            int f, rem, oy, ox;
            if (p.M < (1 << 24)) {
                divmod24(mm, ohw, 1.0f / (float)ohw, f, rem);
                divmod24(rem, p.outW, 1.0f / (float)p.outW, oy, ox);
            } else {
                f = mm / ohw; rem = mm - f * ohw;
                oy = rem / p.outW; ox = rem - oy * p.outW;
            }
            row_off[g] = (int64_t)f * p.inH * p.inW;
            row_y[g] = oy * p.stride - 1 + p.nopad_lo + (p.up_phase ? (p.up_phase - 1) >> 1 : 0);
            row_x[g] = ox * p.stride - 1 + p.nopad_lo + (p.up_phase ? (p.up_phase - 1) & 1 : 0);
        } else {
            int frame, pix, vid, t;
            if (p.M < (1 << 24)) {
                divmod24(mm, p.HW, 1.0f / (float)p.HW, frame, pix);
                divmod24(frame, p.T, 1.0f / (float)p.T, vid, t);
            } else {
                frame = mm / p.HW; t = frame % p.T;
            }
            row_off[g] = mm;
            row_y[g] = t;
            row_x[g] = 0;
        }
    }

    __device__ __forceinline__ void set_tap(int tap) {
        tap_cur = tap;
        if (AMODE == MOCA_A_LINEAR) {
#pragma unroll
            for (int g = 0; g < NAP; ++g) a_base[g] = row_ok[g] ? Aptr + row_off[g] + lch * 8 : zero;
        } else if (AMODE == MOCA_A_CONV3X3) {
            // (up_phase: one of the four 2 x 2 convs a nearest-x2 upsample + 3 x 3 conv splits into -- tap t = (t >> 1, t & 1))
            const int ky = p.up_phase ? tap >> 1 : tap / 3, kx = p.up_phase ? tap & 1 : tap - ky * 3;
            const int limH = p.up ? 2 * p.inH : p.inH, limW = p.up ? 2 * p.inW : p.inW;
#pragma unroll
            for (int g = 0; g < NAP; ++g) {
                int iy = row_y[g] + ky, ix = row_x[g] + kx;
                const bool ok = tap < (p.up_phase ? 4 : 9) && row_ok[g] && iy >= 0 && iy < limH && ix >= 0 && ix < limW;
                if (p.up) { iy >>= 1; ix >>= 1; }
                const half_t* src = Aptr + (row_off[g] + (int64_t)iy * p.inW + ix) * p.C + lch * 8;
                a_base[g] = ok ? src : zero;
            }
        } else {
#pragma unroll
            for (int g = 0; g < NAP; ++g) {
                const int tt = row_y[g] + tap - 1;
                const bool ok = tap < 3 && row_ok[g] && tt >= 0 && tt < p.T;
                const half_t* src = Aptr + (row_off[g] + (int64_t)(tap - 1) * p.HW) * p.C + lch * 8;
                a_base[g] = ok ? src : zero;
            }
        }
    }

    // block-uniform per-tile state of the DMA stream (fast path): element offset added to every a_base
    __device__ __forceinline__ void begin_tile(int kt) {
        if constexpr (FAST) {
            const int tap = kt / tiles_per_tap;
            if (tap != tap_cur) set_tap(tap);
            a_koff = (kt - tap * tiles_per_tap) * KS;
        }
    }

    __device__ __forceinline__ const half_t* slow_src(int kt, int g) const {
        const int k = kt * KS + lch * 8;
        if (AMODE == MOCA_A_LINEAR) {
            return (k < p.K && row_ok[g]) ? Aptr + row_off[g] + k : zero;
        } else if (AMODE == MOCA_A_CONV3X3) {
            const int tap = k / p.C, c = k - tap * p.C;
            const int ky = tap / 3, kx = tap - ky * 3;
            const int limH = p.up ? 2 * p.inH : p.inH, limW = p.up ? 2 * p.inW : p.inW;
            int iy = row_y[g] + ky, ix = row_x[g] + kx;
            const bool ok = tap < 9 && row_ok[g] && iy >= 0 && iy < limH && ix >= 0 && ix < limW;
            if (p.up) { iy >>= 1; ix >>= 1; }
            return ok ? Aptr + (row_off[g] + (int64_t)iy * p.inW + ix) * p.C + c : zero;
        } else {
            const int tap = k / p.C, c = k - tap * p.C;
            const int tt = row_y[g] + tap - 1;
            const bool ok = tap < 3 && row_ok[g] && tt >= 0 && tt < p.T;
            return ok ? Aptr + (row_off[g] + (int64_t)(tap - 1) * p.HW) * p.C + c : zero;
        }
    }

    // source of row slot g for k-tile kt; `odd` = kt is the second tile of the pair begin_tile() was called for
    __device__ __forceinline__ const half_t* src(int kt, int g, int odd = 0) const {
        if constexpr (FAST) return a_base[g] + a_koff + odd * KS;
        else return slow_src(kt, g);
    }
};

// =====================================================================================
// Large-tile kernel: 256 x BN x 64 block tile (BN = 128 or 160), 512 threads = 8
// wavefronts (4 x 2), wave tile 64 x BN/2 as 4 x (BN/32) v_mfma_f32_16x16x32_f16
// accumulators.  Operands are staged global -> LDS directly (global_load_lds_dwordx4,
// no VGPR round trip) into a 3-slot ring, two k-tiles in flight, ONE raw s_barrier per
// k-tile behind a counted s_waitcnt vmcnt(N) (never 0 in the steady state).  The LDS
// image of a DMA is lane-linear, so the bank-conflict XOR swizzle is applied on the
// per-lane SOURCE address (logical chunk = physical chunk ^ ((row>>1)&7)) and again on
// the fragment reads.  Zero padding (conv halo, M/K tails) is a lane whose source is a
// 16-byte zero page.
// =====================================================================================
template <int BN, int AMODE, bool FAST>
__global__ __launch_bounds__(512, 2) void gemm_glds_kernel(const moca_gemm_params p) {
    constexpr int TM = 256;
    constexpr int NT = BN / 32;                       // 16-wide n tiles per wave
    constexpr int A_BYTES = TM * ROW_BYTES;           // 32 KiB
    constexpr int B_BYTES = BN * ROW_BYTES;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int B_GROUPS = BN / 8;                  // 1 KiB row groups of the W tile (16 or 20)

    extern __shared__ __attribute__((aligned(16))) char smem[];
    MOCA_STAMP(0);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1;

    const int tiles_m = (p.M + TM - 1) / TM;
    const int tiles_n = p.N / BN;
    const int nk_total = (p.K + BK - 1) / BK;      // (W rows are readable and zero beyond K up to the next multiple of 64)
    int split, tile, kt_begin, kt_end;
    {
        const int nblk = tiles_m * tiles_n * p.splits;
        if (prefetch_block(p, nblk, 512)) return;
        int logical;
        remap_block<BN>(nblk, logical);
        split = logical % p.splits;
        tile = logical / p.splits;
        const int kts = (nk_total + p.splits - 1) / p.splits;
        kt_begin = split * kts;
        kt_end = min(kt_begin + kts, nk_total);
    }
    const int tile_m = tile / tiles_n, tile_n = tile % tiles_n;
    const int m0 = tile_m * TM, n0 = tile_n * BN;
    const int nk = kt_end - kt_begin;
    MOCA_STAMP_P(8, m0 + n0 + nk);

    const half_t* __restrict__ Wptr = reinterpret_cast<const half_t*>(p.w);

    // ---- DMA coordinates: instruction g of this wave fills row group q = g*8 + wave,
    //      i.e. rows q*8 + (lane>>3), physical chunk lane&7
    const int lrow = lane >> 3, pch = lane & 7;
    const int swz = (((wave * 8 + lrow) >> 1) & 7);   // same for every g (64 g rows apart)
    const int lch = pch ^ swz;                        // logical 16-byte chunk of the k-tile this lane fetches

    AGather<AMODE, FAST, 4, BK> ga(p, lch);
#pragma unroll
    for (int g = 0; g < 4; ++g) ga.init_row(g, m0 + (g * 8 + wave) * 8 + lrow);
    MOCA_STAMP_P(9, (int)ga.row_ok[0]);
    // W rows of this lane: group q = g*8 + wave (valid while q < B_GROUPS)
    const half_t* w_row[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int q = g * 8 + wave;
        const int n = n0 + (q < B_GROUPS ? q : 0) * 8 + lrow;
        w_row[g] = Wptr + (int64_t)n * p.ldw + lch * 8;
    }

    // DMA piece j (0..3: A row groups, 4..6: W row groups) of tile kt into ring slot `slot`
    auto dma_piece = [&](int kt, int slot, int j) {
        const lds_ptr sa = (lds_ptr)smem + slot * STAGE;
        if (j < 4) {
            const half_t* src;
            src = ga.src(kt, j);
            __builtin_amdgcn_global_load_lds((glb_ptr)src, sa + (j * 8 + wave) * 1024, 16, 0, 0);
        } else {
            const int g = j - 4;
            if (g * 8 + 7 < B_GROUPS || (g * 8 < B_GROUPS && wave < B_GROUPS - g * 8))
                __builtin_amdgcn_global_load_lds((glb_ptr)(w_row[g] + kt * BK), sa + A_BYTES + (g * 8 + wave) * 1024, 16, 0, 0);
        }
    };
    auto issue = [&](int kt, int slot) {
        ga.begin_tile(kt);
#pragma unroll
        for (int j = 0; j < 7; ++j) dma_piece(kt, slot, j);
    };

    f32x4 acc[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fg = lane >> 4;
    int a_row_b[4], a_swz[4], b_row_b[NT], b_swz[NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int row = wave_m * 64 + mt * 16 + fr;
        a_row_b[mt] = row * ROW_BYTES;
        a_swz[mt] = (row >> 1) & 7;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int row = wave_n * (BN / 2) + nt * 16 + fr;
        b_row_b[nt] = A_BYTES + row * ROW_BYTES;
        b_swz[nt] = (row >> 1) & 7;
    }

    // number of DMA instructions this wave issues per k-tile (for the counted wait)
    const bool extra_w = (B_GROUPS % 8) != 0 && wave < (B_GROUPS % 8);

    // ---- software-pipelined, hand-interleaved main loop ---------------------------------------
    // Two fragment register sets.  Per k-tile i each wave runs
    //   P0: MFMAs on set0 (k 0..31 of tile i), with the ds_reads of k 32..63 (-> set1) and the 6-7 DMA
    //       instructions of tile i+2 dropped one at a time into the gaps between MFMA pairs
    //   sync: counted vmcnt (tile i+1 landed), lgkmcnt(0), ONE s_barrier
    //   P1: MFMAs on set1, with the ds_reads of k 0..31 of tile i+1 (-> set0) in the gaps
    // sched_barrier(0) pins the interleave the source spells out.
    half8v af0[4], bf0[NT], af1[4], bf1[NT];
    auto read_one = [&](const char* st, int ks, int r, half8v (&af)[4], half8v (&bf)[NT]) {
        const int ch = ks * 4 + fg;
        if (r < 4) af[r] = *reinterpret_cast<const half8v*>(st + a_row_b[r] + ((ch ^ a_swz[r]) << 4));
        else bf[r - 4] = *reinterpret_cast<const half8v*>(st + b_row_b[r - 4] + ((ch ^ b_swz[r - 4]) << 4));
    };
    auto wait_tile = [&](bool more_in_flight) {
        // this wave's DMAs of the awaited tile are complete once at most one tile's worth is outstanding
        if (more_in_flight) {
            if (B_GROUPS % 8 == 0) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
            else if (extra_w) asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
    };
    constexpr int NMMA = 4 * NT;     // MFMAs per half k-tile
    constexpr int NRD = 4 + NT;      // fragment reads per half k-tile

    LnFoldRaw lraw = {float2{0.f, 0.f}, float2{0.f, 0.f}, 0.f, 0.f};
    if (p.flags & MOCA_EP_LNFOLD) lraw = lnfold_issue<TM, BN>(p, m0 + tid, n0 + tid, tid);
    MOCA_STAMP_P(10, a_row_b[0] + b_row_b[0]);
    if (nk > 0) issue(kt_begin, 0);
    MOCA_STAMP_P(11, 0);
    if (nk > 1) issue(kt_begin + 1, 1);
    LnFoldRegs lf = {0.f, 0.f, 0.f, 0.f};
    if (p.flags & MOCA_EP_LNFOLD) lf = lnfold_finish<TM, BN>(p, lraw, m0 + tid, tid);
    MOCA_STAMP(1);
    if (nk > 0) {
        wait_tile(nk > 1);
        MOCA_STAMP(2);
#pragma unroll
        for (int r = 0; r < NRD; ++r) read_one(smem, 0, r, af0, bf0);
    }
    int s_cur = 0, s_nxt = 1, s_far = 2;      // ring slots of tiles i, i+1, i+2 (rotated, no modulo in the loop)
    // one k-tile step; ISSUE (compile time) = tile i+2 exists and its DMA pieces go into the gaps of P0
    auto step = [&](auto issue_tag, int i, bool has_next) {
        constexpr bool do_issue = decltype(issue_tag)::value;
        const char* cur = smem + s_cur * STAGE;
        const int kt2 = kt_begin + i + 2, slot2 = s_far;     // ring slot (i-1)%3: every wave passed sync(i-1) after its last read of it
        if constexpr (do_issue) ga.begin_tile(kt2);
        // ---- P0 ----
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < NMMA; ++j) {
            const int mt = j / NT, nt = j % NT;
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf0[nt], af0[mt], acc[mt][nt], 0, 0, 0);
            if (j & 1) {
                const int r = j >> 1;
                if (r < NRD) read_one(cur, 1, r, af1, bf1);
                if constexpr (do_issue) { if (r >= 1 && r <= 7) dma_piece(kt2, slot2, r - 1); }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        // ---- sync ----
        if (has_next) wait_tile(do_issue);
        const char* nxt = smem + (has_next ? s_nxt : s_cur) * STAGE;
        // ---- P1 ----
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < NMMA; ++j) {
            const int mt = j / NT, nt = j % NT;
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf1[nt], af1[mt], acc[mt][nt], 0, 0, 0);
            if (j & 1) {
                const int r = j >> 1;
                if (r < NRD) read_one(nxt, 0, r, af0, bf0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        { const int t = s_cur; s_cur = s_nxt; s_nxt = s_far; s_far = t; }
    };
    int i = 0;
    for (; i + 2 < nk; ++i) step(yes_t{}, i, true);        // steady state: branch-free DMA issue
    for (; i < nk; ++i) step(no_t{}, i, i + 1 < nk);       // last two tiles: nothing left to prefetch
    MOCA_STAMP(3);
    __syncthreads();   // all fragment reads done before the ring is reused by the epilogue

    // The MFMAs above compute the TRANSPOSED tile (W fragment as A operand), so accumulator element r
    // of tile (mt, nt) is row m = wave_m*64 + mt*16 + fr, column n = wave_n*BN/2 + nt*16 + 4*fg + r:
    // each lane owns 4 CONSECUTIVE output columns of one row -> 8-byte fp16 / 16-byte fp32 accesses.
    if (p.splits > 1) {
        if (p.reserved4_ & 4) {
            // fp16 slabs (MOCA_TUNE_SLAB_F16, A/B only): the partial tile is rounded to fp16, staged like the fp16 epilogue and leaves as whole rows
            constexpr int pitch16 = BN * 2 + 16;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = wave_n * (BN / 2) + nt * 16 + 4 * fg;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const int row = wave_m * 64 + mt * 16 + fr;
                    *reinterpret_cast<half4v*>(smem + row * pitch16 + col * 2) = __builtin_convertvector(acc[mt][nt], half4v);
                }
            }
            __syncthreads();
            half_t* ws16 = reinterpret_cast<half_t*>(p.splitk_ws) + (int64_t)split * p.M * p.N;
            constexpr int cpr = BN / 8;
            for (int idx = tid; idx < TM * cpr; idx += 512) {
                const int row = idx / cpr, ch = idx - row * cpr;
                const int m = m0 + row;
                if (m < p.M) *reinterpret_cast<half8v*>(ws16 + (int64_t)m * p.N + n0 + ch * 8) = *reinterpret_cast<const half8v*>(smem + row * pitch16 + ch * 16);
            }
            return;
        }
        float* ws = p.splitk_ws + (int64_t)split * p.M * p.N;
        // the fp32 partial tile is staged in LDS and leaves as whole 4 BN-byte rows (round 5: straight from registers it left as 64-byte
        // segments, 16 rows x 4 lanes per instruction -- 1.2-1.4 us slower per launch at the 5 x 8-latent level, profiles/r05_ab_slab_store.txt)
        float* sC = reinterpret_cast<float*>(smem);
        constexpr int PF = BN == 128 ? BN + 4 : BN;           // floats per staged row (+16 B where the 160 KiB allow it: BN = 160 fills them)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = wave_n * (BN / 2) + nt * 16 + 4 * fg;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int row = wave_m * 64 + mt * 16 + fr;
                *reinterpret_cast<f32x4*>(sC + row * PF + col) = acc[mt][nt];
            }
        }
        __syncthreads();
        constexpr int cpr4 = BN / 4;
        for (int idx = tid; idx < TM * cpr4; idx += 512) {
            const int row = idx / cpr4, ch = idx - row * cpr4;
            const int m = m0 + row;
            if (m < p.M) *reinterpret_cast<f32x4*>(ws + (int64_t)m * p.N + n0 + ch * 4) = *reinterpret_cast<const f32x4*>(sC + row * PF + ch * 4);
        }
        return;
    }

    const bool geglu = (p.flags & MOCA_EP_GEGLU) != 0;
    const int out_bn = geglu ? BN / 2 : BN;
    const int on0 = geglu ? n0 / 2 : n0;
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);

    if (p.flags & MOCA_EP_OUT_F32) {
        // fp32 output: stage the tile in fp32 (no intermediate rounding)
        float* sC = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = wave_n * (BN / 2) + nt * 16 + 4 * fg;
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + n0 + col);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int row = wave_m * 64 + mt * 16 + fr;
                *reinterpret_cast<f32x4*>(sC + row * BN + col) = acc[mt][nt] + bv;
            }
        }
        __syncthreads();
        const int cpr = BN / 4;
        for (int idx = tid; idx < TM * cpr; idx += 512) {
            const int row = idx / cpr, ch = idx - row * cpr;
            const int m = m0 + row;
            if (m >= p.M) continue;
            const int col = n0 + ch * 4;
            f32x4 v = *reinterpret_cast<const f32x4*>(sC + row * BN + ch * 4);
            if (rowadd) {
                const half4v e = *reinterpret_cast<const half4v*>(rowadd + (int64_t)(m / p.rowadd_div) * p.ld_rowadd + col);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] += (float)e[j];
            }
            if (resid) {
                const half4v e = *reinterpret_cast<const half4v*>(resid + (int64_t)m * p.ldr + col);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] += (float)e[j];
            }
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.out) + (int64_t)m * p.ldo + col) = v;
        }
        return;
    }

    // fp16 output: stage fp16 rows (pitch = out_bn*2 + 16 bytes: conflict-free ds_write_b64 / ds_read_b128)
    const int pitch = out_bn * 2 + 16;
    if (geglu) {
        if constexpr (NT == 4) {
            // wave span of 64 packed columns = 32 value columns (tiles 0,1) then their 32 gate columns (tiles 2,3)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int ncol = n0 + wave_n * 64 + nt * 16 + 4 * fg;
                f32x4 bv = {0.f, 0.f, 0.f, 0.f}, bg = {0.f, 0.f, 0.f, 0.f};
                if (p.bias) { bv = *reinterpret_cast<const f32x4*>(p.bias + ncol); bg = *reinterpret_cast<const f32x4*>(p.bias + ncol + 32); }
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const int row = wave_m * 64 + mt * 16 + fr;
                    const f32x4 va = acc[mt][nt] + bv, ga = acc[mt][nt + 2] + bg;
                    const f32x2 lo = moca_geglu2(f32x2{va[0], va[1]}, f32x2{ga[0], ga[1]});
                    const f32x2 hi = moca_geglu2(f32x2{va[2], va[3]}, f32x2{ga[2], ga[3]});
                    half4v h;
                    h[0] = (half_t)lo[0]; h[1] = (half_t)lo[1]; h[2] = (half_t)hi[0]; h[3] = (half_t)hi[1];
                    *reinterpret_cast<half4v*>(smem + row * pitch + (wave_n * 32 + nt * 16 + 4 * fg) * 2) = h;
                }
            }
        }
    } else {
        const bool fold = (p.flags & MOCA_EP_LNFOLD) != 0;     // Linear(LayerNorm(x)) from x (no GEGLU / split-k on this kernel)
        float* rst = reinterpret_cast<float*>(smem + TM * (BN * 2 + 16));
        if (fold) lnfold_publish<TM, BN>(lf, rst, tid);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = wave_n * (BN / 2) + nt * 16 + 4 * fg;
            f32x4 bv, ws4 = {0.f, 0.f, 0.f, 0.f};
            if (fold) { ws4 = *reinterpret_cast<const f32x4*>(rst + 2 * TM + col); bv = *reinterpret_cast<const f32x4*>(rst + 2 * TM + BN + col); }
            else bv = ld4_or_zero(p.bias, n0 + col);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int row = wave_m * 64 + mt * 16 + fr;
                f32x4 v;
                if (fold) v = lnfold_apply(acc[mt][nt], *reinterpret_cast<const float2*>(rst + 2 * row), ws4, bv);
                else v = acc[mt][nt] + bv;
                *reinterpret_cast<half4v*>(smem + row * pitch + col * 2) = __builtin_convertvector(v, half4v);
            }
        }
    }
    __syncthreads();
    MOCA_STAMP(4);

    // (MOCA_EP_COLSUM / MOCA_EP_ROWSUM are only accepted without GEGLU / split-k: out_bn == BN; 256 x 272 B or 256 x 336 B of
    //  staged rows + the 32 x BN x 2 / 25 x BN x 2 floats of row-subset sums fit inside the 144 / 156 KiB ring)
    if (p.flags & (MOCA_EP_COLSUM | MOCA_EP_GSTAT)) store_fp16_tile_colsum<TM, BN>(p, smem, reinterpret_cast<float*>(smem + TM * (BN * 2 + 16)), pitch, m0, n0, tile_m, tid);
    else if (p.flags & MOCA_EP_ROWSUM) store_fp16_tile_rowsum<512, BN, 4>(p, smem, pitch, TM, m0, n0, tid);
    else store_fp16_tile<512>(p, smem, pitch, TM, out_bn, m0, on0, tid);
    MOCA_STAMP(5);
    MOCA_STAMP_HW();
}

// =====================================================================================
// "g4" kernel: 256 x 128 x 32 block tile, 256 threads = 4 wavefronts (2 x 2), wave tile 128 x 64 as 8 x 4
// v_mfma_f32_16x16x32_f16 accumulators, 3-slot direct-to-LDS ring of 24 KiB k-tiles = 72 KiB per block, so
// TWO blocks are resident per CU (8 waves, 2 per SIMD, <= 256 VGPRs each).  The two blocks run different
// tiles out of phase: one block's prologue (first-DMA latency), barriers and epilogue (bias/GEGLU/stores)
// sit under the other block's MFMAs -- the structural stall of the 8-wave kernel above, where the single
// resident block leaves the matrix pipe idle in those phases (s_memtime stamps: main loop only 35-42 % of a
// K = 320 tile).  One 32-deep k-tile = one MFMA k-step: per tile 32 MFMAs, 12 fragment ds_read_b128 and 6 DMA
// pieces per wave, one s_barrier; fragments are double-buffered in registers, the DMA runs three tiles ahead.
// LDS rows are 64 B, their 16-byte chunks swizzled by swz64() (gemm_device.h).
// =====================================================================================
template <int AMODE, bool FAST>
__global__ __launch_bounds__(256, 2) void gemm_g4_kernel(const moca_gemm_params p) {
    constexpr int TM = 256, BN = 128, KS = 32;
    constexpr int RB = KS * 2;                         // 64-byte LDS rows
    constexpr int MT = 8, NT = 4;
    constexpr int A_BYTES = TM * RB;                   // 16 KiB
    constexpr int B_BYTES = BN * RB;                   // 8 KiB
    constexpr int STAGE = A_BYTES + B_BYTES;           // 24 KiB
    constexpr int NMMA = MT * NT;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    MOCA_STAMP(0);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1;

    const int tiles_m = (p.M + TM - 1) / TM;
    const int tiles_n = p.N / BN;
    const int nblk = tiles_m * tiles_n * p.splits;
    if (prefetch_block(p, nblk, 256)) return;
    int split = 0, tile_m, tile_n;
    if ((p.reserved4_ >> 8) > 1) {                       // 2-D XCD partition (see remap_tile_2d)
        remap_tile_2d(tiles_m, tiles_n, p.reserved4_ >> 8, tile_m, tile_n);
    } else {
        int logical;
        remap_block<BN>(nblk, logical);
        split = logical % p.splits;
        const int tile = logical / p.splits;
        tile_m = tile / tiles_n; tile_n = tile % tiles_n;
    }
    const int m0 = tile_m * TM, n0 = tile_n * BN;

    const int nk_total = 2 * ((p.K + 63) / 64);        // 64-deep units -> even
    const int kts = 2 * (((p.K + 63) / 64 + p.splits - 1) / p.splits);   // 64-deep units, as the host sizes the splits -> even
    const int kt_begin = split * kts;
    const int nk = min(kt_begin + kts, nk_total) - kt_begin;

    const half_t* __restrict__ Wptr = reinterpret_cast<const half_t*>(p.w);

    // DMA piece = 1 KiB = 16 rows x 64 B: lane -> row (lane>>2), physical chunk lane&3; A piece g of this
    // wave covers rows (g*4 + wave)*16 .. +15 (g = 0..3), W piece g rows (g*4 + wave)*16 .. (g = 0..1)
    const int lrow = lane >> 2, pch = lane & 3;
    const int lch = pch ^ swz64(lrow);     // logical chunk fetched into this lane's slot
    AGather<AMODE, FAST, 4, KS> ga(p, lch);
#pragma unroll
    for (int g = 0; g < 4; ++g) ga.init_row(g, m0 + (g * 4 + wave) * 16 + lrow);
    const half_t* w_row[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int n = n0 + (g * 4 + wave) * 16 + lrow;
        w_row[g] = Wptr + (int64_t)n * p.ldw + lch * 8;
    }

    // DMA piece j (0..3: A, 4..5: W) of tile kt (= the tile begin_tile() was called for, + odd) into ring slot `slot`
    auto dma_piece = [&](int kt, int slot, int j, int odd) {
        const lds_ptr sa = (lds_ptr)smem + slot * STAGE;
        if (j < 4) {
            __builtin_amdgcn_global_load_lds((glb_ptr)ga.src(kt, j, odd), sa + (j * 4 + wave) * 1024, 16, 0, 0);
        } else {
            const int g = j - 4;
            __builtin_amdgcn_global_load_lds((glb_ptr)(w_row[g] + kt * KS), sa + A_BYTES + (g * 4 + wave) * 1024, 16, 0, 0);
        }
    };
    // k-tiles travel in (even, odd) pairs: the two 64-byte halves of every 128-byte line are requested back to back
    // (one phase apart the 32 KiB vector L1 has turned over and every line crosses L2 -> L1 twice: +10-22 % on the short-K
    // linears, measured); the pair's 12 DMA instructions are interleaved, so a pair lands as a unit
    auto issue_pair = [&](int kt_even, int slot_even, int slot_odd) {
        ga.begin_tile(kt_even);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            dma_piece(kt_even, slot_even, j, 0);
            dma_piece(kt_even + 1, slot_odd, j, 1);
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fg = lane >> 4;
    // fragment byte offsets inside a slot (row base + swizzled chunk): constant per lane
    int a_off[MT], b_off[NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int row = wave_m * 128 + mt * 16 + fr;
        a_off[mt] = row * RB + ((fg ^ swz64(row)) << 4);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int row = wave_n * 64 + nt * 16 + fr;
        b_off[nt] = A_BYTES + row * RB + ((fg ^ swz64(row)) << 4);
    }

    // ONE fragment set: the LDS-read latency at the head of a phase is covered by the co-resident block's
    // wave on the same SIMD (the two blocks of a CU run out of phase), not by a second register set --
    // 128 accumulator + 48 fragment registers leave room for two blocks per CU.
    half8v af[MT], bf[NT];
    int s0 = 0, s1 = 1, s2 = 2;                 // ring slots of tiles i, i+1, i+2 (rotating registers, no modulo)
    const int kt_last_pair = kt_begin + nk - 2;  // nk is even
    // phase i: read tile i's fragments, 32 MFMAs.  EVEN phases also issue the pair (i+2, i+3): tile i+2 into the slot of
    // tile i-1, tile i+3 into tile i's own slot -- hence the barrier after the fragment reads (every wave has tile i in
    // registers before any wave's DMA overwrites it).  The pair must be complete at the end of the following odd phase.
    auto phase = [&](auto even_tag, int i) {
        constexpr bool even = decltype(even_tag)::value;
        const char* cur = smem + s0 * STAGE;
        const int kt2 = min(kt_begin + i + 2, kt_last_pair);
        if constexpr (even) ga.begin_tile(kt2);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = *reinterpret_cast<const half8v*>(cur + a_off[mt]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bf[nt] = *reinterpret_cast<const half8v*>(cur + b_off[nt]);
        if constexpr (even) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < NMMA; ++j) {
            const int mt = j / NT, nt = j % NT;
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[nt], af[mt], acc[mt][nt], 0, 0, 0);   // D^T: lane = row m
            if constexpr (even) {
                if (j % 5 == 2 && j / 5 < 6) {              // after MFMA 2, 7, ..., 27: piece j/5 of both tiles of the pair
                    dma_piece(kt2, s2, j / 5, 0);
                    dma_piece(kt2 + 1, s0, j / 5, 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        { const int t = s0; s0 = s1; s1 = s2; s2 = t; }
    };

    // ---- prologue: pair (0, 1) ----
    LnFoldRaw lraw = {float2{0.f, 0.f}, float2{0.f, 0.f}, 0.f, 0.f};
    if (p.flags & MOCA_EP_LNFOLD) lraw = lnfold_issue<TM, BN>(p, m0 + tid, n0 + tid, tid);
    issue_pair(kt_begin, 0, 1);
    LnFoldRegs lf = {0.f, 0.f, 0.f, 0.f};
    if (p.flags & MOCA_EP_LNFOLD) lf = lnfold_finish<TM, BN>(p, lraw, m0 + tid, tid);
    MOCA_STAMP(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    MOCA_STAMP(2);
    for (int i = 0; i < nk; i += 2) {
        phase(yes_t{}, i);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // tile i+1 landed with its partner; everyone is past tile i's MFMAs
        __builtin_amdgcn_s_barrier();
        phase(no_t{}, i + 1);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // pair (i+2, i+3) complete
        __builtin_amdgcn_s_barrier();
    }
    // (the last barrier also ends every fragment read: the ring is free for the epilogue)
    MOCA_STAMP(3);

    // ---- epilogue (same scheme as the 8-wave kernel): lane owns 4 consecutive columns of row
    //      m = wave_m*128 + mt*16 + fr: column n = wave_n*64 + nt*16 + 4*fg + r ----
    if (p.splits > 1) {
        float* ws = p.splitk_ws + (int64_t)split * p.M * p.N;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int row = m0 + wave_m * 128 + mt * 16 + fr;
            if (row < p.M) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int col = n0 + wave_n * 64 + nt * 16 + 4 * fg;
                    *reinterpret_cast<f32x4*>(ws + (int64_t)row * p.N + col) = acc[mt][nt];
                }
            }
        }
        return;
    }
    const bool geglu = (p.flags & MOCA_EP_GEGLU) != 0;
    const int out_bn = geglu ? BN / 2 : BN;
    const int on0 = geglu ? n0 / 2 : n0;
    const int pitch = out_bn * 2 + 16;
    const bool fold = (p.flags & MOCA_EP_LNFOLD) != 0;         // Linear(LayerNorm(x)) from x: row statistics -> LDS behind the staged tile
    float* rst = reinterpret_cast<float*>(smem + TM * (BN * 2 + 16));
    if (fold) lnfold_publish<TM, BN>(lf, rst, tid);
    if (geglu) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int lcol = wave_n * 64 + nt * 16 + 4 * fg, ncol = n0 + lcol;
            f32x4 bv, bg, wv = {0.f, 0.f, 0.f, 0.f}, wg = wv;
            if (fold) {
                wv = *reinterpret_cast<const f32x4*>(rst + 2 * TM + lcol); wg = *reinterpret_cast<const f32x4*>(rst + 2 * TM + lcol + 32);
                bv = *reinterpret_cast<const f32x4*>(rst + 2 * TM + BN + lcol); bg = *reinterpret_cast<const f32x4*>(rst + 2 * TM + BN + lcol + 32);
            } else {
                bv = ld4_or_zero(p.bias, ncol); bg = ld4_or_zero(p.bias, ncol + 32);
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int row = wave_m * 128 + mt * 16 + fr;
                f32x4 va, ga;
                if (fold) {
                    const float2 st = *reinterpret_cast<const float2*>(rst + 2 * row);
                    va = lnfold_apply(acc[mt][nt], st, wv, bv); ga = lnfold_apply(acc[mt][nt + 2], st, wg, bg);
                } else {
                    va = acc[mt][nt] + bv; ga = acc[mt][nt + 2] + bg;
                }
                const f32x2 lo = moca_geglu2(f32x2{va[0], va[1]}, f32x2{ga[0], ga[1]});
                const f32x2 hi = moca_geglu2(f32x2{va[2], va[3]}, f32x2{ga[2], ga[3]});
                half4v h;
                h[0] = (half_t)lo[0]; h[1] = (half_t)lo[1]; h[2] = (half_t)hi[0]; h[3] = (half_t)hi[1];
                *reinterpret_cast<half4v*>(smem + row * pitch + (wave_n * 32 + nt * 16 + 4 * fg) * 2) = h;
            }
        }
    } else {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = wave_n * 64 + nt * 16 + 4 * fg;
            f32x4 bv, ws4 = {0.f, 0.f, 0.f, 0.f};
            if (fold) { ws4 = *reinterpret_cast<const f32x4*>(rst + 2 * TM + col); bv = *reinterpret_cast<const f32x4*>(rst + 2 * TM + BN + col); }
            else bv = ld4_or_zero(p.bias, n0 + col);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int row = wave_m * 128 + mt * 16 + fr;
                f32x4 v;
                if (fold) v = lnfold_apply(acc[mt][nt], *reinterpret_cast<const float2*>(rst + 2 * row), ws4, bv);
                else v = acc[mt][nt] + bv;
                *reinterpret_cast<half4v*>(smem + row * pitch + col * 2) = __builtin_convertvector(v, half4v);
            }
        }
    }
    __syncthreads();
    MOCA_STAMP(4);
    store_fp16_tile<256>(p, smem, pitch, TM, out_bn, m0, on0, tid);
    MOCA_STAMP(5);
    MOCA_STAMP_HW();
}


// cross-lane steps of the in-epilogue temporal attention as VALU lane swaps (v_permlane16_swap / v_permlane32_swap: with both operands
// equal to x, the two results hold x and its partner 16 / 32 lanes away in every lane -- cdna_hip_programming.md T12 / T21) instead of
// ds_bpermute round trips through the LDS pipe; and the V^T operand by the transposing LDS read (common.h: lds_tr_read_b64)
#if defined(__HIP_DEVICE_COMPILE__)
#define MOCA_XLANE(NAME, SWAP, OP)                                                                         \
    __device__ __forceinline__ float NAME(float x) {                                                       \
        const auto r = SWAP(__float_as_uint(x), __float_as_uint(x), false, false);                         \
        const float a = __uint_as_float(r[0]), b = __uint_as_float(r[1]);                                  \
        return OP;                                                                                         \
    }
MOCA_XLANE(xlane16_max, __builtin_amdgcn_permlane16_swap, fmaxf(a, b))
MOCA_XLANE(xlane32_max, __builtin_amdgcn_permlane32_swap, fmaxf(a, b))
MOCA_XLANE(xlane16_sum, __builtin_amdgcn_permlane16_swap, a + b)
MOCA_XLANE(xlane32_sum, __builtin_amdgcn_permlane32_swap, a + b)
#undef MOCA_XLANE
#else
__device__ __forceinline__ float xlane16_max(float x) { return x; }
__device__ __forceinline__ float xlane32_max(float x) { return x; }
__device__ __forceinline__ float xlane16_sum(float x) { return x; }
__device__ __forceinline__ float xlane32_sum(float x) { return x; }
#endif

// =====================================================================================
// "w80s" kernel: the 320 x 160 x 32 tile / 80 x 80 wave tile / 5-slot ring of w80b, with the main loop cut into
// LOAD and MFMA SEGMENTS and the two waves of every SIMD running half an iteration apart.
//
// Why.  In w80/w80b every wave interleaves its own ds_reads and DMA instructions with its own MFMAs and all eight waves
// run in lockstep (one barrier per k-tile), so the two waves of a SIMD want the matrix pipe at the same moments and issue
// their memory instructions at the same moments.  Ablations on the same device (tools/ab_run1.sh): without the DMA
// instructions the conv loop runs 20 % faster, without the fragment reads 18 %, without both 39 % (1.6-1.8 PFLOP/s) --
// the costs ADD, i.e. nothing overlaps them; moving the DMA addressing to SGPR descriptors (w80b) or dropping 8 of 9 A
// fetches changes nothing, so it is neither the address arithmetic nor the L2->LDS bytes: it is the in-order issue of
// each wave.  Here a wave's MFMAs issue back to back from registers (25 per k-tile, nothing in between) while its SIMD
// partner is in its LOAD segment (fragment reads for two k-tiles, or the 8 DMA instructions of a k-tile pair, and the
// counted waits), and vice versa: waves 4..7 pass one extra barrier before the loop and waves 0..3 one after it, so the
// halves stay exactly one barrier apart (MI355X_MICROARCH.md, "Two waves per SIMD", items 5 and 9).
//
// One iteration = two k-tiles (i, i+1), four barriers:
//   LOADe : 10 ds_read_b128 -- the fragments of tile i;  lgkmcnt(0);  barrier
//   MFMAe : 25 MFMAs of tile i with the 10 fragment reads of tile i+1 (second register set) in the gaps;  lgkmcnt(0);  barrier
//   LOADo : 8 DMA instructions = the pair (i+4, i+5) into the slots of tiles i-1 and i (both in registers everywhere: the
//           partner half finished its LOADe reads before the barrier this half has just passed);  vmcnt(8): the pair
//           (i+2, i+3) of this wave has landed;  barrier
//   MFMAo : 25 MFMAs of tile i+1;  barrier
// A DMA has two k-tiles of time to land (as in w80); data is read two barriers after the wait that retires it.
// =====================================================================================
// WIDE = false: 320 x 160 block tile, waves 4 (M) x 2 (N).  WIDE = true ("w80t"): 160 x 320, waves 2 x 4 -- the same 80 x 80 wave
// tiles, ring and DMA stream with the roles of A and W swapped (10 A pieces + 20 W pieces per k-tile): a block then owns
// COMPLETE output rows when N = 320, so A is fetched once instead of once per 160-column tile and the LayerNorm that follows the
// attention / projection linears of the 320-channel level (attention.py:199-201,216-219) runs in the store loop (MOCA_EP_LN).
// SHAPE 2 ("sq256"): 256 x 256 block tile, waves 4 x 2, wave tile 64 x 128 (4 x 8 MFMA tiles, 32 MFMAs per k-tile) -- the same
// staggered structure for the wide projections (GEGLU N = 2560 / 5120 / 10240, QKV N = 3840): 7.8 B of L2->LDS traffic per kFLOP
// against 9.4 for 320 x 160 and 11.7 for 256 x 128; 16 + 16 DMA pieces per k-tile = 4 per wave, no repeats; the ring takes all
// 160 KiB of LDS.  GEGLU epilogue: a wave's 128 packed columns = two 64-column groups of 32 value + 32 gate columns.
// The kernel's text lives in gemm_w80s_kernel.inc and is compiled twice: as gemm_w80s_kernel<AMODE, SHAPE> -- the text and the code
// it always was -- and as gemm_w80s_causal_kernel<MOCA_A_LINEAR, 3>, whose MOCA_EP_TATTN epilogue carries the causal mask of
// TemporalTransformer(causal_attention=True) (moca_gemm_params.tattn_causal).  A compile-time switch of a second template, not a
// third template argument or a run-time flag: the non-causal kernels keep their names and their instruction streams.
#define MOCA_W80S_NAME gemm_w80s_kernel
#define MOCA_W80S_CAUSAL false
#include "gemm_w80s_kernel.inc"
#undef MOCA_W80S_NAME
#undef MOCA_W80S_CAUSAL
#define MOCA_W80S_NAME gemm_w80s_causal_kernel
#define MOCA_W80S_CAUSAL true
#include "gemm_w80s_kernel.inc"
#undef MOCA_W80S_NAME
#undef MOCA_W80S_CAUSAL

// CAUSAL (SHAPE 3 only): the same launch on gemm_w80s_causal_kernel (moca_gemm_params.tattn_causal)
template <int AMODE, int SHAPE, bool CAUSAL = false>
int launch_gemm_w80s(const moca_gemm_params& p, hipStream_t st) {
    constexpr auto kernel = [] {
        if constexpr (CAUSAL) return &gemm_w80s_causal_kernel<AMODE, SHAPE>;
        else return &gemm_w80s_kernel<AMODE, SHAPE>;
    }();
    constexpr int TM = SHAPE == 2 ? 256 : (SHAPE == 1 ? 160 : 320), BN = SHAPE == 2 ? 256 : (SHAPE == 1 ? 320 : (SHAPE == 3 ? 192 : 160));
    const int tiles_m = (p.M + TM - 1) / TM, tiles_n = p.N / BN;
    const int nblk = tiles_m * tiles_n * p.splits;
    moca_gemm_params pl = p;
    pl.reserved4_ = (pl.reserved4_ & 0xff) | ((SHAPE == 3 ? 1 : choose_xcd_n(p, tiles_m, tiles_n, BN)) << 8);
    constexpr int lds = 5 * (TM + BN) * 64;              // 150 KiB (160 KiB for 256 x 256); the fp16 epilogue tile fits inside the ring
    if (!dyn_lds_once<kernel>(lds)) return MOCA_E_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3(nblk + prefetch_blocks(pl)), dim3(512), lds, st, pl);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

template <int BN, int AMODE, bool FAST>
int launch_gemm_glds(const moca_gemm_params& p, hipStream_t st) {
    const int tiles_m = (p.M + 255) / 256, tiles_n = p.N / BN;
    const int nblk = tiles_m * tiles_n * p.splits;
    constexpr int lds_pipe = 3 * (256 + BN) * ROW_BYTES;
    constexpr int lds_epi = 256 * BN * 4;
    constexpr int lds = lds_pipe > lds_epi ? lds_pipe : lds_epi;
    if (!dyn_lds_once<&gemm_glds_kernel<BN, AMODE, FAST>>(lds)) return MOCA_E_LAUNCH;
    hipLaunchKernelGGL((gemm_glds_kernel<BN, AMODE, FAST>), dim3(nblk + prefetch_blocks(p)), dim3(512), lds, st, p);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

template <int AMODE, bool FAST>
int launch_gemm_g4(const moca_gemm_params& p, hipStream_t st) {
    const int tiles_m = (p.M + 255) / 256, tiles_n = p.N / 128;
    const int nblk = tiles_m * tiles_n * p.splits;
    constexpr int lds = 3 * (256 + 128) * 64;       // 72 KiB ring; the fp16 epilogue tile (256 x 272 B) fits inside it
    if (!dyn_lds_once<&gemm_g4_kernel<AMODE, FAST>>(lds)) return MOCA_E_LAUNCH;
    moca_gemm_params pl = p;
    pl.reserved4_ = (pl.reserved4_ & 0xff) | (choose_xcd_n(p, tiles_m, tiles_n, 128) << 8);
    hipLaunchKernelGGL((gemm_g4_kernel<AMODE, FAST>), dim3(nblk + 2 * prefetch_blocks(pl)), dim3(256), lds, st, pl);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

}  // namespace

int moca_gemm_glds_launch(int bn, const moca_gemm_params& p, hipStream_t st) {
    if (bn == 128) return with_gather(p, [&](auto am, auto fast) { return launch_gemm_glds<128, decltype(am)::value, decltype(fast)::value>(p, st); });
    return with_gather(p, [&](auto am, auto fast) { return launch_gemm_glds<160, decltype(am)::value, decltype(fast)::value>(p, st); });
}
int moca_gemm_g4_launch(const moca_gemm_params& p, hipStream_t st) {
    return with_gather(p, [&](auto am, auto fast) { return launch_gemm_g4<decltype(am)::value, decltype(fast)::value>(p, st); });
}

int moca_gemm_w80s_launch(int shape, const moca_gemm_params& p, hipStream_t st) {
    switch (shape) {
        case 0:
            if (p.a2) return launch_gemm_w80s<MOCA_A_LINEAR2, 0>(p, st);
            return with_gather(p, [&](auto am, auto) { return launch_gemm_w80s<decltype(am)::value, 0>(p, st); });
        case 1:
            if (p.a2) return launch_gemm_w80s<MOCA_A_LINEAR2, 1>(p, st);
            return with_gather(p, [&](auto am, auto) { return launch_gemm_w80s<decltype(am)::value, 1>(p, st); });
        case 2: return launch_gemm_w80s<MOCA_A_LINEAR, 2>(p, st);
        case 3: return p.tattn_causal ? launch_gemm_w80s<MOCA_A_LINEAR, 3, true>(p, st) : launch_gemm_w80s<MOCA_A_LINEAR, 3>(p, st);
    }
    return MOCA_E_BADARG;
}
