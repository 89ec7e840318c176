// "w80h": the 320 x 160 staggered kernel (gemm_w80s_kernel.inc, SHAPE 0) with an LDS-RESIDENT HALO TILE as its A operand, for the
// stride-1 3 x 3 convs whose 320-row tiles are whole image rows of one frame (inW = 64: 5 rows, inW = 32: 10 rows).
//
// The gather of w80s sends every input row through the LDS-DMA path once per tap, nine times in all.  Here the (rows + 2) x inW
// input pixels a tile's 3 x 3 neighbourhood covers are fetched ONCE per 32-channel slice, and the fragment read of tap (dy, dx) reads
// the halo at (row + dy, x + dx - 1).
//
// k walk: channel-slice-major, tap-minor, two slices at a time -- iteration (pair jp, tap t) = the two k-tiles (tap t, slice 2 jp)
// and (tap t, slice 2 jp + 1).  Their W k-tiles are the two 64-byte halves of one 128-byte line of the packed [N][(ky,kx,c)]
// weights at k = t C + 64 jp: the (even, odd) pair of w80s, no repacking.  Their A operands are two halo slots that stay in LDS
// for the nine taps.  An odd slice count (C % 64 == 32) ends with a pair whose odd half is zero (out-of-range DMA offsets).
//
// Halo slot (one 32-channel slice): [64 B gap] then per halo row [inW pixels as inW / 16 DMA pieces][64 B gap]; the gaps are zeroed
// once per block and never written again: they are the two padding columns.  A DMA piece (1 KiB, lane-linear) holds 16 pixels
// CHUNK-major -- lane = chunk * 16 + pixel -- so the 16 lanes of a ds_read_b128 group (one chunk, 16 consecutive pixels, from ANY
// starting pixel, also across two pieces) cover all 64 banks: the dx = +-1 shifts are conflict-free by construction, no XOR swizzle.
// Wave (wave_m, wave_n) owns the 16-pixel column block cb = wave_m % (inW / 16) of the image rows 5 (wave_m / (inW / 16)) + mt, so
// that the fragment address of (mt, dy) is an IMMEDIATE (mt + dy) * row pitch on one of three per-lane registers (one per dx, which
// carry the pad-column redirection of the block's first / last lane).  Rows above / below the image take offsets >= 2^31: the
// range check writes zeros.
//
// LDS: 4 halo slots (two pairs: one in use, one landing) of 29 184 B (inW = 64) / 25 408 B (inW = 32) + a 4-slot W ring of 10 KiB
// k-tiles + 1 KiB for the DMA instructions that have nothing to fetch = 158 720 B / 143 616 B.  The W ring has 4 slots, not 5,
// because the halves of the workgroup split the pair: waves 0..3 fetch the even W k-tile into the slot of tile i (read by everyone),
// waves 4..7 -- one barrier behind -- the odd one into the slot of tile i + 1, which their own half has just finished reading.
//
// vmcnt accounting: every wave issues exactly 4 DMA instructions per iteration in LOADo -- 2 or 3 W pieces of its half of the pair
// two iterations ahead and 2 or 1 halo pieces of the NEXT slice pair (12 per iteration, tap-iterations 0..4 carry the 56 / 48
// pieces, later ones go to the 1 KiB dump with out-of-range offsets) -- then `s_waitcnt vmcnt(4)`: the previous iteration's four
// have landed; they are read two barriers later, as in w80s.  The (even, odd) halves of a 128-byte line are NOT issued back to back
// by one wave as in w80s: for W they come from the two halves of the workgroup, one barrier apart; for the halo they are neighbouring
// piece indices, i.e. neighbouring waves (wave w takes piece 12 t + 4 + w) in the same LOADo segment.  Measured: FETCH_SIZE per launch
// -21 % against the gather (profiles/r07_ab_conv_halo.txt).  The segments (LOADe / MFMAe / LOADo / MFMAo), the stagger of the two
// halves, the 5 x 5 16x16x32 wave tile and the epilogues are those of w80s SHAPE 0.
//
// A translation unit of its own: the code hipcc generates for the shared store loops follows all their callers in a unit
// (gemm_tiled.hip), and the kernels there keep their instruction streams.
#include "gemm_launch.h"

namespace {

template <int IW>
__global__ __launch_bounds__(512, 2) void gemm_w80h_kernel(const moca_gemm_params p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int MT = 5, NT = 5, KS = 32, RB = 64;
    constexpr int TM = 320, BN = 160, WTN = 80;
    constexpr int NB = IW / 16;                          // 16-pixel column blocks per image row
    constexpr int HR = TM / IW + 2;                      // halo rows
    constexpr int ROWB = IW * RB + 64;                   // halo row pitch: pixels + gap
    constexpr int HSLOT = 64 + HR * ROWB;
    constexpr int NP2 = 2 * HR * NB;                     // DMA pieces of a slice pair, index = (halo row * NB + block) * 2 + parity
    constexpr int WT = BN * RB;
    constexpr int WRING = 4 * HSLOT, DUMP = WRING + 4 * WT;
    constexpr int APER = 12;                             // halo pieces per iteration: 4 in slot j = 2, 8 in slot j = 3
    static_assert(8 * APER >= NP2 && HSLOT + (MT + 1) * ROWB < 65536, "halo schedule / ds_read immediates");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1, wq = wave & 3;
    const int cb = wave_m % NB, rg = wave_m / NB;
    const bool late = wave >= 4;                         // the half of the workgroup that runs one barrier behind
    const int half = late ? 1 : 0;                       // ... and fetches the odd W k-tile of every pair

    const int tiles_n = p.N / BN;
    const int nblk = (p.M / TM) * tiles_n;
    if (prefetch_block(p, nblk, 512)) return;
    int logical;
    remap_block<BN>(nblk, logical);
    const int tile_m = logical / tiles_n, tile_n = logical % tiles_n;
    const int m0 = tile_m * TM, n0 = tile_n * BN;
    const int hw = p.inH * IW;
    const int frame = m0 / hw;
    const int y0 = (m0 - frame * hw) / IW;
    const int pix0 = frame * hw;
    const int npairs = (p.C / KS + 1) >> 1;

    // gaps (padding columns) of the four halo slots
    if (tid < 16 * (HR + 1)) {
        const int sl = tid / (4 * (HR + 1)), rem = tid - sl * 4 * (HR + 1);
        *reinterpret_cast<f32x4*>(smem + sl * HSLOT + (rem >> 2) * ROWB + (rem & 3) * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, OOB_OFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, OOB_OFF, 0x00020000);
    // halo piece: lane -> pixel lane & 15 of the block, chunk lane >> 4
    const unsigned a_voff = (unsigned)(((lane & 15) * p.C + (lane >> 4) * 8) * 2);
    // W piece (as w80s): lane -> row lane >> 2, physical chunk lane & 3; this wave's pieces wq, 4 + wq and (wq < 2) 8 + wq
    const int lrow = lane >> 2, pch = lane & 3;
    const int lch = pch ^ swz64(lrow);
    unsigned w_off[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) w_off[g] = (unsigned)(((int64_t)(n0 + ((g < 2 ? g * 4 + wq : 8 + (wq & 1))) * 16 + lrow) * p.ldw + lch * 8) * 2);

    // (everything but a_voff is wave-uniform.  y0v / pix0v / wavev = y0 / pix0 / wave behind an empty asm in the loop: otherwise the
    //  row offset, the LDS address and the in-image flag of each of the loop body's halo pieces are hoisted out of the slice-pair loop
    //  and spill 50 SGPRs)
    auto dma_a = [&](int idx, int jpA, bool live, int y0v, int pix0v) {
        const int par = idx & 1, pq = idx >> 1;
        const int Y = pq / NB, q = pq % NB;
        const int iy = y0v - 1 + Y, slice = 2 * jpA + par;
        const bool listed = live && idx < NP2;
        const bool ok = listed && iy >= 0 && iy < p.inH && slice * KS < p.C;
        const unsigned soff = ok ? ((unsigned)((pix0v + iy * IW + q * 16) * p.C + slice * KS)) * 2u : 0u;
        const int dst = listed ? ((jpA & 1) * 2 + par) * HSLOT + 64 + Y * ROWB + q * 1024 : DUMP;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (lds_ptr)smem + dst, 16, ok ? a_voff : OOB_OFF, soff, 0, 0);
    };
    // the four DMA instructions of a wave: its half of the W pair (tap t2, slice pair jp2) into ring slots wsl / wsl + 1, and the halo
    // pieces tA * 12 + k of slice pair jpA
    auto issue = [&](int t2, int jp2, int wsl, int tA, int jpA, int y0v, int pix0v, int wavev) {
        const bool wok = jp2 < npairs && (!late || (2 * jp2 + 1) * KS < p.C);
        const unsigned w_s = wok ? (unsigned)((t2 * p.C + jp2 * 64 + half * KS) * 2) : 0u;
        const lds_ptr wd = (lds_ptr)smem + WRING + (wsl + half) * WT;
        const bool alive = tA < 8 && jpA < npairs;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, wd + wq * 1024, 16, wok ? w_off[0] : OOB_OFF, w_s, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, wd + (4 + wq) * 1024, 16, wok ? w_off[1] : OOB_OFF, w_s, 0, 0);
        if (wq < 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, wd + (8 + wq) * 1024, 16, wok ? w_off[2] : OOB_OFF, w_s, 0, 0);
        else dma_a(tA * APER + half * 2 + (wq - 2), jpA, alive, y0v, pix0v);
        dma_a(tA * APER + 4 + wavev, jpA, alive, y0v, pix0v);
    };

    const int fr = lane & 15, fg = lane >> 4;
    f32x4 acc[MT][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + n0 + wave_n * WTN + nt * 16 + 4 * fg);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = bv;
    }

    // fragment addresses.  W as w80s.  A: per dx one register = the lane's pixel (fr + dx - 1 of block cb) in halo row 5 rg of slot 0;
    // (mt, dy) and the odd slot are immediates.  The block's pixel -1 / 16 is the neighbouring piece, or -- at the image's edge -- the gap.
    const int swz = (fg ^ swz64(fr)) << 4;
    const int b_off0 = WRING + (wave_n * WTN + fr) * RB + swz;
    int a_base[3], a_cur[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
        const int X = fr + dx - 1;
        int o = cb * 1024 + (X >> 4) * 1024 + (X & 15) * 16 + fg * 256;
        if (X < 0 && cb == 0) o = -16;
        if (X > 15 && cb == NB - 1) o = IW * RB;
        a_base[dx] = 64 + rg * 5 * ROWB + o;
    }

    half8v af[2][MT], bf[2][NT];

    // ---- prologue: halo pair 0 and the W pairs of iterations 0 and 1 in flight, all but the last landed everywhere ----
#pragma unroll
    for (int k = 0; k < (NP2 + 7) / 8; ++k) dma_a(k * 8 + wave, 0, true, y0, pix0);
    issue(0, 0, 0, 8, 0, y0, pix0, wave);
    issue(1, 0, 2, 8, 0, y0, pix0, wave);
    asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (late) __builtin_amdgcn_s_barrier();            // from here on waves 4..7 run one barrier behind waves 0..3

    int wsl = 0;                                         // W ring slot of the iteration's even k-tile (0 or 2)
    for (int jp = 0; jp < npairs; ++jp) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) a_cur[dx] = a_base[dx] + (jp & 1) * 2 * HSLOT;
        auto iter = [&](auto tap_tag) {
            constexpr int T = decltype(tap_tag)::value, DY = T / 3, DX = T % 3;
            const char* we = smem + wsl * WT + b_off0;
            const char* ae = smem + a_cur[DX];
            // ---- LOADe: the fragments of the even k-tile ----
#pragma unroll
            for (int r = 0; r < NT; ++r) bf[0][r] = *reinterpret_cast<const half8v*>(we + r * 1024);
#pragma unroll
            for (int r = 0; r < MT; ++r) af[0][r] = *reinterpret_cast<const half8v*>(ae + (r + DY) * ROWB);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // ---- MFMAe with the reads of the odd k-tile in the gaps ----
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int j = 0; j < MT * NT; ++j) {
                const int mt = j / NT, nt = j % NT;
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[0][nt], af[0][mt], acc[mt][nt], 0, 0, 0);
                if (j % 2 == 0 && j / 2 < MT + NT) {
                    const int r = j / 2;
                    __builtin_amdgcn_sched_barrier(0);
                    if (r < NT) bf[1][r] = *reinterpret_cast<const half8v*>(we + WT + r * 1024);
                    else af[1][r - NT] = *reinterpret_cast<const half8v*>(ae + HSLOT + (r - NT + DY) * ROWB);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __builtin_amdgcn_s_setprio(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // ---- LOADo: W of the iteration after next into this iteration's slots, halo pieces of the next slice pair ----
            int y0v = y0, pix0v = pix0, wavev = wave;
            asm volatile("" : "+s"(y0v), "+s"(pix0v), "+s"(wavev));
            issue((T + 2) % 9, jp + (T + 2) / 9, wsl, T, jp + 1, y0v, pix0v, wavev);
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // ---- MFMAo ----
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[1][nt], af[1][mt], acc[mt][nt], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            wsl ^= 2;
        };
        iter(int_c<0>{}); iter(int_c<1>{}); iter(int_c<2>{});
        iter(int_c<3>{}); iter(int_c<4>{}); iter(int_c<5>{});
        iter(int_c<6>{}); iter(int_c<7>{}); iter(int_c<8>{});
    }
    if (!late) __builtin_amdgcn_s_barrier();           // the halves meet again
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                      // every DMA is done: LDS is free for the epilogue

    // ---- epilogue (as w80s SHAPE 0): lane owns 4 consecutive columns of tile row (5 rg + mt) * IW + 16 cb + fr ----
    constexpr int pitch = BN * 2 + 16;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = wave_n * WTN + nt * 16 + 4 * fg;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int row = (rg * 5 + mt) * IW + cb * 16 + fr;
            *reinterpret_cast<half4v*>(smem + row * pitch + col * 2) = __builtin_convertvector(acc[mt][nt], half4v);
        }
    }
    __syncthreads();
    if (p.flags & (MOCA_EP_COLSUM | MOCA_EP_GSTAT)) store_fp16_tile_colsum<TM, BN>(p, smem, reinterpret_cast<float*>(smem + TM * pitch), pitch, m0, n0, tile_m, tid);
    else if (p.flags & MOCA_EP_ROWSUM) store_fp16_tile_rowsum<512, BN, 4>(p, smem, pitch, TM, m0, n0, tid);
    else store_fp16_tile<512>(p, smem, pitch, TM, BN, m0, n0, tid);
#endif
}

template <int IW>
int launch_gemm_w80h(const moca_gemm_params& p, hipStream_t st) {
    constexpr int HR = 320 / IW + 2;
    constexpr int lds = 4 * (64 + HR * (IW * 64 + 64)) + 4 * 160 * 64 + 1024;
    const int nblk = (p.M / 320) * (p.N / 160);
    moca_gemm_params pl = p;
    pl.reserved4_ = (pl.reserved4_ & 0xff) | (1 << 8);    // (1-D XCD partition: what choose_xcd_n gives every conv launch)
    if (!dyn_lds_once<&gemm_w80h_kernel<IW>>(lds)) return MOCA_E_LAUNCH;
    hipLaunchKernelGGL(gemm_w80h_kernel<IW>, dim3(nblk + prefetch_blocks(pl)), dim3(512), lds, st, pl);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

}  // namespace

int moca_gemm_w80h_launch(const moca_gemm_params& p, hipStream_t st) {
    if (p.inW == 64) return launch_gemm_w80h<64>(p, st);
    if (p.inW == 32) return launch_gemm_w80h<32>(p, st);
    return MOCA_E_BADARG;
}
