// Device helpers that more than one GEMM kernel family uses (gemm.hip, gemm_tiled.hip, gemm_persistent.hip): tile
// constants and block remaps (remap_block, xcd_range), the chunk swizzle of 64-byte LDS rows (swz64), the prefetch blocks, the stamps of
// the diagnostic build, the buffer-addressed A gather, the store loops of the staged fp16 tile, the plain store from registers
// (store8_rowadd_res) and the LayerNorm fold (lnfold_*).  Everything here has internal linkage; the guard lets the diagnostic unity build
// (gemm_diag.hip) see it once.
#ifndef MOCA_GEMM_DEVICE_H
#define MOCA_GEMM_DEVICE_H
#include "common.h"

namespace {

template <int V> struct int_c { static constexpr int value = V; };
struct yes_t { static constexpr bool value = true; };
struct no_t { static constexpr bool value = false; };

constexpr int BM = 128;
constexpr int BK = 64;
constexpr int MOCA_A_LINEAR2 = 3;      // internal: MOCA_A_LINEAR with moca_gemm_params.a2 (two-source A = virtual torch.cat), staggered kernels only
constexpr int ROW_BYTES = BK * 2;  // 128 B per LDS row

struct Geo {
    // conv3x3 / tconv geometry in registers
    int C, inH, inW, outH, outW, stride, up, T, HW;
};

// 2-D XCD partition of the tile grid: XCD (i, j) of an xm x xn arrangement (xm * xn = 8) owns the sub-grid of tiles_m / xm row
// tiles x tiles_n / xn column tiles and walks it column-fastest.  With the 1-D partition above every XCD streams ALL of W once per
// M tile it owns: at the 1280-channel level (K = 1280, N = 10240: W = 26 MB against a 4 MB L2) rocprofv3 shows 559 MB of fabric
// reads per GEGLU launch for 39 MB of operands.  (xm, xn) is chosen on the host to minimise (rows of A + rows of W) per XCD and only
// when both divide; p.reserved4_ >> 8 carries xn (0 / 1: the 1-D partition).
__device__ __forceinline__ void remap_tile_2d(int tiles_m, int tiles_n, int xn, int& tile_m, int& tile_n) {
    const int xm = 8 / xn;
    const int sm = tiles_m / xm, sn = tiles_n / xn;          // sub-grid of one XCD
    const int b = blockIdx.x;
    const int xcd = b & 7, j = b >> 3;                        // j-th tile of this XCD
    const int xi = xcd / xn, xj = xcd - xi * xn;
    tile_m = xi * sm + j / sn;
    tile_n = xj * sn + j % sn;
}

// Blocks nblk .. gridDim.x - 1 of a launch with p.prefetch: no tile, they read the next weight-heavy launch's weights once (plain
// 16-byte loads, 8 in flight per lane; the values are dropped) so that those lines sit in the Infinity Cache when that launch asks
// for them.  They are dispatched after every tile block, i.e. onto the CUs this launch leaves idle or onto its tail.
constexpr int PREFETCH_BLOCKS = 24;
__device__ __forceinline__ bool prefetch_block(const moca_gemm_params& p, int nblk, int nthreads) {
    if ((int)blockIdx.x < nblk) return false;
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(p.prefetch);
    const int64_t n16 = (int64_t)p.prefetch_kib << 6;
    const int64_t stride = (int64_t)((int)gridDim.x - nblk) * nthreads;
    int64_t i = (int64_t)((int)blockIdx.x - nblk) * nthreads + threadIdx.x;
    unsigned acc = 0;
    for (; i + 7 * stride < n16; i += 8 * stride) {
        uint4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[i + j * stride];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc ^= v[j].x ^ v[j].y ^ v[j].z ^ v[j].w;
    }
    for (; i < n16; i += stride) { const uint4 v = src[i]; acc ^= v.x ^ v.y ^ v.z ^ v.w; }
    asm volatile("" :: "v"(acc));                     // keeps the loads; nothing is stored
    return true;
}
static inline int prefetch_blocks(const moca_gemm_params& p) { return (p.prefetch && p.prefetch_kib > 0) ? PREFETCH_BLOCKS : 0; }

// 1-D XCD partition of a raster of ntiles tiles: XCD x (0..7) owns the contiguous range [start, start + count), the first ntiles % 8
// XCDs one tile more than the others
__device__ __forceinline__ void xcd_range(int ntiles, int x, int& start, int& count) {
    const int q = ntiles >> 3, r = ntiles & 7;
    start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    count = q + (x < r ? 1 : 0);
}

template <int BN>
__device__ __forceinline__ void remap_block(int nblk, int& logical) {
    // XCD-aware bijective remap: physical blocks b, b+8, b+16, ... share an XCD (L2);
    // give each XCD a contiguous range of logical tiles so neighbours share A rows.
    const int b = blockIdx.x;
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = b & 7, j = b >> 3;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

// 64-byte LDS rows (one 32-deep k-tile row = four 16-byte chunks): chunk swizzle phys = chunk ^ swz64(row), swz64 = f((row >> 2) & 3) with
// f = {0, 2, 3, 1} -- conflict-free for the four 16-lane groups of ds_read_b128 on the 16x16x32 operand map (derivation in DESIGN.md).
// The LDS image of a DMA is lane-linear, so the DMA applies it to the SOURCE chunk a lane fetches; the fragment reads to the address.
__device__ __forceinline__ int swz64(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }

#ifdef MOCA_STAMPS
// diagnostic build only (-DMOCA_STAMPS): per-block s_memtime stamps, read back with moca_debug_stamps()
constexpr int STAMP_SLOTS = 16, STAMP_BLOCKS = 16384;
__device__ unsigned long long g_stamps[STAMP_BLOCKS * STAMP_SLOTS];
#define MOCA_STAMP(k)                                                                              \
    do {                                                                                           \
        if (threadIdx.x == 0 && blockIdx.x < STAMP_BLOCKS) {                                       \
            unsigned long long t__;                                                                \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");            \
            g_stamps[blockIdx.x * STAMP_SLOTS + (k)] = t__;                                        \
        }                                                                                          \
    } while (0)
#define MOCA_STAMP_W(k, w)                                                                         \
    do {                                                                                           \
        if (threadIdx.x == (w) * 64 && blockIdx.x < STAMP_BLOCKS) {                                \
            unsigned long long t__;                                                                \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");            \
            g_stamps[blockIdx.x * STAMP_SLOTS + (k)] = t__;                                        \
        }                                                                                          \
    } while (0)
// the main-loop segment stamps (MOCA_STAMP_W) of the staggered kernels: which wave stamps, in which loop iteration (-DSEG_WAVE= / -DSEG_ITER=)
#ifndef SEG_WAVE
#define SEG_WAVE 0
#endif
#ifndef SEG_ITER
#define SEG_ITER 2
#endif
#define MOCA_STAMP_P(k, dep)                                                                       \
    do {                                                                                           \
        int dep__ = (dep);                                                                         \
        asm volatile("" : "+v"(dep__));                                                            \
        if (threadIdx.x == 0 && blockIdx.x < STAMP_BLOCKS) {                                       \
            unsigned long long t__;                                                                \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");            \
            g_stamps[blockIdx.x * STAMP_SLOTS + (k)] = t__ + (dep__ & 0);                          \
        }                                                                                          \
    } while (0)
#define MOCA_STAMP_HW()                                                                            \
    do {                                                                                           \
        if (threadIdx.x == 0 && blockIdx.x < STAMP_BLOCKS) {                                       \
            unsigned hw__, xcc__;                                                                  \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw__));                     \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc__));                   \
            g_stamps[blockIdx.x * STAMP_SLOTS + 6] = hw__;                                         \
            g_stamps[blockIdx.x * STAMP_SLOTS + 7] = xcc__;                                        \
        }                                                                                          \
    } while (0)
#else
#define MOCA_STAMP(k) do {} while (0)
#define MOCA_STAMP_P(k, dep) do {} while (0)
#define MOCA_STAMP_HW() do {} while (0)
#endif

// q = n / d, r = n % d for 0 <= n < 2^24 via one float multiply and a +-1 fix-up (rd = 1.0f / d);
// the row-descriptor set-up of a block does 8-12 of these and sits on its critical path
__device__ __forceinline__ void divmod24(int n, int d, float rd, int& q, int& r) {
    q = (int)((float)n * rd);
    r = n - q * d;
    if (r < 0) { r += d; --q; }
    else if (r >= d) { r -= d; ++q; }
}

// ---- A-operand gather for BUFFER-addressed LDS-DMA (buffer_load_dwordx4 ... offen lds) --------------------------------------
// Same sources as AGather's fast path, expressed as  descriptor base (SGPRs) + per-lane 32-bit byte offset (one VGPR per
// row slot, recomputed only when the tap changes) + a block-uniform scalar byte offset per k-tile.  The hot loop then has NO
// 64-bit per-lane pointer arithmetic (the flat-address form costs v_lshl_add_u64 / v_mov_b64 pairs per DMA instruction, which
// compete with the MFMAs for the SIMD's issue slots), and rows that must read zeros (conv halo, t-1/t+1 outside the clip, M
// tail) carry an offset >= 2^31 = num_records of the descriptor: the hardware range check then writes ZEROS into LDS
// (tools/micro/buflds.hip verifies both facts on gfx950: out-of-range lanes of an LDS-DMA store 0, soffset is range-checked).
// Requires every in-range byte offset < 2^31 (host-checked) and C % 64 == 0 resp. K % 64 == 0 (the FAST conditions).
constexpr unsigned OOB_OFF = 0x80000000u;
template <int AMODE, int NAP, int KS>
struct BGather {
    const moca_gemm_params& p;
    int lch;
    int64_t row_off[NAP];
    int row_y[NAP], row_x[NAP];
    bool row_ok[NAP];
    unsigned a_off[NAP];          // per-lane byte offset of row slot g for the current tap
    int tap = -1, tin = 0, tiles_per_tap;
    int kt_next, kt_last;         // even tile of the next pair to issue; last pair of this block's k range
    // The k range is walked tap-major (the packing order of W): all channels of tap 0, then tap 1, ...  A channel-major walk (the
    // nine taps of one 64-channel slice before the next slice, so that the taps hit L2) was measured in round 2: -8 % GEMM fabric
    // reads, +2-5 % on some convs in isolation, -0.4 % on the whole step (profiles/r02_ab_conv_channel_major.txt) -- removed.
    // MOCA_A_LINEAR2 (internal: MOCA_A_LINEAR with p.a2): the virtual torch.cat([a, a2], channels) -- two "taps" of k1 / KS and
    // (K - k1) / KS tiles; tap 0 walks the rows of a (row stride lda), tap 1 those of a2 (lda2).  The kernel switches the buffer
    // descriptor with the tap (`tap` is block-uniform); k1 % 64 == 0, so a k-tile pair never straddles the sources.
    __device__ __forceinline__ BGather(const moca_gemm_params& p_, int lch_, int kt_begin, int kt_last_pair)
        : p(p_), lch(lch_), tiles_per_tap(AMODE == MOCA_A_LINEAR ? (1 << 30) : (AMODE == MOCA_A_LINEAR2 ? p_.k1 / KS : p_.C / KS)),
          kt_next(kt_begin), kt_last(kt_last_pair) {}

    __device__ __forceinline__ void init_row(int g, int m) {
        row_ok[g] = m < p.M;
        const int mm = row_ok[g] ? m : 0;
        if (AMODE == MOCA_A_LINEAR) {
            row_off[g] = (int64_t)mm * p.lda;
            row_y[g] = row_x[g] = 0;
        } else if (AMODE == MOCA_A_LINEAR2) {
            row_off[g] = mm;
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

    __device__ __forceinline__ void set_tap(int t) {
        tap = t;
        if (AMODE == MOCA_A_LINEAR) {
#pragma unroll
            for (int g = 0; g < NAP; ++g) a_off[g] = row_ok[g] ? (unsigned)((row_off[g] + lch * 8) * 2) : OOB_OFF;
        } else if (AMODE == MOCA_A_LINEAR2) {
            const int ld = t ? p.lda2 : p.lda;
            if (t) tiles_per_tap = 1 << 30;                  // (the second source runs to the end of the k range)
#pragma unroll
            for (int g = 0; g < NAP; ++g) a_off[g] = row_ok[g] ? (unsigned)((row_off[g] * ld + lch * 8) * 2) : OOB_OFF;
        } else if (AMODE == MOCA_A_CONV3X3) {
            const int ky = p.up_phase ? t >> 1 : t / 3, kx = p.up_phase ? t & 1 : t - ky * 3;      // (up_phase: see AGather::set_tap)
            const int limH = p.up ? 2 * p.inH : p.inH, limW = p.up ? 2 * p.inW : p.inW;
#pragma unroll
            for (int g = 0; g < NAP; ++g) {
                int iy = row_y[g] + ky, ix = row_x[g] + kx;
                const bool ok = t < (p.up_phase ? 4 : 9) && row_ok[g] && iy >= 0 && iy < limH && ix >= 0 && ix < limW;
                if (p.up) { iy >>= 1; ix >>= 1; }
                a_off[g] = ok ? (unsigned)(((row_off[g] + (int64_t)iy * p.inW + ix) * p.C + lch * 8) * 2) : OOB_OFF;
            }
        } else {
#pragma unroll
            for (int g = 0; g < NAP; ++g) {
                const int tt = row_y[g] + t - 1;
                const bool ok = t < 3 && row_ok[g] && tt >= 0 && tt < p.T;
                a_off[g] = ok ? (unsigned)(((row_off[g] + (int64_t)(t - 1) * p.HW) * p.C + lch * 8) * 2) : OOB_OFF;
            }
        }
    }

    // position the stream on the pair whose even tile is kt (one integer division, prologue only)
    __device__ __forceinline__ void seek(int kt) {
        kt_next = kt;
        const int t = AMODE == MOCA_A_LINEAR2 ? (kt >= tiles_per_tap ? 1 : 0) : kt / tiles_per_tap;
        tin = kt - t * tiles_per_tap;
        set_tap(t);
    }
    // step to the following pair; past the end of the k range the last pair repeats (uniform DMA accounting)
    __device__ __forceinline__ void advance() {
        if (kt_next + 2 <= kt_last) {
            kt_next += 2;
            tin += 2;
            if (tin >= tiles_per_tap) { tin = 0; set_tap(tap + 1); }
        }
    }
    // block-uniform byte offsets of the pair's EVEN tile (the odd one is + KS*2 bytes)
    __device__ __forceinline__ unsigned a_soff() const { return (unsigned)(tin * KS * 2); }
    __device__ __forceinline__ unsigned w_soff() const { return (unsigned)(kt_next * KS * 2); }
};

// ---- epilogue stage 2 of the direct-to-LDS kernels: the fp16 tile staged in LDS (`rows` x `out_bn`, row pitch `pitch` bytes)
//      leaves as 16-byte coalesced stores; the time-embedding row add and the residual are added in fp32 on the way ----
// Output rows of a launch whose output is at least half the 256 MiB Infinity Cache leave with non-temporal stores: the consumer could
// re-read little of them from a cache anyway, and they stop evicting the operands the running blocks share.  Same box, alternating
// (threshold sweep 0 / 64 / 128 / 256 MiB / never): the B = 16 FIFO iteration 220.7 -> 218.2 ms at every threshold <= 256 MiB; the
// B = 2 step 61.85 UNet-steps/s with plain stores, 62.1-62.2 at 64-128 MiB (the 320-channel GEGLU / q|k|v outputs stream), 60.7 with
// `nt` on every output (the consumers of the small outputs find them in the Infinity Cache).
__device__ __forceinline__ bool out_streams(const moca_gemm_params& p) { return p.reserved4_ & 1; }   // (decided by moca_gemm_f16)
__device__ __forceinline__ void st_out8(half_t* ptr, const half8v v, bool nt) {
#if defined(__HIP_DEVICE_COMPILE__)
    // (an `nt` store in one arm of a branch is merged with the plain one and loses the hint: the streaming arm is an instruction of its own)
    if (nt) asm volatile("global_store_dwordx4 %0, %1, off nt" :: "v"(ptr), "v"(v) : "memory");
    else *reinterpret_cast<half8v*>(ptr) = v;
#endif
}

// The plain epilogue of the kernels that store from registers (gemm_persistent.hip): o = eight consecutive columns `col` .. of row m as
// fp32 tile values.  As the staged kernels: the tile value rounded to fp16 first, then + row add, + residual in fp32, one rounding out.
__device__ __forceinline__ void store8_rowadd_res(const moca_gemm_params& p, int m, int col, float (&o)[8], const half_t* __restrict__ rowadd,
                                                  const half_t* __restrict__ resid, bool nt_out) {
    if (m >= p.M) return;
    if (rowadd) {
        const half8v e = *reinterpret_cast<const half8v*>(rowadd + (int64_t)(m / p.rowadd_div) * p.ld_rowadd + col);
#pragma unroll
        for (int r = 0; r < 8; ++r) o[r] = (float)(half_t)o[r] + (float)e[r];
    }
    if (resid) {
        const half8v e = *reinterpret_cast<const half8v*>(resid + (int64_t)m * p.ldr + col);
#pragma unroll
        for (int r = 0; r < 8; ++r) o[r] = (rowadd ? o[r] : (float)(half_t)o[r]) + (float)e[r];
    }
    half8v h;
#pragma unroll
    for (int r = 0; r < 8; ++r) h[r] = (half_t)o[r];
    st_out8(reinterpret_cast<half_t*>(p.out) + (int64_t)m * p.ldo + col, h, nt_out);
}

// Residual rows of a launch whose output streams (>= 128 MiB: out_streams) are read with non-temporal loads: they are read once and,
// at that size, come from HBM -- same box, alternating (profiles/r05_ab_nt_loads.txt): the B = 16 `163840 x 640 x 640 +res` linears
// 218 -> 199 us, `655360 x 320 x 320 +res` -1 %; on the B = 2 tensors (served by the Infinity Cache) the hint costs 8 %, hence the size
// rule.  (Non-temporal LDS-DMA of an A operand that is read once measured 13 % slower.)
// (a compile-time choice: a hinted load in one arm of a runtime branch is merged with the plain one and loses the hint, as with stores;
//  the store loops are instantiated for both policies and chosen once per block)
template <bool NT>
__device__ __forceinline__ half8v ld_res8(const half_t* ptr) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const half8v*>(ptr));
    else return *reinterpret_cast<const half8v*>(ptr);
}

// Row-add / residual operands of the store loops are fetched several chunks AHEAD of the stores.  `out` may alias `residual`, so the
// compiler keeps every load behind the previous iteration's store, and each 16-byte chunk paid a global-load round trip plus the store
// drain (`s_waitcnt vmcnt(0)`).  With operands served by the Infinity Cache (B = 2 forward) that costs nothing measurable; from HBM
// (B = 16: the FIFO iteration, configs[4]) the +residual linears run 3.5-9 % faster with the operands in flight together
// (tools/bench_gemm.py "linear+res", BG_B=16).  A thread only ever reads the addresses it writes itself.
constexpr int EPI_U = 8;

template <int NTHREADS, bool NT>
__device__ __forceinline__ void store_fp16_tile_impl(const moca_gemm_params& p, const char* stage, int pitch, int rows, int out_bn,
                                                int m0, int on0, int tid) {
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);
    constexpr bool nt_out = NT;                        // (= out_streams(p), chosen by the wrapper below)
    const int chunks_per_row = out_bn / 8;
    const int total_chunks = rows * chunks_per_row;
    if (!rowadd && !resid) {
        // up_phase (a, b): GEMM row m = pixel (f, i, j) of the low-resolution grid is output pixel (f, 2i + a, 2j + b) of the upsampled
        // one: row 4 m - 2 (m mod W) + 2 W a + b
        const int upW = p.up_phase ? p.outW : 0, upC = p.up_phase ? 2 * p.outW * ((p.up_phase - 1) >> 1) + ((p.up_phase - 1) & 1) : 0;
        for (int idx = tid; idx < total_chunks; idx += NTHREADS) {
            const int row = idx / chunks_per_row, ch = idx - row * chunks_per_row;
            const int m = m0 + row;
            if (m >= p.M) continue;
            const int64_t mo = upW ? 4 * (int64_t)m - 2 * (m % upW) + upC : m;
            st_out8(reinterpret_cast<half_t*>(p.out) + mo * p.ldo + on0 + ch * 8, *reinterpret_cast<const half8v*>(stage + row * pitch + ch * 16), nt_out);
        }
        return;
    }
    const half8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int base = tid; base < total_chunks; base += EPI_U * NTHREADS) {
        half8v ea[EPI_U], er[EPI_U];
        int soff[EPI_U];
        int64_t ooff[EPI_U];
        bool ok[EPI_U];
#pragma unroll
        for (int u = 0; u < EPI_U; ++u) {
            const int idx = base + u * NTHREADS;
            const int row = idx / chunks_per_row, ch = idx - row * chunks_per_row;
            const int m = m0 + row, col = on0 + ch * 8;
            ok[u] = idx < total_chunks && m < p.M;
            soff[u] = row * pitch + ch * 16;
            ooff[u] = (int64_t)m * p.ldo + col;
            ea[u] = zero8; er[u] = zero8;
            if (ok[u]) {
                if (rowadd) ea[u] = *reinterpret_cast<const half8v*>(rowadd + (int64_t)(m / p.rowadd_div) * p.ld_rowadd + col);
                if (resid) er[u] = ld_res8<NT>(resid + (int64_t)m * p.ldr + col);
            }
        }
#pragma unroll
        for (int u = 0; u < EPI_U; ++u) {
            if (!ok[u]) continue;
            half8v h = *reinterpret_cast<const half8v*>(stage + soff[u]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {                     // (same order as ever: + row add, then + residual, in fp32)
                float v = (float)h[j];
                if (rowadd) v += (float)ea[u][j];
                if (resid) v += (float)er[u][j];
                h[j] = (half_t)v;
            }
            st_out8(reinterpret_cast<half_t*>(p.out) + ooff[u], h, nt_out);
        }
    }
}

template <int NTHREADS>
__device__ __forceinline__ void store_fp16_tile(const moca_gemm_params& p, const char* stage, int pitch, int rows, int out_bn,
                                                int m0, int on0, int tid) {
    if (out_streams(p)) store_fp16_tile_impl<NTHREADS, true>(p, stage, pitch, rows, out_bn, m0, on0, tid);
    else store_fp16_tile_impl<NTHREADS, false>(p, stage, pitch, rows, out_bn, m0, on0, tid);
}

// ---- store loop of the 320 x 160 kernels with GroupNorm statistics (MOCA_EP_COLSUM): as store_fp16_tile, but every thread
//      keeps a FIXED 16-byte column chunk (thread -> chunk tid % 20, rows tid / 20 + 25 i) so that it can accumulate the sum and
//      the sum of squares of its 8 columns in registers on the way out (fp32 values after row add / residual, i.e. what the
//      consumer's GroupNorm would read back, before the fp16 rounding); the 25 row subsets are then combined through LDS in a
//      fixed order (deterministic) and the block writes colsum[tile_m][n0 .. n0+160)[2].  `red` = 32 000 B of LDS scratch
//      behind the staged tile.
template <int ROWS, int BNC, bool NT>
__device__ __forceinline__ void store_fp16_tile_colsum_impl(const moca_gemm_params& p, const char* stage, float* red, int pitch,
                                                       int m0, int n0, int tile_m, int tid) {
    constexpr int CPR = BNC / 8, RS = 512 / CPR;          // 320 x 160: 20 chunks per row, 25 row subsets; 160 x 320: 40 and 12
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);
    constexpr bool nt_out = NT;                        // (= out_streams(p), chosen by the wrapper below)
    const int ch = tid % CPR, rs = tid / CPR;
    // (up_phase: rows scattered to the upsampled grid as in store_fp16_tile; a row tile of the low-resolution grid lies inside one frame)
    const int upW = p.up_phase ? p.outW : 0, upC = p.up_phase ? 2 * p.outW * ((p.up_phase - 1) >> 1) + ((p.up_phase - 1) & 1) : 0;
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[j] = 0.f; q[j] = 0.f; }
    if (rs < RS) {
        const int col = n0 + ch * 8;
        const half8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        constexpr int U = 4;                                       // operands fetched U rows ahead of the stores (see store_fp16_tile)
        for (int row0 = rs; row0 < ROWS && m0 + row0 < p.M; row0 += U * RS) {
            half8v ea[U], er[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int row = row0 + u * RS, m = m0 + row;
                ea[u] = zero8; er[u] = zero8;
                if (row < ROWS && m < p.M) {
                    if (rowadd) ea[u] = *reinterpret_cast<const half8v*>(rowadd + (int64_t)(m / p.rowadd_div) * p.ld_rowadd + col);
                    if (resid) er[u] = ld_res8<NT>(resid + (int64_t)m * p.ldr + col);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int row = row0 + u * RS, m = m0 + row;
                if (row >= ROWS || m >= p.M) break;
                const half8v h = *reinterpret_cast<const half8v*>(stage + row * pitch + ch * 16);
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    v[j] = (float)h[j];
                    if (rowadd) v[j] += (float)ea[u][j];
                    if (resid) v[j] += (float)er[u][j];
                }
                half8v o;
#pragma unroll
                for (int j = 0; j < 8; ++j) { o[j] = (half_t)v[j]; s[j] += v[j]; q[j] += v[j] * v[j]; }
                const int64_t mo = upW ? 4 * (int64_t)m - 2 * (m % upW) + upC : m;
                st_out8(reinterpret_cast<half_t*>(p.out) + mo * p.ldo + col, o, nt_out);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { red[(rs * BNC + ch * 8 + j) * 2] = s[j]; red[(rs * BNC + ch * 8 + j) * 2 + 1] = q[j]; }
    }
    __syncthreads();
    if (p.flags & MOCA_EP_GSTAT) {
        // finished statistics: column totals -> LDS, then one thread per (GroupNorm channel group touched by this tile, sum or sum
        // of squares) adds its columns and issues ONE fixed-point atomic on gstat[statistics group][channel group] (a row tile lies
        // inside one statistics group).  Sums of <= 320 x 40 values per atomic in fp32; the cross-tile accumulation is 64-bit fixed point (order independent, common.h).
        float a[2] = {0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = tid + h * 512;
            if (i < 2 * BNC) {
#pragma unroll 4
                for (int r = 0; r < RS; ++r) a[h] += red[r * BNC * 2 + i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = tid + h * 512;
            if (i < 2 * BNC) red[i] = a[h];
        }
        __syncthreads();
        // (gstat_cpg / gstat_coff: this output is one source of a virtual concat and its columns are channels coff + n of the consumer's
        //  tensor, whose groups are cpg wide -- a group at the seam is completed by the other source's producer)
        const int cpg = p.gstat_cpg > 0 ? p.gstat_cpg : p.N / 32, coff = p.gstat_coff;
        const int g0 = (coff + n0) / cpg, g1 = (coff + n0 + BNC - 1) / cpg;
        if (tid < 2 * (g1 - g0 + 1)) {
            const int g = g0 + (tid >> 1), comp = tid & 1;
            const int c0 = max(g * cpg - coff, n0) - n0, c1 = min((g + 1) * cpg - coff, n0 + BNC) - n0;
            float t = 0.f;
            for (int c = c0; c < c1; ++c) t += red[c * 2 + comp];
            const int sg = m0 / p.gstat_rows;
            moca_gstat_add(p.gstat + ((int64_t)sg * 32 + g) * 2 + comp, comp, t);
        }
        return;
    }
    for (int i = tid; i < 2 * BNC; i += 512) {
        float a = 0.f;
#pragma unroll 4
        for (int r = 0; r < RS; ++r) a += red[r * BNC * 2 + i];
        p.colsum[((int64_t)tile_m * p.N + n0) * 2 + i] = a;
    }
}

template <int ROWS, int BNC>
__device__ __forceinline__ void store_fp16_tile_colsum(const moca_gemm_params& p, const char* stage, float* red, int pitch,
                                                       int m0, int n0, int tile_m, int tid) {
    if (out_streams(p)) store_fp16_tile_colsum_impl<ROWS, BNC, true>(p, stage, red, pitch, m0, n0, tile_m, tid);
    else store_fp16_tile_colsum_impl<ROWS, BNC, false>(p, stage, red, pitch, m0, n0, tile_m, tid);
}

// ---- store loop of the 160 x 320 tile with LayerNorm (MOCA_EP_LN, N == 320: the block owns complete rows): 8 lanes per row,
//      lane l8 -> 16-byte chunks l8, l8 + 8, ..., l8 + 32 (40 columns), 64 rows per pass.  Adds the residual in fp32, stores
//      x = the linear's output (fp16) AND ln_out = LayerNorm(x) * gamma + beta (fp16; statistics of the fp32 values, variance
//      two-pass from registers, reduced over the 8 lanes of a row with shuffles).
template <int ROWS = 160>
__device__ __forceinline__ void store_fp16_tile_ln(const moca_gemm_params& p, const char* stage, float* gb, int pitch, int m0, int tid) {
    constexpr int NC = 320, CPL = 5;
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
    const bool nt_out = out_streams(p);
    const int l8 = tid & 7, rsub = tid >> 3;
    // gamma / beta go through LDS (`gb` = 2 x 320 floats behind the staged tile): 80 more live registers per thread would not
    // fit beside the row
    for (int i = tid; i < 2 * NC; i += 512) gb[i] = i < NC ? p.ln_gamma[i] : p.ln_beta[i - NC];
    __syncthreads();
    for (int row = rsub; row < ROWS; row += 64) {
        const int m = m0 + row;
        const bool ok = m < p.M;                         // (all 8 lanes of a row agree; the shuffles below need every lane)
        float v[CPL][8];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int col = (l8 + 8 * c) * 8;
            const half8v h = *reinterpret_cast<const half8v*>(stage + row * pitch + col * 2);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[c][j] = (float)h[j];
            if (rowadd && ok) {
                const half8v e = *reinterpret_cast<const half8v*>(rowadd + (int64_t)(m / p.rowadd_div) * p.ld_rowadd + col);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[c][j] += (float)e[j];
            }
            if (resid && ok) {
                const half8v e = *reinterpret_cast<const half8v*>(resid + (int64_t)m * p.ldr + col);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[c][j] += (float)e[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[c][j];
        }
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
        const float mean = s * (1.0f / NC);
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CPL; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = v[c][j] - mean; q += d * d; }
        q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64); q += __shfl_xor(q, 4, 64);
        const float rstd = rsqrtf(q * (1.0f / NC) + p.ln_eps);
        if (ok) {
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const int col = (l8 + 8 * c) * 8;
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(gb + col), g1 = *reinterpret_cast<const f32x4*>(gb + col + 4);
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(gb + NC + col), b1 = *reinterpret_cast<const f32x4*>(gb + NC + col + 4);
                half8v o, n;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o[j] = (half_t)v[c][j]; o[4 + j] = (half_t)v[c][4 + j];
                    n[j] = (half_t)((v[c][j] - mean) * rstd * g0[j] + b0[j]);
                    n[4 + j] = (half_t)((v[c][4 + j] - mean) * rstd * g1[j] + b1[j]);
                }
                st_out8(reinterpret_cast<half_t*>(p.out) + (int64_t)m * p.ldo + col, o, nt_out);
                *reinterpret_cast<half8v*>(reinterpret_cast<half_t*>(p.ln_out) + (int64_t)m * p.ld_ln + col) = n;
            }
        }
    }
}

// ---- store loop with LayerNorm statistics of the consumer (MOCA_EP_ROWSUM): as store_fp16_tile, but LPR lanes share a row
//      (lane l -> 16-byte chunks l, l + LPR, ...), so the sum and the sum of squares of the stored (fp16-rounded) values of a
//      row's BNC columns are reduced with shuffles and written to rowsum[column tile][m][2].  The consumer
//      (MOCA_EP_LNFOLD) combines the N / BNC partials of a row. ----
template <int NTHREADS, int BNC, int LPR, bool NT>
__device__ __forceinline__ void store_fp16_tile_rowsum_impl(const moca_gemm_params& p, const char* stage, int pitch, int rows,
                                                       int m0, int n0, int tid) {
    constexpr int CPL = BNC / 8 / LPR;
    static_assert(CPL * LPR * 8 == BNC, "column tile = LPR lanes x CPL chunks of 8");
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
    constexpr bool nt_out = NT;                        // (= out_streams(p), chosen by the wrapper below)
    const int l = tid % LPR, rsub = tid / LPR;
    float* dst = p.rowsum + (int64_t)(n0 / BNC) * p.M * 2;
    const half8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    constexpr int RSTEP = NTHREADS / LPR;
    half8v ea[CPL], er[CPL], na[CPL], nr[CPL];           // operands of this row pass / of the next one, fetched a pass ahead of the
    auto fetch = [&](int row, half8v* fa, half8v* fr) {  // stores (see store_fp16_tile)
        const int m = m0 + row;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int col = (l + LPR * c) * 8;
            fa[c] = zero8; fr[c] = zero8;
            if (row < rows && m < p.M) {
                if (rowadd) fa[c] = *reinterpret_cast<const half8v*>(rowadd + (int64_t)(m / p.rowadd_div) * p.ld_rowadd + n0 + col);
                if (resid) fr[c] = ld_res8<NT>(resid + (int64_t)m * p.ldr + n0 + col);
            }
        }
    };
    if (rowadd || resid) fetch(rsub, ea, er);
    for (int row = rsub; row < rows; row += RSTEP) {
        const int m = m0 + row;
        const bool ok = m < p.M;                         // (all lanes of a row agree; the shuffles below need every lane)
        float s = 0.f, q = 0.f;
        if (rowadd || resid) fetch(row + RSTEP, na, nr);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int col = (l + LPR * c) * 8;
            half8v h = *reinterpret_cast<const half8v*>(stage + row * pitch + col * 2);
            if ((rowadd || resid) && ok) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float v = (float)h[j];
                    if (rowadd) v += (float)ea[c][j];
                    if (resid) v += (float)er[c][j];
                    h[j] = (half_t)v;
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float a = (float)h[j]; s += a; q += a * a; }
            if (ok) st_out8(reinterpret_cast<half_t*>(p.out) + (int64_t)m * p.ldo + n0 + col, h, nt_out);
        }
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
        if (l == 0 && ok) *reinterpret_cast<float2*>(dst + (int64_t)m * 2) = float2{s, q};
#pragma unroll
        for (int c = 0; c < CPL; ++c) { ea[c] = na[c]; er[c] = nr[c]; }
    }
}

template <int NTHREADS, int BNC, int LPR>
__device__ __forceinline__ void store_fp16_tile_rowsum(const moca_gemm_params& p, const char* stage, int pitch, int rows,
                                                       int m0, int n0, int tid) {
    if (out_streams(p)) store_fp16_tile_rowsum_impl<NTHREADS, BNC, LPR, true>(p, stage, pitch, rows, m0, n0, tid);
    else store_fp16_tile_rowsum_impl<NTHREADS, BNC, LPR, false>(p, stage, pitch, rows, m0, n0, tid);
}

// ---- MOCA_EP_LNFOLD, step 1: thread t < TM owns the LayerNorm statistics of A row m0 + t, thread t < BN the wsum / bias of
//      column n0 + t.  lnfold_issue() goes BEFORE the prologue's DMA instructions (loads return in order: by the time the first
//      k-tiles have landed these have too, so their latency costs nothing; measured 7-14 us per launch when they were issued
//      behind the DMAs) and keeps the raw values of the first two row partials in registers; lnfold_finish() (after the
//      prologue DMAs are out) adds any further partials and turns the sums into (rstd, -mean * rstd).  Four registers are carried
//      through the main loop; lnfold_publish() puts them into LDS behind the staged tile for the accumulator -> fp16 staging
//      pass (rows past M repeat the last row; their stores are skipped anyway).
//      g4p / g4q (gemm_persistent.hip) run the same three steps per tile: `col` = n0 + their W-row permutation of tid,
//      `fold` = false for a launch without the flag, which yields (1, 0, 0, bias), and a publish without the barrier (they have their own). ----
struct LnFoldRegs { float rs, rb, ws, b; };
struct LnFoldRaw { float2 p0, p1; float ws, b; };
// the formula alone: sum and sum of squares of a row of K values -> (rstd, -mean * rstd)
__device__ __forceinline__ float2 lnfold_stats(float s, float q, int K, float eps) {
    const float inv_k = 1.0f / (float)K;
    const float mean = s * inv_k;
    const float var = fmaxf(q * inv_k - mean * mean, 0.f);
    const float rs = rsqrtf(var + eps);
    return float2{rs, -mean * rs};
}
// (`row` = the global A row of this thread's tile row: m0 + tid, or the gathered row of the temporal-attention tiling; `col` = the
//  packed W row whose wsum / bias this thread < BN owns: n0 + tid)
template <int TM, int BN>
__device__ __forceinline__ LnFoldRaw lnfold_issue(const moca_gemm_params& p, int row, int col, int tid, bool fold = true) {
    LnFoldRaw r = {float2{0.f, 0.f}, float2{0.f, 0.f}, 0.f, 0.f};
    if (tid < BN) {
        if (fold) r.ws = p.lnf_wsum[col];
        r.b = p.bias ? p.bias[col] : 0.f;
    }
    if (fold && tid < TM) {
        const int m = min(row, p.M - 1);
        r.p0 = *reinterpret_cast<const float2*>(p.lnf_part + (int64_t)m * 2);
        if (p.lnf_nparts > 1) r.p1 = *reinterpret_cast<const float2*>(p.lnf_part + ((int64_t)p.M + m) * 2);
    }
    return r;
}
template <int TM, int BN>
__device__ __forceinline__ LnFoldRegs lnfold_finish(const moca_gemm_params& p, const LnFoldRaw& raw, int row, int tid, bool fold = true) {
    LnFoldRegs r = {fold ? 0.f : 1.f, 0.f, raw.ws, raw.b};
    if (fold && tid < TM) {
        const int m = min(row, p.M - 1);
        float s = raw.p0.x + raw.p1.x, q = raw.p0.y + raw.p1.y;
        for (int i = 2; i < p.lnf_nparts; ++i) {
            const float2 v = *reinterpret_cast<const float2*>(p.lnf_part + ((int64_t)i * p.M + m) * 2);
            s += v.x; q += v.y;
        }
        const float2 st = lnfold_stats(s, q, p.K, p.ln_eps);
        r.rs = st.x;
        r.rb = st.y;
    }
    return r;
}
// lds: [TM] float2 (rstd, -mean * rstd), then [BN] wsum, then [BN] bias
template <int TM, int BN, bool SYNC = true>
__device__ __forceinline__ void lnfold_publish(const LnFoldRegs& r, float* lds, int tid) {
    if (tid < TM) *reinterpret_cast<float2*>(lds + 2 * tid) = float2{r.rs, r.rb};
    if (tid < BN) { lds[2 * TM + tid] = r.ws; lds[2 * TM + BN + tid] = r.b; }
    if constexpr (SYNC) __syncthreads();
}
// step 2, per accumulator tile: v = rstd * acc + (-mean * rstd) * wsum + bias
__device__ __forceinline__ f32x4 lnfold_apply(const f32x4 acc, const float2 st, const f32x4 ws, const f32x4 b) {
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = st.x * acc[j] + (st.y * ws[j] + b[j]);
    return r;
}
__device__ __forceinline__ f32x4 ld4_or_zero(const float* ptr, int i) {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return ptr ? *reinterpret_cast<const f32x4*>(ptr + i) : z;
}

typedef __attribute__((address_space(3))) char* lds_ptr;
typedef const __attribute__((address_space(1))) void* glb_ptr;

}  // namespace

#endif
