// Implicit-GEMM for the VideoCrafter2 3D-UNet on gfx950 (MI355X).
//
//   out[M][N] = epilogue( gather(A)[M][K] . W[N][K]^T )
//
// One kernel family covers every contraction on the denoising path: 3x3 conv2d
// (stride 1/2, optional fused nearest x2 upsample), the (3,1,1) temporal conv3d and
// all nn.Linear layers; the A operand is gathered on the fly from channels-last fp16
// activations ([frame][y][x][c]), so no im2col buffer and no layout shuffles exist.
//
// This file reads top to bottom as: the kernels that stay here, what a call is and where it goes (the dispatch: route_of(),
// route_info(), route_can(), prepare()), what it launches (launch_route()), the C entry points.  The other kernel families live in
// gemm_tiled.hip and gemm_persistent.hip; their host entries and what they share with the dispatch: gemm_launch.h; shared device
// helpers: gemm_device.h.
//
// The kernels (k-tiles of 64 everywhere; which one runs a call: route_of() below):
//  here
//   gemm_f16_kernel<BN, AMODE>      128 x BN (BN = 128 or 64), 4 waves (2 x 2) of 2 x (BN/64) v_mfma_f32_32x32x16_f16
//                                   accumulators.  A/B k-tiles are staged through registers (the gather needs zero fill) into
//                                   double-buffered LDS with 128-byte rows and an XOR swizzle on the 16-byte chunk index
//                                   (chunk ^ ((row>>1)&7)) so that the ds_read_b128 fragment reads are bank-conflict free.  The
//                                   epilogue goes through an fp32 LDS tile so that bias / time-embedding / residual are applied in
//                                   fp32 and the result leaves as full 16-byte coalesced stores.  Any M, fp32 output, plain GELU.
//   splitk_reduce_kernel, splitk_gn_kernel<CPT>  the split-K reduce, alone or with the GroupNorm that consumes it
//  gemm_tiled.hip
//   gemm_glds_kernel<BN, AMODE, FAST>  256 x BN (128 or 160), 8 waves, direct-to-LDS 3-slot ring; column / row statistics,
//                                   LayerNorm fold, fp32 output, split-K slabs (fp32 or fp16)
//   gemm_g4_kernel<AMODE, FAST>     256 x 128, 4 waves, two blocks per CU: one block's epilogue under the other's MFMAs
//   gemm_w80s_kernel<AMODE, SHAPE>  (gemm_w80s_kernel.inc) the staggered, buffer-addressed 8-wave kernel on 320 x 160, 160 x 320
//                                   (LayerNorm store loop), 256 x 256 and 320 x 192 (temporal attention in the epilogue, also
//                                   gemm_w80s_causal_kernel) tiles; two-source A, per-row-group weights, every statistics epilogue
//  gemm_persistent.hip
//   gemm_g4p_kernel / gemm_g4q_kernel<GEGLU>, gemm_sqp_kernel<GEGLU>  the persistent forms of g4 (either MFMA shape) and of the
//                                   256 x 256 staggered kernel: register epilogue, bias / LayerNorm fold / GEGLU / row add / residual
// (The weight-stationary kernel of the 320 -> 320 linears is gemm_ws.hip; it is dispatched from here.)
#include "gemm_launch.h"

namespace {

template <int BN, int AMODE>
__global__ __launch_bounds__(256, 2) void gemm_f16_kernel(const moca_gemm_params p) {
    constexpr int NT = BN / 64;          // 32-wide n tiles per wave
    constexpr int B_SLOTS = BN / 32;     // 16-B chunks of W per thread per k-tile
    constexpr int A_BYTES = BM * ROW_BYTES;
    constexpr int B_BYTES = BN * ROW_BYTES;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sA = smem;                  // [2][A_BYTES]
    char* sB = smem + 2 * A_BYTES;    // [2][B_BYTES]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_m = wave >> 1, wave_n = wave & 1;

    const int tiles_m = (p.M + BM - 1) / BM;
    const int tiles_n = p.N / BN;
    const int nblk = tiles_m * tiles_n * p.splits;
    int logical;
    remap_block<BN>(nblk, logical);
    const int split = logical % p.splits;
    const int tile = logical / p.splits;
    const int tile_m = tile / tiles_n, tile_n = tile % tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int nk_total = (p.K + BK - 1) / BK;      // (W rows are readable and zero beyond K up to the next multiple of 64)
    const int kts = (nk_total + p.splits - 1) / p.splits;
    const int kt_begin = split * kts;
    const int kt_end = min(kt_begin + kts, nk_total);

    // ---- per-thread staging coordinates --------------------------------------
    const int cc = tid & 7;     // 16-byte chunk column inside the k-tile
    const int r0 = tid >> 3;    // rows r0 + 32*i
    const int swz = (r0 >> 1) & 7;  // identical for all rows r0+32i

    const half_t* __restrict__ Aptr = reinterpret_cast<const half_t*>(p.a);
    const half_t* __restrict__ Wptr = reinterpret_cast<const half_t*>(p.w);

    // row descriptors
    int64_t row_off[4];   // LINEAR: m*lda ; CONV: frame pixel base ; TCONV: m
    int row_y[4], row_x[4];
    bool row_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + r0 + 32 * i;
        row_ok[i] = m < p.M;
        const int mm = row_ok[i] ? m : 0;
        if (AMODE == MOCA_A_LINEAR) {
            row_off[i] = (int64_t)mm * p.lda;
            row_y[i] = row_x[i] = 0;
        } else if (AMODE == MOCA_A_CONV3X3) {
            const int ohw = p.outH * p.outW;
            const int f = mm / ohw, rem = mm - f * ohw;
            const int oy = rem / p.outW, ox = rem - oy * p.outW;
            row_off[i] = (int64_t)f * p.inH * p.inW;
            row_y[i] = oy * p.stride - 1 + p.nopad_lo;
            row_x[i] = ox * p.stride - 1 + p.nopad_lo;
        } else {  // TCONV3
            const int frame = mm / p.HW;
            row_off[i] = mm;
            row_y[i] = frame % p.T;  // t
            row_x[i] = 0;
        }
    }

    half8v ra[4], rb[B_SLOTS];

    auto load_tile = [&](int kt) {
        const int k = kt * BK + cc * 8;
        // ---- A ----
        if (AMODE == MOCA_A_LINEAR) {
            const bool kok = k < p.K;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                half8v v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (kok && row_ok[i]) v = *reinterpret_cast<const half8v*>(Aptr + row_off[i] + k);
                ra[i] = v;
            }
        } else if (AMODE == MOCA_A_CONV3X3) {
            const int tap = k / p.C, c = k - tap * p.C;
            const int ky = tap / 3, kx = tap - ky * 3;
            const int limH = p.up ? 2 * p.inH : p.inH, limW = p.up ? 2 * p.inW : p.inW;
            const bool kok = tap < 9;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int iy = row_y[i] + ky, ix = row_x[i] + kx;
                const bool ok = kok && row_ok[i] && iy >= 0 && iy < limH && ix >= 0 && ix < limW;
                if (p.up) { iy >>= 1; ix >>= 1; }
                half8v v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (ok) v = *reinterpret_cast<const half8v*>(Aptr + (row_off[i] + (int64_t)iy * p.inW + ix) * p.C + c);
                ra[i] = v;
            }
        } else {
            const int tap = k / p.C, c = k - tap * p.C;
            const bool kok = tap < 3;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int tt = row_y[i] + tap - 1;
                const bool ok = kok && row_ok[i] && tt >= 0 && tt < p.T;
                half8v v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (ok) v = *reinterpret_cast<const half8v*>(Aptr + (row_off[i] + (int64_t)(tap - 1) * p.HW) * p.C + c);
                ra[i] = v;
            }
        }
        // ---- W (always in range: N % BN == 0, ldw % 64 == 0, zero padded) ----
#pragma unroll
        for (int i = 0; i < B_SLOTS; ++i) {
            const int n = n0 + r0 + 32 * i;
            rb[i] = *reinterpret_cast<const half8v*>(Wptr + (int64_t)n * p.ldw + k);
        }
    };

    auto store_tile = [&](int buf) {
        char* a = sA + buf * A_BYTES;
        char* b = sB + buf * B_BYTES;
        const int coff = (cc ^ swz) << 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<half8v*>(a + (r0 + 32 * i) * ROW_BYTES + coff) = ra[i];
#pragma unroll
        for (int i = 0; i < B_SLOTS; ++i)
            *reinterpret_cast<half8v*>(b + (r0 + 32 * i) * ROW_BYTES + coff) = rb[i];
    };

    f32x16 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    // fragment read coordinates
    const int frow = lane & 31, fh = lane >> 5;
    int a_row_b[2], a_swz[2], b_row_b[NT], b_swz[NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int row = wave_m * 64 + mt * 32 + frow;
        a_row_b[mt] = row * ROW_BYTES;
        a_swz[mt] = (row >> 1) & 7;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int row = wave_n * (BN / 2) + nt * 32 + frow;
        b_row_b[nt] = row * ROW_BYTES;
        b_swz[nt] = (row >> 1) & 7;
    }

    if (kt_begin < kt_end) {
        load_tile(kt_begin);
        store_tile(0);
    }
    __syncthreads();

    int cur = 0;
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const bool has_next = kt + 1 < kt_end;
        if (has_next) load_tile(kt + 1);

        const char* a = sA + cur * A_BYTES;
        const char* b = sB + cur * B_BYTES;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int ch = ks * 2 + fh;
            half8v af[2], bf[NT];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                af[mt] = *reinterpret_cast<const half8v*>(a + a_row_b[mt] + ((ch ^ a_swz[mt]) << 4));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                bf[nt] = *reinterpret_cast<const half8v*>(b + b_row_b[nt] + ((ch ^ b_swz[nt]) << 4));
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
        }
        if (has_next) store_tile(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // ---- split-K: raw fp32 partials, epilogue runs in splitk_reduce_kernel ----
    if (p.splits > 1) {
        float* ws = p.splitk_ws + (int64_t)split * p.M * p.N;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wave_m * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                    const int col = n0 + wave_n * (BN / 2) + nt * 32 + frow;
                    if (row < p.M) ws[(int64_t)row * p.N + col] = acc[mt][nt][r];
                }
        return;
    }

    // ---- epilogue stage 1: registers -> fp32 LDS tile (bias, GEGLU) ----
    // (the main loop's last __syncthreads() makes the pipeline buffers reusable)
    float* sC = reinterpret_cast<float*>(smem);
    const bool geglu = (p.flags & MOCA_EP_GEGLU) != 0;
    const int out_bn = geglu ? BN / 2 : BN;  // output columns of this tile
    if (geglu) {
        if constexpr (NT == 2) {
            const int ncol = n0 + wave_n * 64 + frow;
            const float bv = p.bias ? p.bias[ncol] : 0.f;
            const float bg = p.bias ? p.bias[ncol + 32] : 0.f;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wave_m * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                    const float v = acc[mt][0][r] + bv;
                    const float g = acc[mt][1][r] + bg;
                    sC[row * out_bn + wave_n * 32 + frow] = v * moca_gelu(g);
                }
        }
    } else {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = wave_n * (BN / 2) + nt * 32 + frow;
            const float bv = p.bias ? p.bias[n0 + col] : 0.f;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wave_m * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                    const float v = acc[mt][nt][r] + bv;
                    sC[row * out_bn + col] = (p.flags & MOCA_EP_GELU) ? moca_gelu(v) : v;
                }
        }
    }
    __syncthreads();

    // ---- epilogue stage 2: coalesced 16-byte rows (+rowadd, +residual) ----
    const int chunks_per_row = out_bn / 8;
    const int total_chunks = BM * chunks_per_row;
    const int on0 = geglu ? n0 / 2 : n0;
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);
    for (int idx = tid; idx < total_chunks; idx += 256) {
        const int row = idx / chunks_per_row, ch = idx - row * chunks_per_row;
        const int m = m0 + row;
        if (m >= p.M) continue;
        const int col = on0 + ch * 8;
        float v[8];
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(sC + row * out_bn + ch * 8);
        const f32x4 c1 = *reinterpret_cast<const f32x4*>(sC + row * out_bn + ch * 8 + 4);
        v[0] = c0[0]; v[1] = c0[1]; v[2] = c0[2]; v[3] = c0[3];
        v[4] = c1[0]; v[5] = c1[1]; v[6] = c1[2]; v[7] = c1[3];
        if (rowadd) {
            const half8v e = *reinterpret_cast<const half8v*>(rowadd + (int64_t)(m / p.rowadd_div) * p.ld_rowadd + col);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += (float)e[j];
        }
        if (resid) {
            const half8v e = *reinterpret_cast<const half8v*>(resid + (int64_t)m * p.ldr + col);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += (float)e[j];
        }
        if (p.flags & MOCA_EP_OUT_F32) {
            float* o = reinterpret_cast<float*>(p.out) + (int64_t)m * p.ldo + col;
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
            half8v h;
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = (half_t)v[j];
            *reinterpret_cast<half8v*>(reinterpret_cast<half_t*>(p.out) + (int64_t)m * p.ldo + col) = h;
        }
    }
}

// Sum the split-K partial slabs and run the same epilogue.  One thread per 8 output
// columns; HBM-bound (reads splits*M*N*4 bytes).
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const moca_gemm_params p) {
    const bool geglu = (p.flags & MOCA_EP_GEGLU) != 0;
    const int out_n = geglu ? p.N / 2 : p.N;
    const int cpr = out_n / 8;
    const int64_t total = (int64_t)p.M * cpr;
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int m = (int)(idx / cpr), ch = (int)(idx - (int64_t)m * cpr);
        const int col = ch * 8;
        float v[8];
        if (geglu) {
            // output col j <- value col (j/32)*64 + j%32, gate = value + 32; 8 | 32 so a chunk never straddles
            const int vc = (col / 32) * 64 + (col % 32);
            float a[8], g[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { a[j] = p.bias ? p.bias[vc + j] : 0.f; g[j] = p.bias ? p.bias[vc + 32 + j] : 0.f; }
            for (int s = 0; s < p.splits; ++s) {
                const float* w = p.splitk_ws + ((int64_t)s * p.M + m) * p.N + vc;
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(w), a1 = *reinterpret_cast<const f32x4*>(w + 4);
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(w + 32), g1 = *reinterpret_cast<const f32x4*>(w + 36);
#pragma unroll
                for (int j = 0; j < 4; ++j) { a[j] += a0[j]; a[4 + j] += a1[j]; g[j] += g0[j]; g[4 + j] += g1[j]; }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = a[j] * moca_gelu(g[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = p.bias ? p.bias[col + j] : 0.f;
            if (p.reserved4_ & 4) {                               // fp16 slabs (MOCA_TUNE_SLAB_F16)
                for (int s = 0; s < p.splits; ++s) {
                    const half8v a = *reinterpret_cast<const half8v*>(reinterpret_cast<const half_t*>(p.splitk_ws) + ((int64_t)s * p.M + m) * p.N + col);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] += (float)a[j];
                }
            } else {
                for (int s = 0; s < p.splits; ++s) {
                    const float* w = p.splitk_ws + ((int64_t)s * p.M + m) * p.N + col;
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(w), a1 = *reinterpret_cast<const f32x4*>(w + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[j] += a0[j]; v[4 + j] += a1[j]; }
                }
            }
        }
        if (rowadd) {
            const half8v e = *reinterpret_cast<const half8v*>(rowadd + (int64_t)(m / p.rowadd_div) * p.ld_rowadd + col);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += (float)e[j];
        }
        if (resid) {
            const half8v e = *reinterpret_cast<const half8v*>(resid + (int64_t)m * p.ldr + col);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += (float)e[j];
        }
        if (p.flags & MOCA_EP_OUT_F32) {
            float* o = reinterpret_cast<float*>(p.out) + (int64_t)m * p.ldo + col;
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
            half8v h;
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = (half_t)v[j];
            *reinterpret_cast<half8v*>(reinterpret_cast<half_t*>(p.out) + (int64_t)m * p.ldo + col) = h;
        }
    }
}

// ---- split-K reduce + the GroupNorm(+SiLU) that consumes the result, in ONE launch (moca_gemm_splitk_groupnorm_f16): at the
// 5 x 8-latent level (M = 1280 at B = 2: 50 tiles per launch, every conv / temporal conv runs split-K) a ResBlock is a chain of
// GEMM -> reduce -> GroupNorm launches of 5-9 us each on tensors of 3 MB.  One block per (statistics group, channel group) slab, as
// gn_slab_reg_kernel: a thread sums the split-K slabs of its <= CPT 16-byte output chunks (+ bias / row add / residual: the epilogue of
// splitk_reduce_kernel, same order), rounds them to fp16 -- the value the two-launch path stores and normalises --, optionally
// writes them (write_x: the residual of a later launch), the block reduces sum / sum of squares and normalises from registers.
template <int CPT>
__global__ __launch_bounds__(1024) void splitk_gn_kernel(const moca_gemm_params p, half_t* __restrict__ y, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int R, int cpg, double inv_count, float eps,
                                                         int silu, int write_x) {
    __shared__ float s_red[2][16];
    __shared__ float s_sc[128], s_sh[128];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int slab = blockIdx.x, sg = slab / 32, g = slab % 32;
    const int vpr = cpg / 8, nchunks = R * vpr;
    const int N = p.N;
    const half_t* __restrict__ rowadd = reinterpret_cast<const half_t*>(p.rowadd);
    const half_t* __restrict__ resid = reinterpret_cast<const half_t*>(p.residual);
    const float gm_t = tid < cpg ? gamma[g * cpg + tid] : 0.f, bt_t = tid < cpg ? beta[g * cpg + tid] : 0.f;   // (in flight under the slab loads)
    half8v v[CPT];
    int mrow[CPT], ccol[CPT];
    float s = 0.f, q = 0.f;
    // (chunk by chunk, split by split.  Prefetching the next split's loads of all CPT chunks -- two register sets -- measured SLOWER, 23.1 against
    //  18.6 us on the 16-frame slabs: what bounds a block is not the dependent round trips but 160-byte row segments of the fp32 slabs at a
    //  5 KiB stride on the 64 CUs the 64 slabs occupy; profiles/r05_ab_splitk_groupnorm.txt)
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int idx = tid + i * nthr;
        mrow[i] = -1;
        if (idx < nchunks) {
            const int row = idx / vpr, c = idx - row * vpr;
            const int m = sg * R + row, col = g * cpg + c * 8;
            mrow[i] = m; ccol[i] = col;
            float a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = p.bias ? p.bias[col + j] : 0.f;
            if (p.reserved4_ & 4) {                               // fp16 slabs (MOCA_TUNE_SLAB_F16)
                for (int sp = 0; sp < p.splits; ++sp) {
                    const half8v h = *reinterpret_cast<const half8v*>(reinterpret_cast<const half_t*>(p.splitk_ws) + ((int64_t)sp * p.M + m) * N + col);
#pragma unroll
                    for (int j = 0; j < 8; ++j) a[j] += (float)h[j];
                }
            } else {
                for (int sp = 0; sp < p.splits; ++sp) {
                    const float* w = p.splitk_ws + ((int64_t)sp * p.M + m) * N + col;
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(w), a1 = *reinterpret_cast<const f32x4*>(w + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { a[j] += a0[j]; a[4 + j] += a1[j]; }
                }
            }
            if (rowadd) {
                const half8v e = *reinterpret_cast<const half8v*>(rowadd + (int64_t)(m / p.rowadd_div) * p.ld_rowadd + col);
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] += (float)e[j];
            }
            if (resid) {
                const half8v e = *reinterpret_cast<const half8v*>(resid + (int64_t)m * p.ldr + col);
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] += (float)e[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) v[i][j] = (half_t)a[j];
            if (write_x) *reinterpret_cast<half8v*>(reinterpret_cast<half_t*>(p.out) + (int64_t)m * p.ldo + col) = v[i];
        }
    }
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (mrow[i] >= 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float a = (float)v[i][j]; s += a; q += a * a; }
        }
    s = wave_sum(s); q = wave_sum(q);
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = s; s_red[1][tid >> 6] = q; }
    __syncthreads();
    if (tid < cpg) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < (nthr >> 6); ++w) { a += (double)s_red[0][w]; b += (double)s_red[1][w]; }
        const double mean = a * inv_count;
        double var = b * inv_count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        const float sc = rstd * gm_t;
        s_sc[tid] = sc;
        s_sh[tid] = bt_t - (float)mean * sc;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (mrow[i] >= 0) {
            const int c0 = ccol[i] - g * cpg;
            half8v r;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float a = (float)v[i][j] * s_sc[c0 + j] + s_sh[c0 + j];
                if (silu) a = moca_silu(a);
                r[j] = (half_t)a;
            }
            *reinterpret_cast<half8v*>(y + (int64_t)mrow[i] * N + ccol[i]) = r;
        }
}

template <int BN, int AMODE>
int launch_gemm(const moca_gemm_params& p, hipStream_t st) {
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = p.N / BN;
    const int nblk = tiles_m * tiles_n * p.splits;
    constexpr int lds_pipe = 2 * (BM + BN) * ROW_BYTES;
    constexpr int lds_epi = BM * BN * 4;
    constexpr int lds = lds_pipe > lds_epi ? lds_pipe : lds_epi;
    if (!dyn_lds_once<&gemm_f16_kernel<BN, AMODE>>(lds)) return MOCA_E_LAUNCH;
    hipLaunchKernelGGL((gemm_f16_kernel<BN, AMODE>), dim3(nblk), dim3(256), lds, st, p);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}
int launch_gemm_small(int bn, const moca_gemm_params& p, hipStream_t st) {
    if (bn == 128) return with_gather(p, [&](auto am, auto) { return launch_gemm<128, decltype(am)::value>(p, st); });
    return with_gather(p, [&](auto am, auto) { return launch_gemm<64, decltype(am)::value>(p, st); });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Dispatch.  Which kernel runs a call is decided by route_of() and nowhere else; what that kernel implements is written down in
// route_info() / route_can() and nowhere else.  moca_gemm_f16, moca_gemm_route and every query (moca_gemm_colsum_rows, _rowsum_cols,
// _ln_ok, _lnfold_ok, _tattn_ok, _wgroup_ok, _cat_ok, _splitk_groupnorm_ok) ask these two: a query that says yes is a launch that is
// accepted, on the kernel the query answered for.
enum Route : int {
    R_NONE = 0,                                       // refused
    R_SMALL64 = MOCA_ROUTE_SMALL64, R_SMALL128 = MOCA_ROUTE_SMALL128, R_GLDS128 = MOCA_ROUTE_GLDS128, R_GLDS160 = MOCA_ROUTE_GLDS160,
    R_G4 = MOCA_ROUTE_G4, R_W80 = MOCA_ROUTE_W80, R_W80W = MOCA_ROUTE_W80W, R_SQ256 = MOCA_ROUTE_SQ256, R_G4P = MOCA_ROUTE_G4P,
    R_SQP = MOCA_ROUTE_SQP, R_TATTN = MOCA_ROUTE_TATTN, R_WS = MOCA_ROUTE_WS, R_W80H = MOCA_ROUTE_W80H,
};

void normalise_splits(moca_gemm_params& p) {
    if (p.splits < 1) p.splits = 1;
    if (p.splits > (p.K + BK - 1) / BK) p.splits = (p.K + BK - 1) / BK;
    if (p.splits > 1) {   // no empty k range: every split writes its slab
        const int nkt = (p.K + BK - 1) / BK, kts = (nkt + p.splits - 1) / p.splits;
        p.splits = (nkt + kts - 1) / kts;
    }
}

// bytes spanned by the A operand / the W operand: the buffer-addressed kernels need every in-range offset below 2^31
inline int64_t a_span_bytes(const moca_gemm_params& p) {
    if (p.a_mode == MOCA_A_LINEAR) return ((int64_t)p.M * p.lda + 64) * 2;
    if (p.a_mode == MOCA_A_CONV3X3) return ((int64_t)(p.M / (p.outH * p.outW)) * p.inH * p.inW * p.C + 64) * 2;
    return ((int64_t)p.M * p.C + 64) * 2;
}
inline bool buffer_addressable(const moca_gemm_params& p) {
    if (p.a2 && ((int64_t)p.M * p.lda2 + 64) * 2 >= (1ll << 31)) return false;
    return a_span_bytes(p) < (1ll << 31) && (int64_t)p.N * p.ldw * 2 < (1ll << 31);
}

// which calls the persistent kernels can run: linears whose tiles (256 x 128: two blocks on every CU; 256 x 256: one) give every
// block at least one; bias, LayerNorm fold, GEGLU or row add / residual -- none of the statistics epilogues
bool persistent_ok(const moca_gemm_params& p, int BN, int blocks) {
    if (p.a_mode != MOCA_A_LINEAR || p.splits != 1 || p.N % BN || p.K % 64 || !buffer_addressable(p)) return false;
    if (p.flags & ~(MOCA_EP_GEGLU | MOCA_EP_LNFOLD)) return false;
    if ((p.flags & MOCA_EP_GEGLU) && (p.residual || p.rowadd)) return false;
    return ((p.M + 255) / 256) * (p.N / BN) >= blocks;
}

// which calls the halo form of the 320 x 160 staggered kernel (gemm_halo.hip) can run: stride-1 3 x 3 convs whose 320-row tiles are
// whole image rows of one frame, image rows of 64 or 32 pixels (the row pitch is a compile-time immediate of its fragment reads),
// 32-channel slices, no split-K (a second A source and per-row-group weights exist for linears only).
bool halo_ok(const moca_gemm_params& p) {
    if (p.a_mode != MOCA_A_CONV3X3 || p.stride != 1 || p.up || p.up_phase || p.nopad_lo || p.splits != 1 || p.a2 || p.wgroup_rows) return false;
    if ((p.inW != 64 && p.inW != 32) || p.inH % (320 / p.inW) || p.C % 32 || p.C > 8192) return false;
    return !(p.flags & ~(MOCA_EP_COLSUM | MOCA_EP_GSTAT | MOCA_EP_ROWSUM));
}

// The kernel family a (validated, split-normalised) call WITH ITS FLAGS runs on.  The only reader of the MOCA_TUNE_GEMM_* kernel-choice
// knobs and the only place that knows the order.  (MOCA_TUNE_GEMM_MF32 and MOCA_TUNE_SQP_WALK pick a variant inside a launcher.)
Route route_of(const moca_gemm_params& p) {
    // MOCA_EP_TATTN: the q|k|v projection of a temporal self-attention with the attention finished in the epilogue (SHAPE 3 of the
    // staggered kernel: 320 x 192 tiles, rows = 16 frames x 20 pixels, columns = one head)
    if (p.flags & MOCA_EP_TATTN) return R_TATTN;
    // the weight-stationary streaming kernel of the 320 -> 320 linears (gemm_ws.hip; MOCA_TUNE_GEMM_WS = 0: never).  Asked before every
    // tiled kernel: a call it takes runs on none of them.  (The kernel has no column sums, no LayerNorm fold, no LayerNorm store: a call
    // with one of those flags is not its call, moca_gemm_ws_ok.)
    // 1: where it was measured ahead of the tiled kernel (profiles/r06_ab_gemm_ws.txt): with a residual at every size, without one from
    // M = 2^17 up (B = 16 forwards; at M = 81920 a block's 10 strips do not amortise its start-up: W fetch + first strip).  2: wherever it applies
    const int ws_mode = moca_tuning_get(MOCA_TUNE_GEMM_WS);
    if (ws_mode && moca_gemm_ws_ok(p) && (ws_mode == 2 || p.residual || p.M >= (1 << 17))) return R_WS;
    // the persistent kernels (MOCA_TUNE_GEMM_SQP / _G4P = 0: never, 1: the GEGLU projections, 2: every linear they can run -- tests, A/B),
    // 256 x 256 before 256 x 128.  Neither reads a second A source or per-row-group weights: such a call goes on to the staggered kernels.
    if (!p.a2 && p.wgroup_rows <= 0) {
        const int sqp_mode = moca_tuning_get(MOCA_TUNE_GEMM_SQP), g4p_mode = moca_tuning_get(MOCA_TUNE_GEMM_G4P);
        if (sqp_mode && persistent_ok(p, 256, SQP_BLOCKS) && (sqp_mode == 2 || (p.flags & MOCA_EP_GEGLU))) return R_SQP;
        if (g4p_mode && persistent_ok(p, 128, G4P_BLOCKS) && (g4p_mode == 2 || (p.flags & MOCA_EP_GEGLU))) return R_G4P;
    }
    // w80 (320 x 160 tiles, 80 x 80 wave tiles, staggered and buffer-addressed): every non-GEGLU contraction whose N is a multiple of
    // 160 and whose 320-row tiles fill the chip.  (MOCA_TUNE_GEMM_W80: 0 never, 2 drops the tile-count rule -- tests.)
    const int w80_mode = moca_tuning_get(MOCA_TUNE_GEMM_W80);
    const int tiles320 = ((p.M + 319) / 320) * (p.N / 160);
    // MOCA_TUNE_CONV_HALO = 1: the convs halo_ok() names run on the halo form of that kernel (which also takes C % 64 == 32)
    const bool halo = moca_tuning_get(MOCA_TUNE_CONV_HALO) && halo_ok(p);
    if (w80_mode && p.N % 160 == 0 && !(p.flags & (MOCA_EP_GEGLU | MOCA_EP_OUT_F32 | MOCA_FORCE_SMALL_TILE)) && p.M > 160 &&
        (tiles320 * p.splits >= 200 || w80_mode == 2) && (fast_gather(p) || halo) && buffer_addressable(p)) {
        if (halo) return R_W80H;
        // which form of the staggered kernel.  The 160 x 320 tiling is required by the LayerNorm store loop and taken by every
        // N % 320 == 0 contraction: A is fetched once per 320 columns instead of once per 160 (linears: 37 vs 38 us at M = 81920,
        // N = K = 320; 99 vs 103 at K = 1280; 182 vs 193 / 366 vs 384 at M = 327680; N = 640: 22.7 vs 25.1).
        // Convs / temporal convs gain nothing from it (+-1 %, A/B on one device) and stay on the 320 x 160 form.
        // MOCA_TUNE_GEMM_WIDE = 0: only with MOCA_EP_LN; 1 (default): linears; 2: convs / temporal convs too (tests)
        if (p.flags & MOCA_EP_LN) return R_W80W;
        const int wide_mode = moca_tuning_get(MOCA_TUNE_GEMM_WIDE);
        if (wide_mode == 0 || p.N % 320) return R_W80;
        return (p.a_mode == MOCA_A_LINEAR || wide_mode == 2) ? R_W80W : R_W80;
    }
    // g4 (4 waves, two blocks per CU) wins where the epilogue is VALU-heavy and K is short (GEGLU at C = 320 / 640:
    // one block's erf-GELU epilogue runs under the other block's MFMAs, -5 % on the same device); the 8-wave kernel's
    // deeper pipeline wins everywhere else (K >= 1280: 1137 vs 880 TFLOP/s).  So: the GEGLU projections with K <= 640 -- but not the
    // very tall ones (M >= 2^17: B = 16 forwards), where the 256 x 256 staggered kernel is 4-5 % ahead (tools/bench_gemm.py geglu,
    // BG_B=16 BG_TUNE=2:2).  MOCA_TUNE_GEMM_G4 = 0 / 2 forces never / always (tests).
    const int g4_mode = moca_tuning_get(MOCA_TUNE_GEMM_G4);
    const bool use_g4 = !(p.flags & MOCA_EP_OUT_F32) &&
                        (g4_mode == 2 || (g4_mode == 1 && (p.flags & MOCA_EP_GEGLU) && p.K <= 640 && p.M < (1 << 17)));
    // the staggered kernel on 256 x 256 tiles for the wide projections (MOCA_TUNE_GEMM_SQ256 = 0: never, 1: not where g4 is preferred,
    // 2: every wide linear -- A/B runs)
    const int sq256_mode = moca_tuning_get(MOCA_TUNE_GEMM_SQ256);
    if (sq256_mode && p.a_mode == MOCA_A_LINEAR && p.N % 256 == 0 && p.N >= 2560 && p.M >= 512 && fast_gather(p) && buffer_addressable(p) &&
        !(p.flags & (MOCA_EP_OUT_F32 | MOCA_FORCE_SMALL_TILE)) && ((p.M + 255) / 256) * (p.N / 256) * p.splits >= 200 &&
        (sq256_mode == 2 || !use_g4)) return R_SQ256;
    // large-tile direct-to-LDS kernel whenever a 256-row tile is at least half full
    const int big_bn = (p.N % 128 == 0) ? 128 : (p.N % 160 == 0 ? 160 : 0);
    if (big_bn != 0 && p.M > 128 && !(p.flags & MOCA_FORCE_SMALL_TILE)) {
        if (big_bn == 128) return use_g4 ? R_G4 : R_GLDS128;
        return R_GLDS160;
    }
    return p.N % 128 == 0 ? R_SMALL128 : R_SMALL64;
}

// What a route's kernel implements: its tile (rows x columns; the weight-stationary kernel: rows per strip x columns per wave) and the
// MOCA_EP_* epilogues it has, with the four things that are not flags as bits above them.  MOCA_FORCE_SMALL_TILE asks for a route and
// MOCA_EP_SLABS is split-K without the reduce launch: neither is an epilogue of its own.
constexpr int CAN_SPLITK = 1 << 16, CAN_A2 = 1 << 17, CAN_WGROUP = 1 << 18, CAN_UP_PHASE = 1 << 19;
constexpr int EP_STATS = MOCA_EP_COLSUM | MOCA_EP_GSTAT;          // (GSTAT: the same sums, finished; same kernels)
struct RouteInfo { int tm, tn, can; };
RouteInfo route_info(Route r) {
    constexpr int GLDS = MOCA_EP_GEGLU | MOCA_EP_OUT_F32 | EP_STATS | MOCA_EP_ROWSUM | MOCA_EP_LNFOLD | CAN_SPLITK | CAN_UP_PHASE;
    constexpr int W80 = EP_STATS | MOCA_EP_ROWSUM | MOCA_EP_LNFOLD | CAN_SPLITK | CAN_UP_PHASE | CAN_A2 | CAN_WGROUP;
    switch (r) {
        // the plain-GELU epilogue (CLIP text MLP) exists in the 128-row kernel only
        case R_SMALL64: return {BM, 64, MOCA_EP_OUT_F32 | MOCA_EP_GELU | CAN_SPLITK};
        case R_SMALL128: return {BM, 128, MOCA_EP_GEGLU | MOCA_EP_OUT_F32 | MOCA_EP_GELU | CAN_SPLITK};
        case R_GLDS128: return {256, 128, GLDS};
        case R_GLDS160: return {256, 160, GLDS};
        case R_G4: return {256, 128, MOCA_EP_GEGLU | MOCA_EP_LNFOLD | CAN_SPLITK | CAN_UP_PHASE};
        case R_W80: return {320, 160, W80};
        case R_W80H: return {320, 160, EP_STATS | MOCA_EP_ROWSUM};  // halo_ok(): no split-K, one source, no row groups
        case R_W80W: return {160, 320, W80 | MOCA_EP_LN};           // a block owns whole rows of N = 320: the LayerNorm store loop
        case R_SQ256: return {256, 256, MOCA_EP_GEGLU | MOCA_EP_LNFOLD | CAN_SPLITK};
        case R_G4P: return {256, 128, MOCA_EP_GEGLU | MOCA_EP_LNFOLD};
        case R_SQP: return {256, 256, MOCA_EP_GEGLU | MOCA_EP_LNFOLD};
        case R_TATTN: return {320, 192, MOCA_EP_TATTN | MOCA_EP_LNFOLD};
        // finished statistics only (strips of 32 rows), one row partial per wave of 80 columns; deals its strips by weight group
        case R_WS: return {32, 80, MOCA_EP_ROWSUM | MOCA_EP_GSTAT | CAN_WGROUP};
        case R_NONE: break;
    }
    return {0, 0, 0};
}

// Can route r's kernel run this (validated, split-normalised) call: everything it asks for is implemented there, under the side
// conditions each feature has.  Pointers are the launch's business (prepare), not a capability.
bool route_can(Route r, const moca_gemm_params& p) {
    const RouteInfo ri = route_info(r);
    const int f = p.flags & ~(MOCA_FORCE_SMALL_TILE | MOCA_EP_SLABS);
    const int wants = f | (p.splits > 1 ? CAN_SPLITK : 0) | (p.a2 ? CAN_A2 : 0) | (p.wgroup_rows ? CAN_WGROUP : 0) | (p.up_phase ? CAN_UP_PHASE : 0);
    if (r == R_NONE || (wants & ~ri.can) || p.wgroup_rows < 0) return false;
    if (r == R_WS) return true;                       // moca_gemm_ws_ok, asked by route_of, is that kernel's whole precondition
    const bool linear1 = p.a_mode == MOCA_A_LINEAR && p.splits == 1;
    if (r == R_TATTN) {
        if (!linear1 || !fast_gather(p) || !buffer_addressable(p) || p.residual || p.rowadd || (p.flags & MOCA_FORCE_SMALL_TILE)) return false;
        if (p.N % 192 || p.T != 16 || p.HW <= 0 || p.HW % 20 || p.M % (16 * p.HW)) return false;
        if (p.ldo % 4 || p.ldo < p.N / 3) return false;
        // tattn_causal: 0 or 1; the mask is applied to the raw scores, so the scale must keep -inf at -inf
        return p.tattn_causal == 0 || (p.tattn_causal == 1 && p.tattn_scale > 0.f);
    }
    // column sums / GroupNorm statistics: fp16 output, no GEGLU, no split-k
    if ((f & EP_STATS) && (p.splits != 1 || (f & (MOCA_EP_GEGLU | MOCA_EP_OUT_F32)))) return false;
    // row sums: of a plain fp16 epilogue only
    if ((f & MOCA_EP_ROWSUM) && (p.splits != 1 || (f & (MOCA_EP_GEGLU | MOCA_EP_OUT_F32 | EP_STATS | MOCA_EP_LN | MOCA_EP_GELU)))) return false;
    // the LayerNorm store loop: a linear whose 320 columns one block owns, no column statistics beside it
    if ((f & MOCA_EP_LN) && !(linear1 && p.N == 320 && !(f & EP_STATS))) return false;
    // the LayerNorm fold: a linear with nothing else but GEGLU in the epilogue; the 256-row kernel has it in its plain epilogue only
    if ((f & MOCA_EP_LNFOLD) && !(linear1 && !(f & (MOCA_EP_OUT_F32 | EP_STATS | MOCA_EP_LN | MOCA_EP_ROWSUM | MOCA_EP_GELU)) &&
                                  !((r == R_GLDS128 || r == R_GLDS160) && (f & MOCA_EP_GEGLU)))) return false;
    if ((f & MOCA_EP_GELU) && (f & MOCA_EP_GEGLU)) return false;
    // two-source A (the virtual torch.cat in front of a ResBlock's skip_connection): a plain linear, sources split at a multiple of 64
    // columns, nothing but bias / residual / row add / row sums / GroupNorm statistics in the epilogue
    if (p.a2) {
        if (!linear1 || (f & ~(EP_STATS | MOCA_EP_ROWSUM))) return false;
        if (p.k1 <= 0 || p.k1 >= p.K || p.k1 % 64 || (p.K - p.k1) % 64 || p.lda % 8 || p.lda2 % 8 || p.lda < p.k1 || p.lda2 < p.K - p.k1) return false;
    }
    // per-row-group weights (wgroup_rows / wgroup_stride): a plain linear whose row tiles (160 rows on the 160 x 320 tiling, 320 on
    // 320 x 160) lie inside one group; bias / residual / row sums / LayerNorm store loop / column statistics
    if (p.wgroup_rows) {
        if (!linear1 || p.a2 || p.wgroup_stride < p.N * p.ldw || (f & ~(EP_STATS | MOCA_EP_ROWSUM | MOCA_EP_LN))) return false;
        if (p.M % p.wgroup_rows || p.wgroup_rows % ri.tm) return false;
        if ((int64_t)(p.M / p.wgroup_rows) * p.wgroup_stride * 2 >= (1ll << 31)) return false;
    }
    // one phase of upsample + conv: a 2 x 2 conv on the low-resolution grid, rows scattered by the plain store loop of the
    // 256- / 320-row kernels (fast gather), nothing else in the epilogue but the GroupNorm statistics
    if (p.up_phase && (p.splits != 1 || p.M <= 160 || !fast_gather(p) || p.residual || p.rowadd || (f & ~MOCA_EP_GSTAT) ||
                       (p.N % 128 && p.N % 160))) return false;
    return true;
}

Route checked_route(const moca_gemm_params& p) {
    const Route r = route_of(p);
    return route_can(r, p) ? r : R_NONE;
}

// What the queries share: the shape preamble, the split count as the launch will see it, the flag asked about added (a query answers
// for the call WITH its flag: the flag can move the call to another kernel), then route and capability.  `p` = that call.
Route query_route(const moca_gemm_params* pp, int flag, moca_gemm_params& p) {
    if (!pp) return R_NONE;
    p = *pp;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.N % 64 || p.K % 8) return R_NONE;
    normalise_splits(p);
    p.flags |= flag;
    return checked_route(p);
}

// fp16 split-K slabs (MOCA_TUNE_SLAB_F16): a split-K call of the 256-row kernel with an fp16 output and no GEGLU
bool slab_f16(Route r, const moca_gemm_params& p) {
    return moca_tuning_get(MOCA_TUNE_SLAB_F16) && p.splits > 1 && !(p.flags & (MOCA_EP_GEGLU | MOCA_EP_OUT_F32)) && (r == R_GLDS128 || r == R_GLDS160);
}
// can moca_gemm_splitk_groupnorm_f16 finish this (validated, split-normalised) MOCA_EP_SLABS call?  fp16 plain epilogue, one block per
// (statistics group, channel group) slab with the slab in registers
bool splitk_gn_ok(const moca_gemm_params& p, int HW, int fps) {
    if (p.splits < 2 || (p.flags & ~MOCA_EP_SLABS) || p.N % 32 || (p.N / 32) % 8 || p.N / 32 > 128 || p.up_phase) return false;
    if (HW <= 0 || fps <= 0 || p.M % (HW * fps)) return false;
    const int64_t nchunks = (int64_t)HW * fps * (p.N / 32 / 8);
    return nchunks >= 64 && nchunks <= 4096;
}

// Everything moca_gemm_f16 does before the launch: the argument contract, the split count, the route and its capability check, the
// launchers' reserved fields.  Returns the route with `p` ready to launch, or R_NONE (MOCA_E_BADARG).
Route prepare(const moca_gemm_params* pp, moca_gemm_params& p) {
    if (!pp) return R_NONE;
    p = *pp;
    if (p.splits < 1) p.splits = 1;
    if (!p.a || !p.w || !p.out) return R_NONE;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0) return R_NONE;
    if (p.N % 64 || p.K % 8 || p.ldw % BK || p.ldw < ((p.K + BK - 1) / BK) * BK) return R_NONE;
    const bool geglu = p.flags & MOCA_EP_GEGLU;
    if (geglu && p.N % 128) return R_NONE;
    if (p.ldo % 8 || (p.residual && p.ldr % 8) || (p.rowadd && (p.ld_rowadd % 8 || p.rowadd_div <= 0))) return R_NONE;
    if (p.splits > 1 && !p.splitk_ws) return R_NONE;
    if (p.prefetch_kib < 0 || (p.prefetch_kib > 0 && (!p.prefetch || (reinterpret_cast<uintptr_t>(p.prefetch) & 15)))) return R_NONE;
    // the plain-GELU epilogue: asked for with the small tile (or at M <= 128, where nothing else runs) and without split-K as given
    if ((p.flags & MOCA_EP_GELU) && (p.splits != 1 || !((p.flags & MOCA_FORCE_SMALL_TILE) || p.M <= 128))) return R_NONE;
    normalise_splits(p);
    if ((p.flags & MOCA_EP_SLABS) && (p.splits < 2 || (p.flags & ~MOCA_EP_SLABS))) return R_NONE;   // ask moca_gemm_splitk_groupnorm_ok() first
    if (p.up_phase && p.a_mode != MOCA_A_CONV3X3) return R_NONE;
    switch (p.a_mode) {
        case MOCA_A_LINEAR:
            if (!p.a2 && (p.lda % 8 || p.lda < p.K)) return R_NONE;      // (two sources: route_can; ask moca_gemm_cat_ok() first)
            break;
        case MOCA_A_CONV3X3:
            if (p.up_phase < 0 || p.up_phase > 4) return R_NONE;
            if (p.C % 8 || p.K != (p.up_phase ? 4 : 9) * p.C || p.inH <= 0 || p.inW <= 0 || p.outH <= 0 || p.outW <= 0) return R_NONE;
            if (p.up_phase && (p.stride != 1 || p.up || p.nopad_lo)) return R_NONE;
            if (p.stride != 1 && p.stride != 2) return R_NONE;
            if (p.nopad_lo != 0 && (p.nopad_lo != 1 || p.stride != 2 || p.up || (p.inH | p.inW) & 1)) return R_NONE;
            if (p.up && (p.stride != 1 || p.outH != 2 * p.inH || p.outW != 2 * p.inW)) return R_NONE;
            if (!p.up && p.stride == 1 && (p.outH != p.inH || p.outW != p.inW)) return R_NONE;
            if (p.stride == 2 && (p.outH != (p.inH - 1) / 2 + 1 || p.outW != (p.inW - 1) / 2 + 1)) return R_NONE;
            if (p.M % (p.outH * p.outW)) return R_NONE;
            break;
        case MOCA_A_TCONV3:
            if (p.C % 8 || p.K != 3 * p.C || p.T <= 0 || p.HW <= 0 || p.M % (p.T * p.HW)) return R_NONE;
            break;
        default:
            return R_NONE;
    }
    if (p.a2 && p.a_mode != MOCA_A_LINEAR) return R_NONE;
    if (p.gstat_cpg < 0 || p.gstat_coff < 0 || ((p.gstat_cpg || p.gstat_coff) && !(p.flags & MOCA_EP_GSTAT))) return R_NONE;
    if (p.tattn_causal && !(p.flags & MOCA_EP_TATTN)) return R_NONE;         // (the mask exists in the MOCA_EP_TATTN epilogue only)
    const Route r = checked_route(p);                 // ask the flag's query first: moca_gemm_colsum_rows(), _ln_ok(), _rowsum_cols(), ...
    if (r == R_NONE) return R_NONE;
    // the outputs and inputs the epilogues need
    if ((p.flags & MOCA_EP_COLSUM) && !p.colsum) return R_NONE;
    if ((p.flags & MOCA_EP_LN) && !(p.ln_gamma && p.ln_beta && p.ln_out && p.ld_ln % 8 == 0)) return R_NONE;
    if ((p.flags & MOCA_EP_ROWSUM) && !p.rowsum) return R_NONE;
    if ((p.flags & MOCA_EP_LNFOLD) && !(p.lnf_part && p.lnf_wsum && p.lnf_nparts >= 1)) return R_NONE;
    // MOCA_EP_GSTAT: a row tile must lie inside one statistics group
    if ((p.flags & MOCA_EP_GSTAT) &&
        !(p.gstat && !(p.flags & MOCA_EP_COLSUM) && p.gstat_rows > 0 && p.gstat_rows % route_info(r).tm == 0 && p.M % p.gstat_rows == 0 &&
          (p.gstat_cpg > 0 ? (p.gstat_coff + p.N - 1) / p.gstat_cpg < 32 : (p.N % 32 == 0 && p.gstat_coff == 0)))) return R_NONE;
    p.reserved4_ = 0;                                 // (bits 8.. carry the XCD partition chosen by the launcher)
    // bit 0: output rows leave with non-temporal stores when the output is at least half the 256 MiB Infinity Cache (see out_streams)
    if ((int64_t)p.M * (geglu ? p.N / 2 : p.N) * 2 >= (128ll << 20)) p.reserved4_ |= 1;
    if (slab_f16(r, p)) p.reserved4_ |= 4;            // bit 2: fp16 split-K slabs (MOCA_TUNE_SLAB_F16; the 256-row kernel only)
    return r;
}

int launch_route(Route r, const moca_gemm_params& p, hipStream_t st) {
    switch (r) {
        case R_TATTN: return moca_gemm_w80s_launch(3, p, st);
        case R_WS: return moca_gemm_ws_launch(p, st);
        case R_SQP: return moca_gemm_sqp_launch(p, st);
        case R_G4P: return moca_gemm_g4p_launch(p, st);
        case R_W80: return moca_gemm_w80s_launch(0, p, st);
        case R_W80W: return moca_gemm_w80s_launch(1, p, st);
        case R_W80H: return moca_gemm_w80h_launch(p, st);
        case R_SQ256: return moca_gemm_w80s_launch(2, p, st);
        case R_G4: return moca_gemm_g4_launch(p, st);
        case R_GLDS128: return moca_gemm_glds_launch(128, p, st);
        case R_GLDS160: return moca_gemm_glds_launch(160, p, st);
        case R_SMALL128: return launch_gemm_small(128, p, st);
        case R_SMALL64: return launch_gemm_small(64, p, st);
        case R_NONE: break;
    }
    return MOCA_E_BADARG;
}

}  // namespace

#ifdef MOCA_STAMPS
extern "C" int moca_debug_stamps(unsigned long long* host_out, int n_blocks) {
    if (n_blocks > STAMP_BLOCKS) n_blocks = STAMP_BLOCKS;
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), (size_t)n_blocks * STAMP_SLOTS * 8) == hipSuccess ? 0 : -2;
}
#endif

extern "C" int moca_gemm_route(const moca_gemm_params* pp) {
    moca_gemm_params p;
    return prepare(pp, p);
}

// rows per tile of the column sums a MOCA_EP_COLSUM launch leaves behind (0: this call cannot): 320 / 160 on the staggered kernel,
// 256 on the 256-row kernel, strips of 32 rows (MOCA_EP_GSTAT only) on the weight-stationary kernel
extern "C" int moca_gemm_colsum_rows(const moca_gemm_params* pp) {
    moca_gemm_params p;
    return route_info(query_route(pp, (pp && (pp->flags & MOCA_EP_GSTAT)) ? 0 : MOCA_EP_COLSUM, p)).tm;
}
// columns per column tile of the row sums a MOCA_EP_ROWSUM launch leaves behind (0: this call cannot)
extern "C" int moca_gemm_rowsum_cols(const moca_gemm_params* pp) {
    moca_gemm_params p;
    return route_info(query_route(pp, MOCA_EP_ROWSUM, p)).tn;
}
extern "C" int moca_gemm_ln_ok(const moca_gemm_params* pp) {
    moca_gemm_params p;
    return query_route(pp, MOCA_EP_LN, p) != R_NONE;
}
extern "C" int moca_gemm_lnfold_ok(const moca_gemm_params* pp) {
    moca_gemm_params p;
    return query_route(pp, MOCA_EP_LNFOLD, p) != R_NONE;
}
extern "C" int moca_gemm_tattn_ok(const moca_gemm_params* pp) {
    moca_gemm_params p;
    return query_route(pp, MOCA_EP_TATTN, p) != R_NONE;
}
extern "C" int moca_gemm_cat_ok(const moca_gemm_params* pp) {
    moca_gemm_params p;
    return query_route(pp, 0, p) != R_NONE && p.a2;
}
extern "C" int moca_gemm_wgroup_ok(const moca_gemm_params* pp) {
    moca_gemm_params p;
    return query_route(pp, 0, p) != R_NONE && p.wgroup_rows > 0;
}
extern "C" int moca_gemm_splitk_groupnorm_ok(const moca_gemm_params* pp, int32_t HW, int32_t frames_per_stat) {
    moca_gemm_params p;
    return query_route(pp, 0, p) != R_NONE && splitk_gn_ok(p, HW, frames_per_stat);
}

extern "C" int moca_gemm_splitk_groupnorm_f16(const moca_gemm_params* pp, void* y, const float* gamma, const float* beta, int32_t HW,
                                              int32_t frames_per_stat, float eps, int32_t silu, int32_t write_x, void* stream) {
    if (!pp || !y || !gamma || !beta) return MOCA_E_BADARG;
    moca_gemm_params p = *pp;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.N % 64 || p.K % 8 || !p.splitk_ws || (write_x && !p.out)) return MOCA_E_BADARG;
    if (p.ldo % 8 || (p.residual && p.ldr % 8) || (p.rowadd && (p.ld_rowadd % 8 || p.rowadd_div <= 0))) return MOCA_E_BADARG;
    normalise_splits(p);
    if (!splitk_gn_ok(p, HW, frames_per_stat)) return MOCA_E_BADARG;
    p.reserved4_ = slab_f16(route_of(p), p) ? 4 : 0;
    const int cpg = p.N / 32, R = HW * frames_per_stat;
    const int nchunks = R * (cpg / 8);
    const int cpt = (nchunks + 1023) / 1024;
    int thr = ((nchunks + cpt - 1) / cpt + 63) / 64 * 64;
    if (thr < (cpg + 63) / 64 * 64) thr = (cpg + 63) / 64 * 64;      // threads tid < cpg fill s_sc / s_sh (cpg = 128 with 64 chunks: ADVICE r5)
    const int n_slabs = (p.M / R) * 32;
    const double inv_count = 1.0 / ((double)R * cpg);
    hipStream_t st = moca_stream(stream);
    half_t* yo = reinterpret_cast<half_t*>(y);
#define MOCA_SKGN(CPT) hipLaunchKernelGGL(splitk_gn_kernel<CPT>, dim3(n_slabs), dim3(thr), 0, st, p, yo, gamma, beta, R, cpg, inv_count, eps, silu, write_x)
    if (cpt == 1) MOCA_SKGN(1); else if (cpt == 2) MOCA_SKGN(2); else if (cpt == 3) MOCA_SKGN(3); else MOCA_SKGN(4);
#undef MOCA_SKGN
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int64_t moca_gemm_splitk_ws_bytes(int32_t M, int32_t N, int32_t splits) {
    return splits > 1 ? (int64_t)splits * M * N * 4 : 0;
}

// validate, route, check (prepare), launch
extern "C" int moca_gemm_f16(const moca_gemm_params* pp, void* stream) {
    moca_gemm_params p;
    const Route r = prepare(pp, p);
    if (r == R_NONE) return MOCA_E_BADARG;
    hipStream_t st = moca_stream(stream);
    const int rc = launch_route(r, p, st);
    if (rc != MOCA_OK) return rc;
    if (p.splits > 1 && !(p.flags & MOCA_EP_SLABS)) {
        const int out_n = (p.flags & MOCA_EP_GEGLU) ? p.N / 2 : p.N;
        const int64_t total = (int64_t)p.M * (out_n / 8);
        int blocks = (int)((total + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, p);
        MOCA_CHECK_LAUNCH();
    }
    return MOCA_OK;
}

// The library's version string lives beside the kernels a diagnostic build changes (`make stamps` / `gndiag` / `diagx` recompile the GEMM
// files only, as one unit: gemm_diag.hip): such a build -- stamps, timing-only variants with wrong results -- reports "DIAG:<name>", and
// moca_video_amd/lib.py refuses to load it unless MOCA_HIP_DIAG=1 is set.
#ifdef MOCA_DIAG_NAME
extern "C" const char* moca_version(void) { return "moca_hip 0.1 (gfx950) DIAG:" MOCA_DIAG_NAME; }
#else
extern "C" const char* moca_version(void) { return "moca_hip 0.1 (gfx950)"; }
#endif
