// GroupNorm(32) (+SiLU) and LayerNorm on channels-last fp16 activations, fp32/fp64
// statistics.  HBM-bound kernels: every access is a 16-byte (8 x fp16) coalesced
// load/store along the channel axis; partial statistics are deterministic (no atomics).
#include "common.h"

namespace {

constexpr int GN_GROUPS = 32;

__host__ __device__ inline int gn_nchunk(int F, int HW) {
    int n = 2048 / (F > 0 ? F : 1);
    if (n < 1) n = 1;
    const int maxc = (HW + 7) / 8;
    if (n > maxc) n = maxc;
    if (n < 1) n = 1;
    return n;
}

// ---- the streaming passes: grid (F, nchunk), blockDim = (C/8, ppb).  Block (f, chunk) owns rows [begin, end) of frame f (the last
// chunks of a frame may be short or empty); thread (cx, py) owns channels [8cx, 8cx+8) of rows begin + py, begin + py + ppb, ... ----
struct gn_rows_t { int begin, end; };
__device__ __forceinline__ gn_rows_t gn_chunk_rows(int HW, int nchunk) {
    const int pc = (HW + nchunk - 1) / nchunk;
    const int begin = blockIdx.y * pc;
    return {begin, min(begin + pc, HW)};
}

// The statistics pass of a block over its chunk: the block's per-row-slot sums (comp 0) / sums of squares (comp 1) of every channel end
// in LDS tables [ppb][C] (dynamic LDS: 2 x ppb x C floats), behind a barrier.  `src` is the thread's first channel in row 0 of the
// frame, `ld` the row stride; `each(row, vector)` sees every vector loaded (the concat stores it).
__device__ __forceinline__ float* gn_lds_table(int comp, int C) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_sum = reinterpret_cast<float*>(smem_raw);
    return comp ? s_sum + blockDim.y * C : s_sum;
}
template <class Each>
__device__ __forceinline__ void gn_chunk_stats(const half_t* src, int ld, int HW, int C, int nchunk, Each each) {
    const int cx = threadIdx.x, py = threadIdx.y, ppb = blockDim.y;
    const gn_rows_t r = gn_chunk_rows(HW, nchunk);
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[j] = 0.f; q[j] = 0.f; }
    // four pixels per trip: the four 16-byte loads of a thread are in flight together (a one-load-per-trip loop leaves the
    // memory pipe of this streaming pass mostly empty)
    int pp = r.begin + py;
    for (; pp + 3 * ppb < r.end; pp += 4 * ppb) {
        half8v v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const half8v*>(src + (int64_t)(pp + u * ppb) * ld);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            each(pp + u * ppb, v[u]);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float a = (float)v[u][j]; s[j] += a; q[j] += a * a; }
        }
    }
    for (; pp < r.end; pp += ppb) {
        const half8v v = *reinterpret_cast<const half8v*>(src + (int64_t)pp * ld);
        each(pp, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float a = (float)v[j]; s[j] += a; q[j] += a * a; }
    }
    float* s_sum = gn_lds_table(0, C);
    float* s_sq = gn_lds_table(1, C);
#pragma unroll
    for (int j = 0; j < 8; ++j) { s_sum[py * C + cx * 8 + j] = s[j]; s_sq[py * C + cx * 8 + j] = q[j]; }
    __syncthreads();
}
// channels [c0, c1) of N of the tables summed over the block's row slots, row slots outermost (the order is part of the result)
template <int N>
__device__ __forceinline__ void gn_lds_sum(const float* const (&tab)[N], int C, int c0, int c1, float (&t)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n) t[n] = 0.f;
    for (int y = 0; y < (int)blockDim.y; ++y)
        for (int c = c0; c < c1; ++c)
#pragma unroll
            for (int n = 0; n < N; ++n) t[n] += tab[n][y * C + c];
}
// The pass for a source whose channel c counts for group (coff + c) / cpg of gstat [statistics group][32][2]: one thread per (group the
// source touches, comp) adds the block's share (fixed-point atomics, as MOCA_EP_GSTAT)
template <class Each>
__device__ __forceinline__ void gn_chunk_gstat(const half_t* src, int ld, int64_t* gstat, int HW, int C, int nchunk, int frames_per_stat,
                                               int cpg, int coff, Each each) {
    gn_chunk_stats(src, ld, HW, C, nchunk, each);
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    const int g0 = coff / cpg, g1 = (coff + C - 1) / cpg;
    if (tid < 2 * (g1 - g0 + 1)) {
        const int g = g0 + (tid >> 1), comp = tid & 1;
        const float* const tab[1] = {gn_lds_table(comp, C)};
        float t[1];
        gn_lds_sum(tab, C, max(g * cpg - coff, 0), min((g + 1) * cpg - coff, C), t);
        moca_gstat_add(gstat + ((int64_t)(blockIdx.x / frames_per_stat) * GN_GROUPS + g) * 2 + comp, comp, t[0]);
    }
}

// ---- K1: per (frame, pixel-chunk) partial sums per group ---------------------
__global__ void gn_partial_kernel(const half_t* __restrict__ x, float* __restrict__ partial,
                                  int HW, int C, int nchunk) {
    const int f = blockIdx.x, chunk = blockIdx.y;
    gn_chunk_stats(x + ((int64_t)f * HW) * C + threadIdx.x * 8, C, HW, C, nchunk, [](int, const half8v&) {});
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    if (tid < GN_GROUPS) {
        const int cpg = C / GN_GROUPS;
        const float* const tab[2] = {gn_lds_table(0, C), gn_lds_table(1, C)};
        float t[2];
        gn_lds_sum(tab, C, tid * cpg, (tid + 1) * cpg, t);
        float* o = partial + (((int64_t)f * nchunk + chunk) * GN_GROUPS + tid) * 2;
        o[0] = t[0]; o[1] = t[1];
    }
}

// ---- K2: finalize mean / rstd per (stat group, channel group) in fp64 --------
// one block of FIN_T threads per (stat group, channel group): grid (stat groups, 32).  Up to 1280 partial pairs per block at
// the 320-channel level with 16 frames per statistics group: every thread issues all its loads before the first add (a
// one-wavefront loop of dependent L2 round trips took ~10 us there), fp64 accumulation, fixed combine order (deterministic).
// `pair(i)` is the address of the block's i-th (sum, sum of squares) pair, i < n.
constexpr int FIN_T = 256;

template <class Pair>
__device__ __forceinline__ void gn_finalize(int n, Pair pair, float* __restrict__ meanrstd, double inv_count, float eps) {
    __shared__ double s_a[FIN_T / 64], s_b[FIN_T / 64];
    double a = 0.0, b = 0.0;
    for (int i0 = threadIdx.x; i0 < n; i0 += 4 * FIN_T) {
        float2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * FIN_T;
            const float* at = pair(i);
            v[u] = i < n ? *reinterpret_cast<const float2*>(at) : float2{0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { a += (double)v[u].x; b += (double)v[u].y; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int w = 0; w < FIN_T / 64; ++w) { sa += s_a[w]; sb += s_b[w]; }
        const moca_gn_stat st = moca_gn_finish(sa, sb, inv_count, eps);
        const int64_t slot = (int64_t)blockIdx.x * GN_GROUPS + blockIdx.y;
        meanrstd[slot * 2] = (float)st.mean;
        meanrstd[slot * 2 + 1] = (float)st.rstd;
    }
}

__global__ __launch_bounds__(FIN_T) void gn_finalize_kernel(const float* __restrict__ partial, float* __restrict__ meanrstd,
                                                            int frames_per_stat, int nchunk, double inv_count, float eps) {
    const int sg = blockIdx.x, g = blockIdx.y;
    const int n = frames_per_stat * nchunk;
    const float* base = partial + (int64_t)sg * n * GN_GROUPS * 2;
    gn_finalize(n, [&](int i) { return base + ((int64_t)i * GN_GROUPS + g) * 2; }, meanrstd, inv_count, eps);
}

// ---- K2': the same from the column sums a MOCA_EP_COLSUM GEMM left behind: colsum[row tile][C][2], a statistics group
// (sg, g) = tiles [sg*tps, (sg+1)*tps) x channels [g*cpg, (g+1)*cpg) ----
__global__ __launch_bounds__(FIN_T) void gn_finalize_colsum_kernel(const float* __restrict__ colsum, float* __restrict__ meanrstd,
                                                                   int tps, int C, int cpg, double inv_count, float eps) {
    const int sg = blockIdx.x, g = blockIdx.y;
    gn_finalize(tps * cpg, [&](int i) {
        const int t = i / cpg, c = g * cpg + (i - t * cpg);
        return colsum + (((int64_t)sg * tps + t) * C + c) * 2;
    }, meanrstd, inv_count, eps);
}

// ---- K3: apply (x - mean) * rstd * gamma + beta, optional SiLU ----------------
// Two batches of four 16-byte loads per thread in flight: the first batch is issued BEFORE the statistics / affine parameters
// are fetched (their latency used to precede the first x load of every block) -- `scale_shift(sc, sh)` fetches them and leaves the
// thread's 8 scales and shifts --, the next batch before the current one is normalised and stored.  Rows past the end of the chunk are
// fetched from the last valid row (cache hits) and not stored.  `src` / `dst`: the thread's first channel in row 0 of the frame; the
// source has row stride `ld`, the output C.
// STREAM: the output is at least half the Infinity Cache (B = 16 forwards at the 320- / 640-channel levels) and leaves with non-temporal
// stores, as the GEMM outputs of that size do (gemm.hip, out_streams)
template <bool STREAM>
__device__ __forceinline__ void gn_st8(half_t* ptr, const half8v v) {
    if constexpr (STREAM) __builtin_nontemporal_store(v, reinterpret_cast<half8v*>(ptr));
    else *reinterpret_cast<half8v*>(ptr) = v;
}
template <bool STREAM, class ScaleShift>
__device__ __forceinline__ void gn_apply_chunk(const half_t* src, int ld, half_t* dst, int HW, int C, int nchunk, int silu, ScaleShift scale_shift) {
    const int py = threadIdx.y, ppb = blockDim.y;
    const gn_rows_t r = gn_chunk_rows(HW, nchunk);
    if (r.begin >= r.end) return;
    auto load4 = [&](half8v (&v)[4], int pp) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const half8v*>(src + (int64_t)min(pp + u * ppb, r.end - 1) * ld);
    };
    int pp = r.begin + py;
    half8v cur[4], nxt[4];
    load4(cur, pp);
    float sc[8], sh[8];
    scale_shift(sc, sh);
    // (written here, not gn_norm<8> on pointers to sc / sh: that form leaves the `more` test twice in the loop, +6 instructions)
    auto norm8 = [&](const half8v& v) {
        half8v o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float a = (float)v[j] * sc[j] + sh[j];
            if (silu) a = moca_silu(a);
            o[j] = (half_t)a;
        }
        return o;
    };
    for (; pp < r.end; pp += 4 * ppb) {
        const bool more = pp + 4 * ppb < r.end;
        if (more) load4(nxt, pp + 4 * ppb);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (pp + u * ppb < r.end) gn_st8<STREAM>(dst + (int64_t)(pp + u * ppb) * C, norm8(cur[u]));
        if (more) {
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
        }
    }
}

// (scalar gamma / beta loads: this entry does not require 16-byte aligned parameters)
__global__ void gn_apply_kernel(const half_t* __restrict__ x, half_t* __restrict__ y,
                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                const float* __restrict__ meanrstd, int HW, int C, int nchunk,
                                int frames_per_stat, int silu) {
    const int f = blockIdx.x, cx = threadIdx.x;
    const int64_t off = ((int64_t)f * HW) * C + cx * 8;
    gn_apply_chunk<false>(x + off, C, y + off, HW, C, nchunk, silu, [&](float (&sc)[8], float (&sh)[8]) {
        const int cpg = C / GN_GROUPS;
        const int sg = f / frames_per_stat;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = cx * 8 + j;
            const int g = c / cpg;
            const float mean = meanrstd[((int64_t)sg * GN_GROUPS + g) * 2];
            const float rstd = meanrstd[((int64_t)sg * GN_GROUPS + g) * 2 + 1];
            sc[j] = rstd * gamma[c];
            sh[j] = beta[c] - mean * sc[j];
        }
    });
}

// ---- K3': apply with the statistics a MOCA_EP_GSTAT producer accumulated: gstat i64 fixed point [statistics group][32][2] = (sum, sum of
// squares), finished.  The first 32 threads of a block turn its statistics group's 32 pairs -- `sums(group, sum, sq)` reads one -- into
// (mean, rstd) in fp64 while the block's first batch of x loads is in flight; no finalize launch exists.
template <class Sums>
__device__ __forceinline__ void gn_gstat_scale_shift(const float* gamma, const float* beta, int cpg, double inv_count, float eps,
                                                     float (&sc)[8], float (&sh)[8], Sums sums) {
    __shared__ float s_mr[2 * GN_GROUPS];
    const int cx = threadIdx.x, tid = threadIdx.y * blockDim.x + cx;
    // (the affine parameters are fetched BEFORE the statistics hand-off: behind the barrier they were a third dependent round trip of
    //  a block whose whole life is one batch of x -- profiles/r05_ab_gn_apply_prologue.txt)
    const f32x4 gm0 = *reinterpret_cast<const f32x4*>(gamma + cx * 8), gm1 = *reinterpret_cast<const f32x4*>(gamma + cx * 8 + 4);
    const f32x4 bt0 = *reinterpret_cast<const f32x4*>(beta + cx * 8), bt1 = *reinterpret_cast<const f32x4*>(beta + cx * 8 + 4);
    if (tid < GN_GROUPS) {
        double a, b;
        sums(tid, a, b);
        const moca_gn_stat st = moca_gn_finish(a, b, inv_count, eps);
        s_mr[2 * tid] = (float)st.mean;
        s_mr[2 * tid + 1] = (float)st.rstd;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = cx * 8 + j;
        const int g = c / cpg;
        sc[j] = s_mr[2 * g + 1] * (j < 4 ? gm0[j & 3] : gm1[j & 3]);
        sh[j] = (j < 4 ? bt0[j & 3] : bt1[j & 3]) - s_mr[2 * g] * sc[j];
    }
}

template <bool STREAM>
__global__ void gn_apply_gstat_kernel(const half_t* __restrict__ x, half_t* __restrict__ y,
                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const int64_t* __restrict__ gstat, int HW, int C, int nchunk,
                                      int frames_per_stat, double inv_count, float eps, int silu) {
    const int f = blockIdx.x;
    const int64_t off = ((int64_t)f * HW) * C + threadIdx.x * 8;
    gn_apply_chunk<STREAM>(x + off, C, y + off, HW, C, nchunk, silu, [&](float (&sc)[8], float (&sh)[8]) {
        const int sg = f / frames_per_stat;
        gn_gstat_scale_shift(gamma, beta, C / GN_GROUPS, inv_count, eps, sc, sh, [&](int g, double& sa, double& sq) {
            const int64_t* gs = gstat + ((int64_t)sg * GN_GROUPS + g) * 2;
            sa = moca_gstat_get(gs, 0); sq = moca_gstat_get(gs + 1, 1);
        });
    });
}

// ---- torch.cat(dim=channels) that also leaves the GroupNorm statistics of its output behind (openaimodel3d.py:571 followed by
// ResBlock.in_layers[0], :149): the copy is a streaming pass over both inputs anyway; every thread owns 8 fixed channels of
// the concatenated row, accumulates their sums / sums of squares over its pixels, the block combines them per channel group
// through LDS and adds them to gstat (fixed-point atomics, as MOCA_EP_GSTAT) -- the consumer GroupNorm is then one apply launch instead
// of partial + finalize + apply.  blockDim = (C/8, ppb), grid (F, nchunk) as the GroupNorm passes: the statistics pass of
// gstat_accum_kernel over the concatenated row (coff = 0, cpg = C / 32) that also stores what it loads. ----
template <bool STREAM>
__global__ void concat_gstat_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, half_t* __restrict__ out,
                                    int64_t* __restrict__ gstat, int HW, int C1, int C2, int nchunk, int frames_per_stat) {
    const int C = C1 + C2;
    const int f = blockIdx.x, cx = threadIdx.x;
    const bool from_a = cx * 8 < C1;
    const half_t* src = from_a ? a + ((int64_t)f * HW) * C1 + cx * 8 : b + ((int64_t)f * HW) * C2 + (cx * 8 - C1);
    half_t* dst = out + ((int64_t)f * HW) * C + cx * 8;
    gn_chunk_gstat(src, from_a ? C1 : C2, gstat, HW, C, nchunk, frames_per_stat, C / GN_GROUPS, 0,
                   [&](int pp, const half8v& v) { gn_st8<STREAM>(dst + (int64_t)pp * C, v); });
}

// ---- the VIRTUAL torch.cat (openaimodel3d.py:571) in front of ResBlock.in_layers[0]: GroupNorm(+SiLU) of cat([a, b], channels) reading a
// and b where their producers left them; only the normalised concat is written.  Thread cx owns 8 channels of the concatenated row (C1 % 8
// == 0: from one source), as in concat_gstat_kernel.  Statistics: gstat_cat (the concat's grouping) holds a's share -- accumulated by a's
// producer (MOCA_EP_GSTAT with gstat_cpg = C / 32) or by gstat_accum_kernel -- and either b's share too (gstat_b == NULL) or b's OWN
// finished statistics are merged here (groups of cpg2 = C2 / 32 channels: cpg % cpg2 == 0 and (C1 % cpg) % cpg2 == 0, host-checked, so
// every group of b lies inside one group of the concat). ----
template <bool STREAM>
__global__ void gn_apply_gstat_cat_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, half_t* __restrict__ y,
                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                          const int64_t* __restrict__ gstat_cat, const int64_t* __restrict__ gstat_b,
                                          int HW, int C1, int C2, int nchunk, int frames_per_stat, int sgb_mod, double inv_count, float eps, int silu) {
    const int C = C1 + C2;
    const int f = blockIdx.x, cx = threadIdx.x;
    const bool from_a = cx * 8 < C1;
    const half_t* src = from_a ? a + ((int64_t)f * HW) * C1 + cx * 8 : b + ((int64_t)f * HW) * C2 + (cx * 8 - C1);
    gn_apply_chunk<STREAM>(src, from_a ? C1 : C2, y + ((int64_t)f * HW) * C + cx * 8, HW, C, nchunk, silu, [&](float (&sc)[8], float (&sh)[8]) {
        const int cpg = C / GN_GROUPS;
        const int sg = f / frames_per_stat;
        gn_gstat_scale_shift(gamma, beta, cpg, inv_count, eps, sc, sh, [&](int g, double& sa, double& sq) {
            const int64_t* ga = gstat_cat + ((int64_t)sg * GN_GROUPS + g) * 2;
            sa = moca_gstat_get(ga, 0); sq = moca_gstat_get(ga + 1, 1);
            if (gstat_b) {
                const int cpg2 = C2 / GN_GROUPS;
                const int lo = max(g * cpg - C1, 0), hi = min((g + 1) * cpg - C1, C2);         // b's channels inside concat group g
                for (int j = lo / cpg2; j * cpg2 < hi; ++j) {
                    const int64_t* gb = gstat_b + ((int64_t)(sg % sgb_mod) * GN_GROUPS + j) * 2;   // (b = `reps` copies of Fb frames: the shared prefix)
                    sa += moca_gstat_get(gb, 0); sq += moca_gstat_get(gb + 1, 1);
                }
            }
        });
    });
}

// ---- statistics only: the share of ONE source x [F][HW][C] of a virtual concat in the concat's GroupNorm statistics, for a source whose
// producer could not leave them (an `Upsample`, the repeat of the shared prefix): channel c counts for group (coff + c) / cpg of
// gstat [statistics group][32][2].  A read-only pass (half the traffic of the copy it replaces). ----
__global__ void gstat_accum_kernel(const half_t* __restrict__ x, int64_t* __restrict__ gstat, int HW, int C, int nchunk,
                                   int frames_per_stat, int cpg, int coff) {
    gn_chunk_gstat(x + ((int64_t)blockIdx.x * HW) * C + threadIdx.x * 8, C, gstat, HW, C, nchunk, frames_per_stat, cpg, coff,
                   [](int, const half8v&) {});
}

// ---- single-launch GroupNorm for small tensors ------------------------------------
// A statistics slab = (statistics group sg, channel group g): R = frames_per_stat*HW consecutive rows x cpg channels.
// S blocks share one slab: each of them reduces the WHOLE slab (redundantly -- a slab is at most a few hundred KB and
// its S blocks are placed on the same XCD, so the repeats are L2 hits) and then normalises its own 1/S of the rows.
// No inter-block hand-off, so the three launches of the streaming path become one and x is fetched from HBM once.
// Used when the tensor is small enough that the streaming path is bound by its launches rather than by HBM.
//
// The block tail of both single-launch kernels (and, written out, of gemm.hip's splitk_gn_kernel): every thread of a block of `nwaves`
// <= NW waves brings its sum / sum of squares over the slab; wave shuffles, then the wave sums through LDS in wave order (fp64, fixed
// order: deterministic), then thread c < cpg leaves scale and shift of the slab's channel c in s_sc / s_sh, from the gamma / beta value
// it holds.  Ends behind its barrier: the tables are ready.
template <int NW>
__device__ __forceinline__ void gn_slab_table(float s, float q, int nwaves, int cpg, float gm_t, float bt_t, double inv_count, float eps,
                                              float* s_sc, float* s_sh) {
    __shared__ float s_red[2][NW];
    const int tid = threadIdx.x;
    s = wave_sum(s); q = wave_sum(q);
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = s; s_red[1][tid >> 6] = q; }
    __syncthreads();
    if (tid < cpg) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < nwaves; ++w) { a += (double)s_red[0][w]; b += (double)s_red[1][w]; }
        const moca_gn_stat st = moca_gn_finish(a, b, inv_count, eps);
        const float sc = (float)st.rstd * gm_t;
        s_sc[tid] = sc;
        s_sh[tid] = bt_t - (float)st.mean * sc;
    }
    __syncthreads();
}
// VEC fp16 values of consecutive channels normalised from those tables: x * scale + shift (+SiLU)
template <int VEC> using halfNv = _Float16 __attribute__((ext_vector_type(VEC)));
template <int VEC>
__device__ __forceinline__ halfNv<VEC> gn_norm(const halfNv<VEC> v, const float* sc, const float* sh, int silu) {
    halfNv<VEC> o;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        float a = (float)v[j] * sc[j] + sh[j];
        if (silu) a = moca_silu(a);
        o[j] = (half_t)a;
    }
    return o;
}

template <int VEC>
__global__ __launch_bounds__(256) void gn_slab_kernel(const half_t* __restrict__ x, half_t* __restrict__ y,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      int R, int C, int cpg, int S, double inv_count,
                                                      float eps, int silu) {
    typedef halfNv<VEC> vec_t;
    __shared__ float s_sc[128], s_sh[128];               // cpg <= 128
    const int tid = threadIdx.x, L = blockIdx.x;
    // consecutive block ids go round-robin over the 8 XCDs: the S blocks of a slab share one (the slab count is a multiple of 32)
    const int w = L >> 3, slab = (L & 7) + 8 * (w / S), split = w % S;
    const int sg = slab / GN_GROUPS, g = slab % GN_GROUPS;
    const int vpr = cpg / VEC;                            // vectors per row
    const int dr = 256 / vpr, dv = 256 % vpr;             // advancing a flat index by 256 = dr rows + dv vectors
    const int64_t base = (int64_t)sg * R * C + g * cpg;
    const half_t* xs = x + base;
    const float gm_t = tid < cpg ? gamma[g * cpg + tid] : 0.f, bt_t = tid < cpg ? beta[g * cpg + tid] : 0.f;   // (in flight under the statistics pass)
    // ---- pass 1: sum / sum of squares of the whole slab ----
    float s = 0.f, q = 0.f;
    {
        int row = tid / vpr, v = tid % vpr;
#pragma unroll 4
        for (; row < R;) {
            const vec_t d = *reinterpret_cast<const vec_t*>(xs + (int64_t)row * C + v * VEC);
#pragma unroll
            for (int j = 0; j < VEC; ++j) { const float a = (float)d[j]; s += a; q += a * a; }
            row += dr; v += dv;
            if (v >= vpr) { v -= vpr; ++row; }
        }
    }
    gn_slab_table<4>(s, q, 4, cpg, gm_t, bt_t, inv_count, eps, s_sc, s_sh);
    // ---- pass 2: normalise rows [r0, r1) of the slab ----
    const int rps = (R + S - 1) / S;
    const int r0 = split * rps, r1 = min(R, r0 + rps);
    half_t* ys = y + base;
    {
        int row = r0 + tid / vpr, v = tid % vpr;
#pragma unroll 2
        for (; row < r1;) {
            const int64_t o = (int64_t)row * C + v * VEC;
            *reinterpret_cast<vec_t*>(ys + o) = gn_norm<VEC>(*reinterpret_cast<const vec_t*>(xs + o), s_sc + v * VEC, s_sh + v * VEC, silu);
            row += dr; v += dv;
            if (v >= vpr) { v -= vpr; ++row; }
        }
    }
}

// ---- single-launch GroupNorm with the slab in REGISTERS: one block per (statistics group, channel group) slab of at most 4096
// 16-byte chunks (64 KiB: the 1280-channel levels -- 640 rows x 80 B with 16-frame statistics at 5 x 8 latents, 160 rows x 80 B per
// frame at 10 x 16), every thread keeps its <= 4 chunks, the block reduces (wave shuffles + LDS), normalises from registers and
// stores: x is read ONCE and nothing is reduced redundantly (gn_slab_kernel: S = 16 blocks each re-reduce the whole slab).
template <int CPT>
__global__ __launch_bounds__(1024) void gn_slab_reg_kernel(const half_t* __restrict__ x, half_t* __restrict__ y,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            int R, int C, int cpg, double inv_count, float eps, int silu) {
    __shared__ float s_sc[128], s_sh[128];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int slab = blockIdx.x, sg = slab / GN_GROUPS, g = slab % GN_GROUPS;
    const int vpr = cpg / 8, nchunks = R * vpr;
    const int64_t base = (int64_t)sg * R * C + g * cpg;
    const float gm_t = tid < cpg ? gamma[g * cpg + tid] : 0.f, bt_t = tid < cpg ? beta[g * cpg + tid] : 0.f;   // (in flight under the slab's loads)
    half8v v[CPT];
    int off[CPT];
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int idx = tid + i * nthr;
        off[i] = -1;
        if (idx < nchunks) {
            const int row = idx / vpr, c = idx - row * vpr;
            off[i] = row * C + c * 8;
            v[i] = *reinterpret_cast<const half8v*>(x + base + off[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (off[i] >= 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float a = (float)v[i][j]; s += a; q += a * a; }
        }
    gn_slab_table<16>(s, q, nthr >> 6, cpg, gm_t, bt_t, inv_count, eps, s_sc, s_sh);
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (off[i] >= 0) {
            const int c0 = (off[i] % C);                 // = c * 8 (row * C is a multiple of C)
            *reinterpret_cast<half8v*>(y + base + off[i]) = gn_norm<8>(v[i], s_sc + c0, s_sh + c0, silu);
        }
}

// ---- LayerNorm: one wavefront per row, row kept in registers; every wave keeps LN_ROWS rows in flight ------
// (one row per wave leaves a CU with ~20 KB of loads in flight -- 3.6 TB/s chip-wide at C = 320; with four rows per
//  wave the loads of all four are issued before the first reduction)
template <int MAXCH, int LN_ROWS>  // max 16-byte chunks per lane; rows per wave (4 when there are enough rows to fill the chip)
__global__ __launch_bounds__(256) void layernorm_kernel(const half_t* __restrict__ x, half_t* __restrict__ y,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int M, int C, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * 4 + wave) * LN_ROWS;
    if (row0 >= M) return;
    const int nch = C / 8;
    half8v v[LN_ROWS][MAXCH];
#pragma unroll
    for (int r = 0; r < LN_ROWS; ++r) {
        const int row = min(row0 + r, M - 1);            // (rows past the end repeat the last row; their store is skipped)
        const half_t* xr = x + (int64_t)row * C;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int ch = lane + 64 * i;
            if (ch < nch) v[r][i] = *reinterpret_cast<const half8v*>(xr + ch * 8);
        }
    }
    float mean[LN_ROWS], rstd[LN_ROWS];
#pragma unroll
    for (int r = 0; r < LN_ROWS; ++r) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int ch = lane + 64 * i;
            if (ch < nch) {
#pragma unroll
                for (int j = 0; j < 8; ++j) s += (float)v[r][i][j];
            }
        }
        s = wave_sum(s);
        mean[r] = s / (float)C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int ch = lane + 64 * i;
            if (ch < nch) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float d = (float)v[r][i][j] - mean[r]; q += d * d; }
            }
        }
        q = wave_sum(q);
        rstd[r] = rsqrtf(q / (float)C + eps);
    }
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + ch * 8), g1 = *reinterpret_cast<const f32x4*>(gamma + ch * 8 + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + ch * 8), b1 = *reinterpret_cast<const f32x4*>(beta + ch * 8 + 4);
#pragma unroll
            for (int r = 0; r < LN_ROWS; ++r) {
                if (row0 + r < M) {
                    half8v o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        o[j] = (half_t)(((float)v[r][i][j] - mean[r]) * rstd[r] * g0[j] + b0[j]);
                        o[4 + j] = (half_t)(((float)v[r][i][4 + j] - mean[r]) * rstd[r] * g1[j] + b1[j]);
                    }
                    *reinterpret_cast<half8v*>(y + (int64_t)(row0 + r) * C + ch * 8) = o;
                }
            }
        }
    }
}

}  // namespace

// ---- GroupNorm folded into the consuming linear as per-statistics-group weights (moca_groupnorm_fold_weights_f16) ----
// block (sg, row block of 16 W rows): the 2 x K scale / beta values of the group in LDS, then thread = one 8-element chunk of a W row:
// scaled copy wg = fp16(w * s) + its share of the shift (reduced over the row's chunks through LDS in a fixed order: deterministic).
// The GEMM multiplies RAW x by the ROUNDED wg, so the mean term of the shift is taken from the stored wg as well:
//     bg[n] = bias[n] + sum_k beta_k * w[n][k] - sum_k mean_g(k) * float(wg[n][k])
// and the launch computes sum_k (x_k - mean) * wg[n][k] + ...: the rounding error of wg multiplies x - mean, not x.  (With the mean term
// taken from the unrounded w * s the error grew with |group mean| / std -- modelled 1.4e-3 at a ratio of 10, 4.4e-3 at 30; the sweep of
// tests/test_groupnorm_gpu.py holds every ratio up to 100 to the fp16 kernel tolerance.)
__global__ __launch_bounds__(256) void gn_fold_weights_kernel(const half_t* __restrict__ w, const float* __restrict__ bias,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const int64_t* __restrict__ gstat, half_t* __restrict__ wg, float* __restrict__ bg,
                                                              int N, int K, int ldw, double inv_count, float eps) {
    extern __shared__ float s_st[];                       // [2][K] scale, beta; then [rows][chunks] partial dots
    const int sg = blockIdx.x, tid = threadIdx.x;
    const int cpg = K / GN_GROUPS;
    __shared__ float s_mr[2 * GN_GROUPS];
    if (tid < GN_GROUPS) {
        const double a = moca_gstat_get(gstat + ((int64_t)sg * GN_GROUPS + tid) * 2, 0), b = moca_gstat_get(gstat + ((int64_t)sg * GN_GROUPS + tid) * 2 + 1, 1);
        const moca_gn_stat st = moca_gn_finish(a, b, inv_count, eps);
        s_mr[2 * tid] = (float)st.mean;
        s_mr[2 * tid + 1] = (float)st.rstd;
    }
    __syncthreads();
    for (int k = tid; k < K; k += 256) {
        const int g = k / cpg;
        s_st[k] = s_mr[2 * g + 1] * gamma[k];
        s_st[K + k] = beta[k];
    }
    __syncthreads();
    const int cpr = ldw / 8;                              // 16-byte chunks per W row (padding included: copied as zeros x scale 0)
    float* s_dot = s_st + 2 * K;
    const int rows_pb = 16;
    const int n0 = blockIdx.y * rows_pb;
    for (int idx = tid; idx < rows_pb * cpr; idx += 256) {
        const int r = idx / cpr, ch = idx - r * cpr, n = n0 + r;
        float dot = 0.f;
        if (n < N) {
            const half8v v = *reinterpret_cast<const half8v*>(w + (int64_t)n * ldw + ch * 8);
            half8v o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = ch * 8 + j;
                const float x = (float)v[j];
                const float sc = k < K ? s_st[k] : 0.f, be = k < K ? s_st[K + k] : 0.f, mu = k < K ? s_mr[2 * (k / cpg)] : 0.f;
                o[j] = (half_t)(x * sc);
                dot += x * be - mu * (float)o[j];
            }
            *reinterpret_cast<half8v*>(wg + ((int64_t)sg * N + n) * ldw + ch * 8) = o;
        }
        s_dot[idx] = dot;
    }
    __syncthreads();
    if (tid < rows_pb && n0 + tid < N) {
        float a = bias ? bias[n0 + tid] : 0.f;
        for (int ch = 0; ch < cpr; ++ch) a += s_dot[tid * cpr + ch];
        bg[(int64_t)sg * N + n0 + tid] = a;
    }
}

namespace {

// What the host side of every streaming pass shares: the conditions on (F, HW, C, frames_per_stat) and the launch they lead to.
// cpg = channels per group; 0 = the tensor is what GroupNorm(32) normalises (C % 32 == 0 required, C / 32 channels per group).
struct gn_stream_t {
    bool ok;            // false: MOCA_E_BADARG
    int nch8, ppb, nchunk;
    dim3 grid, block;   // (F, nchunk) x (C / 8, ppb)
    double inv_count;   // 1 / values of a (statistics group, channel group)
    size_t lds;         // bytes of the statistics walk's tables (gn_lds_table)
    bool streams;       // the output leaves with non-temporal stores (the STREAM instantiations): 128 MiB or more
};

gn_stream_t gn_stream(int32_t F, int32_t HW, int32_t C, int32_t frames_per_stat, int32_t cpg = 0) {
    gn_stream_t g = {};
    if (F <= 0 || HW <= 0 || C <= 0 || C % 8 || frames_per_stat <= 0 || F % frames_per_stat) return g;
    if (!cpg) {
        if (C % GN_GROUPS) return g;
        cpg = C / GN_GROUPS;
    }
    g.nch8 = C / 8;
    if (g.nch8 > 1024) return g;
    g.ppb = 256 / g.nch8;
    if (g.ppb < 1) g.ppb = 1;
    g.nchunk = gn_nchunk(F, HW);
    g.grid = dim3(F, g.nchunk);
    g.block = dim3(g.nch8, g.ppb);
    g.inv_count = 1.0 / ((double)frames_per_stat * HW * cpg);
    g.lds = (size_t)g.ppb * C * 2 * sizeof(float);
    g.streams = (int64_t)F * HW * C * 2 >= (128ll << 20);
    g.ok = true;
    return g;
}

// Everything moca_groupnorm_nhwc_f16 decides before its first launch: the launch and moca_groupnorm_route() both read it from here.
struct gn_plan_t {
    int route;        // MOCA_GN_ROUTE_*, 0 = MOCA_E_BADARG
    gn_stream_t geo;  // streaming path
    int n_slabs, R;   // slab paths: (statistics group, channel group) slabs of R rows
    int S;            // gn_slab_kernel: blocks per slab
    int cpt, threads; // gn_slab_reg_kernel: 16-byte chunks per thread, threads per block
};

gn_plan_t gn_plan(int32_t F, int32_t HW, int32_t C, int32_t frames_per_stat) {
    gn_plan_t pl = {};
    pl.geo = gn_stream(F, HW, C, frames_per_stat);
    if (!pl.geo.ok) return pl;
    pl.threads = pl.geo.nch8 * pl.geo.ppb;
    pl.route = MOCA_GN_ROUTE_STREAM;
    // small tensors: one launch (gn_slab_kernel)
    const int slab_mode = moca_tuning_get(MOCA_TUNE_GN_SLAB);   // 0: always the streaming path, 2: always the slab path (tests)
    const int cpg = C / GN_GROUPS;
    const int64_t bytes = (int64_t)F * HW * C * 2;
    const int64_t R64 = (int64_t)frames_per_stat * HW;
    if (slab_mode && cpg % 2 == 0 && cpg <= 128 && R64 < (1 << 24) &&
        (slab_mode == 2 || bytes <= (8 << 20) || (frames_per_stat == 1 && HW <= 160 && bytes <= (28 << 20)))) {
        // (measured on the bench workload, profiles/r01_plan_profile_*.txt: the slab kernel's 20..160-byte row segments
        //  lose to the streaming path's full-row reads as soon as the tensor is more than a few MB)
        pl.R = (int)R64;
        pl.n_slabs = (F / frames_per_stat) * GN_GROUPS;
        {   // slab in registers: <= 4096 chunks of 16 B, rows of >= 160 B ... or many rows
            const int nchunks = pl.R * (cpg / 8);
            if (cpg % 8 == 0 && nchunks <= 4096 && nchunks >= 256) {
                pl.cpt = (nchunks + 1023) / 1024;
                pl.threads = ((nchunks + pl.cpt - 1) / pl.cpt + 63) / 64 * 64;
                pl.route = MOCA_GN_ROUTE_SLABREG1 + pl.cpt - 1;
                return pl;
            }
        }
        int S = 1024 / pl.n_slabs;
        if (S > 16) S = 16;
        if (S > pl.R) S = pl.R;
        if (S < 1) S = 1;
        pl.S = S;
        pl.threads = 256;
        pl.route = cpg % 8 == 0 ? MOCA_GN_ROUTE_SLAB8 : cpg % 4 == 0 ? MOCA_GN_ROUTE_SLAB4 : MOCA_GN_ROUTE_SLAB2;
    }
    return pl;
}

const half_t* f16(const void* p) { return reinterpret_cast<const half_t*>(p); }
half_t* f16(void* p) { return reinterpret_cast<half_t*>(p); }
bool misaligned16(const void* a, const void* b) { return (reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15; }

}  // namespace

extern "C" int64_t moca_groupnorm_ws_bytes(int32_t F, int32_t HW, int32_t) {
    const int nchunk = gn_nchunk(F, HW);
    return ((int64_t)F * nchunk * GN_GROUPS * 2 + (int64_t)F * GN_GROUPS * 2) * 4;
}

extern "C" int moca_groupnorm_route(int32_t F, int32_t HW, int32_t C, int32_t frames_per_stat) {
    return gn_plan(F, HW, C, frames_per_stat).route;
}

extern "C" int moca_groupnorm_nchunk(int32_t F, int32_t HW) {
    if (F <= 0 || HW <= 0) return 0;
    return gn_nchunk(F, HW);
}

extern "C" int moca_groupnorm_nhwc_f16(const void* x, void* y, const float* gamma, const float* beta,
                                       int32_t F, int32_t HW, int32_t C, int32_t frames_per_stat,
                                       float eps, int32_t silu, float* ws, void* stream) {
    if (!x || !y || !gamma || !beta || !ws) return MOCA_E_BADARG;
    const gn_plan_t pl = gn_plan(F, HW, C, frames_per_stat);
    if (!pl.route) return MOCA_E_BADARG;
    const gn_stream_t& g = pl.geo;
    float* partial = ws;
    float* meanrstd = ws + (int64_t)F * g.nchunk * GN_GROUPS * 2;
    hipStream_t st = moca_stream(stream);
    const half_t* xi = f16(x);
    half_t* yo = f16(y);
    const int cpg = C / GN_GROUPS;
    if (pl.route >= MOCA_GN_ROUTE_SLABREG1 && pl.route <= MOCA_GN_ROUTE_SLABREG4) {
        decltype(&gn_slab_reg_kernel<1>) const reg[4] = {gn_slab_reg_kernel<1>, gn_slab_reg_kernel<2>, gn_slab_reg_kernel<3>, gn_slab_reg_kernel<4>};
        hipLaunchKernelGGL(reg[pl.cpt - 1], dim3(pl.n_slabs), dim3(pl.threads), 0, st, xi, yo, gamma, beta, pl.R, C, cpg, g.inv_count, eps, silu);
        MOCA_CHECK_LAUNCH();
        return MOCA_OK;
    }
    if (pl.route != MOCA_GN_ROUTE_STREAM) {
        const auto slab = pl.route == MOCA_GN_ROUTE_SLAB8 ? gn_slab_kernel<8> : pl.route == MOCA_GN_ROUTE_SLAB4 ? gn_slab_kernel<4> : gn_slab_kernel<2>;
        hipLaunchKernelGGL(slab, dim3(pl.n_slabs * pl.S), dim3(256), 0, st, xi, yo, gamma, beta, pl.R, C, cpg, pl.S, g.inv_count, eps, silu);
        MOCA_CHECK_LAUNCH();
        return MOCA_OK;
    }
    hipLaunchKernelGGL(gn_partial_kernel, g.grid, g.block, g.lds, st, xi, partial, HW, C, g.nchunk);
    MOCA_CHECK_LAUNCH();
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(F / frames_per_stat, GN_GROUPS), dim3(FIN_T), 0, st, partial, meanrstd,
                       frames_per_stat, g.nchunk, g.inv_count, eps);
    MOCA_CHECK_LAUNCH();
    hipLaunchKernelGGL(gn_apply_kernel, g.grid, g.block, 0, st, xi, yo, gamma, beta, meanrstd, HW, C, g.nchunk, frames_per_stat, silu);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_groupnorm_colsum_f16(const void* x, void* y, const float* gamma, const float* beta, const float* colsum,
                                         int32_t tile_rows, int32_t F, int32_t HW, int32_t C, int32_t frames_per_stat,
                                         float eps, int32_t silu, float* ws, void* stream) {
    if (!x || !y || !gamma || !beta || !ws || !colsum) return MOCA_E_BADARG;
    const gn_stream_t g = gn_stream(F, HW, C, frames_per_stat);
    if (!g.ok) return MOCA_E_BADARG;
    if (tile_rows <= 0 || ((int64_t)frames_per_stat * HW) % tile_rows) return MOCA_E_BADARG;   // a row tile must not straddle two statistics groups
    float* meanrstd = ws + (int64_t)F * g.nchunk * GN_GROUPS * 2;       // same workspace layout as the three-launch path
    hipStream_t st = moca_stream(stream);
    const int tps = (int)(((int64_t)frames_per_stat * HW) / tile_rows);   // row tiles per statistics group
    hipLaunchKernelGGL(gn_finalize_colsum_kernel, dim3(F / frames_per_stat, GN_GROUPS), dim3(FIN_T), 0, st, colsum, meanrstd,
                       tps, C, C / GN_GROUPS, g.inv_count, eps);
    MOCA_CHECK_LAUNCH();
    hipLaunchKernelGGL(gn_apply_kernel, g.grid, g.block, 0, st, f16(x), f16(y), gamma, beta, meanrstd, HW, C, g.nchunk, frames_per_stat, silu);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_groupnorm_gstat_f16(const void* x, void* y, const float* gamma, const float* beta, const int64_t* gstat,
                                        int32_t F, int32_t HW, int32_t C, int32_t frames_per_stat,
                                        float eps, int32_t silu, void* stream) {
    if (!x || !y || !gamma || !beta || !gstat) return MOCA_E_BADARG;
    if (misaligned16(gamma, beta)) return MOCA_E_BADARG;                  // (fetched as 16-byte vectors)
    const gn_stream_t g = gn_stream(F, HW, C, frames_per_stat);
    if (!g.ok) return MOCA_E_BADARG;
    if (g.nch8 * g.ppb < GN_GROUPS) return MOCA_E_BADARG;                 // (the first 32 threads of a block finish the statistics)
    hipLaunchKernelGGL(g.streams ? gn_apply_gstat_kernel<true> : gn_apply_gstat_kernel<false>, g.grid, g.block, 0, moca_stream(stream),
                       f16(x), f16(y), gamma, beta, gstat, HW, C, g.nchunk, frames_per_stat, g.inv_count, eps, silu);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_groupnorm_fold_weights_f16(const void* w, const float* bias, const float* gamma, const float* beta, const int64_t* gstat,
                                               void* wg, float* bg, int32_t n_sg, int32_t N, int32_t K, int32_t ldw, int64_t count, float eps,
                                               void* stream) {
    if (!w || !gamma || !beta || !gstat || !wg || !bg) return MOCA_E_BADARG;
    if (n_sg <= 0 || N <= 0 || K <= 0 || K % GN_GROUPS || K % 8 || ldw % 8 || ldw < K || count <= 0) return MOCA_E_BADARG;
    if (misaligned16(w, wg)) return MOCA_E_BADARG;
    const size_t lds = (size_t)(2 * K + 16 * (ldw / 8)) * sizeof(float);
    if (lds > 60 * 1024) return MOCA_E_BADARG;
    hipLaunchKernelGGL(gn_fold_weights_kernel, dim3(n_sg, (N + 15) / 16), dim3(256), lds, moca_stream(stream), f16(w), bias,
                       gamma, beta, gstat, f16(wg), bg, N, K, ldw, 1.0 / (double)count, eps);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_concat_channels_gstat_f16(const void* a, const void* b, void* out, int32_t F, int32_t HW, int32_t C1, int32_t C2,
                                              int32_t frames_per_stat, int64_t* gstat, void* stream) {
    if (!a || !b || !out || !gstat || C1 <= 0 || C2 <= 0 || C1 % 8 || C2 % 8) return MOCA_E_BADARG;
    const gn_stream_t g = gn_stream(F, HW, C1 + C2, frames_per_stat);
    if (!g.ok) return MOCA_E_BADARG;
    if (g.nch8 * g.ppb < 2 * GN_GROUPS) return MOCA_E_BADARG;             // (one thread per (group, sum / sum of squares) adds to gstat)
    if (g.lds > 64 * 1024) return MOCA_E_BADARG;
    hipLaunchKernelGGL(g.streams ? concat_gstat_kernel<true> : concat_gstat_kernel<false>, g.grid, g.block, g.lds, moca_stream(stream),
                       f16(a), f16(b), f16(out), gstat, HW, C1, C2, g.nchunk, frames_per_stat);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_groupnorm_gstat_cat_f16(const void* a, const void* b, void* y, const float* gamma, const float* beta,
                                            const int64_t* gstat_cat, const int64_t* gstat_b, int32_t Fb, int32_t F, int32_t HW, int32_t C1,
                                            int32_t C2, int32_t frames_per_stat, float eps, int32_t silu, void* stream) {
    if (!a || !b || !y || !gamma || !beta || !gstat_cat || C1 <= 0 || C2 <= 0 || C1 % 8 || C2 % 8) return MOCA_E_BADARG;
    if (misaligned16(gamma, beta)) return MOCA_E_BADARG;                  // (fetched as 16-byte vectors)
    const int C = C1 + C2;
    const gn_stream_t g = gn_stream(F, HW, C, frames_per_stat);
    if (!g.ok) return MOCA_E_BADARG;
    if (g.nch8 * g.ppb < GN_GROUPS) return MOCA_E_BADARG;
    if (Fb <= 0) Fb = F;
    if (Fb > F || F % Fb || Fb % frames_per_stat) return MOCA_E_BADARG;
    if (gstat_b) {                                                       // b's own groups must nest in the concat's
        const int cpg = C / GN_GROUPS, cpg2 = C2 / GN_GROUPS;
        if (C2 % GN_GROUPS || cpg % cpg2 || (C1 % cpg) % cpg2) return MOCA_E_BADARG;
    }
    hipLaunchKernelGGL(g.streams ? gn_apply_gstat_cat_kernel<true> : gn_apply_gstat_cat_kernel<false>, g.grid, g.block, 0, moca_stream(stream),
                       f16(a), f16(b), f16(y), gamma, beta, gstat_cat, gstat_b, HW, C1, C2, g.nchunk, frames_per_stat, Fb / frames_per_stat,
                       g.inv_count, eps, silu);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_gstat_accum_f16(const void* x, int32_t F, int32_t HW, int32_t C, int32_t frames_per_stat, int32_t cpg, int32_t coff,
                                    int64_t* gstat, void* stream) {
    if (!x || !gstat || cpg <= 0 || coff < 0) return MOCA_E_BADARG;
    const gn_stream_t g = gn_stream(F, HW, C, frames_per_stat, cpg);      // (no C % 32 rule: the source is a share of the normalised tensor)
    if (!g.ok) return MOCA_E_BADARG;
    const int g0 = coff / cpg, g1 = (coff + C - 1) / cpg;                 // the groups the source touches
    if (g1 >= GN_GROUPS || g.nch8 * g.ppb < 2 * (g1 - g0 + 1)) return MOCA_E_BADARG;
    if (g.lds > 64 * 1024) return MOCA_E_BADARG;
    hipLaunchKernelGGL(gstat_accum_kernel, g.grid, g.block, g.lds, moca_stream(stream), f16(x), gstat, HW, C, g.nchunk, frames_per_stat, cpg, coff);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_layernorm_f16(const void* x, void* y, const float* gamma, const float* beta,
                                  int32_t M, int32_t C, float eps, void* stream) {
    if (!x || !y || !gamma || !beta || M <= 0 || C <= 0 || C % 8) return MOCA_E_BADARG;
    if (misaligned16(x, y) || misaligned16(gamma, beta)) return MOCA_E_BADARG;   // (all four move as 16-byte vectors)
    // by 16-byte chunks of a row (<= 64 per chunk a lane holds): four rows per wave when there are enough rows to fill the chip, else one
    static const struct { int nch; decltype(&layernorm_kernel<1, 4>) many, few; } tab[] = {
        {64, layernorm_kernel<1, 4>, layernorm_kernel<1, 1>}, {128, layernorm_kernel<2, 4>, layernorm_kernel<2, 1>},
        {192, layernorm_kernel<3, 4>, layernorm_kernel<3, 1>}, {320, layernorm_kernel<5, 4>, layernorm_kernel<5, 1>}};
    const int rows = M >= 16384 ? 4 : 1;
    for (const auto& t : tab)
        if (C / 8 <= t.nch) {
            hipLaunchKernelGGL(rows == 4 ? t.many : t.few, dim3((M + 4 * rows - 1) / (4 * rows)), dim3(256), 0, moca_stream(stream), f16(x), f16(y),
                               gamma, beta, M, C, eps);
            MOCA_CHECK_LAUNCH();
            return MOCA_OK;
        }
    return MOCA_E_BADARG;
}
