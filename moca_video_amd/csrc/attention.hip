// Attention kernels for gfx950, head dim 64, fp16 I/O, fp32 softmax.
//
// moca_attention_f16: flash-style softmax(QK^T*scale)V for the spatial self / cross
//   attention (N = H*W up to 2560 queries; 77/154 context keys).  256 threads = 4
//   wavefronts x 32 query rows; K/V tiles of 64 keys double-buffered in LDS, both
//   row-major as they come from HBM (16-byte coalesced staging): K XOR-swizzled for the
//   ds_read_b128 fragment reads, V XOR-swizzled for ds_read_b64_tr_b16, the CDNA4
//   transposing LDS read that delivers the V^T operand of P.V without any data movement.
//   The score tile is computed "swapped" (S^T = K.Q^T with v_mfma_f32_32x32x16_f16) so
//   every lane owns ONE query column: the online-softmax row reduction is 31 in-lane
//   max/adds plus one lane<->lane+32 exchange, and the S^T accumulator registers are
//   directly the B operand of O^T += V^T.P^T (k order of the accumulator-as-operand
//   trick: key = 16s + 8(j>>2) + 4h + (j&3), matched by two 4-key transposed reads).
//   One barrier per key tile; the accumulator rescale is skipped (wave-uniform branch)
//   when no lane's running maximum moved.
//
// moca_temporal_attention_f16: attention over the frame axis (T <= 16) per
//   (pixel, head): one wavefront per problem with v_mfma_f32_16x16x32_f16 (QK^T) and
//   v_mfma_f32_16x16x16_f16 (PV); gathers the T frames of a pixel straight from the
//   channels-last token matrix, so the reference's (b t) c h w <-> (b h w) t c
//   reshuffles (attention.py:335-338,367) never touch memory.
//
// moca_temporal_attention_long_f16: the same over 17 <= T <= 32 frames: one wavefront per
//   problem, the 32 x 32 score tile of v_mfma_f32_32x32x16_f16 whose accumulator registers
//   are the B operand of P.V (tattn_long_kernel).
//
// Layout of this file: the LDS images and MFMA fragment maps that attention_kernel, attention_short_kernel, attention_v4_kernel and
// tattn_long_kernel share are written ONCE, in the first section below (k_img / v_img, score_key, load_q_frags, put_kv, pv_step,
// store_o_frags / put_o_tile, the temporal problem decode); the kernels only call them.  A change of an image or a map is a change there.
// temporal_attention_kernel (16 x 16 MFMAs, padded V rows) shares the problem decode only.  The entry points at the end share one
// argument check (attn_args_ok) and one launch list (launch_qkvo).
#include "common.h"
#include <stdlib.h>

namespace {

constexpr int D = 64;        // head dim
constexpr int KT = 64;       // keys per LDS tile
constexpr int QB = 128;      // queries per block
constexpr int ROWB = 128;    // bytes per LDS row (64 halves)

template <int V> struct int_c { static constexpr int value = V; };
typedef __attribute__((address_space(3))) char* lds_c_ptr;

// ---- LDS images and fragment maps of the 32 x 32 kernels -----------------------------------------------------------------
// A lane is (fr = lane & 31, fh = lane >> 5).  In S^T = K.Q^T (v_mfma_f32_32x32x16_f16, A = K, B = Q) it supplies K[key fr][16 ks +
// 8 fh + j] and Q[query fr][16 ks + 8 fh + j] and receives S^T[key = score_key(r, fh)][query fr] in accumulator register r.

// Byte offset of 16-byte chunk `ch` of row `row` in an image of 128-byte rows: the K image (and the per-wave Q / O tile) is swizzled
// for ds_read_b128 fragment reads down a column of chunks, the V image for the transposed reads (rows r and r + 8 keep their chunk).
__device__ __forceinline__ int k_chunk(int row, int ch) { return ch ^ ((row >> 1) & 7); }
__device__ __forceinline__ int v_chunk(int row, int ch) { return ch ^ (((row >> 1) & 1) << 2); }
__device__ __forceinline__ int k_img(int row, int ch) { return row * ROWB + (k_chunk(row, ch) << 4); }
__device__ __forceinline__ int v_img(int row, int ch) { return row * ROWB + (v_chunk(row, ch) << 4); }

// key, inside its 32-key sub-tile, of score register r of lane half fh
__device__ __forceinline__ int score_key(int r, int fh) { return (r & 3) + 8 * (r >> 2) + 4 * fh; }

// Q fragments (B operand of S^T = K.Q^T) of query row `qrow` from global memory: zero when the row does not exist
__device__ __forceinline__ void load_q_frags(half8v (&qf)[4], const half_t* qb, int qrow, int ldq, int fh, bool q_ok) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        half8v t = {0, 0, 0, 0, 0, 0, 0, 0};
        if (q_ok) t = *reinterpret_cast<const half8v*>(qb + (int64_t)qrow * ldq + ks * 16 + fh * 8);
        qf[ks] = t;
    }
}

// staging store of chunk `ch` of key row `row` into both images
__device__ __forceinline__ void put_kv(char* sK, char* sV, int row, int ch, half8v a, half8v b) {
    *reinterpret_cast<half8v*>(sK + k_img(row, ch)) = a;
    *reinterpret_cast<half8v*>(sV + v_img(row, ch)) = b;
}

// O^T += V^T . P^T over the 16 keys [key0, key0 + 16) of a V image (key0 a multiple of 16); pf = the 8 score registers of those keys,
// rounded to fp16.  The transposed read of a 16-lane group (lane i = 4 tq + tp) delivers to lane i the column d = 32 dt + 16 tcol16 + i
// of the 4 keys key0 + 4 fh + (0 .. 3); the second read is 8 keys further: together the key order of the accumulator-as-operand trick.
// pv_lane_offsets: the lane's two read addresses inside the first 16-key group, per-lane constants; a group further on, and the second
// read, only add whole rows (16 and 8 of them: v_chunk does not change), so the kernels' unrolled steps add immediates.
__device__ __forceinline__ void pv_lane_offsets(int (&v_off)[2], int lane) {
    const int fh = lane >> 5, tq = (lane & 15) >> 2, tp = lane & 3, tcol16 = (lane >> 4) & 1;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        const int dcol = dt * 32 + tcol16 * 16 + 4 * tp;     // first of this lane's 4 address columns
        v_off[dt] = v_img(4 * fh + tq, dcol >> 3) + (dcol & 7) * 2;
    }
}
__device__ __forceinline__ void pv_step(f32x16 (&o)[2], const char* vbuf, const int (&v_off)[2], int key0, half8v pf) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        const char* a0 = vbuf + v_off[dt] + key0 * ROWB;
        const half4v lo = lds_tr_read_b64(a0);
        const half4v hi = lds_tr_read_b64(a0 + 8 * ROWB);
        const half8v vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[dt], 0, 0, 0);
    }
}

// The lane holds O^T[d = 32 dt + 8 g + 4 fh + j][query fr] in o[dt][4 g + j]; o_frag: those four d, normalised and rounded.
__device__ __forceinline__ half4v o_frag(const f32x16 (&o)[2], float inv, int dt, int g) {
    half4v h4;
#pragma unroll
    for (int j = 0; j < 4; ++j) h4[j] = (half_t)(o[dt][g * 4 + j] * inv);
    return h4;
}
// 8-byte stores straight to the lane's output row (`orow` = its first element of this head)
__device__ __forceinline__ void store_o_frags(half_t* orow, const f32x16 (&o)[2], float inv, int fh) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<half4v*>(orow + dt * 32 + 8 * g + 4 * fh) = o_frag(o, inv, dt, g);
}
// Into the wave's own 32-row LDS tile `wq` (K image), from which whole 128-byte rows leave (8 lanes x 16 B) instead of one 8-byte piece
// of 32 different rows per instruction.  Each wave touches only its own tile: no block barrier.  (The copy-out loop stays in the two
// kernels: as a function it moves attention_short_kernel from 154 to 127 VGPRs with 16 instructions more per query group.)
__device__ __forceinline__ void put_o_tile(char* wq, const f32x16 (&o)[2], float inv, int lane) {
    const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d0 = dt * 32 + 8 * g + 4 * fh;
            *reinterpret_cast<half4v*>(wq + k_img(fr, d0 >> 3) + (d0 & 7) * 2) = o_frag(o, inv, dt, g);
        }
}

// The problem of a wave of the temporal kernels: (video, pixel, head) = blockIdx.x * 4 + wave.  Token row of frame t:
// (b T + t) HW + pix = row0 + t HW.  The waves past the last problem redo it and store nothing (`active`).
struct TemporalProblem {
    int head;
    int64_t row0;        // token row of frame 0
    int64_t rstride;     // elements between the q / k / v rows of consecutive frames
    int64_t base;        // element offset of frame 0's q / k / v row of this head
    bool active;
};
__device__ __forceinline__ TemporalProblem temporal_problem(int B, int T, int HW, int heads, int ld, int wave) {
    TemporalProblem p;
    const int64_t total = (int64_t)B * HW * heads;
    int64_t prob = (int64_t)blockIdx.x * 4 + wave;
    p.active = prob < total;
    if (!p.active) prob = total - 1;
    p.head = (int)(prob % heads);
    const int64_t bp = prob / heads;
    const int pix = (int)(bp % HW), b = (int)(bp / HW);
    p.row0 = (int64_t)b * T * HW + pix;
    p.rstride = (int64_t)HW * ld;
    p.base = p.row0 * ld + p.head * D;
    return p;
}

// XCD-aware block order: the hardware deals consecutive workgroup ids round-robin to the 8 XCDs (each with its own L2).  With
// the natural order the 20 query blocks of one (frame, head) land on all 8 XCDs and every L2 fetches that head's K and V from
// the fabric (rocprofv3 FETCH_SIZE: 2 GB per 2560-token launch, ~6 TB/s during the kernel).  Here all query blocks of a
// (frame, head) pair go to XCD (pair % 8), consecutive in time, so K/V cross the fabric once.
__device__ __forceinline__ void attn_block_coords(int& bx, int& by) {
    const int nx = gridDim.x, ny = gridDim.y;
    if (ny % 8 == 0) {
        const int b = blockIdx.y * nx + blockIdx.x;       // dispatch order
        const int xcd = b & 7, slot = b >> 3;
        by = (slot / nx) * 8 + xcd;
        bx = slot % nx;
    } else {
        bx = blockIdx.x; by = blockIdx.y;
    }
}

template <bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attention_kernel(
    const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, half_t* __restrict__ out,
    int heads, int Nq, int Nk, int ldq, int ldk, int ldv, int ldo, int kv_div, float scale_log2e) {
    // double-buffered K / V tiles, row-major [key][d]: the K image and the V image
    __shared__ __attribute__((aligned(16))) char sK[2][KT * ROWB];
    __shared__ __attribute__((aligned(16))) char sV[2][KT * ROWB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, by;
    attn_block_coords(bx, by);
    const int bq = by / heads, head = by % heads;
    const int bkv = bq / kv_div;
    const int q0 = bx * QB + wave * 32;
    const int fr = lane & 31, fh = lane >> 5;

    const half_t* qb = q + (int64_t)bq * Nq * ldq + head * D;
    const half_t* kb = k + (int64_t)bkv * Nk * ldk + head * D;
    const half_t* vb = v + (int64_t)bkv * Nk * ldv + head * D;

    half8v qf[4];
    const int qrow = q0 + fr;
    const bool q_ok = qrow < Nq;
    load_q_frags(qf, qb, qrow, ldq, fh, q_ok);

    f32x16 o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // staging coordinates: thread -> rows (tid>>3) + 32 i, chunk tid&7
    const int cc = tid & 7, r0 = tid >> 3;
    half8v rk[2], rv[2];
    auto load_kv = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = kt * KT + r0 + 32 * i;
            half8v a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
            if (key < Nk) {
                a = *reinterpret_cast<const half8v*>(kb + (int64_t)key * ldk + cc * 8);
                b = *reinterpret_cast<const half8v*>(vb + (int64_t)key * ldv + cc * 8);
            }
            rk[i] = a; rv[i] = b;
        }
    };
    auto store_kv = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) put_kv(sK[buf], sV[buf], r0 + 32 * i, cc, rk[i], rv[i]);
    };

    int v_off[2];
    pv_lane_offsets(v_off, lane);

    const int nkt = (Nk + KT - 1) / KT;
    load_kv(0);
    store_kv(0);
    if (nkt > 1) load_kv(1);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        // stage the next tile into the other buffer (its last readers passed the previous barrier),
        // then fetch the tile after it into registers: both overlap the MFMA/softmax work below
        if (kt + 1 < nkt) {
            store_kv(cur ^ 1);
            if (kt + 2 < nkt) load_kv(kt + 2);
        }
        const char* kbuf = sK[cur];
        const char* vbuf = sV[cur];

        // ---- S^T = K . Q^T ----
        f32x16 s[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[sub][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const half8v kf = *reinterpret_cast<const half8v*>(kbuf + k_img(sub * 32 + fr, ks * 2 + fh));
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s[sub], 0, 0, 0);
            }
        }
        // mask keys beyond Nk (last tile only); CAUSAL: also keys after this lane's query (text tower of the CLIP encoder)
        if (CAUSAL || (kt + 1) * KT > Nk) {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kt * KT + sub * 32 + score_key(r, fh);
                    if (key >= Nk || (CAUSAL && key > qrow)) s[sub][r] = -INFINITY;
                }
        }
        // ---- online softmax (this lane = one query column; partner lane^32 has the other keys) ----
        float tmax = s[0][0];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[sub][r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);
        const float mb = m_new * scale_log2e;
        float psum = 0.f;
        half8v pf[2][2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(s[sub][r] * scale_log2e - mb);
                psum += pv;
                pf[sub][r >> 3][r & 7] = (half_t)pv;
            }
        // rescale only when some lane's running max moved (wave-uniform branch; alpha == 1 otherwise)
        if (__any(m_new > m_run)) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2e);
            l_run *= alpha;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }
        l_run += psum;
        m_run = m_new;
        // ---- O^T += V^T . P^T ; V^T fragments by transposed LDS reads of the row-major V tile ----
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) pv_step(o, vbuf, v_off, sub * 32 + ss * 16, pf[sub][ss]);
        __syncthreads();   // everyone is done with buffers [cur]; the other buffers' stores are visible
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (q_ok) store_o_frags(out + ((int64_t)bq * Nq + qrow) * ldo + head * D, o, inv, fh);
}

// ---- cross-attention against a SHORT context (N_k <= 96: the 77 CLIP tokens): ONE key tile of 96 (three 32-key sub-tiles; the
// general kernel runs two 64-key tiles of which the second is 80 % padding, with an online-softmax step and a barrier in
// between), plain softmax (no running maximum), and K / V staged ONCE per block for `q_iters` consecutive 128-query groups
// (the general kernel re-stages them per 128 queries: 20 times per (frame, head) at 2560 tokens).
//
// IP (moca_attention_ip_f16, the img_cross_attention of attention.py:82-87,117-124): the tile holds TWO contexts, text keys from k / v
// in rows [0, Nt) and image keys from k_ip / v_ip in rows [IP_ROW0, IP_ROW0 + Ni) = [80, 96), and the block computes
//   softmax(q k^T s) v + ip_scale * softmax(q k_ip^T s) v_ip
// with two separate softmaxes: row maximum and row sum are taken per segment, and the image segment's P is multiplied by
// ip_scale * l_text / l_img before its fp16 conversion, so that the one P.V MFMA chain and the 1 / l_text epilogue finish both.
// The image rows start at a fixed multiple of 8: a lane's score register r of sub-tile `sub` holds key 32 sub + score_key(r, fh),
// so with the segment boundary on an 8-key group every register belongs to one segment at COMPILE time, the same for all
// lanes (a boundary at a runtime Nt costs a lane mask per register, 48 of them live across the softmax: SGPR spills).  Hence
// Nt <= 80 and Ni <= 16, which covers the reference's 77 text tokens + 16 (Resampler) or 4 (ImageProjModel) image tokens.
// (The IP = false instance ignores k_ip, v_ip, ldk_ip, ldv_ip, Nt and ip_scale; for IP = true, Nk = IP_ROW0 + Ni.)
constexpr int KS96 = 96;
constexpr int IP_ROW0 = 80;
template <bool IP>
__global__ __launch_bounds__(256, 2) void attention_short_kernel(
    const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, half_t* __restrict__ out,
    int heads, int Nq, int Nk, int ldq, int ldk, int ldv, int ldo, int kv_div, float scale_log2e, int q_iters,
    const half_t* __restrict__ k_ip, const half_t* __restrict__ v_ip, int ldk_ip, int ldv_ip, int Nt, float ip_scale) {
    __shared__ __attribute__((aligned(16))) char sK[KS96 * ROWB];
    __shared__ __attribute__((aligned(16))) char sV[KS96 * ROWB];
    // Q rows in / O rows out pass through a per-wave LDS tile (32 rows x 128 B, the K image): the global accesses are whole 128-byte
    // rows (8 lanes x 16 B) instead of one 16-byte / 8-byte piece of 32 different rows per instruction.  Each wave touches only its
    // own 32 rows, so no block barrier is needed inside the query loop.
    __shared__ __attribute__((aligned(16))) char sQ[QB * ROWB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, by;
    attn_block_coords(bx, by);
    const int bq = by / heads, head = by % heads;
    const int bkv = bq / kv_div;
    const int fr = lane & 31, fh = lane >> 5;
    const half_t* qb = q + (int64_t)bq * Nq * ldq + head * D;
    const int Ntx = IP ? Nt : Nk;                          // text keys per video (all of them unless IP)
    const half_t* kb = k + (int64_t)bkv * Ntx * ldk + head * D;
    const half_t* vb = v + (int64_t)bkv * Ntx * ldv + head * D;
    {   // stage K and V (rows >= Nk are zero; they are masked below); IP: rows [Nt, Nk) are the image tokens' k_ip / v_ip
        const int cc = tid & 7, r0 = tid >> 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int row = r0 + 32 * i;
            half8v a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
            if (row < Ntx) {
                a = *reinterpret_cast<const half8v*>(kb + (int64_t)row * ldk + cc * 8);
                b = *reinterpret_cast<const half8v*>(vb + (int64_t)row * ldv + cc * 8);
            } else if (IP && row >= IP_ROW0 && row < Nk) {
                const int Ni = Nk - IP_ROW0, ri = row - IP_ROW0;
                a = *reinterpret_cast<const half8v*>(k_ip + ((int64_t)bkv * Ni + ri) * ldk_ip + head * D + cc * 8);
                b = *reinterpret_cast<const half8v*>(v_ip + ((int64_t)bkv * Ni + ri) * ldv_ip + head * D + cc * 8);
            }
            put_kv(sK, sV, row, cc, a, b);
        }
    }
    __syncthreads();
    int v_off[2];
    pv_lane_offsets(v_off, lane);
    char* wq = sQ + wave * 32 * ROWB;
    half8v nq[4];                                          // the NEXT query group's rows travel while the current one is computed
    auto load_q = [&](int q0n) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {                      // 32 rows x 8 chunks = 256 chunks, 4 per lane, row-contiguous
            const int c = lane + 64 * i, row = c >> 3, ch = c & 7;
            half8v t = {0, 0, 0, 0, 0, 0, 0, 0};
            if (q0n + row < Nq) t = *reinterpret_cast<const half8v*>(qb + (int64_t)(q0n + row) * ldq + ch * 8);
            nq[i] = t;
        }
    };
    load_q(bx * q_iters * QB + wave * 32);
    for (int it = 0; it < q_iters; ++it) {
        const int q0 = (bx * q_iters + it) * QB + wave * 32;
        if (q0 >= Nq) break;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i, row = c >> 3, ch = c & 7;
            *reinterpret_cast<half8v*>(wq + k_img(row, ch)) = nq[i];
        }
        if (it + 1 < q_iters) load_q(q0 + QB);
        half8v qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const half8v*>(wq + k_img(fr, ks * 2 + fh));
        f32x16 s[3];
#pragma unroll
        for (int sub = 0; sub < 3; ++sub) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[sub][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const half8v kf = *reinterpret_cast<const half8v*>(sK + k_img(sub * 32 + fr, ks * 2 + fh));
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s[sub], 0, 0, 0);
            }
        }
        float tmax = -INFINITY;
        half8v pf[3][2];
        float inv;
        if constexpr (!IP) {
#pragma unroll
            for (int sub = 0; sub < 3; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = sub * 32 + score_key(r, fh);
                    if (key >= Nk) s[sub][r] = -INFINITY;
                    tmax = fmaxf(tmax, s[sub][r]);
                }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float mb = tmax * scale_log2e;
            float psum = 0.f;
#pragma unroll
            for (int sub = 0; sub < 3; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(s[sub][r] * scale_log2e - mb);
                    psum += pv;
                    pf[sub][r >> 3][r & 7] = (half_t)pv;
                }
            inv = 1.0f / (psum + __shfl_xor(psum, 32, 64));
        } else {
            // per-segment maxima: registers of sub-tiles 0, 1 and r < 8 of sub-tile 2 are text keys (< 80), the rest image keys
            float imax = -INFINITY;
#pragma unroll
            for (int sub = 0; sub < 3; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = sub * 32 + score_key(r, fh);
                    const bool txt = sub < 2 || r < 8;                       // compile time
                    if (txt ? key >= Nt : key >= Nk) s[sub][r] = -INFINITY;
                    if (txt) tmax = fmaxf(tmax, s[sub][r]);
                    else imax = fmaxf(imax, s[sub][r]);
                }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            imax = fmaxf(imax, __shfl_xor(imax, 32, 64));
            const float mb = tmax * scale_log2e, mbi = imax * scale_log2e;
            float psum = 0.f, isum = 0.f;
#pragma unroll
            for (int sub = 0; sub < 3; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool txt = sub < 2 || r < 8;
                    const float pv = __builtin_amdgcn_exp2f(s[sub][r] * scale_log2e - (txt ? mb : mbi));
                    if (txt) psum += pv;
                    else isum += pv;
                    s[sub][r] = pv;
                }
            const float lt = psum + __shfl_xor(psum, 32, 64), li = isum + __shfl_xor(isum, 32, 64);
            const float fi = ip_scale * lt / li;              // image P in units of the text row sum
#pragma unroll
            for (int sub = 0; sub < 3; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool txt = sub < 2 || r < 8;
                    pf[sub][r >> 3][r & 7] = (half_t)(txt ? s[sub][r] : s[sub][r] * fi);
                }
            inv = 1.0f / lt;
        }
        f32x16 o[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
        for (int sub = 0; sub < 3; ++sub)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) pv_step(o, sV, v_off, sub * 32 + ss * 16, pf[sub][ss]);
        // O rows leave through the wave's Q tile (the Q fragments are in registers), whole rows as they came in
        put_o_tile(wq, o, inv, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i, row = c >> 3, ch = c & 7;
            if (q0 + row < Nq)
                *reinterpret_cast<half8v*>(out + ((int64_t)bq * Nq + q0 + row) * ldo + head * D + ch * 8) =
                    *reinterpret_cast<const half8v*>(wq + k_img(row, ch));
        }
    }
}

// ---- "v4": the VALU-lean flash attention for long key sequences ---------------------------------------------------------
// rocprofv3 counters of attention_kernel at N = 2560 (tools/pmc_attn.sh): 222 VALU instructions per wave per 64-key tile,
// the VALU active in 61 % of all SIMD cycles, the matrix pipe in 30 % -- at head dim 64 the kernel is VALU-bound, so v4 removes
// vector instructions instead of re-arranging them.  Per score element the first-generation kernel spends
// fma (scale, - max) + exp + add (row sum) + 0.5 max3 + ~1.5 conversions + its share of zero-initialising the score
// accumulators and of LDS / global address arithmetic.  Here:
//   * Q is multiplied by scale*log2(e) once, when it is loaded (one fp16 rounding of Q more), and the running reference
//     maximum enters through the ACCUMULATOR INPUT of the first score MFMA (a 16-register operand holding -m_ref, rebuilt
//     only when m_ref moves): S'' = K.Q'^T - m_ref comes out of the matrix pipe ready for exp2 -- no fma, no zero fill;
//   * the reference maximum is lazy (cdna_hip_programming.md T13): it is moved (O, l rescaled) only when a tile maximum
//     exceeds it by more than THR = 8, i.e. P <= 2^8 in fp16, whose relative precision does not depend on magnitude; the
//     first tile always sets it;
//   * the row sums are v_dot2_f32_f16 of the PACKED P against (1, 1): 16 instructions per tile instead of 32 adds;
//   * P is packed with v_cvt_pk_f16_f32 only; LDS fragment addresses are per-lane constants + immediates (key loop
//     unrolled over the two buffers); the staging pointers advance by one 64-bit add per tile.
// What is left per element: 0.5 max3 + exp + 0.5 cvt_pk + 0.5 dot2.  121 VGPRs: four waves per SIMD.  Tiles, LDS images and fragment
// maps are those of attention_kernel (k_img / v_img, hoisted into per-lane constants here).
// Measured and not kept (the variants are no longer in the source):
//   * row sums from the matrix pipe (l^T += 1^T.P^T, one more MFMA per 16 keys): 5 % slower, the matrix pipe is the longer pole once the VALU work is cut;
//   * -m_ref living across the tile instead of 16 v_mov per tile: 141 instead of 121 VGPRs (three waves per SIMD), 3.5 % slower;
//   * without the zero-reference inline constant below: the 16 v_mov cost 64 of the tile's 960 issue-port cycles;
//   * 8 wavefronts (256 queries) per block: -2.8 % at 2560 tokens in isolation, -0.1 % on the whole step.
[[maybe_unused]] constexpr float LAZY_THR = 8.0f;
[[maybe_unused]] constexpr float REF0_BAND = 6.0f;     // first-tile maxima inside [-6, 6] (in log2 units) leave the reference at 0
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// NW = 4 wavefronts (32 queries each) share every K/V tile (the template parameter is part of the kernel's name in profiles and tools)
template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void attention_v4_kernel(
    const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, half_t* __restrict__ out,
    int heads, int Nq, int Nk, int ldq, int ldk, int ldv, int ldo, int kv_div, float scale_log2e) {
    static_assert(NW == 4 && 32 * NW == QB, "the DMA pieces and the per-wave output tiles below are laid out for four waves");
#if defined(__HIP_DEVICE_COMPILE__)   // (__amdgpu_buffer_rsrc_t is a device-only type; the host pass only needs the launch stub)
    __shared__ __attribute__((aligned(16))) char smem[4 * KT * ROWB];      // sK[0], sK[1], sV[0], sV[1]
    constexpr int TILE = KT * ROWB;                                       // 8 KiB
    char* const sK = smem;
    char* const sV = smem + 2 * TILE;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, by;
    attn_block_coords(bx, by);
    const int bq = by / heads, head = by % heads;
    const int bkv = bq / kv_div;
    const int q0 = bx * QB + wave * 32;
    const int fr = lane & 31, fh = lane >> 5;

    const half_t* qb = q + (int64_t)bq * Nq * ldq + head * D;
    // Q' = Q * scale * log2(e)
    half8v qf[4];
    load_q_frags(qf, qb, q0 + fr, ldq, fh, q0 + fr < Nq);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[ks][j] = (half_t)((float)qf[ks][j] * scale_log2e);

    f32x16 o[2];               // O^T accumulators
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    float m_ref = 0.f;
    bool ref_zero = true;      // (wave-uniform) no query of this wave has moved its reference off 0
    float lsum = 0.f;          // this lane's share of the row sum (its 32 of the 64 keys of every tile)

    // staging by LDS-DMA (buffer_load_dwordx4 ... lds: no staging registers, no ds_write): a 1 KiB piece = 8 key rows x 128 B,
    // lane -> row (lane >> 3), PHYSICAL chunk lane & 7; the swizzles of the two LDS images go on the per-lane SOURCE address
    // (logical chunk = physical ^ swizzle(row)).  Wave w moves pieces w and w + 4 of K and of V (rows 8w.., 32 + 8w..): 4 DMA
    // instructions per wave per key tile.  Rows >= Nk lie beyond num_records of the descriptors: the range check writes zeros.
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int lr = lane >> 3, pc = lane & 7;
    const int srow = wv * 8 + lr;                                          // + 32 for the second piece (same swizzles)
    const unsigned k_voff = (unsigned)(srow * ldk * 2 + (k_chunk(srow, pc) << 4));
    const unsigned v_voff = (unsigned)(srow * ldv * 2 + (v_chunk(srow, pc) << 4));
    const half_t* kbase = k + (int64_t)bkv * Nk * ldk + head * D;
    const half_t* vbase = v + (int64_t)bkv * Nk * ldv + head * D;
    const __amdgpu_buffer_rsrc_t rsrc_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(kbase), 0, (unsigned)(Nk * ldk * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(vbase), 0, (unsigned)(Nk * ldv * 2), 0x00020000);
    auto dma_k = [&](int kt, int buf) {
        const lds_c_ptr dk = (lds_c_ptr)sK + buf * TILE + wv * 1024;
        const unsigned ks0 = (unsigned)(kt * KT * ldk * 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_k, dk, 16, k_voff, ks0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_k, dk + 4096, 16, k_voff, ks0 + (unsigned)(32 * ldk * 2), 0, 0);
    };
    auto dma_v = [&](int kt, int buf) {
        const lds_c_ptr dv = (lds_c_ptr)sV + buf * TILE + wv * 1024;
        const unsigned vs0 = (unsigned)(kt * KT * ldv * 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_v, dv, 16, v_voff, vs0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_v, dv + 4096, 16, v_voff, vs0 + (unsigned)(32 * ldv * 2), 0, 0);
    };
    // fragment read offsets inside a tile: per-lane constants; (sub, ss, buffer) only add immediates
    int k_off[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) k_off[ks] = k_img(fr, ks * 2 + fh);       // + sub * 32 * ROWB
    int v_off[2];
    pv_lane_offsets(v_off, lane);
    const int nkt = (Nk + KT - 1) / KT;

    // scores of one key tile: S'' = K.Q'^T - m_ref (`acc0`, the accumulator input of the first MFMA of each chain, is -m_ref)
    auto qk = [&](const char* kbuf, f32x16 (&s)[2], const f32x16& acc0) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const half8v kf = *reinterpret_cast<const half8v*>(kbuf + k_off[ks] + sub * 32 * ROWB);
                s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], ks == 0 ? acc0 : s[sub], 0, 0, 0);
            }
    };
    // one key tile (K and V in slot B): scores, lazy reference, exp2/pack in four 16-key groups each followed by its 2 MFMAs
    // (two O tiles), so a group's MFMAs run under the next group's exp2
    auto tile = [&](auto b_tag, f32x16 (&sc)[2], int kt) {
        constexpr int VB = decltype(b_tag)::value;
        // While the reference of every query of the wave is still 0 (`ref_zero`, wave-uniform) the score MFMAs take the inline constant 0
        // as their accumulator input and the 16 v_mov that rebuild the -m_ref operand per tile are not executed.  The reference starts
        // at 0 unless the first tile's maximum lies outside [-REF0_BAND, REF0_BAND] (then it is that maximum) and moves when a tile
        // maximum exceeds it by more than LAZY_THR: P <= 2^8 and the row's largest P >= 2^-REF0_BAND either way.
        if (ref_zero) {
            const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            qk(sK + VB * TILE, sc, zero16);
        } else {
            f32x16 negm;                              // -m_ref replicated, rebuilt per tile
#pragma unroll
            for (int r = 0; r < 16; ++r) negm[r] = -m_ref;
            qk(sK + VB * TILE, sc, negm);
        }
        if ((kt + 1) * KT > Nk) {                     // keys beyond Nk (last tile only)
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kt * KT + sub * 32 + score_key(r, fh);
                    if (key >= Nk) sc[sub][r] = -INFINITY;
                }
        }
        // tile maximum as four independent chains of v_max3_f32.  As instructions, not fmaxf: on accumulator outputs the compiler puts a
        // canonicalising v_max_f32 x, x in front of every fmaxf operand (47 vector instructions for these 32 values instead of 18 -- a
        // fifth of the key tile's vector issue, which is the longer pole of this kernel).  Scores are finite or -inf, never NaN.
        float t4[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            t4[c] = vmax3(sc[0][c], sc[1][c], sc[0][4 + c]);
            t4[c] = vmax3(t4[c], sc[1][4 + c], sc[0][8 + c]);
            t4[c] = vmax3(t4[c], sc[1][8 + c], sc[0][12 + c]);
            t4[c] = vmax3(t4[c], sc[1][12 + c], sc[1][12 + c]);
        }
        float tmax = vmax3(vmax3(t4[0], t4[1], t4[2]), t4[3], t4[3]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));      // both key halves of this query: the two lanes agree from here on
        if (kt == 0 || __any(tmax > LAZY_THR)) {      // move the reference (first tile: to its maximum unless that lies in the zero band)
            const float delta = kt == 0 ? (fabsf(tmax) > REF0_BAND ? tmax : 0.f) : fmaxf(tmax, 0.f);
            const float alpha = __builtin_amdgcn_exp2f(-delta);          // (kt == 0: O and l are still zero)
            m_ref += delta;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                o[0][r] *= alpha; o[1][r] *= alpha;
                if (r == 0) lsum *= alpha;
                sc[0][r] -= delta; sc[1][r] -= delta;
            }
            ref_zero = !__any(m_ref != 0.f);
        }
        const char* vbuf = sV + VB * TILE;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                half2v h[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p0 = __builtin_amdgcn_exp2f(sc[sub][ss * 8 + 2 * j]);
                    const float p1 = __builtin_amdgcn_exp2f(sc[sub][ss * 8 + 2 * j + 1]);
                    h[j] = __builtin_convertvector(f32x2{p0, p1}, half2v);
                }
                const half4v plo = __builtin_shufflevector(h[0], h[1], 0, 1, 2, 3);
                const half4v phi = __builtin_shufflevector(h[2], h[3], 0, 1, 2, 3);
                const half8v pf = __builtin_shufflevector(plo, phi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int j = 0; j < 4; ++j) lsum = __builtin_amdgcn_fdot2(h[j], half2v{(half_t)1.0f, (half_t)1.0f}, lsum, false);
                pv_step(o, vbuf, v_off, sub * 32 + ss * 16, pf);
            }
    };

    // tile kt+1 is fetched while tile kt is computed: DMA issued after the barrier that retired the buffer's last readers,
    // awaited (vmcnt(0): a whole tile of compute later) before the barrier that publishes it.  (A software-pipelined variant
    // -- scores of tile kt+1 issued under the softmax of tile kt, `step(...)` with two score register sets -- needs 196 VGPRs =
    // two waves per SIMD and measured 446 us against 401 us for this form at 157 VGPRs = three waves per SIMD: occupancy wins.)
    f32x16 sa[2];
    dma_k(0, 0); dma_v(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < nkt; kt += 2) {
        if (kt + 1 < nkt) { dma_k(kt + 1, 1); dma_v(kt + 1, 1); }
        tile(int_c<0>{}, sa, kt);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + 1 < nkt) {
            if (kt + 2 < nkt) { dma_k(kt + 2, 0); dma_v(kt + 2, 0); }
            tile(int_c<1>{}, sa, kt + 1);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    }

    const float inv = 1.0f / (lsum + __shfl_xor(lsum, 32, 64));
    // O rows leave as whole 128-byte rows through the (now free) K/V buffers: wave w owns 4 KiB at smem + 4096 w (the last
    // barrier of the key loop retired every fragment read; each wave touches only its own 32 rows, so no further barrier)
    {
        char* wq = smem + wave * 32 * ROWB;
        put_o_tile(wq, o, inv, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i, row = c >> 3, ch = c & 7;
            if (q0 + row < Nq)
                *reinterpret_cast<half8v*>(out + ((int64_t)bq * Nq + q0 + row) * ldo + head * D + ch * 8) =
                    *reinterpret_cast<const half8v*>(wq + k_img(row, ch));
        }
    }
#endif
}

// ---- temporal attention: one wavefront per (video, pixel, head), T <= 16 -------
constexpr int TV_ROWB = 144;  // 128 B + 16 B pad per V row in LDS

// CAUSAL (TemporalTransformer(causal_attention=True): attention.py:309-311,342-346 -> :101-105): a frame attends to itself and
// earlier frames only.  In the S^T register layout a key above the query gets -inf BEFORE the row maximum; the diagonal is never
// masked, so the maximum is finite and exp2f(-inf) = 0 exactly -- the values of masked_fill_(-finfo.max) followed by softmax.
template <bool CAUSAL>
__global__ __launch_bounds__(256) void temporal_attention_kernel(
    const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, half_t* __restrict__ out,
    int B, int T, int HW, int heads, int ld, int ldo, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) char sV[4][16 * TV_ROWB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TemporalProblem p = temporal_problem(B, T, HW, heads, ld, wave);
    const int64_t rstride = p.rstride, base = p.base;

    const int fr = lane & 15, fg = lane >> 4;
    // K (A operand) and Q (B operand) fragments of S^T = K.Q^T: row fr, d = 32 ks + 8 fg + j
    half8v kf[2], qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        half8v a = {0, 0, 0, 0, 0, 0, 0, 0}, c = {0, 0, 0, 0, 0, 0, 0, 0};
        if (fr < T) {
            a = *reinterpret_cast<const half8v*>(k + base + fr * rstride + ks * 32 + fg * 8);
            c = *reinterpret_cast<const half8v*>(q + base + fr * rstride + ks * 32 + fg * 8);
        }
        kf[ks] = a; qf[ks] = c;
    }
    // V -> LDS row-major [key][d], padded rows (no swizzle: the 16 x 16 P.V reads single halves)
    char* sv = sV[wave];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (lane >> 3) + 8 * i, ch = lane & 7;
        half8v a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < T) a = *reinterpret_cast<const half8v*>(v + base + row * rstride + ch * 8);
        *reinterpret_cast<half8v*>(sv + row * TV_ROWB + ch * 16) = a;
    }
    __syncthreads();

    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    s = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[0], qf[0], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[1], qf[1], s, 0, 0, 0);
    // lane holds S^T[key = 4 fg + r][q = fr]
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (4 * fg + r >= T) s[r] = -INFINITY;
        if (CAUSAL && 4 * fg + r > fr) s[r] = -INFINITY;
        mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
    half4v pf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float pv = exp2f((s[r] - mx) * scale_log2e);
        sum += pv;
        pf[r] = (half_t)pv;
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;

    // O^T[d][q] = V^T[d][key] . P^T[key][q]; A: lane (d = fr, k = 4 fg + j) = V[4fg+j][16dt + fr]
    const bool st_ok = p.active && fr < T;
    half_t* ob = out + (p.row0 + (int64_t)fr * HW) * ldo + p.head * D;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        half4v vf;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            vf[j] = *reinterpret_cast<const half_t*>(sv + (4 * fg + j) * TV_ROWB + (dt * 16 + fr) * 2);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf, acc, 0, 0, 0);
        // lane holds O^T[d = 16dt + 4fg + r][q = fr]
        if (st_ok) {
            half4v h4;
#pragma unroll
            for (int r = 0; r < 4; ++r) h4[r] = (half_t)(acc[r] * inv);
            *reinterpret_cast<half4v*>(ob + dt * 16 + 4 * fg) = h4;
        }
    }
}

// ---- temporal attention over 17 .. 32 frames: one wavefront per (video, pixel, head) -------
// The 32 frames of a pixel are one 32 x 32 score tile.  S^T = K.Q^T by four v_mfma_f32_32x32x16_f16 over d = 64: the lane
// (r = lane & 31, h = lane >> 5) then holds S^T[key = score_key(reg, h)][query = r], i.e. the key index lies in its 16
// registers and the query on the lane -- the softmax over keys is 15 in-lane max / adds and one exchange with lane ^ 32.  Registers
// 8s .. 8s+7, rounded to fp16 once, ARE the B operand of k-step s of O^T = V^T.P^T (element j = key 16s + 8(j>>2) + 4h + (j&3)); the A
// operand takes V in that same key order by two transposing 4-key LDS reads of the row-major V image (pv_step).
// Keys >= T get -inf before the row maximum, with CAUSAL keys above the query too (attention.py:101-105); the diagonal is never
// masked and T >= 17 > 4h + 3, so every lane's maximum is finite.  Rows t >= T are neither loaded (zero fragments) nor stored.
// No atomics, fixed order of every sum: replays are bit-identical.
constexpr int TL_T = 32;     // frames of the tile
template <bool CAUSAL>
__global__ __launch_bounds__(256) void tattn_long_kernel(
    const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, half_t* __restrict__ out,
    int B, int T, int HW, int heads, int ld, int ldo, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) char sV[4][TL_T * ROWB];          // one V image per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TemporalProblem p = temporal_problem(B, T, HW, heads, ld, wave);
    const int64_t rstride = p.rstride, base = p.base;

    const int fr = lane & 31, fh = lane >> 5;
    // K (A operand) and Q (B operand) fragments of S^T = K.Q^T: row fr, d = 16 ks + 8 fh + j
    half8v kf[4], qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        half8v a = {0, 0, 0, 0, 0, 0, 0, 0}, c = {0, 0, 0, 0, 0, 0, 0, 0};
        if (fr < T) {
            a = *reinterpret_cast<const half8v*>(k + base + fr * rstride + ks * 16 + fh * 8);
            c = *reinterpret_cast<const half8v*>(q + base + fr * rstride + ks * 16 + fh * 8);
        }
        kf[ks] = a; qf[ks] = c;
    }
    // V -> LDS: lane -> rows (lane >> 3) + 8 i, 16-byte chunk lane & 7; rows >= T are zero (their P is zero: 0 * 0, never 0 * garbage)
    char* sv = sV[wave];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (lane >> 3) + 8 * i, ch = lane & 7;
        half8v a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < T) a = *reinterpret_cast<const half8v*>(v + base + row * rstride + ch * 8);
        *reinterpret_cast<half8v*>(sv + v_img(row, ch)) = a;
    }
    __syncthreads();

    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qf[ks], s, 0, 0, 0);
    // the last key this lane's query sees is T - 1, with CAUSAL min(T - 1, fr); taken relative to the lane half's first key, so that
    // the mask is ONE comparison per register in both instantiations
    const int last = (CAUSAL ? min(T - 1, fr) : T - 1) - score_key(0, fh);
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (score_key(r, 0) > last) s[r] = -INFINITY;
        mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
    half8v pf[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        // (a masked key is zero whatever the sign of the scale: the tail keys are masked in the non-causal form too)
        const float pv = score_key(r, 0) > last ? 0.f : exp2f((s[r] - mx) * scale_log2e);
        sum += pv;
        pf[r >> 3][r & 7] = (half_t)pv;
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;

    int v_off[2];
    pv_lane_offsets(v_off, lane);
    f32x16 o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) pv_step(o, sv, v_off, ss * 16, pf[ss]);
    if (p.active && fr < T) store_o_frags(out + (p.row0 + (int64_t)fr * HW) * ldo + p.head * D, o, inv, fh);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
constexpr float LOG2E = 1.4426950408889634f;      // the kernels take scale * log2(e): their exponentials are exp2

inline bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

// The checks every entry shares, following the widest access a kernel makes on an operand.  `in`: q, k, v (and k_ip, v_ip) with
// their leading dimensions, read by 16-byte loads / LDS-DMA everywhere: 16-byte aligned, ld % 8.  `out` is stored in pieces of
// `store_bytes`: 16 (whole 16-byte pieces of a row: the short and the long-key kernel, so every route of moca_attention_f16) or 8 (one
// lane's four halves: attention_kernel alone, the temporal kernels), i.e. ldo % 8 or ldo % 4.  `grid_y`: blocks along y (65535 at most).
struct AttnOperand { const void* p; int ld; };
template <size_t N>
bool attn_args_ok(const AttnOperand (&in)[N], const void* out, int ldo, int store_bytes, int heads, int64_t grid_y) {
    if (heads <= 0 || !out || misaligned(out, store_bytes) || ldo % (store_bytes / 2) || ldo < heads * D) return false;
    for (const AttnOperand& a : in)
        if (!a.p || misaligned(a.p, 16) || a.ld % 8 || a.ld < heads * D) return false;
    return grid_y <= 65535;
}

// the launch list every kernel starts with: 256 threads, q, k, v, out as halves, then the kernel's own arguments
template <class Kernel, class... Args>
void launch_qkvo(Kernel kernel, dim3 grid, void* stream, const void* q, const void* k, const void* v, void* out, Args... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, moca_stream(stream), reinterpret_cast<const half_t*>(q), reinterpret_cast<const half_t*>(k),
                       reinterpret_cast<const half_t*>(v), reinterpret_cast<half_t*>(out), args...);
}

template <bool IP>
void launch_short(const void* q, const void* k, const void* v, const void* k_ip, const void* v_ip, void* out, int Bq, int heads, int Nq,
                  int Nt, int Nk, int ldq, int ldk, int ldv, int ldk_ip, int ldv_ip, int ldo, int kv_div, float scale, float ip_scale,
                  void* stream) {
    // query groups of 128 per block: as many as keep >= ~3 blocks per CU in the launch (K / V are staged once per block)
    const int qgroups = (Nq + QB - 1) / QB;
    int q_iters = (int)(((int64_t)qgroups * Bq * heads) / 768);
    if (q_iters < 1) q_iters = 1;
    if (q_iters > 8) q_iters = 8;
    if (q_iters > qgroups) q_iters = qgroups;
    launch_qkvo(attention_short_kernel<IP>, dim3((qgroups + q_iters - 1) / q_iters, Bq * heads), stream, q, k, v, out,
                heads, Nq, Nk, ldq, ldk, ldv, ldo, kv_div, scale * LOG2E, q_iters,
                reinterpret_cast<const half_t*>(k_ip), reinterpret_cast<const half_t*>(v_ip), ldk_ip, ldv_ip, Nt, ip_scale);
}

// The three temporal entries: frame counts [t_min, t_max] go to `kernel` (one wave per problem, four per block).  `grid_check`:
// refuse a launch of more than INT32_MAX blocks (the long entry; the T <= 16 entries never have).
typedef void (*temporal_kernel_t)(const half_t*, const half_t*, const half_t*, half_t*, int, int, int, int, int, int, float);
int launch_temporal(temporal_kernel_t kernel, int t_min, int t_max, bool grid_check, const void* q, const void* k, const void* v, void* out,
                    int32_t B, int32_t T, int32_t HW, int32_t heads, int32_t ld_qkv, int32_t ldo, float scale, void* stream) {
    if (B <= 0 || T < t_min || T > t_max || HW <= 0) return MOCA_E_BADARG;
    if (!attn_args_ok({{q, ld_qkv}, {k, ld_qkv}, {v, ld_qkv}}, out, ldo, 8, heads, 1)) return MOCA_E_BADARG;
    const int64_t total = (int64_t)B * HW * heads;
    if (grid_check && (total + 3) / 4 > INT32_MAX) return MOCA_E_BADARG;
    launch_qkvo(kernel, dim3((unsigned)((total + 3) / 4)), stream, q, k, v, out, B, T, HW, heads, ld_qkv, ldo, scale * LOG2E);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

}  // namespace

extern "C" int moca_attention_f16(const void* q, const void* k, const void* v, void* out,
                                  int32_t Bq, int32_t heads, int32_t Nq, int32_t Nk,
                                  int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                                  int32_t kv_div, float scale, void* stream) {
    if (Bq <= 0 || heads <= 0 || Nq <= 0 || Nk <= 0 || kv_div <= 0 || Bq % kv_div) return MOCA_E_BADARG;
    if (!attn_args_ok({{q, ldq}, {k, ldk}, {v, ldv}}, out, ldo, 16, heads, (int64_t)Bq * heads)) return MOCA_E_BADARG;
    // the long-key kernel addresses K and V of one video by 32-bit byte offsets (buffer descriptor, whole 64-key tiles)
    if (((int64_t)Nk + KT - 1) / KT * KT * (ldk > ldv ? ldk : ldv) * 2 > INT32_MAX) return MOCA_E_BADARG;
    const dim3 grid((Nq + QB - 1) / QB, Bq * heads);
    if (Nk >= 2 * KT)
        launch_qkvo(attention_v4_kernel<4>, grid, stream, q, k, v, out, heads, Nq, Nk, ldq, ldk, ldv, ldo, kv_div, scale * LOG2E);
    else if (Nk <= KS96)
        launch_short<false>(q, k, v, nullptr, nullptr, out, Bq, heads, Nq, Nk, Nk, ldq, ldk, ldv, 0, 0, ldo, kv_div, scale, 0.f, stream);
    else
        launch_qkvo(attention_kernel<false>, grid, stream, q, k, v, out, heads, Nq, Nk, ldq, ldk, ldv, ldo, kv_div, scale * LOG2E);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_attention_ip_f16(const void* q, const void* k, const void* v, const void* k_ip, const void* v_ip, void* out,
                                     int32_t Bq, int32_t heads, int32_t Nq, int32_t Nt, int32_t Ni,
                                     int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldk_ip, int32_t ldv_ip, int32_t ldo,
                                     int32_t kv_div, float scale, float ip_scale, void* stream) {
    if (Bq <= 0 || heads <= 0 || Nq <= 0 || Nt < 1 || Ni < 0 || Nt + Ni > KS96 || kv_div <= 0 || Bq % kv_div) return MOCA_E_BADARG;
    if (Ni > 0 && (Nt > IP_ROW0 || Ni > KS96 - IP_ROW0)) return MOCA_E_BADARG;     // the fixed text / image rows of the tile
    if (!attn_args_ok({{q, ldq}, {k, ldk}, {v, ldv}, {k_ip, ldk_ip}, {v_ip, ldv_ip}}, out, ldo, 16, heads, (int64_t)Bq * heads))
        return MOCA_E_BADARG;
    // |ip_scale| <= 64: the scaled image P (<= ip_scale * l_text <= 64 * 80) stays far inside the fp16 range; rejects inf and NaN too
    if (!(fabsf(ip_scale) <= 64.f)) return MOCA_E_BADARG;
    if (Ni == 0)   // no image tokens (a 77-token context): exactly moca_attention_f16's launch, bit for bit
        launch_short<false>(q, k, v, nullptr, nullptr, out, Bq, heads, Nq, Nt, Nt, ldq, ldk, ldv, 0, 0, ldo, kv_div, scale, 0.f, stream);
    else
        launch_short<true>(q, k, v, k_ip, v_ip, out, Bq, heads, Nq, Nt, IP_ROW0 + Ni, ldq, ldk, ldv, ldk_ip, ldv_ip, ldo, kv_div, scale,
                           ip_scale, stream);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_attention_causal_f16(const void* q, const void* k, const void* v, void* out,
                                         int32_t B, int32_t heads, int32_t N, int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                                         float scale, void* stream) {
    if (B <= 0 || heads <= 0 || N <= 0) return MOCA_E_BADARG;
    if (!attn_args_ok({{q, ldq}, {k, ldk}, {v, ldv}}, out, ldo, 8, heads, (int64_t)B * heads)) return MOCA_E_BADARG;
    launch_qkvo(attention_kernel<true>, dim3((N + QB - 1) / QB, B * heads), stream, q, k, v, out, heads, N, N, ldq, ldk, ldv, ldo, 1,
                scale * LOG2E);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_temporal_attention_f16(const void* q, const void* k, const void* v, void* out,
                                           int32_t B, int32_t T, int32_t HW, int32_t heads,
                                           int32_t ld_qkv, int32_t ldo, float scale, void* stream) {
    return launch_temporal(temporal_attention_kernel<false>, 1, 16, false, q, k, v, out, B, T, HW, heads, ld_qkv, ldo, scale, stream);
}

extern "C" int moca_temporal_attention_causal_f16(const void* q, const void* k, const void* v, void* out,
                                                  int32_t B, int32_t T, int32_t HW, int32_t heads,
                                                  int32_t ld_qkv, int32_t ldo, float scale, void* stream) {
    if (!(scale > 0.f)) return MOCA_E_BADARG;          // (the mask is applied before the scale: -inf must stay -inf)
    return launch_temporal(temporal_attention_kernel<true>, 1, 16, false, q, k, v, out, B, T, HW, heads, ld_qkv, ldo, scale, stream);
}

// 17 <= T <= 32 (T <= 16 stays with the two entries above: one kernel per frame count, and their bits do not move)
extern "C" int moca_temporal_attention_long_f16(const void* q, const void* k, const void* v, void* out,
                                                int32_t B, int32_t T, int32_t HW, int32_t heads,
                                                int32_t ld_qkv, int32_t ldo, float scale, int32_t causal, void* stream) {
    if (causal != 0 && causal != 1) return MOCA_E_BADARG;
    if (causal && !(scale > 0.f)) return MOCA_E_BADARG;          // (the mask is applied before the scale: -inf must stay -inf)
    return launch_temporal(causal ? tattn_long_kernel<true> : tattn_long_kernel<false>, 17, TL_T, true, q, k, v, out, B, T, HW, heads, ld_qkv,
                           ldo, scale, stream);
}
