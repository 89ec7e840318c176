// Kernels of the OpenCLIP ViT-H/14 vision tower (the image embedder of the i2v model, moca_video_amd/clip_vision.py).  The
// transformer blocks run on the library's LayerNorm and GEMM kernels; what is new here is the part those do not cover:
//
// moca_attention_d80_f16: non-causal self-attention with head dim 80 (1280 / 16) over one image's tokens (N = 257).  Block =
//   4 waves x 16 queries; K/V tiles of 64 keys staged in LDS (row-major, 176-byte rows), the next tile's global loads in flight
//   under the current tile's MFMAs.  The score tile is computed swapped, S^T = K.Q^T with v_mfma_f32_16x16x32_f16 (3 k-steps,
//   the third zero-padded from d 80 to 96), so that every lane owns one query column: the online softmax reduces 4 in-lane values
//   per key sub-tile and two lane-group exchanges, and the S^T accumulator registers are directly the B operand of
//   O^T += V^T.P^T (v_mfma_f32_16x16x16_f16, 5 d-tiles of 16), whose A operand comes from ds_read_b64_tr_b16 on the row-major V
//   tile.  O^T has the query on the lane too, so the rescale by exp(m_old - m_new) is in-lane.
//   Registers: <= 128 VGPR + AGPR (four waves per SIMD at least; asserted by tests/test_clip_vision_cpu.py), no scratch.
//
// moca_clip_preprocess_patches_f16: FrozenOpenCLIPImageEmbedder(V2).preprocess (condition.py:355-363: kornia resize to 224 x 224,
//   bicubic, align_corners, antialias; (x + 1) / 2; CLIP mean / std) fused with the patchify of conv1, writing the patch GEMM's
//   A operand [B * 256][ldo] fp16 in conv1's (c, ky, kx) order, zero columns up to ldo.  One thread per output element.
//
// moca_clip_assemble_tokens_f16: [class token; patch tokens] + positional embedding (open_clip VisionTransformer.forward), fp16.
#include "common.h"
#include <math.h>

namespace {

constexpr int D80 = 80;            // head dim
constexpr int A80_KT = 64;         // keys per LDS tile
constexpr int A80_QW = 16;         // queries per wave
constexpr int A80_QB = 64;         // queries per block (4 waves)
constexpr int A80_ROWB = 176;      // bytes per LDS row: 160 B of data + 16 B pad (16-byte aligned rows, staggered banks)
constexpr int A80_CH = D80 / 8;    // 16-byte chunks per row
constexpr int A80_PIECES = 2 * A80_KT * A80_CH / 256;   // 16-byte K and V pieces per thread and tile (5)

__global__ __launch_bounds__(256, 4) void clip_attention_d80_kernel(
    const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, half_t* __restrict__ out,
    int heads, int N, int ldq, int ldk, int ldv, int ldo, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) char sK[A80_KT * A80_ROWB];
    __shared__ __attribute__((aligned(16))) char sV[A80_KT * A80_ROWB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y / heads, head = blockIdx.y % heads;
    const int fr = lane & 15, fg = lane >> 4;
    const half_t* qb = q + (int64_t)b * N * ldq + head * D80;
    const half_t* kb = k + (int64_t)b * N * ldk + head * D80;
    const half_t* vb = v + (int64_t)b * N * ldv + head * D80;
    const half8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // Q fragments (B operand of S^T = K.Q^T, 16x16x32): lane (q = fr, g = fg) holds Q[q][32 ks + 8 g + j]; d >= 80 and rows >= N are 0
    const int qrow = blockIdx.x * A80_QB + wave * A80_QW + fr;
    half8v qf[3];
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
        const int d = 32 * ks + 8 * fg;
        half8v t = zero8;
        if (qrow < N && d < D80) t = *reinterpret_cast<const half8v*>(qb + (int64_t)qrow * ldq + d);
        qf[ks] = t;
    }

    // staging: piece e = tid + 256 i of the tile's 2 x 64 x 10 16-byte pieces (K first, then V); keys >= N are zero-filled, so that
    // their P = 0 never meets a non-finite V
    half8v st[A80_PIECES];
    auto load_kv = [&](int kt) {
#pragma unroll
        for (int i = 0; i < A80_PIECES; ++i) {
            const int e = tid + 256 * i;
            const bool isv = e >= A80_KT * A80_CH;
            const int ee = isv ? e - A80_KT * A80_CH : e;
            const int key = kt * A80_KT + ee / A80_CH, ch = ee % A80_CH;
            half8v a = zero8;
            if (key < N) a = isv ? *reinterpret_cast<const half8v*>(vb + (int64_t)key * ldv + ch * 8)
                                 : *reinterpret_cast<const half8v*>(kb + (int64_t)key * ldk + ch * 8);
            st[i] = a;
        }
    };
    auto store_kv = [&]() {
#pragma unroll
        for (int i = 0; i < A80_PIECES; ++i) {
            const int e = tid + 256 * i;
            const bool isv = e >= A80_KT * A80_CH;
            const int ee = isv ? e - A80_KT * A80_CH : e;
            char* dst = (isv ? sV : sK) + (ee / A80_CH) * A80_ROWB + (ee % A80_CH) * 16;
            *reinterpret_cast<half8v*>(dst) = st[i];
        }
    };

    f32x4 o[5];
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    const int nkt = (N + A80_KT - 1) / A80_KT;
    load_kv(0);
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt) __syncthreads();                 // every wave is done with the previous tile
        store_kv();
        __syncthreads();
        if (kt + 1 < nkt) load_kv(kt + 1);       // in flight under this tile's MFMAs

        // S^T[key 16t + 4g + r][q = fr] for the 4 key sub-tiles; A operand: lane (key = fr, g) holds K[key][32 ks + 8 g + j]
        f32x4 s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const char* kr = sK + (16 * t + fr) * A80_ROWB;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) {
                const int d = 32 * ks + 8 * fg;
                const half8v a = d < D80 ? *reinterpret_cast<const half8v*>(kr + d * 2) : zero8;   // (the row pad is not initialised)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[ks], acc, 0, 0, 0);
            }
            s[t] = acc;
        }
        // online softmax over this tile's keys, logits in log2 units; keys >= N are -inf before the maximum
        float tmax = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * A80_KT + 16 * t + 4 * fg + r;
                s[t][r] = key < N ? s[t][r] * scale_log2e : -INFINITY;
                tmax = fmaxf(tmax, s[t][r]);
            }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);  // finite: every tile holds at least one key < N
        const float alpha = exp2f(m_run - m_new);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) o[dt] *= alpha;
        half4v pf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = exp2f(s[t][r] - m_new);
                l_run += p;
                pf[t][r] = (half_t)p;
            }
        // O^T[d][q] += V^T[d][key] . P^T[key][q]; A: lane (d = fr, g) holds V[16t + 4g + j][16 dt + fr] (transposed read: lane
        // 4qq + pp of group g addresses row 16t + 4g + qq, columns 16 dt + 4 pp); B: pf[t] as it came out of the S^T accumulator
#pragma unroll
        for (int dt = 0; dt < 5; ++dt)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const half4v vf = lds_tr_read_b64(sV + (16 * t + 4 * fg + (fr >> 2)) * A80_ROWB + (16 * dt + 4 * (fr & 3)) * 2);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[t], o[dt], 0, 0, 0);
            }
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (qrow < N) {                               // lane holds O^T[d = 16 dt + 4 g + r][q = fr]
        const float inv = 1.0f / l_run;
        half_t* ob = out + ((int64_t)b * N + qrow) * ldo + head * D80;
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) {
            half4v h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = (half_t)(o[dt][r] * inv);
            *reinterpret_cast<half4v*>(ob + 16 * dt + 4 * fg) = h;
        }
    }
}

// ---- preprocess + patchify ------------------------------------------------------------------------------------------------
constexpr int PP_MAX_TAPS = 63;

struct PreprocessArgs {
    float gy[PP_MAX_TAPS], gx[PP_MAX_TAPS];    // normalised Gaussian taps (a single tap 1.0 without the blur)
    int ky, kx;                                // tap counts (odd)
    float scale_y, scale_x;                    // bicubic align_corners source step: (in - 1) / (out - 1)
};

__device__ __forceinline__ int reflect_idx(int i, int n) {     // F.pad(mode="reflect"): -1 -> 1, n -> n - 2 (pad < n)
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

// torch upsample_bicubic2d: A = -0.75, taps at floor(x) - 1 .. floor(x) + 2 (aten/src/ATen/native/UpSample.h,
// get_cubic_upsample_coefficients)
__device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
    const float A = -0.75f;
    auto conv1 = [&](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };
    auto conv2 = [&](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };
    c[0] = conv2(t + 1.f);
    c[1] = conv1(t);
    c[2] = conv1(1.f - t);
    c[3] = conv2(2.f - t);
}

template <typename T>
__global__ __launch_bounds__(256) void clip_preprocess_patches_kernel(const T* __restrict__ img, half_t* __restrict__ out, int B,
                                                                      int H, int W, int size, int patch, int ldo, PreprocessArgs a) {
    const int grid = size / patch, kp = 3 * patch * patch;
    const int64_t total = (int64_t)B * grid * grid * ldo;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int col = (int)(idx % ldo);
    const int64_t row = idx / ldo;
    if (col >= kp) {
        out[idx] = (half_t)0.f;
        return;
    }
    const int p = (int)(row % (grid * grid)), b = (int)(row / (grid * grid));
    const int c = col / (patch * patch), kyx = col % (patch * patch);
    const int oy = (p / grid) * patch + kyx / patch, ox = (p % grid) * patch + kyx % patch;
    const float ry = a.scale_y * (float)oy, rx = a.scale_x * (float)ox;
    const int iy = (int)floorf(ry), ix = (int)floorf(rx);
    float cy[4], cx[4];
    cubic_coeffs(ry - (float)iy, cy);
    cubic_coeffs(rx - (float)ix, cx);
    const T* src = img + ((int64_t)b * 3 + c) * H * W;
    const int hy = a.ky / 2, hx = a.kx / 2;
    float acc = 0.f;
    for (int i = 0; i < 4; ++i) {
        const int yy = min(max(iy - 1 + i, 0), H - 1);
        float rowv = 0.f;
        for (int j = 0; j < 4; ++j) {
            const int xx = min(max(ix - 1 + j, 0), W - 1);
            float bl = 0.f;                   // the (blurred) pixel (yy, xx)
            for (int u = 0; u < a.ky; ++u) {
                const T* sr = src + (int64_t)reflect_idx(yy + u - hy, H) * W;
                float h = 0.f;
                for (int w = 0; w < a.kx; ++w) h += a.gx[w] * (float)sr[reflect_idx(xx + w - hx, W)];
                bl += a.gy[u] * h;
            }
            rowv += cx[j] * bl;
        }
        acc += cy[i] * rowv;
    }
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
    const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    out[idx] = (half_t)(((acc + 1.f) * 0.5f - mean[c]) / stdv[c]);
}

__global__ __launch_bounds__(256) void clip_assemble_tokens_kernel(const float* __restrict__ patch, int ldp, const float* __restrict__ cls,
                                                                   const float* __restrict__ pos, half_t* __restrict__ out, int B, int P,
                                                                   int C) {
    const int64_t total = (int64_t)B * (P + 1) * C;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int64_t bt = idx / C;
    const int t = (int)(bt % (P + 1)), b = (int)(bt / (P + 1));
    const float x = t == 0 ? cls[c] : patch[((int64_t)b * P + t - 1) * ldp + c];
    out[idx] = (half_t)(x + pos[(int64_t)t * C + c]);
}

}  // namespace

extern "C" int moca_attention_d80_f16(const void* q, const void* k, const void* v, void* out,
                                      int32_t B, int32_t heads, int32_t N, int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                                      float scale, void* stream) {
    auto misaligned = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1)) != 0; };
    if (!q || !k || !v || !out || B <= 0 || heads <= 0 || N <= 0) return MOCA_E_BADARG;
    if (misaligned(q, 16) || misaligned(k, 16) || misaligned(v, 16) || misaligned(out, 8)) return MOCA_E_BADARG;
    if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4) return MOCA_E_BADARG;
    if (ldq < heads * D80 || ldk < heads * D80 || ldv < heads * D80 || ldo < heads * D80) return MOCA_E_BADARG;
    if ((int64_t)B * heads > 65535 || !isfinite(scale * 1.4426950408889634f)) return MOCA_E_BADARG;
    const dim3 grid((N + A80_QB - 1) / A80_QB, B * heads), block(256);
    hipLaunchKernelGGL(clip_attention_d80_kernel, grid, block, 0, moca_stream(stream),
                       reinterpret_cast<const half_t*>(q), reinterpret_cast<const half_t*>(k),
                       reinterpret_cast<const half_t*>(v), reinterpret_cast<half_t*>(out),
                       heads, N, ldq, ldk, ldv, ldo, scale * 1.4426950408889634f);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_clip_preprocess_patches_f16(const void* img, int32_t img_is_f32, void* out, int32_t B, int32_t H, int32_t W,
                                                int32_t size, int32_t patch, int32_t ldo, int32_t antialias, void* stream) {
    if (!img || !out || B <= 0 || H < 2 || W < 2 || H > 16384 || W > 16384 || size < 2 || patch <= 0 || size % patch) return MOCA_E_BADARG;
    if (ldo < 3 * patch * patch || ldo % 8) return MOCA_E_BADARG;
    PreprocessArgs a{};
    a.ky = a.kx = 1;
    a.gy[0] = a.gx[0] = 1.f;
    // kornia.geometry.resize(antialias=True): blur iff max(factor) > 1 with sigma = max((factor - 1) / 2, 0.001) per axis,
    // kernel size int(max(4 sigma, 3)) bumped to odd, normalised Gaussian taps, reflect border (kornia/geometry/transform/affwarp.py)
    if (antialias && (H > size || W > size)) {
        const double sg[2] = {fmax(((double)H / size - 1.0) / 2.0, 0.001), fmax(((double)W / size - 1.0) / 2.0, 0.001)};
        int* ks[2] = {&a.ky, &a.kx};
        float* g[2] = {a.gy, a.gx};
        const int dim[2] = {H, W};
        for (int ax = 0; ax < 2; ++ax) {
            int n = (int)fmax(4.0 * sg[ax], 3.0);
            if (n % 2 == 0) ++n;
            if (n > PP_MAX_TAPS || n / 2 >= dim[ax]) return MOCA_E_BADARG;
            float sum = 0.f;
            for (int i = 0; i < n; ++i) {
                const float x = (float)(i - n / 2);
                g[ax][i] = expf(-x * x / (float)(2.0 * sg[ax] * sg[ax]));
                sum += g[ax][i];
            }
            for (int i = 0; i < n; ++i) g[ax][i] /= sum;
            *ks[ax] = n;
        }
    }
    a.scale_y = (float)(H - 1) / (float)(size - 1);
    a.scale_x = (float)(W - 1) / (float)(size - 1);
    const int grid = size / patch;
    const int64_t total = (int64_t)B * grid * grid * ldo;
    const dim3 g((unsigned)((total + 255) / 256)), block(256);
    if (img_is_f32)
        hipLaunchKernelGGL(clip_preprocess_patches_kernel<float>, g, block, 0, moca_stream(stream), reinterpret_cast<const float*>(img),
                           reinterpret_cast<half_t*>(out), B, H, W, size, patch, ldo, a);
    else
        hipLaunchKernelGGL(clip_preprocess_patches_kernel<half_t>, g, block, 0, moca_stream(stream), reinterpret_cast<const half_t*>(img),
                           reinterpret_cast<half_t*>(out), B, H, W, size, patch, ldo, a);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_clip_assemble_tokens_f16(const float* patch, int32_t ldp, const float* cls, const float* pos, void* out, int32_t B,
                                             int32_t P, int32_t C, void* stream) {
    if (!patch || !cls || !pos || !out || B <= 0 || P <= 0 || C <= 0 || ldp < C) return MOCA_E_BADARG;
    const int64_t total = (int64_t)B * (P + 1) * C;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    hipLaunchKernelGGL(clip_assemble_tokens_kernel, grid, block, 0, moca_stream(stream), patch, ldp, cls, pos, reinterpret_cast<half_t*>(out),
                       B, P, C);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}
