#pragma clang fp contract(off)
// ^ first, and at file scope, so it holds for everything after it in the including translation unit: the fp32 step arithmetic of
// sampler.hip and fifo.hip.  The reference evaluates these expressions as separate fp32 torch ops (mul, sub, div ...), and the tests
// compare with torch.equal; one fused multiply-add changes the last bit.  The Makefile passes -ffp-contract=off for both files too,
// but a helper moved to another file or a build that bypasses the Makefile must not contract silently.
// Device-inline only: formulas that sampler.hip and fifo.hip both evaluate, and what more than one kernel of sampler.hip shares.
#pragma once
#include <stdint.h>

// classifier-free guidance, ddim.py:304 / :372: e_t = e_u + s (e_c - e_u)
__device__ __forceinline__ float cfg_guidance(float e_c, float e_u, float scale) { return e_u + scale * (e_c - e_u); }

// q_sample, ddpm3d.py:415-420: orig = (sac x0) [scale] + s1mac noise, in the reference's order of operations
__device__ __forceinline__ float q_sample_orig(float x0, float nq, float sac, float s1mac, float scale, bool use_scale) {
    float s = sac * x0;
    if (use_scale) s = s * scale;
    return s + s1mac * nq;
}

// the mask blend of the sampling loops, ddpm3d.py:648: img = img_orig * mask + (1 - mask) * img (mask == 1 keeps x0)
__device__ __forceinline__ float mask_blend(float orig, float m, float x) { return orig * m + (1.f - m) * x; }

// ---- the walk of q_sample_kernel and ddpm_step_kernel: one thread per group of four consecutive elements of the
// FLAT [B * per] range, each sample with its own coefficients.  A group that lies inside one sample (and every pointer being 16-byte
// aligned) moves as float4; a group that straddles two samples (per % 4 != 0) or the end goes element by element -- nothing is read
// or written past B * per.
struct group4 {
    int64_t e0, b0;   // first element, its sample
    int cnt;          // elements inside [0, total)
    bool vec;         // whole, inside sample b0, pointers aligned
};

__device__ __forceinline__ group4 group4_at(int64_t q, int64_t total, int64_t per, int vec_ok) {
    group4 g;
    g.e0 = q * 4;
    g.b0 = g.e0 / per;
    g.cnt = total - g.e0 < 4 ? (int)(total - g.e0) : 4;
    g.vec = vec_ok && g.cnt == 4 && (g.e0 + 3) / per == g.b0;
    return g;
}

// p NULL: v keeps what it holds / nothing is stored
__device__ __forceinline__ void group4_ld(const float* p, int64_t e0, bool vec, int cnt, float (&v)[4]) {
    if (!p) return;
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p + e0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        for (int j = 0; j < cnt; ++j) v[j] = p[e0 + j];
    }
}

__device__ __forceinline__ void group4_st(float* p, int64_t e0, bool vec, int cnt, const float (&v)[4]) {
    if (!p) return;
    if (vec) {
        *reinterpret_cast<float4*>(p + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < cnt; ++j) p[e0 + j] = v[j];
    }
}

// the mask of group g: [B][per] (`c0` false), or one channel [B][inner] read with channel stride 0 (`c0`: per % inner == 0).  With
// `mask_vec` (mask 16-byte aligned, per % 4 == 0 and inner % 4 == 0) a vector group stays inside one channel and reads one float4;
// else element by element, each at its own sample and offset.
__device__ __forceinline__ void mask_read4(const float* mask, const group4& g, int64_t per, int64_t inner, bool c0, bool mask_vec,
                                           float (&mk)[4]) {
    if (!c0) {
        group4_ld(mask, g.e0, g.vec, g.cnt, mk);
    } else if (g.vec && mask_vec) {
        group4_ld(mask, g.b0 * inner + (g.e0 - g.b0 * per) % inner, true, 4, mk);
    } else {
        for (int j = 0; j < g.cnt; ++j) {
            const int64_t b = (g.e0 + j) / per;
            mk[j] = mask[b * inner + (g.e0 + j - b * per) % inner];
        }
    }
}
