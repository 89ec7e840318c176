// Shared device/host helpers for libmoca_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/moca_hip.h"

typedef _Float16 half_t;
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef _Float16 half8v __attribute__((ext_vector_type(8)));
typedef float    f32x4  __attribute__((ext_vector_type(4)));
typedef float    f32x16 __attribute__((ext_vector_type(16)));

#define MOCA_WAVE 64

// ds_read_b64_tr_b16, the CDNA4 transposing LDS read: a 16-lane group reads a 4-row x 16-column block of 16-bit elements and receives
// it column-major (lane i gets column i of the 4 rows, element j from row j).  Lane i = 4q+p supplies the address of row q, columns
// 4p..4p+3.  (The host pass only needs a body: the builtin belongs to the device target.)
typedef short lds_short4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) lds_short4v* lds_short4v_ptr;
__device__ __forceinline__ half4v lds_tr_read_b64(const char* addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    const lds_short4v v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v_ptr)addr);
    return __builtin_bit_cast(half4v, v);
#else
    return half4v{0, 0, 0, 0};
#endif
}

#define MOCA_CHECK_LAUNCH()                                  \
    do {                                                     \
        hipError_t e__ = hipGetLastError();                  \
        if (e__ != hipSuccess) return MOCA_E_LAUNCH;         \
    } while (0)

static inline hipStream_t moca_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// blocks of 256 threads for `total` work items of a grid-stride kernel: at most 4096, beyond that a thread loops
static inline int grid_for(int64_t total) {
    int64_t g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

// current value of a MOCA_TUNE_* knob (runtime.hip; set through moca_set_tuning)
int moca_tuning_get(int knob);

// gemm_ws.hip: the weight-stationary streaming kernel of the 320 -> 320 linears (dispatched by moca_gemm_f16)
bool moca_gemm_ws_ok(const moca_gemm_params& p);
int moca_gemm_ws_launch(const moca_gemm_params& p, hipStream_t st);

// x * sigmoid(x) with v_exp + v_rcp (1 ulp each, far below the fp16 output resolution) instead of an IEEE division: the
// GroupNorm apply pass runs it on every activation and the division's ~10 instructions were a third of its VALU work
__device__ __forceinline__ float moca_silu(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
}
// erf GELU, as F.gelu default (attention.py:383).  erf by Abramowitz-Stegun 7.1.26
// (|abs err| <= 1.5e-7 + 1 ulp of v_rcp_f32, far below the fp16 output resolution): 1 v_rcp + 1 v_exp
// + 6 FMA instead of libm erff's ~40-instruction branchy polynomial.  The GEGLU epilogue runs it
// M*4C times per FeedForward and is VALU-bound, so the 2-wide form below is written on float2 vectors:
// hipcc emits v_pk_mul_f32 / v_pk_fma_f32 for it (half the VALU issue slots of the scalar form).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float moca_erf(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
    float y = 1.061405429f;
    y = y * t - 1.453152027f;
    y = y * t + 1.421413741f;
    y = y * t - 0.284496736f;
    y = y * t + 0.254829592f;
    y = 1.0f - y * t * __builtin_amdgcn_exp2f(ax * ax * -1.4426950408889634f);
    return copysignf(y, x);
}
__device__ __forceinline__ float moca_gelu(float x) { return 0.5f * x * (1.0f + moca_erf(x * 0.70710678118654752f)); }

__device__ __forceinline__ f32x2 moca_erf2(f32x2 x) {
    const f32x2 ax = {fabsf(x[0]), fabsf(x[1])};
    const f32x2 d = ax * 0.3275911f + 1.0f;
    const f32x2 t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    f32x2 y = t * 1.061405429f - 1.453152027f;
    y = y * t + 1.421413741f;
    y = y * t - 0.284496736f;
    y = y * t + 0.254829592f;
    const f32x2 a2 = ax * ax * -1.4426950408889634f;
    const f32x2 e = {__builtin_amdgcn_exp2f(a2[0]), __builtin_amdgcn_exp2f(a2[1])};
    y = 1.0f - y * t * e;
    return f32x2{copysignf(y[0], x[0]), copysignf(y[1], x[1])};
}
// value * gelu(gate) for two (value, gate) pairs.  gelu(g) = g * Phi(g) with Phi from the same A&S 7.1.26 erf, written so that no
// sign has to be restored:  for x = |g| / sqrt(2), t = 1 / (1 + p x), q = (a1 t + ... + a5 t^5) exp(-x^2) = 1 - erf(x):
//     gelu(g) = max(g, 0) - |g| q / 2 = g / 2 + |g| (1 - q) / 2
// (g >= 0: g (1 - q / 2) = g (1 + erf) / 2;  g < 0: g q / 2 = g (1 - erf(|x|)) / 2).  The 1/2 is folded into the coefficients, the
// 1/sqrt(2) into p, exp(-x^2) = exp2(-(g c)^2) with c = sqrt(log2(e) / 2): 12 plain + 2 transcendental instructions per output in
// scalar form, 9 issue slots in the packed form below (the round-4 form took 18.5: copysign, 1 - y, (erf + 1), g / 2 and the moves
// the packed operands needed).
#ifdef MOCA_GELU_OLD
__device__ __forceinline__ f32x2 moca_geglu2(f32x2 v, f32x2 g) {
    return v * (g * 0.5f) * (moca_erf2(g * 0.70710678118654752f) + 1.0f);
}
#else
__device__ __forceinline__ f32x2 moca_geglu2(f32x2 v, f32x2 g) {
    const f32x2 ag = {fabsf(g[0]), fabsf(g[1])};
    const f32x2 d = ag * (0.3275911f * 0.70710678118654752f) + 1.0f;
    const f32x2 t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    f32x2 y = t * (0.5f * 1.061405429f) - (0.5f * 1.453152027f);
    y = y * t + (0.5f * 1.421413741f);
    y = y * t - (0.5f * 0.284496736f);
    y = y * t + (0.5f * 0.254829592f);
    y = y * t;
    const f32x2 u = g * 0.84932180028801904f;                    // sqrt(log2(e) / 2)
    const f32x2 s = -u * u;
    const f32x2 e = {__builtin_amdgcn_exp2f(s[0]), __builtin_amdgcn_exp2f(s[1])};
    // max(g, 0) - |g| y e = g / 2 + |g| (1 / 2 - y e)      ((g + |g|) / 2 is exact; no v_max, which costs two instructions under IEEE mode)
    const f32x2 w = 0.5f - y * e;
    return v * (g * 0.5f + ag * w);
}
#endif
// four (value, gate) pairs at once: the same arithmetic on 4-vectors, so that two independent packed chains sit next to each other in
// program order and fill each other's dependent-issue slots (the 2-wide form leaves an s_nop behind every step of the Horner chain)
typedef float f32x4g __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4g moca_geglu4(f32x4g v, f32x4g g) {
    const f32x4g ag = {fabsf(g[0]), fabsf(g[1]), fabsf(g[2]), fabsf(g[3])};
    const f32x4g d = ag * (0.3275911f * 0.70710678118654752f) + 1.0f;
    const f32x4g t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1]), __builtin_amdgcn_rcpf(d[2]), __builtin_amdgcn_rcpf(d[3])};
    // yn = -(a1 t + ... + a5 t^5) / 2 (negated coefficients: 1 / 2 + yn e needs no sign flip, which the 4-wide form would do with v_xor)
    float c1n = -0.5f * 1.061405429f;
    asm("" : "+s"(c1n));                                         // (opaque: a visible negative factor is rewritten as (-t) * |c|, i.e. 4 v_xor)
    f32x4g yn = t * c1n + (0.5f * 1.453152027f);
    yn = yn * t - (0.5f * 1.421413741f);
    yn = yn * t + (0.5f * 0.284496736f);
    yn = yn * t - (0.5f * 0.254829592f);
    yn = yn * t;
    const f32x4g u = g * 0.84932180028801904f;
    const f32x4g s = u * u;                                      // (the sign rides on v_exp_f32's source modifier)
    const f32x4g e = {__builtin_amdgcn_exp2f(-s[0]), __builtin_amdgcn_exp2f(-s[1]), __builtin_amdgcn_exp2f(-s[2]), __builtin_amdgcn_exp2f(-s[3])};
    const f32x4g w = yn * e + 0.5f;
    return v * (g * 0.5f + ag * w);
}

// GroupNorm statistics accumulated across blocks (MOCA_EP_GSTAT, concat with statistics): 64-bit FIXED-POINT atomics -- integer
// addition is associative, so the finished statistics do not depend on the order in which the producer's blocks arrive and a
// replayed graph reproduces its output bit for bit by construction (f64 atomicAdd did so only "in practice").
// Units (round 6; 2^-30 / 2^-16 before): sum 2^-20, sum of squares 2^-12.  What they must hold: one PARTIAL (tiled GEMM: a row tile
// x a channel group, <= 320 x 40 = 12 800 values, whatever the frame count; the weight-stationary kernel's partial is larger, see
// below) is accepted up to 2^53 units; a group's TOTAL is READ up to 2^61 units of the sum of squares:
//     sum:            |partial| < 8.6e9 (a mean of 6.7e5 over 12 800 values)                         -- beyond fp16 (max 65 504)
//     sum of squares:  partial  < 2.2e12 (rms 1.3e4 over 12 800 values),      total  < 2^49 = 5.6e14.
//   The total is what grows with the frames of a statistics group (the 5-D GroupNorms of the temporal convs and of the temporal
//   transformers: T x HW rows x C / 32 channels, largest at the 320-channel level).  5.6e14 is an rms of
//       3.7e4 over   409 600 values (16 frames, 40 x 64 latents): such a tensor already holds fp16 infinities;
//       2.6e4 over   819 200 values (32 frames, 40 x 64);
//       2.1e4 over 1 310 720 values (32 frames, 64 x 64): 5 x the largest rms the tests or bench.py's synthetic video reach (~4e3).
//   A finite fp16 tensor above those rms values is possible (every |x| near 3e4); its statistics then read back as NaN (below), not
//   as a wrong number.
//   The WEIGHT-STATIONARY kernel (gemm_ws.hip, the 320 -> 320 linears: 10 channels per group) adds ONE partial per block and
//   statistics group over ALL the block's rows of that group: rows of the group / bpg, bpg = 256 CUs / statistics groups of the launch.
//   That partial does grow with the frames and with the videos of a launch, and it is poisoned (NaN, never a wrong number) at
//   2^41 = 2.2e12, i.e. at an rms of sqrt(2.2e12 / values) -- BELOW the group range above once several videos share the launch:
//       32 frames x 2560 pixels, B = 1:   320 rows =  3 200 values: rms 2.6e4 (the group range itself);
//                                B = 8:  2560 rows = 25 600 values: rms 9.3e3  (16 frames: B = 16);
//                                B = 16: 5120 rows = 51 200 values: rms 6.6e3  (16 frames: B = 32)
//   -- still above the ~4e3 of the tests and of bench.py's synthetic video, but the figure to know for such a launch.
//   The sum cannot wrap while the sum of squares is readable: |sum| <= sqrt(values x sum of squares)
//   < sqrt(2^21 x 2^49) = 2^35 = 2^55 units.
//   The old units stopped at a partial rms of 3.3e3 -- reached by the latents of bench.py's synthetic video (~4e3), whose statistics
//   were then CLAMPED, i.e. silently wrong.  Precision: rounding a partial to the units changes a group's mean by
//   < 2^-21 * partials / values and its mean of squares by < 2^-13 * partials / values <= 2^-13 / 400 = 3e-7 at worst (a 5 x 8 x
//   10-value partial), below the 1e-6 / 1e-5 eps added to the variance -- a ratio per partial, independent of the frame count.
// A NON-FINITE partial (NaN / Inf activations) or one beyond +-2^53 units must not turn into finite statistics: it sets bit 62 of
// the group's sum-of-squares accumulator (acc layout [group][2] = {sum, sum of squares}) and adds nothing; OR is idempotent, so the
// bit survives however many partials are poisoned.  moca_gstat_get returns NaN when the sum-of-squares accumulator, read as unsigned,
// is >= 2^61 -- the poison bit, or accepted adds that came within a factor 2 of it.  That reading is sound while the accepted adds
// cannot wrap the 64-bit word: every one is <= 2^53 units and non-negative, so FEWER THAN 2^11 PARTIALS per (statistics group, channel
// group) keep the total below 2^64, and everything in [2^61, 2^64) reads NaN.  Partials per accumulator:
//     tiled GEMM epilogue (MOCA_EP_GSTAT): row tiles of >= 160 rows; a channel group (<= 80 columns) lies in <= 2 column tiles
//         (>= 128 columns): <= 2 x ceil(rows of the statistics group / 160).  16 frames x 2560 pixels: 512; 32 x 2560: 1024 = 2^10;
//         32 x 4096 (64 x 64 latents): 1640 by this bound, which counts 160-row tiles whatever the route (131 072 rows are no
//         multiple of 160, so the launch itself takes 256-row tiles: 1024).  The bound 2047 is reached past 1023 x 160 = 163 680
//         rows = 32 frames x 5115 pixels, and the plan refuses a group of MORE THAN 16 FRAMES beyond that (plan.py,
//         _check_gstat_range) instead of running it.  Groups of up to 16 frames are not checked, so that every forward that ran
//         before still runs: 16 frames x more than 10 230 pixels (e.g. 128 x 80 latents) lie outside this bound likewise.  PER-FRAME groups have HW rows whatever the frame count and are not checked: the largest one in
//         use, the VAE decoder's 320 x 512 frame (163 840 rows), receives at most 2^11 partials, where a wrap would need EVERY
//         partial to be exactly 2^53 units -- outside the strict argument by that one case, as before this derivation;
//     weight-stationary kernel: one per block and 80-column wave that touches the group, <= 2 x the blocks of the launch;
//     concat / statistics passes (norm.hip): per-frame statistics only, gn_nchunk(F, HW) <= 2048 / F partials per frame.
// So statistics outside the fixed-point range read back as NaN, never as a wrong finite number, and finite adds can not alias the
// poison bit unnoticed.
#define MOCA_GSTAT_SUM_SCALE 1048576.0        /* 2^20 */
#define MOCA_GSTAT_SQ_SCALE 4096.0            /* 2^12 */
#define MOCA_GSTAT_POISON (1ull << 62)
#define MOCA_GSTAT_MAX_UNITS 9007199254740992.0      /* 2^53 */
__device__ __forceinline__ void moca_gstat_add(int64_t* acc, int comp, float partial) {
    if (!(fabsf(partial) <= 3.0e38f)) {            // NaN or Inf
        atomicOr(reinterpret_cast<unsigned long long*>(acc + (1 - comp)), MOCA_GSTAT_POISON);
        return;
    }
    double v = (double)partial * (comp ? MOCA_GSTAT_SQ_SCALE : MOCA_GSTAT_SUM_SCALE);
    if (!(fabs(v) <= MOCA_GSTAT_MAX_UNITS)) {      // out of the fixed-point range: poison, never clamp (a clamped partial would read
        atomicOr(reinterpret_cast<unsigned long long*>(acc + (1 - comp)), MOCA_GSTAT_POISON);      // back as finite, WRONG statistics)
        return;
    }
    atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)__double2ll_rn(v));
}
__device__ __forceinline__ double moca_gstat_get(const int64_t* acc, int comp) {
    if (comp && (unsigned long long)*acc >= (MOCA_GSTAT_POISON >> 1)) return __longlong_as_double(0x7ff8000000000000ll);
    return (double)*acc * (comp ? 1.0 / MOCA_GSTAT_SQ_SCALE : 1.0 / MOCA_GSTAT_SUM_SCALE);
}
// GroupNorm statistics finished: the sum and the sum of squares of 1 / inv_count values -> mean and 1 / sqrt(variance + eps), in fp64
// (E[x^2] - mean^2 cancels; what rounding leaves below zero is zero)
struct moca_gn_stat { double mean, rstd; };
__device__ __forceinline__ moca_gn_stat moca_gn_finish(double sum, double sq, double inv_count, float eps) {
    const double mean = sum * inv_count;
    double var = sq * inv_count - mean * mean;
    if (var < 0.0) var = 0.0;
    return {mean, 1.0 / sqrt(var + (double)eps)};
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
