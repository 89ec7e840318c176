// fp32 step arithmetic of ONE trajectory (lvdm/models/samplers/ddim.py, lvdm/models/ddpm3d.py): guidance, the DDIM update as a
// host-parameterised call and as the device-resident base-sampling step, the encoder's Gaussian sample, q_sample and the DDPM step.
// The MoCA FIFO (ring queue, windows, per-frame recurrence) is fifo.hip.  No FMA contraction (step_math.h, and -ffp-contract=off in
// the Makefile): the reference evaluates these expressions as separate fp32 torch ops (mul, sub, div ...), and the results are
// compared bit for bit.  HBM-bound, one thread per latent element or group of four.
#include "common.h"
#include "step_math.h"

namespace {

__global__ __launch_bounds__(256) void cfg_combine_kernel(const float* __restrict__ ec, const float* __restrict__ eu,
                                                          float* __restrict__ out, float scale, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = cfg_guidance(ec[i], eu[i], scale);   // ddim.py:304,372
}

// the tail of p_sample_ddim (ddim.py:339-356) for one element
struct ddim_coef {
    float sqrt_at, sqrt_aprev, sigma_t, sqrt_one_minus_at, dir_coef, scale_t, scale_prev;
};

__device__ __forceinline__ void ddim_tail(float x, float et, float noise, const ddim_coef& k, int use_scale, float& x_prev,
                                          float& pred_x0) {
    float p0 = (x - k.sqrt_one_minus_at * et) / k.sqrt_at;     // ddim.py:339
    const float dir = k.dir_coef * et;                          // :343
    const float nz = k.sigma_t * noise;                         // :345
    if (use_scale) {
        p0 = p0 / k.scale_t;                                    // :353
        x_prev = k.sqrt_aprev * k.scale_prev * p0 + dir + nz;   // :354
    } else {
        x_prev = k.sqrt_aprev * p0 + dir + nz;                  // :356
    }
    pred_x0 = p0;
}

__global__ __launch_bounds__(256) void ddim_update_kernel(const float* __restrict__ x, const float* __restrict__ e,
                                                          const float* __restrict__ noise, float* __restrict__ x_prev,
                                                          float* __restrict__ pred_x0, float sqrt_at, float sqrt_aprev,
                                                          float sigma_t, float sqrt_one_minus_at, float dir_coef,
                                                          int use_scale, float scale_t, float scale_prev, int64_t n) {
    const ddim_coef k = {sqrt_at, sqrt_aprev, sigma_t, sqrt_one_minus_at, dir_coef, scale_t, scale_prev};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float xp, p0;
        ddim_tail(x[i], e[i], noise[i], k, use_scale, xp, p0);
        x_prev[i] = xp;
        pred_x0[i] = p0;
    }
}

// ---- base sampling (ddim.py:226-252): one DDIM step of `ddim_sampling` as device-side work.  Step i of the loop uses schedule
// index S - 1 - i (ddim.py:238); i = state->iter mod S, so a captured step replays for every i.
// rows[0:n] = table[S - 1 - i]: the timestep rows of the UNet plan (ddim.py:239 `ts = torch.full((b,), step)`)
__global__ __launch_bounds__(256) void base_set_timestep_kernel(const moca_fifo_state* __restrict__ st, const int64_t* __restrict__ table,
                                                                int S, int64_t* __restrict__ rows, int n) {
    const int64_t t = table[S - 1 - st->iter % S];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) rows[i] = t;
}

// guidance (ddim.py:304) + the tail of p_sample_ddim (ddim.py:328-357, as ddim_update_kernel) with the coefficients of schedule
// index S - 1 - i: coef[idx] = {sqrt(a_t), sqrt(a_prev), sigma_t, sqrt(1 - a_t), sqrt(1 - a_prev - sigma_t^2), scale_t, scale_prev, -}.
// x is updated IN PLACE (it is the UNet plan's input buffer: the next step reads it there).
__global__ __launch_bounds__(256) void base_step_kernel(const moca_fifo_state* __restrict__ st, float* __restrict__ x,
                                                        const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                        const float* __restrict__ noise, float* __restrict__ pred_x0,
                                                        const float* __restrict__ coef, int S, float cfg_scale, int use_scale, int64_t n) {
    const float* cf = coef + (int64_t)(S - 1 - st->iter % S) * 8;
    const ddim_coef k = {cf[0], cf[1], cf[2], cf[3], cf[4], cf[5], cf[6]};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float et = eps_c[i];
        if (eps_u) et = cfg_guidance(et, eps_u[i], cfg_scale);  // :304
        float xp, p0;
        ddim_tail(x[i], et, noise[i], k, use_scale, xp, p0);
        x[i] = xp;
        if (pred_x0) pred_x0[i] = p0;
    }
}

// ---- DPM-Solver++(2M) (Lu et al., 2022) on the same table walk: one multistep update in the data-prediction form for one element.
// p0 is ddim_tail's pred_x0, operation for operation (ddim.py:339,353), so both samplers see the same bits of it.
struct multistep_coef {
    float sqrt_at, c0, c1, sqrt_one_minus_at, cx, scale_t;
};

// x' = (c_x x + c_0 p0) + c_1 (p0 - *hist); a first-order row (c_1 == 0) leaves the history term out and never looks at *hist
__device__ __forceinline__ void multistep_tail(float x, float et, const float* hist, const multistep_coef& k, int use_scale, float& x_next,
                                               float& pred_x0) {
    float p0 = (x - k.sqrt_one_minus_at * et) / k.sqrt_at;     // ddim.py:339
    if (use_scale) p0 = p0 / k.scale_t;                        // :353
    float xn = k.cx * x + k.c0 * p0;
    if (k.c1 != 0.f) xn = xn + k.c1 * (p0 - *hist);
    x_next = xn;
    pred_x0 = p0;
}

// coef[idx] = {sqrt(a_t), c_0, c_1, sqrt(1 - a_t), c_x, scale_t, -, -} (the host's float64 table, rounded once).  `hist` is the history
// operand: the previous step's pred_x0 on entry, this step's on exit, each element read and written by the same thread.  A row whose
// c_1 is 0 (the first step of a trajectory, the last one with lower_order_final, order 1) does NOT read it -- the branch is uniform, on
// the table value -- so that what an earlier trajectory or nobody left there, NaN included, never reaches x.  x is updated IN PLACE.
__global__ __launch_bounds__(256) void multistep_step_kernel(const moca_fifo_state* __restrict__ st, float* __restrict__ x,
                                                             const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                             float* hist, const float* __restrict__ coef, int S, float cfg_scale,
                                                             int use_scale, int64_t n) {
    const float* cf = coef + (int64_t)(S - 1 - st->iter % S) * 8;
    const multistep_coef k = {cf[0], cf[1], cf[2], cf[3], cf[4], cf[5]};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float et = eps_c[i];
        if (eps_u) et = cfg_guidance(et, eps_u[i], cfg_scale);  // :304
        float xn, p0;
        multistep_tail(x[i], et, hist + i, k, use_scale, xn, p0);
        x[i] = xn;
        hist[i] = p0;
    }
}

// the end of a trajectory step (base sampling, DDPM): the next replay of the captured step sees the next schedule index
__global__ void state_bump_kernel(moca_fifo_state* st) {
    st->iter = st->iter + 1;
    st->ext_noise = 0;
}

// ---- DiagonalGaussianDistribution.sample / .mode (lvdm/distributions.py:24-40) + get_first_stage_encoding's scale_factor
//      (ddpm3d.py:458-465): moments [n][2z][hw] = (mean | logvar) -> out [n][z][hw]
__global__ void gaussian_sample_kernel(const float* __restrict__ mom, const float* __restrict__ noise, float* __restrict__ out,
                                       int n, int z, int hw, float scale) {
    const int64_t total = (int64_t)n * z * hw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / ((int64_t)z * hw), r = i - b * z * hw;
        const float mean = mom[b * 2 * z * hw + r];
        float v = mean;
        if (noise) {
            float lv = mom[b * 2 * z * hw + (int64_t)z * hw + r];
            lv = fminf(fmaxf(lv, -30.0f), 20.0f);
            const float sd = expf(0.5f * lv);
            v = mean + sd * noise[i];
        }
        out[i] = scale * v;
    }
}

// q_sample over per-sample schedule indices (ddim.py:652-671 `stochastic_encode`): out[b][p] = ca[t[b]] * x0[b][p] + cb[t[b]] * noise[b][p].
// The gather of both tables runs here (t and the tables are device memory: nothing for the host to read, the launch can be captured).
// mul, mul, add with no contraction = the torch expression bit for bit.  out may alias x0 (every element is read before it is written,
// by the same thread).  An index outside [0, n_tab) reads no table entry: that sample's output is NaN.
__device__ __forceinline__ void q_coef(const float* __restrict__ ca, const float* __restrict__ cb, const int64_t* __restrict__ t, int64_t b,
                                       int n_tab, float& a, float& c, bool& bad) {
    const int64_t tb = t[b];
    bad = tb < 0 || tb >= (int64_t)n_tab;
    a = bad ? 0.f : ca[tb];
    c = bad ? 0.f : cb[tb];
}

__global__ __launch_bounds__(256) void q_sample_kernel(const float* x0, const float* __restrict__ noise, float* out,
                                                       const float* __restrict__ ca, const float* __restrict__ cb,
                                                       const int64_t* __restrict__ t, int B, int n_tab, int64_t per, int vec_ok) {
    const int64_t total = (int64_t)B * per;
    const int64_t n4 = (total + 3) / 4;
    const float qnan = __builtin_nanf("");
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (int64_t)gridDim.x * 256) {
        const group4 g = group4_at(q, total, per, vec_ok);
        float xv[4] = {}, nv[4] = {}, o[4];
        group4_ld(x0, g.e0, g.vec, g.cnt, xv);
        group4_ld(noise, g.e0, g.vec, g.cnt, nv);
        float a, c;
        bool bad;
        q_coef(ca, cb, t, g.b0, n_tab, a, c, bad);
        int64_t b_cur = g.b0;
        for (int j = 0; j < g.cnt; ++j) {
            if (!g.vec) {
                const int64_t b = (g.e0 + j) / per;
                if (b != b_cur) {
                    q_coef(ca, cb, t, b, n_tab, a, c, bad);
                    b_cur = b;
                }
            }
            const float v = a * xv[j] + c * nv[j];
            o[j] = bad ? qnan : v;
        }
        group4_st(out, g.e0, g.vec, g.cnt, o);
    }
}

// One reverse step of the DDPM sampler, `LatentDiffusion.p_sample` (ddpm3d.py:591-610) with the mask blend of `p_sample_loop`
// (:646-648), per element of sample b at that sample's timestep t_b = t[b * t_stride], in the reference's order of fp32 operations:
//   eps = e_u + s (e_c - e_u)                               ddim.py:304 (eps_u NULL: eps = e_c)
//   x_recon = srac x - srm1 eps  |  eps                     :212-216, :573-576     [clamp to -1 .. 1, :580-581]
//   mean = c1 x_recon + c2 x                                :219-222
//   out = mean + (nonzero(t) std) (noise temperature)       :601-610, std = exp(0.5 posterior_log_variance_clipped) from the host
//   orig = sac x0 [scale] + s1mac noise_q                   :415-420
//   out = orig mask + (1 - mask) out                        :648
// mul / add / sub only and no contraction: bit-equal to the torch expression over the same tables.  coef[t] = {srac, srm1, c1, c2,
// std, sac, s1mac, scale}.  eps_c NULL: no reverse step, out = orig (`q_sample`), or with a mask out = orig mask + (1 - mask) x: the
// blend alone, which upstream's DDIM loop runs BEFORE the model call of a step (DDIM / DPM-Solver inpainting).  Groups of four as above (vec_ok: every pointer
// is 16-byte aligned); out may alias x (each thread reads all it needs before it writes).  t_b outside [0, n_tab): nothing is read
// from the table and every output of sample b is NaN.
struct ddpm_args {
    const float* x; float* out; const float* eps_c; const float* eps_u; const float* noise; float* x_recon; float* mean;
    const float* mask; const float* x0; const float* noise_q; const float* coef; const int64_t* t;
    int64_t t_stride, per, mask_inner;
    float cfg_scale, temperature;
    int B, n_tab, flags, vec_ok, mask_vec;
};

struct ddpm_coef {
    float srac, srm1, c1, c2, sd, sac, s1mac, scale;
    bool bad;
};

__device__ __forceinline__ ddpm_coef ddpm_load_coef(const ddpm_args& a, int64_t b) {
    const int64_t tb = a.t[b * a.t_stride];
    ddpm_coef k;
    k.bad = tb < 0 || tb >= (int64_t)a.n_tab;
    k.srac = k.srm1 = k.c1 = k.c2 = k.sd = k.sac = k.s1mac = k.scale = 0.f;
    if (k.bad) return k;
    const float* c = a.coef + tb * 8;
    k.srac = c[0]; k.srm1 = c[1]; k.c1 = c[2]; k.c2 = c[3];
    k.sd = (tb == 0 ? 0.f : 1.f) * c[4];                        // nonzero_mask * (0.5 * model_log_variance).exp(), :605-610
    k.sac = c[5]; k.s1mac = c[6]; k.scale = c[7];
    return k;
}

__global__ __launch_bounds__(256) void ddpm_step_kernel(const ddpm_args a) {
    const int64_t per = a.per, total = (int64_t)a.B * per;
    const int64_t n4 = (total + 3) / 4;
    const float qnan = __builtin_nanf("");
    const bool x0_param = a.flags & MOCA_DDPM_X0, clip = a.flags & MOCA_DDPM_CLIP, use_scale = a.flags & MOCA_DDPM_SCALE;
    const bool blend = a.mask != nullptr;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (int64_t)gridDim.x * 256) {
        const group4 g = group4_at(q, total, per, a.vec_ok);
        const int64_t e0 = g.e0, b0 = g.b0;
        const int cnt = g.cnt;
        const bool vec = g.vec;
        float x[4] = {}, ec[4] = {}, eu[4] = {}, nz[4] = {}, mk[4] = {}, x0[4] = {}, nq[4] = {}, o[4], rc[4], mn[4];
        group4_ld(a.x, e0, vec, cnt, x);
        group4_ld(a.eps_c, e0, vec, cnt, ec);
        group4_ld(a.eps_u, e0, vec, cnt, eu);
        if (a.out) group4_ld(a.noise, e0, vec, cnt, nz);
        group4_ld(a.x0, e0, vec, cnt, x0);
        group4_ld(a.noise_q, e0, vec, cnt, nq);
        if (blend) mask_read4(a.mask, g, per, a.mask_inner, a.flags & MOCA_DDPM_MASK_C0, a.mask_vec, mk);
        ddpm_coef k = ddpm_load_coef(a, b0);
        int64_t b_cur = b0;
        for (int j = 0; j < cnt; ++j) {
            if (!vec) {
                const int64_t b = (e0 + j) / per;
                if (b != b_cur) {
                    k = ddpm_load_coef(a, b);
                    b_cur = b;
                }
            }
            float orig = 0.f;
            if (a.x0) orig = q_sample_orig(x0[j], nq[j], k.sac, k.s1mac, k.scale, use_scale);   // :415-420
            float v = orig;
            rc[j] = mn[j] = qnan;
            if (a.eps_c) {
                float e = ec[j];
                if (a.eps_u) e = cfg_guidance(e, eu[j], a.cfg_scale);         // ddim.py:304
                float r = x0_param ? e : k.srac * x[j] - k.srm1 * e;          // :573-576
                if (clip) r = r < -1.f ? -1.f : (r > 1.f ? 1.f : r);          // :581 (NaN stays NaN, as clamp_)
                const float m = k.c1 * r + k.c2 * x[j];                       // :219-222
                v = m + k.sd * (nz[j] * a.temperature);                       // :601,608
                if (blend) v = mask_blend(orig, mk[j], v);                     // :648
                if (!k.bad) {
                    rc[j] = r;
                    mn[j] = m;
                }
            } else if (blend) {
                v = mask_blend(orig, mk[j], x[j]);                             // the blend alone, in front of a DDIM / solver step
            }
            o[j] = k.bad ? qnan : v;
        }
        group4_st(a.out, e0, vec, cnt, o);
        group4_st(a.x_recon, e0, vec, cnt, rc);
        group4_st(a.mean, e0, vec, cnt, mn);
    }
}

}  // namespace

extern "C" int moca_cfg_combine_f32(const float* e_c, const float* e_u, float* out, float scale,
                                    int64_t n, void* stream) {
    if (!e_c || !e_u || !out || n <= 0) return MOCA_E_BADARG;
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(grid_for(n)), dim3(256), 0, moca_stream(stream), e_c, e_u, out, scale, n);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_ddim_update_f32(const float* x, const float* e, const float* noise, float* x_prev,
                                    float* pred_x0, float a_t, float a_prev, float sigma_t,
                                    float sqrt_one_minus_at, int32_t use_scale, float scale_t,
                                    float scale_prev, int64_t n, void* stream) {
    if (!x || !e || !noise || !x_prev || !pred_x0 || n <= 0 || a_t <= 0.f) return MOCA_E_BADARG;
    // same fp32 scalar ops as the torch.full(...).sqrt() tensors of ddim.py:331-343
    const float sqrt_at = sqrtf(a_t), sqrt_aprev = sqrtf(a_prev);
    const float dir_coef = sqrtf(1.0f - a_prev - sigma_t * sigma_t);
    hipLaunchKernelGGL(ddim_update_kernel, dim3(grid_for(n)), dim3(256), 0, moca_stream(stream), x, e, noise, x_prev, pred_x0,
                       sqrt_at, sqrt_aprev, sigma_t, sqrt_one_minus_at, dir_coef, use_scale, scale_t, scale_prev, n);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_base_set_timestep(const moca_fifo_state* state, const int64_t* table, int32_t S, int64_t* rows, int32_t n, void* stream) {
    if (!state || !table || !rows || S <= 0 || n <= 0) return MOCA_E_BADARG;
    hipLaunchKernelGGL(base_set_timestep_kernel, dim3(grid_for(n)), dim3(256), 0, moca_stream(stream), state, table, S, rows, n);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_base_ddim_step_f32(moca_fifo_state* state, float* x, const float* eps_c, const float* eps_u, const float* noise,
                                       float* pred_x0, const float* coef, int32_t S, float cfg_scale, int32_t use_scale, int64_t n,
                                       void* stream) {
    if (!state || !x || !eps_c || !noise || !coef || S <= 0 || n <= 0) return MOCA_E_BADARG;
    if ((use_scale & MOCA_BASE_MULTISTEP) && !pred_x0) return MOCA_E_BADARG;   // the history operand
    hipStream_t st = moca_stream(stream);
    const int scale_bit = use_scale & MOCA_BASE_SCALE;
    if (use_scale & MOCA_BASE_MULTISTEP) {
        hipLaunchKernelGGL(multistep_step_kernel, dim3(grid_for(n)), dim3(256), 0, st, state, x, eps_c, eps_u, pred_x0, coef, S, cfg_scale,
                           scale_bit, n);
    } else {
        hipLaunchKernelGGL(base_step_kernel, dim3(grid_for(n)), dim3(256), 0, st, state, x, eps_c, eps_u, noise, pred_x0, coef, S, cfg_scale,
                           scale_bit, n);
    }
    MOCA_CHECK_LAUNCH();
    hipLaunchKernelGGL(state_bump_kernel, dim3(1), dim3(1), 0, st, state);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_gaussian_sample_f32(const float* moments, const float* noise, float* out, int32_t n, int32_t z, int32_t hw,
                                        float scale, void* stream) {
    if (!moments || !out || n <= 0 || z <= 0 || hw <= 0) return MOCA_E_BADARG;
    hipLaunchKernelGGL(gaussian_sample_kernel, dim3(grid_for((int64_t)n * z * hw)), dim3(256), 0, moca_stream(stream), moments, noise, out,
                       n, z, hw, scale);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_q_sample_f32(const float* x0, const float* noise, float* out, const float* coef_x, const float* coef_n,
                                 const int64_t* t, int32_t B, int32_t n_tab, int64_t per, void* stream) {
    if (!x0 || !noise || !out || !coef_x || !coef_n || !t || B <= 0 || per <= 0 || n_tab <= 0) return MOCA_E_BADARG;
    const int vec_ok = (((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)out) & 15) == 0;
    const int64_t n4 = ((int64_t)B * per + 3) / 4;
    hipLaunchKernelGGL(q_sample_kernel, dim3(grid_for(n4)), dim3(256), 0, moca_stream(stream), x0, noise, out, coef_x, coef_n, t, B, n_tab,
                       per, vec_ok);
    MOCA_CHECK_LAUNCH();
    return MOCA_OK;
}

extern "C" int moca_ddpm_step_f32(moca_fifo_state* state, const float* x, float* out, const float* eps_c, const float* eps_u,
                                  const float* noise, float* x_recon, float* mean, const float* mask, const float* x0,
                                  const float* noise_q, const float* coef, const int64_t* t, int64_t t_stride, int32_t B, int32_t n_tab,
                                  int64_t per, int64_t mask_inner, float cfg_scale, float temperature, int32_t flags, void* stream) {
    if (!coef || !t || B <= 0 || n_tab <= 0 || per <= 0 || t_stride < 0) return MOCA_E_BADARG;
    if (flags & ~(MOCA_DDPM_X0 | MOCA_DDPM_CLIP | MOCA_DDPM_SCALE | MOCA_DDPM_MASK_C0)) return MOCA_E_BADARG;
    if (!x0 != !noise_q) return MOCA_E_BADARG;
    if (eps_c) {                                                 // a reverse step: at least one output; the blend wants all three
        if (!x || !(out || x_recon || mean) || (out && !noise)) return MOCA_E_BADARG;
        if (!mask != !x0 || (mask && !out)) return MOCA_E_BADARG;
    } else if (!x0 || !out || eps_u || x_recon || mean || (mask && !x)) {   // q_sample only; with a mask the blend alone, which reads x
        return MOCA_E_BADARG;
    }
    const bool c0 = mask && (flags & MOCA_DDPM_MASK_C0);
    if (c0 && (mask_inner <= 0 || per % mask_inner != 0)) return MOCA_E_BADARG;
    const uintptr_t all = (uintptr_t)x | (uintptr_t)out | (uintptr_t)eps_c | (uintptr_t)eps_u | (uintptr_t)noise | (uintptr_t)x_recon |
                          (uintptr_t)mean | (uintptr_t)x0 | (uintptr_t)noise_q;
    if (((all | (uintptr_t)mask | (uintptr_t)coef) & 3) || ((uintptr_t)t & 7) || ((uintptr_t)state & 3)) return MOCA_E_BADARG;
    ddpm_args a;
    a.x = x; a.out = out; a.eps_c = eps_c; a.eps_u = eps_u; a.noise = noise; a.x_recon = x_recon; a.mean = mean;
    a.mask = mask; a.x0 = x0; a.noise_q = noise_q; a.coef = coef; a.t = t;
    a.t_stride = t_stride; a.per = per; a.mask_inner = c0 ? mask_inner : per;
    a.cfg_scale = cfg_scale; a.temperature = temperature;
    a.B = B; a.n_tab = n_tab; a.flags = flags;
    a.vec_ok = ((all | (c0 ? 0 : (uintptr_t)mask)) & 15) == 0;
    a.mask_vec = c0 && ((uintptr_t)mask & 15) == 0 && per % 4 == 0 && mask_inner % 4 == 0;
    hipStream_t st = moca_stream(stream);
    const int64_t n4 = ((int64_t)B * per + 3) / 4;
    hipLaunchKernelGGL(ddpm_step_kernel, dim3(grid_for(n4)), dim3(256), 0, st, a);
    MOCA_CHECK_LAUNCH();
    if (state) {
        hipLaunchKernelGGL(state_bump_kernel, dim3(1), dim3(1), 0, st, state);
        MOCA_CHECK_LAUNCH();
    }
    return MOCA_OK;
}
