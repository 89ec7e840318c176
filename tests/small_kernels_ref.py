"""References, case tables and the per-element bound of tests/test_small_kernels_cpu.py and tests/test_small_kernels_gpu.py: the kernels of
csrc/elementwise.hip, the LayerNorm of csrc/norm.hip, moca_memset_zero, moca_gaussian_sample_f32, the plain DDIM arithmetic kernels and
the FreeInit DFT.

Every operation is restated in plain torch from the reference's formula (the line each kernel's comment cites), with the dtype as a
parameter: float64 is the reference, float32 "what plain torch gives before the final rounding".  `wrong=` selects a WRONG restatement
(MUTANTS): the CPU file shows that every case tells every wrong restatement that applies to it from the right one.

The bound (fp16 outputs), per element, no share of elements left out:

    |got - ref64| <= bound(ref64, slack) = 2^-10 |ref64| + 2^-24 + slack,        slack = 2 max|fp32 - ref64| over the case

2^-10 |ref| is one fp16 ulp (the kernel may round to either neighbour of the exact value), 2^-24 the fp16 subnormal step, and the slack
what fp32 arithmetic costs on THIS case's inputs -- measured on the spot, doubled for a different fp32 summation order (wave butterfly
against torch's).  fp32 outputs of mul/add/sub/div kernels (built without contraction) must be torch.equal to the fp32 torch expression;
gaussian_sample with noise (expf) is held to 4 * 2^-23 |ref| + slack; FreeInit keeps the project's 2e-5 of max|ref| (a DFT spreads its
error over the volume: the max-norm is the right norm there); layout, concat, repeat and memset are exact.

Worst |err| / bound over all elements of all cases, measured on the CPU (test_small_kernels_cpu.py::test_reference_stays_inside_the_bound
prints them): `torch` is the fp32 torch evaluation rounded to fp16, `kernel order` the fp32 restatement that sums as the kernels do
(lane-strided partial sums, then the xor butterfly of wave_sum; exp2 form of the softmax):

    layernorm            torch 0.50   kernel order 0.50
    softmax_rows         torch 0.49   kernel order 0.49   (row sums: 0.01 of their bound)
    silu_add_rows        torch 0.50
    timestep_embedding   torch 0.49
    channel_mix          torch 0.50
    embed_tokens         torch 0.50
    gaussian_sample      torch 0.21   (of 4 * 2^-23 |ref| + slack: the slack is twice this evaluation's own error)

(0.50 = a correctly rounded fp16 result: half an ulp of the one ulp allowed.)  A kernel that exceeds the bound where these do not is wrong.
"""
import math

import torch

# csrc/common.h grid_for(): `if (g > 4096) g = 4096;` blocks of 256 threads, the one definition that csrc/elementwise.hip, sampler.hip,
# fifo.hip and freeinit.hip launch with (moca_gaussian_sample_f32 included): more work items than this and a thread loops
GRID_CAP = 4096 * 256
# csrc/runtime.hip moca_memset_zero(): `if (blocks > 1024) blocks = 1024;` blocks of 256 threads, one 16-byte chunk per trip
ZERO_CAP = 1024 * 256
WRAP = GRID_CAP + 300                      # = 4 * 262219 work items
WRAP4 = WRAP // 4

FREEINIT_TOL = 2e-5                        # of max|ref| (tests/test_sampler_gpu.py)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bound(ref64, slack):
    return 2.0 ** -10 * ref64.abs() + 2.0 ** -24 + slack


def bound_f32_exp(ref64, slack):
    return 4 * 2.0 ** -23 * ref64.abs() + slack


def slack_of(f32, ref64):
    return 2.0 * (f32.double() - ref64).abs().max().item()


def ratio(got, ref64, slack, bound_fn=bound):
    """|got - ref| / bound per element; a non-finite output where the reference is finite counts as infinitely far"""
    r = (got.double() - ref64).abs() / bound_fn(ref64, slack)
    return torch.nan_to_num(r, nan=float("inf"))


def worst(got, ref64, slack, bound_fn=bound):
    return ratio(got, ref64, slack, bound_fn).max().item()


def edge_items(n):
    """flat indices a wrong grid stride corrupts first: the items around the cap and the last 300"""
    idx = [i for i in (GRID_CAP - 1, GRID_CAP, GRID_CAP + 1) if i < n]
    return idx + list(range(max(n - 300, 0), n))


# ----------------------------------------------------------------------------------------------------------------- LayerNorm
# attention.py:199-201 (nn.LayerNorm, eps 1e-5): y = (x - E[x]) / sqrt(Var[x] + eps) * gamma + beta, biased variance over C
LN_KINDS = ("randn", "offset", "ulp", "big")


def layernorm(x, gamma, beta, eps, dtype=torch.float64, wrong=None):
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    C = x.shape[-1]
    mean = (x[:, :-8] if wrong == "mean_drops_last_chunk" else x).mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / (C - 1 if wrong == "var_over_c_minus_1" else C)
    if wrong == "eps_1e-6":
        eps = 1e-6
    return d / torch.sqrt(var + eps) * gamma + beta


def _butterfly(v):
    """wave_sum of csrc/common.h on [..., 64] lane values: v += v[lane ^ o], o = 32 .. 1; every lane ends with the same sum"""
    lanes = torch.arange(64, device=v.device)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def _lane_chunks(x):
    """[M][C] -> [M][i][64 lanes][8]: lane l holds the 8-channel chunks l, l + 64, ... (zero chunks past C: x + 0 is exact)"""
    M, C = x.shape
    nch = C // 8
    maxch = (nch + 63) // 64
    p = torch.zeros(M, maxch * 64 * 8, dtype=x.dtype, device=x.device)
    p[:, :C] = x
    return p.view(M, maxch, 64, 8), (torch.arange(maxch * 64, device=x.device) < nch).view(1, maxch, 64, 1)


def layernorm_kernel_order(x, gamma, beta, eps):
    """fp32, the sums in layernorm_kernel's order: per lane over its chunks and their 8 channels, then the butterfly; two passes"""
    x = x.float()
    M, C = x.shape
    v, live = _lane_chunks(x)
    s = torch.zeros(M, 64, dtype=torch.float32, device=x.device)
    for i in range(v.shape[1]):
        for j in range(8):
            s = s + v[:, i, :, j]
    mean = _butterfly(s) / float(C)
    d = torch.where(live, v - mean.view(M, 1, 1, 1), torch.zeros((), device=x.device))
    q = torch.zeros(M, 64, dtype=torch.float32, device=x.device)
    for i in range(v.shape[1]):
        for j in range(8):
            q = q + d[:, i, :, j] * d[:, i, :, j]
    rstd = torch.rsqrt(_butterfly(q) / float(C) + torch.tensor(eps, dtype=torch.float32, device=x.device))
    return (x - mean[:, None]) * rstd[:, None] * gamma.float() + beta.float()


def ln_instantiation(M, C):
    nch = C // 8
    return "ln%dx%d" % (1 if nch <= 64 else 2 if nch <= 128 else 3 if nch <= 192 else 5, 4 if M >= 16384 else 1)


def _ln_cases():
    cases, seed = {}, [100]

    def add(C, M, kind, eps=1e-5, gamma0=False):
        seed[0] += 1
        name = "c%d_m%d_%s_eps%s_%s%s" % (C, M, kind, "1e-5" if eps == 1e-5 else "1e-6", ln_instantiation(M, C), "_gamma0" if gamma0 else "")
        cases[name] = dict(C=C, M=M, kind=kind, eps=eps, gamma0=gamma0, seed=seed[0])
    Cs = (8, 512, 520, 1024, 1032, 1536, 1544, 2560)
    for n, C in enumerate(Cs):                           # every C with a small M (all four row kinds) ...
        for k, kind in enumerate(LN_KINDS):
            add(C, (1, 3)[(n + k) % 2], kind)
        add(C, 3, "ulp", eps=1e-6)
        add(C, (16384, 16385)[n % 2], LN_KINDS[n % 4])   # ... and one M >= 16384: four rows per wave, all eight instantiations
    for M in (16383, 16384, 16385, 16399):               # the M tails around the switch and inside a block of 16 rows
        add(520, M, "randn")
    add(520, 16399, "offset", eps=1e-6)
    add(2560, 16384, "ulp", eps=1e-6)
    add(520, 3, "randn", gamma0=True)
    add(1032, 16385, "big", gamma0=True)
    return cases


LN_CASES = _ln_cases()


def ln_wrongs(c):
    """the wrong restatements a case can tell.  The variance over C - 1 moves y - beta by 1 / (2 C) of itself: one fp16 ulp at C = 520 and
    nothing a one-ulp bound sees where eps dominates the variance (the near-constant rows) or where the fp32 slack of a wide row at
    offset 100 (2e-4) is larger.  eps = 1e-6 for 1e-5 shows on the near-constant rows only."""
    if c["gamma0"]:
        return ()
    w = ("mean_drops_last_chunk",)
    if c["kind"] in ("randn", "big") or (c["kind"] == "offset" and c["C"] <= 520):
        w += ("var_over_c_minus_1",)
    return w + (("eps_1e-6",) if c["kind"] == "ulp" and c["eps"] == 1e-5 else ())


def ln_inputs(c):
    g = gen(c["seed"])
    M, C = c["M"], c["C"]
    n = min(M, 1031)                                     # (big M: 1031 different rows, row r = base[389 r mod 1031]; neighbours differ)
    r = torch.randn(n, C, generator=g)
    if c["kind"] == "randn":
        x = 2 * r + 0.5
    elif c["kind"] == "offset":
        x = 100 + 0.05 * r
    elif c["kind"] == "ulp":                             # 0.5 and its two fp16 neighbours at distance 2^-11: var ~ 1.6e-7
        x = 0.5 + torch.randint(-1, 2, (n, C), generator=g).float() * 2.0 ** -11
    else:
        x = 3000 * r
    x = x.half()
    if M > n:
        x = x[(torch.arange(M) * 389) % n].contiguous()
    gamma = torch.zeros(C) if c["gamma0"] else 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    return x, gamma, beta


# ----------------------------------------------------------------------------------------------------------------- softmax
# ae_modules.py:66-68: w_ = w_ * c**-0.5; softmax(w_, dim=2)
LOG2E_F32 = 1.4426950408889634


def softmax_rows(s, scale, dtype=torch.float64, wrong=None):
    s = s.to(dtype)
    if wrong == "no_row_max":                            # overflows where scale * max > 88 in fp32
        e = torch.exp(s * scale)
        return e / e.sum(-1, keepdim=True)
    if wrong == "scale_after_exp":                       # exp(s - m) * scale / sum(exp(s - m) * scale): the scale cancels
        e = torch.exp(s - s.max(-1, keepdim=True).values) * scale
        return e / e.sum(-1, keepdim=True)
    return torch.softmax(s * scale, -1)


def softmax_kernel_order(s, scale):
    """fp32, softmax_rows_kernel's form: exp2((v - max) * scale * log2 e), lane l sums elements 4l .. 4l + 3 (+ 256 k), butterfly, one 1 / sum"""
    s = s.float()
    R, N = s.shape
    c = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32)).to(s.device)
    e = torch.exp2((s - s.max(-1, keepdim=True).values) * c)
    trips = (N + 255) // 256
    p = torch.zeros(R, trips * 256, dtype=torch.float32, device=s.device)
    p[:, :N] = e
    p = p.view(R, trips, 64, 4)
    acc = torch.zeros(R, 64, dtype=torch.float32, device=s.device)
    for k in range(trips):
        for q in range(4):
            acc = acc + p[:, k, :, q]
    inv = 1.0 / _butterfly(acc)
    return e * inv[:, None]


VAE_SCALE = 512 ** -0.5
SOFTMAX_CASES = {
    "n4_r1_zero_scale1": dict(N=4, R=1, fill="zero", spread=0.0, scale=1.0, seed=201, wrongs=()),
    "n252_r5_spread30_vae": dict(N=252, R=5, fill="randn", spread=30.0, scale=VAE_SCALE, seed=202, wrongs=("scale_after_exp",)),
    "n256_r8_spread30_scale1": dict(N=256, R=8, fill="randn", spread=30.0, scale=1.0, seed=203, wrongs=("no_row_max",)),
    "n260_r5_spread400_scale1": dict(N=260, R=5, fill="randn", spread=400.0, scale=1.0, seed=204, wrongs=("no_row_max",)),
    "n2560_r8_spread30_vae": dict(N=2560, R=8, fill="randn", spread=30.0, scale=VAE_SCALE, seed=205, wrongs=("scale_after_exp",)),
    "n4096_r1_spread400_vae": dict(N=4096, R=1, fill="randn", spread=400.0, scale=VAE_SCALE, seed=206, wrongs=("scale_after_exp",)),
    "n260_r5_half_inf_vae": dict(N=260, R=5, fill="half_inf", spread=30.0, scale=VAE_SCALE, seed=207, wrongs=("scale_after_exp",)),
    "n516_r8_half_inf_scale1": dict(N=516, R=8, fill="half_inf", spread=30.0, scale=1.0, seed=208, wrongs=("no_row_max",)),
    "n256_r5_one_finite_vae": dict(N=256, R=5, fill="one_finite", spread=30.0, scale=VAE_SCALE, seed=209, wrongs=()),
}


def softmax_inputs(c):
    """fp32 logits [R][N]; the GPU file embeds them in rows of lds = N + 4 floats and writes rows of ldp = N + 8 halves"""
    g = gen(c["seed"])
    R, N = c["R"], c["N"]
    s = torch.randn(R, N, generator=g) * c["spread"]
    if c["fill"] == "zero":
        s.zero_()
    elif c["fill"] == "half_inf":
        s[torch.rand(R, N, generator=g) < 0.5] = -math.inf
        s[:, N // 3] = 1.0                               # (no row is all -inf)
    elif c["fill"] == "one_finite":
        keep = torch.randint(0, N, (R,), generator=g)
        keep[0], keep[-1] = 0, N - 1
        v = s[torch.arange(R), keep].clone()
        s.fill_(-math.inf)
        s[torch.arange(R), keep] = v
    return s


def softmax_sum_bound(ref64, N, slack):
    """per row: |sum(p) - 1| <= N * 2^-11 * max(p) + slack (every stored p is within half an fp16 ulp of max(p) of its fp32 value)"""
    return N * 2.0 ** -11 * ref64.max(-1).values + slack


# ----------------------------------------------------------------------------------------------------------------- silu_add_rows
# openaimodel3d.py time_embed / fps_embedding MLPs: out[r] = silu(a[r / div_a] + b[r / div_b])
def silu_add_rows(a, div_a, b, div_b, rows, silu, dtype=torch.float64, wrong=None):
    if wrong == "div_a_div_b_exchanged":
        div_a, div_b = div_b, div_a
    r = torch.arange(rows, device=a.device)
    v = a.to(dtype)[(r // div_a) % a.shape[0]]
    if b is not None:
        v = v + b.to(dtype)[(r // div_b) % b.shape[0]]
    return v / (1 + torch.exp(-v)) if silu else v


SILU_CASES = {
    "silu_b_div3": dict(rows=6, C=128, div_a=1, div_b=3, silu=True, rng="randn", seed=301, wrongs=("div_a_div_b_exchanged",)),
    "silu_no_b": dict(rows=5, C=72, div_a=1, div_b=0, silu=True, rng="randn", seed=302, wrongs=()),
    "silu_div_a4_div_b2": dict(rows=12, C=40, div_a=4, div_b=2, silu=True, rng="randn", seed=303, wrongs=("div_a_div_b_exchanged",)),
    "add_only_div_a2": dict(rows=7, C=33, div_a=2, div_b=1, silu=False, rng="randn", seed=304, wrongs=("div_a_div_b_exchanged",)),
    "silu_sums_to_100": dict(rows=9, C=257, div_a=1, div_b=3, silu=True, rng="wide", seed=305, wrongs=("div_a_div_b_exchanged",)),
    "wrap_cap_plus_300": dict(rows=WRAP4, C=4, div_a=1, div_b=3, silu=True, rng="randn", seed=306, wrongs=()),
}


def silu_inputs(c):
    g = gen(c["seed"])
    na, nb = -(-c["rows"] // c["div_a"]), (-(-c["rows"] // c["div_b"]) if c["div_b"] else 0)
    if c["rng"] == "wide":                               # sums over [-100, 100], the ends included: exp2 overflows inside moca_silu
        a, b = torch.rand(na, c["C"], generator=g) * 100 - 50, torch.rand(nb, c["C"], generator=g) * 100 - 50
        a[0, :4], b[0, :4] = torch.tensor([-50.0, 50.0, -50.0, -44.0]), torch.tensor([-50.0, 50.0, -39.0, -45.0])
    else:
        a, b = torch.randn(na, c["C"], generator=g) * 2, torch.randn(nb, c["C"], generator=g) * 2
    return a.half(), (b.half() if c["div_b"] else None)


# ----------------------------------------------------------------------------------------------------------------- timestep_embedding
# utils_diffusion.py:8-28.  The reference computes f_k and the argument t * f_k in fp32; the float64 restatement keeps that (an argument
# rounded to fp32 is the operation's input here: at t = 999 its rounding alone moves cos / sin by 6e-5) and takes cos / sin in `dtype`
def timestep_embedding(t, dim, max_period, dtype=torch.float64, wrong=None):
    half = dim // 2
    k = torch.arange(half, dtype=torch.float32)          # on the host, as the reference makes them (`.to(device=...)` follows the exp)
    freqs = torch.exp(-math.log(max_period) * k / (half - 1 if wrong == "k_over_half_minus_1" else half)).to(t.device)
    args = (t[:, None].float() * freqs[None]).to(dtype)
    parts = [torch.sin(args), torch.cos(args)] if wrong == "cos_sin_exchanged" else [torch.cos(args), torch.sin(args)]
    if dim % 2:
        parts.append(torch.zeros_like(args[:, :1]))
    return torch.cat(parts, -1)


def _ts_cases():
    cases, seed = {}, 400
    for dim in (2, 3, 320, 321):
        for P in (10000, 100):
            seed += 1
            cases["dim%d_period%d" % (dim, P)] = dict(dim=dim, n=5, max_period=P, seed=seed,
                                                        wrongs=("cos_sin_exchanged",) + (("k_over_half_minus_1",) if dim > 3 else ()))
    cases["wrap_cap_plus_300"] = dict(dim=4, n=WRAP4, max_period=10000, seed=seed + 1, wrongs=())
    return cases


TIMESTEP_CASES = _ts_cases()


def timestep_inputs(c):
    t = torch.tensor([0, 1, 999, 17, 500], dtype=torch.int64)
    return t[torch.arange(c["n"]) % 5].contiguous()


# ----------------------------------------------------------------------------------------------------------------- layout and copies
def _flat_gather(x, idx):
    return x.reshape(-1)[idx % x.numel()]


def ncthw_to_nhwc(x, Cpad, wrong=None):
    """x [B][Cin][T][HW] -> fp16 rows [(b T + t) HW + p][Cpad], zero pad columns (the permute in front of the first conv)"""
    B, Cin, T, HW = x.shape
    if wrong == "t_hw_swapped":
        y = x.reshape(B, Cin, HW, T).permute(0, 3, 2, 1)
    elif wrong == "cpad_as_cin":                         # channel stride of the source taken from the padded width
        b, t, p, c = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(HW), torch.arange(Cin), indexing="ij")
        y = _flat_gather(x, ((b * Cpad + c) * T + t) * HW + p)
    else:
        y = x.permute(0, 2, 3, 1)
    out = torch.full((B * T * HW, Cpad), 1.0 if wrong == "pad_not_zeroed" else 0.0, dtype=torch.float16, device=x.device)
    out[:, :Cin] = y.reshape(B * T * HW, Cin).half()
    return out


def nhwc_to_ncthw(y, B, Cout, T, HW, dtype, wrong=None):
    """fp16 rows [(b T + t) HW + p][ld] (first Cout columns) -> [B][Cout][T][HW] (openaimodel3d.py:573-577)"""
    v = y[:, :Cout]
    if wrong == "t_hw_swapped":
        return v.reshape(B, HW, T, Cout).permute(0, 3, 2, 1).reshape(B, Cout, T, HW).to(dtype)
    return v.reshape(B, T, HW, Cout).permute(0, 3, 1, 2).to(dtype).contiguous()


TO_NHWC_CASES = {
    "f32_cin4_cpad8": dict(B=2, Cin=4, T=5, HW=33, Cpad=8, f32=True, seed=501, wrongs=("t_hw_swapped", "cpad_as_cin", "pad_not_zeroed")),
    "f16_cin4_cpad8": dict(B=2, Cin=4, T=5, HW=33, Cpad=8, f32=False, seed=502, wrongs=("t_hw_swapped", "cpad_as_cin", "pad_not_zeroed")),
    "f32_cin_eq_cpad": dict(B=3, Cin=8, T=2, HW=7, Cpad=8, f32=True, seed=503, wrongs=("t_hw_swapped",)),
    "f16_cin1": dict(B=2, Cin=1, T=3, HW=5, Cpad=8, f32=False, seed=504, wrongs=("t_hw_swapped", "cpad_as_cin", "pad_not_zeroed")),
    "f32_cin5_cpad16": dict(B=2, Cin=5, T=3, HW=7, Cpad=16, f32=True, seed=505, wrongs=("t_hw_swapped", "cpad_as_cin", "pad_not_zeroed")),
    "wrap_cap_plus_300_f16_cin4_cpad8": dict(B=2, Cin=4, T=2, HW=WRAP4, Cpad=8, f32=False, seed=506, wrongs=()),
}
FROM_NHWC_CASES = {
    "f32_ld_eq_cout": dict(B=3, Cout=8, T=2, HW=7, ld=8, f32=True, seed=511, wrongs=("t_hw_swapped",)),
    "f32_ld8_cout4": dict(B=2, Cout=4, T=5, HW=33, ld=8, f32=True, seed=512, wrongs=("t_hw_swapped",)),
    "f16_ld12_cout4": dict(B=2, Cout=4, T=5, HW=33, ld=12, f32=False, seed=513, wrongs=("t_hw_swapped",)),
    "f16_cout1": dict(B=2, Cout=1, T=3, HW=5, ld=8, f32=False, seed=514, wrongs=("t_hw_swapped",)),
    "wrap_cap_plus_300_f16": dict(B=1, Cout=4, T=1, HW=WRAP4, ld=8, f32=False, seed=515, wrongs=()),
    "wrap_cap_plus_300_f32": dict(B=2, Cout=2, T=1, HW=WRAP4, ld=4, f32=True, seed=516, wrongs=()),
}
CONCAT_CASES = {
    "c1_8_c2_2560": dict(rows=37, C1=8, C2=2560, seed=521),
    "c1_2560_c2_8": dict(rows=37, C1=2560, C2=8, seed=522),
    "rows1": dict(rows=1, C1=64, C2=40, seed=523),
    "at_cap": dict(rows=GRID_CAP // 16, C1=64, C2=64, seed=524),
    "wrap_cap_plus_300": dict(rows=WRAP4, C1=8, C2=24, seed=525),
}
REPEAT_CASES = {
    "reps1_16_bytes": dict(n16=1, reps=1, seed=531),
    "reps3_16_bytes": dict(n16=1, reps=3, seed=532),
    "reps3_below_cap": dict(n16=1000, reps=3, seed=533),
    "wrap_cap_plus_300_reps2": dict(n16=WRAP, reps=2, seed=534),
}
MEMSET_CASES = {"bytes_%d" % n: n for n in (0, 1, 15, 16, 17, 16 * 37 + 7)}
MEMSET_CASES.update({"at_cap": ZERO_CAP * 16, "wrap_cap_plus_5_chunks": (ZERO_CAP + 5) * 16, "wrap_cap_plus_5_chunks_tail7": (ZERO_CAP + 5) * 16 + 7})


def randh(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).half()


# ----------------------------------------------------------------------------------------------------------------- channel_mix
# ddpm3d.py:559 `z = 1 / scale_factor * z` + autoencoder.py:105 post_quant_conv (1 x 1) + the shuffle to channels-last rows
def channel_mix(z, w, bias, Cpad, inv_scale, dtype=torch.float64, wrong=None):
    B, Cin, T, HW = z.shape
    Cout = w.shape[0]
    v = z.to(dtype) * inv_scale
    if wrong == "t_hw_swapped":
        v = v.reshape(B, Cin, HW, T).permute(0, 3, 2, 1)
    else:
        v = v.permute(0, 2, 3, 1)
    o = v.reshape(B * T * HW, Cin) @ w.to(dtype).t()
    if bias is not None:
        o = o + bias.to(dtype)
    out = torch.full((B * T * HW, Cpad), 1.0 if wrong == "pad_not_zeroed" else 0.0, dtype=dtype, device=z.device)
    out[:, :Cout] = o
    return out


MIX_CASES = {
    "f32_bias_cout4_cpad8": dict(B=2, Cin=4, T=3, HW=35, Cout=4, Cpad=8, f32=True, bias=True, inv_scale=1 / 0.18215, seed=601,
                                 wrongs=("t_hw_swapped", "pad_not_zeroed")),
    "f16_z": dict(B=2, Cin=4, T=3, HW=35, Cout=4, Cpad=8, f32=False, bias=True, inv_scale=1.0, seed=602, wrongs=("t_hw_swapped", "pad_not_zeroed")),
    "no_bias": dict(B=3, Cin=3, T=2, HW=9, Cout=5, Cpad=8, f32=True, bias=False, inv_scale=1.0, seed=603, wrongs=("t_hw_swapped", "pad_not_zeroed")),
    "cout_eq_cpad_cin8": dict(B=2, Cin=8, T=3, HW=5, Cout=8, Cpad=8, f32=True, bias=True, inv_scale=0.5, seed=604, wrongs=("t_hw_swapped",)),
    "wrap_cap_plus_300": dict(B=2, Cin=4, T=2, HW=WRAP4, Cout=4, Cpad=8, f32=False, bias=True, inv_scale=1.0, seed=605, wrongs=()),
}


def mix_inputs(c):
    g = gen(c["seed"])
    z = torch.randn(c["B"], c["Cin"], c["T"], c["HW"], generator=g) * 3
    z = z.half().float() if c["f32"] else z.half()        # (fp16-representable either way: both dtypes see the same values)
    w = torch.randn(c["Cout"], c["Cin"], generator=g) * 0.5
    return z, w, (torch.randn(c["Cout"], generator=g) if c["bias"] else None)


# ----------------------------------------------------------------------------------------------------------------- gaussian_sample
# lvdm/distributions.py:24-40 (clamp of the log variance, std = exp(0.5 logvar), mean + std * noise) and the `scale_factor *` of
# get_first_stage_encoding (ddpm3d.py:458-465); noise None = .mode()
def gaussian_sample(mom, noise, scale, dtype=torch.float64, wrong=None):
    n, z2, hw = mom.shape
    mean, lv = mom[:, :z2 // 2].to(dtype), mom[:, z2 // 2:].to(dtype)
    if noise is None:
        return scale * mean
    if wrong != "logvar_not_clamped":
        lv = torch.clamp(lv, -30.0, 20.0)
    return scale * (mean + torch.exp(0.5 * lv) * noise.to(dtype))


GAUSS_CASES = {
    "mode_no_noise": dict(n=2, z=4, hw=35, noise=False, lv="randn", scale=0.18215, seed=701, wrongs=()),
    "noise": dict(n=3, z=4, hw=35, noise=True, lv="randn", scale=0.18215, seed=702, wrongs=()),
    "logvar_at_the_clamps": dict(n=2, z=2, hw=12, noise=True, lv="clamps", scale=1.0, seed=703, wrongs=("logvar_not_clamped",)),
    "wrap_cap_plus_300": dict(n=2, z=2, hw=WRAP4, noise=True, lv="randn", scale=0.18215, seed=704, wrongs=()),
}


def gauss_inputs(c):
    g = gen(c["seed"])
    mom = torch.randn(c["n"], 2 * c["z"], c["hw"], generator=g)
    if c["lv"] == "clamps":                              # below, at, at, above the clamps of the reference
        mom[:, c["z"]:] = torch.tensor([-40.0, -30.0, 20.0, 25.0]).repeat(c["hw"] // 4)
    else:
        mom[:, c["z"]:] *= 2
    return mom, (torch.randn(c["n"], c["z"], c["hw"], generator=g) if c["noise"] else None)


# ----------------------------------------------------------------------------------------------------------------- embed_tokens
# condition.py:206-207: token_embedding(text) + positional_embedding; a token outside the vocabulary is clamped into it
def embed_tokens(tokens, table, pos, dtype=torch.float64, wrong=None):
    vocab, L = table.shape[0], pos.shape[0]
    t = torch.arange(tokens.shape[0], device=tokens.device)
    tok = tokens % vocab if wrong == "token_not_clamped" else tokens.clamp(0, vocab - 1)
    p = t.clamp(max=L - 1) if wrong == "position_without_wrap" else t % L
    return table.to(dtype)[tok] + pos.to(dtype)[p]


EMBED_CASES = {
    "tokens_outside_vocab_and_l_wrap": dict(n=200, L=77, C=72, vocab=300, seed=801, wrongs=("token_not_clamped", "position_without_wrap")),
    "one_row": dict(n=1, L=77, C=8, vocab=5, seed=802, wrongs=()),
    "wrap_cap_plus_300": dict(n=WRAP4, L=77, C=4, vocab=1000, seed=803, wrongs=()),
}


def embed_inputs(c):
    g = gen(c["seed"])
    tokens = torch.randint(0, c["vocab"], (c["n"],), generator=g)
    if c["n"] >= 100:
        tokens[[3, 50, 90]] = torch.tensor([-1, c["vocab"], c["vocab"] + 7])
    return tokens, torch.randn(c["vocab"], c["C"], generator=g), torch.randn(c["L"], c["C"], generator=g) * 0.1


# ----------------------------------------------------------------------------------------------------------------- DDIM arithmetic
def cfg_combine(e_c, e_u, scale, dtype=torch.float64):
    """ddim.py:304,372: e_t_uncond + scale * (e_t - e_t_uncond)"""
    e_c, e_u = e_c.to(dtype), e_u.to(dtype)
    return e_u + scale * (e_c - e_u)


def ddim_update(x, e, noise, a_t, a_prev, sigma_t, sqrt_one_minus_at, use_scale, scale_t, scale_prev, dtype=torch.float64):
    """ddim.py:331-356 with the reference's torch.full(...) scalars as 0-dim tensors of `dtype` built from the fp32 arguments"""
    sc = lambda v: torch.tensor(v, dtype=torch.float32, device=x.device).to(dtype)
    x, e, noise = x.to(dtype), e.to(dtype), noise.to(dtype)
    a_t, a_prev, sigma_t, s1m, scale_t, scale_prev = (sc(v) for v in (a_t, a_prev, sigma_t, sqrt_one_minus_at, scale_t, scale_prev))
    pred_x0 = (x - s1m * e) / a_t.sqrt()                                  # :339
    dir_xt = (1.0 - a_prev - sigma_t * sigma_t).sqrt() * e                # :343
    nz = sigma_t * noise                                                  # :345
    if use_scale:
        pred_x0 = pred_x0 / scale_t                                       # :353
        x_prev = a_prev.sqrt() * scale_prev * pred_x0 + dir_xt + nz       # :354
    else:
        x_prev = a_prev.sqrt() * pred_x0 + dir_xt + nz                    # :356
    return x_prev, pred_x0


DDIM_ARGS = dict(a_t=0.4137, a_prev=0.5023, sigma_t=0.2719, sqrt_one_minus_at=math.sqrt(1 - 0.4137), scale_t=0.7301, scale_prev=0.7713)
CFG_CASES = {"n1001_below_cap": dict(n=1001, scale=12.0, seed=901), "at_cap": dict(n=GRID_CAP, scale=7.5, seed=902),
             "wrap_cap_plus_300": dict(n=WRAP, scale=12.0, seed=903)}
DDIM_CASES = {"n1001_below_cap_use_scale0": dict(n=1001, use_scale=0, seed=911), "n1001_below_cap_use_scale1": dict(n=1001, use_scale=1, seed=912),
              "at_cap_use_scale1": dict(n=GRID_CAP, use_scale=1, seed=913),
              "wrap_cap_plus_300_use_scale0": dict(n=WRAP, use_scale=0, seed=914), "wrap_cap_plus_300_use_scale1": dict(n=WRAP, use_scale=1, seed=915)}


def randn_set(seed, n, count):
    g = gen(seed)
    return [torch.randn(n, generator=g) for _ in range(count)]


# ----------------------------------------------------------------------------------------------------------------- FreeInit
def freq_mix_3d(x, noise, lpf, wrong=None):
    """utils/freeinit_utils.py:7-47 on [C][T][H][W] in complex128, fftshift / ifftshift as the reference writes them"""
    dims = (-3, -2, -1)
    fft = torch.fft
    xf = fft.fftshift(fft.fftn(x.double(), dim=dims), dim=dims)
    nf = fft.fftshift(fft.fftn(noise.double(), dim=dims), dim=dims)
    lpf = lpf.double()
    mixed = xf * lpf + nf * (1 - lpf)
    mixed = (fft.fftshift if wrong == "fftshift_for_ifftshift" else fft.ifftshift)(mixed, dim=dims)
    return fft.ifftn(mixed, dim=dims).real


FREEINIT_CASES = {
    "c3_t1_h5_w7_below_cap": dict(shape=(3, 1, 5, 7), seed=1001, wrongs=("fftshift_for_ifftshift",)),
    "c2_t5_h9_w6_below_cap": dict(shape=(2, 5, 9, 6), seed=1002, wrongs=("fftshift_for_ifftshift",)),
    "wrap_c4_t5_h229_w229": dict(shape=(4, 5, 229, 229), seed=1003, wrongs=("fftshift_for_ifftshift",)),   # 1 048 820 bins > GRID_CAP, odd T, H, W
}


def freeinit_inputs(c):
    g = gen(c["seed"])
    C, T, H, W = c["shape"]
    return torch.randn(C, T, H, W, generator=g), torch.randn(C, T, H, W, generator=g), torch.rand(T, H, W, generator=g)


# ----------------------------------------------------------------------------------------------------------------- wrong restatements
MUTANTS = {
    "layout": ("t_hw_swapped", "cpad_as_cin", "pad_not_zeroed"),
    "silu_add_rows": ("div_a_div_b_exchanged",),
    "timestep_embedding": ("cos_sin_exchanged", "k_over_half_minus_1"),
    "layernorm": ("var_over_c_minus_1", "mean_drops_last_chunk", "eps_1e-6"),
    "softmax_rows": ("no_row_max", "scale_after_exp"),
    "freq_mix_3d": ("fftshift_for_ifftshift",),
    "gaussian_sample": ("logvar_not_clamped",),
    "embed_tokens": ("token_not_clamped", "position_without_wrap"),
}

# ----------------------------------------------------------------------------------------------------------------- ledger
# every entry point of lib.SIGNATURES: the GPU tests ("module::test") that launch it and check what it computed, or why none does
_S = "test_small_kernels_gpu::"
N_ = "test_norm_edges_gpu::"
K_ = "test_step_kernels_gpu::"
F_ = "test_gemm_fused_gpu::"
LEDGER = {
    "moca_gemm_f16": ["test_gemm_edges_gpu::test_index_probe", "test_gemm_edges_gpu::test_geometry_random_operands", "test_kernels_gpu::test_gemm_linear",
                      F_ + "test_ln_store_loop", F_ + "test_fold_tiled_routes", F_ + "test_fold_persistent_routes", F_ + "test_two_source_a", F_ + "test_wgroup",
                      F_ + "test_gstat_virtual_concat", F_ + "test_tattn"],
    "moca_gemm_colsum_rows": ["test_gemm_edges_gpu::test_statistics_at_m_tail", "test_kernels_gpu::test_gemm_colsum_feeds_groupnorm"],
    "moca_gemm_ln_ok": ["test_kernels_gpu::test_gemm_layernorm_epilogue", F_ + "test_ln_store_loop"],
    "moca_gemm_rowsum_cols": ["test_gemm_edges_gpu::test_epilogue_matrix", "test_kernels_gpu::test_gemm_rowsum_feeds_lnfold"],
    "moca_gemm_lnfold_ok": ["test_kernels_gpu::test_gemm_rowsum_feeds_lnfold", "test_kernels_gpu::test_gemm_lnfold_offset_rows",
                            F_ + "test_fold_tiled_routes", F_ + "test_fold_persistent_routes", F_ + "test_tattn"],
    "moca_gemm_tattn_ok": ["test_kernels_gpu::test_gemm_temporal_attention_fused", F_ + "test_tattn", F_ + "test_tattn_refused"],
    "moca_gemm_cat_ok": ["test_kernels_gpu::test_gemm_two_source_a", F_ + "test_two_source_a"],
    "moca_gemm_wgroup_ok": ["test_gemm_edges_gpu::test_wgroup_never_on_persistent_kernels", "test_kernels_gpu::test_gemm_groupnorm_folded_into_per_group_weights",
                            F_ + "test_wgroup", F_ + "test_ln_store_loop"],
    "moca_gemm_route": ["test_gemm_edges_gpu::test_wgroup_never_on_persistent_kernels", F_ + "test_ln_store_loop", F_ + "test_fold_tiled_routes",
                        F_ + "test_two_source_a", F_ + "test_tattn"],
    "moca_groupnorm_fold_weights_f16": ["test_groupnorm_gpu::test_gemm_groupnorm_fold_constant_group_and_poison",
                                        "test_kernels_gpu::test_gemm_groupnorm_folded_into_per_group_weights", N_ + "test_fold_weights_edges"],
    "moca_gemm_splitk_groupnorm_ok": ["test_groupnorm_gpu::test_gemm_splitk_groupnorm_large_group_mean"],
    "moca_gemm_splitk_groupnorm_f16": ["test_groupnorm_gpu::test_gemm_splitk_groupnorm_large_group_mean", "test_kernels_gpu::test_gemm_splitk_groupnorm"],
    "moca_groupnorm_gstat_cat_f16": ["test_groupnorm_gpu::test_groupnorm_from_gstat_accum_and_concat", "test_kernels_gpu::test_groupnorm_virtual_cat", N_ + "test_spike_probe", N_ + "test_streaming_store_variants"],
    "moca_gstat_accum_f16": ["test_groupnorm_gpu::test_groupnorm_from_gstat_accum_and_concat", N_ + "test_spike_probe", N_ + "test_accumulators_exact"],
    "moca_groupnorm_colsum_f16": ["test_groupnorm_gpu::test_groupnorm_from_gemm_column_sums_and_tiled_gstat", "test_kernels_gpu::test_gemm_colsum_feeds_groupnorm", N_ + "test_spike_probe"],
    "moca_groupnorm_nhwc_f16": ["test_groupnorm_gpu::test_groupnorm_large_group_mean", "test_kernels_gpu::test_groupnorm", N_ + "test_spike_probe", N_ + "test_surroundings"],
    "moca_groupnorm_ws_bytes": ["test_groupnorm_gpu::test_groupnorm_large_group_mean", "test_kernels_gpu::test_groupnorm", N_ + "test_surroundings"],
    "moca_groupnorm_route": [N_ + "test_spike_probe"],        # host query: asserted before every standalone launch, which then must be right
    "moca_groupnorm_nchunk": [N_ + "test_spike_probe", N_ + "test_streaming_store_variants"],   # host query: places the probes of every chunked kernel
    "moca_groupnorm_gstat_f16": ["test_groupnorm_gpu::test_groupnorm_from_320_gstat", "test_kernels_gpu::test_groupnorm_gstat_rejects_misaligned_affine_parameters", N_ + "test_spike_probe", N_ + "test_streaming_store_variants"],
    "moca_memset_zero": [_S + "test_memset_zero"],
    "moca_concat_channels_gstat_f16": ["test_groupnorm_gpu::test_groupnorm_from_gstat_accum_and_concat", "test_kernels_gpu::test_concat_with_groupnorm_statistics", N_ + "test_accumulators_exact", N_ + "test_streaming_store_variants"],
    "moca_layernorm_f16": [_S + "test_layernorm", _S + "test_layernorm_gamma_zero", "test_kernels_gpu::test_layernorm"],
    "moca_attention_f16": ["test_kernels_gpu::test_attention", "test_attention_edges_gpu::test_logit_regimes"],
    "moca_attention_ip_f16": ["test_i2v_gpu::test_attention_ip_segment_maxima_differ", "test_i2v_gpu::test_attention_ip_without_image_tokens_is_attention"],
    "moca_attention_causal_f16": ["test_attention_edges_gpu::test_xcd_remap_causal", "test_kernels_gpu::test_attention_causal"],
    "moca_embed_tokens_f16": [_S + "test_embed_tokens", "test_kernels_gpu::test_gemm_gelu_epilogue_and_token_embedding"],
    "moca_attention_d80_f16": ["test_clip_vision_gpu::test_attention_d80_vs_fp32", "test_attention_edges_gpu::test_logit_regimes"],
    "moca_clip_preprocess_patches_f16": ["test_clip_vision_gpu::test_preprocess_patches_vs_restatement"],
    "moca_clip_assemble_tokens_f16": ["test_clip_vision_gpu::test_reduced_tower_vs_restatement"],
    "moca_temporal_attention_f16": ["test_kernels_gpu::test_temporal_attention"],
    "moca_temporal_attention_causal_f16": ["test_temporal_variants_gpu::test_causal_temporal_attention_kernel"],
    "moca_temporal_attention_long_f16": ["test_long_frames_gpu::test_long_temporal_attention_kernel"],
    "moca_ncthw_to_nhwc_f16": [_S + "test_ncthw_to_nhwc", "test_kernels_gpu::test_layout_roundtrip_and_concat"],
    "moca_ncthw_scatter_f16": ["test_hybrid_gpu::test_scatter_kernel"],
    "moca_nchw_add_rows_f16": ["test_adapter_gpu::test_add_rows_kernel_is_one_correctly_rounded_sum"],
    "moca_nhwc_to_ncthw": [_S + "test_nhwc_to_ncthw", "test_kernels_gpu::test_layout_roundtrip_and_concat"],
    "moca_concat_channels_f16": [_S + "test_concat_channels", "test_kernels_gpu::test_layout_roundtrip_and_concat"],
    "moca_repeat_f16": [_S + "test_repeat"],
    "moca_timestep_embedding_f16": [_S + "test_timestep_embedding", "test_kernels_gpu::test_timestep_embedding_and_silu_rows"],
    "moca_silu_add_rows_f16": [_S + "test_silu_add_rows", "test_kernels_gpu::test_timestep_embedding_and_silu_rows"],
    "moca_channel_mix_f16": [_S + "test_channel_mix"],
    "moca_softmax_rows_f16": [_S + "test_softmax_rows"],
    "moca_gaussian_sample_f32": [_S + "test_gaussian_sample"],
    "moca_cfg_combine_f32": [_S + "test_cfg_combine", "test_loops_gpu::test_fifo_step_windows_equals_per_window_kernel"],
    "moca_ddim_update_f32": [_S + "test_ddim_update", "test_sampler_gpu::test_p_sample_ddim_cfg"],
    "moca_q_sample_f32": ["test_v2v_gpu::test_q_sample_kernel_bit_equal_to_torch"],
    "moca_fifo_ddim_step_f32": ["test_loops_gpu::test_fifo_step_windows_equals_per_window_kernel", "test_sampler_gpu::test_ddim_step_moca", K_ + "test_moca_step"],
    "moca_fifo_randn_f32": ["test_loops_gpu::test_fifo_randn_kernel_is_philox_box_muller", K_ + "test_randn"],
    "moca_fifo_gather_windows_f32": ["test_loops_gpu::test_fifo_graph_iteration_vs_reference_golden_masks", K_ + "test_gather_windows"],
    "moca_fifo_step_windows_f32": ["test_loops_gpu::test_fifo_step_windows_equals_per_window_kernel", K_ + "test_step_windows"],
    "moca_sam_select_masks_f32": ["test_loops_gpu::test_sam_select_kernel_equals_host_bookkeeping", K_ + "test_sam_select_scripted"],
    "moca_fifo_advance_f32": ["test_loops_gpu::test_fifo_step_windows_equals_per_window_kernel", K_ + "test_advance"],
    "moca_fifo_prepare_queue_f32": ["test_sampler_gpu::test_fifo_queue", K_ + "test_prepare_queue"],
    "moca_base_set_timestep": ["test_loops_gpu::test_base_step_graph_equals_p_sample_ddim", K_ + "test_base_set_timestep"],
    "moca_base_ddim_step_f32": ["test_loops_gpu::test_base_step_graph_equals_p_sample_ddim", K_ + "test_base_step"],
    "moca_ddpm_step_f32": ["test_ddpm_gpu::test_ddpm_step_kernel_bit_equal_to_torch"],
    "moca_mask_frame_sums_f32": ["test_loops_gpu::test_fifo_step_windows_equals_per_window_kernel", K_ + "test_mask_frame_sums", K_ + "test_moca_step"],
    "moca_freq_mix_3d_f32": [_S + "test_freq_mix_3d", "test_sampler_gpu::test_freeinit_filters_and_mix"],
    "moca_freq_mix_ws_bytes": [_S + "test_freq_mix_3d"],
    "moca_freq_filter_f32": ["test_sampler_gpu::test_freeinit_filters_and_mix", K_ + "test_freq_filter"],
}
LEDGER_EXEMPT = {
    "moca_gemm_splitk_ws_bytes": "size query, no launch: its value is asserted on the CPU (test_gemm_edges_cpu::test_normalise_splits, test_abi_cpu)",
    "moca_graph_begin": "graph: capture and replay are exercised by every engine test (test_loops_gpu), there is nothing per element to compare",
    "moca_graph_end": "graph", "moca_graph_launch": "graph", "moca_graph_destroy": "graph",
    "moca_stream_create": "stream", "moca_stream_destroy": "stream", "moca_stream_sync": "stream",
    "moca_event_create": "event", "moca_event_record": "event", "moca_event_elapsed_ms": "event", "moca_event_destroy": "event",
    "moca_set_tuning": "tuning: chooses a kernel, never a result; return codes asserted in test_abi_cpu",
    "moca_debug_clock_sampler": "diagnostic: a measurement aid of tools/, computes nothing the product reads",
    "moca_device_info": "device info",
    "moca_version": "device info: the build string, asserted in test_abi_cpu",
}
