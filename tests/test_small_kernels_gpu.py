"""GPU: the small kernels -- csrc/elementwise.hip, the LayerNorm of csrc/norm.hip, moca_memset_zero, moca_gaussian_sample_f32, the plain
DDIM arithmetic kernels, the FreeInit DFT -- element by element against the float64 restatements of tests/small_kernels_ref.py, at the
grid-stride wrap (more work items than 4096 blocks of 256: a thread loops), at the tails, strides, dtypes and argument variants the
whole-model tests never reach.

fp16 outputs: every element within bound(ref, slack) = 2^-10 |ref| + 2^-24 + slack (one fp16 ulp, the subnormal step, twice the error
of plain fp32 torch on the same inputs, measured on the spot).  fp32 mul/add/sub/div kernels: torch.equal with the fp32 torch expression.
Layout, concat, repeat, memset: exact.  Every output buffer carries sentinel rows behind its end and sentinel columns [C, ld) where
it has a row stride; they must come back untouched.  Inputs come from the case's seed on the CPU (the CPU file sees the same)."""
import ctypes as C

import pytest
import torch

import small_kernels_ref as R

pytestmark = pytest.mark.gpu

from moca_video_amd import lib as L  # noqa: E402
from moca_video_amd import ops  # noqa: E402

DEV = "cuda"
S16 = -7776.0                      # sentinel, exact in fp16 and fp32
F16, F32, F64 = torch.float16, torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _stream():
    ops.set_stream(None)
    yield
    torch.cuda.synchronize()


def cases(table):
    return pytest.mark.parametrize("name", list(table))


def guarded(rows, cols, dtype=F16, ld=None, tail=3):
    """a sentinel-filled buffer [rows + tail][ld] and the [rows][cols] window a kernel may write"""
    full = torch.full((rows + tail, ld or cols), S16, dtype=dtype, device=DEV)
    return full, full[:rows, :cols]


def guards_intact(full, rows, cols):
    assert (full[rows:] == S16).all(), "rows behind the end of the output were written"
    assert (full[:rows, cols:] == S16).all(), "columns [C, ld) of the output were written"


def within(got, ref, slack, what, bound_fn=R.bound):
    r = R.ratio(got, ref, slack, bound_fn)
    w = r.max().item()
    print(f"[small] {what}: worst |err| / bound {w:.3f} (slack {slack:.2e})")
    if w > 1.0:
        flat = r.reshape(-1)
        i = int(flat.argmax())
        n_bad = int((flat > 1).sum())
        raise AssertionError(f"{what}: {n_bad} of {flat.numel()} elements outside the bound, worst {w:.2f} x at flat index {i} "
                             f"(got {got.reshape(-1)[i].item()!r}, ref {ref.reshape(-1)[i].item()!r}; wrap edge items {R.edge_items(flat.numel())[:3]})")


def exact(got, ref, what):
    if not torch.equal(got, ref):
        bad = (got != ref).reshape(-1).nonzero()
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ, first at flat index {int(bad[0])}, last at {int(bad[-1])}")


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@cases({k: v for k, v in R.LN_CASES.items() if not v["gamma0"]})
def test_layernorm(name):
    c = R.LN_CASES[name]
    x, gamma, beta = (t.to(DEV) for t in R.ln_inputs(c))
    M, Cn = c["M"], c["C"]
    full, y = guarded(M, Cn)
    ops.layernorm(x, y, gamma, beta, M=M, Cn=Cn, eps=c["eps"])
    ref = R.layernorm(x, gamma, beta, c["eps"])
    slack = R.slack_of(R.layernorm(x, gamma, beta, c["eps"], F32), ref)
    within(y, ref, slack, f"layernorm {name}")
    guards_intact(full, M, Cn)


@cases({k: v for k, v in R.LN_CASES.items() if v["gamma0"]})
def test_layernorm_gamma_zero(name):
    """gamma = 0: whatever the statistics are, the output is fp16(beta) exactly (and never NaN)"""
    c = R.LN_CASES[name]
    x, gamma, beta = (t.to(DEV) for t in R.ln_inputs(c))
    M, Cn = c["M"], c["C"]
    full, y = guarded(M, Cn)
    ops.layernorm(x, y, gamma, beta, M=M, Cn=Cn, eps=c["eps"])
    exact(y, beta.half()[None].expand(M, Cn), f"layernorm {name}")
    guards_intact(full, M, Cn)


# ---------------------------------------------------------------------------------------------------------------- softmax
@cases(R.SOFTMAX_CASES)
def test_softmax_rows(name):
    c = R.SOFTMAX_CASES[name]
    Rr, N = c["R"], c["N"]
    lds, ldp = N + 4, N + 8
    s = R.softmax_inputs(c).to(DEV)
    s_full = torch.full((Rr, lds), 3e38, dtype=F32, device=DEV)          # (a logit read past N would be the row maximum)
    s_full[:, :N] = s
    full, p = guarded(Rr, N, ld=ldp)
    ops.softmax_rows(s_full[:, :N], p, R=Rr, N=N, scale=c["scale"])
    ref = R.softmax_rows(s, c["scale"])
    slack = R.slack_of(R.softmax_rows(s, c["scale"], F32), ref)
    within(p, ref, slack, f"softmax_rows {name}")
    rs = ((p.double().sum(-1) - 1).abs() / R.softmax_sum_bound(ref, N, slack)).max().item()
    print(f"[small] softmax_rows {name}: row sums {rs:.3f} of their bound")
    assert rs <= 1.0, f"softmax_rows {name}: row sums {rs:.2f} of their bound"
    if c["fill"] == "one_finite":
        assert (p.max(-1).values == 1.0).all() and (p.sum(-1) == 1.0).all(), "a row with one finite logit is exactly one-hot"
    guards_intact(full, Rr, N)


# ---------------------------------------------------------------------------------------------------------------- elementwise
@cases(R.SILU_CASES)
def test_silu_add_rows(name):
    c = R.SILU_CASES[name]
    a, b = R.silu_inputs(c)
    a, b = a.to(DEV), (b.to(DEV) if b is not None else None)
    rows, Cn = c["rows"], c["C"]
    full, out = guarded(rows, Cn)
    ops.silu_add_rows(a, c["div_a"], b, c["div_b"], out, rows=rows, Cn=Cn, silu=c["silu"])
    ev = lambda dt: R.silu_add_rows(a, c["div_a"], b, c["div_b"] or 1, rows, c["silu"], dt)
    ref = ev(F64)
    assert torch.isfinite(out).all(), "silu_add_rows: non-finite output"
    within(out, ref, R.slack_of(ev(F32), ref), f"silu_add_rows {name}")
    guards_intact(full, rows, Cn)


@cases(R.TIMESTEP_CASES)
def test_timestep_embedding(name):
    c = R.TIMESTEP_CASES[name]
    t = R.timestep_inputs(c).to(DEV)
    n, dim = c["n"], c["dim"]
    full, out = guarded(n, dim)
    ops.timestep_embedding(t, out, n=n, dim=dim, max_period=float(c["max_period"]))
    ref = R.timestep_embedding(t, dim, c["max_period"])
    within(out, ref, R.slack_of(R.timestep_embedding(t, dim, c["max_period"], F32), ref), f"timestep_embedding {name}")
    if dim % 2:
        assert (out[:, -1] == 0).all()
    guards_intact(full, n, dim)


@cases(R.MIX_CASES)
def test_channel_mix(name):
    c = R.MIX_CASES[name]
    z, w, bias = R.mix_inputs(c)
    z, w, bias = z.to(DEV), w.to(DEV), (bias.to(DEV) if bias is not None else None)
    rows = c["B"] * c["T"] * c["HW"]
    full, out = guarded(rows, c["Cpad"])
    ops.channel_mix(z, w, bias, out, B=c["B"], Cin=c["Cin"], T=c["T"], HW=c["HW"], Cout=c["Cout"], Cpad=c["Cpad"], inv_scale=c["inv_scale"])
    ref = R.channel_mix(z, w, bias, c["Cpad"], c["inv_scale"])
    within(out, ref, R.slack_of(R.channel_mix(z, w, bias, c["Cpad"], c["inv_scale"], F32), ref), f"channel_mix {name}")
    assert (out[:, c["Cout"]:] == 0).all(), "pad columns are zero"
    guards_intact(full, rows, c["Cpad"])


@cases(R.EMBED_CASES)
def test_embed_tokens(name):
    c = R.EMBED_CASES[name]
    tokens, table, pos = (t.to(DEV) for t in R.embed_inputs(c))
    n, Cn = c["n"], c["C"]
    full, out = guarded(n, Cn)
    ops.embed_tokens(tokens, table, pos, out, n_tokens=n, L=c["L"], Cn=Cn, vocab=c["vocab"])
    ref = R.embed_tokens(tokens, table, pos)
    within(out, ref, R.slack_of(R.embed_tokens(tokens, table, pos, F32), ref), f"embed_tokens {name}")
    guards_intact(full, n, Cn)


@cases(R.GAUSS_CASES)
def test_gaussian_sample(name):
    c = R.GAUSS_CASES[name]
    mom, noise = R.gauss_inputs(c)
    mom, noise = mom.to(DEV), (noise.to(DEV) if noise is not None else None)
    n, z, hw = c["n"], c["z"], c["hw"]
    full, out = guarded(1, n * z * hw, dtype=F32)
    ops.gaussian_sample(mom, noise, out, n=n, z=z, hw=hw, scale=c["scale"])
    got = out.view(n, z, hw)
    f32 = R.gaussian_sample(mom, noise, c["scale"], F32)
    if noise is None:
        exact(got, f32, f"gaussian_sample {name} (the mode: one fp32 product)")
    else:
        ref = R.gaussian_sample(mom, noise, c["scale"])
        within(got, ref, R.slack_of(f32, ref), f"gaussian_sample {name}", R.bound_f32_exp)
    guards_intact(full, 1, n * z * hw)


# ---------------------------------------------------------------------------------------------------------------- DDIM arithmetic
@cases(R.CFG_CASES)
def test_cfg_combine(name):
    c = R.CFG_CASES[name]
    ec, eu = (t.to(DEV) for t in R.randn_set(c["seed"], c["n"], 2))
    full, out = guarded(1, c["n"], dtype=F32)
    L.check(L.load().moca_cfg_combine_f32(L.ptr(ec), L.ptr(eu), L.ptr(out), c["scale"], c["n"], None), "moca_cfg_combine_f32")
    exact(out[0], R.cfg_combine(ec, eu, c["scale"], F32), f"cfg_combine {name}")
    guards_intact(full, 1, c["n"])


@cases(R.DDIM_CASES)
def test_ddim_update(name):
    c = R.DDIM_CASES[name]
    n, a = c["n"], R.DDIM_ARGS
    x, e, nz = (t.to(DEV) for t in R.randn_set(c["seed"], n, 3))
    full_p, xp = guarded(1, n, dtype=F32)
    full_0, p0 = guarded(1, n, dtype=F32)
    L.check(L.load().moca_ddim_update_f32(L.ptr(x), L.ptr(e), L.ptr(nz), L.ptr(xp), L.ptr(p0), a["a_t"], a["a_prev"], a["sigma_t"],
                                          a["sqrt_one_minus_at"], c["use_scale"], a["scale_t"], a["scale_prev"], n, None), "moca_ddim_update_f32")
    want_xp, want_p0 = R.ddim_update(x, e, nz, use_scale=c["use_scale"], dtype=F32, **a)
    exact(p0[0], want_p0, f"ddim_update {name} pred_x0")
    exact(xp[0], want_xp, f"ddim_update {name} x_prev")
    guards_intact(full_p, 1, n)
    guards_intact(full_0, 1, n)


# ---------------------------------------------------------------------------------------------------------------- layout and copies
@cases(R.TO_NHWC_CASES)
def test_ncthw_to_nhwc(name):
    c = R.TO_NHWC_CASES[name]
    x = torch.randn(c["B"], c["Cin"], c["T"], c["HW"], generator=R.gen(c["seed"]))
    x = (x if c["f32"] else x.half()).to(DEV)
    rows = c["B"] * c["T"] * c["HW"]
    full, y = guarded(rows, c["Cpad"])
    ops.ncthw_to_nhwc(x, y, B=c["B"], Cin=c["Cin"], T=c["T"], HW=c["HW"], Cpad=c["Cpad"])
    exact(y, R.ncthw_to_nhwc(x, c["Cpad"]), f"ncthw_to_nhwc {name}")
    guards_intact(full, rows, c["Cpad"])


@cases(R.FROM_NHWC_CASES)
def test_nhwc_to_ncthw(name):
    c = R.FROM_NHWC_CASES[name]
    B, Cout, T, HW = c["B"], c["Cout"], c["T"], c["HW"]
    y = R.randh(R.gen(c["seed"]), B * T * HW, c["ld"]).to(DEV)
    dt = F32 if c["f32"] else F16
    n = B * Cout * T * HW
    full, x = guarded(1, n, dtype=dt)
    ops.nhwc_to_ncthw(y, c["ld"], x, B=B, Cout=Cout, T=T, HW=HW)
    exact(x.view(B, Cout, T, HW), R.nhwc_to_ncthw(y, B, Cout, T, HW, dt), f"nhwc_to_ncthw {name}")
    guards_intact(full, 1, n)


@cases(R.CONCAT_CASES)
def test_concat_channels(name):
    c = R.CONCAT_CASES[name]
    g = R.gen(c["seed"])
    a, b = R.randh(g, c["rows"], c["C1"]).to(DEV), R.randh(g, c["rows"], c["C2"]).to(DEV)
    full, out = guarded(c["rows"], c["C1"] + c["C2"])
    ops.concat_channels(a, b, out, rows=c["rows"], C1=c["C1"], C2=c["C2"])
    exact(out, torch.cat([a, b], 1), f"concat_channels {name}")
    guards_intact(full, c["rows"], c["C1"] + c["C2"])


@cases(R.REPEAT_CASES)
def test_repeat(name):
    c = R.REPEAT_CASES[name]
    n16, reps = c["n16"], c["reps"]
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n16 * 4,), generator=R.gen(c["seed"]), dtype=torch.int64).to(torch.int32).to(DEV)
    full = torch.full((reps * n16 * 4 + 16,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    L.check(L.load().moca_repeat_f16(L.ptr(src), L.ptr(full), n16 * 16, reps, None), "moca_repeat_f16")
    exact(full[:reps * n16 * 4], src.repeat(reps), f"repeat {name}")
    assert (full[reps * n16 * 4:] == 0x5A5A5A5A).all(), "bytes behind the last copy were written"


@cases(R.MEMSET_CASES)
def test_memset_zero(name):
    n = R.MEMSET_CASES[name]
    full = torch.full((16 + n + 32,), 0xAB, dtype=torch.uint8, device=DEV)
    assert full.data_ptr() % 16 == 0
    L.check(L.load().moca_memset_zero(C.c_void_p(full.data_ptr() + 16), n, None), "moca_memset_zero")
    assert (full[:16] == 0xAB).all() and (full[16 + n:] == 0xAB).all(), "bytes outside [ptr, ptr + bytes) were written"
    exact(full[16:16 + n], torch.zeros(n, dtype=torch.uint8, device=DEV), f"memset_zero {name}")


# ---------------------------------------------------------------------------------------------------------------- FreeInit
@cases(R.FREEINIT_CASES)
def test_freq_mix_3d(name):
    c = R.FREEINIT_CASES[name]
    Cc, T, H, W = c["shape"]
    x, noise, lpf = (t.to(DEV) for t in R.freeinit_inputs(c))
    lib = L.load()
    ws_bytes = int(lib.moca_freq_mix_ws_bytes(Cc, T, H, W))
    assert ws_bytes == 2 * 2 * Cc * T * H * W * 8
    ws = torch.empty(ws_bytes // 4, dtype=F32, device=DEV)
    n = Cc * T * H * W
    full, out = guarded(1, n, dtype=F32)
    L.check(lib.moca_freq_mix_3d_f32(L.ptr(x), L.ptr(noise), L.ptr(lpf), L.ptr(out), Cc, T, H, W, L.ptr(ws), None), "moca_freq_mix_3d_f32")
    ref = R.freq_mix_3d(x, noise, lpf).reshape(-1)
    err = (out[0].double() - ref).abs()
    e = (err.max() / ref.abs().max()).item()
    e_edge = (err[R.edge_items(n)].max() / ref.abs().max()).item()
    print(f"[small] freq_mix_3d {name}: max|err| / max|ref| {e:.2e} (wrap edge items {e_edge:.2e})")
    assert e <= R.FREEINIT_TOL, f"freq_mix_3d {name}: {e:.2e} of max|ref|, worst at flat index {int(err.argmax())}"
    guards_intact(full, 1, n)
