"""Operands, layouts and float64 torch restatements for tests/test_attention_edges_gpu.py; at the end, the cases whose outputs
tests/test_attention_parent_gpu.py pins by hash against the parent commit.

Every reference works on the fp16-rounded operands it is handed (any strides, any device) and returns float64; the metric is taken
per (batch, head) slice so that a wrong slice cannot hide under another slice's maximum.  Nothing here touches a GPU by itself:
the builders make their tensors on the CPU from a seeded generator and the caller moves them."""
import torch

L2E = 1.4426950408889634
TOL16 = 3e-3                    # tests/test_kernels_gpu.py: one fp16-output kernel against torch on the same fp16 operands
NAN = float("nan")


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randh(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).half()


# ---------------------------------------------------------------- references (float64), one per entry point
def _heads(t, heads, D):
    B, N = t.shape[0], t.shape[1]
    return t.double().reshape(B, N, heads, D).permute(0, 2, 1, 3)                  # [B, heads, N, D]


def scores(q, k, heads, kv_div, scale, D=64):
    """float64 logits [Bq, heads, Nq, Nk] in natural-log units"""
    return _heads(q, heads, D) @ _heads(k, heads, D).repeat_interleave(kv_div, 0).transpose(-1, -2) * scale


def ref_plain(q, k, v, heads, kv_div, scale, D=64, causal=False):
    """softmax(q k^T scale) v; q [Bq, Nq, C], k / v [Bq / kv_div, Nk, C] -> [Bq, Nq, C]"""
    s = scores(q, k, heads, kv_div, scale, D)
    if causal:
        Nq, Nk = s.shape[-2:]
        s = s.masked_fill(torch.ones(Nq, Nk, device=s.device).triu(1) > 0.5, float("-inf"))
    o = s.softmax(-1) @ _heads(v, heads, D).repeat_interleave(kv_div, 0)
    return o.permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[1], heads * D)


def ref_ip(q, k, v, ki, vi, heads, kv_div, scale, ip_scale):
    """the two-softmax image cross-attention of tests/test_i2v_gpu.py::ip_ref"""
    return ref_plain(q, k, v, heads, kv_div, scale) + ip_scale * ref_plain(q, ki, vi, heads, kv_div, scale)


def ref_causal(q, k, v, heads, scale):
    return ref_plain(q, k, v, heads, 1, scale, causal=True)


def ref_d80(q, k, v, heads, scale):
    return ref_plain(q, k, v, heads, 1, scale, D=80)


def from_tokens(x, B, T, HW):
    """channels-last token rows [(b T + t) HW + p][C] -> one attention problem per pixel [B HW, T, C]"""
    return x.reshape(B, T, HW, x.shape[-1]).permute(0, 2, 1, 3).reshape(B * HW, T, x.shape[-1])


def to_tokens(x, B, T, HW):
    return x.reshape(B, HW, T, x.shape[-1]).permute(0, 2, 1, 3).reshape(B * T * HW, x.shape[-1])


def ref_temporal(q, k, v, B, T, HW, heads, scale, causal):
    """attention over the frames of every (video, pixel, head), with the layout gather; token rows in, token rows out"""
    o = ref_plain(from_tokens(q, B, T, HW), from_tokens(k, B, T, HW), from_tokens(v, B, T, HW), heads, 1, scale, causal=causal)
    return to_tokens(o, B, T, HW)


# ---------------------------------------------------------------- metric
def slice_errors(got, ref, nb, heads, D=64):
    """max|got - ref| / max|ref| per (batch, head) slice -> [nb, heads]; got / ref are [nb * rows, C] or [nb, rows, C]"""
    g = got.double().reshape(nb, -1, heads, D)
    r = ref.double().reshape(nb, -1, heads, D)
    return (g - r).abs().amax((1, 3)) / r.abs().amax((1, 3)).clamp_min(1e-30)


def check_slices(got, ref, nb, heads, what, D=64, tol=TOL16):
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    e = slice_errors(got, ref, nb, heads, D)
    worst = e.max().item()
    print(f"[parity] {what}: worst (batch, head) slice {worst:.2e} of its max|ref| (bound {tol:.1e})")
    assert worst <= tol, f"{what}: slice errors {e.tolist()}"
    return worst


# ---------------------------------------------------------------- layouts
def packed(g, rows, widths, pad=8, extra=0, poison=NAN, dev="cpu", data=None):
    """One buffer [rows + extra][sum(widths) + pad] holding unit Gaussian operands side by side; the pad columns and the `extra`
    rows after the operands hold `poison`.  Returns (buffer, [column view [rows, w] per width], row stride)."""
    W = sum(widths)
    buf = torch.full((rows + extra, W + pad), poison, dtype=torch.float16)
    buf[:rows, :W] = randh(g, rows, W) if data is None else data
    buf = buf.to(dev)
    views, off = [], 0
    for w in widths:
        views.append(buf[:rows, off:off + w])
        off += w
    return buf, views, W + pad


def canary_out(rows, C, dev, pad=8, guard=4):
    """NaN-filled [guard + rows + guard][C + pad]; the output is the column view [rows, C] that starts at column 0 of row `guard`"""
    buf = torch.full((rows + 2 * guard, C + pad), NAN, dtype=torch.float16, device=dev)
    return buf, buf[guard:guard + rows, :C], C + pad


def assert_canary(buf, rows, C, what, guard=4):
    assert torch.isnan(buf[:guard]).all(), f"{what}: a store landed in the guard rows before the output"
    assert torch.isnan(buf[guard + rows:]).all(), f"{what}: a store landed in the guard rows after the output"
    assert torch.isnan(buf[guard:guard + rows, C:]).all(), f"{what}: a store landed in the pad columns"


# ---------------------------------------------------------------- logit regimes (tests/test_kernels_gpu.py::test_attention_reference_regimes)
REGIMES = ("low", "high", "late_peak", "mixed", "band_edge")
REGIME_TARGET = {"low": -14.0, "high": 11.0, "mixed": -14.0, "band_edge": 6.0}       # log2 units


def apply_regime(regime, q, ks, scale, D, peaks, kv_div=1):
    """In place on CPU fp16 operands q [Bq, Nq, C] and the key tensors of `ks` = [(k [Bk, Nk, C], c0), ...].
    low / high / mixed / band_edge: every score of the selected query rows (all; `mixed`: every third) against a key of segment i moves
    by c0_i * target log2 units: channel 0 of every head of q holds the shift, channel 0 of every key c0_i.
    late_peak: `peaks` = [(segment, key, query row, gain), ...] sets key <- gain * that query row: one key far above the rest."""
    if regime == "late_peak":
        for seg, key, row, gain in peaks:
            ks[seg][0][:, key] = q[::kv_div, row] * gain
        return
    shift = REGIME_TARGET[regime] / (scale * L2E)
    rows = slice(None) if regime != "mixed" else slice(0, q.shape[1], 3)
    for k, c0 in ks:
        k[..., 0::D] = c0
    q[:, rows, 0::D] = shift


# ---------------------------------------------------------------- one-hot softmax
def hot_keys(Nq, Nk, heads, causal=False):
    """[Nq, heads]: the hot key of query row r in head h is (7 r + 3 h + 1) % Nk; causal: min(that, r)"""
    r = torch.arange(Nq)[:, None]
    hot = (7 * r + 3 * torch.arange(heads)[None, :] + 1) % Nk
    return torch.minimum(hot, r.expand_as(hot)) if causal else hot


def onehot_operands(g, Bq, Nq, Nk, heads, kv_div, hot, D=64, amp=4.0):
    """K rows are amp * (+-1 code vectors), one random code per (kv batch, head, key); the query row (b, r, h) is amp * the code of
    its hot key, so its hot score is amp^2 D and every other score amp^2 (code . code') -- the gap is asserted by the caller from
    the float64 reference (onehot_gap).  V is unit Gaussian.  Returns q [Bq, Nq, C], k, v [Bk, Nk, C] and the expected output
    [Bq, Nq, C]: the V row of the hot key, bit for bit."""
    Bk = Bq // kv_div
    codes = (torch.randint(0, 2, (Bk, heads, Nk, D), generator=g) * 2 - 1).half() * amp
    vh = randh(g, Bk, heads, Nk, D)
    idx = hot.t()[None, :, :, None].expand(Bq, heads, Nq, D)
    pick = lambda t: torch.gather(t.repeat_interleave(kv_div, 0), 2, idx)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], heads * D).contiguous()
    return flat(pick(codes)), flat(codes), flat(vh), flat(pick(vh))


def onehot_gap(q, k, heads, kv_div, scale, hot, D=64, causal=False):
    """smallest distance, in log2 units, between a query's hot score and its largest other (unmasked) score"""
    s = scores(q, k, heads, kv_div, scale, D) * L2E
    Nq, Nk = s.shape[-2:]
    if causal:
        s = s.masked_fill(torch.ones(Nq, Nk, device=s.device).triu(1) > 0.5, float("-inf"))
    idx = hot.t()[None, :, :, None].expand(s.shape[0], heads, Nq, 1).to(s.device)
    top = torch.gather(s, 3, idx)
    rest = s.scatter(3, idx, float("-inf")).amax(-1, keepdim=True)
    return (top - rest).min().item()


# ---------------------------------------------------------------- outputs pinned by hash against the parent commit
# tests/golden/attention_parent_sha.npz (tools/record_parent_fixtures.py --attention-sha; tests/test_attention_parent_gpu.py): the smallest
# shapes that reach every instantiation and branch of csrc/attention.hip, plus one head-dim-80 launch.  (route, name, kind, parameters);
# the operands of a case come from gen(crc32(name)), so recorder and test build the same bits in any order.
def _parent_cases():
    out = []
    add = lambda route, kind, **p: out.append((route, ".".join([kind] + [f"{k}{v}" for k, v in p.items()]), kind, p))
    two = [dict(Bq=4, heads=2, kv_div=2, Nq=130), dict(Bq=64, heads=8, kv_div=16, Nq=300)]          # the second: q_iters = 2
    add("short", "attn", Nk=77, **two[0]), add("short", "attn", Nk=96, **two[0]), add("short", "attn", Nk=77, **two[1])
    for shape in two:
        for Ni in (16, 4):
            add("short_ip", "ip", Nt=77, Ni=Ni, **shape)
    for Nk in (97, 127):
        for Nq in (1, 33, 130):
            add("generic", "attn", Nk=Nk, Bq=4, heads=2, kv_div=2, Nq=Nq)
    for N in (77, 200):
        for B, heads in ((4, 2), (3, 3)):                         # grid.y = 8: remapped block order; 9: plain
            add("causal", "causal", N=N, B=B, heads=heads)
    for Nk in (128, 129, 191, 193, 320):
        for Nq in (130, 300):
            add("v4", "attn", Nk=Nk, Bq=4, heads=2, kv_div=2, Nq=Nq), add("v4", "attn", Nk=Nk, Bq=3, heads=3, kv_div=1, Nq=Nq)
    for regime in ("high", "late_peak", "band_edge"):             # the reference moves off 0 / moves late / stays in the zero band
        add("v4_regimes", "regime", regime=regime, Nk=320, Bq=2, heads=2, Nq=256)
    for B, T, HW, heads in ((2, 16, 50, 5), (1, 8, 64, 8), (1, 16, 2560, 5), (3, 5, 7, 2)):          # temporal_variants_ref.STANDALONE
        add("temporal_causal", "temporal", causal=1, B=B, T=T, HW=HW, heads=heads)
    for T in (17, 24, 32):
        for causal in (0, 1):
            for B, HW, heads in ((2, 7, 2), (1, 64, 5)):
                add("temporal_long", "temporal", causal=causal, B=B, T=T, HW=HW, heads=heads)
    add("d80", "d80", B=1, heads=16, N=257)
    return out


PARENT_CASES = _parent_cases()
PARENT_ROUTES = sorted({c[0] for c in PARENT_CASES})


def sha(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_parent_case(ops, name, kind, p, dev="cuda"):
    """one launch of a PARENT_CASES entry on freshly generated operands; returns the output, which was pre-filled with NaN"""
    import zlib
    g = gen(zlib.crc32(name.encode()))
    nan_out = lambda *shape: torch.full(shape, NAN, dtype=torch.float16, device=dev)
    scale = 0.125
    if kind in ("attn", "ip", "regime"):
        Bq, heads, Nq, kv_div = p["Bq"], p["heads"], p["Nq"], p.get("kv_div", 1)
        C, Bk, Nk = heads * 64, Bq // kv_div, p.get("Nk", p.get("Nt"))
        q, k, v = randh(g, Bq, Nq, C), randh(g, Bk, Nk, C), randh(g, Bk, Nk, C)
        if kind == "regime":
            apply_regime(p["regime"], q, [(k, 1.0)], scale, 64, [(0, 300, 7, 6.0), (0, 30, 7, 1.5)])
        q, k, v = q.to(dev), k.to(dev), v.to(dev)
        out = nan_out(Bq, Nq, C)
        if kind == "ip":
            ki, vi = randh(g, Bk, p["Ni"], C).to(dev), randh(g, Bk, p["Ni"], C).to(dev)
            ops.attention_ip(q, k, v, ki, vi, out, Bq=Bq, heads=heads, Nq=Nq, Nt=Nk, Ni=p["Ni"], ldq=C, ldk=C, ldv=C, ldk_ip=C, ldv_ip=C,
                             ldo=C, kv_div=kv_div, scale=scale, ip_scale=0.7)
        else:
            ops.attention(q, k, v, out, Bq=Bq, heads=heads, Nq=Nq, Nk=Nk, ldq=C, ldk=C, ldv=C, ldo=C, kv_div=kv_div, scale=scale)
    elif kind in ("causal", "d80"):
        B, heads, N = p["B"], p["heads"], p["N"]
        C = heads * (80 if kind == "d80" else 64)
        q, k, v = (randh(g, B, N, C).to(dev) for _ in range(3))
        out = nan_out(B, N, C)
        fn, scale = (ops.attention_d80, 80 ** -0.5) if kind == "d80" else (ops.attention_causal, scale)
        fn(q, k, v, out, B=B, heads=heads, N=N, ldq=C, ldk=C, ldv=C, ldo=C, scale=scale)
    else:
        B, T, HW, heads, causal = p["B"], p["T"], p["HW"], p["heads"], bool(p["causal"])
        C = heads * 64
        qkv = randh(g, B * T * HW, 3 * C).to(dev)                  # q | k | v side by side, as the projection leaves them
        out = nan_out(B * T * HW, C)
        kw = dict(B=B, T=T, HW=HW, heads=heads, ld_qkv=3 * C, ldo=C, scale=scale)
        if T > 16:
            ops.temporal_attention_long(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, causal=causal, **kw)
        else:
            (ops.temporal_attention_causal if causal else ops.temporal_attention)(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, **kw)
    return out
