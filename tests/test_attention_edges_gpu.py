"""GPU: the attention kernels of csrc/attention.hip (and the head-dim-80 kernel of clip_vision.hip) at every dispatch route, stride,
tail and mask edge, against float64 torch on the same fp16 operands (tests/attention_edges_ref.py).  The error is taken per
(batch, head) slice -- max|got - ref| over the slice / max|ref| of that slice -- and every slice must meet TOL16 = 3e-3.

Which gap of the kernel-level suite each test closes:
  1. attention_kernel<false> (97 <= Nk <= 127) never run ............ test_dispatch_table
  2. query-group loop of attention_short_kernel (q_iters > 1) ....... test_short_kernel_query_loop
  3. XCD block remap (grid.y % 8 == 0) on v4 / generic / short ...... test_xcd_remap
  4. strides, pad columns, guard rows, stray writes ................. test_packed_operands_and_canaries
  5. memory past the operands (load guards, num_records) ............ test_poisoned_surroundings
  6. key <-> value pairing, head / batch slices ..................... test_onehot_returns_the_v_row
  7. logit regimes on the short / generic / ip / causal / d80 /
     temporal kernels ............................................... test_logit_regimes
  8. temporal T in {1, 2, 15, 16}, ld_qkv != 3C, ldo != C ........... test_temporal_tails
  9. entry validation matches the kernels' access widths ............ tests/test_abi_cpu.py::test_bad_arguments_are_rejected_without_a_gpu

Dispatch of moca_attention_f16 (attention.hip: KT = 64, KS96 = 96): Nk <= KS96 = 96 -> attention_short_kernel (one 96-key tile);
Nk >= 2 KT = 128 -> attention_v4_kernel (LDS-DMA, lazy reference); 97 <= Nk <= 127 -> attention_kernel<false> (two 64-key tiles, the
second partial).  moca_attention_causal_f16 -> attention_kernel<true>; moca_attention_ip_f16 -> attention_short_kernel<true> (Ni > 0)
or <false> (Ni == 0).  clip_attention_d80_kernel takes blockIdx directly (no attn_block_coords), so it has no remap case."""
import pytest
import torch

import attention_edges_ref as R
from attention_edges_ref import NAN, TOL16

pytestmark = pytest.mark.gpu

from moca_video_amd import ops  # noqa: E402

DEV = "cuda"
SCALE = 0.125
SCALE80 = 80 ** -0.5


@pytest.fixture(autouse=True)
def _stream():
    ops.set_stream(None)
    yield
    torch.cuda.synchronize()


def nan_out(*shape):
    return torch.full(shape, NAN, dtype=torch.float16, device=DEV)


def attn(q, k, v, out, heads, kv_div, ldq, ldk, ldv, ldo, Bq, Nq, Nk, scale=SCALE):
    ops.attention(q, k, v, out, Bq=Bq, heads=heads, Nq=Nq, Nk=Nk, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, kv_div=kv_div, scale=scale)


def attn_ip(q, k, v, ki, vi, out, heads, kv_div, ldq, ldk, ldki, ldo, Bq, Nq, Nt, Ni, ip_scale, scale=SCALE):
    ops.attention_ip(q, k, v, ki, vi, out, Bq=Bq, heads=heads, Nq=Nq, Nt=Nt, Ni=Ni, ldq=ldq, ldk=ldk, ldv=ldk, ldk_ip=ldki, ldv_ip=ldki,
                     ldo=ldo, kv_div=kv_div, scale=scale, ip_scale=ip_scale)


def route(Nk):
    return "short" if Nk <= 96 else ("v4" if Nk >= 128 else "generic")


def short_q_iters(Bq, heads, Nq):
    """launch_short (attention.hip): query groups of 128 per block"""
    qgroups = (Nq + 127) // 128
    return max(1, min(8, qgroups, qgroups * Bq * heads // 768)), qgroups


# ---------------------------------------------------------------- A. dispatch table
@pytest.mark.parametrize("Bq,heads,kv_div", [(2, 3, 1), (4, 2, 2)])
@pytest.mark.parametrize("Nk", [95, 96, 97, 112, 127, 128, 129, 191, 192, 193])
def test_dispatch_table(Nk, Bq, heads, kv_div):
    """Nk 95, 96 -> short kernel; 97, 112, 127 -> attention_kernel<false> (partial second tile); 128 .. 193 -> v4 (whole tiles at 128
    and 192, one-key and 63-key tails at 129 and 191, one key in a fourth tile at 193).  Nq 1 and 33: one partial wave; 130: a second
    block with two live rows."""
    C, Bk = heads * 64, Bq // kv_div
    g = R.gen(1000 + Nk * 7 + Bq)
    k, v = R.randh(g, Bk, Nk, C).to(DEV), R.randh(g, Bk, Nk, C).to(DEV)
    for Nq in (1, 33, 130):
        q = R.randh(g, Bq, Nq, C).to(DEV)
        out = nan_out(Bq, Nq, C)
        attn(q, k, v, out, heads, kv_div, C, C, C, C, Bq, Nq, Nk)
        R.check_slices(out, R.ref_plain(q, k, v, heads, kv_div, SCALE), Bq, heads, f"dispatch Nk={Nk} ({route(Nk)}) Nq={Nq} Bq={Bq}")


# ---------------------------------------------------------------- B. query loop of the short kernel
@pytest.mark.parametrize("entry", ["attention", "attention_ip"])
@pytest.mark.parametrize("Bq,heads,Nq,kv_div,iters,gridx", [(64, 8, 300, 16, 2, 2), (96, 8, 330, 16, 3, 1)])
def test_short_kernel_query_loop(Bq, heads, Nq, kv_div, iters, gridx, entry):
    """(64, 8, 300): 3 query groups, q_iters = 2, two blocks per (batch, head): the second block runs one group and breaks, wave 1 of
    that group holds 12 live rows, waves 2 and 3 none.  (96, 8, 330): q_iters = 3 in one block; the third group holds 74 rows."""
    q_iters, qgroups = short_q_iters(Bq, heads, Nq)
    assert q_iters >= 2 and q_iters == iters and (qgroups + q_iters - 1) // q_iters == gridx, (q_iters, qgroups)
    C, Bk, Nt, Ni, ip_scale = heads * 64, Bq // kv_div, 77, 16, 0.7
    g = R.gen(2000 + Nq)
    q = R.randh(g, Bq, Nq, C).to(DEV)
    k, v = R.randh(g, Bk, Nt, C).to(DEV), R.randh(g, Bk, Nt, C).to(DEV)
    out = nan_out(Bq, Nq, C)
    if entry == "attention":
        attn(q, k, v, out, heads, kv_div, C, C, C, C, Bq, Nq, Nt)
        ref = R.ref_plain(q, k, v, heads, kv_div, SCALE)
    else:
        ki, vi = R.randh(g, Bk, Ni, C).to(DEV), R.randh(g, Bk, Ni, C).to(DEV)
        attn_ip(q, k, v, ki, vi, out, heads, kv_div, C, C, C, C, Bq, Nq, Nt, Ni, ip_scale)
        ref = R.ref_ip(q, k, v, ki, vi, heads, kv_div, SCALE, ip_scale)
    R.check_slices(out, ref, Bq, heads, f"short kernel {entry} q_iters={q_iters} grid.x={gridx} Nq={Nq}")


# ---------------------------------------------------------------- C. XCD remap
@pytest.mark.parametrize("Bq,heads,Nq,Nk", [(4, 2, 300, 200), (8, 2, 260, 120), (2, 4, 260, 77), (3, 3, 300, 200)])
def test_xcd_remap(Bq, heads, Nq, Nk):
    """grid.y = Bq heads = 8 or 16 takes the remapped branch of attn_block_coords with grid.x = 3 (v4, generic, short kernel);
    (3, 3): grid.y = 9, the plain branch, same grid.x.  A wrong (bx, by) puts a whole 128-query block into another slice."""
    assert (Bq * heads % 8 == 0) == ((Bq, heads) != (3, 3)) and (Nq + 127) // 128 == 3
    C = heads * 64
    g = R.gen(3000 + Nk + Bq)
    q, k, v = R.randh(g, Bq, Nq, C).to(DEV), R.randh(g, Bq, Nk, C).to(DEV), R.randh(g, Bq, Nk, C).to(DEV)
    out = nan_out(Bq, Nq, C)
    attn(q, k, v, out, heads, 1, C, C, C, C, Bq, Nq, Nk)
    R.check_slices(out, R.ref_plain(q, k, v, heads, 1, SCALE), Bq, heads, f"xcd remap grid.y={Bq * heads} ({route(Nk)})")


def test_xcd_remap_causal():
    B, heads, N = 4, 2, 200
    C = heads * 64
    g = R.gen(3100)
    q, k, v = (R.randh(g, B, N, C).to(DEV) for _ in range(3))
    out = nan_out(B, N, C)
    ops.attention_causal(q, k, v, out, B=B, heads=heads, N=N, ldq=C, ldk=C, ldv=C, ldo=C, scale=SCALE)
    R.check_slices(out, R.ref_causal(q, k, v, heads, SCALE), B, heads, "xcd remap grid.y=8 (causal)")


# ---------------------------------------------------------------- D / E. packed operands, canaries, poisoned surroundings
def run_packed(case, Nq, seed, extra=0, poison=NAN, canary=True):
    """One launch of `case` with q / k / v as column views of packed buffers (self-attention: one [rows][3C + 8] buffer; cross: q in a
    [rows][3C + 8] buffer, K | V in a [rows][2C + 8] buffer), pad columns and `extra` trailing rows = `poison`.  Returns
    (out view, out buffer, reference, batches, heads, D, rows)."""
    kind = case[0]
    g = R.gen(seed)
    Bq, heads, kv_div = 4, 3, 2
    D = 80 if kind == "d80" else 64
    C = heads * D
    if kind in ("temporal", "temporal_causal"):
        B, T, HW = 2, case[1], 9
        rows = B * T * HW
        _, (q, k, v), ld = R.packed(g, rows, [C, C, C], extra=extra, poison=poison, dev=DEV)
        obuf, out, ldo = R.canary_out(rows, C, DEV) if canary else (None, nan_out(rows, C), C)
        fn = ops.temporal_attention_causal if kind == "temporal_causal" else ops.temporal_attention
        fn(q, k, v, out, B=B, T=T, HW=HW, heads=heads, ld_qkv=ld, ldo=ldo, scale=SCALE)
        return out, obuf, R.ref_temporal(q, k, v, B, T, HW, heads, SCALE, kind == "temporal_causal"), B, heads, D, rows
    rows = Bq * Nq
    obuf, out, ldo = R.canary_out(rows, C, DEV) if canary else (None, nan_out(rows, C), C)
    if kind in ("self", "causal", "d80"):                          # q, k, v of a self-attention: one fused projection output
        _, (q, k, v), ld = R.packed(g, rows, [C, C, C], extra=extra, poison=poison, dev=DEV)
        q3, k3, v3 = (t.unflatten(0, (Bq, Nq)) for t in (q, k, v))
        if kind == "self":
            attn(q, k, v, out, heads, 1, ld, ld, ld, ldo, Bq, Nq, Nq)
            ref = R.ref_plain(q3, k3, v3, heads, 1, SCALE)
        elif kind == "causal":
            ops.attention_causal(q, k, v, out, B=Bq, heads=heads, N=Nq, ldq=ld, ldk=ld, ldv=ld, ldo=ldo, scale=SCALE)
            ref = R.ref_causal(q3, k3, v3, heads, SCALE)
        else:
            ops.attention_d80(q, k, v, out, B=Bq, heads=heads, N=Nq, ldq=ld, ldk=ld, ldv=ld, ldo=ldo, scale=SCALE80)
            ref = R.ref_d80(q3, k3, v3, heads, SCALE80)
        return out, obuf, ref, Bq, heads, D, rows
    Bk = Bq // kv_div
    _, (q, _, _), ldq = R.packed(g, rows, [C, C, C], extra=extra, poison=poison, dev=DEV)
    q3 = q.unflatten(0, (Bq, Nq))
    if kind == "cross":
        Nk = case[1]
        _, (k, v), ldk = R.packed(g, Bk * Nk, [C, C], extra=extra, poison=poison, dev=DEV)
        attn(q, k, v, out, heads, kv_div, ldq, ldk, ldk, ldo, Bq, Nq, Nk)
        ref = R.ref_plain(q3, k.unflatten(0, (Bk, Nk)), v.unflatten(0, (Bk, Nk)), heads, kv_div, SCALE)
    else:
        assert kind == "ip"
        Nt, Ni, ip_scale = 77, case[1], 0.7
        _, (k, v), ldk = R.packed(g, Bk * Nt, [C, C], extra=extra, poison=poison, dev=DEV)
        _, (ki, vi), ldki = R.packed(g, Bk * max(Ni, 1), [C, C], extra=extra, poison=poison, dev=DEV)
        attn_ip(q, k, v, ki, vi, out, heads, kv_div, ldq, ldk, ldki, ldo, Bq, Nq, Nt, Ni, ip_scale)
        k3, v3 = k.unflatten(0, (Bk, Nt)), v.unflatten(0, (Bk, Nt))
        ref = R.ref_plain(q3, k3, v3, heads, kv_div, SCALE) if Ni == 0 else \
            R.ref_ip(q3, k3, v3, ki.unflatten(0, (Bk, Ni)), vi.unflatten(0, (Bk, Ni)), heads, kv_div, SCALE, ip_scale)
    return out, obuf, ref, Bq, heads, D, rows


PACKED_CASES = [("cross", 77), ("cross", 120), ("cross", 200), ("self",), ("ip", 0), ("ip", 16), ("causal",), ("temporal", 16),
                ("temporal_causal", 16), ("d80",)]


@pytest.mark.parametrize("case", PACKED_CASES, ids=lambda c: "-".join(map(str, c)))
def test_packed_operands_and_canaries(case):
    """every entry point on column views of packed buffers (row strides 3C + 8 and 2C + 8), writing a column view (row stride
    C + 8) of a NaN buffer with 4 guard rows before and after: the live region meets the bound, every pad column and guard row is
    still NaN.  Nq = 130 (a second block with 2 live rows) and 33 (one partial wave), 4 batches, kv_div 2."""
    for Nq in (130, 33):
        out, obuf, ref, nb, heads, D, rows = run_packed(case, Nq, 4000 + Nq)
        what = f"packed {'-'.join(map(str, case))} Nq={Nq}"
        R.check_slices(out, ref, nb, heads, what, D=D)
        R.assert_canary(obuf, rows, heads * D, what)
        if case[0].startswith("temporal"):
            break                                                   # (no query count: one launch)


POISON_CASES = [("cross", 77), ("cross", 120), ("cross", 200), ("ip", 16), ("causal",), ("temporal", 5)]


@pytest.mark.parametrize("case", POISON_CASES, ids=lambda c: "-".join(map(str, c)))
def test_poisoned_surroundings(case):
    """the operands sit inside larger allocations: 8 rows after the last batch's rows and the 8 pad columns of every row hold NaN in
    one run and zeros in the other.  Both runs meet the bound and are equal bit for bit: nothing past an operand reaches the result
    (a row read one too far and multiplied by P = 0 turns the NaN run into NaN).  Every pointer handed over has its full
    batches x rows x ld range inside the allocation; the poison lies behind it."""
    outs = []
    for poison in (NAN, 0.0):
        out, _, ref, nb, heads, D, _ = run_packed(case, 130, 5000, extra=8, poison=poison, canary=False)
        R.check_slices(out, ref, nb, heads, f"poison={poison} {'-'.join(map(str, case))}", D=D)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- F. one-hot softmax
ONEHOT_CASES = [("attn", 77, 7), ("attn", 120, 2), ("attn", 200, 2), ("attn", 512, 2), ("causal", 200, 2), ("d80", 257, 2),
                ("temporal", 16, 3), ("temporal_causal", 16, 3)]


@pytest.mark.parametrize("kind,Nk,heads", ONEHOT_CASES, ids=lambda c: str(c))
def test_onehot_returns_the_v_row(kind, Nk, heads):
    """every query has one key whose score lies >= 30 log2 units above all its others (asserted on the inputs): P is 1 for it and
    rounds to 0 in fp16 for the rest, so the output row must be the V row of the hot key of ITS batch and head, bit for bit.  The
    hot key (7 r + 3 h + 1) % Nk walks over every key position of every head (asserted), the last key of a partial tile included
    (Nk = 77 needs 7 heads for that: 7 divides 77); causal: min(hot, r).  The float64 reference must give the V row for every query
    before the kernel is asked."""
    causal = kind in ("causal", "temporal_causal")
    D = 80 if kind == "d80" else 64
    scale = SCALE80 if kind == "d80" else SCALE
    g = R.gen(6000 + Nk + heads)
    if kind == "attn":
        Bq, kv_div, Nq = 4, 2, max(Nk, 128) + 3
    elif kind in ("causal", "d80"):
        Bq, kv_div, Nq = 2, 1, Nk
    else:
        B, HW = 2, 9
        Bq, kv_div, Nq = B * HW, 1, Nk
    hot = R.hot_keys(Nq, Nk, heads, causal)
    if not causal:
        assert all(set(hot[:, h].tolist()) == set(range(Nk)) for h in range(heads)) or (Nk == 77 and set(hot.flatten().tolist()) == set(range(77)))
    q, k, v, want = (t.to(DEV) for t in R.onehot_operands(g, Bq, Nq, Nk, heads, kv_div, hot, D=D))
    gap = R.onehot_gap(q, k, heads, kv_div, scale, hot, D=D, causal=causal)
    assert gap >= 30.0, gap
    ref = R.ref_plain(q, k, v, heads, kv_div, scale, D=D, causal=causal)
    assert torch.equal(ref.half(), want), "the construction itself does not select the V row"
    C = heads * D
    if kind.startswith("temporal"):
        qt, kt, vt = (R.to_tokens(t, B, Nk, HW).contiguous() for t in (q, k, v))
        out = nan_out(B * Nk * HW, C)
        fn = ops.temporal_attention_causal if causal else ops.temporal_attention
        fn(qt, kt, vt, out, B=B, T=Nk, HW=HW, heads=heads, ld_qkv=C, ldo=C, scale=scale)
        out = R.from_tokens(out, B, Nk, HW)
    else:
        out = nan_out(Bq, Nq, C)
        if kind == "attn":
            attn(q, k, v, out, heads, kv_div, C, C, C, C, Bq, Nq, Nk)
        elif kind == "causal":
            ops.attention_causal(q, k, v, out, B=Bq, heads=heads, N=Nk, ldq=C, ldk=C, ldv=C, ldo=C, scale=scale)
        else:
            ops.attention_d80(q, k, v, out, B=Bq, heads=heads, N=Nk, ldq=C, ldk=C, ldv=C, ldo=C, scale=scale)
    bad = (out.reshape(Bq, Nq, heads, D) != want.reshape(Bq, Nq, heads, D)).any(-1).nonzero()
    print(f"[parity] one-hot {kind} Nk={Nk}: gap {gap:.1f} log2 units, {len(bad)} of {Bq * Nq * heads} rows differ from their V row")
    assert torch.equal(out, want), f"(batch, query, head) rows that are not their V row: {bad[:8].tolist()}"


# ---------------------------------------------------------------- G. logit regimes
def regime_operands(kind, regime, seed):
    """CPU fp16 operands of one regime case: (q, [k segments], [v segments], peaks) with q [B, N, C]"""
    g = R.gen(seed)
    heads = 2
    D = 80 if kind == "d80" else 64
    C = heads * D
    B, Nq, Nks = {"short": (2, 256, [77]), "generic": (2, 256, [120]), "ip": (2, 256, [77, 16]), "causal": (2, 200, [200]),
                  "d80": (2, 257, [257]), "temporal": (18, 16, [16]), "temporal_causal": (18, 16, [16])}[kind]
    q = R.randh(g, B, Nq, C)
    ks = [R.randh(g, B, n, C) for n in Nks]
    vs = [R.randh(g, B, n, C) for n in Nks]
    # late_peak: (segment, key, query row, gain); the second, weaker key comes earlier (the maximum moves between tiles / sub-tiles)
    peaks = {"short": [(0, 70, 7, 6.0), (0, 5, 7, 1.5)], "generic": [(0, 110, 7, 6.0), (0, 30, 7, 1.5)],
             "ip": [(0, 70, 7, 6.0), (0, 5, 7, 1.5), (1, 12, 9, 6.0)],
             # causal: key 150 = 6 x query 150 sits ON the diagonal of row 150; key 180 = 6 x query 20 lies ABOVE the diagonal of row 20
             # (masked there: it must not move row 20) and is an ordinary key for the rows from 180 on
             "causal": [(0, 150, 150, 6.0), (0, 180, 20, 6.0), (0, 30, 150, 1.5)],
             "d80": [(0, 250, 7, 6.0), (0, 30, 7, 1.5)],
             "temporal": [(0, 13, 7, 6.0), (0, 2, 7, 1.5)],
             "temporal_causal": [(0, 5, 5, 6.0), (0, 13, 7, 6.0), (0, 2, 5, 1.5)]}[kind]
    c0 = [1.0, -0.5][:len(ks)]                                      # ip: the image scores move the other way, half as far
    scale = SCALE80 if D == 80 else SCALE
    R.apply_regime(regime, q, list(zip(ks, c0)), scale, D, peaks)
    return q, ks, vs, heads, D, scale


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("kind", ["short", "generic", "ip", "causal", "d80", "temporal", "temporal_causal"])
def test_logit_regimes(kind, regime):
    """the five regimes of test_attention_reference_regimes (all scores of a row near -14 / +11 / +6 log2 units, every third row at -14,
    one late key far above the rest) on the kernels that test leaves out.  ip: text scores move by the target, image scores by
    -0.5 x the target, so the two segment maxima lie up to 21 log2 units apart, in either order."""
    q, ks, vs, heads, D, scale = regime_operands(kind, regime, 7000 + len(kind))
    q = q.to(DEV)
    ks, vs = [t.to(DEV) for t in ks], [t.to(DEV) for t in vs]
    B, Nq, C = q.shape
    k, v = ks[0], vs[0]
    Nk = k.shape[1]
    what = f"regime {regime} on {kind}"
    if kind.startswith("temporal"):
        Bv, HW, T, causal = 2, 9, 16, kind == "temporal_causal"
        qt, kt, vt = (R.to_tokens(t, Bv, T, HW).contiguous() for t in (q, k, v))
        out = nan_out(Bv * T * HW, C)
        fn = ops.temporal_attention_causal if causal else ops.temporal_attention
        fn(qt, kt, vt, out, B=Bv, T=T, HW=HW, heads=heads, ld_qkv=C, ldo=C, scale=scale)
        R.check_slices(out, R.ref_temporal(qt, kt, vt, Bv, T, HW, heads, scale, causal), Bv, heads, what)
        return
    out = nan_out(B, Nq, C)
    if kind in ("short", "generic"):
        assert route(Nk) == kind
        attn(q, k, v, out, heads, 1, C, C, C, C, B, Nq, Nk)
        ref = R.ref_plain(q, k, v, heads, 1, scale)
    elif kind == "ip":
        attn_ip(q, k, v, ks[1], vs[1], out, heads, 1, C, C, C, C, B, Nq, Nk, ks[1].shape[1], 0.7)
        ref = R.ref_ip(q, k, v, ks[1], vs[1], heads, 1, scale, 0.7)
    elif kind == "causal":
        ops.attention_causal(q, k, v, out, B=B, heads=heads, N=Nk, ldq=C, ldk=C, ldv=C, ldo=C, scale=scale)
        ref = R.ref_causal(q, k, v, heads, scale)
    else:
        ops.attention_d80(q, k, v, out, B=B, heads=heads, N=Nk, ldq=C, ldk=C, ldv=C, ldo=C, scale=scale)
        ref = R.ref_d80(q, k, v, heads, scale)
    R.check_slices(out, ref, B, heads, what, D=D)


# ---------------------------------------------------------------- H. temporal tails
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("B,HW,heads", [(1, 1, 1), (2, 9, 3), (1, 64, 5)])
@pytest.mark.parametrize("T", [1, 2, 15, 16])
def test_temporal_tails(T, B, HW, heads, causal):
    """one frame (softmax over one key), two, 15 (one masked key row, one query column never stored) and the full 16; a single problem
    (three idle waves that recompute it and must not store), 54 problems (a last block with two), 320; q | k | v in one
    [rows][3C + 8] buffer, out a column view (row stride C + 8) of a NaN buffer with guard rows."""
    C, rows = heads * 64, B * T * HW
    g = R.gen(8000 + T * 10 + HW)
    _, (q, k, v), ld = R.packed(g, rows, [C, C, C], dev=DEV)
    obuf, out, ldo = R.canary_out(rows, C, DEV)
    fn = ops.temporal_attention_causal if causal else ops.temporal_attention
    fn(q, k, v, out, B=B, T=T, HW=HW, heads=heads, ld_qkv=ld, ldo=ldo, scale=SCALE)
    what = f"temporal T={T} B={B} HW={HW} heads={heads} causal={causal}"
    R.check_slices(out, R.ref_temporal(q, k, v, B, T, HW, heads, SCALE, causal), B, heads, what)
    R.assert_canary(obuf, rows, C, what)
