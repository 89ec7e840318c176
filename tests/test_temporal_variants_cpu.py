"""CPU: the two TemporalTransformer variants of the reference's constructor signature -- `use_causal_attention=True`
(attention.py:309-311,342-346,101-105) and `temporal_selfatt_only=False` (:313-314,353-363): construction, state-dict surface against
key / shape lists taken from the REAL reference modules (tools/make_golden_temporal_variants.py), the refusals, the C-ABI entry and
the gemm-params field of the mask, the ISA of the two causal kernels, and what a plan RECORDS for them (plans built on the host: the
launch list is read, nothing runs) -- including that the FULL configuration still records the launch list of the parent commit."""
import ctypes as C
import os
import shutil
import sys

import pytest
import torch

from helpers import FULL, REDUCED, golden
from plan_cpu import aliases, cpu_plan, fixture_plans, signature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _meta_unet(**kw):
    from moca_video_amd import UNetModel
    with torch.device("meta"):
        return UNetModel(**kw)


def _names(plan):
    out = []
    for s in plan.steps:
        n = s.func.__name__
        t = s.keywords.get("tattn")
        if n == "gemm" and t is not None:
            n = "gemm:tattn_causal" if len(t) > 3 and t[3] else "gemm:tattn"
        out.append(n)
    return out


# ---------------------------------------------------------------- construction / state dict
def test_construction_no_longer_raises_and_the_rest_of_the_list_stays():
    from moca_video_amd import UNetModel
    m = _meta_unet(**dict(REDUCED, use_causal_attention=True))
    tts = [t for t in m.modules() if type(t).__name__ == "_TemporalTransformer"]
    assert len(tts) == 17 and all(t.causal and t.temporal_length == 16 and t.only_self_att for t in tts)
    assert all(b.attn2.is_self for t in tts for b in t.transformer_blocks)
    m = _meta_unet(**dict(REDUCED, temporal_selfatt_only=False, use_causal_attention=True))
    tts = [t for t in m.modules() if type(t).__name__ == "_TemporalTransformer"]
    # the cross branch passes no mask (attention.py:362-363): the flag is kept, the mask reaches nothing
    assert all(not t.only_self_att and t.causal_attention and not t.causal for t in tts)
    assert all(not b.attn2.is_self and b.attn1.is_self for t in tts for b in t.transformer_blocks)
    assert tuple(m.init_attn[0].transformer_blocks[0].attn2.to_k.weight.shape) == (512, 128)
    for bad in (dict(use_relative_position=True), dict(tempspatial_aware=True), dict(use_scale_shift_norm=True), dict(resblock_updown=True),
                dict(dims=3), dict(conv_resample=False), dict(num_head_channels=32),
                dict(use_image_attention=True, temporal_selfatt_only=False)):
        with pytest.raises(NotImplementedError):
            UNetModel(**dict(REDUCED, **bad))
    with pytest.raises(AssertionError):                          # attention.py:310
        UNetModel(**dict(REDUCED, use_causal_attention=True, temporal_length=None))


@pytest.mark.parametrize("tag,kw", [("causal", dict(use_causal_attention=True)), ("cross", dict(temporal_selfatt_only=False))])
def test_full_width_state_dict_equals_the_reference_lists(tag, kw):
    g = golden("unet_tvariants_keys")
    want = {str(k): tuple(int(x) for x in str(s).split(",")) for k, s in zip(g[tag + "_keys"], g[tag + "_shapes"])}
    m = _meta_unet(**dict(FULL, **kw))
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g[tag + "_keys"]], "state-dict names / order differ from the reference module's"
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    # load_state_dict(strict=True) against exactly that list
    m.load_state_dict({k: torch.empty(s, device="meta") for k, s in want.items()}, strict=True)
    plain = _meta_unet(**FULL).state_dict()
    if tag == "causal":                                          # the mask is a plain attribute of the reference module: no key
        assert list(sd) == list(plain) and all(sd[k].shape == plain[k].shape for k in sd)
    else:                                                        # 17 temporal attn2.to_k / to_v go from [inner, inner] to [inner, 1024]
        changed = [k for k in sd if sd[k].shape != plain[k].shape]
        assert list(sd) == list(plain) and len(changed) == 34
        assert all(k.endswith(("attn2.to_k.weight", "attn2.to_v.weight")) and sd[k].shape[1] == 1024 for k in changed)


# ---------------------------------------------------------------- C-ABI
def test_abi_entry_and_mask_field_refusals():
    """nothing is launched: every refusal returns MOCA_E_BADARG (-1) before a launch, every query only reads the struct"""
    from moca_video_amd import lib, ops
    l = lib.load()
    f = l.moca_temporal_attention_causal_f16
    P = [C.c_void_p(0x10000 * (i + 1)) for i in range(4)]
    assert f(*P, 1, 17, 4, 1, 192, 64, 0.125, None) == -1        # T > 16
    assert f(*P, 1, 16, 4, 1, 100, 64, 0.125, None) == -1        # ld_qkv % 8
    assert f(*P, 1, 16, 4, 1, 192, 64, 0.0, None) == -1 and f(*P, 1, 16, 4, 1, 192, 64, -0.125, None) == -1    # scale > 0
    assert f(None, *P[1:], 1, 16, 4, 1, 192, 64, 0.125, None) == -1
    # the field sits in what was padding: the struct keeps its size and the offsets of every other field
    assert lib.GemmParams.tattn_causal.offset == lib.GemmParams.prefetch_kib.offset + 4
    assert lib.GemmParams.colsum.offset == lib.GemmParams.tattn_causal.offset + 4
    x = torch.empty(2 * 16 * 40, 320, dtype=torch.float16)
    pw = ops.pack_qkv_per_head(*(torch.zeros(320, 320) for _ in range(3)), 5, device="cpu")
    kw = dict(M=x.shape[0], lda=320, splits=1)
    assert ops.gemm_tattn_ok(x, pw, tattn=(16, 40, 0.125), **kw) and ops.gemm_tattn_ok(x, pw, tattn=(16, 40, 0.125, True), **kw)
    assert not ops.gemm_tattn_ok(x, pw, tattn=(16, 40, -0.125, True), **kw)       # the query answers for the call WITH the field
    assert not ops.gemm_tattn_ok(x, pw, tattn=(16, 30, 0.125, True), **kw)
    p = ops._gemm_params(x, pw, x, tattn=(16, 40, 0.125, True), **kw)
    assert p.tattn_causal == 1 and ops._gemm_params(x, pw, x, tattn=(16, 40, 0.125), **kw).tattn_causal == 0
    p.tattn_causal = 2
    assert l.moca_gemm_tattn_ok(C.byref(p)) == 0 and l.moca_gemm_f16(C.byref(p), None) == -1
    # the mask exists in the MOCA_EP_TATTN epilogue only: a plain linear that carries the field is refused
    q = ops._gemm_params(x, ops.pack_linear(torch.zeros(320, 320), None, device="cpu"), x, **kw)
    q.tattn_causal = 1
    assert l.moca_gemm_f16(C.byref(q), None) == -1


def test_isa_of_the_causal_kernels():
    """the causal instantiation of the fused kernel keeps the main loop (60 MFMAs, 8 LDS-DMA, 22 fragment reads, 4 barriers, no
    `s_waitcnt vmcnt(0)`), the register count and the spill-free epilogue of gemm_w80s_kernel<0, 3>; the mask costs a few VALU
    instructions of the epilogue; the standalone causal kernel keeps the registers of the plain one"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from moca_video_amd import lib
    if not os.path.exists(os.path.join(isa_report.LLVM, "llvm-objdump")) or shutil.which("c++filt") is None:
        pytest.skip("llvm-objdump / c++filt not available")
    r = isa_report.analyse(lib.LIB_PATH)
    base, cau = r["gemm_w80s_kernel<0, 3>"], r["gemm_w80s_causal_kernel<0, 3>"]
    for k in ("mfma", "lds_dma", "ds_read", "barrier", "vmcnt0", "ds_write", "global_load", "scratch"):
        assert cau["loop"][k] == base["loop"][k], k
    assert (cau["loop"]["mfma"], cau["loop"]["lds_dma"], cau["loop"]["ds_read"], cau["loop"]["barrier"], cau["loop"]["vmcnt0"]) == (60, 8, 22, 4, 0)
    assert cau["vgpr_count"] <= base["vgpr_count"] and cau["agpr_count"] == 0 and cau["vgpr_spill_count"] == 0
    assert cau["sgpr_spill_count"] <= base["sgpr_spill_count"] and cau["scratch"] == 0 and cau["private_segment_fixed_size"] == 0
    assert cau["mfma_total"] == base["mfma_total"] and 0 < cau["instructions_total"] - base["instructions_total"] <= 64
    ta = {k: v for k, v in r.items() if "temporal_attention_kernel" in k}
    assert len(ta) == 2
    plain = next(v for k, v in ta.items() if "<false>" in k or "ILb0E" in k)
    caus = next(v for k, v in ta.items() if "<true>" in k or "ILb1E" in k)
    assert caus["vgpr_count"] <= plain["vgpr_count"] and caus["scratch"] == 0 and caus["mfma_total"] == plain["mfma_total"] == 6


# ---------------------------------------------------------------- what a plan records
def test_causal_plan_records_the_mask_in_both_forms():
    """[1,4,16,8,40]: HW = 320 / 80 / 20 take the fused launch, HW = 5 (not a multiple of 20) the standalone kernel; every temporal
    self-attention of the model -- attn1 AND attn2 (attention.py:217-218) -- is causal, no spatial launch changes"""
    _, pc = cpu_plan(dict(REDUCED, use_causal_attention=True), 1, 16, 8, 40, 77)
    _, pp = cpu_plan(REDUCED, 1, 16, 8, 40, 77)
    nc, npl = _names(pc), _names(pp)
    assert len(nc) == len(npl)
    assert nc.count("gemm:tattn_causal") == npl.count("gemm:tattn") > 0 and "gemm:tattn" not in nc
    assert nc.count("temporal_attention_causal") == npl.count("temporal_attention") > 0 and "temporal_attention" not in nc
    assert nc.count("gemm:tattn_causal") + nc.count("temporal_attention_causal") == 2 * 17        # attn1 and attn2 of 17 blocks
    swap = {"gemm:tattn_causal": "gemm:tattn", "temporal_attention_causal": "temporal_attention"}
    assert [swap.get(n, n) for n in nc] == npl


def test_causal_forward_with_another_frame_count_is_refused():
    with pytest.raises(ValueError, match=r"T = 8 .*temporal_length = 16"):
        cpu_plan(dict(REDUCED, use_causal_attention=True), 1, 8, 16, 16, 77)
    # both flags: the mask is never used, so no T is refused (the reference runs such a forward)
    cpu_plan(dict(REDUCED, use_causal_attention=True, temporal_selfatt_only=False), 1, 4, 16, 16, 77)


def test_temporal_cross_refuses_maps_the_reference_fails_on():
    with pytest.raises(ValueError, match=r"hw = 4 .*T = 8"):      # 16 x 16 latents: the lowest level has 2 x 2 pixels
        cpu_plan(dict(REDUCED, temporal_selfatt_only=False), 1, 8, 16, 16, 77)


def test_temporal_cross_joins_the_upfront_context_gemm():
    m, pl = cpu_plan(dict(REDUCED, temporal_selfatt_only=False), 2, 4, 16, 16, 77)
    mp, pp = cpu_plan(REDUCED, 2, 4, 16, 16, 77)
    tcross = [b.attn2 for t in m.modules() if type(t).__name__ == "_TemporalTransformer" for b in t.transformer_blocks]
    assert len(tcross) == 17 and all(id(a) in m._kv_cols for a in tcross) and len(m._kv_cols) == 17 + 16
    width = sum(2 * inner for _, inner in m._kv_cols.values())
    assert pl.kv_all.shape == (2 * 77, width) and width == pp.kv_all.shape[1] + sum(2 * a.to_k.weight.shape[0] for a in tcross)
    cols = sorted(m._kv_cols.values())                            # disjoint column ranges that tile the GEMM's output
    assert cols[0][0] == 0 and all(a[0] + 2 * a[1] == b[0] for a, b in zip(cols, cols[1:]))
    n, npl = _names(pl), _names(pp)
    # still ONE context GEMM in front of everything; 17 more cross-attention launches, 17 fewer temporal self-attentions
    assert n.count("attention") == npl.count("attention") + 17
    assert n.count("temporal_attention") + n.count("gemm:tattn") == npl.count("temporal_attention") + npl.count("gemm:tattn") - 17
    ctx_gemms = [s for s in pl.steps if s.func.__name__ == "gemm" and s.args[0] is pl.ctx]
    assert len(ctx_gemms) == 1 and ctx_gemms[0].args[2].data_ptr() == pl.kv_all.data_ptr()
    # every temporal cross-attention reads its own columns of that one buffer, one K|V per video (kv_div = T)
    cross = [s for s in pl.steps if s.func.__name__ == "attention" and s.keywords["kv_div"] == 4 and s.keywords["Nk"] == 77]
    assert len(cross) == 33 and all(s.keywords["ldk"] == width for s in cross)


def test_shared_prefix_ends_at_the_first_cross_attention_of_either_kind():
    """with addition_attention the first cross-attention of a temporal-cross model is init_attn's attn2, right behind conv_in: the
    branches of a shared-latents plan separate there (one `repeat` for h, one for the transformer's outer residual)"""
    segs = ((1, 154), (1, 77))
    _, pl = cpu_plan(dict(REDUCED, temporal_selfatt_only=False), 2, 4, 16, 16, segs, shared_x=True)
    _, pp = cpu_plan(REDUCED, 2, 4, 16, 16, segs, shared_x=True)
    n, npl = _names(pl), _names(pp)
    first, first_plain = n.index("repeat"), npl.index("repeat")
    convs = lambda names: sum(1 for s in names if s == "gemm")
    assert first < first_plain
    # in front of the split: the embedding MLPs, the context GEMM, conv_in, init_attn's proj_in, its attn1 (+ to_out) and attn2's to_q
    # and the two segments' cross-attention launches; the plain model's prefix also holds the rest of init_attn and the first ResBlock
    assert "attention" in n[first - 3:first] and n[:first].count("attention") == 2 == n[first - 3:first].count("attention")
    assert convs(n[:first]) < convs(npl[:first_plain])
    assert pl.x_in.shape[0] == 1 and pl.out.shape[0] == 2


def test_full_configuration_records_the_parent_commits_launch_list():
    """no behaviour change for existing models: the launch list of the FULL (t2v) configuration at the headline shape -- names, operand
    shapes, every scalar argument (plan_cpu.signature) -- AND the buffer every operand of a launch is bound to (plan_cpu.aliases:
    which pool buffer a launch was handed, when it went back) equal the lists recorded at the parent commit
    (tests/golden/plan_full_launches.npz; tools/record_parent_fixtures.py --plans re-records it when a plan change is meant), for
    every plan of plan_cpu.fixture_plans: seven signatures of the FULL configuration and the hybrid `pieces` plan of the reduced one.
    The heaviest test of the CPU set (~15 s: the full-width tree is packed ONCE on the host and serves its seven plans); the reduced
    model would not do -- the kernel choices under test (fused temporal attention, GroupNorm folds, split-K) depend on the full widths."""
    g = golden("plan_full_launches")
    tags = []
    for tag, plan in fixture_plans(FULL, REDUCED):
        tags.append(tag)
        for key, got in ((tag, signature(plan)), (tag + ".aliases", aliases(plan))):
            want = [str(s) for s in g[key]]
            assert len(got) == len(want), key
            diff = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
            assert not diff, f"{key}: {len(diff)} launches differ from the parent commit's, first: {diff[0]}"
    assert sorted(g.files) == sorted(tags + [t + ".aliases" for t in tags]) and len(tags) == 8
