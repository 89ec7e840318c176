"""CPU: the references, case tables and the bound of tests/test_small_kernels_gpu.py check themselves (tests/small_kernels_ref.py).

  test_reference_stays_inside_the_bound . for every arithmetic case the fp32 torch evaluation rounded to fp16 -- for LayerNorm and softmax
                                          also the fp32 restatement that sums in the kernel's order -- is within `bound` of the float64
                                          restatement on every element (prints the worst ratio per kernel: the ref module's docstring)
  test_cases_tell_errors ................ at every case each wrong restatement that applies (small_kernels_ref.MUTANTS) breaks the
                                          case's own check, evaluated in fp32 and rounded as a wrong kernel would; every wrong restatement
                                          applies to at least one case
  test_fp32_kernels_reference ........... cfg_combine / ddim_update in fp32 are the float64 restatement to fp32 rounding, and the wrap cases
                                          sit on both sides of the grid cap
  test_ledger ........................... every key of lib.SIGNATURES has GPU tests that exist, or a reason why it has none
  test_case_ids_name_the_edges .......... all eight layernorm_kernel instantiations and both sides of every grid cap appear in case ids"""
import importlib

import pytest
import torch

import small_kernels_ref as R

BIG = 1 << 21          # cases above this many output elements are checked on their head, tail and cap neighbourhood rows only


def _ln_eval(c):
    x, gamma, beta = R.ln_inputs(c)
    if x.numel() > BIG:                                   # rows are independent: the first and last 24 rows say what every row says
        x = torch.cat([x[:24], x[-24:]])
    ref = R.layernorm(x, gamma, beta, c["eps"])
    f32 = R.layernorm(x, gamma, beta, c["eps"], torch.float32)
    return x, gamma, beta, ref, f32, R.slack_of(f32, ref)


def _sm_eval(c):
    s = R.softmax_inputs(c)
    ref = R.softmax_rows(s, c["scale"])
    f32 = R.softmax_rows(s, c["scale"], torch.float32)
    return s, ref, f32, R.slack_of(f32, ref)


def _silu_eval(c, dtype, wrong=None):
    a, b = R.silu_inputs(c)
    return R.silu_add_rows(a, c["div_a"], b, c["div_b"] or 1, c["rows"], c["silu"], dtype, wrong)


def _ts_eval(c, dtype, wrong=None):
    return R.timestep_embedding(R.timestep_inputs(c), c["dim"], c["max_period"], dtype, wrong)


def _mix_eval(c, dtype, wrong=None):
    z, w, bias = R.mix_inputs(c)
    return R.channel_mix(z, w, bias, c["Cpad"], c["inv_scale"], dtype, wrong)


def _gauss_eval(c, dtype, wrong=None):
    mom, noise = R.gauss_inputs(c)
    return R.gaussian_sample(mom, noise, c["scale"], dtype, wrong)


def _embed_eval(c, dtype, wrong=None):
    return R.embed_tokens(*R.embed_inputs(c), dtype, wrong)


ELEMENTWISE = {"silu_add_rows": (R.SILU_CASES, _silu_eval), "timestep_embedding": (R.TIMESTEP_CASES, _ts_eval),
               "channel_mix": (R.MIX_CASES, _mix_eval), "embed_tokens": (R.EMBED_CASES, _embed_eval)}


def test_reference_stays_inside_the_bound():
    worst = {}
    w_t = w_k = 0.0
    for name, c in R.LN_CASES.items():
        x, gamma, beta, ref, f32, slack = _ln_eval(c)
        a, b = R.worst(f32.half(), ref, slack), R.worst(R.layernorm_kernel_order(x, gamma, beta, c["eps"]).half(), ref, slack)
        assert a <= 1.0 and b <= 1.0, f"layernorm {name}: torch {a:.2f}, kernel order {b:.2f} of the bound"
        w_t, w_k = max(w_t, a), max(w_k, b)
    worst["layernorm"] = (w_t, w_k)
    w_t = w_k = w_s = 0.0
    for name, c in R.SOFTMAX_CASES.items():
        s, ref, f32, slack = _sm_eval(c)
        ko = R.softmax_kernel_order(s, c["scale"]).half()
        a, b = R.worst(f32.half(), ref, slack), R.worst(ko, ref, slack)
        assert a <= 1.0 and b <= 1.0, f"softmax {name}: torch {a:.2f}, kernel order {b:.2f} of the bound"
        rs = ((ko.double().sum(-1) - 1).abs() / R.softmax_sum_bound(ref, c["N"], slack)).max().item()
        assert rs <= 1.0, f"softmax {name}: row sums {rs:.2f} of their bound"
        if c["fill"] == "one_finite":
            assert ko.max(-1).values.eq(1.0).all() and ko.sum(-1).eq(1.0).all()
        w_t, w_k, w_s = max(w_t, a), max(w_k, b), max(w_s, rs)
    worst["softmax_rows"] = (w_t, w_k, w_s)
    for op, (cases, ev) in ELEMENTWISE.items():
        w = 0.0
        for name, c in cases.items():
            ref, f32 = ev(c, torch.float64), ev(c, torch.float32)
            a = R.worst(f32.half(), ref, R.slack_of(f32, ref))
            assert a <= 1.0, f"{op} {name}: torch {a:.2f} of the bound"
            w = max(w, a)
        worst[op] = (w,)
    w = 0.0
    for name, c in R.GAUSS_CASES.items():
        ref, f32 = _gauss_eval(c, torch.float64), _gauss_eval(c, torch.float32)
        a = R.worst(f32, ref, R.slack_of(f32, ref), R.bound_f32_exp)
        assert a <= 1.0, f"gaussian_sample {name}: torch {a:.2f} of the bound"
        w = max(w, a)
    worst["gaussian_sample"] = (w,)
    print("\nworst |err| / bound: " + ", ".join("%s %s" % (k, "/".join("%.2f" % v for v in vs)) for k, vs in worst.items()))


def _breaks(bad16, ref, slack, what):
    r = R.worst(bad16, ref, slack)
    assert r > 1.0, f"{what}: the wrong restatement stays within {r:.2f} of the bound"


def test_cases_tell_errors():
    seen = set()
    for name, c in R.LN_CASES.items():
        x, gamma, beta, ref, f32, slack = _ln_eval(c)
        for wrong in R.ln_wrongs(c):
            seen.add(wrong)
            bad = R.layernorm(x, gamma, beta, c["eps"], torch.float32, wrong).half()
            _breaks(bad, ref, slack, f"layernorm {name} {wrong}")
            if wrong == "var_over_c_minus_1" and c["C"] == 520 and c["kind"] == "randn":      # 1 / (2 C) = one fp16 ulp: nearly half the elements
                share = (R.ratio(bad, ref, slack) > 1).float().mean().item()
                assert share > 0.4, f"layernorm {name} {wrong}: only {share:.0%} of the elements leave the bound"
    for name, c in R.SOFTMAX_CASES.items():
        s, ref, f32, slack = _sm_eval(c)
        for wrong in c["wrongs"]:
            seen.add(wrong)
            _breaks(R.softmax_rows(s, c["scale"], torch.float32, wrong).half(), ref, slack, f"softmax {name} {wrong}")
    for op, (cases, ev) in ELEMENTWISE.items():
        for name, c in cases.items():
            ref, f32 = ev(c, torch.float64), ev(c, torch.float32)
            for wrong in c["wrongs"]:
                seen.add(wrong)
                _breaks(ev(c, torch.float32, wrong).half(), ref, R.slack_of(f32, ref), f"{op} {name} {wrong}")
    for name, c in R.GAUSS_CASES.items():
        ref, f32 = _gauss_eval(c, torch.float64), _gauss_eval(c, torch.float32)
        for wrong in c["wrongs"]:
            seen.add(wrong)
            r = R.worst(_gauss_eval(c, torch.float32, wrong), ref, R.slack_of(f32, ref), R.bound_f32_exp)
            assert r > 1.0, f"gaussian_sample {name} {wrong}: within {r:.2f} of the bound"
    # exact operations: the wrong restatement must not be equal
    for name, c in R.TO_NHWC_CASES.items():
        x = torch.randn(c["B"], c["Cin"], c["T"], c["HW"], generator=R.gen(c["seed"]))
        x = x if c["f32"] else x.half()
        for wrong in c["wrongs"]:
            seen.add(wrong)
            assert not torch.equal(R.ncthw_to_nhwc(x, c["Cpad"], wrong), R.ncthw_to_nhwc(x, c["Cpad"])), (name, wrong)
    for name, c in R.FROM_NHWC_CASES.items():
        y = R.randh(R.gen(c["seed"]), c["B"] * c["T"] * c["HW"], c["ld"])
        dt = torch.float32 if c["f32"] else torch.float16
        for wrong in c["wrongs"]:
            seen.add(wrong)
            assert not torch.equal(R.nhwc_to_ncthw(y, c["B"], c["Cout"], c["T"], c["HW"], dt, wrong),
                                   R.nhwc_to_ncthw(y, c["B"], c["Cout"], c["T"], c["HW"], dt)), (name, wrong)
    for name, c in R.FREEINIT_CASES.items():
        if name.startswith("wrap"):
            continue                                      # (the same wrong restatement at 1M bins: the small odd shapes already tell it)
        x, n, lpf = R.freeinit_inputs(c)
        ref = R.freq_mix_3d(x, n, lpf)
        for wrong in c["wrongs"]:
            seen.add(wrong)
            e = ((R.freq_mix_3d(x, n, lpf, wrong) - ref).abs().max() / ref.abs().max()).item()
            assert e > 100 * R.FREEINIT_TOL, (name, wrong, e)
    missing = {w for ws in R.MUTANTS.values() for w in ws} - seen
    assert not missing, f"wrong restatements no case applies: {missing}"


def test_fp32_kernels_reference():
    for name, c in list(R.CFG_CASES.items())[:1]:
        ec, eu = R.randn_set(c["seed"], c["n"], 2)
        f32, ref = R.cfg_combine(ec, eu, c["scale"], torch.float32), R.cfg_combine(ec, eu, c["scale"])
        assert f32.dtype == torch.float32 and (f32.double() - ref).abs().max() <= 4 * 2.0 ** -24 * ref.abs().max()
    for name, c in list(R.DDIM_CASES.items())[:2]:
        x, e, nz = R.randn_set(c["seed"], c["n"], 3)
        for got, ref in zip(R.ddim_update(x, e, nz, use_scale=c["use_scale"], dtype=torch.float32, **R.DDIM_ARGS),
                            R.ddim_update(x, e, nz, use_scale=c["use_scale"], **R.DDIM_ARGS)):
            assert got.dtype == torch.float32 and (got.double() - ref).abs().max() <= 8 * 2.0 ** -24 * ref.abs().max()
    assert R.GRID_CAP == 1 << 20 and R.WRAP == R.GRID_CAP + 300 and R.WRAP % 4 == 0 and R.ZERO_CAP == 1 << 18
    C, T, H, W = R.FREEINIT_CASES["wrap_c4_t5_h229_w229"]["shape"]
    assert C * T * H * W > R.GRID_CAP and T % 2 and H % 2 and W % 2
    # the caps are what the sources say
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "moca_video_amd", "csrc")
    common = open(os.path.join(csrc, "common.h")).read()
    assert common.count("if (g > 4096) g = 4096;") == 1 and common.count("int grid_for(") == 1
    for f in ("elementwise.hip", "sampler.hip", "fifo.hip", "freeinit.hip"):          # ... once: every launch goes through common.h's
        s = open(os.path.join(csrc, f)).read()
        assert "grid_for(" in s and "int grid_for" not in s and "4096" not in s, f
    assert "if (blocks > 1024) blocks = 1024;" in open(os.path.join(csrc, "runtime.hip")).read()


def test_ledger():
    from moca_video_amd import lib
    assert not set(R.LEDGER) & set(R.LEDGER_EXEMPT)
    assert set(R.LEDGER) | set(R.LEDGER_EXEMPT) == set(lib.SIGNATURES), \
        f"unaccounted: {set(lib.SIGNATURES) - set(R.LEDGER) - set(R.LEDGER_EXEMPT)}, unknown: {(set(R.LEDGER) | set(R.LEDGER_EXEMPT)) - set(lib.SIGNATURES)}"
    assert all(R.LEDGER_EXEMPT.values()) and len(R.LEDGER_EXEMPT) <= 16
    for sym, tests in R.LEDGER.items():
        assert tests, sym
        for t in tests:
            mod, fn = t.split("::")
            assert mod.endswith("_gpu"), t
            m = importlib.import_module(mod)
            assert callable(getattr(m, fn, None)), f"{sym}: {t} does not exist"
            marks = [k.name for k in getattr(m, "pytestmark", [])] if isinstance(getattr(m, "pytestmark", None), list) \
                else [getattr(getattr(m, "pytestmark", None), "name", None)]
            assert "gpu" in marks or any(k.name == "gpu" for k in getattr(getattr(m, fn), "pytestmark", [])), f"{t} is not a GPU test"


def test_case_ids_name_the_edges():
    inst = {n.split("_")[-1] if not n.endswith("gamma0") else n.split("_")[-2] for n in R.LN_CASES}
    assert inst == {"ln%dx%d" % (a, b) for a in (1, 2, 3, 5) for b in (1, 4)}
    for c in R.LN_CASES.values():
        assert R.ln_instantiation(c["M"], c["C"]) in ("ln1x1", "ln2x1", "ln3x1", "ln5x1", "ln1x4", "ln2x4", "ln3x4", "ln5x4")
    assert {c["C"] for c in R.LN_CASES.values()} == {8, 512, 520, 1024, 1032, 1536, 1544, 2560}
    assert {c["M"] for c in R.LN_CASES.values()} == {1, 3, 16383, 16384, 16385, 16399}
    for C in (8, 512, 520, 1024, 1032, 1536, 1544, 2560):
        assert {c["M"] >= 16384 for c in R.LN_CASES.values() if c["C"] == C} == {True, False}
    for table in (R.SILU_CASES, R.TIMESTEP_CASES, R.TO_NHWC_CASES, R.FROM_NHWC_CASES, R.CONCAT_CASES, R.REPEAT_CASES, R.MEMSET_CASES,
                  R.MIX_CASES, R.GAUSS_CASES, R.EMBED_CASES, R.CFG_CASES, R.DDIM_CASES, R.FREEINIT_CASES):
        assert any(n.startswith("wrap") for n in table) and any(not n.startswith("wrap") for n in table)
    assert {c["N"] for c in R.SOFTMAX_CASES.values()} >= {4, 252, 256, 260, 2560, 4096}
    assert {c["R"] for c in R.SOFTMAX_CASES.values()} == {1, 5, 8}
