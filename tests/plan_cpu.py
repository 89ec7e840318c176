"""Record a UNet plan on the HOST (no GPU): `_Plan` only binds pointers and records C-ABI calls while it is built, so its launch list can be
read -- never run -- on torch.device("cpu").  `signature()` turns the list into one line per launch: the wrapper's name, the shapes of
its tensor arguments and every scalar keyword (tensor keywords as their shape), i.e. everything of a launch but the addresses."""
import torch


def cpu_plan(cfg, B, T, H, W, L, **kw):
    from moca_video_amd import UNetModel
    from moca_video_amd.plan import _Plan
    m = UNetModel(**cfg)
    dev = torch.device("cpu")
    m._pack(dev)
    return m, _Plan(m, B, T, H, W, L, torch.float32, dev, **kw)


def _show(v):
    if torch.is_tensor(v):
        return "t" + "x".join(str(int(s)) for s in v.shape)
    if isinstance(v, (tuple, list)):
        return "(" + ",".join(_show(x) for x in v) + ")"
    if isinstance(v, float):
        return f"{v:.6g}"
    if hasattr(v, "w") and hasattr(v, "N"):                      # ops.PackedWeight
        return f"pw[N={v.N},K={v.K},geglu={int(bool(v.geglu))}]"
    return str(v)


def signature(plan):
    out = []
    for s in plan.steps:
        args = ",".join(_show(a) for a in s.args)
        kws = ",".join(f"{k}={_show(v)}" for k, v in sorted(s.keywords.items()) if v is not None)
        out.append(f"{s.func.__name__}({args};{kws})")
    return out


def aliases(plan):
    """what `signature` leaves out: WHICH buffer every operand of a launch is.  One line per launch; every tensor reachable from the
    step's arguments and sorted keywords (inside tuples, a PackedWeight's `w` and `bias`) appears as the ordinal of the first
    appearance of its address in the list.  The steps keep all their tensors alive, so no address is ever recycled, and two builds
    of one plan give the same lines: the lines pin which pool buffer a launch was handed and when it went back to the pool."""
    seen = {}

    def show(v):
        if torch.is_tensor(v):
            return f"#{seen.setdefault(v.data_ptr(), len(seen))}"
        if isinstance(v, (tuple, list)):
            return "(" + ",".join(x for x in map(show, v) if x) + ")"
        if hasattr(v, "w") and hasattr(v, "N"):                  # ops.PackedWeight
            return f"pw[{show(v.w)},{show(v.bias)}]"
        return ""
    out = []
    for s in plan.steps:
        args = ",".join(show(a) for a in s.args)
        kws = ",".join(f"{k}={x}" for k, x in ((k, show(v)) for k, v in sorted(s.keywords.items())) if x and x != "()")
        out.append(f"{s.func.__name__}({args};{kws})")
    return out


# the plans of tests/golden/plan_full_launches.npz, shared by the recorder (tools/record_parent_fixtures.py --plans) and the test
# (tests/test_temporal_variants_cpu.py): (tag, (B, T, H, W, L), keywords).  The FULL ones together reach the slab -> gemm_splitk_groupnorm
# move, the finished-statistics re-target, groupnorm_fold_weights with wgroup, the virtual concat with re-targeted and gstat_accum
# shares, concat_channels_gstat, repeat, nchw_add_rows (adapter = the FULL model's four sites), the up-phase convs, prefetch re-targets,
# the plain groupnorm / layernorm fallbacks and all three temporal-attention forms
FULL_PLANS = (
    ("b1_77", (1, 16, 40, 64, 77), {}),
    ("cfg_shared", (2, 16, 40, 64, ((1, 77), (1, 77))), dict(shared_x=True)),
    ("fifo_b8", (8, 16, 40, 64, ((4, 154), (4, 77))), {}),
    ("long32", (1, 32, 40, 64, 77), {}),
    ("adapter", (2, 16, 40, 64, ((1, 77), (1, 77))), dict(shared_x=True, adapter=4)),
    ("small", (1, 8, 16, 16, 77), {}),
    ("odd", (1, 16, 20, 36, 77), {}),
)
# the hybrid `pieces` plan (x_rows outside the pool, ncthw_scatter) on the reduced 8-channel model of tests/test_hybrid_cpu.py
HYBRID_PLANS = (
    ("hybrid", (2, 8, 16, 16, ((1, 77), (1, 77))), dict(shared_x=True, pieces=(4,))),
)


def fixture_plans(full_cfg, reduced_cfg):
    """yields (tag, plan) for every entry of the fixture; each model is packed once on the host (the FULL one takes ~15 s)"""
    from moca_video_amd import UNetModel
    from moca_video_amd.plan import _Plan
    dev = torch.device("cpu")
    for cfg, plans in ((full_cfg, FULL_PLANS), (dict(reduced_cfg, in_channels=8), HYBRID_PLANS)):
        m = UNetModel(**cfg)
        m._pack(dev)
        for tag, args, kw in plans:
            yield tag, _Plan(m, *args, torch.float32, dev, **kw)
