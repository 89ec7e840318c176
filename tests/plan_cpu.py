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
