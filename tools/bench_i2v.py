#!/usr/bin/env python3
"""Image cross-attention timings on the GPU, alternating A / B on the same device (profiles/r07_i2v_*.txt):

  kernel: moca_attention_ip_f16 at Bq = 32, heads 5, Nq = 2560, Nt = 77, Ni = 16 against moca_attention_f16 at Nk = 77 (same q / K / V);
  step:   the B = 2 classifier-free-guidance UNet forward of the full-width model (shared-prefix plan, both branches in one hipGraph) with
          93-token contexts on the image-attention UNet against 77-token contexts on the t2v UNet, [2, 4, 16, 40, 64] latents.

    python tools/bench_i2v.py [kernel|step ...] [--reps N]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n       # us per call


def alternate(fa, fb, reps, inner):
    for f in (fa, fb):
        timed(f, inner)                       # warm-up
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa, inner))
        tb.append(timed(fb, inner))
    return statistics.median(ta), statistics.median(tb), min(ta), min(tb)


def kernel(reps):
    from moca_video_amd import ops
    Bq, h, Nq, C = 32, 5, 2560, 320
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).half().cuda()
    q, kv, kvi = r(Bq, Nq, C), r(Bq // 16, 77, 2 * C), r(Bq // 16, 16, 2 * C)
    o = torch.empty(Bq, Nq, C, dtype=torch.float16, device="cuda")
    fa = lambda: ops.attention(q, kv[..., :C], kv[..., C:], o, Bq=Bq, heads=h, Nq=Nq, Nk=77, ldq=C, ldk=2 * C, ldv=2 * C, ldo=C,
                               kv_div=16, scale=0.125)
    fb = lambda: ops.attention_ip(q, kv[..., :C], kv[..., C:], kvi[..., :C], kvi[..., C:], o, Bq=Bq, heads=h, Nq=Nq, Nt=77, Ni=16,
                                  ldq=C, ldk=2 * C, ldv=2 * C, ldk_ip=2 * C, ldv_ip=2 * C, ldo=C, kv_div=16, scale=0.125, ip_scale=1.0)
    ma, mb, na, nb = alternate(fa, fb, reps, 50)
    return (f"kernel  Bq=32 h=5 Nq=2560 kv_div=16 (B=2 x 16 frames)\n"
            f"  moca_attention_f16     Nk=77        median {ma:8.2f} us  min {na:8.2f} us\n"
            f"  moca_attention_ip_f16  Nt=77 Ni=16  median {mb:8.2f} us  min {nb:8.2f} us\n"
            f"  ratio (median) {mb / ma:.3f}   (target <= 1.10)\n")


def step(reps):
    from helpers import FULL, inp
    from moca_video_amd import UNetModel
    from moca_video_amd.weightgen import gen_state_dict
    res = {}
    models = {}
    for tag, kw, L in (("t2v", {}, 77), ("i2v", {"use_image_attention": True}, 93)):
        m = UNetModel(**dict(FULL, **kw))
        m.load_state_dict(gen_state_dict({k: v.shape for k, v in m.state_dict().items()}, 11), strict=True)
        models[tag] = (m.cuda(), L)
    x = inp("bench_i2v.x", (1, 4, 16, 40, 64)).cuda()
    t = torch.tensor([500]).cuda()
    fps = torch.tensor([16]).cuda()
    calls = {}
    for tag, (m, L) in models.items():
        c, u = inp("bench_i2v.c", (1, L, 1024)).cuda(), inp("bench_i2v.u", (1, L, 1024)).cuda()
        calls[tag] = (lambda m=m, c=c, u=u: m.forward_segments(x, t, [c, u], fps=[fps, fps], shared_x=True))
    ma, mb, na, nb = alternate(calls["t2v"], calls["i2v"], reps, 5)
    return (f"step    B=2 CFG UNet forward (shared prefix, one hipGraph), full width, latents [1, 4, 16, 40, 64] x 2 branches\n"
            f"  t2v  77-token contexts  median {ma / 1e3:8.3f} ms  min {na / 1e3:8.3f} ms\n"
            f"  i2v  93-token contexts  median {mb / 1e3:8.3f} ms  min {nb / 1e3:8.3f} ms\n"
            f"  ratio (median) {mb / ma:.4f}   (target <= 1.015)\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "step"])
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"device: {torch.cuda.get_device_name(0)}")
    for w in a.what:
        print({"kernel": kernel, "step": step}[w](a.reps), flush=True)


if __name__ == "__main__":
    main()
