#!/usr/bin/env python3
"""Record the "as at another commit" fixtures of tests/test_temporal_variants_{cpu,gpu}.py and tests/test_sampler_routes_cpu.py from a
CHECKOUT of that commit (its tree with its own built libmoca_hip.so), so that they can be audited and re-recorded when a plan
optimisation or a compiler bump legitimately changes them:

  tests/golden/plan_full_launches.npz            (--plans, no GPU)  the launch lists of tests/plan_cpu.py::fixture_plans (seven plans of
                                                 the FULL configuration, the hybrid `pieces` plan of the reduced one), one line per
                                                 launch: `<tag>` = what is launched (plan_cpu.signature), `<tag>.aliases` = which
                                                 buffer every operand is (plan_cpu.aliases)
  tests/golden/temporal_attention_parent_sha.npz (--sha, on the GPU)  sha256 of the outputs of moca_temporal_attention_f16 and of the
                                                 non-causal MOCA_EP_TATTN launch on the host-generated operands of
                                                 tests/temporal_variants_ref.py
  tests/golden/attention_parent_sha.npz          (--attention-sha, on the GPU)  sha256 of the outputs of every kernel of csrc/attention.hip
                                                 (and of moca_attention_d80_f16) on the cases and host-generated operands of
                                                 tests/attention_edges_ref.py::PARENT_CASES
  tests/golden/norm_parent_sha.npz               (--norm-sha, on the GPU)  sha256 of what every launch of the GroupNorm family of csrc/norm.hip
                                                 leaves on the cases and host-generated operands of
                                                 tests/norm_edges_ref.py::parent_names (outputs, and the accumulators the concat /
                                                 accum launches add to)
  tests/golden/gemm_persistent_parent_sha.npz    (--persistent-sha, on the GPU)  sha256 of the output rows of the persistent GEMM kernels
                                                 of csrc/gemm_persistent.hip (g4p, g4q, sqp) on the cases and host-generated operands
                                                 of tests/gemm_edges_ref.py::PERSISTENT_PARENT_CASES
  tests/golden/sampler_routes.npz                (--samplers, no GPU)  the traces of tests/sampler_routes_cpu.py::record: the UNet entry
                                                 points and launches of the sampling layer (guidance routing, host-issued loops,
                                                 ddim_step, queue noising, the host-driven FIFO loop, `supported()` tables, the
                                                 three trajectory engines' launches, resets, refusals and cache hits) as lines,
                                                 the coefficient tables as arrays

    git worktree add ../base <commit> && make -C ../base/moca_video_amd/csrc
    python tools/record_parent_fixtures.py --tree ../base --plans          (any host)
    python tools/record_parent_fixtures.py --tree ../base --sha            (on the MI355X)
    python tools/record_parent_fixtures.py --tree ../base --attention-sha  (on the MI355X)
    python tools/record_parent_fixtures.py --tree ../base --norm-sha       (on the MI355X)
    python tools/record_parent_fixtures.py --tree ../base --persistent-sha (on the MI355X)
    python tools/record_parent_fixtures.py --tree ../base --samplers       (any host)

The package is imported from --tree, the helpers (tests/plan_cpu.py, tests/temporal_variants_ref.py, tests/attention_edges_ref.py,
tests/norm_edges_ref.py, tests/gemm_edges_ref.py) and the output directory are this checkout's.  A tree older than the host-recordable plan (no `UNetModel._pack(dev)`, a stream created unconditionally) is recorded
through two stand-ins defined here; nothing of it is modified."""
import argparse
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(HERE, "tests", "golden")


def record_plans():
    import inspect
    from moca_video_amd import UNetModel, ops
    import moca_video_amd.unet as U
    if "dev" not in inspect.signature(UNetModel._pack).parameters:          # a tree from before the host-recordable plan
        class _NoStream:
            def __init__(self, *a, **k):
                pass
        torch.cuda.Stream = _NoStream

        def _pack(self, dev=None):
            P, self._emb_cols, self._kv_cols = U.pack_tree(self, dev)
            f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
            for sq in (self.time_embed,) + ((self.fps_embedding,) if self.fps_cond else ()):
                for m in (sq[0], sq[2]):
                    P[id(m)] = ops.pack_linear(m.weight.detach(), m.bias.detach(), device=dev)
            cin = self.input_blocks[0][0]
            P[id(cin)] = ops.pack_conv3x3(cin.weight.detach(), cin.bias.detach(), cpad=self.in_cpad, device=dev)
            P[id(self.out[0])] = (f32(self.out[0].weight), f32(self.out[0].bias))
            P[id(self.out[2])] = ops.pack_conv3x3(self.out[2].weight.detach(), self.out[2].bias.detach(), device=dev)
            self._packed = P
        UNetModel._pack = _pack
    from helpers import FULL, REDUCED
    import plan_cpu
    out = {}
    for tag, plan in plan_cpu.fixture_plans(FULL, REDUCED):
        sig, ali = plan_cpu.signature(plan), plan_cpu.aliases(plan)
        print(f"{tag}: {len(sig)} launches, {1 + max(int(n) for l in ali for n in re.findall(r'#([0-9]+)', l))} buffers")
        out[tag], out[tag + ".aliases"] = np.asarray(sig), np.asarray(ali)
    np.savez_compressed(os.path.join(GOLD, "plan_full_launches.npz"), **out)


def record_sha():
    from moca_video_amd import ops
    import temporal_variants_ref as R
    names, shas = [], []
    for B, T, HW, heads in R.STANDALONE:
        C = heads * 64
        qkv = R.standalone_operands(B, T, HW, heads)
        out = torch.zeros(B * T * HW, C, dtype=torch.float16, device="cuda")
        ops.temporal_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, B=B, T=T, HW=HW, heads=heads, ld_qkv=3 * C, ldo=C,
                               scale=R.SCALE)
        torch.cuda.synchronize()
        names.append(f"standalone.{B}.{T}.{HW}.{heads}")
        shas.append(R.sha(out))
    for B, HW, heads, K, fold in R.FUSED:
        x, ws, gb = R.fused_operands(B, HW, heads, K, fold)
        out = R.fused_run(ops, x, ws, gb, B, HW, heads, False)
        torch.cuda.synchronize()
        names.append(f"fused.{B}.{HW}.{heads}.{K}.{int(fold)}")
        shas.append(R.sha(out))
    for n, s in zip(names, shas):
        print(n, s)
    np.savez_compressed(os.path.join(GOLD, "temporal_attention_parent_sha.npz"), names=np.asarray(names), sha256=np.asarray(shas))


def record_attention_sha():
    from moca_video_amd import ops
    import attention_edges_ref as R
    names, shas = [], []
    for route, name, kind, p in R.PARENT_CASES:
        out = R.run_parent_case(ops, name, kind, p)
        torch.cuda.synchronize()
        assert not torch.isnan(out).any(), f"{name}: an output row was not written"
        names.append(name)
        shas.append(R.sha(out))
        print(route, name, shas[-1])
    np.savez_compressed(os.path.join(GOLD, "attention_parent_sha.npz"), names=np.asarray(names), sha256=np.asarray(shas))


def record_norm_sha():
    import norm_edges_ref as R
    names, shas = [], []
    for group in R.PARENT_GROUPS:
        got = R.parent_hashes(group)
        torch.cuda.synchronize()
        assert list(got) == R.parent_names(group)
        for n, h in got.items():
            names.append(n)
            shas.append(h)
            print(group, n, h)
    np.savez_compressed(os.path.join(GOLD, "norm_parent_sha.npz"), names=np.asarray(names), sha256=np.asarray(shas))


def record_persistent_sha():
    import gemm_edges_ref as R
    names, shas = [], []
    for route in R.PARENT_ROUTES:
        got = R.persistent_parent_hashes(route)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        for n, h in got.items():
            names.append(n)
            shas.append(h)
            print(route, n, h)
    assert names == [n for _, n, _ in R.PERSISTENT_PARENT_CASES]
    np.savez_compressed(os.path.join(GOLD, "gemm_persistent_parent_sha.npz"), names=np.asarray(names), sha256=np.asarray(shas))


def record_samplers():
    import sampler_routes_cpu
    out = sampler_routes_cpu.record()
    print(f"{len(out)} traces, {sum(len(v) for k, v in out.items() if v.dtype.kind == 'U')} lines")
    np.savez_compressed(os.path.join(GOLD, "sampler_routes.npz"), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="checkout (with its built library) to record from")
    ap.add_argument("--plans", action="store_true")
    ap.add_argument("--sha", action="store_true")
    ap.add_argument("--attention-sha", action="store_true")
    ap.add_argument("--norm-sha", action="store_true")
    ap.add_argument("--persistent-sha", action="store_true")
    ap.add_argument("--samplers", action="store_true")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    sys.path.insert(1, os.path.join(HERE, "tests"))
    import moca_video_amd
    assert os.path.abspath(moca_video_amd.__file__).startswith(tree + os.sep), f"moca_video_amd came from {moca_video_amd.__file__}"
    if a.plans:
        record_plans()
    if a.sha:
        record_sha()
    if a.attention_sha:
        record_attention_sha()
    if a.norm_sha:
        record_norm_sha()
    if a.persistent_sha:
        record_persistent_sha()
    if a.samplers:
        record_samplers()


if __name__ == "__main__":
    main()
