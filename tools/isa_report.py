#!/usr/bin/env python3
"""Static report over the gfx950 code objects inside libmoca_hip.so (no GPU needed: hipcc cross-compiles, llvm-objdump disassembles).

For every kernel: registers / spills / LDS from the code-object metadata, and for its MAIN LOOP (the innermost backward-branch loop
holding the most MFMAs): MFMAs, LDS-DMA loads (`buffer_load ... lds`), LDS fragment reads, barriers and -- the regression guard of
DESIGN 4.1 -- every `s_waitcnt vmcnt(0)` that sits between the first and the last MFMA of the loop body (a full drain of the DMA
stream inside the MFMA segment: what hipcc inserts when it cannot prove an LDS access disjoint from an LDS-DMA in flight, or when a
register that is a known load destination is rewritten).

    python tools/isa_report.py [libmoca_hip.so] [name filter ...]
    python tools/isa_report.py --diff OLD NEW      (two builds of the library or of one object file, e.g. csrc/gemm_tiled.o)

`--diff` is the check of a host-only change: the same kernel symbols, per kernel the same instruction encodings and the same register /
LDS / scratch figures.  Moving host code moves the kernels inside the code object, so two things may differ and are counted, not
failed: the 32-bit literal of an `s_add_u32` (a pc-relative offset to another symbol) and the padding behind a kernel's last
instruction.  Exit status 1 on any other difference.

`analyse(lib_path)` and `kernel_owners(lib_path)` are what tests/test_isa_cpu.py calls."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def code_objects(lib_path, workdir):
    """extract the gfx950 code objects of every translation unit bundled into the shared library"""
    tmp_lib = os.path.join(workdir, "lib.so")
    shutil.copy(lib_path, tmp_lib)                     # (llvm-objdump --offloading writes next to its input)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", tmp_lib], check=True, capture_output=True, cwd=workdir)
    return sorted(os.path.join(workdir, f) for f in os.listdir(workdir) if "amdgcn" in f and f.endswith("gfx950"))


def metadata(co):
    out = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if line.lstrip().startswith("- ") and k in ("agpr_count", "args"):
            cur = {}
        if cur is None:
            continue
        if k == "name" and "kernel" in v and not v.endswith(".kd"):
            cur["name"] = v
            kernels[v] = cur
        elif k in ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
                   "private_segment_fixed_size", "max_flat_workgroup_size"):
            cur[k] = int(v)
    return kernels


_INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")


def disassemble(co):
    """{mangled kernel name: [(addr, mnemonic, operands)]}"""
    out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    funcs, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        m = _INS.match(line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return funcs


def _target(ins, i):
    """address a branch instruction jumps to, or None"""
    a, _, ops = ins[i]
    m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>|<([^>+]+)>$", ops)
    m2 = re.match(r"(\d+)", ops)
    if m and m.group(1):
        return ins[0][0] + int(m.group(1), 16)
    if m2:                                             # raw simm16: target = next instruction + 4 * simm16
        off = int(m2.group(1))
        if off >= 0x8000:
            off -= 0x10000
        return a + 4 + 4 * off
    return None


def natural_loops(ins):
    """the loops of the control-flow graph: {header index: set of instruction indices}, every back edge into a header merged.  Unlike
    loops() (the address span of one backward branch) this holds blocks that hipcc laid out BEFORE the header or after the branch --
    e.g. the store / latch block of gemm_ws_kernel without a residual sits in front of the strip loop's header."""
    addr_to_idx = {a: i for i, (a, _, _) in enumerate(ins)}
    starts = {0}
    for i, (_, mn, _) in enumerate(ins):
        if mn.startswith("s_cbranch") or mn in ("s_branch", "s_endpgm", "s_setpc_b64"):
            starts.add(i + 1)
            t = _target(ins, i)
            if t in addr_to_idx:
                starts.add(addr_to_idx[t])
    starts = sorted(x for x in starts if x < len(ins))
    blocks = [(lo, hi) for lo, hi in zip(starts, starts[1:] + [len(ins)])]
    blk_of = {lo: b for b, (lo, _) in enumerate(blocks)}
    succ = [[] for _ in blocks]
    for b, (lo, hi) in enumerate(blocks):
        mn = ins[hi - 1][1]
        if mn.startswith(("s_cbranch", "s_branch")):
            t = _target(ins, hi - 1)
            if t in addr_to_idx and addr_to_idx[t] in blk_of:
                succ[b].append(blk_of[addr_to_idx[t]])
        if not (mn in ("s_branch", "s_endpgm", "s_setpc_b64")) and b + 1 < len(blocks):
            succ[b].append(b + 1)
    pred = [[] for _ in blocks]
    for b, ss in enumerate(succ):
        for t in ss:
            pred[t].append(b)
    # dominators (iterative; the graphs here are a few hundred blocks)
    allb = set(range(len(blocks)))
    dom = [allb.copy() for _ in blocks]
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for b in range(1, len(blocks)):
            ps = [dom[q] for q in pred[b]]
            nd = (set.intersection(*ps) if ps else set()) | {b}
            if nd != dom[b]:
                dom[b], changed = nd, True
    out = {}
    for b, ss in enumerate(succ):
        for h in ss:
            if h in dom[b]:                            # back edge b -> h
                body, stack = {h, b}, [b]
                while stack:
                    x = stack.pop()
                    if x == h:
                        continue
                    for q in pred[x]:
                        if q not in body:
                            body.add(q)
                            stack.append(q)
                out.setdefault(blocks[h][0], set()).update(body)
    return {hd: {i for bb in body for i in range(*blocks[bb])} for hd, body in out.items()}


def strip_loop(ins):
    """vector-memory stores / atomics of the innermost natural loops holding the most MFMAs (global_ / buffer_ / flat_: what a
    hand-counted `s_waitcnt vmcnt(N)` must count besides the loads), one entry per copy hipcc emitted of such a loop"""
    lps = []
    for body in natural_loops(ins).values():
        mf = sum(1 for i in body if ins[i][1].startswith("v_mfma"))
        if mf:
            lps.append((body, mf))
    inner = [(b, mf) for b, mf in lps if not any(o is not b and o < b and omf for o, omf in lps)]
    if not inner:
        return None
    top = max(mf for _, mf in inner)
    out = []
    for body in sorted((b for b, mf in inner if mf == top), key=min):
        mns = [ins[i][1] for i in body]
        out.append(dict(instructions=len(body), mfma=top, vm_store=sum(1 for mn in mns if mn.startswith(("global_store", "buffer_store", "flat_store"))),
                        vm_atomic=sum(1 for mn in mns if mn.startswith(("global_atomic", "buffer_atomic", "flat_atomic")))))
    return out


def loops(ins):
    """backward branches -> (start index, end index) of loop bodies"""
    addr_to_idx = {a: i for i, (a, _, _) in enumerate(ins)}
    out = []
    for i, (a, mn, ops) in enumerate(ins):
        if mn.startswith("s_cbranch") or mn == "s_branch":
            m = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>|<([^>+]+)>$", ops)
            tgt = None
            m2 = re.match(r"(\d+)", ops)
            if m and m.group(1):
                base = ins[0][0]
                tgt = base + int(m.group(1), 16)
            elif m2:                                   # raw simm16: target = next instruction + 4 * simm16
                off = int(m2.group(1))
                if off >= 0x8000:
                    off -= 0x10000
                tgt = a + 4 + 4 * off
            if tgt is not None and tgt <= a and tgt in addr_to_idx:
                out.append((addr_to_idx[tgt], i))
    return out


def loop_stats(ins, lo, hi):
    body = ins[lo:hi + 1]
    mf = [j for j, (_, mn, _) in enumerate(body) if mn.startswith("v_mfma")]
    st = dict(instructions=len(body), mfma=len(mf), lds_dma=0, ds_read=0, ds_write=0, barrier=0, vmcnt0_inside=0, vmcnt0=0, global_load=0, scratch=0)
    for j, (_, mn, ops) in enumerate(body):
        if (mn.startswith("buffer_load") and re.search(r"\blds\b", ops)) or "_lds_" in mn:
            st["lds_dma"] += 1
        elif mn.startswith(("buffer_load", "global_load")):
            st["global_load"] += 1
        elif mn.startswith("ds_read") or mn.startswith("ds_load"):
            st["ds_read"] += 1
        elif mn.startswith("ds_write") or mn.startswith("ds_store"):
            st["ds_write"] += 1
        elif mn == "s_barrier":
            st["barrier"] += 1
        elif mn.startswith("scratch_"):
            st["scratch"] += 1
        elif mn == "s_waitcnt" and re.search(r"vmcnt\(0\)", ops):
            st["vmcnt0"] += 1
            if mf and mf[0] < j < mf[-1]:
                st["vmcnt0_inside"] += 1
    return st


def main_loop(ins):
    """the steady-state loop: among the INNERMOST loops that hold MFMAs (a loop that encloses another MFMA loop -- a tile / group walk --
    is not one) -- those that also issue LDS-DMA, if any -- the one with the most MFMAs, shortest body first"""
    spans = [(lo, hi, loop_stats(ins, lo, hi)) for lo, hi in loops(ins)]
    spans = [sp for sp in spans if sp[2]["mfma"] > 0]
    inner = [sp for sp in spans if not any((o[0] >= sp[0] and o[1] <= sp[1] and (o[0], o[1]) != (sp[0], sp[1])) for o in spans)]
    cands = [sp[2] for sp in inner]
    if any(c["lds_dma"] for c in cands):
        cands = [c for c in cands if c["lds_dma"]]
    if not cands:
        return None
    top = max(c["mfma"] for c in cands)
    return min((c for c in cands if c["mfma"] == top), key=lambda c: c["instructions"])


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def analyse(lib_path=None):
    """{demangled kernel name: dict(metadata..., loop=dict(...) or None, mfma_total=...)} for every kernel of the library"""
    lib_path = lib_path or os.path.join(ROOT, "moca_video_amd", "libmoca_hip.so")
    res = {}
    with tempfile.TemporaryDirectory() as wd:
        for co in code_objects(lib_path, wd):
            md, fn = metadata(co), disassemble(co)
            dm = demangle(list(md))
            for name, info in md.items():
                ins = fn.get(name)
                if ins is None:
                    continue
                d = dict(info)
                d["mfma_total"] = sum(1 for _, mn, _ in ins if mn.startswith("v_mfma"))
                d["instructions_total"] = len(ins)
                d["scratch"] = sum(1 for _, mn, _ in ins if mn.startswith("scratch_"))
                d["loop"] = main_loop(ins)
                d["strip_loop"] = strip_loop(ins) if "gemm_ws_kernel" in name else None
                short = re.sub(r"\(anonymous namespace\)::", "", dm[name])
                short = re.sub(r"^void ", "", short)
                short = re.sub(r"\(.*\)$", "", short)
                res[short] = d
    return res


def kernel_owners(lib_path=None):
    """{mangled kernel name: number of gfx950 code objects (= translation units) of the library that define it}.  analyse() and
    encodings() key by name, so a kernel instantiated in two units would silently merge there."""
    lib_path = lib_path or os.path.join(ROOT, "moca_video_amd", "libmoca_hip.so")
    owners = {}
    with tempfile.TemporaryDirectory() as wd:
        for co in code_objects(lib_path, wd):
            for name in metadata(co):
                owners[name] = owners.get(name, 0) + 1
    return owners


_ENC = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*[0-9A-Fa-f]+:((?:\s+[0-9A-Fa-f]{8})+)\s*$")
_PAD = {"00000000", "BF800000", "BF9F0000"}            # zero fill, s_nop 0, s_code_end
_FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
            "private_segment_fixed_size")


def encodings(path):
    """({symbol: [(mnemonic, encoding words)] without trailing padding}, {kernel: register / LDS / scratch figures}) of every gfx950
    code object inside `path`"""
    syms, figs = {}, {}
    with tempfile.TemporaryDirectory() as wd:
        for co in code_objects(path, wd):
            for name, info in metadata(co).items():
                figs[name] = {k: info.get(k, 0) for k in _FIGURES}
            out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
            cur = None
            for line in out.splitlines():
                m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
                if m:
                    cur = syms.setdefault(m.group(1), [])
                    continue
                m = _ENC.match(line)
                if m and cur is not None:
                    cur.append((m.group(1), tuple(w.upper() for w in m.group(3).split())))
    for ins in syms.values():
        while ins and all(w in _PAD for w in ins[-1][1]):
            ins.pop()
    return syms, figs


def diff(old, new):
    """compare two builds kernel by kernel; returns the number of differences that a host-only change cannot explain"""
    (so, fo), (sn, fn) = encodings(old), encodings(new)
    bad = 0
    for name in sorted(set(so) ^ set(sn)):
        print(f"only in {'OLD' if name in so else 'NEW'}: {name}")
        bad += 1
    literals = touched = 0
    for name in sorted(set(so) & set(sn)):
        a, b = so[name], sn[name]
        if len(a) != len(b):
            print(f"{name}: {len(a)} instructions -> {len(b)}")
            bad += 1
            continue
        lit = 0
        for i, ((ma, ea), (mb, eb)) in enumerate(zip(a, b)):
            if ea == eb:
                continue
            if ma == mb == "s_add_u32" and len(ea) == len(eb) == 2 and ea[0] == eb[0]:
                lit += 1                               # the same instruction with another 32-bit literal: a pc-relative symbol offset
            else:
                print(f"{name}: instruction {i}: {ma} {' '.join(ea)} -> {mb} {' '.join(eb)}")
                bad += 1
        literals += lit
        touched += lit > 0
        if fo.get(name) != fn.get(name):
            print(f"{name}: figures {fo.get(name)} -> {fn.get(name)}")
            bad += 1
    print(f"{len(set(so) & set(sn))} symbols in both ({len(fo)} kernels with metadata), {touched} differ in {literals} s_add_u32 literals, "
          f"{bad} other differences")
    return bad


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--diff":
        sys.exit(1 if diff(args[1], args[2]) else 0)
    lib = args.pop(0) if args and args[0].endswith(".so") else None
    r = analyse(lib)
    print(f"{'kernel':46s} vgpr agpr sgpr spill | main loop: ins mfma dma dsrd barr vmcnt0(inside MFMA span) | mfma total")
    for k in sorted(r):
        if args and not any(a in k for a in args):
            continue
        d, lp = r[k], r[k]["loop"]
        ls = "-" if lp is None else f"{lp['instructions']:5d} {lp['mfma']:4d} {lp['lds_dma']:3d} {lp['ds_read']:4d} {lp['barrier']:4d} {lp['vmcnt0']:3d} ({lp['vmcnt0_inside']})"
        print(f"{k:46s} {d.get('vgpr_count', 0):4d} {d.get('agpr_count', 0):4d} {d.get('sgpr_count', 0):4d} "
              f"{d.get('vgpr_spill_count', 0) + d.get('sgpr_spill_count', 0):5d} | {ls} | {d['mfma_total']}")
        for sl in d.get("strip_loop") or []:
            print(f"{'':46s} natural loop: {sl['instructions']} instructions, {sl['mfma']} MFMA, {sl['vm_store']} stores, {sl['vm_atomic']} atomics")
