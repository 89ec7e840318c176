"""GPU: the device-side sampling step -- all of csrc/fifo.hip (the MoCA recurrence of one call's windows, fifo_step_kernel /
mask_sum_kernel, included), the base-sampling step (base_set_timestep_kernel / base_step_kernel / state_bump_kernel) of
csrc/sampler.hip, filter_kernel of csrc/freeinit.hip -- element by element against the restatements of tests/step_kernels_ref.py: at
HW below, at and above a wave and a block, at the ring's wrap (head = Q - 1, windows that straddle the ring end), at iter >= S and
iter >= n_slots, with every optional pointer NULL once, and past the grid cap (4096 blocks of 256 work items: a thread makes a
second trip).

Standard: torch.equal with the fp32 restatement (these translation units are built without contraction: the fp32 torch evaluation in
the reference's order of operations is the expected output bit for bit).  Exceptions: moca_fifo_randn_f32 is held per element to the
measured bound of step_kernels_ref (device logf / sqrtf / sincosf); the Gaussian and Butterworth filters to one fp32 ulp of the
Python-float reference (device and host exp / pow may differ in the last bits of the double, which can move only an fp32 tie).
Every output has sentinel elements behind it; every input a kernel must not write is compared with its copy afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_kernels_ref as R

pytestmark = pytest.mark.gpu

from moca_video_amd import lib as L  # noqa: E402
from moca_video_amd import ops  # noqa: E402

DEV = "cuda"
SENT = -7776.0
TAIL = 64
F32 = torch.float32


@pytest.fixture(autouse=True)
def _stream():
    ops.set_stream(None)
    yield
    torch.cuda.synchronize()


def cases(table):
    return pytest.mark.parametrize("name", list(table))


class Buffers:
    """device copies of a call's operands: outputs live in front of TAIL sentinel elements, inputs keep a host copy"""

    def __init__(self):
        self.full, self.view, self.host = {}, {}, {}

    def inp(self, name, t):
        """an operand the kernel may only read (None stays NULL)"""
        if t is None:
            self.view[name] = None
            return None
        self.host[name] = t.clone()
        return self.out(name, t)

    def out(self, name, t, fill=None):
        """a buffer the kernel writes: shaped like `t`, holding `t` (or `fill`), sentinels behind it"""
        sent = SENT if t.dtype.is_floating_point else -77
        full = torch.full((t.numel() + TAIL,), sent, dtype=t.dtype, device=DEV)
        full[:t.numel()] = t.reshape(-1).to(DEV) if fill is None else fill
        self.full[name], self.view[name] = full, full[:t.numel()].view(t.shape)
        return self.view[name]

    def ptr(self, name, v=None):
        t = self.view.get(name)
        return None if t is None else t.data_ptr()

    def check(self, what):
        """sentinels behind every buffer and every read-only operand unchanged"""
        for name, full in self.full.items():
            n = self.view[name].numel()
            sent = SENT if full.dtype.is_floating_point else -77
            assert bool((full[n:] == sent).all()), f"{what}: elements behind the end of `{name}` were written"
        for name, h in self.host.items():
            exact(self.view[name].cpu(), h, f"{what}: read-only operand `{name}`")


def exact(got, ref, what):
    got = got.cpu() if got.is_cuda else got
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {tuple(got.shape)} {got.dtype} against {tuple(ref.shape)} {ref.dtype}"
    same = (got == ref) | (torch.isnan(got) & torch.isnan(ref)) if got.dtype.is_floating_point else got == ref
    if not bool(same.all()):
        bad = (~same).reshape(-1).nonzero().reshape(-1)
        edge = set(R.edge_items(got.numel()))
        n_edge = sum(int(i) in edge for i in bad[:1000])
        i0 = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ, first at flat index {i0} (got {got.reshape(-1)[i0].item()!r}, "
                             f"ref {ref.reshape(-1)[i0].item()!r}), last at {int(bad[-1])}; {n_edge} of the first {min(bad.numel(), 1000)} are wrap-edge items")


def state_words(head=0, it=0, seed=0, ext=0):
    st = L.FifoState(head, it, seed & 0xffffffff, (seed >> 32) & 0xffffffff, ext)
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.int32).clone()


def launch(entry, b, **scalars):
    args = {a.lstrip("*"): None for a in R.ENTRY[entry]}
    args.update(scalars)
    args["stream"] = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(R.call(L, entry, args, b.ptr), entry)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- moca_fifo_ddim_step_f32
@cases(R.STEP_CASES)
def test_moca_step(name):
    c = R.STEP_CASES[name]
    t = R.step_inputs(c)
    b = Buffers()
    for k_arg, k_in in (("sample", "sample"), ("eps", "eps"), ("noise", "noise"), ("coef", "coef"), ("mask", "mask"), ("cond", "cond"),
                        ("mask_index", "mask_index"), ("enh", "enh")):
        b.inp(k_arg, t[k_in])
    mom = b.out("momentum", t["mom"])
    xp, p0 = b.out("x_prev", t["sample"], SENT), b.out("pred_x0", t["sample"], SENT)
    ws = b.out("ws", torch.zeros(c["Fm"]), SENT) if c["mask"] else None
    launch("moca_fifo_ddim_step_f32", b, B=c["B"], C=c["C"], F=c["F"], Fm=c["Fm"], HW=c["HW"], **R.STEP_ARGS)
    want_xp, want_p0, want_mom = R.step_eval(c, F32, t=t)
    exact(xp, want_xp, f"moca_step {name} x_prev")
    exact(p0, want_p0, f"moca_step {name} pred_x0")
    exact(mom, want_mom, f"moca_step {name} momentum")
    exact(mom[:, :, 0], t["mom"][:, :, 0], f"moca_step {name} momentum frame 0 (never written)")
    if c["mask"]:
        exact(ws, R.mask_batch_sums(t["mask"], F32), f"moca_step {name} batch-wide mask sums (workspace)")
    b.check(f"moca_step {name}")


# ---------------------------------------------------------------------------------------------------------------- moca_sam_select_masks_f32
def run_sam_select(windows, HW, b=None, prefix=""):
    pool, off, cnt, ts = R.sam_pool(windows, HW)
    b = b or Buffers()
    nW, f = len(windows), len(windows[0][1])
    for k, v in (("cand", pool), ("cand_off", off), ("ncand", cnt), ("t_rows", ts)):
        b.inp(prefix + k, v)
    eff = b.out(prefix + "eff", torch.zeros(nW, f, HW), R.SAM_SENTINEL)
    idx = b.out(prefix + "eff_idx", torch.zeros(nW, f, dtype=torch.int32), 99)
    bb = Buffers()
    bb.view = {k[len(prefix):]: v for k, v in b.view.items() if k.startswith(prefix)}
    launch("moca_sam_select_masks_f32", bb, nW=nW, f=f, HW=HW)
    return b, eff, idx


@pytest.mark.parametrize("HW", [1, 65, 260])
def test_sam_select_scripted(HW):
    """the scripted windows of step_kernels_ref.SAM_SCRIPTS, all windows of one HW in one launch (one block per window); rows of
    frames without injection stay at their sentinel"""
    names = [n for n, (hw, _) in R.SAM_SCRIPTS.items() if hw == HW]
    windows = [R.sam_script(n)[1:] for n in names]
    b, eff, idx = run_sam_select(windows, HW)
    for w, n in enumerate(names):
        want_eff, want_idx = R.sam_select(*windows[w], HW)
        exact(idx[w], torch.from_numpy(want_idx), f"sam_select {n} frame flags")
        exact(eff[w], want_eff, f"sam_select {n} effective masks")
    b.check(f"sam_select hw{HW}")


# ---------------------------------------------------------------------------------------------------------------- moca_fifo_step_windows_f32
@cases(R.WIN_CASES)
def test_step_windows(name):
    c = R.WIN_CASES[name]
    t = R.win_inputs(c)
    nW, f, HW, Cc, Q = len(c["starts"]), c["f"], c["HW"], c["C"], c["Q"]
    b = Buffers()
    b.inp("state", state_words(c["head"], 3, 11, 1))
    for k_arg, k_in in (("x", "x"), ("eps_c", "e_c"), ("eps_u", "e_u"), ("noise", "noise"), ("coef", "coef"), ("cond", "cond"), ("enh", "enh"),
                        ("mask", "mask"), ("mask_sums", "mask_sums"), ("mask_frame", "mask_frame")):
        b.inp(k_arg, t[k_in])
    b.inp("win_start", torch.tensor(c["starts"], dtype=torch.int32))
    if c["branch"] == "seg":                                 # fed by the selection kernel's own output, -1 frames (sentinel rows) included
        wins = R.sam_windows_for(nW, f, HW, c["seed"] + 500)
        _, eff, idx = run_sam_select(wins, HW, b, prefix="sel_")
        exact(eff, t["sam_eff"], f"step_windows {name}: selection kernel masks")
        exact(idx, t["sam_idx"], f"step_windows {name}: selection kernel flags")
        assert bool((t["sam_idx"] < 0).any()) and bool((eff.cpu()[t["sam_idx"] < 0] == R.SAM_SENTINEL).all())
        b.view["sam_eff"], b.view["sam_idx"] = eff, idx
        b.host["sel_eff"], b.host["sel_eff_idx"] = t["sam_eff"].clone(), t["sam_idx"].clone()
    mom = b.out("momentum", t["mom"])
    queue = b.out("queue", t["queue"]) if c["queue"] else None
    xp = b.out("x_prev", t["x"], SENT) if c["x_prev"] else None
    p0 = b.out("pred_x0", t["x"], SENT) if c["pred_x0"] else None
    launch("moca_fifo_step_windows_f32", b, nW=nW, C=Cc, Q=Q if c["queue"] or c["branch"] == "mask" else 0, f=f, HW=HW, wb_from=c["wb_from"], **R.WIN_ARGS)
    want = R.win_eval(c, F32, t=t)
    for key, got in (("x_prev", xp), ("pred_x0", p0), ("mom", mom), ("queue", queue)):
        if got is not None:
            exact(got, want[key], f"step_windows {name} {key}")
    exact(mom[:, :, 0], t["mom"][:, :, 0], f"step_windows {name} momentum frame 0 (never written)")
    if queue is not None:                                    # queue frames outside the write-back set keep their values
        lin, lin0 = R.from_ring(queue.cpu(), c["head"], 1), t["queue_lin"]
        wb = {s0 + j for s0 in c["starts"] for j in range(c["wb_from"], f)}
        keep = [j for j in range(Q) if j not in wb]
        exact(lin[:, keep], lin0[:, keep], f"step_windows {name}: queue frames outside the write-back set")
    b.check(f"step_windows {name}")


# ---------------------------------------------------------------------------------------------------------------- moca_fifo_gather_windows_f32
@cases(R.GATHER_CASES)
def test_gather_windows(name):
    c = R.GATHER_CASES[name]
    q, want_x, want_a = R.gather_eval(c)
    nW = len(c["starts"])
    b = Buffers()
    b.inp("state", state_words(c["head"], 5, 11, 1))
    b.inp("queue", q)
    b.inp("win_start", torch.tensor(c["starts"], dtype=torch.int32) if c["x"] else None)
    x = b.out("x", want_x, SENT) if c["x"] else None
    a = b.out("anchor", want_a, SENT) if c["anchor"] else None
    launch("moca_fifo_gather_windows_f32", b, nW=nW, reps=c["reps"], C=c["C"], Q=c["Q"], f=c["f"], HW=c["HW"])
    if c["x"]:
        exact(x, want_x, f"gather_windows {name} x")
    if c["anchor"]:
        exact(a, want_a, f"gather_windows {name} anchor")
    b.check(f"gather_windows {name}")


# ---------------------------------------------------------------------------------------------------------------- moca_fifo_advance_f32
@cases(R.ADV_CASES)
def test_advance(name):
    c = R.ADV_CASES[name]
    t = R.adv_inputs(c)
    b = Buffers()
    st = b.out("state", state_words(c["head"], c["iter"], 0x1234567_89abcdef, 1))
    queue = b.out("queue", t["queue"])
    emitted = b.out("emitted", t["emitted"]) if c["emitted"] else None
    mask = b.out("mask", t["mask"]) if c["mask"] else None
    sums = b.out("mask_sums", t["mask_sums"]) if c["mask"] else None
    scal = dict(n_slots=c["n_slots"] if c["emitted"] else 0, emit_frame=c["emit_frame"], C=c["C"], Q=c["Q"], HW=c["HW"])
    want = R.adv_eval(c, t=t)
    for call, key in enumerate(("newframe", "newframe2")):   # two calls in a row: the second sees the bumped state
        b.inp("newframe", t[key])
        launch("moca_fifo_advance_f32", b, **scal)
        (head, it, ext), w_q, w_e, w_m, w_s = want[call]
        what = f"advance {name} call {call + 1}"
        exact(st, torch.tensor([head, it, 0x89abcdef - (1 << 32), 0x1234567, ext, 0, 0, 0], dtype=torch.int32), what + " state (head, iter, seed untouched, ext_noise 0)")
        exact(queue, w_q, what + " queue")
        if c["emitted"]:
            exact(emitted, w_e, what + " emitted (the other slots keep their values)")
        if c["mask"]:
            exact(mask, w_m, what + " mask ring")
            exact(sums, w_s, what + " mask sums")
        b.check(what)


# ---------------------------------------------------------------------------------------------------------------- moca_fifo_prepare_queue_f32
@cases(R.PREP_CASES)
def test_prepare_queue(name):
    c = R.PREP_CASES[name]
    t = R.prep_inputs(c)
    b = Buffers()
    for k_arg, k_in in (("z", "z"), ("noise", "noise"), ("coef_z", "ca"), ("coef_noise", "cb"), ("frame_idx", "fidx")):
        b.inp(k_arg, t[k_in])
    out = b.out("queue", t["noise"], SENT)
    launch("moca_fifo_prepare_queue_f32", b, BC=c["BC"], Tz=c["Tz"], Q=c["Q"], HW=c["HW"])
    exact(out, R.prep_eval(c, F32, t=t), f"prepare_queue {name}")
    b.check(f"prepare_queue {name}")


# ---------------------------------------------------------------------------------------------------------------- base sampling
@cases(R.BASE_CASES)
def test_base_step(name):
    c = R.BASE_CASES[name]
    t = R.base_inputs(c)
    b = Buffers()
    st = b.out("state", state_words(7, c["iter"], 0x1234567_89abcdef, 1))
    for k_arg, k_in in (("eps_c", "e_c"), ("eps_u", "e_u"), ("noise", "noise"), ("coef", "coef")):
        b.inp(k_arg, t[k_in])
    x = b.out("x", t["x"])
    p0 = b.out("pred_x0", t["x"], SENT) if c["pred_x0"] else None
    launch("moca_base_ddim_step_f32", b, S=c["S"], cfg_scale=R.BASE_CFG, use_scale=c["use_scale"], n=c["n"])
    want_xp, want_p0 = R.base_eval(c, F32, t=t)
    exact(x, want_xp, f"base_step {name} x (in place)")
    if c["pred_x0"]:
        exact(p0, want_p0, f"base_step {name} pred_x0")
    exact(st, torch.tensor([7, c["iter"] + 1, 0x89abcdef - (1 << 32), 0x1234567, 0, 0, 0, 0], dtype=torch.int32), f"base_step {name} state (iter + 1, ext_noise 0, head and seed untouched)")
    b.check(f"base_step {name}")


@cases(R.TIMESTEP_ROW_CASES)
def test_base_set_timestep(name):
    c = R.TIMESTEP_ROW_CASES[name]
    table = R.timestep_table(c["S"])
    b = Buffers()
    b.inp("state", state_words(7, c["iter"], 5, 1))
    b.inp("table", table)
    rows = b.out("rows", torch.zeros(c["n"], dtype=torch.int64), -5)
    launch("moca_base_set_timestep", b, S=c["S"], n=c["n"])
    exact(rows, table[R.schedule_row(c["iter"], c["S"])].expand(c["n"]).contiguous(), f"set_timestep {name}")
    b.check(f"set_timestep {name}")


# ---------------------------------------------------------------------------------------------------------------- moca_mask_frame_sums_f32
@pytest.mark.parametrize("HW", R.HWS)
def test_mask_frame_sums(HW):
    m = R.sums_inputs(HW, 6000 + HW)
    b = Buffers()
    b.inp("mask", m)
    sums = b.out("sums", torch.zeros(m.shape[0]), SENT)
    launch("moca_mask_frame_sums_f32", b, frames=m.shape[0], HW=HW)
    want = R.mask_frame_sums(m, F32)
    assert want[1] == 0 and want[2] == 0.75
    exact(sums, want, f"mask_frame_sums hw{HW}")
    b.check(f"mask_frame_sums hw{HW}")


# ---------------------------------------------------------------------------------------------------------------- moca_fifo_randn_f32
_randn_worst = {}


@cases(R.RANDN_CASES)
def test_randn(name):
    """per element against the float64 evaluation of the same fp32 uniforms and fp32 angle, within RANDN_BOUND (2^-23 |ref| + 2^-24 r);
    the project's 2e-4 against the plain float64 evaluation as the outer ceiling; two iterations and two seed halves: four streams"""
    n = R.RANDN_CASES[name]
    seeds = [(R.RANDN_SEED, 0), (R.RANDN_SEED, 5)] + ([(R.RANDN_SEED ^ 1, 0), (R.RANDN_SEED ^ (1 << 32), 0)] if n <= 1023 else [])
    outs = []
    for seed, it in seeds:
        b = Buffers()
        b.inp("state", state_words(3, it, seed, 0))
        out = b.out("out", torch.zeros(n), SENT)
        launch("moca_fifo_randn_f32", b, n=n)
        got = out.cpu().numpy()
        ref, r = R.philox_numpy(seed, it, n, f32_angle=True, with_r=True)
        ratio = R.randn_ratio(got, ref, r)
        w = float(ratio.max())
        _randn_worst[name] = max(_randn_worst.get(name, 0.0), w)
        print(f"[step] randn {name} seed {seed:#x} iter {it}: worst |err| / (2^-23 |ref| + 2^-24 r) = {w:.3f} (bound {R.RANDN_BOUND}); so far {max(_randn_worst.values()):.3f}")
        i = int(ratio.argmax())
        assert w <= R.RANDN_BOUND, f"randn {name}: {int((ratio > R.RANDN_BOUND).sum())} of {n} elements outside the bound, worst {w:.2f} at flat index {i} (got {got[i]!r}, ref {ref[i]!r})"
        assert np.abs(got.astype(np.float64) - R.philox_numpy(seed, it, n)).max() < R.RANDN_CEILING
        b.check(f"randn {name}")
        outs.append(got)
    for i in range(len(outs)):
        for j in range(i):
            assert not np.array_equal(outs[i], outs[j]), "two iterations / seed halves gave the same stream"
    b = Buffers()                                            # ext_noise: the host filled the buffer, the kernel leaves it alone
    b.inp("state", state_words(3, 0, R.RANDN_SEED, 1))
    out = b.out("out", torch.zeros(n), 7.0)
    launch("moca_fifo_randn_f32", b, n=n)
    assert bool((out == 7.0).all())
    b.check(f"randn {name} ext_noise")


# ---------------------------------------------------------------------------------------------------------------- moca_freq_filter_f32
@cases(R.FILTER_CASES)
def test_freq_filter(name):
    c = R.FILTER_CASES[name]
    T, H, W = c["shape"]
    b = Buffers()
    lpf = b.out("lpf", torch.zeros(T, H, W), SENT)
    launch("moca_freq_filter_f32", b, T=T, H=H, W=W, type=R.FILTER_TYPES[c["kind"]], n=c["n"], d_s=c["d_s"], d_t=c["d_t"])
    want = R.filter_eval(c)
    if c["kind"] in ("box", "ideal") or c["d_s"] == 0 or c["d_t"] == 0:
        exact(lpf, want, f"freq_filter {name}")
    else:
        got = lpf.cpu()
        lo, hi = torch.nextafter(want, torch.full_like(want, -1.0)), torch.nextafter(want, torch.full_like(want, 2.0))
        bad = ((got < lo) | (got > hi) | torch.isnan(got)).reshape(-1).nonzero().reshape(-1)
        print(f"[step] freq_filter {name}: {int((got != want).sum())} of {got.numel()} elements one fp32 ulp from the Python-float reference")
        assert bad.numel() == 0, f"freq_filter {name}: {bad.numel()} elements more than one fp32 ulp off, first at flat index {int(bad[0])}, last at {int(bad[-1])}"
    b.check(f"freq_filter {name}")


# ---------------------------------------------------------------------------------------------------------------- accepted argument sets
@cases(R.REFUSALS)
def test_accepted_argument_sets(name):
    """the argument sets the CPU refusals are variations of: launched on zero-filled buffers, accepted, nothing behind the buffers touched"""
    ok, _ = R.REFUSALS[name]
    for over in [{}] + R.ACCEPTED_ALSO.get(name, []):
        args = dict(ok, **over)
        b = Buffers()
        for a in R.ENTRY[name]:
            if a.startswith("*") and args[a[1:]] is not None:
                b.out(a[1:], torch.zeros(16384, dtype=torch.int32), 0)
        launch(name, b, **{k: v for k, v in args.items() if "*" + k not in R.ENTRY[name]})
        b.check(f"{name} accepted {over}")
