"""Recorded forward of the MI355X UNet: walks the reference-shaped module tree ONCE per
input signature, allocates every intermediate from a pool and records the launch
sequence (C-ABI calls with bound device pointers).  Replays are a single hipGraph launch.

Data layout in HBM: every activation is a row-major [B*T*H*W][C] fp16 matrix
(channels-last, frame outermost).  Spatial ops see contiguous channels per pixel; the
temporal conv / temporal attention reach the other frames of a pixel with a constant
row stride of H*W, so the reference's `(b t) c h w <-> b c t h w <-> (b h w) t c`
rearranges (openaimodel3d.py:43-45,231-233; attention.py:268,275,335-338,352,367) do
not exist here.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
import warnings

import torch

from . import lib as _l
from . import ops
from .unet import (IMAGE_CONTEXT_MAX, TEXT_CONTEXT_LEN, _BasicTransformerBlock, _CatMap, _Downsample, _FMap, _Pool, _ResBlock,
                   _SpatialTransformer, _TemporalTransformer, _Upsample)

N_CU = 256


def gemm_splits(M, pw):
    """split-K factor: only when the launch cannot give every CU a tile (mirrors the tile choice of moca_gemm_f16)."""
    nk = pw.w.shape[1] // 64
    tiles = 0
    if pw.N % 160 == 0 and not pw.geglu and M > 160:        # w80 kernel: 320 x 160 tiles when they fill the chip
        tiles = ((M + 319) // 320) * (pw.N // 160)
        if tiles < 200:
            tiles = 0
    if tiles == 0:
        if M > 128 and (pw.N % 128 == 0 or pw.N % 160 == 0):
            tm, bn = 256, (128 if pw.N % 128 == 0 else 160)
        else:
            tm, bn = 128, (128 if pw.N % 128 == 0 else 64)
        tiles = ((M + tm - 1) // tm) * (pw.N // bn)
    if tiles >= (N_CU * 3) // 4:
        return 1
    cap = N_CU // tiles
    if tiles >= 40:
        # measured at M = N = 1280 (50 tiles, tools/bench_l3.py): K = 1280 runs 17.9 us unsplit against 22-25 us with any split
        # (the slabs and the reduce launch cost more than the idle CUs); K = 2560..5120 is best at 4 splits (one round of 200
        # blocks, 20 % less slab traffic than 5); only the 3x3 convs (K >= 11520) want every CU
        if nk <= 24:
            return 1
        if nk <= 100:
            return max(1, min(cap, 4))
    return max(1, min(cap, nk // 8))


# weight prefetch (moca_gemm_params.prefetch): weights of a launch worth warming the memory-side cache for, and the least work a host
# launch must have so that its spare blocks finish before its tiles do (same-box A/B: profiles/r04_ab_weight_prefetch_in_kernel.txt;
# the environment variables exist for such A/B runs only)
PREFETCH_MIN_BYTES = int(float(os.environ.get("MOCA_PREFETCH_MIN_MB", "4")) * (1 << 20))
PREFETCH_HOST_FLOP = float(os.environ.get("MOCA_PREFETCH_HOST_GF", "50")) * 1e9
# virtual torch.cat in the output blocks (A/B switch: MOCA_VCAT=0 materialises every concat as before round 5)
VIRTUAL_CAT = os.environ.get("MOCA_VCAT", "1") != "0"
# split-K reduce inside the GroupNorm that consumes it (the 5 x 8-latent level of the B = 2 forward; A/B switch MOCA_SKGN=0)
SPLITK_GN = os.environ.get("MOCA_SKGN", "1") != "0"
# GroupNorm of a transformer entry folded into its proj_in as per-statistics-group weights (moca_groupnorm_fold_weights_f16 +
# moca_gemm_params.wgroup_rows): the normalised tensor is never written.  MOCA_GNFOLD=0: A/B
GN_FOLD = os.environ.get("MOCA_GNFOLD", "1") != "0"
SPLITK_GN_ALL = os.environ.get("MOCA_SKGN", "1") == "2"     # (A/B: also the 16-frame GroupNorms of the temporal convs)
# frames of one temporal-attention problem: T <= 16 one 16 x 16 MFMA tile (moca_temporal_attention_f16 / _causal_f16 and the fused
# MOCA_EP_TATTN launch), 17 .. 32 one 32 x 32 tile (moca_temporal_attention_long_f16)
MAX_FRAMES = 32
# MOCA_EP_GSTAT: a (statistics group, channel group) accumulator takes fewer than 2^11 partials of <= 2^53 units each, so it cannot
# wrap past 2^64 (csrc/common.h).  Its producer is a tiled GEMM with row tiles of >= 160 rows, and a channel group (<= 80 columns)
# lies in at most two of its column tiles (>= 128 columns): 2 * ceil(rows / 160) partials.  Checked for the statistics groups of MORE THAN 16
# FRAMES (the 5-D GroupNorms of a T > 16 forward: the shapes that were refused before); every plan of up to 16 frames is built as before
GSTAT_MAX_PARTIALS = (1 << 11) - 1


def _check_gstat_range(rows):
    if 2 * -(-rows // 160) > GSTAT_MAX_PARTIALS:
        raise ValueError(f"GroupNorm statistics over {rows} rows (frames x pixels of one group) are outside the range of the fixed-point "
                         f"accumulators: at most {GSTAT_MAX_PARTIALS // 2 * 160} rows, e.g. 32 frames of 5115 latent pixels")


class _LNRef:
    """a LayerNorm that exists only as statistics: x (fp16 [M][C]) + the row partial sums its producer left behind
    (f32 [nparts][M][2]); consumed by a MOCA_EP_LNFOLD GEMM"""
    __slots__ = ("x", "part", "nparts")

    def __init__(self, x, part, nparts):
        self.x, self.part, self.nparts = x, part, nparts


class _PlanBase:
    """pool + recorded launch list + hipGraph capture/replay, shared by the UNet plan and the VAE-decoder plan"""
    _defer_slabs = False     # (UNet plan only: every feature map it creates reaches gn() or _retire(), which release the deferred workspace)

    def __init__(self, model, device):
        self.model = model
        self.device = device
        self.P = model._packed
        self.pool = _Pool(device)
        # (a plan recorded on a host device -- the CPU tests read its launch list -- is never launched and has no stream)
        self.stream = torch.cuda.Stream(device=device) if torch.device(device).type == "cuda" else None
        self.steps = []
        self._pinned = set()
        self.graph = None
        self.graph_failed = False
        self.n_runs = 0
        self._gstat_buf, self._gstat_used, self._last_gemm_step = None, 0, None
        self._held = {}          # data_ptr -> [pending deferred reduces that read it, buffer released meanwhile]
        self._gstat_full = []
        self.reps = 1            # > 1: the batch is `reps` context variants of the same Bx latents (_Plan: shared prefix)
        self._prefetch_at = {}   # during the build: index of a recorded GEMM step -> weights of later launches to prefetch in front of it
        self.prefetch_on = getattr(model, "weight_prefetch", True)

    def _note_gemm(self, pw):
        """called right before a GEMM step is recorded: weight-heavy -> its weights ride on the PREVIOUS GEMM launch (moca_gemm_params.prefetch:
        spare blocks of that launch's grid stream them into the Infinity Cache while its tiles compute; the small launches in between do
        not matter)"""
        if self._last_gemm_step is not None and not pw.derived and pw.w.numel() * pw.w.element_size() >= PREFETCH_MIN_BYTES:
            self._prefetch_at.setdefault(self._last_gemm_step, []).append(pw.w)
        self._last_gemm_step = len(self.steps)

    def _finish_prefetch(self):
        """end of the build (every re-targeting of recorded steps is done): the host launches get their `prefetch` operand (one per
        launch: the largest of the weights that asked for it)"""
        if self.prefetch_on:
            for j, ws in self._prefetch_at.items():
                host = self.steps[j]
                # the spare blocks must be done before the host's tiles are, or they prolong it: only hosts with enough work
                if 2.0 * host.keywords["M"] * host.args[1].N * host.args[1].K >= PREFETCH_HOST_FLOP:
                    self._retarget(j, prefetch=max(ws, key=lambda w: w.numel()))
        self._prefetch_at = {}

    def close(self):
        """release the instantiated hipGraph (moca_graph_destroy); the plan falls back to eager launches if used again"""
        if self.graph is not None:
            g, self.graph = self.graph, None
            try:
                torch.cuda.synchronize(self.device)
                _l.load().moca_graph_destroy(g)
            except Exception:
                pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ emit helpers
    def _emit(self, fn, *args, **kw):
        self.steps.append(functools.partial(fn, *args, **kw))

    def _retarget(self, i, **changes):
        """re-record launch `i` with some keywords replaced: the ONE place a recorded step is rewritten (a producer that takes on,
        or is relieved of, what it leaves behind for its consumer; the prefetch operand).  Returns the step as it was."""
        prod = self.steps[i]
        self.steps[i] = functools.partial(prod.func, *prod.args, **{**prod.keywords, **changes})
        return prod

    def _release(self, *bufs):
        for b in bufs:
            if b is None:
                continue
            if b.data_ptr() in self._pinned:
                continue
            held = self._held.get(b.data_ptr())
            if held is not None:               # an operand a deferred split-K reduce still has to read (see _gemm): back to the pool
                held[1] = b                    # only once the consumer that performs the reduce has been recorded (_unhold)
                continue
            self.pool.put(b)

    def _unhold(self, slabs):
        """the deferred reduce of `slabs` has been recorded (or dropped): operands released meanwhile go back to the pool NOW, i.e.
        after the fused GroupNorm took its output buffer -- it can never be handed one of the operands it re-reads"""
        for ptr in slabs[2]:
            held = self._held.get(ptr)
            if held is None:
                continue
            held[0] -= 1
            if held[0] == 0:
                del self._held[ptr]
                if held[1] is not None:
                    self.pool.put(held[1])

    def _splits(self, M, pw):
        return gemm_splits(M, pw)

    def _gemm(self, a, pw, M, *, out_cols=None, want_colsum=False, **kw):
        """returns `out`, or `(out, colsum, slabs)` with want_colsum (the two promises of _FMap, see _gemm_map):
        colsum = (f32 [row tiles][N][2], rows per tile) when this launch can leave the GroupNorm statistics of its output behind
        (moca_gemm_colsum_rows), else None; slabs = the split-K workspace whose reduce may still move into the consumer, else None"""
        n_out = pw.n_out if pw.geglu else pw.N
        out = self.pool.get(M, n_out)
        splits = self._splits(M, pw)
        ws = None
        if splits > 1:
            ws = self.pool.get(splits * M, pw.N, torch.float32)
        cs = None
        if want_colsum:
            rows = ops.gemm_colsum_rows(a, pw, M=M, splits=splits, **kw)
            if rows > 0:
                cs = (self.pool.get((M + rows - 1) // rows, 2 * pw.N, torch.float32), rows)
        self._note_gemm(pw)
        self._emit(ops.gemm, a, pw, out, M=M, splits=splits, splitk_ws=ws, colsum=None if cs is None else cs[0], **kw)
        slabs = None
        if ws is not None:
            if want_colsum and SPLITK_GN and self._defer_slabs:   # the workspace stays reserved until the consumer is known
                ptrs = []                                       # ... and so do the operands a fused reduce re-reads there
                for t in (kw.get("residual"), kw.get("rowadd")):
                    if t is not None and t.data_ptr() not in self._pinned:
                        self._held.setdefault(t.data_ptr(), [0, None])[0] += 1
                        ptrs.append(t.data_ptr())
                slabs = (ws, self._last_gemm_step, tuple(ptrs))   # (_FMap.slabs; released by gn() / _drop_colsum())
            else:
                self.pool.put(ws)
        return (out, cs, slabs) if want_colsum else out

    def _gemm_map(self, F, H, W, a, pw, **kw):
        """a GEMM whose output is a feature map [F*H*W][pw.N]: the map is made HERE with everything its producer promised -- per-tile
        column sums (with the index of the launch, so that a consumer can re-target it) and / or the deferred split-K workspace"""
        out, cs, slabs = self._gemm(a, pw, F * H * W, want_colsum=True, **kw)
        o = _FMap(out, F, H, W, pw.N, cs, src=self._last_gemm_step if cs is not None else None)
        o.slabs = slabs
        return o

    def linear(self, a, M, pw, residual=None, lda=None):
        return self._gemm(a, pw, M, lda=lda if lda is not None else a.stride(-2), residual=residual)

    def conv(self, fm, pw, *, stride=1, up=0, rowadd=None, rowadd_div=1, residual=None):
        """3x3 conv; the output carries its GroupNorm statistics when the launch can produce them"""
        if up:
            oH, oW = fm.H * 2, fm.W * 2
        elif stride == 2:
            oH, oW = (fm.H - 1) // 2 + 1, (fm.W - 1) // 2 + 1
        else:
            oH, oW = fm.H, fm.W
        return self._gemm_map(fm.F, oH, oW, fm.buf, pw, mode=_l.MOCA_A_CONV3X3, conv=(fm.C, fm.H, fm.W, oH, oW, stride, up),
                              rowadd=rowadd, rowadd_div=rowadd_div, residual=residual)

    def upconv(self, fm, conv):
        """`Upsample` (openaimodel3d.py:96-106: nearest x2, then conv3x3).  With enough low-resolution rows to fill the chip per
        launch: four 2 x 2 convs on the low-resolution grid, one per output parity, each writing its quarter of the pixels (4/9 of
        the FLOPs: the 3x3 taps that read the same input pixel are summed at pack time).  Otherwise the 3x3 conv whose gather
        reads in[y // 2][x // 2]."""
        phases = self.P.get(("up_phases", id(conv)))
        M = fm.F * fm.H * fm.W
        if phases is None or M < 5120 or self._splits(M, phases[0]) != 1:       # (below: split-k per phase costs more than it saves)
            return self.conv(fm, self.P[id(conv)], up=1)
        out = self.pool.get(4 * M, phases[0].N)
        kw = dict(M=M, mode=_l.MOCA_A_CONV3X3, conv=(fm.C, fm.H, fm.W, fm.H, fm.W, 1, 0), splits=1)
        idx = []
        for ph, pw in enumerate(phases):
            self._note_gemm(pw)
            idx.append(len(self.steps))
            self._emit(ops.gemm, fm.buf, pw, out, up_phase=ph + 1, **kw)
        up = _FMap(out, fm.F, fm.H * 2, fm.W * 2, phases[0].N, None)
        # the four launches can leave GroupNorm statistics of the upsampled map behind (a consumer that is a virtual concat re-targets
        # them): a row tile of the LOW-resolution grid lies inside one frame
        up.cs_rows = ops.gemm_colsum_rows(fm.buf, phases[0], **kw)
        if up.cs_rows > 0:
            up.src = tuple(idx)
        return up

    def tconv(self, fm, pw, residual=None):
        return self._gemm_map(fm.F, fm.H, fm.W, fm.buf, pw, mode=_l.MOCA_A_TCONV3, tconv=(fm.C, self.T, fm.H * fm.W), residual=residual)

    def gn(self, fm, gb, *, fps, eps, silu, x_dead=False):
        """GroupNorm(32) (+SiLU), cashing in whatever the producer of `fm` promised (_FMap): a deferred split-K reduce moves into this
        launch; finished statistics (accumulated by a concat, or by the producing GEMM once it is re-targeted) leave only the apply
        pass; otherwise the plain statistics + apply launch."""
        if isinstance(fm, _CatMap):                            # the virtual concat: both sources read in place, statistics finished
            y = self.pool.get(fm.M, fm.C)
            self._emit(ops.groupnorm_gstat_cat, fm.h.buf, fm.skip.buf, y, gb[0], gb[1], fm.gcat, fm.gb, F=fm.F, HW=fm.H * fm.W,
                       C1=fm.h.C, C2=fm.skip.C, frames_per_stat=fps, eps=eps, silu=silu, Fb=fm.Fb)
            assert fps == 1
            return y
        HW = fm.H * fm.W
        if fm.slabs is not None:
            # the producer ran split-K: its reduce launch moves into this GroupNorm (x_dead: nobody else reads fm.buf -- it is not written)
            slabs, fm.slabs = fm.slabs, None
            prod = self.steps[slabs[1]]
            kw, y = prod.keywords, None
            # (only per-frame statistics: 1024 slabs fill the chip and the launch beats reduce + GroupNorm by 2.3 us; the 64 slabs of the
            #  16-frame GroupNorms are slower fused, 18.6 against 7.9 + 7.9 us -- profiles/r05_ab_splitk_groupnorm.txt)
            if (fps == 1 or SPLITK_GN_ALL) and ops.gemm_splitk_groupnorm_ok(prod.args[0], prod.args[1], HW=HW, frames_per_stat=fps, **kw):
                y = self.pool.get(fm.M, fm.C)
                self._retarget(slabs[1], slabs=True)
                self._emit(ops.gemm_splitk_groupnorm, prod.args[0], prod.args[1], prod.args[2], y, gb[0], gb[1], HW=HW,
                           frames_per_stat=fps, eps=eps, silu=silu, write_x=not x_dead, **kw, slabs=True)
            self.pool.put(slabs[0])
            self._unhold(slabs)
            if y is not None:
                return y
        y = self.pool.get(fm.M, fm.C)
        ws = self.pool.get(1, ops.groupnorm_ws_floats(fm.F, HW, fm.C), torch.float32)
        if self._stats_ready(fm, fps):
            self._emit(ops.groupnorm_gstat, fm.buf, y, gb[0], gb[1], self._finished_stats(fm, fps), F=fm.F, HW=HW, Cn=fm.C,
                       frames_per_stat=fps, eps=eps, silu=silu)
        else:                                                 # (nothing promised, or row tiles that straddle two statistics groups)
            self._emit(ops.groupnorm, fm.buf, y, gb[0], gb[1], F=fm.F, HW=HW, Cn=fm.C, frames_per_stat=fps,
                       eps=eps, silu=silu, ws=ws)
        self.pool.put(ws)
        return y

    def _stats_ready(self, fm, fps):
        """can `_finished_stats(fm, fps)` deliver?  Either the concat that produced fm accumulated these statistics, or fm's producer left
        per-tile column sums whose row tiles lie inside one statistics group (fps frames): then it can be re-targeted"""
        if fm.gstat is not None and fm.gstat[1] == fps:
            return True
        return fm.colsum is not None and (fps * fm.H * fm.W) % fm.colsum[1] == 0

    def _finished_stats(self, fm, fps):
        """the FINISHED GroupNorm statistics of fm over groups of `fps` frames (call only where _stats_ready): returns the accumulators.
        Where fm still holds per-tile column sums its producer is re-targeted: it accumulates the finished statistics instead
        (fixed-point atomics per (statistics group, channel group), MOCA_EP_GSTAT) -- no finalize launch; the column-sum buffer goes back
        to the pool and the map moves to `gstat_own`"""
        if fm.gstat is not None and fm.gstat[1] == fps:
            return fm.gstat[0]
        rows = fps * fm.H * fm.W
        if fps > 16:                                          # (groups of up to 16 frames, per-frame ones included: as before)
            _check_gstat_range(rows)
        slot = self._gstat_slot((fm.F // fps) * 64)
        self._retarget(fm.src, colsum=None, gstat=(slot, rows))
        self.pool.put(fm.colsum[0])
        fm.colsum = None
        fm.gstat_own = (slot, fps)
        return slot

    def _gstat_slot(self, n_doubles):
        """64-bit fixed-point accumulators of one GEMM -> GroupNorm pair, carved from ONE buffer that a single memset zeroes at the start of
        every run (_run_steps)"""
        if self._gstat_buf is None or self._gstat_used + n_doubles > self._gstat_buf.numel():
            if self._gstat_buf is not None:                # the chunk is full: keep it (its slots are in use), open another one
                self._gstat_full.append(self._gstat_buf[:self._gstat_used])
            self._gstat_buf = torch.zeros(max(1 << 20, n_doubles), dtype=torch.int64, device=self.device)      # 8 MiB chunks
            self._gstat_used = 0
        s = self._gstat_buf[self._gstat_used:self._gstat_used + n_doubles]
        self._gstat_used += n_doubles
        return s

    def _drop_colsum(self, fm):
        """settle what fm's producer still promises once no consumer can take it up any more (the statistics half of _retire; alone only
        where fm's rows are still read: in front of the launch that reuses the freed workspace, or when the rows are about to change)"""
        if fm.slabs is not None:                               # a split-K producer whose consumer was no GroupNorm: its own reduce stays
            self.pool.put(fm.slabs[0])
            self._unhold(fm.slabs)
            fm.slabs = None
        if fm.colsum is not None:                              # nobody read the column sums (the consumer was a conv / a concat / a
            self._retarget(fm.src, colsum=None)                # GroupNorm whose statistics groups the row tiles straddle): the
            self.pool.put(fm.colsum[0])                        # producer goes back to the plain store loop
            fm.colsum = None

    def _retire(self, fm):
        """`fm` is consumed -- every launch that reads it has been recorded: its buffer goes back to the pool (unless pinned, or held
        for a deferred reduce) and whatever its producer still promised is settled.  A virtual concat retires both of its sources.
        (Settle first: operands held for the reduce re-enter the pool in front of fm's own buffer.  The pool hands out the buffer put
        back last, so the order decides which one the next launch gets; tests/golden/plan_full_launches.npz pins it.)"""
        for m in ((fm.h, fm.skip) if isinstance(fm, _CatMap) else (fm,)):
            self._drop_colsum(m)
            self._release(m.buf)

    def ln(self, x, M, Cn, gb):
        y = self.pool.get(M, Cn)
        self._emit(ops.layernorm, x, y, gb[0], gb[1], M=M, Cn=Cn, eps=1e-5)
        return y

    def _run_steps(self):
        if self._prefetch_at:                  # plans whose build does not end in _finish_prefetch (VAE decoder, single blocks)
            self._finish_prefetch()
        for full in self._gstat_full:
            ops.memset_zero(full)
        if self._gstat_used:
            ops.memset_zero(self._gstat_buf[:self._gstat_used])
        for s in self.steps:
            s()

    @contextlib.contextmanager
    def _enqueue(self, cur=None):
        """`with plan._enqueue(cur):` -- the plan's stream is ordered after `cur` (default: the current stream) and entered: whatever the
        body enqueues (input copies, then `_replay()`) runs on it; the caller joins (`cur.wait_stream(plan.stream)`) when it wants"""
        self.stream.wait_stream(cur if cur is not None else torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            yield

    @contextlib.contextmanager
    def _ops_stream(self):
        """the C-ABI launches of `ops` go to the plan's stream inside, to torch's current stream again afterwards"""
        ops.set_stream(self.stream.cuda_stream)
        try:
            yield
        finally:
            ops.set_stream(None)

    def _replay(self):
        """one run of the recorded sequence on the plan's stream (inside `_enqueue`): the ONE caller of `_launch`, which decides
        eager / capture / replay from the runs counted so far"""
        with self._ops_stream():
            self._launch(self.stream.cuda_stream)
        self.n_runs += 1

    def _launch(self, handle):
        lib = _l.load()
        if self.graph is not None:
            _l.check(lib.moca_graph_launch(self.graph, C.c_void_p(handle)), "moca_graph_launch")
            return
        use_graph = self.model.use_graph and not self.graph_failed
        if self.n_runs == 0 or not use_graph:
            self._run_steps()          # first pass eager: surfaces argument errors outside of capture
            return
        # second pass: record the same launch sequence into a hipGraph, then replay it
        rc = lib.moca_graph_begin(C.c_void_p(handle))
        if rc != 0:
            self.graph_failed = True
            warnings.warn("moca_video_amd: hipStreamBeginCapture failed; staying on eager HIP launches")
            self._run_steps()
            return
        try:
            self._run_steps()
        finally:
            g = C.c_void_p()
            rc = lib.moca_graph_end(C.c_void_p(handle), C.byref(g))
        if rc != 0 or not g.value:
            self.graph_failed = True
            warnings.warn("moca_video_amd: hipGraph instantiate failed; staying on eager HIP launches")
            self._run_steps()
            return
        self.graph = g
        _l.check(lib.moca_graph_launch(self.graph, C.c_void_p(handle)), "moca_graph_launch")


class _Plan(_PlanBase):
    _defer_slabs = True

    def __init__(self, model, B, T, H, W, L, in_dtype, device, shared_x=False, pieces=None, adapter=None):
        """shared_x: the B videos are `len(L)` context variants of the SAME B / len(L) latents (the two `apply_model` calls of
        classifier-free guidance, ddim.py:298-299,366-369, on one x): `x_in` holds the distinct latents only, everything up to the
        first cross-attention (conv_in, init_attn, the first ResBlock, the first SpatialTransformer's self-attention and to_q:
        8 % of the forward) is computed once and repeated where the contexts first enter (`_expand`).  With
        temporal_selfatt_only=False the temporal attn2 is a cross-attention too: the first one of EITHER kind ends the prefix -- with
        addition_attention that is init_attn's attn2, right behind conv_in.
        pieces: channel counts of the c_concat tensors of a `hybrid*` call (UNetModel.forward_concat): `x_in` holds the remaining
        (latent) channels only, the first conv reads the persistent rows `x_rows` whose columns the sources are scattered into --
        x_in's by a recorded launch, the c_concat ones by `set_concat` (outside the recorded sequence: they change per call on the
        host-issued path and once per trajectory in fifo_graph.BaseEngine).
        adapter: None, or the number of `features_adapter` maps (openaimodel3d.py:562-564): one per input block `i` with
        (i + 1) % 3 == 0, added to that block's output in front of `hs.append` from the plan-owned buffers `adapter_in[k]`
        ([Bx*T, C_k, H_k, W_k] fp32, outside the pool like x_rows; written by `set_adapter`, read by a recorded launch)."""
        self.image_attn = getattr(model, "use_image_attention", False)
        if self.image_attn:
            for Ls in ([L] if isinstance(L, int) else [l for _, l in L]):
                if Ls > IMAGE_CONTEXT_MAX:
                    raise ValueError(f"image-attention UNet: a context of {Ls} tokens is longer than {IMAGE_CONTEXT_MAX} ({TEXT_CONTEXT_LEN} "
                                     f"text + {IMAGE_CONTEXT_MAX - TEXT_CONTEXT_LEN} image tokens, the fused attention's key tile)")
        if T > MAX_FRAMES:
            raise ValueError(f"x has T = {T} frames: the temporal attention kernels take at most {MAX_FRAMES}")
        super().__init__(model, device)
        self.B, self.T, self.H, self.W, self.L = B, T, H, W, L
        self.BT = B * T
        # context segments (videos, tokens) in batch order: one segment normally; the batched FIFO call carries the conditional
        # windows (two prompts, 154 tokens) and the unconditional ones (77) in ONE forward: every cross-attention then runs one
        # launch per segment on its own rows of the shared K|V projection -- no padded or masked keys
        self.segs = [(B, L)] if isinstance(L, int) else [(int(n), int(l)) for n, l in L]
        assert sum(n for n, _ in self.segs) == B
        m = model
        # image cross-attention (use_image_attention): the first 77 rows of a context are text, the rest image tokens (attention.py:82-84);
        # `ctx` holds the text rows of every video, `ctx_img` the image rows, each projected by its own up-front K|V GEMM
        if self.image_attn:
            self.seg_txt = [min(Ls, TEXT_CONTEXT_LEN) for _, Ls in self.segs]
        else:
            self.seg_txt = [Ls for _, Ls in self.segs]
        self.ctx_rows = sum(n * lt for (n, _), lt in zip(self.segs, self.seg_txt))
        self.img_rows = sum(n * (l - lt) for (n, l), lt in zip(self.segs, self.seg_txt))
        if shared_x:
            assert len(self.segs) > 1 and all(n == self.segs[0][0] for n, _ in self.segs)
            self.reps = len(self.segs)
        self.Bx = B // self.reps
        self.pieces = None if pieces is None else tuple(int(k) for k in pieces)
        self.kx = m.in_channels - sum(self.pieces or ())         # channels of x_in (all of them without c_concat)
        if self.kx <= 0 or any(k <= 0 for k in self.pieces or ()):
            raise ValueError(f"c_concat channels {self.pieces} leave no room for x in in_channels={m.in_channels}")
        self.x_in = torch.empty(self.Bx, self.kx, T, H, W, dtype=in_dtype, device=device)
        self.x_rows = None
        self.adapter_sites = [i for i in range(len(m.input_blocks)) if (i + 1) % 3 == 0]
        if adapter is not None and int(adapter) != len(self.adapter_sites):
            raise ValueError(f"adapter={adapter}: this UNet has {len(self.adapter_sites)} adapter sites (input blocks {self.adapter_sites})")
        self.adapter_in = None if adapter is None else []
        self.t_rows = torch.empty(self.BT, dtype=torch.int64, device=device)
        self.fps_rows = torch.empty(self.BT, dtype=torch.int64, device=device)
        self.ctx = torch.empty(self.ctx_rows, m.context_dim, dtype=torch.float16, device=device)
        self.ctx_img = torch.empty(self.img_rows, m.context_dim, dtype=torch.float16, device=device) if self.img_rows else None
        self.out = torch.empty(B, m.out_channels, T, H, W, dtype=in_dtype, device=device)
        self._build()

    # ------------------------------------------------------------------ blocks
    def res_block(self, mod, x):
        """ResBlock._forward, openaimodel3d.py:208-234"""
        P, HW = self.P, x.H * x.W
        g1 = self.gn(x, P[id(mod.in_layers[0])], fps=1, eps=1e-5, silu=True)
        off, width = self.model._emb_cols[id(mod)]
        emb_out = self.emb_all[:, off:off + width]               # this block's columns of the fused emb_layers GEMM
        h1 = self.conv(_FMap(g1, x.F, x.H, x.W, x.C), P[id(mod.in_layers[2])], rowadd=emb_out, rowadd_div=HW)
        self._release(g1)
        g2 = self.gn(h1, P[id(mod.out_layers[0])], fps=1, eps=1e-5, silu=True, x_dead=True)
        self._retire(h1)
        if isinstance(mod.skip_connection, torch.nn.Identity):
            sk = x.buf
        elif isinstance(x, _CatMap):                             # 1x1 conv over the virtual concat: two A sources, split at h's channels
            pw = P[id(mod.skip_connection)]
            sk = self.pool.get(x.M, pw.N)
            self._note_gemm(pw)
            self._emit(ops.gemm, x.h.buf, pw, sk, M=x.M, lda=x.h.buf.stride(-2), splits=1, a2=(x.skip.buf, x.h.C))
        else:
            sk = self.linear(x.buf, x.M, P[id(mod.skip_connection)])
        h2 = self.conv(_FMap(g2, x.F, x.H, x.W, mod.cout), P[id(mod.out_layers[3])], residual=sk)
        self._release(g2)
        if isinstance(x, _CatMap) or sk is not x.buf:
            self._release(sk)
        if not mod.use_temporal_conv:
            return h2
        # TemporalConvBlock.forward, openaimodel3d.py:269-276 (GroupNorm statistics over (C/32, T, H, W))
        tc = mod.temopral_conv
        cur = h2
        for i, (name, idx) in enumerate((("conv1", 2), ("conv2", 3), ("conv3", 3), ("conv4", 3))):
            sq = getattr(tc, name)
            g = self.gn(cur, P[id(sq[0])], fps=self.T, eps=1e-5, silu=True, x_dead=cur is not h2)
            self._drop_colsum(cur)      # (now: the tconv below reuses the freed workspace; h2's rows are read until conv4's residual)
            nxt = self.tconv(_FMap(g, cur.F, cur.H, cur.W, cur.C), P[id(sq[idx])], residual=h2.buf if i == 3 else None)
            self._release(g)
            if cur is not h2:
                self._retire(cur)
            cur = nxt
        self._retire(h2)
        return cur

    # ---- LayerNorm folded into the linear that consumes it ------------------------------------------------------------
    def _folded(self, key, build):
        """LayerNorm-folded packed weights of one consumer (built on first use, kept beside the plain ones)"""
        k = ("lnfold", key)
        if k not in self.P:
            self.P[k] = build()
        return self.P[k]

    def _fold_pw(self, kind, mod, norm):
        """W' = W diag(gamma), b' = b + W beta for the linear `mod` that reads LayerNorm `norm` (ops.fold_layernorm)"""
        g, b = self.P[id(norm)]
        dev = self.device

        def build():
            if kind == "qkv":                                    # fused to_q | to_k | to_v (no biases, attention.py:54-56)
                w = torch.cat([mod.to_q.weight.detach(), mod.to_k.weight.detach(), mod.to_v.weight.detach()], dim=0).to(dev)
                wf, bf = ops.fold_layernorm(w, None, g, b)
                return ops.finish_lnfold(ops.pack_linear(wf, bf, device=dev))
            if kind == "q":
                wf, bf = ops.fold_layernorm(mod.to_q.weight.detach().to(dev), None, g, b)
                return ops.finish_lnfold(ops.pack_linear(wf, bf, device=dev))
            wf, bf = ops.fold_layernorm(mod.weight.detach().to(dev), mod.bias.detach().to(dev), g, b)      # GEGLU.proj
            return ops.finish_lnfold(ops.pack_geglu(wf, bf, device=dev))
        return self._folded(id(mod), build)

    def linear_of_ln(self, l, M, pw, fold_pw):
        """linear(LayerNorm(x)): `l` is either the LayerNorm output (a tensor) or an _LNRef (x + row partial sums left by its
        producer): then the fold runs in this GEMM's epilogue on the folded weights and no LayerNorm pass exists"""
        if isinstance(l, _LNRef):
            pwf = fold_pw()
            out = self.pool.get(M, pwf.n_out if pwf.geglu else pwf.N)
            self._note_gemm(pwf)
            self._emit(ops.gemm, l.x, pwf, out, M=M, lda=l.x.stride(-2), splits=1, lnfold=(l.part, l.nparts, 1e-5))
            return out
        return self.linear(l, M, pw)

    def _release_ln(self, l):
        self._release(l.part if isinstance(l, _LNRef) else l)

    def _tattn_pw(self, att, norm, heads, folded):
        """to_q|to_k|to_v packed per head for MOCA_EP_TATTN (LayerNorm-folded when the input arrives as an _LNRef)"""
        dev = self.device

        def build():
            wq, wk, wv = (m.weight.detach().to(dev) for m in (att.to_q, att.to_k, att.to_v))
            if not folded:
                return ops.pack_qkv_per_head(wq, wk, wv, heads, device=dev)
            g, b = self.P[id(norm)]
            wf, bf = ops.fold_layernorm(torch.cat([wq, wk, wv], dim=0), None, g, b)
            c = wq.shape[0]
            return ops.finish_lnfold(ops.pack_qkv_per_head(wf[:c], wf[c:2 * c], wf[2 * c:], heads, bias=bf, device=dev))
        k = ("tqkv_fold" if folded else "tqkv", id(att))
        if k not in self.P:
            self.P[k] = build()
        return self.P[k]

    def _attn_temporal_fused(self, att, l, M, Cn, heads, HW, norm, causal=False):
        """q|k|v projection + attention over the frame axis in ONE launch (MOCA_EP_TATTN) where its 320-row tiles (16 frames x 20
        pixels, one head) come in whole rounds of the chip; None -> the caller runs projection + temporal_attention.
        Used wherever the kernel applies (round-2 same-device A/B of the whole CFG step: never 37.2 ms, only where the tile count is a
        multiple of 256 or >= 1024 36.4, everywhere 36.0 -- the launch and the q|k|v round trip it removes outweigh the partial last
        round of tiles at the 640- and 1280-channel levels).
        causal: the mask of TemporalTransformer(causal_attention=True) in the epilogue's softmax (moca_gemm_params.tattn_causal), so a
        causal model keeps the fused form wherever the non-causal one has it."""
        if self.T != 16 or HW % 20:
            return None
        folded = isinstance(l, _LNRef)
        x = l.x if folded else l
        pw = self._tattn_pw(att, norm, heads, folded)
        scale = att.dim_head ** -0.5
        kw = dict(M=M, lda=x.stride(-2), splits=1, tattn=(self.T, HW, scale, True) if causal else (self.T, HW, scale))
        if not ops.gemm_tattn_ok(x, pw, lnfold=(None, l.nparts, 1e-5) if folded else None, **kw):
            return None
        o = self.pool.get(M, Cn)
        self._note_gemm(pw)
        self._emit(ops.gemm, x, pw, o, lnfold=(l.part, l.nparts, 1e-5) if folded else None, **kw)
        return o

    def _attn_self(self, att, l, M, Cn, heads, spatial, F, HW, norm=None, causal=False):
        P = self.P
        assert not (spatial and causal)
        if not spatial:
            o = self._attn_temporal_fused(att, l, M, Cn, heads, HW, norm, causal)
            if o is not None:
                return o
        qkv = self.linear_of_ln(l, M, P[id(att)], lambda: self._fold_pw("qkv", att, norm))   # [M][3C] fused to_q|to_k|to_v
        o = self.pool.get(M, Cn)
        q, k, v = qkv[:, :Cn], qkv[:, Cn:2 * Cn], qkv[:, 2 * Cn:]
        scale = att.dim_head ** -0.5
        if spatial:
            self._emit(ops.attention, q, k, v, o, Bq=F, heads=heads, Nq=HW, Nk=HW, ldq=3 * Cn, ldk=3 * Cn, ldv=3 * Cn,
                       ldo=Cn, kv_div=1, scale=scale)
        elif self.T > 16:                    # one 32 x 32 score tile per (video, pixel, head)
            self._emit(ops.temporal_attention_long, q, k, v, o, B=M // (self.T * HW), T=self.T, HW=HW, heads=heads, ld_qkv=3 * Cn,
                       ldo=Cn, scale=scale, causal=causal)
        else:
            self._emit(ops.temporal_attention_causal if causal else ops.temporal_attention, q, k, v, o, B=M // (self.T * HW), T=self.T,
                       HW=HW, heads=heads, ld_qkv=3 * Cn, ldo=Cn, scale=scale)
        self._release(qkv)
        return o

    def _attn_cross(self, att, l, M, Cn, heads, F, HW, norm=None, expand=False):
        """expand: `l` (and so q) still has the rows of the Bx distinct latents; every context segment attends with the SAME q rows
        and writes its own rows of o, which comes out with reps x M rows"""
        q = self.linear_of_ln(l, M, self.P[id(att)], lambda: self._fold_pw("q", att, norm))
        off, inner = self.model._kv_cols[id(att)]                # one K/V per video (context.repeat_interleave, :547),
        ld = self.kv_all.shape[1]                                # all layers' K|V projected by one GEMM up front
        o = self.pool.get(M * (self.reps if expand else 1), Cn)
        r0 = k0 = i0 = 0
        segs = self.segs
        if not expand and len(segs) > 1 and all(Ls == segs[0][1] for _, Ls in segs):
            segs = [(sum(nv for nv, _ in segs), segs[0][1])]     # equal context lengths: the segments are one contiguous batch
        for nv, Ls in segs:                                      # (one launch per context segment: rows of q / o, rows of K|V)
            rows = nv * self.T * HW
            Lt = min(Ls, TEXT_CONTEXT_LEN) if self.image_attn else Ls
            Li = Ls - Lt
            kv = self.kv_all[k0:k0 + nv * Lt]
            qs = q[0:rows] if expand else q[r0:r0 + rows]
            if Li:                                               # text + image tokens: both softmaxes in one launch
                kvi = self.kv_ip_all[i0:i0 + nv * Li]
                ldi = self.kv_ip_all.shape[1]
                self._emit(ops.attention_ip, qs, kv[:, off:off + inner], kv[:, off + inner:off + 2 * inner], kvi[:, off:off + inner],
                           kvi[:, off + inner:off + 2 * inner], o[r0:r0 + rows], Bq=nv * self.T, heads=heads, Nq=HW, Nt=Lt, Ni=Li,
                           ldq=Cn, ldk=ld, ldv=ld, ldk_ip=ldi, ldv_ip=ldi, ldo=Cn, kv_div=self.T, scale=att.dim_head ** -0.5,
                           ip_scale=att.image_cross_attention_scale)
            else:                                                # (<= 77 tokens: the reference's image slice is empty, adds 0)
                self._emit(ops.attention, qs, kv[:, off:off + inner], kv[:, off + inner:off + 2 * inner], o[r0:r0 + rows],
                           Bq=nv * self.T, heads=heads, Nq=HW, Nk=Lt, ldq=Cn, ldk=ld, ldv=ld, ldo=Cn, kv_div=self.T,
                           scale=att.dim_head ** -0.5)
            r0 += rows
            k0 += nv * Lt
            i0 += nv * Li
        self._release(q)
        return o

    def _expand(self, buf, rows, cols):
        """[rows][cols] -> reps copies (the branches of a shared-latents batch separate here)"""
        out = self.pool.get(rows * self.reps, cols)
        self._emit(ops.repeat, buf.reshape(-1)[:rows * cols], out, reps=self.reps)
        return out

    def linear_ln(self, a, M, pw, gb, residual=None, consumer=None, wgroup=None):
        """`out = linear(a) (+ residual)` and `l = LayerNorm(out)` (eps 1e-5, attention.py:199-201).
        (1) `consumer` = a callable returning the LayerNorm-folded weights of the ONE linear that reads l: when this launch can
        leave row sums behind (MOCA_EP_ROWSUM) and the consumer's kernel has the fold epilogue (MOCA_EP_LNFOLD), l is an
        _LNRef and LayerNorm never touches memory; (2) ONE launch writing out and LayerNorm(out) where the 160 x 320 tiling
        applies (N = 320: a block owns whole rows and normalises them in its store loop, MOCA_EP_LN); (3) otherwise the linear
        followed by the LayerNorm kernel."""
        lda = a.stride(-2)
        splits = self._splits(M, pw)
        wk = {} if wgroup is None else {"wgroup": wgroup}      # (`pw` = per-row-group weights: a GroupNorm folded in, see transformer())
        ln_epilogue = ops.gemm_ln_ok(a, pw, M=M, lda=lda, residual=residual, splits=splits, ln=(gb[0], gb[1], None, 1e-5), **wk)
        # Measured (same device, whole CFG step, tools/ab_run7.sh): fold wherever possible 36.9 ms, fold only where neither the
        # LayerNorm store loop (N = 320) nor more than two row partials apply 37.3, never 37.6.  In isolation the consumers pay
        # 3-12 % for the two FMAs per accumulator and the statistics loads (tools/bench_lnfold.py; worst at K = 320 and with the
        # 10 partials of the 1280-channel level), less than the LayerNorm pass and the second output they replace cost in the
        # graph.  So: fold wherever producer and consumer kernels allow.
        if consumer is not None and splits == 1:
            cols = ops.gemm_rowsum_cols(a, pw, M=M, lda=lda, residual=residual, splits=1, rowsum=True, **wk)
            nparts = pw.N // cols if cols > 0 else 0
            if cols > 0:
                pwf = consumer()
                if ops.gemm_lnfold_ok(a, pwf, M=M, lda=pw.N, splits=self._splits(M, pwf), lnfold=(None, nparts, 1e-5)) and \
                        self._splits(M, pwf) == 1:
                    out = self.pool.get(M, pw.N)
                    part = self.pool.get(nparts * M, 2, torch.float32)
                    self._note_gemm(pw)
                    self._emit(ops.gemm, a, pw, out, M=M, lda=lda, residual=residual, splits=1, rowsum=part, **wk)
                    return out, _LNRef(out, part, nparts)
        if ln_epilogue:
            out, l = self.pool.get(M, pw.N), self.pool.get(M, pw.N)
            self._note_gemm(pw)
            self._emit(ops.gemm, a, pw, out, M=M, lda=lda, residual=residual, splits=1, ln=(gb[0], gb[1], l, 1e-5), **wk)
            return out, l
        assert wgroup is None or splits == 1
        out = self._gemm(a, pw, M, lda=lda, residual=residual, **wk)
        return out, self.ln(out, M, pw.N, gb)

    def tblock(self, blk, h, l, M, Cn, heads, spatial, F, HW, next_gb=None, next_consumer=None, causal=False):
        """BasicTransformerBlock._forward, attention.py:216-220.  `l` = norm1(h), already computed by the producer of h;
        returns (h_out, norm1 of the NEXT block applied to it or None, rows, frames) -- rows / frames grow by `reps` when this
        block holds the first cross-attention of a shared-latents plan (a spatial attn2, or the attn2 of a temporal block with
        only_self_att=False: its rows are (frame, pixel) queries of their video's tokens exactly as the spatial ones).
        causal: `mask` of :217-218 -- it reaches attn1 AND attn2, both self-attentions over the frames (the cross branch of
        TemporalTransformer.forward passes none, :362-363)."""
        P = self.P
        geglu = blk.ff.net[0].proj
        consumers = (self._ln_consumer(blk.attn2, blk.norm2), lambda: self._fold_pw("geglu", geglu, blk.norm3))
        for (att, cur, nxt), cons in zip(((blk.attn1, blk.norm1, blk.norm2), (blk.attn2, blk.norm2, blk.norm3)), consumers):
            if att.is_self:
                o = self._attn_self(att, l, M, Cn, heads, spatial, F, HW, norm=cur, causal=causal)
            else:
                assert not causal
                expand = self.reps > 1 and F == self.Bx * self.T      # first use of the contexts: the shared prefix ends here
                o = self._attn_cross(att, l, M, Cn, heads, F, HW, norm=cur, expand=expand)
                if expand:
                    h2 = self._expand(h, M, Cn)
                    self._release(h)
                    h, M, F = h2, M * self.reps, F * self.reps
            self._release_ln(l)
            nh, l = self.linear_ln(o, M, P[id(att.to_out[0])], P[id(nxt)], residual=h, consumer=cons)
            self._release(o, h)
            h = nh
        ff = self.linear_of_ln(l, M, P[id(geglu)], consumers[1])  # GEGLU fused into the epilogue
        self._release_ln(l)
        if next_gb is not None:
            nh, l = self.linear_ln(ff, M, P[id(blk.ff.net[2])], next_gb, residual=h, consumer=next_consumer)
        else:
            nh, l = self.linear(ff, M, P[id(blk.ff.net[2])], residual=h), None
        self._release(ff, h)
        return nh, l, M, F

    def _ln_consumer(self, att, norm):
        """the folded weights of the projection that reads `norm` in front of attention `att`"""
        return lambda: self._fold_pw("qkv" if att.is_self else "q", att, norm)

    def _gn_fold(self, fm, gb, pw, *, fps, eps):
        """GroupNorm(32, no activation) -> Linear as ONE GEMM on per-statistics-group weights, where (a) the producer of `fm` can leave the
        FINISHED statistics behind (the condition of gn()'s single-launch path: a GEMM whose row tiles lie inside one statistics group, or
        a concat that accumulated them) and (b) the linear runs on a staggered kernel whose row tiles lie inside one group
        (moca_gemm_wgroup_ok).  Returns (per-group PackedWeight, (rows per group, stride)) or None (the caller runs gn() + the linear)."""
        if not GN_FOLD or isinstance(fm, _CatMap) or fm.slabs is not None or fm.C % 32 or pw.geglu:
            return None
        rows = fps * fm.H * fm.W
        # worth it only while the derived weights (written once, read by the group's row tiles) are small against the tensor the GroupNorm
        # pass would read and write: rows per group >= 4 N.  (640-channel level, per-frame statistics: 640 rows per group -- 256 frames x
        # 819 KB of weights at B = 16, as many bytes as the pass itself: measured no gain; that norm stays a launch)
        if not self._stats_ready(fm, fps) or fm.F % fps or rows < 4 * pw.N:
            return None
        stride = pw.N * pw.w.stride(0)
        if not ops.gemm_wgroup_ok(fm.buf, pw, M=fm.M, lda=fm.buf.stride(-2), splits=self._splits(fm.M, pw), wgroup=(rows, stride)):
            return None
        n_sg = fm.F // fps
        slot = self._finished_stats(fm, fps)
        wg = self.pool.get(n_sg * pw.N, pw.w.stride(0))
        bg = self.pool.get(1, n_sg * pw.N, torch.float32)
        self._emit(ops.groupnorm_fold_weights, pw, gb[0], gb[1], slot, wg, bg, n_sg=n_sg, count=rows * (fm.C // 32), eps=eps)
        pwg = ops.PackedWeight(wg, bg.reshape(-1), pw.N, pw.K, pw.n_out)
        pwg.derived = True
        return pwg, (rows, stride)

    def transformer(self, mod, x, spatial):
        """SpatialTransformer.forward attention.py:262-278 / TemporalTransformer.forward :331-373"""
        P = self.P
        blocks = list(mod.transformer_blocks)
        causal = False
        if not spatial:
            causal = mod.causal
            if causal and self.T != mod.temporal_length:
                # the reference's mask is tril(ones(1, temporal_length, temporal_length)) (attention.py:311): it broadcasts against
                # the [.., T, T] scores only when the two agree
                raise ValueError(f"causal temporal attention: x has T = {self.T} frames, the model was built with temporal_length = "
                                 f"{mod.temporal_length} (the reference's mask broadcasts only when they are equal)")
            if not mod.only_self_att and (x.H * x.W) % self.T:
                # attention.py:359-361 repeats the context over the pixels as (t r), r = hw // t: with hw % t != 0 it has fewer rows than
                # the hw queries and the reference fails.  (With one context per video the mapping itself never matters.)
                raise ValueError(f"temporal cross-attention (temporal_selfatt_only=False): a {x.H} x {x.W} map has hw = {x.H * x.W} "
                                 f"pixels, not a multiple of T = {self.T}; the reference's context repeat (t r), r = hw // t, fails there")
        fold = self._gn_fold(x, P[id(mod.norm)], P[id(mod.proj_in)], fps=1 if spatial else self.T, eps=1e-6)
        if fold is not None:
            # `x = self.norm(x)` (attention.py:262-268 / :333-341) lives in proj_in's per-statistics-group weights: no GroupNorm launch,
            # the normalised tensor is never written
            pwg, wgroup = fold
            h, l = self.linear_ln(x.buf, x.M, pwg, P[id(blocks[0].norm1)], consumer=self._ln_consumer(blocks[0].attn1, blocks[0].norm1),
                                  wgroup=wgroup)
            self._release(pwg.w, pwg.bias)
        else:
            n = self.gn(x, P[id(mod.norm)], fps=1 if spatial else self.T, eps=1e-6, silu=False)
            h, l = self.linear_ln(n, x.M, P[id(mod.proj_in)], P[id(blocks[0].norm1)],
                                  consumer=self._ln_consumer(blocks[0].attn1, blocks[0].norm1))
            self._release(n)
        M, Fr, xres = x.M, x.F, x.buf
        for i, blk in enumerate(blocks):
            last = i + 1 >= len(blocks)
            nxt = None if last else P[id(blocks[i + 1].norm1)]
            ncons = None if last else self._ln_consumer(blocks[i + 1].attn1, blocks[i + 1].norm1)
            h, l, M, Fr = self.tblock(blk, h, l, M, mod.inner, mod.heads, spatial, Fr, x.H * x.W, next_gb=nxt, next_consumer=ncons,
                                      causal=causal)
        if Fr != x.F:                                            # the shared prefix ended inside: the outer residual too
            xres = self._expand(x.buf, x.M, x.C)
        # (a split-K proj_out, e.g. M = 640 at B = 1, defers its reduce like the convs: gn() or _retire() of the map settles it)
        o = self._gemm_map(Fr, x.H, x.W, h, P[id(mod.proj_out)], lda=h.stride(-2), residual=xres)
        assert o.C == x.C and o.M == M
        self._release(h)
        if xres is not x.buf:
            self._release(xres)
        return o

    def run_seq(self, seq, h):
        """TimestepEmbedSequential.forward, openaimodel3d.py:36-48"""
        for layer in seq:
            if isinstance(layer, _ResBlock):
                nh = self.res_block(layer, h)
            elif isinstance(layer, _SpatialTransformer):
                nh = self.transformer(layer, h, True)
            elif isinstance(layer, _TemporalTransformer):
                nh = self.transformer(layer, h, False)
            elif isinstance(layer, _Downsample):
                nh = self.conv(h, self.P[id(layer.op)], stride=2)
            elif isinstance(layer, _Upsample):
                nh = self.upconv(h, layer.conv)
            else:
                raise TypeError(type(layer))
            self._retire(h)     # (of a virtual concat: whatever _virtual_cat did not re-target -- column sums nobody read, a deferred workspace)
            h = nh
        return h

    # ------------------------------------------------------------------ whole forward
    def _embed_mlp(self, sq, rows_t):
        """timestep_embedding -> Linear -> SiLU -> Linear (openaimodel3d.py:362-372,536-543)"""
        m, P, BT = self.model, self.P, self.BT
        te = self.pool.get(BT, m.model_channels)
        self._emit(ops.timestep_embedding, rows_t, te, n=BT, dim=m.model_channels)
        e1 = self.linear(te, BT, P[id(sq[0])])
        s1 = self.pool.get(BT, e1.shape[1])
        self._emit(ops.silu_add_rows, e1, 1, None, 1, s1, rows=BT, Cn=e1.shape[1], silu=True)
        e2 = self.linear(s1, BT, P[id(sq[2])])
        self._release(te, e1, s1)
        return e2

    def _build(self):
        m, P, B, T, H, W = self.model, self.P, self.B, self.T, self.H, self.W
        BT = self.BT
        emb = self._embed_mlp(m.time_embed, self.t_rows)
        femb = self._embed_mlp(m.fps_embedding, self.fps_rows) if m.fps_cond else None
        # every consumer of `emb` is ResBlock.emb_layers = SiLU -> Linear (openaimodel3d.py:166-172)
        self.emb_silu = self.pool.get(BT, emb.shape[1])
        self._emit(ops.silu_add_rows, emb, 1, femb, 1, self.emb_silu, rows=BT, Cn=emb.shape[1], silu=True)
        self._release(emb, femb)
        self._pinned.add(self.emb_silu.data_ptr())
        self.emb_all = self.linear(self.emb_silu, BT, P["emb_all"])          # [BT][sum Cout]: every ResBlock's emb_layers
        self._pinned.add(self.emb_all.data_ptr())
        self.kv_all = None
        if "ctx_kv_all" in P:
            self.kv_all = self.linear(self.ctx, self.ctx_rows, P["ctx_kv_all"])  # [sum B_i L_i][sum 2C]: every cross-attention K|V
            self._pinned.add(self.kv_all.data_ptr())
        self.kv_ip_all = None
        if self.ctx_img is not None:
            self.kv_ip_all = self.linear(self.ctx_img, self.img_rows, P["ctx_kv_ip_all"])  # [sum B_i (L_i - 77)][sum 2C]: image K|V
            self._pinned.add(self.kv_ip_all.data_ptr())

        FT = self.Bx * T                                         # frames of the distinct latents (= BT unless shared_x)
        Cpad = m.in_cpad
        if self.pieces is None:
            x8 = self.pool.get(FT * H * W, Cpad)
            self._emit(ops.ncthw_to_nhwc, self.x_in, x8, B=self.Bx, Cin=m.in_channels, T=T, HW=H * W, Cpad=Cpad)
            h = self.conv(_FMap(x8, FT, H, W, Cpad), P[id(m.input_blocks[0][0])])
            self._release(x8)
        else:
            # torch.cat([x] + c_concat, dim=1) (ddpm3d.py:715) never exists: the rows live outside the pool (the c_concat columns must
            # survive from set_concat to the conv, and across the steps of a trajectory), pad columns zeroed here once
            self.x_rows = torch.zeros(FT * H * W, Cpad, dtype=torch.float16, device=self.device)
            self._emit(ops.ncthw_scatter, self.x_in, self.x_rows, B=self.Bx, k=self.kx, T=T, HW=H * W, Cpad=Cpad, c0=0)
            h = self.conv(_FMap(self.x_rows, FT, H, W, Cpad), P[id(m.input_blocks[0][0])])
        hs = []
        for i, module in enumerate(m.input_blocks):
            if i == 0:
                if m.addition_attention:
                    nh = self.transformer(m.init_attn[0], h, False)
                    self._retire(h)
                    h = nh
            else:
                h = self.run_seq(module, h)
            if self.adapter_in is not None and (i + 1) % 3 == 0:
                self._adapter_add(h, FT)
            hs.append(h)
            self._pinned.add(h.buf.data_ptr())
        h = self.run_seq(m.middle_block, h)
        if h.F != BT:                                            # (no cross-attention anywhere: nothing ever separated the branches)
            h = _FMap(self._expand(h.buf, h.M, h.C), BT, h.H, h.W, h.C)
        for module in m.output_blocks:
            skip = hs.pop()
            if skip.F != h.F:                                    # a skip connection from the shared prefix
                self._pinned.discard(skip.buf.data_ptr())
                wide = self._expand(skip.buf, skip.M, skip.C)
                self._retire(skip)
                own, own_F = skip.gstat_own, skip.F
                skip = _FMap(wide, h.F, skip.H, skip.W, skip.C)
                skip.gstat_own, skip.own_F = own, own_F          # (the copies share the statistics of the frames they repeat)
            vc = self._virtual_cat(module, h, skip)
            if vc is not None:
                self._pinned.discard(skip.buf.data_ptr())
                h = self.run_seq(module, vc)                     # (run_seq releases h.buf and skip.buf behind the ResBlock)
                continue
            cat = self.pool.get(h.M, h.C + skip.C)
            gst = None
            Cc = h.C + skip.C
            if isinstance(module[0], _ResBlock) and Cc % 32 == 0 and \
                    64 <= (Cc // 8) * max(1, 256 // (Cc // 8)) and Cc // 8 <= 1024:
                # torch.cat(dim=1), :571, leaving the statistics of ResBlock.in_layers[0] (per-frame GroupNorm) behind
                gst = (self._gstat_slot(h.F * 64), 1)
                self._emit(ops.concat_channels_gstat, h.buf, skip.buf, cat, gst[0], F=h.F, HW=h.H * h.W, C1=h.C, C2=skip.C,
                           frames_per_stat=1)
            else:
                self._emit(ops.concat_channels, h.buf, skip.buf, cat, rows=h.M, C1=h.C, C2=skip.C)   # torch.cat(dim=1), :571
            self._pinned.discard(skip.buf.data_ptr())
            self._retire(h)               # (a concat consumed h: its producer goes back to the plain store loop)
            self._retire(skip)
            h = self.run_seq(module, _FMap(cat, h.F, h.H, h.W, Cc, gstat=gst))
        g = self.gn(h, P[id(m.out[0])], fps=1, eps=1e-5, silu=True)
        self._retire(h)
        o = self.conv(_FMap(g, h.F, h.H, h.W, h.C), P[id(m.out[2])])
        self._release(g)
        self._emit(ops.nhwc_to_ncthw, o.buf, o.C, self.out, B=B, Cout=m.out_channels, T=T, HW=H * W)
        self._retire(o)
        self._finish_prefetch()

    def _adapter_add(self, h, FT):
        """`h = h + features_adapter[adapter_idx]` (openaimodel3d.py:562-564) in place on h's rows; both branches of a shared prefix
        read the same FT source frames.  Whatever h's producer left behind or promised for a GroupNorm consumer (per-tile column
        sums, a split-K reduce that could still move into the consumer) describes the tensor BEFORE the add: it is dropped -- the
        producer goes back to its plain store loop and its own reduce -- and every consumer of the sum (the next block's GroupNorm or
        transformer norm, the output block that reads it as skip) runs its own statistics pass."""
        self._drop_colsum(h)
        assert h.gstat is None and h.gstat_own is None      # (set by consumers only: h has none yet)
        h.src, h.cs_rows = None, 0
        src = torch.empty(FT, h.C, h.H, h.W, dtype=torch.float32, device=self.device)
        self.adapter_in.append(src)
        self._emit(ops.nchw_add_rows, h.buf, src, F=h.F, Fsrc=FT, Cn=h.C, HW=h.H * h.W)

    def _virtual_cat(self, module, h, skip):
        """torch.cat([h, skip], dim=1) (openaimodel3d.py:571) WITHOUT the copy, where both consumers can read two sources: the
        ResBlock's in_layers GroupNorm (moca_groupnorm_gstat_cat_f16) and its skip_connection 1x1 conv (moca_gemm_params.a2, the
        staggered kernels: the 320- / 640-channel levels).  The statistics of the concat's 32 groups come from the producers: h's
        last GEMM is re-targeted to accumulate ITS share in the concat's grouping (gstat_cpg); skip's share is its own finished
        per-frame statistics when its producer already left them for the input path (merged by the GroupNorm), else its producer
        is re-targeted likewise; a source without such a producer (an `Upsample`, the repeat that ends the shared prefix) gets a
        read-only statistics pass.  Returns a _CatMap, or None (the caller materialises the concat)."""
        if not VIRTUAL_CAT or not isinstance(module[0], _ResBlock) or isinstance(module[0].skip_connection, torch.nn.Identity):
            return None
        Cc, HW = h.C + skip.C, h.H * h.W
        if Cc % 32 or h.C % 64 or skip.C % 64 or Cc // 8 > 1024 or h.F != skip.F:
            return None
        pw = self.P[id(module[0].skip_connection)]
        if self._splits(h.M, pw) != 1 or not ops.gemm_cat_ok(h.buf, pw, M=h.M, lda=h.buf.stride(-2), splits=1, a2=(skip.buf, h.C)):
            return None
        gw = Cc // 32
        slot = self._gstat_slot(h.F * 64)

        def retarget(fm, coff):
            """fm's producer accumulates fm's share of the concat's per-frame statistics (a row tile must lie inside one frame)"""
            rows = fm.colsum[1] if fm.colsum is not None else fm.cs_rows
            phases = isinstance(fm.src, tuple)                   # an `Upsample` as four 2 x 2 convs on the low-resolution grid
            grp = HW // 4 if phases else HW                     # GEMM rows per frame
            if fm.src is None or rows <= 0 or grp % rows or fm.gstat_own is not None:
                return False
            for i in (fm.src if phases else (fm.src,)):
                kw = self.steps[i].keywords
                if kw.get("gstat") is not None or kw.get("rowsum") is not None:
                    return False
                self._retarget(i, colsum=None, gstat=(slot, grp, gw, coff))
            if fm.colsum is not None:
                self.pool.put(fm.colsum[0])
                fm.colsum = None
            fm.src = None
            return True

        if not retarget(h, 0):
            self._drop_colsum(h)
            self._emit(ops.gstat_accum, h.buf, slot, F=h.F, HW=HW, Cn=h.C, frames_per_stat=1, cpg=gw, coff=0)
        gb, Fb = None, 0
        cpg2 = skip.C // 32
        if skip.gstat_own is not None and skip.gstat_own[1] == 1 and skip.C % 32 == 0 and gw % cpg2 == 0 and (h.C % gw) % cpg2 == 0:
            gb, Fb = skip.gstat_own[0], skip.own_F
        elif not retarget(skip, h.C):
            self._drop_colsum(skip)
            self._emit(ops.gstat_accum, skip.buf, slot, F=skip.F, HW=HW, Cn=skip.C, frames_per_stat=1, cpg=gw, coff=h.C)
        return _CatMap(h, skip, slot, gb, Fb)

    def set_context(self, context):
        """context [B, L, D], or one [n_i, L_i, D] tensor per segment"""
        if torch.is_tensor(context) and not self.img_rows:
            self.ctx.copy_(context.reshape(self.ctx_rows, -1), non_blocking=True)
            return
        if torch.is_tensor(context):
            context = [context]
        r = ri = 0
        for (nv, Ls), Lt, c in zip(self.segs, self.seg_txt, context):
            if Lt == Ls:
                self.ctx[r:r + nv * Ls].copy_(c.reshape(nv * Ls, -1), non_blocking=True)
            else:                                                # text rows -> ctx, image rows -> ctx_img
                self.ctx[r:r + nv * Lt].view(nv, Lt, -1).copy_(c[:, :Lt], non_blocking=True)
                self.ctx_img[ri:ri + nv * (Ls - Lt)].view(nv, Ls - Lt, -1).copy_(c[:, Lt:], non_blocking=True)
            r += nv * Lt
            ri += nv * (Ls - Lt)

    def set_concat(self, c_concat):
        """write the c_concat tensors [Bx, k_i, T, H, W] into their columns of the first conv's input rows (launches on the current
        ops stream; the latent columns [0, kx) belong to the recorded scatter of x_in)"""
        if self.pieces is None or len(c_concat) != len(self.pieces):
            raise ValueError(f"this plan was built for c_concat channels {self.pieces}")
        c0 = self.kx
        for k, c in zip(self.pieces, c_concat):
            if tuple(c.shape) != (self.Bx, k, self.T, self.H, self.W):
                raise ValueError(f"c_concat entry {tuple(c.shape)}: expected {(self.Bx, k, self.T, self.H, self.W)}")
            if c.dtype not in (torch.float32, torch.float16):
                c = c.float()
            ops.ncthw_scatter(c.to(self.device).contiguous(), self.x_rows, B=self.Bx, k=k, T=self.T, HW=self.H * self.W,
                              Cpad=self.x_rows.shape[1], c0=c0)
            c0 += k

    def set_adapter(self, features):
        """copy the `features_adapter` maps into the plan's buffers (on the current torch stream).  Every entry must be exactly
        [Bx*T, C_k, H_k, W_k], fp32 or fp16: the reference's `h + feat` would broadcast other shapes, here they are refused."""
        if self.adapter_in is None or len(features) != len(self.adapter_in):
            raise ValueError(f"this plan was built for {0 if self.adapter_in is None else len(self.adapter_in)} features_adapter maps")
        for k, (f, dst) in enumerate(zip(features, self.adapter_in)):
            if not torch.is_tensor(f) or tuple(f.shape) != tuple(dst.shape):
                raise ValueError(f"features_adapter[{k}] {tuple(f.shape) if torch.is_tensor(f) else type(f)}: expected {tuple(dst.shape)}")
            if f.dtype not in (torch.float32, torch.float16):
                raise ValueError(f"features_adapter[{k}] is {f.dtype}: expected float32 or float16")
        for f, dst in zip(features, self.adapter_in):
            dst.copy_(f, non_blocking=True)

    def launch_async(self, x, t_rows, fps_rows, context, cur, c_concat=None, features_adapter=None):
        """enqueue one forward on this plan's stream (ordered after `cur`); the caller joins"""
        if (c_concat is None) != (self.pieces is None):
            raise ValueError("c_concat goes with a plan built for it (UNetModel.forward_concat)")
        if (features_adapter is None) != (self.adapter_in is None):
            raise ValueError("features_adapter goes with a plan built for it (UNetModel.forward(features_adapter=...))")
        with self._enqueue(cur):
            self.x_in.copy_(x, non_blocking=True)
            self.t_rows.copy_(t_rows, non_blocking=True)
            self.fps_rows.copy_(fps_rows, non_blocking=True)
            self.set_context(context)
            if features_adapter is not None:
                self.set_adapter(features_adapter)
            if c_concat is not None:
                with self._ops_stream():
                    self.set_concat(c_concat)
            self._replay()
            return self.out.clone()

    def run(self, x, t_rows, fps_rows, context, c_concat=None, features_adapter=None):
        cur = torch.cuda.current_stream(self.device)
        out = self.launch_async(x, t_rows, fps_rows, context, cur, c_concat=c_concat, features_adapter=features_adapter)
        out.record_stream(cur)
        cur.wait_stream(self.stream)
        return out

