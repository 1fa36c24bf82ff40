"""torch.autograd Functions over the libcsts_hip.so C ABI.

PyTorch is plumbing here (device memory from the caching allocator, the current HIP stream, the
autograd tape); every FLOP of the CSTS path runs in the hand-written gfx950 kernels.  There is no
eager fallback: tensors must be on a GPU and the library must load, otherwise these raise.
Each Function cites the reference op it replaces (paths under the reference repo).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import functools
import math
import os
import weakref
from typing import Optional, Sequence, Tuple

import torch
from torch.autograd import Function

from . import lib as L

F32, BF16 = L.F32, L.BF16


def _lib():
    return L.load()


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == L.half_dtype():       # bfloat16, or float16 in a process that runs the fp16 build (lib.set_half)
        return BF16
    raise L.CstsError(f"unsupported dtype {t.dtype} (this process runs the {L.HALF} kernel library)")


def torch_dtype(dt: int):
    return torch.float32 if dt == F32 else L.half_dtype()


try:
    _raw_stream, _cur_dev = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice
except AttributeError:          # CPU-only build of torch: ops raise before they get here
    _raw_stream = _cur_dev = None


def _stream():
    """Raw hipStream_t of torch's current stream (torch.cuda.current_stream().cuda_stream costs ~4 us per call, and
    there are ~1200 launches per step)."""
    if _raw_stream is not None:
        return _raw_stream(_cur_dev())
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor], off_elems: int = 0):
    if t is None:
        return None
    return t.data_ptr() + off_elems * t.element_size()


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.CstsError("csts_amd ops need GPU tensors (no CPU fallback); got a CPU tensor")


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


_host_tables = []       # weak references to every HostTable of the process


def refill_capture_pools():
    """Called by the graph-capturing steps (csts_amd.train) right before a capture pass: every table gets its full set of
    capture buffers back, so a process may capture any number of steps one after the other."""
    for r in list(_host_tables):
        t = r()
        if t is None:
            _host_tables.remove(r)
        else:
            t.refill()


class HostTable:
    """Small host -> device table upload that is safe while the host runs ahead of the GPU (a ring of pinned buffers,
    a slot is reused only after its copy has executed) and under HIP-graph capture (pre-allocated pinned buffers that
    are never written again, so a replay copies the captured contents)."""

    def __init__(self, nbytes: int, device, ring: int = 4, captures: int = 8):
        self.nbytes, self.device = nbytes, device
        self._ring = [torch.zeros(nbytes, dtype=torch.uint8).pin_memory() for _ in range(ring)]
        self._ev = [None] * ring
        self._pos = 0
        self._captures = captures
        self._pool = [torch.zeros(nbytes, dtype=torch.uint8).pin_memory() for _ in range(captures)]
        self._captured = []
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        _host_tables.append(weakref.ref(self))

    def refill(self):
        """Top the capture pool up again (outside a capture: pinned allocations are not allowed while one is open)."""
        while len(self._pool) < self._captures:
            self._pool.append(torch.zeros(self.nbytes, dtype=torch.uint8).pin_memory())

    def upload(self, payload: bytes) -> int:
        n = len(payload)
        if n > self.nbytes:
            raise L.CstsError(f"HostTable: {n} bytes > capacity {self.nbytes}")
        src = torch.frombuffer(bytearray(payload), dtype=torch.uint8)
        if torch.cuda.is_current_stream_capturing():
            if not self._pool:
                raise L.CstsError("HostTable: out of capture buffers")
            host = self._pool.pop()
            host[:n].copy_(src)
            self._captured.append(host)
            self.dev[:n].copy_(host[:n], non_blocking=True)
        else:
            k = self._pos
            self._pos = (k + 1) % len(self._ring)
            if self._ev[k] is not None:
                self._ev[k].synchronize()
            self._ring[k][:n].copy_(src)
            self.dev[:n].copy_(self._ring[k][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._ev[k] = ev
        return self.dev.data_ptr()


# Second stages of the cross-workgroup reductions of backward (LayerNorm dgamma/dbeta, stencil dweight): ~190 tiny
# launches per step when done in line.  Inside a backward pass they are deferred instead: the first-stage kernels leave
# their partial rows in a workspace, and ONE csts_reduce_rows_batched launch finishes all of them from an autograd final
# callback (which runs on the caller's stream after the engine has joined every stream backward used).
#
# A deferred gradient is NOT handed to autograd (an unfilled buffer would be adopted by AccumulateGrad only while the
# parameter has no .grad yet, and be ADDED, garbage and all, when it has one: gradient accumulation, a module applied twice).
# The Function returns None for that input; the final callback launches the finishing kernels and then hands every
# finished tensor to its leaf parameter itself: p.grad = g, or p.grad += g when a gradient is already there.  Strong
# references to operands, partial rows and results are held until then.
#
# Everything a backward pass postpones to its end lives in ONE object, a _Pass: the queues, autograd's graph-task id of the
# pass that owns them, the side streams the pass has forked launches onto and the tensors those launches still use.  The
# module has one current pass (_pass) and a stack of suspended outer ones (_suspended, see nested_backward).  Final callbacks
# are dropped when backward raises, so a pass that finds another task id's leftovers discards them (stale device addresses:
# reset_deferred, which first waits for the side streams of the dead pass) and registers its own callback.  A new kind of
# per-pass state is a new field of _Pass -- reset, suspension and the flush need no word about it.
#
# What outlives a pass stays at module level: the streams and host tables (expensive to create, and a captured graph replays
# copies out of the tables' buffers), the cached launch plans, the previous pass's 192 x 384 count, the gradient targets.
DEFER_REDUCTIONS = os.environ.get("CSTS_DEFER_REDUCE", "1") != "0"


class _Pass:
    """The deferred work of ONE backward pass."""

    def __init__(self, lane=None):
        self.lane = lane        # None at top level; inside nested_backward the lane label of the inner pass (selects its host tables)
        self.task = -1          # graph-task id the queues belong to (-1: none)
        self.deferred = []      # (ws tensor, out tensor, nrows, ncols)
        self.assign = []        # (leaf parameter, finished gradient tensor)
        self.wgq = []           # (dY, X, dW, db, tokens, N_out, K_in)
        self.wg_prod = {}       # raw stream id -> torch stream that produced operands queued since the last flush
        self.w8_count = 0       # 192 x 384-class problems queued so far
        self.swq = []           # (DwconvGeom copy, fine ptr, coarse ptr, workspace ptr, dt, (tensors kept alive))
        self.forked = []        # side streams with launches of this pass in flight, in fork order
        self.keep = []          # what those launches read / write, alive until the streams are joined


_pass = _Pass()
_suspended = []         # the outer passes set aside by nested_backward, innermost last
_w8_total = [0]         # 192 x 384-class problems of the whole PREVIOUS pass: tells this one which problem is its last
_side_streams = {}      # (role, device index) -> stream: created once, the captured steps name them
_tables = {}            # (kind, _table_key) -> HostTable: pinned rings and device buffers, created once per device and lane


def reset_deferred():
    """Drop everything queued for an end-of-backward flush (used when a backward pass died before its final callback)."""
    global _pass
    for st in _pass.forked:             # a dead pass may have launches in flight that read / write what is dropped below
        st.synchronize()
    _pass = _Pass(_pass.lane)


# A backward pass that starts INSIDE a backward pass (an activation-checkpointed block re-runs its forward and back-propagates
# through the fresh sub-graph from its own backward: CheckpointFn) is a graph task of its own.  Its queues must not be mixed
# with the outer pass's, and the outer pass's must not be taken for a dead pass's leftovers.  nested_backward() is the scope of
# such an inner pass: it sets the outer pass aside, the inner pass queues into a fresh one and its own final callback finishes
# that -- its weight gradients, reductions and hand-overs are complete, and its operands released, when the inner
# torch.autograd.backward returns -- and the outer pass comes back untouched.
@contextlib.contextmanager
def nested_backward(lane=0):
    """Scope of a backward pass run from inside another pass's node (torch.autograd.backward in a Function's backward): the
    outer pass's deferred work is set aside and comes back untouched; everything the inner pass defers is finished by the inner
    pass's own final callback, on the stream the inner pass was started from, before the scope ends.  lane: a small label for
    that stream -- inner passes that may run concurrently on different streams (the video and the audio trunk) need different
    lanes, because a lane owns the device tables its finishing launches read."""
    global _pass
    _suspended.append(_pass)
    _pass = _Pass(lane)
    try:
        yield
    finally:
        reset_deferred()                # the inner pass raised before its final callback ran: its leftovers go, the outer queue stays
        _pass = _suspended.pop()


def _table_key(dev_index, *extra):
    """Key of a flush's host -> device table: per device at top level (as ever), per (device, lane) inside a nested pass -- a
    nested flush on the audio stream must not overwrite the table a nested flush on the main stream is still reading."""
    lane = _pass.lane
    key = (dev_index,) + extra if extra else dev_index
    return key if lane is None else ("nested", lane, key)


# host tables of nested flushes: one block's work per upload, one upload per checkpointed block and capture
_NESTED_CAPTURES = 32


def _host_table(kind, dev, nbytes, ring, captures, *extra):
    """The HostTable of this flush: one per kind ("reduce", "wgrad", "stencil"), device, lane and `extra`, created on first use.
    captures: the capture buffers of a top-level table (a nested pass's table has _NESTED_CAPTURES)."""
    key = (kind, _table_key(dev.index, *extra))
    tab = _tables.get(key)
    if tab is None:
        tab = _tables[key] = HostTable(nbytes, dev, ring=ring, captures=captures if _pass.lane is None else _NESTED_CAPTURES)
    return tab


def _fork(role, device, producers):
    """The side stream `role` ("early", "tail") of `device`, waiting for everything enqueued so far on the `producers` streams
    (autograd runs every node of a device on ONE thread: whatever produced the operands is already enqueued there), and
    recorded as forked by the current pass: _join makes the pass's stream wait for it, reset_deferred the host."""
    st = _side_streams.get((role, device.index))
    if st is None:
        st = _side_streams[(role, device.index)] = torch.cuda.Stream(device=device)
    for p_ in producers:
        st.wait_stream(p_)
    if st not in _pass.forked:
        _pass.forked.append(st)
    return st


def _join():
    """Make the current stream wait for every side stream this pass forked (the last forked first), then release what the
    launches there were using."""
    if _pass.forked:
        cur = torch.cuda.current_stream()
        for st in reversed(_pass.forked):
            cur.wait_stream(st)
        _pass.forked.clear()
    _pass.keep.clear()


def _can_defer(*params) -> bool:
    """True when the caller may leave its gradient for the end-of-backward flush: inside a backward pass, and every
    given parameter is a leaf the flush can assign to (None entries are ignored)."""
    if not DEFER_REDUCTIONS:
        return False
    for p_ in params:
        if p_ is not None and not (p_.is_leaf and p_.requires_grad):
            return False
    tid = torch._C._current_graph_task_id()
    if tid < 0:                        # not inside a backward pass
        return False
    if _pass.task != tid:
        reset_deferred()               # leftovers of a pass that raised before its callback ran
        torch.autograd.Variable._execution_engine.queue_callback(flush_deferred)
        _pass.task = tid
    return True


def _defer(ws: torch.Tensor, out: torch.Tensor, nrows: int, ncols: int):
    _pass.deferred.append((ws, out, int(nrows), int(ncols)))


# Gradient targets (csts_amd.train.SegmentedTrainStep, data-parallel chain): parameter storage address -> a view of a flat
# all-reduce bucket shaped like the parameter.  A producer that allocates a parameter gradient (queued Linear weight gradients,
# the fusion convs' TN GEMM) writes it THERE, so the bucket needs no copy afterwards.  One use per backward pass: a second
# gradient for the same parameter (a module applied twice) gets an ordinary buffer and is accumulated as before.
# (Module level: the targets are set once per step object, and a bucket view stays single-use across the nested passes of the
# outer pass -- _hand_over of the OUTER pass frees them.)
_grad_targets = {}
_grad_targets_used = set()


def set_grad_targets(pairs=None):
    _grad_targets.clear()
    _grad_targets_used.clear()
    for p_, v_ in (pairs or []):
        if v_.dtype == torch.float32 and v_.is_contiguous() and v_.numel() == p_.numel():
            _grad_targets[p_.data_ptr()] = v_


def _grad_buffer(param_like, shape, device):
    """fp32 buffer for the gradient of `param_like` (a Parameter or a saved alias of it): its bucket view if one is registered,
    unused in this backward pass and the parameter has no gradient yet; else a fresh tensor."""
    key = param_like.data_ptr()
    v = _grad_targets.get(key)
    if v is not None and key not in _grad_targets_used and getattr(param_like, "grad", None) is None and v.device == device:
        _grad_targets_used.add(key)
        return v.view(shape)
    return torch.empty(shape, dtype=torch.float32, device=device)


def _assign_later(param, grad):
    if param is not None and grad is not None:
        _pass.assign.append((param, grad))


def _hand_over():
    """Give the finished gradients to their parameters (stream-ordered after the finishing kernels)."""
    for p_, g_ in _pass.assign:
        if p_.grad is None:
            p_.grad = g_ if g_.dtype == p_.dtype else g_.to(p_.dtype)
        else:
            p_.grad.add_(g_)
    _pass.assign.clear()
    if _pass.lane is None:              # a nested pass ends in the middle of the outer one: the bucket views stay single-use until that ends
        _grad_targets_used.clear()


def flush_deferred():
    """Finish the queued weight gradients and every deferred reduction on the current stream, then hand the results to
    their parameters (idempotent)."""
    ps = _pass
    ps.task = -1
    nested = ps.lane is not None
    if ps.w8_count and not nested:
        _w8_total[0] = ps.w8_count
    ps.w8_count = 0
    # the grouped stencil weight gradients (0.8 ms of load-latency-bound work, no matrix math) run on a side stream BESIDE the
    # grouped Linear weight gradients (MFMA-bound, one persistent workgroup per CU whose last items leave most CUs idle)
    # (a nested pass finishes ONE block: its two or three pools stay on the pass's own stream -- a fork / join pair per block would
    # cost more in the captured graph than the overlap returns, and the audio trunk's blocks already run beside the video trunk's)
    if ps.swq and ps.wgq and STENCIL_TAIL_SIDE and ps.swq[0][5][0].is_cuda and not nested:
        cur = torch.cuda.current_stream()
        with torch.cuda.stream(_fork("tail", cur.device, [cur])):
            ps.keep.append(flush_stencil_wgrads())      # allocated on this stream, read on the tail stream: alive until the join
        flush_wgrads()
    else:
        flush_wgrads()
        flush_stencil_wgrads()
    _join()
    if not ps.deferred:
        _hand_over()
        return
    # wide & shallow (split-K slabs) after narrow & deep (LayerNorm / stencil partial rows): two kernels
    wide = lambda it: it[3] >= 8192 and it[3] % 4 == 0 and it[2] <= 64
    items = sorted(ps.deferred, key=lambda it: (wide(it), it[3]))
    ps.deferred.clear()
    tab = _host_table("reduce", items[0][0].device, C.sizeof(L.ReduceDesc) * 2048, 4, 16)
    # one launch per size class (the grid is sized by the widest reduction of the launch)
    descs = (L.ReduceDesc * len(items))()
    for i, (ws, out, nrows, ncols) in enumerate(items):
        descs[i].ws, descs[i].out = ws.data_ptr(), out.data_ptr()
        descs[i].nrows, descs[i].ncols, descs[i].scale = nrows, ncols, 1.0
    raw = bytes(descs)
    sz = C.sizeof(L.ReduceDesc)
    if len(items) > 2048:
        raise L.CstsError("too many deferred reductions in one backward pass")
    base = tab.upload(raw)
    lo = 0
    while lo < len(items):
        hi = lo + 1
        w = wide(items[lo])
        while hi < len(items) and wide(items[hi]) == w and items[hi][3] <= (64 if w else 4) * items[lo][3]:
            hi += 1
        fn = _lib().csts_reduce_rows_wide if w else _lib().csts_reduce_rows_batched
        L.check(fn(base + lo * sz, hi - lo, items[hi - 1][3], _stream()), "csts_reduce_rows_batched")
        lo = hi
    del items
    _hand_over()


# Weight gradients of the Linear layers (dW = dY^T X) are off the critical path of backward: inside a backward pass they
# are queued and computed by csts_wgrad_grouped at the end, all layers in one launch per dY dtype.  A weight gradient on
# its own needs a deep split-K to fill the chip; together they provide thousands of (tile, token-chunk) work items, so
# chunks are long (WGRAD_CHUNK tokens) and most layers need no split-K partials at all.
# "capture" (default): only while the step is being captured into a HIP graph -- replayed, the grouped tail costs nothing
# on the host and the graph's private pool makes the longer tensor lifetimes free.  In eager mode the end-of-backward
# release of every queued operand at once fragments torch's caching allocator (hipMalloc stalls of ~20 ms in the next
# forward were measured), so eager steps keep the in-line split-K weight gradients unless CSTS_GROUP_WGRADS=1 forces
# grouping; CSTS_GROUP_WGRADS=0 switches it off everywhere.
GROUP_WGRADS = {"0": "never", "1": "always"}.get(os.environ.get("CSTS_GROUP_WGRADS", ""), "capture")
# 192 x 384 tiles on 8-wave workgroups (wgrad8.hip: half the operand bytes per FLOP, k-tiles by LDS-DMA into a 2-stage ring,
# no ds_write phase) for the layers they divide (the 384- and 768-channel stages).  Measured on MI355X
# (profiles/r2_wgrad8_ab.txt): the register-staged first version 1541 us against the 1497-1565 us those layers cost as
# 128 x 128 / 256 x 128 items (neutral); the LDS-DMA version 1472 us (-6 %), 24.38-24.42 vs 24.37-24.48 ms per step over three
# interleaved pairs.  On by default; CSTS_WGRAD8=0 is the A/B switch.  Token chunk: 8192 (4096 / 2048 measured +0.05 / +0.15 ms).
WGRAD8 = os.environ.get("CSTS_WGRAD8", "1") != "0"
WGRAD8_CHUNK = int(os.environ.get("CSTS_WGRAD8_CHUNK", "8192"))
# Round 5: the thin layers (output and input features multiples of 96 that the 192 x 384 class does not take; bf16 dY) as 96 x 96 tiles, one
# (tile, token chunk) item per WAVE of csts_wgrad_grouped5 (wgrad5.hip: every wave its own LDS-DMA stream, no workgroup barrier)
WG_DUMP = os.environ.get("CSTS_WGRAD_DUMP", "")
WGRAD5 = os.environ.get("CSTS_WGRAD5", "1") != "0"
WGRAD5_CHUNK = int(os.environ.get("CSTS_WGRAD5_CHUNK", "4096"))
WGRAD5_STRIDED = os.environ.get("CSTS_WGRAD5_STRIDED", "1") != "0"
WGRAD5_MIN = int(os.environ.get("CSTS_WGRAD5_MIN", "96"))          # layers with min(N, K) below this stay on the 128-wide classes
# first: beside the stencil weight gradients; mid (default): after the 128-wide classes -- the stencil launch then starts beside the fp32-dY class
# and the remaining 128-wide items (wgrad5 and the stencil kernel side by side take the SUM of their times: profiles/r5_wgrad5.txt)
WGRAD5_POS = os.environ.get("CSTS_WGRAD5_POS", "mid")
WGRAD_CHUNK = int(os.environ.get("CSTS_WGRAD_CHUNK", "8192"))   # tokens per work item (measured per step: 4096 -> 24.93 ms, 8192 -> 24.95, 16384 -> 25.47)
WG_STATS = None         # a list while bench.py instruments a step: (C-ABI entry, algorithmic bytes, flop) per grouped launch
# WGRAD8_LAST (with CSTS_STENCIL_TAIL_SIDE=1): the 192 x 384 class -- one 144 KB-LDS workgroup per CU, nothing fits beside it -- goes
# last, so that the grouped stencil weight gradients on the side stream (vector-bound, 20 KB of LDS, 124 registers) start beside the
# 128-wide classes (memory-bound, 40 KB of LDS, 154 registers), which they CAN share a CU with: -0.2 ... -0.26 ms per step
# (profiles/r5_wgrad_tail_ab.txt).  The same side stream was neutral in round 4 only because that class went first.  =0 restores either.
WGRAD8_LAST = os.environ.get("CSTS_WGRAD8_LAST", "1") != "0"
STENCIL_TAIL_SIDE = os.environ.get("CSTS_STENCIL_TAIL_SIDE", "1") != "0"
# Round 5 (CSTS_WGRAD8_EARLY_WGS = n > 0): the grouped weight gradients of the 384- / 768-channel stages (wgrad8: matrix-bound, 1.1 ms, one
# 144 KB-LDS workgroup per CU) are launched on n workgroups on the side stream as soon as the backward pass has produced their last operand
# -- the rest of backward (the 96- / 192-channel stages: large-M, memory-bound kernels, a third of the trunk backward) runs beside them on
# the remaining CUs -- instead of on all CUs after the pass (profiles/r5_wgrad8_early_ab.txt).
W8_EARLY_WGS = int(os.environ.get("CSTS_WGRAD8_EARLY_WGS", "0"))
# Retired experiments (measured slower or neutral: DESIGN.md, "Retired switches"): the code and the environment variables are gone;
# the names stay as inert constants for callers that set them back to their defaults.  Nothing reads them.
WG_FLUSH_FLOP, W8_PARALLEL, WGRAD_CAST_F32 = 0.0, False, False

# The tile classes of a grouped launch, one row each: tile rows x columns (output x input features), the module attribute that
# holds its tokens per work item (read at call time), the token granule its k-loop needs, whether its items may interleave
# 16-token stages (WGRAD5_STRIDED), the C-ABI entry (also its name in WG_STATS) and that entry's arguments between the item
# count and the stream.  192 x 384 on 8-wave workgroups where it divides the layer (the 384- and 768-channel stages: half the
# operand bytes per FLOP of a 128 x 128 tile); 96 x 96 per wave for the thin layers; else 256 x 128 where 256 divides the output
# rows; else 128 x 128.  fp32 dY (a handful per step: the stage-transition projections, whose output gradient has no 16-bit
# copy) is always 128 x 128: the kernel rounds it to the 16-bit type while staging.
_WgClass = collections.namedtuple("_WgClass", "name rows cols chunk granule strided entry args")
_WG_CLASSES = {c.name: c for c in (
    _WgClass("192", 192, 384, "WGRAD8_CHUNK", 64, False, "csts_wgrad_grouped8", ()),
    _WgClass("96", 96, 96, "WGRAD5_CHUNK", 16, True, "csts_wgrad_grouped5", ()),
    _WgClass("256", 256, 128, "WGRAD_CHUNK", 1, False, "csts_wgrad_grouped", (0, 256)),
    _WgClass("128", 128, 128, "WGRAD_CHUNK", 1, False, "csts_wgrad_grouped", (0, 128)),
    _WgClass("128f", 128, 128, "WGRAD_CHUNK", 1, False, "csts_wgrad_grouped", (1, 128)),
)}


def _wg_class(dy_is_f32, tokens, N, K):
    """The tile class of the problem dW[N, K] = dY[tokens, N]^T X[tokens, K] under the current switches."""
    if dy_is_f32:
        return _WG_CLASSES["128f"]
    for name, on in (("192", WGRAD8), ("96", WGRAD5 and min(N, K) >= WGRAD5_MIN)):
        c = _WG_CLASSES[name]
        if on and N % c.rows == 0 and K % c.cols == 0 and tokens % c.granule == 0 and globals()[c.chunk] % c.granule == 0:
            return c
    return _WG_CLASSES["256" if N % 256 == 0 else "128"]


def queue_wgrad(dY, X, tokens, N, K, Wp, bp):
    """Queue dW[N,K] = dY[tokens,N]^T X[tokens,K] (+ db[N] when bp is given) for the grouped launch at the end of this
    backward pass, which also hands the results to the leaf parameters Wp / bp (see the note on deferred gradients
    above).  Returns False when the problem has to run in line."""
    if GROUP_WGRADS == "never" or (GROUP_WGRADS == "capture" and not torch.cuda.is_current_stream_capturing()):
        return False
    if not (DEFER_REDUCTIONS and X.dtype == L.half_dtype() and dY.dtype in (torch.float32, L.half_dtype())
            and N % 8 == 0 and K % 8 == 0 and dY.is_contiguous() and X.is_contiguous() and tokens >= 256):
        return False
    if Wp is None or Wp.dtype != torch.float32 or tuple(Wp.shape) != (N, K) or not _can_defer(Wp, bp):
        return False
    dW = _grad_buffer(Wp, (N, K), dY.device)
    db = _grad_buffer(bp, (N,), dY.device) if bp is not None else None
    _pass.wgq.append((dY, X, dW, db, tokens, N, K))
    _assign_later(Wp, dW)
    _assign_later(bp, db)
    cur = torch.cuda.current_stream()
    _pass.wg_prod[cur.cuda_stream] = cur
    if W8_EARLY_WGS > 0 and _wg_class(dY.dtype == torch.float32, tokens, N, K).name == "192":
        # the 192 x 384 class goes out EARLY, on few workgroups, as soon as its last problem of this backward pass is queued (the count
        # of the previous pass tells which one that is; a wrong guess only moves work between this launch and the final one)
        _pass.w8_count += 1
        if _pass.w8_count == _w8_total[0]:
            flush_wgrads(only_w8=True)
    return True


_WG_DTYPE = None
_wg_plans = {}          # (tuple of (tokens, N, K) per problem, class geometry) -> cached work-item layout: a function of shapes alone


def _wg_dtype():
    global _WG_DTYPE
    if _WG_DTYPE is None:
        import numpy as np
        _WG_DTYPE = np.dtype([("A", "u8"), ("B", "u8"), ("C", "u8"), ("colsum", "u8"), ("lda", "i8"), ("ldb", "i8"), ("ldc", "i8"),
                              ("kbeg", "i8"), ("kend", "i8"), ("M", "i4"), ("N", "i4"), ("m0", "i4"), ("n0", "i4")], align=True)
        assert _WG_DTYPE.itemsize == C.sizeof(L.WgradItem)
    return _WG_DTYPE


def _wg_plan(sig, rows=128, cols=128, chunk_tokens=None, strided=False):
    """Work-item layout of one grouped launch for the problem list `sig` = ((tokens, N, K), ...): everything except the
    device addresses, which change from step to step.  Cached: building ~7000 items in Python costs ~15 ms.

    Workgroups are dealt round-robin over the 8 XCDs (block b -> XCD b % 8), each with its own L2: the tiles of one
    (layer, token chunk) go to ONE XCD, these groups are spread over the XCDs by load (long chunks first), and XCD x's list
    is laid out at positions x, x + 8, x + 16, ... (rocprofv3: 7x the algorithmic HBM bytes when consecutive tiles landed
    on different XCDs).  Padding slots keep A == NULL (the kernel skips them)."""
    import numpy as np
    CH = chunk_tokens or WGRAD_CHUNK
    plan = _wg_plans.get((sig, rows, cols, CH, strided))
    if plan is not None:
        return plan
    # (Cutting the layers with the fewest tiles into half-length chunks, so that the 192 x 384 class's 310 full-length items
    # of the b=4 step do not leave 54 of them for a second, almost empty round on 256 CUs, was measured: kernel 1335 ->
    # 1276 us, step unchanged -- the partial slabs and their reduction cost what the balance returns.)
    CHs = [CH] * len(sig)
    groups = []
    for pi, (tokens, N, K) in enumerate(sig):
        CHp = CHs[pi]
        nch = -(-tokens // CHp)
        for c in range(nch):
            kb, ke = c * CHp, min(tokens, (c + 1) * CHp)
            if strided:
                # csts_wgrad_grouped5: the nch items of a tile INTERLEAVE 16-token stages (item c takes stages c, c + nch, ...: kbeg = its
                # first stage, kend = the layer's tokens, M = the stage stride) -- the waves that work on one layer then read ONE moving
                # window of its token rows instead of nch distant ranges (2048 wave streams of 3 KB bursts: 3.0 TB/s, tools/wgrad5_bench.py)
                nst = -(-tokens // 16)
                groups.append([(16 * len(range(c, nst, nch)), pi, c, 16 * c, tokens, m0, n0, nch) for m0 in range(0, N, rows) for n0 in range(0, K, cols)])
                continue
            # one group = ALL tiles of this (layer, token chunk): they run together on one XCD and stream the same
            # token range in near lockstep, so its L2 serves every dY / X panel slice to all the tiles that share it
            # (grouping by tile-row only reused the dY panel: rocprofv3 still counted 18.6 GB per launch)
            groups.append([(ke - kb, pi, c, kb, ke, m0, n0, 0) for m0 in range(0, N, rows) for n0 in range(0, K, cols)])
    # two levels of longest-first: groups go to the least-loaded XCD in order of their total work; inside an XCD's list the
    # groups with the longest ITEMS start first (a 8192-token item runs 4 x as long as a 2048-token one: started last it
    # is the tail of the launch, with most CUs idle -- 1448 -> 1317 us for the 192 x 384 class of the b=4 step)
    groups.sort(key=lambda g_: -g_[0][0] * len(g_))
    glists, load = [[] for _ in range(8)], [0] * 8
    for g_ in groups:
        x = load.index(min(load))
        glists[x].append(g_)
        load[x] += g_[0][0] * len(g_)
    lists = []
    for gl in glists:
        gl.sort(key=lambda g_: -g_[0][0])          # stable: equal item lengths keep the by-work order
        lists.append([it for g_ in gl for it in g_])
    depth = max(len(l_) for l_ in lists)
    n_items = depth * 8
    if n_items > 16384:
        raise L.CstsError("too many grouped weight-gradient work items")
    tmpl = np.zeros(n_items, dtype=_wg_dtype())
    pidx = np.full(n_items, -1, dtype=np.int64)
    chunk = np.zeros(n_items, dtype=np.int64)
    for x in range(8):
        for slot, (_, pi, c, kb, ke, m0, n0, stride) in enumerate(lists[x]):
            i = slot * 8 + x
            tokens, N, K = sig[pi]
            tmpl[i] = (0, 0, 0, 0, N, K, K, kb, ke, stride if rows == 96 else N, K, m0, n0)     # 96 x 96 per-wave class: M carries the stage step
            pidx[i], chunk[i] = pi, c
    valid = pidx >= 0
    plan = _wg_plans[(sig, rows, cols, CH, strided)] = (tmpl, valid, pidx[valid], chunk[valid], n_items, CHs)
    return plan


def flush_wgrads(only_w8: bool = False):
    """Launch the queued weight gradients on the current stream (end of backward).  only_w8 (from queue_wgrad, in the middle of
    backward): just the 192 x 384-class problems, on W8_EARLY_WGS workgroups on the "early" side stream, after everything the
    producing streams have enqueued so far; everything else stays queued."""
    ps = _pass
    if not ps.wgq:
        return
    import numpy as np
    q = [(t, _wg_class(t[0].dtype == torch.float32, t[4], t[5], t[6])) for t in ps.wgq]
    ps.wgq.clear()
    if only_w8:
        ps.wgq.extend(t for t, c in q if c.name != "192")
        q = [(t, c) for t, c in q if c.name == "192"]
        if not q:
            return
    if WG_DUMP and not os.path.exists(WG_DUMP):      # diagnostics: the problem list of one flush, for tools/wgrad5_bench.py
        with open(WG_DUMP, "w") as f:
            for t, _ in q:
                f.write(f"{'f32' if t[0].dtype == torch.float32 else 'h16'} {t[4]} {t[5]} {t[6]} {t[0].stride(0)} {t[1].stride(0)} {int(t[3] is not None)}\n")
    dev = q[0][0][0].device
    # (the early launch runs on the side stream CONCURRENTLY with launches of the main stream: its own device table -- one table for two
    # streams let the second upload overwrite the items the first launch was still reading: a GPU memory fault, round 5.  A nested
    # pass uploads one block's items at a time: a single tile class is capped at 16384 items)
    tab = _host_table("wgrad", dev, C.sizeof(L.WgradItem) * (24576 if ps.lane is None else 16384), 8, 40 if only_w8 else 16, only_w8)
    launch_stream = _fork("early", dev, ps.wg_prod.values()) if only_w8 else None
    ps.wg_prod.clear()
    pend = []           # (item table image, items, tile class) per tile class
    order = ("96", "256", "128", "128f", "192") if WGRAD8_LAST else ("192", "96", "256", "128", "128f")
    if WGRAD8_LAST and WGRAD5_POS == "mid":
        order = ("256", "128", "128f", "96", "192")
    for c in (_WG_CLASSES[name] for name in order):
        probs = [t for t, c_ in q if c_ is c]
        if not probs:
            continue
        tmpl, valid, pidx, chunk, n_items, CHs = _wg_plan(tuple((t[4], t[5], t[6]) for t in probs), c.rows, c.cols, globals()[c.chunk],
                                                          strided=c.strided and WGRAD5_STRIDED)
        A = np.empty(len(probs), dtype=np.uint64); B = np.empty_like(A); Cb = np.empty_like(A); Cs = np.zeros_like(A)
        cstride = np.zeros(len(probs), dtype=np.uint64); sstride = np.zeros_like(cstride)
        for i, (dY, X, dW, db, tokens, N, K) in enumerate(probs):
            A[i], B[i] = dY.data_ptr(), X.data_ptr()
            nch = -(-tokens // CHs[i])
            if nch == 1:
                Cb[i], Cs[i] = dW.data_ptr(), (db.data_ptr() if db is not None else 0)
            else:          # several token chunks: one partial slab per chunk, summed by the batched reducer (which keeps the slabs alive)
                slab = torch.empty(nch, N, K, dtype=torch.float32, device=dev)
                _defer(slab, dW, nch, N * K)
                Cb[i], cstride[i] = slab.data_ptr(), N * K * 4
                if db is not None:
                    cs = torch.empty(nch, N, dtype=torch.float32, device=dev)
                    _defer(cs, db, nch, N)
                    Cs[i], sstride[i] = cs.data_ptr(), N * 4
        arr = tmpl.copy()
        ch = chunk.astype(np.uint64)
        arr["A"][valid] = A[pidx]
        arr["B"][valid] = B[pidx]
        arr["C"][valid] = Cb[pidx] + ch * cstride[pidx]
        arr["colsum"][valid] = Cs[pidx] + ch * sstride[pidx]
        if WG_STATS is not None:      # dY + X read once, dW written once; 2 tokens N K flop
            WG_STATS.append((c.entry, sum(t[4] * t[5] * t[0].element_size() + t[4] * t[6] * 2 + t[5] * t[6] * 4 for t in probs),
                             sum(2.0 * t[4] * t[5] * t[6] for t in probs)))
        pend.append((arr.tobytes(), n_items, c))
    # the item tables of all tile classes travel in ONE host -> device copy (a copy node per class cost ~12 us each in the replayed
    # step, gap included); one copy per class only when they do not fit the table together
    with (torch.cuda.stream(launch_stream) if launch_stream is not None else contextlib.nullcontext()):
        offs, total = [], 0
        for blob, *_ in pend:
            offs.append(total)
            total += (len(blob) + 255) // 256 * 256
        base = None
        if pend and total <= tab.nbytes:
            base = tab.upload(b"".join(blob + bytes((-len(blob)) % 256) for blob, *_ in pend))
        for (blob, n_items, c), off in zip(pend, offs):
            ptr = base + off if base is not None else tab.upload(blob)
            entry, args = ("csts_wgrad_grouped8_limited", (W8_EARLY_WGS,)) if only_w8 else (c.entry, c.args)
            L.check(getattr(_lib(), entry)(ptr, n_items, *args, _stream()), entry)
    if only_w8:
        ps.keep.append(q)       # the operands, alive until the final callback has joined the side stream


# Stencil weight gradients, grouped (csts_dwconv_wgrad_grouped): 34 first-stage launches of ~24 us per step -- each a single round
# of <= 1024 latency-bound workgroups -- become ONE launch at the end of backward (their second stages were deferred already).
# Same policy as the grouped Linear weight gradients: while the step is captured (GROUP_WGRADS), and only when the gradient may be
# deferred; the operands (the saved q / k / v tensors and the conv-output gradients) stay alive until the flush.  With
# STENCIL_TAIL_SIDE that launch (vector-issue-bound, 20 KB of LDS, 124 registers) runs on the "tail" side stream beside the 128-wide
# classes of the grouped Linear weight gradients (flush_deferred).
STENCIL_WGRAD_GROUPED = os.environ.get("CSTS_STENCIL_WGRAD_GROUPED", "1") != "0"


def _stencil_group_now() -> bool:
    return STENCIL_WGRAD_GROUPED and GROUP_WGRADS != "never" and (GROUP_WGRADS == "always" or torch.cuda.is_current_stream_capturing())


def _queue_stencil_wgrad(g, fine, fine_off, coarse, coarse_off, ws):
    """One csts_dwconv_wgrad problem for the grouped launch of flush_stencil_wgrads (first stage only: the caller defers the row sums
    of `ws` itself)."""
    gg = L.DwconvGeom()
    C.memmove(C.byref(gg), C.byref(g), C.sizeof(L.DwconvGeom))
    _pass.swq.append((gg, _p(fine, fine_off), _p(coarse, coarse_off), _p(ws), _dt(fine), (fine, coarse, ws)))


def flush_stencil_wgrads():
    if not _pass.swq:
        return None
    q = list(_pass.swq)
    _pass.swq.clear()
    tab = _host_table("stencil", q[0][5][0].device, L.DWCONV_WGRAD_TABLE_ENTRY * 256, 4, 16)
    for dt in sorted({e[4] for e in q}):
        sel = [e for e in q if e[4] == dt]
        if len(sel) > 256:
            raise L.CstsError("too many grouped stencil weight gradients")
        items = (L.DwconvWgradItem * len(sel))()
        for i, (gg, fp, cp, wp, _, _) in enumerate(sel):
            items[i].geom, items[i].fine, items[i].coarse, items[i].workspace = gg, fp, cp, wp
        image = (C.c_uint8 * (L.DWCONV_WGRAD_TABLE_ENTRY * len(sel)))()
        nblocks = C.c_int(0)
        L.check(_lib().csts_dwconv_wgrad_grouped_plan(items, len(sel), image, len(image), C.byref(nblocks)), "csts_dwconv_wgrad_grouped_plan")
        ptr = tab.upload(bytes(image))
        if WG_STATS is not None:          # fine + coarse read once; 2 x 27 flop per coarse cell and channel
            esz = 4 if dt == F32 else 2
            cells = lambda gg: (gg.B * gg.Tf * gg.Hf * gg.Wf, gg.B * gg.Tc * gg.Hc * gg.Wc)
            WG_STATS.append(("csts_dwconv_wgrad_grouped", sum(sum(cells(e[0])) * e[0].C * esz for e in sel),
                             sum(54.0 * cells(e[0])[1] * e[0].C for e in sel)))
        L.check(_lib().csts_dwconv_wgrad_grouped(ptr, len(sel), nblocks.value, dt, _stream()), "csts_dwconv_wgrad_grouped")
    return q            # the operands: the caller keeps them alive until the launch stream has been joined


# ----------------------------------------------------------------------------------------- raw wrappers
AUTO_SPLIT_SMALL_M = True
MID_M_SPLIT = int(os.environ.get("CSTS_MID_M_SPLIT", "1"))


def _auto_split(layout, M, N, K, compute):
    """Deterministic split-K for activation GEMMs with a handful of rows (embedding projections and similarity matrices
    of the EgoNCE loss: M = batch; the temporal-fusion block: M = B*2T'): one or two row tiles leave 1..24 workgroups
    walking the whole K serially (55-100 us per call measured); slabs + the finishing pass spread K over the chip."""
    if layout != L.GEMM_TN and compute == BF16 and MID_M_SPLIT > 1 and 1024 <= M <= 4096 and K >= 2304 and N <= 1024:
        # the 768-channel stage at b = 4 (M = 2048 tokens): fc2 / the qkv data gradient are 64-96 output tiles on 256 CUs with a
        # 36-48 step k-loop each -- cut the loop so that every CU has a tile (deterministic slabs + finishing pass)
        return MID_M_SPLIT
    if layout == L.GEMM_TN or M > 128:
        return 1
    ksteps = -(-K // (64 if compute == BF16 else 32))
    tiles = -(-M // 64) * -(-N // 128)
    split = min(ksteps // (4 if compute == BF16 else 2), -(-192 // tiles))
    return split if split >= 2 else 1


def gemm(layout, A, a_off, lda, B, b_off, ldb, Cm, ldc, M, N, K, *, compute, bias=None, epilogue=L.EPI_NONE, aux=None,
         residual=None, ldr=0, res_row_mod=0, row_scale=None, rows_per_scale=1, split_k=1, deterministic=True, tile_rows=0,
         want_colsum=False, algo=0, debug_ws=None, res_up=None):
    """res_up = (coarse thw, fine thw): `residual` is the coarse token grid and the epilogue adds its trilinear up-sampling
    (csts_gemm_args.res_up)."""
    if split_k == 1 and AUTO_SPLIT_SMALL_M and not want_colsum and algo == 0 and tile_rows == 0 and res_up is None:
        split_k = _auto_split(layout, M, N, K, compute)
    a = L.GemmArgs()
    a.layout = layout
    a.A, a.a_dt, a.lda = _p(A, a_off), _dt(A), lda
    a.B, a.b_dt, a.ldb = _p(B, b_off), _dt(B), ldb
    a.C, a.c_dt, a.ldc = _p(Cm), _dt(Cm), ldc
    a.M, a.N, a.K = M, N, K
    a.bias = _p(bias)
    a.epilogue = epilogue
    # GELU without a kept pre-activation (inference): aux_dt still names the activation dtype -- it selects the GELU flavour
    # (exact erf in fp32 mode, the 1.5e-7 polynomial in the 16-bit modes), which must not depend on whether h is kept
    a.aux, a.aux_dt, a.ldaux = _p(aux), (_dt(aux) if aux is not None else (_dt(Cm) if epilogue == L.EPI_GELU else 0)), (N if aux is not None else 0)
    a.residual, a.r_dt, a.ldr = _p(residual), (_dt(residual) if residual is not None else 0), ldr
    a.res_row_mod = res_row_mod
    a.row_scale, a.rows_per_scale = _p(row_scale), rows_per_scale
    a.compute, a.split_k = compute, split_k
    a.tile_rows = tile_rows
    a.algo = algo
    if res_up is not None:
        for i, v in enumerate(list(res_up[0]) + list(res_up[1])):
            a.res_up[i] = int(v)
    ws = None
    if debug_ws is not None:   # diagnostics builds only (gemm3 cycle stamps)
        a.workspace, a.ws_bytes = _p(debug_ws), debug_ws.numel() * debug_ws.element_size()
    if split_k > 1 and deterministic:
        nb = _lib().csts_gemm_splitk_workspace(M, N, K, split_k)
        if nb <= SPLITK_WS_LIMIT:
            ws = _ws(nb, Cm.device)
            a.workspace, a.ws_bytes = _p(ws), ws.numel()
    fused = None
    if want_colsum and (split_k == 1 or ws is not None) and _lib().csts_gemm_v2_eligible(C.byref(a)):
        fused = torch.empty(M, dtype=torch.float32, device=Cm.device)
        a.colsum = _p(fused)
    L.check(_lib().csts_gemm(C.byref(a), _stream()), "csts_gemm")
    return fused


def colsum(X: torch.Tensor, batch: int, M: int, N: int, row_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = torch.empty(batch * N, dtype=torch.float32, device=X.device)
    nbytes = _lib().csts_colsum_workspace(batch, M, N)
    ws = _ws(nbytes, X.device)
    L.check(_lib().csts_colsum(_p(X), _dt(X), _p(row_weight), _p(out), batch, M, N, _p(ws), ws.numel(), _stream()),
            "csts_colsum")
    return out


def scale_rows(x: torch.Tensor, row_scale: torch.Tensor, rows_per_scale: int, M: int, N: int, out_dt=None) -> torch.Tensor:
    out = torch.empty_like(x) if out_dt is None else torch.empty(x.shape, dtype=torch_dtype(out_dt), device=x.device)
    L.check(_lib().csts_scale_rows(_p(x), _dt(x), _p(row_scale), rows_per_scale, _p(out), _dt(out), M, N, _stream()),
            "csts_scale_rows")
    return out


SPLITK_WS_LIMIT = 256 << 20   # deterministic split-K slabs up to this size, atomics beyond


def _wgrad_split(M_out: int, N_out: int, Kred: int) -> int:
    tiles = math.ceil(M_out / 128) * math.ceil(N_out / 128)
    return max(1, min(512 // max(tiles, 1), math.ceil(Kred / 512)))


def _wgrad(dY: torch.Tensor, X: torch.Tensor, M: int, N: int, K: int, compute: int, want_bias: bool = False,
           params=None):
    """dW[N,K] = dY[M,N]^T X[M,K] (fp32, split over M); with want_bias also db[N] = colsum(dY), fused into the same
    kernel when the bf16 v2 GEMM applies.  params = (W, b) leaf parameters: inside a backward pass the problem may then be
    queued for the grouped end-of-backward launch, which assigns the gradients itself -- the return value is None (or
    (None, None)) in that case and the caller returns None to autograd for those inputs."""
    if compute == BF16 and params is not None:
        if queue_wgrad(dY, X, M, N, K, params[0], params[1] if want_bias else None):
            return (None, None) if want_bias else None
    split = _wgrad_split(N, K, M)
    det = split > 1 and _lib().csts_gemm_splitk_workspace(N, K, M, split) <= SPLITK_WS_LIMIT
    dW = (torch.zeros if (split > 1 and not det) else torch.empty)(N, K, dtype=torch.float32, device=dY.device)
    db = gemm(L.GEMM_TN, dY, 0, N, X, 0, K, dW, K, N, K, M, compute=compute, split_k=split, deterministic=det,
              want_colsum=want_bias)
    if want_bias:
        return dW, (db if db is not None else colsum(dY, 1, M, N))
    return dW


# ----------------------------------------------------------------------------------------- LayerNorm
BF16_GRAD_COPY = os.environ.get("CSTS_BF16_GRAD_COPY", "1") != "0"


def _ln_bwd_call(dy, x, gamma, mean, rstd, addend, rows, Cc, what, want16=False, params=None, copy_scale=None, dy2=None):
    """dx (+ addend) and the [2*C] dgamma|dbeta buffer.  params = (gamma, beta) leaf parameters: inside a backward pass
    the second stage is then deferred and the flush assigns the two halves itself -- the returned buffer is None.
    want16: also emit a bf16 copy of dx, attached as dx._csts_bf16, for the weight/data-gradient GEMMs that read it next
    (LinearFn / MlpFn backward pick it up; any other consumer simply ignores the attribute)."""
    dx = torch.empty_like(x)
    dx16 = torch.empty(x.shape, dtype=L.half_dtype(), device=x.device) if (want16 and BF16_GRAD_COPY) else None
    dgb = torch.empty(2 * Cc, dtype=torch.float32, device=x.device)
    nbytes = _lib().csts_layernorm_bwd_workspace(rows, Cc)
    ws = _ws(nbytes, x.device)
    defer = params is not None and _can_defer(*params)
    if dx16 is None or copy_scale is None or rows % copy_scale[1] != 0 or copy_scale[0].numel() * copy_scale[1] != rows:
        copy_scale = None
    cs, rps = (copy_scale[0], copy_scale[1]) if copy_scale is not None else (None, 1)
    L.check(_lib().csts_layernorm_bwd_ex(_p(dy), _p(dy2), _dt(dy), _p(x), _dt(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _dt(dx),
                                         _p(addend), _p(dx16), _p(cs), rps, None if defer else _p(dgb),
                                         None if defer else _p(dgb, Cc), _p(ws), ws.numel(), rows, Cc, _stream()), what)
    if defer:
        _defer(ws, dgb, nbytes // (2 * Cc * 4), 2 * Cc)
        _assign_later(params[0], dgb[:Cc])
        _assign_later(params[1], dgb[Cc:])
        dgb = None
    if dx16 is not None:
        _attach16(dx, dx16, copy_scale)
    return dx, dgb


def _scale_key(scale):
    """Identity of a (row_scale tensor, rows_per_scale) pair: saved tensors come back as new Python objects, so the storage
    address stands for the tensor."""
    if scale is None:
        return None
    return (scale[0].data_ptr(), scale[0].numel(), int(scale[1]))


def _attach16(dx: torch.Tensor, dx16: torch.Tensor, scale=None):
    """Remember the bf16 copy of the fp32 gradient `dx` on the tensor object, together with dx's version counter: autograd
    accumulates the gradients of a tensor with several consumers IN PLACE into the first one that arrives, which keeps
    the Python object (and this attribute) but bumps the version -- the copy is then stale and must not be used.
    scale = (row_scale, rows_per_scale): the copy holds dx times that per-sample scale (csts_layernorm_bwd_ex)."""
    dx._csts_bf16 = (dx16, dx._version, _scale_key(scale))


def _grad16(dy: torch.Tensor, compute: int, scale=None):
    """The bf16 copy of a residual-stream gradient left by the kernel that produced it (or None: no copy, `dy` was
    modified since the copy was made, or the copy was not made with the per-sample scale the caller needs)."""
    if compute != BF16 or dy.dtype != torch.float32:
        return None
    tag = getattr(dy, "_csts_bf16", None)
    if tag is None:
        return None
    d16, ver, key = tag
    if dy._version != ver or d16.shape != dy.shape or d16.device != dy.device or key != _scale_key(scale):
        return None
    return d16


def _mark_scaled_output(y, row_scale, rows_per_scale):
    """y = f(...) * row_scale + residual: remember the scale on the output tensor, so that the LayerNorm that reads y next can
    leave the bf16 copy of dL/dy already multiplied by it (LayerNormFn / _ln_bwd_call)."""
    if row_scale is not None and SCALED_GRAD_COPY:
        y._csts_prod_scale = (row_scale, int(rows_per_scale))
    return y


SCALED_GRAD_COPY = os.environ.get("CSTS_SCALED_GRAD_COPY", "1") != "0"


class LayerNormFn(Function):
    """nn.LayerNorm over the last dim (attention.py:192,214 eps 1e-6; :108,112,116 eps 1e-5).

    With ``passthrough`` the input is returned as a second output (an alias): the pre-norm residual pattern
    x + f(LN(x)) (attention.py:242,247) then hands BOTH gradients of x to this node, and the backward kernel writes
    dx = LN'(d_xn) + d_residual in one pass instead of leaving the sum to a separate autograd add."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float, out_dt: int, passthrough: bool, fanout: bool = False, addend=None):
        _need_gpu(x, gamma, beta)
        if passthrough and not x.is_contiguous():
            raise L.CstsError("layer_norm(passthrough=True) needs a contiguous input")
        x_in = x
        x = x.contiguous()
        Cc = x.shape[-1]
        rows = x.numel() // Cc
        y = torch.empty(x.shape, dtype=torch_dtype(out_dt), device=x.device)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        ctx.has_add = addend is not None
        if addend is not None:              # LN(x + addend); the sum (the new residual stream) is the pass-through output
            if not passthrough or addend.shape != x.shape or addend.dtype != x.dtype:
                raise L.CstsError("layer_norm(addend=...) needs passthrough=True and an addend like x")
            addend = addend.contiguous()
            xs = torch.empty_like(x)
            L.check(_lib().csts_layernorm_fwd_add(_p(x), _p(addend), _p(xs), _dt(x), _p(gamma), _p(beta), _p(y), out_dt, _p(mean),
                                                  _p(rstd), rows, Cc, eps, _stream()), "csts_layernorm_fwd_add")
            x = xs
        else:
            L.check(_lib().csts_layernorm_fwd(_p(x), _dt(x), _p(gamma), _p(beta), _p(y), out_dt, _p(mean), _p(rstd), rows, Cc,
                                              eps, _stream()), "csts_layernorm_fwd")
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.params = (gamma, beta)
        ctx.copy_scale = getattr(x_in, "_csts_prod_scale", None) if passthrough else None
        ctx.set_materialize_grads(False)
        ctx.fanout = bool(fanout)
        if fanout:                          # two aliases of y, one per consumer: backward receives both gradients
            if not passthrough:
                raise L.CstsError("layer_norm(fanout=True) comes with passthrough=True")
            return y, y.view_as(y), x
        if passthrough:
            return y, x
        return y

    @staticmethod
    def backward(ctx, dy, *rest):
        x, gamma, mean, rstd = ctx.saved_tensors
        dy2 = None
        if ctx.fanout:
            dy2, dpass = rest
            if dy is None:
                dy, dy2 = dy2, None
        else:
            dpass = rest[0] if rest else None
        nret = 8
        # LN(x + addend): x and the addend receive the same gradient (d(x + a)/dx = d(x + a)/da = 1)
        both = (lambda g_: (g_,) + (None,) * (nret - 2) + (g_,)) if ctx.has_add else (lambda g_: (g_,) + (None,) * (nret - 1))
        if dy is None:                      # only the residual branch carried a gradient
            return both(dpass)
        dy = dy.contiguous()
        if dy2 is not None:
            dy2 = dy2.contiguous()
            if dy2.dtype != dy.dtype or dy2.shape != dy.shape:
                dy, dy2 = dy + dy2, None
        Cc = x.shape[-1]
        rows = x.numel() // Cc
        if dpass is not None:
            dpass = dpass.contiguous()
            if dpass.dtype != x.dtype:
                dpass = dpass.to(x.dtype)
        dx, dgb = _ln_bwd_call(dy, x, gamma, mean, rstd, dpass, rows, Cc, "csts_layernorm_bwd",
                               want16=(x.dtype == torch.float32 and dy.dtype == L.half_dtype()), params=ctx.params,
                               copy_scale=ctx.copy_scale, dy2=dy2)
        if dgb is None:                     # finished and assigned by the end-of-backward flush
            return both(dx)
        return (dx, dgb[:Cc], dgb[Cc:]) + (None,) * (nret - 4) + ((dx,) if ctx.has_add else (None,))


def layer_norm(x, gamma, beta, eps, out_dt, passthrough: bool = False, fanout: bool = False, addend=None):
    """passthrough=False: y.  passthrough=True: (y, x_alias) -- use x_alias wherever x is used afterwards.
    fanout=True (with passthrough): (y_a, y_b, x_alias) for a LayerNorm output with TWO consumers -- the backward kernel reads
    both incoming gradients itself (csts_layernorm_bwd_ex) instead of autograd adding them first.
    addend (with passthrough): LayerNorm(x + addend), and x_alias is that sum (csts_layernorm_fwd_add) -- a skip connection
    folded into the norm that follows it."""
    return LayerNormFn.apply(x, gamma, beta, eps, out_dt, passthrough, fanout, addend)


# ----------------------------------------------------------------------------------------- element dropout
class Dropout:
    """One dropout site of one forward: nn.Dropout(p) in train mode (csts_dropout_fwd / _bwd).  key: int64 tensor of one element
    on the device (the forward's key, never read by the host); site: the fixed site id (include/csts_hip.h); p in (0, 1).
    For a Block, site is the base of its three sites (2 + 3*i): proj = site, MLP hidden = site + 1, MLP out = site + 2."""
    __slots__ = ("key", "site", "p", "thr", "scale")

    def __init__(self, key: torch.Tensor, site: int, p: float):
        if not (0.0 < p < 1.0):
            raise ValueError(f"dropout rate must be in (0, 1), got {p}")
        if key.dtype != torch.int64 or key.numel() != 1 or not key.is_cuda:
            raise L.CstsError("dropout key must be a one-element int64 GPU tensor")
        self.key, self.site, self.p = key, int(site), float(p)
        self.thr, self.scale = dropout_params(p)

    def at(self, offset: int) -> "Dropout":
        return Dropout(self.key, self.site + offset, self.p)


@functools.lru_cache(maxsize=None)
def dropout_params(p: float):
    """(thr, scale) of rate p: drop iff Philox word < thr = floor(p * 2^32) (double), kept elements times 1.0f / (1.0f - p)."""
    thr = min(int(math.floor(float(p) * 4294967296.0)), 0xFFFFFFFF)
    one = torch.tensor(1.0, dtype=torch.float32)
    scale = float(one / (one - torch.tensor(float(p), dtype=torch.float32)))
    return thr, scale


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _dropout_fwd(z: torch.Tensor, drop: Dropout, residual=None, row_scale=None, rows_per_scale=1):
    """z <- residual + row_scale * mask * scale * z, in place (z: a fresh contiguous GEMM output)."""
    cols = z.shape[-1]
    rows = z.numel() // cols
    if residual is not None:
        residual = _aligned(residual if residual.dtype == z.dtype else residual.to(z.dtype))
    L.check(_lib().csts_dropout_fwd(_p(z), _p(residual), _p(row_scale), rows_per_scale, _p(z), _dt(z), _p(drop.key), drop.site,
                                    drop.thr, drop.scale, rows, cols, _stream()), "csts_dropout_fwd")
    return z


def _dropout_bwd(dy: torch.Tensor, drop: Dropout, row_scale=None, rows_per_scale=1, out_dt=None, inplace=False):
    """dy * row_scale * mask * scale: a new tensor of dtype out_dt (default: dy's), or dy itself (inplace)."""
    cols = dy.shape[-1]
    rows = dy.numel() // cols
    if inplace:
        out = dy
    else:
        dy = _aligned(dy)
        out = torch.empty(dy.shape, dtype=dy.dtype if out_dt is None else torch_dtype(out_dt), device=dy.device)
    L.check(_lib().csts_dropout_bwd(_p(dy), _dt(dy), _p(row_scale), rows_per_scale, _p(out), _dt(out), _p(drop.key), drop.site,
                                    drop.thr, drop.scale, rows, cols, _stream()), "csts_dropout_bwd")
    return out


class DropoutFn(Function):
    """Out-of-place nn.Dropout(p) of a whole tensor (pos_drop, custom_multimodal_builder.py:375-377)."""

    @staticmethod
    def forward(ctx, x, drop: Dropout):
        _need_gpu(x)
        ctx.drop = drop
        return _dropout_bwd(x, drop)

    @staticmethod
    def backward(ctx, dy):
        return _dropout_bwd(dy, ctx.drop), None


def dropout(x: torch.Tensor, drop: Optional[Dropout]):
    return x if drop is None else DropoutFn.apply(x, drop)


def dropout_mask(key: torch.Tensor, site: int, rows: int, cols: int, p: float) -> torch.Tensor:
    """The (rows, cols) uint8 drop mask (1 = dropped) of a site under `key`, evaluated on the device (csts_dropout_mask)."""
    _need_gpu(key)
    thr, _ = dropout_params(p)
    out = torch.empty(rows, cols, dtype=torch.uint8, device=key.device)
    L.check(_lib().csts_dropout_mask(_p(key), int(site), thr, _p(out), rows * cols, _stream()), "csts_dropout_mask")
    return out


def dropout_mask_host(key: int, site: int, first: int, count: int, p: float):
    """The same mask evaluated on the CPU (csts_dropout_mask_host): a uint8 numpy array of elements first .. first + count - 1."""
    import numpy as np
    thr, _ = dropout_params(p)
    out = np.zeros(max(count, 1), dtype=np.uint8)
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    L.check(_lib().csts_dropout_mask_host(k & 0xFFFFFFFF, k >> 32, int(site), thr, int(first), int(count),
                                          out.ctypes.data_as(C.c_void_p)), "csts_dropout_mask_host")
    return out[:count]


# ----------------------------------------------------------------------------------------- Linear
class LinearFn(Function):
    """y = (x W^T + b) * row_scale + residual  (nn.Linear: attention.py:130,159,232,246; drop_path + residual
    of attention.py:242,247 folded into the epilogue)."""

    @staticmethod
    def forward(ctx, x, W, b, residual, row_scale, rows_per_scale: int, out_dt: int, compute: int, w16, w16t=None, res_up=None,
                drop=None):
        """res_up = (coarse thw, fine thw): `residual` is the decoder skip on the COARSE grid and the GEMM epilogue adds
        nn.Upsample(scale_factor=stride_q, mode='trilinear')(residual) (attention.py:463-471) -- x_res is never written.
        drop (optional Dropout): y = residual + row_scale * dropout(x W^T + b) -- the GEMM runs without its residual / row-scale
        epilogue and csts_dropout_fwd applies mask, drop-path and residual in one pass over its output."""
        _need_gpu(x, W)
        x = x.contiguous()
        W = W.contiguous()
        K = x.shape[-1]
        N = W.shape[0]
        M = x.numel() // K
        y = torch.empty(*x.shape[:-1], N, dtype=torch_dtype(out_dt), device=x.device)
        if residual is not None:
            residual = residual.contiguous()
        Wop = w16 if (w16 is not None and compute == BF16) else W     # bf16 shadow of the fp32 master weight
        if drop is not None:
            if res_up is not None:
                raise L.CstsError("linear(drop=...) does not take res_up: up-sample the skip first (ops.trilinear)")
            gemm(L.GEMM_NT, x, 0, K, Wop, 0, K, y, N, M, N, K, compute=compute, bias=b)
            _dropout_fwd(y, drop, residual, row_scale, rows_per_scale)
        else:
            gemm(L.GEMM_NT, x, 0, K, Wop, 0, K, y, N, M, N, K, compute=compute, bias=b, residual=residual, ldr=N,
                 row_scale=row_scale, rows_per_scale=rows_per_scale, res_up=res_up)
        ctx.drop = drop
        ctx.res_up = None
        if res_up is not None:
            thw_c, thw_f = list(res_up[0]), list(res_up[1])
            Bc = residual.shape[0]
            ctx.res_up = (_pool_geom(Bc, N, thw_c, thw_f, [f // c for f, c in zip(thw_f, thw_c)]), tuple(residual.shape))
        ctx.save_for_backward(x, Wop, row_scale)
        ctx.wdtype = W.dtype
        ctx.params = (W, b)
        ctx.w16t = w16t if (w16t is not None and compute == BF16 and Wop is w16) else None
        ctx.meta = (M, N, K, rows_per_scale, compute, b is not None, residual is not None,
                    residual.dtype if residual is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W, row_scale = ctx.saved_tensors
        M, N, K, rps, compute, has_b, has_res, res_dtype = ctx.meta
        sc = (row_scale, rps) if row_scale is not None else None
        drop = ctx.drop
        d16 = _grad16(dy, compute, sc) if (dy.is_contiguous() and drop is None) else None   # with drop-path: pre-multiplied
        dy = dy.contiguous()
        if drop is not None:               # the masked copy (times drop-path), straight to bf16 when the GEMMs run in bf16
            dys = _dropout_bwd(dy, drop, row_scale, rps, out_dt=BF16 if (compute == BF16 and BF16_GRAD_COPY) else None)
        elif d16 is not None:
            dys = d16
        elif row_scale is not None:        # drop-path: the scaled copy goes straight to bf16 when the GEMMs run in bf16
            dys = scale_rows(dy, row_scale, rps, M, N, out_dt=BF16 if (compute == BF16 and BF16_GRAD_COPY) else None)
        else:
            dys = dy
        dx = dW = db = dres = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _dgrad(dys, W, ctx.w16t, dx, M, N, K, compute)
        if ctx.needs_input_grad[1]:
            if has_b and ctx.needs_input_grad[2]:
                dW, db = _wgrad(dys, x, M, N, K, compute, want_bias=True, params=ctx.params)
            else:
                dW = _wgrad(dys, x, M, N, K, compute, params=(ctx.params[0], None))
            if dW is not None:
                dW = dW.to(ctx.wdtype)
        elif has_b and ctx.needs_input_grad[2]:
            db = colsum(dys, 1, M, N)
        if has_res and ctx.needs_input_grad[3]:
            if ctx.res_up is not None:      # adjoint of the up-sampling the epilogue applied to the coarse skip
                g, shape = ctx.res_up
                dres = torch.empty(shape, dtype=res_dtype, device=dy.device)
                L.check(_lib().csts_trilinear_bwd(C.byref(g), _p(dy), _dt(dy), _p(dres), _dt(dres), _stream()), "csts_trilinear_bwd(res_up)")
            else:
                dres = dy if dy.dtype == res_dtype else dy.to(res_dtype)
        return dx, dW, db, dres, None, None, None, None, None, None, None, None


def _dgrad(dy, W, Wt, dx, M, N, K, compute, epilogue=L.EPI_NONE, aux=None):
    """dx[M,K] = dy[M,N] W[N,K].  With the [K][N] twin of the bf16 shadow (csts_transpose_multi) and a bf16 dy this is an
    NT GEMM -- both operands contiguous along the reduction, the forward's kernels -- else NN on W itself."""
    if Wt is not None and dy.dtype == L.half_dtype() and USE_W16T:
        gemm(L.GEMM_NT, dy, 0, N, Wt, 0, N, dx, K, M, K, N, compute=compute, epilogue=epilogue, aux=aux)
    else:
        gemm(L.GEMM_NN, dy, 0, N, W, 0, K, dx, K, M, K, N, compute=compute, epilogue=epilogue, aux=aux)


USE_W16T = os.environ.get("CSTS_W16T", "1") != "0"


class _TransposeSet:
    """The [in][out] twins of a fixed set of bf16 matrices, refreshed by ONE csts_transpose_multi launch (tile table built
    once: the buffers never move)."""

    def __init__(self, pairs):
        self.pairs = list(pairs)                 # (src [R, C] bf16, dst [C, R] bf16)
        tiles = []
        for src, dst in self.pairs:
            R, Cc = src.shape
            assert src.dtype == L.half_dtype() and dst.dtype == L.half_dtype() and tuple(dst.shape) == (Cc, R)
            assert R % 8 == 0 and Cc % 8 == 0 and src.is_contiguous() and dst.is_contiguous()
            for r0 in range(0, R, 64):
                for c0 in range(0, Cc, 64):
                    tiles.append((src.data_ptr(), dst.data_ptr(), R, Cc, r0, c0))
        arr = (L.TransposeTile * len(tiles))()
        for i, t in enumerate(tiles):
            arr[i].src, arr[i].dst, arr[i].R, arr[i].C, arr[i].r0, arr[i].c0 = t
        self.n = len(tiles)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.pairs[0][0].device)

    def refresh(self):
        L.check(_lib().csts_transpose_multi(self.table.data_ptr(), self.n, _stream()), "csts_transpose_multi")


RES_UP_FUSE = os.environ.get("CSTS_RES_UP_FUSE", "1") != "0"     # decoder skip up-sampled inside the proj GEMM's epilogue


def res_up_ok(thw_fine) -> bool:
    """The fused form needs power-of-two fine grid sizes (csts_gemm_args.res_up)."""
    return RES_UP_FUSE and all(v > 0 and (v & (v - 1)) == 0 for v in thw_fine)


def linear(x, W, b=None, *, residual=None, row_scale=None, rows_per_scale=1, out_dt=F32, compute=F32, w16=None, w16t=None,
           res_up=None, drop: Optional[Dropout] = None):
    """drop: nn.Dropout on the Linear's output before drop-path and the residual add (proj_drop, attention.py:159-161)."""
    y = LinearFn.apply(x, W, b, residual, row_scale, rows_per_scale, out_dt, compute, w16, w16t, res_up, drop)
    if drop is not None:        # an elementwise mask: the next LayerNorm must not pre-scale its gradient copy by row_scale alone
        return y
    return _mark_scaled_output(y, row_scale if residual is not None else None, rows_per_scale)


class MlpFn(Function):
    """fc2(GELU_erf(fc1(x))) * row_scale + residual  (Mlp.forward common.py:26-34; attention.py:244-247).
    GELU lives in fc1's epilogue, GELU' in the epilogue of fc2's data-gradient GEMM."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, residual, row_scale, rows_per_scale: int, act_dt: int, out_dt: int, compute: int,
                w16_1, w16_2, w16t_1=None, w16t_2=None, drop=None):
        """drop (optional Dropout, sites drop.site = hidden, drop.site + 1 = out): Mlp.drop of common.py:26-34 on the GELU output
        (in place on g: the masked g is what fc2 and fc2's weight gradient read) and on fc2's output (csts_dropout_fwd with
        drop-path and residual, the GEMM without that epilogue)."""
        _need_gpu(x, W1, W2)
        ctx.params = (W1, b1, W2, b2)
        ctx.w16t = (None, None)
        if compute == BF16 and w16_1 is not None and w16_2 is not None:   # bf16 shadows of the fp32 master weights
            W1, W2 = w16_1, w16_2
            ctx.w16t = (w16t_1, w16t_2)
        x = x.contiguous()
        K = x.shape[-1]
        Hd = W1.shape[0]
        N = W2.shape[0]
        M = x.numel() // K
        # the pre-activation h is kept for backward only: an inference forward (no input needs a gradient) does not write it
        # (M x 4C x 2 bytes per block: 1.26 GB of a b = 4 forward at 16 x 256^2)
        train = any(ctx.needs_input_grad)
        g = torch.empty(M, Hd, dtype=torch_dtype(act_dt), device=x.device)
        h = torch.empty_like(g) if train else None   # pre-activation
        gemm(L.GEMM_NT, x, 0, K, W1, 0, K, g, Hd, M, Hd, K, compute=compute, bias=b1, epilogue=L.EPI_GELU, aux=h)
        y = torch.empty(*x.shape[:-1], N, dtype=torch_dtype(out_dt), device=x.device)
        if residual is not None:
            residual = residual.contiguous()
        ctx.drop = drop
        if drop is not None:
            _dropout_fwd(g, drop)
            gemm(L.GEMM_NT, g, 0, Hd, W2, 0, Hd, y, N, M, N, Hd, compute=compute, bias=b2)
            _dropout_fwd(y, drop.at(1), residual, row_scale, rows_per_scale)
        else:
            gemm(L.GEMM_NT, g, 0, Hd, W2, 0, Hd, y, N, M, N, Hd, compute=compute, bias=b2, residual=residual, ldr=N,
                 row_scale=row_scale, rows_per_scale=rows_per_scale)
        if train:
            ctx.save_for_backward(x, W1, W2, h, g, row_scale)
        ctx.meta = (M, K, Hd, N, rows_per_scale, compute, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W1, W2, h, g, row_scale = ctx.saved_tensors
        M, K, Hd, N, rps, compute, has_res = ctx.meta
        sc = (row_scale, rps) if row_scale is not None else None
        drop = ctx.drop
        d16 = _grad16(dy, compute, sc) if (dy.is_contiguous() and drop is None) else None   # with drop-path: pre-multiplied
        dy = dy.contiguous()
        if drop is not None:
            dys = _dropout_bwd(dy, drop.at(1), row_scale, rps, out_dt=BF16 if (compute == BF16 and BF16_GRAD_COPY) else None)
        elif d16 is not None:
            dys = d16
        elif row_scale is not None:
            dys = scale_rows(dy, row_scale, rps, M, N, out_dt=BF16 if (compute == BF16 and BF16_GRAD_COPY) else None)
        else:
            dys = dy
        P1, pb1, P2, pb2 = ctx.params
        dW2, db2 = _wgrad(dys, g, M, N, Hd, compute, want_bias=True, params=(P2, pb2))
        dh = torch.empty_like(h)
        _dgrad(dys, W2, ctx.w16t[1], dh, M, N, Hd, compute, epilogue=L.EPI_DGELU, aux=h)
        if drop is not None:               # dh = (dys W2) * GELU'(h) * mask * scale
            _dropout_bwd(dh, drop, inplace=True)
        dW1, db1 = _wgrad(dh, x, M, Hd, K, compute, want_bias=True, params=(P1, pb1))
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _dgrad(dh, W1, ctx.w16t[0], dx, M, Hd, K, compute)
        return dx, dW1, db1, dW2, db2, (dy if has_res else None), None, None, None, None, None, None, None, None, None, None


def mlp(x, W1, b1, W2, b2, *, residual=None, row_scale=None, rows_per_scale=1, act_dt=F32, out_dt=F32, compute=F32,
        w16_1=None, w16_2=None, w16t_1=None, w16t_2=None, drop: Optional[Dropout] = None):
    """drop: Mlp.drop (common.py:26-34) at sites drop.site (GELU output) and drop.site + 1 (fc2 output)."""
    y = MlpFn.apply(x, W1, b1, W2, b2, residual, row_scale, rows_per_scale, act_dt, out_dt, compute, w16_1, w16_2,
                    w16t_1, w16t_2, drop)
    if drop is not None:
        return y
    return _mark_scaled_output(y, row_scale if residual is not None else None, rows_per_scale)


# ----------------------------------------------------------------------------------------- attention inner
def _conv_geom(B, Cc, HD, fine_thw, stride, f_bs, f_ts, c_bs, c_ts) -> L.DwconvGeom:
    g = L.DwconvGeom()
    g.B, g.C, g.HD = B, Cc, HD
    g.Tf, g.Hf, g.Wf = fine_thw
    g.st, g.sh, g.sw = stride
    g.Tc, g.Hc, g.Wc = [(f - 1) // s + 1 for f, s in zip(fine_thw, stride)]
    g.fine_batch_stride, g.fine_token_stride = f_bs, f_ts
    g.coarse_batch_stride, g.coarse_token_stride = c_bs, c_ts
    return g


def _ln_rows_fwd(c, gamma, beta, HD, act_dt):
    rows = c.numel() // HD
    y = torch.empty(c.shape, dtype=torch_dtype(act_dt), device=c.device)
    mean = torch.empty(rows, dtype=torch.float32, device=c.device)
    rstd = torch.empty_like(mean)
    L.check(_lib().csts_layernorm_fwd(_p(c), _dt(c), _p(gamma), _p(beta), _p(y), act_dt, _p(mean), _p(rstd), rows, HD, 1e-5,
                                      _stream()), "csts_layernorm_fwd(head)")
    return y, mean, rstd


def _ln_rows_bwd(dy, c, gamma, mean, rstd, HD, params=None):
    rows = c.numel() // HD
    dc, dgb = _ln_bwd_call(dy, c, gamma, mean, rstd, None, rows, HD, "csts_layernorm_bwd(head)", params=params)
    if dgb is None:
        return dc, None, None
    return dc, dgb[:HD], dgb[HD:]


def _attn_args(dt, dims, mask, qd, kd, vd, o=None, lse=None, do=None, delta=None, tq=None, tk=None, tv=None):
    """The csts_attn_args of one call.  dims = (B, H, Nq, Nk, HD), mask = (mode, T, HW); qd / kd / vd and the gradient targets
    tq / tk / tv are (tensor, element offset, strides, ...) descriptors; o and do are contiguous (B, Nq, H * HD)."""
    B, H, Nq, Nk, HD = dims
    a = L.AttnArgs()
    a.dtype, a.B, a.H, a.Nq, a.Nk, a.head_dim = dt, B, H, Nq, Nk, HD
    for name, d in (("Q", qd), ("K", kd), ("V", vd), ("dQ", tq), ("dK", tk), ("dV", tv)):
        if d is not None:
            setattr(a, name, _p(d[0], d[1]))
            setattr(a, name.lower() + "_strides", (C.c_int64 * 3)(*d[2]))
    a.O, a.LSE, a.dO, a.delta = _p(o), _p(lse), _p(do), _p(delta)
    if o is not None:
        a.o_strides = (C.c_int64 * 3)(Nq * H * HD, H * HD, HD)
    if do is not None:
        a.do_strides = (C.c_int64 * 3)(Nq * H * HD, H * HD, HD)
    a.scale = HD ** -0.5
    a.mask_mode, a.mask_T, a.mask_HW = mask
    return a


class AttnInnerFn(Function):
    """Everything between the qkv Linear and the output projection of MultiScaleAttention /
    MultiScaleDecoderAttention / SpatialAttention / TemporalAttention (attention.py:130-158, :374-388;
    av_attention.py:127-141, :324-350): conv-pool (or ConvTranspose upsample of q) + LayerNorm(hd) of
    q/k/v read straight from the token-major qkv buffer, then the fused attention core.
    kind: 'enc' | 'dec' | 'plain'.  Returns o (B, Nq, C)."""

    @staticmethod
    def forward(ctx, qkv, kvc, wq, gq, bq, wk, gk, bk, wv, gv, bv, meta):
        """kvc is None: qkv is the (B, N, 3C) output of the qkv Linear.  kvc given (qkv_compact): `qkv` holds q only, (B, N, C),
        and kvc = k|v (B, Nc, 2C) on the COMPACT grid of the rows the K/V pools read (csts_kv_rows_geom): the pools then run
        over that grid with stride (1, 3, 3) -- the same taps, the same arithmetic."""
        _need_gpu(qkv)
        (B, N, Cc, H, thw, kind, stride_q, stride_kv, has_pool_q, has_pool_kv, mask_mode, mask_T, mask_HW, act_dt) = meta
        qkv = qkv.contiguous()
        HD = Cc // H
        dev = qkv.device
        lib = _lib()
        s = _stream()
        saved = {}
        QW = Cc if kvc is not None else 3 * Cc          # row width of the tensor that holds q
        if kvc is not None:
            kvc = kvc.contiguous()
            kv_thw = [thw[0]] + list(kv_compact_dims(thw, stride_kv))
            assert has_pool_kv and kv_thw[0] * kv_thw[1] * kv_thw[2] == kvc.shape[1] and kvc.shape[2] == 2 * Cc
            kv_src, kv_off, kv_w, kv_n, kv_stride = kvc, (0, Cc), 2 * Cc, kvc.shape[1], (1, 3, 3)
        else:
            kv_thw, kv_src, kv_off, kv_w, kv_n, kv_stride = list(thw), qkv, (Cc, 2 * Cc), 3 * Cc, N, stride_kv

        def slot_view(slot):   # (tensor, elem offset, strides) of q/k/v inside the qkv buffer
            return (qkv, slot * Cc, (N * QW, QW, HD), N)

        def pooled(slot, w, gamma, beta, stride, transposed):
            if transposed:   # decoder q: ConvTranspose3d, fine = output grid
                fine_thw = [t * st for t, st in zip(thw, stride)]
                Nf = fine_thw[0] * fine_thw[1] * fine_thw[2]
                g = _conv_geom(B, Cc, HD, fine_thw, stride, Nf * Cc, Cc, N * QW, QW)
                c = torch.empty(B, Nf, Cc, dtype=qkv.dtype, device=dev)
                L.check(lib.csts_dwconv_transposed(C.byref(g), _p(qkv, slot * Cc), _dt(qkv), _p(w), _p(c), _dt(c), s),
                        "csts_dwconv_transposed")
                n_out = Nf
                out_thw = fine_thw
            else:
                g = _conv_geom(B, Cc, HD, list(thw), stride, N * QW, QW, 0, Cc)
                n_out = g.Tc * g.Hc * g.Wc
                g.coarse_batch_stride = n_out * Cc
                c = torch.empty(B, n_out, Cc, dtype=qkv.dtype, device=dev)
                L.check(lib.csts_dwconv_strided(C.byref(g), _p(qkv, slot * Cc), _dt(qkv), _p(w), _p(c), _dt(c), s),
                        "csts_dwconv_strided")
                out_thw = [g.Tc, g.Hc, g.Wc]
            y, mean, rstd = _ln_rows_fwd(c, gamma, beta, HD, act_dt)
            saved[slot] = (c, mean, rstd, g)
            return (y, 0, (n_out * Cc, Cc, HD), n_out), out_thw

        def pooled_fused(slots, ws_, gammas, betas, stride):
            """Conv-pool + LayerNorm(hd) of 1 or 2 slots that share the geometry in ONE launch (csts_pool_ln_fwd)."""
            ns = len(slots)
            if slots[0] == 0:       # q: from the tensor that holds q
                src, offs, g = qkv, (0,), _conv_geom(B, Cc, HD, list(thw), stride, N * QW, QW, 0, Cc)
            else:                   # k | v: from the qkv buffer, or from the compact k|v tensor with the compact grid's stride
                src, offs, g = kv_src, kv_off, _conv_geom(B, Cc, HD, kv_thw, kv_stride, kv_n * kv_w, kv_w, 0, Cc)
            n_out = g.Tc * g.Hc * g.Wc
            g.coarse_batch_stride = n_out * Cc
            rows = B * n_out * H
            c = torch.empty(ns, B, n_out, Cc, dtype=qkv.dtype, device=dev)
            y = torch.empty_like(c)
            mean = torch.empty(ns, rows, dtype=torch.float32, device=dev)
            rstd = torch.empty_like(mean)
            pa = L.PoolLnArgs()
            pa.geom, pa.nslots, pa.dt, pa.eps = g, ns, _dt(qkv), 1e-5
            for i, slot in enumerate(slots):
                pa.fine[i], pa.weight[i], pa.gamma[i], pa.beta[i] = _p(src, offs[i]), _p(ws_[i]), _p(gammas[i]), _p(betas[i])
                pa.conv_out[i], pa.y[i], pa.mean[i], pa.rstd[i] = _p(c[i]), _p(y[i]), _p(mean[i]), _p(rstd[i])
            L.check(lib.csts_pool_ln_fwd(C.byref(pa), s), "csts_pool_ln_fwd")
            for i, slot in enumerate(slots):
                saved[slot] = (c[i], mean[i], rstd[i], g)
            if ns == 2:
                saved["kv"] = (c, mean, rstd, g)       # stacked pair: one-launch backward kernels
            return [(y[i], 0, (n_out * Cc, Cc, HD), n_out) for i in range(ns)]

        if kind == "dec":
            qd, _ = pooled(0, wq, gq, bq, stride_q, True)
        elif has_pool_q:
            qd, = pooled_fused([0], [wq], [gq], [bq], stride_q)
        else:
            qd = slot_view(0)
        if has_pool_kv:
            kd, vd = pooled_fused([1, 2], [wk, wv], [gk, gv], [bk, bv], stride_kv)
        else:
            kd, vd = slot_view(1), slot_view(2)
        Nq, Nk = qd[3], kd[3]
        o = torch.empty(B, Nq, Cc, dtype=qkv.dtype, device=dev)
        lse = torch.empty(B, H, Nq, dtype=torch.float32, device=dev)
        a = _attn_args(_dt(qkv), (B, H, Nq, Nk, HD), (mask_mode, mask_T, mask_HW), qd, kd, vd, o=o, lse=lse)
        L.check(lib.csts_attn_fwd(C.byref(a), s), "csts_attn_fwd")
        ctx.meta = meta
        ctx.saved_slots = saved
        ctx.descr = (qd, kd, vd, Nq, Nk)
        ctx.save_for_backward(qkv, o, lse, wq, gq, wk, gk, wv, gv, kvc)
        ctx.params = (wq, gq, bq, wk, gk, bk, wv, gv, bv)
        ctx.mark_non_differentiable(lse)
        ctx.set_materialize_grads(False)     # no zero-filled d(lse) tensor per backward
        return o, lse

    @staticmethod
    def backward(ctx, do, _dlse):
        (B, N, Cc, H, thw, kind, stride_q, stride_kv, has_pool_q, has_pool_kv, mask_mode, mask_T, mask_HW, act_dt) = ctx.meta
        qkv, o, lse, wq, gq, wk, gk, wv, gv, kvc = ctx.saved_tensors
        qd, kd, vd, Nq, Nk = ctx.descr
        saved = ctx.saved_slots
        HD = Cc // H
        dev = qkv.device
        lib = _lib()
        s = _stream()
        do = do.contiguous()
        dqkv = torch.empty_like(qkv)
        QW = Cc if kvc is not None else 3 * Cc
        if kvc is not None:             # compact k|v: its gradient has the compact grid's rows only
            dkvc = torch.empty_like(kvc)
            kv_fine, kv_dfine, kv_off = kvc, dkvc, (0, Cc)
        else:
            dkvc, kv_fine, kv_dfine, kv_off = None, qkv, dqkv, (Cc, 2 * Cc)
        delta = torch.empty(B, H, Nq, dtype=torch.float32, device=dev)

        def grad_target(slot, n_rows):   # where attention bwd writes d(q|k|v)
            if slot in saved:
                t = torch.empty(B, n_rows, Cc, dtype=qkv.dtype, device=dev)
                return t, 0, (n_rows * Cc, Cc, HD)
            return dqkv, slot * Cc, (N * QW, QW, HD)

        tq = grad_target(0, Nq)
        if "kv" in saved:               # dK | dV stacked like the saved pooled pair
            dkv = torch.empty(2, B, Nk, Cc, dtype=qkv.dtype, device=dev)
            tk, tv = (dkv[0], 0, (Nk * Cc, Cc, HD)), (dkv[1], 0, (Nk * Cc, Cc, HD))
        else:
            tk, tv = grad_target(1, Nk), grad_target(2, Nk)
        a = _attn_args(_dt(qkv), (B, H, Nq, Nk, HD), (mask_mode, mask_T, mask_HW), qd, kd, vd, o=o, lse=lse, do=do, delta=delta,
                       tq=tq, tk=tk, tv=tv)
        ws = _ws(lib.csts_attn_bwd_workspace(C.byref(a)), dev)
        L.check(lib.csts_attn_bwd(C.byref(a), _p(ws), ws.numel(), s), "csts_attn_bwd")

        grads = {}

        P = ctx.params                      # leaf parameters (wq, gq, bq, wk, gk, bk, wv, gv, bv)

        def pooled_bwd(slot, dy, w, gamma, transposed):
            c, mean, rstd, g = saved[slot]
            pw, pg, pb = P[3 * slot], P[3 * slot + 1], P[3 * slot + 2]
            dc, dg, db = _ln_rows_bwd(dy, c, gamma, mean, rstd, HD, params=(pg, pb))
            defer = _can_defer(pw)
            grouped = defer and _stencil_group_now()
            wsz = (lib.csts_dwconv_wgrad_grouped_workspace if grouped else lib.csts_dwconv_wgrad_workspace)(C.byref(g))
            wws = _ws(wsz, dev)
            dw = torch.empty(HD * 27, dtype=torch.float32, device=dev)
            dwp = None if defer else _p(dw)
            if grouped:
                if transposed:
                    _queue_stencil_wgrad(g, dc, 0, qkv, slot * Cc, wws)
                else:
                    _queue_stencil_wgrad(g, qkv, slot * Cc, dc, 0, wws)
            elif transposed:   # fine = dc (output side), coarse = qkv slot
                L.check(lib.csts_dwconv_wgrad(C.byref(g), _p(dc), _dt(dc), _p(qkv, slot * Cc), _dt(qkv), dwp, _p(wws),
                                              wws.numel(), s), "csts_dwconv_wgrad")
            else:            # fine = qkv slot, coarse = dc
                L.check(lib.csts_dwconv_wgrad(C.byref(g), _p(qkv, slot * Cc), _dt(qkv), _p(dc), _dt(dc), dwp, _p(wws),
                                              wws.numel(), s), "csts_dwconv_wgrad")
            if transposed:
                L.check(lib.csts_dwconv_strided(C.byref(g), _p(dc), _dt(dc), _p(w), _p(dqkv, slot * Cc), _dt(dqkv), s),
                        "csts_dwconv_strided(bwd)")
            else:
                L.check(lib.csts_dwconv_transposed(C.byref(g), _p(dc), _dt(dc), _p(w), _p(dqkv, slot * Cc), _dt(dqkv), s),
                        "csts_dwconv_transposed(bwd)")
            dwv = dw.view(HD, 1, 3, 3, 3)
            if defer:
                _defer(wws, dw, wsz // (HD * 27 * 4), HD * 27)
                _assign_later(pw, dwv)
                dwv = None
            grads[slot] = (dwv, dg, db)

        def pooled_bwd_kv():
            """LayerNorm backward, transposed conv (data gradient) and stencil weight gradient of the k AND v pools,
            one launch each."""
            c2, mean2, rstd2, g = saved["kv"]
            rows = B * Nk * H
            dc2 = torch.empty_like(c2)
            dgb = torch.empty(2, 2 * HD, dtype=torch.float32, device=dev)
            nbytes = lib.csts_layernorm_bwd_workspace(rows, HD)
            lws = _ws(2 * nbytes, dev)
            defer = _can_defer(P[3], P[4], P[5], P[6], P[7], P[8])
            L.check(lib.csts_layernorm_bwd2(_p(dkv), _dt(dkv), _p(c2), _dt(c2), _p(gk), _p(gv), _p(mean2), _p(rstd2), _p(dc2),
                                            _dt(dc2), None if defer else _p(dgb[0]), None if defer else _p(dgb[1]), _p(lws),
                                            lws.numel(), rows, HD, s), "csts_layernorm_bwd2")
            if defer:
                nrow = nbytes // (2 * HD * 4)
                _defer(lws[:nbytes], dgb[0], nrow, 2 * HD)
                _defer(lws[nbytes:], dgb[1], nrow, 2 * HD)
            vp2 = C.c_void_p * 2
            L.check(lib.csts_dwconv_transposed2(C.byref(g), vp2(_p(dc2[0]), _p(dc2[1])), _dt(dc2), vp2(_p(wk), _p(wv)),
                                                vp2(_p(kv_dfine, kv_off[0]), _p(kv_dfine, kv_off[1])), _dt(kv_dfine), s),
                    "csts_dwconv_transposed2")
            grouped = defer and _stencil_group_now()
            wsz = (lib.csts_dwconv_wgrad_grouped_workspace if grouped else lib.csts_dwconv_wgrad_workspace)(C.byref(g))
            wws = _ws(2 * wsz, dev)
            dw = torch.empty(2, HD * 27, dtype=torch.float32, device=dev)
            dwp = vp2(None, None) if defer else vp2(_p(dw[0]), _p(dw[1]))
            if grouped:
                for i in (0, 1):
                    _queue_stencil_wgrad(g, kv_fine, kv_off[i], dc2[i], 0, wws[i * wsz:(i + 1) * wsz])
            else:
                L.check(lib.csts_dwconv_wgrad2(C.byref(g), vp2(_p(kv_fine, kv_off[0]), _p(kv_fine, kv_off[1])), _dt(kv_fine),
                                               vp2(_p(dc2[0]), _p(dc2[1])), _dt(dc2), dwp, _p(wws), wws.numel(), s), "csts_dwconv_wgrad2")
            if defer:
                nrow = wsz // (HD * 27 * 4)
                _defer(wws[:wsz], dw[0], nrow, HD * 27)
                _defer(wws[wsz:], dw[1], nrow, HD * 27)
            for i, slot in enumerate((1, 2)):
                gw, gg, gb = dw[i].view(HD, 1, 3, 3, 3), dgb[i, :HD], dgb[i, HD:]
                if defer:
                    _assign_later(P[3 * slot], gw)
                    _assign_later(P[3 * slot + 1], gg)
                    _assign_later(P[3 * slot + 2], gb)
                    gw = gg = gb = None
                grads[slot] = (gw, gg, gb)

        if 0 in saved:
            pooled_bwd(0, tq[0], wq, gq, kind == "dec")
        if "kv" in saved:
            pooled_bwd_kv()
        elif 1 in saved:
            pooled_bwd(1, tk[0], wk, gk, False)
            pooled_bwd(2, tv[0], wv, gv, False)
        gq_ = grads.get(0, (None, None, None))
        gk_ = grads.get(1, (None, None, None))
        gv_ = grads.get(2, (None, None, None))
        return (dqkv, dkvc, gq_[0], gq_[1], gq_[2], gk_[0], gk_[1], gk_[2], gv_[0], gv_[1], gv_[2], None)


def attention_inner(qkv, wq, gq, bq, wk, gk, bk, wv, gv, bv, meta, kvc=None):
    return AttnInnerFn.apply(qkv, kvc, wq, gq, bq, wk, gk, bk, wv, gv, bv, meta)


# ----------------------------------------------------------------------------------------- qkv Linear, k|v on the rows that are read
KV_COMPACT_MIN_STRIDE = int(os.environ.get("CSTS_KV_COMPACT", "8"))     # 0 = off; pools with spatial stride >= this take the compact path


def kv_compact_dims(thw, stride_kv):
    """(Hc, Wc) of the compact grid of the token rows a 3x3x3 pool with stride (1, s, s), padding 1 reads (csts_kv_rows_geom):
    3 cells per output cell minus the padding cell in front, minus the last one when it falls outside the grid."""
    out = []
    for n, st in zip(thw[1:], stride_kv[1:]):
        no = (n - 1) // st + 1
        out.append(3 * no - 1 - (1 if (no - 1) * st + 1 > n - 1 else 0))
    return tuple(out)


def kv_compact_ok(thw, stride_kv, has_pool_kv) -> bool:
    return bool(has_pool_kv and KV_COMPACT_MIN_STRIDE > 0 and stride_kv[0] == 1 and stride_kv[1] >= max(3, KV_COMPACT_MIN_STRIDE)
                and stride_kv[2] >= max(3, KV_COMPACT_MIN_STRIDE))


def _kv_rows_geom(B, Cc, thw, stride_kv) -> L.KvRowsGeom:
    g = L.KvRowsGeom()
    g.B, g.C, g.T, g.H, g.W = B, Cc, thw[0], thw[1], thw[2]
    g.sh, g.sw = stride_kv[1], stride_kv[2]
    g.Hc, g.Wc = kv_compact_dims(thw, stride_kv)
    return g


class QkvCompactFn(Function):
    """The qkv Linear of a block whose K/V pools have spatial stride s >= 4 (attention.py:88,130 feeding :104-116): the pools
    are 3x3x3 convs with stride (1, s, s), so only (3/s)^2 of the token rows of k and v are ever read -- 14 % at s = 8, 3.5 % at
    s = 16.  q = x Wq^T + bq over all rows; k|v = x[rows] Wkv^T + bkv over the gathered rows only, laid out on the compact grid
    the pools then walk with stride (1, 3, 3).  Rows of a Linear are independent: the values that ARE computed equal the
    reference's.  Backward: dx = dq Wq + scatter_add(dkv Wkv); dW = [dq^T x ; dkv^T x[rows]]."""

    @staticmethod
    def forward(ctx, x, W, b, thw, stride_kv, out_dt: int, compute: int, w16, w16t):
        _need_gpu(x, W)
        x = x.contiguous()
        B, N, K = x.shape
        Cc = W.shape[0] // 3
        assert W.shape[1] == K and N == thw[0] * thw[1] * thw[2]
        g = _kv_rows_geom(B, K, thw, stride_kv)
        Nc = g.T * g.Hc * g.Wc
        xk = torch.empty(B, Nc, K, dtype=x.dtype, device=x.device)
        L.check(_lib().csts_rows_gather(C.byref(g), _p(x), _dt(x), _p(xk), _stream()), "csts_rows_gather")
        Wop = w16 if (w16 is not None and compute == BF16) else W.contiguous()
        q = torch.empty(B, N, Cc, dtype=torch_dtype(out_dt), device=x.device)
        kv = torch.empty(B, Nc, 2 * Cc, dtype=torch_dtype(out_dt), device=x.device)
        gemm(L.GEMM_NT, x, 0, K, Wop, 0, K, q, Cc, B * N, Cc, K, compute=compute, bias=(b[:Cc] if b is not None else None))
        gemm(L.GEMM_NT, xk, 0, K, Wop, Cc * K, K, kv, 2 * Cc, B * Nc, 2 * Cc, K, compute=compute,
             bias=(b[Cc:] if b is not None else None))
        ctx.save_for_backward(x, xk, Wop)
        ctx.params = (W, b)
        ctx.w16t = w16t if (w16t is not None and compute == BF16 and Wop is w16) else None
        ctx.meta = (B, N, Nc, K, Cc, compute, g)
        return q, kv

    @staticmethod
    def backward(ctx, dq, dkv):
        x, xk, W = ctx.saved_tensors
        B, N, Nc, K, Cc, compute, g = ctx.meta
        Wp, bp = ctx.params
        dq, dkv = dq.contiguous(), dkv.contiguous()
        Wt = ctx.w16t
        dx = torch.empty_like(x)
        dxk = torch.empty(B, Nc, K, dtype=torch.float32, device=x.device)     # fp32: one rounding when it joins dx
        if Wt is not None and dq.dtype == L.half_dtype() and USE_W16T:         # NT on the [in][out] twin (columns 0..C | C..3C)
            gemm(L.GEMM_NT, dq, 0, Cc, Wt, 0, 3 * Cc, dx, K, B * N, K, Cc, compute=compute)
            gemm(L.GEMM_NT, dkv, 0, 2 * Cc, Wt, Cc, 3 * Cc, dxk, K, B * Nc, K, 2 * Cc, compute=compute)
        else:
            gemm(L.GEMM_NN, dq, 0, Cc, W, 0, K, dx, K, B * N, K, Cc, compute=compute)
            gemm(L.GEMM_NN, dkv, 0, 2 * Cc, W, Cc * K, K, dxk, K, B * Nc, K, 2 * Cc, compute=compute)
        L.check(_lib().csts_rows_scatter_add(C.byref(g), _p(dxk), _dt(dxk), _p(dx), _dt(dx), _stream()), "csts_rows_scatter_add")
        # weight / bias gradients: rows 0..C from all tokens, rows C..3C from the gathered ones, into ONE gradient tensor
        dW = db = None
        queued = False
        if compute == BF16 and GROUP_WGRADS != "never" and (GROUP_WGRADS != "capture" or torch.cuda.is_current_stream_capturing()) \
                and DEFER_REDUCTIONS and x.dtype == L.half_dtype() and Cc % 8 == 0 and K % 8 == 0 and B * Nc >= 256 \
                and Wp.dtype == torch.float32 and _can_defer(Wp, bp):
            dWf = _grad_buffer(Wp, (3 * Cc, K), x.device)
            dbf = _grad_buffer(bp, (3 * Cc,), x.device) if bp is not None else None
            _pass.wgq.append((dq, x, dWf[:Cc], dbf[:Cc] if dbf is not None else None, B * N, Cc, K))
            _pass.wgq.append((dkv, xk, dWf[Cc:], dbf[Cc:] if dbf is not None else None, B * Nc, 2 * Cc, K))
            _assign_later(Wp, dWf)
            _assign_later(bp, dbf)
            cur = torch.cuda.current_stream()
            _pass.wg_prod[cur.cuda_stream] = cur
            queued = True
        if not queued:
            dW = torch.empty(3 * Cc, K, dtype=torch.float32, device=x.device)
            db = torch.empty(3 * Cc, dtype=torch.float32, device=x.device) if bp is not None else None
            for dy_, x_, r0, nr, tok in ((dq, x, 0, Cc, B * N), (dkv, xk, Cc, 2 * Cc, B * Nc)):
                split = _wgrad_split(nr, K, tok)
                det = split > 1 and _lib().csts_gemm_splitk_workspace(nr, K, tok, split) <= SPLITK_WS_LIMIT
                part = dW[r0:r0 + nr]
                if split > 1 and not det:
                    part.zero_()
                cs = gemm(L.GEMM_TN, dy_, 0, nr, x_, 0, K, part, K, nr, K, tok, compute=compute, split_k=split, deterministic=det,
                          want_colsum=db is not None)
                if db is not None:
                    db[r0:r0 + nr].copy_(cs if cs is not None else colsum(dy_, 1, tok, nr))
            dW = dW.to(Wp.dtype)
        return dx, dW, db, None, None, None, None, None, None


def qkv_compact(x, W, b, thw, stride_kv, *, out_dt, compute, w16=None, w16t=None):
    """(q (B, N, C), k|v (B, Nc, 2C) on the compact grid) -- see QkvCompactFn."""
    return QkvCompactFn.apply(x, W, b, list(thw), tuple(stride_kv), out_dt, compute, w16, w16t)


def attention_probs(qkv, B, N, Cc, H, lse, mask_mode, mask_T, mask_HW):
    """Probabilities of an un-pooled attention (fusion blocks) for return_spatial_attn / return_temporal_attn
    (av_attention.py:150-153,358-359); forward-only visualisation output."""
    HD = Cc // H
    probs = torch.empty(B, H, N, N, dtype=torch.float32, device=qkv.device)
    qd, kd, vd = ((qkv, slot * Cc, (N * 3 * Cc, 3 * Cc, HD)) for slot in range(3))
    a = _attn_args(_dt(qkv), (B, H, N, N, HD), (mask_mode, mask_T, mask_HW), qd, kd, vd, lse=lse)
    L.check(_lib().csts_attn_probs(C.byref(a), _p(probs), _stream()), "csts_attn_probs")
    return probs


class AudioAttnFn(Function):
    """Per-token weight from the audio -> pixel attention of the spatial fusion block (MVIT.SPATIAL_AUDIO_ATTN):
    av_attention.py:356-370 (probabilities of audio token t over frame t's video tokens, min-max rescaled per head) and the
    head mean of custom_multimodal_builder.py:438.  Differentiable w.r.t. the block's qkv projection (the reference
    back-propagates through the rescaled map in train mode).  Returns (wmap (B, T*HW), audio_attn (B, H, T, HW))."""

    @staticmethod
    def forward(ctx, qkv, T: int, HW: int, Cc: int, H: int):
        _need_gpu(qkv)
        qkv = qkv.contiguous()
        B = qkv.shape[0]
        if qkv.shape[1] != T * HW + T or qkv.shape[2] != 3 * Cc:
            raise L.CstsError(f"audio_attn: qkv {tuple(qkv.shape)} is not (B, {T * HW + T}, {3 * Cc})")
        aa = torch.empty(B, H, T, HW, dtype=torch.float32, device=qkv.device)
        wmap = torch.empty(B, T * HW, dtype=torch.float32, device=qkv.device)
        scale = (Cc // H) ** -0.5
        L.check(_lib().csts_audio_attn_fwd(_p(qkv), _dt(qkv), _p(aa), _p(wmap), B, T, HW, Cc, H, scale, _stream()),
                "csts_audio_attn_fwd")
        ctx.save_for_backward(qkv)
        ctx.meta = (B, T, HW, Cc, H, scale)
        ctx.mark_non_differentiable(aa)
        ctx.set_materialize_grads(False)
        return wmap, aa

    @staticmethod
    def backward(ctx, dwmap, _daa):
        (qkv,) = ctx.saved_tensors
        B, T, HW, Cc, H, scale = ctx.meta
        if dwmap is None:
            return None, None, None, None, None
        dwmap = dwmap.contiguous().float()
        dqkv = torch.zeros_like(qkv)
        L.check(_lib().csts_audio_attn_bwd(_p(qkv), _dt(qkv), _p(dwmap), _p(dqkv), B, T, HW, Cc, H, scale, _stream()),
                "csts_audio_attn_bwd")
        return dqkv, None, None, None, None


def audio_attn(qkv, T, HW, Cc, H):
    return AudioAttnFn.apply(qkv, int(T), int(HW), int(Cc), int(H))


class RowWeightFn(Function):
    """x (B, N, C) * w (B, N)[:, :, None]  (x_temporal * audio_attn, custom_multimodal_builder.py:439-440)."""

    @staticmethod
    def forward(ctx, x, w):
        _need_gpu(x, w)
        x = x.contiguous()
        w = w.contiguous().float()
        Cc = x.shape[-1]
        M = x.numel() // Cc
        if w.numel() != M:
            raise L.CstsError("row_weight: one weight per row expected")
        y = torch.empty_like(x)
        L.check(_lib().csts_scale_rows(_p(x), _dt(x), _p(w), 1, _p(y), _dt(y), M, Cc, _stream()), "csts_scale_rows")
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        Cc = x.shape[-1]
        M = x.numel() // Cc
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            L.check(_lib().csts_scale_rows(_p(dy), _dt(dy), _p(w), 1, _p(dx), _dt(dx), M, Cc, _stream()), "csts_scale_rows(bwd)")
        if ctx.needs_input_grad[1]:
            dw = torch.empty(w.shape, dtype=torch.float32, device=x.device)
            L.check(_lib().csts_rowdot2(_p(dy), _dt(dy), _p(x), _dt(x), _p(dw), M, Cc, _stream()), "csts_rowdot2")
        return dx, dw


def row_weight(x, w):
    return RowWeightFn.apply(x, w)


# ----------------------------------------------------------------------------------------- resampling
def _pool_geom(B, Cc, thw_in, thw_out, stride) -> L.PoolGeom:
    g = L.PoolGeom()
    g.B, g.C = B, Cc
    g.Ti, g.Hi, g.Wi = thw_in
    g.To, g.Ho, g.Wo = thw_out
    g.st, g.sh, g.sw = stride
    return g


class MaxPoolFn(Function):
    """pool_skip MaxPool3d on tokens (attention.py:193-195,234-236,240)."""

    @staticmethod
    def forward(ctx, x, thw, stride):
        _need_gpu(x)
        x = x.contiguous()
        B, N, Cc = x.shape
        k = [s + 1 if s > 1 else 1 for s in stride]
        out = [(d + 2 * (kk // 2) - kk) // s + 1 for d, kk, s in zip(thw, k, stride)]
        g = _pool_geom(B, Cc, thw, out, stride)
        y = torch.empty(B, out[0] * out[1] * out[2], Cc, dtype=x.dtype, device=x.device)
        arg = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
        L.check(_lib().csts_maxpool_fwd(C.byref(g), _p(x), _dt(x), _p(y), _p(arg), _stream()), "csts_maxpool_fwd")
        ctx.save_for_backward(arg)
        ctx.g = g
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty(ctx.shape, dtype=dy.dtype, device=dy.device)
        L.check(_lib().csts_maxpool_bwd(C.byref(ctx.g), _p(dy), _dt(dy), _p(arg), _p(dx), _stream()), "csts_maxpool_bwd")
        return dx, None, None


class TrilinearFn(Function):
    """nn.Upsample(scale_factor=stride, mode='trilinear') on tokens (attention.py:463-467,471); with `addend`
    it is also feat + F.interpolate(en_feat) of custom_multimodal_builder.py:479."""

    @staticmethod
    def forward(ctx, x, thw, stride, addend):
        _need_gpu(x)
        x = x.contiguous()
        B, N, Cc = x.shape
        out = [d * s for d, s in zip(thw, stride)]
        g = _pool_geom(B, Cc, thw, out, stride)
        y = torch.empty(B, out[0] * out[1] * out[2], Cc, dtype=x.dtype, device=x.device)
        if addend is not None:
            addend = addend.contiguous()
        L.check(_lib().csts_trilinear_fwd(C.byref(g), _p(x), _dt(x), _p(addend), _dt(addend) if addend is not None else 0,
                                          _p(y), _dt(y), _stream()), "csts_trilinear_fwd")
        ctx.g = g
        ctx.shape = x.shape
        ctx.has_add = addend is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty(ctx.shape, dtype=dy.dtype, device=dy.device)
        L.check(_lib().csts_trilinear_bwd(C.byref(ctx.g), _p(dy), _dt(dy), _p(dx), _dt(dx), _stream()), "csts_trilinear_bwd")
        return dx, None, None, (dy if ctx.has_add else None)


def maxpool_skip(x, thw, stride):
    return MaxPoolFn.apply(x, list(thw), list(stride))


def trilinear(x, thw, stride, addend=None):
    return TrilinearFn.apply(x, list(thw), list(stride), addend)


# ----------------------------------------------------------------------------------------- patch embed
class PatchEmbedFn(Function):
    """PatchEmbed.forward (stem_helper.py:35-38) + separable pos-embed add (custom_multimodal_builder.py:362-370):
    im2col -> MFMA GEMM with bias and the (broadcast) positional embedding in the epilogue."""

    @staticmethod
    def forward(ctx, x, W, b, pos_s, pos_t, kernel, stride, padding, act_dt: int, compute: int):
        _need_gpu(x, W)
        x = x.contiguous()
        B, Cin, T, H, Wd = x.shape
        Cout = W.shape[0]
        K = Cin * kernel[0] * kernel[1] * kernel[2]
        Kpad = (K + 31) // 32 * 32
        g = L.Im2colGeom()
        g.B, g.Cin, g.T, g.H, g.W = B, Cin, T, H, Wd
        g.kernel = (C.c_int * 3)(*kernel)
        g.stride = (C.c_int * 3)(*stride)
        g.padding = (C.c_int * 3)(*padding)
        out = [(d + 2 * p - k) // s + 1 for d, p, k, s in zip((T, H, Wd), padding, kernel, stride)]
        g.To, g.Ho, g.Wo = out
        g.Kpad = Kpad
        N = out[0] * out[1] * out[2]
        M = B * N
        col = torch.empty(M, Kpad, dtype=torch_dtype(act_dt), device=x.device)
        L.check(_lib().csts_im2col(C.byref(g), _p(x), _dt(x), _p(col), act_dt, _stream()), "csts_im2col")
        Wp = torch.zeros(Cout, Kpad, dtype=torch.float32, device=x.device)
        Wp[:, :K] = W.reshape(Cout, K)            # weight-layout plumbing (42 K elements)
        pos = torch.empty(N, Cout, dtype=torch.float32, device=x.device)
        HW = out[1] * out[2]
        L.check(_lib().csts_posembed_build(_p(pos_s), _p(pos_t), _p(pos), out[0], HW, Cout, _stream()), "csts_posembed_build")
        y = torch.empty(B, N, Cout, dtype=torch.float32, device=x.device)
        gemm(L.GEMM_NT, col, 0, Kpad, Wp, 0, Kpad, y, Cout, M, Cout, Kpad, compute=compute, bias=b, residual=pos, ldr=Cout,
             res_row_mod=N)
        ctx.save_for_backward(col)
        ctx.meta = (B, N, out[0], HW, Cout, K, Kpad, compute, tuple(W.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        (col,) = ctx.saved_tensors
        B, N, T, HW, Cout, K, Kpad, compute, wshape = ctx.meta
        dy = dy.contiguous()
        M = B * N
        dWp = _wgrad(dy, col, M, Cout, Kpad, compute)
        dW = dWp[:, :K].reshape(wshape)
        dpos = colsum(dy, 1, B, N * Cout)                       # sum over batch -> (N*Cout): the only pass over dy itself
        dps = colsum(dpos, 1, T, HW * Cout).view(1, HW, Cout)   # sum over t
        dpt = colsum(dpos, T, HW, Cout).view(1, T, Cout)        # sum over hw, per t
        db = colsum(dpt, 1, T, Cout)                            # bias gradient = sum over every token: from the T partial rows
        return None, dW, db, dps, dpt, None, None, None, None, None


def patch_embed(x, W, b, pos_s, pos_t, kernel, stride, padding, act_dt, compute):
    return PatchEmbedFn.apply(x, W, b, pos_s, pos_t, list(kernel), list(stride), list(padding), act_dt, compute)


# ----------------------------------------------------------------------------------------- fusion conv
# Data-parallel factor exchange (csts_amd.train.SegmentedTrainStep, CSTS_AMD.FUSION_GRAD_FACTORS): the weight gradient of a fusion
# conv is dW = dY^T A with only B*T' token rows (32 at b = 4, 16 frames) -- a rank-32 update of a 768 x 49152 matrix, 151 MB in
# fp32, 60 % of all gradient bytes for the three of them.  Across W ranks the averaged gradient is (1/W) [dY_0; ..; dY_W-1]^T
# [A_0; ..; A_W-1]: the ranks exchange the FACTORS (all-gather of 32 x 768 fp32 + 32 x 49152 16-bit rows: 3.2 MB per conv) and each
# forms the product itself, instead of all-reducing the 151 MB.  While a sink is set, FusionConvFn.backward hands its factors over
# and computes no dW (the parameter's gradient is written later by the step that owns the sink).
_factor_sink = None          # None, or {"params": set of weight data_ptrs, "items": [(W, dy, A, compute)], optional "accept": f(W, rows)}


def set_factor_sink(sink=None):
    global _factor_sink
    _factor_sink = sink


class FusionConvFn(Function):
    """Conv3d(C, C, kernel (1,8,8)) over the folded token grid -> (B, T, C)
    (custom_multimodal_builder.py:227-229,420-421,442-445): token fold (batched transpose) + skinny split-K GEMM
    that streams the 37.7 M-parameter weight once, in its native (Cout, Cin*H*W) layout."""

    @staticmethod
    def forward(ctx, x, W, b, T: int, HW: int, act_dt: int, compute: int, w16=None):
        _need_gpu(x, W)
        x = x.contiguous()
        B, N, Cc = x.shape
        Cout = W.shape[0]
        BT = B * T
        K = Cc * HW
        A = torch.empty(BT, K, dtype=torch_dtype(act_dt), device=x.device)
        L.check(_lib().csts_transpose_batched(_p(x), _dt(x), _p(A), act_dt, BT, HW, Cc, _stream()), "csts_transpose_batched")
        y = torch.empty(B, T, Cout, dtype=torch.float32, device=x.device)
        Wop = w16 if (w16 is not None and compute == BF16 and w16.numel() == W.numel()) else W     # bf16 shadow: half the stream
        Wv = Wop.reshape(Cout, K)
        split = max(1, min(128, K // 256))
        gemm(L.GEMM_NT, A, 0, K, Wv, 0, K, y, Cout, BT, Cout, K, compute=compute, bias=b, split_k=split)
        ctx.save_for_backward(A, W, Wop)
        ctx.meta = (B, T, HW, Cc, Cout, compute, x.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        A, W, Wop = ctx.saved_tensors
        B, T, HW, Cc, Cout, compute, xdtype = ctx.meta
        BT, K = B * T, Cc * HW
        dy = dy.contiguous()
        Wv = Wop.reshape(Cout, K)
        sink = _factor_sink
        if (sink is not None and W.data_ptr() in sink["params"] and ctx.needs_input_grad[1]
                and ("accept" not in sink or sink["accept"](W, BT))):
            sink["items"].append((W, dy, A, compute))      # factors only: the owner of the sink forms dW after the exchange
            dW = None
        else:
            dW = _grad_buffer(W, (Cout, K), dy.device)        # the data-parallel chain: straight into its all-reduce bucket
            gemm(L.GEMM_TN, dy, 0, Cout, A, 0, K, dW, K, Cout, K, BT, compute=compute)
        db = colsum(dy, 1, BT, Cout)
        dx = None
        if ctx.needs_input_grad[0]:
            dA = torch.empty_like(A)
            gemm(L.GEMM_NN, dy, 0, Cout, Wv, 0, K, dA, K, BT, K, Cout, compute=compute)
            dx = torch.empty(B, T * HW, Cc, dtype=xdtype, device=dy.device)
            L.check(_lib().csts_transpose_batched(_p(dA), _dt(dA), _p(dx), _dt(dx), BT, Cc, HW, _stream()),
                    "csts_transpose_batched(bwd)")
        return dx, (dW.view(W.shape) if dW is not None else None), db, None, None, None, None, None


def fusion_conv(x, W, b, T, HW, act_dt, compute, w16=None):
    return FusionConvFn.apply(x, W, b, T, HW, act_dt, compute, w16)


# ----------------------------------------------------------------------------------------- glue
class ReweightFn(Function):
    """x.view(B,T,H,W,C) * w[:, :, None, None, :]  (custom_multimodal_builder.py:454-461)."""

    @staticmethod
    def forward(ctx, x, w, T: int, HW: int):
        _need_gpu(x, w)
        x = x.contiguous().float()
        w = w.contiguous().float()
        B, N, Cc = x.shape
        y = torch.empty_like(x)
        L.check(_lib().csts_reweight_fwd(_p(x), _p(w), _p(y), B * T, HW, Cc, _stream()), "csts_reweight_fwd")
        ctx.save_for_backward(x, w)
        ctx.meta = (B * T, HW, Cc)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        BT, HW, Cc = ctx.meta
        dy = dy.contiguous().float()
        dx = torch.empty_like(x)
        dw = torch.empty_like(w)
        L.check(_lib().csts_reweight_bwd(_p(x), _p(w), _p(dy), _p(dx), _p(dw), BT, HW, Cc, _stream()), "csts_reweight_bwd")
        return dx, dw, None, None


class TokenMeanFn(Function):
    """x.mean(dim=1)  (custom_multimodal_builder.py:493-494)."""

    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        x = x.contiguous().float()
        B, N, Cc = x.shape
        out = torch.empty(B, Cc, dtype=torch.float32, device=x.device)
        L.check(_lib().csts_token_mean_fwd(_p(x), _p(out), B, N, Cc, _stream()), "csts_token_mean_fwd")
        ctx.meta = (B, N, Cc)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, N, Cc = ctx.meta
        dout = dout.contiguous().float()
        dx = torch.empty(B, N, Cc, dtype=torch.float32, device=dout.device)
        L.check(_lib().csts_token_mean_bwd(_p(dout), _p(dx), B, N, Cc, _stream()), "csts_token_mean_bwd")
        return dx


class AddFn(Function):
    """a + b (decoder encoder-skip adds, custom_multimodal_builder.py:467,470,473)."""

    @staticmethod
    def forward(ctx, a, b):
        _need_gpu(a, b)
        a = a.contiguous()
        b = b.contiguous()
        out = torch.empty_like(a)
        L.check(_lib().csts_axpby(_p(a), _dt(a), _p(b), _dt(b), _p(out), _dt(out), a.numel(), 1.0, 1.0, _stream()), "csts_axpby")
        ctx.bdtype = b.dtype
        return out

    @staticmethod
    def backward(ctx, d):
        return d, (d if d.dtype == ctx.bdtype else d.to(ctx.bdtype))


class TapFn(Function):
    """Identity with two outputs for a residual-stream tensor that has TWO consumers (the encoder features the decoder
    skips re-use, custom_multimodal_builder.py:384-403,467-479): both gradients meet in ONE backward kernel
    (d = d_a + d_b, plus the bf16 copy the next block's GEMMs read) instead of autograd's own in-place accumulation."""

    @staticmethod
    def forward(ctx, x, compute: int):
        _need_gpu(x)
        ctx.compute = compute
        ctx.copy_scale = getattr(x, "_csts_prod_scale", None)     # x = f(...) * s + residual: its gradient's next reader wants s * dx
        ctx.set_materialize_grads(False)
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, da, db):
        if da is None or db is None:
            return (da if da is not None else db), None
        da, db = da.contiguous(), db.contiguous()
        out = torch.empty(da.shape, dtype=torch.float32, device=da.device)
        want16 = ctx.compute == BF16 and BF16_GRAD_COPY
        out16 = torch.empty(da.shape, dtype=L.half_dtype(), device=da.device) if want16 else None
        cs = ctx.copy_scale if out16 is not None else None
        if cs is not None:
            rows = da.numel() // da.shape[-1]
            if rows % cs[1] != 0 or cs[0].numel() * cs[1] != rows or (cs[1] * da.shape[-1]) % 4 != 0:
                cs = None
        L.check(_lib().csts_add2_scaled_copy(_p(da), _dt(da), _p(db), _dt(db), _p(out), _p(out16), _p(cs[0]) if cs else None,
                                             cs[1] * da.shape[-1] if cs else 4, da.numel(), _stream()), "csts_add2")
        if out16 is not None:
            _attach16(out, out16, cs)
        return out, None


# ----------------------------------------------------------------------------------------- token-axis cat / split
# torch.cat(dim=1) and x[:, :n] / x[:, n:] of (B, N, C) tensors as ONE library launch per direction (csts_copy_token_segments).  Through
# torch the fusion head's joins and cuts were ~30 cat / slice-copy / zero-fill / gradient-add nodes per captured step (0.15 ms of
# 5 us kernels).  CSTS_TOKEN_GLUE=0: the torch ops again (same values: pure copies).
TOKEN_GLUE = os.environ.get("CSTS_TOKEN_GLUE", "1") != "0"


def _copy_segments(pairs, B, Cc, dt):
    """pairs: [(src tensor, src batch stride, src element offset, dst tensor, dst batch stride, dst element offset, rows)]"""
    arr = (L.TokenSegment * len(pairs))()
    for i, (src, sbs, soff, dst, dbs, doff, n) in enumerate(pairs):
        arr[i].src, arr[i].dst = src.data_ptr(), dst.data_ptr()
        arr[i].src_bs, arr[i].dst_bs, arr[i].src_off, arr[i].dst_off, arr[i].n = sbs, dbs, soff, doff, n
    L.check(_lib().csts_copy_token_segments(arr, len(pairs), B, Cc, dt, _stream()), "csts_copy_token_segments")


class CatTokensFn(Function):
    """torch.cat([a, b], dim=1) of (B, Na, C) and (B, Nb, C)."""

    @staticmethod
    def forward(ctx, a, b):
        _need_gpu(a, b)
        a, b = a.contiguous(), b.contiguous()
        B, Na, Cc = a.shape
        Nb = b.shape[1]
        out = torch.empty(B, Na + Nb, Cc, dtype=a.dtype, device=a.device)
        _copy_segments([(a, Na * Cc, 0, out, (Na + Nb) * Cc, 0, Na), (b, Nb * Cc, 0, out, (Na + Nb) * Cc, Na * Cc, Nb)], B, Cc, _dt(a))
        ctx.meta = (B, Na, Nb, Cc)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, Na, Nb, Cc = ctx.meta
        dout = dout.contiguous()
        da = torch.empty(B, Na, Cc, dtype=dout.dtype, device=dout.device)
        db = torch.empty(B, Nb, Cc, dtype=dout.dtype, device=dout.device)
        _copy_segments([(dout, (Na + Nb) * Cc, 0, da, Na * Cc, 0, Na), (dout, (Na + Nb) * Cc, Na * Cc, db, Nb * Cc, 0, Nb)], B, Cc, _dt(dout))
        return da, db


class SplitTokensFn(Function):
    """(x[:, :n], x[:, n:]) of a (B, N, C) tensor as two contiguous tensors."""

    @staticmethod
    def forward(ctx, x, n: int):
        _need_gpu(x)
        x = x.contiguous()
        B, N, Cc = x.shape
        a = torch.empty(B, n, Cc, dtype=x.dtype, device=x.device)
        b = torch.empty(B, N - n, Cc, dtype=x.dtype, device=x.device)
        _copy_segments([(x, N * Cc, 0, a, n * Cc, 0, n), (x, N * Cc, n * Cc, b, (N - n) * Cc, 0, N - n)], B, Cc, _dt(x))
        ctx.meta = (B, N, n, Cc)
        return a, b

    @staticmethod
    def backward(ctx, da, db):
        B, N, n, Cc = ctx.meta
        # a part nobody used has no gradient (None): zeros, like the slice's backward
        ref = da if da is not None else db
        if da is None:
            da = torch.zeros(B, n, Cc, dtype=ref.dtype, device=ref.device)
        if db is None:
            db = torch.zeros(B, N - n, Cc, dtype=ref.dtype, device=ref.device)
        da, db = da.contiguous(), db.contiguous()
        dx = torch.empty(B, N, Cc, dtype=da.dtype, device=da.device)
        _copy_segments([(da, n * Cc, 0, dx, N * Cc, 0, n), (db, (N - n) * Cc, 0, dx, N * Cc, n * Cc, N - n)], B, Cc, _dt(da))
        return dx, None


def cat_tokens(a, b):
    if not TOKEN_GLUE or a.dtype != b.dtype or (a.shape[2] * a.element_size()) % 16:
        return torch.cat([a, b], dim=1)
    return CatTokensFn.apply(a, b)


def split_tokens(x, n: int):
    if not TOKEN_GLUE or (x.shape[2] * x.element_size()) % 16:
        return x[:, :n, :], x[:, n:, :]
    return SplitTokensFn.apply(x, n)


def tap(x, compute):
    """(x_a, x_b): two aliases of x, one per consumer."""
    return TapFn.apply(x, compute)


# ----------------------------------------------------------------------------------------- activation checkpointing
class _GradCatch(Function):
    """Identity in front of a recomputed block: its backward keeps the block-input gradient -- the very tensor object the block's
    first LayerNorm returned, with the 16-bit copy attached to it (_attach16) -- for CheckpointFn to pass on, and gives autograd
    nothing to accumulate."""

    @staticmethod
    def forward(ctx, x, box):
        ctx.box = box
        ctx.set_materialize_grads(False)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.box.append(g)
        return None, None


class CheckpointFn(Function):
    """One encoder block as ONE autograd node (MODEL.ACT_CHECKPOINT: fairscale's checkpoint_wrapper around every video / audio
    encoder block, custom_multimodal_builder.py:154,178,214).  Forward runs the block without a tape and keeps its input, the token
    grid, the drop-path scales, the dropout key and the stream; backward re-runs the block with a tape on that stream -- same
    kernels, same scales, same key, hence the same masks -- and back-propagates through the fresh sub-graph as a nested pass
    (nested_backward): the block's parameter gradients reach the parameters there (AccumulateGrad, or the nested pass's own
    end-of-pass hand-over), and the recomputed activations are gone when this node returns."""

    @staticmethod
    def forward(ctx, x, block, thw, km, lane, box):
        _need_gpu(x)
        ctx.block, ctx.thw, ctx.km, ctx.lane = block, list(thw), km, lane
        ctx.key = block.rt.drop_key
        ctx.stream = torch.cuda.current_stream()
        ctx.prod_scale = getattr(x, "_csts_prod_scale", None)
        ctx.save_for_backward(x)
        ctx.set_materialize_grads(False)
        with torch.no_grad():
            out, q_thw, _ = block(x, thw, km)
        box["thw"], box["prod_scale"] = q_thw, getattr(out, "_csts_prod_scale", None)
        return out

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None, None, None, None, None, None
        x, = ctx.saved_tensors
        block, rt = ctx.block, ctx.block.rt
        caught = []
        key_now, rt.drop_key = rt.drop_key, ctx.key
        try:
            with torch.cuda.stream(ctx.stream), nested_backward(ctx.lane):
                with torch.enable_grad():
                    xin = _GradCatch.apply(x.detach().requires_grad_(True), caught)
                    if ctx.prod_scale is not None:      # what the producer of x left for the LayerNorm that reads it
                        xin._csts_prod_scale = ctx.prod_scale
                    out, _, _ = block(xin, ctx.thw, ctx.km)
                torch.autograd.backward(out, dy)
                del out, xin
        finally:
            rt.drop_key = key_now
        return (caught[0] if caught else None), None, None, None, None, None


def checkpoint_block(block, x, thw, km=None, lane=0):
    """block(x, thw, km) -> (out, thw_out, None) with the block's activations recomputed in backward (CheckpointFn).  The
    drop-path scales are fixed here, once, so that both runs of the block read the same tensors.  lane: see nested_backward."""
    s1, s2 = block._drop_scales(x.shape[0], x.device, km)
    km = ("scales", s1, s2) if s1 is not None else None
    if not x.requires_grad:             # nothing in front of the block trains: the node still has to run for the block's own parameters
        x = x.detach().requires_grad_(True)
    box = {}
    out = CheckpointFn.apply(x, block, thw, km, lane, box)
    if box["prod_scale"] is not None:
        out._csts_prod_scale = box["prod_scale"]
    return out, box["thw"], None


def cast(x: torch.Tensor, dt: int) -> torch.Tensor:
    out = torch.empty(x.shape, dtype=torch_dtype(dt), device=x.device)
    x = x.contiguous()
    L.check(_lib().csts_axpby(_p(x), _dt(x), None, 0, _p(out), dt, x.numel(), 1.0, 0.0, _stream()), "csts_axpby(cast)")
    return out


def cast_into(dst: torch.Tensor, src: torch.Tensor, scale: float = 1.0):
    """dst = scale * src across dtypes (flat gradient buckets: fp32 -> the 16-bit type before the all-reduce).  GPU: one
    vectorised csts_axpby launch; CPU tensors (the gloo tests of the bucket logic): torch."""
    assert dst.numel() == src.numel() and dst.is_contiguous() and src.is_contiguous()
    if not dst.is_cuda:
        dst.copy_(src if scale == 1.0 else src * scale)
        return dst
    L.check(_lib().csts_axpby(_p(src), _dt(src), None, 0, _p(dst), _dt(dst), src.numel(), float(scale), 0.0, _stream()), "csts_axpby(cast)")
    return dst


def reweight(x, w, T, HW):
    return ReweightFn.apply(x, w, T, HW)


def token_mean(x):
    return TokenMeanFn.apply(x)


def add(a, b):
    return AddFn.apply(a, b)


# ----------------------------------------------------------------------------------------- head + losses
class ClassifierFn(Function):
    """classifier(feat + F.interpolate(en_feat, (2T', H, W), 'trilinear'))  with classifier = Conv3d(96, 1, 1)
    (custom_multimodal_builder.py:476-481)."""

    @staticmethod
    def forward(ctx, feat, en_feat, w, b, thw_en, compute: int = F32):
        _need_gpu(feat, en_feat)
        ctx.compute = compute
        feat = feat.contiguous()
        en_feat = en_feat.contiguous()
        B, N2, Cc = feat.shape
        out_thw = [thw_en[0] * 2, thw_en[1], thw_en[2]]
        g = _pool_geom(B, Cc, thw_en, out_thw, (2, 1, 1))
        z = torch.empty_like(feat)
        L.check(_lib().csts_trilinear_fwd(C.byref(g), _p(en_feat), _dt(en_feat), _p(feat), _dt(feat), _p(z), _dt(z), _stream()),
                "csts_trilinear_fwd(head)")
        logits = torch.empty(B * N2, dtype=torch.float32, device=feat.device)
        wf = w.reshape(-1).contiguous()
        L.check(_lib().csts_rowdot_fwd(_p(z), _dt(z), _p(wf), _p(b), _p(logits), B * N2, Cc, _stream()), "csts_rowdot_fwd")
        ctx.save_for_backward(z, wf)
        ctx.g = g
        ctx.meta = (B, N2, Cc, tuple(w.shape), en_feat.shape, en_feat.dtype)
        return logits.view(B, 1, out_thw[0], out_thw[1], out_thw[2])

    @staticmethod
    def backward(ctx, dl):
        z, wf = ctx.saved_tensors
        B, N2, Cc, wshape, enshape, endtype = ctx.meta
        dl = dl.contiguous().view(-1).float()
        M = B * N2
        dz = torch.empty_like(z)
        L.check(_lib().csts_rowdot_dx(_p(dl), _p(wf), _p(dz), _dt(dz), M, Cc, _stream()), "csts_rowdot_dx")
        if ctx.compute == BF16 and BF16_GRAD_COPY and dz.dtype == torch.float32:
            # the last decoder block has no drop-path and nothing else would give its GEMMs a bf16 copy of this gradient:
            # without one its two data-gradient GEMMs and its weight gradients stream the fp32 tensor (M = 262 k rows)
            dz16 = torch.empty(dz.shape, dtype=L.half_dtype(), device=dz.device)
            L.check(_lib().csts_rowdot_dx(_p(dl), _p(wf), _p(dz16), BF16, M, Cc, _stream()), "csts_rowdot_dx(bf16)")
            _attach16(dz, dz16)
        dw = colsum(z, 1, M, Cc, row_weight=dl).view(wshape)
        db = colsum(dl, 1, M, 1)
        den = torch.empty(enshape, dtype=endtype, device=dl.device)
        L.check(_lib().csts_trilinear_bwd(C.byref(ctx.g), _p(dz), _dt(dz), _p(den), _dt(den), _stream()), "csts_trilinear_bwd(head)")
        return dz, den, dw, db, None, None


def classifier_head(feat, en_feat, w, b, thw_en, compute: int = F32):
    return ClassifierFn.apply(feat, en_feat, w, b, list(thw_en), compute)


class FrameSoftmaxFn(Function):
    """frame_softmax(logits, temperature): softmax over H*W per (b, t)  (slowfast/utils/utils.py:5-12)."""

    @staticmethod
    def forward(ctx, logits, temperature: float):
        _need_gpu(logits)
        x = logits.contiguous().float()
        n = x.shape[-1] * x.shape[-2]
        rows = x.numel() // n
        p = torch.empty_like(x)
        L.check(_lib().csts_softmax_fwd(_p(x), _p(p), rows, n, temperature, _stream()), "csts_softmax_fwd")
        ctx.save_for_backward(x)
        ctx.meta = (rows, n, temperature)
        return p

    @staticmethod
    def backward(ctx, dp):
        (x,) = ctx.saved_tensors
        rows, n, temperature = ctx.meta
        dp = dp.contiguous().float()
        dx = torch.empty_like(x)
        L.check(_lib().csts_softmax_bwd(_p(x), _p(dp), _p(dx), rows, n, temperature, _stream()), "csts_softmax_bwd")
        return dx, None


class KLDivFn(Function):
    """KLDiv.forward (slowfast/models/losses.py:59-82): sum_t KL(p || q) / (T log HW), mean over batch."""

    @staticmethod
    def forward(ctx, pred, target):
        _need_gpu(pred)
        p = pred.contiguous().float()
        B, T, H, W = p.shape[0], p.shape[2], p.shape[3], p.shape[4]
        n = H * W
        rows = p.numel() // n
        q = target.contiguous().float() if target is not None else None
        scale = 1.0 / (T * math.log(n) * B)
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        ws = torch.empty(rows, dtype=torch.float32, device=p.device)
        L.check(_lib().csts_kldiv_fwd(_p(p), _p(q), _p(loss), _p(ws), rows, n, scale, _stream()), "csts_kldiv_fwd")
        if q is None:   # uniform prior: - log(1/HW) per frame (losses.py:69-73)
            loss = loss + math.log(n) * T * B * scale
        ctx.save_for_backward(p, q)
        ctx.meta = (rows, n, scale)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        p, q = ctx.saved_tensors
        rows, n, scale = ctx.meta
        g = g.contiguous().float().view(1)
        dp = torch.empty_like(p)
        L.check(_lib().csts_kldiv_bwd(_p(p), _p(q), _p(g), _p(dp), rows, n, scale, _stream()), "csts_kldiv_bwd")
        return dp, None


class RowNormFn(Function):
    """a / max(||a||, eps) per row (sim_matrix, slowfast/utils/utils.py:20-22)."""

    @staticmethod
    def forward(ctx, a, eps: float):
        _need_gpu(a)
        a = a.contiguous().float()
        rows, D = a.shape
        an = torch.empty_like(a)
        nrm = torch.empty(rows, dtype=torch.float32, device=a.device)
        L.check(_lib().csts_rownorm_fwd(_p(a), _p(an), _p(nrm), rows, D, eps, _stream()), "csts_rownorm_fwd")
        ctx.save_for_backward(a, nrm)
        ctx.eps = eps
        return an

    @staticmethod
    def backward(ctx, dan):
        a, nrm = ctx.saved_tensors
        dan = dan.contiguous().float()
        da = torch.empty_like(a)
        L.check(_lib().csts_rownorm_bwd(_p(a), _p(nrm), _p(dan), _p(da), a.shape[0], a.shape[1], ctx.eps, _stream()),
                "csts_rownorm_bwd")
        return da, None


class EgoNCEFn(Function):
    """EgoNCE.forward (slowfast/models/losses.py:157-170), temperature 0.05."""

    @staticmethod
    def forward(ctx, sim, temperature: float):
        _need_gpu(sim)
        x = sim.contiguous().float()
        n = x.shape[0]
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        lr = torch.empty(n, dtype=torch.float32, device=x.device)
        lc = torch.empty_like(lr)
        L.check(_lib().csts_egonce_fwd(_p(x), _p(loss), _p(lr), _p(lc), n, temperature, _stream()), "csts_egonce_fwd")
        ctx.save_for_backward(x, lr, lc)
        ctx.meta = (n, temperature)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        x, lr, lc = ctx.saved_tensors
        n, temperature = ctx.meta
        g = g.contiguous().float().view(1)
        dx = torch.empty_like(x)
        L.check(_lib().csts_egonce_bwd(_p(x), _p(lr), _p(lc), _p(g), _p(dx), n, temperature, _stream()), "csts_egonce_bwd")
        return dx, None


def frame_softmax(logits, temperature):
    return FrameSoftmaxFn.apply(logits, float(temperature))


def kldiv(pred, target=None):
    return KLDivFn.apply(pred, target)


def sim_matrix(a, b, eps=1e-8):
    an = RowNormFn.apply(a, eps)
    bn = RowNormFn.apply(b, eps)
    return linear(an, bn, None, out_dt=F32, compute=F32)


def egonce(sim, temperature=0.05):
    return EgoNCEFn.apply(sim, float(temperature))


# ----------------------------------------------------------------------------------------- inference head
_DECODE_OUTPUTS = ("preds", "rescaled", "points", "peak")


def _wanted(want, allowed, table, device):
    """The outputs of a wrapper that computes only what `want` names: {name: an empty tensor} for the rows (name, shape, dtype)
    of `table` that are wanted.  A name outside `allowed`, or no name at all, is a ValueError."""
    want = tuple(want)
    if not want or [k for k in want if k not in allowed]:
        raise ValueError(f"want must name some of {allowed}, got {want}")
    return {k: torch.empty(shape, dtype=dt, device=device) for k, shape, dt in table if k in want}


def _track_table(n, h, w):
    """The per-frame outputs of the track wrappers for n frames of h x w maps, as _wanted takes them; each wrapper allows its own
    subset of the names."""
    f32, i32 = torch.float32, torch.int32
    return (("heatmaps", (n, h, w), f32), ("rescaled", (n, h, w), f32), ("points", (n, 2), f32), ("peak", (n,), f32),
            ("count", (n,), i32), ("neighbours", (n, 2), i32))


def gaze_decode(logits, temperature=2.0, want=_DECODE_OUTPUTS):
    """csts_gaze_decode on the (B, 1, T, H, W) model output (fp32 or the library's 16-bit type): one read of each frame's logits
    gives preds = frame_softmax(logits, temperature) and rescaled = its per-frame min-max rescale (tools/test_avgaze_net.py:68-70),
    both fp32 shaped like logits, points (B, T, 2) = (x, y) of the frame's maximum in [0, 1) and peak (B, T) = its probability.
    Returns a dict of the outputs named in `want`; the others are not computed.  Inference only: raises when the logits
    carry a gradient.  No host sync: it can be captured in a graph."""
    _need_gpu(logits)
    if logits.requires_grad and torch.is_grad_enabled():
        raise L.CstsError("gaze_decode is the inference head: it has no backward (call it under torch.no_grad(), or use "
                          "frame_softmax for a differentiable heat map)")
    if logits.dim() != 5 or logits.shape[1] != 1:
        raise ValueError(f"logits must be (B, 1, T, H, W), got {tuple(logits.shape)}")
    B, _, T, H, W = logits.shape
    f32 = torch.float32
    out = _wanted(want, _DECODE_OUTPUTS, (("preds", logits.shape, f32), ("rescaled", logits.shape, f32), ("points", (B, T, 2), f32),
                                          ("peak", (B, T), f32)), logits.device)
    x = logits.detach().contiguous()                             # after `want` is checked: a refusal launches nothing
    L.check(_lib().csts_gaze_decode(_p(x), _dt(x), B * T, H, W, float(temperature), _p(out.get("preds")), _p(out.get("rescaled")),
                                    _p(out.get("points")), _p(out.get("peak")), _stream()), "csts_gaze_decode")
    return out


_TRACK_OUTPUTS = ("heatmaps", "rescaled", "points", "peak", "count")


def _target_lists(target_idx, n_frames):
    """int64 (P,) target frames -> the device lists csts_gaze_track / csts_attention_track take: order int32 (P,) = the rows
    sorted by target (stable: ascending row within a frame), offsets int32 (n_frames + 1,) = each frame's bounds in it.  Targets
    outside [0, n_frames) go to a discard bucket behind the last frame.  No host sync."""
    inside = (target_idx >= 0) & (target_idx < n_frames)
    bucket = torch.where(inside, target_idx, torch.full_like(target_idx, n_frames))      # n_frames: the discard bucket
    sorted_t, order = torch.sort(bucket, stable=True)
    offsets = torch.searchsorted(sorted_t, torch.arange(n_frames + 1, device=target_idx.device, dtype=torch.int64))
    return order.to(torch.int32), offsets.to(torch.int32)


def gaze_track(preds, target_idx, n_frames, want=_TRACK_OUTPUTS):
    """csts_gaze_track: P per-window heat maps preds (P, H, W) fp32, each predicting video frame target_idx[p] (int64 (P,)), ->
    one entry per frame of the video: heatmaps (n_frames, H, W) = the mean of the maps that target the frame (added in
    ascending p), rescaled = its min-max rescale, points (n_frames, 2) and peak (n_frames,) as gaze_decode defines them on
    that mean, count (n_frames,) int32 = how many maps the frame got.  Frames nobody predicts: maps 0, points NaN, peak 0.
    Targets outside [0, n_frames) are dropped.  The row lists are built on the device (stable sort by target; the list
    bounds by a binary search of the sorted targets, which unlike torch.bincount reads nothing back): no host sync."""
    _need_gpu(preds, target_idx)
    if preds.dim() != 3 or preds.dtype != torch.float32:
        raise ValueError(f"preds must be fp32 (P, H, W), got {tuple(preds.shape)} {preds.dtype}")
    P, H, W = preds.shape
    n_frames = int(n_frames)
    if target_idx.dtype != torch.int64 or tuple(target_idx.shape) != (P,):
        raise ValueError(f"target_idx must be int64 ({P},), got {tuple(target_idx.shape)} {target_idx.dtype}")
    if n_frames < 1 or P < 1:
        raise ValueError(f"gaze_track needs P >= 1 maps and n_frames >= 1, got {P} and {n_frames}")
    out = _wanted(want, _TRACK_OUTPUTS, _track_table(n_frames, H, W), preds.device)
    x = preds.detach().contiguous()
    order, offsets = _target_lists(target_idx, n_frames)
    L.check(_lib().csts_gaze_track(_p(x), _p(order), _p(offsets), n_frames, H, W, _p(out.get("heatmaps")), _p(out.get("rescaled")),
                                   _p(out.get("points")), _p(out.get("peak")), _p(out.get("count")), _stream()), "csts_gaze_track")
    return out


_FILL_OUTPUTS = ("heatmaps", "rescaled", "points", "peak", "neighbours")
_FILL_MODES = ("hold", "linear")        # the kernel's mode is the position


def gaze_track_fill(heatmaps, count, mode="linear", max_gap=9, want=_FILL_OUTPUTS):
    """csts_gaze_track_fill: the sparse track of gaze_track -- heatmaps fp32 (F, H, W) and count int32 (F,) -- with every frame
    between two neighbouring predictions filled.  A frame with count > 0 passes through bit for bit; a frame with count 0 whose
    nearest predicted neighbours a < n < b lie at most max_gap frames apart gets H_a (mode "hold") or the time-linear blend
    ((b - n) H_a + (n - a) H_b) / (b - a) (mode "linear"); any other frame stays unpredicted (maps 0, points NaN, peak 0).
    rescaled, points and peak are decoded from the new map as gaze_track decodes them; neighbours int32 (F, 2) = (a, b),
    (n, n) on a predicted frame, (-1, -1) on an unpredicted one.  Nothing is extrapolated outside the predicted span.
    Returns a dict of the outputs named in `want` (new tensors: the inputs are not written).  One launch, no host sync: it can
    be captured in a graph.  The rule is stated in include/csts_hip.h and restated on the host by infer.fill_plan."""
    _need_gpu(heatmaps, count)
    if mode not in _FILL_MODES:
        raise ValueError(f"mode must be one of {_FILL_MODES}, got {mode!r}")
    if heatmaps.dim() != 3 or heatmaps.dtype != torch.float32:
        raise ValueError(f"heatmaps must be fp32 (F, H, W), got {tuple(heatmaps.shape)} {heatmaps.dtype}")
    F, H, W = heatmaps.shape
    if count.dtype != torch.int32 or tuple(count.shape) != (F,):
        raise ValueError(f"count must be int32 ({F},), got {tuple(count.shape)} {count.dtype}")
    if F < 1:
        raise ValueError(f"gaze_track_fill needs F >= 1 frames, got {F}")
    out = _wanted(want, _FILL_OUTPUTS, _track_table(F, H, W), heatmaps.device)
    x = heatmaps.detach().contiguous()
    c = count.contiguous()
    L.check(_lib().csts_gaze_track_fill(_p(x), _p(c), F, H, W, _FILL_MODES.index(mode), int(max_gap), _p(out.get("heatmaps")),
                                        _p(out.get("rescaled")), _p(out.get("points")), _p(out.get("peak")),
                                        _p(out.get("neighbours")), _stream()), "csts_gaze_track_fill")
    return out


# ----------------------------------------------------------------------------------------- live gaze track
_LIVE_OUTPUTS = ("heatmaps", "rescaled", "points", "peak", "count", "neighbours")


def live_track_ring(slots, h, w, device):
    """An empty track ring of `slots` frames of h x w maps on `device`: {"sum" fp32 (slots, h, w) zeros, "count" int32 (slots,)
    zeros, "frame" int64 (slots,) -1}.  Frame t lives in slot t mod slots (include/csts_hip.h, live gaze track)."""
    return _new_track_ring((), slots, h, w, device)


def _ring_sizes_ok(lead, Rt, h, w):
    """The sizes a track ring, or with lead = (streams,) an arena of them, may have; ValueError otherwise."""
    if Rt < 1 or Rt > 65535 or h < 1 or w < 1 or h * w > L.GAZE_DECODE_MAX_HW:
        raise ValueError(f"a track ring holds 1..65535 slots of maps with h * w <= {L.GAZE_DECODE_MAX_HW}, got {Rt} of {h} x {w}")
    if lead and (lead[0] < 1 or lead[0] > 65535 or lead[0] * Rt >= 2 ** 31):
        raise ValueError(f"a track arena holds 1..65535 rings and fewer than 2^31 slots, got {lead[0]} rings of {Rt}")


def _new_track_ring(lead, slots, h, w, device):
    """live_track_ring (lead = ()) and group_live_ring (lead = (streams,)): the same three tensors under `lead`."""
    lead, slots, h, w = tuple(int(v) for v in lead), int(slots), int(h), int(w)
    _ring_sizes_ok(lead, slots, h, w)
    device = torch.device(device)
    if device.type != "cuda":
        raise L.CstsError(f"the track {'arena' if lead else 'ring'} lives on MI355X only (there is no CPU fallback)")
    return {"sum": torch.zeros(*lead, slots, h, w, dtype=torch.float32, device=device),
            "count": torch.zeros(*lead, slots, dtype=torch.int32, device=device),
            "frame": torch.full((*lead, slots), -1, dtype=torch.int64, device=device)}


def _check_live_ring(ring, arena=False):
    """The three tensors of a track ring, or of an arena of rings, checked: (sum, count, frame, streams, Rt, h, w); streams is
    None for a single ring."""
    try:
        s, c, f = ring["sum"], ring["count"], ring["frame"]
    except (KeyError, TypeError, IndexError):
        raise ValueError(f"ring must be a dict with \"sum\", \"count\" and \"frame\" (ops.{'group_live_ring' if arena else 'live_track_ring'})")
    _need_gpu(s, c, f)
    if s.dim() != (4 if arena else 3) or s.dtype != torch.float32 or not s.is_contiguous():
        raise ValueError(f"ring[\"sum\"] must be contiguous fp32 ({'streams, ' if arena else ''}Rt, h, w), got {tuple(s.shape)} {s.dtype}")
    slots = tuple(s.shape[:-2])                                  # (Rt,), or (streams, Rt) in an arena: one count and tag each
    if c.dtype != torch.int32 or tuple(c.shape) != slots or not c.is_contiguous():
        raise ValueError(f"ring[\"count\"] must be contiguous int32 {slots}, got {tuple(c.shape)} {c.dtype}")
    if f.dtype != torch.int64 or tuple(f.shape) != slots or not f.is_contiguous():
        raise ValueError(f"ring[\"frame\"] must be contiguous int64 {slots}, got {tuple(f.shape)} {f.dtype}")
    Rt, h, w = s.shape[-3:]
    _ring_sizes_ok(slots[:-1], Rt, h, w)
    return s, c, f, (slots[0] if arena else None), Rt, h, w


def _check_live_maps(name, maps, target_idx, h, w):
    """The maps and device targets of live_track_add / group_live_add, checked against the ring's h x w -> P, their number."""
    if maps.dim() != 3 or maps.dtype != torch.float32 or tuple(maps.shape[1:]) != (h, w):
        raise ValueError(f"maps must be fp32 (P, {h}, {w}), got {tuple(maps.shape)} {maps.dtype}")
    P = maps.shape[0]
    if target_idx.dtype != torch.int64 or tuple(target_idx.shape) != (P,):
        raise ValueError(f"target_idx must be int64 ({P},), got {tuple(target_idx.shape)} {target_idx.dtype}")
    if P < 1 or P > 65535:
        raise ValueError(f"{name} takes 1..65535 maps a call, got {P}")
    return P


def _live_host_table(values, n, name, of):
    """The host copy of a device table of n integers, as an int64 numpy array."""
    import numpy as np
    if torch.is_tensor(values):
        raise ValueError(f"{name} is the host copy of {of}: a sequence or numpy array of ints, not a tensor")
    host = np.asarray(values)
    if host.shape != (n,) or not np.issubdtype(host.dtype, np.integer):
        raise ValueError(f"{name} must hold the {n} entries of {of} as integers on the host, got shape {host.shape} {host.dtype}")
    return host.astype(np.int64)


def _check_rows_mode(mode, max_gap):
    """The fill rule of live_track_rows / group_live_rows, checked -> max_gap as an int."""
    if mode not in _FILL_MODES:
        raise ValueError(f"mode must be one of {_FILL_MODES}, got {mode!r}")
    max_gap = int(max_gap)
    if max_gap < 1 or max_gap > L.GAZE_FILL_MAX_GAP:
        raise ValueError(f"max_gap must lie in 1..{L.GAZE_FILL_MAX_GAP}, got {max_gap}")
    return max_gap


def live_track_add(maps, target_idx, targets, ring, live_from=0):
    """csts_live_track_add: the maps of newly run windows, fp32 (P, h, w), each predicting frame target_idx[p] (int64 (P,) on the
    device), folded into the track ring (ops.live_track_ring) in place.  A slot whose frame tag differs from the target restarts
    (sum = the map, count 1, retagged: stale slots are recycled without a clearing pass); a slot whose tag matches is added to in
    ascending p and its count bumped -- the order and the arithmetic of ops.gaze_track, when the windows come in the order they ran.
    targets: the same P targets on the HOST (a sequence or numpy array of ints; the stream has them from stream_window), so
    that what cannot be written is refused before the launch and without a host sync: a negative target, and a target
    t >= live_from + Rt, which would overwrite the slot of frame t - Rt >= live_from.  live_from: the lowest frame whose row may
    still be asked for, minus max_gap - 1 (a row reads that far back).  One launch, no atomics, no host sync."""
    _need_gpu(maps, target_idx)
    s, c, f, _, Rt, h, w = _check_live_ring(ring)
    P = _check_live_maps("live_track_add", maps, target_idx, h, w)
    host = _live_host_table(targets, P, "targets", "target_idx")
    live_from = int(live_from)
    if int(host.min()) < 0:
        raise ValueError(f"targets must be frame numbers >= 0, got {int(host.min())}")
    if int(host.max()) >= live_from + Rt:
        t = int(host.max())
        raise ValueError(f"the track ring holds {Rt} frames: target {t} would overwrite the slot of frame {t - Rt}, which is still "
                         f"inside the live span (it starts at frame {live_from}); nothing was written")
    x = maps.detach().contiguous()
    L.check(_lib().csts_live_track_add(_p(x), _p(target_idx.contiguous()), P, h, w, _p(s), _p(c), _p(f), Rt, _stream()),
            "csts_live_track_add")


def live_track_rows(ring, f0, K, mode="linear", max_gap=9, want=_LIVE_OUTPUTS):
    """csts_live_track_rows: the track rows of frames f0 .. f0 + K - 1 out of the track ring.  Row n is row n of
    ops.gaze_track_fill(mode, max_gap) of ops.gaze_track(everything added so far, n_frames = n + max_gap + 1), bit for bit, as long
    as the frames in [n - max_gap + 1, n + max_gap - 1] have not been recycled (live_track_add's live_from): heatmaps and rescaled
    (K, h, w), points (K, 2), peak (K,), count int32 (K,) (0 on a filled or unpredicted frame) and neighbours int32 (K, 2).  A
    slot that holds another frame counts as empty.  Returns the outputs named in `want`; the others are not computed.  The ring
    is only read.  One launch, no host sync: it can be captured in a graph."""
    s, c, f, _, Rt, h, w = _check_live_ring(ring)
    max_gap = _check_rows_mode(mode, max_gap)
    f0, K = int(f0), int(K)
    if f0 < 0 or K < 1 or K > 65535 or f0 + K + max_gap >= 2 ** 31:
        raise ValueError(f"live_track_rows answers 1..65535 frames from f0 >= 0 with f0 + K + max_gap < 2^31, got f0 {f0}, K {K}")
    out = _wanted(want, _LIVE_OUTPUTS, _track_table(K, h, w), s.device)
    L.check(_lib().csts_live_track_rows(_p(s), _p(c), _p(f), Rt, f0, K, h, w, _FILL_MODES.index(mode), max_gap,
                                        _p(out.get("heatmaps")), _p(out.get("rescaled")), _p(out.get("points")), _p(out.get("peak")),
                                        _p(out.get("count")), _p(out.get("neighbours")), _stream()), "csts_live_track_rows")
    return out


# ----------------------------------------------------------------------------------------- live gaze track of a stream group
def group_live_ring(streams, slots, h, w, device):
    """An empty arena of `streams` track rings of `slots` frames of h x w maps on `device`: {"sum" fp32 (streams, slots, h, w)
    zeros, "count" int32 (streams, slots) zeros, "frame" int64 (streams, slots) -1}.  Frame t of slot i lives at [i, t mod slots];
    the ring of slot i is the ring live_track_ring(slots, h, w) describes (include/csts_hip.h, live track of a stream group)."""
    return _new_track_ring((streams,), slots, h, w, device)


def group_live_add(maps, target_idx, stream_of, targets, streams_host, ring, live_from):
    """csts_group_live_add: live_track_add for the slots of a track arena (ops.group_live_ring), in ONE launch.  maps fp32 (P, h, w),
    row p predicting frame target_idx[p] (int64 (P,) on the device) of slot stream_of[p] (int32 (P,) on the device); the ring of
    slot i takes the rows with stream_of[p] == i in ascending p by live_track_add's rule -- restart or carry on, the same
    arithmetic -- so it ends as live_track_add leaves it on those rows alone.  A ring slot no row names is not touched.
    targets, streams_host: the same two tables on the HOST (sequences or numpy arrays of ints), so that what cannot be written is
    refused before the launch and without a host sync: a negative target, a stream outside [0, streams), and a target
    t >= live_from[i] + Rt on its slot i, which would overwrite the slot of frame t - Rt >= live_from[i].  live_from: one entry
    per slot of the arena, the lowest frame of that slot whose row may still be asked for, minus max_gap - 1.  A refusal leaves
    the arena untouched.  One launch, no atomics, no host sync."""
    import numpy as np
    _need_gpu(maps, target_idx, stream_of)
    s, c, f, n, Rt, h, w = _check_live_ring(ring, arena=True)
    P = _check_live_maps("group_live_add", maps, target_idx, h, w)
    if stream_of.dtype != torch.int32 or tuple(stream_of.shape) != (P,):
        raise ValueError(f"stream_of must be int32 ({P},), got {tuple(stream_of.shape)} {stream_of.dtype}")
    host_t = _live_host_table(targets, P, "targets", "target_idx")
    host_s = _live_host_table(streams_host, P, "streams_host", "stream_of")
    if torch.is_tensor(live_from):
        raise ValueError("live_from is a sequence of ints on the host, one per slot, not a tensor")
    start = np.asarray(live_from)
    if start.shape != (n,) or not np.issubdtype(start.dtype, np.integer):
        raise ValueError(f"live_from must hold one integer per slot of the arena ({n}), got shape {start.shape} {start.dtype}")
    if int(host_t.min()) < 0:
        raise ValueError(f"targets must be frame numbers >= 0, got {int(host_t.min())}")
    if int(host_s.min()) < 0 or int(host_s.max()) >= n:
        bad = int(host_s.min()) if int(host_s.min()) < 0 else int(host_s.max())
        raise ValueError(f"the arena holds the rings of streams 0..{n - 1}, a row names stream {bad}; nothing was written")
    over = host_t >= start.astype(np.int64)[host_s] + Rt
    if over.any():
        p = int(np.argmax(over))
        t, i = int(host_t[p]), int(host_s[p])
        raise ValueError(f"a track ring holds {Rt} frames: target {t} of stream {i} would overwrite the slot of frame {t - Rt}, which "
                         f"is still inside the live span (it starts at frame {int(start[i])}); nothing was written")
    x = maps.detach().contiguous()
    L.check(_lib().csts_group_live_add(_p(x), _p(target_idx.contiguous()), _p(stream_of.contiguous()), P, h, w, _p(s), _p(c), _p(f),
                                       n, Rt, _stream()), "csts_group_live_add")


def group_live_rows(ring, stream_of, frame_of, mode="linear", max_gap=9, want=_LIVE_OUTPUTS):
    """csts_group_live_rows: live_track_rows over a track arena, in ONE launch: row k answers frame frame_of[k] of slot
    stream_of[k] by live_track_rows' rule on that slot's ring, bit for bit.  stream_of, frame_of: the tables on the HOST
    (sequences or numpy arrays of K ints); they are checked -- frames >= 0 and frame + max_gap < 2^31 -- and uploaded as int32
    and int64.  A stream outside the arena is not refused: its row is the unpredicted one (zero maps, NaN points, peak 0, count
    0, neighbours (-1, -1)).  The outputs are live_track_rows', K rows in the order of the tables, those named in `want`.  The
    arena is only read.  One launch, no host sync."""
    import numpy as np
    s, c, f, n, Rt, h, w = _check_live_ring(ring, arena=True)
    max_gap = _check_rows_mode(mode, max_gap)
    K = len(frame_of)
    if K < 1 or K > 65535:
        raise ValueError(f"group_live_rows answers 1..65535 frames a call, got {K}")
    host_f = _live_host_table(frame_of, K, "frame_of", "the frame table")
    host_s = _live_host_table(stream_of, K, "stream_of", "the stream table")
    if int(host_f.min()) < 0 or int(host_f.max()) + max_gap >= 2 ** 31:
        raise ValueError(f"group_live_rows answers frames >= 0 with frame + max_gap < 2^31, got {int(host_f.min())}..{int(host_f.max())}")
    if int(host_s.min()) < -2 ** 31 or int(host_s.max()) >= 2 ** 31:
        raise ValueError("stream_of holds int32 stream numbers")
    out = _wanted(want, _LIVE_OUTPUTS, _track_table(K, h, w), s.device)
    streams_dev = torch.from_numpy(host_s.astype(np.int32)).to(s.device)
    frames_dev = torch.from_numpy(host_f).to(s.device)
    L.check(_lib().csts_group_live_rows(_p(s), _p(c), _p(f), n, Rt, _p(streams_dev), _p(frames_dev), K, h, w,
                                        _FILL_MODES.index(mode), max_gap, _p(out.get("heatmaps")), _p(out.get("rescaled")),
                                        _p(out.get("points")), _p(out.get("peak")), _p(out.get("count")), _p(out.get("neighbours")),
                                        _stream()), "csts_group_live_rows")
    return out


# ----------------------------------------------------------------------------------------- gaze overlay
def jet_table():
    """The heat colours of gaze_overlay on the host: uint8 numpy (256, 3) RGB, row q = the classic JET by the integer formula of
    include/csts_hip.h, r = clamp(383 - |4q - 765|, 0, 255), g = clamp(383 - |4q - 510|, 0, 255), b = clamp(383 - |4q - 255|, 0, 255)."""
    import numpy as np
    q4 = 4 * np.arange(256, dtype=np.int64)
    return np.stack([np.clip(383 - np.abs(q4 - c), 0, 255) for c in (765, 510, 255)], axis=-1).astype(np.uint8)


def _overlay_params(params, crop_size, device):
    """The params row of gaze_overlay as an int32 device tensor.  A row given on the host (5 integers) is checked against the
    sampler's range and uploaded; a device tensor is taken as it is (the kernel reads it when it runs: no host sync)."""
    if torch.is_tensor(params):
        _need_gpu(params)
        if params.dtype != torch.int32 or params.numel() != 5:
            raise ValueError(f"params must hold 5 int32 values (new h, new w, y0, x0, flip), got {tuple(params.shape)} {params.dtype}")
        return params.contiguous()
    return torch.tensor(_host_params_row(params, crop_size), dtype=torch.int32, device=device)


def _parse_params_row(params):
    """A params row given on the host as five Python ints: (new h, new w, y0, x0, flip)."""
    import numpy as np
    row = np.asarray(params)
    if row.size != 5 or not np.issubdtype(row.dtype, np.integer):
        raise ValueError(f"params must hold 5 integers (new h, new w, y0, x0, flip), got {params!r}")
    return tuple(int(v) for v in row.reshape(5))


def _host_params_row(params, crop_size):
    """A params row given on the host, checked against the sampler's range: [new h, new w, y0, x0, 0]."""
    nh, nw, y0, x0, flip = _parse_params_row(params)
    if flip != 0:
        raise ValueError("gaze_overlay draws test-mode crops, which are never flipped: params has flip != 0")
    S = int(crop_size)
    if nh < S or nw < S or not 0 <= y0 <= nh - S or not 0 <= x0 <= nw - S:
        raise ValueError(f"params {(nh, nw, y0, x0)} do not hold a {S} x {S} crop")
    return [nh, nw, y0, x0, 0]


def _check_overlay_args(name, pairs, rescaled, centers, alpha, radius, crop_size, per_job=False):
    """What gaze_overlay, gaze_overlay_yuv and group_gaze_overlay (`name`) check alike -> (alpha, radius, crop_size) as float, int,
    int.  pairs: [(frames, out or None)], the frames already checked for dtype and dimensions; rescaled fp32 (N, mh, mw) and
    centers int32 (N, 2) or None hold one row per frame of all the pairs.  alpha lies in [0, 1], radius is >= 0, crop_size and N
    are >= 1; frames are contiguous and an `out` is a contiguous uint8 tensor of its frames' shape, the message about pair j
    prefixed "job j: " with per_job."""
    N = sum([int(frames.shape[0]) for frames, _ in pairs])
    if rescaled.dtype != torch.float32 or rescaled.dim() != 3 or rescaled.shape[0] != N:
        raise ValueError(f"rescaled must be fp32 ({N}, mh, mw), got {tuple(rescaled.shape)} {rescaled.dtype}")
    if centers is not None and (centers.dtype != torch.int32 or tuple(centers.shape) != (N, 2)):
        raise ValueError(f"centers must be int32 ({N}, 2), got {tuple(centers.shape)} {centers.dtype}")
    alpha, radius, S = float(alpha), int(radius), int(crop_size)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must lie in [0, 1], got {alpha}")
    if radius < 0 or S < 1 or N < 1:
        raise ValueError(f"{name} needs N >= 1 frames, crop_size >= 1 and radius >= 0, got {N}, {S} and {radius}")
    for j, (frames, out) in enumerate(pairs):
        job = f"job {j}: " if per_job else ""
        if not frames.is_contiguous():
            raise ValueError(f"{job}frames must be contiguous")
        if out is not None and (out.dtype != torch.uint8 or out.shape != frames.shape or not out.is_contiguous()):
            raise ValueError(f"{job}out must be contiguous uint8 {tuple(frames.shape)}, got {tuple(out.shape)} {out.dtype}")
    return alpha, radius, S


def gaze_overlay(frames_u8, rescaled, params, crop_size, centers=None, alpha=0.4, radius=5, out=None):
    """csts_gaze_overlay: frames uint8 (N, H, W, 3) RGB + rescaled fp32 (N, mh, mw) in [0, 1] (gaze_decode / gaze_track) -> uint8
    (N, H, W, 3): inside the crop that `params` (new h, new w, y0, x0, flip = 0: the row of inputs.spatial_sample / clip_sample,
    5 integers on the host or an int32 device tensor) cut out of the frame, (1 - alpha) frame + alpha JET(map), the map sampled
    bilinearly; outside it the frame; a filled (0, 255, 0) disc of `radius` pixels at centers int32 (N, 2) = (X, Y) in source
    pixels.  A frame whose centre X is negative comes back untouched; centers=None draws no markers.  out=frames_u8 renders
    in place.  One launch, no host sync: it can be captured in a graph.  The rule is stated in include/csts_hip.h."""
    _need_gpu(frames_u8, rescaled, centers, out)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError(f"frames must be uint8 (N, H, W, 3), got {tuple(frames_u8.shape)} {frames_u8.dtype}")
    N, H, W, _ = frames_u8.shape
    alpha, radius, S = _check_overlay_args("gaze_overlay", [(frames_u8, out)], rescaled, centers, alpha, radius, crop_size)
    if out is None:
        out = torch.empty_like(frames_u8)
    par = _overlay_params(params, S, frames_u8.device)
    maps = rescaled.detach().contiguous()
    cen = None if centers is None else centers.contiguous()
    L.check(_lib().csts_gaze_overlay(_p(frames_u8), _p(maps), _p(cen), _p(par), _p(out), N, H, W, S, maps.shape[1], maps.shape[2],
                                     alpha, radius, _stream()), "csts_gaze_overlay")
    return out


def gaze_overlay_yuv(frames_yuv, rescaled, params, crop_size, pixel_format, matrix="bt601", full_range=False, centers=None,
                     alpha=0.4, radius=5, out=None, window=None):
    """csts_gaze_overlay_yuv: gaze_overlay drawn onto 4:2:0 frames uint8 (N, H * 3 / 2, W) in `pixel_format` ("nv12" | "i420",
    with `matrix` and `full_range` as inputs.yuv_to_rgb takes them) -> uint8 of the same shape and layout, 1.5 bytes in and 1.5
    out per pixel and no RGB picture in memory.  With D = gaze_overlay(inputs.yuv_to_rgb(frames), ...) and M the drawn mask
    (inside the crop of a frame with centre X >= 0 or centers=None, or under the disc), out = where(M, inputs.rgb_to_yuv(D),
    frames), M per pixel for luma and per 2 x 2 block (any) for chroma: an untouched frame, row pair or block comes back byte
    for byte, and a drawn pixel is re-encoded even at alpha = 0.  Every other argument as gaze_overlay takes it; frames and out
    may start at any byte; out=frames_yuv renders in place.  One launch, no host sync.  The rule is stated in
    include/csts_hip.h.  window (top, left, H, W): the frames are surfaces (N, Hs * 3 / 2, Ws) and the pictures their windows
    (inputs.check_window; csts_gaze_overlay_yuv_win): out is a surface as well, its window the overlay of the window and every
    byte around it the input's (not written at all in place; otherwise the surface is copied first, one more device copy)."""
    from .inputs import check_pixel_format, _yuv_geom
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    if layout == 0:
        raise ValueError("gaze_overlay_yuv draws 'nv12' or 'i420' frames; packed RGB goes through gaze_overlay")
    _need_gpu(frames_yuv, rescaled, centers, out)
    if frames_yuv.dtype != torch.uint8 or frames_yuv.dim() != 3:
        raise ValueError(f"{pixel_format} frames must be uint8 (N, H * 3 / 2, W), got {tuple(frames_yuv.shape)} {frames_yuv.dtype}")
    H, W, surf = _yuv_geom(frames_yuv.shape, pixel_format, window)
    N = frames_yuv.shape[0]
    alpha, radius, S = _check_overlay_args("gaze_overlay_yuv", [(frames_yuv, out)], rescaled, centers, alpha, radius, crop_size)
    if out is None:
        out = torch.empty_like(frames_yuv)
    a, b, nbytes = frames_yuv.data_ptr(), out.data_ptr(), frames_yuv.numel()
    if a != b and a < b + nbytes and b < a + nbytes:
        raise ValueError("out must be the frames themselves (in place) or share no memory with them")
    par = _overlay_params(params, S, frames_yuv.device)
    maps = rescaled.detach().contiguous()
    cen = None if centers is None else centers.contiguous()
    if surf:
        L.check(_lib().csts_gaze_overlay_yuv_win(_p(frames_yuv), _p(maps), _p(cen), _p(par), _p(out), N, H, W, *surf, S, maps.shape[1],
                                                 maps.shape[2], alpha, radius, layout, mat, fr, _stream()),
                "csts_gaze_overlay_yuv_win")
        return out
    L.check(_lib().csts_gaze_overlay_yuv(_p(frames_yuv), _p(maps), _p(cen), _p(par), _p(out), N, H, W, S, maps.shape[1],
                                         maps.shape[2], alpha, radius, layout, mat, fr, _stream()), "csts_gaze_overlay_yuv")
    return out


# ----------------------------------------------------------------------------------------- gaze overlay of a group
_OVG_COLS = 13      # job row of include/csts_hip.h: src, dst, K, H, W, new h, new w, y0, x0, flip, first row, first workgroup, vector


def _disjoint_jobs(src, dst, nbytes):
    """No job may write what another reads or writes; a job may write its own frames (dst == src).  int64 arrays, one entry a job."""
    import numpy as np
    order = np.argsort(dst, kind="stable")
    lo, hi = dst[order], (dst + nbytes)[order]
    clash = np.nonzero(hi[:-1] > lo[1:])[0]
    if clash.size:
        a, b = sorted((int(order[clash[0]]), int(order[clash[0] + 1])))
        raise ValueError(f"job {b}: out overlaps the out of job {a}")
    for j in range(len(src)):
        k = int(np.searchsorted(hi, src[j], side="right"))       # the first out that ends after the job's first source byte
        if k < len(lo) and int(order[k]) == j and lo[k] == src[j]:
            k += 1                                               # in place
        if k < len(lo) and lo[k] < src[j] + nbytes[j]:
            other = int(order[k])
            raise ValueError(f"job {other}: out overlaps the frames of job {j}" if other != j else
                             f"job {j}: out must be the frames themselves (in place) or share no memory with them")


def group_gaze_overlay(jobs, rescaled, centers, crop_size, alpha=0.4, radius=5, outs=None, pixel_format="rgb24", matrix="bt601",
                       full_range=False, window=None):
    """gaze_overlay / gaze_overlay_yuv for several jobs of different sizes in ONE launch (csts_group_gaze_overlay / _yuv): jobs is a
    list of (frames, params_row) -- frames uint8 (K, H, W, 3) on the device, or (K, H * 3 / 2, W) in the one 4:2:0 pixel_format
    (with matrix and full_range) of the call, each job of its own K, H, W; params_row its five integers on the HOST -- and
    rescaled fp32 (P, mh, mw), centers int32 (P, 2) or None hold the rows of all jobs in job order, P = the sum of K.  Returns
    the list of outputs, out[j] = gaze_overlay(frames_j, rescaled[rows of j], params_row_j, crop_size, centers[rows of j], alpha,
    radius) byte for byte (gaze_overlay_yuv in a 4:2:0 format).  outs: None, or one entry per job, each None or the tensor to
    draw into; outs[j] may be the frames of job j themselves (in place).  The outputs that are not given are views of ONE
    allocation, each starting at a 16-byte boundary.  No job's out may overlap another job's frames or out.  Validation is
    gaze_overlay's per job, the messages prefixed "job j: ", all on the host before anything is launched; the table goes up in
    one copy.  Inside the launch a job takes the 4-pixel path when W % 4 == 0 and frames and out are 4-byte aligned, else the byte
    path (packed RGB); a 4:2:0 job that cannot take the 4-pixel path goes through gaze_overlay_yuv, one launch for that job.
    The frames are tight pictures: a window is refused."""
    import numpy as np
    from .inputs import check_pixel_format, _yuv_hw, _upload, no_window
    no_window(window, "group_gaze_overlay")
    from .infer import overlay_group_table
    layout, mat, fr = check_pixel_format(pixel_format, matrix, full_range)
    jobs = list(jobs)
    J = len(jobs)
    if J < 1 or J > 65535:
        raise ValueError(f"group_gaze_overlay takes 1..65535 jobs a call, got {J}")
    outs = [None] * J if outs is None else list(outs)
    if len(outs) != J:
        raise ValueError(f"outs must hold one entry per job ({J}), got {len(outs)}")
    _need_gpu(rescaled, centers)
    S = int(crop_size)
    sizes, rows, shapes = [], [], []
    for j, job in enumerate(jobs):
        try:
            frames, row = job
            _need_gpu(frames, outs[j])
            if layout:
                if frames.dtype != torch.uint8 or frames.dim() != 3:
                    raise ValueError(f"{pixel_format} frames must be uint8 (K, H * 3 / 2, W), got {tuple(frames.shape)} {frames.dtype}")
                H, W = _yuv_hw(frames.shape, pixel_format)
            else:
                if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
                    raise ValueError(f"frames must be uint8 (K, H, W, 3), got {tuple(frames.shape)} {frames.dtype}")
                H, W = int(frames.shape[1]), int(frames.shape[2])
            K = int(frames.shape[0])
            if K < 1 or H < 1 or W < 1:
                raise ValueError(f"frames must hold K >= 1 frames of H, W >= 1, got {tuple(frames.shape)}")
            if W > 8192 or H > 65535:
                raise ValueError(f"frames wider than 8192 or taller than 65535 pixels are not supported, got {H} x {W}")
            rows.append(_host_params_row(row, S))
        except L.CstsError as e:
            raise L.CstsError(f"job {j}: {e}") from None
        except (ValueError, TypeError) as e:
            raise ValueError(f"job {j}: {e}") from None
        sizes.append((K, H, W))
        shapes.append(frames.shape)
    alpha, radius, S = _check_overlay_args("group_gaze_overlay", [(job[0], o) for job, o in zip(jobs, outs)], rescaled, centers, alpha,
                                           radius, S, per_job=True)
    dev = jobs[0][0].device
    nbytes = np.asarray([int(np.prod(s)) for s in shapes], dtype=np.int64)
    fresh = [j for j in range(J) if outs[j] is None]
    if fresh:                                                    # one allocation, every view at a 16-byte boundary
        offs = np.concatenate([[0], np.cumsum((nbytes[fresh] + 15) // 16 * 16)])
        buf = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
        for j, o in zip(fresh, offs[:-1]):
            outs[j] = buf[int(o):int(o) + int(nbytes[j])].view(shapes[j])
    src = np.asarray([job[0].data_ptr() for job in jobs], dtype=np.int64)
    dst = np.asarray([o.data_ptr() for o in outs], dtype=np.int64)
    _disjoint_jobs(src, dst, nbytes)
    maps = rescaled.detach().contiguous()
    cen = None if centers is None else centers.contiguous()
    vector = [W % 4 == 0 and int(a) % 4 == 0 and int(b) % 4 == 0 for (_, _, W), a, b in zip(sizes, src, dst)]
    first_row = overlay_group_table(sizes, vector)["first_row"]
    take = list(range(J))
    if layout:                                                   # the tiled byte path of 4:2:0 stays with the single-tensor kernel
        take = [j for j in range(J) if vector[j]]
        for j in range(J):
            if not vector[j]:
                sel = slice(int(first_row[j]), int(first_row[j]) + sizes[j][0])
                gaze_overlay_yuv(jobs[j][0], maps[sel], rows[j], S, pixel_format, matrix=matrix, full_range=full_range,
                                 centers=None if cen is None else cen[sel], alpha=alpha, radius=radius, out=outs[j])
    if take:
        t = overlay_group_table([sizes[j] for j in take], [vector[j] for j in take])
        table = np.zeros((len(take), _OVG_COLS), dtype=np.int64)
        table[:, 0], table[:, 1] = src[take], dst[take]
        table[:, 2:5] = np.asarray([sizes[j] for j in take], dtype=np.int64)
        table[:, 5:10] = np.asarray([rows[j] for j in take], dtype=np.int64)
        table[:, 10], table[:, 11], table[:, 12] = first_row[take], t["first_workgroup"], t["vector"]
        (d_jobs,) = _upload(dev, table)
        args = (_p(d_jobs), table.ctypes.data, len(take), _p(maps), _p(cen), S, maps.shape[1], maps.shape[2], alpha, radius)
        with torch.cuda.device(dev):
            if layout:
                L.check(_lib().csts_group_gaze_overlay_yuv(*args, layout, mat, fr, _stream()), "csts_group_gaze_overlay_yuv")
            else:
                L.check(_lib().csts_group_gaze_overlay(*args, _stream()), "csts_group_gaze_overlay")
    return outs


def group_points_source(points, jobs, crop_size):
    """infer.points_to_source followed by infer.marker_centers for the rows of several jobs in ONE launch
    (csts_group_points_source): points fp32 (P, 2) on the device, the rows of all jobs in job order; jobs a HOST list of (K,
    params_row, H, W) -- K rows under that params row (new h, new w, y0, x0, flip) on a source of H x W; P = the sum of K ->
    {"points_source": fp64 (P, 2), "centers": int32 (P, 2)}: x_src = (x S + x0) / new w in IEEE double arithmetic and
    X = floor(x_src W), likewise y; a NaN point stays NaN and gets the centre (-1, -1).  Bit for bit what the two torch functions
    give per job, on either device."""
    import numpy as np
    from .inputs import _upload
    from .infer import overlay_group_table
    _need_gpu(points)
    jobs = [tuple(job) for job in jobs]
    J, S = len(jobs), int(crop_size)
    if J < 1 or J > 65535 or S < 1:
        raise ValueError(f"group_points_source takes 1..65535 jobs and crop_size >= 1, got {J} and {S}")
    table = np.zeros((J, _OVG_COLS), dtype=np.int64)
    sizes = []
    for j, job in enumerate(jobs):
        try:
            K, row, H, W = job
            nh, nw, y0, x0, flip = _parse_params_row(row)
            if not (1 <= nh <= 1 << 24 and 1 <= nw <= 1 << 24 and 0 <= y0 <= 1 << 24 and 0 <= x0 <= 1 << 24):
                raise ValueError(f"params {(nh, nw, y0, x0)} are out of range (1 <= new h, new w <= 2^24, 0 <= y0, x0 <= 2^24)")
            sizes.append((int(K), int(H), int(W)))
            table[j, 2:10] = (int(K), int(H), int(W), nh, nw, y0, x0, flip)
        except (ValueError, TypeError) as e:
            raise ValueError(f"job {j}: {e}") from None
    t = overlay_group_table(sizes, [False] * J)
    table[:, 10], table[:, 11] = t["first_row"], t["first_workgroup"]
    P = t["rows"]
    if points.dtype != torch.float32 or tuple(points.shape) != (P, 2):
        raise ValueError(f"points must be fp32 ({P}, 2), one row per frame of the jobs, got {tuple(points.shape)} {points.dtype}")
    x = points.detach().contiguous()
    out = {"points_source": torch.empty(P, 2, dtype=torch.float64, device=x.device),
           "centers": torch.empty(P, 2, dtype=torch.int32, device=x.device)}
    (d_jobs,) = _upload(x.device, table)
    with torch.cuda.device(x.device):
        L.check(_lib().csts_group_points_source(_p(d_jobs), table.ctypes.data, J, _p(x), S, _p(out["points_source"]),
                                                _p(out["centers"]), _stream()), "csts_group_points_source")
    return out


# ----------------------------------------------------------------------------------------- fusion attention maps
def audio_pixel_attn(qkv, lse, thw, heads, n_frames, crop_size):
    """csts_audio_pixel_attn on what the spatial fusion block's forward holds: qkv (B, N, 3C) packed q | k | v rows (fp32 or the
    library's 16-bit type), N = T' h w + T' for the grid thw = (T', h, w), and lse fp32 (B, heads, N), the rows' log-sum-exp in
    the log2 domain (attention_inner) -> the audio-visual correlation map of visualization.py:172-228 without the (N, N) matrix:
    {"column": (B, heads, T', h, w) = the probability each image region of frame t gives that frame's audio token,
     "column_mean": (B, T', h, w) = its head mean,
     "maps": (B, heads + 1, T, h, w) = per input frame (T = n_frames) the time-linear mix of the column, rescaled by the extrema its
             bilinear upsample takes on the S x S crop lattice (S = crop_size) -- what gaze_overlay draws; index `heads` = the mean,
     "range": (B, heads + 1, T, 2) = those extrema (lo, hi)}, all fp32.
    Inference only: raises when an input carries a gradient.  Two launches, no host sync: it can be captured in a graph.  The
    rule is stated in include/csts_hip.h."""
    _need_gpu(qkv, lse)
    if (qkv.requires_grad or lse.requires_grad) and torch.is_grad_enabled():
        raise L.CstsError("audio_pixel_attn is an inference output: it has no backward (call it under torch.no_grad(), or use "
                          "audio_attn for the differentiable MVIT.SPATIAL_AUDIO_ATTN map)")
    thw = [int(v) for v in thw]
    heads, T, S = int(heads), int(n_frames), int(crop_size)
    if len(thw) != 3 or min(thw) < 1 or heads < 1:
        raise ValueError(f"thw must be three positive sizes (T', h, w) and heads positive, got {thw} and {heads}")
    if T < 1 or S < 1:
        raise ValueError(f"audio_pixel_attn needs n_frames >= 1 and crop_size >= 1, got {T} and {S}")
    Tp, h, w = thw
    N = Tp * h * w + Tp
    if qkv.dim() != 3 or qkv.shape[1] != N or qkv.shape[2] % (3 * heads) != 0:
        raise ValueError(f"qkv must be (B, {N}, 3 * heads * head_dim) for the grid {tuple(thw)} and {heads} heads, got {tuple(qkv.shape)}")
    B = qkv.shape[0]
    hd = qkv.shape[2] // (3 * heads)
    if lse.dtype != torch.float32 or tuple(lse.shape) != (B, heads, N):
        raise ValueError(f"lse must be fp32 ({B}, {heads}, {N}), got {tuple(lse.shape)} {lse.dtype}")
    if B < 1:
        raise ValueError("audio_pixel_attn needs B >= 1 clips")
    x, l = qkv.detach().contiguous(), lse.detach().contiguous()
    dev = x.device
    out = {"column": torch.empty(B, heads, Tp, h, w, dtype=torch.float32, device=dev),
           "column_mean": torch.empty(B, Tp, h, w, dtype=torch.float32, device=dev),
           "maps": torch.empty(B, heads + 1, T, h, w, dtype=torch.float32, device=dev),
           "range": torch.empty(B, heads + 1, T, 2, dtype=torch.float32, device=dev)}
    L.check(_lib().csts_audio_pixel_attn(_p(x), _dt(x), _p(l), B, heads, hd, Tp, h, w, T, S, hd ** -0.5, _p(out["column"]),
                                         _p(out["column_mean"]), _p(out["maps"]), _p(out["range"]), _stream()),
            "csts_audio_pixel_attn")
    return out


def _attention_grid(h, w, what):
    if h < 1 or w < 1 or h > L.AUDIO_PIXEL_MAX_SIDE or w > L.AUDIO_PIXEL_MAX_SIDE or h * w > L.AUDIO_PIXEL_MAX_HW:
        raise ValueError(f"{what} needs 1 <= h, w <= CSTS_AUDIO_PIXEL_MAX_SIDE ({L.AUDIO_PIXEL_MAX_SIDE}) and h * w <= "
                         f"CSTS_AUDIO_PIXEL_MAX_HW ({L.AUDIO_PIXEL_MAX_HW}), got {h} x {w}")


def attention_track(column, frames_idx, n_frames, n_input_frames, crop_size):
    """csts_attention_track: the audio_attention of every window of a recording -- column fp32 (Wn, heads, T', h, w), windows
    concatenated -- and frames_idx, an integer (Wn, T) device tensor = the video frame each window's input frame j shows (T =
    n_input_frames, plan_video's "frames_idx") -> one attention map per video frame, head and head mean:
    {"mixed": (F, heads + 1, h, w) = the mean over the (window, input frame) pairs that land on the frame (added in ascending
              w T + j) of the map audio_pixel_attn mixes in time for that pair; index `heads` = the head mean,
     "maps": same shape = mixed rescaled by the extrema its bilinear upsample takes on the S x S crop lattice (S = crop_size) --
             what gaze_overlay draws,
     "range": (F, heads + 1, 2) = those extrema (lo, hi),
     "count": (F,) int32 = pairs that landed on the frame}, F = n_frames.  A frame no pair lands on: mixed and maps 0, range NaN.
    Frames outside [0, F) are dropped.  A frame with one pair carries audio_pixel_attn's maps / range of that pair bit for bit.
    The pair lists are built on the device as gaze_track builds its rows (stable sort, binary search): two launches of the
    library, no host sync, graph-capturable.  The rule is stated in include/csts_hip.h."""
    _need_gpu(column, frames_idx)
    if column.requires_grad and torch.is_grad_enabled():
        raise L.CstsError("attention_track is an inference output: it has no backward (call it under torch.no_grad())")
    if column.dim() != 5 or column.dtype != torch.float32:
        raise ValueError(f"column must be fp32 (Wn, heads, T', h, w), got {tuple(column.shape)} {column.dtype}")
    Wn, heads, Tp, h, w = column.shape
    F_, T, S = int(n_frames), int(n_input_frames), int(crop_size)
    if frames_idx.dtype not in (torch.int32, torch.int64) or tuple(frames_idx.shape) != (Wn, T):
        raise ValueError(f"frames_idx must be int32 or int64 ({Wn}, {T}), got {tuple(frames_idx.shape)} {frames_idx.dtype}")
    if F_ < 1 or T < 1 or S < 1 or Wn < 1 or heads < 1 or Tp < 1:
        raise ValueError(f"attention_track needs n_frames, n_input_frames, crop_size, Wn, heads and T' >= 1, got {F_}, {T}, {S}, "
                         f"{Wn}, {heads} and {Tp}")
    _attention_grid(h, w, "attention_track")
    x = column.detach().contiguous()
    dev = x.device
    order, offsets = _target_lists(frames_idx.reshape(-1).to(torch.int64), F_)
    out = {"mixed": torch.empty(F_, heads + 1, h, w, dtype=torch.float32, device=dev),
           "maps": torch.empty(F_, heads + 1, h, w, dtype=torch.float32, device=dev),
           "range": torch.empty(F_, heads + 1, 2, dtype=torch.float32, device=dev),
           "count": torch.empty(F_, dtype=torch.int32, device=dev)}
    L.check(_lib().csts_attention_track(_p(x), _p(order), _p(offsets), F_, Wn, heads, Tp, h, w, T, S, _p(out["mixed"]),
                                        _p(out["maps"]), _p(out["range"]), _p(out["count"]), _stream()), "csts_attention_track")
    return out


def attention_rescale(mixed, crop_size, valid=None):
    """csts_attention_rescale: coarse maps mixed fp32 (F, G, h, w) -> {"maps": (F, G, h, w) = (mixed - lo) / (hi - lo + 1e-6),
    "range": (F, G, 2) = (lo, hi)}, the extrema of each map's bilinear upsample over the S x S crop lattice (S = crop_size) --
    the second half of attention_track, for maps that changed after it (a filled track).  valid (optional, int32 or bool (F,)
    on the device): a frame with valid <= 0 gets maps 0 and range NaN.  One launch, no host sync: graph-capturable."""
    _need_gpu(mixed, valid)
    if mixed.dim() != 4 or mixed.dtype != torch.float32:
        raise ValueError(f"mixed must be fp32 (F, G, h, w), got {tuple(mixed.shape)} {mixed.dtype}")
    F_, G, h, w = mixed.shape
    S = int(crop_size)
    if F_ < 1 or G < 1 or S < 1:
        raise ValueError(f"attention_rescale needs F >= 1 frames, G >= 1 maps a frame and crop_size >= 1, got {F_}, {G} and {S}")
    _attention_grid(h, w, "attention_rescale")
    v = None
    if valid is not None:
        if valid.dtype not in (torch.int32, torch.bool) or tuple(valid.shape) != (F_,):
            raise ValueError(f"valid must be int32 or bool ({F_},), got {tuple(valid.shape)} {valid.dtype}")
        v = valid.to(torch.int32).contiguous()
    x = mixed.detach().contiguous()
    out = {"maps": torch.empty_like(x), "range": torch.empty(F_, G, 2, dtype=torch.float32, device=x.device)}
    L.check(_lib().csts_attention_rescale(_p(x), _p(v), G, F_, h, w, S, _p(out["maps"]), _p(out["range"]), _stream()),
            "csts_attention_rescale")
    return out


# ----------------------------------------------------------------------------------------- live attention ring
_LIVE_ATTENTION_OUTPUTS = ("mixed", "maps", "range", "frame", "count")


def live_attention_ring(slots, heads, h, w, device):
    """An empty attention ring of `slots` frames of heads + 1 maps of h x w on `device`: {"sum" fp32 (slots, heads + 1, h, w)
    zeros, "count" int32 (slots,) zeros, "frame" int64 (slots,) -1, "newest": -1}.  Frame t lives in slot t mod slots
    (include/csts_hip.h, live attention ring).  "newest" is a host int, the highest frame added so far: live_attention_add keeps
    it, so that it can refuse a pair that would land on a slot holding a newer frame without reading the device."""
    slots, heads, h, w = int(slots), int(heads), int(h), int(w)
    if slots < 1 or slots > 65535 or heads < 1 or heads > 65534:
        raise ValueError(f"an attention ring holds 1..65535 slots of 2..65535 maps, got {slots} slots and {heads} heads")
    _attention_grid(h, w, "live_attention_ring")
    device = torch.device(device)
    if device.type != "cuda":
        raise L.CstsError("the attention ring lives on MI355X only (there is no CPU fallback)")
    return {"sum": torch.zeros(slots, heads + 1, h, w, dtype=torch.float32, device=device),
            "count": torch.zeros(slots, dtype=torch.int32, device=device),
            "frame": torch.full((slots,), -1, dtype=torch.int64, device=device), "newest": -1}


def _check_attention_ring(ring):
    """The tensors of an attention ring, checked: (sum, count, frame, Ra, heads, h, w)."""
    try:
        s, c, f, newest = ring["sum"], ring["count"], ring["frame"], ring["newest"]
    except (KeyError, TypeError, IndexError):
        raise ValueError("ring must be a dict with \"sum\", \"count\", \"frame\" and \"newest\" (ops.live_attention_ring)")
    _need_gpu(s, c, f)
    if s.dim() != 4 or s.dtype != torch.float32 or not s.is_contiguous() or s.shape[1] < 2:
        raise ValueError(f"ring[\"sum\"] must be contiguous fp32 (Ra, heads + 1, h, w), got {tuple(s.shape)} {s.dtype}")
    Ra, G, h, w = s.shape
    if c.dtype != torch.int32 or tuple(c.shape) != (Ra,) or not c.is_contiguous():
        raise ValueError(f"ring[\"count\"] must be contiguous int32 ({Ra},), got {tuple(c.shape)} {c.dtype}")
    if f.dtype != torch.int64 or tuple(f.shape) != (Ra,) or not f.is_contiguous():
        raise ValueError(f"ring[\"frame\"] must be contiguous int64 ({Ra},), got {tuple(f.shape)} {f.dtype}")
    if isinstance(newest, bool) or not isinstance(newest, int):
        raise ValueError(f"ring[\"newest\"] must be a host int (the highest frame added so far, -1: none), got {newest!r}")
    if Ra < 1 or Ra > 65535 or G > 65535:
        raise ValueError(f"an attention ring holds 1..65535 slots of 2..65535 maps, got {Ra} slots of {G} maps")
    _attention_grid(h, w, "the attention ring")
    return s, c, f, Ra, G - 1, h, w


def live_attention_add(column, frames_idx, frames_host, ring, live_from=0):
    """csts_live_attention_add: the audio_attention of the windows a step ran -- column fp32 (Wn, heads, T', h, w) -- and
    frames_idx int64 (Wn, T) on the device, the video frame each window's input frame j shows, folded into the attention ring
    (ops.live_attention_ring) in place.  Pair p = w T + j adds, for every head and the head mean, the map attention_track mixes
    for it to the slot of frames_idx[w, j]: a slot whose frame tag differs restarts (sum = 0 + map, count 1, retagged), a slot
    whose tag matches is added to and its count bumped, in ascending p -- the order and the arithmetic of ops.attention_track
    when the windows come in the order they ran.  frames_host: the same (Wn, T) frames on the HOST (a numpy array or nested
    sequence of ints; the stream has them from stream_window), so that what cannot be written is refused before the launch and
    without a host sync:
      a negative frame;
      a frame t >= live_from + Ra, which would restart the slot of frame t - Ra >= live_from.  live_from: the lowest frame a row
      still to come may read (its frame minus max_age);
      a pair whose frame lies Ra or more below the highest frame added before it (ring["newest"], or an earlier pair of this
      call): it could land on a slot that holds a NEWER frame and would wipe that frame out.
    A refusal writes nothing.  One launch, no atomics, no host sync: the launch can be captured in a graph, but ring["newest"]
    is host state set when this function runs: a replay of the graph does not move it, so the third refusal only tracks eager
    calls, and a caller who replays keeps the two conditions themselves (stream.attention_ring_slots)."""
    import numpy as np
    _need_gpu(column, frames_idx)
    s, c, f, Ra, heads, h, w = _check_attention_ring(ring)
    if column.dim() != 5 or column.dtype != torch.float32 or tuple(column.shape[1:2] + column.shape[3:]) != (heads, h, w):
        raise ValueError(f"column must be fp32 (Wn, {heads}, T', {h}, {w}), got {tuple(column.shape)} {column.dtype}")
    Wn, _, Tp = column.shape[:3]
    if frames_idx.dtype != torch.int64 or frames_idx.dim() != 2 or frames_idx.shape[0] != Wn:
        raise ValueError(f"frames_idx must be int64 ({Wn}, T), got {tuple(frames_idx.shape)} {frames_idx.dtype}")
    T = frames_idx.shape[1]
    if Wn < 1 or T < 1 or Tp < 1 or Wn * T > 65535:
        raise ValueError(f"live_attention_add takes 1..65535 (window, input frame) pairs a call, got {Wn} windows of {T}")
    if not torch.is_tensor(frames_host):                         # a tensor is refused by _live_host_table, with its message
        frames_host = np.asarray(frames_host)
        if frames_host.shape != (Wn, T):
            raise ValueError(f"frames_host must hold the ({Wn}, {T}) entries of frames_idx as integers on the host, got shape "
                             f"{frames_host.shape}")
        frames_host = frames_host.reshape(-1)
    host = _live_host_table(frames_host, Wn * T, "frames_host", "frames_idx").reshape(Wn, T)
    live_from = int(live_from)
    if int(host.min()) < 0:
        raise ValueError(f"frames must be frame numbers >= 0, got {int(host.min())}")
    if int(host.max()) >= live_from + Ra:
        t = int(host.max())
        raise ValueError(f"the attention ring holds {Ra} frames: frame {t} would overwrite the slot of frame {t - Ra}, which is still "
                         f"inside the live span (it starts at frame {live_from}); nothing was written")
    flat = host.reshape(-1)
    before = np.maximum.accumulate(np.concatenate([[int(ring["newest"])], flat]))      # [p]: the highest frame added before pair p
    behind = np.nonzero(before[:-1] - flat >= Ra)[0]
    if behind.size:
        p = int(behind[0])
        raise ValueError(f"the attention ring holds {Ra} frames: frame {int(flat[p])} (window row {p // T}) lies {int(before[p] - flat[p])} "
                         f"below frame {int(before[p])}, which was added before it, and could land on the slot of a newer frame; "
                         "nothing was written")
    x = column.detach().contiguous()
    L.check(_lib().csts_live_attention_add(_p(x), _p(frames_idx.contiguous()), Wn, heads, Tp, h, w, T, _p(s), _p(c), _p(f), Ra,
                                           _stream()), "csts_live_attention_add")
    ring["newest"] = int(before[-1])


def live_attention_rows(ring, f0, K, crop_size, max_age, want=_LIVE_ATTENTION_OUTPUTS):
    """csts_live_attention_rows: the attention rows of frames f0 .. f0 + K - 1 out of the attention ring, by the rule HOLD THE
    NEWEST MAP.  With A = ops.attention_track of everything added so far (n_frames = n + 1) and g = the largest frame in
    [max(0, n - max_age), n] with A["count"][g] > 0, row n is {"frame": g (int64, -1 when there is none), "count":
    A["count"][g] (int32, 0), "mixed": A["mixed"][g], "maps": A["maps"][g], "range": A["range"][g]} -- (K,), (K,),
    (K, heads + 1, h, w) twice and (K, heads + 1, 2) -- bit for bit, as long as no frame of [n - max_age, n] has been recycled
    (live_attention_add's live_from).  A row without a g has zero maps and a NaN range.  crop_size: the S of the lattice the
    extrema are taken on.  Returns the outputs named in `want`; the others are not computed (maps and range are computed
    together).  The ring is only read.  One launch, no host sync: it can be captured in a graph."""
    s, c, f, Ra, heads, h, w = _check_attention_ring(ring)
    f0, K, S, max_age = int(f0), int(K), int(crop_size), int(max_age)
    if f0 < 0 or K < 1 or K > 65535 or f0 + K >= 2 ** 62:
        raise ValueError(f"live_attention_rows answers 1..65535 frames from f0 >= 0, got f0 {f0}, K {K}")
    if max_age < 0 or max_age > 65535 or S < 1 or S > 65536:
        raise ValueError(f"max_age must lie in 0..65535 and crop_size in 1..65536, got {max_age} and {S}")
    f32 = torch.float32
    table = (("mixed", (K, heads + 1, h, w), f32), ("maps", (K, heads + 1, h, w), f32), ("range", (K, heads + 1, 2), f32),
             ("frame", (K,), torch.int64), ("count", (K,), torch.int32))
    out = _wanted(want, _LIVE_ATTENTION_OUTPUTS, table, s.device)
    pair = dict(out)                                             # the kernel writes maps and range together
    if ("maps" in out) != ("range" in out):
        pair.update(_wanted(("maps", "range"), _LIVE_ATTENTION_OUTPUTS, table, s.device))
        pair.update(out)
    L.check(_lib().csts_live_attention_rows(_p(s), _p(c), _p(f), Ra, f0, K, heads, h, w, S, max_age, _p(pair.get("mixed")),
                                            _p(pair.get("maps")), _p(pair.get("range")), _p(pair.get("frame")), _p(pair.get("count")),
                                            _stream()), "csts_live_attention_rows")
    return out
