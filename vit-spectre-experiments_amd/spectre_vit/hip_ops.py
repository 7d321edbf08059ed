"""torch.autograd Functions over the C-ABI of libspv_hip.so.

Host-side mirror of the arithmetic the reference modules issue as stock ATen ops; every Function
borrows ``data_ptr()``s, launches on torch's current HIP stream and never synchronises.  Tensors must be
on a HIP device: a CPU tensor raises (there is deliberately no CPU / eager-PyTorch fallback).

  _launch.py     dtype codes, raw pointers, the current stream's handle, the device check
  shadows.py     the compute-dtype copies of the weights (_ShadowCache, ShadowSet, PinnedShadows)
  timing.py      KernelTimer and the work model of every entry point (bench.py's roofline pass)
  branch_ops.py  the SpectreBranch ops
  hip_ops.py     the GEMM and weight-gradient dispatch, the held launches of the backward pass, GradSink, the Functions, the flags
"""
from __future__ import annotations

import collections
import ctypes
import math
import os
import warnings
import weakref
from typing import NamedTuple

import torch

from . import _native, prologue, shadows
from ._launch import _DT, BF16, F32, _dt, _p, _require_gpu, _stream  # noqa: F401  (tools/ and tests read them here)
from .shadows import invalidate_weight_shadows  # noqa: F401  (the documented name: INTEGRATION.md)
from .timing import KernelTimer, _timing, set_kernel_timer  # noqa: F401  (bench.py reads the timer here)


_warned_fp16 = False


def compute_dtype(x: torch.Tensor) -> torch.dtype:
    """dtype the kernels run in for input x: the autocast dtype when autocast is on (bf16; an fp16 autocast
    region -- spectre_vit/repl/train.py:219 -- is served in bf16, same speed and no loss scaling issues),
    otherwise x's own dtype (fp32 parity runs, or bf16 activations)."""
    global _warned_fp16
    if torch.is_autocast_enabled("cuda"):
        dt = torch.get_autocast_dtype("cuda")
        if dt == torch.float16:
            if not _warned_fp16:
                warnings.warn("spectre_vit (MI355X): fp16 autocast is served by the bf16 kernels")
                _warned_fp16 = True
            return torch.bfloat16
        if dt == torch.bfloat16:
            return torch.bfloat16
    if x.dtype in (torch.float32, torch.bfloat16):
        return x.dtype
    return torch.float32


def cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """differentiable dtype cast through spv_cast (no-op when already `dtype`)."""
    if x.dtype == dtype:
        return x
    return _Cast.apply(x, dtype)


def _raw_cast(x, dtype):
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _native.call("spv_cast", _p(x), _dt(x), _p(out), _DT[dtype], x.numel(), _stream())
    return out


class _Cast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        _require_gpu(x)
        ctx.src = x.dtype
        return _raw_cast(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return _raw_cast(g, ctx.src), None


def _gemm(a, b, bias, c, M, N, K, lda, ldb, ldc, accumulate=0, splits=1, workspace=None):
    if splits == 1 and K >= 256:
        # a handful of output tiles (the 512 x 100 classifier head: 4) would run on a handful of CUs for the whole K
        # loop -- 42 us for 52 MFLOP in fp32; split the reduction so that ~256 workgroups share it
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        # (bf16 problems of few rows take the library's 32 x 32-tile kernel instead: no workspace, no reduce launch)
        rows_kernel = (a.dtype == torch.bfloat16 and M <= 2048 and K <= 1536 and K % 16 == 0 and lda % 8 == 0 and ldb % 8 == 0
                       and 64 <= ((M + 31) // 32) * ((N + 31) // 32) <= 1024)
        if tiles <= 32 and not rows_kernel:
            splits = max(1, min(K // 64, 256 // tiles))
            if splits > 1:
                workspace = torch.empty((splits * M * N,), dtype=torch.float32, device=c.device)
    _gemm_launch(a, b, bias, c, M, N, K, lda, ldb, ldc, accumulate, splits, workspace)


def _gemm_launch(a, b, bias, c, M, N, K, lda, ldb, ldc, accumulate=0, splits=1, workspace=None):
    """the raw C-ABI call (development tools time it directly)"""
    _native.call("spv_gemm_nt", _p(a), _p(b), _p(bias), _p(c), M, N, K, lda, ldb, ldc, _dt(a), _dt(c), accumulate, splits,
                 _p(workspace), _stream())


# (the flags of this module are plain attributes -- tests, spectre_vit.graph and bench.py set some; none is read from the environment)
_SIDE_MIN_FLOPS = 1e11  # weight gradients at least this big fork to the side stream
_side_streams = {}
_side_keep = []  # tensors a side-stream kernel still reads/writes: kept alive until the join


def _side_stream(dev):
    s = _side_streams.get(dev)
    if s is None:
        s = _side_streams[dev] = torch.cuda.Stream(device=dev)
    return s


def join_side_stream():
    """Make the current stream wait for everything launched on the side stream (no-op when nothing is pending)."""
    if _side_keep:
        dev = _side_keep[0][0].device
        torch.cuda.current_stream().wait_stream(_side_streams[dev])
        _side_keep.clear()


# ------------------------------------------------------------------------------------------------
# folds travel with launches that happen anyway: a row kernel's fold of its partial column sums (dgamma / dbeta / dbias) either rides
# in its own layer's weight-gradient reduce (_sl_backward) or -- the FNet kernel has no GEMM beside it -- is held back for the next
# weight-gradient reduce of the same backward pass; whatever is still held when the autograd engine finishes runs as one launch.
# Held folds need gradient memory that outlives the node (a GradReducer sink): autograd would otherwise copy the unfinished tensor.
# With data parallelism the bucket hooks need every gradient as soon as its node has run: nothing is held.
# ------------------------------------------------------------------------------------------------
PATH_COUNTS = collections.Counter()   # host-side dispatch census (tests assert that the shapes they ran took the batched / side paths)
_held_folds = []   # _Fold jobs
_held_task = -2    # the autograd graph task (backward pass) the held folds belong to
FOLD_RIDERS = 6    # fold jobs a layer's own reduce launch carries
# Layer weight gradients travel together as well: alone each is 24 tiles of 128 x 128, i.e. ~21 K-slices to fill the chip (25 K-tiles
# per workgroup, 33 MB of partial sums written and re-read); eight of them in one launch fill it with 5 slices.  Same conditions as a
# held fold (sink-backed outputs, one process), and only gradients nothing reads before the backward pass ends.
_held_wgrads = []  # _HeldWgrad records
WGRAD_BATCH = 8    # problems per launch (csrc/spv_gemm.hip TNB_MAX)
BATCH_FOLDS = 16   # fold jobs the batch's reduce launch carries (FJ_MAX)
_WGRAD_HOLD = True   # layer weight gradients are held for the batch launch
# The class head's parameter gradients (dW, dgamma, dbeta, dbias: spv_small_sl_bwd_w) are read by nothing inside the backward pass
# either, and alone their launch leaves nine tenths of the chip idle between the loss and the last layer's backward: held under the
# same conditions, they are issued on the main stream at the end of the patch embedding's backward, where the batched layer weight
# gradients run on the side stream (start_held_wgrads .. join_side_stream) -- or by the end-of-pass callback.
HEAD_WGRAD_HOLD = True
_held_head = []    # _HeldHead records
FOLD_RIDE = True     # tail folds ride in their layer's weight-gradient reduce


# Under data parallelism the overlapped (eager) exchange needs every gradient as soon as its node has run, so nothing is held.  A
# step that exchanges its gradients in ONE call after the backward pass (spectre_vit.graph.GraphedDPStep) has no such need and
# sets this flag while its backward passes run.
HOLD_UNDER_DP = False
TIME_HELD = False   # bench.py's roofline pass: bracket the launch sequence the headline times (held + batched weight gradients)


# Two private torch entry points carry the held launches: the id of the running backward pass and the autograd engine's end-of-pass
# callback.  Where a torch build lacks either, nothing is held (every launch runs at its own node: slower, same results).
_task_id_fn = getattr(torch._C, "_current_graph_task_id", None)
_engine = getattr(getattr(torch.autograd, "Variable", None), "_execution_engine", None)
_HOLD_API = _task_id_fn is not None and hasattr(_engine, "queue_callback")


def _graph_task_id():
    return _task_id_fn() if _task_id_fn is not None else -1


def _hold_ok():
    if not _HOLD_API:
        return False
    if _timing() and not TIME_HELD:
        return False
    if HOLD_UNDER_DP:
        return True
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)


_T = torch.Tensor
# The fold of a row kernel's partial column sums (`parts` slabs of rows of length n) into its parameter gradients, to ride in / be
# deferred with a weight gradient's reduction.  outs are raw addresses, never tensors: a second reference to a gradient tensor makes
# AccumulateGrad clone the -- still unfolded -- gradient (see _hold_fold); whoever makes the job holds the tensors until it is issued or held.
_Fold = NamedTuple("_Fold", [("partials", _T), ("outs", tuple), ("parts", int), ("n", int)])
# A layer weight gradient dw[n, k] = dh[rows, n]^T . x[rows, k] held for the batch launch at the end of the backward pass: dw is the
# address of its sink slot, fold the _Fold that rides in its reduce (or None)
_HeldWgrad = NamedTuple("_HeldWgrad", [("dh", _T), ("x", _T), ("dw", int), ("rows", int), ("n", int), ("k", int), ("fold", object)])


# dh, xs, partials: what the launch reads (held until it is issued); outs: the addresses of the four sink slots (dW, dgamma, dbeta, dbias)
_HeldHead = NamedTuple("_HeldHead", [("dh", _T), ("xs", _T), ("partials", _T), ("outs", tuple), ("rows", int), ("n", int), ("k", int)])


def _addrs(tensors):
    return tuple(t.data_ptr() for t in tensors)


def _fold_array(folds):
    arr = (_native.FoldJob * len(folds))()
    for j, f in zip(arr, folds):
        j.partials = _p(f.partials)
        for i, o in enumerate(f.outs):
            j.out[i] = o
        j.parts, j.nsum, j.n = f.parts, len(f.outs), f.n
    return arr


def _batch_splits(tiles):
    """K-slices of a batch of `tiles` 128 x 128 tiles: the count whose workgroups fill whole rounds of the chip's ~512 slots (two
    4-wave workgroups per CU) best; measured on 192 tiles: 5 slices (960 workgroups) 307 us, 2: 321, 4: 355, 3: 396"""
    if 160 <= tiles <= 224:
        # the six 33 280-row layer gradients of the Small model (192 tiles): re-measured in round 3 on both tile shapes of the batched
        # kernel (tools/tnb_bench.py: 3: 296 / 278 us, 4: 305 / 341, 5: 259 / 281, 6: 247 / 249, 7: 231 / 229, 8: 256 / 267, 10: 242 / 240)
        # and inside the replayed step (5 -> 7 slices: 1.734 / 1.719 -> 1.702 / 1.712 ms)
        return 7
    best, best_score = 1, -1.0
    for sp in range(1, 11):
        rounds = tiles * sp / 512.0
        score = rounds / max(1.0, float(-(-tiles * sp // 512))) - 0.01 * sp
        if rounds >= 0.7 and score > best_score:
            best, best_score = sp, score
    return best


def _flush_held_wgrads():
    """the weight gradients held back during this backward pass: one launch (+ one reduce that carries their folds and the folds held
    so far) per group of up to eight.  Returns every tensor the launches read or write (operands, fold partials, split-K
    workspaces): a caller that runs this on a side stream keeps them alive until the streams are joined."""
    used = []
    while _held_wgrads:
        # up to eight per launch, the long reductions first; gradients over fewer rows (the CLS-only last layer's: 512) ride in the same
        # launch as short problems -- one workgroup per tile, no split-K, no launch + reduce of their own behind the big one
        rows = max(w.rows for w in _held_wgrads)
        group = sorted(_held_wgrads, key=lambda w: -w.rows)[:WGRAD_BATCH]
        taken = {id(w) for w in group}
        _held_wgrads[:] = [w for w in _held_wgrads if id(w) not in taken]   # (by identity: the records hold tensors)
        probs = (_native.TnProblem * len(group))()
        tiles = floats = 0
        flops = 0.0
        folds = []
        for q, w in zip(probs, group):
            n, k = w.n, w.k
            q.a, q.b, q.c, q.m, q.n, q.lda, q.ldb, q.ldc, q.k = _p(w.dh), _p(w.x), w.dw, n, k, n, k, k, w.rows
            if w.rows == rows:
                tiles += ((n + 127) // 128) * ((k + 127) // 128)
                floats += n * k
            flops += 2.0 * w.rows * n * k
            used += [w.dh, w.x]
            if w.fold is not None:
                folds.append(w.fold)
        while _held_folds and len(folds) < BATCH_FOLDS:
            folds.append(_held_folds.pop(0))
        splits = max(1, min(_batch_splits(tiles), rows // 256))   # (the CLS-only last layer: 512 rows)
        ws = torch.empty((splits * floats,), dtype=torch.float32, device=group[0].dh.device)
        used.append(ws)
        used += [f.partials for f in folds]   # the folds' partial column sums: read by the reduce launch, long after this function returns
        arr = _fold_array(folds) if folds else None
        batch = (ctypes.addressof(probs), len(group), rows, splits, _p(ws), ctypes.addressof(arr) if folds else 0, len(folds))
        if _timing():   # a measuring pass brackets the GEMM launch and the reduce launch separately (same kernels, same order)
            for part, work in ((1, flops), (2, 4.0 * floats * (splits + 1))):
                _native.hint = int(work)
                _native.call("spv_gemm_tn_batch_part", *batch, part, _stream())
        else:
            _native.call("spv_gemm_tn_batch", *batch, _stream())
        PATH_COUNTS["wgrad_batch"] += 1
        PATH_COUNTS["wgrad_batch_problems"] += len(group)
    return used


def start_held_wgrads():
    """Called by the LAST node of the backward pass that does real work (the patch embedding): every layer's weight gradient is held
    by now, so their batch starts here on the side stream and runs beside the embedding's backward -- a chain of small, latency-bound
    launches that leaves most of the chip idle.  The end-of-pass callback joins the streams.  True when something was started."""
    if not (_held_wgrads and _held_task == _graph_task_id()) or _timing():
        return False   # (a timed pass keeps the batch on the main stream: its event brackets must not overlap other kernels)
    side = _side_stream(_held_wgrads[0].dh.device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        used = _flush_held_wgrads()
    # everything the side-stream launches touch stays referenced until join_side_stream(): the operands AND the fold partials (they
    # were allocated on the main stream and had no other owner once the flush returned -- the caching allocator could hand their
    # blocks to the embedding's backward, which runs on the main stream beside the batch, before the reduce has read them)
    if used:
        _side_keep.append(tuple(used))
    PATH_COUNTS["wgrad_side_start"] += 1
    return True


def _begin_pass(task):
    """the first hold of backward pass `task`: leftovers cleared, the end-of-pass callback queued, the task recorded"""
    global _held_task
    if _held_task != task:
        _held_folds.clear()   # leftovers of a backward pass that never finished (an exception): their launch must not ride along
        _held_wgrads.clear()
        _held_head.clear()
        _engine.queue_callback(flush_held_folds)
        _held_task = task


def _hold_wgrad(dh, x, dw, sink, rows, n, k, fold, fold_sunk):
    """hold a layer weight gradient for the batch launch at the end of this backward pass (see _held_wgrads).  False: not held."""
    if not (_WGRAD_HOLD and _hold_ok() and _in_sink(dw, sink) and (fold is None or fold_sunk)):
        return False
    task = _graph_task_id()
    if task < 0:
        return False
    _begin_pass(task)
    _held_wgrads.append(_HeldWgrad(dh, x, dw.data_ptr(), rows, n, k, fold))
    return True


def _hold_head_wgrad(dh, xs, partials, outs, sinks, rows, n, k):
    """hold the class head's weights launch for the end of the embedding's backward (see HEAD_WGRAD_HOLD).  False: not held."""
    if not (HEAD_WGRAD_HOLD and _hold_ok() and _sunk(outs, sinks)):
        return False
    task = _graph_task_id()
    if task < 0:
        return False
    _begin_pass(task)
    _held_head.append(_HeldHead(dh, xs, partials, _addrs(outs), rows, n, k))
    return True


def flush_held_head(end_of_pass=False):
    """issue the held class-head weights launches of this backward pass on the current stream.  The record kept the tensors they read
    alive until here; they were allocated on this stream and are read on it, so the allocator's stream order covers them from here on
    (no entry in _side_keep: that list is for what a SIDE-stream kernel touches).  (Records of another pass -- one that never
    finished -- are dropped; the end-of-pass callback only ever sees its own pass's.)"""
    if not _held_head:
        return
    if end_of_pass or _held_task == _graph_task_id():
        for h in _held_head:
            _native.call("spv_small_sl_bwd_w", _p(h.dh), _p(h.xs), _p(h.partials), *h.outs, h.rows, h.n, h.k, _stream())
            PATH_COUNTS["head_wgrad_held"] += 1
    _held_head.clear()


def _in_sink(dw, sink):
    """dw is the parameter's sink slot or a row range of it (memory that outlives the node: it may be written at the end of the pass)"""
    if sink is None:
        return False
    base = sink.view.data_ptr()
    return base <= dw.data_ptr() and dw.data_ptr() + dw.numel() * dw.element_size() <= base + sink.view.numel() * sink.view.element_size()


def flush_held_folds():
    """run the weight gradients and folds still held (called by the autograd engine when the backward pass is over)"""
    global _held_task
    _flush_held_wgrads()
    flush_held_head(True)   # (no embedding node in this pass, or one that issued nothing)
    if _held_folds:
        arr = _fold_array(_held_folds)
        _native.call("spv_fold_multi", ctypes.addressof(arr), len(_held_folds), _stream())
        _held_folds.clear()
    _held_task = -2
    join_side_stream()   # a batch started early by start_held_wgrads


def _hold_fold(partials, outs, sinks, parts, n):
    """hold a fold for the next weight-gradient reduce of this backward pass.  Only when every output IS its parameter's sink slot
    (memory that outlives the node; autograd adopts the alias without copying), and never by keeping the output tensors themselves:
    a second reference makes AccumulateGrad clone the -- still unfolded -- gradient.  False (not held) otherwise."""
    if not _hold_ok() or not _sunk(outs, sinks):
        return False
    task = _graph_task_id()
    if task < 0:   # not inside a backward pass
        return False
    _begin_pass(task)
    _held_folds.append(_Fold(partials, _addrs(outs), parts, n))
    return True


def _fold_rides(dtype, rows, n, k):
    """the tail backward's fold can ride in this weight gradient's split-K reduce (bf16 TN path on the main stream)"""
    return (dtype == torch.bfloat16 and n % 8 == 0 and k % 8 == 0 and FOLD_RIDE
            and not (not _timing() and 2.0 * rows * n * k >= _SIDE_MIN_FLOPS))


def _fold_job(partials, outs, rows, n):
    """the fold of a tail backward's column sums over `rows` rows (the caller holds `outs` until the weight gradient has been issued)"""
    return _Fold(partials, _addrs(outs), _native.call("spv_tail_bwd_parts", rows), n)


def _sunk(outs, sinks):
    """every gradient tensor IS its parameter's sink slot (memory that outlives the node: its content may be written later)"""
    return all(sk is not None and o.data_ptr() == sk.view.data_ptr() for o, sk in zip(outs, sinks))


def _weight_grad(dh, x, rows, n, k, sink=None, fold=None, fold_sunk=False, out=None):
    """dW[n,k] = dh[rows,n]^T . x[rows,k], split-K over rows.  bf16: TN kernel straight from the row-major activations
    (transposing LDS reads); fp32 (parity path): NT kernel over explicit transposes.  fold (a _fold_job, only when
    _fold_rides): the same layer's dgamma / dbeta / dbias fold, run as extra workgroups of the split-K reduce.
    out: a contiguous [n, k] row range of a larger gradient to write instead (held like the whole slot when it lies in `sink`)."""
    dev = dh.device
    dw = out if out is not None else _grad_buf(sink, (n, k), dev)
    tiles = ((n + 127) // 128) * ((k + 127) // 128)
    # ~2 workgroups per CU: measured optimum on the 768 x 512 x 33280 weight gradient (21 splits: 51 us; 12: 69; 42: 56; 64: 64)
    splits = max(1, min(512 // tiles, (rows + 511) // 512 if tiles >= 8 else (rows + 63) // 64))
    if tiles < 8:
        splits = min(splits, 64)  # the patch-embedding gradient (512 x 48): 128 slices made the reduce (10 us) as long as the GEMM
    elif n == 512 and k % 128 == 0 and k >= 1024 and rows >= 8192:
        # the 512 x 128 tile (spv_gemm_tn takes it from 192 workgroups up): one workgroup per CU
        splits = max(1, min(256 // (k // 128), rows // 2048))
    # (The 256 x 128 tile at 4 slices is 8 % faster on the MHPermutMix gradient [512, 8192, 33280] in isolation -- 320 against 348 us --
    # and SLOWER where it runs, on the side stream beside the data-gradient GEMM and the inverse gather: 701 against ~500 us, step 5.92
    # -> 6.25 ms.  Its 112 KB of LDS per workgroup leave those kernels less of every CU than the 128 x 128 tile's 40 KB.)
    ws = None
    if dh.dtype == torch.bfloat16 and n % 8 == 0 and k % 8 == 0:
        if tiles >= 8 and 2.0 * rows * n * k < _SIDE_MIN_FLOPS and _hold_wgrad(dh, x, dw, sink, rows, n, k, fold, fold_sunk):
            return dw   # computed with the other layers' at the end of the backward pass
        def launch(riders=True):
            nonlocal ws
            if ws is None and splits > 1:
                ws = torch.empty((splits * n * k,), dtype=torch.float32, device=dev)
            folds = [fold] if fold is not None else []
            if riders and _held_task == _graph_task_id():
                while _held_folds and len(folds) < FOLD_RIDERS:
                    folds.append(_held_folds.pop(0))
            if folds:
                arr = _fold_array(folds)
                _native.call("spv_gemm_tn_fold", _p(dh), _p(x), _p(dw), n, k, rows, n, k, k, F32, 0, splits, _p(ws), ctypes.addressof(arr),
                             len(folds), _stream())
            else:
                _native.call("spv_gemm_tn", _p(dh), _p(x), _p(dw), n, k, rows, n, k, k, F32, 0, splits, _p(ws), _stream())
        if not _timing() and 2.0 * rows * n * k >= _SIDE_MIN_FLOPS:
            # a big weight gradient (the MHPermutMix 8192 -> 512 linear: 279 GFLOP) has no consumer inside the backward
            # chain: run it on a second HIP stream so that it fills the ramp/tail gaps of the data-gradient GEMM and
            # overlaps the HBM-bound inverse gather on the main stream (10.57 -> 10.38 ms/step).  Not worth it for the
            # 26-GFLOP layer GEMMs (3.32 -> 3.42 ms/step: the fork/join costs more than the overlap gains).
            # join_side_stream() (end of the calling autograd node) orders everything after it again.
            side = _side_stream(dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                launch(False)  # allocates its split-K workspace from the side stream's pool; held folds stay with the main stream
            _side_keep.append((dh, x, ws, dw))
        else:
            launch()
        return dw
    ws = torch.empty((splits * n * k,), dtype=torch.float32, device=dev) if splits > 1 else None
    ld = (rows + 7) // 8 * 8
    dht = torch.empty((n, ld), dtype=dh.dtype, device=dev)
    xt = torch.empty((k, ld), dtype=x.dtype, device=dev)
    st = _stream()
    _native.call("spv_cast_transpose", _p(dh), _dt(dh), _p(dht), _dt(dht), rows, n, ld, 0, 0, 0, st)
    _native.call("spv_cast_transpose", _p(x), _dt(x), _p(xt), _dt(xt), rows, k, ld, 0, 0, 0, st)
    _gemm(dht, xt, None, dw, n, k, ld, ld, ld, k, 0, splits, ws)
    return dw


class GradSink:
    """A parameter's slot in a flat gradient bucket (installed by spectre_vit.dp.GradReducer as ``p._spv_grad_sink``).
    Backward kernels write a parameter's gradient straight into the slot, so autograd's AccumulateGrad adopts that
    tensor as ``p.grad`` without the extra ``grad += new`` pass over every weight.  ``used`` guards the (never taken
    here) case of a parameter that receives two gradient contributions in one step: the second one goes to fresh memory
    and autograd sums them."""
    __slots__ = ("view", "used")

    def __init__(self, view):
        self.view = view
        self.used = False


def _sink(p):
    return getattr(p, "_spv_grad_sink", None)


def _grad_buf(sink, shape, device):
    if sink is not None and not sink.used and tuple(sink.view.shape) == tuple(shape):
        sink.used = True
        # a FRESH alias of the slot: autograd's AccumulateGrad adopts an incoming gradient as p.grad only when nothing else holds
        # that tensor object (use_count check); returning sink.view itself made it clone the gradient and the reducer copy it back
        return sink.view.detach()
    return torch.empty(shape, dtype=torch.float32, device=device)


def _new_seed():
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _rows2d(x, k):
    """x as a contiguous [rows, k] matrix (a view where x's memory allows)"""
    x2 = x.reshape(-1, k)
    return x2 if x2.is_contiguous() else x2.contiguous()


def _row_stats(rows, dev):
    """(mean, rstd): the fp32 LayerNorm statistics a row kernel writes for its backward"""
    return torch.empty((rows,), dtype=torch.float32, device=dev), torch.empty((rows,), dtype=torch.float32, device=dev)


_CHANNEL_ERRORS = {
    "SpectreLinear": "SpectreLinear({k}->{n}) in {dt}: channel counts must be multiples of {mult}",
    "Linear": "Linear({k}->{n}) in {dt}: feature counts must be multiples of {mult}",
    "MHPermutMix": "MHPermutMix linear ({k}->{n}) in {dt}: channel counts must be multiples of {mult}",
    "patch embedding": "patch embedding: C*P*P={k} and embed_dim={n} must be multiples of {mult}",
}


def _check_channels(kind, n, k, dt):
    """the vector width of the kernels: both channel counts in multiples of 8 (bf16) / 4 (fp32)"""
    mult = 8 if dt == torch.bfloat16 else 4
    if n % mult or k % mult:
        raise ValueError(_CHANNEL_ERRORS[kind].format(n=n, k=k, dt=dt, mult=mult))


def _colsum(d2, out):
    rows, n = d2.shape
    part = torch.empty((min(rows, 512) * n,), dtype=torch.float32, device=d2.device)
    _native.call("spv_colsum", _p(d2), _p(out), _p(part), rows, n, _dt(d2), _stream())
    return out


def _zero_workspace(cache, dev, floats_entry):
    """the zeroed counter block of a loss kernel, `floats_entry` floats, kept in `cache`"""
    key = dev.index   # one loss per step and device; not per stream, so that a graph capture reuses the warm-up's (zeroed) counter
    ws = cache.get(key)
    if ws is None:
        ws = cache[key] = torch.zeros((_native.call(floats_entry),), dtype=torch.float32, device=dev)
    return ws


# Saved-for-backward state of the raw forwards below.  ctx.saved keeps these (not save_for_backward: no version-counter checks).
# _sl_forward -> _sl_backward; sinks = (weight, bias, gamma, beta)
_SLSaved = NamedTuple("_SLSaved", [("x2", _T), ("h", _T), ("mean", _T), ("rstd", _T), ("gamma", _T), ("beta", _T), ("wt", _T),
                                   ("sinks", tuple), ("rows", int), ("n", int), ("k", int), ("p_drop", float), ("seed", int)])
# _addln_forward -> _addln_backward; sinks = (gamma, beta)
_AddLNSaved = NamedTuple("_AddLNSaved", [("a2", _T), ("b2", _T), ("mean", _T), ("rstd", _T), ("gamma", _T), ("sinks", tuple),
                                         ("rows", int), ("n", int), ("mode", int)])
# LayerNorm-2's share of the fused linear3 tail + LayerNorm-2 kernel (FFResidualFn, beside linear3's _SLSaved); sinks = (n2w, n2b)
_TailLN2Saved = NamedTuple("_TailLN2Saved", [("f3", _T), ("x1", _T), ("mean2", _T), ("rstd2", _T), ("n2w", _T), ("sinks", tuple)])
# the fused FNet mixer + LayerNorm-1 kernel (FNetResidualFn); sinks = (n1w, n1b)
_FNetLN1Saved = NamedTuple("_FNetLN1Saved", [("m", _T), ("mean", _T), ("rstd", _T), ("gamma", _T), ("sinks", tuple)])


# ------------------------------------------------------------------------------------------------
# SpectreLinear: GELU(LN(x W^T + b)) + avgpool(x) [+ dropout]      (reference layers.py:76-101)
# ------------------------------------------------------------------------------------------------
def _sl_forward(x2, weight, bias, gamma, beta, p_drop, out_fp32):
    """raw SpectreLinear forward on a contiguous [rows, k] tensor -> (out [rows, n], _SLSaved)"""
    n, k = weight.shape
    rows = x2.shape[0]
    dt = x2.dtype
    _check_channels("SpectreLinear", n, k, dt)
    wc, wt = shadows.get(weight, dt)
    dev = x2.device
    h = torch.empty((rows, n), dtype=dt, device=dev)
    _gemm(x2, wc, bias, h, rows, n, k, k, k, n)
    out = torch.empty((rows, n), dtype=torch.float32 if out_fp32 else dt, device=dev)
    mean, rstd = _row_stats(rows, dev)
    seed = _new_seed() if p_drop > 0.0 else 0
    _native.call("spv_spectre_tail_fwd", _p(h), _p(x2), _p(gamma), _p(beta), _p(out), _p(mean), _p(rstd), rows, n, k,
                 _dt(h), _dt(out), float(p_drop), seed, _stream())
    sinks = (_sink(weight), _sink(bias), _sink(gamma), _sink(beta))
    return out, _SLSaved(x2, h, mean, rstd, gamma, beta, wt, sinks, rows, n, k, float(p_drop), seed)


def _sl_backward(dout2, saved, need_dx=True, dx_add=None, up=None):
    """raw SpectreLinear backward of a contiguous dout2 [rows, n] -> (dx or None, dW, dbias, dgamma, dbeta); dx_add: a gradient of the same input that is
    folded into dx by the tail kernel (saves a separate elementwise add); up = (src, p_drop, seed): the skip gradient of the
    layer above, formed here from its source instead of being written by that layer and accumulated by its GEMM"""
    x2, h, mean, rstd, gamma, beta, wt, sinks, rows, n, k, p_drop, seed = saved
    dev = x2.device
    dh = torch.empty_like(h)
    dx = torch.empty_like(x2)
    s_w, s_b, s_g, s_be = sinks
    dgamma = _grad_buf(s_g, (n,), dev)
    dbeta = _grad_buf(s_be, (n,), dev)
    dbias = _grad_buf(s_b, (n,), dev)
    partials = torch.empty((_native.call("spv_rowop_partial_floats", n),), dtype=torch.float32, device=dev)
    ride = _fold_rides(dh.dtype, rows, n, k)  # the fold of the three column sums rides in the weight gradient's split-K reduce
    pg, pb, pbi = (0, 0, 0) if ride else (_p(dgamma), _p(dbeta), _p(dbias))
    if up is not None:
        _native.call("spv_spectre_tail_bwd_up", _p(dout2), _p(h), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dh), _p(dx),
                     pg, pb, pbi, _p(partials), rows, n, k, _dt(h), _dt(dout2), p_drop, seed,
                     _p(dx_add) if need_dx else 0, _p(up[0]), float(up[1]), int(up[2]), _stream())
    else:
        _native.call("spv_spectre_tail_bwd", _p(dout2), _p(h), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dh), _p(dx),
                     pg, pb, pbi, _p(partials), rows, n, k, _dt(h), _dt(dout2), p_drop, seed,
                     _p(dx_add) if need_dx else 0, _stream())
    dw = _weight_grad(dh, x2, rows, n, k, s_w, _fold_job(partials, (dgamma, dbeta, dbias), rows, n) if ride else None,
                      ride and _sunk((dgamma, dbeta, dbias), (s_g, s_be, s_b)))
    if need_dx:
        _gemm(dh, wt, None, dx, rows, k, n, n, wt.shape[1], k, accumulate=1)
    else:
        dx = None
    return dx, dw, dbias, dgamma, dbeta


class SpectreLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, p_drop, out_fp32):
        _require_gpu(x, weight)
        n, k = weight.shape
        shape = x.shape
        out, saved = _sl_forward(_rows2d(x, k), weight, bias, gamma, beta, p_drop, out_fp32)
        ctx.saved = saved
        ctx.shape = shape
        return out.reshape(*shape[:-1], n)

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved
        dx, dw, dbias, dgamma, dbeta = _sl_backward(_rows2d(dout, saved.n), saved, ctx.needs_input_grad[0])
        join_side_stream()
        return (dx.reshape(ctx.shape) if dx is not None else None), dw, dbias, dgamma, dbeta, None, None


def spectre_linear(x, weight, bias, gamma, beta, p_drop=0.0, out_fp32=False):
    return SpectreLinearFn.apply(x, weight, bias, gamma, beta, p_drop, out_fp32)


# ------------------------------------------------------------------------------------------------
# residual + LayerNorm   mode 0: LN(a) + b (spectre.py:66)    mode 1: LN(a + b) (spectre.py:67)
# ------------------------------------------------------------------------------------------------
def _addln_forward(a2, b2, gamma, beta, mode):
    rows, n = a2.shape
    out = torch.empty_like(a2)
    mean, rstd = _row_stats(rows, a2.device)
    _native.call("spv_add_layernorm_fwd", _p(a2), _p(b2), _p(gamma), _p(beta), _p(out), _p(mean), _p(rstd), rows, n, mode,
                 _dt(a2), _stream())
    return out, _AddLNSaved(a2, b2, mean, rstd, gamma, (_sink(gamma), _sink(beta)), rows, n, mode)


def _addln_backward(d2, saved):
    """d2: contiguous [rows, n]"""
    a2, b2, mean, rstd, gamma, sinks, rows, n, mode = saved
    din = torch.empty_like(a2)
    dgamma = _grad_buf(sinks[0], (n,), a2.device)
    dbeta = _grad_buf(sinks[1], (n,), a2.device)
    partials = torch.empty((_native.call("spv_rowop_partial_floats", n),), dtype=torch.float32, device=a2.device)
    _native.call("spv_add_layernorm_bwd", _p(d2), _p(a2), _p(b2), _p(mean), _p(rstd), _p(gamma), _p(din), _p(dgamma),
                 _p(dbeta), _p(partials), rows, n, mode, _dt(a2), _stream())
    return din, dgamma, dbeta


class AddLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, gamma, beta, mode):
        _require_gpu(a, b)
        n = a.shape[-1]
        out, saved = _addln_forward(_rows2d(a, n), _rows2d(b, n), gamma, beta, mode)
        ctx.saved = saved
        ctx.shape = a.shape
        return out.reshape(a.shape)

    @staticmethod
    def backward(ctx, dout):
        din, dgamma, dbeta = _addln_backward(_rows2d(dout, ctx.saved.n), ctx.saved)
        din = din.reshape(ctx.shape)
        return din, (dout if ctx.saved.mode == 0 else din), dgamma, dbeta, None


def add_layernorm(a, b, gamma, beta, mode):
    return AddLayerNormFn.apply(a, b, gamma, beta, mode)


# ------------------------------------------------------------------------------------------------
# MHPermutMix gather (layers.py:68-72)
# ------------------------------------------------------------------------------------------------
def permut_pack(perms: torch.Tensor, signs: torch.Tensor) -> torch.Tensor:
    _require_gpu(perms, signs)
    heads, d = perms.shape
    # opaque to the caller: wide uint32 tables [2][heads][d] + (when d fits 16 bits) the compact 16-bit / sign-bit tables
    idx = torch.empty((_native.call("spv_permut_table_words", heads, d),), dtype=torch.int32, device=perms.device)
    _native.call("spv_permut_pack", _p(perms.contiguous()), _p(signs.contiguous().float()), _p(idx), heads, d, _stream())
    return idx


class PermutGatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, heads):
        _require_gpu(x, idx)
        B = x.shape[0]
        xc = x.contiguous()
        d = xc.numel() // B
        g = torch.empty((B, heads * d), dtype=x.dtype, device=x.device)
        _native.call("spv_permut_gather_fwd", _p(xc), _p(idx), _p(g), 0, 0, B, heads, d, _dt(xc), _stream())
        ctx.idx = idx
        ctx.meta = (x.shape, B, heads, d)
        return g

    @staticmethod
    def backward(ctx, dg):
        shape, B, heads, d = ctx.meta
        dgc = dg.contiguous()
        dx = torch.empty((B, d), dtype=dg.dtype, device=dg.device)
        _native.call("spv_permut_gather_bwd", _p(dgc), _p(ctx.idx), _p(dx), B, heads, d, _dt(dgc), _stream())
        return dx.reshape(shape), None, None


# ------------------------------------------------------------------------------------------------
# spectral mixers
# ------------------------------------------------------------------------------------------------
_twiddles = {}


def _fnet_twiddle(tokens, device):
    key = (tokens, device)
    t = _twiddles.get(key)
    if t is None:
        t = torch.empty((_native.call("spv_fnet_twiddle_floats", tokens),), dtype=torch.float32, device=device)
        _native.call("spv_fnet_make_twiddle", _p(t), tokens, _stream())
        _twiddles[key] = t
    return t


def _fnet_raw(x, add_in=None):
    B, N, D = x.shape
    xc = x.contiguous()
    y = torch.empty_like(xc)
    wsn = _native.call("spv_fnet_workspace_floats", B, N, D)
    ws = torch.empty((wsn,), dtype=torch.float32, device=x.device) if wsn else None
    tw = _fnet_twiddle(N, x.device)

    _native.call("spv_fnet_mix", _p(xc), _p(y), _p(add_in), _p(tw), B, N, D, _dt(xc), _p(ws), _stream())
    return y


class FNetMixFn(torch.autograd.Function):
    """y = Re(fft2(x)) over the last two axes; symmetric operator => backward is the same kernel."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        return _fnet_raw(x)

    @staticmethod
    def backward(ctx, dy):
        return _fnet_raw(dy)


_hadamard_ws = {}


def _next_pow2(n):
    return 1 << max(0, int(n) - 1).bit_length()


def hadamard_scale(tokens, dim, normalize=True):
    """s of y = crop(H_Np pad(x) H_Dp) s: (Np Dp)^-1/2 (fwht's normalize=True on both axes) or 1; the kernels receive it rounded to float32"""
    return float(_next_pow2(tokens) * _next_pow2(dim)) ** -0.5 if normalize else 1.0


def _hadamard_raw(x, normalize=True, add_in=None):
    B, N, D = x.shape
    xc = x.contiguous()
    y = torch.empty_like(xc)
    wsn = _native.call("spv_hadamard_workspace_floats", B, N, D)
    ws = None
    if wsn:   # one workspace per shape and device, reused by every call (stream-ordered; nothing here synchronises the host)
        key = (B, N, D, xc.device)
        ws = _hadamard_ws.get(key)
        if ws is None:
            ws = _hadamard_ws[key] = torch.empty((wsn,), dtype=torch.float32, device=xc.device)
    if add_in is not None:
        add_in = add_in.contiguous()
    _native.call("spv_hadamard_mix", _p(xc), _p(y), _p(add_in), B, N, D, hadamard_scale(N, D, normalize), _dt(xc), _p(ws), _stream())
    return y


class HadamardMixFn(torch.autograd.Function):
    """y = crop(H_Np . pad(x) . H_Dp) s over the last two axes (reference hadamar.py: fwht on both axes with LearnableHadamard's pad /
    crop); symmetric operator => backward is the same kernel."""

    @staticmethod
    def forward(ctx, x, normalize):
        _require_gpu(x)
        ctx.normalize = normalize
        return _hadamard_raw(x, normalize)

    @staticmethod
    def backward(ctx, dy):
        return _hadamard_raw(dy, ctx.normalize), None


_gfilter_tables = {}


def gfilter_tables(tokens, device):
    """the fp32 DFT table of spv_gfilter_fwd / _bwd for one token count, built once per device"""
    key = (tokens, device)
    t = _gfilter_tables.get(key)
    if t is None:
        t = torch.empty((_native.call("spv_gfilter_table_floats", tokens),), dtype=torch.float32, device=device)
        _native.call("spv_gfilter_make_tables", _p(t), tokens, _stream())
        _gfilter_tables[key] = t
    return t


class GlobalFilterFn(torch.autograd.Function):
    """y = irfft(rfft(x, dim=1, ortho) * W, n=N, dim=1, ortho), W = view_as_complex(complex_weight) (K, D, 2) fp32, K = N // 2 + 1.
    The backward saves nothing but x: one call gives dx and the filter's gradient (fp32, written into the parameter's gradient slot)."""

    @staticmethod
    def forward(ctx, x, complex_weight, tables=None):
        _require_gpu(x, complex_weight)
        B, N, D = x.shape
        if tuple(complex_weight.shape) != (N // 2 + 1, D, 2) or complex_weight.dtype != torch.float32:
            raise ValueError(f"GlobalFilterFn: complex_weight must be float32 {(N // 2 + 1, D, 2)} for x {tuple(x.shape)}, "
                             f"got {complex_weight.dtype} {tuple(complex_weight.shape)}")
        xc = x.contiguous()
        w = complex_weight.detach().contiguous()
        if tables is None:
            tables = gfilter_tables(N, xc.device)
        y = torch.empty_like(xc)
        _native.call("spv_gfilter_fwd", _p(xc), _p(w), _p(y), _p(tables), B, N, D, _dt(xc), 0, _stream())   # no kernel of this version needs a workspace
        ctx.saved = (xc, w, tables, _sink(complex_weight))
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, w, tables, sink = ctx.saved
        B, N, D = xc.shape
        dyc = dy.contiguous()
        dx = torch.empty_like(xc)
        dw = _grad_buf(sink, w.shape, xc.device)
        partials = torch.empty((_native.call("spv_gfilter_partial_floats", B, N, D),), dtype=torch.float32, device=xc.device)
        _native.call("spv_gfilter_bwd", _p(xc), _p(dyc), _p(w), _p(dx), _p(dw), _p(tables), _p(partials), B, N, D, _dt(xc), 0, _stream())
        return dx, dw, None


class RfftRealFn(torch.autograd.Function):
    """rfft(x, dim=-1).real (reference spectre_vit/modules/spectre.py:9-14)."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        D = x.shape[-1]
        xc = _rows2d(x, D)
        y = torch.empty((xc.shape[0], D // 2 + 1), dtype=x.dtype, device=x.device)
        _native.call("spv_rfft_real", _p(xc), _p(y), xc.shape[0], D, 0, _dt(xc), _stream())
        ctx.meta = (x.shape, D)
        return y.reshape(*x.shape[:-1], D // 2 + 1)

    @staticmethod
    def backward(ctx, dy):
        shape, D = ctx.meta
        dyc = _rows2d(dy, D // 2 + 1)
        dx = torch.empty((dyc.shape[0], D), dtype=dy.dtype, device=dy.device)
        _native.call("spv_rfft_real", _p(dyc), _p(dx), dyc.shape[0], D, 1, _dt(dyc), _stream())
        return dx.reshape(shape)


def _haar_raw(x, axis, levels, inverse, zero_mode=False):
    B, N, D = x.shape
    xc = x.contiguous()
    y = torch.empty_like(xc)
    scratch = torch.empty_like(xc) if levels > 1 else None
    _native.call("spv_haar_dwt", _p(xc), _p(y), B, N, D, axis, levels, inverse | (2 if zero_mode else 0), _dt(xc), _p(scratch), _stream())
    return y


class HaarDWTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, axis, levels, zero_mode=False):
        _require_gpu(x)
        ctx.meta = (axis, levels, bool(zero_mode))
        return _haar_raw(x, axis, levels, 0, zero_mode)

    @staticmethod
    def backward(ctx, dy):
        axis, levels, zero_mode = ctx.meta
        return _haar_raw(dy, axis, levels, 1, zero_mode), None, None, None


# ------------------------------------------------------------------------------------------------
# patch embedding  (spectre.py:124-156, patch_embeddings.py:28-43)
# ------------------------------------------------------------------------------------------------
class SpectralFoldFn(torch.autograd.Function):
    """W_full[e,(c,p,q)] = sum_uv proj_w[e,(c,u,v)] fh[u] fw[v] Re(rfft2_ortho)[(u,v),(p,q)]."""

    @staticmethod
    def forward(ctx, proj_w, fh, fw, chans, patch):
        _require_gpu(proj_w)
        E = proj_w.shape[0]
        ready = prologue.take("fold", (proj_w, fh, fw), (chans, patch)) if torch.is_autocast_enabled("cuda") else None
        if ready is not None:   # the step prologue's launch has folded these very tensors already
            wf, wf._spv_bf16 = ready
            ctx.save_for_backward(proj_w, fh, fw)
            ctx.sinks = (_sink(proj_w), _sink(fh), _sink(fw))
            ctx.meta = (E, chans, patch)
            return wf
        wf = torch.empty((E, chans * patch * patch), dtype=torch.float32, device=proj_w.device)
        if torch.is_autocast_enabled("cuda"):   # a bf16 step: the token GEMM's operand comes out of the same launch (PatchEmbedFn picks it up)
            wb = torch.empty(wf.shape, dtype=torch.bfloat16, device=proj_w.device)
            _native.call("spv_spectral_fold_bf16", _p(proj_w), _p(fh), _p(fw), _p(wf), _p(wb), E, chans, patch, _stream())
            wf._spv_bf16 = wb
        else:
            _native.call("spv_spectral_fold", _p(proj_w), _p(fh), _p(fw), _p(wf), E, chans, patch, _stream())
        ctx.save_for_backward(proj_w, fh, fw)
        ctx.sinks = (_sink(proj_w), _sink(fh), _sink(fw))
        ctx.meta = (E, chans, patch)
        return wf

    @staticmethod
    def backward(ctx, dwf):
        proj_w, fh, fw = ctx.saved_tensors
        E, chans, patch = ctx.meta
        dwf = dwf.contiguous()
        dw = _grad_buf(ctx.sinks[0], proj_w.shape, proj_w.device)
        dfh = _grad_buf(ctx.sinks[1], fh.shape, fh.device)
        dfw = _grad_buf(ctx.sinks[2], fw.shape, fw.device)
        scratch = torch.empty_like(proj_w)
        _native.call("spv_spectral_fold_bwd", _p(dwf), _p(proj_w), _p(fh), _p(fw), _p(dw), _p(dfh), _p(dfw), _p(scratch), E,
                     chans, patch, _stream())
        return dw, dfh, dfw, None, None


class _EmbedKey:
    """identity of one PatchEmbedFn node (its output tensor carries it; TapClsFn stashes the CLS-row gradient under it)"""
    __slots__ = ("__weakref__",)


_cls_grad_stash = weakref.WeakKeyDictionary()


class PatchEmbedFn(torch.autograd.Function):
    """tokens[b,0] = cls + pos[0]; tokens[b,1+n] = W_full . patch(b,n) + bias + pos[1+n]."""

    @staticmethod
    def forward(ctx, img, w_full, bias, cls, pos, patch, dtype, norm=None, p_drop=0.0):
        """img: float NCHW (the reference's input contract), or -- SURVEY 8f-3 -- the loader's uint8 NHWC batch with
        norm = (mean[C], inv_std[C]) device tensors: /255 + Normalize are then folded into the patch gather.
        p_drop: the nn.Dropout that follows the embedding (reference spectre.py:156), kept inside this node so that its backward,
        the CLS-row gradient of the global residual and the three column sums are one pass over the token gradient."""
        _require_gpu(img, w_full)
        u8 = img.dtype == torch.uint8
        if u8:
            if norm is None:
                raise ValueError("uint8 images need the (mean, inv_std) normalisation tensors")
            B, H, W, C = img.shape
        else:
            B, C, H, W = img.shape
        E, K = w_full.shape
        Np = (H // patch) * (W // patch)
        T = Np + 1
        dev = img.device
        img = img.contiguous() if u8 else img.contiguous().float()
        _check_channels("patch embedding", E, K, dtype)
        st = _stream()
        # token rows [B][T][K], the CLS slot of every image zero: the GEMM below then writes cls + pos[0] there by itself (its row bias
        # holds that sum in row 0), and the backward's TN weight-gradient GEMM reads the same matrix against dtok as both lie in memory
        patches = None if u8 else prologue.take("patchify", (img,), (patch, dtype))   # made by the step prologue's launch?
        if patches is not None:
            pass
        elif u8:
            patches = torch.empty((B * T, K), dtype=dtype, device=dev)
            _native.call("spv_patchify_u8", _p(img), _p(norm[0]), _p(norm[1]), _p(patches), B, C, H, W, patch, K, 2, _DT[dtype], st)
        else:
            patches = torch.empty((B * T, K), dtype=dtype, device=dev)
            _native.call("spv_patchify", _p(img), _p(patches), B, C, H, W, patch, K, 2, _DT[dtype], st)
        wc = w_full if dtype == torch.float32 else (getattr(w_full, "_spv_bf16", None) if dtype == torch.bfloat16 else None)
        if wc is None:
            wc = _raw_cast(w_full, dtype)
        posbias = prologue.take("posbias", (pos, bias, cls), (Np, E))
        if posbias is None:
            posbias = torch.empty((T, E), dtype=torch.float32, device=dev)
            _native.call("spv_embed_posbias", _p(pos), _p(bias), _p(cls), _p(posbias), Np, E, st)
        tokens = torch.empty((B, T, E), dtype=dtype, device=dev)
        seed = _new_seed() if p_drop > 0.0 else 0
        # the dropout rides in the GEMM's epilogue (the mask spv_dropout would draw from the same seed; the backward re-derives it)
        if TOKEN_EMBED_KERNEL and _native.call("spv_token_embed_supported", B * T, E, K, _DT[dtype]):
            # thin K (16..64), bf16: the kernel that walks row blocks with the weight in registers; the same bits as the call below
            _native.call("spv_token_embed_fwd", _p(patches), _p(wc), _p(posbias), _p(tokens), B * T, E, K, T, float(p_drop), seed, st)
            PATH_COUNTS["token_embed"] += 1
        else:
            _native.call("spv_gemm_nt_grouped_rows_drop", _p(patches), _p(wc), 0, _p(posbias), _p(tokens), B * T, E, K, K, K, E,
                         _DT[dtype], _DT[dtype], T, T, 0, float(p_drop), seed, st)
        # bf16: the backward's TN weight-gradient GEMM reads the patch matrix as it lies here (3 MB), so keep it
        ctx.save_for_backward(None if u8 else img, patches if (dtype == torch.bfloat16 or u8) else None)
        ctx.meta = (B, C, H, W, patch, E, K, Np, T, dtype, cls.shape, pos.shape, float(p_drop), seed)
        ctx.sinks = (_sink(bias), _sink(cls), _sink(pos))
        ctx.key = _EmbedKey()   # TapClsFn hands the CLS-row gradient of the global residual to this node's backward under this key
        tokens._spv_embed_key = ctx.key
        return tokens

    @staticmethod
    def backward(ctx, dtok):
        img, patches = ctx.saved_tensors
        B, C, H, W, patch, E, K, Np, T, dtype, cls_shape, pos_shape, p_drop, seed = ctx.meta
        dev = dtok.device
        st = _stream()
        dtok = dtok.contiguous()
        early = start_held_wgrads()   # the layers' weight gradients, one batched launch on the side stream beside everything below
        gcls = _cls_grad_stash.pop(ctx.key, None)   # (B, E): the global residual's CLS-row gradient, not yet added (TapClsFn)
        if gcls is not None:
            gcls = gcls.to(dtok.dtype).contiguous()
        s_bias, s_cls, s_pos = ctx.sinks
        dpos_full = _grad_buf(s_pos, pos_shape, dev)  # straight into the data-parallel bucket / the optimizer's fixed gradient slot
        dbias = _grad_buf(s_bias, (E,), dev)
        dcls = _grad_buf(s_cls, cls_shape, dev)
        part = torch.empty((_native.call("spv_embed_bwd_groups", B) * T * E,), dtype=torch.float32, device=dev)
        # one pass: + CLS-row gradient, dropout mask, the batch sums of the three parameter gradients; then their fold
        masked = torch.empty_like(dtok) if (gcls is not None or p_drop > 0.0) else None
        _native.call("spv_embed_bwd", _p(dtok), _p(gcls), _p(masked), _p(part), _p(dpos_full), _p(dbias), _p(dcls), B, T, E, p_drop, seed,
                     _dt(dtok), st)
        if masked is not None:
            dtok = masked
        if patches is not None and dtok.dtype == torch.bfloat16:
            # dW = dtok^T . P over all B*T token rows, with P the patch matrix widened by a zero row per image (the CLS
            # row): the TN kernel then takes dtok as it lies in memory -- no transposed copies of a 34 MB tensor
            dwf = _weight_grad(dtok.view(B * T, E), patches, B * T, E, K)
            flush_held_head()   # the class head's parameter gradients: beside the batch, at the end of this node's chain
            if not early:   # (with a batch in flight the end-of-pass callback joins: the spectral fold's backward overlaps it too)
                join_side_stream()
            return None, dwf, dbias, dcls, dpos_full, None, None, None, None
        rows = B * Np
        ld = (rows + 7) // 8 * 8
        dyt = torch.empty((E, ld), dtype=dtok.dtype, device=dev)
        _native.call("spv_cast_transpose", _p(dtok), _dt(dtok), _p(dyt), _dt(dyt), rows, E, ld, Np, T, 1, st)
        pt = torch.empty((K, ld), dtype=dtok.dtype, device=dev)
        if img is None:  # uint8 input: the forward kept the normalised patch matrix instead of a float image
            _native.call("spv_cast_transpose", _p(patches), _dt(patches), _p(pt), _dt(pt), rows, K, ld, Np, T, 1, st)  # token rows -> patch rows
        else:
            _native.call("spv_patchify", _p(img), _p(pt), B, C, H, W, patch, ld, 1, _dt(pt), st)
        dwf = torch.empty((E, K), dtype=torch.float32, device=dev)
        tiles = ((E + 127) // 128) * ((K + 127) // 128)
        splits = max(1, min(1024 // tiles, (ld + 511) // 512))
        ws = torch.empty((splits * E * K,), dtype=torch.float32, device=dev) if splits > 1 else None
        _gemm(dyt, pt, None, dwf, E, K, ld, ld, ld, K, 0, splits, ws)
        return None, dwf, dbias, dcls, dpos_full, None, None, None, None


# CIFAR-100 statistics of the reference loader (spectre_vit/repl/train.py:109-112)
CIFAR100_MEAN = (0.5071, 0.4867, 0.4408)
CIFAR100_STD = (0.2675, 0.2565, 0.2761)


class PixelNorm:
    """(mean, 1/std) per channel for uint8 NHWC input, kept as device tensors."""

    def __init__(self, mean=CIFAR100_MEAN, std=CIFAR100_STD):
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(v) for v in std)
        self._cache = {}

    def tensors(self, device, channels):
        if len(self.mean) != channels or len(self.std) != channels:
            raise ValueError(f"pixel normalisation has {len(self.mean)} channels, the image has {channels}")
        t = self._cache.get(device)
        if t is None:
            t = (torch.tensor(self.mean, dtype=torch.float32, device=device),
                 torch.tensor([1.0 / v for v in self.std], dtype=torch.float32, device=device))
            self._cache[device] = t
        return t

    def __deepcopy__(self, memo):
        return PixelNorm(self.mean, self.std)


def patch_embed(x, w_full, bias, cls, pos, patch, pixel_norm, p_drop=0.0):
    """float NCHW or uint8 NHWC images -> token tensor (B, 1 + patches, E) [-> dropout(p_drop)]."""
    if x.dtype == torch.uint8:
        dt = torch.bfloat16 if torch.is_autocast_enabled("cuda") else torch.float32
        norm = pixel_norm.tensors(x.device, x.shape[-1])
        return PatchEmbedFn.apply(x, w_full, bias, cls, pos, patch, dt, norm, float(p_drop))
    return PatchEmbedFn.apply(x, w_full, bias, cls, pos, patch, compute_dtype(x), None, float(p_drop))


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        _require_gpu(x)
        xc = x.contiguous()
        seed = _new_seed()
        y = torch.empty_like(xc)
        _native.call("spv_dropout", _p(xc), _p(y), xc.numel(), float(p), seed, _dt(xc), _stream())
        ctx.meta = (float(p), seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed = ctx.meta
        dyc = dy.contiguous()
        dx = torch.empty_like(dyc)
        _native.call("spv_dropout", _p(dyc), _p(dx), dyc.numel(), p, seed, _dt(dyc), _stream())
        return dx, None


def dropout(x, p, training):
    if not training or p <= 0.0:
        return x
    return DropoutFn.apply(x, p)


class AddFn(torch.autograd.Function):
    """out = a + b through spv_axpby (the encoder's global residual, spectre.py:103)."""

    @staticmethod
    def forward(ctx, a, b):
        _require_gpu(a, b)
        ac, bc = a.contiguous(), b.contiguous()
        out = torch.empty_like(ac)
        _native.call("spv_axpby", _p(ac), _p(bc), _p(out), 1.0, 1.0, ac.numel(), _dt(ac), _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


class TapClsFn(torch.autograd.Function):
    """x -> (x, x[:, 0, :].copy): the encoder's global residual `output + src` (spectre.py:103) is consumed at the CLS row only
    (spectre.py:198), so SpectreViT takes src's CLS row here, at the entrance of the layer stack.  src then has ONE consumer in the
    autograd graph: its gradient is not accumulated from two full (B, N, E) tensors (a 102 MB torch add per step); the CLS row's
    gradient is added in place to row 0 of the stack's input gradient instead."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        ctx.key = getattr(x, "_spv_embed_key", None)   # x is a PatchEmbedFn output: its backward adds the CLS rows in its own pass
        return x.view_as(x), x[:, 0, :]   # a strided view: the class head reads the CLS rows where they lie

    @staticmethod
    def backward(ctx, gx, gcls):
        if gcls is None:
            return gx
        if gx is None:
            raise RuntimeError("TapClsFn: the layer stack produced no input gradient")
        if ctx.key is not None:
            _cls_grad_stash[ctx.key] = gcls
            return gx
        if not gx.is_contiguous():
            gx = gx.contiguous()
        gx[:, 0, :] += gcls.to(gx.dtype)  # in place: this edge owns the tensor (it was written for it by the first layer's backward)
        return gx


_cls_grad_bufs = {}
# SpectreViT reads the CLS row of the stack's output and nothing else (reference spectre.py:198), and everything behind the LAST
# layer's token mixer works row by row (LayerNorm, SpectreLinear, residual): that layer's feed-forward half only has to exist at the
# CLS rows -- the same logits, loss and gradients (the other rows' gradients are exactly zero in the reference too).
# SPV_FULL_LAST_LAYER=1 computes every row, as the reference does.
LAST_LAYER_CLS_ONLY = os.environ.get("SPV_FULL_LAST_LAYER", "0") == "0"


class TakeClsFn(torch.autograd.Function):
    """x (B, N, E) -> x[:, 0, :] as a contiguous (B, E) tensor.  Backward: the dense gradient that is zero off the CLS row, in the kept
    buffer of _cls_row_gradient (its consumer, the token mixer's backward, only reads it)."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        ctx.meta = (x.shape, x.dtype)
        return x[:, 0, :].contiguous()

    @staticmethod
    def backward(ctx, g):
        shape, dtype = ctx.meta
        return _cls_row_gradient(shape, dtype, g.device, g)


class PermutClsFn(torch.autograd.Function):
    """x (B, N, E) -> (token row 0 of the MHPermutMix gather (B, n), x[:, 0, :] (B, E)): the two things the LAST layer of a stack needs
    of its input when the consumer reads the CLS row only (MHPermutMix.forward_cls).  Backward: ONE dense input gradient -- the CLS
    row's own gradient in row 0, zero elsewhere, + the n scattered values -- instead of two (B, N, E) tensors for autograd to add."""

    @staticmethod
    def forward(ctx, x, table, n):
        _require_gpu(x)
        B, N, E = x.shape
        xc = x.contiguous()
        g0 = torch.empty((B, n), dtype=xc.dtype, device=xc.device)
        x0 = torch.empty((B, E), dtype=xc.dtype, device=xc.device)
        _native.call("spv_permut_row0_fwd", _p(xc), _p(table), _p(g0), _p(x0), B, N * E, n, E, _dt(xc), _stream())
        ctx.table = table
        ctx.meta = (B, N, E, n, xc.dtype)
        return g0, x0

    @staticmethod
    def backward(ctx, dg0, dx0):
        B, N, E, n, dtype = ctx.meta
        dev = ctx.table.device
        dg0 = torch.zeros((B, n), dtype=dtype, device=dev) if dg0 is None else dg0.to(dtype).contiguous()
        dx0 = torch.zeros((B, E), dtype=dtype, device=dev) if dx0 is None else dx0.to(dtype).contiguous()
        dx = torch.empty((B, N, E), dtype=dtype, device=dev)
        _native.call("spv_permut_row0_bwd", _p(dg0), _p(dx0), _p(ctx.table), _p(dx), B, N * E, n, E, _DT[dtype], _stream())
        return dx, None, None


def _cls_row_gradient(shape, dtype, dev, rows):
    """The stack's output gradient when only the CLS rows carry one: a (B, N, E) tensor that is zero off row 0.  The buffer is kept
    across steps -- nothing ever writes its other rows (the consumers read it; TapClsFn adds in place to row 0 only) -- so a step
    costs the CLS-row copy, not a 34 MB fill."""
    if shape[1] == 1:   # the stack handed over its CLS rows only (LAST_LAYER_CLS_ONLY): the gradient is those rows
        return rows.to(dtype).reshape(shape)
    key = (tuple(shape), dtype, dev.index)   # not per stream: a graph capture runs on its own stream and must find the warm-up's buffer
    full = _cls_grad_bufs.get(key)
    if full is None:
        if len(_cls_grad_bufs) > 8:
            _cls_grad_bufs.clear()
        full = torch.zeros(shape, dtype=dtype, device=dev)
        _cls_grad_bufs[key] = full
    full[:, 0, :] = rows
    return full


class ClsAddFn(torch.autograd.Function):
    """(output, src_cls) -> output[:, 0, :] + src_cls: the only rows of `output + src` the model reads.  Backward hands the stack a
    dense gradient that is zero off the CLS row (what slicing the full sum gave it before)."""

    @staticmethod
    def forward(ctx, out, src_cls):
        _require_gpu(out, src_cls)
        ctx.meta = (out.shape, out.dtype)
        return out[:, 0, :] + src_cls

    @staticmethod
    def backward(ctx, g):
        shape, dtype = ctx.meta
        return _cls_row_gradient(shape, dtype, g.device, g), g


# ------------------------------------------------------------------------------------------------
# the step prologue: the small launches that open a graph-replayed training step, as one (csrc/spv_misc.hip: step_prologue_kernel)
# ------------------------------------------------------------------------------------------------
# The seed word's advance, the layer weights' bf16 copies, the spectral embedding's folded projection, the patch rows and the
# position/bias rows are mutually independent and all needed only in front of the token GEMM, yet as five dependent graph nodes each
# paid its own launch and drain.  False: the step issues spv_seed_advance and every node launches for itself, as an eager forward does.
STEP_PROLOGUE = True
# The embedding's token GEMM on spv_token_embed_fwd where spv_token_embed_supported says so (bf16, K = 16..64, E % 64 == 0).  False: every
# call goes to spv_gemm_nt_grouped_rows_drop, as all other shapes do; the two write the same bits (A/B runs, tests).
TOKEN_EMBED_KERNEL = True


def step_prologue(model, img, seed_word, autocast_dtype):
    """ONE launch in front of a graph-replayed step's forward (spectre_vit.graph): the seed word, plus every role whose inputs `model`
    has.  The outputs wait in spectre_vit.prologue for the nodes that would have launched them; a node that finds none launches as
    always, so a role left out here (baseline ViT, SpectreBranch, uint8 images, fp32 steps, a model without the spectral embedding)
    costs nothing but its old launch.  The registry is emptied first: nothing of an earlier step can be served."""
    prologue.clear()
    if not STEP_PROLOGUE:
        _native.call("spv_seed_advance", _p(seed_word), _stream())
        return
    jobs = _native.PrologueJobs()
    jobs.seed_word = _p(seed_word)
    work = 16.0
    deposits = []
    emb = getattr(model, "embeddings_block", None)
    if autocast_dtype == torch.bfloat16 and torch.is_grad_enabled() and img.is_cuda:
        weights_fn = getattr(model, "_shadow_weights", None)
        weights = weights_fn() if callable(weights_fn) else None
        ss = shadows.shadow_set(model, weights) if weights else None
        if ss is not None and ss.dtype == torch.bfloat16:
            table, tt, tx, ty, ntiles = ss._tables
            jobs.shadow_table, jobs.tile_tensor, jobs.tile_x, jobs.tile_y = _p(table), _p(tt), _p(tx), _p(ty)
            jobs.ntiles, jobs.shadow_dtype = ntiles, BF16
            work += 2048.0 * ntiles * 8
            deposits.append(("shadows", weights, (ss.dtype,), ss))
        # the embedding module itself names what its forward will hand SpectralFoldFn and PatchEmbedFn (SpectralPatchEmbed
        # ._prologue_sources); a module without that method launches for itself
        sources_fn = getattr(emb, "_prologue_sources", None)
        sources = sources_fn(img) if callable(sources_fn) and img.dtype == torch.float32 and img.is_contiguous() else None
        if sources is not None:
            (w, fh, fw, C, P), (bias, cls, pos) = sources
            B, _, H, W = img.shape
            dev = img.device
            E, K = w.shape[0], C * P * P
            Np = (H // P) * (W // P)
            fp32 = all(t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda for t in (w, fh, fw, pos, bias, cls))
            if fp32 and P > 0 and H >= P and W >= P and w.dim() == 2 and w.shape[1] == C * P * (P // 2 + 1) and pos.numel() == (Np + 1) * E:
                wf = torch.empty((E, K), dtype=torch.float32, device=dev)
                wb = torch.empty((E, K), dtype=torch.bfloat16, device=dev)
                jobs.fold_w, jobs.fold_fh, jobs.fold_fw, jobs.fold_out, jobs.fold_out_bf16 = _p(w), _p(fh), _p(fw), _p(wf), _p(wb)
                jobs.fold_embed, jobs.fold_chans, jobs.fold_patch = E, C, P
                work += 4.0 * w.numel() + 6.0 * E * K
                deposits.append(("fold", (w, fh, fw), (C, P), (wf, wb)))
                patches = torch.empty((B * (Np + 1), K), dtype=torch.bfloat16, device=dev)
                jobs.patch_img, jobs.patch_out = _p(img), _p(patches)
                jobs.patch_batch, jobs.patch_chans, jobs.patch_height, jobs.patch_width = B, C, H, W
                jobs.patch_size, jobs.patch_ld, jobs.patch_dtype = P, K, BF16
                work += 4.0 * img.numel() + 2.0 * patches.numel()
                deposits.append(("patchify", (img,), (P, torch.bfloat16), patches))
                posbias = torch.empty((Np + 1, E), dtype=torch.float32, device=dev)
                jobs.pos_pos, jobs.pos_bias, jobs.pos_cls, jobs.pos_out = _p(pos), _p(bias), _p(cls), _p(posbias)
                jobs.pos_patches, jobs.pos_embed = Np, E
                work += 8.0 * (Np + 1) * E
                deposits.append(("posbias", (pos, bias, cls), (Np, E), posbias))
    if _timing():
        _native.hint = int(work)
    _native.call("spv_step_prologue", ctypes.addressof(jobs), _stream())
    PATH_COUNTS["step_prologue"] += 1
    for role, sources, extra, value in deposits:
        prologue.deposit(role, sources, extra, value)


# ------------------------------------------------------------------------------------------------
# the classifier end of the step: class head over the CLS rows + mean cross-entropy (csrc/spv_head.hip)
# ------------------------------------------------------------------------------------------------
def small_head_ok(rows: int, n: int, k: int) -> bool:
    return bool(_native.call("spv_small_sl_supported", int(rows), int(n), int(k)))


class ClsHeadFn(torch.autograd.Function):
    """(output, src_cls, head parameters) -> (logits fp32, CLS features fp32): SpectreLinear((output + src)[:, 0]) of the reference
    (spectre.py:198-202, layers.py:95-101) as ONE launch over the fp32 master weights; backward two launches.  The generic path
    (ClsAddFn + cast + fp32 shadow + split-K GEMM + reduce + tail, and five launches more in the backward) costs the same
    arithmetic 13 launches at their 4-6 us floor."""

    @staticmethod
    def forward(ctx, out, src_cls, weight, bias, gamma, beta):
        _require_gpu(out, src_cls, weight)
        B, N, E = out.shape
        n = weight.shape[0]
        if not out.is_contiguous():
            out = out.contiguous()
        if src_cls.stride(-1) != 1:
            src_cls = src_cls.contiguous()
        if src_cls.dtype != out.dtype or weight.dtype != torch.float32 or not weight.is_contiguous():
            raise ValueError("ClsHeadFn: src_cls must have the stack's dtype and the head weight must be contiguous fp32")
        dev = out.device
        logits = torch.empty((B, n), dtype=torch.float32, device=dev)
        h = torch.empty((B, n), dtype=torch.float32, device=dev)
        xs = torch.empty((B, E), dtype=torch.float32, device=dev)
        mean, rstd = _row_stats(B, dev)
        _native.call("spv_small_sl_fwd", _p(out), N * E, _p(src_cls), src_cls.stride(0), _p(weight), _p(bias), _p(gamma), _p(beta), _p(logits), _p(h),
                     _p(xs), _p(mean), _p(rstd), B, n, E, _dt(out), _stream())
        ctx.save_for_backward(h, xs, mean, rstd, weight, gamma, beta)
        ctx.meta = (out.shape, out.dtype)
        ctx.sinks = (_sink(weight), _sink(bias), _sink(gamma), _sink(beta))
        ctx.set_materialize_grads(False)
        return logits, xs

    @staticmethod
    def backward(ctx, dlogits, dfeats):
        h, xs, mean, rstd, weight, gamma, beta = ctx.saved_tensors
        shape, dtype = ctx.meta
        B, n = h.shape
        E = xs.shape[1]
        dev = h.device
        if dlogits is None:
            dlogits = torch.zeros_like(h)
        dlogits = dlogits.contiguous().float()
        s_w, s_b, s_g, s_be = ctx.sinks
        dh = torch.empty_like(h)
        dx = torch.empty((B, E), dtype=dtype, device=dev)
        dw = _grad_buf(s_w, (n, E), dev)
        dbias = _grad_buf(s_b, (n,), dev)
        dgamma = _grad_buf(s_g, (n,), dev)
        dbeta = _grad_buf(s_be, (n,), dev)
        partials = torch.empty((_native.call("spv_small_sl_partial_floats", B, n),), dtype=torch.float32, device=dev)
        _native.call("spv_small_sl_bwd_rows", _p(dlogits), _p(h), _p(mean), _p(rstd), _p(weight), _p(gamma), _p(beta), _p(dh), _p(dx),
                     _p(partials), B, n, E, _DT[dtype], _stream())
        if not _hold_head_wgrad(dh, xs, partials, (dw, dgamma, dbeta, dbias), (s_w, s_g, s_be, s_b), B, n, E):
            _native.call("spv_small_sl_bwd_w", _p(dh), _p(xs), _p(partials), _p(dw), _p(dgamma), _p(dbeta), _p(dbias), B, n, E, _stream())
        if dfeats is not None:
            dx = dx + dfeats.to(dx.dtype)
        return _cls_row_gradient(shape, dtype, dev, dx), dx, dw, dbias, dgamma, dbeta  # the stack's gradient is dense: zero off the CLS row


_ce_workspaces = {}


class CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss() with its defaults (mean over rows; reference repl/train.py:196,226): one launch forward (row-wise
    logsumexp, deterministic sum), one backward -- stock torch runs log_softmax, nll_loss, two fills and their two backwards."""

    @staticmethod
    def forward(ctx, logits, labels):
        _require_gpu(logits, labels)
        if logits.dim() != 2 or logits.dtype != torch.float32 or labels.dtype != torch.int64 or labels.shape != logits.shape[:1]:
            raise ValueError("cross_entropy: fp32 logits [rows, classes] and int64 labels [rows] expected")
        z = logits.contiguous()
        y = labels.contiguous()
        rows, C = z.shape
        lse = torch.empty((rows,), dtype=torch.float32, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        _native.call("spv_cross_entropy_fwd", _p(z), _p(y), _p(lse), _p(loss), _p(_zero_workspace(_ce_workspaces, z.device, "spv_cross_entropy_workspace_floats")), rows, C, _stream())
        ctx.save_for_backward(z, y, lse)
        return loss

    @staticmethod
    def backward(ctx, go):
        z, y, lse = ctx.saved_tensors
        go = go.reshape(1).float().contiguous()
        dz = torch.empty_like(z)
        _native.call("spv_cross_entropy_bwd", _p(z), _p(y), _p(lse), _p(go), _p(dz), z.shape[0], z.shape[1], _stream())
        return dz, None


def _meter_block(meter, dev, what):
    """the block and k of a spectre_vit.meter.TrainMeter, checked against the device of the logits"""
    block = meter.tensor()
    if block.dtype != torch.int64 or not block.is_contiguous() or block.device != dev:
        raise ValueError(f"{what}: the meter's block is a contiguous int64 tensor on the logits' device ({dev}), got {block.dtype} on {block.device}")
    return block, int(meter.topk)


_ce_meter_workspaces = {}


class CrossEntropyMeterFn(torch.autograd.Function):
    """CrossEntropyFn with the training meter (spectre_vit.meter.TrainMeter): the forward launch also counts the batch's top-1 / top-k
    hits and logs the step into the meter's block; loss and lse keep CrossEntropyFn's bits, the backward is CrossEntropyFn's."""

    @staticmethod
    def forward(ctx, logits, labels, meter):
        _require_gpu(logits, labels)
        if logits.dim() != 2 or logits.dtype != torch.float32 or labels.dtype != torch.int64 or labels.shape != logits.shape[:1]:
            raise ValueError("cross_entropy: fp32 logits [rows, classes] and int64 labels [rows] expected")
        block, k = _meter_block(meter, logits.device, "cross_entropy")
        z = logits.contiguous()
        y = labels.contiguous()
        rows, C = z.shape
        lse = torch.empty((rows,), dtype=torch.float32, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        _native.call("spv_cross_entropy_meter_fwd", _p(z), _p(y), _p(lse), _p(loss),
                     _p(_zero_workspace(_ce_meter_workspaces, z.device, "spv_cross_entropy_meter_workspace_floats")), rows, C, _p(block), k, _stream())
        ctx.save_for_backward(z, y, lse)
        return loss

    @staticmethod
    def backward(ctx, go):
        return CrossEntropyFn.backward(ctx, go) + (None,)


def cross_entropy(logits, labels, meter=None):
    """meter (a spectre_vit.meter.TrainMeter): the metered launch -- the same loss bits, and the step logs itself"""
    if meter is not None:
        return CrossEntropyMeterFn.apply(logits, labels, meter)
    return CrossEntropyFn.apply(logits, labels)


def eval_head_stats(device):
    """a zeroed stats block of spv_eval_head: int64 words, [0:3] = seen, top1, topk, [3] = loss_sum (float64 bits)"""
    return torch.zeros((_native.call("spv_eval_head_stats_words"),), dtype=torch.int64, device=device)


def eval_head(logits, labels, n_valid, pred, stats, k=5):
    """One launch at the end of an inference batch (csrc/spv_infer.hip): pred[r] = first maximum of logits[r], and the rows with
    r < n_valid[0] and 0 <= label < classes are ADDED to ``stats`` (eval_head_stats): seen, top-1 and top-k hits as int64, the sum of
    logsumexp(z) - z_y as float64, joined in a fixed order.  n_valid is an int32 device tensor: a captured launch follows it."""
    _require_gpu(logits, labels, n_valid, pred, stats)
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("eval_head: contiguous logits [rows, classes] expected")
    rows, C = logits.shape
    if (labels.dtype != torch.int64 or pred.dtype != torch.int64 or n_valid.dtype != torch.int32 or stats.dtype != torch.int64
            or labels.numel() < rows or pred.numel() < rows or n_valid.numel() < 1
            or stats.numel() < _native.call("spv_eval_head_stats_words")
            or not (labels.is_contiguous() and pred.is_contiguous() and stats.is_contiguous())):
        raise ValueError("eval_head: int64 labels[rows] and pred[rows], an int32 n_valid word and an eval_head_stats block expected")
    _native.call("spv_eval_head", _p(logits), _p(labels), _p(n_valid), _p(pred), _p(stats), rows, C, int(k), _dt(logits), _stream())
    return pred


_distill_workspaces = {}


class DistillLossFn(torch.autograd.Function):
    """w_soft T^2 / B sum p_t (log p_t - log p_s) + w_ce CE (reference repl/train.py:300-302, 334-348): one launch forward, one
    backward -- the stock chain is two divisions, softmax, log_softmax, log, subtract, multiply, sum, two scalings, the cross-entropy
    and autograd's backward of each.  Gradient to the student logits only."""

    @staticmethod
    def forward(ctx, student_logits, teacher_logits, labels, T, w_soft, w_ce):
        _require_gpu(student_logits, teacher_logits, labels)
        z, t = student_logits, teacher_logits
        if (z.dim() != 2 or z.dtype != torch.float32 or t.dtype != torch.float32 or t.shape != z.shape or labels.dtype != torch.int64
                or labels.shape != z.shape[:1]):
            raise ValueError("distill_loss: fp32 student and teacher logits [rows, classes] and int64 labels [rows] expected")
        z, t, y = z.contiguous(), t.detach().contiguous(), labels.contiguous()
        rows, C = z.shape
        lse = torch.empty((3, rows), dtype=torch.float32, device=z.device)
        out = torch.empty((3,), dtype=torch.float32, device=z.device)
        _native.call("spv_distill_loss_fwd", _p(z), _p(t), _p(y), _p(lse), _p(out), _p(_zero_workspace(_distill_workspaces, z.device, "spv_distill_loss_workspace_floats")), rows, C, float(T),
                     float(w_soft), float(w_ce), _stream())
        ctx.save_for_backward(z, t, y, lse)
        ctx.consts = (float(T), float(w_soft), float(w_ce))
        loss, soft, ce = out[0], out[1], out[2]
        ctx.mark_non_differentiable(soft, ce)
        return loss, soft, ce

    @staticmethod
    def backward(ctx, go, _gsoft, _gce):
        z, t, y, lse = ctx.saved_tensors
        T, w_soft, w_ce = ctx.consts
        go = go.reshape(1).float().contiguous()
        dz = torch.empty_like(z)
        _native.call("spv_distill_loss_bwd", _p(z), _p(t), _p(y), _p(lse), _p(go), _p(dz), z.shape[0], z.shape[1], T, w_soft, w_ce, _stream())
        return dz, None, None, None, None, None


_distill_meter_workspaces = {}


class DistillLossMeterFn(torch.autograd.Function):
    """DistillLossFn with the training meter: the forward launch also counts the student's top-1 / top-k hits and logs the step (loss,
    soft, ce) into the meter's block; every output keeps DistillLossFn's bits, the backward is DistillLossFn's."""

    @staticmethod
    def forward(ctx, student_logits, teacher_logits, labels, T, w_soft, w_ce, meter):
        _require_gpu(student_logits, teacher_logits, labels)
        z, t = student_logits, teacher_logits
        if (z.dim() != 2 or z.dtype != torch.float32 or t.dtype != torch.float32 or t.shape != z.shape or labels.dtype != torch.int64
                or labels.shape != z.shape[:1]):
            raise ValueError("distill_loss: fp32 student and teacher logits [rows, classes] and int64 labels [rows] expected")
        block, k = _meter_block(meter, z.device, "distill_loss")
        z, t, y = z.contiguous(), t.detach().contiguous(), labels.contiguous()
        rows, C = z.shape
        lse = torch.empty((3, rows), dtype=torch.float32, device=z.device)
        out = torch.empty((3,), dtype=torch.float32, device=z.device)
        _native.call("spv_distill_loss_meter_fwd", _p(z), _p(t), _p(y), _p(lse), _p(out),
                     _p(_zero_workspace(_distill_meter_workspaces, z.device, "spv_distill_loss_meter_workspace_floats")), rows, C, float(T),
                     float(w_soft), float(w_ce), _p(block), k, _stream())
        ctx.save_for_backward(z, t, y, lse)
        ctx.consts = (float(T), float(w_soft), float(w_ce))
        loss, soft, ce = out[0], out[1], out[2]
        ctx.mark_non_differentiable(soft, ce)
        return loss, soft, ce

    @staticmethod
    def backward(ctx, go, _gsoft, _gce):
        return DistillLossFn.backward(ctx, go, _gsoft, _gce) + (None,)


def distill_loss(student_logits, teacher_logits, labels, T=2.0, w_soft=0.25, w_ce=0.75, meter=None):
    """(loss, soft, ce): the weighted loss (differentiable in the student logits) and the two unweighted terms, detached.
    meter (a spectre_vit.meter.TrainMeter): the metered launch -- the same bits, and the step logs itself."""
    if meter is not None:
        return DistillLossMeterFn.apply(student_logits, teacher_logits, labels, T, w_soft, w_ce, meter)
    return DistillLossFn.apply(student_logits, teacher_logits, labels, T, w_soft, w_ce)


class DistillLossIdxFn(torch.autograd.Function):
    """DistillLossFn with the teacher's rows read from the resident logit cache [n_cache, classes] through the batch's index (int64
    [rows]): the bits of DistillLossFn on cache[index], without the gather.  The cache and the index are read by address -- a captured
    launch follows whatever they hold at replay.  A row whose index lies outside the cache, or whose cache row was never filled (NaN),
    poisons the loss."""

    @staticmethod
    def forward(ctx, student_logits, cache, index, labels, T, w_soft, w_ce):
        _require_gpu(student_logits, cache, index, labels)
        z = student_logits
        if (z.dim() != 2 or z.dtype != torch.float32 or cache.dim() != 2 or cache.dtype != torch.float32 or cache.shape[1] != z.shape[1]
                or cache.shape[0] < 1 or not cache.is_contiguous() or labels.dtype != torch.int64 or labels.shape != z.shape[:1]
                or index.dtype != torch.int64 or index.shape != z.shape[:1]):
            raise ValueError("distill_loss_cached: fp32 student logits [rows, classes], a contiguous fp32 cache [n, classes], int64 index "
                             "[rows] and int64 labels [rows] expected")
        z, t, idx, y = z.contiguous(), cache.detach(), index.contiguous(), labels.contiguous()
        rows, C = z.shape
        lse = torch.empty((3, rows), dtype=torch.float32, device=z.device)
        out = torch.empty((3,), dtype=torch.float32, device=z.device)
        _native.call("spv_distill_loss_idx_fwd", _p(z), _p(t), _p(idx), _p(y), _p(lse), _p(out),
                     _p(_zero_workspace(_distill_workspaces, z.device, "spv_distill_loss_workspace_floats")), rows, t.shape[0], C, float(T),
                     float(w_soft), float(w_ce), _stream())
        ctx.save_for_backward(z, y, lse)
        ctx.resident = (t, idx)   # read by address again in the backward; not save_for_backward: the cache is written in place by design
        ctx.consts = (float(T), float(w_soft), float(w_ce))
        loss, soft, ce = out[0], out[1], out[2]
        ctx.mark_non_differentiable(soft, ce)
        return loss, soft, ce

    @staticmethod
    def backward(ctx, go, _gsoft, _gce):
        z, y, lse = ctx.saved_tensors
        t, idx = ctx.resident
        T, w_soft, w_ce = ctx.consts
        go = go.reshape(1).float().contiguous()
        dz = torch.empty_like(z)
        _native.call("spv_distill_loss_idx_bwd", _p(z), _p(t), _p(idx), _p(y), _p(lse), _p(go), _p(dz), z.shape[0], t.shape[0], z.shape[1], T,
                     w_soft, w_ce, _stream())
        return dz, None, None, None, None, None, None


class DistillLossIdxMeterFn(torch.autograd.Function):
    """DistillLossIdxFn with the training meter (see DistillLossMeterFn): the bits and the backward of DistillLossIdxFn."""

    @staticmethod
    def forward(ctx, student_logits, cache, index, labels, T, w_soft, w_ce, meter):
        _require_gpu(student_logits, cache, index, labels)
        z = student_logits
        if (z.dim() != 2 or z.dtype != torch.float32 or cache.dim() != 2 or cache.dtype != torch.float32 or cache.shape[1] != z.shape[1]
                or cache.shape[0] < 1 or not cache.is_contiguous() or labels.dtype != torch.int64 or labels.shape != z.shape[:1]
                or index.dtype != torch.int64 or index.shape != z.shape[:1]):
            raise ValueError("distill_loss_cached: fp32 student logits [rows, classes], a contiguous fp32 cache [n, classes], int64 index "
                             "[rows] and int64 labels [rows] expected")
        block, k = _meter_block(meter, z.device, "distill_loss_cached")
        z, t, idx, y = z.contiguous(), cache.detach(), index.contiguous(), labels.contiguous()
        rows, C = z.shape
        lse = torch.empty((3, rows), dtype=torch.float32, device=z.device)
        out = torch.empty((3,), dtype=torch.float32, device=z.device)
        _native.call("spv_distill_loss_idx_meter_fwd", _p(z), _p(t), _p(idx), _p(y), _p(lse), _p(out),
                     _p(_zero_workspace(_distill_meter_workspaces, z.device, "spv_distill_loss_meter_workspace_floats")), rows, t.shape[0], C,
                     float(T), float(w_soft), float(w_ce), _p(block), k, _stream())
        ctx.save_for_backward(z, y, lse)
        ctx.resident = (t, idx)
        ctx.consts = (float(T), float(w_soft), float(w_ce))
        loss, soft, ce = out[0], out[1], out[2]
        ctx.mark_non_differentiable(soft, ce)
        return loss, soft, ce

    @staticmethod
    def backward(ctx, go, _gsoft, _gce):
        return DistillLossIdxFn.backward(ctx, go, _gsoft, _gce) + (None,)


def distill_loss_cached(student_logits, cache, index, labels, T=2.0, w_soft=0.25, w_ce=0.75, meter=None):
    """distill_loss(student_logits, cache[index], labels, ...) without materialising cache[index]: (loss, soft, ce)"""
    if meter is not None:
        return DistillLossIdxMeterFn.apply(student_logits, cache, index, labels, T, w_soft, w_ce, meter)
    return DistillLossIdxFn.apply(student_logits, cache, index, labels, T, w_soft, w_ce)


_feature_workspaces = {}


def _add_weighted(base, feat, w):
    """base + w * feat as one launch (base None: w * feat)"""
    if base is None:
        return feat * w
    if base.dim() != 0 or base.dtype != torch.float32 or base.device != feat.device:
        raise ValueError(f"feature_cosine: base is an fp32 scalar tensor on the features' device, got {base.dtype} {tuple(base.shape)}")
    return torch.add(base, feat, alpha=w)


def _check_feature_weight(w):
    w = float(w)
    if not math.isfinite(w):
        raise ValueError(f"feature_cosine: the weight w={w!r} is not finite")
    return w


class FeatureCosineFn(torch.autograd.Function):
    """w * (1 - mean_r cos(s_r, t_r)) and the unweighted term (reference repl/train.py:306, 343-346: two F.normalize, nn.CosineSimilarity,
    mean, 1 -): one launch forward, one backward.  Student features fp32 or bf16 [rows, width], teacher features fp32 or bf16 of the same
    shape; gradient to the student only, in its dtype.  Returns (base + w * feat, feat) as fp32 device scalars, feat detached; base
    (the loss the term is added to, a scalar tensor or None for 0) passes its gradient through untouched, so adding the term to a loss
    costs one small launch forward and none backward."""

    @staticmethod
    def forward(ctx, student_feat, teacher_feat, w, base=None):
        _require_gpu(student_feat, teacher_feat)
        s, t = student_feat, teacher_feat
        if (s.dim() != 2 or t.shape != s.shape or s.dtype not in (torch.float32, torch.bfloat16)
                or t.dtype not in (torch.float32, torch.bfloat16) or s.shape[0] < 1 or s.shape[1] < 1):
            raise ValueError("feature_cosine: fp32 or bf16 student and teacher features of one shape [rows, width] expected, got "
                             f"{s.dtype} {tuple(s.shape)} and {t.dtype} {tuple(t.shape)}")
        w = _check_feature_weight(w)
        s, t = s.contiguous(), t.detach().contiguous()
        rows, width = s.shape
        stat = torch.empty((3, rows), dtype=torch.float32, device=s.device)
        out = torch.empty((1,), dtype=torch.float32, device=s.device)
        _native.call("spv_feature_cosine_fwd", _p(s), _p(t), _p(stat), _p(out),
                     _p(_zero_workspace(_feature_workspaces, s.device, "spv_feature_cosine_workspace_floats")), rows, width, _dt(s), _dt(t),
                     _stream())
        ctx.save_for_backward(s, t, stat)
        ctx.w = w
        feat = out[0]
        ctx.mark_non_differentiable(feat)
        return _add_weighted(base, feat, w), feat

    @staticmethod
    def backward(ctx, go, _gfeat):
        s, t, stat = ctx.saved_tensors
        go = go.reshape(1).float().contiguous()
        ds = torch.empty_like(s)
        _native.call("spv_feature_cosine_bwd", _p(s), _p(t), _p(stat), _p(go), _p(ds), s.shape[0], s.shape[1], _dt(s), _dt(t), ctx.w, _stream())
        return ds, None, None, go.reshape(()) if ctx.needs_input_grad[3] else None


class FeatureCosineIdxFn(torch.autograd.Function):
    """FeatureCosineFn with the teacher's rows read from the resident fp32 feature cache [n_cache, width] through the batch's index (int64
    [rows]): the bits of FeatureCosineFn on cache[index], without the gather.  Cache and index are read by address -- a captured launch
    follows whatever they hold at replay.  A row whose index lies outside the cache, or whose cache row was never filled (NaN), poisons
    the term and gets a NaN gradient row."""

    @staticmethod
    def forward(ctx, student_feat, cache, index, w, base=None):
        _require_gpu(student_feat, cache, index)
        s = student_feat
        if (s.dim() != 2 or s.dtype not in (torch.float32, torch.bfloat16) or cache.dim() != 2 or cache.dtype != torch.float32
                or cache.shape[1] != s.shape[1] or cache.shape[0] < 1 or not cache.is_contiguous() or s.shape[0] < 1 or s.shape[1] < 1
                or index.dtype != torch.int64 or index.shape != s.shape[:1]):
            raise ValueError("feature_cosine_cached: fp32 or bf16 student features [rows, width], a contiguous fp32 cache [n, width] and an "
                             f"int64 index [rows] expected, got {s.dtype} {tuple(s.shape)}, {cache.dtype} {tuple(cache.shape)}, "
                             f"{index.dtype} {tuple(index.shape)}")
        w = _check_feature_weight(w)
        s, t, idx = s.contiguous(), cache.detach(), index.contiguous()
        rows, width = s.shape
        stat = torch.empty((3, rows), dtype=torch.float32, device=s.device)
        out = torch.empty((1,), dtype=torch.float32, device=s.device)
        _native.call("spv_feature_cosine_idx_fwd", _p(s), _p(t), _p(idx), _p(stat), _p(out),
                     _p(_zero_workspace(_feature_workspaces, s.device, "spv_feature_cosine_workspace_floats")), rows, t.shape[0], width,
                     _dt(s), _stream())
        ctx.save_for_backward(s, stat)
        ctx.resident = (t, idx)   # read by address again in the backward (see DistillLossIdxFn)
        ctx.w = w
        feat = out[0]
        ctx.mark_non_differentiable(feat)
        return _add_weighted(base, feat, w), feat

    @staticmethod
    def backward(ctx, go, _gfeat):
        s, stat = ctx.saved_tensors
        t, idx = ctx.resident
        go = go.reshape(1).float().contiguous()
        ds = torch.empty_like(s)
        _native.call("spv_feature_cosine_idx_bwd", _p(s), _p(t), _p(idx), _p(stat), _p(go), _p(ds), s.shape[0], t.shape[0], s.shape[1], _dt(s),
                     ctx.w, _stream())
        return ds, None, None, None, go.reshape(()) if ctx.needs_input_grad[4] else None


def feature_cosine(student_feat, teacher_feat, w=1.0, base=None):
    """(base + w * feat, feat): feat = 1 - mean_r cos(student_feat[r], teacher_feat[r]); the first is differentiable in the student
    features (and in base, a scalar loss tensor; None: 0)"""
    return FeatureCosineFn.apply(student_feat, teacher_feat, w, base)


def feature_cosine_cached(student_feat, cache, index, w=1.0, base=None):
    """feature_cosine(student_feat, cache[index], w, base) without materialising cache[index]"""
    return FeatureCosineIdxFn.apply(student_feat, cache, index, w, base)


# ------------------------------------------------------------------------------------------------
# baseline ViT pieces: plain Linear, GELU, softmax attention core  (reference vit.py:30-40)
# ------------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    """y = x W^T + b on the MFMA GEMM (nn.Linear: in_proj / out_proj / linear1 / linear2 / the ViT head)."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_fp32):
        _require_gpu(x, weight)
        n, k = weight.shape
        x2 = _rows2d(x, k)
        rows = x2.shape[0]
        _check_channels("Linear", n, k, x2.dtype)
        wc, wt = shadows.get(weight, x2.dtype)
        y = torch.empty((rows, n), dtype=torch.float32 if out_fp32 else x2.dtype, device=x2.device)
        _gemm(x2, wc, bias, y, rows, n, k, k, k, n)
        ctx.save_for_backward(x2, weight)
        ctx.wt = wt
        ctx.sinks = (_sink(weight), _sink(bias))
        ctx.meta = (x.shape, rows, n, k, bias is not None)
        return y.reshape(*x.shape[:-1], n)

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        shape, rows, n, k, has_bias = ctx.meta
        dy2 = dy.reshape(rows, n)
        if dy2.dtype != x2.dtype:
            dy2 = _raw_cast(dy2, x2.dtype)
        elif not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dw = _weight_grad(dy2, x2, rows, n, k, ctx.sinks[0])
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x2)
            _gemm(dy2, ctx.wt, None, dx, rows, k, n, n, ctx.wt.shape[1], k)
            dx = dx.reshape(shape)
        db = None
        if has_bias:
            db = _colsum(dy2, _grad_buf(ctx.sinks[1], (n,), x2.device))
        join_side_stream()
        return dx, dw, db, None


def linear(x, weight, bias=None, out_fp32=False):
    return LinearFn.apply(x, weight, bias, out_fp32)


class GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        xc = x.contiguous()
        y = torch.empty_like(xc)
        _native.call("spv_gelu_fwd", _p(xc), _p(y), xc.numel(), _dt(xc), _stream())
        ctx.save_for_backward(xc)
        return y

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        dyc = dy.contiguous()
        dx = torch.empty_like(xc)
        _native.call("spv_gelu_bwd", _p(dyc), _p(xc), _p(dx), xc.numel(), _dt(xc), _stream())
        return dx


class AttentionFn(torch.autograd.Function):
    """ctx = dropout(softmax(q k^T / sqrt(hd))) v per (sequence, head); qkv [seqs, len, 3E] -> [seqs, len, E]."""

    @staticmethod
    def forward(ctx, qkv, heads, p_drop):
        _require_gpu(qkv)
        seqs, length, e3 = qkv.shape
        E = e3 // 3
        hd = E // heads
        q = qkv.contiguous()
        out = torch.empty((seqs, length, E), dtype=q.dtype, device=q.device)
        probs = torch.empty((seqs, heads, length, length), dtype=q.dtype, device=q.device)
        seed = _new_seed() if p_drop > 0.0 else 0
        _native.call("spv_attention_fwd", _p(q), _p(out), _p(probs), seqs, length, heads, hd, _dt(q), float(p_drop), seed, _stream())
        ctx.save_for_backward(q, probs)
        ctx.meta = (seqs, length, heads, hd, float(p_drop), seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, probs = ctx.saved_tensors
        seqs, length, heads, hd, p_drop, seed = ctx.meta
        d = dout.contiguous()
        dqkv = torch.empty_like(q)
        ds = torch.empty_like(probs)
        _native.call("spv_attention_bwd", _p(d), _p(q), _p(probs), _p(ds), _p(dqkv), seqs, length, heads, hd, _dt(q), p_drop, seed,
                     _stream())
        return dqkv, None, None


def attn_row0_ok(x, heads):
    """the single-query-row kernels take x (B, N, E) with `heads` heads (include/spv.h spv_attention_row0_fwd)"""
    E, cv = x.shape[-1], (8 if x.dtype == torch.bfloat16 else 4)
    return E % heads == 0 and E % cv == 0 and E <= 256 * cv and heads * x.shape[1] <= 8192


def _row0_fwd(q0, kv, heads, p_drop, seed):
    """ctx0 (B, E) and the saved probabilities (B, heads, N) fp32 of query row 0 against kv (B, N, 2E) = [k | v]"""
    B, N, E2 = kv.shape
    E = E2 // 2
    ctx0 = torch.empty((B, E), dtype=q0.dtype, device=q0.device)
    probs = torch.empty((B, heads, N), dtype=torch.float32, device=q0.device)
    _native.call("spv_attention_row0_fwd", _p(q0), _p(kv), _p(kv) + E * kv.element_size(), E2, _p(ctx0), _p(probs), B, N, heads,
                 E // heads, _dt(q0), float(p_drop), seed, _stream())
    return ctx0, probs


def _row0_bwd(dctx0, q0, kv, probs, heads, p_drop, seed):
    """(dq0 (B, E), dkv (B, N, 2E) = [dk | dv], every key row written)"""
    B, N, E2 = kv.shape
    E = E2 // 2
    dq0 = torch.empty_like(q0)
    dkv = torch.empty_like(kv)
    _native.call("spv_attention_row0_bwd", _p(dctx0), _p(q0), _p(kv), _p(kv) + E * kv.element_size(), E2, _p(probs), _p(dq0), _p(dkv),
                 _p(dkv) + E * dkv.element_size(), E2, B, N, heads, E // heads, _dt(q0), float(p_drop), seed, _stream())
    return dq0, dkv


def _grad_in(g, like):
    """an incoming gradient in the compute dtype and dense (zeros when autograd hands None)"""
    if g is None:
        return torch.zeros_like(like)
    return g.to(like.dtype).contiguous()


class AttentionRow0Fn(torch.autograd.Function):
    """ctx0 = dropout(softmax(q0 k^T / sqrt(hd))) v for query row 0 only: q0 (B, E), kv (B, N, 2E) = [k | v] -> (B, E).  The same
    numbers, dropout mask included, as row 0 of AttentionFn over [q | k | v] with the same seed."""

    @staticmethod
    def forward(ctx, q0, kv, heads, p_drop):
        _require_gpu(q0, kv)
        q0, kv = q0.contiguous(), kv.contiguous()
        seed = _new_seed() if p_drop > 0.0 else 0
        ctx0, probs = _row0_fwd(q0, kv, heads, p_drop, seed)
        ctx.save_for_backward(q0, kv, probs)
        ctx.meta = (heads, float(p_drop), seed)
        return ctx0

    @staticmethod
    def backward(ctx, dctx0):
        q0, kv, probs = ctx.saved_tensors
        heads, p_drop, seed = ctx.meta
        dq0, dkv = _row0_bwd(_grad_in(dctx0, q0), q0, kv, probs, heads, p_drop, seed)
        return dq0, dkv, None, None


class AttnClsFn(torch.autograd.Function):
    """The attention mixer's part of a CLS-only last layer (SelfAttentionMixer.forward_cls): x (B, N, E) -> (attention context of
    query row 0 (B, E), x[:, 0, :] (B, E)).  K and V are projected over every row with rows E..3E of in_proj_weight (one GEMM, N = 2E),
    Q at the CLS rows only with rows 0..E; the out-projection is the caller's (a plain Linear over B rows).  Backward: ONE dense input
    gradient, and in_proj's gradient as one (3E, E) tensor whose two row blocks are written by the two weight-gradient GEMMs."""

    @staticmethod
    def forward(ctx, x, w_in, b_in, heads, p_drop):
        _require_gpu(x, w_in)
        B, N, E = x.shape
        xc = x.contiguous()
        dt = xc.dtype
        x2 = xc.view(B * N, E)
        x0 = xc[:, 0, :].contiguous()
        wc, wt = shadows.get(w_in, dt)   # (the cached copies of the whole parameter, sliced: the cache is keyed on the parameter)
        bq = bk = None
        if b_in is not None:
            bq, bk = b_in[:E], b_in[E:]
        kv = torch.empty((B, N, 2 * E), dtype=dt, device=xc.device)
        _gemm(x2, wc[E:], bk, kv, B * N, 2 * E, E, E, E, 2 * E)
        q0 = torch.empty((B, E), dtype=dt, device=xc.device)
        _gemm(x0, wc[:E], bq, q0, B, E, E, E, E, E)
        seed = _new_seed() if p_drop > 0.0 else 0
        ctx0, probs = _row0_fwd(q0, kv, heads, p_drop, seed)
        ctx.save_for_backward(x2, x0, q0, kv, probs)
        ctx.wt = wt
        ctx.sinks = (_sink(w_in), _sink(b_in) if b_in is not None else None)
        ctx.meta = (B, N, E, heads, float(p_drop), seed, b_in is not None)
        return ctx0, x0

    @staticmethod
    def backward(ctx, dctx0, dx0):
        x2, x0, q0, kv, probs = ctx.saved_tensors
        B, N, E, heads, p_drop, seed, has_bias = ctx.meta
        dev = x2.device
        dq0, dkv = _row0_bwd(_grad_in(dctx0, q0), q0, kv, probs, heads, p_drop, seed)
        dkv2 = dkv.view(B * N, 2 * E)
        dw = db = None
        if ctx.needs_input_grad[1]:
            dw = _grad_buf(ctx.sinks[0], (3 * E, E), dev)
            _weight_grad(dq0, x0, B, E, E, ctx.sinks[0], out=dw[:E])
            _weight_grad(dkv2, x2, B * N, 2 * E, E, ctx.sinks[0], out=dw[E:])
        if has_bias and ctx.needs_input_grad[2]:
            db = _grad_buf(ctx.sinks[1], (3 * E,), dev)
            part = torch.empty((min(B * N, 512) * 2 * E,), dtype=torch.float32, device=dev)
            _native.call("spv_colsum", _p(dq0), _p(db), _p(part), B, E, _dt(dq0), _stream())
            _native.call("spv_colsum", _p(dkv2), _p(db) + 4 * E, _p(part), B * N, 2 * E, _dt(dkv2), _stream())
        dx = None
        if ctx.needs_input_grad[0]:
            wt = ctx.wt
            dx = torch.empty((B, N, E), dtype=x2.dtype, device=dev)
            # dx = dkv . W_kv over every row, then row 0 += dq0 . W_q + the CLS row's own gradient
            _gemm(dkv2, wt[:, E:], None, dx, B * N, E, 2 * E, 2 * E, wt.shape[1], E)
            _gemm(dq0, wt, None, dx, B, E, E, E, wt.shape[1], N * E, accumulate=1)
            if dx0 is not None:
                dx[:, 0, :] += dx0.to(dx.dtype)
        join_side_stream()
        return dx, dw, db, None, None


# ------------------------------------------------------------------------------------------------
# fused halves of the encoder layer: same kernels, hand-written backward so that the residual-stream gradients are
# folded into the producing kernels instead of being summed by separate elementwise passes
# ------------------------------------------------------------------------------------------------
class FFResidualFn(torch.autograd.Function):
    """x2 = LayerNorm2(x1 + SpectreLinear3(SpectreLinear1(x1)))   (reference spectre.py:67,70-73)."""

    @staticmethod
    def forward(ctx, x1, w1, b1, g1, be1, w3, b3, g3, be3, n2w, n2b, p_drop):
        _require_gpu(x1, w1)
        shape = x1.shape
        x2d = _rows2d(x1, shape[-1])
        f1, s1 = _sl_forward(x2d, w1, b1, g1, be1, p_drop, False)
        ctx.shape = shape
        n3, k3 = w3.shape
        if _native.call("spv_tail_ln_supported", n3, k3, _dt(f1)):
            # linear3's GEMM, then ONE row kernel: LayerNorm/GELU/pooled skip/dropout of the SpectreLinear tail, + x1, LayerNorm-2
            rows, dt, dev = f1.shape[0], f1.dtype, f1.device
            wc3, wt3 = shadows.get(w3, dt)
            h3 = torch.empty((rows, n3), dtype=dt, device=dev)
            _gemm(f1, wc3, b3, h3, rows, n3, k3, k3, k3, n3)
            f3 = torch.empty_like(h3)
            out = torch.empty_like(h3)
            mean3, rstd3 = _row_stats(rows, dev)
            mean2, rstd2 = _row_stats(rows, dev)
            seed = _new_seed() if p_drop > 0.0 else 0
            _native.call("spv_spectre_tail_ln_fwd", _p(h3), _p(f1), _p(g3), _p(be3), _p(f3), _p(mean3), _p(rstd3), _p(x2d), _p(n2w),
                         _p(n2b), _p(out), _p(mean2), _p(rstd2), rows, n3, k3, _dt(h3), float(p_drop), seed, _stream())
            s3 = _SLSaved(f1, h3, mean3, rstd3, g3, be3, wt3, (_sink(w3), _sink(b3), _sink(g3), _sink(be3)), rows, n3, k3, float(p_drop), seed)
            ctx.saved = (s1, s3, _TailLN2Saved(f3, x2d, mean2, rstd2, n2w, (_sink(n2w), _sink(n2b))))
            return out.reshape(shape)
        f3, s3 = _sl_forward(f1, w3, b3, g3, be3, p_drop, False)
        out, sn = _addln_forward(f3, x2d, n2w, n2b, 1)
        ctx.saved = (s1, s3, sn)
        return out.reshape(shape)

    @staticmethod
    def backward(ctx, dout):
        s1, s3, sn = ctx.saved
        if isinstance(sn, _TailLN2Saved):  # LayerNorm-2 backward inside the linear3 tail backward
            f3, x1, mean2, rstd2, n2w, sinks2 = sn
            f1, h3, mean3, rstd3, g3, be3, wt3, sinks3, rows, n, k, p_drop, seed = s3
            dev = f1.device
            d2 = _rows2d(dout, n)
            ds = torch.empty_like(f3)
            dh3 = torch.empty_like(h3)
            df1 = torch.empty_like(f1)
            s_w, s_b, s_g, s_be = sinks3
            dg3, dbe3, db3 = _grad_buf(s_g, (n,), dev), _grad_buf(s_be, (n,), dev), _grad_buf(s_b, (n,), dev)
            dn2w, dn2b = _grad_buf(sinks2[0], (n,), dev), _grad_buf(sinks2[1], (n,), dev)
            partials = torch.empty((_native.call("spv_tail_ln_partial_floats", n),), dtype=torch.float32, device=dev)
            # linear3's skip gradient (its transposed pooling) is taken by linear1's tail backward from `ds` itself when the
            # shapes allow: df1 is then a plain GEMM output (no [rows, 768] tensor written here and re-read by the GEMM)
            defer = _native.call("spv_tail_up_supported", s1.n, s1.k, _dt(h3)) and s1.n == k
            ride = _fold_rides(dh3.dtype, rows, n, k)   # the five column sums' fold rides in the weight gradient's split-K reduce
            pp = (lambda t: 0) if ride else _p
            _native.call("spv_spectre_tail_ln_bwd", _p(d2), _p(f3), _p(x1), _p(mean2), _p(rstd2), _p(n2w), _p(ds), pp(dn2w), pp(dn2b),
                         _p(h3), _p(mean3), _p(rstd3), _p(g3), _p(be3), _p(dh3), 0 if defer else _p(df1), pp(dg3), pp(dbe3), pp(db3),
                         _p(partials), rows, n, k, _dt(h3), p_drop, seed, _stream())
            dw3 = _weight_grad(dh3, f1, rows, n, k, s_w, _fold_job(partials, (dg3, dbe3, db3, dn2w, dn2b), rows, n) if ride else None,
                               ride and _sunk((dg3, dbe3, db3, dn2w, dn2b), (s_g, s_be, s_b, sinks2[0], sinks2[1])))
            _gemm(dh3, wt3, None, df1, rows, k, n, n, wt3.shape[1], k, accumulate=0 if defer else 1)
            up = (ds, p_drop, seed) if defer else None
        else:
            ds, dn2w, dn2b = _addln_backward(_rows2d(dout, sn.n), sn)      # d(x1 + f3)
            df1, dw3, db3, dg3, dbe3 = _sl_backward(ds, s3, True)
            up = None
        dx1, dw1, db1, dg1, dbe1 = _sl_backward(df1, s1, True, dx_add=ds, up=up)  # + the residual path, folded in
        join_side_stream()
        return dx1.reshape(ctx.shape), dw1, db1, dg1, dbe1, dw3, db3, dg3, dbe3, dn2w, dn2b, None


class FNetResidualFn(torch.autograd.Function):
    """x1 = LayerNorm1(Re(fft2(x))) + x   (reference spectre.py:66 with the 'fft_bare' mixer)."""

    @staticmethod
    def forward(ctx, x, n1w, n1b):
        _require_gpu(x)
        B, N, D = x.shape
        xc = x.contiguous()
        ctx.shape = (B, N, D)
        if _native.call("spv_fnet_ln_supported", N, D, _dt(xc)):
            # one kernel: mixer, LayerNorm statistics per finished row, residual
            dev = xc.device
            m = torch.empty_like(xc)
            out = torch.empty_like(xc)
            mean, rstd = _row_stats(B * N, dev)
            tw = _fnet_twiddle(N, dev)
            _native.call("spv_fnet_ln_fwd", _p(xc), _p(m), _p(out), _p(n1w), _p(n1b), _p(mean), _p(rstd), _p(tw), B, N, D, _dt(xc),
                         _stream())
            ctx.saved = _FNetLN1Saved(m, mean, rstd, n1w, (_sink(n1w), _sink(n1b)))
            return out
        m = _fnet_raw(xc)
        out, sn = _addln_forward(m.reshape(-1, D), xc.reshape(-1, D), n1w, n1b, 0)
        ctx.saved = sn
        return out.reshape(B, N, D)

    @staticmethod
    def backward(ctx, dout):
        sn = ctx.saved
        B, N, D = ctx.shape
        d2 = _rows2d(dout, D)
        if isinstance(sn, _FNetLN1Saved):
            m, mean, rstd, gamma, sinks = sn
            dev = m.device
            dx = torch.empty_like(m)
            dn1w = _grad_buf(sinks[0], (D,), dev)
            dn1b = _grad_buf(sinks[1], (D,), dev)
            partials = torch.empty((B * 2 * D,), dtype=torch.float32, device=dev)
            tw = _fnet_twiddle(N, dev)
            # the fold of the per-sample column sums travels with the next weight-gradient reduce (the layer below's); only into
            # sink memory -- a fresh tensor would be copied by autograd before the fold has run
            held = _hold_fold(partials, (dn1w, dn1b), sinks, B, D)
            _native.call("spv_fnet_ln_bwd", _p(d2), _p(m), _p(mean), _p(rstd), _p(gamma), _p(dx), 0 if held else _p(dn1w),
                         0 if held else _p(dn1b), _p(partials), _p(tw), B, N, D, _dt(m), _stream())
            return dx, dn1w, dn1b
        dm, dn1w, dn1b = _addln_backward(d2, sn)
        dx = _fnet_raw(dm.reshape(B, N, D), add_in=d2)  # symmetric operator; + the residual gradient, folded in
        return dx, dn1w, dn1b


def fnet_cls_ok(x):
    """row 0 of the FFT mixer + LayerNorm-1 + residual can come from the one-FFT kernels (spv_fnet_cls_fwd / _bwd)"""
    return x.is_cuda and x.dim() == 3 and x.dtype in _DT and bool(_native.call("spv_fnet_cls_supported", x.shape[1], x.shape[2], _dt(x)))


class FNetClsFn(torch.autograd.Function):
    """x (B, N, D) -> (LayerNorm1(Re(fft2(x))) + x)[:, 0, :] as (B, D): what the LAST layer of a stack needs of FNetResidualFn when the
    consumer reads the CLS row only.  Token frequency 0 is the sum over tokens, so the row is ONE D-point FFT of the token sum
    (spv_fnet_cls_fwd: one pass over x); the backward hands every token the same spectrum (+ the residual's gradient in row 0)."""

    @staticmethod
    def forward(ctx, x, n1w, n1b):
        _require_gpu(x)
        B, N, D = x.shape
        xc = x.contiguous()
        dev = xc.device
        out = torch.empty((B, D), dtype=xc.dtype, device=dev)
        m0 = torch.empty((B, D), dtype=torch.float32, device=dev)
        mean, rstd = _row_stats(B, dev)
        _native.call("spv_fnet_cls_fwd", _p(xc), _p(n1w), _p(n1b), _p(out), _p(m0), _p(mean), _p(rstd), B, N, D, _dt(xc), _stream())
        ctx.saved = (m0, mean, rstd, n1w, (_sink(n1w), _sink(n1b)))
        ctx.meta = (B, N, D, xc.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        m0, mean, rstd, n1w, sinks = ctx.saved
        B, N, D, dtype = ctx.meta
        dev = m0.device
        g = g.to(dtype).contiguous()
        dx = torch.empty((B, N, D), dtype=dtype, device=dev)
        dn1w = _grad_buf(sinks[0], (D,), dev)
        dn1b = _grad_buf(sinks[1], (D,), dev)
        partials = torch.empty((B * 2 * D,), dtype=torch.float32, device=dev)
        _native.call("spv_fnet_cls_bwd", _p(g), _p(m0), _p(mean), _p(rstd), _p(n1w), _p(dx), _p(partials), B, N, D, _DT[dtype], _stream())
        if not _hold_fold(partials, (dn1w, dn1b), sinks, B, D):   # the batch sums of dgamma / dbeta: with the next reduce, or now
            arr = _fold_array([_Fold(partials, _addrs((dn1w, dn1b)), B, D)])
            _native.call("spv_fold_multi", ctypes.addressof(arr), 1, _stream())
        return dx, dn1w, dn1b


def hadamard_ln_ok(x):
    """the Hadamard mixer + LayerNorm-1 + residual can run as the fused kernels (spv_hadamard_ln_fwd / _bwd)"""
    return x.is_cuda and x.dim() == 3 and x.dtype in _DT and bool(_native.call("spv_hadamard_ln_supported", x.shape[1], x.shape[2], _dt(x)))


def hadamard_cls_ok(x):
    """row 0 of the same node can come from the one-transform kernels (spv_hadamard_cls_fwd / _bwd)"""
    return x.is_cuda and x.dim() == 3 and x.dtype in _DT and bool(_native.call("spv_hadamard_cls_supported", x.shape[1], x.shape[2], _dt(x)))


class HadamardResidualFn(torch.autograd.Function):
    """x1 = LayerNorm1(hadamard_mix(x)) + x   (reference spectre.py:66 with the Walsh-Hadamard mixer): one kernel each way inside
    spv_hadamard_ln_supported's window, spv_hadamard_mix + the LayerNorm kernels outside it."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, normalize):
        _require_gpu(x)
        B, N, D = x.shape
        xc = x.contiguous()
        ctx.shape = (B, N, D)
        ctx.normalize = normalize
        if _native.call("spv_hadamard_ln_supported", N, D, _dt(xc)):
            dev = xc.device
            m = torch.empty_like(xc)
            out = torch.empty_like(xc)
            mean, rstd = _row_stats(B * N, dev)
            _native.call("spv_hadamard_ln_fwd", _p(xc), _p(m), _p(out), _p(n1w), _p(n1b), _p(mean), _p(rstd), hadamard_scale(N, D, normalize),
                         B, N, D, _dt(xc), _stream())
            ctx.saved = _FNetLN1Saved(m, mean, rstd, n1w, (_sink(n1w), _sink(n1b)))
            return out
        m = _hadamard_raw(xc, normalize)
        out, sn = _addln_forward(m.reshape(-1, D), xc.reshape(-1, D), n1w, n1b, 0)
        ctx.saved = sn
        return out.reshape(B, N, D)

    @staticmethod
    def backward(ctx, dout):
        sn = ctx.saved
        B, N, D = ctx.shape
        d2 = _rows2d(dout, D)
        if isinstance(sn, _FNetLN1Saved):
            m, mean, rstd, gamma, sinks = sn
            dev = m.device
            dx = torch.empty_like(m)
            dn1w = _grad_buf(sinks[0], (D,), dev)
            dn1b = _grad_buf(sinks[1], (D,), dev)
            partials = torch.empty((B * 2 * D,), dtype=torch.float32, device=dev)
            held = _hold_fold(partials, (dn1w, dn1b), sinks, B, D)   # the fold travels with the next weight-gradient reduce
            _native.call("spv_hadamard_ln_bwd", _p(d2), _p(m), _p(mean), _p(rstd), _p(gamma), _p(dx), 0 if held else _p(dn1w),
                         0 if held else _p(dn1b), _p(partials), hadamard_scale(N, D, ctx.normalize), B, N, D, _dt(m), _stream())
            return dx, dn1w, dn1b, None
        dm, dn1w, dn1b = _addln_backward(d2, sn)
        dx = _hadamard_raw(dm.reshape(B, N, D), ctx.normalize, add_in=d2)  # symmetric operator; + the residual gradient, folded in
        return dx, dn1w, dn1b, None


class HadamardClsFn(torch.autograd.Function):
    """x (B, N, D) -> (LayerNorm1(hadamard_mix(x)) + x)[:, 0, :] as (B, D): row 0 of H_Np is all ones, so the row is ONE D-point transform
    of the token sum (spv_hadamard_cls_fwd: one pass over x); the backward hands every token the same transformed row (+ the residual's
    gradient in row 0)."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, normalize):
        _require_gpu(x)
        B, N, D = x.shape
        xc = x.contiguous()
        dev = xc.device
        out = torch.empty((B, D), dtype=xc.dtype, device=dev)
        m0 = torch.empty((B, D), dtype=torch.float32, device=dev)
        mean, rstd = _row_stats(B, dev)
        scale = hadamard_scale(N, D, normalize)
        _native.call("spv_hadamard_cls_fwd", _p(xc), _p(n1w), _p(n1b), _p(out), _p(m0), _p(mean), _p(rstd), scale, B, N, D, _dt(xc), _stream())
        ctx.saved = (m0, mean, rstd, n1w, (_sink(n1w), _sink(n1b)))
        ctx.meta = (B, N, D, xc.dtype, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        m0, mean, rstd, n1w, sinks = ctx.saved
        B, N, D, dtype, scale = ctx.meta
        dev = m0.device
        g = g.to(dtype).contiguous()
        dx = torch.empty((B, N, D), dtype=dtype, device=dev)
        dn1w = _grad_buf(sinks[0], (D,), dev)
        dn1b = _grad_buf(sinks[1], (D,), dev)
        partials = torch.empty((B * 2 * D,), dtype=torch.float32, device=dev)
        _native.call("spv_hadamard_cls_bwd", _p(g), _p(m0), _p(mean), _p(rstd), _p(n1w), _p(dx), _p(partials), scale, B, N, D, _DT[dtype],
                     _stream())
        if not _hold_fold(partials, (dn1w, dn1b), sinks, B, D):   # the batch sums of dgamma / dbeta: with the next reduce, or now
            arr = _fold_array([_Fold(partials, _addrs((dn1w, dn1b)), B, D)])
            _native.call("spv_fold_multi", ctypes.addressof(arr), 1, _stream())
        return dx, dn1w, dn1b, None


class HaarResidualFn(torch.autograd.Function):
    """x1 = LayerNorm1(haar(x)) + x, one-level Haar DWT along the embedding axis (reference spectre.py:66 with the 'dwt_embed' mixer of
    BASELINE config 3): one row kernel each way (spv_haar_ln_fwd / _bwd; the transform is lane-local, nothing of the mixer is stored)."""

    @staticmethod
    def forward(ctx, x, n1w, n1b):
        _require_gpu(x)
        xc = x.contiguous()
        D = xc.shape[-1]
        rows = xc.numel() // D
        dev = xc.device
        out = torch.empty_like(xc)
        mean, rstd = _row_stats(rows, dev)
        _native.call("spv_haar_ln_fwd", _p(xc), _p(n1w), _p(n1b), _p(out), _p(mean), _p(rstd), rows, D, _dt(xc), _stream())
        ctx.save_for_backward(xc, mean, rstd, n1w)
        ctx.sinks = (_sink(n1w), _sink(n1b))
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, mean, rstd, n1w = ctx.saved_tensors
        D = xc.shape[-1]
        rows = xc.numel() // D
        dev = xc.device
        d2 = dout.contiguous()
        dx = torch.empty_like(xc)
        dn1w = _grad_buf(ctx.sinks[0], (D,), dev)
        dn1b = _grad_buf(ctx.sinks[1], (D,), dev)
        partials = torch.empty((_native.call("spv_rowop_partial_floats", D),), dtype=torch.float32, device=dev)
        # the fold of the column sums travels with the next weight-gradient reduce of the backward pass (sink memory only: _hold_fold)
        held = _hold_fold(partials, (dn1w, dn1b), ctx.sinks, _native.call("spv_tail_bwd_parts", rows), D)
        _native.call("spv_haar_ln_bwd", _p(d2), _p(xc), _p(mean), _p(rstd), _p(n1w), _p(dx), 0 if held else _p(dn1w), 0 if held else _p(dn1b),
                     _p(partials), rows, D, _dt(xc), _stream())
        return dx, dn1w, dn1b


def haar_ln_ok(x, axis, levels):
    return bool(axis == "embed" and levels == 1 and x.is_cuda and x.dtype == torch.bfloat16
                and _native.call("spv_haar_ln_supported", x.shape[-1], _dt(x)))


class PermutMixFn(torch.autograd.Function):
    """MHPermutMix as one autograd node: SpectreLinear(gather(x)) (reference layers.py:68-73).

    Forward: the gather kernel also emits the averages of every `heads` consecutive gathered elements, which is exactly
    the SpectreLinear skip (AdaptiveAvgPool1d(E) over E*heads channels), so the tail kernel does not re-read the 16x larger
    gathered tensor.  Backward: the transposed pooling is added in the data-gradient GEMM's epilogue instead of being
    written to and re-read from a (B*N, E*heads) buffer."""

    @staticmethod
    def forward(ctx, x, idx, heads, weight, bias, gamma, beta):
        _require_gpu(x, weight)
        B = x.shape[0]
        xc = x.contiguous()
        d = xc.numel() // B
        n, k = weight.shape
        total = heads * d
        rows = (B * total) // k
        dt = xc.dtype
        _check_channels("MHPermutMix", n, k, dt)
        pw = k // n if k % n == 0 else 0
        es = 2 if dt == torch.bfloat16 else 4
        can_pool = pw in (4, 8, 16, 32) and (d * es) % 16 == 0 and d * es <= 150 * 1024 and (total // 4) % 1024 == 0 and total % pw == 0
        if not can_pool and pw > 0 and total % pw == 0:   # rows longer than the LDS (Base / 224, window 12): the scatter gather pools too
            can_pool = bool(_native.call("spv_permut_pool_supported", heads, d, pw, _dt(xc)))
        dev = xc.device
        g = torch.empty((rows, k), dtype=dt, device=dev)
        pooled = torch.empty((rows, n), dtype=dt, device=dev) if can_pool else None
        st = _stream()
        _native.call("spv_permut_gather_fwd", _p(xc), _p(idx), _p(g), _p(pooled), pw, B, heads, d, _dt(xc), st)
        wc, wt = shadows.get(weight, dt)
        h = torch.empty((rows, n), dtype=dt, device=dev)
        _gemm(g, wc, bias, h, rows, n, k, k, k, n)
        out = torch.empty((rows, n), dtype=dt, device=dev)
        mean, rstd = _row_stats(rows, dev)
        skip = pooled if can_pool else g
        _native.call("spv_spectre_tail_fwd", _p(h), _p(skip), _p(gamma), _p(beta), _p(out), _p(mean), _p(rstd), rows, n,
                     n if can_pool else k, _dt(h), _dt(out), 0.0, 0, st)
        ctx.save_for_backward(g, h, mean, rstd, gamma, beta)
        ctx.aux = (idx, wt, (_sink(weight), _sink(bias), _sink(gamma), _sink(beta)), x.shape, B, heads, d, rows, n, k, pw)
        return out.reshape(B, rows // B, n)

    @staticmethod
    def backward(ctx, dout):
        g, h, mean, rstd, gamma, beta = ctx.saved_tensors
        idx, wt, sinks, xshape, B, heads, d, rows, n, k, pw = ctx.aux
        dev = g.device
        st = _stream()
        d2 = _rows2d(dout, n)
        s_w, s_b, s_g, s_be = sinks
        dh = torch.empty_like(h)
        dgamma = _grad_buf(s_g, (n,), dev)
        dbeta = _grad_buf(s_be, (n,), dev)
        dbias = _grad_buf(s_b, (n,), dev)
        partials = torch.empty((_native.call("spv_rowop_partial_floats", n),), dtype=torch.float32, device=dev)
        dg = torch.empty_like(g)
        fast = pw > 0
        _native.call("spv_spectre_tail_bwd", _p(d2), _p(h), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dh), 0 if fast else _p(dg),
                     _p(dgamma), _p(dbeta), _p(dbias), _p(partials), rows, n, k, _dt(h), _dt(d2), 0.0, 0, 0, st)
        dw = _weight_grad(dh, g, rows, n, k, s_w)  # side stream: overlaps the data gradient and the inverse gather
        if fast:
            _native.call("spv_gemm_nt_pool_bwd", _p(dh), _p(wt), _p(dg), _p(d2), pw, rows, k, n, n, wt.shape[1], k, _dt(dh),
                         _dt(dg), _dt(d2), st)
        else:
            _gemm(dh, wt, None, dg, rows, k, n, n, wt.shape[1], k, accumulate=1)
        dx = torch.empty((B, d), dtype=g.dtype, device=dev)
        _native.call("spv_permut_gather_bwd", _p(dg), _p(idx), _p(dx), B, heads, d, _dt(dg), st)
        join_side_stream()
        return dx.reshape(xshape), None, None, dw, dbias, dgamma, dbeta


def __getattr__(name):
    """the SpectreBranch ops lived here before branch_ops.py: callers that still ask here for one are served from there"""
    if not name.startswith("_"):
        from . import branch_ops
        if hasattr(branch_ops, name):
            return getattr(branch_ops, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
