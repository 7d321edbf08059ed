"""Weight shadows: the compute-dtype copy of W and of W^T, rebuilt only when the parameter changes.

Three providers share one allocation helper and one table builder: ``_ShadowCache`` (per weight, on demand), ``ShadowSet`` (a model's
layer weights, one launch per training forward) and ``PinnedShadows`` (fixed addresses for an InferenceSession's captured forward).
"""
from __future__ import annotations

import contextlib
import weakref

import torch

from . import _native, prologue
from ._launch import _DT, _p, _stream


def _pair(w, dtype):
    """allocate (W in dtype, W^T in dtype padded to 8 columns) -- fp32 aliases the weight itself -- and fill them (one launch)"""
    n, k = w.shape
    wd = w.detach()
    wc = wd if dtype == torch.float32 else torch.empty((n, k), dtype=dtype, device=w.device)
    ldt = (n + 7) // 8 * 8
    wt = torch.empty((k, ldt), dtype=dtype, device=w.device)
    _native.call("spv_weight_shadows", _p(wd), 0 if wc is wd else _p(wc), _p(wt), n, k, ldt, _DT[dtype], _stream())
    return wc, wt


def _multi_table(ents):
    """[(w, wc, wt)] -> (int64 table of {src, plain, tr, (rows, cols), ld} rows, the three int32 lists of 32 x 64 tiles, tile count)
    of one spv_weight_shadows_multi launch; `plain` is 0 where wc is the weight's own storage (fp32: nothing to copy)"""
    dev = ents[0][0].device
    rows, tt, tx, ty = [], [], [], []
    for i, (w, wc, wt) in enumerate(ents):
        n, k = w.shape
        ld = wt.shape[1]
        rows += [w.data_ptr(), 0 if wc.data_ptr() == w.data_ptr() else wc.data_ptr(), wt.data_ptr(), n | (k << 32), ld]
        for by in range((ld + 31) // 32):
            for bx in range((k + 63) // 64):
                tt.append(i)
                tx.append(bx)
                ty.append(by)
    return (torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(tt, dtype=torch.int32).to(dev),
            torch.tensor(tx, dtype=torch.int32).to(dev), torch.tensor(ty, dtype=torch.int32).to(dev), len(tt))


def _refresh_multi(tables, dtype):
    table, tt, tx, ty, ntiles = tables
    _native.call("spv_weight_shadows_multi", table.data_ptr(), tt.data_ptr(), tx.data_ptr(), ty.data_ptr(), ntiles, _DT[dtype], _stream())


class _ShadowCache:
    """(weight tensor, dtype) -> (W in dtype, W^T in dtype, padded to 8 columns).

    While a weight is being trained (grad mode on, requires_grad) the shadows are rebuilt at every forward: optimizers may
    update parameters without touching the tensor's version counter -- ``torch.optim.AdamW(fused=True)`` does exactly that --
    so no cheap test can prove a cached copy current, and a stale copy would silently freeze the layer.  Outside training
    (eval / no_grad inference loops) entries are reused, validated by a weak reference to the parameter (ids and addresses
    are recycled once a tensor dies), its version counter and the global optimizer-step epoch."""

    def __init__(self):
        self._d = {}
        self._fresh = {}
        self.epoch = 0

    def get(self, w: torch.Tensor, dtype: torch.dtype):
        if _pinned is not None:   # an InferenceSession's forward: its own fixed buffers, never this cache's
            return _pinned.get(w, dtype)
        key = (id(w), dtype)
        ent = self._d.get(key)
        ver = (w.data_ptr(), w._version, tuple(w.shape), self.epoch)
        training = torch.is_grad_enabled() and w.requires_grad
        if not training and ent is not None and ent[0]() is w and ent[1] == ver:
            return ent[2], ent[3]
        fresh = self._fresh.pop(key, None)
        # rebuilt for THIS forward by refresh_weight_shadows (one launch for all weights); void if an optimizer has stepped since
        if fresh is not None and fresh[0]() is w and fresh[3] == (w._version, self.epoch):
            return fresh[1], fresh[2]
        wc, wt = _pair(w, dtype)
        if len(self._d) > 1024:
            self._d = {kk: e for kk, e in self._d.items() if e[0]() is not None}
        self._d[key] = (weakref.ref(w), ver, wc, wt)
        return wc, wt

    def reset(self):
        """drop (and free) every cached and every fresh entry; the epoch only ever grows"""
        self._d = {}
        self._fresh = {}


_shadows = _ShadowCache()
get = _shadows.get


def reset_shadow_cache():
    """Forget every copy the cache holds: the next forward casts each weight again (a graph capture must record those launches)."""
    _shadows.reset()


class ShadowSet:
    """Persistent bf16 (W, W^T) copies of a fixed list of fp32 nn.Linear weights, rebuilt by ONE spv_weight_shadows_multi launch
    per training forward (eight 4.9-us launches and sixteen allocations per step otherwise).  The copies are handed to the layers
    through _ShadowCache.get, which consumes them once per weight and forward."""

    def __init__(self, weights, dtype=torch.bfloat16):
        self.weights = [weakref.ref(w) for w in weights]
        self.dtype = dtype
        self.key = tuple((w.data_ptr(), tuple(w.shape)) for w in weights)
        dev = weights[0].device
        self.bufs = [(torch.empty(tuple(w.shape), dtype=dtype, device=dev),
                      torch.empty((w.shape[1], (w.shape[0] + 7) // 8 * 8), dtype=dtype, device=dev)) for w in weights]
        self._tables = _multi_table([(w, wc, wt) for w, (wc, wt) in zip(weights, self.bufs)])

    def refresh(self):
        _refresh_multi(self._tables, self.dtype)
        self.mark_fresh()

    def mark_fresh(self):
        """the copies were just rebuilt (by refresh, or by the step prologue's launch): hand them to this forward's layers"""
        for wr, (wc, wt) in zip(self.weights, self.bufs):
            w = wr()
            if w is not None:
                _shadows._fresh[(id(w), self.dtype)] = (wr, wc, wt, (w._version, _shadows.epoch))


class PinnedShadows:
    """(W, W^T) copies at FIXED addresses, owned by one spectre_vit.inference.InferenceSession.  While the session's forward runs
    (``with pinned_shadows(p):`` -- warm-up and capture) every ``_ShadowCache.get`` is served from here: the eager warm-up allocates
    and fills a weight's copies on first sight, the capture then finds them and launches nothing, so a replay neither casts a weight
    nor reads memory that ``invalidate_weight_shadows`` or ``reset_shadow_cache`` could free.  ``refresh()`` recasts every copy in
    place with one spv_weight_shadows_multi launch per dtype."""

    def __init__(self):
        self.ent = {}      # (id(w), dtype) -> (w, W in dtype, W^T in dtype); w is held: the session owns the weights it reads
        self._tables = {}  # dtype -> (entries, table and tile tensors of _multi_table)

    def get(self, w, dtype):
        key = (id(w), dtype)
        e = self.ent.get(key)
        if e is not None and e[0] is w:
            return e[1], e[2]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a weight asked for its compute-dtype copies for the first time inside a graph capture: the warm-up "
                               "forward must run the very launch sequence that is captured")
        wc, wt = _pair(w, dtype)
        self.ent[key] = (w, wc, wt)
        return wc, wt

    def refresh(self):
        for dtype in {dt for _, dt in self.ent}:
            ents = [e for (_, dt), e in self.ent.items() if dt == dtype]
            t = self._tables.get(dtype)
            if t is None or t[0] != len(ents):
                t = self._tables[dtype] = (len(ents), _multi_table(ents))
            _refresh_multi(t[1], dtype)


_pinned = None


@contextlib.contextmanager
def pinned_shadows(p):
    global _pinned
    prev, _pinned = _pinned, p
    try:
        yield p
    finally:
        _pinned = prev


def shadow_set(module, weights):
    """module._spv_shadow_set, (re)built when a weight moved or changed shape; None where it cannot be built (inside a capture)"""
    ss = getattr(module, "_spv_shadow_set", None)
    key = tuple((w.data_ptr(), tuple(w.shape)) for w in weights)
    if ss is None or ss.key != key:
        if torch.cuda.is_current_stream_capturing():
            return None  # (tables cannot be uploaded inside a capture: the per-weight path serves this forward)
        ss = ShadowSet(weights)
        object.__setattr__(module, "_spv_shadow_set", ss)
    return ss


def refresh_weight_shadows(module, weights_fn):
    """called at the top of a model's bf16 training forward: one launch rebuilds every copy of module._spv_shadow_set -- unless the
    step prologue has just done so for exactly these weights (spectre_vit.prologue), in which case nothing is launched"""
    weights = weights_fn()
    if not weights:
        return
    ss = shadow_set(module, weights)
    if ss is None:
        return
    if prologue.take("shadows", weights, (ss.dtype,)) is ss:
        ss.mark_fresh()
    else:
        ss.refresh()


def invalidate_weight_shadows(*_args, **_kwargs):
    """Drop every cached bf16 / transposed weight copy (needed only after updating weights in place, outside autograd's
    view, between two no_grad forwards).  Registered as a global optimizer post-step hook."""
    _shadows.epoch += 1


from torch.optim.optimizer import register_optimizer_step_post_hook as _register_post_step  # noqa: E402

_register_post_step(invalidate_weight_shadows)  # any torch optimizer's step() invalidates the inference-time cache
