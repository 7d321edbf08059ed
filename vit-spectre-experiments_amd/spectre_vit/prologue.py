"""The single-use registry between the step prologue and the nodes that would otherwise launch its roles themselves.

A graph-replayed training step opens with ONE launch (``spv_step_prologue``, issued by ``hip_ops.step_prologue``) that does the work of
five small ones: the dropout seed word, the layer weights' compute-dtype copies, the spectral embedding's folded projection, the patch
rows and the position/bias rows.  Their outputs wait here until ``SpectralFoldFn.forward``, ``PatchEmbedFn.forward`` and
``shadows.refresh_weight_shadows`` ask for them.

An entry is keyed by its role, by the IDENTITY of the source tensors -- data pointer, shape and dtype of each -- and by the role's
scalar arguments.  ``take`` removes what it returns, so an entry serves one consumer; a consumer whose key does not match gets
``None`` and launches as it always did.  ``clear`` runs at every prologue call: what nobody took (a model that skipped a node) can
never be served to a later step, whose parameters have changed.  Pure host code: nothing here touches the GPU library.
"""
from __future__ import annotations

_entries = {}


def ident(*tensors):
    """identity of source tensors: (data pointer, shape, dtype) of each"""
    return tuple((int(t.data_ptr()), tuple(t.shape), t.dtype) for t in tensors)


def clear():
    _entries.clear()


def deposit(role, sources, extra, value):
    """`value` is what the prologue prepared for `role` from the tensors `sources` with the scalar arguments `extra`"""
    _entries[(role, ident(*sources), tuple(extra))] = value


def take(role, sources, extra=()):
    """the prepared value for exactly these sources and arguments, removed from the registry -- or None"""
    if not _entries:
        return None
    return _entries.pop((role, ident(*sources), tuple(extra)), None)


def pending():
    """roles still waiting for their consumer (tests and diagnostics)"""
    return sorted(k[0] for k in _entries)
