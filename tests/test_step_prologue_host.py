"""The single-use registry of the step prologue (spectre_vit/prologue.py): host code only, nothing native is called."""
import torch

from spectre_vit import prologue


def setup_function(_):
    prologue.clear()


def test_an_entry_is_consumed_once():
    a, b = torch.zeros(4, 3), torch.zeros(3)
    value = object()
    prologue.deposit("fold", (a, b), (3, 4), value)
    assert prologue.pending() == ["fold"]
    assert prologue.take("fold", (a, b), (3, 4)) is value
    assert prologue.take("fold", (a, b), (3, 4)) is None and prologue.pending() == []


def test_a_mismatch_in_pointer_shape_or_dtype_falls_back():
    a = torch.zeros(8, 6)
    value = object()
    prologue.deposit("patchify", (a,), (4, torch.bfloat16), value)
    assert prologue.take("patchify", (a.clone(),), (4, torch.bfloat16)) is None           # same shape and dtype, another address
    assert prologue.take("patchify", (a.view(6, 8),), (4, torch.bfloat16)) is None        # same address, another shape
    assert prologue.take("patchify", (a.view(torch.int32),), (4, torch.bfloat16)) is None  # same address and shape, another dtype
    assert prologue.take("patchify", (a,), (2, torch.bfloat16)) is None                   # another scalar argument
    assert prologue.take("posbias", (a,), (4, torch.bfloat16)) is None                    # another role
    assert prologue.take("patchify", (a, a), (4, torch.bfloat16)) is None                 # another number of sources
    # none of the misses consumed or disturbed the entry
    assert prologue.take("patchify", (a,), (4, torch.bfloat16)) is value


def test_identity_is_pointer_shape_dtype():
    a = torch.zeros(5, 2)
    assert prologue.ident(a) == ((a.data_ptr(), (5, 2), torch.float32),)
    assert prologue.ident(a, a[1:]) [1] == (a.data_ptr() + 8, (4, 2), torch.float32)


def test_a_second_prologue_call_clears_leftovers():
    a = torch.zeros(2)
    prologue.deposit("shadows", (a,), (torch.bfloat16,), "old")
    prologue.deposit("posbias", (a,), (1, 2), "old")
    prologue.clear()   # what hip_ops.step_prologue does first
    assert prologue.pending() == []
    assert prologue.take("shadows", (a,), (torch.bfloat16,)) is None and prologue.take("posbias", (a,), (1, 2)) is None
    prologue.deposit("posbias", (a,), (1, 2), "new")
    assert prologue.take("posbias", (a,), (1, 2)) == "new"
