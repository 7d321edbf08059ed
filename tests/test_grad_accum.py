"""On-device gradient accumulation, the host side (no GPU): the restatement's own invariants (tests/accum_ref.py), the new symbols
and their declarations, the C-ABI's and the constructor's refusals before any launch, the harness's arguments, and the optimizer
without the option (its control block, its keys and its state_dict are what they were)."""
import os
import struct
import warnings

import numpy as np
import pytest
import torch

import accum_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 5, 2048, 2049, 4095]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_restatement_counts_over_three_windows_with_a_nonfinite_micro_step(k):
    """3 windows of k micro-steps, an inf in the middle window's middle micro-step, skip_nonfinite on: micro runs 1 .. k-1, 0; apply
    is 1 only at the boundaries of windows 1 and 3; the schedule ticks once per window, dropped or not; one window is skipped; and
    outside a boundary no other field of the block moves"""
    rng = np.random.default_rng(k)
    ref = R.AccumRef(k, SIZES, schedule=(8, 3, 1e-5), max_grad_norm=1.0, skip_nonfinite=True)
    assert len(ref.block_bytes()) == 64
    bad = k + k // 2   # a micro-step of window 2 (its only one for k = 1)
    for m in range(3 * k):
        grads = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
        if m == bad:
            grads[4][2048] = np.inf   # the first slot of a short last chunk
        before = dict(ref.ctl)
        want_acc = [g.copy() if m % k == 0 else (a + g).astype(np.float32) for a, g in zip(ref.acc, grads)]
        c = ref.micro_step(grads)
        window, boundary = m // k, m % k == k - 1
        assert c["micro"] == (m + 1) % k
        assert all(np.array_equal(a, w) for a, w in zip(ref.acc, want_acc))
        if not boundary:
            assert c["apply"] == 0
            assert {f: c[f] for f in c if f not in ("apply", "micro")} == {f: before[f] for f in before if f not in ("apply", "micro")}
            continue
        assert c["apply"] == (0 if window == 1 else 1)
        assert c["sched_step"] == window + 1
        assert c["skipped"] == (1 if window >= 1 else 0)
        a, b = R.cosine_ab(window, 3, 8, 1e-5)
        assert (c["a"], c["b"]) == (a, b)
        if window != 1:   # the norm of the mean gradient, the clip coefficient with the 1 / k folded in
            norm = np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in ref.acc)) / k
            assert abs(float(c["grad_norm"]) - norm) <= 1e-6 * norm
            assert abs(float(c["clip_coef"]) - min(1.0, 1.0 / (norm + 1e-6)) / k) <= 1e-6 / k
        else:
            assert not np.isfinite(ref.sumsq)
    assert ref.adam_steps == 2 and ref.ctl["sched_step"] == 3 and ref.ctl["skipped"] == 1 and ref.ctl["micro"] == 0
    assert all(np.isfinite(a).all() for a in ref.acc), "window 3 opened with an assignment: nothing of window 2's inf is left"


def test_restatement_sum_of_squares_order_and_k1():
    """the chunk sum against a plain float64 sum (a few ulp), non-finite exactly when an element is; k = 1: every step is a boundary
    and the block is the plain control path's (norm of the gradient itself, clip coefficient undivided)"""
    rng = np.random.default_rng(0)
    for n in (1, 5, 1029, 2048):
        x = rng.standard_normal(n).astype(np.float32)
        want = float((x.astype(np.float64) ** 2).sum())
        assert abs(R.chunk_sumsq(x) - want) <= 1e-13 * want
    x = np.full(2048, 1e25, dtype=np.float32)   # the fp32 square overflows, the fp64 sum stays finite
    assert np.isfinite(R.chunk_sumsq(x))
    x[2047] = np.nan
    assert np.isnan(R.chunk_sumsq(x))
    assert R.fold_partials([1.0] * 600) == 600.0
    ref = R.AccumRef(1, [5], max_grad_norm=1.0)
    g = np.array([3.0, 0.0, 4.0, 0.0, 0.0], dtype=np.float32)
    c = ref.micro_step([g])
    assert (c["apply"], c["micro"], c["sched_step"]) == (1, 0, 1)
    assert c["grad_norm"] == np.float32(5.0) and c["clip_coef"] == np.float32(1.0) / (np.float32(5.0) + np.float32(1e-6))


def test_symbols_are_exported_bound_declared_and_modelled(built):
    from spectre_vit import _native, timing
    lib = _native.load()
    src = open(os.path.join(ROOT, "include", "spv.h")).read()
    for name in ("spv_grad_accumulate", "spv_step_control_accum"):
        assert hasattr(lib, name) and name in _native.SIGNATURES and f"int {name}(" in src, name
        assert getattr(lib, name).argtypes == _native.SIGNATURES[name]
        assert name in timing._WORK_MODELS, "bench.py's roofline pass brackets every launch it sees"
        assert name in _native._LAUNCHERS
    S = _native.SIGNATURES
    # spv_grad_sumsq's arguments with the accumulator table behind the table and the control block in front of the partials
    assert S["spv_grad_accumulate"] == [_native.c_vp] * 5 + [_native.c_i] + [_native.c_vp] * 3
    # spv_step_control's arguments, then accumulate_steps, then the stream
    assert S["spv_step_control_accum"] == S["spv_step_control"][:-1] + [_native.c_i, _native.c_vp]
    assert len(S["spv_step_control"]) == 11 and len(S["spv_grad_sumsq"]) == 7   # the old entry points keep their signatures
    # the accumulate launch: the gradient read, the accumulator read and written, per 2048-element chunk
    assert timing._WORK_MODELS["spv_grad_accumulate"]((10, 0, 0))[4] == 3 * timing._WORK_MODELS["spv_grad_sumsq"]((10, 0, 0))[4]
    assert timing._WORK_MODELS["spv_step_control_accum"]((10, 2, 7, 0, 8, 4, 0, 0))[4] == timing._WORK_MODELS["spv_step_control"]((10, 2, 7, 0, 8, 0, 0))[4]
    # micro takes the first reserved word: the block stays 64 bytes and every older field keeps its offset
    from spectre_vit import optim
    assert struct.calcsize(optim._CTL_FMT) == 64
    packed = struct.pack(optim._CTL_FMT, 0.5, 0.25, 2.0, 1, 3.0, 7, 2, 5)
    assert struct.unpack("<ddfifii28x", packed[:36] + bytes(28)) == (0.5, 0.25, 2.0, 1, 3.0, 7, 2)
    assert struct.unpack_from("<i", packed, 36) == (5,) and packed[40:] == bytes(24)
    assert "int micro;" in src and "int reserved[6];" in src


def test_c_abi_rejects_bad_accumulation_arguments_before_any_launch(built):
    """every call fails validation on the host (non-zero return, spv_last_error text, RuntimeError from the ctypes wrapper)"""
    from spectre_vit import _native
    P = 16   # any non-null "pointer": validation fails before it would be used
    SCHEDULE, CLIP = 1, 2
    cases = [
        ("spv_grad_accumulate", (0, P, P, P, P, 1, P, P, 0), "null table"),
        ("spv_grad_accumulate", (P, P, P, P, 0, 1, P, P, 0), "null table"),
        ("spv_grad_accumulate", (P, 0, P, P, P, 1, P, P, 0), "null acc_table"),
        ("spv_grad_accumulate", (P, P, P, P, P, 1, 0, P, 0), "null control block"),
        ("spv_grad_accumulate", (P, P, P, P, P, 1, P, 0, 0), "null partials"),
        ("spv_grad_accumulate", (P, P, P, P, P, -1, P, P, 0), "nchunks"),
        ("spv_step_control_accum", (P, -1, P, 1, P, 0, 0, 0, 0.0, 0.0, 2, 0), "npartials"),
        ("spv_step_control_accum", (P, 1, P, 1, 0, 0, 0, 0, 0.0, 0.0, 2, 0), "null control block"),
        ("spv_step_control_accum", (0, 1, P, 1, P, 0, 0, 0, 0.0, 0.0, 2, 0), "null partials"),
        ("spv_step_control_accum", (P, 1, 0, 1, P, 0, 0, 0, 0.0, 0.0, 2, 0), "step_ptrs"),
        ("spv_step_control_accum", (P, 1, P, 1, P, 0, 0, 0, 0.0, 0.0, 0, 0), "accumulate_steps"),
        ("spv_step_control_accum", (P, 1, P, 1, P, 0, 0, 0, 0.0, 0.0, -3, 0), "accumulate_steps"),
        ("spv_step_control_accum", (P, 1, P, 1, P, SCHEDULE, 3, 3, 0.0, 0.0, 2, 0), "total_steps"),
        ("spv_step_control_accum", (P, 1, P, 1, P, SCHEDULE, 0, 8, -1e-6, 0.0, 2, 0), "eta_min"),
        ("spv_step_control_accum", (P, 1, P, 1, P, CLIP, 0, 0, 0.0, 0.0, 2, 0), "max_norm"),
        ("spv_step_control_accum", (P, 1, P, 1, P, 8, 0, 0, 0.0, 0.0, 2, 0), "flags"),
    ]
    lib = _native.load()
    for name, args, needle in cases:
        assert getattr(lib, name)(*args) != 0, (name, args)
        assert needle in lib.spv_last_error().decode(), (name, needle, lib.spv_last_error().decode())
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, needle, str(e.value))


def test_constructor_refusals():
    from spectre_vit.optim import FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(4))]
    for bad in (True, False, 0, -1, 2.0, "2", 1.5):
        with pytest.raises(ValueError, match="accumulate_steps"):
            FusedAdamW(p, capturable=True, accumulate_steps=bad)
    with pytest.raises(ValueError, match="capturable"):
        FusedAdamW(p, capturable=False, accumulate_steps=2)
    for k in (1, 2, 7):
        o = FusedAdamW(p, capturable=True, accumulate_steps=k)
        assert o.accumulate_steps == k and o.step_control   # the option alone turns the control path on
        assert (o.micro_step(), o.schedule_step(), o.skipped_steps()) == (0, 0, 0)
    off = FusedAdamW(p, capturable=True, max_grad_norm=1.0)
    for reader in (off.micro_step, off.accumulated_grads):
        with pytest.raises(RuntimeError, match="accumulate_steps"):
            reader()


def test_optimizer_without_the_option_is_untouched():
    """the constructor keys, the state_dict and the control block a fresh optimizer starts from"""
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(4))]
    o = FusedAdamW(p, capturable=True)
    assert o.accumulate_steps is None and not o.step_control
    assert set(o.state_dict().keys()) == {"state", "param_groups"}
    assert set(o.param_groups[0].keys()) == {"params", "lr", "betas", "eps", "weight_decay", "capturable"}
    c = FusedAdamW(p, capturable=True, schedule=CosineSchedule(8, 3), skip_nonfinite=True)
    # (a, b, clip_coef, apply, grad_norm, sched_step, skipped) and 28 zero bytes: the layout before the micro count took a word
    assert c.control_block_bytes() == struct.pack("<ddfifii28x", 1.0, 0.0, 1.0, 1, 0.0, 0, 0)
    assert c.state_dict()["step_control"] == dict(schedule_step=0, skipped_steps=0)
    on = FusedAdamW(p, capturable=True, schedule=CosineSchedule(8, 3), skip_nonfinite=True, accumulate_steps=2)
    assert on.control_block_bytes() == c.control_block_bytes()   # a fresh window: micro = 0
    assert set(on.param_groups[0].keys()) == set(o.param_groups[0].keys())


def test_micro_step_travels_through_state_dict_and_the_window_restarts():
    from spectre_vit.optim import FusedAdamW
    mk = lambda **kw: FusedAdamW([torch.nn.Parameter(torch.zeros(4))], capturable=True, skip_nonfinite=True, **kw)
    o = mk(accumulate_steps=3)
    sd = o.state_dict()
    assert sd["step_control"] == dict(schedule_step=0, skipped_steps=0, micro_step=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # a closed window loads silently
        sd["step_control"] = dict(schedule_step=5, skipped_steps=2, micro_step=0)
        o2 = mk(accumulate_steps=3)
        o2.load_state_dict(sd)
    assert (o2.schedule_step(), o2.skipped_steps(), o2.micro_step()) == (5, 2, 0)
    sd["step_control"]["micro_step"] = 2
    o3 = mk(accumulate_steps=3)
    with pytest.warns(UserWarning, match="window restarts"):
        o3.load_state_dict(sd)
    assert (o3.schedule_step(), o3.skipped_steps(), o3.micro_step()) == (5, 2, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # an optimizer without the option ignores the entry
        o4 = mk()
        o4.load_state_dict(sd)
    assert "micro_step" not in o4.state_dict()["step_control"]


def test_harness_arguments():
    from spectre_vit import harness
    from spectre_vit.optim import CosineSchedule
    a = harness.build_parser().parse_args([])
    assert a.accumulate_steps is None
    a = harness.build_parser().parse_args(["--accumulate-steps", "4", "--lr-schedule", "cosine", "--graph"])
    assert a.accumulate_steps == 4
    # total_steps = (epochs * steps) // k; warm-up counts optimizer steps
    for total, k, want in ((6, 2, 3), (7, 2, 3), (12, 4, 3), (6, 1, 6)):
        kw = harness._step_control_args("cosine", 1, 1e-5, None, False, total, k)
        assert isinstance(kw["schedule"], CosineSchedule) and kw["schedule"].total_steps == want == total // k
        assert kw["schedule"].warmup_steps == 1 and kw["accumulate_steps"] == k
    # the option alone is a control argument; without it the keyword does not appear, and nothing at all means no control path
    assert harness._step_control_args(None, 0, 0.0, None, False, 6, 2) == dict(schedule=None, max_grad_norm=None, skip_nonfinite=False,
                                                                                accumulate_steps=2)
    assert harness._step_control_args("cosine", 0, 0.0, 1.0, True, 6).keys() == {"schedule", "max_grad_norm", "skip_nonfinite"}
    assert harness._step_control_args(None, 0, 0.0, None, False, 6) == {}
    for bad in (True, 0, -2, 2.0, "2"):
        with pytest.raises(ValueError, match="accumulate_steps"):
            harness._step_control_args(None, 0, 0.0, None, False, 6, bad)
    with pytest.raises(ValueError, match="total_steps"):   # fewer loader steps than one window: no optimizer step to schedule
        harness._step_control_args("cosine", 0, 0.0, None, False, 3, 4)
    import inspect
    for fn in (harness.train, harness.train_distill):
        assert inspect.signature(fn).parameters["accumulate_steps"].default is None
