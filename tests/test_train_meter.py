"""The training meter, host side (no GPU): the new symbols and their declarations, the C-ABI's refusals before any launch, the Python
surface's refusals before a device is touched, the block decoder, and the float64 restatement (tests/meter_ref.py) against torch's own
cross_entropy / argmax / topk and against the tie, NaN-row and out-of-range-label rules."""
import inspect
import os

import numpy as np
import pytest
import torch

import meter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METERED = ("spv_cross_entropy_meter_fwd", "spv_distill_loss_meter_fwd", "spv_distill_loss_idx_meter_fwd")
SIZES = ("spv_train_meter_words", "spv_cross_entropy_meter_workspace_floats", "spv_distill_loss_meter_workspace_floats")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_symbols_are_exported_bound_declared_and_modelled(built):
    from spectre_vit import _native, timing
    lib = _native.load()
    src = open(os.path.join(ROOT, "include", "spv.h")).read()
    for name in METERED:
        assert hasattr(lib, name) and name in _native.SIGNATURES and f"int {name}(" in src
        assert name in timing._WORK_MODELS, "bench.py's roofline pass brackets every launch it sees"
        assert name in _native._LAUNCHERS
    for name in SIZES:
        assert hasattr(lib, name) and name in _native.SIGNATURES and f"int64_t {name}(" in src and name in _native._NO_STATUS
    # the arguments of the un-metered entry point, then meter, k, then the stream
    S = _native.SIGNATURES
    for name in METERED:
        base = S[name.replace("_meter", "")]
        assert S[name] == base[:-1] + [_native.c_vp, _native.c_i, _native.c_vp], name
    assert lib.spv_version() == 1
    # the un-metered symbols keep their signatures
    assert len(S["spv_cross_entropy_fwd"]) == 8 and len(S["spv_distill_loss_fwd"]) == 12 and len(S["spv_distill_loss_idx_fwd"]) == 14
    # the work models take the launch's integer arguments as _native.call hands them over (+ the null mask and the hint)
    assert timing._WORK_MODELS["spv_cross_entropy_meter_fwd"]((512, 100, 5, 0, 0))[4] == timing._WORK_MODELS["spv_cross_entropy_fwd"]((512, 100, 0, 0))[4]
    assert timing._WORK_MODELS["spv_distill_loss_idx_meter_fwd"]((512, 4096, 100, 5, 0, 0))[1] == (512, 100)


def test_block_and_workspace_sizes(built):
    from spectre_vit import _native, meter
    lib = _native.load()
    for cap in (1, 3, 98, 1 << 24):
        assert _native.call("spv_train_meter_words", cap) == meter.HEADER_WORDS + meter.ROW_WORDS * cap
    for bad in (0, -1, (1 << 24) + 1):
        assert _native.call("spv_train_meter_words", bad) == 0
        assert "capacity" in lib.spv_last_error().decode()
    # the un-metered workspace in front, three hit counts per workgroup behind it
    assert _native.call("spv_cross_entropy_meter_workspace_floats") >= _native.call("spv_cross_entropy_workspace_floats") + 3 * 64
    assert _native.call("spv_distill_loss_meter_workspace_floats") >= _native.call("spv_distill_loss_workspace_floats") + 3 * 64
    src = open(os.path.join(ROOT, "include", "spv.h")).read()
    assert f"#define SPV_TRAIN_METER_HEADER {meter.HEADER_WORDS}" in src and f"#define SPV_TRAIN_METER_ROW {meter.ROW_WORDS}" in src


def test_c_abi_refuses_bad_meter_arguments_before_any_launch(built):
    from spectre_vit import _native
    P = 16   # any non-null, 8-byte aligned "pointer": validation fails before it would be used
    ce = lambda **kw: (P, P, P, P, P, kw.get("rows", 4), kw.get("classes", 10), kw.get("meter", P), kw.get("k", 5), 0)
    dl = lambda **kw: (P, P, P, P, P, P, kw.get("rows", 4), kw.get("classes", 10), kw.get("T", 2.0), 0.25, 0.75, kw.get("meter", P), kw.get("k", 5), 0)
    di = lambda **kw: (P, P, kw.get("index", P), P, P, P, P, kw.get("rows", 4), kw.get("n_cache", 8), kw.get("classes", 10), kw.get("T", 2.0), 0.25,
                       0.75, kw.get("meter", P), kw.get("k", 5), 0)
    cases = []
    for name, mk in zip(METERED, (ce, dl, di)):
        cases += [(name, mk(meter=0), "meter missing"), (name, mk(meter=12), "8-byte aligned"), (name, mk(k=0), "k=0"), (name, mk(k=9), "k=9"),
                  (name, mk(k=-1), "k=-1"), (name, mk(rows=(1 << 24) + 1), "rows="), (name, mk(classes=1 << 24), "classes=")]
    cases += [(METERED[0], ce(rows=0), "rows=0"), (METERED[0], ce(classes=0), "classes=0"),
              (METERED[1], dl(rows=0), "empty"), (METERED[1], dl(T=0.0), "temperature"),
              (METERED[2], di(rows=0), "empty"), (METERED[2], di(index=0), "index missing"), (METERED[2], di(n_cache=0), "empty cache")]
    lib = _native.load()
    for name, args, needle in cases:
        assert getattr(lib, name)(*args) != 0, (name, args)
        assert needle in lib.spv_last_error().decode(), (name, needle, lib.spv_last_error().decode())
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, needle, str(e.value))


def test_train_meter_refuses_bad_arguments_before_a_device_is_touched():
    from spectre_vit.meter import TrainMeter
    for bad in (0, -3, 1.5, None, True, "8", (1 << 24) + 1):
        with pytest.raises(ValueError, match="capacity"):
            TrainMeter(bad)
    for bad in (0, 9, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="topk"):
            TrainMeter(4, topk=bad)
    with pytest.raises(ValueError, match="GPU"):
        TrainMeter(4, device="cpu")
    sig = inspect.signature(TrainMeter.__init__)
    assert sig.parameters["topk"].default == 5
    for name in ("reset", "read", "tensor"):
        assert callable(getattr(TrainMeter, name))


def test_criteria_take_a_meter_or_none_and_nothing_else():
    from spectre_vit.distillation import DistillationLoss
    from spectre_vit.loss import CrossEntropyLoss
    assert CrossEntropyLoss().meter is None and DistillationLoss().meter is None
    assert inspect.signature(CrossEntropyLoss.__init__).parameters["meter"].default is None
    assert inspect.signature(DistillationLoss.__init__).parameters["meter"].default is None
    for bad in (5, "meter", torch.zeros(21, dtype=torch.int64), object()):
        with pytest.raises(TypeError, match="TrainMeter"):
            CrossEntropyLoss(meter=bad)
        with pytest.raises(TypeError, match="TrainMeter"):
            DistillationLoss(meter=bad)
    # the options nn.CrossEntropyLoss has and the reference never sets stay refused, meter or not
    for kw in (dict(label_smoothing=0.1), dict(reduction="sum"), dict(weight=torch.ones(3))):
        with pytest.raises(NotImplementedError):
            CrossEntropyLoss(**kw)
    with pytest.raises(RuntimeError, match="GPU"):
        CrossEntropyLoss()(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def test_harness_refusals_and_the_flag():
    from spectre_vit import harness
    cfg = "spectre_vit/configs/spectre_vit_mnist.py"
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="device_meter"):
            harness.train(cfg, device_meter=bad)
        with pytest.raises(ValueError, match="device_meter"):
            harness.train_distill(cfg, device_meter=bad)
    with pytest.raises(ValueError, match="device_meter"):
        harness.train(cfg, device_meter=True, distill=True)
    assert inspect.signature(harness.train).parameters["device_meter"].default is False
    assert inspect.signature(harness.train_distill).parameters["device_meter"].default is False
    p = harness.build_parser()
    assert p.parse_args([]).device_meter is False
    assert p.parse_args(["--device-meter", "--graph"]).device_meter is True
    assert p.parse_args(["--distill-paired", "--cache-teacher", "--graph", "--device-meter"]).device_meter is True


def test_decode_reads_the_block_as_the_header_says():
    from spectre_vit import meter as M
    cap = 4
    w = np.zeros(M.HEADER_WORDS + M.ROW_WORDS * cap, np.int64)
    losses = [np.float32(4.6051702), np.float32(np.nan), np.float32(1e-3)]
    w[M.CURSOR], w[M.CAPACITY], w[M.DROPPED] = 3, cap, 2
    w[M.SEEN], w[M.TOP1], w[M.TOPK] = 40, 7, 19
    w[M.LOSS_SUM:M.CE_SUM + 1] = np.array([12.5, 0.25, -0.0], np.float64).view(np.int64)
    for i, l in enumerate(losses):
        row = w[M.HEADER_WORDS + M.ROW_WORDS * i:][:M.ROW_WORDS]
        row[0] = int(np.array([l]).view(np.uint32)[0])   # fp32 bits in the low half, the high half zero
        row[1] = int(np.array([np.float32(0.5)]).view(np.uint32)[0])
        row[2] = int(np.array([np.float32(-2.0)]).view(np.uint32)[0])   # a set sign bit must not leak into the high half's reading
        row[3], row[4] = i, 10 + i
    w[M.HEADER_WORDS + M.ROW_WORDS * 3:] = -1   # the unwritten row is not reported
    d = M.decode(w)
    assert (d["steps"], d["dropped"], d["seen"], d["top1"], d["topk"]) == (5, 2, 40, 7, 19)
    assert (d["loss_sum"], d["soft_sum"]) == (12.5, 0.25) and d["ce_sum"] == 0.0
    assert d["loss_mean"] == 12.5 / 5 and d["accuracy"] == 7 / 40 and d["accuracy_topk"] == 19 / 40
    assert len(d["rows"]) == 3
    for i, l in enumerate(losses):
        got = d["rows"][i]
        assert (M.float_bits(got[0]) == M.float_bits(float(l))) or (np.isnan(l) and np.isnan(got[0]))
        assert got[1:] == (0.5, -2.0, i, 10 + i)
    empty = M.decode(np.zeros(M.HEADER_WORDS + M.ROW_WORDS, np.int64))
    assert empty["steps"] == 0 and empty["rows"] == [] and empty["loss_mean"] == 0.0 and empty["accuracy"] == 0.0


# ---------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("shape", [(1, 1), (7, 2), (33, 10), (64, 100), (17, 1000)], ids=lambda s: "rows{}-classes{}".format(*s))
def test_ref_agrees_with_torch_on_random_float64_inputs(shape):
    rows, C = shape
    g = torch.Generator().manual_seed(1000 * rows + C)
    z = 3 * torch.randn(rows, C, generator=g, dtype=torch.float64)
    y = torch.randint(0, C, (rows,), generator=g)
    want_loss = torch.nn.functional.cross_entropy(z, y).item()
    got_loss = float(R.step_loss(z.numpy(), y.numpy()))
    print(f"loss torch {want_loss!r} ref (rounded to fp32) {got_loss!r}")
    assert abs(got_loss - want_loss) <= 2.0 ** -23 * abs(want_loss), "one fp32 rounding of the float64 mean"
    assert np.array_equal(R.predictions(z.numpy()), torch.argmax(z, dim=1).numpy())
    for k in (1, 5, 8):
        kk = min(k, C)
        topk = torch.topk(z, kk, dim=1).indices     # random float64: no ties
        want = (int(rows), int((torch.argmax(z, dim=1) == y).sum()), int((topk == y[:, None]).any(dim=1).sum()))
        assert R.hits(z.numpy(), y.numpy(), k) == want, (k, want)


def test_ref_tie_nan_and_label_rules():
    z = np.array([[1.0, 3.0, 3.0, 0.0],      # duplicated maximum: the first one is the prediction
                  [2.0, 2.0, 2.0, 2.0],      # all equal
                  [np.nan] * 4,              # a row without an ordered maximum
                  [0.0, np.nan, 5.0, 1.0]])  # a NaN entry never wins
    assert R.predictions(z).tolist() == [1, 0, 0, 2]
    # label among the tied: the FIRST of the tied maxima is a top-1 hit, the second is not, but it is in the top 2
    assert R.hits(z[:1], [1], 1) == (1, 1, 1) and R.hits(z[:1], [2], 1) == (1, 0, 0) and R.hits(z[:1], [2], 2) == (1, 0, 1)
    # all equal: label c has c entries ranked in front of it
    assert [R.hits(z[1:2], [c], 2)[2] for c in range(4)] == [1, 1, 0, 0]
    assert [R.hits(z[1:2], [c], 1)[1] for c in range(4)] == [1, 0, 0, 0]
    # an all-NaN row with a valid label is counted; nothing compares greater than NaN, so it is a top-k hit, and a top-1 hit for label 0
    assert R.hits(z[2:3], [0], 1) == (1, 1, 1) and R.hits(z[2:3], [3], 1) == (1, 0, 1)
    assert np.isnan(R.step_loss(z[2:3], [0]))
    # labels outside [0, C): not counted, the step's loss NaN, the step still logged and in the totals
    for bad in (-1, -100, 4):
        assert R.hits(z[:2], [1, bad], 5) == (1, 1, 1)
        assert np.isnan(R.step_loss(z[:2], [1, bad]))
    m = R.Meter(2, 5)
    m.step(z[:2], [1, 0])
    m.step(z[:2], [1, -100])
    m.step(z[:2], [2, 3])
    d = m.read()
    assert (d["steps"], d["dropped"], len(d["rows"]), d["seen"], d["top1"]) == (3, 1, 2, 5, 3)
    assert np.isnan(d["rows"][1][0]) and d["rows"][1][3:] == (1, 1) and np.isnan(d["loss_sum"]) and np.isnan(d["loss_mean"])
    assert not np.isnan(d["rows"][0][0]) and d["soft_sum"] == 0.0 and d["ce_sum"] == 0.0


def test_ref_sums_are_float64_sums_of_the_fp32_step_values():
    m = R.Meter(3, 1)
    z = np.zeros((2, 3))
    vals = [np.float32(0.1), np.float32(1e8), np.float32(-1e8), np.float32(0.3), np.float32(7.0)]
    acc = np.float64(0.0)
    for v in vals:
        m.step(z, [0, 1], loss=v, soft=v, ce=np.float32(2) * v)
        acc = acc + np.float64(v)
    d = m.read()
    assert d["loss_sum"] == float(acc) == d["soft_sum"] and d["ce_sum"] == 2 * float(acc)
    assert d["steps"] == 5 and d["dropped"] == 2 and [r[0] for r in d["rows"]] == [float(v) for v in vals[:3]]
    assert d["loss_mean"] == float(acc) / 5 and (d["seen"], d["top1"]) == (10, 5)
    m.reset()
    assert m.read()["steps"] == 0 and m.read()["rows"] == []
