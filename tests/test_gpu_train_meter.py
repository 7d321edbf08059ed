"""GPU checks of the training meter (csrc/spv_head.hip, csrc/spv_distill.hip: spv_cross_entropy_meter_fwd, spv_distill_loss_meter_fwd,
spv_distill_loss_idx_meter_fwd; spectre_vit.meter.TrainMeter; the criteria's meter=; harness.train / train_distill(device_meter=True)).

The meter is bookkeeping next to an unchanged loss, so every comparison here is EQUALITY: loss and lse against the un-metered launch
bit for bit, hit counts against tests/meter_ref.py exactly, a log row's loss against the returned loss bit for bit, loss_sum against the
float64 sum of the logged fp32 losses bit for bit.  The one tolerance is the harness's epoch mean: 1 ulp of the float64 division.
Shapes: rows 1 / 16 / 17 / 1025 = one wave of a workgroup, a full workgroup, a second workgroup, one row past 64 workgroups x 16 waves
(the grid-stride loop); classes around the 64-lane walk (63, 64, 65, 129), the training shape (100) and a long row (1000).  Logits sit on
a grid of 0.5, so equal logits -- and with them the tie rules -- occur in every case.  Figures are printed before they are asserted."""
import json
import math
import os

import numpy as np
import pytest
import torch

import meter_ref as R

pytestmark = pytest.mark.gpu

MNIST = "spectre_vit/configs/spectre_vit_mnist.py"
SENTINEL = 0x5A5A5A5A5A5A5A5A


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def ibits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(ibits(a), ibits(b))


def fbits(x):
    from spectre_vit.meter import float_bits
    return float_bits(x)


def grid_logits(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.round(4 * torch.randn(rows, C, generator=g)) / 2          # a grid of 0.5: ties everywhere
    y = torch.randint(0, C, (rows,), generator=g)
    return z, y


_ws = {}


def workspace(entry, d):
    """a zeroed workspace per entry point, as hip_ops keeps them"""
    from spectre_vit import _native
    if entry not in _ws:
        _ws[entry] = torch.zeros((_native.call(entry),), dtype=torch.float32, device=d)
    return _ws[entry]


def ce_launch(z, y, block=None, k=5):
    """the C-ABI itself: -> (loss, lse).  block: the meter's int64 words (None: the un-metered entry point)"""
    from spectre_vit import _native
    from spectre_vit.hip_ops import _p, _stream
    rows, C = z.shape
    lse = torch.empty(rows, dtype=torch.float32, device=z.device)
    loss = torch.empty((), dtype=torch.float32, device=z.device)
    if block is None:
        _native.call("spv_cross_entropy_fwd", _p(z), _p(y), _p(lse), _p(loss), _p(workspace("spv_cross_entropy_workspace_floats", z.device)), rows, C,
                     _stream())
    else:
        _native.call("spv_cross_entropy_meter_fwd", _p(z), _p(y), _p(lse), _p(loss), _p(workspace("spv_cross_entropy_meter_workspace_floats", z.device)),
                     rows, C, _p(block), k, _stream())
    return loss, lse


def distill_launch(z, t, y, index=None, block=None, k=5, consts=(2.0, 0.25, 0.75)):
    """-> (out3, lse3); index: t is the cache"""
    from spectre_vit import _native
    from spectre_vit.hip_ops import _p, _stream
    rows, C = z.shape
    lse = torch.empty((3, rows), dtype=torch.float32, device=z.device)
    out = torch.empty(3, dtype=torch.float32, device=z.device)
    name = "spv_distill_loss" + ("_idx" if index is not None else "") + ("_meter" if block is not None else "") + "_fwd"
    ws = workspace("spv_distill_loss_meter_workspace_floats" if block is not None else "spv_distill_loss_workspace_floats", z.device)
    args = [_p(z), _p(t)] + ([_p(index)] if index is not None else []) + [_p(y), _p(lse), _p(out), _p(ws), rows]
    args += ([t.shape[0]] if index is not None else []) + [C, *consts] + ([_p(block), k] if block is not None else []) + [_stream()]
    _native.call(name, *args)
    return out, lse


def check_read(got, want, what):
    print(f"{what}: meter {dict((k, v) for k, v in got.items() if k != 'rows')}")
    for key in ("steps", "dropped", "seen", "top1", "topk"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert len(got["rows"]) == len(want["rows"]), what
    for i, (g, w) in enumerate(zip(got["rows"], want["rows"])):
        assert g[3:] == w[3:], (what, "row", i, g, w)
        assert [fbits(v) for v in g[:3]] == [fbits(v) for v in w[:3]], (what, "row", i, g, w)
    for key in ("loss_sum", "soft_sum", "ce_sum"):   # bit for bit; a NaN sum is a NaN sum
        assert np.float64(got[key]).view(np.int64) == np.float64(want[key]).view(np.int64) or (math.isnan(got[key]) and math.isnan(want[key])), \
            (what, key, got[key], want[key])


# ---------------------------------------------------------------- the shape sweep
@pytest.mark.parametrize("classes", [1, 2, 63, 64, 65, 100, 129, 1000])
@pytest.mark.parametrize("rows", [1, 16, 17, 1025])
def test_metered_cross_entropy_keeps_the_bits_and_counts_what_the_reference_counts(rows, classes):
    from spectre_vit.meter import TrainMeter
    d = dev()
    batches = [grid_logits(rows, classes, 7 * rows + classes + s) for s in range(2)]
    for k in (1, 5, 8):
        meter = TrainMeter(4, topk=k, device=d)
        ref = R.Meter(4, k)
        for z, y in batches:
            zd, yd = z.to(d), y.to(d)
            loss0, lse0 = ce_launch(zd, yd)
            loss1, lse1 = ce_launch(zd, yd, meter.tensor(), k)
            assert same_bits(loss0, loss1) and same_bits(lse0, lse1), "loss and lse: the un-metered launch's bits"
            if k == 1:   # a figure, not a check: tests/test_gpu_ops.py holds the loss itself to the oracle
                print(f"rows {rows} classes {classes}: loss {loss1.item()!r}, float64 restatement {float(R.step_loss(z.numpy(), y.numpy()))!r}")
            ref.step(z.numpy(), y.numpy(), loss=loss1.item())
        got = meter.read()
        check_read(got, ref.read(), f"rows {rows} classes {classes} k {k}")
        assert got["steps"] == 2 and got["seen"] == 2 * rows and got["soft_sum"] == 0.0 and got["ce_sum"] == 0.0
        assert np.float64(got["loss_sum"]) == np.float64(np.float32(got["rows"][0][0])) + np.float64(np.float32(got["rows"][1][0]))
        if k == 1:   # rows without NaN: the first maximum is torch.argmax
            t1 = sum(int((torch.argmax(z, dim=1) == y).sum()) for z, y in batches)
            assert got["top1"] == got["topk"] == t1


# ---------------------------------------------------------------- ties, NaN rows, labels outside the classes
def test_tie_nan_and_label_rules():
    from spectre_vit.meter import TrainMeter
    d = dev()
    nan = float("nan")
    z = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0, -1.0, 2.0, 0.5, 0.0],     # three tied maxima
                      [2.0] * 9,                                            # all equal
                      [nan] * 9,                                            # no ordered maximum
                      [0.0, nan, 5.0, 1.0, 5.0, -2.0, 0.0, 0.0, 0.0],       # a NaN entry never wins; the first 5.0 does
                      [-1.0, -1.0, -1.0, 0.0, -1.0, -1.0, -1.0, -1.0, 0.0]])
    C = z.shape[1]
    cases = {
        "label = first of the tied maxima": [1, 0, 0, 2, 3],
        "label = second / third of the tied": [2, 5, 3, 4, 8],
        "label on the NaN entry": [4, 8, 8, 1, 0],
    }
    for what, labels in cases.items():
        y = torch.tensor(labels)
        for k in (1, 2, 5):
            meter = TrainMeter(2, topk=k, device=d)
            loss, _ = ce_launch(z.to(d), y.to(d), meter.tensor(), k)
            ref = R.Meter(2, k)
            ref.step(z.numpy(), y.numpy(), loss=loss.item())
            check_read(meter.read(), ref.read(), f"{what}, k {k}")
            assert meter.read()["seen"] == 5 and math.isnan(meter.read()["rows"][0][0]), "the NaN row poisons the step's loss; it is still counted"
    # hand-checked: k = 1 on the first case counts rows 0, 1, 3, 4 and the all-NaN row with label 0
    meter = TrainMeter(1, topk=1, device=d)
    ce_launch(z.to(d), torch.tensor(cases["label = first of the tied maxima"]).to(d), meter.tensor(), 1)
    assert (meter.read()["top1"], meter.read()["topk"]) == (5, 5)
    # labels outside [0, C): not counted, the step's loss NaN, the step logged and in loss_sum
    fin = z[[0, 1, 4]]
    for bad in (-1, -100, C):
        y = torch.tensor([1, bad, 3])
        meter = TrainMeter(2, topk=5, device=d)
        loss0, lse0 = ce_launch(fin.to(d), y.to(d))
        loss1, lse1 = ce_launch(fin.to(d), y.to(d), meter.tensor(), 5)
        got = meter.read()
        print(f"label {bad}: loss {loss1.item()} meter {got}")
        assert same_bits(loss0, loss1) and same_bits(lse0, lse1) and math.isnan(loss1.item())
        assert (got["steps"], got["seen"], got["top1"], got["topk"]) == (1, 2, 2, 2)
        assert len(got["rows"]) == 1 and math.isnan(got["rows"][0][0]) and got["rows"][0][3:] == (2, 2) and math.isnan(got["loss_sum"])
        assert R.hits(fin.numpy(), y.numpy(), 5) == (2, 2, 2)


# ---------------------------------------------------------------- a full log
def test_a_full_log_drops_rows_keeps_totals_and_writes_nothing_past_the_block():
    from spectre_vit import _native
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.meter import CAPACITY, HEADER_WORDS, TrainMeter
    d = dev()
    cap, k, guard = 3, 5, 64
    words = _native.call("spv_train_meter_words", cap)
    buf = torch.full((words + guard,), SENTINEL, dtype=torch.int64, device=d)   # the block, then a guard region
    buf[:words] = 0
    buf[CAPACITY] = cap
    ref = R.Meter(cap, k)
    for s in range(5):
        z, y = grid_logits(17, 100, 50 + s)
        loss, _ = ce_launch(z.to(d), y.to(d), buf[:words], k)
        ref.step(z.numpy(), y.numpy(), loss=loss.item())
    from spectre_vit.meter import decode
    host = buf.cpu().numpy()
    got = decode(host[:words])
    check_read(got, ref.read(), "capacity 3, 5 steps")
    assert (got["steps"], got["dropped"], len(got["rows"]), got["seen"]) == (5, 2, 3, 5 * 17)
    assert int(host[0]) == cap and int(host[CAPACITY]) == cap, "the cursor stops at the capacity"
    assert (host[words:] == SENTINEL).all(), "the guard region behind the block is untouched"
    assert (host[9:HEADER_WORDS] == 0).all(), "the reserved header words stay zero"
    # the same through the Python surface, and reset()
    meter = TrainMeter(cap, topk=k, device=d)
    crit = CrossEntropyLoss(meter=meter)
    ptr = meter.tensor().data_ptr()
    for s in range(5):
        z, y = grid_logits(17, 100, 50 + s)
        crit(z.to(d), y.to(d))
    check_read(meter.read(), ref.read(), "CrossEntropyLoss(meter=), capacity 3, 5 steps")
    meter.reset()
    blank = meter.tensor().cpu().numpy()
    assert blank[CAPACITY] == cap and np.delete(blank, CAPACITY).any() == False and meter.tensor().data_ptr() == ptr   # noqa: E712
    assert meter.read()["steps"] == 0 and meter.read()["rows"] == []
    z, y = grid_logits(17, 100, 50)
    crit(z.to(d), y.to(d))
    assert meter.read()["steps"] == 1 and meter.read()["rows"][0] == ref.read()["rows"][0], "the log starts over at row 0"


# ---------------------------------------------------------------- the distillation forwards
@pytest.mark.parametrize("classes", [2, 100])
@pytest.mark.parametrize("rows", [1, 17])
@pytest.mark.parametrize("cached", [False, True], ids=["teacher", "cache+index"])
def test_metered_distillation_forwards(rows, classes, cached):
    from spectre_vit.distillation import DistillationLoss
    from spectre_vit.meter import TrainMeter
    d = dev()
    k, n_cache = 5, 40
    g = torch.Generator().manual_seed(31 * rows + classes)
    meter = TrainMeter(2, topk=k, device=d)    # 3 steps into 2 rows: the full-log rule on this path too
    plain, metered = DistillationLoss(), DistillationLoss(meter=meter)
    ref = R.Meter(2, k)
    cache = (2 * torch.randn(n_cache, classes, generator=g)).to(d)
    for s in range(3):
        z, y = grid_logits(rows, classes, 900 + 10 * rows + classes + s)
        index = torch.randperm(n_cache, generator=g)[:rows].to(d)       # permuted rows of the cache
        t = cache if cached else cache[index].contiguous()
        idx = index if cached else None
        zd, yd = z.to(d), y.to(d)
        out0, lse0 = distill_launch(zd, t, yd, idx)
        out1, lse1 = distill_launch(zd, t, yd, idx, meter.tensor(), k)
        assert same_bits(out0, out1) and same_bits(lse0, lse1), "out3 and lse3: the un-metered launch's bits"
        ref.step(z.numpy(), y.numpy(), loss=out1[0].item(), soft=out1[1].item(), ce=out1[2].item())
        # the criterion: the same launch through the Python surface; its .soft / .ce are the row's
        zr = zd.clone().requires_grad_(True)
        la = plain(zd, t, yd, index=idx) if cached else plain(zd, t, yd)
        lb = metered(zr, t, yd, index=idx) if cached else metered(zr, t, yd)
        assert same_bits(la, lb.detach()) and same_bits(plain.soft, metered.soft) and same_bits(plain.ce, metered.ce)
        assert same_bits(lb.detach(), out1[0]) and same_bits(metered.soft, out1[1]) and same_bits(metered.ce, out1[2])
        ref.step(z.numpy(), y.numpy(), loss=lb.item(), soft=metered.soft.item(), ce=metered.ce.item())
        if s == 0:   # the backward is the un-metered one
            lb.backward()
            z0 = zd.clone().requires_grad_(True)
            (plain(z0, t, yd, index=idx) if cached else plain(z0, t, yd)).backward()
            assert same_bits(zr.grad, z0.grad)
    got = meter.read()
    check_read(got, ref.read(), f"rows {rows} classes {classes} cached {cached}")
    assert (got["steps"], got["dropped"], len(got["rows"]), got["seen"]) == (6, 4, 2, 6 * rows)
    assert got["rows"][0][1] != 0.0 and got["rows"][0][2] != 0.0 and got["soft_sum"] != 0.0 and got["ce_sum"] != 0.0


# ---------------------------------------------------------------- graph replay
def test_a_captured_launch_logs_a_new_row_at_every_replay():
    from spectre_vit import hip_ops
    from spectre_vit.meter import TrainMeter
    d = dev()
    rows, C, k = 17, 100, 5
    batches = [grid_logits(rows, C, 300 + s) for s in range(4)]
    meter = TrainMeter(8, topk=k, device=d)
    eager = []
    for z, y in batches:   # eager results first (this also builds the workspace outside the capture)
        loss = hip_ops.cross_entropy(z.to(d), y.to(d), meter)
        eager.append(loss.clone())
    want = meter.read()
    meter.reset()
    zs, ys = batches[0][0].to(d).clone(), batches[0][1].to(d).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = hip_ops.cross_entropy(zs, ys, meter)
    assert meter.read()["steps"] == 0, "a capture launches nothing"
    for s, (z, y) in enumerate(batches):
        zs.copy_(z)
        ys.copy_(y)
        graph.replay()
        assert same_bits(loss, eager[s]), f"replay {s}: the eager loss"
    got = meter.read()
    check_read(got, want, "4 replays against 4 eager launches")
    assert got["steps"] == 4 and int(meter.tensor()[0].item()) == 4
    assert len({fbits(r[0]) for r in got["rows"]}) == 4, "four distinct rows"


# ---------------------------------------------------------------- the graphed training step
def test_graphed_train_step_logs_itself():
    from spectre_vit import harness
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.meter import TrainMeter
    from spectre_vit.optim import FusedAdamW
    d = dev()
    c = parse_config(MNIST)
    torch.manual_seed(11)
    model = harness.build_model(c, "fft", d).train()
    g = torch.Generator().manual_seed(5)
    imgs = [torch.randn(16, c.in_channels, c.img_size, c.img_size, generator=g).to(d) for _ in range(4)]
    labels = [torch.randint(0, c.num_classes, (16,), generator=g).to(d) for _ in range(4)]
    meter = TrainMeter(8, topk=5, device=d)
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True)
    step = GraphedTrainStep(model, opt, CrossEntropyLoss(meter=meter), imgs[0], labels[0], autocast_dtype=torch.bfloat16, warmup=1)
    try:
        for s in range(4):
            if s == 0:
                loss, out = step.warm_loss, step.warm_out   # the warm-up step WAS step 0
            else:
                loss, out = step(imgs[s], labels[s]), step.out
            got = meter.read()
            row = got["rows"][-1]
            top1 = int((torch.argmax(out.float(), dim=1) == labels[s]).sum())
            print(f"step {s}: loss {loss.item()!r} row {row} host top1 {top1}")
            assert got["steps"] == s + 1 == len(got["rows"]), "one row per step: the warm-up step, then one per replay"
            assert row[3] == top1 and fbits(row[0]) == fbits(loss.item()) and row[3] <= row[4] <= 16
        assert step.replays == 3 and meter.read()["seen"] == 4 * 16
    finally:
        step.close()


# ---------------------------------------------------------------- the harness
EPOCH_KEYS = {"epoch", "Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation", "steps", "val_samples"}


def _run(tmp_path, tag, fn, monkeypatch=None, **kw):
    from spectre_vit import meter as M
    reads, labels = [], []
    if monkeypatch is not None:
        real = M.TrainMeter.read
        monkeypatch.setattr(M.TrainMeter, "read", lambda self: reads.append(real(self)) or reads[-1])
    out = str(tmp_path / tag)
    hook = lambda kind, step, img, label: labels.append(label.detach().cpu()) if kind == "train" else None
    _, hist = fn(MNIST, mixer="fft", out_dir=out, log=lambda r: None, batch_hook=hook, epochs=2, steps_per_epoch=3, batch_size=16, n_train=64,
                 n_val=32, graph=True, **kw)
    lines = [json.loads(l) for l in open(os.path.join(out, "scalars.jsonl"))]
    return dict(hist=hist, lines=lines, reads=reads, labels=labels)


def _check_metered_run(on, off, batch_keys):
    assert len(on["reads"]) == 2 and len(on["labels"]) == 6, "one read per epoch"
    per_step = [l for l in on["lines"] if "step" in l]
    assert [l["step"] for l in per_step] == list(range(6)) and all(set(l) == batch_keys for l in per_step)
    for e, (rec, host) in enumerate(zip(on["hist"], off["hist"])):
        m = on["reads"][e]
        seen = sum(int(l.numel()) for l in on["labels"][3 * e:3 * e + 3])
        assert (m["steps"], m["dropped"], len(m["rows"]), m["seen"]) == (3, 0, 3, seen), "warm-up = the first batch's one row"
        print(f"epoch {e + 1}: metered {rec}  host-accounted {host}")
        # accuracy: exact, against the meter's own rows and against the host-accounted run of the same (deterministic) training
        assert rec["Accuracy/Train"] == sum(r[3] for r in m["rows"]) / seen == host["Accuracy/Train"]
        assert rec["Accuracy/TrainTop5"] == sum(r[4] for r in m["rows"]) / seen >= rec["Accuracy/Train"]
        # loss: the float64 mean of the logged per-step losses, to 1 ulp of the float64 division
        logged = [l["Batch Loss/Train"] for l in per_step[3 * e:3 * e + 3]]
        assert [fbits(v) for v in logged] == [fbits(r[0]) for r in m["rows"]]
        acc = np.float64(0.0)
        for v in logged:
            acc = acc + np.float64(v)
        want = float(acc) / 3
        assert abs(rec["Loss/Train"] - want) <= math.ulp(want), (rec["Loss/Train"], want)
        # the host-accounted run keeps an fp32 running sum (train) or the same float64 sum (train_distill): two fp32 adds and a divide,
        # each within 2^-24 relative, of losses of one sign
        assert abs(rec["Loss/Train"] - host["Loss/Train"]) <= 4 * 2.0 ** -24 * abs(want), (rec["Loss/Train"], host["Loss/Train"])
        assert set(rec) == EPOCH_KEYS | {"Accuracy/TrainTop5"} and set(host) == EPOCH_KEYS
        for key in ("Loss/Validation", "Accuracy/Validation", "steps", "val_samples"):
            assert rec[key] == host[key], key   # the training itself is untouched: the same weights reach validation


def test_harness_train_with_the_device_meter(tmp_path, monkeypatch):
    from spectre_vit.harness import train
    off = _run(tmp_path, "off", train)
    assert [set(l) for l in off["lines"]] == [EPOCH_KEYS, EPOCH_KEYS, {"Training time"}], "device_meter=False: the record as it was"
    on = _run(tmp_path, "on", train, monkeypatch, device_meter=True)
    _check_metered_run(on, off, {"step", "Batch Loss/Train"})


def test_harness_train_distill_with_the_device_meter(tmp_path, monkeypatch):
    from spectre_vit.harness import train_distill
    batch_keys = {"step", "Batch Loss/Train", "Batch Loss/Dist", "Batch Loss/CE"}
    off = _run(tmp_path, "off", train_distill, cache_teacher=True)
    kinds = [set(l) for l in off["lines"]]
    assert kinds == [{"TeacherCache"}] + ([batch_keys] * 3 + [EPOCH_KEYS]) * 2 + [{"Training time"}], "device_meter=False: the record as it was"
    on = _run(tmp_path, "on", train_distill, monkeypatch, cache_teacher=True, device_meter=True)
    assert [set(l) for l in on["lines"]] == [{"TeacherCache"}] + ([batch_keys] * 3 + [EPOCH_KEYS | {"Accuracy/TrainTop5"}]) * 2 + [{"Training time"}]
    _check_metered_run(on, off, batch_keys)
    # the three per-batch scalars are the un-metered run's, bit for bit, and the rows' soft / ce
    strip = lambda run: [(l["step"], fbits(l["Batch Loss/Train"]), fbits(l["Batch Loss/Dist"]), fbits(l["Batch Loss/CE"])) for l in run["lines"] if "step" in l]
    assert strip(on) == strip(off)
    rows = [r for m in on["reads"] for r in m["rows"]]
    assert [(fbits(r[0]), fbits(r[1]), fbits(r[2])) for r in rows] == [s[1:] for s in strip(on)]
    for e, rec in enumerate(on["hist"]):
        assert rec["Loss/Train"] == off["hist"][e]["Loss/Train"], "the same float64 adds in the same order"
