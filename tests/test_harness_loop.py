"""The harness's shared loop (spectre_vit/harness.py: _run_epochs, _TrainBooks, _epoch_tail) driven on the CPU with stand-ins for the
step object, the meter, the optimizer and the validation pass: the epoch record's keys and their order, the lines of scalars.jsonl, who
writes them, where the "train" hook stands, the best-checkpoint rule; and the argument refusals of train() / train_distill(), which come
before any device is touched and in a fixed order."""
import contextlib
import itertools
import json
import os
import time
from types import SimpleNamespace

import pytest
import torch

BASE = ["epoch", "Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation", "steps", "val_samples"]
TRAIN_NAMES = ("Batch Loss/Train",)
DISTILL_NAMES = ("Batch Loss/Train", "Batch Loss/Dist", "Batch Loss/CE")
EPOCH_STEPS = 2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


class FakeMeter:
    """two log rows per epoch, (loss, soft, ce, one more column), as spectre_vit.meter.TrainMeter.read() returns them"""

    def __init__(self):
        self.reads = self.resets = 0

    def read(self):
        self.reads += 1
        rows = [[self.reads + 0.5, 0.25, 0.75, 9.0], [self.reads + 1.5, 0.5, 1.5, 9.0]]
        return {"loss_mean": self.reads + 1.0, "accuracy": 0.5, "accuracy_topk": 0.875, "rows": rows}

    def reset(self):
        self.resets += 1


class FakeOptimizer:
    accumulate_steps = 2

    def __init__(self):
        self.ctl_reads, self.averaged = 0, False

    def _read_ctl(self):
        self.ctl_reads += 1
        return {"grad_norm": 1.5, "skipped": 0, "sched_step": self.ctl_reads}

    def last_lr(self, c):
        return [1e-3]

    @contextlib.contextmanager
    def ema_weights(self):
        self.averaged = True
        yield
        self.averaged = False

    def ema_state_dict(self, model):
        return {"ema": torch.zeros(1)}


def make_run(out, rank=0, meter=False, named=False, control=False, ema=False):
    """the fields of _setup's record that the loop and its tail read"""
    os.makedirs(out, exist_ok=True)
    return SimpleNamespace(rank=rank, device=torch.device("cpu"), model=torch.nn.Linear(2, 2), epoch_steps=EPOCH_STEPS,
                           control=dict(skip_nonfinite=True) if control else {}, ema=dict(ema_decay=0.9) if ema else {},
                           meter=FakeMeter() if meter else None, optimizer_name="sgd" if named else None, optimizer=FakeOptimizer(),
                           out_dir=out, log_f=open(os.path.join(out, "scalars.jsonl"), "a") if rank == 0 else None, global_step=0,
                           history=[], best_acc=0.0, best_ema_acc=0.0, session=SimpleNamespace(closed=0, close=None),
                           start=time.perf_counter())


def make_step(events, terms):
    """three batches a pass (one more than the epoch takes); three of a batch's four predictions hit; the loss of step n is 1 + n"""
    label = torch.tensor([0, 1, 2, 0])
    closed = []

    def batches():
        for k in range(EPOCH_STEPS + 1):
            yield torch.full((4, 2), float(k)), label

    def run_step(batch, n):
        events.append(("run", n))
        extra = (torch.tensor(0.25), torch.tensor(0.75))[:terms]
        return (torch.tensor(1.0 + n, requires_grad=True), torch.eye(3)[[0, 1, 2, 1]], batch[0] + 100, batch[1], *extra)
    return SimpleNamespace(batches=batches, run=run_step, close=lambda: closed.append(1), closed=closed)


def drive(run, names, hook_after, epochs=2, accuracies=None, ema_accuracies=None):
    from spectre_vit import harness
    events, logged, passes = [], [], []
    step = make_step(events, len(names) - 1)
    run.session.close = lambda: setattr(run.session, "closed", run.session.closed + 1)

    def hook(kind, n, img, label):
        events.append((kind, n, float(img[0, 0])))

    def validate(h):
        passes.append((h is hook, run.optimizer.averaged))
        seq = ema_accuracies if run.optimizer.averaged else accuracies
        return (seq[len(run.history)] if seq else 0.5), 2.0, 40
    model, history = harness._run_epochs(run, step, harness._TrainBooks(run, names, block=len(names) > 1), validate, epochs, hook,
                                         hook_after, logged.append)
    assert model is run.model and history is run.history and step.closed == [1] and run.session.closed == 1
    return events, logged, passes


@pytest.mark.parametrize("names", [TRAIN_NAMES, DISTILL_NAMES], ids=["train", "train_distill"])
@pytest.mark.parametrize("meter,named,control,ema", list(itertools.product([False, True], repeat=4)))
def test_record_and_log_lines(tmp_path, names, meter, named, control, ema):
    out = str(tmp_path / "rank0")
    run = make_run(out, 0, meter, named, control, ema)
    events, logged, passes = drive(run, names, hook_after=False)
    want = BASE + ["Accuracy/TrainTop5"] * meter + ["Optimizer"] * named \
        + ["LR", "GradNorm", "SkippedSteps", "AccumulateSteps", "OptimizerSteps"] * control \
        + ["Accuracy/ValidationEMA", "Loss/ValidationEMA"] * ema
    assert len(run.history) == 2 and logged == run.history
    for e, rec in enumerate(run.history):
        assert list(rec) == want, "the record's keys, in order"
        assert (rec["epoch"], rec["steps"], rec["val_samples"]) == (e + 1, EPOCH_STEPS, 40)
        if meter:
            assert (rec["Loss/Train"], rec["Accuracy/Train"], rec["Accuracy/TrainTop5"]) == (e + 2.0, 0.5, 0.875)
        else:   # steps 2e and 2e + 1, losses 1 + n; three hits of four
            assert (rec["Loss/Train"], rec["Accuracy/Train"]) == (1.5 + 2 * e, 0.75)
        if named:
            assert rec["Optimizer"] == "sgd"
        if control:
            assert rec["OptimizerSteps"] == e + 1, "ONE read of the control block per epoch"
    if meter:
        assert (run.meter.reads, run.meter.resets) == (2, 2), "the meter is read once per epoch"
    assert run.optimizer.ctl_reads == (2 if control else 0)
    # validation: the hooked pass on the trained weights, then (averaging) the un-hooked one inside ema_weights()
    assert passes == ([(True, False), (False, True)] if ema else [(True, False)]) * 2
    # scalars.jsonl: per epoch the per-step lines, then the record; "Training time" last
    lines = [json.loads(text) for text in open(os.path.join(out, "scalars.jsonl"))]
    assert list(lines.pop()) == ["Training time"]
    per_step = meter or len(names) > 1   # train() logs steps only with the meter, train_distill() always
    want_lines = []
    for e in range(2):
        for k in range(EPOCH_STEPS if per_step else 0):
            n = 2 * e + k
            terms = [e + 1 + k + 0.5, 0.25 * (k + 1), 0.75 * (k + 1)] if meter else [1.0 + n, 0.25, 0.75]
            want_lines.append(dict(zip(("step",) + names, [n] + terms)))
        want_lines.append(run.history[e])
    assert lines == want_lines
    assert [list(l) for l in lines] == [list(l) for l in want_lines], "the fields' order too"
    assert sorted(os.listdir(out)) == ["model_best.pt"] + ["model_ema_best.pt"] * ema + ["scalars.jsonl"]


@pytest.mark.parametrize("hook_after", [False, True], ids=["host_batches", "loader_batches"])
def test_train_hook_placement_and_step_numbers(tmp_path, hook_after):
    """without a loader the hook sees the batch in front of its step, with one the step's buffers after it; the numbers run on across
    the epoch boundary, and an epoch takes epoch_steps batches of the pass"""
    events, _, _ = drive(make_run(str(tmp_path / "r")), TRAIN_NAMES, hook_after)
    want = []
    for n in range(2 * EPOCH_STEPS):
        k = float(n % EPOCH_STEPS)   # the batch's fill value; the step hands back batch + 100
        want += [("run", n), ("train", n, k + 100)] if hook_after else [("train", n, k), ("run", n)]
    assert events == want


def test_only_rank_zero_writes(tmp_path):
    out = str(tmp_path / "rank1")
    run = make_run(out, rank=1, meter=True, named=True, control=True, ema=True)
    _, logged, passes = drive(run, DISTILL_NAMES, hook_after=True)
    assert os.listdir(out) == [] and logged == [], "no log line, no log(rec), no checkpoint"
    assert len(run.history) == 2 and "Accuracy/ValidationEMA" in run.history[0] and len(passes) == 4, "the record is still made"


def test_best_checkpoint_rule(tmp_path, monkeypatch):
    """saved when the accuracy beats the best so far, or in the first epoch (train.py:288-290); the averaged weights by the same rule"""
    from spectre_vit import harness
    saves = []
    run = make_run(str(tmp_path / "r"), ema=True)
    monkeypatch.setattr(harness.torch, "save", lambda obj, path: saves.append((os.path.basename(path), len(run.history), sorted(obj))))
    drive(run, TRAIN_NAMES, False, epochs=6, accuracies=[0.0, 0.0, 0.3, 0.2, 0.3, 0.4], ema_accuracies=[0.0, 0.1, 0.1, 0.5, 0.4, 0.5])
    assert [(e, keys) for name, e, keys in saves if name == "model_best.pt"] == [(e, ["bias", "weight"]) for e in (1, 3, 6)]
    assert [(e, keys) for name, e, keys in saves if name == "model_ema_best.pt"] == [(e, ["ema"]) for e in (1, 2, 4)]


# ---------------------------------------------------------------- the refusals: before a device, in a fixed order
MNIST = "spectre_vit/configs/spectre_vit_mnist.py"
TRAIN_REFUSALS = [   # in the order train() raises them
    (dict(device_meter=1), "device_meter=1 must be True or False"),
    (dict(device_loader="yes"), "device_loader='yes' must be True or False"),
    (dict(augment=True, uint8_input=True), "augment=True yields normalised float batches"),
    (dict(ema_warmup=True), "ema_warmup=True needs ema_decay"),
    (dict(optimizer="lamb"), "optimizer='lamb'"),
    (dict(model="spectre_branch", uint8_input=True), "the SpectreBranch spectrum takes fp32 images"),
    (dict(graph=True, distill=True), "graph=True replays the plain training step"),
]
DISTILL_REFUSALS = [   # in the order train_distill() raises them; WORLD_SIZE=2 is set for all of them
    (dict(device_meter=1), "device_meter=1 must be True or False"),
    (dict(device_loader="yes"), "device_loader='yes' must be True or False"),
    (dict(ema_warmup=True), "ema_warmup=True needs ema_decay"),
    (dict(optimizer="lamb"), "optimizer='lamb'"),
    (dict(teacher_cache_path="t.pt"), "it needs cache_teacher=True"),
    (dict(graph=True), "graph=True replays the single-process distillation step"),
    (dict(crop=300), "the teacher view kernel does not take"),
    (dict(T=0.0), "temperature T=0.0 must be positive"),
]


@pytest.mark.parametrize("which", ["train", "train_distill"])
def test_refusals_come_before_a_device_and_in_order(built, tmp_path, monkeypatch, which):
    from spectre_vit import harness
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was touched"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    fn, refusals = (harness.train, TRAIN_REFUSALS) if which == "train" else (harness.train_distill, DISTILL_REFUSALS)
    out = str(tmp_path / "x")
    for kw, message in refusals:
        with pytest.raises(ValueError) as e:
            fn(MNIST, out_dir=out, **kw)
        assert message in str(e.value)
    for (kw_a, message), (kw_b, _) in itertools.combinations(refusals, 2):   # two bad arguments: the earlier refusal wins
        with pytest.raises(ValueError) as e:
            fn(MNIST, out_dir=out, **kw_a, **{k: v for k, v in kw_b.items() if k not in kw_a})
        assert message in str(e.value), (kw_a, kw_b)
    assert not os.path.exists(out), "a refused run leaves nothing behind"
    # the other early distill=True refusals of train()
    if which == "train":
        for kw, message in ((dict(device_meter=True), "device_meter=True meters"), (dict(device_loader=True), "device_loader=True fetches"),
                            (dict(augment=True), "augment=True yields")):
            with pytest.raises(ValueError) as e:
                fn(MNIST, out_dir=out, distill=True, **kw)
            assert message in str(e.value)
