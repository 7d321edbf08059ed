"""harness.train / train_distill on the GPU in the argument combinations no other GPU test runs through the shared loop: the device meter
on the loader-fed replayed step, the averaged weights through the evaluation session after eager training, a named rule with step
control and accumulation on the eager path, and train_distill with meter + averaging + session and with a named rule.  Each case is one
small run (two epochs of two steps, a 40-sample validation set whose tail batch is short) held to facts that need no other run."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = "spectre_vit/configs/spectre_vit_mnist.py"
EPOCHS, STEPS, N_VAL = 2, 2, 40
BASE = ["epoch", "Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation", "steps", "val_samples"]
CONTROL = ["LR", "GradNorm", "SkippedSteps"]
ACCUM = ["AccumulateSteps", "OptimizerSteps"]
EMA = ["Accuracy/ValidationEMA", "Loss/ValidationEMA"]
DISTILL_LINE = ["step", "Batch Loss/Train", "Batch Loss/Dist", "Batch Loss/CE"]

# name -> (entry point, its arguments, the record's keys behind BASE, the fields of a per-step log line or None)
CASES = {
    "train-graph-loader-augment-meter": ("train", dict(graph=True, device_loader=True, augment=True, device_meter=True),
                                         ["Accuracy/TrainTop5"], ["step", "Batch Loss/Train"]),
    "train-eager-grapheval-ema": ("train", dict(graph_eval=True, ema_decay=0.9), EMA, None),
    "train-eager-cosine-clip-accum-sgd": ("train", dict(lr_schedule="cosine", clip_grad_norm=1.0, accumulate_steps=2, optimizer="sgd"),
                                          ["Optimizer"] + CONTROL + ACCUM, None),
    "distill-meter-ema-grapheval": ("train_distill", dict(device_meter=True, ema_decay=0.9, graph_eval=True),
                                    ["Accuracy/TrainTop5"] + EMA, DISTILL_LINE),
    "distill-adam-accum-skip": ("train_distill", dict(optimizer="adam", accumulate_steps=2, skip_nonfinite=True),
                                ["Optimizer"] + CONTROL + ACCUM, DISTILL_LINE),
}


def _run(out, fn_name, kw, monkeypatch):
    """one harness call -> (history, the log's lines, the "train" / "val" hook events with the loss-backward launches between them)"""
    from spectre_vit import _native, harness
    events, real = [], _native.call

    def recorder(name, *a):
        if name.endswith("_bwd") and ("loss" in name or "cross_entropy" in name):
            events.append(("loss_bwd", None))
        return real(name, *a)

    monkeypatch.setattr(_native, "call", recorder)
    _, history = getattr(harness, fn_name)(CFG, mixer="fft", n_train=64, n_val=N_VAL, batch_size=16, steps_per_epoch=STEPS, epochs=EPOCHS,
                                           out_dir=out, log=lambda r: None,
                                           batch_hook=lambda kind, step, img, label: events.append((kind, step)), **kw)
    monkeypatch.setattr(_native, "call", real)
    torch.cuda.synchronize()
    return history, [json.loads(text) for text in open(os.path.join(out, "scalars.jsonl"))], events


@pytest.mark.parametrize("case", list(CASES))
def test_harness_loop_case(tmp_path, monkeypatch, case):
    fn_name, kw, extra, step_line = CASES[case]
    out = str(tmp_path / "a")
    history, lines, events = _run(out, fn_name, kw, monkeypatch)
    print(case, history)
    assert len(history) == EPOCHS
    for e, rec in enumerate(history):
        assert list(rec) == BASE + extra
        assert (rec["epoch"], rec["steps"], rec["val_samples"]) == (e + 1, STEPS, N_VAL)
        assert all(math.isfinite(v) for v in rec.values() if isinstance(v, float))
    if "accumulate_steps" in kw:
        assert [r["OptimizerSteps"] for r in history] == [1, 2] and all(r["AccumulateSteps"] == 2 for r in history)
    if "optimizer" in kw:
        assert all(r["Optimizer"] == kw["optimizer"] for r in history)
    # the "train" hooks: consecutive step numbers across the epoch boundary, every step once
    assert [s for k, s in events if k == "train"] == list(range(EPOCHS * STEPS))
    if fn_name == "train_distill":
        assert [s for k, s in events if k == "teacher"] == list(range(EPOCHS * STEPS))
    from spectre_vit.configs.parser import parse_config
    val_batch = min(parse_config(CFG).val_batch_size, N_VAL)
    assert [s for k, s in events if k == "val"] == list(range(-(-N_VAL // val_batch))) * EPOCHS, "every validation batch, the tail too"
    # ... in front of the step without a loader, behind it with one: has the step's loss backward been launched when hook 0 is called?
    first = events.index(("train", 0))
    assert (("loss_bwd", None) in events[:first]) == bool(kw.get("device_loader"))
    if not kw.get("graph"):   # an eager step launches every time: the same at the second epoch's first step
        val_end = max(i for i, ev in enumerate(events[:events.index(("train", STEPS))]) if ev[0] == "val")
        assert (("loss_bwd", None) in events[val_end:events.index(("train", STEPS))]) == bool(kw.get("device_loader"))
    # scalars.jsonl: per epoch the per-step lines, then the record; the time last
    want = []
    for e in range(EPOCHS):
        want += [("step", e * STEPS + k) for k in range(STEPS if step_line else 0)] + [("epoch", e + 1)]
    assert [("step", l["step"]) if "step" in l else ("epoch", l.get("epoch")) for l in lines[:-1]] == want
    assert all(list(l) == step_line for l in lines if "step" in l) and list(lines[-1]) == ["Training time"]
    assert [l for l in lines if "epoch" in l] == history
    assert sorted(os.listdir(out)) == ["model_best.pt"] + ["model_ema_best.pt"] * ("ema_decay" in kw) + ["scalars.jsonl"]
    if kw.get("graph"):   # the run closed its graphed step and released the seed word: a second replayed run in the process succeeds
        again, _, _ = _run(str(tmp_path / "b"), fn_name, kw, monkeypatch)
        assert [r["steps"] for r in again] == [STEPS] * EPOCHS
