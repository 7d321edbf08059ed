"""Bit-exact resume through harness.train / train_distill: a 4-epoch run of 4 steps per epoch with checkpoint_every=1 is interrupted the
way a preemption interrupts it -- batch_hook raises at the first "train" call of epoch 3 -- and continued with resume=True and the same
arguments.  Held against the uninterrupted run, bit for bit: the final model.state_dict(), every optimizer state tensor with the control
block, the accumulators and the averages, the loader's cursor and the seed word (all of them ride in the last train_state.pt), every key
of history, and the "epoch" and "step" lines of scalars.jsonl.  The graphed cases' first step after the resume is the new step object's
eager warm-up step where the uninterrupted run replays: the same launches, hence the same bits (the step is built under the seed word
and the generator state of the interrupted run's capture)."""
import json
import os
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = "spectre_vit/configs/spectre_vit_mnist.py"
EPOCHS, STEPS, N_TRAIN, BATCH = 4, 4, 64, 16
CUT = 2 * STEPS   # the first "train" call of epoch 3
CASES = {
    "eager-defaults": ("train", dict()),
    "eager-fused-sgd": ("train", dict(lr_schedule="cosine", warmup_steps=2, clip_grad_norm=1.0, accumulate_steps=3, ema_decay=0.9,
                                      optimizer="sgd")),
    "graphed": ("train", dict(graph=True, device_loader=True, augment=True, device_meter=True, accumulate_steps=3, ema_decay=0.9,
                              lr_schedule="cosine")),
    "distill-graphed": ("train_distill", dict(graph=True, cache_teacher=True, device_loader=True)),
}
CTL_FMT = "<ddfifiii24x"   # include/spv.h: spv_step_ctl (..., sched_step, skipped, micro)


class Preempted(Exception):
    pass


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _call(fn_name, kw, out, hook=None, **more):
    from spectre_vit import harness
    model, history = getattr(harness, fn_name)(CFG, mixer="fft", n_train=N_TRAIN, n_val=40, batch_size=BATCH, steps_per_epoch=STEPS,
                                               epochs=EPOCHS, out_dir=out, log=lambda r: None, batch_hook=hook, **kw, **more)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, history


def _lines(out):
    return [json.loads(text) for text in open(os.path.join(out, "scalars.jsonl"))]


def _state(out):
    from spectre_vit.checkpoint import FILE_NAME, load_train_state
    return load_train_state(os.path.join(out, FILE_NAME))


def _same_bits(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].cpu().contiguous().reshape(-1).view(torch.uint8).equal(
            b[k].cpu().contiguous().reshape(-1).view(torch.uint8)), f"{what}: {k}"


def _interrupt_and_resume(fn_name, kw, out, hook=None):
    """the interrupted run (checkpoints after epochs 1 and 2, cut at the first step of epoch 3), then the resumed one"""
    def cut(kind, step, img, label):
        if hook is not None:
            hook(kind, step, img, label)
        if kind == "train" and step == CUT:
            raise Preempted
    with pytest.raises(Preempted):
        _call(fn_name, kw, out, cut, checkpoint_every=1)
    assert not [f for f in os.listdir(out) if f.endswith(".tmp")], "the pending write was finished"


@pytest.mark.parametrize("case", list(CASES))
def test_resume_is_bit_exact(tmp_path, monkeypatch, case):
    from spectre_vit import harness
    from spectre_vit.data import ResidentLoader
    fn_name, kw = CASES[case]
    a, b = str(tmp_path / "whole"), str(tmp_path / "cut")
    whole_sd, whole_history = _call(fn_name, kw, a, checkpoint_every=1)
    _interrupt_and_resume(fn_name, kw, b)
    saved = _state(b)
    assert saved["host"]["epoch"] == 2 and saved["host"]["global_step"] == CUT
    if "accumulate_steps" in kw:   # four steps per epoch, windows of three: the window straddles every epoch boundary
        micro = struct.unpack(CTL_FMT, saved["tensors"]["optim/control_block"].numpy().tobytes())[7]
        assert micro == CUT % 3 != 0, "the checkpoint was taken inside an open accumulation window"
        assert any(k.startswith("optim/accumulators/") for k in saved["tensors"])

    loaders, seen = [], []
    real = harness._resident_loader
    monkeypatch.setattr(harness, "_resident_loader", lambda *args: loaders.append(real(*args)) or loaders[-1])

    def hook(kind, step, img, label):
        if kind == "train" and loaders:
            seen.append((step, loaders[-1].index.cpu().numpy().copy()))
    resumed_sd, resumed_history = _call(fn_name, kw, b, hook, checkpoint_every=1, resume=True)

    _same_bits(whole_sd, resumed_sd, "the final model.state_dict()")
    assert resumed_history == whole_history and [list(r) for r in resumed_history] == [list(r) for r in whole_history]
    assert [r["epoch"] for r in resumed_history] == [1, 2, 3, 4]
    kept = lambda lines: [l for l in lines if "epoch" in l or "step" in l]   # noqa: E731
    assert kept(_lines(b)) == kept(_lines(a)), 'the "epoch" and "step" lines of scalars.jsonl'
    # every job of the last checkpoint: optimizer state, control block, accumulators, averages, cursor, seed word, the model again
    end_whole, end_resumed = _state(a), _state(b)
    _same_bits(end_whole["tensors"], end_resumed["tensors"], "the state after epoch 4")
    names = set(end_whole["tensors"])
    assert any(k.startswith("optim/") for k in names) and {"model/" + k for k in whole_sd} <= names
    for key in ("epoch", "global_step", "history", "best_acc", "best_ema_acc", "param_groups", "loader"):
        assert end_whole["host"][key] == end_resumed["host"][key], key
    assert (end_whole["host"]["epoch"], end_whole["host"]["global_step"]) == (EPOCHS, EPOCHS * STEPS)
    if "optim/control_block" in names:
        ctl = struct.unpack(CTL_FMT, end_resumed["tensors"]["optim/control_block"].numpy().tobytes())
        k = kw.get("accumulate_steps") or 1
        assert ctl[5:] == (EPOCHS * STEPS // k, 0, EPOCHS * STEPS % k), "schedule step, skipped steps, micro-step"
    if kw.get("ema_decay"):
        assert any(k.endswith("/ema") for k in names)
    if kw.get("graph"):
        assert {"step/seed_word", "loader/cursor"} <= names
        assert int(end_resumed["tensors"]["loader/cursor"][0]) == EPOCHS * STEPS
        # the loader's index of every step after the resume is the order's own
        assert [s for s, _ in seen] == list(range(CUT, EPOCHS * STEPS))
        for s, index in seen:
            want = ResidentLoader.indices(N_TRAIN, BATCH, harness.loader_seed(42), s, steps_per_epoch=STEPS)
            assert (index == want).all(), f"step {s}"
    want_files = ["model_best.pt"] + ["model_ema_best.pt"] * ("ema_decay" in kw) + ["scalars.jsonl", "train_state.pt"]
    assert sorted(os.listdir(b)) == want_files and sorted(os.listdir(a)) == want_files, "no .tmp is left"
    checkpoints = [l["Checkpoint"] for l in _lines(b) if "Checkpoint" in l]
    assert [c["epoch"] for c in checkpoints] == [1, 2, 3, 4]
    assert all(list(c) == ["epoch", "bytes", "take_ms", "wait_ms", "write_ms"] for c in checkpoints)
    assert sum("Training time" in l for l in _lines(b)) == 1, "the interrupted run wrote none"


def test_checkpoints_do_not_change_a_run(tmp_path):
    """the run with checkpoint_every=1 computes what the run without the argument computes, and that one writes no train_state.pt"""
    fn_name, kw = CASES["graphed"]
    plain_sd, plain_history = _call(fn_name, kw, str(tmp_path / "plain"))
    saved_sd, saved_history = _call(fn_name, kw, str(tmp_path / "saved"), checkpoint_every=2)
    _same_bits(plain_sd, saved_sd, "the final model.state_dict()")
    assert plain_history == saved_history
    assert sorted(os.listdir(tmp_path / "plain")) == ["model_best.pt", "model_ema_best.pt", "scalars.jsonl"]
    assert [l["Checkpoint"]["epoch"] for l in _lines(str(tmp_path / "saved")) if "Checkpoint" in l] == [2, 4]


def test_a_nan_weight_keeps_the_previous_checkpoint(tmp_path):
    """a weight set to NaN before epoch 2's end: that epoch's checkpoint is skipped, train_state.pt stays epoch 1's, and the resume
    continues from there -- to the uninterrupted run's bits"""
    from spectre_vit import harness
    fn_name, kw = CASES["eager-defaults"]
    a, b = str(tmp_path / "whole"), str(tmp_path / "cut")
    whole_sd, whole_history = _call(fn_name, kw, a, checkpoint_every=1)
    models, real = [], harness.build_model
    harness.build_model = lambda *args, **kwargs: models.append(real(*args, **kwargs)) or models[-1]
    try:
        def poison(kind, step, img, label):
            if kind == "train" and step == CUT - 1:
                with torch.no_grad():
                    next(models[-1].parameters()).view(-1)[0] = float("nan")
        _interrupt_and_resume(fn_name, kw, b, poison)
    finally:
        harness.build_model = real
    skipped = [l["CheckpointSkipped"] for l in _lines(b) if "CheckpointSkipped" in l]
    assert len(skipped) == 1 and skipped[0]["epoch"] == 2 and skipped[0]["nonfinite"] > 0 and skipped[0]["job"].startswith("model/")
    assert _state(b)["host"]["epoch"] == 1, "the previous file is in place"
    resumed_sd, resumed_history = _call(fn_name, kw, b, checkpoint_every=1, resume=True)
    _same_bits(whole_sd, resumed_sd, "the final model.state_dict()")
    assert resumed_history == whole_history
    _same_bits(_state(a)["tensors"], _state(b)["tensors"], "the state after epoch 4")
