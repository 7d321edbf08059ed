"""Checkpoints and resume, the host side (no GPU): the chunk plan of spv_snapshot_multi, the checksum's restatement (tests/snapshot_ref.py)
against hand-computed vectors and against the package's own, the file's round trip and its refusals by name, the write that fails
between the .tmp and the move, the non-finite gate, the shared loop started from a loaded record, and the argument refusals that come
before any device is touched."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import snapshot_ref as R
import test_harness_loop as L

CHUNK = 64
SIZES = [0, 1, 3, 4, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]


# ---------------------------------------------------------------- the chunk plan
@pytest.mark.parametrize("chunk", [16, CHUNK, 4096])
def test_plan_chunks_covers_every_byte_once(chunk):
    from spectre_vit.checkpoint import plan_chunks
    sizes = [0, 1, 3, 4, 15, 16, 17, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]
    chunk_job, chunk_off = plan_chunks(sizes, chunk)
    assert len(chunk_job) == len(chunk_off)
    seen = [np.zeros(s, dtype=np.int64) for s in sizes]
    for j, off in zip(chunk_job, chunk_off):
        assert off % 16 == 0 and 0 <= off < sizes[j], "a multiple of 16 inside its job"
        seen[j][off:min(off + chunk, sizes[j])] += 1
    assert all((s == 1).all() for s in seen), "every byte of every job in exactly one chunk"
    assert 0 not in chunk_job, "a job of 0 bytes has no chunk"
    assert len(chunk_job) == sum(-(-s // chunk) for s in sizes)


def test_plan_chunks_refuses_a_bad_chunk_size():
    from spectre_vit.checkpoint import plan_chunks
    for bad in (0, -16, 24, 15):
        with pytest.raises(ValueError, match="multiple of 16"):
            plan_chunks([64], bad)


def test_plan_slots_are_aligned_and_disjoint():
    from spectre_vit.checkpoint import plan_slots
    offsets, total = plan_slots(SIZES)
    assert all(o % 256 == 0 for o in offsets) and total % 256 == 0
    ends = [o + s for o, s in zip(offsets, SIZES)]
    assert all(e <= o for e, o in zip(ends, offsets[1:])) and ends[-1] <= total


# ---------------------------------------------------------------- the checksum
def test_checksum_hand_vectors():
    assert R.checksum(b"") == 0
    assert R.checksum(bytes([1, 2, 3, 4])) == 0x04030201
    assert R.checksum(bytes([1, 2, 3, 4, 5])) == 0x04030201 + 5, "the last partial word is zero-padded"
    assert R.checksum(bytes([0xAA, 0xBB, 0xCC])) == 0xCCBBAA
    assert R.checksum(bytes([0xFF] * 8 + [0x01, 0x80])) == 2 * 0xFFFFFFFF + 0x8001
    assert R.checksum(b"\xff" * 4 * 3) == 3 * 0xFFFFFFFF, "the words are summed in 64 bits: no wrap at 2^32"


def test_fold_wraps_past_two_to_the_64():
    from spectre_vit.checkpoint import fold_partials
    sums, bad = fold_partials([0, 1, 0, 1], [2 ** 64 - 1, 7, 5, 2 ** 63], [1, 0, 2, 0], 3)
    assert sums == [4, (7 + 2 ** 63) % 2 ** 64, 0] and bad == [3, 0, 0]


@pytest.mark.parametrize("nbytes", [1, 3, 17, 1000, 1003])
def test_checksum_is_independent_of_the_chunking(nbytes):
    from spectre_vit.checkpoint import checksum32
    data = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)
    want = R.checksum(data)
    assert checksum32(data) == want and checksum32(data.tobytes()) == want, "the package's own definition"
    for chunk in (16, 64, 4096):
        parts = R.chunk_partials(data, 0, chunk)
        assert sum(s for _, s, _ in parts) % 2 ** 64 == want
        assert sum(s for _, s, _ in reversed(parts)) % 2 ** 64 == want


def test_nonfinite_restatement():
    values = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 3.4e38, 1.0], dtype=np.float32)
    assert R.nonfinite(values, 1) == 3 and R.nonfinite(values, 0) == 0
    assert R.nonfinite(values.tobytes() + b"\xff\xff\xff", 1) == 3, "a partial last word is no fp32 value"


# ---------------------------------------------------------------- the file
def _tensors():
    g = torch.Generator().manual_seed(5)
    return [("model/w", torch.randn(7, 5, generator=g)), ("model/perms", torch.randint(0, 9, (3, 11), generator=g)),
            ("optim/0/exp_avg", torch.randn(33, generator=g).to(torch.bfloat16)), ("empty", torch.zeros(0)),
            ("bytes", torch.arange(13, dtype=torch.uint8)), ("optim/control_block", torch.arange(64, dtype=torch.uint8))]


def _host(**over):
    return dict({"fingerprint": {"mixer": "fft", "epochs": 4, "graph": False}, "epoch": 2, "global_step": 8, "history": [{"epoch": 1}]}, **over)


def test_round_trip_through_the_writer(tmp_path):
    from spectre_vit import checkpoint as C
    path = str(tmp_path / C.FILE_NAME)
    writer = C._Writer()
    writer.submit(lambda: C.write_train_state(path, _host(), _tensors(), gated={"model/w"}, epoch=2))
    rec, waited = writer.close()
    assert list(rec) == ["Checkpoint"] and rec["Checkpoint"]["epoch"] == 2 and rec["Checkpoint"]["bytes"] == os.path.getsize(path)
    assert waited >= 0.0 and sorted(os.listdir(tmp_path)) == [C.FILE_NAME], "no .tmp is left"
    state = C.load_train_state(path, fingerprint=_host()["fingerprint"])
    assert state["version"] == C.FORMAT_VERSION and state["host"] == _host()
    for name, t in _tensors():
        got = state["tensors"][name]
        assert got.dtype == t.dtype and got.shape == t.shape and got.view(torch.uint8).equal(t.contiguous().view(torch.uint8)), name
    for job, (name, t) in zip(state["jobs"], _tensors()):
        assert (job["name"], job["bytes"], job["offset"] % 256) == (name, t.numel() * t.element_size(), 0)
        assert job["checksum"] == R.checksum(t.contiguous().view(torch.uint8).numpy())


def _written(tmp_path):
    from spectre_vit import checkpoint as C
    path = str(tmp_path / C.FILE_NAME)
    C.write_train_state(path, _host(), _tensors())
    data = open(path, "rb").read()
    _, _, hlen, _ = struct.unpack(C._PREAMBLE, data[:struct.calcsize(C._PREAMBLE)])
    return C, path, data, struct.calcsize(C._PREAMBLE) + hlen


def test_a_flipped_byte_is_refused_by_the_jobs_name(tmp_path):
    C, path, data, payload = _written(tmp_path)
    jobs = {j["name"]: j for j in C.load_train_state(path)["jobs"]}
    for name in ("model/w", "optim/0/exp_avg", "bytes"):
        at = payload + jobs[name]["offset"] + jobs[name]["bytes"] - 1
        open(path, "wb").write(data[:at] + bytes([data[at] ^ 0x10]) + data[at + 1:])
        with pytest.raises(ValueError, match=f"job '{name}'.*checksum"):
            C.load_train_state(path)
    open(path, "wb").write(data[:40] + bytes([data[40] ^ 1]) + data[41:])   # inside the header
    with pytest.raises(ValueError, match="header"):
        C.load_train_state(path)


def test_a_truncated_file_is_refused_by_name(tmp_path):
    C, path, data, payload = _written(tmp_path)
    jobs = {j["name"]: j for j in C.load_train_state(path)["jobs"]}
    open(path, "wb").write(data[:payload + jobs["model/perms"]["offset"] + 5])
    with pytest.raises(ValueError, match="truncated inside job 'model/perms'"):
        C.load_train_state(path)
    open(path, "wb").write(data[:payload - 3])
    with pytest.raises(ValueError, match="truncated in its header"):
        C.load_train_state(path)
    open(path, "wb").write(data[:5])
    with pytest.raises(ValueError, match="truncated in its preamble"):
        C.load_train_state(path)


def test_a_wrong_version_is_refused(tmp_path):
    C, path, data, _ = _written(tmp_path)
    open(path, "wb").write(data[:8] + struct.pack("<I", C.FORMAT_VERSION + 1) + data[12:])
    with pytest.raises(ValueError, match=f"unknown format version {C.FORMAT_VERSION + 1}"):
        C.load_train_state(path)
    open(path, "wb").write(b"NOTSTATE" + data[8:])
    with pytest.raises(ValueError, match="not a train-state file"):
        C.load_train_state(path)


def test_a_fingerprint_that_differs_in_one_key_names_it(tmp_path):
    C, path, _, _ = _written(tmp_path)
    mine = dict(_host()["fingerprint"])
    assert C.load_train_state(path, fingerprint=mine)["host"]["epoch"] == 2
    with pytest.raises(ValueError, match="differs in 'epochs': 4 in the file, 5 in this call"):
        C.load_train_state(path, fingerprint=dict(mine, epochs=5))
    with pytest.raises(ValueError, match="differs in 'ema_decay'"):
        C.load_train_state(path, fingerprint=dict(mine, ema_decay=0.9))
    with pytest.raises(ValueError, match="differs in 'graph'"):
        C.load_train_state(path, fingerprint={k: v for k, v in mine.items() if k != "graph"})


def test_a_write_that_fails_before_the_move_leaves_the_old_file(tmp_path, monkeypatch):
    C, path, data, _ = _written(tmp_path)

    def killed(src, dst):
        raise OSError("killed between the .tmp and the move")
    monkeypatch.setattr(C.os, "replace", killed)
    writer = C._Writer()
    writer.submit(lambda: C.write_train_state(path, _host(epoch=3), [(n, t + 1 if t.numel() else t) for n, t in _tensors()]))
    with pytest.raises(RuntimeError, match="the checkpoint writer failed.*killed"):
        writer.close()
    monkeypatch.undo()
    assert open(path, "rb").read() == data, "the previous file is whole"
    assert C.load_train_state(path)["host"]["epoch"] == 2
    assert os.path.exists(path + ".tmp"), "what the killed write left is the .tmp alone"


def test_the_nonfinite_gate_keeps_the_old_file(tmp_path):
    C, path, data, _ = _written(tmp_path)
    bad = [(n, t.clone()) for n, t in _tensors()]
    bad[0][1][3, 2] = float("nan")
    bad[0][1][0, 0] = float("-inf")
    rec = C.write_train_state(path, _host(epoch=3), bad, gated={"model/w"}, epoch=3)
    assert rec == {"CheckpointSkipped": {"epoch": 3, "job": "model/w", "nonfinite": 2}}
    assert json.loads(json.dumps(rec)) == rec, "a line of scalars.jsonl"
    assert open(path, "rb").read() == data and not os.path.exists(path + ".tmp")
    # a non-finite value in a job that is not gated (a moment, an accumulator of an open window) is saved as it is
    rec = C.write_train_state(path, _host(epoch=3), bad, gated={"optim/0/ema"}, epoch=3)
    assert list(rec) == ["Checkpoint"]
    w = C.load_train_state(path)["tensors"]["model/w"]
    assert torch.isnan(w[3, 2]) and w[0, 0] == float("-inf")


# ---------------------------------------------------------------- the loop, started from a loaded record
class _Optimizer(L.FakeOptimizer):
    param_groups = []
    loaded = None

    def load_state_dict(self, sd):
        self.loaded = sd


def test_run_epochs_with_a_resumed_record(tmp_path):
    """starts at the saved epoch, continues global_step, keeps best_acc (a worse epoch does not rewrite model_best.pt), restores the
    generators last, adds the saved seconds to the training time"""
    from spectre_vit import checkpoint as C
    from spectre_vit import harness
    out = str(tmp_path / "r")
    run = L.make_run(out)
    run.optimizer = _Optimizer()
    run.session = None
    torch.manual_seed(77)
    rng = C.host_rng_state()
    want_draw = torch.rand(1)
    torch.manual_seed(1)
    saved_w = torch.full((2, 2), 3.0)
    run.resume = {"host": dict(epoch=2, global_step=2 * L.EPOCH_STEPS, elapsed=1000.0, history=[{"epoch": 1}, {"epoch": 2}], best_acc=0.9,
                               best_ema_acc=0.0, rng=rng, param_groups=[], optim_host={0: {"step": 5}}, optim_aliases={}),
                  "tensors": {"model/weight": saved_w, "model/bias": torch.zeros(2), "optim/0/exp_avg": torch.ones(2)}}
    events, draws = [], []
    step = L.make_step(events, 0)

    def hook(kind, n, img, label):
        if kind == "train" and not draws:
            draws.append(torch.rand(1))
    _, history = harness._run_epochs(run, step, harness._TrainBooks(run, L.TRAIN_NAMES, block=False), lambda h: (0.5, 2.0, 40), 4, hook,
                                     False, lambda rec: None)
    assert [e for e in events if e[0] == "run"] == [("run", n) for n in range(2 * L.EPOCH_STEPS, 4 * L.EPOCH_STEPS)]
    assert [r["epoch"] for r in history] == [1, 2, 3, 4] and run.global_step == 4 * L.EPOCH_STEPS
    assert run.model.weight.equal(saved_w), "the saved weights are in the model"
    loaded = run.optimizer.loaded["state"][0]
    assert sorted(loaded) == ["exp_avg", "step"] and loaded["step"] == 5 and loaded["exp_avg"].equal(torch.ones(2))
    assert draws[0].equal(want_draw), "the generators' states are restored right before the loop"
    assert run.best_acc == 0.9 and sorted(os.listdir(out)) == ["scalars.jsonl"], "0.5 < 0.9: model_best.pt is not rewritten"
    lines = [json.loads(text) for text in open(os.path.join(out, "scalars.jsonl"))]
    assert [l.get("epoch") for l in lines[:-1]] == [3, 4] and lines[-1]["Training time"] >= 1000.0
    assert step.closed == [1]


def test_an_exception_still_closes_step_and_log(tmp_path):
    from spectre_vit import harness
    run = L.make_run(str(tmp_path / "r"))
    run.session.close = lambda: setattr(run.session, "closed", run.session.closed + 1)
    step = L.make_step([], 0)

    def hook(kind, n, img, label):
        if kind == "train" and n == L.EPOCH_STEPS:
            raise KeyboardInterrupt("preempted")
    with pytest.raises(KeyboardInterrupt):
        harness._run_epochs(run, step, harness._TrainBooks(run, L.TRAIN_NAMES, block=False), lambda h: (0.5, 2.0, 40), 3, hook, False,
                            lambda rec: None)
    assert step.closed == [1] and run.session.closed == 1 and run.log_f.closed
    lines = [json.loads(text) for text in open(os.path.join(run.out_dir, "scalars.jsonl"))]
    assert [l.get("epoch") for l in lines] == [1], "the finished epoch's record, and no training time"


# ---------------------------------------------------------------- the refusals, before a device
@pytest.mark.parametrize("which", ["train", "train_distill"])
def test_checkpoint_refusals_come_before_a_device(tmp_path, monkeypatch, which):
    import __graft_entry__ as g
    g.build()
    from spectre_vit import checkpoint as C
    from spectre_vit import harness
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was touched"))
    fn = getattr(harness, which)
    out = str(tmp_path / "x")
    cases = [(dict(checkpoint_every=0), "must be None or an int >= 1"), (dict(checkpoint_every=True), "must be None or an int >= 1"),
             (dict(checkpoint_every=0.5), "mid-epoch checkpoints are not built"), (dict(resume=3), "None, True"),
             (dict(resume=True), "no such file"), (dict(resume=str(tmp_path / "nowhere.pt")), "no such file")]
    for kw, message in cases:
        with pytest.raises(ValueError) as e:
            fn(L.MNIST, out_dir=out, **kw)
        assert message in str(e.value), kw
    monkeypatch.setenv("WORLD_SIZE", "2")
    for kw in (dict(checkpoint_every=1), dict(resume=True)):
        with pytest.raises(ValueError, match="world > 1"):
            fn(L.MNIST, out_dir=out, **kw)
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert not os.path.exists(out), "a refused run leaves nothing behind"
    # another run's file: refused by the first differing key, still before a device
    os.makedirs(out)
    C.write_train_state(os.path.join(out, C.FILE_NAME), {"fingerprint": {"entry": "elsewhere"}}, _tensors())
    with pytest.raises(ValueError, match="differs in 'entry'"):
        fn(L.MNIST, out_dir=out, resume=True)
    with open(os.path.join(out, C.FILE_NAME), "r+b") as f:
        f.truncate(os.path.getsize(os.path.join(out, C.FILE_NAME)) - 700)
    with pytest.raises(ValueError, match="truncated inside job"):
        fn(L.MNIST, out_dir=out, resume=True)


def test_cli_arguments():
    from spectre_vit import harness
    a = harness.build_parser().parse_args([])
    assert a.checkpoint_every is None and a.resume is None
    a = harness.build_parser().parse_args(["--checkpoint-every", "2", "--resume"])
    assert a.checkpoint_every == 2 and a.resume is True
    assert harness.build_parser().parse_args(["--resume", "runs/x/train_state.pt"]).resume == "runs/x/train_state.pt"


def test_native_symbol_is_declared():
    from spectre_vit import _native
    assert "spv_snapshot_multi" in _native.SIGNATURES and len(_native.SIGNATURES["spv_snapshot_multi"]) == 8
