#!/usr/bin/env python3
"""What does a full-state checkpoint cost a run, and what does the one launch replace?  

The workload: harness.train on the Small / CIFAR-100 config, fft mixer, batch 512, 100 steps per epoch, graph=True, device_loader=True,
ema_decay on -- the step is one replay.  Three arms alternate in ONE process (round by round, so the drift of the box hits every arm
alike); every call runs --epochs epochs and the first (it holds the capture) is left out of the figures:

    none    no checkpoint
    snap    checkpoint_every=1: spectre_vit.checkpoint.StateSnapshot -- one spv_snapshot_multi launch, the file written by a thread
    save    the same state saved the obvious way: a synchronous torch.save of model.state_dict() + optimizer.state_dict() at every
            epoch's end, the host (and, the step being host-issued replays, the training stream) standing still meanwhile

Per arm: the epoch's wall time (record to record, validation included), median and range.  Per checkpoint the time training stood still:
for `snap` the take's host time plus the wait for a write still in flight (the {"Checkpoint": ...} records' take_ms + wait_ms) plus the
launch's device time; for `save` the wall time of the save.  And the launch against what it replaces: torch._foreach_copy_ of the same
tensors into views of the same staging buffer, device events around both, in alternating blocks.

    python tools/checkpoint_probe.py [--rounds 3] [--epochs 4] [--out profiles/checkpoint_v1_probe.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/checkpoint_probe.py --kernel-only      # the launch alone, for its trace

Fails without a GPU.  One JSON line.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

CFG = "spectre_vit/configs/spectre_vit_cifar100.py"
HBM_COPY_TBS = 6.29   # MI355X, measured float4 copy rate


def _spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def run_arm(arm, a, out_dir):
    """one harness.train call -> (epoch wall times in ms without the first epoch, per-checkpoint stalls in ms, the Checkpoint records)"""
    from spectre_vit import harness
    stamps, stalls, made = [time.perf_counter()], [], []
    real = harness._make_optimizer

    def keep(*args, **kw):
        made.append(real(*args, **kw))
        return made[-1]

    def log(rec):
        if arm == "save":   # the obvious way, at the epoch's end
            t0 = time.perf_counter()
            torch.save({"model": model_of[0].state_dict(), "optimizer": made[-1].state_dict()}, os.path.join(out_dir, "obvious.pt"))
            stalls.append((time.perf_counter() - t0) * 1e3)
        stamps.append(time.perf_counter())

    model_of, real_build = [], harness.build_model

    def keep_model(*args, **kw):
        model_of[:] = [real_build(*args, **kw)]
        return model_of[0]
    harness._make_optimizer, harness.build_model = keep, keep_model
    try:
        harness.train(CFG, mixer="fft", epochs=a.epochs, steps_per_epoch=a.steps, batch_size=a.batch, n_train=a.batch * a.steps, n_val=1024,
                      graph=True, device_loader=True, ema_decay=0.999, out_dir=out_dir, log=log,
                      checkpoint_every=1 if arm == "snap" else None)
    finally:
        harness._make_optimizer, harness.build_model = real, real_build
    torch.cuda.synchronize()
    epochs = [(b - c) * 1e3 for c, b in zip(stamps[1:], stamps[2:])]   # the first epoch holds set-up and the capture
    records = [json.loads(text)["Checkpoint"] for text in open(os.path.join(out_dir, "scalars.jsonl")) if '"Checkpoint"' in text]
    if arm == "snap":
        stalls = [r["take_ms"] + r["wait_ms"] for r in records[1:]]
    return epochs, stalls[1:] if arm == "save" else stalls, records


def kernel_arm(a, reps):
    """the launch against torch._foreach_copy_ of the same tensors into views of the same staging buffer -> the figures' dict"""
    from bench import SMALL
    from spectre_vit.checkpoint import StateSnapshot
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SpectreViT(**SMALL, mixer="fft").to(dev)
    opt = FusedAdamW(model.parameters(), lr=1e-3, capturable=True, ema_decay=0.999)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()
    blocks = [("model/" + k, v) for k, v in model.state_dict().items()] + opt.state_blocks()[0]
    tmp = tempfile.mkdtemp(prefix="spv_ckpt_probe_")
    snap = StateSnapshot(blocks, tmp)
    srcs = [t for _, t in blocks if t.numel()]
    views = [snap.staging[m["offset"]:m["offset"] + m["bytes"]].view(t.dtype).view(t.shape)
             for m, (_, t) in zip(snap.metas, blocks) if t.numel()]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    launch_us, foreach_us = [], []
    try:
        for _ in range(5):
            snap.launch()
            torch._foreach_copy_(views, srcs)
        torch.cuda.synchronize()
        for _ in range(reps):   # alternating
            launch_us.append(timed(snap.launch))
            foreach_us.append(timed(lambda: torch._foreach_copy_(views, srcs)))
    finally:
        snap.close()
        shutil.rmtree(tmp, ignore_errors=True)
    moved = 2 * snap.state_bytes
    med = statistics.median(launch_us)
    return {"state_bytes": snap.state_bytes, "jobs": len(blocks), "chunks": snap.nchunks, "chunk_bytes": snap.chunk_bytes,
            "launch_us": _spread(launch_us), "foreach_copy_us": _spread(foreach_us),
            "launch_TBps": moved / (med * 1e-6) / 1e12, "share_of_hbm_copy_rate": moved / (med * 1e-6) / 1e12 / HBM_COPY_TBS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="the launch / _foreach_copy_ comparison alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("checkpoint_probe needs a GPU")
    rec = {"workload": f"harness.train Small fft cifar100, bs {a.batch}, {a.steps} steps/epoch, graph + device_loader + ema",
           "kernel": kernel_arm(a, a.kernel_reps)}
    if not a.kernel_only:
        arms = ("none", "snap", "save")
        epochs, stalls, ckpt = {k: [] for k in arms}, {k: [] for k in arms}, []
        for _ in range(a.rounds):
            for arm in arms:
                out_dir = tempfile.mkdtemp(prefix=f"spv_ckpt_{arm}_")
                try:
                    e, s, records = run_arm(arm, a, out_dir)
                finally:
                    shutil.rmtree(out_dir, ignore_errors=True)
                epochs[arm] += e
                stalls[arm] += s
                ckpt += records
        launch_ms = rec["kernel"]["launch_us"]["median"] / 1e3
        rec["rounds"], rec["epochs_per_call"] = a.rounds, a.epochs
        rec["epoch_ms"] = {k: _spread(v) for k, v in epochs.items()}
        rec["stall_ms_per_checkpoint"] = {"snap_host": _spread(stalls["snap"]), "snap_launch_device": launch_ms,
                                          "snap": statistics.median(stalls["snap"]) + launch_ms, "save": _spread(stalls["save"])}
        rec["checkpoint_records"] = {"bytes": ckpt[0]["bytes"], "take_ms": _spread([c["take_ms"] for c in ckpt]),
                                     "wait_ms": _spread([c["wait_ms"] for c in ckpt]), "write_ms": _spread([c["write_ms"] for c in ckpt])}
        base = rec["epoch_ms"]["none"]["median"]
        rec["epoch_ms_over_none"] = {k: rec["epoch_ms"][k]["median"] - base for k in ("snap", "save")}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
