#!/usr/bin/env python3
"""What does the on-device step control cost per training step?  

The graph-replayed bs-512 FFT step of bench.py (SMALL, bf16 autocast, FusedAdamW(static_grads=True)), captured twice in ONE process on
one build: with the controls off (the shipped launch: spv_adamw_multi, rate by value) and with all three on (CosineSchedule +
max_grad_norm + skip_nonfinite: spv_grad_sumsq, spv_step_control, spv_adamw_multi_ctl).  The two graphs are timed alternately, round
by round, BASELINE.md section 3's counts (>= 20 warm-up replays, >= 100 timed ones, device-synchronised, median).  One JSON line.

    python tools/step_control_probe.py [--rounds 10] [--per-round 20] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/step_control_probe.py --rounds 2     # per-kernel durations

Only one graph-replayed step may own the library's dropout seed word, so the first step object is closed after its capture and its
graph replayed directly: its dropout kernels (p = 0.001) then draw their masks from the second step's seed word, which changes no
launch and no byte moved.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import SMALL  # noqa: E402
from spectre_vit.graph import GraphedTrainStep  # noqa: E402
from spectre_vit.loss import CrossEntropyLoss  # noqa: E402
from spectre_vit.models.spectre.spectre import SpectreViT  # noqa: E402
from spectre_vit.optim import CosineSchedule, FusedAdamW  # noqa: E402


def build(controls, img, labels, total_steps):
    torch.manual_seed(0)
    model = SpectreViT(**SMALL, mixer="fft").to(img.device).train()
    kw = dict(schedule=CosineSchedule(total_steps, warmup_steps=10, eta_min=1e-6), max_grad_norm=1.0, skip_nonfinite=True) if controls else {}
    opt = FusedAdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True, **kw)
    step = GraphedTrainStep(model, opt, CrossEntropyLoss(), img, labels, autocast_dtype=torch.bfloat16)
    return model, opt, step


def timed(graph, n):
    """n replays between two device events -> ms per replay"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per-round", type=int, default=20, help="replays per timed window; rounds * per-round >= 100 timed steps per side")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(a.batch, 3, 32, 32, generator=g).to(dev)
    labels = torch.randint(0, 100, (a.batch,), generator=g).to(dev)
    total = 2 * (a.warmup + a.rounds * a.per_round) + 64   # the schedule stays inside its cosine for the whole probe
    _, _, off = build(False, img, labels, total)
    off.close()
    _, opt_on, on = build(True, img, labels, total)
    try:
        for _ in range(a.warmup):
            off.graph.replay()
            on.graph.replay()
        torch.cuda.synchronize()
        t_off, t_on = [], []
        for _ in range(a.rounds):   # alternating windows: drift of the box hits both sides alike
            t_off.append(timed(off.graph, a.per_round))
            t_on.append(timed(on.graph, a.per_round))
        rec = {"workload": f"SpectreViT Small fft, bs {a.batch}, bf16, graph replay", "rounds": a.rounds, "replays_per_round": a.per_round,
               "controls_off_ms": statistics.median(t_off), "controls_on_ms": statistics.median(t_on),
               "controls_off_ms_min_max": [min(t_off), max(t_off)], "controls_on_ms_min_max": [min(t_on), max(t_on)],
               "delta_us": (statistics.median(t_on) - statistics.median(t_off)) * 1e3,
               "loss_off": float(off.loss), "loss_on": float(on.loss), "last_lr": opt_on.last_lr()[0],
               "last_grad_norm": opt_on.last_grad_norm(), "skipped_steps": opt_on.skipped_steps(), "schedule_step": opt_on.schedule_step()}
    finally:
        on.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
