#!/usr/bin/env python3
"""What does on-device gradient accumulation cost per replayed micro-step?  

The graph-replayed bs-512 FFT step of bench.py (SMALL, bf16 autocast, FusedAdamW(static_grads=True)), captured once per arm in ONE
process on one build:

    none   accumulate_steps=None: the shipped launch (spv_adamw_multi, rate by value) -- the launch sequence of a build without the option
    k1     accumulate_steps=1: spv_grad_accumulate, spv_step_control_accum, spv_adamw_multi_ctl; every replay applies
    k4     accumulate_steps=4: the same graph shape; three replays in four stop at the optimizer launch's first instruction

The arms' graphs are timed alternately, block by block (>= 20 warm-up replays, rounds x per-round timed ones, device-synchronised); per
arm the median over the blocks and their spread.  per-round is a multiple of 4, so every k4 block holds whole windows.  One JSON line.

    python tools/accum_probe.py [--arms none,k1,k4] [--rounds 10] [--per-round 20] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/accum_probe.py --arms k4 --rounds 2     # per-kernel durations

An arm may be named twice (--arms none,none): two captures of the same step, whose difference is the run-to-run spread of the box.
Only one graph-replayed step may own the library's dropout seed word, so every step object but the last is closed after its capture
and its graph replayed directly: its dropout kernels (p = 0.001) then draw their masks from the last step's seed word, which changes
no launch and no byte moved.
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
from spectre_vit.optim import FusedAdamW  # noqa: E402

ARMS = {"none": None, "k1": 1, "k4": 4}


def build(k, img, labels):
    torch.manual_seed(0)
    model = SpectreViT(**SMALL, mixer="fft").to(img.device).train()
    kw = {} if k is None else dict(accumulate_steps=k)
    opt = FusedAdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True, **kw)
    step = GraphedTrainStep(model, opt, CrossEntropyLoss(), img, labels, autocast_dtype=torch.bfloat16, warmup=4)
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
    ap.add_argument("--arms", default="none,k1,k4", help="comma-separated, from none / k1 / k4; a name may repeat")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10, help="timed blocks per arm (at least 5)")
    ap.add_argument("--per-round", type=int, default=20, help="replays per block, a multiple of 4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arms = a.arms.split(",")
    if any(n not in ARMS for n in arms) or a.per_round % 4 or a.warmup % 4:
        ap.error("--arms takes none / k1 / k4; --per-round and --warmup are multiples of 4")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(a.batch, 3, 32, 32, generator=g).to(dev)
    labels = torch.randint(0, 100, (a.batch,), generator=g).to(dev)
    built = []
    for i, name in enumerate(arms):
        _, opt, step = build(ARMS[name], img, labels)
        if i < len(arms) - 1:
            step.close()
        built.append((f"{name}#{i}" if arms.count(name) > 1 else name, opt, step))
    try:
        for _ in range(a.warmup):
            for _, _, step in built:
                step.graph.replay()
        torch.cuda.synchronize()
        times = {tag: [] for tag, _, _ in built}
        for _ in range(a.rounds):   # alternating blocks: drift of the box hits every arm alike
            for tag, _, step in built:
                times[tag].append(timed(step.graph, a.per_round))
        rec = {"workload": f"SpectreViT Small fft, bs {a.batch}, bf16, graph replay", "rounds": a.rounds, "replays_per_round": a.per_round,
               "arms": {}}
        for tag, opt, step in built:
            t = times[tag]
            arm = {"ms_per_replay_median": statistics.median(t), "ms_min_max": [min(t), max(t)], "blocks_ms": t, "loss": float(step.loss)}
            if opt.accumulate_steps is not None:
                arm.update(accumulate_steps=opt.accumulate_steps, optimizer_steps=opt.schedule_step(), micro_step=opt.micro_step(),
                           last_grad_norm=opt.last_grad_norm())
            rec["arms"][tag] = arm
        base = rec["arms"][built[0][0]]["ms_per_replay_median"]
        rec["delta_us_vs_first_arm"] = {tag: (rec["arms"][tag]["ms_per_replay_median"] - base) * 1e3 for tag, _, _ in built[1:]}
    finally:
        built[-1][2].close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
