#!/usr/bin/env python3
"""What does the update rule cost per replayed step?  

The graph-replayed bs-512 FFT step of bench.py (SMALL, bf16 autocast, static_grads=True), captured once per arm in ONE process on one
build, tools/accum_probe.py's method:

    adamw   FusedAdamW(weight_decay=0.01): the shipped launch (spv_adamw_multi)
    adam    FusedAdam(weight_decay=0.01): spv_adam_multi
    sgd     FusedSGD(momentum=0.9, nesterov=True, weight_decay=0.01): spv_sgd_multi

The arms' graphs are timed alternately, block by block (>= 20 warm-up replays, rounds x per-round timed ones, device-synchronised); per
arm the median over the blocks and their spread.  One JSON line.

    python tools/optim_rules_probe.py [--arms adamw,adam,sgd] [--rounds 10] [--per-round 20] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/optim_rules_probe.py --rounds 4 --per-round 4 --warmup 4     # per-kernel durations:
        # 24 launches of each arm's optimizer kernel = 4 eager warm-up steps of the capture + 4 warm-up replays + 4 x 4 timed ones

An arm may be named twice.  Only one graph-replayed step may own the library's dropout seed word, so every step object but the last is
closed after its capture and its graph replayed directly (tools/accum_probe.py).
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
from spectre_vit.optim import FusedAdam, FusedAdamW, FusedSGD  # noqa: E402

ARMS = {"adamw": lambda ps: FusedAdamW(ps, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True),
        "adam": lambda ps: FusedAdam(ps, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True),
        "sgd": lambda ps: FusedSGD(ps, lr=1e-3, momentum=0.9, nesterov=True, weight_decay=0.01, capturable=True, static_grads=True)}


def build(name, img, labels):
    torch.manual_seed(0)
    model = SpectreViT(**SMALL, mixer="fft").to(img.device).train()
    opt = ARMS[name](model.parameters())
    return opt, GraphedTrainStep(model, opt, CrossEntropyLoss(), img, labels, autocast_dtype=torch.bfloat16, warmup=4)


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
    ap.add_argument("--arms", default="adamw,adam,sgd", help="comma-separated, from adamw / adam / sgd; a name may repeat")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10, help="timed blocks per arm")
    ap.add_argument("--per-round", type=int, default=20, help="replays per block")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arms = a.arms.split(",")
    if any(n not in ARMS for n in arms):
        ap.error("--arms takes adamw / adam / sgd")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(a.batch, 3, 32, 32, generator=g).to(dev)
    labels = torch.randint(0, 100, (a.batch,), generator=g).to(dev)
    built = []
    for i, name in enumerate(arms):
        opt, step = build(name, img, labels)
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
            rec["arms"][tag] = {"optimizer": type(opt).__name__, "ms_per_replay_median": statistics.median(t), "ms_min_max": [min(t), max(t)],
                                "blocks_ms": t, "loss": float(step.loss)}
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
