#!/usr/bin/env python3
"""What does the weight average cost per training step, inside the optimizer launch and from outside?  

The graph-replayed bs-512 FFT step of bench.py (SMALL, bf16 autocast, FusedAdamW(static_grads=True)), captured twice in ONE process on
one build: with averaging off (the shipped launch: spv_adamw_multi) and with ema_decay=0.999, ema_warmup=True (spv_adamw_multi_ema:
the same launch, one more 4-byte read and write per element).  Three sides are timed alternately, round by round, BASELINE.md
section 3's counts (>= 20 warm-up replays, >= 100 timed ones, device-synchronised, median):

    off        the graph without averaging
    on         the graph with the average inside the optimizer launch
    off+lerp   the graph without averaging, and after every replay a host-issued torch._foreach_lerp_ over the model's tensors --
               what a user can do from outside (with a constant weight: a warm-up would need a host-side count on top)

One JSON line.

    python tools/ema_probe.py [--rounds 10] [--per-round 20] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ema_probe.py --rounds 2     # per-kernel durations

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
from spectre_vit.optim import FusedAdamW  # noqa: E402

DECAY = 0.999


def build(ema, img, labels):
    torch.manual_seed(0)
    model = SpectreViT(**SMALL, mixer="fft").to(img.device).train()
    kw = dict(ema_decay=DECAY, ema_warmup=True) if ema else {}
    opt = FusedAdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True, **kw)
    step = GraphedTrainStep(model, opt, CrossEntropyLoss(), img, labels, autocast_dtype=torch.bfloat16)
    return model, opt, step


def timed(graph, n, after=None):
    """n replays (each followed by after(), when given) between two device events -> ms per replay"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
        if after is not None:
            after()
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
    model_off, _, off = build(False, img, labels)
    off.close()
    _, opt_on, on = build(True, img, labels)
    params = [p.detach() for p in model_off.parameters()]
    host_ema = [p.clone() for p in params]

    def host_lerp():
        torch._foreach_lerp_(host_ema, params, 1.0 - DECAY)

    try:
        for _ in range(a.warmup):
            off.graph.replay()
            on.graph.replay()
            off.graph.replay()
            host_lerp()
        torch.cuda.synchronize()
        t_off, t_on, t_lerp = [], [], []
        for _ in range(a.rounds):   # alternating windows: drift of the box hits every side alike
            t_off.append(timed(off.graph, a.per_round))
            t_on.append(timed(on.graph, a.per_round))
            t_lerp.append(timed(off.graph, a.per_round, host_lerp))
        med = statistics.median
        ema = opt_on.ema_parameters()
        rec = {"workload": f"SpectreViT Small fft, bs {a.batch}, bf16, graph replay", "rounds": a.rounds, "replays_per_round": a.per_round,
               "tensors": len(params), "elements": sum(p.numel() for p in params),
               "ema_off_ms": med(t_off), "ema_on_ms": med(t_on), "ema_off_host_lerp_ms": med(t_lerp),
               "ema_off_ms_min_max": [min(t_off), max(t_off)], "ema_on_ms_min_max": [min(t_on), max(t_on)],
               "ema_off_host_lerp_ms_min_max": [min(t_lerp), max(t_lerp)],
               "delta_on_us": (med(t_on) - med(t_off)) * 1e3, "delta_host_lerp_us": (med(t_lerp) - med(t_off)) * 1e3,
               "loss_off": float(off.loss), "loss_on": float(on.loss), "adam_step_on": float(opt_on.state[opt_on.param_groups[0]["params"][0]]["step"]),
               "ema_finite": bool(all(torch.isfinite(e).all() for e in ema))}
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
