#!/usr/bin/env python3
"""What does the training loop's bookkeeping cost per step, issued from the host and kept by the loss kernel?  

The graph-replayed bs-512 FFT step of bench.py (SMALL, bf16 autocast, FusedAdamW(static_grads=True)), captured twice in ONE process on
one build: with CrossEntropyLoss() (the un-metered launch, spv_cross_entropy_fwd) and with CrossEntropyLoss(meter=TrainMeter(...))
(spv_cross_entropy_meter_fwd).  Two loops, each the loop of harness.train(graph=True) around its step:

    host    batch copy, replay, then  correct += (label == argmax(out)).sum();  running += loss   -- five eager launches per step, and
            two .item() reads per epoch
    meter   batch copy, replay                                                                     -- and one meter.read() + reset()
            per epoch

An epoch is --epoch-steps steps (97: CIFAR-100's 50 000 samples at batch 512).  The sides are timed alternately, window by window, with a
host clock around --per-round steps that end in a device synchronise (BASELINE.md section 3's counts: >= 20 warm-up steps, >= 100 timed
ones per side); the host side is measured as three interleaved series, whose medians' spread is the run-to-run spread the difference
is judged against.  "host_launches_per_step" counts what the host issues per step: the two batch copies, the graph launch, and the
bookkeeping launches.  One JSON line.

    python tools/meter_probe.py [--rounds 12] [--per-round 97] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/meter_probe.py --rounds 2      # per-kernel durations (ce_fwd_kernel,
                                                                                            # ce_meter_fwd_kernel, the five eager kernels)

Only one graph-replayed step may own the library's dropout seed word, so the first step object is closed after its capture and its
graph replayed directly (as tools/ema_probe.py does): its dropout kernels then draw their masks from the second step's seed word, which
changes no launch and no byte moved.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import SMALL  # noqa: E402
from spectre_vit.graph import GraphedTrainStep  # noqa: E402
from spectre_vit.loss import CrossEntropyLoss  # noqa: E402
from spectre_vit.meter import TrainMeter  # noqa: E402
from spectre_vit.models.spectre.spectre import SpectreViT  # noqa: E402
from spectre_vit.optim import FusedAdamW  # noqa: E402


def build(meter, img, labels):
    torch.manual_seed(0)
    model = SpectreViT(**SMALL, mixer="fft").to(img.device).train()
    opt = FusedAdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True)
    return GraphedTrainStep(model, opt, CrossEntropyLoss(meter=meter), img, labels, autocast_dtype=torch.bfloat16, warmup=1)


class HostLoop:
    """harness.train(graph=True)'s loop as it accounts on the host"""
    launches_per_step = 2 + 1 + 5   # img / label copy, graph launch; argmax, ==, sum, +=, +=

    def __init__(self, step, epoch_steps):
        self.step, self.epoch_steps, self.n = step, epoch_steps, 0
        dev = step.img.device
        self.running = torch.zeros((), device=dev)
        self.correct = torch.zeros((), device=dev, dtype=torch.int64)
        self.last = None

    def __call__(self, img, label):
        s = self.step
        s.img.copy_(img, non_blocking=True)
        s.labels.copy_(label, non_blocking=True)
        s.graph.replay()
        self.correct += (label == torch.argmax(s.out, dim=1)).sum()
        self.running += s.loss.detach()
        self.n += 1
        if self.n % self.epoch_steps == 0:
            self.last = ((self.running / self.epoch_steps).item(), self.correct.item() / (self.epoch_steps * label.size(0)))
            self.running.zero_()
            self.correct.zero_()


class MeterLoop:
    """the same loop with the books kept by the loss launch"""
    launches_per_step = 2 + 1

    def __init__(self, step, meter, epoch_steps):
        self.step, self.meter, self.epoch_steps, self.n = step, meter, epoch_steps, 0
        self.last = None

    def __call__(self, img, label):
        s = self.step
        s.img.copy_(img, non_blocking=True)
        s.labels.copy_(label, non_blocking=True)
        s.graph.replay()
        self.n += 1
        if self.n % self.epoch_steps == 0:
            m = self.meter.read()
            self.meter.reset()
            self.last = (m["loss_mean"], m["accuracy"], m["steps"], m["dropped"])


def window(loop, img, label, n):
    """n steps between two host clock reads, the second behind a device synchronise -> ms per step"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loop(img, label)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--epoch-steps", type=int, default=97)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=97, help="steps per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(a.batch, 3, 32, 32, generator=g).to(dev)
    labels = torch.randint(0, 100, (a.batch,), generator=g).to(dev)
    plain = build(None, img, labels)
    plain.close()
    meter = TrainMeter(a.epoch_steps, topk=5, device=dev)
    metered = build(meter, img, labels)
    meter.reset()   # the warm-up step logged its row
    host = [HostLoop(plain, a.epoch_steps) for _ in range(3)]   # three series of the same loop: their spread is the yardstick
    dev_loop = MeterLoop(metered, meter, a.epoch_steps)
    try:
        for _ in range(a.warmup):
            for loop in host:
                loop(img, labels)
            dev_loop(img, labels)
        meter.reset()
        dev_loop.n = 0
        for loop in host:
            loop.n = 0
            loop.running.zero_()
            loop.correct.zero_()
        t_host, t_meter = [[], [], []], []
        for _ in range(a.rounds):   # alternating windows: drift of the box hits every side alike
            for series, loop in zip(t_host, host):
                series.append(window(loop, img, labels, a.per_round))
            t_meter.append(window(dev_loop, img, labels, a.per_round))
        med = statistics.median
        host_meds = [med(s) for s in t_host]
        rec = {"workload": f"SpectreViT Small fft, bs {a.batch}, bf16, graph replay", "rounds": a.rounds, "steps_per_window": a.per_round,
               "epoch_steps": a.epoch_steps,
               "host_ms_per_step_series": host_meds, "host_ms_per_step": med(host_meds), "host_spread_us": (max(host_meds) - min(host_meds)) * 1e3,
               "host_ms_min_max": [min(min(s) for s in t_host), max(max(s) for s in t_host)],
               "meter_ms_per_step": med(t_meter), "meter_ms_min_max": [min(t_meter), max(t_meter)],
               "delta_us": (med(t_meter) - med(host_meds)) * 1e3,
               "host_launches_per_step": {"host": HostLoop.launches_per_step, "meter": MeterLoop.launches_per_step},
               "host_reads_per_epoch": {"host": 2, "meter": 1},
               "last_epoch_host": host[0].last, "last_epoch_meter": dev_loop.last}
    finally:
        metered.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
