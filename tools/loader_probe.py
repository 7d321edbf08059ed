#!/usr/bin/env python3
"""What does the resident loader do to a graph-replayed training step?  

The bs-512 FFT step of bench.py (SMALL = the CIFAR-100 config, bf16 autocast, FusedAdamW(static_grads=True)) over a resident uint8
set of CIFAR's size, captured twice in ONE process on one build.  Two arms, timed alternately in blocks of >= 200 steps (three blocks
each, >= 20 warm-up steps of each arm excluded, the host clock around a block that begins and ends in a device synchronise):

    host_fed    GraphedTrainStep fed by the harness's own batch assembly (spectre_vit/harness.py SyntheticCifar.batches): a randperm
                uploaded once per epoch; per step a slice, images[sel], .float(), / 255, - mean, / std, labels[sel], .long(), the two
                copies into the captured buffers, then the replay -- nine host-issued launches and one replay
    loader_fed  GraphedTrainStep(loader=ResidentLoader(...)): the replay and nothing else

Reports each arm's block medians, min and max, and whether loader_fed's median is within host_fed's median plus host_fed's own
max - min spread over its blocks.  One JSON line.

    python tools/loader_probe.py [--blocks 3] [--steps 200] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/loader_probe.py --blocks 1 --steps 50    # the fetch kernel's duration

--augment: the same question for the augmented step, two arms again:

    three_launch  the harness's path before the fused fetch: ResidentLoader(output="none").fetch(), TrainAugment's draw and apply
                  (spv_loader_fetch, spv_augment_params, spv_augment_u8) host-issued, the two copies into the captured buffers, the replay
    fused         GraphedTrainStep(loader=ResidentLoader(output="augment", augment=...)): the replay and nothing else

The record's keys keep their names: host_fed_* is the three-launch arm, loader_fed_* the fused one.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/loader_probe.py --augment --blocks 1 --steps 50   # the four kernels' durations

Only one graph-replayed step may own the library's dropout seed word, so the host-fed step object is closed after its capture and its
graph replayed directly (as tools/ema_probe.py does): its dropout kernels (p = 0.001) then draw their masks from the loader-fed
step's seed word, which changes no launch and no byte moved.
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
from spectre_vit import shadows  # noqa: E402
from spectre_vit.augment import TrainAugment  # noqa: E402
from spectre_vit.data import CIFAR_MEAN, CIFAR_STD, ResidentLoader  # noqa: E402
from spectre_vit.graph import GraphedTrainStep  # noqa: E402
from spectre_vit.loss import CrossEntropyLoss  # noqa: E402
from spectre_vit.models.spectre.spectre import SpectreViT  # noqa: E402
from spectre_vit.optim import FusedAdamW  # noqa: E402


def build(img, labels, loader):
    torch.manual_seed(0)
    dev = loader.img.device if loader is not None else img.device
    model = SpectreViT(**SMALL, mixer="fft").to(dev).train()
    opt = FusedAdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True)
    return GraphedTrainStep(model, opt, CrossEntropyLoss(), img, labels, autocast_dtype=torch.bfloat16, loader=loader)


class HostFed:
    """the harness's batch assembly (SyntheticCifar.index_batches / batches) in front of a captured step's replay"""

    def __init__(self, images_nchw, labels, batch, step, seed=0):
        self.images, self.labels, self.batch, self.step = images_nchw, labels, batch, step
        self.mean = torch.tensor(CIFAR_MEAN, device=images_nchw.device).view(1, -1, 1, 1)
        self.std = torch.tensor(CIFAR_STD, device=images_nchw.device).view(1, -1, 1, 1)
        self.gen = torch.Generator().manual_seed(seed)
        self.idx, self.at = None, 0

    def batch_of_next_step(self):
        n = self.images.shape[0]
        if self.idx is None or self.at + self.batch > n:
            self.idx, self.at = torch.randperm(n, generator=self.gen).to(self.images.device), 0   # once per epoch
        sel = self.idx[self.at:self.at + self.batch]
        self.at += self.batch
        return (self.images[sel].float() / 255.0 - self.mean) / self.std, self.labels[sel].long()

    def __call__(self):
        img, labels = self.batch_of_next_step()
        self.step.img.copy_(img, non_blocking=True)
        self.step.labels.copy_(labels, non_blocking=True)
        self.step.graph.replay()   # (the step object is closed: its __call__, minus the check)
        shadows.invalidate_weight_shadows()


class ThreeLaunch:
    """the harness's augmented step before the fused fetch (spectre_vit/harness.py train(device_loader=True, augment=True, graph=True)
    with a loader of output "none"): fetch, draw and apply host-issued in front of a captured step's replay"""

    def __init__(self, images_nhwc, loader, aug, step):
        self.images, self.loader, self.aug, self.step = images_nhwc, loader, aug, step

    def batch_of_next_step(self):
        t = self.loader.step
        self.loader.fetch()
        return self.aug(self.images, self.loader.index, step=t), self.loader.labels

    def __call__(self):
        img, labels = self.batch_of_next_step()
        self.step.img.copy_(img, non_blocking=True)
        self.step.labels.copy_(labels, non_blocking=True)
        self.step.graph.replay()   # (the step object is closed: its __call__, minus the check)
        shadows.invalidate_weight_shadows()


def block(run, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--n", type=int, default=50000, help="samples of the resident set (CIFAR's training split)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--augment", action="store_true", help="the augmented step: three host-issued launches + replay against the fused fetch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    images_nhwc = torch.randint(0, 256, (a.n, 32, 32, 3), dtype=torch.uint8, device=dev, generator=g)
    images_nchw = images_nhwc.permute(0, 3, 1, 2).contiguous()   # the layout harness.SyntheticCifar keeps
    labels = torch.randint(0, 100, (a.n,), device=dev, generator=g).to(torch.uint8)
    if a.augment:
        aug = TrainAugment(CIFAR_MEAN, CIFAR_STD, seed=7)
        feeder = ThreeLaunch(images_nhwc, ResidentLoader(images_nhwc, labels, a.batch, seed=42, output="none"), aug, None)
    else:
        feeder = HostFed(images_nchw, labels, a.batch, None)
    img0, lab0 = feeder.batch_of_next_step()
    feeder.step = build(img0, lab0, None)
    feeder.step.close()
    if a.augment:
        loader = ResidentLoader(images_nhwc, labels, a.batch, seed=42, output="augment", augment=aug)
    else:
        loader = ResidentLoader(images_nhwc, labels, a.batch, seed=42)
    fed = build(None, None, loader)
    try:
        for _ in range(a.warmup):
            feeder()
            fed()
        t_host, t_loader = [], []
        for _ in range(a.blocks):   # alternating blocks: drift of the box hits both arms alike
            t_host.append(block(feeder, a.steps))
            t_loader.append(block(fed, a.steps))
        med = statistics.median
        spread = max(t_host) - min(t_host)
        rec = {"workload": f"SpectreViT Small fft, bs {a.batch}, bf16, graph replay, resident set of {a.n}" + (", augmented" if a.augment else ""),
               "arms": {"host_fed": "three_launch", "loader_fed": "fused"} if a.augment else {"host_fed": "host_fed", "loader_fed": "loader_fed"},
               "blocks": a.blocks,
               "steps_per_block": a.steps, "host_fed_ms": med(t_host), "loader_fed_ms": med(t_loader), "host_fed_ms_blocks": t_host,
               "loader_fed_ms_blocks": t_loader, "host_fed_spread_ms": spread, "delta_us": (med(t_loader) - med(t_host)) * 1e3,
               "within_bound": bool(med(t_loader) <= med(t_host) + spread),
               "host_issued_per_step": {"host_fed": "3 launches + 2 copies + 1 replay" if a.augment else "9 launches + 1 replay",
                                        "loader_fed": "1 replay"},
               "loss_host_fed": float(feeder.step.loss.detach()), "loss_loader_fed": float(fed.loss.detach()), "loader_step": loader.step,
               "loader_device_step": loader.device_step()}
    finally:
        fed.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
