#!/usr/bin/env python3
"""What do the fused tiled fetch and the loader-fed distillation step cost or save?  

One process, one build, both sides of every comparison alternating; the parent's own path is timed TWICE in every comparison (arms
`parent_a` and `parent_b`), and the spread between its two medians is the margin the new path is held to.  For the steps the two
parent arms are two separately built and captured host-fed steps: two captures of one model differ in where their buffers lie, and
the loader-fed step is a third capture.

    calls    spv_loader_fetch_augment_tiled against the three calls it replaces (spv_loader_fetch mode none, spv_augment_params,
             spv_augment_tiled_u8) at 3 x 64 x 64, B = 512 and 3 x 224 x 224, B = 64: HIP events round each side, per iteration
             parent_a, fused, parent_b; median of --iters after --warmup.
    step     the graph-replayed training step, loader-fed (GraphedTrainStep(loader=ResidentLoader(output="augment_tiled")): one
             replay) against the parent's host-fed step (mode-none fetch, draw, apply, two copies, the replay): the 64-pixel config of
             tests/test_gpu_augment_tiled.py at bs 128 and, with --base224, the Base/224 student of tools/base224_probe.py at bs 64.
             Host clock round blocks of --steps steps that begin and end in a device synchronise; per round parent_a, fused, parent_b.
    distill  GraphedDistillStep in cache mode on the CIFAR preset (bench.py SMALL, fft, bs 512): loader-fed (one replay) against
             host-fed as harness.train_distill(graph=True, cache_teacher=True) feeds it (index slice of an uploaded randperm, label
             gather, draw, apply, three copies, the replay).  Blocks as for `step`.

Only one graph-replayed step may own the library's dropout seed word, so the host-fed step object is closed after its capture and its
graph replayed directly (tools/loader_probe.py): its dropout kernels then read the loader-fed step's seed word, which changes no
launch and no byte moved.  One JSON line.

    python tools/loader_tiled_probe.py [--only calls,step,distill] [--base224] [--out FILE]
"""
import argparse
import ctypes
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
from spectre_vit import _native, shadows  # noqa: E402
from spectre_vit.augment import TrainAugment  # noqa: E402
from spectre_vit.data import CIFAR_MEAN, CIFAR_STD, ResidentLoader  # noqa: E402
from spectre_vit.distillation import DistillationLoss, TeacherLogitCache  # noqa: E402
from spectre_vit.graph import GraphedDistillStep, GraphedTrainStep  # noqa: E402
from spectre_vit.loss import CrossEntropyLoss  # noqa: E402
from spectre_vit.models.spectre.spectre import SpectreViT  # noqa: E402
from spectre_vit.optim import FusedAdamW  # noqa: E402

PX64 = dict(img_size=64, patch_size=8, in_channels=3, num_classes=100, embed_dim=512, num_encoders=2, num_heads=16, hidden_dim=768,
            dropout=0.001, activation="gelu")
BASE224 = dict(img_size=224, patch_size=16, in_channels=3, num_classes=100, embed_dim=768, num_encoders=12, num_heads=12, hidden_dim=3072,
               dropout=0.1)
med = statistics.median


def resident_set(n, side, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (n, side, side, 3), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.randint(0, 100, (n,), device=dev, generator=g).to(torch.uint8)
    return images, labels


def summary(arms):
    """arms: name -> list of times.  The fused arm against the parent's two runs."""
    m = {k: med(v) for k, v in arms.items()}
    parent = 0.5 * (m["parent_a"] + m["parent_b"])
    spread = abs(m["parent_a"] - m["parent_b"])
    return dict(median=m, parent_spread=spread, fused_minus_parent=m["fused"] - parent, within_bound=bool(m["fused"] <= max(m["parent_a"], m["parent_b"])),
                min={k: min(v) for k, v in arms.items()}, max={k: max(v) for k, v in arms.items()})


# ---------------------------------------------------------------- the call against the three calls
def probe_calls(dev, side, batch, n, warmup, iters):
    images, labels = resident_set(n, side, dev)
    aug = TrainAugment(CIFAR_MEAN, CIFAR_STD, seed=7, kernel="tiled")
    fused = ResidentLoader(images, labels, batch, seed=42, output="augment_tiled", augment=aug)
    none_a, none_b = (ResidentLoader(images, labels, batch, seed=42, output="none") for _ in range(2))   # the three arms stay in step
    # the parent's three calls as TrainAugment issues them, on buffers allocated once (the allocator is not what is measured)
    cfg = aug.cfg()
    mean, inv_std = aug.norm(dev)
    params = torch.empty((batch, 16), dtype=torch.float32, device=dev)
    out = torch.empty((batch, 3, side, side), dtype=torch.float32, device=dev)
    ws = torch.empty(_native.call("spv_augment_tiled_ws_bytes", batch, side, side), dtype=torch.uint8, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def three(none):
        t = none.step
        none.fetch()
        _native.call("spv_augment_params", params.data_ptr(), batch, 3, side, side, ctypes.addressof(cfg), aug.seed, t, stream())
        _native.call("spv_augment_tiled_u8", images.data_ptr(), none.index.data_ptr(), params.data_ptr(), mean.data_ptr(), inv_std.data_ptr(),
                     out.data_ptr(), batch, n, 3, side, side, ws.data_ptr(), ws.numel(), stream())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1
    arms = dict(parent_a=[], fused=[], parent_b=[])
    events = []
    for it in range(warmup + iters):
        row = (timed(lambda: three(none_a)), timed(fused.fetch), timed(lambda: three(none_b)))
        if it >= warmup:
            events.append(row)
    torch.cuda.synchronize()
    for row in events:
        for name, (e0, e1) in zip(arms, row):
            arms[name].append(e0.elapsed_time(e1) * 1e3)
    assert bool((fused.img.view(torch.int32) == out.view(torch.int32)).all()), "the two sides fetched the same step: the same bits"
    return dict(shape=[3, side, side], batch=batch, n=n, unit="us", iters=iters, warmup=warmup, **summary(arms))


# ---------------------------------------------------------------- the graph-replayed steps
class HostFedTrain:
    """the parent's augmented step at the tiled sizes: fetch (mode none), draw and apply host-issued, two copies, the replay"""

    def __init__(self, images, loader, aug):
        self.images, self.loader, self.aug, self.step = images, loader, aug, None

    def batch(self):
        t = self.loader.step
        self.loader.fetch()
        return self.aug(self.images, self.loader.index, step=t), self.loader.labels

    def __call__(self):
        img, labels = self.batch()
        self.step.img.copy_(img, non_blocking=True)
        self.step.labels.copy_(labels, non_blocking=True)
        self.step.graph.replay()   # (the step object is closed: its __call__, minus the check)
        shadows.invalidate_weight_shadows()


class HostFedDistill:
    """harness.train_distill(graph=True, cache_teacher=True) without the loader: the index slice of a randperm uploaded once per epoch,
    the label gather, draw and apply, three copies, the replay"""

    def __init__(self, images, labels, batch, aug):
        self.images, self.labels, self.batch_size, self.aug, self.step = images, labels, batch, aug, None
        self.gen = torch.Generator().manual_seed(0)
        self.idx, self.at, self.t = None, 0, 0

    def batch(self):
        n = self.images.shape[0]
        if self.idx is None or self.at + self.batch_size > n:
            self.idx, self.at = torch.randperm(n, generator=self.gen).to(self.images.device), 0
        sel = self.idx[self.at:self.at + self.batch_size]
        self.at += self.batch_size
        self.t += 1
        return self.aug(self.images, sel, step=self.t - 1), self.labels[sel].long(), sel

    def __call__(self):
        img, labels, sel = self.batch()
        self.step.img.copy_(img, non_blocking=True)
        self.step.labels.copy_(labels, non_blocking=True)
        self.step.index.copy_(sel, non_blocking=True)
        self.step.graph.replay()
        shadows.invalidate_weight_shadows()


def block(run, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def time_steps(feeder_a, feeder_b, fed, warmup, blocks, steps):
    for _ in range(warmup):
        feeder_a()
        fed()
        feeder_b()
    arms = dict(parent_a=[], fused=[], parent_b=[])
    for _ in range(blocks):
        arms["parent_a"].append(block(feeder_a, steps))
        arms["fused"].append(block(fed, steps))
        arms["parent_b"].append(block(feeder_b, steps))
    return dict(unit="ms", blocks=blocks, steps_per_block=steps, warmup=warmup, **summary(arms))


def probe_step(dev, cfg, mixer, batch, n, warmup, blocks, steps, lr):
    side = cfg["img_size"]
    images, labels = resident_set(n, side, dev)
    aug = TrainAugment(CIFAR_MEAN, CIFAR_STD, seed=7)

    def build(img, lab, loader):
        torch.manual_seed(0)
        model = SpectreViT(**cfg, mixer=mixer).to(dev).train()
        opt = FusedAdamW(model.parameters(), lr=lr, weight_decay=0.01, capturable=True, static_grads=True)
        return GraphedTrainStep(model, opt, CrossEntropyLoss(), img, lab, autocast_dtype=torch.bfloat16, loader=loader)
    feeders = []
    for _ in range(2):
        feeder = HostFedTrain(images, ResidentLoader(images, labels, batch, seed=42, output="none"), aug)
        img0, lab0 = feeder.batch()
        feeder.step = build(img0, lab0, None)
        feeder.step.close()
        feeders.append(feeder)
    loader = ResidentLoader(images, labels, batch, seed=42, output="augment_tiled", augment=aug)
    fed = build(None, None, loader)
    try:
        rec = time_steps(feeders[0], feeders[1], fed, warmup, blocks, steps)
        rec.update(workload=f"SpectreViT {cfg['embed_dim']}x{cfg['num_encoders']} {mixer} at {side}/{cfg['patch_size']}, bs {batch}, bf16, "
                            f"graph replay, augmented, resident set of {n}",
                   host_issued_per_step={"parent": "4 launches + 2 copies + 1 replay", "fused": "1 replay"},
                   loss_parent=float(feeder.step.loss.detach()), loss_fused=float(fed.loss.detach()), loader_step=loader.step,
                   loader_device_step=loader.device_step())
    finally:
        fed.close()
    return rec


def probe_distill(dev, batch, n, warmup, blocks, steps):
    images, labels = resident_set(n, 32, dev)
    aug = TrainAugment(CIFAR_MEAN, CIFAR_STD, seed=7)
    cache = TeacherLogitCache(n, 100, dev)
    cache.store(None, torch.randn(n, 100, generator=torch.Generator().manual_seed(1)).to(dev))

    def build(img, lab, idx, loader):
        torch.manual_seed(0)
        model = SpectreViT(**SMALL, mixer="fft").to(dev).train()
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True)
        kw = dict(loader=loader) if loader is not None else dict(example_index=idx)
        return GraphedDistillStep(model, opt, DistillationLoss(), img, lab, teacher_cache=cache, **kw)
    feeders = []
    for _ in range(2):
        feeder = HostFedDistill(images, labels, batch, aug)
        img0, lab0, idx0 = feeder.batch()
        feeder.step = build(img0, lab0, idx0, None)
        feeder.step.close()
        feeders.append(feeder)
    loader = ResidentLoader(images, labels, batch, seed=42, output="augment", augment=aug)
    fed = build(None, None, None, loader)
    try:
        rec = time_steps(feeders[0], feeders[1], fed, warmup, blocks, steps)
        rec.update(workload=f"SpectreViT Small fft, bs {batch}, fp32, GraphedDistillStep in cache mode, augmented, resident set of {n}",
                   host_issued_per_step={"parent": "slice + gather + cast + 2 launches + 3 copies + 1 replay", "fused": "1 replay"},
                   loss_parent=float(feeder.step.loss.detach()), loss_fused=float(fed.loss.detach()), loader_step=loader.step,
                   loader_device_step=loader.device_step())
    finally:
        fed.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="calls,step,distill")
    ap.add_argument("--base224", action="store_true", help="step: also the Base/224 student (12 layers of 768) at bs 64")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=120, help="calls: timed iterations")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100, help="step / distill: steps per timed block")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    only = set(a.only.split(","))
    rec = {}
    if "calls" in only:
        rec["calls"] = [probe_calls(dev, 64, 512, 8192, a.warmup, a.iters), probe_calls(dev, 224, 64, 1024, a.warmup, a.iters)]
    if "step" in only:
        rec["step"] = [probe_step(dev, PX64, "fft", 128, 8192, a.warmup, a.blocks, a.steps, 1e-3)]
        if a.base224:
            rec["step"].append(probe_step(dev, BASE224, "permut", 64, 1024, a.warmup, a.blocks, max(a.steps // 4, 10), 1e-4))
    if "distill" in only:
        rec["distill"] = probe_distill(dev, 512, 50000, a.warmup, a.blocks, a.steps)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
