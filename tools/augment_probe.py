"""Cost of the on-GPU training augmentation (spectre_vit.augment) at the Small preset (configs/spectre_vit_cifar100.py), bs 512, bf16,
over a CIFAR-sized resident set (50 000 uint8 images):

  * the two kernels alone, spv_augment_params and spv_augment_u8 at B = 512, 3 x 32 x 32 with a shuffled index: HIP-event time of a
    run of back-to-back launches divided by their number (a launch-rate figure when the kernel is shorter than a launch; the kernels'
    own durations come from `rocprofv3 --kernel-trace --stats -- python tools/augment_probe.py --kernels-only`);
  * the harness step -- draw the batch as spectre_vit.harness does, hand it to the graphed training step (GraphedTrainStep:
    forward + loss + backward + FusedAdamW replayed from a HIP graph) -- with augmentation off and on, alternating in one process,
    one pass over the set (97 steps) per window, host clock around a window that ends in a device synchronise.

Prints one JSON line.  Not a bench.py line.  `--pkg DIR` times another checkout's package (its own library, e.g. the parent commit's:
only the `off` windows exist there), so that two builds can alternate inside one GPU job.

`--img-size N` times the kernels on N x N images (the tiled apply path above the LDS kernel's limit; give a `--set-size` that fits
the card: 2048 images of 224 x 224 are 308 MB) and implies `--kernels-only`: the harness windows are the Small preset's.

    python tools/augment_probe.py [--rounds 4] [--kernels-only] [--pkg DIR] [--img-size 224 --set-size 2048]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def event_ms(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def kernels(dev, n_set, bs, img_size=32):
    """HIP-event time per launch of the parameter draw, the apply path(s) this size can take ("lds" and / or "tiled": at 32 both, so
    that the default of "auto" there can be judged) and the yardstick -- the un-augmented batch as the harness makes it from torch ops
    (index gather, cast, divide, subtract, divide) -- beside the byte floor: fp32 output + uint8 source at 6.3 TB/s."""
    import torch
    from spectre_vit import _native, harness
    from spectre_vit.augment import TrainAugment
    g = torch.Generator().manual_seed(0)
    nhwc = torch.randint(0, 256, (n_set, img_size, img_size, 3), generator=g, dtype=torch.uint8).to(dev)
    nchw = nhwc.permute(0, 3, 1, 2).contiguous()
    index = torch.randperm(n_set, generator=g)[:bs].to(dev)
    mean = torch.tensor(harness.CIFAR_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(harness.CIFAR_STD, device=dev).view(1, 3, 1, 1)
    tiled_built = "spv_augment_plan" in _native.SIGNATURES   # False in a --pkg checkout from before the tiled path
    plan = _native.call("spv_augment_plan", 3, img_size, img_size) if tiled_built else 1
    paths = ["tiled"] if plan == 2 else (["lds", "tiled"] if tiled_built else ["lds"])
    kw = lambda k: dict(kernel=k) if tiled_built else {}
    augs = {k: TrainAugment(harness.CIFAR_MEAN, harness.CIFAR_STD, seed=1, **kw(k)) for k in paths}
    auto = TrainAugment(harness.CIFAR_MEAN, harness.CIFAR_STD, seed=1)
    table = auto.draw(bs, 0, height=img_size, width=img_size)
    step = [0]

    def draw():
        step[0] += 1
        auto.draw(bs, step[0], height=img_size, width=img_size)

    fns = [("params_us", draw)]
    fns += [(f"apply_{k}_us", lambda a=a: a(nhwc, index, params=table)) for k, a in augs.items()]
    fns += [("params_and_apply_us", lambda: auto(nhwc, index, step=3)),
            ("torch_ops_unaugmented_us", lambda: (nchw[index].float() / 255.0 - mean) / std)]
    n = 200 if img_size <= 64 else 50
    out = {"img_size": img_size, "paths": paths, "byte_floor_us": round(bs * 3 * img_size * img_size * 5 / 6.3e6, 2)}
    for name, fn in fns:
        event_ms(fn, 10)
        out[name] = [round(1e3 * event_ms(fn, n), 2) for _ in range(3)]
    return out


def harness_windows(dev, n_set, bs, rounds, have_augment):
    import torch
    from spectre_vit import harness
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.optim import FusedAdamW
    c = parse_config("spectre_vit/configs/spectre_vit_cifar100.py")
    data = harness.SyntheticCifar(n_set, c, dev, seed=0)
    torch.manual_seed(0)
    m = harness.build_model(c, mixer="fft", device=dev).train()
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01, capturable=True, static_grads=True)
    gen = torch.Generator().manual_seed(0)
    img0, lab0 = next(iter(data.batches(bs, True, torch.Generator().manual_seed(1))))
    step = GraphedTrainStep(m, opt, CrossEntropyLoss(), img0, lab0.long(), autocast_dtype=torch.bfloat16)
    aug = nhwc = None
    if have_augment:
        from spectre_vit.augment import TrainAugment
        aug = TrainAugment(harness.CIFAR_MEAN, harness.CIFAR_STD, seed=harness.augment_seed(42, 0))
        nhwc = data.images.permute(0, 2, 3, 1).contiguous()
    k = [0]

    def epoch(on):
        """one pass over the set, the batches drawn as harness.train draws them"""
        n = 0
        if on:
            for sel in data.index_batches(bs, True, gen):
                step(aug(nhwc, sel, step=k[0]), data.labels[sel].long())
                k[0] += 1
                n += 1
        else:
            for img, lab in data.batches(bs, True, gen):
                step(img, lab.long())
                n += 1
        return n

    def replay_only():
        for _ in range(n_set // bs):
            step()
        return n_set // bs

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 4)

    try:
        epoch(False)
        if have_augment:
            epoch(True)
        out = {"off_ms_per_step": [], "on_ms_per_step": [], "replay_only_ms_per_step": []}
        for _ in range(rounds):
            out["replay_only_ms_per_step"].append(window(replay_only))
            out["off_ms_per_step"].append(window(lambda: epoch(False)))
            if have_augment:
                out["on_ms_per_step"].append(window(lambda: epoch(True)))
    finally:
        step.close()
    out["steps_per_window"] = n_set // bs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "vit-spectre-experiments_amd"), help="the package directory to time")
    ap.add_argument("--set-size", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--img-size", type=int, default=32, help="side of the images the kernels are timed on (not 32: kernels only)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    os.chdir(os.path.abspath(a.pkg))
    import torch
    try:
        import spectre_vit.augment  # noqa: F401
        have_augment = True
    except ImportError:
        have_augment = False
    assert torch.cuda.is_available(), "augment_probe measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    out = {"pkg": os.path.abspath(a.pkg), "preset": "small", "mixer": "fft", "batch": a.batch, "dtype": "bf16", "graph": True,
           "set_size": a.set_size, "augment_built": have_augment}
    if have_augment:
        out["kernels"] = kernels(dev, a.set_size, a.batch, a.img_size)
    if not a.kernels_only and a.img_size == 32:
        out["harness"] = harness_windows(dev, a.set_size, a.batch, a.rounds, have_augment)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
