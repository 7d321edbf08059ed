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

    python tools/augment_probe.py [--rounds 4] [--kernels-only] [--pkg DIR]
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


def kernels(dev, n_set, bs):
    import torch
    from spectre_vit import harness
    from spectre_vit.augment import TrainAugment
    g = torch.Generator().manual_seed(0)
    nhwc = torch.randint(0, 256, (n_set, 32, 32, 3), generator=g, dtype=torch.uint8).to(dev)
    index = torch.randperm(n_set, generator=g)[:bs].to(dev)
    aug = TrainAugment(harness.CIFAR_MEAN, harness.CIFAR_STD, seed=1)
    table = aug.draw(bs, 0)
    step = [0]

    def draw():
        step[0] += 1
        aug.draw(bs, step[0])

    out = {}
    for name, fn in (("params_us", draw), ("apply_us", lambda: aug(nhwc, index, params=table)),
                     ("params_and_apply_us", lambda: aug(nhwc, index, step=3))):
        event_ms(fn, 20)
        out[name] = [round(1e3 * event_ms(fn, 200), 2) for _ in range(3)]
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
        out["kernels"] = kernels(dev, a.set_size, a.batch)
    if not a.kernels_only:
        out["harness"] = harness_windows(dev, a.set_size, a.batch, a.rounds, have_augment)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
