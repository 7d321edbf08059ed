"""Cost of the paired-view distillation step (spectre_vit.distillation, csrc/spv_distill.hip) at the Small preset
(configs/spectre_vit_cifar100.py), bs 512, fp32 student (the reference's distillation cell sets use_amp = False), synthetic teacher,
over a CIFAR-sized resident set (50 000 uint8 images).  One mode per process, so that a job can alternate them:

  --mode kernels   spv_teacher_view_u8 at B = 512, 3 x 32 x 32 -> 3 x 224 x 224 (fp32 and bf16, shuffled index) and the yardstick a user
                   of stock torch ops would write on the same device -- F.interpolate(u8.float(), 256, "bicubic"), round, clamp, crop,
                   normalise (NOT Pillow-exact: float bicubic with a = -0.75, one rounding) -- alternating; the fused loss forward +
                   backward against distillation_loss() + autograd at [512, 100].  HIP-event time of a run of back-to-back calls divided
                   by their number; the kernels' own durations and launch counts come from
                   `rocprofv3 --kernel-trace --stats -- python tools/distill_probe.py --mode kernels`.  Where the package has the cached
                   teacher: the indexed loss (the teacher's rows read from a [set, 100] cache through a shuffled index) beside the dense
                   one, and spv_logit_cache_store of one batch.
  --mode eager     the step of harness.train_distill(graph=False): index -> augmented student view + teacher view -> teacher forward ->
                   student forward, fused loss, backward, torch AdamW.
  --mode graph     the same with the student's step replayed by GraphedDistillStep + FusedAdamW.
  --mode cached-eager   the eager step with the teacher's logits resident (TeacherLogitCache, filled before the windows; the fill is
                   timed and reported apart): index -> augmented student view -> student forward, indexed fused loss, backward, AdamW.
                   No teacher view, no teacher forward.
  --mode cached-graph   the same replayed by GraphedDistillStep in cache mode: the augmentation launches, an index copy, one replay.
  --mode parent    the step harness.train(distill=True) runs (also on the parent commit): the teacher sees F.interpolate(img, 64,
                   "bicubic") of the student's own normalised batch -- a 64 x 64 view, 12 times fewer teacher pixels than the 224 view --
                   and the loss is distillation_loss()'s torch-op chain.

The step modes time windows of --steps steps (host clock around a window that ends in a device synchronise) and print every window.
Prints one JSON line.  Not a bench.py line.  `--pkg DIR` times another checkout's package (a package from before the paired-view step
has --mode parent only; one from before the cached teacher lacks the cached modes).

    python tools/distill_probe.py --mode graph [--windows 5] [--steps 97] [--pkg DIR]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def event_us(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(1e3 * a.elapsed_time(b) / n, 2)


def kernels(dev, n_set, bs, rounds):
    import torch
    import torch.nn.functional as F
    from spectre_vit import harness, hip_ops
    from spectre_vit.distillation import TeacherView, distillation_loss
    g = torch.Generator().manual_seed(0)
    nhwc = torch.randint(0, 256, (n_set, 32, 32, 3), generator=g, dtype=torch.uint8).to(dev)
    index = torch.randperm(n_set, generator=g)[:bs].to(dev)
    v32 = TeacherView(harness.CIFAR_MEAN, harness.CIFAR_STD)
    v16 = TeacherView(harness.CIFAR_MEAN, harness.CIFAR_STD, dtype=torch.bfloat16)
    mean = torch.tensor(harness.CIFAR_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(harness.CIFAR_STD, device=dev).view(1, 3, 1, 1)

    def torch_ops():
        x = nhwc[index].permute(0, 3, 1, 2).float()
        x = F.interpolate(x, size=256, mode="bicubic", align_corners=False).round_().clamp_(0, 255)[:, :, 16:240, 16:240]
        return (x / 255.0 - mean) / std

    z = (3 * torch.randn(bs, 100, generator=g)).to(dev).requires_grad_(True)
    t = (3 * torch.randn(bs, 100, generator=g)).to(dev)
    y = torch.randint(0, 100, (bs,), generator=g).to(dev)

    def fused():
        z.grad = None
        hip_ops.distill_loss(z, t, y)[0].backward()

    def chain():
        z.grad = None
        distillation_loss(z, t, y)[0].backward()

    fns = {"teacher_view_fp32_us": lambda: v32(nhwc, index), "teacher_view_bf16_us": lambda: v16(nhwc, index),
           "torch_ops_view_fp32_us": torch_ops, "fused_loss_fwd_bwd_us": fused, "torch_chain_loss_fwd_bwd_us": chain}
    if hasattr(hip_ops, "distill_loss_cached"):
        from spectre_vit.distillation import TeacherLogitCache
        cache = TeacherLogitCache(n_set, 100, dev)
        cache.store(None, (3 * torch.randn(n_set, 100, generator=g)).to(dev))

        def indexed():
            z.grad = None
            hip_ops.distill_loss_cached(z, cache.logits, index, y)[0].backward()

        fns["indexed_loss_fwd_bwd_us"] = indexed
        fns["logit_cache_store_us"] = lambda: cache.store(index, t)
    out = {k: [] for k in fns}
    for fn in fns.values():
        event_us(fn, 5)
    for _ in range(rounds):   # alternating
        for k, fn in fns.items():
            out[k].append(event_us(fn, 20))
    out["teacher_view_bytes"] = {"read": bs * 3072 + 5 * 224 * 4 + 3 * 1024, "write_fp32": bs * 3 * 224 * 224 * 4, "write_bf16": bs * 3 * 224 * 224 * 2}
    return out


def step_windows(dev, mode, n_set, bs, windows, steps):
    import torch
    from torch import nn
    from spectre_vit import harness
    from spectre_vit.augment import TrainAugment
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.distillation import SyntheticTeacher, distillation_loss
    from spectre_vit.dp import GradReducer
    c = parse_config("spectre_vit/configs/spectre_vit_cifar100.py")
    data = harness.SyntheticCifar(n_set, c, dev, seed=0)
    nhwc = data.images.permute(0, 2, 3, 1).contiguous()
    torch.manual_seed(0)
    m = harness.build_model(c, mixer="fft", device=dev).train()
    teacher = SyntheticTeacher(c.num_classes, 384, c.in_channels).to(dev)
    gen = torch.Generator().manual_seed(0)
    aug = TrainAugment(harness.CIFAR_MEAN, harness.CIFAR_STD, seed=harness.augment_seed(42, 0))
    k = [0]
    gstep = None
    extra = {}
    if mode == "parent":
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
        red = GradReducer(m)

        def one(sel):
            img = (data.images[sel].float() / 255.0 - data.mean) / data.std
            label = data.labels[sel]
            logits, _ = m(img, return_features=True)
            with torch.no_grad():
                tl, _ = teacher(nn.functional.interpolate(img, size=64, mode="bicubic"), return_features=True)
            loss, _, _ = distillation_loss(logits, tl, label.long())
            red.zero_grad()
            loss.backward()
            red.finish()
            opt.step()
    else:
        from spectre_vit.distillation import DistillationLoss, TeacherView
        view = TeacherView(harness.CIFAR_MEAN, harness.CIFAR_STD)
        crit = DistillationLoss()

        def views(sel):
            img = aug(nhwc, sel, step=k[0])
            k[0] += 1
            with torch.no_grad():
                tl, _ = teacher(view(nhwc, sel), return_features=True)
            return img, data.labels[sel].long(), tl

        if mode.startswith("cached"):
            from spectre_vit.distillation import TeacherLogitCache
            cache = TeacherLogitCache(n_set, c.num_classes, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = cache.fill(teacher, view, nhwc, batch_size=bs)
            torch.cuda.synchronize()
            extra["fill"] = {"seconds": round(time.perf_counter() - t0, 4), "teacher_batches": calls, "complete": cache.complete(),
                             "cache_bytes": cache.logits.numel() * 4}

            def student_view(sel):
                img = aug(nhwc, sel, step=k[0])
                k[0] += 1
                return img, data.labels[sel].long()

        if mode == "cached-eager":
            opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
            red = GradReducer(m)

            def one(sel):
                img, label = student_view(sel)
                loss = crit(m(img), cache, label, index=sel)
                red.zero_grad()
                loss.backward()
                red.finish()
                opt.step()
        elif mode == "cached-graph":
            from spectre_vit.graph import GraphedDistillStep
            from spectre_vit.optim import FusedAdamW
            opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01, capturable=True, static_grads=True)
            sel0 = next(iter(data.index_batches(bs, True, torch.Generator().manual_seed(1))))
            gstep = GraphedDistillStep(m, opt, crit, *student_view(sel0), autocast_dtype=None, teacher_cache=cache, example_index=sel0)

            def one(sel):
                gstep(*student_view(sel), index=sel)
        elif mode == "eager":
            opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
            red = GradReducer(m)

            def one(sel):
                img, label, tl = views(sel)
                loss = crit(m(img), tl, label)
                red.zero_grad()
                loss.backward()
                red.finish()
                opt.step()
        else:
            from spectre_vit.graph import GraphedDistillStep
            from spectre_vit.optim import FusedAdamW
            opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01, capturable=True, static_grads=True)
            sel0 = next(iter(data.index_batches(bs, True, torch.Generator().manual_seed(1))))
            gstep = GraphedDistillStep(m, opt, crit, *views(sel0), autocast_dtype=None)

            def one(sel):
                gstep(*views(sel))

    def window():
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while n < steps:
            for sel in data.index_batches(bs, True, gen):
                one(sel)
                n += 1
                if n >= steps:
                    break
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / n, 4)

    try:
        window()
        return dict({"ms_per_step": [window() for _ in range(windows)], "steps_per_window": steps}, **extra)
    finally:
        if gstep is not None:
            gstep.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "eager", "graph", "cached-eager", "cached-graph", "parent"), default="kernels")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=97)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "vit-spectre-experiments_amd"), help="the package directory to time")
    ap.add_argument("--set-size", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=512)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    os.chdir(os.path.abspath(a.pkg))
    import torch
    assert torch.cuda.is_available(), "distill_probe measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    out = {"pkg": os.path.abspath(a.pkg), "mode": a.mode, "preset": "small", "mixer": "fft", "batch": a.batch, "student_dtype": "fp32",
           "set_size": a.set_size}
    if a.mode == "kernels":
        out["kernels"] = kernels(dev, a.set_size, a.batch, a.rounds)
    else:
        out["step"] = step_windows(dev, a.mode, a.set_size, a.batch, a.windows, a.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
