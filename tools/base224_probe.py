"""BASELINE config 5, student side, for the record: Spectre-ViT-Base (E 768, 12 layers, 12 heads, F 3072, HEAD mixer) at 224 / 16 on one
GPU -- train step (fwd + CE + bwd + FusedAdamW) in bf16, eager and replayed.  Not a bench line (bench.py measures config 2).

    python tools/base224_probe.py [BATCH [MIXER]] [--augment] [--set-size 1024]

--augment: every step draws its batch from a resident uint8 set of 224 x 224 images as the harness does -- windows with the training
transform chain on (spectre_vit.augment.TrainAugment: the tiled apply path) and off (index gather + cast + normalise as torch ops)
alternate in this one process, three windows of ten steps each, and the bare replay is timed beside them."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
import torch  # noqa: E402

from spectre_vit.graph import GraphedTrainStep  # noqa: E402
from spectre_vit.loss import CrossEntropyLoss  # noqa: E402
from spectre_vit.models.spectre.spectre import SpectreViT  # noqa: E402
from spectre_vit.optim import FusedAdamW  # noqa: E402


def window(fn, n=10):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", type=int, nargs="?", default=64)
    ap.add_argument("mixer", nargs="?", default="permut")
    ap.add_argument("--augment", action="store_true", help="time the step with the batch drawn from a uint8 set, augmentation on and off")
    ap.add_argument("--set-size", type=int, default=1024, help="--augment: images in the resident set (150 KB each)")
    a = ap.parse_args()
    bs, mixer = a.batch, a.mixer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = SpectreViT(img_size=224, patch_size=16, in_channels=3, num_classes=100, embed_dim=768, num_encoders=12, num_heads=12,
                   hidden_dim=3072, dropout=0.1, mixer=mixer).to(dev).train()
    img = torch.randn(bs, 3, 224, 224, device=dev)
    lab = torch.randint(0, 100, (bs,), device=dev)
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01, capturable=True, static_grads=True)
    step = GraphedTrainStep(m, opt, CrossEntropyLoss(), img, lab, autocast_dtype=torch.bfloat16)
    for _ in range(3):
        step()
    dt, loss = window(step)
    print(f"Base/224 {mixer} bs {bs}: {dt * 1e3:.2f} ms/step, {bs / dt:.0f} img/s, loss {loss.item():.3f}, "
          f"max mem {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    if a.augment:
        from spectre_vit import harness
        from spectre_vit.augment import TrainAugment
        g = torch.Generator().manual_seed(0)
        nhwc = torch.randint(0, 256, (a.set_size, 224, 224, 3), generator=g, dtype=torch.uint8).to(dev)
        nchw = nhwc.permute(0, 3, 1, 2).contiguous()
        labels = torch.randint(0, 100, (a.set_size,), device=dev)
        mean = torch.tensor(harness.CIFAR_MEAN, device=dev).view(1, 3, 1, 1)
        std = torch.tensor(harness.CIFAR_STD, device=dev).view(1, 3, 1, 1)
        aug = TrainAugment(harness.CIFAR_MEAN, harness.CIFAR_STD, seed=harness.augment_seed(42, 0))
        k = [0]

        def on():
            sel = torch.randperm(a.set_size, generator=g)[:bs].to(dev)
            k[0] += 1
            return step(aug(nhwc, sel, step=k[0]), labels[sel])

        def off():
            sel = torch.randperm(a.set_size, generator=g)[:bs].to(dev)
            return step((nchw[sel].float() / 255.0 - mean) / std, labels[sel])

        on(), off()
        res = {"replay_only": [], "off": [], "on": []}
        for _ in range(3):
            for name, fn in (("replay_only", step), ("off", off), ("on", on)):
                res[name].append(round(window(fn)[0] * 1e3, 3))
        print(f"Base/224 {mixer} bs {bs} ms/step, batch drawn per step from {a.set_size} uint8 images: {res}")
    step.close()


if __name__ == "__main__":
    main()
