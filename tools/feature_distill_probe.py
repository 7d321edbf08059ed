"""Timing probe of the feature-matching term ("feature term"), MI355X:

  pair   the forward + backward launch pair of hip_ops.feature_cosine against the torch-op sequence of the reference's three lines
         (two F.normalize, nn.CosineSimilarity, mean, 1 -) with autograd, at (512, 512) and (64, 768), fp32
  step   the graph-replayed cached distillation step (GraphedDistillStep, Small student, batch 512) with the term on against the same
         step with it off

Both arms of a comparison alternate inside one process; each round is a device-event bracket around `iters` calls behind a warm-up, and
the medians of the rounds are reported.  One JSON document on stdout and, with --out, in a file.

    python tools/feature_distill_probe.py --out profiles/feature_distill_v1_probe.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vit-spectre-experiments_amd"), ROOT]


def bracket(fn, iters, warm=10):
    """microseconds per call of fn over `iters` calls"""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def pair(rows, width, rounds, iters):
    from spectre_vit import hip_ops
    d = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(rows + width)
    s = torch.randn(rows, width, generator=g).to(d).requires_grad_(True)
    t = torch.randn(rows, width, generator=g).to(d)
    one = torch.ones((), device=d)
    cos = torch.nn.CosineSimilarity()

    def fused():
        s.grad = None
        hip_ops.feature_cosine(s, t, 0.5)[0].backward(one)

    def stock():
        s.grad = None
        a, b = torch.nn.functional.normalize(s, dim=-1), torch.nn.functional.normalize(t, dim=-1)
        ((1 - cos(a, b).mean()) * 0.5).backward(one)

    fused()
    gf = s.grad.clone()
    stock()
    diff = float((gf - s.grad).abs().max() / s.grad.abs().max())
    f, k = [], []
    for _ in range(rounds):
        f.append(bracket(fused, iters))
        k.append(bracket(stock, iters))
    return dict(rows=rows, width=width, fused_us=f, torch_us=k, fused_median_us=statistics.median(f), torch_median_us=statistics.median(k),
                gradient_rel_diff=diff)


def step(rounds, iters, batch=512, n=2048):
    from spectre_vit.distillation import DistillationLoss, TeacherLogitCache
    from spectre_vit.graph import GraphedDistillStep
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    d = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(7)
    img = torch.randn(batch, 3, 32, 32, generator=g).to(d)
    lab = torch.randint(0, 100, (batch,), generator=g).to(d)
    idx = torch.randperm(n, generator=g)[:batch].to(d)
    cache = TeacherLogitCache(n, 100, d, feature_dim=512)
    cache.store(None, (3 * torch.randn(n, 100, generator=g)).to(d), torch.randn(n, 512, generator=g).to(d))

    def arm(w):
        torch.manual_seed(11)
        m = SpectreViT(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=512, num_encoders=4, num_heads=16,
                       hidden_dim=768, activation="gelu", dropout=0.0, mixer="fft").to(d).train()
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True)
        s = GraphedDistillStep(m, opt, DistillationLoss(feature_loss_weight=w), img, lab, autocast_dtype=torch.bfloat16, warmup=2,
                               teacher_cache=cache, example_index=idx)
        try:
            return bracket(lambda: s(img, lab, index=idx), iters)
        finally:
            s.close()

    on, off = [], []
    for _ in range(rounds):
        on.append(arm(0.5))
        off.append(arm(0.0))
    return dict(batch=batch, on_us=on, off_us=off, on_median_us=statistics.median(on), off_median_us=statistics.median(off))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs an MI355X"
    res = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters,
               pair=[pair(512, 512, a.rounds, a.iters), pair(64, 768, a.rounds, a.iters)], step=step(a.rounds, a.step_iters))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
