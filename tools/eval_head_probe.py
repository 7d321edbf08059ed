#!/usr/bin/env python3
"""The end of a validation batch at (512, 100) fp32 logits, two ways, for a `rocprofv3 --kernel-trace --stats` run of each:

    --mode torch    the ops of the harness's eager validation loop: argmax, ==, sum, accumulate; the cross-entropy kernel, the
                    sample weighting, accumulate  (spectre_vit/harness.py, graph_eval=False)
    --mode kernel   ONE spv_eval_head launch (hip_ops.eval_head)

Without a profiler it prints the mean time per batch end from HIP events.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
import torch  # noqa: E402

from spectre_vit import hip_ops  # noqa: E402
from spectre_vit.loss import CrossEntropyLoss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["torch", "kernel"])
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    z = torch.randn(a.rows, a.classes, generator=g).to(dev)
    label = torch.randint(0, a.classes, (a.rows,), generator=g).to(torch.uint8 if a.classes <= 256 else torch.int64).to(dev)
    criterion = CrossEntropyLoss()
    v_correct = torch.zeros((), device=dev, dtype=torch.int64)
    v_loss = torch.zeros((), device=dev)
    stats = hip_ops.eval_head_stats(dev)
    pred = torch.zeros(a.rows, dtype=torch.int64, device=dev)
    labels64 = label.long()
    n_valid = torch.full((1,), a.rows, dtype=torch.int32, device=dev)

    def torch_end():
        nonlocal v_correct, v_loss
        with torch.no_grad():
            v_correct += (label == torch.argmax(z, dim=1)).sum()
            v_loss += criterion(z, label.long()) * label.size(0)

    def kernel_end():
        hip_ops.eval_head(z, labels64, n_valid, pred, stats, 5)

    fn = torch_end if a.mode == "torch" else kernel_end
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"mode": a.mode, "rows": a.rows, "classes": a.classes, "iters": a.iters + 10,
                      "us_per_batch_end": round(e0.elapsed_time(e1) / a.iters * 1e3, 2)}))


if __name__ == "__main__":
    main()
