"""SpectreViT(mixer="attention") at the Small preset (configs/spectre_vit_cifar100.py: 32 x 32, patch 4, E 512, 16 heads, 4 encoders,
100 classes) at bs 512 in bf16: ms per training step (forward + spectre_vit.loss.CrossEntropyLoss + backward + FusedAdamW), replayed
from a HIP graph (GraphedTrainStep) and eager, each with the last layer at the CLS rows only (the default,
hip_ops.LAST_LAYER_CLS_ONLY: the row-0 attention kernels) and over every row.  Prints one JSON line.  Not a bench.py line.

    python tools/attn_mixer_probe.py [batch] [steps]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
import torch  # noqa: E402

from spectre_vit import harness, hip_ops  # noqa: E402
from spectre_vit.configs.parser import parse_config  # noqa: E402
from spectre_vit.graph import GraphedTrainStep  # noqa: E402
from spectre_vit.loss import CrossEntropyLoss  # noqa: E402
from spectre_vit.optim import FusedAdamW  # noqa: E402


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, loss


def run(c, img, lab, n, cls_only):
    hip_ops.LAST_LAYER_CLS_ONLY = cls_only
    dev = img.device
    crit = CrossEntropyLoss()
    torch.manual_seed(0)
    m = harness.build_model(c, mixer="attention", device=dev).train()
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01, capturable=True)

    def eager():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(img)
        loss = crit(out, lab)
        loss.backward()
        opt.step()
        return loss

    timed(eager, 3)
    t_eager, loss_e = timed(eager, n)
    torch.manual_seed(0)
    m2 = harness.build_model(c, mixer="attention", device=dev).train()
    opt2 = FusedAdamW(m2.parameters(), lr=1e-4, weight_decay=0.01, capturable=True, static_grads=True)
    step = GraphedTrainStep(m2, opt2, crit, img, lab, autocast_dtype=torch.bfloat16)
    try:
        timed(step, 3)
        t_graph, loss_g = timed(step, n)
    finally:
        step.close()
    return dict(graph_ms=round(t_graph * 1e3, 3), eager_ms=round(t_eager * 1e3, 3), graph_loss=round(loss_g.item(), 4),
                eager_loss=round(loss_e.item(), 4))


def main():
    bs = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    c = parse_config("spectre_vit/configs/spectre_vit_cifar100.py")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(bs, 3, c.img_size, c.img_size, generator=g).to(dev)
    lab = torch.randint(0, c.num_classes, (bs,), generator=g).to(dev)
    keep = hip_ops.LAST_LAYER_CLS_ONLY
    try:
        out = {"model": "SpectreViT", "mixer": "attention", "preset": "small", "batch": bs, "dtype": "bf16", "steps": n,
               "cls_only_last_layer": run(c, img, lab, n, True), "every_row_last_layer": run(c, img, lab, n, False)}
    finally:
        hip_ops.LAST_LAYER_CLS_ONLY = keep
    out["max_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
