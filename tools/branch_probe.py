"""SpectreBranch at its shipped preset (configs/spectre_branch.py: 32 x 32, patch 4, E 768, F 256, 4 encoders = 4 conv stages,
100 classes, bs 512) in bf16: ms per training step (forward + spectre_vit.loss.CrossEntropyLoss + backward + FusedAdamW), replayed
from a HIP graph (GraphedTrainStep, capturable FusedAdamW) and eager.  Not a bench.py line.

    python tools/branch_probe.py [batch] [steps]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
import torch  # noqa: E402

from spectre_vit import harness  # noqa: E402
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


def main():
    bs = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    c = parse_config("spectre_vit/configs/spectre_branch.py")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(bs, 3, c.img_size, c.img_size, generator=g).to(dev)
    lab = torch.randint(0, c.num_classes, (bs,), generator=g).to(dev)
    crit = CrossEntropyLoss()

    torch.manual_seed(0)
    m = harness.build_model(c, model="spectre_branch", device=dev).train()
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
    m2 = harness.build_model(c, model="spectre_branch", device=dev).train()
    opt2 = FusedAdamW(m2.parameters(), lr=1e-4, weight_decay=0.01, capturable=True)
    step = GraphedTrainStep(m2, opt2, crit, img, lab, autocast_dtype=torch.bfloat16)
    timed(step, 3)
    t_graph, loss_g = timed(step, n)
    step.close()
    print(f"SpectreBranch preset bs {bs} bf16: graph {t_graph * 1e3:.3f} ms/step ({bs / t_graph:.0f} img/s, loss {loss_g.item():.4f}), "
          f"eager {t_eager * 1e3:.3f} ms/step (loss {loss_e.item():.4f}), max mem {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


if __name__ == "__main__":
    main()
