#!/usr/bin/env python3
"""The Walsh-Hadamard mixer next to the FFT mixer, kernel by kernel and step by step, in ONE process on one build.  

    kernels   spv_hadamard_ln_fwd / _bwd and spv_fnet_ln_fwd / _bwd at (512, 65, 512) bf16; the row-0 pair of each
              (spv_hadamard_cls_* / spv_fnet_cls_*) at the same shape.  Each kernel is captured as a graph of --launches back-to-back
              launches on the same buffers; a graph replay's time over --launches is the kernel's time under back-to-back issue.
    steps     the graph-replayed Small / CIFAR-100 bs-512 training step of bench.py (bf16 autocast, FusedAdamW(static_grads=True)) for
              mixer="hadamard" and mixer="fft".

Every side is timed in alternating windows, round by round (>= 20 warm-up replays, rounds * per-round >= 100 timed replays per side,
device events, median and min / max over the rounds), so a drift of the box hits both mixers alike.  One JSON line.

    python tools/hadamard_probe.py [--rounds 10] [--per-round 20] [--out profiles/hadamard_v1_probe.json]

Only one graph-replayed step may own the library's dropout seed word, so the first step object is closed after its capture and its
graph replayed directly (as tools/ema_probe.py does): no launch and no byte moved changes.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import SMALL  # noqa: E402
from spectre_vit import _native, hip_ops  # noqa: E402
from spectre_vit.graph import GraphedTrainStep  # noqa: E402
from spectre_vit.loss import CrossEntropyLoss  # noqa: E402
from spectre_vit.models.spectre.spectre import SpectreViT  # noqa: E402
from spectre_vit.optim import FusedAdamW  # noqa: E402

B, N, D = 512, 65, 512


def timed(graph, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def kernel_graphs(dev, launches):
    """name -> graph of `launches` launches of one entry point at (B, N, D) bf16"""
    bf, f32 = torch.bfloat16, torch.float32
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, N, D, generator=g).to(dev, bf)
    dout = torch.randn(B, N, D, generator=g).to(dev, bf)
    g1 = torch.randn(B, D, generator=g).to(dev, bf)
    gamma, beta = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)
    pre, out, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(B * N, device=dev, dtype=f32), torch.empty(B * N, device=dev, dtype=f32)
    out0, m0 = torch.empty(B, D, device=dev, dtype=bf), torch.empty(B, D, device=dev, dtype=f32)
    mean0, rstd0 = torch.empty(B, device=dev, dtype=f32), torch.empty(B, device=dev, dtype=f32)
    dg, db = torch.empty(D, device=dev, dtype=f32), torch.empty(D, device=dev, dtype=f32)
    partials = torch.empty(B * 2 * D, device=dev, dtype=f32)
    tw = hip_ops._fnet_twiddle(N, dev)
    s = hip_ops.hadamard_scale(N, D)
    p, call = hip_ops._p, _native.call
    keep = [x, dout, g1, gamma, beta, pre, out, dx, mean, rstd, out0, m0, mean0, rstd0, dg, db, partials, tw]

    def st():
        return hip_ops._stream()

    # every backward reads the prenorm / m0 and statistics its own forward left: forward first, in the table's order
    sides = {
        "hadamard_ln_fwd": lambda: call("spv_hadamard_ln_fwd", p(x), p(pre), p(out), p(gamma), p(beta), p(mean), p(rstd), s, B, N, D, 1, st()),
        "hadamard_ln_bwd": lambda: call("spv_hadamard_ln_bwd", p(dout), p(pre), p(mean), p(rstd), p(gamma), p(dx), 0, 0, p(partials), s, B, N, D, 1,
                                        st()),
        "hadamard_cls_fwd": lambda: call("spv_hadamard_cls_fwd", p(x), p(gamma), p(beta), p(out0), p(m0), p(mean0), p(rstd0), s, B, N, D, 1, st()),
        "hadamard_cls_bwd": lambda: call("spv_hadamard_cls_bwd", p(g1), p(m0), p(mean0), p(rstd0), p(gamma), p(dx), p(partials), s, B, N, D, 1, st()),
        "fnet_ln_fwd": lambda: call("spv_fnet_ln_fwd", p(x), p(pre), p(out), p(gamma), p(beta), p(mean), p(rstd), p(tw), B, N, D, 1, st()),
        "fnet_ln_bwd": lambda: call("spv_fnet_ln_bwd", p(dout), p(pre), p(mean), p(rstd), p(gamma), p(dx), 0, 0, p(partials), p(tw), B, N, D, 1, st()),
        "fnet_cls_fwd": lambda: call("spv_fnet_cls_fwd", p(x), p(gamma), p(beta), p(out0), p(m0), p(mean0), p(rstd0), B, N, D, 1, st()),
        "fnet_cls_bwd": lambda: call("spv_fnet_cls_bwd", p(g1), p(m0), p(mean0), p(rstd0), p(gamma), p(dx), p(partials), B, N, D, 1, st()),
    }
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in sides.items():
        with torch.cuda.stream(side):
            fn()   # load the code object, leave valid forward outputs for the backward that follows
        side.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            for _ in range(launches):
                fn()
        graphs[name] = gr
    return graphs, keep


def build_step(mixer, img, labels):
    torch.manual_seed(0)
    model = SpectreViT(**SMALL, mixer=mixer).to(img.device).train()
    opt = FusedAdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True)
    return model, GraphedTrainStep(model, opt, CrossEntropyLoss(), img, labels, autocast_dtype=torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per-round", type=int, default=20, help="replays per timed window; rounds * per-round >= 100 timed replays per side")
    ap.add_argument("--launches", type=int, default=10, help="launches of one kernel per graph")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    med = statistics.median
    rec = {"shape": [B, N, D], "dtype": "bf16", "rounds": a.rounds, "replays_per_round": a.per_round, "launches_per_graph": a.launches,
           "bytes_ln": 3 * B * N * D * 2, "bytes_cls": B * (N + 1) * D * 2}

    graphs, keep = kernel_graphs(dev, a.launches)
    for _ in range(a.warmup):
        for gr in graphs.values():
            gr.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, gr in graphs.items():
            times[k].append(timed(gr, a.per_round) / a.launches * 1e3)
    rec["kernel_us"] = {k: med(v) for k, v in times.items()}
    rec["kernel_us_min_max"] = {k: [min(v), max(v)] for k, v in times.items()}
    rec["kernel_gbps"] = {k: (rec["bytes_cls"] if "cls" in k else rec["bytes_ln"]) / (med(v) * 1e-6) / 1e9 for k, v in times.items()}
    del graphs, keep

    g = torch.Generator().manual_seed(0)
    img = torch.randn(B, 3, 32, 32, generator=g).to(dev)
    labels = torch.randint(0, 100, (B,), generator=g).to(dev)
    _, fft = build_step("fft", img, labels)
    fft.close()
    _, had = build_step("hadamard", img, labels)
    try:
        for _ in range(a.warmup):
            fft.graph.replay()
            had.graph.replay()
        torch.cuda.synchronize()
        t_fft, t_had = [], []
        for _ in range(a.rounds):
            t_fft.append(timed(fft.graph, a.per_round))
            t_had.append(timed(had.graph, a.per_round))
        rec.update(workload=f"SpectreViT Small, bs {B}, bf16, graph replay", step_fft_ms=med(t_fft), step_hadamard_ms=med(t_had),
                   step_fft_ms_min_max=[min(t_fft), max(t_fft)], step_hadamard_ms_min_max=[min(t_had), max(t_had)],
                   step_delta_us=(med(t_had) - med(t_fft)) * 1e3, loss_fft=float(fft.loss), loss_hadamard=float(had.loss))
    finally:
        had.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
