#!/usr/bin/env python3
"""The global-filter mixer measured on one box and one build.  

    --mode kernels   launches spv_gfilter_fwd / _bwd (the fast path: gfilter_fast_kernel<0> / <1>) and, beside them, spv_fnet_ln_fwd /
                     _bwd (fnet_mfma_kernel<1> / <2>) at (512, 65, 512) bf16, --launches times each after a warm-up launch.  Prints nothing to time: it is the program a
                     profiler runs.
    --mode profile   starts `rocprofv3 --kernel-trace --stats` on a child process in --mode kernels (a run of its own, nothing else
                     traced), reads its kernel_stats.csv and reports each kernel's average time, the HBM floor of the 2 B N D 2-byte
                     payload at the float4 copy rate this project measured (6.29 TB/s) and the share of that rate each kernel reaches.
    --mode steps     the graph-replayed Small / CIFAR-100 bs-512 training step (bf16 autocast, FusedAdamW(static_grads=True)) for
                     mixer="filter", "fft" and "attention": alternating windows in one process, medians and min / max over the rounds.

    python tools/gfilter_probe.py --mode profile --out profiles/gfilter_v1_kernels.json
    python tools/gfilter_probe.py --mode steps --out profiles/gfilter_v1_steps.json

Only one graph-replayed step may own the library's dropout seed word, so every step object but the last is closed after its capture
and its graph replayed directly (as tools/hadamard_probe.py does): no launch and no byte moved changes.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
sys.path.insert(0, ROOT)

B, N, D = 512, 65, 512
COPY_TBPS = 6.29   # the float4 copy rate measured on this hardware
KERNELS = ("gfilter_fast_kernel<0>", "gfilter_fast_kernel<1>", "gfilter_fold_kernel", "fnet_mfma_kernel<1>", "fnet_mfma_kernel<2>")


def run_kernels(launches):
    import torch
    from spectre_vit import _native, hip_ops
    dev = torch.device("cuda:0")
    bf, f32 = torch.bfloat16, torch.float32
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, N, D, generator=g).to(dev, bf)
    dy = torch.randn(B, N, D, generator=g).to(dev, bf)
    w = torch.randn(N // 2 + 1, D, 2, generator=g).to(dev)
    gamma, beta = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)
    y, dx, pre, out = (torch.empty_like(x) for _ in range(4))
    dw = torch.empty_like(w)
    mean, rstd = torch.empty(B * N, device=dev, dtype=f32), torch.empty(B * N, device=dev, dtype=f32)
    parts = torch.empty(_native.call("spv_gfilter_partial_floats", B, N, D), device=dev, dtype=f32)
    ln_parts = torch.empty(B * 2 * D, device=dev, dtype=f32)
    tab, tw = hip_ops.gfilter_tables(N, dev), hip_ops._fnet_twiddle(N, dev)
    p, call, st = hip_ops._p, _native.call, hip_ops._stream
    sides = [lambda: call("spv_gfilter_fwd", p(x), p(w), p(y), p(tab), B, N, D, 1, 0, st()),
             lambda: call("spv_gfilter_bwd", p(x), p(dy), p(w), p(dx), p(dw), p(tab), p(parts), B, N, D, 1, 0, st()),
             lambda: call("spv_fnet_ln_fwd", p(x), p(pre), p(out), p(gamma), p(beta), p(mean), p(rstd), p(tw), B, N, D, 1, st()),
             lambda: call("spv_fnet_ln_bwd", p(dy), p(pre), p(mean), p(rstd), p(gamma), p(dx), 0, 0, p(ln_parts), p(tw), B, N, D, 1, st())]
    for fn in sides:
        for _ in range(launches + 1):
            fn()
        torch.cuda.synchronize()


def profile(launches):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "gfilter", "--",
               sys.executable, os.path.abspath(__file__), "--mode", "kernels", "--launches", str(launches)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(found[0])))
    payload = 2 * B * N * D * 2
    floor_us = payload / (COPY_TBPS * 1e12) * 1e6
    rec = {"shape": [B, N, D], "dtype": "bf16", "launches": launches, "payload_bytes": payload, "copy_rate_TBps": COPY_TBPS,
           "hbm_floor_us": floor_us, "kernel_us": {}, "calls": {}}
    for r in rows:
        for k in KERNELS:
            if k in r["Name"]:
                rec["kernel_us"][k] = float(r["AverageNs"]) / 1e3
                rec["calls"][k] = int(r["Calls"])
    ku = rec["kernel_us"]
    # floor time over kernel time = the share of the copy rate the kernel reaches
    if "gfilter_fast_kernel<0>" in ku:
        rec["fwd_share_of_copy_rate"] = floor_us / ku["gfilter_fast_kernel<0>"]
    if "gfilter_fast_kernel<1>" in ku:   # the backward's payload: x and dy in, dx out
        rec["bwd_share_of_copy_rate"] = 1.5 * floor_us / (ku["gfilter_fast_kernel<1>"] + ku.get("gfilter_fold_kernel", 0.0))
    return rec


def timed(graph, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def steps(warmup, rounds, per_round):
    import torch
    from bench import SMALL
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(B, 3, 32, 32, generator=g).to(dev)
    labels = torch.randint(0, 100, (B,), generator=g).to(dev)
    mixers = ("filter", "fft", "attention")
    made = {}
    for i, mixer in enumerate(mixers):
        torch.manual_seed(0)
        model = SpectreViT(**SMALL, mixer=mixer).to(dev).train()
        opt = FusedAdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True)
        made[mixer] = GraphedTrainStep(model, opt, CrossEntropyLoss(), img, labels, autocast_dtype=torch.bfloat16)
        if i + 1 < len(mixers):
            made[mixer].close()
    try:
        for _ in range(warmup):
            for s in made.values():
                s.graph.replay()
        torch.cuda.synchronize()
        times = {m: [] for m in mixers}
        for _ in range(rounds):
            for m in mixers:
                times[m].append(timed(made[m].graph, per_round))
    finally:
        made[mixers[-1]].close()
    med = statistics.median
    return {"workload": f"SpectreViT Small, bs {B}, bf16, graph replay", "rounds": rounds, "replays_per_round": per_round,
            "step_ms": {m: med(v) for m, v in times.items()}, "step_ms_min_max": {m: [min(v), max(v)] for m, v in times.items()},
            "loss": {m: float(made[m].loss) for m in mixers}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "profile", "steps"), default="profile")
    ap.add_argument("--launches", type=int, default=20, help="launches of each kernel in the profiled run")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per-round", type=int, default=10, help="replays per timed window; rounds * per-round >= 100 timed replays per side")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "kernels":
        run_kernels(a.launches)
        return
    rec = profile(a.launches) if a.mode == "profile" else steps(a.warmup, a.rounds, a.per_round)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
