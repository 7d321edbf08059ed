#!/usr/bin/env python3
"""Inference latency / throughput of the mirrored models -- counterpart of the reference's spectre_vit/repl/test.py:30-62
(which times forward passes without synchronising the device; here every sample is bracketed by HIP events).

    python tools/infer_bench.py [--mixer fft|permut|dwt_embed|dwt_token|attention] [--model spectre|vit] [--batches 1,8,64,512]
    python tools/infer_bench.py --session ...     # the graph-replayed spectre_vit.inference.InferenceSession beside the eager loop

--session: both paths run in the same process on the same model and input, alternating eager / session windows per batch size
(three of each; the median is reported, the extremes as the spread), every timed window at least 0.5 s long.
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
from spectre_vit.models.spectre.spectre import SpectreViT  # noqa: E402
from spectre_vit.models.vit.vit import ViT  # noqa: E402


def timed(fn, iters):
    """mean milliseconds per call of `iters` back-to-back calls, bracketed by HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def iters_for(fn, window_s):
    """calls that fill a window of `window_s` seconds, from a short calibration run"""
    ms = timed(fn, 20)
    return max(20, int(window_s * 1e3 / ms) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixer", default="fft")
    ap.add_argument("--model", default="spectre", choices=["spectre", "vit"])
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--session", action="store_true", help="time InferenceSession replays beside the eager loop, alternating the two")
    ap.add_argument("--window", type=float, default=0.5, help="--session: least length of a timed window, seconds")
    ap.add_argument("--only", choices=["eager", "session"], default=None,
                    help="--session: run one of the two paths alone (for a kernel trace of its own); no comparison is printed")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    model = (SpectreViT(**SMALL, mixer=args.mixer) if args.model == "spectre" else ViT(**SMALL)).to(dev).eval()
    batches = [int(b) for b in args.batches.split(",")]
    out = []
    session = None
    if args.session:
        from spectre_vit.inference import InferenceSession
        session = InferenceSession(model, batch_sizes=batches, autocast_dtype=torch.bfloat16)
    for bs in batches:
        x = torch.randn(bs, 3, 32, 32, device=dev)

        def eager():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                model(x)

        for _ in range(5):
            eager()
        if session is None:
            ms = timed(eager, args.iters)
            out.append({"batch": bs, "latency_ms": round(ms, 4), "images_per_s": round(bs / ms * 1e3, 1)})
            continue
        replay = lambda: session(x)  # noqa: E731
        if args.only is not None:
            fn = eager if args.only == "eager" else replay
            for _ in range(5):
                fn()
            n = iters_for(fn, args.window)
            out.append({"batch": bs, "path": args.only, "latency_ms": round(timed(fn, n), 4), "iters": n})
            continue
        for _ in range(5):
            replay()
        n_e, n_s = iters_for(eager, args.window), iters_for(replay, args.window)
        e_ms, s_ms = [], []
        for _ in range(3):   # eager, session, eager, session, ...: drift of the box lands on both
            e_ms.append(timed(eager, n_e))
            s_ms.append(timed(replay, n_s))
        e, s = statistics.median(e_ms), statistics.median(s_ms)
        out.append({"batch": bs, "eager_latency_ms": round(e, 4), "session_latency_ms": round(s, 4),
                    "eager_windows_ms": [round(v, 4) for v in e_ms], "session_windows_ms": [round(v, 4) for v in s_ms],
                    "eager_iters": n_e, "session_iters": n_s, "speedup": round(e / s, 3),
                    "eager_images_per_s": round(bs / e * 1e3, 1), "session_images_per_s": round(bs / s * 1e3, 1)})
    if session is not None:
        session.close()
    print(json.dumps({"model": args.model, "mixer": args.mixer if args.model == "spectre" else None, "dtype": "bf16",
                      "session": bool(args.session), "results": out}))


if __name__ == "__main__":
    main()
