#!/usr/bin/env python3
"""What does reading a real dataset cost a run, and does the training step notice?  

--what kernel   spv_dataset_ingest on 50 000 x 3 x 32 x 32 and 60 000 x 1 x 28 x 28 random bytes resident on the device (labels and a
                100- / 10-class histogram with it; once more with labels NULL), device events around each launch; beside it, for information, a torch restatement in
                the same process -- permute(0, 2, 3, 1).contiguous() plus the four reductions (per-channel sum and sum of squares in
                int64, the label histogram, the count of labels out of range) -- the two in alternating windows, medians and ranges.
--what load     the whole FileDataset load from local disk: files in the CIFAR-100 and MNIST formats written from random bytes into a
                temporary directory, then load_files (host) and upload (device: pinned chunks, side stream, one ingest per chunk) timed
                apart, several times.
--what step     harness.train, Small / CIFAR-100 config, fft mixer, batch 512, graph + device_loader + augment: the file-fed run and its
                synthetic twin alternate in ONE process; per call the epochs' wall time per step (the first epoch, which holds set-up
                and the capture, left out).  The synthetic arm's spread across its calls is stated next to the difference.
--what trace    ONE such run (--arm files | synthetic), short, for rocprofv3 --kernel-trace --stats; tools/dataset_probe.py --compare
                A_kernel_stats.csv B_kernel_stats.csv then lists both arms' kernels and call counts side by side.

    python tools/dataset_probe.py --what kernel load step --out profiles/dataset_v1_probe.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o files -- python tools/dataset_probe.py --what trace --arm files

Fails without a GPU.  One JSON line.
"""
import argparse
import csv
import gzip
import json
import os
import pickle
import shutil
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-spectre-experiments_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG = "spectre_vit/configs/spectre_vit_cifar100.py"
HBM_COPY_TBS = 6.29   # MI355X, measured float4 copy rate


def _spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def _events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def probe_kernel(rounds, reps):
    from spectre_vit import _native
    res = {}
    for name, (n, c, h, w), classes in (("cifar_50000x3x32x32", (50000, 3, 32, 32), 100), ("mnist_60000x1x28x28", (60000, 1, 28, 28), 10)):
        g = torch.Generator(device="cuda").manual_seed(n)
        src = torch.randint(0, 256, (n, c, h, w), dtype=torch.uint8, device="cuda", generator=g)
        labels = torch.randint(0, classes, (n,), dtype=torch.uint8, device="cuda", generator=g)
        dst = torch.empty((n, h, w, c), dtype=torch.uint8, device="cuda")
        stats = torch.zeros(int(_native.call("spv_dataset_stats_words", c, classes)), dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def ingest():
            _native.call("spv_dataset_ingest", src.data_ptr(), dst.data_ptr(), labels.data_ptr(), 0, stats.data_ptr(), n, c, h, w, 0, classes, st)

        def ingest_unlabelled():
            _native.call("spv_dataset_ingest", src.data_ptr(), dst.data_ptr(), 0, 0, stats.data_ptr(), n, c, h, w, 0, classes, st)

        def restated():
            out = src.permute(0, 2, 3, 1).contiguous()
            x = src.view(n, c, h * w)
            s = x.sum(dim=(0, 2), dtype=torch.int64)
            q = (x.to(torch.int32) ** 2).sum(dim=(0, 2), dtype=torch.int64)
            lab = labels.long()
            hist = torch.bincount(lab.clamp(0, classes - 1), minlength=classes)
            stray = ((lab < 0) | (lab >= classes)).sum()
            return out, s, q, hist, stray
        ingest()
        out, s, q, hist, stray = restated()
        torch.cuda.synchronize()
        got = stats.tolist()
        assert torch.equal(out, dst) and got[:c] == s.tolist() and got[c:2 * c] == q.tolist() and got[2 * c + 2:] == hist.tolist()
        k_us, u_us, t_us = [], [], []
        for _ in range(rounds):   # alternating windows
            k_us += _events(ingest, reps)
            u_us += _events(ingest_unlabelled, reps)
            t_us += _events(restated, reps)
        bytes_moved = 2 * n * c * h * w
        med = statistics.median(k_us)
        res[name] = {"bytes_read_and_written": bytes_moved, "ingest_us": _spread(k_us), "ingest_without_labels_us": _spread(u_us), "torch_restatement_us": _spread(t_us),
                     "ingest_TBps": bytes_moved / med / 1e6, "share_of_hbm_copy_rate": bytes_moved / med / 1e6 / HBM_COPY_TBS}
    return res


def _write_sets(root, n_train, n_test):
    """CIFAR-100 and MNIST files from random bytes (Python-3 protocol-2 pickles: the readers take both styles)"""
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "cifar-100-python"))
    os.makedirs(os.path.join(root, "MNIST", "raw"))
    for split, n in (("train", n_train), ("test", n_test)):
        d = {"data": rng.integers(0, 256, size=(n, 3072), dtype=np.uint8), "fine_labels": rng.integers(0, 100, size=n).tolist()}
        with open(os.path.join(root, "cifar-100-python", split), "wb") as f:
            pickle.dump(d, f, protocol=2)
        stem = "train" if split == "train" else "t10k"
        m = n * 6 // 5   # 60 000 / 12 000 beside 50 000 / 10 000
        with open(os.path.join(root, "MNIST", "raw", f"{stem}-images-idx3-ubyte"), "wb") as f:
            f.write(struct.pack(">4I", 0x803, m, 28, 28) + rng.integers(0, 256, size=m * 784, dtype=np.uint8).tobytes())
        with gzip.open(os.path.join(root, "MNIST", "raw", f"{stem}-labels-idx1-ubyte.gz"), "wb") as f:
            f.write(struct.pack(">2I", 0x801, m) + rng.integers(0, 10, size=m, dtype=np.uint8).tobytes())
    with open(os.path.join(root, "cifar-100-python", "meta"), "wb") as f:
        pickle.dump({"fine_label_names": [f"class_{i}" for i in range(100)]}, f, protocol=2)


def probe_load(root, reps):
    from spectre_vit import datasets
    res = {}
    for dataset in ("cifar100", "mnist"):
        host, dev = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            ds = datasets.FileDataset(root, dataset, "train", None, "measured")
            t1 = time.perf_counter()
            ds.upload(torch.device("cuda", torch.cuda.current_device()))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host.append((t1 - t0) * 1e3)
            dev.append((t2 - t1) * 1e3)
        res[dataset] = {"images": len(ds), "bytes": int(ds.images.numel()), "read_ms": _spread(host[1:]), "upload_ingest_ms": _spread(dev[1:]),
                        "mean": list(ds.mean_values), "std": list(ds.std_values), "digest": ds.digest}
    return res


def run_arm(arm, root, a, out_dir, epochs):
    """one harness.train call -> the wall time per step, in ms, of every epoch but the first"""
    from spectre_vit import harness
    stamps = [time.perf_counter()]
    data = dict(data_root=root, dataset="cifar100") if arm == "files" else dict(n_train=a.n_train, n_val=a.n_val)
    harness.train(CFG, mixer="fft", epochs=epochs, steps_per_epoch=a.steps, batch_size=a.batch, graph=True, device_loader=True, augment=True,
                  out_dir=out_dir, log=lambda rec: stamps.append(time.perf_counter()), **data)
    torch.cuda.synchronize()
    return [(b - c) * 1e3 / a.steps for c, b in zip(stamps[1:], stamps[2:])]


def probe_step(root, a, tmp):
    calls = {"synthetic": [], "files": []}
    for k in range(2 * a.rounds + 1):   # synthetic, files, synthetic, ..., synthetic
        arm = "files" if k % 2 else "synthetic"
        calls[arm].append(statistics.median(run_arm(arm, root, a, os.path.join(tmp, f"run{k}"), a.epochs)))
    syn, fil = calls["synthetic"], calls["files"]
    return {"workload": f"harness.train Small fft cifar100, bs {a.batch}, {a.steps} steps/epoch, graph + device_loader + augment; "
                        "per call the median over its epochs (validation included, the first epoch left out)",
            "ms_per_step": {"synthetic": _spread(syn), "files": _spread(fil)},
            "difference_ms": statistics.median(fil) - statistics.median(syn),
            "synthetic_run_to_run_spread_ms": max(syn) - min(syn)}


def compare(path_a, path_b, out):
    """two rocprofv3 kernel_stats.csv files -> one table: every kernel's calls and average in both arms"""
    arms = []
    for p in (path_a, path_b):
        arms.append({r["Name"]: r for r in csv.DictReader(open(p))})
    names = sorted(set(arms[0]) | set(arms[1]), key=lambda k: -max(float(arm[k]["TotalDurationNs"]) for arm in arms if k in arm))
    with open(out, "w", newline="") as f:
        wr = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        wr.writerow(["Name", "CallsSynthetic", "CallsFiles", "AverageNsSynthetic", "AverageNsFiles", "SameCalls"])
        for k in names:
            ca, cb = (int(arm[k]["Calls"]) if k in arm else 0 for arm in arms)
            aa, ab = (round(float(arm[k]["AverageNs"]), 1) if k in arm else "" for arm in arms)
            wr.writerow([k, ca, cb, aa, ab, "yes" if ca == cb else "no"])
    differ = [k for k in names if (int(arms[0][k]["Calls"]) if k in arms[0] else 0) != (int(arms[1][k]["Calls"]) if k in arms[1] else 0)]
    print(json.dumps({"kernels": len(names), "differing": differ}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["kernel", "load", "step"], choices=("kernel", "load", "step", "trace"))
    ap.add_argument("--arm", default="files", choices=("files", "synthetic"))
    ap.add_argument("--compare", nargs=2, default=None, metavar="CSV")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=90)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--n-train", type=int, default=50000)
    ap.add_argument("--n-val", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.compare:
        compare(a.compare[0], a.compare[1], a.out or "kernel_stats_compare.csv")
        return
    assert torch.cuda.is_available(), "needs an MI355X"
    res = {}
    tmp = tempfile.mkdtemp(prefix="dataset_probe_")
    try:
        root = os.path.join(tmp, "data")
        if set(a.what) & {"load", "step", "trace"}:
            _write_sets(root, a.n_train, a.n_val)
        if "kernel" in a.what:
            res["kernel"] = probe_kernel(a.rounds, a.reps)
        if "load" in a.what:
            res["load"] = probe_load(root, a.rounds)
        if "step" in a.what:
            res["step"] = probe_step(root, a, tmp)
        if "trace" in a.what:
            res["trace"] = {"arm": a.arm, "ms_per_step": run_arm(a.arm, root, a, os.path.join(tmp, "trace"), a.epochs)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
