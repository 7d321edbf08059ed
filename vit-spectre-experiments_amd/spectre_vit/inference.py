"""Frozen-model inference replayed from HIP graphs, with predictions and running metrics computed on the device -- the build's
counterpart of the reference's forward-latency loop (spectre_vit/repl/test.py:30-62, at the config's batch_size = 8) and of the
"freeze a checkpoint for deployment" half of repl/export.py.  An eager ``model(x)`` costs the host ~70 launches through
the training path's autograd Functions, which is what sets the latency below batch 64; a replay costs it one call.

    s = InferenceSession(model, batch_sizes=(1, 8, 64, 512), autocast_dtype=torch.bfloat16, input="float", topk=5)
    logits = s(img)                       # any B >= 1 -> (B, num_classes) fp32
    pred = s.predict(img)                 # (B,) int64: index of the FIRST maximum (torch.argmax's documented tie rule)
    s.reset_stats(); s.accumulate(img, labels); ...; s.stats()      # ONE host read: seen / top1 / topk / loss_sum + accuracy, loss
    s.refresh()                           # take the model's current weights
    s.close()

    python -m spectre_vit.inference --config spectre_vit/configs/spectre_vit_cifar100.py --mixer fft --checkpoint model_best.pt

THE FROZEN-WEIGHTS RULE.  A session's outputs change only at ``refresh()``.  The session reads nothing the model, an optimizer or
``shadows``' weight-copy cache owns: at construction (and at every ``refresh()``) the model's parameters and buffers are copied into
the session's own eval-mode replica, whose tensors never move, and the compute-dtype (W, W^T) copies the GEMMs read live in buffers
the session owns as well (``shadows.PinnedShadows``; ``refresh()`` recasts them in place with one spv_weight_shadows_multi launch).
Training the model, stepping an optimizer, replaying a ``GraphedTrainStep`` (which writes weights through raw pointers and empties
that cache) or freeing the model leaves a session's results bit for bit where they were.  The source model is never put into
another mode: the replica is the module that runs, always in ``eval()``.

WHAT ONE GRAPH HOLDS.  One graph per bucket of ``batch_sizes``, captured on first use, on one stream (the forward has no side-stream
work, so the graph is a chain): the replica's eval forward under ``no_grad`` and the given autocast, reading the bucket's static
input buffer, then ONE spv_eval_head launch (csrc/spv_infer.hip) that turns the logits into predictions and adds the batch to the
running metrics.  By-value kernel arguments are frozen at capture, so the number of valid rows lives in a device word the kernel reads
(the idea of the dropout seed word in spectre_vit.graph) and the labels in a static int64 buffer; label -1 means "no label": the row
gets a prediction and is not counted.  A batch goes into the smallest bucket that holds it (rows past B are padding: no op of
SpectreViT / SpectreBranch mixes samples, SURVEY 8e, so they cannot change rows [:B]); B above the largest bucket runs as chunks of
the largest bucket plus one remainder.  The baseline ``ViT`` attends ACROSS the batch axis, so padding would change its
results: it is served only when every part of a call fills its bucket exactly.

RETURNED TENSORS are views of static buffers that the next call overwrites (as ``GraphedTrainStep.out``): clone what must outlive
it.  (A call that was split into chunks returns a fresh concatenation.)
"""
from __future__ import annotations

import copy

import torch

DEFAULT_BUCKETS = (1, 8, 64, 512)


# ---------------------------------------------------------------------------------------------------------------------------------
# bucket choice and chunk plan: pure functions of the batch size
# ---------------------------------------------------------------------------------------------------------------------------------
def normalize_buckets(batch_sizes):
    b = sorted({int(v) for v in batch_sizes})
    if not b or b[0] < 1:
        raise ValueError(f"batch_sizes must be positive integers, got {tuple(batch_sizes)!r}")
    return tuple(b)


def pick_bucket(batch, buckets=DEFAULT_BUCKETS):
    """the smallest bucket that holds `batch` rows; the largest one when none does (the caller chunks)"""
    if batch < 1:
        raise ValueError(f"a batch needs at least one row, got {batch}")
    for b in buckets:
        if b >= batch:
            return b
    return buckets[-1]


def chunk_plan(batch, buckets=DEFAULT_BUCKETS, exact=False):
    """[(first row, rows, bucket)] for a call with `batch` rows: chunks of the largest bucket, then one remainder in the smallest
    bucket that holds it.  exact=True (a model that mixes samples across the batch axis): every part must fill its bucket."""
    if batch < 1:
        raise ValueError(f"a batch needs at least one row, got {batch}")
    big = buckets[-1]
    plan, at = [], 0
    while batch - at > big:
        plan.append((at, big, big))
        at += big
    plan.append((at, batch - at, pick_bucket(batch - at, buckets)))
    if exact:
        for _, rows, bucket in plan:
            if rows != bucket:
                raise ValueError(f"a batch of {batch} does not fill the buckets {tuple(buckets)} exactly ({rows} rows would sit in a "
                                 f"bucket of {bucket}): the baseline ViT attends across the batch axis (SURVEY 0.4), so padding rows "
                                 "would change every result -- pass batch_sizes that contain the batch size")
    return plan


def eval_buckets(n, batch):
    """buckets of a validation pass over n samples in batches of `batch`: the batch size, and the tail rounded up to a multiple of 8"""
    batch = max(1, min(int(batch), int(n)))
    tail = int(n) % batch
    out = {batch}
    if tail:
        out.add(min((tail + 7) // 8 * 8, batch))
    return tuple(sorted(out))


def derive_stats(seen, top1, topk, loss_sum):
    seen, top1, topk, loss_sum = int(seen), int(top1), int(topk), float(loss_sum)
    d = max(seen, 1)
    return {"seen": seen, "top1": top1, "topk": topk, "loss_sum": loss_sum, "accuracy": top1 / d, "topk_accuracy": topk / d,
            "loss": loss_sum / d}


class _Bucket:
    __slots__ = ("rows", "img", "labels", "labelled", "pred", "logits", "features", "graph")


class InferenceSession:
    """See the module docstring.  ``input="uint8"``: NHWC uint8 batches through the model's PixelNorm patch gather (SpectreViT only, as
    the eager forward).  ``return_features=True``: ``s.features`` holds the CLS features of the last call's (last) bucket."""

    def __init__(self, model, batch_sizes=DEFAULT_BUCKETS, autocast_dtype=torch.bfloat16, input="float", topk=5, return_features=False):
        from spectre_vit import hip_ops, shadows
        from spectre_vit.models.spectre.spectre import SpectreViT
        from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranch
        from spectre_vit.models.vit.vit import ViT
        if not isinstance(model, (SpectreViT, SpectreBranch, ViT)):
            raise TypeError(f"InferenceSession serves SpectreViT, SpectreBranch and ViT, got {type(model).__name__}")
        if input not in ("float", "uint8"):
            raise ValueError(f"input must be 'float' or 'uint8', got {input!r}")
        if not 1 <= int(topk) <= 8:
            raise ValueError(f"topk={topk} outside 1..8")
        if input == "uint8" and not isinstance(model, SpectreViT):
            raise ValueError(f"the uint8 NHWC input path is SpectreViT's patch gather: {type(model).__name__} takes float images")
        self.buckets = normalize_buckets(batch_sizes)
        p0 = next(model.parameters())
        if not p0.is_cuda:
            raise RuntimeError("InferenceSession needs the model on an AMD GPU (cuda/HIP device); there is no CPU fallback in this package")
        self.device = p0.device
        self.model = model
        self.exact = isinstance(model, ViT)
        self.autocast_dtype = autocast_dtype
        self.input = input
        self.topk = int(topk)
        self.return_features = bool(return_features)
        self._closed = False
        # the replica: every tensor the kernels read is the session's own, at an address that never changes
        net = copy.deepcopy(model)
        for mod in net.modules():
            mod.__dict__.pop("_spv_shadow_set", None)   # (a training forward's copies: not this replica's business)
        net.eval().requires_grad_(False)
        self._net = net
        self._dst = dict(net.named_parameters())
        self._dst.update(net.named_buffers())
        self._pinned = shadows.PinnedShadows()
        self._n_valid = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._rows_word = 0   # the host's copy of the device word
        self._stats = hip_ops.eval_head_stats(self.device)
        self._b = {}
        self._sample_shape = None
        self.features = None
        self.replays = 0

    # -- weights --------------------------------------------------------------------------------------------------------------------
    def refresh(self):
        """re-snapshot the model's current parameters and buffers into the session's fixed buffers: a few copies, the permutation
        tables repacked in place, ONE weight-cast launch per compute dtype.  The only call after which outputs may differ."""
        from spectre_vit import _native, hip_ops
        from spectre_vit.models.spectre.layers import MHPermutMix
        self._check_open()
        src = dict(self.model.named_parameters())
        src.update(self.model.named_buffers())
        if src.keys() != self._dst.keys():
            raise RuntimeError("the model's parameters / buffers changed names since the session was built")
        names = list(self._dst)
        with torch.no_grad(), torch.cuda.device(self.device):
            torch._foreach_copy_([self._dst[k] for k in names], [src[k].detach() for k in names])
            for mod in self._net.modules():
                if isinstance(mod, MHPermutMix) and mod._packed is not None:
                    table = mod._packed[1]   # the captured launches read this very tensor
                    perms, signs = mod.perms, mod.signs.reshape(mod.num_heads, -1)
                    _native.call("spv_permut_pack", perms.data_ptr(), signs.data_ptr(), table.data_ptr(), perms.shape[0], perms.shape[1],
                                 hip_ops._stream())
                    mod._packed = ((mod.perms.data_ptr(), mod.perms._version, mod.signs.data_ptr(), mod.signs._version), table)
            self._pinned.refresh()

    # -- one bucket -----------------------------------------------------------------------------------------------------------------
    def _forward(self, b):
        from spectre_vit import hip_ops
        with torch.no_grad(), torch.autocast("cuda", dtype=self.autocast_dtype or torch.bfloat16, enabled=self.autocast_dtype is not None):
            if self.return_features:
                logits, feats = self._net(b.img, return_features=True)
            else:
                logits, feats = self._net(b.img), None
        logits = logits.float().contiguous()   # (fp32 already: the heads write fp32 logits, as under stock autocast)
        hip_ops.eval_head(logits, b.labels, self._n_valid, b.pred, self._stats, self.topk)
        return logits, feats

    def _bucket(self, rows, like):
        b = self._b.get(rows)
        if b is not None:
            return b
        from spectre_vit import shadows
        if self._sample_shape is None:
            self._sample_shape = tuple(like.shape[1:])
        b = _Bucket()
        b.rows = rows
        b.img = torch.zeros((rows, *self._sample_shape), dtype=torch.uint8 if self.input == "uint8" else torch.float32, device=self.device)
        b.labels = torch.full((rows,), -1, dtype=torch.int64, device=self.device)
        b.labelled = False
        b.pred = torch.zeros((rows,), dtype=torch.int64, device=self.device)
        # warm-up on a side stream (allocator pools, lazily built tables, the session's weight copies), then the capture; the warm-up
        # counts nothing: its labels are all -1
        keep = self._n_valid.clone()
        self._n_valid.zero_()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), shadows.pinned_shadows(self._pinned):
            self._forward(b)
        torch.cuda.current_stream().wait_stream(side)
        b.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(b.graph), shadows.pinned_shadows(self._pinned):
            b.logits, b.features = self._forward(b)
        self._n_valid.copy_(keep)
        self._b[rows] = b
        return b

    def _run(self, img, labels):
        """-> [(bucket, rows)] after replaying every part of the call"""
        self._check_open()
        if not img.is_cuda:
            raise RuntimeError("InferenceSession needs its batches on the GPU")
        want = torch.uint8 if self.input == "uint8" else None
        if (img.dtype == torch.uint8) != (want is torch.uint8):
            raise ValueError(f"this session was built with input={self.input!r}, got a {img.dtype} batch")
        if self._sample_shape is not None and tuple(img.shape[1:]) != self._sample_shape:
            raise ValueError(f"sample shape {tuple(img.shape[1:])} differs from the captured {self._sample_shape}")
        if labels is not None and labels.shape[0] != img.shape[0]:
            raise ValueError(f"{img.shape[0]} images but {labels.shape[0]} labels")
        if torch.cuda.current_device() != self.device.index:
            raise RuntimeError(f"the session lives on {self.device} but the current device is cuda:{torch.cuda.current_device()}")
        plan = chunk_plan(img.shape[0], self.buckets, self.exact)
        done = []
        for at, rows, bucket in plan:
            b = self._bucket(bucket, img)
            b.img[:rows].copy_(img[at:at + rows], non_blocking=True)
            if labels is not None:
                b.labels[:rows].copy_(labels[at:at + rows], non_blocking=True)   # (any integer dtype: the copy widens it)
                b.labelled = True
            elif b.labelled:   # (a launch only after an accumulate: the buffer already holds -1 otherwise)
                b.labels.fill_(-1)
                b.labelled = False
            if rows != self._rows_word:   # the device word follows the host's copy of it: a launch only when the row count changes
                self._n_valid.fill_(rows)
                self._rows_word = rows
            b.graph.replay()
            self.replays += 1
            if len(plan) == 1:
                done.append((b, rows))
            else:   # a chunked call hands back a concatenation: keep this part before its bucket is replayed again
                done.append((b, rows, b.logits[:rows].clone(), b.pred[:rows].clone()))
        self.features = done[-1][0].features[:done[-1][1]] if self.return_features else None
        return done

    @staticmethod
    def _gather(done, what):
        if len(done[0]) == 2:
            b, rows = done[0]
            return (b.logits if what == 0 else b.pred)[:rows]
        return torch.cat([d[2 + what] for d in done])

    # -- public calls ---------------------------------------------------------------------------------------------------------------
    def __call__(self, img):
        """(B, num_classes) fp32 logits; a view of a static buffer (see the module docstring)"""
        return self._gather(self._run(img, None), 0)

    def predict(self, img):
        """(B,) int64: the index of the first maximum of every row of logits"""
        return self._gather(self._run(img, None), 1)

    def accumulate(self, img, labels):
        """the batch's rows with 0 <= label < num_classes are added to the running metrics (label -1: skipped); returns the logits"""
        return self._gather(self._run(img, labels), 0)

    def reset_stats(self):
        self._check_open()
        self._stats.zero_()

    def stats_tensor(self):
        """float64 device tensor (seen, top1, topk, loss_sum) -- counts are exact below 2^53 -- for a caller that reduces it across
        ranks before its one host read"""
        return torch.cat([self._stats[:3].double(), self._stats[3:4].view(torch.float64)])

    def stats(self):
        """ONE host read: {"seen", "top1", "topk", "loss_sum"} and the derived "accuracy", "topk_accuracy", "loss" (means over seen)"""
        self._check_open()
        w = self._stats[:4].cpu()
        return derive_stats(w[0].item(), w[1].item(), w[2].item(), w[3:4].view(torch.float64).item())

    def _check_open(self):
        if self._closed:
            raise RuntimeError("this InferenceSession was closed")

    def close(self):
        """drop the graphs and every buffer of the session"""
        self._closed = True
        self._b = {}
        self._net = self._dst = self._pinned = self.features = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# python -m spectre_vit.inference: score the harness's synthetic validation set, or a split of dataset files, with a checkpoint
# ---------------------------------------------------------------------------------------------------------------------------------
def build_parser():
    import argparse
    ap = argparse.ArgumentParser(description="score a checkpoint on the harness's synthetic validation set; prints one JSON line")
    ap.add_argument("--config", default="spectre_vit/configs/spectre_vit_cifar100.py")
    ap.add_argument("--mixer", default="permut")
    ap.add_argument("--model", default="spectre", choices=("spectre", "spectre_branch"))
    ap.add_argument("--checkpoint", required=True, help="a state_dict written by the harness (model_best.pt); loaded strictly")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--no-amp", action="store_true", help="fp32 kernels instead of bf16 autocast")
    ap.add_argument("--data-root", default=None, metavar="DIR",
                    help="score the dataset files under DIR (spectre_vit.datasets) instead of the synthetic set; --n is then ignored")
    ap.add_argument("--dataset", default=None, choices=("cifar100", "cifar10", "mnist", "npz"),
                    help="--data-root: the files' format; left out it follows the config's file name")
    ap.add_argument("--split", default="test", choices=("train", "test"), help="--data-root: the split that is scored")
    return ap


def score(config_path, checkpoint, mixer="permut", model="spectre", batch=512, n=10000, use_amp=True, data_root=None, dataset=None,
          split="test", normalize=None):
    """data_root: the split of the dataset files under it (spectre_vit.datasets.FileDataset; dataset left out follows the config's file
    name, normalize as there) is scored, every sample, the ragged last batch included; n is then the split's size"""
    import time

    from spectre_vit.configs.parser import parse_config
    from spectre_vit.harness import SyntheticCifar, build_model
    c = parse_config(config_path)
    files = None
    if data_root is not None:   # read and checked on the host, before a device is touched
        from spectre_vit import datasets
        files = datasets.FileDataset(data_root, dataset or datasets.dataset_of_config(config_path), split, None, normalize)
        if (files.channels, files.height, files.width) != (c.in_channels, c.img_size, c.img_size) or files.num_classes > c.num_classes:
            raise ValueError(f"{files.root} ({files.dataset}, {split}) holds {files.channels} x {files.height} x {files.width} images of "
                             f"{files.num_classes} classes, the config in_channels={c.in_channels}, img_size={c.img_size}, "
                             f"num_classes={c.num_classes}")
        files.num_classes, n = int(c.num_classes), len(files)
    elif dataset is not None or normalize is not None:
        raise ValueError("dataset / normalize describe the files under data_root: they need data_root")
    device = torch.device("cuda", torch.cuda.current_device())
    net = build_model(c, mixer, device, model)
    net.load_state_dict(torch.load(checkpoint, map_location=device), strict=True)
    val_set = files.upload(device) if files is not None else SyntheticCifar(n, c, device, seed=getattr(c, "random_seed", 42) + 1)
    with InferenceSession(net, batch_sizes=eval_buckets(n, batch), autocast_dtype=torch.bfloat16 if use_amp else None) as s:
        def one_pass():
            s.reset_stats()
            for img, label in val_set.batches(min(batch, n), False, drop_last=False):
                s.accumulate(img, label)
            return s.stats()
        one_pass()   # captures the graphs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = one_pass()   # (its host read is the synchronisation)
        dt = time.perf_counter() - t0
    return {"accuracy": st["accuracy"], "top5": st["topk_accuracy"], "loss": st["loss"], "images_per_s": round(st["seen"] / dt, 1),
            "seen": st["seen"]}


def main(argv=None):
    import json
    a = build_parser().parse_args(argv)
    print(json.dumps(score(a.config, a.checkpoint, a.mixer, a.model, a.batch, a.n, not a.no_amp, a.data_root, a.dataset, a.split)))


if __name__ == "__main__":
    main()
