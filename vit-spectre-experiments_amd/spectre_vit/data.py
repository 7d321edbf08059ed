"""The resident loader: the ``DataLoader(shuffle=True)`` of reference spectre_vit/repl/train.py:147-155, 216-218 on the device.

The training set lives on the GPU as uint8; ``fetch()`` is ONE launch (``spv_loader_fetch``, csrc/spv_loader.hip) that reads the step
from a device cursor, writes that step's shuffled batch -- index, labels, image -- into buffers at fixed addresses and advances the
cursor.  Nothing of the launch depends on a by-value step, so it can be captured: every replay fetches the next batch, and a
graph-replayed training step (``spectre_vit.graph.GraphedTrainStep(loader=...)``) needs nothing from the host in front of it.

    loader = ResidentLoader(train_u8_nhwc, labels, 512, mean=CIFAR_MEAN, std=CIFAR_STD, seed=42)
    loader.fetch()                 # loader.img (fp32 NCHW, normalised), loader.labels (int64), loader.index (int64): step 0
    loader.fetch()                 # the same buffers now hold step 1

The order is not torch's randperm: each epoch's permutation is a keyed bijection of [0, n) evaluated per sample (a six-round Feistel
network with cycle-walking, include/spv.h "the resident loader"), sharded over the ranks as ``idx[rank::world]`` with the tail dropped.
``ResidentLoader.indices`` restates it on the host.

``output="augment"`` with ``augment=TrainAugment(...)`` fetches AND augments in that one launch (``spv_loader_fetch_augment``,
csrc/spv_augment.hip): the transform's parameter table is drawn on the device under the key (augment seed, the cursor's step, slot), so
a captured fetch draws a new table at every replay; ``loader.params`` holds the step's table, ``loader.img`` the augmented batch.
``output="augment_tiled"`` is the same for the images that launch cannot stage, 64 x 64 up to 512 x 512 (``spv_loader_fetch_augment_tiled``,
csrc/spv_augment_tiled.hip): the fetch and the draw ride in the tiled chain's contrast pre-pass, the tile kernel follows -- two launches,
neither with a by-value step, so ``fetch()`` is as capturable.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from spectre_vit import _native
from spectre_vit._launch import _p, _require_gpu, _stream

CIFAR_MEAN = (0.5071, 0.4867, 0.4408)
CIFAR_STD = (0.2675, 0.2565, 0.2761)

_U64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
ROUNDS = 6          # SPV_LOADER_ROUNDS
_MODES = {"none": 0, "float": 1, "uint8": 2}   # SPV_LOADER_NONE / _FLOAT / _UINT8
_FUSED = {"augment": "spv_loader_fetch_augment", "augment_tiled": "spv_loader_fetch_augment_tiled"}   # fetch and augment in one call
_OUTPUTS = tuple(_MODES) + tuple(_FUSED)


def _mix64(x):
    x &= _U64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & _U64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & _U64
    return x ^ (x >> 33)


def _mix32(x):
    m = np.uint64(0xFFFFFFFF)
    x = x & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def _permute(key, n, x):
    """the epoch's bijection of [0, n) on a uint64 array of positions < n (csrc/spv_loader_core.h ldr_permute)"""
    h = 1
    while (1 << (2 * h)) < n:
        h += 1
    mask, sh = np.uint64((1 << h) - 1), np.uint64(h)
    keys = [np.uint64(_mix64(key + (r + 1) * _GOLDEN) & 0xFFFFFFFF) for r in range(ROUNDS)]
    x = x.copy()
    walking = np.ones(x.shape, dtype=bool)
    while walking.any():
        v = x[walking]
        left, right = v >> sh, v & mask
        for k in keys:
            left, right = right, left ^ (_mix32(right + k) & mask)
        v = (left << sh) | right
        x[walking] = v
        walking[walking] = v >= np.uint64(n)
    return x


class ResidentLoader:
    """Shuffled batches of a GPU-resident uint8 set, fetched by one capturable launch.

    images_u8_nhwc  uint8 (N, H, W, C), contiguous, on the GPU; C 1 or 3, H and W 1..512, N < 2^31
    labels          uint8 or int64 (N,), contiguous, on the same device
    output          "float": ``img`` fp32 (B, C, H, W) = (x / 255 - mean) / std (the kernel multiplies by 1 / std, rounded once);
                    "uint8": ``img`` uint8 (B, H, W, C), the rows unchanged (models built with uint8_input=True normalise themselves);
                    "none": no image -- hand ``index`` to ``TrainAugment`` or to ``DistillationLoss(index=)``;
                    "augment": ``img`` fp32 (B, C, H, W) = ``augment``'s chain on the step's rows, its table drawn at the cursor's
                    step, and ``params`` fp32 (B, 16) = that table -- ``augment(images, index, step=t)`` and
                    ``augment.draw(B, step=t, ...)`` bit for bit, in the same launch as the fetch;
                    "augment_tiled": the same buffers from the tiled chain (``TrainAugment(kernel="tiled")``'s bits), for 1 or 3
                    channels and sides 2 .. 512: fetch, draw and contrast pre-pass in one launch, then the tile kernel; the loader
                    owns the pre-pass's workspace at a fixed address
    augment         with output="augment" / "augment_tiled" only: the ``spectre_vit.augment.TrainAugment`` whose mean / std, ranges and seed the launch
                    takes (``mean`` / ``std`` here are unused); images the fused kernel cannot stage -- the tiled sizes, and the one
                    LDS border shape -- are refused: output="none", then ``augment(images, loader.index, step=...)`` serves them
    rank, world     this process's shard: position p of the epoch's order belongs to rank p mod world.  Every rank passes the SAME
                    seed (the ranks share one permutation and take disjoint parts of it)
    steps_per_epoch None: every whole batch of the shard, (N // world) // batch_size; a smaller number ends the epoch earlier (the
                    next epoch draws a new permutation)
    shuffle=False   arange order

    ``img``, ``labels`` (int64), ``index`` (int64), ``params`` keep their addresses for the object's life.  ``step`` is the host's count of the
    fetches (a captured fetch is counted when it is replayed: ``count_replay``); ``device_step()`` reads the device's.
    Every refusal below is raised before a device is touched; there is no CPU fallback."""

    def __init__(self, images_u8_nhwc, labels, batch_size, mean=CIFAR_MEAN, std=CIFAR_STD, seed=42, rank=0, world=1, output="float",
                 shuffle=True, steps_per_epoch=None, augment=None):
        x = images_u8_nhwc
        if output not in _OUTPUTS:
            raise ValueError(f"output is one of {_OUTPUTS}, got {output!r}")
        if augment is not None and output not in _FUSED:
            raise ValueError(f"augment= goes with output='augment' (the fused fetch), not with output={output!r}")
        if output in _FUSED:
            from spectre_vit.augment import TrainAugment
            if not isinstance(augment, TrainAugment):
                raise ValueError(f"output={output!r} needs augment=TrainAugment(...), got {augment!r}")
            if output == "augment" and augment.kernel == "tiled":
                raise ValueError("output='augment' runs the whole-image LDS chain: not with TrainAugment(kernel='tiled')")
            if output == "augment_tiled" and augment.kernel == "lds":
                raise ValueError("output='augment_tiled' runs the tiled chain: not with TrainAugment(kernel='lds')")
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
            raise TypeError("the resident loader takes a contiguous uint8 (N, H, W, C) set, got "
                            f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
        n, H, W, C = x.shape
        if C not in (1, 3) or not (1 <= H <= 512 and 1 <= W <= 512):
            raise ValueError(f"images of {H} x {W} x {C}: the fetch kernel takes 1 or 3 channels and sides 1 .. 512")
        if not 1 <= n < 2 ** 31:
            raise ValueError(f"a set of {n} samples: the permutation is defined for 1 <= n < 2^31")
        if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.uint8, torch.int64) or labels.dim() != 1 \
                or not labels.is_contiguous() or labels.shape[0] != n:
            raise TypeError(f"labels is a contiguous uint8 or int64 vector of the set's {n} rows, got "
                            f"{getattr(labels, 'dtype', type(labels))} {tuple(getattr(labels, 'shape', ()))}")
        if output == "float":
            if mean is None or std is None or len(mean) != C or len(std) != C:
                raise ValueError(f"{C}-channel images, but mean / std name {0 if mean is None else len(mean)} / "
                                 f"{0 if std is None else len(std)} channels")
            if min(float(s) for s in std) <= 0.0:
                raise ValueError(f"std must be positive, got {tuple(std)}")
        if output in _FUSED and len(augment.mean) != C:
            raise ValueError(f"{C}-channel images, but the TrainAugment's mean / std name {len(augment.mean)} channels")
        if output == "augment_tiled" and not _native.call("spv_loader_augment_tiled_supported", C, H, W):   # a host predicate
            raise ValueError(f"a {C} x {H} x {W} image is outside the tiled fetch's shapes (1 or 3 channels, height and width 2 .. 512)")
        if output == "augment":
            if not _native.call("spv_loader_augment_supported", C, H, W):   # a host predicate: no device is touched
                raise ValueError(f"a {C} x {H} x {W} image does not fit the fused fetch's LDS staging (two fp32 copies, the reduction "
                                 "slots and 80 bytes of hand-over within 64 KiB): use output='none', then "
                                 "augment(images, loader.index, step=...) -- spv_loader_fetch, spv_augment_params and spv_augment_u8 / "
                                 "spv_augment_tiled_u8 -- which still serves it")
        batch_size, rank, world = int(batch_size), int(rank), int(world)
        if batch_size < 1:
            raise ValueError(f"batch_size={batch_size} must be positive")
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"rank={rank} outside [0, world={world})")
        if n < batch_size * world:
            raise ValueError(f"a set of {n} samples holds no batch of {batch_size} for each of {world} ranks (n < batch * world)")
        per_pass = (n // world) // batch_size
        if steps_per_epoch is None:
            steps_per_epoch = per_pass
        if isinstance(steps_per_epoch, bool) or not 1 <= int(steps_per_epoch) <= per_pass:
            raise ValueError(f"steps_per_epoch={steps_per_epoch!r} outside 1 .. {per_pass} = (n // world) // batch_size")
        if labels.device != x.device:
            raise ValueError(f"the set is on {x.device} but its labels are on {labels.device}")
        _require_gpu(x, labels)   # no CPU fallback
        self.images, self.labels_src = x, labels
        self.n, self.shape = n, (C, H, W)
        self.batch_size, self.rank, self.world = batch_size, rank, world
        self.steps_per_epoch = int(steps_per_epoch)
        self.seed = int(seed) & _U64
        self.shuffle = bool(shuffle)
        self.output = output
        dev = x.device
        self.mean = self.inv_std = self.params = self._ws = None
        self.augment = augment
        if output in _FUSED:
            self.mean, self.inv_std = augment.norm(dev)
            self.params = torch.zeros((batch_size, 16), dtype=torch.float32, device=dev)   # SPV_AUG_NPARAM
            self._cfg = augment.cfg()   # a host struct read during each call: kept alive here
        if output == "float":   # (mean, 1 / std) as spectre_vit.augment.TrainAugment.norm makes them: the inverse in float64, rounded once
            self.mean = torch.tensor([float(m) for m in mean], dtype=torch.float32, device=dev)
            self.inv_std = (1.0 / torch.tensor([float(s) for s in std], dtype=torch.float64)).float().to(dev)
        self.img = {"float": lambda: torch.empty((batch_size, C, H, W), dtype=torch.float32, device=dev),
                    "uint8": lambda: torch.empty((batch_size, H, W, C), dtype=torch.uint8, device=dev),
                    "augment": lambda: torch.empty((batch_size, C, H, W), dtype=torch.float32, device=dev),
                    "augment_tiled": lambda: torch.empty((batch_size, C, H, W), dtype=torch.float32, device=dev),
                    "none": lambda: None}[output]()
        self.index = torch.zeros(batch_size, dtype=torch.int64, device=dev)
        self.labels = torch.zeros(batch_size, dtype=torch.int64, device=dev)
        self._cursor = torch.zeros(int(_native.call("spv_loader_cursor_bytes")) // 8, dtype=torch.int64, device=dev)
        self.step = 0
        label_dtype = 1 if labels.dtype == torch.int64 else 0
        if output in _FUSED:
            self._entry = _FUSED[output]
            self._args = (_p(x), _p(labels), _p(self._cursor), _p(self.index), _p(self.labels), _p(self.params), _p(self.img),
                          _p(self.mean), _p(self.inv_std), ctypes.addressof(self._cfg), n, batch_size, C, H, W, world, rank,
                          self.steps_per_epoch, self.seed, int(self.shuffle), label_dtype, augment.seed)
            if output == "augment_tiled":   # the contrast pre-pass's partial sums: written and read inside every fetch
                self._ws = torch.empty(_native.call("spv_augment_tiled_ws_bytes", batch_size, H, W), dtype=torch.uint8, device=dev)
                self._args += (_p(self._ws), self._ws.numel())
        else:
            self._entry = "spv_loader_fetch"
            self._args = (_p(x), _p(labels), _p(self._cursor), _p(self.index), _p(self.labels), _p(self.img), _p(self.mean),
                          _p(self.inv_std), n, batch_size, C, H, W, world, rank, self.steps_per_epoch, self.seed, int(self.shuffle),
                          _MODES[output], label_dtype)

    # -- the launch -------------------------------------------------------------------------------------------------------------
    def fetch(self):
        """ONE launch (output="augment_tiled": two) on the current stream: the buffers take the batch of the cursor's step, the cursor moves on.  Allocates
        nothing and uploads nothing, so it may be captured; a captured (recorded, not run) fetch is not counted in ``step``."""
        _native.call(self._entry, *self._args, _stream())
        if not torch.cuda.is_current_stream_capturing():
            self.step += 1

    def count_replay(self, fetches=1):
        """tell the host's mirror that a graph holding this loader's fetch was replayed"""
        self.step += int(fetches)

    # -- the cursor -------------------------------------------------------------------------------------------------------------
    def seek(self, step):
        """the next fetch is step `step` (resume).  A host write into the cursor block: never under capture."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ResidentLoader.seek writes the cursor from the host: not under graph capture")
        step = int(step)
        if step < 0:
            raise ValueError(f"step={step} must be >= 0")
        block = torch.zeros(self._cursor.numel(), dtype=torch.int64)
        block[0] = step if step < 2 ** 63 else step - 2 ** 64
        self._cursor.copy_(block)   # the step, and a re-armed arrival counter
        self.step = step & _U64

    def device_step(self):
        """the cursor as the device holds it (a synchronising read: tests and diagnostics)"""
        return int(self._cursor[0].item()) & _U64

    def state_dict(self):
        return dict(step=self.step, seed=self.seed, n=self.n, batch_size=self.batch_size, rank=self.rank, world=self.world,
                    steps_per_epoch=self.steps_per_epoch, shuffle=self.shuffle)

    def load_state_dict(self, sd):
        """takes the step of a loader of the same order: every other entry must match this loader's"""
        mine = self.state_dict()
        for k in mine:
            if k != "step" and sd.get(k) != mine[k]:
                raise ValueError(f"ResidentLoader.load_state_dict: {k} is {mine[k]!r} here but {sd.get(k)!r} in the saved state")
        self.seek(sd["step"])

    # -- the order, on the host -------------------------------------------------------------------------------------------------
    @staticmethod
    def indices(n, batch, seed, step, rank=0, world=1, steps_per_epoch=None, shuffle=True):
        """numpy int64 (batch,): the rows that the fetch of step `step` writes into ``index`` -- the definition of include/spv.h
        restated on the host (no device, no library)"""
        n, batch, rank, world = int(n), int(batch), int(rank), int(world)
        steps = (n // world) // batch if steps_per_epoch is None else int(steps_per_epoch)
        if not (1 <= n < 2 ** 31 and batch >= 1 and world >= 1 and 0 <= rank < world and steps >= 1 and steps * batch * world <= n):
            raise ValueError(f"no such order: n={n}, batch={batch}, rank={rank}, world={world}, steps_per_epoch={steps}")
        t = int(step) & _U64
        pos = np.array([((t % steps) * batch + r) * world + rank for r in range(batch)], dtype=np.uint64)
        if shuffle:
            pos = _permute(_mix64(_mix64((int(seed) & _U64) + _GOLDEN) + t // steps), n, pos)
        return pos.astype(np.int64)
