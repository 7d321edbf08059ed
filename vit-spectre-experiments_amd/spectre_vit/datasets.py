"""Real datasets for the resident path: the files torchvision leaves under ``root`` (what the reference's ``./data`` holds), read on the
host without torchvision or a network, uploaded as they are and turned into the resident uint8 set by one HIP launch per chunk.

    train_set = FileDataset("./data", "cifar100", "train", device)       # images (N, 3, 32, 32) + images_nhwc, labels, mean, std
    loader = ResidentLoader(train_set.images_nhwc, train_set.labels, 512, train_set.mean_values, train_set.std_values, seed=42)

``load_files`` is the host side: CIFAR-100 / CIFAR-10 pickles (through an unpickler that admits a numpy array's globals and nothing
else), MNIST idx files (raw or .gz) and ``{train,test}.npz`` for a user's own set.  Every failure is a ValueError naming the file and
the field; an absent file is an error with every path that was tried in it (there is no download code).  ``ResidentSet`` is what the
harness needs from a set (its SyntheticCifar has this shape); ``FileDataset`` fills one from files: a pinned staging buffer, a side
stream, ``spv_dataset_ingest`` per chunk -- the other layout written and the set's integer statistics taken in the same walk.
"""
from __future__ import annotations

import gzip
import io
import math
import os
import pickle
import struct
import zlib
from fractions import Fraction

import numpy as np
import torch

PLANAR, INTERLEAVED = "planar", "interleaved"   # (N, C, H, W) as the CIFAR / MNIST files hold it; (N, H, W, C)
DATASETS = ("cifar100", "cifar10", "mnist", "npz")
SPLITS = ("train", "test")
# the constants the reference hard-codes: CIFAR-100 train.py:109-112; MNIST repl/vit_spectre_mnist.py:127.  None: it gives none
REFERENCE_NORM = {"cifar100": ((0.5071, 0.4867, 0.4408), (0.2675, 0.2565, 0.2761)), "mnist": ((0.5,), (0.5,))}

# what a pickled numpy array needs, and nothing else (_codecs.encode: Python-3 protocol-2 dumps of bytes go through it)
PICKLE_ALLOWED = frozenset({("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"), ("numpy", "ndarray"),
                            ("numpy", "dtype"), ("_codecs", "encode")})


class _ArrayUnpickler(pickle.Unpickler):
    """refuses every global outside PICKLE_ALLOWED by name, before anything is constructed"""

    def __init__(self, file, path):
        super().__init__(file, encoding="latin1")
        self._path = path

    def find_class(self, module, name):
        if (module, name) not in PICKLE_ALLOWED:
            raise ValueError(f"{self._path}: the pickle names the global {module}.{name}, which a dataset file has no use for "
                             "(only a numpy array's globals are admitted)")
        return super().find_class(module, name)


def _first_existing(paths):
    for p in paths:
        if os.path.isfile(p):
            return p
    raise ValueError("dataset file not found; tried: " + ", ".join(paths))


def _read_pickle(path):
    path = _first_existing([path])
    with open(path, "rb") as f:
        blob = f.read()
    try:
        d = _ArrayUnpickler(io.BytesIO(blob), path).load()
    except ValueError:
        raise
    except Exception as e:   # a truncated or damaged stream
        raise ValueError(f"{path}: not a readable pickle ({type(e).__name__}: {e})") from None
    if not isinstance(d, dict):
        raise ValueError(f"{path}: the pickle holds a {type(d).__name__}, not a dict")
    return path, {(k.decode("latin1") if isinstance(k, bytes) else k): v for k, v in d.items()}


def _field(d, path, name):
    if name not in d:
        raise ValueError(f"{path}: no field {name!r} (it has {sorted(map(str, d))})")
    return d[name]


def _names(seq):
    return [s.decode("latin1") if isinstance(s, bytes) else str(s) for s in seq]


def _cifar_batch(path, label_field):
    """-> (the file's path, data uint8 (N, 3072), labels int64 (N,))"""
    path, d = _read_pickle(path)
    data = _field(d, path, "data")
    if not isinstance(data, np.ndarray) or data.dtype != np.uint8:
        raise ValueError(f"{path}: field 'data' has dtype {getattr(data, 'dtype', type(data).__name__)}, not uint8")
    if data.ndim != 2 or data.shape[1] != 3072:
        raise ValueError(f"{path}: field 'data' has rows of length {data.shape[1:] if data.ndim != 2 else data.shape[1]}, not C*H*W = 3072")
    labels = np.asarray(_field(d, path, label_field))
    if labels.ndim != 1 or labels.shape[0] != data.shape[0] or labels.dtype.kind not in "iu":
        raise ValueError(f"{path}: field {label_field!r} has {labels.shape} {labels.dtype} entries for N = {data.shape[0]} images "
                         "(len(labels) != N, or not integers)")
    return path, np.ascontiguousarray(data), labels.astype(np.int64)


def _load_cifar(root, split, folder, files, label_field, meta_file, names_field):
    crc, datas, labels = 0, [], []
    for name in files:
        _, data, lab = _cifar_batch(os.path.join(root, folder, name), label_field)
        crc = zlib.crc32(data, crc)
        datas.append(data)
        labels.append(lab)
    labels = np.concatenate(labels)
    crc = zlib.crc32(labels.astype("<i8").tobytes(), crc)
    meta_path, meta = _read_pickle(os.path.join(root, folder, meta_file))
    class_names = _names(_field(meta, meta_path, names_field))
    images = (datas[0] if len(datas) == 1 else np.concatenate(datas)).reshape(-1, 3, 32, 32)
    return images, PLANAR, labels, class_names, crc


def _read_idx(root, stem, magic, dims):
    """-> (path, the count, the further header words, the payload as a view `4 * (2 + dims)` bytes into the file's bytes)"""
    base = os.path.join(root, "MNIST", "raw", stem)
    path = _first_existing([base, base + ".gz"])
    try:
        with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
            blob = f.read()
    except (OSError, EOFError, zlib.error) as e:
        raise ValueError(f"{path}: truncated or damaged gzip stream ({type(e).__name__}: {e})") from None
    head = 4 * (2 + dims)
    if len(blob) < head:
        raise ValueError(f"{path}: truncated header: {len(blob)} bytes, {head} expected")
    words = struct.unpack(f">{2 + dims}I", blob[:head])
    if words[0] != magic:
        raise ValueError(f"{path}: bad magic 0x{words[0]:08x}, expected 0x{magic:08x}")
    return path, words[1], words[2:], np.frombuffer(blob, dtype=np.uint8, offset=head)


def _load_mnist(root, split):
    stem = "train" if split == "train" else "t10k"
    ipath, n, (rows, cols), pixels = _read_idx(root, f"{stem}-images-idx3-ubyte", 0x00000803, 2)
    if not (rows >= 1 and cols >= 1):
        raise ValueError(f"{ipath}: rows = {rows}, columns = {cols}")
    want = n * rows * cols
    if pixels.size < want:
        raise ValueError(f"{ipath}: truncated payload: {pixels.size} bytes for count = {n} images of {rows} x {cols} ({want} bytes)")
    if pixels.size != want:
        raise ValueError(f"{ipath}: the count = {n} disagrees with the payload length {pixels.size} (count * rows * columns = {want})")
    lpath, nl, _, lab = _read_idx(root, f"{stem}-labels-idx1-ubyte", 0x00000801, 0)
    if lab.size < nl:
        raise ValueError(f"{lpath}: truncated payload: {lab.size} bytes for count = {nl} labels")
    if lab.size != nl:
        raise ValueError(f"{lpath}: the count = {nl} disagrees with the payload length {lab.size}")
    if nl != n:
        raise ValueError(f"{lpath}: len(labels) = {nl} != N = {n} images in {ipath}")
    labels = lab.astype(np.int64)
    crc = zlib.crc32(labels.astype("<i8").tobytes(), zlib.crc32(pixels, 0))
    return pixels.reshape(n, 1, rows, cols), PLANAR, labels, None, crc


def _load_npz(root, split):
    path = _first_existing([os.path.join(root, f"{split}.npz")])
    try:
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files if k in ("images", "labels")}
    except ValueError as e:   # (a pickled member is refused by allow_pickle=False)
        raise ValueError(f"{path}: {e}") from None
    except Exception as e:
        raise ValueError(f"{path}: not a readable npz ({type(e).__name__}: {e})") from None
    images, labels = _field(d, path, "images"), _field(d, path, "labels")
    if images.dtype != np.uint8:
        raise ValueError(f"{path}: field 'images' has dtype {images.dtype}, not uint8")
    if images.ndim != 4 or images.shape[3] not in (1, 3):
        raise ValueError(f"{path}: field 'images' has shape {images.shape}, not (N, H, W, C) with C of 1 or 3 (a row length other than C*H*W)")
    if labels.ndim != 1 or labels.shape[0] != images.shape[0] or labels.dtype.kind not in "iu":
        raise ValueError(f"{path}: field 'labels' has {labels.shape} {labels.dtype} entries for N = {images.shape[0]} images "
                         "(len(labels) != N, or not integers)")
    images, labels = np.ascontiguousarray(images), labels.astype(np.int64)
    crc = zlib.crc32(labels.astype("<i8").tobytes(), zlib.crc32(images, 0))
    return images, INTERLEAVED, labels, None, crc


def load_files(root, dataset, split):
    """-> (images uint8 ndarray, layout, labels int64 ndarray, class_names | None, digest).  images is (N, C, H, W) with layout
    "planar" (cifar100, cifar10, mnist: the files' own order) or (N, H, W, C) with "interleaved" (npz).  digest: the CRC-32, as eight
    hex digits, of the image bytes and then the labels (as little-endian int64), formed from what was read."""
    if dataset not in DATASETS:
        raise ValueError(f"dataset={dataset!r}: one of {DATASETS}")
    if split not in SPLITS:
        raise ValueError(f"split={split!r}: one of {SPLITS}")
    root = os.fspath(root)
    if dataset == "cifar100":
        out = _load_cifar(root, split, "cifar-100-python", [split], "fine_labels", "meta", "fine_label_names")
    elif dataset == "cifar10":
        files = [f"data_batch_{i}" for i in range(1, 6)] if split == "train" else ["test_batch"]
        out = _load_cifar(root, split, "cifar-10-batches-py", files, "labels", "batches.meta", "label_names")
    elif dataset == "mnist":
        out = _load_mnist(root, split)
    else:
        out = _load_npz(root, split)
    return out[:4] + (f"{out[4] & 0xFFFFFFFF:08x}",)


def mean_std_from_sums(sums, sumsqs, pixels):
    """per channel, from the integer sums of x and x^2 over `pixels` 8-bit values: the mean and the population standard deviation of
    x / 255, formed in exact rational arithmetic and rounded once to a float each -> (means, stds)"""
    if pixels <= 0:
        raise ValueError("no pixel was counted: the mean and the standard deviation of an empty set are not defined")
    means, stds = [], []
    for s, q in zip(sums, sumsqs):
        s, q = int(s), int(q)
        means.append(float(Fraction(s, 255 * pixels)))
        # sqrt((N q - s^2) / (255 N)^2): the integer square root of the numerator scaled by 2^256 is exact to 2^-128 of the root
        root = math.isqrt((pixels * q - s * s) << 256)
        stds.append(float(Fraction(root, (255 * pixels) << 128)))
    return tuple(means), tuple(stds)


def dataset_of_config(config_path):
    """dataset left unsaid: *cifar100* in the config's file name gives "cifar100", *mnist* gives "mnist", anything else is refused"""
    name = os.path.basename(os.fspath(config_path)).lower()
    for dataset in ("cifar100", "mnist"):
        if dataset in name:
            return dataset
    raise ValueError(f"dataset=None: the config's file name {name!r} names neither cifar100 nor mnist; say dataset= ({', '.join(DATASETS)})")


def resolve_normalize(dataset, normalize):
    """normalize=None: "reference" where the reference has constants, "measured" otherwise -> "reference", "measured" or a checked
    ((mean, ...), (std, ...)) pair"""
    if normalize is None:
        return "reference" if dataset in REFERENCE_NORM else "measured"
    if normalize == "reference":
        if dataset not in REFERENCE_NORM:
            raise ValueError(f"normalize='reference': the reference gives no constants for {dataset!r}; use 'measured' or (mean, std)")
        return normalize
    if normalize == "measured":
        return normalize
    try:
        mean, std = normalize
        mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
    except (TypeError, ValueError):
        raise ValueError(f"normalize={normalize!r}: 'reference', 'measured' or a (mean, std) pair of per-channel tuples") from None
    if len(mean) != len(std) or not mean or min(std) <= 0.0:
        raise ValueError(f"normalize={normalize!r}: mean and std name one value per channel, every std positive")
    return mean, std


class ResidentSet:
    """What the harness needs from a set: ``images`` (uint8 NCHW, on the device), ``labels`` (uint8 when num_classes <= 256, else
    int64), ``mean`` / ``std`` shaped (1, C, 1, 1), and the two batch iterators.  A set may also carry ``images_nhwc`` (the same
    pixels as uint8 NHWC; None: formed on demand), ``class_names``, ``digest`` and ``stats``."""
    images_nhwc = None
    class_names = None
    digest = None
    stats = None

    def nhwc(self):
        """the set as contiguous uint8 NHWC: the resident copy where the set has one"""
        return self.images_nhwc if self.images_nhwc is not None else self.images.permute(0, 2, 3, 1).contiguous()

    def index_batches(self, batch_size, shuffle, generator=None, rank=0, world=1, drop_last=True):
        """the row indices (int64, on the set's device) of every batch of one pass, in the order `batches` draws them"""
        n = self.images.shape[0]
        idx = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
        idx = idx[rank::world].to(self.images.device)
        stop = idx.numel() - batch_size + 1 if drop_last else idx.numel()
        for i in range(0, stop, batch_size):
            yield idx[i:i + batch_size]

    def batches(self, batch_size, shuffle, generator=None, rank=0, world=1, raw_uint8=False, drop_last=True):
        """raw_uint8: yield the uint8 NHWC batch itself; the model's patch gather normalises it.
        drop_last=False (validation): the short tail batch is yielded too, so every sample of the rank's shard is seen
        (the reference's DataLoader default, train.py:151-155)."""
        for sel in self.index_batches(batch_size, shuffle, generator, rank, world, drop_last):
            if raw_uint8:
                if self.images_nhwc is not None:
                    yield self.images_nhwc[sel], self.labels[sel]
                else:
                    yield self.images[sel].permute(0, 2, 3, 1).contiguous(), self.labels[sel]
                continue
            img = (self.images[sel].float() / 255.0 - self.mean) / self.std
            yield img, self.labels[sel]


class FileDataset(ResidentSet):
    """One split of a dataset on disk as a resident set.

    root, dataset, split   as load_files
    device                 where the set lives; None: the files are read and checked and nothing else happens until ``upload(device)``
    normalize              "reference": the constants the reference hard-codes (cifar100, mnist; refused for cifar10 and npz);
                           "measured": the mean and population standard deviation of the TRAIN split's pixels / 255, from the ingest
                           kernel's integer sums (a test split takes the train split's values: ``upload(measured_from=train_set)``, or
                           the train files are read and walked, statistics only); a (mean, std) pair; None: "reference" where there
                           is one, else "measured"
    limit                  keep the first `limit` samples
    chunk_images           images per uploaded chunk (the pinned staging buffer's size)
    num_classes            the width of the label histogram; None: the count of class names, or 1 + the largest label without names

    A set with a label outside [0, num_classes) is refused.  ``stats``: {"sum", "sumsq", "pixels", "labels_out_of_range",
    "histogram"} as Python integers, from the kernel's block."""

    def __init__(self, root, dataset, split, device=None, normalize=None, limit=None, chunk_images=8192, num_classes=None):
        self.normalize = resolve_normalize(dataset, normalize)
        if isinstance(chunk_images, bool) or not isinstance(chunk_images, int) or chunk_images < 1:
            raise ValueError(f"chunk_images={chunk_images!r} must be an int >= 1")
        images, layout, labels, self.class_names, self.digest = load_files(root, dataset, split)
        self.root, self.dataset, self.split, self.layout, self.chunk_images = os.fspath(root), dataset, split, layout, chunk_images
        self.split_size = images.shape[0]
        if limit is not None:
            if isinstance(limit, bool) or not isinstance(limit, int) or limit < 1:
                raise ValueError(f"limit={limit!r} must be None or an int >= 1")
            if limit > images.shape[0]:
                raise ValueError(f"limit={limit} is above the {split} split's {images.shape[0]} samples ({self.root}, {dataset})")
            images, labels = images[:limit], labels[:limit]
        self.limit = limit
        n = images.shape[0]
        if layout == PLANAR:
            _, self.channels, self.height, self.width = images.shape
        else:
            _, self.height, self.width, self.channels = images.shape
        if self.channels not in (1, 3) or not (1 <= self.height <= 512 and 1 <= self.width <= 512) or not 1 <= n < 2 ** 31:
            raise ValueError(f"{self.root} ({dataset}, {split}): {n} images of {self.channels} x {self.height} x {self.width}: the resident "
                             "path takes 1 or 3 channels, sides 1 .. 512 and 1 <= N < 2^31")
        if self.normalize not in ("reference", "measured") and len(self.normalize[0]) != self.channels:
            raise ValueError(f"normalize names {len(self.normalize[0])} channels, the images have {self.channels}")
        own = len(self.class_names) if self.class_names is not None else max(int(labels.max()) + 1, 1)
        self.num_classes = own if num_classes is None else int(num_classes)
        if not 1 <= self.num_classes <= 1 << 24 or own > self.num_classes:
            raise ValueError(f"{self.root} ({dataset}, {split}): the data has {own} classes, num_classes={self.num_classes}")
        self._host = (images, labels)
        self.images = self.labels = self.mean = self.std = self.mean_values = self.std_values = None
        if device is not None:
            self.upload(device)

    def __len__(self):
        return self._host[0].shape[0] if self._host is not None else self.images.shape[0]

    def _ingest(self, device, images, labels, keep):
        """upload `images` chunk by chunk on a side stream and run the ingest kernel on every chunk into ONE statistics block;
        keep=False: statistics only (a chunk-sized device buffer, no second layout).  -> (uploaded, written, device labels, stats)"""
        from spectre_vit import _native
        from spectre_vit._launch import _require_gpu
        n, C, H, W = images.shape[0], self.channels, self.height, self.width
        per = C * H * W
        flat = images.reshape(n, per)
        chunk = min(self.chunk_images, n)
        words = int(_native.call("spv_dataset_stats_words", C, self.num_classes))
        label_dtype = torch.uint8 if self.num_classes <= 256 else torch.int64
        if label_dtype == torch.uint8 and ((labels < 0) | (labels > 255)).any():   # (a byte could not even hold it)
            raise ValueError(f"{self.root} ({self.dataset}, {self.split}): a label outside [0, {self.num_classes})")
        host_labels = torch.from_numpy(np.ascontiguousarray(labels if label_dtype == torch.int64 else labels.astype(np.uint8)))
        side = torch.cuda.Stream(device)
        with torch.cuda.stream(side):
            stats = torch.zeros(words, dtype=torch.int64, device=device)
            dev_labels = host_labels.to(device)
            uploaded = torch.empty((n if keep else chunk, per), dtype=torch.uint8, device=device)
            written = torch.empty((n, per), dtype=torch.uint8, device=device) if keep else None
            _require_gpu(uploaded, stats)
            pinned = [torch.empty((chunk, per), dtype=torch.uint8).pin_memory() for _ in range(2)]
            free = [None, None]   # the event after which a staging buffer may be refilled
            src_layout = 0 if self.layout == PLANAR else 1   # SPV_DATASET_PLANAR / SPV_DATASET_INTERLEAVED
            for k, at in enumerate(range(0, n, chunk)):
                rows = min(chunk, n - at)
                stage = pinned[k % 2]
                if free[k % 2] is not None:
                    free[k % 2].synchronize()
                stage[:rows].numpy()[...] = flat[at:at + rows]
                target = uploaded[at:at + rows] if keep else uploaded[:rows]
                target.copy_(stage[:rows], non_blocking=True)
                free[k % 2] = torch.cuda.Event()
                free[k % 2].record(side)
                _native.call("spv_dataset_ingest", target.data_ptr(), written[at:at + rows].data_ptr() if keep else 0,
                             dev_labels.data_ptr() + at * dev_labels.element_size(), 0 if label_dtype == torch.uint8 else 1,
                             stats.data_ptr(), rows, C, H, W, src_layout, self.num_classes, side.cuda_stream)
        torch.cuda.current_stream(device).wait_stream(side)   # joined before first use
        for t in (stats, dev_labels, uploaded, written):
            if t is not None:
                t.record_stream(torch.cuda.current_stream(device))
        block = [int(v) & (2 ** 64 - 1) for v in stats.tolist()]
        out = {"sum": block[:C], "sumsq": block[C:2 * C], "pixels": block[2 * C], "labels_out_of_range": block[2 * C + 1],
               "histogram": block[2 * C + 2:]}
        return uploaded, written, dev_labels, out

    def upload(self, device, measured_from=None):
        """the device side; measured_from: the uploaded train set whose measured values a test split takes.  -> self"""
        if self._host is None:
            raise RuntimeError("this FileDataset is already on its device")
        device = torch.device(device)
        images, labels = self._host
        n, C, H, W = images.shape[0], self.channels, self.height, self.width
        uploaded, written, dev_labels, self.stats = self._ingest(device, images, labels, keep=True)
        if self.stats["labels_out_of_range"]:
            raise ValueError(f"{self.root} ({self.dataset}, {self.split}): {self.stats['labels_out_of_range']} labels lie outside "
                             f"[0, {self.num_classes})")
        if self.stats["pixels"] != n * H * W:
            raise RuntimeError(f"the ingest kernel counted {self.stats['pixels']} pixels per channel of {n * H * W}")
        planar, inter = (uploaded, written) if self.layout == PLANAR else (written, uploaded)
        self.images, self.images_nhwc, self.labels = planar.view(n, C, H, W), inter.view(n, H, W, C), dev_labels
        if self.normalize == "reference":
            mean, std = REFERENCE_NORM[self.dataset]
        elif self.normalize == "measured":
            if self.split == "train":
                mean, std = mean_std_from_sums(self.stats["sum"], self.stats["sumsq"], self.stats["pixels"])
            elif measured_from is not None:
                mean, std = measured_from.mean_values, measured_from.std_values
            else:   # the train split's values: its files read and walked, statistics only
                train = FileDataset(self.root, self.dataset, "train", None, "measured", None, self.chunk_images, self.num_classes)
                s = train._ingest(device, *train._host, keep=False)[3]
                mean, std = mean_std_from_sums(s["sum"], s["sumsq"], s["pixels"])
        else:
            mean, std = self.normalize
        if len(mean) != C:
            raise ValueError(f"the normalisation names {len(mean)} channels, the images have {C}")
        self.mean_values, self.std_values = tuple(mean), tuple(std)
        self.mean = torch.tensor(self.mean_values, device=device).view(1, -1, 1, 1)
        self.std = torch.tensor(self.std_values, device=device).view(1, -1, 1, 1)
        self._host = None
        return self
