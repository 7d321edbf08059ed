"""Fixture writers for the dataset tests: files in the real on-disk formats, written from generated pixels into a test's tmp_path.

* a hand-made protocol-2 pickle in Python-2 style -- `c`-opcode globals, SHORT_BINSTRING / BINSTRING payloads, no memo -- the way cPickle
  wrote the CIFAR files (Python 3's pickler cannot be made to emit these opcodes);
* idx files (big-endian header), raw or gzip;
* npz files.
Nothing here reads a file back: the readers under test are spectre_vit.datasets'."""
import gzip
import os
import struct

import numpy as np


# ---------------------------------------------------------------- the pickle writer
def _str(b):
    if isinstance(b, str):
        b = b.encode("latin1")
    return (b"U" + bytes([len(b)]) if len(b) < 256 else b"T" + struct.pack("<i", len(b))) + b   # SHORT_BINSTRING / BINSTRING


def _int(i):
    i = int(i)
    if 0 <= i < 256:
        return b"K" + bytes([i])            # BININT1
    if 0 <= i < 65536:
        return b"M" + struct.pack("<H", i)  # BININT2
    return b"J" + struct.pack("<i", i)      # BININT


def _global(module, name):
    return b"c" + module.encode() + b"\n" + name.encode() + b"\n"


def _tuple(items):
    return b"(" + b"".join(items) + b"t"


def _list(items):
    return b"](" + b"".join(items) + b"e"   # EMPTY_LIST MARK ... APPENDS


def _array(a, module="numpy.core.multiarray"):
    """numpy's reduce of a C-contiguous array, as Python 2 wrote it: _reconstruct(ndarray, (0,), 'b') then BUILD with
    (1, shape, dtype, False, the bytes as a str)"""
    a = np.ascontiguousarray(a)
    code = {np.dtype(np.uint8): "u1", np.dtype(np.float64): "f8", np.dtype(np.int64): "i8"}[a.dtype]
    order = "|" if a.dtype.itemsize == 1 else "<"
    dtype = (_global("numpy", "dtype") + _tuple([_str(code), _int(0), _int(1)]) + b"R"
             + _tuple([_int(3), _str(order), b"N", b"N", b"N", _int(-1), _int(-1), _int(0)]) + b"b")
    new = _global(module, "_reconstruct") + _tuple([_global("numpy", "ndarray"), _tuple([_int(0)]), _str("b")]) + b"R"
    state = _tuple([_int(1), _tuple([_int(d) for d in a.shape]), dtype, b"\x89", _str(a.tobytes())])
    return new + state + b"b"


def _value(v, module):
    if isinstance(v, np.ndarray):
        return _array(v, module)
    if isinstance(v, (list, tuple)):
        return _list([_value(x, module) for x in v])
    if isinstance(v, (str, bytes)):
        return _str(v)
    return _int(v)


def py2_pickle(d, module="numpy.core.multiarray"):
    """a dict of str -> ndarray | list | str | int as a protocol-2 pickle in cPickle's style"""
    items = b"".join(_str(k) + _value(v, module) for k, v in d.items())
    return b"\x80\x02}(" + items + b"u."   # PROTO 2, EMPTY_DICT, MARK, ..., SETITEMS, STOP


def foreign_global_pickle(module="builtins", name="print"):
    """a pickle whose only content is a global outside the readers' allow-list (harmless: loading it would only hand the object back)"""
    return b"\x80\x02" + _global(module, name) + b"."


def _write(path, blob):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(blob)
    return path


# ---------------------------------------------------------------- a config module of a test's own
def write_config(directory, name, preset, **overrides):
    """A config module `name`.py holding the shipped preset's values with `overrides` on top, in a fresh package under `directory`
    (which the caller puts on sys.path) -> the slash path parse_config takes.  The shipped MNIST presets keep the reference's
    in_channels = 3 (tests/golden/configs.json holds them to it), so a run on one-channel idx files needs in_channels = 1 from here."""
    import uuid
    package = f"cfg_{uuid.uuid4().hex[:12]}"
    lines = ["from spectre_vit.configs._presets import PRESETS", f"globals().update(PRESETS[{preset!r}])"]
    lines += [f"{k} = {v!r}" for k, v in overrides.items()]   # (a preset with a __base__ key would need its base module beside it)
    _write(os.path.join(str(directory), package, "__init__.py"), b"")
    _write(os.path.join(str(directory), package, name + ".py"), ("\n".join(lines) + "\n").encode())
    return f"{package}/{name}.py"


# ---------------------------------------------------------------- the datasets
def write_cifar100(root, splits, names, module="numpy.core.multiarray"):
    """splits: {"train": (images (N, 3, 32, 32) uint8, labels), "test": ...}"""
    for split, (images, labels) in splits.items():
        d = {"filenames": [f"img_{i}.png" for i in range(len(labels))], "batch_label": f"{split}ing batch 1 of 1",
             "fine_labels": [int(v) for v in labels], "coarse_labels": [int(v) % 20 for v in labels],
             "data": np.asarray(images, dtype=np.uint8).reshape(len(labels), 3072)}
        _write(os.path.join(root, "cifar-100-python", split), py2_pickle(d, module))
    _write(os.path.join(root, "cifar-100-python", "meta"),
           py2_pickle({"fine_label_names": list(names), "coarse_label_names": [f"super_{i}" for i in range(20)]}))


def write_cifar10(root, train_parts, test, names):
    """train_parts: five (images, labels) pairs -> data_batch_1..5; test: one pair -> test_batch"""
    parts = [(f"data_batch_{i + 1}", p) for i, p in enumerate(train_parts)] + [("test_batch", test)]
    for name, (images, labels) in parts:
        d = {"batch_label": name, "labels": [int(v) for v in labels],
             "data": np.asarray(images, dtype=np.uint8).reshape(len(labels), 3072), "filenames": [f"i{i}.png" for i in range(len(labels))]}
        _write(os.path.join(root, "cifar-10-batches-py", name), py2_pickle(d))
    _write(os.path.join(root, "cifar-10-batches-py", "batches.meta"),
           py2_pickle({"num_cases_per_batch": len(train_parts[0][1]), "label_names": list(names), "num_vis": 3072}))


def idx_bytes(array, magic):
    array = np.asarray(array, dtype=np.uint8)
    return struct.pack(f">{1 + array.ndim}I", magic, *array.shape) + array.tobytes()


def write_mnist(root, splits, gz=False):
    """splits: {"train": (images (N, H, W) or (N, 1, H, W) uint8, labels), "test": ...}; gz: .gz files instead of raw ones"""
    for split, (images, labels) in splits.items():
        stem = "train" if split == "train" else "t10k"
        images = np.asarray(images, dtype=np.uint8)
        images = images.reshape(images.shape[0], images.shape[-2], images.shape[-1])
        for name, blob in ((f"{stem}-images-idx3-ubyte", idx_bytes(images, 0x00000803)),
                           (f"{stem}-labels-idx1-ubyte", idx_bytes(np.asarray(labels, dtype=np.uint8), 0x00000801))):
            _write(os.path.join(root, "MNIST", "raw", name + (".gz" if gz else "")), gzip.compress(blob) if gz else blob)


def write_npz(root, splits):
    """splits: {"train": (images (N, H, W, C) uint8, labels), "test": ...}"""
    os.makedirs(root, exist_ok=True)
    for split, (images, labels) in splits.items():
        np.savez(os.path.join(root, f"{split}.npz"), images=np.asarray(images), labels=np.asarray(labels))
