"""spectre_vit.datasets on the host: every format round-trips through files written in the real on-disk formats (tests/dataset_files.py),
every refusal names its file and field, the unpickler admits a numpy array's globals and nothing else, the measured mean / std rule is
held to numpy float64, the harness's data arguments are checked before a device is touched, and the new C-ABI symbols are declared,
bound and registered."""
import gzip
import os
import re
import struct

import numpy as np
import pytest
import torch

import dataset_files as F
from conftest import ROOT

CIFAR100_CFG = "spectre_vit/configs/spectre_vit_cifar100.py"
MNIST_CFG = "spectre_vit/configs/spectre_vit_mnist.py"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def _pixels(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _labels(seed, n, classes):
    return np.random.default_rng(seed).integers(0, classes, size=n)


def _cifar100(root, n_train=7, n_test=5, module="numpy.core.multiarray"):
    splits = {"train": (_pixels(1, n_train, 3, 32, 32), _labels(2, n_train, 100)), "test": (_pixels(3, n_test, 3, 32, 32), _labels(4, n_test, 100))}
    names = [f"class_{i}" for i in range(100)]
    F.write_cifar100(str(root), splits, names, module)
    return splits, names


def _mnist(root, gz=False, n_train=9, n_test=4, side=28):
    splits = {"train": (_pixels(5, n_train, 1, side, side), _labels(6, n_train, 10)), "test": (_pixels(7, n_test, 1, side, side), _labels(8, n_test, 10))}
    F.write_mnist(str(root), splits, gz=gz)
    return splits


# ---------------------------------------------------------------- round trips
@pytest.mark.parametrize("module", ["numpy.core.multiarray", "numpy._core.multiarray"])
def test_cifar100_round_trip(tmp_path, module):
    from spectre_vit import datasets
    splits, names = _cifar100(tmp_path, module=module)
    for split, (images, labels) in splits.items():
        got, layout, got_labels, got_names, digest = datasets.load_files(str(tmp_path), "cifar100", split)
        assert layout == datasets.PLANAR and got.dtype == np.uint8 and got.shape == images.shape and (got == images).all()
        assert got_labels.dtype == np.int64 and (got_labels == labels).all() and got_names == names
        assert re.fullmatch(r"[0-9a-f]{8}", digest)
    assert datasets.load_files(str(tmp_path), "cifar100", "train")[4] != datasets.load_files(str(tmp_path), "cifar100", "test")[4]


def test_cifar10_concatenates_its_five_files_in_order(tmp_path):
    from spectre_vit import datasets
    parts = [(_pixels(10 + i, 3 + i, 3, 32, 32), _labels(20 + i, 3 + i, 10)) for i in range(5)]
    test = (_pixels(30, 4, 3, 32, 32), _labels(31, 4, 10))
    names = [f"thing_{i}" for i in range(10)]
    F.write_cifar10(str(tmp_path), parts, test, names)
    got, layout, labels, got_names, _ = datasets.load_files(str(tmp_path), "cifar10", "train")
    assert layout == datasets.PLANAR and (got == np.concatenate([p[0] for p in parts])).all()
    assert (labels == np.concatenate([p[1] for p in parts])).all() and got_names == names
    got, _, labels, _, _ = datasets.load_files(str(tmp_path), "cifar10", "test")
    assert (got == test[0]).all() and (labels == test[1]).all()


def test_mnist_raw_and_gz_give_the_same_arrays_and_digest(tmp_path):
    from spectre_vit import datasets
    raw, gz = tmp_path / "raw", tmp_path / "gz"
    splits = _mnist(raw)
    _mnist(gz, gz=True)
    assert all(name.endswith(".gz") for name in os.listdir(gz / "MNIST" / "raw"))
    for split, (images, labels) in splits.items():
        a = datasets.load_files(str(raw), "mnist", split)
        b = datasets.load_files(str(gz), "mnist", split)
        assert a[1] == datasets.PLANAR and a[0].shape == images.shape and (a[0] == images).all() and (a[2] == labels).all() and a[3] is None
        assert (b[0] == a[0]).all() and (b[2] == a[2]).all() and b[4] == a[4]
    # raw first: a raw file next to the .gz wins
    other = {"train": (_pixels(99, 9, 1, 28, 28), splits["train"][1])}
    F.write_mnist(str(gz), other)
    assert (datasets.load_files(str(gz), "mnist", "train")[0] == other["train"][0]).all()


def test_npz_round_trip(tmp_path):
    from spectre_vit import datasets
    splits = {"train": (_pixels(40, 6, 5, 7, 3), _labels(41, 6, 300)), "test": (_pixels(42, 3, 5, 7, 3), _labels(43, 3, 300))}
    F.write_npz(str(tmp_path), splits)
    for split, (images, labels) in splits.items():
        got, layout, got_labels, names, _ = datasets.load_files(str(tmp_path), "npz", split)
        assert layout == datasets.INTERLEAVED and (got == images).all() and (got_labels == labels).all() and names is None


# ---------------------------------------------------------------- the unpickler
def test_a_global_outside_the_allow_list_is_refused_by_name(tmp_path, monkeypatch):
    from spectre_vit import datasets
    _cifar100(tmp_path)
    path = tmp_path / "cifar-100-python" / "train"
    path.write_bytes(F.foreign_global_pickle("builtins", "print"))
    import builtins
    monkeypatch.setattr(builtins, "print", lambda *a, **k: pytest.fail("the refused global was called"))
    with pytest.raises(ValueError) as e:
        datasets.load_files(str(tmp_path), "cifar100", "train")
    assert str(path) in str(e.value) and "builtins.print" in str(e.value)
    for module, name in (("os", "system"), ("numpy", "load"), ("numpy.core.multiarray", "scalar")):
        path.write_bytes(F.foreign_global_pickle(module, name))
        with pytest.raises(ValueError, match=re.escape(f"{module}.{name}")):
            datasets.load_files(str(tmp_path), "cifar100", "train")
    assert datasets.PICKLE_ALLOWED == {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
                                       ("numpy", "ndarray"), ("numpy", "dtype"), ("_codecs", "encode")}


def test_a_python3_protocol2_dump_loads(tmp_path):
    """pickle.dumps(protocol=2) of bytes goes through _codecs.encode: the fifth entry of the allow-list"""
    import pickle
    from spectre_vit import datasets
    splits, names = _cifar100(tmp_path)
    images, labels = splits["train"]
    d = {b"data": images.reshape(-1, 3072), b"fine_labels": [int(v) for v in labels], b"batch_label": b"training batch 1 of 1"}
    (tmp_path / "cifar-100-python" / "train").write_bytes(pickle.dumps(d, protocol=2))
    got, _, got_labels, _, _ = datasets.load_files(str(tmp_path), "cifar100", "train")
    assert (got == images).all() and (got_labels == labels).all()


# ---------------------------------------------------------------- refusals: the file and the field
def _refused(tmp_path, dataset, split, *needles):
    from spectre_vit import datasets
    with pytest.raises(ValueError) as e:
        datasets.load_files(str(tmp_path), dataset, split)
    for needle in needles:
        assert needle in str(e.value), (needle, str(e.value))


def test_missing_files_name_every_path_tried(tmp_path):
    _refused(tmp_path, "cifar100", "train", str(tmp_path / "cifar-100-python" / "train"))
    _refused(tmp_path, "cifar10", "train", str(tmp_path / "cifar-10-batches-py" / "data_batch_1"))
    raw = str(tmp_path / "MNIST" / "raw" / "t10k-images-idx3-ubyte")
    _refused(tmp_path, "mnist", "test", raw + ",", raw + ".gz")
    _refused(tmp_path, "npz", "test", str(tmp_path / "test.npz"))
    _cifar100(tmp_path)
    os.remove(tmp_path / "cifar-100-python" / "meta")
    _refused(tmp_path, "cifar100", "train", str(tmp_path / "cifar-100-python" / "meta"))
    from spectre_vit import datasets
    with pytest.raises(ValueError, match="dataset='imagenet'"):
        datasets.load_files(str(tmp_path), "imagenet", "train")
    with pytest.raises(ValueError, match="split='val'"):
        datasets.load_files(str(tmp_path), "cifar100", "val")


def test_idx_refusals(tmp_path):
    splits = _mnist(tmp_path)
    images, labels = splits["train"]
    raw = tmp_path / "MNIST" / "raw"
    ipath, lpath = raw / "train-images-idx3-ubyte", raw / "train-labels-idx1-ubyte"
    good_i, good_l = ipath.read_bytes(), lpath.read_bytes()
    ipath.write_bytes(struct.pack(">I", 0x00000801) + good_i[4:])
    _refused(tmp_path, "mnist", "train", str(ipath), "bad magic 0x00000801", "0x00000803")
    ipath.write_bytes(good_i[:-5])
    _refused(tmp_path, "mnist", "train", str(ipath), "truncated payload")
    ipath.write_bytes(good_i[:10])
    _refused(tmp_path, "mnist", "train", str(ipath), "truncated header")
    ipath.write_bytes(good_i + b"\0" * 3)
    _refused(tmp_path, "mnist", "train", str(ipath), "count = 9 disagrees with the payload length")
    ipath.write_bytes(good_i)
    lpath.write_bytes(struct.pack(">I", 0x00000803) + good_l[4:])
    _refused(tmp_path, "mnist", "train", str(lpath), "bad magic")
    lpath.write_bytes(good_l[:-1])
    _refused(tmp_path, "mnist", "train", str(lpath), "truncated payload")
    lpath.write_bytes(F.idx_bytes(labels[:-1], 0x00000801))
    _refused(tmp_path, "mnist", "train", str(lpath), "len(labels) = 8 != N = 9")
    os.remove(ipath)
    (raw / "train-images-idx3-ubyte.gz").write_bytes(gzip.compress(good_i)[:-20])
    _refused(tmp_path, "mnist", "train", str(ipath) + ".gz", "gzip")


def test_cifar_refusals(tmp_path):
    splits, _ = _cifar100(tmp_path)
    images, labels = splits["train"]
    path = tmp_path / "cifar-100-python" / "train"
    good = path.read_bytes()
    data = images.reshape(-1, 3072)
    path.write_bytes(good[:len(good) // 2])
    _refused(tmp_path, "cifar100", "train", str(path), "pickle")
    path.write_bytes(F.py2_pickle({"data": data, "fine_labels": list(labels[:-1])}))
    _refused(tmp_path, "cifar100", "train", str(path), "'fine_labels'", "len(labels) != N")
    path.write_bytes(F.py2_pickle({"data": data[:, :3000], "fine_labels": list(labels)}))
    _refused(tmp_path, "cifar100", "train", str(path), "'data'", "C*H*W = 3072")
    path.write_bytes(F.py2_pickle({"data": data.astype(np.float64), "fine_labels": list(labels)}))
    _refused(tmp_path, "cifar100", "train", str(path), "'data'", "float64", "uint8")
    path.write_bytes(F.py2_pickle({"data": data}))
    _refused(tmp_path, "cifar100", "train", str(path), "'fine_labels'")
    path.write_bytes(good)
    meta = tmp_path / "cifar-100-python" / "meta"
    meta.write_bytes(F.py2_pickle({"coarse_label_names": ["a"]}))
    _refused(tmp_path, "cifar100", "train", str(meta), "'fine_label_names'")


def test_npz_refusals(tmp_path):
    path = tmp_path / "train.npz"
    np.savez(path, images=np.zeros((4, 5, 7, 3), np.float32), labels=np.zeros(4, np.int64))
    _refused(tmp_path, "npz", "train", str(path), "'images'", "float32", "uint8")
    np.savez(path, images=np.zeros((4, 5, 7, 2), np.uint8), labels=np.zeros(4, np.int64))
    _refused(tmp_path, "npz", "train", str(path), "'images'", "(4, 5, 7, 2)")
    np.savez(path, images=np.zeros((4, 5, 7, 3), np.uint8), labels=np.zeros(3, np.int64))
    _refused(tmp_path, "npz", "train", str(path), "'labels'", "len(labels) != N")
    np.savez(path, images=np.zeros((4, 5, 7, 3), np.uint8))
    _refused(tmp_path, "npz", "train", str(path), "'labels'")
    np.savez(path, images=np.zeros((4, 5, 7, 3), np.uint8), labels=np.array([print, 1, 2, 3], dtype=object))
    _refused(tmp_path, "npz", "train", str(path), "pickle")   # allow_pickle=False


# ---------------------------------------------------------------- normalisation
def _ulps(a, b):
    return abs(a - b) / np.spacing(abs(b))


@pytest.mark.parametrize("shape", [(50, 3, 32, 32), (60, 1, 28, 28), (3, 3, 5, 7)])
def test_measured_mean_std_is_held_to_numpy_float64(shape):
    """The rule forms mean and population std of x / 255 from the integer sums exactly and rounds once, so it is the more exact side.
    The float64 restatement: sum(x), sum(x^2), N sum(x^2) - sum(x)^2 and 255 N are integers below 2^53 for these sets, hence exact in
    float64; the mean is ONE rounded division, the std a rounded square root (1/2 ulp) and a rounded division (1/2 ulp) -- at most
    1 1/2 ulps from the true value, and the rule itself 1/2 ulp: 4 ulps bound both with room, from the restatement's own rounding.
    numpy's mean() / std() of the float pixels add one rounding per element of a pairwise sum (about log2(N) eps relative, 2e-15
    here): they are held to 1e-13 absolute on values of order 0.3 .. 0.5."""
    from spectre_vit import datasets
    x = _pixels(sum(shape), *shape)
    ints = x.astype(np.int64)
    c, pixels = shape[1], shape[0] * shape[2] * shape[3]
    sums = [int(ints[:, k].sum()) for k in range(c)]
    sumsqs = [int((ints[:, k] ** 2).sum()) for k in range(c)]
    mean, std = datasets.mean_std_from_sums(sums, sumsqs, pixels)
    for k in range(c):
        spread = pixels * sumsqs[k] - sums[k] ** 2
        assert max(spread, pixels * sumsqs[k], sums[k] ** 2, 255 * pixels) < 2 ** 53
        want_mean = np.float64(sums[k]) / np.float64(255 * pixels)
        want_std = np.sqrt(np.float64(spread)) / np.float64(255 * pixels)
        assert _ulps(mean[k], want_mean) <= 4 and _ulps(std[k], want_std) <= 4, (k, mean[k], want_mean, std[k], want_std)
        # and numpy's own mean / std of the float pixels: the same quantities, to float64's rounding of a longer sum
        f = x[:, k].astype(np.float64) / 255.0
        assert abs(mean[k] - f.mean()) <= 1e-13 and abs(std[k] - f.std()) <= 1e-13
    assert datasets.mean_std_from_sums([0], [0], 10) == ((0.0,), (0.0,))
    assert datasets.mean_std_from_sums([2550], [255 * 2550], 10) == ((1.0,), (0.0,))
    with pytest.raises(ValueError, match="no pixel"):
        datasets.mean_std_from_sums([0], [0], 0)


def test_reference_constants_and_their_refusals(tmp_path):
    from spectre_vit import datasets, harness
    assert datasets.REFERENCE_NORM["cifar100"] == (harness.CIFAR_MEAN, harness.CIFAR_STD) == ((0.5071, 0.4867, 0.4408), (0.2675, 0.2565, 0.2761))
    assert datasets.REFERENCE_NORM["mnist"] == ((0.5,), (0.5,))
    assert datasets.resolve_normalize("cifar100", None) == "reference" and datasets.resolve_normalize("mnist", None) == "reference"
    assert datasets.resolve_normalize("cifar10", None) == "measured" and datasets.resolve_normalize("npz", None) == "measured"
    for dataset in ("cifar10", "npz"):
        with pytest.raises(ValueError, match=f"no constants for '{dataset}'"):
            datasets.resolve_normalize(dataset, "reference")
    assert datasets.resolve_normalize("npz", ([0.1, 0.2, 0.3], [1, 2, 3])) == ((0.1, 0.2, 0.3), (1.0, 2.0, 3.0))
    for bad in ("zscore", ((0.5,), (0.0,)), ((0.5, 0.5), (0.5,)), 3):
        with pytest.raises(ValueError, match="normalize="):
            datasets.resolve_normalize("mnist", bad)
    # a host-side FileDataset (device=None): read, checked, nothing uploaded
    _mnist(tmp_path)
    ds = datasets.FileDataset(str(tmp_path), "mnist", "train", None, limit=5)
    assert (len(ds), ds.split_size, ds.channels, ds.height, ds.width, ds.num_classes, ds.normalize) == (5, 9, 1, 28, 28, 10, "reference")
    assert ds.images is None and ds.class_names is None and re.fullmatch(r"[0-9a-f]{8}", ds.digest)
    with pytest.raises(ValueError, match="limit=10 is above the train split's 9 samples"):
        datasets.FileDataset(str(tmp_path), "mnist", "train", None, limit=10)
    with pytest.raises(ValueError, match="normalize names 3 channels, the images have 1"):
        datasets.FileDataset(str(tmp_path), "mnist", "train", None, normalize=((0.5,) * 3, (0.5,) * 3))
    with pytest.raises(ValueError, match="the data has 10 classes, num_classes=5"):
        datasets.FileDataset(str(tmp_path), "mnist", "train", None, num_classes=5)


def test_resident_set_is_shared_with_the_synthetic_set():
    from spectre_vit import datasets, harness
    assert issubclass(harness.SyntheticCifar, datasets.ResidentSet) and issubclass(datasets.FileDataset, datasets.ResidentSet)
    assert "index_batches" not in vars(harness.SyntheticCifar) and "batches" not in vars(harness.SyntheticCifar), "shared, not forked"


# ---------------------------------------------------------------- the harness's argument checks: before a device
@pytest.mark.parametrize("which", ["train", "train_distill"])
def test_data_arguments_are_checked_before_a_device(built, tmp_path, monkeypatch, which):
    from spectre_vit import harness
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was touched"))
    for name in ("is_available", "current_device", "synchronize", "Stream", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, lambda *a, **k: pytest.fail("a CUDA call was made"))
    fn = getattr(harness, which)
    out = str(tmp_path / "out")
    cifar, mnist, small = tmp_path / "cifar", tmp_path / "mnist", tmp_path / "small"
    _cifar100(cifar)
    _mnist(mnist)
    _mnist(small, side=20)
    monkeypatch.syspath_prepend(str(tmp_path))
    # the shipped MNIST presets keep the reference's in_channels = 3: one-channel idx files go with a config that says 1
    MNIST1 = F.write_config(tmp_path, "spectre_vit_mnist_1ch", "spectre_vit_mnist", in_channels=1)
    cases = [
        (MNIST_CFG, dict(normalize="measured"), "they need data_root"),
        (MNIST_CFG, dict(dataset="mnist"), "they need data_root"),
        ("spectre_vit/configs/spectre_branch.py", dict(data_root=str(mnist)), "names neither cifar100 nor mnist"),
        (MNIST1, dict(data_root=str(cifar), dataset="cifar100"), "holds 3 x 32 x 32 images, the config in_channels=1, img_size=28"),
        (MNIST_CFG, dict(data_root=str(mnist)), "holds 1 x 28 x 28 images, the config in_channels=3, img_size=28"),
        (MNIST1, dict(data_root=str(small)), "holds 1 x 20 x 20 images"),
        (MNIST1, dict(data_root=str(mnist), n_train=10), "n_train: limit=10 is above the train split's 9 samples"),
        (MNIST1, dict(data_root=str(mnist), n_val=5), "n_val: limit=5 is above the test split's 4 samples"),
        (MNIST1, dict(data_root=str(mnist), n_train=0), "n_train=0 must be None"),
        (MNIST1, dict(data_root=str(mnist), dataset="cifar10"), "cifar-10-batches-py"),
        (MNIST1, dict(data_root=str(tmp_path / "nowhere")), "not found; tried"),
        (CIFAR100_CFG, dict(data_root=str(cifar), dataset="cifar10", normalize="reference"), "no constants for 'cifar10'"),
    ]
    for config, kw, message in cases:
        with pytest.raises(ValueError) as e:
            fn(config, out_dir=out, **kw)
        assert message in str(e.value), (kw, str(e.value))
    # more classes in the data than the model has
    many = tmp_path / "many"
    F.write_mnist(str(many), {"train": (_pixels(1, 4, 28, 28), [0, 1, 2, 150]), "test": (_pixels(2, 4, 28, 28), [0, 1, 2, 3])})
    with pytest.raises(ValueError, match="has 151 classes, the config num_classes=100"):
        fn(MNIST1, out_dir=out, data_root=str(many))
    assert not os.path.exists(out), "a refused run leaves nothing behind"


def test_the_command_line_has_the_flags():
    from spectre_vit import harness, inference
    a = harness.build_parser().parse_args(["--data-root", "./data", "--dataset", "cifar10", "--normalize", "measured"])
    assert (a.data_root, a.dataset, a.normalize) == ("./data", "cifar10", "measured")
    a = harness.build_parser().parse_args([])
    assert (a.data_root, a.dataset, a.normalize) == (None, None, None)
    b = inference.build_parser().parse_args(["--checkpoint", "m.pt", "--data-root", "./data"])
    assert (b.data_root, b.dataset, b.split) == ("./data", None, "test")


# ---------------------------------------------------------------- the C-ABI's two new symbols
def test_symbols_are_declared_bound_and_registered(built):
    from spectre_vit import _native, timing
    header = open(os.path.join(ROOT, "include", "spv.h")).read()
    lib = _native.load()
    for name in ("spv_dataset_ingest", "spv_dataset_stats_words"):
        assert re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)) and name in _native.SIGNATURES and hasattr(lib, name)
    assert "#define SPV_DATASET_PLANAR 0" in header and "#define SPV_DATASET_INTERLEAVED 1" in header
    assert "spv_dataset_ingest" in _native._LAUNCHERS and "spv_dataset_stats_words" not in _native._LAUNCHERS
    assert "spv_dataset_ingest" in timing._WORK_MODELS, "bench.py's roofline pass brackets every launch it sees"
    assert "spv_dataset.hip" in open(os.path.join(ROOT, "vit-spectre-experiments_amd", "csrc", "Makefile")).read()
    for c, classes in ((1, 10), (3, 100), (3, 0)):
        assert _native.call("spv_dataset_stats_words", c, classes) == 2 * c + 2 + classes
    # ints in header order: label dtype, n, c, h, w, layout, classes; then the NULL-pointer mask (bit 1: dst) and the hint
    model = timing._WORK_MODELS["spv_dataset_ingest"]
    label, shape, _, bound, work = model((0, 50000, 3, 32, 32, 0, 100, 0, 0))
    assert (label, tuple(shape), bound, work) == ("dataset_ingest", (50000, 3, 32, 32), "hbm", 2.0 * 50000 * 3072)
    assert model((0, 50000, 3, 32, 32, 0, 100, 2, 0))[4] == 1.0 * 50000 * 3072, "statistics only: the payload read, nothing written"


def test_ingest_refusals_need_no_device(built):
    """bad arguments are refused on the host through spv_last_error before any launch (this test runs without a GPU)"""
    from spectre_vit import _native
    good = dict(src=256, dst=1 << 20, labels=0, label_dtype=0, stats=4096, n=4, c=3, h=5, w=7, layout=0, classes=10)
    refused = [(dict(c=2), "c = 2"), (dict(c=4), "c = 4"), (dict(h=0), "h = 0"), (dict(w=513), "w = 513"), (dict(n=-1), "n = -1"),
               (dict(n=1 << 31), "n = 2147483648"), (dict(layout=2), "src_layout = 2"), (dict(classes=-1), "classes = -1"),
               (dict(label_dtype=3), "label_dtype = 3"), (dict(stats=0), "stats"), (dict(stats=4100), "8-byte aligned"),
               (dict(src=0), "null src"), (dict(dst=300), "overlap"), (dict(dst=256), "overlap")]
    for change, message in refused:
        args = list({**good, **change}.values())
        with pytest.raises(RuntimeError) as e:
            _native.call("spv_dataset_ingest", *args, 0)
        assert "spv_dataset_ingest" in str(e.value) and message in str(e.value), (change, str(e.value))
    assert _native.call("spv_dataset_ingest", 0, 0, 0, 0, 4096, 0, 3, 5, 7, 0, 10, 0) == 0, "n == 0: nothing to launch"
