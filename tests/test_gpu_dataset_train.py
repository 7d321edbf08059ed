"""Training from dataset files, end to end: SyntheticCifar's own images and labels are written out in a real on-disk format
(tests/dataset_files.py), the harness trains from the files (data_root=...), and the run is held to its synthetic twin's BITS -- every
batch the model saw, the per-step losses, every record of history and every final weight.  What differs between the twins is the file
route alone: the reader, the chunked upload, spv_dataset_ingest's second layout, the set's own mean / std handed to the loader, the
augmentation, the teacher's view and the model's uint8 patch gather.  Then the teacher cache's tag, the fingerprint, resume, and
inference.score on a ragged test split.

The shipped MNIST presets keep the reference's in_channels = 3, so the idx case (one channel) runs the spectre_vit_mnist preset's values
with in_channels = 1 from a config module the test writes; the three-channel 28 x 28 cases go through the npz route."""
import json
import os

import numpy as np
import pytest
import torch

import dataset_files as F

pytestmark = pytest.mark.gpu

CIFAR_CFG = "spectre_vit/configs/spectre_vit_cifar100.py"
MNIST_CFG = "spectre_vit/configs/spectre_vit_mnist.py"
N_TRAIN, N_VAL, BATCH, STEPS = 128, 64, 16, 4
DATASET_KEYS = ["name", "root", "n_train", "n_val", "digest", "mean", "std"]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _synthetic(config, n, seed_offset=0, seed=42):
    """the harness's own synthetic set for `config` as numpy: (images (n, C, H, W) uint8, labels)"""
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.harness import SyntheticCifar
    ds = SyntheticCifar(n, parse_config(config), torch.device("cpu"), seed=seed + seed_offset)
    return ds.images.numpy(), ds.labels.numpy().astype(np.int64)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """the twins' files, written once: the synthetic train set (seed 42) and validation set (seed 43) of each config"""
    import sys
    base = tmp_path_factory.mktemp("data")
    sys.path.insert(0, str(base))
    out = {"base": base}
    names = [f"class_{i}" for i in range(100)]
    out["cifar100"] = str(base / "cifar100")
    F.write_cifar100(out["cifar100"], {"train": _synthetic(CIFAR_CFG, N_TRAIN), "test": _synthetic(CIFAR_CFG, N_VAL, 1)}, names)
    out["cifar100_70"] = str(base / "cifar100_70")   # a ragged test split: 70 = 2 x 32 + 6
    F.write_cifar100(out["cifar100_70"], {"train": _synthetic(CIFAR_CFG, 8), "test": _synthetic(CIFAR_CFG, 70, 1)}, names)
    out["mnist1_cfg"] = F.write_config(base, "spectre_vit_mnist_1ch", "spectre_vit_mnist", in_channels=1)
    out["mnist"] = str(base / "mnist")
    F.write_mnist(out["mnist"], {"train": _synthetic(out["mnist1_cfg"], N_TRAIN), "test": _synthetic(out["mnist1_cfg"], N_VAL, 1)}, gz=True)
    for key, seed in (("npz", 42), ("npz_other", 7)):   # three-channel 28 x 28, interleaved; "npz_other": other pixels, the same shapes
        out[key] = str(base / key)
        (tr, trl), (te, tel) = _synthetic(MNIST_CFG, N_TRAIN, 0, seed), _synthetic(MNIST_CFG, N_VAL, 1, seed)
        F.write_npz(out[key], {"train": (tr.transpose(0, 2, 3, 1), trl), "test": (te.transpose(0, 2, 3, 1), tel)})
    yield out
    sys.path.remove(str(base))


def _run(fn_name, config, out, hook=None, epochs=1, **kw):
    """-> (final weights, history, what every batch hook call saw, the lines of scalars.jsonl)"""
    from spectre_vit import harness
    seen = []

    def watch(kind, step, img, label):
        seen.append((kind, step, tuple(img.shape), float(img.double().sum()), int(label.long().sum())))
        if hook is not None:
            hook(kind, step, img, label)
    kw.setdefault("n_train", N_TRAIN)
    kw.setdefault("n_val", N_VAL)
    model, history = getattr(harness, fn_name)(config, mixer="fft", batch_size=BATCH, steps_per_epoch=STEPS, epochs=epochs, out_dir=str(out),
                                               log=lambda r: None, batch_hook=watch, **kw)
    torch.cuda.synchronize()
    lines = [json.loads(text) for text in open(os.path.join(str(out), "scalars.jsonl"))]
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, history, seen, lines


def _assert_twins(synthetic, files, root, name):
    sd_a, hist_a, seen_a, lines_a = synthetic
    sd_b, hist_b, seen_b, lines_b = files
    assert seen_b == seen_a and len(seen_a) >= STEPS, "every batch the model saw: shape, pixel sum, label sum"
    steps = lambda lines: [l for l in lines if "step" in l]   # noqa: E731
    assert steps(lines_b) == steps(lines_a), "the per-step loss lines"
    assert [{k: v for k, v in r.items() if k != "Dataset"} for r in hist_b] == hist_a, "every record of history"
    assert all("Dataset" not in r for r in hist_a), "the synthetic run's record keys are what they were"
    for rec in hist_b:
        d = rec["Dataset"]
        assert list(d) == DATASET_KEYS and (d["name"], d["root"], d["n_train"], d["n_val"]) == (name, root, N_TRAIN, N_VAL)
    assert sorted(sd_a) == sorted(sd_b)
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), f"final weight {k}"


CIFAR_CASES = {
    "eager": dict(),                                                                      # (a) host-fed eager
    "eager-uint8-graph-eval": dict(uint8_input=True, graph_eval=True),                    #     the set's values in the model's PixelNorm
    "loader-augment-graph": dict(device_loader=True, augment=True, graph=True, device_meter=True),   # (b) the one-replay step
}


@pytest.mark.parametrize("case", list(CIFAR_CASES))
def test_cifar100_pickles_train_to_the_synthetic_bits(roots, tmp_path, case):
    kw = CIFAR_CASES[case]
    synthetic = _run("train", CIFAR_CFG, tmp_path / "synthetic", **kw)
    files = _run("train", CIFAR_CFG, tmp_path / "files", data_root=roots["cifar100"], n_train=None, n_val=None, **kw)
    _assert_twins(synthetic, files, roots["cifar100"], "cifar100")
    d = files[1][0]["Dataset"]
    assert d["mean"] == [0.5071, 0.4867, 0.4408] and d["std"] == [0.2675, 0.2565, 0.2761], "the reference's constants"
    if kw.get("device_meter"):
        assert len([l for l in files[3] if "step" in l]) == STEPS


def test_mnist_idx_files_train_to_the_synthetic_bits(roots, tmp_path):
    """(c) one channel, .gz idx files; normalize = the synthetic set's own constants, so the file route is the only difference"""
    from spectre_vit.harness import CIFAR_MEAN, CIFAR_STD
    cfg = roots["mnist1_cfg"]
    kw = dict(device_loader=True, augment=True)
    synthetic = _run("train", cfg, tmp_path / "synthetic", **kw)
    files = _run("train", cfg, tmp_path / "files", data_root=roots["mnist"], n_train=None, n_val=None,
                 normalize=(CIFAR_MEAN[:1], CIFAR_STD[:1]), **kw)
    _assert_twins(synthetic, files, roots["mnist"], "mnist")
    # limit: an explicit number keeps the first samples
    limited = _run("train", cfg, tmp_path / "limited", data_root=roots["mnist"], n_train=64, n_val=40,
                   normalize=(CIFAR_MEAN[:1], CIFAR_STD[:1]))
    d = limited[1][0]["Dataset"]
    assert (d["n_train"], d["n_val"], limited[1][0]["val_samples"]) == (64, 40, 40)


def test_distillation_with_a_cached_teacher_and_the_cache_tag(roots, tmp_path):
    """(d) train_distill(cache_teacher=True) from npz files equals its synthetic twin; a cache saved from one set is refused for
    another by its tag"""
    from spectre_vit.harness import CIFAR_MEAN, CIFAR_STD
    kw = dict(cache_teacher=True, graph=True, device_loader=True)
    norm = (CIFAR_MEAN, CIFAR_STD)
    synthetic = _run("train_distill", MNIST_CFG, tmp_path / "synthetic", **kw)
    cache = str(tmp_path / "teacher.pt")
    files = _run("train_distill", MNIST_CFG, tmp_path / "files", data_root=roots["npz"], dataset="npz", normalize=norm, n_train=None,
                 n_val=None, teacher_cache_path=cache, **kw)
    _assert_twins(synthetic, files, roots["npz"], "npz")
    assert os.path.exists(cache)
    again = _run("train_distill", MNIST_CFG, tmp_path / "again", data_root=roots["npz"], dataset="npz", normalize=norm, n_train=None,
                 n_val=None, teacher_cache_path=cache, **kw)
    assert [l["TeacherCache"]["loaded"] for l in again[3] if "TeacherCache" in l] == [True]
    assert all(torch.equal(files[0][k], again[0][k]) for k in files[0]), "the loaded cache serves the same run"
    with pytest.raises(ValueError, match="tag"):
        _run("train_distill", MNIST_CFG, tmp_path / "other", data_root=roots["npz_other"], dataset="npz", normalize=norm, n_train=None,
             n_val=None, teacher_cache_path=cache, **kw)
    with pytest.raises(ValueError, match="tag"):   # ... and for the synthetic set, whose tag names no files
        _run("train_distill", MNIST_CFG, tmp_path / "synthetic2", teacher_cache_path=cache, **kw)


class Preempted(Exception):
    pass


def test_fingerprint_and_resume(roots, tmp_path):
    """(e) a synthetic run's train_state.pt is refused for the file run by the first differing key; a file run interrupted and
    resumed ends on the uninterrupted file run's bits"""
    from spectre_vit.harness import CIFAR_MEAN, CIFAR_STD
    kw = dict(graph=True, device_loader=True, augment=True, checkpoint_every=1)
    data = dict(data_root=roots["npz"], dataset="npz", normalize=(CIFAR_MEAN, CIFAR_STD), n_train=None, n_val=None)
    synthetic_out = tmp_path / "synthetic"
    _run("train", MNIST_CFG, synthetic_out, epochs=2, **kw)
    state = str(synthetic_out / "train_state.pt")
    with pytest.raises(ValueError, match=r"the saved run's fingerprint differs in 'dataset': '<absent>' in the file, 'npz' in this call"):
        _run("train", MNIST_CFG, tmp_path / "refused", epochs=2, resume=state, **kw, **data)
    whole = _run("train", MNIST_CFG, tmp_path / "whole", epochs=2, **kw, **data)
    with pytest.raises(ValueError, match="fingerprint differs in 'dataset_digest'"):   # other files: refused as well
        _run("train", MNIST_CFG, tmp_path / "refused", epochs=2, resume=str(tmp_path / "whole" / "train_state.pt"), **kw,
             **{**data, "data_root": roots["npz_other"]})

    def cut(kind, step, img, label):
        if kind == "train" and step == STEPS:   # the first step of epoch 2
            raise Preempted
    with pytest.raises(Preempted):
        _run("train", MNIST_CFG, tmp_path / "cut", hook=cut, epochs=2, **kw, **data)
    resumed = _run("train", MNIST_CFG, tmp_path / "cut", epochs=2, resume=True, **kw, **data)
    assert resumed[1] == whole[1] and [r["epoch"] for r in resumed[1]] == [1, 2]
    for k in whole[0]:
        assert torch.equal(whole[0][k], resumed[0][k]), f"final weight {k}"


def test_inference_scores_a_ragged_split(roots, tmp_path):
    """(f) 70 test images in batches of 32: every sample is seen, the last batch of 6 included"""
    from spectre_vit import inference
    sd, history, _, _ = _run("train", CIFAR_CFG, tmp_path / "run", data_root=roots["cifar100"], n_train=None, n_val=None)
    ckpt = str(tmp_path / "run" / "model_best.pt")
    got = inference.score(CIFAR_CFG, ckpt, mixer="fft", batch=32, data_root=roots["cifar100_70"])
    assert got["seen"] == 70 and np.isfinite(got["loss"]) and 0.0 <= got["accuracy"] <= 1.0
    # the 64-image test split holds the synthetic validation set's pixels: the same session scores both to the same figures
    from_files = inference.score(CIFAR_CFG, ckpt, mixer="fft", batch=32, data_root=roots["cifar100"])
    synthetic = inference.score(CIFAR_CFG, ckpt, mixer="fft", batch=32, n=N_VAL)
    assert from_files["seen"] == N_VAL and all(from_files[k] == synthetic[k] for k in ("accuracy", "top5", "loss", "seen"))
    with pytest.raises(ValueError, match="they need data_root"):
        inference.score(CIFAR_CFG, ckpt, mixer="fft", dataset="cifar100")
