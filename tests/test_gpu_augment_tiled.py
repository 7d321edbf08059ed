"""GPU checks of the tiled augmentation path (csrc/spv_augment_tiled.hip through spectre_vit.augment.TrainAugment(kernel="tiled") and the
"auto" dispatch): spv_augment_tiled_u8 with explicit parameter tables against the float64 restatement tests/augment_ref.py on the tables
of tests/augment_tiled_cases.py, and harness.train / train_distill on a 64-pixel config.

Tolerance: the rule of tests/test_gpu_augment.py, measured per comparison.  The restatement runs a second time in numpy float32 and the
kernel is allowed 4 x the largest |float32 - float64| over the compared pixels.  On top of it (a) that allowance must itself stay below
1.4e-3, a tenth of one 8-bit step of the normalised image (1 / (255 * 0.2761) / 10): a gather that differed between the two numpy runs
would inflate it to O(0.1) and hide anything; (b) the pixels left out are only rotation ties (augment_ref.TIE) and, under a blur,
their 3 x 3 neighbourhood, at most 1 % / 5 % of the batch (tests/test_augment_tiled.py holds the restatement to that on these tables
without a GPU); with no rotation every pixel is compared.  Every comparison prints its figures before it asserts (pytest -s)."""
import sys

import numpy as np
import pytest
import torch

import augment_ref as R
import augment_tiled_cases as T

pytestmark = pytest.mark.gpu

CASES = {name: (shape, build) for name, shape, build in T.all_cases()}


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def count():
    from spectre_vit import _native
    return _native.call("spv_path_count", _native.PATH["augment"])


def make_aug(C, kernel="tiled", **kw):
    from spectre_vit.augment import TrainAugment
    return TrainAugment(T.MEAN[:C], T.STD[:C], kernel=kernel, **kw)


def norm_of(C):
    return tuple(t.cpu().numpy() for t in make_aug(C).norm(dev()))


def launch(imgs, index, params, shape, kernel="tiled"):
    d = dev()
    aug = make_aug(shape[0], kernel)
    before = count()
    out = aug(torch.from_numpy(imgs).to(d), None if index is None else torch.from_numpy(np.asarray(index, np.int64)).to(d),
              params=torch.from_numpy(params).to(d))
    assert count() == before + 1, "the census slot counts one per call, whichever kernel serves it"
    return out.cpu().numpy()


def compare(out, imgs, index, params, shape, what):
    """hold a kernel's output to the float64 restatement under the float32-run tolerance.  Returns (ref64, left_out)."""
    C, H, W = shape
    mean, inv_std = norm_of(C)
    ref64, left = R.apply(imgs, index, params, mean, inv_std, np.float64)
    ref32, _ = R.apply(imgs, index, params, mean, inv_std, np.float32)
    assert out.shape == ref64.shape == (params.shape[0], C, H, W) and out.dtype == np.float32
    share, cap = float(left.mean()), T.cap_of(params)
    assert np.array_equal(left, T.left_out(params, shape)), "left out: rotation ties and their blur neighbourhood, nothing else"
    assert share <= cap, f"{what}: {100 * share:.2f} % of pixels left out, cap {100 * cap:.0f} %"
    keep = np.broadcast_to(~left[:, None], out.shape)
    tol = 4.0 * float(np.abs(ref32.astype(np.float64) - ref64)[keep].max())
    err = float(np.abs(out.astype(np.float64) - ref64)[keep].max())
    print(f"{what}: max |kernel - f64| {err:.3e}, allowed 4 x max |f32 - f64| = {tol:.3e}, left out {100 * share:.3f} %")
    assert tol < T.ALLOWANCE_CAP, f"{what}: the allowance {tol:.3e} is itself above a tenth of an 8-bit step"
    assert np.isfinite(out).all()
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return ref64, left


def check_exact_pixels(out, params, shape, left):
    """erased pixels are exactly 0; pixels the rotation fills with zero are exactly (0 - mean) * inv_std as fp32 computes it (those
    of a blurred sample excepted: the blur mixes them with their neighbours) unless erased"""
    C, H, W = shape
    mean, inv_std = norm_of(C)
    fill = (np.float32(0) - mean) * inv_std
    erased_px = filled_px = 0
    for b, p in enumerate(params):
        i, j, h, w = (int(p[k]) for k in (R.ERASE_I, R.ERASE_J, R.ERASE_H, R.ERASE_W))
        erased = np.zeros((H, W), bool)
        if h > 0 and w > 0:
            erased[i:i + h, j:j + w] = True
            assert (out[b][:, erased] == 0).all(), b
            erased_px += int(erased.sum())
        if p[R.ANGLE] != 0 and p[R.BLUR] == 0:
            sx, sy = R.rotation_source(float(p[R.ANGLE]), H, W)
            outside = ((np.floor(sx) < 0) | (np.floor(sx) >= W) | (np.floor(sy) < 0) | (np.floor(sy) >= H)) & ~left[b] & ~erased
            assert (out[b][:, outside] == fill[:, None]).all(), b
            filled_px += int(outside.sum())
    return erased_px, filled_px


@pytest.mark.parametrize("name", list(CASES))
def test_tiled_kernel_against_the_restatement(name):
    shape, build = CASES[name]
    imgs, index, params = build()
    out = launch(imgs, index, params, shape)
    ref, left = compare(out, imgs, index, params, shape, name)
    erased_px, filled_px = check_exact_pixels(out, params, shape, left)
    kind = name.split("-")[0]
    if kind == "erase":
        assert erased_px > 0
    if kind == "rotate":
        assert filled_px > 100
    if kind == "orders" and shape[0] == 3:
        assert len({out[o].tobytes() for o in range(24)}) == 24, "the orders differ from one another on the same image"
    if kind == "identity":
        C = shape[0]
        mean, std = np.array(T.MEAN[:C], np.float64), np.array(T.STD[:C], np.float64)
        want = (np.transpose(imgs, (0, 3, 1, 2)) / 255.0 - mean[None, :, None, None]) / std[None, :, None, None]
        assert np.abs(ref - want).max() < 1e-6
    # two calls give equal bits
    if kind in ("chain", "orders"):
        assert np.array_equal(out, launch(imgs, index, params, shape))


@pytest.mark.parametrize("shape", T.BOTH, ids=T.sid)
@pytest.mark.parametrize("kind", ["contrast", "rotate", "blur", "orders", "chain"])
def test_both_kernels_pass_on_the_same_tables(shape, kind):
    """at the sizes both kernels take, each is held to the restatement on the same table (not to the other's bits: contraction and the
    order of the mean's additions may differ); "auto" stays on the LDS kernel there"""
    name = {"orders": f"orders-{T.sid(shape)}", "chain": f"chain-{T.sid(shape)}-64-index"}.get(kind, f"{kind}-{T.sid(shape)}")
    imgs, index, params = CASES[name][1]()
    lds = launch(imgs, index, params, shape, "lds")
    compare(lds, imgs, index, params, shape, f"lds {name}")
    compare(launch(imgs, index, params, shape, "tiled"), imgs, index, params, shape, f"tiled {name}")
    assert np.array_equal(launch(imgs, index, params, shape, "auto"), lds), "auto: the LDS kernel where spv_augment_supported says so"


@pytest.mark.parametrize("shape", [(3, 64, 64), (3, 70, 45), (3, 224, 224), (1, 33, 97)], ids=T.sid)
def test_auto_takes_the_tiled_kernel_where_the_lds_kernel_refuses(shape):
    from spectre_vit import _native
    C = shape[0]
    imgs, index, params = T.case_op(shape, "contrast")
    d = dev()
    args = (torch.from_numpy(imgs).to(d), torch.from_numpy(index).to(d))
    table = torch.from_numpy(params).to(d)
    tiled = make_aug(C, "tiled")(*args, params=table)
    auto = make_aug(C, "auto")(*args, params=table)
    if _native.call("spv_augment_plan", *shape) == 2:
        assert torch.equal(auto, tiled)
        with pytest.raises(ValueError, match="does not fit"):
            make_aug(C, "lds")(*args, params=table)
    else:   # 1 x 33 x 97: both take it, auto is the LDS kernel
        assert torch.equal(auto, make_aug(C, "lds")(*args, params=table))
    with pytest.raises(ValueError, match="does not fit"):
        make_aug(C, "auto")(torch.zeros((2, 513, 64, C), dtype=torch.uint8, device=d), params=table[:2].contiguous())


@pytest.mark.parametrize("shape", [(3, 64, 64), (3, 70, 45), (3, 224, 224), (1, 33, 97)], ids=T.sid)
def test_constant_image_under_contrast_is_bit_uniform(shape):
    """contrast alone on a constant colour: f x + (1 - f) m with one m per image, so every pixel of a channel carries the same bits in
    every tile.  A mean that differed between the tiles of an image would show here and nowhere else."""
    C, H, W = shape
    imgs = np.empty((3, H, W, C), np.uint8)
    imgs[0], imgs[1], imgs[2] = (200, 100, 50)[:C], (17, 230, 99)[:C], (255, 255, 255)[:C]
    params = R.identity_params(3)
    params[:, R.CONTRAST] = 1.3
    out = launch(imgs, None, params, shape)
    compare(out, imgs, None, params, shape, f"constant colour, contrast 1.3 {shape}")
    for b in range(3):
        for c in range(C):
            assert len(np.unique(out[b, c].view(np.uint32))) == 1, (b, c)
    if C == 3:   # (one channel: the mean of a constant image is the pixel, and contrast the identity up to rounding)
        assert not np.array_equal(out, launch(imgs, None, R.identity_params(3), shape))


def test_index_outside_the_set_poisons_its_image_only():
    """the host cannot see a device index; both kernels read nothing for a row outside [0, n_src) and the tiles write NaN to its image"""
    for shape in ((3, 70, 45), (3, 64, 64)):
        imgs = T.image_set(8, shape, 6)
        index = np.array([0, -1, 3, 8, 7, 1 << 40], np.int64)
        ops = tuple(o for o in T.ALL_OPS if o != "rotate")   # contrast and blur on: the pre-pass must skip the row too
        params = T.random_table(6, shape, np.random.default_rng(1), ops)
        d = dev()
        out = make_aug(3)(torch.from_numpy(imgs).to(d), torch.from_numpy(index).to(d), params=torch.from_numpy(params).to(d)).cpu().numpy()
        assert np.isnan(out[[1, 3, 5]]).all() and np.isfinite(out[[0, 2, 4]]).all()
        good = [0, 2, 4]
        compare(out[good], imgs, index[good], params[good], shape, f"the rows beside a poisoned one {shape}")


@pytest.mark.parametrize("shape", [(3, 64, 64), (3, 224, 224)], ids=T.sid)
def test_drawn_tables_through_the_tiled_chain(shape):
    """the table spv_augment_params draws for this size, applied by __call__(step=...) and by params=: the same batch, equal to the
    restatement"""
    C, H, W = shape
    batch = 16 if T.big(shape) else 64
    aug = make_aug(C, "auto", seed=7)
    d = dev()
    imgs = T.image_set(batch + 8, shape, 5)
    x = torch.from_numpy(imgs).to(d)
    index = torch.from_numpy(np.random.default_rng(0).permutation(batch + 8)[:batch]).to(d)
    table = aug.draw(batch, 11, height=H, width=W)
    a = aug(x, index, step=11)
    b = aug(x, index, params=table)
    assert torch.equal(a, b)
    p = table.cpu().numpy()
    on = p[:, R.ERASE_H] > 0
    assert on.any() and (p[on, R.ERASE_I] + p[on, R.ERASE_H] <= H).all() and (p[on, R.ERASE_J] + p[on, R.ERASE_W] <= W).all()
    compare(a.cpu().numpy(), imgs, index.cpu().numpy(), p, shape, f"drawn table {shape}")


# ---------------------------------------------------------------- harness, on a 64-pixel config
CONFIG = '''"""Small widths on 64 x 64 images in 8 x 8 patches: 64 patches, as the CIFAR preset has"""
random_seed = 42
learning_rate = 1e-3
batch_size = 8
val_batch_size = 256
epochs = 1
num_classes = 100
patch_size = 8
img_size = 64
in_channels = 3
num_heads = 16
dropout = 0.001
hidden_dim = 768
adam_weight_decay = 0.01
adam_betas = (0.9, 0.999)
activation = "gelu"
num_encoders = 2
embed_dim = 512
num_patches = 64
use_spectre = True
spectre_threshold = 1.0
'''


@pytest.fixture()
def config64(tmp_path):
    (tmp_path / "cfg_aug_tiled_64.py").write_text(CONFIG)
    sys.path.insert(0, str(tmp_path))
    try:
        yield "cfg_aug_tiled_64.py"
    finally:
        sys.path.remove(str(tmp_path))
        sys.modules.pop("cfg_aug_tiled_64", None)


def _run(fn, tmp_path, tag, **kw):
    rec = {}

    def hook(kind, step, img, label):
        rec.setdefault(kind, []).append((step, img.detach().float().cpu().clone(), label.detach().cpu().clone()))
    _, hist = fn(out_dir=str(tmp_path / tag), log=lambda r: None, batch_hook=hook, epochs=2, steps_per_epoch=4, mixer="fft", batch_size=32,
                 n_train=256, n_val=64, **kw)
    assert len(hist) == 2 and all(r["steps"] == 4 for r in hist)
    for r in hist:
        assert all(np.isfinite(r[k]) for k in ("Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation")), r
    return rec


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_harness_train_augments_64_pixel_images(tmp_path, config64, graph):
    from spectre_vit.harness import train
    before = count()
    on1 = _run(train, tmp_path, "a", config_path=config64, augment=True, graph=graph)
    assert count() == before + 8, "one apply per training step"
    on2 = _run(train, tmp_path, "b", config_path=config64, augment=True, graph=graph)
    off = _run(train, tmp_path, "c", config_path=config64, graph=graph)
    assert count() == before + 16
    assert [s for s, _, _ in on1["train"]] == list(range(8))
    for (_, a, la), (_, b, lb), (_, c, lc) in zip(on1["train"], on2["train"], off["train"]):
        assert a.dtype == torch.float32 and a.shape == c.shape == (32, 3, 64, 64)
        assert torch.equal(a, b) and torch.equal(la, lb), "same seed: bit-equal augmented batches"
        assert torch.equal(la, lc) and not torch.equal(a, c) and torch.isfinite(a).all()
    for (_, a, la), (_, c, lc) in zip(on1["val"], off["val"]):
        assert torch.equal(a, c) and torch.equal(la, lc), "validation batches are untouched"


def test_harness_train_distill_augments_64_pixel_images(tmp_path, config64):
    from spectre_vit.harness import train_distill
    before = count()
    on1 = _run(train_distill, tmp_path, "a", config_path=config64)   # augment=True is the default
    assert count() == before + 8, "one apply per training step"
    on2 = _run(train_distill, tmp_path, "b", config_path=config64)
    off = _run(train_distill, tmp_path, "c", config_path=config64, augment=False)
    assert count() == before + 16
    for (_, a, la), (_, b, lb), (_, c, lc) in zip(on1["train"], on2["train"], off["train"]):
        assert a.shape == (32, 3, 64, 64) and torch.equal(a, b) and torch.equal(la, lb) and torch.equal(la, lc) and not torch.equal(a, c)
        assert torch.isfinite(a).all()
    assert len(on1["teacher"]) == len(off["teacher"]) == 8
    for (_, t1, _), (_, t0, _) in zip(on1["teacher"], off["teacher"]):
        assert t1.shape == (32, 3, 224, 224) and torch.equal(t1, t0), "the teacher's view is untouched by the augmentation"
