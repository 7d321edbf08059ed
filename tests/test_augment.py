"""CPU checks of the training augmentation (spectre_vit.augment, csrc/spv_augment.hip): the public surface, the C-ABI's refusals, and
the float64 restatement tests/augment_ref.py -- the reference of the GPU tests -- against outside anchors: PIL for flip, brightness,
contrast, saturation, grey and the rotation, the standard library's colorsys for the hue round trip.  The bounds against PIL are
quantisation bounds (PIL works on 8-bit integers and truncates its blends), not measurements.  The blur has no usable PIL counterpart
(PIL's GaussianBlur is a box approximation) and is held to its written definition only."""
import colorsys
import inspect
import os

import numpy as np
import pytest

import augment_ref as R

N_IMAGES = 400


def images(seed, n=N_IMAGES, shape=(32, 32, 3)):
    """random uint8 images with some structure: half pure noise, half smooth gradients plus noise (a flat histogram alone would never
    exercise low-saturation pixels)"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, size=(n,) + shape, dtype=np.uint8)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    for k in range(0, n, 2):
        base = rng.uniform(0, 200, size=shape[2]) + rng.uniform(-2, 2, size=shape[2]) * xx[..., None] + rng.uniform(-2, 2) * yy[..., None]
        out[k] = np.clip(base + rng.uniform(0, 30) * rng.standard_normal(shape), 0, 255).astype(np.uint8)
    return out


def chw(img):
    return np.transpose(img, (2, 0, 1)).astype(np.float64) / 255.0


def steps(x_chw, pil_img):
    """largest difference in 8-bit steps between a float (C, H, W) image in [0, 1] and a PIL image"""
    a = np.asarray(pil_img, np.float64)
    a = a[None] if a.ndim == 2 else np.transpose(a, (2, 0, 1))
    return float(np.abs(x_chw * 255.0 - a).max())


# ---------------------------------------------------------------- public surface (fails on the parent commit)
def test_train_augment_defaults_are_the_reference_recipe():
    """reference spectre_vit/repl/train.py:102-115: RandomHorizontalFlip(p=0.5), ColorJitter(0.4, 0.4, 0.4, 0.1), RandomGrayscale(p=0.2),
    RandomAffine(30), RandomApply([GaussianBlur(3)]) (p = 0.5, sigma (0.1, 2.0): torchvision's defaults), Normalize(CIFAR mean, std),
    RandomErasing(0.5) (scale (0.02, 0.33), ratio (0.3, 3.3): torchvision's defaults)."""
    from spectre_vit import harness
    from spectre_vit.augment import NPARAM, TrainAugment
    a = TrainAugment(harness.CIFAR_MEAN, harness.CIFAR_STD)
    assert (a.flip, a.jitter, a.grayscale, a.degrees) == (0.5, (0.4, 0.4, 0.4, 0.1), 0.2, 30.0)
    assert (a.blur, a.blur_sigma) == (0.5, (0.1, 2.0))
    assert (a.erase, a.erase_scale, a.erase_ratio) == (0.5, (0.02, 0.33), (0.3, 3.3))
    assert a.mean == (0.5071, 0.4867, 0.4408) and a.std == (0.2675, 0.2565, 0.2761) and a.seed == 0
    c = a.cfg()
    got = [round(getattr(c, n), 6) for n, _ in c._fields_]
    assert got == [0.5, 0.6, 1.4, 0.6, 1.4, 0.6, 1.4, -0.1, 0.1, 0.2, 30.0, 0.5, 0.1, 2.0, 0.5, 0.02, 0.33, 0.3, 3.3], got
    assert NPARAM == R.NPARAM == 16
    off = TrainAugment((0.5,), (0.5,), flip=0, jitter=(0, 0, 0, 0), grayscale=0, degrees=0, blur=0, erase=0).cfg()
    assert (off.bright_lo, off.bright_hi, off.hue_lo, off.hue_hi, off.degrees, off.flip_p) == (1.0, 1.0, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        TrainAugment((0.5, 0.5), (0.5, 0.5))
    with pytest.raises(ValueError):
        a(None, step=0, params=0)   # exactly one of step and params


def test_harness_train_accepts_augment():
    from spectre_vit import harness
    sig = inspect.signature(harness.train)
    assert sig.parameters["augment"].default is False
    assert harness.augment_seed(42, 0) == 42 and harness.augment_seed(42, 1) == 42 + (1 << 32)
    assert harness.augment_seed(42, 0) != harness.augment_seed(42, 1)
    for kw in (dict(uint8_input=True), dict(distill=True)):   # refused before anything touches a device
        with pytest.raises(ValueError, match="augment"):
            harness.train("spectre_vit/configs/spectre_vit_mnist.py", augment=True, **kw)


def test_index_batches_are_the_batches_rows():
    import types
    import torch
    from spectre_vit.harness import SyntheticCifar
    c = types.SimpleNamespace(num_classes=10, in_channels=3, img_size=8)
    ds = SyntheticCifar(200, c, torch.device("cpu"), seed=3)
    idx = list(ds.index_batches(64, True, torch.Generator().manual_seed(5), 1, 2))
    got = list(ds.batches(64, True, torch.Generator().manual_seed(5), 1, 2, raw_uint8=True))
    assert len(idx) == len(got) == 1 and idx[0].dtype == torch.int64
    for sel, (img, lab) in zip(idx, got):
        assert torch.equal(ds.images[sel].permute(0, 2, 3, 1), img) and torch.equal(ds.labels[sel], lab)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_census_index_and_support(built):
    import re
    from conftest import ROOT
    from spectre_vit import _native
    hdr = open(os.path.join(ROOT, "include", "spv.h")).read()
    enum = dict(re.findall(r"(SPV_PATH_[A-Z0-9_]+)\s*=\s*(\d+)", hdr))
    assert int(enum["SPV_PATH_AUGMENT"]) == _native.PATH["augment"] == 22 < int(enum["SPV_PATH_COUNT"])
    assert int(re.search(r"#define SPV_AUG_NPARAM (\d+)", hdr).group(1)) == R.NPARAM
    for name in ("FLIP", "BRIGHT", "CONTRAST", "SAT", "HUE", "ORDER", "GRAY", "ANGLE", "BLUR", "SIGMA", "ERASE_I", "ERASE_J", "ERASE_H",
                 "ERASE_W"):
        assert int(re.search(rf"#define SPV_AUG_{name} (\d+)", hdr).group(1)) == getattr(R, name), name
    sup = lambda c, h, w: _native.call("spv_augment_supported", c, h, w)
    assert sup(3, 32, 32) == 1 and sup(1, 28, 28) == 1
    assert sup(3, 224, 224) == 0 and sup(1, 224, 224) == 0 and sup(2, 32, 32) == 0 and sup(3, 1, 32) == 0 and sup(3, 0, 0) == 0


def test_augment_entry_points_reject_bad_arguments_before_any_launch(built):
    """Every call fails validation on the host: nothing is launched (no GPU here).  An index outside the set is NOT among them: the index
    lives on the device and calls never synchronise, so the host cannot see it (the kernel writes NaN to such a row's image)."""
    import ctypes
    from spectre_vit import _native
    from spectre_vit.augment import TrainAugment
    cfg = TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2)).cfg()
    pc = ctypes.addressof(cfg)
    bad_p = TrainAugment((0.5,), (0.2,)).cfg()
    bad_p.blur_p = 1.5
    bad_r = TrainAugment((0.5,), (0.2,)).cfg()
    bad_r.sigma_lo = 0.0
    cases = [
        ("spv_augment_u8", (16, 0, 16, 16, 16, 16, 4, 8, 3, 224, 224, 0), "not supported"),
        ("spv_augment_u8", (16, 0, 16, 16, 16, 16, 4, 8, 2, 32, 32, 0), "not supported"),
        ("spv_augment_u8", (16, 0, 0, 16, 16, 16, 4, 8, 3, 32, 32, 0), "params"),
        ("spv_augment_u8", (16, 0, 16, 0, 16, 16, 4, 8, 3, 32, 32, 0), "mean"),
        ("spv_augment_u8", (0, 0, 16, 16, 16, 16, 4, 8, 3, 32, 32, 0), "src"),
        ("spv_augment_u8", (16, 0, 16, 16, 16, 16, 0, 8, 3, 32, 32, 0), "bad shape"),
        ("spv_augment_u8", (16, 0, 16, 16, 16, 16, 9, 8, 3, 32, 32, 0), "n_src"),
        ("spv_augment_params", (0, 4, 3, 32, 32, pc, 0, 0, 0), "params"),
        ("spv_augment_params", (16, 4, 3, 32, 32, 0, 0, 0, 0), "cfg"),
        ("spv_augment_params", (16, 0, 3, 32, 32, pc, 0, 0, 0), "bad shape"),
        ("spv_augment_params", (16, 4, 3, 32, 32, ctypes.addressof(bad_p), 0, 0, 0), "probability"),
        ("spv_augment_params", (16, 4, 3, 32, 32, ctypes.addressof(bad_r), 0, 0, 0), "range"),
    ]
    for name, args, needle in cases:
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, needle, str(e.value))


# ---------------------------------------------------------------- the restatement against PIL / colorsys
def test_order_index_is_lexicographic():
    assert R.order_of(0) == (0, 1, 2, 3) and R.order_of(1) == (0, 1, 3, 2) and R.order_of(6) == (1, 0, 2, 3) and R.order_of(23) == (3, 2, 1, 0)
    assert len({R.order_of(i) for i in range(24)}) == 24


def test_flip_brightness_contrast_saturation_grey_against_pil():
    from PIL import Image, ImageEnhance, ImageOps
    rng = np.random.default_rng(11)
    worst = dict(brightness=0.0, contrast=0.0, saturation=0.0, grey=0.0)
    for img in images(1):
        pil = Image.fromarray(img)
        x = chw(img)
        assert np.array_equal(np.rint(x[:, :, ::-1] * 255).astype(np.uint8), np.transpose(np.asarray(ImageOps.mirror(pil)), (2, 0, 1)))
        f = rng.uniform(0.6, 1.4)
        worst["brightness"] = max(worst["brightness"], steps(R.brightness(x, f), ImageEnhance.Brightness(pil).enhance(f)))
        worst["contrast"] = max(worst["contrast"], steps(R.contrast(x, f), ImageEnhance.Contrast(pil).enhance(f)))
        worst["saturation"] = max(worst["saturation"], steps(R.saturation(x, f), ImageEnhance.Color(pil).enhance(f)))
        worst["grey"] = max(worst["grey"], steps(R.grey(x)[None], pil.convert("L")))
    print("largest differences in 8-bit steps:", worst)
    assert worst["brightness"] <= 1.0 + 1e-9, worst     # PIL truncates the blend
    assert worst["contrast"] <= 1.5, worst              # 1 (truncated blend) + |1 - f| <= 0.4 times the rounding of PIL's integer grey and mean
    assert worst["saturation"] <= 1.5, worst
    assert worst["grey"] <= 0.6, worst                  # rounding, plus 0.2989 against PIL's 0.299


def test_hue_round_trip_against_colorsys():
    """torchvision's hexcone formulas are those of the standard library: the restatement is held to colorsys per pixel in float64"""
    rng = np.random.default_rng(5)
    px = np.concatenate([chw(images(2, 6)[k]).reshape(3, -1) for k in range(6)], axis=1)
    special = np.array([[0, 0, 0], [1, 1, 1], [.5, .5, .5], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [.3, .3, .1],
                        [.3, .1, .3], [.1, .3, .3]]).T
    px = np.concatenate([special, px, rng.uniform(0, 1, size=(3, 4000))], axis=1)
    h, s, v = R.rgb_to_hsv(px)
    want = np.array([colorsys.rgb_to_hsv(*px[:, k]) for k in range(px.shape[1])]).T
    dh = np.abs(h - want[0])
    assert np.minimum(dh, 1 - dh).max() < 1e-12 and np.abs(s - want[1]).max() < 1e-14 and np.array_equal(v, want[2])
    assert np.array_equal(R.hsv_to_rgb(want[0], want[1], want[2]), np.array([colorsys.hsv_to_rgb(*want[:, k]) for k in range(px.shape[1])]).T)
    for shift in (-0.1, -0.03, 0.07, 0.1, 0.5):
        got = R.hue(px, shift)
        ref = np.array([colorsys.hsv_to_rgb((want[0, k] + shift) % 1.0, want[1, k], want[2, k]) for k in range(px.shape[1])]).T
        assert np.abs(got - ref).max() < 1e-12, shift
    assert R.hue(px, 0.0) is px   # a zero shift is skipped, not a round trip
    one = px[:1]
    assert R.hue(one, 0.1) is one and R.saturation(one, 0.7) is one   # one channel: saturation and hue are the identity


@pytest.mark.parametrize("shape", [(32, 32, 3), (28, 28, 1)])
def test_rotation_against_pil_affine_nearest(shape):
    """Image.transform(AFFINE, NEAREST) with the six coefficients of the inverse map.  PIL's nearest path is fixed point, so pixels whose
    float64 source coordinate lies within 1e-3 of an integer are left out: at most 1 % of them, and every other pixel equal."""
    from PIL import Image
    H, W, C = shape
    rng = np.random.default_rng(3)
    imgs = images(4, 8, shape)
    left_out = total = diff_in = 0
    for k, angle in enumerate(rng.uniform(-30, 30, size=300)):
        img = imgs[k % len(imgs)]
        got, ties = R.rotate(chw(img), angle)
        got = np.rint(got * 255).astype(np.uint8)
        pil = Image.fromarray(img if C == 3 else img[..., 0])
        want = np.asarray(pil.transform((W, H), Image.AFFINE, tuple(float(v) for v in R.rotation_coefficients(angle, H, W)), Image.NEAREST))
        want = want[None] if C == 1 else np.transpose(want, (2, 0, 1))
        differ = (got != want).any(axis=0)
        diff_in += int((differ & ~ties).sum())
        left_out += int(ties.sum())
        total += H * W
    print(f"{shape}: left out {100 * left_out / total:.3f} % of pixels, different outside them: {diff_in}")
    assert left_out <= 0.01 * total, left_out / total
    assert diff_in == 0, diff_in
    # the map itself: angle 0 is the identity, the centre pixel pair stays put, corners leave the image
    assert R.rotate(chw(imgs[0]), 0.0)[0] is not None and np.array_equal(R.rotate(chw(imgs[0]), 0.0)[0], chw(imgs[0]))
    out, _ = R.rotate(np.ones((1, H, W)), 30.0)
    assert out[0, 0, 0] == 0 and out[0, H // 2, W // 2] == 1


def test_blur_definition():
    """no outside anchor: weights sum to one, a constant image is unchanged, sigma -> 0 is the identity, reflect padding does not
    repeat the edge pixel, and the separable passes equal the outer-product kernel"""
    rng = np.random.default_rng(9)
    x = rng.uniform(0, 1, size=(3, 6, 7))
    assert np.abs(R.blur(np.full((1, 5, 5), 0.3), 1.3) - 0.3).max() < 1e-15
    assert np.abs(R.blur(x, 0.1) - x).max() < 1e-20 + 1e-15
    sigma = 0.8
    e = np.exp(-1 / (2 * sigma * sigma))
    k1 = np.array([e, 1, e]) / (1 + 2 * e)
    p = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    assert np.array_equal(p[0, 0, 1:-1], x[0, 1]) and np.array_equal(p[0, 1:-1, 0], x[0, :, 1])
    want = sum(k1[a] * k1[b] * p[:, a:a + 6, b:b + 7] for a in range(3) for b in range(3))
    assert np.abs(R.blur(x, sigma) - want).max() < 1e-14


def test_chain_identity_and_erase():
    mean, inv_std = np.array([0.5071, 0.4867, 0.4408], np.float32), (1 / np.array([0.2675, 0.2565, 0.2761])).astype(np.float32)
    imgs = images(6, 4)
    p = R.identity_params(4)
    out, left = R.apply(imgs, None, p, mean, inv_std)
    want = (np.transpose(imgs, (0, 3, 1, 2)) / 255.0 - mean.astype(np.float64)[None, :, None, None]) * inv_std.astype(np.float64)[None, :, None, None]
    assert np.array_equal(out, want) and not left.any()
    p[:, R.ERASE_I], p[:, R.ERASE_J], p[:, R.ERASE_H], p[:, R.ERASE_W] = 3, 5, 7, 9
    p[1, R.FLIP] = 1
    out2, _ = R.apply(imgs, np.array([3, 2, 1, 0]), p, mean, inv_std)
    assert (out2[:, :, 3:10, 5:14] == 0).all() and np.array_equal(out2[0, :, 10:], want[3, :, 10:])
    assert np.array_equal(out2[1, :, :3], want[2, :, :3, ::-1])
    o32, _ = R.apply(imgs, None, p, mean, inv_std, np.float32)
    assert o32.dtype == np.float32
