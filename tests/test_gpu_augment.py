"""GPU checks of the training augmentation (csrc/spv_augment.hip, spectre_vit.augment): spv_augment_u8 with explicit parameter tables
against the float64 restatement tests/augment_ref.py, spv_augment_params' draws against their distributions, and harness.train with
augment=True.

Tolerance of the kernel tests: not a constant.  Every comparison evaluates the restatement a second time in numpy float32 on the same
inputs and allows the kernel 4 x the largest |float32 - float64| difference that run shows (the margin covers FMA contraction, another
reduction order for the contrast mean and the hardware's division / exp).  Pixels left out: rotation ties (source coordinate within 1e-3
of an integer; at most 1 %) and, when a blur follows the rotation, their 3 x 3 neighbourhood (at most 5 %).  Nothing else: a test
without rotation compares every pixel.  Every comparison prints its figures before it asserts (pytest -s); DESIGN.md section 4c
records a run: the kernel stayed between 0.2 and 0.3 of what was allowed in every case (full chain at batch 512, 3 x 32 x 32:
4.9e-6 against 2.0e-5 allowed)."""

import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(3, 32, 32), (1, 28, 28)]
MEAN = (0.5071, 0.4867, 0.4408)
STD = (0.2675, 0.2565, 0.2761)


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def count():
    from spectre_vit import _native
    return _native.call("spv_path_count", _native.PATH["augment"])


def make_aug(C, **kw):
    from spectre_vit.augment import TrainAugment
    return TrainAugment(MEAN[:C], STD[:C], **kw)


def image_set(n, shape, seed):
    C, H, W = shape
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, size=(n, H, W, C), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(0, n, 2):   # every other image smooth: low-saturation pixels, flat areas, black and white patches
        base = rng.uniform(0, 220, size=C) + rng.uniform(-3, 3, size=C) * xx[..., None] + rng.uniform(-3, 3) * yy[..., None]
        imgs[k] = np.clip(base + rng.uniform(0, 20) * rng.standard_normal((H, W, C)), 0, 255).astype(np.uint8)
    return imgs


def random_table(batch, shape, rng, ops):
    """identity table with the named ops switched on at random values inside the reference recipe's ranges"""
    C, H, W = shape
    p = R.identity_params(batch)
    u = lambda lo, hi: rng.uniform(lo, hi, size=batch).astype(np.float32)
    if "flip" in ops:
        p[:, R.FLIP] = rng.integers(0, 2, size=batch)
    if "brightness" in ops:
        p[:, R.BRIGHT] = u(0.6, 1.4)
    if "contrast" in ops:
        p[:, R.CONTRAST] = u(0.6, 1.4)
    if "saturation" in ops:
        p[:, R.SAT] = u(0.6, 1.4)
    if "hue" in ops:
        p[:, R.HUE] = u(-0.1, 0.1)
    if "order" in ops:
        p[:, R.ORDER] = (np.arange(batch) + rng.integers(0, 24)) % 24
    if "gray" in ops:
        p[:, R.GRAY] = rng.integers(0, 2, size=batch)
    if "rotate" in ops:
        p[:, R.ANGLE] = u(-30, 30)
    if "blur" in ops:
        p[:, R.BLUR] = 1
        p[:, R.SIGMA] = u(0.1, 2.0)
    if "erase" in ops:
        h, w = rng.integers(1, H, size=batch), rng.integers(1, W, size=batch)
        p[:, R.ERASE_H], p[:, R.ERASE_W] = h, w
        p[:, R.ERASE_I], p[:, R.ERASE_J] = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
    return p


ALL_OPS_ALONE = ["flip", "brightness", "contrast", "saturation", "hue", "gray", "rotate", "blur", "erase"]
ALL_OPS = ("flip", "brightness", "contrast", "saturation", "hue", "order", "gray", "rotate", "blur", "erase")


def run_and_compare(imgs, index, params, shape, what):
    """launch spv_augment_u8 once and hold its output to the float64 restatement under the float32-run tolerance.  Returns
    (out, ref64, left_out)."""
    C, H, W = shape
    aug = make_aug(C)
    d = dev()
    mean, inv_std = (t.cpu().numpy() for t in aug.norm(d))
    before = count()
    out = aug(torch.from_numpy(imgs).to(d), None if index is None else torch.from_numpy(index).to(d), params=torch.from_numpy(params).to(d))
    assert count() == before + 1, "the census slot counts one launch per call"
    out = out.cpu().numpy()
    ref64, left = R.apply(imgs, index, params, mean, inv_std, np.float64)
    ref32, _ = R.apply(imgs, index, params, mean, inv_std, np.float32)
    assert out.shape == ref64.shape == (params.shape[0], C, H, W) and out.dtype == np.float32
    rotated, blurred = (params[:, R.ANGLE] != 0).any(), (params[:, R.BLUR] != 0).any()
    share = left.mean()
    if not rotated:
        assert not left.any(), "only rotation ties may be left out"
    else:
        assert share <= (0.05 if blurred else 0.01), f"{what}: {100 * share:.2f} % of pixels left out"
    keep = np.broadcast_to(~left[:, None], out.shape)
    tol = 4.0 * float(np.abs(ref32.astype(np.float64) - ref64)[keep].max())
    err = float(np.abs(out.astype(np.float64) - ref64)[keep].max())
    print(f"{what}: max |kernel - f64| {err:.3e}, allowed 4 x max |f32 - f64| = {tol:.3e}, left out {100 * share:.3f} %")
    assert np.isfinite(out).all()
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return out, ref64, left


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identity_parameters_are_totensor_normalize(shape):
    C, H, W = shape
    imgs = image_set(16, shape, 1)
    out, ref, _ = run_and_compare(imgs, None, R.identity_params(16), shape, f"identity {shape}")
    mean, std = np.array(MEAN[:C], np.float64), np.array(STD[:C], np.float64)
    want = (np.transpose(imgs, (0, 3, 1, 2)) / 255.0 - mean[None, :, None, None]) / std[None, :, None, None]
    assert np.abs(ref - want).max() < 1e-6   # the float32 mean / inv_std the kernel is handed against the float64 statistics


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("op", ALL_OPS_ALONE)
def test_every_op_alone(shape, op):
    rng = np.random.default_rng(100 * ALL_OPS_ALONE.index(op) + shape[0])
    imgs = image_set(64, shape, 2)
    index = rng.integers(0, 64, size=48)
    params = random_table(48, shape, rng, (op,))
    if op in ("flip", "gray"):
        params[:2, R.FLIP if op == "flip" else R.GRAY] = (0, 1)
    out, ref, left = run_and_compare(imgs, index, params, shape, f"{op} {shape}")
    if op == "erase":
        for b in range(48):
            i, j, h, w = (int(params[b, k]) for k in (R.ERASE_I, R.ERASE_J, R.ERASE_H, R.ERASE_W))
            assert (out[b, :, i:i + h, j:j + w] == 0).all() and h * w > 0
    if op == "rotate":
        aug = make_aug(shape[0])
        mean, inv_std = (t.cpu().numpy() for t in aug.norm(dev()))
        fill = (np.float32(0) - mean) * inv_std    # as fp32 computes it
        H, W = shape[1:]
        seen = 0
        for b in range(48):
            sx, sy = R.rotation_source(float(params[b, R.ANGLE]), H, W)
            outside = ((np.floor(sx) < 0) | (np.floor(sx) >= W) | (np.floor(sy) < 0) | (np.floor(sy) >= H)) & ~left[b]
            seen += int(outside.sum())
            assert (out[b][:, outside] == fill[:, None]).all(), b
        assert seen > 100


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_jitter_order(shape):
    """each of the 24 orders, three images each, all four factors drawn; the orders must differ from one another on the same image"""
    rng = np.random.default_rng(24)
    imgs = image_set(8, shape, 3)
    params = random_table(72, shape, rng, ("brightness", "contrast", "saturation", "hue"))
    params[:, R.ORDER] = np.arange(72) % 24
    index = np.repeat(np.arange(3), 24)
    for k in range(3):   # the same factors for the 24 orders of one image
        params[24 * k:24 * k + 24, R.BRIGHT:R.HUE + 1] = params[24 * k, R.BRIGHT:R.HUE + 1]
    out, ref, _ = run_and_compare(imgs, index, params, shape, f"24 orders {shape}")
    if shape[0] == 3:
        for k in range(3):
            distinct = {out[24 * k + o].tobytes() for o in range(24)}
            assert len(distinct) == 24, len(distinct)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("batch", [1, 7, 512])
@pytest.mark.parametrize("with_index", [False, True], ids=["rows", "index"])
def test_full_chain(shape, batch, with_index):
    rng = np.random.default_rng(batch + shape[0] + with_index)
    n = 600
    imgs = image_set(n, shape, 4)
    index = rng.integers(0, n, size=batch) if with_index else None
    params = random_table(batch, shape, rng, ALL_OPS)
    params[:, R.BLUR] = rng.integers(0, 2, size=batch)
    half = rng.integers(0, 2, size=batch).astype(bool)
    params[half, R.ERASE_H] = 0   # no rectangle
    out, ref, left = run_and_compare(imgs, index, params, shape, f"chain {shape} batch {batch} {'index' if with_index else 'rows'}")
    for b in range(batch):
        i, j, h, w = (int(params[b, k]) for k in (R.ERASE_I, R.ERASE_J, R.ERASE_H, R.ERASE_W))
        if h > 0:
            assert (out[b, :, i:i + h, j:j + w] == 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_drawn_tables_through_the_chain(shape):
    """the table spv_augment_params draws, applied by __call__(step=...) and by params=: the same batch, equal to the restatement"""
    C, H, W = shape
    aug = make_aug(C, seed=7)
    d = dev()
    imgs = image_set(300, shape, 5)
    x = torch.from_numpy(imgs).to(d)
    index = torch.from_numpy(np.random.default_rng(0).permutation(300)[:256]).to(d)
    table = aug.draw(256, 11, height=H, width=W)
    a = aug(x, index, step=11)
    b = aug(x, index, params=table)
    assert torch.equal(a, b)
    out, _, _ = run_and_compare(imgs, index.cpu().numpy(), table.cpu().numpy(), shape, f"drawn table {shape}")
    assert np.array_equal(out, a.cpu().numpy())


def test_index_outside_the_set_poisons_its_image_only():
    """the host cannot see a device index; the kernel reads nothing for a row outside [0, n_src) and writes NaN to its image"""
    shape = (3, 32, 32)
    imgs = image_set(8, shape, 6)
    aug = make_aug(3)
    d = dev()
    index = torch.tensor([0, -1, 3, 8, 7], dtype=torch.int64, device=d)
    out = aug(torch.from_numpy(imgs).to(d), index, params=torch.from_numpy(R.identity_params(5)).to(d)).cpu().numpy()
    assert np.isnan(out[1]).all() and np.isnan(out[3]).all() and np.isfinite(out[[0, 2, 4]]).all()


# ---------------------------------------------------------------- spv_augment_params
N = 65536


def five_sigma_rate(hits, p, n, what):
    sigma = np.sqrt(p * (1 - p) / n)
    assert abs(hits / n - p) <= 5 * sigma, f"{what}: rate {hits / n:.4f}, p {p}, 5 sigma {5 * sigma:.4f}"


def five_sigma_mean(x, lo, hi, what):
    assert x.min() >= lo - 1e-6 and x.max() <= hi + 1e-6, f"{what}: [{x.min()}, {x.max()}] outside [{lo}, {hi}]"
    sigma = (hi - lo) / np.sqrt(12 * x.size)
    assert abs(x.mean(dtype=np.float64) - 0.5 * (lo + hi)) <= 5 * sigma, f"{what}: mean {x.mean():.5f}, 5 sigma {5 * sigma:.5f}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_params_distributions(shape):
    C, H, W = shape
    aug = make_aug(C, seed=42)
    t = aug.draw(N, 3, height=H, width=W)
    p = t.cpu().numpy()
    assert p.shape == (N, 16) and (p[:, 14:] == 0).all()
    assert torch.equal(t, aug.draw(N, 3, height=H, width=W)), "same (seed, step): the same table"
    other_step, other_seed = aug.draw(N, 4, height=H, width=W).cpu().numpy(), make_aug(C, seed=43).draw(N, 3, height=H, width=W).cpu().numpy()
    high_word = make_aug(C, seed=42 + (1 << 32)).draw(N, 3, height=H, width=W).cpu().numpy()
    for q, what in ((other_step, "step"), (other_seed, "seed"), (high_word, "seed high word")):
        assert (q[:, R.BRIGHT] != p[:, R.BRIGHT]).mean() > 0.99 and (q[:, R.ANGLE] != p[:, R.ANGLE]).mean() > 0.99, what
    for col in (R.FLIP, R.GRAY, R.BLUR):
        assert set(np.unique(p[:, col])) <= {0.0, 1.0}
    five_sigma_rate((p[:, R.FLIP] == 1).sum(), 0.5, N, "flip")
    five_sigma_rate((p[:, R.GRAY] == 1).sum(), 0.2, N, "grayscale")
    five_sigma_rate((p[:, R.BLUR] == 1).sum(), 0.5, N, "blur")
    for col, what in ((R.BRIGHT, "brightness"), (R.CONTRAST, "contrast"), (R.SAT, "saturation")):
        five_sigma_mean(p[:, col], 0.6, 1.4, what)
    five_sigma_mean(p[:, R.HUE], -0.1, 0.1, "hue")
    five_sigma_mean(p[:, R.ANGLE], -30.0, 30.0, "angle")
    five_sigma_mean(p[:, R.SIGMA], 0.1, 2.0, "sigma")
    order = p[:, R.ORDER]
    assert (order == np.floor(order)).all() and order.min() == 0 and order.max() == 23
    counts = np.bincount(order.astype(int), minlength=24)
    sigma = np.sqrt(N * (1 / 24) * (23 / 24))
    assert (np.abs(counts - N / 24) <= 5 * sigma).all(), counts
    # the draws are independent of one another: flip against grayscale, flip against the sign of the angle
    both = ((p[:, R.FLIP] == 1) & (p[:, R.GRAY] == 1)).sum()
    five_sigma_rate(both, 0.1, N, "flip and grayscale")
    five_sigma_rate(((p[:, R.FLIP] == 1) & (p[:, R.ANGLE] > 0)).sum(), 0.25, N, "flip and angle > 0")
    # erasing: the rectangle lies inside the image; area and aspect inside the configured ranges up to the rounding of h and w
    i, j, h, w = (p[:, k] for k in (R.ERASE_I, R.ERASE_J, R.ERASE_H, R.ERASE_W))
    for v in (i, j, h, w):
        assert (v == np.floor(v)).all() and (v >= 0).all()
    on = h > 0
    assert ((w > 0) == on).all() and (i[~on] == 0).all() and (j[~on] == 0).all()
    # the search of ten attempts all but never fails at these sizes, so the rate of rectangles is the rate of the Bernoulli draw
    five_sigma_rate(on.sum(), 0.5, N, "erase")
    i, j, h, w = i[on], j[on], h[on], w[on]
    assert (h < H).all() and (w < W).all() and (i + h <= H).all() and (j + w <= W).all()
    area = H * W
    assert ((h - 0.5) * (w - 0.5) <= 0.33 * area * (1 + 1e-5)).all() and ((h + 0.5) * (w + 0.5) >= 0.02 * area * (1 - 1e-5)).all()
    assert ((h - 0.5) / (w + 0.5) <= 3.3 * (1 + 1e-5)).all() and ((h + 0.5) / (w - 0.5) >= 0.3 * (1 - 1e-5)).all()
    # positions are uniform on what keeps the rectangle inside: i / (H - h) has mean 1/2 and a standard deviation of at most 1/2, so
    # the mean over n rectangles lies within 5 * 0.5 / sqrt(n) of 1/2
    frac_i, frac_j = i / (H - h), j / (W - w)
    for frac in (frac_i, frac_j):
        assert abs(frac.mean() - 0.5) <= 2.5 / np.sqrt(frac.size), frac.mean()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_params_all_off_is_the_identity_table(shape):
    C, H, W = shape
    aug = make_aug(C, flip=0, jitter=(0, 0, 0, 0), grayscale=0, degrees=0, blur=0, blur_sigma=(1.0, 1.0), erase=0, seed=5)
    p = aug.draw(N, 9, height=H, width=W).cpu().numpy()
    want = R.identity_params(N)
    order = p[:, R.ORDER].copy()
    p[:, R.ORDER] = 0    # the order of four identities is still drawn, and does not matter
    assert np.array_equal(p, want) and order.min() >= 0 and order.max() <= 23
    imgs = image_set(32, shape, 8)
    q = aug.draw(32, 9, height=H, width=W)
    out = aug(torch.from_numpy(imgs).to(dev()), params=q).cpu().numpy()
    base = aug(torch.from_numpy(imgs).to(dev()), params=torch.from_numpy(R.identity_params(32)).to(dev())).cpu().numpy()
    assert np.array_equal(out, base)


# ---------------------------------------------------------------- harness
def _run(tmp_path, tag, records, **kw):
    from spectre_vit.harness import train

    def hook(kind, step, img, label):
        records.setdefault(kind, []).append((step, img.detach().float().cpu().clone(), label.detach().cpu().clone()))
    _, hist = train(out_dir=str(tmp_path / tag), log=lambda r: None, batch_hook=hook, epochs=2, steps_per_epoch=8, **kw)
    return hist


@pytest.mark.parametrize("case", ["fft-eager", "fft-graph", "spectre_branch"])
def test_harness_trains_on_augmented_batches(tmp_path, case):
    from spectre_vit import harness
    if case == "spectre_branch":
        kw = dict(config_path="spectre_vit/configs/spectre_branch.py", model="spectre_branch", batch_size=512, n_train=4096, n_val=512)
    else:
        kw = dict(config_path="spectre_vit/configs/spectre_vit_cifar100.py", mixer="fft", batch_size=64, n_train=1024, n_val=256,
                  graph=case == "fft-graph")
    before = count()
    on1, on2, off = {}, {}, {}
    h1 = _run(tmp_path, "a", on1, augment=True, **kw)
    assert count() == before + 16, "one apply launch per training step"
    h2 = _run(tmp_path, "b", on2, augment=True, **kw)
    h0 = _run(tmp_path, "c", off, **kw)
    assert count() == before + 32
    for hist in (h1, h2, h0):
        assert len(hist) == 2 and all(r["steps"] == 8 for r in hist)
        for r in hist:
            assert all(np.isfinite(r[k]) for k in ("Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation")), r
    assert len(on1["train"]) == len(on2["train"]) == len(off["train"]) == 16
    assert [s for s, _, _ in on1["train"]] == list(range(16)), "the augmentation's step is the global step"
    for (_, a, la), (_, b, lb), (_, c, lc) in zip(on1["train"], on2["train"], off["train"]):
        assert a.dtype == torch.float32 and a.shape == c.shape
        assert torch.equal(a, b) and torch.equal(la, lb), "same seed: bit-equal augmented batches"
        assert torch.equal(la, lc) and not torch.equal(a, c), "the same rows in the same order, transformed"
        assert torch.isfinite(a).all()
    assert len(on1["val"]) == len(off["val"]) > 0
    for (_, a, la), (_, c, lc) in zip(on1["val"], off["val"]):
        assert torch.equal(a, c) and torch.equal(la, lc), "validation batches are untouched"


def test_ranks_draw_different_augmentations():
    from spectre_vit import harness
    shape = (3, 32, 32)
    d = dev()
    x = torch.from_numpy(image_set(64, shape, 9)).to(d)
    idx = torch.arange(64, device=d)
    r0 = make_aug(3, seed=harness.augment_seed(42, 0))
    r1 = make_aug(3, seed=harness.augment_seed(42, 1))
    a, b = r0(x, idx, step=5), r1(x, idx, step=5)
    assert torch.equal(a, make_aug(3, seed=harness.augment_seed(42, 0))(x, idx, step=5))
    differ = sum(not torch.equal(a[k], b[k]) for k in range(64))
    assert differ == 64, differ
    assert not torch.equal(r0.draw(64, 5), r0.draw(64, 6))
