"""CPU checks of the paired-view distillation (spectre_vit.distillation.TeacherView / DistillationLoss, harness.train_distill,
csrc/spv_distill.hip): the numpy restatement tests/distill_ref.py -- the reference of the GPU tests -- against Pillow itself on every
pixel (equality: both are integer arithmetic), the product's coefficient table against the restatement's, the C-ABI's refusals, and
the public surface.  Everything here fails on the parent commit (nothing to import)."""
import inspect
import os

import numpy as np
import pytest

import distill_ref as D

RESIZE, CROP = 256, 224


def pillow_view(img):
    from PIL import Image
    lo = (RESIZE - CROP) // 2
    pil = Image.fromarray(img if img.shape[-1] == 3 else img[..., 0])
    out = np.asarray(pil.resize((RESIZE, RESIZE), Image.BICUBIC))[lo:lo + CROP, lo:lo + CROP]
    return out if out.ndim == 3 else out[..., None]


def two_level_images():
    """0 / 255 images, where the bicubic ringing leaves 0..255 and the clamp acts: checkerboards, stripes, a disc, random bits"""
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:32, 0:32]
    planes = [(yy + xx) % 2, (xx // 2) % 2, (yy // 3) % 2, ((yy - 15.5) ** 2 + (xx - 15.5) ** 2 < 90), rng.integers(0, 2, (32, 32)),
              ((yy // 4 + xx // 4) % 2)]
    imgs = np.stack([np.stack([p, 1 - p if k % 2 else p, np.roll(p, k, axis=1)], axis=-1) for k, p in enumerate(planes)])
    return (imgs.astype(np.uint8) * 255)


FAMILIES = {
    "random 32x32x3": lambda: np.random.default_rng(1).integers(0, 256, size=(60, 32, 32, 3), dtype=np.uint8),
    "random 28x28x1": lambda: np.random.default_rng(2).integers(0, 256, size=(60, 28, 28, 1), dtype=np.uint8),
    "two-level 32x32x3": two_level_images,
}
PIXELS = {"random 32x32x3": 9_031_680, "random 28x28x1": 3_010_560, "two-level 32x32x3": 903_168}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_restatement_equals_pillow_on_every_pixel(family):
    imgs = FAMILIES[family]()
    got, (acc_lo, acc_hi) = D.teacher_view_u8(imgs, RESIZE, CROP, return_range=True)
    want = np.stack([pillow_view(im) for im in imgs])
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    differing = int((got != want).sum())
    print(f"{family}: {differing} of {got.size} values differ from Pillow; accumulator range [{acc_lo}, {acc_hi}]")
    assert got.size >= PIXELS[family]
    assert differing == 0
    assert -2 ** 31 <= acc_lo and acc_hi < 2 ** 31, "the kernel's accumulator is int32"
    if family.startswith("two-level"):
        assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()


@pytest.mark.parametrize("n", [28, 32, 64, 256])
def test_product_table_equals_the_restatement(n):
    from spectre_vit.distillation import teacher_view_table
    xmin, taps = teacher_view_table(n, RESIZE, CROP)
    rx, rt, count = D.table(n, RESIZE, CROP)
    assert xmin.dtype == taps.dtype == np.int32 and xmin.shape == (CROP,) and taps.shape == (CROP, 4)
    assert (count == 4).all(), "every cropped output has exactly four taps"
    assert np.array_equal(xmin, rx) and np.array_equal(taps, rt)
    assert (taps.astype(np.int64).sum(axis=1) == 1 << 22).all(), "every row's integer taps sum to 2^22"
    assert xmin.min() >= 0 and xmin.max() + 4 <= n
    distinct = len({tuple(r) for r in taps.tolist()})
    print(f"n={n}: {distinct} distinct tap rows")
    if n == 32:
        assert distinct == 8, "the eight phases of an 8:1 up-scaling"
    if n == 256:
        assert distinct == 1 and taps[0].tolist() == [0, 1 << 22, 0, 0], "resize == n is the identity"


def test_table_refuses_what_the_kernel_does_not_take():
    from spectre_vit.distillation import teacher_view_table
    for bad in (dict(n=300), dict(n=1), dict(n=32, crop=300), dict(n=32, crop=0), dict(n=32, crop=256)):   # crop 256: edge windows are clipped
        kw = dict(n=32, resize=RESIZE, crop=CROP)
        kw.update(bad)
        with pytest.raises(ValueError, match="teacher view"):
            teacher_view_table(**kw)


def test_normalize_lut_is_torch_totensor_normalize():
    import torch
    from spectre_vit.distillation import normalize_lut
    from spectre_vit.harness import CIFAR_MEAN, CIFAR_STD
    for C in (1, 3):
        lut = normalize_lut(CIFAR_MEAN[:C], CIFAR_STD[:C])
        assert lut.shape == (C, 256) and lut.dtype == torch.float32
        img = np.random.default_rng(C).integers(0, 256, size=(5, 9, 11, C), dtype=np.uint8)
        want = D.normalise(img, CIFAR_MEAN[:C], CIFAR_STD[:C])
        got = torch.stack([lut[c][torch.from_numpy(img[..., c].astype(np.int64))] for c in range(C)], dim=1)
        assert torch.equal(got, want)


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
    assert int(enum["SPV_PATH_TEACHER_VIEW"]) == _native.PATH["teacher_view"] == 23 < int(enum["SPV_PATH_COUNT"]) == 27
    assert sorted(_native.PATH.values()) == list(range(27))
    sup = lambda c, n, r, k: _native.call("spv_teacher_view_supported", c, n, r, k)
    assert sup(3, 32, 256, 224) == 1 and sup(1, 28, 256, 224) == 1 and sup(3, 28, 256, 224) == 1 and sup(3, 256, 256, 224) == 1
    assert sup(2, 32, 256, 224) == 0, "2 channels"
    assert sup(3, 300, 256, 224) == 0, "n > resize"
    assert sup(3, 32, 256, 300) == 0, "crop > resize"
    assert sup(3, 1, 256, 224) == 0 and sup(3, 0, 256, 224) == 0, "n < 2"
    assert sup(3, 32, 256, 0) == 0 and sup(3, 32, 256, 256) == 0, "no crop / clipped edge windows"
    assert sup(3, 2048, 2048, 2048 - 64) == 0, "staging beyond the LDS bound"
    assert _native.call("spv_augment_supported", 3, 224, 224) == 0
    assert _native.call("spv_distill_loss_workspace_floats") >= 3


def test_distill_entry_points_reject_bad_arguments_before_any_launch(built):
    """Every call fails validation on the host: nothing is launched (no GPU here).  An index outside the set is not among them: it lives
    on the device (the kernel writes NaN to such an image)."""
    from spectre_vit import _native
    tv, fw, bw = "spv_teacher_view_u8", "spv_distill_loss_fwd", "spv_distill_loss_bwd"
    cases = [
        (tv, (16, 0, 16, 16, 16, 4, 8, 2, 32, 256, 224, 0, 0), "not supported"),
        (tv, (16, 0, 16, 16, 16, 4, 8, 3, 300, 256, 224, 0, 0), "not supported"),
        (tv, (16, 0, 16, 16, 16, 4, 8, 3, 32, 256, 300, 0, 0), "not supported"),
        (tv, (16, 0, 16, 16, 16, 4, 8, 3, 1, 256, 224, 0, 0), "not supported"),
        (tv, (16, 0, 16, 16, 16, 4, 8, 3, 32, 256, 224, 2, 0), "dtype"),
        (tv, (0, 0, 16, 16, 16, 4, 8, 3, 32, 256, 224, 0, 0), "src"),
        (tv, (16, 0, 16, 16, 0, 4, 8, 3, 32, 256, 224, 1, 0), "out"),
        (tv, (16, 0, 0, 16, 16, 4, 8, 3, 32, 256, 224, 0, 0), "table"),
        (tv, (16, 0, 16, 0, 16, 4, 8, 3, 32, 256, 224, 0, 0), "lut"),
        (tv, (16, 0, 16, 16, 16, 0, 8, 3, 32, 256, 224, 0, 0), "bad shape"),
        (tv, (16, 0, 16, 16, 16, 9, 8, 3, 32, 256, 224, 0, 0), "n_src"),
        (fw, (0, 16, 16, 16, 16, 16, 4, 10, 2.0, 0.25, 0.75, 0), "student"),
        (fw, (16, 0, 16, 16, 16, 16, 4, 10, 2.0, 0.25, 0.75, 0), "teacher"),
        (fw, (16, 16, 0, 16, 16, 16, 4, 10, 2.0, 0.25, 0.75, 0), "labels"),
        (fw, (16, 16, 16, 16, 16, 0, 4, 10, 2.0, 0.25, 0.75, 0), "workspace"),
        (fw, (16, 16, 16, 16, 16, 16, 0, 10, 2.0, 0.25, 0.75, 0), "empty"),
        (fw, (16, 16, 16, 16, 16, 16, 4, 0, 2.0, 0.25, 0.75, 0), "empty"),
        (fw, (16, 16, 16, 16, 16, 16, 4, 10, 0.0, 0.25, 0.75, 0), "temperature"),
        (fw, (16, 16, 16, 16, 16, 16, 4, 10, float("nan"), 0.25, 0.75, 0), "temperature"),
        (fw, (16, 16, 16, 16, 16, 16, 4, 10, 2.0, float("inf"), 0.75, 0), "weight"),
        (bw, (0, 16, 16, 16, 16, 16, 4, 10, 2.0, 0.25, 0.75, 0), "student"),
        (bw, (16, 16, 16, 16, 16, 0, 4, 10, 2.0, 0.25, 0.75, 0), "output"),
        (bw, (16, 16, 16, 16, 16, 16, -1, 10, 2.0, 0.25, 0.75, 0), "empty"),
        (bw, (16, 16, 16, 16, 16, 16, 4, 10, -1.0, 0.25, 0.75, 0), "temperature"),
    ]
    for name, args, needle in cases:
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, needle, str(e.value))


def test_public_surface_and_refusals_before_a_device_is_touched(built, monkeypatch, tmp_path):
    import torch
    from spectre_vit import harness, hip_ops
    from spectre_vit.distillation import DistillationLoss, TeacherView
    from spectre_vit.graph import GraphedDistillStep, GraphedTrainStep
    want = dict(mixer="permut", epochs=1, steps_per_epoch=None, batch_size=None, n_train=4096, n_val=1024, use_amp=False, graph=False,
                augment=True, teacher=None, T=2.0, soft_target_loss_weight=0.25, ce_loss_weight=0.75, resize=256, crop=224, log=print,
                batch_hook=None)
    sig = inspect.signature(harness.train_distill)
    assert list(sig.parameters)[0] == "config_path" and "out_dir" in sig.parameters
    for k, v in want.items():
        assert sig.parameters[k].default == v, k
    lsig = inspect.signature(hip_ops.distill_loss)
    assert [lsig.parameters[k].default for k in ("T", "w_soft", "w_ce")] == [2.0, 0.25, 0.75]
    crit = DistillationLoss()
    assert (crit.T, crit.soft_target_loss_weight, crit.ce_loss_weight) == (2.0, 0.25, 0.75) and crit.soft is None and crit.ce is None
    with pytest.raises(ValueError):
        DistillationLoss(T=0.0)
    v = TeacherView(harness.CIFAR_MEAN, harness.CIFAR_STD)
    assert (v.resize, v.crop, v.dtype) == (256, 224, torch.float32)
    with pytest.raises(ValueError):
        TeacherView((0.5, 0.5), (0.5, 0.5))
    with pytest.raises(TypeError):
        TeacherView((0.5,), (0.5,), dtype=torch.float16)
    with pytest.raises(TypeError):
        v(torch.zeros(4, 32, 32, 3))                      # not uint8
    with pytest.raises(RuntimeError, match="GPU"):
        v(torch.zeros(4, 32, 32, 3, dtype=torch.uint8))   # no CPU fallback
    with pytest.raises(RuntimeError, match="GPU"):
        hip_ops.distill_loss(torch.zeros(4, 10), torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64))
    assert issubclass(GraphedDistillStep, GraphedTrainStep)

    cfg = "spectre_vit/configs/spectre_vit_mnist.py"
    out = str(tmp_path / "x")
    for kw in (dict(resize=16), dict(crop=300), dict(crop=256), dict(crop=0)):
        with pytest.raises(ValueError, match="teacher view"):
            harness.train_distill(cfg, out_dir=out, **kw)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="graph=True"):
        harness.train_distill(cfg, out_dir=out, graph=True)
    monkeypatch.delenv("WORLD_SIZE")
    assert not os.path.exists(out), "a refused run leaves nothing behind"
    # the old loop keeps its refusals
    with pytest.raises(ValueError, match="augment"):
        harness.train(cfg, augment=True, distill=True)
