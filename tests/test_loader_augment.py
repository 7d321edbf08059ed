"""Fetch and augment in one launch, the host side (no GPU): the ABI of spv_loader_fetch_augment, the truth table of
spv_loader_augment_supported, every refusal of the C entry point -- the fetch's, the draw's and the kernel's own -- with dummy pointers,
and every refusal of ResidentLoader(output="augment") with the library's launches replaced by an assertion."""
import ctypes
import os

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_abi(built):
    from conftest import ROOT
    from spectre_vit import _native, timing
    lib = _native.load()
    src = open(os.path.join(ROOT, "include", "spv.h")).read()
    assert hasattr(lib, "spv_loader_fetch_augment") and "int spv_loader_fetch_augment(" in src
    assert hasattr(lib, "spv_loader_augment_supported") and "int spv_loader_augment_supported(" in src
    # 10 pointers (src, labels_src, cursor, index, labels, params, out, mean, inv_std, cfg), 8 geometry ints, the loader's seed, shuffle,
    # label dtype, the augmentation's seed, the stream: no by-value step
    sig = _native.SIGNATURES["spv_loader_fetch_augment"]
    assert len(sig) == 23 and sig.count(ctypes.c_uint64) == 2 and sig[-1] is ctypes.c_void_p
    assert len(_native.SIGNATURES["spv_loader_augment_supported"]) == 3 and "spv_loader_augment_supported" in _native._NO_STATUS
    # no new census slot, no version change
    assert "SPV_PATH_COUNT = 27" in src and len(_native.PATH) == 27 and lib.spv_version() == 1
    # the work model: (n, batch, chans, height, width, world, rank, steps, shuffle, label dtype, null mask, hint)
    assert "spv_loader_fetch_augment" in timing._WORK_MODELS, "bench.py's roofline pass brackets every launch it sees"
    model = timing._WORK_MODELS["spv_loader_fetch_augment"]
    base = (50000, 512, 3, 32, 32, 1, 0, 97, 1)
    assert model(base + (0, 0, 0))[3:] == ("hbm", 512 * (17.0 + 64.0 + 3072 * 5))
    assert model(base + (1, 0, 0))[4] == 512 * (24.0 + 64.0 + 3072 * 5)


def test_support_truth_table(built):
    from spectre_vit import _native
    fused = lambda c, h, w: _native.call("spv_loader_augment_supported", c, h, w)
    apply_only = lambda c, h, w: _native.call("spv_augment_supported", c, h, w)
    assert fused(3, 32, 32) == 1 and fused(1, 28, 28) == 1 and fused(3, 5, 7) == 1
    # the LDS border: two fp32 copies of 1 x 89 x 92 and the eight reduction slots are (2 * 8188 + 8) * 4 = 65536 bytes, all of
    # spv_augment_u8's 64 KiB -- nothing is left for the fused kernel's step, row and table row
    assert fused(1, 89, 92) == 0 and apply_only(1, 89, 92) == 1
    assert fused(1, 89, 91) == 1   # one column fewer: 364 bytes free, 80 needed
    assert fused(3, 64, 64) == 0 and fused(3, 224, 224) == 0
    assert fused(2, 32, 32) == 0
    assert fused(3, 1, 32) == 0 and fused(3, 32, 1) == 0 and fused(1, 1, 1) == 0 and fused(3, 0, 0) == 0
    assert fused(1, 2, 4000) == 0 and apply_only(1, 2, 4000) == 1   # the loader's sides end at 512


def test_c_abi_rejects_bad_arguments_before_any_launch(built):
    """every call fails validation on the host (non-zero return, spv_last_error text, RuntimeError from the ctypes wrapper), so nothing
    is launched and no GPU is needed: the fetch's refusals, the draw's, and the fused kernel's own"""
    from spectre_vit import _native
    from spectre_vit.augment import TrainAugment
    P = 16   # any non-null, 16-byte aligned "pointer": validation fails before it would be used
    good = TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2)).cfg()

    def cfg_with(**kw):
        c = TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2)).cfg()
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    keep = []   # the structs stay alive while their addresses are in the case list

    def args(src=P, labels_src=P, cursor=P, index=P, labels=P, params=P, out=P, mean=P, inv_std=P, cfg=good, n=100, batch=10, chans=3,
             height=32, width=32, world=1, rank=0, steps=10, seed=42, shuffle=1, label_dtype=0, aug_seed=7):
        keep.append(cfg)
        return (src, labels_src, cursor, index, labels, params, out, mean, inv_std, ctypes.addressof(cfg) if cfg is not None else 0, n,
                batch, chans, height, width, world, rank, steps, seed, shuffle, label_dtype, aug_seed, 0)

    cases = [
        # spv_loader_fetch's
        (args(labels_src=0), "null labels_src"), (args(cursor=0), "null labels_src"), (args(index=0), "null labels_src"),
        (args(labels=0), "null labels_src"),
        (args(src=0), "null src_nhwc"), (args(out=0), "null src_nhwc"),
        (args(cursor=12), "8-byte aligned"),
        (args(mean=0), "mean and inv_std"), (args(inv_std=0), "mean and inv_std"),
        (args(n=0), "n = 0"),
        (args(batch=0), "batch"), (args(batch=-3), "batch"),
        (args(world=0), "world"), (args(world=-1), "world"), (args(rank=-1), "rank"), (args(rank=1), "rank"),
        (args(world=2, rank=2, steps=5), "rank"),
        (args(steps=0), "steps_per_epoch"), (args(steps=-1), "steps_per_epoch"), (args(steps=11), "steps_per_epoch"),
        (args(world=2, rank=1, steps=6), "steps_per_epoch"),
        (args(n=2 ** 31 - 1, batch=2 ** 16, world=2 ** 8, steps=2 ** 8), "steps_per_epoch"),
        (args(chans=2), "chans"), (args(chans=0), "chans"), (args(chans=4), "chans"),
        (args(height=0), "height"), (args(height=513), "height"), (args(width=0), "width"), (args(width=513), "width"),
        (args(label_dtype=2), "unknown label dtype"), (args(label_dtype=-1), "unknown label dtype"),
        # spv_augment_params's
        (args(params=0), "params / cfg missing"), (args(cfg=None), "params / cfg missing"),
        (args(params=24), "16-byte aligned"),
        (args(height=1), "bad shape"), (args(width=1), "bad shape"),
        (args(cfg=cfg_with(blur_p=1.5)), "probability"), (args(cfg=cfg_with(flip_p=-0.1)), "probability"),
        (args(cfg=cfg_with(gray_p=2.0)), "probability"), (args(cfg=cfg_with(erase_p=1.01)), "probability"),
        (args(cfg=cfg_with(sigma_lo=0.0)), "range"), (args(cfg=cfg_with(bright_lo=2.0, bright_hi=1.0)), "range"),
        (args(cfg=cfg_with(hue_hi=0.6)), "range"), (args(cfg=cfg_with(degrees=181.0)), "range"),
        (args(cfg=cfg_with(scale_hi=1.5)), "range"), (args(cfg=cfg_with(ratio_lo=0.0)), "range"),
        # the fused kernel's own: the predicate (the message names the path that still serves the shape), the output's alignment
        (args(chans=1, height=89, width=92), "not supported"), (args(chans=1, height=89, width=92), "spv_augment_u8"),
        (args(height=64, width=64), "not supported"), (args(height=224, width=224), "spv_augment_tiled_u8"),
        (args(out=18), "4-byte aligned"),
    ]
    lib = _native.load()
    counted = _native.call("spv_path_count", _native.PATH["augment"])
    for a, needle in cases:
        assert lib.spv_loader_fetch_augment(*a) != 0, a
        assert needle in lib.spv_last_error().decode(), (needle, lib.spv_last_error().decode())
        with pytest.raises(RuntimeError) as e:
            _native.call("spv_loader_fetch_augment", *a)
        assert "spv_loader_fetch_augment" in str(e.value) and needle in str(e.value), (needle, str(e.value))
    assert _native.call("spv_path_count", _native.PATH["augment"]) == counted, "a refused call is not counted"


def test_python_refusals_touch_no_device(built, monkeypatch):
    """every refusal of ResidentLoader(output="augment") is raised on the host: the only library entry the constructor may reach is
    the host predicate (it computes a byte count and touches no device); any other call fails this test, and the tensors stay on the
    CPU"""
    from spectre_vit import _native
    from spectre_vit.augment import TrainAugment
    from spectre_vit.data import ResidentLoader
    real = _native.call

    def no_launch(name, *a):
        if name == "spv_loader_augment_supported":
            return real(name, *a)
        raise AssertionError(f"{name} called: a refusal must come before any device work")
    monkeypatch.setattr(_native, "call", no_launch)
    x = torch.zeros((64, 8, 8, 3), dtype=torch.uint8)
    y = torch.zeros(64, dtype=torch.uint8)
    aug3 = TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), seed=1)
    aug1 = TrainAugment((0.5,), (0.2,), seed=1)
    for output in ("float", "uint8", "none"):
        with pytest.raises(ValueError, match="goes with output='augment'"):
            ResidentLoader(x, y, 8, output=output, augment=aug3)
    with pytest.raises(ValueError, match="goes with output='augment'"):
        ResidentLoader(x, y, 8, augment=aug3)   # the default output
    with pytest.raises(ValueError, match="needs augment=TrainAugment"):
        ResidentLoader(x, y, 8, output="augment")
    with pytest.raises(ValueError, match="needs augment=TrainAugment"):
        ResidentLoader(x, y, 8, output="augment", augment=lambda *a, **k: None)
    with pytest.raises(ValueError, match="channels"):
        ResidentLoader(x, y, 8, output="augment", augment=aug1)
    with pytest.raises(ValueError, match="channels"):
        ResidentLoader(torch.zeros((64, 8, 8, 1), dtype=torch.uint8), y, 8, output="augment", augment=aug3)
    with pytest.raises(ValueError, match="kernel='tiled'"):
        ResidentLoader(x, y, 8, output="augment", augment=TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), kernel="tiled"))
    # shapes the predicate refuses: the message names the three-launch path that still serves them
    for shape, aug in (((4, 64, 64, 3), aug3), ((4, 89, 92, 1), aug1), ((4, 1, 8, 3), aug3), ((4, 224, 224, 3), aug3)):
        with pytest.raises(ValueError, match=r"output='none'.*spv_augment_params") as e:
            ResidentLoader(torch.zeros(shape, dtype=torch.uint8), y[:4], 2, output="augment", augment=aug)
        assert "spv_loader_fetch" in str(e.value) and "spv_augment_u8" in str(e.value)
    # the loader's own refusals hold for this output too
    with pytest.raises(ValueError, match="n < batch"):
        ResidentLoader(x, y, 65, output="augment", augment=aug3)
    with pytest.raises(ValueError, match="steps_per_epoch"):
        ResidentLoader(x, y, 8, output="augment", augment=aug3, steps_per_epoch=9)
    with pytest.raises(ValueError, match="output is one of"):
        ResidentLoader(x, y, 8, output="augmented", augment=aug3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # everything in order but the device: still nothing is launched
        ResidentLoader(x, y, 8, output="augment", augment=aug3)
