"""The resident loader for the tiled sizes and for distillation, the host side (no GPU): the ABI of spv_loader_fetch_augment_tiled, the
truth table of spv_loader_augment_tiled_supported against spv_augment_plan, every refusal of the C entry point -- the fetch's, the
draw's and the tiled apply's -- with dummy pointers, every refusal of ResidentLoader(output="augment_tiled") with the library's
launches replaced by an assertion, train_distill's argument checks and GraphedDistillStep(loader=)'s constructor refusals."""
import ctypes
import inspect
import os
import types

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
    assert hasattr(lib, "spv_loader_fetch_augment_tiled") and "int spv_loader_fetch_augment_tiled(" in src
    assert hasattr(lib, "spv_loader_augment_tiled_supported") and "int spv_loader_augment_tiled_supported(" in src
    # spv_loader_fetch_augment's arguments, then the workspace and its size in front of the stream: no by-value step
    sig, lds = _native.SIGNATURES["spv_loader_fetch_augment_tiled"], _native.SIGNATURES["spv_loader_fetch_augment"]
    assert len(sig) == 25 and sig[:22] == lds[:22] and sig[22:] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert sig[:22].count(ctypes.c_uint64) == 2   # the two seeds
    assert len(_native.SIGNATURES["spv_loader_augment_tiled_supported"]) == 3 and "spv_loader_augment_tiled_supported" in _native._NO_STATUS
    # no new census slot, no version change
    assert "SPV_PATH_COUNT = 27" in src and len(_native.PATH) == 27 and lib.spv_version() == 1
    # the work model: (n, batch, chans, height, width, world, rank, steps, shuffle, label dtype, null mask, hint); the image is read twice
    model = timing._WORK_MODELS["spv_loader_fetch_augment_tiled"]
    base = (50000, 64, 3, 224, 224, 1, 0, 97, 1)
    assert model(base + (0, 0, 0))[3:] == ("hbm", 64 * (17.0 + 64.0 + 3 * 224 * 224 * 6))
    assert model(base + (1, 0, 0))[4] == 64 * (24.0 + 64.0 + 3 * 224 * 224 * 6)


def test_support_truth_table_against_the_plan(built):
    from spectre_vit import _native
    fused = lambda c, h, w: _native.call("spv_loader_augment_tiled_supported", c, h, w)
    plan = lambda c, h, w: _native.call("spv_augment_plan", c, h, w)
    sides = (0, 1, 2, 3, 28, 32, 45, 64, 70, 89, 92, 130, 224, 511, 512, 513, 4000)
    for c in (0, 1, 2, 3, 4):
        for h in sides:
            for w in sides:
                want = int(plan(c, h, w) >= 1 and 2 <= h <= 512 and 2 <= w <= 512)
                assert fused(c, h, w) == want, (c, h, w)
    assert fused(3, 64, 64) == 1 and fused(3, 224, 224) == 1 and fused(1, 130, 64) == 1 and fused(3, 70, 45) == 1 and fused(3, 512, 512) == 1
    assert fused(3, 32, 32) == 1 and plan(3, 32, 32) == 1, "a plan-1 shape may be forced through"
    assert fused(1, 89, 92) == 1, "the LDS border shape: the tiled fetch takes it, with the tiled chain's bits"
    assert fused(1, 2, 4000) == 0 and plan(1, 2, 4000) == 1, "the loader's sides end at 512"
    assert fused(2, 64, 64) == 0 and fused(3, 1, 64) == 0 and fused(3, 64, 513) == 0 and fused(3, -4, 64) == 0


def test_c_abi_rejects_bad_arguments_before_any_launch(built):
    """every call fails validation on the host (non-zero return, spv_last_error text, RuntimeError from the ctypes wrapper), so nothing
    is launched and no GPU is needed: the fetch's refusals, the draw's, and the tiled apply's"""
    from spectre_vit import _native
    from spectre_vit.augment import TrainAugment
    P = 16   # any non-null, 16-byte aligned "pointer": validation fails before it would be used
    good = TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2)).cfg()
    ws_bytes = lambda b, h, w: _native.call("spv_augment_tiled_ws_bytes", b, h, w)

    def cfg_with(**kw):
        c = TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2)).cfg()
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    keep = []   # the structs stay alive while their addresses are in the case list

    def args(src=P, labels_src=P, cursor=P, index=P, labels=P, params=P, out=P, mean=P, inv_std=P, cfg=good, n=100, batch=10, chans=3,
             height=64, width=64, world=1, rank=0, steps=10, seed=42, shuffle=1, label_dtype=0, aug_seed=7, ws=P, nbytes=None):
        keep.append(cfg)
        if nbytes is None:
            nbytes = ws_bytes(batch, height, width)
        return (src, labels_src, cursor, index, labels, params, out, mean, inv_std, ctypes.addressof(cfg) if cfg is not None else 0, n,
                batch, chans, height, width, world, rank, steps, seed, shuffle, label_dtype, aug_seed, ws, nbytes, 0)

    assert ws_bytes(10, 64, 64) == 40 and ws_bytes(10, 224, 224) == 10 * 13 * 4
    cases = [
        # spv_loader_fetch's
        (args(labels_src=0), "null labels_src"), (args(cursor=0), "null labels_src"), (args(index=0), "null labels_src"),
        (args(labels=0), "null labels_src"),
        (args(src=0), "null src_nhwc"), (args(out=0), "null src_nhwc"),
        (args(cursor=12), "8-byte aligned"),
        (args(mean=0), "mean and inv_std"), (args(inv_std=0), "mean and inv_std"),
        (args(n=0), "n = 0"),
        (args(batch=0, nbytes=40), "batch"), (args(batch=-3, nbytes=40), "batch"),
        (args(world=0), "world"), (args(world=-1), "world"), (args(rank=-1), "rank"), (args(rank=1), "rank"),
        (args(world=2, rank=2, steps=5), "rank"),
        (args(steps=0), "steps_per_epoch"), (args(steps=-1), "steps_per_epoch"), (args(steps=11), "steps_per_epoch"),
        (args(world=2, rank=1, steps=6), "steps_per_epoch"),
        (args(n=2 ** 31 - 1, batch=2 ** 16, world=2 ** 8, steps=2 ** 8), "steps_per_epoch"),
        (args(chans=2), "chans"), (args(chans=0), "chans"), (args(chans=4), "chans"),
        (args(height=0, nbytes=40), "height"), (args(height=513, nbytes=1 << 20), "height"), (args(width=0, nbytes=40), "width"),
        (args(width=513, nbytes=1 << 20), "width"),
        (args(label_dtype=2), "unknown label dtype"), (args(label_dtype=-1), "unknown label dtype"),
        # spv_augment_params's
        (args(params=0), "params / cfg missing"), (args(cfg=None), "params / cfg missing"),
        (args(params=24), "16-byte aligned"),
        (args(height=1, nbytes=40), "bad shape"), (args(width=1, nbytes=40), "bad shape"),
        (args(cfg=cfg_with(blur_p=1.5)), "probability"), (args(cfg=cfg_with(flip_p=-0.1)), "probability"),
        (args(cfg=cfg_with(gray_p=2.0)), "probability"), (args(cfg=cfg_with(erase_p=1.01)), "probability"),
        (args(cfg=cfg_with(sigma_lo=0.0)), "range"), (args(cfg=cfg_with(bright_lo=2.0, bright_hi=1.0)), "range"),
        (args(cfg=cfg_with(hue_hi=0.6)), "range"), (args(cfg=cfg_with(degrees=181.0)), "range"),
        (args(cfg=cfg_with(scale_hi=1.5)), "range"), (args(cfg=cfg_with(ratio_lo=0.0)), "range"),
        # spv_augment_tiled_u8's: the output's alignment, the workspace's presence, size and alignment, the grid
        (args(out=18), "4-byte aligned"),
        (args(ws=0), "workspace missing or too small"), (args(nbytes=39), "workspace missing or too small"),
        (args(nbytes=0), "workspace missing or too small"), (args(ws=0, nbytes=0), "workspace missing or too small"),
        (args(height=224, width=224, nbytes=10 * 13 * 4 - 1), "workspace missing or too small"),
        (args(ws=18), "workspace must be 4-byte aligned"),
        (args(n=2 ** 31 - 1, batch=2 ** 23, steps=1, height=512, width=512, nbytes=1 << 40), "too large a grid"),
    ]
    lib = _native.load()
    counted = _native.call("spv_path_count", _native.PATH["augment"])
    for a, needle in cases:
        assert lib.spv_loader_fetch_augment_tiled(*a) != 0, a
        assert needle in lib.spv_last_error().decode(), (needle, lib.spv_last_error().decode())
        with pytest.raises(RuntimeError) as e:
            _native.call("spv_loader_fetch_augment_tiled", *a)
        assert "spv_loader_fetch_augment_tiled" in str(e.value) and needle in str(e.value), (needle, str(e.value))
    assert _native.call("spv_path_count", _native.PATH["augment"]) == counted, "a refused call is not counted"


def test_python_refusals_touch_no_device(built, monkeypatch):
    """every refusal of ResidentLoader(output="augment_tiled") is raised on the host: the only library entries the constructor may
    reach are host predicates; any other call fails this test, and the tensors stay on the CPU"""
    from spectre_vit import _native
    from spectre_vit.augment import TrainAugment
    from spectre_vit.data import ResidentLoader
    real = _native.call

    def no_launch(name, *a):
        if name in ("spv_loader_augment_tiled_supported", "spv_loader_augment_supported"):
            return real(name, *a)
        raise AssertionError(f"{name} called: a refusal must come before any device work")
    monkeypatch.setattr(_native, "call", no_launch)
    x = torch.zeros((64, 64, 64, 3), dtype=torch.uint8)
    y = torch.zeros(64, dtype=torch.uint8)
    aug3 = TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), seed=1)
    aug1 = TrainAugment((0.5,), (0.2,), seed=1)
    with pytest.raises(ValueError, match="needs augment=TrainAugment"):
        ResidentLoader(x, y, 8, output="augment_tiled")
    with pytest.raises(ValueError, match="needs augment=TrainAugment"):
        ResidentLoader(x, y, 8, output="augment_tiled", augment=lambda *a, **k: None)
    with pytest.raises(ValueError, match="channels"):
        ResidentLoader(x, y, 8, output="augment_tiled", augment=aug1)
    with pytest.raises(ValueError, match="channels"):
        ResidentLoader(torch.zeros((64, 64, 64, 1), dtype=torch.uint8), y, 8, output="augment_tiled", augment=aug3)
    with pytest.raises(ValueError, match="kernel='lds'"):
        ResidentLoader(x, y, 8, output="augment_tiled", augment=TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), kernel="lds"))
    # shapes outside the predicate (the loader's own side limit refuses 513 first)
    for shape in ((4, 1, 64, 3), (4, 64, 1, 3)):
        with pytest.raises(ValueError, match="outside the tiled fetch's shapes"):
            ResidentLoader(torch.zeros(shape, dtype=torch.uint8), y[:4], 2, output="augment_tiled", augment=aug3)
    with pytest.raises(ValueError, match="sides 1 .. 512"):
        ResidentLoader(torch.zeros((4, 513, 8, 3), dtype=torch.uint8), y[:4], 2, output="augment_tiled", augment=aug3)
    # the other outputs keep refusing an augment= of their own, and output="augment" the tiled sizes
    with pytest.raises(ValueError, match="goes with output='augment'"):
        ResidentLoader(x, y, 8, output="none", augment=aug3)
    with pytest.raises(ValueError, match=r"output='none'.*spv_augment_params"):
        ResidentLoader(x, y, 8, output="augment", augment=aug3)
    # the loader's own refusals hold for this output too
    with pytest.raises(ValueError, match="n < batch"):
        ResidentLoader(x, y, 65, output="augment_tiled", augment=aug3)
    with pytest.raises(ValueError, match="steps_per_epoch"):
        ResidentLoader(x, y, 8, output="augment_tiled", augment=aug3, steps_per_epoch=9)
    with pytest.raises(ValueError, match="output is one of"):
        ResidentLoader(x, y, 8, output="augment-tiled", augment=aug3)
    for kernel in ("auto", "tiled"):   # everything in order but the device: still nothing is launched
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ResidentLoader(x, y, 8, output="augment_tiled", augment=TrainAugment((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), kernel=kernel))


def test_harness_picks_the_output_by_shape(built):
    from spectre_vit import harness
    pick = harness._loader_output
    assert pick(False, False, 3, 32, 32) == "float" and pick(False, True, 3, 32, 32) == "uint8" and pick(False, False, 3, 224, 224) == "float"
    assert pick(True, False, 3, 32, 32) == "augment" and pick(True, False, 1, 28, 28) == "augment"
    assert pick(True, False, 3, 64, 64) == "augment_tiled" and pick(True, False, 3, 224, 224) == "augment_tiled"
    assert pick(True, False, 1, 130, 64) == "augment_tiled"
    assert pick(True, False, 1, 89, 92) == "none", "plan 1, refused by the fused LDS fetch: today's path, the whole-image chain's bits"


def test_train_distill_argument_checks_touch_no_device(built, monkeypatch, tmp_path):
    from spectre_vit import harness
    sig = inspect.signature(harness.train_distill)
    assert sig.parameters["device_loader"].default is False
    a = harness.build_parser().parse_args(["--distill-paired", "--device-loader"])
    assert a.device_loader is True and a.distill_paired is True
    assert "--distill-paired" in harness.build_parser().format_help().split("--device-loader")[1]
    cfg = "spectre_vit/configs/spectre_vit_mnist.py"
    out = str(tmp_path / "x")
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="device_loader"):
            harness.train_distill(cfg, out_dir=out, device_loader=bad)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="graph=True"):
        harness.train_distill(cfg, out_dir=out, graph=True, device_loader=True)
    monkeypatch.delenv("WORLD_SIZE")
    assert not os.path.exists(out), "a refused run leaves nothing behind"


def test_graphed_distill_step_loader_refusals_come_first():
    """no model, optimizer or device is looked at: the loader is a stand-in with the three buffers the step would adopt"""
    from spectre_vit.distillation import TeacherLogitCache
    from spectre_vit.graph import GraphedDistillStep, GraphedTrainStep
    gsig = inspect.signature(GraphedDistillStep.__init__)
    assert gsig.parameters["loader"].default is None and gsig.parameters["loader"].kind is inspect.Parameter.KEYWORD_ONLY
    img, lab, tl = torch.zeros(2, 3, 64, 64), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 10)
    cache, idx = TeacherLogitCache(4, 10, "cpu"), torch.zeros(2, dtype=torch.int64)
    fed = types.SimpleNamespace(img=img, labels=lab, index=idx)
    bare = types.SimpleNamespace(img=None, labels=lab, index=idx)
    for teacher in (dict(teacher_cache=cache), dict(example_teacher_logits=tl)):
        with pytest.raises(ValueError, match="no image output"):
            GraphedDistillStep(None, None, None, None, None, loader=bare, **teacher)
        with pytest.raises(ValueError, match="the batch comes from the loader"):
            GraphedDistillStep(None, None, None, img, lab, loader=fed, **teacher)
        with pytest.raises(ValueError, match="the batch comes from the loader"):
            GraphedDistillStep(None, None, None, None, lab, loader=fed, **teacher)
        with pytest.raises(ValueError, match="pass no example_index"):
            GraphedDistillStep(None, None, None, None, None, loader=fed, example_index=idx, **teacher)
    with pytest.raises(ValueError, match="one of the two"):
        GraphedDistillStep(None, None, None, None, None, loader=fed)
    with pytest.raises(ValueError, match="one of the two"):
        GraphedDistillStep(None, None, None, None, None, tl, teacher_cache=cache, loader=fed)
    # the plain step's refusals are worded alike
    with pytest.raises(ValueError, match="no image output"):
        GraphedTrainStep(None, None, None, None, None, loader=bare)
