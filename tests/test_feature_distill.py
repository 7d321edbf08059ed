"""CPU checks of the feature-matching term of distillation (csrc/spv_distill.hip: spv_feature_cosine_*; hip_ops.FeatureCosineFn /
FeatureCosineIdxFn; DistillationLoss(feature_loss_weight=); TeacherLogitCache(feature_dim=); harness.train_distill(feature_loss_weight=)):
the numpy restatement against float64 torch, the stated zero-row deviation, the C-ABI's symbols and host-side refusals, and the public
surface's defaults and refusals.  Everything but the restatement's own checks fails on the parent commit (no such symbols or arguments)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import feature_cosine_ref as R


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def torch_oracle(s, t, go=1.0, w=1.0):
    """the reference's three lines in float64 torch, with autograd -> (feat, d(go * w * feat)/ds)"""
    st = torch.from_numpy(np.asarray(s, np.float64)).requires_grad_(True)
    tt = torch.from_numpy(np.asarray(t, np.float64))
    a = torch.nn.functional.normalize(st, dim=-1)
    b = torch.nn.functional.normalize(tt, dim=-1)
    feat = 1 - torch.nn.CosineSimilarity()(a, b).mean()
    (feat * (go * w)).backward()
    return feat.item(), st.grad.numpy()


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("width", [1, 3, 64, 65, 384])
def test_restatement_equals_float64_torch(width):
    rng = np.random.default_rng(100 + width)
    s, t = R.rows_in_range(rng, 37, width), R.rows_in_range(rng, 37, width)
    norms = np.sqrt((s.astype(np.float64) ** 2).sum(1))
    assert norms.min() >= 1e-3 and norms.max() <= 1e3
    feat, stat = R.forward(s, t)
    ds = R.backward(s, t, stat, go=1.7, w=0.5)
    rf, rds = torch_oracle(s, t, go=1.7, w=0.5)
    scale = np.abs(rds).max()
    print(f"width {width}: feat {feat:.17g} torch {rf:.17g}; ds max |diff| {np.abs(ds - rds).max():.3e} of {scale:.3e}")
    assert abs(feat - rf) <= 1e-12
    assert np.abs(ds - rds).max() <= 1e-12 * scale
    assert np.abs(stat[2]).max() <= 1 + 1e-12


def test_the_zero_row_deviation_is_what_the_document_says():
    """a row whose |s| (or |t|) is below 1e-12: the oracle's clamp_min leaves a gradient of order 1e12 for it; the restatement gives
    cos = 0 and a zero gradient row, and every other row is untouched"""
    rng = np.random.default_rng(5)
    s, t = R.rows_in_range(rng, 6, 48), R.rows_in_range(rng, 6, 48)
    s[2] = 0.0
    s[2, 0] = 1e-19
    t[4] = 0.0
    feat, stat = R.forward(s, t)
    ds = R.backward(s, t, stat)
    assert stat[2][2] == 0.0 and stat[2][4] == 0.0 and not ds[2].any() and not ds[4].any()
    rf, rds = torch_oracle(s, t)
    assert np.abs(rds[2]).max() > 1e9, "the oracle's gradient of the clamped row is huge"
    keep = [0, 1, 3, 5]
    assert np.abs(ds[keep] - rds[keep]).max() <= 1e-12 * np.abs(rds[keep]).max()
    # forward: an exactly zero row (row 4) has cos = 0 in the oracle too (0 / eps).  The tiny but non-zero row 2 keeps its direction
    # through both clamps there -- cos = t[2, 0] / |t[2]| -- where the restatement says 0: the deviation moves feat by that over rows
    kept = float(t[2, 0]) / float(np.sqrt((t[2].astype(np.float64) ** 2).sum()))
    assert abs(kept) > 1e-3 and abs((feat - rf) - kept / 6) <= 1e-12
    f32, s32 = R.forward32(s, t)
    assert s32[2][2] == 0.0 and s32[2][4] == 0.0 and not R.backward32(s, t, s32)[2].any()


# ---------------------------------------------------------------- the C ABI
FW, BW, IFW, IBW = "spv_feature_cosine_fwd", "spv_feature_cosine_bwd", "spv_feature_cosine_idx_fwd", "spv_feature_cosine_idx_bwd"


def test_symbols_are_exported_and_bound_and_no_census_slot_is_added(built):
    from conftest import ROOT
    from spectre_vit import _native, hip_ops, timing
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "spv.h")).read()
    for name, nargs in ((FW, 10), (BW, 11), (IFW, 11), (IBW, 12)):
        assert name in _native.SIGNATURES and getattr(lib, name).argtypes == _native.SIGNATURES[name]
        assert len(_native.SIGNATURES[name]) == nargs and _native.SIGNATURES[name][-1] is _native.c_vp
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in timing._WORK_MODELS, "bench.py's roofline pass brackets every launch it sees"
    assert _native.call("spv_feature_cosine_workspace_floats") == 65
    enum = dict(re.findall(r"(SPV_PATH_[A-Z0-9_]+)\s*=\s*(\d+)", hdr))
    assert int(enum["SPV_PATH_COUNT"]) == 27 and sorted(_native.PATH.values()) == list(range(27))
    for fn in (hip_ops.FeatureCosineFn, hip_ops.FeatureCosineIdxFn):
        assert issubclass(fn, torch.autograd.Function)
    assert hip_ops.FeatureCosineFn is not hip_ops.FeatureCosineIdxFn
    label, shape, dt, bound, work = timing._WORK_MODELS[FW]((512, 768, 0, 1, 0, 0))
    assert (label, list(shape), bound) == ("feature_cosine_fwd", [512, 768], "hbm") and work == 512 * 768 * 6


def test_entry_points_reject_bad_arguments_before_any_launch(built):
    """Every call fails validation on the host: nothing is launched (no GPU here; the pointers are never followed)"""
    from spectre_vit import _native
    nan, inf = float("nan"), float("inf")
    from spectre_vit._launch import BF16, F32
    bad_dt = max(F32, BF16) + 5
    # fwd:  student, teacher, stat3, out, workspace, rows, width, s_dtype, t_dtype, stream
    # bwd:  student, teacher, stat3, grad_out, dstudent, rows, width, s_dtype, t_dtype, w, stream
    # ifwd: student, cache, index, stat3, out, workspace, rows, n_cache, width, s_dtype, stream
    # ibwd: student, cache, index, stat3, grad_out, dstudent, rows, n_cache, width, s_dtype, w, stream
    ok = {FW: (16, 16, 16, 16, 16, 4, 48, F32, BF16, 0), BW: (16, 16, 16, 16, 16, 4, 48, BF16, F32, 0.5, 0),
          IFW: (16, 16, 16, 16, 16, 16, 4, 9, 48, F32, 0), IBW: (16, 16, 16, 16, 16, 16, 4, 9, 48, BF16, 0.5, 0)}

    def but(name, **kw):
        a = list(ok[name])
        for k, v in kw.items():
            a[int(k[1:])] = v
        return tuple(a)

    cases = []
    for name, nptr, rows_at in ((FW, 5, 5), (BW, 5, 5), (IFW, 6, 6), (IBW, 6, 6)):
        for p in range(nptr):
            cases.append((name, but(name, **{f"a{p}": 0}), "missing"))
        cases += [(name, but(name, **{f"a{rows_at}": 0}), "empty"), (name, but(name, **{f"a{rows_at}": -2}), "empty"),
                  (name, but(name, **{f"a{rows_at}": (1 << 24) + 1}), "2^24")]
    for name in (FW, BW):
        cases += [(name, but(name, a6=0), "empty"), (name, but(name, a6=-1), "empty"), (name, but(name, a7=bad_dt), "dtype"),
                  (name, but(name, a8=bad_dt), "dtype"), (name, but(name, a7=-1), "dtype")]
    for name in (IFW, IBW):
        cases += [(name, but(name, a7=0), "n_cache"), (name, but(name, a7=-5), "n_cache"), (name, but(name, a8=0), "empty"),
                  (name, but(name, a9=bad_dt), "dtype")]
    cases += [(BW, but(BW, a9=nan), "weight"), (BW, but(BW, a9=inf), "weight"), (IBW, but(IBW, a10=nan), "weight"),
              (IBW, but(IBW, a10=-inf), "weight")]
    counts = [_native.call("spv_path_count", k) for k in range(27)]
    for name, args, needle in cases:
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, args, needle, str(e.value))
    assert [_native.call("spv_path_count", k) for k in range(27)] == counts, "a refused call counts nothing"


# ---------------------------------------------------------------- DistillationLoss
def test_distillation_loss_surface_defaults_and_refusals():
    from spectre_vit import hip_ops
    from spectre_vit.distillation import DistillationLoss, TeacherLogitCache
    from spectre_vit.meter import TrainMeter
    sig = inspect.signature(DistillationLoss.__init__)
    assert list(sig.parameters) == ["self", "T", "soft_target_loss_weight", "ce_loss_weight", "meter", "feature_loss_weight"]
    assert sig.parameters["feature_loss_weight"].default == 0.0
    fsig = inspect.signature(DistillationLoss.forward)
    assert list(fsig.parameters) == ["self", "student_logits", "teacher_logits", "labels", "index", "student_feat", "teacher_feat"]
    assert fsig.parameters["student_feat"].default is None and fsig.parameters["teacher_feat"].default is None
    lsig = inspect.signature(hip_ops.distill_loss)
    assert list(lsig.parameters) == ["student_logits", "teacher_logits", "labels", "T", "w_soft", "w_ce", "meter"], "pinned: unchanged"
    crit = DistillationLoss()
    assert crit.feature_loss_weight == 0.0 and crit.feat is None and crit.soft is None and crit.ce is None
    on = DistillationLoss(feature_loss_weight=0.5)
    assert on.feature_loss_weight == 0.5 and on.feat is None
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="feature_loss_weight"):
            DistillationLoss(feature_loss_weight=bad)
    meter = object.__new__(TrainMeter)   # the refusal looks at no device
    with pytest.raises(ValueError, match=r"feature_loss_weight=0\.5.*meter"):
        DistillationLoss(feature_loss_weight=0.5, meter=meter)
    z, y = torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"feature_loss_weight=0\.5.*student_feat=None"):
        on(z, z, y)
    with pytest.raises(ValueError, match=r"teacher_feat=None"):
        on(z, z, y, student_feat=torch.zeros(2, 48))
    with pytest.raises(ValueError, match=r"\(2, 48\).*\(2, 64\).*project inside the teacher module"):
        on(z, z, y, student_feat=torch.zeros(2, 48), teacher_feat=torch.zeros(2, 64))
    cache = TeacherLogitCache(4, 10, "cpu")   # no features
    with pytest.raises(ValueError, match=r"teacher_feat=None"):
        on(z, cache, y, index=y, student_feat=torch.zeros(2, 48))
    with pytest.raises(RuntimeError, match="GPU"):   # the checks passed; there is no CPU fallback
        on(z, z, y, student_feat=torch.zeros(2, 48), teacher_feat=torch.zeros(2, 48))
    with pytest.raises(RuntimeError, match="GPU"):   # weight 0.0: features are allowed and ignored (of any shape)
        crit(z, z, y, student_feat=torch.zeros(2, 48), teacher_feat=torch.zeros(3, 7))
    assert on.feat is None and crit.feat is None


# ---------------------------------------------------------------- TeacherLogitCache(feature_dim=)
def _filled(n=9, classes=10, feature_dim=6, seed=0):
    from spectre_vit.distillation import TeacherLogitCache
    c = TeacherLogitCache(n, classes, "cpu", feature_dim=feature_dim)
    g = torch.Generator().manual_seed(seed)
    c.logits.copy_(torch.randn(n, classes, generator=g))
    if feature_dim is not None:
        assert c.features.shape == (n, feature_dim) and c.features.dtype == torch.float32 and torch.isnan(c.features).all()
        assert not c.complete(), "the logits alone do not complete a cache with features"
        c.features.copy_(torch.randn(n, feature_dim, generator=g))
        c.features[3, 4] = -0.0
    assert c.complete()
    return c


def test_feature_cache_saves_and_loads_bit_for_bit_and_old_files_still_load(tmp_path):
    from spectre_vit.distillation import TeacherLogitCache
    assert inspect.signature(TeacherLogitCache.__init__).parameters["feature_dim"].default is None
    assert inspect.signature(TeacherLogitCache.store).parameters["features"].default is None
    plain = TeacherLogitCache(4, 10, "cpu")
    assert plain.features is None and plain.feature_dim is None
    with pytest.raises(ValueError, match="feature_dim"):
        TeacherLogitCache(4, 10, "cpu", feature_dim=0)
    c = _filled()
    path = str(tmp_path / "with.pt")
    c.save(path, resize=256, crop=224, tag="SyntheticTeacher")
    blob = torch.load(path, weights_only=True)
    assert set(blob) == {"logits", "features", "meta"} and blob["meta"]["feature_dim"] == 6
    back = TeacherLogitCache.load(path, "cpu", feature_dim=6, n=9, classes=10, resize=256, crop=224, tag="SyntheticTeacher")
    assert back.feature_dim == 6
    assert torch.equal(back.logits.view(torch.int32), c.logits.view(torch.int32)), "the same bits"
    assert torch.equal(back.features.view(torch.int32), c.features.view(torch.int32)), "the same bits"
    with pytest.raises(ValueError, match=r"feature_dim=6.*feature_dim=48"):
        TeacherLogitCache.load(path, "cpu", feature_dim=48)
    assert TeacherLogitCache.load(path, "cpu").features is None, "features not asked for are left out"
    # the file of a cache without features: today's format, key for key; it loads, and is refused by name when features are wanted
    old = str(tmp_path / "old.pt")
    o = _filled(feature_dim=None)
    o.save(old, resize=256, crop=224, tag="t")
    blob = torch.load(old, weights_only=True)
    assert set(blob) == {"logits", "meta"} and blob["meta"] == dict(n=9, classes=10, resize=256, crop=224, tag="t")
    assert torch.equal(TeacherLogitCache.load(old, "cpu", n=9).logits.view(torch.int32), o.logits.view(torch.int32))
    with pytest.raises(ValueError, match=r"old\.pt holds no features"):
        TeacherLogitCache.load(old, "cpu", feature_dim=6)
    # a hole in the features makes the file incomplete
    c.features[5] = float("nan")
    assert not c.complete()
    c.save(path)
    with pytest.raises(ValueError, match="incomplete"):
        TeacherLogitCache.load(path, "cpu", feature_dim=6)
    # store's host-side refusals
    with pytest.raises(ValueError, match="needs features"):
        c.store(None, torch.zeros(2, 10))
    with pytest.raises(ValueError, match="takes no features"):
        plain.store(None, torch.zeros(2, 10), torch.zeros(2, 6))
    with pytest.raises(ValueError, match=r"features \[2, 6\]"):
        c.store(None, torch.zeros(2, 10), torch.zeros(2, 7))
    with pytest.raises(RuntimeError, match="GPU"):
        c.store(None, torch.zeros(2, 10), torch.zeros(2, 6))


# ---------------------------------------------------------------- harness
def test_train_distill_default_refusals_and_flag_before_a_device_is_touched(built, monkeypatch, tmp_path):
    from spectre_vit import harness
    from spectre_vit.graph import GraphedDistillStep
    sig = inspect.signature(harness.train_distill)
    assert sig.parameters["feature_loss_weight"].default == 0.0
    gsig = inspect.signature(GraphedDistillStep.__init__)
    assert gsig.parameters["example_teacher_feat"].default is None
    assert gsig.parameters["example_teacher_feat"].kind is inspect.Parameter.KEYWORD_ONLY

    a = harness.build_parser().parse_args([])
    assert a.feature_loss_weight == 0.0
    a = harness.build_parser().parse_args(["--distill-paired", "--feature-loss-weight", "0.5"])
    assert a.feature_loss_weight == 0.5
    seen = {}
    monkeypatch.setattr(harness, "train_distill", lambda *args, **kw: seen.update(kw))
    harness.main(["--distill-paired", "--feature-loss-weight", "0.25"])
    assert seen["feature_loss_weight"] == 0.25
    monkeypatch.undo()

    def no_device(*args, **kw):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    cfg = "spectre_vit/configs/spectre_vit_mnist.py"
    out = str(tmp_path / "x")
    for bad in (float("nan"), float("inf"), -0.5, "0.5", True):
        with pytest.raises(ValueError, match="feature_loss_weight"):
            harness.train_distill(cfg, out_dir=out, feature_loss_weight=bad)
    with pytest.raises(ValueError, match=r"feature_loss_weight=0\.5 with device_meter=True"):
        harness.train_distill(cfg, out_dir=out, feature_loss_weight=0.5, device_meter=True)
    # later than the existing refusals: each of those still wins
    with pytest.raises(ValueError, match="cache_teacher"):
        harness.train_distill(cfg, out_dir=out, feature_loss_weight=-1.0, teacher_cache_path=str(tmp_path / "t.pt"))
    with pytest.raises(ValueError, match="teacher view"):
        harness.train_distill(cfg, out_dir=out, feature_loss_weight=-1.0, crop=300)
    with pytest.raises(ValueError, match="temperature"):
        harness.train_distill(cfg, out_dir=out, feature_loss_weight=-1.0, T=0.0)
    with pytest.raises(ValueError, match="device_loader"):
        harness.train_distill(cfg, out_dir=out, feature_loss_weight=-1.0, device_loader=1)
    assert not os.path.exists(out), "a refused run leaves nothing behind"


def test_graphed_distill_step_refuses_a_featured_criterion_without_teacher_features():
    """the refusal comes first: no model, optimizer or device is looked at"""
    from spectre_vit.distillation import DistillationLoss, TeacherLogitCache
    from spectre_vit.graph import GraphedDistillStep
    img, lab, tl = torch.zeros(2, 1, 28, 28), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 10)
    crit = DistillationLoss(feature_loss_weight=0.5)
    with pytest.raises(ValueError, match=r"feature_loss_weight=0\.5 needs example_teacher_feat"):
        GraphedDistillStep(None, None, crit, img, lab, tl)
    with pytest.raises(ValueError, match=r"feature_loss_weight=0\.5 needs a teacher cache with features"):
        GraphedDistillStep(None, None, crit, img, lab, teacher_cache=TeacherLogitCache(4, 10, "cpu"), example_index=lab)
