"""CPU checks of the cached teacher (spectre_vit.distillation.TeacherLogitCache, the indexed distillation loss of csrc/spv_distill.hip,
harness.train_distill(cache_teacher=True)): the C-ABI's symbols, census slot and host-side refusals, the pure split of the fill over
ranks, the file format, and the public surface's defaults and refusals.  Everything here fails on the parent commit (no such symbols,
classes or arguments)."""
import inspect
import os
import re

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


ST, FW, BW = "spv_logit_cache_store", "spv_distill_loss_idx_fwd", "spv_distill_loss_idx_bwd"


def test_symbols_are_exported_and_bound_and_the_census_slot_is_8(built):
    from conftest import ROOT
    from spectre_vit import _native
    lib = _native.load()
    for name in (ST, FW, BW):
        assert name in _native.SIGNATURES and getattr(lib, name).argtypes == _native.SIGNATURES[name]
    assert len(_native.SIGNATURES[ST]) == 7 and len(_native.SIGNATURES[FW]) == len(_native.SIGNATURES[BW]) == 14
    hdr = open(os.path.join(ROOT, "include", "spv.h")).read()
    for name in (ST, FW, BW):
        assert re.search(r"\bint " + name + r"\(", hdr), name
    enum = dict(re.findall(r"(SPV_PATH_[A-Z0-9_]+)\s*=\s*(\d+)", hdr))
    assert int(enum["SPV_PATH_DISTILL_CACHED"]) == _native.PATH["distill_cached"] == 8
    assert int(enum["SPV_PATH_COUNT"]) == 27
    assert sorted(_native.PATH.values()) == list(range(27)), "every census slot has one name"


def test_entry_points_reject_bad_arguments_before_any_launch(built):
    """Every call fails validation on the host: nothing is launched (no GPU here; the pointers are never followed).  An index outside
    the cache is not among them: it lives on the device."""
    from spectre_vit import _native
    nan, inf = float("nan"), float("inf")
    # store: cache, index, logits, rows, n_cache, classes, stream
    # idx:   student, cache, index, labels, lse3 | lse3, out3 | grad_out, workspace | dlogits, rows, n_cache, classes, T, w_soft, w_ce, stream
    ok = (16, 16, 16, 16, 16, 16, 16, 4, 9, 10, 2.0, 0.25, 0.75, 0)

    def but(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return tuple(a)

    cases = [
        (ST, (0, 16, 16, 4, 9, 10, 0), "cache"),
        (ST, (16, 16, 0, 4, 9, 10, 0), "logits"),
        (ST, (16, 16, 16, 0, 9, 10, 0), "empty"),
        (ST, (16, 16, 16, -3, 9, 10, 0), "empty"),
        (ST, (16, 16, 16, 4, 0, 10, 0), "empty"),
        (ST, (16, 16, 16, 4, 9, 0, 0), "empty"),
        (ST, (16, 0, 16, 10, 9, 10, 0), "n_cache"),      # index == NULL and more rows than the cache has
        (ST, (18, 16, 16, 4, 9, 10, 0), "aligned"),
    ]
    for name in (FW, BW):
        cases += [
            (name, but(a0=0), "student"),
            (name, but(a1=0), "teacher"),
            (name, but(a2=0), "index"),
            (name, but(a3=0), "labels"),
            (name, but(a4=0), "missing"),
            (name, but(a5=0), "missing"),
            (name, but(a6=0), "missing"),
            (name, but(a7=0), "empty"),
            (name, but(a7=-1), "empty"),
            (name, but(a8=0), "n_cache"),
            (name, but(a8=-5), "n_cache"),
            (name, but(a9=0), "empty"),
            (name, but(a10=0.0), "temperature"),
            (name, but(a10=-1.0), "temperature"),
            (name, but(a10=nan), "temperature"),
            (name, but(a10=inf), "temperature"),
            (name, but(a11=inf), "weight"),
            (name, but(a12=nan), "weight"),
        ]
    before = _native.call("spv_path_count", 8)
    for name, args, needle in cases:
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, args, needle, str(e.value))
    assert _native.call("spv_path_count", 8) == before, "a refused call is not counted"


@pytest.mark.parametrize("n", [1, 7, 512, 1000])
@pytest.mark.parametrize("batch", [1, 64, 512])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_fill_plan_covers_every_row_exactly_once(n, batch, world):
    from spectre_vit.distillation import fill_plan
    seen = [0] * n
    blocks = (n + batch - 1) // batch
    per_rank = []
    for rank in range(world):
        plan = fill_plan(n, batch, rank, world)
        per_rank.append(len(plan))
        for j, (start, stop) in enumerate(plan):
            assert 0 <= start < stop <= n and stop - start <= batch
            assert start == (j * world + rank) * batch, "a rank's j-th block is block j * world + rank: round j of the exchange"
            for r in range(start, stop):
                seen[r] += 1
    assert seen == [1] * n
    assert sum(per_rank) == blocks and max(per_rank) - min(per_rank) <= 1
    assert fill_plan(n, batch) == fill_plan(n, batch, 0, 1)


def test_fill_plan_refuses_nonsense():
    from spectre_vit.distillation import fill_plan
    for bad in ((0, 4, 0, 1), (4, 0, 0, 1), (4, 4, 1, 1), (4, 4, -1, 2), (4, 4, 0, 0)):
        with pytest.raises(ValueError, match="fill_plan"):
            fill_plan(*bad)


def _filled(n=9, classes=10, seed=0):
    from spectre_vit.distillation import TeacherLogitCache
    c = TeacherLogitCache(n, classes, "cpu")
    assert c.logits.shape == (n, classes) and c.logits.dtype == torch.float32 and torch.isnan(c.logits).all() and not c.complete()
    c.logits.copy_(torch.randn(n, classes, generator=torch.Generator().manual_seed(seed)))
    c.logits[3, 4] = -0.0   # a sign bit a value comparison would not see
    assert c.complete()
    return c


def test_save_and_load_round_trip_bit_for_bit_and_check_the_meta(tmp_path):
    from spectre_vit.distillation import TeacherLogitCache
    c = _filled()
    path = str(tmp_path / "teacher.pt")
    c.save(path, resize=256, crop=224, tag="SyntheticTeacher")
    meta = dict(n=9, classes=10, resize=256, crop=224, tag="SyntheticTeacher")
    blob = torch.load(path, weights_only=True)
    assert set(blob) == {"logits", "meta"} and blob["meta"] == meta and blob["logits"].dtype == torch.float32
    back = TeacherLogitCache.load(path, "cpu", **meta)
    assert (back.n, back.classes) == (9, 10) and back.logits.data_ptr() != c.logits.data_ptr()
    assert torch.equal(back.logits.view(torch.int32), c.logits.view(torch.int32)), "the same bits"
    assert torch.equal(TeacherLogitCache.load(path, "cpu").logits.view(torch.int32), c.logits.view(torch.int32))   # nothing expected
    for field, other in dict(n=10, classes=100, resize=224, crop=192, tag="DinoClassifier").items():
        with pytest.raises(ValueError, match=rf"\b{field}="):
            TeacherLogitCache.load(path, "cpu", **dict(meta, **{field: other}))
    with pytest.raises(ValueError, match="unknown meta"):
        TeacherLogitCache.load(path, "cpu", colour=1)
    with pytest.raises(ValueError, match="unknown meta"):
        c.save(path, colour=1)


def test_an_incomplete_file_is_refused(tmp_path):
    from spectre_vit.distillation import TeacherLogitCache
    c = _filled()
    c.logits[5] = float("nan")
    assert not c.complete()
    path = str(tmp_path / "holes.pt")
    c.save(path, resize=256, crop=224, tag="t")
    with pytest.raises(ValueError, match="incomplete"):
        TeacherLogitCache.load(path, "cpu")


def test_cache_refusals_on_the_host():
    from spectre_vit.distillation import DistillationLoss, SyntheticTeacher, TeacherLogitCache
    for bad in ((0, 10), (4, 0)):
        with pytest.raises(ValueError, match="TeacherLogitCache"):
            TeacherLogitCache(*bad, "cpu")
    c = TeacherLogitCache(4, 10, "cpu")
    with pytest.raises(ValueError, match="store"):
        c.store(None, torch.zeros(2, 11))
    with pytest.raises(ValueError, match="store"):
        c.store(torch.zeros(2, dtype=torch.int32), torch.zeros(2, 10))
    with pytest.raises(ValueError, match="store"):
        c.store(torch.zeros(3, dtype=torch.int64), torch.zeros(2, 10))
    with pytest.raises(RuntimeError, match="GPU"):
        c.store(None, torch.zeros(2, 10))            # no CPU fallback
    teacher = SyntheticTeacher(10, 384, 1)
    images = torch.zeros(4, 28, 28, 1, dtype=torch.uint8)
    with pytest.raises(ValueError, match="train mode"):
        c.fill(teacher.train(), None, images)
    with pytest.raises(ValueError, match="4 rows"):
        c.fill(teacher.eval(), None, images[:3])
    assert torch.isnan(c.logits).all(), "a refused call writes nothing"
    crit = DistillationLoss()
    with pytest.raises(RuntimeError, match="GPU"):
        crit(torch.zeros(2, 10), c, torch.zeros(2, dtype=torch.int64), index=torch.zeros(2, dtype=torch.int64))


def test_public_surface_defaults_and_refusals_before_a_device_is_touched(built, monkeypatch, tmp_path):
    from spectre_vit import harness, hip_ops
    from spectre_vit.distillation import DistillationLoss, TeacherLogitCache
    from spectre_vit.graph import GraphedDistillStep
    sig = inspect.signature(harness.train_distill)
    assert sig.parameters["cache_teacher"].default is False and sig.parameters["teacher_cache_path"].default is None
    assert list(sig.parameters)[-2:] == ["cache_teacher", "teacher_cache_path"], "added behind the existing arguments"
    fsig = inspect.signature(TeacherLogitCache.fill)
    assert [fsig.parameters[k].default for k in ("batch_size", "rank", "world", "process_group", "batch_hook")] == [512, 0, 1, None, None]
    assert inspect.signature(DistillationLoss.forward).parameters["index"].default is None
    lsig = inspect.signature(hip_ops.distill_loss_cached)
    assert list(lsig.parameters)[:4] == ["student_logits", "cache", "index", "labels"]
    assert [lsig.parameters[k].default for k in ("T", "w_soft", "w_ce")] == [2.0, 0.25, 0.75]
    assert issubclass(hip_ops.DistillLossIdxFn, torch.autograd.Function) and hip_ops.DistillLossIdxFn is not hip_ops.DistillLossFn
    gsig = inspect.signature(GraphedDistillStep.__init__)
    assert gsig.parameters["example_teacher_logits"].default is None
    for k in ("teacher_cache", "example_index"):
        assert gsig.parameters[k].default is None and gsig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY

    a = harness.build_parser().parse_args([])
    assert a.cache_teacher is False and a.teacher_cache is None
    a = harness.build_parser().parse_args(["--distill-paired", "--cache-teacher", "--teacher-cache", "t.pt"])
    assert a.cache_teacher is True and a.teacher_cache == "t.pt"

    cfg = "spectre_vit/configs/spectre_vit_mnist.py"
    out = str(tmp_path / "x")
    with pytest.raises(ValueError, match="cache_teacher"):
        harness.train_distill(cfg, out_dir=out, teacher_cache_path=str(tmp_path / "t.pt"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="graph=True"):
        harness.train_distill(cfg, out_dir=out, graph=True, cache_teacher=True)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="teacher view"):
        harness.train_distill(cfg, out_dir=out, cache_teacher=True, crop=300)
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "t.pt"), "a refused run leaves nothing behind"


def test_graphed_distill_step_refuses_both_and_neither_teacher_arguments():
    """the refusal comes first: no model, optimizer or device is looked at"""
    from spectre_vit.distillation import TeacherLogitCache
    from spectre_vit.graph import GraphedDistillStep
    img, lab, tl = torch.zeros(2, 1, 28, 28), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 10)
    cache, idx = TeacherLogitCache(4, 10, "cpu"), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="one of the two"):
        GraphedDistillStep(None, None, None, img, lab)
    with pytest.raises(ValueError, match="one of the two"):
        GraphedDistillStep(None, None, None, img, lab, tl, teacher_cache=cache, example_index=idx)
    with pytest.raises(ValueError, match="go together"):
        GraphedDistillStep(None, None, None, img, lab, teacher_cache=cache)
    with pytest.raises(ValueError, match="go together"):
        GraphedDistillStep(None, None, None, img, lab, tl, example_index=idx)
