"""GPU checks of the feature-matching term of distillation (csrc/spv_distill.hip: spv_feature_cosine_fwd / _bwd / _idx_fwd / _idx_bwd)
and of everything built on it: hip_ops.FeatureCosineFn / FeatureCosineIdxFn, DistillationLoss(feature_loss_weight=),
TeacherLogitCache(feature_dim=), GraphedDistillStep and harness.train_distill(feature_loss_weight=).

Bars of the kernels (DESIGN.md section 4d's rule for a quantity without a fixed bound): for each quantity -- feat, |s|, |t|, cos and
dstudent -- the float32 sequential restatement of tests/feature_cosine_ref.py is run on the same inputs, its own largest gap to the
float64 restatement is measured, and the kernel may differ from float64 by 4 x that.  A dstudent stored as bf16 gets one bf16 unit
roundoff (2^-8) of its largest magnitude more.  A gap read off ONE number is a lottery -- the restatement's single result may land
arbitrarily close to the float64 value -- so at a row count below 32 a case repeats the launch on ceil(32 / rows) independent draws of
that shape and takes gap and error as the largest over the draws: every per-row quantity is then measured over at least 32 rows.
Through DistillationLoss the total loss adds the fused loss's existing bound
(2e-6 |ref| + 1e-7, tests/test_gpu_distill.py) to the weighted feature bar and two fp32 roundings of the weighted add.  Eager against
graph: 1e-2 relative per step, the existing eager-vs-graph bound.  Every comparison prints its figures before it asserts (pytest -s).
Every test here fails on the parent commit (a missing symbol or a TypeError)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import feature_cosine_ref as R

pytestmark = pytest.mark.gpu

MNIST = "spectre_vit/configs/spectre_vit_mnist.py"
SENT = -7.0          # exact in fp32 and bf16
GUARD = 64           # sentinel elements on either side of a buffer (a multiple of 16 bytes in both dtypes)
U_BF16 = 2.0 ** -8   # bf16's unit roundoff (8 significand bits, round to nearest)
NAN = float("nan")


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", torch.cuda.current_device())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


class Guarded:
    """a device buffer between two runs of sentinels, its interior `off` elements past a 16-byte aligned address"""

    def __init__(self, shape, dtype, off=0, fill=NAN):
        n = int(np.prod(shape))
        self.base = torch.full((n + 2 * GUARD + 8,), SENT, dtype=dtype, device=dev())
        assert self.base.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.base[self.lo:self.hi].view(shape)
        self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.base[:self.lo] == SENT).all()) and bool((self.base[self.hi:] == SENT).all())


_ws = {}


def workspace():
    """zeroed ONCE for the whole module: every later call finds the counter re-armed by the call before it"""
    from spectre_vit import _native
    if "ws" not in _ws:
        _ws["ws"] = torch.zeros(_native.call("spv_feature_cosine_workspace_floats"), dtype=torch.float32, device=dev())
    return _ws["ws"]


def raw(s, t, go=1.7, w=0.5, off=0, index=None):
    """one forward and one backward through the C ABI on guarded buffers: s, t CPU tensors (fp32 or bf16); index (CPU int64): t is the
    fp32 cache.  off: bytes both input bases (and dstudent) lie past 16-byte alignment.  -> (feat, stat3, dstudent as float32)"""
    from spectre_vit import _native
    from spectre_vit._launch import _DT, _stream
    rows, width = s.shape
    gs = Guarded(s.shape, s.dtype, off // s.element_size())
    gt = Guarded(t.shape, t.dtype, off // t.element_size())
    gs.t.copy_(s)
    gt.t.copy_(t)
    stat, out = Guarded((3, rows), torch.float32), Guarded((1,), torch.float32)
    ds = Guarded(s.shape, s.dtype, off // s.element_size())
    g = torch.tensor([go], dtype=torch.float32, device=dev())
    ws = workspace()
    if index is None:
        assert gs.ptr() % 16 == off and gt.ptr() % 16 == off
        _native.call("spv_feature_cosine_fwd", gs.ptr(), gt.ptr(), stat.ptr(), out.ptr(), ws.data_ptr(), rows, width, _DT[s.dtype],
                     _DT[t.dtype], _stream())
        _native.call("spv_feature_cosine_bwd", gs.ptr(), gt.ptr(), stat.ptr(), g.data_ptr(), ds.ptr(), rows, width, _DT[s.dtype],
                     _DT[t.dtype], w, _stream())
    else:
        idx = index.to(dev())
        _native.call("spv_feature_cosine_idx_fwd", gs.ptr(), gt.ptr(), idx.data_ptr(), stat.ptr(), out.ptr(), ws.data_ptr(), rows,
                     t.shape[0], width, _DT[s.dtype], _stream())
        _native.call("spv_feature_cosine_idx_bwd", gs.ptr(), gt.ptr(), idx.data_ptr(), stat.ptr(), g.data_ptr(), ds.ptr(), rows,
                     t.shape[0], width, _DT[s.dtype], w, _stream())
    torch.cuda.synchronize()
    for name, b in (("student", gs), ("teacher", gt), ("stat3", stat), ("out", out), ("dstudent", ds)):
        assert b.intact(), f"{name}: a sentinel was overwritten"
    bits = {2: torch.int16, 4: torch.int32}   # compared as bits: an unfilled cache row is NaN
    for b, x in ((gs, s), (gt, t)):
        assert torch.equal(b.t.cpu().contiguous().view(bits[x.element_size()]), x.contiguous().view(bits[x.element_size()])), "the inputs are read only"
    assert int(ws[-1:].view(torch.int32)[0].item()) == 0, "the arrival counter is re-armed"
    return out.t.item(), stat.t.cpu().numpy(), ds.t.float().cpu().numpy()


def inputs(rows, width, dtype, seed, t_dtype=torch.float32):
    rng = np.random.default_rng(seed)
    s = torch.from_numpy(R.rows_in_range(rng, rows, width)).to(dtype)
    t = torch.from_numpy(R.rows_in_range(rng, rows, width)).to(t_dtype)
    return s, t


def bars(s, t, go, w):
    """float64 reference and, per quantity, 4 x the float32 sequential restatement's own gap to it"""
    s32, t32 = s.float().numpy(), t.float().numpy()
    feat, stat = R.forward(s32, t32)
    ds = R.backward(s32, t32, stat, go, w)
    f32, st32 = R.forward32(s32, t32)
    ds32 = R.backward32(s32, t32, st32, go, w)
    bar = {"feat": 4 * abs(float(f32) - feat), "|s|": 4 * np.abs(st32[0] - stat[0]).max(), "|t|": 4 * np.abs(st32[1] - stat[1]).max(),
           "cos": 4 * np.abs(st32[2] - stat[2]).max(), "ds": 4 * np.abs(ds32 - ds).max()}
    if s.dtype == torch.bfloat16:
        bar["ds"] += U_BF16 * np.abs(ds).max()
    return feat, stat, ds, bar


def check(what, got, s, t, go, w):
    feat, stat, ds = got
    rf, rstat, rds, bar = bars(s, t, go, w)
    err = {"feat": abs(feat - rf), "|s|": np.abs(stat[0] - rstat[0]).max(), "|t|": np.abs(stat[1] - rstat[1]).max(),
           "cos": np.abs(stat[2] - rstat[2]).max(), "ds": np.abs(ds - rds).max()}
    print(f"{what}: " + "  ".join(f"{k} err {err[k]:.3e} bar {bar[k]:.3e}" for k in err))
    return err, bar


ROWS = [1, 3, 4, 5, 130, 512]
WIDTHS = [1, 3, 4, 63, 64, 65, 384, 385, 768]


# ---------------------------------------------------------------- the kernels against the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
def test_kernels_against_the_restatement(rows, dtype):
    """every width of the list at this row count (ceil(32 / rows) draws of each): forward stats, the loss and the student's gradient
    inside their bars; a second call returns the same bits"""
    failures, draws = [], -(-32 // rows)
    for width in WIDTHS:
        err, bar = {}, {}
        for draw in range(draws):
            s, t = inputs(rows, width, dtype, seed=100000 * draw + 1000 * rows + width)
            got = raw(s, t)
            e, b = check(f"{rows} x {width} {'bf16' if dtype == torch.bfloat16 else 'fp32'} draw {draw}", got, s, t, 1.7, 0.5)
            err = {k: max(e[k], err.get(k, 0.0)) for k in e}
            bar = {k: max(b[k], bar.get(k, 0.0)) for k in b}
            if draw == 0:
                again = raw(s, t)
                assert got[0] == again[0] and same_bits(got[1], again[1]) and same_bits(got[2], again[2]), (width, "two calls, the same bits")
        print(f"{rows} x {width} over {draws} draw(s): " + "  ".join(f"{k} err {err[k]:.3e} bar {bar[k]:.3e}" for k in err))
        failures += [(width, k, float(err[k]), float(bar[k])) for k in err if not err[k] <= bar[k]]
    assert not failures, failures


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_bases_four_bytes_off_alignment(dtype):
    """both input bases 4 bytes past a 16-byte boundary: the element-load path, inside the same bars -- and the bits of the aligned call"""
    s, t = inputs(130, 384, dtype, seed=77, t_dtype=dtype)
    got = raw(s, t, off=4)
    err, bar = check("130 x 384 misaligned", got, s, t, 1.7, 0.5)
    assert all(err[k] <= bar[k] for k in err), (err, bar)
    aligned = raw(s, t)
    assert got[0] == aligned[0] and same_bits(got[1], aligned[1]) and same_bits(got[2], aligned[2])


def test_bf16_teacher_and_fp32_student():
    failures = []
    for rows, width in ((130, 65), (130, 384)):
        s, t = inputs(rows, width, torch.float32, seed=rows + width, t_dtype=torch.bfloat16)
        err, bar = check(f"{rows} x {width} fp32 student, bf16 teacher", raw(s, t), s, t, 1.7, 0.5)
        failures += [(rows, width, k) for k in err if not err[k] <= bar[k]]
    assert not failures, failures


# ---------------------------------------------------------------- the indexed form
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("width", [65, 384])
def test_indexed_equals_dense_on_the_gathered_cache_bit_for_bit(width, dtype):
    rows, n = 130, 50
    rng = np.random.default_rng(width)
    s, _ = inputs(rows, width, dtype, seed=3)
    cache = torch.from_numpy(R.rows_in_range(rng, n, width))
    index = torch.from_numpy(rng.integers(0, n, size=rows).astype(np.int64))
    assert len(set(index.tolist())) < rows, "the index repeats rows"
    dense = raw(s, cache[index].contiguous())
    indexed = raw(s, cache, index=index)
    assert dense[0] == indexed[0] and same_bits(dense[1], indexed[1]) and same_bits(dense[2], indexed[2])
    assert math.isfinite(dense[0])


def test_bad_index_and_unfilled_row_poison_their_rows_only():
    """an index outside [0, n_cache) (either side) and an unfilled (NaN) cache row: their stat3 cos and their dstudent rows are NaN,
    out is NaN, every other row keeps the dense call's bits, no sentinel is touched (raw checks every buffer's)"""
    rows, n, width = 9, 12, 65
    rng = np.random.default_rng(8)
    s, _ = inputs(rows, width, torch.float32, seed=4)
    cache = torch.from_numpy(R.rows_in_range(rng, n, width))
    cache[7] = NAN
    index = torch.tensor([0, 3, n, 5, -1, 7, 11, 3, 2 ** 40], dtype=torch.int64)
    bad = [2, 4, 5, 8]
    good = [r for r in range(rows) if r not in bad]
    feat, stat, ds = raw(s, cache, index=index)
    assert math.isnan(feat)
    assert np.isnan(stat[2][bad]).all() and np.isnan(ds[bad]).all()
    safe = index.clone()
    safe[bad] = 0
    _, dstat, dds = raw(s, cache[safe].contiguous())
    assert same_bits(stat[:, good], dstat[:, good]) and same_bits(ds[good], dds[good]) and np.isfinite(ds[good]).all()
    # the dense form with a NaN teacher row: the same poison
    t = cache[safe].contiguous()
    t[1, 3] = NAN
    feat, stat, ds = raw(s, t)
    assert math.isnan(feat) and np.isnan(stat[2][1]) and np.isnan(ds[1]).all() and np.isfinite(np.delete(ds, 1, 0)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_zero_norm_rows_give_cos_zero_and_a_zero_gradient_row(dtype):
    s, t = inputs(6, 48, dtype, seed=5)
    s[2] = 0.0
    s[2, 0] = 1e-19     # |s| = 1e-19 < 1e-12
    t[4] = 0.0
    got = raw(s, t)
    feat, stat, ds = got
    assert stat[2][2] == 0.0 and stat[2][4] == 0.0 and not ds[2].any() and not ds[4].any()
    assert np.isfinite(ds).all() and ds[[0, 1, 3, 5]].any(axis=1).all()
    # the loss is the mean of the cosines the launch stored, zero rows included: at most ten fp32 roundings of numbers of size at most rows = 6
    assert abs(feat - (1.0 - stat[2].astype(np.float64).mean())) <= 10 * 2.0 ** -24 * 6


# ---------------------------------------------------------------- DistillationLoss
def _logits(rows, classes, seed):
    rng = np.random.default_rng(seed)
    z = (3 * rng.standard_normal((rows, classes))).astype(np.float32)
    t = (3 * rng.standard_normal((rows, classes))).astype(np.float32)
    y = rng.integers(0, classes, size=rows).astype(np.int64)
    return z, t, y


def test_weight_zero_is_the_unchanged_loss_launch_for_launch(monkeypatch):
    from spectre_vit import _native
    from spectre_vit.distillation import DistillationLoss
    d = dev()
    z, t, y = _logits(64, 100, seed=1)
    sf, tf = inputs(64, 48, torch.float32, seed=2)
    real = _native.call

    def run(crit, **feats):
        issued = []

        def recorder(name, *a):
            issued.append(name)
            return real(name, *a)
        zt = torch.from_numpy(z).to(d).requires_grad_(True)
        monkeypatch.setattr(_native, "call", recorder)
        loss = crit(zt, torch.from_numpy(t).to(d), torch.from_numpy(y).to(d), **feats)
        loss.backward()
        monkeypatch.setattr(_native, "call", real)
        return loss.detach().cpu().numpy(), zt.grad.cpu().numpy(), issued

    run(DistillationLoss())   # the first call of a process also asks for the workspace's size: not a step's call
    base = run(DistillationLoss())
    sfd = sf.to(d).requires_grad_(True)
    off = DistillationLoss(feature_loss_weight=0.0)
    zero = run(off, student_feat=sfd, teacher_feat=tf.to(d))
    assert zero[2] == base[2] == ["spv_distill_loss_fwd", "spv_distill_loss_bwd"], (base[2], zero[2])
    assert same_bits(zero[0], base[0]) and same_bits(zero[1], base[1])
    assert off.feat is None and sfd.grad is None, "the features are allowed and ignored"


@pytest.mark.parametrize("shape", [(512, 100, 512), (3, 10, 48)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cached", [False, True], ids=["dense", "cached"])
def test_distillation_loss_with_the_feature_term_against_float64_torch(shape, cached):
    from oracle import spectre_oracle as O
    from spectre_vit.distillation import DistillationLoss, TeacherLogitCache
    rows, classes, width = shape
    d = dev()
    T, ws, wc, wf, up = 2.0, 0.25, 0.75, 0.5, 1.7
    z, t, y = _logits(rows, classes, seed=rows + classes)
    s, tf = inputs(rows, width, torch.float32, seed=rows + width)
    # float64 torch: the reference's three lines with autograd, added to the float64 oracle of the fused loss
    st = s.double().requires_grad_(True)
    feat64 = 1 - torch.nn.CosineSimilarity()(torch.nn.functional.normalize(st, dim=-1), torch.nn.functional.normalize(tf.double(), dim=-1)).mean()
    (feat64 * (wf * up)).backward()
    logit64, dz64, _, _ = O.distill_loss_fwd_bwd(z.astype(np.float64), t.astype(np.float64), y, T, ws, wc)
    ref_loss, ref_feat, ref_ds = float(logit64) + wf * feat64.item(), feat64.item(), st.grad.numpy()

    crit = DistillationLoss(T, ws, wc, feature_loss_weight=wf)
    assert crit.feat is None
    zt, sd = torch.from_numpy(z).to(d).requires_grad_(True), s.to(d).requires_grad_(True)
    if cached:
        n = rows + 7
        index = torch.from_numpy(np.random.default_rng(1).permutation(n)[:rows].astype(np.int64)).to(d)
        cache = TeacherLogitCache(n, classes, d, feature_dim=width)
        cache.store(index, torch.from_numpy(t).to(d), tf.to(d))
        assert not cache.complete(), "seven rows were never stored"
        loss = crit(zt, cache, torch.from_numpy(y).to(d), index=index, student_feat=sd, teacher_feat=cache.features)
    else:
        loss = crit(zt, torch.from_numpy(t).to(d), torch.from_numpy(y).to(d), student_feat=sd, teacher_feat=tf.to(d))
    (loss * up).backward()
    assert crit.feat.dim() == 0 and not crit.feat.requires_grad and crit.feat.is_cuda and loss.requires_grad
    _, _, _, bar = bars(s, tf, up, wf)
    got_loss, got_feat, got_ds = loss.item(), crit.feat.item(), sd.grad.cpu().numpy()
    loss_bar = 2e-6 * abs(float(logit64)) + 1e-7 + wf * bar["feat"] + 2 * 2.0 ** -24 * abs(ref_loss)
    print(f"{shape} {'cached' if cached else 'dense'}: loss {got_loss:.9g} float64 {ref_loss:.9g} |diff| {abs(got_loss - ref_loss):.3e} "
          f"allowed {loss_bar:.3e}; feat {got_feat:.9g} float64 {ref_feat:.9g} |diff| {abs(got_feat - ref_feat):.3e} allowed "
          f"{bar['feat']:.3e}; dstudent max |diff| {np.abs(got_ds - ref_ds).max():.3e} allowed {bar['ds']:.3e}")
    assert abs(got_feat - ref_feat) <= bar["feat"]
    assert abs(got_loss - ref_loss) <= loss_bar
    assert np.abs(got_ds - ref_ds).max() <= bar["ds"]
    scale = np.abs(dz64).max() * up
    assert np.abs(zt.grad.cpu().numpy() - dz64 * up).max() <= 2e-6 * scale, "the logits' gradient is the fused loss's, untouched"


# ---------------------------------------------------------------- GraphedDistillStep
def _student():
    from spectre_vit.models.spectre.spectre import SpectreViT
    torch.manual_seed(11)
    return SpectreViT(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=512, num_encoders=2, num_heads=16,
                      hidden_dim=768, activation="gelu", dropout=0.0, mixer="fft").to(dev()).train()


@pytest.mark.parametrize("mode", ["dense", "cached", "cached_loader"])
def test_graphed_distill_step_with_the_feature_term_follows_the_eager_step(mode, monkeypatch):
    from spectre_vit import _native
    from spectre_vit.data import CIFAR_MEAN, CIFAR_STD, ResidentLoader
    from spectre_vit.distillation import DistillationLoss, TeacherLogitCache
    from spectre_vit.dp import GradReducer
    from spectre_vit.graph import GraphedDistillStep
    from spectre_vit.optim import FusedAdamW
    d = dev()
    g = torch.Generator().manual_seed(3)
    steps, B, n, wf = 5, 64, 400, 0.5
    set_u8 = torch.randint(0, 256, (n, 32, 32, 3), generator=g, dtype=torch.uint8).to(d)
    set_y = torch.randint(0, 100, (n,), generator=g).to(torch.uint8).to(d)
    cache = TeacherLogitCache(n, 100, d, feature_dim=512)
    cache.store(None, (3 * torch.randn(n, 100, generator=g)).to(d), torch.randn(n, 512, generator=g).to(d))
    assert cache.complete()
    new_loader = lambda: ResidentLoader(set_u8, set_y, B, CIFAR_MEAN, CIFAR_STD, seed=9, output="float")
    ld = new_loader()
    fed = []
    for _ in range(steps):
        ld.fetch()
        fed.append((ld.img.clone(), ld.labels.clone().long(), ld.index.clone()))

    def call(crit, logits, feat, k):
        img, lab, idx = fed[k]
        if mode == "dense":
            return crit(logits, cache.logits[idx], lab, student_feat=feat, teacher_feat=cache.features[idx])
        return crit(logits, cache, lab, index=idx, student_feat=feat, teacher_feat=cache.features)

    m = _student()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    red = GradReducer(m)
    crit = DistillationLoss(feature_loss_weight=wf)
    eager = []
    for k in range(steps):
        logits, feat = m(fed[k][0], return_features=True)
        loss = call(crit, logits, feat, k)
        red.zero_grad()
        loss.backward()
        red.finish()
        opt.step()
        eager.append((loss.item(), crit.soft.item(), crit.ce.item(), crit.feat.item()))

    m = _student()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True)
    crit = DistillationLoss(feature_loss_weight=wf)
    img, lab, idx = fed[0]
    if mode == "dense":
        step = GraphedDistillStep(m, opt, crit, img, lab, cache.logits[idx], warmup=1, example_teacher_feat=cache.features[idx])
    elif mode == "cached":
        step = GraphedDistillStep(m, opt, crit, img, lab, warmup=1, teacher_cache=cache, example_index=idx)
    else:
        loader = new_loader()
        step = GraphedDistillStep(m, opt, crit, None, None, warmup=1, teacher_cache=cache, loader=loader)
    real, issued = _native.call, []

    def recorder(name, *a):
        issued.append(name)
        return real(name, *a)
    try:
        graph = [(step.warm_loss.item(), step.warm_soft.item(), step.warm_ce.item(), step.warm_feat.item())]   # the warm-up WAS step 0
        for k in range(1, steps):
            img, lab, idx = fed[k]
            if mode == "dense":
                loss = step(img, lab, cache.logits[idx], teacher_feat=cache.features[idx])
            elif mode == "cached":
                loss = step(img, lab, index=idx)
            else:
                monkeypatch.setattr(_native, "call", recorder)
                loss = step()
                monkeypatch.setattr(_native, "call", real)
                assert torch.equal(loader.index, idx) and step.index is loader.index
            graph.append((loss.item(), step.soft.item(), step.ce.item(), step.feat.item()))
        assert step.replays == steps - 1
        if mode == "cached_loader":
            assert issued == [], f"a step is the one replay: nothing is issued beside it, got {issued}"
            assert loader.step == steps == loader.device_step()
    finally:
        step.close()
    for k, (a, b) in enumerate(zip(eager, graph)):
        print(f"{mode} step {k}: eager (loss, soft, ce, feat) {a}  graph {b}  relative loss difference {abs(a[0] - b[0]) / abs(a[0]):.3e}")
    for a, b in zip(eager, graph):
        for u, v in zip(a, b):
            assert abs(u - v) <= 1e-2 * abs(u), (eager, graph)
    assert eager[-1][0] != eager[0][0]


# ---------------------------------------------------------------- harness.train_distill
KEYS = {"epoch", "Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation", "steps", "val_samples"}


def _train(tmp_path, tag, **kw):
    from spectre_vit.harness import train_distill
    out = str(tmp_path / tag)
    _, hist = train_distill(MNIST, mixer="fft", out_dir=out, log=lambda r: None, epochs=2, steps_per_epoch=4, batch_size=16, n_train=64,
                            n_val=32, **kw)
    lines = [json.loads(l) for l in open(os.path.join(out, "scalars.jsonl"))]
    return hist, [l for l in lines if "Batch Loss/Train" in l]


@pytest.mark.parametrize("fast", [False, True], ids=["eager", "graph_cached_loader"])
def test_train_distill_with_the_feature_term(tmp_path, fast):
    """Two epochs of four steps with feature_loss_weight=0.5, twice.  With the default logit weights (0.25, 0.75) the record, the step
    lines and the logged total are checked.  "Loss/Feat" falling from epoch 1 to epoch 2 is asserted on a run with the logit weights
    at 0, which isolates the term: with the logit terms on, their gradient (a loss near 5.3 against 0.5 x 0.88) moves the shared CLS
    features far more than the feature term does in eight steps, and the epoch mean of "Loss/Feat" moves by less than its own
    batch-to-batch scatter in either direction.  Measured on one MI355X, default logit weights, (epoch 1, epoch 2): batch 16 of 64
    samples 0.8877 -> 0.8950 eager and 0.8903 -> 0.9045 graphed; batch 64 of 256 0.8770 -> 0.8811 and 0.8766 -> 0.8826; batch 256 of
    1024 0.8814 -> 0.8797 and 0.8788 -> 0.8779; per-batch values scatter over 0.84 .. 0.98.  With the logit weights at 0, batch 16:
    0.8506 -> 0.7649 eager (batches 0.866, 0.853, 0.786, 0.898, 0.810, 0.782, 0.755, 0.713) and 0.8430 -> 0.7636 graphed."""
    kw = dict(graph=True, cache_teacher=True, device_loader=True) if fast else {}
    hist, batch = _train(tmp_path, "f", feature_loss_weight=0.5, **kw)
    print("default logit weights:", [(r["Loss/Train"], r["Loss/Feat"]) for r in hist], [l["Batch Loss/Feat"] for l in batch])
    assert len(hist) == 2 and all(set(r) == KEYS | {"Loss/Feat"} and r["steps"] == 4 for r in hist)
    assert all(math.isfinite(r["Loss/Feat"]) and math.isfinite(r["Loss/Train"]) for r in hist)
    assert len(batch) == 8 and all(set(l) == {"step", "Batch Loss/Train", "Batch Loss/Dist", "Batch Loss/CE", "Batch Loss/Feat"} for l in batch)
    for r, rows in zip(hist, (batch[:4], batch[4:])):
        assert r["Loss/Feat"] == sum(l["Batch Loss/Feat"] for l in rows) / 4
    for l in batch:   # the logged total is the three terms' weighted sum
        want = 0.25 * l["Batch Loss/Dist"] + 0.75 * l["Batch Loss/CE"] + 0.5 * l["Batch Loss/Feat"]
        assert abs(l["Batch Loss/Train"] - want) <= 1e-5 * abs(want)
    hist, batch = _train(tmp_path, "only", feature_loss_weight=0.5, soft_target_loss_weight=0.0, ce_loss_weight=0.0, **kw)
    print("the term alone:", [(r["Loss/Train"], r["Loss/Feat"]) for r in hist], [l["Batch Loss/Feat"] for l in batch])
    assert all(set(r) == KEYS | {"Loss/Feat"} and math.isfinite(r["Loss/Feat"]) for r in hist)
    assert hist[1]["Loss/Feat"] < hist[0]["Loss/Feat"], "the student's features turn towards the synthetic teacher's"
    assert all(abs(l["Batch Loss/Train"] - 0.5 * l["Batch Loss/Feat"]) <= 1e-6 for l in batch)


def test_train_distill_default_weight_is_the_run_without_the_argument(tmp_path):
    a_hist, a_batch = _train(tmp_path, "a")
    b_hist, b_batch = _train(tmp_path, "b", feature_loss_weight=0.0)
    assert all(set(r) == KEYS for r in a_hist)
    assert a_hist == b_hist, "key for key and value for value"
    assert a_batch == b_batch and all("Batch Loss/Feat" not in l for l in b_batch)


def test_train_distill_refuses_a_teacher_of_another_feature_width(tmp_path):
    from spectre_vit.distillation import SyntheticTeacher
    with pytest.raises(ValueError, match=r"\(1, 384\).*embed_dim=48.*project inside the teacher module"):
        _train(tmp_path, "w", feature_loss_weight=0.5, teacher=SyntheticTeacher(100, 384, 3).to(dev()))
