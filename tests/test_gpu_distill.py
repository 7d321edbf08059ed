"""GPU checks of the paired-view distillation (csrc/spv_distill.hip): the teacher view against the Pillow-exact restatement
tests/distill_ref.py (EQUALITY of every element: the resampling is integer arithmetic and the normalisation a table torch built), the
fused loss against the float64 oracle, GraphedDistillStep against the eager step, and harness.train_distill end to end.

Bounds of the loss: 2e-6 |ref| + 1e-7 on the three scalars and 2e-6 of the largest |dlogits|, the bounds test_cross_entropy_vs_torch_and_oracle
holds the same kind of quantity to (the oracle itself, evaluated in numpy float32, stays within 2.1e-7 / 2.8e-7 of its float64 run on
these shapes).  Where the soft term is a cancellation (teacher = student + 1e-3 noise, soft ~ 5e-7) it is bounded absolutely by 4 x the
|float32 - float64| gap of the oracle on that input, measured by the test.  Eager against graph: 1e-2 relative per step, the bound of
tests/test_harness.py's eager-vs-graph comparison.  Every comparison prints its figures before it asserts (pytest -s)."""
import json
import os

import numpy as np
import pytest
import torch

import distill_ref as D

pytestmark = pytest.mark.gpu

MEAN = (0.5071, 0.4867, 0.4408)
STD = (0.2675, 0.2565, 0.2761)


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def count():
    from spectre_vit import _native
    return _native.call("spv_path_count", _native.PATH["teacher_view"])


def image_set(n, side, chans, seed):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, size=(n, side, side, chans), dtype=np.uint8)
    yy, xx = np.mgrid[0:side, 0:side]
    for k in range(0, n, 4):    # smooth ramps: long runs of equal taps
        base = rng.uniform(0, 220, size=chans) + rng.uniform(-3, 3, size=chans) * xx[..., None] + rng.uniform(-3, 3) * yy[..., None]
        imgs[k] = np.clip(base, 0, 255).astype(np.uint8)
    for k in range(1, n, 4):    # two levels: the ringing clips at 0 and 255
        imgs[k] = (rng.integers(0, 2, size=(side, side, chans)) * 255).astype(np.uint8)
    return imgs


def reference_view(imgs, index, chans):
    sel = imgs if index is None else imgs[index]
    return torch.cat([D.teacher_view(sel[i:i + 64], None, MEAN[:chans], STD[:chans]) for i in range(0, len(sel), 64)])


def make_view(chans, **kw):
    from spectre_vit.distillation import TeacherView
    return TeacherView(MEAN[:chans], STD[:chans], **kw)


# ---------------------------------------------------------------- teacher view
@pytest.mark.parametrize("case", ["3x32x32 B=512 of 2048, shuffled with repeats", "1x28x28 B=7", "3x28x28 index=None", "3x64x64 B=5"])
def test_teacher_view_equals_the_pillow_restatement(case):
    d = dev()
    if case.startswith("3x32x32"):
        chans, imgs = 3, image_set(2048, 32, 3, 1)
        index = np.random.default_rng(5).integers(0, 2048, size=512)
        index[:4] = (7, 7, 2047, 0)
    elif case.startswith("1x28x28"):
        chans, imgs, index = 1, image_set(40, 28, 1, 2), np.array([39, 0, 3, 3, 17, 20, 1])
    elif case.startswith("3x28x28"):
        chans, imgs, index = 3, image_set(9, 28, 3, 3), None
    else:
        chans, imgs, index = 3, image_set(12, 64, 3, 4), np.array([11, 0, 5, 5, 2])
    x = torch.from_numpy(imgs).to(d)
    idx = None if index is None else torch.from_numpy(index).to(d)
    before = count()
    out = make_view(chans)(x, idx)
    out16 = make_view(chans, dtype=torch.bfloat16)(x, idx)
    assert count() == before + 2, "the census slot counts one launch per call"
    want = reference_view(imgs, index, chans)
    B = len(imgs) if index is None else len(index)
    assert out.shape == want.shape == (B, chans, 224, 224) and out.dtype == torch.float32 and out16.dtype == torch.bfloat16
    out, out16 = out.cpu(), out16.cpu()
    differing = int((out != want).sum())
    differing16 = int((out16 != want.to(torch.bfloat16)).sum())
    print(f"{case}: fp32 {differing} of {out.numel()} elements differ, bf16 {differing16}")
    assert differing == 0 and torch.equal(out, want)
    assert differing16 == 0 and torch.equal(out16, out.to(torch.bfloat16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_teacher_view_poisons_an_index_outside_the_set(dtype):
    d = dev()
    imgs = image_set(16, 32, 3, 6)
    index = np.array([3, 16, 5, -1, 15], np.int64)
    out = make_view(3, dtype=dtype)(torch.from_numpy(imgs).to(d), torch.from_numpy(index).to(d)).float().cpu()
    good = [0, 2, 4]
    want = reference_view(imgs, index[good], 3)
    if dtype == torch.bfloat16:
        want = want.to(torch.bfloat16).float()
    assert torch.isnan(out[1]).all() and torch.isnan(out[3]).all()
    assert torch.equal(out[good], want), "the neighbours of a poisoned image are right"


def test_teacher_view_refuses_unsupported_sources():
    d = dev()
    with pytest.raises(ValueError, match="teacher view"):
        make_view(3)(torch.zeros(2, 32, 28, 3, dtype=torch.uint8, device=d))       # not square
    with pytest.raises(ValueError, match="teacher view"):
        make_view(3, resize=16, crop=8)(torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device=d))   # down-scaling
    with pytest.raises(ValueError):
        make_view(1)(torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device=d))       # channels


# ---------------------------------------------------------------- fused loss
def oracle(z, t, y, T, ws, wc, dtype):
    from oracle import spectre_oracle as O
    loss, dz, soft, ce = O.distill_loss_fwd_bwd(z.astype(dtype), t.astype(dtype), y, dtype(T), dtype(ws), dtype(wc))
    return float(loss), np.asarray(dz), float(soft), float(ce)


def run_loss(z, t, y, T, ws, wc, upstream):
    from spectre_vit import hip_ops
    d = dev()
    zt = torch.from_numpy(z).to(d).requires_grad_(True)
    loss, soft, ce = hip_ops.distill_loss(zt, torch.from_numpy(t).to(d), torch.from_numpy(y).to(d), T, ws, wc)
    assert not soft.requires_grad and not ce.requires_grad and loss.requires_grad
    (loss * upstream).backward()
    return loss.item(), soft.item(), ce.item(), zt.grad.cpu().numpy()


def logits(rows, classes, seed):
    rng = np.random.default_rng(seed)
    z = (3 * rng.standard_normal((rows, classes))).astype(np.float32)
    t = (3 * rng.standard_normal((rows, classes))).astype(np.float32)
    y = rng.integers(0, classes, size=rows).astype(np.int64)
    return z, t, y


def check_scalars(what, got, ref):
    for name, g, r in zip(("loss", "soft", "ce"), got, ref):
        tol = 2e-6 * abs(r) + 1e-7
        print(f"{what}: {name} kernel {g:.9g} float64 {r:.9g} |diff| {abs(g - r):.3e} allowed {tol:.3e}")
    for name, g, r in zip(("loss", "soft", "ce"), got, ref):
        assert abs(g - r) <= 2e-6 * abs(r) + 1e-7, (what, name, g, r)


def check_grad(what, dz, ref, upstream):
    ref = ref * upstream
    err, scale = float(np.abs(dz - ref).max()), float(np.abs(ref).max())
    print(f"{what}: dlogits max |diff| {err:.3e} = {err / scale:.3e} of the largest magnitude (allowed 2e-6)")
    assert err <= 2e-6 * scale, (what, err, scale)


@pytest.mark.parametrize("shape", [(512, 100), (3, 10), (130, 1000), (64, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("consts", [(2.0, 0.25, 0.75), (4.0, 0.5, 0.5), (1.0, 0.25, 0.75)], ids=lambda c: f"T{c[0]:g}-{c[1]:g}-{c[2]:g}")
def test_distill_loss_vs_oracle(shape, consts):
    from spectre_vit.distillation import distillation_loss
    T, ws, wc = consts
    z, t, y = logits(*shape, seed=shape[0] + shape[1])
    what = f"{shape} T={T} w=({ws}, {wc})"
    upstream = 1.7
    loss, soft, ce, dz = run_loss(z, t, y, T, ws, wc, upstream)
    rl, rdz, rs, rc = oracle(z, t, y, T, ws, wc, np.float64)
    check_scalars(what, (loss, soft, ce), (rl, rs, rc))
    check_grad(what, dz, rdz, upstream)
    assert abs(loss - (ws * soft + wc * ce)) <= 1e-6 * abs(loss)
    # a second call: the same bits (fixed-order reduction, the counter re-armed itself)
    again = run_loss(z, t, y, T, ws, wc, upstream)
    assert (loss, soft, ce) == again[:3] and np.array_equal(dz, again[3])
    # the existing torch-op chain computes the same thing
    d = dev()
    old = distillation_loss(torch.from_numpy(z).to(d), torch.from_numpy(t).to(d), torch.from_numpy(y).to(d), T, ws, wc)
    check_scalars(what + " vs distillation_loss()", (loss, soft, ce), tuple(v.item() for v in old))


def test_distill_loss_where_the_soft_term_cancels():
    """teacher = student + 1e-3 noise: soft ~ 5e-7 is the difference of quantities near 1e-4.  Bound: 4 x the oracle's own float32 gap."""
    rng = np.random.default_rng(77)
    z, _, y = logits(512, 100, seed=9)
    t = (z + 1e-3 * rng.standard_normal(z.shape)).astype(np.float32)
    loss, soft, ce, dz = run_loss(z, t, y, 2.0, 0.25, 0.75, 1.0)
    rl, rdz, rs, rc = oracle(z, t, y, 2.0, 0.25, 0.75, np.float64)
    _, _, rs32, _ = oracle(z, t, y, 2.0, 0.25, 0.75, np.float32)
    tol = 4.0 * abs(rs32 - rs)
    print(f"cancellation: soft kernel {soft:.9g} float64 {rs:.9g} float32 oracle {rs32:.9g}; |kernel - f64| {abs(soft - rs):.3e} "
          f"allowed 4 x |f32 - f64| = {tol:.3e}")
    assert 1e-7 < rs < 5e-6, rs
    assert abs(soft - rs) <= tol
    for name, g, r in (("loss", loss, rl), ("ce", ce, rc)):
        assert abs(g - r) <= 2e-6 * abs(r) + 1e-7, (name, g, r)
    check_grad("cancellation", dz, rdz, 1.0)


def test_distill_loss_underflowing_teacher_probability_is_the_limit():
    """a teacher logit gap of 400 at T = 2: p_t underflows in fp32 and the reference's log(softmax) gives 0 * -inf = NaN; the kernel takes
    log p_t = t / T - lse and returns the limit.  Reference: the float64 oracle's formula with that log p_t."""
    from oracle import spectre_oracle as O
    z, t, y = logits(64, 100, seed=21)
    t[:, 0] += 400.0
    t[5, 3] -= 300.0
    T, ws, wc = 2.0, 0.25, 0.75
    with np.errstate(all="ignore"):
        pt32 = np.exp(O.log_softmax(t / np.float32(T)))
        naive32 = (pt32 * (np.log(pt32) - O.log_softmax(z / np.float32(T)))).sum()
    assert (pt32 == 0).any() and np.isnan(naive32), "the input does underflow in fp32"
    lpt = O.log_softmax(t.astype(np.float64) / T)
    rs = float((np.exp(lpt) * (lpt - O.log_softmax(z.astype(np.float64) / T))).sum() / z.shape[0] * T * T)
    rc, _ = O.cross_entropy_fwd_bwd(z.astype(np.float64), y)
    loss, soft, ce, dz = run_loss(z, t, y, T, ws, wc, 1.0)
    assert np.isfinite(loss) and np.isfinite(dz).all()
    check_scalars("underflow", (loss, soft, ce), (ws * rs + wc * float(rc), rs, float(rc)))


def test_distill_loss_bad_label_and_bad_dtypes():
    from spectre_vit import hip_ops
    z, t, y = logits(16, 10, seed=3)
    y[4] = 10
    loss, soft, ce, dz = run_loss(z, t, y, 2.0, 0.25, 0.75, 1.0)
    assert np.isnan(loss) and np.isnan(ce) and np.isfinite(soft) and np.isfinite(dz).all()
    y[4] = -1
    assert np.isnan(run_loss(z, t, y, 2.0, 0.25, 0.75, 1.0)[0])
    d = dev()
    zt, tt, yt = torch.from_numpy(z).to(d), torch.from_numpy(t).to(d), torch.from_numpy(np.abs(y)).to(d)
    for bad in ((zt.bfloat16(), tt, yt), (zt, tt.double(), yt), (zt, tt, yt.int()), (zt, tt[:, :5], yt), (zt[0], tt[0], yt[:1])):
        with pytest.raises(ValueError, match="distill_loss"):
            hip_ops.distill_loss(*bad)


def test_distillation_loss_module():
    from spectre_vit.distillation import DistillationLoss
    d = dev()
    z, t, y = logits(32, 100, seed=4)
    crit = DistillationLoss(T=3.0, soft_target_loss_weight=0.4, ce_loss_weight=0.6)
    zt = torch.from_numpy(z).to(d).requires_grad_(True)
    loss = crit(zt, torch.from_numpy(t).to(d), torch.from_numpy(y).to(d))
    loss.backward()
    rl, rdz, rs, rc = oracle(z, t, y, 3.0, 0.4, 0.6, np.float64)
    check_scalars("module", (loss.item(), crit.soft.item(), crit.ce.item()), (rl, rs, rc))
    check_grad("module", zt.grad.cpu().numpy(), rdz, 1.0)


# ---------------------------------------------------------------- the graph-replayed step
def _student(layers=2):
    from spectre_vit.models.spectre.spectre import SpectreViT
    torch.manual_seed(11)
    return SpectreViT(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=512, num_encoders=layers, num_heads=16,
                      hidden_dim=768, activation="gelu", dropout=0.0, mixer="fft").to(dev()).train()


def test_graphed_distill_step_follows_the_eager_step():
    from spectre_vit import hip_ops
    from spectre_vit.distillation import DistillationLoss
    from spectre_vit.dp import GradReducer
    from spectre_vit.graph import GraphedDistillStep
    from spectre_vit.optim import FusedAdamW
    d = dev()
    g = torch.Generator().manual_seed(3)
    steps, B = 5, 64
    imgs = [torch.randn(B, 3, 32, 32, generator=g).to(d) for _ in range(steps)]
    labels = [torch.randint(0, 100, (B,), generator=g).to(d) for _ in range(steps)]
    teach = [(3 * torch.randn(B, 100, generator=g)).to(d) for _ in range(steps)]

    m = _student()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    red = GradReducer(m)
    crit = DistillationLoss()
    eager = []
    for img, lab, tl in zip(imgs, labels, teach):
        loss = crit(m(img), tl, lab)
        red.zero_grad()
        loss.backward()
        red.finish()
        opt.step()
        eager.append((loss.item(), crit.soft.item(), crit.ce.item()))

    m = _student()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True)
    crit = DistillationLoss()
    step = GraphedDistillStep(m, opt, crit, imgs[0], labels[0], teach[0], autocast_dtype=None, warmup=1)
    try:
        graph = [(step.warm_loss.item(), step.warm_soft.item(), step.warm_ce.item())]   # the warm-up step WAS step 0
        for k in range(1, steps):
            loss = step(imgs[k], labels[k], teach[k])
            graph.append((loss.item(), step.soft.item(), step.ce.item()))
            # the replay used THIS step's teacher logits: the captured outputs are the loss of (captured logits, teach[k]) to the bit,
            # and not the loss of the previous step's teacher logits
            here = hip_ops.distill_loss(step.out.detach(), teach[k], labels[k])
            prev = hip_ops.distill_loss(step.out.detach(), teach[k - 1], labels[k])
            assert here[0].item() == loss.item() and here[1].item() == step.soft.item()
            assert prev[1].item() != step.soft.item()
        assert step.replays == steps - 1
    finally:
        step.close()
    for k, (a, b) in enumerate(zip(eager, graph)):
        print(f"step {k}: eager (loss, soft, ce) {a}  graph {b}  relative loss difference {abs(a[0] - b[0]) / abs(a[0]):.3e}")
    for a, b in zip(eager, graph):
        for u, v in zip(a, b):
            assert abs(u - v) <= 1e-2 * abs(u), (eager, graph)
    assert eager[-1][0] != eager[0][0]


# ---------------------------------------------------------------- harness.train_distill
def _run(tmp_path, tag, **kw):
    from spectre_vit.harness import train_distill
    rec = {}

    def hook(kind, step, img, label):
        if kind == "val" or step < 2:   # (a 224 x 224 batch is 38 MB: two steps of them are kept)
            rec.setdefault(kind, []).append((step, img.detach().float().cpu().clone(), label.detach().cpu().clone()))
    out = str(tmp_path / tag)
    _, hist = train_distill(out_dir=out, log=lambda r: None, batch_hook=hook, epochs=2, steps_per_epoch=8, mixer="fft", batch_size=64,
                            n_train=1024, n_val=256, **kw)
    lines = [json.loads(l) for l in open(os.path.join(out, "scalars.jsonl"))]
    return hist, rec, lines, out


@pytest.mark.parametrize("config", ["spectre_vit_mnist", "spectre_vit_cifar100"])
def test_train_distill_end_to_end(tmp_path, config):
    cfg = f"spectre_vit/configs/{config}.py"
    before = count()
    h_plain, r_plain, lines, out = _run(tmp_path, "plain", config_path=cfg, augment=False)
    assert count() == before + 16, "one teacher view launch per training step"
    h_aug, r_aug, _, _ = _run(tmp_path, "aug", config_path=cfg, augment=True)
    h_graph, _, g_lines, g_out = _run(tmp_path, "graph", config_path=cfg, augment=False, graph=True)

    for hist in (h_plain, h_aug, h_graph):
        assert len(hist) == 2 and all(r["steps"] == 8 and r["val_samples"] == 256 for r in hist)
        for r in hist:
            assert all(np.isfinite(r[k]) for k in ("Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation")), r
    print("Loss/Train per epoch: plain", [r["Loss/Train"] for r in h_plain], "augmented", [r["Loss/Train"] for r in h_aug], "graph",
          [r["Loss/Train"] for r in h_graph])
    assert h_plain[1]["Loss/Train"] < h_plain[0]["Loss/Train"] and h_graph[1]["Loss/Train"] < h_graph[0]["Loss/Train"]
    assert os.path.exists(os.path.join(out, "model_best.pt")) and os.path.exists(os.path.join(g_out, "model_best.pt"))

    # one per-batch record per step, Train = 0.25 Dist + 0.75 CE to fp32 rounding
    for ls in (lines, g_lines):
        batch = [l for l in ls if "Batch Loss/Train" in l]
        assert [l["step"] for l in batch] == list(range(16))
        for l in batch:
            want = 0.25 * l["Batch Loss/Dist"] + 0.75 * l["Batch Loss/CE"]
            assert abs(l["Batch Loss/Train"] - want) <= 1e-6 * abs(want), l
        assert len([l for l in ls if "epoch" in l]) == 2
        for e, rec in enumerate(l for l in ls if "epoch" in l):
            mean = sum(l["Batch Loss/Train"] for l in batch[8 * e:8 * e + 8]) / 8
            assert abs(rec["Loss/Train"] - mean) <= 1e-6 * abs(mean)

    # both views come from one sample: the student's un-augmented image, mapped back to 8 bits, resampled by the restatement and
    # normalised, IS the teacher's image of the same step
    C = r_plain["train"][0][1].shape[1]
    mean = torch.tensor(MEAN[:C]).view(1, -1, 1, 1)
    std = torch.tensor(STD[:C]).view(1, -1, 1, 1)
    assert [s for s, _, _ in r_plain["train"]] == [s for s, _, _ in r_plain["teacher"]] == [0, 1]
    for (_, x, lx), (_, tv, lt) in zip(r_plain["train"], r_plain["teacher"]):
        u8 = torch.round((x * std + mean) * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
        want = D.teacher_view(u8, None, MEAN[:C], STD[:C])
        assert tv.shape == (64, C, 224, 224) and torch.equal(lx, lt)
        differing = int((tv != want).sum())
        print(f"{config}: teacher view of the hook's own sample: {differing} of {tv.numel()} elements differ")
        assert differing == 0
    # the augmentation touches the student's view only
    for (_, x, lx), (_, xa, la), (_, tv, _), (_, tva, _) in zip(r_plain["train"], r_aug["train"], r_plain["teacher"], r_aug["teacher"]):
        assert torch.equal(lx, la) and not torch.equal(x, xa) and torch.equal(tv, tva)
    for (_, a, la), (_, b, lb) in zip(r_plain["val"], r_aug["val"]):
        assert torch.equal(a, b) and torch.equal(la, lb), "validation batches are untouched"

    # graph against eager: the bound of tests/test_harness.py's comparison
    for a, b in zip(h_plain, h_graph):
        print(f"{config}: eager {a['Loss/Train']:.6f} graph {b['Loss/Train']:.6f}")
        assert abs(a["Loss/Train"] - b["Loss/Train"]) < 1e-2 * abs(a["Loss/Train"]), (a, b)
