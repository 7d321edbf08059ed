"""On-device step control of FusedAdamW (schedule / max_grad_norm / skip_nonfinite) on the GPU: the control path's update against the
shipped kernel (bit for bit) and against torch.optim.AdamW + clip_grad_norm_ + SequentialLR, the skipped step, determinism, and
the three graph-replayed steps and the harness carrying the control launches.

Every optimizer test walks one tensor list chosen to hit each path of the chunk walk: a scalar, sub-vector tails, an exact
2048-element chunk, chunk + 1, an unaligned tail, a multi-chunk tensor, and one tensor (parameter AND gradient) whose storage is
offset by one element, so that its base is not 16-byte aligned (the scalar-load branch)."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (5,), (2048,), (2049,), (4095,), (65, 512)]
OFFSET_N = 1029   # the tensor behind a one-element storage offset


def offset_view(values):
    """a contiguous tensor holding `values` whose data pointer is 4 bytes past a 16-byte boundary"""
    buf = torch.empty(values.numel() + 1, device=values.device, dtype=values.dtype)
    v = buf[1:].view(values.shape)
    v.copy_(values)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def make_params(seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g).to(dev).requires_grad_(True) for s in SHAPES]
    ps.append(offset_view(torch.randn(OFFSET_N, generator=g).to(dev)).requires_grad_(True))
    return ps


def clone_params(ps):
    return [(offset_view(p.detach()) if p.data_ptr() % 16 else p.detach().clone()).requires_grad_(True) for p in ps]


def make_grads(gen, scale, dev="cuda"):
    return [torch.randn(s, generator=gen).to(dev) * scale for s in SHAPES + [(OFFSET_N,)]]


def set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = offset_view(g) if p.data_ptr() % 16 else g.clone()


def norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


def snapshot(opt, ps):
    st = opt.state
    return ([p.detach().clone() for p in ps], [st[p]["exp_avg"].clone() for p in ps], [st[p]["exp_avg_sq"].clone() for p in ps],
            [st[p]["step"].clone() for p in ps])


def assert_unchanged(opt, ps, snap):
    now = snapshot(opt, ps)
    for kind, a, b in zip(("param", "exp_avg", "exp_avg_sq", "step"), snap, now):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (kind, i)


def clip64(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ on float64 copies of the gradients, rounded back to fp32: clip_grad_norm_ on the fp32
    tensors squares in fp32 and overflows at 1e25, which is the failure the fp64 sum of squares exists to avoid"""
    d = [torch.zeros_like(g, dtype=torch.float64).requires_grad_(True) for g in grads]
    for t, g in zip(d, grads):
        t.grad = g.double()
    torch.nn.utils.clip_grad_norm_(d, max_norm)
    return [t.grad.float() for t in d]


def test_noop_controls_match_the_shipped_kernel_bit_for_bit():
    """max_grad_norm=1e30 (never clips: coefficient exactly 1) + skip_nonfinite on finite gradients == FusedAdamW(capturable=True):
    the control path runs the shipped kernel's update arithmetic"""
    from spectre_vit.optim import FusedAdamW
    a = make_params(0)
    b = clone_params(a)
    oa = FusedAdamW(a, lr=1e-3, weight_decay=0.01, capturable=True, max_grad_norm=1e30, skip_nonfinite=True)
    ob = FusedAdamW(b, lr=1e-3, weight_decay=0.01, capturable=True)
    gen = torch.Generator().manual_seed(1)
    for step in range(5):
        grads = make_grads(gen, 0.1 + step)
        set_grads(a, grads)
        set_grads(b, grads)
        oa.step()
        ob.step()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (i, (x - y).abs().max().item())
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[x][k], ob.state[y][k]), (i, k)
        assert float(oa.state[x]["step"]) == 5.0 and float(ob.state[y]["step"]) == 5.0
    assert oa.skipped_steps() == 0 and oa.schedule_step() == 5
    assert oa.last_lr() == [float(np.float32(1e-3))]


def test_trajectory_matches_torch_adamw_with_clip_and_schedule():
    """two groups (1e-3, 3e-4), CosineSchedule(8, 3, 1e-5), max_grad_norm=1 against torch.optim.AdamW + clip_grad_norm_ +
    SequentialLR([LinearLR, CosineAnnealingLR]); step 5's gradient norm is below 1 (the no-clip branch)"""
    import warnings
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    W, T, eta_min, bases = 3, 8, 1e-5, (1e-3, 3e-4)
    a = make_params(2)
    b = [p.detach().clone().requires_grad_(True) for p in a]
    sched = CosineSchedule(T, warmup_steps=W, eta_min=eta_min)
    oa = FusedAdamW([dict(params=a[:4], lr=bases[0]), dict(params=a[4:], lr=bases[1])], weight_decay=0.01, capturable=True,
                    schedule=sched, max_grad_norm=1.0)
    ob = torch.optim.AdamW([dict(params=b[:4], lr=bases[0]), dict(params=b[4:], lr=bases[1])], weight_decay=0.01)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sb = SequentialLR(ob, [LinearLR(ob, start_factor=1.0 / (W + 1), total_iters=W),
                               CosineAnnealingLR(ob, T_max=T - W, eta_min=eta_min)], milestones=[W])
    gen = torch.Generator().manual_seed(3)
    for step in range(8):
        grads = make_grads(gen, 1e-5 if step == 5 else 0.1 + step)
        want_norm = norm64(grads)
        assert (want_norm < 1.0) == (step == 5)
        set_grads(a, grads)
        for p, g in zip(b, grads):
            p.grad = g.clone()
        oa.step()
        torch.nn.utils.clip_grad_norm_(b, 1.0)
        ob.step()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sb.step()
        for i, (x, y) in enumerate(zip(a, b)):
            err = (x - y).abs().max().item()
            assert torch.allclose(x, y, rtol=2e-6, atol=2e-7), (step, i, err)
        for got, base in zip(oa.last_lr(), bases):
            want = np.float32(sched.lr_at(step, base))
            print(f"step {step} base {base}: last_lr {got!r} float32(lr_at) {float(want)!r}")
            assert abs(np.float32(got) - want) <= np.spacing(want), (step, base, got, float(want))
        got_norm = oa.last_grad_norm()
        print(f"step {step}: grad norm {got_norm!r}, float64 {want_norm!r}, rel {abs(got_norm - want_norm) / want_norm:.2e}")
        assert abs(got_norm - want_norm) <= 1e-5 * want_norm, (step, got_norm, want_norm)
    for i, g in enumerate(grads):   # p.grad is not rewritten by the clip
        assert torch.equal(a[i].grad, g), i
    assert oa.schedule_step() == 8 and oa.skipped_steps() == 0


def test_nonfinite_steps_are_skipped_and_finite_overflowing_ones_are_not():
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    cfg = dict(lr=1e-3, weight_decay=0.01, capturable=True, schedule=CosineSchedule(20, warmup_steps=2, eta_min=1e-5),
               max_grad_norm=1.0, skip_nonfinite=True)
    a = make_params(4)
    oa = FusedAdamW(a, **cfg)
    gen = torch.Generator().manual_seed(5)
    for step in range(2):   # two clean steps: non-zero moments
        set_grads(a, make_grads(gen, 0.1 + step))
        oa.step()
    before = copy.deepcopy(oa.state_dict())
    twin_params = clone_params(a)
    assert before["step_control"] == dict(schedule_step=2, skipped_steps=0)
    i2049 = SHAPES.index((2049,))
    bad_steps = [(0, 0, float("nan")),            # element 0 of the first tensor
                 (i2049, 2047, float("inf")),      # the last slot of a full chunk
                 (i2049, 2048, float("nan")),      # the first slot of the tensor's short chunk
                 (0, 0, float("-inf")),            # the scalar tensor
                 (len(SHAPES), OFFSET_N - 1, float("nan"))]   # the last element of the unaligned tensor (scalar-load branch)
    for k, (ti, idx, value) in enumerate(bad_steps):
        grads = make_grads(gen, 1.0)
        grads[ti].view(-1)[idx] = value
        set_grads(a, grads)
        snap = snapshot(oa, a)
        oa.step()
        assert_unchanged(oa, a, snap)
        assert oa.skipped_steps() == k + 1 and oa.schedule_step() == 3 + k, (k, oa.skipped_steps(), oa.schedule_step())
        assert float(oa.state[a[0]]["step"]) == 2.0
    # a clean step afterwards == the same step on a twin that never saw the bad ones but whose schedule count advanced equally
    before["step_control"]["schedule_step"] += len(bad_steps)
    before["step_control"]["skipped_steps"] += len(bad_steps)
    ot = FusedAdamW(twin_params, **cfg)
    ot.load_state_dict(before)
    grads = make_grads(gen, 1.0)
    set_grads(a, grads)
    set_grads(twin_params, grads)
    oa.step()
    ot.step()
    for i, (x, y) in enumerate(zip(a, twin_params)):
        assert torch.equal(x, y), (i, (x - y).abs().max().item())
        assert torch.equal(oa.state[x]["exp_avg_sq"], ot.state[y]["exp_avg_sq"]), i
        assert float(oa.state[x]["step"]) == float(ot.state[y]["step"]) == 3.0
    assert oa.last_lr() == ot.last_lr() and oa.control_block_bytes() == ot.control_block_bytes()
    assert oa.schedule_step() == 3 + len(bad_steps) and oa.skipped_steps() == len(bad_steps)

    # a finite gradient of 1e25 in every element (its fp32 square overflows) is NOT skipped; the clipped update follows torch's
    c = make_params(6)
    d = [p.detach().clone().requires_grad_(True) for p in c]
    oc = FusedAdamW(c, lr=1e-3, weight_decay=0.01, capturable=True, max_grad_norm=1.0, skip_nonfinite=True)
    od = torch.optim.AdamW(d, lr=1e-3, weight_decay=0.01)
    for step, grads in enumerate([make_grads(gen, 1.0), [torch.full_like(g, 1e25) for g in make_grads(gen, 1.0)]]):
        set_grads(c, grads)
        for p, g in zip(d, clip64(grads, 1.0)):
            p.grad = g
        oc.step()
        od.step()
        for i, (x, y) in enumerate(zip(c, d)):
            assert torch.allclose(x, y, rtol=2e-6, atol=2e-7), (step, i, (x - y).abs().max().item())
        want = norm64(grads)
        assert abs(oc.last_grad_norm() - want) <= 1e-5 * want, (step, oc.last_grad_norm(), want)
    assert oc.skipped_steps() == 0 and float(oc.state[c[0]]["step"]) == 2.0


def test_control_block_is_deterministic():
    """the same gradients through two fresh optimizers: the norm bit for bit, the control blocks equal as raw bytes"""
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    blocks, norms, weights = [], [], []
    for _ in range(2):
        a = make_params(7)
        o = FusedAdamW(a, lr=1e-3, capturable=True, schedule=CosineSchedule(8, 3, 1e-5), max_grad_norm=1.0, skip_nonfinite=True)
        gen = torch.Generator().manual_seed(8)
        seq_b, seq_n = [], []
        for step in range(3):
            set_grads(a, make_grads(gen, 0.1 + step))
            o.step()
            seq_b.append(o.control_block_bytes())
            seq_n.append(np.float32(o.last_grad_norm()).tobytes())
        blocks.append(seq_b)
        norms.append(seq_n)
        weights.append([p.detach().clone() for p in a])
    assert norms[0] == norms[1]
    assert blocks[0] == blocks[1] and len(blocks[0][0]) == 64
    assert all(torch.equal(x, y) for x, y in zip(*weights))


def test_graph_replay_follows_schedule_and_skips_a_nan_batch():
    """GraphedTrainStep (warm-up step = t 0, then four replays, the third on a batch with one NaN pixel) against an eager loop over the
    same optimizer configuration; the same sequence through GraphedDPStep in a single process (collective skipped), whose optimizer
    graph (graph B) must hold the control launches"""
    from spectre_vit.graph import GraphedDPStep, GraphedTrainStep
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    cfg = dict(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=512, num_encoders=1, num_heads=16, hidden_dim=768,
               activation="gelu", dropout=0.0, mixer="fft")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    img = torch.randn(16, 3, 32, 32, generator=g).to(dev)
    labels = torch.randint(0, 100, (16,), generator=g).to(dev)
    img_bad = img.clone()
    img_bad[0, 0, 0, 0] = float("nan")
    crit = torch.nn.CrossEntropyLoss()
    sched = CosineSchedule(6, 2)
    want_lr = [float(np.float32(sched.lr_at(t, 1e-3))) for t in range(5)]
    batches = [img, img, img_bad, img]   # the four replays (after the warm-up step on img)

    def make():
        torch.manual_seed(11)
        m = SpectreViT(**cfg).to(dev).train()
        return m, FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, schedule=sched, max_grad_norm=1.0,
                             skip_nonfinite=True)

    m1, o1 = make()
    eager_losses = []
    for x in [img] + batches:
        o1.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m1(x)
        loss = crit(out, labels)
        loss.backward()
        o1.step()
        eager_losses.append(loss.item())
    assert o1.skipped_steps() == 1 and o1.schedule_step() == 5

    for cls in (GraphedTrainStep, GraphedDPStep):
        m2, o2 = make()
        step = cls(m2, o2, crit, img, labels, warmup=1)
        try:
            assert o2.schedule_step() == 1 and o2.last_lr() == [want_lr[0]]   # the warm-up step consumed t = 0
            losses, lrs = [], []
            for r, x in enumerate(batches):
                before = [p.detach().clone() for p in m2.parameters()]
                losses.append(step(x, labels).item())
                lrs.append(o2.last_lr()[0])
                moved = any(not torch.equal(p, q) for p, q in zip(m2.parameters(), before))
                assert o2.schedule_step() == r + 2, (cls.__name__, r, o2.schedule_step())
                if r == 2:   # the NaN batch: every parameter as before, one skipped step
                    assert not moved and o2.skipped_steps() == 1, (cls.__name__, moved, o2.skipped_steps())
                else:
                    assert moved and math.isfinite(losses[-1]), (cls.__name__, r, losses)
                    assert o2.skipped_steps() == (1 if r == 3 else 0)
            print(cls.__name__, "lr", lrs, "want", want_lr[1:], "losses", losses, "eager", eager_losses[1:])
            assert lrs == want_lr[1:], (cls.__name__, lrs, want_lr[1:])
            for r in (0, 1, 3):
                assert abs(losses[r] - eager_losses[r + 1]) <= 5e-4 * abs(eager_losses[r + 1]), (cls.__name__, r, losses, eager_losses)
            assert float(o2.state[next(iter(m2.parameters()))]["step"]) == 4.0   # warm-up + three applied replays
            if cls is GraphedDPStep:
                # graph A (forward + backward) holds no control launch, graph B (the optimizer) holds them all
                before = [p.detach().clone() for p in m2.parameters()]
                step.graph.replay()
                assert o2.schedule_step() == 5 and all(torch.equal(p, q) for p, q in zip(m2.parameters(), before))
                step.graph_opt.replay()
                assert o2.schedule_step() == 6 and any(not torch.equal(p, q) for p, q in zip(m2.parameters(), before))
        finally:
            step.close()


def test_harness_records_step_control(tmp_path):
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.harness import train
    from spectre_vit.optim import CosineSchedule
    cfg = "spectre_vit/configs/spectre_vit_cifar100.py"
    lr = getattr(parse_config(cfg), "learning_rate", 1e-3)
    kw = dict(mixer="fft", epochs=2, steps_per_epoch=3, batch_size=16, n_train=64, n_val=32, graph=True, log=lambda r: None)
    _, h = train(cfg, out_dir=str(tmp_path / "c"), lr_schedule="cosine", warmup_steps=1, clip_grad_norm=1.0, skip_nonfinite=True, **kw)
    sched = CosineSchedule(6, warmup_steps=1)   # T = steps per epoch * epochs
    assert len(h) == 2
    for rec, t in zip(h, (2, 5)):   # read after the third and after the sixth step
        assert {"LR", "GradNorm", "SkippedSteps"} <= set(rec)
        print(rec["LR"], float(np.float32(sched.lr_at(t, lr))), rec["GradNorm"])
        assert rec["LR"] == float(np.float32(sched.lr_at(t, lr))), (rec, t)
        assert rec["SkippedSteps"] == 0 and math.isfinite(rec["GradNorm"]) and rec["GradNorm"] > 0.0
    _, h0 = train(cfg, out_dir=str(tmp_path / "p"), **kw)
    for rec in h0:
        assert set(rec) == {"epoch", "Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation", "steps", "val_samples"}
