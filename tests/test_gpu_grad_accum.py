"""On-device gradient accumulation (FusedAdamW(accumulate_steps=k)) on the GPU: the accumulate kernel against the numpy restatement
(tests/accum_ref.py) bit for bit, nothing moving inside a window, the trajectory against torch.optim.AdamW fed the window means,
k = 1 against the plain control path bit for bit, a dropped window, and the graph-replayed steps, the loader-fed step and the harness
running k replays per optimizer step.

The optimizer tests walk the tensor list of tests/test_gpu_step_control.py -- a scalar, sub-vector tails, an exact 2048-element
chunk, chunk + 1, an unaligned tail, a multi-chunk tensor -- plus one tensor (parameter AND gradient) whose storage is offset by one
element, so that its gradient takes the scalar branch while its accumulator slot is aligned."""
import math
import warnings

import numpy as np
import pytest
import torch

import accum_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (5,), (2048,), (2049,), (4095,), (65, 512)]
OFFSET_N = 1029   # the tensor behind a one-element storage offset
SIZES = [int(np.prod(s)) for s in SHAPES] + [OFFSET_N]


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


def snapshot(opt, ps):
    st = opt.state
    snap = dict(param=[p.detach().clone() for p in ps], exp_avg=[st[p]["exp_avg"].clone() for p in ps],
                exp_avg_sq=[st[p]["exp_avg_sq"].clone() for p in ps], step=[st[p]["step"].clone() for p in ps])
    if opt.ema_enabled:
        snap["ema"] = [st[p]["ema"].clone() for p in ps]
    return snap


def changed(a, b):
    """kinds of state with at least one tensor that differs bit for bit"""
    return {kind for kind in a if any(not torch.equal(x, y) for x, y in zip(a[kind], b[kind]))}


def bits(t):
    return t.detach().cpu().contiguous().view(-1).numpy().view(np.uint32)


def test_accumulators_match_the_restatement_bit_for_bit():
    """k = 3, two windows, gradients set by hand, the accumulators poisoned with NaN beforehand: after every micro-step each
    accumulator is the float32 sequential sum bit for bit (the first micro-step of a window assigns, so the NaN is gone and window 2
    starts from its own first gradient), the integer fields of the control block are the restatement's, and at a boundary
    last_grad_norm() is the fp64 norm of acc / k to 1e-5 relative"""
    from spectre_vit.optim import FusedAdamW
    k = 3
    ps = make_params(20)
    opt = FusedAdamW(ps, lr=1e-3, weight_decay=0.01, capturable=True, max_grad_norm=1.0, accumulate_steps=k)
    accs = opt.accumulated_grads()
    assert [a.shape for a in accs] == [p.shape for p in ps] and all(a.data_ptr() % 16 == 0 and a.dtype == torch.float32 for a in accs)
    for a in accs:
        a.fill_(float("nan"))
    ref = R.AccumRef(k, SIZES, max_grad_norm=1.0)
    gen = torch.Generator().manual_seed(21)
    for m in range(2 * k):
        grads = make_grads(gen, 0.5 + m)
        set_grads(ps, grads)
        opt.step()
        want = ref.micro_step([g.cpu().numpy() for g in grads])
        got = opt._read_ctl()
        for i, (a, w) in enumerate(zip(opt.accumulated_grads(), ref.acc)):
            assert a.data_ptr() == accs[i].data_ptr()
            assert np.array_equal(bits(a), w.view(np.uint32)), (m, i, float((a.cpu() - torch.from_numpy(w).view(a.shape)).abs().max()))
        for f in ("apply", "sched_step", "skipped", "micro"):
            assert got[f] == want[f], (m, f, got, want)
        assert opt.micro_step() == (m + 1) % k
        for p, g in zip(ps, grads):   # p.grad holds the last micro-batch's gradient, untouched
            assert torch.equal(p.grad, g)
        if m % k == k - 1:
            norm = math.sqrt(sum(float((a.double() ** 2).sum()) for a in opt.accumulated_grads())) / k
            rel = abs(opt.last_grad_norm() - norm) / norm
            print(f"micro-step {m}: grad norm {opt.last_grad_norm()!r}, float64 of acc / k {norm!r}, rel {rel:.2e}; restatement {float(want['grad_norm'])!r}")
            assert rel <= 1e-5, (m, opt.last_grad_norm(), norm)
            assert abs(got["clip_coef"] - float(want["clip_coef"])) <= 1e-5 * float(want["clip_coef"])
    assert float(opt.state[ps[0]]["step"]) == 2.0 and opt.schedule_step() == 2


def test_nothing_moves_inside_a_window():
    """k = 3 with ema_decay=0.9: after micro-steps 1 and 2 the parameters, both moments, the Adam count, the average and the
    schedule count are bit-equal to before; after micro-step 3 they moved.  Twice: the second window starts from non-zero moments."""
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    ps = make_params(22)
    opt = FusedAdamW(ps, lr=1e-3, weight_decay=0.01, capturable=True, schedule=CosineSchedule(8, 3, 1e-5), max_grad_norm=1.0,
                     ema_decay=0.9, accumulate_steps=3)
    gen = torch.Generator().manual_seed(23)
    set_grads(ps, make_grads(gen, 1.0))
    opt.step()   # creates the state; a micro-step inside window 1
    for window in range(2):
        for m in range(1 if window == 0 else 0, 3):
            before, t, lr, norm = snapshot(opt, ps), opt.schedule_step(), opt.last_lr(), opt.last_grad_norm()
            set_grads(ps, make_grads(gen, 1.0))
            opt.step()
            moved = changed(before, snapshot(opt, ps))
            if m < 2:
                assert not moved, (window, m, moved)
                assert (opt.schedule_step(), opt.last_lr(), opt.last_grad_norm()) == (t, lr, norm), (window, m)
            else:
                assert moved == {"param", "exp_avg", "exp_avg_sq", "step", "ema"}, (window, m, moved)
                assert opt.schedule_step() == t + 1 == window + 1
    assert float(opt.state[ps[0]]["step"]) == 2.0 and opt.skipped_steps() == 0


def test_trajectory_matches_torch_adamw_on_the_window_means():
    """k = 4, two groups (1e-3, 3e-4), CosineSchedule(8, 3, 1e-5), max_grad_norm=1, 8 windows against torch.optim.AdamW +
    clip_grad_norm_ + SequentialLR fed the fp64 mean of each window's gradients rounded to fp32; window 5's mean norm is below 1 (the
    no-clip branch).  The bounds of test_trajectory_matches_torch_adamw_with_clip_and_schedule."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    k, W, T, eta_min, bases = 4, 3, 8, 1e-5, (1e-3, 3e-4)
    a = make_params(24)
    b = [p.detach().clone().requires_grad_(True) for p in a]
    sched = CosineSchedule(T, warmup_steps=W, eta_min=eta_min)
    oa = FusedAdamW([dict(params=a[:4], lr=bases[0]), dict(params=a[4:], lr=bases[1])], weight_decay=0.01, capturable=True,
                    schedule=sched, max_grad_norm=1.0, accumulate_steps=k)
    ob = torch.optim.AdamW([dict(params=b[:4], lr=bases[0]), dict(params=b[4:], lr=bases[1])], weight_decay=0.01)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sb = SequentialLR(ob, [LinearLR(ob, start_factor=1.0 / (W + 1), total_iters=W),
                               CosineAnnealingLR(ob, T_max=T - W, eta_min=eta_min)], milestones=[W])
    gen = torch.Generator().manual_seed(25)
    worst = 0.0
    for window in range(8):
        mean = [torch.zeros(n, dtype=torch.float64, device="cuda") for n in SIZES]
        for m in range(k):
            grads = make_grads(gen, 1e-5 if window == 5 else 0.1 + window)
            for s, g in zip(mean, grads):
                s += g.double().view(-1)
            set_grads(a, grads)
            oa.step()
            assert oa.schedule_step() == window + (1 if m == k - 1 else 0)
        mean = [s / k for s in mean]
        want_norm = math.sqrt(sum(float((s ** 2).sum()) for s in mean))
        assert (want_norm < 1.0) == (window == 5)
        for p, s in zip(b, mean):
            p.grad = s.float().view(p.shape)
        torch.nn.utils.clip_grad_norm_(b, 1.0)
        ob.step()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sb.step()
        for i, (x, y) in enumerate(zip(a, b)):
            err = (x - y).abs().max().item()
            worst = max(worst, err)
            assert torch.allclose(x, y, rtol=2e-6, atol=2e-7), (window, i, err)
        for got, base in zip(oa.last_lr(), bases):
            want = np.float32(sched.lr_at(window, base))
            assert abs(np.float32(got) - want) <= np.spacing(want), (window, base, got, float(want))
        got_norm = oa.last_grad_norm()
        print(f"window {window}: mean-gradient norm {got_norm!r}, float64 {want_norm!r}, rel {abs(got_norm - want_norm) / want_norm:.2e}, "
              f"lr {oa.last_lr()}, worst |weight difference| so far {worst:.3e}")
        assert abs(got_norm - want_norm) <= 1e-5 * want_norm, (window, got_norm, want_norm)
    assert oa.schedule_step() == 8 and oa.skipped_steps() == 0 and float(oa.state[a[0]]["step"]) == 8.0


def test_k1_is_the_plain_control_path_bit_for_bit():
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    cfg = dict(lr=1e-3, weight_decay=0.01, capturable=True, max_grad_norm=1.0, skip_nonfinite=True, schedule=CosineSchedule(8, 3, 1e-5))
    a = make_params(26)
    b = clone_params(a)
    oa = FusedAdamW(a, accumulate_steps=1, **cfg)
    ob = FusedAdamW(b, **cfg)
    gen = torch.Generator().manual_seed(27)
    for step in range(5):
        grads = make_grads(gen, 1e-5 if step == 3 else 0.1 + step)   # step 3: the no-clip branch
        set_grads(a, grads)
        set_grads(b, grads)
        oa.step()
        ob.step()
        assert oa.control_block_bytes() == ob.control_block_bytes(), (step, oa._read_ctl(), ob._read_ctl())
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (i, (x - y).abs().max().item())
        for kind in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(oa.state[x][kind], ob.state[y][kind]), (i, kind)
    assert oa.schedule_step() == 5 and oa.micro_step() == 0 and len(oa.control_block_bytes()) == 64


def test_a_nonfinite_micro_step_drops_its_window_and_the_next_one_starts_clean():
    """k = 2, an inf in the FIRST micro-step of window 2.  skip_nonfinite: window 2 changes nothing, is counted, and the schedule
    ticks; window 3 applies and every weight stays finite -- its first micro-step assigned the accumulators, or the inf would still
    be in them.  Without skip_nonfinite the inf reaches the weights, as it does without accumulation."""
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    for skip in (True, False):
        ps = make_params(28)
        opt = FusedAdamW(ps, lr=1e-3, weight_decay=0.01, capturable=True, schedule=CosineSchedule(8, 1), max_grad_norm=1.0,
                         skip_nonfinite=skip, accumulate_steps=2)
        gen = torch.Generator().manual_seed(29)
        for m in range(2):   # window 1
            set_grads(ps, make_grads(gen, 1.0))
            opt.step()
        assert (opt.schedule_step(), opt.skipped_steps(), float(opt.state[ps[0]]["step"])) == (1, 0, 1.0)
        before = snapshot(opt, ps)
        i2049 = SHAPES.index((2049,))
        for m in range(2):   # window 2
            grads = make_grads(gen, 1.0)
            if m == 0:
                grads[i2049][2048] = float("inf")   # the first slot of the tensor's short chunk
            set_grads(ps, grads)
            opt.step()
        assert opt.schedule_step() == 2 and opt.micro_step() == 0
        if not skip:
            assert opt.skipped_steps() == 0 and torch.isnan(ps[i2049].detach()[2048]).item()
            continue
        assert not changed(before, snapshot(opt, ps)) and opt.skipped_steps() == 1
        assert torch.isinf(opt.accumulated_grads()[i2049][2048]).item()
        for m in range(2):   # window 3
            set_grads(ps, make_grads(gen, 1.0))
            opt.step()
        assert changed(before, snapshot(opt, ps)) == {"param", "exp_avg", "exp_avg_sq", "step"}
        assert all(torch.isfinite(p).all().item() for p in ps) and all(torch.isfinite(x).all().item() for x in opt.accumulated_grads())
        assert (opt.schedule_step(), opt.skipped_steps(), float(opt.state[ps[0]]["step"])) == (3, 1, 2.0)
        assert opt.last_lr() == [float(np.float32(CosineSchedule(8, 1).lr_at(2, 1e-3)))]


def test_graph_replay_applies_every_second_replay():
    """the 1-layer fft model and 16-image batch of test_graph_replay_follows_schedule_and_skips_a_nan_batch with k = 2 and warmup=2
    (one whole window, t = 0), then six replays: odd replays leave every parameter bit-equal, even ones move them, a NaN pixel in
    replay 3 drops window 2 (replay 4 moves nothing either), last_lr() after each boundary is the schedule's float32 value, and the
    losses follow an eager loop over the same optimizer configuration.  Through GraphedTrainStep, then single-process GraphedDPStep."""
    from spectre_vit.graph import GraphedDPStep, GraphedTrainStep
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    cfg = dict(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=512, num_encoders=1, num_heads=16, hidden_dim=768,
               activation="gelu", dropout=0.0, mixer="fft")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    img = torch.randn(16, 3, 32, 32, generator=g).to(dev)
    labels = torch.randint(0, 100, (16,), generator=g).to(dev)
    img2 = torch.randn(16, 3, 32, 32, generator=g).to(dev)   # a second batch: the two micro-batches of a window differ
    img_bad = img.clone()
    img_bad[0, 0, 0, 0] = float("nan")
    crit = torch.nn.CrossEntropyLoss()
    sched = CosineSchedule(6, 2)
    want_lr = [float(np.float32(sched.lr_at(t, 1e-3))) for t in range(4)]
    batches = [img, img2, img_bad, img2, img, img2]   # the six replays (after the warm-up window on img, img)

    def make():
        torch.manual_seed(11)
        m = SpectreViT(**cfg).to(dev).train()
        return m, FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, schedule=sched, max_grad_norm=1.0,
                             skip_nonfinite=True, accumulate_steps=2)

    m1, o1 = make()
    eager_losses = []
    for x in [img, img] + batches:
        o1.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m1(x)
        loss = crit(out, labels)
        loss.backward()
        o1.step()
        eager_losses.append(loss.item())
    assert o1.skipped_steps() == 1 and o1.schedule_step() == 4 and o1.micro_step() == 0

    for cls in (GraphedTrainStep, GraphedDPStep):
        m2, o2 = make()
        step = cls(m2, o2, crit, img, labels, warmup=2)
        try:
            assert o2.schedule_step() == 1 and o2.micro_step() == 0 and o2.last_lr() == [want_lr[0]]   # the warm-up was window 1
            losses = []
            for r, x in enumerate(batches, start=1):
                before = [p.detach().clone() for p in m2.parameters()]
                losses.append(step(x, labels).item())
                moved = any(not torch.equal(p, q) for p, q in zip(m2.parameters(), before))
                assert o2.micro_step() == r % 2 and o2.schedule_step() == 1 + r // 2, (cls.__name__, r, o2.micro_step(), o2.schedule_step())
                assert moved == (r in (2, 6)), (cls.__name__, r, moved)
                assert o2.skipped_steps() == (1 if r >= 4 else 0), (cls.__name__, r, o2.skipped_steps())
                if r % 2 == 0:
                    assert o2.last_lr() == [want_lr[r // 2]], (cls.__name__, r, o2.last_lr(), want_lr)
            print(cls.__name__, "losses", losses, "eager", eager_losses[2:])
            for r in (1, 2, 4, 5, 6):
                want = eager_losses[r + 1]
                assert math.isfinite(losses[r - 1]) and abs(losses[r - 1] - want) <= 5e-4 * abs(want), (cls.__name__, r, losses, eager_losses)
            assert float(o2.state[next(iter(m2.parameters()))]["step"]) == 3.0   # the warm-up window and windows 1 and 3
        finally:
            step.close()


def test_loader_fed_step_accumulates():
    """GraphedTrainStep(loader=ResidentLoader(...)) over 64 samples at batch size 16 with k = 2 and a warm-up of one window: four
    replays are two optimizer steps and four loader steps; the odd replays move no parameter"""
    from spectre_vit.data import ResidentLoader
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    cfg = dict(img_size=8, patch_size=4, in_channels=3, num_classes=10, embed_dim=16, num_encoders=2, num_heads=4, hidden_dim=32,
               dropout=0.0, activation="gelu", mixer="fft")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.integers(0, 256, size=(64, 8, 8, 3), dtype=np.uint8)).to(dev)
    y = torch.from_numpy(rng.integers(0, 10, size=64).astype(np.uint8)).to(dev)
    torch.manual_seed(21)
    model = SpectreViT(**cfg).to(dev).train()
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True, accumulate_steps=2)
    loader = ResidentLoader(x, y, 16, seed=42)
    step = GraphedTrainStep(model, opt, CrossEntropyLoss(), None, None, autocast_dtype=None, warmup=2, loader=loader)
    try:
        assert (opt.schedule_step(), opt.micro_step(), loader.step) == (1, 0, 2)
        for r in range(1, 5):
            before = [p.detach().clone() for p in model.parameters()]
            loss = step()
            moved = any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
            assert math.isfinite(loss.item()) and moved == (r % 2 == 0), (r, moved)
        assert opt.schedule_step() == 3 and opt.micro_step() == 0, "four replays are two optimizer steps"
        assert float(opt.state[next(iter(model.parameters()))]["step"]) == 3.0
        assert loader.step == 6 == loader.device_step(), "two warm-up steps, then four replays consumed four loader steps"
    finally:
        step.close()


def test_harness_accumulates(tmp_path):
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.harness import train
    from spectre_vit.optim import CosineSchedule
    cfg = "spectre_vit/configs/spectre_vit_cifar100.py"
    lr = getattr(parse_config(cfg), "learning_rate", 1e-3)
    kw = dict(mixer="fft", epochs=2, steps_per_epoch=3, batch_size=16, n_train=64, n_val=32, graph=True, log=lambda r: None)
    _, h = train(cfg, out_dir=str(tmp_path / "a"), lr_schedule="cosine", accumulate_steps=2, **kw)
    sched = CosineSchedule(3)   # T = (epochs * steps per epoch) // k
    assert [rec["OptimizerSteps"] for rec in h] == [1, 3]   # the window that spans the epoch boundary closes in epoch 2
    for rec, t in zip(h, (0, 2)):   # the last boundary before the epoch's end
        print(rec["LR"], float(np.float32(sched.lr_at(t, lr))), rec["GradNorm"])
        assert rec["AccumulateSteps"] == 2 and rec["steps"] == 3
        assert rec["LR"] == float(np.float32(sched.lr_at(t, lr))), (rec, t)
        assert rec["SkippedSteps"] == 0 and math.isfinite(rec["GradNorm"]) and rec["GradNorm"] > 0.0
        assert math.isfinite(rec["Loss/Train"])
    _, h0 = train(cfg, out_dir=str(tmp_path / "p"), **kw)
    for rec in h0:
        assert set(rec) == {"epoch", "Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation", "steps", "val_samples"}
    assert set(h[0]) == set(h0[0]) | {"LR", "GradNorm", "SkippedSteps", "AccumulateSteps", "OptimizerSteps"}
