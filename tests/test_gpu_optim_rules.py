"""FusedSGD and FusedAdam on the GPU: SGD against the float32 restatement bit for bit (tests/optim_rules_ref.py) on both walks, Adam
against FusedAdamW bit for bit without decay and against float64 torch.optim.Adam with it, the control path of both rules (schedule
and clip trajectory, the dropped step, accumulation windows, k = 1), the weights' average, six graph replays, and the harness.

Every optimizer test walks the tensor list of tests/optim_rules_ref.py: a scalar, sub-vector tails, an exact 2048-element chunk,
chunk + 1, an unaligned tail, a multi-chunk tensor, and one tensor (parameter AND gradient) whose storage is offset by one element,
so that its base is not 16-byte aligned (the scalar walk)."""
import math
import warnings

import numpy as np
import pytest
import torch

import ema_ref as E
import optim_rules_ref as R

pytestmark = pytest.mark.gpu

SGD_ARMS = {"plain": dict(), "momentum": dict(momentum=0.9), "nesterov": dict(momentum=0.9, nesterov=True),
            "dampening_wd": dict(momentum=0.9, dampening=0.1, weight_decay=0.01)}
RULES = {"sgd": dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=0.01),
         "sgd_dampened": dict(lr=1e-3, momentum=0.9, dampening=0.1, weight_decay=0.01),
         "adam": dict(lr=1e-3, weight_decay=0.01)}
STATE = {"sgd": ("momentum_buffer",), "sgd_dampened": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq")}


def fused(rule):
    from spectre_vit.optim import FusedAdam, FusedSGD
    return FusedAdam if rule == "adam" else FusedSGD


def torch_cls(rule):
    return torch.optim.Adam if rule == "adam" else torch.optim.SGD


def snapshot(opt, ps, rule):
    snap = dict(param=[p.detach().clone() for p in ps], step=[opt.state[p]["step"].clone() for p in ps])
    for k in STATE[rule]:
        snap[k] = [opt.state[p][k].clone() for p in ps]
    if opt.ema_enabled:
        snap["ema"] = [opt.state[p]["ema"].clone() for p in ps]
    return snap


def changed(a, b):
    return {kind for kind in a if any(not torch.equal(x, y) for x, y in zip(a[kind], b[kind]))}


def cosine_pair(opt, W, T, eta_min):
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return SequentialLR(opt, [LinearLR(opt, start_factor=1.0 / (W + 1), total_iters=W),
                                  CosineAnnealingLR(opt, T_max=T - W, eta_min=eta_min)], milestones=[W])


# ---------------------------------------------------------------- 1. SGD: the restatement's bits, on both walks
@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("arm", list(SGD_ARMS))
def test_sgd_equals_the_restatement_bit_for_bit(arm, capturable):
    """six steps; after every one each parameter and each momentum buffer holds sgd_ref's bits.  The last tensor is an ALIGNED copy
    of the one behind the storage offset, fed the same gradients: the vector and the scalar walk end with equal bits."""
    from spectre_vit.optim import FusedSGD
    kw = dict(lr=1e-2, **SGD_ARMS[arm])
    ps = R.make_params(50)
    ps.append(ps[-1].detach().clone().requires_grad_(True))
    assert ps[-2].data_ptr() % 16 == 4 and ps[-1].data_ptr() % 16 == 0
    opt = FusedSGD(ps, capturable=capturable, **kw)
    ref_p = [p.detach().cpu().numpy().reshape(-1).copy() for p in ps]
    ref_b = [None] * len(ps)
    gen = torch.Generator().manual_seed(51)
    for step in range(6):
        grads = R.make_grads(gen, 0.1 + step)
        grads.append(grads[-1].clone())
        R.set_grads(ps, grads)
        opt.step()
        for i, g in enumerate(grads):
            ref_p[i], ref_b[i] = R.sgd_ref(ref_p[i], g.cpu().numpy().reshape(-1), ref_b[i], step + 1, **kw)
            assert np.array_equal(R.bits(ps[i]), R.bits(ref_p[i])), (arm, step, i, float(np.abs(ps[i].detach().cpu().numpy().reshape(-1) - ref_p[i]).max()))
            if "momentum" in SGD_ARMS[arm]:
                assert np.array_equal(R.bits(opt.state[ps[i]]["momentum_buffer"]), R.bits(ref_b[i])), (arm, step, i)
            else:
                assert "momentum_buffer" not in opt.state[ps[i]]
        assert torch.equal(ps[-1], ps[-2])
        assert float(opt.state[ps[0]]["step"]) == step + 1


# ---------------------------------------------------------------- 2. Adam without decay IS AdamW without decay
@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("controlled", [False, True])
def test_adam_without_decay_equals_adamw_bit_for_bit(controlled, ema):
    from spectre_vit.optim import CosineSchedule, FusedAdam, FusedAdamW
    kw = dict(lr=1e-3, weight_decay=0.0, capturable=True)
    if controlled:
        kw.update(schedule=CosineSchedule(8, 3, 1e-5), max_grad_norm=1.0)
    if ema:
        kw.update(ema_decay=0.9, ema_warmup=True)
    a = R.make_params(52)
    b = R.clone_params(a)
    oa, ob = FusedAdam(a, **kw), FusedAdamW(b, **kw)
    gen = torch.Generator().manual_seed(53)
    for step in range(5):
        grads = R.make_grads(gen, 1e-5 if step == 3 else 0.1 + step)
        R.set_grads(a, grads)
        R.set_grads(b, grads)
        oa.step()
        ob.step()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (i, (x - y).abs().max().item())
        for k in ("exp_avg", "exp_avg_sq", "step") + (("ema",) if ema else ()):
            assert torch.equal(oa.state[x][k], ob.state[y][k]), (i, k)
    if controlled:
        assert oa.control_block_bytes() == ob.control_block_bytes()


# ---------------------------------------------------------------- 3. Adam with L2 decay against float64 torch
@pytest.mark.parametrize("capturable", [False, True])
def test_adam_with_decay_against_float64_torch(capturable):
    from spectre_vit.optim import FusedAdam
    a = R.make_params(54)
    b = [p.detach().double().requires_grad_(True) for p in a]
    oa = FusedAdam(a, lr=1e-3, weight_decay=0.01, capturable=capturable)
    ob = torch.optim.Adam(b, lr=1e-3, weight_decay=0.01)
    gen = torch.Generator().manual_seed(55)
    worst = 0.0
    for step in range(8):
        grads = R.make_grads(gen, 0.1 + step)
        R.set_grads(a, grads)
        for p, g in zip(b, grads):
            p.grad = g.double()
        oa.step()
        ob.step()
        for i, (x, y) in enumerate(zip(a, b)):
            worst = max(worst, (x.double() - y).abs().max().item())
            assert torch.allclose(x.double(), y, rtol=R.RTOL, atol=R.ATOL), (step, i, (x.double() - y).abs().max().item())
    print(f"FusedAdam(weight_decay=0.01, capturable={capturable}): worst |weight - float64 torch| over 8 steps {worst:.3e}")


# ---------------------------------------------------------------- 4. the control path of both rules
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_trajectory_with_clip_and_schedule_against_float64_torch(rule):
    """two groups (1e-3, 3e-4), CosineSchedule(8, 3, 1e-5), max_grad_norm=1 against torch's optimizer + clip_grad_norm_ + SequentialLR
    in float64; step 5's gradient norm is below 1 (the no-clip branch)"""
    from spectre_vit.optim import CosineSchedule
    W, T, eta_min, bases = 3, 8, 1e-5, (1e-3, 3e-4)
    kw = {k: v for k, v in RULES[rule].items() if k != "lr"}
    a = R.make_params(56)
    b = [p.detach().double().requires_grad_(True) for p in a]
    sched = CosineSchedule(T, warmup_steps=W, eta_min=eta_min)
    oa = fused(rule)([dict(params=a[:4], lr=bases[0]), dict(params=a[4:], lr=bases[1])], capturable=True, schedule=sched,
                     max_grad_norm=1.0, **kw)
    ob = torch_cls(rule)([dict(params=b[:4], lr=bases[0]), dict(params=b[4:], lr=bases[1])], **kw)
    sb = cosine_pair(ob, W, T, eta_min)
    gen = torch.Generator().manual_seed(57)
    worst = 0.0
    for step in range(8):
        grads = R.make_grads(gen, 1e-5 if step == 5 else 0.1 + step)
        want_norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
        assert (want_norm < 1.0) == (step == 5)
        R.set_grads(a, grads)
        for p, g in zip(b, grads):
            p.grad = g.double()
        oa.step()
        torch.nn.utils.clip_grad_norm_(b, 1.0)
        ob.step()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sb.step()
        for i, (x, y) in enumerate(zip(a, b)):
            err = (x.double() - y).abs().max().item()
            worst = max(worst, err)
            assert torch.allclose(x.double(), y, rtol=R.RTOL, atol=R.ATOL), (rule, step, i, err)
        for got, base in zip(oa.last_lr(), bases):
            want = np.float32(sched.lr_at(step, base))
            assert abs(np.float32(got) - want) <= np.spacing(want), (step, base, got, float(want))
        got_norm = oa.last_grad_norm()
        assert abs(got_norm - want_norm) <= 1e-5 * want_norm, (step, got_norm, want_norm)
    print(f"{rule}: worst |weight - float64 torch| over 8 controlled steps {worst:.3e}")
    for i, g in enumerate(grads):   # p.grad is not rewritten by the clip
        assert torch.equal(a[i].grad, g), i
    assert oa.schedule_step() == 8 and oa.skipped_steps() == 0 and float(oa.state[a[0]]["step"]) == 8.0


@pytest.mark.parametrize("rule", ["sgd_dampened", "adam"])
def test_a_nonfinite_step_changes_nothing_and_a_dropped_first_step_stays_the_first(rule):
    """skip_nonfinite with ema_decay: a NaN in the very FIRST step, then two clean steps, then an inf.  The dropped steps change no
    parameter, no buffer or moment, no count and no average, and bump skipped_steps().  For SGD with dampening the step after the
    dropped first one is still the first: buf = d (not 0.9 * 0 + 0.9 * d), bit for bit the restatement's count-1 step."""
    kw = RULES[rule]
    ps = R.make_params(58)
    opt = fused(rule)(ps, capturable=True, skip_nonfinite=True, ema_decay=0.9, **kw)
    gen = torch.Generator().manual_seed(59)
    i2049 = R.SHAPES.index((2049,))
    grads = R.make_grads(gen, 1.0)
    grads[i2049][2048] = float("nan")   # the first slot of the tensor's short chunk
    R.set_grads(ps, grads)
    p0 = [p.detach().clone() for p in ps]
    opt.step()
    first = snapshot(opt, ps, rule)
    assert all(torch.equal(x, y) for x, y in zip(first["param"], p0)) and all(torch.equal(x, y) for x, y in zip(first["ema"], p0))
    assert all(not s.any() for k in STATE[rule] for s in first[k])
    assert (opt.skipped_steps(), opt.schedule_step(), float(opt.state[ps[0]]["step"])) == (1, 1, 0.0)
    grads = R.make_grads(gen, 1.0)
    R.set_grads(ps, grads)
    opt.step()
    assert float(opt.state[ps[0]]["step"]) == 1.0 and opt.skipped_steps() == 1
    if rule == "sgd_dampened":
        for i, (p, g) in enumerate(zip(ps, grads)):
            want_p, want_b = R.sgd_ref(p0[i].cpu().numpy().reshape(-1), g.cpu().numpy().reshape(-1), None, 1, gscale=1.0, **kw)
            assert np.array_equal(R.bits(opt.state[p]["momentum_buffer"]), R.bits(want_b)), i
            assert np.array_equal(R.bits(p), R.bits(want_p)), i
    R.set_grads(ps, R.make_grads(gen, 1.0))
    opt.step()
    before = snapshot(opt, ps, rule)
    grads = R.make_grads(gen, 1.0)
    grads[-1][R.OFFSET_N - 1] = float("inf")   # the last element of the unaligned tensor (scalar walk)
    R.set_grads(ps, grads)
    opt.step()
    assert not changed(before, snapshot(opt, ps, rule))
    assert (opt.skipped_steps(), opt.schedule_step(), float(opt.state[ps[0]]["step"])) == (2, 4, 2.0)
    R.set_grads(ps, R.make_grads(gen, 1.0))
    opt.step()
    assert changed(before, snapshot(opt, ps, rule)) == {"param", "step", "ema", *STATE[rule]}
    assert all(torch.isfinite(p).all().item() for p in ps)


@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_two_accumulation_windows_against_the_float64_window_means(rule):
    """accumulate_steps=3, clip 1.0, ema_decay: nothing moves inside a window; at each boundary the weights follow float64 torch fed
    the float64 mean of the window's gradients (clipped), and last_grad_norm() is the mean's norm"""
    k = 3
    kw = RULES[rule]
    a = R.make_params(60)
    b = [p.detach().double().requires_grad_(True) for p in a]
    oa = fused(rule)(a, capturable=True, max_grad_norm=1.0, ema_decay=0.9, accumulate_steps=k, **kw)
    ob = torch_cls(rule)(b, **kw)
    gen = torch.Generator().manual_seed(61)
    for window in range(2):
        mean = [torch.zeros(n, dtype=torch.float64, device="cuda") for n in R.SIZES]
        for m in range(k):
            grads = R.make_grads(gen, 0.5 + window)
            for s, g in zip(mean, grads):
                s += g.double().view(-1)
            R.set_grads(a, grads)
            before = snapshot(oa, a, rule) if (window, m) != (0, 0) else None
            oa.step()
            if before is not None:
                moved = changed(before, snapshot(oa, a, rule))
                assert moved == (set() if m < k - 1 else {"param", "step", "ema", *STATE[rule]}), (window, m, moved)
            assert oa.micro_step() == (m + 1) % k and oa.schedule_step() == window + (1 if m == k - 1 else 0)
        mean = [s / k for s in mean]
        want_norm = math.sqrt(sum(float((s ** 2).sum()) for s in mean))
        for p, s in zip(b, mean):
            p.grad = s.view(p.shape).clone()
        torch.nn.utils.clip_grad_norm_(b, 1.0)
        ob.step()
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.allclose(x.double(), y, rtol=R.RTOL, atol=R.ATOL), (rule, window, i, (x.double() - y).abs().max().item())
        assert abs(oa.last_grad_norm() - want_norm) <= 1e-5 * want_norm
    assert float(oa.state[a[0]]["step"]) == 2.0 and oa.skipped_steps() == 0


@pytest.mark.parametrize("rule", ["sgd_dampened", "adam"])
def test_k1_is_the_plain_control_path_bit_for_bit(rule):
    from spectre_vit.optim import CosineSchedule
    cfg = dict(capturable=True, max_grad_norm=1.0, skip_nonfinite=True, schedule=CosineSchedule(8, 3, 1e-5), **RULES[rule])
    a = R.make_params(62)
    b = R.clone_params(a)
    oa, ob = fused(rule)(a, accumulate_steps=1, **cfg), fused(rule)(b, **cfg)
    gen = torch.Generator().manual_seed(63)
    for step in range(5):
        grads = R.make_grads(gen, 1e-5 if step == 3 else 0.1 + step)
        R.set_grads(a, grads)
        R.set_grads(b, grads)
        oa.step()
        ob.step()
        assert oa.control_block_bytes() == ob.control_block_bytes(), (step, oa._read_ctl(), ob._read_ctl())
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (i, (x - y).abs().max().item())
        for kind in STATE[rule] + ("step",):
            assert torch.equal(oa.state[x][kind], ob.state[y][kind]), (i, kind)
    assert oa.schedule_step() == 5 and oa.micro_step() == 0


# ---------------------------------------------------------------- 5. the weights' average
@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("rule,capturable", [("sgd", True), ("sgd", False), ("adam", True)])
def test_average_follows_the_definition_and_exchanges_in_place(rule, capturable, warmup):
    """six steps with ema_decay=0.9: the average against the float64 recurrence fed the device's own weights after every step, w_t the
    fp32 value the kernel forms from the step count (tests/ema_ref.py, its bound); the training itself is bit for bit what it is
    without the average; ema_weights() exchanges and restores bit for bit"""
    kw = RULES[rule]
    a = R.make_params(64)
    b = R.clone_params(a)
    oa = fused(rule)(a, capturable=capturable, ema_decay=0.9, ema_warmup=warmup, **kw)
    ob = fused(rule)(b, capturable=capturable, **kw)
    avg = [E.Average(p.detach().cpu().numpy()) for p in a]
    gen = torch.Generator().manual_seed(65)
    worst = 0.0
    for step in range(6):
        grads = R.make_grads(gen, 0.1 + step)
        R.set_grads(a, grads)
        R.set_grads(b, grads)
        oa.step()
        ob.step()
        w = E.weight(step + 1, 0.9, warmup)
        for i, p in enumerate(a):
            assert torch.equal(p, b[i]), (step, i)
            pn = p.detach().cpu().numpy()
            want = avg[i].update(pn, w)
            ratio = E.ratio(oa.state[p]["ema"].cpu().numpy(), want, step + 1, pn)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (rule, step, i, ratio)
    print(f"{rule} capturable={capturable} warmup={warmup}: worst |e - e64| / bound over 6 steps {worst:.3f}")
    live = [p.detach().clone() for p in a]
    ema = [oa.state[p]["ema"].clone() for p in a]
    ptrs = [p.data_ptr() for p in a]
    with oa.ema_weights():
        assert all(torch.equal(p, e) for p, e in zip(a, ema)) and all(torch.equal(oa.state[p]["ema"], q) for p, q in zip(a, live))
        with pytest.raises(RuntimeError, match=type(oa).__name__):
            oa.step()
    assert all(torch.equal(p, q) for p, q in zip(a, live)) and all(torch.equal(oa.state[p]["ema"], e) for p, e in zip(a, ema))
    assert ptrs == [p.data_ptr() for p in a]


# ---------------------------------------------------------------- 6. six graph replays
def test_graph_replays_follow_the_eager_loop():
    """the 1-layer fft model and 16-image batches of the graph tests with FusedSGD(nesterov, schedule, accumulate_steps=2): a warm-up
    window and six steps, eagerly TWICE (the spread of the eager loop against itself) and through GraphedTrainStep(warmup=2) + six
    replays.  last_lr(), last_grad_norm() and every weight of the replayed run against the eager run: bit-equal when eager twice is
    bit-equal, otherwise within 4 x the eager spread."""
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import CosineSchedule, FusedSGD
    cfg = dict(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=512, num_encoders=1, num_heads=16, hidden_dim=768,
               activation="gelu", dropout=0.0, mixer="fft")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    img = torch.randn(16, 3, 32, 32, generator=g).to(dev)
    labels = torch.randint(0, 100, (16,), generator=g).to(dev)
    img2 = torch.randn(16, 3, 32, 32, generator=g).to(dev)
    crit = torch.nn.CrossEntropyLoss()
    sched = CosineSchedule(6, 2)
    batches = [img, img2, img2, img, img, img2]

    def make():
        torch.manual_seed(11)
        m = SpectreViT(**cfg).to(dev).train()
        return m, FusedSGD(m.parameters(), lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.01, capturable=True, schedule=sched,
                           max_grad_norm=1.0, accumulate_steps=2)

    def eager():
        m, o = make()
        for x in [img, img] + batches:
            o.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = m(x)
            crit(out, labels).backward()
            o.step()
        return o.last_lr(), o.last_grad_norm(), [p.detach().clone() for p in m.parameters()], o.schedule_step()

    def gap(x, y):
        return (abs(x[0][0] - y[0][0]), abs(x[1] - y[1]), max((p - q).abs().max().item() for p, q in zip(x[2], y[2])))

    e1, e2 = eager(), eager()
    own = gap(e1, e2)
    m2, o2 = make()
    step = GraphedTrainStep(m2, o2, crit, img, labels, warmup=2)
    try:
        assert o2.schedule_step() == 1 and o2.micro_step() == 0
        for r, x in enumerate(batches, start=1):
            before = [p.detach().clone() for p in m2.parameters()]
            loss = step(x, labels).item()
            moved = any(not torch.equal(p, q) for p, q in zip(m2.parameters(), before))
            assert math.isfinite(loss) and moved == (r % 2 == 0), (r, loss, moved)
            assert o2.micro_step() == r % 2 and o2.schedule_step() == 1 + r // 2
        replayed = (o2.last_lr(), o2.last_grad_norm(), [p.detach().clone() for p in m2.parameters()], o2.schedule_step())
    finally:
        step.close()
    got = gap(e1, replayed)
    print(f"eager twice: |lr|, |norm|, |weight| gaps {own}; replayed against eager: {got}; lr {replayed[0]}, norm {replayed[1]}")
    assert replayed[3] == e1[3] == 4 and float(o2.state[next(iter(m2.parameters()))]["step"]) == 4.0
    assert replayed[0] == [float(np.float32(sched.lr_at(3, 1e-2)))]
    if own == (0.0, 0.0, 0.0):
        assert got == (0.0, 0.0, 0.0), "the eager loop repeats bit for bit, so the replayed one must equal it bit for bit"
    else:
        assert all(x <= 4.0 * y for x, y in zip(got, own)), (got, own)


# ---------------------------------------------------------------- 7., 8. the harness
PARENT_KEYS = {"epoch", "Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation", "steps", "val_samples"}


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_harness_trains_with_the_rule_from_a_graph(tmp_path, name):
    from spectre_vit.harness import train
    _, h = train("spectre_vit/configs/spectre_vit_cifar100.py", mixer="fft", epochs=1, steps_per_epoch=4, batch_size=16, n_train=64,
                 n_val=32, graph=True, log=lambda r: None, out_dir=str(tmp_path), optimizer=name)
    assert len(h) == 1 and h[0]["Optimizer"] == name and h[0]["steps"] == 4
    assert set(h[0]) == PARENT_KEYS | {"Optimizer"}
    assert math.isfinite(h[0]["Loss/Train"]) and math.isfinite(h[0]["Loss/Validation"])


def test_default_record_is_the_parent_commits(tmp_path):
    from spectre_vit.harness import train
    _, h = train("spectre_vit/configs/spectre_vit_cifar100.py", mixer="fft", epochs=1, steps_per_epoch=4, batch_size=16, n_train=64,
                 n_val=32, graph=True, log=lambda r: None, out_dir=str(tmp_path))
    assert len(h) == 1 and set(h[0]) == PARENT_KEYS and math.isfinite(h[0]["Loss/Train"])
