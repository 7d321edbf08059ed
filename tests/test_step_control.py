"""On-device step control, the host side (no GPU): the schedule's float64 definition against torch's own schedulers, the
constructor's refusals, and the C-ABI's argument validation (nothing is launched)."""
import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def torch_schedule(base_lr, warmup, total, eta_min):
    """the learning rates of SequentialLR([LinearLR, CosineAnnealingLR]) (CosineAnnealingLR alone without warm-up) at t = 0 .. total,
    read from an optimizer that is stepped once per iteration"""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.SGD([p], lr=base_lr)
    if warmup == 0:
        sched = CosineAnnealingLR(opt, T_max=total, eta_min=eta_min)
    else:
        sched = SequentialLR(opt, [LinearLR(opt, start_factor=1.0 / (warmup + 1), total_iters=warmup),
                                   CosineAnnealingLR(opt, T_max=total - warmup, eta_min=eta_min)], milestones=[warmup])
    lrs = []
    for _ in range(total + 1):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return lrs


@pytest.mark.parametrize("warmup,total,eta_min", [(0, 6, 0.0), (3, 8, 1e-5), (1, 2, 0.0)])
@pytest.mark.parametrize("base_lr", [1e-3, 3e-4])
def test_lr_at_matches_torch_schedulers(warmup, total, eta_min, base_lr):
    import warnings
    from spectre_vit.optim import CosineSchedule
    s = CosineSchedule(total, warmup_steps=warmup, eta_min=eta_min)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (SequentialLR's own calls of scheduler.step(epoch) warn)
        ref = torch_schedule(base_lr, warmup, total, eta_min)
    for t, want in enumerate(ref):
        got = s.lr_at(t, base_lr)
        print(f"W={warmup} T={total} eta_min={eta_min} base={base_lr} t={t}: lr_at {got!r} torch {want!r}")
        assert abs(got - want) <= 1e-15 * abs(want), (t, got, want)
    # past T the schedule stays at eta_min (torch's closed form would rise again)
    for t in (total + 1, total + 2, 3 * total, 10 ** 6):
        assert s.lr_at(t, base_lr) == eta_min


def test_constructors_refuse_bad_arguments():
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    with pytest.raises(ValueError, match="total_steps"):
        CosineSchedule(3, warmup_steps=3)
    with pytest.raises(ValueError, match="total_steps"):
        CosineSchedule(0)
    with pytest.raises(ValueError, match="eta_min"):
        CosineSchedule(8, eta_min=-1e-6)
    p = [torch.nn.Parameter(torch.zeros(4))]
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW(p, capturable=True, max_grad_norm=bad)
    for control in (dict(schedule=CosineSchedule(8)), dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="capturable"):
            FusedAdamW(p, capturable=False, **control)
        FusedAdamW(p, capturable=True, **control)   # the same arguments with capturable=True are accepted
    with pytest.raises(ValueError, match="schedule"):
        FusedAdamW(p, capturable=True, schedule="cosine")


def test_default_optimizer_is_untouched():
    """without the new arguments: no control path, torch's state_dict, and the readers say that there is nothing to read"""
    from spectre_vit.optim import FusedAdamW
    o = FusedAdamW([torch.nn.Parameter(torch.zeros(4))], capturable=True)
    assert not o.step_control
    assert set(o.state_dict().keys()) == {"state", "param_groups"}
    assert set(o.param_groups[0].keys()) == {"params", "lr", "betas", "eps", "weight_decay", "capturable"}
    with pytest.raises(RuntimeError, match="step-control"):
        o.last_lr()


def test_counters_travel_through_state_dict():
    """before the first step the control block is the one the optimizer will start from; load_state_dict() takes the counters"""
    from spectre_vit.optim import CosineSchedule, FusedAdamW
    mk = lambda: FusedAdamW([torch.nn.Parameter(torch.zeros(4))], lr=2e-3, capturable=True, schedule=CosineSchedule(8, 3), skip_nonfinite=True)
    o = mk()
    assert (o.schedule_step(), o.skipped_steps(), o.last_grad_norm()) == (0, 0, 0.0)
    sd = o.state_dict()
    assert sd["step_control"] == dict(schedule_step=0, skipped_steps=0)
    sd["step_control"] = dict(schedule_step=5, skipped_steps=2)
    o2 = mk()
    o2.load_state_dict(sd)
    assert (o2.schedule_step(), o2.skipped_steps()) == (5, 2)
    assert o2.state_dict()["step_control"] == dict(schedule_step=5, skipped_steps=2)


def test_c_abi_rejects_bad_step_control_arguments_before_any_launch(built):
    """as test_host_logic.test_c_abi_rejects_bad_arguments_before_any_launch: every call fails validation on the host (non-zero
    return, spv_last_error text, RuntimeError from the ctypes wrapper), so nothing is launched and no GPU is needed"""
    from spectre_vit import _native
    P = 16  # any non-null "pointer": validation fails before it would be used
    SCHEDULE, CLIP = 1, 2
    adam = (1e-3, 0.9, 0.999, 0.1, 0.001, 1e-8, 0.01)
    cases = [
        ("spv_grad_sumsq", (0, P, P, P, 1, P, 0), "null table"),
        ("spv_grad_sumsq", (P, P, P, 0, 1, P, 0), "null table"),
        ("spv_grad_sumsq", (P, P, P, P, 1, 0, 0), "null partials"),
        ("spv_grad_sumsq", (P, P, P, P, -1, P, 0), "nchunks"),
        ("spv_step_control", (P, -1, P, 1, P, 0, 0, 0, 0.0, 0.0, 0), "npartials"),
        ("spv_step_control", (P, 1, P, 1, 0, 0, 0, 0, 0.0, 0.0, 0), "null control block"),
        ("spv_step_control", (0, 1, P, 1, P, 0, 0, 0, 0.0, 0.0, 0), "null partials"),
        ("spv_step_control", (P, 1, 0, 1, P, 0, 0, 0, 0.0, 0.0, 0), "step_ptrs"),
        ("spv_step_control", (P, 1, P, 1, P, SCHEDULE, 3, 3, 0.0, 0.0, 0), "total_steps"),
        ("spv_step_control", (P, 1, P, 1, P, SCHEDULE, 3, 2, 0.0, 0.0, 0), "total_steps"),
        ("spv_step_control", (P, 1, P, 1, P, SCHEDULE, 0, 8, -1e-6, 0.0, 0), "eta_min"),
        ("spv_step_control", (P, 1, P, 1, P, CLIP, 0, 0, 0.0, 0.0, 0), "max_norm"),
        ("spv_step_control", (P, 1, P, 1, P, CLIP, 0, 0, 0.0, -1.0, 0), "max_norm"),
        ("spv_step_control", (P, 1, P, 1, P, 8, 0, 0, 0.0, 0.0, 0), "flags"),
        ("spv_adamw_multi_ctl", (0, P, P, P, 1) + adam + (P, P, 0), "null table"),
        ("spv_adamw_multi_ctl", (P, P, P, P, -1) + adam + (P, P, 0), "nchunks"),
        ("spv_adamw_multi_ctl", (P, P, P, P, 1) + adam + (0, P, 0), "null step count"),
        ("spv_adamw_multi_ctl", (P, P, P, P, 1) + adam + (P, 0, 0), "control block"),
        ("spv_adamw_multi_ctl", (P, P, P, P, 1, -1e-3) + adam[1:] + (P, P, 0), "base_lr"),
    ]
    lib = _native.load()
    for name, args, needle in cases:
        assert getattr(lib, name)(*args) != 0, (name, args)
        assert needle in lib.spv_last_error().decode(), (name, needle, lib.spv_last_error().decode())
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, needle, str(e.value))
