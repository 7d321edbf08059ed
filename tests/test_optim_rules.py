"""FusedSGD and FusedAdam, the host side (no GPU): the new symbols and their declarations, the C-ABI's, the constructors' and the
harness's refusals before any launch, the float32 restatements (tests/optim_rules_ref.py) against torch's own optimizers in float64,
and state dicts travelling to torch.optim.SGD / torch.optim.Adam and back."""
import copy
import inspect
import os
import re

import numpy as np
import pytest
import torch

import optim_rules_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [f"spv_{rule}_multi{suffix}" for rule in ("sgd", "adam") for suffix in ("", "_ema", "_ctl", "_ctl_ema")]

SGD_ARMS = {"plain": dict(), "momentum": dict(momentum=0.9), "nesterov": dict(momentum=0.9, nesterov=True),
            "dampening_wd": dict(momentum=0.9, dampening=0.1, weight_decay=0.01)}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


@pytest.fixture(scope="module")
def grads10():
    """ten steps of gradients on the tensor list, made once and shared (CPU, float32)"""
    gen = torch.Generator().manual_seed(41)
    return [R.make_grads(gen, 0.1 + step, dev="cpu") for step in range(10)]


def test_symbols_are_exported_bound_and_declared(built):
    from spectre_vit import _native
    lib = _native.load()
    header = open(os.path.join(ROOT, "include", "spv.h")).read()
    for name in NAMES:
        assert name in _native.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header), name
        assert _native.SIGNATURES[name][-1] is _native.c_vp   # the stream: a bracketed launcher like the AdamW ones


def test_c_abi_rejects_bad_arguments_before_any_launch(built):
    """every call fails validation on the host (non-zero return, spv_last_error text, RuntimeError from the ctypes wrapper): nothing
    is launched and no GPU is needed"""
    from spectre_vit import _native
    P = 16   # any non-null "pointer"
    tab, bad_tab = (P, P, P, P, 1), (0, P, P, P, 1)
    sgd = (0.9, 1.0, 0.01, 1)             # momentum, 1 - dampening, weight_decay, nesterov
    adam = (0.9, 0.999, 0.1, 0.001, 1e-8, 0.01)
    ema = (P, 0.01, 0)
    tails = {   # name -> (what follows the rule's arguments when all is well, index of step_dev / ctl in it)
        "spv_sgd_multi": (1.0, 0), "spv_sgd_multi_ema": (1.0, 0) + ema, "spv_sgd_multi_ctl": (P, P), "spv_sgd_multi_ctl_ema": (P, P) + ema,
        "spv_adam_multi": (0.1, 0.001, 0), "spv_adam_multi_ema": (0.1, 0.001, 0) + ema + (1.0,), "spv_adam_multi_ctl": (P, P),
        "spv_adam_multi_ctl_ema": (P, P) + ema}
    cases = []
    for name, tail in tails.items():
        rule = sgd if "sgd" in name else adam
        ctl = "_ctl" in name
        lr = (1e-3,)
        ok = lambda t=tab, r=rule, tl=tail: t + lr + r + tl + (0,)
        cases += [(name, ok(t=bad_tab), "null table"), (name, ok(t=(P, P, 0, P, 1)), "null table"),
                  (name, ok(t=(P, P, P, P, -1)), "nchunks"), (name, tab + (-1e-3,) + rule + tail + (0,), "lr")]
        if ctl:
            cases += [(name, ok(tl=(0,) + tail[1:]), "null step count"), (name, ok(tl=(P, 0) + tail[2:]), "control block")]
        if "ema" in name:
            i = tail.index(P, 2 if ctl else 0)
            cases += [(name, ok(tl=tail[:i] + (0,) + tail[i + 1:]), "null ema_table"),
                      (name, ok(tl=tail[:i + 1] + (0.0,) + tail[i + 2:]), "ema_weight")]
        if "sgd" in name:
            cases += [(name, ok(r=(1.0,) + sgd[1:]), "momentum"), (name, ok(r=(-0.1,) + sgd[1:]), "momentum"),
                      (name, ok(r=(0.9, 0.0, 0.01, 0)), "dampening"), (name, ok(r=(0.9, 1.1, 0.01, 0)), "dampening"),
                      (name, ok(r=(0.9, 0.9, 0.01, 1)), "nesterov"), (name, ok(r=(0.0, 1.0, 0.01, 1)), "nesterov"),
                      (name, ok(r=(0.9, 1.0, -0.01, 0)), "weight_decay")]
            if not ctl:   # no device count and no count by value
                cases.append((name, ok(tl=(0.0, 0) + tail[2:]), "null step count"))
        else:
            cases += [(name, ok(r=(1.0,) + adam[1:]), "betas"), (name, ok(r=adam[:5] + (-0.01,)), "weight_decay")]
            if not ctl:
                cases.append((name, ok(tl=(0.0, 0.001, 0) + tail[3:]), "bias corrections"))
    lib = _native.load()
    assert {c[0] for c in cases} == set(NAMES)
    for name, args, needle in cases:
        assert len(args) == len(_native.SIGNATURES[name]), (name, args)
        assert getattr(lib, name)(*args) != 0, (name, args, needle)
        assert needle in lib.spv_last_error().decode(), (name, needle, lib.spv_last_error().decode())
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, needle, str(e.value))


def test_constructor_refusals_name_the_class():
    from spectre_vit.optim import CosineSchedule, FusedAdam, FusedAdamW, FusedSGD
    p = [torch.nn.Parameter(torch.zeros(4))]
    # torch's own refusals
    for kw in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError, match="[Nn]esterov"):
            torch.optim.SGD(p, lr=0.1, **kw)
        with pytest.raises(ValueError, match="FusedSGD.*Nesterov"):
            FusedSGD(p, lr=0.1, **kw)
    for kw in (dict(lr=-1.0), dict(momentum=-0.1), dict(momentum=1.0), dict(dampening=1.0), dict(dampening=-0.1), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError, match="FusedSGD: invalid"):
            FusedSGD(p, **kw)
    with pytest.raises(ValueError, match="FusedSGD.*Nesterov"):
        FusedSGD([dict(params=p, momentum=0.0)], lr=0.1, momentum=0.9, nesterov=True)
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError, match="FusedAdam: invalid"):
            FusedAdam(p, **kw)
    # the control path's: everything that needs it needs capturable, and the message names the class in use
    for cls in (FusedSGD, FusedAdam, FusedAdamW):
        who = cls.__name__ + ":"
        for control in (dict(schedule=CosineSchedule(8)), dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(accumulate_steps=2)):
            with pytest.raises(ValueError, match=who + ".*capturable"):
                cls(p, capturable=False, **control)
            assert cls(p, capturable=True, **control).step_control
        for bad, needle in ((dict(max_grad_norm=0.0), "max_grad_norm"), (dict(schedule="cosine"), "schedule"),
                            (dict(accumulate_steps=0), "accumulate_steps"), (dict(ema_decay=1.0), "ema_decay"),
                            (dict(ema_warmup=True), "ema_warmup"), (dict(ema_exclude=p), "ema_exclude")):
            with pytest.raises(ValueError, match=who + ".*" + needle):
                cls(p, capturable=True, **bad)
        o = cls(p, capturable=True)
        assert not o.step_control and set(o.state_dict()) == {"state", "param_groups"}
        for reader in (o.last_lr, o.last_grad_norm, o.skipped_steps, o.schedule_step):
            with pytest.raises(RuntimeError, match=who + ".*step-control"):
                reader()
        for reader in (o.micro_step, o.accumulated_grads):
            with pytest.raises(RuntimeError, match=who + ".*accumulate_steps"):
                reader()
        with pytest.raises(RuntimeError, match=cls.__name__ + r"\.ema_weights\(\)"):
            with o.ema_weights():
                pass
        cpu = cls([torch.nn.Parameter(torch.zeros(4))])
        cpu.param_groups[0]["params"][0].grad = torch.zeros(4)
        with pytest.raises(RuntimeError, match=who + ".*no CPU fallback"):
            cpu.step()
    assert set(FusedSGD(p).param_groups[0]) == {"params", "lr", "momentum", "dampening", "weight_decay", "nesterov", "capturable"}
    assert set(FusedAdam(p).param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay", "capturable"}
    assert FusedAdam(p).defaults["weight_decay"] == 0.0 and FusedSGD(p).defaults["momentum"] == 0.0   # torch's defaults
    # the shared keywords are the same on all three
    shared = ["capturable", "static_grads", "schedule", "max_grad_norm", "skip_nonfinite", "ema_decay", "ema_warmup", "ema_exclude",
              "accumulate_steps"]
    for cls in (FusedSGD, FusedAdam, FusedAdamW):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[-len(shared):] == shared, (cls.__name__, names)


def run_torch(cls, grads, seed, dtype=torch.float64, **kw):
    ps = [p.detach().to(dtype).requires_grad_(True) for p in R.make_params(seed, dev="cpu")]
    opt = cls(ps, **kw)
    out = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(dtype).view(p.shape)
        opt.step()
        out.append([p.detach().clone() for p in ps])
    return out


def worst_ratio(got, want):
    """max over elements of |got - want| / (ATOL + RTOL |want|): <= 1 is torch.allclose(got, want, RTOL, ATOL)"""
    want = want.reshape(-1).numpy()
    got = got.detach().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.max(np.abs(got.reshape(-1).astype(np.float64) - want) / (R.ATOL + R.RTOL * np.abs(want))))


def allowed_ratio(cls, grads, seed, want, **kw):
    """the bound of a restatement against float64 torch, in units of (ATOL + RTOL |want|): 1, the optimizer tests' own bound.  Only
    where torch's OWN float32 CPU optimizer misses that bound against its float64 one on these inputs (the number format cannot meet
    it; measured without the code under test) is the arm allowed four times that distance instead."""
    t32 = run_torch(cls, grads, seed, dtype=torch.float32, **kw)
    d32 = max(worst_ratio(x, y) for xs, ys in zip(t32, want) for x, y in zip(xs, ys))
    return (1.0 if d32 <= 1.0 else 4.0 * d32), d32


@pytest.mark.parametrize("arm", list(SGD_ARMS))
def test_sgd_restatement_against_float64_torch(arm, grads10):
    kw = dict(lr=1e-2, **SGD_ARMS[arm])
    want = run_torch(torch.optim.SGD, grads10, 40, **kw)
    allowed, d32 = allowed_ratio(torch.optim.SGD, grads10, 40, want, **kw)
    ps = [p.detach().numpy().reshape(-1).copy() for p in R.make_params(40, dev="cpu")]
    bufs = [None] * len(ps)
    worst = 0.0
    for step, gs in enumerate(grads10):
        for i, g in enumerate(gs):
            ps[i], bufs[i] = R.sgd_ref(ps[i], g.numpy().reshape(-1), bufs[i], step + 1, **kw)
            worst = max(worst, worst_ratio(ps[i], want[step][i]))
    print(f"sgd[{arm}]: worst |ref32 - torch64| / (atol + rtol |torch64|) over 10 steps = {worst:.3f}; "
          f"torch's own float32 optimizer: {d32:.3f}; allowed {allowed:.3f}")
    assert worst <= allowed


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_restatement_against_float64_torch(wd, grads10):
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    want = run_torch(torch.optim.Adam, grads10, 42, **kw)
    allowed, d32 = allowed_ratio(torch.optim.Adam, grads10, 42, want, **kw)
    ps = [p.detach().numpy().reshape(-1).copy() for p in R.make_params(42, dev="cpu")]
    ms = [np.zeros_like(p) for p in ps]
    vs = [np.zeros_like(p) for p in ps]
    worst = 0.0
    for step, gs in enumerate(grads10):
        for i, g in enumerate(gs):
            ps[i], ms[i], vs[i] = R.adam_ref(ps[i], g.numpy().reshape(-1), ms[i], vs[i], step + 1, **kw)
            worst = max(worst, worst_ratio(ps[i], want[step][i]))
    print(f"adam[wd={wd}]: worst |ref32 - torch64| / (atol + rtol |torch64|) over 10 steps = {worst:.3f}; "
          f"torch's own float32 optimizer: {d32:.3f}; allowed {allowed:.3f}")
    assert worst <= allowed


def test_sgd_restatement_first_step_and_walk_independence():
    """count == 1 assigns the buffer (dampening does not touch the first gradient, as torch's clone), and the restatement is
    elementwise: a tensor and a copy of it give the same bits wherever they lie"""
    g = np.linspace(-1, 1, 7, dtype=np.float32)
    p = np.ones(7, dtype=np.float32)
    p1, b1 = R.sgd_ref(p, g, None, 1, lr=0.1, momentum=0.9, dampening=0.5)
    assert np.array_equal(b1, g) and np.array_equal(p1, p - np.float32(0.1) * g)
    p2, b2 = R.sgd_ref(p1, g, b1, 2, lr=0.1, momentum=0.9, dampening=0.5)
    assert np.array_equal(b2, np.float32(0.9) * b1 + np.float32(0.5) * g)
    p0, b0 = R.sgd_ref(p, g, None, 1, lr=0.1)
    assert b0 is None and np.array_equal(p0, p - np.float32(0.1) * g)


def test_state_dicts_travel_to_torch_and_back():
    """on CPU tensors (no step is taken by the fused side): torch.optim.SGD / Adam step twice, their state loads into FusedSGD /
    FusedAdam, comes out again and loads into a fresh torch optimizer, which then continues exactly as the original does"""
    from spectre_vit.optim import FusedAdam, FusedSGD
    gen = torch.Generator().manual_seed(43)
    shapes = [(5,), (3, 4)]
    grads = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(3)]
    for tcls, fcls, kw, keys in ((torch.optim.SGD, FusedSGD, dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=0.01), ["momentum_buffer"]),
                                 (torch.optim.Adam, FusedAdam, dict(lr=1e-2, weight_decay=0.01), ["exp_avg", "exp_avg_sq", "step"])):
        init = [torch.randn(s, generator=gen) for s in shapes]
        mk = lambda: [torch.nn.Parameter(t.clone()) for t in init]
        a = mk()
        oa = tcls(a, **kw)
        for gs in grads[:2]:
            for p, g in zip(a, gs):
                p.grad = g.clone()
            oa.step()
        sd = copy.deepcopy(oa.state_dict())
        f = mk()
        of = fcls(f, **kw)
        of.load_state_dict(copy.deepcopy(sd))
        for p, q in zip(a, f):
            for k in keys:
                assert torch.equal(torch.as_tensor(of.state[q][k]).float(), torch.as_tensor(oa.state[p][k]).float()), (fcls.__name__, k)
        assert "capturable" in of.param_groups[0]
        back = of.state_dict()
        assert set(back) == {"state", "param_groups"}
        b = mk()
        with torch.no_grad():
            for p, q in zip(b, a):
                p.copy_(q)
        ob = tcls(b, **kw)
        ob.load_state_dict(back)
        for x, y in ((a, oa), (b, ob)):
            for p, g in zip(x, grads[2]):
                p.grad = g.clone()
            y.step()
        for p, q in zip(a, b):
            assert torch.equal(p, q), tcls.__name__
        # the fused side's own state (a step count beside the buffers) loads into torch as well
        g2 = mk()
        og = fcls(g2, **kw)
        for q in g2:
            og._init_state(q, og.param_groups[0])
            og.state[q]["step"] = torch.tensor(2.0)
        tcls(mk(), **kw).load_state_dict(og.state_dict())


def test_a_torch_sgd_checkpoint_starts_the_count_at_one():
    """momentum buffers without a step count have been through a step: the count starts at 1, so that the next step (count 2) uses
    the buffers; a fresh state starts at 0, so that its first step assigns them"""
    from spectre_vit.optim import FusedSGD
    p = torch.nn.Parameter(torch.zeros(4))
    o = FusedSGD([p], lr=0.1, momentum=0.9)
    o._init_state(p, o.param_groups[0])
    assert o.state[p]["step"] is None and torch.equal(o.state[p]["momentum_buffer"], torch.zeros(4))
    t = torch.optim.SGD([p], lr=0.1, momentum=0.9)
    p.grad = torch.ones(4)
    t.step()
    o2 = FusedSGD([p], lr=0.1, momentum=0.9)
    o2.load_state_dict(t.state_dict())
    assert "step" not in o2.state[p]
    o2._init_state(p, o2.param_groups[0])
    assert float(o2.state[p]["step"]) == 1.0 and torch.equal(o2.state[p]["momentum_buffer"], torch.ones(4))
    o3 = FusedSGD([p], lr=0.1)   # momentum 0: no buffer at all, torch's layout
    o3._init_state(p, o3.param_groups[0])
    assert "momentum_buffer" not in o3.state[p]


def test_harness_refuses_bad_combinations_without_a_device(tmp_path, monkeypatch):
    from spectre_vit import harness
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was touched"))
    cfg = "spectre_vit/configs/spectre_vit_cifar100.py"
    bad = [(dict(optimizer="lamb"), "optimizer"), (dict(optimizer="sgd", momentum=1.0), "momentum"),
           (dict(optimizer="sgd", momentum=-0.1), "momentum"), (dict(optimizer="sgd", momentum=0.0), "nesterov"),
           (dict(optimizer="sgd", nesterov=1), "nesterov"), (dict(optimizer="adam", momentum=0.5), "belong to optimizer='sgd'"),
           (dict(optimizer="adamw", nesterov=False), "belong to optimizer='sgd'"), (dict(nesterov=False), "belong to optimizer='sgd'")]
    for fn in (harness.train, harness.train_distill):
        for kw, needle in bad:
            with pytest.raises(ValueError, match=needle):
                fn(cfg, out_dir=str(tmp_path), **kw)
        sig = inspect.signature(fn).parameters
        assert (sig["optimizer"].default, sig["momentum"].default, sig["nesterov"].default) == (None, 0.9, True)
    assert harness._optimizer_choice(None, 0.9, True) == (None, {})
    assert harness._optimizer_choice("adamw", 0.9, True) == ("adamw", {})
    assert harness._optimizer_choice("adam", 0.9, True) == ("adam", {})
    assert harness._optimizer_choice("sgd", 0.9, True) == ("sgd", dict(momentum=0.9, nesterov=True))
    assert harness._optimizer_choice("sgd", 0.0, False) == ("sgd", dict(momentum=0.0, nesterov=False))
    a = harness.build_parser().parse_args([])
    assert (a.optimizer, a.momentum, a.no_nesterov) == (None, 0.9, False)
    a = harness.build_parser().parse_args(["--optimizer", "sgd", "--momentum", "0.8", "--no-nesterov"])
    assert (a.optimizer, a.momentum, a.no_nesterov) == ("sgd", 0.8, True)
    with pytest.raises(SystemExit):
        harness.build_parser().parse_args(["--optimizer", "lamb"])
