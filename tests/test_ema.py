"""Weight averaging (EMA) of FusedAdamW, the host side (no GPU): the new symbols, the constructor's and the harness's refusals before
a device is touched, the float64 / float32 definition of the per-step weight, the state-dict rules and the CLI flags."""
import inspect
import os

import numpy as np
import pytest
import torch

import ema_ref as R


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def params():
    return [torch.nn.Parameter(torch.zeros(4))]


def test_symbols_are_exported_and_bound(built):
    from spectre_vit import _native, optim, timing
    lib = _native.load()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spv.h")).read()
    for name in ("spv_adamw_multi_ema", "spv_adamw_multi_ctl_ema"):
        assert hasattr(lib, name) and name in _native.SIGNATURES and f"int {name}(" in src
        assert name in timing._WORK_MODELS, "bench.py's roofline pass brackets every launch it sees"
    # the siblings' arguments, then ema_table / ema_weight / ema_warmup (/ ema_step), then the stream
    S = _native.SIGNATURES
    assert S["spv_adamw_multi_ema"][:15] == S["spv_adamw_multi"][:15] and len(S["spv_adamw_multi_ema"]) == len(S["spv_adamw_multi"]) + 4
    assert S["spv_adamw_multi_ctl_ema"][:14] == S["spv_adamw_multi_ctl"][:14]
    assert len(S["spv_adamw_multi_ctl_ema"]) == len(S["spv_adamw_multi_ctl"]) + 3
    assert lib.spv_version() == 1
    for name in ("ema_weight_at", "FusedAdamW"):
        assert hasattr(optim, name)
    sig = inspect.signature(optim.FusedAdamW.__init__)
    assert sig.parameters["ema_decay"].default is None and sig.parameters["ema_warmup"].default is False
    for name in ("ema_parameters", "ema_state_dict", "ema_weights"):
        assert callable(getattr(optim.FusedAdamW, name))


def test_c_abi_rejects_bad_ema_arguments_before_any_launch(built):
    from spectre_vit import _native
    P = 16  # any non-null "pointer": validation fails before it would be used
    adam = (1e-3, 0.9, 0.999, 0.1, 0.001, 1e-8, 0.01)
    cases = [
        ("spv_adamw_multi_ema", (0, P, P, P, 1) + adam + (0.0, 0.0, P, P, 0.1, 0, 0.0, 0), "null table"),
        ("spv_adamw_multi_ema", (P, P, P, P, -1) + adam + (0.0, 0.0, P, P, 0.1, 0, 0.0, 0), "nchunks"),
        ("spv_adamw_multi_ema", (P, P, P, P, 1) + adam + (0.0, 0.0, P, 0, 0.1, 0, 0.0, 0), "null ema_table"),
        ("spv_adamw_multi_ema", (P, P, P, P, 1) + adam + (0.0, 0.5, 0, P, 0.1, 0, 1.0, 0), "bias corrections"),
        ("spv_adamw_multi_ema", (P, P, P, P, 1) + adam + (0.0, 0.0, P, P, 0.0, 0, 0.0, 0), "ema_weight"),
        ("spv_adamw_multi_ema", (P, P, P, P, 1) + adam + (0.0, 0.0, P, P, 1.5, 0, 0.0, 0), "ema_weight"),
        ("spv_adamw_multi_ema", (P, P, P, P, 1) + adam + (0.5, 0.5, 0, P, 0.1, 1, 0.0, 0), "ema_step"),
        ("spv_adamw_multi_ctl_ema", (0, P, P, P, 1) + adam + (P, P, P, 0.1, 0, 0), "null table"),
        ("spv_adamw_multi_ctl_ema", (P, P, P, P, -1) + adam + (P, P, P, 0.1, 0, 0), "nchunks"),
        ("spv_adamw_multi_ctl_ema", (P, P, P, P, 1) + adam + (0, P, P, 0.1, 0, 0), "null step count"),
        ("spv_adamw_multi_ctl_ema", (P, P, P, P, 1) + adam + (P, 0, P, 0.1, 0, 0), "control block"),
        ("spv_adamw_multi_ctl_ema", (P, P, P, P, 1) + adam + (P, P, 0, 0.1, 0, 0), "null ema_table"),
        ("spv_adamw_multi_ctl_ema", (P, P, P, P, 1) + adam + (P, P, P, 0.0, 0, 0), "ema_weight"),
        ("spv_adamw_multi_ctl_ema", (P, P, P, P, 1, -1e-3) + adam[1:] + (P, P, P, 0.1, 0, 0), "base_lr"),
    ]
    lib = _native.load()
    for name, args, needle in cases:
        assert getattr(lib, name)(*args) != 0, (name, args)
        assert needle in lib.spv_last_error().decode(), (name, needle, lib.spv_last_error().decode())
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, needle, str(e.value))


def test_constructor_refusals():
    from spectre_vit.optim import FusedAdamW
    for bad in (1.0, -0.1, 1.5, float("nan"), True):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW(params(), ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW([dict(params=params(), ema_decay=bad)])
    with pytest.raises(ValueError, match="ema_warmup"):
        FusedAdamW(params(), ema_warmup=True)
    with pytest.raises(ValueError, match="ema_warmup"):
        FusedAdamW([dict(params=params(), ema_decay=None)], ema_warmup=True)
    with pytest.raises(ValueError, match="ema_exclude"):
        FusedAdamW(params(), ema_exclude=params())
    # accepted: with and without capturable, with step control, a group of its own, a group that opts out
    for kw in (dict(), dict(capturable=True), dict(capturable=True, skip_nonfinite=True, max_grad_norm=1.0), dict(static_grads=True)):
        o = FusedAdamW(params(), ema_decay=0.0, ema_warmup=True, **kw)
        assert o.ema_enabled and o.param_groups[0]["ema_decay"] == 0.0
    o = FusedAdamW([dict(params=params(), ema_decay=0.99), dict(params=params())], ema_warmup=True)
    assert [g["ema_decay"] for g in o.param_groups] == [0.99, None]
    o = FusedAdamW([dict(params=params(), ema_decay=None), dict(params=params())], ema_decay=0.9)
    assert [g["ema_decay"] for g in o.param_groups] == [None, 0.9]


def test_off_is_exactly_the_optimizer_as_it_was():
    from spectre_vit.optim import FusedAdamW
    o = FusedAdamW(params(), capturable=True)
    assert not o.ema_enabled
    assert set(o.param_groups[0].keys()) == {"params", "lr", "betas", "eps", "weight_decay", "capturable"}
    sd = o.state_dict()
    assert set(sd) == {"state", "param_groups"} and "ema_decay" not in sd["param_groups"][0]
    ref = torch.optim.AdamW(params()).state_dict()
    assert sd["state"] == ref["state"] == {}
    with pytest.raises(RuntimeError, match="ema_decay"):
        with o.ema_weights():
            pass
    assert o.ema_parameters() == []
    # every group opted out: the key is there for the groups, but a saved state does not carry it
    o = FusedAdamW([dict(params=params(), ema_decay=None)])
    assert not o.ema_enabled and "ema_decay" not in o.state_dict()["param_groups"][0]


def test_loading_a_state_without_the_average_keeps_the_decay():
    """a torch.optim.AdamW checkpoint, or one saved with averaging off, into an averaging optimizer: its groups keep their ema_decay
    (torch's loader replaces the groups wholesale), and a saved decay wins like every other saved hyper-parameter"""
    from spectre_vit.optim import FusedAdamW
    o = FusedAdamW([dict(params=params(), ema_decay=0.5), dict(params=params())], ema_decay=0.9, ema_warmup=True)
    plain = torch.optim.AdamW([dict(params=params()), dict(params=params())]).state_dict()
    o.load_state_dict(plain)
    assert [g["ema_decay"] for g in o.param_groups] == [0.5, 0.9] and o.ema_enabled
    saved = FusedAdamW([dict(params=params()), dict(params=params(), ema_decay=None)], ema_decay=0.75).state_dict()
    assert [g["ema_decay"] for g in saved["param_groups"]] == [0.75, None]
    o.load_state_dict(saved)
    assert [g["ema_decay"] for g in o.param_groups] == [0.75, None]
    saved["param_groups"][0]["ema_decay"] = 1.0
    with pytest.raises(ValueError, match="ema_decay"):
        o.load_state_dict(saved)


def test_ema_weight_at_is_the_definition():
    from spectre_vit.optim import ema_weight_at
    for d in (0.9, 0.999, 0.9999):
        w = np.float32(1.0 - d)
        assert ema_weight_at(1, d, False) == ema_weight_at(12345, d, False) == float(w)
        assert ema_weight_at(1, d) == float(w)
        larger = 0
        for s in range(1, 2001):
            got = ema_weight_at(s, d, True)
            assert got == float(np.float32(got)), "an fp32 value"
            ramp64 = 9.0 / (10.0 + s)
            assert abs(got - max(1.0 - d, ramp64)) <= 2.0 ** -24 * got, (d, s, got)     # max(1 - d, 9 / (10 + s)), rounded to fp32
            ramp32 = np.float32(9) / np.float32(10 + s)
            if ramp32 > w:
                larger += 1
                assert got == float(ramp32), (d, s)
            else:
                assert got == float(w), (d, s)
            assert got == float(R.weight(s, d, True)), (d, s)
            # timm: decay_t = min(d, (1 + s) / (10 + s)) -> w_t = 1 - decay_t
            assert abs(got - (1.0 - min(d, (1.0 + s) / (10.0 + s)))) <= 1e-7
        assert larger == {0.9: 79, 0.999: 2000, 0.9999: 2000}[d]   # 9 / (10 + s) > 0.1 up to s = 79
    assert ema_weight_at(1, 0.0, True) == 1.0 and ema_weight_at(1, 0.999, True) == float(np.float32(9) / np.float32(11))


def test_harness_refuses_before_a_device_is_touched(tmp_path, monkeypatch):
    from spectre_vit import harness
    touched = []
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: touched.append(a))
    cfg = "spectre_vit/configs/spectre_vit_mnist.py"
    out = str(tmp_path / "x")
    for fn in (harness.train, harness.train_distill):
        for bad in (1.0, -0.5, 2.0):
            with pytest.raises(ValueError, match="ema_decay"):
                fn(cfg, out_dir=out, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_warmup"):
            fn(cfg, out_dir=out, ema_warmup=True)
        sig = inspect.signature(fn)
        assert sig.parameters["ema_decay"].default is None and sig.parameters["ema_warmup"].default is False
    assert not touched and not os.path.exists(out), "a refused run touches no device and leaves nothing behind"
    assert harness._ema_args(None, False) == {}
    assert harness._ema_args(0.99, True) == dict(ema_decay=0.99, ema_warmup=True)


def test_cli_flags_parse():
    from spectre_vit import harness
    a = harness.build_parser().parse_args([])
    assert a.ema_decay is None and a.ema_warmup is False
    a = harness.build_parser().parse_args(["--graph", "--ema-decay", "0.999", "--ema-warmup"])
    assert a.ema_decay == 0.999 and a.ema_warmup is True and a.graph is True
    a = harness.build_parser().parse_args(["--distill-paired", "--ema-decay", "0.9"])
    assert a.ema_decay == 0.9 and a.ema_warmup is False
