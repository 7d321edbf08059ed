"""Distillation on the resident loader, on the GPU: GraphedDistillStep(loader=) in cache mode (the fetch is the graph's first node, the
loss reads the cache through loader.index: one replay, no host call) and in teacher-logits mode (eager fetch, then the replay) against
the same step fed by hand with the same loader's batches, bit for bit; harness.train_distill(device_loader=True) eager and graph-replayed,
cached and uncached, with the device meter, on the MNIST config (the fused LDS fetch) and a 64-pixel config (the fused tiled fetch)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MNIST = "spectre_vit/configs/spectre_vit_mnist.py"
CONFIG64 = '''"""Small widths on 64 x 64 images in 8 x 8 patches: 64 patches, as the CIFAR preset has"""
random_seed = 42
learning_rate = 1e-3
batch_size = 8
val_batch_size = 256
epochs = 1
num_classes = 100
patch_size = 8
img_size = 64
in_channels = 3
num_heads = 16
dropout = {dropout}
hidden_dim = 768
adam_weight_decay = 0.01
adam_betas = (0.9, 0.999)
activation = "gelu"
num_encoders = 2
embed_dim = 512
num_patches = 64
use_spectre = True
spectre_threshold = 1.0
'''
# the MNIST preset with dropout off, for the one comparison that needs equal masks on both sides
MNIST_NO_DROPOUT = '''from spectre_vit.configs._presets import PRESETS as _P

globals().update(_P["spectre_vit_mnist"])
dropout = 0.0
'''


@pytest.fixture()
def configs(tmp_path):
    """name -> config path: the MNIST preset, a 64-pixel config, and a copy of each with dropout 0"""
    files = {"cfg_distill_loader_64": CONFIG64.format(dropout=0.001), "cfg_distill_loader_64_nodrop": CONFIG64.format(dropout=0.0),
             "cfg_distill_loader_mnist_nodrop": MNIST_NO_DROPOUT}
    for name, text in files.items():
        (tmp_path / f"{name}.py").write_text(text)
    sys.path.insert(0, str(tmp_path))
    try:
        yield {"mnist": MNIST, "px64": "cfg_distill_loader_64.py", "mnist_nodrop": "cfg_distill_loader_mnist_nodrop.py",
               "px64_nodrop": "cfg_distill_loader_64_nodrop.py"}
    finally:
        sys.path.remove(str(tmp_path))
        for name in files:
            sys.modules.pop(name, None)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---------------------------------------------------------------- GraphedDistillStep(loader=)
def _student(c):
    """the config's student with dropout 0: the step fed by hand and the loader-fed step then see the same arithmetic"""
    from spectre_vit.models.spectre.spectre import SpectreViT
    torch.manual_seed(11)
    return SpectreViT(img_size=c.img_size, patch_size=c.patch_size, in_channels=c.in_channels, num_classes=c.num_classes,
                      embed_dim=c.embed_dim, num_encoders=c.num_encoders, num_heads=c.num_heads, hidden_dim=c.hidden_dim, dropout=0.0,
                      activation=c.activation, mixer="fft").to(dev()).train()


@pytest.mark.parametrize("cached", [True, False], ids=["cache_mode", "teacher_logits_mode"])
@pytest.mark.parametrize("which,output", [("mnist", "augment"), ("px64", "augment_tiled")])
def test_loader_fed_step_equals_the_step_fed_by_hand(configs, monkeypatch, which, output, cached):
    """four steps (one warm-up, three replays): loss / soft / ce of every step and the weights afterwards, bit for bit; in cache mode the
    wrapped _native.call sees nothing during a replay, in teacher-logits mode nothing but the eager fetch in front of it"""
    from spectre_vit import _native, harness
    from spectre_vit.augment import TrainAugment
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.data import CIFAR_MEAN, CIFAR_STD, ResidentLoader
    from spectre_vit.distillation import DistillationLoss, TeacherLogitCache
    from spectre_vit.graph import GraphedDistillStep
    from spectre_vit.optim import FusedAdamW
    c = parse_config(configs[which])
    d, steps, B, n = dev(), 4, 8, 40
    assert harness._loader_output(True, False, c.in_channels, c.img_size, c.img_size) == output
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(0, 256, size=(n, c.img_size, c.img_size, c.in_channels), dtype=np.uint8)).to(d)
    y = torch.from_numpy(rng.integers(0, c.num_classes, size=n).astype(np.uint8)).to(d)
    aug = TrainAugment(CIFAR_MEAN[:c.in_channels], CIFAR_STD[:c.in_channels], seed=5)
    cache = TeacherLogitCache(n, c.num_classes, d)
    cache.store(None, (3 * torch.randn(n, c.num_classes, generator=torch.Generator().manual_seed(3))).to(d))
    teacher = lambda index: cache.logits[index]   # the stand-in teacher of teacher-logits mode: a function of the sample alone
    new_loader = lambda: ResidentLoader(x, y, B, seed=9, output=output, augment=aug)

    # the batches, from a loader of their own
    ld = new_loader()
    fed = []
    for _ in range(steps):
        ld.fetch()
        fed.append((ld.img.clone(), ld.labels.clone(), ld.index.clone()))

    def run(loader):
        m = _student(c)
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True)
        crit = DistillationLoss()
        issued, real = [], _native.call

        def recorder(name, *a):
            issued.append(name)
            return real(name, *a)
        if loader is None:
            img, lab, idx = fed[0]
            kw = dict(teacher_cache=cache, example_index=idx) if cached else dict(example_teacher_logits=teacher(idx))
            step = GraphedDistillStep(m, opt, crit, img, lab, warmup=1, **kw)
        else:
            if not cached:
                loader.fetch()
            kw = dict(teacher_cache=cache) if cached else dict(example_teacher_logits=teacher(loader.index))
            step = GraphedDistillStep(m, opt, crit, None, None, warmup=1, loader=loader, **kw)
        try:
            rec = [(step.warm_loss.item(), step.warm_soft.item(), step.warm_ce.item())]   # the warm-up step WAS step 0
            for k in range(1, steps):
                img, lab, idx = fed[k]
                if loader is None:
                    loss = step(img, lab, index=idx) if cached else step(img, lab, teacher(idx))
                else:
                    logits = None
                    monkeypatch.setattr(_native, "call", recorder)
                    if not cached:
                        loader.fetch()
                        monkeypatch.setattr(_native, "call", real)
                        logits = teacher(loader.index)
                        monkeypatch.setattr(_native, "call", recorder)
                    loss = step() if cached else step(teacher_logits=logits)
                    monkeypatch.setattr(_native, "call", real)
                    assert step.img is loader.img and step.labels is loader.labels
                    assert (step.index is loader.index) if cached else (step.index is None)
                    assert torch.equal(loader.index, idx) and torch.equal(loader.labels, lab) and same_bits(loader.img, img), k
                rec.append((loss.item(), step.soft.item(), step.ce.item()))
            assert step.replays == steps - 1
            if loader is not None:
                assert loader.step == steps == loader.device_step(), "cache mode: the capture consumed no step"
                assert issued == ([] if cached else [{"augment": "spv_loader_fetch_augment", "augment_tiled": "spv_loader_fetch_augment_tiled"}[output]] * (steps - 1)), issued
                with pytest.raises(ValueError, match="pass no index"):
                    step(index=fed[0][2])
                with pytest.raises(ValueError, match="without arguments"):
                    step(fed[0][0], fed[0][1])
        finally:
            step.close()
        return rec, {k: v.detach().clone() for k, v in m.state_dict().items()}

    by_hand, w_hand = run(None)
    by_loader, w_loader = run(new_loader())
    for k, (a, b) in enumerate(zip(by_hand, by_loader)):
        print(f"step {k}: fed by hand (loss, soft, ce) {a}  loader-fed {b}")
    assert by_hand == by_loader, "loss, soft and ce of every step, bit for bit"
    assert all(math.isfinite(v) for r in by_loader for v in r) and by_loader[0] != by_loader[-1]
    differing = [k for k in w_hand if not same_bits(w_hand[k], w_loader[k])]
    assert not differing, differing


# ---------------------------------------------------------------- harness.train_distill(device_loader=True)
class ProbeTeacher(torch.nn.Module):
    """logits = fixed elements of the flattened 224 view times a constant: pure indexing, no reduction, so a sample's logits do not
    depend on the batch it arrives in (tests/test_gpu_teacher_cache.py)"""

    def __init__(self, classes, in_channels, crop=224):
        super().__init__()
        g = torch.Generator().manual_seed(17)
        self.register_buffer("pick", torch.randint(0, in_channels * crop * crop, (classes,), generator=g))
        self.calls = 0

    def forward(self, x, return_features=False):
        self.calls += 1
        logits = x.flatten(1)[:, self.pick] * 1.5
        return (logits, logits) if return_features else logits


N_TRAIN, BATCH, STEPS = 64, 16, 3


def _train(tmp_path, config, tag, **kw):
    from spectre_vit.harness import train_distill
    events, seen = [], []

    def hook(kind, step, img, label):
        events.append((kind, step))
        if kind == "train":
            seen.append((step, img.detach().cpu().numpy(), label.detach().cpu().numpy()))
    out = str(tmp_path / tag)
    model, hist = train_distill(config, mixer="fft", out_dir=out, log=lambda r: None, batch_hook=hook, epochs=2, steps_per_epoch=STEPS,
                                batch_size=BATCH, n_train=N_TRAIN, n_val=32, teacher=ProbeTeacher(100, 3).to(dev()).eval(), **kw)
    lines = [json.loads(l) for l in open(os.path.join(out, "scalars.jsonl"))]
    batch = [(l["step"], l["Batch Loss/Train"], l["Batch Loss/Dist"], l["Batch Loss/CE"]) for l in lines if "Batch Loss/Train" in l]
    weights = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return dict(batch=batch, weights=weights, hist=hist, events=events, seen=seen)


def _differing(a, b):
    return [k for k in a["weights"] if not same_bits(a["weights"][k], b["weights"][k])]


def _restated(config):
    """the rows the loader draws in the six steps and the student's batches TrainAugment makes of them"""
    from spectre_vit import harness
    from spectre_vit.augment import TrainAugment
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.data import CIFAR_MEAN, CIFAR_STD, ResidentLoader
    c = parse_config(config)
    seed = getattr(c, "random_seed", 42)
    train_set = harness.SyntheticCifar(N_TRAIN, c, "cpu", seed=seed)
    nhwc = train_set.images.permute(0, 2, 3, 1).contiguous().to(dev())
    rows = [ResidentLoader.indices(N_TRAIN, BATCH, harness.loader_seed(seed), t, 0, 1, STEPS) for t in range(2 * STEPS)]
    aug = TrainAugment(CIFAR_MEAN[:c.in_channels], CIFAR_STD[:c.in_channels], seed=harness.augment_seed(seed, 0))
    batches = [aug(nhwc, torch.from_numpy(r).to(dev()), step=t).cpu().numpy() for t, r in enumerate(rows)]
    return train_set.labels.numpy(), rows, batches


@pytest.mark.parametrize("which", ["mnist", "px64"])
def test_train_distill_on_the_loader_eager(tmp_path, configs, which):
    """the "train" hook's batches are the restatement's, bit for bit; cached and uncached runs give bit-equal per-batch loss lines and
    weights (the rule of test_train_distill_cached_equals_uncached_bit_for_bit); the "teacher" hook fires uncached only"""
    config = configs[which]
    labels, rows, batches = _restated(config)
    u = _train(tmp_path, config, "u", device_loader=True)
    c = _train(tmp_path, config, "c", device_loader=True, cache_teacher=True)
    for run in (u, c):
        assert [s[0] for s in run["seen"]] == list(range(2 * STEPS)), "the hook is called once per step, after it"
        for t, (_, img, label) in enumerate(run["seen"]):
            assert (label.astype(np.int64) == labels[rows[t]].astype(np.int64)).all(), t
            assert img.dtype == np.float32 and img.shape == batches[t].shape, t
            assert (img.view(np.int32) == batches[t].view(np.int32)).all(), (t, float(np.abs(img - batches[t]).max()))
    print("uncached per-batch (step, Train, Dist, CE):", u["batch"])
    print("cached   per-batch (step, Train, Dist, CE):", c["batch"])
    assert len(u["batch"]) == 2 * STEPS and all(math.isfinite(v) for r in u["batch"] for v in r[1:])
    assert c["batch"] == u["batch"], "every per-batch scalar, bit for bit"
    assert not _differing(c, u), "every final weight, bit for bit"
    assert [e for e in u["events"] if e[0] == "teacher"] == [("teacher", t) for t in range(2 * STEPS)]
    assert not [e for e in c["events"] if e[0] == "teacher"] and [e for e in c["events"] if e[0] == "teacher_fill"]
    # the teacher hook keeps its place in front of the step, the train hook follows the step
    order = [e for e in u["events"] if e[0] in ("teacher", "train")]
    assert order == [(k, t) for t in range(2 * STEPS) for k in ("teacher", "train")]
    for r, ru in zip(c["hist"], u["hist"]):
        assert set(r) == set(ru) and r["steps"] == STEPS and r["Loss/Train"] == ru["Loss/Train"]


def _gap(a, b):
    loss = max(abs(p - q) for ra, rb in zip(a["batch"], b["batch"]) for p, q in zip(ra[1:], rb[1:]))
    weight = max(float((a["weights"][k].double() - b["weights"][k].double()).abs().max()) for k in a["weights"])
    return loss, weight


@pytest.mark.parametrize("cache_teacher", [True, False], ids=["cached", "uncached"])
@pytest.mark.parametrize("which", ["mnist_nodrop", "px64_nodrop"])
def test_train_distill_on_the_loader_graph_against_eager(tmp_path, configs, which, cache_teacher):
    """graph=True held to graph=False by the rule of test_graphed_step_fetches_and_augments_its_own_batches -- a control's own spread
    is the margin: zero spread asks for equal bits, otherwise 4 x the spread.  That rule's control and candidate run the same code
    path; an eager step and a replayed one do not.  Measured here, MI355X, (largest per-batch loss gap, largest weight gap): the eager
    loader-fed run repeats bit for bit, (0, 0); the replayed loader-fed run differs from it by (4.8e-07, 2.4e-07) in all four cases,
    one ulp of a loss near 4 and of a weight; the HOST-fed replayed run differs from the host-fed eager run by (9.5e-07, 6.0e-08) on the
    MNIST preset and (2.4e-07, 1.2e-07) on the 64-pixel config, cached and uncached alike -- the gap is the step classes', not the
    loader's.  So the control's spread has two parts, both taken in this test from code the
    loader does not touch: the eager loader-fed run twice, and the HOST-fed eager run against the HOST-fed replayed run (the same
    randperm batches on both sides).  The loader-fed replayed run may differ from the loader-fed eager run by 4 x the larger of the
    two, and must equal it bit for bit if both are zero.
    Dropout is off in the two configs -- a replayed step adds the graph's seed word to every mask seed, so with dropout on the two
    sides draw different masks by construction -- and both sides run the one-launch optimizer (skip_nonfinite=True puts FusedAdamW on
    the eager path too; no step is skipped)."""
    config = configs[which]
    kw = dict(cache_teacher=cache_teacher, skip_nonfinite=True)
    e1 = _train(tmp_path, config, "e1", device_loader=True, **kw)
    e2 = _train(tmp_path, config, "e2", device_loader=True, **kw)
    g = _train(tmp_path, config, "g", device_loader=True, graph=True, **kw)
    he = _train(tmp_path, config, "he", **kw)
    hg = _train(tmp_path, config, "hg", graph=True, **kw)
    own, base, got = _gap(e1, e2), _gap(he, hg), _gap(e1, g)
    print(f"eager loader-fed control twice: loss / weight gap {own}; host-fed graph against host-fed eager: {base}; "
          f"loader-fed graph against loader-fed eager: {got}; graph per-batch {g['batch']}")
    assert all(r["SkippedSteps"] == 0 for run in (e1, g, he, hg) for r in run["hist"])
    assert [s[0] for s in g["seen"]] == list(range(2 * STEPS))
    for (_, a, la), (_, b, lb) in zip(e1["seen"], g["seen"]):
        assert (a.view(np.int32) == b.view(np.int32)).all() and (la == lb).all(), "the same batches on both sides"
    for (_, a, la), (_, b, lb) in zip(he["seen"], hg["seen"]):
        assert (a.view(np.int32) == b.view(np.int32)).all() and (la == lb).all(), "the host-fed control: the same batches on both sides"
    assert all(math.isfinite(v) for r in g["batch"] for v in r[1:])
    margin = (max(own[0], base[0]), max(own[1], base[1]))
    if margin == (0.0, 0.0):
        assert got == (0.0, 0.0), "both controls repeat bit for bit, so the graph-replayed run must equal the eager one bit for bit"
    else:
        assert got[0] <= 4 * margin[0] and got[1] <= 4 * margin[1]


def test_train_distill_graph_cached_issues_no_call_per_step(tmp_path, configs, monkeypatch):
    """graph=True, cache_teacher=True on the loader: after step 0 built the step, a training step is ONE replay"""
    from spectre_vit import _native
    events, real = [], _native.call

    def recorder(name, *a):
        events.append(("call", name))
        return real(name, *a)

    def hook(kind, step, img, label):
        events.append((kind, step))
    from spectre_vit.harness import train_distill
    monkeypatch.setattr(_native, "call", recorder)
    train_distill(configs["px64"], mixer="fft", out_dir=str(tmp_path / "g"), log=lambda r: events.append(("log", r["epoch"])),
                  batch_hook=hook, epochs=2, steps_per_epoch=STEPS, batch_size=BATCH, n_train=N_TRAIN, n_val=32,
                  teacher=ProbeTeacher(100, 3).to(dev()).eval(), graph=True, cache_teacher=True, device_loader=True)
    monkeypatch.setattr(_native, "call", real)
    issued, window = {}, []
    for ev in events:
        if ev[0] == "call":
            window.append(ev[1])
        elif ev[0] == "train":
            issued[ev[1]] = [name for name in window if name.startswith("spv_")]
            window = []
        else:   # a validation batch, the teacher's fill, the epoch's log line
            window = []
    assert sorted(issued) == list(range(2 * STEPS))
    assert issued[0].count("spv_loader_fetch_augment_tiled") == 2, "step 0 builds the step: an eager warm-up fetch, then the capture"
    for t in range(1, 2 * STEPS):
        assert issued[t] == [], (t, issued[t])


def test_train_distill_device_meter_on_the_loader(tmp_path, configs):
    """the meter's books equal the host's, with the loader feeding the step: per-batch lines and the epoch's loss, bit for bit"""
    config = configs["mnist"]
    host = _train(tmp_path, config, "host", device_loader=True, cache_teacher=True)
    metered = _train(tmp_path, config, "meter", device_loader=True, cache_teacher=True, device_meter=True)
    assert metered["batch"] == host["batch"] and not _differing(metered, host)
    for rm, rh in zip(metered["hist"], host["hist"]):
        assert rm["Accuracy/Train"] == rh["Accuracy/Train"] and "Accuracy/TrainTop5" in rm and rm["steps"] == STEPS
        assert rm["Loss/Train"] == rh["Loss/Train"], "the same float64 adds in the same order (tests/test_gpu_train_meter.py)"


def test_train_distill_without_the_loader_is_unchanged(tmp_path, configs):
    """device_loader=False (the default) keeps the host's randperm order and its hook protocol: the "train" hook comes BEFORE the step,
    two runs agree bit for bit, and the batches differ from the loader's (another order)"""
    a = _train(tmp_path, configs["mnist"], "a")
    b = _train(tmp_path, configs["mnist"], "b", device_loader=False)
    on = _train(tmp_path, configs["mnist"], "on", device_loader=True)
    assert a["batch"] == b["batch"] and not _differing(a, b)
    order = [e for e in a["events"] if e[0] in ("teacher", "train")]
    assert order == [(k, t) for t in range(2 * STEPS) for k in ("train", "teacher")]
    assert any((x[2] != y[2]).any() for x, y in zip(a["seen"], on["seen"])), "the loader draws another order"
