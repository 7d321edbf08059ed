"""The resident loader on the GPU: every fetch against the numpy restatement tests/loader_ref.py (index, labels, both image modes, both
access widths, both label stores, across two epoch boundaries), sharding and arange order, resume, the captured fetch, the
graph-replayed training step that fetches its own batch against a host-fed one, and the harness flag."""
import json
import os

import numpy as np
import pytest
import torch

import loader_ref as R

pytestmark = pytest.mark.gpu

MEAN, STD = (0.5071, 0.4867, 0.4408), (0.2675, 0.2565, 0.2761)
MNIST = "spectre_vit/configs/spectre_vit_mnist.py"


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def make_set(n, C, H, W, label_dtype, seed=0):
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(n, H, W, C), dtype=np.uint8)
    labels = rng.integers(0, 100, size=n).astype(np.uint8 if label_dtype == torch.uint8 else np.int64)
    return images, labels


def offset_view(images):
    """the same set 4 bytes into its allocation: the base is not 16-byte aligned, so every 16-byte access is ruled out"""
    flat = torch.empty(images.size + 16, dtype=torch.uint8, device=dev())
    view = flat[4:4 + images.size].view(images.shape)
    view.copy_(torch.from_numpy(images))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def check_fetch(loader, images, labels, want_index, tag):
    """the buffers after one fetch against the restatement's rows `want_index`"""
    index = loader.index.cpu().numpy()
    assert (index == want_index).all(), (tag, index, want_index)
    assert (loader.labels.cpu().numpy() == labels[want_index].astype(np.int64)).all(), tag
    C = images.shape[3]
    if loader.output == "uint8":
        assert loader.img.dtype == torch.uint8 and (loader.img.cpu().numpy() == images[want_index]).all(), tag
    elif loader.output == "float":
        ref = R.normalise(images, want_index, MEAN[:C], STD[:C])
        err = float(np.abs(loader.img.cpu().numpy().astype(np.float64) - ref).max())
        assert loader.img.dtype == torch.float32 and err <= 1e-6, (tag, err)
        return err
    return 0.0


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["labels_u8", "labels_i64"])
@pytest.mark.parametrize("n,B", [(7, 3), (64, 64), (1000, 130)])
@pytest.mark.parametrize("C,H,W", [(3, 32, 32), (1, 28, 28), (3, 5, 7), (3, 64, 48)])
def test_fetch_against_the_restatement(C, H, W, n, B, label_dtype):
    """(3, 32, 32), (1, 28, 28), (3, 64, 48): 16-byte accesses (the last: three spans per image); (3, 5, 7): the scalar path; the
    4-byte-offset view sends the vectorisable shapes through the scalar path too.  2 S + 1 fetches cross two epoch boundaries."""
    from spectre_vit.data import ResidentLoader
    images, labels = make_set(n, C, H, W, label_dtype)
    S = R.steps_per_epoch(n, B, 1)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    assert x.data_ptr() % 16 == 0
    shifted = offset_view(images)
    kw = dict(mean=MEAN[:C], std=STD[:C], seed=42)
    loaders = {"float": ResidentLoader(x, y, B, output="float", **kw), "uint8": ResidentLoader(x, y, B, output="uint8", **kw),
               "none": ResidentLoader(x, y, B, output="none", **kw),
               "float@4": ResidentLoader(shifted, y, B, output="float", **kw), "uint8@4": ResidentLoader(shifted, y, B, output="uint8", **kw)}
    worst = 0.0
    for t in range(2 * S + 1):
        want = R.indices(n, B, 42, t, 0, 1, S)
        for tag, ld in loaders.items():
            assert ld.steps_per_epoch == S and ld.step == t
            ld.fetch()
            worst = max(worst, check_fetch(ld, images, labels, want, (tag, t)))
            assert ld.device_step() == t + 1 == ld.step, (tag, t)
    assert (loaders["float"].img == loaders["float@4"].img).all(), "both access widths compute the same bits"
    assert int(loaders["float"]._cursor[1].item()) == 0, "the arrival counter re-arms itself"
    print(f"{C}x{H}x{W} n={n} B={B}: {2 * S + 1} fetches x {len(loaders)} loaders, float mode max |err| {worst:.3e} (bound 1e-6)")


def test_sharding_and_arange_order():
    from spectre_vit.data import ResidentLoader
    n, B = 100, 8
    images, labels = make_set(n, 3, 5, 7, torch.int64, seed=1)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    sharded = ResidentLoader(x, y, B, seed=7, rank=1, world=3)
    S = R.steps_per_epoch(n, B, 3)
    assert sharded.steps_per_epoch == S == 4
    plain = ResidentLoader(x, y, B, seed=7, shuffle=False, steps_per_epoch=5)
    for t in range(2 * S + 1):
        sharded.fetch()
        check_fetch(sharded, images, labels, R.indices(n, B, 7, t, 1, 3, S), ("rank 1 of 3", t))
        plain.fetch()
        want = R.indices(n, B, 7, t, 0, 1, 5, shuffle=False)
        assert (want == np.arange(B) + (t % 5) * B).all()
        check_fetch(plain, images, labels, want, ("arange", t))


def test_resume():
    from spectre_vit.data import ResidentLoader
    n, B = 64, 8
    images, labels = make_set(n, 1, 28, 28, torch.uint8, seed=2)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    kw = dict(mean=MEAN[:1], std=STD[:1], seed=11)
    a = ResidentLoader(x, y, B, **kw)
    for k in (13, 0, 5):
        a.seek(k)
        assert a.device_step() == k == a.step
        a.fetch()
        check_fetch(a, images, labels, R.indices(n, B, 11, k), ("seek", k))
        assert a.device_step() == k + 1
    sd = a.state_dict()
    assert sd["step"] == 6 and json.loads(json.dumps(sd)) == sd
    b = ResidentLoader(x, y, B, **kw)
    b.load_state_dict(sd)
    assert b.step == 6 == b.device_step()
    a.fetch()
    b.fetch()
    check_fetch(b, images, labels, R.indices(n, B, 11, 6), "resumed")
    assert (a.img == b.img).all() and (a.index == b.index).all()
    with pytest.raises(ValueError, match="seed"):
        ResidentLoader(x, y, B, mean=MEAN[:1], std=STD[:1], seed=12).load_state_dict(sd)


def test_captured_fetch_replays_through_the_epochs():
    from spectre_vit.data import ResidentLoader
    n, B = 24, 8   # S = 3: five replays cross an epoch boundary
    images, labels = make_set(n, 3, 32, 32, torch.uint8, seed=3)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    eager = ResidentLoader(x, y, B, seed=5)
    want = []
    for t in range(5):
        eager.fetch()
        want.append((eager.index.clone(), eager.labels.clone(), eager.img.clone()))
    ld = ResidentLoader(x, y, B, seed=5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (a first launch outside the capture loads the code object; then the cursor goes back to 0)
        ld.fetch()
    torch.cuda.current_stream().wait_stream(side)
    ld.seek(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ld.fetch()
    assert ld.step == 0 == ld.device_step(), "a recorded launch does not run and is not counted"
    for t in range(5):   # nothing host-written between the replays
        graph.replay()
        ld.count_replay()
        assert (ld.index == want[t][0]).all() and (ld.labels == want[t][1]).all() and (ld.img == want[t][2]).all(), t
        check_fetch(ld, images, labels, R.indices(n, B, 5, t), ("replay", t))
    assert ld.device_step() == 5 == ld.step


# ---------------------------------------------------------------- the graph-replayed training step
def test_graphed_step_fetches_its_own_batches():
    """GraphedTrainStep(loader=...) against a host-fed GraphedTrainStep given the batches the restatement names, four steps (one
    warm-up, three replays).  The host-fed control runs twice: if its two runs agree bit for bit, so must the loader-fed run;
    otherwise the loader-fed run may differ by 4 x their largest difference."""
    from spectre_vit.data import ResidentLoader
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    cfg = dict(img_size=8, patch_size=4, in_channels=3, num_classes=10, embed_dim=16, num_encoders=2, num_heads=4, hidden_dim=32,
               dropout=0.0, activation="gelu", mixer="fft")
    n, B, seed, steps = 64, 8, 42, 4
    rng = np.random.default_rng(4)
    images = rng.integers(0, 256, size=(n, 8, 8, 3), dtype=np.uint8)
    labels = rng.integers(0, 10, size=n).astype(np.uint8)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    # the control's batches: the restatement's rows, normalised by the kernel's three fp32 operations in numpy (IEEE, no contraction)
    mean32 = np.asarray(MEAN, np.float32).reshape(1, 3, 1, 1)
    inv32 = (1.0 / np.asarray(STD, np.float64)).astype(np.float32).reshape(1, 3, 1, 1)
    rows = [R.indices(n, B, seed, t) for t in range(steps)]
    host_img = [torch.from_numpy((images[r].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0) - mean32) * inv32).to(dev())
                for r in rows]
    host_lab = [torch.from_numpy(labels[r].astype(np.int64)).to(dev()) for r in rows]

    def run(loader):
        torch.manual_seed(21)
        model = SpectreViT(**cfg).to(dev()).train()
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True)
        if loader is None:
            step = GraphedTrainStep(model, opt, CrossEntropyLoss(), host_img[0], host_lab[0], autocast_dtype=None, warmup=1)
        else:
            step = GraphedTrainStep(model, opt, CrossEntropyLoss(), None, None, autocast_dtype=None, warmup=1, loader=loader)
        try:
            losses = [step.warm_loss.clone()]
            for t in range(1, steps):
                losses.append((step(host_img[t], host_lab[t]) if loader is None else step()).detach().clone())
                if loader is not None:   # the buffers hold the batch the replay trained on
                    assert (loader.index.cpu().numpy() == rows[t]).all() and (step.img is loader.img) and (step.labels is loader.labels)
            torch.cuda.synchronize()
            return torch.stack(losses).cpu().double(), [p.detach().cpu().double() for p in model.parameters()]
        finally:
            step.close()

    def gap(a, b):
        return (float((a[0] - b[0]).abs().max()), max(float((p - q).abs().max()) for p, q in zip(a[1], b[1])))

    c1, c2 = run(None), run(None)
    own = gap(c1, c2)
    loader = ResidentLoader(x, y, B, seed=seed)
    fed = run(loader)
    assert loader.step == steps == loader.device_step(), "one warm-up step and three replays; the capture consumed none"
    got = gap(c1, fed)
    print(f"host-fed control twice: loss / weight gap {own}; loader-fed against it: {got}; losses {fed[0].tolist()}")
    assert torch.isfinite(fed[0]).all()
    if own == (0.0, 0.0):
        assert got == (0.0, 0.0), "the control repeats bit for bit, so the loader-fed step must equal it bit for bit"
    else:
        assert got[0] <= 4 * own[0] and got[1] <= 4 * own[1]


# ---------------------------------------------------------------- the harness
def _train(tmp_path, tag, **kw):
    from spectre_vit.harness import train
    seen = []
    hook = lambda kind, step, img, label: seen.append((step, img.detach().cpu().numpy(), label.detach().cpu().numpy())) if kind == "train" else None
    _, hist = train(MNIST, mixer="fft", out_dir=str(tmp_path / tag), log=lambda r: None, batch_hook=hook, epochs=2, steps_per_epoch=3,
                    n_train=64, n_val=16, batch_size=8, **kw)
    return hist, seen


@pytest.fixture(scope="module")
def harness_reference():
    """the harness's training set rebuilt on the host, and the rows the loader draws from it in the six steps"""
    from spectre_vit import harness
    from spectre_vit.configs.parser import parse_config
    c = parse_config(MNIST)
    seed = getattr(c, "random_seed", 42)
    train_set = harness.SyntheticCifar(64, c, "cpu", seed=seed)
    images = train_set.images.permute(0, 2, 3, 1).contiguous().numpy()
    rows = [R.indices(64, 8, harness.loader_seed(seed), t, 0, 1, 3) for t in range(6)]
    return images, train_set.labels.numpy(), rows, c.in_channels


@pytest.fixture(scope="module")
def host_fed_keys(tmp_path_factory):
    hist, seen = _train(tmp_path_factory.mktemp("host_fed"), "off")
    assert len(seen) == 6
    return [set(r) for r in hist]


@pytest.mark.parametrize("graph,augment,uint8_input", [(False, False, False), (True, False, False), (False, True, False), (True, True, False),
                                                       (True, False, True)],
                         ids=["eager", "graph", "eager_augment", "graph_augment", "graph_uint8"])
def test_harness_with_the_device_loader(tmp_path, harness_reference, host_fed_keys, graph, augment, uint8_input):
    images, labels, rows, C = harness_reference
    hist, seen = _train(tmp_path, "on", device_loader=True, graph=graph, augment=augment, uint8_input=uint8_input)
    assert [s[0] for s in seen] == list(range(6)), "the hook is called once per step, after it"
    for t, (_, img, label) in enumerate(seen):
        assert (label.astype(np.int64) == labels[rows[t]].astype(np.int64)).all(), t
        if uint8_input:
            assert img.dtype == np.uint8 and (img == images[rows[t]]).all(), t
        elif not augment:
            err = float(np.abs(img.astype(np.float64) - R.normalise(images, rows[t], MEAN[:C], STD[:C])).max())
            assert err <= 1e-6, (t, err)
        else:
            assert img.shape == (8, C) + images.shape[1:3] and np.isfinite(img).all()
    assert [set(r) for r in hist] == host_fed_keys, "the record is the host-fed run's"
    for rec in hist:
        assert rec["steps"] == 3 and np.isfinite(rec["Loss/Train"]) and np.isfinite(rec["Loss/Validation"])
        assert 0.0 <= rec["Accuracy/Train"] <= 1.0
    print(f"graph={graph} augment={augment} uint8={uint8_input}: {hist}")
