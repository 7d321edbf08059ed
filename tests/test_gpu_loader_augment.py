"""Fetch and augment in one launch on the GPU: ResidentLoader(output="augment") against the three-launch path it replaces -- the mode-none
fetch's rows (ResidentLoader.indices), TrainAugment.draw's table and TrainAugment's apply -- bit for bit, at the shapes where
tests/test_gpu_resident_loader.py and tests/test_gpu_augment.py hold those three to the numpy restatements and to float64; sharding
with two seeds, resume, the captured fetch, the graph-replayed step, and the harness (a step is one replay: the host issues no
library call)."""
import numpy as np
import pytest
import torch

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
    """the same set 4 bytes into its allocation"""
    flat = torch.empty(images.size + 16, dtype=torch.uint8, device=dev())
    view = flat[4:4 + images.size].view(images.shape)
    view.copy_(torch.from_numpy(images))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def same_bits(a, b):
    """two fp32 tensors hold the same 32-bit words (an == on floats would let -0 pass for +0 and fail NaN for NaN)"""
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def check_fetch(loader, aug, x, labels, t, tag, rank=0, world=1):
    """the loader's buffers after the fetch of step t against the three-launch path: the restated rows, aug.draw, aug's apply"""
    from spectre_vit.data import ResidentLoader
    _, H, W, _ = x.shape
    B = loader.batch_size
    want = ResidentLoader.indices(loader.n, B, loader.seed, t, rank, world, loader.steps_per_epoch, loader.shuffle)
    assert (loader.index.cpu().numpy() == want).all(), (tag, t)
    assert (loader.labels.cpu().numpy() == labels[want].astype(np.int64)).all(), (tag, t)
    table = aug.draw(B, step=t, height=H, width=W)
    assert same_bits(loader.params, table), (tag, t, "params")
    img = aug(x, torch.from_numpy(want).to(x.device), params=table)
    assert same_bits(loader.img, img), (tag, t, "img", float((loader.img - img).abs().max()))
    return table


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["labels_u8", "labels_i64"])
@pytest.mark.parametrize("n,B", [(7, 3), (64, 64), (1000, 130)])
@pytest.mark.parametrize("C,H,W", [(3, 32, 32), (1, 28, 28), (3, 5, 7)])
def test_fused_fetch_against_the_three_launch_path(C, H, W, n, B, label_dtype):
    """2 S + 1 fetches cross two epoch boundaries; (3, 5, 7) takes the scalar store, the others 16-byte stores"""
    from spectre_vit.augment import TrainAugment
    from spectre_vit.data import ResidentLoader
    images, labels = make_set(n, C, H, W, label_dtype)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    aug = TrainAugment(MEAN[:C], STD[:C], seed=(9 << 32) | 1234)
    ld = ResidentLoader(x, y, B, seed=42, output="augment", augment=aug)
    assert ld.img.shape == (B, C, H, W) and ld.params.shape == (B, 16) and ld.params.data_ptr() % 16 == 0
    addresses = (ld.img.data_ptr(), ld.params.data_ptr(), ld.index.data_ptr(), ld.labels.data_ptr())
    S = ld.steps_per_epoch
    assert S == n // B
    seen = set()
    for t in range(2 * S + 1):
        assert ld.step == t
        ld.fetch()
        table = check_fetch(ld, aug, x, labels, t, (C, H, W, n, B))
        assert ld.device_step() == t + 1 == ld.step, t
        seen.add(table.cpu().numpy().tobytes())
    assert len(seen) == 2 * S + 1, "every step draws a table of its own"
    assert addresses == (ld.img.data_ptr(), ld.params.data_ptr(), ld.index.data_ptr(), ld.labels.data_ptr())
    assert int(ld._cursor[1].item()) == 0, "the arrival counter re-arms itself"


def test_every_op_off_equals_the_float_mode():
    from spectre_vit.augment import TrainAugment
    from spectre_vit.data import ResidentLoader
    n, B = 64, 24
    images, labels = make_set(n, 3, 32, 32, torch.uint8, seed=5)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    off = TrainAugment(MEAN, STD, flip=0.0, jitter=(0.0, 0.0, 0.0, 0.0), grayscale=0.0, degrees=0.0, blur=0.0, erase=0.0, seed=3)
    fused = ResidentLoader(x, y, B, seed=8, output="augment", augment=off)
    plain = ResidentLoader(x, y, B, mean=MEAN, std=STD, seed=8, output="float")
    for t in range(2 * fused.steps_per_epoch + 1):
        fused.fetch()
        plain.fetch()
        assert (fused.index == plain.index).all() and (fused.labels == plain.labels).all(), t
        assert same_bits(fused.img, plain.img), t
        p = fused.params.cpu().numpy()
        assert (p[:, [0, 4, 6, 7, 8, 10, 11, 12, 13, 14, 15]] == 0).all() and (p[:, 1:4] == 1).all(), "the identity table (sigma aside)"


def test_offset_view_of_the_set():
    from spectre_vit.augment import TrainAugment
    from spectre_vit.data import ResidentLoader
    n, B = 40, 9
    images, labels = make_set(n, 3, 32, 32, torch.int64, seed=6)
    y = torch.from_numpy(labels).to(dev())
    shifted = offset_view(images)
    aug = TrainAugment(MEAN, STD, seed=77)
    ld = ResidentLoader(shifted, y, B, seed=1, output="augment", augment=aug)
    aligned = ResidentLoader(torch.from_numpy(images).to(dev()), y, B, seed=1, output="augment", augment=aug)
    for t in range(2 * ld.steps_per_epoch + 1):
        ld.fetch()
        aligned.fetch()
        check_fetch(ld, aug, shifted, labels, t, "set 4 bytes into its allocation")
        assert same_bits(ld.img, aligned.img) and same_bits(ld.params, aligned.params), t


def test_sharding_takes_two_seeds():
    """rank 1 of 3: the rows are the restatement's under the SHARED loader seed, the table is that of THIS rank's augment seed"""
    from spectre_vit import harness
    from spectre_vit.augment import TrainAugment
    from spectre_vit.data import ResidentLoader
    n, B, seed = 100, 8, 7
    images, labels = make_set(n, 3, 5, 7, torch.int64, seed=1)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    augs = [TrainAugment(MEAN, STD, seed=harness.augment_seed(seed, r)) for r in range(3)]
    ld = ResidentLoader(x, y, B, seed=harness.loader_seed(seed), rank=1, world=3, output="augment", augment=augs[1])
    assert ld.steps_per_epoch == 4 and ld.seed == 7 and augs[1].seed == (1 << 32) | 7
    for t in range(2 * ld.steps_per_epoch + 1):
        ld.fetch()
        table = check_fetch(ld, augs[1], x, labels, t, "rank 1 of 3", rank=1, world=3)
        for other in (augs[0], augs[2]):
            assert not same_bits(table, other.draw(B, step=t, height=5, width=7)), "the ranks draw different tables"


def test_resume():
    from spectre_vit.augment import TrainAugment
    from spectre_vit.data import ResidentLoader
    n, B = 64, 8
    images, labels = make_set(n, 1, 28, 28, torch.uint8, seed=2)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    aug = TrainAugment(MEAN[:1], STD[:1], seed=19)
    fresh = ResidentLoader(x, y, B, seed=11, output="augment", augment=aug)
    kth = []
    for t in range(14):
        fresh.fetch()
        kth.append((fresh.index.clone(), fresh.params.clone(), fresh.img.clone()))
    a = ResidentLoader(x, y, B, seed=11, output="augment", augment=aug)
    for k in (13, 0, 5):
        a.seek(k)
        assert a.device_step() == k == a.step
        a.fetch()
        assert (a.index == kth[k][0]).all() and same_bits(a.params, kth[k][1]) and same_bits(a.img, kth[k][2]), k
        assert a.device_step() == k + 1
    b = ResidentLoader(x, y, B, seed=11, output="augment", augment=aug)
    b.load_state_dict(a.state_dict())
    b.fetch()
    assert b.step == 7 and (b.index == kth[6][0]).all() and same_bits(b.params, kth[6][1]) and same_bits(b.img, kth[6][2])


def test_captured_fetch_replays_through_the_epochs():
    from spectre_vit.augment import TrainAugment
    from spectre_vit.data import ResidentLoader
    n, B = 24, 8   # S = 3: five replays cross an epoch boundary
    images, labels = make_set(n, 3, 32, 32, torch.uint8, seed=3)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    aug = TrainAugment(MEAN, STD, seed=31)
    eager = ResidentLoader(x, y, B, seed=5, output="augment", augment=aug)
    assert eager.steps_per_epoch == 3
    want = []
    for t in range(5):
        eager.fetch()
        want.append((eager.index.clone(), eager.labels.clone(), eager.params.clone(), eager.img.clone()))
    ld = ResidentLoader(x, y, B, seed=5, output="augment", augment=aug)
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
    got = []
    for t in range(5):   # nothing host-written between the replays
        graph.replay()
        ld.count_replay()
        got.append((ld.index.clone(), ld.labels.clone(), ld.params.clone(), ld.img.clone()))
    for t in range(5):
        assert (got[t][0] == want[t][0]).all() and (got[t][1] == want[t][1]).all(), t
        assert same_bits(got[t][2], want[t][2]) and same_bits(got[t][3], want[t][3]), t
    assert not same_bits(got[0][2], got[1][2]) and not same_bits(got[0][2], got[3][2]), "a replay draws its own step's table"
    assert ld.device_step() == 5 == ld.step


# ---------------------------------------------------------------- the graph-replayed training step
def test_graphed_step_fetches_and_augments_its_own_batches():
    """GraphedTrainStep(loader=fused) against a host-fed GraphedTrainStep given TrainAugment(...)(images, rows[t], step=t), four steps
    (one warm-up, three replays).  The rule of test_gpu_resident_loader.test_graphed_step_fetches_its_own_batches: the host-fed control
    runs twice; if its two runs agree bit for bit, so must the loader-fed run; otherwise it may differ by 4 x their largest gap."""
    from spectre_vit.augment import TrainAugment
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
    aug = TrainAugment(MEAN, STD, seed=99)
    rows = [ResidentLoader.indices(n, B, seed, t) for t in range(steps)]
    host_img = [aug(x, torch.from_numpy(r).to(dev()), step=t) for t, r in enumerate(rows)]
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
                    assert same_bits(loader.img, host_img[t]), t
            torch.cuda.synchronize()
            return torch.stack(losses).cpu().double(), [p.detach().cpu().double() for p in model.parameters()]
        finally:
            step.close()

    def gap(a, b):
        return (float((a[0] - b[0]).abs().max()), max(float((p - q).abs().max()) for p, q in zip(a[1], b[1])))

    c1, c2 = run(None), run(None)
    own = gap(c1, c2)
    loader = ResidentLoader(x, y, B, seed=seed, output="augment", augment=aug)
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
def _train(tmp_path, tag, events=None, **kw):
    from spectre_vit.harness import train
    seen = []

    def hook(kind, step, img, label):
        if events is not None:
            events.append(("hook", kind, step))
        if kind == "train":
            seen.append((step, img.detach().cpu().numpy(), label.detach().cpu().numpy()))

    def log(rec):
        if events is not None:
            events.append(("log", rec["epoch"]))
    _, hist = train(MNIST, mixer="fft", out_dir=str(tmp_path / tag), log=log, batch_hook=hook, epochs=2, steps_per_epoch=3, n_train=64,
                    n_val=16, batch_size=8, **kw)
    return hist, seen


@pytest.fixture(scope="module")
def harness_reference():
    """the harness's training set, the rows the loader draws from it in the six steps, and the augmented batches of those steps as
    the three-launch path computes them"""
    from spectre_vit import harness
    from spectre_vit.augment import TrainAugment
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.data import CIFAR_MEAN, CIFAR_STD, ResidentLoader
    c = parse_config(MNIST)
    seed = getattr(c, "random_seed", 42)
    train_set = harness.SyntheticCifar(64, c, "cpu", seed=seed)
    nhwc = train_set.images.permute(0, 2, 3, 1).contiguous().to(dev())
    rows = [ResidentLoader.indices(64, 8, harness.loader_seed(seed), t, 0, 1, 3) for t in range(6)]
    aug = TrainAugment(CIFAR_MEAN[:c.in_channels], CIFAR_STD[:c.in_channels], seed=harness.augment_seed(seed, 0))
    batches = [aug(nhwc, torch.from_numpy(r).to(dev()), step=t).cpu().numpy() for t, r in enumerate(rows)]
    return train_set.labels.numpy(), rows, batches


@pytest.fixture(scope="module")
def host_fed_keys(tmp_path_factory):
    hist, seen = _train(tmp_path_factory.mktemp("host_fed"), "off", augment=True)
    assert len(seen) == 6
    return [set(r) for r in hist]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_harness_trains_on_the_fused_batches(tmp_path, monkeypatch, harness_reference, host_fed_keys, graph):
    from spectre_vit import _native
    labels, rows, batches = harness_reference
    events = []
    real = _native.call

    def recorder(name, *a):
        events.append(("call", name))
        return real(name, *a)
    monkeypatch.setattr(_native, "call", recorder)
    hist, seen = _train(tmp_path, "on", events=events, device_loader=True, augment=True, graph=graph)
    monkeypatch.setattr(_native, "call", real)
    assert [s[0] for s in seen] == list(range(6)), "the hook is called once per step, after it"
    for t, (_, img, label) in enumerate(seen):
        assert (label.astype(np.int64) == labels[rows[t]].astype(np.int64)).all(), t
        assert img.dtype == np.float32 and img.shape == batches[t].shape, t
        assert (img.view(np.int32) == batches[t].view(np.int32)).all(), (t, float(np.abs(img - batches[t]).max()))
    assert [set(r) for r in hist] == host_fed_keys, "the record is the host-fed run's"
    for rec in hist:
        assert rec["steps"] == 3 and np.isfinite(rec["Loss/Train"]) and np.isfinite(rec["Loss/Validation"])
    # what the host issued per step: the library calls between the end of the step before (its hook, or the epoch's log line after
    # the validation) and this step's hook
    issued, window = {}, []
    for ev in events:
        if ev[0] == "call":
            window.append(ev[1])
        elif ev[0] == "log" or ev[1] == "val":
            window = []
        else:
            issued[ev[2]] = [name for name in window if name.startswith("spv_")]
            window = []
    assert sorted(issued) == list(range(6))
    fetches = [names.count("spv_loader_fetch_augment") for names in issued.values()]
    if graph:
        assert "spv_loader_fetch_augment" in issued[0], "step 0 builds the step: an eager warm-up fetch, then the capture"
        for t in range(1, 6):
            assert issued[t] == [], (t, issued[t], "a step is one replay: the host issues no library call")
    else:
        assert fetches == [1] * 6, "one fused launch per step"
        for names in issued.values():
            assert not {"spv_loader_fetch", "spv_augment_params", "spv_augment_u8"} & set(names), names
