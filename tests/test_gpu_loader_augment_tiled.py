"""Fetch, draw and contrast pre-pass in one launch on the GPU: ResidentLoader(output="augment_tiled") against the three calls it replaces
-- the mode-none fetch's rows (ResidentLoader.indices), TrainAugment.draw's table and the tiled apply (TrainAugment(kernel="tiled")) --
bit for bit, at one part, several parts, partial tiles and a plan-1 shape forced through; contrast off (every workgroup of the pre-pass
takes its early path), sharding with two seeds, the offset set, resume, the captured fetch, the graph-replayed step and the harness (a
step is one replay: the host issues no library call)."""
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN, STD = (0.5071, 0.4867, 0.4408), (0.2675, 0.2565, 0.2761)
CONTRAST = 2   # SPV_AUG_CONTRAST


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def count():
    from spectre_vit import _native
    return _native.call("spv_path_count", _native.PATH["augment"])


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


def tiled(C, seed, **kw):
    from spectre_vit.augment import TrainAugment
    return TrainAugment(MEAN[:C], STD[:C], seed=seed, kernel="tiled", **kw)


def check_fetch(loader, aug, x, labels, t, tag, rank=0, world=1):
    """the loader's buffers after the fetch of step t against the three calls: the restated rows, aug.draw, the tiled apply -- and the
    cursor block: the step moved on, the arrival counter re-armed"""
    from spectre_vit.data import ResidentLoader
    assert aug.kernel == "tiled"
    _, H, W, _ = x.shape
    B = loader.batch_size
    want = ResidentLoader.indices(loader.n, B, loader.seed, t, rank, world, loader.steps_per_epoch, loader.shuffle)
    assert (loader.index.cpu().numpy() == want).all(), (tag, t)
    assert (loader.labels.cpu().numpy() == labels[want].astype(np.int64)).all(), (tag, t)
    table = aug.draw(B, step=t, height=H, width=W)
    assert same_bits(loader.params, table), (tag, t, "params")
    img = aug(x, torch.from_numpy(want).to(x.device), params=table)
    assert same_bits(loader.img, img), (tag, t, "img", float((loader.img - img).abs().max()))
    assert loader.device_step() == t + 1, (tag, t)
    assert int(loader._cursor[1].item()) == 0, (tag, t, "the arrival counter re-arms itself")
    return table


def walk(C, H, W, n, B, label_dtype, aug=None, seed=42):
    """2 S + 1 fetches cross two epoch boundaries"""
    from spectre_vit import _native
    from spectre_vit.data import ResidentLoader
    images, labels = make_set(n, C, H, W, label_dtype)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    aug = aug or tiled(C, (9 << 32) | 1234)
    ld = ResidentLoader(x, y, B, seed=seed, output="augment_tiled", augment=aug)
    assert ld.img.shape == (B, C, H, W) and ld.params.shape == (B, 16) and ld.params.data_ptr() % 16 == 0
    assert ld._ws.numel() == _native.call("spv_augment_tiled_ws_bytes", B, H, W)
    addresses = (ld.img.data_ptr(), ld.params.data_ptr(), ld.index.data_ptr(), ld.labels.data_ptr(), ld._ws.data_ptr())
    S = ld.steps_per_epoch
    assert S == n // B
    tables = []
    before = count()
    for t in range(2 * S + 1):
        assert ld.step == t
        ld.fetch()
        tables.append(check_fetch(ld, aug, x, labels, t, (C, H, W, n, B)))
        assert ld.step == t + 1
    assert count() == before + 2 * (2 * S + 1), "one census count per fetch (and one per apply of the check)"
    assert len({tb.cpu().numpy().tobytes() for tb in tables}) == 2 * S + 1, "every step draws a table of its own"
    assert addresses == (ld.img.data_ptr(), ld.params.data_ptr(), ld.index.data_ptr(), ld.labels.data_ptr(), ld._ws.data_ptr())
    return tables


@pytest.mark.parametrize("C,H,W,n,B", [(3, 64, 64, 7, 3), (3, 64, 64, 64, 64), (3, 70, 45, 7, 3), (1, 130, 64, 7, 3), (3, 224, 224, 9, 4),
                                       (3, 32, 32, 7, 3)],
                         ids=["one_part", "one_part_b64", "partial_tiles_scalar_stores", "three_parts", "thirteen_parts", "plan1_forced"])
def test_fused_fetch_against_the_three_calls(C, H, W, n, B):
    from spectre_vit import _native
    parts = {(64, 64): 1, (70, 45): 1, (130, 64): 3, (224, 224): 13, (32, 32): 1}[(H, W)]
    assert _native.call("spv_augment_tiled_ws_bytes", B, H, W) == 4 * B * parts
    assert _native.call("spv_augment_plan", C, H, W) == (1 if H == 32 else 2)
    tables = walk(C, H, W, n, B, torch.uint8)
    contrast = torch.cat(tables)[:, CONTRAST]
    assert bool((contrast != 1.0).any()), "the pre-pass's summing path ran"


def test_int64_labels():
    walk(3, 64, 64, 7, 3, torch.int64)


def test_contrast_off_every_workgroup_takes_the_early_path():
    """contrast jitter 0 draws the factor 1 + 0 * u = 1 exactly: no workgroup of the pre-pass sums anything, all of them must still read
    the step and arrive (check_fetch: the cursor moved on, the counter is back at 0), and the images still match"""
    tables = walk(1, 130, 64, 7, 3, torch.uint8, aug=tiled(1, 77, jitter=(0.4, 0.0, 0.4, 0.1)))
    assert bool((torch.cat(tables)[:, CONTRAST] == 1.0).all())


def test_sharding_takes_two_seeds():
    """rank 1 of 2: the rows are the restatement's under the SHARED loader seed, the table is that of THIS rank's augment seed"""
    from spectre_vit import harness
    from spectre_vit.data import ResidentLoader
    n, B, seed = 30, 4, 7
    images, labels = make_set(n, 3, 70, 45, torch.int64, seed=1)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    augs = [tiled(3, harness.augment_seed(seed, r)) for r in range(2)]
    ld = ResidentLoader(x, y, B, seed=harness.loader_seed(seed), rank=1, world=2, output="augment_tiled", augment=augs[1])
    assert ld.steps_per_epoch == 3 and ld.seed == 7 and augs[1].seed == (1 << 32) | 7
    for t in range(2 * ld.steps_per_epoch + 1):
        ld.fetch()
        table = check_fetch(ld, augs[1], x, labels, t, "rank 1 of 2", rank=1, world=2)
        assert not same_bits(table, augs[0].draw(B, step=t, height=70, width=45)), "the ranks draw different tables"


def test_offset_view_of_the_set():
    from spectre_vit.data import ResidentLoader
    n, B = 10, 4
    images, labels = make_set(n, 3, 64, 64, torch.int64, seed=6)
    y = torch.from_numpy(labels).to(dev())
    shifted = offset_view(images)
    aug = tiled(3, 77)
    ld = ResidentLoader(shifted, y, B, seed=1, output="augment_tiled", augment=aug)
    aligned = ResidentLoader(torch.from_numpy(images).to(dev()), y, B, seed=1, output="augment_tiled", augment=aug)
    for t in range(2 * ld.steps_per_epoch + 1):
        ld.fetch()
        aligned.fetch()
        check_fetch(ld, aug, shifted, labels, t, "set 4 bytes into its allocation")
        assert same_bits(ld.img, aligned.img) and same_bits(ld.params, aligned.params), t


def test_resume():
    from spectre_vit.data import ResidentLoader
    n, B = 24, 4
    images, labels = make_set(n, 1, 130, 64, torch.uint8, seed=2)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    aug = tiled(1, 19)
    fresh = ResidentLoader(x, y, B, seed=11, output="augment_tiled", augment=aug)
    kth = []
    for t in range(14):
        fresh.fetch()
        kth.append((fresh.index.clone(), fresh.params.clone(), fresh.img.clone()))
    a = ResidentLoader(x, y, B, seed=11, output="augment_tiled", augment=aug)
    for k in (13, 0, 5):
        a.seek(k)
        assert a.device_step() == k == a.step
        a.fetch()
        assert (a.index == kth[k][0]).all() and same_bits(a.params, kth[k][1]) and same_bits(a.img, kth[k][2]), k
        assert a.device_step() == k + 1
    b = ResidentLoader(x, y, B, seed=11, output="augment_tiled", augment=aug)
    b.load_state_dict(a.state_dict())
    b.fetch()
    assert b.step == 7 and (b.index == kth[6][0]).all() and same_bits(b.params, kth[6][1]) and same_bits(b.img, kth[6][2])


def test_captured_fetch_replays_through_the_epochs():
    from spectre_vit.data import ResidentLoader
    C, H, W, n, B = 3, 64, 64, 20, 6   # S = 3: seven replays cross two epoch boundaries
    images, labels = make_set(n, C, H, W, torch.uint8, seed=3)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    aug = tiled(C, 31)
    ld = ResidentLoader(x, y, B, seed=5, output="augment_tiled", augment=aug)
    S = ld.steps_per_epoch
    assert S == 3
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
    tables = []
    for t in range(2 * S + 1):   # the check's own launches aside, nothing is host-written between the replays
        graph.replay()
        ld.count_replay()
        tables.append(check_fetch(ld, aug, x, labels, t, "replay"))
    assert not same_bits(tables[0], tables[1]) and not same_bits(tables[0], tables[S]), "a replay draws its own step's table"
    assert ld.device_step() == 2 * S + 1 == ld.step


# ---------------------------------------------------------------- the graph-replayed training step and the harness, on a 64-pixel config
CONFIG = '''"""Small widths on 64 x 64 images in 8 x 8 patches: 64 patches, as the CIFAR preset has"""
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
dropout = 0.001
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


@pytest.fixture()
def config64(tmp_path):
    (tmp_path / "cfg_loader_tiled_64.py").write_text(CONFIG)
    sys.path.insert(0, str(tmp_path))
    try:
        yield "cfg_loader_tiled_64.py"
    finally:
        sys.path.remove(str(tmp_path))
        sys.modules.pop("cfg_loader_tiled_64", None)


def test_graphed_step_is_one_replay_with_no_host_call(config64, monkeypatch):
    """GraphedTrainStep(loader=tiled) on the 64-pixel config: after the step is built the host issues NO library call, and every replay
    trains on the batch the three calls restate"""
    from spectre_vit import _native, harness
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.data import ResidentLoader
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.optim import FusedAdamW
    c = parse_config(config64)
    n, B, seed, steps = 64, 16, 42, 4
    images, labels = make_set(n, 3, 64, 64, torch.uint8, seed=4)
    x, y = torch.from_numpy(images).to(dev()), torch.from_numpy(labels).to(dev())
    aug = tiled(3, 99)
    rows = [ResidentLoader.indices(n, B, seed, t) for t in range(steps)]
    host_img = [aug(x, torch.from_numpy(r).to(dev()), step=t) for t, r in enumerate(rows)]
    torch.manual_seed(21)
    model = harness.build_model(c, "fft", dev()).train()
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True)
    loader = ResidentLoader(x, y, B, seed=seed, output="augment_tiled", augment=aug)
    step = GraphedTrainStep(model, opt, CrossEntropyLoss(), None, None, autocast_dtype=torch.bfloat16, warmup=1, loader=loader)
    try:
        assert same_bits(loader.img, host_img[0]), "the warm-up step trained on step 0's batch; the capture consumed none"
        issued = []
        real = _native.call

        def recorder(name, *a):
            issued.append(name)
            return real(name, *a)
        losses = [step.warm_loss.item()]
        for t in range(1, steps):
            monkeypatch.setattr(_native, "call", recorder)
            loss = step()
            monkeypatch.setattr(_native, "call", real)
            losses.append(loss.item())
            assert (loader.index.cpu().numpy() == rows[t]).all() and step.img is loader.img and step.labels is loader.labels
            assert (loader.labels.cpu().numpy() == labels[rows[t]].astype(np.int64)).all()
            assert same_bits(loader.img, host_img[t]), t
        assert issued == [], ("a step is one replay: the host issues no library call", issued)
        assert loader.step == steps == loader.device_step()
        assert all(np.isfinite(v) for v in losses) and losses[0] != losses[-1], losses
    finally:
        step.close()


def _train(tmp_path, config, tag, events=None, **kw):
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
    _, hist = train(config, mixer="fft", out_dir=str(tmp_path / tag), log=log, batch_hook=hook, epochs=2, steps_per_epoch=3, n_train=64,
                    n_val=16, batch_size=8, **kw)
    return hist, seen


def harness_reference(config):
    """the harness's training set, the rows the loader draws from it in the six steps, and the augmented batches of those steps as
    the three calls compute them"""
    from spectre_vit import harness
    from spectre_vit.augment import TrainAugment
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.data import CIFAR_MEAN, CIFAR_STD, ResidentLoader
    c = parse_config(config)
    seed = getattr(c, "random_seed", 42)
    train_set = harness.SyntheticCifar(64, c, "cpu", seed=seed)
    nhwc = train_set.images.permute(0, 2, 3, 1).contiguous().to(dev())
    rows = [ResidentLoader.indices(64, 8, harness.loader_seed(seed), t, 0, 1, 3) for t in range(6)]
    aug = TrainAugment(CIFAR_MEAN[:c.in_channels], CIFAR_STD[:c.in_channels], seed=harness.augment_seed(seed, 0))
    batches = [aug(nhwc, torch.from_numpy(r).to(dev()), step=t).cpu().numpy() for t, r in enumerate(rows)]
    return train_set.labels.numpy(), rows, batches


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_harness_trains_on_the_fused_tiled_batches(tmp_path, monkeypatch, config64, graph):
    from spectre_vit import _native
    labels, rows, batches = harness_reference(config64)
    host_keys = [set(r) for r in _train(tmp_path, config64, "off", augment=True, graph=graph)[0]]
    events = []
    real = _native.call

    def recorder(name, *a):
        events.append(("call", name))
        return real(name, *a)
    before = count()
    monkeypatch.setattr(_native, "call", recorder)
    hist, seen = _train(tmp_path, config64, "on", events=events, device_loader=True, augment=True, graph=graph)
    monkeypatch.setattr(_native, "call", real)
    # the census counts host-issued calls: one per step run eagerly; with graph=True the warm-up step and the capture, a replay none
    assert count() - before == (2 if graph else 6)
    assert [s[0] for s in seen] == list(range(6)), "the hook is called once per step, after it"
    for t, (_, img, label) in enumerate(seen):
        assert (label.astype(np.int64) == labels[rows[t]].astype(np.int64)).all(), t
        assert img.dtype == np.float32 and img.shape == batches[t].shape == (8, 3, 64, 64), t
        assert (img.view(np.int32) == batches[t].view(np.int32)).all(), (t, float(np.abs(img - batches[t]).max()))
    assert [set(r) for r in hist] == host_keys, "the record is the host-fed run's"
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
    if graph:
        assert issued[0].count("spv_loader_fetch_augment_tiled") == 2, "step 0 builds the step: an eager warm-up fetch, then the capture"
        for t in range(1, 6):
            assert issued[t] == [], (t, issued[t], "a step is one replay: the host issues no library call")
    else:
        assert [names.count("spv_loader_fetch_augment_tiled") for names in issued.values()] == [1] * 6, "one fused call per step"
        for names in issued.values():
            assert not {"spv_loader_fetch", "spv_augment_params", "spv_augment_tiled_u8"} & set(names), names
