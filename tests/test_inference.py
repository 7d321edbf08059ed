"""CPU-side checks of spectre_vit.inference (no GPU compute): the float64 metrics reference (tests/eval_ref.py) against torch and against
the tie / ignore rules themselves, the bucket choice and chunk plan, the refusals, the --graph-eval flag and the exported symbol."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_ref as R
from spectre_vit import inference as I

TINY = dict(img_size=8, patch_size=4, in_channels=3, num_classes=8, embed_dim=16, num_encoders=1, num_heads=2, hidden_dim=24, dropout=0.0)


@pytest.mark.parametrize("rows,C,seed", [(37, 100, 0), (64, 1000, 1)])
def test_eval_ref_matches_torch(rows, C, seed):
    """argmax, topk and F.cross_entropy(reduction="sum") in float64 on seeded fp32 normal logits.  topk's order among tied values is
    unspecified, so the comparison needs rows without ties: asserted first (fp32 normals satisfy it; bf16-rounded ones would not)."""
    g = torch.Generator().manual_seed(seed)
    z32 = torch.randn(rows, C, generator=g, dtype=torch.float32)
    labels = torch.randint(0, C, (rows,), generator=g)
    for r in range(rows):
        assert np.unique(z32[r].numpy()).size == C, f"row {r} holds tied values"
    z = z32.double()
    k = 5
    pred, st = R.eval_head(z.numpy(), labels.numpy(), rows, k)
    assert np.array_equal(pred, torch.argmax(z, dim=1).numpy())
    top = torch.topk(z, k, dim=1).indices
    assert st["seen"] == rows
    assert st["top1"] == int((torch.argmax(z, dim=1) == labels).sum())
    assert st["topk"] == int((top == labels[:, None]).any(dim=1).sum())
    ref = F.cross_entropy(z, labels, reduction="sum").item()
    assert abs(st["loss_sum"] - ref) <= 1e-12 * abs(ref)
    # accumulation: a second batch adds to the first
    _, st2 = R.eval_head(z.numpy(), labels.numpy(), rows, k, st)
    assert st2["seen"] == 2 * rows and st2["topk"] == 2 * st["topk"] and abs(st2["loss_sum"] - 2 * ref) <= 1e-12 * abs(ref)
    assert st["seen"] == rows   # the argument is not modified


def test_tie_rules():
    C = 10
    flat = np.zeros((C, C))   # all-equal rows, one per label
    labels = np.arange(C)
    for k in (1, 2, 5, 8):
        pred, st = R.eval_head(flat, labels, C, k)
        assert (pred == 0).all()
        assert st["topk"] == k and st["top1"] == 1   # a hit iff y < k; top-1 only for y = 0
        for y in range(C):
            assert R.topk_hit(flat[y], y, k) == (y < k)
    row = np.linspace(-1.0, 0.0, C)
    row[3] = row[7] = 2.0   # the maximum, twice
    z = row[None]
    pred, st1 = R.eval_head(z, [7], 1, 1)
    assert pred[0] == 3 and st1["top1"] == 0 and st1["topk"] == 0     # label 7: a top-1 miss ...
    _, st2 = R.eval_head(z, [7], 1, 2)
    assert st2["top1"] == 0 and st2["topk"] == 1                      # ... and a top-2 hit
    _, st3 = R.eval_head(z, [3], 1, 1)
    assert st3["top1"] == 1 and st3["topk"] == 1
    # k = 1 is exactly pred == y, ties or not
    rng = np.random.default_rng(0)
    zt = rng.integers(0, 3, (200, 6)).astype(np.float64)
    yt = rng.integers(0, 6, 200)
    pred, st = R.eval_head(zt, yt, 200, 1)
    assert st["topk"] == st["top1"] == int((pred == yt).sum())


def test_ignore_rules():
    rng = np.random.default_rng(1)
    z = rng.standard_normal((12, 7))
    labels = np.array([0, -1, 3, 7, 6, 100, 2, -5, 1, 1, 4, 5])
    pred, st = R.eval_head(z, labels, 9, 3)   # rows 9.. are padding
    counted = [r for r in range(9) if 0 <= labels[r] < 7]
    assert counted == [0, 2, 4, 6, 8]
    assert st["seen"] == len(counted)
    assert pred.shape == (12,) and np.array_equal(pred, z.argmax(1))   # every row is predicted, counted or not
    assert abs(st["loss_sum"] - sum(R.row_loss(z[r], labels[r]) for r in counted)) < 1e-12
    assert st["top1"] == sum(int(pred[r] == labels[r]) for r in counted)
    _, none = R.eval_head(z, np.full(12, -1), 12, 3)
    assert none == R.new_stats()
    _, zero = R.eval_head(z, labels, 0, 3)
    assert zero == R.new_stats()


def test_bucket_choice_and_chunk_plan():
    want = {1: [(0, 1, 1)], 2: [(0, 2, 8)], 8: [(0, 8, 8)], 9: [(0, 9, 64)], 64: [(0, 64, 64)], 65: [(0, 65, 512)],
            512: [(0, 512, 512)], 513: [(0, 512, 512), (512, 1, 1)], 1100: [(0, 512, 512), (512, 512, 512), (1024, 76, 512)]}
    for B, plan in want.items():
        assert I.chunk_plan(B) == plan, B
        assert I.chunk_plan(B, I.DEFAULT_BUCKETS) == plan
        assert sum(p[1] for p in plan) == B and all(p[1] <= p[2] for p in plan)
        assert I.pick_bucket(min(B, 512)) == plan[0][2]
    with pytest.raises(ValueError):
        I.chunk_plan(0)
    with pytest.raises(ValueError):
        I.pick_bucket(0)
    assert I.normalize_buckets((64, 8, 8, 1)) == (1, 8, 64)
    with pytest.raises(ValueError):
        I.normalize_buckets(())
    # the baseline ViT attends across the batch axis: only batches that fill their buckets
    assert I.chunk_plan(64, exact=True) == [(0, 64, 64)]
    assert I.chunk_plan(1024, exact=True) == [(0, 512, 512), (512, 512, 512)]
    for B in (2, 9, 65, 1100):
        with pytest.raises(ValueError, match="batch axis"):
            I.chunk_plan(B, exact=True)
    # the harness's validation buckets: the batch size, and the tail rounded up to a multiple of 8
    assert I.eval_buckets(1024, 512) == (512,)
    assert I.eval_buckets(1000, 512) == (488, 512)
    assert I.eval_buckets(1001, 512) == (496, 512)
    assert I.eval_buckets(100, 512) == (100,)
    assert I.eval_buckets(1029, 512) == (8, 512)


def test_cpu_model_raises():
    from spectre_vit.models.spectre.spectre import SpectreViT
    m = SpectreViT(**TINY, mixer="fft")
    with pytest.raises(RuntimeError, match="GPU"):
        I.InferenceSession(m)


def test_argument_refusals_come_before_the_device_check():
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.models.vit.vit import ViT
    m = SpectreViT(**TINY, mixer="fft")
    with pytest.raises(TypeError):
        I.InferenceSession(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError):
        I.InferenceSession(m, topk=9)
    with pytest.raises(ValueError):
        I.InferenceSession(m, input="int8")
    with pytest.raises(ValueError, match="uint8"):
        I.InferenceSession(ViT(**TINY), input="uint8")


def test_derived_stats():
    d = I.derive_stats(8, 2, 6, 12.0)
    assert d == {"seen": 8, "top1": 2, "topk": 6, "loss_sum": 12.0, "accuracy": 0.25, "topk_accuracy": 0.75, "loss": 1.5}
    assert I.derive_stats(0, 0, 0, 0.0)["accuracy"] == 0.0


def test_parsers_accept_the_new_flags():
    from spectre_vit import harness
    a = harness.build_parser().parse_args(["--graph-eval", "--graph", "--epochs", "2"])
    assert a.graph_eval and a.graph and a.epochs == 2
    assert not harness.build_parser().parse_args([]).graph_eval
    b = I.build_parser().parse_args(["--checkpoint", "model_best.pt", "--mixer", "fft"])
    assert b.checkpoint == "model_best.pt" and b.batch == 512 and b.n == 10000


def test_library_exports_eval_head():
    from spectre_vit import _native
    lib = _native.load()
    assert hasattr(lib, "spv_eval_head") and hasattr(lib, "spv_eval_head_stats_words")
    assert lib.spv_eval_head_stats_words() >= 4
