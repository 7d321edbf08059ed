"""GPU checks of the cached teacher (csrc/spv_distill.hip: spv_logit_cache_store, spv_distill_loss_idx_fwd / _bwd;
spectre_vit.distillation.TeacherLogitCache; GraphedDistillStep's cache mode; harness.train_distill(cache_teacher=True)).

The cache is an exact restructuring, so almost every comparison here is EQUALITY of bits: the stored rows against their source, the
indexed loss against the dense entry points on cache[index], the cache-mode graph step against the dense-mode step fed
cache.logits[index], a cached training run against the uncached one (with a teacher that is pure indexing, so that batching cannot
matter).  The one tolerance is the float64 oracle's, taken over from tests/test_gpu_distill.py: 2e-6 |ref| + 1e-7 on the scalars, 2e-6 of
the largest |dlogits|.  Every comparison prints its figures before it asserts (pytest -s)."""
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

MNIST = "spectre_vit/configs/spectre_vit_mnist.py"
CONSTS = [(2.0, 0.25, 0.75), (4.0, 0.5, 0.5), (1.0, 0.25, 0.75)]   # the triples of test_distill_loss_vs_oracle


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def census(name):
    from spectre_vit import _native
    return _native.call("spv_path_count", _native.PATH[name])


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """equality of every bit (torch.equal on the values would call NaN != NaN and -0.0 == 0.0)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------- store
@pytest.mark.parametrize("shape", [(3, 5, 10), (130, 257, 1000), (512, 2048, 100)], ids=lambda s: "rows{}-n{}-classes{}".format(*s))
@pytest.mark.parametrize("indexed", [True, False], ids=["shuffled", "index=None"])
def test_store_writes_the_indexed_rows_and_nothing_else(shape, indexed):
    from spectre_vit.distillation import TeacherLogitCache
    rows, n, classes = shape
    d = dev()
    g = torch.Generator().manual_seed(rows)
    src = torch.randn(rows, classes, generator=g).to(d)
    index = torch.randperm(n, generator=g)[:rows].to(d) if indexed else None   # no repeats
    cache = TeacherLogitCache(n, classes, d)
    assert cache.logits.shape == (n, classes) and torch.isnan(cache.logits).all()
    ptr = cache.logits.data_ptr()
    cache.store(index, src)
    where = index if indexed else torch.arange(rows, device=d)
    assert torch.equal(cache.logits[where], src), "the stored rows are the source rows"
    untouched = torch.ones(n, dtype=torch.bool, device=d)
    untouched[where] = False
    assert torch.isnan(cache.logits[untouched]).all(), "every other row is still NaN"
    assert cache.logits.data_ptr() == ptr and cache.complete() == (rows == n)


@pytest.mark.parametrize("shape", [(3, 5, 10), (6, 9, 100)], ids=["scalar", "vector"])
def test_store_skips_an_index_outside_the_cache(shape):
    from spectre_vit.distillation import TeacherLogitCache
    rows, n, classes = shape
    d = dev()
    src = torch.randn(rows, classes, generator=torch.Generator().manual_seed(1)).to(d)
    cache = TeacherLogitCache(n, classes, d)
    index = torch.tensor([-1, n] + [n + 7] * (rows - 2), device=d)
    cache.store(index, src)
    assert torch.isnan(cache.logits).all(), "indices -1 and n write nothing"
    index = torch.tensor([-1, 2, n] + [-(2 ** 40)] * (rows - 3), device=d)
    cache.store(index, src)
    assert torch.equal(cache.logits[2], src[1])
    cache.logits[2] = float("nan")
    assert torch.isnan(cache.logits).all(), "the neighbours of a skipped row are stored, the rest is untouched"


def test_store_with_a_misaligned_source_takes_the_scalar_path():
    """classes % 4 == 0 but the source rows start 4 bytes into an allocation: 16-byte accesses are not allowed there"""
    from spectre_vit.distillation import TeacherLogitCache
    d = dev()
    flat = torch.randn(1 + 7 * 12, generator=torch.Generator().manual_seed(2)).to(d)
    src = flat[1:].view(7, 12)
    assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    cache = TeacherLogitCache(7, 12, d)
    cache.store(None, src)
    assert torch.equal(cache.logits, src)


# ---------------------------------------------------------------- indexed loss against the dense entry points
def _inputs(rows, classes, n_cache, seed):
    g = torch.Generator().manual_seed(seed)
    d = dev()
    z = (3 * torch.randn(rows, classes, generator=g)).to(d)
    cache = (3 * torch.randn(n_cache, classes, generator=g)).to(d)
    y = torch.randint(0, classes, (rows,), generator=g).to(d)
    index = torch.randint(0, n_cache, (rows,), generator=g)
    index[0] = n_cache - 1            # the last row of the cache
    index[rows - 1] = index[1]        # a repeat
    return z, cache, index.to(d), y


def _raw(indexed, z, teacher, index, y, consts, upstream=1.7):
    """(out3, lse3, dlogits) of the forward + backward entry points themselves, on a fresh zeroed workspace; called twice, the second
    call's results must be the first's (fixed-order join, the arrival counter re-armed)"""
    from spectre_vit import _native
    from spectre_vit.hip_ops import _p, _stream
    d = z.device
    rows, C = z.shape
    T, ws, wc = consts
    work = torch.zeros(_native.call("spv_distill_loss_workspace_floats"), device=d)
    go = torch.full((1,), upstream, device=d)
    res = []
    for _ in range(2):
        lse, out, dz = torch.empty(3, rows, device=d), torch.empty(3, device=d), torch.empty(rows, C, device=d)
        if indexed:
            _native.call("spv_distill_loss_idx_fwd", _p(z), _p(teacher), _p(index), _p(y), _p(lse), _p(out), _p(work), rows, teacher.shape[0],
                         C, T, ws, wc, _stream())
            _native.call("spv_distill_loss_idx_bwd", _p(z), _p(teacher), _p(index), _p(y), _p(lse), _p(go), _p(dz), rows, teacher.shape[0], C,
                         T, ws, wc, _stream())
        else:
            _native.call("spv_distill_loss_fwd", _p(z), _p(teacher), _p(y), _p(lse), _p(out), _p(work), rows, C, T, ws, wc, _stream())
            _native.call("spv_distill_loss_bwd", _p(z), _p(teacher), _p(y), _p(lse), _p(go), _p(dz), rows, C, T, ws, wc, _stream())
        res.append((out, lse, dz))
    for a, b in zip(*res):
        assert same_bits(a, b), "two calls give the same bits"
    return res[0]


@pytest.mark.parametrize("shape", [(3, 10), (130, 1000), (512, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n_kind", ["n1", "rows+1", "n2048"])
@pytest.mark.parametrize("consts", CONSTS, ids=lambda c: f"T{c[0]:g}-{c[1]:g}-{c[2]:g}")
def test_indexed_loss_equals_the_dense_loss_on_the_gathered_rows(shape, n_kind, consts):
    rows, classes = shape
    n_cache = {"n1": 1, "rows+1": rows + 1, "n2048": 2048}[n_kind]
    z, cache, index, y = _inputs(rows, classes, n_cache, seed=rows + classes + n_cache)
    assert int(index.max()) == n_cache - 1 and (n_cache == 1 or len(set(index.tolist())) < rows)
    before = census("distill_cached")
    got = _raw(True, z, cache, index, y, consts)
    assert census("distill_cached") == before + 2, "one per indexed forward launch"
    want = _raw(False, z, cache[index].contiguous(), None, y, consts)
    assert census("distill_cached") == before + 2, "the dense entry point is not counted"
    for name, a, b in zip(("out3", "lse3", "dlogits"), got, want):
        differing = int((bits(a) != bits(b)).sum())
        print(f"{shape} n_cache={n_cache} {consts}: {name}: {differing} of {a.numel()} elements differ from the dense entry point")
        assert torch.equal(a, b) and differing == 0, name
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all()


def test_indexed_loss_vs_the_float64_oracle():
    from oracle import spectre_oracle as O
    from spectre_vit import hip_ops
    rows, classes, n_cache = 130, 1000, 257
    T, ws, wc = CONSTS[0]
    upstream = 1.7
    z, cache, index, y = _inputs(rows, classes, n_cache, seed=5)
    zt = z.clone().requires_grad_(True)
    loss, soft, ce = hip_ops.distill_loss_cached(zt, cache, index, y, T, ws, wc)
    assert loss.requires_grad and not soft.requires_grad and not ce.requires_grad
    (loss * upstream).backward()
    t = cache[index].cpu().numpy().astype(np.float64)
    rl, rdz, rs, rc = O.distill_loss_fwd_bwd(z.cpu().numpy().astype(np.float64), t, y.cpu().numpy(), np.float64(T), np.float64(ws), np.float64(wc))
    for name, g, r in zip(("loss", "soft", "ce"), (loss.item(), soft.item(), ce.item()), (float(rl), float(rs), float(rc))):
        tol = 2e-6 * abs(r) + 1e-7
        print(f"indexed {rows}x{classes}: {name} kernel {g:.9g} float64 {r:.9g} |diff| {abs(g - r):.3e} allowed {tol:.3e}")
        assert abs(g - r) <= tol, (name, g, r)
    ref = np.asarray(rdz) * upstream
    err, scale = float(np.abs(zt.grad.cpu().numpy() - ref).max()), float(np.abs(ref).max())
    print(f"indexed {rows}x{classes}: dlogits max |diff| {err:.3e} = {err / scale:.3e} of the largest magnitude (allowed 2e-6)")
    assert err <= 2e-6 * scale


@pytest.mark.parametrize("shape", [(6, 10), (130, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_an_index_outside_the_cache_poisons_its_row_and_reads_nothing(shape):
    rows, classes = shape
    n_cache = rows + 1
    z, cache, index, y = _inputs(rows, classes, n_cache, seed=11)
    bad = [1, rows - 2]
    clean = index.clone()
    index[bad[0]], index[bad[1]] = -1, n_cache
    got = _raw(True, z, cache, index, y, CONSTS[0])
    want = _raw(False, z, cache[clean].contiguous(), None, y, CONSTS[0])
    out, lse, dz = got
    print(f"bad index {shape}: out3 {out.tolist()}  dense out3 {want[0].tolist()}")
    assert torch.isnan(out[0]) and torch.isnan(out[1])
    assert same_bits(out[2], want[0][2]), "the cross-entropy is still the true value"
    good = [r for r in range(rows) if r not in bad]
    assert torch.isnan(lse[2][bad]).all() and same_bits(lse[2][good], want[1][2][good])
    assert same_bits(lse[:2], want[1][:2]), "the student's log-sum-exps are the true ones"
    assert torch.isnan(dz[bad]).all(), "those rows of dlogits are NaN"
    assert same_bits(dz[good], want[2][good]), "every other row equals the dense result"


def test_an_unfilled_cache_row_poisons_the_loss_and_bad_arguments_are_refused():
    from spectre_vit import hip_ops
    from spectre_vit.distillation import DistillationLoss, TeacherLogitCache
    d = dev()
    z, filled, index, y = _inputs(8, 10, 9, seed=3)
    cache = TeacherLogitCache(9, 10, d)
    keep = [r for r in range(9) if r != int(index[4])]
    cache.store(torch.tensor(keep, device=d), filled[keep])
    crit = DistillationLoss()
    zt = z.clone().requires_grad_(True)
    loss = crit(zt, cache, y, index=index)          # a TeacherLogitCache ...
    loss.backward()
    assert torch.isnan(loss) and torch.isnan(crit.soft) and torch.isfinite(crit.ce)
    hit = index == index[4]
    assert torch.isnan(zt.grad[hit]).all() and torch.isfinite(zt.grad[~hit]).all()
    cache.store(index[4:5], filled[index[4:5]])
    assert cache.complete()
    a = crit(z, cache, y, index=index)
    b = crit(z, cache.logits, y, index=index)       # ... or its matrix
    c = crit(z, filled[index], y)
    assert same_bits(a, b) and same_bits(a, c) and torch.isfinite(a)
    for bad in ((z.bfloat16(), filled, index, y), (z, filled.double(), index, y), (z, filled[:, :5], index, y), (z, filled, index.int(), y),
                (z, filled, index[:3], y), (z, filled, index, y.int()), (z, filled.t().contiguous().t(), index, y)):
        with pytest.raises(ValueError, match="distill_loss_cached"):
            hip_ops.distill_loss_cached(*bad)


# ---------------------------------------------------------------- GraphedDistillStep in cache mode
def _mnist_student():
    from spectre_vit import harness
    from spectre_vit.configs.parser import parse_config
    torch.manual_seed(11)
    return harness.build_model(parse_config(MNIST), "fft", dev()).train()


def test_graphed_step_in_cache_mode_equals_the_dense_mode_step_on_the_gathered_logits():
    from spectre_vit.distillation import DistillationLoss, TeacherLogitCache
    from spectre_vit.graph import GraphedDistillStep
    from spectre_vit.optim import FusedAdamW
    d = dev()
    steps, B, n = 5, 8, 40
    g = torch.Generator().manual_seed(3)
    imgs = [torch.randn(B, 3, 28, 28, generator=g).to(d) for _ in range(steps)]
    labels = [torch.randint(0, 100, (B,), generator=g).to(d) for _ in range(steps)]
    index = [torch.randint(0, n, (B,), generator=g).to(d) for _ in range(steps)]
    cache = TeacherLogitCache(n, 100, d)
    cache.store(None, (3 * torch.randn(n, 100, generator=g)).to(d))

    def run(cached):
        m = _mnist_student()
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True)
        crit = DistillationLoss()
        before = census("distill_cached")
        if cached:
            step = GraphedDistillStep(m, opt, crit, imgs[0], labels[0], teacher_cache=cache, example_index=index[0], warmup=1)
        else:
            step = GraphedDistillStep(m, opt, crit, imgs[0], labels[0], cache.logits[index[0]], warmup=1)
        try:
            built = census("distill_cached") - before
            rec = [(step.warm_loss.item(), step.warm_soft.item(), step.warm_ce.item())]   # the warm-up step WAS step 0
            for k in range(1, steps):
                loss = step(imgs[k], labels[k], index=index[k]) if cached else step(imgs[k], labels[k], cache.logits[index[k]])
                rec.append((loss.item(), step.soft.item(), step.ce.item()))
            assert step.replays == steps - 1
            if cached:
                assert step.index.dtype == torch.int64 and torch.equal(step.index, index[-1]) and step.teacher_logits is None
                with pytest.raises(ValueError, match="index="):
                    step(imgs[0], labels[0], cache.logits[index[0]])
            else:
                with pytest.raises(ValueError, match="teacher_cache"):
                    step(imgs[0], labels[0], index=index[0])
            replayed = census("distill_cached") - before - built
        finally:
            step.close()
        return rec, {k: v.detach().clone() for k, v in m.state_dict().items()}, built, replayed

    dense, w_dense, built_d, replayed_d = run(False)
    cached, w_cached, built_c, replayed_c = run(True)
    for k, (a, b) in enumerate(zip(dense, cached)):
        print(f"step {k}: dense-mode (loss, soft, ce) {a}  cache-mode {b}")
    assert dense == cached, "loss, soft and ce of every step, bit for bit"
    assert all(math.isfinite(v) for r in cached for v in r) and cached[0] != cached[-1]
    differing = [k for k in w_dense if not same_bits(w_dense[k], w_cached[k])]
    assert not differing, differing
    # the census counts host launches: one cached forward per step the host issued (the warm-up step and the captured one); a replay
    # is the graph's launch.  The dense-mode step never takes the slot.
    assert (built_c, replayed_c) == (2, 0) and (built_d, replayed_d) == (0, 0)


# ---------------------------------------------------------------- harness.train_distill
class ProbeTeacher(torch.nn.Module):
    """logits = fixed elements of the flattened 224 view times a constant: pure indexing, no reduction, so a sample's logits do not
    depend on the batch it arrives in"""

    def __init__(self, classes, in_channels, crop=224):
        super().__init__()
        g = torch.Generator().manual_seed(17)
        self.register_buffer("pick", torch.randint(0, in_channels * crop * crop, (classes,), generator=g))
        self.calls = 0

    def forward(self, x, return_features=False):
        self.calls += 1
        logits = x.flatten(1)[:, self.pick] * 1.5
        return (logits, logits) if return_features else logits


def _train(tmp_path, tag, teacher, **kw):
    from spectre_vit.harness import train_distill
    kinds = []
    out = str(tmp_path / tag)
    model, hist = train_distill(MNIST, mixer="fft", out_dir=out, log=lambda r: None, batch_hook=lambda kind, *a: kinds.append(kind),
                                epochs=2, steps_per_epoch=4, batch_size=64, n_train=256, n_val=64, teacher=teacher, **kw)
    lines = [json.loads(l) for l in open(os.path.join(out, "scalars.jsonl"))]
    batch = [(l["step"], l["Batch Loss/Train"], l["Batch Loss/Dist"], l["Batch Loss/CE"]) for l in lines if "Batch Loss/Train" in l]
    weights = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return dict(batch=batch, weights=weights, hist=hist, lines=lines, kinds=kinds)


def _differing(a, b):
    return [k for k in a["weights"] if not same_bits(a["weights"][k], b["weights"][k])]


def test_train_distill_cached_equals_uncached_bit_for_bit(tmp_path):
    d = dev()
    probe = lambda: ProbeTeacher(100, 3).to(d).eval()
    # the project's own determinism claim first: two uncached runs agree
    u1 = _train(tmp_path, "u1", probe())
    u2 = _train(tmp_path, "u2", probe())
    print("uncached per-batch (step, Train, Dist, CE):", u1["batch"])
    assert len(u1["batch"]) == 8 and all(math.isfinite(v) for r in u1["batch"] for v in r[1:])
    assert u1["batch"] == u2["batch"] and not _differing(u1, u2), "two uncached runs agree on every per-batch scalar and final weight"
    assert u1["kinds"].count("teacher") == 8 and "teacher_fill" not in u1["kinds"]

    before = census("distill_cached"), census("teacher_view")
    t = probe()
    c = _train(tmp_path, "c", t, cache_teacher=True)
    print("cached   per-batch (step, Train, Dist, CE):", c["batch"])
    assert c["batch"] == u1["batch"], "every per-batch scalar, bit for bit"
    assert not _differing(c, u1), "every final weight, bit for bit"
    assert t.calls == 4 and c["kinds"].count("teacher_fill") == 4 and "teacher" not in c["kinds"] and c["kinds"].count("train") == 8
    assert (census("distill_cached") - before[0], census("teacher_view") - before[1]) == (8, 4), "one cached forward per step, one view per fill batch"
    rec = [l["TeacherCache"] for l in c["lines"] if "TeacherCache" in l]
    assert len(rec) == 1 and rec[0]["rows"] == 256 and rec[0]["teacher_batches"] == 4 and rec[0]["loaded"] is False and rec[0]["seconds"] > 0
    assert c["lines"].index({"TeacherCache": rec[0]}) == 0, "logged before epoch 0"

    gu = _train(tmp_path, "gu", probe(), graph=True)
    t = probe()
    gc = _train(tmp_path, "gc", t, graph=True, cache_teacher=True)
    print("graph uncached:", gu["batch"])
    print("graph cached:  ", gc["batch"])
    assert gc["batch"] == gu["batch"] and not _differing(gc, gu), "graph=True: cached equals uncached, bit for bit"
    assert t.calls == 4 and "teacher" not in gc["kinds"]


def test_train_distill_with_the_synthetic_teacher_calls_it_once_per_fill_batch_and_reloads_the_file(tmp_path):
    from spectre_vit.distillation import SyntheticTeacher, TeacherLogitCache
    d = dev()
    path = str(tmp_path / "teacher_logits.pt")
    runs = []
    for tag in ("fill", "reload"):
        teacher = SyntheticTeacher(100, 384, 3).to(d)
        calls = []
        teacher.register_forward_hook(lambda mod, args, out: calls.append(args[0].shape[0]))
        views = census("teacher_view")
        r = _train(tmp_path, tag, teacher, cache_teacher=True, teacher_cache_path=path)
        r["calls"], r["views"] = calls, census("teacher_view") - views
        r["record"] = [l["TeacherCache"] for l in r["lines"] if "TeacherCache" in l]
        runs.append(r)
    fill, reload = runs
    batches = math.ceil(256 / 64)
    # a teacher call inside the epochs would make the list longer than the fill's batches
    assert fill["calls"] == [64] * batches and fill["views"] == batches and fill["kinds"].count("teacher_fill") == batches
    assert fill["record"] == [dict(fill["record"][0], rows=256, teacher_batches=batches, loaded=False)]
    saved = TeacherLogitCache.load(path, d, n=256, classes=100, resize=256, crop=224, tag="DinoClassifier")   # raises if a row holds NaN
    assert saved.complete() and saved.logits.shape == (256, 100)
    assert reload["calls"] == [] and reload["views"] == 0 and "teacher_fill" not in reload["kinds"]
    assert reload["record"] == [dict(reload["record"][0], rows=256, teacher_batches=0, loaded=True)]
    assert reload["batch"] == fill["batch"] and not _differing(reload, fill), "the loaded logits are the filled ones"
    with pytest.raises(ValueError, match="crop="):
        _train(tmp_path, "other_view", SyntheticTeacher(100, 384, 3).to(d), cache_teacher=True, teacher_cache_path=path, crop=192)


# ---------------------------------------------------------------- two ranks
N_DP, BATCH_DP = 150, 32   # five blocks, the last one short: rank 0 computes three, rank 1 two


def _fill(rank, world, hook=None):
    from spectre_vit.distillation import TeacherLogitCache, TeacherView
    d = torch.device("cuda:0")
    images = torch.randint(0, 256, (N_DP, 28, 28, 1), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).to(d)
    cache = TeacherLogitCache(N_DP, 10, d)
    calls = cache.fill(ProbeTeacher(10, 1).to(d).eval(), TeacherView((0.5,), (0.25,)), images, batch_size=BATCH_DP, rank=rank, world=world,
                       batch_hook=hook)
    return cache, calls


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fill_worker(rank, world, port, outdir):
    import torch.distributed as dist
    sys.path.insert(0, PKG)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    blocks = []
    cache, calls = _fill(rank, world, hook=lambda kind, k, img, idx: blocks.append((kind, k, idx.tolist())))
    torch.save(dict(logits=cache.logits.cpu(), calls=calls, blocks=blocks, complete=cache.complete()), os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_fill_the_same_bits_as_one(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_fill_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(2))
    single, calls = _fill(0, 1)
    assert calls == 5 and single.complete()
    assert (r0["calls"], r1["calls"]) == (3, 2) and r0["complete"] and r1["complete"]
    seen = sorted(i for r in (r0, r1) for _, _, idx in r["blocks"] for i in idx)
    assert seen == list(range(N_DP)), "every row is computed by exactly one rank"
    assert [k for _, k, _ in r0["blocks"]] == [0, 2, 4] and [k for _, k, _ in r1["blocks"]] == [1, 3]
    for r in (r0, r1):
        assert same_bits(r["logits"], single.logits.cpu()), "both ranks hold the single-rank fill's bits"
