"""GPU checks of spectre_vit.inference: the metrics kernel (spv_eval_head) against the float64 reference of tests/eval_ref.py, the
graph-replayed session against the eager eval forward bit for bit (and, through it, against the float64 oracle at the bars of
tests/test_gpu_model.py), padding, the frozen-weights rule, chunking, uint8 input, memory, and the harness's graph_eval mode.

Loss bound: 2e-6 * |ref| + 1e-7, the project's cross-entropy bound (test_cross_entropy_vs_torch_and_oracle, restated in the header
of tests/test_gpu_distill.py)."""
import gc
import os

import numpy as np
import pytest
import torch

import eval_ref as R
from conftest import load_model_fixture
from oracle import spectre_oracle as O
from test_gpu_model import BF16_L2, check_l2
from test_gpu_ops import check, dev, t

pytestmark = pytest.mark.gpu

MIXERS = ("permut", "fft", "dwt_embed", "dwt_token", "attention")
DTYPES = [torch.float32, torch.bfloat16]


def loss_close(got, ref):
    return abs(got - ref) <= 2e-6 * abs(ref) + 1e-7


def read_stats(stats):
    w = stats[:4].cpu()
    return {"seen": int(w[0]), "top1": int(w[1]), "topk": int(w[2]), "loss_sum": float(w[3:4].view(torch.float64)[0])}


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C", [(1, 10), (37, 100), (512, 100), (64, 1000)])
def test_eval_head_vs_reference(rows, C, dtype):
    """pred and the three counts exact, loss_sum within the cross-entropy bound, over three accumulating calls; labels include -1 and
    values >= C; n_valid < rows (and, in the last call, == rows); bf16 logits are seen by the reference as rounded, so their ties
    must follow the rule; the whole sequence repeated gives the same bits."""
    from spectre_vit import hip_ops
    k = 5
    g = torch.Generator().manual_seed(rows * 1000 + C)
    calls = []
    for i, nv in enumerate((rows - max(1, rows // 4), rows - 1, rows)):
        z = torch.randn(rows, C, generator=g).to(dtype)
        y = torch.randint(-1, C + 2, (rows,), generator=g)
        if rows > 4:
            y[1], y[2] = -1, C
        if i == 0 and C >= 8:   # a built-in tie at the top: columns 3 and 7 share the row maximum, label 7
            z[0, 3] = z[0, 7] = 30.0
            y[0] = 7
        calls.append((z, y, nv))
    ties = sum(int(np.unique(z[r].float().numpy()).size < C) for z, _, _ in calls for r in range(rows))
    print(f"rows with tied values ({dtype}, {rows} x {C}): {ties} of {3 * rows}")

    def run():
        stats = hip_ops.eval_head_stats(dev())
        n_valid = torch.zeros(1, dtype=torch.int32, device=dev())
        snaps = []
        for z, y, nv in calls:
            pred = torch.full((rows,), -7, dtype=torch.int64, device=dev())
            n_valid.fill_(nv)
            hip_ops.eval_head(z.to(dev()), y.to(dev()), n_valid, pred, stats, k)
            snaps.append((pred.cpu().numpy(), read_stats(stats), stats[:4].clone()))
        return snaps

    first, second = run(), run()
    ref = R.new_stats()
    for (z, y, nv), (pred, st, _) in zip(calls, first):
        pred_ref, ref = R.eval_head(z.float().numpy(), y.numpy(), nv, k, ref)
        assert np.array_equal(pred, pred_ref)
        print(f"stats {st}  reference {ref}  loss rel err {abs(st['loss_sum'] - ref['loss_sum']) / max(abs(ref['loss_sum']), 1e-30):.2e}")
        assert (st["seen"], st["top1"], st["topk"]) == (ref["seen"], ref["top1"], ref["topk"])
        assert loss_close(st["loss_sum"], ref["loss_sum"]), (st, ref)
    for a, b in zip(first, second):
        assert np.array_equal(a[0], b[0]) and torch.equal(a[2], b[2]), "the same calls must give the same bits"


def test_eval_head_k1_is_pred_equals_label_and_refusals():
    from spectre_vit import hip_ops
    g = torch.Generator().manual_seed(3)
    z = torch.randint(0, 3, (300, 6), generator=g).float()   # ties everywhere
    y = torch.randint(0, 6, (300,), generator=g)
    stats = hip_ops.eval_head_stats(dev())
    pred = torch.zeros(300, dtype=torch.int64, device=dev())
    nv = torch.full((1,), 300, dtype=torch.int32, device=dev())
    hip_ops.eval_head(z.to(dev()), y.to(dev()), nv, pred, stats, 1)
    st = read_stats(stats)
    _, ref = R.eval_head(z.numpy(), y.numpy(), 300, 1)
    assert st["top1"] == st["topk"] == ref["top1"] == int((pred.cpu() == y).sum()) and st["seen"] == 300
    with pytest.raises(RuntimeError, match="k="):
        hip_ops.eval_head(z.to(dev()), y.to(dev()), nv, pred, stats, 9)
    with pytest.raises(ValueError):
        hip_ops.eval_head(z.to(dev()), y.to(dev()).int(), nv, pred, stats, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# models from the golden fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
def fixture_model(mixer, name="model_small_cut"):
    """SpectreViT(mixer) with the fixture's weights: strictly for the fixture's own mixer (permut); the other mixers take every tensor
    they share with it (embedding, feed-forward halves, norms, head) and keep their seeded own ones (attention's projections)"""
    from spectre_vit.models.spectre.spectre import SpectreViT
    d, cfg = load_model_fixture(name)
    sd = {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}
    torch.manual_seed(42)
    m = SpectreViT(**cfg, mixer=mixer).to(dev())
    if mixer == "permut":
        m.load_state_dict(sd, strict=True)
    else:
        own = m.state_dict()
        shared = {k: v for k, v in sd.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}
        assert len(shared) >= len(own) - 4 * cfg["num_encoders"], (len(shared), len(own))
        m.load_state_dict(shared, strict=False)
    return m.eval(), cfg, t(d["img"]), torch.from_numpy(d["labels"]).to(dev())


def eager(m, img, dtype, **kw):
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        return m(img, **kw)


def oracle_logits(m, cfg, img, mixer):
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    params = O.params_from_state_dict(sd, cfg["num_encoders"], mixer, np.float64)
    for i, lp in enumerate(params["layers"]):
        lp["dwt_levels"] = 1
        if mixer == "attention":
            from test_gpu_attention_mixer import MIX
            pre = f"encoder_blocks.layers.{i}.mix_layer."
            lp["mix_layer"] = {o: np.asarray(sd[pre + s], np.float64) for o, s in MIX}
            lp["heads"] = cfg["num_heads"]
    return O.spectre_vit_fwd(img.cpu().numpy().astype(np.float64), params, cfg["patch_size"], mixer)[0]


def sess(m, dtype, **kw):
    from spectre_vit.inference import InferenceSession
    return InferenceSession(m, autocast_dtype=torch.bfloat16 if dtype == torch.bfloat16 else None, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. session against eager, bitwise
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mixer", MIXERS)
def test_session_equals_eager_spectre_vit(mixer, dtype, monkeypatch):
    """the same kernels in the same order (the property test_graphed_train_step_matches_eager_steps relies on): bitwise equal logits at
    a batch equal to a bucket; those logits within test_gpu_model.py's bars of the float64 oracle (fp32 2e-4 max-norm, bf16 2.5e-2
    relative L2)"""
    if mixer == "attention":
        from test_gpu_attention_mixer import _route_attention
        _route_attention(monkeypatch)
    m, cfg, img, labels = fixture_model(mixer)
    want, want_cls = eager(m, img, dtype, return_features=True)
    with sess(m, dtype, batch_sizes=(img.shape[0],), return_features=True) as s:
        got = s(img)
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got, want), (got - want).abs().max().item()
        assert torch.equal(s.features, want_cls)
        assert torch.equal(s(img), want)   # a second replay
        assert torch.equal(s.predict(img), torch.argmax(want, dim=1))
        s.reset_stats()
        s.accumulate(img, labels)
        st = s.stats()
        _, ref = R.eval_head(want.cpu().numpy(), labels.cpu().numpy(), img.shape[0], 5)
        assert (st["seen"], st["top1"], st["topk"]) == (ref["seen"], ref["top1"], ref["topk"]) and loss_close(st["loss_sum"], ref["loss_sum"])
        got = got.clone()
    ref_logits = oracle_logits(m, cfg, img, mixer)
    if dtype == torch.float32:
        check(got, ref_logits, 2e-4, "logits vs float64")
    else:
        check_l2(got, ref_logits, BF16_L2, "logits vs float64")


@pytest.mark.parametrize("dtype", DTYPES)
def test_session_equals_eager_spectre_branch(dtype):
    """SpectreBranch with the golden fixture's weights (the reference's same-seed initialisation) and image: bitwise the eager eval
    forward; within test_gpu_spectre_branch.py's bars of the reference's own logits (fp32 5e-5, bf16 2.5e-2 relative L2)"""
    from test_gpu_spectre_branch import build
    d = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "model_spectre_branch.npz")))
    m = build(int(d["cfg.seed"])).eval()
    img = t(d["img"])
    want = eager(m, img, dtype)
    with sess(m, dtype, batch_sizes=(img.shape[0],)) as s:
        got = s(img)
        assert torch.equal(got, want), (got - want).abs().max().item()
        got = got.clone()
    if dtype == torch.float32:
        check(got, d["logits"], 5e-5, "logits vs the reference")
    else:
        check_l2(got, d["logits"], BF16_L2, "logits vs the reference")
    with pytest.raises(ValueError, match="uint8"):
        sess(m, dtype, input="uint8")


def test_vit_only_at_exact_buckets():
    from spectre_vit.models.vit.vit import ViT
    torch.manual_seed(0)
    m = ViT(img_size=8, patch_size=4, in_channels=3, num_classes=8, embed_dim=16, num_encoders=2, num_heads=4, hidden_dim=24,
            dropout=0.0).to(dev()).eval()
    x = torch.randn(8, 3, 8, 8, device=dev())
    with sess(m, torch.float32, batch_sizes=(8,)) as s:
        assert torch.equal(s(x), eager(m, x, torch.float32))
        with pytest.raises(ValueError, match="batch axis"):
            s(x[:5])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. padding
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixer", ["fft", "permut"])
def test_padding_rows_do_not_reach_the_valid_rows(mixer):
    m, cfg, _, _ = fixture_model(mixer)
    g = torch.Generator().manual_seed(11)
    shape = (3, cfg["img_size"], cfg["img_size"])
    img = torch.randn(37, *shape, generator=g).to(dev())
    other = torch.randn(37, *shape, generator=g).to(dev())
    pad_a = torch.randn(27, *shape, generator=g).to(dev())
    pad_b = torch.randn(27, *shape, generator=g).to(dev()) * 5.0
    labels = torch.randint(0, cfg["num_classes"], (37,), generator=g).to(dev())
    dtype = torch.bfloat16
    with sess(m, dtype, batch_sizes=(64,)) as s:
        s(torch.cat([other, pad_a]))           # the pad rows of the static buffer now hold pad_a
        out_a = s(img).clone()
        assert out_a.shape == (37, cfg["num_classes"])
        assert torch.equal(out_a, eager(m, torch.cat([img, pad_a]), dtype)[:37])
        s(torch.cat([other, pad_b]))           # other data in the pad rows
        assert torch.equal(s(img), out_a), "rows [:37] must not depend on the pad rows"
        s.reset_stats()
        s.accumulate(img, labels)
        st = s.stats()
        assert st["seen"] == 37
        _, ref = R.eval_head(out_a.cpu().numpy(), labels.cpu().numpy(), 37, 5)
        assert (st["top1"], st["topk"]) == (ref["top1"], ref["topk"]) and loss_close(st["loss_sum"], ref["loss_sum"])
        s(img)                                 # __call__ counts nothing
        assert s.stats()["seen"] == 37


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. frozen weights
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixer", ["fft", "permut", "attention"])
def test_outputs_change_only_at_refresh(mixer):
    """a test of values: after an optimizer step, a replaced weight-copy cache (as GraphedTrainStep._warm does), a collection and fresh
    allocations over whatever was freed, the session still returns its old output bit for bit; after refresh() the new weights'"""
    from spectre_vit import shadows
    m, cfg, img, labels = fixture_model(mixer)
    dtype = torch.bfloat16
    eager(m, img, dtype)   # (the eager cache holds copies of the weights, as in a run that validated eagerly before)
    s = sess(m, dtype, batch_sizes=(img.shape[0],))
    old = s(img).clone()
    assert torch.equal(old, eager(m, img, dtype))
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=5e-2)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = torch.nn.functional.cross_entropy(m(img), labels)
    loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    shadows.reset_shadow_cache()
    gc.collect()
    total = sum(p.numel() for p in m.parameters())
    junk = [torch.full((total,), 1e4, device=dev()) for _ in range(3)] + [torch.full((total,), 1e4, device=dev(), dtype=torch.bfloat16)
                                                                          for _ in range(4)]
    torch.cuda.synchronize()
    new = eager(m, img, dtype)
    assert not torch.equal(new, old), "the optimizer step must have changed the model's output"
    assert torch.equal(s(img), old), "a session's outputs change only at refresh()"
    s.refresh()
    assert torch.equal(s(img), new)
    assert torch.equal(s(img), eager(m, img, dtype))
    del junk
    s.close()
    with pytest.raises(RuntimeError, match="closed"):
        s(img)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. - 7. chunking, uint8 input, memory
# ---------------------------------------------------------------------------------------------------------------------------------
def test_chunked_call_equals_its_parts():
    m, cfg, _, _ = fixture_model("fft", "model_tiny_mnist")
    g = torch.Generator().manual_seed(5)
    img = torch.randn(1100, 3, cfg["img_size"], cfg["img_size"], generator=g).to(dev())
    labels = torch.randint(0, cfg["num_classes"], (1100,), generator=g).to(dev())
    with sess(m, torch.bfloat16) as s:   # buckets (1, 8, 64, 512)
        whole = s(img)
        pred = s.predict(img)
        parts = [s(img[a:b]).clone() for a, b in ((0, 512), (512, 1024), (1024, 1100))]
        assert whole.shape == (1100, cfg["num_classes"])
        assert torch.equal(whole, torch.cat(parts))
        assert torch.equal(pred, torch.argmax(whole, dim=1))
        assert sorted(s._b) == [512]
        s.reset_stats()
        s.accumulate(img, labels)
        st = s.stats()
        _, ref = R.eval_head(whole.cpu().numpy(), labels.cpu().numpy(), 1100, 5)
        assert (st["seen"], st["top1"], st["topk"]) == (1100, ref["top1"], ref["topk"]) and loss_close(st["loss_sum"], ref["loss_sum"])
        assert s(img[:9]).shape == (9, cfg["num_classes"]) and sorted(s._b) == [64, 512]   # a second bucket, captured on first use


@pytest.mark.parametrize("dtype", DTYPES)
def test_uint8_input_equals_eager_uint8_forward(dtype):
    m, cfg, _, _ = fixture_model("fft", "model_tiny_mnist")
    g = torch.Generator().manual_seed(6)
    img = torch.randint(0, 256, (8, cfg["img_size"], cfg["img_size"], 3), generator=g, dtype=torch.uint8).to(dev())
    want = eager(m, img, dtype)
    with sess(m, dtype, batch_sizes=(8,), input="uint8") as s:
        assert torch.equal(s(img), want)
        with pytest.raises(ValueError, match="uint8"):
            s(img.permute(0, 3, 1, 2).float())


def test_fifty_calls_allocate_nothing():
    m, cfg, img, labels = fixture_model("permut")
    with sess(m, torch.bfloat16, batch_sizes=(8,)) as s:
        s(img)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for i in range(50):
            (s, s.predict)[i % 2](img)
            s.accumulate(img, labels)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the harness
# ---------------------------------------------------------------------------------------------------------------------------------
CFG = "spectre_vit/configs/spectre_vit_mnist.py"


@pytest.mark.parametrize("graph", [False, True])
def test_harness_graph_eval_matches_the_eager_validation(tmp_path, graph):
    """Tiny/MNIST preset, 2 epochs, n_val = 2 batches of 512: same accuracy and sample count; Loss/Validation within
    5e-6 * |ref| + 2e-7 -- twice the cross-entropy bound (both sides carry it) plus the eager loop's fp32 accumulation of at most 8
    batch terms"""
    from spectre_vit.harness import build_model, train
    from spectre_vit.configs.parser import parse_config
    kw = dict(mixer="fft", epochs=2, steps_per_epoch=10, batch_size=64, n_train=1024, n_val=1024, log=lambda r: None, graph=graph)
    _, h_ref = train(CFG, out_dir=str(tmp_path / "e"), **kw)
    _, h_new = train(CFG, out_dir=str(tmp_path / "s"), graph_eval=True, **kw)
    assert len(h_ref) == len(h_new) == 2
    for a, b in zip(h_ref, h_new):
        print("eager", a, "\nsession", b)
        assert a["Accuracy/Validation"] == b["Accuracy/Validation"]
        assert a["val_samples"] == b["val_samples"] == 1024
        assert abs(a["Loss/Validation"] - b["Loss/Validation"]) <= 5e-6 * abs(a["Loss/Validation"]) + 2e-7, (a, b)
    ck = torch.load(os.path.join(tmp_path, "s", "model_best.pt"), weights_only=True)
    build_model(parse_config(CFG), "fft", dev()).load_state_dict(ck, strict=True)


@pytest.mark.parametrize("graph", [False, True])
def test_harness_graph_eval_tail_batch(tmp_path, graph, monkeypatch):
    """n_val = 1000 in batches of 512: buckets 512 and 488, every sample seen; the epoch's record equals the float64 reference on the
    logits the session produced (recorded at its accumulate calls; batch_hook marks the epoch's first validation batch)"""
    from spectre_vit import inference
    from spectre_vit.harness import train
    seen = []
    orig = inference.InferenceSession.accumulate

    def recording(self, img, labels):
        out = orig(self, img, labels)
        seen.append((out.clone(), labels.clone(), sorted(self._b)))
        return out

    def hook(kind, step, img, label):
        if kind == "val" and step == 0:
            seen.clear()

    monkeypatch.setattr(inference.InferenceSession, "accumulate", recording)
    _, hist = train(CFG, mixer="fft", epochs=2, steps_per_epoch=10, batch_size=64, n_train=1024, n_val=1000, log=lambda r: None, graph=graph,
                    graph_eval=True, out_dir=str(tmp_path), batch_hook=hook)
    assert [h["val_samples"] for h in hist] == [1000, 1000]
    assert [len(z) for z, _, _ in seen] == [512, 488] and seen[-1][2] == [488, 512]
    ref = R.new_stats()
    for z, y, _ in seen:
        _, ref = R.eval_head(z.cpu().numpy(), y.cpu().numpy(), len(z), 5, ref)
    last = hist[-1]
    print(last, ref)
    assert ref["seen"] == 1000 and last["Accuracy/Validation"] == ref["top1"] / 1000
    assert loss_close(last["Loss/Validation"], ref["loss_sum"] / 1000)
    ck = torch.load(os.path.join(tmp_path, "model_best.pt"), weights_only=True)
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.harness import build_model
    build_model(parse_config(CFG), "fft", dev()).load_state_dict(ck, strict=True)


def test_distill_harness_graph_eval(tmp_path):
    """train_distill(graph_eval=True): the student's validation through the session, same record as the eager validation (n_val a multiple
    of the batch size: the eager loop forms its accuracy in fp32, exact for k / 1024)"""
    from spectre_vit.harness import train_distill
    kw = dict(mixer="fft", epochs=1, steps_per_epoch=3, batch_size=32, n_train=256, n_val=1024, log=lambda r: None, augment=False)
    _, h_ref = train_distill(CFG, out_dir=str(tmp_path / "e"), **kw)
    _, h_new = train_distill(CFG, out_dir=str(tmp_path / "s"), graph_eval=True, **kw)
    a, b = h_ref[-1], h_new[-1]
    print("eager", a, "\nsession", b)
    assert a["Accuracy/Validation"] == b["Accuracy/Validation"] and a["val_samples"] == b["val_samples"] == 1024
    assert abs(a["Loss/Validation"] - b["Loss/Validation"]) <= 5e-6 * abs(a["Loss/Validation"]) + 2e-7, (a, b)


def test_cli_scores_a_checkpoint(tmp_path, capsys):
    import json
    from spectre_vit import inference
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.harness import build_model
    torch.manual_seed(1)
    m = build_model(parse_config(CFG), "fft", dev())
    path = str(tmp_path / "model_best.pt")
    torch.save(m.state_dict(), path)
    inference.main(["--config", CFG, "--mixer", "fft", "--checkpoint", path, "--n", "700", "--batch", "512"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["seen"] == 700 and 0.0 <= rec["accuracy"] <= rec["top5"] <= 1.0 and rec["loss"] > 0 and rec["images_per_s"] > 0
