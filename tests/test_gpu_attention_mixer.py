"""SpectreViT(mixer="attention") on the GPU: the single-query-row attention kernels (spv_attention_row0_fwd / _bwd) against numpy
float64 and against the full attention core, the whole model against a float64 reference built from the oracle's own MHSA, and the
graph-replayed training step.

The float64 model reference is oracle/spectre_oracle.py with its mixer hooks routed to mhsa_fwd / mhsa_bwd(batch_first=True) for
"attention" (tests/test_attention_mixer.py pins that definition to torch's nn.MultiheadAttention in float64)."""
import copy

import numpy as np
import pytest
import torch

from oracle import spectre_oracle as O
from test_gpu_bench_shapes import BOUND, SMALL, TINY_BF16_BOUND, TINY_NUMEL, _setup, census, rel_l2
from test_gpu_ops import dev, n64, relerr, t

pytestmark = pytest.mark.gpu

SHAPES = [(3, 65, 16, 32), (2, 50, 8, 6), (2, 197, 12, 64), (4, 1, 2, 32), (2, 257, 4, 32)]   # (B, N, H, hd)
TOL = {torch.float32: 3e-5, torch.bfloat16: 2e-2}   # the bars of test_gpu_model.test_attention_core_vs_oracle


def _softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def row0_reference(q0, kv, dctx0, H):
    """float64 attention of query row 0: ctx0, dq0, dkv = [dk | dv]"""
    B, N, E2 = kv.shape
    E = E2 // 2
    hd = E // H
    k, v = kv[..., :E].reshape(B, N, H, hd), kv[..., E:].reshape(B, N, H, hd)
    q = q0.reshape(B, H, hd)
    p = _softmax(np.einsum("bhd,bnhd->bhn", q, k) / np.sqrt(hd))
    ctx = np.einsum("bhn,bnhd->bhd", p, v).reshape(B, E)
    dc = dctx0.reshape(B, H, hd)
    dp = np.einsum("bhd,bnhd->bhn", dc, v)
    ds = p * (dp - (p * dp).sum(-1, keepdims=True)) / np.sqrt(hd)
    dq = np.einsum("bhn,bnhd->bhd", ds, k).reshape(B, E)
    dk = np.einsum("bhn,bhd->bnhd", ds, q).reshape(B, N, E)
    dv = np.einsum("bhn,bhd->bnhd", p, dc).reshape(B, N, E)
    return ctx, dq, np.concatenate([dk, dv], -1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N,H,hd", SHAPES)
def test_row0_kernels_vs_float64(B, N, H, hd, dtype):
    from spectre_vit import hip_ops
    rng = np.random.default_rng(B * 1000 + N * 10 + H)
    E = H * hd
    q0 = n64(t(rng.standard_normal((B, E)), dtype))
    kv = n64(t(rng.standard_normal((B, N, 2 * E)), dtype))
    dctx0 = n64(t(rng.standard_normal((B, E)), dtype))
    ctx_ref, dq_ref, dkv_ref = row0_reference(q0, kv, dctx0, H)
    before = census()
    Q = t(q0, dtype).requires_grad_(True)
    KV = t(kv, dtype).requires_grad_(True)
    Y = hip_ops.AttentionRow0Fn.apply(Q, KV, H, 0.0)
    Y.backward(t(dctx0, dtype))
    torch.cuda.synchronize()
    took = {k: census()[k] - before[k] for k in before}
    assert took["attn_row0_fwd"] == 1 and took["attn_row0_bwd"] == 1, took
    tol = TOL[dtype]
    errs = dict(ctx=relerr(Y, ctx_ref), dq=relerr(Q.grad, dq_ref), dk=relerr(KV.grad[..., :E], dkv_ref[..., :E]),
                dv=relerr(KV.grad[..., E:], dkv_ref[..., E:]))
    print(f"row0 attention B={B} N={N} H={H} hd={hd} {dtype}: {errs}")
    assert all(v <= tol for v in errs.values()), errs


@pytest.mark.parametrize("B,N,H,hd", [(3, 65, 16, 32), (2, 50, 8, 6), (2, 197, 12, 64)])
def test_row0_dropout_matches_attention_core(B, N, H, hd):
    """p = 0.3, one seed, fp32: the row-0 forward equals row 0 of spv_attention_fwd over [q | k | v] (same mask), and with dctx
    non-zero at row 0 only the row-0 backward's dK / dV (and dq of row 0) equal the full backward's."""
    from spectre_vit import _native, hip_ops
    F32, p, seed = 0, 0.3, 0x1234_5678_9abc
    rng = np.random.default_rng(N)
    E = H * hd
    qkv = t(rng.standard_normal((B, N, 3 * E)))
    ctx = torch.empty((B, N, E), device=dev())
    probs = torch.empty((B, H, N, N), device=dev())
    st = hip_ops._stream()
    _native.call("spv_attention_fwd", qkv.data_ptr(), ctx.data_ptr(), probs.data_ptr(), B, N, H, hd, F32, p, seed, st)
    q0 = qkv[:, 0, :E].contiguous()
    kv = qkv[:, :, E:].contiguous()
    ctx0 = torch.empty((B, E), device=dev())
    p0 = torch.empty((B, H, N), device=dev())
    kp, vp = kv.data_ptr(), kv.data_ptr() + 4 * E
    _native.call("spv_attention_row0_fwd", q0.data_ptr(), kp, vp, 2 * E, ctx0.data_ptr(), p0.data_ptr(), B, N, H, hd, F32, p, seed, st)
    nodrop = torch.empty((B, E), device=dev())
    _native.call("spv_attention_row0_fwd", q0.data_ptr(), kp, vp, 2 * E, nodrop.data_ptr(), 0, B, N, H, hd, F32, 0.0, 0, st)
    torch.cuda.synchronize()
    assert relerr(ctx0, n64(ctx[:, 0])) <= 1e-6
    assert relerr(nodrop, n64(ctx[:, 0])) > 1e-2   # the mask does drop something
    assert torch.allclose(p0, probs[:, :, 0, :], rtol=1e-6, atol=1e-7)   # the saved probabilities are the core's (unmasked)
    dctx = torch.zeros((B, N, E), device=dev())
    dctx[:, 0] = t(rng.standard_normal((B, E)))
    dqkv = torch.empty_like(qkv)
    ds = torch.empty_like(probs)
    _native.call("spv_attention_bwd", dctx.data_ptr(), qkv.data_ptr(), probs.data_ptr(), ds.data_ptr(), dqkv.data_ptr(), B, N, H, hd, F32,
                 p, seed, st)
    dc0 = dctx[:, 0].contiguous()
    dq0 = torch.empty((B, E), device=dev())
    dkv = torch.empty((B, N, 2 * E), device=dev())
    _native.call("spv_attention_row0_bwd", dc0.data_ptr(), q0.data_ptr(), kp, vp, 2 * E, p0.data_ptr(), dq0.data_ptr(), dkv.data_ptr(),
                 dkv.data_ptr() + 4 * E, 2 * E, B, N, H, hd, F32, p, seed, st)
    torch.cuda.synchronize()
    errs = dict(dk=relerr(dkv[..., :E], n64(dqkv[:, :, E:2 * E])), dv=relerr(dkv[..., E:], n64(dqkv[:, :, 2 * E:])),
                dq=relerr(dq0, n64(dqkv[:, 0, :E])))
    print(f"row0 vs core, p=0.3, B={B} N={N} H={H} hd={hd}: {errs}")
    assert errs["dv"] <= 1e-6 and errs["dk"] <= 1e-5 and errs["dq"] <= 1e-5, errs


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole model against float64
# ---------------------------------------------------------------------------------------------------------------------------------
def _route_attention(monkeypatch):
    real_fwd, real_bwd = O.mixer_fwd, O.mixer_bwd

    def fwd(x, lp, mixer):
        if mixer == "attention":
            return O.mhsa_fwd(x, lp["mix_layer"], lp["heads"], batch_first=True)
        return real_fwd(x, lp, mixer)

    def bwd(dy, lp, mixer, cache):
        if mixer == "attention":
            return O.mhsa_bwd(dy, lp["mix_layer"], lp["heads"], cache, batch_first=True)
        return real_bwd(dy, lp, mixer, cache)

    monkeypatch.setattr(O, "mixer_fwd", fwd)
    monkeypatch.setattr(O, "mixer_bwd", bwd)


MIX = (("in_proj_weight", "in_proj_weight"), ("in_proj_bias", "in_proj_bias"), ("out_proj_weight", "out_proj.weight"),
       ("out_proj_bias", "out_proj.bias"))


def attention_train_step(img, labels, sd, layers, patch, heads):
    """O.train_step for mixer="attention" (needs _route_attention): loss, logits, grads by state_dict name"""
    f64 = np.float64
    params = O.params_from_state_dict(sd, layers, "attention", f64)
    for i, lp in enumerate(params["layers"]):
        pre = f"encoder_blocks.layers.{i}.mix_layer."
        lp["mix_layer"] = {o: np.asarray(sd[pre + s], f64) for o, s in MIX}
        lp["heads"] = heads
    logits, _, cache = O.spectre_vit_fwd(np.asarray(img, f64), params, patch, "attention")
    loss, dlogits = O.cross_entropy_fwd_bwd(logits, np.asarray(labels, np.int64))
    g = O.spectre_vit_bwd(dlogits, params, patch, cache, "attention")
    mix = [gl.pop("mix_layer") for gl in g["layers"]]
    grads = O.grads_to_state_dict(g)
    for i, gm in enumerate(mix):
        pre = f"encoder_blocks.layers.{i}.mix_layer."
        for o, s in MIX:
            grads[pre + s] = gm[o]
    return float(loss), logits, grads


_ref_cache = {}


@pytest.mark.parametrize("cls_only", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_model_step_vs_float64(dtype, cls_only, monkeypatch):
    """Small widths (E 512, 16 heads, head dim 32), 4 layers, bs 128, dropout off: loss, logits, every gradient -- in_proj's Q block
    (rows 0..E) and K|V block (rows E..3E) on their own as well -- and the weights after one torch.optim.AdamW step, against float64;
    the last layer through the row-0 kernels (default) and over every row."""
    from spectre_vit import hip_ops
    _route_attention(monkeypatch)
    m, img, labels, sd = _setup(SMALL, "attention", 128, 41)
    if "ref" not in _ref_cache:
        _ref_cache["ref"] = attention_train_step(img.numpy(), labels.numpy(), sd, 4, 4, SMALL["num_heads"])
    loss_ref, logits_ref, grads_ref = _ref_cache["ref"]
    keep = hip_ops.LAST_LAYER_CLS_ONLY
    hip_ops.LAST_LAYER_CLS_ONLY = cls_only
    try:
        m = m.to(dev()).train()
        before = census()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            logits = m(img.to(dev()))
        loss = torch.nn.CrossEntropyLoss()(logits, labels.to(dev()))
        loss.backward()
        torch.cuda.synchronize()
        took = {k: census()[k] - before[k] for k in before}
    finally:
        hip_ops.LAST_LAYER_CLS_ONLY = keep
    n = 1 if cls_only else 0
    assert took["attn_row0_fwd"] == n and took["attn_row0_bwd"] == n, took
    bound = BOUND[dtype]
    assert abs(loss.item() - loss_ref) <= bound * abs(loss_ref), (loss.item(), loss_ref)
    errs = {"logits": rel_l2(logits, logits_ref)}
    limit = {}
    E = SMALL["embed_dim"]
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        errs[k] = rel_l2(p.grad, grads_ref[k])
        if k.endswith("in_proj_weight"):
            errs[k + "[q]"] = rel_l2(p.grad[:E], grads_ref[k][:E])
            errs[k + "[kv]"] = rel_l2(p.grad[E:], grads_ref[k][E:])
        if dtype == torch.bfloat16 and p.numel() <= TINY_NUMEL:
            limit[k] = max(bound, TINY_BF16_BOUND)
    worst = max(errs, key=errs.get)
    print(f"attention bs128 {dtype} cls_only={cls_only}: worst rel-L2 {errs[worst]:.3e} ({worst}); logits {errs['logits']:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= limit.get(k, bound)}
    assert not bad, bad
    # one AdamW step on those gradients
    w0 = {k: n64(p) for k, p in m.named_parameters()}
    torch.optim.AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01).step()
    for k, p in m.named_parameters():
        z = np.zeros_like(w0[k])
        w_ref, _, _ = O.adamw_step(w0[k], grads_ref[k], z, z, 1)
        assert rel_l2(p, w_ref) <= bound, (k, rel_l2(p, w_ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# the timed path: graph replay at Small, bs 512, bf16
# ---------------------------------------------------------------------------------------------------------------------------------
def _graphed(m, img, labels, lr, dp=False):
    from spectre_vit.graph import GraphedDPStep, GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.optim import FusedAdamW
    opt = FusedAdamW(m.parameters(), lr=lr, betas=(0.9, 0.999), weight_decay=0.0 if lr == 0.0 else 0.01, capturable=True, static_grads=True)
    torch.cuda.empty_cache()
    cls = GraphedDPStep if dp else GraphedTrainStep
    return cls(m, opt, CrossEntropyLoss(), img.to(dev()), labels.to(dev()), autocast_dtype=torch.bfloat16, warmup=1)


@pytest.mark.parametrize("dp_sequence", [False, True])
def test_graph_replay_gradients_equal_eager_step(dp_sequence):
    """one replay of the captured step (gradient sinks, the held and batched weight gradients -- both in_proj blocks of the CLS-only
    last layer among them) against the eager bf16 step on the same weights and batch"""
    from spectre_vit import hip_ops
    assert hip_ops.LAST_LAYER_CLS_ONLY
    m, img, labels, _ = _setup(SMALL, "attention", 512, 43)
    m = m.to(dev()).train()
    before = census()
    step = _graphed(m, img, labels, 1e-3, dp=dp_sequence)
    try:
        sd0 = copy.deepcopy(m.state_dict())
        loss = step()
        torch.cuda.synchronize()
        grads = {k: n64(p.grad) for k, p in m.named_parameters()}
    finally:
        step.close()
    took = {k: census()[k] - before[k] for k in before}
    assert took["attn_row0_fwd"] >= 2 and took["attn_row0_bwd"] >= 2, took   # the warm-up step and the capture
    assert took["gemm_tn_batch"] >= 2, took
    from spectre_vit.models.spectre.spectre import SpectreViT
    e = SpectreViT(**SMALL, mixer="attention").to(dev()).train()
    e.load_state_dict(sd0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = e(img.to(dev()))
    loss_e = torch.nn.CrossEntropyLoss()(logits, labels.to(dev()))
    loss_e.backward()
    bound = BOUND[torch.bfloat16]
    assert abs(loss.item() - loss_e.item()) <= bound * abs(loss_e.item()), (loss.item(), loss_e.item())
    errs = {k: rel_l2(torch.from_numpy(grads[k]), n64(p.grad)) for k, p in e.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"graph replay vs eager (attention, bs512{', two graphs' if dp_sequence else ''}): worst gradient rel-L2 {errs[worst]:.3e} ({worst})")
    bad = {k: v for k, v in errs.items() if v > (max(bound, TINY_BF16_BOUND) if grads[k].size <= TINY_NUMEL else bound)}
    assert not bad, bad


def test_graph_replay_fresh_dropout_masks_and_training():
    """dropout 0.1 (attention probabilities included) with the optimizer at lr = 0: two replays on the same batch and weights give
    different losses (the seed word advances inside the graph); then, at lr = 1e-3, a few replays lower the loss"""
    cfg = dict(SMALL, dropout=0.1)
    m, img, labels, _ = _setup(cfg, "attention", 512, 47)
    m = m.to(dev()).train()
    step = _graphed(m, img, labels, 0.0)
    try:
        a = float(step())
        b = float(step())
    finally:
        step.close()
    assert np.isfinite(a) and np.isfinite(b) and a != b, (a, b)
    m2, img2, labels2, _ = _setup(SMALL, "attention", 512, 53)
    m2 = m2.to(dev()).train()
    step = _graphed(m2, img2, labels2, 1e-3)
    try:
        losses = [float(step()) for _ in range(6)]
    finally:
        step.close()
    print("graph-replayed attention losses:", losses)
    assert losses[-1] < losses[0], losses


def test_eager_fp16_autocast_gradscaler_adamw_trains():
    """the reference script's loop shape (fp16 autocast, served by the bf16 kernels, + GradScaler + torch.optim.AdamW) trains"""
    m, img, labels, _ = _setup(dict(SMALL, num_encoders=2), "attention", 128, 59)
    m = m.to(dev()).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda")
    img, labels = img.to(dev()), labels.to(dev())
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            loss = torch.nn.CrossEntropyLoss()(m(img), labels)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
