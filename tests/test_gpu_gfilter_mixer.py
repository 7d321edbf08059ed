"""SpectreViT(mixer="filter") on the GPU: spv_gfilter_fwd / spv_gfilter_bwd through the C-ABI against the float64 reference of
tests/gfilter_ref.py at the project's bars (spectral_edge_cases.TRANSFORM_BAR / GRAD_BAR and bar()), measured as
tests/test_gpu_spectral_edges.py measures (max-abs over the reference's max-abs, per sample for y / dx, over the tensor for dW); the
refusals; the autograd surface; the whole model against a float64 reference built from the oracle with its mixer hooks routed to
gfilter_ref; and the graph-replayed training step and the InferenceSession.

tests/test_gfilter_mixer.py checks on the CPU that the tables reach every branch, that a float32 restatement of the generic kernels on
exactly these inputs stays within a quarter of each fp32 bar, and that a restatement of the fast path's arithmetic (hi + lo bf16
tables and spectrum on the MFMA) stays within half of each bf16 bar."""
import copy

import numpy as np
import pytest
import torch

import gfilter_ref as G
import spectral_ref as R
from oracle import spectre_oracle as O
from test_gpu_attention_edges import Guarded, delta
from test_gpu_bench_shapes import BOUND, SMALL, TINY_BF16_BOUND, TINY_NUMEL, _setup, census, rel_l2
from test_gpu_ops import dev, n64, t
from test_gpu_spectral_edges import check_memory, judge, scratch

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F32 = torch.float32


def _native():
    from spectre_vit import _native as n
    return n


def _st():
    from spectre_vit import hip_ops
    return hip_ops._stream()


def _bits(a):
    return a.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


_tables = {}


def _table(tokens):
    """the test's own guarded table, NaN before spv_gfilter_make_tables fills it; judged against float64 once"""
    if tokens not in _tables:
        n = _native().call("spv_gfilter_table_floats", tokens)
        assert n == G.table_floats(tokens)
        tab = Guarded((n,), F32)
        _native().call("spv_gfilter_make_tables", tab.ptr, tokens, _st())
        torch.cuda.synchronize()
        a = 2.0 * np.pi * np.arange(tokens) / tokens
        want = np.stack([np.cos(a), np.sin(a)], axis=-1).reshape(-1)
        assert tab.intact() and np.abs(tab.f64()[:2 * tokens] - want).max() <= 2.0 ** -24, "each entry is float64's, rounded once"
        if tokens <= G.FAST_MAX_TOKENS:   # the fast path's matrices behind it: the same entries as hi + lo bf16, zero padded
            t1, t2 = G.fast_tables(tokens)
            got = tab.t[G.generic_table_floats(tokens):].view(torch.bfloat16).float().cpu().numpy()
            assert got.size == t1.size + t2.size
            g1, g2 = got[:t1.size].reshape(t1.shape), got[t1.size:].reshape(t2.shape)
            assert np.abs((g1[0] + g1[1]) - (t1[0] + t1[1])).max() <= 2.0 ** -23 and np.abs((g2[0] + g2[1]) - (t2[0] + t2[1])).max() <= 2.0 ** -23
            assert not g1[:, :, G.bins(tokens):].any() and not g1[:, :, :, tokens:].any() and not g2[:, :, tokens:].any()
        _tables[tokens] = tab
    return _tables[tokens]


# ------------------------------------------------------------------------------------------------------------------ A. the C-ABI
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_gfilter_fwd_and_bwd_vs_float64(case):
    nat, c = _native(), case
    code = G.CODE[c.dtype]
    path = G.path(c.dtype, c.tokens, c.dim, not c.off)
    assert nat.call("spv_gfilter_path", code, c.tokens, c.dim, int(not c.off)) == path and path in (G.FAST, G.GENERIC)
    shape, dtype, K = (c.batch, c.tokens, c.dim), DT[c.dtype], G.bins(c.tokens)
    x64, dy64, w64 = G.inputs(c)
    data = dict(x=x64, dy=dy64, filter=w64)
    off = c.off // (2 if c.dtype == "bf16" else 4)
    tab = _table(c.tokens)
    tab_bits = _bits(tab.t)   # (the floats between the fp32 table and the 16-byte start of the fast tables stay NaN)
    ins = dict(x=Guarded(shape, dtype, x64, off), dy=Guarded(shape, dtype, dy64, off), filter=Guarded((K, c.dim, 2), F32, w64))
    wsn, pn = nat.call("spv_gfilter_workspace_floats", *shape), nat.call("spv_gfilter_partial_floats", *shape)
    assert wsn == G.workspace_floats(*shape) and pn == G.partial_floats(*shape)
    outs = dict(y=Guarded(shape, dtype, off=off), dx=Guarded(shape, dtype, off=off), dfilter=Guarded((K, c.dim, 2), F32), partials=scratch(pn),
                workspace=scratch(wsn))
    before = census()
    nat.call("spv_gfilter_fwd", ins["x"].ptr, ins["filter"].ptr, outs["y"].ptr, tab.ptr, *shape, code, outs["workspace"].ptr, _st())
    nat.call("spv_gfilter_bwd", ins["x"].ptr, ins["dy"].ptr, ins["filter"].ptr, outs["dx"].ptr, outs["dfilter"].ptr, tab.ptr,
             outs["partials"].ptr, *shape, code, outs["workspace"].ptr, _st())
    torch.cuda.synchronize()
    assert delta(before) == {}, "the census keeps its 27 slots"
    check_memory(ins, outs, data, dict(partials=pn, workspace=wsn))
    assert tab.intact() and torch.equal(_bits(tab.t), tab_bits), "the table is read only"
    got = {k: b.f64() for k, b in outs.items()}
    errs = dict(y=R.err(got["y"], G.fwd(x64, w64), 1), dx=R.err(got["dx"], G.dx(dy64, w64), 1), dw=R.err(got["dfilter"], G.dw(x64, dy64)))
    bars = dict(y=G.bar(G.TRANSFORM_BAR, c.dtype), dx=G.bar(G.GRAD_BAR, c.dtype), dw=G.GRAD_BAR)
    judge(f"gfilter {'fast' if path == G.FAST else 'generic'} {G.case_id(c)}", errs, bars)
    # the inert imaginary parts: exactly +0, in the gradient and in every slab
    raw = outs["dfilter"].t.cpu().numpy()
    slabs = outs["partials"].t[:pn].cpu().numpy().reshape(G.slabs(c.batch), K, c.dim, 2)
    for k in G.inert(c.tokens):
        assert not raw[k, :, 1].any() and not np.signbit(raw[k, :, 1]).any() and not slabs[:, k, :, 1].any() and not np.signbit(slabs[:, k, :, 1]).any()
    # the same call again: the same bits
    again = dict(dx=Guarded(shape, dtype, off=off), dfilter=Guarded((K, c.dim, 2), F32), partials=scratch(pn))
    nat.call("spv_gfilter_bwd", ins["x"].ptr, ins["dy"].ptr, ins["filter"].ptr, again["dx"].ptr, again["dfilter"].ptr, tab.ptr,
             again["partials"].ptr, *shape, code, 0, _st())
    torch.cuda.synchronize()
    for k, b in again.items():
        n = pn if k == "partials" else b.t.numel()
        assert b.intact() and torch.equal(_bits(b.t)[:n * b.t.element_size()], _bits(outs[k].t)[:n * b.t.element_size()]), k


@pytest.mark.parametrize("case", G.MISALIGNED_REFUSED, ids=G.case_id)
def test_fast_path_refuses_the_pointer_the_generic_path_takes(case):
    nat, c = _native(), case
    shape, K = (c.batch, c.tokens, c.dim), G.bins(c.tokens)
    off = c.off // 2
    assert G.path(c.dtype, c.tokens, c.dim) == G.FAST and G.path(c.dtype, c.tokens, c.dim, False) == G.REFUSE_ALIGN
    assert nat.call("spv_gfilter_path", 1, c.tokens, c.dim, 0) == G.REFUSE_ALIGN and G.Case("bf16", 3, 7, 12, c.off) in G.CASES
    x64, dy64, w64 = G.inputs(c)
    bf = torch.bfloat16
    tab, w = _table(c.tokens), Guarded((K, c.dim, 2), F32, w64)
    pn = nat.call("spv_gfilter_partial_floats", *shape)
    before = census()
    # each of x, y, dy, dx in turn off 16-byte alignment, the others on it
    for which in ("x", "y", "dy", "dx"):
        o = {k: off if k == which else 0 for k in ("x", "y", "dy", "dx")}
        x, dy = Guarded(shape, bf, x64, o["x"]), Guarded(shape, bf, dy64, o["dy"])
        outs = dict(y=Guarded(shape, bf, off=o["y"]), dx=Guarded(shape, bf, off=o["dx"]), dfilter=Guarded((K, c.dim, 2), F32), partials=scratch(pn))
        if which in ("x", "y"):
            with pytest.raises(RuntimeError, match="16-byte aligned"):
                nat.call("spv_gfilter_fwd", x.ptr, w.ptr, outs["y"].ptr, tab.ptr, *shape, 1, 0, _st())
        if which != "y":
            with pytest.raises(RuntimeError, match="16-byte aligned"):
                nat.call("spv_gfilter_bwd", x.ptr, dy.ptr, w.ptr, outs["dx"].ptr, outs["dfilter"].ptr, tab.ptr, outs["partials"].ptr, *shape, 1, 0, _st())
        torch.cuda.synchronize()
        for k, b in outs.items():
            assert bool(torch.isnan(b.t).all()) and b.intact(), (which, k)
    assert delta(before) == {}


REFUSED = [("fp32", 3, 0, 8, "empty shape"), ("bf16", 3, 8, 0, "empty shape"), ("fp32", 0, 5, 8, "empty shape"), (2, 3, 8, 8, "unknown dtype"),
           ("fp32", 1, G.MAX_TOKENS + 1, 8, "too many tokens")]


@pytest.mark.parametrize("dt,batch,tokens,dim,why", REFUSED)
def test_refusals_raise_write_nothing_and_count_nothing(dt, batch, tokens, dim, why):
    """real, NaN-filled buffers of a small shape behind the refused arguments"""
    nat = _native()
    shape = (3, 5, 8)
    x, dy, w = Guarded(shape, F32, np.ones(shape)), Guarded(shape, F32, np.ones(shape)), Guarded((3, 8, 2), F32, np.ones((3, 8, 2)))
    tab = _table(5)
    outs = dict(y=Guarded(shape, F32), dx=Guarded(shape, F32), dfilter=Guarded((3, 8, 2), F32), partials=scratch(3 * 3 * 8 * 2))
    before = census()
    code = G.CODE.get(dt, dt)
    with pytest.raises(RuntimeError, match=why):
        nat.call("spv_gfilter_fwd", x.ptr, w.ptr, outs["y"].ptr, tab.ptr, batch, tokens, dim, code, 0, _st())
    with pytest.raises(RuntimeError, match=why):
        nat.call("spv_gfilter_bwd", x.ptr, dy.ptr, w.ptr, outs["dx"].ptr, outs["dfilter"].ptr, tab.ptr, outs["partials"].ptr, batch, tokens, dim,
                 code, 0, _st())
    with pytest.raises(RuntimeError, match="null pointer"):
        nat.call("spv_gfilter_fwd", x.ptr, w.ptr, outs["y"].ptr, 0, *shape, 0, 0, _st())
    torch.cuda.synchronize()
    assert delta(before) == {}
    for k, b in outs.items():
        assert bool(torch.isnan(b.t).all()) and b.intact(), k
    assert nat.call("spv_gfilter_path", code, tokens, dim, 1) < 0 or batch < 1


# ------------------------------------------------------------------------------------------------------------------ B. autograd
@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("shape,dtn", [((2, 5, 24), "fp32"), ((3, 65, 512), "bf16"), ((3, 65, 512), "fp32")])
def test_global_filter_fn_forward_backward_and_gradient_dtypes(shape, dtn, autocast):
    from spectre_vit.modules.mixers import GlobalFilterMixer
    c = G.Case(dtn, *shape)
    x64, dy64, w64 = G.inputs(c)
    out_dt = "bf16" if autocast else dtn
    if autocast:   # the mixer casts x to the autocast dtype: the reference sees the rounded x
        x64 = n64(t(x64, DT[dtn]).to(torch.bfloat16))
    mix = GlobalFilterMixer(shape[1], shape[2]).to(dev())
    assert mix.complex_weight.dtype == F32 and tuple(mix.complex_weight.shape) == (G.bins(shape[1]), shape[2], 2)
    with torch.no_grad():
        mix.complex_weight.copy_(t(w64, F32))
    x = t(x64, DT[dtn]).requires_grad_(True)
    addr = []
    for _ in range(2):
        x.grad = None
        mix.complex_weight.grad = None if not addr else mix.complex_weight.grad.zero_()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = mix(x)
        assert y.dtype == DT[out_dt] and y.shape == x.shape
        y.backward(t(dy64, DT[out_dt]))
        addr.append(mix.complex_weight.grad.data_ptr())
    torch.cuda.synchronize()
    assert addr[0] == addr[1], "the filter's gradient keeps its address"
    assert x.grad.dtype == DT[dtn] and mix.complex_weight.grad.dtype == F32 and mix.complex_weight.dtype == F32
    if autocast:
        dy64 = n64(t(dy64, DT[out_dt]))
    errs = dict(y=R.err(n64(y), G.fwd(x64, w64), 1), dx=R.err(n64(x.grad), G.dx(dy64, w64), 1), dw=R.err(n64(mix.complex_weight.grad), G.dw(x64, dy64)))
    judge(f"GlobalFilterMixer {shape} {dtn} autocast={autocast}", errs,
          dict(y=G.bar(G.TRANSFORM_BAR, out_dt), dx=G.bar(G.GRAD_BAR, out_dt), dw=G.GRAD_BAR))
    with pytest.raises(ValueError):
        mix(x[:, :-1] if shape[1] > 1 else x[:, :, :-1])


# ------------------------------------------------------------------------------------------------------------------ C. the whole model
def _route_filter(monkeypatch):
    real_fwd, real_bwd = O.mixer_fwd, O.mixer_bwd

    def fwd(x, lp, mixer):
        return (G.fwd(x, lp["mix_layer"]), x) if mixer == "filter" else real_fwd(x, lp, mixer)

    def bwd(dy, lp, mixer, cache):
        return (G.dx(dy, lp["mix_layer"]), dict(complex_weight=G.dw(cache, dy))) if mixer == "filter" else real_bwd(dy, lp, mixer, cache)

    monkeypatch.setattr(O, "mixer_fwd", fwd)
    monkeypatch.setattr(O, "mixer_bwd", bwd)


def _randomise_filters(m, sd=None):
    """0.02 randn would leave the filter's share of every number near the bars' noise: a unit-scale filter, seeded per layer"""
    with torch.no_grad():
        for i, layer in enumerate(m.encoder_blocks.layers):
            g = torch.Generator().manual_seed(900 + i)
            layer.mix_layer.complex_weight.copy_(0.5 * torch.randn(layer.mix_layer.complex_weight.shape, generator=g))
            if sd is not None:
                sd[f"encoder_blocks.layers.{i}.mix_layer.complex_weight"] = layer.mix_layer.complex_weight.numpy().copy()


def _reference_step(img, labels, sd, layers):
    params = O.params_from_state_dict(sd, layers, "filter", np.float64)
    for i, lp in enumerate(params["layers"]):
        lp["mix_layer"] = np.asarray(sd[f"encoder_blocks.layers.{i}.mix_layer.complex_weight"], np.float64)
    logits, _, cache = O.spectre_vit_fwd(np.asarray(img, np.float64), params, 4, "filter")
    loss, dlogits = O.cross_entropy_fwd_bwd(logits, np.asarray(labels, np.int64))
    g = O.spectre_vit_bwd(dlogits, params, 4, cache, "filter")
    filters = {f"encoder_blocks.layers.{i}.mix_layer.complex_weight": gl.pop("mix_layer")["complex_weight"] for i, gl in enumerate(g["layers"])}
    grads = O.grads_to_state_dict(g)
    grads.update(filters)
    return float(loss), logits, grads


_ref_cache = {}


@pytest.mark.parametrize("cls_only", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_filter_model_step_vs_float64(dtype, cls_only, monkeypatch):
    """Small widths, 4 layers, bs 128, dropout off: loss, logits, every gradient (each complex_weight included) and the weights after one
    torch.optim.AdamW step against float64; the last layer at the CLS rows only (default) and over every row"""
    from spectre_vit import hip_ops
    _route_filter(monkeypatch)
    m, img, labels, sd = _setup(SMALL, "filter", 128, 47)
    _randomise_filters(m, sd)
    if "ref" not in _ref_cache:
        _ref_cache["ref"] = _reference_step(img.numpy(), labels.numpy(), sd, 4)
    loss_ref, logits_ref, grads_ref = _ref_cache["ref"]
    keep = hip_ops.LAST_LAYER_CLS_ONLY
    hip_ops.LAST_LAYER_CLS_ONLY = cls_only
    try:
        m = m.to(dev()).train()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            logits = m(img.to(dev()))
        loss = torch.nn.CrossEntropyLoss()(logits, labels.to(dev()))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        hip_ops.LAST_LAYER_CLS_ONLY = keep
    bound = BOUND[dtype]
    assert abs(loss.item() - loss_ref) <= bound * abs(loss_ref), (loss.item(), loss_ref)
    errs, limit = {"logits": rel_l2(logits, logits_ref)}, {}
    names = [k for k, _ in m.named_parameters()]
    assert sum(k.endswith("mix_layer.complex_weight") for k in names) == 4 and set(names) == set(grads_ref)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        errs[k] = rel_l2(p.grad, grads_ref[k])
        if dtype == torch.bfloat16 and p.numel() <= TINY_NUMEL:
            limit[k] = max(bound, TINY_BF16_BOUND)
    worst = max(errs, key=errs.get)
    print(f"filter bs128 {dtype} cls_only={cls_only}: worst rel-L2 {errs[worst]:.3e} ({worst}); logits {errs['logits']:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= limit.get(k, bound)}
    assert not bad, bad
    w0 = {k: n64(p) for k, p in m.named_parameters()}
    torch.optim.AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01).step()
    for k, p in m.named_parameters():
        z = np.zeros_like(w0[k])
        w_ref, _, _ = O.adamw_step(w0[k], grads_ref[k], z, z, 1)
        assert rel_l2(p, w_ref) <= bound, (k, rel_l2(p, w_ref))


# ------------------------------------------------------------------------------------------------------------------ D. graphs and sessions
def test_graph_replay_gradients_equal_eager_step():
    """one replay of the captured step against the eager bf16 step on the same weights and batch"""
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    m, img, labels, _ = _setup(SMALL, "filter", 128, 53)
    _randomise_filters(m)
    m = m.to(dev()).train()
    opt = FusedAdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True)
    torch.cuda.empty_cache()
    step = GraphedTrainStep(m, opt, CrossEntropyLoss(), img.to(dev()), labels.to(dev()), autocast_dtype=torch.bfloat16, warmup=1)
    try:
        sd0 = copy.deepcopy(m.state_dict())
        loss = step()
        torch.cuda.synchronize()
        grads = {k: n64(p.grad) for k, p in m.named_parameters()}
        moved = {k: not torch.equal(v, sd0[k]) for k, v in m.state_dict().items() if k.endswith("complex_weight")}
    finally:
        step.close()
    assert len(moved) == 4 and all(moved.values()), "the replayed optimizer step moves every filter"
    e = SpectreViT(**SMALL, mixer="filter").to(dev()).train()
    e.load_state_dict(sd0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = e(img.to(dev()))
    loss_e = torch.nn.CrossEntropyLoss()(logits, labels.to(dev()))
    loss_e.backward()
    bound = BOUND[torch.bfloat16]
    assert abs(loss.item() - loss_e.item()) <= bound * abs(loss_e.item()), (loss.item(), loss_e.item())
    errs = {k: rel_l2(torch.from_numpy(grads[k]), n64(p.grad)) for k, p in e.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"graph replay vs eager (filter, bs128): worst gradient rel-L2 {errs[worst]:.3e} ({worst})")
    bad = {k: v for k, v in errs.items() if v > (max(bound, TINY_BF16_BOUND) if grads[k].size <= TINY_NUMEL else bound)}
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inference_session_equals_eager_eval_and_owns_its_filter(dtype):
    """the same kernels in the same order: bitwise equal logits and features at a batch equal to a bucket, replayed twice; the session's
    own copy of the filter changes at refresh() and not before"""
    from spectre_vit.inference import InferenceSession
    m, img, _, _ = _setup(SMALL, "filter", 64, 59)
    _randomise_filters(m)
    m = m.to(dev()).eval()
    img = img.to(dev())
    amp = dict(device_type="cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16)
    with torch.no_grad(), torch.autocast(**amp):
        want, want_cls = m(img, return_features=True)
    with InferenceSession(m, autocast_dtype=torch.bfloat16 if dtype == torch.bfloat16 else None, batch_sizes=(64,), return_features=True) as s:
        got = s(img)
        assert got.dtype == torch.float32 and torch.equal(got, want), (got - want).abs().max().item()
        assert torch.equal(s.features, want_cls)
        assert torch.equal(s(img), want)
        with torch.no_grad():
            for layer in m.encoder_blocks.layers:
                layer.mix_layer.complex_weight.mul_(-1.5)
        assert torch.equal(s(img), want), "the model's filter changed in place: the session still holds its own"
        with torch.no_grad(), torch.autocast(**amp):
            new = m(img)
        assert not torch.equal(new, want)
        s.refresh()
        assert torch.equal(s(img), new)
