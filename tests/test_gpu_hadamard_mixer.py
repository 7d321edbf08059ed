"""SpectreViT(mixer="hadamard") on the GPU: every kernel of csrc/spv_hadamard.hip's 2-D family against the float64 reference of
tests/hadamard_ref.py at the project's bars (spectral_edge_cases.TRANSFORM_BAR / LN_BAR / GRAD_BAR and bar()), measured as
tests/test_gpu_spectral_edges.py measures (max-abs over the reference's max-abs, per sample or over the whole tensor); the autograd
surface; the whole model against a float64 reference built from the oracle with its mixer hooks routed to hadamard_ref.mix; and the
graph-replayed training step and the InferenceSession.

tests/test_hadamard_mixer.py checks on the CPU that the tables reach every branch and that the float32 floor of the references on
exactly these inputs stays within a quarter of each fp32 bar.

FUSED_DX_BAR: dx of the fused bf16 backward is held to bar(GRAD_BAR, "bf16") = 6e-5 + 2^-8 -- the bf16 store's unit roundoff and
nothing else, which the hi + lo split of the LayerNorm gradient is there to make possible."""
import copy

import numpy as np
import pytest
import torch

import hadamard_ref as H
import spectral_ref as R
from oracle import spectre_oracle as O
from test_gpu_attention_edges import Guarded, delta
from test_gpu_bench_shapes import BOUND, SMALL, TINY_BF16_BOUND, TINY_NUMEL, _setup, census, rel_l2
from test_gpu_ops import dev, n64, t
from test_gpu_spectral_edges import check_memory, judge, scratch

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F32 = torch.float32
FUSED_DX_BAR = H.bar(H.GRAD_BAR, "bf16")


def _native():
    from spectre_vit import _native as n
    return n


def _st():
    from spectre_vit import hip_ops
    return hip_ops._stream()


# ------------------------------------------------------------------------------------------------------------------ A. spv_hadamard_mix
@pytest.mark.parametrize("run", ["A", "B"])
@pytest.mark.parametrize("case", H.MIX_CASES, ids=H.case_id)
def test_hadamard_mix_vs_float64(case, run):
    """run A: add_in = NULL; run B: a random add_in"""
    nat, c = _native(), case
    path = H.path(c.dtype, c.tokens, c.dim)
    assert path in (H.ONE_KERNEL, H.GENERIC) and nat.call("spv_hadamard_path", H.CODE[c.dtype], c.tokens, c.dim, 1) == path
    rng, shape, dtype = H.rng_of(c, run), (c.batch, c.tokens, c.dim), DT[c.dtype]
    data = dict(x=H.normal(rng, shape, c.dtype))
    if run == "B":
        data["add_in"] = H.normal(rng, shape, c.dtype)
    off = c.off // (2 if c.dtype == "bf16" else 4)
    assert not off or path == H.GENERIC
    ins = {k: Guarded(shape, dtype, v, off) for k, v in data.items()}
    wsn = nat.call("spv_hadamard_workspace_floats", *shape)
    assert wsn == H.workspace_floats(*shape) and (wsn == 0) == (path == H.ONE_KERNEL)
    outs = dict(y=Guarded(shape, dtype, off=off))
    if wsn:
        outs["workspace"] = scratch(wsn)
    before = census()
    nat.call("spv_hadamard_mix", ins["x"].ptr, outs["y"].ptr, ins["add_in"].ptr if run == "B" else 0, *shape, H.scale32(c.tokens, c.dim),
             H.CODE[c.dtype], outs["workspace"].ptr if wsn else 0, _st())
    torch.cuda.synchronize()
    assert delta(before) == {}, "the census keeps its 27 slots"
    check_memory(ins, outs, data, dict(workspace=wsn))
    ref = H.mix(data["x"], True, data.get("add_in"))
    kind = "one-kernel" if path == H.ONE_KERNEL else "generic"
    judge(f"hadamard mix {kind} {H.case_id(c)} {run}", dict(y=R.err(outs["y"].f64(), ref, 1)), dict(y=H.bar(H.TRANSFORM_BAR, c.dtype)))


def test_hadamard_mix_unnormalised_scale_is_the_callers():
    nat = _native()
    x64 = H.normal(np.random.default_rng(3), (2, 5, 24), "fp32")
    x, y = Guarded(x64.shape, F32, x64), Guarded(x64.shape, F32)
    nat.call("spv_hadamard_mix", x.ptr, y.ptr, 0, 2, 5, 24, 1.0, 0, 0, _st())
    torch.cuda.synchronize()
    assert R.err(y.f64(), H.mix(x64, normalize=False), 1) <= H.TRANSFORM_BAR and x.intact() and y.intact()


@pytest.mark.parametrize("case", H.MISALIGNED_REFUSED, ids=H.case_id)
def test_one_kernel_path_refuses_the_pointer_the_generic_path_takes(case):
    nat, c = _native(), case
    shape, dtype = (c.batch, c.tokens, c.dim), DT[c.dtype]
    off = c.off // (2 if c.dtype == "bf16" else 4)
    assert H.path(c.dtype, c.tokens, c.dim) == H.ONE_KERNEL and H.Mix(c.dtype, 3, 7, 12, c.off) in H.MIX_CASES
    x, y = Guarded(shape, dtype, H.normal(H.rng_of(c), shape, c.dtype), off), Guarded(shape, dtype, off=off)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        nat.call("spv_hadamard_mix", x.ptr, y.ptr, 0, *shape, 1.0, H.CODE[c.dtype], 0, _st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t).all()) and y.intact()


# ------------------------------------------------------------------------------------------------------------------ B. the fused pair
def _fused(case, mode):
    """spv_hadamard_ln_fwd, then spv_hadamard_ln_bwd fed the forward's own prenorm, mean and rstd"""
    nat, c, dtn, bf = _native(), case, "bf16", torch.bfloat16
    B, N, Dm = c.batch, c.tokens, 512
    shape = (B, N, Dm)
    rng = H.rng_of(c, "fold")   # both modes on the same inputs
    data = dict(x=H.normal(rng, shape, dtn))
    data["gamma"], data["beta"] = H.affine(rng, Dm)
    data["dout"] = H.normal(rng, shape, dtn)
    defer = mode == "defer"
    ins = dict(x=Guarded(shape, bf, data["x"]), gamma=Guarded((Dm,), F32, data["gamma"]), beta=Guarded((Dm,), F32, data["beta"]),
               dout=Guarded(shape, bf, data["dout"]))
    outs = dict(prenorm=Guarded(shape, bf), out=Guarded(shape, bf), mean=Guarded((B, N), F32), rstd=Guarded((B, N), F32), dx=Guarded(shape, bf),
                partials=scratch(B * 2 * Dm))
    if not defer:
        outs.update(dgamma=Guarded((Dm,), F32), dbeta=Guarded((Dm,), F32))
    s = H.scale32(N, Dm)
    nat.call("spv_hadamard_ln_fwd", ins["x"].ptr, outs["prenorm"].ptr, outs["out"].ptr, ins["gamma"].ptr, ins["beta"].ptr, outs["mean"].ptr,
             outs["rstd"].ptr, s, B, N, Dm, 1, _st())
    nat.call("spv_hadamard_ln_bwd", ins["dout"].ptr, outs["prenorm"].ptr, outs["mean"].ptr, outs["rstd"].ptr, ins["gamma"].ptr, outs["dx"].ptr,
             0 if defer else outs["dgamma"].ptr, 0 if defer else outs["dbeta"].ptr, outs["partials"].ptr, s, B, N, Dm, 1, _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, data, dict(partials=B * 2 * Dm))
    got = {k: b.f64() for k, b in outs.items()}
    if defer:   # the caller's fold: slab layout [batch][2][512]
        got["dgamma"], got["dbeta"] = got["partials"][:B * 2 * Dm].reshape(B, 2, Dm).sum(0)
    return data, got


@pytest.mark.parametrize("mode", H.LN_MODES)
@pytest.mark.parametrize("case", H.LN_CASES, ids=H.case_id)
def test_fused_pair_vs_float64(case, mode):
    c = case
    assert _native().call("spv_hadamard_ln_supported", c.tokens, 512, 1) == H.ln_supported("bf16", c.tokens, 512) == 1
    data, got = _fused(c, mode)
    fwd = H.ln_fwd(data["x"], data["gamma"], data["beta"], prenorm=got["prenorm"])
    bwd = H.ln_bwd(data["dout"], got["prenorm"], data["gamma"])
    errs = dict(prenorm=R.err(got["prenorm"], fwd["prenorm"], 1), mean=R.err(got["mean"], fwd["mean"]), rstd=R.err(got["rstd"], fwd["rstd"]),
                out=R.err(got["out"], fwd["out"], 1), dx=R.err(got["dx"], bwd["dx"], 1), dgamma=R.err(got["dgamma"], bwd["dgamma"]),
                dbeta=R.err(got["dbeta"], bwd["dbeta"]), partials=R.err(got["partials"][:c.batch * 1024].reshape(c.batch, 2, 512), bwd["partials"]))
    bars = dict(prenorm=H.bar(H.LN_BAR, "bf16"), mean=H.LN_BAR, rstd=H.LN_BAR, out=H.bar(H.LN_BAR, "bf16"), dx=FUSED_DX_BAR,
                dgamma=H.GRAD_BAR, dbeta=H.GRAD_BAR, partials=H.GRAD_BAR)
    judge(f"hadamard ln {mode} {H.case_id(c)}", errs, bars)


@pytest.mark.parametrize("case", [c for c in H.LN_CASES if c.batch == 3], ids=H.case_id)
def test_fused_pair_equals_the_composition(case):
    """spv_hadamard_mix + spv_add_layernorm_fwd(mode 0) on the same inputs: the same node, kernel by kernel, within the same bars.
    prenorm is compared with spv_hadamard_mix's output; the LayerNorm kernel is then given the FUSED kernel's stored prenorm, as every
    reference here is computed downstream of the kernel's own stored tensor: the two bf16 prenorm tensors differ by one bf16 step
    wherever the fp32 values straddle a rounding boundary (measured: prenorm 1.1e-3 of the sample maximum), and a row mean taken over
    the other tensor then differs by that step / 512 -- measured 5.1e-5 of the largest mean at (3, 16, 512), above LN_BAR with both
    kernels right."""
    nat, c, bf = _native(), case, torch.bfloat16
    B, N, Dm = c.batch, c.tokens, 512
    shape = (B, N, Dm)
    data, got = _fused(c, "fold")
    x, gamma, beta = Guarded(shape, bf, data["x"]), Guarded((Dm,), F32, data["gamma"]), Guarded((Dm,), F32, data["beta"])
    m, own = Guarded(shape, bf), Guarded(shape, bf, got["prenorm"])
    out, mean, rstd = Guarded(shape, bf), Guarded((B, N), F32), Guarded((B, N), F32)
    nat.call("spv_hadamard_mix", x.ptr, m.ptr, 0, B, N, Dm, H.scale32(N, Dm), 1, 0, _st())
    nat.call("spv_add_layernorm_fwd", own.ptr, x.ptr, gamma.ptr, beta.ptr, out.ptr, mean.ptr, rstd.ptr, B * N, Dm, 0, 1, _st())
    torch.cuda.synchronize()
    assert np.array_equal(own.f64(), got["prenorm"])
    errs = dict(prenorm=R.err(got["prenorm"], m.f64(), 1), out=R.err(got["out"], out.f64(), 1), mean=R.err(got["mean"], mean.f64()),
                rstd=R.err(got["rstd"], rstd.f64()))
    bars = dict(prenorm=H.bar(H.LN_BAR, "bf16"), out=H.bar(H.LN_BAR, "bf16"), mean=H.LN_BAR, rstd=H.LN_BAR)
    judge(f"hadamard ln vs composition {H.case_id(c)}", errs, bars)


# ------------------------------------------------------------------------------------------------------------------ C. the row-0 pair
@pytest.mark.parametrize("case", H.CLS_CASES, ids=H.case_id)
def test_row0_pair_vs_float64_and_vs_the_full_node(case):
    nat, c = _native(), case
    dtype, B, N, Dm = DT[c.dtype], c.batch, c.tokens, c.dim
    assert nat.call("spv_hadamard_cls_supported", N, Dm, H.CODE[c.dtype]) == H.cls_supported(c.dtype, N, Dm) == 1
    rng = H.rng_of(c)
    data = dict(x=H.normal(rng, (B, N, Dm), c.dtype), g1=H.normal(rng, (B, Dm), c.dtype))
    data["gamma"], data["beta"] = H.affine(rng, Dm)
    ins = dict(x=Guarded((B, N, Dm), dtype, data["x"]), g1=Guarded((B, Dm), dtype, data["g1"]), gamma=Guarded((Dm,), F32, data["gamma"]),
               beta=Guarded((Dm,), F32, data["beta"]))
    outs = dict(out=Guarded((B, Dm), dtype), m0=Guarded((B, Dm), F32), mean=Guarded((B,), F32), rstd=Guarded((B,), F32),
                dx=Guarded((B, N, Dm), dtype), partials=scratch(B * 2 * Dm))
    s = H.scale32(N, Dm)
    nat.call("spv_hadamard_cls_fwd", ins["x"].ptr, ins["gamma"].ptr, ins["beta"].ptr, outs["out"].ptr, outs["m0"].ptr, outs["mean"].ptr,
             outs["rstd"].ptr, s, B, N, Dm, H.CODE[c.dtype], _st())
    nat.call("spv_hadamard_cls_bwd", ins["g1"].ptr, outs["m0"].ptr, outs["mean"].ptr, outs["rstd"].ptr, ins["gamma"].ptr, outs["dx"].ptr,
             outs["partials"].ptr, s, B, N, Dm, H.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, data, dict(partials=B * 2 * Dm))
    got = {k: b.f64() for k, b in outs.items()}
    fwd = H.cls_fwd(data["x"], data["gamma"], data["beta"], m0=got["m0"])
    bwd = H.cls_bwd(data["g1"], got["m0"], data["gamma"], N)
    errs = dict(m0=R.err(got["m0"], fwd["m0"], 1), mean=R.err(got["mean"], fwd["mean"]), rstd=R.err(got["rstd"], fwd["rstd"]),
                out=R.err(got["out"], fwd["out"], 1), dx=R.err(got["dx"], bwd["dx"], 1),
                partials=R.err(got["partials"][:B * 2 * Dm].reshape(B, 2, Dm), bwd["partials"]))
    bars = dict(m0=H.TRANSFORM_BAR, mean=H.LN_BAR, rstd=H.LN_BAR, out=H.bar(H.LN_BAR, c.dtype), dx=H.bar(H.GRAD_BAR, c.dtype), partials=H.GRAD_BAR)
    # row 0 of the full node, float64: the same numbers
    full = H.ln_fwd(data["x"], data["gamma"], data["beta"])
    errs["out_vs_full"] = R.err(got["out"], full["out"][:, 0], 1)
    bars["out_vs_full"] = H.bar(H.LN_BAR, c.dtype)
    judge(f"hadamard cls {H.case_id(c)}", errs, bars)


# ------------------------------------------------------------------------------------------------------------------ D. autograd
@pytest.mark.parametrize("shape,dtn", [((2, 5, 24), "fp32"), ((2, 65, 512), "bf16")])
def test_hadamard_mixer_module_forward_and_backward(shape, dtn):
    from spectre_vit.modules.mixers import HadamardMixer
    rng = np.random.default_rng(shape[1])
    x64, dy64 = H.normal(rng, shape, dtn), H.normal(rng, shape, dtn)
    x = t(x64, DT[dtn]).requires_grad_(True)
    mix = HadamardMixer()
    assert copy.deepcopy(mix).normalize and not list(mix.parameters())
    y = mix(x)
    y.backward(t(dy64, DT[dtn]))
    torch.cuda.synchronize()
    assert y.shape == x.shape and y.dtype == x.dtype
    errs = dict(y=R.err(n64(y), H.mix(x64), 1), dx=R.err(n64(x.grad), H.mix(dy64), 1))
    judge(f"HadamardMixer {shape} {dtn}", errs, dict(y=H.bar(H.TRANSFORM_BAR, dtn), dx=H.bar(H.TRANSFORM_BAR, dtn)))
    raw = HadamardMixer(normalize=False)(x.detach())
    assert R.err(n64(raw), H.mix(x64, normalize=False), 1) <= H.bar(H.TRANSFORM_BAR, dtn)


# ------------------------------------------------------------------------------------------------------------------ E. the whole model
def _route_hadamard(monkeypatch):
    real_fwd, real_bwd = O.mixer_fwd, O.mixer_bwd

    def fwd(x, lp, mixer):
        return (H.mix(x), None) if mixer == "hadamard" else real_fwd(x, lp, mixer)

    def bwd(dy, lp, mixer, cache):
        return (H.mix(dy), {}) if mixer == "hadamard" else real_bwd(dy, lp, mixer, cache)

    monkeypatch.setattr(O, "mixer_fwd", fwd)
    monkeypatch.setattr(O, "mixer_bwd", bwd)


_ref_cache = {}


@pytest.mark.parametrize("cls_only", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_hadamard_model_step_vs_float64(dtype, cls_only, monkeypatch):
    """Small widths, 4 layers, bs 128, dropout off: loss, logits, every gradient and the weights after one torch.optim.AdamW step against
    float64; the last layer through the row-0 kernels (default) and over every row"""
    from spectre_vit import hip_ops
    _route_hadamard(monkeypatch)
    m, img, labels, sd = _setup(SMALL, "hadamard", 128, 47)
    if "ref" not in _ref_cache:
        loss, logits, _, grads = O.train_step(img.numpy(), labels.numpy(), sd, 4, 4, "hadamard", np.float64)
        _ref_cache["ref"] = (float(loss), logits, grads)
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
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        errs[k] = rel_l2(p.grad, grads_ref[k])
        if dtype == torch.bfloat16 and p.numel() <= TINY_NUMEL:
            limit[k] = max(bound, TINY_BF16_BOUND)
    worst = max(errs, key=errs.get)
    print(f"hadamard bs128 {dtype} cls_only={cls_only}: worst rel-L2 {errs[worst]:.3e} ({worst}); logits {errs['logits']:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= limit.get(k, bound)}
    assert not bad, bad
    w0 = {k: n64(p) for k, p in m.named_parameters()}
    torch.optim.AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01).step()
    for k, p in m.named_parameters():
        z = np.zeros_like(w0[k])
        w_ref, _, _ = O.adamw_step(w0[k], grads_ref[k], z, z, 1)
        assert rel_l2(p, w_ref) <= bound, (k, rel_l2(p, w_ref))


# ------------------------------------------------------------------------------------------------------------------ F. graphs
def test_graph_replay_gradients_equal_eager_step():
    """one replay of the captured step against the eager bf16 step on the same weights and batch"""
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    m, img, labels, _ = _setup(SMALL, "hadamard", 128, 53)
    m = m.to(dev()).train()
    opt = FusedAdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, capturable=True, static_grads=True)
    torch.cuda.empty_cache()
    step = GraphedTrainStep(m, opt, CrossEntropyLoss(), img.to(dev()), labels.to(dev()), autocast_dtype=torch.bfloat16, warmup=1)
    try:
        sd0 = copy.deepcopy(m.state_dict())
        loss = step()
        torch.cuda.synchronize()
        grads = {k: n64(p.grad) for k, p in m.named_parameters()}
    finally:
        step.close()
    e = SpectreViT(**SMALL, mixer="hadamard").to(dev()).train()
    e.load_state_dict(sd0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = e(img.to(dev()))
    loss_e = torch.nn.CrossEntropyLoss()(logits, labels.to(dev()))
    loss_e.backward()
    bound = BOUND[torch.bfloat16]
    assert abs(loss.item() - loss_e.item()) <= bound * abs(loss_e.item()), (loss.item(), loss_e.item())
    errs = {k: rel_l2(torch.from_numpy(grads[k]), n64(p.grad)) for k, p in e.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"graph replay vs eager (hadamard, bs128): worst gradient rel-L2 {errs[worst]:.3e} ({worst})")
    bad = {k: v for k, v in errs.items() if v > (max(bound, TINY_BF16_BOUND) if grads[k].size <= TINY_NUMEL else bound)}
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inference_session_equals_eager_eval(dtype):
    """the same kernels in the same order: bitwise equal logits and features at a batch equal to a bucket, replayed twice"""
    from spectre_vit.inference import InferenceSession
    m, img, _, _ = _setup(SMALL, "hadamard", 64, 59)
    m = m.to(dev()).eval()
    img = img.to(dev())
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        want, want_cls = m(img, return_features=True)
    with InferenceSession(m, autocast_dtype=torch.bfloat16 if dtype == torch.bfloat16 else None, batch_sizes=(64,), return_features=True) as s:
        got = s(img)
        assert got.dtype == torch.float32 and torch.equal(got, want), (got - want).abs().max().item()
        assert torch.equal(s.features, want_cls)
        assert torch.equal(s(img), want)
