"""GPU checks of SpectreBranch (reference spectre_vit/models/spectre_branch/spectre_branch.py) on the kernels of csrc/spv_branch.hip:
each kernel against float64 numpy (asserting its dispatch-census counter), the whole model against the reference's own fp32 ->
float64 training step (tests/golden/model_spectre_branch*.npz, make_golden_branch.py), bf16 autocast, and the preset's bs-512
step replayed from a HIP graph."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_model import BF16_L2, check_l2, rel_l2
from test_gpu_ops import check, dev, n64, t

pytestmark = pytest.mark.gpu

PRESET = dict(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=768, num_encoders=4, num_heads=8, hidden_dim=256,
              activation="gelu")
STAGES = [(3, 32, 17), (9, 30, 15), (27, 28, 13), (81, 26, 11)]   # (Cin, H, W) of the preset's four conv stages


def count(name):
    from spectre_vit import _native
    return _native.call("spv_path_count", _native.PATH[name])


def bf(a):
    """round to bf16 (the kernel's storage) so numpy sees the same inputs"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


# ---------------------------------------------------------------- float64 references
def np_conv(x, w, b):
    """x (B, H, W, Cin) channels-last, w (Cout, Cin, 3, 3) -> (B, H-2, W-2, Cout)"""
    win = np.lib.stride_tricks.sliding_window_view(x, (3, 3), axis=(1, 2))   # (B, Ho, Wo, Cin, 3, 3)
    return np.einsum("bhwcij,ocij->bhwo", win, w) + b


def np_conv_dgrad(dy, w):
    B, ho, wo, _ = dy.shape
    dx = np.zeros((B, ho + 2, wo + 2, w.shape[1]))
    for ky in range(3):
        for kx in range(3):
            dx[:, ky:ky + ho, kx:kx + wo] += np.einsum("bhwo,oc->bhwc", dy, w[:, :, ky, kx])
    return dx


def np_conv_wgrad(dy, x):
    win = np.lib.stride_tricks.sliding_window_view(x, (3, 3), axis=(1, 2))
    return np.einsum("bhwo,bhwcij->ocij", dy, win)


def np_pool_matrix(L, T):
    P = np.zeros((T, L))
    for i in range(T):
        s, e = (i * L) // T, -((-(i + 1) * L) // T)
        P[i, s:e] = 1.0 / (e - s)
    return P


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("shape", [(3, 3, 32, 32), (2, 1, 28, 28), (2, 3, 17, 9)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_spectrum_log1p(shape, dtype):
    from spectre_vit import branch_ops
    x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    ref = np.log1p(np.abs(np.fft.rfft2(x.astype(np.float64), axes=(-2, -1)))).transpose(0, 2, 3, 1)
    before = count("spectrum")
    y = branch_ops.spectrum_log1p(t(x), dtype)
    assert count("spectrum") == before + 1
    assert y.shape == ref.shape and y.dtype == dtype
    if dtype == torch.float32:
        check(y, ref, 1e-5, "spectrum")
    else:
        check_l2(y, ref, 1e-2, "spectrum bf16")


def test_spectrum_refuses_image_gradients():
    from spectre_vit import branch_ops
    with pytest.raises(RuntimeError, match="no backward"):
        branch_ops.spectrum_log1p(torch.randn(1, 3, 8, 8, device=dev(), requires_grad=True))


@pytest.mark.parametrize("cin,H,W,cout", [(c, h, w, 3 * c) for c, h, w in STAGES] + [(1, 5, 4, 5)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv3x3_fwd_dgrad_wgrad(cin, H, W, cout, dtype):
    from spectre_vit import branch_ops
    rng = np.random.default_rng(cin * 100 + H)
    B = 3
    x = rng.standard_normal((B, H, W, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    dy = rng.standard_normal((B, H - 2, W - 2, cout)).astype(np.float32)
    if dtype == torch.bfloat16:
        x, w, dy = bf(x), bf(w), bf(dy)
    xt, wt, bt, dyt = t(x, dtype), t(w), t(b), t(dy, dtype)
    c0 = (count("conv_fwd"), count("conv_dgrad"), count("conv_wgrad"))
    y = branch_ops.conv3x3_fwd(xt, wt, bt)
    dx = branch_ops.conv3x3_dgrad(dyt, wt)
    dw = branch_ops.conv3x3_wgrad(dyt, xt)
    assert (count("conv_fwd"), count("conv_dgrad"), count("conv_wgrad")) == (c0[0] + 1, c0[1] + 1, c0[2] + 1)
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    refs = dict(y=np_conv(x64, w64, b), dx=np_conv_dgrad(dy64, w64), dw=np_conv_wgrad(dy64, x64))
    assert dw.dtype == torch.float32 and tuple(dw.shape) == w.shape
    for name, got in (("y", y), ("dx", dx), ("dw", dw)):
        assert tuple(got.shape) == refs[name].shape, name
        if dtype == torch.float32:
            check(got, refs[name], 1e-5, f"conv {name}")
        else:
            check_l2(got, refs[name], 1e-2, f"conv bf16 {name}")


@pytest.mark.parametrize("L", [450, 364, 286, 216, 65, 64, 40])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_token_pool_fwd_bwd(L, dtype):
    from spectre_vit import branch_ops
    rng = np.random.default_rng(L)
    B, C, T, ldo = 2, 7, 65, 8
    y = rng.standard_normal((B, L, C)).astype(np.float32)
    dout = rng.standard_normal((B, T, ldo)).astype(np.float32)
    add = rng.standard_normal((B, L, C)).astype(np.float32)
    if dtype == torch.bfloat16:
        y, dout, add = bf(y), bf(dout), bf(add)
    P = np_pool_matrix(L, T)
    before = (count("token_pool"), count("token_unpool"))
    out = branch_ops.token_pool_fwd(t(y, dtype), T, ldo)
    dy = branch_ops.token_pool_bwd(t(dout, dtype), L, C)
    dya = branch_ops.token_pool_bwd(t(dout, dtype), L, C, t(add, dtype))
    assert (count("token_pool"), count("token_unpool")) == (before[0] + 1, before[1] + 2)
    ref = np.einsum("tl,blc->btc", P, y.astype(np.float64))
    dref = np.einsum("tl,btc->blc", P, dout[..., :C].astype(np.float64))
    assert not n64(out)[..., C:].any()   # the GEMM pad columns are zero
    tol = 1e-6 if dtype == torch.float32 else 1e-2
    assert rel_l2(out[..., :C], ref) <= tol and rel_l2(dy, dref) <= tol and rel_l2(dya, dref + add) <= tol


# ---------------------------------------------------------------- the model against the reference's training step
@pytest.fixture(scope="module")
def golden():
    d = dict(np.load(os.path.join(GOLDEN, "model_spectre_branch.npz")))
    d.update(np.load(os.path.join(GOLDEN, "model_spectre_branch_after.npz")))
    return d


def build(seed, **kw):
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranch
    torch.manual_seed(seed)
    return SpectreBranch(**dict(PRESET, dropout=0.0, **kw)).to(dev())   # drawn on the CPU exactly as the reference's


def matrix(a):
    return a.reshape(-1, a.shape[-1]) if a.shape[0] == 1 else a.reshape(a.shape[0], -1)


def compare(d, prefix, got, cmp, sum_cmp=None):
    """got vs the fixture: whole tensors, or (row sums, column sums, 8 rows) of the larger ones (make_golden_branch.summary).  A sum
    is measured against the scale of what it adds up (its terms' magnitude times the square root of their count), not against its
    own value: some sums vanish by construction (LayerNorm's input gradient sums to zero over the features, so the column sums of
    linear3's weight gradient are ~1e-17 in float64 and ~1e-9 in fp32), and the patch tokens of this model get no gradient at all
    (the head reads the CLS row and nothing mixes tokens), so the patch embedding's gradients are exactly zero."""
    a = n64(got)
    assert np.isfinite(a).all(), f"{prefix}: non-finite values"
    if prefix in d:
        cmp(a, d[prefix], prefix, 0.0)
        return
    m = matrix(a)
    rows = d[prefix + ".rows"].astype(np.float64)
    scale = np.abs(rows).max()
    sum_cmp = sum_cmp or cmp
    sum_cmp(m.sum(1), d[prefix + ".rowsum"], prefix + " row sums", scale * np.sqrt(m.shape[1]))
    sum_cmp(m.sum(0), d[prefix + ".colsum"], prefix + " column sums", scale * np.sqrt(m.shape[0]))
    cmp(m[np.linspace(0, m.shape[0] - 1, 8).astype(np.int64)], rows, prefix + " rows", 0.0)


def maxnorm(tol):
    def cmp(a, ref, what, floor):
        ref = np.asarray(ref, np.float64)
        e = np.abs(a - ref).max() / (max(np.abs(ref).max(), floor) + 1e-30)
        assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    return cmp


def l2(tol):
    def cmp(a, ref, what, floor):
        ref = np.asarray(ref, np.float64)
        e = np.linalg.norm(a - ref) / (max(np.linalg.norm(ref), floor * np.sqrt(ref.size)) + 1e-300)
        assert e <= tol, f"{what}: rel-L2 {e:.3e} > {tol:.1e}"
    return cmp


def adam_first_step_check(got, ref, gref, what, lr=1e-3, eps=1e-8, grad_tol=3e-4, tol=2e-4):
    """post-AdamW weights of a tensor stored whole.  The first AdamW step moves an entry by lr * g / (|g| + eps): its sensitivity to
    an error in g is lr * eps / (|g| + eps)^2, 1e-3 / |g| for |g| ~ eps -- 6e3 for the stage-3 conv bias entry whose reference
    gradient is 3.0e-8 (2.4e-6 of that tensor's largest).  An fp32 error of 3.6e-9 in it (3e-7 of the scale, within the gradient
    bound) moves that one weight by 2.2e-5, 5.8e-4 of the tensor's largest weight.  So each entry is allowed `tol` of the weight
    scale plus the gradient bound (`grad_tol` of the largest gradient) carried through that sensitivity."""
    ref, gref = np.asarray(ref, np.float64), np.asarray(gref, np.float64)
    carried = lr * eps / (np.abs(gref) + eps) ** 2 * grad_tol * np.abs(gref).max()
    bound = tol * np.abs(ref).max() + carried
    worst = np.argmax(np.abs(got - ref) - bound)
    assert (np.abs(got - ref) <= bound).all(), f"after-AdamW {what}: entry {worst} off by {abs(got - ref).flat[worst]:.3e} > {bound.flat[worst]:.3e}"


def test_model_train_step_golden(golden):
    """fp32 kernels vs the reference's forward / CE / backward / AdamW step (same seed, same weights, same image), at the bounds of
    test_gpu_model.test_model_train_step_golden.  Post-AdamW weights: tensors stored whole get 2e-4 plus the gradient bound carried
    through the first Adam step (adam_first_step_check).  Tensors stored as summaries get 3e-4 on their rows (measured 2.17e-4 before
    the carried term existed, on layers.0.norm1.bias: zero-initialised, so one lr step is its whole scale) and 1e-3 on their row /
    column sums, which add up to 1536 such update errors (measured 3.4e-4 on spectre_project.2.weight's row sums, a third of one lr
    step against sums of order 1)."""
    d = golden
    m = build(int(d["cfg.seed"])).train()
    mix_before = {k: p.detach().clone() for k, p in m.named_parameters() if ".mix_layer." in k}
    img, labels = t(d["img"]), torch.from_numpy(d["labels"]).to(dev())
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
    with torch.no_grad():
        _, feats = m.encoder_blocks.spectre_branch(img)
    for k, f in enumerate(feats):
        check(f.reshape(-1, f.shape[-1])[torch.from_numpy(d["feat_rows"]).to(dev())], d[f"feats.{k}"], 5e-5, f"feats[{k}]")
    logits, cls = m(img, return_features=True)
    loss = torch.nn.CrossEntropyLoss()(logits, labels)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    check(logits, d["logits"], 5e-5, "logits")
    check(cls, d["cls"], 5e-5, "cls")
    assert abs(loss.item() - float(d["loss"])) < 5e-5 * abs(float(d["loss"]))
    for k, p in m.named_parameters():
        if "nograd." + k in d:
            assert p.grad is None, k
        else:
            compare(d, "grad." + k, p.grad, maxnorm(3e-4))
    assert all(m.encoder_blocks.layers[i].mix_layer.weight.grad is None for i in range(PRESET["num_encoders"]))
    opt.step()
    for k, p in m.named_parameters():
        if "after." + k in d and "grad." + k in d:
            adam_first_step_check(n64(p), d["after." + k], d["grad." + k], k)
        else:
            compare(d, "after." + k, p, maxnorm(3e-4), maxnorm(1e-3))
    for k, v in mix_before.items():
        assert torch.equal(dict(m.named_parameters())[k], v), k   # never updated, not even by weight decay
    with torch.no_grad():
        check(m(img), n64(m(img, return_features=True)[0]), 0.0, "return_features=False logits")


def test_model_bf16_autocast(golden):
    d = golden
    m = build(int(d["cfg.seed"])).train()
    img, labels = t(d["img"]), torch.from_numpy(d["labels"]).to(dev())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits, cls = m(img, return_features=True)
    loss = torch.nn.CrossEntropyLoss()(logits.float(), labels)
    loss.backward()
    check_l2(logits, d["logits"], BF16_L2, "logits")
    check_l2(cls, d["cls"], BF16_L2, "cls")
    for k, p in m.named_parameters():
        if "nograd." + k in d:
            assert p.grad is None, k
        else:
            compare(d, "grad." + k, p.grad, l2(BF16_L2))


def test_spectre_mix_golden(golden):
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreMix
    d = golden
    m = SpectreMix(64, 2, 5).to(dev())
    m.load_state_dict({k[len("mix.sd."):]: torch.from_numpy(v) for k, v in d.items() if k.startswith("mix.sd.")}, strict=True)
    x = t(d["mix.x"]).requires_grad_(True)
    y = m(x)
    y.backward(t(d["mix.dy"]))
    check(y, d["mix.y"], 1e-5, "y")
    check(x.grad, d["mix.dx"], 1e-5, "dx")
    for k, p in m.named_parameters():
        check(p.grad, d["mix.grad." + k], 1e-5, "grad " + k)


# ---------------------------------------------------------------- the preset's bs-512 step, replayed from a HIP graph
def _graphed(m, img, labels):
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.optim import FusedAdamW
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True)
    return GraphedTrainStep(m, opt, CrossEntropyLoss(), img, labels, warmup=3), opt


def test_bench_shape_graphed_steps_learn():
    from spectre_vit import harness
    from spectre_vit.configs.parser import parse_config
    c = parse_config("spectre_vit/configs/spectre_branch.py")
    c.dropout = 0.001
    data = harness.SyntheticCifar(2048, c, dev(), seed=5)
    batches = list(data.batches(512, True, torch.Generator().manual_seed(0)))
    m = harness.build_model(c, model="spectre_branch", device=dev()).train()
    mix = [l.mix_layer.weight.detach().clone() for l in m.encoder_blocks.layers]
    img0, lab0 = batches[0]
    step, _ = _graphed(m, img0.clone(), lab0.long())
    losses = []
    for i in range(20):
        img, lab = batches[i % len(batches)]
        losses.append(step(img, lab.long()).item())
    step.close()
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-4:]) < np.mean(losses[:4]), losses
    for l, w in zip(m.encoder_blocks.layers, mix):
        assert l.mix_layer.weight.grad is None and torch.equal(l.mix_layer.weight, w)


def test_bench_shape_graphed_matches_eager():
    from spectre_vit import hip_ops
    from spectre_vit.loss import CrossEntropyLoss
    from spectre_vit.optim import FusedAdamW
    g = torch.Generator().manual_seed(9)
    img = torch.randn(512, 3, 32, 32, generator=g).to(dev())
    labels = torch.randint(0, 100, (512,), generator=g).to(dev())
    crit = CrossEntropyLoss()
    m1 = build(21).train()
    o1 = FusedAdamW(m1.parameters(), lr=1e-3, weight_decay=0.01, capturable=True)
    eager = []
    for _ in range(6):   # GraphedTrainStep runs 3 warm-up steps before the capture
        o1.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m1(img)
        loss = crit(out, labels)
        loss.backward()
        o1.step()
        eager.append(loss.item())
    m2 = build(21).train()
    keep = hip_ops._WGRAD_HOLD
    hip_ops._WGRAD_HOLD = False
    try:
        step, _ = _graphed(m2, img, labels)
        graph = [step().item() for _ in range(3)]
        step.close()
    finally:
        hip_ops._WGRAD_HOLD = keep
    np.testing.assert_allclose(graph, eager[3:], rtol=1e-3)
    # the six updates of the whole model, graph against eager: the replay writes the gradients into the bucket's slots, whose
    # alignment can pick other GEMM kernels (other fp32 summation orders), and AdamW turns such differences in near-zero gradient
    # entries into up to a whole lr step each (a zero-initialised bias is nothing but those steps), so the measure is the update
    # vector of the model, not one tensor's entries
    p0 = [p.detach() for p in build(21).parameters()]
    d1 = torch.cat([(p - q).flatten() for p, q in zip(m1.parameters(), p0)])
    d2 = torch.cat([(p - q).flatten() for p, q in zip(m2.parameters(), p0)])
    assert float((d2 - d1).norm() / d1.norm()) <= 1e-2
