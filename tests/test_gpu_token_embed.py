"""spv_token_embed_fwd (csrc/spv_patch.hip: token_embed_kernel) against the call it replaces and against float64: raw C-ABI calls with an
explicit seed, eagerly, with no graph open, so live_seed(seed) == seed.

Every run asserts: (a) the output equals spv_gemm_nt_grouped_rows_drop's on the same inputs and seed bit for bit; (b) it lies within the
bar tests/test_gpu_gemm_edges.py holds a bf16 output of the tile kernel to, u |ref| + (n + 2) 2^-24 S, against tests/gemm_ref.py's float64
reference with the position rows as its 2-D bias and tests/dropout_ref.py's mask; (c) it is exactly zero where that mask drops, and
elsewhere only where the reference itself lies within the fp32 part of its bar; (d) every CLS row (a zero patch row) is
bf16(posbias[0] * scale) exactly; (e) the sentinels around all four buffers are intact and the inputs unchanged.

Shapes (images x tokens, n, k): fewer rows than one 32-row block; four blocks and a ragged one over eight column shares; the largest k;
258 blocks; and -- added to the four the kernel was specified with, because this kernel sizes its grid in WAVES (12 per CU, a wave per
column share) and so walks 258 blocks of 8 shares in one trip on 256 CUs -- 393 blocks, which 3072 resident waves take as 197 walkers of
two blocks and the last of one: the persistent loop, its prefetch of the next block and its uneven last share.

The whole path: hip_ops.patch_embed forward and backward under autograd, and a graph-replayed training step, with
hip_ops.TOKEN_EMBED_KERNEL on and off."""
import collections

import numpy as np
import pytest
import torch

import dropout_ref as D
import gemm_edge_cases as C
import gemm_ref as R
from test_gpu_attention_edges import Guarded
from test_gpu_bench_shapes import census
from test_gpu_permut_edges import raw_bits

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(3, 5, 64, 16), (2, 65, 512, 48), (1, 65, 128, 64), (127, 65, 512, 48), (193, 65, 512, 48)]
PS = (0.0, 0.3)


def problem(shape, p):
    """float64 storage-exact inputs and the reference of one run"""
    B, T, n, k = shape
    rng = C.rng_of("token_embed", shape)
    A = C.draw(rng, (B * T, k), "bf16", "normal")
    A[::T] = 0.0   # the CLS slot of every image: a zero patch row
    W = C.draw(rng, (n, k), "bf16", "normal")
    pb = C.draw(rng, (T, n), "fp32", "normal")
    ref, S, kept = R.nt(A, W, None, pb, T, T, 0, drop=(C.SEED, p) if p > 0 else None, ldc=n)
    return dict(A=A, W=W, pb=pb, ref=ref, S=S, kept=kept)


@pytest.mark.parametrize("p", PS, ids=lambda p: f"p{p}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{}x{}-{}-{}".format(*s))
def test_token_embed_vs_tile_kernel_and_float64(shape, p):
    from spectre_vit import _native, hip_ops
    B, T, n, k = shape
    rows = B * T
    d = problem(shape, p)
    assert _native.call("spv_token_embed_supported", rows, n, k, 1) == 1
    a, w, pb = Guarded((rows, k), BF, d["A"]), Guarded((n, k), BF, d["W"]), Guarded((T, n), F32, d["pb"])
    new, old = Guarded((rows, n), BF), Guarded((rows, n), BF)
    bits = {name: raw_bits(b.t).copy() for name, b in dict(a=a, w=w, pb=pb).items()}
    seed, st = (C.SEED if p > 0 else 0), hip_ops._stream()
    before = census()
    _native.call("spv_token_embed_fwd", a.ptr, w.ptr, pb.ptr, new.ptr, rows, n, k, T, p, seed, st)
    torch.cuda.synchronize()
    assert census() == before   # no census slot: the new kernel is told apart on the host
    _native.call("spv_gemm_nt_grouped_rows_drop", a.ptr, w.ptr, 0, pb.ptr, old.ptr, rows, n, k, k, k, n, 1, 1, T, T, 0, p, seed, st)
    torch.cuda.synchronize()
    # (e) memory
    for name, b in dict(a=a, w=w, pb=pb, new=new, old=old).items():
        assert b.intact(), f"{name}: sentinel overwritten"
    for name, b in dict(a=a, w=w, pb=pb).items():
        assert np.array_equal(raw_bits(b.t), bits[name]), f"input {name} changed"
    got = new.f64()
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} elements left unwritten or NaN"
    # (a) the bits of the call it replaces
    same = raw_bits(new.t) == raw_bits(old.t)
    print(f"TOKEN_EMBED {shape} p={p}: {int((~same).sum())} of {same.size} elements differ from the tile kernel's")
    assert same.all()
    # (b) float64, the bar of a bf16 output of the tile kernel
    chain = k + 1 + 1 + (2 if p > 0 else 0)   # gemm_edge_cases.nt_chain: K products, one slab, the 2-D bias, the dropout factor
    ok, worst = C.worst_ratio(got, d["ref"], C.bar(d["ref"], d["S"], chain, "bf16"))
    print(f"TOKEN_EMBED {shape} p={p}: worst ratio to the bar = {worst:.3f}")
    assert ok, worst
    # (c) zero exactly where the mask drops; elsewhere only where the reference is zero to within the fp32 part of its bar
    if p > 0:
        assert 0.2 < 1.0 - d["kept"].mean() < 0.4   # (p = 0.3 over at least 960 elements)
        assert (got[~d["kept"]] == 0).all(), "a dropped element is not zero"
    stray = d["kept"] & (got == 0)
    assert (np.abs(d["ref"][stray]) <= C.bar(d["ref"], d["S"], chain, "fp32")[stray]).all(), "a kept element is zero"
    # (d) the CLS rows: + 0 + posbias[0], times the factor, one rounding
    f = np.where(d["kept"][::T], np.float32(D.inv_keep(p)), np.float32(0.0)).astype(np.float32) if p > 0 else np.ones((B, n), np.float32)
    want = C.q((d["pb"][0].astype(np.float32)[None, :] * f).astype(np.float32), "bf16")
    assert np.array_equal(got[::T], want), "a CLS row is not bf16(posbias[0] * scale)"


def _embed_once(on, p_drop=0.3):
    from spectre_vit import hip_ops
    g = torch.Generator().manual_seed(5)
    B, Cn, H, P, E = 4, 3, 8, 4, 64
    K, T = Cn * P * P, (H // P) ** 2 + 1
    img = torch.randn(B, Cn, H, H, generator=g).cuda()
    w = torch.randn(E, K, generator=g).cuda().requires_grad_()
    bias, cls = torch.randn(E, generator=g).cuda().requires_grad_(), torch.randn(1, 1, E, generator=g).cuda().requires_grad_()
    pos = torch.randn(1, T, E, generator=g).cuda().requires_grad_()
    dtok = torch.randn(B, T, E, generator=g).cuda().to(BF)
    keep = hip_ops.TOKEN_EMBED_KERNEL
    hip_ops.TOKEN_EMBED_KERNEL = on
    counts = collections.Counter(hip_ops.PATH_COUNTS)
    try:
        torch.manual_seed(77)   # the node draws its dropout seed from torch's generator
        with torch.autocast("cuda", dtype=BF):
            tokens = hip_ops.patch_embed(img, w, bias, cls, pos, P, None, p_drop)
        tokens.backward(dtok)
        torch.cuda.synchronize()
    finally:
        hip_ops.TOKEN_EMBED_KERNEL = keep
    moved = {key: v - counts[key] for key, v in hip_ops.PATH_COUNTS.items() if v != counts[key]}
    return tokens.detach().clone(), [t.grad.detach().clone() for t in (w, bias, cls, pos)], moved


def test_patch_embed_forward_and_backward_are_bit_equal_with_the_switch_on_and_off():
    tok_on, grads_on, moved_on = _embed_once(True)
    tok_off, grads_off, moved_off = _embed_once(False)
    assert tok_on.dtype == BF and tok_on.shape == (4, 5, 64)
    assert moved_on.pop("token_embed") == 1 and "token_embed" not in moved_off
    assert moved_on == moved_off, (moved_on, moved_off)   # everything else of the node took the same paths
    assert torch.equal(tok_on.view(torch.int16), tok_off.view(torch.int16))
    dropped = float((tok_on == 0).float().mean())
    assert 0.15 < dropped < 0.45, dropped   # the dropout ran (p = 0.3 over 1280 elements) ...
    for a, b, name in zip(grads_on, grads_off, ("w", "bias", "cls", "pos")):
        assert torch.equal(a, b), name   # ... and the backward found the same mask
    assert float(grads_on[0].abs().sum()) > 0


def test_whole_step_is_bit_equal_with_the_switch_on_and_off():
    """the model of test_gpu_step_prologue.test_whole_step_is_bit_equal_and_issues_one_prologue_call, replayed for two steps"""
    from spectre_vit import _native, hip_ops
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    cfg = dict(img_size=8, patch_size=4, in_channels=3, num_classes=10, embed_dim=64, num_encoders=2, num_heads=4, hidden_dim=96,
               dropout=0.1, activation="gelu", mixer="fft")
    g = torch.Generator().manual_seed(9)
    img = torch.randn(4, 3, 8, 8, generator=g).cuda()
    labels = torch.randint(0, 10, (4,), generator=g).cuda()
    orig = _native.call

    def run(on):
        keep = hip_ops.TOKEN_EMBED_KERNEL
        hip_ops.TOKEN_EMBED_KERNEL = on
        log = collections.Counter()

        def spy(name, *a):
            log[name] += 1
            return orig(name, *a)
        _native.call = spy
        try:
            torch.manual_seed(33)
            m = SpectreViT(**cfg).cuda().train()
            opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True)
            step = GraphedTrainStep(m, opt, torch.nn.CrossEntropyLoss(), img, labels, autocast_dtype=BF, warmup=2)
            try:
                losses = [step(img, labels).detach().clone() for _ in range(2)]
                torch.cuda.synchronize()
                return losses, {k: p.detach().clone() for k, p in m.named_parameters()}, log
            finally:
                step.close()
        finally:
            _native.call = orig
            hip_ops.TOKEN_EMBED_KERNEL = keep

    la, pa, log_on = run(True)
    lb, pb, log_off = run(False)
    assert log_on["spv_token_embed_fwd"] == 3 and log_on["spv_gemm_nt_grouped_rows_drop"] == 0, log_on   # two warm-up steps and the capture
    assert log_off["spv_token_embed_fwd"] == 0 and log_off["spv_gemm_nt_grouped_rows_drop"] == 3, log_off
    for x, y in zip(la, lb):
        assert torch.equal(x, y), (la, lb)
    assert float(la[0]) != float(la[1])   # two different steps (dropout masks move with the seed word)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
