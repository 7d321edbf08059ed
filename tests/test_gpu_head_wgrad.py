"""The class head's parameter gradients on their own launch (spv_small_sl_bwd_w: dW = dh^T xs in 256-thread workgroups of 8 row groups x
32 columns, and the 16-slice fold of dgamma / dbeta / dbias) against float64, at the tolerance tests/test_gpu_ops.py::test_cls_head_vs_oracle
holds these gradients to; and the held form (issued beside the batched layer weight gradients) against the launch in place, bit for bit."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 4e-5   # test_cls_head_vs_oracle: tol * 2 on dW, db, dgamma, dbeta

# rows 5 / 37 / 512 (2, 10 and 128 partial slabs); n 7 (odd: the last output pair is clamped), 10, 100; k 24 (below one 32-column block),
# 200 (a partial block), 512 -- every combination the kernel family accepts (n <= k) -- and the partial-slab counts 1 (rows 3) and 131
# (rows 523: past the fold's first round of 16 slices x 8 loads)
CASES = [c for c in itertools.product((5, 37, 512), (7, 10, 100), (24, 200, 512)) if c[1] <= c[2]] + [(3, 10, 24), (523, 100, 200)]


@pytest.mark.parametrize("rows,n,k", CASES)
def test_weights_entry_vs_float64(rows, n, k):
    from spectre_vit import _native
    assert _native.call("spv_small_sl_supported", rows, n, k)
    nparts = (rows + 3) // 4
    assert _native.call("spv_small_sl_partial_floats", rows, n) == nparts * 3 * n
    rng = np.random.default_rng(rows * 1009 + n * 31 + k)
    dh = torch.from_numpy(rng.standard_normal((rows, n)).astype(np.float32)).cuda()
    xs = torch.from_numpy(rng.standard_normal((rows, k)).astype(np.float32)).cuda()
    partials = torch.from_numpy(rng.standard_normal((nparts, 3, n)).astype(np.float32)).cuda()
    guard = 7.5
    dW = torch.full((n * k + 64,), guard, device="cuda")
    vecs = torch.full((3, n + 64), guard, device="cuda")
    _native.call("spv_small_sl_bwd_w", dh.data_ptr(), xs.data_ptr(), partials.data_ptr(), dW.data_ptr(), vecs[0].data_ptr(), vecs[1].data_ptr(),
                 vecs[2].data_ptr(), rows, n, k, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref_w = dh.double().cpu().numpy().T @ xs.double().cpu().numpy()
    ref_v = partials.double().cpu().numpy().sum(axis=0)
    got_w = dW[:n * k].view(n, k).double().cpu().numpy()
    e = np.abs(got_w - ref_w).max() / np.abs(ref_w).max()
    print(f"rows={rows} n={n} k={k}: dW rel err {e:.3e}")
    assert e <= TOL, f"dW: rel err {e:.3e} > {TOL:.1e}"
    for i, name in enumerate(("dgamma", "dbeta", "dbias")):
        e = np.abs(vecs[i, :n].double().cpu().numpy() - ref_v[i]).max() / np.abs(ref_v[i]).max()
        print(f"rows={rows} n={n} k={k}: {name} rel err {e:.3e}")
        assert e <= TOL, f"{name}: rel err {e:.3e} > {TOL:.1e}"
    # nothing written past the outputs
    assert float(dW[n * k:].min()) == guard == float(dW[n * k:].max())
    assert float(vecs[:, n:].min()) == guard == float(vecs[:, n:].max())


@pytest.mark.parametrize("rows,n,k", [(37, 7, 200), (512, 100, 512)])
def test_old_entry_is_the_two_launches(rows, n, k):
    """spv_small_sl_bwd == spv_small_sl_bwd_rows then spv_small_sl_bwd_w, bit for bit"""
    from spectre_vit import _native
    rng = np.random.default_rng(rows + n + k)

    def r(*shape):
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    dout, h, xs, W = r(rows, n), r(rows, n), r(rows, k), r(n, k)
    mean, rstd, gamma, beta = r(rows), r(rows).abs() + 0.5, r(n), r(n)
    st = torch.cuda.current_stream().cuda_stream
    nparts = (rows + 3) // 4

    def bufs():
        return dict(dh=torch.zeros(rows, n, device="cuda"), dx=torch.zeros(rows, k, device="cuda"), dW=torch.zeros(n, k, device="cuda"),
                    dg=torch.zeros(n, device="cuda"), dbe=torch.zeros(n, device="cuda"), db=torch.zeros(n, device="cuda"),
                    part=torch.zeros(nparts * 3 * n, device="cuda"))
    a, b = bufs(), bufs()
    P = lambda t: t.data_ptr()
    _native.call("spv_small_sl_bwd", P(dout), P(h), P(xs), P(mean), P(rstd), P(W), P(gamma), P(beta), P(a["dh"]), P(a["dx"]), P(a["dW"]), P(a["dg"]),
                 P(a["dbe"]), P(a["db"]), P(a["part"]), rows, n, k, 0, st)
    _native.call("spv_small_sl_bwd_rows", P(dout), P(h), P(mean), P(rstd), P(W), P(gamma), P(beta), P(b["dh"]), P(b["dx"]), P(b["part"]), rows, n, k,
                 0, st)
    _native.call("spv_small_sl_bwd_w", P(b["dh"]), P(xs), P(b["part"]), P(b["dW"]), P(b["dg"]), P(b["dbe"]), P(b["db"]), rows, n, k, st)
    torch.cuda.synchronize()
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_held_form_inside_a_graph_is_bit_equal():
    """a tiny SpectreViT, graph-replayed: the head's weights launch held for the end of the embedding's backward (beside the batched
    layer weight gradients) leaves every gradient and every parameter exactly as the launch in place does"""
    from spectre_vit import hip_ops
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    cfg = dict(img_size=8, patch_size=4, in_channels=3, num_classes=10, embed_dim=64, num_encoders=2, num_heads=4, hidden_dim=96,
               dropout=0.0, activation="gelu", mixer="fft")
    g = torch.Generator().manual_seed(5)
    img = torch.randn(4, 3, 8, 8, generator=g).cuda()
    labels = torch.randint(0, 10, (4,), generator=g).cuda()

    def run(hold):
        keep = hip_ops.HEAD_WGRAD_HOLD
        hip_ops.HEAD_WGRAD_HOLD = hold
        held0 = hip_ops.PATH_COUNTS["head_wgrad_held"]
        try:
            torch.manual_seed(21)
            m = SpectreViT(**cfg).cuda().train()
            opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True)
            step = GraphedTrainStep(m, opt, torch.nn.CrossEntropyLoss(), img, labels, autocast_dtype=torch.bfloat16, warmup=1)
            try:
                for _ in range(2):
                    loss = step(img, labels)
                torch.cuda.synchronize()
                assert not hip_ops._held_head
                return (loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()},
                        {k: p.detach().clone() for k, p in m.named_parameters()}, hip_ops.PATH_COUNTS["head_wgrad_held"] - held0)
            finally:
                step.close()
        finally:
            hip_ops.HEAD_WGRAD_HOLD = keep

    l0, g0, p0, n0 = run(False)
    l1, g1, p1, n1 = run(True)
    assert n0 == 0 and n1 == 2, (n0, n1)   # one warm-up step and the capture
    assert torch.equal(l0, l1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"grad {k}"
        assert torch.equal(p0[k], p1[k]), f"param {k}"
