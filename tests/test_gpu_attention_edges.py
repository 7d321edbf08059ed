"""Every attention kernel family of csrc/spv_attn.hip (v1 general, v2 LDS-staged, v3 bf16 MFMA flash, the row-0 pair) at its edges
against tests/dropout_ref.py's float64 reference, with the attention-probability dropout on: raw C-ABI calls with an explicit seed,
the mask predicted on the host (tests/test_gpu_dropout_mask.py pins that prediction to the device).

Every case (tests/attention_edge_cases.py) runs twice -- run A: standard-normal inputs, p = 0; run B: q and k scaled by 2, p = 0.3 --
and asserts three things: the dispatch census moved by {its family: 2} and nothing else, the sentinels around (and the pad columns
inside) every buffer are intact, and ctx, dq, dk, dv each match float64 per (sequence, head) block, max |got - ref| / max |ref| over
the block, within the bars of test_gpu_model.test_attention_core_vs_oracle (gradients: twice the ctx bar).  Outputs start as NaN, so an
element nobody writes fails.  tests/test_dropout_ref.py checks on the CPU that the reference's own rounding floor on these inputs
stays within a quarter (fp32) resp. half (bf16) of every bar."""
import numpy as np
import pytest
import torch

import attention_edge_cases as C
import dropout_ref as D
from test_dropout_ref import bar
from test_gpu_bench_shapes import census
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
PAD = 256          # sentinel elements before and after every buffer
SENT = -7680.0     # exact in bf16


class Guarded:
    """a tensor inside a larger allocation: PAD sentinels (+ `off` elements, to misalign the pointer) before it and PAD after it;
    filled from `data`, or with NaN"""

    def __init__(self, shape, dtype, data=None, off=0):
        n = int(np.prod(shape))
        self.big = torch.full((PAD + off + n + PAD,), SENT, dtype=dtype, device=dev())
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.big[self.lo:self.hi].view(shape)
        if data is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)).to(dtype))
        assert self.big.data_ptr() % 16 == 0 and self.ptr % 16 == (off * self.big.element_size()) % 16

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.big[:self.lo] == SENT).all() and (self.big[self.hi:] == SENT).all())

    def f64(self):
        return self.t.detach().float().cpu().numpy().astype(np.float64)


def delta(before):
    now = census()
    return {k: now[k] - before[k] for k in now if now[k] != before[k]}


def judge(tag, dtype, got, ref, names):
    errs = {n: float(D.block_errors(got[n], ref[n]).max()) for n in names}
    print(f"EDGE {tag} " + " ".join(f"{n}={errs[n]:.3e}" for n in names))
    bad = {n: (e, bar(dtype, n)) for n, e in errs.items() if not e <= bar(dtype, n)}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("run", ["A", "B"])
@pytest.mark.parametrize("case", C.CORE_CASES, ids=C.case_id)
def test_attention_core_edges_vs_float64(case, run):
    from spectre_vit import _native, hip_ops
    family, dtn, seqs, L, heads, hd, off_bytes, _ = case
    dtype, E, p = DT[dtn], heads * hd, C.RUNS[run]["p"]
    off = off_bytes // (2 if dtn == "bf16" else 4)
    seed = C.SEED if p > 0 else 0
    qkv64, dctx64 = C.core_inputs(case, run)
    ref = C.core_reference(case, run)
    qkv, dctx = Guarded((seqs, L, 3 * E), dtype, qkv64, off), Guarded((seqs, L, E), dtype, dctx64, off)
    ctx, dqkv = Guarded((seqs, L, E), dtype, off=off), Guarded((seqs, L, 3 * E), dtype, off=off)
    probs, ds = Guarded((seqs, heads, L, L), dtype), Guarded((seqs, heads, L, L), dtype)   # as hip_ops.AttentionFn sizes them
    code, st = hip_ops._dt(qkv.t), hip_ops._stream()
    before = census()
    _native.call("spv_attention_fwd", qkv.ptr, ctx.ptr, probs.ptr, seqs, L, heads, hd, code, p, seed, st)
    _native.call("spv_attention_bwd", dctx.ptr, qkv.ptr, probs.ptr, ds.ptr, dqkv.ptr, seqs, L, heads, hd, code, p, seed, st)
    torch.cuda.synchronize()
    assert delta(before) == {"attn_" + family: 2}, (C.case_id(case), delta(before))
    for name, b in dict(qkv=qkv, dctx=dctx, ctx=ctx, dqkv=dqkv, probs=probs, ds=ds).items():
        assert b.intact(), f"{name}: sentinel overwritten"
    assert np.array_equal(qkv.f64(), qkv64) and np.array_equal(dctx.f64(), dctx64), "an input changed"
    dq, dk, dv = (D.split_heads(a, heads) for a in np.split(dqkv.f64(), 3, axis=-1))
    got = dict(ctx=D.split_heads(ctx.f64(), heads), dq=dq, dk=dk, dv=dv)
    judge(f"{family} {dtn} {C.case_id(case)} {run}", dtn, got, ref, ("ctx", "dq", "dk", "dv"))


@pytest.mark.parametrize("run", ["A", "B"])
@pytest.mark.parametrize("case", C.ROW0_CASES, ids=C.case_id)
def test_attention_row0_edges_vs_float64(case, run):
    """operands padded: ldkv = 2E + cv, ldd = 2E + 2 cv; the pad columns hold sentinels and must stay untouched"""
    from spectre_vit import _native, hip_ops
    dtn, B, N, H, hd = case
    dtype, E, p, cv = DT[dtn], H * hd, C.RUNS[run]["p"], C.CV[dtn]
    es = 2 if dtn == "bf16" else 4
    ldkv, ldd = 2 * E + cv, 2 * E + 2 * cv
    seed = C.SEED if p > 0 else 0
    q64, k64, v64, g64 = C.row0_inputs(case, run)
    ref = C.row0_reference(case, run)
    kv64 = np.concatenate([k64, v64, np.full((B, N, cv), SENT)], axis=-1)
    q0, kv, dctx0 = Guarded((B, E), dtype, q64), Guarded((B, N, ldkv), dtype, kv64), Guarded((B, E), dtype, g64)
    ctx0, probs, dq0 = Guarded((B, E), dtype), Guarded((B, H, N), torch.float32), Guarded((B, E), dtype)
    dkv64 = np.full((B, N, ldd), np.nan)
    dkv64[..., 2 * E:] = SENT
    dkv = Guarded((B, N, ldd), dtype, dkv64)
    code, st = hip_ops._dt(q0.t), hip_ops._stream()
    before = census()
    _native.call("spv_attention_row0_fwd", q0.ptr, kv.ptr, kv.ptr + E * es, ldkv, ctx0.ptr, probs.ptr, B, N, H, hd, code, p, seed, st)
    _native.call("spv_attention_row0_bwd", dctx0.ptr, q0.ptr, kv.ptr, kv.ptr + E * es, ldkv, probs.ptr, dq0.ptr, dkv.ptr, dkv.ptr + E * es,
                 ldd, B, N, H, hd, code, p, seed, st)
    torch.cuda.synchronize()
    assert delta(before) == {"attn_row0_fwd": 1, "attn_row0_bwd": 1}, (C.case_id(case), delta(before))
    for name, b in dict(q0=q0, kv=kv, dctx0=dctx0, ctx0=ctx0, probs=probs, dq0=dq0, dkv=dkv).items():
        assert b.intact(), f"{name}: sentinel overwritten"
    assert np.array_equal(kv.f64(), kv64) and np.array_equal(q0.f64(), q64) and np.array_equal(dctx0.f64(), g64), "an input changed"
    out = dkv.f64()
    assert (out[..., 2 * E:] == SENT).all(), "dK / dV pad columns written"
    got = dict(ctx=D.split_heads(ctx0.f64()[:, None], H), dq=D.split_heads(dq0.f64()[:, None], H), dk=D.split_heads(out[..., :E], H),
               dv=D.split_heads(out[..., E:2 * E], H), probs=probs.f64()[:, :, None, :])
    judge(f"row0 {dtn} {C.case_id(case)} {run}", dtn, got, ref, ("ctx", "dq", "dk", "dv", "probs"))


def test_attention_fn_counts_two_in_one_slot():
    """a forward plus backward through hip_ops.AttentionFn adds 2 to the slot of the family that served it and 0 to the other two"""
    from spectre_vit import hip_ops
    for dtype, shape, family in ((torch.bfloat16, (2, 33, 2 * 3 * 32), "attn_v3"), (torch.float32, (2, 33, 2 * 3 * 32), "attn_v2"),
                                 (torch.float32, (2, 33, 2 * 3 * 20), "attn_v1")):
        x = torch.randn(shape, device=dev()).to(dtype).requires_grad_(True)
        before = census()
        y = hip_ops.AttentionFn.apply(x, 2, 0.0)
        y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
        assert delta(before) == {family: 2}, (dtype, shape, delta(before))
