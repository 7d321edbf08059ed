"""Every SpectreLinear tail kernel of csrc/spv_rowops.hip (lane-contiguous, wide, generic <VEC, MAXI> in its four pooling modes, the
fused tail + LayerNorm-2 pair, the skip-gradient-at-source backward) at its edges against tests/tail_ref.py's float64 reference, with
dropout on: raw C-ABI calls with an explicit seed, the mask predicted on the host (tests/test_gpu_dropout_mask.py pins that prediction
to the device).  Eager mode, no GraphedTrainStep open, so live_seed(seed) == seed.

Every case (tests/tail_edge_cases.py) runs twice -- run A: p = 0; run B: p = 0.3 -- forward then backward, the backward fed the forward's
own mean / rstd, and asserts: the dispatch census moved by exactly what the case's kernel class counts; the sentinels around every
buffer are intact, every input is bit-identical afterwards, no output element is left NaN and `partials` is untouched past the slabs
the grid writes; the outputs are zero exactly where the predicted mask drops; and every output matches float64 within the bars of
tail_edge_cases.bar (fp32: 3e-5 forward, 6e-5 gradients; bf16-stored tensors: 2^-8 more).  The fused kernels re-read the f3 / ds they
stored, so their downstream reference is computed from the kernel's own f3 / ds.  tests/test_tail_ref.py checks on the CPU that the
reference's rounding floor on these inputs stays within a quarter of every fp32 bar."""
import numpy as np
import pytest
import torch

import tail_edge_cases as C
from oracle import spectre_oracle as O
from test_gpu_attention_edges import Guarded, delta
from test_gpu_bench_shapes import census
from test_gpu_ops import TOL, check, q

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F32 = torch.float32


@pytest.mark.parametrize("run", ["A", "B"])
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_tail_edges_vs_float64(case, run):
    from spectre_vit import _native, hip_ops
    c, i = case, {name: np.array(a) for name, a in C.inputs(case, run).items()}   # writable copies: torch wraps them
    p, seed = C.RUNS[run]["p"], C.RUNS[run]["seed"]
    rows, n, k = c.rows, c.n, c.k_in
    dtype = DT[c.dtype]
    other = F32 if c.mixed else dtype                      # dtype of `out` (forward) and `dout` (backward)
    off = c.off // (2 if c.dtype == "bf16" else 4)
    ln, np_ = c.entry == "ln", 5 if c.entry == "ln" else 3
    ins = dict(h=Guarded((rows, n), dtype, i["h"], off), x=Guarded((rows, k), dtype, i["x"]), gamma=Guarded((n,), F32, i["gamma"]),
               beta=Guarded((n,), F32, i["beta"]))
    if ln:
        ins.update(x1=Guarded((rows, n), dtype, i["x1"]), gamma2=Guarded((n,), F32, i["gamma2"]), beta2=Guarded((n,), F32, i["beta2"]),
                   dout2=Guarded((rows, n), dtype, i["dout2"]))
    else:
        ins.update(dout=Guarded((rows, n), other, i["dout"], off))
    if c.dx_add:
        ins.update(dx_add=Guarded((rows, k), dtype, i["dx_add"]))
    if c.entry == "up":
        ins.update(up_src=Guarded((rows, 512), dtype, i["up_src"]))
    outs = dict(out=Guarded((rows, n), other, off=off), mean=Guarded((rows,), F32), rstd=Guarded((rows,), F32), dh=Guarded((rows, n), dtype, off=off))
    if ln:
        outs.update(out2=Guarded((rows, n), dtype), mean2=Guarded((rows,), F32), rstd2=Guarded((rows,), F32), ds=Guarded((rows, n), dtype))
    if not c.null_dx:
        outs.update(dx_pool=Guarded((rows, k), dtype))
    sums = ("dgamma", "dbeta", "dbias") + (("dgamma2", "dbeta2") if ln else ())
    if not c.defer:
        outs.update({s: Guarded((n,), F32) for s in sums})
    floats = _native.call("spv_tail_ln_partial_floats" if ln else "spv_rowop_partial_floats", n)
    partials = Guarded((floats,), F32)
    ptr = lambda name: {**ins, **outs}[name].ptr if name in ins or name in outs else 0
    code, ocode, st = hip_ops._dt(ins["h"].t), hip_ops._dt(outs["out"].t), hip_ops._stream()

    before = census()
    if ln:
        _native.call("spv_spectre_tail_ln_fwd", ptr("h"), ptr("x"), ptr("gamma"), ptr("beta"), ptr("out"), ptr("mean"), ptr("rstd"), ptr("x1"),
                     ptr("gamma2"), ptr("beta2"), ptr("out2"), ptr("mean2"), ptr("rstd2"), rows, n, k, code, p, seed, st)
        _native.call("spv_spectre_tail_ln_bwd", ptr("dout2"), ptr("out"), ptr("x1"), ptr("mean2"), ptr("rstd2"), ptr("gamma2"), ptr("ds"),
                     ptr("dgamma2"), ptr("dbeta2"), ptr("h"), ptr("mean"), ptr("rstd"), ptr("gamma"), ptr("beta"), ptr("dh"), ptr("dx_pool"),
                     ptr("dgamma"), ptr("dbeta"), ptr("dbias"), partials.ptr, rows, n, k, code, p, seed, st)
    else:
        _native.call("spv_spectre_tail_fwd", ptr("h"), ptr("x"), ptr("gamma"), ptr("beta"), ptr("out"), ptr("mean"), ptr("rstd"), rows, n, k,
                     code, ocode, p, seed, st)
        bwd = (ptr("dout"), ptr("h"), ptr("mean"), ptr("rstd"), ptr("gamma"), ptr("beta"), ptr("dh"), ptr("dx_pool"), ptr("dgamma"), ptr("dbeta"),
               ptr("dbias"), partials.ptr, rows, n, k, code, ocode, p, seed, ptr("dx_add"))
        if c.entry == "up":
            _native.call("spv_spectre_tail_bwd_up", *bwd, ptr("up_src"), c.p_up, C.UP_SEED, st)
        else:
            _native.call("spv_spectre_tail_bwd", *bwd, st)
    torch.cuda.synchronize()

    # 1. which kernel class served the two calls (the wide and the generic kernels have no slot: an empty delta says no LC kernel ran)
    assert delta(before) == C.expected_census(c), (C.case_id(c), delta(before))
    # 2. nothing written outside the outputs, nothing left unwritten inside
    for name, b in {**ins, **outs, "partials": partials}.items():
        assert b.intact(), f"{name}: sentinel overwritten"
    for name, b in ins.items():
        assert np.array_equal(b.f64(), i[name]), f"input {name} changed"
    got = {name: b.f64() for name, b in outs.items()}
    for name, a in got.items():
        assert not np.isnan(a).any(), f"{name}: {int(np.isnan(a).sum())} elements left unwritten"
    parts = _native.call("spv_tail_bwd_parts", rows)
    assert parts == min(-(-rows // 4), 1024)
    slabs = partials.t[:parts * np_ * n].cpu().numpy().astype(np.float64)
    assert not np.isnan(slabs).any(), "a partial slab the grid owns was not written"
    assert bool(torch.isnan(partials.t[parts * np_ * n:]).all()), "partials written past the grid's slabs"
    if c.defer:   # the caller's fold: slab layout [part][p][n]
        got.update(zip(sums, slabs.reshape(parts, np_, n).sum(axis=0)))

    ref = C.reference(c, run, f3=got["out"], ds=got["ds"]) if ln else C.exact_reference(c, run)
    # 3. the mask, exactly: zero where it drops, non-zero where it keeps.  "Non-zero" is asked of the elements whose reference is
    # non-zero as fp32 resolves it, i.e. beyond the fp32 bar of the row: GELU(ln) + pool cancels to an exact 0.0f in a right kernel
    # a few times in 4 M elements (numpy float32 gives 0 for the reference's 9.1e-9 in ln-fp32-512-768-r8197, run B)
    if p > 0:
        keep = C.keep_mask(c, run)
        masked = ["out"] + (["dx_pool"] if n == k and not c.dx_add and not c.null_dx and not ln else [])
        for name in masked:
            live = np.abs(ref[name]) > (C.GRAD_BAR if name == "dx_pool" else C.FP32_BAR["out"]) * np.abs(ref[name]).max(-1, keepdims=True)
            assert (got[name][~keep] == 0).all(), f"{name}: a dropped element is not zero"
            assert (got[name][keep & live] != 0).all(), f"{name}: a kept element is zero"
    # 4. values
    errs = C.errors(c, got, ref)
    kind = C.case_paths(c)[1][0]
    print(f"TAIL {kind} {c.dtype} {C.case_id(c)} {run} " + " ".join(f"{name}={e:.3e}" for name, e in errs.items()))
    bad = {name: (e, C.bar(c, name)) for name, e in errs.items() if not e <= C.bar(c, name)}
    assert not bad, (C.case_id(c), run, bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", [0, 1])
def test_add_layernorm_bwd_misaligned_din_takes_the_generic_kernel(dtype, mode):
    """(130, 512) is a fast-kernel shape; `din` 8 bytes off 16-byte alignment sends it to the generic kernel instead.  Same oracle and
    bars as test_gpu_ops.test_add_layernorm."""
    from spectre_vit import _native, hip_ops
    rows, n = 130, 512
    rng = np.random.default_rng(rows + n + mode)
    a, b, dy = (q(rng.standard_normal((rows, n)), dtype) for _ in range(3))
    g = q(rng.random(n) + 0.5, F32)
    _, cache = O.layernorm_fwd(a + b if mode else a, g, np.zeros(n))
    din_ref, dg_ref, db_ref = O.layernorm_bwd(dy, g, cache)
    s = a + b if mode else a
    mean_ref, rstd_ref = s.mean(-1), 1.0 / np.sqrt(s.var(-1) + 1e-5)
    A, B, DY, G = Guarded((rows, n), dtype, a), Guarded((rows, n), dtype, b), Guarded((rows, n), dtype, dy), Guarded((n,), F32, g)
    mean, rstd = Guarded((rows,), F32, mean_ref), Guarded((rows,), F32, rstd_ref)
    din = Guarded((rows, n), dtype, off=8 // A.t.element_size())
    dgamma, dbeta = Guarded((n,), F32), Guarded((n,), F32)
    partials = Guarded((_native.call("spv_rowop_partial_floats", n),), F32)
    assert din.ptr % 16 == 8
    _native.call("spv_add_layernorm_bwd", DY.ptr, A.ptr, B.ptr, mean.ptr, rstd.ptr, G.ptr, din.ptr, dgamma.ptr, dbeta.ptr, partials.ptr, rows, n,
                 mode, hip_ops._dt(A.t), hip_ops._stream())
    torch.cuda.synchronize()
    for name, buf in dict(a=A, b=B, dy=DY, g=G, mean=mean, rstd=rstd, din=din, dgamma=dgamma, dbeta=dbeta, partials=partials).items():
        assert buf.intact(), f"{name}: sentinel overwritten"
    assert np.array_equal(A.f64(), a) and np.array_equal(B.f64(), b) and np.array_equal(DY.f64(), dy), "an input changed"
    parts = _native.call("spv_tail_bwd_parts", rows)
    assert bool(torch.isnan(partials.t[parts * 2 * n:]).all()), "partials written past the grid's slabs"
    tol = TOL[dtype]
    check(din.t, din_ref, tol * 2, "din")
    check(dgamma.t, dg_ref, tol * 2, "dgamma")
    check(dbeta.t, db_ref, tol * 2, "dbeta")
