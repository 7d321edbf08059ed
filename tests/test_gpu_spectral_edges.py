"""Every spectral kernel (csrc/spv_fft.hip: the bf16 MFMA kernel in its three fusions, fnet_lds_kernel<4 / 9 / 13 / 17 / 20>, the
two-stage generic fallback, the row-0 pair, rfft_real, both Haar kernels; the haar_ln pair of csrc/spv_rowops.hip; csrc/spv_hadamard.hip)
at its edges against tests/spectral_ref.py's float64 references: raw C-ABI calls, once, in eager mode, on the current stream.

Every case (tests/spectral_edge_cases.py) asserts, in this order: 1. dispatch -- the census moved by exactly {fnet_mfma: calls} for the
MFMA cases and by nothing otherwise, and the library's host-side answers equal the restated rules; 2. memory -- the sentinels around
every buffer are intact, every input is bit-identical afterwards, no output or table element is left NaN (they all start as NaN), and
a workspace / partials buffer is non-NaN exactly in the floats its entry point is documented to use; 3. values -- every elementwise
output per block (the sample; for rfft_real, fwht and Haar the line the transform runs along), max |got - ref| / max |ref| over the
block, worst block reported; row statistics and column sums over the whole vector, as the tail suite measures them.  The bars are
spectral_edge_cases': none is fitted to a kernel.  tests/test_spectral_ref.py checks on the CPU that the float32 floor of the
references on these inputs stays within a quarter of each fp32 bar."""
import numpy as np
import pytest
import torch

import spectral_edge_cases as C
import spectral_ref as R
from test_gpu_attention_edges import Guarded, delta
from test_gpu_bench_shapes import census

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F32 = torch.float32
SLACK = 64     # NaN floats behind a workspace / partials buffer that must stay NaN


def _native():
    from spectre_vit import _native as n
    return n


def _st():
    from spectre_vit import hip_ops
    return hip_ops._stream()


def twiddle_table(tokens):
    """the test's own guarded table, NaN before spv_fnet_make_twiddle fills it"""
    n = _native().call("spv_fnet_twiddle_floats", tokens)
    assert n == C.twiddle_floats(tokens)
    tw = Guarded((n,), F32)
    _native().call("spv_fnet_make_twiddle", tw.ptr, tokens, _st())
    return tw


def scratch(floats):
    """`floats` + SLACK NaN floats: the entry point must write exactly the first `floats`"""
    return Guarded((floats + SLACK,), F32)


def check_memory(ins, outs, data, used=None):
    """sentinels, inputs unchanged, outputs fully written; used = {name: floats}: that buffer is non-NaN exactly in its first floats"""
    used = used or {}
    for name, b in {**ins, **outs}.items():
        assert b.intact(), f"{name}: sentinel overwritten"
    for name, b in ins.items():
        assert np.array_equal(b.f64(), data[name]), f"input {name} changed"
    for name, b in outs.items():
        flat = b.t.reshape(-1)
        n = used.get(name, flat.numel())
        bad = int(torch.isnan(flat[:n]).sum())
        assert bad == 0, f"{name}: {bad} elements left unwritten"
        assert bool(torch.isnan(flat[n:]).all()), f"{name}: written past the {n} floats it is documented to use"


def judge(tag, errs, bars):
    print(f"SPECTRAL {tag} " + " ".join(f"{k}={e:.3e}" for k, e in errs.items()))
    bad = {k: (e, bars[k]) for k, e in errs.items() if not e <= bars[k]}
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------------------------------ A. LDS + generic
@pytest.mark.parametrize("run", ["A", "B"])
@pytest.mark.parametrize("case", C.MIX_CASES, ids=C.case_id)
def test_fnet_mix_lds_and_generic_vs_float64(case, run):
    """run A: add_in = NULL; run B: a random add_in"""
    nat, c = _native(), case
    path = C.mix_path(c.dtype, c.tokens, c.dim)
    assert path[0] in ("lds", "generic"), path
    rng, shape, dtype = C.rng_of(c, run), (c.batch, c.tokens, c.dim), DT[c.dtype]
    data = dict(x=C.normal(rng, shape, c.dtype))
    if run == "B":
        data["add_in"] = C.normal(rng, shape, c.dtype)
    off = c.off // (2 if c.dtype == "bf16" else 4)
    assert not off or path[0] == "generic"
    ins = {k: Guarded(shape, dtype, v, off) for k, v in data.items()}
    wsn = nat.call("spv_fnet_workspace_floats", *shape)
    tw = twiddle_table(c.tokens)
    outs = dict(y=Guarded(shape, dtype, off=off), twiddle=tw)
    if wsn:
        outs["workspace"] = scratch(wsn)
    before = census()
    nat.call("spv_fnet_mix", ins["x"].ptr, outs["y"].ptr, ins["add_in"].ptr if run == "B" else 0, tw.ptr, *shape, C.CODE[c.dtype],
             outs["workspace"].ptr if wsn else 0, _st())
    torch.cuda.synchronize()
    assert delta(before) == {}, (C.case_id(c), delta(before))
    assert wsn == C.workspace_floats(c.dtype, *shape) and (wsn == 0) == (path[0] == "lds"), (wsn, path)
    assert nat.call("spv_fnet_ln_supported", c.tokens, c.dim, C.CODE[c.dtype]) == C.fnet_ln_supported(c.dtype, c.tokens, c.dim) == 0
    check_memory(ins, outs, data, dict(workspace=wsn))
    ref = R.fnet_mix(data["x"], data.get("add_in"))
    kind = "lds<%d>" % path[1] if path[0] == "lds" else "generic(%s)" % path[1]
    judge(f"mix {kind} {C.case_id(c)} {run}", dict(y=R.err(outs["y"].f64(), ref, 1)), dict(y=C.bar(C.TRANSFORM_BAR, c.dtype)))


# ------------------------------------------------------------------------------------------------------------------ B. MFMA
@pytest.mark.parametrize("mode", C.MFMA_MODES)
@pytest.mark.parametrize("case", C.MFMA_CASES, ids=C.case_id)
def test_fnet_mfma_vs_float64(case, mode):
    """mixA / mixB: spv_fnet_mix without / with add_in.  ln: spv_fnet_ln_fwd, then spv_fnet_ln_bwd fed the forward's own prenorm,
    mean and rstd, dgamma / dbeta given; ln_defer: both NULL, the test folds partials[batch][2][512] itself in float64."""
    nat, c, dtn, bf = _native(), case, "bf16", torch.bfloat16
    assert C.mix_path(dtn, c.tokens, 512) == ("mfma",)
    B, N, Dm = c.batch, c.tokens, 512
    shape = (B, N, Dm)
    rng = C.rng_of(c, mode)
    assert nat.call("spv_fnet_ln_supported", N, Dm, C.SPV_BF16) == C.fnet_ln_supported(dtn, N, Dm) == 1
    assert nat.call("spv_fnet_workspace_floats", *shape) == C.workspace_floats(dtn, *shape) == 0
    tw = twiddle_table(N)
    data = dict(x=C.normal(rng, shape, dtn))
    if mode.startswith("mix"):
        if mode == "mixB":
            data["add_in"] = C.normal(rng, shape, dtn)
        ins = {k: Guarded(shape, bf, v) for k, v in data.items()}
        outs = dict(y=Guarded(shape, bf), twiddle=tw)
        before = census()
        nat.call("spv_fnet_mix", ins["x"].ptr, outs["y"].ptr, ins["add_in"].ptr if mode == "mixB" else 0, tw.ptr, *shape, C.SPV_BF16, 0, _st())
        torch.cuda.synchronize()
        assert delta(before) == {"fnet_mfma": 1}, (C.case_id(c), delta(before))
        check_memory(ins, outs, data)
        ref = R.fnet_mix(data["x"], data.get("add_in"))
        return judge(f"mfma {mode} {C.case_id(c)}", dict(y=R.err(outs["y"].f64(), ref, 1)), dict(y=C.MFMA_BAR))

    defer = mode == "ln_defer"
    data["gamma"], data["beta"] = C.affine(rng, Dm)
    data["dout"] = C.normal(rng, shape, dtn)
    ins = dict(x=Guarded(shape, bf, data["x"]), gamma=Guarded((Dm,), F32, data["gamma"]), beta=Guarded((Dm,), F32, data["beta"]),
               dout=Guarded(shape, bf, data["dout"]))
    outs = dict(prenorm=Guarded(shape, bf), out=Guarded(shape, bf), mean=Guarded((B, N), F32), rstd=Guarded((B, N), F32), dx=Guarded(shape, bf),
                partials=scratch(B * 2 * Dm), twiddle=tw)
    if not defer:
        outs.update(dgamma=Guarded((Dm,), F32), dbeta=Guarded((Dm,), F32))
    before = census()
    nat.call("spv_fnet_ln_fwd", ins["x"].ptr, outs["prenorm"].ptr, outs["out"].ptr, ins["gamma"].ptr, ins["beta"].ptr, outs["mean"].ptr,
             outs["rstd"].ptr, tw.ptr, B, N, Dm, C.SPV_BF16, _st())
    nat.call("spv_fnet_ln_bwd", ins["dout"].ptr, outs["prenorm"].ptr, outs["mean"].ptr, outs["rstd"].ptr, ins["gamma"].ptr, outs["dx"].ptr,
             0 if defer else outs["dgamma"].ptr, 0 if defer else outs["dbeta"].ptr, outs["partials"].ptr, tw.ptr, B, N, Dm, C.SPV_BF16, _st())
    torch.cuda.synchronize()
    assert delta(before) == {"fnet_mfma": 2}, (C.case_id(c), delta(before))
    check_memory(ins, outs, data, dict(partials=B * 2 * Dm))
    got = {k: b.f64() for k, b in outs.items()}
    if defer:   # the caller's fold: slab layout [batch][2][512]
        got["dgamma"], got["dbeta"] = got["partials"][:B * 2 * Dm].reshape(B, 2, Dm).sum(0)
    fwd = R.fnet_ln_fwd(data["x"], data["gamma"], data["beta"], prenorm=got["prenorm"])
    bwd = R.fnet_ln_bwd(data["dout"], got["prenorm"], data["gamma"])
    errs = dict(prenorm=R.err(got["prenorm"], fwd["prenorm"], 1), mean=R.err(got["mean"], fwd["mean"]), rstd=R.err(got["rstd"], fwd["rstd"]),
                out=R.err(got["out"], fwd["out"], 1), dx=R.err(got["dx"], bwd["dx"], 1), dgamma=R.err(got["dgamma"], bwd["dgamma"]),
                dbeta=R.err(got["dbeta"], bwd["dbeta"]))
    bars = dict(prenorm=C.MFMA_BAR, mean=C.LN_BAR, rstd=C.LN_BAR, out=C.bar(C.LN_BAR, dtn), dx=C.MFMA_DX_BAR,
                dgamma=C.GRAD_BAR + C.BF16_HALF_ULP, dbeta=C.GRAD_BAR + C.BF16_HALF_ULP)
    judge(f"mfma {mode} {C.case_id(c)}", errs, bars)


# ------------------------------------------------------------------------------------------------------------------ C. row 0
@pytest.mark.parametrize("case", C.CLS_CASES, ids=C.case_id)
def test_fnet_cls_vs_float64(case):
    nat, c, dtype = _native(), case, DT[case.dtype]
    B, N, Dm, code = c.batch, c.tokens, c.dim, C.CODE[c.dtype]
    assert nat.call("spv_fnet_cls_supported", N, Dm, code) == C.cls_supported(c.dtype, N, Dm) == 1
    rng = C.rng_of(c)
    data = dict(x=C.normal(rng, (B, N, Dm), c.dtype), g1=C.normal(rng, (B, Dm), c.dtype))
    data["gamma"], data["beta"] = C.affine(rng, Dm)
    ins = dict(x=Guarded((B, N, Dm), dtype, data["x"]), g1=Guarded((B, Dm), dtype, data["g1"]), gamma=Guarded((Dm,), F32, data["gamma"]),
               beta=Guarded((Dm,), F32, data["beta"]))
    outs = dict(out=Guarded((B, Dm), dtype), m0=Guarded((B, Dm), F32), mean=Guarded((B,), F32), rstd=Guarded((B,), F32),
                dx=Guarded((B, N, Dm), dtype), partials=scratch(B * 2 * Dm))
    before = census()
    nat.call("spv_fnet_cls_fwd", ins["x"].ptr, ins["gamma"].ptr, ins["beta"].ptr, outs["out"].ptr, outs["m0"].ptr, outs["mean"].ptr,
             outs["rstd"].ptr, B, N, Dm, code, _st())
    nat.call("spv_fnet_cls_bwd", ins["g1"].ptr, outs["m0"].ptr, outs["mean"].ptr, outs["rstd"].ptr, ins["gamma"].ptr, outs["dx"].ptr,
             outs["partials"].ptr, B, N, Dm, code, _st())
    torch.cuda.synchronize()
    assert delta(before) == {}, (C.case_id(c), delta(before))
    check_memory(ins, outs, data, dict(partials=B * 2 * Dm))
    got = {k: b.f64() for k, b in outs.items()}
    fwd = R.cls_fwd(data["x"], data["gamma"], data["beta"], m0=got["m0"])
    bwd = R.cls_bwd(data["g1"], got["m0"], data["gamma"], N)
    errs = dict(m0=R.err(got["m0"], fwd["m0"], 1), mean=R.err(got["mean"], fwd["mean"]), rstd=R.err(got["rstd"], fwd["rstd"]),
                out=R.err(got["out"], fwd["out"], 1), dx=R.err(got["dx"], bwd["dx"], 2),
                partials=R.err(got["partials"][:B * 2 * Dm].reshape(B, 2, Dm), bwd["partials"], 1))
    bars = dict(m0=C.TRANSFORM_BAR, mean=C.LN_BAR, rstd=C.LN_BAR, out=C.bar(C.LN_BAR, c.dtype), dx=C.bar(C.GRAD_BAR, c.dtype), partials=C.GRAD_BAR)
    judge(f"cls {C.case_id(c)}", errs, bars)


# ------------------------------------------------------------------------------------------------------------------ D. rfft_real
@pytest.mark.parametrize("case", C.RFFT_CASES, ids=C.case_id)
def test_rfft_real_vs_float64(case):
    nat, c, dtype = _native(), case, DT[case.dtype]
    K = c.dim // 2 + 1
    n_in, n_out = (K, c.dim) if c.transpose else (c.dim, K)
    data = dict(x=C.normal(C.rng_of(c), (c.rows, n_in), c.dtype))
    ins, outs = dict(x=Guarded((c.rows, n_in), dtype, data["x"])), dict(y=Guarded((c.rows, n_out), dtype))
    before = census()
    nat.call("spv_rfft_real", ins["x"].ptr, outs["y"].ptr, c.rows, c.dim, c.transpose, C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    assert delta(before) == {}, (C.case_id(c), delta(before))
    check_memory(ins, outs, data)
    ref = R.rfft_real(data["x"], c.dim, c.transpose)
    judge(f"rfft {C.case_id(c)}", dict(y=R.err(outs["y"].f64(), ref, 1)), dict(y=C.bar(C.TRANSFORM_BAR, c.dtype)))


# ------------------------------------------------------------------------------------------------------------------ E. Haar
def _haar(case):
    nat, c, dtype = _native(), case, DT[case.dtype]
    shape = (c.batch, c.tokens, c.dim)
    off = c.off // (2 if c.dtype == "bf16" else 4)
    data = dict(x=C.normal(C.rng_of(c), shape, c.dtype))
    ins, outs = dict(x=Guarded(shape, dtype, data["x"], off)), dict(y=Guarded(shape, dtype))
    assert ins["x"].ptr % 16 == c.off and outs["y"].ptr % 16 == 0
    if c.levels > 1:
        outs["scratch"] = Guarded(shape, dtype)
    before = census()
    nat.call("spv_haar_dwt", ins["x"].ptr, outs["y"].ptr, *shape, c.axis, c.levels, c.inverse, C.CODE[c.dtype],
             outs["scratch"].ptr if c.levels > 1 else 0, _st())
    torch.cuda.synchronize()
    assert delta(before) == {}, (C.case_id(c), delta(before))
    check_memory(ins, outs, data)
    ref, got = R.haar(data["x"], c.axis, c.levels, c.inverse), outs["y"].f64()
    if c.axis == 1:   # the line the transform runs along: (sample, :, column)
        ref, got = np.swapaxes(ref, 1, 2), np.swapaxes(got, 1, 2)
    judge(f"haar {'+'.join(C.haar_plan(c))} {C.case_id(c)}", dict(y=R.err(got, ref, 2)), dict(y=C.haar_bar(c)))


@pytest.mark.parametrize("case", C.HAAR_CASES, ids=C.case_id)
def test_haar_dwt_vs_float64(case):
    _haar(case)


@pytest.mark.parametrize("case", C.HAAR_BIG_CASES, ids=C.case_id)
def test_haar_dwt_grid_stride_trips_vs_float64(case):
    """more elements (scalar kernel) / 8-element chunks (vector kernel) than one sweep of the capped grid covers"""
    c = case
    if C.haar_plan(c) == ["vector"]:
        assert c.batch * c.tokens * c.dim // 8 > C.HAAR_DIM_CAP
    else:
        assert C.haar_plan(c) == ["scalar"] and c.batch * c.tokens * c.dim > C.HAAR_LEVEL_CAP
    _haar(c)


# ------------------------------------------------------------------------------------------------------------------ F. haar_ln
@pytest.mark.parametrize("mode", C.HAAR_LN_MODES)
@pytest.mark.parametrize("case", C.HAAR_LN_CASES, ids=C.case_id)
def test_haar_ln_vs_float64(case, mode):
    """forward, then the backward fed the forward's own mean / rstd; "defer": dgamma / dbeta NULL, the test folds the
    spv_tail_bwd_parts(rows) slabs"""
    nat, c, dtn, bf = _native(), case, "bf16", torch.bfloat16
    rows, Dm, defer = c.rows, c.dim, mode == "defer"
    assert nat.call("spv_haar_ln_supported", Dm, C.SPV_BF16) == C.haar_ln_supported(dtn, Dm) == 1
    rng = C.rng_of(c, mode)
    data = dict(x=C.normal(rng, (rows, Dm), dtn), dout=C.normal(rng, (rows, Dm), dtn))
    data["gamma"], data["beta"] = C.affine(rng, Dm)
    ins = dict(x=Guarded((rows, Dm), bf, data["x"]), dout=Guarded((rows, Dm), bf, data["dout"]), gamma=Guarded((Dm,), F32, data["gamma"]),
               beta=Guarded((Dm,), F32, data["beta"]))
    parts = nat.call("spv_tail_bwd_parts", rows)
    assert parts == min(-(-rows // 4), 1024)
    outs = dict(out=Guarded((rows, Dm), bf), mean=Guarded((rows,), F32), rstd=Guarded((rows,), F32), dx=Guarded((rows, Dm), bf),
                partials=Guarded((nat.call("spv_rowop_partial_floats", Dm),), F32))
    if not defer:
        outs.update(dgamma=Guarded((Dm,), F32), dbeta=Guarded((Dm,), F32))
    before = census()
    nat.call("spv_haar_ln_fwd", ins["x"].ptr, ins["gamma"].ptr, ins["beta"].ptr, outs["out"].ptr, outs["mean"].ptr, outs["rstd"].ptr, rows, Dm,
             C.SPV_BF16, _st())
    nat.call("spv_haar_ln_bwd", ins["dout"].ptr, ins["x"].ptr, outs["mean"].ptr, outs["rstd"].ptr, ins["gamma"].ptr, outs["dx"].ptr,
             0 if defer else outs["dgamma"].ptr, 0 if defer else outs["dbeta"].ptr, outs["partials"].ptr, rows, Dm, C.SPV_BF16, _st())
    torch.cuda.synchronize()
    assert delta(before) == {}, (C.case_id(c), delta(before))
    check_memory(ins, outs, data, dict(partials=parts * 2 * Dm))
    got = {k: b.f64() for k, b in outs.items()}
    if defer:
        got["dgamma"], got["dbeta"] = got["partials"][:parts * 2 * Dm].reshape(parts, 2, Dm).sum(0)
    fwd, bwd = R.haar_ln_fwd(data["x"], data["gamma"], data["beta"]), R.haar_ln_bwd(data["dout"], data["x"], data["gamma"])
    errs = dict(mean=R.err(got["mean"], fwd["mean"]), rstd=R.err(got["rstd"], fwd["rstd"]), out=R.err(got["out"], fwd["out"], 1),
                dx=R.err(got["dx"], bwd["dx"], 1), dgamma=R.err(got["dgamma"], bwd["dgamma"]), dbeta=R.err(got["dbeta"], bwd["dbeta"]))
    bars = dict(mean=C.LN_BAR, rstd=C.LN_BAR, out=C.bar(C.LN_BAR, dtn), dx=C.bar(C.GRAD_BAR, dtn), dgamma=C.GRAD_BAR + C.BF16_HALF_ULP,
                dbeta=C.GRAD_BAR + C.BF16_HALF_ULP)
    judge(f"haar_ln {mode} {C.case_id(c)}", errs, bars)


# ------------------------------------------------------------------------------------------------------------------ G. fwht
def _fwht(c, x64, res64=None):
    """one guarded call of spv_fwht -> y as float64"""
    nat, dtype = _native(), DT[c.dtype]
    data = dict(x=x64)
    if res64 is not None:
        data["residual"] = res64
    ins = {k: Guarded(v.shape, dtype, v) for k, v in data.items()}
    outs = dict(y=Guarded((c.rows, c.n_out), dtype))
    before = census()
    nat.call("spv_fwht", ins["x"].ptr, outs["y"].ptr, ins["residual"].ptr if res64 is not None else 0, c.rows, c.n_in, c.n, c.n_out, c.mode,
             c.repeat, C.fwht_scale(c), C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    assert delta(before) == {}, (C.case_id(c), delta(before))
    check_memory(ins, outs, data)
    return outs["y"].f64()


@pytest.mark.parametrize("case", C.FWHT_CASES, ids=C.case_id)
def test_fwht_vs_float64(case):
    c, rng = case, C.rng_of(case)
    x = C.normal(rng, (c.rows, c.n_in), c.dtype)
    res = C.normal(rng, (c.rows, c.n_out), c.dtype) if c.residual else None
    ref = R.fwht(x, c.n, c.n_out, c.mode, c.repeat, C.fwht_scale(c), res)
    judge(f"fwht rpw{C.fwht_rpw(c.n)} {C.case_id(c)}", dict(y=R.err(_fwht(c, x, res), ref, 1)), dict(y=C.bar(C.TRANSFORM_BAR, c.dtype)))


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n_in,n,n_out,repeat", [(8, 8, 8, 1), (100, 128, 100, 3), (1, 8, 5, 1), (1024, 1024, 1024, 1)])
def test_fwht_mode_2_is_the_adjoint_of_mode_1(n_in, n, n_out, repeat, dtype):
    """<y, A x> = <A^T y, x> in float64 between the kernel's own outputs of mode 1 (x: n_in -> n_out) and mode 2 (y: n_out -> n_in);
    each side carries one output rounding of its transform, so the two agree within the transform's bar of |y| |A x| + |A^T y| |x|"""
    fwd, bwd = C.Fwht(dtype, 3, n_in, n, n_out, 1, repeat, False), C.Fwht(dtype, 3, n_out, n, n_in, 2, repeat, False)
    rng = C.rng_of(fwd, "adjoint")
    x, y = C.normal(rng, (3, n_in), dtype), C.normal(rng, (3, n_out), dtype)
    ax, aty = _fwht(fwd, x), _fwht(bwd, y)
    lhs, rhs = (y * ax).sum(-1), (aty * x).sum(-1)
    scale = np.abs(y).sum(-1) * np.abs(ax).max(-1) + np.abs(aty).max(-1) * np.abs(x).sum(-1)
    e = float((np.abs(lhs - rhs) / scale).max())
    print(f"SPECTRAL fwht-adjoint {dtype} {n_in}-{n}-{n_out}-x{repeat} e={e:.3e}")
    assert e <= C.bar(C.TRANSFORM_BAR, dtype), e
