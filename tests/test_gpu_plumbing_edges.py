"""The plumbing kernels of csrc/spv_misc.hip (spv_cast, spv_cast_transpose, spv_weight_shadows and _multi, spv_gelu_fwd / _bwd,
spv_axpby, spv_colsum) at their edges against tests/plumbing_ref.py's float64 references: raw C-ABI calls within include/spv.h's
contract, one per entry point, in eager mode, on the current stream, then one synchronize.

Every case (tests/plumbing_edge_cases.py) asserts, in this order: memory -- the sentinels around every buffer are intact, every input
is bit-identical afterwards, every output element is written (outputs start as NaN, no reference value is NaN); values -- casts,
transposes, shadows and the fp32 x + y bit for bit (padding exactly + 0), GELU, a x + b y and the column sums within the elementwise
bars derived in plumbing_edge_cases, the worst ratio to the bar printed.  Inputs carry +-0, subnormals, +-inf and the largest finite
value where the operation tolerates them.  tests/test_plumbing_ref.py shows on the CPU that a float32 restatement of each kernel
passes this judge on these inputs and that plausible mistakes do not."""
import numpy as np
import pytest
import torch

import plumbing_edge_cases as C
from test_gpu_permut_edges import buf, raw_bits

pytestmark = pytest.mark.gpu


def _native():
    from spectre_vit import _native as n
    return n


def _st():
    from spectre_vit import hip_ops
    return hip_ops._stream()


def off_elems(off_bytes, dtn):
    return off_bytes // C.ES[dtn]


def check_memory(ins, outs, data, scratch=()):
    for name, b in {**ins, **outs, **dict(scratch)}.items():
        assert b.intact(), f"{name}: sentinel overwritten"
    for name, b in ins.items():
        assert np.array_equal(raw_bits(b.t), C.bits(data[name], b.dtn).reshape(-1)), f"input {name} changed"


def judge(tag, family, case, outs):
    ok, worst = C.verdict(C.expect(family, case), {k: b.f64() for k, b in outs.items()})
    print(f"PLUMBING {tag} {C.case_id(case)} worst ratio to the bar: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert ok, (tag, case, worst)


# ------------------------------------------------------------------------------------------------------------------ cast
@pytest.mark.parametrize("case", C.CAST_CASES, ids=C.case_id)
def test_cast_bit_for_bit(case):
    c, d = case, C.inputs("cast", case)
    ins, outs = dict(src=buf((c.n,), c.src, d["src"])), dict(dst=buf((c.n,), c.dst))
    _native().call("spv_cast", ins["src"].ptr, C.CODE[c.src], outs["dst"].ptr, C.CODE[c.dst], c.n, _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("cast", "cast", c, outs)


@pytest.mark.parametrize("which", ["src", "dst"])
def test_cast_refuses_a_misaligned_pointer(which):
    src, dst = buf((16,), "fp32", np.ones(16), 2 if which == "src" else 0), buf((16,), "bf16", off=4 if which == "dst" else 0)
    with pytest.raises(RuntimeError, match="spv_cast"):
        _native().call("spv_cast", src.ptr, C.CODE["fp32"], dst.ptr, C.CODE["bf16"], 16, _st())
    torch.cuda.synchronize()
    assert src.intact() and dst.intact() and bool(torch.isnan(dst.t).all()), "a refused call wrote"


def _ct_call(c, src, dst):
    _native().call("spv_cast_transpose", src.ptr, C.CODE[c.src], dst.ptr, C.CODE[c.dst], c.rows, c.cols, c.ld, c.rg, c.gs, c.roff, _st())
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", C.CT_CASES, ids=C.case_id)
def test_cast_transpose_bit_for_bit(case):
    c, d = case, C.inputs("cast_transpose", case)
    ins, outs = dict(src=buf(d["src"].shape, c.src, d["src"])), dict(dst=buf((c.cols, c.ld), c.dst))
    _ct_call(c, ins["src"], outs["dst"])
    check_memory(ins, outs, d)
    judge("cast_transpose", "cast_transpose", c, outs)


@pytest.mark.parametrize("case", C.CT_REFUSED, ids=C.case_id)
def test_cast_transpose_refuses_a_short_ld(case):
    c = case
    src, dst = buf((c.rows, c.cols), c.src, np.ones((c.rows, c.cols))), buf((c.cols, c.rows), c.dst)
    with pytest.raises(RuntimeError, match="spv_cast_transpose"):
        _ct_call(c, src, dst)
    torch.cuda.synchronize()
    assert src.intact() and dst.intact() and bool(torch.isnan(dst.t).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------------------ weight shadows
def _ws_buffers(c):
    d = C.inputs("shadows", c)
    ins, outs = dict(w=buf((c.rows, c.cols), "fp32", d["w"])), dict(tr=buf((c.cols, c.ld), c.dtype))
    if c.plain:
        outs["plain"] = buf((c.rows, c.cols), c.dtype)
    return d, ins, outs


def _ws_single(c, ins, outs):
    _native().call("spv_weight_shadows", ins["w"].ptr, outs["plain"].ptr if c.plain else 0, outs["tr"].ptr, c.rows, c.cols, c.ld, C.CODE[c.dtype], _st())


@pytest.mark.parametrize("case", C.WS_CASES, ids=C.case_id)
def test_weight_shadows_bit_for_bit(case):
    d, ins, outs = _ws_buffers(case)
    _ws_single(case, ins, outs)
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("shadows", "shadows", case, outs)


@pytest.mark.parametrize("cases", C.WS_MULTI, ids=[c[0].dtype for c in C.WS_MULTI])
def test_weight_shadows_multi_equals_the_single_launches(cases):
    from spectre_vit import shadows
    single, multi = [_ws_buffers(c) for c in cases], [_ws_buffers(c) for c in cases]
    for c, (_, ins, outs) in zip(cases, single):
        _ws_single(c, ins, outs)
    # plain NULL: _multi_table writes 0 where the compute copy is the weight's own storage
    ents = [(ins["w"].t, outs["plain"].t if c.plain else ins["w"].t, outs["tr"].t) for c, (_, ins, outs) in zip(cases, multi)]
    table, tt, tx, ty, ntiles = shadows._multi_table(ents)
    assert ntiles == sum(C.cdiv(c.ld, 32) * C.cdiv(c.cols, 64) for c in cases)
    _native().call("spv_weight_shadows_multi", table.data_ptr(), tt.data_ptr(), tx.data_ptr(), ty.data_ptr(), ntiles, C.CODE[cases[0].dtype], _st())
    torch.cuda.synchronize()
    for c, (d, ins, outs), (_, _, outs1) in zip(cases, multi, single):
        check_memory(ins, outs, d)
        judge("shadows_multi", "shadows", c, outs)
        for name in outs:
            assert np.array_equal(raw_bits(outs[name].t), raw_bits(outs1[name].t)), f"{C.case_id(c)}: {name} differs from the single launch"


# ------------------------------------------------------------------------------------------------------------------ GELU, axpby
@pytest.mark.parametrize("case", C.GELU_CASES, ids=C.case_id)
def test_gelu_vs_float64(case):
    c, d = case, C.inputs("gelu", case)
    ins = dict(x=buf((c.n,), c.dtype, d["x"]), dy=buf((c.n,), c.dtype, d["dy"]))
    outs = dict(y=buf((c.n,), c.dtype), dx=buf((c.n,), c.dtype))
    _native().call("spv_gelu_fwd", ins["x"].ptr, outs["y"].ptr, c.n, C.CODE[c.dtype], _st())
    _native().call("spv_gelu_bwd", ins["dy"].ptr, ins["x"].ptr, outs["dx"].ptr, c.n, C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("gelu", "gelu", c, outs)


@pytest.mark.parametrize("case", C.AXPBY_CASES, ids=C.case_id)
def test_axpby_vs_float64(case):
    c, d = case, C.inputs("axpby", case)
    ins, outs = dict(x=buf((c.n,), c.dtype, d["x"]), y=buf((c.n,), c.dtype, d["y"])), dict(out=buf((c.n,), c.dtype))
    _native().call("spv_axpby", ins["x"].ptr, ins["y"].ptr, outs["out"].ptr, c.a, c.b, c.n, C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("axpby", "axpby", c, outs)


# ------------------------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("case", C.COLSUM_CASES, ids=C.case_id)
def test_colsum_vs_float64(case):
    c, d = case, C.inputs("colsum", case)
    ins, outs = dict(x=buf((c.rows, c.n), c.dtype, d["x"], off_elems(c.off, c.dtype))), dict(out=buf((c.n,), "fp32"))
    assert ins["x"].ptr % 16 == c.off
    partials = buf((min(c.rows, 512) * c.n,), "fp32")        # exactly what include/spv.h asks for
    _native().call("spv_colsum", ins["x"].ptr, outs["out"].ptr, partials.ptr, c.rows, c.n, C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d, dict(partials=partials))
    judge("colsum", "colsum", c, outs)
