"""The SpectreBranch feature extractor's kernels (csrc/spv_branch.hip: spv_spectrum_log1p, spv_conv3x3_fwd / _dgrad / _wgrad with
their gather launches, spv_token_pool_fwd / _bwd) at their edges against tests/branch_ref.py's float64 references.  Raw C-ABI calls
within include/spv.h's contract, in eager mode, on the current stream, then one synchronize per case.

Every case (tests/branch_edge_cases.py) asserts, in this order: memory -- the sentinels around every input, output and workspace are
intact, every input is bit-identical afterwards, every output element is written (outputs start as NaN; where NaN is a legitimate
value -- a planted NaN, a poisoned window -- as a finite marker); values -- each output and each gather workspace within its Spec,
the worst ratio to the bar printed; repeat -- a second call into fresh outputs gives the same bits, the weight gradient's split-K
fold included.  A refused call raises by name, leaves the sentinels alone and every output NaN.  tests/test_branch_ref.py shows on
the CPU that a float32 restatement of each kernel passes this judge on these inputs and that plausible mistakes do not."""
import numpy as np
import pytest
import torch

import branch_edge_cases as C
from test_gpu_head_edges import MARK, _native, _st, call, obuf
from test_gpu_permut_edges import buf, raw_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def stop_after_a_device_fault():
    """a sticky HIP error ends the session here: nothing more is started on a device that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error ({e}); no further case is started on it", returncode=3)


def off_of(c, name):
    return 1 if c.off in (name, "both") else 0


def ibuf(c, name, data, dtn):
    return buf(data.shape, dtn, data, off_of(c, name))


def check_memory(ins, outs, data, scratch=(), marked=False):
    for name, b in {**ins, **outs, **dict(scratch)}.items():
        assert b.intact(), f"{name}: sentinel overwritten"
    for name, b in ins.items():
        nan = np.isnan(data[name]).reshape(-1)
        assert np.array_equal(torch.isnan(b.t).reshape(-1).cpu().numpy(), nan), f"input {name} changed"
        assert np.array_equal(raw_bits(b.t)[~nan], C.bits(np.nan_to_num(data[name], posinf=np.inf, neginf=-np.inf), b.dtn).reshape(-1)[~nan]), f"input {name} changed"
    for name, b in outs.items():
        t = b.t.float()
        bad = int((t == MARK).sum()) if marked else int(torch.isnan(t).sum())
        assert bad == 0, f"{name}: {bad} elements left unwritten"


def judge(tag, case, family, got):
    ok, worst = C.settle(C.expect(family, case), got, C.poison(family, case))
    print(f"BRANCH {tag} {C.case_id(case)} worst ratio to the bar: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert ok, (tag, case, worst)


def same_bits(first, second):
    for name in first:
        a, b = raw_bits(first[name].t), raw_bits(second[name].t)
        nan = torch.isnan(first[name].t).reshape(-1).cpu().numpy()
        assert np.array_equal(nan, torch.isnan(second[name].t).reshape(-1).cpu().numpy()) and np.array_equal(a[~nan], b[~nan]), \
            f"{name}: the second call gave other bits"


def code_of(c):
    return C.CODE.get(c.dtype, 99)


# ------------------------------------------------------------------------------------------------------------------ A. spectrum
@pytest.mark.parametrize("case", C.SPECTRUM_CASES, ids=C.case_id)
def test_spectrum_vs_float64(case):
    c, img = case, C.spectrum_inputs(case)
    assert _native().call("spv_spectrum_floats", c.H, c.W) == C.spectrum_floats(c.H, c.W) <= C.SPECTRUM_LIMIT
    marked = c.kind == "special"
    ins = dict(img=ibuf(c, "img", img, "fp32"))
    shape = (c.B, c.H, c.W // 2 + 1, c.C)
    outs = [dict(out=buf(shape, c.dtype, np.full(shape, MARK) if marked else None, off_of(c, "out"))) for _ in range(2)]
    for o in outs:
        call("spv_spectrum_log1p", ins["img"], o["out"], c.B, c.C, c.H, c.W, code_of(c), _st())
    torch.cuda.synchronize()
    check_memory(ins, {**outs[0], "out2": outs[1]["out"]}, dict(img=img), marked=marked)
    judge("spectrum", c, "spectrum", dict(out=outs[0]["out"].f64()))
    same_bits(*outs)


@pytest.mark.parametrize("case", C.SPECTRUM_REFUSED, ids=C.case_id)
def test_spectrum_refuses(case):
    c = case.case
    img, out = buf((128, 128), "fp32", np.ones((128, 128))), obuf((128, 128))
    with pytest.raises(RuntimeError, match=f"spv_spectrum_log1p: .*{case.match}"):
        call("spv_spectrum_log1p", img, out, c.B, c.C, c.H, c.W, code_of(c), _st())
    torch.cuda.synchronize()
    assert img.intact() and out.intact() and bool(torch.isnan(out.t).all())


# ------------------------------------------------------------------------------------------------------------------ B. convolutions
def _conv_ins(c):
    d, (w, wd) = C.conv_inputs(c), C.packed(c)
    data = dict(x=d["x"], dy=d["dy"], w=w, wd=wd, bias=d["bias"])
    return data, {k: ibuf(c, k, v, "fp32" if k == "bias" else c.dtype) for k, v in data.items()}


def _conv_outs(c, entry, marked=False, shapes=None):
    """(outputs, gather workspaces, split-K workspace or None) of one launch of `entry`, every one fresh"""
    g = shapes or C.geometry(c)
    mk = lambda name, shape, dtn: buf(shape, dtn, np.full(shape, MARK) if marked else None, off_of(c, name))
    if entry == "fwd":
        return dict(y=mk("y", (g["M"], c.Cout), c.dtype)), dict(cols=mk("cols", (g["M"], g["Kp"]), c.dtype)), None
    if entry == "dgrad":
        return dict(dx=mk("dx", (g["Mi"], c.Cin), c.dtype)), dict(cols=mk("cols", (g["Mi"], g["Kd"]), c.dtype)), None
    ws = None if c.splits <= 1 or c.ws == "null" else buf((max(c.splits, 1) * c.Cout * g["K"],), "fp32", None, off_of(c, "ws"))
    return dict(dw=mk("dw", (c.Cout, g["K"]), "fp32")), dict(dyt=mk("dyt", (c.Cout, g["Mp"]), c.dtype), colst=mk("colst", (g["K"], g["Mp"]), c.dtype)), ws


def _conv_call(c, entry, i, o, w, ws):
    dims = (c.B, c.H, c.W, c.Cin, c.Cout, code_of(c), _st())
    if entry == "fwd":
        call("spv_conv3x3_fwd", i["x"], i["w"], i["bias"], o["y"], w["cols"], *dims)
    elif entry == "dgrad":
        call("spv_conv3x3_dgrad", i["dy"], i["wd"], o["dx"], w["cols"], *dims)
    else:
        call("spv_conv3x3_wgrad", i["dy"], i["x"], o["dw"], w["dyt"], w["colst"], ws, c.splits, *dims)


@pytest.mark.parametrize("case", C.CONV_CASES, ids=C.case_id)
def test_conv_vs_float64(case):
    c = case
    marked = c.which == "special"
    data, ins = _conv_ins(c)
    runs = {e: [_conv_outs(c, e, marked) for _ in range(2)] for e in C.entries_of(c)}
    for e, pair in runs.items():
        for o, w, ws in pair:
            _conv_call(c, e, ins, o, w, ws)
    torch.cuda.synchronize()
    for e, pair in runs.items():
        for n, (o, w, ws) in enumerate(pair):
            check_memory(ins if n == 0 else {}, {**o, **w}, data, dict(ws=ws) if ws is not None else (), marked)
            if ws is not None and C.slabs_of(c) == 1:
                assert bool(torch.isnan(ws.t).all()), "a request that collapses to one slab wrote its workspace"
        o, w, _ = pair[0]
        judge(e, c, e, {k: b.f64() for k, b in {**o, **w}.items()})
        same_bits({**pair[0][0], **pair[0][1]}, {**pair[1][0], **pair[1][1]})


@pytest.mark.parametrize("case", C.CONV_REFUSED, ids=C.case_id)
def test_conv_refuses(case):
    """a refusal of the entry point itself comes before any launch; one that comes from the GEMM behind it (an operand off 16-byte
    alignment, splits = 0, split-K without a workspace) finds the gather workspaces named in case.wrote already written"""
    r, c = case, case.case
    sized = c._replace(**{k: max(getattr(c, k), lo) for k, lo in (("B", 1), ("H", 3), ("W", 3), ("Cin", 1), ("Cout", 1))},
                       dtype=c.dtype if c.dtype in C.CODE else "fp32", splits=max(c.splits, 1), ws="given")
    g = C.geometry(sized)
    ones = lambda name, shape, dtn: buf(shape, dtn, np.ones(shape), off_of(c, name))
    ins = dict(x=ones("x", (sized.B, sized.H, sized.W, sized.Cin), sized.dtype), dy=ones("dy", (g["M"], sized.Cout), sized.dtype),
               w=ones("w", (sized.Cout, g["Kp"]), sized.dtype), wd=ones("wd", (sized.Cin, g["Kd"]), sized.dtype), bias=ones("bias", (sized.Cout,), "fp32"))
    o, w, ws = _conv_outs(sized._replace(off=c.off, splits=max(c.splits, 2)), r.entry, shapes=g)
    with pytest.raises(RuntimeError, match=r.match):
        _conv_call(c, r.entry, ins, o, w, None if c.ws == "null" else ws)
    torch.cuda.synchronize()
    for name, b in {**ins, **o, **w, "ws": ws}.items():
        if b is not None:
            assert b.intact(), name
    for name, b in {**o, **{k: v for k, v in w.items() if k not in r.wrote}, "ws": ws}.items():
        if b is not None:
            assert bool(torch.isnan(b.t).all()), f"a refused call wrote {name}"
    for name in r.wrote:        # written in full, or not at all: never in part
        assert int(torch.isnan(w[name].t).sum()) in (0, w[name].t.numel()), name


# ------------------------------------------------------------------------------------------------------------------ C. pooling
def _pool_call(c, d, i, o):
    if d == "f":
        call("spv_token_pool_fwd", i["y"], o["out"], c.B, c.L, c.C, c.T, c.ldo, code_of(c), _st())
    else:
        call("spv_token_pool_bwd", i["dout"], c.ldo, i.get("add"), o["dy"], c.B, c.L, c.C, c.T, code_of(c), _st())


@pytest.mark.parametrize("case", C.POOL_CASES, ids=C.case_id)
def test_token_pool_vs_float64(case):
    c = case
    data = {k: v for k, v in C.pool_inputs(c).items() if v is not None}
    ins = {k: ibuf(c, k, v, c.dtype) for k, v in data.items()}
    shapes = dict(f=("out", (c.B, c.T, c.ldo)), b=("dy", (c.B, c.L, c.C)))
    runs = {d: [{shapes[d][0]: buf(shapes[d][1], c.dtype, None, off_of(c, shapes[d][0]))} for _ in range(2)] for d in c.dirs}
    for d, pair in runs.items():
        for o in pair:
            _pool_call(c, d, ins, o)
    torch.cuda.synchronize()
    for d, pair in runs.items():
        for n, o in enumerate(pair):
            check_memory(ins if n == 0 else {}, o, data)
        judge("pool_fwd" if d == "f" else "pool_bwd", c, "pool_fwd" if d == "f" else "pool_bwd", {k: b.f64() for k, b in pair[0].items()})
        same_bits(*pair)


@pytest.mark.parametrize("case", C.POOL_REFUSED, ids=C.case_id)
def test_token_pool_refuses(case):
    r, c = case, case.case
    ins = dict(y=buf((64,), "fp32", np.ones(64)), dout=buf((64,), "fp32", np.ones(64)), add=buf((64,), "fp32", np.ones(64)))
    o = dict(out=obuf((64,)), dy=obuf((64,)))
    with pytest.raises(RuntimeError, match=r.match):
        _pool_call(c, r.entry[0], ins, o)
    torch.cuda.synchronize()
    for name, b in {**ins, **o}.items():
        assert b.intact(), name
    assert bool(torch.isnan(o["out"].t).all()) and bool(torch.isnan(o["dy"].t).all())
