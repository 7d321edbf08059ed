"""The classifier end of the step at its edges against tests/head_ref.py's float64 references: the class head (csrc/spv_head.hip:
spv_small_sl_fwd, _bwd_rows, _bwd_w and _bwd as the two launches), mean cross-entropy (spv_cross_entropy_fwd / _bwd), the distillation
loss (csrc/spv_distill.hip: spv_distill_loss_fwd / _bwd and the _idx_ pair) and the eval head (csrc/spv_infer.hip: spv_eval_head).  Raw
C-ABI calls within include/spv.h's contract, in eager mode, on the current stream, then one synchronize per case.

Every case (tests/head_edge_cases.py) asserts, in this order: memory -- the sentinels around every input, output, workspace and stats
buffer are intact, every input is bit-identical afterwards, every output element is written (outputs start as NaN, pred as -7; where a
reference value is itself NaN -- a label outside the classes, a poisoned cache row -- they start as a finite marker instead); values --
each output within its Spec, the worst ratio to the bar printed; repeat -- where the kernel keeps an arrival counter (CE forward,
distillation forward, eval head) a second call on the same workspace, zeroed once here, returns the same bits.  The backward launches are
fed the forward's own tensors.  tests/test_head_ref.py shows on the CPU that a float32 restatement of each kernel passes this judge on
these inputs and that plausible mistakes do not."""
import numpy as np
import pytest
import torch

import head_edge_cases as C
from test_gpu_attention_edges import Guarded
from test_gpu_permut_edges import buf, raw_bits

pytestmark = pytest.mark.gpu

MARK = 777.0        # what an output starts as where NaN is a legitimate result


def _native():
    from spectre_vit import _native as n
    return n


def _st():
    from spectre_vit import hip_ops
    return hip_ops._stream()


def call(name, *args):
    return _native().call(name, *[a.ptr if isinstance(a, Guarded) else (0 if a is None else a) for a in args])


def ibuf(data, dtype=torch.int64):
    data = np.atleast_1d(np.asarray(data))
    return Guarded(data.shape, dtype, data)


def obuf(shape, dtn="fp32", marked=False):
    return buf(shape, dtn, np.full(shape, MARK) if marked else None)


def zeros(n, dtn="fp32"):
    return buf((n,), dtn, np.zeros(n))


def check_memory(ins, outs, data, scratch=(), marked=False):
    for name, b in {**ins, **outs, **dict(scratch)}.items():
        assert b.intact(), f"{name}: sentinel overwritten"
    for name, b in ins.items():
        if b.t.dtype in (torch.int64, torch.int32):
            assert np.array_equal(b.t.cpu().numpy().reshape(-1), np.asarray(data[name]).reshape(-1)), f"input {name} changed"
            continue
        want, nan = C.bits(np.nan_to_num(data[name]), b.dtn).reshape(-1), np.isnan(data[name]).reshape(-1)
        assert np.array_equal(torch.isnan(b.t).reshape(-1).cpu().numpy(), nan), f"input {name} changed"
        assert np.array_equal(raw_bits(b.t)[~nan], want[~nan]), f"input {name} changed"
    for name, b in outs.items():
        t = b.t.float()
        bad = int((t == MARK).sum()) if marked else int(torch.isnan(t).sum())
        assert bad == 0, f"{name}: {bad} elements left unwritten"


def judge(tag, case, specs, got):
    ok, worst = C.verdict(specs, got)
    print(f"HEAD {tag} {C.case_id(case)} worst ratio to the bar: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert ok, (tag, case, worst)


def same_bits(a, b, what):
    assert np.array_equal(raw_bits(a.t), raw_bits(b.t)), f"{what}: the second call on the same workspace gave other bits"


# ------------------------------------------------------------------------------------------------------------------ A. the class head
def _head_buffers(rows, n, k, lda, ldb, dtn, d=None):
    """(inputs, forward outputs, backward outputs, partials)"""
    get = (lambda name, shape: d[name]) if d is not None else (lambda name, shape: np.ones(shape))
    ins = {name: buf(shape, dt, get(name, shape)) for name, shape, dt in (
        ("xa", (rows, lda), dtn), ("W", (n, k), "fp32"), ("bias", (n,), "fp32"), ("gamma", (n,), "fp32"), ("beta", (n,), "fp32"),
        ("dout", (rows, n), "fp32"))}
    if ldb and (d is None or d["xb"] is not None):
        ins["xb"] = buf((rows, ldb), dtn, get("xb", (rows, ldb)))
    fo = dict(out=obuf((rows, n)), h=obuf((rows, n)), xs=obuf((rows, k)), mean=obuf((rows,)), rstd=obuf((rows,)))
    bo = dict(dh=obuf((rows, n)), dx=obuf((rows, k), dtn), dW=obuf((n, k)), dgamma=obuf((n,)), dbeta=obuf((n,)), dbias=obuf((n,)))
    return ins, fo, bo, obuf((-(-rows // 4) * 3 * n,))


def _head_fwd(i, fo, lda, ldb, rows, n, k, code):
    call("spv_small_sl_fwd", i["xa"], lda, i.get("xb"), ldb if "xb" in i else 0, i["W"], i["bias"], i["gamma"], i["beta"], fo["out"], fo["h"],
         fo["xs"], fo["mean"], fo["rstd"], rows, n, k, code, _st())


def _head_bwd(i, fo, bo, partials, rows, n, k, code, fused):
    if fused:
        call("spv_small_sl_bwd", i["dout"], fo["h"], fo["xs"], fo["mean"], fo["rstd"], i["W"], i["gamma"], i["beta"], bo["dh"], bo["dx"], bo["dW"],
             bo["dgamma"], bo["dbeta"], bo["dbias"], partials, rows, n, k, code, _st())
    else:
        call("spv_small_sl_bwd_rows", i["dout"], fo["h"], fo["mean"], fo["rstd"], i["W"], i["gamma"], i["beta"], bo["dh"], bo["dx"], partials,
             rows, n, k, code, _st())
        call("spv_small_sl_bwd_w", bo["dh"], fo["xs"], partials, bo["dW"], bo["dgamma"], bo["dbeta"], bo["dbias"], rows, n, k, _st())


@pytest.mark.parametrize("case", C.HEAD_CASES, ids=C.case_id)
def test_class_head_vs_float64(case):
    c, d = case, C.head_inputs(case)
    lda, ldb = c.k + c.pad, c.k + 3
    assert _native().call("spv_small_sl_supported", c.rows, c.n, c.k) == 1
    assert _native().call("spv_small_sl_partial_floats", c.rows, c.n) == -(-c.rows // 4) * 3 * c.n
    ins, fo, bo, partials = _head_buffers(c.rows, c.n, c.k, lda, ldb, c.dtype, d)
    _head_fwd(ins, fo, lda, ldb, c.rows, c.n, c.k, C.CODE[c.dtype])
    _head_bwd(ins, fo, bo, partials, c.rows, c.n, c.k, C.CODE[c.dtype], c.fused)
    torch.cuda.synchronize()
    check_memory(ins, {**fo, **bo}, d, dict(partials=partials))
    fwd = {k: b.f64() for k, b in fo.items()}
    judge("head_fwd", c, C.expect("head_fwd", c), fwd)
    got = {k: b.f64() for k, b in bo.items()}
    got["dx_rows"] = got["dx"]
    judge("head_bwd", c, C.expect("head_bwd", c, fwd, got["dh"]), got)


@pytest.mark.parametrize("case", C.BWDW_CASES, ids=C.case_id)
def test_class_head_weights_launch_alone(case):
    c, d = case, C.bwdw_inputs(case)
    ins = dict(dh=buf((c.rows, c.n), "fp32", d["dh"]), xs=buf((c.rows, c.k), "fp32", d["xs"]), partials=buf(d["partials"].shape, "fp32", d["partials"]))
    outs = dict(dW=obuf((c.n, c.k)), dgamma=obuf((c.n,)), dbeta=obuf((c.n,)), dbias=obuf((c.n,)))
    call("spv_small_sl_bwd_w", ins["dh"], ins["xs"], ins["partials"], outs["dW"], outs["dgamma"], outs["dbeta"], outs["dbias"], c.rows, c.n, c.k, _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("head_bwd_w", c, C.expect("bwd_w", c), {k: b.f64() for k, b in outs.items()})


@pytest.mark.parametrize("case", C.HEAD_REFUSED, ids=[r.why for r in C.HEAD_REFUSED])
def test_class_head_refuses(case):
    r = case
    lda, dtn = r.k + r.pad, r.dtype if r.dtype in C.CODE else "fp32"
    code = C.CODE.get(r.dtype, 99)
    assert _native().call("spv_small_sl_supported", r.rows, r.n, r.k) == int(C.head_supported(r.rows, r.n, r.k))
    ins, fo, bo, partials = _head_buffers(r.rows, r.n, r.k, max(lda, r.k), 0, dtn)
    with pytest.raises(RuntimeError, match="spv_small_sl_fwd"):
        _head_fwd(ins, fo, lda, 0, r.rows, r.n, r.k, code)
    if r.why != "lda<k":
        for fused in (1, 0):
            with pytest.raises(RuntimeError, match="spv_small_sl_bwd"):
                _head_bwd(ins, fo, bo, partials, r.rows, r.n, r.k, code, fused)
    if r.why not in ("lda<k", "dtype"):
        with pytest.raises(RuntimeError, match="spv_small_sl_bwd_w"):
            call("spv_small_sl_bwd_w", bo["dh"], fo["xs"], partials, bo["dW"], bo["dgamma"], bo["dbeta"], bo["dbias"], r.rows, r.n, r.k, _st())
    torch.cuda.synchronize()
    for name, b in {**ins, **fo, **bo, "partials": partials}.items():
        assert b.intact(), name
    for name, b in {**fo, **bo, "partials": partials}.items():
        assert bool(torch.isnan(b.t).all()), f"a refused call wrote {name}"


# ------------------------------------------------------------------------------------------------------------------ B. cross-entropy
@pytest.mark.parametrize("case", C.CE_CASES, ids=C.case_id)
def test_cross_entropy_vs_float64(case):
    c, d = case, C.ce_inputs(case)
    specs = C.expect("ce", c)
    marked = any(np.isnan(s.ref).any() for s in specs.values())
    data = dict(d, go=np.array([c.go]))
    ins = dict(z=buf(d["z"].shape, "fp32", d["z"]), labels=ibuf(d["labels"]), go=buf((1,), "fp32", data["go"]))
    outs = dict(lse=obuf((c.rows,), marked=marked), loss=obuf((1,), marked=marked), dz=obuf(d["z"].shape, marked=marked))
    again = dict(lse=obuf((c.rows,), marked=marked), loss=obuf((1,), marked=marked))
    ws = zeros(_native().call("spv_cross_entropy_workspace_floats"))
    call("spv_cross_entropy_fwd", ins["z"], ins["labels"], outs["lse"], outs["loss"], ws, c.rows, c.classes, _st())
    call("spv_cross_entropy_bwd", ins["z"], ins["labels"], outs["lse"], ins["go"], outs["dz"], c.rows, c.classes, _st())
    call("spv_cross_entropy_fwd", ins["z"], ins["labels"], again["lse"], again["loss"], ws, c.rows, c.classes, _st())
    torch.cuda.synchronize()
    check_memory(ins, {**outs, "lse2": again["lse"], "loss2": again["loss"]}, data, dict(ws=ws), marked)
    judge("ce", c, specs, {k: b.f64() for k, b in outs.items()})
    for name in again:
        same_bits(outs[name], again[name], name)


# ------------------------------------------------------------------------------------------------------------------ C. distillation
@pytest.mark.parametrize("case", C.DL_CASES + [C.DL_POISON], ids=C.case_id)
def test_distill_loss_vs_float64(case):
    c, d = case, C.distill_inputs(case)
    T, w_soft, w_ce = C.CFGS[c.cfg]
    specs = C.expect("distill", c)
    marked = c.kind == "poison"
    data = dict(d, go=np.array([1.0]))
    ins = dict(z=buf(d["z"].shape, "fp32", d["z"]), labels=ibuf(d["labels"]), go=buf((1,), "fp32", data["go"]))
    if c.n_cache:
        ins.update(cache=buf(d["cache"].shape, "fp32", d["cache"]), index=ibuf(d["index"]))
        teacher, fwd, bwd = (ins["cache"], ins["index"]), "spv_distill_loss_idx_fwd", "spv_distill_loss_idx_bwd"
        shape = (c.rows, c.n_cache, c.classes)
    else:
        ins.update(t=buf(d["t"].shape, "fp32", d["t"]))
        teacher, fwd, bwd, shape = (ins["t"],), "spv_distill_loss_fwd", "spv_distill_loss_bwd", (c.rows, c.classes)
    outs = dict(lse3=obuf((3, c.rows), marked=marked), out3=obuf((3,), marked=marked), dz=obuf(d["z"].shape, marked=marked))
    again = dict(lse3=obuf((3, c.rows), marked=marked), out3=obuf((3,), marked=marked))
    ws = zeros(_native().call("spv_distill_loss_workspace_floats"))
    call(fwd, ins["z"], *teacher, ins["labels"], outs["lse3"], outs["out3"], ws, *shape, T, w_soft, w_ce, _st())
    call(bwd, ins["z"], *teacher, ins["labels"], outs["lse3"], ins["go"], outs["dz"], *shape, T, w_soft, w_ce, _st())
    call(fwd, ins["z"], *teacher, ins["labels"], again["lse3"], again["out3"], ws, *shape, T, w_soft, w_ce, _st())
    dense = None
    if c.n_cache and not marked:        # include/spv.h: bit for bit the dense call on the gathered matrix cache[index]
        dense = dict(t=buf(d["t"].shape, "fp32", d["t"]), lse3=obuf((3, c.rows)), out3=obuf((3,)), dz=obuf(d["z"].shape), ws=zeros(ws.t.numel()))
        call("spv_distill_loss_fwd", ins["z"], dense["t"], ins["labels"], dense["lse3"], dense["out3"], dense["ws"], c.rows, c.classes, T, w_soft, w_ce, _st())
        call("spv_distill_loss_bwd", ins["z"], dense["t"], ins["labels"], dense["lse3"], ins["go"], dense["dz"], c.rows, c.classes, T, w_soft, w_ce, _st())
    torch.cuda.synchronize()
    check_memory(ins, {**outs, "lse3_2": again["lse3"], "out3_2": again["out3"]}, data, dict(ws=ws), marked)
    judge("distill", c, specs, {k: b.f64() for k, b in outs.items()})
    for name in again:
        same_bits(outs[name], again[name], name)
    if dense is not None:
        for name in outs:
            assert dense[name].intact() and np.array_equal(raw_bits(outs[name].t), raw_bits(dense[name].t)), f"{name} differs from the dense call"


# ------------------------------------------------------------------------------------------------------------------ D. the eval head
def _stats_of(words):
    w = words.cpu().numpy()
    return dict(seen=np.array([float(w[0])]), top1=np.array([float(w[1])]), topk=np.array([float(w[2])]), loss_sum=w[3:4].view(np.float64).copy())


def _eval_call(c, ins, pred, stats):
    call("spv_eval_head", ins["z"], ins["labels"], ins["n_valid"], pred, stats, c.rows, c.classes, c.k, C.CODE[c.dtype], _st())


def _eval_ins(c, batch=0):
    d = C.eval_inputs(c, batch)
    data = dict(z=d["z"], labels=d["labels"], n_valid=np.array([d["n_valid"]]))
    return data, dict(z=buf(d["z"].shape, c.dtype, d["z"]), labels=ibuf(d["labels"]), n_valid=ibuf(data["n_valid"], torch.int32))


@pytest.mark.parametrize("case", C.EVAL_CASES, ids=C.case_id)
def test_eval_head_vs_float64(case):
    c = case
    data, ins = _eval_ins(c)
    words = _native().call("spv_eval_head_stats_words")
    stats = ibuf(np.zeros(words, np.int64))
    pred, pred2 = ibuf(np.full(c.rows, -7)), ibuf(np.full(c.rows, -7))
    _eval_call(c, ins, pred, stats)
    first = stats.t[:4].clone()         # on the stream, between the two calls
    _eval_call(c, ins, pred2, stats)
    torch.cuda.synchronize()
    for name, b in dict(ins, pred=pred, pred2=pred2, stats=stats).items():
        assert b.intact(), f"{name}: sentinel overwritten"
    check_memory(ins, {}, data)
    assert int((pred.t == -7).sum()) == 0, "pred: elements left unwritten"
    got = _stats_of(first)
    got["pred"] = pred.t.cpu().numpy().astype(np.float64)
    judge("eval", c, C.expect("eval", c), got)
    # the second call added the same batch: the same predictions, the counts twice, and loss_sum + loss_sum (exact) only if its batch
    # sum has the first call's bits
    assert torch.equal(pred.t, pred2.t)
    both = _stats_of(stats.t[:4])
    for name in ("seen", "top1", "topk", "loss_sum"):
        assert both[name][0] == 2 * got[name][0], f"{name}: the second call on the same stats block added something else"


@pytest.mark.parametrize("case", C.EVAL_ACCUMULATE, ids=C.case_id)
def test_eval_head_accumulates_three_batches(case):
    c = case
    stats = ibuf(np.zeros(_native().call("spv_eval_head_stats_words"), np.int64))
    batches = [_eval_ins(c, b) for b in range(3)]
    preds = [ibuf(np.full(c.rows, -7)) for _ in batches]
    for (_, ins), pred in zip(batches, preds):
        _eval_call(c, ins, pred, stats)
    torch.cuda.synchronize()
    assert stats.intact()
    for (data, ins), pred in zip(batches, preds):
        check_memory(ins, {}, data)
        assert pred.intact() and int((pred.t == -7).sum()) == 0
    got = _stats_of(stats.t[:4])
    got["pred"] = preds[-1].t.cpu().numpy().astype(np.float64)
    judge("eval_x3", c, C.expect("eval", c, 3), got)
