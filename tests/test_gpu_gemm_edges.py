"""Every GEMM kernel of csrc/spv_gemm.hip (NT: tile, rows, direct-to-LDS, the twelve strip instantiations, the split-K reduce, the
pool-backward, grouped-rows and dropout epilogues; TN: tile at depth 1 and 3, wide, tall, the folds, the batched forms) at its dispatch
edges against tests/gemm_ref.py's float64 references: raw C-ABI calls, once, eagerly, on the current stream, with no graph open, so
live_seed(seed) == seed.

Every case (tests/gemm_edge_cases.py) asserts, in this order: 1. dispatch -- the census moved by exactly what the source counts for the
kernel the restated selector names, and nothing else; 2. memory -- the sentinels around every buffer are intact (the split-K workspace,
sized as include/spv.h states for the requested splits, among them), the operands sit in [rows + 2, ld] buffers whose gap columns and
two trailing rows hold NaN, every input is bit-identical afterwards, the gap columns of C keep their sentinel, rows outside a grouped
row map stay untouched and every element that is due is written (outputs start as NaN, or as data with accumulate); 3. values -- the
integer input set exactly (an fp32 output equals the float64 reference, a bf16 output its bf16 rounding), the normal set elementwise
within the derived bar u |ref| + (n + 2) 2^-24 S, the worst ratio printed; with dropout the kept / dropped pattern equals
tests/dropout_ref.py's prediction.  tests/test_gemm_ref.py shows on the CPU that a float32 restatement of each kernel passes on these
inputs and that eleven plausible mistakes do not."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_edge_cases as C
from test_gpu_attention_edges import Guarded, delta
from test_gpu_bench_shapes import census
from test_gpu_permut_edges import raw_bits

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F32 = torch.float32


def _native():
    from spectre_vit import _native as n
    return n


def _st():
    from spectre_vit import hip_ops
    return hip_ops._stream()


def buf(data, dtn, off=0):
    """a guarded buffer holding `data` (float64, NaN allowed); .bits: its storage bits before the call"""
    b = Guarded(data.shape, DT[dtn], data, off)
    b.bits = raw_bits(b.t).copy()
    return b


def operand(a, ld, dtn):
    """[rows + 2, ld]: NaN in the gap columns and in the two rows behind the last one"""
    return buf(C.padded(a, ld), dtn)


def check_memory(ins, outs):
    for name, b in {**ins, **outs}.items():
        assert b.intact(), f"{name}: sentinel overwritten"
    for name, b in ins.items():
        assert np.array_equal(raw_bits(b.t), b.bits), f"input {name} changed"


def judged(tag, ok, worst, msg):
    print(f"GEMM {tag} worst ratio to the bar = {worst:.3f}")
    assert ok, (tag, msg, worst)


def ptr(b):
    return b.ptr if b is not None else 0


class Reserved:
    """spv_set_reserved_cus(n) for the body, 0 again afterwards"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        if self.n:
            _native().call("spv_set_reserved_cus", self.n)

    def __exit__(self, *exc):
        if self.n:
            _native().call("spv_set_reserved_cus", 0)


# ----------------------------------------------------------------------------------------------------------------------- NT
def nt_buffers(c, which):
    d = C.nt_inputs(c, which)
    ins = dict(A=operand(d["A"], c.lda, c.din), B=operand(d["B"], c.ldb, c.din))
    if c.bias:
        ins["bias"] = buf(d["bias"], "fp32", c.bias - 1)
    if c.b2:
        ins["bias2d"] = buf(d["bias2d"], "fp32", c.b2 - 1)
    if c.pw:
        ins["pool"] = buf(d["pool"], c.pdt)
    outs = dict(C=buf(C.nt_c_initial(c, which), c.dout, c.coff))
    if c.splits > 1:
        outs["ws"] = Guarded((c.splits * c.M * c.N,), F32)
    return ins, outs


def nt_call(c, which, ins, outs):
    nat, st = _native(), _st()
    shape = (c.M, c.N, c.K, c.lda, c.ldb, c.ldc, C.CODE[c.din], C.CODE[c.dout])
    a, b, cc, bias, b2 = ins["A"].ptr, ins["B"].ptr, outs["C"].ptr, ptr(ins.get("bias")), ptr(ins.get("bias2d"))
    if c.entry == "nt":
        nat.call("spv_gemm_nt", a, b, bias, cc, *shape, c.acc, c.splits, ptr(outs.get("ws")), st)
    elif c.entry == "grouped":
        nat.call("spv_gemm_nt_grouped_rows", a, b, bias, b2, cc, *shape, c.rg, c.gs, c.roff, st)
    elif c.entry == "drop":
        p = c.p_of(which)
        nat.call("spv_gemm_nt_grouped_rows_drop", a, b, bias, b2, cc, *shape, c.rg, c.gs, c.roff, p, C.SEED if p > 0 else 0, st)
    else:
        nat.call("spv_gemm_nt_pool_bwd", a, b, cc, ins["pool"].ptr, c.pw, *shape, C.CODE[c.pdt], st)
    torch.cuda.synchronize()


@pytest.mark.parametrize("run", C.NT_RUNS, ids=C.nt_run_id)
def test_nt_edges_vs_float64(run):
    c, which = run
    pl = C.nt_case_plan(c, which)
    assert (C.nt_plan_name(pl), pl["splits"]) == (c.kernel, c.slabs)
    ins, outs = nt_buffers(c, which)
    assert outs["C"].ptr % 16 == (c.coff * C.ES[c.dout]) % 16 and (not c.bias or ins["bias"].ptr % 16 == 4 * (c.bias - 1))
    with Reserved(c.reserved):
        before = census()
        nt_call(c, which, ins, outs)
        moved = delta(before)
    assert moved == C.nt_census(pl), (C.nt_run_id(run), pl, moved)
    check_memory(ins, outs)
    judged(C.nt_run_id(run), *C.nt_judge(c, which, outs["C"].f64()))


# ----------------------------------------------------------------------------------------------------------------------- TN
class Folds:
    """the guarded buffers of a list of fold jobs and the spv_fold_job array that names them"""

    def __init__(self, jobs, data):
        self.jobs, self.data = jobs, data
        self.partials = [buf(pt, "fp32") for pt, _, _ in data]
        self.outs = [[Guarded((n,), F32) for _ in range(nsum)] for _, nsum, n in jobs]
        self.arr = (_native().FoldJob * max(len(jobs), 1))()
        for j, (parts, nsum, n), pt, outs in zip(self.arr, jobs, self.partials, self.outs):
            j.partials = pt.ptr
            for i, o in enumerate(outs):
                j.out[i] = o.ptr
            j.parts, j.nsum, j.n = parts, nsum, n

    @property
    def ptr(self):
        return ctypes.addressof(self.arr) if self.jobs else 0

    def check(self, tag, which):
        for i, ((pt, value, S), (parts, nsum, n)) in enumerate(zip(self.data, self.jobs)):
            check_memory({f"partials{i}": self.partials[i]}, {f"fold{i}.{u}": o for u, o in enumerate(self.outs[i])})
            got = np.stack([o.f64() for o in self.outs[i]])
            judged(f"{tag} fold {parts}x{nsum}x{n}", *C.fold_judge(which, got, value, S, parts))

    def untouched(self):
        return all(bool(torch.isnan(o.t).all()) and o.intact() for outs in self.outs for o in outs)


@pytest.mark.parametrize("run", C.TN_RUNS, ids=C.tn_run_id)
def test_tn_edges_vs_float64(run):
    c, which = run
    nat, pl = _native(), C.tn_case_plan(c)
    assert (pl["kernel"], pl["splits"]) == (c.kernel, c.slabs)
    d = C.tn_inputs(c, which)
    ins = dict(A=operand(d["A"], c.lda, "bf16"), B=operand(d["B"], c.ldb, "bf16"))
    outs = dict(C=buf(C.tn_c_initial(c, which), c.dout, c.coff))
    if c.splits > 1:
        outs["ws"] = Guarded((c.splits * c.M * c.N,), F32)
    folds = Folds(c.folds, d["folds"])
    args = (ins["A"].ptr, ins["B"].ptr, outs["C"].ptr, c.M, c.N, c.K, c.lda, c.ldb, c.ldc, C.CODE[c.dout], c.acc, c.splits, ptr(outs.get("ws")))
    before = census()
    if c.folds:
        nat.call("spv_gemm_tn_fold", *args, folds.ptr, len(c.folds), _st())
    else:
        nat.call("spv_gemm_tn", *args, _st())
    torch.cuda.synchronize()
    assert delta(before) == C.tn_census(pl), (C.tn_run_id(run), pl, delta(before))
    check_memory(ins, outs)
    judged(C.tn_run_id(run), *C.tn_judge(c, which, outs["C"].f64()))
    folds.check(C.tn_run_id(run), which)


@pytest.mark.parametrize("which", ["int", "normal"])
def test_fold_multi_seventeen_jobs(which):
    """17 jobs: spv_fold_multi takes sixteen per launch, so two launches"""
    jobs = C.FOLDS_17
    assert len(jobs) == 17 and C.fold_exact_ok(jobs)
    folds = Folds(jobs, C.fold_inputs(jobs, "multi", which))
    before = census()
    _native().call("spv_fold_multi", folds.ptr, len(jobs), _st())
    torch.cuda.synchronize()
    assert delta(before) == {}
    folds.check("fold_multi", which)


# ----------------------------------------------------------------------------------------------------------------- TN batch
class Batch:
    def __init__(self, c, which):
        nat = _native()
        self.c, self.which, self.pl = c, which, C.tnb_case_plan(c)
        self.data, fold_data = C.tnb_inputs(c, which)
        self.ins, self.outs = {}, {}
        self.arr = (nat.TnProblem * len(c.probs))()
        for i, ((m, n, pa, pb, pc, k), d, q) in enumerate(zip(c.probs, self.data, self.arr)):
            a, b = operand(d["A"], m + pa, "bf16"), operand(d["B"], n + pb, "bf16")
            init = np.full((m, n + pc), np.nan)
            init[:, n:] = C.SENT
            cc = buf(init, "fp32")
            self.ins.update({f"A{i}": a, f"B{i}": b})
            self.outs[f"C{i}"] = cc
            q.a, q.b, q.c, q.m, q.n, q.lda, q.ldb, q.ldc, q.k = a.ptr, b.ptr, cc.ptr, m, n, m + pa, n + pb, n + pc, k
        self.outs["ws"] = Guarded((c.splits * sum(m * n for m, n, *_ in c.probs),), F32)       # as include/spv.h sizes it
        self.folds = Folds(c.folds, fold_data)

    def call(self, part=None):
        args = (ctypes.addressof(self.arr), len(self.c.probs), self.c.K, self.c.splits, self.outs["ws"].ptr, self.folds.ptr, len(self.c.folds))
        if part is None:
            _native().call("spv_gemm_tn_batch", *args, _st())
        else:
            _native().call("spv_gemm_tn_batch_part", *args, part, _st())
        torch.cuda.synchronize()


@pytest.mark.parametrize("run", C.TNB_RUNS, ids=C.tnb_run_id)
def test_tn_batch_edges_vs_float64(run):
    c, which = run
    one = Batch(c, which)
    assert (one.pl["kernel"], one.pl["splits"]) == (c.kernel, c.slabs)
    before = census()
    one.call()
    assert delta(before) == C.tnb_census(one.pl), (C.tnb_run_id(run), one.pl, delta(before))
    check_memory(one.ins, one.outs)
    for i, ((m, n, pa, pb, pc, k), d) in enumerate(zip(c.probs, one.data)):
        judged(f"{C.tnb_run_id(run)} problem {i}", *C.dense_judge(which, one.outs[f"C{i}"].f64(), n, d["ref"], d["S"], d["chain"], "fp32"))
    one.folds.check(C.tnb_run_id(run), which)
    # the same call as two: part 1 is the GEMM launch (the short problems are complete after it), part 2 the reduce and the folds
    two = Batch(c, which)
    before = census()
    two.call(1)
    assert delta(before) == C.tnb_census(one.pl)
    assert two.folds.untouched(), "part 1 ran a fold"
    before = census()
    two.call(2)
    assert delta(before) == {}
    check_memory(two.ins, two.outs)
    for name in one.outs:
        if name != "ws":
            assert np.array_equal(raw_bits(one.outs[name].t), raw_bits(two.outs[name].t)), f"{name}: parts 1 + 2 differ from the single call"
    for a, b in zip(one.folds.outs, two.folds.outs):
        assert all(np.array_equal(raw_bits(x.t), raw_bits(y.t)) for x, y in zip(a, b)), "a fold differs between the single call and parts 1 + 2"


# ---------------------------------------------------------------------------------------------------------------- refusals
def refused(name, args, needle, outs, folds=None):
    """the call fails with `needle` in its message before any launch: nothing counted, nothing written"""
    before = census()
    with pytest.raises(RuntimeError) as e:
        _native().call(name, *args)
    torch.cuda.synchronize()
    assert needle in str(e.value), (name, needle, str(e.value))
    assert delta(before) == {}, (name, needle, delta(before))
    for b in outs:
        assert b.intact() and bool(torch.isnan(b.t).all()), f"{name} ({needle}): a refused call wrote"
    assert folds is None or folds.untouched(), f"{name} ({needle}): a refused call ran a fold"


def test_nt_refusals():
    st, M, N, K = _st(), 16, 24, 32
    A, B = Guarded((M + 2, K + 8), torch.bfloat16, np.ones((M + 2, K + 8))), Guarded((N + 2, K + 8), torch.bfloat16, np.ones((N + 2, K + 8)))
    bias, b2, pool = Guarded((N,), F32, np.ones(N)), Guarded((4, N), F32, np.ones((4, N))), Guarded((M, N // 8), F32, np.ones((M, N // 8)))
    Cb, ws = Guarded((4 * M, N + 8), F32), Guarded((4 * M * N + 4,), F32)
    outs = [Cb, ws]

    def nt(**kw):
        a = dict(A=A.ptr, B=B.ptr, bias=bias.ptr, C=Cb.ptr, M=M, N=N, K=K, lda=K + 8, ldb=K + 8, ldc=N + 8, din=1, dout=0, acc=0, splits=1, ws=ws.ptr)
        a.update(kw)
        return tuple(a[k] for k in ("A", "B", "bias", "C", "M", "N", "K", "lda", "ldb", "ldc", "din", "dout", "acc", "splits", "ws")) + (st,)
    for kw, needle in ((dict(M=0), "empty problem"), (dict(N=0), "empty problem"), (dict(K=-8), "empty problem"), (dict(din=2), "dtype"), (dict(dout=7), "dtype"),
                       (dict(K=28), "multiples of 8"), (dict(lda=K + 4), "multiples of 8"), (dict(ldb=K + 2), "multiples of 8"),
                       (dict(din=0, K=30), "multiples of 4"), (dict(A=A.ptr + 8), "16-byte aligned"), (dict(B=B.ptr + 2), "16-byte aligned"),
                       (dict(lda=K - 8), "leading dimension"), (dict(ldb=K - 8), "leading dimension"), (dict(ldc=N - 1), "leading dimension"),
                       (dict(splits=0), "splits=0"), (dict(splits=-3), "splits=-3"), (dict(splits=2, ws=0), "workspace"),
                       (dict(splits=2, ws=ws.ptr + 4), "workspace")):
        refused("spv_gemm_nt", nt(**kw), needle, outs)

    def grouped(rg, gs, roff, p=None, ldc=N + 8):
        a = (A.ptr, B.ptr, bias.ptr, b2.ptr, Cb.ptr, M, N, K, K + 8, K + 8, ldc, 1, 0, rg, gs, roff)
        return a + ((st,) if p is None else (p, C.SEED, st))
    for rg, gs, roff in ((0, 5, 1), (4, 4, 1), (4, 5, -1), (-4, 5, 0)):
        refused("spv_gemm_nt_grouped_rows", grouped(rg, gs, roff), "bad grouping", outs)
        refused("spv_gemm_nt_grouped_rows_drop", grouped(rg, gs, roff, 0.5, N), "bad grouping", outs)
    for p in (-0.25, 1.0, 1.5):
        refused("spv_gemm_nt_grouped_rows_drop", grouped(4, 5, 1, p, N), "p_drop", outs)
    refused("spv_gemm_nt_grouped_rows_drop", grouped(4, 5, 1, 0.5, N + 8), "ldc == N", outs)

    def pooled(dout=pool.ptr, pw=8, dd=0, **kw):
        a = dict(M=M, N=N, K=K, lda=K + 8, ldb=K + 8, ldc=N + 8, din=1, dout=0)
        a.update(kw)
        return (A.ptr, B.ptr, Cb.ptr, dout, pw) + tuple(a[k] for k in ("M", "N", "K", "lda", "ldb", "ldc", "din", "dout")) + (dd, st)
    for args, needle in ((pooled(dout=0), "bad pooling window"), (pooled(pw=0), "bad pooling window"), (pooled(pw=-8), "bad pooling window"),
                         (pooled(pw=7), "bad pooling window"), (pooled(dd=2), "bad dout dtype"), (pooled(K=28), "multiples of 8")):
        refused("spv_gemm_nt_pool_bwd", args, needle, outs)
    refused("spv_set_reserved_cus", (129,), "outside 0..128", outs)
    refused("spv_set_reserved_cus", (-1,), "outside 0..128", outs)
    for b in (A, B, bias, b2, pool):
        assert b.intact()


def test_tn_refusals():
    st, M, N, K = _st(), 16, 24, 40
    A, B = Guarded((K + 2, M + 8), torch.bfloat16, np.ones((K + 2, M + 8))), Guarded((K + 2, N + 8), torch.bfloat16, np.ones((K + 2, N + 8)))
    Cb, ws = Guarded((M, N + 8), F32), Guarded((4 * M * N + 4,), F32)
    jobs = ((3, 2, 8),)
    folds = Folds(jobs, C.fold_inputs(jobs, "refusals", "int"))
    outs = [Cb, ws]

    def tn(fold=None, **kw):
        a = dict(A=A.ptr, B=B.ptr, C=Cb.ptr, M=M, N=N, K=K, lda=M + 8, ldb=N + 8, ldc=N + 8, dout=0, acc=0, splits=1, ws=ws.ptr)
        a.update(kw)
        return tuple(a[k] for k in ("A", "B", "C", "M", "N", "K", "lda", "ldb", "ldc", "dout", "acc", "splits", "ws")) + (() if fold is None else fold) + (st,)
    checks = ((dict(M=0), "empty problem"), (dict(N=-8), "empty problem"), (dict(K=0), "empty problem"), (dict(dout=2), "bad out_dtype"),
              (dict(M=12), "multiples of 8"), (dict(N=20), "multiples of 8"), (dict(lda=M + 4), "multiples of 8"), (dict(ldb=N + 4), "multiples of 8"),
              (dict(A=A.ptr + 8), "16-byte aligned"), (dict(B=B.ptr + 4), "16-byte aligned"), (dict(lda=M - 8), "leading dimension"),
              (dict(ldb=N - 8), "leading dimension"), (dict(ldc=N - 1), "leading dimension"), (dict(splits=0), "workspace"), (dict(splits=2, ws=0), "workspace"),
              (dict(splits=2, ws=ws.ptr + 8), "workspace"))
    for kw, needle in checks:
        refused("spv_gemm_tn", tn(**kw), needle, outs)
        refused("spv_gemm_tn_fold", tn(fold=(folds.ptr, 1), **kw), needle, outs, folds)
    # fold jobs are checked before the GEMM is launched: a bad one leaves C untouched
    refused("spv_gemm_tn_fold", tn(fold=(folds.ptr, 17)), "fold jobs", outs, folds)
    refused("spv_gemm_tn_fold", tn(fold=(folds.ptr, -1)), "fold jobs", outs, folds)
    refused("spv_gemm_tn_fold", tn(fold=(0, 1)), "fold jobs", outs, folds)
    for field, value in (("parts", 0), ("nsum", 0), ("nsum", 6), ("n", 0), ("partials", None)):
        keep = getattr(folds.arr[0], field)
        setattr(folds.arr[0], field, value)
        refused("spv_gemm_tn_fold", tn(fold=(folds.ptr, 1)), "fold jobs", outs, folds)
        refused("spv_gemm_tn_fold", tn(fold=(folds.ptr, 1), splits=2), "fold jobs", outs, folds)
        refused("spv_fold_multi", (folds.ptr, 1, st), "bad fold job", outs, folds)
        setattr(folds.arr[0], field, keep)
    keep = folds.arr[0].out[0]
    folds.arr[0].out[0] = None
    refused("spv_gemm_tn_fold", tn(fold=(folds.ptr, 1)), "fold jobs", outs, folds)
    folds.arr[0].out[0] = keep
    refused("spv_fold_multi", (0, 1, st), "no jobs", outs, folds)
    refused("spv_fold_multi", (folds.ptr, 0, st), "no jobs", outs, folds)
    assert A.intact() and B.intact()


def test_tn_batch_refusals():
    st, K = _st(), 200
    c = C.TNB("batch128", K, 3, 2, ((16, 24, 8, 8, 0, 0), (8, 8, 0, 0, 0, 65)))     # (no gap columns: a refused call leaves every C all NaN)
    for entry, tail in (("spv_gemm_tn_batch", ()), ("spv_gemm_tn_batch_part", (1,)), ("spv_gemm_tn_batch_part", (2,))):
        b = Batch(c, "int")
        jobs = ((3, 2, 8),)
        folds = Folds(jobs, C.fold_inputs(jobs, "refusals", "int"))
        outs = list(b.outs.values())
        probs = ctypes.addressof(b.arr)

        def call(probs=probs, nprob=2, K=K, splits=3, ws=b.outs["ws"].ptr, fold=folds.ptr, nfolds=1):
            return (probs, nprob, K, splits, ws, fold, nfolds) + tail + (st,)
        for args, needle in ((call(probs=0), "problems"), (call(nprob=0), "problems"), (call(nprob=9), "problems"), (call(K=0), "workspace"),
                             (call(splits=0), "workspace"), (call(ws=0), "workspace"), (call(ws=b.outs["ws"].ptr + 4), "workspace"),
                             (call(nfolds=17), "fold jobs"), (call(nfolds=-1), "fold jobs"), (call(fold=0), "fold jobs")):
            refused(entry, args, needle, outs, folds)
        folds.arr[0].nsum = 6
        refused(entry, call(), "fold jobs", outs, folds)
        folds.arr[0].nsum = 2
        for i, field, value, needle in ((1, "k", -1, "problem 1: k must be"), (1, "k", K + 1, "problem 1: k must be"), (0, "k", 5, "no problem reduces"),
                                        (0, "a", None, "empty problem 0"), (1, "b", None, "empty problem 1"), (1, "c", None, "empty problem 1"),
                                        (0, "m", 0, "empty problem 0"), (1, "n", -8, "empty problem 1"), (0, "m", 12, "problem 0: M, N"),
                                        (1, "n", 4, "problem 1: M, N"), (0, "lda", 20, "problem 0: M, N"), (1, "ldb", 12, "problem 1: M, N"),
                                        (0, "lda", 8, "problem 0: M, N"), (1, "ldb", 0, "problem 1: M, N"), (0, "ldc", 23, "problem 0: M, N"),
                                        (0, "a", b.ins["A0"].ptr + 8, "problem 0: A/B"), (1, "b", b.ins["B1"].ptr + 2, "problem 1: A/B"),
                                        (1, "ldc", 10, "problem 1 (short)")):
            keep = getattr(b.arr[i], field)
            setattr(b.arr[i], field, value)
            refused(entry, call(), needle, outs, folds)
            setattr(b.arr[i], field, keep)
        if tail:
            refused(entry, (probs, 2, K, 3, b.outs["ws"].ptr, folds.ptr, 1, 3, st), "part must be", outs, folds)
            refused(entry, (probs, 2, K, 3, b.outs["ws"].ptr, folds.ptr, 1, 0, st), "part must be", outs, folds)
        for x in b.ins.values():
            assert x.intact()
