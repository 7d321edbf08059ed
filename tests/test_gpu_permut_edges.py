"""Every permutation-gather kernel (csrc/spv_permut.hip: spv_permut_pack's tables, the pair / LDS / scatter / global forward with its
pooled output, the DMA / compact / wide-LDS / parts / scatter / global backward, the row-0 pair in LDS and in global memory) at its
edges against tests/permut_ref.py's float64 references: raw C-ABI calls, once, in eager mode, on the current stream.

Every case (tests/permut_edge_cases.py) asserts, in this order: 1. dispatch -- the census moved by exactly what the source counts for
the path the restated selector names (gather_lds for the pair and the bf16 LDS forward, permut_row0 for the row-0 pair, nothing else),
and the library's table_words / pool_supported equal the restatement; 2. memory -- the sentinels around every buffer are intact, every
input and the table are bit-identical afterwards, every output element is written (outputs start as NaN, inputs hold none; a pooled
average may be NaN only where +inf - inf is the true answer); 3. values -- g, g0 and x0 bit for bit (a gather is a copy and a sign
flip), pooled and dx within the derived elementwise bars of permut_edge_cases, the worst ratio to the bar printed.  Inputs carry +-0,
subnormals, +-inf and the largest finite value.  tests/test_permut_ref.py shows on the CPU that a float32 restatement of each kernel
passes these bars on these inputs and that eight plausible mistakes do not."""
import numpy as np
import pytest
import torch

import permut_edge_cases as C
import permut_ref as R
from test_gpu_attention_edges import Guarded, delta
from test_gpu_bench_shapes import census
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
I32 = torch.int32


def _native():
    from spectre_vit import _native as n
    return n


def _st():
    from spectre_vit import hip_ops
    return hip_ops._stream()


def raw_bits(t):
    """the storage bits of a float32 / bfloat16 / int32 tensor: uint32 or uint16, flat"""
    v = t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).reshape(-1).cpu().numpy()
    return v.view(np.uint16 if t.dtype == torch.bfloat16 else np.uint32)


def off_elems(c, name):
    """elements a buffer sits off 16-byte alignment: one 8-byte step when the case names it"""
    return 8 // C.ES[c.dtype] if c.off == name else 0


class Table:
    """a guarded table, every word 0xFFFFFFFF before spv_permut_pack fills it; .words: its uint32 content after the pack"""

    def __init__(self, perms, signs):
        heads, d = perms.shape
        n = _native().call("spv_permut_table_words", heads, d)
        assert n == C.table_words(heads, d)
        self.buf = Guarded((n,), I32, np.full(n, -1.0))
        self.perms, self.signs = torch.from_numpy(perms).to(dev()), torch.from_numpy(signs).to(dev())
        _native().call("spv_permut_pack", self.perms.data_ptr(), self.signs.data_ptr(), self.buf.ptr, heads, d, _st())
        torch.cuda.synchronize()
        self.words = raw_bits(self.buf.t)

    @property
    def ptr(self):
        return self.buf.ptr

    def unchanged(self):
        return self.buf.intact() and np.array_equal(raw_bits(self.buf.t), self.words)


def check_memory(ins, outs, data, table, may_be_nan=None):
    """sentinels, inputs and the table bit-identical, outputs fully written; may_be_nan = {name: mask of elements whose true value is NaN}"""
    for name, b in {**ins, **outs}.items():
        assert b.intact(), f"{name}: sentinel overwritten"
    assert table.unchanged(), "the table changed"
    for name, b in ins.items():
        assert np.array_equal(raw_bits(b.t), C.bits(data[name], b.dtn).reshape(-1)), f"input {name} changed"
    for name, b in outs.items():
        nan = torch.isnan(b.t).reshape(-1).cpu().numpy()
        allowed = (may_be_nan or {}).get(name)
        bad = int((nan & ~allowed.reshape(-1)).sum()) if allowed is not None else int(nan.sum())
        assert bad == 0, f"{name}: {bad} elements left unwritten"


def buf(shape, dtn, data=None, off=0):
    b = Guarded(shape, DT[dtn], data, off)
    b.dtn = dtn
    return b


def judge(tag, ok, worst):
    print(f"PERMUT {tag} worst ratio to the bar = {worst:.3f}")
    assert ok, (tag, worst)


# ------------------------------------------------------------------------------------------------------------------ A. pack
@pytest.mark.parametrize("case", C.PACK_CASES, ids=C.case_id)
def test_pack_tables_bit_for_bit(case):
    c = case
    perms, signs = C.pack_inputs(c)
    t = Table(perms, signs)
    assert t.buf.intact(), "sentinel overwritten"
    assert np.array_equal(t.perms.cpu().numpy(), perms) and np.array_equal(t.signs.cpu().numpy(), signs), "an input changed"
    lay, total = R.table_layout(c.heads, c.d), c.heads * c.d
    fwd, inv = R.wide_tables(perms, signs)
    assert np.array_equal(t.words[:total], fwd.reshape(-1)), "forward table"
    assert np.array_equal(t.words[total:2 * total], inv.reshape(-1)), "inverse table"
    if "compact" in lay:
        at, n = lay["compact"]
        by = t.words[at:at + n].view(np.uint8)
        (f16, fsg), (i16, isg) = R.compact_tables(fwd), R.compact_tables(inv)
        assert np.array_equal(by[:4 * total].view(np.uint16), np.concatenate([f16, i16])), "compact indices"
        assert np.array_equal(by[4 * total:4 * total + total // 4], np.concatenate([fsg, isg])), "compact sign bits"
        assert (by[4 * total + total // 4:] == 0xff).all(), "written past the sign bits"
    for s, wide in enumerate((fwd, inv)):
        if f"scat{s}" not in lay:
            continue
        at, n = lay[f"scat{s}"]
        got = R.split_scatter_set(t.words[at:at + n], c.heads, c.d)
        off, lists = R.scatter_lists(wide)
        assert np.array_equal(got["off"], off), f"set {s}: off"
        assert np.array_equal(got["cur"], off[:, 1:]), f"set {s}: the cursors end where the next part begins"
        assert (got["pad"] == 0xffff).all(), f"set {s}: written past et"
        for (h, q), want in lists.items():     # placement order inside a part is not deterministic: compared as a set
            e = slice(off[h, q], off[h, q + 1])
            have = np.sort(got["ej"][h, e].astype(np.uint64) << np.uint64(16) | got["et"][h, e].astype(np.uint64))
            assert np.array_equal(have, want), f"set {s}: list of head {h}, part {q}"
    assert sum(n for _, n in lay.values()) == len(t.words)     # every word is one of the documented sections


# ------------------------------------------------------------------------------------------------------------------ B. forward
def _fwd_buffers(c, x64):
    total = c.heads * c.d
    ins = dict(x=buf((c.batch, c.d), c.dtype, x64, off_elems(c, "x")))
    outs = dict(g=buf((c.batch, total), c.dtype, off=off_elems(c, "g")))
    if c.pw:
        outs["pooled"] = buf((c.batch, total // c.pw), c.dtype)
    assert ins["x"].ptr % 16 == (8 if c.off == "x" else 0) and outs["g"].ptr % 16 == (8 if c.off == "g" else 0)
    return ins, outs


def _fwd_call(c, ins, outs, table):
    _native().call("spv_permut_gather_fwd", ins["x"].ptr, table.ptr, outs["g"].ptr, outs["pooled"].ptr if c.pw else 0, c.pw, c.batch, c.heads, c.d,
                   C.CODE[c.dtype], _st())
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", C.FWD_CASES, ids=C.case_id)
def test_gather_fwd_vs_float64(case):
    nat, c = _native(), case
    path = C.fwd_case_path(c)
    perms, signs, x64 = C.fwd_inputs(c)
    table = Table(perms, signs)
    ins, outs = _fwd_buffers(c, x64)
    before = census()
    _fwd_call(c, ins, outs, table)
    assert delta(before) == C.census_of(path, c.dtype), (C.case_id(c), path, delta(before))
    for pw in C.WINDOWS + (12, c.pw):
        assert nat.call("spv_permut_pool_supported", c.heads, c.d, pw, C.CODE[c.dtype]) == C.pool_supported(c.heads, c.d, pw, c.dtype)
    if c.pw:
        g, pooled, ab = R.gather_fwd(x64, perms, signs, c.pw)
    else:
        g, pooled = R.gather_fwd(x64, perms, signs), None
    check_memory(ins, outs, dict(x=x64), table, dict(pooled=np.isnan(pooled)) if c.pw else None)
    bad = int((raw_bits(outs["g"].t) != C.bits(g, c.dtype).reshape(-1)).sum())
    assert bad == 0, f"{path} {C.case_id(c)}: {bad} elements of g differ"
    if c.pw:
        judge(f"fwd {path} pooled {C.case_id(c)}", *C.worst_ratio(outs["pooled"].f64(), pooled, C.pooled_bar(pooled, ab, c.pw, c.dtype)))


@pytest.mark.parametrize("case,why", C.FWD_REFUSED, ids=[C.case_id(c) for c, _ in C.FWD_REFUSED])
def test_gather_fwd_given_pooled_writes_it_or_fails(case, why):
    """a call that was given `pooled` and that no pooling kernel serves is refused before any launch: nothing is written, nothing counted"""
    c = case
    assert C.fwd_case_path(c) == why
    perms, signs, x64 = C.fwd_inputs(c)
    table = Table(perms, signs)
    ins, outs = _fwd_buffers(c, x64)
    before = census()
    with pytest.raises(RuntimeError) as e:
        _fwd_call(c, ins, outs, table)
    assert "spv_permut_gather_fwd" in str(e.value) and "pool" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert delta(before) == {}
    for name, b in {**ins, **outs}.items():
        assert b.intact(), f"{name}: sentinel overwritten"
    assert bool(torch.isnan(outs["g"].t).all()) and bool(torch.isnan(outs["pooled"].t).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------------------ C. backward
@pytest.mark.parametrize("case", C.BWD_CASES, ids=C.case_id)
def test_gather_bwd_vs_float64(case):
    nat, c = _native(), case
    path = C.bwd_case_path(c)
    perms, signs, dg64 = C.bwd_inputs(c)
    table = Table(perms, signs)
    ins = dict(dg=buf((c.batch, c.heads * c.d), c.dtype, dg64, off_elems(c, "dg")))
    outs = dict(dx=buf((c.batch, c.d), c.dtype, off=off_elems(c, "dx")))
    assert ins["dg"].ptr % 16 == (8 if c.off == "dg" else 0) and outs["dx"].ptr % 16 == (8 if c.off == "dx" else 0)
    before = census()
    nat.call("spv_permut_gather_bwd", ins["dg"].ptr, table.ptr, outs["dx"].ptr, c.batch, c.heads, c.d, C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    assert delta(before) == {}, (C.case_id(c), path, delta(before))
    dx, ab = R.gather_bwd(dg64, perms, signs)
    check_memory(ins, outs, dict(dg=dg64), table, dict(dx=np.isnan(dx)))
    judge(f"bwd {path} dx {C.case_id(c)}", *C.worst_ratio(outs["dx"].f64(), dx, C.dx_bar(dx, ab, c.heads, c.dtype)))


# ------------------------------------------------------------------------------------------------------------------ D. row 0
def _row0_fwd(c, table, perms, signs, x64):
    path = C.row0_case_paths(c)[0]
    ins = dict(x=buf((c.batch, c.d), c.dtype, x64, 8 // C.ES[c.dtype] if c.off == "a" else 0))
    outs = dict(g0=buf((c.batch, c.n), c.dtype), x0=buf((c.batch, c.embed), c.dtype, off=8 // C.ES[c.dtype] if c.off == "b" else 0))
    before = census()
    _native().call("spv_permut_row0_fwd", ins["x"].ptr, table.ptr, outs["g0"].ptr, outs["x0"].ptr, c.batch, c.d, c.n, c.embed, C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    assert delta(before) == C.census_of(path, c.dtype), (C.case_id(c), path, delta(before))
    check_memory(ins, outs, dict(x=x64), table)
    g0, x0 = R.row0_fwd(x64, perms[0], signs[0], c.n, c.embed)
    for name, want in (("g0", g0), ("x0", x0)):
        bad = int((raw_bits(outs[name].t) != C.bits(want, c.dtype).reshape(-1)).sum())
        assert bad == 0, f"{path} {C.case_id(c)}: {bad} elements of {name} differ"


@pytest.mark.parametrize("case", C.ROW0_CASES, ids=C.case_id)
def test_row0_pair_vs_float64(case):
    c = case
    perms, signs, x64, dg064, dx064 = C.row0_inputs(c)
    table = Table(perms, signs)
    _row0_fwd(c, table, perms, signs, x64)
    path = C.row0_case_paths(c)[1]
    ins = dict(dg0=buf((c.batch, c.n), c.dtype, dg064), dx0=buf((c.batch, c.embed), c.dtype, dx064, 8 // C.ES[c.dtype] if c.off == "b" else 0))
    outs = dict(dx=buf((c.batch, c.d), c.dtype, off=8 // C.ES[c.dtype] if c.off == "a" else 0))
    before = census()
    _native().call("spv_permut_row0_bwd", ins["dg0"].ptr, ins["dx0"].ptr, table.ptr, outs["dx"].ptr, c.batch, c.d, c.n, c.embed, C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    assert delta(before) == C.census_of(path, c.dtype), (C.case_id(c), path, delta(before))
    dx, a, s = R.row0_bwd(dg064, dx064, perms[0], signs[0], c.d)
    check_memory(ins, outs, dict(dg0=dg064, dx0=dx064), table, dict(dx=np.isnan(dx)))
    judge(f"row0 {path} dx {C.case_id(c)}", *C.worst_ratio(outs["dx"].f64(), dx, C.row0_dx_bar(dx, a, s, c.dtype)))


@pytest.mark.parametrize("case", C.ROW0_FWD_ONLY, ids=C.case_id)
def test_row0_fwd_off_the_backwards_multiple_of_8(case):
    perms, signs, x64, _, _ = C.row0_inputs(case)
    _row0_fwd(case, Table(perms, signs), perms, signs, x64)
