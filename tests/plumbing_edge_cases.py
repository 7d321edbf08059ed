"""The case tables of tests/test_gpu_plumbing_edges.py (the plumbing half of csrc/spv_misc.hip: spv_cast, spv_cast_transpose,
spv_weight_shadows and _multi, spv_gelu_fwd / _bwd, spv_axpby, spv_colsum), their seeded inputs, a host restatement of each dispatch
rule written in that source, and what each case is judged by (tests/edge_judge.py holds the judging function both test files share).  tests/test_plumbing_ref.py shows on the CPU that the
tables reach every branch, that a float32 restatement of each kernel passes the judge on exactly these inputs and that plausible
mistakes do not.

expect(family, case) -> {output name: Spec}.  A Spec of kind "bits" holds the output to the reference bit for bit (a copy, a cast, a
single IEEE operation); kind "bar" holds |got - ref| elementwise within  c 2^-24 S_i (+ half a bf16 ulp of the reference for bf16
outputs), S_i the float64 sum of the absolute values of the terms of element i.

c is four times the floor, rounded up: the floor is the worst err_i / (2^-24 S_i) of the float32 restatement of plumbing_ref.py
against float64 on exactly these inputs (tests/test_plumbing_ref.py prints it and asserts floor <= c / 4); the factor 4 leaves room
for fused multiply-adds, another fixed summation tree and the few-ulp device erff / __expf.  Measured floors and the bars they set:

    gelu_fwd   floor 2.09   c = 9
    gelu_bwd   floor 2.82   c = 12
    axpby      floor 1.92   c = 8
    colsum     floor 2.02   c = 9"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import plumbing_ref as R
from edge_judge import EPS, LIMIT_BYTES, Spec, cdiv, floor_ratio, round8, values, verdict  # noqa: F401  (re-exported to the tests)
from permut_edge_cases import CODE, DTYPES, ES, bits  # noqa: F401

C_BAR = dict(gelu_fwd=9, gelu_bwd=12, axpby=8, colsum=9)
PAIRS = [(s, d) for s in DTYPES for d in DTYPES]


# ------------------------------------------------------------------------------------------------------------------ dispatch
EW_CAP = 2048          # ew_blocks: min(cdiv(n, 256), 2048) workgroups of 256 threads


def ew_trips(work_items):
    """trips of the capped grid-stride loop of spv_misc.hip over `work_items` items (elements; spv_cast: 4-element vectors)"""
    return cdiv(work_items, 256 * min(cdiv(work_items, 256), EW_CAP))


def shadow_paths(rows, cols, ld):
    """weight_shadow_tile: (16-byte loads along the columns, 8-row vector stores of the transposed copy, tile rows wholly past `rows`)"""
    return cols % 4 == 0, ld % 8 == 0, cdiv(ld, 32) > cdiv(rows, 32)


def colsum_plan(rows, n, aligned=True):
    """spv_colsum: dict(vec, tx_log2, ty, gx, parts)"""
    vec = 4 if n % 4 == 0 and aligned else 1
    cthreads = cdiv(n, vec)
    tx_log2 = 5
    while tx_log2 < 8 and (1 << tx_log2) < cthreads:
        tx_log2 += 1
    ty = 256 >> tx_log2
    gx = cdiv(cthreads, 1 << tx_log2)
    parts = max(1, min(min(cdiv(rows, ty), 512), max(1, 1024 // gx)))
    return dict(vec=vec, tx_log2=tx_log2, ty=ty, gx=gx, parts=parts)


# ------------------------------------------------------------------------------------------------------------------ tables
Cast = namedtuple("Cast", "src dst n")
CT = namedtuple("CT", "src dst rows cols ld rg gs roff", defaults=(0, 0, 0))
WS = namedtuple("WS", "dtype rows cols ld plain", defaults=(1,))
Gelu = namedtuple("Gelu", "dtype n")
Axpby = namedtuple("Axpby", "dtype a b n")
Colsum = namedtuple("Colsum", "dtype rows n off", defaults=(0,))

CAST_BIG = 2097159           # 524 289 vectors against 2048 x 256 threads, and a 3-element tail
CAST_CASES = [Cast(s, d, n) for s, d in PAIRS for n in (1, 2, 3, 4, 5, 7, 1023, CAST_BIG)]

_LD = (lambda r: r, round8, lambda r: r + 70)
_CT_SHAPES = ((1, 1), (63, 65), (64, 64), (65, 63), (130, 1), (1, 130), (130, 130), (65, 130))
CT_CASES = ([CT(s, d, r, c, _LD[(i + j) % 3](r)) for i, (r, c) in enumerate(_CT_SHAPES) for j, (s, d) in enumerate(PAIRS)]
            # grouped rows: the embedding's call (every image's token rows without its CLS row) and a wider skip
            + [CT(s, d, 68, 65, 72, 4, 5, 1) for s, d in PAIRS] + [CT(s, d, 66, 63, 66, 3, 7, 2) for s, d in PAIRS])
CT_REFUSED = [CT("fp32", "bf16", 65, 63, 64)]

WS_SHAPES = ((40, 24), (8, 72), (1, 1), (32, 64), (31, 63), (33, 65), (33, 66))
WS_CASES = [WS(dt, r, c, ld) for dt in DTYPES for r, c in WS_SHAPES for ld in sorted({r, round8(r), round8(r) + 40})] + [
    WS(dt, r, c, ld, 0) for dt in DTYPES for r, c, ld in ((40, 24, 40), (31, 63, 31), (33, 66, 80))]
# one spv_weight_shadows_multi launch over three tensors, against their three single launches
WS_MULTI = [tuple(WS(dt, r, c, ld, pl) for r, c, ld, pl in ((40, 24, 40, 1), (31, 63, 31, 1), (33, 66, 80, 0))) for dt in DTYPES]

GELU_POINTS = 20001
GELU_EXTRA = (0.0, -0.0, 1e-30, -1e-30, 30.0, -30.0, 1e4, -1e4, 3e38, -3e38)
GELU_SMALL, EW_BIG = GELU_POINTS + len(GELU_EXTRA), 524293      # both odd; 524 293 elements against 2048 x 256 threads
GELU_CASES = [Gelu(dt, n) for dt in DTYPES for n in (GELU_SMALL, EW_BIG)]

AXPBY_CASES = [Axpby(dt, a, b, n) for dt in DTYPES for a, b in ((1.0, 1.0), (0.75, -1.5)) for n in (1, 5, EW_BIG)]

COLSUM_CASES = [Colsum(dt, r, n) for dt in DTYPES for r, n in (
    (1, 1), (5, 3), (9, 100), (33, 132), (7, 260), (3, 516), (5, 1028), (5, 259), (4100, 8))] + [Colsum(dt, 9, 100, 8) for dt in DTYPES]

ALL = dict(cast=CAST_CASES, cast_transpose=CT_CASES, shadows=WS_CASES, gelu=GELU_CASES, axpby=AXPBY_CASES, colsum=COLSUM_CASES)
for _cases in ALL.values():
    assert len(set(_cases)) == len(_cases)


def case_id(c):
    return "-".join(str(v) for v in c)


def ct_src_rows(c):
    return c.rows if c.rg == 0 else cdiv(c.rows, c.rg) * c.gs


def device_bytes(family, c):
    """bytes of device buffers a case allocates (sentinels aside), by arithmetic from the table"""
    if family == "cast":
        return c.n * (ES[c.src] + ES[c.dst])
    if family == "cast_transpose":
        return ct_src_rows(c) * c.cols * ES[c.src] + c.cols * c.ld * ES[c.dst]
    if family == "shadows":
        return c.rows * c.cols * (4 + ES[c.dtype]) + c.cols * c.ld * ES[c.dtype]
    if family == "gelu":
        return 5 * c.n * ES[c.dtype]            # x, y, dy, dx and the forward's x again
    if family == "axpby":
        return 3 * c.n * ES[c.dtype]
    return c.rows * c.n * ES[c.dtype] + 4 * (c.n + min(c.rows, 512) * c.n)


# ------------------------------------------------------------------------------------------------------------------ inputs
def rng_of(c, tag=""):
    return np.random.default_rng(zlib.crc32(f"{type(c).__name__}/{case_id(c)}/{tag}".encode()))


@functools.lru_cache(maxsize=4)
def inputs(family, c):
    """{name: float64 array of storage values} of a case"""
    rng = rng_of(c)
    if family == "cast":
        return dict(src=values(rng, (c.n,), c.src))
    if family == "cast_transpose":
        return dict(src=values(rng, (ct_src_rows(c), c.cols), c.src))
    if family == "shadows":
        return dict(w=values(rng, (c.rows, c.cols), "fp32"))
    if family == "gelu":
        pts = np.concatenate([np.linspace(-10.0, 10.0, GELU_POINTS), np.array(GELU_EXTRA), 3.0 * rng.standard_normal(c.n - GELU_SMALL)])
        x = R.cast(pts, c.dtype)
        assert np.isfinite(x).all()
        x.setflags(write=False)
        return dict(x=x, dy=values(rng, (c.n,), c.dtype, "zeros"))
    if family == "axpby":
        return dict(x=values(rng, (c.n,), c.dtype, "zeros"), y=values(rng, (c.n,), c.dtype, "zeros"))
    return dict(x=values(rng, (c.rows, c.n), c.dtype, "finite"))


# ------------------------------------------------------------------------------------------------------------------ the judge
def bar_of(name, ref, S, dtype):
    return C_BAR[name] * EPS * S + R.half_ulp(ref, dtype)


@functools.lru_cache(maxsize=4)
def expect(family, c):
    d = inputs(family, c)
    if family == "cast":
        return dict(dst=Spec("bits", R.cast_ref(d["src"], c.dst), c.dst))
    if family == "cast_transpose":
        return dict(dst=Spec("bits", R.cast_transpose_ref(d["src"], c.dst, c.rows, c.cols, c.ld, c.rg, c.gs, c.roff), c.dst))
    if family == "shadows":
        plain, tr = R.shadows_ref(d["w"], c.dtype, c.ld)
        out = dict(tr=Spec("bits", tr, c.dtype))
        if c.plain:
            out["plain"] = Spec("bits", plain, c.dtype)
        return out
    if family == "gelu":
        (y, sy), (dx, sdx) = R.gelu_fwd_ref(d["x"]), R.gelu_bwd_ref(d["dy"], d["x"])
        return dict(y=Spec("bar", y, c.dtype, bar_of("gelu_fwd", y, sy, c.dtype)), dx=Spec("bar", dx, c.dtype, bar_of("gelu_bwd", dx, sdx, c.dtype)))
    if family == "axpby":
        out, S = R.axpby_ref(d["x"], d["y"], c.a, c.b)
        if (c.a, c.b, c.dtype) == (1.0, 1.0, "fp32"):
            return dict(out=Spec("bits", R.cast(out, "fp32"), "fp32"))       # one IEEE addition
        return dict(out=Spec("bar", out, c.dtype, bar_of("axpby", out, S, c.dtype)))
    out, S = R.colsum_ref(d["x"])
    return dict(out=Spec("bar", out, "fp32", bar_of("colsum", out, S, "fp32")))


def restate(family, c, mutant=None):
    """{output name: float64 storage values} of the float32 restatement of a case (unwritten elements NaN)"""
    d = inputs(family, c)
    if family == "cast":
        return dict(dst=R.cast_restate(d["src"], c.dst, mutant))
    if family == "cast_transpose":
        return dict(dst=R.cast_transpose_restate(d["src"], c.dst, c.rows, c.cols, c.ld, c.rg, c.gs, c.roff, mutant))
    if family == "shadows":
        plain, tr = R.shadows_restate(d["w"], c.dtype, c.ld, mutant)
        return dict(plain=plain, tr=tr) if c.plain else dict(tr=tr)
    if family == "gelu":
        return dict(y=R.gelu_fwd_restate(d["x"], c.dtype, mutant), dx=R.gelu_bwd_restate(d["dy"], d["x"], c.dtype))
    if family == "axpby":
        return dict(out=R.axpby_restate(d["x"], d["y"], c.a, c.b, c.dtype))
    plan = colsum_plan(c.rows, c.n, c.off == 0)
    return dict(out=R.colsum_restate(d["x"], plan["ty"], plan["parts"], mutant))
