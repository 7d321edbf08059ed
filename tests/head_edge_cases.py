"""The case tables of tests/test_gpu_head_edges.py -- the classifier end of the step: the class head (csrc/spv_head.hip:
spv_small_sl_fwd / _bwd_rows / _bwd_w / _bwd), mean cross-entropy (spv_cross_entropy_fwd / _bwd), the distillation loss (csrc/
spv_distill.hip: spv_distill_loss_fwd / _bwd and the _idx_ pair) and the eval head (csrc/spv_infer.hip: spv_eval_head) -- their seeded
inputs, a host restatement of every dispatch rule written in those three sources, and what each case is judged by
(tests/edge_judge.py's Spec / verdict).  tests/test_head_ref.py shows on the CPU that the tables reach every branch, that the float32
restatements of tests/head_ref.py pass the judge on exactly these inputs and that plausible mistakes do not.

Two kinds of bar, neither chosen by hand:

  sums and products (h, dW, dgamma / dbeta / dbias, the matrix part of dx, lse, the losses, dlogits, loss_sum): elementwise
      c 2^-24 S_i (+ half a bf16 ulp of the reference for a bf16 store), S_i the float64 sum of the absolute terms of element i
      (head_ref.py derives it beside each reference: for lse the last addition's |m| + |log s| plus the relative error of s; for
      dlogits (p (1 + |z - lse|) + onehot) |scale| -- the rounding of the exponent's argument z - lse is a relative error of p, so p
      carries it beside its own -- plus p |scale| times the lse bar, plus the smallest normal float32 times |scale| for a
      probability that underflows).  c is four times the floor, rounded up; the floor is the worst
      err_i / (2^-24 S_i) of the float32 restatement against float64 on exactly these inputs (tests/test_head_ref.py prints it and
      asserts floor <= c / 4).  The factor 4 leaves room for fused multiply-adds, another fixed tree and the device exp / log / erf.
  behind LayerNorm and GELU (out, mean, rstd, dh, dx as a whole): the tail family's measure and numbers -- max-abs error over the
      reference's max-abs per row (mean, rstd: over the vector), tail_edge_cases.FP32_BAR = 3e-5 forward, GRAD_BAR = 6e-5 backward,
      2^-8 more for a bf16 store; a reference row that is identically zero must come back as zeros.  The restatement's floor stays
      within a quarter of each.

xs is held bit for bit (one IEEE addition of two storage values, or a copy); counts and predictions are exact.  The backward is fed
the forward's own h, xs, mean, rstd (and the loss backwards the forward's own lse), as the tail edge test does; dW, dbias and the
matrix part of dx are sums over the dh the rows launch itself stored, so their reference is taken over THAT tensor.

Measured floors and the bars they set:

    head_h       floor 2.03   c = 9
    head_dx      floor 6.42   c = 26     (sequential sums of up to 128 terms per slice)
    head_dW      floor 3.11   c = 13     (up to 523 rows, 66 in a row group's chain)
    head_dgamma  floor 1.88   c = 8
    head_dbeta   floor 1.58   c = 7
    head_dbias   floor 1.98   c = 8
    ce_lse       floor 1.08   c = 5
    ce_loss      floor 0.83   c = 4
    ce_dz        floor 1.92   c = 8      (what is left after the allowance for the lse it is fed)
    dl_lse       floor 1.12   c = 5
    dl_soft      floor 0.38   c = 2
    dl_ce        floor 1.01   c = 5
    dl_dz        floor 2.20   c = 9      (as ce_dz)
    ev_loss      floor 0.36   c = 2

    behind LayerNorm and GELU, worst row of the restatement: out 9.7e-7, mean 9.2e-7, rstd 1.1e-7 (bar 3e-5); dh 5.9e-6,
    dx as a whole 6.2e-7 (bar 6e-5)"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import head_ref as R
from edge_judge import EPS, LIMIT_BYTES, Spec, cast, cdiv, floor_ratio, half_ulp, values, verdict  # noqa: F401  (re-exported to the tests)
from permut_edge_cases import CODE, DTYPES, ES, bits  # noqa: F401
from tail_edge_cases import BF16_HALF_ULP, FP32_BAR, GRAD_BAR

C_BAR = dict(head_h=9, head_dx=26, head_dW=13, head_dgamma=8, head_dbeta=7, head_dbias=8, ce_lse=5, ce_loss=4, ce_dz=8, dl_lse=5, dl_soft=2,
             dl_ce=5, dl_dz=9, ev_loss=2)
OUT_BAR = FP32_BAR["out"]


# ------------------------------------------------------------------------------------------------------------------ dispatch
def head_supported(rows, n, k):
    return 0 < rows <= 4096 and 0 < n <= 128 and 0 < k <= 1024 and n <= k


def head_fwd_plan(n, k, xb):
    """small_sl_fwd_kernel: dict(kj: the instantiation, clamped: slots past k (the clamped load and its mask), second: 'none' / 'part' /
    'full' use of a lane's second output slot, trips: batches of outputs per wave, same: n == k (no pooling), bsc: xb given)"""
    kj = 8 if k <= 512 else (12 if k <= 768 else 16)
    ob = 7 if kj <= 8 else (3 if kj <= 12 else 2)
    return dict(kj=kj, clamped=k < 64 * kj, second="none" if n <= 64 else ("full" if n == 128 else "part"), trips=cdiv(n, ob * 16), same=n == k,
                bsc=xb != "null")


def head_bwd_rows_plan(n, k):
    """small_sl_bwd_rows_kernel: dict(cols, nq: output slices joined through LDS, idle: threads past the last slice, ragged: overlapping
    pooling windows (k % n != 0))"""
    cols = min(k, 1024)
    return dict(cols=cols, nq=1024 // cols, idle=1024 - 1024 // cols * cols, ragged=n != k and k % n != 0)


def head_bwd_w_plan(rows, n, k):
    """small_sl_bwd_w_kernel: dict(jobs, nparts, fold_rounds: trips of a fold slice over its partials (16 slices, 8 loads in flight),
    row_rounds: trips of a row group (8 groups, 16 rows in flight), odd_n: the last output pair is half live)"""
    nparts = cdiv(rows, R.HR)
    return dict(jobs=cdiv(n, 2) * cdiv(k, 32) + 1, nparts=nparts, fold_rounds=cdiv(nparts, 128), row_rounds=cdiv(rows, 128), odd_n=n % 2 == 1)


def sweeps(rows, waves, max_wg):
    """trips of a wave-per-row grid-stride loop: min(cdiv(rows, waves), max_wg) workgroups"""
    return cdiv(rows, min(cdiv(rows, waves), max_wg) * waves)


def ew_sweeps(total, threads):
    """trips of an elementwise grid capped at 1024 workgroups"""
    return cdiv(total, min(cdiv(total, threads), 1024) * threads)


def eval_kj(classes):
    """eval_head_kernel's instantiation: rows in registers (2 or 8 per lane) or walked (0)"""
    return 2 if classes <= 128 else (8 if classes <= 512 else 0)


# ------------------------------------------------------------------------------------------------------------------ tables
Head = namedtuple("Head", "dtype rows n k pad xb fused seed", defaults=(0,))       # lda = k + pad; xb: "null" / "ldb" (ldb = k + 3)
BwdW = namedtuple("BwdW", "rows n k")
Refused = namedtuple("Refused", "why rows n k pad dtype")
CE = namedtuple("CE", "rows classes kind go seed", defaults=(0,))
Distill = namedtuple("Distill", "rows classes cfg kind n_cache seed", defaults=(0, 0))      # n_cache 0: the dense entry points
Eval = namedtuple("Eval", "dtype rows classes nv k kind seed", defaults=(0,))

_HEAD_SHAPES = [(1, 1, 1, 0, "null"), (3, 1, 63, 5, "ldb"), (4, 2, 64, 0, "ldb"), (5, 7, 65, 5, "null"), (3, 63, 100, 0, "ldb"),
                (4, 64, 64, 5, "null"), (5, 65, 512, 0, "ldb"), (1, 100, 513, 5, "ldb"), (3, 127, 600, 0, "null"), (4, 128, 128, 5, "ldb"),
                (5, 100, 768, 0, "null"), (3, 64, 769, 5, "ldb"), (4, 128, 1023, 0, "null"), (523, 100, 1024, 5, "ldb"),
                (4096, 2, 2, 0, "ldb"), (5, 1, 1024, 0, "ldb"), (523, 63, 100, 0, "null"), (4, 100, 100, 5, "ldb"), (3, 7, 7, 0, "null"),
                (5, 128, 512, 5, "null"), (1, 64, 1024, 0, "ldb"), (4, 65, 65, 0, "ldb")]
# both storage types per shape; spv_small_sl_bwd (fused = 1) and its two launches on their own alternate
HEAD_CASES = [Head(DTYPES[(i + j) % 2], r, n, k, pad, xb, i % 2) for i, (r, n, k, pad, xb) in enumerate(_HEAD_SHAPES) for j in range(2)]
BWDW_CASES = [BwdW(523, 5, 33)]           # the weights launch alone, on seeded dh and partials (131 partial slabs: two fold rounds)
HEAD_REFUSED = [Refused("n>k", 4, 8, 7, 0, "fp32"), Refused("k=1025", 4, 8, 1025, 0, "fp32"), Refused("n=129", 4, 129, 256, 0, "bf16"),
                Refused("rows=4097", 4097, 2, 2, 0, "fp32"), Refused("lda<k", 4, 8, 16, -1, "bf16"), Refused("dtype", 4, 8, 16, 0, "bad")]

CE_BIG = (1025, 1024)                      # above 1 048 576 elements: the backward's second sweep
CE_CASES = [CE(1, 1, "plain", 1.0), CE(15, 2, "plain", 0.75), CE(16, 63, "plain", 1.0), CE(17, 64, "edges", 1.0), CE(1024, 65, "plain", 0.75),
            CE(1025, 129, "plain", 1.0), CE(17, 1000, "edges", 0.75), CE(16, 65, "edges", 1.0), CE(1, 1000, "plain", 0.75),
            CE(1025, 1, "plain", 1.0), CE(1025, 1024, "plain", 1.0), CE(15, 63, "label_-1", 1.0), CE(17, 129, "label_C", 0.75),
            CE(1024, 2, "edges", 1.0), CE(16, 129, "edges", 0.75), CE(16, 1, "plain", 0.75), CE(15, 64, "plain", 0.75), CE(17, 65, "plain", 1.0),
            CE(1025, 63, "edges", 0.75), CE(1024, 1000, "plain", 1.0), CE(16, 1000, "label_C", 1.0)]

CFGS = ((2.0, 0.25, 0.75), (1.0, 1.0, 0.0), (4.0, 0.0, 1.0))
DL_BIG = (257, 1021)                       # above 262 144 elements: the backward's second sweep
DL_CASES = [Distill(1, 1, 0, "same"), Distill(4, 1, 1, "far"), Distill(1, 2, 0, "near1e-3"), Distill(1, 63, 1, "near0.49"),
            Distill(1, 64, 0, "near0.51"), Distill(1, 65, 1, "same"), Distill(1, 1000, 0, "near1e-3"), Distill(1, 1000, 1, "near0.49"),
            Distill(1, 65, 2, "near0.51"), Distill(4, 2, 2, "plain"), Distill(5, 63, 0, "plain"), Distill(256, 64, 1, "plain"),
            Distill(257, 65, 0, "plain"), Distill(257, 1021, 0, "plain"), Distill(5, 1000, 2, "plain"), Distill(5, 64, 0, "level"),
            Distill(4, 65, 1, "underflow"), Distill(256, 2, 0, "near1e-3"), Distill(5, 63, 1, "near0.49"), Distill(4, 63, 2, "plain"),
            Distill(5, 64, 1, "plain"), Distill(257, 2, 1, "plain"), Distill(256, 1000, 2, "plain"), Distill(4, 1000, 1, "level"),
            Distill(1, 64, 2, "near1e-3"), Distill(1, 2, 1, "near0.49"), Distill(1, 63, 2, "near0.51"), Distill(5, 2, 0, "underflow"),
            # the resident cache through the batch's index: shuffled, with repeats
            Distill(5, 63, 0, "plain", 1), Distill(4, 64, 1, "plain", 5), Distill(257, 65, 0, "plain", 258), Distill(256, 2, 2, "plain", 2048),
            Distill(1, 1000, 0, "near1e-3", 2048), Distill(5, 1, 1, "far", 6), Distill(4, 65, 2, "plain", 5)]
DL_POISON = Distill(9, 65, 0, "poison", 12)      # one index outside the cache, one NaN cache row

_NV = ("rows", "rows-1", "zero", "neg", "rows+5")
EVAL_CASES = [Eval(DTYPES[(i + j) % 2], r, c, _NV[(i + 2 * j) % 5] if kind == "plain" else "rows", k, kind)
              for i, (r, c, k, kind) in enumerate([(1, 1, 1, "plain"), (7, 2, 5, "plain"), (8, 63, 8, "plain"), (9, 64, 1, "plain"),
                                                   (512, 65, 5, "plain"), (513, 128, 8, "plain"), (9, 129, 1, "ties"), (8, 512, 5, "ties"),
                                                   (513, 513, 1, "plain"), (9, 513, 8, "ties"), (9, 128, 5, "ties"), (8, 65, 1, "nan"),
                                                   (9, 513, 5, "nan"), (7, 129, 8, "labels")]) for j in range(2)] + [
    Eval(dt, 9, 65, nv, 5, "plain") for dt in DTYPES for nv in _NV]          # every *n_valid in both storage types
EVAL_ACCUMULATE = [Eval(dt, 513, 129, "rows-1", 5, "plain") for dt in DTYPES]        # three calls into one stats block

ALL = dict(head=HEAD_CASES, ce=CE_CASES, distill=DL_CASES, eval=EVAL_CASES)
for _cases in ALL.values():
    assert len(set(_cases)) == len(_cases)


def case_id(c):
    return "-".join(str(v) for v in c)


def n_valid_of(c):
    return {"rows": c.rows, "rows-1": c.rows - 1, "zero": 0, "neg": -3, "rows+5": c.rows + 5}[c.nv]


def device_bytes(family, c):
    """bytes of device buffers a case allocates (sentinels aside), by arithmetic from the table"""
    if family == "head":
        return 2 * c.rows * (c.k + 5) * ES[c.dtype] + 4 * (3 * c.rows * c.n + 2 * c.rows * c.k + 2 * c.n * c.k + 9 * c.n + 3 * c.rows) + \
            c.rows * c.k * ES[c.dtype] + 4 * 3 * c.n * cdiv(c.rows, 4)
    if family == "ce":
        return 8 * c.rows * c.classes + 16 * c.rows
    if family == "distill":
        return 12 * c.rows * c.classes + 4 * c.n_cache * c.classes + 40 * c.rows
    return c.rows * (c.classes * ES[c.dtype] + 16)


# ------------------------------------------------------------------------------------------------------------------ inputs
def rng_of(c, tag=""):
    return np.random.default_rng(zlib.crc32(f"{type(c).__name__}/{case_id(c)}/{tag}".encode()))


def _ro(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def f32(a):
    return cast(a, "fp32")


@functools.lru_cache(maxsize=4)
def head_inputs(c):
    """{name: float64 array of storage values}: xa [rows, lda] and xb [rows, ldb] with their padding columns (xb None when NULL)"""
    rng = rng_of(c)
    lda, ldb = c.k + c.pad, c.k + 3
    # n = 2 is ill conditioned under a per-row measure however the seed falls: LayerNorm over two values gives +-1 once their gap is
    # large against sqrt(1e-5), and dh is then a cancellation to nothing in every arithmetic; and dh is (t0 - t1) / 2 times (1, -1),
    # which some of 4096 seeded rows always bring close to zero.  So these cases are seeded where the operation is well conditioned:
    # weights at 2^-8 put a row's variance around 1e-5 -- from far below it to ten times above, a quarter of the 4096 rows above
    # (tests/test_head_ref.py asserts both sides) -- and dout's two columns carry opposite signs (t0 - t1 is then |t0| + |t1|)
    wscale = 2.0 ** -8 if c.n == 2 else 1.0
    dout = rng.standard_normal((c.rows, c.n))
    if c.n == 2:
        dout = np.abs(dout) * np.array([1.0, -1.0])
    return _ro(dict(xa=values(rng, (c.rows, lda), c.dtype, "zeros"), xb=None if c.xb == "null" else values(rng, (c.rows, ldb), c.dtype, "zeros"),
                    W=f32(wscale * rng.standard_normal((c.n, c.k)) / np.sqrt(c.k)), bias=f32(wscale * 0.5 * rng.standard_normal(c.n)),
                    gamma=f32(1.0 + 0.25 * rng.standard_normal(c.n)), beta=f32(0.25 * rng.standard_normal(c.n)),
                    dout=f32(dout)))


@functools.lru_cache(maxsize=2)
def bwdw_inputs(c):
    rng = rng_of(c)
    return _ro(dict(dh=f32(rng.standard_normal((c.rows, c.n))), xs=f32(rng.standard_normal((c.rows, c.k))),
                    partials=f32(rng.standard_normal((cdiv(c.rows, R.HR), 3, c.n)))))


def _logits(rng, rows, classes):
    return 3.0 * rng.standard_normal((rows, classes))


@functools.lru_cache(maxsize=4)
def ce_inputs(c):
    rng = rng_of(c)
    z = _logits(rng, c.rows, c.classes)
    labels = rng.integers(0, c.classes, c.rows)
    if c.kind == "edges":       # one row each (as far as there are rows): level + 1e4, level - 1e4, a spread that underflows, +-0, a tie
        r = np.arange(5) % c.rows
        z[r[0]] += 1e4
        z[r[1]] -= 1e4
        z[r[2]] *= 100.0
        z[r[3], ::2], z[r[3], 1::4] = 0.0, -0.0
        z[r[4], c.classes - 1] = z[r[4], labels[r[4]]] = z[r[4]].max() + 1.0
    if c.kind == "label_-1":
        labels[c.rows // 2] = -1
    if c.kind == "label_C":
        labels[c.rows // 2] = c.classes
    return _ro(dict(z=f32(z), labels=labels.astype(np.int64)))


NEAR = {"near1e-3": 1e-3, "near0.49": 0.49, "near0.51": 0.51}


@functools.lru_cache(maxsize=4)
def distill_inputs(c):
    """z, labels, and the teacher: t [rows, C] (dense), or cache [n_cache, C] + index [rows] with t = cache[index] where held"""
    rng = rng_of(c)
    T = CFGS[c.cfg][0]
    z = f32(_logits(rng, c.rows, c.classes))
    labels = rng.integers(0, c.classes, c.rows).astype(np.int64)
    if c.kind in NEAR:          # teacher = student + d, max |d| / T at the named value: on a 2^-12 grid, so that z + d is exact in float32
        z = np.round(z * 256) / 256
        d = np.round(rng.uniform(-1, 1, z.shape) * NEAR[c.kind] * T * 4096) / 4096
        d[:, rng.integers(0, c.classes)] = np.round(NEAR[c.kind] * T * 4096) / 4096
        t = z + d
    elif c.kind == "same":
        t = z.copy()
    elif c.kind == "far":
        t = f32(z + 3.0)
    else:
        t = f32(_logits(rng, c.rows, c.classes))
        if c.kind == "level":
            t = f32(t + 1e4)
        if c.kind == "underflow":
            t[0] = f32(t[0] * 100.0)
    assert np.array_equal(t, f32(t)) and np.array_equal(z, f32(z))
    d = dict(z=z, labels=labels, t=t)
    if c.n_cache:
        # every row's teacher lives at a shuffled cache slot; with fewer slots than rows, or by chance, slots repeat
        index = rng.integers(0, c.n_cache, c.rows).astype(np.int64)
        if c.rows > 1:
            index[-1] = index[0]
        cache = f32(_logits(rng, c.n_cache, c.classes))
        uniq, firsts = np.unique(index, return_index=True)
        cache[uniq] = t[firsts]
        d.update(index=index, cache=cache, t=cache[index])
        if c.kind == "poison":                  # distinct slots but for one repeat; row 2's slot is NaN, row 5's index is outside
            index[:] = rng.permutation(c.n_cache)[:c.rows]
            index[3] = index[0]
            cache[index] = t
            cache[index[3]] = t[3] = t[0]
            cache[index[2]] = np.nan
            index[5] = c.n_cache
            tt = cache[np.clip(index, 0, c.n_cache - 1)]
            tt[5] = np.nan
            d.update(t=tt)
    return _ro(d)


# (label, the column tied with it, the hit): the label's own logit tied with a lower index, a higher one, a lower one in its own lane
TIE_LABELS = ((70, 3, False), (5, 90, True), (100, 36, False))


def tie_pairs(C):
    """columns that share the row's maximum: the same lane (c, c + 64), neighbouring lanes, both sides of the 128 edge, the last column"""
    return [(a, b) for a, b in ((1, 65), (63, 64), (127, 128), (C - 65, C - 1)) if 0 <= a < b < C]


@functools.lru_cache(maxsize=4)
def eval_inputs(c, batch=0):
    """z in storage values of c.dtype, labels, n_valid"""
    rng = rng_of(c, str(batch))
    z = cast(_logits(rng, c.rows, c.classes), c.dtype).copy()
    labels = rng.integers(0, c.classes, c.rows).astype(np.int64)
    C = c.classes
    if c.kind == "ties":
        top = cast(np.abs(z).max() + 2.0, c.dtype)
        pairs = tie_pairs(C)
        for r, (a, b) in enumerate(pairs):      # the same lane (c, c + 64), neighbouring lanes, both sides of the 128 edge
            z[r, a] = z[r, b] = top
        # the label's own logit tied with one other column, with exactly k - 1 entries strictly above it (k = 1: the tie is the row's
        # maximum), so that the tie alone decides the top-k hit: one hit in three rows.  A rule that ignores ties hits all three, one
        # that counts the higher indices hits two, one that counts both sides hits none
        r = len(pairs)
        for i, (y, other, _) in enumerate(TIE_LABELS):
            labels[r + i] = y
            z[r + i, y] = z[r + i, other] = cast(top - 1.0, c.dtype)
            z[r + i, 10:10 + c.k - 1] = top
        r += len(TIE_LABELS) - 2
        if c.dtype == "bf16":                  # a tie made by the storage rounding
            z[r + 2, 10], z[r + 2, 100] = cast(top + 2.0 ** -12, "bf16"), top
            assert z[r + 2, 10] == top
    if c.kind == "nan":                         # a NaN entry never wins; an all-NaN row predicts 0 -- neither row is counted (label -1)
        z[0, int(np.argmax(z[0]))] = np.nan
        z[0, C - 1] = np.nan
        z[1, :] = np.nan
        labels[0] = labels[1] = -1
    if c.kind == "labels":
        labels[0], labels[1] = -1, C
    return _ro(dict(z=z, labels=labels, n_valid=n_valid_of(c)))


# ------------------------------------------------------------------------------------------------------------------ the judge
def sum_bar(name, ref, S, dtype="fp32"):
    return C_BAR[name] * EPS * np.asarray(S, np.float64) + half_ulp(ref, dtype)


def row_bar(ref, rel, dtype="fp32"):
    """the tail family's measure as an elementwise bar: rel (+ 2^-8 for a bf16 store) times the row's largest |reference|; a vector is one row"""
    ref = np.asarray(ref, np.float64)
    peak = np.abs(ref).max(-1, keepdims=True) if ref.ndim == 2 else np.abs(ref).max()
    return np.broadcast_to((rel + (BF16_HALF_ULP if dtype == "bf16" else 0.0)) * peak, ref.shape)


def head_x(c):
    """(xa [rows, k], xb [rows, k] or None) of a case: the columns the kernel reads"""
    d = head_inputs(c)
    return d["xa"][:, :c.k], None if d["xb"] is None else d["xb"][:, :c.k]


@functools.lru_cache(maxsize=4)
def _expect_head_fwd(c):
    d = head_inputs(c)
    xa, xb = head_x(c)
    xs = f32(xa if xb is None else xa + xb)
    ref = R.head_fwd_ref(xs, d["W"], d["bias"], d["gamma"], d["beta"])
    return dict(xs=Spec("bits", xs, "fp32"), h=Spec("bar", ref["h"], "fp32", sum_bar("head_h", ref["h"], ref["S_h"])),
                mean=Spec("bar", ref["mean"], "fp32", row_bar(ref["mean"], FP32_BAR["mean"])),
                rstd=Spec("bar", ref["rstd"], "fp32", row_bar(ref["rstd"], FP32_BAR["rstd"])),
                out=Spec("bar", ref["out"], "fp32", row_bar(ref["out"], OUT_BAR)))


def _expect_head_bwd(c, fwd, dh_got):
    """fwd: the forward's own h, xs, mean, rstd; dh_got: the dh the rows launch stored.  dx is judged twice: `dx` elementwise against
    dh_got W + pool^T(dout), `dx_rows` as a whole per row against the float64 backward"""
    d = head_inputs(c)
    ref = R.head_bwd_ref(d["dout"], fwd["h"], fwd["xs"], fwd["mean"], fwd["rstd"], d["W"], d["gamma"], d["beta"], dh_got)
    out = dict(dh=Spec("bar", ref["dh"], "fp32", row_bar(ref["dh"], GRAD_BAR)),
               dx_rows=Spec("bar", ref["dx_whole"], c.dtype, row_bar(ref["dx_whole"], GRAD_BAR, c.dtype)),
               dx=Spec("bar", ref["dx"], c.dtype, sum_bar("head_dx", ref["dx"], ref["S_dx"], c.dtype)))
    for name in ("dW", "dgamma", "dbeta", "dbias"):
        out[name] = Spec("bar", ref[name], "fp32", sum_bar("head_" + name, ref[name], ref["S_" + name]))
    return out


def _expect_bwdw(c):
    d = bwdw_inputs(c)
    p = d["partials"]
    out = dict(dW=Spec("bar", d["dh"].T @ d["xs"], "fp32", sum_bar("head_dW", 0.0, np.abs(d["dh"]).T @ np.abs(d["xs"]))))
    for i, name in enumerate(("dgamma", "dbeta", "dbias")):     # a plain sum: the bar of the plainest of the three
        out[name] = Spec("bar", p[:, i].sum(0), "fp32", sum_bar("head_dbias", 0.0, np.abs(p[:, i]).sum(0)))
    return out


def lse_bar(name, S):
    return C_BAR[name] * EPS * S


@functools.lru_cache(maxsize=4)
def ce_reference(c):
    d = ce_inputs(c)
    return _ro(R.ce_ref(d["z"], d["labels"], c.go))


def _expect_ce(c):
    ref = ce_reference(c)
    bl = lse_bar("ce_lse", ref["S_lse"])
    scale = abs(c.go) / c.rows
    return dict(lse=Spec("bar", ref["lse"], "fp32", bl), loss=Spec("bar", ref["loss"], "fp32", sum_bar("ce_loss", ref["loss"], ref["S_loss"])),
                dz=Spec("bar", ref["dz"], "fp32", C_BAR["ce_dz"] * EPS * ref["S_dz"] + ref["prop"] * bl[:, None] + R.TINY_NORMAL * scale))


@functools.lru_cache(maxsize=4)
def distill_reference(c):
    d = distill_inputs(c)
    T, ws, wc = CFGS[c.cfg]
    if c.kind == "poison":      # the poisoned rows' own values are judged by their NaN pattern; the reference of the rest needs finite rows
        t = np.where(np.isnan(d["t"]), d["z"], d["t"])
        ref = R.distill_ref(d["z"], t, d["labels"], T, ws, wc, 1.0)
        bad = np.isnan(d["t"]).any(1)
        ref["lse3"][2][bad] = np.nan
        ref["dz"][bad] = np.nan
        ref["out3"][0] = ref["out3"][1] = np.nan
        return _ro(ref)
    return _ro(R.distill_ref(d["z"], d["t"], d["labels"], T, ws, wc, 1.0))


def _expect_distill(c):
    """grad_out = 1.  classes == 1: the soft term and the CE are exactly 0"""
    ref = distill_reference(c)
    T, ws, wc = CFGS[c.cfg]
    bl = lse_bar("dl_lse", ref["S_lse3"])
    b1, b2 = C_BAR["dl_soft"] * EPS * ref["S_out3"][1], C_BAR["dl_ce"] * EPS * ref["S_out3"][2]
    with np.errstate(invalid="ignore"):
        b0 = abs(ws) * b1 + abs(wc) * b2 + 2 * EPS * (abs(ws * ref["out3"][1]) + abs(wc * ref["out3"][2]))
    bo = np.zeros(3) if c.classes == 1 else np.array([b0, b1, b2])
    with np.errstate(invalid="ignore"):
        bz = C_BAR["dl_dz"] * EPS * ref["S_dz"] + (ref["prop3"] * bl[:, :, None]).sum(0) + R.TINY_NORMAL * (abs(ws * T) + abs(wc)) / c.rows
    return dict(lse3=Spec("bar", ref["lse3"], "fp32", bl), out3=Spec("bar", ref["out3"], "fp32", bo), dz=Spec("bar", ref["dz"], "fp32", bz))


def _expect_eval(c, batches=1):
    """after `batches` accumulating calls (batch b's inputs: eval_inputs(c, b))"""
    stats, S = None, 0.0
    for b in range(batches):
        d = eval_inputs(c, b)
        pred, stats, s = R.eval_ref(d["z"], d["labels"], d["n_valid"], c.k, stats)
        S += s
    out = {name: Spec("bar", np.array([float(stats[name])]), "fp32", 0.0) for name in ("seen", "top1", "topk")}
    out["pred"] = Spec("bar", pred.astype(np.float64), "fp32", 0.0)         # of the last batch
    out["loss_sum"] = Spec("bar", np.array([stats["loss_sum"]]), "fp32", C_BAR["ev_loss"] * EPS * S)
    return out


def expect(family, c, *more):
    """{output name: Spec} of a case.  family "head_fwd"; "head_bwd" (more: the forward's own tensors, the dh the rows launch stored);
    "bwd_w"; "ce"; "distill"; "eval" (more: the number of accumulated batches)"""
    return dict(head_fwd=_expect_head_fwd, head_bwd=_expect_head_bwd, bwd_w=_expect_bwdw, ce=_expect_ce, distill=_expect_distill,
                eval=_expect_eval)[family](c, *more)


# ------------------------------------------------------------------------------------------------------------------ restatements
def restate_head(c, mutant=None):
    """({forward outputs}, {backward outputs}) of the float32 restatement, the backward fed the restated forward's own tensors; dx in
    storage values, once more as dx_rows"""
    d = head_inputs(c)
    xa, xb = head_x(c)
    fwd = R.head_fwd_restate(xa, xb, d["W"], d["bias"], d["gamma"], d["beta"], mutant)
    bwd = R.head_bwd_restate(d["dout"], fwd["h"], fwd["xs"], fwd["mean"], fwd["rstd"], d["W"], d["gamma"], d["beta"], mutant)
    bwd.pop("partials")
    bwd["dx"] = cast(bwd["dx"], c.dtype)
    bwd["dx_rows"] = bwd["dx"]
    return {k: np.asarray(v, np.float64) for k, v in fwd.items()}, {k: np.asarray(v, np.float64) for k, v in bwd.items()}


def restate_ce(c, mutant=None):
    d = ce_inputs(c)
    fwd = R.ce_fwd_restate(d["z"], d["labels"], mutant)
    lse = R.ce_fwd_restate(d["z"], d["labels"])["lse"] if mutant else fwd["lse"]        # a mutant of one launch leaves the other right
    return dict(fwd, **R.ce_bwd_restate(d["z"], d["labels"], lse, c.go, mutant))


def restate_distill(c, mutant=None):
    d = distill_inputs(c)
    T, ws, wc = CFGS[c.cfg]
    fwd = R.distill_fwd_restate(d["z"], d["t"], d["labels"], T, ws, wc, mutant)
    lse3 = R.distill_fwd_restate(d["z"], d["t"], d["labels"], T, ws, wc)["lse3"] if mutant else fwd["lse3"]
    return dict(fwd, **R.distill_bwd_restate(d["z"], d["t"], d["labels"], lse3, T, ws, wc, 1.0, mutant))


def restate_eval(c, mutant=None, batches=1):
    tot = dict(seen=0, top1=0, topk=0, loss_sum=0.0)
    for b in range(batches):
        d = eval_inputs(c, b)
        pred, st = R.eval_restate(d["z"], d["labels"], d["n_valid"], c.k, mutant)
        tot = {k: tot[k] + st[k] for k in tot}
    return dict({k: np.array([float(v)]) for k, v in tot.items()}, pred=pred.astype(np.float64))
