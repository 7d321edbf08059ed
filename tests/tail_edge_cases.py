"""The case table of tests/test_gpu_tail_edges.py, its seeded inputs and references, and a host restatement of the tail's dispatch
(csrc/spv_rowops.hip: pick_cfg, pool_mode_of, the LC_FWD / LC_BWD lists with the k_lc rule, the wide condition), shared with
tests/test_tail_ref.py, which checks on the CPU that the table reaches every branch and that the reference's own rounding floor on
exactly these inputs stays well inside the bars.

The shapes are the smallest at which each branch exists: rows = 5 is one full workgroup (4 waves = 4 rows) plus a ragged one.
Every case runs twice: run A p = 0, seed 0; run B p = 0.3 with attention_edge_cases.SEED (high word non-zero)."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

import dropout_ref as D
import tail_ref as R
from attention_edge_cases import SEED, storage_round

RUNS = {"A": dict(p=0.0, seed=0), "B": dict(p=0.3, seed=SEED)}
UP_SEED = 0x5BD1_E995_0BAD_CAFE      # the layer above has its own dropout seed
FWD_CAP_ROWS, BWD_CAP_ROWS, WIDE_FWD_CAP_ROWS = 2048 * 4, 1024 * 4, 2048    # rows one sweep of the capped grids covers

# entry: "tail" (spv_spectre_tail_fwd + _bwd), "ln" (.._ln_fwd + .._ln_bwd), "up" (spv_spectre_tail_fwd + .._bwd_up)
# off: bytes h / out / dout / dh sit off 16-byte alignment; mixed: bf16 storage with fp32 out (forward) and fp32 dout (backward)
# dx_add: a residual gradient is folded into dx_pool; null_dx: dx_pool == NULL; defer: parameter gradients NULL, the caller folds
# `partials`; p_up: the dropout of the layer above ("up" only)
Case = namedtuple("Case", "entry dtype n k_in rows off mixed dx_add null_dx defer p_up", defaults=(0, False, False, False, False, None))


def _both(entry, n, k_in, rows=5, **kw):
    return [Case(entry, dt, n, k_in, rows, **kw) for dt in ("fp32", "bf16")]


CASES = (
    # lane-contiguous kernels
    _both("tail", 768, 512, dx_add=True)            # LC<12,8>: up-sampling windows
    + _both("tail", 512, 768)                       # LC<8,12>: overlapping windows
    + _both("tail", 512, 512, dx_add=True)          # LC<8,8>: identity skip
    + _both("tail", 768, 3072, dx_add=True)         # LC<12,48>: exact windows of 4, WIDE_IN's chunked skip gradient with dx_add
    + _both("tail", 768, 3072)
    # four waves per row
    + _both("tail", 3072, 768, dx_add=True)         # wide
    + _both("tail", 3072, 768, off=8, dx_add=True)  # misaligned: generic <4,12>, REPEAT
    # generic kernel
    + [Case("tail", "bf16", 512, 768, 5, mixed=True)]   # LC refused: generic <4,2>, TABLE, mixed dtype
    + _both("tail", 64, 64) + _both("tail", 64, 64, dx_add=True)    # <4,2> IDENT
    + _both("tail", 64, 256, dx_add=True)           # EXACT pw = 4: LDS quad sums forward, 4-wide stores backward
    + _both("tail", 16, 48)                         # EXACT pw = 3: scalar window loops, 4 live lanes
    + _both("tail", 96, 48, dx_add=True)            # REPEAT r = 2
    + _both("tail", 96, 64)                         # TABLE, up-sampling
    + _both("tail", 104, 512, dx_add=True)          # TABLE, ragged overlapping windows of 5-6
    + _both("tail", 640, 640)                       # <4,3>
    + _both("tail", 1024, 256, dx_add=True)         # <4,4>, REPEAT r = 4
    + _both("tail", 2048, 512)                      # <4,12>
    + _both("tail", 4096, 1024)                     # <4,16>: the longest row, backward LDS 48 KB
    + _both("tail", 10, 8, dx_add=True)             # VEC 1, TABLE, 4-wide LDS staging of x
    + _both("tail", 7, 8)                           # VEC 1, TABLE, 2 n % 4 != 0: scalar staging
    + _both("tail", 1023, 33, dx_add=True)          # VEC 1, all 16 steps, scalar staging
    # fused tail + LayerNorm-2, skip gradient at source
    + _both("ln", 512, 768)
    + _both("up", 768, 512, p_up=0.0) + _both("up", 768, 512, p_up=0.25, dx_add=True)
    # row-count edges
    + _both("tail", 512, 768, rows=1) + _both("tail", 64, 64, rows=1)
    + _both("tail", 512, 768, rows=8197) + _both("ln", 512, 768, rows=8197) + _both("up", 768, 512, rows=8197, p_up=0.25)
    + _both("tail", 64, 64, rows=8197, dx_add=True)
    + _both("tail", 3072, 768, rows=2053)           # the wide forward's 2048 one-row workgroups; `par` alternates
    # dx_pool == NULL, where the header accepts it
    + _both("ln", 512, 768, null_dx=True) + _both("tail", 512, 768, null_dx=True) + _both("tail", 3072, 768, null_dx=True)
    + _both("tail", 64, 256, null_dx=True)
    # deferred fold
    + _both("tail", 512, 768, defer=True) + _both("ln", 512, 768, defer=True) + _both("tail", 64, 64, defer=True)
    + _both("tail", 3072, 768, defer=True)
)
assert len(set(CASES)) == len(CASES)


def case_id(c):
    flags = [f"off{c.off}"] * bool(c.off) + [k for k in ("mixed", "dx_add", "null_dx", "defer") if getattr(c, k)]
    flags += [] if c.p_up is None else [f"pup{c.p_up}"]
    return "-".join([c.entry, c.dtype, str(c.n), str(c.k_in), f"r{c.rows}"] + flags)


# ------------------------------------------------------------------------------------------------------------------ dispatch
LC_PAIRS = ((12, 8), (8, 12), (8, 8), (12, 48))
POOL_IDENT, POOL_EXACT, POOL_TABLE, POOL_REPEAT = "ident", "exact", "table", "repeat"


def pick_cfg(n):
    if n % 4 == 0:
        ni = -(-n // 256)
        for maxi in (2, 3, 4, 12, 16):
            if ni <= maxi:
                return 4, maxi
        return None
    return (1, 16) if n <= 1024 else None


def pool_mode_of(n, k_in):
    return POOL_IDENT if k_in == n else POOL_EXACT if k_in % n == 0 else POOL_REPEAT if n % k_in == 0 else POOL_TABLE


def expected_path(entry, n, k_in, dtype, out_dtype, aligned16=True, dx_pool_null=False, up=False):
    """What serves a call of the C entry point `entry`: ("ln", 8, 12), ("up", 12, 8), ("lc", CO, CI), ("wide",),
    ("generic", vec, maxi, pool mode, sub-branch) or ("refused", why).  out_dtype: the dtype of `out` (forward) / `dout` (backward).
    Sub-branches -- forward EXACT: "quad" (LDS sums of 4 inputs) / "scalar"; forward TABLE: "stage4" (16-byte LDS staging of x) /
    "stage1"; backward EXACT: "store4" / "scalar"; otherwise None."""
    fwd = entry.endswith("_fwd")
    if entry.startswith("spv_spectre_tail_ln_"):
        return ("ln", 8, 12) if (n, k_in) == (512, 768) else ("refused", "shape")
    if entry == "spv_spectre_tail_bwd_up":
        if (n, k_in) != (768, 512) or not up:
            return ("refused", "shape")
        return ("up", 12, 8) if out_dtype == dtype else ("refused", "dout dtype")
    assert entry in ("spv_spectre_tail_fwd", "spv_spectre_tail_bwd") and not up
    cfg = pick_cfg(n)
    if cfg is None:
        return ("refused", "row length")
    k_lc = n if (not fwd and dx_pool_null) else k_in     # no skip gradient asked for: the input width plays no part
    if out_dtype == dtype:
        for co, ci in LC_PAIRS:
            if (n, k_lc) == (64 * co, 64 * ci):
                return ("lc", co, ci)
        if n == 3072 and k_in * 4 == n and aligned16:
            return ("wide",)
    vec, maxi = cfg
    pm = pool_mode_of(n, k_in)
    if not fwd and dx_pool_null and pm != POOL_EXACT:
        return ("refused", "dx_pool == NULL")
    sub = None
    if pm == POOL_EXACT:
        four = vec == 4 and (k_in // n) % 4 == 0
        sub = ("quad" if four else "scalar") if fwd else ("store4" if four else "scalar")
    elif pm == POOL_TABLE and fwd:
        sub = "stage4" if k_in % 4 == 0 and (2 * n) % 4 == 0 else "stage1"
    lds = ((2 * n + 4 * k_in) * 4 if pm == POOL_TABLE else 0) if fwd else 3 * n * 4 + ((2 * k_in + n + 4 * n) * 4 if pm == POOL_TABLE else 0)
    if lds > 64 * 1024:
        return ("refused", "LDS")
    return ("generic", vec, maxi, pm, sub)


ENTRIES = {"tail": ("spv_spectre_tail_fwd", "spv_spectre_tail_bwd"), "ln": ("spv_spectre_tail_ln_fwd", "spv_spectre_tail_ln_bwd"),
           "up": ("spv_spectre_tail_fwd", "spv_spectre_tail_bwd_up")}


def case_paths(c):
    """(forward path, backward path) of a case"""
    f, b = ENTRIES[c.entry]
    other = "fp32" if c.mixed else c.dtype
    return (expected_path(f, c.n, c.k_in, c.dtype, other, c.off == 0),
            expected_path(b, c.n, c.k_in, c.dtype, other, c.off == 0, c.null_dx, c.entry == "up"))


def expected_census(c):
    """what the two calls of a case add to the dispatch census: the wide and the generic kernels have no slot"""
    slot = {"lc": "tail_lc", "ln": "tail_ln", "up": "tail_up"}
    out = {}
    for path in case_paths(c):
        assert path[0] != "refused", (case_id(c), path)
        if path[0] in slot:
            out[slot[path[0]]] = out.get(slot[path[0]], 0) + 1
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
def _rng(c, run):
    return np.random.default_rng(zlib.crc32(f"{case_id(c)}/{run}".encode()))


@lru_cache(maxsize=8)
def inputs(c, run):
    """dict of float64 arrays exactly representable in the case's storage dtype (gamma, beta: fp32 always; dout of a mixed case:
    fp32): h, x, gamma, beta, dout, dx_add [+ x1, gamma2, beta2, dout2 ("ln")] [+ up_src ("up")]"""
    rng = _rng(c, run)
    st = lambda a: storage_round(a, c.dtype)
    f32 = lambda a: storage_round(a, "fp32")
    rows, n, k = c.rows, c.n, c.k_in
    d = dict(h=st(1.5 * rng.standard_normal((rows, n)) + 0.3), x=st(rng.standard_normal((rows, k))),     # the mean of h matters
             gamma=f32(0.5 + rng.random(n)), beta=f32(0.1 * rng.standard_normal(n)),
             dout=(f32 if c.mixed else st)(rng.standard_normal((rows, n))), dx_add=st(rng.standard_normal((rows, k))))
    if c.entry == "ln":
        d.update(x1=st(rng.standard_normal((rows, n))), gamma2=f32(0.5 + rng.random(n)), beta2=f32(0.1 * rng.standard_normal(n)),
                 dout2=st(rng.standard_normal((rows, n))))
    if c.entry == "up":
        d.update(up_src=st(rng.standard_normal((rows, 512))))
    for a in d.values():
        a.setflags(write=False)
    return d


@lru_cache(maxsize=8)
def keep_mask(c, run):
    p = RUNS[run]["p"]
    return D.keep(RUNS[run]["seed"], c.rows, c.n, p) if p > 0 else None


@lru_cache(maxsize=8)
def keep_up(c):
    return D.keep(UP_SEED, c.rows, 512, c.p_up) if c.p_up else None


def reference(c, run, mode="exact", f3=None, ds=None, **perturb):
    """tail_ref on inputs(c, run) under the predicted mask.  f3 / ds ("ln"): the kernel's own stored tensors (tail_ref.tail_ln2).
    perturb: replacements for the arguments dx_add, up, keep, p, x1, P (sensitivity tests)."""
    i, p = inputs(c, run), RUNS[run]["p"]
    keep = perturb.pop("keep", keep_mask(c, run))
    p = perturb.pop("p", p)
    if c.entry == "ln":
        x1 = perturb.pop("x1", i["x1"])
        return R.tail_ln2(i["h"], i["x"], i["gamma"], i["beta"], x1, i["gamma2"], i["beta2"], i["dout2"], keep, p, f3=f3, ds=ds, mode=mode,
                          **perturb)
    dx_add = perturb.pop("dx_add", i["dx_add"] if c.dx_add else None)
    up = perturb.pop("up", (i["up_src"], keep_up(c), c.p_up) if c.entry == "up" else None)
    return R.tail(i["h"], i["x"], i["gamma"], i["beta"], i["dout"], keep, p, dx_add=dx_add, up=up, mode=mode, out_fp32=c.mixed, **perturb)


@lru_cache(maxsize=8)
def exact_reference(c, run):
    """the float64 reference of a case, computed once ("ln": from the reference's own f3 / ds)"""
    ref = reference(c, run)
    for a in ref.values():
        a.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------------------------------ bars
FP32_BAR = {"out": 3e-5, "out2": 3e-5, "mean": 3e-5, "rstd": 3e-5, "mean2": 3e-5, "rstd2": 3e-5}    # test_gpu_ops.TOL[float32]
GRAD_BAR = 6e-5                                                                                    # twice that: test_spectre_linear
BF16_HALF_ULP = 2.0 ** -8    # half an ulp of bf16 at the row's maximum: fp32 arithmetic, each compared tensor rounded once


def bar(c, name):
    """fp32 kernels and the fp32 outputs of bf16 kernels (statistics, column sums, a mixed case's out): the fp32 bars;
    bf16-stored outputs: 2^-8 more"""
    fp32_bar = FP32_BAR.get(name, GRAD_BAR)
    stored_bf16 = c.dtype == "bf16" and name in R.ELEMENTWISE and not (c.mixed and name == "out")
    return fp32_bar + (BF16_HALF_ULP if stored_bf16 else 0.0)


def outputs(c):
    """the names a case's kernels write, in the order they are reported"""
    names = ["out", "mean", "rstd"] + (["out2", "mean2", "rstd2", "ds"] if c.entry == "ln" else []) + ["dh"]
    names += [] if c.null_dx else ["dx_pool"]
    return names + ["dgamma", "dbeta", "dbias"] + (["dgamma2", "dbeta2"] if c.entry == "ln" else [])


def errors(c, got, ref):
    """{name: error as the bars measure it}: the worst row for elementwise outputs, the whole vector otherwise"""
    return {k: float(R.row_errors(got[k], ref[k]).max()) if k in R.ELEMENTWISE else R.col_error(got[k], ref[k]) for k in outputs(c)}
