"""The case tables of tests/test_gpu_branch_edges.py (csrc/spv_branch.hip: spv_spectrum_log1p, spv_conv3x3_fwd / _dgrad / _wgrad,
spv_token_pool_fwd / _bwd), their seeded inputs, a host restatement of the dispatch written in that source and what each case is judged
by (tests/edge_judge.py holds the judging function).  tests/test_branch_ref.py shows on the CPU that the tables reach every branch they
claim, that a float32 restatement of each kernel (tests/branch_ref.py) passes the judge on exactly these inputs and that plausible
mistakes do not.  No GPU, no spectre_vit.

expect(family, case) -> {output name: Spec}; poison(family, case) -> {output name: (mode, mask)} names the elements the Spec cannot
speak for: mode "nan" -- a planted NaN copied by a gather, NaN by position; mode "nonfinite" -- an output whose window holds a planted
inf or NaN (a whole plane of the spectrum), which must be inf or NaN.  settle() checks those and hands the rest to verdict().

Bars.  Gather workspaces, the "int" set of the convolutions (operands integers in [-3, 3]: exact in float32, exact_ok() asserts it) and
the pooling cases with power-of-two windows over integers: kind "bits".  The "normal" (and "special") set of the convolutions:
gemm_edge_cases.bar(ref, S, n, dout), n = the products of the padded reduction + one per slab + one for the bias; it holds no measured
constant.  Pooling: |got - ref| <= (n + 2) 2^-24 S_i (+ half a bf16 ulp), forward n = the window's length and S_i its mean |y|,
backward n = two per contributing window + one for `add`.

The spectrum's bar is the one with a measured constant, because the device's sincospi / hypotf / log1pf carry a few ulp:

    |got - ref| <= c 2^-24 (S_i / (1 + |X_i|) + |ref_i|)   (+ half a bf16 ulp of the reference for bf16 outputs)

S_i the plane's sum of |x|, X_i the float64 bin (an error e of the bin's magnitude moves log1p by e / (1 + |X|); the second term is
the rounding of log1pf itself); where S_i = 0 the output must be the reference's +0.  c is four times the floor, rounded up: the floor
is the worst ratio of branch_ref.spectrum_restate (float32) against float64 on exactly these inputs (tests/test_branch_ref.py prints
it and asserts floor <= c / 4); the factor 4 leaves room for fused multiply-adds, another summation order and the few-ulp device
functions -- the convention of tests/embed_edge_cases.py.  Measured on the CPU, never from the kernel's output:

    spectrum      floor 0.697   c = 3      (1 x 1: 0.51, 2 x 2: 0.70, 17 x 9: 0.54, 32 x 32: 0.44, 126 x 124: 0.27, 147 x 107: 0.29)"""
import functools
from collections import namedtuple

import numpy as np

import branch_ref as R
from edge_judge import EPS, LIMIT_BYTES, Spec, cast, cdiv, floor_ratio, half_ulp, round8, verdict  # noqa: F401  (re-exported)
from gemm_edge_cases import bar, draw, nt_plan, q, rng_of, worst_ratio  # noqa: F401
from permut_edge_cases import CODE, DTYPES, ES, HUGE, TINY, bits  # noqa: F401

C_BAR = dict(spectrum=3)
F32 = np.float32
STAGES = [(3, 32, 17), (9, 30, 15), (27, 28, 13), (81, 26, 11)]      # test_gpu_spectre_branch.STAGES: (Cin, H, W) of the preset's stages


# ------------------------------------------------------------------------------------------------------------------ dispatch
GRID_CAP = 65536
SPECTRUM_LIMIT = 16384         # floats of LDS (64 KiB)


def grid_for(total):
    return min(cdiv(total, 256), GRID_CAP)


def trips(total):
    """trips of a grid-stride loop over `total` elements"""
    return cdiv(total, 256 * grid_for(total))


def spectrum_floats(H, W):
    return 2 * W + 2 * H + 2 * H * (W // 2 + 1)


def geometry(c):
    """dict(M, Mp, K, Kp, Mi, Kd) of a convolution case"""
    M = c.B * (c.H - 2) * (c.W - 2)
    return dict(M=M, Mp=round8(M), K=9 * c.Cin, Kp=round8(9 * c.Cin), Mi=c.B * c.H * c.W, Kd=round8(9 * c.Cout))


def gather_totals(c):
    g = geometry(c)
    return dict(fwd=g["M"] * g["Kp"], dgrad=g["Mi"] * g["Kd"], dyt=c.Cout * g["Mp"], colst=g["K"] * g["Mp"])


def _lo(c, name):
    return ES[c.dtype if name not in ("bias", "dw", "ws") else "fp32"] % 16 if c.off == name else 0


def conv_plan(entry, c):
    """nt_plan of the GEMM call the entry makes"""
    g, d = geometry(c), CODE.get(c.dtype, 99)
    if entry == "fwd":
        return nt_plan(d, d, g["M"], c.Cout, g["Kp"], g["Kp"], g["Kp"], c.Cout, _lo(c, "cols"), _lo(c, "w"), _lo(c, "y"), _lo(c, "bias"))
    if entry == "dgrad":
        return nt_plan(d, d, g["Mi"], c.Cin, g["Kd"], g["Kd"], g["Kd"], c.Cin, _lo(c, "cols"), _lo(c, "wd"), _lo(c, "dx"))
    return nt_plan(d, 0, c.Cout, g["K"], g["Mp"], g["Mp"], g["Mp"], g["K"], _lo(c, "dyt"), _lo(c, "colst"), _lo(c, "dw"), splits=c.splits,
                   ws_lo=-1 if c.ws == "null" else _lo(c, "ws"))


def preset_splits(cin, cout, mp):
    """branch_ops.conv3x3_wgrad's choice"""
    tiles = cdiv(cout, 128) * cdiv(9 * cin, 128)
    return max(1, min(256 // tiles, mp // 1024, 256))


def preset_census(B=512):
    """{(entry, dtype, kernel, reduce)} of the preset's four stages at batch B"""
    out = set()
    for cin, H, W in STAGES:
        for dt in DTYPES:
            c = CV(dt, B, H, W, cin, 3 * cin)
            c = c._replace(splits=preset_splits(cin, 3 * cin, geometry(c)["Mp"]))
            for entry in ("fwd", "dgrad", "wgrad"):
                p = conv_plan(entry, c)
                out.add((entry, dt, p["kernel"], p["reduce"]))
    return out


# ------------------------------------------------------------------------------------------------------------------ tables
SP = namedtuple("SP", "dtype B C H W kind off", defaults=("plain", ""))
CV = namedtuple("CV", "dtype B H W Cin Cout which entries splits off ws tag", defaults=("normal", "fdw", 1, "", "given", ""))
PL = namedtuple("PL", "dtype B L C T ldo which add off dirs", defaults=("normal", 1, "", "fb"))
Refused = namedtuple("Refused", "entry why case match wrote", defaults=((),))

PLANES = ((1, 1), (1, 8), (8, 1), (2, 2), (17, 9), (13, 31), (32, 32), (28, 28), (126, 124), (147, 107))       # 16 376 floats, and 16 384: the limit itself
SPECIAL_PLANES = ("zero", "constant", "inf", "nan", "plain", "plain")        # the (2, 3) planes of the special case, in order

SPECTRUM_CASES = [SP(dt, b, ch, h, w) for dt in DTYPES for h, w in PLANES for b, ch in ((1, 1), (2, 3))] + \
    [SP(dt, 2, 3, 17, 9, "special") for dt in DTYPES] + [SP(dt, 2, 3, 17, 9, "plain", "both") for dt in DTYPES]
SPECTRUM_REFUSED = [Refused("spectrum", why, SP("fp32", *v), m) for why, v, m in (
    ("plane-127x124", (1, 1, 127, 124), "66016"), ("plane-148x107", (1, 1, 148, 107), "65976"), ("B=0", (0, 1, 4, 4), "empty"), ("H=0", (1, 1, 0, 4), "empty"))] + \
    [Refused("spectrum", "dtype", SP("99", 1, 1, 4, 4), "bad dtype")]

CONV_SHAPES = (
    (1, 3, 3, 1, 1),         # one output position: Mp = 8 > M = 1
    (2, 5, 4, 1, 5),         # M = 12
    (3, 6, 7, 3, 9),         # 27 real columns of 32, M = 60
    (2, 5, 5, 8, 3),         # 72 columns, no padding, ldc = 3
    (2, 9, 8, 27, 5),        # Kp = 248, M = 84
    (2, 4, 6, 2, 8),         # M = 16: M % 8 == 0, Mp == M; 72 data-gradient columns, no padding
    (3, 7, 3, 2, 3))         # M = 15: M % 8 == 7
ALIGNED_OK = ("x", "y", "dy", "dx", "dw", "bias")
ALIGNED_MUST = (("fwd", "cols"), ("fwd", "w"), ("dgrad", "cols"), ("dgrad", "wd"), ("wgrad", "dyt"), ("wgrad", "colst"), ("wgrad", "ws"))
ENTRY_OF = dict(x="fw", y="f", dy="dw", dx="d", dw="w", bias="f")


def _conv_cases():
    out = []
    for dt in DTYPES:
        for shape in CONV_SHAPES:
            out += [CV(dt, *shape, which) for which in ("int", "normal")]
        # the weight gradient's split-K: 2, 3 and 7 slabs asked for; at Mp = 88 bf16 (64-element K-tiles) gets 2, 2 and 2, fp32 (32) 2, 3
        # and 3: fewer than asked
        for s in (2, 3, 7):
            out += [CV(dt, 2, 9, 8, 27, 5, which, "w", s) for which in ("int", "normal")]
        out.append(CV(dt, 1, 3, 3, 1, 1, "normal", "w", 4, tag="collapses"))        # one slab: the workspace stays untouched
        out.append(CV(dt, 3, 6, 7, 3, 9, "special"))
        out += [CV(dt, 2, 5, 4, 1, 5, "normal", ENTRY_OF[name], off=name) for name in ALIGNED_OK]
        # Mp = 2176 = 34 x 64: slices of 2176 and 1088 (bf16: the direct-to-LDS kernel) and of 768 (the tile kernel)
        out += [CV(dt, 2, 34, 36, 1, 3, which, "w", s, tag=f"slice{k}") for which in ("int", "normal") for s, k in ((1, 2176), (2, 1088), (3, 768))]
        # second trip of each gather loop: the smallest totals above 65536 x 256 = 16 777 216 elements
        out.append(CV(dt, 18, 250, 250, 1, 1, "int", "f", tag="trip2"))             # 1 107 072 x 16 = 17 713 152
        out.append(CV(dt, 18, 250, 250, 1, 1, "int", "d", tag="trip2"))             # 1 125 000 x 16 = 18 000 000
        out.append(CV(dt, 16, 250, 250, 2, 18, "int", "w", 4, tag="trip2"))         # 18 x 984 064 = 17 713 152, twice
    return out


CONV_CASES = _conv_cases()
_BASE = CV("fp32", 2, 5, 4, 1, 5)
_SPLIT = CV("fp32", 2, 9, 8, 27, 5, entries="w")       # Mp = 88: two slabs and more in both dtypes
CONV_REFUSED = [Refused(e, why, _BASE._replace(**kw), f"spv_conv3x3_{e}: bad") for e in ("fwd", "dgrad", "wgrad") for why, kw in (
    ("B=0", dict(B=0)), ("H=2", dict(H=2)), ("W=2", dict(W=2)), ("Cin=0", dict(Cin=0)), ("Cout=0", dict(Cout=0)), ("dtype", dict(dtype="99")))] + \
    [Refused("wgrad", "splits=0", _SPLIT._replace(splits=0), "spv_gemm_nt: splits=0", ("dyt", "colst")),
     Refused("wgrad", "splits=2-null-workspace", _SPLIT._replace(splits=2, ws="null"), "spv_gemm_nt: split-K needs", ("dyt", "colst"))] + \
    [Refused(e, f"{name}-off-{dt}", _SPLIT._replace(dtype=dt, off=name, splits=2 if name == "ws" else 1),
             "spv_gemm_nt: split-K needs a 16-byte aligned workspace" if name == "ws" else "spv_gemm_nt: A/B must be 16-byte aligned",
             dict(fwd=("cols",), dgrad=("cols",), wgrad=("dyt", "colst"))[e]) for dt in DTYPES for e, name in ALIGNED_MUST]

POOL_LT = ((1, 1), (1, 5), (5, 1), (40, 65), (64, 65), (65, 65), (66, 65), (130, 65), (260, 65), (450, 65), (7, 3))
POOL_EXACT = ((130, 65), (260, 65))


def _pool_cases():
    out = []
    for dt in DTYPES:
        i = 0
        for L, T in POOL_LT:
            for C in (1, 7, 8):
                for ldo in sorted({C, round8(C), C + 3}):
                    out.append(PL(dt, (1, 3)[i % 2], L, C, T, ldo, "int" if (L, T) in POOL_EXACT else "normal", (i // 2) % 2))
                    i += 1
        out += [PL(dt, 3, 66, 7, 65, 10, "normal", 1, name, "f" if name in ("y", "out") else "b") for name in ("y", "out", "dout", "add", "dy")]
        out.append(PL(dt, 2, 5, 2050, 4100, 2056, "normal", 0, "", "f"))        # second trip: 2 x 4100 x 2056 = 16 859 200 outputs
        out.append(PL(dt, 2, 4100, 2050, 3, 2056, "normal", 1, "", "b"))        # second trip: 2 x 4100 x 2050 = 16 810 000 outputs
    return out


POOL_CASES = _pool_cases()
_PBASE = PL("fp32", 2, 6, 5, 4, 8)
POOL_REFUSED = [Refused(e, why, _PBASE._replace(**kw), f"spv_token_pool_{e}: bad") for e in ("fwd", "bwd") for why, kw in (
    ("B=0", dict(B=0)), ("L=0", dict(L=0)), ("C=0", dict(C=0)), ("T=0", dict(T=0)), ("ldo=C-1", dict(ldo=4)), ("dtype", dict(dtype="99")))]

ALL = dict(spectrum=SPECTRUM_CASES, conv=CONV_CASES, pool=POOL_CASES)


def case_id(c):
    if isinstance(c, Refused):
        return f"{c.entry}-{c.why}"
    s = "-".join(str(v) for v in c if v != "")
    return s


# ------------------------------------------------------------------------------------------------------------------ spectrum
@functools.lru_cache(maxsize=4)
def spectrum_inputs(c):
    """img (B, C, H, W) float64, storage-exact fp32; the same for both output types"""
    rng = rng_of("spectrum", c.B, c.C, c.H, c.W, c.kind)
    img = rng.standard_normal((c.B, c.C, c.H, c.W)).astype(F32).astype(np.float64)
    if c.kind == "special":
        planes = img.reshape(c.B * c.C, c.H, c.W)
        for p, kind in enumerate(SPECIAL_PLANES):
            if kind == "zero":
                planes[p] = 0.0
            elif kind == "constant":
                planes[p] = 1.25
            elif kind in ("inf", "nan"):
                planes[p, 5, 3] = np.inf if kind == "inf" else np.nan
    img.setflags(write=False)
    return img


def spectrum_bar(ref, dtype):
    with np.errstate(invalid="ignore"):
        b = C_BAR["spectrum"] * EPS * (ref["S"] / (1 + ref["X"]) + np.abs(ref["out"]))
    return np.nan_to_num(b) + half_ulp(np.nan_to_num(ref["out"]), dtype)


def _spectrum_model(c):
    ref = R.spectrum_ref(spectrum_inputs(c))
    bad = np.isnan(ref["out"])
    return {"out": Spec("bar", np.nan_to_num(ref["out"]), c.dtype, spectrum_bar(ref, c.dtype))}, ({"out": ("nonfinite", bad)} if bad.any() else {})


# ------------------------------------------------------------------------------------------------------------------ convolutions
def slabs_of(c):
    return conv_plan("wgrad", c._replace(off="", ws="given"))["splits"]


def chain(entry, c):
    """n of the bar: the products of the padded reduction + one per slab + one for the bias"""
    g = geometry(c)
    return dict(fwd=g["Kp"] + 1 + 1, dgrad=g["Kd"] + 1, wgrad=g["Mp"] + slabs_of(c))[entry]


def exact_ok(c):
    """the integer set is exact in float32: operands in [-3, 3], so every partial sum stays below 2^24"""
    g = geometry(c)
    return all(9 * n + 3 < 2 ** 24 for n in (g["Kp"], g["Kd"], g["Mp"]))


@functools.lru_cache(maxsize=2)
def conv_inputs(c):
    """dict(x (B, H, W, Cin), dy (B, Ho, Wo, Cout), w (Cout, Cin, 3, 3), bias (Cout,)) float32 arrays holding storage-exact values (w in
    the case's dtype, as the packed operands are; bias fp32)"""
    key = c._replace(entries="", splits=1, off="", ws="given", tag="")
    rng = rng_of("conv", *key)
    which = "normal" if c.which == "special" else c.which
    shapes = dict(x=(c.B, c.H, c.W, c.Cin), dy=(c.B, c.H - 2, c.W - 2, c.Cout), w=(c.Cout, c.Cin, 3, 3), bias=(c.Cout,))
    d = {k: draw(rng, s, "fp32" if k == "bias" else c.dtype, which).astype(F32) for k, s in shapes.items()}
    if c.which == "special":
        # an eighth of the scale, so that the largest finite value times a weight or a neighbour, summed, stays finite (test_branch_ref.py
        # asserts S < 2^127 on every output outside the poisoned windows)
        d = {k: v * F32(0.125) for k, v in d.items()}
        finite, poisonous = [0.0, -0.0, TINY[c.dtype], -TINY[c.dtype], HUGE[c.dtype]], [np.inf, -np.inf, np.nan]
        for k in ("x", "dy"):       # the non-finite ones in channel 0, so that the weight gradient keeps outputs no poisoned window reaches
            flat, ch = d[k].reshape(-1), d[k].shape[-1]
            at = rng.permutation(flat.size // ch)[:len(finite) + len(poisonous)] * ch
            flat[at[:len(poisonous)]] = np.array(poisonous, F32)
            flat[at[len(poisonous):] + (ch - 1)] = np.array(finite, F32)
    for v in d.values():
        v.setflags(write=False)
    return d


def packed(c):
    """the operands the caller packs: w [Cout][Kp] and wd [Cin][Kd], zero past the real columns"""
    d, g = conv_inputs(c), geometry(c)
    w = np.zeros((c.Cout, g["Kp"]), F32)
    w[:, :g["K"]] = d["w"].reshape(c.Cout, -1)
    wd = np.zeros((c.Cin, g["Kd"]), F32)
    wd[:, :9 * c.Cout] = R.wd_of(d["w"])
    return w, wd


def _clean(a):
    """(a with its non-finite values replaced by zero, where they were)"""
    bad = ~np.isfinite(a)
    return (np.where(bad, F32(0), a), bad) if bad.any() else (a, None)


def _value_spec(c, ref, S, n, dout):
    if c.which == "int":
        return Spec("bits", cast(ref, dout), dout)
    return Spec("bar", ref, dout, bar(ref, S, n, dout))


def _ws_spec(c, ref, poison, name):
    nan = np.isnan(ref)
    if nan.any():
        poison[name] = ("nan", nan)
        ref = np.where(nan, F32(0), ref)
    return Spec("bits", ref, c.dtype)


@functools.lru_cache(maxsize=2)
def _conv_model(c):
    """{entry: (specs, poison)} of the entries the case runs"""
    d, g = conv_inputs(c), geometry(c)
    w64 = d["w"].astype(np.float64)
    out = {}
    x, xbad = _clean(d["x"])
    dy, dybad = _clean(d["dy"])
    hit = lambda a, b: (np.asarray(a, np.float64) @ np.asarray(b, np.float64).T) > 0       # a window holds a planted non-finite value
    if "f" in c.entries:
        poison = {}
        specs = dict(cols=_ws_spec(c, R.im2col(d["x"], g["Kp"]), poison, "cols"))
        ref, S = R.conv_fwd(x, w64, d["bias"].astype(np.float64))
        specs["y"] = _value_spec(c, ref, S, chain("fwd", c), c.dtype)
        if xbad is not None:
            poison["y"] = ("nonfinite", hit(R.im2col(xbad.astype(F32), g["K"]), np.ones((c.Cout, g["K"]))))
        out["fwd"] = (specs, poison)
    if "d" in c.entries:
        poison = {}
        specs = dict(cols=_ws_spec(c, R.dcols(d["dy"], g["Kd"]), poison, "cols"))
        ref, S = R.conv_dgrad(dy, w64)
        specs["dx"] = _value_spec(c, ref, S, chain("dgrad", c), c.dtype)
        if dybad is not None:
            poison["dx"] = ("nonfinite", hit(R.dcols(dybad.astype(F32), 9 * c.Cout), np.ones((c.Cin, 9 * c.Cout))))
        out["dgrad"] = (specs, poison)
    if "w" in c.entries:
        poison = {}
        specs = dict(dyt=_ws_spec(c, R.transposed(d["dy"].reshape(g["M"], c.Cout), g["Mp"]), poison, "dyt"),
                     colst=_ws_spec(c, R.transposed(R.im2col(d["x"], g["K"]), g["Mp"]), poison, "colst"))
        ref, S = R.conv_wgrad(dy, x)
        specs["dw"] = _value_spec(c, ref, S, chain("wgrad", c), "fp32")
        if xbad is not None or dybad is not None:
            a = (dybad if dybad is not None else np.zeros(d["dy"].shape, bool)).reshape(g["M"], c.Cout).astype(F32)
            b = R.im2col((xbad if xbad is not None else np.zeros(d["x"].shape, bool)).astype(F32), g["K"])
            poison["dw"] = ("nonfinite", hit(a.T, np.ones((g["K"], g["M"]))) | hit(np.ones((c.Cout, g["M"])), b.T))
        out["wgrad"] = (specs, poison)
    return out


def restate_conv(entry, c, mutant=None):
    """the entry's workspaces and output as float32 arithmetic on the restated layouts gives them, as float64 storage values"""
    d, g = conv_inputs(c), geometry(c)
    w, wd = packed(c)
    order = dict(k_order_yxc="yxc", swap_kykx="cxy").get(mutant, "cyx")
    pad = np.nan if mutant == "pads_unwritten" else 0.0
    f64 = lambda a: np.asarray(a, np.float64)
    if entry == "fwd":
        cols = R.im2col(d["x"], g["Kp"], order, pad)
        return dict(cols=f64(cols), y=cast(R.matmul32(cols, w, d["bias"]), c.dtype))
    if entry == "dgrad":
        cols = R.dcols(d["dy"], g["Kd"], mutant, pad)
        return dict(cols=f64(cols), dx=cast(R.matmul32(cols, wd), c.dtype))
    dyt = R.transposed(d["dy"].reshape(g["M"], c.Cout), g["Mp"], mutant)
    colst = R.transposed(R.im2col(d["x"], g["K"], order), g["Mp"], mutant)
    if mutant == "pads_unwritten":
        dyt[:, g["M"]:], colst[:, g["M"]:] = np.nan, np.nan
    return dict(dyt=f64(dyt), colst=f64(colst), dw=cast(R.matmul32(dyt, colst), "fp32"))


# ------------------------------------------------------------------------------------------------------------------ pooling
@functools.lru_cache(maxsize=2)
def pool_inputs(c):
    """dict(y (B, L, C), dout (B, T, ldo) with NaN in its pad columns, add (B, L, C) or None) float32 arrays of storage-exact values"""
    rng = rng_of("pool", c.dtype, c.B, c.L, c.C, c.T, c.ldo, c.which)
    d = dict(y=draw(rng, (c.B, c.L, c.C), c.dtype, c.which).astype(F32) if "f" in c.dirs else None)
    if "b" in c.dirs:
        dout = draw(rng, (c.B, c.T, c.ldo), c.dtype, c.which).astype(F32)
        dout[..., c.C:] = np.nan
        d.update(dout=dout, add=draw(rng, (c.B, c.L, c.C), c.dtype, c.which).astype(F32) if c.add else None)
    return d


def pool_exact_ok(c):
    """integers in [-3, 3] over windows of one power-of-two length: every average and every sum is exact in float32 and in bf16 (at
    most 3 + 3 + 3 with two fractional bits)"""
    return c.L % c.T == 0 and c.L // c.T in (1, 2, 4)


def _pool_model(c):
    d = pool_inputs(c)
    out = {}
    for entry, name, r in (("pool_fwd", "out", R.pool_fwd(d["y"], c.T, c.ldo) if "f" in c.dirs else None),
                           ("pool_bwd", "dy", R.pool_bwd(d["dout"], c.L, c.C, d["add"]) if "b" in c.dirs else None)):
        if r is None:
            continue
        ref = r[name]
        if c.which == "int":
            out[entry] = {name: Spec("bits", ref, c.dtype)}
        else:
            out[entry] = {name: Spec("bar", ref, c.dtype, (r["n"] + 2) * EPS * r["S"] + half_ulp(ref, c.dtype))}
    return out


def restate_pool(entry, c, mutant=None):
    d = pool_inputs(c)
    if entry == "pool_fwd":
        return dict(out=cast(R.pool_fwd_restate(d["y"], c.T, c.ldo, mutant), c.dtype))
    return dict(dy=cast(R.pool_bwd_restate(d["dout"], c.L, c.C, d["add"], mutant), c.dtype))


# ------------------------------------------------------------------------------------------------------------------ judging
def expect(family, c):
    """{output name: Spec} of family "spectrum", "fwd", "dgrad", "wgrad", "pool_fwd" or "pool_bwd\""""
    if family == "spectrum":
        return _spectrum_model(c)[0]
    if family.startswith("pool"):
        return _pool_model(c)[family]
    return _conv_model(c)[family][0]


def poison(family, c):
    if family == "spectrum":
        return _spectrum_model(c)[1]
    return {} if family.startswith("pool") else _conv_model(c)[family][1]


def settle(specs, got, poisoned):
    """verdict() after the elements it cannot speak for: (ok, {name: worst ratio})"""
    got, fine = dict(got), True
    for name, (mode, mask) in poisoned.items():
        g = np.asarray(got[name], np.float64)
        if g.shape != mask.shape:
            return False, {name: np.inf}
        fine = fine and bool(np.isnan(g[mask]).all() if mode == "nan" else (~np.isfinite(g[mask])).all())
        got[name] = np.where(mask, specs[name].ref, g)
    ok, worst = verdict(specs, got)
    if not fine:
        worst = dict(worst, poisoned=np.inf)
    return ok and fine, worst


def restate(family, c, mutant=None):
    if family == "spectrum":
        return dict(out=cast(R.spectrum_restate(spectrum_inputs(c), mutant), c.dtype))
    return restate_pool(family, c, mutant) if family.startswith("pool") else restate_conv(family, c, mutant)


def entries_of(c):
    return [e for e, k in (("fwd", "f"), ("dgrad", "d"), ("wgrad", "w")) if k in c.entries]


def buffer_elems(c):
    """{buffer: elements} of the larger device buffers of a case"""
    if isinstance(c, SP):
        return dict(img=c.B * c.C * c.H * c.W)
    if isinstance(c, PL):
        big = c.B * c.L * c.C
        return dict(y=big if "f" in c.dirs else 0, out=c.B * c.T * c.ldo, dy=big if "b" in c.dirs else 0)
    g = geometry(c)
    t = gather_totals(c)
    return dict(x=c.B * c.H * c.W * c.Cin, dy=g["M"] * c.Cout, cols=t["fwd"] if "f" in c.entries else 0, dcols=t["dgrad"] if "d" in c.entries else 0,
                dyt=t["dyt"] if "w" in c.entries else 0, colst=t["colst"] if "w" in c.entries else 0)
