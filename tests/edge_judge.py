"""What tests/plumbing_edge_cases.py and tests/embed_edge_cases.py (with their *_ref.py) share: the storage rounding, half a bf16 ulp,
seeded inputs with planted special values, and the judging function of the GPU tests and of the CPU tests that prove it.  Pure numpy.

A Spec of kind "bits" holds an output to its reference bit for bit; kind "bar" holds |got - ref| elementwise within the bar.  Where the
bar is 0 and the reference is a zero -- padding, a CLS slot, a product with a planted zero -- the output must be that zero, sign
included."""
from collections import namedtuple

import numpy as np

from dropout_ref import bf16_round
from permut_edge_cases import HUGE, TINY, bits, worst_ratio

F32 = np.float32
EPS = 2.0 ** -24
LIMIT_BYTES = 80 * 2 ** 20


def cdiv(a, b):
    return -(-a // b)


def round8(n):
    return (n + 7) // 8 * 8


def cast(a, dtype):
    """round to nearest even onto the storage grid of `dtype` ("fp32" / "bf16"), as float64; the largest finite float32 becomes bf16 inf"""
    with np.errstate(over="ignore"):
        a32 = np.asarray(a, np.float64).astype(F32)
    return bf16_round(a32) if dtype == "bf16" else a32.astype(np.float64)


def half_ulp(ref, dtype):
    """half a unit in the last place of `dtype` at the reference value: 0 at a reference of exactly 0 (and for fp32 outputs, whose
    roundings are in the bar's sum term)"""
    ref = np.asarray(ref, np.float64)
    if dtype != "bf16":
        return np.zeros(ref.shape)
    with np.errstate(invalid="ignore"):
        e = np.frexp(np.where(np.isfinite(ref), np.abs(ref), 0.0))[1] - 1        # |ref| in [2^e, 2^(e+1))
    return np.where(ref == 0, 0.0, np.ldexp(1.0, np.maximum(e, -126) - 8))


def values(rng, shape, dtype, plant="all"):
    """standard normals rounded to the storage type; plant "all": + 0, - 0, a subnormal, + inf, - inf and the largest finite value at
    seeded places (arrays of two elements and more), "finite": + 0, - 0 and the subnormals only (sums: an addition cannot underflow),
    "finite_huge": those and +- the largest finite value, "zeros": + 0 and - 0 (products under a relative bar, which a subnormal
    result cannot meet), "": none.  Read-only."""
    a = cast(rng.standard_normal(shape), dtype).reshape(-1)
    finite = [0.0, -0.0, TINY[dtype], -TINY[dtype]]
    vals = dict(all=finite + [np.inf, -np.inf, HUGE[dtype]], finite=finite, finite_huge=finite + [HUGE[dtype], -HUGE[dtype]],
                zeros=[0.0, -0.0]).get(plant, [])
    k = min(len(vals), a.size // 2)
    if k:
        a[rng.permutation(a.size)[:k]] = np.array(vals)[rng.permutation(len(vals))[:k]]
    a = a.reshape(shape)
    a.setflags(write=False)
    return a


Spec = namedtuple("Spec", "kind ref dtype bar", defaults=(None,))


def verdict(specs, got):
    """(every output within its Spec, {name: worst ratio to the bar -- 0 or inf for a bit-for-bit output})"""
    assert set(got) == set(specs), (sorted(got), sorted(specs))
    ok, worst = True, {}
    for name, s in specs.items():
        g = np.asarray(got[name], np.float64)
        assert g.shape == s.ref.shape, (name, g.shape, s.ref.shape)
        if s.kind == "bits":
            bad = int((np.isnan(g) | (bits(np.where(np.isnan(g), 0.0, g), s.dtype) != bits(s.ref, s.dtype))).sum())
            good, w = bad == 0, (0.0 if bad == 0 else np.inf)
        else:
            good, w = worst_ratio(g, s.ref, s.bar)
            zero = (s.ref == 0) & (np.broadcast_to(s.bar, s.ref.shape) == 0)
            if not bool(((g[zero] == 0) & (np.signbit(g[zero]) == np.signbit(s.ref[zero]))).all()):
                good, w = False, np.inf
        ok, worst[name] = ok and good, w
    return ok, worst


def floor_ratio(got, ref, S):
    """the worst err_i / (2^-24 S_i) of a restated fp32 output (elements with S_i == 0 must be exact)"""
    got, ref, S = (np.asarray(v, np.float64).reshape(-1) for v in (got, ref, S))
    err = np.abs(got - ref)
    assert bool((err[S == 0] == 0).all())
    return float((err[S > 0] / (EPS * S[S > 0])).max()) if (S > 0).any() else 0.0
