"""Float64 references and float32 / bf16-storage restatements of the plumbing kernels of csrc/spv_misc.hip (spv_cast,
spv_cast_transpose, spv_weight_shadows[_multi], spv_gelu_fwd / _bwd, spv_axpby, spv_colsum), written from include/spv.h's definitions.
Pure numpy: a reference states the operation on whole arrays in float64; a restatement walks the indices, tiles and summation order of
the kernel in float32, and takes a `mutant` that plants one plausible mistake.  Values travel as float64 arrays holding exactly what
the storage type holds (plumbing_edge_cases.bits turns them into bit patterns)."""
import math

import numpy as np

from edge_judge import F32, cast, half_ulp  # noqa: F401  (half_ulp: re-exported)


def cast_trunc(a, dtype):
    """the mistake: bf16 by dropping the low 16 bits"""
    a32 = np.asarray(a, np.float64).astype(F32)
    if dtype != "bf16":
        return a32.astype(np.float64)
    return (a32.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- cast / transpose
def cast_ref(x, dst):
    return cast(x, dst)


def cast_restate(x, dst, mutant=None):
    """cast_kernel: n / 4 vectors, then the n % 4 tail by workgroup 0"""
    x = np.asarray(x, np.float64).reshape(-1)
    f = cast_trunc if mutant == "truncate" else cast
    n4 = x.size // 4 * 4
    return np.concatenate([f(x[:n4].reshape(-1, 4), dst).reshape(-1), f(x[n4:], dst)])


def grouped_rows(rows, rg, gs, roff):
    """the source row of each of the `rows` rows of a grouped read: (r / rg) * gs + roff + r % rg; rg == 0: the identity"""
    r = np.arange(rows)
    return r if rg == 0 else (r // rg) * gs + roff + r % rg


def cast_transpose_ref(src, dst, rows, cols, ld, rg, gs, roff):
    """dst [cols][ld]: the transpose of the picked rows, + 0 past `rows`"""
    src = np.asarray(src, np.float64)
    if rg:
        picked = src.reshape(-1, gs, cols)[:, roff:roff + rg].reshape(-1, cols)[:rows]
    else:
        picked = src[:rows]
    out = np.zeros((cols, ld))
    out[:, :rows] = cast(picked, dst).T
    return out


def cast_transpose_restate(src, dst, rows, cols, ld, rg, gs, roff, mutant=None):
    """cast_transpose_kernel: grid (cdiv(cols, 64), cdiv(ld, 64)) of 64 x 64 tiles; an element outside [rows, cols] is + 0 in the tile;
    stores where c < cols and r < ld.  Unwritten elements stay NaN."""
    src = np.asarray(src, np.float64)
    out = np.full((cols, ld), np.nan)
    source_rows = grouped_rows(rows, rg, gs, 0 if mutant == "no_roff" else roff)
    for by in range(-(-ld // 64)):
        for bx in range(-(-cols // 64)):
            tile = np.zeros((64, 64))
            for i in range(64):
                r = by * 64 + i
                if r >= rows:
                    continue
                sr = source_rows[r]
                c = np.arange(bx * 64, min(bx * 64 + 64, cols))
                tile[i, :c.size] = src[sr, c]
            cs, rs = min(64, cols - bx * 64), min(64, ld - by * 64)
            out[bx * 64:bx * 64 + cs, by * 64:by * 64 + rs] = (cast_trunc if mutant == "truncate" else cast)(tile[:rs, :cs], dst).T
    return out


# ---------------------------------------------------------------------------------------------------------------- weight shadows
def shadows_ref(w, dtype, ld):
    """(plain [rows, cols], transposed [cols, ld] with + 0 past `rows`)"""
    w = np.asarray(w, np.float64)
    rows, cols = w.shape
    tr = np.zeros((cols, ld))
    tr[:, :rows] = cast(w, dtype).T
    return cast(w, dtype), tr


def shadows_restate(w, dtype, ld, mutant=None):
    """weight_shadow_tile over grid (cdiv(cols, 64), cdiv(ld, 32)): 32 x 64 tiles, zero outside the weight; the transposed copy leaves
    as 8 consecutive rows per thread -- one vector store when ld % 8 == 0, else element by element under r < ld"""
    w = np.asarray(w, np.float64)
    rows, cols = w.shape
    plain, tr = np.full((rows, cols), np.nan), np.full((cols, ld), np.nan)
    tile_rows = -(-(rows if mutant == "pad_rows_unwritten" else ld) // 32)
    for by in range(tile_rows):
        for bx in range(-(-cols // 64)):
            r0, c0 = by * 32, bx * 64
            tile = np.zeros((32, 64))
            rs, cs = max(0, min(32, rows - r0)), min(64, cols - c0)
            tile[:rs, :cs] = w[r0:r0 + rs, c0:c0 + cs]
            plain[r0:r0 + rs, c0:c0 + cs] = cast(tile[:rs, :cs], dtype)
            for r8 in range(0, 32, 8):
                if ld % 8 == 0:
                    n = 8 if r0 + r8 + 7 < ld else 0
                else:
                    n = max(0, min(8, ld - r0 - r8))
                tr[c0:c0 + cs, r0 + r8:r0 + r8 + n] = cast(tile[r8:r8 + n, :cs], dtype).T
    return plain, tr


# ---------------------------------------------------------------------------------------------------------------- GELU
RSQRT2, RSQRT2PI = 0.70710678118654752440, 0.39894228040143267794


def erf64(a):
    a = np.asarray(a, np.float64)
    return np.array([math.erf(v) for v in a.reshape(-1)]).reshape(a.shape)


def gelu_fwd_ref(x):
    """(y, S): y = x/2 + x erf(x / sqrt 2) / 2 in float64 and the sum of the absolute values of its two terms"""
    x = np.asarray(x, np.float64)
    e = erf64(x * math.sqrt(0.5))
    return 0.5 * x * (1.0 + e), 0.5 * np.abs(x) * (1.0 + np.abs(e))


def gelu_bwd_ref(dy, x):
    """(dx, S): dx = dy (1/2 + erf(x / sqrt 2) / 2 + x phi(x))"""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    e = erf64(x * math.sqrt(0.5))
    with np.errstate(under="ignore"):
        xphi = x * np.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    return dy * (0.5 * (1.0 + e) + xphi), np.abs(dy) * (0.5 + 0.5 * np.abs(e) + np.abs(xphi))


def _erf32(z):
    """erff of a float32 array, correctly rounded"""
    return erf64(z.astype(np.float64)).astype(F32)


def gelu_fwd_restate(x, dtype, mutant=None):
    """gelu_erf in float32 operations, then the storage rounding"""
    x = np.asarray(x, np.float64).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if mutant == "tanh":
            y = F32(0.5) * x * (F32(1) + np.tanh(F32(0.7978845608028654) * (x + F32(0.044715) * x * x * x)))
        else:
            y = F32(0.5) * x * (F32(1) + _erf32(x * F32(RSQRT2)))
    return cast(y, dtype)


def gelu_bwd_restate(dy, x, dtype):
    dy, x = np.asarray(dy, np.float64).astype(F32), np.asarray(x, np.float64).astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        g = F32(0.5) * (F32(1) + _erf32(x * F32(RSQRT2))) + x * np.exp(F32(-0.5) * x * x) * F32(RSQRT2PI)
    return cast(dy * g, dtype)


# ---------------------------------------------------------------------------------------------------------------- axpby
def axpby_ref(x, y, a, b):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return a * x + b * y, np.abs(a * x) + np.abs(b * y)


def axpby_restate(x, y, a, b, dtype):
    x, y = np.asarray(x, np.float64).astype(F32), np.asarray(y, np.float64).astype(F32)
    return cast(F32(a) * x + F32(b) * y, dtype)


# ---------------------------------------------------------------------------------------------------------------- column sums
def colsum_ref(x):
    x = np.asarray(x, np.float64)
    return x.sum(0), np.abs(x).sum(0)


def colsum_restate(x, ty, parts, mutant=None):
    """colsum_partial_kernel + colsum_fold_kernel in float32 and in their order: slab y's thread row t adds rows y ty + t, + parts ty,
    ...; a slab's ty thread rows meet in ascending order; the fold's 8 thread rows take slabs p, p + 8, ... and meet in ascending order"""
    x = np.asarray(x, np.float64).astype(F32)
    rows, n = x.shape
    partials = np.zeros((parts, n), F32)
    for y in range(parts - 1 if mutant == "last_slab" else parts):
        for t in range(ty):
            s = np.zeros(n, F32)
            for r in range(y * ty + t, rows, parts * ty):
                s = s + x[r]
            partials[y] = s if t == 0 else partials[y] + s
    red = np.zeros((8, n), F32)
    for py in range(8):
        for p in range(py, parts, 8):
            red[py] = red[py] + partials[p]
    out = np.zeros(n, F32)
    for q in range(8):
        out = out + red[q]
    return out.astype(np.float64)
