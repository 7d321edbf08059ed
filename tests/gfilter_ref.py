"""The learnable global-filter token mixer's float64 reference, a host restatement of csrc/spv_gfilter_core.h, a float32 restatement of
the generic kernels' arithmetic, and the case tables of tests/test_gpu_gfilter_mixer.py.  Shared with tests/test_gfilter_mixer.py,
which checks on the CPU that the reference equals torch.fft + torch.autograd in float64, that the circulant form agrees, that the
tables reach every branch and that the restatement agrees with the library's host-side answers.

Definition, for x (B, N, D) and K = N // 2 + 1, W (K, D) complex:

    X = rfft(x, axis=1, ortho);   y = irfft(X * W, n=N, axis=1, ortho)

irfft ignores the imaginary part of the DC bin and, for even N, of the Nyquist bin: W_eff is W with those zeroed.
    dx = irfft(rfft(dy) * conj(W_eff))          dW[k, d] = c_k sum_b conj(X[b, k, d]) G[b, k, d],  G = rfft(dy),
c_k = 1 at the DC / Nyquist bins, else 2; the imaginary part of dW there is exactly +0.

The bars are the project's: spectral_edge_cases.TRANSFORM_BAR, GRAD_BAR and bar()."""
from collections import namedtuple

import numpy as np

import spectral_edge_cases as C
from spectral_edge_cases import GRAD_BAR, TRANSFORM_BAR, bar, case_id, rng_of  # noqa: F401  (the test files read them here)

DTYPES = C.DTYPES
CODE = C.CODE


# ------------------------------------------------------------------------------------------------------------------ reference
def bins(tokens):
    return tokens // 2 + 1


def as_complex(w):
    """(K, D, 2) real -> (K, D) complex128"""
    w = np.asarray(w, np.float64)
    return w[..., 0] + 1j * w[..., 1]


def inert(tokens):
    """the bins whose imaginary part irfft ignores"""
    return [0] + ([tokens // 2] if tokens % 2 == 0 else [])


def weights(tokens):
    """c_k: how often bin k stands in the Hermitian spectrum"""
    c = np.full(bins(tokens), 2.0)
    c[inert(tokens)] = 1.0
    return c


def w_eff(w, tokens):
    wc = as_complex(w).copy()
    wc[inert(tokens)] = wc[inert(tokens)].real
    return wc


def fwd(x, w):
    x = np.asarray(x, np.float64)
    N = x.shape[1]
    return np.fft.irfft(np.fft.rfft(x, axis=1, norm="ortho") * as_complex(w), n=N, axis=1, norm="ortho")


def dx(dy, w):
    dy = np.asarray(dy, np.float64)
    N = dy.shape[1]
    return np.fft.irfft(np.fft.rfft(dy, axis=1, norm="ortho") * np.conj(w_eff(w, N)), n=N, axis=1, norm="ortho")


def dw(x, dy):
    """(K, D, 2) float64; the inert imaginary parts are +0"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    N = x.shape[1]
    X, G = np.fft.rfft(x, axis=1, norm="ortho"), np.fft.rfft(dy, axis=1, norm="ortho")
    g = weights(N)[:, None] * (np.conj(X) * G).sum(0)
    out = np.stack([g.real, g.imag], axis=-1)
    out[inert(N), :, 1] = 0.0
    return out


def circulant(x, w):
    """y[n, d] = sum_m c[(n - m) mod N, d] x[m, d], c = irfft(W_eff, n=N, axis=0) (backward norm)"""
    x = np.asarray(x, np.float64)
    N = x.shape[1]
    c = np.fft.irfft(w_eff(w, N), n=N, axis=0)
    idx = (np.arange(N)[:, None] - np.arange(N)[None, :]) % N
    return np.einsum("nmd,bmd->bnd", c[idx], x)


# ------------------------------------------------------------------------------------------------------------------ the kernels' arithmetic
def table32(tokens):
    """spv_gfilter_make_tables: (cos, sin)(2 pi j / N) from float64, stored as float32"""
    a = 2.0 * np.pi * np.arange(tokens) / tokens
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)


def _dft32(tokens):
    cos, sin = table32(tokens)
    m = (np.arange(bins(tokens))[:, None] * np.arange(tokens)[None, :]) % tokens
    return cos[m], sin[m]   # (K, N)


def _weights32(w, tokens):
    w = np.asarray(w, np.float32)
    wr, wi = w[..., 0], w[..., 1].copy()
    wi[inert(tokens)] = 0.0
    ck = (weights(tokens).astype(np.float32) * np.float32(1.0 / tokens))[:, None]
    return wr, wi, ck


def _token32(zr, zi, fc, fs):
    return np.einsum("kn,bkd->bnd", fc, zr) - np.einsum("kn,bkd->bnd", fs, zi)


def generic_fwd32(x, w):
    """gfilter_fwd_kernel in float32: X = c - i s from the fp32 table, Z = c_k / N * X W_eff, y = sum_k Zr cos - Zi sin.  x has been
    rounded to its storage dtype by the caller; the store's rounding of y is the bar's 2^-8 and is not restated."""
    x = np.asarray(x, np.float32)
    N = x.shape[1]
    fc, fs = _dft32(N)
    c, s = np.einsum("kn,bnd->bkd", fc, x), np.einsum("kn,bnd->bkd", fs, x)
    wr, wi, ck = _weights32(w, N)
    zr, zi = ck * (c * wr + s * wi), ck * (c * wi - s * wr)
    y = _token32(zr, zi, fc, fs)
    assert y.dtype == np.float32
    return y


def generic_bwd32(x, dy, w):
    """gfilter_bwd_kernel in float32: (dx, dW)"""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    N = x.shape[1]
    fc, fs = _dft32(N)
    cx, sx = np.einsum("kn,bnd->bkd", fc, x), np.einsum("kn,bnd->bkd", fs, x)
    cg, sg = np.einsum("kn,bnd->bkd", fc, dy), np.einsum("kn,bnd->bkd", fs, dy)
    wr, wi, ck = _weights32(w, N)
    zr, zi = ck * (cg * wr - sg * wi), -ck * (sg * wr + cg * wi)
    gw = np.stack([(ck * (cx * cg + sx * sg)).sum(0, dtype=np.float32), (ck * (sx * cg - cx * sg)).sum(0, dtype=np.float32)], axis=-1)
    gw[inert(N), :, 1] = 0.0
    out = _token32(zr, zi, fc, fs)
    assert out.dtype == gw.dtype == np.float32
    return out, gw


def _bf16(a):
    return C.storage_round(np.asarray(a, np.float64), "bf16").astype(np.float32)


def _split(a):
    """a float32 value as hi + lo bf16 (both returned as float32)"""
    a = np.asarray(a, np.float32)
    hi = _bf16(a)
    return hi, _bf16(a - hi)


def fast_tables(tokens):
    """spv_gfilter_make_tables' fast part: T1 [hi, lo][cos, sin][KP][NP] and T2 [hi, lo][cos, sin][NPO][KP], zero outside K x N; each entry
    float64's cos / sin rounded to float32, then split into hi + lo bf16"""
    NP, NPO, KP = fast_pads(tokens)
    K = bins(tokens)
    cos, sin = table32(tokens)
    m = (np.arange(K)[:, None] * np.arange(tokens)[None, :]) % tokens
    t1 = np.zeros((2, 2, KP, NP), np.float32)
    t2 = np.zeros((2, 2, NPO, KP), np.float32)
    for part, f in enumerate((cos[m], sin[m])):
        hi, lo = _split(f)
        t1[0, part, :K, :tokens], t1[1, part, :K, :tokens] = hi, lo
        t2[0, part, :tokens, :K], t2[1, part, :tokens, :K] = hi.T, lo.T
    return t1, t2


def _fast_bins(t1, v, K, N):
    """step 1: products of bf16 values, summed in float32 (hi and lo terms into the same accumulator)"""
    c = np.einsum("kn,bnd->bkd", t1[0, 0, :K, :N], v) + np.einsum("kn,bnd->bkd", t1[1, 0, :K, :N], v)
    s = np.einsum("kn,bnd->bkd", t1[0, 1, :K, :N], v) + np.einsum("kn,bnd->bkd", t1[1, 1, :K, :N], v)
    return c.astype(np.float32), s.astype(np.float32)


def _fast_tokens(t2, zr, zi, K, N):
    """step 3: Zr and -Zi split into hi + lo bf16; hi.hi + lo.hi + hi.lo per term"""
    (rh, rl), (ih, il) = _split(zr), _split(-zi)
    gc, gs = t2[:, 0, :N, :K], t2[:, 1, :N, :K]
    e = lambda g, z: np.einsum("nk,bkd->bnd", g, z)   # noqa: E731
    y = e(gc[0], rh) + e(gs[0], ih) + e(gc[1], rh) + e(gs[1], ih) + e(gc[0], rl) + e(gs[0], il)
    assert y.dtype == np.float32
    return y


def fast_fwd32(x, w):
    """gfilter_fast_kernel<0>: every rounding before the store of y (which is the bar's 2^-8 and is not restated)"""
    x = np.asarray(x, np.float32)   # bf16 values
    N, K = x.shape[1], bins(x.shape[1])
    t1, t2 = fast_tables(N)
    c, s = _fast_bins(t1, x, K, N)
    wr, wi, ck = _weights32(w, N)
    return _fast_tokens(t2, ck * (c * wr + s * wi), ck * (c * wi - s * wr), K, N)


def fast_bwd32(x, dy, w):
    """gfilter_fast_kernel<1>: (dx before its store, dW)"""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    N, K = x.shape[1], bins(x.shape[1])
    t1, t2 = fast_tables(N)
    (cx, sx), (cg, sg) = _fast_bins(t1, x, K, N), _fast_bins(t1, dy, K, N)
    wr, wi, ck = _weights32(w, N)
    gw = np.stack([(ck * (cx * cg + sx * sg)).sum(0, dtype=np.float32), (ck * (sx * cg - cx * sg)).sum(0, dtype=np.float32)], axis=-1)
    gw[inert(N), :, 1] = 0.0
    return _fast_tokens(t2, ck * (cg * wr - sg * wi), -ck * (sg * wr + cg * wi), K, N), gw


# ------------------------------------------------------------------------------------------------------------------ dispatch
# codes of spv_gfilter_path (include/spv.h)
FAST, GENERIC = 1, 2
REFUSE_EMPTY, REFUSE_DTYPE, REFUSE_TOKENS, REFUSE_ALIGN = -1, -2, -3, -4
FAST_MAX_TOKENS, FAST_COLS = 80, 64
LDS_FLOATS, MAX_COLS, MAX_SLABS = 16384, 64, 32
MAX_TOKENS = (LDS_FLOATS - 4) // 6

Plan = namedtuple("Plan", "path bins cols_fwd cols_bwd", defaults=(0, 0, 0))


def select(dtype, tokens, dim, aligned=True):
    """gfilter_select of csrc/spv_gfilter_core.h; dtype: "fp32" / "bf16" or a raw code.  aligned: x, y (dy, dx) and the tables sit on
    16 bytes; it matters inside the fast window only."""
    code = CODE.get(dtype, dtype)
    if tokens < 1 or dim < 1:
        return Plan(REFUSE_EMPTY)
    if code not in (0, 1):
        return Plan(REFUSE_DTYPE)
    if tokens > MAX_TOKENS:
        return Plan(REFUSE_TOKENS)
    k = bins(tokens)
    if fast_window(code, tokens, dim):
        return Plan(FAST if aligned else REFUSE_ALIGN, k, FAST_COLS, FAST_COLS)
    room = LDS_FLOATS - 2 * tokens   # the table sits in LDS beside the columns
    return Plan(GENERIC, k, min(room // (tokens + 2 * k), MAX_COLS, dim), min(room // (2 * tokens + 4 * k), MAX_COLS, dim))


def fast_window(code, tokens, dim):
    return code == 1 and 1 <= tokens <= FAST_MAX_TOKENS and dim >= 1 and dim % FAST_COLS == 0


def fast_pads(tokens):
    """(NP, NPO, KP): tokens as a K axis (steps of 16) and as output rows (tiles of 32), bins as rows and as a K axis"""
    return (tokens + 15) // 16 * 16, (tokens + 31) // 32 * 32, 32 if bins(tokens) <= 32 else 64


def generic_table_floats(tokens):
    return (2 * tokens + 3) // 4 * 4


def path(dtype, tokens, dim, aligned=True):
    return select(dtype, tokens, dim, aligned).path


def table_floats(tokens):
    if tokens < 1:
        return 0
    if tokens > FAST_MAX_TOKENS:
        return 2 * tokens
    NP, NPO, KP = fast_pads(tokens)
    return generic_table_floats(tokens) + (4 * KP * NP + 4 * NPO * KP) // 2


def workspace_floats(batch, tokens, dim):
    return 0


def slabs(batch):
    return min(batch, MAX_SLABS) if batch >= 1 else 0


def partial_floats(batch, tokens, dim):
    return slabs(batch) * bins(tokens) * dim * 2 if min(batch, tokens, dim) >= 1 else 0


# ------------------------------------------------------------------------------------------------------------------ tables
# off: bytes x, dy, y and dx sit off 16-byte alignment
Case = namedtuple("Case", "dtype batch tokens dim off", defaults=(0,))

# 1: DC only; 2: DC + Nyquist, no doubled bin; 63 / 64: the backward's column block drops below 64 columns (the table's 2 N floats and
# 2 N + 4 K floats per column inside 16384); 125 / 126: the forward's does; 197: both well below (40 and 20 columns)
# fast path (bf16, dim 64 / 512): 16 / 17, 32 / 33, 48 / 49, 64 / 65: its K steps of 16 tokens; 32 / 33, 64 / 65: its output tiles of 32
# tokens; 63 / 64: 32 / 33 bins, one bin tile or two; 80 / 81: the end of its window
TOKENS = (1, 2, 3, 4, 5, 16, 17, 32, 33, 48, 49, 63, 64, 65, 80, 81, 125, 126, 197)
DIMS = (8, 24, 64, 72, 512)   # 72: one whole block of 64 columns and a part of one
CASES = (
    [Case(dt, b, t, d) for t in TOKENS for d in DIMS for b in (1, 3) for dt in DTYPES]
    # more samples than slabs: workgroups own 3 and 2 samples each, and the fold sums 32 slabs
    + [Case(dt, 70, t, d) for t, d in ((5, 24), (65, 64)) for dt in DTYPES]
    # any alignment of the element type
    + [Case(dt, 3, 7, 12, 8) for dt in DTYPES]
    # the largest token count the selector accepts: 2 columns per workgroup forward, 1 backward, exactly LDS_FLOATS each
    + [Case(dt, 2, MAX_TOKENS, 3) for dt in DTYPES]
)
assert len(set(CASES)) == len(CASES)
MISALIGNED_REFUSED = [Case("bf16", 3, 7, 64, 8), Case("bf16", 1, 65, 512, 8)]   # fast shapes, x / dy / y / dx off 16-byte alignment
# (dtype, tokens, dim) -> refusal
REFUSALS = {("fp32", 0, 8): REFUSE_EMPTY, ("bf16", 8, 0): REFUSE_EMPTY, (2, 8, 8): REFUSE_DTYPE, ("fp32", MAX_TOKENS + 1, 8): REFUSE_TOKENS}


def normal(rng, shape, dtype):
    return C.normal(rng, shape, dtype)


def inputs(c):
    """(x, dy, filter) of a case: x and dy in the storage dtype; the filter a float32 randn (not 0.02 randn: the bars should mean
    something) with non-zero imaginary parts planted at the DC and Nyquist bins"""
    rng = rng_of(c)
    shape = (c.batch, c.tokens, c.dim)
    x, dy = normal(rng, shape, c.dtype), normal(rng, shape, c.dtype)
    w = rng.standard_normal((bins(c.tokens), c.dim, 2))
    w[inert(c.tokens), :, 1] = np.where(np.arange(c.dim) % 2 == 0, 1.5, -2.5)
    w = C.storage_round(w, "fp32")
    w.setflags(write=False)
    return x, dy, w
