"""Float64 references of the spectral kernels (csrc/spv_fft.hip, spv_hadamard.hip, the haar_ln pair of spv_rowops.hip) for
tests/test_gpu_spectral_edges.py: thin wrappers over oracle/spectre_oracle.py plus the row-0 node and the fused LayerNorm compositions.
Re(fft2) and rfft(x).real are taken with numpy's float64 FFT (the oracle's explicit cos / sin products need D x D matrices, 268 MB at
D = 4096); tests/test_spectral_ref.py pins them to the oracle's matrix products at 1e-12.

Where a kernel is documented to round an intermediate tensor to bf16 (include/spv.h: spv_fnet_ln_bwd's LayerNorm backward feeding the
transform, spv_haar_ln_*'s band tensor), the reference rounds the same tensor, or is computed downstream of the kernel's own stored
tensor, so that every compared output is one rounding away from float64."""
import numpy as np

import dropout_ref as D
from oracle import spectre_oracle as O

SQRT_HALF32 = np.float32(0.70710678118654752440)
EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------ transforms
def fnet_mix(x, add_in=None):
    """Re(fft2(x)) over the last two axes (+ add_in) == oracle fnet_mix_fwd"""
    y = np.fft.fft2(np.asarray(x, np.float64), axes=(-2, -1)).real
    return y if add_in is None else y + add_in


def rfft_real(x, dim, transpose):
    """transpose 0: rfft(x).real [rows, D] -> [rows, D/2+1] == oracle fft_module_fwd; 1: its adjoint == fft_module_bwd"""
    x = np.asarray(x, np.float64)
    return np.fft.fft(x, n=dim, axis=-1).real if transpose else np.fft.rfft(x, axis=-1).real


def haar(x, axis, levels, inverse):
    """spv_haar_dwt's `inverse` argument: bit 0 the adjoint, bit 1 pywt's 'zero' extension; axis 1 tokens, 2 dim of [B, N, D]"""
    mode = "zero" if inverse & 2 else "passthrough"
    fn = O.haar_dwt_bwd if inverse & 1 else O.haar_dwt_fwd
    return fn(np.asarray(x, np.float64), axis=axis - 3, levels=levels, mode=mode)


def fwht(x, n, n_out, mode, repeat, scale, residual=None):
    """spv_fwht: rows of n_in values zero-padded to n, `repeat` passes of mode 0 (natural order) / 1 (fwht_fast) / 2 (its transpose),
    times scale, the first n_out kept, + residual"""
    x = np.asarray(x, np.float64)
    y = np.concatenate([x, np.zeros((x.shape[0], n - x.shape[1]))], axis=1)
    step = {0: lambda a: O.fwht(a, normalize=False), 1: O.fwht_fast_fwd, 2: O.fwht_fast_bwd}[mode]
    for _ in range(repeat):
        y = step(y)
    y = y[:, :n_out] * float(scale)
    return y if residual is None else y + residual


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def stats(a):
    mean = a.mean(-1)
    return mean, 1.0 / np.sqrt(((a - mean[..., None]) ** 2).mean(-1) + EPS)


def ln_fwd(a, gamma, beta):
    """(out, mean, rstd) of oracle layernorm_fwd over the last axis"""
    out, _ = O.layernorm_fwd(a, gamma, beta, EPS)
    return (out,) + stats(a)


def ln_bwd(dy, a, gamma):
    """d(LayerNorm input), and the per-element dgamma / dbeta contributions (dy * xhat, dy)"""
    _, cache = O.layernorm_fwd(a, gamma, np.zeros_like(gamma), EPS)
    da, _, _ = O.layernorm_bwd(dy, gamma, cache)
    return da, dy * cache[0], dy


# ------------------------------------------------------------------------------------------------------------------ fused nodes
def fnet_ln_fwd(x, gamma, beta, prenorm=None):
    """x1 = LN(Re fft2(x)) gamma + beta + x.  prenorm given: the kernel's own stored tensor, everything after it is computed from it."""
    pre = fnet_mix(x)
    own = pre if prenorm is None else np.asarray(prenorm, np.float64)
    ln, mean, rstd = ln_fwd(own, gamma, beta)
    return dict(prenorm=pre, mean=mean, rstd=rstd, out=ln + x)


def fnet_ln_bwd(dout, prenorm, gamma):
    """dx = Re fft2(bf16(LN-backward(dout))) + dout; dgamma / dbeta: column sums over batch and tokens; partials [batch][2][D]"""
    dm, dg, db = ln_bwd(dout, np.asarray(prenorm, np.float64), gamma)
    parts = np.stack([dg.sum(1), db.sum(1)], axis=1)
    return dict(dx=fnet_mix(D.bf16_round(dm)) + dout, dgamma=parts[:, 0].sum(0), dbeta=parts[:, 1].sum(0), partials=parts)


def cls_fwd(x, gamma, beta, m0=None, lose_group=None):
    """row 0 of the same node: m0 = Re(FFT_D(sum_n x[n])), out = LN(m0) gamma + beta + x[:, 0].  lose_group = (g, RG): the tokens
    n = g mod RG are left out of the sum (sensitivity tests)."""
    x = np.asarray(x, np.float64)
    keep = np.ones(x.shape[1], bool)
    if lose_group is not None:
        keep[lose_group[0]::lose_group[1]] = False
    pre = np.fft.fft(x[:, keep].sum(1), axis=-1).real
    own = pre if m0 is None else np.asarray(m0, np.float64)
    ln, mean, rstd = ln_fwd(own, gamma, beta)
    return dict(m0=pre, mean=mean, rstd=rstd, out=ln + x[:, 0])


def cls_bwd(g1, m0, gamma, tokens):
    """dx[b, n] = Re(FFT_D(LN-backward(g1[b]))) for every n, + g1 in row 0; partials [batch][2][D] = g1 xhat, g1"""
    dm, dg, db = ln_bwd(g1, np.asarray(m0, np.float64), gamma)
    dx = np.repeat(np.fft.fft(dm, axis=-1).real[:, None, :], tokens, axis=1)
    dx[:, 0] += g1
    return dict(dx=dx, partials=np.stack([dg, db], axis=1))


def haar_band_bf16(x):
    """the band tensor [a | d] of one Haar level along the last axis as spv_haar_ln_* form it: float32 (x0 + x1) * fl(1/sqrt2), rounded
    to bf16 (the tensor the unfused path stores between spv_haar_dwt and the LayerNorm kernel)"""
    x = np.asarray(x, np.float32)
    e, o = x[..., 0::2], x[..., 1::2]
    band = np.concatenate([(e + o) * SQRT_HALF32, (e - o) * SQRT_HALF32], axis=-1)
    return D.bf16_round(band.astype(np.float64))


def haar_ln_fwd(x, gamma, beta):
    ln, mean, rstd = ln_fwd(haar_band_bf16(x), gamma, beta)
    return dict(mean=mean, rstd=rstd, out=ln + x)


def haar_ln_bwd(dout, x, gamma):
    """dx = haar^T(bf16(LN-backward(dout))) + dout"""
    dm, dg, db = ln_bwd(dout, haar_band_bf16(x), gamma)
    dx = O.haar_dwt_bwd(D.bf16_round(dm), axis=-1, levels=1) + dout
    return dict(dx=dx, dgamma=dg.sum(0), dbeta=db.sum(0))


# ------------------------------------------------------------------------------------------------------------------ errors
def block_errors(got, ref, keep_axes):
    """max |got - ref| / max |ref| over each block -> float64 [blocks]; a block is what remains after the first `keep_axes` axes
    (keep_axes = 1: per sample; ndim - 1: per row).  An all-zero reference block must be all zero in `got` (error 0, else inf);
    NaN counts as inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nb = int(np.prod(ref.shape[:keep_axes], dtype=np.int64))
    g, r = got.reshape(nb, -1), ref.reshape(nb, -1)
    d, m = np.abs(g - r).max(-1), np.abs(r).max(-1)
    d = np.where(np.isnan(d), np.inf, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m > 0, d / m, np.where(d == 0, 0.0, np.inf))


def err(got, ref, keep_axes=0):
    """the worst block"""
    return float(block_errors(got, ref, keep_axes).max())
