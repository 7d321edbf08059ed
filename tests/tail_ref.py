"""Float64 reference of the SpectreLinear tail (csrc/spv_rowops.hip, include/spv.h) and of the tail followed by LayerNorm-2, forward and
backward, written from the definitions and independent of spectre_vit:

    out = mask * (GELU_erf(LayerNorm(h)) + adaptive_avg_pool(x)),      mask = keep / (1 - p)
    dout_eff = dout [+ P_up^T (mask_up * up_src)]                      (spv.h: spv_spectre_tail_bwd_up)
    dh = LayerNorm-backward(mask * dout_eff * GELU'(ln)),  dx_pool = P^T (mask * dout_eff) [+ dx_add]
    dgamma, dbeta = the LayerNorm's column sums,  dbias = sum over rows of dh

The mask is an argument (tests/dropout_ref.py's keep(seed, rows, n, p) predicts the device's), so a test can also hand in a wrong one.

mode "exact": float64 throughout.  The other two give the rounding floor of a kernel that is right:
mode "fp32": every array and every operation in numpy float32;
mode "bf16": float64, with the STORED tensors (out, out2, ds, dh, dx_pool) rounded to bf16 and nothing else -- statistics and column
             sums leave the kernels as fp32."""
import numpy as np

import dropout_ref as D
from oracle import spectre_oracle as O

ELEMENTWISE = ("out", "out2", "ds", "dh", "dx_pool")
ROW_STATS = ("mean", "rstd", "mean2", "rstd2")
COLUMN_SUMS = ("dgamma", "dbeta", "dbias", "dgamma2", "dbeta2")


def _types(mode):
    assert mode in ("exact", "fp32", "bf16"), mode
    ft = np.float32 if mode == "fp32" else np.float64
    return ft, (D.bf16_round if mode == "bf16" else (lambda a: a))


def _mask(keep, p, ft):
    """keep / (1 - p) with the device's float32 constant; None: no dropout"""
    return ft(1.0) if keep is None else keep.astype(ft) * ft(D.inv_keep(p))


def _stats(h, ft):
    mean = h.mean(axis=-1)
    var = ((h - mean[:, None]) ** 2).mean(axis=-1)
    return mean, ft(1.0) / np.sqrt(var + ft(1e-5))


def tail(h, x, gamma, beta, dout, keep, p, dx_add=None, up=None, mode="exact", P=None, out_fp32=False):
    """h, dout [rows, n]; x, dx_add [rows, k_in]; keep bool [rows, n] or None (p == 0); up = (up_src [rows, n_up], keep_up, p_up): the
    incoming gradient of the layer above (n inputs, n_up outputs) before its mask.  P: another pooling matrix [n, k_in] than
    AdaptiveAvgPool1d's (for sensitivity tests).  out_fp32: `out` is stored as float32 by a bf16 kernel, so mode "bf16" leaves it.
    Returns dict(out, mean, rstd, dh, dx_pool, dgamma, dbeta, dbias)."""
    ft, rnd = _types(mode)
    h, x, gamma, beta, dout = (np.asarray(a, dtype=ft) for a in (h, x, gamma, beta, dout))
    n, k_in = h.shape[1], x.shape[1]
    P = O.adaptive_pool_matrix(k_in, n, ft) if P is None else np.asarray(P, dtype=ft)
    m = _mask(keep, p, ft)
    ln, cache = O.layernorm_fwd(h, gamma, beta)
    mean, rstd = _stats(h, ft)
    out = (O.gelu(ln) + x @ P.T) * m
    d = dout
    if up is not None:
        up_src, keep_up, p_up = up
        up_src = np.asarray(up_src, dtype=ft)
        d = d + (up_src * _mask(keep_up, p_up, ft)) @ O.adaptive_pool_matrix(n, up_src.shape[1], ft)
    dm = d * m
    dh, dgamma, dbeta = O.layernorm_bwd(dm * O.gelu_grad(ln), gamma, cache)
    dx_pool = dm @ P
    if dx_add is not None:
        dx_pool = dx_pool + np.asarray(dx_add, dtype=ft)
    res = dict(out=out if out_fp32 else rnd(out), mean=mean, rstd=rstd, dh=rnd(dh), dx_pool=rnd(dx_pool), dgamma=dgamma, dbeta=dbeta,
               dbias=dh.sum(axis=0))
    assert all(a.dtype == ft for a in res.values()), {k: a.dtype for k, a in res.items()}
    return res


def tail_ln2(h, x, gamma, beta, x1, gamma2, beta2, dout2, keep, p, f3=None, ds=None, mode="exact", P=None):
    """The tail followed by x2 = LayerNorm2(x1 + f3); backward: ds = LayerNorm2-backward(dout2), then the tail's backward of ds.
    The kernels re-read two tensors they stored: f3 (forward, into LayerNorm-2) and ds (backward, into the tail).  f3 / ds given: the
    downstream part is computed from THOSE values (the kernel's own), so every returned tensor is one rounding away from float64;
    None: from this function's own (rounded as stored in mode "bf16").
    Returns tail()'s dict (out = f3) + out2, mean2, rstd2, ds, dgamma2, dbeta2."""
    ft, rnd = _types(mode)
    x1, gamma2, beta2, dout2 = (np.asarray(a, dtype=ft) for a in (x1, gamma2, beta2, dout2))
    fwd = tail(h, x, gamma, beta, np.zeros_like(dout2), keep, p, mode=mode, P=P)
    s = x1 + (fwd["out"] if f3 is None else np.asarray(f3, dtype=ft))
    out2, cache2 = O.layernorm_fwd(s, gamma2, beta2)
    mean2, rstd2 = _stats(s, ft)
    ds_own, dgamma2, dbeta2 = O.layernorm_bwd(dout2, gamma2, cache2)
    res = tail(h, x, gamma, beta, rnd(ds_own) if ds is None else np.asarray(ds, dtype=ft), keep, p, mode=mode, P=P)
    res.update(out2=rnd(out2), mean2=mean2, rstd2=rstd2, ds=rnd(ds_own), dgamma2=dgamma2, dbeta2=dbeta2)
    assert all(a.dtype == ft for a in res.values())
    return res


def row_errors(got, ref):
    """max |got - ref| / max |ref| over each row of [rows, n] arrays -> float64 [rows].  A row whose reference is zero throughout must
    be zero in `got` as well: error 0, otherwise inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and ref.ndim == 2, (got.shape, ref.shape)
    d, r = np.abs(got - ref).max(-1), np.abs(ref).max(-1)
    d = np.where(np.isnan(d), np.inf, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r > 0, d / r, np.where(d == 0, 0.0, np.inf))


def col_error(got, ref):
    """max |got - ref| / max |ref| over a vector (row statistics, column sums) -> float"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(row_errors(got[None], ref[None])[0])
