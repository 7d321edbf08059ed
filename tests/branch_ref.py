"""Float64 references of the SpectreBranch kernels (csrc/spv_branch.hip) and, next to each, a float32 restatement that follows the
kernel's order of operations.  Pure numpy; tests/test_branch_ref.py holds the references to torch's float64 CPU operators.

Layouts, as the source's comments state them (m = (b, ho, wo) over the OUTPUT map unless said otherwise, k = (c, ky, kx)):

    cols [m][k]   = x[b, ho + ky, wo + kx, c]         k < 9 Cin, zero for k in [9 Cin, ld)
    colsT[k][m]   = the same, k < 9 Cin, m < Mp       zero for m in [M, Mp)
    dcols[m][k]   = dy[b, h - ky, w - kx, co]         m = (b, h, w) over the INPUT map, k = (co, ky, kx), zero off the output map
    dyT  [co][m]  = dy[m][co]                         zero for m in [M, Mp)

A restatement takes `mutant`: a plausible mistake, which the judge of the GPU test must catch (tests/test_branch_ref.py)."""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ spectrum
def _twiddles(n):
    """(cos, sin)(2 pi k / n), k < n, in float64, exact at the quarter turns as sincospi is"""
    k = np.arange(n)
    co, s = np.cos(2 * np.pi * k / n), np.sin(2 * np.pi * k / n)
    q = 4 * k
    for turn, (c1, s1) in enumerate(((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))):
        at = q == turn * n
        co[at], s[at] = c1, s1
    return co, s


def spectrum_ref(img):
    """img (B, C, H, W) -> dict(out = log1p(|rfft2|) as (B, H, Wf, C), X = |rfft2| in that layout, S = the plane's sum of |x|
    broadcast to it); a plane holding a non-finite value is NaN throughout"""
    img = np.asarray(img, np.float64)
    fin = np.isfinite(img).all(axis=(2, 3))
    X = np.abs(np.fft.rfft2(np.where(fin[:, :, None, None], img, 0.0), axes=(2, 3)))
    X = np.where(fin[:, :, None, None], X, np.nan).transpose(0, 2, 3, 1)
    with np.errstate(invalid="ignore"):
        S = np.broadcast_to(np.abs(img).sum(axis=(2, 3))[:, None, None, :], X.shape)
    return dict(out=np.log1p(X), X=X, S=S)


def spectrum_restate(img, mutant=None):
    """spectrum_kernel in float32: double-precision twiddles rounded to fp32 and indexed by the stepped integer phase, the row DFT, the
    column DFT, hypot, log1p.  Returns (B, H, Wf, C) float32"""
    img = np.asarray(img, F32)
    B, C, H, W = img.shape
    Wf = W // 2 + 1
    wf = W // 2 if mutant == "nyquist_dropped" and W >= 2 else Wf
    cw, sw = (t.astype(F32) for t in _twiddles(W))
    ch, sh = (t.astype(F32) for t in _twiddles(H))
    if mutant == "w_table_for_columns":
        k = np.arange(H)
        ch, sh = np.cos(2 * np.pi * k / W).astype(F32), np.sin(2 * np.pi * k / W).astype(F32)
    x = img.reshape(B * C, H, W)
    v, u = np.arange(wf), np.arange(H)
    re, im = np.zeros((B * C, H, wf), F32), np.zeros((B * C, H, wf), F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for w in range(W):
            ph = (v * w) % W
            a = x[:, :, w, None]
            re = re + a * cw[ph]
            im = im - a * sw[ph]
        ore, oim = np.zeros((B * C, H, wf), F32), np.zeros((B * C, H, wf), F32)
        for h in range(H):
            ph = (u * h) % H
            a, b = re[:, h, None, :], im[:, h, None, :]
            co, s = ch[ph][None, :, None], sh[ph][None, :, None]
            ore = ore + (a * co + b * s)
            oim = oim + (b * co - a * s)
        mag = np.hypot(ore, oim)
        val = (np.log(mag) if mutant == "log" else np.log1p(mag)).astype(F32)
    flat = np.full((B, H * Wf, C), np.nan, F32)        # a kernel with fewer bins per row packs them and leaves the rest unwritten
    flat[:, :H * wf, :] = val.reshape(B, C, H * wf).transpose(0, 2, 1)
    return flat.reshape(B, H, Wf, C)


# ------------------------------------------------------------------------------------------------------------------ gathers
def _k_split(k, order):
    """(c, ky, kx) of column index k < 9 C: "cyx" is the kernel's, "yxc" and "cxy" are mistakes"""
    C9 = k.max() + 1 if k.size else 0
    if order == "yxc":
        C = C9 // 9
        return k % C, k // C // 3, k // C % 3
    c, r = k // 9, k % 9
    return (c, r % 3, r // 3) if order == "cxy" else (c, r // 3, r % 3)


def im2col(x, ld, order="cyx", pad=0.0):
    """x (B, H, W, Cin) -> cols [M][ld] in x's dtype, columns 9 Cin .. ld - 1 holding `pad`"""
    B, H, W, Cin = x.shape
    Ho, Wo, K = H - 2, W - 2, 9 * Cin
    b, ho, wo = np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), indexing="ij")
    base = (((b * H + ho) * W + wo) * Cin).reshape(-1).astype(np.int32)
    c, ky, kx = _k_split(np.arange(K), order)
    off = ((ky * W + kx) * Cin + c).astype(np.int32)
    cols = np.full((base.size, ld), pad, x.dtype)
    cols[:, :K] = x.reshape(-1)[base[:, None] + off[None, :]]
    return cols


def transposed(a, ldm, mutant=None):
    """a [M][K] -> [K][ldm], zero for m in [M, ldm); mutant "ld_M": rows laid M apart in the same buffer, the rest never written"""
    M, K = a.shape
    out = np.zeros((K, ldm), a.dtype)
    out[:, :M] = a.T
    if mutant == "ld_M":
        flat = np.full(K * ldm, np.nan, a.dtype)
        flat[:K * M] = a.T.reshape(-1)
        out = flat.reshape(K, ldm)
    return out


def dcols(dy, ld, mutant=None, pad=0.0):
    """dy (B, Ho, Wo, Cout) -> dcols [B H W][ld] over the input map"""
    B, Ho, Wo, Cout = dy.shape
    H, W, K = Ho + 2, Wo + 2, 9 * Cout
    b, h, w = (v.reshape(-1, 1).astype(np.int32) for v in np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij"))
    co, ky, kx = (v[None, :].astype(np.int32) for v in _k_split(np.arange(K), "cyx"))
    ho, wo = (h + ky, w + kx) if mutant == "dgrad_sign" else (h - ky, w - kx)
    ok = (ho >= 0) & (ho < Ho) & (wo >= 0) & (wo < Wo)
    hc, wc = np.clip(ho, 0, Ho - 1), np.clip(wo, 0, Wo - 1)
    val = dy.reshape(-1)[((b * Ho + hc) * Wo + wc) * Cout + co]
    out = np.full((B * H * W, ld), pad, dy.dtype)
    out[:, :K] = val if mutant == "dgrad_clamp" else np.where(ok, val, np.zeros((), dy.dtype))
    return out


def wd_of(w):
    """w (Cout, Cin, 3, 3) -> wd [Cin][9 Cout], wd[c][(co, ky, kx)] = w[co][c][ky][kx]"""
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)).reshape(w.shape[1], -1)


# ------------------------------------------------------------------------------------------------------------------ convolution
def _product(a, b):
    """(a b^T, |a| |b|^T) in float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a @ b.T, np.abs(a) @ np.abs(b).T


def conv_fwd(x, w, bias):
    """(y [M][Cout], S): the gather followed by the matrix product, plus the bias"""
    v, S = _product(im2col(x, 9 * x.shape[3]), w.reshape(w.shape[0], -1))
    return v + bias, S + np.abs(bias)


def conv_dgrad(dy, w):
    """(dx [B H W][Cin], S)"""
    return _product(dcols(dy, 9 * dy.shape[3]), wd_of(w))


def conv_wgrad(dy, x):
    """(dw [Cout][9 Cin], S)"""
    return _product(dy.reshape(-1, dy.shape[3]).T, im2col(x, 9 * x.shape[3]).T)


def matmul32(a, b, bias=None):
    """a b^T (+ bias) in float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(a, F32) @ np.asarray(b, F32).T
        return v + np.asarray(bias, F32) if bias is not None else v


# ------------------------------------------------------------------------------------------------------------------ pooling
def windows(L, T, mutant=None):
    """(start, end) of AdaptiveAvgPool1d's T windows over L: [floor(t L / T), ceil((t + 1) L / T))"""
    t = np.arange(T)
    s = t * L // T
    e = (t + 1) * L // T if mutant == "end_floor" else -(-(t + 1) * L // T)
    return s, np.maximum(e, s + 1) if mutant == "end_floor" else e


def pool_matrix(L, T):
    P = np.zeros((T, L))
    for t, (s, e) in enumerate(zip(*windows(L, T))):
        P[t, s:e] = 1.0 / (e - s)
    return P


def pool_fwd(y, T, ldo):
    """y (B, L, C) -> dict(out (B, T, ldo) with zero pad columns, S = the window's mean |y|, n = its length, both in out's shape)"""
    y = np.asarray(y, np.float64)
    B, L, C = y.shape
    P = pool_matrix(L, T)
    out, S, n = np.zeros((B, T, ldo)), np.zeros((B, T, ldo)), np.zeros((B, T, ldo))
    out[..., :C] = np.einsum("tl,blc->btc", P, y)
    S[..., :C] = np.einsum("tl,blc->btc", P, np.abs(y))
    s, e = windows(L, T)
    n[..., :C] = (e - s)[None, :, None]
    return dict(out=out, S=S, n=n)


def pool_bwd(dout, L, C, add=None):
    """dout (B, T, ldo) -> dict(dy (B, L, C), S = the sum of the absolute values of its terms, n = two per contributing window + one
    for `add`); columns C .. ldo - 1 of dout are never read"""
    d = np.asarray(dout, np.float64)[..., :C]
    P = pool_matrix(L, d.shape[1])
    dy, S = np.einsum("tl,btc->blc", P, d), np.einsum("tl,btc->blc", P, np.abs(d))
    n = 2.0 * (P > 0).sum(0)[None, :, None] * np.ones_like(dy)
    if add is not None:
        dy, S, n = dy + add, S + np.abs(add), n + 1
    return dict(dy=dy, S=S, n=n)


def pool_fwd_restate(y, T, ldo, mutant=None):
    y = np.asarray(y, F32)
    B, L, C = y.shape
    out = np.zeros((B, T, ldo), F32)
    if mutant == "pads_unwritten":
        out[..., C:] = np.nan
    for t, (s, e) in enumerate(zip(*windows(L, T, mutant))):
        v = np.zeros((B, C), F32)
        for l in range(s, e):
            v = v + y[:, l]
        out[:, t, :C] = v / F32(e - s)
    return out


def pool_bwd_restate(dout, L, C, add=None, mutant=None):
    d = np.asarray(dout, F32)[..., :C]
    B, T = d.shape[:2]
    dy = np.zeros((B, L, C), F32)
    s, e = windows(L, T)
    seen = np.zeros(L, bool)
    for t in range(T):
        n = e[t] - s[t]
        if mutant == "bwd_wrong_len":
            n = e[min(t + 1, T - 1)] - s[min(t + 1, T - 1)] if T > 1 else n + 1
        rows = np.arange(s[t], e[t])
        if mutant == "bwd_one_window":
            rows = rows[~seen[rows]]
        seen[s[t]:e[t]] = True
        dy[:, rows] = dy[:, rows] + (d[:, t] / F32(n))[:, None, :]
    return dy + np.asarray(add, F32) if add is not None else dy
