"""Float64 references and float32 / bf16-storage restatements of the patch-embedding kernels of csrc/spv_patch.hip and
csrc/spv_prologue_core.h (spv_patchify, spv_patchify_u8, spv_embed_posbias, spv_embed_cls_rows, spv_spectral_fold[_bf16],
spv_spectral_fold_bwd, spv_embed_bwd, spv_dropout), written from include/spv.h's definitions.  Pure numpy: a reference states the
operation on whole arrays in float64 (the spectral basis from numpy.fft.rfft2 of impulses, not from the kernel's cosine formula); a
restatement walks the flat indices, unrolls and summation order of the kernel in float32, and takes a `mutant` that plants one
plausible mistake.  Values travel as float64 arrays holding exactly what the storage type holds."""
import functools

import numpy as np

import dropout_ref as D
from edge_judge import F32, cast


def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- patch rows
def patch_rows(img, P):
    """[B, C, H, W] -> [B, Np, K]: the (c, p, q)-ordered P x P blocks in (ih, iw) order; pixels past the last whole patch are unused"""
    B, C, H, W = img.shape
    nH, nW = H // P, W // P
    return img[:, :, :nH * P, :nW * P].reshape(B, C, nH, P, nW, P).transpose(0, 2, 4, 1, 3, 5).reshape(B, nH * nW, C * P * P)


def layout(rows3, mode, ld):
    """[B, Np, K] patch rows in the output layout of `mode`: 0 [B Np, ld], 1 [K, ld], 2 [B, Np + 1, ld] with a zero row in front of
    every image; + 0 wherever no patch element lands"""
    B, Np, K = rows3.shape
    if mode == 1:
        out = np.zeros((K, ld))
        out[:, :B * Np] = rows3.reshape(B * Np, K).T
    elif mode == 2:
        out = np.zeros((B, Np + 1, ld))
        out[:, 1:, :K] = rows3
    else:
        out = np.zeros((B * Np, ld))
        out[:, :K] = rows3.reshape(B * Np, K)
    return out


def patchify_ref(img, P, mode, ld, dtype):
    return cast(layout(patch_rows(np.asarray(img, np.float64), P), mode, ld), dtype)


def _patch_index(total, B, C, H, W, P, mode, ld, mutant=None):
    """patchify_body / patchify_u8_kernel: for each flat output element e < total, (valid, b, c, y, x) of the pixel it reads"""
    nH, nW = H // P, W // P
    Np, K = nH * nW, C * P * P
    rows = B * Np
    e = np.arange(total, dtype=np.int64)
    if mode == 1:
        k, row = e // ld, e % ld
    else:
        row, k = e // ld, e % ld
    if mode == 2:
        b2, t2 = row // (Np + 1), row % (Np + 1)
        row = np.where(t2 == 0, b2 * Np if mutant == "cls_not_zero" else rows, b2 * Np + t2 - 1)
    if mutant == "pad_not_zero" and mode != 1:
        k = k % K
    valid = (row < rows) & (k < K)
    row, k = np.where(valid, row, 0), np.where(valid, k, 0)
    b, n = row // Np, row % Np
    ih, iw = n // nW, n % nW
    c, p, q = k // (P * P), (k // P) % P, k % P
    if mutant == "swap_pq":
        p, q = q, p
    return valid, b, c, ih * P + p, iw * P + q


def out_shape(B, C, H, W, P, mode, ld):
    Np, K = (H // P) * (W // P), C * P * P
    return {0: (B * Np, ld), 1: (K, ld), 2: (B, Np + 1, ld)}[mode]


def patchify_restate(img, P, mode, ld, dtype, mutant=None):
    img = np.asarray(img, np.float64)
    B, C, H, W = img.shape
    shape = out_shape(B, C, H, W, P, mode, ld)
    valid, b, c, y, x = _patch_index(int(np.prod(shape)), B, C, H, W, P, mode, ld, mutant)
    return cast(np.where(valid, img[b, c, y, x], 0.0), dtype).reshape(shape)


def patchify_u8_ref(img, mean, inv_std, P, mode, ld):
    """(out, S): (px / 255 - mean[c]) * inv_std[c] from the uint8 [B, H, W, C] image, and (px / 255 + |mean|) |inv_std|"""
    x = np.asarray(img, np.float64).transpose(0, 3, 1, 2) / 255.0
    m, s = (np.asarray(v, np.float64).reshape(1, -1, 1, 1) for v in (mean, inv_std))
    return layout(patch_rows((x - m) * s, P), mode, ld), layout(patch_rows((x + np.abs(m)) * np.abs(s), P), mode, ld)


def patchify_u8_restate(img, mean, inv_std, P, mode, ld, dtype, mutant=None):
    B, H, W, C = img.shape
    shape = out_shape(B, C, H, W, P, mode, ld)
    valid, b, c, y, x = _patch_index(int(np.prod(shape)), B, C, H, W, P, mode, ld, mutant)
    mean, inv_std = np.asarray(mean, np.float64).astype(F32), np.asarray(inv_std, np.float64).astype(F32)
    v = (img[b, y, x, c].astype(F32) * (F32(1) / F32(255)) - mean[c]) * inv_std[c]
    nothing = {"pad_small": F32(0.0019), "pad_neg_zero": F32(-0.0)}.get(mutant, F32(0))       # what the CLS slot and the padding hold
    return cast(np.where(valid, v, nothing), dtype).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------- position rows
def posbias_ref(pos, bias, cls):
    """[Np (+ 1 with cls), E] in float32 arithmetic -- one IEEE addition per element"""
    pos, bias = np.asarray(pos, np.float64).astype(F32), np.asarray(bias, np.float64).astype(F32)
    with np.errstate(over="ignore"):
        body = pos[1:] + bias[None, :]
        if cls is None:
            return body.astype(np.float64)
        return np.concatenate([(np.asarray(cls, np.float64).astype(F32) + pos[0])[None, :], body]).astype(np.float64)


def posbias_restate(pos, bias, cls, mutant=None):
    """posbias_body over the flat output"""
    pos, bias = np.asarray(pos, np.float64).astype(F32).reshape(-1), np.asarray(bias, np.float64).astype(F32)
    E = bias.size
    Np = pos.size // E - 1
    lead = E if cls is not None else 0
    i = np.arange(Np * E + lead)
    j = np.maximum(i - lead, 0)
    with np.errstate(over="ignore"):
        body = pos[(0 if mutant == "pos_t" else E) + j] + bias[j % E]
        if cls is None:
            return body.astype(np.float64).reshape(Np, E)
        c = np.asarray(cls, np.float64).astype(F32)
        return np.where(i < lead, c[i % E] + pos[i % E], body).astype(np.float64).reshape(Np + 1, E)


def cls_rows_ref(tokens, cls, pos, dtype):
    """tokens [B, T, E] with row 0 of every image replaced by cls + pos[0]"""
    out = np.array(tokens, np.float64)
    with np.errstate(over="ignore"):
        out[:, 0, :] = cast(np.asarray(cls, np.float64).astype(F32) + np.asarray(pos, np.float64).astype(F32)[0], dtype)
    return out


def cls_rows_restate(tokens, cls, pos, dtype):
    """cls_rows_kernel over i < B E: element (i / E) T E + i % E of the flat token tensor, nothing else"""
    out = np.array(tokens, np.float64)
    B, T, E = out.shape
    cls, pos = np.asarray(cls, np.float64).astype(F32), np.asarray(pos, np.float64).astype(F32).reshape(-1)
    i = np.arange(B * E)
    with np.errstate(over="ignore"):
        out.reshape(-1)[(i // E) * T * E + i % E] = cast(cls[i % E] + pos[i % E], dtype)
    return out


# ---------------------------------------------------------------------------------------------------------------- spectral fold
@functools.lru_cache(maxsize=None)
def basis(P):
    """R [P, Pv, P, P] float64: R[u, v, p, q] = Re(rfft2(impulse at (p, q), norm="ortho"))[u, v]"""
    def impulses(i, n):
        imp = np.zeros((n, P * P))
        imp[np.arange(n), i + np.arange(n)] = 1.0
        return imp.reshape(n, P, P)

    R = np.concatenate([np.fft.rfft2(impulses(i, min(256, P * P - i)), norm="ortho").real for i in range(0, P * P, 256)])
    R = np.ascontiguousarray(R.reshape(P, P, P, P // 2 + 1).transpose(2, 3, 0, 1))
    R.setflags(write=False)
    return R


def fold_ref(w, fh, fw):
    """(W_full [E, C, P, P], S): W_full[e, c, p, q] = sum_{u, v} w[e, c, u, v] fh[u] fw[v] R[u, v, p, q]"""
    w, fh, fw = (np.asarray(a, np.float64) for a in (w, fh, fw))
    E, C, P, Pv = w.shape
    R = basis(P).reshape(P * Pv, P * P)
    a = (w * fh[:, None] * fw[None, :]).reshape(E * C, P * Pv)
    return (a @ R).reshape(E, C, P, P), (np.abs(a) @ np.abs(R)).reshape(E, C, P, P)


def fold_bwd_ref(dwf, w, fh, fw):
    """dict(dw, gw [E, C, P, Pv], dfh [P], dfw [Pv]) and the matching sums of absolute terms: G = dwf . R^T, dw = G fh fw, gw = G w,
    dfh[u] = sum_{e, c, v} gw fw[v], dfw[v] = sum_{e, c, u} gw fh[u]"""
    dwf, w, fh, fw = (np.asarray(a, np.float64) for a in (dwf, w, fh, fw))
    E, C, P, Pv = w.shape
    R = basis(P).reshape(P * Pv, P * P)
    G = (dwf.reshape(E * C, P * P) @ R.T).reshape(E, C, P, Pv)
    A = (np.abs(dwf.reshape(E * C, P * P)) @ np.abs(R).T).reshape(E, C, P, Pv)
    hw = fh[:, None] * fw[None, :]
    ref = dict(dw=G * hw, gw=G * w, dfh=(G * w * fw[None, :]).sum((0, 1, 3)), dfw=(G * w * fh[:, None]).sum((0, 1, 2)))
    S = dict(dw=A * np.abs(hw), gw=A * np.abs(w), dfh=(A * np.abs(w * fw[None, :])).sum((0, 1, 3)), dfw=(A * np.abs(w * fh[:, None])).sum((0, 1, 2)))
    return ref, S


def cospi32(x):
    """cospif of a float32 array, correctly rounded (the argument is exact in float64)"""
    x = np.asarray(x, np.float64)
    r = np.abs(x) % 2.0                                            # exact
    c = np.cos(np.pi * r)
    c = np.where(r == 0.5, 0.0, np.where(r == 1.5, 0.0, c))      # the zeros of cos(pi x) are exact
    return c.astype(F32)


def rcoef32(u, v, p, q, P):
    """rcoef: cospif(2.0f * (float)((u p + v q) % P) / (float)P) / (float)P"""
    m = ((u * p + v * q) % P).astype(F32)
    return cospi32(F32(2) * m / F32(P)) / F32(P)


def fold_restate(w, fh, fw, mutant=None):
    """spectral_fold_body: one fmaf per (u, v) in row-major order from a zero accumulator, the weight product as (w fh[u]) fw[v]"""
    w, fh, fw = (np.asarray(a, np.float64).astype(F32) for a in (w, fh, fw))
    E, C, P, Pv = w.shape
    p, q = np.arange(P)[:, None], np.arange(P)[None, :]
    a = np.zeros((E, C, P, P), F32)
    for u in range(P):
        for v in range(Pv):
            r = rcoef32(u, v, p, q, P)
            if mutant == "no_1_over_P":
                r = r * F32(P)
            if mutant == "half_as_full" and 0 < v < (P + 1) // 2:
                r = r * F32(2)                                    # the weight irfft2 gives a column that stands for its mirror too
            a = fma32((w[:, :, u, v] * fh[u] * fw[v])[:, :, None, None], r[None, None], a)
    return a.astype(np.float64)


def fold_bwd_threads(P):
    """spv_spectral_fold_bwd: the power-of-two workgroup of freq_weight_grad_kernel whose [P + Pv] rows fit 48 KiB of LDS"""
    nt = 1024
    while nt > 64 and nt * (P + P // 2 + 1) * 4 > 48 * 1024:
        nt >>= 1
    return nt


def fold_bwd_restate(dwf, w, fh, fw):
    """spectral_fold_bwd_kernel (fmaf over (p, q) row-major) and freq_weight_grad_kernel (thread t takes (e, c) slices t, t + nt, ...;
    a binary tree over the threads' rows)"""
    dwf, w, fh, fw = (np.asarray(a, np.float64).astype(F32) for a in (dwf, w, fh, fw))
    E, C, P, Pv = w.shape
    u, v = np.arange(P)[:, None], np.arange(Pv)[None, :]
    g = np.zeros((E, C, P, Pv), F32)
    for p in range(P):
        for q in range(P):
            g = fma32(dwf[:, :, p, q][:, :, None, None], rcoef32(u, v, p, q, P)[None, None], g)
    dw, gw = g * fh[:, None] * fw[None, :], g * w
    nt, EC = fold_bwd_threads(P), E * C
    t = gw.reshape(EC, P, Pv)
    pad = (-EC) % nt
    t = np.concatenate([t, np.zeros((pad, P, Pv), F32)]).reshape(-1, nt, P, Pv)        # [trip, thread, u, v]
    mh, mw = np.zeros((nt, P), F32), np.zeros((nt, Pv), F32)
    for trip in t:
        for uu in range(P):
            for vv in range(Pv):
                mh[:, uu] = mh[:, uu] + trip[:, uu, vv] * fw[vv]
                mw[:, vv] = mw[:, vv] + trip[:, uu, vv] * fh[uu]
    stride = nt >> 1
    while stride >= 1:
        mh[:stride], mw[:stride] = mh[:stride] + mh[stride:2 * stride], mw[:stride] + mw[stride:2 * stride]
        stride >>= 1
    return {k: a.astype(np.float64) for k, a in dict(dw=dw, gw=gw, dfh=mh[0], dfw=mw[0]).items()}


# ---------------------------------------------------------------------------------------------------------------- dropout
def mask_scale(seed, idx, p, shift=12):
    """float32 scale of spv_dropout / spv_embed_bwd / the token GEMM for flat indices idx: key(idx >> 12) hashed with the pair
    (idx & 4095) >> 1, the low 16 bits for an even column; 0 where dropped, 1 / (1 - p) where kept"""
    idx = np.asarray(idx, np.uint64)
    if p == 0:
        return np.ones(idx.shape, F32)
    key = D.row_key(seed, (idx >> np.uint64(shift)).reshape(-1)).reshape(idx.shape)
    col = (idx & np.uint64(4095)).astype(np.uint32)
    h = D.mix32(key + (col >> np.uint32(1)) * D.GOLDEN).reshape(idx.shape)
    u16 = np.where(col & np.uint32(1), h >> np.uint32(16), h & np.uint32(0xFFFF))
    return np.where(u16 < np.uint32(D.threshold(p)), F32(0), D.inv_keep(p)).astype(F32)


def dropout_ref(x, p, seed, dtype):
    """y = x * keep / (1 - p) with dropout_ref.keep's mask over 4096-element rows: one float32 multiplication, then the storage rounding"""
    x = np.asarray(x, np.float64).astype(F32).reshape(-1)
    if p == 0:
        return cast(x, dtype)
    keep = D.keep(seed, (x.size + 4095) // 4096, 4096, p).reshape(-1)[:x.size]
    with np.errstate(over="ignore"):
        return cast(x * np.where(keep, D.inv_keep(p), F32(0)).astype(F32), dtype)


def dropout_restate(x, p, seed, dtype, mutant=None):
    x = np.asarray(x, np.float64).astype(F32).reshape(-1)
    with np.errstate(over="ignore"):
        return cast(x * mask_scale(seed, np.arange(x.size), p, 11 if mutant == "key_shift_11" else 12), dtype)


# ---------------------------------------------------------------------------------------------------------------- embedding backward
EB_GS = 16


def embed_dtok(g, gcls, p, seed, dtype, mutant=None):
    """dtok [B, T, E]: (g [+ gcls on row 0]) * mask(b T E + col), float32 operations, then the storage rounding"""
    x = np.array(g, np.float64).astype(F32)
    B, T, E = x.shape
    if gcls is not None:
        c = np.asarray(gcls, np.float64).astype(F32)
        if mutant == "gcls_every_row":
            x = x + c[:, None, :]
        else:
            x[:, 0, :] = x[:, 0, :] + c
    idx = np.arange(B * T * E, dtype=np.uint64).reshape(B, T, E)
    if mutant == "mask_no_sample_offset":
        idx = idx % np.uint64(T * E)
    return cast(x * mask_scale(seed, idx, p, 11 if mutant == "key_shift_11" else 12), dtype)


def embed_bwd_ref(dtok):
    """dict(dpos [T, E], dbias [E], dcls [E]) as float64 sums of the dtok values, and the sums of their absolute values"""
    d = np.asarray(dtok, np.float64)
    ref = dict(dpos=d.sum(0), dbias=d[:, 1:].sum((0, 1)), dcls=d[:, 0].sum(0))
    S = dict(dpos=np.abs(d).sum(0), dbias=np.abs(d[:, 1:]).sum((0, 1)), dcls=np.abs(d[:, 0]).sum(0))
    return ref, S


def _sum4x8(terms):
    """the fold kernels' order over terms [n, ...]: batches of 8 into four accumulators (term u to a[u & 3]), the tail into a[0],
    (a0 + a1) + (a2 + a3)"""
    a = np.zeros((4,) + terms.shape[1:], F32)
    g = 0
    while g + 8 <= len(terms):
        for u in range(8):
            a[u & 3] = a[u & 3] + terms[g + u]
        g += 8
    for t in terms[g:]:
        a[0] = a[0] + t
    return (a[0] + a[1]) + (a[2] + a[3])


def embed_bwd_restate(dtok, mutant=None):
    """embed_bwd_rows_kernel's per-group sums (16 samples in order), embed_bwd_fold_kernel and embed_bwd_bias_kernel in float32"""
    d = np.asarray(dtok, np.float64).astype(F32)
    B, T, E = d.shape
    groups = -(-B // EB_GS)
    partials = np.zeros((groups, T, E), F32)
    for gi in range(groups - 1 if mutant == "last_group_dropped" else groups):
        for b in range(gi * EB_GS, min(B, (gi + 1) * EB_GS)):
            partials[gi] = partials[gi] + d[b]
    dpos = _sum4x8(partials)
    dbias = _sum4x8(dpos[0 if mutant == "dbias_with_cls" else 1:])
    dcls = dpos[1 if mutant == "dcls_row_1" and T > 1 else 0]
    return {k: a.astype(np.float64) for k, a in dict(dpos=dpos, dbias=dbias, dcls=dcls).items()}
