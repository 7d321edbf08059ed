"""Float64 references of the dense contractions of csrc/spv_gemm.hip, written from the definitions in include/spv.h and independent
of spectre_vit: the NT form A B^T with every epilogue term, the TN form A^T B over the first k rows, and the column folds.  Each
returns, beside the value, S = the sum of the absolute values of every term of each element (products, biases, pool term, old C):
the scale of tests/gemm_edge_cases.py's first-order rounding bar."""
import numpy as np

import dropout_ref as D


def flat_keep(seed, total, p):
    """bool[total]: the dropout mask over a flat index, mask(i) = hash(key(i >> 12), i & 4095) (csrc/spv_patch.hip)"""
    blocks = (total + 4095) // 4096
    return D.keep_rows(seed, np.arange(blocks, dtype=np.uint64), 4096, p).reshape(-1)[:total]


def out_rows(M, rg=0, gs=0, roff=0):
    """the output row of each of the M product rows: the identity, or the grouped map (row / rg) * gs + roff + row % rg"""
    r = np.arange(M)
    return r if rg == 0 else (r // rg) * gs + roff + r % rg


def nt(A, B, bias=None, bias2d=None, rg=0, gs=0, roff=0, pool=None, pw=0, old=None, drop=None, ldc=None, scale=True):
    """C[out_rows(m)][n] = (sum_k A[m][k] B[n][k] + bias[n] + bias2d[m % rg][n] + pool[m][n / pw] / pw) * factor(flat index) + old.

    A [M, K], B [N, K]; old: the previous content of the M output rows, [M, N]; drop = (seed, p): the factor is 0 where the mask over the
    flat index out_row * ldc + n drops and the float32 value 1 / (1 - p) elsewhere.  Returns (value [M, N], S [M, N], kept [M, N] bool);
    S is None when scale is False (an exact comparison needs none)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    M, N = A.shape[0], B.shape[0]
    v = A @ B.T
    S = np.abs(A) @ np.abs(B).T if scale else None

    def add(t):
        nonlocal v, S
        v = v + t
        if scale:
            S = S + np.abs(t)
    if bias is not None:
        add(np.asarray(bias, np.float64)[None, :])
    if bias2d is not None:
        add(np.asarray(bias2d, np.float64)[np.arange(M) % rg])
    if pool is not None:
        add(np.repeat(np.asarray(pool, np.float64), pw, axis=1) / pw)        # column n takes window n / pw
    kept = np.ones((M, N), bool)
    if drop is not None and drop[1] > 0:
        seed, p = drop
        rows = out_rows(M, rg, gs, roff)
        flat = rows[:, None] * ldc + np.arange(N)[None, :]
        kept = flat_keep(seed, int(flat.max()) + 1, p)[flat]
        f = np.where(kept, np.float64(D.inv_keep(p)), 0.0)
        v = v * f
        if scale:
            S = S * f
    if old is not None:
        add(np.asarray(old, np.float64))
    return v, S, kept


def tn(A, B, k=None, old=None):
    """C[m][n] = sum_{r < k} A[r][m] B[r][n] (+ old).  A [K, M], B [K, N].  Returns (value [M, N], S [M, N])."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    k = A.shape[0] if k is None else k
    v, S = A[:k].T @ B[:k], np.abs(A[:k]).T @ np.abs(B[:k])
    if old is not None:
        v, S = v + old, S + np.abs(old)
    return v, S


def fold(partials):
    """out[p][c] = sum_w partials[w][p][c].  partials [parts, nsum, n].  Returns (value [nsum, n], S [nsum, n])."""
    partials = np.asarray(partials, np.float64)
    return partials.sum(0), np.abs(partials).sum(0)
