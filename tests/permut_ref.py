"""float64 references of the permutation-gather family (csrc/spv_permut.hip): the packed tables of spv_permut_pack, the gather forward
with its pooled output, the gather backward, and the row-0 pair -- written from the definitions (g[b, h, j] = sign[h, j] x[b, perm[h, j]])
with plain numpy indexing, none of the kernels' tiling.  tests/test_permut_ref.py checks them against the dense signed-permutation
matrix and the oracle.  Below them, float32 restatements of the kernels' arithmetic with switches for the mistakes the bars must catch."""
import numpy as np

import permut_edge_cases as C

SIGN = np.uint32(0x80000000)


# ------------------------------------------------------------------------------------------------------------------ pack
def wide_tables(perms, signs):
    """(fwd, inv) uint32 [heads, d]: fwd[h, j] = perm[h, j] | sign[h, j] << 31; inv[h, perm[h, j]] = j | sign[h, j] << 31"""
    heads, d = perms.shape
    s = np.where(signs < 0, SIGN, np.uint32(0)).astype(np.uint32)
    fwd = perms.astype(np.uint32) | s
    inv = np.empty_like(fwd)
    j = np.arange(d, dtype=np.uint32)
    for h in range(heads):
        inv[h, perms[h]] = j | s[h]
    return fwd, inv


def compact_tables(wide):
    """(uint16 [heads * d] indices, uint8 [heads * d / 8] sign bits, element k of an octet in bit k) of one wide table"""
    flat = wide.reshape(-1)
    sg = ((flat >> 31).astype(np.uint8).reshape(-1, 8) << np.arange(8, dtype=np.uint8)).sum(1).astype(np.uint8)
    return (flat & 0xffff).astype(np.uint16), sg


def scatter_lists(wide):
    """one list set of a long row: off int32 [heads, parts + 1] and, per (head, part), the set of (ej, et) = (source | sign << 31,
    target - part * L) over the sources whose target -- the table's entry -- lies in that part"""
    heads, d = wide.shape
    L, parts = C.scat_len(d), C.scat_parts(d)
    tgt = (wide & 0x7fffffff).astype(np.int64)
    part = tgt // L
    off = np.zeros((heads, parts + 1), np.int32)
    lists = {}
    src = np.arange(d, dtype=np.uint32)
    for h in range(heads):
        off[h, 1:] = np.cumsum(np.bincount(part[h], minlength=parts))
        ej = src | (wide[h] & SIGN)
        et = (tgt[h] - part[h] * L).astype(np.uint16)
        for q in range(parts):
            m = part[h] == q
            lists[(h, q)] = np.sort(ej[m].astype(np.uint64) << np.uint64(16) | et[m].astype(np.uint64))
    return off, lists


def table_layout(heads, d):
    """word offsets of the table's sections: {name: (first word, words)}"""
    total = heads * d
    out, at = dict(fwd=(0, total), inv=(total, total)), 2 * total
    if C.compact_ok(d):
        out["compact"] = (at, total + (total // 4 + 3) // 4)
        at += out["compact"][1]
    if C.long_row(d):
        for s in range(2):
            out[f"scat{s}"] = (at, C.scat_set_words(heads, d))
            at += C.scat_set_words(heads, d)
    assert at == C.table_words(heads, d)
    return out


def split_scatter_set(words, heads, d):
    """the sections of one list set as the device wrote them: off, cur [heads, parts], ej [heads, d], et uint16 [heads, d] + the pad"""
    parts, total = C.scat_parts(d), heads * d
    a = heads * (parts + 1)
    b = a + heads * parts
    et = words[b + total:].view(np.uint16)
    return dict(off=words[:a].view(np.int32).reshape(heads, parts + 1), cur=words[a:b].view(np.int32).reshape(heads, parts),
                ej=words[b:b + total].reshape(heads, d), et=et[:total].reshape(heads, d), pad=et[total:])


# ------------------------------------------------------------------------------------------------------------------ values
def gather_fwd(x, perms, signs, pw=0):
    """x [B, d] -> g [B, heads * d]; with pw: also pooled [B, heads * d / pw] and the windows' sum |terms|"""
    B = x.shape[0]
    with np.errstate(invalid="ignore"):
        g = (x[:, perms] * signs[None].astype(np.float64)).reshape(B, -1)
        if not pw:
            return g
        w = g.reshape(B, -1, pw)
        return g, w.sum(-1) / pw, np.abs(w).sum(-1)


def gather_bwd(dg, perms, signs):
    """dg [B, heads * d] -> dx [B, d] = sum_h sign[h, inv_h(i)] dg[b, h, inv_h(i)], and sum_h |term|"""
    heads, d = perms.shape
    B = dg.shape[0]
    t = dg.reshape(B, heads, d) * signs[None].astype(np.float64)
    dx, ab = np.zeros((B, d)), np.zeros((B, d))
    with np.errstate(invalid="ignore"):
        for h in range(heads):
            dx[:, perms[h]] += t[:, h]
            ab[:, perms[h]] += np.abs(t[:, h])
    return dx, ab


def row0_fwd(x, perm0, sign0, n, embed):
    """g0 [B, n] = sign x[b, perm] over the first n entries of head 0; x0 [B, embed] = the sample's own first embed elements"""
    return x[:, perm0[:n]] * sign0[None, :n].astype(np.float64), x[:, :embed].copy()


def row0_bwd(dg0, dx0, perm0, sign0, d):
    """dx [B, d] = dx0 in the first embed elements, zero elsewhere, + the n scattered values; and (|dx0 part|, |dg0 part|)"""
    B, n = dg0.shape
    a = np.zeros((B, d))
    a[:, :dx0.shape[1]] = dx0
    s = np.zeros((B, d))
    s[:, perm0[:n]] = dg0 * sign0[None, :n].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return a + s, np.abs(a), np.abs(s)


def dense(perms, signs):
    """the signed permutation matrices P[h] [d, d]: g[:, h] = x @ P[h].T"""
    heads, d = perms.shape
    P = np.zeros((heads, d, d))
    for h in range(heads):
        P[h, np.arange(d), perms[h]] = signs[h]
    return P


# ------------------------------------------------------------------------------------------------------------------ float32 restatements
def _store(a32, dtype):
    return C.storage_round(a32.astype(np.float64), dtype)


def _tree_sum(w):
    """fp32 sum over the last axis (a power of two, or any length: then left to right), pairs first: the DPP order"""
    w = w.astype(np.float32)
    n = w.shape[-1]
    if n & (n - 1):
        acc = np.zeros(w.shape[:-1], np.float32)
        for k in range(n):
            acc = (acc + w[..., k]).astype(np.float32)
        return acc
    while w.shape[-1] > 1:
        w = (w[..., 0::2] + w[..., 1::2]).astype(np.float32)
    return w[..., 0]


def emulate_fwd(x, fwd, inv, dtype, pw=0, mistake=None):
    """the forward kernels in float32 from the packed tables: the copy with its sign bit, the fp32 window sum, * 1 / pw, the storage
    rounding.  x [B, d] float64 (storage-exact), fwd / inv uint32 [heads, d].  Returns g (, pooled) as float64.
    mistakes: "sign" (the sign bit dropped for the last head), "inverse" (the inverse table read), "last_piece" (the last 16 bytes of
    the row never staged: zeros), "ror" (window 32's upper half from the neighbour window: row_ror the wrong way), "pair" (the second
    sample of a pair served from the first sample's row), "part" (a scatter part written 8 elements late)"""
    heads, d = fwd.shape
    B = x.shape[0]
    tab = inv if mistake == "inverse" else fwd
    row = x.astype(np.float32)
    if mistake == "last_piece":
        row = row.copy()
        row[:, d - 16 // C.ES[dtype]:] = 0.0
    if mistake == "pair":
        row = row.copy()
        row[1::2] = row[0::2][:B // 2]
    neg = (tab >> 31).astype(bool)
    if mistake == "sign":
        neg = neg.copy()
        neg[-1] = False
    with np.errstate(invalid="ignore", over="ignore"):
        g = row[:, tab & 0x7fffffff]
        g = np.where(neg[None], -g, g).reshape(B, -1)
        if mistake == "part":
            L = C.scat_len(d)
            g3 = g.reshape(B, heads, d).copy()
            for q in range(1, C.scat_parts(d)):
                g3[:, :, q * L + 8:min((q + 1) * L, d)] = g.reshape(B, heads, d)[:, :, q * L:min((q + 1) * L, d) - 8]
            g = g3.reshape(B, -1)
        if not pw:
            return g.astype(np.float64)
        w = g.reshape(B, -1, pw)
        if mistake == "ror":
            assert pw == 32 and w.shape[1] % 2 == 0
            w = w.copy()
            up = w[:, :, 16:].copy()
            w[:, 0::2, 16:], w[:, 1::2, 16:] = up[:, 1::2], up[:, 0::2]
        pooled = (_tree_sum(w) * np.float32(1.0 / pw)).astype(np.float32)
    return g.astype(np.float64), _store(pooled, dtype)


def emulate_bwd(dg, inv, dtype, mistake=None):
    """dx[b, i] = fp32 sum over the heads in ascending order of +-dg[b, h, inv[h, i]], rounded to the storage type.
    mistake "head": the last head left out"""
    heads, d = inv.shape
    B = dg.shape[0]
    t = dg.reshape(B, heads, d).astype(np.float32)
    acc = np.zeros((B, d), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(heads - (mistake == "head")):
            v = t[:, h, inv[h] & 0x7fffffff]
            acc = (acc + np.where((inv[h] >> 31).astype(bool)[None], -v, v)).astype(np.float32)
    return _store(acc, dtype)


def emulate_row0_fwd(x, fwd0, n, embed, dtype, mistake=None):
    """(g0, x0); mistake "x0": x0 left unwritten (NaN) from n on -- the global kernel's thread per gathered element"""
    row = x.astype(np.float32)
    w = fwd0[:n]
    v = row[:, w & 0x7fffffff]
    g0 = np.where((w >> 31).astype(bool)[None], -v, v)
    x0 = x[:, :embed].copy()
    if mistake == "x0":
        x0[:, n:] = np.nan
    return _store(g0, dtype), x0


def emulate_row0_bwd(dg0, dx0, fwd0, d, dtype):
    """the row starts as dx0 | 0 in the storage type; each scattered value is added in fp32 and the sum stored"""
    B, n = dg0.shape
    row = np.zeros((B, d), np.float32)
    row[:, :dx0.shape[1]] = dx0
    w = fwd0[:n]
    v = dg0.astype(np.float32)
    tgt = w & 0x7fffffff
    with np.errstate(invalid="ignore", over="ignore"):
        row[:, tgt] = _store((row[:, tgt] + np.where((w >> 31).astype(bool)[None], -v, v)).astype(np.float32), dtype)
    return row.astype(np.float64)
