"""Host restatement of the counter-hash dropout mask (csrc/spv_common.h: mix32 / dropout_row_key / dropout_scale) in numpy uint32
arithmetic, and a float64 reference of the attention core with that mask (csrc/spv_attn.hip), written from the definitions and
independent of spectre_vit.  tests/test_gpu_dropout_mask.py pins keep() to the device bit for bit; the attention tests then compare
every kernel family with attention() under the mask keep() predicts."""
import numpy as np

GOLDEN = np.uint32(0x9E3779B1)


def mix32(x):
    """the murmur3-style 32-bit finaliser, elementwise on a uint32 array (products wrap modulo 2^32)"""
    x = np.array(x, dtype=np.uint32, ndmin=1)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def row_key(seed, rows):
    """dropout_row_key: mix32(seed_lo + row_lo * golden) ^ mix32(seed_hi + row_hi) for an array of 64-bit row ids"""
    rows = np.asarray(rows, dtype=np.uint64)
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    return mix32(lo + (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32) * GOLDEN) ^ mix32(hi + (rows >> np.uint64(32)).astype(np.uint32))


def threshold(p):
    """the 16-bit drop threshold, in float32 as the device computes it: (unsigned)(p * 65536.0f + 0.5f)"""
    return int(np.float32(p) * np.float32(65536) + np.float32(0.5))


def inv_keep(p):
    """the factor a kept element is scaled by, as the device's float32 arithmetic gives it: 1.0f / (1.0f - p)"""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def hash_words(seed, row_ids, pairs):
    """uint32[len(row_ids), pairs]: the one hash word that serves columns 2j and 2j + 1 of each row"""
    key = row_key(seed, np.asarray(row_ids).reshape(-1))
    j = np.arange(pairs, dtype=np.uint32) * GOLDEN
    return mix32(key[:, None] + j[None, :])


def keep_rows(seed, row_ids, cols, p):
    """bool[len(row_ids), cols]: True where the element (row id, column) is kept"""
    h = hash_words(seed, row_ids, (cols + 1) // 2)
    u16 = np.stack([h & np.uint32(0xFFFF), h >> np.uint32(16)], axis=-1).reshape(h.shape[0], -1)[:, :cols]   # even column: low half
    return u16 >= np.uint32(threshold(p))


def keep(seed, rows, cols, p):
    """bool[rows, cols] of the rows 0 .. rows - 1"""
    return keep_rows(seed, np.arange(rows, dtype=np.uint64), cols, p)


def attention_keep(seed, seqs, heads, length, p, row0=False):
    """the attention kernels' mask, bool[seqs, heads, len (1 if row0), len]: row id (s * heads + h) * len + i, column = key index"""
    i = np.arange(1 if row0 else length, dtype=np.uint64)
    ids = (np.arange(seqs * heads, dtype=np.uint64) * np.uint64(length))[:, None] + i[None, :]
    return keep_rows(seed, ids, length, p).reshape(seqs, heads, -1, length)


# ----------------------------------------------------------------------------------------------------------------- attention
def bf16_round(a):
    """round to nearest even onto the bf16 grid (through float32), returned as float64"""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def split_heads(x, heads):
    """[S, L, heads * hd] -> [S, heads, L, hd]"""
    S, L, E = x.shape
    return x.reshape(S, L, heads, E // heads).transpose(0, 2, 1, 3)


def attention(q, k, v, dctx, keep_mask=None, p=0.0, mode="exact"):
    """ctx = (softmax(q k^T / sqrt(hd)) * keep / (1 - p)) v and its gradients, per (sequence, head).

    q, dctx [S, H, Lq, hd]; k, v [S, H, L, hd]; keep_mask bool [S, H, Lq, L] or None.  Returns dict(ctx, dq [S, H, Lq, hd], dk, dv
    [S, H, L, hd], probs [S, H, Lq, L] (unmasked)).  The mask multiplies P in the forward and dP in the backward.
    mode "exact": float64 throughout.  The other two give the rounding floor of a kernel that is right:
    mode "fp32": every array and every operation in numpy float32;
    mode "bf16": float64, with the masked P, dS and the four outputs rounded to bf16 -- where the bf16 kernels round."""
    ft = np.float32 if mode == "fp32" else np.float64
    rnd = bf16_round if mode == "bf16" else (lambda a: a)
    q, k, v, dctx = (np.asarray(a, dtype=ft) for a in (q, k, v, dctx))
    scale = ft(1.0) / np.sqrt(ft(q.shape[-1]))
    T = lambda a: np.swapaxes(a, -1, -2)
    s = (q @ T(k)) * scale
    e = np.exp(s - s.max(-1, keepdims=True))
    probs = e / e.sum(-1, keepdims=True)
    m = ft(1.0) if keep_mask is None else keep_mask.astype(ft) * (ft(1.0) / (ft(1.0) - ft(np.float32(p))))
    pm = rnd(probs * m)
    dp = (dctx @ T(v)) * m
    ds = rnd(probs * (dp - (probs * dp).sum(-1, keepdims=True)) * scale)
    out = dict(ctx=rnd(pm @ v), dq=rnd(ds @ k), dk=rnd(T(ds) @ q), dv=rnd(T(pm) @ dctx), probs=probs)
    assert all(a.dtype == ft for a in out.values())
    return out


def block_errors(got, ref):
    """max |got - ref| / max |ref| over each (sequence, head) block of [S, H, ...] arrays -> float64 [S, H].  A block whose reference
    is zero throughout (one key row: dS = 0) must be zero in `got` as well: error 0, otherwise inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    S, H = ref.shape[:2]
    d = np.abs(got - ref).reshape(S, H, -1).max(-1)
    r = np.abs(ref).reshape(S, H, -1).max(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r > 0, d / r, np.where(d == 0, 0.0, np.inf))
