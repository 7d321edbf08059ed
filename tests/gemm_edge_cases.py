"""Case tables, bars and the Python restatement of csrc/spv_gemm_core.h for tests/test_gemm_ref.py (CPU) and
tests/test_gpu_gemm_edges.py (GPU).  No GPU, no spectre_vit.

Restatement: strip_plan, nt_plan, tn_plan, tnb_plan answer as the header's strip_plan, gemm_nt_plan, gemm_tn_plan and
gemm_tn_batch_plan do; test_gemm_ref.py compiles the header and compares them over a grid around every threshold.

Two input sets per case.  "int": every operand an integer in [-3, 3] (pool windows powers of two, p = 0.5 so that 1 / (1 - p) = 2):
every product and every partial sum in any order is an integer (or, with a pool term, a multiple of 1 / window) below 2^24 in
magnitude, which float32 holds exactly -- exact_ok() asserts it per case -- so an fp32 output equals the float64 reference exactly and
a bf16 output equals its bf16 rounding.  "normal": storage-exact standard normals against the elementwise bar

    |got - ref| <= u |ref| + (n + 2) 2^-24 S

u = 2^-8 for a bf16-stored output (the unit roundoff of its 8 significant bits under round-to-nearest: an element that rounds at the
worst place of a binade sits just below ratio 1 by construction) and 0 for fp32; S = the sum of the absolute values of every term of the element; n = the fp32 additions on the element's
longest chain: K products, one per slab, and one per epilogue operation (bias, 2-D bias, pool scale and add, dropout scale, old C).
That is the first-order bound (1 + 2^-24)^n - 1 ~ n 2^-24 of a sum taken in ANY order, relative to S; it holds no measured constant."""
import zlib
from dataclasses import dataclass

import numpy as np

import dropout_ref as D
import gemm_ref as R

SENT = -7680.0          # test_gpu_attention_edges.SENT: exact in bf16
SEED = 0x5EED0123456789
EPS = 2.0 ** -24
CODE = {"fp32": 0, "bf16": 1}
ES = {"fp32": 4, "bf16": 2}


def cdiv(a, b):
    return -(-a // b)


# =========================================================================================== restatement of spv_gemm_core.h
def reduce_blocks(M, N, threads):
    return min((M * N // (4 if N % 4 == 0 else 1) + threads - 1) // threads, 2048)


def strip_plan(M, N, K, reserved=0):
    """None, or (MB, nstrips, groups, base, rem)"""
    if N <= 0 or N % 256 or N > 16384 or K % 128 or K < 128 or M < 8192:
        return None
    nstrips, nblk = N // 256, cdiv(M, 32)
    groups = (256 - reserved) // nstrips
    if groups < 1:
        return None
    groups = min(groups, nblk)
    base, rem = divmod(nblk, groups)

    def padded(mb, c):
        slots = 0
        while c > 0:
            take = 2 * mb + 1 if (c % (2 * mb) and c >= 2 * mb + 1) else min(2 * mb, c)
            slots += max(take, 2 * mb)
            c -= take
        return slots
    worst = base + (1 if rem else 0)
    best, best_slots = 0, 1 << 30
    for mb in (4, 3, 2):
        s = padded(mb, worst)
        if s < best_slots:
            best, best_slots = mb, s
    if best == 0 or best_slots * 100 > worst * 115:
        return None
    return best, nstrips, groups, base, rem


def nt_plan(din, dout, M, N, K, lda, ldb, ldc, a_lo=0, b_lo=0, c_lo=0, bias_lo=-1, accumulate=0, splits=1, ws_lo=-1, rg=0, bias2d_lo=-1,
            pool=0, pool_pw=0, pool_bf16=0, drop=0, reserved=0):
    """dict(kernel, splits, k_per_split, grid, mb, epi, nstrips, groups, base, rem, reduce, reduce_blocks); a refusal has only `kernel`.
    din / dout: dtype codes (0 fp32, 1 bf16)"""
    def out(kernel, **kw):
        d = dict(kernel=kernel, splits=0, k_per_split=0, grid=0, mb=0, epi=0, nstrips=0, groups=0, base=0, rem=0, reduce=0, reduce_blocks=0)
        d.update(kw)
        return d
    if not (M > 0 and N > 0 and K > 0):
        return out("refuse_empty")
    if din not in (0, 1) or dout not in (0, 1):
        return out("refuse_dtype")
    ch = 8 if din == 1 else 4
    if K % ch or lda % ch or ldb % ch:
        return out("refuse_chunk")
    if a_lo != 0 or b_lo != 0:
        return out("refuse_align")
    if lda < K or ldb < K or ldc < N:
        return out("refuse_ld")
    if splits < 1:
        return out("refuse_splits")
    if splits > 1 and ws_lo != 0:
        return out("refuse_workspace")
    BK = 64 if din == 1 else 32
    s, kps = 1, K
    if splits > 1:
        kps = cdiv(cdiv(K, splits), BK) * BK
        s = cdiv(K, kps)
    com = dict(splits=s, k_per_split=kps, grid=cdiv(M, 128) * cdiv(N, 128) * s, reduce=int(s > 1), reduce_blocks=reduce_blocks(M, N, 256) if s > 1 else 0)
    plain = rg == 0 and bias2d_lo < 0 and not drop
    t32 = cdiv(M, 32) * cdiv(N, 32)
    if din == 1 and s == 1 and M <= 2048 and K <= 1536 and plain and not pool and K % 16 == 0 and 64 <= t32 <= 1024:
        return out("rows", **{**com, "grid": t32})
    if din == 1 and dout == 1:
        pool_ok = (not pool) or (pool_bf16 and not accumulate and pool_pw >= 8 and N % pool_pw == 0)
        span32 = M * lda * 2 < 2 ** 32 and N * ldb * 2 < 2 ** 32
        sp = strip_plan(M, N, K, reserved) if (s == 1 and plain and pool_ok and span32 and ldc % 8 == 0 and c_lo == 0 and (bias_lo < 0 or bias_lo % 4 == 0)) else None
        if sp is not None:
            mb, nstrips, groups, base, rem = sp
            epi = (3 if pool_pw % 8 else 2) if pool else (1 if accumulate else 0)
            return out("strip", **{**com, "grid": groups * nstrips, "mb": mb, "epi": epi, "nstrips": nstrips, "groups": groups, "base": base, "rem": rem})
    glds = din == 1 and K % 64 == 0 and kps % 64 == 0 and min(K, kps) > 1024
    return out("glds" if glds else "tile", **com)


def tn_plan(dout, M, N, K, lda, ldb, ldc, a_lo=0, b_lo=0, splits=1, ws_lo=-1, fold_blocks=0):
    """dict(kernel, reduce, splits, k_per_split, grid, reduce_blocks); reduce: 0 none, 1 plain, 2 with folds, 3 the fold alone"""
    def out(kernel, **kw):
        d = dict(kernel=kernel, reduce=0, splits=0, k_per_split=0, grid=0, reduce_blocks=0)
        d.update(kw)
        return d
    if not (M > 0 and N > 0 and K > 0):
        return out("refuse_empty")
    if dout not in (0, 1):
        return out("refuse_dtype")
    if M % 8 or N % 8 or lda % 8 or ldb % 8:
        return out("refuse_chunk")
    if a_lo != 0 or b_lo != 0:
        return out("refuse_align")
    if lda < M or ldb < N or ldc < N:
        return out("refuse_ld")
    if not (splits >= 1 and (splits == 1 or ws_lo == 0)):
        return out("refuse_workspace")
    if fold_blocks < 0:
        return out("refuse_folds")
    tiles_m, tiles_n = cdiv(M, 128), cdiv(N, 128)
    s, kps = 1, K
    if splits > 1:
        kps = cdiv(cdiv(K, splits), 64) * 64
        s = cdiv(K, kps)
    if M == 512 and N % 128 == 0 and N >= 1024 and tiles_n * s >= 192 and kps >= 512:
        kernel, grid = "tall", tiles_n * s
    elif s >= 4 and M % 256 == 0 and N % 128 == 0 and (M // 256) * tiles_n * s >= 128:
        kernel, grid = "wide", (M // 256) * tiles_n * s
    else:
        kernel, grid = ("tile1" if N <= 64 else "tile3"), tiles_m * tiles_n * s
    red = (2 if fold_blocks > 0 else 1) if s > 1 else (3 if fold_blocks > 0 else 0)
    return out(kernel, reduce=red, splits=s, k_per_split=kps, grid=grid, reduce_blocks=reduce_blocks(M, N, 256) if s > 1 else 0)


def tnb_plan(probs, K, splits, ws_lo=0, fold_blocks=0):
    """probs: list of dict(m, n, lda, ldb, ldc, k[, a_lo, b_lo, has_ptrs]) or None.  dict(kernel, bad, splits, k_per_split, nlong, order,
    first_tile, wide_first_tile, ws_off, grid, reduce_blocks); a refusal has only kernel and bad"""
    def refuse(kernel, bad=-1):
        return dict(kernel=kernel, bad=bad)
    if probs is None or not 1 <= len(probs) <= 8:
        return refuse("refuse_count")
    if not (K > 0 and splits >= 1 and ws_lo == 0):
        return refuse("refuse_call")
    if fold_blocks < 0:
        return refuse("refuse_folds")
    kps = cdiv(cdiv(K, splits), 64) * 64
    s = cdiv(K, kps)
    for i, q in enumerate(probs):
        if not 0 <= q["k"] <= K:
            return refuse("refuse_k", i)
    is_long = [q["k"] in (0, K) for q in probs]
    order = [i for i, l in enumerate(is_long) if l] + [i for i, l in enumerate(is_long) if not l]
    nlong = sum(is_long)
    if nlong < 1:
        return refuse("refuse_no_long")
    tiles = wt = long_tiles = wlong = off = 0
    rb, wide = 1, kps >= 512
    first, wfirst, ws_off = [], [], []
    for i, o in enumerate(order):
        q = probs[o]
        if not (q.get("has_ptrs", 1) and q["m"] > 0 and q["n"] > 0):
            return refuse("refuse_empty", o)
        if q["m"] % 8 or q["n"] % 8 or q["lda"] % 8 or q["ldb"] % 8 or q["lda"] < q["m"] or q["ldb"] < q["n"] or q["ldc"] < q["n"]:
            return refuse("refuse_shape", o)
        if q.get("a_lo", 0) != 0 or q.get("b_lo", 0) != 0:
            return refuse("refuse_align", o)
        if i >= nlong and q["ldc"] % 4:
            return refuse("refuse_short_ldc", o)
        wide = wide and q["m"] % 256 == 0 and q["n"] % 128 == 0 and (q["k"] == 0 or q["k"] >= 64)
        first.append(tiles), wfirst.append(wt), ws_off.append(off)
        tiles += cdiv(q["m"], 128) * cdiv(q["n"], 128)
        wt += (q["m"] // 256) * cdiv(q["n"], 128)
        if i < nlong:
            long_tiles, wlong = tiles, wt
            off += s * q["m"] * q["n"]
            rb = max(rb, reduce_blocks(q["m"], q["n"], 1024))
    first.append(tiles), wfirst.append(wt)
    grid = wlong * s + ((wt - wlong + 7) & ~7) if wide else long_tiles * s + ((tiles - long_tiles + 7) & ~7)
    return dict(kernel="batch_wide" if wide else "batch128", bad=-1, splits=s, k_per_split=kps, nlong=nlong, order=order, first_tile=first,
                wide_first_tile=wfirst, ws_off=ws_off, grid=grid, reduce_blocks=rb)


def fold_blocks(jobs):
    """workgroups of a list of (parts, nsum, n) fold jobs; -1 for a bad list"""
    if len(jobs) > 16:
        return -1
    if any(not (parts > 0 and 1 <= nsum <= 5 and n > 0) for parts, nsum, n in jobs):
        return -1
    return sum(cdiv(nsum * n, 32) for _, nsum, n in jobs)


# ======================================================================================================== number formats, bars
def q(a, dt):
    """round float64 values to the storage type `dt`, returned as float64 (bf16: dropout_ref.bf16_round's rounding in 32-bit words, for
    finite values well below the largest -- test_gemm_ref.py holds the two to each other)"""
    a32 = np.asarray(a, np.float32)
    if dt == "bf16":
        u = a32.view(np.uint32)
        a32 = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return a32.astype(np.float64)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def draw(rng, shape, dt, which):
    if which == "int":
        return rng.integers(-3, 4, size=shape, dtype=np.int8).astype(np.float64)
    return q(rng.standard_normal(shape, dtype=np.float32), dt)


def bar(ref, S, n, dout):
    b = S * ((n + 2) * EPS)
    if dout == "bf16":
        b += 2.0 ** -8 * np.abs(ref)
    return b


def worst_ratio(got, ref, b):
    """(every element within its bar, the largest |got - ref| / bar); a zero bar asks for equality; a NaN fails"""
    err = np.abs(got - ref)
    ok = bool((err <= b).all())
    if (b > 0).all():
        r = np.divide(err, b, out=err)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    return ok, float(np.nanmax(r)) if r.size and not np.isnan(r).all() else float("nan")


# ================================================================================================================= NT cases
@dataclass(frozen=True)
class NT:
    kernel: str                 # what the table claims: "tile", "rows", "glds" or "strip<MB>.<EPI>"
    din: str
    dout: str
    M: int
    N: int
    K: int
    tag: str = ""
    pa: int = 0                 # lda - K, ldb - K, ldc - N
    pb: int = 0
    pc: int = 0
    coff: int = 0               # elements C sits off 16-byte alignment
    bias: int = 0               # 0 none, 1 aligned, 2 one element (4 bytes) off alignment
    acc: int = 0
    splits: int = 1
    slabs: int = 1              # what `splits` recomputes to
    entry: str = "nt"           # "nt", "grouped", "drop", "pool"
    rg: int = 0
    gs: int = 0
    roff: int = 0
    b2: int = 0                 # 2-D bias: 0 none, 1 aligned, 2 one element off
    pw: int = 0
    pdt: str = "bf16"           # dtype of the pool operand
    p: float = 0.0              # dropout probability of the normal set (the integer set runs 0.5)
    reserved: int = 0
    sets: str = "IN"            # which input sets run: I(nt), N(ormal)

    @property
    def lda(self):
        return self.K + self.pa

    @property
    def ldb(self):
        return self.K + self.pb

    @property
    def ldc(self):
        return self.N + self.pc

    @property
    def out_rows(self):
        """rows of the output buffer"""
        return self.M if self.rg == 0 else cdiv(self.M, self.rg) * self.gs

    def p_of(self, which):
        return 0.0 if self.p == 0 else (0.5 if which == "int" else self.p)


def nt_id(c):
    s = f"{c.kernel}-{c.din}-{c.dout}-{c.M}x{c.N}x{c.K}"
    for name, v in (("pa", c.pa), ("pb", c.pb), ("pc", c.pc), ("coff", c.coff), ("bias", c.bias), ("acc", c.acc), ("splits", c.splits - 1 and c.splits), ("rg", c.rg), ("gs", c.gs),
                    ("roff", c.roff), ("b2", c.b2), ("pw", c.pw), ("p", c.p), ("res", c.reserved)):
        if v:
            s += f"-{name}{v}"
    if c.pw and c.pdt != "bf16":
        s += "-pool32"
    return s + (f"-{c.tag}" if c.tag else "")


def nt_case_plan(c, which="normal"):
    lo = lambda off, es: (off * es) % 16
    return nt_plan(CODE[c.din], CODE[c.dout], c.M, c.N, c.K, c.lda, c.ldb, c.ldc, 0, 0, lo(c.coff, ES[c.dout]), -1 if not c.bias else lo(c.bias - 1, 4),
                   c.acc, c.splits, 0 if c.splits > 1 else -1, c.rg, -1 if not c.b2 else lo(c.b2 - 1, 4), int(c.pw > 0), c.pw, int(c.pdt == "bf16"),
                   int(c.p_of(which) > 0), c.reserved)


def nt_plan_name(pl):
    return f"strip{pl['mb']}.{pl['epi']}" if pl["kernel"] == "strip" else pl["kernel"]


def nt_census(pl):
    if pl["kernel"] == "rows":
        return {"gemm_rows": 1}
    if pl["kernel"] == "strip":
        return {("gemm_strip", "gemm_strip_acc", "gemm_strip_pool", "gemm_strip_pool")[pl["epi"]]: 1}
    return {}


DTS = (("bf16", "bf16"), ("bf16", "fp32"), ("fp32", "fp32"), ("fp32", "bf16"))


def _tile_cases():
    out = []
    for din, dout in DTS:
        for M, N, K in ((5, 12, 8), (129, 130, 72), (257, 36, 200)):
            out.append(NT("tile", din, dout, M, N, K))
        out.append(NT("tile", din, dout, 129, 130, 72, pa=8, pb=8, pc=8))                 # every leading dimension above its extent
        out.append(NT("tile", din, dout, 129, 136, 72, bias=1, acc=1))                     # the 8-wide store with bias and the old C
    for din in ("bf16", "fp32"):
        ch = 8 if din == "bf16" else 4
        for chunks in range(1, 17):                                                        # the K tail at every chunk count mod 8, one and two K-tiles
            if (5, 12, chunks * ch) != (5, 12, 8):
                out.append(NT("tile", din, "fp32", 5, 12, chunks * ch))
        out += [NT("tile", din, "fp32", 1, 1, 2 * ch), NT("tile", din, "bf16", 1, 13, 2 * ch), NT("tile", din, "fp32", 13, 1, 2 * ch)]
    for dout in ("fp32", "bf16"):
        out.append(NT("tile", "bf16", dout, 129, 136, 72, coff=1, bias=1, tag="c-off"))   # C one element off: the element-wide store
        out.append(NT("tile", "bf16", dout, 129, 136, 72, bias=2, tag="bias-off"))        # bias 4 bytes off: the element-wide store as well
        out.append(NT("tile", "bf16", dout, 129, 136, 72, coff=1, bias=2, acc=1))
        out.append(NT("tile", "bf16", dout, 129, 130, 72, acc=1, bias=1))                  # N % 8 != 0: a ragged last column group
    out.append(NT("tile", "bf16", "bf16", 129, 136, 72, pc=4, bias=1))                     # ldc % 8 != 0 with bf16 out
    out.append(NT("tile", "bf16", "fp32", 129, 136, 72, pc=2, acc=1))                      # ldc % 4 != 0 with fp32 out
    out.append(NT("tile", "bf16", "fp32", 129, 136, 72, pc=4, acc=1))                      # ldc % 8 == 4 with fp32 out: still the 8-wide store
    # more than 8 column tiles: tile_coords walks groups of 8 row tiles column by column, the last group (2 row tiles) short
    out.append(NT("tile", "bf16", "bf16", 9 * 128 + 5, 9 * 128 + 8, 72, bias=1))
    out.append(NT("tile", "fp32", "fp32", 9 * 128 + 5, 9 * 128 + 8, 8))
    return out


def _rows_cases():
    out = [NT("rows", "bf16", "fp32", 225, 257, 16), NT("rows", "bf16", "bf16", 225, 257, 16, bias=1),
           NT("rows", "bf16", "bf16", 256, 256, 528, tag="64-tiles"), NT("tile", "bf16", "bf16", 224, 288, 528, tag="63-tiles"),
           NT("rows", "bf16", "fp32", 225, 257, 528, bias=1, acc=1),                       # 33 k-steps: not a multiple of the 32-step batch
           NT("rows", "bf16", "bf16", 225, 260, 1536, acc=1), NT("tile", "bf16", "bf16", 225, 260, 1544, tag="K-past-1536"),
           NT("rows", "bf16", "bf16", 2048, 64, 528, bias=1), NT("tile", "bf16", "bf16", 2049, 64, 528, bias=1),
           NT("rows", "bf16", "bf16", 1024, 1024, 16, tag="1024-tiles"), NT("tile", "bf16", "bf16", 1025, 1024, 16, tag="1056-tiles"),
           NT("tile", "bf16", "bf16", 225, 257, 24, tag="K-not-16"),
           NT("rows", "bf16", "fp32", 225, 260, 64, pc=4, acc=1), NT("rows", "bf16", "fp32", 225, 260, 64, pc=2, bias=1),
           NT("rows", "bf16", "bf16", 225, 260, 64, pc=4, bias=1), NT("rows", "bf16", "bf16", 225, 260, 64, pc=2, acc=1),
           NT("rows", "bf16", "bf16", 225, 260, 64, pa=8, pb=16, coff=1, bias=2, tag="c-off"),
           NT("rows", "bf16", "bf16", 225, 258, 64, acc=1, bias=1)]
    return out


def _glds_cases():
    out = [NT("glds", "bf16", "bf16", 130, 136, 1088), NT("glds", "bf16", "fp32", 130, 136, 1088, bias=1, acc=1),
           NT("glds", "bf16", "bf16", 130, 136, 1088, pa=8, pb=16, pc=8, bias=1, acc=1),
           NT("glds", "bf16", "bf16", 130, 136, 2304, splits=2, slabs=2, bias=1), NT("glds", "bf16", "fp32", 130, 133, 2304, splits=2, slabs=2, acc=1, pc=3),
           NT("tile", "bf16", "bf16", 130, 136, 1024, tag="K-1024"), NT("tile", "bf16", "bf16", 130, 136, 1096, tag="K-not-64"),
           NT("glds", "bf16", "bf16", 130, 136, 1088, entry="grouped", rg=13, gs=15, roff=1, b2=1, bias=1),
           NT("glds", "bf16", "fp32", 130, 136, 1088, entry="grouped", rg=13, gs=15, roff=1, b2=2),
           NT("glds", "bf16", "bf16", 130, 96, 1088, entry="pool", pw=12, sets="N"), NT("glds", "bf16", "fp32", 130, 96, 1088, entry="pool", pw=8, pdt="fp32")]
    return out


def _splitk_cases():
    out = []
    flags = {2: dict(dout="fp32", bias=1), 3: dict(dout="bf16", acc=1), 4: dict(dout="fp32", bias=1, acc=1, pc=8), 5: dict(dout="bf16", bias=1, pc=3),
             7: dict(dout="fp32", acc=1, pc=3)}
    for s, kw in flags.items():
        for N in (24, 27):       # the 4-column branch of the reduce and its scalar branch
            out.append(NT("tile", "bf16", kw["dout"], 37, N, 64 * s, splits=s, slabs=s, **{k: v for k, v in kw.items() if k != "dout"}))
    out.append(NT("tile", "bf16", "bf16", 37, 24, 64, splits=4, slabs=1, bias=1, tag="collapses"))       # K = 64, splits = 4: one slab, no reduce
    out.append(NT("tile", "fp32", "fp32", 37, 24, 96, splits=3, slabs=3, bias=1))
    out.append(NT("tile", "bf16", "fp32", 130, 264, 200, splits=3, slabs=2, acc=1, tag="ragged-slab"))    # slabs of 128 and 72
    return out


def _strip_cases():
    S = lambda mb, epi, M, N, K=128, **kw: NT(f"strip{mb}.{epi}", "bf16", "bf16", M, N, K, **kw)
    out = [S(4, 0, 8192, 2048), S(2, 0, 8192, 1024, bias=1), S(3, 0, 12288, 1024, bias=2),              # (a bias 4 bytes off is still the strip)
           S(4, 1, 8192, 2048, acc=1, bias=1), S(2, 1, 8192, 1024, acc=1), S(3, 1, 12288, 1024, acc=1, pc=8, pa=8, pb=8),
           S(4, 2, 8192, 2048, entry="pool", pw=8), S(2, 2, 8192, 1024, entry="pool", pw=16), S(3, 2, 12288, 1024, entry="pool", pw=8, pc=8),
           # the two-window epilogue needs a window of at least 8 that is no multiple of 8 (24 is one: it takes epilogue 2) and divides N
           S(4, 3, 10240, 1536, entry="pool", pw=12, sets="N"), S(2, 3, 8192, 768, entry="pool", pw=12, sets="N"),
           S(3, 3, 8192, 1280, entry="pool", pw=20, sets="N", pc=8), S(2, 2, 8192, 768, entry="pool", pw=24, sets="N"),
           # a remainder (rem != 0) and M not a multiple of 32
           S(2, 0, 8359, 1024, K=256, bias=1), S(3, 1, 9000, 1536, acc=1), S(2, 2, 8359, 1024, entry="pool", pw=16),
           S(3, 3, 9000, 1536, entry="pool", pw=12, sets="N"),
           S(2, 0, 8192, 1024, pc=8, tag="ldc"), NT("tile", "bf16", "bf16", 8192, 1024, 128, pc=4, tag="ldc-falls-through"),
           NT("tile", "bf16", "bf16", 8192, 1024, 128, coff=1, tag="c-off-falls-through"),
           NT("tile", "bf16", "bf16", 8191, 1024, 128, tag="M-below-8192"), NT("tile", "bf16", "bf16", 8192, 1024, 64, tag="K-below-128"),
           NT("tile", "bf16", "bf16", 8192, 256, 128, tag="refused-padding"),
           NT("tile", "bf16", "fp32", 8192, 1024, 128, tag="fp32-out"),
           NT("tile", "bf16", "bf16", 8192, 1024, 128, entry="pool", pw=8, pdt="fp32", tag="fp32-pool-operand"),
           # 16 reserved CUs: fewer row groups (a remainder appears; at 9000 x 1536 the wave-row height changes from 3 to 4)
           S(2, 0, 8192, 1024, reserved=16), S(3, 1, 12288, 1024, acc=1, reserved=16), S(4, 0, 9000, 1536, bias=1, reserved=16)]
    return out


def _pool_cases():
    out = []
    for din, dout in DTS:
        out.append(NT("tile", din, dout, 300, 96, 64, entry="pool", pw=12, pdt="fp32", sets="N"))        # a window that 8 columns straddle
        out.append(NT("tile", din, dout, 300, 96, 64, entry="pool", pw=8, pdt="bf16"))
    out += [NT("tile", "bf16", "bf16", 300, 96, 64, entry="pool", pw=4, pdt="bf16", pc=8), NT("tile", "bf16", "bf16", 300, 100, 64, entry="pool", pw=20, sets="N"),
            NT("tile", "bf16", "fp32", 300, 96, 64, entry="pool", pw=24, coff=1, sets="N"), NT("tile", "bf16", "fp32", 300, 96, 64, entry="pool", pw=16, coff=1)]
    return out


def _grouped_cases():
    G = lambda din, dout, M, N, K, **kw: NT("tile", din, dout, M, N, K, **{"entry": "grouped", **kw})
    out = [G("bf16", "bf16", 50, 64, 48, rg=16, gs=17, roff=1, b2=1, bias=1), G("fp32", "fp32", 50, 64, 48, rg=16, gs=16, roff=0, b2=1),
           G("bf16", "fp32", 50, 64, 48, rg=16, gs=19, roff=1, b2=2, bias=1), G("fp32", "bf16", 50, 60, 48, rg=7, gs=9, roff=2, b2=1),
           G("bf16", "bf16", 50, 64, 48, rg=16, gs=17, roff=1, pc=8), G("bf16", "bf16", 200, 136, 48, rg=64, gs=65, roff=1, b2=2, coff=1)]
    for p in (0.5, 0.25):
        out.append(G("bf16", "bf16", 200, 64, 48, entry="drop", rg=64, gs=65, roff=1, b2=1, bias=1, p=p))
        out.append(G("fp32", "fp32", 200, 64, 48, entry="drop", rg=64, gs=65, roff=1, b2=1, p=p))
        # N = 12, fp32 out: ldc * 4 is a multiple of 16, so columns 0..7 take the 8-wide store; output row 341 starts at flat index 4092 and
        # its columns 4..7 lie in the next 4096-element block of the mask
        out.append(G("bf16", "fp32", 352, 12, 48, entry="drop", rg=16, gs=17, roff=1, b2=1, p=p, tag="key-boundary"))
        out.append(G("fp32", "fp32", 352, 12, 48, entry="drop", rg=16, gs=17, roff=1, bias=1, p=p, tag="key-boundary"))
        out.append(G("bf16", "bf16", 352, 12, 48, entry="drop", rg=16, gs=17, roff=1, p=p, tag="scalar-store"))
    out.append(G("bf16", "bf16", 200, 64, 48, entry="drop", rg=64, gs=65, roff=1, b2=1, tag="p0"))
    return out


NT_TABLES = dict(tile=_tile_cases(), rows=_rows_cases(), glds=_glds_cases(), splitk=_splitk_cases(), strip=_strip_cases(), pool=_pool_cases(),
                 grouped=_grouped_cases())
NT_CASES = [c for t in NT_TABLES.values() for c in t]
NT_RUNS = [(c, w) for c in NT_CASES for w in ("int", "normal") if w[0].upper() in c.sets]


def nt_run_id(run):
    return f"{nt_id(run[0])}-{run[1]}"


def nt_chain(c, which):
    """fp32 additions on an element's longest chain"""
    return c.K + c.slabs + (1 if c.bias else 0) + (1 if c.b2 else 0) + (2 if c.pw else 0) + (2 if c.p_of(which) > 0 else 0) + (1 if c.acc else 0)


def nt_exact_ok(c):
    """the integer set is exact in float32: every partial sum, scaled to an integer, stays below 2^24"""
    terms = 9 * c.K + 3 * (1 if c.bias else 0) + 3 * (1 if c.b2 else 0) + (3 if c.pw else 0)
    scale = c.pw if c.pw else 1
    return (c.pw == 0 or c.pw & (c.pw - 1) == 0) and (terms * 2 + 3) * scale < 2 ** 24


_nt_cache = {}


def nt_inputs(c, which):
    """dict of float64 storage-exact operands: A [M, K], B [N, K], bias [N], bias2d [rg, N], pool [M, N / pw], old [M, N] (accumulate)"""
    key = (c, which)
    d = _nt_cache.get(key)
    if d is None:
        rng = rng_of(nt_id(c), which)
        d = dict(A=draw(rng, (c.M, c.K), c.din, which), B=draw(rng, (c.N, c.K), c.din, which))
        if c.bias:
            d["bias"] = draw(rng, (c.N,), "fp32", which)
        if c.b2:
            d["bias2d"] = draw(rng, (c.rg, c.N), "fp32", which)
        if c.pw:
            d["pool"] = draw(rng, (c.M, c.N // c.pw), c.pdt, which)
        if c.acc:
            d["old"] = draw(rng, (c.M, c.N), c.dout, which)
        p = c.p_of(which)
        v, S, kept = R.nt(d["A"], d["B"], d.get("bias"), d.get("bias2d"), c.rg, c.gs, c.roff, d.get("pool"), c.pw, d.get("old"),
                          (SEED, p) if p > 0 else None, c.ldc, scale=which != "int")
        d.update(ref=v, S=S, kept=kept)
        if len(_nt_cache) > 4:
            _nt_cache.clear()
        _nt_cache[key] = d
    return d


def padded(a, ld, extra_rows=2):
    """[rows + extra_rows, ld]: `a` in the leading columns, NaN in the gap columns and in the rows that follow"""
    out = np.full((a.shape[0] + extra_rows, ld), np.nan)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def nt_c_initial(c, which):
    """the output buffer before the call, [out_rows, ldc]: NaN where a value is due (the old C with accumulate), NaN in rows the call must
    not touch, the sentinel in the gap columns"""
    buf = np.full((c.out_rows, c.ldc), np.nan)
    buf[:, c.N:] = SENT
    if c.acc:
        buf[R.out_rows(c.M, c.rg, c.gs, c.roff), :c.N] = nt_inputs(c, which)["old"]
    return buf


def nt_judge(c, which, got):
    """got: the output buffer after the call, float64 [out_rows, ldc].  Returns (ok, worst ratio, message)"""
    d = nt_inputs(c, which)
    rows = R.out_rows(c.M, c.rg, c.gs, c.roff)
    if not (got[:, c.N:] == SENT).all():
        return False, np.inf, "gap columns written"
    untouched = np.ones(c.out_rows, bool)
    untouched[rows] = False
    if not np.isnan(got[untouched, :c.N]).all():
        return False, np.inf, "a row outside the row map was written"
    val = got[:, :c.N] if c.rg == 0 else got[rows, :c.N]
    if np.isnan(val).any():
        return False, np.inf, f"{int(np.isnan(val).sum())} elements left unwritten or NaN"
    if c.p_of(which) > 0 and not np.array_equal(val != 0, d["kept"] & (d["ref"] != 0)):
        return False, np.inf, "the kept / dropped pattern differs from the predicted mask"
    if which == "int":
        want = q(d["ref"], c.dout)
        bad = int((val != want).sum())
        return bad == 0, 0.0 if bad == 0 else np.inf, f"{bad} elements differ from the exact result"
    ok, worst = worst_ratio(val, d["ref"], bar(d["ref"], d["S"], nt_chain(c, which), c.dout))
    return ok, worst, "outside the bar"


# ================================================================================================================= TN cases
@dataclass(frozen=True)
class TN:
    kernel: str                 # "tile1", "tile3", "wide" or "tall"
    dout: str
    M: int
    N: int
    K: int
    tag: str = ""
    pa: int = 0                 # lda - M, ldb - N, ldc - N
    pb: int = 0
    pc: int = 0
    coff: int = 0
    acc: int = 0
    splits: int = 1
    slabs: int = 1
    folds: tuple = ()           # (parts, nsum, n) per fold job riding in the call (spv_gemm_tn_fold)

    @property
    def lda(self):
        return self.M + self.pa

    @property
    def ldb(self):
        return self.N + self.pb

    @property
    def ldc(self):
        return self.N + self.pc


def tn_id(c):
    s = f"{c.kernel}-{c.dout}-{c.M}x{c.N}x{c.K}"
    for name, v in (("pa", c.pa), ("pb", c.pb), ("pc", c.pc), ("coff", c.coff), ("acc", c.acc), ("splits", c.splits - 1 and c.splits), ("folds", len(c.folds))):
        if v:
            s += f"-{name}{v}"
    return s + (f"-{c.tag}" if c.tag else "")


def tn_case_plan(c):
    return tn_plan(CODE[c.dout], c.M, c.N, c.K, c.lda, c.ldb, c.ldc, 0, 0, c.splits, 0 if c.splits > 1 else -1, fold_blocks(c.folds))


def tn_census(pl):
    return {"gemm_tn": 1, **({"gemm_tn_wide": 1} if pl["kernel"] == "wide" else {})}


FOLDS_A = ((1, 1, 40), (300, 5, 40), (33, 3, 8))       # parts 1 and many (past the 8 x 32 unrolled loop), nsum 1 and 5, n no multiple of 32
FOLDS_17 = tuple((1 + 19 * j, 1 + j % 5, 8 + 5 * j) for j in range(17))     # spv_fold_multi: two launches


def _tn_cases():
    T = TN
    out = [T("tile1", "fp32", 8, 16, 40), T("tile1", "bf16", 264, 48, 100, acc=1), T("tile1", "fp32", 264, 48, 100, pa=8, pb=16, pc=3),
           T("tile1", "fp32", 264, 64, 200, splits=3, slabs=2, acc=1), T("tile3", "fp32", 264, 72, 200, tag="N-past-64")]
    # depth 3: nfull = 0..4 full K-tiles of a slice, with and without a partial one behind them
    for K in (40, 64, 100, 128, 192, 230, 256, 300):
        out.append(T("tile3", "fp32", 264, 136, K))
    out += [T("tile3", "bf16", 264, 136, 300), T("tile3", "bf16", 264, 136, 300, acc=1, pa=8, pb=8, pc=8),
            T("tile3", "fp32", 264, 136, 300, acc=1, pc=4, coff=1), T("tile3", "fp32", 264, 136, 300, splits=3, slabs=3, acc=1),
            T("tile3", "bf16", 264, 136, 300, splits=5, slabs=5, pc=8), T("tile3", "fp32", 264, 136, 300, splits=5, slabs=5, pa=8, pb=8),
            T("tile3", "bf16", 264, 136, 64, splits=4, slabs=1, tag="collapses"),
            T("tile3", "fp32", 136, 1032, 72, tag="m-fast"), T("tile3", "fp32", 136, 1032, 200, splits=2, slabs=2, tag="m-fast"),
            # folds: riding a reduce, and alone
            T("tile3", "fp32", 264, 136, 300, splits=3, slabs=3, folds=FOLDS_A), T("tile3", "bf16", 264, 136, 300, folds=FOLDS_A),
            T("tile1", "fp32", 8, 16, 40, folds=FOLDS_A[:1])]
    # wide: >= 4 slabs, M % 256 == 0, N % 128 == 0 and at least 128 workgroups
    out += [T("wide", "fp32", 512, 512, 1000, splits=16, slabs=16), T("wide", "bf16", 512, 512, 1024, splits=16, slabs=16, acc=1),
            T("wide", "fp32", 512, 512, 1024, splits=16, slabs=16, acc=1, pa=8, pb=8, pc=8), T("wide", "bf16", 256, 128, 8192, splits=128, slabs=128),
            T("tile3", "fp32", 256, 128, 8128, splits=127, slabs=127, tag="127-workgroups"),
            T("tile3", "fp32", 512, 520, 1024, splits=16, slabs=16, tag="N-not-128"), T("tile3", "fp32", 264, 512, 1024, splits=16, slabs=16, tag="M-not-256"),
            T("wide", "fp32", 512, 512, 1024, splits=16, slabs=16, folds=FOLDS_A)]
    # tall: M = 512, N a multiple of 128 from 1024 up, at least 192 workgroups, slices of at least 512 rows
    out += [T("tall", "fp32", 512, 1024, 12280, splits=24, slabs=24), T("tall", "bf16", 512, 1024, 12288, splits=24, slabs=24, acc=1),
            T("tall", "fp32", 512, 1024, 12288, splits=24, slabs=24, acc=1, pb=8, pc=8), T("tall", "bf16", 512, 3072, 4096, splits=8, slabs=8, pb=8),
            T("wide", "fp32", 512, 1024, 11776, splits=23, slabs=23, tag="184-workgroups")]
    return out


TN_CASES = _tn_cases()
TN_RUNS = [(c, w) for c in TN_CASES for w in ("int", "normal")]


def tn_run_id(run):
    return f"{tn_id(run[0])}-{run[1]}"


_tn_cache = {}


def fold_inputs(jobs, key, which):
    """per job: (partials [parts, nsum, n] float64 storage-exact fp32, value [nsum, n], S)"""
    rng = rng_of("folds", key, which)
    out = []
    for parts, nsum, n in jobs:
        pt = draw(rng, (parts, nsum, n), "fp32", which)
        out.append((pt,) + R.fold(pt))
    return out


def tn_inputs(c, which):
    key = (c, which)
    d = _tn_cache.get(key)
    if d is None:
        rng = rng_of(tn_id(c), which)
        d = dict(A=draw(rng, (c.K, c.M), "bf16", which), B=draw(rng, (c.K, c.N), "bf16", which))
        if c.acc:
            d["old"] = draw(rng, (c.M, c.N), c.dout, which)
        d["ref"], d["S"] = R.tn(d["A"], d["B"], None, d.get("old"))
        d["folds"] = fold_inputs(c.folds, tn_id(c), which)
        if len(_tn_cache) > 2:
            _tn_cache.clear()
        _tn_cache[key] = d
    return d


def tn_c_initial(c, which):
    buf = np.full((c.M, c.ldc), np.nan)
    buf[:, c.N:] = SENT
    if c.acc:
        buf[:, :c.N] = tn_inputs(c, which)["old"]
    return buf


def dense_judge(which, got, N, ref, S, chain, dout):
    """got [rows, ldc] against ref [rows, N]: gap columns untouched, every element written, exact (int) or within the bar (normal)"""
    if not (got[:, N:] == SENT).all():
        return False, np.inf, "gap columns written"
    val = got[:, :N]
    if np.isnan(val).any():
        return False, np.inf, f"{int(np.isnan(val).sum())} elements left unwritten or NaN"
    if which == "int":
        bad = int((val != q(ref, dout)).sum())
        return bad == 0, 0.0 if bad == 0 else np.inf, f"{bad} elements differ from the exact result"
    ok, worst = worst_ratio(val, ref, bar(ref, S, chain, dout))
    return ok, worst, "outside the bar"


def tn_judge(c, which, got):
    d = tn_inputs(c, which)
    return dense_judge(which, got, c.N, d["ref"], d["S"], c.K + c.slabs + c.acc, c.dout)


def fold_judge(which, got, value, S, parts):
    """got, value [nsum, n]: a fold is a sum of `parts` terms"""
    return dense_judge(which, got, got.shape[1], value, S, parts, "fp32")


def fold_exact_ok(jobs):
    return all(3 * parts < 2 ** 24 for parts, _, _ in jobs)


# ============================================================================================================ TN batch cases
@dataclass(frozen=True)
class TNB:
    kernel: str                 # "batch128" or "batch_wide"
    K: int
    splits: int
    slabs: int
    probs: tuple                # (m, n, pa, pb, pc, k) per problem; k = 0: the call's K
    tag: str = ""
    folds: tuple = ()


def tnb_id(c):
    return f"{c.kernel}-K{c.K}-s{c.splits}-" + "_".join(f"{m}x{n}k{k}" + (f"p{pa}.{pb}.{pc}" if pa or pb or pc else "") for m, n, pa, pb, pc, k in c.probs) + \
        (f"-folds{len(c.folds)}" if c.folds else "") + (f"-{c.tag}" if c.tag else "")


def tnb_probs(c):
    return [dict(m=m, n=n, lda=m + pa, ldb=n + pb, ldc=n + pc, k=k) for m, n, pa, pb, pc, k in c.probs]


def tnb_case_plan(c):
    return tnb_plan(tnb_probs(c), c.K, c.splits, 0, fold_blocks(c.folds))


def tnb_census(pl):
    return {"gemm_tn": 1, "gemm_tn_batch": 1, **({"gemm_tn_wide": 1} if pl["kernel"] == "batch_wide" else {})}


TNB_CASES = [
    TNB("batch128", 200, 3, 2, ((136, 72, 0, 0, 0, 0),), tag="one-long"),
    # eight problems: three long ones around short ones with k = 1, 63, 64, 65 and K - 1; five short tiles are padded to 8 workgroups
    TNB("batch128", 200, 3, 2, ((136, 72, 0, 0, 0, 0), (8, 264, 0, 0, 0, 1), (264, 8, 8, 8, 3, 200), (16, 16, 0, 0, 0, 63), (24, 40, 8, 16, 4, 64),
                                (128, 128, 0, 0, 8, 0), (40, 24, 0, 0, 0, 65), (8, 8, 0, 0, 4, 199)), folds=FOLDS_A),
    TNB("batch128", 1536, 3, 3, ((256, 128, 0, 0, 0, 0), (256, 128, 0, 0, 0, 63)), tag="k63-not-wide"),
    TNB("batch128", 1536, 4, 4, ((256, 128, 0, 0, 0, 0), (512, 256, 0, 0, 0, 0)), tag="slices-below-512"),
    TNB("batch_wide", 1536, 3, 3, ((256, 128, 0, 0, 0, 0),), tag="one-long"),
    TNB("batch_wide", 1536, 3, 3, ((256, 128, 0, 0, 0, 64), (512, 256, 8, 8, 8, 0), (256, 128, 0, 0, 4, 65), (256, 256, 0, 0, 0, 1536), (256, 128, 8, 0, 0, 1535)),
        folds=FOLDS_A[:2]),
]
TNB_RUNS = [(c, w) for c in TNB_CASES for w in ("int", "normal")]


def tnb_run_id(run):
    return f"{tnb_id(run[0])}-{run[1]}"


def tnb_inputs(c, which):
    """per problem dict(A [K, m], B [K, n], ref, S, chain); folds as fold_inputs"""
    rng = rng_of(tnb_id(c), which)
    out = []
    for m, n, pa, pb, pc, k in c.probs:
        A, B = draw(rng, (c.K, m), "bf16", which), draw(rng, (c.K, n), "bf16", which)
        kk = c.K if k == 0 else k
        ref, S = R.tn(A, B, kk)
        out.append(dict(A=A, B=B, ref=ref, S=S, chain=kk + (c.slabs if kk == c.K else 1)))
    return out, fold_inputs(c.folds, tnb_id(c), which)
