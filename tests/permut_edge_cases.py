"""The case tables of tests/test_gpu_permut_edges.py, their seeded inputs, a Python restatement of csrc/spv_permut_core.h (the table
geometry of spv_permut_pack and the four selectors that name the kernel -- or the refusal -- of every call of spv_permut_gather_fwd,
spv_permut_gather_bwd, spv_permut_row0_fwd and spv_permut_row0_bwd) and the value bars.  Shared with tests/test_permut_ref.py, which
compiles the header with the host compiler and holds it to this restatement over a grid that straddles every threshold, asserts that
the tables stand on both sides of every boundary of every reachable path, and shows that a float32 restatement of each kernel passes
every bar on exactly these inputs while eight plausible mistakes do not.

A path is the name csrc/spv_permut_core.h's permut_path_name gives it: "fwd_pair", "bwd_dma", "refuse_pool_lds", ..."""
import zlib
from collections import namedtuple

import numpy as np

from attention_edge_cases import storage_round

DTYPES = ("fp32", "bf16")
SPV_F32, SPV_BF16 = 0, 1
CODE = {"fp32": SPV_F32, "bf16": SPV_BF16}
ES = {"fp32": 4, "bf16": 2}

# ------------------------------------------------------------------------------------------------------------------ geometry
PT = 1024
LDS_LIMIT = 150 * 1024
C_IT, MAX_IT = 5, 10
WINDOWS = (4, 8, 16, 32)


def compact_ok(d):
    return d <= 65536 and d % 8 == 0


def long_row(d):
    return d * 2 > LDS_LIMIT


def scat_parts(d):
    return (d * 4 + LDS_LIMIT - 1) // LDS_LIMIT


def scat_len(d):
    n = scat_parts(d)
    return ((d + n - 1) // n + 7) // 8 * 8


def scat_set_words(heads, d):
    total = heads * d
    return heads * (scat_parts(d) + 1) + heads * scat_parts(d) + total + (total + 1) // 2


def scat_words(heads, d):
    return 2 * scat_set_words(heads, d)


def table_words(heads, d):
    total = heads * d
    return 2 * total + (total + (total // 4 + 3) // 4 if compact_ok(d) else 0) + (scat_words(heads, d) if long_row(d) else 0)


def pool_supported(heads, d, pw, dtype):
    return int(dtype == "bf16" and long_row(d) and d % 8 == 0 and heads <= 65535 and pw > 0 and d % pw == 0 and scat_len(d) % pw == 0)


# ------------------------------------------------------------------------------------------------------------------ selectors
def fwd_path(dtype, heads, d, batch, pooled=False, pw=0, x16=True, g16=True, idx16=True):
    if batch <= 0 or heads <= 0 or d <= 0:
        return "refuse_empty"
    if dtype not in DTYPES:
        return "refuse_dtype"
    bf, es, total = dtype == "bf16", ES[dtype], heads * d
    aligned = (d * es) % 16 == 0 and total % 4 == 0
    fits = d * es <= LDS_LIMIT
    scat_pool = pooled and bf and long_row(d) and pw > 0 and d % pw == 0 and scat_len(d) % pw == 0
    if pooled and not scat_pool:
        if not (aligned and fits):
            return "refuse_pool_lds"
        if not (pw in WINDOWS and total % pw == 0 and (total // 4) % PT == 0):
            return "refuse_pool_window"
    ptrs = x16 and g16 and idx16
    if ptrs and bf and compact_ok(d) and d * 4 <= LDS_LIMIT and (not pooled or (pw in (8, 16, 32) and (total // 8) % PT == 0)):
        p = "fwd_pair"
    elif ptrs and aligned and fits:
        p = "fwd_lds"
    elif bf and long_row(d) and d % 8 == 0 and x16 and g16 and heads <= 65535 and batch <= 65535:
        p = "fwd_scatter"
    else:
        p = "fwd_global"
    return "refuse_pool_unserved" if pooled and p == "fwd_global" else p


def bwd_path(dtype, heads, d, batch, dg16=True, dx16=True, idx16=True):
    if batch <= 0 or heads <= 0 or d <= 0:
        return "refuse_empty"
    if dtype not in DTYPES:
        return "refuse_dtype"
    bf, es = dtype == "bf16", ES[dtype]
    aligned = (d * es) % 16 == 0 and d % 4 == 0
    ptrs = dg16 and dx16 and idx16
    if ptrs and bf and compact_ok(d) and (d * 2) % 1024 == 0 and d * 4 <= LDS_LIMIT and d <= 8 * PT * C_IT:
        return "bwd_dma"
    if ptrs and bf and compact_ok(d) and d * 2 <= LDS_LIMIT and d <= 8 * PT * C_IT:
        return "bwd_c16"
    if ptrs and not bf and aligned and d * es <= LDS_LIMIT and d <= 4 * PT * MAX_IT:
        return "bwd_lds"
    if bf and long_row(d) and d % 8 == 0 and dx16 and scat_len(d) * 4 <= LDS_LIMIT:
        return "bwd_scatter"
    if ptrs and bf and d % 8 == 0 and not long_row(d):
        return "bwd_parts"
    return "bwd_global"


def row0_fwd_path(dtype, batch, d, n, embed, x16=True, x016=True):
    if not (batch > 0 and d > 0 and 0 < n <= d and 0 < embed <= d):
        return "refuse_row0_shape"
    if dtype not in DTYPES:
        return "refuse_dtype"
    vec = 8 if dtype == "bf16" else 4
    return "row0_fwd_lds" if d * ES[dtype] <= LDS_LIMIT and d % vec == 0 and embed % vec == 0 and x16 and x016 else "row0_fwd_global"


def row0_bwd_path(dtype, batch, d, n, embed, dx16=True, dx016=True):
    if not (batch > 0 and d > 0 and 0 < n <= d and 0 < embed <= d and d % 8 == 0 and embed % 8 == 0):
        return "refuse_row0_shape"
    if dtype not in DTYPES:
        return "refuse_dtype"
    return "row0_bwd_lds" if d * ES[dtype] <= LDS_LIMIT and dx16 and dx016 else "row0_bwd_global"


KERNEL_PATHS = ("fwd_pair", "fwd_lds", "fwd_scatter", "fwd_global", "bwd_dma", "bwd_c16", "bwd_lds", "bwd_scatter", "bwd_parts", "bwd_global",
                "row0_fwd_lds", "row0_fwd_global", "row0_bwd_lds", "row0_bwd_global")
POOLING_PATHS = ("fwd_pair", "fwd_lds", "fwd_scatter")       # the forward kernels that can emit `pooled`
CENSUS = {"fwd_pair": {"gather_lds": 1}, "row0_fwd_lds": {"permut_row0": 1}, "row0_fwd_global": {"permut_row0": 1},
          "row0_bwd_lds": {"permut_row0": 1}, "row0_bwd_global": {"permut_row0": 1}}


def census_of(path, dtype):
    """what the source counts for a launch of `path`: gather_lds for the pair kernel and the bf16 LDS forward, permut_row0 for row 0"""
    if path == "fwd_lds":
        return {"gather_lds": 1} if dtype == "bf16" else {}
    return CENSUS.get(path, {})


# the grid tests/test_permut_ref.py sweeps: every threshold of d with its neighbours one vector (and one element) either side
D_GRID = sorted({v for t in (4, 8, 512, 1024, 2048, 4096, 38400, 40960, 65536, 76800, 115200, 151296) for v in (t - 8, t - 4, t - 1, t, t + 1, t + 2, t + 4, t + 8)
                 if v > 0} | {12, 520, 38912, 151296})
PW_GRID = (0, 3, 4, 8, 12, 16, 32, 64, 256)

# ------------------------------------------------------------------------------------------------------------------ tables
# perm: "rand" / "id" / "rev"; sign: "rand" / "pos" / "neg"; pw: 0 = no pooled output; off: the pointers that sit one 8-byte step off
# 16-byte alignment ("" = none; "x", "g", "dg", "dx", "x0", "dx0")
Pack = namedtuple("Pack", "heads d perm sign", defaults=("rand", "rand"))
Fwd = namedtuple("Fwd", "dtype batch heads d pw perm sign off", defaults=(0, "rand", "rand", ""))
Bwd = namedtuple("Bwd", "dtype batch heads d perm sign off", defaults=("rand", "rand", ""))
Row0 = namedtuple("Row0", "dtype batch d n embed off", defaults=("",))

PACK_CASES = [Pack(1 + i % 3, d) for i, d in enumerate((8, 12, 65536, 65544, 76800, 76808, 115200, 115208, 151296))] + [
    Pack(3, 8, "id", "pos"), Pack(2, 12, "rev", "neg"), Pack(2, 76808, "rev", "rand"), Pack(1, 76808, "id", "neg")]

FWD_CASES = (
    # the pair kernel: batch 1 (one sample, no partner), 2, 3 (a pair and a single)
    [Fwd("bf16", b, h, d) for d, hs in ((8, (1, 16)), (38400, (2,))) for h in hs for b in (1, 2, 3)]
    + [Fwd("bf16", 3, 3, 8, 0, "id", "pos"), Fwd("bf16", 3, 3, 8, 0, "rev", "neg"), Fwd("bf16", 2, 2, 520, 0, "rev", "rand")]
    # the LDS kernel
    + [Fwd("bf16", 2, 1, 38408), Fwd("bf16", 1, 3, 76800), Fwd("fp32", 3, 1, 4), Fwd("fp32", 2, 16, 4), Fwd("fp32", 2, 3, 38400),
       Fwd("fp32", 2, 2, 8, 0, "id", "neg"), Fwd("fp32", 2, 2, 8, 0, "rev", "pos")]
    # the scatter kernel
    + [Fwd("bf16", b, h, d) for d, h, b in ((76808, 1, 2), (115200, 2, 1), (115208, 3, 1), (151296, 2, 2))]
    + [Fwd("bf16", 1, 2, 76808, 0, "rev", "neg"), Fwd("bf16", 1, 1, 76808, 0, "id", "rand")]
    # the global kernel: fp32 off the 16-byte row (heads * d % 4 != 0 is one of these: a row of whole 16-byte pieces has d % 4 == 0),
    # fp32 over the LDS, bf16 off the 16-byte row, short and long
    + [Fwd("fp32", 2, 3, 6), Fwd("fp32", 3, 1, 1), Fwd("fp32", 2, 2, 38404), Fwd("bf16", 2, 3, 12), Fwd("bf16", 3, 1, 1), Fwd("bf16", 1, 2, 76804),
       Fwd("fp32", 1, 16, 7, 0, "rev", "neg")]
    # pooled: the pair kernel where (total / 8) % 1024 == 0, the LDS kernel otherwise (both dtypes; window 4 always)
    + [Fwd("bf16", 3, 2, 4096, pw) for pw in WINDOWS]
    + [Fwd(dt, 2, 2, 2048, pw) for dt in DTYPES for pw in WINDOWS]
    + [Fwd("fp32", 1, 2, 4096, 32), Fwd("bf16", 2, 16, 1024, 32), Fwd("bf16", 2, 3, 4096, 32), Fwd("fp32", 2, 1, 4096, 32, "id", "pos")]
    # pooled on the scatter path
    + [Fwd("bf16", 2, 2, 151296, 8), Fwd("bf16", 2, 2, 151296, 12)]
    # x or g one 8-byte step off 16-byte alignment: the global kernel
    + [Fwd(dt, 2, 2, d, 0, "rand", "rand", off) for dt, d in (("bf16", 520), ("bf16", 38408), ("fp32", 8)) for off in ("x", "g")]
    + [Fwd("bf16", 1, 1, 76808, 0, "rand", "rand", off) for off in ("x", "g")]
)
# refused: a window d admits and scat_len does not; pooled with a misaligned pointer; pooled on a row the global kernel would serve
FWD_REFUSED = [(Fwd("bf16", 2, 2, 151296, 256), "refuse_pool_lds"), (Fwd("bf16", 2, 2, 2048, 16, "rand", "rand", "x"), "refuse_pool_unserved"),
               (Fwd("fp32", 2, 2, 2048, 32, "rand", "rand", "g"), "refuse_pool_unserved"), (Fwd("bf16", 1, 2, 151296, 12, "rand", "rand", "g"), "refuse_pool_unserved"),
               (Fwd("bf16", 1, 1, 76804, 4), "refuse_pool_unserved"), (Fwd("bf16", 2, 2, 2048, 64), "refuse_pool_window"),
               (Fwd("bf16", 2, 2, 2056, 8), "refuse_pool_window"), (Fwd("fp32", 2, 2, 38404, 4), "refuse_pool_lds"), (Fwd("fp32", 2, 2, 6, 4), "refuse_pool_lds")]

BWD_CASES = (
    # the DMA kernel: min(batch, 256) workgroups, then several samples per workgroup
    [Bwd("bf16", b, h, 512) for b, h in ((1, 1), (2, 3), (257, 2), (513, 1))] + [Bwd("bf16", 3, 16, 512), Bwd("bf16", 1, 2, 38400), Bwd("bf16", 2, 1, 38400)]
    + [Bwd("bf16", 3, 2, 1024, "id", "neg"), Bwd("bf16", 3, 2, 1024, "rev", "pos")]
    + [Bwd("bf16", b, h, d) for d, h, b in ((8, 1, 3), (8, 16, 2), (520, 3, 2), (38912, 2, 1), (40960, 1, 2))]     # c16
    + [Bwd("bf16", 2, 3, 8, "rev", "neg")]
    + [Bwd("fp32", 3, 1, 4), Bwd("fp32", 2, 16, 4), Bwd("fp32", 1, 2, 38400), Bwd("fp32", 2, 3, 8, "rev", "neg"), Bwd("fp32", 2, 3, 8, "id", "pos")]   # lds<float>
    + [Bwd("bf16", 2, 2, 40968), Bwd("bf16", 1, 3, 76800)]                                                           # parts
    + [Bwd("bf16", b, h, d) for d, h, b in ((76808, 1, 2), (115200, 2, 1), (115208, 3, 1), (151296, 2, 2))]        # scatter
    + [Bwd("bf16", 1, 2, 76808, "rev", "neg")]
    + [Bwd("bf16", 2, 3, 12), Bwd("bf16", 2, 16, 7), Bwd("bf16", 1, 2, 76804), Bwd("fp32", 2, 2, 38404), Bwd("fp32", 2, 3, 6), Bwd("fp32", 1, 1, 1)]   # global
    # dg or dx off alignment: the global kernel -- but the scatter reads dg one element at a time and keeps it
    + [Bwd(dt, 2, 2, d, "rand", "rand", off) for dt, d in (("bf16", 512), ("bf16", 520), ("bf16", 40968), ("fp32", 8)) for off in ("dg", "dx")]
    + [Bwd("bf16", 1, 1, 76808, "rand", "rand", off) for off in ("dg", "dx")]
)


def _row0(dt, lds_d, over_d):
    """embed 8: the bf16 vector, and the least the backward takes in either dtype"""
    return ([Row0(dt, b, 2048, n, e) for b in (1, 3) for n, e in ((1000, 8), (1024, 8), (1032, 2048), (2048, 64), (8, 64), (24, 1024))]
            + [Row0(dt, 1, lds_d, 1032, 8), Row0(dt, 3, over_d, 1032, 8), Row0(dt, 1, over_d, 8, 1024), Row0(dt, 1, over_d, over_d, over_d)]
            + [Row0(dt, 2, 8, 8, 8), Row0(dt, 2, 2048, 1040, 8, "a"), Row0(dt, 2, 2048, 8, 64, "b")])


# off "a": x (forward) / dx (backward) misaligned; "b": x0 / dx0
ROW0_CASES = _row0("bf16", 76800, 76808) + _row0("fp32", 38400, 38408)
# forward only: d or embed off the backward's multiple of 8 (embed 4: the fp32 vector)
ROW0_FWD_ONLY = [Row0("bf16", 2, 2052, 1030, 4), Row0("fp32", 2, 38404, 1030, 4), Row0("fp32", 3, 2050, 7, 2050), Row0("bf16", 1, 2048, 3, 20),
                 Row0("fp32", 2, 2044, 1000, 4)]

ALL = dict(pack=PACK_CASES, fwd=FWD_CASES, bwd=BWD_CASES, row0=ROW0_CASES, row0_fwd=ROW0_FWD_ONLY)
for _cases in ALL.values():
    assert len(set(_cases)) == len(_cases)


def case_id(c):
    return "-".join(str(v) if v != "" else "_" for v in c)


def fwd_case_path(c):
    return fwd_path(c.dtype, c.heads, c.d, c.batch, c.pw > 0, c.pw, c.off != "x", c.off != "g")


def bwd_case_path(c):
    return bwd_path(c.dtype, c.heads, c.d, c.batch, c.off != "dg", c.off != "dx")


def row0_case_paths(c):
    return (row0_fwd_path(c.dtype, c.batch, c.d, c.n, c.embed, c.off != "a", c.off != "b"),
            row0_bwd_path(c.dtype, c.batch, c.d, c.n, c.embed, c.off != "a", c.off != "b"))


# Both sides of every boundary of every reachable path: (family, what the case must look like, the path it must take).  A `want` is a
# dict of case fields; pooled = True / False asks for pw > 0 / pw == 0.  tests/test_permut_ref.py fails if a line has no case.
BOUNDARIES = [
    # forward, no pooled
    ("fwd", dict(dtype="bf16", d=8, pooled=False), "fwd_pair"), ("fwd", dict(dtype="bf16", d=12), "fwd_global"),                   # d % 8
    ("fwd", dict(dtype="bf16", d=38400, pooled=False), "fwd_pair"), ("fwd", dict(dtype="bf16", d=38408), "fwd_lds"),               # two rows in LDS
    ("fwd", dict(dtype="bf16", d=76800), "fwd_lds"), ("fwd", dict(dtype="bf16", d=76808, pooled=False, off=""), "fwd_scatter"),   # one row in LDS
    ("fwd", dict(dtype="bf16", d=76804), "fwd_global"),
    ("fwd", dict(dtype="fp32", d=4), "fwd_lds"), ("fwd", dict(dtype="fp32", d=6), "fwd_global"),                                   # d % 4
    ("fwd", dict(dtype="fp32", d=38400), "fwd_lds"), ("fwd", dict(dtype="fp32", d=38404), "fwd_global"),
    ("fwd", dict(dtype="bf16", batch=1), "fwd_pair"), ("fwd", dict(dtype="bf16", batch=2), "fwd_pair"), ("fwd", dict(dtype="bf16", batch=3), "fwd_pair"),
    ("fwd", dict(d=115200), "fwd_scatter"), ("fwd", dict(d=115208), "fwd_scatter"), ("fwd", dict(d=151296, pooled=False), "fwd_scatter"),
    # forward, pooled
    ("fwd", dict(dtype="bf16", heads=2, d=4096, pw=8), "fwd_pair"), ("fwd", dict(dtype="bf16", heads=2, d=4096, pw=4), "fwd_lds"),     # the pair kernel has no window 4
    ("fwd", dict(dtype="bf16", heads=2, d=2048, pw=8), "fwd_lds"),                                                               # (total / 8) % 1024
    ("fwd", dict(dtype="bf16", heads=2, d=4096, pw=32), "fwd_pair"), ("fwd", dict(dtype="bf16", heads=2, d=4096, pw=16), "fwd_pair"),
    ("fwd", dict(dtype="bf16", d=151296, pw=8), "fwd_scatter"), ("fwd", dict(dtype="bf16", d=151296, pw=12), "fwd_scatter"),
    # misaligned pointers
    ("fwd", dict(dtype="bf16", d=520, off="x"), "fwd_global"), ("fwd", dict(dtype="bf16", d=520, off="g"), "fwd_global"),
    ("fwd", dict(dtype="bf16", d=38408, off="x"), "fwd_global"), ("fwd", dict(dtype="fp32", d=8, off="g"), "fwd_global"),
    ("fwd", dict(dtype="bf16", d=76808, off="x"), "fwd_global"), ("fwd", dict(dtype="bf16", d=76808, off="g"), "fwd_global"),
    # backward
    ("bwd", dict(d=512, batch=1), "bwd_dma"), ("bwd", dict(d=512, batch=2), "bwd_dma"), ("bwd", dict(d=512, batch=257), "bwd_dma"),
    ("bwd", dict(d=512, batch=513), "bwd_dma"), ("bwd", dict(dtype="bf16", d=520, off=""), "bwd_c16"),                              # d % 512
    ("bwd", dict(d=38400, dtype="bf16"), "bwd_dma"), ("bwd", dict(d=38912), "bwd_c16"),                                            # two slices in LDS
    ("bwd", dict(d=40960), "bwd_c16"), ("bwd", dict(d=40968, off=""), "bwd_parts"),                                               # C_IT
    ("bwd", dict(d=76800), "bwd_parts"), ("bwd", dict(d=76808, off=""), "bwd_scatter"),                                           # one row in LDS
    ("bwd", dict(dtype="bf16", d=8), "bwd_c16"), ("bwd", dict(dtype="bf16", d=12), "bwd_global"), ("bwd", dict(dtype="bf16", d=76804), "bwd_global"),
    ("bwd", dict(dtype="fp32", d=4), "bwd_lds"), ("bwd", dict(dtype="fp32", d=6), "bwd_global"),
    ("bwd", dict(dtype="fp32", d=38400), "bwd_lds"), ("bwd", dict(dtype="fp32", d=38404), "bwd_global"),
    ("bwd", dict(d=115200), "bwd_scatter"), ("bwd", dict(d=115208), "bwd_scatter"), ("bwd", dict(d=151296), "bwd_scatter"),
    ("bwd", dict(d=512, off="dg"), "bwd_global"), ("bwd", dict(d=512, off="dx"), "bwd_global"), ("bwd", dict(d=520, off="dg"), "bwd_global"),
    ("bwd", dict(d=520, off="dx"), "bwd_global"), ("bwd", dict(d=40968, off="dg"), "bwd_global"), ("bwd", dict(d=40968, off="dx"), "bwd_global"),
    ("bwd", dict(dtype="fp32", d=8, off="dg"), "bwd_global"), ("bwd", dict(dtype="fp32", d=8, off="dx"), "bwd_global"),
    ("bwd", dict(d=76808, off="dg"), "bwd_scatter"), ("bwd", dict(d=76808, off="dx"), "bwd_global"),
] + [line for h in (1, 2, 3, 16) for line in (("fwd", dict(heads=h), None), ("bwd", dict(heads=h), None))] + [
    # row 0: (forward path, backward path)
    ("row0", dict(dtype="bf16", d=76800), ("row0_fwd_lds", "row0_bwd_lds")), ("row0", dict(dtype="bf16", d=76808), ("row0_fwd_global", "row0_bwd_global")),
    ("row0", dict(dtype="fp32", d=38400), ("row0_fwd_lds", "row0_bwd_lds")), ("row0", dict(dtype="fp32", d=38408), ("row0_fwd_global", "row0_bwd_global")),
    ("row0_fwd", dict(dtype="fp32", d=38404), ("row0_fwd_global",)), ("row0_fwd", dict(dtype="bf16", d=2052), ("row0_fwd_global",)),
    ("row0_fwd", dict(dtype="bf16", embed=20), ("row0_fwd_global",)), ("row0_fwd", dict(dtype="fp32", embed=2050), ("row0_fwd_global",)),
    ("row0_fwd", dict(dtype="fp32", embed=4, d=2044), ("row0_fwd_lds",)),
] + [("row0", dict(dtype=dt, **kw), None) for dt in DTYPES for kw in (
    dict(n=1000), dict(n=1024), dict(n=1032), dict(batch=1), dict(batch=3), dict(embed=8), dict(off="a"), dict(off="b"))
] + [("row0", dict(dtype=dt, d=2048, embed=2048), ("row0_fwd_lds", "row0_bwd_lds")) for dt in DTYPES]


def matches(c, want):
    for k, v in want.items():
        if k == "pooled":
            if (c.pw > 0) != v:
                return False
        elif getattr(c, k) != v:
            return False
    return True


def path_of(family, c):
    return {"fwd": fwd_case_path, "bwd": bwd_case_path, "row0": row0_case_paths, "row0_fwd": lambda k: row0_case_paths(k)[:1]}[family](c)


# ------------------------------------------------------------------------------------------------------------------ inputs
def rng_of(c, tag=""):
    return np.random.default_rng(zlib.crc32(f"{type(c).__name__}/{case_id(c)}/{tag}".encode()))


def perms_signs(rng, heads, d, perm="rand", sign="rand"):
    """perms int64 [heads, d], signs float32 [heads, d] in {-1, +1}"""
    if perm == "id":
        p = np.tile(np.arange(d, dtype=np.int64), (heads, 1))
    elif perm == "rev":
        p = np.tile(np.arange(d, dtype=np.int64)[::-1], (heads, 1))
    else:
        p = np.stack([rng.permutation(d).astype(np.int64) for _ in range(heads)])
    s = {"pos": np.ones((heads, d)), "neg": -np.ones((heads, d))}.get(sign)
    if s is None:
        s = np.where(rng.random((heads, d)) < 0.5, -1.0, 1.0)
    return np.ascontiguousarray(p), s.astype(np.float32)


TINY = {"bf16": 2.0 ** -133, "fp32": 2.0 ** -149}         # the smallest subnormal of the storage type
HUGE = {"bf16": float(np.float32(3.3895313892515355e38)), "fp32": float(np.finfo(np.float32).max)}   # the largest finite value
PLANTS = ("+0", "-0", "+tiny", "-tiny", "+inf", "-inf", "huge")


def values(rng, shape, dtype, plant=True):
    """standard normals rounded to the storage type with +-0, +-subnormal, +-inf and the largest finite value planted at seeded places
    (as many of them as a tenth of the elements allows: the gather copies, so every one of them must come out bit for bit); read-only"""
    a = storage_round(rng.standard_normal(shape), dtype).reshape(-1)
    assert bool((a != 0).all())
    if plant:
        vals = np.array([0.0, -0.0, TINY[dtype], -TINY[dtype], np.inf, -np.inf, HUGE[dtype]])
        k = min(len(vals), a.size // 10)
        where = rng.permutation(a.size)[:k]
        a[where] = vals[rng.permutation(len(vals))[:k]]
    a = a.reshape(shape)
    a.setflags(write=False)
    return a


def pack_inputs(c):
    return perms_signs(rng_of(c), c.heads, c.d, c.perm, c.sign)


def fwd_inputs(c):
    """(perms, signs, x [batch, d])"""
    rng = rng_of(c)
    perms, signs = perms_signs(rng, c.heads, c.d, c.perm, c.sign)
    return perms, signs, values(rng, (c.batch, c.d), c.dtype)


def bwd_inputs(c):
    """(perms, signs, dg [batch, heads * d])"""
    rng = rng_of(c)
    perms, signs = perms_signs(rng, c.heads, c.d, c.perm, c.sign)
    return perms, signs, values(rng, (c.batch, c.heads * c.d), c.dtype)


def row0_inputs(c):
    """(perms [1, d], signs [1, d], x [batch, d], dg0 [batch, n], dx0 [batch, embed])"""
    rng = rng_of(c)
    perms, signs = perms_signs(rng, 1, c.d)
    return perms, signs, values(rng, (c.batch, c.d), c.dtype), values(rng, (c.batch, c.n), c.dtype), values(rng, (c.batch, c.embed), c.dtype)


def bits(a64, dtype):
    """the storage bit pattern of exactly representable float64 values: uint32 (fp32) or uint16 (bf16)"""
    w = np.ascontiguousarray(a64, np.float64).astype(np.float32).view(np.uint32)
    return w if dtype == "fp32" else (w >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------ bars
# Derived, elementwise, not fitted.  u_T: the unit roundoff of the storage type of a computed output (one rounding to bf16: 2^-8 of
# the value; fp32 outputs carry their roundings in the second term).  The kernels add in fp32: a sum of k terms by any order is within
# (k - 1) 2^-24 sum |terms| of the exact one (to first order), the pooled average's multiplication by the rounded 1 / pw and the
# product's rounding are two more, one more for slack of the first-order bound: (pw + 2) 2^-24 sum |terms| / pw.
U = {"bf16": 2.0 ** -8, "fp32": 0.0}
EPS = 2.0 ** -24


def pooled_bar(ref, abs_sum, pw, dtype):
    """abs_sum: sum |terms| over the window"""
    with np.errstate(invalid="ignore"):     # 0 * inf where the reference is not finite: those elements are held to equality
        return U[dtype] * np.abs(ref) + (pw + 2) * EPS * abs_sum / pw


def dx_bar(ref, abs_sum, heads, dtype):
    """abs_sum: sum_h |dg term|"""
    with np.errstate(invalid="ignore"):     # 0 * inf where the reference is not finite: those elements are held to equality
        return U[dtype] * np.abs(ref) + heads * EPS * abs_sum


def row0_dx_bar(ref, abs_dx0, abs_dg0, dtype):
    with np.errstate(invalid="ignore"):     # 0 * inf where the reference is not finite: those elements are held to equality
        return U[dtype] * np.abs(ref) + 2 * EPS * (abs_dx0 + abs_dg0)


def worst_ratio(got, ref, bar):
    """(every element within its bar, the worst |got - ref| / bar).  Elements whose reference is not finite (a planted inf, or
    +inf - inf) are held to equality / isnan; bar == 0 demands equality."""
    got, ref, bar = (np.asarray(v, np.float64).reshape(-1) for v in (got, ref, np.broadcast_to(bar, np.shape(ref))))
    fin = np.isfinite(ref)
    same = np.where(np.isnan(ref), np.isnan(got), got == ref)
    ok = bool(same[~fin].all())
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(got[fin] - ref[fin])
        b = bar[fin]
        ratio = np.where(err == 0, 0.0, np.where(b > 0, err / np.where(b > 0, b, 1.0), np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    return ok and worst <= 1.0, worst
