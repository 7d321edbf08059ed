"""The case tables of tests/test_gpu_spectral_edges.py, their seeded inputs, a host restatement of every dispatch rule of the spectral
kernels (csrc/spv_fft.hip: spv_fnet_mix's selector, the fused and row-0 entry points, spv_rfft_real, spv_haar_dwt's per-level kernel
choice; csrc/spv_hadamard.hip: rows per workgroup; csrc/spv_rowops.hip: the haar_ln pair) and the bars.  Shared with
tests/test_spectral_ref.py, which checks on the CPU that the tables reach every branch, that expected_path agrees with the library's
host-side answers, and that the float32 floor of the references on exactly these inputs stays within a quarter of each fp32 bar.

Shapes are the smallest at which each branch exists.  Family tags: "mix" (LDS kernels and generic fallback), "mfma" (bf16, dim 512),
"cls", "rfft", "haar", "haar_ln", "fwht"."""
import zlib
from collections import namedtuple

import numpy as np

from attention_edge_cases import storage_round

# A. spv_fnet_mix off the MFMA window.  off: bytes x, y and add_in sit off 16-byte alignment (the generic path only: the others refuse)
Mix = namedtuple("Mix", "dtype batch tokens dim off", defaults=(0,))
# B. fnet_mfma_kernel: bf16, dim 512
Mfma = namedtuple("Mfma", "batch tokens")
Cls = namedtuple("Cls", "dtype batch tokens dim")
Rfft = namedtuple("Rfft", "dtype rows dim transpose")
# off: bytes x sits off 16-byte alignment
Haar = namedtuple("Haar", "dtype batch tokens dim axis levels inverse off", defaults=(0,))
HaarLn = namedtuple("HaarLn", "rows dim")
Fwht = namedtuple("Fwht", "dtype rows n_in n n_out mode repeat residual")

DTYPES = ("fp32", "bf16")
SPV_F32, SPV_BF16 = 0, 1
CODE = {"fp32": SPV_F32, "bf16": SPV_BF16}


def _both(make, *a, **kw):
    return [make(dt, *a, **kw) for dt in DTYPES]


# ------------------------------------------------------------------------------------------------------------------ dispatch
FNET_MH, FNET_TWS = 20, 40
MH_STEPS = (4, 9, 13, 17, 20)
LDS_LIMIT = 160 * 1024


def mix_path(dtype, tokens, dim, workspace=True, twiddle=True, count=1):
    """what serves spv_fnet_mix: ("mfma",), ("lds", MH), ("generic", reason) or ("refused", why)"""
    if count <= 0 or tokens <= 0 or dim <= 0:
        return ("refused", "empty")
    if dtype == "bf16" and dim == 512 and 2 <= tokens <= 65:
        return ("mfma",) if twiddle else ("refused", "twiddle")
    reason = None
    if dim & (dim - 1):
        reason = "non-power-of-two"
    elif dim < 8:
        reason = "dim < 8"
    elif dim > 4096:
        reason = "dim > 4096"
    elif tokens // 2 + 1 > 2 * FNET_MH:
        reason = "tokens > 79"
    elif (tokens + 3) * dim * 4 > LDS_LIMIT:
        reason = "over the LDS"
    if reason is None:
        if not twiddle:
            return ("refused", "twiddle")
        mh = (tokens // 2 + 1 + 1) // 2
        return ("lds", next(s for s in MH_STEPS if mh <= s))
    if not workspace:
        return ("refused", "workspace")
    if dim * 12 > 64 * 1024 or tokens * 8 > 64 * 1024:
        return ("refused", "shape too large")
    return ("generic", reason)


def fft_passes(dim):
    """radices of make_fft_plan(dim): radix 8 while it divides, then the remainder"""
    out = []
    while dim >= 8:
        out.append(8)
        dim //= 8
    return out + ([dim] if dim > 1 else [])


def workspace_floats(dtype, batch, tokens, dim):
    """spv_fnet_workspace_floats: a function of the shape only (the MFMA window lies inside the LDS rule)"""
    p = mix_path("fp32", tokens, dim)
    return 0 if p[0] == "lds" else batch * tokens * dim * 2


def twiddle_floats(tokens):
    return (tokens + 1) * 2 * FNET_TWS + 2 * 5 * 64 * 8 // 2 + 8 * 2 * 16 * 5 + (8 * 64 * 8 + 4 * 64 * 8) // 2


def fnet_ln_supported(dtype, tokens, dim):
    return int(dtype == "bf16" and dim == 512 and 2 <= tokens <= 65)


def cls_supported(dtype, tokens, dim):
    return int(dim in (256, 512, 1024) and tokens >= 1)


def cls_row_groups(dtype):
    return 4 if dtype == "bf16" else 2


def haar_ln_supported(dtype, dim):
    return int(dtype == "bf16" and dim in (512, 1024))


HAAR_LEVEL_CAP, HAAR_DIM_CAP = 4096 * 256, 8192 * 256    # elements / 8-element chunks one sweep of the capped grids covers
HAAR_LN_FWD_CAP_ROWS, HAAR_LN_BWD_CAP_ROWS = 2048 * 4, 1024 * 4


def haar_plan(c):
    """the kernel of each launch of spv_haar_dwt, in launch order: "vector" (haar_dim_bf16_kernel) or "scalar" (haar_level_kernel).
    The first launch reads x, the others the aligned y / scratch."""
    length, lens = (c.tokens if c.axis == 1 else c.dim), []
    for _ in range(c.levels):
        lens.append(length)
        length -= length // 2
    order = lens[::-1] if c.inverse & 1 else lens
    return ["vector" if c.axis == 2 and c.dtype == "bf16" and c.dim % 8 == 0 and ln % 16 == 0 and not (i == 0 and c.off % 16) else "scalar"
            for i, ln in enumerate(order)]


def haar_refused(axis, levels, scratch=True):
    return "axis" if axis not in (1, 2) else "levels" if not 1 <= levels <= 16 else "scratch" if levels > 1 and not scratch else None


def fwht_rpw(n):
    return 1 if n >= 512 else 512 // n


def fwht_refused(n_in, n, n_out):
    return "power of two" if n < 1 or n & (n - 1) or n > 16384 else "outside" if not (1 <= n_in <= n and 1 <= n_out <= n) else None


# ------------------------------------------------------------------------------------------------------------------ tables
MH_TOKENS = (1, 2, 15, 16, 35, 36, 51, 52, 67, 68, 79, 80)
MIX_CASES = (
    # MH selector; dims 8, 16, 32: the plans (8), (8, 2), (8, 4); the dim sweep below adds the three- and four-pass ones
    [Mix(dt, 3, t, (8, 16, 32)[i % 3]) for i, t in enumerate(MH_TOKENS) for dt in DTYPES]
    + [Mix(dt, 3, t, d) for t, d in ((36, 8), (51, 16), (79, 32)) for dt in DTYPES]     # <13>, <20>: every plan
    # dim sweep: tokens 5 (the zeroed pad row is live) and 6; dim 1024: two trips of phase C over k
    + [Mix(dt, 3, t, d) for t in (5, 6) for d in (8, 64, 128, 256, 1024) for dt in DTYPES]
    # LDS capacity
    + [Mix(dt, 3, t, d) for t, d in ((37, 1024), (38, 1024), (17, 2048), (18, 2048), (7, 4096), (8, 4096)) for dt in DTYPES]
    + [Mix("fp32", 3, 77, 512), Mix("fp32", 3, 78, 512)]
    + [Mix(dt, b, t, 4096) for b in (1, 2) for t in (7, 8) for dt in DTYPES]
    # the ends of the MFMA window
    + [Mix("bf16", 3, 1, 512), Mix("bf16", 3, 66, 512)]
    # generic only
    + [Mix(dt, 3, t, d) for t, d in ((1, 1), (2, 3), (7, 48), (197, 96), (5, 100), (3, 257), (6, 520), (300, 24), (2, 4)) for dt in DTYPES]
    + [Mix(dt, 3, 7, 48, 8) for dt in DTYPES]      # any alignment of the element type
)
MFMA_TOKENS = (2, 3, 8, 9, 16, 17, 31, 32, 33, 48, 49, 62, 63, 64, 65)
MFMA_CASES = [Mfma(b, t) for t in MFMA_TOKENS for b in (1, 3)] + [Mfma(513, 2)]
MFMA_MODES = ("mixA", "mixB", "ln", "ln_defer")
CLS_CASES = [Cls(dt, b, t, d) for d in (256, 512, 1024) for t in (1, 2, 3, 4, 5, 7, 65) for b in (1, 3) for dt in DTYPES]
RFFT_CASES = [Rfft(dt, r, d, tr) for d in (1, 2, 7, 16, 255, 256, 257, 1000, 8192) for r in (1, 3) for tr in (0, 1) for dt in DTYPES]
_VEC_SHAPES = ((16, 1), (16, 2), (48, 2), (24, 2), (512, 1), (512, 5), (512, 6))
HAAR_CASES = (
    [Haar(dt, 2, 65, 8, 1, lv, inv) for lv in (1, 3, 7, 8) for inv in range(4) for dt in DTYPES]
    + [Haar(dt, 3, 5, 33, 2, lv, inv) for lv in (1, 2, 6) for inv in range(4) for dt in DTYPES]
    + [Haar(dt, 1, 1, 1, 2, 1, inv) for inv in range(4) for dt in DTYPES]
    + [Haar(dt, 2, 3, d, 2, lv, inv) for d, lv in _VEC_SHAPES for inv in range(4) for dt in DTYPES]
    + [Haar("bf16", 2, 3, d, 2, lv, inv, 8) for d, lv in _VEC_SHAPES for inv in range(4)]
)
# grid-stride trips: the only cases larger than a few hundred KB
HAAR_BIG_CASES = [Haar("fp32", 2, 1031, 512, 1, 1, 2), Haar("bf16", 1, 32776, 512, 2, 1, 0), Haar("bf16", 1, 32776, 512, 2, 1, 1)]
HAAR_LN_CASES = [HaarLn(r, d) for d in (512, 1024) for r in (1, 5, HAAR_LN_FWD_CAP_ROWS + 1)]
HAAR_LN_MODES = ("fold", "defer")


def _fwht_rows(n):
    return (1, fwht_rpw(n) + 1, 3)


FWHT_CASES = (
    [Fwht(dt, r, n, n, n, m, 1, False) for n in (1, 2, 8, 256, 512, 1024, 16384) for r in sorted(set(_fwht_rows(n))) for m in (0, 1, 2)
     for dt in DTYPES]
    + [Fwht(dt, 3, a, n, b, m, rep, res) for a, n, b in ((100, 128, 100), (1, 8, 5)) for m in (0, 1, 2) for rep, res in ((1, False), (3, True))
       for dt in DTYPES]
    + [Fwht(dt, 3, n, n, n, m, 3, True) for n in (8, 1024) for m in (0, 1, 2) for dt in DTYPES]
)
ALL = dict(mix=MIX_CASES, mfma=MFMA_CASES, cls=CLS_CASES, rfft=RFFT_CASES, haar=HAAR_CASES + HAAR_BIG_CASES, haar_ln=HAAR_LN_CASES, fwht=FWHT_CASES)
for _cases in ALL.values():
    assert len(set(_cases)) == len(_cases)


def expected_path(c):
    """what serves a case of any family, by the rules above"""
    if isinstance(c, Mix):
        return mix_path(c.dtype, c.tokens, c.dim)
    if isinstance(c, Mfma):
        return mix_path("bf16", c.tokens, 512)
    if isinstance(c, Cls):
        return ("cls", c.dim, cls_row_groups(c.dtype)) if cls_supported(c.dtype, c.tokens, c.dim) else ("refused", "unsupported")
    if isinstance(c, Rfft):
        return ("rfft",) if c.dim * 8 <= 64 * 1024 else ("refused", "dim too large")
    if isinstance(c, Haar):
        why = haar_refused(c.axis, c.levels)
        return ("refused", why) if why else ("haar",) + tuple(haar_plan(c))
    if isinstance(c, HaarLn):
        return ("haar_ln", c.dim) if haar_ln_supported("bf16", c.dim) else ("refused", "unsupported")
    why = fwht_refused(c.n_in, c.n, c.n_out)
    return ("refused", why) if why else ("fwht", fwht_rpw(c.n))


def case_id(c):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


def fwht_scale(c):
    """mode 0 is run normalised (hadamard_transform's n^-1/2 as the float the entry point receives), the fwht_fast modes as they are"""
    return float(np.float32(float(c.n) ** (-0.5 * c.repeat))) if c.mode == 0 else 1.0


# ------------------------------------------------------------------------------------------------------------------ inputs
def rng_of(c, tag=""):
    return np.random.default_rng(zlib.crc32(f"{type(c).__name__}/{case_id(c)}/{tag}".encode()))


def normal(rng, shape, dtype):
    """standard normal, rounded to the storage dtype; read-only"""
    a = storage_round(rng.standard_normal(shape), dtype)
    a.setflags(write=False)
    return a


def affine(rng, n):
    """LayerNorm gamma in [0.5, 1.5), beta 0.1 N(0, 1), as float32 stores them"""
    g, b = storage_round(0.5 + rng.random(n), "fp32"), storage_round(0.1 * rng.standard_normal(n), "fp32")
    g.setflags(write=False)
    b.setflags(write=False)
    return g, b


# ------------------------------------------------------------------------------------------------------------------ bars
TRANSFORM_BAR = 2e-5      # test_gpu_ops.test_fnet_mix / test_rfft_real, float32
HAAR_BAR = 1e-6           # test_gpu_ops.test_haar_dwt, float32
LN_BAR = 3e-5             # tail_edge_cases.FP32_BAR: LayerNorm outputs and statistics
GRAD_BAR = 6e-5           # tail_edge_cases.GRAD_BAR: parameter-gradient sums and what a LayerNorm backward feeds
BF16_HALF_ULP = 2.0 ** -8  # a bf16-stored output: the tail suite's rule (the unit roundoff of bf16, of the block's maximum)
MFMA_BAR = 1e-2           # test_fnet_mix's bf16 bar: y / prenorm of the kernel that keeps bf16 in LDS
MFMA_DX_BAR = 3e-2        # test_fnet_layernorm_residual_fused: dx of the fused backward


def haar_bar(c):
    """spv_haar_dwt stores every level's tensor in the storage dtype (y / scratch ping-pong), so a bf16 coefficient of level J has been
    rounded J times: one unit roundoff, 2^-8, per bf16 store on its path.  One level: the rule below.  tests/test_spectral_ref.py shows
    with a bf16 restatement of the level loop that 2^-8 alone cannot be met from two levels on (6.5e-3 at seven)."""
    return HAAR_BAR + (c.levels * BF16_HALF_ULP if c.dtype == "bf16" else 0.0)


def bar(fp32_bar, dtype, stored=True):
    """fp32 kernels and the fp32 outputs of bf16 kernels: the fp32 bar; outputs stored as bf16: 2^-8 more"""
    return fp32_bar + (BF16_HALF_ULP if dtype == "bf16" and stored else 0.0)
