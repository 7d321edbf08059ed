"""The Walsh-Hadamard token mixer's float64 reference, a host restatement of csrc/spv_hadamard_core.h's selector, and the case tables
of tests/test_gpu_hadamard_mixer.py.  Shared with tests/test_hadamard_mixer.py, which checks on the CPU that the reference equals the
reference project's own functions (tests/golden/hadamard_mixer.npz), that the tables reach every branch and every refusal, that this
restatement agrees with the library's host-side answers, and that the float32 floor of the references on exactly these inputs stays
within a quarter of each fp32 bar.

Definition:  y = crop_{N,D}( H_Np . pad_{Np,Dp}(x) . H_Dp ) . s,  Np / Dp = next_pow2, H natural order (oracle.spectre_oracle.fwht),
s = (Np Dp)^-1/2 when normalised.  The fused and row-0 nodes follow tests/spectral_ref.py's convention: what comes after a tensor the
kernel stores (prenorm, m0) is computed from the kernel's own stored tensor, so every compared output is one rounding from float64.

The bars are the project's: spectral_edge_cases.TRANSFORM_BAR, LN_BAR, GRAD_BAR and bar()."""
from collections import namedtuple

import numpy as np

import spectral_edge_cases as C
import spectral_ref as R
from oracle import spectre_oracle as O
from spectral_edge_cases import GRAD_BAR, LN_BAR, TRANSFORM_BAR, bar, case_id, rng_of  # noqa: F401  (the test files read them here)

DTYPES = C.DTYPES
CODE = C.CODE

# codes of spv_hadamard_path (include/spv.h)
ONE_KERNEL, GENERIC = 1, 2
REFUSE_EMPTY, REFUSE_DTYPE, REFUSE_DIM, REFUSE_TOKENS, REFUSE_WORKSPACE = -1, -2, -3, -4, -5
MAX_DP, MAX_NP, ONE_MAX_TOKENS = 16384, 32768, 128
LDS_LIMIT, SLAB_LDS = 160 * 1024, 128 * 1024


# ------------------------------------------------------------------------------------------------------------------ reference
def next_pow2(n):
    return 1 << max(0, n - 1).bit_length()


def scale(tokens, dim, normalize=True):
    return float(next_pow2(tokens) * next_pow2(dim)) ** -0.5 if normalize else 1.0


def scale32(tokens, dim, normalize=True):
    """the float the entry points receive"""
    return float(np.float32(scale(tokens, dim, normalize)))


def mix(x, normalize=True, add_in=None):
    """fwht(fwht(pad(x), dim=-1), dim=-2)[..., :N, :D] in float64 (+ add_in)"""
    x = np.asarray(x, np.float64)
    N, Dm = x.shape[-2:]
    Np, Dp = next_pow2(N), next_pow2(Dm)
    p = np.zeros(x.shape[:-2] + (Np, Dp))
    p[..., :N, :Dm] = x
    p = O.fwht(p, normalize=False)                                            # along dim
    p = np.swapaxes(O.fwht(np.swapaxes(p, -1, -2).copy(), normalize=False), -1, -2)   # along tokens
    y = p[..., :N, :Dm] * scale(N, Dm, normalize)
    return y if add_in is None else y + add_in


def row0(x, normalize=True):
    """row 0 of mix(x) in its token-sum form: s . H_Dp . pad(sum_t x[t, :]), cropped"""
    x = np.asarray(x, np.float64)
    N, Dm = x.shape[-2:]
    p = np.zeros(x.shape[:-2] + (next_pow2(Dm),))
    p[..., :Dm] = x.sum(-2)
    return O.fwht(p, normalize=False)[..., :Dm] * scale(N, Dm, normalize)


def ln_fwd(x, gamma, beta, normalize=True, prenorm=None):
    """x1 = LN(mix(x)) gamma + beta + x.  prenorm given: the kernel's own stored tensor, everything after it is computed from it."""
    pre = mix(x, normalize)
    own = pre if prenorm is None else np.asarray(prenorm, np.float64)
    ln, mean, rstd = R.ln_fwd(own, gamma, beta)
    return dict(prenorm=pre, mean=mean, rstd=rstd, out=ln + x)


def ln_bwd(dout, prenorm, gamma, normalize=True):
    """dx = mix(LN-backward(dout)) + dout (no rounding between the two: the kernel carries the fp32 value as hi + lo); dgamma / dbeta:
    column sums over batch and tokens; partials [batch][2][D]"""
    dm, dg, db = R.ln_bwd(dout, np.asarray(prenorm, np.float64), gamma)
    parts = np.stack([dg.sum(1), db.sum(1)], axis=1)
    return dict(dx=mix(dm, normalize) + dout, dgamma=parts[:, 0].sum(0), dbeta=parts[:, 1].sum(0), partials=parts)


def cls_fwd(x, gamma, beta, normalize=True, m0=None):
    pre = row0(x, normalize)
    own = pre if m0 is None else np.asarray(m0, np.float64)
    ln, mean, rstd = R.ln_fwd(own, gamma, beta)
    return dict(m0=pre, mean=mean, rstd=rstd, out=ln + np.asarray(x, np.float64)[:, 0])


def cls_bwd(g1, m0, gamma, tokens, normalize=True):
    """dx[b, n] = s . H_D . LN-backward(g1[b]) for every n, + g1 in row 0; partials [batch][2][D] = g1 xhat, g1"""
    dm, dg, db = R.ln_bwd(g1, np.asarray(m0, np.float64), gamma)
    Dm = dm.shape[-1]
    row = O.fwht(dm, normalize=False) * scale(tokens, Dm, normalize)
    dx = np.repeat(row[:, None, :], tokens, axis=1)
    dx[:, 0] += g1
    return dict(dx=dx, partials=np.stack([dg, db], axis=1))


# ------------------------------------------------------------------------------------------------------------------ dispatch
Plan = namedtuple("Plan", "path np dp rpw cs lds", defaults=(0, 0, 0, 0, 0))


def select(dtype, tokens, dim, workspace=True):
    """hadamard_select of csrc/spv_hadamard_core.h; dtype: "fp32" / "bf16" or a raw code"""
    code = CODE.get(dtype, dtype)
    if tokens < 1 or dim < 1:
        return Plan(REFUSE_EMPTY)
    if code not in (0, 1):
        return Plan(REFUSE_DTYPE)
    if dim > MAX_DP:
        return Plan(REFUSE_DIM)
    dp = next_pow2(dim)
    if dim % 8 == 0 and tokens <= ONE_MAX_TOKENS and tokens * dp * 4 <= LDS_LIMIT:
        return Plan(ONE_KERNEL, next_pow2(tokens), dp, 0, 0, tokens * dp * 4)
    if tokens > MAX_NP:
        return Plan(REFUSE_TOKENS, 0, dp)
    npad = next_pow2(tokens)
    if not workspace:
        return Plan(REFUSE_WORKSPACE, npad, dp)
    rpw = 1 if dp >= 512 else 512 // dp
    cs = min(SLAB_LDS // 4 // npad, 64, dp)
    return Plan(GENERIC, npad, dp, rpw, cs, max(rpw * dp * 4, npad * cs * 4))


def path(dtype, tokens, dim, workspace=True):
    return select(dtype, tokens, dim, workspace).path


def workspace_floats(batch, tokens, dim):
    return batch * tokens * dim if batch >= 1 and path("fp32", tokens, dim) == GENERIC else 0


def ln_supported(dtype, tokens, dim):
    return int(CODE.get(dtype, dtype) == 1 and dim == 512 and 2 <= tokens <= 65)


def cls_supported(dtype, tokens, dim):
    return int(CODE.get(dtype, dtype) in (0, 1) and dim in (256, 512, 1024) and tokens >= 1)


# ------------------------------------------------------------------------------------------------------------------ tables
# off: bytes x, y and add_in sit off 16-byte alignment (the generic path takes it, the one-kernel path refuses it)
Mix = namedtuple("Mix", "dtype batch tokens dim off", defaults=(0,))
Ln = namedtuple("Ln", "batch tokens")
Cls = namedtuple("Cls", "dtype batch tokens dim")

MIX_TOKENS, MIX_DIMS = (1, 2, 3, 5, 64, 65, 66), (8, 24, 512, 768)
MIX_CASES = (
    # the grid: dim 768 pads to 1024, so tokens 64 .. 66 are over the LDS there (generic); everything else is one kernel
    [Mix(dt, b, t, d) for t in MIX_TOKENS for d in MIX_DIMS for b in (1, 3) for dt in DTYPES]
    # generic only: rows that are no 16-byte pieces (dim 1, 5, 100; rpw > 1), over the LDS (Base / 224), tokens > 128, a padded column of
    # 1024 rows (slabs of 32 columns, not 64), one row per workgroup of the row pass (dim 520 -> 1024)
    + [Mix(dt, b, t, d) for b, t, d in ((3, 1, 1), (3, 7, 5), (2, 5, 100), (1, 197, 768), (2, 129, 8), (1, 1000, 40), (2, 6, 520)) for dt in DTYPES]
    # the end of the one-kernel window in tokens, and of the LDS at dim 512 (80 rows fit, 81 do not)
    + [Mix(dt, 1, t, d) for t, d in ((128, 8), (80, 512), (81, 512)) for dt in DTYPES]
    # any alignment of the element type on the generic path
    + [Mix(dt, 3, 7, 12, 8) for dt in DTYPES]
)
MISALIGNED_REFUSED = [Mix(dt, 3, 7, 8, 8) for dt in DTYPES]   # the same offset on a one-kernel shape
# (dtype, tokens, dim, workspace) -> refusal
REFUSALS = {("fp32", 0, 8, True): REFUSE_EMPTY, ("fp32", 8, 0, True): REFUSE_EMPTY, (2, 8, 8, True): REFUSE_DTYPE,
            ("bf16", 3, 16385, True): REFUSE_DIM, ("fp32", 32769, 5, True): REFUSE_TOKENS, ("bf16", 7, 5, False): REFUSE_WORKSPACE,
            ("fp32", 197, 768, False): REFUSE_WORKSPACE}
# the fused pair introduces no grid cap (one workgroup per sample in grid.x), so there is no batch beyond one to add
LN_TOKENS = (2, 3, 16, 17, 32, 33, 64, 65)
LN_CASES = [Ln(b, t) for t in LN_TOKENS for b in (1, 3)]
LN_MODES = ("fold", "defer")
CLS_CASES = [Cls(dt, b, t, d) for d in (256, 512, 1024) for t in (1, 2, 5, 65) for b in (1, 3) for dt in DTYPES]
for _cases in (MIX_CASES, LN_CASES, CLS_CASES):
    assert len(set(_cases)) == len(_cases)


def normal(rng, shape, dtype):
    return C.normal(rng, shape, dtype)


affine = C.affine
