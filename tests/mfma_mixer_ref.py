"""The two token mixers whose token-axis product runs on the matrix cores with compensated bf16 arithmetic -- gfilter_fast_kernel<0/1>
(csrc/spv_gfilter.hip) and hadamard_mfma_kernel<0/1> (csrc/spv_hadamard.hip, the fused spv_hadamard_ln_fwd / _bwd) -- held to float64
element by element: beside each float64 reference the sum S_i of the absolute values of every product that reaches element i, a
restatement of each kernel's roundings in numpy float32 that can make named mistakes, the case tables and seeded inputs of
tests/test_gpu_mfma_mixer_edges.py, and the judge both that file and tests/test_mfma_mixer_ref.py use.  The generic global-filter
kernels are judged the same way with a c of their own.  Pure numpy.

Bars.  |got_i - ref_i| <= c 2^-24 S_i, plus half a bf16 ulp of the reference where the output is stored as bf16.  One c per quantity
and path (C_BAR): four times the floor, rounded up, the floor being the worst err_i / (2^-24 S_i) of the restatement BEFORE its store
against float64 on exactly the GPU tests' inputs -- the planted ones of this module and the seeded normals the older GPU tests of the
same kernels use (tests/test_mfma_mixer_ref.py measures it and asserts c == ceil(4 floor)).  The
factor 4 leaves room for fused multiply-adds and the matrix cores' own order of accumulation.  A value carried as hi + lo bf16 is
exact to 2^-17 of itself, 128 units of 2^-24: where one or two terms make an element (1 and 2 tokens) that is the floor, and it is why
the fast path's c is in the hundreds while a dropped lo part (2^-9 of a term, 32768 units) still stands far above it.

S_i of the global filter runs through both token sums and the filter multiply:
    AC[k] = sum_m |cos(2 pi k m / N)| |x[m]|,  AS[k] likewise;   AZr[k] = c_k / N (AC |wr| + AS |wi|),  AZi[k] = c_k / N (AC |wi| + AS |wr|)
    S_y[n] = sum_k AZr[k] |cos(2 pi k n / N)| + AZi[k] |sin(2 pi k n / N)|          (dx: the same with dy)
    S_dW[k] = c_k / N sum_b (ACx ACg + ASx ASg,  ASx ACg + ACx ASg)
with wi = 0 at the inert bins (DC, and Nyquist of an even length) and S = 0 for dW's inert imaginary parts, which must be +0 bit for
bit.  The trigonometric values are exact where the angle is a multiple of a quarter turn, so the inert parts contribute nothing.

S_i of the Hadamard pair: prenorm  s sum |x| over the sample's N x 512 block;  dx  |dout_i| + s sum |e| over the block, e the float64
LayerNorm gradient computed from the kernel's own stored prenorm;  the column sums  sum |dout xhat| and sum |dout|.  mean, rstd and
out sit behind a LayerNorm and keep the project's measure and bars (LN_BAR, bar()).

Underflow.  The inputs carry planted subnormals.  A value below the smallest normal number 2^-126 -- an input, a product, a spectrum entry, a
lo part -- may be flushed to zero by a matrix core or land on the subnormal grid of bf16, an absolute error and not a relative one, so
every bar has a third term U_i: 2^-126 times the same sum with every |input| set to 1 (and one unit for each later value), 0 where
S_i is 0.  It is some 1e-36 against values of order 1 and decides only elements made of subnormals alone (1 token: y = x w).  The
floors are measured on what is left of the error after U_i.

The sign of a zero output is not held (numpy.fft's is no reference): y, dx and dW are compared with -0 read as +0; dW's inert
imaginary parts are checked for +0 separately, bit for bit."""
import numpy as np

import edge_judge as J
import gfilter_ref as G
import hadamard_ref as H
import spectral_ref as R
from oracle import spectre_oracle as O

F32 = np.float32
EPS = J.EPS
TINY_NORMAL = 2.0 ** -126

# four times the floors tests/test_mfma_mixer_ref.py::test_floors_set_the_bars prints, rounded up
C_BAR = dict(fast_y=648, fast_dx=613, fast_dw=269, generic_y=13, generic_dx=11, generic_dw=9,
             had_prenorm=1, had_dx=25, had_partials=17, had_dgamma=14, had_dbeta=1)


def bf16(a):
    """round to nearest even onto bf16, kept as float32"""
    return J.cast(a, "bf16").astype(F32)


# ------------------------------------------------------------------------------------------------------------------ tables
FAST_TOKENS = (1, 2, 3, 4, 5, 16, 17, 32, 33, 48, 49, 63, 64, 65, 80)
FAST_CASES = ([G.Case("bf16", b, t, d) for t in FAST_TOKENS for d in (64, 512) for b in (1, 3)]
              + [G.Case("bf16", 70, 65, 64)])          # more samples than slabs
# (2, 2730, 3): the largest token count gfilter_select accepts -- 2 columns per workgroup forward, 1 backward, 65536 bytes of LDS each
GENERIC_CASES = [G.Case(dt, 3, t, d) for t, d in ((5, 24), (65, 72), (126, 8), (197, 24)) for dt in G.DTYPES] + [G.Case(dt, 2, 2730, 3) for dt in G.DTYPES]
FILTER_CASES = FAST_CASES + GENERIC_CASES
HADAMARD_CASES = H.LN_CASES
assert len(set(FILTER_CASES)) == len(FILTER_CASES)


def path_name(c):
    return "fast" if G.path(c.dtype, c.tokens, c.dim, not c.off) == G.FAST else "generic"


def filter_inputs(c):
    """(x, dy, filter): seeded normals in the storage dtype with +0, -0 and +- the smallest subnormal planted at seeded places, then one
    column of x and one of dy zeroed in one sample each (columns are independent: that column of y / dx must come back as zeros); the
    filter as gfilter_ref.inputs makes it.  Read-only."""
    rng = G.rng_of(c, "edges")
    shape = (c.batch, c.tokens, c.dim)
    x, dy = (J.values(rng, shape, c.dtype, plant="finite").copy() for _ in range(2))
    x[rng.integers(c.batch), :, rng.integers(c.dim)] = 0.0
    dy[rng.integers(c.batch), :, rng.integers(c.dim)] = 0.0
    w = rng.standard_normal((G.bins(c.tokens), c.dim, 2))
    w[G.inert(c.tokens), :, 1] = np.where(np.arange(c.dim) % 2 == 0, 1.5, -2.5)
    w = G.C.storage_round(w, "fp32")
    for a in (x, dy, w):
        a.setflags(write=False)
    return x, dy, w


def hadamard_inputs(c, planted=True):
    """dict(x, gamma, beta, dout) of a fused-pair case, x and dout planted as above; both LN_MODES run on the same inputs.  planted =
    False: the seeded normals tests/test_gpu_hadamard_mixer.py feeds the same case."""
    rng = H.rng_of(c, "edges" if planted else "fold")
    shape = (c.batch, c.tokens, 512)
    draw = (lambda: J.values(rng, shape, "bf16", plant="finite")) if planted else (lambda: H.normal(rng, shape, "bf16"))
    d = dict(x=draw())
    d["gamma"], d["beta"] = H.affine(rng, 512)
    d["dout"] = draw()
    return d


# ------------------------------------------------------------------------------------------------------------------ the filter: reference
def trig(tokens):
    """float64 (cos, sin)(2 pi k n / N) as (K, N), exact at the multiples of a quarter turn"""
    m = (np.arange(G.bins(tokens))[:, None] * np.arange(tokens)[None, :]) % tokens
    a = 2.0 * np.pi * m / tokens
    fc, fs = np.cos(a), np.sin(a)
    quarter = (4 * m) % tokens == 0
    q = (4 * m // tokens) % 4
    fc[quarter] = np.array([1.0, 0.0, -1.0, 0.0])[q[quarter]]
    fs[quarter] = np.array([0.0, 1.0, 0.0, -1.0])[q[quarter]]
    return fc, fs


def filter_dft(x, dy, w):
    """y, dx, dW as the two real DFT products the kernels compute, in float64 (tests/test_mfma_mixer_ref.py pins it to gfilter_ref's
    numpy.fft form at 1e-12)"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    N = x.shape[1]
    fc, fs = trig(N)
    wc = G.w_eff(w, N)
    wr, wi, ck = wc.real, wc.imag, (G.weights(N) / N)[:, None]
    cx, sx, cg, sg = fc @ x, fs @ x, fc @ dy, fs @ dy
    back = lambda zr, zi: fc.T @ zr - fs.T @ zi   # noqa: E731
    dw = np.stack([ck * (cx * cg + sx * sg).sum(0), ck * (sx * cg - cx * sg).sum(0)], axis=-1)
    dw[G.inert(N), :, 1] = 0.0
    return dict(y=back(ck * (cx * wr + sx * wi), ck * (cx * wi - sx * wr)), dx=back(ck * (cg * wr - sg * wi), -ck * (sg * wr + cg * wi)), dw=dw)


def filter_reference(x, dy, w):
    """dict(y, dx, dw, S_y, S_dx, S_dw): gfilter_ref's float64 references and the sums of absolute terms of the module docstring"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    N = x.shape[1]
    fc, fs = (np.abs(f) for f in trig(N))
    wc = G.w_eff(w, N)
    wr, wi, ck = np.abs(wc.real), np.abs(wc.imag), (G.weights(N) / N)[:, None]
    acx, asx, acg, asg = fc @ np.abs(x), fs @ np.abs(x), fc @ np.abs(dy), fs @ np.abs(dy)
    back = lambda zr, zi: fc.T @ zr + fs.T @ zi   # noqa: E731
    tokens = lambda ac, as_: back(ck * (ac * wr + as_ * wi), ck * (ac * wi + as_ * wr))   # noqa: E731
    S_dw = np.stack([ck * (acx * acg + asx * asg).sum(0), ck * (asx * acg + acx * asg).sum(0)], axis=-1)
    ref = dict(y=G.fwd(x, w), dx=G.dx(dy, w), dw=G.dw(x, dy), S_y=tokens(acx, asx), S_dx=tokens(acg, asg), S_dw=S_dw)
    # underflow: the same sums with every |x[m]| (|dy[m]|) = 1, and one unit per bin for Z, per sample for dW's products
    ac1, as1 = fc.sum(1)[:, None], fs.sum(1)[:, None]
    U = tokens(ac1, as1) + (fc + fs).sum(0)[:, None]
    ref["U_y"] = ref["U_dx"] = TINY_NORMAL * np.broadcast_to(U, x.shape)
    ref["U_dw"] = TINY_NORMAL * (np.stack([ck * (ac1 * (acg + acx) + as1 * (asg + asx)).sum(0), ck * (as1 * (acg + acx) + ac1 * (asg + asx)).sum(0)], axis=-1)
                                 + x.shape[0])
    for k in ("y", "dx", "dw"):     # no term, no value (the sign numpy.fft gives its zero there is not held), and no allowance
        if k == "dw":
            ref["S_dw"][G.inert(N), :, 1] = 0.0
        none = ref["S_" + k] == 0
        assert not ref[k][none].any()
        ref[k], ref["U_" + k] = np.where(none, 0.0, ref[k]), np.where(none, 0.0, ref["U_" + k])
    return ref


def plus_zero(a):
    """-0 read as +0"""
    return np.asarray(a, np.float64) + 0.0


def floor_units(got, ref, name):
    """the worst err_i / (2^-24 S_i) of a restated output before its store, of what is left of err_i after the underflow allowance"""
    left = np.maximum(np.abs(np.asarray(got, np.float64) - ref[name]) - ref["U_" + name], 0.0)
    return J.floor_ratio(ref[name] + left, ref[name], ref["S_" + name])


def _bar(ref, name, c, dtype):
    return J.Spec("bar", ref[name], dtype, c * EPS * ref["S_" + name] + ref["U_" + name] + J.half_ulp(ref[name], dtype))


def filter_specs(c, ref):
    p = path_name(c)
    return dict(y=_bar(ref, "y", C_BAR[p + "_y"], c.dtype), dx=_bar(ref, "dx", C_BAR[p + "_dx"], c.dtype), dw=_bar(ref, "dw", C_BAR[p + "_dw"], "fp32"))


def filter_verdict(c, ref, got):
    """(ok, {y, dx, dw: worst ratio to the bar}); got: the stored outputs as float64.  dW's inert imaginary parts: +0 bit for bit."""
    ok, worst = J.verdict(filter_specs(c, ref), {k: plus_zero(got[k]) for k in ("y", "dx", "dw")})
    im = np.asarray(got["dw"])[G.inert(c.tokens), :, 1]
    if im.any() or np.signbit(im).any():
        ok, worst["dw"] = False, np.inf
    return ok, worst


def excess_units(ref, got, name, dtype):
    """what is left of |got_i - ref_i| after the store's half ulp and the underflow allowance, in units of 2^-24 S_i, at its worst:
    the figure the floors are stated in, for a stored output"""
    left = np.maximum(np.abs(plus_zero(got) - ref[name]) - ref["U_" + name] - J.half_ulp(ref[name], dtype), 0.0)
    some = ref["S_" + name] > 0
    return float((left[some] / (EPS * ref["S_" + name][some])).max()) if some.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------ the filter: restatement
FAST_LO_MISTAKES = ("t1_lo_zero", "t2_lo_zero", "z_lo_zero")
# inert_kept: the kernels' `inert` rule dropped -- the filter's imaginary part read as stored, the gradient's written as computed.  In y
# and dx the first half is invisible, and rightly: that part of the filter meets only the sines of whole half turns, which are zero (to
# 1e-16 in the float32 table); the gradient's inert imaginary part then is a -0 or some 1e-16 where +0 is owed.
FILTER_MISTAKES = FAST_LO_MISTAKES + ("sine_cross_term", "inert_kept", "nyquist_twice", "zi_sign", "dw_no_ck")


def _weights32(w, tokens, mistake):
    w = np.asarray(w, F32)
    wr, wi = w[..., 0], w[..., 1].copy()
    if mistake != "inert_kept":
        wi[G.inert(tokens)] = 0.0
    c = G.weights(tokens).astype(F32)
    if mistake == "nyquist_twice" and tokens % 2 == 0:
        c[tokens // 2] = 2.0
    inv_n = F32(1.0 / tokens)
    return wr, wi, (c * inv_n)[:, None], (np.full_like(c, inv_n) if mistake == "dw_no_ck" else c * inv_n)[:, None]


def _fast_tokens(t2, zr, zi, K, N, mistake):
    """gfilter_ref._fast_tokens with the mistakes: the lo parts of Z dropped; the hi . lo term of the sine part dropped"""
    (rh, rl), (ih, il) = G._split(zr), G._split(-zi)
    if mistake == "z_lo_zero":
        rl, il = np.zeros_like(rl), np.zeros_like(il)
    gc, gs = t2[:, 0, :N, :K], t2[:, 1, :N, :K]
    e = lambda g, z: np.einsum("nk,bkd->bnd", g, z)   # noqa: E731
    y = e(gc[0], rh) + e(gs[0], ih) + e(gc[1], rh) + e(gs[1], ih) + e(gc[0], rl)
    if mistake != "sine_cross_term":
        y = y + e(gs[0], il)
    assert y.dtype == F32
    return y


def filter_restate(c, x, dy, w, mistake=None):
    """dict(y, dx, dw) in float32 before any store, by the path that serves the case: every rounding of gfilter_fast_kernel<0/1>
    (gfilter_ref.fast_fwd32 / fast_bwd32 when no mistake is asked for) or of the generic kernels (generic_fwd32 / generic_bwd32)"""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    N, K = x.shape[1], G.bins(x.shape[1])
    wr, wi, ck, ckw = _weights32(w, N, mistake)
    flip = F32(-1.0 if mistake == "zi_sign" else 1.0)
    if path_name(c) == "fast":
        t1, t2 = G.fast_tables(N)
        if mistake == "t1_lo_zero":
            t1[1] = 0.0
        if mistake == "t2_lo_zero":
            t2[1] = 0.0
        (cx, sx), (cg, sg) = G._fast_bins(t1, x, K, N), G._fast_bins(t1, dy, K, N)
        back = lambda zr, zi: _fast_tokens(t2, zr, zi, K, N, mistake)   # noqa: E731
    else:
        fc, fs = G._dft32(N)
        cx, sx, cg, sg = (np.einsum("kn,bnd->bkd", f, v) for v in (x, dy) for f in (fc, fs))
        back = lambda zr, zi: G._token32(zr, zi, fc, fs)   # noqa: E731
    dw = np.stack([(ckw * (cx * cg + sx * sg)).sum(0, dtype=F32), (ckw * (sx * cg - cx * sg)).sum(0, dtype=F32)], axis=-1)
    if mistake != "inert_kept":
        dw[G.inert(N), :, 1] = 0.0
    out = dict(y=back(ck * (cx * wr + sx * wi), flip * (ck * (cx * wi - sx * wr))),
               dx=back(ck * (cg * wr - sg * wi), flip * (-ck * (sg * wr + cg * wi))), dw=dw)
    assert all(v.dtype == F32 for v in out.values())
    return out


def filter_store(c, pre):
    """the stores: y and dx into the storage dtype, dW stays float32; as float64"""
    return dict(y=J.cast(pre["y"], c.dtype), dx=J.cast(pre["dx"], c.dtype), dw=np.asarray(pre["dw"], np.float64))


# ------------------------------------------------------------------------------------------------------------------ Hadamard: reference
HADAMARD_ELEMENTWISE = ("prenorm", "dx", "partials", "dgamma", "dbeta")


def hadamard_reference(data, got):
    """float64 references of the fused pair downstream of the kernel's own stored prenorm (hadamard_ref.ln_fwd / ln_bwd), with S_* for
    the outputs held element by element"""
    x, dout, gamma = (np.asarray(data[k], np.float64) for k in ("x", "dout", "gamma"))
    B, N, Dm = x.shape
    s = H.scale(N, Dm)
    own = np.asarray(got["prenorm"], np.float64)
    ref = {**H.ln_fwd(x, gamma, data["beta"], prenorm=own), **H.ln_bwd(dout, own, gamma)}
    e, dg, db = R.ln_bwd(dout, own, gamma)
    whole = lambda a: np.broadcast_to(np.abs(a).sum((1, 2), keepdims=True), a.shape)   # noqa: E731
    ref["S_prenorm"] = s * whole(x)
    ref["S_dx"] = np.abs(dout) + s * whole(e)
    ref["S_partials"] = np.stack([np.abs(dg).sum(1), np.abs(db).sum(1)], axis=1)
    ref["S_dgamma"], ref["S_dbeta"] = ref["S_partials"][:, 0].sum(0), ref["S_partials"][:, 1].sum(0)
    # underflow: one unit per term -- x (prenorm), dout and the hi and lo parts of e (dx), a row's product (the column sums)
    units = dict(prenorm=s * N * Dm, dx=1 + 2 * s * N * Dm, partials=N, dgamma=N * B, dbeta=N * B)
    for k, n in units.items():
        ref["U_" + k] = np.where(ref["S_" + k] == 0, 0.0, TINY_NORMAL * n)
    return ref


def hadamard_specs(ref):
    stored = dict(prenorm="bf16", dx="bf16")
    return {k: _bar(ref, k, C_BAR["had_" + k], stored.get(k, "fp32")) for k in HADAMARD_ELEMENTWISE}


LN_BARS = dict(mean=H.LN_BAR, rstd=H.LN_BAR, out=H.bar(H.LN_BAR, "bf16"))


def hadamard_verdict(data, got):
    """(ok, {name: worst ratio to its bar}); got: prenorm, out, mean, rstd, dx, partials (B, 2, 512), dgamma, dbeta as float64.  The
    elementwise outputs by edge_judge.verdict; mean, rstd and out by the project's measure (per sample for out) and bars."""
    ref = hadamard_reference(data, got)
    ok, worst = J.verdict(hadamard_specs(ref), {k: plus_zero(got[k]) for k in HADAMARD_ELEMENTWISE})
    for k, b in LN_BARS.items():
        worst[k] = R.err(got[k], ref[k], 1 if k == "out" else 0) / b
        ok = ok and worst[k] <= 1.0
    return ok, worst


# ------------------------------------------------------------------------------------------------------------------ Hadamard: restatement
HADAMARD_LO_MISTAKES = ("lo_zero", "lo_of_hi")
HADAMARD_MISTAKES = HADAMARD_LO_MISTAKES + ("residual_before_scale", "pad_rows_live", "stats_unrounded")
STALE = 1.0   # what the restatement finds in the LDS rows behind an operand image


def _factor(N, zeroed):
    """the MFMA's A operand: (-1)^popcount(m & k) as (32-row tiles, K steps of 16), zero where m >= N or k >= N"""
    m, k = np.arange((N + 31) // 32 * 32)[:, None], np.arange((N + 15) // 16 * 16)[None, :]
    ones = sum(((m & k) >> i) & 1 for i in range(8))
    a = np.where(ones & 1, -1.0, 1.0).astype(F32)
    if zeroed:
        a[(m >= N) | (k >= N)] = 0.0
    return a


def _token_axis(images, N, mistake):
    """step 2: the +-1 factor times the bf16 operand images on the MFMA, every image into the same float32 accumulator.  The rows from
    N to the K step's end are not part of an image: the kernel reads neither them nor the factor's entries there."""
    a = _factor(N, mistake != "pad_rows_live")
    acc = None
    for img in images:
        full = np.full((img.shape[0], a.shape[1], img.shape[2]), STALE, F32)
        full[:, :N] = img
        t = np.matmul(a, full)
        acc = t if acc is None else acc + t
    assert acc.dtype == F32
    return acc[:, :N]


def hadamard_fwd32(data, mistake=None):
    """hadamard_mfma_kernel<0>: exact +-1 sums of the bf16 x in float32, the scale, the bf16 store of prenorm; mean / rstd of the STORED
    prenorm in float32; out.  dict(prenorm32 (before its store), prenorm, mean, rstd, out)"""
    x = np.asarray(data["x"], F32)
    B, N, Dm = x.shape
    v = O.fwht(_token_axis([x], N, mistake), normalize=False)
    pre32 = v * F32(H.scale32(N, Dm))
    assert pre32.dtype == F32
    pre = bf16(pre32)
    src = pre32 if mistake == "stats_unrounded" else pre
    mean = src.sum(-1, dtype=F32) * F32(1.0 / Dm)
    d = src - mean[..., None]
    rstd = (F32(1.0) / np.sqrt((d * d).sum(-1, dtype=F32) * F32(1.0 / Dm) + F32(1e-5))).astype(F32)
    out = (pre - mean[..., None]) * rstd[..., None] * np.asarray(data["gamma"], F32) + np.asarray(data["beta"], F32) + x
    return dict(prenorm32=pre32, prenorm=pre, mean=mean, rstd=rstd, out=bf16(out))


def _wave_colsum(t):
    """a sample's column sums as the eight waves form them: wave w adds rows w, w + 8, ... in order, then the waves are added in order"""
    acc = np.zeros((t.shape[0], 8, t.shape[2]), F32)
    for r in range(t.shape[1]):
        acc[:, r % 8] += t[:, r]
    s = np.zeros((t.shape[0], t.shape[2]), F32)
    for w in range(8):
        s += acc[:, w]
    return s


def hadamard_bwd32(data, fwd, mistake=None):
    """hadamard_mfma_kernel<1> fed the forward's stored prenorm and float32 mean / rstd: the LayerNorm backward in float32, e as hi + lo
    bf16, the +-1 sums in float32, the scale, + dout, the store; the column sums.  dict(dx32 (before its store), dx, partials, dgamma,
    dbeta)"""
    d, p = np.asarray(data["dout"], F32), np.asarray(fwd["prenorm"], F32)
    B, N, Dm = d.shape
    mu, rs = np.asarray(fwd["mean"], F32)[..., None], np.asarray(fwd["rstd"], F32)[..., None]
    h = (p - mu) * rs
    q = d * np.asarray(data["gamma"], F32)
    sa = q.sum(-1, dtype=F32, keepdims=True) * F32(1.0 / Dm)
    sb = (q * h).sum(-1, dtype=F32, keepdims=True) * F32(1.0 / Dm)
    e = rs * (q - sa - h * sb)
    assert e.dtype == F32
    hi = bf16(e)
    lo = bf16(e - hi)
    if mistake == "lo_zero":
        lo = np.zeros_like(hi)
    if mistake == "lo_of_hi":
        lo = bf16(bf16(e) - hi)
    v = O.fwht(_token_axis([hi, lo], N, mistake), normalize=False)
    s = F32(H.scale32(N, Dm))
    dx32 = (v + d) * s if mistake == "residual_before_scale" else v * s + d
    assert dx32.dtype == F32
    partials = np.stack([_wave_colsum(d * h), _wave_colsum(d)], axis=1)
    fold = np.zeros((2, Dm), F32)
    for b in range(B):
        fold += partials[b]
    return dict(dx32=dx32, dx=bf16(dx32), partials=partials, dgamma=fold[0], dbeta=fold[1])


def hadamard_restate(data, mistake=None):
    """the fused pair as the GPU test runs it, stored outputs as float64 (and prenorm32 / dx32)"""
    fwd = hadamard_fwd32(data, mistake)
    return {k: np.asarray(v, np.float64) for k, v in {**fwd, **hadamard_bwd32(data, fwd, mistake)}.items()}
