"""References behind tests/test_gpu_head_edges.py: the classifier end of the step (csrc/spv_head.hip: spv_small_sl_fwd / _bwd_rows /
_bwd_w, spv_cross_entropy_fwd / _bwd), the loss half of csrc/spv_distill.hip (spv_distill_loss_fwd / _bwd and the _idx_ pair) and
csrc/spv_infer.hip (spv_eval_head).  Pure numpy, written from include/spv.h's definitions.

*_ref: float64, returning beside each value the per-element sum of absolute terms S_i where its bar needs one.
*_restate: float32 numpy in the kernel's operation order (lane-strided partial sums, the wave tree, the fixed joins), with named
mutants -- plausible mistakes that tests/test_head_ref.py shows the judge to catch.  Unwritten elements are NaN (pred: -7)."""
import numpy as np

import eval_ref as E
import meter_ref as M
import plumbing_ref as P
from edge_judge import F32, cdiv

TINY_NORMAL = 2.0 ** -126        # below it a float32 result may be flushed to zero
LOG2E, LN2 = F32(1.4426950408889634), F32(0.6931471805599453)
HR, MAXN = 4, 128                # spv_head.hip: rows per workgroup, output slots per row


# ------------------------------------------------------------------------------------------------------------------ float32 pieces
def fexp(x):
    """__expf: exp2 of the float32 product x log2(e), a subnormal result flushed"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        r = np.exp2((np.asarray(x, F32) * LOG2E).astype(F32)).astype(F32)
    return np.where(r < TINY_NORMAL, F32(0), r).astype(F32)


def flog(x):
    """__logf: log2 times ln 2"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.log2(np.asarray(x, F32)).astype(F32) * LN2).astype(F32)


def wave_sum(v):
    """the 64 lanes joined by the balanced tree of spv_common.h's wave_sum: [..., 64] -> [...]"""
    v = np.asarray(v, F32)
    assert v.shape[-1] == 64
    with np.errstate(over="ignore", invalid="ignore"):
        while v.shape[-1] > 1:
            v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def seq_sum(v, axis):
    """float32 additions in index order along `axis`, starting from 0"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.add.accumulate(np.asarray(v, F32), axis=axis, dtype=F32).take(-1, axis=axis)


def lane_sum(e):
    """a wave's sum over a row [rows, C]: lane l adds columns l, l + 64, ... in order, then the tree"""
    rows, C = e.shape
    pad = np.zeros((rows, cdiv(C, 64) * 64), F32)
    pad[:, :C] = e
    return wave_sum(seq_sum(pad.reshape(rows, -1, 64), 1))


def join_rows(term, waves, max_wg):
    """the loss kernels' fixed join of per-row terms: wave w of workgroup b adds its rows b waves + w, + grid waves, ... in order, thread
    0 adds the waves in order, the last workgroup joins the partials by the wave tree"""
    term = np.asarray(term, F32)
    rows = term.size
    wgs = min(cdiv(rows, waves), max_wg)
    pad = np.zeros(cdiv(rows, wgs * waves) * wgs * waves, F32)
    pad[:rows] = term
    part = np.zeros(64, F32)
    part[:wgs] = seq_sum(seq_sum(pad.reshape(-1, wgs, waves), 0), 1)
    return wave_sum(part)


def gelu32(x):
    return F32(0.5) * x * (F32(1) + P._erf32(x * F32(P.RSQRT2)))


def gelu_grad32(x):
    with np.errstate(under="ignore"):
        return F32(0.5) * (F32(1) + P._erf32(x * F32(P.RSQRT2))) + x * fexp(F32(-0.5) * x * x) * F32(P.RSQRT2PI)


# ------------------------------------------------------------------------------------------------------------------ A. the class head
def windows(n, k, mutant=None):
    """AdaptiveAvgPool1d(n)'s windows over k columns: [floor(i k / n), ceil((i + 1) k / n))"""
    i = np.arange(n, dtype=np.int64)
    e0 = (i + 1) * k // n if mutant == "pool_end_floor" else -(-(i + 1) * k // n)
    return i * k // n, e0


def pool_matrix(n, k):
    s0, e0 = windows(n, k)
    Pm = np.zeros((n, k))
    for i in range(n):
        Pm[i, s0[i]:e0[i]] = 1.0 / (e0[i] - s0[i])
    return Pm


def head_fwd_ref(xs, W, b, gamma, beta):
    """xs: the summed input as float32 values.  -> dict(h, S_h, mean, rstd, out)"""
    n, k = W.shape
    h = xs @ W.T + b
    mean = h.mean(1)
    var = ((h - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    ln = (h - mean[:, None]) * rstd[:, None] * gamma + beta
    return dict(h=h, S_h=np.abs(xs) @ np.abs(W).T + np.abs(b), mean=mean, rstd=rstd, out=P.gelu_fwd_ref(ln)[0] + xs @ pool_matrix(n, k).T)


def head_bwd_ref(dout, h, xs, mean, rstd, W, gamma, beta, dh_used=None):
    """The backward from the forward's own h, xs, mean, rstd.  S of dgamma / dbeta: the absolute terms of GELU' (1/2, erf / 2, x phi, and
    the two terms of its argument) times |dout| (|xh|), summed over the rows.  dh_used: the dh the kernel itself stored (None: this
    reference's) -- dW, dbias and the matrix part of dx are sums over THAT tensor, so they stay one summation away from float64.
    -> dict(dh, dx_whole, dx, S_dx, dW, S_dW, dgamma, S_dgamma, dbeta, S_dbeta, dbias, S_dbias)"""
    n, k = W.shape
    xh = (h - mean[:, None]) * rstd[:, None]
    ln = xh * gamma + beta
    dl, S_dl = P.gelu_bwd_ref(dout, ln)
    S_dl = S_dl + np.abs(dout) * (np.abs(xh * gamma) + np.abs(beta))        # GELU'' <= 1.13: the rounding of ln's two terms enters as it is
    t = dl * gamma
    dh = rstd[:, None] * (t - t.mean(1)[:, None] - xh * (t * xh).mean(1)[:, None])
    d = dh if dh_used is None else dh_used
    Pm = pool_matrix(n, k)
    return dict(dh=dh + 0.0, dx_whole=dh @ W + dout @ Pm, dx=d @ W + dout @ Pm, S_dx=np.abs(d) @ np.abs(W) + np.abs(dout) @ Pm,
                dW=d.T @ xs, S_dW=np.abs(d).T @ np.abs(xs), dgamma=(dl * xh).sum(0) + 0.0,
                S_dgamma=(S_dl * np.abs(xh)).sum(0), dbeta=dl.sum(0) + 0.0, S_dbeta=S_dl.sum(0), dbias=d.sum(0) + 0.0, S_dbias=np.abs(d).sum(0))


def head_fwd_restate(xa, xb, W, b, gamma, beta, mutant=None):
    """small_sl_fwd_kernel: -> dict(xs, h, mean, rstd, out), float32"""
    xa, W, b, gamma, beta = (np.asarray(a, np.float64).astype(F32) for a in (xa, W, b, gamma, beta))
    xs = xa if xb is None else (xa + np.asarray(xb, np.float64).astype(F32)).astype(F32)
    rows, k = xs.shape
    n = W.shape[0]
    kj = 8 if k <= 512 else (12 if k <= 768 else 16)
    # lane l holds columns l, l + 64, ... (KJ of them); a slot past k loads column k - 1 and is multiplied by 0
    col = np.minimum(np.arange(64 * kj), k - 1)
    live = (np.arange(64 * kj) < k).astype(F32)
    xr = xs[:, col] * (F32(1) if mutant == "mask_dropped" else live)
    wr = W[:, col].reshape(n, kj, 64)
    xr = xr.reshape(rows, kj, 64)
    acc = np.zeros((rows, n, 64), F32)
    for j in range(kj):
        acc = acc + xr[:, None, j, :] * wr[None, :, j, :]
    h = wave_sum(acc) + b
    slots = MAXN if mutant == "stats_128" else n
    hp = np.zeros((rows, MAXN), F32)
    hp[:, :n] = h
    mu = wave_sum(hp[:, :64] + hp[:, 64:]) / F32(slots)
    d = np.where(np.arange(MAXN) < n, hp - mu[:, None], F32(0)).astype(F32)
    dd = d * d
    with np.errstate(divide="ignore", invalid="ignore"):        # the mutant without 1e-5 divides by a zero variance
        rs = F32(1) / np.sqrt(wave_sum(dd[:, :64] + dd[:, 64:]) / F32(slots) + (F32(0) if mutant == "no_eps" else F32(1e-5)), dtype=F32)
        ln = (h - mu[:, None]) * rs[:, None] * gamma + beta
    s0, e0 = windows(n, k, mutant)
    skip = np.empty((rows, n), F32)
    for o in range(n):
        if n == k:
            skip[:, o] = xs[:, o]
        else:
            skip[:, o] = seq_sum(xs[:, s0[o]:e0[o]], 1) / F32(n if mutant == "pool_div_n" else e0[o] - s0[o])
    return dict(xs=xs, h=h, mean=mu, rstd=rs, out=(gelu32(ln) + skip).astype(F32))


def head_bwd_restate(dout, h, xs, mean, rstd, W, gamma, beta, mutant=None, partials=None, dh_in=None):
    """small_sl_bwd_rows_kernel + small_sl_bwd_w_kernel: -> dict(dh, dx, partials, dW, dgamma, dbeta, dbias), float32 (dx before its
    storage rounding).  partials / dh_in: the weights launch on its own, fed these."""
    dout, h, xs, mean, rstd, W, gamma, beta = (np.asarray(a, np.float64).astype(F32) for a in (dout, h, xs, mean, rstd, W, gamma, beta))
    rows, n = h.shape
    k = W.shape[1]
    with np.errstate(invalid="ignore"):
        xh = (h - mean[:, None]) * rstd[:, None]
    dl = dout * gelu_grad32(xh * gamma + beta)
    t = dl * gamma

    def row_mean(v):
        p = np.zeros((rows, MAXN), F32)
        p[:, :n] = v
        return wave_sum(p[:, :64] + p[:, 64:]) / F32(n)
    dh = (rstd[:, None] * (t - row_mean(t)[:, None] - xh * row_mean(t * xh)[:, None])).astype(F32)
    nparts = cdiv(rows, HR)
    if partials is None:
        three = np.zeros((nparts * HR, 3, n), F32)
        three[:rows, 0], three[:rows, 1], three[:rows, 2] = dl * xh, dl, dh
        partials = seq_sum(three.reshape(nparts, HR, 3, n), 1)
    else:
        partials = np.asarray(partials, np.float64).astype(F32).reshape(nparts, 3, n)
    # dx: thread (column c, slice q) adds outputs q, q + nq, ... in order; the slices meet in order; then the transposed pooling
    cols = min(k, 1024)
    nq = 1024 // cols
    sl = np.zeros((min(nq, n), rows, k), F32)
    for o in range(n):
        sl[o % nq] = sl[o % nq] + dh[:, o, None] * W[o][None, :]
    dx = seq_sum(sl, 0)
    if n == k:
        dx = dx + dout
    else:
        s0, e0 = windows(n, k)
        i0 = np.arange(k, dtype=np.int64) * n // k
        for di in {"no_i0_minus_1": (0, 1), "no_i0_plus_1": (-1, 0)}.get(mutant, (-1, 0, 1)):
            i = i0 + di
            ic = np.clip(i, 0, n - 1)
            inside = (i >= 0) & (i < n) & (np.arange(k) >= s0[ic]) & (np.arange(k) < e0[ic])
            inv = (F32(1) / (e0[ic] - s0[ic]).astype(F32)).astype(F32)
            dx = np.where(inside, dx + dout[:, ic] * inv, dx).astype(F32)
    # dW: row group g takes rows g, g + 8, ... in order; the groups meet in order
    d = dh if dh_in is None else np.asarray(dh_in, np.float64).astype(F32)
    steps = cdiv(rows, 8)
    dp, xp = np.zeros((steps * 8, n), F32), np.zeros((steps * 8, k), F32)
    dp[:rows], xp[:rows] = d, xs
    acc = np.zeros((8, n, k), F32)
    for s in range(steps):
        acc = acc + dp[8 * s:8 * s + 8, :, None] * xp[8 * s:8 * s + 8, None, :]
    dW = seq_sum(acc, 0)
    # the fold: slice q adds partials q, q + 16, ... in order; the 16 slices meet in order
    pp = np.zeros((cdiv(nparts, 16) * 16, 3, n), F32)
    pp[:nparts] = partials
    fold = seq_sum(seq_sum(pp.reshape(-1, 16, 3, n), 0), 0)
    return dict(dh=dh, dx=dx, partials=partials, dW=dW, dgamma=fold[0], dbeta=fold[1], dbias=fold[2])


# ------------------------------------------------------------------------------------------------------------------ log-sum-exp
def lse_ref(z):
    """(lse, S) per row of z [rows, C]: lse = m + log s, s = sum exp(z - m); S = |m| + |log s| for the last addition, plus the relative
    error of s, which enters log s absolutely: each term exp(z_c - m) carries its own rounding and that of its argument"""
    z = np.asarray(z, np.float64)
    m = z.max(1)
    with np.errstate(under="ignore"):
        e = np.exp(z - m[:, None])
    s = e.sum(1)
    return m + np.log(s), np.abs(m) + np.abs(np.log(s)) + (e * (1.0 + np.abs(z - m[:, None]))).sum(1) / s


def softmax_terms(arg_minus_lse):
    """(p, p (1 + |a - lse|)): a probability exp(a - lse) and the absolute terms of its own error"""
    with np.errstate(under="ignore"):
        p = np.exp(arg_minus_lse)
    return p, p * (1.0 + np.abs(arg_minus_lse))


# ------------------------------------------------------------------------------------------------------------------ B. cross-entropy
def ce_ref(z, labels, go):
    """-> dict(lse, S_lse, loss, S_loss, dz, S_dz, prop): dz's bar adds prop (= p |scale|) times the lse bar"""
    z, labels = np.asarray(z, np.float64), np.asarray(labels, np.int64)
    rows, C = z.shape
    lse, S_lse = lse_ref(z)
    ok = (labels >= 0) & (labels < C)
    zy = z[np.arange(rows), np.clip(labels, 0, C - 1)]
    loss = (lse - zy).sum() / rows if ok.all() else np.nan
    scale = go / rows
    p, sp = softmax_terms(z - lse[:, None])
    onehot = (labels[:, None] == np.arange(C)[None, :]).astype(np.float64)
    return dict(lse=lse, S_lse=S_lse, loss=np.array([loss]), S_loss=np.array([(S_lse + np.abs(zy)).sum() / rows]), dz=(p - onehot) * scale,
                S_dz=(sp + onehot) * abs(scale), prop=p * abs(scale))


CE_WAVES, CE_MAX_WG, CE_BWD_SWEEP = 16, 64, 1024 * 1024


def ce_fwd_restate(z, labels, mutant=None):
    z, labels = np.asarray(z, np.float64).astype(F32), np.asarray(labels, np.int64)
    rows, C = z.shape
    m = np.zeros(rows, F32) if mutant == "no_max_shift" else z.max(1)
    with np.errstate(over="ignore", invalid="ignore"):
        lse = (m + flog(lane_sum(fexp(z - m[:, None])))).astype(F32)
        ok = (labels >= 0) & (labels < C)
        term = np.where(ok, lse - z[np.arange(rows), np.clip(labels, 0, C - 1)], F32(np.nan)).astype(F32)
        if mutant == "first_sweep_only":
            first = min(cdiv(rows, CE_WAVES), CE_MAX_WG) * CE_WAVES
            lse[first:], term[first:] = np.nan, 0
        total = join_rows(term, CE_WAVES, CE_MAX_WG)
    return dict(lse=lse, loss=np.array([total if mutant == "no_div_rows" else total / F32(rows)], F32))


def ce_bwd_restate(z, labels, lse, go, mutant=None):
    z, labels, lse = np.asarray(z, np.float64).astype(F32), np.asarray(labels, np.int64), np.asarray(lse, np.float64).astype(F32)
    rows, C = z.shape
    scale = F32(go) if mutant == "no_div_rows" else F32(go) / F32(rows)
    onehot = (labels[:, None] == np.arange(C)[None, :]).astype(F32)
    dz = ((fexp(z - lse[:, None]) - (F32(0) if mutant == "no_onehot" else onehot)) * scale).astype(F32)
    if mutant == "first_sweep_only":
        dz.reshape(-1)[CE_BWD_SWEEP:] = np.nan
    return dict(dz=dz)


# ------------------------------------------------------------------------------------------------------------------ C. distillation
def nearby_rows(z, t, T):
    """the forward's rule per row: max |t - z| / T < 1/2 takes the log1p / expm1 form"""
    return (np.abs(np.asarray(t, np.float64) - np.asarray(z, np.float64)) / T).max(1) < 0.5


def distill_ref(z, t, labels, T, w_soft, w_ce, go):
    """-> dict(lse3, S_lse3 [3, rows]; soft_rows, S_soft_rows; out3, S_out3 [3] (S_out3[0] unused: out3[0]'s bar is built from the other
    two); dz, S_dz, prop3 [3, rows, C]: dz's bar adds prop3[i] times the bar of lse3[i])"""
    z, t, labels = np.asarray(z, np.float64), np.asarray(t, np.float64), np.asarray(labels, np.int64)
    rows, C = z.shape
    (lz, S_lz), (lzt, S_lzt), (ltt, S_ltt) = lse_ref(z), lse_ref(z / T), lse_ref(t / T)
    az, bt = (z - z.max(1)[:, None]) / T, (t - t.max(1)[:, None]) / T
    with np.errstate(under="ignore"):
        ez, et = np.exp(az), np.exp(bt)
    s2, s3 = ez.sum(1), et.sum(1)
    q, p = ez / s2[:, None], et / s3[:, None]
    d = (t - z) / T
    near = nearby_rows(z, t, T)
    u = bt - az
    # the value, shifted form in float64 (a teacher probability that underflows contributes its limit 0)
    soft = (p * u).sum(1) - (np.log(s3) - np.log(s2))
    # the absolute terms of the form the kernel takes (the other form's may overflow: not used)
    old = np.seterr(over="ignore", invalid="ignore")
    x = (q * np.expm1(d)).sum(1)
    S_near = (p * np.abs(d) * (1 + np.abs(bt))).sum(1) + (q * np.abs(np.expm1(d)) * (1 + np.abs(az))).sum(1) / (1 + x) + \
        np.abs((p * d).sum(1)) + np.abs(np.log1p(x))
    S_gen = (p * np.abs(u) * (1 + np.abs(bt))).sum(1) + np.abs((p * u).sum(1)) + 2 * np.abs(np.log(s3)) + 2 * np.abs(np.log(s2)) + \
        (p * (1 + np.abs(bt))).sum(1) + (q * (1 + np.abs(az))).sum(1)
    S_soft = np.where(near, S_near, S_gen)
    np.seterr(**old)
    ok = (labels >= 0) & (labels < C)
    zy = z[np.arange(rows), np.clip(labels, 0, C - 1)]
    ce = (lz - zy).sum() / rows if ok.all() else np.nan
    soft_mean = soft.sum() * T * T / rows
    out3 = np.array([w_soft * soft_mean + w_ce * ce, soft_mean, ce])
    S_out3 = np.array([0.0, (S_soft + np.abs(soft)).sum() * T * T / rows, (S_lz + np.abs(zy)).sum() / rows])
    scale, ks = go / rows, w_soft * T
    (qq, sq), (pp, sp), (ss, s_s) = softmax_terms(z / T - lzt[:, None]), softmax_terms(t / T - ltt[:, None]), softmax_terms(z - lz[:, None])
    onehot = (labels[:, None] == np.arange(C)[None, :]).astype(np.float64)
    return dict(lse3=np.stack([lz, lzt, ltt]), S_lse3=np.stack([S_lz, S_lzt, S_ltt]), soft_rows=soft, S_soft_rows=S_soft, out3=out3, S_out3=S_out3,
                dz=scale * (ks * (qq - pp) + w_ce * (ss - onehot)), S_dz=abs(scale) * (abs(ks) * (sq + sp) + abs(w_ce) * (s_s + onehot)),
                prop3=abs(scale) * np.stack([abs(w_ce) * ss, abs(ks) * qq, abs(ks) * pp]))


DL_WAVES, DL_MAX_WG, DL_BWD_SWEEP = 4, 64, 256 * 1024


def distill_fwd_restate(z, t, labels, T, w_soft, w_ce, mutant=None):
    """distill_fwd_body in float32: -> dict(lse3 [3, rows], out3 [3])"""
    z, t, labels = np.asarray(z, np.float64).astype(F32), np.asarray(t, np.float64).astype(F32), np.asarray(labels, np.int64)
    rows, C = z.shape
    T, invT = F32(T), F32(1) / F32(T)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        mz, mt = z.max(1), t.max(1)
        d = (t - z) * invT
        near = np.abs(d).max(1) < F32(0.5)
        near = np.ones_like(near) if mutant == "nearby_always" else np.zeros_like(near) if mutant == "nearby_never" else near
        az, bt = (z - mz[:, None]) * invT, (t - mt[:, None]) * invT
        ez, et = np.exp(az), np.exp(bt)
        s1, s2, s3 = lane_sum(np.exp(z - mz[:, None])), lane_sum(ez), lane_sum(et)
        pu = lane_sum(et * np.where(near[:, None], d, bt - az))
        qe = lane_sum(ez * np.expm1(np.where(near[:, None], d, F32(0))))
        lz, lzt, ltt = mz + np.log(s1), mz * invT + np.log(s2), mt * invT + np.log(s3)
        gap = np.where(near, np.log1p(qe / s2), np.log(s3) - np.log(s2)).astype(F32)
        soft_rows = (pu / s3 - gap).astype(F32)
        ok = (labels >= 0) & (labels < C)
        ce_rows = np.where(ok, lz - z[np.arange(rows), np.clip(labels, 0, C - 1)], F32(np.nan)).astype(F32)
        if mutant == "first_sweep_only":
            first = min(cdiv(rows, DL_WAVES), DL_MAX_WG) * DL_WAVES
            lz[first:], lzt[first:], ltt[first:], soft_rows[first:], ce_rows[first:] = np.nan, np.nan, np.nan, 0, 0
        a, b = join_rows(soft_rows, DL_WAVES, DL_MAX_WG), join_rows(ce_rows, DL_WAVES, DL_MAX_WG)
        soft = (a if mutant == "no_T2" else a * (T * T)) / F32(rows)
        ce = b / F32(rows)
        total = F32(w_soft) * soft + F32(w_ce) * ce
    return dict(lse3=np.stack([lz, lzt, ltt]).astype(F32), out3=np.array([total, soft, ce], F32))


def distill_bwd_restate(z, t, labels, lse3, T, w_soft, w_ce, go, mutant=None):
    z, t, lse3 = (np.asarray(a, np.float64).astype(F32) for a in (z, t, lse3))
    labels = np.asarray(labels, np.int64)
    rows, C = z.shape
    scale, invT, ks = F32(go) / F32(rows), F32(1) / F32(T), F32(w_soft) * F32(T)
    onehot = (labels[:, None] == np.arange(C)[None, :]).astype(F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        q, p, s = np.exp(z * invT - lse3[1][:, None]), np.exp(t * invT - lse3[2][:, None]), np.exp(z - lse3[0][:, None])
        dz = ((ks * (q - p) + F32(w_ce) * (s - (F32(0) if mutant == "no_onehot" else onehot))) * scale).astype(F32)
    if mutant == "first_sweep_only":
        dz.reshape(-1)[DL_BWD_SWEEP:] = np.nan
    return dict(dz=dz)


# ------------------------------------------------------------------------------------------------------------------ D. the eval head
def eval_ref(z, labels, n_valid, k, stats=None):
    """include/spv.h's counting rules on storage values z (float64): -> (pred, stats, S_loss).  pred: meter_ref's first ordered maximum
    (a NaN never wins, an all-NaN row predicts 0); counted rows hold no NaN."""
    z, labels = np.asarray(z, np.float64), np.asarray(labels, np.int64)
    rows, C = z.shape
    stats = dict(stats) if stats is not None else E.new_stats()
    pred = M.predictions(z)
    batch, S = 0.0, 0.0
    for r in range(max(0, min(int(n_valid), rows))):
        y = int(labels[r])
        if not 0 <= y < C:
            continue
        assert not np.isnan(z[r]).any()
        stats["seen"] += 1
        stats["top1"] += int(pred[r] == y)
        stats["topk"] += int(E.topk_hit(z[r], y, k))
        batch += E.row_loss(z[r], y)
        S += float(lse_ref(z[r:r + 1])[1][0]) + abs(z[r, y])
    stats["loss_sum"] += batch
    return pred, stats, S


EW, E_MAX_WG = 8, 64


def eval_restate(z, labels, n_valid, k, mutant=None):
    """eval_head_kernel on storage values: -> (pred int64 [rows] (-7: unwritten), dict(seen, top1, topk, loss_sum))"""
    z, labels = np.asarray(z, np.float64).astype(F32), np.asarray(labels, np.int64)
    rows, C = z.shape
    nv = rows if mutant == "n_valid_ignored" else min(max(int(n_valid), 0), rows)
    wgs = min(cdiv(rows, EW), E_MAX_WG)
    pred = np.full(rows, -7, np.int64)
    seen = top1 = topk = 0
    wave_loss = np.zeros((wgs, EW))
    cols = np.arange(C)
    for r in range(rows):
        if mutant == "first_sweep_only" and r >= wgs * EW:
            break
        y = int(labels[r])
        counted = r < nv and 0 <= y < C
        zy = z[r, y if counted else 0]
        with np.errstate(invalid="ignore"):
            wm = np.fmax.reduce(z[r]) if not np.isnan(z[r]).all() else F32(-np.inf)
            at = np.nonzero(z[r] == wm)[0]
            first = 0 if wm == -np.inf or at.size == 0 else int(at[-1] if mutant == "last_max" else at[0])
            pred[r] = first
            if not counted:
                continue
            l = wm + np.log(lane_sum(np.exp(z[r:r + 1] - wm))[0]) - zy
            ahead = {"tie_le": cols <= y, "tie_ignored": cols < 0, "tie_gt": cols > y, "tie_all": cols != y}.get(mutant, cols < y)
            above = int(((z[r] > zy) | ((z[r] == zy) & ahead)).sum())
        seen, top1, topk = seen + 1, top1 + int(first == y), topk + int(above < k)
        b, w = (r // EW) % wgs, r % EW
        wave_loss[b, w] += float(F32(l))
    return pred, dict(seen=seen, top1=top1, topk=topk, loss_sum=float(sum(float(sum(wave_loss[b])) for b in range(wgs))))
