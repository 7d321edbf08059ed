"""SpectreBranch ops (reference spectre_branch/spectre_branch.py:92-173): spectrum, 3x3 conv chain, token pooling, the two-half
projection.  Same contract as hip_ops: borrowed ``data_ptr()``s, torch's current HIP stream, no synchronisation, no CPU fallback."""
from __future__ import annotations

import torch

from . import _native, shadows
from ._launch import _DT, F32, _dt, _p, _require_gpu, _stream
from .hip_ops import _colsum, _gemm, _gemm_launch, _grad_buf, _raw_cast, _sink


def _r8(v):
    return (v + 7) // 8 * 8


def _wgrad_into(dh, x, rows, n, k, out, ldc, ldx=None):
    """out[n, k] (leading dimension ldc, fp32) = dh[rows, n]^T . x[rows, k] (x's leading dimension ldx >= k), split-K and folded in
    a fixed order, written NOW (never held for the end-of-backward batch: the caller may hand a view of a larger gradient)"""
    ldx = k if ldx is None else ldx
    dev = dh.device
    tiles = ((n + 127) // 128) * ((k + 127) // 128)
    splits = max(1, min(512 // tiles, (rows + 511) // 512 if tiles >= 8 else (rows + 63) // 64, 64))
    ws = torch.empty((splits * n * k,), dtype=torch.float32, device=dev) if splits > 1 else None
    st = _stream()
    if dh.dtype == torch.bfloat16 and n % 8 == 0 and k % 8 == 0 and ldx % 8 == 0:
        _native.call("spv_gemm_tn", _p(dh), _p(x), _p(out), n, k, rows, n, ldx, ldc, F32, 0, splits, _p(ws), st)
        return out
    ld = _r8(rows)
    dht = torch.empty((n, ld), dtype=dh.dtype, device=dev)
    xt = torch.empty((ldx, ld), dtype=x.dtype, device=dev)
    _native.call("spv_cast_transpose", _p(dh), _dt(dh), _p(dht), _dt(dht), rows, n, ld, 0, 0, 0, st)
    _native.call("spv_cast_transpose", _p(x), _dt(x), _p(xt), _dt(xt), rows, ldx, ld, 0, 0, 0, st)
    _native.call("spv_gemm_nt", _p(dht), _p(xt), 0, _p(out), n, k, ld, ld, ld, ldc, _dt(dht), F32, 0, splits, _p(ws), st)
    return out


def spectrum_log1p(img, dtype=torch.float32):
    """log1p(|rfft2(img)|) of fp32 NCHW images, channels-last (B, H, W//2+1, C) in `dtype` (spectre_branch.py:151).  Forward only."""
    _require_gpu(img)
    if img.requires_grad:
        raise RuntimeError("spectrum_log1p: the SpectreBranch spectrum has no backward (gradients to the input image are not built)")
    if img.dtype != torch.float32 or img.dim() != 4:
        raise TypeError(f"spectrum_log1p takes fp32 (B, C, H, W) images, got {img.dtype} {tuple(img.shape)}")
    img = img.contiguous()
    B, C, H, W = img.shape
    out = torch.empty((B, H, W // 2 + 1, C), dtype=dtype, device=img.device)
    _native.call("spv_spectrum_log1p", _p(img), _p(out), B, C, H, W, _DT[dtype], _stream())
    return out


def conv3x3_fwd(x, weight, bias):
    """valid 3x3 stride-1 conv of channels-last x (B, H, W, Cin) -> (B, H-2, W-2, Cout) in x's dtype (spectre_branch.py:133)"""
    _require_gpu(x, weight)
    B, H, W, cin = x.shape
    cout = weight.shape[0]
    kp = _r8(9 * cin)
    wpack = torch.zeros((cout, kp), dtype=x.dtype, device=x.device)
    wpack[:, :9 * cin] = weight.detach().reshape(cout, 9 * cin)
    cols = torch.empty(((B * (H - 2) * (W - 2)) * kp,), dtype=x.dtype, device=x.device)
    y = torch.empty((B, H - 2, W - 2, cout), dtype=x.dtype, device=x.device)
    _native.call("spv_conv3x3_fwd", _p(x), _p(wpack), _p(bias), _p(y), _p(cols), B, H, W, cin, cout, _dt(x), _stream())
    return y


def conv3x3_dgrad(dy, weight):
    """input gradient (B, H, W, Cin) of conv3x3_fwd from dy (B, H-2, W-2, Cout): the full correlation with the kernel"""
    B, ho, wo, cout = dy.shape
    cin = weight.shape[1]
    kd = _r8(9 * cout)
    wd = torch.zeros((cin, kd), dtype=dy.dtype, device=dy.device)
    wd[:, :9 * cout] = weight.detach().transpose(0, 1).reshape(cin, 9 * cout)
    H, W = ho + 2, wo + 2
    cols = torch.empty((B * H * W * kd,), dtype=dy.dtype, device=dy.device)
    dx = torch.empty((B, H, W, cin), dtype=dy.dtype, device=dy.device)
    _native.call("spv_conv3x3_dgrad", _p(dy), _p(wd), _p(dx), _p(cols), B, H, W, cin, cout, _dt(dy), _stream())
    return dx


def conv3x3_wgrad(dy, x, out=None):
    """weight gradient (Cout, Cin, 3, 3) fp32 of conv3x3_fwd: dy^T . im2col(x) over every output position, split and folded in order"""
    B, H, W, cin = x.shape
    cout = dy.shape[-1]
    M = B * (H - 2) * (W - 2)
    mp = _r8(M)
    k = 9 * cin
    dev = x.device
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=dev) if out is None else out
    tiles = ((cout + 127) // 128) * ((k + 127) // 128)
    splits = max(1, min(256 // tiles, mp // 1024, 256))
    ws = torch.empty((splits * cout * k,), dtype=torch.float32, device=dev) if splits > 1 else None
    dyt = torch.empty((cout * mp,), dtype=dy.dtype, device=dev)
    colst = torch.empty((k * mp,), dtype=x.dtype, device=dev)
    _native.call("spv_conv3x3_wgrad", _p(dy), _p(x), _p(dw), _p(dyt), _p(colst), _p(ws), splits, B, H, W, cin, cout, _dt(x), _stream())
    return dw


def token_pool_fwd(y, tokens, ldo=None):
    """AdaptiveAvgPool1d(tokens) over the flattened map of channels-last y (B, H, W, C) -> (B, tokens, ldo), columns >= C zero"""
    _require_gpu(y)
    B, C = y.shape[0], y.shape[-1]
    L = y.numel() // (B * C)
    ldo = C if ldo is None else ldo
    out = torch.empty((B, tokens, ldo), dtype=y.dtype, device=y.device)
    _native.call("spv_token_pool_fwd", _p(y), _p(out), B, L, C, tokens, ldo, _dt(y), _stream())
    return out


def token_pool_bwd(dout, L, C, add=None):
    """transpose of token_pool_fwd: dout (B, T, ldo) -> (B, L, C) (+ add)"""
    _require_gpu(dout)
    B, T, ldo = dout.shape
    dy = torch.empty((B, L, C), dtype=dout.dtype, device=dout.device)
    _native.call("spv_token_pool_bwd", _p(dout), ldo, _p(add), _p(dy), B, L, C, T, _dt(dout), _stream())
    return dy


class BranchFeatFn(torch.autograd.Function):
    """SpectreFeatExtractor.forward (spectre_branch.py:147-173) as one autograd node: (x_last, feats[0..S-1]).

    Pool first, then project: pool(W y + b) = W pool(y) + b (a window averages the constant bias to itself), so each 1x1 projection
    is a (B T, C_k) x (C_k, E) GEMM on the pooled map and the (B, E, H'W') maps are never built.  Backward runs from the last stage
    to the first: d y_k = unpool(dFeat_k W_k) + dgrad(conv_{k+1}), then conv k's weight / bias gradients and its data gradient.
    x_last (channels-last storage, NCHW view) carries no gradient."""

    @staticmethod
    def forward(ctx, img, tokens, dtype, *params):
        S = len(params) // 4
        convs = [(params[2 * i], params[2 * i + 1]) for i in range(S)]
        projs = [(params[2 * S + 2 * i], params[2 * S + 2 * i + 1]) for i in range(S)]
        x = spectrum_log1p(img, dtype)
        B = x.shape[0]
        xs, pooled, wps, feats = [], [], [], []
        for (cw, cb), (pw, pb) in zip(convs, projs):
            y = conv3x3_fwd(x, cw, cb)
            cout, E = y.shape[-1], pw.shape[0]
            ldo = _r8(cout)
            pk = token_pool_fwd(y, tokens, ldo)
            wp = torch.zeros((E, ldo), dtype=dtype, device=x.device)
            wp[:, :cout] = pw.detach().reshape(E, cout)
            f = torch.empty((B, tokens, E), dtype=dtype, device=x.device)
            _gemm(pk, wp, pb, f, B * tokens, E, ldo, ldo, ldo, E)
            xs.append(x)
            pooled.append(pk)
            wps.append(wp)
            feats.append(f)
            x = y
        ctx.saved = (xs, pooled, wps, [cw for cw, _ in convs], [t.shape for t in xs[1:] + [x]])
        ctx.sinks = [(_sink(cw), _sink(cb)) for cw, cb in convs] + [(_sink(pw), _sink(pb)) for pw, pb in projs]
        ctx.meta = (S, tokens, B)
        x_last = x.permute(0, 3, 1, 2)
        ctx.mark_non_differentiable(x_last)
        return (x_last, *feats)

    @staticmethod
    def backward(ctx, _dx_last, *dfeats):
        xs, pooled, wps, cws, yshapes = ctx.saved
        S, T, B = ctx.meta
        dev, dt = xs[0].device, xs[0].dtype
        conv_grads, proj_grads = [None] * (2 * S), [None] * (2 * S)
        g_next = None
        for k in range(S - 1, -1, -1):
            _, ho, wo, cout = yshapes[k]
            E, ldo = wps[k].shape
            rows = B * T
            df = dfeats[k]
            df = torch.zeros((rows, E), dtype=dt, device=dev) if df is None else df.reshape(rows, E)
            df = _raw_cast(df, dt) if df.dtype != dt else df.contiguous()
            dpool = torch.empty((B, T, ldo), dtype=dt, device=dev)
            wpt = wps[k].t().contiguous()
            _gemm(df, wpt, None, dpool, rows, ldo, E, E, E, ldo)
            (sw, sb), (spw, spb) = ctx.sinks[k], ctx.sinks[S + k]
            dpw = _grad_buf(spw, (E, cout, 1, 1), dev)
            _wgrad_into(df, pooled[k], rows, E, cout, dpw, cout, ldo)
            dpb = _colsum(df, _grad_buf(spb, (E,), dev))
            dy = token_pool_bwd(dpool, ho * wo, cout, g_next).view(B, ho, wo, cout)
            dw = conv3x3_wgrad(dy, xs[k], _grad_buf(sw, tuple(cws[k].shape), dev))
            db = _colsum(dy.reshape(-1, cout), _grad_buf(sb, (cout,), dev))
            conv_grads[2 * k], conv_grads[2 * k + 1] = dw, db
            proj_grads[2 * k], proj_grads[2 * k + 1] = dpw, dpb
            g_next = conv3x3_dgrad(dy, cws[k]) if k > 0 else None
        return (None, None, None, *conv_grads, *proj_grads)


def branch_features(img, convs, projs, tokens, dtype):
    """(x_last, [feats]) of the SpectreFeatExtractor: convs / projs = [(weight, bias)] per stage"""
    _require_gpu(img, *[w for w, _ in convs])
    params = [t for wb in convs for t in wb] + [t for wb in projs for t in wb]
    out = BranchFeatFn.apply(img, tokens, dtype, *params)
    return out[0], list(out[1:])


class BranchProjectFn(torch.autograd.Function):
    """spectre_project[i](cat([x, feat], -1)) (+ src) (spectre_branch.py:113-119) without the concat: two NT GEMMs into one output over
    the column halves of W (ldb = 2E, the second accumulating); backward writes dx and dfeat from the two halves of W^T and the two
    dW halves through ldc = 2E.  `src` (the encoder's global residual, :119) is folded into the last projection's output."""

    @staticmethod
    def forward(ctx, x, feat, weight, bias, src):
        _require_gpu(x, feat, weight)
        n, k2 = weight.shape
        k = k2 // 2
        dt = x.dtype
        x2, f2 = x.reshape(-1, k).contiguous(), _raw_cast(feat, dt).reshape(-1, k) if feat.dtype != dt else feat.reshape(-1, k).contiguous()
        rows = x2.shape[0]
        wc, wt = shadows.get(weight, dt)
        out = torch.empty((rows, n), dtype=dt, device=x2.device)
        acc = 0
        if src is not None:
            out.copy_(src.reshape(rows, n))
            acc = 1
        _gemm_launch(x2, wc, bias, out, rows, n, k, k, k2, n, acc)
        _gemm_launch(f2, wc[:, k:], None, out, rows, n, k, k, k2, n, 1)
        ctx.saved = (x2, f2, wt, (_sink(weight), _sink(bias)), x.shape, feat.dtype, rows, n, k, src is not None)
        return out.reshape(*x.shape[:-1], n)

    @staticmethod
    def backward(ctx, dout):
        x2, f2, wt, sinks, shape, fdt, rows, n, k, has_src = ctx.saved
        d2 = dout.reshape(rows, n)
        d2 = _raw_cast(d2, x2.dtype) if d2.dtype != x2.dtype else d2.contiguous()
        dev = x2.device
        dx = torch.empty_like(x2)
        df = torch.empty_like(f2)
        _gemm(d2, wt, None, dx, rows, k, n, n, wt.shape[1], k)
        _gemm(d2, wt[k:], None, df, rows, k, n, n, wt.shape[1], k)
        dw = _grad_buf(sinks[0], (n, 2 * k), dev)
        _wgrad_into(d2, x2, rows, n, k, dw, 2 * k)
        _wgrad_into(d2, f2, rows, n, k, dw[:, k:], 2 * k)
        db = _colsum(d2, _grad_buf(sinks[1], (n,), dev))
        dsrc = d2.reshape(shape) if has_src else None
        return dx.reshape(shape), df.reshape(shape), dw, db, dsrc


def branch_project(x, feat, weight, bias, src=None):
    return BranchProjectFn.apply(x, feat, weight, bias, src)
