"""float32 numpy restatements of the two update rules beside AdamW (include/spv.h: spv_sgd_multi, spv_adam_multi), written from
torch.optim.SGD's and torch.optim.Adam's definitions and independent of spectre_vit.optim, and the tensor list the optimizer tests
walk.

sgd_ref rounds every operation on its own in float32, in the order the header gives; the kernel does the same on its vector and on
its scalar walk, so the two agree bit for bit.  adam_ref is the float32 rule without fused operations; the kernel's two walks fuse
different pairs (as AdamW's do), so it is held to float64 torch at a tolerance, not to this restatement bit for bit."""
import numpy as np
import torch

# a scalar, sub-vector tails, an exact 2048-element chunk, chunk + 1, an unaligned tail, a multi-chunk tensor ...
SHAPES = [(1,), (3,), (5,), (2048,), (2049,), (4095,), (65, 512)]
OFFSET_N = 1029   # ... and one tensor (parameter AND gradient) behind a one-element storage offset: 4 bytes off alignment
SIZES = [int(np.prod(s)) for s in SHAPES] + [OFFSET_N]
RTOL, ATOL = 2e-6, 2e-7   # the optimizer tests' bounds against float64 torch

f32 = np.float32


def offset_view(values):
    """a contiguous tensor holding `values` whose data pointer is 4 bytes past a 16-byte boundary (on the GPU; any offset on the CPU)"""
    buf = torch.empty(values.numel() + 1, device=values.device, dtype=values.dtype)
    v = buf[1:].view(values.shape)
    v.copy_(values)
    assert v.is_contiguous() and (not v.is_cuda or v.data_ptr() % 16 == 4)
    return v


def make_params(seed, dev="cuda", dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g).to(dev, dtype).requires_grad_(True) for s in SHAPES]
    ps.append(offset_view(torch.randn(OFFSET_N, generator=g).to(dev, dtype)).requires_grad_(True))
    return ps


def clone_params(ps):
    return [(offset_view(p.detach()) if p.data_ptr() % 16 else p.detach().clone()).requires_grad_(True) for p in ps]


def make_grads(gen, scale, dev="cuda"):
    return [torch.randn(s, generator=gen).to(dev) * scale for s in SHAPES + [(OFFSET_N,)]]


def set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = offset_view(g) if p.data_ptr() % 16 else g.clone()


def bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().view(-1).numpy()
    return np.ascontiguousarray(t, dtype=np.float32).reshape(-1).view(np.uint32)


def sgd_ref(p, g, buf, count, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, gscale=None):
    """one step of torch.optim.SGD on float32 arrays; count = the group's count of applied steps INCLUDING this one (1: buf = d).
    Returns (p', buf'); buf is passed through untouched with momentum == 0."""
    assert p.dtype == g.dtype == np.float32
    lr, mom, wd = f32(lr), f32(momentum), f32(weight_decay)
    omd = f32(1.0 - float(dampening))   # formed in double, rounded once
    d = g if gscale is None else g * f32(gscale)
    if wd != 0:
        t = wd * p
        d = d + t
    if mom != 0:
        if count == 1:
            buf = d.copy()
        else:
            t1 = mom * buf
            t2 = omd * d
            buf = t1 + t2
        if nesterov:
            t = mom * buf
            d = d + t
        else:
            d = buf
    t = lr * d
    out = p - t
    assert out.dtype == np.float32
    return out, buf


def adam_ref(p, g, m, v, count, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """one step of torch.optim.Adam (L2 decay in the gradient, amsgrad off) on float32 arrays, count = this step's number (1 first)"""
    b1, b2 = f32(betas[0]), f32(betas[1])
    omb1, omb2 = f32(1.0 - betas[0]), f32(1.0 - betas[1])
    lr, eps, wd = f32(lr), f32(eps), f32(weight_decay)
    d = g
    if wd != 0:
        d = d + wd * p
    m = b1 * m + omb1 * d
    v = b2 * v + omb2 * d * d
    bc1 = f32(1.0) - np.power(b1, f32(count))
    bc2 = f32(1.0) - np.power(b2, f32(count))
    step_size = lr / bc1
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    p = p - step_size * m / denom
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v

