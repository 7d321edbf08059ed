"""numpy restatement of the training transform chain (include/spv.h): the seven ops of reference
spectre_vit/repl/train.py:100-115 as torchvision defines them on float tensors, taking the same per-sample parameter table as
spv_augment_u8.  Every op works in `dtype` (float64 = the reference of the GPU tests, float32 = the run that sizes their tolerance).
A plain helper module: imported by tests/test_augment.py and tests/test_gpu_augment.py."""
import math

import numpy as np

NPARAM = 16
FLIP, BRIGHT, CONTRAST, SAT, HUE, ORDER, GRAY, ANGLE, BLUR, SIGMA, ERASE_I, ERASE_J, ERASE_H, ERASE_W = range(14)
TIE = 1e-3   # a rotation source coordinate this close to an integer is a rounding tie: the pixel is left out of comparisons


def identity_params(batch):
    p = np.zeros((batch, NPARAM), np.float32)
    p[:, [BRIGHT, CONTRAST, SAT, SIGMA]] = 1.0
    return p


def order_of(index):
    """the index-th permutation of (0 brightness, 1 contrast, 2 saturation, 3 hue) in lexicographic order"""
    import itertools
    return list(itertools.permutations(range(4)))[int(index)]


def grey(x):
    """x (C, H, W) -> (H, W): torchvision's rgb_to_grayscale weights; one channel is its own grey"""
    if x.shape[0] == 1:
        return x[0]
    return 0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]


def clamp(x):
    return np.minimum(np.maximum(x, 0.0), 1.0)


def brightness(x, f):
    return clamp(x * f)


def contrast(x, f):
    m = grey(x).mean(dtype=x.dtype)
    return clamp(f * x + (1.0 - f) * m)


def saturation(x, f):
    if x.shape[0] == 1:
        return x
    return clamp(f * x + (1.0 - f) * grey(x)[None])


def rgb_to_hsv(x):
    """torchvision's _rgb2hsv (hexcone); x (3, ...) -> h, s, v"""
    r, g, b = x[0], x[1], x[2]
    one = np.ones_like(r)
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    flat = d == 0
    s = np.where(flat, 0.0 * one, d / np.where(flat, one, mx))
    dd = np.where(flat, one, d)
    rc, gc, bc = (mx - r) / dd, (mx - g) / dd, (mx - b) / dd
    h6 = np.where(mx == r, bc - gc, np.where(mx == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = h6 / 6.0 + 1.0
    return h - np.floor(h), s, mx


def hsv_to_rgb(h, s, v):
    """torchvision's _hsv2rgb"""
    h6 = h * 6.0
    fi = np.floor(h6)
    f = h6 - fi
    i = fi.astype(np.int64) % 6
    p, q, t = clamp(v * (1.0 - s)), clamp(v * (1.0 - s * f)), clamp(v * (1.0 - s * (1.0 - f)))
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    return np.stack([r, g, b])


def hue(x, shift):
    if x.shape[0] == 1 or shift == 0:
        return x
    h, s, v = rgb_to_hsv(x)
    h = h + shift
    h = h - np.floor(h)
    return hsv_to_rgb(h, s, v).astype(x.dtype)


def rotation_coefficients(angle, H, W, dtype=np.float64):
    """(a, b, c, d, e, f) of the inverse map sx = a X + b Y + c, sy = d X + e Y + f that torchvision hands to PIL for
    RandomAffine(degrees) with translate 0, scale 1, shear 0 (X, Y = output pixel centres)"""
    T = np.dtype(dtype).type
    r = T(-angle) * T(math.pi / 180.0)
    cs, sn = np.cos(r), np.sin(r)
    cx, cy = T(0.5) * T(W), T(0.5) * T(H)
    return cs, sn, cx - cx * cs - cy * sn, -sn, cs, cy + cx * sn - cy * cs


def rotation_source(angle, H, W, dtype=np.float64):
    """float source coordinates (sx, sy), each (H, W), of every output pixel"""
    a, b, c, d, e, f = rotation_coefficients(angle, H, W, dtype)
    X = (np.arange(W, dtype=dtype) + 0.5)[None, :]
    Y = (np.arange(H, dtype=dtype) + 0.5)[:, None]
    return a * X + b * Y + c, d * X + e * Y + f


def rotate(x, angle):
    """nearest neighbour, zero fill; returns (image, ties): ties (H, W) marks the pixels whose float64 source coordinate lies within TIE
    of an integer in x or y"""
    C, H, W = x.shape
    if angle == 0:
        return x, np.zeros((H, W), bool)
    sx, sy = rotation_source(angle, H, W, x.dtype)
    ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    out = np.where(inside[None], x[:, np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)], 0.0).astype(x.dtype)
    sx64, sy64 = rotation_source(angle, H, W, np.float64)
    ties = (np.abs(sx64 - np.rint(sx64)) < TIE) | (np.abs(sy64 - np.rint(sy64)) < TIE)
    return out, ties


def blur(x, sigma):
    """separable 3 taps exp(-d^2 / (2 sigma^2)) normalised to sum 1, reflect padding (edge pixel not repeated)"""
    T = x.dtype.type
    e = np.exp(T(-1.0) / (T(2.0) * T(sigma) * T(sigma)))
    norm = T(1.0) + T(2.0) * e
    w0, w1 = T(1.0) / norm, e / norm
    p = np.pad(x, ((0, 0), (0, 0), (1, 1)), mode="reflect")
    x = w1 * p[:, :, :-2] + w0 * p[:, :, 1:-1] + w1 * p[:, :, 2:]
    p = np.pad(x, ((0, 0), (1, 1), (0, 0)), mode="reflect")
    return w1 * p[:, :-2] + w0 * p[:, 1:-1] + w1 * p[:, 2:]


def dilate3(mask):
    """every pixel whose 3 x 3 neighbourhood (reflect padded, as the blur reads it) holds a marked pixel"""
    p = np.pad(mask, 1, mode="reflect")
    H, W = mask.shape
    out = np.zeros_like(mask)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + H, dx:dx + W]
    return out


JITTER = (lambda x, p: brightness(x, p[BRIGHT]), lambda x, p: contrast(x, p[CONTRAST]), lambda x, p: saturation(x, p[SAT]),
          lambda x, p: hue(x, p[HUE]))


def apply_one(img_hwc_u8, p, mean, inv_std, dtype=np.float64):
    """one image through the chain; p = its row of the parameter table.  Returns (out (C, H, W), left_out (H, W) bool)."""
    T = np.dtype(dtype).type
    p = np.asarray(p, np.float32).astype(dtype)
    x = np.ascontiguousarray(np.transpose(img_hwc_u8, (2, 0, 1))).astype(dtype) / T(255.0)
    C, H, W = x.shape
    if p[FLIP] != 0:
        x = x[:, :, ::-1]
    for op in order_of(p[ORDER]):
        x = JITTER[op](x, p)
    if p[GRAY] != 0 and C == 3:
        x = np.repeat(grey(x)[None], 3, axis=0)
    x, left_out = rotate(x, p[ANGLE])
    if p[BLUR] != 0:
        x = blur(x, p[SIGMA])
        left_out = dilate3(left_out)
    x = (x - np.asarray(mean, np.float32).astype(dtype)[:, None, None]) * np.asarray(inv_std, np.float32).astype(dtype)[:, None, None]
    i, j, h, w = (int(p[k]) for k in (ERASE_I, ERASE_J, ERASE_H, ERASE_W))
    if h > 0 and w > 0:
        x = x.copy()
        x[:, i:i + h, j:j + w] = 0.0
    assert x.dtype == np.dtype(dtype), x.dtype
    return x, left_out


def apply(images_u8_nhwc, index, params, mean, inv_std, dtype=np.float64):
    """the batch: out (B, C, H, W) in `dtype`, left_out (B, H, W) bool (rotation ties, and their 3 x 3 neighbourhood under a blur)"""
    params = np.asarray(params)
    rows = np.arange(params.shape[0]) if index is None else np.asarray(index)
    outs, masks = zip(*(apply_one(images_u8_nhwc[r], params[b], mean, inv_std, dtype) for b, r in enumerate(rows)))
    return np.stack(outs), np.stack(masks)
