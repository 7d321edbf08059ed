"""Restatement of the distillation teacher's view (csrc/spv_distill.hip, spectre_vit.distillation.TeacherView) in numpy:

    Resize(resize, BICUBIC) -> CenterCrop(crop) -> ToTensor -> Normalize        (reference spectre_vit/repl/train.py:92-100)

on 8-bit images, where torchvision's Resize of a PIL image is Image.resize(..., BICUBIC): Pillow's integer resampling.  Written from
Pillow's documented behaviour -- per axis a window of support 2 around the output's centre, bicubic weights (a = -0.5) normalised in
float64, rounded half away from zero to 22 fractional bits; each pass an integer sum plus 2^21, shifted right by 22 and clamped to
0..255; the horizontal pass first, stored as uint8, the vertical pass over it.  tests/test_distill_views.py holds it to Pillow itself
on every pixel; the GPU tests hold the kernel to it, exactly."""
import numpy as np
import torch

PRECISION_BITS = 22


def bicubic(t, a=-0.5):
    t = np.abs(np.asarray(t, np.float64))
    inner = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    outer = (((t - 5) * t + 8) * t - 4) * a
    return np.where(t < 1.0, inner, np.where(t < 2.0, outer, 0.0))


def table(n, resize=256, crop=224):
    """(xmin int64 [crop], taps int64 [crop, 4], count int64 [crop]): the window start, the integer taps (zero past `count`) and the
    number of taps inside the image for every cropped output coordinate of an n-pixel axis"""
    lo = (resize - crop) // 2
    xx = np.arange(lo, lo + crop, dtype=np.float64)
    scale = n / resize
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - 2.0 + 0.5).astype(np.int64), 0)       # C's (int): truncation towards zero
    xmax = np.minimum((center + 2.0 + 0.5).astype(np.int64), n)
    count = xmax - xmin
    assert count.max() <= 4
    w = np.zeros((crop, 4), np.float64)
    for d in range(4):
        w[:, d] = np.where(d < count, bicubic(d + xmin - center + 0.5), 0.0)
    ww = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]                      # summed in tap order, as a loop does
    w = w / ww[:, None]
    taps = np.where(w < 0, w * (1 << PRECISION_BITS) - 0.5, w * (1 << PRECISION_BITS) + 0.5).astype(np.int64)
    return xmin, taps, count


def _pass(x, xmin, taps, axis):
    """one resampling pass of uint8 `x` along `axis`: clip8((2^21 + sum_d x[xmin + d] taps[d]) >> 22)"""
    x = np.moveaxis(x, axis, -1).astype(np.int64)
    n = x.shape[-1]
    acc = np.full(x.shape[:-1] + (xmin.size,), 1 << (PRECISION_BITS - 1), np.int64)
    for d in range(4):
        acc += x[..., np.minimum(xmin + d, n - 1)] * taps[:, d]        # (a tap past the image has coefficient 0)
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, -1, axis), acc


def teacher_view_u8(img, resize=256, crop=224, return_range=False):
    """img uint8 (..., n, n, C) -> uint8 (..., crop, crop, C): Image.resize((resize, resize), BICUBIC) cropped to the centre"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-3] == img.shape[-2] and img.shape[-2] <= resize
    xmin, taps, _ = table(img.shape[-2], resize, crop)
    h, acc_h = _pass(img, xmin, taps, -2)      # horizontal: along W
    v, acc_v = _pass(h, xmin, taps, -3)        # vertical: along H
    if return_range:
        return v, (int(min(acc_h.min(), acc_v.min())), int(max(acc_h.max(), acc_v.max())))
    return v


def normalise(u8_nhwc, mean, std):
    """torch-CPU fp32 ToTensor + Normalize of a uint8 (B, H, W, C) batch -> float32 (B, C, H, W)"""
    x = torch.from_numpy(np.ascontiguousarray(u8_nhwc)).permute(0, 3, 1, 2).float() / 255
    m = torch.tensor(mean, dtype=torch.float32).view(1, -1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(1, -1, 1, 1)
    return ((x - m) / s).contiguous()


def teacher_view(u8_nhwc, index, mean, std, resize=256, crop=224):
    """the whole view of a batch: float32 (B, C, crop, crop) on the CPU"""
    sel = u8_nhwc if index is None else u8_nhwc[np.asarray(index)]
    return normalise(teacher_view_u8(sel, resize, crop), mean, std)
