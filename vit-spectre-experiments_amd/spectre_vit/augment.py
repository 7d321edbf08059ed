"""On-GPU training augmentation: the transform chain of reference spectre_vit/repl/train.py:100-115

    RandomHorizontalFlip(0.5) -> ColorJitter(0.4, 0.4, 0.4, 0.1) -> RandomGrayscale(0.2) -> RandomAffine(30)
    -> RandomApply([GaussianBlur(3)]) -> ToTensor -> Normalize(mean, std) -> RandomErasing(0.5)

as HIP kernels: ``spv_augment_params`` draws a per-sample parameter table on the device and an apply kernel runs it, reading the
resident uint8 NHWC set through the batch's index and writing the normalised fp32 NCHW batch the models take.  Two apply paths with one
definition: ``spv_augment_u8`` (csrc/spv_augment.hip), one workgroup per image staged whole in LDS -- CIFAR and MNIST sizes -- and
``spv_augment_tiled_u8`` (csrc/spv_augment_tiled.hip), a contrast-mean pre-pass plus one workgroup per 16 x 64 output tile, for
everything larger up to 512 x 512 (the 224 view the reference distils at).  The ops are torchvision's definitions on float tensors (no
rounding to 8 bits between them, which the reference's PIL pipeline does); the random stream is the library's counter hash keyed by (seed, step, sample, draw),
not torch's generator.  include/spv.h has the table layout, DESIGN.md section 4c the formulas.
"""
from __future__ import annotations

import ctypes

import torch

from spectre_vit import _native
from spectre_vit.hip_ops import _p, _require_gpu, _stream

NPARAM = 16   # SPV_AUG_NPARAM
# columns of the parameter table (SPV_AUG_* of include/spv.h)
FLIP, BRIGHT, CONTRAST, SAT, HUE, ORDER, GRAY, ANGLE, BLUR, SIGMA, ERASE_I, ERASE_J, ERASE_H, ERASE_W = range(14)


def identity_params(batch, device=None):
    """the table that leaves every image as ToTensor + Normalize makes it"""
    p = torch.zeros((batch, NPARAM), dtype=torch.float32, device=device)
    p[:, [BRIGHT, CONTRAST, SAT, SIGMA]] = 1.0
    return p


class TrainAugment:
    """The reference's training transform (train.py:100-115) with its numbers as defaults.  ``jitter`` = ColorJitter's (brightness,
    contrast, saturation, hue): factors U[max(0, 1 - v), 1 + v], hue shift U[-v, v].  A probability of 0 or a jitter / degrees of 0
    switches that op off.

        aug = TrainAugment(CIFAR_MEAN, CIFAR_STD, seed=42)
        img = aug(train_u8_nhwc, index, step=global_step)        # float32 (B, C, H, W), normalised

    ``draw(batch, step)`` returns the (batch, 16) parameter table; ``aug(images, index, params=table)`` applies a given table: the
    apply kernel is a pure function of (images, index, params).

    ``kernel``: "auto" (the default) takes the whole-image LDS kernel where ``spv_augment_supported`` says it fits and the tiled one
    otherwise; "lds" and "tiled" force one (a forced kernel that cannot take the image raises in the call)."""

    KERNELS = ("auto", "lds", "tiled")

    def __init__(self, mean, std, *, flip=0.5, jitter=(0.4, 0.4, 0.4, 0.1), grayscale=0.2, degrees=30, blur=0.5, blur_sigma=(0.1, 2.0),
                 erase=0.5, erase_scale=(0.02, 0.33), erase_ratio=(0.3, 3.3), seed=0, kernel="auto"):
        if kernel not in self.KERNELS:
            raise ValueError(f"kernel is one of {self.KERNELS}, got {kernel!r}")
        self.kernel = kernel
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        if len(self.mean) != len(self.std) or len(self.mean) not in (1, 3):
            raise ValueError(f"mean / std name {len(self.mean)} / {len(self.std)} channels; the augment kernel takes 1 or 3")
        self.flip, self.jitter, self.grayscale, self.degrees = float(flip), tuple(float(v) for v in jitter), float(grayscale), float(degrees)
        self.blur, self.blur_sigma = float(blur), tuple(float(v) for v in blur_sigma)
        self.erase, self.erase_scale, self.erase_ratio = float(erase), tuple(float(v) for v in erase_scale), tuple(float(v) for v in erase_ratio)
        if len(self.jitter) != 4 or min(self.jitter) < 0 or self.jitter[3] > 0.5:
            raise ValueError(f"jitter = (brightness, contrast, saturation, hue) >= 0 with hue <= 0.5, got {jitter}")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._norm = {}   # device -> (mean, 1 / std) fp32 tensors

    def cfg(self):
        """the spv_augment_cfg of this transform"""
        b, c, s, h = self.jitter
        return _native.AugmentCfg(flip_p=self.flip, bright_lo=max(0.0, 1 - b), bright_hi=1 + b, contrast_lo=max(0.0, 1 - c),
                                  contrast_hi=1 + c, sat_lo=max(0.0, 1 - s), sat_hi=1 + s, hue_lo=-h, hue_hi=h, gray_p=self.grayscale,
                                  degrees=self.degrees, blur_p=self.blur, sigma_lo=self.blur_sigma[0], sigma_hi=self.blur_sigma[1],
                                  erase_p=self.erase, scale_lo=self.erase_scale[0], scale_hi=self.erase_scale[1],
                                  ratio_lo=self.erase_ratio[0], ratio_hi=self.erase_ratio[1])

    def norm(self, device):
        """(mean, 1 / std) on `device`, the inverse taken in float64 and rounded once"""
        key = str(device)
        if key not in self._norm:
            self._norm[key] = (torch.tensor(self.mean, dtype=torch.float32, device=device),
                               (1.0 / torch.tensor(self.std, dtype=torch.float64)).float().to(device))
        return self._norm[key]

    def draw(self, batch, step, *, height=32, width=32, device=None):
        """the parameter table of `batch` samples at `step`, drawn on the device: same (seed, step) -> the same table.  The image
        size only enters RandomErasing's rectangle search."""
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        params = torch.empty((int(batch), NPARAM), dtype=torch.float32, device=device)
        _require_gpu(params)
        cfg = self.cfg()
        _native.call("spv_augment_params", _p(params), int(batch), len(self.mean), int(height), int(width), ctypes.addressof(cfg),
                     self.seed, int(step) & 0xFFFFFFFFFFFFFFFF, _stream())
        return params

    def __call__(self, images_u8_nhwc, index=None, *, step=None, params=None):
        """images_u8_nhwc: the resident uint8 set (N, H, W, C); index: int64 (B,) rows of it (None: the first B = len(params) rows, or
        all of them); exactly one of `step` (draw the table) and `params` (use this one).  Returns float32 (B, C, H, W)."""
        if (step is None) == (params is None):
            raise ValueError("give exactly one of step= (draw the parameter table) and params= (apply this table)")
        x = images_u8_nhwc
        if x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
            raise TypeError(f"the augment kernel takes a contiguous uint8 (N, H, W, C) set, got {x.dtype} {tuple(x.shape)}")
        n, H, W, C = x.shape
        if C != len(self.mean):
            raise ValueError(f"{C}-channel images, but mean / std name {len(self.mean)} channels")
        if index is not None:
            if index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
                raise TypeError(f"index is a contiguous int64 vector, got {index.dtype} {tuple(index.shape)}")
            batch = index.numel()
        else:
            batch = params.shape[0] if params is not None else n
        _require_gpu(x, index, params)
        plan = _native.call("spv_augment_plan", C, H, W)
        if plan == 0 or (self.kernel == "lds" and plan != 1):
            raise ValueError(f"a {C} x {H} x {W} image does not fit the augment kernel's LDS staging (two fp32 copies within 64 KiB)"
                             + (" and kernel='lds' rules the tiled one out" if plan else " nor the tiled kernel (sides 2 .. 512)"))
        tiled = self.kernel == "tiled" or plan == 2
        if params is None:
            params = self.draw(batch, step, height=H, width=W, device=x.device)
        elif params.dtype != torch.float32 or tuple(params.shape) != (batch, NPARAM) or not params.is_contiguous():
            raise TypeError(f"params is a contiguous float32 ({batch}, {NPARAM}) table, got {params.dtype} {tuple(params.shape)}")
        mean, inv_std = self.norm(x.device)
        out = torch.empty((batch, C, H, W), dtype=torch.float32, device=x.device)
        if tiled:
            ws = torch.empty(_native.call("spv_augment_tiled_ws_bytes", batch, H, W), dtype=torch.uint8, device=x.device)
            _native.call("spv_augment_tiled_u8", _p(x), _p(index), _p(params), _p(mean), _p(inv_std), _p(out), batch, n, C, H, W, _p(ws),
                         ws.numel(), _stream())
        else:
            _native.call("spv_augment_u8", _p(x), _p(index), _p(params), _p(mean), _p(inv_std), _p(out), batch, n, C, H, W, _stream())
        return out
