"""Leaf helpers of every host-side launch: dtype codes, raw pointers, the raw handle of torch's current stream, the device check."""
from __future__ import annotations

import torch

F32, BF16 = 0, 1
_DT = {torch.float32: F32, torch.bfloat16: BF16}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """raw HIP handle of torch's current stream on the current device (the C getter: torch.cuda.current_stream() builds a Python
    Stream object per call -- 10 us, 38 times per training step)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"libspv_hip kernels take float32 or bfloat16 tensors, got {t.dtype}") from None


def _require_gpu(*tensors):
    """every tensor on a HIP device, and on the CURRENT one: kernels are launched on torch.cuda.current_stream(), which belongs
    to the current device -- raw pointers of another GPU on that stream would fault or run unordered."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("Spectre-ViT HIP kernels need tensors on an AMD GPU (cuda/HIP device); "
                               "there is no CPU fallback in this package")
        if t.device.index != torch.cuda.current_device():
            raise RuntimeError(f"tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}: call "
                               "torch.cuda.set_device(local_rank) (or use `with torch.cuda.device(...)`) before the model runs")
