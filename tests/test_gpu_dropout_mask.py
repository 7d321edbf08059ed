"""Pins tests/dropout_ref.py's restatement of the counter-hash mask to the device: spv_dropout on ones must give keep * 1 / (1 - p)
bit for bit (the mask is integer arithmetic; no tolerance).  Eager mode, no GraphedTrainStep open, so live_seed(seed) == seed."""
import numpy as np
import pytest
import torch

import dropout_ref as D
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 5                    # flat index i -> row i >> 12, column i & 4095: three whole rows, a ragged one, a scalar tail
SEED = 0xC0FF_EE11_0000_0007        # high word non-zero


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_device_mask_equals_restatement(dtype, p):
    from spectre_vit import _native, hip_ops
    x = torch.ones(N, dtype=dtype, device=dev())
    y = torch.full((N + 64,), float("nan"), dtype=dtype, device=dev())
    _native.call("spv_dropout", x.data_ptr(), y.data_ptr(), N, p, SEED, hip_ops._dt(x), hip_ops._stream())
    torch.cuda.synchronize()
    assert torch.isnan(y[N:]).all(), "wrote past n"
    keep = D.keep(SEED, 4, 4096, p).reshape(-1)[:N]
    assert 0 < keep.sum() < N
    scale = torch.tensor(np.array([D.inv_keep(p)]), dtype=torch.float32).to(dtype)   # bf16: the constant rounded to bf16
    want = torch.from_numpy(keep).to(dtype) * scale
    got = y[:N].cpu()
    wrong = (got != want).nonzero().reshape(-1)   # NaN != anything: an unwritten element counts
    assert wrong.numel() == 0, (dtype, p, wrong.numel(), wrong[:8].tolist(), got[wrong[:8]].tolist(), want[wrong[:8]].tolist())
    # the other seed word matters on the device too
    y2 = torch.empty(N, dtype=dtype, device=dev())
    _native.call("spv_dropout", x.data_ptr(), y2.data_ptr(), N, p, SEED & 0xFFFF_FFFF, hip_ops._dt(x), hip_ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(y2.cpu() != 0, torch.from_numpy(D.keep(SEED & 0xFFFF_FFFF, 4, 4096, p).reshape(-1)[:N]))
    assert not torch.equal(y2.cpu(), got)
