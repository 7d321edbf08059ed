"""Generate tests/golden/hadamard_mixer.npz by EXECUTING the reference's own Walsh-Hadamard functions.

Run in the build container only (the reference is imported from SPV_REFERENCE, never copied, and never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hadamard.py

For each shape (B, N, D): a seeded float64 x and
    y = fwht(fwht(F.pad(x, (0, Dp - D, 0, Np - N)), dim=-1), dim=-2)[..., :N, :D]        (Np / Dp = next_pow2; normalize=True)
with the reference's fwht and next_pow2 (spectre_vit/models/spectre/hadamar.py:8-32) and LearnableHadamard's pad / crop convention
(:130-139).  Only arrays are written."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("SPV_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from spectre_vit.models.spectre.hadamar import fwht, next_pow2  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((2, 5, 8), (1, 65, 24), (1, 3, 512))


def main():
    d = {}
    for i, (B, N, D) in enumerate(SHAPES):
        x = torch.randn(B, N, D, generator=torch.Generator().manual_seed(900 + i), dtype=torch.float64)
        Np, Dp = next_pow2(N), next_pow2(D)
        p = F.pad(x, (0, Dp - D, 0, Np - N))
        d[f"y_{B}_{N}_{D}"] = fwht(fwht(p, dim=-1), dim=-2)[..., :N, :D].contiguous().numpy()
        d[f"x_{B}_{N}_{D}"] = x.numpy()
    np.savez_compressed(os.path.join(OUT, "hadamard_mixer.npz"), **d)
    print({k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
