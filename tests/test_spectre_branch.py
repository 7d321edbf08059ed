"""CPU-side checks of SpectreBranch (reference spectre_vit/models/spectre_branch/spectre_branch.py): the five classes import from the
reference's path, the state_dict ABI and the same-seed initialisation match the reference's (tests/golden/model_spectre_branch.npz,
written by make_golden_branch.py), the reference's limits are refused in the constructors, CPU tensors fail loudly."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

PRESET = dict(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=768, num_encoders=4, num_heads=8, hidden_dim=256,
              dropout=0.0, activation="gelu")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "model_spectre_branch.npz")))


def strided(a, n=32):
    f = a.reshape(-1)
    return f[np.linspace(0, f.size - 1, n).astype(np.int64)]


def test_classes_import_from_reference_path():
    from spectre_vit.models.spectre_branch.spectre_branch import (  # noqa: F401
        SpectreBranch, SpectreBranchEncoder, SpectreBranchEncoderLayer, SpectreFeatExtractor, SpectreMix)


def test_state_dict_keys_and_shapes_match_reference(golden):
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranch
    sd = SpectreBranch(**PRESET).state_dict()
    assert list(sd.keys()) == [str(k) for k in golden["keys"]]   # same names in the same registration order
    for (k, v), shp in zip(sd.items(), golden["shapes"]):
        assert list(v.shape) == [int(s) for s in shp[:v.dim()]] and not shp[v.dim():].any(), k
        assert v.dtype == torch.float32, k


def test_same_seed_init_matches_reference(golden):
    """the reference's RNG order (every `net` conv before every `project` conv, deep-cloned layers) is part of the weight ABI"""
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranch
    torch.manual_seed(int(golden["cfg.seed"]))
    sd = SpectreBranch(**PRESET).state_dict()
    for k, v in sd.items():
        a = v.numpy().astype(np.float64)
        got = np.concatenate([[a.sum(), np.abs(a).sum()], strided(a)])
        ref = golden["init." + k]
        np.testing.assert_array_equal(got[2:], ref[2:], err_msg=k)
        np.testing.assert_allclose(got[:2], ref[:2], rtol=1e-9, atol=1e-9, err_msg=k)


def test_mix_state_dict_matches_reference(golden):
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreMix
    sd = SpectreMix(64, 2, 5).state_dict()
    ref = {k[len("mix.sd."):]: v for k, v in golden.items() if k.startswith("mix.sd.")}
    assert list(sd.keys()) == list(ref.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k].shape, k


@pytest.mark.parametrize("kw,match", [
    (dict(embed_dim=512), "spectre_branch.py:105"),
    (dict(in_channels=1), "spectre_branch.py:102"),
    (dict(num_encoders=9), "empty the 32x17 spectrum"),
    (dict(), "empty"),   # the constructor defaults: 12 encoders on 32 x 32 images
])
def test_constructor_refuses_reference_limits(kw, match):
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranch
    cfg = dict(PRESET, **kw) if kw else {}
    with pytest.raises(ValueError, match=match):
        SpectreBranch(**cfg)


def test_eight_stages_are_the_limit_at_32x32():
    """built on the meta device: eight stages are 1.3 G parameters (the last conv is 6561 -> 19683 channels), nine are 11.8 G"""
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranch, SpectreFeatExtractor
    with torch.device("meta"):
        m = SpectreBranch(**dict(PRESET, num_encoders=8))
        ext = SpectreFeatExtractor(3, 8, 65, num_stages=9)
    assert m.encoder_blocks.spectre_branch.net[-1][0].weight.shape == (3 ** 9, 3 ** 8, 3, 3)
    with pytest.raises(ValueError, match="empty"):
        ext(torch.zeros(1, 3, 32, 32, device="meta"))   # the extractor alone refuses in forward, before touching the image


def test_reduction_is_not_built():
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreFeatExtractor
    with pytest.raises(NotImplementedError, match="161-164"):
        SpectreFeatExtractor(3, 768, 65, reduction=2, num_stages=1)


def test_encoder_refuses_other_widths():
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranchEncoder, SpectreBranchEncoderLayer
    layer = SpectreBranchEncoderLayer(seq_length=5, d_model=64, nhead=2, dim_feedforward=32, dropout=0.0, activation="gelu")
    with pytest.raises(ValueError, match="768"):
        SpectreBranchEncoder(layer, 5, 1)


def test_cpu_tensors_fail_loudly():
    from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranch, SpectreMix
    m = SpectreBranch(**dict(PRESET, num_encoders=1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.randn(2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SpectreMix(64, 2, 5)(torch.randn(2, 5, 64))


def test_harness_builds_the_branch_model():
    from spectre_vit import harness
    from spectre_vit.configs.parser import parse_config
    c = parse_config("spectre_vit/configs/spectre_branch.py")
    m = harness.build_model(c, model="spectre_branch", device="cpu")
    assert type(m).__name__ == "SpectreBranch" and len(m.encoder_blocks.layers) == c.num_encoders
