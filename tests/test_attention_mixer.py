"""CPU-side checks of the self-attention token mixer (SpectreViT(mixer="attention"), SelfAttentionMixer): the model surface, the
nn.MultiheadAttention parameter ABI and same-seed init, the float64 definition the GPU tests compare against, and the host-side
argument checks of the two single-query-row attention entry points (nothing is launched)."""
import copy

import numpy as np
import pytest
import torch

from oracle import spectre_oracle as O

TINY = dict(img_size=32, patch_size=4, in_channels=3, num_classes=10, embed_dim=48, num_encoders=3, num_heads=8, hidden_dim=96,
            dropout=0.1, activation="gelu")
MIX_KEYS = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")


def _model(**kw):
    from spectre_vit.models.spectre.spectre import SpectreViT
    return SpectreViT(**dict(TINY, **kw), mixer="attention")


def test_model_builds_with_mha_keys_per_layer():
    m = _model()
    sd = m.state_dict()
    E = TINY["embed_dim"]
    shapes = {"in_proj_weight": (3 * E, E), "in_proj_bias": (3 * E,), "out_proj.weight": (E, E), "out_proj.bias": (E,)}
    for i in range(TINY["num_encoders"]):
        pre = f"encoder_blocks.layers.{i}.mix_layer."
        got = sorted(k[len(pre):] for k in sd if k.startswith(pre))
        assert got == sorted(MIX_KEYS), got
        for k, shp in shapes.items():
            assert tuple(sd[pre + k].shape) == shp, (pre + k, sd[pre + k].shape)
            assert sd[pre + k].dtype == torch.float32
    assert not any(k.endswith(("perms", "signs")) for k in sd), [k for k in sd if k.endswith(("perms", "signs"))]


def test_clones_start_identical_and_deepcopy_works():
    m = _model()
    layers = m.encoder_blocks.layers
    for k in MIX_KEYS:
        a = layers[0].mix_layer.state_dict()[k]
        for layer in layers[1:]:
            assert torch.equal(layer.mix_layer.state_dict()[k], a), k
    c = copy.deepcopy(m)
    for (k, v), (k2, v2) in zip(m.state_dict().items(), c.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k
    assert c.encoder_blocks.layers[0].mix_layer.in_proj_weight.data_ptr() != layers[0].mix_layer.in_proj_weight.data_ptr()
    c.eval()
    assert not c.encoder_blocks.layers[0].mix_layer.training and m.encoder_blocks.layers[0].mix_layer.training
    c.to(torch.float64)
    assert c.encoder_blocks.layers[0].mix_layer.in_proj_weight.dtype == torch.float64


def test_mixer_dropout_follows_the_layer():
    from spectre_vit.modules.mixers import SelfAttentionMixer
    m = _model(dropout=0.25)
    mix = m.encoder_blocks.layers[0].mix_layer
    assert isinstance(mix, SelfAttentionMixer) and mix.dropout == 0.25 and mix.num_heads == 8 and mix.head_dim == 6


@pytest.mark.parametrize("d_model,nhead", [(48, 5), (64, 0), (10, 4)])
def test_bad_nhead_raises_naming_both(d_model, nhead):
    from spectre_vit.modules.mixers import SelfAttentionMixer
    with pytest.raises(ValueError) as e:
        SelfAttentionMixer(d_model, nhead)
    assert f"nhead={nhead}" in str(e.value) and f"d_model={d_model}" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        _model(embed_dim=d_model, num_heads=nhead)


def test_unknown_mixer_still_refused():
    from spectre_vit.models.spectre.spectre import MIXERS, SpectreViT
    assert "attention" in MIXERS
    with pytest.raises(ValueError):
        SpectreViT(**TINY, mixer="fft_mh")


@pytest.mark.parametrize("E,H", [(48, 8), (512, 16), (768, 12)])
def test_same_seed_init_equals_multihead_attention(E, H):
    from spectre_vit.modules.mixers import SelfAttentionMixer
    torch.manual_seed(7)
    a = SelfAttentionMixer(E, H, 0.1)
    torch.manual_seed(7)
    b = torch.nn.MultiheadAttention(E, H, dropout=0.1, bias=True, batch_first=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.count_nonzero(sa["in_proj_bias"]) == 0 and torch.count_nonzero(sa["out_proj.bias"]) == 0


def test_state_dict_loads_strict_both_ways():
    from spectre_vit.modules.mixers import SelfAttentionMixer
    torch.manual_seed(1)
    a = SelfAttentionMixer(64, 4)
    torch.manual_seed(2)
    b = torch.nn.MultiheadAttention(64, 4, batch_first=True)
    b.load_state_dict(a.state_dict(), strict=True)
    for k, v in a.state_dict().items():
        assert torch.equal(b.state_dict()[k], v), k
    torch.manual_seed(3)
    c = torch.nn.MultiheadAttention(64, 4, batch_first=True)
    a.load_state_dict(c.state_dict(), strict=True)
    for k, v in c.state_dict().items():
        assert torch.equal(a.state_dict()[k], v), k
    # and a whole layer's mixer out of a model state_dict
    m = _model(embed_dim=64, num_heads=4)
    pre = "encoder_blocks.layers.1.mix_layer."
    sub = {k[len(pre):]: v for k, v in m.state_dict().items() if k.startswith(pre)}
    c.load_state_dict(sub, strict=True)


def test_torch_mha_float64_equals_oracle_mhsa_batch_first():
    """the definition the GPU tests use: torch's own MHA in float64 on CPU == the oracle's mhsa_fwd(batch_first=True), with the
    parameters of a SelfAttentionMixer (non-zero biases so that every term counts), and its backward == mhsa_bwd."""
    from spectre_vit.modules.mixers import SelfAttentionMixer
    torch.manual_seed(4)
    E, H, B, N = 48, 8, 3, 17
    mix = SelfAttentionMixer(E, H)
    with torch.no_grad():
        mix.in_proj_bias.normal_(0, 0.1)
        mix.out_proj.bias.normal_(0, 0.1)
    mha = torch.nn.MultiheadAttention(E, H, batch_first=True).double()
    mha.load_state_dict({k: v.double() for k, v in mix.state_dict().items()}, strict=True)
    x = torch.randn(B, N, E, dtype=torch.float64, requires_grad=True)
    y = mha(x, x, x, need_weights=False)[0]
    dy = torch.randn(B, N, E, dtype=torch.float64)
    y.backward(dy)
    p = {"in_proj_weight": mha.in_proj_weight.detach().numpy(), "in_proj_bias": mha.in_proj_bias.detach().numpy(),
         "out_proj_weight": mha.out_proj.weight.detach().numpy(), "out_proj_bias": mha.out_proj.bias.detach().numpy()}
    ref, cache = O.mhsa_fwd(x.detach().numpy(), p, H, batch_first=True)
    assert np.abs(y.detach().numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
    dx, g = O.mhsa_bwd(dy.numpy(), p, H, cache, batch_first=True)
    assert np.abs(x.grad.numpy() - dx).max() <= 1e-12 * np.abs(dx).max()
    assert np.abs(mha.in_proj_weight.grad.numpy() - g["in_proj_weight"]).max() <= 1e-12 * np.abs(g["in_proj_weight"]).max()
    assert np.abs(mha.out_proj.weight.grad.numpy() - g["out_proj_weight"]).max() <= 1e-12 * np.abs(g["out_proj_weight"]).max()


def test_cpu_tensors_fail_loudly():
    m = _model()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.randn(2, 3, 32, 32))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_row0_entry_points_reject_bad_arguments_before_any_launch(built):
    """the error contract of include/spv.h for spv_attention_row0_fwd / _bwd: every call below fails the host-side checks, returns
    non-zero and leaves a message naming the function and the reason (no GPU needed: nothing is launched)"""
    from spectre_vit import _native
    BF16, F32 = 1, 0
    P = 4096   # a 16-byte aligned stand-in address (never dereferenced: the checks fail first)
    fwd = lambda q0=P, k=P, v=P, ld=1024, ctx0=P, probs=P, b=4, n=65, h=16, hd=32, dt=BF16, p=0.0: (  # noqa: E731
        q0, k, v, ld, ctx0, probs, b, n, h, hd, dt, p, 0, 0)
    bwd = lambda dc=P, q0=P, k=P, v=P, ld=1024, probs=P, dq=P, dk=P, dv=P, ldd=1024, b=4, n=65, h=16, hd=32, dt=BF16, p=0.0: (  # noqa: E731
        dc, q0, k, v, ld, probs, dq, dk, dv, ldd, b, n, h, hd, dt, p, 0, 0)
    cases = [
        ("spv_attention_row0_fwd", fwd(b=0), "empty"),
        ("spv_attention_row0_fwd", fwd(n=0), "empty"),
        ("spv_attention_row0_fwd", fwd(dt=7), "dtype"),
        ("spv_attention_row0_fwd", fwd(h=2, hd=3), "multiple of 8"),
        ("spv_attention_row0_fwd", fwd(h=1, hd=6, dt=F32), "multiple of 4"),
        ("spv_attention_row0_fwd", fwd(h=64, hd=64, ld=8192), "heads * head_dim"),
        ("spv_attention_row0_fwd", fwd(ld=256), "ldkv"),
        ("spv_attention_row0_fwd", fwd(ld=1028), "ldkv"),
        ("spv_attention_row0_fwd", fwd(n=1024), "heads * len"),
        ("spv_attention_row0_fwd", fwd(p=1.0), "p_drop"),
        ("spv_attention_row0_fwd", fwd(p=-0.1), "p_drop"),
        ("spv_attention_row0_fwd", fwd(k=P + 2), "16-byte aligned"),
        ("spv_attention_row0_fwd", fwd(v=0), "16-byte aligned"),
        ("spv_attention_row0_fwd", fwd(q0=0), "non-NULL"),
        ("spv_attention_row0_bwd", bwd(h=0), "empty"),
        ("spv_attention_row0_bwd", bwd(dt=2), "dtype"),
        ("spv_attention_row0_bwd", bwd(ldd=504), "ldd"),
        ("spv_attention_row0_bwd", bwd(ld=100), "ldkv"),
        ("spv_attention_row0_bwd", bwd(dk=P + 8), "16-byte aligned"),
        ("spv_attention_row0_bwd", bwd(probs=0), "non-NULL"),
        ("spv_attention_row0_bwd", bwd(p=1.5), "p_drop"),
        ("spv_attention_row0_bwd", bwd(h=128, hd=8, n=65), "heads * len"),
    ]
    for name, args, needle in cases:
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value), (name, str(e.value))
        assert needle in str(e.value), (name, needle, str(e.value))


def test_census_indices_match_header(built):
    import os
    import re
    from conftest import ROOT
    from spectre_vit import _native
    src = open(os.path.join(ROOT, "include", "spv.h")).read()
    assert int(re.search(r"SPV_PATH_ATTN_ROW0_FWD = (\d+)", src).group(1)) == _native.PATH["attn_row0_fwd"] == 20
    assert int(re.search(r"SPV_PATH_ATTN_ROW0_BWD = (\d+)", src).group(1)) == _native.PATH["attn_row0_bwd"] == 21
    assert int(re.search(r"SPV_PATH_COUNT = (\d+)", src).group(1)) == 27
    assert sorted(_native.PATH.values()) == list(range(27))
