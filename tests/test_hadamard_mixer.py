"""CPU side of the Walsh-Hadamard token mixer (SpectreViT(mixer="hadamard")): tests/hadamard_ref.py's float64 reference against the
reference project's own functions (tests/golden/hadamard_mixer.npz) and against its algebra (symmetry, the token-sum form of row 0);
the host restatement of csrc/spv_hadamard_core.h against the library's host-side answers over tables that reach every branch and every
refusal; and the float32 floor of the references on exactly the inputs tests/test_gpu_hadamard_mixer.py uses."""
import os
import re

import numpy as np
import pytest

import hadamard_ref as H
import spectral_ref as R
from oracle import spectre_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hadamard_mixer.npz")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


# ------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("shape", [(2, 5, 8), (1, 65, 24), (1, 3, 512)])
def test_reference_equals_the_golden_fixture(shape):
    g = np.load(GOLDEN)
    tag = "_".join(map(str, shape))
    x, y = g["x_" + tag], g["y_" + tag]
    assert x.dtype == y.dtype == np.float64 and x.shape == y.shape == shape
    assert np.abs(H.mix(x) - y).max() <= 1e-12 * np.abs(y).max()
    # normalize=False is the same operator without s
    assert np.abs(H.mix(x, normalize=False) * H.scale(shape[1], shape[2]) - y).max() <= 1e-12 * np.abs(y).max()


def test_reference_is_the_explicit_matrix_product():
    """H_n[i][j] = (-1)^popcount(i & j), padded and cropped"""
    rng = np.random.default_rng(5)
    for N, Dm in ((5, 24), (1, 1), (65, 8), (3, 5)):
        x = rng.standard_normal((2, N, Dm))
        Np, Dp = H.next_pow2(N), H.next_pow2(Dm)
        hn = np.array([[(-1.0) ** bin(i & j).count("1") for j in range(N)] for i in range(N)])
        hd = np.array([[(-1.0) ** bin(i & j).count("1") for j in range(Dm)] for i in range(Dm)])
        want = np.einsum("mk,bkd,de->bme", hn, x, hd) * (Np * Dp) ** -0.5
        assert np.abs(H.mix(x) - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("shape", [(2, 5, 24), (1, 65, 512), (3, 1, 8), (1, 197, 768)])
@pytest.mark.parametrize("normalize", [True, False])
def test_operator_is_symmetric_and_row0_is_the_token_sum(shape, normalize):
    rng = np.random.default_rng(sum(shape))
    a, b = rng.standard_normal(shape), rng.standard_normal(shape)
    lhs, rhs = (H.mix(a, normalize) * b).sum(), (a * H.mix(b, normalize)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)
    y = H.mix(a, normalize)
    assert np.abs(y[:, 0] - H.row0(a, normalize)).max() <= 1e-12 * np.abs(y[:, 0]).max()


def test_fused_and_row0_references_agree_with_each_other_and_with_the_oracle_layer():
    rng = np.random.default_rng(11)
    x, dout = rng.standard_normal((2, 5, 512)), rng.standard_normal((2, 5, 512))
    gamma, beta = H.affine(rng, 512)
    f = H.ln_fwd(x, gamma, beta)
    n1, cache = O.layernorm_fwd(H.mix(x), gamma, beta)
    assert np.abs(f["out"] - (n1 + x)).max() <= 1e-12
    dm, dg, db = O.layernorm_bwd(dout, gamma, cache)
    b = H.ln_bwd(dout, f["prenorm"], gamma)
    assert np.abs(b["dx"] - (H.mix(dm) + dout)).max() <= 1e-12 and np.abs(b["dgamma"] - dg).max() <= 1e-12 and np.abs(b["dbeta"] - db).max() <= 1e-12
    assert np.abs(b["partials"].sum(0) - np.stack([dg, db])).max() <= 1e-12
    c = H.cls_fwd(x, gamma, beta)
    assert np.abs(c["out"] - f["out"][:, 0]).max() <= 1e-12 and np.abs(c["m0"] - f["prenorm"][:, 0]).max() <= 1e-12
    # a gradient that arrives at row 0 only: the full node's backward is the row-0 node's
    g1 = rng.standard_normal((2, 512))
    d0 = np.zeros_like(dout)
    d0[:, 0] = g1
    full, cls = H.ln_bwd(d0, f["prenorm"], gamma), H.cls_bwd(g1, c["m0"], gamma, 5)
    assert np.abs(full["dx"] - cls["dx"]).max() <= 1e-12 and np.abs(full["partials"] - cls["partials"]).max() <= 1e-12


# ------------------------------------------------------------------------------------------ 2. the public surface
def test_hadamard_is_a_mixer_and_unknown_names_still_raise(built):
    import copy

    from spectre_vit.models.spectre.spectre import MIXERS, SpectreViT
    from spectre_vit.modules.mixers import HadamardMixer
    assert "hadamard" in MIXERS and MIXERS[:5] == ("permut", "fft", "dwt_embed", "dwt_token", "attention")
    cfg = dict(img_size=8, patch_size=4, in_channels=3, num_classes=10, embed_dim=16, num_encoders=2, num_heads=2, hidden_dim=24, dropout=0.0)
    m = SpectreViT(**cfg, mixer="hadamard")
    ref = SpectreViT(**cfg, mixer="fft")
    assert list(m.state_dict()) == list(ref.state_dict()), "the mixer has no parameters: the same keys as the FFT model"
    mix = m.encoder_blocks.layers[0].mix_layer
    assert isinstance(mix, HadamardMixer) and mix.normalize is True and not list(mix.parameters()) and not list(mix.buffers())
    assert copy.deepcopy(HadamardMixer(normalize=False)).normalize is False
    with pytest.raises(ValueError):
        SpectreViT(**cfg, mixer="nope")


def test_symbols_are_declared_bound_and_the_census_is_unchanged(built):
    from conftest import ROOT
    from spectre_vit import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "spv.h")).read()
    names = ["spv_hadamard_path", "spv_hadamard_workspace_floats", "spv_hadamard_mix", "spv_hadamard_ln_supported", "spv_hadamard_ln_fwd",
             "spv_hadamard_ln_bwd", "spv_hadamard_cls_supported", "spv_hadamard_cls_fwd", "spv_hadamard_cls_bwd"]
    for name in names:
        assert name in _native.SIGNATURES and getattr(lib, name).argtypes == _native.SIGNATURES[name]
        assert re.search(r"\b(int|int64_t) " + name + r"\(", hdr), name
    enum = dict(re.findall(r"(SPV_PATH_[A-Z0-9_]+)\s*=\s*(\d+)", hdr))
    assert int(enum["SPV_PATH_COUNT"]) == 27 and len(_native.PATH) == 27 and sorted(_native.PATH.values()) == list(range(27))
    assert lib.spv_version() == 1
    codes = dict(re.findall(r"#define (SPV_HADAMARD_[A-Z_]+) \(?(-?\d+)\)?", hdr))
    assert {k: int(v) for k, v in codes.items()} == dict(
        SPV_HADAMARD_ONE_KERNEL=H.ONE_KERNEL, SPV_HADAMARD_GENERIC=H.GENERIC, SPV_HADAMARD_REFUSE_EMPTY=H.REFUSE_EMPTY,
        SPV_HADAMARD_REFUSE_DTYPE=H.REFUSE_DTYPE, SPV_HADAMARD_REFUSE_DIM=H.REFUSE_DIM, SPV_HADAMARD_REFUSE_TOKENS=H.REFUSE_TOKENS,
        SPV_HADAMARD_REFUSE_WORKSPACE=H.REFUSE_WORKSPACE)


# ------------------------------------------------------------------------------------------ 3. dispatch
def test_selector_agrees_with_the_library_over_the_tables(built):
    from spectre_vit import _native as nat
    for c in H.MIX_CASES + H.MISALIGNED_REFUSED:
        for ws in (True, False):
            assert nat.call("spv_hadamard_path", H.CODE[c.dtype], c.tokens, c.dim, int(ws)) == H.path(c.dtype, c.tokens, c.dim, ws), (c, ws)
        assert nat.call("spv_hadamard_workspace_floats", c.batch, c.tokens, c.dim) == H.workspace_floats(c.batch, c.tokens, c.dim), c
        assert H.path(c.dtype, c.tokens, c.dim) in (H.ONE_KERNEL, H.GENERIC), c
    for (dt, t, d, ws), why in H.REFUSALS.items():
        assert nat.call("spv_hadamard_path", H.CODE.get(dt, dt), t, d, int(ws)) == H.path(dt, t, d, ws) == why, (dt, t, d, ws)
    # a sweep that straddles every threshold of the selector
    for t in (1, 2, 39, 40, 41, 80, 81, 128, 129, 160, 161, 512, 513, 32768, 32769):
        for d in (1, 7, 8, 9, 16, 24, 256, 512, 513, 768, 1024, 1032, 16384, 16385):
            for dt in H.DTYPES:
                for ws in (True, False):
                    assert nat.call("spv_hadamard_path", H.CODE[dt], t, d, int(ws)) == H.path(dt, t, d, ws), (dt, t, d, ws)
            assert nat.call("spv_hadamard_workspace_floats", 3, t, d) == H.workspace_floats(3, t, d), (t, d)
    for dt in H.DTYPES + (2,):
        code = H.CODE.get(dt, dt)
        for t in (0, 1, 2, 3, 64, 65, 66):
            for d in (128, 256, 512, 768, 1024, 2048):
                assert nat.call("spv_hadamard_ln_supported", t, d, code) == H.ln_supported(dt, t, d), (dt, t, d)
                assert nat.call("spv_hadamard_cls_supported", t, d, code) == H.cls_supported(dt, t, d), (dt, t, d)
    for c in H.LN_CASES:
        assert H.ln_supported("bf16", c.tokens, 512) == 1 and H.path("bf16", c.tokens, 512) == H.ONE_KERNEL
    for c in H.CLS_CASES:
        assert H.cls_supported(c.dtype, c.tokens, c.dim) == 1


def test_tables_reach_every_branch_and_every_refusal():
    plans = [H.select(c.dtype, c.tokens, c.dim) for c in H.MIX_CASES]
    assert {p.path for p in plans} == {H.ONE_KERNEL, H.GENERIC}
    gen = [p for p in plans if p.path == H.GENERIC]
    assert any(p.rpw > 1 for p in gen) and any(p.rpw == 1 for p in gen), "row pass: several rows and one row per workgroup"
    assert any(p.cs < min(64, p.dp) for p in gen) and any(p.cs == 64 for p in gen) and any(p.cs == p.dp < 64 for p in gen), "slab widths"
    assert any(p.np > c.tokens for p, c in zip(plans, H.MIX_CASES)) and any(p.dp > c.dim for p, c in zip(plans, H.MIX_CASES)), "padding on both axes"
    # why a generic case is generic: every reason appears
    reasons = set()
    for c in H.MIX_CASES:
        if H.path(c.dtype, c.tokens, c.dim) == H.GENERIC:
            reasons.add("pieces" if c.dim % 8 else "tokens" if c.tokens > H.ONE_MAX_TOKENS else "lds")
    assert reasons == {"pieces", "tokens", "lds"}
    # the ends of the windows lie in the tables
    assert H.path("fp32", 128, 8) == H.ONE_KERNEL and H.path("fp32", 129, 8) == H.GENERIC
    assert H.path("bf16", 80, 512) == H.ONE_KERNEL and H.path("bf16", 81, 512) == H.GENERIC
    assert H.path("bf16", 197, 768) == H.GENERIC and H.path("bf16", 65, 768) == H.GENERIC and H.path("bf16", 5, 768) == H.ONE_KERNEL
    assert any(c.off for c in H.MIX_CASES) and all(H.path(c.dtype, c.tokens, c.dim) == H.GENERIC for c in H.MIX_CASES if c.off)
    assert all(H.path(c.dtype, c.tokens, c.dim) == H.ONE_KERNEL and c.off for c in H.MISALIGNED_REFUSED)
    assert set(H.REFUSALS.values()) == {H.REFUSE_EMPTY, H.REFUSE_DTYPE, H.REFUSE_DIM, H.REFUSE_TOKENS, H.REFUSE_WORKSPACE}
    assert {c.tokens for c in H.LN_CASES} == {2, 3, 16, 17, 32, 33, 64, 65} and {c.batch for c in H.LN_CASES} == {1, 3}
    assert H.ln_supported("bf16", 1, 512) == H.ln_supported("bf16", 66, 512) == H.ln_supported("fp32", 5, 512) == H.ln_supported("bf16", 5, 256) == 0


def test_refused_calls_fail_on_the_host_and_are_not_counted(built):
    """NULL tensors: a call that got past the host checks would fault"""
    from spectre_vit import _native
    before = {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()}
    calls = [("spv_hadamard_mix", (0, 0, 0, 3, t, d, 1.0, H.CODE.get(dt, dt), 16 if ws else 0, 0)) for (dt, t, d, ws) in H.REFUSALS]
    calls += [("spv_hadamard_mix", (0, 0, 0, 0, 5, 8, 1.0, 0, 0, 0)),                      # empty batch
              ("spv_hadamard_mix", (0, 0, 0, 3, 5, 8, 1.0, 0, 0, 0)),                      # null tensors
              ("spv_hadamard_mix", (24, 32, 0, 3, 5, 8, 1.0, 0, 0, 0)),                    # one kernel, x off 16-byte alignment
              ("spv_hadamard_ln_fwd", (16, 16, 16, 16, 16, 16, 16, 1.0, 3, 66, 512, 1, 0)),
              ("spv_hadamard_ln_fwd", (16, 16, 16, 16, 16, 16, 16, 1.0, 3, 5, 512, 0, 0)),
              ("spv_hadamard_ln_fwd", (24, 16, 16, 16, 16, 16, 16, 1.0, 3, 5, 512, 1, 0)),
              ("spv_hadamard_ln_bwd", (16, 16, 16, 16, 16, 16, 16, 16, 16, 1.0, 3, 1, 512, 1, 0)),
              ("spv_hadamard_ln_bwd", (16, 16, 16, 16, 16, 16, 16, 0, 16, 1.0, 3, 5, 512, 1, 0)),   # dgamma without dbeta
              ("spv_hadamard_ln_bwd", (16, 16, 16, 16, 16, 24, 16, 16, 16, 1.0, 3, 5, 512, 1, 0)),
              ("spv_hadamard_cls_fwd", (16, 16, 16, 16, 16, 16, 16, 1.0, 3, 5, 128, 1, 0)),
              ("spv_hadamard_cls_fwd", (24, 16, 16, 16, 16, 16, 16, 1.0, 3, 5, 256, 1, 0)),
              ("spv_hadamard_cls_bwd", (16, 16, 16, 16, 16, 16, 16, 1.0, 3, 0, 256, 1, 0)),
              ("spv_hadamard_cls_bwd", (16, 16, 16, 16, 16, 8, 16, 1.0, 3, 5, 256, 1, 0))]
    for name, args in calls:
        assert len(args) == len(_native.SIGNATURES[name]), name
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value), (name, args, str(e.value))
    assert {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()} == before, "a refused call is not counted"


# ------------------------------------------------------------------------------------------ 4. rounding floors
def _mix32(x, tokens, dim):
    """the definition in float32: butterflies along dim, then along tokens, then s"""
    Np, Dp = H.next_pow2(tokens), H.next_pow2(dim)
    p = np.zeros(x.shape[:-2] + (Np, Dp), np.float32)
    p[..., :tokens, :dim] = np.asarray(x, np.float32)
    p = O.fwht(p, normalize=False)
    p = np.swapaxes(O.fwht(np.swapaxes(p, -1, -2).copy(), normalize=False), -1, -2)
    assert p.dtype == np.float32
    return p[..., :tokens, :dim] * np.float32(H.scale32(tokens, dim))


@pytest.mark.parametrize("case", [c for c in H.MIX_CASES if c.batch == max(b.batch for b in H.MIX_CASES if b[2:4] == c[2:4])], ids=H.case_id)
def test_float32_floor_of_the_mixer(case):
    c = case
    x = H.normal(H.rng_of(c, "A"), (c.batch, c.tokens, c.dim), c.dtype)
    e = R.err(_mix32(x, c.tokens, c.dim).astype(np.float64), H.mix(x), 1)
    assert e <= H.TRANSFORM_BAR / 4, (H.case_id(c), e)


def _ln32(a, gamma, beta):
    import torch
    t = torch.from_numpy(np.asarray(a, np.float32))
    return torch.nn.functional.layer_norm(t, (a.shape[-1],), torch.from_numpy(np.asarray(gamma, np.float32)),
                                          torch.from_numpy(np.asarray(beta, np.float32)), 1e-5).numpy()


@pytest.mark.parametrize("case", [c for c in H.LN_CASES if c.batch == 3], ids=H.case_id)
def test_float32_floor_of_the_fused_node(case):
    """forward and backward in float32 from the float32 prenorm; every quantity within a quarter of its fp32 bar"""
    import torch
    c, rng = case, H.rng_of(case, "fold")
    shape = (c.batch, c.tokens, 512)
    x = H.normal(rng, shape, "bf16")
    gamma, beta = H.affine(rng, 512)
    dout = H.normal(rng, shape, "bf16")
    pre32 = _mix32(x, c.tokens, 512)
    ref = H.ln_fwd(x, gamma, beta, prenorm=pre32)
    out32 = _ln32(pre32, gamma, beta) + np.asarray(x, np.float32)
    assert R.err(pre32, ref["prenorm"], 1) <= H.TRANSFORM_BAR / 4 and R.err(out32, ref["out"], 1) <= H.LN_BAR / 4
    mean32 = pre32.mean(-1, dtype=np.float32)
    rstd32 = 1.0 / np.sqrt(((pre32 - mean32[..., None]) ** 2).mean(-1, dtype=np.float32) + np.float32(1e-5))
    assert R.err(mean32, ref["mean"]) <= H.LN_BAR / 4 and R.err(rstd32, ref["rstd"]) <= H.LN_BAR / 4
    t = torch.from_numpy(pre32).requires_grad_(True)
    g, b = torch.from_numpy(np.asarray(gamma, np.float32)).requires_grad_(True), torch.from_numpy(np.asarray(beta, np.float32)).requires_grad_(True)
    torch.nn.functional.layer_norm(t, (512,), g, b, 1e-5).backward(torch.from_numpy(np.asarray(dout, np.float32)))
    bref = H.ln_bwd(dout, pre32, gamma)
    dx32 = _mix32(t.grad.numpy(), c.tokens, 512) + np.asarray(dout, np.float32)
    assert R.err(dx32, bref["dx"], 1) <= H.GRAD_BAR / 4
    assert R.err(g.grad.numpy(), bref["dgamma"]) <= H.GRAD_BAR / 4 and R.err(b.grad.numpy(), bref["dbeta"]) <= H.GRAD_BAR / 4


@pytest.mark.parametrize("case", [c for c in H.CLS_CASES if c.batch == 3], ids=H.case_id)
def test_float32_floor_of_the_row0_node(case):
    c, rng = case, H.rng_of(case)
    x, g1 = H.normal(rng, (c.batch, c.tokens, c.dim), c.dtype), H.normal(rng, (c.batch, c.dim), c.dtype)
    gamma, beta = H.affine(rng, c.dim)
    s32 = np.float32(H.scale32(c.tokens, c.dim))
    m0 = O.fwht(np.asarray(x, np.float32).sum(1, dtype=np.float32), normalize=False) * s32
    assert m0.dtype == np.float32
    ref = H.cls_fwd(x, gamma, beta, m0=m0)
    out = _ln32(m0, gamma, beta) + np.asarray(x, np.float32)[:, 0]
    assert R.err(m0, ref["m0"], 1) <= H.TRANSFORM_BAR / 4 and R.err(out, ref["out"], 1) <= H.LN_BAR / 4
    assert R.err(m0.mean(-1, dtype=np.float32), ref["mean"]) <= H.LN_BAR / 4
    import torch
    t = torch.from_numpy(m0).requires_grad_(True)
    torch.nn.functional.layer_norm(t, (c.dim,), torch.from_numpy(np.asarray(gamma, np.float32)), None, 1e-5).backward(
        torch.from_numpy(np.asarray(g1, np.float32)))
    row = O.fwht(t.grad.numpy(), normalize=False) * s32
    bref = H.cls_bwd(g1, m0, gamma, c.tokens)
    assert R.err(row + np.asarray(g1, np.float32), bref["dx"][:, 0], 1) <= H.GRAD_BAR / 4
    if c.tokens > 1:
        assert R.err(row, bref["dx"][:, 1], 1) <= H.GRAD_BAR / 4
