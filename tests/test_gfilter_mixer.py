"""CPU side of the learnable global-filter token mixer (SpectreViT(mixer="filter")): tests/gfilter_ref.py's float64 reference against
torch.fft + torch.autograd in float64 and against its circulant form; the float32 restatement of the generic kernels on exactly the
inputs tests/test_gpu_gfilter_mixer.py uses, within a quarter of each fp32 bar; the host restatement of csrc/spv_gfilter_core.h
against the header compiled by the host compiler and against the library's host-side answers; the public surface.

The generic kernels compute in float32 whatever the storage dtype.  The fast path (bf16, dim % 64 == 0, tokens <= 80) runs both
products on the MFMA with hi + lo bf16 tables and a hi + lo bf16 spectrum; gfilter_ref.fast_fwd32 / fast_bwd32 restate every rounding
of it before the final store and must stay within half of each bf16 bar, and element by element within a quarter of the c of
tests/mfma_mixer_ref.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gfilter_ref as G
import mfma_mixer_ref as M
import spectral_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CORE = os.path.join(os.path.dirname(HERE), "vit-spectre-experiments_amd", "csrc", "spv_gfilter_core.h")
TINY = dict(img_size=8, patch_size=4, in_channels=3, num_classes=10, embed_dim=16, num_encoders=2, num_heads=2, hidden_dim=24, dropout=0.0)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def _planted(rng, tokens, dim):
    w = rng.standard_normal((G.bins(tokens), dim, 2))
    w[G.inert(tokens), :, 1] = 1.5
    return w


# ------------------------------------------------------------------------------------------ 1. the definition and its gradients
@pytest.mark.parametrize("tokens", sorted(set(G.TOKENS) | {7, 6}))
def test_reference_equals_torch_fft_and_autograd_in_float64(tokens):
    rng = np.random.default_rng(tokens)
    x, dy, w = rng.standard_normal((3, tokens, 5)), rng.standard_normal((3, tokens, 5)), _planted(rng, tokens, 5)
    xt, wt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    y = torch.fft.irfft(torch.fft.rfft(xt, dim=1, norm="ortho") * torch.view_as_complex(wt), n=tokens, dim=1, norm="ortho")
    y.backward(torch.from_numpy(dy))
    assert R.err(G.fwd(x, w), y.detach().numpy(), 1) <= 1e-12
    assert R.err(G.dx(dy, w), xt.grad.numpy(), 1) <= 1e-12
    got = G.dw(x, dy)
    assert R.err(got, wt.grad.numpy()) <= 1e-12
    # the planted imaginary parts move nothing and receive exactly zero
    for k in G.inert(tokens):
        assert not wt.grad.numpy()[k, :, 1].any() and not got[k, :, 1].any() and not np.signbit(got[k, :, 1]).any()
    flat = w.copy()
    flat[G.inert(tokens), :, 1] = 0.0
    assert np.array_equal(G.fwd(x, flat), G.fwd(x, w))


@pytest.mark.parametrize("tokens", G.TOKENS)
def test_circulant_form_is_the_spectral_form(tokens):
    rng = np.random.default_rng(100 + tokens)
    x, w = rng.standard_normal((2, tokens, 6)), _planted(rng, tokens, 6)
    assert R.err(G.circulant(x, w), G.fwd(x, w), 1) <= 1e-12


# ------------------------------------------------------------------------------------------ 2. the generic kernels' arithmetic
def _fast(c):
    return G.path(c.dtype, c.tokens, c.dim, not c.off) == G.FAST


@pytest.mark.parametrize("case", [c for c in G.CASES if c.batch != 1 and _fast(c)], ids=G.case_id)
def test_restatement_of_the_fast_paths_arithmetic(case):
    """hi + lo bf16 tables, fp32 accumulation, the spectrum split into hi + lo bf16, hi.hi + lo.hi + hi.lo: on exactly the GPU test's
    inputs (the store of y / dx, the bar's 2^-8, is not part of it) within half of each bf16 bar, and, element by element in units of
    2^-24 S_i (tests/mfma_mixer_ref.py), within a quarter of the c the edge tests hold the kernel to: a restatement that drops a lo
    part does not meet the second (tests/test_mfma_mixer_ref.py)"""
    x, dy, w = G.inputs(case)
    y32 = G.fast_fwd32(x, w)
    dx32, dw32 = G.fast_bwd32(x, dy, w)
    errs = dict(y=R.err(y32, G.fwd(x, w), 1), dx=R.err(dx32, G.dx(dy, w), 1), dw=R.err(dw32, G.dw(x, dy)))
    print("GFILTER fast restatement", G.case_id(case), errs)
    assert errs["y"] <= G.bar(G.TRANSFORM_BAR, "bf16") / 2 and errs["dx"] <= G.bar(G.GRAD_BAR, "bf16") / 2 and errs["dw"] <= G.GRAD_BAR / 2, errs
    assert not dw32[G.inert(case.tokens), :, 1].any() and not np.signbit(dw32[G.inert(case.tokens), :, 1]).any()
    ref = M.filter_reference(x, dy, w)
    floors = {k: M.floor_units(v, ref, k) for k, v in dict(y=y32, dx=dx32, dw=dw32).items()}
    print("GFILTER fast restatement", G.case_id(case), "floors in units of 2^-24 S_i:", " ".join(f"{k}={v:.2f} (c / 4 = {M.C_BAR['fast_' + k] / 4})" for k, v in floors.items()))
    assert all(v <= M.C_BAR["fast_" + k] / 4 for k, v in floors.items()), floors


def test_fast_tables_are_a_hi_lo_split_of_the_float32_table():
    for tokens in (1, 2, 17, 63, 64, 65, 80):
        NP, NPO, KP = G.fast_pads(tokens)
        t1, t2 = G.fast_tables(tokens)
        K = G.bins(tokens)
        cos, sin = G.table32(tokens)
        m = (np.arange(K)[:, None] * np.arange(tokens)[None, :]) % tokens
        for part, f in enumerate((cos[m], sin[m])):
            assert np.abs((t1[0, part] + t1[1, part])[:K, :tokens] - f).max() <= 2.0 ** -17
            assert np.array_equal(t2[:, part, :tokens, :K], np.swapaxes(t1[:, part, :K, :tokens], 1, 2))
        assert not t1[:, :, K:].any() and not t1[:, :, :, tokens:].any() and not t2[:, :, tokens:].any() and not t2[:, :, :, K:].any()
        assert G.table_floats(tokens) == G.generic_table_floats(tokens) + (t1.size + t2.size) // 2
        assert NP % 16 == 0 and NPO % 32 == 0 and KP in (32, 64) and KP >= K and NP >= tokens and NPO >= tokens


@pytest.mark.parametrize("case", [c for c in G.CASES if c.batch != 1 and not _fast(c)], ids=G.case_id)
def test_float32_restatement_of_the_generic_kernels(case):
    """on exactly the GPU test's inputs: within a quarter of each fp32 bar"""
    x, dy, w = G.inputs(case)
    y32 = G.generic_fwd32(x, w)
    dx32, dw32 = G.generic_bwd32(x, dy, w)
    errs = dict(y=R.err(y32, G.fwd(x, w), 1), dx=R.err(dx32, G.dx(dy, w), 1), dw=R.err(dw32, G.dw(x, dy)))
    print("GFILTER fp32 restatement", G.case_id(case), errs)
    assert errs["y"] <= G.TRANSFORM_BAR / 4 and errs["dx"] <= G.GRAD_BAR / 4 and errs["dw"] <= G.GRAD_BAR / 4, errs
    assert not dw32[G.inert(case.tokens), :, 1].any()
    ref = M.filter_reference(x, dy, w)      # element by element, in units of 2^-24 S_i: within a quarter of the generic path's c
    floors = {k: M.floor_units(v, ref, k) for k, v in dict(y=y32, dx=dx32, dw=dw32).items()}
    assert all(v <= M.C_BAR["generic_" + k] / 4 for k, v in floors.items()), floors


# ------------------------------------------------------------------------------------------ 3. dispatch
def test_tables_reach_every_branch_and_both_sides_of_every_edge():
    plans = {c: G.select(c.dtype, c.tokens, c.dim) for c in G.CASES}
    assert {p.path for p in plans.values()} == {G.FAST, G.GENERIC}
    # the fast window: bf16 only, whole blocks of 64 columns only, up to 80 tokens, 16-byte aligned pointers only
    assert G.path("bf16", 80, 64) == G.path("bf16", 1, 512) == G.FAST and G.path("bf16", 81, 64) == G.GENERIC
    assert G.path("fp32", 65, 512) == G.path("bf16", 65, 72) == G.path("bf16", 65, 24) == G.GENERIC
    assert G.path("bf16", 65, 512, aligned=False) == G.REFUSE_ALIGN and G.path("bf16", 65, 72, aligned=False) == G.GENERIC
    fast = [c for c, p in plans.items() if p.path == G.FAST]
    assert {c.dim for c in fast} == {64, 512} and {c.batch for c in fast} == {1, 3, 70}
    # both sides of its tile edges: K steps of 16 tokens, output tiles of 32 tokens, one or two bin tiles, the end of the window
    assert {1, 2, 16, 17, 32, 33, 48, 49, 63, 64, 65, 80} <= {c.tokens for c in fast} and 81 in {c.tokens for c in G.CASES}
    assert G.fast_pads(63)[2] == 32 and G.fast_pads(64)[2] == 64 and G.fast_pads(16)[0] == 16 and G.fast_pads(17)[0] == 32
    assert all(G.path(c.dtype, c.tokens, c.dim, False) == G.REFUSE_ALIGN and c.off for c in G.MISALIGNED_REFUSED)
    assert all(G.path(c.dtype, c.tokens, c.dim, False) == G.GENERIC for c in G.CASES if c.off)
    assert {1, 2, 3, 4, 5, 16, 17, 32, 33, 64, 65, 197} <= {c.tokens for c in G.CASES} and {8, 24, 64, 512} <= {c.dim for c in G.CASES}
    assert {c.batch for c in G.CASES} == {1, 2, 3, 70} and G.slabs(70) == 32 < 70 and G.slabs(3) == 3
    assert [c for c in G.CASES if c.batch == 2] == [G.Case(dt, 2, G.MAX_TOKENS, 3) for dt in G.DTYPES]
    # column blocks: the whole dim, 64 of a larger dim (with and without a part block), fewer than 64 because of the LDS
    assert any(p.cols_fwd == c.dim < 64 for c, p in plans.items()) and any(p.cols_fwd == 64 and c.dim % 64 for c, p in plans.items())
    assert any(p.cols_fwd == 64 and c.dim % 64 == 0 and c.dim > 64 for c, p in plans.items())
    assert G.select("bf16", 125, 512).cols_fwd == 64 and G.select("bf16", 126, 512).cols_fwd == 63
    assert G.select("fp32", 63, 512).cols_bwd == 64 and G.select("fp32", 64, 512).cols_bwd == 62
    assert G.select("fp32", 197, 512).cols_fwd == 40 and G.select("fp32", 197, 512).cols_bwd == 20
    assert any(c.off for c in G.CASES)
    # the end of the token window, and the budget it comes from
    assert G.path("fp32", G.MAX_TOKENS, 8) == G.GENERIC and G.path("fp32", G.MAX_TOKENS + 1, 8) == G.REFUSE_TOKENS
    assert G.select("fp32", G.MAX_TOKENS, 8).cols_bwd == 1 and 4 * G.MAX_TOKENS + 4 * G.bins(G.MAX_TOKENS) <= G.LDS_FLOATS
    # ... which a case launches: 2 columns per workgroup forward, 1 backward, and both ask for exactly the accepted 16384 LDS floats
    for dt in G.DTYPES:
        p = plans[G.Case(dt, 2, 2730, 3)]
        assert G.MAX_TOKENS == 2730 and (p.path, p.bins, p.cols_fwd, p.cols_bwd) == (G.GENERIC, 1366, 2, 1)
        assert p.cols_fwd * (2730 + 2 * p.bins) + 2 * 2730 == p.cols_bwd * (2 * 2730 + 4 * p.bins) + 2 * 2730 == G.LDS_FLOATS == 16384
        assert G.LDS_FLOATS * 4 == 65536
    assert set(G.REFUSALS.values()) == {G.REFUSE_EMPTY, G.REFUSE_DTYPE, G.REFUSE_TOKENS}
    for p, c in ((p, c) for c, p in plans.items() if p.path == G.GENERIC):
        assert (p.cols_fwd * (c.tokens + 2 * p.bins) + 2 * c.tokens <= G.LDS_FLOATS
                and p.cols_bwd * (2 * c.tokens + 4 * p.bins) + 2 * c.tokens <= G.LDS_FLOATS)


SWEEP_T = (0, 1, 2, 3, 16, 17, 62, 63, 64, 65, 80, 81, 124, 125, 126, 127, 197, 1000, 2729, 2730, 2731, 4096, 32768)
SWEEP_D = (0, 1, 7, 8, 20, 41, 63, 64, 65, 72, 128, 512, 513)
SWEEP_B = (0, 1, 3, 31, 32, 33, 70, 512)

PROBE = r"""
#include <stdio.h>
#include <stdlib.h>
#include "%s"
int main(int argc, char** argv) {
    for (int i = 1; i + 4 < argc; i += 5) {
        const int dt = atoi(argv[i]), t = atoi(argv[i + 1]), d = atoi(argv[i + 2]), b = atoi(argv[i + 3]), al = atoi(argv[i + 4]);
        const GfilterPlan p = gfilter_select(dt, t, d, al != 0);
        printf("%%d %%d %%d %%d %%lld %%lld %%lld %%d\n", p.path, p.bins, p.cols_fwd, p.cols_bwd, (long long)gfilter_table_floats(t),
               (long long)gfilter_workspace_floats(b, t, d), (long long)gfilter_partial_floats(b, t, d), gfilter_slabs(b));
    }
    return 0;
}
"""


def test_host_selector_compiled_from_the_header_agrees_with_the_restatement(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE % CORE)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", str(src), "-o", str(exe)])
    quads = [(dt, t, d, b, al) for dt in (0, 1, 2) for t in SWEEP_T for d in SWEEP_D for al in (1, 0)
             for b in (SWEEP_B if (t, d) in ((65, 512), (5, 8), (0, 8)) else (3,))]
    lines = []
    for i in range(0, len(quads), 400):   # argv stays short
        args = [str(v) for q in quads[i:i + 400] for v in q]
        lines += subprocess.check_output([str(exe)] + args, text=True).split("\n")[:-1]
    assert len(lines) == len(quads)
    for (dt, t, d, b, al), line in zip(quads, lines):
        p = G.select(dt, t, d, bool(al))
        want = (p.path, p.bins, p.cols_fwd, p.cols_bwd, G.table_floats(t), G.workspace_floats(b, t, d), G.partial_floats(b, t, d), G.slabs(b))
        assert tuple(int(v) for v in line.split()) == want, ((dt, t, d, b, al), line, want)


def test_library_answers_agree_with_the_restatement(built):
    from spectre_vit import _native as nat
    for c in G.CASES:
        for al in (0, 1):
            assert nat.call("spv_gfilter_path", G.CODE[c.dtype], c.tokens, c.dim, al) == G.path(c.dtype, c.tokens, c.dim, bool(al)), c
        assert nat.call("spv_gfilter_workspace_floats", c.batch, c.tokens, c.dim) == G.workspace_floats(c.batch, c.tokens, c.dim)
        assert nat.call("spv_gfilter_partial_floats", c.batch, c.tokens, c.dim) == G.partial_floats(c.batch, c.tokens, c.dim)
        assert nat.call("spv_gfilter_table_floats", c.tokens) == G.table_floats(c.tokens)
    for (dt, t, d), why in G.REFUSALS.items():
        assert nat.call("spv_gfilter_path", G.CODE.get(dt, dt), t, d, 1) == G.path(dt, t, d) == why, (dt, t, d)
    for t in SWEEP_T:
        for d in SWEEP_D:
            for dt in (0, 1, 2):
                for al in (0, 1):
                    assert nat.call("spv_gfilter_path", dt, t, d, al) == G.path(dt, t, d, bool(al)), (dt, t, d, al)
            assert nat.call("spv_gfilter_table_floats", t) == G.table_floats(t), t
            for b in SWEEP_B:
                assert nat.call("spv_gfilter_partial_floats", b, t, d) == G.partial_floats(b, t, d), (b, t, d)


def test_refused_calls_fail_on_the_host_and_are_not_counted(built):
    """NULL tensors: a call that got past the host checks would fault"""
    from spectre_vit import _native
    before = {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()}
    calls = []
    for (dt, t, d), _ in G.REFUSALS.items():
        calls += [("spv_gfilter_fwd", (16, 16, 16, 16, 3, t, d, G.CODE.get(dt, dt), 0, 0)),
                  ("spv_gfilter_bwd", (16, 16, 16, 16, 16, 16, 16, 3, t, d, G.CODE.get(dt, dt), 0, 0))]
    calls += [("spv_gfilter_fwd", (16, 16, 16, 16, 0, 5, 8, 0, 0, 0)),              # empty batch
              ("spv_gfilter_bwd", (16, 16, 16, 16, 16, 16, 16, 0, 5, 8, 0, 0, 0)),
              ("spv_gfilter_fwd", (0, 0, 0, 0, 3, 5, 8, 0, 0, 0)),                  # null tensors
              ("spv_gfilter_fwd", (16, 16, 16, 0, 3, 5, 8, 0, 0, 0)),               # no table
              ("spv_gfilter_bwd", (16, 16, 16, 16, 16, 16, 0, 3, 5, 8, 1, 0, 0)),   # no slabs
              ("spv_gfilter_fwd", (24, 16, 32, 16, 3, 7, 64, 1, 0, 0)),             # fast shape, x off 16-byte alignment
              ("spv_gfilter_fwd", (16, 16, 40, 16, 3, 7, 64, 1, 0, 0)),             # ... y
              ("spv_gfilter_bwd", (16, 24, 16, 32, 16, 16, 16, 3, 65, 512, 1, 0, 0)),   # ... dy
              ("spv_gfilter_bwd", (16, 16, 16, 40, 16, 16, 16, 3, 65, 512, 1, 0, 0)),   # ... dx
              ("spv_gfilter_make_tables", (0, 5, 0)), ("spv_gfilter_make_tables", (16, 0, 0))]
    for name, args in calls:
        assert len(args) == len(_native.SIGNATURES[name]), name
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value), (name, args, str(e.value))
    assert {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()} == before, "a refused call is not counted"


# ------------------------------------------------------------------------------------------ 4. the public surface
def test_symbols_are_declared_bound_and_the_census_is_unchanged(built):
    from conftest import ROOT
    from spectre_vit import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "spv.h")).read()
    names = ["spv_gfilter_path", "spv_gfilter_table_floats", "spv_gfilter_make_tables", "spv_gfilter_workspace_floats",
             "spv_gfilter_partial_floats", "spv_gfilter_fwd", "spv_gfilter_bwd"]
    assert sorted(n for n in _native.SIGNATURES if "gfilter" in n) == sorted(names)
    assert sorted(set(re.findall(r"\b(spv_gfilter_[a-z_]+)\(", hdr))) == sorted(names)
    for name in names:
        assert getattr(lib, name).argtypes == _native.SIGNATURES[name]
        decl = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", hdr)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name]), name
    enum = dict(re.findall(r"(SPV_PATH_[A-Z0-9_]+)\s*=\s*(\d+)", hdr))
    assert int(enum["SPV_PATH_COUNT"]) == 27 and len(_native.PATH) == 27 and sorted(_native.PATH.values()) == list(range(27))
    assert lib.spv_version() == 1
    codes = dict(re.findall(r"#define (SPV_GFILTER_[A-Z_]+) \(?(-?\d+)\)?", hdr))
    assert {k: int(v) for k, v in codes.items()} == dict(SPV_GFILTER_FAST=G.FAST, SPV_GFILTER_REFUSE_ALIGN=G.REFUSE_ALIGN, SPV_GFILTER_GENERIC=G.GENERIC, SPV_GFILTER_REFUSE_EMPTY=G.REFUSE_EMPTY,
                                                         SPV_GFILTER_REFUSE_DTYPE=G.REFUSE_DTYPE, SPV_GFILTER_REFUSE_TOKENS=G.REFUSE_TOKENS)


def test_filter_model_constructs_on_the_cpu_and_round_trips_its_state(built):
    from spectre_vit.models.spectre.spectre import MIXERS, SpectreViT
    from spectre_vit.modules.mixers import GlobalFilterMixer
    assert MIXERS[-1] == "filter" and MIXERS[:6] == ("permut", "fft", "dwt_embed", "dwt_token", "attention", "hadamard")
    torch.manual_seed(3)
    m = SpectreViT(**TINY, mixer="filter")
    tokens, dim = (8 // 4) ** 2 + 1, 16
    for i, layer in enumerate(m.encoder_blocks.layers):
        assert isinstance(layer.mix_layer, GlobalFilterMixer)
        w = layer.mix_layer.complex_weight
        assert isinstance(w, torch.nn.Parameter) and w.dtype == torch.float32 and tuple(w.shape) == (tokens // 2 + 1, dim, 2) and w.requires_grad
        assert 0.005 < float(w.detach().std()) < 0.04, "0.02 * randn"
        assert f"encoder_blocks.layers.{i}.mix_layer.complex_weight" in m.state_dict()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    other = SpectreViT(**TINY, mixer="filter")
    assert other.load_state_dict(sd, strict=True).missing_keys == []
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items())
    fft_keys = set(SpectreViT(**TINY, mixer="fft").state_dict())
    assert set(sd) - fft_keys == {f"encoder_blocks.layers.{i}.mix_layer.complex_weight" for i in range(2)}
    with pytest.raises(ValueError):
        SpectreViT(**TINY, mixer="nope")
    with pytest.raises(ValueError):
        GlobalFilterMixer(0, 8)
