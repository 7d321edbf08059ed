"""tests/dropout_ref.py on the CPU: the properties of the restated mask, the float64 attention reference against the oracle's MHSA
core, and the condition under which the per-block bars of tests/test_gpu_attention_edges.py mean something: on every case of
tests/attention_edge_cases.py, both runs, the reference's own rounding floor (the same operation evaluated in numpy float32, resp. in
float64 with the masked P, dS and the outputs rounded to bf16) stays within 1/4 (fp32) resp. 1/2 (bf16) of the bar of every block."""
import numpy as np
import pytest
import torch

import attention_edge_cases as C
import dropout_ref as D
from oracle import spectre_oracle as O
from test_gpu_attention_mixer import TOL   # the bars of test_gpu_model.test_attention_core_vs_oracle: the one shared constant

BAR = {"fp32": TOL[torch.float32], "bf16": TOL[torch.bfloat16]}
GRAD_FACTOR = 2.0                          # gradients: twice the ctx bar, as test_attention_core_vs_oracle has it
SHARE = {"fp32": 0.25, "bf16": 0.5}        # the share of a bar the floor may take


def bar(dtype, name):
    """ctx: the dtype's bar; dq / dk / dv: twice that; the row-0 kernels' saved probabilities are fp32 whatever the dtype"""
    if name == "probs":
        return BAR["fp32"]
    return BAR[dtype] * (1.0 if name == "ctx" else GRAD_FACTOR)


def test_p_zero_keeps_everything():
    assert D.threshold(0.0) == 0
    assert D.keep(0x1234_5678_9ABC_DEF0, 37, 65, 0.0).all()
    assert D.inv_keep(0.0) == np.float32(1)


def test_thresholds_are_float32_arithmetic():
    assert [D.threshold(p) for p in (0.1, 0.3, 0.5)] == [6554, 19661, 32768]
    assert D.inv_keep(0.5) == np.float32(2) and D.inv_keep(0.3).dtype == np.float32


def test_column_pairs_share_one_hash_word():
    seed, rows, cols = 0xABCD_0000_1234, 9, 41
    h = D.hash_words(seed, np.arange(rows), (cols + 1) // 2)
    assert h.dtype == np.uint32 and len(np.unique(h)) == h.size
    for p in (0.1, 0.3, 0.5):
        k, thr = D.keep(seed, rows, cols, p), D.threshold(p)
        for j in range(cols // 2):
            assert np.array_equal(k[:, 2 * j], (h[:, j] & 0xFFFF) >= thr), (p, j)       # even column: the low 16 bits
            assert np.array_equal(k[:, 2 * j + 1], (h[:, j] >> 16) >= thr), (p, j)      # odd column: the high 16 bits
        assert np.array_equal(k[:, cols - 1], (h[:, cols // 2] & 0xFFFF) >= thr)        # an odd count's last column is an even one
    # a sub-range of the rows or columns is the same mask
    assert np.array_equal(D.keep_rows(seed, np.arange(3, 7), 20, 0.3), D.keep(seed, rows, cols, 0.3)[3:7, :20])


def test_high_seed_word_and_high_row_word_change_the_mask():
    lo = 0x0123_4567
    a, b = D.keep(lo, 64, 64, 0.5), D.keep(lo | (1 << 32), 64, 64, 0.5)
    assert 0.4 < (a != b).mean() < 0.6
    r = np.arange(64, dtype=np.uint64)
    assert 0.4 < (D.keep_rows(lo, r, 64, 0.5) != D.keep_rows(lo, r + np.uint64(1 << 32), 64, 0.5)).mean() < 0.6
    assert np.array_equal(a, D.keep_rows(lo, r, 64, 0.5))


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_keep_fraction_within_four_sigma(p):
    n_rows, n_cols = 1024, 1024
    k = D.keep(0xFEED_BEEF_0BAD_CAFE, n_rows, n_cols, p)
    q = 1.0 - D.threshold(p) / 65536.0
    n = n_rows * n_cols
    sigma = np.sqrt(q * (1.0 - q) / n)
    assert abs(k.mean() - q) <= 4.0 * sigma, (p, k.mean(), q, sigma)
    # and neither half of the hash word is worse than the other
    for half in (k[:, 0::2], k[:, 1::2]):
        assert abs(half.mean() - q) <= 4.0 * sigma * np.sqrt(2.0), (p, half.mean(), q)


def test_attention_keep_row_ids():
    S, H, L, p, seed = 2, 3, 5, 0.3, C.SEED
    m = D.attention_keep(seed, S, H, L, p)
    assert m.shape == (S, H, L, L)
    assert np.array_equal(m.reshape(S * H * L, L), D.keep(seed, S * H * L, L, p))
    assert np.array_equal(D.attention_keep(seed, S, H, L, p, row0=True), m[:, :, :1])


def test_reference_with_all_ones_mask_equals_oracle_mhsa():
    """identity projections turn the oracle's MHSA into its bare core: qkv = [x | x | x], out = ctx"""
    rng = np.random.default_rng(5)
    S, L, H, hd = 2, 9, 3, 4
    E = H * hd
    x, dout = rng.standard_normal((S, L, E)), rng.standard_normal((S, L, E))
    prm = dict(in_proj_weight=np.concatenate([np.eye(E) * a for a in (1.0, 0.5, -2.0)]), in_proj_bias=np.zeros(3 * E),
               out_proj_weight=np.eye(E), out_proj_bias=np.zeros(E))
    out, cache = O.mhsa_fwd(x, prm, H, batch_first=True)
    O.mhsa_bwd(dout, prm, H, cache, batch_first=True)
    _, q, k, v, att, _ = cache
    dctx = D.split_heads(dout, H)
    datt = dctx @ np.swapaxes(v, -1, -2)
    ds = att * (datt - (datt * att).sum(-1, keepdims=True)) / np.sqrt(hd)
    want = dict(ctx=D.split_heads(out, H), dq=ds @ k, dk=np.swapaxes(ds, -1, -2) @ q, dv=np.swapaxes(att, -1, -2) @ dctx, probs=att)
    for mask in (None, np.ones((S, H, L, L), bool)):
        got = D.attention(q, k, v, dctx, mask, 0.0)
        for name in want:
            np.testing.assert_allclose(got[name], want[name], rtol=1e-12, atol=1e-14, err_msg=name)
    # the mask multiplies P in the forward and dP in the backward: ctx is linear in V under a fixed mask, and a masked key gets no dV
    m = D.attention_keep(C.SEED, S, H, L, 0.3)
    got = D.attention(q, k, v, dctx, m, 0.3)
    np.testing.assert_allclose(got["ctx"], (att * m / (1.0 - np.float64(np.float32(0.3)))) @ v, rtol=1e-12)
    np.testing.assert_allclose((got["ctx"] * dctx).sum(), (got["dv"] * v).sum(), rtol=1e-10)


def test_block_errors_is_per_block_and_strict_on_zero_blocks():
    ref = np.zeros((1, 3, 2, 2)); ref[0, 0] = 100.0; ref[0, 1] = 1e-3
    got = ref.copy(); got[0, 1, 0, 0] += 1e-4; got[0, 2, 1, 1] = 1e-30
    e = D.block_errors(got, ref)
    assert e[0, 0] == 0 and abs(e[0, 1] - 0.1) < 1e-9 and np.isinf(e[0, 2])
    assert D.block_errors(ref, ref).max() == 0
    got[0, 0, 0, 0] = np.nan
    assert not D.block_errors(got, ref)[0, 0] <= 1.0


def test_bf16_round_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415926, 0.0])
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    assert np.array_equal(D.bf16_round(x), want) and want[1] == 1.0 and want[2] == 1.0 + 2.0 ** -6


def floors(ref, emu, names):
    return {n: float(D.block_errors(emu[n], ref[n]).max()) for n in names}


@pytest.mark.parametrize("run", ["A", "B"])
@pytest.mark.parametrize("case", C.CORE_CASES, ids=C.case_id)
def test_rounding_floor_within_its_share_of_the_bar_core(case, run):
    dtype = case[1]
    f = floors(C.core_reference(case, run), C.core_reference(case, run, dtype), ("ctx", "dq", "dk", "dv"))
    print(f"floor {C.case_id(case)} run {run}: {f}")
    bad = {n: v for n, v in f.items() if not v <= SHARE[dtype] * bar(dtype, n)}
    assert not bad, bad


@pytest.mark.parametrize("run", ["A", "B"])
@pytest.mark.parametrize("case", C.ROW0_CASES, ids=C.case_id)
def test_rounding_floor_within_its_share_of_the_bar_row0(case, run):
    dtype = case[0]
    ref = C.row0_reference(case, run)
    f = floors(ref, C.row0_reference(case, run, dtype), ("ctx", "dq", "dk", "dv"))
    f["probs"] = float(D.block_errors(C.row0_reference(case, run, "fp32")["probs"], ref["probs"]).max())
    print(f"floor row0 {C.case_id(case)} run {run}: {f}")
    bad = {n: v for n, v in f.items() if not v <= (SHARE["fp32"] if n == "probs" else SHARE[dtype]) * bar(dtype, n)}
    assert not bad, bad


def test_case_table_covers_every_family_in_every_dtype_it_exists_in():
    assert {(c[0], c[1]) for c in C.CORE_CASES} == {("v3", "bf16"), ("v2", "bf16"), ("v1", "bf16"), ("v2", "fp32"), ("v1", "fp32")}
    assert {c[0] for c in C.ROW0_CASES} == {"bf16", "fp32"}
    assert len(set(C.CORE_CASES)) == len(C.CORE_CASES) and C.SEED >> 32
