"""CPU checks behind tests/test_gpu_spectral_edges.py: the restated dispatch rules agree with the library's host-side answers on every
case and the tables reach every branch; tests/spectral_ref.py agrees with independent float64 formulations at 1e-12; the float32 floor
of each transform on the tables' inputs stays within a quarter of its fp32 bar, and a bf16 restatement of the multi-level Haar within
the bf16 bar; each of nine plausible kernel mistakes, made in a numpy emulation, exceeds the bar of a case; and the host refuses what no
kernel serves before any launch."""
import numpy as np
import pytest
import torch

import dropout_ref as D
import spectral_edge_cases as C
import spectral_ref as R
from oracle import spectre_oracle as O


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


# ------------------------------------------------------------------------------------------ 1. dispatch
def test_expected_path_agrees_with_the_library(built):
    from spectre_vit import _native as nat
    for c in C.MIX_CASES:
        assert nat.call("spv_fnet_workspace_floats", c.batch, c.tokens, c.dim) == C.workspace_floats(c.dtype, c.batch, c.tokens, c.dim), c
        assert nat.call("spv_fnet_ln_supported", c.tokens, c.dim, C.CODE[c.dtype]) == C.fnet_ln_supported(c.dtype, c.tokens, c.dim) == 0, c
        assert C.mix_path(c.dtype, c.tokens, c.dim)[0] in ("lds", "generic"), c
    for c in C.MFMA_CASES:
        assert nat.call("spv_fnet_workspace_floats", c.batch, c.tokens, 512) == 0
        assert nat.call("spv_fnet_ln_supported", c.tokens, 512, C.SPV_BF16) == 1 and C.mix_path("bf16", c.tokens, 512) == ("mfma",)
    for t in (1, 2, 65, 79, 300):
        assert nat.call("spv_fnet_twiddle_floats", t) == C.twiddle_floats(t)
    for dt in C.DTYPES:
        for t, d in ((1, 512), (2, 512), (65, 512), (66, 512), (65, 256), (65, 1024)):
            assert nat.call("spv_fnet_ln_supported", t, d, C.CODE[dt]) == C.fnet_ln_supported(dt, t, d)
        for d in (128, 256, 512, 1024, 2048):
            assert nat.call("spv_fnet_cls_supported", 5, d, C.CODE[dt]) == C.cls_supported(dt, 5, d) == int(d in (256, 512, 1024))
            assert nat.call("spv_haar_ln_supported", d, C.CODE[dt]) == C.haar_ln_supported(dt, d)
    for c in C.HAAR_LN_CASES:
        assert nat.call("spv_tail_bwd_parts", c.rows) == min(-(-c.rows // 4), 1024)
    # the LDS rule is include/spv.h's (tokens + 3) * dim * 4 <= 160 KiB, swept over the whole fast range
    for dim in (8, 64, 512, 1024, 2048, 4096, 8192):
        for t in range(1, 90):
            assert (nat.call("spv_fnet_workspace_floats", 1, t, dim) == 0) == (C.mix_path("fp32", t, dim)[0] == "lds"), (t, dim)


def test_tables_cover_every_dispatch_branch():
    missing = []

    def need(what, ok):
        if not ok:
            missing.append(what)

    mix = {(C.mix_path(c.dtype, c.tokens, c.dim), c.dtype) for c in C.MIX_CASES}
    for dt in C.DTYPES:
        for mh in C.MH_STEPS:
            need(f"lds<{mh}> {dt}", (("lds", mh), dt) in mix)
            plans = {tuple(C.fft_passes(c.dim)) for c in C.MIX_CASES if c.dtype == dt and C.mix_path(dt, c.tokens, c.dim) == ("lds", mh)}
            need(f"lds<{mh}> {dt} at two FFT plans", len(plans) >= 2)
        for reason in ("non-power-of-two", "dim < 8", "tokens > 79", "over the LDS"):
            need(f"generic {reason} {dt}", (("generic", reason), dt) in mix)
        need(f"odd and even tokens on the LDS path {dt}", {c.tokens % 2 for c in C.MIX_CASES if c.dtype == dt and c.dim == 1024} == {0, 1})
        need(f"fwht rpw > 1 {dt}", any(c.dtype == dt and C.fwht_rpw(c.n) > 1 and c.rows == C.fwht_rpw(c.n) + 1 for c in C.FWHT_CASES))
        need(f"fwht rpw = 1 {dt}", any(c.dtype == dt and C.fwht_rpw(c.n) == 1 and c.rows > 1 for c in C.FWHT_CASES))
        for d in (256, 512, 1024):
            rg = C.cls_row_groups(dt)
            toks = {c.tokens for c in C.CLS_CASES if c.dtype == dt and c.dim == d}
            need(f"cls {d} {dt}", any(t < rg for t in toks) and rg in toks and any(t > rg and t % rg for t in toks))
        plans = {tuple(C.haar_plan(c)) for c in C.HAAR_CASES + C.HAAR_BIG_CASES if c.dtype == dt}
        need(f"haar scalar {dt}", ("scalar",) in plans and ("scalar", "scalar") in plans)
        need(f"haar vector never in fp32 / present in bf16 {dt}", any("vector" in p for p in plans) == (dt == "bf16"))
    need("generic off 16-byte alignment", all(any(c.off and c.dtype == dt and C.mix_path(dt, c.tokens, c.dim)[0] == "generic" for c in C.MIX_CASES) for dt in C.DTYPES)
         and all(C.mix_path(c.dtype, c.tokens, c.dim)[0] == "generic" for c in C.MIX_CASES if c.off))
    need("one- to four-pass FFT plans", {len(C.fft_passes(c.dim)) for c in C.MIX_CASES if C.mix_path(c.dtype, c.tokens, c.dim)[0] == "lds"} >= {1, 2, 3, 4})
    # every selector and capacity boundary, from both sides
    for lo, hi in ((15, 16), (35, 36), (51, 52), (67, 68), (79, 80)):
        a = {C.mix_path("fp32", t, 8) for t in (lo, hi)}
        need(f"token boundary {lo}/{hi}", len(a) == 2 and all(any(c.tokens == t and c.dim <= 32 for c in C.MIX_CASES) for t in (lo, hi)))
    for (lo, hi), dim, dt in (((37, 38), 1024, "bf16"), ((17, 18), 2048, "bf16"), ((7, 8), 4096, "bf16"), ((77, 78), 512, "fp32")):
        need(f"LDS boundary {lo}|{hi} x {dim}", C.mix_path(dt, lo, dim)[0] == "lds" and C.mix_path(dt, hi, dim) == ("generic", "over the LDS")
             and all(C.Mix(dt, 3, t, dim) in C.MIX_CASES for t in (lo, hi)))
    need("MFMA window ends", C.mix_path("bf16", 1, 512) == ("lds", 4) and C.mix_path("bf16", 66, 512) == ("lds", 17)
         and C.Mix("bf16", 3, 1, 512) in C.MIX_CASES and C.Mix("bf16", 3, 66, 512) in C.MIX_CASES)
    need("mfma with and without row 32, stagger", {c.tokens >= 64 for c in C.MFMA_CASES} == {False, True} and any(c.batch >= 512 for c in C.MFMA_CASES))
    bf = [c for c in C.HAAR_CASES if c.dtype == "bf16"]
    for plan in (["vector"], ["vector", "scalar"], ["scalar", "vector"], ["scalar", "scalar"], ["vector"] * 6, ["scalar"] + ["vector"] * 4, ["scalar"] + ["vector"] * 5):
        need(f"haar plan {plan}", any(C.haar_plan(c) == plan for c in bf))
    need("haar misaligned x takes the scalar kernel first", all(C.haar_plan(c)[0] == "scalar" for c in bf if c.off) and any(c.off for c in bf))
    need("haar grid-stride trips", {tuple(C.haar_plan(c)) for c in C.HAAR_BIG_CASES} == {("scalar",), ("vector",)})
    need("haar_ln beyond both caps", any(c.rows > max(C.HAAR_LN_FWD_CAP_ROWS, C.HAAR_LN_BWD_CAP_ROWS) for c in C.HAAR_LN_CASES))
    assert not missing, missing


def test_no_case_is_refused():
    for family, cases in C.ALL.items():
        for c in cases:
            assert C.expected_path(c)[0] != "refused", (family, C.case_id(c))
    assert C.expected_path(C.Rfft("fp32", 3, 8193, 0)) == ("refused", "dim too large") and C.expected_path(C.Cls("bf16", 3, 5, 128))[0] == "refused"
    assert C.expected_path(C.Haar("bf16", 2, 3, 48, 2, 2, 0)) == ("haar", "vector", "scalar") and C.expected_path(C.Mfma(3, 65)) == ("mfma",)


def test_restated_rules_at_their_edges():
    assert C.mix_path("fp32", 4, 8192) == ("refused", "shape too large") and C.mix_path("fp32", 8193, 3) == ("refused", "shape too large")
    assert C.mix_path("fp32", 7, 48, workspace=False) == ("refused", "workspace") and C.mix_path("fp32", 5, 64, twiddle=False) == ("refused", "twiddle")
    assert C.mix_path("bf16", 65, 512, twiddle=False) == ("refused", "twiddle") and C.mix_path("fp32", 5, 64, count=0) == ("refused", "empty")
    assert C.mix_path("fp32", 65, 512) == ("lds", 17) and C.mix_path("bf16", 65, 512) == ("mfma",)
    assert [C.fft_passes(d) for d in (8, 16, 32, 64, 512, 4096)] == [[8], [8, 2], [8, 4], [8, 8], [8, 8, 8], [8, 8, 8, 8]]
    assert C.haar_plan(C.Haar("bf16", 2, 3, 48, 2, 2, 1)) == ["scalar", "vector"] and C.haar_plan(C.Haar("fp32", 2, 3, 512, 2, 5, 0)) == ["scalar"] * 5
    assert C.haar_refused(0, 1) == "axis" and C.haar_refused(2, 0) == C.haar_refused(2, 17) == "levels" and C.haar_refused(2, 2, False) == "scratch"
    assert C.fwht_refused(12, 12, 12) == C.fwht_refused(8, 32768, 8) == "power of two" and C.fwht_refused(9, 8, 8) == "outside"
    assert [C.fwht_rpw(n) for n in (1, 256, 512, 16384)] == [512, 2, 1, 1]


def test_bars_are_the_stated_ones():
    assert (C.TRANSFORM_BAR, C.HAAR_BAR, C.LN_BAR, C.GRAD_BAR, C.MFMA_BAR, C.MFMA_DX_BAR) == (2e-5, 1e-6, 3e-5, 6e-5, 1e-2, 3e-2)
    assert C.bar(2e-5, "fp32") == 2e-5 and C.bar(2e-5, "bf16") == 2e-5 + 2.0 ** -8 and C.bar(3e-5, "bf16", stored=False) == 3e-5


# ------------------------------------------------------------------------------------------ 2. references vs independent formulas
@pytest.mark.parametrize("case", [c for c in C.MIX_CASES if c.dtype == "fp32" and c.dim <= 1024 and c.batch == 3], ids=C.case_id)
def test_re_fft2_equals_the_cos_sin_matrix_product(case):
    x = C.normal(C.rng_of(case, "A"), (case.batch, case.tokens, case.dim), "fp32")
    assert R.err(R.fnet_mix(x), O.fnet_mix_fwd(np.array(x)), 1) <= 1e-12


@pytest.mark.parametrize("dim", [1, 2, 7, 16, 255, 256, 257, 1000])
def test_rfft_real_equals_the_cosine_matrix_product(dim):
    rng = np.random.default_rng(dim)
    x, dy = rng.standard_normal((3, dim)), rng.standard_normal((3, dim // 2 + 1))
    assert R.err(R.rfft_real(x, dim, 0), O.fft_module_fwd(x), 1) <= 1e-12
    assert R.err(R.rfft_real(dy, dim, 1), O.fft_module_bwd(dy, dim), 1) <= 1e-12


def test_haar_reference_on_the_pywt_vectors():
    """the vectors PyWavelets documents for 'haar' (tests/test_oracle_golden.py cites them), through spv_haar_dwt's argument convention"""
    x = np.array([1.0, 2.0, 3.0, 4.0]).reshape(1, 1, 4)
    assert np.allclose(R.haar(x, 2, 1, 0)[0, 0], [2.12132034, 4.94974747, -0.70710678, -0.70710678], atol=1e-8)
    assert np.allclose(R.haar(x.reshape(1, 4, 1), 1, 1, 0)[0, :, 0], [2.12132034, 4.94974747, -0.70710678, -0.70710678], atol=1e-8)
    odd = np.array([1.0, 2.0, 3.0]).reshape(1, 1, 3)
    assert np.allclose(R.haar(odd, 2, 1, 0)[0, 0], [3 / np.sqrt(2), 3.0, -1 / np.sqrt(2)])             # pass-through
    assert np.allclose(R.haar(odd, 2, 1, 2)[0, 0], [3 / np.sqrt(2), 3 / np.sqrt(2), -1 / np.sqrt(2)])  # pywt mode="zero": cA of (3, 0)
    cA, _ = O.haar_level_pywt_zero(odd[0, 0])
    assert np.allclose(R.haar(odd, 2, 1, 2)[0, 0, :2], cA)
    # bit 0 is the adjoint: <y, A x> = <A^T y, x> in both modes, several levels, both axes
    rng = np.random.default_rng(7)
    for axis, mode in ((1, 0), (1, 2), (2, 0), (2, 2)):
        a, b = rng.standard_normal((2, 9, 11)), rng.standard_normal((2, 9, 11))
        assert abs((b * R.haar(a, axis, 3, mode)).sum() - (R.haar(b, axis, 3, mode | 1) * a).sum()) <= 1e-12 * 200


@pytest.mark.parametrize("n", [1, 2, 8, 256])
def test_fwht_reference_equals_the_sylvester_matrix(n):
    H = np.array([[1.0]])
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    x = np.random.default_rng(n).standard_normal((3, n))
    assert R.err(R.fwht(x, n, n, 0, 1, 1.0), x @ H.T, 1) <= 1e-12
    # mode 1 is a signed permutation of the same rows (a Hadamard matrix), and mode 2 its transpose
    A = R.fwht(np.eye(n), n, n, 1, 1, 1.0).T
    assert np.array_equal(A @ A.T, n * np.eye(n)) and np.array_equal(R.fwht(np.eye(n), n, n, 2, 1, 1.0).T, A.T)
    assert np.array_equal(A, A.T)   # ... and symmetric: mode 2 equals mode 1 as an operator, whatever the stage order
    assert sorted(map(tuple, A.tolist())) == sorted(map(tuple, H.tolist()))


def test_fused_references_equal_torch_float64_autograd():
    rng = np.random.default_rng(3)
    T = lambda a: torch.from_numpy(np.array(a, np.float64))
    B, N, Dm = 2, 5, 16
    x, dout, g1 = rng.standard_normal((B, N, Dm)), rng.standard_normal((B, N, Dm)), rng.standard_normal((B, Dm))
    gamma, beta = 0.5 + rng.random(Dm), 0.1 * rng.standard_normal(Dm)
    xt, gt, bt = T(x).requires_grad_(True), T(gamma).requires_grad_(True), T(beta).requires_grad_(True)
    pre = torch.fft.fft2(xt).real
    out = torch.nn.functional.layer_norm(pre, (Dm,), gt, bt, 1e-5) + xt
    fwd = R.fnet_ln_fwd(x, gamma, beta)
    assert R.err(fwd["out"], out.detach().numpy(), 1) <= 1e-12 and R.err(fwd["prenorm"], pre.detach().numpy(), 1) <= 1e-12
    (out * T(dout)).sum().backward()
    # the reference rounds LN-backward(dout) to bf16 before the transform, as the kernel does: undo that here by feeding a dout whose
    # LayerNorm backward is exact in bf16 -- instead compare the unrounded composition
    dm, dg, db = R.ln_bwd(dout, fwd["prenorm"], gamma)
    assert R.err(R.fnet_mix(dm) + dout, xt.grad.numpy(), 1) <= 1e-12
    assert R.err(dg.sum((0, 1)), gt.grad.numpy()) <= 1e-12 and R.err(db.sum((0, 1)), bt.grad.numpy()) <= 1e-12
    bwd = R.fnet_ln_bwd(dout, fwd["prenorm"], gamma)
    assert R.err(bwd["dgamma"], gt.grad.numpy()) <= 1e-12 and R.err(bwd["partials"].sum(0)[1], bt.grad.numpy()) <= 1e-12
    assert R.err(bwd["dx"], xt.grad.numpy(), 1) <= 2.0 ** -8     # one bf16 rounding of dm, through a unitary-like map
    # row 0 of the same node
    xt.grad = gt.grad = bt.grad = None
    out0 = (torch.nn.functional.layer_norm(torch.fft.fft2(xt).real, (Dm,), gt, bt, 1e-5) + xt)[:, 0]
    cf = R.cls_fwd(x, gamma, beta)
    assert R.err(cf["out"], out0.detach().numpy(), 1) <= 1e-12 and R.err(cf["m0"], pre.detach().numpy()[:, 0], 1) <= 1e-12
    (out0 * T(g1)).sum().backward()
    cb = R.cls_bwd(g1, cf["m0"], gamma, N)
    assert R.err(cb["dx"], xt.grad.numpy(), 1) <= 1e-12 and R.err(cb["partials"].sum(0)[0], gt.grad.numpy()) <= 1e-12
    # Haar + LayerNorm: the band the fused kernels form is the oracle's level, rounded once
    xb = D.bf16_round(rng.standard_normal((5, 512)))
    band = O.haar_dwt_fwd(xb, axis=-1, levels=1)
    assert R.err(R.haar_band_bf16(xb), band, 1) <= 2.0 ** -8 and np.array_equal(R.haar_band_bf16(xb), D.bf16_round(R.haar_band_bf16(xb)))


# ------------------------------------------------------------------------------------------ 3. rounding floors
def _f32(a):
    return torch.from_numpy(np.array(a, np.float32))


@pytest.mark.parametrize("case", C.MIX_CASES + [C.Mix("bf16", c.batch, c.tokens, 512) for c in C.MFMA_CASES if c.batch <= 3], ids=C.case_id)
def test_float32_floor_of_re_fft2(case):
    """measured on these inputs: <= 2.4e-7"""
    x = C.normal(C.rng_of(case, "A"), (case.batch, case.tokens, case.dim), case.dtype)
    low = torch.fft.fft2(_f32(x)).real.numpy().astype(np.float64)
    assert R.err(low, R.fnet_mix(x), 1) <= C.TRANSFORM_BAR / 4


@pytest.mark.parametrize("case", [c for c in C.RFFT_CASES if c.rows == 3], ids=C.case_id)
def test_float32_floor_of_rfft_real(case):
    """a float32 matrix product; measured: <= 4.7e-7"""
    c = case
    K = c.dim // 2 + 1
    x = C.normal(C.rng_of(c), (c.rows, K if c.transpose else c.dim), c.dtype)
    k, n = np.arange(K), np.arange(c.dim)
    Cm = np.cos(2.0 * np.pi * ((k[:, None] * n[None, :]) % c.dim) / c.dim).astype(np.float32)
    low = (_f32(x) @ torch.from_numpy(Cm if c.transpose else Cm.T.copy())).numpy().astype(np.float64)
    assert R.err(low, R.rfft_real(x, c.dim, c.transpose), 1) <= C.TRANSFORM_BAR / 4


def _lines(c, a):
    return np.swapaxes(a, 1, 2) if c.axis == 1 else a


def _haar_low(c, x, rnd):
    """the level loop of spv_haar_dwt in float32, every level's tensor stored through rnd"""
    mode = "zero" if c.inverse & 2 else "passthrough"
    x = np.moveaxis(np.array(x, np.float32), c.axis, -1)
    length, lens = x.shape[-1], []
    for _ in range(c.levels):
        lens.append(length)
        length -= length // 2
    for ln in (lens[::-1] if c.inverse & 1 else lens):
        head = x[..., :ln]
        if c.inverse & 1:
            new = O.haar_level_bwd(head[..., :ln - ln // 2], head[..., ln - ln // 2:], -1, mode)
        else:
            new = np.concatenate(O.haar_level_fwd(head, -1, mode), axis=-1)
        x = rnd(np.concatenate([new.astype(np.float32), x[..., ln:]], axis=-1))
    return np.moveaxis(x, -1, c.axis).astype(np.float64)


@pytest.mark.parametrize("case", C.HAAR_CASES, ids=C.case_id)
def test_low_precision_restatement_of_the_haar_levels_stays_inside_the_bar(case):
    """fp32: the level loop in float32 within a quarter of the fp32 bar.  bf16: every level's tensor is STORED as bf16 (y / scratch
    ping-pong), so a level-J coefficient carries J roundings.  With exact arithmetic and nothing but those roundings the loop misses
    1e-6 + 2^-8 from two levels on (measured on these inputs: up to 4.7e-3 at two levels, 6.5e-3 at seven), which is why
    spectral_edge_cases.haar_bar allows one unit roundoff per store; the restatement stays within that bar at every depth."""
    c = case
    x = C.normal(C.rng_of(c), (c.batch, c.tokens, c.dim), c.dtype)
    if c.dtype == "fp32":
        low, limit = _haar_low(c, x, lambda a: a), C.HAAR_BAR / 4
    else:
        low, limit = _haar_low(c, x, lambda a: D.bf16_round(a.astype(np.float64)).astype(np.float32)), C.haar_bar(c)
    e = R.err(_lines(c, low), _lines(c, R.haar(x, c.axis, c.levels, c.inverse)), 2)
    assert e <= limit, (C.case_id(c), e, limit)


@pytest.mark.parametrize("case", [c for c in C.FWHT_CASES if c.dtype == "fp32"], ids=C.case_id)
def test_float32_floor_of_fwht(case):
    c, rng = case, C.rng_of(case)
    x = C.normal(rng, (c.rows, c.n_in), c.dtype)
    y = np.concatenate([np.array(x, np.float32), np.zeros((c.rows, c.n - c.n_in), np.float32)], axis=1)
    step = {0: lambda a: O.fwht(a, normalize=False), 1: O.fwht_fast_fwd, 2: O.fwht_fast_bwd}[c.mode]
    for _ in range(c.repeat):
        y = step(y)
    assert y.dtype == np.float32
    low = (y[:, :c.n_out] * np.float32(C.fwht_scale(c))).astype(np.float64)
    assert R.err(low, R.fwht(x, c.n, c.n_out, c.mode, c.repeat, C.fwht_scale(c)), 1) <= C.TRANSFORM_BAR / 4


@pytest.mark.parametrize("case", [c for c in C.CLS_CASES if c.batch == 3 and c.tokens in (1, 65)], ids=C.case_id)
def test_float32_floor_of_the_row0_node(case):
    c, rng = case, C.rng_of(case)
    x, g1 = C.normal(rng, (c.batch, c.tokens, c.dim), c.dtype), C.normal(rng, (c.batch, c.dim), c.dtype)
    gamma, beta = C.affine(rng, c.dim)
    m0 = torch.fft.fft(_f32(x).sum(1)).real
    out = torch.nn.functional.layer_norm(m0, (c.dim,), _f32(gamma), _f32(beta), 1e-5) + _f32(x)[:, 0]
    ref = R.cls_fwd(x, gamma, beta)
    assert R.err(m0.numpy(), ref["m0"], 1) <= C.TRANSFORM_BAR / 4 and R.err(out.numpy(), ref["out"], 1) <= C.LN_BAR / 4
    assert R.err(m0.mean(-1).numpy(), ref["mean"]) <= C.LN_BAR / 4


# ------------------------------------------------------------------------------------------ 4. sensitivity
def emulate_quadrants(x, add_in=None, mut=None, pad=0.0):
    """float64 restatement of how fnet_lds_kernel (and, with m = 32 on its own path, fnet_mfma_kernel) fills y [N, D] of one sample:
    P, Q for m <= N / 2, k <= D / 2; y[m, k] = y[N-m, D-k] = P - Q, y[N-m, k] = y[m, D-k] = P + Q; four store sites plus the Nyquist
    column; rows in pairs, the pad row of an odd N holding `pad` under a zero twiddle.  mut: the mistake to make."""
    N, Dm = x.shape
    NF = (N + 1) // 2
    xp = np.concatenate([x, np.full((2 * NF - N, Dm), pad)], axis=0)
    n, d, k = np.arange(2 * NF), np.arange(Dm), np.arange(Dm // 2 + 1)
    A = xp @ np.cos(2 * np.pi * np.outer(d, k) / Dm)
    Bm = xp @ np.sin(2 * np.pi * np.outer(d, k) / Dm)
    m = np.arange(N // 2 + 1)
    live = (n < N).astype(np.float64)
    with np.errstate(invalid="ignore"):
        P = (np.cos(2 * np.pi * np.outer(m, n) / N) * live) @ A
        Q = (np.sin(2 * np.pi * np.outer(m, n) / N) * live) @ Bm
    y = np.full((N, Dm), np.nan)
    add = np.zeros((N, Dm)) if add_in is None else add_in

    def store(site, M, K, v):
        y[M, K] = v + (0.0 if mut == ("no add_in", site) else add[M, K])

    for M in m:
        if mut == "m32 dropped" and M == 32:
            continue
        mm = 0 if M == 0 else N - M
        for K in range(Dm // 2):
            mk = 0 if K == 0 else Dm - K
            dd, ss = P[M, K] - Q[M, K], P[M, K] + Q[M, K]
            store(0, M, K, dd)
            if mm != M:
                store(1, mm, K, ss)
            if K != 0:
                store(2, M, mk, dd if mut == "swapped" else ss)
                if mm != M:
                    store(3, mm, mk, ss if mut == "swapped" else dd)
        store(0, M, Dm // 2, P[M, Dm // 2])
        if mm != M and mut != "nyquist mirror":
            store(1, mm, Dm // 2, P[M, Dm // 2])
    return y


def _mix_inputs(c, run="B"):
    rng = C.rng_of(c, run)
    return C.normal(rng, (c.batch, c.tokens, c.dim), c.dtype), C.normal(rng, (c.batch, c.tokens, c.dim), c.dtype)


def test_the_emulation_is_the_reference_when_nothing_is_wrong():
    for c in (C.Mix("fp32", 3, 5, 8), C.Mix("fp32", 3, 6, 64), C.Mix("fp32", 3, 67, 16)):
        x, add = _mix_inputs(c)
        assert R.err(np.stack([emulate_quadrants(x[b], add[b], pad=1e30) for b in range(3)]), R.fnet_mix(x, add), 1) <= 1e-12


MIX_MUTATIONS = ["swapped", "nyquist mirror", ("no add_in", 0), ("no add_in", 1), ("no add_in", 2), ("no add_in", 3), "pad row", "m32 dropped"]


@pytest.mark.parametrize("mut", MIX_MUTATIONS, ids=str)
def test_a_wrong_mixer_kernel_would_exceed_a_bar(mut):
    """P + Q and P - Q swapped in a mirrored quadrant; the Nyquist column's mirror row written once too few; add_in skipped at one of
    the four store sites; the pad row of an odd token count not zeroed (uninitialised LDS: NaN at worst); m = 32 dropped for tokens >= 64"""
    if mut == "m32 dropped":
        cases, barv = [C.Mix("bf16", 1, t, 512) for t in (64, 65)], C.MFMA_BAR
    else:
        cases, barv = [c for c in C.MIX_CASES if c.tokens in (5, 6) and c.dim == 64], None
    assert cases
    hit = 0
    for c in cases:
        x, add = _mix_inputs(c)
        pad = np.nan if mut == "pad row" else 0.0
        wrong = np.stack([emulate_quadrants(x[b], add[b], mut, pad) for b in range(c.batch)])
        e = R.err(wrong, R.fnet_mix(x, add), 1)
        hit += e > 4 * (barv or C.bar(C.TRANSFORM_BAR, c.dtype))
        if mut != "pad row":
            assert e > 4 * (barv or C.bar(C.TRANSFORM_BAR, c.dtype)), (mut, C.case_id(c), e)
    assert hit, mut     # the pad row is live in the odd-token cases only


def test_a_wrong_haar_fwht_or_cls_kernel_would_exceed_a_bar():
    # the adjoint used where the forward is meant in zero mode; the unpaired odd element scaled by 1 instead of 1 / sqrt2
    for c in (c for c in C.HAAR_CASES if c.inverse == 2 and c.levels == 1 and (c.tokens if c.axis == 1 else c.dim) % 2 and c.dim > 1):
        x = C.normal(C.rng_of(c), (c.batch, c.tokens, c.dim), c.dtype)
        ref = _lines(c, R.haar(x, c.axis, c.levels, 2))
        for wrong in (R.haar(x, c.axis, c.levels, 3), R.haar(x, c.axis, c.levels, 0)):
            assert R.err(_lines(c, wrong), ref, 2) > 4 * C.haar_bar(c), C.case_id(c)
    # fwht: "mode 1 stages run in mode 2 order" cannot show, in any kernel: the fwht_fast matrix is symmetric (asserted in
    # test_fwht_reference_equals_the_sylvester_matrix), so mode 2 computes what mode 1 does.  The mistake that does show is a mode 1
    # stage written in mode 0's layout (sum / difference in halves instead of interleaved)
    for c in (c for c in C.FWHT_CASES if c.mode == 1 and c.n_in >= 8):   # (a single input element meets column 0 only: all ones)
        rng = C.rng_of(c)
        x = C.normal(rng, (c.rows, c.n_in), c.dtype)
        res = C.normal(rng, (c.rows, c.n_out), c.dtype) if c.residual else None
        right = R.fwht(x, c.n, c.n_out, 1, c.repeat, 1.0, res)
        assert R.err(R.fwht(x, c.n, c.n_out, 2, c.repeat, 1.0, res), right, 1) <= 1e-12
        assert R.err(R.fwht(x, c.n, c.n_out, 0, c.repeat, 1.0, res), right, 1) > 4 * C.bar(C.TRANSFORM_BAR, c.dtype), C.case_id(c)
    # one row group lost in the cls token sum: every group, at every token count that reaches it
    for c in C.CLS_CASES:
        rng, rg = C.rng_of(c), C.cls_row_groups(c.dtype)
        x = C.normal(rng, (c.batch, c.tokens, c.dim), c.dtype)
        C.normal(rng, (c.batch, c.dim), c.dtype)
        gamma, beta = C.affine(rng, c.dim)
        ref = R.cls_fwd(x, gamma, beta)
        for g in range(min(rg, c.tokens)):
            wrong = R.cls_fwd(x, gamma, beta, lose_group=(g, rg))
            assert R.err(wrong["m0"], ref["m0"], 1) > 4 * C.TRANSFORM_BAR, (C.case_id(c), g)


# ------------------------------------------------------------------------------------------ 5. host refusals
def test_entry_points_refuse_on_the_host_before_any_launch(built):
    """fake pointers that are never followed: every call fails validation, nothing is launched (there is no GPU here), the message
    names the function, and the census does not move"""
    from spectre_vit import _native
    P, Q = 4096, 4096 + 8   # non-null "pointers": 16-byte aligned, and 8 bytes off

    def mix(x=P, y=P, add=0, tw=P, b=3, t=5, d=64, dt=0, ws=P):
        return (x, y, add, tw, b, t, d, dt, ws, 0)

    def lnf(x=P, pre=P, out=P, t=65, d=512, dt=1):
        return (x, pre, out, P, P, P, P, P, 3, t, d, dt, 0)

    def lnb(dout=P, pre=P, dx=P, dg=P, db=P, t=65, d=512, dt=1):
        return (dout, pre, P, P, P, dx, dg, db, P, P, 3, t, d, dt, 0)

    def clsf(x=P, out=P, d=512, dt=1):
        return (x, P, P, out, P, P, P, 3, 5, d, dt, 0)

    def clsb(dx=P, d=512, dt=1):
        return (P, P, P, P, P, dx, P, 3, 5, d, dt, 0)

    def haar(axis=2, levels=1, scr=P):
        return (P, P, 2, 3, 16, axis, levels, 0, 1, scr, 0)

    def hlf(x=P, out=P):
        return (x, P, P, out, P, P, 5, 512, 1, 0)

    def hlb(dout=P, x=P, dx=P):
        return (dout, x, P, P, P, dx, P, P, P, 5, 512, 1, 0)

    def fwht(n_in, n, n_out):
        return (P, P, 0, 3, n_in, n, n_out, 0, 1, 1.0, 0, 0)

    cases = [
        ("spv_fnet_mix", mix(t=4, d=8192), "too large"), ("spv_fnet_mix", mix(t=8193, d=3), "too large"),
        ("spv_fnet_mix", mix(t=7, d=48, ws=0), "workspace"), ("spv_fnet_mix", mix(tw=0), "twiddle"),
        ("spv_fnet_mix", mix(tw=0, t=65, d=512, dt=1), "twiddle"), ("spv_fnet_mix", mix(b=0), "empty"), ("spv_fnet_mix", mix(t=0), "empty"),
        ("spv_fnet_mix", mix(d=0), "empty"), ("spv_fnet_mix", mix(dt=2), "dtype"),
        # 16-byte accesses: the LDS and MFMA paths refuse a misaligned tensor
        ("spv_fnet_mix", mix(x=Q), "aligned"), ("spv_fnet_mix", mix(y=Q), "aligned"), ("spv_fnet_mix", mix(add=Q), "aligned"),
        ("spv_fnet_mix", mix(x=Q, t=65, d=512, dt=1), "aligned"), ("spv_fnet_mix", mix(add=Q, t=65, d=512, dt=1), "aligned"),
        ("spv_fnet_ln_fwd", lnf(x=Q), "aligned"), ("spv_fnet_ln_fwd", lnf(pre=Q), "aligned"), ("spv_fnet_ln_fwd", lnf(out=Q), "aligned"),
        ("spv_fnet_ln_fwd", lnf(t=66), "unsupported"), ("spv_fnet_ln_fwd", lnf(t=1), "unsupported"), ("spv_fnet_ln_fwd", lnf(d=256), "unsupported"),
        ("spv_fnet_ln_fwd", lnf(dt=0), "unsupported"), ("spv_fnet_ln_fwd", lnf(pre=0), "null"),
        ("spv_fnet_ln_bwd", lnb(dout=Q), "aligned"), ("spv_fnet_ln_bwd", lnb(dx=Q), "aligned"), ("spv_fnet_ln_bwd", lnb(pre=Q), "aligned"),
        ("spv_fnet_ln_bwd", lnb(t=66), "unsupported"), ("spv_fnet_ln_bwd", lnb(dg=0), "null"), ("spv_fnet_ln_bwd", lnb(db=0), "null"),
        ("spv_fnet_cls_fwd", clsf(d=128), "unsupported"), ("spv_fnet_cls_fwd", clsf(d=2048), "unsupported"), ("spv_fnet_cls_fwd", clsf(x=Q), "aligned"),
        ("spv_fnet_cls_fwd", clsf(out=Q), "aligned"), ("spv_fnet_cls_bwd", clsb(d=128), "unsupported"), ("spv_fnet_cls_bwd", clsb(d=2048), "unsupported"),
        ("spv_fnet_cls_bwd", clsb(dx=Q), "aligned"),
        ("spv_rfft_real", (P, P, 3, 8193, 0, 0, 0), "too large"), ("spv_rfft_real", (P, P, 0, 16, 0, 0, 0), "empty"),
        ("spv_haar_dwt", haar(levels=0), "levels"), ("spv_haar_dwt", haar(levels=17), "levels"), ("spv_haar_dwt", haar(axis=0), "axis"),
        ("spv_haar_dwt", haar(levels=2, scr=0), "scratch"),
        ("spv_haar_ln_fwd", hlf(x=Q), "aligned"), ("spv_haar_ln_fwd", hlf(out=Q), "aligned"), ("spv_haar_ln_bwd", hlb(dout=Q), "aligned"),
        ("spv_haar_ln_bwd", hlb(x=Q), "aligned"), ("spv_haar_ln_bwd", hlb(dx=Q), "aligned"),
        ("spv_fwht", fwht(12, 12, 12), "power of two"), ("spv_fwht", fwht(8, 32768, 8), "power of two"), ("spv_fwht", fwht(9, 8, 8), "outside"),
    ]
    before = {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()}
    for name, args, needle in cases:
        assert len(args) == len(_native.SIGNATURES[name]), name
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, args, needle, str(e.value))
    assert {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()} == before, "a refused call is not counted"
    # the restated rules name the same refusals
    assert C.mix_path("fp32", 4, 8192)[0] == C.mix_path("fp32", 8193, 3)[0] == C.mix_path("fp32", 7, 48, workspace=False)[0] == "refused"
    assert C.haar_refused(2, 0) and C.haar_refused(0, 1) and C.haar_refused(2, 2, False) and C.fwht_refused(12, 12, 12) and C.fwht_refused(9, 8, 8)
