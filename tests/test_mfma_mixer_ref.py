"""CPU proof of tests/mfma_mixer_ref.py, the element-by-element judge of tests/test_gpu_mfma_mixer_edges.py: the tables reach what they
claim; the two-DFT form and the +-1 factor are the references' own operators; the floors of the float32 restatements on exactly the
GPU inputs set every c (c == ceil(4 floor)); the restatements pass the judge; every named mistake, made in the restatement, fails it
-- a dropped lo part on every fast-path case from 5 tokens on and on every Hadamard case; and the measure the older GPU tests use
(max-abs error over the sample's max-abs reference, tests/spectral_ref.err) lets each dropped lo part through, which is why this
judge exists."""
import math

import numpy as np
import pytest

import edge_judge as J
import gfilter_ref as G
import hadamard_ref as H
import mfma_mixer_ref as M
import spectral_ref as R


def _show(tag, c, worst):
    print(f"MFMA-MIXER {tag} {G.case_id(c)} worst ratio to the bar: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------ 1. tables and operators
def test_tables_reach_what_they_claim():
    assert all(M.path_name(c) == "fast" and c.dtype == "bf16" and not c.off for c in M.FAST_CASES)
    assert {c.tokens for c in M.FAST_CASES} == {1, 2, 3, 4, 5, 16, 17, 32, 33, 48, 49, 63, 64, 65, 80}
    assert {(c.batch, c.dim) for c in M.FAST_CASES if c.batch != 70} == {(b, d) for b in (1, 3) for d in (64, 512)}
    assert G.Case("bf16", 70, 65, 64) in M.FAST_CASES and G.Case("bf16", 70, 65, 64) in G.CASES and G.slabs(70) < 70
    for t in M.FAST_TOKENS:
        assert sum(c.tokens == t for c in M.FAST_CASES) >= 4
    assert all(M.path_name(c) == "generic" for c in M.GENERIC_CASES)
    assert {(c.tokens, c.dim, c.batch) for c in M.GENERIC_CASES} == {(5, 24, 3), (65, 72, 3), (126, 8, 3), (197, 24, 3), (2730, 3, 2)}
    assert all(sum(c[1:] == g[1:] for g in M.GENERIC_CASES) == 2 for c in M.GENERIC_CASES), "fp32 and bf16"
    # the largest token count the selector accepts: launched here, and in gfilter_ref.CASES at the older bars
    big = G.select("fp32", 2730, 3)
    assert G.MAX_TOKENS == 2730 and big == G.select("bf16", 2730, 3) and (big.path, big.cols_fwd, big.cols_bwd) == (G.GENERIC, 2, 1)
    assert big.cols_fwd * (2730 + 2 * big.bins) + 2 * 2730 == big.cols_bwd * (2 * 2730 + 4 * big.bins) + 2 * 2730 == G.LDS_FLOATS == 65536 // 4
    assert all(G.Case(dt, 2, 2730, 3) in G.CASES for dt in G.DTYPES)
    assert M.HADAMARD_CASES == H.LN_CASES and {c.tokens for c in H.LN_CASES} == {2, 3, 16, 17, 32, 33, 64, 65}
    assert {c.batch for c in H.LN_CASES} == {1, 3} and H.LN_MODES == ("fold", "defer")
    # a few hundred KB at most per tensor
    assert max(c.batch * c.tokens * c.dim * (2 if c.dtype == "bf16" else 4) for c in M.FILTER_CASES) <= 600 * 1024
    assert set(M.C_BAR) == {f"{p}_{k}" for p in ("fast", "generic") for k in ("y", "dx", "dw")} | {"had_" + k for k in M.HADAMARD_ELEMENTWISE}


def _planted(a, dtype):
    flat = np.asarray(a).reshape(-1)
    return (bool(((flat == 0) & ~np.signbit(flat)).any()) and bool(((flat == 0) & np.signbit(flat)).any())
            and bool((np.abs(flat) == J.TINY[dtype]).any()) and bool(np.isfinite(flat).all()))


def test_inputs_are_planted_and_seeded():
    for c in M.FILTER_CASES:
        x, dy, w = M.filter_inputs(c)
        x2, dy2, w2 = M.filter_inputs(c)
        assert np.array_equal(x, x2) and np.array_equal(dy, dy2) and np.array_equal(w, w2)
        assert np.array_equal(J.cast(x, c.dtype), x) and np.array_equal(J.cast(dy, c.dtype), dy) and not x.flags.writeable
        for a in (x, dy):
            assert bool((~a.any(1)).any()), "one column of one sample is all zeros"
            if a.size >= 64:
                assert _planted(a, c.dtype), c
        assert (w[G.inert(c.tokens), :, 1] != 0).all(), "the inert imaginary parts are planted non-zero"
    for c in M.HADAMARD_CASES:
        d = M.hadamard_inputs(c)
        assert _planted(d["x"], "bf16") and _planted(d["dout"], "bf16") and np.array_equal(d["x"], M.hadamard_inputs(c)["x"])


@pytest.mark.parametrize("tokens", (1, 2, 3, 4, 5, 8, 12, 17, 64, 65, 80, 126))
def test_two_dft_form_is_the_fft_reference_and_its_tables_are_exact_at_quarter_turns(tokens):
    rng = np.random.default_rng(tokens)
    x, dy, w = rng.standard_normal((3, tokens, 5)), rng.standard_normal((3, tokens, 5)), rng.standard_normal((G.bins(tokens), 5, 2))
    got = M.filter_dft(x, dy, w)
    assert R.err(got["y"], G.fwd(x, w), 1) <= 1e-12 and R.err(got["dx"], G.dx(dy, w), 1) <= 1e-12 and R.err(got["dw"], G.dw(x, dy)) <= 1e-12
    fc, fs = M.trig(tokens)
    a = 2.0 * np.pi * np.arange(G.bins(tokens))[:, None] * np.arange(tokens)[None, :] / tokens
    assert np.abs(fc - np.cos(a)).max() <= 1e-12 and np.abs(fs - np.sin(a)).max() <= 1e-12
    assert not fs[G.inert(tokens)].any() and set(np.unique(np.abs(fc[G.inert(tokens)]))) == {1.0}
    # S bounds the value it belongs to, and is 0 exactly where nothing arrives
    ref = M.filter_reference(x, dy, w)
    for k in ("y", "dx", "dw"):
        assert (np.abs(ref[k]) <= ref["S_" + k] * (1 + 1e-12)).all()
    assert not ref["S_dw"][G.inert(tokens), :, 1].any() and (ref["S_dw"][..., 0] > 0).all()


def test_the_factor_is_the_references_token_transform():
    for N in (2, 3, 16, 17, 33, 65):
        a = M._factor(N, True)
        x = np.random.default_rng(N).standard_normal((1, N, 8))
        want = H.mix(x, normalize=False)
        got = M.O.fwht(np.matmul(a.astype(np.float64)[:N, :N], x), normalize=False)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert not a[N:].any() and not a[:, N:].any() and set(np.unique(a[:N, :N])) == {-1.0, 1.0}
        assert M._factor(N, False).all()


def test_restatement_without_a_mistake_is_gfilter_refs():
    for c in (G.Case("bf16", 3, 65, 64), G.Case("bf16", 3, 2, 64), G.Case("bf16", 3, 65, 72), G.Case("fp32", 3, 5, 24)):
        x, dy, w = M.filter_inputs(c)
        got = M.filter_restate(c, x, dy, w)
        if M.path_name(c) == "fast":
            y, (dx, dw) = G.fast_fwd32(x, w), G.fast_bwd32(x, dy, w)
        else:
            y, (dx, dw) = G.generic_fwd32(x, w), G.generic_bwd32(x, dy, w)
        assert np.array_equal(got["y"], y) and np.array_equal(got["dx"], dx) and np.array_equal(got["dw"], dw)


# ------------------------------------------------------------------------------------------------------------------ 2. floors and bars
def _filter_floors(c, inputs):
    x, dy, w = inputs(c)
    ref, pre = M.filter_reference(x, dy, w), M.filter_restate(c, x, dy, w)
    return {k: M.floor_units(pre[k], ref, k) for k in ("y", "dx", "dw")}


def _hadamard_floors(c, planted):
    data = M.hadamard_inputs(c, planted)
    got = M.hadamard_restate(data)
    ref = M.hadamard_reference(data, got)
    pre = dict(prenorm="prenorm32", dx="dx32")
    return {k: M.floor_units(got[pre.get(k, k)], ref, k) for k in M.HADAMARD_ELEMENTWISE}


def test_floors_set_the_bars():
    """the restatements before their stores against float64 on exactly the GPU inputs -- the planted inputs of the edge file, and the
    seeded normals of tests/test_gpu_gfilter_mixer.py and tests/test_gpu_hadamard_mixer.py at the batch their CPU files restate:
    c == ceil(4 floor), per quantity and path"""
    fl = dict.fromkeys(M.C_BAR, 0.0)
    runs = [(c, M.filter_inputs, "edges") for c in M.FILTER_CASES] + [(c, G.inputs, "older") for c in G.CASES if c.batch != 1]
    for c, inputs, tag in runs:
        f = _filter_floors(c, inputs)
        if tag == "edges":
            print(f"MFMA-MIXER-FLOOR {M.path_name(c)} {G.case_id(c)} " + " ".join(f"{k}={v:.2f}" for k, v in f.items()))
        for k, v in f.items():
            fl[f"{M.path_name(c)}_{k}"] = max(fl[f"{M.path_name(c)}_{k}"], v)
    for c in M.HADAMARD_CASES:
        for planted in (True, False):
            f = _hadamard_floors(c, planted)
            print(f"MFMA-MIXER-FLOOR hadamard {H.case_id(c)} {'edges' if planted else 'older'} " + " ".join(f"{k}={v:.2f}" for k, v in f.items()))
            for k, v in f.items():
                fl["had_" + k] = max(fl["had_" + k], v)
    for name, f in fl.items():
        print(f"MFMA-MIXER-FLOOR {name} floor = {f:.3f}  c = {M.C_BAR[name]}  floor <= c / 4: {f <= M.C_BAR[name] / 4}")
    for name, f in fl.items():
        assert f <= M.C_BAR[name] / 4, (name, f)
        assert M.C_BAR[name] == math.ceil(4 * f), (name, f)      # four times the floor, rounded up: not a looser one


@pytest.mark.parametrize("case", M.FILTER_CASES, ids=G.case_id)
def test_filter_restatement_passes_the_judge(case):
    x, dy, w = M.filter_inputs(case)
    ref = M.filter_reference(x, dy, w)
    ok, worst = M.filter_verdict(case, ref, M.filter_store(case, M.filter_restate(case, x, dy, w)))
    _show(M.path_name(case), case, worst)
    assert ok, worst
    # the zeroed columns come back as zeros
    got = M.filter_store(case, M.filter_restate(case, x, dy, w))
    assert not got["y"][~x.any(1)[:, None, :].repeat(case.tokens, 1)].any() and not got["dx"][~dy.any(1)[:, None, :].repeat(case.tokens, 1)].any()


@pytest.mark.parametrize("case", M.HADAMARD_CASES, ids=H.case_id)
def test_hadamard_restatement_passes_the_judge(case):
    data = M.hadamard_inputs(case)
    ok, worst = M.hadamard_verdict(data, M.hadamard_restate(data))
    _show("hadamard", case, worst)
    assert ok, worst


# ------------------------------------------------------------------------------------------------------------------ 3. mistakes fail
def _filter_mistakes():
    """{mistake: {case: ok}} over every table case but the 2730-token pair (seconds each, and no mistake needs it)"""
    seen = {m: {} for m in M.FILTER_MISTAKES}
    for c in (c for c in M.FILTER_CASES if c.tokens <= 197):
        x, dy, w = M.filter_inputs(c)
        ref = M.filter_reference(x, dy, w)
        for m in M.FILTER_MISTAKES:
            if m in M.FAST_LO_MISTAKES + ("sine_cross_term",) and M.path_name(c) != "fast":
                continue
            ok, worst = M.filter_verdict(c, ref, M.filter_store(c, M.filter_restate(c, x, dy, w, m)))
            seen[m][c] = (ok, worst)
    return seen


def test_every_filter_mistake_fails_the_judge():
    seen = _filter_mistakes()
    for m, cases in seen.items():
        failed = [c for c, (ok, _) in cases.items() if not ok]
        worst = max(max(w.values()) for _, w in cases.values())
        print(f"MFMA-MIXER-MISTAKE filter {m}: fails {len(failed)} of {len(cases)} cases, worst ratio {worst:.1f}")
        assert failed, m
        if m in M.FAST_LO_MISTAKES:
            passed = [c for c, (ok, _) in cases.items() if ok and c.tokens >= 5]
            assert not passed, (m, passed)
            low = min(max(w.values()) for c, (_, w) in cases.items() if c.tokens >= 5)
            print(f"MFMA-MIXER-MISTAKE filter {m}: the least worst ratio over the cases from 5 tokens on {low:.1f}")


def test_every_hadamard_mistake_fails_the_judge():
    for m in M.HADAMARD_MISTAKES:
        res = {}
        for c in M.HADAMARD_CASES:
            data = M.hadamard_inputs(c)
            res[c] = M.hadamard_verdict(data, M.hadamard_restate(data, m))
        failed = [c for c, (ok, _) in res.items() if not ok]
        print(f"MFMA-MIXER-MISTAKE hadamard {m}: fails {len(failed)} of {len(res)} cases; ratios "
              + " ".join(f"{H.case_id(c)}:{max(w.values()):.1f}" for c, (_, w) in res.items()))
        assert failed, m
        if m in M.HADAMARD_LO_MISTAKES:
            assert len(failed) == len(res), (m, [c for c in res if c not in failed])
    # rows N .. of a K step exist only where N is no multiple of 16
    data = M.hadamard_inputs(H.Ln(3, 32))
    assert M.hadamard_verdict(data, M.hadamard_restate(data, "pad_rows_live"))[0]


# ------------------------------------------------------------------------------------------------------------------ 4. the gap
def test_the_per_sample_measure_lets_every_dropped_lo_part_through():
    """what tests/test_gpu_gfilter_mixer.py and tests/test_gpu_hadamard_mixer.py assert of these outputs -- max-abs error over the
    sample's max-abs reference within 2e-5 / 6e-5 + 2^-8 -- holds with a lo part dropped, on at least one case each (in fact nearly
    all): 2^-8 of the largest of some 33 000 elements is about ten times what the missing part does.  The per-sample measure is that
    of the bf16 outputs y, dx and the Hadamard dx.  dW, a float32 output held to 6e-5 of the tensor's maximum, is printed beside them:
    the lo plane of T1 feeds it too, and there the older test does see it in the backward kernel -- not in the forward kernel, whose
    only output is y."""
    for m in M.FAST_LO_MISTAKES:
        through = []
        for c in (G.Case("bf16", 3, 80, 64), G.Case("bf16", 3, 65, 512), G.Case("bf16", 3, 33, 64), G.Case("bf16", 3, 5, 64)):
            x, dy, w = G.inputs(c)       # the older test's own inputs
            got = M.filter_store(c, M.filter_restate(c, x, dy, w, m))
            errs = dict(y=R.err(got["y"], G.fwd(x, w), 1), dx=R.err(got["dx"], G.dx(dy, w), 1), dw=R.err(got["dw"], G.dw(x, dy)))
            old = errs["y"] <= G.bar(G.TRANSFORM_BAR, "bf16") and errs["dx"] <= G.bar(G.GRAD_BAR, "bf16")
            ref = M.filter_reference(x, dy, w)
            new, worst = M.filter_verdict(c, ref, got)
            print(f"MFMA-MIXER-GAP filter {m} {G.case_id(c)}: old measure y={errs['y']:.3e} dx={errs['dx']:.3e} dw={errs['dw']:.3e} "
                  f"({'passes' if old else 'fails'}); new judge worst ratio {max(worst.values()):.1f}")
            assert not new
            through += [c] if old else []
        assert through, m
    for m in M.HADAMARD_LO_MISTAKES:
        through = []
        for c in (H.Ln(3, 65), H.Ln(1, 16), H.Ln(3, 2)):
            data = M.hadamard_inputs(c, planted=False)    # the older test's own inputs
            got = M.hadamard_restate(data, m)
            e = R.err(got["dx"], H.ln_bwd(data["dout"], got["prenorm"], data["gamma"])["dx"], 1)
            new, worst = M.hadamard_verdict(data, got)
            print(f"MFMA-MIXER-GAP hadamard {m} {H.case_id(c)}: old measure dx={e:.3e} (bar {H.bar(H.GRAD_BAR, 'bf16'):.3e}); "
                  f"new judge worst ratio {max(worst.values()):.1f}")
            assert not new
            through += [c] if e <= H.bar(H.GRAD_BAR, "bf16") else []
        assert through, m
