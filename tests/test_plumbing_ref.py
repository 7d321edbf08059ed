"""CPU checks behind tests/test_gpu_plumbing_edges.py: the case tables of tests/plumbing_edge_cases.py reach every branch the restated
dispatch of csrc/spv_misc.hip has; the float32 / bf16-storage restatement of every kernel (tests/plumbing_ref.py) passes the GPU
test's own judging function on every case; each plausible mistake made in that restatement fails it on at least one case; the floors
behind the bars are measured here, on the reference side alone, and stay within a quarter of each bar; ids are unique and no case
needs more than 80 MB of device buffers."""
import numpy as np
import pytest

import plumbing_edge_cases as C
import plumbing_ref as R


# ------------------------------------------------------------------------------------------------------------------ 1. branches
def test_tables_reach_every_branch():
    # the second trip of every capped grid-stride loop, and the single trip
    assert {C.ew_trips(C.cdiv(c.n, 4)) for c in C.CAST_CASES} == {1, 2}
    assert {C.ew_trips(c.n) for c in C.GELU_CASES} == {1, 2} and {C.ew_trips(c.n) for c in C.AXPBY_CASES} == {1, 2}
    assert all(c.n % 2 for c in C.GELU_CASES)
    assert {c.n % 4 for c in C.CAST_CASES} == {0, 1, 2, 3} and {(c.src, c.dst) for c in C.CAST_CASES} == set(C.PAIRS)
    # cast_transpose: every dtype pair with every ld form, a whole tile row of padding, both grouped row maps
    forms = {(c.src, c.dst, "rows" if c.ld == c.rows else "round8" if c.ld == C.round8(c.rows) else "pad") for c in C.CT_CASES if not c.rg}
    assert {f[:2] for f in forms} == set(C.PAIRS) and {f[2] for f in forms} == {"rows", "round8", "pad"}
    assert any(C.cdiv(c.ld, 64) > C.cdiv(c.rows, 64) for c in C.CT_CASES)
    assert {(c.rg, c.gs, c.roff) for c in C.CT_CASES if c.rg} == {(4, 5, 1), (3, 7, 2)}
    assert {v for c in C.CT_CASES for v in (c.rows, c.cols)} >= {1, 63, 64, 65, 130}
    assert all(c.ld < c.rows for c in C.CT_REFUSED)
    # weight shadows: vector / scalar loads, vector / scalar stores, tile rows wholly past `rows`, plain given and NULL -- per dtype
    for dt in C.DTYPES:
        paths = {C.shadow_paths(c.rows, c.cols, c.ld) for c in C.WS_CASES if c.dtype == dt}
        assert {p[0] for p in paths} == {p[1] for p in paths} == {p[2] for p in paths} == {True, False}
        assert {c.plain for c in C.WS_CASES if c.dtype == dt} == {0, 1}
    assert {(c.rows, c.cols) for c in C.WS_CASES} == set(C.WS_SHAPES)
    assert all(len(m) == 3 and {c.plain for c in m} == {0, 1} for m in C.WS_MULTI)
    # column sums: every value of vec, tx_log2 and gx, and parts 1, in between and at its cap
    plans = [C.colsum_plan(c.rows, c.n, c.off == 0) for c in C.COLSUM_CASES]
    assert {p["vec"] for p in plans} == {1, 4} and {p["tx_log2"] for p in plans} == {5, 6, 7, 8} and {p["gx"] for p in plans} == {1, 2}
    assert {min(max(p["parts"], 1), 2) if p["parts"] < 512 else 512 for p in plans} == {1, 2, 512}
    assert any(p["vec"] == 1 and p["gx"] == 2 for p in plans) and any(p["vec"] == 4 and p["gx"] == 2 for p in plans)
    assert any(c.off and c.n % 4 == 0 for c in C.COLSUM_CASES)
    assert all(p["parts"] <= min(c.rows, 512) for p, c in zip(plans, C.COLSUM_CASES))      # the partials buffer of include/spv.h holds them


def test_ids_unique_and_buffers_small():
    for family, cases in C.ALL.items():
        ids = [C.case_id(c) for c in cases]
        assert len(set(ids)) == len(ids), family
        for c in cases:
            assert C.device_bytes(family, c) <= C.LIMIT_BYTES, (family, c)


# ------------------------------------------------------------------------------------------------------------------ 2. restatements pass
@pytest.mark.parametrize("family", list(C.ALL))
def test_restatement_passes_the_judge(family):
    for c in C.ALL[family]:
        ok, worst = C.verdict(C.expect(family, c), C.restate(family, c))
        print(f"PLUMBING-REF {family} {C.case_id(c)} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
        assert ok, (family, c, worst)


def test_floors_stay_within_a_quarter_of_the_bars():
    """the float32 restatement, before any storage rounding, against float64 on the GPU cases' inputs"""
    floors = dict.fromkeys(C.C_BAR, 0.0)
    for c in C.GELU_CASES:
        d = C.inputs("gelu", c)
        (y, sy), (dx, sdx) = R.gelu_fwd_ref(d["x"]), R.gelu_bwd_ref(d["dy"], d["x"])
        floors["gelu_fwd"] = max(floors["gelu_fwd"], C.floor_ratio(R.gelu_fwd_restate(d["x"], "fp32"), y, sy))
        floors["gelu_bwd"] = max(floors["gelu_bwd"], C.floor_ratio(R.gelu_bwd_restate(d["dy"], d["x"], "fp32"), dx, sdx))
    for c in C.AXPBY_CASES:
        d = C.inputs("axpby", c)
        out, S = R.axpby_ref(d["x"], d["y"], c.a, c.b)
        floors["axpby"] = max(floors["axpby"], C.floor_ratio(R.axpby_restate(d["x"], d["y"], c.a, c.b, "fp32"), out, S))
    for c in C.COLSUM_CASES:
        out, S = R.colsum_ref(C.inputs("colsum", c)["x"])
        floors["colsum"] = max(floors["colsum"], C.floor_ratio(C.restate("colsum", c)["out"], out, S))
    for name, f in floors.items():
        print(f"PLUMBING-FLOOR {name} floor = {f:.3f}  c = {C.C_BAR[name]}")
        assert f <= C.C_BAR[name] / 4, (name, f)
        assert C.C_BAR[name] < 4 * f + 2, (name, f)      # the bar is the measured floor's, not a looser one


# ------------------------------------------------------------------------------------------------------------------ 3. mistakes fail
MISTAKES = [("cast", "truncate"), ("cast_transpose", "truncate"), ("cast_transpose", "no_roff"), ("shadows", "pad_rows_unwritten"),
            ("gelu", "tanh"), ("colsum", "last_slab")]


@pytest.mark.parametrize("family,mutant", MISTAKES, ids=[f"{f}-{m}" for f, m in MISTAKES])
def test_a_plausible_mistake_fails_the_judge(family, mutant):
    failed = [c for c in C.ALL[family] if not C.verdict(C.expect(family, c), C.restate(family, c, mutant))[0]]
    print(f"PLUMBING-MUTANT {family} {mutant}: fails {len(failed)} of {len(C.ALL[family])} cases")
    assert failed


def test_tanh_gelu_is_orders_of_magnitude_over_the_bar():
    c = C.GELU_CASES[0]
    d = C.inputs("gelu", c)
    y, sy = R.gelu_fwd_ref(d["x"])
    assert C.floor_ratio(R.gelu_fwd_restate(d["x"], "fp32", "tanh"), y, sy) > 100 * C.C_BAR["gelu_fwd"]


# ------------------------------------------------------------------------------------------------------------------ the references
def test_references_agree_with_plain_numpy():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((12, 7))
    assert np.array_equal(R.cast(x, "fp32"), x.astype(np.float32).astype(np.float64))
    b = R.cast(x, "bf16")
    assert np.array_equal(b.astype(np.float32).view(np.uint32) & 0xFFFF, np.zeros_like(b, np.uint32)) and (np.abs(b - x) <= np.abs(x) * 2.0 ** -8).all()
    assert np.isposinf(R.cast(np.float64(np.finfo(np.float32).max), "bf16")) and R.cast(1.0 + 2.0 ** -8, "bf16") == 1.0      # ties to even
    assert R.cast(1.0 + 3 * 2.0 ** -8, "bf16") == 1.0 + 2.0 ** -6
    t = R.cast_transpose_ref(x, "fp32", 12, 7, 16, 0, 0, 0)
    assert np.array_equal(t[:, :12], R.cast(x, "fp32").T) and not t[:, 12:].any() and not np.signbit(t[:, 12:]).any()
    g = R.cast_transpose_ref(x, "fp32", 6, 7, 6, 2, 4, 1)
    assert np.array_equal(g, R.cast(x[[1, 2, 5, 6, 9, 10]], "fp32").T)
    assert np.array_equal(C.expect("colsum", C.COLSUM_CASES[2])["out"].ref, C.inputs("colsum", C.COLSUM_CASES[2])["x"].sum(0))
    y, _ = R.gelu_fwd_ref(np.array([0.0, 1.0, -1.0]))
    assert np.allclose(y, [0.0, 0.8413447460685429, -0.15865525393145707], rtol=1e-15, atol=0)
