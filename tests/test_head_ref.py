"""CPU checks behind tests/test_gpu_head_edges.py: the case tables of tests/head_edge_cases.py reach every branch the restated dispatch
of csrc/spv_head.hip, the loss half of csrc/spv_distill.hip and csrc/spv_infer.hip has; the float32 restatement of every kernel
(tests/head_ref.py) passes the GPU test's own judging function on every case; each plausible mistake made in that restatement fails
it on at least one case; the floors behind the bars are measured here, on the reference side alone, and stay within a quarter of each
bar; ids are unique and no case needs more than 80 MB of device buffers."""
import math

import numpy as np
import pytest

import eval_ref as E
import head_edge_cases as C
import head_ref as R
from tail_ref import col_error, row_errors


def f64(d):
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


def show(tag, c, worst):
    print(f"HEAD-REF {tag} {C.case_id(c)} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------ 1. branches
def test_head_tables_reach_every_branch():
    cases = C.HEAD_CASES
    assert {c.k for c in cases} == {1, 2, 7, 63, 64, 65, 100, 128, 512, 513, 600, 768, 769, 1023, 1024}
    assert {c.n for c in cases} == {1, 2, 7, 63, 64, 65, 100, 127, 128} and all(c.n <= c.k for c in cases)
    assert {c.n for c in cases if c.n == c.k} == {1, 2, 7, 64, 65, 100, 128}
    assert {c.rows for c in cases} == {1, 3, 4, 5, 523, 4096} and [(c.n, c.k) for c in cases if c.rows == 4096] == [(2, 2)] * 2
    for dt in C.DTYPES:
        mine = [c for c in cases if c.dtype == dt]
        assert {c.pad for c in mine} == {0, 5} and {c.xb for c in mine} == {"null", "ldb"} and {c.fused for c in mine} == {0, 1}
        assert {(c.rows, c.n, c.k) for c in mine} == {s[:3] for s in C._HEAD_SHAPES}
        plans = [C.head_fwd_plan(c.n, c.k, c.xb) for c in mine]
        assert {p["kj"] for p in plans} == {8, 12, 16} and {p["second"] for p in plans} == {"none", "part", "full"}
        for kj in (8, 12, 16):      # each instantiation with and without slots past k, i.e. at its first size and at its last
            assert {p["clamped"] for p in plans if p["kj"] == kj} == {True, False}
        assert {p["same"] for p in plans} == {p["bsc"] for p in plans} == {True, False} and {p["trips"] for p in plans} >= {1, 2}
        assert any(c.k < 64 for c in mine) and any(c.k > 64 and c.k % 64 for c in mine)
        rp = [C.head_bwd_rows_plan(c.n, c.k) for c in mine]
        assert {p["nq"] for p in rp} >= {1, 2, 8, 10, 16, 512, 1024} and any(p["idle"] == 24 for p in rp) and any(p["idle"] == 424 for p in rp)
        assert {p["ragged"] for p in rp} == {True, False}
        wp = [C.head_bwd_w_plan(c.rows, c.n, c.k) for c in mine]
        assert {p["fold_rounds"] for p in wp} == {1, 2, 8} and {p["row_rounds"] for p in wp} == {1, 5, 32} and {p["odd_n"] for p in wp} == {True, False}
        assert any(p["nparts"] == 131 for p in wp)
    assert all(C.head_supported(c.rows, c.n, c.k) for c in cases)
    for c in [c for c in cases if c.n == 2]:        # LayerNorm over two values on both sides of its 1e-5: variance below and above it
        var = 1.0 / C.expect("head_fwd", c)["rstd"].ref ** 2 - 1e-5
        assert var.min() < 1e-6 and var.max() > 2e-5 and (c.rows < 4096 or (var > 1e-5).mean() > 0.2), c
    for r in C.HEAD_REFUSED:
        assert (not C.head_supported(r.rows, r.n, r.k)) == (r.why in ("n>k", "k=1025", "n=129", "rows=4097")), r
    assert {r.why for r in C.HEAD_REFUSED} == {"n>k", "k=1025", "n=129", "rows=4097", "lda<k", "dtype"}
    assert C.head_bwd_w_plan(*C.BWDW_CASES[0])["fold_rounds"] == 2


def test_loss_tables_reach_every_branch():
    ce = C.CE_CASES
    assert {c.rows for c in ce} == {1, 15, 16, 17, 1024, 1025} and {c.classes for c in ce} >= {1, 2, 63, 64, 65, 129, 1000}
    assert {C.sweeps(c.rows, R.CE_WAVES, R.CE_MAX_WG) for c in ce} == {1, 2} and {c.go for c in ce} == {1.0, 0.75}
    assert {C.ew_sweeps(c.rows * c.classes, 1024) for c in ce} == {1, 2} and C.CE_BIG[0] * C.CE_BIG[1] > R.CE_BWD_SWEEP
    assert {c.kind for c in ce} == {"plain", "edges", "label_-1", "label_C"}
    dl = C.DL_CASES
    assert {c.rows for c in dl} == {1, 4, 5, 256, 257} and {c.classes for c in dl} >= {1, 2, 63, 64, 65, 1000}
    assert {c.cfg for c in dl} == {0, 1, 2} and C.CFGS == ((2.0, 0.25, 0.75), (1.0, 1.0, 0.0), (4.0, 0.0, 1.0))
    assert {C.sweeps(c.rows, R.DL_WAVES, R.DL_MAX_WG) for c in dl} == {1, 2}
    assert {C.ew_sweeps(c.rows * c.classes, 256) for c in dl} == {1, 2} and C.DL_BIG[0] * C.DL_BIG[1] > R.DL_BWD_SWEEP
    assert {c.kind for c in dl} == {"same", "far", "near1e-3", "near0.49", "near0.51", "plain", "level", "underflow"}
    for c in dl:        # the rule itself, on the inputs: both forms are taken, and the named cases sit on the side they name
        d = C.distill_inputs(c)
        near = R.nearby_rows(d["z"], d["t"], C.CFGS[c.cfg][0])
        if c.kind in ("same", "near1e-3", "near0.49"):
            assert near.all(), c
        if c.kind in ("near0.51", "far", "level"):
            assert not near.any(), c
        if c.kind in C.NEAR:
            assert math.isclose(float((np.abs(d["t"] - d["z"]) / C.CFGS[c.cfg][0]).max()), C.NEAR[c.kind], rel_tol=0.03), c
    assert any(c.rows == 1 and c.kind == k for c in dl for k in C.NEAR)
    idx = [c for c in dl if c.n_cache]
    assert {c.n_cache for c in idx} >= {1, 2048} and any(c.n_cache == c.rows + 1 for c in idx)
    assert any(len(set(C.distill_inputs(c)["index"])) < c.rows for c in idx) and any(np.any(np.diff(C.distill_inputs(c)["index"]) < 0) for c in idx)
    p = C.distill_inputs(C.DL_POISON)
    assert (p["index"] == C.DL_POISON.n_cache).sum() == 1 and np.isnan(p["cache"]).any(1).sum() == 1 and np.isnan(p["t"]).any(1).sum() == 2


def test_eval_tables_reach_every_branch():
    ev = C.EVAL_CASES
    assert {c.classes for c in ev} == {1, 2, 63, 64, 65, 128, 129, 512, 513} and {c.rows for c in ev} == {1, 7, 8, 9, 512, 513}
    for dt in C.DTYPES:
        mine = [c for c in ev if c.dtype == dt]
        assert {(C.eval_kj(c.classes), c.classes) for c in mine} >= {(2, 128), (8, 129), (8, 512), (0, 513)}
        assert {C.sweeps(c.rows, R.EW, R.E_MAX_WG) for c in mine} == {1, 2} and {c.k for c in mine} == {1, 5, 8}
        assert {c.kind for c in mine} == {"plain", "ties", "nan", "labels"} and any(c.k > c.classes for c in mine)
        assert {C.eval_kj(c.classes) for c in mine if c.kind == "ties"} == {2, 8, 0} and {c.k for c in mine if c.kind == "ties"} == {1, 5, 8}
        assert {c.nv for c in mine} == {"rows", "rows-1", "zero", "neg", "rows+5"}
    assert {C.n_valid_of(c) - c.rows for c in ev if c.nv in ("rows", "rows-1", "rows+5")} == {0, -1, 5}
    for c in [c for c in ev if c.kind == "ties"]:       # the planted ties are there, in storage values, and the first of each pair wins
        d = C.eval_inputs(c)
        z, pred = d["z"], R.eval_ref(d["z"], d["labels"], d["n_valid"], c.k)[0]
        pairs = C.tie_pairs(c.classes)
        assert len(pairs) >= 3
        for r, (a, b) in enumerate(pairs):
            assert z[r, a] == z[r, b] == z[r].max() and pred[r] == a, (c, r)
        # the label's own ties decide the hit: k - 1 entries strictly above, one column tied, and each other way of counting ties
        # changes the number of hits
        r = len(pairs)
        for row, (y, other, hit) in enumerate(C.TIE_LABELS, r):
            assert d["labels"][row] == y and z[row, y] == z[row, other] and int((z[row] > z[row, y]).sum()) == c.k - 1
            assert int((z[row] == z[row, y]).sum()) == 2 and E.topk_hit(z[row], y, c.k) == hit and (other < y) != hit
        r += len(C.TIE_LABELS) - 2
        right = R.eval_restate(d["z"], d["labels"], d["n_valid"], c.k)[1]["topk"]
        for mutant in ("tie_ignored", "tie_gt", "tie_all"):
            assert R.eval_restate(d["z"], d["labels"], d["n_valid"], c.k, mutant)[1]["topk"] != right, (c, mutant)
        if c.dtype == "bf16":
            assert z[r + 2, 10] == z[r + 2, 100] == z[r + 2].max() and pred[r + 2] == 10
    for c in [c for c in ev if c.kind == "nan"]:
        d = C.eval_inputs(c)
        pred = R.eval_ref(d["z"], d["labels"], d["n_valid"], c.k)[0]
        assert np.isnan(d["z"][1]).all() and pred[1] == 0 and np.isnan(d["z"][0]).sum() == 2 and not np.isnan(d["z"][0, pred[0]])


def test_ids_unique_and_buffers_small():
    for family, cases in C.ALL.items():
        ids = [C.case_id(c) for c in cases]
        assert len(set(ids)) == len(ids), family
        for c in cases + ([C.DL_POISON] if family == "distill" else []):
            assert C.device_bytes(family, c) <= C.LIMIT_BYTES, (family, c)


# ------------------------------------------------------------------------------------------------------------------ 2. restatements pass
def head_verdict(c, mutant=None):
    fwd, bwd = C.restate_head(c, mutant)
    ok1, w1 = C.verdict(C.expect("head_fwd", c), fwd)
    good = C.restate_head(c)[0] if mutant else fwd        # the backward is judged on a forward that is right
    ok2, w2 = C.verdict(C.expect("head_bwd", c, good, bwd["dh"]), bwd) if not mutant or mutant.startswith("no_i0") else (True, {})
    return ok1 and ok2, {**w1, **w2}


def loss_verdict(family, c, mutant=None):
    if family == "ce":
        return C.verdict(C.expect("ce", c), f64(C.restate_ce(c, mutant)))
    if family == "distill":
        return C.verdict(C.expect("distill", c), f64(C.restate_distill(c, mutant)))
    return C.verdict(C.expect("eval", c), C.restate_eval(c, mutant))


@pytest.mark.parametrize("case", C.HEAD_CASES, ids=C.case_id)
def test_head_restatement_passes_the_judge(case):
    ok, worst = head_verdict(case)
    show("head", case, worst)
    assert ok, (case, worst)


@pytest.mark.parametrize("family", ["ce", "distill", "eval"])
def test_loss_restatement_passes_the_judge(family):
    for c in C.ALL[family] + ([C.DL_POISON] if family == "distill" else []):
        ok, worst = loss_verdict(family, c)
        show(family, c, worst)
        assert ok, (family, c, worst)
    if family == "eval":
        for c in C.EVAL_ACCUMULATE:
            ok, worst = C.verdict(C.expect("eval", c, 3), C.restate_eval(c, None, 3))
            assert ok, (c, worst)


def test_bwd_w_alone_passes_the_judge():
    c = C.BWDW_CASES[0]
    d = C.bwdw_inputs(c)
    z = np.zeros((c.rows, c.n))
    got = R.head_bwd_restate(z, z, d["xs"], z[:, 0], z[:, 0], np.zeros((c.n, c.k)), z[0], z[0], partials=d["partials"], dh_in=d["dh"])
    ok, worst = C.verdict(C.expect("bwd_w", c), f64({k: got[k] for k in ("dW", "dgamma", "dbeta", "dbias")}))
    show("bwd_w", c, worst)
    assert ok, worst


def test_floors_stay_within_a_quarter_of_the_bars():
    """the float32 restatement, before any storage rounding, against float64 on the GPU cases' inputs"""
    fl = dict.fromkeys(C.C_BAR, 0.0)
    ln = dict(out=0.0, mean=0.0, rstd=0.0, dh=0.0, dx_rows=0.0)

    def up(name, got, ref, S):
        S = np.where(np.asarray(S) * C.EPS > 0, S, 0.0)        # a probability so small that 2^-24 S is no float64: exact there (dz: flushed to 0 within its allowance)
        fl[name] = max(fl[name], C.floor_ratio(got, ref, S))

    for c in C.HEAD_CASES:
        d = C.head_inputs(c)
        xa, xb = C.head_x(c)
        fwd = f64(R.head_fwd_restate(xa, xb, d["W"], d["bias"], d["gamma"], d["beta"]))
        ref = R.head_fwd_ref(fwd["xs"], d["W"], d["bias"], d["gamma"], d["beta"])
        up("head_h", fwd["h"], ref["h"], ref["S_h"])
        ln["out"] = max(ln["out"], float(row_errors(fwd["out"], ref["out"]).max()))
        ln["mean"], ln["rstd"] = max(ln["mean"], col_error(fwd["mean"], ref["mean"])), max(ln["rstd"], col_error(fwd["rstd"], ref["rstd"]))
        bwd = f64(R.head_bwd_restate(d["dout"], fwd["h"], fwd["xs"], fwd["mean"], fwd["rstd"], d["W"], d["gamma"], d["beta"]))
        rb = R.head_bwd_ref(d["dout"], fwd["h"], fwd["xs"], fwd["mean"], fwd["rstd"], d["W"], d["gamma"], d["beta"], bwd["dh"])
        for name in ("dx", "dW", "dgamma", "dbeta", "dbias"):
            up("head_" + name, bwd[name], rb[name], rb["S_" + name])
        ln["dh"] = max(ln["dh"], float(row_errors(bwd["dh"], rb["dh"]).max()))
        ln["dx_rows"] = max(ln["dx_rows"], float(row_errors(bwd["dx"], rb["dx_whole"]).max()))
    for c in C.CE_CASES:
        d, ref = C.ce_inputs(c), C.ce_reference(c)
        got = f64(C.restate_ce(c))
        up("ce_lse", got["lse"], ref["lse"], ref["S_lse"])
        if np.isfinite(ref["loss"]).all():
            up("ce_loss", got["loss"], ref["loss"], ref["S_loss"])
        # what remains of dz's error after the allowance for the lse it is fed
        allow = ref["prop"] * C.lse_bar("ce_lse", ref["S_lse"])[:, None] + R.TINY_NORMAL * abs(c.go) / c.rows
        up("ce_dz", ref["dz"] + np.maximum(np.abs(got["dz"] - ref["dz"]) - allow, 0.0), ref["dz"], ref["S_dz"])
    for c in C.DL_CASES:
        ref, got = C.distill_reference(c), f64(C.restate_distill(c))
        up("dl_lse", got["lse3"], ref["lse3"], ref["S_lse3"])
        up("dl_soft", got["out3"][1], ref["out3"][1], ref["S_out3"][1])
        up("dl_ce", got["out3"][2], ref["out3"][2], ref["S_out3"][2])
        T, ws, wc = C.CFGS[c.cfg]
        allow = (ref["prop3"] * C.lse_bar("dl_lse", ref["S_lse3"])[:, :, None]).sum(0) + R.TINY_NORMAL * (abs(ws * T) + abs(wc)) / c.rows
        up("dl_dz", ref["dz"] + np.maximum(np.abs(got["dz"] - ref["dz"]) - allow, 0.0), ref["dz"], ref["S_dz"])
    for c in C.EVAL_CASES:
        d = C.eval_inputs(c)
        _, stats, S = R.eval_ref(d["z"], d["labels"], d["n_valid"], c.k)
        up("ev_loss", R.eval_restate(d["z"], d["labels"], d["n_valid"], c.k)[1]["loss_sum"], stats["loss_sum"], S)
    for name, f in fl.items():
        print(f"HEAD-FLOOR {name} floor = {f:.3f}  c = {C.C_BAR[name]}")
    for name, f in ln.items():
        bar = C.OUT_BAR if name in ("out", "mean", "rstd") else C.GRAD_BAR
        print(f"HEAD-FLOOR {name} worst row error = {f:.3e}  bar = {bar:.0e}")
    for name, f in fl.items():
        assert f <= C.C_BAR[name] / 4, (name, f)
        assert C.C_BAR[name] == math.ceil(4 * f), (name, f)      # four times the floor, rounded up: not a looser one
    for name, f in ln.items():
        assert f <= (C.OUT_BAR if name in ("out", "mean", "rstd") else C.GRAD_BAR) / 4, (name, f)


# ------------------------------------------------------------------------------------------------------------------ 3. mistakes fail
MISTAKES = [("head", "mask_dropped"), ("head", "pool_end_floor"), ("head", "pool_div_n"), ("head", "stats_128"), ("head", "no_eps"),
            ("head", "no_i0_plus_1"), ("eval", "last_max"), ("eval", "tie_le"), ("eval", "tie_ignored"), ("eval", "tie_gt"), ("eval", "tie_all"), ("ce", "no_onehot"), ("distill", "no_onehot"), ("ce", "no_div_rows"),
            ("ce", "no_max_shift"), ("distill", "nearby_always"), ("distill", "nearby_never"), ("distill", "no_T2"), ("eval", "n_valid_ignored"),
            ("ce", "first_sweep_only"), ("distill", "first_sweep_only"), ("eval", "first_sweep_only")]


@pytest.mark.parametrize("family,mutant", MISTAKES, ids=[f"{f}-{m}" for f, m in MISTAKES])
def test_a_plausible_mistake_fails_the_judge(family, mutant):
    if family == "head":
        cases = [c for c in C.HEAD_CASES if c.rows <= 5]
        failed = [c for c in cases if not head_verdict(c, mutant)[0]]
    else:
        cases = C.ALL[family]
        failed = [c for c in cases if not loss_verdict(family, c, mutant)[0]]
    print(f"HEAD-MUTANT {family} {mutant}: fails {len(failed)} of {len(cases)} cases")
    assert failed


@pytest.mark.parametrize("mutant", ["tie_ignored", "tie_gt", "tie_all"])
def test_every_planted_label_tie_catches_a_wrong_tie_rule(mutant):
    """ties ignored, counted at higher indices, counted on both sides: each fails every ties case -- both storage types, each of the
    three instantiations -- and does so through topk alone"""
    cases = [c for c in C.EVAL_CASES if c.kind == "ties"]
    assert len(cases) == 8
    for c in cases:
        ok, worst = loss_verdict("eval", c, mutant)
        assert not ok and worst["topk"] == np.inf and worst["pred"] == worst["top1"] == worst["seen"] == 0, (c, worst)


def test_the_window_below_never_holds_the_column():
    """small_sl_bwd_rows_kernel searches the windows i0 - 1, i0, i0 + 1 for column c, i0 = floor(c n / k).  Window i0 - 1 ends at
    ceil(i0 k / n) <= c (i0 k / n <= c, and c is an integer): it never holds c, so a search without it is the same function -- shown
    here for every (n, k) of the table, and by the restatement's bits -- and the mistake to catch is the search without i0 + 1."""
    for n, k in {(c.n, c.k) for c in C.HEAD_CASES}:
        s0, e0 = R.windows(n, k)
        i0 = np.arange(k) * n // k
        assert ((s0[i0] <= np.arange(k)) & (np.arange(k) < e0[i0])).all()
        assert (e0[np.maximum(i0 - 1, 0)][i0 > 0] <= np.arange(k)[i0 > 0]).all()
    c = next(c for c in C.HEAD_CASES if C.head_bwd_rows_plan(c.n, c.k)["ragged"])
    assert np.array_equal(C.restate_head(c)[1]["dx"], C.restate_head(c, "no_i0_minus_1")[1]["dx"])


def test_the_general_formula_fails_at_a_thousandth():
    """a forward that always took the shifted log-sum-exps misses the soft term of the single-row case at max |d| / T = 1e-3, by far"""
    for c in [c for c in C.DL_CASES if c.kind == "near1e-3" and c.rows == 1]:
        ok, worst = loss_verdict("distill", c, "nearby_never")
        print(f"HEAD-MUTANT nearby_never {C.case_id(c)} out3 ratio {worst['out3']:.1f}")
        assert not ok and worst["out3"] > 4


# ------------------------------------------------------------------------------------------------------------------ the references
def test_references_agree_with_plain_numpy_and_torch():
    import torch
    rng = np.random.default_rng(3)
    z, t, y = rng.standard_normal((6, 11)) * 3, rng.standard_normal((6, 11)) * 3, rng.integers(0, 11, 6)
    zt, tt, yt = torch.tensor(z, requires_grad=True), torch.tensor(t), torch.tensor(y)
    loss = torch.nn.functional.cross_entropy(zt, yt)
    loss.backward()
    ref = R.ce_ref(z, y, 0.75)
    assert np.allclose(ref["loss"][0], loss.item(), rtol=1e-13) and np.allclose(ref["dz"], 0.75 * zt.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert np.allclose(ref["lse"], torch.logsumexp(zt, 1).detach().numpy(), rtol=1e-14)
    T, ws, wc = 2.0, 0.25, 0.75
    zt.grad = None
    soft = torch.nn.functional.kl_div(torch.log_softmax(zt / T, 1), torch.softmax(tt / T, 1), reduction="batchmean") * T * T
    total = ws * soft + wc * torch.nn.functional.cross_entropy(zt, yt)
    total.backward()
    dref = R.distill_ref(z, t, y, T, ws, wc, 1.0)
    assert np.allclose(dref["out3"], [total.item(), soft.item(), loss.item()], rtol=1e-12)
    assert np.allclose(dref["dz"], zt.grad.numpy(), rtol=1e-11, atol=1e-15)
    # the head: windows are AdaptiveAvgPool1d's, the backward is autograd's
    for n, k in ((7, 65), (63, 100), (64, 64), (1, 5)):
        x = rng.standard_normal((3, k))
        assert np.allclose(x @ R.pool_matrix(n, k).T, torch.nn.functional.adaptive_avg_pool1d(torch.tensor(x)[None], n)[0].numpy(), rtol=1e-14)
    n, k = 7, 20
    x, W, b, g, be, dout = (torch.tensor(rng.standard_normal(s), requires_grad=True) for s in ((3, k), (n, k), (n,), (n,), (n,), (3, n)))
    h = x @ W.T + b
    out = torch.nn.functional.gelu(torch.nn.functional.layer_norm(h, (n,), g, be, 1e-5)) + torch.nn.functional.adaptive_avg_pool1d(x[None], n)[0]
    (out * dout).sum().backward()
    a = [v.detach().numpy() for v in (x, W, b, g, be, dout)]
    f = R.head_fwd_ref(a[0], a[1], a[2], a[3], a[4])
    assert np.allclose(f["out"], out.detach().numpy(), rtol=1e-12) and np.allclose(f["h"], h.detach().numpy(), rtol=1e-13)
    r = R.head_bwd_ref(a[5], f["h"], a[0], f["mean"], f["rstd"], a[1], a[3], a[4])
    for name, p in (("dx", x), ("dW", W), ("dbias", b), ("dgamma", g), ("dbeta", be)):
        assert np.allclose(r[name], p.grad.numpy(), rtol=1e-10, atol=1e-13), name
    assert np.allclose(r["dx"], r["dx_whole"], rtol=1e-14)
