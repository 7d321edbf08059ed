"""CPU checks behind tests/test_gpu_branch_edges.py: the case tables of tests/branch_edge_cases.py reach every branch the restated
dispatch of csrc/spv_branch.hip has (padded and unpadded K, Mp > M and Mp == M, one and two trips of each grid-stride loop, the GEMM
kernels the preset reaches at batch 512, collapsed splits); the float32 restatement of every kernel (tests/branch_ref.py) passes the
GPU test's own judging function on every case; each plausible mistake made in that restatement fails it on at least one case; the
spectrum's floor is measured here, on the reference side alone, and stays within a quarter of its bar; the references agree with
torch's float64 CPU operators; ids are unique and no buffer exceeds 80 MiB."""
import math

import numpy as np
import pytest

import branch_edge_cases as C
import branch_ref as R

SMALL = 200_000        # elements: the cases above it (the second trips) are restated once, in the test that is about them


def small(c):
    return max(C.buffer_elems(c).values()) <= SMALL


def families(c):
    if isinstance(c, C.SP):
        return ["spectrum"]
    if isinstance(c, C.PL):
        return [f for f, k in (("pool_fwd", "f"), ("pool_bwd", "b")) if k in c.dirs]
    return C.entries_of(c)


def judged(family, c, mutant=None):
    return C.settle(C.expect(family, c), C.restate(family, c, mutant), C.poison(family, c))


# ------------------------------------------------------------------------------------------------------------------ 1. branches
def test_spectrum_table_reaches_every_branch():
    planes = {(c.H, c.W) for c in C.SPECTRUM_CASES}
    assert planes == set(C.PLANES) and {(c.B, c.C) for c in C.SPECTRUM_CASES if c.kind == "plain" and not c.off} == {(1, 1), (2, 3)}
    assert C.spectrum_floats(126, 124) == 16376 and max(C.spectrum_floats(*p) for p in planes) == C.spectrum_floats(147, 107) == C.SPECTRUM_LIMIT
    assert C.spectrum_floats(127, 124) == 16504 and C.spectrum_floats(148, 107) == 16494        # the first refused next to each
    assert any(h == 1 for h, _ in planes) and any(w == 1 for _, w in planes) and any(w == 2 for _, w in planes)
    assert any(h > 256 // (w // 2 + 1) for h, w in planes)        # more bins than threads: the per-thread loops take a second trip
    assert {c.dtype for c in C.SPECTRUM_CASES if c.kind == "special"} == {c.dtype for c in C.SPECTRUM_CASES if c.off} == set(C.DTYPES)
    c = next(c for c in C.SPECTRUM_CASES if c.kind == "special")
    img, ref = C.spectrum_inputs(c).reshape(6, 17, 9), R.spectrum_ref(C.spectrum_inputs(c))
    out = ref["out"].transpose(0, 3, 1, 2).reshape(6, 17, 5)
    assert not img[0].any() and not out[0].any() and not np.signbit(out[0]).any()
    assert (img[1] == 1.25).all() and out[1, 0, 0] == np.log1p(1.25 * 153) and np.abs(np.delete(out[1].reshape(-1), 0)).max() < 1e-12
    assert np.isinf(img[2]).sum() == 1 and np.isnan(img[3]).sum() == 1 and np.isnan(out[2:4]).all() and np.isfinite(out[4:]).all()
    assert {r.why for r in C.SPECTRUM_REFUSED} == {"plane-127x124", "plane-148x107", "B=0", "H=0", "dtype"}


def test_conv_tables_reach_every_branch():
    for dt in C.DTYPES:
        mine = [c for c in C.CONV_CASES if c.dtype == dt]
        geo = [C.geometry(c) for c in mine]
        assert {g["Kp"] > g["K"] for g in geo} == {g["Mp"] > g["M"] for g in geo} == {g["Kd"] > 9 * c.Cout for g, c in zip(geo, mine)} == {True, False}
        assert {g["M"] % 8 for g in geo} >= {0, 1, 7} and any(g["M"] == 1 for g in geo)
        assert {(c.B, c.H, c.W, c.Cin, c.Cout) for c in mine} >= set(C.CONV_SHAPES)
        for c in mine:
            assert c.which != "int" or C.exact_ok(c), c
        # one and two trips of each of the four gather launches
        t = dict(fwd=set(), dgrad=set(), dyt=set(), colst=set())
        for c in mine:
            tot = C.gather_totals(c)
            for e, names in (("f", ("fwd",)), ("d", ("dgrad",)), ("w", ("dyt", "colst"))):
                if e in c.entries:
                    for n in names:
                        t[n].add(C.trips(tot[n]))
        assert all(v == {1, 2} for v in t.values()), t
        big = [c for c in mine if c.tag == "trip2"]
        assert sorted(C.gather_totals(c)[n] for c in big for e, n in (("f", "fwd"), ("d", "dgrad"), ("w", "dyt"), ("w", "colst")) if e in c.entries) == \
            [17713152, 17713152, 17713152, 18000000]
        assert all(9 * C.geometry(c)["Mp"] < 2 ** 24 for c in big)
        # the weight gradient's slabs: asked 1, 2, 3, 4, 7; fewer than asked; collapsed to one
        w = [c for c in mine if "w" in c.entries]
        assert {c.splits for c in w} >= {1, 2, 3, 4, 7} and any(1 < C.slabs_of(c) < c.splits for c in w)
        assert [C.slabs_of(c) for c in w if c.tag == "collapses"] == [1] and all(c.splits == 4 for c in w if c.tag == "collapses")
        assert any(C.slabs_of(c) * C.conv_plan("wgrad", c)["k_per_split"] > C.geometry(c)["Mp"] for c in w if c.splits > 1)   # splits do not divide the K-tiles
        kern = {c.tag: C.conv_plan("wgrad", c)["kernel"] for c in w if c.tag.startswith("slice")}
        assert kern == (dict(slice2176="glds", slice1088="glds", slice768="tile") if dt == "bf16" else dict.fromkeys(kern, "tile")) and len(kern) == 3
        assert {c.off for c in mine} == {""} | set(C.ALIGNED_OK) and {c.which for c in mine} == {"int", "normal", "special"}
    # the census: what the preset reaches at batch 512 is reached here, and nothing else is
    census = C.preset_census()
    here = {(e, c.dtype, C.conv_plan(e, c)["kernel"], C.conv_plan(e, c)["reduce"]) for c in C.CONV_CASES for e in C.entries_of(c)}
    print("BRANCH-CENSUS preset:", sorted(census))
    print("BRANCH-CENSUS cases: ", sorted(here))
    assert census <= here and {k[:3] for k in here} == {k[:3] for k in census}
    # beyond the preset: the one-slab weight gradient of the small maps, on both of its kernels
    assert here - census == {("wgrad", dt, "tile", 0) for dt in C.DTYPES} | {("wgrad", "bf16", "glds", 0)}
    # the refusals are refusals of the restated plan too, and the accepted misalignments are not
    for r in C.CONV_REFUSED:
        if r.match.startswith("spv_gemm_nt"):
            assert C.conv_plan(r.entry, r.case)["kernel"] == dict(A="refuse_align", s="refuse_splits")[r.match[13]] if "split-K" not in r.match \
                else C.conv_plan(r.entry, r.case)["kernel"] == "refuse_workspace", r
    assert {(r.entry, r.why.split("-off-")[0]) for r in C.CONV_REFUSED if "-off-" in r.why} == set(C.ALIGNED_MUST)
    assert {r.why for r in C.CONV_REFUSED if "-off-" not in r.why} == {"B=0", "H=2", "W=2", "Cin=0", "Cout=0", "dtype", "splits=0", "splits=2-null-workspace"}
    for c in C.CONV_CASES:
        if c.off:
            assert all(not C.conv_plan(e, c)["kernel"].startswith("refuse") for e in C.entries_of(c)), c


def test_special_values_leave_clean_and_poisoned_outputs():
    for c in [c for c in C.CONV_CASES if c.which == "special"]:
        d = C.conv_inputs(c)
        for k in ("x", "dy"):
            v = d[k].reshape(-1)
            assert np.isnan(v).sum() == 1 and np.isposinf(v).sum() == 1 and np.isneginf(v).sum() == 1 and (v == C.HUGE[c.dtype]).sum() == 1
            assert (np.abs(v) == C.TINY[c.dtype]).sum() == 2 and (v == 0).sum() == 2 and np.signbit(v[v == 0]).sum() == 1
        for e in C.entries_of(c):
            specs, poison = C.expect(e, c), C.poison(e, c)
            name = dict(fwd="y", dgrad="dx", wgrad="dw")[e]
            mode, mask = poison[name]
            assert mode == "nonfinite" and 0 < mask.sum() < mask.size, (c, e)
            s = specs[name]
            S = (s.bar - (2.0 ** -8 * np.abs(s.ref) if s.dtype == "bf16" else 0.0)) / ((C.chain(e, c) + 2) * C.EPS)
            assert np.isfinite(s.ref).all() and float(S[~mask].max()) < 2.0 ** 127        # no partial sum of a clean output overflows
            assert all(poison[k][0] == "nan" and poison[k][1].sum() >= 1 for k in specs if k != name), (c, e)


def test_pool_table_reaches_every_branch():
    for dt in C.DTYPES:
        mine = [c for c in C.POOL_CASES if c.dtype == dt]
        assert {(c.L, c.T) for c in mine} >= set(C.POOL_LT) and {c.C for c in mine} >= {1, 7, 8} and {c.B for c in mine} >= {1, 3}
        for C_ in (1, 7, 8):
            assert {c.ldo for c in mine if c.C == C_ and not c.off} >= {C_, C.round8(C_), C_ + 3}
        assert {c.add for c in mine if "b" in c.dirs} == {0, 1} and {c.off for c in mine} == {"", "y", "out", "dout", "add", "dy"}
        assert {(c.L, c.T) for c in mine if c.which == "int"} == set(C.POOL_EXACT) and all(C.pool_exact_ok(c) for c in mine if c.which == "int")
        assert {(c.L < c.T, c.L == c.T, c.L % c.T == 0) for c in mine} >= {(True, False, False), (False, True, True), (False, False, True), (False, False, False)}
        assert {C.trips(c.B * c.T * c.ldo) for c in mine if "f" in c.dirs} == {C.trips(c.B * c.L * c.C) for c in mine if "b" in c.dirs} == {1, 2}
        assert all(np.isnan(C.pool_inputs(c)["dout"][..., c.C:]).all() for c in mine[:40] if "b" in c.dirs)
    assert {r.why for r in C.POOL_REFUSED} == {"B=0", "L=0", "C=0", "T=0", "ldo=C-1", "dtype"} and {r.entry for r in C.POOL_REFUSED} == {"fwd", "bwd"}


def test_ids_unique_and_buffers_small():
    for family, cases in C.ALL.items():
        ids = [C.case_id(c) for c in cases]
        assert len(set(ids)) == len(ids), family
    for c in C.CONV_CASES + C.POOL_CASES:
        assert max(C.buffer_elems(c).values()) * 4 <= C.LIMIT_BYTES, c
    assert len({C.case_id(r) for r in C.CONV_REFUSED}) == len(C.CONV_REFUSED)


# ------------------------------------------------------------------------------------------------------------------ 2. restatements pass
@pytest.mark.parametrize("family", ["spectrum", "conv", "pool"])
def test_restatement_passes_the_judge(family):
    for c in [c for c in C.ALL[family] if small(c)]:
        for f in families(c):
            ok, worst = judged(f, c)
            print(f"BRANCH-REF {f} {C.case_id(c)} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
            assert ok, (f, c, worst)


@pytest.mark.parametrize("case", [c for c in C.CONV_CASES + C.POOL_CASES if not small(c)], ids=C.case_id)
def test_second_trip_restatement_passes_the_judge(case):
    for f in families(case):
        ok, worst = judged(f, case)
        assert ok, (f, case, worst)


def test_spectrum_floor_stays_within_a_quarter_of_the_bar():
    """the float32 restatement, before any storage rounding, against float64 on the GPU cases' inputs"""
    floor, per = 0.0, {}
    for c in [c for c in C.SPECTRUM_CASES if c.dtype == "fp32"]:
        img = C.spectrum_inputs(c)
        ref = R.spectrum_ref(img)
        fin = np.isfinite(ref["out"])
        got = R.spectrum_restate(img).astype(np.float64)
        f = C.floor_ratio(got[fin], ref["out"][fin], (ref["S"] / (1 + ref["X"]) + np.abs(ref["out"]))[fin])
        per[(c.H, c.W)] = max(per.get((c.H, c.W), 0.0), f)
        floor = max(floor, f)
    print(f"BRANCH-FLOOR spectrum floor = {floor:.3f}  c = {C.C_BAR['spectrum']}  " + " ".join(f"{h}x{w}:{f:.3f}" for (h, w), f in per.items()))
    assert floor <= C.C_BAR["spectrum"] / 4
    assert C.C_BAR["spectrum"] == math.ceil(4 * floor)        # four times the floor, rounded up: not a looser one


# ------------------------------------------------------------------------------------------------------------------ 3. mistakes fail
MISTAKES = [("fwd", "k_order_yxc"), ("wgrad", "k_order_yxc"), ("fwd", "swap_kykx"), ("wgrad", "swap_kykx"), ("fwd", "pads_unwritten"),
            ("dgrad", "pads_unwritten"), ("wgrad", "pads_unwritten"), ("pool_fwd", "pads_unwritten"), ("dgrad", "dgrad_sign"), ("dgrad", "dgrad_clamp"),
            ("wgrad", "ld_M"), ("pool_fwd", "end_floor"), ("pool_bwd", "bwd_wrong_len"), ("pool_bwd", "bwd_one_window"),
            ("spectrum", "nyquist_dropped"), ("spectrum", "w_table_for_columns"), ("spectrum", "log")]


@pytest.mark.parametrize("family,mutant", MISTAKES, ids=[f"{f}-{m}" for f, m in MISTAKES])
def test_a_plausible_mistake_fails_the_judge(family, mutant):
    table = C.SPECTRUM_CASES if family == "spectrum" else C.POOL_CASES if family.startswith("pool") else C.CONV_CASES
    cases = [c for c in table if small(c) and family in families(c)]
    failed = [c for c in cases if not judged(family, c, mutant)[0]]
    print(f"BRANCH-MUTANT {family} {mutant}: fails {len(failed)} of {len(cases)} cases")
    assert failed


def test_one_wrong_element_fails_where_relative_l2_passed():
    """what the wrapper tests' relative L2 of 1e-2 lets through: one border element of a bf16 data gradient off by a quarter"""
    c = next(c for c in C.CONV_CASES if c.dtype == "bf16" and c.which == "normal" and (c.H, c.W, c.Cin) == (9, 8, 27))
    got = C.restate("dgrad", c)
    ref = C.expect("dgrad", c)["dx"].ref
    got["dx"] = got["dx"].copy()
    got["dx"][0, 0] += 0.25
    assert np.linalg.norm(got["dx"] - ref) / np.linalg.norm(ref) < 1e-2
    assert not C.settle(C.expect("dgrad", c), got, C.poison("dgrad", c))[0]


# ------------------------------------------------------------------------------------------------------------------ the references
def test_references_agree_with_torch_float64():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(11)
    for shape in ((2, 3, 17, 9), (1, 1, 1, 8), (1, 2, 8, 1), (1, 1, 13, 31)):
        img = rng.standard_normal(shape)
        want = torch.log1p(torch.fft.rfft2(torch.tensor(img)).abs()).permute(0, 2, 3, 1).numpy()
        assert np.allclose(R.spectrum_ref(img)["out"], want, rtol=1e-12, atol=1e-13)
        assert np.allclose(R.spectrum_restate(img), want, rtol=1e-4, atol=1e-4)
    for B, H, W, Cin, Cout in ((2, 5, 4, 1, 5), (3, 6, 7, 3, 9), (1, 3, 3, 2, 1)):
        x, w, b, dy = (rng.standard_normal(s) for s in ((B, H, W, Cin), (Cout, Cin, 3, 3), (Cout,), (B, H - 2, W - 2, Cout)))
        xt, wt, bt = (torch.tensor(v, requires_grad=True) for v in (x.transpose(0, 3, 1, 2), w, b))
        y = F.conv2d(xt, wt, bt)
        y.backward(torch.tensor(dy.transpose(0, 3, 1, 2)))
        M = B * (H - 2) * (W - 2)
        assert np.allclose(R.conv_fwd(x, w, b)[0], y.detach().permute(0, 2, 3, 1).reshape(M, Cout).numpy(), rtol=1e-12, atol=1e-13)
        assert np.allclose(R.conv_dgrad(dy, w)[0], xt.grad.permute(0, 2, 3, 1).reshape(B * H * W, Cin).numpy(), rtol=1e-12, atol=1e-13)
        assert np.allclose(R.conv_wgrad(dy, x)[0], wt.grad.reshape(Cout, 9 * Cin).numpy(), rtol=1e-12, atol=1e-13)
        # the layouts against their definitions, element by element
        cols, dc = R.im2col(x, C.round8(9 * Cin)), R.dcols(dy, C.round8(9 * Cout))
        for m in range(M):
            bb, ho, wo = m // ((H - 2) * (W - 2)), m // (W - 2) % (H - 2), m % (W - 2)
            for k in range(cols.shape[1]):
                c, ky, kx = k // 9, k % 9 // 3, k % 3
                assert cols[m, k] == (x[bb, ho + ky, wo + kx, c] if k < 9 * Cin else 0.0)
        for m in range(B * H * W):
            bb, h, ww = m // (H * W), m // W % H, m % W
            for k in range(dc.shape[1]):
                co, ky, kx = k // 9, k % 9 // 3, k % 3
                inside = k < 9 * Cout and 0 <= h - ky < H - 2 and 0 <= ww - kx < W - 2
                assert dc[m, k] == (dy[bb, h - ky, ww - kx, co] if inside else 0.0)
        t = R.transposed(cols[:, :9 * Cin], C.round8(M))
        assert t.shape == (9 * Cin, C.round8(M)) and np.array_equal(t[:, :M], cols[:, :9 * Cin].T) and not t[:, M:].any()
    for L, T in ((40, 65), (65, 65), (66, 65), (130, 65), (450, 65), (7, 3), (1, 5), (5, 1)):        # L < T, L == T, L no multiple of T
        y, dout, add = rng.standard_normal((2, L, 3)), rng.standard_normal((2, T, 5)), rng.standard_normal((2, L, 3))
        yt = torch.tensor(y.transpose(0, 2, 1), requires_grad=True)
        out = F.adaptive_avg_pool1d(yt, T)
        out.backward(torch.tensor(dout[..., :3].transpose(0, 2, 1)))
        f = R.pool_fwd(y, T, 5)
        assert np.allclose(f["out"][..., :3], out.detach().permute(0, 2, 1).numpy(), rtol=1e-13, atol=1e-14) and not f["out"][..., 3:].any()
        assert np.allclose(R.pool_bwd(dout, L, 3, add)["dy"], yt.grad.permute(0, 2, 1).numpy() + add, rtol=1e-13, atol=1e-14)
        assert np.allclose(R.pool_fwd_restate(y, T, 5), f["out"], rtol=1e-5, atol=1e-6)
        assert np.allclose(R.pool_bwd_restate(dout, L, 3, add), R.pool_bwd(dout, L, 3, add)["dy"], rtol=1e-5, atol=1e-6)
