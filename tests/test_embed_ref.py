"""CPU checks behind tests/test_gpu_embed_edges.py: the case tables of tests/embed_edge_cases.py reach every branch the restated
dispatch of csrc/spv_patch.hip has; the float32 / bf16-storage restatement of every kernel (tests/embed_ref.py) passes the GPU test's
own judging function on every case; each plausible mistake made in that restatement fails it on at least one case; the floors behind
the bars are measured here, on the reference side alone, and stay within a quarter of each bar; ids are unique and no case needs more
than 80 MB of device buffers."""
import numpy as np
import pytest

import embed_edge_cases as C
import embed_ref as R


# ------------------------------------------------------------------------------------------------------------------ 1. branches
def test_tables_reach_every_branch():
    for dt in C.DTYPES:
        pf = [c for c in C.PATCHIFY_CASES if c.dtype == dt]
        # both kernels in one trip and in two; every mode; the element kernel by each refusing condition alone
        assert {(C.patchify_vec4(c), C.patch_trips(C.patchify_items(c))) for c in pf} == {(True, 1), (True, 2), (False, 1), (False, 2)}
        assert {c.mode for c in pf} == {0, 1, 2} and {c.mode for c in pf if C.patchify_vec4(c)} == {0, 2}
        alone = dict(P=lambda c: c.P % 4, W=lambda c: c.W % 4, ld=lambda c: c.ld % 4, img=lambda c: c.off == "img", out=lambda c: c.off == "out")
        for name, refuses in alone.items():
            if name == "W":     # a width off 4 pixels with a whole number of 4-pixel patches does not exist: W = 10 leaves two pixels unused
                assert any(refuses(c) and c.mode != 1 and c.P % 4 == 0 and c.ld % 4 == 0 and c.off == "" for c in pf), name
            else:
                assert any(refuses(c) and c.mode != 1 and not any(r(c) for n, r in alone.items() if n != name) for c in pf), name
        for c in pf:
            if c.off:
                assert c._replace(off="") in pf and C.patchify_vec4(c._replace(off=""))       # the aligned twin, on the other kernel
        Ks = {c: C.geometry(c)[1] for c in pf}
        assert any(c.mode == 2 and c.ld == Ks[c] for c in pf) and any(c.mode == 0 and c.ld > Ks[c] for c in pf) and any(c.mode == 2 and c.ld > Ks[c] for c in pf)
        assert any(c.mode == 1 and c.ld == C.round8(c.B * C.geometry(c)[0]) > c.B * C.geometry(c)[0] for c in pf)
        assert any(c.B == 1 for c in pf) and any(c.H % c.P and c.W % c.P for c in pf) and any(c.P == 7 and c.ld == 49 for c in pf)
        u8 = [c for c in C.U8_CASES if c.dtype == dt]
        assert {(c.mode, c.C, c.P) for c in u8} >= {(m, ch, p) for m in (0, 1, 2) for ch, p in ((3, 4), (1, 7))} and {c.C for c in u8} == {1, 3}
        assert {C.patch_trips(C.out_elems(c)) for c in u8} == {1, 2}
        assert any(c.ld > (C.geometry(c)[1] if c.mode != 1 else c.B * C.geometry(c)[0]) for c in u8)
        cr = [c for c in C.CLS_ROWS_CASES if c.dtype == dt]
        assert {C.patch_trips(c.B * c.E) for c in cr} == {1, 2} and any(c.T > 1 for c in cr)
        dr = [c for c in C.DROPOUT_CASES if c.dtype == dt]
        assert {C.patch_trips(C.cdiv(c.n, 8)) for c in dr} == {1, 2} and {c.p for c in dr} == {0.0, C.P_DROP}
        assert {c.n for c in dr} >= {1, 7, 8, 9, 4095, 4096, 4097, 8200} and any(c.n % 8 for c in dr if c.n > 2 ** 20)
    for cls in (0, 1):
        assert {C.patch_trips((c.Np + 1) * c.E if cls else c.Np * c.E) for c in C.POSBIAS_CASES if c.cls == cls} == {1, 2}
    # spectral fold: every patch size, every workgroup size of the frequency-weight sums, E C below / at / above it, the second trips
    assert {c.P for c in C.FOLD_CASES} == {1, 2, 3, 4, 7, 8, 16, 32, 64}
    assert {R.fold_bwd_threads(c.P) for c in C.FOLD_CASES} == {1024, 512, 256, 128, 64}
    assert {np.sign(c.E * c.C - R.fold_bwd_threads(c.P)) for c in C.FOLD_CASES} == {-1, 0, 1}
    assert {C.patch_trips(c.E * c.C * c.P * c.P) for c in C.FOLD_CASES} == {1, 2} == {C.patch_trips(c.E * c.C * c.P * (c.P // 2 + 1)) for c in C.FOLD_CASES}
    assert all(R.fold_bwd_threads(c.P) * (c.P + c.P // 2 + 1) * 4 <= 64 * 1024 for c in C.FOLD_CASES) and all(c.P > 64 for c in C.FOLD_BWD_REFUSED)
    # embedding backward
    for dt in C.DTYPES:
        eb = [c for c in C.EMBED_BWD_CASES if c.dtype == dt]
        plans = [C.embed_bwd_plan(c) for c in eb]
        assert {c.B for c in eb} == {1, 8, 9, 16, 17, 33, 120, 130}
        assert {p["last"] for p in plans} >= {1, 2, 8, 9, 16}                       # ragged half-group, the half, half + 1, a whole group
        assert {p["fold"] for p in plans} >= {(0, 1), (0, 2), (0, 3), (1, 0), (1, 1)}     # scalar tails, one unrolled batch, a batch and a tail
        assert {p["bias"] for p in plans} >= {(0, 0), (0, 1), (0, 4), (1, 0), (1, 1), (2, 0)}
        assert {p["cblocks"] for p in plans} == {1, 2} and any(c.T * c.E == 2304 for c in eb) and {c.E for c in eb} == {8, 24, 256}
        assert {(c.gcls, c.p > 0) for c in eb} == {(0, False), (0, True), (1, True)} | ({(1, False)} if any(c.gcls and c.p == 0 for c in eb) else set())
        assert any(not c.dtok for c in eb) and all(c.dtok or (not c.gcls and c.p == 0) for c in eb)
        assert any(all(C.mask_crossings(c)) and c.p > 0 for c in eb) and any(c == c._replace(B=33, T=9, E=24) and c.p > 0 for c in eb)
    assert {(c.gcls, c.p > 0) for c in C.EMBED_BWD_CASES} == {(0, False), (0, True), (1, True), (1, False)}
    assert len(C.EMBED_BWD_CASES) == 30


def test_ids_unique_and_buffers_small():
    for family, cases in C.ALL.items():
        ids = [C.case_id(c) for c in cases]
        assert len(set(ids)) == len(ids), family
        for c in cases:
            assert C.device_bytes(family, c) <= C.LIMIT_BYTES, (family, c, C.device_bytes(family, c))


# ------------------------------------------------------------------------------------------------------------------ 2. restatements pass
@pytest.mark.parametrize("family", list(C.ALL))
def test_restatement_passes_the_judge(family):
    for c in C.ALL[family]:
        got = C.restate(family, c)
        ok, worst = C.verdict(C.expect(family, c), got)
        print(f"EMBED-REF {family} {C.case_id(c)} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
        assert ok, (family, c, worst)
        if family == "embed_bwd":
            assert np.array_equal(got["dcls"], got["dpos"][0])


def test_floors_stay_within_a_quarter_of_the_bars():
    """the float32 restatement, before any storage rounding, against float64 on the GPU cases' inputs"""
    floors = dict.fromkeys(C.C_BAR, 0.0)
    per_p = {}
    for c in C.U8_CASES:
        d = C.inputs("patchify_u8", c)
        out, S = R.patchify_u8_ref(d["img"], d["mean"], d["inv_std"], c.P, c.mode, c.ld)
        floors["patchify_u8"] = max(floors["patchify_u8"], C.floor_ratio(R.patchify_u8_restate(d["img"], d["mean"], d["inv_std"], c.P, c.mode, c.ld, "fp32"), out, S))
    for c in C.FOLD_CASES:
        s = C.expect("fold", c)["wf"]
        per_p[c.P] = max(per_p.get(c.P, 0.0), C.floor_ratio(C.restate("fold", c)["wf"], s.ref, s.bar / (C.C_BAR["fold"] * C.EPS)))
        got = C.restate("fold_bwd", c)
        for k, s in C.expect("fold_bwd", c).items():
            floors["fold_bwd"] = max(floors["fold_bwd"], C.floor_ratio(got[k], s.ref, s.bar / (C.C_BAR["fold_bwd"] * C.EPS)))
    floors["fold"] = max(per_p.values())
    print("EMBED-FLOOR fold by patch size: " + " ".join(f"P={p}:{f:.2f}" for p, f in sorted(per_p.items())))
    for c in C.EMBED_BWD_CASES:
        got = C.restate("embed_bwd", c)
        for k, s in C.expect("embed_bwd", c).items():
            if s.kind == "bar":
                floors["embed_bwd"] = max(floors["embed_bwd"], C.floor_ratio(got[k], s.ref, s.bar / (C.C_BAR["embed_bwd"] * C.EPS)))
    for name, f in floors.items():
        print(f"EMBED-FLOOR {name} floor = {f:.3f}  c = {C.C_BAR[name]}")
        assert f <= C.C_BAR[name] / 4, (name, f)
        assert C.C_BAR[name] < 4 * f + 2, (name, f)      # the bar is the measured floor's, not a looser one


# ------------------------------------------------------------------------------------------------------------------ 3. mistakes fail
MISTAKES = [("patchify", "swap_pq"), ("patchify", "cls_not_zero"), ("patchify", "pad_not_zero"), ("patchify_u8", "swap_pq"),
            ("patchify_u8", "cls_not_zero"), ("patchify_u8", "pad_not_zero"), ("patchify_u8", "pad_small"), ("patchify_u8", "pad_neg_zero"), ("posbias", "pos_t"), ("fold", "no_1_over_P"),
            ("fold", "half_as_full"), ("embed_bwd", "dbias_with_cls"), ("embed_bwd", "dcls_row_1"), ("embed_bwd", "gcls_every_row"),
            ("embed_bwd", "mask_no_sample_offset"), ("embed_bwd", "key_shift_11"), ("embed_bwd", "last_group_dropped"),
            ("dropout", "key_shift_11")]


@pytest.mark.parametrize("family,mutant", MISTAKES, ids=[f"{f}-{m}" for f, m in MISTAKES])
def test_a_plausible_mistake_fails_the_judge(family, mutant):
    big = dict(patchify=2 ** 19, patchify_u8=2 ** 19, dropout=2 ** 20)       # (the second-trip cases add nothing to a mistake's verdict)
    cases = [c for c in C.ALL[family] if family not in big or C.device_bytes(family, c) < big[family]]
    failed = [c for c in cases if not C.verdict(C.expect(family, c), C.restate(family, c, mutant))[0]]
    print(f"EMBED-MUTANT {family} {mutant}: fails {len(failed)} of {len(cases)} cases")
    assert failed


# ------------------------------------------------------------------------------------------------------------------ the references
def test_references_agree_with_plain_numpy():
    rng = np.random.default_rng(11)
    img = rng.standard_normal((2, 3, 8, 12))
    rows = R.patch_rows(img, 4)
    assert rows.shape == (2, 6, 48)
    assert np.array_equal(rows[1, 4].reshape(3, 4, 4), img[1, :, 4:8, 4:8])       # patch (ih, iw) = (1, 1), (c, p, q) order
    t = R.layout(rows, 2, 56)
    assert not t[:, 0].any() and not t[:, :, 48:].any() and np.array_equal(t[:, 1:, :48], rows)
    assert np.array_equal(R.layout(rows, 1, 16)[:, :12], rows.reshape(12, 48).T)
    # the basis is the real part of the orthonormal rfft2: folding equals transforming
    P = 6
    x = rng.standard_normal((P, P))
    assert np.allclose(np.einsum("uvpq,pq->uv", R.basis(P), x), np.fft.rfft2(x, norm="ortho").real, rtol=0, atol=1e-13)
    w, fh, fw = rng.standard_normal((2, 3, P, P // 2 + 1)), rng.standard_normal(P), rng.standard_normal(P // 2 + 1)
    wf, _ = R.fold_ref(w, fh, fw)
    patch = rng.standard_normal((3, P, P))
    direct = ((w * fh[:, None] * fw[None, :]) * np.fft.rfft2(patch, norm="ortho").real[None]).sum((1, 2, 3))
    assert np.allclose((wf * patch[None]).sum((1, 2, 3)), direct, rtol=0, atol=1e-12)
    # the fold's backward is the transpose of the fold
    dwf = rng.standard_normal(wf.shape)
    ref, _ = R.fold_bwd_ref(dwf, w, fh, fw)
    h = 1e-6
    for name, arr, grad in (("dw", w, ref["dw"]), ("dfh", fh, ref["dfh"]), ("dfw", fw, ref["dfw"])):
        d = rng.standard_normal(arr.shape)
        args = [a + h * d if a is arr else a for a in (w, fh, fw)]
        num = ((R.fold_ref(*args)[0] - wf) * dwf).sum() / h
        assert abs(num - (grad * d).sum()) <= 1e-4 * max(1.0, abs(num)), name
    # the two statements of the mask agree
    import dropout_ref as D
    keep = D.keep(C.SEED, 3, 4096, 0.3).reshape(-1)
    assert np.array_equal(R.mask_scale(C.SEED, np.arange(3 * 4096), 0.3) != 0, keep) and 0.6 < keep.mean() < 0.8
