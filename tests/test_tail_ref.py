"""CPU checks behind tests/test_gpu_tail_edges.py: tests/tail_ref.py against torch's float64 autograd; the case table reaches every
dispatch branch of the SpectreLinear tail (through tail_edge_cases.expected_path, so deleting a row fails here); the reference's own
rounding floor on the table's inputs stays within a quarter of each fp32 bar and within 2^-8 per row in bf16; each of seven plausible
kernel mistakes, made in the reference, exceeds a bar in both dtypes; and the host refuses what no kernel serves before any launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_ref as D
import tail_edge_cases as C
import tail_ref as R
from oracle import spectre_oracle as O


def small(entry=None, **kw):
    """the 5-row cases of an entry, filtered by fields"""
    return [c for c in C.CASES if c.rows == 5 and (entry is None or c.entry == entry) and all(getattr(c, k) == v for k, v in kw.items())]


# ------------------------------------------------------------------------------------------ 1. reference vs an independent definition
def _autograd(c, run):
    i, p = C.inputs(c, run), C.RUNS[run]["p"]
    T = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    leaf = lambda a: T(a).requires_grad_(True)
    mask = lambda keep, pp: 1.0 if keep is None else T(keep.astype(np.float64) * float(D.inv_keep(pp)))
    pool = lambda a, n_out: F.adaptive_avg_pool1d(a.unsqueeze(1), n_out).squeeze(1)
    h, x, gamma, beta = (leaf(i[k]) for k in ("h", "x", "gamma", "beta"))
    m = mask(C.keep_mask(c, run), p)
    out = (F.gelu(F.layer_norm(h, (c.n,), gamma, beta, 1e-5)) + pool(x, c.n)) * m
    out.retain_grad()
    got = dict(out=out, mean=h.mean(-1), rstd=1.0 / torch.sqrt(h.var(-1, unbiased=False) + 1e-5))
    if c.entry == "ln":
        gamma2, beta2 = leaf(i["gamma2"]), leaf(i["beta2"])
        s = T(i["x1"]) + out
        s.retain_grad()
        out2 = F.layer_norm(s, (c.n,), gamma2, beta2, 1e-5)
        (out2 * T(i["dout2"])).sum().backward()
        got.update(out2=out2, mean2=s.mean(-1), rstd2=1.0 / torch.sqrt(s.var(-1, unbiased=False) + 1e-5), ds=s.grad, dgamma2=gamma2.grad,
                   dbeta2=beta2.grad)
    else:
        loss = (out * T(i["dout"])).sum()
        if c.entry == "up":   # the layer above pools this layer's output into its own skip, under its own mask
            loss = loss + (pool(out, 512) * mask(C.keep_up(c), c.p_up) * T(i["up_src"])).sum()
        loss.backward()
    got.update(dh=h.grad, dx_pool=x.grad + (T(i["dx_add"]) if c.dx_add else 0.0), dgamma=gamma.grad, dbeta=beta.grad, dbias=h.grad.sum(0))
    return {k: v.detach().numpy() for k, v in got.items()}


AUTOGRAD_CASES = [small("tail", dtype="fp32", n=n, k_in=k, off=0, null_dx=False, defer=False)[-1]
                  for n, k in ((64, 64), (64, 256), (16, 48), (96, 48), (96, 64), (104, 512), (768, 512), (7, 8))]
AUTOGRAD_CASES += small("ln", dtype="fp32", null_dx=False, defer=False) + small("up", dtype="fp32") + small("ln", dtype="bf16", null_dx=False, defer=False)


@pytest.mark.parametrize("run", ["A", "B"])
@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=C.case_id)
def test_reference_equals_torch_float64_autograd(case, run):
    """one shape per pooling mode (identity, exact, repeat, both table kinds), LayerNorm-2 and the skip gradient of the layer above"""
    ref, got = C.exact_reference(case, run), _autograd(case, run)
    for name in C.outputs(case):
        e = np.abs(got[name] - ref[name]).max() / np.abs(ref[name]).max()
        assert e <= 1e-12, (C.case_id(case), run, name, e)


def test_row_errors_and_col_error():
    ref = np.array([[1.0, -4.0], [0.0, 0.0], [0.0, 0.0], [2.0, 0.0]])
    got = np.array([[1.5, -4.0], [0.0, 0.0], [0.0, 1e-30], [np.nan, 0.0]])
    assert R.row_errors(got, ref).tolist() == [0.125, 0.0, np.inf, np.inf]
    assert R.col_error([1.0, 2.5], [1.0, 2.0]) == 0.25 and R.col_error([0.0], [0.0]) == 0.0


# ------------------------------------------------------------------------------------------ 2. the table reaches every branch
def test_no_case_is_refused_and_the_census_follows_the_family():
    for c in C.CASES:
        fwd, bwd = C.case_paths(c)
        assert fwd[0] != "refused" and bwd[0] != "refused", (C.case_id(c), fwd, bwd)
        want = {"ln": {"tail_ln": 2}, "up": {"tail_lc": 1, "tail_up": 1}}.get(c.entry)
        if want is None:
            want = {"tail_lc": 2} if fwd[0] == "lc" else {}
            assert (fwd[0] == "lc") == (bwd[0] == "lc"), C.case_id(c)
        assert C.expected_census(c) == want, C.case_id(c)


def test_table_covers_every_dispatch_branch():
    fwd = {(C.case_paths(c)[0], c.dtype) for c in C.CASES}
    bwd = {(C.case_paths(c)[1], c.dtype) for c in C.CASES}
    missing = []

    def need(what, ok):
        if not ok:
            missing.append(what)

    for dt in ("fp32", "bf16"):
        for co, ci in C.LC_PAIRS:
            need(f"LC<{co},{ci}> forward {dt}", (("lc", co, ci), dt) in fwd)
            need(f"LC<{co},{ci}> backward {dt}", (("lc", co, ci), dt) in bwd)
        need(f"LN2 {dt}", (("ln", 8, 12), dt) in fwd and (("ln", 8, 12), dt) in bwd)
        need(f"bwd_up {dt}", (("up", 12, 8), dt) in bwd)
        need(f"wide {dt}", (("wide",), dt) in fwd and (("wide",), dt) in bwd)
        for side, paths in (("forward", fwd), ("backward", bwd)):
            gen = {p[1:] for p, d in paths if p[0] == "generic" and d == dt}
            for vm in ((4, 2), (4, 3), (4, 4), (4, 12), (4, 16), (1, 16)):
                need(f"generic <{vm[0]},{vm[1]}> {side} {dt}", any(g[:2] == vm for g in gen))
            for pm in (C.POOL_IDENT, C.POOL_EXACT, C.POOL_TABLE, C.POOL_REPEAT):
                need(f"pool mode {pm} {side} {dt}", any(g[2] == pm for g in gen))
            subs = ("quad", "scalar", "stage4", "stage1") if side == "forward" else ("store4", "scalar")
            for sub in subs:
                need(f"sub-branch {sub} {side} {dt}", any(g[3] == sub for g in gen))
            need(f"VEC 1 with 4-wide staging {dt}", side == "backward" or (1, 16, C.POOL_TABLE, "stage4") in gen)
            need(f"VEC 1 with scalar staging {dt}", side == "backward" or (1, 16, C.POOL_TABLE, "stage1") in gen)
        # the wide kernel's misaligned fallback
        need(f"wide fallback {dt}", any(c.dtype == dt and c.off % 16 and C.case_paths(c) == (("generic", 4, 12, C.POOL_REPEAT, None),) * 2
                                        for c in C.CASES))
        # both grid caps exceeded, per kernel class, and the single-row launch
        for entry, kind in (("tail", "lc"), ("tail", "generic"), ("ln", "ln"), ("up", "up")):
            need(f"{kind} beyond both caps {dt}", any(c.dtype == dt and c.entry == entry and C.case_paths(c)[1][0] == kind and
                                                      c.rows > max(C.FWD_CAP_ROWS, C.BWD_CAP_ROWS) and c.rows % 4 for c in C.CASES))
        need(f"wide beyond its caps {dt}", any(c.dtype == dt and C.case_paths(c)[0] == ("wide",) and c.rows % 2 and
                                               C.WIDE_FWD_CAP_ROWS < c.rows for c in C.CASES))
        for kind in ("lc", "generic"):
            need(f"{kind} one row {dt}", any(c.dtype == dt and c.rows == 1 and C.case_paths(c)[0][0] == kind for c in C.CASES))
        # variants of the backward
        for kind in ("ln", "lc", "wide", "generic"):
            need(f"dx_pool NULL {kind} {dt}", any(c.dtype == dt and c.null_dx and C.case_paths(c)[1][0] == kind for c in C.CASES))
            need(f"deferred fold {kind} {dt}", any(c.dtype == dt and c.defer and C.case_paths(c)[1][0] == kind for c in C.CASES))
        need(f"LC<12,48> with dx_add {dt}", any(c.dtype == dt and c.dx_add and C.case_paths(c)[1] == ("lc", 12, 48) for c in C.CASES))
        for flag in (False, True):
            need(f"IDENT dx_add={flag} {dt}", any(c.dtype == dt and c.dx_add == flag and c.rows == 5 and not c.defer and
                                                  C.case_paths(c)[1][:4] == ("generic", 4, 2, C.POOL_IDENT) for c in C.CASES))
        need(f"p_up in (0, 0.25) {dt}", {c.p_up for c in C.CASES if c.dtype == dt and c.entry == "up"} == {0.0, 0.25})
    need("mixed dtype", any(c.mixed and C.case_paths(c) == (("generic", 4, 2, C.POOL_TABLE, "stage4"), ("generic", 4, 2, C.POOL_TABLE, None))
                            for c in C.CASES))
    assert not missing, missing


def test_expected_path_restates_the_host_rules():
    f, b = "spv_spectre_tail_fwd", "spv_spectre_tail_bwd"
    assert C.expected_path(b, 768, 512, "bf16", "bf16", dx_pool_null=True) == ("refused", "dx_pool == NULL")   # k_lc = 768: no LC pair
    assert C.expected_path(b, 512, 100, "bf16", "bf16", dx_pool_null=True) == ("lc", 8, 8)
    assert C.expected_path(b, 768, 3072, "fp32", "fp32", dx_pool_null=True) == ("generic", 4, 3, C.POOL_EXACT, "store4")
    assert C.expected_path(f, 4100, 8, "fp32", "fp32") == C.expected_path(f, 1025, 8, "fp32", "fp32") == ("refused", "row length")
    assert C.expected_path(f, 1022, 8, "fp32", "fp32")[:3] == ("generic", 1, 16)
    assert C.expected_path("spv_spectre_tail_bwd_up", 512, 768, "fp32", "fp32", up=True)[0] == "refused"
    assert C.expected_path("spv_spectre_tail_ln_fwd", 768, 512, "fp32", "fp32")[0] == "refused"
    assert C.expected_path(b, 4096, 1000, "fp32", "fp32") == ("refused", "LDS")
    assert C.pick_cfg(2048) == (4, 12) and C.pick_cfg(3076) == (4, 16) and C.pick_cfg(4100) is None


# ------------------------------------------------------------------------------------------ 3. rounding floors
def _floor(c, run, mode):
    low = C.reference(c, run, mode)
    ref = C.reference(c, run, f3=low["out"], ds=low["ds"]) if c.entry == "ln" else C.exact_reference(c, run)
    return C.errors(c, low, ref)


# the many-row cases are measured once, with dropout on (their float64 references are the slow part of this file)
FLOOR_RUNS = [(c, run) for c in C.CASES for run in ("A", "B") if c.rows <= 5 or run == "B"]


@pytest.mark.parametrize("case,run", FLOOR_RUNS, ids=lambda v: v if isinstance(v, str) else C.case_id(v))
def test_rounding_floor_of_the_reference_stays_inside_the_bars(case, run):
    """fp32 cases: the all-float32 reference within a quarter of each fp32 bar; bf16 cases: the stored tensors rounded once, within
    2^-8 of the row's maximum, everything else exact.  Measured on these inputs: float32 elementwise <= 4.0e-7, column sums
    over 8197 rows <= 3.5e-6; bf16: <= 3.89e-3 per row."""
    errs = _floor(case, run, "fp32" if case.dtype == "fp32" else "bf16")
    for name, e in errs.items():
        if case.dtype == "fp32":
            assert e <= C.bar(case, name) / 4, (C.case_id(case), run, name, e)
        else:
            stored = C.bar(case, name) > C.BF16_HALF_ULP      # a tensor the kernel stores as bf16
            assert e <= (C.BF16_HALF_ULP if stored else 0.0), (C.case_id(case), run, name, e)


def test_bars_are_the_stated_ones():
    fp, bf, mixed = small("tail", dtype="fp32")[0], small("tail", dtype="bf16")[0], small("tail", mixed=True)[0]
    assert [C.bar(fp, k) for k in ("out", "out2", "mean", "rstd2", "dh", "ds", "dx_pool", "dbias", "dgamma2")] == [3e-5] * 4 + [6e-5] * 5
    assert C.bar(bf, "out") == 2.0 ** -8 + 3e-5 and C.bar(bf, "dh") == C.bar(bf, "dx_pool") == C.bar(bf, "ds") == 2.0 ** -8 + 6e-5
    assert [C.bar(bf, k) for k in ("mean", "rstd", "dgamma", "dbeta", "dbias", "dbeta2")] == [3e-5, 3e-5] + [6e-5] * 4
    assert C.bar(mixed, "out") == 3e-5 and C.bar(mixed, "dh") == 2.0 ** -8 + 6e-5


# ------------------------------------------------------------------------------------------ 4. sensitivity
def _swap_halves(keep):
    """the mask with the two 16-bit halves of every hash word exchanged: columns 2j and 2j + 1 swap"""
    r, n = keep.shape
    if n % 2:
        keep = np.concatenate([keep, keep[:, -1:]], axis=1)
    return keep.reshape(r, -1, 2)[:, :, ::-1].reshape(r, -1)[:, :n]


def _shifted_pool(c):
    return np.roll(O.adaptive_pool_matrix(c.k_in, c.n), 1, axis=1)


PERTURBATIONS = {
    # name: (cases it is made on, the reference's arguments it replaces)
    "pooling window shifted by one input": (
        lambda dt: small("tail", dtype=dt, n=768, k_in=3072, dx_add=True) + small("tail", dtype=dt, n=512, k_in=768, mixed=False, null_dx=False, defer=False)
        + small("tail", dtype=dt, n=104) + small("ln", dtype=dt, null_dx=False, defer=False),
        lambda c: dict(P=_shifted_pool(c))),
    "hash halves swapped": (
        lambda dt: small("tail", dtype=dt, n=768, k_in=512) + small("tail", dtype=dt, n=3072, off=0, dx_add=True) + small("tail", dtype=dt, n=10),
        lambda c: dict(keep=_swap_halves(C.keep_mask(c, "B")))),
    "row id offset by one": (
        lambda dt: small("tail", dtype=dt, n=768, k_in=512) + small("tail", dtype=dt, n=64, k_in=64, dx_add=False, defer=False)
        + small("ln", dtype=dt, null_dx=False, defer=False),
        lambda c: dict(keep=D.keep_rows(C.SEED, np.arange(c.rows, dtype=np.uint64) + np.uint64(1), c.n, C.RUNS["B"]["p"]))),
    "inv_keep omitted": (
        lambda dt: small("tail", dtype=dt, n=768, k_in=512) + small("tail", dtype=dt, n=3072, off=0, dx_add=True)
        + small("ln", dtype=dt, null_dx=False, defer=False),
        lambda c: dict(p=0.0)),
    "LayerNorm-2 of f3 without the residual": (
        lambda dt: small("ln", dtype=dt, null_dx=False, defer=False),
        lambda c: dict(x1=np.zeros((c.rows, c.n)))),
    "dx_add dropped": (
        lambda dt: small("tail", dtype=dt, n=768, k_in=3072, dx_add=True) + small("tail", dtype=dt, n=64, k_in=64, dx_add=True)
        + small("up", dtype=dt, dx_add=True),
        lambda c: dict(dx_add=None)),
    "p_up's mask from the layer's own seed": (
        lambda dt: small("up", dtype=dt, p_up=0.25),
        lambda c: dict(up=(C.inputs(c, "B")["up_src"], D.keep(C.SEED, c.rows, 512, c.p_up), c.p_up))),
}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(PERTURBATIONS))
def test_a_wrong_kernel_would_exceed_a_bar(name, dtype):
    """each mistake is made in the reference (run B, dropout on) and must push at least one output of EVERY case it is tried on past
    that output's bar -- if one stays under, the bar or the inputs are too weak"""
    pick, change = PERTURBATIONS[name]
    cases = pick(dtype)
    assert cases, (name, dtype)
    for c in cases:
        wrong = C.reference(c, "B", **change(c))
        errs = C.errors(c, wrong, C.exact_reference(c, "B"))
        over = {k: e for k, e in errs.items() if e > C.bar(c, k)}
        assert over, (name, C.case_id(c), errs)
        assert max(over.values()) > 4 * max(C.bar(c, k) for k in over), (name, C.case_id(c), over)   # not a marginal pass


# ------------------------------------------------------------------------------------------ 5. host refusals
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_entry_points_refuse_on_the_host_before_any_launch(built):
    """fake pointers that are never followed: every call fails validation, nothing is launched (there is no GPU here), the message
    names the function, and the census does not move"""
    from spectre_vit import _native
    FWD, BWD, UP = "spv_spectre_tail_fwd", "spv_spectre_tail_bwd", "spv_spectre_tail_bwd_up"
    LNF, LNB = "spv_spectre_tail_ln_fwd", "spv_spectre_tail_ln_bwd"
    P = 4096   # a non-null, 16-byte aligned "pointer"

    def fwd(n, k, p=0.0, dt=0, odt=0):
        return (P,) * 7 + (5, n, k, dt, odt, p, 0, 0)

    def bwd(n, k, dx_pool=P, h=P, dt=0, ddt=0):
        return (P, h, P, P, P, P, P, dx_pool, P, P, P, P, 5, n, k, dt, ddt, 0.0, 0, 0, 0)

    def up(n, k, src=P, p_up=0.0, dx_pool=P, dt=0, ddt=0):
        return (P,) * 7 + (dx_pool,) + (P,) * 4 + (5, n, k, dt, ddt, 0.0, 0, 0, src, p_up, 0, 0)

    def lnf(n, k, p=0.0, null=None):
        a = [P] * 13
        if null is not None:
            a[null] = 0
        return tuple(a) + (5, n, k, 1, p, 0, 0)

    def lnb(n, k, null=()):
        # dout2, f3, res, mean2, rstd2, gamma2, ds, dgamma2 (7), dbeta2 (8), h, mean, rstd, gamma, beta, dh, dx_pool (15), dgamma (16),
        # dbeta (17), dbias (18), partials
        a = [P] * 20
        for j in null:
            a[j] = 0
        return tuple(a) + (5, n, k, 1, 0.0, 0, 0)

    cases = [
        (FWD, fwd(4100, 512), "row length"), (FWD, fwd(1025, 512), "row length"), (FWD, fwd(768, 512, p=1.0), "p_drop"),
        (FWD, fwd(768, 512, dt=2), "dtype"), (FWD, fwd(0, 512), "empty"),
        (BWD, bwd(4100, 512), "row length"), (BWD, bwd(1025, 512), "row length"),
        # dx_pool == NULL where no kernel honours it: table (the k_lc rule sends 768 <- 512 past the LC list), identity, repeat,
        # VEC 1, the wide shape on a misaligned pointer, and a mixed-dtype call that the LC list refuses
        (BWD, bwd(768, 512, dx_pool=0), "dx_pool"), (BWD, bwd(64, 64, dx_pool=0), "dx_pool"), (BWD, bwd(96, 48, dx_pool=0), "dx_pool"),
        (BWD, bwd(7, 8, dx_pool=0), "dx_pool"), (BWD, bwd(3072, 768, dx_pool=0, h=P + 8), "dx_pool"),
        (BWD, bwd(512, 768, dx_pool=0, dt=1, ddt=0), "dx_pool"),
        (UP, up(512, 768), "unsupported shape"), (UP, up(768, 3072), "unsupported shape"), (UP, up(64, 64), "unsupported shape"),
        (UP, up(768, 512, src=0), "unsupported shape"), (UP, up(768, 512, p_up=1.0), "up_p_drop"),
        (UP, up(768, 512, dt=1, ddt=0), "dtype"),
        (LNF, lnf(768, 512), "unsupported shape"), (LNF, lnf(512, 512), "unsupported shape"), (LNF, lnf(512, 768, p=1.0), "p_drop"),
        (LNF, lnf(512, 768, null=7), "null pointer"),
        (LNB, lnb(768, 512), "unsupported shape"), (LNB, lnb(64, 64), "unsupported shape"), (LNB, lnb(512, 768, null=(6,)), "null pointer"),
        (LNB, lnb(512, 768, null=(19,)), "null pointer"),
        (LNB, lnb(512, 768, null=(16,)), "together"), (LNB, lnb(512, 768, null=(7, 8)), "together"),
        (LNB, lnb(512, 768, null=(16, 17, 18, 7)), "together"),
    ]
    before = {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()}
    for name, args, needle in cases:
        assert len(args) == len(_native.SIGNATURES[name]), name
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, args, needle, str(e.value))
    assert {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()} == before, "a refused call is not counted"
