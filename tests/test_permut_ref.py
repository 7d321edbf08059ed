"""CPU checks behind tests/test_gpu_permut_edges.py: csrc/spv_permut_core.h, compiled by the host compiler into a stand-alone program,
names the same path as tests/permut_edge_cases.py's restatement over a grid that straddles every threshold, and the library's
spv_permut_table_words / spv_permut_pool_supported answer as restated; the case tables stand on both sides of every boundary of every
reachable path; tests/permut_ref.py agrees with the dense signed-permutation matrix (exactly) and with the oracle; a float32
restatement of each kernel passes every bar on every case's own inputs; each of eight plausible mistakes made in that restatement
breaks exactness or exceeds a bar; and the host refuses, before any launch, what no kernel serves."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import permut_edge_cases as C
import permut_ref as R
from oracle import spectre_oracle as O


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


CORE_MAIN = r"""
#include "spv_permut_core.h"
#include <stdio.h>
#include <string.h>
// stdin, one query per line; stdout, one answer per line.
// "f dtype heads d batch pooled pw x16 g16 idx16" / "b dtype heads d batch dg16 dx16 idx16" / "r dtype batch d n embed a16 b16" (row-0
// forward) / "s ..." (row-0 backward): the path's name.  "g heads d": table words, compact_ok, long_row, scat_parts, scat_len,
// scat_set_words.  "p heads d pw dtype": pool_supported.
int main() {
    char what[4];
    long long a[9];
    while (scanf("%3s", what) == 1) {
        const int n = what[0] == 'f' ? 9 : what[0] == 'b' ? 7 : (what[0] == 'r' || what[0] == 's') ? 7 : what[0] == 'g' ? 2 : what[0] == 'p' ? 4 : -1;
        if (n < 0) return 2;
        for (int i = 0; i < n; ++i)
            if (scanf("%lld", &a[i]) != 1) return 1;
        switch (what[0]) {
        case 'f': puts(permut_path_name(permut_fwd_path((int)a[0], (int)a[1], (int)a[2], (int)a[3], a[4] != 0, (int)a[5], a[6] != 0, a[7] != 0, a[8] != 0))); break;
        case 'b': puts(permut_path_name(permut_bwd_path((int)a[0], (int)a[1], (int)a[2], (int)a[3], a[4] != 0, a[5] != 0, a[6] != 0))); break;
        case 'r': puts(permut_path_name(permut_row0_fwd_path((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], a[5] != 0, a[6] != 0))); break;
        case 's': puts(permut_path_name(permut_row0_bwd_path((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], a[5] != 0, a[6] != 0))); break;
        case 'g': printf("%lld %d %d %d %d %lld\n", (long long)permut_table_words((int)a[0], (int)a[1]), (int)compact_ok((int)a[1]), (int)long_row((int)a[1]),
                         scat_parts((int)a[1]), scat_len((int)a[1]), (long long)scat_set_words((int)a[0], (int)a[1])); break;
        case 'p': printf("%d\n", permut_pool_supported((int)a[0], (int)a[1], (int)a[2], (int)a[3])); break;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """the compiled header: core(lines) -> the program's output lines"""
    from conftest import ROOT
    csrc = os.path.join(ROOT, "vit-spectre-experiments_amd", "csrc")
    d = tmp_path_factory.mktemp("permut_core")
    src, exe = d / "core_main.cpp", d / "core_main"
    src.write_text(CORE_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=300)
        got = out.stdout.split("\n")[:-1]
        assert len(got) == len(lines)
        return got
    return run


DT_GRID = (("fp32", 0), ("bf16", 1), ("int8", 2))
FLAGS3 = list(itertools.product((True, False), repeat=3))
FLAGS2 = list(itertools.product((True, False), repeat=2))


def fwd_grid():
    """(dtype name, code, heads, d, batch, pooled, pw, x16, g16, idx16): every d of the grid with every window and every head / batch
    count that changes a rule; the alignment flags in all eight combinations without pooled and at two windows"""
    for (dt, code), d in itertools.product(DT_GRID, C.D_GRID):
        for heads, batch in ((1, 1), (2, 3), (3, 2), (16, 257), (65535, 1), (65536, 1), (2, 65535), (2, 65536), (0, 1), (1, 0)):
            for pw in C.PW_GRID:
                for fl in (FLAGS3 if pw in (0, 8, 12) else FLAGS3[:1]):
                    yield (dt, code, heads, d, batch, pw > 0, pw) + fl
    yield ("bf16", 1, 2, 0, 2, False, 0, True, True, True)
    yield ("bf16", 1, 2, 2048, 2, True, 0, True, True, True)      # pooled given, window 0
    yield ("bf16", 1, 2, 2048, 2, True, -8, True, True, True)


def bwd_grid():
    for (dt, code), d, fl in itertools.product(DT_GRID, C.D_GRID, FLAGS3):
        for heads, batch in ((1, 1), (2, 3), (3, 513), (16, 257), (65536, 1), (2, 65536), (0, 1), (1, 0)):
            yield (dt, code, heads, d, batch) + fl
    yield ("bf16", 1, 2, 0, 2, True, True, True)


def row0_grid():
    for (dt, code), d, fl in itertools.product(DT_GRID, C.D_GRID, FLAGS2):
        for batch in (1, 3, 0):
            for n, embed in ((1, 1), (d, d), (max(d - 1, 1), 8), (8, d), (d + 1, 8), (8, d + 1), (0, 8), (8, 0), (4, 4), (1000, 12), (16, 1024)):
                yield (dt, code, batch, d, n, embed) + fl
    yield ("bf16", 1, 1, 0, 1, 1, True, True)


def _line(tag, q):
    return tag + " " + " ".join(str(int(v)) for v in q[1:])


# ------------------------------------------------------------------------------------------ 1. dispatch
def test_compiled_selectors_equal_the_restatement(core):
    seen = set()
    for tag, grid, fn in (("f", fwd_grid, C.fwd_path), ("b", bwd_grid, C.bwd_path), ("r", row0_grid, C.row0_fwd_path), ("s", row0_grid, C.row0_bwd_path)):
        qs = list(grid())
        got = core([_line(tag, q) for q in qs])
        for q, g in zip(qs, got):
            want = fn(q[0], *q[2:])
            assert g == want, (tag, q, g, want)
            seen.add(g)
    # the grid is not blind: it reaches every path and every refusal the header names
    assert seen == set(C.KERNEL_PATHS) | {"refuse_empty", "refuse_dtype", "refuse_pool_lds", "refuse_pool_window", "refuse_pool_unserved", "refuse_row0_shape"}, seen


def geometry_grid():
    return [(h, d) for d in C.D_GRID for h in (1, 2, 3, 16)]


def test_compiled_geometry_equals_the_restatement(core):
    qs = geometry_grid()
    for (h, d), line in zip(qs, core([f"g {h} {d}" for h, d in qs])):
        want = (C.table_words(h, d), int(C.compact_ok(d)), int(C.long_row(d)), C.scat_parts(d), C.scat_len(d), C.scat_set_words(h, d))
        assert tuple(int(v) for v in line.split()) == want, (h, d, line, want)
        if C.long_row(d):   # what the kernels lean on: a part's accumulators fit the LDS, its targets 16 bits, the parts cover the row
            assert C.scat_len(d) * 4 <= C.LDS_LIMIT and C.scat_len(d) <= 65536 and C.scat_len(d) * C.scat_parts(d) >= d > C.scat_len(d) * (C.scat_parts(d) - 1)
    ps = [(h, d, pw, code) for d in C.D_GRID for h in (1, 3, 65535, 65536) for pw in C.PW_GRID + (-4,) for _, code in DT_GRID]
    for (h, d, pw, code), line in zip(ps, core([f"p {h} {d} {pw} {code}" for h, d, pw, code in ps])):
        assert int(line) == C.pool_supported(h, d, pw, {0: "fp32", 1: "bf16"}.get(code, "int8")), (h, d, pw, code)


def test_library_answers_equal_the_restatement(built):
    from spectre_vit import _native as nat
    for h, d in geometry_grid():
        assert nat.call("spv_permut_table_words", h, d) == C.table_words(h, d), (h, d)
        for pw in C.PW_GRID + (-4,):
            for dt, code in DT_GRID:
                assert nat.call("spv_permut_pool_supported", h, d, pw, code) == C.pool_supported(h, d, pw, dt), (h, d, pw, dt)
    assert nat.call("spv_permut_pool_supported", 65536, 151296, 12, 1) == 0 and nat.call("spv_permut_pool_supported", 65535, 151296, 12, 1) == 1


def test_pool_supported_answers_only_for_what_the_forward_honours():
    """wherever spv_permut_pool_supported says 1, the forward -- with aligned pointers and a batch the grid takes -- emits pooled on
    the scatter kernel; PermutMixFn's own LDS-path rule likewise lands on a kernel that emits it"""
    for d in C.D_GRID:
        for h in (1, 2, 3, 16, 65535, 65536):
            for pw in C.PW_GRID[1:]:
                if C.pool_supported(h, d, pw, "bf16"):
                    assert C.fwd_path("bf16", h, d, 2, True, pw) == "fwd_scatter", (h, d, pw)
                for dt in C.DTYPES:
                    es, total = C.ES[dt], h * d
                    if pw in C.WINDOWS and (d * es) % 16 == 0 and d * es <= 150 * 1024 and (total // 4) % 1024 == 0 and total % pw == 0:   # hip_ops.PermutMixFn
                        assert C.fwd_path(dt, h, d, 2, True, pw) in ("fwd_pair", "fwd_lds"), (dt, h, d, pw)


# ------------------------------------------------------------------------------------------ 2. coverage
def test_tables_stand_on_both_sides_of_every_boundary():
    missing = []
    for family, want, path in C.BOUNDARIES:
        hits = [c for c in C.ALL[family] if C.matches(c, want) and (path is None or C.path_of(family, c) == path)]
        if not hits:
            missing.append((family, want, path))
    assert not missing, missing


def test_every_reachable_path_has_a_case():
    """reachable: named by the restatement somewhere on the selector grid.  Every such kernel has a case; every forward kernel that
    can emit pooled has one with and one without; window 32 runs on both kernels whose lanes share a window."""
    reach = {C.fwd_path(q[0], *q[2:]) for q in fwd_grid()} | {C.bwd_path(q[0], *q[2:]) for q in bwd_grid()}
    for q in row0_grid():
        reach |= {C.row0_fwd_path(q[0], *q[2:]), C.row0_bwd_path(q[0], *q[2:])}
    reach = {p for p in reach if not p.startswith("refuse")}
    assert reach == set(C.KERNEL_PATHS)
    have = {(C.fwd_case_path(c), c.dtype, c.pw > 0) for c in C.FWD_CASES} | {(C.bwd_case_path(c), c.dtype, False) for c in C.BWD_CASES}
    for c in C.ROW0_CASES:
        have |= {(p, c.dtype, False) for p in C.row0_case_paths(c)}
    have |= {(C.row0_case_paths(c)[0], c.dtype, False) for c in C.ROW0_FWD_ONLY}
    bf_only = {"fwd_pair", "fwd_scatter", "bwd_dma", "bwd_c16", "bwd_scatter", "bwd_parts"}
    for p in sorted(reach):
        for dt in C.DTYPES:
            if dt == "fp32" and p in bf_only or dt == "bf16" and p == "bwd_lds":
                assert not any(k[0] == p and k[1] == dt for k in have)
                continue
            assert (p, dt, False) in have, (p, dt)
            if p in C.POOLING_PATHS:
                assert (p, dt, True) in have, (p, dt, "pooled")
    for p, dt in (("fwd_pair", "bf16"), ("fwd_lds", "bf16"), ("fwd_lds", "fp32")):
        for pw in (C.WINDOWS[1:] if p == "fwd_pair" else C.WINDOWS):
            assert any(C.fwd_case_path(c) == p and c.dtype == dt and c.pw == pw for c in C.FWD_CASES), (p, dt, pw)
    # no case is refused, every refusal case is; every permutation / sign kind runs on the forward and the backward
    for c in C.FWD_CASES:
        assert not C.fwd_case_path(c).startswith("refuse"), c
    for c, why in C.FWD_REFUSED:
        assert C.fwd_case_path(c) == why, (c, C.fwd_case_path(c))
    for cases in (C.FWD_CASES, C.BWD_CASES, C.PACK_CASES):
        assert {c.perm for c in cases} == {"rand", "id", "rev"} and {c.sign for c in cases} == {"rand", "pos", "neg"}
    assert {c.d for c in C.PACK_CASES} == {8, 12, 65536, 65544, 76800, 76808, 115200, 115208, 151296} and {c.heads for c in C.PACK_CASES} == {1, 2, 3}
    # the limits: nothing above d = 151 296 x heads 2 x batch 2 elements
    for c in C.FWD_CASES + C.BWD_CASES:
        assert c.batch * c.heads * c.d <= 2 * 2 * 151296, c


def test_parts_kernels_beyond_one_part_are_unreachable():
    """what the removed code served: the forward parts kernel ran only with heads or batch above 65 535 on a long row (tables of tens of
    GB; now the global kernel), the bf16 wide-table LDS backward never, and the backward parts kernel only on rows that fit the LDS
    whole -- one part"""
    for q in bwd_grid():
        if C.bwd_path(q[0], *q[2:]) == "bwd_parts":
            assert 40960 < q[3] <= 76800 and q[3] * 2 <= C.LDS_LIMIT and q[0] == "bf16", q
        if C.bwd_path(q[0], *q[2:]) == "bwd_lds":
            assert q[0] == "fp32", q
    n = 0
    for q in fwd_grid():
        dt, _, heads, d, batch, pooled, pw, x16, g16, i16 = q
        if C.fwd_path(dt, heads, d, batch, pooled, pw, x16, g16, i16) == "fwd_global" and dt == "bf16" and d % 8 == 0 and x16 and g16 and i16:
            assert C.long_row(d) and (heads > 65535 or batch > 65535), q     # all the forward parts kernel ever served
            assert batch > 65535 or C.table_words(heads, d) * 4 > 2 ** 30, q
            n += 1
    assert n > 0


# ------------------------------------------------------------------------------------------ 3. the references
@pytest.mark.parametrize("heads,d,kind", [(1, 1, "rand"), (2, 5, "rand"), (3, 8, "rand"), (3, 12, "id"), (2, 12, "rev"), (16, 7, "rand")])
def test_references_equal_the_dense_signed_permutation_product(heads, d, kind):
    rng = np.random.default_rng(heads * 100 + d)
    perms, signs = C.perms_signs(rng, heads, d, kind)
    P = R.dense(perms, signs)
    x, dg = rng.integers(-8, 9, (3, d)).astype(np.float64), rng.integers(-8, 9, (3, heads * d)).astype(np.float64)   # small integers: exact
    g = R.gather_fwd(x, perms, signs)
    assert np.array_equal(g, np.einsum("hji,bi->bhj", P, x).reshape(3, -1))
    dx, ab = R.gather_bwd(dg, perms, signs)
    assert np.array_equal(dx, np.einsum("hji,bhj->bi", P, dg.reshape(3, heads, d)))
    assert np.array_equal(ab, np.einsum("hji,bhj->bi", np.abs(P), np.abs(dg.reshape(3, heads, d))))
    # <g, dg> = <x, dx>: the backward is the forward's adjoint
    assert (g * dg).sum() == (x * dx).sum()
    if heads * d % 4 == 0:
        _, pooled, ab = R.gather_fwd(x, perms, signs, 4)
        assert np.array_equal(pooled, g.reshape(3, -1, 4).mean(-1)) and np.array_equal(ab, np.abs(g).reshape(3, -1, 4).sum(-1))
    # the tables are the same statement: the inverse table undoes the forward one, sign for sign
    fwd, inv = R.wide_tables(perms, signs)
    for h in range(heads):
        assert np.array_equal(inv[h][fwd[h] & 0x7fffffff] & 0x7fffffff, np.arange(d)) and np.array_equal(inv[h][fwd[h] & 0x7fffffff] >> 31, fwd[h] >> 31)
        assert np.array_equal(fwd[h] >> 31, (signs[h] < 0).astype(np.uint32))
    # row 0: the first n entries of head 0
    n, embed = min(d, 3), min(d, 2)
    g0, x0 = R.row0_fwd(x, perms[0], signs[0], n, embed)
    assert np.array_equal(g0, g[:, :n]) and np.array_equal(x0, x[:, :embed])
    dg0, dx0 = dg[:, :n], dg[:, n:n + embed] if heads * d >= n + embed else x[:, :embed]
    full = np.zeros((3, heads * d))
    full[:, :n] = dg0
    want = R.gather_bwd(full, perms, signs)[0]
    want[:, :dx0.shape[1]] += dx0
    assert np.array_equal(R.row0_bwd(dg0, dx0, perms[0], signs[0], d)[0], want)


def test_references_equal_the_oracle():
    rng = np.random.default_rng(7)
    B, N, E, H = 3, 5, 8, 4
    perms, signs = C.perms_signs(rng, H, N * E)
    x, dg = rng.standard_normal((B, N, E)), rng.standard_normal((B, N, E * H))
    assert np.array_equal(R.gather_fwd(x.reshape(B, -1), perms, signs), O.permut_gather_fwd(x, perms, signs.astype(np.float64)).reshape(B, -1))
    got = R.gather_bwd(dg.reshape(B, -1), perms, signs)[0]
    assert np.abs(got - O.permut_gather_bwd(dg, perms, signs.astype(np.float64), N, E).reshape(B, -1)).max() <= 1e-14


def test_pack_reference_is_self_consistent():
    """compact tables hold the wide ones' bits; the scatter lists hold every source once, in the part its target lies in"""
    for c in C.PACK_CASES:
        perms, signs = C.pack_inputs(c)
        fwd, inv = R.wide_tables(perms, signs)
        lay = R.table_layout(c.heads, c.d)
        assert ("compact" in lay) == C.compact_ok(c.d) and ("scat0" in lay) == ("scat1" in lay) == C.long_row(c.d), c
        if C.compact_ok(c.d):
            i16, sg = R.compact_tables(fwd)
            assert np.array_equal(i16.astype(np.uint32) | (np.unpackbits(sg, bitorder="little").astype(np.uint32) << 31), fwd.reshape(-1))
        if C.long_row(c.d):
            L = C.scat_len(c.d)
            for wide in (fwd, inv):
                off, lists = R.scatter_lists(wide)
                assert (off[:, 0] == 0).all() and (off[:, -1] == c.d).all()
                for h in range(c.heads):
                    src = np.concatenate([(lists[(h, q)] >> np.uint64(16)) & np.uint64(0x7fffffff) for q in range(C.scat_parts(c.d))])
                    assert np.array_equal(np.sort(src), np.arange(c.d))
                    for q in range(C.scat_parts(c.d)):
                        e = lists[(h, q)]
                        assert len(e) == off[h, q + 1] - off[h, q]
                        s, t = ((e >> np.uint64(16)) & np.uint64(0x7fffffff)).astype(np.int64), (e & np.uint64(0xffff)).astype(np.int64)
                        assert np.array_equal(wide[h][s] & 0x7fffffff, t + q * L) and np.array_equal(wide[h][s] >> 31, (e >> np.uint64(47)).astype(np.uint32))


# ------------------------------------------------------------------------------------------ 4. the float32 restatement passes every bar
def _fwd_check(c, got_g, got_pooled, perms, signs, x):
    """(exact, pooled within its bar, worst ratio) of a forward result against the float64 reference"""
    if c.pw:
        g, pooled, ab = R.gather_fwd(x, perms, signs, c.pw)
        ok, worst = C.worst_ratio(got_pooled, pooled, C.pooled_bar(pooled, ab, c.pw, c.dtype))
    else:
        g, ok, worst = R.gather_fwd(x, perms, signs), True, 0.0
    return np.array_equal(C.bits(got_g, c.dtype), C.bits(g, c.dtype)), ok, worst


def test_float32_restatement_passes_every_bar_on_every_case():
    worst = {}
    for c in C.FWD_CASES:
        perms, signs, x = C.fwd_inputs(c)
        fwd, inv = R.wide_tables(perms, signs)
        out = R.emulate_fwd(x, fwd, inv, c.dtype, c.pw)
        exact, ok, w = _fwd_check(c, out[0] if c.pw else out, out[1] if c.pw else None, perms, signs, x)
        assert exact and ok, (c, w)
        worst["pooled"] = max(worst.get("pooled", 0.0), w)
    for c in C.BWD_CASES:
        perms, signs, dg = C.bwd_inputs(c)
        dx, ab = R.gather_bwd(dg, perms, signs)
        ok, w = C.worst_ratio(R.emulate_bwd(dg, R.wide_tables(perms, signs)[1], c.dtype), dx, C.dx_bar(dx, ab, c.heads, c.dtype))
        assert ok, (c, w)
        worst["dx"] = max(worst.get("dx", 0.0), w)
    for c in C.ROW0_CASES + C.ROW0_FWD_ONLY:
        perms, signs, x, dg0, dx0 = C.row0_inputs(c)
        fwd0 = R.wide_tables(perms, signs)[0][0]
        g0, x0 = R.row0_fwd(x, perms[0], signs[0], c.n, c.embed)
        e_g0, e_x0 = R.emulate_row0_fwd(x, fwd0, c.n, c.embed, c.dtype)
        assert np.array_equal(C.bits(e_g0, c.dtype), C.bits(g0, c.dtype)) and np.array_equal(C.bits(e_x0, c.dtype), C.bits(x0, c.dtype)), c
        if c in C.ROW0_CASES:
            dx, a, s = R.row0_bwd(dg0, dx0, perms[0], signs[0], c.d)
            ok, w = C.worst_ratio(R.emulate_row0_bwd(dg0, dx0, fwd0, c.d, c.dtype), dx, C.row0_dx_bar(dx, a, s, c.dtype))
            assert ok, (c, w)
            worst["row0_dx"] = max(worst.get("row0_dx", 0.0), w)
    print("PERMUT float32 restatement, worst ratio to the bar: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(0 < v <= 1 for v in worst.values()), worst   # the bars are used, not idle


def test_inputs_carry_every_planted_value():
    for c in (C.Fwd("bf16", 2, 2, 2048, 32), C.Fwd("fp32", 2, 2, 2048, 32), C.Bwd("bf16", 2, 3, 520), C.Bwd("fp32", 2, 2, 38404)):
        a = (C.fwd_inputs(c) if isinstance(c, C.Fwd) else C.bwd_inputs(c))[2]
        w = C.bits(a, c.dtype).astype(np.uint32) << (16 if c.dtype == "bf16" else 0)
        for pat in (0x00000000, 0x80000000, 0x7f800000, 0xff800000):     # +-0, +-inf
            assert (w == pat).sum() == 1, (c, hex(pat))
        sub = (w & 0x7f800000 == 0) & (w & 0x007fffff != 0)
        assert sub.sum() == 2 and (a == C.HUGE[c.dtype]).sum() == 1 and not np.isnan(a).any(), c
        assert np.array_equal(C.storage_round(a, c.dtype)[np.isfinite(a)], a[np.isfinite(a)])


# ------------------------------------------------------------------------------------------ 5. the mistakes
def _case(cases, **want):
    return next(c for c in cases if C.matches(c, want))


def test_a_dropped_sign_bit_breaks_exactness():
    for c in (_case(C.FWD_CASES, dtype="bf16", d=38400, batch=3), _case(C.FWD_CASES, dtype="fp32", d=4, heads=16), _case(C.FWD_CASES, d=151296, pw=0)):
        perms, signs, x = C.fwd_inputs(c)
        fwd, inv = R.wide_tables(perms, signs)
        assert not _fwd_check(c, R.emulate_fwd(x, fwd, inv, c.dtype, 0, "sign"), None, perms, signs, x)[0], c


def test_the_inverse_table_in_place_of_the_forward_breaks_exactness():
    for c in (_case(C.FWD_CASES, dtype="bf16", d=8, heads=16), _case(C.FWD_CASES, dtype="fp32", d=38400), _case(C.FWD_CASES, d=115208)):
        assert c.perm == "rand"   # the identity and the reversal are their own inverses: only a random permutation tells
        perms, signs, x = C.fwd_inputs(c)
        fwd, inv = R.wide_tables(perms, signs)
        assert not _fwd_check(c, R.emulate_fwd(x, fwd, inv, c.dtype, 0, "inverse"), None, perms, signs, x)[0], c
    for c in (_case(C.BWD_CASES, dtype="bf16", d=512, batch=2), _case(C.BWD_CASES, dtype="fp32", d=38400)):
        perms, signs, dg = C.bwd_inputs(c)
        dx, ab = R.gather_bwd(dg, perms, signs)
        assert not C.worst_ratio(R.emulate_bwd(dg, R.wide_tables(perms, signs)[0], c.dtype), dx, C.dx_bar(dx, ab, c.heads, c.dtype))[0], c


def test_a_skipped_last_piece_of_the_row_breaks_exactness():
    for c in (_case(C.FWD_CASES, dtype="bf16", d=38408, off=""), _case(C.FWD_CASES, dtype="bf16", d=8, batch=1, heads=1), _case(C.FWD_CASES, dtype="fp32", d=4, heads=1),
              _case(C.FWD_CASES, dtype="fp32", d=38400), _case(C.FWD_CASES, dtype="bf16", d=76800)):
        perms, signs, x = C.fwd_inputs(c)
        fwd, inv = R.wide_tables(perms, signs)
        assert not _fwd_check(c, R.emulate_fwd(x, fwd, inv, c.dtype, 0, "last_piece"), None, perms, signs, x)[0], c


def test_window_32_from_the_wrong_quads_exceeds_the_pooled_bar():
    n = 0
    for c in C.FWD_CASES:
        if c.pw == 32 and C.fwd_case_path(c) == "fwd_lds":
            perms, signs, x = C.fwd_inputs(c)
            fwd, inv = R.wide_tables(perms, signs)
            g, pooled = R.emulate_fwd(x, fwd, inv, c.dtype, 32, "ror")
            exact, ok, w = _fwd_check(c, g, pooled, perms, signs, x)
            assert exact and not ok and w > 10, (c, w)     # g is untouched; the averages are other windows' by O(1)
            n += 1
    assert n >= 4


def test_the_second_sample_from_the_first_samples_row_breaks_exactness():
    for c in C.FWD_CASES:
        if C.fwd_case_path(c) == "fwd_pair" and c.batch >= 2:
            perms, signs, x = C.fwd_inputs(c)
            fwd, inv = R.wide_tables(perms, signs)
            out = R.emulate_fwd(x, fwd, inv, c.dtype, c.pw, "pair")
            exact, ok, _ = _fwd_check(c, out[0] if c.pw else out, out[1] if c.pw else None, perms, signs, x)
            assert not exact and (not c.pw or not ok), c


def test_a_scatter_part_boundary_off_by_8_breaks_exactness():
    for c in C.FWD_CASES:
        if C.fwd_case_path(c) == "fwd_scatter":
            perms, signs, x = C.fwd_inputs(c)
            fwd, inv = R.wide_tables(perms, signs)
            out = R.emulate_fwd(x, fwd, inv, c.dtype, c.pw, "part")
            exact, ok, _ = _fwd_check(c, out[0] if c.pw else out, out[1] if c.pw else None, perms, signs, x)
            assert not exact and (not c.pw or not ok), c


def test_x0_unwritten_from_n_on_is_seen():
    n = 0
    for c in C.ROW0_CASES + C.ROW0_FWD_ONLY:
        if c.n < c.embed:
            perms, signs, x, _, _ = C.row0_inputs(c)
            _, x0 = R.emulate_row0_fwd(x, R.wide_tables(perms, signs)[0][0], c.n, c.embed, c.dtype, "x0")
            assert np.isnan(x0).sum() == c.batch * (c.embed - c.n), c     # the GPU test's "every output element is written"
            n += "row0_fwd_global" == C.row0_case_paths(c)[0]
    assert n >= 4      # on the kernel that made the mistake, in both dtypes, by shape and by alignment


def test_a_head_left_out_of_the_backward_sum_exceeds_the_dx_bar():
    for c in C.BWD_CASES:
        if c.heads == 1:
            continue
        perms, signs, dg = C.bwd_inputs(c)
        dx, ab = R.gather_bwd(dg, perms, signs)
        ok, w = C.worst_ratio(R.emulate_bwd(dg, R.wide_tables(perms, signs)[1], c.dtype, "head"), dx, C.dx_bar(dx, ab, c.heads, c.dtype))
        assert not ok and w > 1, (c, w)


# ------------------------------------------------------------------------------------------ 6. host refusals
def test_entry_points_refuse_on_the_host_before_any_launch(built):
    """fake pointers that are never followed: every call fails validation, nothing is launched (there is no GPU here), the message
    names the function, and the census does not move"""
    from spectre_vit import _native
    P, Q = 4096, 4096 + 8   # non-null "pointers": 16-byte aligned, and 8 bytes off

    def fwd(x=P, g=P, pooled=0, pw=0, b=2, h=2, d=2048, dt=1, idx=P):
        return (x, idx, g, pooled, pw, b, h, d, dt, 0)

    def bwd(b=2, h=2, d=2048, dt=1):
        return (P, P, P, b, h, d, dt, 0)

    def r0(b=2, d=2048, n=16, e=8, dt=1):
        return (P, P, P, P, b, d, n, e, dt, 0)

    cases = [
        ("spv_permut_gather_fwd", fwd(b=0), "empty"), ("spv_permut_gather_fwd", fwd(h=0), "empty"), ("spv_permut_gather_fwd", fwd(d=0), "empty"),
        ("spv_permut_gather_fwd", fwd(dt=2), "dtype"),
        # pooled off the LDS path: a row that is not whole 16-byte pieces, a row over the LDS, a long row whose quarters the window does not divide
        ("spv_permut_gather_fwd", fwd(pooled=P, pw=4, d=2052), "LDS path"), ("spv_permut_gather_fwd", fwd(pooled=P, pw=4, d=38404, dt=0), "LDS path"),
        ("spv_permut_gather_fwd", fwd(pooled=P, pw=256, d=151296), "LDS path"), ("spv_permut_gather_fwd", fwd(pooled=P, pw=8, d=151296, dt=0), "LDS path"),
        ("spv_permut_gather_fwd", fwd(pooled=P, pw=64), "window"), ("spv_permut_gather_fwd", fwd(pooled=P, pw=12), "window"),
        ("spv_permut_gather_fwd", fwd(pooled=P, pw=0), "window"), ("spv_permut_gather_fwd", fwd(pooled=P, pw=8, d=2056), "window"),
        # this pull request's: pooled is written or the call fails
        ("spv_permut_gather_fwd", fwd(x=Q, pooled=P, pw=16), "aligned"), ("spv_permut_gather_fwd", fwd(g=Q, pooled=P, pw=16), "aligned"),
        ("spv_permut_gather_fwd", fwd(idx=Q, pooled=P, pw=16), "aligned"), ("spv_permut_gather_fwd", fwd(g=Q, pooled=P, pw=32, dt=0), "aligned"),
        ("spv_permut_gather_fwd", fwd(x=Q, pooled=P, pw=12, d=151296), "aligned"), ("spv_permut_gather_fwd", fwd(g=Q, pooled=P, pw=12, d=151296), "aligned"),
        ("spv_permut_gather_fwd", fwd(pooled=P, pw=4, d=76804, h=1), "d % 8"), ("spv_permut_gather_fwd", fwd(pooled=P, pw=12, d=151296, b=65536), "65535"),
        ("spv_permut_gather_bwd", bwd(b=0), "empty"), ("spv_permut_gather_bwd", bwd(h=0), "empty"), ("spv_permut_gather_bwd", bwd(d=0), "empty"),
        ("spv_permut_gather_bwd", bwd(dt=3), "dtype"),
        ("spv_permut_pack", (P, P, P, 0, 8, 0), "empty"), ("spv_permut_pack", (P, P, P, 2, 0, 0), "empty"),
    ]
    for name in ("spv_permut_row0_fwd", "spv_permut_row0_bwd"):
        cases += [(name, r0(b=0), "batch=0"), (name, r0(n=0), "n=0"), (name, r0(n=2049), "n=2049"), (name, r0(e=0), "embed=0"), (name, r0(e=2056), "embed=2056"),
                  (name, r0(d=0), "d=0"), (name, r0(dt=2), "dtype")]
    cases += [("spv_permut_row0_bwd", r0(d=2052), "multiples of 8"), ("spv_permut_row0_bwd", r0(e=12), "multiples of 8"),
              ("spv_permut_row0_bwd", r0(d=2044, e=4, dt=0), "multiples of 8")]
    before = {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()}
    for name, args, needle in cases:
        assert len(args) == len(_native.SIGNATURES[name]), name
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (name, args, needle, str(e.value))
    assert {k: _native.call("spv_path_count", v) for k, v in _native.PATH.items()} == before, "a refused call is not counted"
    # the restated rules name the same refusals
    assert C.fwd_path("bf16", 2, 2048, 2, True, 16, x16=False) == C.fwd_path("bf16", 1, 76804, 2, True, 4) == "refuse_pool_unserved"
    assert C.fwd_path("bf16", 2, 151296, 2, True, 256) == "refuse_pool_lds" and C.fwd_path("bf16", 2, 2048, 2, True, 64) == "refuse_pool_window"
    assert C.row0_bwd_path("bf16", 2, 2052, 16, 8) == C.row0_fwd_path("bf16", 2, 2048, 2049, 8) == "refuse_row0_shape"
