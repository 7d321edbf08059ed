"""CPU checks behind tests/test_gpu_gemm_edges.py: csrc/spv_gemm_core.h, compiled by the host compiler into a stand-alone program,
answers as tests/gemm_edge_cases.py's restatement over a grid that straddles every threshold the dispatch names; every shape in the
case tables selects the kernel its table claims, and the tables reach all twelve strip instantiations and every TN form; the integer
input set is exact in float32 for every case that runs it; a float32 restatement of each kernel (the same K order in chunks, the same
slab sums, one rounding at the store) meets every bar on every case's own inputs; and each of eleven plausible mistakes made in that
restatement is caught on at least one shipped case."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import dropout_ref as D
import gemm_edge_cases as C
import gemm_ref as R

CORE_MAIN = r"""
#include "spv_gemm_core.h"
#include <stdio.h>
// stdin, one query per line; stdout, one answer per line.
// "s M N K reserved": strip_plan.  "n <22 ints>": gemm_nt_plan, the fields of GemmNtCall in order.  "t <12 ints>": gemm_tn_plan, its
// arguments in order.  "b null nprob listed K splits ws_lo fold_blocks" then 9 ints per listed problem: gemm_tn_batch_plan.
int main() {
    char what[4];
    long long a[32];
    while (scanf("%3s", what) == 1) {
        const int n = what[0] == 's' ? 4 : what[0] == 'n' ? 22 : what[0] == 't' ? 12 : what[0] == 'b' ? 7 : -1;
        if (n < 0) return 2;
        for (int i = 0; i < n; ++i)
            if (scanf("%lld", &a[i]) != 1) return 1;
        if (what[0] == 's') {
            int mb = 0, nstrips = 0, groups = 0, base = 0, rem = 0;
            const bool ok = strip_plan((int)a[0], (int)a[1], (int)a[2], (int)a[3], mb, nstrips, groups, base, rem);
            if (ok) printf("1 %d %d %d %d %d\n", mb, nstrips, groups, base, rem);
            else puts("0");
        } else if (what[0] == 'n') {
            GemmNtCall c{};
            int* f = &c.in_dtype;
            static_assert(sizeof(GemmNtCall) == 22 * sizeof(int), "GemmNtCall is 22 ints");
            for (int i = 0; i < 22; ++i) f[i] = (int)a[i];
            const GemmNtPlan p = gemm_nt_plan(c);
            printf("%s %d %d %d %d %d %d %d %d %d %d %d\n", gemm_nt_kernel_name(p.kernel), p.splits, p.k_per_split, p.grid, p.mb, p.epi, p.nstrips, p.groups,
                   p.base, p.rem, p.reduce, p.reduce_blocks);
        } else if (what[0] == 't') {
            const GemmTnPlan p = gemm_tn_plan((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[8], (int)a[9],
                                              (int)a[10], (int)a[11]);
            printf("%s %d %d %d %d %d\n", gemm_tn_kernel_name(p.kernel), (int)p.reduce, p.splits, p.k_per_split, p.grid, p.reduce_blocks);
        } else {
            GemmTnBatchProblem q[16];
            const int nprob = (int)a[1], listed = (int)a[2];
            if (listed > 16) return 3;
            for (int i = 0; i < listed; ++i) {
                long long v[9];
                for (int j = 0; j < 9; ++j)
                    if (scanf("%lld", &v[j]) != 1) return 1;
                q[i] = {(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8]};
            }
            const GemmTnBatchPlan p = gemm_tn_batch_plan(a[0] ? nullptr : q, nprob, (int)a[3], (int)a[4], (int)a[5], (int)a[6]);
            printf("%s %d", gemm_tnb_kernel_name(p.kernel), p.bad);
            if (p.kernel >= GEMM_TNB_128) {
                printf(" %d %d %d", p.splits, p.k_per_split, p.nlong);
                for (int i = 0; i < nprob; ++i) printf(" %d", p.order[i]);
                for (int i = 0; i <= nprob; ++i) printf(" %d", p.first_tile[i]);
                for (int i = 0; i <= nprob; ++i) printf(" %d", p.wide_first_tile[i]);
                for (int i = 0; i < nprob; ++i) printf(" %lld", p.ws_off[i]);
                printf(" %d %d", p.grid, p.reduce_blocks);
            }
            puts("");
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
    d = tmp_path_factory.mktemp("gemm_core")
    src, exe = d / "core_main.cpp", d / "core_main"
    src.write_text(CORE_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=300)
        got = out.stdout.split("\n")[:-1]
        assert len(got) == len(lines)
        return got
    return run


def around(*xs, steps=(1, 8)):
    return sorted({x + s * d for x in xs for d in steps for s in (-1, 1)} | set(xs))


# --------------------------------------------------------------------------------------------------------------- 1. dispatch
NT_FIELDS = ("din", "dout", "M", "N", "K", "lda", "ldb", "ldc", "a_lo", "b_lo", "c_lo", "bias_lo", "accumulate", "splits", "ws_lo", "rg", "bias2d_lo", "pool",
             "pool_pw", "pool_bf16", "drop", "reserved")


def nt_query(**kw):
    d = dict(din=1, dout=1, M=128, N=128, K=64, a_lo=0, b_lo=0, c_lo=0, bias_lo=-1, accumulate=0, splits=1, ws_lo=0, rg=0, bias2d_lo=-1, pool=0, pool_pw=0,
             pool_bf16=0, drop=0, reserved=0)
    d.update(kw)
    for name, ext in (("lda", "K"), ("ldb", "K"), ("ldc", "N")):
        d.setdefault(name, d[ext])
    return tuple(d[f] for f in NT_FIELDS)


def nt_grid():
    Ms = around(2048, 8192, 256, 512, steps=(1,)) + [1, 224, 1024, 1025]
    Ns = around(64, 128, 256, 1024, 16384, steps=(1,)) + [1, 12, 136, 768, 2048]
    Ks = around(16, 64, 128, 1024, 1536) + [32, 48, 80, 192, 256, 320, 1088, 2304, 4096]
    rng = np.random.default_rng(7)
    for din, dout in itertools.product((0, 1), repeat=2):
        for M, N, K in itertools.product(Ms, Ns, Ks):
            yield nt_query(din=din, dout=dout, M=M, N=N, K=K)
            # one random dressing of the same shape: leading dimensions, alignment, epilogue operands, split-K
            pw = int(rng.choice((0, 0, 4, 8, 12, 16, 24)))
            yield nt_query(din=din, dout=dout, M=M, N=N, K=K, lda=K + int(rng.choice((0, 4, 8))), ldb=K + int(rng.choice((0, 8, 16))),
                           ldc=N + int(rng.choice((0, 0, 2, 4, 8))), c_lo=int(rng.choice((0, 0, 2, 4, 8))), bias_lo=int(rng.choice((-1, 0, 4, 8))),
                           accumulate=int(rng.integers(2)), splits=int(rng.choice((1, 1, 2, 3, 5))), rg=int(rng.choice((0, 0, 0, 16))),
                           bias2d_lo=int(rng.choice((-1, -1, 0, 4))), pool=int(pw > 0), pool_pw=pw, pool_bf16=int(rng.integers(2)), drop=int(rng.choice((0, 0, 1))),
                           reserved=int(rng.choice((0, 16))))
    # the 32 x 32 tile count at 63, 64, 1024 and 1025, on both sides of every other rule of the rows kernel
    for (M, N), K, dout, kw in itertools.product(((224, 288), (256, 256), (2016, 1), (2048, 1), (1024, 1024), (1025, 1024), (2048, 512), (2049, 512), (32, 32800)),
                                                 (8, 16, 24, 528, 1536, 1544, 1552), (0, 1),
                                                 (dict(), dict(splits=2), dict(rg=4), dict(bias2d_lo=0), dict(pool=1, pool_pw=8, pool_bf16=1), dict(drop=1),
                                                  dict(accumulate=1, bias_lo=4), dict(c_lo=4), dict(din=0))):
        yield nt_query(**{**dict(M=M, N=N, K=K, dout=dout), **kw})
    # splits 1..13 (and a few more) against K: requests that collapse (K = 64, splits = 4), ragged last slabs, the direct-to-LDS kernel's slices
    for K, s, din, ws in itertools.product(around(64, 128, 1024, 1536, 2304, steps=(8,)) + [16, 4096, 8192, 33280], list(range(0, 14)) + [24, 128],
                                           (0, 1), (0, -1, 4)):
        yield nt_query(din=din, M=130, N=136, K=K, splits=s, ws_lo=ws)
        yield nt_query(din=din, dout=0, M=37, N=27, K=K, splits=s, ws_lo=ws)
    # the strip kernel: reserved CUs, every alignment combination of A, B, C and bias, ldc % 8, pool windows and dtypes, the 4 GiB spans
    shapes = ((8192, 2048, 128), (8192, 1024, 128), (12288, 1024, 128), (8359, 2048, 256), (9000, 1536, 128), (16384, 256, 128), (32768, 256, 128),
              (8192, 768, 128), (8192, 16384, 128), (8192, 16640, 128), (33280, 512, 768), (33280, 9216, 512))
    for (M, N, K), res in itertools.product(shapes, (0, 16, 40, 128)):
        yield nt_query(M=M, N=N, K=K, reserved=res)
        yield nt_query(M=M, N=N, K=K, reserved=res, accumulate=1, bias_lo=4)
        for pw, pbf, acc in itertools.product((4, 8, 12, 16, 24), (0, 1), (0, 1)):
            yield nt_query(M=M, N=N, K=K, reserved=res, pool=1, pool_pw=pw, pool_bf16=pbf, accumulate=acc)
    for a, b, c, bias in itertools.product((0, 8), (0, 8), (0, 2, 8), (-1, 0, 4, 2, 8)):
        for M, N, K in ((8192, 2048, 128), (130, 136, 72), (225, 257, 16), (130, 136, 1088)):
            yield nt_query(M=M, N=N, K=K, a_lo=a, b_lo=b, c_lo=c, bias_lo=bias)
    for pc, acc, dout in itertools.product(range(0, 17), (0, 1), (0, 1)):
        yield nt_query(M=8192, N=2048, K=128, ldc=2048 + pc, accumulate=acc, dout=dout)
    for M, lda, N, ldb in ((1 << 22, 512, 2048, 512), (1 << 22, 504, 2048, 504), (8192, 128, 16384, 131072), (8192, 128, 16384, 131064)):
        yield nt_query(M=M, N=N, K=128, lda=lda, ldb=ldb)
    # refusals
    for kw in (dict(M=0), dict(N=0), dict(K=0), dict(K=-8), dict(din=2), dict(dout=2), dict(dout=-1), dict(K=68), dict(din=0, K=66), dict(lda=68), dict(ldb=68),
               dict(a_lo=8), dict(b_lo=2), dict(lda=56), dict(ldb=56), dict(ldc=127), dict(splits=0), dict(splits=-1), dict(splits=2, ws_lo=-1),
               dict(splits=2, ws_lo=4), dict(splits=2, ws_lo=0)):
        yield nt_query(**kw)


def tn_grid():
    Ms = (8, 128, 248, 256, 264, 504, 512, 520, 768)
    Ns = (8, 56, 64, 72, 120, 128, 136, 512, 1016, 1024, 1032, 1152, 3072)
    Ks = (1, 63, 64, 65, 511, 512, 1000, 1024, 4096, 8128, 8192, 11776, 12280, 12288)
    for M, N, K, s in itertools.product(Ms, Ns, Ks, list(range(1, 14)) + [16, 23, 24, 25, 127, 128]):
        for dout, fb in ((0, 0), (1, 5)):
            yield (dout, M, N, K, M, N, N, 0, 0, s, 0, fb)
    for kw in itertools.product((0, 1, 2), (264, 0, 260), (136, 0, 132), (300, 0), (0, 8), (0, 4), (0, 3), (0, 8), (0, 2), (1, 3), (-1, 0, 8), (-1, 0, 7)):
        dout, M, N, K, pa, pb, pc, a_lo, b_lo, s, ws, fb = kw
        yield (dout, M, N, K, M + pa, N + pb, N + pc, a_lo, b_lo, s, ws, fb)
        yield (dout, M, N, K, M - pa, N, N, a_lo, b_lo, s, ws, fb)
        yield (dout, M, N, K, M, N - pb, N - pc, a_lo, b_lo, s, ws, fb)


def tnb_grid():
    pool = [dict(m=m, n=n, lda=m + pa, ldb=n + pb, ldc=n + pc, k=k) for m, n in ((8, 8), (136, 72), (256, 128), (512, 256), (264, 8), (256, 136), (128, 128))
            for pa, pb, pc in ((0, 0, 0), (8, 16, 4), (0, 0, 3)) for k in (0, 1, 63, 64, 65)]
    rng = np.random.default_rng(11)
    for K, s in itertools.product((64, 200, 511, 512, 513, 1024, 1536, 4096), (1, 2, 3, 4, 8, 13)):
        for n in (1, 2, 5, 8):
            for _ in range(6):
                probs = [dict(pool[int(i)]) for i in rng.choice(len(pool), n)]
                for q in probs:
                    if rng.integers(4) == 0:
                        q["k"] = int(rng.choice((K, K - 1, K + 1)))
                yield probs, K, s, 0, int(rng.choice((0, 0, 7)))
    base = dict(m=256, n=128, lda=256, ldb=128, ldc=128, k=0)
    yield None, 200, 2, 0, 0
    yield [], 200, 2, 0, 0
    yield [base] * 9, 200, 2, 0, 0
    for kw in (dict(K=0), dict(splits=0), dict(ws_lo=-1), dict(ws_lo=4), dict(fb=-1)):
        a = dict(K=200, splits=2, ws_lo=0, fb=0)
        a.update(kw)
        yield [base], a["K"], a["splits"], a["ws_lo"], a["fb"]
    for kw in (dict(k=-1), dict(k=201), dict(k=5), dict(has_ptrs=0), dict(m=0), dict(n=-8), dict(m=12), dict(n=12), dict(lda=260), dict(ldb=132), dict(lda=248),
               dict(ldb=120), dict(ldc=127), dict(a_lo=8), dict(b_lo=4)):
        yield [base, {**base, **kw}], 200, 2, 0, 0
    yield [base, {**base, "k": 5, "ldc": 130}], 200, 2, 0, 0
    yield [{**base, "ldc": 130}, {**base, "k": 5, "ldc": 132}], 200, 2, 0, 0


def tnb_line(probs, K, s, ws, fb):
    listed = [] if probs is None else probs[:16]
    head = f"b {int(probs is None)} {0 if probs is None else len(probs)} {len(listed)} {K} {s} {ws} {fb}"
    return head + "".join(" " + " ".join(str(q.get(f, d)) for f, d in (("m", 0), ("n", 0), ("lda", 0), ("ldb", 0), ("ldc", 0), ("k", 0), ("a_lo", 0), ("b_lo", 0),
                                                                     ("has_ptrs", 1))) for q in listed)


def tnb_answer(pl, nprob):
    s = f"{pl['kernel']} {pl['bad']}"
    if not pl["kernel"].startswith("refuse"):
        s += " " + " ".join(str(v) for v in [pl["splits"], pl["k_per_split"], pl["nlong"]] + pl["order"] + pl["first_tile"] + pl["wide_first_tile"] + pl["ws_off"] +
                            [pl["grid"], pl["reduce_blocks"]])
    return s


def test_compiled_selectors_equal_the_restatement(core):
    seen = set()
    qs = list(nt_grid())
    for qy, got in zip(qs, core(["n " + " ".join(map(str, qy)) for qy in qs])):
        pl = C.nt_plan(*qy)
        want = " ".join(str(pl[f]) for f in ("kernel", "splits", "k_per_split", "grid", "mb", "epi", "nstrips", "groups", "base", "rem", "reduce", "reduce_blocks"))
        assert got == want, (dict(zip(NT_FIELDS, qy)), got, want)
        seen.add(("nt", C.nt_plan_name(pl), pl["reduce"]))
    qs = list(tn_grid())
    for qy, got in zip(qs, core(["t " + " ".join(map(str, qy)) for qy in qs])):
        pl = C.tn_plan(*qy)
        want = " ".join(str(pl[f]) for f in ("kernel", "reduce", "splits", "k_per_split", "grid", "reduce_blocks"))
        assert got == want, (qy, got, want)
        seen.add(("tn", pl["kernel"], pl["reduce"]))
    qs = list(tnb_grid())
    for qy, got in zip(qs, core([tnb_line(*qy) for qy in qs])):
        pl = C.tnb_plan(*qy)
        assert got == tnb_answer(pl, 0 if qy[0] is None else len(qy[0])), (qy, got, pl)
        seen.add(("tnb", pl["kernel"]))
    # the grid is not blind: every kernel, every strip instantiation, every reduce and every refusal the header names is reached
    want = {("nt", k, 0) for k in ("refuse_empty", "refuse_dtype", "refuse_chunk", "refuse_align", "refuse_ld", "refuse_splits", "refuse_workspace", "rows")}
    want |= {("nt", f"strip{mb}.{epi}", 0) for mb in (2, 3, 4) for epi in range(4)} | {("nt", k, r) for k in ("glds", "tile") for r in (0, 1)}
    want |= {("tn", k, 0) for k in ("refuse_empty", "refuse_dtype", "refuse_chunk", "refuse_align", "refuse_ld", "refuse_workspace", "refuse_folds")}
    want |= {("tn", k, r) for k in ("tile1", "tile3") for r in range(4)} | {("tn", k, r) for k in ("wide", "tall") for r in (1, 2)}
    want |= {("tnb", k) for k in ("refuse_count", "refuse_call", "refuse_folds", "refuse_k", "refuse_no_long", "refuse_empty", "refuse_shape", "refuse_align",
                                  "refuse_short_ldc", "batch128", "batch_wide")}
    assert seen == want, (sorted(map(str, seen - want)), sorted(map(str, want - seen)))


def test_compiled_strip_plan_equals_the_restatement(core):
    qs = [(M, N, K, res) for M in around(8192, 12288, 33280, steps=(1, 32)) + [8359, 9000, 16384, 32768, 65536] for N in (0, 128, 256, 512, 768, 1024, 1280,
          1536, 2048, 2304, 9216, 16384, 16640) for K in (64, 127, 128, 192, 256, 512) for res in (0, 16, 40, 128, 250, 256)]
    got = core([f"s {M} {N} {K} {res}" for M, N, K, res in qs])
    answers = set()
    for (M, N, K, res), g in zip(qs, got):
        sp = C.strip_plan(M, N, K, res)
        assert g == ("0" if sp is None else "1 " + " ".join(map(str, sp))), (M, N, K, res, g, sp)
        answers.add(None if sp is None else sp[0])
    assert answers == {None, 2, 3, 4}
    # the two shapes an earlier test took for strip shapes are refused; its replacement is served
    assert C.strip_plan(16384, 256, 128) is None and C.strip_plan(8192, 256, 128) is None and C.strip_plan(32768, 256, 128) is not None


def test_tables_select_what_they_claim():
    for c, which in C.NT_RUNS:
        pl = C.nt_case_plan(c, which)
        assert (C.nt_plan_name(pl), pl["splits"]) == (c.kernel, c.slabs), (C.nt_id(c), pl)
        assert which != "int" or C.nt_exact_ok(c), C.nt_id(c)
    for c in C.TN_CASES:
        pl = C.tn_case_plan(c)
        assert (pl["kernel"], pl["splits"]) == (c.kernel, c.slabs), (C.tn_id(c), pl)
        assert 9 * c.K + 3 < 2 ** 24 and C.fold_exact_ok(c.folds)
    for c in C.TNB_CASES:
        pl = C.tnb_case_plan(c)
        assert (pl["kernel"], pl["splits"]) == (c.kernel, c.slabs), (C.tnb_id(c), pl)
    for runs, ident in ((C.NT_RUNS, C.nt_run_id), (C.TN_RUNS, C.tn_run_id), (C.TNB_RUNS, C.tnb_run_id)):
        assert len({ident(r) for r in runs}) == len(runs), "case ids are not unique"
    # all twelve strip instantiations, every NT kernel with and without a reduce, every TN form and every reduce are in the tables
    reached = {(c.kernel, w) for c, w in C.NT_RUNS}
    for mb, epi in itertools.product((2, 3, 4), range(4)):
        assert (f"strip{mb}.{epi}", "normal") in reached and (epi == 3 or (f"strip{mb}.{epi}", "int") in reached), (mb, epi)
    assert {(c.kernel, c.slabs > 1) for c in C.NT_CASES} >= {("tile", False), ("tile", True), ("glds", False), ("glds", True), ("rows", False)}
    assert {(c.kernel, C.tn_case_plan(c)["reduce"]) for c in C.TN_CASES} >= {("tile1", 0), ("tile1", 1), ("tile1", 3), ("tile3", 0), ("tile3", 1), ("tile3", 2),
                                                                          ("tile3", 3), ("wide", 1), ("wide", 2), ("tall", 1)}
    assert {c.kernel for c in C.TNB_CASES} == {"batch128", "batch_wide"}
    # the key-boundary case: some written row starts a 4-aligned, not 8-aligned flat index within 8 of a 4096 boundary
    for c in C.NT_CASES:
        if c.tag == "key-boundary":
            flat = R.out_rows(c.M, c.rg, c.gs, c.roff) * c.ldc
            assert ((flat % 4096) == 4092).any() and c.dout == "fp32" and (c.ldc * 4) % 16 == 0


# ------------------------------------------------------------------------------------- 2. float32 restatements and mistakes
F32 = np.float32


def gather(flat, ld, rows, k0, k1):
    """[rows, k1 - k0] of a flat row-major buffer with leading dimension ld (columns past ld run into the next row, as on the device)"""
    return flat[np.arange(rows)[:, None] * ld + np.arange(k0, k1)[None, :]]


def slab_sum(slabs, skip_remainder=False):
    """the split-K sum: four slabs at a time, ((((v + a0) + a1) + a2) + a3), then the one to three that remain"""
    v = np.zeros_like(slabs[0])
    full = len(slabs) // 4 * 4
    for a in slabs[:full] if skip_remainder else slabs:
        v = v + a
    return v


def buggy_keep(seed, flat, p):
    """the mask of an 8-wide column group whose key is taken once, from its first element: columns past a 4096 boundary are hashed as
    columns 4096.. of the old key"""
    first = flat[:, :1] + (np.arange(flat.shape[1])[None, :] // 8) * 8      # flat index of the group's first column
    col = (first % 4096) + (flat - first)
    key = D.row_key(seed, (first // 4096).reshape(-1)).reshape(first.shape)
    h = D.mix32((key + (col // 2).astype(np.uint32) * D.GOLDEN).reshape(-1)).reshape(first.shape)
    u16 = np.where(col % 2 == 1, h >> np.uint32(16), h & np.uint32(0xFFFF))
    return u16 >= np.uint32(D.threshold(p))


def sim_nt(c, which, bug=None):
    """the NT kernels in float32: K in the kernel's chunks, slab by slab, the epilogue in the kernel's order, one rounding at the store.
    Returns the output buffer [out_rows, ldc] as float64"""
    d, pl = C.nt_inputs(c, which), C.nt_case_plan(c, which)
    M, N, K = c.M, c.N, c.K
    A = C.padded(d["A"], c.lda).astype(F32).reshape(-1)
    B = C.padded(d["B"], c.ldb).astype(F32).reshape(-1)
    lda = K if bug == "lda_as_K" else c.lda
    ch = 8 if c.din == "bf16" else 4
    BK = 64 if c.din == "bf16" else 32
    bias = d["bias"].astype(F32) if c.bias else None
    slabs = []
    for s in range(pl["splits"]):
        kbeg, kend = s * pl["k_per_split"], min(K, (s + 1) * pl["k_per_split"])
        acc = np.zeros((M, N), F32)
        if c.kernel == "rows":      # the k-steps of 16 dealt over four waves, joined in LDS
            part = []
            for w in range(4):
                ks = np.arange(w, K // 16, 4)
                cols = (ks[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)
                a, b = A[np.arange(M)[:, None] * lda + cols[None, :]], B[np.arange(N)[:, None] * c.ldb + cols[None, :]]
                part.append(a @ b.T if cols.size else np.zeros((M, N), F32))
            acc = ((part[0] + part[1]) + part[2]) + part[3]
        else:
            for k0 in range(kbeg, kend, BK):
                k1 = min(k0 + BK, kend)
                if bug == "skip_last_ktile" and k1 == kend:
                    continue
                if bug == "ktail_chunk" and k1 == kend and k1 < k0 + BK:
                    k1 += ch        # the chunk behind the slice's end is multiplied in instead of zeroed
                acc = acc + gather(A, lda, M, k0, k1) @ gather(B, c.ldb, N, k0, k1).T
        if bug == "bias_per_slab" and bias is not None:
            acc = acc + bias[None, :]
        slabs.append(acc)
    v = slab_sum(slabs, bug == "reduce_skip_remainder") if pl["splits"] > 1 else slabs[0]
    cols = np.arange(N)
    if c.pw:
        pool = d["pool"].astype(F32) * (F32(1) / F32(c.pw))
        v = v + (pool[:, (cols // 8 * 8) // c.pw] if bug == "pool_first_window" else np.repeat(pool, c.pw, axis=1))
    if bias is not None and bug != "bias_per_slab":
        v = v + bias[None, :]
    if c.b2:
        v = v + d["bias2d"].astype(F32)[np.arange(M) % c.rg]
    rows = R.out_rows(M, c.rg, c.gs, 0 if bug == "no_roff" else c.roff)
    p = c.p_of(which)
    if p > 0:
        flat = rows[:, None] * c.ldc + cols[None, :]
        vec = (c.ldc * C.ES[c.dout]) % 16 == 0 and N >= 8
        if bug == "key_not_advanced" and vec:
            kept = buggy_keep(C.SEED, flat, p)
            tail = cols >= N // 8 * 8          # the ragged last column group takes the element-wide branch
            kept[:, tail] = R.flat_keep(C.SEED, int(flat.max()) + 1, p)[flat][:, tail]
        else:
            kept = R.flat_keep(C.SEED, int(flat.max()) + 1, p)[flat]
        v = v * np.where(kept, D.inv_keep(p), F32(0))
    if c.acc:
        old = d["old"].astype(F32)
        if bug == "acc_dropped_bf16_vec" and c.dout == "bf16" and c.ldc % 8 == 0 and c.coff == 0 and c.bias != 2:
            old = np.where((cols < N // 8 * 8)[None, :], F32(0), old)
        v = v + old
    assert v.dtype == F32
    buf = C.nt_c_initial(c, which)
    if bug == "ldc_as_N":
        buf.reshape(-1)[(rows[:, None] * N + cols[None, :]).reshape(-1)] = C.q(v, c.dout).reshape(-1)
    else:
        buf[rows, :N] = C.q(v, c.dout)
    return buf


def sim_tn_one(A, B, lda, ldb, M, N, k_rows, kps, nslabs, bug=None):
    """one TN problem in float32: 64 k rows at a time, slab by slab.  A, B: flat padded buffers"""
    slabs = []
    for s in range(nslabs):
        kbeg, kend = s * kps, min(k_rows, (s + 1) * kps)
        acc = np.zeros((M, N), F32)
        for k0 in range(kbeg, kend, 64):
            k1 = min(k0 + 64, kend)
            if bug == "skip_last_ktile" and k1 == kend:
                continue
            a = A[np.arange(k0, k1)[:, None] * lda + np.arange(M)[None, :]]
            b = B[np.arange(k0, k1)[:, None] * ldb + np.arange(N)[None, :]]
            acc = acc + a.T @ b
        slabs.append(acc)
    return slab_sum(slabs, bug == "reduce_skip_remainder") if nslabs > 1 else slabs[0]


def sim_tn(c, which, bug=None):
    d, pl = C.tn_inputs(c, which), C.tn_case_plan(c)
    A, B = (C.padded(d[n], ld).astype(F32).reshape(-1) for n, ld in (("A", c.lda), ("B", c.ldb)))
    v = sim_tn_one(A, B, c.M if bug == "lda_as_K" else c.lda, c.ldb, c.M, c.N, c.K, pl["k_per_split"], pl["splits"], bug)
    if c.acc:
        v = v + d["old"].astype(F32)
    buf = C.tn_c_initial(c, which)
    buf[:, :c.N] = C.q(v.astype(np.float64), c.dout)
    return buf


def sim_fold(pt):
    """a fold in float32: 32 thread rows take every 32nd partial row, then 32 -> 4 -> 1 in a fixed order"""
    pt = pt.astype(F32)
    rows = [pt[r::32].sum(0, dtype=F32) if r < pt.shape[0] else np.zeros(pt.shape[1:], F32) for r in range(32)]
    quarter = [sum(rows[8 * i + 1:8 * i + 8], rows[8 * i]) for i in range(4)]
    return ((quarter[0] + quarter[1]) + (quarter[2] + quarter[3])).astype(np.float64)


def test_float32_restatement_meets_every_bar():
    worst = 0.0     # over the fp32 outputs: a bf16 output that rounds at the worst place of a binade sits just below 1 by construction
    for c, which in C.NT_RUNS:
        ok, w, msg = C.nt_judge(c, which, sim_nt(c, which))
        assert ok, (C.nt_id(c), which, msg, w)
        worst = max(worst, w if c.dout == "fp32" else 0.0)
    for c, which in C.TN_RUNS:
        ok, w, msg = C.tn_judge(c, which, sim_tn(c, which))
        assert ok, (C.tn_id(c), which, msg, w)
        worst = max(worst, w if c.dout == "fp32" else 0.0)
        for (pt, value, S), (parts, _, _) in zip(C.tn_inputs(c, which)["folds"], c.folds):
            ok, w, msg = C.fold_judge(which, sim_fold(pt), value, S, parts)
            assert ok, (C.tn_id(c), which, "fold", parts, msg, w)
    for c, which in C.TNB_RUNS:
        pl = C.tnb_case_plan(c)
        probs, _ = C.tnb_inputs(c, which)
        for (m, n, pa, pb, pc, k), d in zip(c.probs, probs):
            long = k in (0, c.K)
            A, B = (C.padded(d[nm], ld).astype(F32).reshape(-1) for nm, ld in (("A", m + pa), ("B", n + pb)))
            v = sim_tn_one(A, B, m + pa, n + pb, m, n, c.K if long else k, pl["k_per_split"] if long else k, pl["splits"] if long else 1)
            buf = np.full((m, n + pc), C.SENT)
            buf[:, :n] = v
            ok, w, msg = C.dense_judge(which, buf, n, d["ref"], d["S"], d["chain"], "fp32")
            assert ok, (C.tnb_id(c), which, (m, n, k), msg, w)
            worst = max(worst, w)
    print(f"float32 restatements, fp32 outputs: worst ratio to the bar = {worst:.3f}")
    assert worst < 0.5      # a correct kernel sits far below the bar: the bound is a worst case over orders, the error a random walk


small = lambda c: c.M * c.N * c.K < 5e7
NT_BUGS = {
    "ktail_chunk": lambda c: small(c),
    "skip_last_ktile": lambda c: small(c),
    "lda_as_K": lambda c: small(c) and c.pa > 0,
    "ldc_as_N": lambda c: small(c) and c.pc > 0,
    "bias_per_slab": lambda c: c.slabs > 1 and c.bias,
    "acc_dropped_bf16_vec": lambda c: small(c) and c.acc and c.dout == "bf16",
    "pool_first_window": lambda c: small(c) and c.pw % 8 != 0,
    "no_roff": lambda c: c.roff > 0,
    "reduce_skip_remainder": lambda c: c.slabs > 1,
    "key_not_advanced": lambda c: c.p > 0,
}


@pytest.mark.parametrize("bug", sorted(NT_BUGS))
def test_a_plausible_mistake_is_caught_nt(bug):
    """made in the float32 restatement, the mistake fails the judge on at least one shipped case -- in both input sets where both run"""
    caught = {"int": [], "normal": []}
    for c, which in C.NT_RUNS:
        if NT_BUGS[bug](c) and not C.nt_judge(c, which, sim_nt(c, which, bug))[0]:
            caught[which].append(C.nt_id(c))
    assert caught["normal"], bug
    assert caught["int"] or bug == "pool_first_window", bug      # (windows that 8 columns straddle are no powers of two: normal set only)
    if bug == "key_not_advanced":   # only the cases built for it see it: everywhere else the 8 columns start a multiple of 8
        assert all("key-boundary" in i for w in caught.values() for i in w) and len(caught["normal"]) >= 2, caught


@pytest.mark.parametrize("bug", ["skip_last_ktile", "lda_as_K", "reduce_skip_remainder"])
def test_a_plausible_mistake_is_caught_tn(bug):
    caught = [C.tn_id(c) for c, which in C.TN_RUNS if c.M * c.N * c.K < 5e7 and not C.tn_judge(c, which, sim_tn(c, which, bug))[0]]
    assert caught, bug


def test_a_short_problem_reduced_over_the_calls_k_is_caught():
    caught = 0
    for c, which in C.TNB_RUNS:
        probs, _ = C.tnb_inputs(c, which)
        for (m, n, pa, pb, pc, k), d in zip(c.probs, probs):
            if k not in (0, c.K):
                A, B = (C.padded(d[nm], ld).astype(F32).reshape(-1) for nm, ld in (("A", m + pa), ("B", n + pb)))
                buf = sim_tn_one(A, B, m + pa, n + pb, m, n, c.K, c.K, 1).astype(np.float64)
                caught += not C.dense_judge(which, buf, n, d["ref"], d["S"], d["chain"], "fp32")[0]
    assert caught >= 8


def test_references_agree_with_einsum_and_the_mask_contract():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(100000) * 10.0 ** rng.integers(-6, 7, 100000), np.arange(-4096.0, 4096.0), [0.0, -0.0, 1.00390625, 1.01171875]])
    assert np.array_equal(C.q(x, "bf16"), D.bf16_round(x))
    A, B, bias, b2, pool, old = rng.standard_normal((10, 7)), rng.standard_normal((12, 7)), rng.standard_normal(12), rng.standard_normal((4, 12)), \
        rng.standard_normal((10, 3)), rng.standard_normal((10, 12))
    v, S, kept = R.nt(A, B, bias, b2, 4, 6, 1, pool, 4, old, (C.SEED, 0.25), 12)
    rows = R.out_rows(10, 4, 6, 1)
    assert list(rows) == [1, 2, 3, 4, 7, 8, 9, 10, 13, 14]
    for m, n in itertools.product(range(10), range(12)):
        i = rows[m] * 12 + n
        k = bool(D.keep_rows(C.SEED, np.array([i >> 12], np.uint64), 4096, 0.25)[0, i & 4095])
        want = (sum(A[m, j] * B[n, j] for j in range(7)) + bias[n] + b2[m % 4, n] + pool[m, n // 4] / 4) * (float(D.inv_keep(0.25)) if k else 0.0) + old[m, n]
        assert kept[m, n] == k and abs(v[m, n] - want) < 1e-12 and S[m, n] >= abs(v[m, n]) - 1e-12
    At, Bt = rng.standard_normal((9, 5)), rng.standard_normal((9, 6))
    assert np.allclose(R.tn(At, Bt, 4)[0], np.einsum("km,kn->mn", At[:4], Bt[:4]))
    pt = rng.standard_normal((7, 2, 3))
    assert np.allclose(R.fold(pt)[0], np.einsum("wpc->pc", pt))
