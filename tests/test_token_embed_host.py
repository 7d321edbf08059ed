"""The host side of the token-embedding kernel (csrc/spv_token_embed_core.h, the two entry points of csrc/spv_patch.hip): declarations,
bindings, work model, census size, the refusals that precede any launch, and the selector against a restatement.  No GPU is touched: a
refusal returns before the first HIP call, and spv_token_embed_supported is arithmetic."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-spectre-experiments_amd", "csrc")
F32, BF16 = 0, 1


def _native():
    from spectre_vit import _native as n
    return n


def _declared(name):
    """the parameter list of `name` in include/spv.h"""
    text = open(os.path.join(ROOT, "include", "spv.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/spv.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_symbols_are_declared_and_bound_with_matching_arity():
    n = _native()
    for name in ("spv_token_embed_supported", "spv_token_embed_fwd"):
        params = _declared(name)
        assert len(params) == len(n.SIGNATURES[name]), (name, params)
        for text, ctype in zip(params, n.SIGNATURES[name]):
            if "*" in text:
                assert ctype is n.c_vp, (name, text)
            elif text.startswith("float"):
                assert ctype is n.c_f, (name, text)
            elif text.startswith("uint64_t"):
                assert ctype is n.c_u64, (name, text)
            else:
                assert text.startswith("int ") and ctype is n.c_i, (name, text)
    assert "spv_token_embed_supported" in n._NO_STATUS and "spv_token_embed_fwd" not in n._NO_STATUS
    lib = n.load()
    assert "spv_token_embed_fwd" in n._LAUNCHERS and "spv_token_embed_supported" not in n._LAUNCHERS   # the launch is timed, the query is not
    assert lib.spv_version() == 1


def test_work_model_keeps_the_bracket_key_of_the_call_it_replaces():
    from spectre_vit import timing
    new = timing._WORK_MODELS["spv_token_embed_fwd"]
    old = timing._WORK_MODELS["spv_gemm_nt_grouped_rows_drop"]
    rows, n, k, T = 33280, 512, 48, 65
    # the integer arguments of each call in header order, then the NULL-pointer mask and the hint (_native.call)
    a = new((rows, n, k, T, 0, 0))
    b = old((rows, n, k, k, k, n, BF16, BF16, T, T, 0, 4, 0))
    assert a == b == ("gemm_grouped_rows", (rows, n, k), BF16, "mfma", 2.0 * rows * n * k)


def test_census_is_still_27_slots():
    n = _native()
    text = open(os.path.join(ROOT, "include", "spv.h")).read()
    assert re.search(r"SPV_PATH_COUNT\s*=\s*27\b", text)
    assert len(n.PATH) == 27 and sorted(n.PATH.values()) == list(range(27))
    assert "token_embed" not in n.PATH   # the host counter hip_ops.PATH_COUNTS["token_embed"] tells the paths apart


P = 16  # any non-null, 16-byte aligned "pointer": validation fails before it would be used
GOOD = dict(patches=P, w=P, posbias=P, tokens=P, rows=130, n=512, k=48, T=65, p=0.3)
REFUSALS = [
    (dict(k=40), "unsupported shape"),
    (dict(k=80), "unsupported shape"),
    (dict(k=0), "unsupported shape"),
    (dict(n=100), "unsupported shape"),
    (dict(n=0), "unsupported shape"),
    (dict(rows=0), "unsupported shape"),
    (dict(rows=-5), "unsupported shape"),
    (dict(T=0), "tokens_per_image"),
    (dict(p=1.0), "p_drop"),
    (dict(p=-0.1), "p_drop"),
    (dict(patches=0), "null pointer"),
    (dict(posbias=0), "null pointer"),
    (dict(tokens=P + 8), "16-byte aligned"),
    (dict(w=P + 2), "16-byte aligned"),
    (dict(posbias=P + 4), "16-byte aligned"),
]


@pytest.mark.parametrize("change,needle", REFUSALS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_bad_arguments_are_refused_before_any_launch(change, needle):
    n = _native()
    lib = n.load()
    a = {**GOOD, **change}
    args = (a["patches"], a["w"], a["posbias"], a["tokens"], a["rows"], a["n"], a["k"], a["T"], a["p"], 1234, 0)
    assert lib.spv_token_embed_fwd(*args) != 0
    assert needle in lib.spv_last_error().decode(), (change, lib.spv_last_error().decode())
    with pytest.raises(RuntimeError) as e:
        n.call("spv_token_embed_fwd", *args)
    assert "spv_token_embed_fwd" in str(e.value) and needle in str(e.value)


def test_fp32_is_not_served():
    """spv_token_embed_fwd takes no dtype (its operands are bf16 by contract): fp32 callers are turned away by the query they dispatch on"""
    n = _native()
    assert n.call("spv_token_embed_supported", 130, 512, 48, F32) == 0
    assert n.call("spv_token_embed_supported", 130, 512, 48, BF16) == 1
    assert n.call("spv_token_embed_supported", 130, 512, 48, 2) == 0


def supported(rows, n, k, dtype):
    """the contract of include/spv.h, restated"""
    return int(dtype == BF16 and rows > 0 and n > 0 and n % 64 == 0 and k in (16, 32, 48, 64))


def plan(rows, n, cus, waves_per_cu=12):
    """token_embed_plan, restated: (shares, walkers, longest walk, workgroups of four waves)"""
    shares, nblk = n // 64, -(-rows // 32)
    most = max(1, cus * waves_per_cu // shares)
    per = -(-nblk // most)
    walkers = -(-nblk // per)
    return shares, walkers, per, -(-walkers * shares // 4)


ROWS = (-1, 0, 1, 15, 31, 32, 33, 130, 8255, 33280, 2 ** 30)
NS = (-64, 0, 8, 63, 64, 65, 100, 128, 192, 512, 768, 1000, 1024)
KS = (-16, 0, 8, 15, 16, 17, 24, 32, 40, 48, 56, 64, 65, 80, 768)


def test_selector_agrees_with_the_restatement():
    n = _native()
    for dtype in (-1, F32, BF16, 2):
        for rows in ROWS:
            for cols in NS:
                for k in KS:
                    assert n.call("spv_token_embed_supported", rows, cols, k, dtype) == supported(rows, cols, k, dtype), (rows, cols, k, dtype)


def test_plan_header_agrees_with_the_restatement(tmp_path):
    """the grid plan, compiled with a plain C++ compiler (the header holds no HIP type): every block has a walker, no walker is idle,
    the shares differ by at most one block and the resident-wave budget holds"""
    cases = [(rows, n, cus) for rows in (1, 15, 32, 33, 130, 8255, 12545, 33280, 100000, 2 ** 30) for n in (64, 128, 512, 768, 4096, 65536)
             for cus in (1, 8, 256, 304)]
    src = tmp_path / "plan.cpp"
    src.write_text('#include <stdio.h>\n#include "spv_token_embed_core.h"\nint main() {\n    int r, n, c;\n'
                   '    while (scanf("%d %d %d", &r, &n, &c) == 3) {\n        const TokenEmbedPlan p = token_embed_plan(r, n, c);\n'
                   '        printf("%d %d %d %d %d\\n", p.shares, p.walkers, p.per, p.grid, token_embed_supported(r, n, 48, 1));\n    }\n    return 0;\n}\n')
    exe = tmp_path / "plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], input="".join(f"{r} {n} {c}\n" for r, n, c in cases), capture_output=True, text=True, check=True).stdout
    lines = [tuple(int(x) for x in ln.split()) for ln in out.strip().splitlines()]
    assert len(lines) == len(cases)
    for (rows, n, cus), got in zip(cases, lines):
        assert got[:4] == plan(rows, n, cus) and got[4] == 1, (rows, n, cus, got)
        shares, walkers, per, grid = got[:4]
        nblk = -(-rows // 32)
        assert 1 <= walkers <= nblk and (walkers - 1) * per < nblk <= walkers * per   # strided walks: the longest is `per`, none is empty
        assert -(-nblk // walkers) == per   # (strided walks differ by at most one block by construction)
        assert walkers * shares <= max(cus * 12, shares) and grid * 4 >= walkers * shares > (grid - 1) * 4
