"""CPU checks of the tiled augmentation path (csrc/spv_augment_tiled.hip, csrc/spv_augment_core.h, spectre_vit.augment): the plan and
workspace functions, every host refusal of spv_augment_tiled_u8, TrainAugment's kernel switch, the share of pixels the restatement
leaves out on the very tables the GPU tests use, and the shared per-pixel header compiled for the host and held to tests/augment_ref.py."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import augment_ref as R
import augment_tiled_cases as T


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


def test_plan_truth_table(built):
    from spectre_vit import _native
    plan = lambda c, h, w: _native.call("spv_augment_plan", c, h, w)
    sup = lambda c, h, w: _native.call("spv_augment_supported", c, h, w)
    assert [plan(*s) for s in T.LARGE] == [2, 2, 1, 2]   # 1 x 33 x 97 fits the LDS kernel too: the GPU tests force it through the tiled one
    assert [plan(*s) for s in T.BOTH] == [1, 1]
    assert plan(1, 224, 224) == 2 and plan(3, 512, 512) == 2 and plan(3, 16, 512) == 2 and plan(3, 2, 512) == 1 and plan(1, 2, 2) == 1
    for bad in ((2, 32, 32), (2, 64, 64), (3, 1, 64), (3, 64, 1), (3, 513, 64), (3, 64, 513), (3, 0, 0), (0, 64, 64), (3, -4, 64)):
        assert plan(*bad) == 0, bad
    # spv_augment_supported keeps its truth table (tests/test_augment.py pins it too)
    assert sup(3, 32, 32) == 1 and sup(1, 28, 28) == 1
    assert sup(3, 224, 224) == 0 and sup(1, 224, 224) == 0 and sup(2, 32, 32) == 0 and sup(3, 1, 32) == 0 and sup(3, 0, 0) == 0
    assert sup(3, 64, 64) == 0 and sup(3, 70, 45) == 0
    for c in (1, 3):
        for h, w in ((2, 2), (28, 28), (32, 32), (52, 52), (53, 53), (64, 64), (90, 90), (91, 91)):
            assert (plan(c, h, w) == 1) == (sup(c, h, w) == 1) and plan(c, h, w) >= 1


def test_workspace_bytes_are_monotone_and_non_zero(built):
    from spectre_vit import _native
    ws = lambda b, h, w: _native.call("spv_augment_tiled_ws_bytes", b, h, w)
    sizes = (2, 3, 28, 32, 45, 64, 70, 97, 224, 511, 512)
    for b in (1, 7, 512):
        for h in sizes:
            for w in sizes:
                v = ws(b, h, w)
                assert v >= 4 * b and v % 4 == 0, (b, h, w, v)
                assert ws(b + 1, h, w) > v
                if h < 512:
                    assert ws(b, h + 1, w) >= v
                if w < 512:
                    assert ws(b, h, w + 1) >= v
    assert ws(512, 512, 512) > ws(512, 224, 224) > ws(512, 32, 32)
    assert ws(0, 64, 64) == 0 and ws(4, 513, 64) == 0 and ws(4, 1, 64) == 0


def test_tiled_entry_point_rejects_bad_arguments_before_any_launch(built):
    """Every call fails validation on the host: nothing is launched (no GPU here).  Pointers are small fake addresses that are never
    dereferenced.  An index outside the set is not among them: the host cannot see a device index."""
    from spectre_vit import _native
    name = "spv_augment_tiled_u8"
    need = _native.call("spv_augment_tiled_ws_bytes", 4, 224, 224)
    #        src idx par mean istd out  B  n  C  H    W    ws  bytes stream
    good = [16, 0, 16, 16, 16, 16, 4, 8, 3, 224, 224, 16, need, 0]

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[dict(src=0, idx=1, par=2, mean=3, istd=4, out=5, B=6, n=7, C=8, H=9, W=10, ws=11, nbytes=12)[k]] = v
        return tuple(a)
    cases = [
        (with_(src=0), "src"), (with_(out=0), "out"), (with_(par=0), "params"), (with_(mean=0), "mean"), (with_(istd=0), "inv_std"),
        (with_(B=0), "bad shape"), (with_(n=0), "bad shape"), (with_(H=0), "bad shape"), (with_(B=-3), "bad shape"),
        (with_(C=2), "not supported"), (with_(H=513), "not supported"), (with_(W=1), "not supported"), (with_(H=4097, W=4097), "not supported"),
        (with_(B=9, nbytes=1 << 20), "n_src"),
        (with_(out=18), "aligned"), (with_(par=17), "aligned"), (with_(ws=18), "aligned"),
        (with_(ws=0), "workspace"), (with_(nbytes=need - 1), "workspace"), (with_(nbytes=0), "workspace"), (with_(ws=0, nbytes=0), "workspace"),
    ]
    for args, needle in cases:
        with pytest.raises(RuntimeError) as e:
            _native.call(name, *args)
        assert name in str(e.value) and needle in str(e.value), (args, needle, str(e.value))
    # the LDS entry point keeps its refusal of a large image
    with pytest.raises(RuntimeError, match="not supported"):
        _native.call("spv_augment_u8", 16, 0, 16, 16, 16, 16, 4, 8, 3, 64, 64, 0)


def test_train_augment_kernel_argument():
    from spectre_vit import harness
    from spectre_vit.augment import TrainAugment
    assert inspect.signature(TrainAugment.__init__).parameters["kernel"].default == "auto"
    assert TrainAugment(T.MEAN, T.STD).kernel == "auto"
    for k in ("auto", "lds", "tiled"):
        assert TrainAugment(T.MEAN, T.STD, kernel=k).kernel == k
    for bad in ("", "LDS", "tile", None, 2):
        with pytest.raises(ValueError, match="kernel"):
            TrainAugment(T.MEAN, T.STD, kernel=bad)
    # the harness needs no new argument: its TrainAugment is the default one
    assert "kernel" not in inspect.signature(harness.train).parameters
    assert inspect.signature(harness.train_distill).parameters["augment"].default is True


def test_restatement_leaves_out_no_more_than_the_caps_on_the_gpu_tables():
    """What the GPU comparisons leave out is decided by the restatement alone: rotation ties and, under a blur, their 3 x 3 neighbourhood,
    at most 1 % / 5 % of the batch -- and nothing when no sample rotates.  Held here on the exact tables, so that no GPU run is needed
    to know the caps hold."""
    worst = {}
    n = 0
    for name, shape, build in T.all_cases():
        _, index, params = build()
        assert params.dtype == np.float32 and params.shape[1] == R.NPARAM
        assert index is None or len(index) == len(params)
        share = float(T.left_out(params, shape).mean())
        cap = T.cap_of(params)
        kind = name.split("-")[0]
        worst[(kind, cap)] = max(worst.get((kind, cap), 0.0), share)
        assert share <= cap, f"{name}: {100 * share:.2f} % left out, cap {100 * cap:.0f} %"
        if kind == "rotate" or (kind == "chain" and len(params) > 1):
            assert (params[:, R.ANGLE] != 0).sum() >= min(len(params), 16) and share > 0
        n += 1
    print({f"{k[0]} (cap {k[1]})": round(v, 5) for k, v in worst.items()})
    assert n == len(T.SHAPES) * (1 + len(T.ALL_OPS_ALONE) + 1 + 6)


CORE_MAIN = r"""
#include "spv_augment_core.h"
#include <stdio.h>
// stdin: n, then n rows "C order bright contrast sat hue gray m stop r g b"; stdout: one row "r g b" per input row (%.9g round-trips fp32)
int main() {
    int n;
    if (scanf("%d", &n) != 1) return 1;
    for (int i = 0; i < n; ++i) {
        int C, gray, stop;
        float order, m, v[3];
        AugJitter j;
        if (scanf("%d %f %f %f %f %f %d %f %d %f %f %f", &C, &order, &j.bright, &j.contrast, &j.sat, &j.hue, &gray, &m, &stop, &v[0], &v[1],
                  &v[2]) != 12) return 2;
        j.order = aug_order_index(order);
        if (stop == AUG_OP_CONTRAST) {
            const float g = C == 3 ? aug_grey_before_contrast<3>(v, j) : aug_grey_before_contrast<1>(v, j);
            printf("%.9g %.9g %.9g\n", g, g, g);
        } else {
            if (C == 3) aug_colour_pixel<3>(v, j, m, gray != 0);
            else aug_colour_pixel<1>(v, j, m, gray != 0);
            printf("%.9g %.9g %.9g\n", v[0], v[1], v[2]);
        }
    }
    return 0;
}
"""


def ref_pixels(px, C, order, f, gray, m, stop, dtype):
    """augment_ref's ops on pixels px (3, n) in `dtype`, in the order's sequence, the contrast mean GIVEN (not taken from px); stop at
    contrast (returning the grey value three times) or run everything plus RandomGrayscale"""
    t = np.dtype(dtype).type
    x = px[:C].astype(dtype)
    b, c, s, h = (t(v) for v in f)
    for op in R.order_of(order):
        if op == 1 and stop:
            g = R.grey(x)
            return np.stack([g, g, g])
        if op == 0:
            x = R.brightness(x, b)
        elif op == 1:
            x = R.clamp(c * x + (t(1.0) - c) * t(m))
        elif op == 2:
            x = R.saturation(x, s)
        else:
            x = R.hue(x, h)
    assert not stop
    if gray and C == 3:
        x = np.repeat(R.grey(x)[None], 3, axis=0)
    return np.concatenate([x, np.zeros((3 - C, x.shape[1]), dtype)])


def test_core_header_on_the_host_against_the_restatement(tmp_path):
    """csrc/spv_augment_core.h is what the mean pre-pass and the tile kernel both run per pixel.  Compiled here by the host compiler into
    a stand-alone program: all 24 orders x (full chain with and without grayscale, the part in front of contrast) x 1 and 3 channels on
    a few hundred pixels with a given m, against augment_ref's ops in float64, allowed 4 x the largest |float32 - float64| of the same
    ops in numpy float32."""
    from conftest import ROOT
    csrc = os.path.join(ROOT, "vit-spectre-experiments_amd", "csrc")
    src, exe = tmp_path / "core_main.cpp", tmp_path / "core_main"
    src.write_text(CORE_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", csrc, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    rng = np.random.default_rng(7)
    npx = 300
    px = (rng.integers(0, 256, size=(3, npx)).astype(np.float32) / np.float32(255.0))
    px[:, :6] = np.array([[0, 0, 0], [1, 1, 1], [.5, .5, .5], [1, 0, 0], [.2, .2, .7], [.3, .3, .1]], np.float32).T   # flat and primary colours
    groups, lines = [], []
    for C in (3, 1):
        for order in range(24):
            for mode in ("full", "gray", "stop"):
                f = np.array([rng.uniform(0.6, 1.4), rng.uniform(0.6, 1.4), rng.uniform(0.6, 1.4), rng.uniform(-0.1, 0.1)], np.float32)
                if order % 5 == 0:
                    f[3] = 0.0   # a zero shift is skipped
                m = np.float32(rng.uniform(0.2, 0.8))
                groups.append((C, order, f, mode == "gray", m, mode == "stop"))
                for k in range(npx):
                    lines.append(f"{C} {order} {f[0]:.9g} {f[1]:.9g} {f[2]:.9g} {f[3]:.9g} {int(mode == 'gray')} {m:.9g} "
                                 f"{1 if mode == 'stop' else 4} {px[0, k]:.9g} {px[1, k]:.9g} {px[2, k]:.9g}")
    out = subprocess.run([str(exe)], input=f"{len(lines)}\n" + "\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=120)
    got = np.array([[float(v) for v in l.split()] for l in out.stdout.splitlines()], np.float32).astype(np.float64).reshape(len(groups), npx, 3)
    worst = 0.0
    for g, (C, order, f, gray, m, stop) in zip(got, groups):
        r64 = ref_pixels(px, C, order, f, gray, m, stop, np.float64)
        r32 = ref_pixels(px, C, order, f, gray, m, stop, np.float32)
        rows = slice(0, 3 if (C == 3 or stop) else 1)
        tol = 4.0 * float(np.abs(r32.astype(np.float64) - r64)[rows].max())
        err = float(np.abs(g.T - r64)[rows].max())
        worst = max(worst, err / tol if tol > 0 else float(err > 0))
        assert tol < T.ALLOWANCE_CAP
        assert err <= tol, f"C {C} order {order} {R.order_of(order)} gray {gray} stop {stop}: {err:.3e} > {tol:.3e}"
    print(f"{len(groups)} groups of {npx} pixels: worst error / allowance {worst:.3f}")
