"""The resident loader, the host side (no GPU): the permutation and the position rule of csrc/spv_loader_core.h -- compiled by the host
compiler into a stand-alone program -- and of ResidentLoader.indices against the numpy restatement tests/loader_ref.py, bit for bit;
the bijection; the shuffle's quality against the uniform permutation's own distribution; the sharding; the ABI; every refusal of the
C entry point and of the Python layers, none of which touches a device."""
import os
import subprocess

import numpy as np
import pytest
import torch

import loader_ref as R

NS = (1, 2, 3, 7, 64, 1000, 4096, 50000)
SEEDS = (0, 42, 2 ** 63 + 5)
EPOCHS = (0, 1, 2 ** 31)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return True


CORE_MAIN = r"""
#include "spv_loader_core.h"
#include <stdio.h>
#include <string.h>
// stdin, one query per line.  "perm n seed epoch": n lines, the image of 0 .. n-1.  "pos n batch world rank steps t": `batch` lines
// "position epoch" of step t (the cursor's 64 bits, unsigned).  "idx n batch world rank steps shuffle seed t": `batch` rows of the set.
int main() {
    char what[8];
    unsigned long long n, batch, world, rank, steps, shuffle, seed, epoch, t;
    while (scanf("%7s", what) == 1) {
        if (!strcmp(what, "perm")) {
            if (scanf("%llu %llu %llu", &n, &seed, &epoch) != 3) return 1;
            const uint64_t k = ldr_key(seed, epoch);
            for (uint32_t x = 0; x < n; ++x) printf("%u\n", ldr_permute(k, (uint32_t)n, x));
        } else if (!strcmp(what, "pos")) {
            if (scanf("%llu %llu %llu %llu %llu %llu", &n, &batch, &world, &rank, &steps, &t) != 6) return 1;
            const LdrGeom g{(uint32_t)n, (uint32_t)batch, (uint32_t)world, (uint32_t)rank, (uint32_t)steps, 1};
            for (uint32_t r = 0; r < batch; ++r) printf("%u %llu\n", ldr_position(t, r, g), (unsigned long long)ldr_epoch(t, g));
        } else if (!strcmp(what, "idx")) {
            if (scanf("%llu %llu %llu %llu %llu %llu %llu %llu", &n, &batch, &world, &rank, &steps, &shuffle, &seed, &t) != 8) return 1;
            const LdrGeom g{(uint32_t)n, (uint32_t)batch, (uint32_t)world, (uint32_t)rank, (uint32_t)steps, (int)shuffle};
            for (uint32_t r = 0; r < batch; ++r) printf("%u\n", ldr_index(seed, t, r, g));
        } else {
            return 2;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    """the compiled header: core(lines) -> the program's output as an int64 array of the numbers it printed"""
    from conftest import ROOT
    csrc = os.path.join(ROOT, "vit-spectre-experiments_amd", "csrc")
    d = tmp_path_factory.mktemp("loader_core")
    src, exe = d / "core_main.cpp", d / "core_main"
    src.write_text(CORE_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", csrc, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=120)
        return np.array(out.stdout.split(), dtype=np.uint64).astype(np.int64)
    return run


@pytest.fixture(scope="module")
def perms():
    """the restatement's permutations over the whole grid, computed once"""
    return {(n, s, e): R.perm(n, s, e) for n in NS for s in SEEDS for e in EPOCHS}


def test_core_header_equals_the_restatement_bit_for_bit(core, perms):
    for (n, seed, epoch), ref in perms.items():
        got = core([f"perm {n} {seed} {epoch}"])
        assert got.shape == ref.shape and (got == ref).all(), (n, seed, epoch)


def test_python_indices_equal_the_restatement(perms):
    """ResidentLoader.indices is a third statement of the order (the package's own, no library call): one step that covers the whole
    set reproduces the epoch's permutation"""
    from spectre_vit.data import ResidentLoader
    for (n, seed, epoch), ref in perms.items():
        got = ResidentLoader.indices(n, n, seed, epoch, 0, 1, 1, True)   # batch = n, one step per epoch: step == epoch
        assert got.dtype == np.int64 and (got == ref).all(), (n, seed, epoch)
    assert (ResidentLoader.indices(10, 3, 42, 4, 0, 1, 3, False) == np.array([3, 4, 5])).all()   # shuffle off: arange, step 4 = epoch 1 step 1


@pytest.mark.parametrize("n", NS)
def test_bijection(n, perms):
    for seed in SEEDS:
        for epoch in EPOCHS:
            assert (np.sort(perms[(n, seed, epoch)]) == np.arange(n)).all(), (n, seed, epoch)


def shuffle_statistics(rounds):
    """n = 4096, seed 42, epochs 0..15: (total fixed points, total p[i+1] == p[i] + 1, largest |Spearman rho| between consecutive epochs)"""
    ps = [R.perm(4096, 42, e, rounds) for e in range(16)]
    fixed = sum(int((p == np.arange(4096)).sum()) for p in ps)
    adjacent = sum(int((p[1:] == p[:-1] + 1).sum()) for p in ps)
    # a permutation's values are their own ranks, so Spearman's rho is Pearson's r of the two index vectors
    rho = max(abs(float(np.corrcoef(ps[i], ps[i + 1])[0, 1])) for i in range(15))
    return fixed, adjacent, rho


def test_shuffle_quality():
    """conditions from the uniform permutation's own distribution: fixed points and adjacencies over 16 epochs are each Poisson(16)
    (P(> 48) < 1e-9); rho between two independent permutations has sigma 1 / sqrt(n - 1), 0.1 is 6.4 sigma"""
    fixed, adjacent, rho = shuffle_statistics(R.ROUNDS)
    print(f"{R.ROUNDS} rounds: fixed points {fixed}, adjacencies {adjacent}, max |rho| {rho:.4f}")
    assert fixed <= 48 and adjacent <= 48 and rho <= 0.1
    # the caps do catch a weak mixer: the same network with one and two rounds
    _, _, rho1 = shuffle_statistics(1)
    _, adjacent2, rho2 = shuffle_statistics(2)
    print(f"1 round: max |rho| {rho1:.4f}; 2 rounds: adjacencies {adjacent2}, max |rho| {rho2:.4f}")
    assert rho1 > 0.1 and (adjacent2 > 48 or rho2 > 0.1)


@pytest.mark.parametrize("n", (7, 512, 1000))
@pytest.mark.parametrize("B", (1, 3, 64))
@pytest.mark.parametrize("world", (1, 2, 3))
def test_position_rule(n, B, world, core):
    from spectre_vit.data import ResidentLoader
    S = R.steps_per_epoch(n, B, world)
    per_pass = (n // world) // B   # the harness's own count (spectre_vit/harness.py train())
    assert S == per_pass
    if S == 0:   # no whole batch for every rank: refused everywhere
        with pytest.raises(ValueError):
            ResidentLoader.indices(n, B, 42, 0, 0, world, None, True)
        return
    for epoch in (0, 1):
        seen = []
        for rank in range(world):
            for k in range(S):
                t = epoch * S + k
                ref = R.indices(n, B, 42, t, rank, world, S)
                assert (ResidentLoader.indices(n, B, 42, t, rank, world, None, True) == ref).all()
                if k in (0, S - 1):   # the compiled core: first and last step of the epoch
                    assert (core([f"idx {n} {B} {world} {rank} {S} 1 42 {t}"]) == ref).all(), (rank, t)
                seen.append(ref)
        seen = np.concatenate(seen)
        assert seen.size == S * B * world and np.unique(seen).size == seen.size   # disjoint, and exactly S B world samples
        assert seen.min() >= 0 and seen.max() < n
    # whatever 64 bits the cursor holds: every position stays inside the epoch's S B world entries, and the row inside the set
    for t in (-1, 2 ** 63 - 1, 2 ** 64 - 1):
        raw = t & R.U64
        for rank in range(world):
            got = core([f"pos {n} {B} {world} {rank} {S} {raw}"]).reshape(B, 2)
            want, epoch = R.positions(n, B, raw, rank, world, S)
            assert (got[:, 0] == np.array(want)).all() and got[:, 0].max() < S * B * world <= n
            assert (got[:, 1].astype(np.uint64) == np.uint64(epoch)).all()
            rows = core([f"idx {n} {B} {world} {rank} {S} 1 42 {raw}"])
            assert (rows == R.indices(n, B, 42, raw, rank, world, S)).all() and rows.max() < n


def test_abi(built):
    from conftest import ROOT
    from spectre_vit import _native, timing
    lib = _native.load()
    src = open(os.path.join(ROOT, "include", "spv.h")).read()
    assert hasattr(lib, "spv_loader_fetch") and "spv_loader_fetch" in _native.SIGNATURES and "int spv_loader_fetch(" in src
    assert "spv_loader_fetch" in timing._WORK_MODELS, "bench.py's roofline pass brackets every launch it sees"
    assert hasattr(lib, "spv_loader_cursor_bytes") and "int64_t spv_loader_cursor_bytes(" in src
    assert _native.call("spv_loader_cursor_bytes") == 64
    assert len(_native.SIGNATURES["spv_loader_fetch"]) == 21
    # off by default: no census slot, no version change
    assert "#define SPV_LOADER_ROUNDS 6" in src and R.ROUNDS == 6
    assert "SPV_PATH_COUNT = 27" in src and len(_native.PATH) == 27 and lib.spv_version() == 1
    # the work model: (n, batch, chans, height, width, world, rank, steps, shuffle, mode, label dtype, null mask, hint)
    model = timing._WORK_MODELS["spv_loader_fetch"]
    base = (50000, 512, 3, 32, 32, 1, 0, 97, 1)
    assert model(base + (1, 0, 0, 0))[3:] == ("hbm", 512 * (17.0 + 3072 * 5))
    assert model(base + (2, 1, 0, 0))[4] == 512 * (24.0 + 3072 * 2)
    assert model(base + (0, 0, 0, 0))[4] == 512 * 17.0


def test_c_abi_rejects_bad_loader_arguments_before_any_launch(built):
    """as test_step_control.test_c_abi_rejects_bad_step_control_arguments_before_any_launch: every call fails validation on the host
    (non-zero return, spv_last_error text, RuntimeError from the ctypes wrapper), so nothing is launched and no GPU is needed"""
    from spectre_vit import _native
    P = 16   # any non-null, 8-byte aligned "pointer": validation fails before it would be used
    NONE, FLOAT, UINT8 = 0, 1, 2

    def args(src=P, labels_src=P, cursor=P, index=P, labels=P, img=P, mean=P, inv_std=P, n=100, batch=10, chans=3, height=32, width=32,
             world=1, rank=0, steps=10, seed=42, shuffle=1, mode=FLOAT, label_dtype=0):
        return (src, labels_src, cursor, index, labels, img, mean, inv_std, n, batch, chans, height, width, world, rank, steps, seed,
                shuffle, mode, label_dtype, 0)

    cases = [
        (args(labels_src=0), "null labels_src"), (args(cursor=0), "null labels_src"), (args(index=0), "null labels_src"),
        (args(labels=0), "null labels_src"),
        (args(src=0), "null src_nhwc"), (args(img=0), "null src_nhwc"), (args(src=0, mode=UINT8), "null src_nhwc"),
        (args(img=0, mode=UINT8), "null src_nhwc"),
        (args(cursor=12), "8-byte aligned"),
        (args(mean=0), "mean and inv_std"), (args(inv_std=0), "mean and inv_std"),
        (args(n=0), "n = 0"),
        (args(batch=0), "batch"), (args(batch=-3), "batch"),
        (args(world=0), "world"), (args(world=-1), "world"), (args(rank=-1), "rank"), (args(rank=1), "rank"), (args(world=2, rank=2, steps=5), "rank"),
        (args(steps=0), "steps_per_epoch"), (args(steps=-1), "steps_per_epoch"), (args(steps=11), "steps_per_epoch"),
        (args(world=2, rank=1, steps=6), "steps_per_epoch"), (args(n=2 ** 31 - 1, batch=2 ** 16, world=2 ** 8, steps=2 ** 8), "steps_per_epoch"),
        (args(chans=2), "chans"), (args(chans=0), "chans"), (args(chans=4), "chans"),
        (args(height=0), "height"), (args(height=513), "height"), (args(width=0), "width"), (args(width=513), "width"),
        (args(mode=3), "unknown mode"), (args(mode=-1), "unknown mode"),
        (args(label_dtype=2), "unknown label dtype"), (args(label_dtype=-1), "unknown label dtype"),
        (args(n=2 ** 31 - 1, batch=2 ** 24, height=512, width=512, steps=1), "workgroups"),
    ]
    lib = _native.load()
    for a, needle in cases:
        assert lib.spv_loader_fetch(*a) != 0, a
        assert needle in lib.spv_last_error().decode(), (needle, lib.spv_last_error().decode())
        with pytest.raises(RuntimeError) as e:
            _native.call("spv_loader_fetch", *a)
        assert "spv_loader_fetch" in str(e.value) and needle in str(e.value), (needle, str(e.value))


def test_python_refusals_touch_no_device(monkeypatch):
    """every refusal of ResidentLoader, of the graph-replayed steps and of the harness is raised on the host: the library is never
    called (a call would fail this test) and the tensors stay on the CPU"""
    from spectre_vit import _native, graph, harness
    from spectre_vit.data import ResidentLoader

    def no_call(name, *a):
        raise AssertionError(f"{name} called: a refusal must come before any device work")
    monkeypatch.setattr(_native, "call", no_call)
    x = torch.zeros((64, 8, 8, 3), dtype=torch.uint8)
    y = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        ResidentLoader(x.float(), y, 8)
    with pytest.raises(TypeError, match="contiguous"):
        ResidentLoader(x[:, :, :, :1].expand(64, 8, 8, 3), y, 8)
    with pytest.raises(TypeError, match="contiguous"):
        ResidentLoader(x.permute(0, 3, 1, 2), y, 8)   # NCHW view of the set
    with pytest.raises(TypeError, match=r"\(N, H, W, C\)"):
        ResidentLoader(x[0], y, 8)
    with pytest.raises(ValueError, match="channels"):
        ResidentLoader(torch.zeros((64, 8, 8, 2), dtype=torch.uint8), y, 8)
    with pytest.raises(ValueError, match="512"):
        ResidentLoader(torch.zeros((4, 513, 1, 1), dtype=torch.uint8), y[:4], 2)
    with pytest.raises(ValueError, match="512"):
        ResidentLoader(torch.zeros((4, 0, 4, 1), dtype=torch.uint8), y[:4], 2, mean=(0.5,), std=(0.5,))
    with pytest.raises(TypeError, match="labels"):
        ResidentLoader(x, y.float(), 8)
    with pytest.raises(TypeError, match="labels"):
        ResidentLoader(x, y[:63], 8)
    with pytest.raises(TypeError, match="labels"):
        ResidentLoader(x, torch.zeros(128, dtype=torch.int64)[::2], 8)
    with pytest.raises(ValueError, match="mean / std"):
        ResidentLoader(x, y, 8, mean=(0.5,), std=(0.5,))
    with pytest.raises(ValueError, match="mean / std"):
        ResidentLoader(torch.zeros((64, 8, 8, 1), dtype=torch.uint8), y, 8)   # the 3-channel defaults against C = 1
    with pytest.raises(ValueError, match="std must be positive"):
        ResidentLoader(x, y, 8, std=(0.2, 0.0, 0.2))
    with pytest.raises(ValueError, match="n < batch"):
        ResidentLoader(x, y, 65)
    with pytest.raises(ValueError, match="n < batch"):
        ResidentLoader(x, y, 33, rank=1, world=2)
    with pytest.raises(ValueError, match="batch_size"):
        ResidentLoader(x, y, 0)
    for rank, world in ((-1, 1), (1, 1), (0, 0), (3, 3)):
        with pytest.raises(ValueError, match="rank"):
            ResidentLoader(x, y, 8, rank=rank, world=world)
    for steps in (0, 9, -1, True):
        with pytest.raises(ValueError, match="steps_per_epoch"):
            ResidentLoader(x, y, 8, steps_per_epoch=steps)
    with pytest.raises(ValueError, match="output"):
        ResidentLoader(x, y, 8, output="bf16")
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # everything in order but the device: still nothing is launched
        ResidentLoader(x, y, 8)
    with pytest.raises(ValueError, match="no such order"):
        ResidentLoader.indices(64, 8, 42, 0, 0, 1, 9, True)
    # the graph-replayed steps: a loader without an image output, a loader AND an example batch
    fake = type("Loader", (), {"img": None, "labels": y})()
    for cls in (graph.GraphedTrainStep, graph.GraphedDPStep):
        with pytest.raises(ValueError, match="no image output"):
            cls(None, None, None, None, None, loader=fake)
        fake_img = type("Loader", (), {"img": x, "labels": y})()
        with pytest.raises(ValueError, match="comes from the loader"):
            cls(None, None, None, x, y, loader=fake_img)
    # the harness: not with the early distillation form, and a flag is a flag
    with pytest.raises(ValueError, match="device_loader"):
        harness.train("unused", device_loader=True, distill=True)
    with pytest.raises(ValueError, match="device_loader"):
        harness.train("unused", device_loader=1)
    assert harness.build_parser().parse_args(["--device-loader"]).device_loader is True
    assert harness.build_parser().parse_args([]).device_loader is False
    # one permutation for all ranks (they take disjoint parts of it), the config seed's low word as augment_seed(seed, 0)
    assert harness.loader_seed(42) == harness.augment_seed(42, 0) == 42
