"""spv_snapshot_multi through the raw C-ABI: every job size around the access widths and the chunk size, four dtypes, sources that are
views 1 / 2 / 4 / 8 bytes off a 256-byte boundary, fp32 specials on the first and last element of a chunk; slots fenced by guard bytes in
a pre-filled staging buffer.  Copies bit for bit, guards intact, folded checksums and non-finite counts equal to the numpy restatement
(tests/snapshot_ref.py), the same job checksums under two chunk sizes, the host refusals, and stream order: a snapshot followed at once by
optimizer steps on the same tensors holds what the tensors held before."""
import numpy as np
import pytest
import torch

import snapshot_ref as R

pytestmark = pytest.mark.gpu

CHUNKS = (64, 4096)
SIZES = sorted({0, 1, 3, 4, 15, 16, 17} | {s for c in CHUNKS for s in (c - 1, c, c + 1, 3 * c + 5)})
DTYPES = ("uint8", "bfloat16", "float32", "int64")
OFFSETS = (0, 1, 2, 4, 8)   # bytes off a 256-byte boundary
GUARD, FILL, FENCE = 64, 0x5A, 0xA5
SPECIALS = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x00000001, 0x807FFFFF, 0x80000000, 0x7F7FFFFF], dtype=np.uint32)
#                    +inf        -inf        NaN         NaN         denormals               -0.0        the largest finite


def _job_bytes(rng, size, dtype):
    """`size` bytes of a `dtype` array; fp32: specials on the first and last element of every chunk of both chunk sizes"""
    raw = rng.integers(0, 256, size + 8, dtype=np.uint8)
    if dtype == "float32":
        words = raw[:(size + 8) // 4 * 4].view("<u4")
        words[:] = rng.standard_normal(words.size).astype(np.float32).view("<u4")
        k, n = 0, size // 4   # the job's whole elements
        for c in CHUNKS:
            for first in range(0, n, c // 4):
                for e in (first, min(first + c // 4, n) - 1):
                    words[e] = SPECIALS[k % SPECIALS.size]
                    k += 1
    elif dtype == "int64" and size % 3 == 0:
        raw[:] = 0xFF   # NaN bit patterns in a job that is not counted
    return raw[:size].copy()


@pytest.fixture(scope="module")
def case():
    """the jobs, their arena of sources and the staging layout, built once: (jobs as dicts, source arena, staging length)"""
    rng = np.random.default_rng(20)
    jobs, src_at, dst_at = [], 256, 256
    for size in SIZES:
        for dtype in DTYPES:
            for off in OFFSETS:
                data = _job_bytes(rng, size, dtype)
                jobs.append(dict(size=size, kind=1 if dtype == "float32" else 0, data=data, src=src_at + off, dst=dst_at))
                src_at = -(-(src_at + off + size) // 256) * 256 + 256
                dst_at = -(-(dst_at + size + 2 * GUARD) // 256) * 256
    arena = np.zeros(src_at, dtype=np.uint8)
    for j in jobs:
        arena[j["src"]:j["src"] + j["size"]] = j["data"]
    return jobs, arena, dst_at


def _staging(jobs, total):
    host = np.full(total, FILL, dtype=np.uint8)
    for j in jobs:
        host[j["dst"] - GUARD:j["dst"]] = FENCE
        host[j["dst"] + j["size"]:j["dst"] + j["size"] + GUARD] = FENCE
    return host


def _launch(jobs, arena_dev, staging_dev, chunk):
    from spectre_vit import _native
    from spectre_vit.checkpoint import fold_partials, plan_chunks
    dev = arena_dev.device
    rows = []
    for j in jobs:
        rows += [arena_dev.data_ptr() + j["src"], staging_dev.data_ptr() + j["dst"], j["size"], j["kind"]]
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    chunk_job, chunk_off = plan_chunks([j["size"] for j in jobs], chunk)
    cj, co = torch.tensor(chunk_job, dtype=torch.int32).to(dev), torch.tensor(chunk_off, dtype=torch.int64).to(dev)
    sums = torch.full((len(chunk_job),), -1, dtype=torch.int64, device=dev)
    bad = torch.full((len(chunk_job),), -1, dtype=torch.int32, device=dev)
    _native.call("spv_snapshot_multi", table.data_ptr(), cj.data_ptr(), co.data_ptr(), len(chunk_job), chunk, sums.data_ptr(),
                 bad.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return fold_partials(chunk_job, sums.cpu().numpy().view(np.uint64).tolist(), bad.cpu().tolist(), len(jobs))


@pytest.fixture(scope="module")
def results(case):
    """both chunk sizes run once: chunk -> (the staging buffer afterwards, the folded checksums, the folded counts)"""
    import __graft_entry__ as g
    g.build()
    jobs, arena, total = case
    assert all(j["dst"] % 256 == 0 for j in jobs) and all((j["src"] - o) % 256 == 0 for j, o in zip(jobs, OFFSETS * (len(jobs) // 5)))
    arena_dev = torch.from_numpy(arena).cuda()
    assert arena_dev.data_ptr() % 256 == 0
    out = {}
    for chunk in CHUNKS:
        staging = torch.from_numpy(_staging(jobs, total)).cuda()
        assert staging.data_ptr() % 256 == 0
        sums, bad = _launch(jobs, arena_dev, staging, chunk)
        out[chunk] = (staging.cpu().numpy(), sums, bad)
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
def test_copies_are_bit_exact_and_guards_intact(case, results, chunk):
    jobs, _, total = case
    got = results[chunk][0]
    want = _staging(jobs, total)
    for j in jobs:
        want[j["dst"]:j["dst"] + j["size"]] = j["data"]
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, f"first differing staging byte at {wrong[:5]}: every job's bytes, every guard and fill byte around them"


@pytest.mark.parametrize("chunk", CHUNKS)
def test_checksums_and_counts_equal_the_restatement(case, results, chunk):
    jobs = case[0]
    _, sums, bad = results[chunk]
    for i, j in enumerate(jobs):
        assert sums[i] == R.checksum(j["data"]), (i, j["size"], j["kind"], j["src"] % 256)
        assert bad[i] == R.nonfinite(j["data"], j["kind"]), (i, j["size"], j["kind"], j["src"] % 256)
    assert any(b > 0 for b in bad), "the fp32 jobs hold inf and NaN"
    assert all(b == 0 for b, j in zip(bad, jobs) if j["kind"] == 0), "a job that is not fp32 is not counted, whatever its bits"
    assert any(j["kind"] == 0 and j["size"] >= 4 and R.nonfinite(j["data"], 1) > 0 for j in jobs), "... and some do hold NaN patterns"


def test_two_chunk_sizes_give_the_same_job_checksums(results):
    assert results[CHUNKS[0]][1] == results[CHUNKS[1]][1] and results[CHUNKS[0]][2] == results[CHUNKS[1]][2]


def test_host_refusals_launch_nothing(results):
    from spectre_vit import _native
    lib = _native.load()
    dev = torch.device("cuda")
    src = torch.arange(64, dtype=torch.uint8, device=dev)
    dst = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    table = torch.tensor([src.data_ptr(), dst.data_ptr(), 64, 0], dtype=torch.int64).to(dev)
    cj, co = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    sums, bad = torch.full((1,), -1, dtype=torch.int64, device=dev), torch.full((1,), -1, dtype=torch.int32, device=dev)
    good = [table.data_ptr(), cj.data_ptr(), co.data_ptr(), 1, 64, sums.data_ptr(), bad.data_ptr()]
    st = torch.cuda.current_stream().cuda_stream
    refused = [(0, 0, "null table"), (1, 0, "null table"), (2, 0, "null table"), (5, 0, "null chunk_sum"), (6, 0, "null chunk_sum"),
               (3, -1, "nchunks"), (4, 0, "multiple of 16"), (4, -16, "multiple of 16"), (4, 24, "multiple of 16")]
    for at, value, message in refused:
        args = list(good)
        args[at] = value
        assert lib.spv_snapshot_multi(*args, st) != 0, (at, value)
        assert message in lib.spv_last_error().decode(), (at, value)
        with pytest.raises(RuntimeError, match="spv_snapshot_multi"):
            _native.call("spv_snapshot_multi", *args, st)
    assert lib.spv_snapshot_multi(0, 0, 0, 0, 64, 0, 0, st) == 0, "no chunk: nothing to check, nothing to launch"
    torch.cuda.synchronize()
    assert (dst == FILL).all() and int(sums[0]) == -1 and int(bad[0]) == -1, "no refused call launched"
    _native.call("spv_snapshot_multi", *good, st)
    torch.cuda.synchronize()
    assert dst.equal(src) and int(sums[0]) == R.checksum(src.cpu().numpy()) and int(bad[0]) == 0


def test_a_snapshot_is_in_stream_order(results, tmp_path):
    """taken and followed AT ONCE by three optimizer steps on the same tensors: the file holds what clones made before the take hold"""
    from spectre_vit.checkpoint import FILE_NAME, StateSnapshot, load_train_state
    from spectre_vit.optim import FusedAdamW
    g = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(shape, generator=g).cuda()) for shape in ((257, 33), (1,), (4099,), (64, 64))]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).cuda()
    opt = FusedAdamW(params, lr=0.1, capturable=True, ema_decay=0.5, accumulate_steps=2)
    opt.step()   # the state exists from here on
    blocks = [(f"model/{i}", p.detach()) for i, p in enumerate(params)] + opt.state_blocks()[0]
    assert {"optim/0/exp_avg", "optim/0/step", "optim/3/ema", "optim/control_block", "optim/accumulators/0"} <= {n for n, _ in blocks}
    assert sum(n.endswith("/step") for n, _ in blocks) == 1, "the group's one step count is one job"
    reports = []
    snap = StateSnapshot(blocks, str(tmp_path), gated={"model/0"}, report=reports.append, chunk_bytes=4096)
    before = [t.clone() for _, t in blocks]
    snap.take({"fingerprint": {}, "epoch": 1}, 1)
    for _ in range(3):
        opt.step()
    snap.close()
    torch.cuda.synchronize()
    assert not params[0].detach().equal(before[0]), "the steps behind the take did move the weights"
    state = load_train_state(str(tmp_path / FILE_NAME))
    for (name, _), want in zip(blocks, before):
        got = state["tensors"][name]
        assert got.dtype == want.dtype and got.shape == want.shape and got.reshape(-1).view(torch.uint8).equal(
            want.cpu().reshape(-1).view(torch.uint8)), name
    rec = reports[0]["Checkpoint"]
    assert len(reports) == 1 and list(rec) == ["epoch", "bytes", "take_ms", "wait_ms", "write_ms"] and rec["epoch"] == 1
    assert sorted(p.name for p in tmp_path.iterdir()) == [FILE_NAME]
