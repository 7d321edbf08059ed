"""spv_dataset_ingest through the raw C-ABI, every comparison BIT-EXACT against numpy (transpose; sums in Python integers): both
layouts, shapes from 1 x 1 x 1 to whole-image groups and (beyond 8192 pixels) pixel tiles, image counts around a group's size, sources
0 / 1 / 3 / 16 bytes and destinations 0 / 1 byte off a 256-byte boundary with guard bytes around the destination, all-zero and all-255
sets (the latter where a 32-bit sum of squares would wrap), uint8 and int64 labels with out-of-range values, chunked calls into one
statistics block, statistics only (dst NULL), the round trip, more units than the launch has workgroups, and the host refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 7), (1, 28, 28), (3, 32, 32), (3, 64, 64), (1, 2, 512)]
NS = (1, 2, 3, 64, 65, 257)
TILED = [((3, 91, 97), (1, 3)), ((1, 100, 100), (1, 2)), ((3, 512, 512), (1,))]   # above 8192 pixels an image is walked in tiles
SRC_OFFSETS, DST_OFFSETS = (0, 1, 3, 16), (0, 1)
PLANAR, INTERLEAVED = 0, 1
U8, I64 = 0, 1
GUARD, FENCE = 256, 0xA5


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _other(x, c, h, w, layout):
    """the flat bytes of a set in `layout` -> the flat bytes of the other layout (numpy transpose)"""
    if layout == PLANAR:
        return np.ascontiguousarray(x.reshape(-1, c, h, w).transpose(0, 2, 3, 1)).reshape(-1)
    return np.ascontiguousarray(x.reshape(-1, h, w, c).transpose(0, 3, 1, 2)).reshape(-1)


def _want_stats(x, c, h, w, layout, labels=None, classes=0):
    """the statistics block as Python integers"""
    planes = (x.reshape(-1, c, h * w) if layout == PLANAR else x.reshape(-1, h * w, c).transpose(0, 2, 1)).astype(np.int64)
    n = planes.shape[0]
    out = [int(planes[:, k].sum()) for k in range(c)] + [int((planes[:, k] ** 2).sum()) for k in range(c)] + [n * h * w, 0] + [0] * classes
    for v in ([] if labels is None else labels.tolist()):
        if 0 <= v < classes:
            out[2 * c + 2 + v] += 1
        else:
            out[2 * c + 1] += 1
    return out


def _at(data, off):
    """a device copy of `data`'s bytes `off` bytes past a 256-byte boundary -> (the buffer that owns them, their address)"""
    data = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1)).cuda()
    buf = torch.zeros(256 + off + data.numel() + 16, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 256 + off
    buf[start:start + data.numel()].copy_(data)
    return buf, buf.data_ptr() + start


def _ingest(src_ptr, dst_ptr, labels_ptr, label_dtype, stats, n, c, h, w, layout, classes):
    from spectre_vit import _native
    _native.call("spv_dataset_ingest", src_ptr, dst_ptr, labels_ptr, label_dtype, stats.data_ptr(), n, c, h, w, layout, classes,
                 torch.cuda.current_stream().cuda_stream)


def _stats_block(c, classes):
    from spectre_vit import _native
    words = _native.call("spv_dataset_stats_words", c, classes)
    assert words == 2 * c + 2 + classes
    return torch.zeros(words, dtype=torch.int64, device="cuda")


def _read(stats):
    return [int(v) & (2 ** 64 - 1) for v in stats.tolist()]


def _case(x, c, h, w, layout, src_off=0, dst_off=0, src_dev=None, want_dev=None):
    """one call on the flat bytes `x`: the destination fenced by guard bytes -> the statistics; asserts the bytes and the guards"""
    n = x.size // (c * h * w)
    src_buf, src_ptr = _at(x if src_dev is None else src_dev, src_off)
    out = torch.full((GUARD + 256 + dst_off + x.size + GUARD,), FENCE, dtype=torch.uint8, device="cuda")
    start = GUARD + (-(out.data_ptr() + GUARD)) % 256 + dst_off   # GUARD fence bytes at the least on either side
    stats = _stats_block(c, 0)
    _ingest(src_ptr, out.data_ptr() + start, 0, U8, stats, n, c, h, w, layout, 0)
    want = torch.from_numpy(_other(x, c, h, w, layout)).cuda() if want_dev is None else want_dev
    where = (c, h, w, n, layout, src_off, dst_off)
    assert torch.equal(out[start:start + x.size], want), where
    assert bool((out[:start] == FENCE).all()) and bool((out[start + x.size:] == FENCE).all()), ("a guard byte was written", where)
    return _read(stats)


def _grid(shape, ns, seed):
    c, h, w = shape
    rng = np.random.default_rng(seed)
    for n in ns:
        x = rng.integers(0, 256, size=n * c * h * w, dtype=np.uint8)
        src_dev = torch.from_numpy(x).cuda()
        for layout in (PLANAR, INTERLEAVED):
            want_stats = _want_stats(x, c, h, w, layout)
            want_dev = torch.from_numpy(_other(x, c, h, w, layout)).cuda()
            for src_off in SRC_OFFSETS:
                for dst_off in DST_OFFSETS:
                    got = _case(x, c, h, w, layout, src_off, dst_off, src_dev, want_dev)
                    assert got == want_stats, (shape, n, layout, src_off, dst_off)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_bytes(shape):
    _grid(shape, NS, seed=sum(shape))


@pytest.mark.parametrize("shape,ns", TILED, ids=lambda s: "x".join(map(str, s)) if len(s) == 3 else None)
def test_images_walked_in_tiles(shape, ns):
    _grid(shape, ns, seed=7 + sum(shape))


def test_more_units_than_workgroups():
    """4100 images of 65 x 64 > 4096 pixels are 4100 one-image units: the launch's 1024 workgroups walk four or five each, and
    keep their sums across them"""
    c, h, w, n = 1, 65, 64, 4100
    x = np.random.default_rng(11).integers(0, 256, size=n * c * h * w, dtype=np.uint8)
    assert _case(x, c, h, w, PLANAR, 3, 1) == _want_stats(x, c, h, w, PLANAR)
    c, h, w, n = 3, 37, 37, 5000   # 1369 pixels: groups of five images, 1000 units
    x = np.random.default_rng(12).integers(0, 256, size=n * c * h * w, dtype=np.uint8)
    assert _case(x, c, h, w, INTERLEAVED, 1, 1) == _want_stats(x, c, h, w, INTERLEAVED)


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
def test_all_zero_and_all_255(layout):
    for (c, h, w), n in (((3, 5, 7), 65), ((1, 28, 28), 3), ((3, 91, 97), 1)):
        x = np.zeros(n * c * h * w, dtype=np.uint8)
        assert _case(x, c, h, w, layout, 1, 1) == [0] * (2 * c) + [n * h * w, 0]
    # 70 images of 32 x 32: 71 680 pixels per channel, sum x^2 = 4.66e9 > 2^32 -- a 32-bit partial anywhere would show
    c, h, w, n = 3, 32, 32, 70
    x = np.full(n * c * h * w, 255, dtype=np.uint8)
    pixels = n * h * w
    assert pixels * 255 * 255 > 2 ** 32
    assert _case(x, c, h, w, layout, 3, 1) == [pixels * 255] * 3 + [pixels * 255 * 255] * 3 + [pixels, 0]


@pytest.mark.parametrize("label_off", [0, 1, 3])
def test_labels_are_histogrammed_and_the_strays_counted(label_off):
    c, h, w, n, classes = 3, 5, 7, 300, 100
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, size=n * c * h * w, dtype=np.uint8)
    _, src_ptr = keep = _at(x, 0)
    # uint8: 200 is outside [0, 100)
    lab8 = rng.integers(0, classes, size=n).astype(np.uint8)
    lab8[[0, 17, 299]] = 200
    lab_buf, lab_ptr = _at(lab8, label_off)
    stats = _stats_block(c, classes)
    _ingest(src_ptr, 0, lab_ptr, U8, stats, n, c, h, w, PLANAR, classes)
    assert _read(stats) == _want_stats(x, c, h, w, PLANAR, lab8.astype(np.int64), classes)
    assert _read(stats)[2 * c + 1] == 3
    # int64: -1 and 2^40 are outside; the values sit at any alignment
    lab64 = rng.integers(0, classes, size=n).astype(np.int64)
    lab64[[1, 2, 150]] = -1
    lab64[[298, 299]] = 2 ** 40
    lab_buf, lab_ptr = _at(lab64, label_off)
    stats = _stats_block(c, classes)
    _ingest(src_ptr, 0, lab_ptr, I64, stats, n, c, h, w, PLANAR, classes)
    assert _read(stats) == _want_stats(x, c, h, w, PLANAR, lab64, classes)
    assert _read(stats)[2 * c + 1] == 5 and sum(_read(stats)[2 * c + 2:]) == n - 5
    # up to 1024 classes a workgroup keeps the histogram in LDS, above that it adds label by label: both sides of the threshold
    for many in (1024, 1025, 5000):
        wide = rng.integers(0, many, size=n).astype(np.int64)
        wide[[0, 299]] = [many - 1, many]
        lab_buf, lab_ptr = _at(wide, label_off)
        stats = _stats_block(c, many)
        _ingest(src_ptr, 0, lab_ptr, I64, stats, n, c, h, w, PLANAR, many)
        assert _read(stats) == _want_stats(x, c, h, w, PLANAR, wide, many) and _read(stats)[2 * c + 1] == 1, many
    # a tiled image's label is counted once, by its first tile
    c, h, w, n = 3, 91, 97, 2
    x = rng.integers(0, 256, size=n * c * h * w, dtype=np.uint8)
    big = _at(x, 0)
    lab_buf, lab_ptr = _at(np.array([7, 7], dtype=np.uint8), label_off)
    stats = _stats_block(c, 10)
    _ingest(big[1], 0, lab_ptr, U8, stats, n, c, h, w, INTERLEAVED, 10)
    assert _read(stats) == _want_stats(x, c, h, w, INTERLEAVED, np.array([7, 7]), 10)
    del keep


@pytest.mark.parametrize("shape,n,cuts", [((3, 5, 7), 257, (100, 101)), ((3, 32, 32), 70, (33,)), ((1, 28, 28), 65, (1, 64))])
@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
def test_chunked_calls_into_one_block_equal_one_call(shape, n, cuts, layout):
    c, h, w = shape
    per, classes = c * h * w, 10
    rng = np.random.default_rng(n)
    x = rng.integers(0, 256, size=n * per, dtype=np.uint8)
    labels = rng.integers(0, classes, size=n).astype(np.uint8)
    src_buf, src_ptr = _at(x, 0)
    lab_buf, lab_ptr = _at(labels, 0)
    want = torch.from_numpy(_other(x, c, h, w, layout)).cuda()
    whole = torch.zeros(n * per, dtype=torch.uint8, device="cuda")
    one = _stats_block(c, classes)
    _ingest(src_ptr, whole.data_ptr(), lab_ptr, U8, one, n, c, h, w, layout, classes)
    parts = torch.zeros(n * per, dtype=torch.uint8, device="cuda")
    many = _stats_block(c, classes)
    edges = (0,) + cuts + (n,)
    for a, b in zip(edges, edges[1:]):   # a chunk of 3 x 5 x 7 images starts anywhere
        _ingest(src_ptr + a * per, parts.data_ptr() + a * per, lab_ptr + a, U8, many, b - a, c, h, w, layout, classes)
    assert torch.equal(whole, want) and torch.equal(parts, want)
    assert _read(one) == _read(many) == _want_stats(x, c, h, w, layout, labels.astype(np.int64), classes)


@pytest.mark.parametrize("shape,n", [((3, 5, 7), 65), ((3, 32, 32), 9), ((3, 91, 97), 2), ((1, 28, 28), 11)])
def test_statistics_only_and_the_round_trip(shape, n):
    c, h, w = shape
    x = np.random.default_rng(n).integers(0, 256, size=n * c * h * w, dtype=np.uint8)
    for layout in (PLANAR, INTERLEAVED):
        src_buf, src_ptr = _at(x, 1)
        before = src_buf.clone()
        stats = _stats_block(c, 0)
        _ingest(src_ptr, 0, 0, U8, stats, n, c, h, w, layout, 0)   # dst NULL: the same statistics, nothing written
        assert _read(stats) == _want_stats(x, c, h, w, layout) and torch.equal(src_buf, before)
    # planar -> interleaved -> planar is the identity
    src_buf, src_ptr = _at(x, 3)
    mid = torch.zeros(x.size + 1, dtype=torch.uint8, device="cuda")
    back = torch.zeros(x.size, dtype=torch.uint8, device="cuda")
    a, b = _stats_block(c, 0), _stats_block(c, 0)
    _ingest(src_ptr, mid.data_ptr() + 1, 0, U8, a, n, c, h, w, PLANAR, 0)
    _ingest(mid.data_ptr() + 1, back.data_ptr(), 0, U8, b, n, c, h, w, INTERLEAVED, 0)
    assert torch.equal(back, torch.from_numpy(x).cuda()) and _read(a) == _read(b)


def test_host_refusals_launch_nothing():
    from spectre_vit import _native
    lib = _native.load()
    c, h, w, n = 3, 5, 7, 4
    x = np.arange(n * c * h * w, dtype=np.uint8)
    src_buf, src_ptr = _at(x, 0)
    dst = torch.full((x.size,), FENCE, dtype=torch.uint8, device="cuda")
    stats = _stats_block(c, 10)
    st = torch.cuda.current_stream().cuda_stream
    good = [src_ptr, dst.data_ptr(), 0, U8, stats.data_ptr(), n, c, h, w, PLANAR, 10]
    refused = [(6, 2, "c = 2"), (7, 0, "h = 0"), (8, 513, "w = 513"), (5, -1, "n = -1"), (5, 1 << 31, "n = 2147483648"), (9, 2, "src_layout"),
               (10, -1, "classes"), (3, 2, "label_dtype"), (4, 0, "stats"), (4, stats.data_ptr() + 4, "8-byte aligned"), (0, 0, "null src"),
               (1, src_ptr + 8, "overlap")]
    for at, value, message in refused:
        args = list(good)
        args[at] = value
        assert lib.spv_dataset_ingest(*args, st) != 0, (at, value)
        assert message in lib.spv_last_error().decode(), (at, value, lib.spv_last_error().decode())
        with pytest.raises(RuntimeError, match="spv_dataset_ingest"):
            _native.call("spv_dataset_ingest", *args, st)
    args = list(good)
    args[5] = 0
    assert lib.spv_dataset_ingest(*args, st) == 0, "n == 0 launches nothing"
    torch.cuda.synchronize()
    assert bool((dst == FENCE).all()) and _read(stats) == [0] * (2 * c + 2 + 10), "no refused call launched"
    _native.call("spv_dataset_ingest", *good, st)
    assert torch.equal(dst, torch.from_numpy(_other(x, c, h, w, PLANAR)).cuda()) and _read(stats)[2 * c] == n * h * w
