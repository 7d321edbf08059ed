"""The resident loader's sample order restated in numpy from its definition in include/spv.h ("the resident loader"): the keyed
bijection of [0, n) and the position rule.  Not a test module; tests/test_resident_loader.py holds csrc/spv_loader_core.h and
ResidentLoader.indices to it bit for bit, tests/test_gpu_resident_loader.py holds the fetch kernel to it."""
import numpy as np

ROUNDS = 6
U64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(x):
    """murmur3's 64-bit finaliser on a Python int"""
    x &= U64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & U64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & U64
    x ^= x >> 33
    return x


def mix32(x):
    """the 32-bit finaliser on a numpy uint32 array (uint64 arithmetic, masked)"""
    x = x.astype(np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def key(seed, epoch):
    return mix64(mix64(seed + GOLDEN) + epoch)


def half_bits(n):
    h = 1
    while (1 << (2 * h)) < n:
        h += 1
    return h


def permute(k, n, x, rounds=ROUNDS):
    """the image of every entry of x (each < n) under the bijection of [0, n) keyed by k"""
    h = half_bits(n)
    mask = np.uint64((1 << h) - 1)
    rk = [np.uint64(mix64(k + (r + 1) * GOLDEN) & 0xFFFFFFFF) for r in range(rounds)]
    x = np.asarray(x, dtype=np.uint64).copy()
    todo = np.ones(x.shape, bool)
    while todo.any():
        v = x[todo]
        left, right = v >> np.uint64(h), v & mask
        for r in range(rounds):
            f = mix32(right + rk[r]) & mask
            left, right = right, left ^ f
        v = (left << np.uint64(h)) | right
        x[todo] = v
        todo[todo] = v >= np.uint64(n)
    return x.astype(np.int64)


def perm(n, seed, epoch, rounds=ROUNDS):
    """the whole permutation of one epoch: perm[position] = row of the set"""
    return permute(key(seed & U64, epoch & U64), n, np.arange(n), rounds)


def steps_per_epoch(n, batch, world):
    return (n // world) // batch


def positions(n, batch, step, rank, world, steps):
    """positions in the epoch's order of the `batch` samples of step `step` (the cursor's 64 bits, unsigned), and the epoch"""
    t = step & U64
    return [((t % steps) * batch + r) * world + rank for r in range(batch)], t // steps


def indices(n, batch, seed, step, rank=0, world=1, steps=None, shuffle=True):
    """int64 rows of the set that rank `rank` fetches at step `step`"""
    steps = steps_per_epoch(n, batch, world) if steps is None else steps
    assert 1 <= steps and steps * batch * world <= n
    pos, epoch = positions(n, batch, step, rank, world, steps)
    pos = np.array(pos, dtype=np.int64)
    return permute(key(seed & U64, epoch), n, pos) if shuffle else pos


def normalise(images_u8_nhwc, index, mean, std):
    """float64 (B, C, H, W): (x / 255 - mean) / std of the rows `index` of the uint8 NHWC set"""
    x = images_u8_nhwc[index].astype(np.float64).transpose(0, 3, 1, 2) / 255.0
    m = np.asarray(mean, np.float64).reshape(1, -1, 1, 1)
    s = np.asarray(std, np.float64).reshape(1, -1, 1, 1)
    return (x - m) / s
