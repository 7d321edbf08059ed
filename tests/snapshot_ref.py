"""The two partials of spv_snapshot_multi (include/spv.h) restated with numpy, from the header's words and nothing else: a job's checksum
-- the sum, mod 2^64, of its bytes read as little-endian 32-bit words from the job's start, the last partial word zero-padded -- and its
count of fp32 values with an all-ones exponent.  Also the per-chunk form, so that a test can fold chunks in any order."""
import numpy as np

MASK = (1 << 64) - 1


def _bytes(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)


def checksum(data):
    """Python integers throughout: no fixed-width arithmetic that could hide a wrap"""
    b = _bytes(data).tolist()
    total = 0
    for i in range(0, len(b), 4):
        word = b[i:i + 4] + [0] * (4 - len(b[i:i + 4]))
        total += word[0] | word[1] << 8 | word[2] << 16 | word[3] << 24
    return total & MASK


def nonfinite(data, kind):
    """kind 1: the whole 32-bit words with exponent bits 30..23 all ones; any other kind: 0"""
    if kind != 1:
        return 0
    b = _bytes(data)
    words = b[:b.size // 4 * 4].view("<u4")
    return int(((words >> 23) & 0xFF == 0xFF).sum())


def chunk_partials(data, kind, chunk_bytes):
    """[(offset, checksum of the chunk, non-finite count of the chunk)] for chunks of chunk_bytes (a multiple of 16) from the job's start"""
    b = _bytes(data)
    return [(off, checksum(b[off:off + chunk_bytes]), nonfinite(b[off:off + chunk_bytes], kind)) for off in range(0, b.size, chunk_bytes)]
