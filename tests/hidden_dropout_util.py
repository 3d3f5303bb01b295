"""numpy restatement of the fused hidden dropout's keep function (rankpo_amd/csrc/bert_ops.hip `hidden_keep`), written from its
description and not from the kernel's code path: Philox2x32-10 with counter (row, column >> 2), a 32-bit key mixed (murmur3
finaliser) from the 64-bit seed and the site, four 16-bit fields of the 64 output bits, one per column of the group of 4; a column
is KEPT when its field >= thr = round(p * 65536).  tests/test_hidden_dropout_host.py checks its statistics on the CPU,
tests/test_gpu_hidden_dropout.py compares the kernels' dump with it bit for bit."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M = np.uint64(0xD256D193)
WEYL = 0x9E3779B9
SEEDS = (0x1234567887654321, 987654321987, 2 ** 63 - 2)      # the call seeds the tests use (before ops.bert_hidden_seed)


def _fmix32(x: int) -> int:
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def key32(seed: int, site: int) -> int:
    seed &= 0xFFFFFFFFFFFFFFFF
    return _fmix32((seed & 0xFFFFFFFF) ^ _fmix32((seed >> 32) ^ _fmix32((site + WEYL) & 0xFFFFFFFF)))


def threshold(p: float) -> int:
    """round(p * 65536) as the library takes it: p as float32, round half to even."""
    return int(np.rint(np.float32(p) * np.float32(65536.0)))


def scale(p: float) -> float:
    """1 / (1 - p) in float32 arithmetic; 1 when p quantises to no dropout."""
    if threshold(p) == 0:
        return 1.0
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def philox2x32_10(key: int, c0, c1):
    """c0, c1: uint64 arrays holding 32-bit values -> the two output words (uint64 arrays below 2^32)."""
    c0 = np.asarray(c0, dtype=np.uint64) & M32
    c1 = np.asarray(c1, dtype=np.uint64) & M32
    c0, c1 = np.broadcast_arrays(c0, c1)
    k = key & 0xFFFFFFFF
    for _ in range(10):
        prod = PHILOX_M * c0                       # < 2^64: both factors are below 2^32
        c0, c1 = (prod >> np.uint64(32)) ^ np.uint64(k) ^ c1, prod & M32
        k = (k + WEYL) & 0xFFFFFFFF
    return c0, c1


def hidden_keep(seed: int, site: int, row0: int, rows: int, d: int, p: float) -> np.ndarray:
    """uint8 [rows, d]: 1 = kept, for packed rows row0 .. row0 + rows - 1 of `site`; `seed` as the kernels get it."""
    r = np.arange(row0, row0 + rows, dtype=np.uint64)[:, None]
    c = np.arange(d, dtype=np.uint64)[None, :]
    w0, w1 = philox2x32_10(key32(seed, site), r, c >> np.uint64(2))
    word = np.where((c & np.uint64(2)) != 0, w1, w0)
    field = (word >> (np.uint64(16) * (c & np.uint64(1)))) & np.uint64(0xFFFF)
    return (field >= np.uint64(threshold(p))).astype(np.uint8)
