"""Numpy restatement of the counter-based generator of csrc/common.h, independent of the library: Philox4x32 in uint64
arithmetic (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers pin it in
tests/test_philox_ref_host.py), the counter layout of the dropout sites, the two threshold rules and the two element layouts
of nrms_dropout_keep_mask (include/nrms_hip.h)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
FIELDS16 = 0x100                            # NRMS_DROPOUT_FIELDS16
RANK_SALT = 0x632BE59BD9B4E019              # run_v0.py: model._rank_salt = rank * RANK_SALT
MASK64 = 0xFFFFFFFFFFFFFFFF


def philox4x32(counter4, key2, rounds):
    """Philox4x32-`rounds`.  counter4: four uint32 words (scalars or equal-shaped arrays), key2: two -> four uint64 arrays that
    hold 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & M32 for c in counter4))
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key2)
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def philox4x32_7(seed, group, site):
    """csrc/common.h philox4x32_7: counter (group lo, group hi, site, 0x9E3779B9), key (seed lo, seed hi), 7 rounds."""
    group = np.asarray(group, dtype=np.uint64)
    seed = int(seed) & MASK64
    return philox4x32((group & M32, group >> S32, np.full_like(group, site), np.full_like(group, 0x9E3779B9)),
                      (seed & 0xFFFFFFFF, seed >> 32), 7)


def drop_threshold(p):
    """csrc/common.h drop_threshold: uint32(p * 2^32) of the fp32 probability the C ABI receives, clamped to [0, 2^32 - 1]."""
    t = float(np.float32(p)) * 4294967296.0
    return 0 if t <= 0.0 else (4294967295 if t >= 4294967295.0 else int(t))


def drop_threshold16(p):
    """csrc/common.h drop_threshold16: uint32(p * 2^16), clamped to [0, 65535]."""
    t = float(np.float32(p)) * 65536.0
    return 0 if t <= 0.0 else (65535 if t >= 65535.0 else int(t))


def inv_keep(p):
    """The scale of a kept element, as make_dropout forms it: fp32 1 / (1 - p), from p and not from the quantised threshold."""
    p = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p) if p > 0 else np.float32(1.0)


def words32(seed, site, n):
    """uint64 [n]: the 32-bit word of every element of a flat layout -- element i takes word i & 3 of call i >> 2."""
    assert n % 4 == 0
    return np.stack(philox4x32_7(seed, np.arange(n // 4, dtype=np.uint64), site), axis=1).reshape(n)


def fields16(seed, site, n):
    """uint64 [n]: the 16-bit field of every element -- 8 elements per call; the low 16 bits of word w go to element 2 w, the high
    16 bits to element 2 w + 1."""
    assert n % 8 == 0
    w = np.stack(philox4x32_7(seed, np.arange(n // 8, dtype=np.uint64), site & 0xFF), axis=1)            # [calls, 4]
    return np.stack([w & np.uint64(0xFFFF), w >> np.uint64(16)], axis=2).reshape(n)                    # [calls, 4, (lo, hi)]


def keep_mask(seed, site, n_rows, d, p):
    """[n_rows, d] uint8: keep <=> word >= drop_threshold(p)."""
    return (words32(seed, site, n_rows * d) >= np.uint64(drop_threshold(p))).astype(np.uint8).reshape(n_rows, d)


def keep_mask16(seed, site, n_rows, d, p):
    """[n_rows, d] uint8, the 16-bit-field scheme: keep <=> field >= drop_threshold16(p)."""
    return (fields16(seed, site, n_rows * d) >= np.uint64(drop_threshold16(p))).astype(np.uint8).reshape(n_rows, d)


def export_mask(seed, site, n_rows, d, p):
    """What nrms_dropout_keep_mask(seed, site, n_rows, d, p) writes."""
    return keep_mask16(seed, site, n_rows, d, p) if site & FIELDS16 else keep_mask(seed, site, n_rows, d, p)


def fp16_column_source(n_cols):
    """The fp16 kernels' column permutation: the mask of column 16 a + 8 b + 4 c + e is the field at 16 a + 8 c + 4 b + e (the
    two middle bits of the index inside a 16-column block swapped).  -> int64 [n_cols], source column of every column."""
    col = np.arange(n_cols, dtype=np.int64)
    return (col & ~np.int64(12)) | ((col & 8) >> 1) | ((col & 4) << 1)


def next_seed(initial_seed, calls, rank_salt=0):
    """_FlatModel._next_seed after it has advanced the call counter to `calls`."""
    return (int(initial_seed) * 0x9E3779B97F4A7C15 + int(calls) * 0xD1B54A32D192ED03 + int(rank_salt)) & MASK64
