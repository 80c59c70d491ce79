"""Restatement of nrms_softmax_sample_dot's draw (include/nrms_hip.h, "Negatives from the model's own softmax") on top of
tests/philox_ref.py, independent of the library: the two-level words, u, the Gumbel perturbation in fp32 and in float64, the
keys (an exact fp32 fma) and the selection by (key descending, id ascending)."""
import numpy as np

from . import philox_ref as ph

SITE_ROW, SITE_ITEM = 8, 9          # csrc/common.h PHILOX_SITE_SOFTMAX_ROW / _ITEM
G_MAX = 17.4                        # g < 17.4 for every u (u <= 1 - 2^-24)


def row_seeds(seed, row_key):
    """uint64 [B]: level one, words 0 and 1 of philox4x32_7(seed, row_key, site 8)."""
    r = ph.philox4x32_7(seed, np.asarray(row_key, dtype=np.uint64), SITE_ROW)
    return r[0] | (r[1] << ph.S32)


def words(seed, row_key, N):
    """uint32 [B, N]: level two, w(b, n) = word n & 3 of philox4x32_7(row_seed[b], n >> 2, site 9)."""
    rs = row_seeds(seed, np.asarray(row_key, dtype=np.uint64).reshape(-1))[:, None]
    groups = np.arange((N + 3) // 4, dtype=np.uint64)[None, :]
    r = philox4x32_7_keyed(rs, groups, SITE_ITEM)                                    # four [B, groups]
    return np.stack(r, axis=2).reshape(rs.shape[0], -1)[:, :N].astype(np.uint32)


def philox4x32_7_keyed(seed, group, site):
    """philox_ref.philox4x32_7 with an ARRAY of seeds (broadcast against group): one key per row."""
    seed, group = np.broadcast_arrays(np.asarray(seed, dtype=np.uint64), np.asarray(group, dtype=np.uint64))
    c0, c1, c2, c3 = group & ph.M32, group >> ph.S32, np.full_like(group, site), np.full_like(group, 0x9E3779B9)
    k0, k1 = seed & ph.M32, seed >> ph.S32
    for _ in range(7):
        p0, p1 = ph.PHILOX_M0 * c0, ph.PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> ph.S32) ^ c1 ^ k0, p1 & ph.M32, (p0 >> ph.S32) ^ c3 ^ k1, p0 & ph.M32
        k0, k1 = (k0 + ph.PHILOX_W0) & ph.M32, (k1 + ph.PHILOX_W1) & ph.M32
    return c0, c1, c2, c3


def uniform(w):
    """float32: u = (2 (w >> 9) + 1) * 2^-24, exact in fp32 and strictly inside (0, 1)."""
    m = (np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.int64)
    return (2 * m + 1).astype(np.float32) * np.float32(2.0 ** -24)


def gumbel32(w):
    """-log(-log(u)) with numpy's float32 log."""
    u = uniform(w)
    assert u.dtype == np.float32
    return -np.log(-np.log(u))


def gumbel64(w):
    u = uniform(w).astype(np.float64)
    return -np.log(-np.log(u))


def fma32(a, b, c):
    """The correctly rounded fp32 a * b + c of float32 arrays.  The product is exact in float64; the float64 sum is within half a
    float64 ulp of the exact value, and rounding it to fp32 differs from rounding the exact value only when it sits exactly on a
    fp32 midpoint that the exact value is not on -- the error term of the sum (TwoSum) says which side."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        finite = np.isfinite(s) & np.isfinite(err)
        tie = finite & (err != 0) & ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000))
        s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def keys(scores, inv_temperature, g):
    """float32 [B, N]: fmaf(score, inv_temperature, g)."""
    return fma32(scores, np.float32(inv_temperature), g)


def select(key, S, exclude=None):
    """ids int64 [B, S] and keys float32 [B, S]: per row the first min(S, #eligible) items by (key descending, id ascending; -0.0
    equals +0.0), eligible = not in exclude[b] and key not NaN; then id -1 / key -inf."""
    key = np.asarray(key, dtype=np.float32)
    B, N = key.shape
    ids = np.full((B, S), -1, dtype=np.int64)
    out = np.full((B, S), -np.inf, dtype=np.float32)
    for b in range(B):
        ok = ~np.isnan(key[b])
        if exclude is not None:
            ex = np.asarray(exclude[b], dtype=np.int64)
            ok[ex[(ex >= 0) & (ex < N)]] = False
        n = np.flatnonzero(ok)
        k = key[b, n] + np.float32(0.0)                      # -0.0 -> +0.0
        order = np.lexsort((n, -k.astype(np.float64)))[:S]
        ids[b, :order.size] = n[order]
        out[b, :order.size] = k[order]
    return ids, out


def sample(scores, row_key, S, inv_temperature, seed, exclude=None, g=None):
    """The whole draw from a [B, N] score matrix (g: the perturbation to use instead of gumbel32 of the words)."""
    scores = np.asarray(scores, dtype=np.float32)
    if g is None:
        g = gumbel32(words(seed, row_key, scores.shape[1]))
    return select(keys(scores, inv_temperature, g), S, exclude)


# ---- the statistics case of the issue: 8 items, first picks against the softmax, ordered pairs against Plackett-Luce ----------------
STAT_SCORES = np.array([0, .5, 1, 1.5, 2, -1, 2, .25], dtype=np.float32)
STAT_ROWS = 65536
STAT_KEYS = (2 ** 33 + np.arange(STAT_ROWS)).astype(np.int64)
STAT_INV_T = (0.0, 1.0, 3.0)
STAT_MIN_EXPECTED = 50.0


def plackett_luce(scores, inv_temperature):
    """(p first [N], p ordered pair [N, N]) of a draw without replacement from softmax(scores * inv_temperature)."""
    z = np.asarray(scores, dtype=np.float64) * float(inv_temperature)
    p = np.exp(z - z.max())
    p /= p.sum()
    pair = p[:, None] * p[None, :] / (1.0 - p[:, None])
    np.fill_diagonal(pair, 0.0)
    return p, pair


def worst_deviation(ids, scores, inv_temperature):
    """The largest |count - expected| / sd over the first picks and over the ordered (first, second) pairs whose expected count
    is at least STAT_MIN_EXPECTED, for ids [T, >= 2] drawn from `scores`."""
    T, N = ids.shape[0], len(scores)
    p, pair = plackett_luce(scores, inv_temperature)
    first = np.bincount(ids[:, 0], minlength=N)
    both = np.bincount(ids[:, 0] * N + ids[:, 1], minlength=N * N).reshape(N, N)
    assert first.sum() == T and both.sum() == T and (np.diag(both) == 0).all()
    dev = np.abs(first - T * p) / np.sqrt(T * p * (1 - p))
    judged = T * pair >= STAT_MIN_EXPECTED
    dev2 = np.abs(both - T * pair)[judged] / np.sqrt(T * pair * (1 - pair))[judged]
    return float(max(dev.max(), dev2.max())), int(judged.sum())
