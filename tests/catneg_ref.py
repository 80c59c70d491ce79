"""Restatement of nrms_catalogue_negative_sample (include/nrms_hip.h, "Click log") on top of tests/philox_ref.py, independent of the
library.  ``sample_row`` is the contract read aloud for ONE row in Python integers; ``catalogue_negative_sample`` draws all attempts
of all rows at once in numpy (the 128-bit product in 32-bit limbs) and resolves the slots row by row;
tests/test_catneg_host.py holds the two against each other."""
import bisect

import numpy as np

from tests.philox_ref import MASK64, philox4x32_7

SITE = 7                                         # PHILOX_SITE_CATALOGUE_NEG (csrc/common.h)
ATTEMPTS = 8
EPOCH_SEED_STEP = 0x9E3779B97F4A7C15
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def epoch_seed(seed, epoch):
    """data_handler.ClickFeed.epoch_seed (= ImpressionFeed's)."""
    return (int(seed) + int(epoch) * EPOCH_SEED_STEP) & MASK64


def cum_of(weights):
    """int64 [n_news + 1]: the exclusive running sum of the weights per news id (weights[0] must be 0)."""
    w = np.asarray(weights, dtype=np.int64)
    assert w[0] == 0 and (w >= 0).all()
    return np.concatenate([[0], np.cumsum(w)]).astype(np.int64)


def draw_int(seed, key, s, a, cum):
    """n(s, a) of the row with key `key`, in Python integers."""
    group = ((((int(key) * 64 + s) << 2) | (a >> 1))) & MASK64
    r4 = [int(w) for w in philox4x32_7(seed, np.uint64(group), SITE)]
    u = (r4[2 * (a & 1)] << 32) | r4[2 * (a & 1) + 1]
    x = (u * int(cum[-1])) >> 64
    return bisect.bisect_right([int(c) for c in cum], x) - 1


def sample_row(key, user_set, pos, cum, S, seed):
    """One good row -> ([pos, negatives ...], slots left without a value)."""
    own, row, short = set(int(v) for v in user_set), [int(pos)], 0
    for s in range(S):
        for a in range(ATTEMPTS):
            n = draw_int(seed, key, s, a, cum)
            if n != 0 and n not in own and n not in row[1:]:
                row.append(n)
                break
        else:
            short += 1
    return row, short


def mulhi64(u, W):
    """(u * W) >> 64 for a uint64 array u and an integer 0 <= W < 2^64, exact, in 32-bit limbs."""
    u = np.asarray(u, dtype=np.uint64)
    wl, wh = np.uint64(int(W) & 0xFFFFFFFF), np.uint64(int(W) >> 32)
    ul, uh = u & M32, u >> S32
    ll, lh, hl, hh = ul * wl, ul * wh, uh * wl, uh * wh
    mid = (ll >> S32) + (lh & M32) + (hl & M32)
    return hh + (lh >> S32) + (hl >> S32) + (mid >> S32)


def draws(seed, row_key, S, cum):
    """int64 [n_rows, S, 8]: n(s, a) of every row."""
    key = np.asarray(row_key, dtype=np.int64).astype(np.uint64)
    s, h = np.arange(S, dtype=np.uint64), np.arange(ATTEMPTS // 2, dtype=np.uint64)
    group = ((key[:, None, None] * np.uint64(64) + s[None, :, None]) << np.uint64(2)) | h[None, None, :]
    r = philox4x32_7(seed, group, SITE)                                                   # four [n, S, 4]
    u = np.stack([(r[0] << S32) | r[1], (r[2] << S32) | r[3]], axis=3).reshape(len(key), S, ATTEMPTS)
    x = mulhi64(u, int(cum[-1]))
    return np.searchsorted(np.asarray(cum, dtype=np.int64).astype(np.uint64), x, side="right").astype(np.int64) - 1


def catalogue_negative_sample(row_key, row_user, row_pos, set_ptr, set_news, cum, S, seed):
    """-> (cand [n_rows, S + 1] int64, clen [n_rows] int64, n_short, n_bad)."""
    row_user, row_pos = np.asarray(row_user, dtype=np.int64), np.asarray(row_pos, dtype=np.int64)
    set_ptr, set_news, cum = np.asarray(set_ptr, dtype=np.int64), np.asarray(set_news, dtype=np.int64), np.asarray(cum, dtype=np.int64)
    n_rows, n_users, n_news = len(row_user), len(set_ptr) - 1, len(cum) - 1
    cand, clen = np.zeros((n_rows, S + 1), dtype=np.int64), np.ones(n_rows, dtype=np.int64)
    if n_rows == 0:
        return cand, clen, 0, 0
    good = (row_user >= 0) & (row_user < n_users) & (row_pos > 0) & (row_pos < n_news)
    n = draws(seed, row_key, S, cum)
    # membership of every attempt at once: the sets as one sorted list of user * n_news + news
    edges = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(set_ptr)) * n_news + set_news
    probe = np.where(good, row_user, 0)[:, None, None] * n_news + n
    at = np.searchsorted(edges, probe)
    own = (at < len(edges)) & (edges[np.minimum(at, max(len(edges) - 1, 0))] == probe) if len(edges) else np.zeros(n.shape, dtype=bool)
    usable = (n != 0) & ~own
    n_short = 0
    for r in np.flatnonzero(good):
        row = [int(row_pos[r])]
        for s in range(S):
            for a in np.flatnonzero(usable[r, s]):
                v = int(n[r, s, a])
                if v not in row[1:]:
                    row.append(v)
                    break
            else:
                n_short += 1
        cand[r, :len(row)] = row
        clen[r] = len(row)
    return cand, clen, n_short, int((~good).sum())


def small_world(rng, n_news=120, n_users=25, zero_runs=True):
    """Zipf weights with zero-weight runs at the front, in the middle and at the end; users with sets of 0 .. 30 news."""
    w = np.floor(65536.0 / np.arange(1, n_news + 1) ** 0.9).astype(np.int64)
    w = w[rng.permutation(n_news)]
    w[0] = 0
    if zero_runs:
        w[1:4] = 0
        w[50:57] = 0
        w[-5:] = 0
    sets = [np.sort(rng.choice(np.arange(1, n_news), size=int(k), replace=False)) for k in rng.integers(0, 31, size=n_users)]
    sets[0] = np.zeros(0, dtype=np.int64)
    set_ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return w, cum_of(w), set_ptr, np.concatenate(sets).astype(np.int32)
