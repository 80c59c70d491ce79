"""The contract of nrms_topk_dot_windowed / nrms_rank_dot_windowed (include/nrms_hip.h) restated in numpy, from the plain score BITS.

Input: scores [B, N] float32, the bits of s(b, n) (nrms_topk_dot's chain; for integer lattice data the float64 product, which is
exact); bias [N] float32 or None; item_time [N] int32; window [B, 2] int32; exclude [B, n] ids or None (ids outside [0, N) are
ignored); k, or targets [B, T].
    s'(b, n) = np.float32(s) + np.float32(bias[n])      one fp32 addition (no bias: s' = s)
    eligible: window[b, 0] <= item_time[n] < window[b, 1] (signed, half-open), n not excluded, s' not NaN.  lo >= hi is the empty
              window; a time of INT32_MAX is below no hi, so it is never eligible.
    order:    s' descending (+inf first, -inf last), equal s' by the SMALLER n, -0.0 equals +0.0 and is returned as +0.0
    padding:  id -1 / score -inf past the eligible items; rank 0 / score -inf for a target that is out of range or not eligible.
Ranks are counted, not read off a sorted list, so `ranks` and `topk` are two statements that the host test holds against each other
and against a brute force."""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
FULL = (I32_MIN, I32_MAX)


def scores_of(scores, bias):
    """s' [B, N] float32 (None: the scores as they are), -0.0 returned as +0.0."""
    s = np.asarray(scores, dtype=np.float32)
    if bias is not None:
        b = np.asarray(bias, dtype=np.float32)
        assert b.shape == (s.shape[1],), (b.shape, s.shape)
        with np.errstate(invalid="ignore", over="ignore"):
            s = s + b[None, :]
        assert s.dtype == np.float32
    s = s.copy()
    s[s == 0.0] = 0.0
    return s


def eligible(sp, item_time, window, exclude):
    """bool [B, N]."""
    B, N = sp.shape
    t = np.asarray(item_time, dtype=np.int64).reshape(N)
    w = np.asarray(window, dtype=np.int64).reshape(B, 2)
    assert t.size == 0 or (t.min() >= I32_MIN and t.max() <= I32_MAX)
    assert w.min() >= I32_MIN and w.max() <= I32_MAX
    ok = (t[None, :] >= w[:, :1]) & (t[None, :] < w[:, 1:]) & ~np.isnan(sp)
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64)
        for b in range(B):
            ok[b, ex[b][(ex[b] >= 0) & (ex[b] < N)]] = False
    return ok


def topk(scores, bias, item_time, window, exclude, k):
    """-> (ids [B, k] int64, scores [B, k] float32), padded with -1 / -inf."""
    sp = scores_of(scores, bias)
    ok = eligible(sp, item_time, window, exclude)
    B = sp.shape[0]
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        n = np.nonzero(ok[b])[0]
        o = n[np.lexsort((n, -sp[b, n].astype(np.float64)))][:k]          # last key first; the float64 negation is exact
        ids[b, :len(o)] = o
        out[b, :len(o)] = sp[b, o]
    return ids, out


def ranks(scores, bias, item_time, window, exclude, targets):
    """-> (ranks [B, T] int32, scores [B, T] float32): 1 + the number of eligible items that precede the target, 0 / -inf for a
    target that is out of range or not eligible itself."""
    sp = scores_of(scores, bias)
    ok = eligible(sp, item_time, window, exclude)
    B, N = sp.shape
    tg = np.asarray(targets, dtype=np.int64)
    rk = np.zeros(tg.shape, dtype=np.int32)
    out = np.full(tg.shape, -np.inf, dtype=np.float32)
    for b in range(B):
        n = np.nonzero(ok[b])[0]
        sn = sp[b, n]
        for j, t in enumerate(tg[b]):
            if 0 <= t < N and ok[b, t]:
                st = sp[b, t]
                rk[b, j] = 1 + int(((sn > st) | ((sn == st) & (n < t))).sum())
                out[b, j] = st
    return rk, out


def window_as_bias(bias, item_time, window_row, N):
    """Consequence (b): the bias' [N] float32 that makes nrms_topk_dot_biased at B = 1 equal row b of the windowed call."""
    t = np.asarray(item_time, dtype=np.int64)
    lo, hi = int(window_row[0]), int(window_row[1])
    out = np.zeros(N, dtype=np.float32) if bias is None else np.array(bias, dtype=np.float32)
    out[~((t >= lo) & (t < hi))] = np.nan
    return out
