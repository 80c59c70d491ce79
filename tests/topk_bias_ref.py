"""The contract of nrms_topk_dot_biased / nrms_rank_dot_biased (include/nrms_hip.h) restated in numpy, from the plain score BITS.

Input: scores [B, N] float32, the bits of s(b, n) (nrms_topk_dot's chain; for integer lattice data the float64 product, which is
exact); bias [N] float32 or None; exclude [B, n] ids or None (ids outside [0, N) are ignored); k, or targets [B, T].
    s'(b, n) = np.float32(s) + np.float32(bias[n])      one fp32 addition, round to nearest
    eligible: n not excluded and s' not NaN               (a NaN bias removes n for everybody; +inf + -inf is NaN)
    order:    s' descending (+inf first, -inf last), equal s' by the SMALLER n, -0.0 equals +0.0 and is returned as +0.0
    padding:  id -1 / score -inf past the eligible items; rank 0 / score -inf for a target that is out of range, excluded or
              not eligible."""
import numpy as np


def biased(scores, bias):
    """s' [B, N] float32: one fp32 add per element (None: the scores as they are), -0.0 returned as +0.0."""
    s = np.asarray(scores, dtype=np.float32)
    if bias is not None:
        b = np.asarray(bias, dtype=np.float32)
        assert b.shape == (s.shape[1],), (b.shape, s.shape)
        with np.errstate(invalid="ignore", over="ignore"):
            s = s + b[None, :]                      # float32 + float32 -> float32
        assert s.dtype == np.float32
    s = s.copy()
    s[s == 0.0] = 0.0                               # -0.0 -> +0.0, as the entry canonicalises it
    return s


def order(sb, exclude_row=None):
    """The eligible ids of one row of s', best first."""
    N = sb.shape[0]
    ok = ~np.isnan(sb)
    if exclude_row is not None:
        ex = np.asarray(exclude_row, dtype=np.int64)
        ok[ex[(ex >= 0) & (ex < N)]] = False
    ids = np.nonzero(ok)[0]
    # lexsort: last key first; the float64 negation is exact and keeps +-inf in their places
    return ids[np.lexsort((ids, -sb[ids].astype(np.float64)))]


def topk(scores, bias, exclude, k):
    """-> (ids [B, k] int64, scores [B, k] float32), padded with -1 / -inf."""
    s = biased(scores, bias)
    B = s.shape[0]
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        o = order(s[b], None if exclude is None else exclude[b])[:k]
        ids[b, :len(o)] = o
        out[b, :len(o)] = s[b, o]
    return ids, out


def ranks(scores, bias, exclude, targets):
    """-> (ranks [B, T] int32, scores [B, T] float32): the 1-based place of every target in `order`, 0 / -inf if it has none."""
    s = biased(scores, bias)
    B, N = s.shape
    tg = np.asarray(targets, dtype=np.int64)
    rk = np.zeros(tg.shape, dtype=np.int32)
    out = np.full(tg.shape, -np.inf, dtype=np.float32)
    for b in range(B):
        pos = np.zeros(N, dtype=np.int32)
        o = order(s[b], None if exclude is None else exclude[b])
        pos[o] = np.arange(1, len(o) + 1)
        for j, t in enumerate(tg[b]):
            if 0 <= t < N and pos[t] > 0:
                rk[b, j] = pos[t]
                out[b, j] = s[b, t]
    return rk, out
