"""The contract of nrms_topk_dot_tagged / nrms_rank_dot_tagged (include/nrms_hip.h) restated in numpy, from the plain score BITS.

Input: scores [B, N] float32, the bits of s(b, n) (nrms_topk_dot's chain; for integer lattice data the float64 product, which is
exact); bias [N] float32 or None; item_tag [N] int32; n_tags; allow bool [B, n_tags]; exclude [B, n] ids or None (ids outside
[0, N) are ignored); k, or targets [B, T].
    s'(b, n) = np.float32(s) + np.float32(bias[n])      one fp32 addition (no bias: s' = s)
    eligible: 0 <= item_tag[n] < n_tags and allow[b, item_tag[n]], n not excluded, s' not NaN.  A tag outside [0, n_tags) is open
              to nobody; an all-False allow row is the empty set.
    order:    s' descending (+inf first, -inf last), equal s' by the SMALLER n, -0.0 equals +0.0 and is returned as +0.0
    padding:  id -1 / score -inf past the eligible items; rank 0 / score -inf for a target that is out of range or not eligible.
Ranks are counted, not read off a sorted list, so `ranks` and `topk` are two statements that the host test holds against each other
and against a brute force.  `pack` is the bit layout of the kernels' allow argument, written with Python integers."""
import numpy as np


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


def eligible(sp, item_tag, n_tags, allow, exclude):
    """bool [B, N]."""
    B, N = sp.shape
    t = np.asarray(item_tag, dtype=np.int64).reshape(N)
    a = np.asarray(allow, dtype=bool).reshape(B, n_tags)
    in_range = (t >= 0) & (t < n_tags)
    ok = np.zeros((B, N), dtype=bool)
    ok[:, in_range] = a[:, t[in_range]]
    ok &= ~np.isnan(sp)
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64)
        for b in range(B):
            ok[b, ex[b][(ex[b] >= 0) & (ex[b] < N)]] = False
    return ok


def topk(scores, bias, item_tag, n_tags, allow, exclude, k):
    """-> (ids [B, k] int64, scores [B, k] float32), padded with -1 / -inf."""
    sp = scores_of(scores, bias)
    ok = eligible(sp, item_tag, n_tags, allow, exclude)
    B = sp.shape[0]
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        n = np.nonzero(ok[b])[0]
        o = n[np.lexsort((n, -sp[b, n].astype(np.float64)))][:k]          # last key first; the float64 negation is exact
        ids[b, :len(o)] = o
        out[b, :len(o)] = sp[b, o]
    return ids, out


def ranks(scores, bias, item_tag, n_tags, allow, exclude, targets):
    """-> (ranks [B, T] int32, scores [B, T] float32): 1 + the number of eligible items that precede the target, 0 / -inf for a
    target that is out of range or not eligible itself."""
    sp = scores_of(scores, bias)
    ok = eligible(sp, item_tag, n_tags, allow, exclude)
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


def tags_as_bias(bias, item_tag, n_tags, allow_row, N):
    """Consequence (b): the bias' [N] float32 that makes nrms_topk_dot_biased at B = 1 equal row b of the tagged call."""
    t = np.asarray(item_tag, dtype=np.int64)
    a = np.asarray(allow_row, dtype=bool).reshape(n_tags)
    open_ = np.zeros(N, dtype=bool)
    in_range = (t >= 0) & (t < n_tags)
    open_[in_range] = a[t[in_range]]
    out = np.zeros(N, dtype=np.float32) if bias is None else np.array(bias, dtype=np.float32)
    out[~open_] = np.nan
    return out


def pack(allow, garbage=None):
    """allow bool [B, n_tags] -> uint32 [B, ceil(n_tags / 32)]: tag t of user b is bit t & 31 of word [b, t >> 5].  garbage: a
    uint32 whose bits fill the positions >= n_tags of the last word (the kernels ignore them); None leaves them zero."""
    a = np.asarray(allow, dtype=bool)
    B, n_tags = a.shape
    W = (n_tags + 31) // 32
    out = np.zeros((B, W), dtype=np.uint32)
    for b in range(B):
        for w in range(W):
            word = 0
            for j in range(32):
                t = 32 * w + j
                if t < n_tags:
                    word |= int(a[b, t]) << j
                elif garbage is not None:
                    word |= ((int(garbage) >> j) & 1) << j
            out[b, w] = word
    return out
