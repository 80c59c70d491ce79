"""The contract of nrms_topk_dot_adjusted / nrms_rank_dot_adjusted (include/nrms_hip.h) restated in numpy, from the plain score BITS.

Input: scores [B, N] float32, the bits of s(b, n) (nrms_topk_dot's chain; for lattice data the float64 product, which is exact);
bias [N] float32 or None; adj_ids [B, E] int64 and adj_delta [B, E] float32 (or None: no adjustment); exclude [B, n] ids or None
(ids outside [0, N) are ignored); k, or targets [B, T].
    s'(b, n)  = np.float32(s) + np.float32(bias[n])     one fp32 addition (no bias: s' = s)
    slot:       the LOWEST e with adj_ids[b, e] == n; an id outside [0, N) is an empty slot
    s''(b, n) = s' + adj_delta[b, e]                    one more fp32 addition, only where (b, n) has a slot
    eligible:   n not excluded and s'' not NaN (a NaN delta closes n for b alone)
    order:      s'' descending (+inf first, -inf last), equal s'' by the SMALLER n, -0.0 equals +0.0 and is returned as +0.0
    padding:    id -1 / score -inf past the eligible items; rank 0 / score -inf for a target that is out of range or not eligible.
Ranks are counted, not read off a sorted list, so `ranks` and `topk` are two statements that the host test holds against each other
and against a brute force."""
import numpy as np


def slots_of(adj_ids, N):
    """int [B, N]: the slot of every pair, -1 where there is none (the lowest-slot rule)."""
    a = np.asarray(adj_ids, dtype=np.int64)
    B, E = a.shape
    slot = np.full((B, N), -1, dtype=np.int64)
    for b in range(B):
        for e in range(E - 1, -1, -1):          # descending, so the lowest e is written last
            n = int(a[b, e])
            if 0 <= n < N:
                slot[b, n] = e
    return slot


def scores_of(scores, bias, adj_ids=None, adj_delta=None):
    """s'' [B, N] float32, -0.0 returned as +0.0."""
    s = np.asarray(scores, dtype=np.float32)
    B, N = s.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if bias is not None:
            b = np.asarray(bias, dtype=np.float32)
            assert b.shape == (N,), (b.shape, s.shape)
            s = s + b[None, :]
        s = s.copy()
        if adj_ids is not None and np.asarray(adj_ids).shape[1] > 0:
            slot = slots_of(adj_ids, N)
            dl = np.asarray(adj_delta, dtype=np.float32)
            assert dl.shape == np.asarray(adj_ids).shape
            bb, nn = np.nonzero(slot >= 0)
            s[bb, nn] = s[bb, nn] + dl[bb, slot[bb, nn]]
    assert s.dtype == np.float32
    s[s == 0.0] = 0.0
    return s


def eligible(spp, exclude):
    """bool [B, N]."""
    B, N = spp.shape
    ok = ~np.isnan(spp)
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64)
        for b in range(B):
            ok[b, ex[b][(ex[b] >= 0) & (ex[b] < N)]] = False
    return ok


def topk(scores, bias, adj_ids, adj_delta, exclude, k):
    """-> (ids [B, k] int64, scores [B, k] float32), padded with -1 / -inf."""
    sp = scores_of(scores, bias, adj_ids, adj_delta)
    ok = eligible(sp, exclude)
    B = sp.shape[0]
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        n = np.nonzero(ok[b])[0]
        o = n[np.lexsort((n, -sp[b, n].astype(np.float64)))][:k]          # last key first; the float64 negation is exact
        ids[b, :len(o)] = o
        out[b, :len(o)] = sp[b, o]
    return ids, out


def ranks(scores, bias, adj_ids, adj_delta, exclude, targets):
    """-> (ranks [B, T] int32, scores [B, T] float32): 1 + the number of eligible items that precede the target, 0 / -inf for a
    target that is out of range or not eligible itself."""
    sp = scores_of(scores, bias, adj_ids, adj_delta)
    ok = eligible(sp, exclude)
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


def adjust_as_bias(adj_ids_row, adj_delta_row, N):
    """Consequence (b): the bias [N] float32 that makes nrms_topk_dot_biased at B = 1 equal row b of the adjusted call without a
    prior: the row's deltas scattered by the lowest-slot rule, +0.0 elsewhere."""
    out = np.zeros(N, dtype=np.float32)
    ids = np.asarray(adj_ids_row, dtype=np.int64)
    dl = np.asarray(adj_delta_row, dtype=np.float32)
    for e in range(len(ids) - 1, -1, -1):
        if 0 <= ids[e] < N:
            out[ids[e]] = dl[e]
    return out
