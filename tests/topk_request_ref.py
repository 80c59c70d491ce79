"""The contract of nrms_topk_dot_request / nrms_rank_dot_request (include/nrms_hip.h) restated in numpy, from the plain score BITS.

Input: scores [B, N] float32, the bits of s(b, n) (nrms_topk_dot's chain; for lattice data the float64 product, which is exact);
bias [N] float32 or None; a Parts of optional pairs (None = the part is absent): item_time [N] / window [B, 2] int32, item_tag [N]
/ allow bool [B, n_tags], adj_ids [B, E] int64 / adj_delta [B, E] float32; exclude [B, n] ids or None; k, or targets [B, T];
after = (after_scores [B] float32, after_ids [B] int64) or None.
    s'(b, n)  = np.float32(s) + np.float32(bias[n])     one fp32 addition (no bias: s' = s)
    s''(b, n) = s' + adj_delta[b, e]                    one more, only where (b, n) has a slot; e the LOWEST slot that names n
    eligible:   n not excluded, s'' not NaN, window[b, 0] <= item_time[n] < window[b, 1] (signed, half-open: a time of INT32_MAX is
                open to nobody), 0 <= item_tag[n] < n_tags and allow[b, item_tag[n]]
    order:      s'' descending (+inf first, -inf last), equal s'' by the SMALLER n, -0.0 equals +0.0 and is returned as +0.0
    cursor:     after_ids[b] == PAGE_BEGIN: none; any other negative id or a NaN after score: END, nothing follows; otherwise only
                the eligible items strictly after (after_scores[b], after_ids[b]) in that order (the position need not be an item)
    padding:    id -1 / score -inf past the eligible items; rank 0 / score -inf for a target that is out of range or not eligible.
Ranks are counted, not read off a sorted list, so `ranks` and `topk` are two statements that the host test holds against each other
and against a brute force."""
import collections

import numpy as np

from tests import topk_adjust_ref, topk_tags_ref, topk_window_ref

PAGE_BEGIN = -2
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

Parts = collections.namedtuple("Parts", "item_time window item_tag n_tags allow adj_ids adj_delta",
                               defaults=(None, None, None, 0, None, None, None))


def scores_of(scores, bias, parts):
    """s'' [B, N] float32, -0.0 returned as +0.0: the prior's add, then the delta's, as topk_adjust_ref forms them."""
    return topk_adjust_ref.scores_of(scores, bias, parts.adj_ids, parts.adj_delta)


def eligible(spp, parts, exclude):
    """bool [B, N]: the AND of the parts' own rules (topk_window_ref, topk_tags_ref) on s''."""
    ok = topk_adjust_ref.eligible(spp, exclude)
    if parts.window is not None:
        ok &= topk_window_ref.eligible(spp, parts.item_time, parts.window, None)
    if parts.allow is not None:
        ok &= topk_tags_ref.eligible(spp, parts.item_tag, parts.n_tags, parts.allow, None)
    return ok


def _after_mask(sp_row, after, b):
    """bool [N]: the items strictly after user b's cursor."""
    N = sp_row.shape[0]
    if after is None:
        return np.ones(N, dtype=bool)
    a_s, a_id = np.float32(np.asarray(after[0], dtype=np.float32)[b]), int(np.asarray(after[1], dtype=np.int64)[b])
    if a_id == PAGE_BEGIN:
        return np.ones(N, dtype=bool)
    if a_id < 0 or np.isnan(a_s):
        return np.zeros(N, dtype=bool)
    a_s = np.float32(0.0) if a_s == 0.0 else a_s
    n = np.arange(N)
    with np.errstate(invalid="ignore"):
        return (sp_row < a_s) | ((sp_row == a_s) & (n > a_id))


def topk(scores, bias, parts, exclude, k, after=None):
    """-> (ids [B, k] int64, scores [B, k] float32), padded with -1 / -inf."""
    sp = scores_of(scores, bias, parts)
    ok = eligible(sp, parts, exclude)
    B = sp.shape[0]
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        n = np.nonzero(ok[b] & _after_mask(sp[b], after, b))[0]
        o = n[np.lexsort((n, -sp[b, n].astype(np.float64)))][:k]          # last key first; the float64 negation is exact
        ids[b, :len(o)] = o
        out[b, :len(o)] = sp[b, o]
    return ids, out


def ranks(scores, bias, parts, exclude, targets):
    """-> (ranks [B, T] int32, scores [B, T] float32): 1 + the number of eligible items that precede the target, 0 / -inf for a
    target that is out of range or not eligible itself."""
    sp = scores_of(scores, bias, parts)
    ok = eligible(sp, parts, exclude)
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


def request_as_bias(parts, b, N):
    """Consequence 3: the bias [N] float32 that makes nrms_topk_dot_biased at B = 1 equal row b of a request without a prior: the
    row's deltas scattered by the lowest-slot rule, +0.0 elsewhere, NaN where the window or the tag set closes the news."""
    if parts.adj_ids is not None:
        out = topk_adjust_ref.adjust_as_bias(parts.adj_ids[b], parts.adj_delta[b], N)
    else:
        out = np.zeros(N, dtype=np.float32)
    if parts.window is not None:
        out = topk_window_ref.window_as_bias(out, parts.item_time, np.asarray(parts.window)[b], N)
    if parts.allow is not None:
        out = topk_tags_ref.tags_as_bias(out, parts.item_tag, parts.n_tags, np.asarray(parts.allow)[b], N)
    return out


def neutral(B, N, n_tags=3, E=2):
    """Every part given but neutral by value: the widest window over times of 0, every tag open, every slot -1."""
    return Parts(np.zeros(N, dtype=np.int32), np.tile(np.array([[I32_MIN, I32_MAX]], dtype=np.int32), (B, 1)),
                 np.zeros(N, dtype=np.int32), n_tags, np.ones((B, n_tags), dtype=bool),
                 np.full((B, E), -1, dtype=np.int64), np.full((B, E), 5.0, dtype=np.float32))
