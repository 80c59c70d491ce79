"""The contract of nrms_topk_dot_after / nrms_topk_dot_deep (include/nrms_hip.h) restated in numpy, from the score BITS.

Input: sp [B, N] float32, the bits of s'(b, n) (the biased score where there is a prior; tests/topk_window_ref.scores_of forms it
with one fp32 addition); ok [B, N] bool, the eligibility of the uncursored call (window, exclude list, NaN rule:
tests/topk_window_ref.eligible); the cursor (after_scores [B] float32, after_ids [B] int64).
    order:   s' descending (+inf first, -inf last), equal s' by the SMALLER n, -0.0 equals +0.0 and is returned as +0.0
    cursor:  id -2 (BEGIN): none.  Any other negative id, or a NaN score: END, the row is all padding.  id >= 0: a position (s, n)
             of the order, whatever item n is (ids above MAX_ID are read as MAX_ID); row b gets the eligible items strictly after it:
             s' < s, or s' == s and n > id.
    padding: id -1 / score -inf past the items there are.
`after` filters and sorts; `after_by_position` finds the same page by walking the fully sorted list.  The host test holds the two
against each other."""
import numpy as np

BEGIN = -2
MAX_ID = 0x7FFF0000
PAGE = 256
DEEP_MAX = 4096


def _canon(x):
    x = np.array(x, dtype=np.float32)
    x[x == 0.0] = 0.0
    return x


def full_order(sp_row, ok_row):
    """The eligible ids of one row in the total order."""
    n = np.nonzero(ok_row & ~np.isnan(sp_row))[0]
    s = _canon(sp_row[n]).astype(np.float64)          # the float64 negation is exact
    return n[np.lexsort((n, -s))]


def _pad(rows, sp, k):
    B = len(rows)
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=np.float32)
    for b, o in enumerate(rows):
        o = o[:k]
        ids[b, :len(o)] = o
        out[b, :len(o)] = _canon(sp[b, o])
    return ids, out


def after(sp, ok, after_scores, after_ids, k):
    """-> (ids [B, k] int64, scores [B, k] float32): the k after the cursor."""
    sp = np.asarray(sp, dtype=np.float32)
    a_s = _canon(after_scores)
    a_i = np.asarray(after_ids, dtype=np.int64)
    B, N = sp.shape
    rows = []
    n = np.arange(N, dtype=np.int64)
    for b in range(B):
        if a_i[b] == BEGIN:
            keep = np.ones(N, dtype=bool)
        elif a_i[b] < 0 or np.isnan(a_s[b]):
            keep = np.zeros(N, dtype=bool)
        else:
            s = _canon(sp[b])
            with np.errstate(invalid="ignore"):
                keep = (s < a_s[b]) | ((s == a_s[b]) & (n > min(int(a_i[b]), MAX_ID)))
        rows.append(full_order(sp[b], np.asarray(ok[b]) & keep))
    return _pad(rows, sp, k)


def after_by_position(sp, ok, after_scores, after_ids, k):
    """The same page, found by walking the full list: skip every listed item that does not come strictly after the cursor."""
    sp = np.asarray(sp, dtype=np.float32)
    a_s = _canon(after_scores)
    a_i = np.asarray(after_ids, dtype=np.int64)
    rows = []
    for b in range(sp.shape[0]):
        o = full_order(sp[b], np.asarray(ok[b]))
        if a_i[b] == BEGIN:
            rows.append(o)
            continue
        if a_i[b] < 0 or np.isnan(a_s[b]):
            rows.append(o[:0])
            continue
        cid = min(int(a_i[b]), MAX_ID)
        start = len(o)
        for j, t in enumerate(o):
            st = _canon(sp[b, t:t + 1])[0]
            if st < a_s[b] or (st == a_s[b] and t > cid):
                start = j
                break
        rows.append(o[start:])
    return _pad(rows, sp, k)


def deep(sp, ok, K):
    """-> (ids [B, K], scores [B, K]): the first min(K, #eligible) items of every row in order, then -1 / -inf."""
    sp = np.asarray(sp, dtype=np.float32)
    assert 1 <= K <= DEEP_MAX
    return _pad([full_order(sp[b], np.asarray(ok[b])) for b in range(sp.shape[0])], sp, K)


def chain(sp, ok, lengths):
    """Pages of the given lengths chained from BEGIN, each cursor the last column of the page before -> (ids, scores) side by side."""
    B = sp.shape[0]
    a_s = np.zeros(B, dtype=np.float32)
    a_i = np.full(B, BEGIN, dtype=np.int64)
    ids, out = [], []
    for k in lengths:
        i, s = after(sp, ok, a_s, a_i, k)
        ids.append(i)
        out.append(s)
        a_i, a_s = i[:, -1].copy(), s[:, -1].copy()
    return np.concatenate(ids, axis=1), np.concatenate(out, axis=1)
