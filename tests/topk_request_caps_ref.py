"""The contract of nrms_topk_dot_request_capped (include/nrms_hip.h) restated in numpy, from the plain score BITS: the eligible set
and the adjusted score s'' of tests/topk_request_ref.py, walked greedily as tests/topk_caps_ref.py walks the biased ranking.

Input: scores [B, N] float32, the bits of s(b, n); bias [N] float32 or None; item_tag [N] int, n_tags and cap int [B, n_tags]
(required); a Parts of the optional pairs (topk_request_ref.Parts; its item_tag / n_tags are read only with parts.allow and must
then be the caps' own); exclude [B, n] ids or None; k; after = (after_scores [B], after_ids [B]) or None.
    eligible:  topk_request_ref's, word for word: s'' = (s + bias[n]) + delta, not excluded, not NaN, the window open, the tag
               allowed (if allow is given), strictly after the cursor (if one is given)
    walk:      that set in s'' descending, then the smaller n; item n with tag t is TAKEN iff 0 <= t < n_tags and fewer than
               cap[b, t] items of tag t were taken before it in this call; the first k taken are the row, then id -1 / score -inf."""
import numpy as np

from tests import topk_caps_ref, topk_request_ref

F = np.float32
Parts = topk_request_ref.Parts
PAGE_BEGIN = topk_request_ref.PAGE_BEGIN


def with_allow(parts, item_tag, n_tags, allow):
    """The parts with the tag set `allow` (bool [B, n_tags] or None) over the caps' own item_tag and n_tags."""
    if allow is None:
        return parts._replace(item_tag=None, n_tags=0, allow=None)
    return parts._replace(item_tag=item_tag, n_tags=n_tags, allow=allow)


def eligible_entries(scores, bias, parts, exclude, after):
    """Per user the eligible items as entries (topk_caps_ref.entries_of: Python ints, a larger entry comes first), unordered:
    topk_request_ref's s'' and eligibility, the cursor included."""
    sp = topk_request_ref.scores_of(np.asarray(scores, dtype=F), bias, parts)
    ok = topk_request_ref.eligible(sp, parts, exclude)
    out = []
    for b in range(sp.shape[0]):
        open_ = ok[b] & topk_request_ref._after_mask(sp[b], after, b)
        out.append(topk_caps_ref.entries_of(np.where(open_, sp[b], F(np.nan))))
    return out


def topk(scores, bias, item_tag, n_tags, cap, parts, exclude, k, after=None):
    """-> (ids [B, k] int64, scores [B, k] float32), padded with -1 / -inf."""
    B = np.asarray(scores).shape[0]
    cap = np.broadcast_to(np.asarray(cap, dtype=np.int64), (B, n_tags))
    if parts.allow is not None:
        assert parts.n_tags == n_tags and np.array_equal(np.asarray(parts.item_tag), np.asarray(item_tag)), "one item_tag, one n_tags"
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=F)
    for b, entries in enumerate(eligible_entries(scores, bias, parts, exclude, after)):
        ids[b], out[b] = topk_caps_ref.pad(topk_caps_ref.greedy(entries, item_tag, n_tags, cap[b], k), k)
    return ids, out


def remaining_caps(cap, served_ids, item_tag, n_tags):
    """Consequence 5's helper: cap minus the per-tag counts of served_ids [B, K] (-1: padding) -> int64 [B, n_tags]."""
    served = np.asarray(served_ids, dtype=np.int64)
    B = served.shape[0]
    out = np.broadcast_to(np.asarray(cap, dtype=np.int64), (B, n_tags)).copy()
    for b in range(B):
        for n in served[b]:
            if n >= 0 and 0 <= int(item_tag[n]) < n_tags:
                out[b, int(item_tag[n])] -= 1
    return out


def pages(scores, bias, item_tag, n_tags, cap, parts, exclude, lengths, after=None):
    """Consequence 5: pages of the given lengths chained through the cursor and remaining_caps -> (ids, scores) laid end to end."""
    B = np.asarray(scores).shape[0]
    got_i, got_s = [], []
    cur, left = after, np.broadcast_to(np.asarray(cap, dtype=np.int64), (B, n_tags)).copy()
    for L in lengths:
        i_, s_ = topk(scores, bias, item_tag, n_tags, left, parts, exclude, L, cur)
        got_i.append(i_)
        got_s.append(s_)
        cur = (s_[:, -1].copy(), i_[:, -1].copy())
        left = remaining_caps(left, i_, item_tag, n_tags)
    return np.concatenate(got_i, axis=1), np.concatenate(got_s, axis=1)


def as_bias(parts, b, N):
    """Consequence 4: the bias [N] that makes nrms_topk_dot_capped at B = 1 equal row b of a capped request without a prior and
    without a cursor (topk_request_ref.request_as_bias: deltas scattered, +0.0 elsewhere, NaN where the window or allow closes)."""
    return topk_request_ref.request_as_bias(parts, b, N)

