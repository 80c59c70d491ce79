"""The contract of nrms_topk_dot_capped (include/nrms_hip.h) restated in numpy, from the plain score BITS, and a pure-Python model of
the one-scan filter that computes it (csrc/topk_kernels.h: tk_select_capped, the CAPS slice kernels, topk_merge_capped_kernel).

Input: scores [B, N] float32, the bits of s(b, n) (nrms_topk_dot's chain; for integer lattice data the float64 product, which is
exact); bias [N] float32 or None; item_tag [N] int; n_tags; cap int [B, n_tags]; exclude [B, n] ids or None (ids outside [0, N)
are ignored); k.
    s'(b, n) = np.float32(s) + np.float32(bias[n])      one fp32 addition (no bias: s' = s)
    ranking:  the items with s' not NaN that are not excluded, s' descending (+inf first, -inf last), equal s' by the SMALLER n,
              -0.0 equals +0.0 and is returned as +0.0
    greedy:   walk the ranking; item n with tag t = item_tag[n] is TAKEN iff 0 <= t < n_tags and fewer than cap[b, t] items of tag
              t were taken before it.  The first k taken items are the row, then id -1 / score -inf.
An entry is the kernels' 64-bit key as a Python int: the score as an order-preserving 32-bit key above the complement of the id,
so a larger entry comes first; entry 0 is padding."""
import numpy as np

F = np.float32


def scores_of(scores, bias):
    """s' [B, N] float32 (None: the scores as they are), -0.0 returned as +0.0."""
    s = np.asarray(scores, dtype=F)
    if bias is not None:
        b = np.asarray(bias, dtype=F)
        assert b.shape == (s.shape[1],), (b.shape, s.shape)
        with np.errstate(invalid="ignore", over="ignore"):
            s = s + b[None, :]
        assert s.dtype == F
    s = s.copy()
    s[s == 0.0] = 0.0
    return s


def entries_of(sp_row, exclude_row=None):
    """The entries of one user's ranking, unordered: [(entry, id)] as Python ints for every item with a non-NaN s' that is not
    excluded.  sp_row: s' [N] float32 with -0.0 already +0.0 (scores_of)."""
    s = np.ascontiguousarray(sp_row, dtype=F)
    u = s.view(np.uint32).astype(np.uint64)
    key = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    n = np.arange(len(s), dtype=np.uint64)
    e = (key << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - n)
    ok = ~np.isnan(s)
    if exclude_row is not None:
        ex = np.asarray(exclude_row, dtype=np.int64)
        ok[ex[(ex >= 0) & (ex < len(s))]] = False
    return [int(x) for x in e[ok]]


def entry_id(e):
    return 0xFFFFFFFF - (e & 0xFFFFFFFF)


def entry_score(e):
    u = e >> 32
    u = (u & 0x7FFFFFFF) if (u & 0x80000000) else (~u & 0xFFFFFFFF)
    return np.array([u], dtype=np.uint32).view(F)[0]


def greedy(entries, item_tag, n_tags, cap_row, k):
    """The greedy walk over entries (any order; distinct): the first k taken entries, best first.  This is C(S) of the issue."""
    taken, used = [], {}
    for e in sorted(entries, reverse=True):
        if len(taken) == k:
            break
        t = int(item_tag[entry_id(e)])
        if 0 <= t < n_tags and used.get(t, 0) < int(cap_row[t]):
            used[t] = used.get(t, 0) + 1
            taken.append(e)
    return taken


def pad(taken, k):
    """-> (ids [k] int64, scores [k] float32) of a list of entries, padded with -1 / -inf."""
    ids = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, -np.inf, dtype=F)
    for j, e in enumerate(taken):
        ids[j], sc[j] = entry_id(e), entry_score(e)
    return ids, sc


def topk(scores, bias, item_tag, n_tags, cap, exclude, k):
    """-> (ids [B, k] int64, scores [B, k] float32), padded with -1 / -inf."""
    sp = scores_of(scores, bias)
    B = sp.shape[0]
    cap = np.asarray(cap, dtype=np.int64).reshape(B, n_tags)
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=F)
    for b in range(B):
        ids[b], out[b] = pad(greedy(entries_of(sp[b], None if exclude is None else exclude[b]), item_tag, n_tags, cap[b], k), k)
    return ids, out


def greedy_over_list(ids_row, scores_row, item_tag, n_tags, cap_row, k):
    """Consequence 6: the greedy walk over one row of an already ranked list (nrms_topk_dot_deep: ids -1 are padding) ->
    (ids [k], scores [k])."""
    ids = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, -np.inf, dtype=F)
    used, j = {}, 0
    for n, s in zip(ids_row, scores_row):
        if j == k:
            break
        if n < 0:
            continue
        t = int(item_tag[n])
        if 0 <= t < n_tags and used.get(t, 0) < int(cap_row[t]):
            used[t] = used.get(t, 0) + 1
            ids[j], sc[j] = n, s
            j += 1
    return ids, sc


def reach(cap_row, k):
    """k_b = min(k, sum_t min(max(cap, 0), k)): the length a capped list can reach."""
    return min(k, sum(min(max(int(c), 0), k) for c in cap_row))


# ---- the filter model ----------------------------------------------------------------------------------------------------------
def select_capped(buf, item_tag, n_tags, cap_row, k, tag_thr=None):
    """The flush: buf -> (C(buf), threshold).  The threshold is the smallest kept entry once k_b entries are kept, else 0.  tag_thr
    (a dict, updated in place): per tag the upper 16 bits of the largest cap-th tag-eligible entry any flush has met."""
    kept = greedy(buf, item_tag, n_tags, cap_row, k)
    kb = reach(cap_row, k)
    if tag_thr is not None:
        used = {}
        for e in greedy(buf, item_tag, n_tags, cap_row, len(buf)):           # every tag-eligible entry, before the cut at k
            t = int(item_tag[entry_id(e)])
            used[t] = used.get(t, 0) + 1
            if used[t] == int(cap_row[t]):
                tag_thr[t] = max(tag_thr.get(t, 0), e >> 48)
    return kept, (kept[-1] if kb > 0 and len(kept) == kb else 0)


def filter_slice(entries, item_tag, n_tags, cap_row, k, P, stats=None):
    """One slice kernel's filter for one user: the entries arrive in the given order; one above the user's threshold whose upper
    16 bits are not below its tag's threshold is appended to a buffer of P; a full buffer is flushed (capped selection, new
    thresholds) and the candidate offered again.  At the end the buffer is flushed once more: the slice's list, at most k entries."""
    buf, thr, tag_thr = [], 0, {}
    for e in entries:
        t = int(item_tag[entry_id(e)])
        if not (0 <= t < n_tags and int(cap_row[t]) > 0) or (e >> 48) < tag_thr.get(t, 0):
            if stats is not None and 0 <= t < n_tags and int(cap_row[t]) > 0:
                stats["refused_by_tag"] = stats.get("refused_by_tag", 0) + 1
            continue                                                         # the bitmap; the tag threshold
        while e > thr:
            if len(buf) < P:
                buf.append(e)
                break
            buf, thr = select_capped(buf, item_tag, n_tags, cap_row, k, tag_thr)
            if stats is not None:
                stats["flushes"] = stats.get("flushes", 0) + 1
    return select_capped(buf, item_tag, n_tags, cap_row, k)[0]


def filter_topk(entries, item_tag, n_tags, cap_row, k, P, n_slices, stats=None):
    """The whole call for one user: the entries (in catalogue order) cut into n_slices contiguous slices, each through
    filter_slice, then the merge: the slice lists streamed 64 at a time through one more buffer of P >= k + 64 with the same flush,
    and a last flush.  -> the list, best first."""
    assert P >= k + 64
    n = len(entries)
    step = -(-n // n_slices) if n else 0
    lists = []
    for s in range(n_slices):
        lists += filter_slice(entries[s * step:(s + 1) * step], item_tag, n_tags, cap_row, k, P, stats)
    buf, thr = [], 0
    for c0 in range(0, len(lists), 64):
        buf += [e for e in lists[c0:c0 + 64] if e > thr]
        if len(buf) + 64 > P:
            buf, thr = select_capped(buf, item_tag, n_tags, cap_row, k)
    return select_capped(buf, item_tag, n_tags, cap_row, k)[0]
