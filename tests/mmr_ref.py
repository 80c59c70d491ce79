"""The contract of nrms_mmr_rerank (include/nrms_hip.h) restated in numpy, one row at a time.

mmr_row(items, ids, scores, lam, k) is the yardstick: the cosine and the value v are formed in float64 from the fp32 inputs
(the relevance from the fp32 scores), the greedy choice uses the contract's order (v descending, -0.0 equal to +0.0, then the
smaller position, NaN after every number), the ILD is 1 - the mean cosine over the unordered pairs of picks.  With dtype =
np.float32 the same code follows the contract's fp32 operation sequence except for the dot products, which stay float64 and are
rounded once: on data whose dot products are exact in fp32 both evaluations are the kernel's, bit for bit.

greedy_gap(...) judges a pick sequence someone else made: at every step, how much better (in float64) the best remaining entry
would have been than the entry that was picked, on that sequence's own prefix."""
import numpy as np


def valid_mask(ids, scores, n_items):
    ids = np.asarray(ids, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    return (ids >= 0) & (ids < n_items) & np.isfinite(scores)


def relevance(scores, valid, dtype=np.float64):
    """(s - s_min) / (s_max - s_min) over the valid entries, 0 everywhere when s_max == s_min (or nothing is valid)."""
    s = np.asarray(scores, dtype=np.float32).astype(dtype)
    rel = np.zeros(len(s), dtype=dtype)
    if valid.any():
        lo, hi = s[valid].min(), s[valid].max()
        if hi != lo:
            with np.errstate(over="ignore", invalid="ignore"):
                rel[valid] = ((s[valid] - lo) / dtype(hi - lo)).astype(dtype)
    return rel


def cosine_matrix(items, ids, valid, dtype=np.float64):
    """cos(i, j) = dot(x_i, x_j) * (r_i * r_j), r_i = 1 / sqrt(dot(x_i, x_i)) or 0 for a zero (or non-finite) norm; rows of
    entries that are not valid are zeros.  No id outside the catalogue is read."""
    M = len(ids)
    x = np.zeros((M, items.shape[1]), dtype=np.float64)
    x[valid] = np.asarray(items, dtype=np.float32)[np.asarray(ids, dtype=np.int64)[valid]].astype(np.float64)
    with np.errstate(all="ignore"):
        dot = (x @ x.T).astype(dtype)
        dd = np.diagonal(dot).copy()
        ok = (dd > 0) & np.isfinite(dd)
        r = np.zeros(M, dtype=dtype)
        r[ok] = (dtype(1) / np.sqrt(dd[ok])).astype(dtype)
        return (dot * np.outer(r, r).astype(dtype)).astype(dtype)


def _value(lam, rel, maxsim, dtype):
    """v = (lam * rel) - ((1 - lam) * maxsim), every operation rounded to dtype."""
    lam = dtype(np.float32(lam))
    c = dtype(dtype(1) - lam)
    with np.errstate(all="ignore"):
        return (lam * rel).astype(dtype) - (c * maxsim).astype(dtype)


def _best(v, live):
    """Position of the largest v among live entries (one is live): ties to the smaller position (-0.0 equals +0.0), NaN after
    every number."""
    idx = np.nonzero(live)[0]
    num = idx[~np.isnan(v[idx])]
    return int(num[np.argmax(v[num])]) if len(num) else int(idx[0])


def ild_of(cos, picks, dtype=np.float64):
    """1 - mean cosine over the unordered pairs of picks, summed in pick order (pairs (p_u, p_t), t ascending, u < t)."""
    n = len(picks)
    if n < 2:
        return dtype(np.nan)
    t, u = np.tril_indices(n, -1)                                # (1, 0), (2, 0), (2, 1), ...: t ascending, u < t ascending
    p = np.asarray(picks)
    with np.errstate(all="ignore"):
        acc = np.add.accumulate(cos[p[u], p[t]].astype(dtype))[-1]       # a running sum: one accumulator, in this order
        return dtype(dtype(1) - dtype(acc / dtype(n * (n - 1) // 2)))


def mmr_row(items, ids, scores, lam, k, dtype=np.float64):
    """One row of the contract -> dict(picks: shortlist positions in pick order, ids [k] int64, scores [k] fp32, value [k]
    dtype, ild).  Slots past the picks hold -1 / -inf / -inf."""
    ids = np.asarray(ids, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    valid = valid_mask(ids, scores, items.shape[0])
    rel = relevance(scores, valid, dtype)
    cos = cosine_matrix(items, ids, valid, dtype)
    live = valid.copy()
    maxsim = np.zeros(len(ids), dtype=dtype)
    picks, values = [], []
    for t in range(min(int(k), int(valid.sum()))):
        v = _value(lam, rel, maxsim, dtype)
        p = _best(v, live)
        picks.append(p)
        values.append(v[p])
        live[p] = False
        maxsim = cos[p].copy() if t == 0 else np.fmax(maxsim, cos[p])
    out_ids = np.full(k, -1, dtype=np.int64)
    out_scores = np.full(k, -np.inf, dtype=np.float32)
    out_value = np.full(k, -np.inf, dtype=dtype)
    n = len(picks)
    out_ids[:n] = ids[picks]
    out_scores[:n] = scores[picks]
    out_value[:n] = values
    return {"picks": picks, "ids": out_ids, "scores": out_scores, "value": out_value, "ild": ild_of(cos, picks, dtype)}


def mmr_batch(items, ids, scores, lam, k, dtype=np.float64):
    rows = [mmr_row(items, ids[b], scores[b], lam, k, dtype) for b in range(len(ids))]
    return {"picks": [r["picks"] for r in rows], "ids": np.stack([r["ids"] for r in rows]),
            "scores": np.stack([r["scores"] for r in rows]), "value": np.stack([r["value"] for r in rows]),
            "ild": np.array([r["ild"] for r in rows], dtype=dtype)}


def picks_from_output(ids, scores, out_ids, out_scores, n_items):
    """Maps a returned row back to shortlist positions -> (picks, problems): each returned (id, score bits) pair must be a valid
    entry that was not used before; among equal pairs the earliest free position is taken (they are interchangeable).  problems
    lists what is wrong: a pick that is padding or repeated, a wrong number of picks, a tail that is not -1 / -inf."""
    ids = np.asarray(ids, dtype=np.int64)
    sbits = np.asarray(scores, dtype=np.float32).view(np.uint32)
    valid = valid_mask(ids, scores, n_items)
    obits = np.asarray(out_scores, dtype=np.float32).view(np.uint32)
    k = len(out_ids)
    n = min(k, int(valid.sum()))
    used = np.zeros(len(ids), dtype=bool)
    picks, problems = [], []
    for t in range(n):
        cand = np.nonzero(valid & ~used & (ids == out_ids[t]) & (sbits == obits[t]))[0]
        if len(cand) == 0:
            problems.append("slot %d: (id %d, score %r) is padding, repeated or not in the shortlist" % (t, out_ids[t], out_scores[t]))
            break
        picks.append(int(cand[0]))
        used[cand[0]] = True
    for t in range(n, k):
        if out_ids[t] != -1 or out_scores[t] != -np.inf:
            problems.append("slot %d past the %d picks holds (%d, %r)" % (t, n, out_ids[t], out_scores[t]))
    return picks, problems


def greedy_gap(items, ids, scores, lam, picks):
    """For the pick sequence ``picks`` (shortlist positions): per step t, max over the entries still available of v minus v of
    the entry that was picked, with v evaluated in float64 on the sequence's own prefix picks[:t] -> (gap [len(picks)] float64,
    value [len(picks)] float64, ild float64).  An exact greedy run has gap 0 everywhere."""
    ids = np.asarray(ids, dtype=np.int64)
    valid = valid_mask(ids, scores, items.shape[0])
    rel = relevance(scores, valid)
    cos = cosine_matrix(items, ids, valid)
    live = valid.copy()
    maxsim = np.zeros(len(ids))
    gap, value = np.zeros(len(picks)), np.zeros(len(picks))
    for t, p in enumerate(picks):
        v = _value(lam, rel, maxsim, np.float64)
        gap[t] = np.max(v[live]) - v[p]
        value[t] = v[p]
        live[p] = False
        maxsim = cos[p].copy() if t == 0 else np.fmax(maxsim, cos[p])
    return gap, value, ild_of(cos, list(picks))


def lattice_case(B, M, d, n_items=97, seed=0):
    """Tie-heavy data on which the whole contract is exact in fp32 -> (items [n_items, d], ids [B, M] int64, scores [B, M] fp32).

    Item rows are +-2^e times a unit axis vector (a few are zero rows), so every dot product is 0 or +-2^(e + e'), every norm a
    power of two and every cosine exactly 0 or +-1.  Scores are integers whose spread over a row's valid entries is 16 (or 0),
    so rel is a multiple of 1/16, and with lambda a multiple of 1/4 every v is a multiple of 1/64 of small magnitude.
    Rows end in -1 / -inf tails: row b's is b entries long while b <= min(M, 30), the next two rows are all padding and all
    but one entry, the rest are random; in front of the tail about one entry in eight is broken (ids -5, n_items, 2^40; scores
    NaN, +inf, -inf) and ids repeat freely (n_items is smaller than the lists are long)."""
    rng = np.random.default_rng([seed, B, M, d])
    items = np.zeros((n_items, d), dtype=np.float32)
    axis = rng.integers(0, d, size=n_items)
    mag = np.ldexp(1.0, rng.integers(-3, 4, size=n_items)) * rng.choice([-1.0, 1.0], size=n_items)
    items[np.arange(n_items), axis] = mag
    items[rng.random(n_items) < 0.08] = 0.0                      # zero-norm rows
    ids = rng.integers(0, n_items, size=(B, M)).astype(np.int64)
    scores = (rng.integers(-40, 41, size=(B, 1)) + rng.integers(0, 17, size=(B, M))).astype(np.float32)
    for b in range(B):
        if b <= min(M, 30):
            tail = b
        elif b == min(M, 30) + 1:
            tail = M
        elif b == min(M, 30) + 2:
            tail = M - 1
        else:
            tail = int(rng.integers(0, M + 1))
        head = M - tail
        broken = np.nonzero(rng.random(head) < 0.125)[0]
        for i in broken:
            kind = int(rng.integers(0, 6))
            if kind < 3:
                ids[b, i] = (-5, n_items, 2 ** 40)[kind]
            else:
                scores[b, i] = (np.nan, np.inf, -np.inf)[kind - 3]
        ids[b, head:] = -1
        scores[b, head:] = -np.inf
        good = np.nonzero(valid_mask(ids[b], scores[b], n_items))[0]
        if len(good) >= 2:                                       # the spread over the valid entries is exactly 16
            lo = np.float32(rng.integers(-40, 41))
            scores[b, good] = lo + rng.integers(0, 17, size=len(good)).astype(np.float32)
            two = rng.choice(good, size=2, replace=False)
            scores[b, two[0]], scores[b, two[1]] = lo, lo + np.float32(16)
    return items, ids, scores
