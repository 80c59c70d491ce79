"""The contract of nrms_attribution_dot (include/nrms_hip.h) restated in numpy.

attribution(ctx, w, items, ids, m, slot_named) -> dict(contrib [B, K, H], total [B, K], top_slots [B, K, m] int32, top_contrib
[B, K, m], unnamed_share [B, K]).  Two uses of the terms:
  terms64: s = ctx . item in float64 and c = w * s in float64: the yardstick of the tolerance checks (with `bound`);
  attribution: the same, rounded to float32 once.  On LATTICE data (lattice_case: small integers times powers of two, every
      product, partial sum of a dot product, term and partial sum of terms exact in fp32) the float64 value IS the fp32 value of
      any summation order, so the result is what the kernel must return bit for bit.
`finish` does everything after the terms, from float32 terms, in the contract's own arithmetic: the sequential fp32 sum from
+0.0 in slot order, the unnamed share likewise, the order (c descending, -0.0 = +0.0, the smaller slot first), NaN and unnamed
slots ineligible, -0.0 returned as +0.0, invalid entries (total -inf, share 0, reasons -1 / -inf, zero terms).  It is also what
the Gaussian-data tests apply to the terms they build from nrms_rank_dot's scores."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def valid_ids(ids, N):
    ids = np.asarray(ids, dtype=np.int64)
    return (ids >= 0) & (ids < N)


def terms64(ctx, w, items, ids):
    """c(b, j, h) in float64 from the fp32 inputs, 0 for invalid entries -> [B, K, H]."""
    ctx, w, items = (np.asarray(a, dtype=np.float64) for a in (ctx, w, items))
    ids = np.asarray(ids, dtype=np.int64)
    B, H, d = ctx.shape
    K = ids.shape[1]
    ok = valid_ids(ids, len(items))
    out = np.zeros((B, K, H))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            if ok[b].any():
                x = items[ids[b][ok[b]]]                               # [k, d]
                # + 0.0: a zero dot product is +0.0, as an accumulator that starts from +0.0 leaves it, whatever the BLAS does
                out[b][ok[b]] = (x @ ctx[b].T + 0.0) * w[b][None, :]
    return out


def bound(ctx, w, items, ids):
    """(d + H + 2) 2^-24 sum_h |w_h| sum_k |ctx_hk x_k| -> [B, K]: the forward error bound of a d-term dot product, one multiply
    and an H-term sum, all in fp32 (unit roundoff 2^-24); 0 for invalid entries."""
    B, H, d = np.asarray(ctx).shape
    mag = terms64(np.abs(ctx), np.abs(w), np.abs(items), ids).sum(-1)
    return (d + H + 2) * 2.0 ** -24 * mag


def seq_sum32(c):
    """The fp32 sum of c[..., h] over h = 0, 1, ... in that order, from +0.0 -> c.shape[:-1]."""
    c = np.asarray(c, dtype=np.float32)
    acc = np.zeros(c.shape[:-1], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(c.shape[-1]):
            acc = (acc + c[..., h]).astype(np.float32)
    return acc


def finish(contrib, ids, N, m, slot_named=None):
    contrib = np.array(contrib, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    B, K, H = contrib.shape
    ok = valid_ids(ids, N)
    named = np.ones((B, H), dtype=bool) if slot_named is None else np.asarray(slot_named).reshape(B, H) != 0
    contrib[~ok] = 0.0
    total = np.where(ok, seq_sum32(contrib), NEG_INF).astype(np.float32)
    unnamed = np.zeros((B, K), dtype=np.float32)
    top_slots = np.full((B, K, m), -1, dtype=np.int32)
    top_contrib = np.full((B, K, m), NEG_INF, dtype=np.float32)
    for b in range(B):
        un = np.nonzero(~named[b])[0]
        for j in range(K):
            if not ok[b, j]:
                continue
            c = contrib[b, j]
            if len(un):
                unnamed[b, j] = seq_sum32(c[un])
            elig = [h for h in range(H) if named[b, h] and not np.isnan(c[h])]
            elig.sort(key=lambda h: (-float(c[h]), h))                  # -0.0 == +0.0 as a key; the smaller slot first
            for p, h in enumerate(elig[:m]):
                top_slots[b, j, p] = h
                top_contrib[b, j, p] = c[h] + np.float32(0.0) if c[h] == 0 else c[h]       # -0.0 is returned as +0.0
    return dict(contrib=contrib, total=total, top_slots=top_slots, top_contrib=top_contrib, unnamed_share=unnamed)


def attribution(ctx, w, items, ids, m, slot_named=None):
    c = terms64(ctx, w, items, ids)
    with np.errstate(over="ignore"):
        return finish(c.astype(np.float32), ids, len(items), m, slot_named)


def lattice_case(B, H, d, K, N, seed=0, ties=True):
    """(ctx, w, items, ids): ctx and items in {-2 .. 2} (mostly 0 for d > 64, so that |dot| <= 2^10), w in {0, 1/8, .. 1} times
    +-1: a dot product is an integer below 2^11, a term a multiple of 1/8 below 2^11, a sum of 64 of them below 2^17: all exact
    in fp32 in every order.  With `ties` half of the slots repeat the ctx row and weight of another slot, so runs of equal
    contributions occur in every row; ids hold -1, N and duplicates."""
    rng = np.random.default_rng(seed)
    keep = min(1.0, 48.0 / d)
    ctx = (rng.integers(-2, 3, (B, H, d)) * (rng.random((B, H, d)) < keep)).astype(np.float32)
    items = (rng.integers(-2, 3, (N, d)) * (rng.random((N, d)) < keep)).astype(np.float32)
    w = (rng.integers(0, 9, (B, H)) / 8.0 * rng.choice([-1.0, 1.0], (B, H))).astype(np.float32)
    if ties and H > 1:
        for b in range(B):
            src = rng.integers(0, H, H // 2)
            dst = rng.integers(0, H, H // 2)
            ctx[b, dst] = ctx[b, src]
            w[b, dst] = w[b, src]
    ids = rng.integers(0, max(N, 1), (B, K)).astype(np.int64)
    if N == 0:
        ids[:] = 0
    flat = ids.reshape(-1)
    flat[rng.random(flat.size) < 0.08] = -1
    flat[rng.random(flat.size) < 0.04] = N
    if K > 2:
        ids[:, K // 2] = ids[:, 0]                                      # a duplicate in every row
    return ctx, w, items, ids


def lattice_is_exact(ctx, w, items, ids):
    """Every |term| and every sum of |terms| of the case stays an exact fp32 number: multiples of 1/8 below 2^20."""
    mag = terms64(np.abs(ctx), np.abs(w), np.abs(items), ids)
    dots = np.abs(np.asarray(items, np.float64)).sum(-1).max(initial=0) * np.abs(np.asarray(ctx, np.float64)).max(initial=0)
    return bool(dots < 2 ** 20 and mag.sum(-1).max(initial=0) < 2 ** 20 and np.array_equal(mag * 8, np.round(mag * 8)))
