"""numpy restatement of the fp16 shortlist with a certificate (include/nrms_hip.h nrms_catalogue_pack_f16 / nrms_topk_dot_coarse):
the element rule h, the pitch and the stats in float64 with nextafter up, the shortlist rule, and the certificate with the coarse
scores passed in or formed in float64."""
import numpy as np

F = np.float32
INF = np.inf


def pitch(d):
    return 32 * ((int(d) + 31) // 32)


def up(x):
    """The next float64 towards +inf of every element."""
    return np.nextafter(np.asarray(x, dtype=np.float64), INF)


def f32_up(x):
    """The smallest float32 >= x (x float64 >= 0)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(F)
    low = f.astype(np.float64) < x
    return np.where(low, np.nextafter(f, F(INF)), f).astype(F)


def h(x):
    """float32 -> float16: a magnitude above 65504 becomes +-65504, one below 2^-14 +-0 (both decided on the fp32 input), the
    rest is rounded to nearest even.  Finite input."""
    x = np.asarray(x, dtype=F)
    a = np.abs(x)
    y = np.where(a > F(65504.0), np.copysign(F(65504.0), x), x)
    y = np.where(a < F(2.0 ** -14), np.copysign(F(0.0), x), y)
    return y.astype(np.float16)


def pack_rows(rows):
    """rows [n, d] float32 -> (bits uint16 [n, pitch], ok [n] bool, norms float64 [n, 3]): the fp16 copy (zeros for a row with a NaN
    or an infinity, ok False) and upper bounds of ||row||, ||h(row)||, ||row - h(row)|| in float64."""
    rows = np.asarray(rows, dtype=F)
    n, d = rows.shape
    ok = np.isfinite(rows).all(axis=1) if n else np.zeros(0, dtype=bool)
    safe = np.where(ok[:, None], rows, F(0))
    r16 = h(safe)
    bits = np.zeros((n, pitch(d)), dtype=np.uint16)
    bits[:, :d] = r16.view(np.uint16)
    x, y = safe.astype(np.float64), r16.astype(np.float64)
    norms = np.empty((n, 3), dtype=np.float64)
    for j, v in enumerate((x, y, x - y)):
        s0 = (v * v).sum(axis=1)
        s = up(s0 * (1.0 + (d + 64) * 2.0 ** -51))
        norms[:, j] = np.where(s0 == 0.0, 0.0, up(up(np.sqrt(s))))         # (a sum of 0 is exact)
    norms[~ok] = INF
    return bits, ok, norms


def pack(items):
    """items [N, d] float32 -> (items16 bits uint16 [N, pitch], stats float32 [2] = (NRM, ERR))."""
    bits, ok, norms = pack_rows(items)
    stats = np.zeros(2, dtype=F)
    if ok.any():
        stats[0] = f32_up(norms[ok, 0].max())
        stats[1] = f32_up(norms[ok, 2].max())
    if (~ok).any():
        stats[0] = F(INF)
    return bits, stats


def true_stats(items):
    """The float64 maxima the packed stats bound: (max ||row||, max ||row - h(row)||) over the finite rows."""
    items = np.asarray(items, dtype=F)
    ok = np.isfinite(items).all(axis=1)
    x = items[ok].astype(np.float64)
    if not len(x):
        return 0.0, 0.0
    y = h(items[ok]).astype(np.float64)
    return float(np.sqrt((x * x).sum(axis=1)).max()), float(np.sqrt(((x - y) ** 2).sum(axis=1)).max())


def halves(bits, d):
    """The float64 values of packed bits [n, pitch], columns [0, d)."""
    return np.ascontiguousarray(bits).view(np.float16)[:, :d].astype(np.float64)


def ordered(scores, exclude, k):
    """scores [B, N] float32, exclude [B, n] or None -> (ids [B, k] int64, scores [B, k] float32): nrms_topk_dot's rule: the
    eligible items (not excluded, not NaN) by score descending, then the smaller id; -1 / -inf in the missing slots."""
    scores = np.asarray(scores, dtype=F)
    B, N = scores.shape
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -INF, dtype=F)
    for b in range(B):
        el = ~np.isnan(scores[b])
        if exclude is not None:
            ex = np.asarray(exclude[b], dtype=np.int64)
            el[ex[(ex >= 0) & (ex < N)]] = False
        n = np.nonzero(el)[0]
        s = scores[b, n] + F(0.0)                                    # -0.0 is +0.0
        order = np.lexsort((n, -s.astype(np.float64)))[:k]
        ids[b, :len(order)] = n[order]
        out[b, :len(order)] = s[order]
    return ids, out


def e_bound(d, un, un16, ue, NRM, ERR):
    """E_b of the certificate in float64, every product and sum rounded up."""
    d = float(d)
    gamma = up(up(d * 2.0 ** -24) / (1.0 - d * 2.0 ** -24))
    alpha = d * 2.0 ** -21
    E = up(ue * NRM)
    E = up(E + up(un16 * ERR))
    E = up(E + up(gamma * up(un * NRM)))
    E = up(E + up(alpha * up(un16 * up(NRM + ERR))))
    return up(E + up(d * 2.0 ** -140))


def alpha(d):
    return d * 2.0 ** -21


def certificate(d, k, M, unorm, stats, short_ids, short_scores, exact_topk_scores):
    """unorm [B, 3] float64 (un, un16, ue), stats float32 [2], the shortlist [B, M] and the exact top-k scores of the shortlist
    [B, k] -> (certified [B] bool, margin [B] = (s_k - c_M) / E_b, NaN where the shortlist is not full)."""
    B = short_ids.shape[0]
    NRM, ERR = float(stats[0]), float(stats[1])
    cert = np.zeros(B, dtype=bool)
    margin = np.full(B, np.nan)
    for b in range(B):
        un, un16, ue = (float(v) for v in unorm[b])
        with np.errstate(invalid="ignore", over="ignore"):
            ok = all(np.isfinite(v) for v in (NRM, ERR, un, un16, ue)) and d < 2 ** 23 and float(up(un * NRM)) <= 2.0 ** 100
            L = int((short_ids[b] >= 0).sum())
            if ok and L >= M:
                E = float(e_bound(d, un, un16, ue, NRM, ERR))
                sk, cM = float(exact_topk_scores[b, k - 1]), float(short_scores[b, M - 1])
                margin[b] = (sk - cM) / E if E > 0 else INF
                ok = np.isfinite(sk) and sk > float(up(cM + E))
        cert[b] = ok
    return cert, margin


def coarse_scores64(user, items):
    """The coarse scores formed in float64 from the fp16 copies, rounded to float32: u16 . n16."""
    u16 = halves(pack_rows(user)[0], user.shape[1])
    n16 = halves(pack_rows(items)[0], items.shape[1])
    return (u16 @ n16.T).astype(F)


def exact_scores64(user, items):
    """The exact scores formed in float64 and rounded to float32 (within gamma_d of any fp32 chain)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(user, dtype=np.float64) @ np.asarray(items, dtype=np.float64).T).astype(F)


def topk_coarse(user, items, k, M, exclude=None, coarse=None, exact=None):
    """The whole call: -> dict(ids, scores [B, k]; certified, margin [B]; short_ids, short_scores [B, M]).  coarse / exact [B, N]
    float32: the score matrices (None: formed in float64)."""
    user, items = np.asarray(user, dtype=F), np.asarray(items, dtype=F)
    d = user.shape[1]
    coarse = coarse_scores64(user, items) if coarse is None else coarse
    exact = exact_scores64(user, items) if exact is None else exact
    short_ids, short_scores = ordered(coarse, exclude, M)
    B = user.shape[0]
    ids = np.full((B, k), -1, dtype=np.int64)
    scores = np.full((B, k), -INF, dtype=F)
    for b in range(B):
        real = short_ids[b][short_ids[b] >= 0]
        masked = np.full((1, exact.shape[1]), np.nan, dtype=F)
        masked[0, real] = exact[b, real]
        i, s = ordered(masked, None, k)
        ids[b], scores[b] = i[0], s[0]
    _, stats = pack(items)
    unorm = pack_rows(user)[2]
    cert, margin = certificate(d, k, M, unorm, stats, short_ids, short_scores, scores)
    return dict(ids=ids, scores=scores, certified=cert, margin=margin, short_ids=short_ids, short_scores=short_scores)
