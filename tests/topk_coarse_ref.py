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


E_TERMS = ("ue*NRM", "un16*ERR", "gamma", "alpha", "underflow")


def e_terms(d, un, un16, ue, NRM, ERR):
    """The terms of E_b in the order of E_TERMS, each with every product rounded up: ue NRM, un16 ERR, gamma_d un NRM,
    alpha_d un16 (NRM + ERR), d 2^-140."""
    d = float(d)
    gamma = up(up(d * 2.0 ** -24) / (1.0 - d * 2.0 ** -24))
    alpha = d * 2.0 ** -21
    return (up(ue * NRM), up(un16 * ERR), up(gamma * up(un * NRM)), up(alpha * up(un16 * up(NRM + ERR))), up(d * 2.0 ** -140))


def e_bound(d, un, un16, ue, NRM, ERR, drop=None):
    """E_b of the certificate in float64: the terms of e_terms added in their order, every sum rounded up.  drop: the name of one
    term to leave out (a deliberately wrong bound, for the tests that show the data can tell)."""
    terms = [t for name, t in zip(E_TERMS, e_terms(d, un, un16, ue, NRM, ERR)) if name != drop]
    E = terms[0]
    for t in terms[1:]:
        E = up(E + t)
    return E


def alpha(d):
    return d * 2.0 ** -21


def certificate(d, k, M, unorm, stats, short_ids, short_scores, exact_topk_scores, drop=None):
    """unorm [B, 3] float64 (un, un16, ue), stats float32 [2], the shortlist [B, M] and the exact top-k scores of the shortlist
    [B, k] -> (certified [B] bool, margin [B] = (s_k - c_M) / E_b, NaN where the shortlist is not full).  drop: as e_bound's."""
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
                E = float(e_bound(d, un, un16, ue, NRM, ERR, drop))
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


def graded(B, N, d, eps, seed):
    """-> (user [B, d], items [N, d]) float32 whose certificate margins are graded inside one batch: items within eps of one
    direction, users of one random part orthogonal to it and a part along it that grows 64-fold over the batch."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((1, d))
    items = (base + eps * rng.standard_normal((N, d))).astype(F)
    bdir = base / np.linalg.norm(base)
    g = rng.standard_normal((B, d))
    g -= (g @ bdir.T) * bdir
    t = 4.0 ** np.linspace(-1.5, 1.5, B)[:, None]
    return (g + t * np.sqrt(d) * bdir).astype(F), items


# (B, N, d, k, M, eps, seed) of graded(): the certified share is between 0.2 and 0.8 at each, and every term of E_b but d 2^-140
# decides rows (tests/test_topk_coarse_host.py::test_graded_margins_straddle_one_and_tell_the_terms_apart holds them to that)
GRADED = [(264, 2500, 300, 10, 64, 0.014, 1), (264, 2500, 80, 5, 16, 0.011, 2), (264, 2500, 160, 1, 8, 0.012, 4),
          (264, 2500, 300, 100, 192, 0.03, 5), (264, 2500, 1024, 10, 64, 0.045, 6)]
# (B, N, d, k) of the runs at M = k
TIGHT = [(70, 2500, 300, 10), (70, 2500, 80, 5), (33, 2500, 160, 1)]


def near_tied(B, N, d, seed, noise=1e-3):
    """Gaussian users; items within noise of one direction: the scores of a user differ by less than the fp16 copy's error."""
    rng = np.random.default_rng(seed)
    user = rng.standard_normal((B, d)).astype(F)
    items = (rng.standard_normal((1, d)) + noise * rng.standard_normal((N, d))).astype(F)
    return user, items


def dominant(B, N, d, k, seed):
    """Gaussian items with k of them multiplied by 50, and Gaussian users moved 6 along each of those k directions, so that every
    user scores the k far above the rest (and NRM, with it E_b, is 50 times a Gaussian catalogue's)."""
    rng = np.random.default_rng(seed)
    items = rng.standard_normal((N, d)).astype(F)
    dom = rng.choice(N, size=k, replace=False)
    items[dom] *= 50
    unit = items[dom].astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    return (rng.standard_normal((B, d)) + 6.0 * unit.sum(axis=0)).astype(F), items


def out_of_range(B, N, d, seed):
    """-> (user, items, kind [B]).  Gaussian items; 400 entries become +-2^-15, +-1e-6 (h: 0) or +-6e-5 (just below 2^-14), and six
    rows get one entry of +-7e4 or +-6.9e4 (h: +-65504), each in a column of its own.  Users by kind: 0 scaled by 2^-16 (h(u) = 0:
    every coarse score is 0), 1 with one entry of +-1e6 (for two thirds of them in the column and with the sign of a clamped item
    entry, so that one exact score is 7e10 beside an E_b of 6.6e10), 2 untouched."""
    rng = np.random.default_rng(seed)
    items = rng.standard_normal((N, d)).astype(F)
    flat = items.reshape(-1)
    at = rng.choice(flat.size, size=400, replace=False)
    flat[at] = (rng.choice([2.0 ** -15, 1e-6, 6.0e-5], size=400) * rng.choice([-1.0, 1.0], size=400)).astype(F)
    rows, cols = rng.choice(N, size=6, replace=False), rng.choice(d, size=6, replace=False)
    items[rows, cols] = (rng.choice([7.0e4, 6.9e4], size=6) * rng.choice([-1.0, 1.0], size=6)).astype(F)
    user = np.clip(rng.standard_normal((B, d)), -3.9, 3.9).astype(F)
    kind = np.arange(B) % 3
    user[kind == 0] *= F(2.0 ** -16)
    for i, b in enumerate(np.nonzero(kind == 1)[0]):
        j = i % 9
        col, sign = (cols[j], np.sign(items[rows[j], cols[j]])) if j < 6 else (int(rng.integers(0, d)), 1.0)
        user[b, col] = 1e6 * sign * (-1.0 if i % 4 == 3 else 1.0)
    return user, items, kind


def topk_coarse(user, items, k, M, exclude=None, coarse=None, exact=None):
    """The whole call: -> dict(ids, scores [B, k]; certified, margin [B]; short_ids, short_scores [B, M]; unorm [B, 3], stats [2]).
    coarse / exact [B, N] float32: the score matrices (None: formed in float64)."""
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
    return dict(ids=ids, scores=scores, certified=cert, margin=margin, short_ids=short_ids, short_scores=short_scores, unorm=unorm,
                stats=stats)
