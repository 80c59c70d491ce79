"""Float64 numpy restatements of the formulas include/nrms_hip.h gives for the news feature rows (nrms_news_features_fwd / _bwd,
csrc/wide.hip) and for HieRec's matching (nrms_hier_match, nrms_hier_query, nrms_hier_score_fwd / _bwd, csrc/hier.hip), with the
quantities an error bound needs beside every sum, and the case table of tests/test_hip_sideops.py.  Checked on the CPU against
float64 torch autograd in tests/test_sideops_ref_host.py.

Bounds.  u = 2^-24 is the unit roundoff of fp32.  A result that adds up m fp32 terms in any order, each term the outcome of at
most r rounded operations on exact inputs, differs from the exact sum by at most (m + r + 2) u S, S = sum |term| (Higham, Accuracy
and Stability of Numerical Algorithms, section 4.2: every term meets at most m - 1 rounded additions and r rounded operations of
its own; the 2 pays for the second-order terms of (1 + u)^(m + r) at these m).  A kernel that contracts a product and an addition
into one fma rounds less often, never more.  Where the finished sum is added to a value the buffer held, that one addition adds
u |start + sum|.  Every function below returns m and S next to its sums; r is stated where the bound is used."""
import numpy as np

U = 2.0 ** -24


def sum_bound(m, r, S, start_plus_ref=None):
    """(m + r + 2) u S, plus u |start + ref| for a sum added to what the buffer held."""
    b = (np.asarray(m, dtype=np.float64) + r + 2) * U * S
    return b if start_plus_ref is None else b + U * np.abs(start_plus_ref)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- news feature rows ---------------------------------------------------------------------------------------------------------------
def _scale(keep, p, shape):
    """The dropout factor per element: keep / (1 - p) with p the fp32 value the library is given; all ones at p = 0."""
    if keep is None or p == 0:
        return np.ones(shape)
    return f64(keep).reshape(shape) / (1.0 - float(np.float32(p)))


def _rows(ids, n_rows):
    ids = np.asarray(ids, dtype=np.int64)
    return np.where((ids < 0) | (ids >= n_rows), 0, ids)


def features_fwd_ref(title, abst, cat_table, sub_table, categ, subcateg, keep, p):
    """out[n] = dropout([title[n] | abst[n] | cat_table[categ[n]] | sub_table[subcateg[n]]]); an id outside its table reads row 0.
    keep: uint8 [n, 2 dt + 2 dc] (nrms_dropout_keep_mask site 3) or None."""
    cat_table, sub_table = f64(cat_table), f64(sub_table)
    row = np.concatenate([f64(title), f64(abst), cat_table[_rows(categ, cat_table.shape[0])],
                          sub_table[_rows(subcateg, sub_table.shape[0])]], axis=1)
    return row * _scale(keep, p, row.shape)


def features_bwd_ref(dout, categ, subcateg, d_text, d_cat, n_cat, n_sub, keep, p):
    """dict: d_title, d_abst [n, dt] = the masked, scaled slices of dout; d_cat [n_cat, dc], d_sub [n_sub, dc] = the sums over the
    slots whose id lies in [1, rows) (row 0 = padding_idx and ids outside the table receive nothing); for each table m_* [rows, 1]
    (terms per element) and S_* (sum |term|)."""
    g = f64(dout) * _scale(keep, p, np.shape(dout))
    out = {"d_title": g[:, :d_text], "d_abst": g[:, d_text:2 * d_text]}
    for name, ids, rows, c0 in (("cat", categ, n_cat, 2 * d_text), ("sub", subcateg, n_sub, 2 * d_text + d_cat)):
        ids = np.asarray(ids, dtype=np.int64)
        named = (ids >= 1) & (ids < rows)
        terms = g[named, c0:c0 + d_cat]
        total, S, m = np.zeros((rows, d_cat)), np.zeros((rows, d_cat)), np.zeros((rows, 1))
        np.add.at(total, ids[named], terms)
        np.add.at(S, ids[named], np.abs(terms))
        np.add.at(m, ids[named], 1.0)
        out["d_" + name], out["S_" + name], out["m_" + name] = total, S, m
    return out


def _features_bwd_chunks(n, dt, dc, n_cat, n_sub):
    """(table rows that take a gradient, chunk count before the fit loop, chunk count after it)."""
    rows = (n_cat - 1) + (n_sub - 1)
    chunks = min(8192 // rows, 64) if rows > 0 else 0
    windows = (n + 127) // 128
    chunks = wanted = min(chunks, windows)
    while chunks > 1 and chunks * rows * dc > n * dt:                   # the partial sums must fit into d_title_vec
        chunks -= 1
    return rows, wanted, chunks


def features_bwd_plan(n, dt, dc, n_cat, n_sub):
    """("single", windows) or ("chunked", n_chunks, slots of the last chunk): which table-gradient path nrms_news_features_bwd takes.
    MUST FOLLOW launch_features_bwd (csrc/wide.hip) -- it restates the launcher's choice and is used only to prove that
    FEATURE_CASES holds every path (tests/test_sideops_ref_host.py); no expected value comes from it."""
    rows, _, chunks = _features_bwd_chunks(n, dt, dc, n_cat, n_sub)
    windows = (n + 127) // 128
    if rows <= 0 or chunks <= 1:
        return ("single", windows)
    chunk = ((n + chunks - 1) // chunks + 127) // 128 * 128
    n_chunks = (n + chunk - 1) // chunk
    return ("chunked", n_chunks, n - (n_chunks - 1) * chunk)


# (n, d_text, d_cat, n_cat, n_sub): derived from launch_features_bwd; test_sideops_ref_host.py states what each one reaches
FEATURE_CASES = [
    (1, 4, 4, 2, 2),            # one slot, one-row tables
    (127, 8, 8, 3, 4),          # single path, one partial window
    (128, 8, 8, 3, 4),          # single path, one full window
    (129, 8, 8, 3, 4),          # chunked, 2 chunks, the last holds 1 slot
    (256, 8, 8, 3, 4),          # chunked, 2 full chunks
    (257, 8, 8, 3, 4),          # chunked, 3 chunks, the last holds 1 slot
    (300, 8, 8, 3, 4),          # chunked, 3 chunks, the last holds 44 slots
    (129, 4, 64, 5, 9),         # the partial sums do not fit: chunks 2 -> 1, single path over 2 windows
    (600, 4, 48, 5, 9),         # chunks 5 -> 4 by the fit loop, chunk = 256 slots, 3 chunks
    (300, 8, 132, 3, 4),        # d_cat > 128: a second column step, chunked
    (100, 8, 132, 3, 4),        # the same on the single path
    (5200, 8, 4, 60, 142),      # 200 rows: 8192 / rows = 40 chunks wanted
    (130, 4, 4, 2, 8300),       # 8192 / rows = 0: single path, thousands of row blocks, 2 windows
    (16385, 4, 4, 3, 4),        # the forward's and the text backward's grid cap of 16 384: one block takes a second slot
    (300, 8, 8, 1, 4),          # n_cat = 1: no category row takes a gradient
]
# one batch, two paths: the ids and the table columns of dout of this case with d_text = 8 (chunked) and d_text = 1 (the fit
# loop leaves one chunk: single path).  The 300-slot case with d_cat = 8 would stay chunked at d_text = 1 (3 * 5 * 8 <= 300).
TWO_PATH_CASE = (300, 132, 3, 4)
TWO_PATH_D_TEXT = (8, 1)


def feature_ids(n, n_cat, n_sub, rng):
    """categ, subcateg int64 [n] from [-1, rows] inclusive (0 = padding, -1 and rows = outside the table), with
    * one row that every window of 128 slots names ("hot": category row 1, or sub-category row 1 when n_cat = 1),
    * rows that no slot names ("cold": the last row of a table that has a row to spare),
    * 0, -1 and rows themselves at slots 1, 2, 3 where n allows.
    Returns (categ, subcateg, cold_cat_rows, cold_sub_rows)."""
    categ = rng.integers(-1, n_cat + 1, size=n)
    sub = rng.integers(-1, n_sub + 1, size=n)
    hot_ids = categ if n_cat >= 2 else sub
    cold_cat = [n_cat - 1] if n_cat >= 3 else []
    cold_sub = [n_sub - 1] if (n_sub >= 3 or n_cat >= 2) and n_sub >= 2 else []
    for ids, cold in ((categ, cold_cat), (sub, cold_sub)):
        for r in cold:
            ids[ids == r] = 0
    if n >= 5:
        for ids, rows, at in ((categ, n_cat, (1, 2, 3)), (sub, n_sub, (3, 1, 2))):
            ids[at[0]], ids[at[1]], ids[at[2]] = 0, -1, rows
    for w in range((n + 127) // 128):
        hot_ids[min(128 * w + (53 * w) % 128, n - 1)] = 1
    assert not (set(cold_cat) & set(categ.tolist())) and not (set(cold_sub) & set(sub.tolist())) and cold_cat + cold_sub
    return categ.astype(np.int64), sub.astype(np.int64), cold_cat, cold_sub


# ---- hierarchical matching -----------------------------------------------------------------------------------------------------------
def _coef(lam, frac, slot):
    """lambda * share where the slot exists, 0 where it is -1 (the share stored beside a missing slot is not read)."""
    return np.where(np.asarray(slot) >= 0, float(np.float32(lam)) * f64(frac), 0.0)


def _lambda_global(lambda_sub, lambda_top):
    return 1.0 - float(np.float32(lambda_sub)) - float(np.float32(lambda_top))


def _user_side(u1, u2, ug, sub_slot, sub_frac, top_slot, top_frac, lambda_sub, lambda_top):
    """The three terms cs u1[ss], ct u2[ts], lg ug[b] per candidate: each [B, C, d]."""
    u1, u2, ug = f64(u1), f64(u2), f64(ug)
    ss, ts = np.asarray(sub_slot, dtype=np.int64), np.asarray(top_slot, dtype=np.int64)
    cs, ct = _coef(lambda_sub, sub_frac, ss), _coef(lambda_top, top_frac, ts)
    return (cs[..., None] * u1[np.maximum(ss, 0)], ct[..., None] * u2[np.maximum(ts, 0)],
            _lambda_global(lambda_sub, lambda_top) * np.broadcast_to(ug[:, None, :], ss.shape + (ug.shape[1],)), cs, ct)


def hier_score_ref(cand, u1, u2, ug, sub_slot, sub_frac, top_slot, top_frac, mask, lambda_sub, lambda_top):
    """score[b, c] = sum_k n[k] (l_s f_s u1[ss][k] + l_t f_t u2[ts][k] + (1 - l_s - l_t) ug[b][k]), a term whose slot is -1 absent;
    masked candidates -1e9.  cand [B, C, d]; slots, shares, mask [B, C].  Returns (scores, S): m = d terms per score, S = sum_k |n[k]|
    (|first| + |second| + |third|)."""
    t1, t2, tg, _, _ = _user_side(u1, u2, ug, sub_slot, sub_frac, top_slot, top_frac, lambda_sub, lambda_top)
    n = f64(cand)
    scores = (n * (t1 + t2 + tg)).sum(-1)
    S = (np.abs(n) * (np.abs(t1) + np.abs(t2) + np.abs(tg))).sum(-1)
    if mask is not None:
        scores = np.where(np.asarray(mask) != 0, scores, -1e9)
    return scores, S


def hier_score_bwd_ref(cand, u1, u2, ug, sub_slot, sub_frac, top_slot, top_frac, mask, lambda_sub, lambda_top, dscores):
    """The gradients of sum(dscores * score) over the live candidates (a masked one passes none).  dict:
    dcand [B, C, d] with S_dcand (m = 3 terms each);  du1, du2 [B * H, d] = the sums over the candidates that point at the row, with
    S_du1 / S_du2 and m_du1 / m_du2 [B * H, 1];  dug [B, d] with S_dug (m = C terms each)."""
    t1, t2, tg, cs, ct = _user_side(u1, u2, ug, sub_slot, sub_frac, top_slot, top_frac, lambda_sub, lambda_top)
    n = f64(cand)
    B, C, d = n.shape
    ds = f64(dscores) if mask is None else np.where(np.asarray(mask) != 0, f64(dscores), 0.0)
    gn = ds[..., None] * n                                                # d score / d (user side), per candidate
    out = {"dcand": ds[..., None] * (t1 + t2 + tg), "S_dcand": np.abs(ds)[..., None] * (np.abs(t1) + np.abs(t2) + np.abs(tg))}
    for name, slot, coef, rows in (("du1", sub_slot, cs, np.shape(u1)[0]), ("du2", top_slot, ct, np.shape(u2)[0])):
        slot = np.asarray(slot, dtype=np.int64)
        has = slot >= 0
        terms = coef[has][:, None] * gn[has]
        total, S, m = np.zeros((rows, d)), np.zeros((rows, d)), np.zeros((rows, 1))
        np.add.at(total, slot[has], terms)
        np.add.at(S, slot[has], np.abs(terms))
        np.add.at(m, slot[has], 1.0)
        out[name], out["S_" + name], out["m_" + name] = total, S, m
    lg = _lambda_global(lambda_sub, lambda_top)
    out["dug"], out["S_dug"] = (lg * gn).sum(1), np.abs(lg * gn).sum(1)
    return out


def hier_match_ref(B, C, H, cand_topic, cand_subtopic, l1_sub, l1_cnt, l2_top, l2_cnt, n_valid):
    """(sub_slot int32, sub_frac float32, top_slot, top_frac), each [B, C]: the lowest occupied slot b * H + g of user b that carries
    the candidate's id (a slot with count 0 never matches; none: -1 and share 0), share = count * (1 / n_valid) in fp32."""
    ct, cs = np.asarray(cand_topic).reshape(B, C), np.asarray(cand_subtopic).reshape(B, C)
    out = (np.full((B, C), -1, np.int32), np.zeros((B, C), np.float32), np.full((B, C), -1, np.int32), np.zeros((B, C), np.float32))
    for b in range(B):
        inv = np.float32(1.0) / np.float32(n_valid[b]) if n_valid[b] > 0 else np.float32(0.0)
        for c in range(C):
            for ids, cnt, want, slot, frac in ((l1_sub, l1_cnt, cs[b, c], out[0], out[1]), (l2_top, l2_cnt, ct[b, c], out[2], out[3])):
                for g in range(H):
                    s = b * H + g
                    if cnt[s] > 0 and ids[s] == want:
                        slot[b, c], frac[b, c] = s, np.float32(cnt[s]) * inv
                        break
    return out


def hier_query_ref(B, H, group_topic, group_subtopic, l1_sub, l1_cnt, l2_top, l2_cnt, n_valid, u1, u2, ug, lambda_sub, lambda_top):
    """query[b, g] = cs u1[ss] + ct u2[ts] + lg ug[b] with the slots and fp32 shares hier_match_ref gives a candidate with group g's
    ids.  Returns (query [B, G, d], S = |cs u1[ss]| + |ct u2[ts]| + |lg ug[b]|)."""
    G = len(group_topic)
    tile = lambda a: np.tile(np.asarray(a).reshape(1, G), (B, 1))
    ss, sf, ts, tf = hier_match_ref(B, G, H, tile(group_topic), tile(group_subtopic), l1_sub, l1_cnt, l2_top, l2_cnt, n_valid)
    t1, t2, tg, _, _ = _user_side(u1, u2, ug, ss, sf, ts, tf, lambda_sub, lambda_top)
    return t1 + t2 + tg, np.abs(t1) + np.abs(t2) + np.abs(tg)


# ---- hand-built matching inputs (tests/test_hip_sideops.py; no interest tree is needed) --------------------------------------------
HIER_H = 6


def hier_score_batch(B, C, d, rng, with_mask=True):
    """Slot lists and data for nrms_hier_score_fwd / _bwd, H = HIER_H.  A candidate's slots lie in its own user's range [b H, b H + H)
    (what nrms_hier_match produces; the backward gives a user's rows to one wave).  Random draws leave a quarter of the slots at -1;
    on top of that, as far as B * C holds them: the last three candidates of the last user point at one u1 row and the first two of
    them at one u2 row, and the other candidates, in flat order, are: both slots -1, only the sub-topic slot, only the topic slot,
    masked (with a finite non-zero dscores), a sub-topic share of 0.  A share beside a -1 slot is non-zero and must not be read.
    |cand|, |dscores| lie in [0.5, 1.5] and non-zero shares in [1/8, 1], so every non-zero term of du1 / du2 is at least
    0.15 / 8 * 0.25 > 0.0046 (see test_hier_score_backward for why that matters)."""
    H = HIER_H
    signed = lambda *shape: (rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    base = (np.arange(B) * H)[:, None]
    ss = np.where(rng.random((B, C)) < 0.25, -1, base + rng.integers(0, H, (B, C))).astype(np.int32)
    ts = np.where(rng.random((B, C)) < 0.25, -1, base + rng.integers(0, H, (B, C))).astype(np.int32)
    sf = (rng.integers(1, 9, (B, C)) / 8.0).astype(np.float32)
    tf = (rng.integers(1, 9, (B, C)) / 8.0).astype(np.float32)
    mask = np.ones((B, C), np.uint8)
    shared = []
    if C >= 3:
        b = B - 1
        shared = [b * C + c for c in (C - 3, C - 2, C - 1)]
        ss[b, C - 3:] = b * H + 2
        ts[b, C - 3:C - 1] = b * H + 4
    free = [i for i in range(B * C) if i not in shared]
    kinds = {}
    for kind, i in zip(("none", "sub_only", "top_only", "masked", "zero_share"), free):
        b, c = divmod(i, C)
        kinds[kind] = (b, c)
        if kind == "none":
            ss[b, c] = ts[b, c] = -1
        elif kind == "sub_only":
            ss[b, c], ts[b, c] = b * H + 1, -1
        elif kind == "top_only":
            ss[b, c], ts[b, c] = -1, b * H + 3
        elif kind == "masked":
            ss[b, c], ts[b, c], mask[b, c] = b * H, b * H + 5, 0
        else:
            ss[b, c], ts[b, c], sf[b, c] = b * H + 5, b * H, 0.0
    return dict(B=B, C=C, d=d, H=H, cand=signed(B, C, d), u1=rng.standard_normal((B * H, d)).astype(np.float32),
                u2=rng.standard_normal((B * H, d)).astype(np.float32), ug=rng.standard_normal((B, d)).astype(np.float32),
                sub_slot=ss, sub_frac=sf, top_slot=ts, top_frac=tf, mask=mask if with_mask else None, dscores=signed(B, C),
                kinds=kinds, shared=shared)


# ids of the hand-built group lists: X sits in several slots of a user, Y in a high slot, Z in none
ID_X, ID_Y, ID_Z = 11, 23, 37
MATCH_N_VALID = (0, 7, 3, 49)


def match_lists(H, rng):
    """Group lists of four users, the same construction for the sub-topic level (l1_sub, l1_cnt) and the topic level (l2_top,
    l2_cnt) with different counts:
      user 0: n_valid = 0, every slot count 0 and id X -- nothing matches, every share 0;
      user 1: X in slots 0 and 1 with count 0, then in two occupied slots (H = 64: slots 2 and 5) -- the lower occupied one wins;
              H = 1: its only slot holds X, occupied;
      user 2: random ids from {X, Y, 40..45}, random counts from {0, 1, 2, 5};
      user 3: Y occupied in slot H - 1 and with count 0 in every slot below.
    Returns dict(l1_sub, l1_cnt, l2_top, l2_cnt int32 [4 H], n_valid int32 [4])."""
    B = 4
    out = {}
    for ids_name, cnt_name, bump in (("l1_sub", "l1_cnt", 0), ("l2_top", "l2_cnt", 1)):
        ids, cnt = np.zeros((B, H), np.int32), np.zeros((B, H), np.int32)
        ids[0] = ID_X
        ids[1] = 50 + np.arange(H)
        cnt[1] = rng.integers(0, 3, H)
        if H >= 6:
            ids[1, [0, 1, 2, 5]] = ID_X
            cnt[1, [0, 1, 2, 5]] = (0, 0, 2 + bump, 3 + bump)
        else:
            ids[1, 0], cnt[1, 0] = ID_X, 2 + bump
        ids[2] = rng.choice([ID_X, ID_Y, 40, 41, 42, 43, 44, 45], H)
        cnt[2] = rng.choice([0, 1, 2, 5], H)
        ids[3] = ID_Y
        cnt[3, H - 1] = 4 + bump
        out[ids_name], out[cnt_name] = ids.reshape(-1), cnt.reshape(-1)
    out["n_valid"] = np.asarray(MATCH_N_VALID, np.int32)
    return out
