"""tests/sideops_ref.py on the CPU: the float64 restatements against float64 torch autograd (the feature rows as
F.embedding(padding_idx=0) -> cat -> mask / (1 - p); the matching through oracle/segpool_oracle.hierarchical_scores on a tree
hierarchical_interest built), hier_match_ref / hier_query_ref on lists small enough to read, and the proof that FEATURE_CASES
holds every path of launch_features_bwd (csrc/wide.hip)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import segpool_oracle as orc
from tests import sideops_ref as sr

TOL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max(initial=0.0)
    assert err <= TOL * max(1.0, np.abs(want).max(initial=0.0)), (what, err)


def _feature_data(case, seed):
    n, dt, dc, n_cat, n_sub = case
    rng = np.random.default_rng(seed)
    categ, sub, cold_cat, cold_sub = sr.feature_ids(n, n_cat, n_sub, rng)
    Fw = 2 * dt + 2 * dc
    return dict(title=rng.standard_normal((n, dt)), abst=rng.standard_normal((n, dt)), cat_table=rng.standard_normal((n_cat, dc)),
                sub_table=rng.standard_normal((n_sub, dc)), categ=categ, sub=sub, dout=rng.standard_normal((n, Fw)),
                keep=(rng.random((n, Fw)) >= 0.2).astype(np.uint8), cold_cat=cold_cat, cold_sub=cold_sub)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("case", sr.FEATURE_CASES, ids=lambda c: "n%d_dt%d_dc%d_cat%d_sub%d" % c)
def test_feature_refs_are_float64_autograd(case, p):
    n, dt, dc, n_cat, n_sub = case
    v = _feature_data(case, 7)
    keep = v["keep"] if p else None
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(True)
    title, abst, ct, st = t(v["title"]), t(v["abst"]), t(v["cat_table"]), t(v["sub_table"])
    fold = lambda ids, rows: torch.from_numpy(np.where((ids < 0) | (ids >= rows), 0, ids))     # outside the table: row 0
    row = torch.cat([title, abst, F.embedding(fold(v["categ"], n_cat), ct, padding_idx=0),
                     F.embedding(fold(v["sub"], n_sub), st, padding_idx=0)], dim=1)
    if p:
        row = row * torch.from_numpy(v["keep"].astype(np.float64)) * (1.0 / (1.0 - float(np.float32(p))))
    (row * torch.from_numpy(v["dout"])).sum().backward()
    _close(sr.features_fwd_ref(v["title"], v["abst"], v["cat_table"], v["sub_table"], v["categ"], v["sub"], keep, p), row.detach(), "out")
    g = sr.features_bwd_ref(v["dout"], v["categ"], v["sub"], dt, dc, n_cat, n_sub, keep, p)
    _close(g["d_title"], title.grad, "d_title")
    _close(g["d_abst"], abst.grad, "d_abst")
    _close(g["d_cat"], ct.grad, "d_cat")
    _close(g["d_sub"], st.grad, "d_sub")
    # what the GPU test leans on: padding and cold rows take nothing, and m / S describe the sums
    for name, ids, cold, rows in (("cat", v["categ"], v["cold_cat"], n_cat), ("sub", v["sub"], v["cold_sub"], n_sub)):
        m, S, tot = g["m_" + name], g["S_" + name], g["d_" + name]
        assert (m[[0] + cold] == 0).all() and (tot[[0] + cold] == 0).all()
        assert np.array_equal(m[:, 0], np.bincount(ids[(ids >= 1) & (ids < rows)], minlength=rows))
        assert (np.abs(tot) <= S * (1 + 1e-12)).all() and (S[m[:, 0] == 0] == 0).all()


def test_feature_ids_hold_what_the_cases_promise():
    for case in sr.FEATURE_CASES:
        n, dt, dc, n_cat, n_sub = case
        categ, sub, cold_cat, cold_sub = sr.feature_ids(n, n_cat, n_sub, np.random.default_rng(3))
        hot = categ if n_cat >= 2 else sub
        for w in range((n + 127) // 128):
            assert (hot[128 * w:128 * (w + 1)] == 1).any(), (case, w)        # one row that every window names
        assert cold_cat or cold_sub, case
        for ids, rows in ((categ, n_cat), (sub, n_sub)):
            assert ids.min() >= -1 and ids.max() <= rows, case
            if n >= 5:
                assert {0, -1, rows} <= set(ids.tolist()), case                # padding, below and above the table


def _tree_inputs(rng, H, d, n_top, n_sub):
    lv = lambda: (torch.from_numpy(rng.standard_normal((5, d))), torch.from_numpy(rng.standard_normal(5)),
                  torch.from_numpy(rng.standard_normal(5)))
    return {"sub": lv(), "top": lv(), "user": lv(), "E_sub": torch.from_numpy(rng.standard_normal((n_sub, d))),
            "E_top": torch.from_numpy(rng.standard_normal((n_top, d)))}


@pytest.mark.parametrize("lambdas", [(0.7, 0.15), (0.0, 0.0)])
def test_hier_score_refs_are_autograd_through_the_oracle(lambdas):
    """Three users with interest trees from hierarchical_interest; the tree's vectors become leaves laid out in slots
    b * H + position (sub-topics and topics in ascending id order), the candidates name present and absent ids.  The oracle is
    given the lambdas as the fp32 values the library receives, which is what the reference computes with."""
    ls, lt = (float(np.float32(v)) for v in lambdas)
    rng = np.random.default_rng(9)
    B, C, H, d = 3, 6, 7, 10
    topic = rng.integers(1, 4, (B, H))
    subtopic = topic * 10 + rng.integers(0, 2, (B, H))
    valid = rng.random((B, H)) < 0.8
    valid[:, 0] = True
    p = _tree_inputs(rng, H, d, 4, 40)
    cand = rng.standard_normal((B, C, d))
    cand_topic = rng.integers(1, 6, (B, C))
    cand_sub = cand_topic * 10 + rng.integers(0, 2, (B, C))
    mask = (rng.random((B, C)) < 0.8).astype(np.uint8)
    dscores = rng.standard_normal((B, C))
    u1, u2, ug = np.zeros((B * H, d)), np.zeros((B * H, d)), np.zeros((B, d))
    want_du1, want_du2 = np.zeros((B * H, d)), np.zeros((B * H, d))
    ss, ts = np.full((B, C), -1), np.full((B, C), -1)
    sf, tf = np.zeros((B, C)), np.zeros((B, C))
    cand_t = torch.from_numpy(cand).requires_grad_(True)
    rows, per_user = [], []
    for b in range(B):
        tree = orc.hierarchical_interest(torch.from_numpy(rng.standard_normal((H, d))), valid[b], topic[b], subtopic[b], p)
        leaf = lambda v: v.detach().clone().requires_grad_(True)
        t_sub, t_top, t_user = {k: leaf(v) for k, v in tree[0].items()}, {k: leaf(v) for k, v in tree[2].items()}, leaf(tree[4])
        per_user.append((t_sub, t_top, t_user))
        for g, k in enumerate(sorted(t_sub)):
            u1[b * H + g] = t_sub[k].detach().numpy()
        for g, k in enumerate(sorted(t_top)):
            u2[b * H + g] = t_top[k].detach().numpy()
        ug[b] = t_user.detach().numpy()
        for c in range(C):
            s_id, t_id = int(cand_sub[b, c]), int(cand_topic[b, c])
            if s_id in t_sub:
                ss[b, c], sf[b, c] = b * H + sorted(t_sub).index(s_id), tree[1][s_id] / tree[5]
            if t_id in t_top:
                ts[b, c], tf[b, c] = b * H + sorted(t_top).index(t_id), tree[3][t_id] / tree[5]
        rows.append(orc.hierarchical_scores(cand_t[b], cand_topic[b], cand_sub[b], (t_sub, tree[1], t_top, tree[3], t_user, tree[5]), ls, lt))
    assert (ss >= 0).any() and (ss < 0).any() and (ts >= 0).any() and (ts < 0).any() and (mask == 0).any()
    want = torch.stack(rows).masked_fill(torch.from_numpy(mask) == 0, -1e9)
    # a masked score is the constant -1e9: masked_fill passes it no gradient, whatever dscores holds there
    (want * torch.from_numpy(dscores)).sum().backward()
    for b, (t_sub, t_top, t_user) in enumerate(per_user):
        for g, k in enumerate(sorted(t_sub)):
            want_du1[b * H + g] = 0 if t_sub[k].grad is None else t_sub[k].grad.numpy()
        for g, k in enumerate(sorted(t_top)):
            want_du2[b * H + g] = 0 if t_top[k].grad is None else t_top[k].grad.numpy()
    scores, S = sr.hier_score_ref(cand, u1, u2, ug, ss, sf, ts, tf, mask, ls, lt)
    _close(scores[mask != 0], want.detach().numpy()[mask != 0], "scores")
    assert (scores[mask == 0] == -1e9).all()
    g = sr.hier_score_bwd_ref(cand, u1, u2, ug, ss, sf, ts, tf, mask, ls, lt, dscores)
    _close(g["dcand"], cand_t.grad, "dcand")
    _close(g["du1"], want_du1, "du1")
    _close(g["du2"], want_du2, "du2")
    _close(g["dug"], np.stack([t_user.grad.numpy() for _, _, t_user in per_user]), "dug")
    assert (g["dcand"][mask == 0] == 0).all()
    for name in ("du1", "du2"):
        assert (np.abs(g[name]) <= g["S_" + name] * (1 + 1e-12)).all() and (g["S_" + name][g["m_" + name][:, 0] == 0] == 0).all()


def test_feature_cases_reach_every_path_of_the_launcher():
    """features_bwd_plan restates launch_features_bwd; the case table must hold every branch it can take."""
    plans = {c: sr.features_bwd_plan(*c) for c in sr.FEATURE_CASES}
    chunks = {c: sr._features_bwd_chunks(*c) for c in sr.FEATURE_CASES}
    chunk_of = lambda c: ((c[0] + chunks[c][2] - 1) // chunks[c][2] + 127) // 128 * 128
    assert any(p == ("single", 1) for p in plans.values())
    assert any(p[0] == "single" and p[1] >= 2 for p in plans.values())
    assert any(p[0] == "chunked" and p[2] == chunk_of(c) for c, p in plans.items())              # full last chunk
    assert any(p[0] == "chunked" and p[2] < chunk_of(c) for c, p in plans.items())               # partial last chunk
    assert any(p[0] == "chunked" and p[2] == 1 for p in plans.values())                          # ... of a single slot
    assert any(p[0] == "chunked" and after < wanted for (c, p), (_, wanted, after) in zip(plans.items(), chunks.values()))
    assert any(p[0] == "single" and after < wanted for (c, p), (_, wanted, after) in zip(plans.items(), chunks.values()))
    assert any(0 < 8192 // rows < 64 and plans[c][0] == "chunked" for c, (rows, _, _) in chunks.items())
    assert any(8192 // rows == 0 and plans[c] == ("single", 2) for c, (rows, _, _) in chunks.items())
    assert any(c[2] > 128 and plans[c][0] == "chunked" for c in plans) and any(c[2] > 128 and plans[c][0] == "single" for c in plans)
    assert any(c[0] > 16384 for c in plans) and any(c[3] == 1 for c in plans)
    # the rows the issue's table spells out
    assert plans[(129, 8, 8, 3, 4)] == ("chunked", 2, 1) and plans[(256, 8, 8, 3, 4)] == ("chunked", 2, 128)
    assert plans[(257, 8, 8, 3, 4)] == ("chunked", 3, 1) and plans[(300, 8, 8, 3, 4)] == ("chunked", 3, 44)
    assert plans[(129, 4, 64, 5, 9)] == ("single", 2) and chunks[(129, 4, 64, 5, 9)][1:] == (2, 1)
    assert plans[(600, 4, 48, 5, 9)] == ("chunked", 3, 88) and chunks[(600, 4, 48, 5, 9)][1:] == (5, 4)
    assert chunks[(5200, 8, 4, 60, 142)] == (200, 40, 40)
    # every chunked case keeps its partial sums inside d_title_vec
    for c, p in plans.items():
        if p[0] == "chunked":
            assert p[1] * chunks[c][0] * c[2] <= c[0] * c[1], c
    # one batch, two paths
    n, dc, n_cat, n_sub = sr.TWO_PATH_CASE
    assert sr.features_bwd_plan(n, sr.TWO_PATH_D_TEXT[0], dc, n_cat, n_sub)[0] == "chunked"
    assert sr.features_bwd_plan(n, sr.TWO_PATH_D_TEXT[1], dc, n_cat, n_sub) == ("single", 3)


@pytest.mark.parametrize("H", [1, 64])
def test_hier_match_ref_on_lists_small_enough_to_read(H):
    v = sr.match_lists(H, np.random.default_rng(2))
    B, C = 4, 3
    ids = np.tile(np.asarray([sr.ID_X, sr.ID_Y, sr.ID_Z]), (B, 1))
    ss, sf, ts, tf = sr.hier_match_ref(B, C, H, ids, ids, v["l1_sub"], v["l1_cnt"], v["l2_top"], v["l2_cnt"], v["n_valid"])
    assert sf.dtype == np.float32 and ss.dtype == np.int32
    assert (ss[0] == -1).all() and (ts[0] == -1).all() and (sf[0] == 0).all() and (tf[0] == 0).all()       # n_valid = 0
    first = 2 if H == 64 else 0
    assert ss[1, 0] == H + first and ts[1, 0] == H + first                           # count-0 slots below it do not match
    assert sf[1, 0] == np.float32(2) * (np.float32(1) / np.float32(7)) and tf[1, 0] == np.float32(3) * (np.float32(1) / np.float32(7))
    assert ss[3, 1] == 4 * H - 1 and tf[3, 1] == np.float32(5) * (np.float32(1) / np.float32(49))
    assert (ss[:, 2] == -1).all() and (ts[:, 2] == -1).all()                          # Z is nowhere
    for b in range(B):                                                               # every match is occupied and the lowest
        for c in range(C):
            for slot, idl, cnt in ((ss, v["l1_sub"], v["l1_cnt"]), (ts, v["l2_top"], v["l2_cnt"])):
                hits = [b * H + g for g in range(H) if cnt[b * H + g] > 0 and idl[b * H + g] == ids[b, c]]
                assert slot[b, c] == (hits[0] if hits else -1)


def test_hier_query_ref_is_the_user_side_of_the_score():
    """<n, query[b, g]> == hier_score_ref for a candidate n with group g's ids, in float64."""
    H, d = 64, 12
    rng = np.random.default_rng(4)
    v = sr.match_lists(H, rng)
    B, gt, gs = 4, [sr.ID_X, sr.ID_Y, sr.ID_Z, sr.ID_X, sr.ID_Z], [sr.ID_X, sr.ID_Y, sr.ID_Z, sr.ID_Z, sr.ID_Y]
    G = len(gt)
    u1, u2, ug = rng.standard_normal((B * H, d)), rng.standard_normal((B * H, d)), rng.standard_normal((B, d))
    lists = (v["l1_sub"], v["l1_cnt"], v["l2_top"], v["l2_cnt"], v["n_valid"])
    q, Sq = sr.hier_query_ref(B, H, gt, gs, *lists, u1, u2, ug, 0.7, 0.15)
    cand = rng.standard_normal((B, G, d))
    ss, sf, ts, tf = sr.hier_match_ref(B, G, H, np.tile(gt, (B, 1)), np.tile(gs, (B, 1)), *lists)
    scores, S = sr.hier_score_ref(cand, u1, u2, ug, ss, sf, ts, tf, None, 0.7, 0.15)
    _close((q * cand).sum(-1), scores, "query . n")
    _close((Sq * np.abs(cand)).sum(-1), S, "S")
    assert (ss >= 0).any() and (ss < 0).any() and ((ss >= 0) != (ts >= 0)).any()


def test_hier_score_batches_hold_what_they_promise():
    """The hand-built batches of tests/test_hip_sideops.py."""
    rng = np.random.default_rng(1)
    for B, Cn in [(B, Cn) for B in (1, 3, 4, 5, 9) for Cn in (1, 5, 7)]:
        v = sr.hier_score_batch(B, Cn, 8, rng)
        ss, ts, H = v["sub_slot"], v["top_slot"], v["H"]
        users = np.arange(B)[:, None]
        assert (((ss == -1) | (ss // H == users)) & ((ts == -1) | (ts // H == users))).all()      # a user's own rows only
        if Cn >= 3:
            assert len(set(ss[B - 1, Cn - 3:].tolist())) == 1 and ss[B - 1, Cn - 1] >= 0 and ts[B - 1, Cn - 3] == ts[B - 1, Cn - 2] >= 0
        if B * Cn - (3 if Cn >= 3 else 0) >= 5:
            assert set(v["kinds"]) == {"none", "sub_only", "top_only", "masked", "zero_share"}
            b, c = v["kinds"]["masked"]
            assert v["mask"][b, c] == 0 and v["dscores"][b, c] != 0 and np.isfinite(v["dscores"][b, c])
            b, c = v["kinds"]["zero_share"]
            assert v["sub_frac"][b, c] == 0 and ss[b, c] >= 0
            b, c = v["kinds"]["none"]
            assert ss[b, c] == ts[b, c] == -1 and v["sub_frac"][b, c] != 0
