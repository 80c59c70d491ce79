"""nrms_topk_grouped_dot and nrms_hier_query on the GPU (include/nrms_hip.h): exact against a host lexsort on tie-heavy data
over awkward partitions, bit-identity with nrms_topk_dot, invariance, and the retrieval of HieRec and nrms_naml built on them
(Model.encode_catalogue / recommend, train_eval.recommend)."""
import re

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
_ENG = []


def _engine():
    if not _ENG:
        _ENG.append(NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), DEV))
    return _ENG[0]


def _dev(x, dt):
    return torch.as_tensor(x).to(DEV, dtype=dt).contiguous()


def _grouped(query, items, item_ids, group_ptr, k, exclude=None, eng=None):
    ex = None if exclude is None else _dev(exclude, torch.int64)
    s, i = (eng or _engine()).top_k_grouped(_dev(query, torch.float32), _dev(items, torch.float32), _dev(item_ids, torch.int32),
                                            _dev(group_ptr, torch.int64), k, ex)
    return s.cpu().numpy(), i.cpu().numpy()


def _host(query, items, item_ids, group_ptr, k, exclude=None):
    """The contract on the host: float64 scores (exact for integer data), eligible = id not excluded and score not NaN,
    np.lexsort((ids, -scores)), then id -1 / score -inf."""
    B, G, _ = query.shape
    grp = np.repeat(np.arange(G), np.diff(group_ptr))
    s = np.einsum("bnd,nd->bn", query.astype(np.float64)[:, grp], items.astype(np.float64))
    out_s = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int64)
    for b in range(B):
        ok = ~np.isnan(s[b])
        if exclude is not None:
            ok &= ~np.isin(item_ids, exclude[b])
        rows = np.nonzero(ok)[0]
        top = rows[np.lexsort((item_ids[rows], -s[b, rows]))][:k]
        out_i[b, :len(top)] = item_ids[top]
        out_s[b, :len(top)] = s[b, top].astype(np.float32) + np.float32(0.0)
    return out_s, out_i


def _assert_exact(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0].view(np.int32), want[0].view(np.int32))


def _partition(rng, N):
    """Group sizes with empty groups, 1-item groups and groups shorter than / straddling 32- and 64-row tiles."""
    sizes = [0, 1, 0, 31, 32, 33, 1, 63, 64, 65, 0, 2, 97, 5]
    while sum(sizes) < N:
        sizes.append(int(rng.choice([0, 1, 3, 17, 40, 70, 129, 300])))
    sizes = np.array(sizes)
    over = sizes.sum() - N
    for j in range(len(sizes) - 1, -1, -1):              # trim to N
        cut = min(over, sizes[j])
        sizes[j] -= cut
        over -= cut
    rng.shuffle(sizes)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _int_case(B, N, d, seed, n_ex=60):
    rng = np.random.default_rng(seed)
    gp = _partition(rng, N)
    G = len(gp) - 1
    query = rng.integers(-3, 4, size=(B, G, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    items[rng.choice(N, size=max(1, N // 97), replace=False)] = np.nan
    ids = rng.permutation(4 * N)[:N].astype(np.int32)                         # shuffled, sparse ids
    ex = ids[rng.integers(0, N, size=(B, n_ex))].astype(np.int64)
    ex[:, 0], ex[:, 1], ex[:, 2], ex[:, 3] = -1, 4 * N + 7, 1 << 40, ex[:, 4]  # out of range, huge, a duplicate
    return query, items, ids, gp, ex


@pytest.mark.parametrize("k", [1, 7, 64, 65, 192, 193, 256])
def test_exact_with_ties_nan_and_awkward_groups(k):
    case = _int_case(37, 3001, 33, seed=k)
    _assert_exact(_grouped(*case[:4], k, case[4]), _host(*case[:4], k, case[4]))


@pytest.mark.parametrize("d", [1, 3, 4, 31, 33, 300, 800])
def test_exact_at_every_width(d):
    query, items, ids, gp, ex = _int_case(35, 2003, d, seed=100 + d, n_ex=70 if d % 2 else 50)
    _assert_exact(_grouped(query, items, ids, gp, 100, ex), _host(query, items, ids, gp, 100, ex))
    _assert_exact(_grouped(query, items, ids, gp, 7), _host(query, items, ids, gp, 7))


def _bench_data(B=512, N=130000, d=300, n_ex=50, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    user = torch.randn(B, d, device=DEV, generator=g)
    items = torch.randn(N, d, device=DEV, generator=g)
    ex = torch.randint(0, N, (B, n_ex), device=DEV, generator=g)
    return user, items, ex


def _skewed_groups(N, G, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.zipf(1.6, size=G).astype(np.float64)
    sizes = np.floor(w / w.sum() * N).astype(np.int64)
    sizes[np.argmax(sizes)] += N - sizes.sum()
    return torch.as_tensor(np.concatenate([[0], np.cumsum(sizes)]), device=DEV)


def test_one_group_is_bitwise_nrms_topk_dot():
    user, items, ex = _bench_data()
    eng = _engine()
    N = items.shape[0]
    for k in (10, 100):
        s0, i0 = eng.top_k(user, items, k, ex)
        s1, i1 = eng.top_k_grouped(user.unsqueeze(1).contiguous(), items, torch.arange(N, device=DEV, dtype=torch.int32),
                                   torch.tensor([0, N], device=DEV), k, ex)
        assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))


def test_bench_size_equals_per_group_topk_dot_merged():
    B, N, d, G, k = 512, 130000, 300, 294, 100
    user, items, ex = _bench_data(B, N, d)
    g = torch.Generator(device=DEV).manual_seed(7)
    query = torch.randn(B, G, d, device=DEV, generator=g)
    gp = _skewed_groups(N, G)
    ids = torch.randperm(N, device=DEV, generator=g).to(torch.int32)
    eng = _engine()
    s, i = eng.top_k_grouped(query, items, ids, gp, k, ex)
    gpl = gp.tolist()
    all_s, all_i = [], []
    for gi in range(G):
        lo, hi = gpl[gi], gpl[gi + 1]
        if hi == lo:
            continue
        # nrms_topk_dot on the group's rows, exclude mapped to row positions inside the group
        pos = torch.full((N,), -1, dtype=torch.int64, device=DEV)
        pos[ids[lo:hi].long()] = torch.arange(hi - lo, device=DEV)
        gs, gidx = eng.top_k(query[:, gi].contiguous(), items[lo:hi].contiguous(), k, pos[ex].contiguous())
        all_s.append(gs)
        all_i.append(torch.where(gidx >= 0, ids[lo:hi].long()[gidx.clamp(min=0)], gidx))
    cs, ci = torch.cat(all_s, 1).cpu().numpy(), torch.cat(all_i, 1).cpu().numpy()
    want_s, want_i = np.empty((B, k), np.float32), np.empty((B, k), np.int64)
    for b in range(B):
        live = ci[b] >= 0
        o = np.lexsort((ci[b][live], -cs[b][live].astype(np.float64)))[:k]
        want_s[b], want_i[b] = cs[b][live][o], ci[b][live][o]
    _assert_exact((s.cpu().numpy(), i.cpu().numpy()), (want_s, want_i))


def test_invariance_and_padding():
    B, N, d, G = 300, 20000, 64, 40
    user, items, ex = _bench_data(B, N, d, seed=1)
    g = torch.Generator(device=DEV).manual_seed(3)
    query = torch.randn(B, G, d, device=DEV, generator=g)
    gp = _skewed_groups(N, G, seed=1)
    ids = torch.arange(N, device=DEV, dtype=torch.int32)
    eng = _engine()
    s, i = eng.top_k_grouped(query, items, ids, gp, 100, ex)
    same = lambda a, b: torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert same((s, i), eng.top_k_grouped(query, items, ids, gp, 100, ex))
    a = eng.top_k_grouped(query[:123].contiguous(), items, ids, gp, 100, ex[:123].contiguous())
    b = eng.top_k_grouped(query[123:].contiguous(), items, ids, gp, 100, ex[123:].contiguous())
    assert same((s, i), (torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]])))
    s50, i50 = eng.top_k_grouped(query, items, ids, gp, 50, ex)
    assert same((s[:, :50], i[:, :50]), (s50, i50))
    # a permuted, regrouped catalogue: the groups in reverse order, rows shuffled inside each group
    gpl = gp.tolist()
    rows, gp2, order = [], [0], list(range(G))[::-1]
    for gi in order:
        lo, hi = gpl[gi], gpl[gi + 1]
        rows.append(lo + torch.randperm(hi - lo, device=DEV, generator=g))
        gp2.append(gp2[-1] + hi - lo)
    rows = torch.cat(rows)
    q2 = query[:, order].contiguous()
    assert same((s, i), eng.top_k_grouped(q2, items[rows].contiguous(), ids[rows].contiguous(), torch.tensor(gp2, device=DEV),
                                          100, ex))
    # a forced small chunk cap: users in many chunks
    old = eng.retrieval_chunk_bytes
    try:
        eng.retrieval_chunk_bytes = 40 * G * d * 4
        assert eng.grouped_chunk_users(B, N, d, 100, G) < B
        assert same((s, i), eng.top_k_grouped(query, items, ids, gp, 100, ex))
    finally:
        eng.retrieval_chunk_bytes = old
    # k above the eligible count, N = 0, B = 0
    few = torch.tensor([0, 2, 2, 5], device=DEV)
    q3 = query[:4, :3].contiguous()
    s3, i3 = eng.top_k_grouped(q3, items[:5].contiguous(), ids[:5].contiguous(), few, 10, ids[:4, None].long().contiguous())
    assert ((i3[:, :4] >= 0).all() and (i3[:, 4:] == -1).all() and (s3[:, 4:] == -float("inf")).all())
    assert not (i3 == torch.arange(4, device=DEV)[:, None]).any()
    s4, i4 = eng.top_k_grouped(q3, items[:0].contiguous(), ids[:0].contiguous(), torch.zeros(4, dtype=torch.int64, device=DEV), 5)
    assert (i4 == -1).all() and (s4 == -float("inf")).all()
    s5, i5 = eng.top_k_grouped(query[:0].contiguous(), items, ids, gp, 5)
    assert s5.shape == (0, 5) and i5.shape == (0, 5)
    with pytest.raises(_lib.NrmsError, match="k <= 256"):
        eng.top_k_grouped(query, items, ids, gp, 257)


# ---- models ---------------------------------------------------------------------------------------------------------------
def _cfg(kind):
    from pytorch_news_recommender_amd.config import Config
    cfg = Config(kind)
    cfg.__nrms__()
    cfg.n_words, cfg.n_words_title, cfg.n_words_abst, cfg.history_len, cfg.sample_size, cfg.max_candidate_size = 600, 12, 16, 10, 4, 24
    cfg.word_embed_size, cfg.num_attention_heads, cfg.title_heads_num, cfg.query_vector_dim = 60, 6, 3, 32
    cfg.category_nums, cfg.subcategory_nums = 8, 40
    cfg.batch_size, cfg.dropout = 32, 0.2
    return cfg


def _model(kind, tmp_path):
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    torch.manual_seed(0)
    cfg = _cfg(kind)
    corpus = SyntheticMind(cfg, n_news=300, n_topics=4, seed=1)
    table = corpus.embedding_table(cfg.word_embed_size)
    if kind == "hierec":
        from pytorch_news_recommender_amd.model.hierec_hip import Model
        model = Model(cfg, pretrained_word_embedding=table).to("cuda")
    else:
        from pytorch_news_recommender_amd.model.nrms_naml_hip import Model
        cfg.user_heads_num, cfg.cate_embed_size, cfg.query_vector_dim_large = 4, 20, 40
        cfg.news_feature_size = 2 * cfg.word_embed_size + 2 * cfg.cate_embed_size
        model = Model(cfg, pretrained_word_embedding=table).to("cuda")
    samples, _ = corpus.eval_samples(100, max_shown=20)
    feed = DeviceFeed(cfg, samples, type=1, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict,
                      batch_size=cfg.batch_size, device=DEV)
    return cfg, model, feed


def _forward_batch(feed, info, batch, ids):
    k = ids.shape[1]
    take = lambda t: t.index_select(0, ids.view(-1)).view(ids.shape[0], k, *t.shape[1:])
    fb = {key: batch[key] for key in ("browsed_ids", "browsed_titles", "browsed_absts", "browsed_categ_ids",
                                      "browsed_subcateg_ids", "browsed_mask")}
    fb.update(candidate_ids=ids, candidate_titles=take(feed.titles), candidate_absts=take(feed.absts),
              candidate_categ_ids=take(info["categ"]), candidate_subcateg_ids=take(info["subcateg"]),
              candidate_mask=torch.ones_like(ids, dtype=torch.uint8))
    return fb


@pytest.mark.parametrize("kind", ["hierec", "nrms_naml"])
def test_model_recommend_matches_forward(kind, tmp_path):
    cfg, model, feed = _model(kind, tmp_path)
    info = feed.news_info()
    model.train()                                   # recommend / encode_catalogue ignore the module's mode
    cat = model.encode_catalogue(feed.titles, **info)
    k = 20
    for batch in feed:
        ids, scores = model.recommend(batch, k, cat)
        hist = batch["browsed_ids"]
        assert ids.shape == scores.shape == (hist.shape[0], k) and ids.dtype == torch.int64
        assert (ids > 0).all()
        assert not (ids.unsqueeze(2) == hist.unsqueeze(1)).any()
        model.eval()
        with torch.no_grad():
            fwd = model(_forward_batch(feed, info, batch, ids))
        model.train()
        assert ((fwd - scores).abs() <= 1e-5 * scores.abs().clamp(min=1)).all(), (fwd - scores).abs().max().item()
        ds, di = scores[:, 1:] - scores[:, :-1], ids[:, 1:] - ids[:, :-1]
        assert ((ds < 0) | ((ds == 0) & (di > 0))).all()
    model.check_recommend_ids()
    model.engine.check_ids()
    bad = {"browsed_ids": torch.tensor([[1, 2, feed.titles.shape[0] + 5]], device=DEV)}
    model.recommend(bad, k, cat)
    with pytest.raises(_lib.NrmsError, match="outside the catalogue"):
        model.check_recommend_ids()


def test_hierec_user_without_clicks_gets_the_smallest_ids(tmp_path):
    cfg, model, feed = _model("hierec", tmp_path)
    cat = model.encode_catalogue(feed.titles, **feed.news_info())
    ids, scores = model.recommend({"browsed_ids": torch.zeros(3, cfg.history_len, dtype=torch.int64, device=DEV)}, 10, cat)
    assert (ids == torch.arange(1, 11, device=DEV)).all()
    assert (scores.view(torch.int32) == 0).all()


def test_hier_query_matches_hier_match_and_float64(tmp_path):
    cfg, model, feed = _model("hierec", tmp_path)
    eng = model.engine
    cat = model.encode_catalogue(feed.titles, **feed.news_info())
    batch = next(iter(feed))
    br = batch["browsed_ids"]
    B, H = br.shape
    G, d = cat.group_topic.shape[0], cfg.word_embed_size
    slots = br.reshape(-1)
    t, u1, u2, ug, _ = eng._interests(model._flat, cat.vectors.index_select(0, slots), (br != 0).to(torch.uint8),
                                      cat.categ.index_select(0, slots), cat.subcateg.index_select(0, slots), B, H, "_test")
    q = torch.empty(B, G, d, device=DEV)
    args = [_lib.ptr(t[x]) for x in ("l1_sub", "l1_cnt", "l2_top", "l2_cnt", "n_valid")]
    _lib.check(eng.lib.nrms_hier_query(B, H, G, d, _lib.ptr(cat.group_topic), _lib.ptr(cat.group_sub), *args, _lib.ptr(u1),
                                       _lib.ptr(u2), _lib.ptr(ug), eng.lambda_sub, eng.lambda_top, _lib.ptr(q), _stream()),
               "nrms_hier_query")
    # the slots of nrms_hier_match on every (user, group) as a candidate
    ctop, csub = cat.group_topic.repeat(B).contiguous(), cat.group_sub.repeat(B).contiguous()
    ss, ts = torch.empty(B * G, dtype=torch.int32, device=DEV), torch.empty(B * G, dtype=torch.int32, device=DEV)
    sf, tf = torch.empty(B * G, device=DEV), torch.empty(B * G, device=DEV)
    _lib.check(eng.lib.nrms_hier_match(B, G, H, _lib.ptr(ctop), _lib.ptr(csub), *args, _lib.ptr(ss), _lib.ptr(sf), _lib.ptr(ts),
                                       _lib.ptr(tf), _stream()), "nrms_hier_match")
    assert (ss >= 0).any() and (ts >= 0).any() and (ss < 0).any()
    ls, lt = eng.lambda_sub, eng.lambda_top
    U1, U2, UG = u1.double(), u2.double(), ug.double()
    pick = lambda U, s: torch.where((s >= 0)[:, None], U[s.clamp(min=0).long()], torch.zeros_like(U[:1]))
    want = (ls * sf.double()[:, None] * pick(U1, ss) + lt * tf.double()[:, None] * pick(U2, ts)
            + (1 - ls - lt) * UG.repeat_interleave(G, 0))
    got = q.view(B * G, d).double()
    scale = (ls * sf.double()[:, None] * pick(U1, ss)).abs() + (lt * tf.double()[:, None] * pick(U2, ts)).abs() \
        + ((1 - ls - lt) * UG.repeat_interleave(G, 0)).abs()
    assert ((got - want).abs() <= 1e-6 * scale + 1e-30).all()


@pytest.mark.parametrize("kind", ["hierec", "nrms_naml"])
def test_train_eval_recommend_writes_one_line_per_impression(kind, tmp_path):
    cfg, model, feed = _model(kind, tmp_path)
    out = train_eval.recommend(cfg, model, feed, feed.titles, 10, out_file=str(tmp_path / "rec.txt"), news_info=feed.news_info())
    lines = open(out).read().splitlines()
    hist = feed.packed["hist"].cpu().numpy()
    assert len(lines) == feed.n
    for i, ln in enumerate(lines):
        m = re.fullmatch(r"(\d+) \[(\d+(?:,\d+)*)\]", ln)
        assert m and int(m.group(1)) == i + 1, ln
        ids = [int(v) for v in m.group(2).split(",")]
        assert len(ids) == 10 == len(set(ids)) and 0 not in ids and not set(ids) & set(hist[i].tolist())
