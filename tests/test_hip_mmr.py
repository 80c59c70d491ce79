"""nrms_mmr_rerank on the GPU (greedy MMR re-ranking of a shortlist, include/nrms_hip.h) against tests/mmr_ref.py: exact on
lattice data where every cosine, relevance and value is exact in fp32, greedy-consistent within a derived bound on real-valued
data, lambda = 1 through Model.recommend, invariance and determinism under guard bands and poisoned workspaces, the effect on a
clustered catalogue, and the layers built on it (NRMSEngine.mmr_rerank, Model.recommend, train_eval.recommend, run_v0)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, synth, train_eval
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream

from tests import mmr_ref
from tests.guarded import POISONS, Pool, assert_same_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENG = []
U = 2.0 ** -24                      # fp32 unit roundoff


def _engine():
    if not _ENG:
        _ENG.append(NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), DEV))
    return _ENG[0]


def _dev(x, dt):
    return torch.as_tensor(x).to(DEV, dtype=dt).contiguous()


def _rerank(items, ids, scores, k, lam):
    out = _engine().mmr_rerank(_dev(items, torch.float32), _dev(ids, torch.int64), _dev(scores, torch.float32), k, lam,
                               return_value=True, return_ild=True)
    return tuple(t.cpu().numpy() for t in out)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- 1: exact on lattice data ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 31, 32, 33, 64, 65, 255, 256])
def test_exact_on_lattice_data(M):
    """Every dot product, norm, cosine, relevance and value of mmr_ref.lattice_case is exact in fp32 (checked first: the float32
    and the float64 evaluation of the reference agree bit for bit), so ids, score bits and value bits must equal the
    reference's, ties included; the ILD differs from float64 by its one division and one subtraction (values below 2)."""
    B = 37
    for d in (1, 3, 31, 64, 301):
        items, ids, scores = mmr_ref.lattice_case(B, M, d)
        for k in sorted({1, min(7, M), M}):
            for lam in (0.0, 0.25, 0.5, 1.0):
                want = mmr_ref.mmr_batch(items, ids, scores, lam, k)
                if d in (3, 301) and k == min(7, M):          # the generator's promise, where it is cheap to check
                    w32 = mmr_ref.mmr_batch(items, ids, scores, lam, k, np.float32)
                    assert np.array_equal(w32["ids"], want["ids"]) and np.array_equal(w32["value"].astype(np.float64), want["value"])
                g_ids, g_scores, g_value, g_ild = _rerank(items, ids, scores, k, lam)
                what = "M=%d d=%d k=%d lambda=%g" % (M, d, k, lam)
                assert np.array_equal(g_ids, want["ids"]), what
                assert np.array_equal(_bits(g_scores), _bits(want["scores"])), what
                assert np.array_equal(_bits(g_value), _bits(want["value"].astype(np.float32))), what
                assert np.array_equal(np.isnan(g_ild), np.isnan(want["ild"])), what
                ok = ~np.isnan(want["ild"])
                assert (np.abs(g_ild[ok] - want["ild"][ok]) <= 4 * U).all(), what


# ---- 2: greedy consistency on real-valued data ----------------------------------------------------------------------------
def _gauss_case(B, N, d, M, seed):
    rng = np.random.default_rng(seed)
    items = rng.standard_normal((N, d)).astype(np.float32)
    ids = np.stack([rng.choice(N, size=M, replace=False) for _ in range(B)]).astype(np.int64)
    scores = rng.standard_normal((B, M)).astype(np.float32)
    ids[1, 5], ids[2, 200:] = ids[1, 9], -1                    # a duplicate; a tail
    scores[2, 200:] = -np.inf
    scores[3, 17], ids[3, 40], ids[3, 41] = np.nan, N, -5      # broken entries inside a row
    return items, ids, scores


@pytest.mark.parametrize("d", [60, 300])
@pytest.mark.parametrize("lam", [0.3, 0.7])
def test_greedy_consistency_on_gaussian_data(d, lam):
    """tol, from d and the fp32 unit roundoff u = 2^-24 (first order): a dot product of d terms is within d u |x_i| |x_j| of
    exact (each of the d products and d sums rounds once, Cauchy-Schwarz for the magnitudes), each squared norm likewise within
    d u of itself, so r_i = 1 / sqrt(.) within (d / 2 + 2) u and the cosine dot * (r_i * r_j), |cos| <= 1, within
    (d + 2 (d / 2 + 2) + 2) u = (2 d + 6) u.  rel takes three roundings of numbers in [0, 1] (3 u), lambda * rel, 1 - lambda, its
    product with maxsim and the final subtraction of numbers below 2 at most 5 u more: |v_fp32 - v_float64| <= (2 d + 14) u.
    tol = (2 d + 16) 2^-23 is that with a factor 2 for the higher-order terms.  A greedy step compares two such values, so the
    entry picked may trail the float64 best by 2 tol at most.  The ILD is a mean of cosines, each within (2 d + 6) u, plus a
    running fp32 sum whose error relative to the number of pairs stays below u times the largest mean |cosine| of a prefix."""
    B, N, M, k = 37, 3001, 256, 100
    tol = (2 * d + 16) * 2.0 ** -23
    items, ids, scores = _gauss_case(B, N, d, M, seed=d)
    g_ids, g_scores, g_value, g_ild = _rerank(items, ids, scores, k, lam)
    worst_gap = worst_val = worst_ild = 0.0
    for b in range(B):
        picks, problems = mmr_ref.picks_from_output(ids[b], scores[b], g_ids[b], g_scores[b], N)
        assert not problems, "row %d: %s" % (b, problems)
        assert len(set(picks)) == len(picks) == min(k, int(mmr_ref.valid_mask(ids[b], scores[b], N).sum()))
        gap, value, ild = mmr_ref.greedy_gap(items, ids[b], scores[b], lam, picks)
        worst_gap = max(worst_gap, float(gap.max()))
        worst_val = max(worst_val, float(np.abs(g_value[b, :len(picks)] - value).max()))
        worst_ild = max(worst_ild, abs(float(g_ild[b]) - float(ild)))
        assert (g_value[b, len(picks):] == -np.inf).all()
    print("d=%d lambda=%g: tol %.3e  worst greedy gap %.3e  |value - f64| %.3e  |ild - f64| %.3e" % (d, lam, tol, worst_gap, worst_val, worst_ild))
    assert worst_gap <= 2 * tol
    assert worst_val <= tol
    assert worst_ild <= tol


# ---- 3: lambda = 1 and the defaults through the models --------------------------------------------------------------------
def _tiny_cfg(kind):
    from pytorch_news_recommender_amd.config import Config
    cfg = Config(kind)
    cfg.__nrms__()
    cfg.n_words, cfg.n_words_title, cfg.n_words_abst, cfg.history_len, cfg.sample_size, cfg.max_candidate_size = 600, 12, 16, 10, 4, 24
    cfg.word_embed_size, cfg.num_attention_heads, cfg.title_heads_num, cfg.query_vector_dim = 60, 6, 3, 32
    cfg.category_nums, cfg.subcategory_nums = 8, 40
    cfg.batch_size, cfg.dropout = 32, 0.2
    return cfg


def _model(kind):
    """(cfg, model, batches, catalogue) at tiny dims, 300 news."""
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    torch.manual_seed(0)
    if kind == "nrms_bert":
        from pytorch_news_recommender_amd.config import Config
        from pytorch_news_recommender_amd.model.nrms_bert_hip import Model
        shape = synth.BertShape(n_news=300, bert_embed_size=64, user_heads_num=8, query_vector_dim_large=16, batch_size=32,
                                history_len=7, n_candidates=4)
        params = synth.make_params_bert(shape, seed=14)
        cfg = Config("nrms_bert")
        cfg.__nrms__()
        cfg.bert_embed_size, cfg.user_heads_num, cfg.query_vector_dim_large, cfg.dropout = 64, 8, 16, 0.0
        model = Model(cfg, pretrained_news_vectors=params["news_encoder.news_embedding.weight"])
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
        model = model.to("cuda")
        batch = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in synth.make_batch_bert(shape, seed=15).items()}
        return cfg, model, [batch], model.encode_catalogue(None)
    cfg = _tiny_cfg(kind)
    corpus = SyntheticMind(cfg, n_news=300, n_topics=4, seed=1)
    table = corpus.embedding_table(cfg.word_embed_size)
    if kind == "nrms_naml":
        from pytorch_news_recommender_amd.model.nrms_naml_hip import Model
        cfg.user_heads_num, cfg.cate_embed_size, cfg.query_vector_dim_large = 4, 20, 40
        cfg.news_feature_size = 2 * cfg.word_embed_size + 2 * cfg.cate_embed_size
    elif kind == "nrms_v1":
        from pytorch_news_recommender_amd.model.nrms_v1_hip import Model
    else:
        from pytorch_news_recommender_amd.model.nrms_hip import Model
    model = Model(cfg, pretrained_word_embedding=table).to("cuda")
    samples, _ = corpus.eval_samples(64, max_shown=20)
    feed = DeviceFeed(cfg, samples, type=1, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict,
                      batch_size=cfg.batch_size, device=DEV)
    cat = model.encode_catalogue(feed.titles, **feed.news_info()) if kind == "nrms_naml" else model.encode_catalogue(feed.titles)
    return cfg, model, list(feed), cat


@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_v1", "nrms_naml", "nrms_bert"])
def test_lambda_one_and_defaults_are_the_plain_list(kind):
    cfg, model, batches, cat = _model(kind)
    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                                 b.view(torch.int32) if b.dtype == torch.float32 else b)
    for batch in batches:
        for k in (1, 10, 20):
            ids, scores = model.recommend(batch, k, cat)
            user, c, ex = model._catalogue_query(batch, cat, True, "recommend")            # today's path, spelled out
            t_scores, t_ids = model.engine.top_k(user, c[1:], k, ex)
            assert same(ids, torch.where(t_ids >= 0, t_ids + 1, t_ids)) and same(scores, t_scores)
            d_ids, d_scores = model.recommend(batch, k, cat, True, diversity=None, shortlist=None, return_ild=False)
            assert same(ids, d_ids) and same(scores, d_scores)
            for shortlist in (None, k, 256):
                m_ids, m_scores, m_ild = model.recommend(batch, k, cat, diversity=1.0, shortlist=shortlist, return_ild=True)
                assert same(ids, m_ids) and same(scores, m_scores), (kind, k, shortlist)
                p_ids, p_scores, p_ild = model.recommend(batch, k, cat, return_ild=True)
                assert same(ids, p_ids) and same(scores, p_scores)
                assert torch.equal(p_ild.view(torch.int32), m_ild.view(torch.int32))       # the plain list's ILD is the same code
                assert bool(torch.isnan(p_ild).all()) == (k == 1)
    with pytest.raises(_lib.NrmsError, match="diversity"):
        model.recommend(batches[0], 5, cat, diversity=1.5)
    with pytest.raises(_lib.NrmsError, match="shortlist"):
        model.recommend(batches[0], 5, cat, diversity=0.5, shortlist=4)
    with pytest.raises(_lib.NrmsError, match="shortlist"):
        model.recommend(batches[0], 5, cat, diversity=0.5, shortlist=257)
    model.check_recommend_ids()


# ---- 4: invariance and determinism ----------------------------------------------------------------------------------------
def _invariance_case():
    rng = np.random.default_rng(77)
    B, N, d, M = 37, 501, 60, 100
    items = rng.standard_normal((N, d)).astype(np.float32)
    ids = rng.integers(0, N, size=(B, M)).astype(np.int64)       # duplicates happen
    scores = rng.standard_normal((B, M)).astype(np.float32)
    for b in range(0, B, 3):
        t = int(rng.integers(0, M + 1))
        ids[b, M - t:], scores[b, M - t:] = -1, -np.inf
    ids[4, 3], ids[5, 3], scores[6, 3] = N, 2 ** 40, np.nan
    return items, ids, scores


def _same(a, b, what):
    for x, y, name in zip(a, b, ("ids", "scores", "value", "ild")):
        assert x.tobytes() == y.tobytes(), "%s: %s differs" % (what, name)


def test_rows_do_not_depend_on_the_batch_the_catalogue_length_or_the_run():
    items, ids, scores = _invariance_case()
    B, N = ids.shape[0], items.shape[0]
    k, lam = 30, 0.5
    whole = _rerank(items, ids, scores, k, lam)
    _same(whole, _rerank(items, ids, scores, k, lam), "two runs")
    for cut in (1, 18):
        a, b = _rerank(items, ids[:cut], scores[:cut], k, lam), _rerank(items, ids[cut:], scores[cut:], k, lam)
        _same(whole, tuple(np.concatenate([x, y]) for x, y in zip(a, b)), "split %d + %d" % (cut, B - cut))
    perm = np.random.default_rng(1).permutation(B)
    _same(tuple(x[perm] for x in whole), _rerank(items, ids[perm], scores[perm], k, lam), "rows permuted")
    # a catalogue twice as long, the rows moved: ids follow their rows, ids that named no row still name none
    new_of = np.random.default_rng(2).permutation(2 * N)[:N]
    items2 = np.random.default_rng(3).standard_normal((2 * N, items.shape[1])).astype(np.float32)
    items2[new_of] = items
    ids2 = np.where((ids >= 0) & (ids < N), new_of[np.clip(ids, 0, N - 1)], np.where(ids == N, 2 * N, ids))
    got = _rerank(items2, ids2, scores, k, lam)
    back = np.full(2 * N, -7, dtype=np.int64)
    back[new_of] = np.arange(N)
    _same(whole, (np.where(got[0] >= 0, back[np.clip(got[0], 0, 2 * N - 1)], got[0]),) + got[1:], "catalogue twice as long")


@pytest.mark.parametrize("M,k,d", [(100, 30, 60), (256, 256, 33), (1, 1, 4)])
def test_guard_bands_and_poisoned_workspace(M, k, d):
    lib = _lib.load()
    items, ids, scores = _invariance_case()
    if M <= 100:
        ids, scores = np.ascontiguousarray(ids[:, :M]), np.ascontiguousarray(scores[:, :M])
    else:
        reps = -(-M // ids.shape[1])
        ids, scores = np.ascontiguousarray(np.tile(ids, reps)[:, :M]), np.ascontiguousarray(np.tile(scores, reps)[:, :M])
    items = np.ascontiguousarray(np.random.default_rng(d).standard_normal((items.shape[0], d)).astype(np.float32))
    B, N = ids.shape[0], items.shape[0]
    lam = 0.5
    t_items, t_ids, t_scores = _dev(items, torch.float32), _dev(ids, torch.int64), _dev(scores, torch.float32)
    nbytes = lib.nrms_mmr_rerank_workspace_bytes(B, M, d, k)
    assert nbytes > 0
    runs = {}
    for poison in POISONS:
        pool = Pool(poison)
        o_ids, o_sc = pool.elems("out_ids", B * k, torch.int64), pool.elems("out_scores", B * k)
        o_val, o_ild = pool.elems("out_value", B * k), pool.elems("ild", B)
        ws = pool.new("workspace", nbytes)
        rc = lib.nrms_mmr_rerank(B, M, d, k, C.c_int64(N), C.c_float(lam), _lib.ptr(t_items), _lib.ptr(t_ids), _lib.ptr(t_scores),
                                 o_ids.ptr, o_sc.ptr, o_val.ptr, o_ild.ptr, ws.ptr, C.c_size_t(nbytes), _stream())
        _lib.check(rc, "nrms_mmr_rerank")
        pool.intact("nrms_mmr_rerank")
        runs[poison] = {"ids": o_ids.numpy((B, k)), "scores": o_sc.numpy((B, k)), "value": o_val.numpy((B, k)), "ild": o_ild.numpy()}
        # the nullable outputs left out: the others do not change
        pool2 = Pool(poison)
        q_ids, q_sc = pool2.elems("out_ids", B * k, torch.int64), pool2.elems("out_scores", B * k)
        ws2 = pool2.new("workspace", nbytes)
        rc = lib.nrms_mmr_rerank(B, M, d, k, C.c_int64(N), C.c_float(lam), _lib.ptr(t_items), _lib.ptr(t_ids), _lib.ptr(t_scores),
                                 q_ids.ptr, q_sc.ptr, None, None, ws2.ptr, C.c_size_t(nbytes), _stream())
        _lib.check(rc, "nrms_mmr_rerank")
        pool2.intact("nrms_mmr_rerank without value / ild")
        assert q_ids.numpy((B, k)).tobytes() == runs[poison]["ids"].tobytes()
        assert q_sc.numpy((B, k)).tobytes() == runs[poison]["scores"].tobytes()
    assert_same_bits(runs, "nrms_mmr_rerank")
    eng = _rerank(items, ids, scores, k, lam)
    first = runs[POISONS[0]]
    _same(eng, (first["ids"], first["scores"], first["value"], first["ild"]), "engine against the raw call")
    rc = lib.nrms_mmr_rerank(B, M, d, k, C.c_int64(N), C.c_float(lam), _lib.ptr(t_items), _lib.ptr(t_ids), _lib.ptr(t_scores),
                             o_ids.ptr, o_sc.ptr, None, None, ws.ptr, C.c_size_t(nbytes - 1), _stream())
    assert rc != 0 and b"workspace" in lib.nrms_last_error()


def test_engine_edges():
    eng = _engine()
    items, ids, scores = _invariance_case()
    t_items, t_ids, t_scores = _dev(items, torch.float32), _dev(ids, torch.int64), _dev(scores, torch.float32)
    o = eng.mmr_rerank(t_items, t_ids[:0].contiguous(), t_scores[:0].contiguous(), 5, 0.5, return_ild=True)
    assert o[0].shape == (0, 5) and o[1].shape == (0, 5) and o[2].shape == (0,)
    o = eng.mmr_rerank(t_items[:0].contiguous(), t_ids, t_scores, 5, 0.5, return_value=True, return_ild=True)       # N = 0
    assert (o[0] == -1).all() and (o[1] == -float("inf")).all() and (o[2] == -float("inf")).all() and torch.isnan(o[3]).all()
    whole = eng.mmr_rerank(t_items, t_ids, t_scores, 7, 0.25, return_value=True, return_ild=True)
    cap = eng.MMR_WORKSPACE_CAP
    try:
        eng.MMR_WORKSPACE_CAP = 5 * eng.lib.nrms_mmr_rerank_workspace_bytes(1, ids.shape[1], items.shape[1], 7)   # row chunks of 5
        parts = eng.mmr_rerank(t_items, t_ids, t_scores, 7, 0.25, return_value=True, return_ild=True)
    finally:
        eng.MMR_WORKSPACE_CAP = cap
    for a, b in zip(whole, parts):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for bad in (dict(k=0), dict(k=101), dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan"))):
        with pytest.raises(_lib.NrmsError, match="mmr_rerank"):
            eng.mmr_rerank(t_items, t_ids, t_scores, bad.get("k", 5), bad.get("lam", 0.5))
    with pytest.raises(_lib.NrmsError, match="short_scores"):
        eng.mmr_rerank(t_items, t_ids, t_scores[:, :50].contiguous(), 5, 0.5)
    with pytest.raises(_lib.NrmsError, match="short_ids"):
        eng.mmr_rerank(t_items, t_ids.to(torch.int32), t_scores, 5, 0.5)


# ---- 5: the effect ----------------------------------------------------------------------------------------------------------
def test_diversity_raises_ild_on_a_clustered_catalogue():
    """8 clusters around orthogonal unit vectors; every user's vector points at cluster 0 (36 news, all of which outscore
    every other news: they fill the top 36 of the shortlist of 40) with a smaller, user-specific liking for the others."""
    cfg, model, batches, _ = _model("nrms_v0")
    rng = np.random.default_rng(5)
    d, B, per = cfg.word_embed_size, 16, 36
    cluster = np.concatenate([[-1], np.repeat(np.arange(8), per)])                       # news id -> cluster (id 0: padding)
    cat = np.zeros((1 + 8 * per, d), dtype=np.float32)
    cat[1:] = np.eye(d, dtype=np.float32)[cluster[1:]] + 0.02 * rng.standard_normal((8 * per, d)).astype(np.float32)
    users = np.zeros((B, d), dtype=np.float32)
    users[:, 0] = 1.0
    users[:, 1:8] = rng.uniform(0.3, 0.7, size=(B, 7))
    t_users = _dev(users, torch.float32)
    model._catalogue_users = lambda hist, browsed=None: t_users                          # the user side is not under test
    batch = {"browsed_ids": torch.zeros(B, cfg.history_len, dtype=torch.int64, device=DEV)}
    t_cat = _dev(cat, torch.float32)
    top40, _ = model.recommend(batch, 40, t_cat)
    assert (cluster[top40.cpu().numpy()[:, :per]] == 0).all()                            # the generator's promise
    p_ids, _, p_ild = model.recommend(batch, 10, t_cat, return_ild=True)
    m_ids, _, m_ild = model.recommend(batch, 10, t_cat, diversity=0.5, return_ild=True)
    p_ild, m_ild = p_ild.cpu().numpy(), m_ild.cpu().numpy()
    print("plain ILD@10 %.4f .. %.4f   diversity 0.5 ILD@10 %.4f .. %.4f" % (p_ild.min(), p_ild.max(), m_ild.min(), m_ild.max()))
    assert (m_ild > p_ild).all()
    p_ids, m_ids = p_ids.cpu().numpy(), m_ids.cpu().numpy()
    assert (m_ids[:, 0] == p_ids[:, 0]).all()                                            # the best news still leads
    assert all(len(set(cluster[row])) > 1 for row in m_ids) and (cluster[p_ids] == 0).all()


# ---- 6: the layers ----------------------------------------------------------------------------------------------------------
def test_train_eval_recommend_with_diversity(tmp_path):
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    torch.manual_seed(0)
    cfg = _tiny_cfg("nrms_v0")
    corpus = SyntheticMind(cfg, n_news=300, n_topics=4, seed=1)
    from pytorch_news_recommender_amd.model.nrms_hip import Model
    model = Model(cfg, pretrained_word_embedding=corpus.embedding_table(cfg.word_embed_size)).to("cuda")
    samples, _ = corpus.eval_samples(100, max_shown=20)
    feed = DeviceFeed(cfg, samples, type=1, id2title_dict=corpus.id2title_dict, batch_size=cfg.batch_size, device=DEV)
    plain = train_eval.recommend(cfg, model, feed, feed.titles, 10, out_file=str(tmp_path / "plain.txt"))
    assert model.last_recommend_stats is None
    one = train_eval.recommend(cfg, model, feed, feed.titles, 10, out_file=str(tmp_path / "one.txt"), diversity=1.0)
    assert open(one).read() == open(plain).read()
    st_plain = dict(model.last_recommend_stats)
    out = train_eval.recommend(cfg, model, feed, feed.titles, 10, out_file=str(tmp_path / "div.txt"), diversity=0.5, shortlist=64)
    st = model.last_recommend_stats
    lines = open(out).read().splitlines()
    hist = feed.packed["hist"].cpu().numpy()
    assert len(lines) == feed.n
    seen = set()
    for i, ln in enumerate(lines):
        m = re.fullmatch(r"(\d+) \[(\d+(?:,\d+)*)\]", ln)
        assert m and int(m.group(1)) == i + 1, ln
        ids = [int(v) for v in m.group(2).split(",")]
        assert len(ids) == 10 == len(set(ids)) and 0 not in ids and not set(ids) & set(hist[i].tolist())
        seen |= set(ids)
    assert set(st) == {"ild", "coverage", "n_users"} and st["n_users"] == feed.n
    assert abs(st["coverage"] - len(seen) / (feed.titles.shape[0] - 1)) < 1e-12
    assert 0.0 <= st_plain["ild"] < st["ild"] <= 2.0
    with pytest.raises(ValueError, match="shortlist"):
        train_eval.recommend(cfg, model, feed, feed.titles, 10, out_file=str(tmp_path / "x.txt"), shortlist=64)


def test_run_v0_diversity_flag(tmp_path):
    out = tmp_path / "rec.txt"
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "pytorch_news_recommender_amd.run_v0", "--model", "nrms_hip", "--dataset", "synthetic",
                        "--max_batches", "2", "--epochs", "1", "--synthetic_users", "128", "--batch_size", "64",
                        "--description", "T", "--data_path", str(tmp_path / "data"), "--save_path", str(tmp_path / "save"),
                        "--recommend", "5", "--diversity", "0.5", "--recommend_out", str(out)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    ild = re.findall(r"^(plain|diversity 0\.5): ILD@5: (\d\.\d+)  coverage: (\d\.\d+)  users: (\d+)$", r.stdout, re.M)
    assert [m[0] for m in ild] == ["plain", "diversity 0.5"], r.stdout[-2000:]
    assert float(ild[1][1]) >= float(ild[0][1])
    lines = out.read_text().splitlines()
    assert len(lines) == 1024 and all(re.fullmatch(r"\d+ \[\d+(?:,\d+){4}\]", ln) for ln in lines)


def test_hierec_and_graph_refuse_diversity():
    from pytorch_news_recommender_amd.data_handler import SyntheticMind
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    cfg = _tiny_cfg("hierec")
    corpus = SyntheticMind(cfg, n_news=50, n_topics=4, seed=1)
    hier = hierec_hip.Model(cfg, pretrained_word_embedding=corpus.embedding_table(cfg.word_embed_size)).to("cuda")
    batch = {"browsed_ids": torch.zeros(2, cfg.history_len, dtype=torch.int64, device=DEV)}
    with pytest.raises(_lib.NrmsError, match="diversity"):
        hier.recommend(batch, 5, None, diversity=0.5)
    with pytest.raises(_lib.NrmsError, match="diversity"):
        hier.recommend(batch, 5, None, return_ild=True)
    shape = synth.G1_ODD
    from pytorch_news_recommender_amd.config import Config
    gcfg = Config("graph")
    gcfg.__nrms__()
    gcfg.word_embed_size, gcfg.num_attention_heads, gcfg.query_vector_dim = shape.word_embed_size, shape.num_attention_heads, shape.query_vector_dim
    params = synth.make_params_graph(shape, seed=3)
    graph = graph_hip.Model(gcfg, pretrained_word_embedding=params["news_encoder.word_embedding.0.weight"]).to("cuda")
    with pytest.raises(_lib.NrmsError, match="diversity"):
        graph.recommend(batch, 5, None, diversity=0.5)
