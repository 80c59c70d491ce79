"""nrms_rank_dot on the GPU (the exact rank of given items in nrms_topk_dot's order, include/nrms_hip.h): exact against a host
lexsort on tie-heavy integer data at every width / target count / exclude path, the score bits and positions of top_k itself,
invariance and determinism, the buffer contract, and the layers built on it (NRMSEngine.rank_of, Model.rank_targets,
train_eval.evaluate_retrieval, run_v0 --retrieval_metrics)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENG = []


def _engine():
    if not _ENG:
        _ENG.append(NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), DEV))
    return _ENG[0]


def _rank(user, items, targets, exclude=None):
    u = torch.as_tensor(user).to(DEV).contiguous()
    it = torch.as_tensor(items).to(DEV).contiguous()
    tg = torch.as_tensor(targets, dtype=torch.int64).to(DEV).contiguous()
    ex = None if exclude is None else torch.as_tensor(exclude, dtype=torch.int64).to(DEV).contiguous()
    r, s = _engine().rank_of(u, it, tg, ex)
    return r.cpu().numpy(), s.cpu().numpy()


def _host_positions(user, items, exclude):
    """The contract on the host: float64 scores (exact for integer inputs), eligible = not excluded and not NaN, the order
    np.lexsort((ids, -scores)).  -> (scores [B, N] f64, pos [B, N]: 1-based place of every eligible item, 0 otherwise)."""
    s = user.astype(np.float64) @ items.astype(np.float64).T
    B, N = s.shape
    pos = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        ok = ~np.isnan(s[b])
        if exclude is not None:
            ex = np.asarray(exclude[b])
            ok[ex[(ex >= 0) & (ex < N)]] = False
        ids = np.nonzero(ok)[0]
        order = ids[np.lexsort((ids, -s[b, ids]))]
        pos[b, order] = np.arange(1, len(order) + 1)
    return s, pos


def _host_rank(user, items, targets, exclude):
    s, pos = _host_positions(user, items, exclude)
    B, N = s.shape
    ranks = np.zeros(targets.shape, dtype=np.int32)
    scores = np.full(targets.shape, -np.inf, dtype=np.float32)
    for b in range(B):
        for j, t in enumerate(targets[b]):
            if 0 <= t < N and pos[b, t] > 0:
                ranks[b, j] = pos[b, t]
                scores[b, j] = np.float32(s[b, t]) + np.float32(0.0)          # -0.0 is returned as +0.0
    return ranks, scores


def _assert_exact(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.int32), want[1].view(np.int32))


@functools.lru_cache(maxsize=2)
def _int_case(B, N, d, n_ex):
    """Integer data as test_hip_topk._int_data: values in [-3, 3] (float64 scores are exact, ties everywhere), NaN item rows,
    exclude lists that hold -1, N, id 0 and a duplicated id.  Also the host's scores and, per item, whether it is NaN."""
    from tests.test_hip_topk import _int_data
    user, items, ex = _int_data(B, N, d, seed=1000 * d + n_ex, n_ex=max(n_ex, 5))
    ex = ex if n_ex else None
    return user, items, ex, np.nonzero(np.isnan(items[:, 0]))[0]


def _targets(B, N, T, ex, nan_ids, seed):
    """Random ids, and in every row (T >= 6; shorter rows take one kind each, row b kind b % 6): -1, N, an excluded id, the id of
    a NaN row, and one id twice."""
    rng = np.random.default_rng(seed)
    tg = rng.integers(0, N, size=(B, T)).astype(np.int64)
    for b in range(B):
        special = [-1, N, int(ex[b, min(5, ex.shape[1] - 1)]) if ex is not None else N + 7, int(nan_ids[b % len(nan_ids)]), int(tg[b, 0])]
        if T >= 6:
            tg[b, 1:6] = special
        elif b % 6:
            tg[b, T - 1] = special[b % 6 - 1]
    return tg


@pytest.mark.parametrize("n_ex", [0, 50, 70])           # none, the exclude list in LDS, the list read from global memory
@pytest.mark.parametrize("T", [1, 5, 32])
@pytest.mark.parametrize("d", [1, 3, 31, 64, 301])      # no whole 32-block, remainder groups, vector and scalar loads
def test_exact_with_ties_nan_and_excludes(d, T, n_ex):
    B, N = 37, 10007                                    # one full and one partial user tile; several slices, a ragged last tile
    user, items, ex, nan_ids = _int_case(B, N, d, n_ex)
    tg = _targets(B, N, T, ex, nan_ids, seed=T)
    got = _rank(user, items, tg, ex)
    want = _host_rank(user, items, tg, ex)
    _assert_exact(got, want)
    if T >= 6:
        assert (got[0][:, 1:5] == 0).all() and (got[1][:, 1:5] == -np.inf).all()       # -1, N, excluded, NaN
        np.testing.assert_array_equal(got[0][:, 5], got[0][:, 0])                        # the id listed twice
    assert (got[0] > 0).any()


def test_small_catalogues_and_empty_calls():
    rng = np.random.default_rng(3)
    user = rng.integers(-3, 4, size=(4, 16)).astype(np.float32)
    items = rng.integers(-3, 4, size=(5, 16)).astype(np.float32)
    items[3] = np.nan
    ex = np.array([[0, 1, 2, 3, 4], [-1, -1, -1, -1, -1], [1, 1, 9, -5, 2], [4, 4, 4, 4, 4]])
    tg = np.tile(np.array([0, 1, 2, 3, 4, 5, -1]), (4, 1))
    got = _rank(user, items, tg, ex)
    _assert_exact(got, _host_rank(user, items, tg, ex))
    assert (got[0][0] == 0).all() and (got[1][0] == -np.inf).all()                   # the user who excludes everything
    assert sorted(got[0][1, [0, 1, 2, 4]].tolist()) == [1, 2, 3, 4] and (got[0][1, [3, 5, 6]] == 0).all()
    r, s = _rank(user, np.zeros((0, 16), np.float32), tg)                            # N = 0: rank 0 / -inf everywhere
    assert r.shape == tg.shape and (r == 0).all() and (s == -np.inf).all()
    r, s = _rank(np.zeros((0, 16), np.float32), items, np.zeros((0, 3), np.int64))   # B = 0
    assert r.shape == (0, 3) and s.shape == (0, 3)


def _normal_data(B=70, N=20000, d=300, n_ex=50, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    user = torch.randn(B, d, device=DEV, generator=g)
    items = torch.randn(N, d, device=DEV, generator=g)
    ex = torch.randint(0, N, (B, n_ex), device=DEV, generator=g)
    return user, items, ex


def test_bit_consistent_with_top_k():
    """Fails for any score chain other than nrms_topk_dot's: a different rounding moves near-ties across positions."""
    user, items, ex = _normal_data()
    B, N = user.shape[0], items.shape[0]
    eng = _engine()
    s, ids = eng.top_k(user, items, 256, ex)
    g = torch.Generator(device=DEV).manual_seed(7)
    extra = torch.randint(0, N, (B, 28), device=DEV, generator=g)
    cols = [0, 9, 99, 255]
    tg = torch.cat([ids[:, cols], extra], dim=1).contiguous()
    ranks, sc = eng.rank_of(user, items, tg, ex)
    want = torch.tensor([1, 10, 100, 256], dtype=torch.int32, device=DEV).expand(B, 4)
    assert torch.equal(ranks[:, :4], want)
    assert torch.equal(sc[:, :4].contiguous().view(torch.int32), s[:, cols].contiguous().view(torch.int32))
    # a further target is within the first 256 exactly when top_k lists it, and then at that place
    hit = extra.unsqueeze(2) == ids.unsqueeze(1)                       # [B, 28, 256]
    place = torch.where(hit.any(2), hit.to(torch.int32).argmax(2).to(torch.int32) + 1, torch.zeros((), dtype=torch.int32, device=DEV))
    r = ranks[:, 4:]
    assert torch.equal((r > 0) & (r <= 256), hit.any(2))
    assert torch.equal(torch.where(hit.any(2), r, torch.zeros_like(r)), place)
    excluded = (extra.unsqueeze(2) == ex.unsqueeze(1)).any(2)
    assert torch.equal(r == 0, excluded)


def test_invariance_and_determinism():
    user, items, ex = _normal_data(seed=1)
    B, N = user.shape[0], items.shape[0]
    eng = _engine()
    g = torch.Generator(device=DEV).manual_seed(11)
    tg = torch.randint(0, N, (B, 32), device=DEV, generator=g)
    bits = lambda t: t.contiguous().view(torch.int32)
    r, s = eng.rank_of(user, items, tg, ex)
    r2, s2 = eng.rank_of(user, items, tg, ex)
    assert torch.equal(r, r2) and torch.equal(bits(s), bits(s2))
    # users split 23 / 47 over two calls
    ra, sa = eng.rank_of(user[:23].contiguous(), items, tg[:23].contiguous(), ex[:23].contiguous())
    rb, sb = eng.rank_of(user[23:].contiguous(), items, tg[23:].contiguous(), ex[23:].contiguous())
    assert torch.equal(torch.cat([ra, rb]), r) and torch.equal(bits(torch.cat([sa, sb])), bits(s))
    # T = 32 is four calls of T = 8 on the column blocks
    for c0 in range(0, 32, 8):
        rc, sc = eng.rank_of(user, items, tg[:, c0:c0 + 8].contiguous(), ex)
        assert torch.equal(rc, r[:, c0:c0 + 8]) and torch.equal(bits(sc), bits(s[:, c0:c0 + 8]))
    # more than 32 columns go in chunks
    wide = torch.cat([tg, tg[:, :5]], dim=1).contiguous()
    rw, sw = eng.rank_of(user, items, wide, ex)
    assert torch.equal(rw, torch.cat([r, r[:, :5]], dim=1)) and torch.equal(bits(sw), bits(torch.cat([s, s[:, :5]], dim=1)))
    # an out-of-range or duplicate id added to the exclude list changes nothing
    more = torch.cat([ex, torch.full((B, 1), N, device=DEV), torch.full((B, 1), -1, device=DEV), ex[:, 3:4]], dim=1).contiguous()
    rm, sm = eng.rank_of(user, items, tg, more)
    assert torch.equal(rm, r) and torch.equal(bits(sm), bits(s))
    # a valid id e added to user b's list lowers exactly the ranks of b's targets that e preceded, by 1
    b = 41
    cand = torch.randint(0, N, (B, 32), device=DEV, generator=g)
    rc, sc = eng.rank_of(user, items, cand, ex)
    taken = set(tg[b].tolist()) | set(ex[b].tolist())
    lo, hi = int(r[b][r[b] > 0].min()), int(r[b].max())
    j = next(j for j in range(32) if lo < int(rc[b, j]) < hi and int(cand[b, j]) not in taken)      # e lies between b's targets
    e, se = int(cand[b, j]), sc[b, j]
    col = torch.full((B, 1), -1, dtype=torch.int64, device=DEV)
    col[b, 0] = e
    r3, s3 = eng.rank_of(user, items, tg, torch.cat([ex, col], dim=1).contiguous())
    preceded = (r[b] > 0) & ((se > s[b]) | ((se == s[b]) & (e < tg[b])))
    assert preceded.any() and not preceded.all()
    want = r.clone()
    want[b] -= preceded.to(torch.int32)
    assert torch.equal(r3, want) and torch.equal(bits(s3), bits(s))


@pytest.mark.parametrize("B,N,d,T,n_ex", [(1, 1, 8, 1, 0), (3, 33, 7, 5, 6), (33, 2100, 20, 32, 70), (2, 64, 300, 7, 3)])
def test_buffer_contract(B, N, d, T, n_ex):
    """ranks, target_scores and the workspace at the queried size between guard bands, the workspace poisoned three ways."""
    from tests.guarded import POISONS, Pool
    from tests.test_hip_buffer_contracts import _stream, dev, ok, refuses_undersized, three_poisons
    lib = _lib.load()
    user, items, ex, nan_ids = _int_case(B, N, d, n_ex)
    ex = None if ex is None else ex[:, :n_ex]
    tg = _targets(B, N, T, ex, nan_ids, seed=N)
    ud, itd, tgd = dev(user), dev(items), dev(tg, torch.int64)
    exd = None if ex is None else dev(ex, torch.int64)
    need = int(lib.nrms_rank_dot_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    assert need > 0

    def call(P, nbytes):
        return lib.nrms_rank_dot(B, C.c_int64(N), d, T, _lib.ptr(ud), _lib.ptr(itd), _lib.ptr(tgd), _lib.ptr(exd), n_ex,
                                 P["ranks"].ptr, P["target_scores"].ptr, P["workspace"].ptr, C.c_size_t(nbytes), _stream())

    def run(poison):
        P = Pool(poison)
        P.elems("ranks", B * T, torch.int32), P.elems("target_scores", B * T), P.new("workspace", need)
        ok(call(P, need), "nrms_rank_dot")
        P.intact("nrms_rank_dot")
        if poison == POISONS[0]:
            refuses_undersized(lambda n: call(P, n), P, need, "nrms_rank_dot")
        return {"ranks": P["ranks"].numpy((B, T)), "scores": P["target_scores"].numpy((B, T))}

    r = three_poisons(run, "nrms_rank_dot")[POISONS[0]]
    _assert_exact((r["ranks"], r["scores"]), _host_rank(user, items, tg, ex))


def _model(kind, n_imps, batch_size=64):
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    from pytorch_news_recommender_amd.model import nrms_hip, nrms_v1_hip
    torch.manual_seed(0)
    cfg = Config(kind)
    cfg.__nrms__()
    cfg.n_words, cfg.n_words_title, cfg.history_len, cfg.sample_size, cfg.max_candidate_size = 600, 12, 10, 4, 24
    cfg.word_embed_size, cfg.num_attention_heads, cfg.title_heads_num, cfg.query_vector_dim = 60, 6, 3, 32
    cfg.batch_size, cfg.dropout = batch_size, 0.2
    corpus = SyntheticMind(cfg, n_news=4000, n_topics=4, seed=1)
    cls = nrms_hip.Model if kind == "nrms_v0" else nrms_v1_hip.Model
    model = cls(cfg, pretrained_word_embedding=corpus.embedding_table(cfg.word_embed_size)).to("cuda")
    samples, labels = corpus.eval_samples(n_imps, max_shown=20)
    feed = DeviceFeed(cfg, samples, type=1, id2title_dict=corpus.id2title_dict, batch_size=cfg.batch_size, device=DEV)
    return cfg, model, feed, labels


@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_v1"])
def test_model_rank_targets_agrees_with_recommend(kind):
    cfg, model, feed, _ = _model(kind, 128)
    cat = model.encode_catalogue(feed.titles)
    n = 0
    for batch in feed:
        n += 1
        ids, scores = model.recommend(batch, 50, cat)
        B = ids.shape[0]
        assert (ids > 0).all()
        ranks, sc = model.rank_targets(batch, ids, cat)
        assert ranks.dtype == torch.int32 and ranks.shape == (B, 50)
        assert torch.equal(ranks, torch.arange(1, 51, dtype=torch.int32, device=DEV).expand(B, 50))
        assert torch.equal(sc.view(torch.int32), scores.view(torch.int32))
        # a browsed id: rank 0 with exclude_history, a place in the list without; news id 0 and padding never rank
        hist = batch["browsed_ids"]
        assert (hist[:, 0] > 0).all()
        tg = torch.stack([hist[:, 0], torch.zeros_like(hist[:, 0]), torch.full_like(hist[:, 0], -1), ids[:, 0]], dim=1)
        r_ex, s_ex = model.rank_targets(batch, tg, cat)
        r_in, _ = model.rank_targets(batch, tg, cat, exclude_history=False)
        assert (r_ex[:, 0] == 0).all() and (s_ex[:, 0] == -float("inf")).all() and (r_in[:, 0] > 0).all()
        assert (r_ex[:, 1:3] == 0).all() and (r_in[:, 1:3] == 0).all()
        assert (r_ex[:, 3] == 1).all() and (r_in[:, 3] >= 1).all()
        with pytest.raises(KeyError):
            model.rank_targets({"browsed_titles": batch["browsed_titles"]}, tg, cat)
    assert n == 2
    model.check_recommend_ids()


def test_evaluate_retrieval_means_and_counts():
    cfg, model, feed, labels = _model("nrms_v0", 256)
    ks = (10, 100)
    res = train_eval.evaluate_retrieval(cfg, model, feed, feed.titles, labels, ks=ks, verbose=False)
    m = model.last_retrieval_metrics
    ranks = m["ranks"].cpu().numpy()
    assert ranks.shape[0] == 256 and ranks.dtype == np.int32
    from tests.test_rank_host import _host_metrics
    want = _host_metrics(ranks, ks)
    have = (ranks > 0).any(axis=1)
    for name, per_user in want.items():
        np.testing.assert_allclose(m[name].cpu().numpy(), per_user, rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
        assert abs(res[name] - per_user[have].mean()) <= 1e-12, name
    assert res["median_rank"] == float(np.median(ranks[ranks > 0]))
    assert res["recall@10"] <= res["recall@100"] and res["ndcg@10"] <= res["ndcg@100"] + 1e-12
    assert res["n_users"] == int(have.sum()) and res["n_targets"] == int((ranks > 0).sum())
    assert res["n_targets"] + res["n_skipped"] == sum(int(np.sum(np.asarray(y[:cfg.max_candidate_size]) == 1)) for y in labels)
    assert res["n_targets"] > 0
    # every ranked target is a clicked candidate of its impression, at the place rank_targets gives it alone
    tg = m["targets"].cpu().numpy()
    cand = feed.packed["cand"].cpu().numpy()
    for i in (0, 100, 255):
        clicked = [c for c, y in zip(cand[i], labels[i]) if y == 1]
        assert tg[i][tg[i] >= 0].tolist() == clicked


def test_run_v0_retrieval_metrics_flag(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "pytorch_news_recommender_amd.run_v0", "--model", "nrms_hip", "--dataset", "synthetic",
                        "--max_batches", "2", "--epochs", "1", "--synthetic_users", "256", "--batch_size", "64",
                        "--description", "T", "--data_path", str(tmp_path / "data"), "--save_path", str(tmp_path / "save"),
                        "--retrieval_metrics", "10,100"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("retrieval over")]
    assert len(line) == 1, r.stdout[-3000:]
    m = re.fullmatch(r"retrieval over 4000 news: recall@10: ([\d.]+)  recall@100: ([\d.]+)  ndcg@10: ([\d.]+)  ndcg@100: ([\d.]+)  "
                     r"mrr: ([\d.]+)  median rank: ([\d.]+)  users: (\d+)  targets: (\d+)  skipped: (\d+)", line[0])
    assert m, line[0]
    assert float(m.group(1)) <= float(m.group(2)) <= 1.0 and int(m.group(7)) <= 1024 and int(m.group(8)) >= int(m.group(7)) > 0
