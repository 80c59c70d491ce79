"""nrms_topk_dot on the GPU (catalogue-wide top-k, include/nrms_hip.h): exact against a host lexsort on tie-heavy integer
data at every k and many widths, padding, the bench size against float64 scores, invariance and determinism, and the layers
built on it (NRMSEngine.top_k, Model.encode_catalogue / recommend, train_eval.recommend, run_v0 --recommend)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import train_eval
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENG = []


def _engine():
    if not _ENG:
        _ENG.append(NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), DEV))
    return _ENG[0]


def _topk(user, items, k, exclude=None):
    u = torch.as_tensor(user).to(DEV).contiguous()
    it = torch.as_tensor(items).to(DEV).contiguous()
    ex = None if exclude is None else torch.as_tensor(exclude, dtype=torch.int64).to(DEV).contiguous()
    s, i = _engine().top_k(u, it, k, ex)
    return s.cpu().numpy(), i.cpu().numpy()


def _host_topk(user, items, k, exclude=None):
    """The contract on the host: float64 scores (exact for these integer inputs), eligible = not excluded and not NaN,
    np.lexsort((ids, -scores)), then id -1 / score -inf."""
    s = user.astype(np.float64) @ items.astype(np.float64).T
    B, N = s.shape
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_i = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        ok = ~np.isnan(s[b])
        if exclude is not None:
            ex = np.asarray(exclude[b])
            ok[ex[(ex >= 0) & (ex < N)]] = False
        ids = np.nonzero(ok)[0]
        top = ids[np.lexsort((ids, -s[b, ids]))][:k]
        out_i[b, :len(top)] = top
        out_s[b, :len(top)] = s[b, top].astype(np.float32) + np.float32(0.0)       # -0.0 is returned as +0.0
    return out_s, out_i


def _assert_exact(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0].view(np.int32), want[0].view(np.int32))


def _int_data(B, N, d, seed, n_ex=60):
    rng = np.random.default_rng(seed)
    user = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    items[rng.choice(N, size=max(1, N // 97), replace=False)] = np.nan
    ex = rng.integers(0, N, size=(B, n_ex))
    ex[:, 0], ex[:, 1], ex[:, 2], ex[:, 3] = -1, N, 0, ex[:, 4]          # out of range, id 0, a duplicate
    return user, items, ex


@pytest.mark.parametrize("k", [1, 10, 100, 256])
def test_exact_with_ties_and_nan(k):
    user, items, ex = _int_data(37, 10007, 300, seed=k)
    _assert_exact(_topk(user, items, k, ex), _host_topk(user, items, k, ex))


@pytest.mark.parametrize("d", [1, 2, 3, 31, 64, 301, 800])
def test_exact_at_every_width(d):
    # 70 exclude ids: longer lists than the kernel stages in LDS take its global-memory path
    user, items, ex = _int_data(37, 3001, d, seed=d, n_ex=70 if d % 2 else 50)
    _assert_exact(_topk(user, items, 100, ex), _host_topk(user, items, 100, ex))
    _assert_exact(_topk(user, items, 7, None), _host_topk(user, items, 7, None))


def test_padding_when_k_exceeds_the_eligible_items():
    rng = np.random.default_rng(3)
    user = rng.integers(-3, 4, size=(4, 16)).astype(np.float32)
    items = rng.integers(-3, 4, size=(5, 16)).astype(np.float32)
    items[3] = np.nan
    ex = np.array([[0, 1, 2, 3, 4], [-1, -1, -1, -1, -1], [1, 1, 9, -5, 2], [4, 4, 4, 4, 4]])
    got = _topk(user, items, 10, ex)
    _assert_exact(got, _host_topk(user, items, 10, ex))
    assert (got[1][0] == -1).all() and (got[0][0] == -np.inf).all()          # the user who excludes everything
    assert (got[1][1, :4] >= 0).all() and (got[1][1, 4:] == -1).all()        # 4 eligible items (one NaN row)
    s, i = _topk(user, np.zeros((0, 16), np.float32), 3)                     # N = 0: all padding
    assert (i == -1).all() and (s == -np.inf).all()
    s, i = _topk(np.zeros((0, 16), np.float32), items, 3)                    # B = 0
    assert s.shape == (0, 3) and i.shape == (0, 3)


def _bench_data(B=512, N=130000, d=300, n_ex=50, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    user = torch.randn(B, d, device=DEV, generator=g)
    items = torch.randn(N, d, device=DEV, generator=g)
    ex = torch.randint(0, N, (B, n_ex), device=DEV, generator=g)
    return user, items, ex


def test_bench_size_against_float64():
    user, items, ex = _bench_data()
    B, N = user.shape[0], items.shape[0]
    k = 100
    s, ids = _engine().top_k(user, items, k, ex)
    assert (ids >= 0).all() and (ids < N).all()
    u64, a64 = user.double(), user.double().abs()
    picked = items.index_select(0, ids.view(-1)).view(B, k, -1).double()
    s64 = torch.einsum("bd,bkd->bk", u64, picked)
    bound = 1e-6 * torch.einsum("bd,bkd->bk", a64, picked.abs())
    assert ((s.double() - s64).abs() <= bound).all()
    # no excluded id, no id twice, sorted by (score desc, id asc)
    assert not (ids.unsqueeze(2) == ex.unsqueeze(1)).any()
    srt = ids.sort(dim=1).values
    assert (srt[:, 1:] != srt[:, :-1]).all()
    ds, di = s[:, 1:] - s[:, :-1], ids[:, 1:] - ids[:, :-1]
    assert ((ds < 0) | ((ds == 0) & (di > 0))).all()
    # nothing eligible left out scores above the k-th plus twice the bound
    theta = s[:, -1].double()
    for c0 in range(0, N, 8192):
        blk = items[c0:c0 + 8192].double()
        sc = u64 @ blk.T
        bd = 1e-6 * (a64 @ blk.abs().T)
        n = torch.arange(c0, c0 + blk.shape[0], device=DEV)
        out = (n[None, :, None] == ex[:, None, :]).any(2) | (n[None, :, None] == ids[:, None, :]).any(2)
        assert not ((sc > theta[:, None] + 2 * bd) & ~out).any()


def test_invariance_and_determinism():
    user, items, ex = _bench_data(B=300, N=20000, seed=1)
    eng = _engine()
    s, i = eng.top_k(user, items, 100, ex)
    s2, i2 = eng.top_k(user, items, 100, ex)
    assert torch.equal(i, i2) and torch.equal(s.view(torch.int32), s2.view(torch.int32))
    # users split over two calls
    sa, ia = eng.top_k(user[:123].contiguous(), items, 100, ex[:123].contiguous())
    sb, ib = eng.top_k(user[123:].contiguous(), items, 100, ex[123:].contiguous())
    assert torch.equal(torch.cat([ia, ib]), i) and torch.equal(torch.cat([sa, sb]).view(torch.int32), s.view(torch.int32))
    # k = 50 is the prefix of k = 100
    s50, i50 = eng.top_k(user, items, 50, ex)
    assert torch.equal(i50, i[:, :50]) and torch.equal(s50.view(torch.int32), s[:, :50].view(torch.int32))
    # permuted catalogue rows: the same score bits per (user, item), the same sets where the k-th and (k+1)-th differ
    perm = torch.randperm(items.shape[0], device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel(), device=DEV)
    sp, ip = eng.top_k(user, items[perm].contiguous(), 101, inv[ex].contiguous())
    orig = perm[ip]
    s101, i101 = eng.top_k(user, items, 101, ex)
    sc_a = {(b, int(n)): int(v) for b in range(user.shape[0]) for n, v in zip(i101[b].tolist(), s101[b].view(torch.int32).tolist())}
    for b in range(user.shape[0]):
        for n, v in zip(orig[b].tolist(), sp[b].view(torch.int32).tolist()):
            if (b, n) in sc_a:
                assert sc_a[(b, n)] == v
        if s101[b, 99] != s101[b, 100]:
            assert set(orig[b, :100].tolist()) == set(i101[b, :100].tolist())


def _model(kind, tmp_path):
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    from pytorch_news_recommender_amd.model import nrms_hip, nrms_v1_hip
    torch.manual_seed(0)
    cfg = Config(kind)
    cfg.__nrms__()
    cfg.n_words, cfg.n_words_title, cfg.history_len, cfg.sample_size, cfg.max_candidate_size = 600, 12, 10, 4, 24
    cfg.word_embed_size, cfg.num_attention_heads, cfg.title_heads_num, cfg.query_vector_dim = 60, 6, 3, 32
    cfg.batch_size, cfg.dropout = 32, 0.2
    corpus = SyntheticMind(cfg, n_news=300, n_topics=4, seed=1)
    cls = nrms_hip.Model if kind == "nrms_v0" else nrms_v1_hip.Model
    model = cls(cfg, pretrained_word_embedding=corpus.embedding_table(cfg.word_embed_size)).to("cuda")
    samples, _ = corpus.eval_samples(100, max_shown=20)
    feed = DeviceFeed(cfg, samples, type=1, id2title_dict=corpus.id2title_dict, batch_size=cfg.batch_size, device=DEV)
    return cfg, model, feed


@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_v1"])
def test_model_recommend_matches_forward(kind, tmp_path):
    cfg, model, feed = _model(kind, tmp_path)
    model.train()                                   # recommend / encode_catalogue ignore the module's mode
    cat = model.encode_catalogue(feed.titles)
    model.eval()
    with torch.no_grad():
        ref = model.get_news_vector(feed.titles)
    assert cat.shape == (feed.titles.shape[0], cfg.word_embed_size)
    assert (cat - ref).abs().max().item() <= 1e-6
    model.train()
    k = 20
    for batch in feed:
        ids, scores = model.recommend(batch, k, cat)
        hist = batch["browsed_ids"]
        assert ids.shape == scores.shape == (hist.shape[0], k) and ids.dtype == torch.int64
        assert (ids > 0).all()
        assert not (ids.unsqueeze(2) == hist.unsqueeze(1)).any()
        model.eval()
        with torch.no_grad():
            fwd = model({"browsed_titles": batch["browsed_titles"], "browsed_ids": hist,
                         "candidate_titles": feed.titles.index_select(0, ids.view(-1)).view(ids.shape[0], k, -1),
                         "candidate_mask": torch.ones_like(ids, dtype=torch.uint8)})
        model.train()
        assert (fwd - scores).abs().max().item() <= 1e-5
        with pytest.raises(KeyError):
            model.recommend({"browsed_titles": batch["browsed_titles"]}, k, cat)


def test_train_eval_recommend_writes_one_line_per_impression(tmp_path):
    cfg, model, feed = _model("nrms_v0", tmp_path)
    out = train_eval.recommend(cfg, model, feed, feed.titles, 10, out_file=str(tmp_path / "rec.txt"))
    lines = open(out).read().splitlines()
    hist = feed.packed["hist"].cpu().numpy()
    assert len(lines) == feed.n
    for i, ln in enumerate(lines):
        m = re.fullmatch(r"(\d+) \[(\d+(?:,\d+)*)\]", ln)
        assert m and int(m.group(1)) == i + 1, ln
        ids = [int(v) for v in m.group(2).split(",")]
        assert len(ids) == 10 == len(set(ids)) and 0 not in ids and not set(ids) & set(hist[i].tolist())


def test_run_v0_recommend_flag(tmp_path):
    out = tmp_path / "rec.txt"
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "pytorch_news_recommender_amd.run_v0", "--model", "nrms_hip", "--dataset", "synthetic",
                        "--max_batches", "4", "--epochs", "1", "--synthetic_users", "256", "--batch_size", "64",
                        "--description", "T", "--data_path", str(tmp_path / "data"), "--save_path", str(tmp_path / "save"),
                        "--recommend", "10", "--recommend_out", str(out)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = out.read_text().splitlines()
    assert len(lines) == 1024                       # run_v0's synthetic dev split
    assert all(re.fullmatch(r"\d+ \[\d+(?:,\d+){9}\]", ln) for ln in lines)
