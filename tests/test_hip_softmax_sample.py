"""nrms_softmax_sample_dot on the GPU (negatives from the model's own softmax over the catalogue, include/nrms_hip.h): the
words and the perturbation against the restatement (tests/softmax_sample_ref.py), the selection bit for bit against keys formed
on the host from nrms_rank_dot's score bits and the hook's perturbation, every shape at which the kernels take another path,
independence of the batch, the statistics of the draw, the buffer contract, and the layers built on it (NRMSEngine.softmax_sample,
Model.sample_negatives, ClickFeed(negatives="adaptive"), run_v0 --negatives adaptive)."""
import ctypes as C

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.config import Config
from pytorch_news_recommender_amd.data_handler import ClickFeed, SyntheticMind
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine

from tests import softmax_sample_ref as ref
from tests.guarded import POISONS, Pool, assert_same_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SEED = 0xC0FFEE0123456789
_ENG = []


def _engine():
    if not _ENG:
        _ENG.append(NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), DEV))
    return _ENG[0]


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _noise(row_key, N, seed):
    """The hook: (words uint32 [B, N], gumbel float32 [B, N])."""
    key = _dev(row_key, torch.int64)
    B = key.numel()
    w = torch.zeros(B, N, dtype=torch.int32, device=DEV)
    g = torch.zeros(B, N, dtype=torch.float32, device=DEV)
    rc = _lib.load().nrms_softmax_sample_noise(B, C.c_int64(N), _lib.ptr(key), C.c_uint64(seed), _lib.ptr(w), _lib.ptr(g), _stream())
    _lib.check(rc, "nrms_softmax_sample_noise")
    return w.cpu().numpy().view(np.uint32), g.cpu().numpy()


def _sample(user, items, row_key, S, inv_t, seed, exclude=None):
    ids, keys = _engine().softmax_sample(_dev(user), _dev(items), _dev(row_key, torch.int64), S, inv_t, seed,
                                         _dev(exclude, torch.int64), return_keys=True)
    return ids.cpu().numpy(), keys.cpu().numpy()


def _host(scores, row_key, S, inv_t, seed, exclude=None):
    """The contract on the host: exact fp32 fma of the given score bits and the HOOK's perturbation bits, then (key desc, id asc)."""
    N = scores.shape[1]
    g = _noise(row_key, N, seed)[1] if N else np.zeros((len(row_key), 0), np.float32)
    return ref.sample(scores, row_key, S, inv_t, seed, exclude, g=g)


def _assert_exact(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.int32), want[1].view(np.int32))


def _int_data(B, N, d, seed, n_ex):
    """Small-integer rows: every score is exact in fp32 whatever the order of the chain, so the host's float64 product has
    nrms_topk_dot's bits; with inv_temperature a power of two the key's product is exact too."""
    rng = np.random.default_rng(seed)
    user = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    if N > 8:
        items[rng.choice(N, size=max(1, N // 97), replace=False)] = np.nan
    ex = None
    if n_ex:
        ex = rng.integers(0, max(N, 1), size=(B, n_ex))
        ex[:, 0] = -1
        if n_ex > 4:
            ex[:, 1], ex[:, 2], ex[:, 3] = N, 0, ex[:, 4]                  # out of range, id 0, a duplicate
    keys = rng.integers(0, 2 ** 48, size=B)
    scores = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32).reshape(B, N)
    return user, items, ex, keys, scores


# ---- 1. the perturbation -----------------------------------------------------------------------------------------------------------
ROW_KEYS = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 48 - 1], dtype=np.int64)


@pytest.mark.parametrize("seed", [0, SEED, 0xFFFFFFFFFFFFFFFF, 0x8000000080000000])
def test_words_are_bit_equal_to_the_restatement(seed):
    for N in (1, 3, 4, 5, 33, 257):
        w, _ = _noise(ROW_KEYS, N, seed)
        np.testing.assert_array_equal(w, ref.words(seed, ROW_KEYS, N), err_msg="N=%d" % N)


def test_gumbel_against_float64():
    """The device's g = -logf(-logf(u)) against the float64 restatement on the 65 536 x 8 words of the statistics case.  Bar: 4 x
    the fp32 restatement's own maximum error on the same words (numpy's float32 log: 5.44e-7, so the bar is 2.18e-6); the margin
    covers a device logf that is within 1 ulp but not numpy's.  Measured on an MI355X: 1.43e-6."""
    w, g = _noise(ref.STAT_KEYS, len(ref.STAT_SCORES), SEED)
    np.testing.assert_array_equal(w, ref.words(SEED, ref.STAT_KEYS, len(ref.STAT_SCORES)))
    g64 = ref.gumbel64(w)
    own = float(np.abs(ref.gumbel32(w).astype(np.float64) - g64).max())
    err = float(np.abs(g.astype(np.float64) - g64).max())
    print("max |g - g64|: device %.3e, fp32 restatement %.3e, bar %.3e" % (err, own, 4 * own))
    assert np.isfinite(g).all() and float(g.max()) < ref.G_MAX
    assert err <= 4 * own
    edge = np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], dtype=np.uint32)       # the extreme words, wherever they fall: |g| stays small
    assert np.abs(ref.gumbel32(edge)).max() < ref.G_MAX


# ---- 2. the selection, exact ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_case():
    """Real-valued rows, the score bits from nrms_rank_dot's target_scores for the same (user, item) pairs."""
    rng = np.random.default_rng(11)
    B, N, d = 33, 700, 300
    user = rng.standard_normal((B, d)).astype(np.float32)
    items = (rng.standard_normal((N, d)) * 0.2).astype(np.float32)
    items[[5, 77]] = np.nan
    keys = rng.integers(0, 2 ** 48, size=B)
    targets = np.broadcast_to(np.arange(N, dtype=np.int64), (B, N))
    _, sc = _engine().rank_of(_dev(user), _dev(items), _dev(targets, torch.int64))
    scores = sc.cpu().numpy()
    assert np.isneginf(scores[:, [5, 77]]).all() and np.isfinite(np.delete(scores, [5, 77], axis=1)).all()
    scores[:, [5, 77]] = np.nan                                     # (rank_dot reports a NaN score as -inf)
    ex = rng.integers(0, N, size=(B, 20))
    return user, items, keys, scores, ex


@pytest.mark.parametrize("inv_t", [0.0, 0.37, 1.0, 6.5])
@pytest.mark.parametrize("S", [4, 100])
def test_selection_is_exact_on_rank_dot_score_bits(real_case, S, inv_t):
    user, items, keys, scores, ex = real_case
    got = _sample(user, items, keys, S, inv_t, SEED, ex)
    _assert_exact(got, _host(scores, keys, S, inv_t, SEED, ex))
    assert (got[0] >= 0).all() and not np.isin(got[0], [5, 77]).any()
    assert (np.diff(got[1].astype(np.float64), axis=1) <= 0).all()               # Plackett-Luce order: keys descending


SHAPES = [  # B, N, d, S, n_exclude
    (1, 0, 8, 4, 0), (31, 1, 1, 1, 1), (33, 3, 31, 4, 0), (65, 5, 32, 5, 64), (33, 33, 33, 64, 65), (31, 513, 300, 193, 1),
    (65, 5000, 8, 256, 65), (33, 5000, 300, 4, 64), (1, 513, 32, 64, 0), (31, 255, 33, 256, 0), (33, 193, 31, 193, 1),
    (65, 129, 1, 193, 0), (33, 63, 8, 64, 1), (1, 33, 300, 5, 65)]


@pytest.mark.parametrize("B,N,d,S,n_ex", SHAPES)
def test_selection_at_every_shape(B, N, d, S, n_ex):
    """N in {0, 1, S - 1, S, 33, one block step + 1 (513 at 8 waves, 129 at 2), 3 slices (5000)}; S 193 crosses to the 2-wave
    kernel; exclude lists in LDS (<= 64) and in global memory (65)."""
    user, items, ex, keys, scores = _int_data(B, N, d, seed=B + N + d + S, n_ex=n_ex)
    for inv_t in (0.5, 2.0):
        got = _sample(user, items, keys, S, inv_t, SEED + S, ex)
        want = _host(scores, keys, S, inv_t, SEED + S, ex)
        _assert_exact(got, want)
    if N < S:
        assert (got[0][:, N:] == -1).all() and np.isneginf(got[1][:, N:]).all()


def test_excluded_nan_and_infinite_items():
    user, items, _, keys, _ = _int_data(33, 40, 16, seed=9, n_ex=0)
    user[:, 0], items[:, 0] = 1.0, 0.0
    items[[3, 17, 29], 0] = np.inf                                   # three +inf scores per user: the smaller id first
    items[21, 0] = -np.inf
    items[8] = np.nan
    with np.errstate(invalid="ignore"):
        scores = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)
    assert np.isposinf(scores[:, [3, 17, 29]]).all() and np.isnan(scores[:, 8]).all()
    S = 8
    got = _sample(user, items, keys, S, 1.0, SEED)
    _assert_exact(got, _host(scores, keys, S, 1.0, SEED))
    assert (got[0][:, :3] == [3, 17, 29]).all() and np.isposinf(got[1][:, :3]).all() and not (got[0] == 8).any()
    # inv_temperature 0: inf * 0 is NaN, so only the finite scores are drawn, uniformly
    got0 = _sample(user, items, keys, 40, 0.0, SEED)
    _assert_exact(got0, _host(scores, keys, 40, 0.0, SEED))
    n_finite = np.isfinite(scores).sum(1)                           # (the integer data carries one more NaN row)
    assert (n_finite <= 40 - 5).all() and ((got0[0] >= 0).sum(1) == n_finite).all() and not np.isin(got0[0], [3, 17, 29, 21, 8]).any()
    # all but S - 2 items excluded: two padding slots
    keep = np.array([1, 4, 10, 22, 30, 39])
    ex = np.broadcast_to(np.setdiff1d(np.arange(40), keep), (33, 34)).copy()
    gotx = _sample(user, items, keys, S, 1.0, SEED, ex)
    _assert_exact(gotx, _host(scores, keys, S, 1.0, SEED, ex))
    assert (np.sort(gotx[0][:, :6], axis=1) == keep).all() and (gotx[0][:, 6:] == -1).all() and np.isneginf(gotx[1][:, 6:]).all()


# ---- 3. a row's draw depends on the row alone ----------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch():
    rng = np.random.default_rng(21)
    n, N, d, S = 70, 1200, 60, 6
    user = rng.standard_normal((n, d)).astype(np.float32)
    items = rng.standard_normal((N, d)).astype(np.float32)
    keys = rng.integers(0, 2 ** 48, size=n)
    ex = rng.integers(0, N, size=(n, 9))
    base = _sample(user, items, keys, S, 0.8, SEED, ex)
    perm = rng.permutation(n)
    moved = _sample(user[perm], items, keys[perm], S, 0.8, SEED, ex[perm])
    _assert_exact(moved, (base[0][perm], base[1][perm]))
    for chunk in (1, 31, 33):
        parts = [_sample(user[c:c + chunk], items, keys[c:c + chunk], S, 0.8, SEED, ex[c:c + chunk]) for c in range(0, n, chunk)][:4]
        got = tuple(np.concatenate([p[j] for p in parts]) for j in (0, 1))
        _assert_exact(got, (base[0][:len(got[0])], base[1][:len(got[0])]))
    other = _sample(user, items, keys, S, 0.8, SEED + 1, ex)
    assert (other[0] != base[0]).mean() > 0.5                                      # the seed moves the draw
    rekeyed = _sample(user, items, keys + 1, S, 0.8, SEED, ex)
    assert (rekeyed[0] != base[0]).mean() > 0.5                                    # and so does the row key
    # a longer catalogue leaves the keys of the first N items alone: the draw over a prefix is the prefix's draw
    few = _sample(user, items[:300], keys, S, 0.8, SEED, None)
    more = _sample(user, items, keys, 256, 0.8, SEED, None)
    for b in range(0, n, 7):
        inside = more[0][b][more[0][b] < 300][:S]
        assert len(inside) == S and inside.tolist() == few[0][b].tolist()


# ---- 4. the statistics of the fused draw ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv_t", ref.STAT_INV_T)
def test_device_draws_from_the_softmax_in_plackett_luce_order(inv_t):
    """tests/test_softmax_sample_host.py's case through the fused kernel: 65 536 users, 8 item rows whose dots are the listed
    scores; first picks and judged ordered pairs within 6 sd; inv_temperature 0 is the uniform draw."""
    n = len(ref.STAT_SCORES)
    user = np.zeros((ref.STAT_ROWS, 8), dtype=np.float32)
    user[:, 2] = 1.0
    items = np.zeros((n, 8), dtype=np.float32)
    items[:, 2] = ref.STAT_SCORES
    ids, keys = _sample(user, items, ref.STAT_KEYS, 2, inv_t, SEED)
    assert (ids >= 0).all() and (ids[:, 0] != ids[:, 1]).all() and (keys[:, 0] >= keys[:, 1]).all()
    worst, judged = ref.worst_deviation(ids, ref.STAT_SCORES, inv_t)
    print("inv_temperature %g: worst deviation %.2f sd over 8 first picks and %d pairs" % (inv_t, worst, judged))
    assert worst <= 6.0


# ---- 5. the buffer contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,d,S,n_ex", [(33, 3000, 60, 5, 3), (5, 700, 33, 200, 70)])
def test_buffers_between_guard_bands_and_poisoned_workspace(B, N, d, S, n_ex):
    user, items, ex, keys, _ = _int_data(B, N, d, seed=S, n_ex=n_ex)
    lib = _lib.load()
    need = int(lib.nrms_softmax_sample_dot_workspace_bytes(B, C.c_int64(N), d, S, n_ex))
    assert need > 0
    ins = [_dev(user), _dev(items), _dev(keys, torch.int64), _dev(ex, torch.int64)]

    def run(poison, with_keys=True):
        P = Pool(poison)
        ids, ky, ws = P.elems("ids", B * S, torch.int64), P.elems("keys", B * S, torch.float32), P.new("workspace", need)
        rc = lib.nrms_softmax_sample_dot(B, C.c_int64(N), d, S, _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), C.c_float(1.5),
                                         C.c_uint64(SEED), _lib.ptr(ins[3]), n_ex, ids.ptr, ky.ptr if with_keys else None, ws.ptr,
                                         C.c_size_t(need), _stream())
        _lib.check(rc, "nrms_softmax_sample_dot")
        P.intact("nrms_softmax_sample_dot")
        if not with_keys:
            assert (ky.numpy().view(np.uint8) == poison).all()                        # a null keys pointer: nothing written
        return {"ids": ids.numpy((B, S)), "keys": ky.numpy((B, S))}

    runs = {p: run(p) for p in POISONS}
    assert_same_bits(runs, "nrms_softmax_sample_dot")
    _assert_exact((runs[POISONS[0]]["ids"], runs[POISONS[0]]["keys"]), _sample(user, items, keys, S, 1.5, SEED, ex))
    assert np.array_equal(run(POISONS[0], with_keys=False)["ids"], runs[POISONS[0]]["ids"])
    P = Pool(POISONS[0])
    ids, ws = P.elems("ids", B * S, torch.int64), P.new("workspace", need)
    snap = P.snapshot()
    rc = lib.nrms_softmax_sample_dot(B, C.c_int64(N), d, S, _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), C.c_float(1.5),
                                     C.c_uint64(SEED), _lib.ptr(ins[3]), n_ex, ids.ptr, None, ws.ptr, C.c_size_t(need - 1), _stream())
    assert rc != 0 and b"workspace" in lib.nrms_last_error()
    P.assert_unchanged(snap, "nrms_softmax_sample_dot (undersized)")


# ---- 6. the model and the feed -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    from pytorch_news_recommender_amd.model import nrms_hip
    torch.manual_seed(0)
    cfg = Config("nrms_v0")
    cfg.__nrms__()
    cfg.n_words, cfg.n_words_title, cfg.history_len, cfg.sample_size = 800, 12, 10, 4
    cfg.word_embed_size, cfg.num_attention_heads, cfg.query_vector_dim = 60, 6, 32
    cfg.batch_size, cfg.dropout, cfg.precision = 32, 0.2, "bf16x3"
    corpus = SyntheticMind(cfg, n_news=500, n_topics=4, seed=1)
    user_ptr, clicks = corpus.click_log(300, min_clicks=3, max_clicks=40)
    model = nrms_hip.Model(cfg, pretrained_word_embedding=corpus.embedding_table(cfg.word_embed_size)).to("cuda").train()
    kw = dict(id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, seed=77, negatives="adaptive", temperature=0.7,
              device=DEV)

    def feed(attach=True, **more):
        f = ClickFeed(cfg, user_ptr, clicks, **dict(kw, **more))
        if attach:
            f.attach_scorer(model)
        return f
    return cfg, model, feed, user_ptr, clicks


def _drawn(feed, epoch=0):
    feed.draw(feed.epoch_seed(epoch))
    lo, hi = feed.row0, feed.row0 + feed.n
    return {k: v[lo:hi].cpu().numpy() for k, v in feed.packed.items()}


def test_adaptive_feed_draws_legal_rows_that_depend_on_the_row_and_the_weights_only(world):
    cfg, model, feed, user_ptr, clicks = world
    S = cfg.sample_size
    f = feed(batch_size=32)
    with pytest.raises(RuntimeError, match="attach_scorer"):
        feed(attach=False).draw(1)
    p = _drawn(f)
    cand, clen = p["cand"], p["clen"]
    assert cand.shape == (f.n_samples, S + 1) and f.n_samples > 2000
    row_user, set_ptr, set_news = f.row_user.cpu().numpy(), f.set_ptr.cpu().numpy(), f.set_news.cpu().numpy()
    assert np.array_equal(cand[:, 0], f.row_pos.cpu().numpy())
    assert f.n_short == int((S + 1 - clen).sum()) == 0 and (clen == S + 1).all()         # 500 news, sets of at most 40
    for r in range(0, f.n_samples, 13):
        own = set_news[set_ptr[row_user[r]]:set_ptr[row_user[r] + 1]]
        neg = cand[r, 1:clen[r]]
        assert (neg > 0).all() and len(set(neg.tolist())) == len(neg) and not np.isin(neg, own).any(), r
        assert cand[r, 0] in own
    # the same bytes for another batch size, another chunking, a shuffled feed and two ranks
    for other in (feed(batch_size=512), feed(batch_size=32, shuffle=True)):
        assert all(np.array_equal(_drawn(other)[k], p[k]) for k in p)
    small = feed(batch_size=32)
    small.draw_chunk = 257
    assert all(np.array_equal(_drawn(small)[k], p[k]) for k in p)
    halves = [_drawn(feed(batch_size=32, rank=r, world=2)) for r in range(2)]
    per = f.n_samples // 2
    assert all(np.array_equal(np.concatenate([h[k] for h in halves]), p[k][:2 * per]) for k in p)
    # it is Model.sample_negatives called by hand
    rows = torch.arange(100, 164, device=DEV)
    ex = [set_news[set_ptr[u]:set_ptr[u + 1]] for u in row_user[100:164]]
    width = max(len(e) for e in ex)
    exm = np.array([np.concatenate([e, np.full(width - len(e), -1)]) for e in ex])
    cat = model.encode_catalogue(f.titles)
    ids = model.sample_negatives({"browsed_ids": f._rows_of("hist", rows)}, f.row_key[100:164], S, cat, 0.7, f.epoch_seed(0), exclude=_dev(exm, torch.int64))
    assert np.array_equal(ids.cpu().numpy(), cand[100:164, 1:])
    # without an exclude matrix the browsed ids are excluded, and only they
    free = model.sample_negatives({"browsed_ids": f._rows_of("hist", rows)}, f.row_key[100:164], 256, cat, 0.7, f.epoch_seed(0)).cpu().numpy()
    hist = f._rows_of("hist", rows).cpu().numpy()
    for b in range(64):
        got = free[b][free[b] >= 0]
        assert len(got) == 256 == len(set(got.tolist())) and not np.isin(got, hist[b]).any() and (got > 0).all()
    # the epoch moves the draw; so do the weights
    e1 = _drawn(f, 1)
    assert (e1["cand"][:, 1:] != cand[:, 1:]).mean() > 0.5 and np.array_equal(e1["cand"][:, 0], cand[:, 0])
    saved = [q.detach().clone() for q in model.parameters()]
    with torch.no_grad():
        for q in model.parameters():
            q.mul_(1.5)
    moved = _drawn(f)
    with torch.no_grad():
        for q, v in zip(model.parameters(), saved):
            q.copy_(v)
    assert (moved["cand"][:, 1:] != cand[:, 1:]).mean() > 0.05
    assert all(np.array_equal(_drawn(f)[k], p[k]) for k in p)                      # and the old weights give the old draw
    # batches: the mask follows clen, candidate_logq is refused
    b = next(iter(feed(batch_size=64)))
    assert b["candidate_ids"].shape == (64, S + 1) and bool(b["candidate_mask"].all())
    with pytest.raises(KeyError, match="no fixed q"):
        b["candidate_logq"]


def test_adaptive_feed_counts_the_slots_it_cannot_fill(world):
    """A catalogue of 12 news and users who clicked most of it: fewer than S eligible news leave empty slots, which are masked
    out and counted."""
    cfg, model, _, _, _ = world
    corpus = SyntheticMind(cfg, n_news=12, n_topics=2, seed=2)
    user_ptr, clicks = corpus.click_log(20, min_clicks=10, max_clicks=30)
    f = ClickFeed(cfg, user_ptr, clicks, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, seed=3, negatives="adaptive",
                  device=DEV, batch_size=16)
    f.attach_scorer(model)
    p = _drawn(f)
    S = cfg.sample_size
    sets = np.diff(f.set_ptr.cpu().numpy())[f.row_user.cpu().numpy()]
    want = np.minimum(S, 12 - sets)
    assert np.array_equal(p["clen"], 1 + want) and f.n_short == int((S - want).sum()) > 0
    assert all((p["cand"][r, p["clen"][r]:] == 0).all() for r in range(len(want)))
    b = next(iter(f))
    assert np.array_equal(b["candidate_mask"].cpu().numpy(), (np.arange(S + 1)[None, :] < p["clen"][:16, None]).astype(np.uint8))


def test_run_v0_with_adaptive_negatives_is_reproducible(tmp_path, monkeypatch):
    """2 epochs over the click log of 200 synthetic users, held-out clicks ranked at the end: finite losses, the same twice."""
    from pytorch_news_recommender_amd import run_v0
    monkeypatch.chdir(tmp_path)
    common = ["--model", "nrms_hip", "--dataset", "synthetic", "--negatives", "adaptive", "--negative_temperature", "0.5", "--synthetic_users",
              "200", "--num_workers", "0", "--description", "T", "--data_path", str(tmp_path / "data_processed"), "--retrieval_metrics", "10",
              "--epochs", "2"]
    runs = [run_v0.main(common + ["--save_path", str(tmp_path / ("save%d" % r))])["losses"] for r in range(2)]
    assert len(runs[0]) >= 4 and np.isfinite(runs[0]).all() and runs[0] == runs[1]
