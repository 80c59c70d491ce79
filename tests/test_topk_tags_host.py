"""CPU-only checks of the per-user tag sets on the catalogue (include/nrms_hip.h nrms_topk_dot_tagged / nrms_rank_dot_tagged): the
numpy restatement against a brute force, pack_tag_mask's bit layout, the four symbols in the header, in _lib.SIGNATURES and in the
library, the workspace queries, the models' methods and refusals, the loops' keywords, ClickFeed.clicked_tags on a hand-written
log and run_v0's --only_categories / --mute_categories checks.  Parity is unpinned: the reference has no catalogue retrieval."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval
from pytorch_news_recommender_amd.engine import pack_tag_mask

from tests import topk_tags_ref as ref
from tests.test_topk_bias_host import _Prior, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrms_topk_dot_tagged_workspace_bytes", "nrms_topk_dot_tagged", "nrms_rank_dot_tagged_workspace_bytes", "nrms_rank_dot_tagged")
F = np.float32
I32_MAX = 2 ** 31 - 1


# ---- 1: the restatement ------------------------------------------------------------------------------------------------------
def _brute(s, bias, tag, n_tags, allow, ex, k, tg):
    """The contract item by item, in Python: a selection sort over the eligible items by (score descending, id ascending)."""
    B, N = s.shape
    ids = np.full((B, k), -1, dtype=np.int64)
    sc = np.full((B, k), -np.inf, dtype=F)
    rk = np.zeros(tg.shape, dtype=np.int32)
    rs = np.full(tg.shape, -np.inf, dtype=F)
    for b in range(B):
        el = []
        for n in range(N):
            v = F(s[b, n]) if bias is None else F(F(s[b, n]) + F(bias[n]))
            if v == 0:
                v = F(0.0)
            t = int(tag[n])
            if not (0 <= t < n_tags and bool(allow[b, t])) or np.isnan(v):
                continue
            if ex is not None and n in [int(x) for x in ex[b]]:
                continue
            el.append((v, n))
        before = lambda a, c: a[0] > c[0] or (a[0] == c[0] and a[1] < c[1])
        rest = list(el)
        for j in range(min(k, len(el))):
            best = rest[0]
            for e in rest[1:]:
                if before(e, best):
                    best = e
            rest.remove(best)
            ids[b, j], sc[b, j] = best[1], best[0]
        for j, t in enumerate(tg[b]):
            mine = [e for e in el if e[1] == t]
            if mine:
                rk[b, j] = 1 + sum(before(e, mine[0]) for e in el)
                rs[b, j] = mine[0][0]
    return (ids, sc), (rk, rs)


@pytest.mark.parametrize("seed,with_bias", [(0, False), (1, True), (2, True)])
def test_ref_against_brute_force(seed, with_bias):
    rng = np.random.default_rng(seed)
    B, N, k, T, n_tags = 7, 40, 9, 6, 5
    s = rng.integers(-3, 4, size=(B, N)).astype(F)                   # ties everywhere, -0.0 among them
    s[0, 3] = -0.0
    s[1, 5] = np.nan
    bias = None
    if with_bias:
        bias = (rng.integers(-4, 5, size=N) * 0.5).astype(F)
        bias[[2, 11]] = np.nan
        bias[7] = -np.inf
    tag = rng.integers(0, n_tags, size=N).astype(np.int64)
    tag[4], tag[9], tag[13] = -1, n_tags, I32_MAX
    allow = rng.random((B, n_tags)) < 0.5
    allow[0], allow[1] = True, False
    ex = rng.integers(-1, N + 1, size=(B, 5))
    tg = rng.integers(-1, N + 1, size=(B, T))
    tg[:, 0] = 4                                                     # untagged: never served
    want_k, want_r = _brute(s, bias, tag, n_tags, allow, ex, k, tg)
    got_k, got_r = ref.topk(s, bias, tag, n_tags, allow, ex, k), ref.ranks(s, bias, tag, n_tags, allow, ex, tg)
    for g, w in zip(got_k + got_r, want_k + want_r):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert (got_k[0][1] == -1).all() and (got_k[0][0] >= 0).all()    # the empty set, the full one
    assert (got_r[0][:, 0] == 0).all() and not np.isin([4, 9, 13], got_k[0]).any()
    # topk and ranks against each other: the served ids rank 1, 2, ... with the same score bits
    rk, rs = ref.ranks(s, bias, tag, n_tags, allow, ex, got_k[0])
    live = got_k[0] >= 0
    assert (rk[live] == np.broadcast_to(np.arange(1, k + 1), (B, k))[live]).all() and (rk[~live] == 0).all()
    assert rs.tobytes() == got_k[1].tobytes()


def test_ref_consequences():
    s = np.array([[5.0, 4.0, 3.0, 2.0, 1.0]], dtype=F)
    tag = np.array([0, 1, 2, 1, -1])
    allow = np.array([[False, True, False]])
    ids, _ = ref.topk(s, None, tag, 3, allow, None, 5)
    assert ids.tolist() == [[1, 3, -1, -1, -1]]
    rk, rs = ref.ranks(s, None, tag, 3, allow, None, np.array([[0, 1, 2, 3, 4, -1, 5]]))
    assert rk.tolist() == [[0, 1, 0, 2, 0, 0, 0]] and rs[0, 0] == -np.inf
    assert ref.topk(s, None, tag, 3, np.ones((1, 3), dtype=bool), None, 5)[0].tolist() == [[0, 1, 2, 3, -1]]      # -1 is open to nobody
    # (b): the tags as a bias of 0 where open and NaN where closed, through the restatement of the biased call
    from tests import topk_bias_ref
    b1 = ref.tags_as_bias(None, tag, 3, allow[0], 5)
    assert np.isnan(b1).tolist() == [True, False, True, False, True]
    assert topk_bias_ref.topk(s, b1, None, 5)[0].tolist() == ids.tolist()
    # tagged ranks of eligible targets never exceed the untagged ones
    rng = np.random.default_rng(3)
    s = rng.normal(size=(6, 50)).astype(F)
    tag = rng.integers(0, 8, size=50)
    allow = rng.random((6, 8)) < 0.5
    tg = rng.integers(0, 50, size=(6, 10))
    rt = ref.ranks(s, None, tag, 8, allow, None, tg)[0]
    r0 = ref.ranks(s, None, tag, 8, np.ones_like(allow), None, tg)[0]
    assert (rt > 0).any() and (rt == 0).any() and (rt[rt > 0] <= r0[rt > 0]).all()


# ---- 2: the bit layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tags", [1, 31, 32, 33, 64, 294, 512])
def test_pack_tag_mask_bit_for_bit(n_tags):
    rng = np.random.default_rng(n_tags)
    a = rng.random((6, n_tags)) < 0.5
    a[0], a[1] = True, False
    a[2] = False
    a[2, [0, min(31, n_tags - 1), min(32, n_tags - 1), n_tags - 1]] = True
    got = pack_tag_mask(torch.from_numpy(a))
    W = (n_tags + 31) // 32
    assert got.dtype == torch.int32 and tuple(got.shape) == (6, W)
    words = got.numpy().view(np.uint32)
    assert np.array_equal(words, ref.pack(a))
    for b in range(6):
        for t in range(32 * W):                                      # bit t & 31 of word t >> 5; nothing past n_tags
            assert ((int(words[b, t >> 5]) >> (t & 31)) & 1) == (int(a[b, t]) if t < n_tags else 0), (b, t)
    assert np.array_equal(ref.pack(a, 0xFFFFFFFF)[:, :W - 1], words[:, :W - 1])
    if n_tags % 32:
        assert (ref.pack(a, 0xFFFFFFFF)[:, -1] >> np.uint32(n_tags % 32) == np.uint32((1 << (32 - n_tags % 32)) - 1)).all()
    with pytest.raises(ValueError, match="allow"):
        pack_tag_mask(torch.from_numpy(a).to(torch.int32))


# ---- 3: the symbols ----------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_signatures_and_library():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, name + " is not declared in include/nrms_hip.h"
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(2).count(",") + 1, name
    # the tagged calls take item_tag, n_tags and allow beside the biased calls' arguments; the queries are the same
    assert len(_lib.SIGNATURES["nrms_topk_dot_tagged"][1]) == len(_lib.SIGNATURES["nrms_topk_dot_biased"][1]) + 3
    assert len(_lib.SIGNATURES["nrms_rank_dot_tagged"][1]) == len(_lib.SIGNATURES["nrms_rank_dot_biased"][1]) + 3
    assert _lib.SIGNATURES["nrms_topk_dot_tagged_workspace_bytes"] == _lib.SIGNATURES["nrms_topk_dot_workspace_bytes"]
    assert _lib.SIGNATURES["nrms_rank_dot_tagged_workspace_bytes"] == _lib.SIGNATURES["nrms_rank_dot_workspace_bytes"]
    lib = _lib.load()                                                # binds every symbol: a missing export raises here
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for word in ("open to nobody", "PARITY UNPINNED, the reference has no catalogue retrieval", "(a)", "(b)", "(c)", "(d)", "(e)",
                 "topk_dot_tagged: ...", "rank_dot_tagged: ...", "1 <= n_tags <= 512"):
        assert word in text, word


def test_tagged_queries_and_host_side_refusals():
    """The queries equal the untagged ones; bad arguments are refused on the host (no GPU is needed to be told so)."""
    import ctypes as C
    lib = _lib.load()
    for B, N, d, k in ((70, 5000, 40, 10), (512, 130000, 300, 100), (1, 0, 1, 1), (0, 5, 3, 256)):
        q = lib.nrms_topk_dot_tagged_workspace_bytes(B, C.c_int64(N), d, k)
        assert q == lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k) > 0
        r = lib.nrms_rank_dot_tagged_workspace_bytes(B, C.c_int64(N), d, min(k, 32), 70)
        assert r == lib.nrms_rank_dot_workspace_bytes(B, C.c_int64(N), d, min(k, 32), 70) > 0
    assert lib.nrms_topk_dot_tagged_workspace_bytes(70, C.c_int64(5000), 40, 257) == 0
    assert lib.nrms_rank_dot_tagged_workspace_bytes(70, C.c_int64(5000), 40, 33, 0) == 0
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)
    for tag, n_tags, allow, word in ((None, 19, p, b"item_tag is null"), (p, 19, None, b"allow is null"),
                                     (odd, 19, p, b"item_tag must be 4-byte aligned"), (p, 19, odd, b"allow must be 4-byte aligned"),
                                     (p, 0, p, b"n_tags must be in [1, 512]"), (p, 513, p, b"n_tags must be in [1, 512]")):
        assert lib.nrms_topk_dot_tagged(2, C.c_int64(4), 2, 2, p, p, None, tag, n_tags, allow, None, 0, p, p, p, C.c_size_t(4096), None) == _lib.NRMS_EINVAL
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_tagged: ") and word in msg, msg
        assert lib.nrms_rank_dot_tagged(2, C.c_int64(4), 2, 2, p, p, None, tag, n_tags, allow, p, None, 0, p, p, p, C.c_size_t(4096), None) == _lib.NRMS_EINVAL
        msg = lib.nrms_last_error()
        assert msg.startswith(b"rank_dot_tagged: ") and word in msg, msg
    assert lib.nrms_topk_dot_tagged(2, C.c_int64(4), 2, 2, p, p, None, p, 19, p, None, 0, p, p, p, C.c_size_t(8), None) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_rank_dot_tagged(2, C.c_int64(4), 2, 2, p, p, None, p, 19, p, p, None, 0, p, p, p, C.c_size_t(8), None) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_topk_dot_tagged(0, C.c_int64(4), 2, 2, None, None, None, None, 19, None, None, 0, None, None, None, C.c_size_t(0), None) == _lib.NRMS_OK
    assert lib.nrms_rank_dot_tagged(0, C.c_int64(4), 2, 2, None, None, None, None, 19, None, None, None, 0, None, None, None, C.c_size_t(0), None) == _lib.NRMS_OK


# ---- 4: the models -----------------------------------------------------------------------------------------------------------
MODELS = ("nrms_hip", "nrms_v1_hip", "nrms_naml_hip", "nrms_bert_hip", "hierec_hip", "graph_hip")


def test_all_six_models_have_both_methods_with_one_signature():
    from importlib import import_module
    sigs = {"recommend_tagged": set(), "rank_targets_tagged": set()}
    for name in MODELS:
        M = import_module("pytorch_news_recommender_amd.model." + name).Model
        for meth in sigs:
            sigs[meth].add(str(inspect.signature(getattr(M, meth))))
        assert M.CATALOGUE_TAGS is (name not in ("hierec_hip", "graph_hip")), name
    assert sigs["recommend_tagged"] == {"(self, batch, k, catalogue, item_tag, allow, exclude_history=True, *, item_bias=None)"}
    assert sigs["rank_targets_tagged"] == {"(self, batch, targets, catalogue, item_tag, allow, exclude_history=True, *, item_bias=None)"}
    from pytorch_news_recommender_amd.model import nrms_hip
    assert nrms_hip.pack_tag_mask is pack_tag_mask                   # the module-level helper callers import beside Model
    # the methods beside them are as they were
    assert list(inspect.signature(nrms_hip.Model.recommend).parameters)[-3:] == ["coarse", "coarse_shortlist", "return_certified"]


def test_models_that_cannot_serve_a_tag_set_refuse_in_their_own_words():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    t, a = torch.zeros(3, dtype=torch.int32), torch.ones(1, 2, dtype=torch.bool)
    for mod, who, why in ((hierec_hip, "hierec", "nrms_topk_grouped_dot"), (graph_hip, "graph", "click graph")):
        with pytest.raises(NotImplementedError, match=who + ": recommend_tagged is not available") as e:
            mod.Model.recommend_tagged(None, {}, 5, None, t, a)
        assert why in str(e.value)
        with pytest.raises(NotImplementedError, match=who + ": rank_targets_tagged is not available") as e:
            mod.Model.rank_targets_tagged(None, {}, None, None, t, a, item_bias=torch.zeros(3))
        assert why in str(e.value)
        # and exactly what they said before for the calls beside them
        with pytest.raises(NotImplementedError, match=who + ": rank_targets is not available"):
            mod.Model.rank_targets(None, {}, None, None)
        with pytest.raises(_lib.NrmsError, match="item_bias"):
            mod.Model.rank_targets(None, {}, None, None, item_bias=torch.zeros(3))
    with pytest.raises(NotImplementedError, match="graph: recommend is not available"):
        graph_hip.Model.recommend(None, {}, 5, None)
    assert hierec_hip.Model.CATALOGUE_RANKING is False


def test_model_tag_rows():
    """nrms_v0's own check, before anything touches the device."""
    from pytorch_news_recommender_amd.model import nrms_hip
    cat = torch.zeros(5, 4)
    t, a = torch.arange(5, dtype=torch.int64), torch.ones(2, 40, dtype=torch.bool)
    f = nrms_hip.Model._tag_rows
    rows, n_tags, allow = f(t, a, cat, 2, "recommend_tagged")
    assert rows.tolist() == [1, 2, 3, 4] and n_tags == 40 and allow is a          # rows 1.. like the catalogue's
    assert f(t.to(torch.int32), pack_tag_mask(a), cat, 2, "recommend_tagged")[1] == 64         # a packed set stands for 32 W tags
    for bad_t, bad_a in ((t[:-1], a), (t.float(), a), (t.tolist(), a), (t, a[:1]), (t, a.view(80)), (t, a.float()), (t, a.tolist())):
        with pytest.raises(_lib.NrmsError, match="item_tag|allow"):
            f(bad_t, bad_a, cat, 2, "rank_targets_tagged")


# ---- 5: the loops ------------------------------------------------------------------------------------------------------------
class _Tagged(_Prior):
    def recommend_tagged(self, batch, k, catalogue, item_tag, allow, exclude_history=True, *, item_bias=None):
        self.tagged.append(("recommend_tagged", item_tag, allow, item_bias))
        return _Stub.recommend(self, batch, k, catalogue, exclude_history)

    def rank_targets_tagged(self, batch, targets, catalogue, item_tag, allow, exclude_history=True, *, item_bias=None):
        self.tagged.append(("rank_targets_tagged", item_tag, allow, item_bias))
        rk, _ = _Stub.rank_targets(self, batch, targets, catalogue, exclude_history)
        t = item_tag[targets.clamp(min=0)]
        return torch.where(allow.gather(1, t), rk, torch.zeros_like(rk)), None             # a closed target: rank 0


def test_loops_hand_every_sample_its_tag_set(tmp_path):
    titles = torch.zeros(20, 3, dtype=torch.int64)
    batches = [{"candidate_ids": torch.tensor([[3, 4, 5], [6, 7, 0]]), "browsed_ids": torch.zeros(2, 2, dtype=torch.int64)},
               {"candidate_ids": torch.tensor([[8, 9, 1]]), "browsed_ids": torch.zeros(1, 2, dtype=torch.int64)}]
    labels = [[0, 1, 0], [1, 1], [0, 0, 1]]
    tag = torch.arange(20, dtype=torch.int64) % 3                    # targets 4 (tag 1); 6 (0), 7 (1); 1 (1)
    allow = torch.tensor([[True, True, False], [True, False, False], [False, False, True]])
    rec = lambda m, **kw: train_eval.recommend(None, m, batches, titles, 4, out_file=str(tmp_path / "a.txt"), **kw)
    ev = lambda m, **kw: train_eval.evaluate_retrieval(None, m, batches, titles, labels, ks=(1,), verbose=False, **kw)
    for call, meth in ((rec, "recommend_tagged"), (ev, "rank_targets_tagged")):
        m = _Tagged()
        m.tagged = []
        p = torch.ones(20)
        call(m, item_tag=tag, allow_tags=allow.numpy() if call is ev else allow, item_bias=p)
        assert [c[0] for c in m.tagged] == [meth] * 2 and all(c[1] is tag and c[3] is p for c in m.tagged)
        assert [c[2].tolist() for c in m.tagged] == [allow[:2].tolist(), allow[2:].tolist()]
        assert all(c[2].dtype == torch.bool for c in m.tagged)
        m.tagged, m.calls = [], []
        call(m)                                                      # absent: no new keyword, the calls from before
        assert m.tagged == [] and len(m.calls) == 2
        call(_Stub())                                                # ... so a model from before the tags still runs
        with pytest.raises(AttributeError, match=meth):
            call(_Stub(), item_tag=tag, allow_tags=allow)            # given, they reach the model and fail there, not silently
        for kw in (dict(item_tag=tag), dict(allow_tags=allow)):
            with pytest.raises(ValueError, match="go together"):
                call(m, **kw)
        with pytest.raises(ValueError, match="allow_tags rows"):
            call(m, item_tag=tag, allow_tags=allow[:2])
        with pytest.raises(ValueError, match="allow_tags must be bool"):
            call(m, item_tag=tag, allow_tags=allow.long())
    # a held-out target closed by its tag counts as skipped, and is reported
    m = _Tagged()
    m.tagged = []
    res = ev(m, item_tag=tag, allow_tags=allow)
    assert res["n_targets"] == 2 and res["n_skipped"] == 2 and res["n_closed"] == 2           # 4 and 6 are open, 7 and 1 closed
    assert "n_closed" not in ev(_Tagged())
    # the combinations the tagged kernels do not have are refused by name
    t32, req = torch.arange(20, dtype=torch.int32), np.array([1, 2, 3])
    for kw, word in ((dict(diversity=0.5), "diversity"), (dict(coarse=True), "coarse"), (dict(explain=3), "explain"),
                     (dict(item_time=t32, request_time=req, window_span=5), "window_span")):
        with pytest.raises(ValueError, match=word):
            rec(m, item_tag=tag, allow_tags=allow, **kw)
    for kw, word in ((dict(nll_temperatures=(1.0,)), "nll_temperatures"), (dict(item_time=t32, request_time=req, window_span=5), "window_span")):
        with pytest.raises(ValueError, match=word):
            ev(m, item_tag=tag, allow_tags=allow, **kw)
    assert list(inspect.signature(train_eval.recommend).parameters)[-3:] == ["item_tag", "allow_tags", "explain"]
    assert list(inspect.signature(train_eval.evaluate_retrieval).parameters)[-2:] == ["item_tag", "allow_tags"]


# ---- 6: ClickFeed ------------------------------------------------------------------------------------------------------------
def test_clicked_tags_on_a_hand_written_log():
    from tests.test_topk_window_host import _hand_log
    feed, user_ptr, clicks, _ = _hand_log(click_time=None)
    # news 1 .. 7 carry tags 0, 1, 2, 0, 1, 3, -1; news 6 (tag 3) is clicked once, as user 1's held-out click
    tag = np.array([9, 0, 1, 2, 0, 1, 3, -1])
    got = feed.clicked_tags(torch.from_numpy(tag), 4)
    assert got.dtype == torch.bool and tuple(got.shape) == (3, 4) and got.device == feed.device
    want = np.zeros((3, 4), dtype=bool)
    for u in range(3):
        for n in clicks[user_ptr[u]:user_ptr[u + 1] - 1]:            # the training part: everything but the last click
            if 0 <= tag[n] < 4:
                want[u, tag[n]] = True
    assert got.numpy().tolist() == want.tolist()
    assert not got[1, 3] and want[0].tolist() == [True, True, True, False]        # the held-out click's tag is not counted
    assert feed.heldout_users().tolist() == [0, 1, 2] and len(feed.heldout_samples()[0]) == 3
    assert feed.clicked_tags(tag, 2).numpy().tolist() == want[:, :2].tolist()     # tags past n_tags set nothing
    with pytest.raises(ValueError, match="item_tag"):
        feed.clicked_tags(tag[:-1], 4)
    with pytest.raises(ValueError, match="n_tags"):
        feed.clicked_tags(tag, 0)


# ---- 7: the CLI's checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,want", [
    (["--recommend", "5", "--only_categories", "own"], ("own", None)),
    (["--retrieval_metrics", "10,100", "--only_categories", "3,5"], ((3, 5), None)),
    (["--recommend", "5", "--mute_categories", "2"], (None, (2,))),
    (["--recommend", "5", "--only_categories", "own", "--mute_categories", "2,4"], ("own", (2, 4))),
    (["--negatives", "catalogue", "--recommend", "5", "--popularity_prior", "0.5", "--only_categories", "own"], ("own", None)),
    (["--model", "nrms_v1", "--recommend", "5", "--only_categories", "own"], ("own", None)),
    (["--model", "nrms_naml", "--retrieval_metrics", "10", "--mute_categories", "1"], (None, (1,))),
    (["--model", "nrms_bert", "--retrieval_metrics", "10", "--only_categories", "1"], ((1,), None)),
    (["--recommend", "5"], (None, None)),                                                          # no flag: nothing to check
    (["--only_categories", "own"], "--only_categories"),                                           # nothing to apply it to
    (["--mute_categories", "2"], "--mute_categories"),
    (["--recommend", "5", "--only_categories", "sports"], "--only_categories"),
    (["--recommend", "5", "--mute_categories", "own"], "--mute_categories"),
    (["--recommend", "5", "--mute_categories", "-1"], "--mute_categories"),
    (["--model", "hierec", "--recommend", "5", "--only_categories", "own"], "--only_categories"),
    (["--model", "graph", "--recommend", "5", "--mute_categories", "2"], "--mute_categories"),
    (["--negatives", "catalogue", "--recommend", "5", "--catalogue_window", "100", "--only_categories", "own"], "--catalogue_window"),
    (["--recommend", "5", "--coarse_catalogue", "--only_categories", "own"], "--coarse_catalogue"),
    (["--recommend_deep", "500", "--retrieval_metrics", "10", "--only_categories", "own"], "--recommend_deep"),
    (["--recommend", "5", "--sections", "category", "--mute_categories", "2"], "--sections"),
    (["--recommend", "5", "--diversity", "0.5", "--only_categories", "own"], "--diversity"),
    (["--retrieval_metrics", "10", "--retrieval_nll", "1.0", "--only_categories", "own"], "--retrieval_nll"),
    (["--recommend", "5", "--explain", "3", "--mute_categories", "2"], "--explain"),
])
def test_check_tag_args(argv, want):
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(["--dataset", "synthetic"] + ([] if "--model" in argv else ["--model", "nrms_hip"]) + argv)
    if isinstance(want, tuple):
        assert run_v0.check_tag_args(args) == want
    else:
        with pytest.raises(SystemExit) as e:
            run_v0.check_tag_args(args)
        flag = "--only_categories" if "--only_categories" in argv else "--mute_categories"
        assert flag in str(e.value) and want in str(e.value)
