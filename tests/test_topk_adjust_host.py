"""CPU-only checks of the per-user score adjustments on the catalogue (include/nrms_hip.h nrms_topk_dot_adjusted /
nrms_rank_dot_adjusted): the numpy restatement against a brute force, the four symbols in the header, in _lib.SIGNATURES and in the
library, the workspace queries and host-side refusals, the models' methods and refusals, the loops' keyword, seen_adjustment and
ClickFeed's seen log on a hand-written log, SyntheticMind.seen_log and run_v0's --seen_discount checks.  Parity is unpinned: the
reference has no catalogue retrieval."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval
from pytorch_news_recommender_amd.data_handler import SyntheticMind, seen_adjustment

from tests import topk_adjust_ref as ref
from tests.test_topk_bias_host import _Prior, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrms_topk_dot_adjusted_workspace_bytes", "nrms_topk_dot_adjusted", "nrms_rank_dot_adjusted_workspace_bytes",
       "nrms_rank_dot_adjusted")
F = np.float32


# ---- 1: the restatement ------------------------------------------------------------------------------------------------------
def _brute(s, bias, aid, adl, ex, k, tg):
    """The contract pair by pair, in Python: the lowest slot by a forward search, one float32 add, and a selection sort over the
    eligible items by (score descending, id ascending)."""
    B, N = s.shape
    ids = np.full((B, k), -1, dtype=np.int64)
    sc = np.full((B, k), -np.inf, dtype=F)
    rk = np.zeros(tg.shape, dtype=np.int32)
    rs = np.full(tg.shape, -np.inf, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            el = []
            for n in range(N):
                v = F(s[b, n]) if bias is None else F(F(s[b, n]) + F(bias[n]))
                for e in range(aid.shape[1]):
                    if int(aid[b, e]) == n:
                        v = F(v + F(adl[b, e]))
                        break
                if v == 0:
                    v = F(0.0)
                if np.isnan(v) or (ex is not None and n in [int(x) for x in ex[b]]):
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


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("seed,with_bias", [(0, False), (1, True), (2, True)])
def test_ref_against_brute_force(seed, with_bias):
    rng = np.random.default_rng(seed)
    B, N, E, k, T = 5, 40, 9, 12, 6
    s = (rng.integers(-8, 9, size=(B, N)) * 0.5).astype(F)
    s[0, 3] = -0.0
    s[1, 5] = np.nan
    bias = None
    if with_bias:
        bias = (rng.integers(-8, 9, size=N) * 0.25).astype(F)
        bias[7], bias[9] = np.nan, -np.inf
    aid = rng.integers(0, N, size=(B, E)).astype(np.int64)
    adl = (rng.integers(-12, 13, size=(B, E)) * 0.25).astype(F)
    aid[:, 0], aid[:, 1], aid[:, 2] = -1, N, 2 ** 63 - 1
    aid[:, 4] = aid[:, 3]                                            # one id twice: the lower slot counts
    adl[:, 4] = adl[:, 3] + 5.0
    adl[0, 5], adl[1, 5], adl[2, 5], adl[3, 5] = np.nan, np.inf, -np.inf, 0.0
    ex = rng.integers(-1, N + 1, size=(B, 4)).astype(np.int64)
    ex[:, 0] = aid[:, 6]                                             # excluded and adjusted
    tg = rng.integers(-1, N + 1, size=(B, T)).astype(np.int64)
    tg[:, 0], tg[:, 1], tg[:, 2] = aid[:, 3], aid[:, 5], aid[:, 6]
    want_k, want_r = _brute(s, bias, aid, adl, ex, k, tg)
    got_k, got_r = ref.topk(s, bias, aid, adl, ex, k), ref.ranks(s, bias, aid, adl, ex, tg)
    for g, w in zip(got_k + got_r, want_k + want_r):
        np.testing.assert_array_equal(_bits(g), _bits(w))
    assert (got_r[0][:, 2] == 0).all()                               # excluded and adjusted: excluded
    # no slots, E = 0 and all-empty slots are one and the same
    none = ref.topk(s, bias, None, None, ex, k)
    for a, d in ((np.zeros((B, 0), dtype=np.int64), np.zeros((B, 0), dtype=F)), (np.full((B, 3), -1), np.ones((B, 3), dtype=F))):
        for g, w in zip(ref.topk(s, bias, a, d, ex, k), none):
            np.testing.assert_array_equal(_bits(g), _bits(w))
    # consequence (b): a row is the biased call with the deltas scattered
    for b in range(B):
        b1 = ref.adjust_as_bias(aid[b], adl[b], N)
        for g, w in zip(ref.topk(s[b:b + 1], None, aid[b:b + 1], adl[b:b + 1], ex[b:b + 1], k), ref.topk(s[b:b + 1], b1, None, None, ex[b:b + 1], k)):
            np.testing.assert_array_equal(_bits(g), _bits(w))


# ---- 2: the symbols ----------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_signatures_and_library():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, name + " is not declared in include/nrms_hip.h"
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(2).count(",") + 1, name
    # the adjusted calls take adj_ids, adj_delta and n_adjust beside the biased calls' arguments; the queries are the same
    assert len(_lib.SIGNATURES["nrms_topk_dot_adjusted"][1]) == len(_lib.SIGNATURES["nrms_topk_dot_biased"][1]) + 3
    assert len(_lib.SIGNATURES["nrms_rank_dot_adjusted"][1]) == len(_lib.SIGNATURES["nrms_rank_dot_biased"][1]) + 3
    assert _lib.SIGNATURES["nrms_topk_dot_adjusted_workspace_bytes"] == _lib.SIGNATURES["nrms_topk_dot_workspace_bytes"]
    assert _lib.SIGNATURES["nrms_rank_dot_adjusted_workspace_bytes"] == _lib.SIGNATURES["nrms_rank_dot_workspace_bytes"]
    lib = _lib.load()                                                # binds every symbol: a missing export raises here
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for word in ("LOWEST e", "PARITY UNPINNED, the reference\n * has no catalogue retrieval", "(a)", "(b)", "(c)", "(d)", "(e)",
                 "topk_dot_adjusted: ...", "rank_dot_adjusted: ...", "#define NRMS_ADJ_MAX 256", "never folded into the chain"):
        assert word in text, word


def test_adjusted_queries_and_host_side_refusals():
    """The queries equal the unadjusted ones; bad arguments are refused on the host (no GPU is needed to be told so)."""
    import ctypes as C
    lib = _lib.load()
    for B, N, d, k in ((70, 5000, 40, 10), (512, 130000, 300, 100), (1, 0, 1, 1), (0, 5, 3, 256)):
        q = lib.nrms_topk_dot_adjusted_workspace_bytes(B, C.c_int64(N), d, k)
        assert q == lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k) > 0
        r = lib.nrms_rank_dot_adjusted_workspace_bytes(B, C.c_int64(N), d, min(k, 32), 70)
        assert r == lib.nrms_rank_dot_workspace_bytes(B, C.c_int64(N), d, min(k, 32), 70) > 0
    assert lib.nrms_topk_dot_adjusted_workspace_bytes(70, C.c_int64(5000), 40, 257) == 0
    assert lib.nrms_rank_dot_adjusted_workspace_bytes(70, C.c_int64(5000), 40, 33, 0) == 0
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)
    for aid, adl, E, word in ((None, p, 4, b"adj_ids is null"), (p, None, 4, b"adj_delta is null"),
                              (odd, p, 4, b"adj_ids must be 8-byte aligned"), (p, odd, 4, b"adj_delta must be 4-byte aligned"),
                              (p, p, -1, b"n_adjust must be in [0, 256]"), (p, p, 257, b"n_adjust must be in [0, 256]")):
        assert lib.nrms_topk_dot_adjusted(2, C.c_int64(4), 2, 2, p, p, None, aid, adl, E, None, 0, p, p, p, C.c_size_t(4096), None) == _lib.NRMS_EINVAL
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_adjusted: ") and word in msg, msg
        assert lib.nrms_rank_dot_adjusted(2, C.c_int64(4), 2, 2, p, p, None, aid, adl, E, p, None, 0, p, p, p, C.c_size_t(4096), None) == _lib.NRMS_EINVAL
        msg = lib.nrms_last_error()
        assert msg.startswith(b"rank_dot_adjusted: ") and word in msg, msg
    for kw_d, word in ((0, b"d must be"),):
        assert lib.nrms_topk_dot_adjusted(2, C.c_int64(4), kw_d, 2, p, p, None, p, p, 4, None, 0, p, p, p, C.c_size_t(4096), None) == _lib.NRMS_EINVAL
        assert word in lib.nrms_last_error()
    assert lib.nrms_topk_dot_adjusted(2, C.c_int64(4), 2, 2, p, p, None, p, p, 4, None, 0, p, p, p, C.c_size_t(8), None) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_rank_dot_adjusted(2, C.c_int64(4), 2, 2, p, p, None, p, p, 4, p, None, 0, p, p, p, C.c_size_t(8), None) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_topk_dot_adjusted(0, C.c_int64(4), 2, 2, None, None, None, None, None, 4, None, 0, None, None, None, C.c_size_t(0), None) == _lib.NRMS_OK
    assert lib.nrms_rank_dot_adjusted(0, C.c_int64(4), 2, 2, None, None, None, None, None, 4, None, None, 0, None, None, None, C.c_size_t(0), None) == _lib.NRMS_OK


# ---- 3: the models -----------------------------------------------------------------------------------------------------------
MODELS = ("nrms_hip", "nrms_v1_hip", "nrms_naml_hip", "nrms_bert_hip", "hierec_hip", "graph_hip")


def test_all_six_models_have_both_methods_with_one_signature():
    from importlib import import_module
    sigs = {"recommend_adjusted": set(), "rank_targets_adjusted": set()}
    for name in MODELS:
        M = import_module("pytorch_news_recommender_amd.model." + name).Model
        for meth in sigs:
            sigs[meth].add(str(inspect.signature(getattr(M, meth))))
        assert M.CATALOGUE_ADJUST is (name not in ("hierec_hip", "graph_hip")), name
    assert sigs["recommend_adjusted"] == {"(self, batch, k, catalogue, adjust, exclude_history=True, *, item_bias=None)"}
    assert sigs["rank_targets_adjusted"] == {"(self, batch, targets, catalogue, adjust, exclude_history=True, *, item_bias=None)"}
    from pytorch_news_recommender_amd.model import nrms_hip
    # the methods beside them are as they were
    assert list(inspect.signature(nrms_hip.Model.recommend).parameters)[-3:] == ["coarse", "coarse_shortlist", "return_certified"]
    assert "adjust" not in inspect.signature(nrms_hip.Model.recommend_tagged).parameters
    assert "adjust" not in inspect.signature(nrms_hip.Model.rank_targets).parameters


def test_models_that_cannot_adjust_refuse_in_their_own_words():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    adj = (torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2))
    for mod, who, why in ((hierec_hip, "hierec", "nrms_topk_grouped_dot"), (graph_hip, "graph", "click graph")):
        with pytest.raises(NotImplementedError, match=who + ": recommend_adjusted is not available") as e:
            mod.Model.recommend_adjusted(None, {}, 5, None, adj)
        assert why in str(e.value)
        with pytest.raises(NotImplementedError, match=who + ": rank_targets_adjusted is not available") as e:
            mod.Model.rank_targets_adjusted(None, {}, None, None, adj, item_bias=torch.zeros(3))
        assert why in str(e.value)


def test_model_adjust_rows():
    """nrms_v0's own check, before anything touches the device: news id n is row n - 1, id 0 and ids beyond the catalogue are empty."""
    from pytorch_news_recommender_amd.model import nrms_hip
    cat = torch.zeros(5, 4)
    f = nrms_hip.Model._adjust_rows
    ids, delta = f((torch.tensor([[0, 1, 4, 5, 9]]), np.array([[1.0, 2.0, 3.0, 4.0, 5.0]])), cat, 1, "recommend_adjusted")
    assert ids.tolist() == [[-1, 0, 3, 4, 8]] and ids.dtype == torch.int64           # (rows >= N - 1 = 4 name nothing: cat[1:] has 4)
    assert delta.dtype == torch.float32 and delta.tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0]]
    good = (torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3))
    for bad in (good[0], (good[0],), (good[0][:1], good[1]), (good[0], good[1][:, :2]), (good[0].view(6), good[1].view(6)),
                (torch.zeros(2, 257, dtype=torch.int64), torch.zeros(2, 257))):
        with pytest.raises(_lib.NrmsError, match="adjust"):
            f(bad, cat, 2, "rank_targets_adjusted")


# ---- 4: the loops ------------------------------------------------------------------------------------------------------------
class _Adjusted(_Prior):
    def recommend_adjusted(self, batch, k, catalogue, adjust, exclude_history=True, *, item_bias=None):
        self.adjusted.append(("recommend_adjusted", adjust, item_bias))
        return _Stub.recommend(self, batch, k, catalogue, exclude_history)

    def rank_targets_adjusted(self, batch, targets, catalogue, adjust, exclude_history=True, *, item_bias=None):
        self.adjusted.append(("rank_targets_adjusted", adjust, item_bias))
        return _Stub.rank_targets(self, batch, targets, catalogue, exclude_history)


def test_loops_hand_every_sample_its_slots(tmp_path):
    titles = torch.zeros(20, 3, dtype=torch.int64)
    batches = [{"candidate_ids": torch.tensor([[3, 4, 5], [6, 7, 0]]), "browsed_ids": torch.zeros(2, 2, dtype=torch.int64)},
               {"candidate_ids": torch.tensor([[8, 9, 1]]), "browsed_ids": torch.zeros(1, 2, dtype=torch.int64)}]
    labels = [[0, 1, 0], [1, 1], [0, 0, 1]]
    ids = torch.tensor([[4, 0], [6, 7], [1, 19]])
    delta = torch.tensor([[-1.0, 0.0], [-0.5, -1.5], [2.0, float("nan")]])
    rec = lambda m, **kw: train_eval.recommend(None, m, batches, titles, 4, out_file=str(tmp_path / "a.txt"), **kw)
    ev = lambda m, **kw: train_eval.evaluate_retrieval(None, m, batches, titles, labels, ks=(1,), verbose=False, **kw)
    for call, meth in ((rec, "recommend_adjusted"), (ev, "rank_targets_adjusted")):
        m = _Adjusted()
        m.adjusted = []
        p = torch.ones(20)
        call(m, adjust=(ids.numpy(), delta.numpy()) if call is ev else (ids, delta), item_bias=p)
        assert [c[0] for c in m.adjusted] == [meth] * 2 and all(c[2] is p for c in m.adjusted)
        assert [c[1][0].tolist() for c in m.adjusted] == [ids[:2].tolist(), ids[2:].tolist()]
        assert m.adjusted[0][1][1].tolist() == delta[:2].tolist() and m.adjusted[1][1][1][0, 0] == 2.0
        assert all(c[1][0].dtype == torch.int64 and c[1][1].dtype == torch.float32 for c in m.adjusted)
        m.adjusted, m.calls = [], []
        call(m)                                                      # absent: no new keyword, the calls from before
        assert m.adjusted == [] and len(m.calls) == 2
        call(_Stub())                                                # ... so a model from before the adjustments still runs
        with pytest.raises(AttributeError, match=meth):
            call(_Stub(), adjust=(ids, delta))                       # given, they reach the model and fail there, not silently
        with pytest.raises(ValueError, match="adjust rows"):
            call(m, adjust=(ids[:2], delta[:2]))
        for bad in (ids, (ids, delta[:, :1]), (ids.float(), delta), (ids, delta.long())):
            with pytest.raises(ValueError, match="adjust must be"):
                call(m, adjust=bad)
    # the combinations the adjusted kernels do not have are refused by name
    m = _Adjusted()
    m.adjusted = []
    t32, req = torch.arange(20, dtype=torch.int32), np.array([1, 2, 3])
    tag, allow = torch.zeros(20, dtype=torch.int64), torch.ones(3, 2, dtype=torch.bool)
    for kw, word in ((dict(diversity=0.5), "diversity"), (dict(coarse=True), "coarse"), (dict(explain=3), "explain"),
                     (dict(item_time=t32, request_time=req, window_span=5), "window_span"),
                     (dict(item_tag=tag, allow_tags=allow), "item_tag / allow_tags"),
                     (dict(item_tag=tag, tag_caps=torch.ones(2, dtype=torch.int32)), "tag_caps")):
        with pytest.raises(ValueError, match=word + " does not go with adjust"):
            rec(m, adjust=(ids, delta), **kw)
    for kw, word in ((dict(nll_temperatures=(1.0,)), "nll_temperatures"), (dict(item_time=t32, request_time=req, window_span=5), "window_span"),
                     (dict(item_tag=tag, allow_tags=allow), "item_tag / allow_tags")):
        with pytest.raises(ValueError, match=word + " does not go with adjust"):
            ev(m, adjust=(ids, delta), **kw)
    assert m.adjusted == []
    assert inspect.signature(train_eval.recommend).parameters["adjust"].default is None
    assert inspect.signature(train_eval.evaluate_retrieval).parameters["adjust"].default is None


# ---- 5: the data layer -------------------------------------------------------------------------------------------------------
def test_seen_adjustment_on_a_hand_written_log():
    # user 0: news 5 three times, 2 twice, 9 and 3 once; user 1: nothing; user 2: news 7 once; user 3: 4, 4, 1, 1, 8
    ptr = np.array([0, 7, 7, 8, 13])
    ids = np.array([5, 2, 9, 5, 3, 2, 5,   7,   4, 1, 4, 1, 8])
    a, d = seen_adjustment(ptr, ids, 0.5, 4)
    assert a.dtype == torch.int64 and d.dtype == torch.float32 and tuple(a.shape) == tuple(d.shape) == (4, 4)
    assert a.tolist() == [[5, 2, 3, 9], [0, 0, 0, 0], [7, 0, 0, 0], [1, 4, 8, 0]]     # most seen first, ties by the smaller id
    assert d.tolist() == [[-1.5, -1.0, -0.5, -0.5], [0.0] * 4, [-0.5, 0.0, 0.0, 0.0], [-1.0, -1.0, -0.5, 0.0]]
    a2, d2 = seen_adjustment(torch.from_numpy(ptr), torch.from_numpy(ids), 2.0, 2)     # more distinct news than slots
    assert a2.tolist() == [[5, 2], [0, 0], [7, 0], [1, 4]] and d2.tolist() == [[-6.0, -4.0], [0.0, 0.0], [-2.0, 0.0], [-4.0, -4.0]]
    a0, d0 = seen_adjustment(ptr, ids, 0.0, 4)
    assert a0.tolist() == a.tolist() and (d0 == 0).all()                               # beta 0: the same slots, no discount
    e_a, e_d = seen_adjustment(np.array([0, 0, 0]), np.array([], dtype=np.int64), 1.0, 3)
    assert e_a.tolist() == [[0, 0, 0]] * 2 and e_d.tolist() == [[0.0] * 3] * 2         # a log in which nobody saw anything
    assert tuple(seen_adjustment(ptr, ids, 1.0, 0)[0].shape) == (4, 0)
    for bad_ptr, bad_slots, word in ((np.array([0, 7, 6, 8, 13]), 4, "seen_ptr"), (np.array([0, 7, 7, 8, 12]), 4, "seen_ptr"),
                                     (ptr, 257, "max_slots"), (ptr, -1, "max_slots")):
        with pytest.raises(ValueError, match=word):
            seen_adjustment(bad_ptr, ids, 1.0, bad_slots)


def test_click_feed_serves_the_slots_of_its_users():
    from tests.test_topk_window_host import _hand_log
    seen = (np.array([0, 3, 3, 5]), np.array([7, 5, 7, 7, 1]))          # user 0: 7 twice, 5; user 1: nothing; user 2: 7, 1
    feed, user_ptr, clicks, _ = _hand_log(click_time=None, seen=seen)
    a, d = feed.seen_adjustment(0.25, 3)
    assert a.device == feed.device and a.tolist() == [[7, 5, 0], [0, 0, 0], [1, 7, 0]]
    assert d.tolist() == [[-0.5, -0.25, 0.0], [0.0, 0.0, 0.0], [-0.25, -0.25, 0.0]]
    a2, d2 = feed.seen_adjustment(0.25, 3, users=[2, 0])                # a batch's users, in its order
    assert a2.tolist() == [a[2].tolist(), a[0].tolist()] and d2.tolist() == [d[2].tolist(), d[0].tolist()]
    held, _ = feed.seen_adjustment(1.0, 2, users=feed.heldout_users())
    assert tuple(held.shape) == (len(feed.heldout_samples()[0]), 2)
    plain, _, _, _ = _hand_log(click_time=None)
    with pytest.raises(ValueError, match="no seen log"):
        plain.seen_adjustment(1.0, 2)
    for bad in ((np.array([0, 3, 5]), seen[1]), (np.array([0, 3, 3, 4]), seen[1]), seen[0], (seen[0], np.array([7, 5, 7, 7, -1]))):
        with pytest.raises(ValueError, match="seen"):
            _hand_log(click_time=None, seen=bad)


def _cfg():
    from tests.test_topk_window_host import _cfg as cfg
    return cfg()


def test_seen_log_leaves_every_other_stream_alone():
    a, b = SyntheticMind(_cfg(), n_news=300, seed=3), SyntheticMind(_cfg(), n_news=300, seed=3)
    ptr_a, clicks_a = a.click_log(20)
    seen_ptr, seen_ids = b.seen_log(ptr_a, clicks_a, n_seen=10, seed=0)               # drawn BEFORE b's click log
    ptr_b, clicks_b = b.click_log(20)
    assert ptr_a.tolist() == ptr_b.tolist() and clicks_a.tolist() == clicks_b.tolist()
    again = b.seen_log(ptr_a, clicks_a, n_seen=10, seed=0)
    assert again[0].tolist() == seen_ptr.tolist() and again[1].tolist() == seen_ids.tolist()
    other = b.seen_log(ptr_a, clicks_a, n_seen=10, seed=1)
    assert other[1].tolist() != seen_ids.tolist()
    assert a.click_log(5)[1].tolist() == b.click_log(5)[1].tolist()                   # ... and the stream goes on in step
    assert seen_ptr.dtype == np.int64 and seen_ptr[0] == 0 and seen_ptr[-1] == seen_ids.size and (np.diff(seen_ptr) <= 10).all()
    assert seen_ids.size > 20 and seen_ids.min() >= 1 and seen_ids.max() <= 300
    for u in range(20):                                                               # shown and NOT clicked
        assert not set(seen_ids[seen_ptr[u]:seen_ptr[u + 1]].tolist()) & set(clicks_a[ptr_a[u]:ptr_a[u + 1]].tolist())


# ---- 6: the CLI's checks -----------------------------------------------------------------------------------------------------
CAT = ["--negatives", "catalogue"]


@pytest.mark.parametrize("argv,want", [
    (CAT + ["--recommend", "5", "--seen_discount", "0.5"], (0.5, 32)),
    (CAT + ["--retrieval_metrics", "10,100", "--seen_discount", "0", "--seen_slots", "256"], (0.0, 256)),
    (["--negatives", "adaptive", "--recommend", "5", "--popularity_prior", "0.5", "--seen_discount", "1"], (1.0, 32)),
    (CAT + ["--model", "nrms_v1", "--recommend", "5", "--seen_discount", "0.25", "--seen_slots", "1"], (0.25, 1)),
    (CAT + ["--model", "nrms_naml", "--retrieval_metrics", "10", "--seen_discount", "0.5"], (0.5, 32)),
    (CAT + ["--model", "nrms_bert", "--retrieval_metrics", "10", "--seen_discount", "0.5"], (0.5, 32)),
    (CAT + ["--recommend", "5"], None),                                                            # no flag: nothing to check
    (CAT + ["--seen_discount", "0.5"], "--recommend"),                                             # nothing to apply it to
    (CAT + ["--recommend", "5", "--seen_slots", "8"], "--seen_discount"),
    (CAT + ["--recommend", "5", "--seen_discount", "nan"], "finite"),
    (CAT + ["--recommend", "5", "--seen_discount", "0.5", "--seen_slots", "0"], "--seen_slots"),
    (CAT + ["--recommend", "5", "--seen_discount", "0.5", "--seen_slots", "257"], "--seen_slots"),
    (["--recommend", "5", "--seen_discount", "0.5"], "seen log"),                                  # no click log, no seen log
    (CAT + ["--model", "hierec", "--recommend", "5", "--seen_discount", "0.5"], "hierec"),
    (CAT + ["--model", "graph", "--recommend", "5", "--seen_discount", "0.5"], "graph"),
    (CAT + ["--recommend", "5", "--catalogue_window", "100", "--seen_discount", "0.5"], "--catalogue_window"),
    (CAT + ["--recommend", "5", "--coarse_catalogue", "--seen_discount", "0.5"], "--coarse_catalogue"),
    (CAT + ["--recommend_deep", "500", "--retrieval_metrics", "10", "--seen_discount", "0.5"], "--recommend_deep"),
    (CAT + ["--recommend", "5", "--sections", "category", "--seen_discount", "0.5"], "--sections"),
    (CAT + ["--recommend", "5", "--diversity", "0.5", "--seen_discount", "0.5"], "--diversity"),
    (CAT + ["--retrieval_metrics", "10", "--retrieval_nll", "1.0", "--seen_discount", "0.5"], "--retrieval_nll"),
    (CAT + ["--recommend", "5", "--explain", "3", "--seen_discount", "0.5"], "--explain"),
    (CAT + ["--recommend", "5", "--only_categories", "own", "--seen_discount", "0.5"], "--only_categories"),
    (CAT + ["--recommend", "5", "--mute_categories", "2", "--seen_discount", "0.5"], "--mute_categories"),
    (CAT + ["--recommend", "5", "--max_per_category", "2", "--seen_discount", "0.5"], "--max_per_category"),
])
def test_check_seen_args(argv, want):
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(["--dataset", "synthetic"] + ([] if "--model" in argv else ["--model", "nrms_hip"]) + argv)
    if not isinstance(want, str):
        assert run_v0.check_seen_args(args) == want
    else:
        with pytest.raises(SystemExit) as e:
            run_v0.check_seen_args(args)
        assert "--seen_" in str(e.value) and want in str(e.value)
