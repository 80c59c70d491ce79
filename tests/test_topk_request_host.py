"""The request calls on the host (no GPU): tests/topk_request_ref.py held against itself, a brute-force sort and the single-part
refs; the lattice data of the GPU test checked for empty cases; the new symbols; and the Python layers with recording fakes: keyword
routing, per-batch slicing, both-or-neither errors, the refusals of HieRec and the graph model, --combine_filters parsing and the old
refusals without the flag."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, run_v0, train_eval

from tests import topk_adjust_ref, topk_request_cases as cases, topk_request_ref as ref, topk_tags_ref, topk_window_ref
from tests.test_topk_bias_host import _Prior, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrms_topk_dot_request_workspace_bytes", "nrms_topk_dot_request", "nrms_rank_dot_request_workspace_bytes",
       "nrms_rank_dot_request")


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def _key(s):
    """The order-preserving integer of a float32 score, -0.0 as +0.0 (the kernels' entry, restated)."""
    u = int(np.float32(0.0 if s == 0.0 else s).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _brute(s, bias, parts, ex, k, tg, after):
    """Python loops and one sort per user: nothing shared with the ref but the statement of the contract."""
    B, N = s.shape
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=np.float32)
    rk = np.zeros(tg.shape, dtype=np.int32)
    rs = np.full(tg.shape, -np.inf, dtype=np.float32)
    for b in range(B):
        rows = []
        for n in range(N):
            v = np.float32(s[b, n])
            if bias is not None:
                v = np.float32(v + np.float32(bias[n]))
            if parts.adj_ids is not None:
                for e in range(parts.adj_ids.shape[1]):
                    if parts.adj_ids[b, e] == n:
                        v = np.float32(v + np.float32(parts.adj_delta[b, e]))
                        break
            if np.isnan(v) or (ex is not None and n in ex[b]):
                continue
            if parts.window is not None and not (int(parts.window[b, 0]) <= int(parts.item_time[n]) < int(parts.window[b, 1])):
                continue
            if parts.allow is not None and not (0 <= parts.item_tag[n] < parts.n_tags and parts.allow[b, parts.item_tag[n]]):
                continue
            rows.append((-_key(v), n, v))
        rows.sort()
        for j, t in enumerate(tg[b]):
            hit = [i for i, r in enumerate(rows) if r[1] == t]
            if hit:
                rk[b, j], rs[b, j] = hit[0] + 1, (np.float32(0.0) if rows[hit[0]][2] == 0.0 else rows[hit[0]][2])
        if after is not None and after[1][b] != ref.PAGE_BEGIN:
            if after[1][b] < 0 or np.isnan(after[0][b]):
                rows = []
            else:
                cur = (-_key(after[0][b]), int(after[1][b]))
                rows = [r for r in rows if (r[0], r[1]) > cur]
        for j, r in enumerate(rows[:k]):
            ids[b, j], out[b, j] = r[1], (np.float32(0.0) if r[2] == 0.0 else r[2])
    return (ids, out), (rk, rs)


# ---- 1: the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2, 3])
def test_ref_against_brute_force(case):
    B, N, d, k, T, n_tags, E, n_ex, with_bias = cases.CASES[case]
    user, items, s, bias, parts, after, ex, tg = cases.lattice(*cases.CASES[case])
    rows = slice(0, 9)                                               # the brute force is slow: nine users are enough
    cut = lambda x: x if x is None or np.ndim(x) == 0 or np.shape(x)[0] != B else x[rows]
    sub = ref.Parts(*[cut(x) for x in parts])
    aft = (after[0][rows], after[1][rows])
    for subset in cases.SUBSETS + [(), ("window",), ("tags",), ("adjust",), ("cursor",)]:
        p, a = cases.select(sub, aft, subset)
        want_k, want_r = _brute(s[rows], bias, p, cut(ex), k, tg[rows], a)
        for g, w in zip(ref.topk(s[rows], bias, p, cut(ex), k, a), want_k):
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=str(subset))
        for g, w in zip(ref.ranks(s[rows], bias, p, cut(ex), tg[rows]), want_r):
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=str(subset))


def test_topk_and_ranks_agree():
    """The ids topk serves (no cursor) get ranks 1, 2, ... from ranks, and a page after the j-th column starts at column j + 1."""
    shape = cases.CASES[4]
    user, items, s, bias, parts, after, ex, tg = cases.lattice(*shape)
    for subset in cases.RANK_SUBSETS:
        p, _ = cases.select(parts, None, subset)
        ids, sc = ref.topk(s, bias, p, ex, 40)
        rk, rs = ref.ranks(s, bias, p, ex, ids)
        np.testing.assert_array_equal(rk, np.where(ids >= 0, np.arange(1, 41)[None, :], 0))
        np.testing.assert_array_equal(_bits(rs), _bits(sc))
        page = ref.topk(s, bias, p, ex, 20, (sc[:, 19], ids[:, 19]))
        np.testing.assert_array_equal(page[0], ids[:, 20:])
        np.testing.assert_array_equal(_bits(page[1]), _bits(sc[:, 20:]))


def test_each_part_alone_is_its_own_ref():
    shape = cases.CASES[3]
    B, N, d, k, T = shape[:5]
    user, items, s, bias, parts, after, ex, tg = cases.lattice(*shape)
    single = {
        "window": (lambda: topk_window_ref.topk(s, bias, parts.item_time, parts.window, ex, k),
                   lambda: topk_window_ref.ranks(s, bias, parts.item_time, parts.window, ex, tg)),
        "tags": (lambda: topk_tags_ref.topk(s, bias, parts.item_tag, parts.n_tags, parts.allow, ex, k),
                 lambda: topk_tags_ref.ranks(s, bias, parts.item_tag, parts.n_tags, parts.allow, ex, tg)),
        "adjust": (lambda: topk_adjust_ref.topk(s, bias, parts.adj_ids, parts.adj_delta, ex, k),
                   lambda: topk_adjust_ref.ranks(s, bias, parts.adj_ids, parts.adj_delta, ex, tg)),
    }
    for name, (want_k, want_r) in single.items():
        p, _ = cases.select(parts, None, (name,))
        for g, w in zip(ref.topk(s, bias, p, ex, k), want_k()):
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=name)
        for g, w in zip(ref.ranks(s, bias, p, ex, tg), want_r()):
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=name)
    # no part at all: the adjusted ref without slots, which is the biased contract
    for g, w in zip(ref.topk(s, bias, ref.Parts(), ex, k), topk_adjust_ref.topk(s, bias, None, None, ex, k)):
        np.testing.assert_array_equal(_bits(g), _bits(w))
    # all parts neutral by value: the same
    for g, w in zip(ref.topk(s, bias, ref.neutral(B, N), ex, k), topk_adjust_ref.topk(s, bias, None, None, ex, k)):
        np.testing.assert_array_equal(_bits(g), _bits(w))


def test_no_case_of_the_gpu_test_is_empty():
    """On the generated data alone: every (shape, subset) on which a list of k can be full (cases.can_fill) has a user with a full
    list and a user with a short one; each of the window and the tag set closes roughly a third of the pairs on its own, and some
    pairs are closed by both at once; the slots close a few pairs (NaN deltas) and move the rest."""
    for shape in cases.CASES + [(33, 2049, 32, 65, 8, 19, 16, 5, True), (65, 2049, 60, 10, 8, 19, 16, 5, True)]:
        B, N, d, k = shape[:4]
        user, items, s, bias, parts, after, ex, tg = cases.lattice(*shape)
        if shape[6] == 256 and N <= 2048:          # one slice: the first block's slots overflow every staged list (2048 words at most)
            assert ((parts.adj_ids[:32] >= 0) & (parts.adj_ids[:32] < N)).sum() > 2048, shape
        for subset in cases.SUBSETS:
            p, a = cases.select(parts, after, subset)
            n = (ref.topk(s, bias, p, ex, k, a)[0] >= 0).sum(axis=1)
            if cases.can_fill(B, N, k):
                assert (n == k).any() and (n < k).any(), (shape, subset, n)
            if "adjust" in subset and N >= 63 and shape[6] >= 16:
                other = ref.Parts(*p[:5])
                assert not np.array_equal(_bits(ref.topk(s, bias, p, ex, k, None)[1]), _bits(ref.topk(s, bias, other, ex, k, None)[1]))
        if N >= 500 and B >= 33:
            zero = np.zeros((B, N), dtype=np.float32)
            w = ~ref.eligible(zero, ref.Parts(*parts[:2]), None)[1:B - 2]
            t = ~ref.eligible(zero, ref.Parts(None, None, *parts[2:5]), None)[1:B - 2]
            assert 0.2 < w.mean() < 0.5, (shape, w.mean())
            if shape[5] > 1:
                assert 0.2 < t.mean() < 0.5, (shape, t.mean())
            assert (w & t).mean() > 0.03, shape


# ---- 2: the symbols ----------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_signatures_and_library():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, name + " is not declared in include/nrms_hip.h"
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(2).count(",") + 1, name
    # a request takes the four pairs, n_tags and n_adjust beside the biased call's arguments; the queries are the same
    assert len(_lib.SIGNATURES["nrms_topk_dot_request"][1]) == len(_lib.SIGNATURES["nrms_topk_dot_biased"][1]) + 10
    assert len(_lib.SIGNATURES["nrms_rank_dot_request"][1]) == len(_lib.SIGNATURES["nrms_rank_dot_biased"][1]) + 8
    assert _lib.SIGNATURES["nrms_topk_dot_request_workspace_bytes"] == _lib.SIGNATURES["nrms_topk_dot_workspace_bytes"]
    assert _lib.SIGNATURES["nrms_rank_dot_request_workspace_bytes"] == _lib.SIGNATURES["nrms_rank_dot_workspace_bytes"]
    lib = _lib.load()                                                # binds every symbol: a missing export raises here
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for word in ("s'' = (s + bias[n]) + delta", "topk_dot_request: ...", "rank_dot_request: ...", "block-uniform", "section 8o"):
        assert word in text, word


def test_request_queries_and_host_side_refusals():
    """The queries equal the plain ones; half-given pairs and bad extents are refused on the host, by name, before any launch."""
    lib = _lib.load()
    for B, N, d, k in ((70, 5000, 40, 10), (512, 130000, 300, 100), (1, 0, 1, 1), (0, 5, 3, 256)):
        assert lib.nrms_topk_dot_request_workspace_bytes(B, C.c_int64(N), d, k) == lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k) > 0
        r = lib.nrms_rank_dot_request_workspace_bytes(B, C.c_int64(N), d, min(k, 32), 70)
        assert r == lib.nrms_rank_dot_workspace_bytes(B, C.c_int64(N), d, min(k, 32), 70) > 0
    assert lib.nrms_topk_dot_request_workspace_bytes(70, C.c_int64(5000), 40, 257) == 0
    assert lib.nrms_rank_dot_request_workspace_bytes(70, C.c_int64(5000), 40, 33, 0) == 0
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    base = dict(time=p, win=p, tag=p, n_tags=3, allow=p, aid=p, adl=p, E=4, a_s=p, a_i=p, nbytes=4096)

    def topk(**over):
        a = dict(base, **over)
        return lib.nrms_topk_dot_request(2, C.c_int64(4), 2, 2, p, p, None, a["time"], a["win"], a["tag"], a["n_tags"], a["allow"],
                                         a["aid"], a["adl"], a["E"], a["a_s"], a["a_i"], None, 0, p, p, p, C.c_size_t(a["nbytes"]), None)

    def rank(**over):
        a = dict(base, **over)
        return lib.nrms_rank_dot_request(2, C.c_int64(4), 2, 2, p, p, None, a["time"], a["win"], a["tag"], a["n_tags"], a["allow"],
                                         a["aid"], a["adl"], a["E"], p, None, 0, p, p, p, C.c_size_t(a["nbytes"]), None)

    pairs = [(dict(time=None), b"item_time is null"), (dict(win=None), b"window is null"), (dict(tag=None), b"item_tag is null"),
             (dict(allow=None), b"allow is null"), (dict(aid=None), b"adj_ids is null"), (dict(adl=None), b"adj_delta is null"),
             (dict(n_tags=0), b"n_tags must be in [1, 512]"), (dict(n_tags=513), b"n_tags must be in [1, 512]"),
             (dict(E=257), b"n_adjust must be in [0, 256]"), (dict(E=-1), b"n_adjust must be in [0, 256]")]
    for call, who, extra in ((topk, b"topk_dot_request: ", [(dict(a_s=None), b"after_scores is null"), (dict(a_i=None), b"after_ids is null")]),
                             (rank, b"rank_dot_request: ", [])):
        for kw, word in pairs + extra:
            assert call(**kw) == _lib.NRMS_EINVAL, (who, kw)
            msg = lib.nrms_last_error()
            assert msg.startswith(who) and word in msg, msg
        assert call(nbytes=8) == _lib.NRMS_EWORKSPACE
        assert lib.nrms_last_error().startswith(who)
    # a single part forwards: the error is the part's own call's
    assert lib.nrms_topk_dot_request(2, C.c_int64(4), 2, 2, p, p, None, p, p, None, 0, None, None, None, 0, None, None, None, 0, p, p, p,
                                     C.c_size_t(8), None) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_last_error().startswith(b"topk_dot_windowed: ")
    assert lib.nrms_topk_dot_request(2, C.c_int64(4), 2, 2, p, p, None, p, p, None, 0, None, None, None, 0, p, p, None, 0, p, p, p,
                                     C.c_size_t(8), None) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_last_error().startswith(b"topk_dot_after: ")                 # window + cursor
    assert lib.nrms_rank_dot_request(2, C.c_int64(4), 2, 2, p, p, None, None, None, p, 3, p, None, None, 0, p, None, 0, p, p, p,
                                     C.c_size_t(8), None) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_last_error().startswith(b"rank_dot_tagged: ")
    assert lib.nrms_topk_dot_request(0, C.c_int64(4), 2, 2, None, None, None, None, None, None, 0, None, None, None, 0, None, None, None,
                                     0, None, None, None, C.c_size_t(0), None) == _lib.NRMS_OK          # B = 0 is a no-op


# ---- 3: the models -----------------------------------------------------------------------------------------------------------
def test_models_have_the_request_methods():
    from importlib import import_module
    from pytorch_news_recommender_amd.model import nrms_hip
    want_k = "(self, batch, k, catalogue, exclude_history=True, *, item_bias=None, item_time=None, window=None, item_tag=None, allow=None, adjust=None, after=None)"
    assert str(inspect.signature(nrms_hip.Model.recommend_request)) == want_k
    assert list(inspect.signature(nrms_hip.Model.rank_targets_request).parameters) == [
        "self", "batch", "targets", "catalogue", "exclude_history", "item_bias", "item_time", "window", "item_tag", "allow", "adjust"]
    for name in ("nrms_v1_hip", "nrms_naml_hip", "nrms_bert_hip"):          # inherited, not restated
        M = import_module("pytorch_news_recommender_amd.model." + name).Model
        assert M.recommend_request is nrms_hip.Model.recommend_request and M.rank_targets_request is nrms_hip.Model.rank_targets_request
    # the methods beside them are as they were
    assert "adjust" not in inspect.signature(nrms_hip.Model.recommend_tagged).parameters
    assert "item_tag" not in inspect.signature(nrms_hip.Model.recommend).parameters


def test_models_that_cannot_serve_a_request_refuse_in_their_own_words():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    for mod, who, why in ((hierec_hip, "hierec", "nrms_topk_grouped_dot"), (graph_hip, "graph", "click graph")):
        with pytest.raises(NotImplementedError, match=who + ": recommend_request is not available") as e:
            mod.Model.recommend_request(None, {}, 5, None, adjust=None, item_bias=torch.zeros(3))
        assert why in str(e.value)
        with pytest.raises(NotImplementedError, match=who + ": rank_targets_request is not available") as e:
            mod.Model.rank_targets_request(None, {}, None, None, item_tag=None)
        assert why in str(e.value)


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def top_k_request(self, user, items, k, exclude=None, bias=None, **kw):
        self.calls.append(("top_k_request", items.shape[0], bias, kw))
        B = user.shape[0]
        return torch.zeros(B, k), torch.arange(k).expand(B, k).contiguous() - 1           # (row ids: the first is padding)

    def rank_of_request(self, user, items, targets, exclude=None, bias=None, **kw):
        self.calls.append(("rank_of_request", targets.clone(), bias, kw))
        return torch.ones_like(targets, dtype=torch.int32), torch.zeros(targets.shape)


def _fake_model():
    from pytorch_news_recommender_amd.model import nrms_hip
    m = object.__new__(nrms_hip.Model)
    m._engine = _FakeEngine()
    cat = torch.zeros(6, 4)
    m._catalogue_query = lambda batch, catalogue, exclude_history, who: (torch.zeros(2, 4), cat, None)
    return m, cat


def test_model_methods_route_the_parts_to_the_engine():
    """Rows 1.. of every per-news array, news ids to rows, absent parts absent, pairs both or neither: before anything touches a
    device."""
    m, cat = _fake_model()
    B, N = 2, 6
    time, tag = torch.arange(N, dtype=torch.int32), torch.arange(N, dtype=torch.int64) % 3
    window = torch.tensor([[0, 4], [2, 9]], dtype=torch.int32)
    allow = torch.tensor([[True, False, True], [False, True, True]])
    adjust = (torch.tensor([[0, 3], [5, 9]]), torch.tensor([[1.0, -1.0], [0.5, 2.0]]))
    prior = torch.arange(N, dtype=torch.float32)
    ids, sc = m.recommend_request({}, 3, cat, item_bias=prior, item_time=time, window=window, item_tag=tag, allow=allow, adjust=adjust,
                                  after=(torch.tensor([0, 4]), torch.tensor([1.0, 2.0])))
    name, n_rows, bias, kw = m._engine.calls[-1]
    assert name == "top_k_request" and n_rows == N - 1 and bias.tolist() == prior[1:].tolist()
    assert kw["item_time"].tolist() == time[1:].tolist() and kw["window"] is window
    assert kw["item_tag"].tolist() == tag[1:].tolist() and kw["n_tags"] == 3 and kw["allow"] is allow
    assert kw["adj_ids"].tolist() == [[-1, 2], [4, 8]] and kw["adj_delta"].tolist() == adjust[1].tolist()
    assert kw["after_ids"].tolist() == [-1, 3] and kw["after_scores"].tolist() == [1.0, 2.0]          # id 0 reads as exhausted
    assert ids.tolist() == [[-1, 1, 2], [-1, 1, 2]]                                                  # rows back to news ids
    m.recommend_request({}, 3, cat)
    assert m._engine.calls[-1][2] is None and m._engine.calls[-1][3] == {}
    m.recommend_request({}, 3, cat, item_tag=tag, allow=allow)
    assert sorted(m._engine.calls[-1][3]) == ["allow", "item_tag", "n_tags"]
    r, _ = m.rank_targets_request({}, torch.tensor([[1, 0], [5, -1]]), cat, item_time=time, window=window, adjust=adjust)
    name, tg, bias, kw = m._engine.calls[-1]
    assert name == "rank_of_request" and tg.tolist() == [[0, -1], [4, -2]] and bias is None
    assert sorted(kw) == ["adj_delta", "adj_ids", "item_time", "window"]
    n_calls = len(m._engine.calls)
    for bad, word in ((dict(item_time=time), "item_time and window go together"), (dict(window=window), "item_time and window go together"),
                      (dict(item_tag=tag), "item_tag and allow go together"), (dict(allow=allow), "item_tag and allow go together"),
                      (dict(adjust=adjust[0]), "adjust must be a pair"), (dict(item_time=time[:-1], window=window), "item_time must be"),
                      (dict(item_tag=tag, allow=allow[:1]), "allow must be")):
        with pytest.raises(_lib.NrmsError, match=word):
            m.recommend_request({}, 3, cat, **bad)
        with pytest.raises(_lib.NrmsError, match=word):
            m.rank_targets_request({}, torch.zeros(2, 1, dtype=torch.int64), cat, **bad)
    with pytest.raises(_lib.NrmsError, match="after must be"):
        m.recommend_request({}, 3, cat, after=torch.zeros(2))
    with pytest.raises(_lib.NrmsError, match="after must be"):
        m.recommend_request({}, 3, cat, after=(torch.zeros(3), torch.zeros(3)))
    assert len(m._engine.calls) == n_calls


# ---- 4: the loops ------------------------------------------------------------------------------------------------------------
class _Request(_Prior):
    def recommend_request(self, batch, k, catalogue, exclude_history=True, **kw):
        self.requests.append(("recommend_request", kw))
        return _Stub.recommend(self, batch, k, catalogue, exclude_history)

    def rank_targets_request(self, batch, targets, catalogue, exclude_history=True, **kw):
        self.requests.append(("rank_targets_request", kw))
        rk, _ = _Stub.rank_targets(self, batch, targets, catalogue, exclude_history)
        closed = torch.zeros_like(rk, dtype=torch.bool)
        if "allow" in kw:          # close what the tag set closes, as the kernel would
            t = kw["item_tag"][targets.clamp(min=0)]
            closed |= ~kw["allow"].gather(1, t)
        if "window" in kw:
            tt = kw["item_time"].to(torch.int64)[targets.clamp(min=0)]
            closed |= ~((tt >= kw["window"][:, :1]) & (tt < kw["window"][:, 1:]))
        return torch.where(closed, torch.zeros_like(rk), rk), None


def test_loops_hand_every_sample_its_parts(tmp_path):
    titles = torch.zeros(20, 3, dtype=torch.int64)
    batches = [{"candidate_ids": torch.tensor([[3, 4, 5], [6, 7, 0]]), "browsed_ids": torch.zeros(2, 2, dtype=torch.int64)},
               {"candidate_ids": torch.tensor([[8, 9, 1]]), "browsed_ids": torch.zeros(1, 2, dtype=torch.int64)}]
    labels = [[0, 1, 0], [1, 1], [0, 0, 1]]
    ids = torch.tensor([[4, 0], [6, 7], [1, 19]])
    delta = torch.tensor([[-1.0, 0.0], [-0.5, -1.5], [2.0, float("nan")]])
    item_time, req = torch.arange(20, dtype=torch.int32), np.array([4, 7, 30])
    tag = torch.arange(20, dtype=torch.int64) % 2
    allow = torch.tensor([[True, False], [True, True], [False, True]])
    p = torch.ones(20)
    every = dict(item_time=item_time, request_time=req, window_span=3, item_tag=tag, allow_tags=allow, adjust=(ids, delta), item_bias=p)
    rec = lambda m, **kw: train_eval.recommend_request(None, m, batches, titles, 4, out_file=str(tmp_path / "a.txt"), **kw)
    ev = lambda m, **kw: train_eval.evaluate_retrieval_request(None, m, batches, titles, labels, ks=(1,), verbose=False, **kw)
    for call, meth in ((rec, "recommend_request"), (ev, "rank_targets_request")):
        m = _Request()
        m.requests = []
        out = call(m, **every)
        assert [c[0] for c in m.requests] == [meth] * 2
        a, b = m.requests[0][1], m.requests[1][1]
        assert sorted(a) == ["adjust", "allow", "item_bias", "item_tag", "item_time", "window"]
        assert a["item_bias"] is p and a["item_time"] is item_time and a["item_tag"] is tag
        assert a["window"].tolist() == [[1, 5], [4, 8]] and b["window"].tolist() == [[27, 31]]          # [t - span, t + 1)
        assert a["allow"].tolist() == allow[:2].tolist() and b["allow"].tolist() == allow[2:].tolist()
        assert a["adjust"][0].tolist() == ids[:2].tolist() and b["adjust"][0].tolist() == ids[2:].tolist()
        assert a["adjust"][1].dtype == torch.float32 and a["adjust"][0].dtype == torch.int64
        if call is ev:
            # targets 4 | 6, 7 | 1: 4 is in [1, 5) and tag 0 is open; 6 is in [4, 8), 7 too; 1 is outside [27, 31): closed
            assert out["n_targets"] == 3 and out["n_skipped"] == 1 and out["n_closed"] == 1 and out["recall@1"] == 1.0
        else:
            assert open(out).read().splitlines() == ["1 [1,2,3,4]", "2 [1,2,3,4]", "3 [1,2,3,4]"]
        m.requests = []
        call(m)                                                      # no part: the request methods, with no keyword at all
        assert [c[1] for c in m.requests] == [{}, {}]
        m.requests = []
        call(m, item_tag=tag, allow_tags=allow, adjust=(ids.numpy(), delta.numpy()))
        assert [sorted(c[1]) for c in m.requests] == [["adjust", "allow", "item_tag"]] * 2
        with pytest.raises(AttributeError, match=meth):
            call(_Stub(), **every)                                   # a model without the methods fails there, not silently
        for bad, word in ((dict(item_time=item_time), "go together"), (dict(item_tag=tag), "go together"),
                          (dict(allow_tags=allow), "go together"), (dict(adjust=ids), "adjust must be"),
                          (dict(item_tag=tag, allow_tags=allow[:2]), "allow_tags rows"), (dict(adjust=(ids[:2], delta[:2])), "adjust rows"),
                          (dict(item_time=item_time, request_time=req[:2], window_span=3), "request times"),
                          (dict(item_time=item_time, request_time=req, window_span=0), "window_span must be")):
            with pytest.raises(ValueError, match=word):
                call(m, **bad)
    # the existing loops keep every refusal they have
    m = _Request()
    m.requests = []
    old_rec = lambda **kw: train_eval.recommend(None, m, batches, titles, 4, out_file=str(tmp_path / "b.txt"), **kw)
    old_ev = lambda **kw: train_eval.evaluate_retrieval(None, m, batches, titles, labels, ks=(1,), verbose=False, **kw)
    for old in (old_rec, old_ev):
        with pytest.raises(ValueError, match="does not go with adjust"):
            old(adjust=(ids, delta), item_tag=tag, allow_tags=allow)
        with pytest.raises(ValueError, match="does not go with adjust"):
            old(adjust=(ids, delta), item_time=item_time, request_time=req, window_span=3)
        with pytest.raises(ValueError, match="does not go with item_tag / allow_tags"):
            old(item_tag=tag, allow_tags=allow, item_time=item_time, request_time=req, window_span=3)
    assert m.requests == []


# ---- 5: the command line -----------------------------------------------------------------------------------------------------
BASE = ["--model", "nrms_v0", "--dataset", "synthetic", "--negatives", "catalogue"]


def _checks(argv):
    args = run_v0.build_parser().parse_args(BASE + argv)
    run_v0.check_prior_args(args)
    run_v0.check_combine_args(args)
    run_v0.check_window_args(args)
    tags = run_v0.check_tag_args(args)
    run_v0.check_caps_args(args)
    seen = run_v0.check_seen_args(args)
    return args, tags, seen


def test_combine_filters_parses_and_lifts_the_three_refusals():
    every = ["--recommend", "10", "--catalogue_window", "5", "--mute_categories", "1,2", "--seen_discount", "0.5", "--popularity_prior", "0.1"]
    args, tags, seen = _checks(every + ["--combine_filters"])
    assert args.combine_filters and tags == (None, (1, 2)) and seen == (0.5, 32) and args.catalogue_window == 5
    args, tags, seen = _checks(["--retrieval_metrics", "10", "--only_categories", "own", "--seen_discount", "0.5", "--combine_filters"])
    assert tags == ("own", None) and seen == (0.5, 32)
    assert not run_v0.build_parser().parse_args(BASE).combine_filters
    # without the flag every refusal stays
    for argv, word in ((every, "--catalogue_window"),
                       (["--recommend", "10", "--mute_categories", "1", "--seen_discount", "0.5"], "--mute_categories"),
                       (["--recommend", "10", "--catalogue_window", "5", "--only_categories", "own"], "--catalogue_window"),
                       (["--recommend", "10", "--catalogue_window", "5", "--seen_discount", "0.5"], "--catalogue_window")):
        with pytest.raises(SystemExit, match="drop " + word):
            _checks(argv)
    # with it, what a request does not compose with is still refused, by name
    for extra in (["--diversity", "0.5"], ["--coarse_catalogue"], ["--max_per_category", "2"], ["--explain", "3"],
                  ["--sections", "category"], ["--retrieval_nll", "1.0", "--retrieval_metrics", "10"]):
        with pytest.raises(SystemExit, match="--combine_filters: .*drop " + extra[0]):
            _checks(every + ["--combine_filters"] + extra)
    with pytest.raises(SystemExit, match="--combine_filters: .*drop --recommend_deep"):
        _checks(["--recommend_deep", "300", "--catalogue_window", "5", "--combine_filters", "--retrieval_metrics", "10"])
    with pytest.raises(SystemExit, match="--combine_filters: combines the filters of"):
        _checks(["--combine_filters"])
    with pytest.raises(SystemExit, match="--combine_filters: model 'hierec'"):
        run_v0.check_combine_args(run_v0.build_parser().parse_args(["--model", "hierec", "--recommend", "5", "--combine_filters"]))
