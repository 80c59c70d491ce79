"""The capped request on the host (no GPU): tests/topk_request_caps_ref.py held against a brute-force sort-and-walk and against the
consequences 1 to 6 the header states; the paging identity over random caps; remaining_caps on hand-made tensors; the lattice data
of the GPU test checked for cases in which no cap rations; the new symbols and the C call's argument checks; and the Python layers
with recording fakes: keyword routing, the loop's per-batch slicing and statistics, the refusals of HieRec and the graph model, the
--request_max_per_category flag and the refusals --max_per_category keeps."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, run_v0, train_eval
from pytorch_news_recommender_amd.engine import remaining_caps

from tests import topk_caps_ref, topk_request_caps_cases as cases, topk_request_caps_ref as ref, topk_request_ref
from tests.test_topk_bias_host import _Prior, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrms_topk_dot_request_capped_workspace_bytes", "nrms_topk_dot_request_capped")


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=str(what))


def _key(s):
    """The order-preserving integer of a float32 score, -0.0 as +0.0 (the kernels' entry, restated)."""
    u = int(np.float32(0.0 if s == 0.0 else s).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _brute(s, bias, item_tag, n_tags, cap, parts, ex, k, after):
    """Python loops, one sort and one walk per user: nothing shared with the ref but the statement of the contract."""
    B, N = s.shape
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=np.float32)
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
            if parts.allow is not None and not (0 <= item_tag[n] < n_tags and parts.allow[b, item_tag[n]]):
                continue
            rows.append((-_key(v), n, v))
        rows.sort()
        if after is not None and after[1][b] != ref.PAGE_BEGIN:
            if after[1][b] < 0 or np.isnan(after[0][b]):
                rows = []
            else:
                cur = (-_key(after[0][b]), int(after[1][b]))
                rows = [r for r in rows if (r[0], r[1]) > cur]
        room = [max(int(c), 0) for c in cap[b]]
        j = 0
        for _, n, v in rows:
            t = int(item_tag[n])
            if j < k and 0 <= t < n_tags and room[t] > 0:
                room[t] -= 1
                ids[b, j], out[b, j] = n, (np.float32(0.0) if v == 0.0 else v)
                j += 1
    return ids, out


# ---- 1: the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2, 3])
def test_ref_against_brute_force(case):
    B, N, d, k, n_tags = cases.CASES[case][:5]
    user, items, s, bias, item_tag, cap, parts, after, ex = cases.lattice(*cases.CASES[case])
    rows = slice(0, 9)                                               # the brute force is slow: nine users are enough
    cut = lambda x: x if x is None or np.ndim(x) == 0 or np.shape(x)[0] != B else x[rows]
    sub = ref.Parts(*[cut(x) for x in parts])
    aft = (after[0][rows], after[1][rows])
    for subset in cases.SUBSETS:
        p, a = cases.select(sub, aft, subset)
        _same(ref.topk(s[rows], bias, item_tag, n_tags, cap[rows], p, cut(ex), k, a),
              _brute(s[rows], bias, item_tag, n_tags, cap[rows], p, cut(ex), k, a), subset)


def _mid():
    shape = cases.CASES[4]                                           # (33, 513, 40, 65, 44, 16, 70, False)
    return shape, cases.lattice(*shape)


def test_uncapped_is_the_request_and_no_part_is_the_capped_call():
    """1 and 2: every cap >= k is topk_request_ref with allow as its tag set (allow absent: every tag in range); no part at all is
    topk_caps_ref."""
    (B, N, d, k, n_tags, E, n_ex, _), (user, items, s, bias, item_tag, cap, parts, after, ex) = _mid()
    big = np.full((B, n_tags), k, dtype=np.int32)
    big[1::2] = k + 7
    every = np.ones((B, n_tags), dtype=bool)
    for subset in cases.SUBSETS:
        p, a = cases.select(parts, after, subset)
        q = p if p.allow is not None else p._replace(item_tag=item_tag, n_tags=n_tags, allow=every)
        _same(ref.topk(s, bias, item_tag, n_tags, big, p, ex, k, a), topk_request_ref.topk(s, bias, q, ex, k, a), subset)
    _same(ref.topk(s, bias, item_tag, n_tags, cap, ref.Parts(), ex, k), topk_caps_ref.topk(s, bias, item_tag, n_tags, cap, ex, k))


def test_prefix_bound_and_row_independence():
    """3, 6 and 7: the first k' columns of k are the call with k'; no row holds more than max(cap, 0) ids of a tag; a row alone is
    the row in the batch."""
    (B, N, d, k, n_tags, E, n_ex, _), (user, items, s, bias, item_tag, cap, parts, after, ex) = _mid()
    for subset in (("window", "allow", "adjust", "cursor"), ("window", "adjust"), ("allow",)):
        p, a = cases.select(parts, after, subset)
        ids, sc = ref.topk(s, bias, item_tag, n_tags, cap, p, ex, k, a)
        for kk in (1, 7, 64):
            _same(ref.topk(s, bias, item_tag, n_tags, cap, p, ex, kk, a), (ids[:, :kk], sc[:, :kk]), (subset, kk))
        for b in range(B):
            served = ids[b][ids[b] >= 0]
            tags = item_tag[served]
            assert ((tags >= 0) & (tags < n_tags)).all()
            counts = np.bincount(tags, minlength=n_tags)
            assert (counts <= np.maximum(cap[b], 0)).all(), (subset, b)
        for b in (0, 5, 6, 32):
            pb = ref.Parts(*[x if x is None or np.ndim(x) == 0 or np.shape(x)[0] != B else x[b:b + 1] for x in p])
            ab = None if a is None else (a[0][b:b + 1], a[1][b:b + 1])
            _same(ref.topk(s[b:b + 1], bias, item_tag, n_tags, cap[b:b + 1], pb, ex[b:b + 1], k, ab), (ids[b:b + 1], sc[b:b + 1]), (subset, b))


def test_row_is_the_capped_call_with_the_parts_as_bias():
    """4: without a prior and a cursor, row b is topk_caps_ref at B = 1 with the deltas scattered and NaN where a part closes the
    item, and so the greedy walk over that bias's full ranking."""
    (B, N, d, k, n_tags, E, n_ex, _), (user, items, s, bias, item_tag, cap, parts, after, ex) = _mid()
    p, _ = cases.select(parts, None, ("window", "allow", "adjust"))
    ids, sc = ref.topk(s, None, item_tag, n_tags, cap, p, ex, k)
    for b in (0, 1, 2, 5, 6, 17, 32):
        as_bias = ref.as_bias(p, b, N)
        _same(topk_caps_ref.topk(s[b:b + 1], as_bias, item_tag, n_tags, cap[b:b + 1], ex[b:b + 1], k), (ids[b:b + 1], sc[b:b + 1]), b)
        deep = topk_request_ref.topk(s[b:b + 1], as_bias, ref.Parts(), ex[b:b + 1], N)
        walk = topk_caps_ref.greedy_over_list(deep[0][0], deep[1][0], item_tag, n_tags, cap[b], k)
        _same(walk, (ids[b], sc[b]), b)


# ---- 2: paging ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_paging_identity_over_random_caps(seed):
    """5: pages chained through the cursor and remaining_caps, laid end to end, are the columns of one call with k = the sum of
    their lengths, then padding: over random caps, with a sum of caps below k and with one dominant tag."""
    rng = np.random.default_rng(seed)
    B, N, n_tags, E = 6, 300, 5, 8
    s = rng.integers(-6, 7, size=(B, N)).astype(np.float32)                  # few values: long runs of ties
    bias = (rng.integers(-8, 9, size=N) * 0.25).astype(np.float32)
    bias[rng.integers(0, N, size=3)] = np.nan
    item_tag = np.where(rng.random(N) < 0.6, 0, rng.integers(0, n_tags, size=N)).astype(np.int32)      # tag 0 dominates
    item_tag[rng.integers(0, N, size=3)] = -1
    cap = rng.integers(0, 40, size=(B, n_tags)).astype(np.int32)
    cap[0] = (1, 2, 0, 1, 3)                                                 # sum(cap) < k: the list cannot fill
    cap[1] = (200, 1, 1, 1, 1)                                               # the dominant tag is uncapped
    cap[2] = (2, 200, 200, 200, 200)                                         # ... and tightly capped
    lo = rng.integers(0, 11, size=B)
    parts = ref.Parts(rng.integers(0, 30, size=N).astype(np.int32), np.stack([lo, lo + 20], axis=1).astype(np.int32), item_tag, n_tags,
                      rng.random((B, n_tags)) < 0.8, rng.integers(-1, N, size=(B, E)).astype(np.int64),
                      (rng.integers(-8, 9, size=(B, E)) * 0.5).astype(np.float32))
    ex = rng.integers(0, N, size=(B, 4)).astype(np.int64)
    for subset in ((), ("window", "allow", "adjust"), ("adjust",)):
        p, _ = cases.select(parts, None, subset)
        for lengths in ([7] * 10, [1, 2, 3, 50, 9, 100], [64, 64, 64, 64]):
            total = sum(lengths)
            want = ref.topk(s, bias, item_tag, n_tags, cap, p, ex, total)
            _same(ref.pages(s, bias, item_tag, n_tags, cap, p, ex, lengths), want, (subset, lengths))
        n = (want[0] >= 0).sum(axis=1)
        assert n[0] <= 7 and (n < 256).any() and n.max() > 30


def test_remaining_caps_on_hand_made_tensors():
    item_tag = torch.tensor([0, 1, 1, 2, -1, 3, 0, 7], dtype=torch.int32)
    cap = torch.tensor([[2, 2, 2, 2], [0, 5, 1, 100]], dtype=torch.int32)
    served = torch.tensor([[0, 6, 1, -1, -1], [1, 2, 3, 4, 7]])
    got = remaining_caps(cap, served, item_tag, 4)
    assert got.dtype == torch.int32 and got.tolist() == [[0, 1, 2, 2], [0, 3, 0, 100]]       # -1, tag -1 and tag 7 are ignored
    # one cap row for every user, int64 ids and tags, an id past the catalogue, counting past the cap
    got = remaining_caps(torch.tensor([1, 1, 1, 1]), torch.tensor([[0, 6, 8], [5, 5, -1]]), item_tag.to(torch.int64), 4)
    assert got.tolist() == [[-1, 1, 1, 1], [1, 1, 1, -1]]
    assert remaining_caps(cap, torch.zeros(2, 0, dtype=torch.int64), item_tag, 4).tolist() == cap.tolist()
    np.testing.assert_array_equal(got.numpy(), ref.remaining_caps(np.array([1, 1, 1, 1]), np.array([[0, 6, -1], [5, 5, -1]]), item_tag.numpy(), 4))
    with pytest.raises(ValueError, match="remaining_caps"):
        remaining_caps(cap, served[0], item_tag, 4)
    with pytest.raises(ValueError, match="remaining_caps"):
        remaining_caps(cap, served, item_tag, 5)


# ---- 3: the GPU test's data --------------------------------------------------------------------------------------------------
GPU_SHAPES = cases.CASES + [(33, 2049, 40, 65, 19, 16, 5, True)]          # the last: the prior / exclude combinations' shape


@pytest.mark.parametrize("case", range(len(GPU_SHAPES)))
def test_a_cap_rations_in_every_case_of_the_gpu_test(case):
    """On the generated data alone: every (shape, subset) on which a cap can ration has a row where one does (the row differs from
    the row with every open tag left uncapped, so some tag reached its cap before the row was full), a row that is short and a row
    that is not empty; the uncapped users' rows are untouched.

    A deliberate departure from "every GPU case": the shapes with k = 1, N = 0 and N = 1 (cases.can_ration) are exempt, because no
    cap can ration there (a cap is 0 or >= k at k = 1, and a tag needs a second item); on them the test asserts the opposite, that
    no row differs from its uncapped row.  They stay in the GPU test for the paths they reach."""
    for shape in [GPU_SHAPES[case]]:
        B, N, d, k, n_tags = shape[:5]
        user, items, s, bias, item_tag, cap, parts, after, ex = cases.lattice(*shape)
        if B > 1:
            assert len({tuple(r) for r in cap[:32].tolist()}) > 8, "the caps differ inside a block"
        for subset in cases.SUBSETS:
            p, a = cases.select(parts, after, subset)
            ids, _ = ref.topk(s, bias, item_tag, n_tags, cap, p, ex, k, a)
            free, _ = ref.topk(s, bias, item_tag, n_tags, cases.uncapped(cap, k), p, ex, k, a)
            rationed = (ids != free).any(axis=1)
            if cases.can_ration(B, N, k):
                assert rationed.any(), (shape, subset)
                if B > 1:
                    n = (ids >= 0).sum(axis=1)
                    assert (n < k).any() and (n > 0).any(), (shape, subset, n)
                    assert not rationed[0::4].any(), (shape, subset)
            else:
                assert not rationed.any(), (shape, subset)


# ---- 4: the symbols and the C call's checks ----------------------------------------------------------------------------------
def test_new_symbols_in_header_signatures_and_library():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, name + " is not declared in include/nrms_hip.h"
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(2).count(",") + 1, name
    assert len(_lib.SIGNATURES["nrms_topk_dot_request_capped"][1]) == len(_lib.SIGNATURES["nrms_topk_dot_request"][1]) + 1       # cap
    assert _lib.SIGNATURES["nrms_topk_dot_request_capped_workspace_bytes"] == _lib.SIGNATURES["nrms_topk_dot_workspace_bytes"]
    lib = _lib.load()                                                # binds every symbol: a missing export raises here
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for word in ("topk_dot_request_capped: ...", "IN THIS CALL", "There is no rank form", "section 8p", "cap <= 0 closes the tag"):
        assert word in text, word


def test_query_and_host_side_refusals():
    """The query equals the plain one; missing required pointers, half-given pairs and bad extents are refused on the host, by
    name, before any launch (the pointers are host memory: a launch would fault)."""
    lib = _lib.load()
    for B, N, d, k in ((70, 5000, 40, 10), (512, 130000, 300, 100), (1, 0, 1, 1), (0, 5, 3, 256)):
        assert lib.nrms_topk_dot_request_capped_workspace_bytes(B, C.c_int64(N), d, k) == lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k) > 0
    assert lib.nrms_topk_dot_request_capped_workspace_bytes(70, C.c_int64(5000), 40, 257) == 0
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)
    base = dict(time=p, win=p, tag=p, n_tags=3, allow=p, cap=p, aid=p, adl=p, E=4, a_s=p, a_i=p, nbytes=4096, ws=p)

    def call(**over):
        a = dict(base, **over)
        return lib.nrms_topk_dot_request_capped(2, C.c_int64(4), 2, 2, p, p, None, a["time"], a["win"], a["tag"], a["n_tags"], a["allow"],
                                                a["cap"], a["aid"], a["adl"], a["E"], a["a_s"], a["a_i"], None, 0, p, p, a["ws"],
                                                C.c_size_t(a["nbytes"]), None)

    bad = [(dict(cap=None), b"cap is null"), (dict(tag=None), b"item_tag is null"),
           (dict(time=None), b"item_time is null"), (dict(win=None), b"window is null"),
           (dict(aid=None), b"adj_ids is null"), (dict(adl=None), b"adj_delta is null"),
           (dict(a_s=None), b"after_scores is null"), (dict(a_i=None), b"after_ids is null"),
           (dict(n_tags=0), b"n_tags must be in [1, 512]"), (dict(n_tags=513), b"n_tags must be in [1, 512]"),
           (dict(E=257), b"n_adjust must be in [0, 256]"), (dict(E=-1), b"n_adjust must be in [0, 256]"),
           (dict(cap=odd), b"cap must be 4-byte aligned"), (dict(tag=odd), b"item_tag must be 4-byte aligned"),
           (dict(allow=odd), b"allow must be 4-byte aligned"), (dict(a_i=odd), b"after_ids must be 8-byte aligned"),
           (dict(ws=odd), b"workspace must be 8-byte aligned"), (dict(ws=None), b"workspace is null")]
    for kw, word in bad:
        assert call(**kw) == _lib.NRMS_EINVAL, kw
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_request_capped: ") and word in msg, msg
    assert call(nbytes=8) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_last_error().startswith(b"topk_dot_request_capped: ")
    # the caps alone: the checks are still this call's, in its own name
    alone = dict(time=None, win=None, allow=None, aid=None, adl=None, E=0, a_s=None, a_i=None)
    assert call(nbytes=8, **alone) == _lib.NRMS_EWORKSPACE and lib.nrms_last_error().startswith(b"topk_dot_request_capped: ")
    assert call(cap=None, **alone) == _lib.NRMS_EINVAL and b"topk_dot_request_capped: cap is null" in lib.nrms_last_error()
    # allow is no pair: it goes with the item_tag the caps already need
    assert lib.nrms_topk_dot_request_capped(0, C.c_int64(4), 2, 2, None, None, None, None, None, None, 3, None, None, None, None, 0, None,
                                            None, None, 0, None, None, None, C.c_size_t(0), None) == _lib.NRMS_OK      # B = 0 is a no-op


# ---- 5: the models -----------------------------------------------------------------------------------------------------------
def test_models_have_the_method():
    from importlib import import_module
    from pytorch_news_recommender_amd.model import nrms_hip
    want = ("(self, batch, k, catalogue, item_tag, cap, exclude_history=True, *, item_bias=None, n_tags=None, item_time=None, "
            "window=None, allow=None, adjust=None, after=None)")
    assert str(inspect.signature(nrms_hip.Model.recommend_request_capped)) == want
    for name in ("nrms_v1_hip", "nrms_naml_hip", "nrms_bert_hip"):          # inherited, not restated
        assert import_module("pytorch_news_recommender_amd.model." + name).Model.recommend_request_capped is nrms_hip.Model.recommend_request_capped
    assert nrms_hip.remaining_caps is remaining_caps
    # the methods beside it are as they were
    assert "cap" not in inspect.signature(nrms_hip.Model.recommend_request).parameters
    assert "window" not in inspect.signature(nrms_hip.Model.recommend_capped).parameters
    from pytorch_news_recommender_amd.engine import NRMSEngine
    assert str(inspect.signature(NRMSEngine.top_k_request_capped)) == (
        "(self, user_vec, items, k, item_tag, n_tags, cap, exclude=None, bias=None, *, item_time=None, window=None, allow=None, "
        "adj_ids=None, adj_delta=None, after_scores=None, after_ids=None)")


def test_models_that_cannot_serve_it_refuse_in_their_own_words():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    for mod, who, why in ((hierec_hip, "hierec", "nrms_topk_grouped_dot"), (graph_hip, "graph", "click graph")):
        with pytest.raises(NotImplementedError, match=who + ": recommend_request_capped is not available") as e:
            mod.Model.recommend_request_capped(None, {}, 5, None, None, 2, adjust=None, item_bias=torch.zeros(3))
        assert why in str(e.value)


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def top_k_request_capped(self, user, items, k, item_tag, n_tags, cap, exclude=None, bias=None, **kw):
        self.calls.append((items.shape[0], item_tag, n_tags, cap, bias, kw))
        B = user.shape[0]
        return torch.zeros(B, k), torch.arange(k).expand(B, k).contiguous() - 1           # (row ids: the first is padding)


def test_model_method_routes_the_parts_to_the_engine():
    from pytorch_news_recommender_amd.model import nrms_hip
    m = object.__new__(nrms_hip.Model)
    m._engine = _FakeEngine()
    cat = torch.zeros(6, 4)
    m._catalogue_query = lambda batch, catalogue, exclude_history, who: (torch.zeros(2, 4), cat, None)
    N = 6
    time, tag = torch.arange(N, dtype=torch.int32), torch.arange(N, dtype=torch.int64) % 3
    window = torch.tensor([[0, 4], [2, 9]], dtype=torch.int32)
    allow = torch.tensor([[True, False, True], [False, True, True]])
    adjust = (torch.tensor([[0, 3], [5, 9]]), torch.tensor([[1.0, -1.0], [0.5, 2.0]]))
    prior = torch.arange(N, dtype=torch.float32)
    ids, sc = m.recommend_request_capped({}, 3, cat, tag, torch.tensor([2, -1, 5]), item_bias=prior, item_time=time, window=window,
                                         allow=allow, adjust=adjust, after=(torch.tensor([0, 4]), torch.tensor([1.0, 2.0])))
    n_rows, tags, n_tags, cap, bias, kw = m._engine.calls[-1]
    assert n_rows == N - 1 and tags.tolist() == tag[1:].tolist() and n_tags == 3 and bias.tolist() == prior[1:].tolist()
    assert cap.dtype == torch.int32 and cap.tolist() == [[2, 0, 5], [2, 0, 5]]
    assert kw["item_time"].tolist() == time[1:].tolist() and kw["window"] is window and kw["allow"] is allow
    assert kw["adj_ids"].tolist() == [[-1, 2], [4, 8]] and kw["after_ids"].tolist() == [-1, 3] and kw["after_scores"].tolist() == [1.0, 2.0]
    assert "item_tag" not in kw and "n_tags" not in kw
    assert ids.tolist() == [[-1, 1, 2], [-1, 1, 2]]                                                  # rows back to news ids
    m.recommend_request_capped({}, 3, cat, tag, 2, n_tags=3)
    assert m._engine.calls[-1][5] == {} and m._engine.calls[-1][3].tolist() == [[2, 2, 2]] * 2
    n_calls = len(m._engine.calls)
    for bad, word in ((dict(item_time=time), "item_time and window go together"), (dict(allow=allow[:, :2]), "allow must be"),
                      (dict(allow=allow[:1]), "allow must be"), (dict(adjust=adjust[0]), "adjust must be a pair"),
                      (dict(after=torch.zeros(2)), "after must be")):
        with pytest.raises(_lib.NrmsError, match=word):
            m.recommend_request_capped({}, 3, cat, tag, torch.tensor([2, 1, 5]), **bad)
    with pytest.raises(_lib.NrmsError, match="an int cap needs n_tags="):
        m.recommend_request_capped({}, 3, cat, tag, 2)
    with pytest.raises(_lib.NrmsError, match="item_tag must be"):
        m.recommend_request_capped({}, 3, cat, tag[:-1], torch.tensor([2, 1, 5]))
    assert len(m._engine.calls) == n_calls


# ---- 6: the loop -------------------------------------------------------------------------------------------------------------
class _Capped(_Prior):
    def recommend_request(self, batch, k, catalogue, exclude_history=True, **kw):
        self.requests.append(("recommend_request", kw))
        return _Stub.recommend(self, batch, k, catalogue, exclude_history)

    def recommend_request_capped(self, batch, k, catalogue, item_tag, cap, exclude_history=True, **kw):
        self.requests.append(("recommend_request_capped", dict(kw, item_tag=item_tag, cap=cap)))
        return _Stub.recommend(self, batch, k, catalogue, exclude_history)


def test_loop_hands_every_sample_its_caps_and_leaves_the_statistics(tmp_path):
    titles = torch.zeros(20, 3, dtype=torch.int64)
    batches = [{"candidate_ids": torch.tensor([[3, 4, 5], [6, 7, 0]]), "browsed_ids": torch.zeros(2, 2, dtype=torch.int64)},
               {"candidate_ids": torch.tensor([[8, 9, 1]]), "browsed_ids": torch.zeros(1, 2, dtype=torch.int64)}]
    ids = torch.tensor([[4, 0], [6, 7], [1, 19]])
    delta = torch.tensor([[-1.0, 0.0], [-0.5, -1.5], [2.0, float("nan")]])
    item_time, req = torch.arange(20, dtype=torch.int32), np.array([4, 7, 30])
    tag = torch.arange(20, dtype=torch.int64) % 2
    allow = torch.tensor([[True, False], [True, True], [False, True]])
    caps = torch.tensor([[1, 2], [2, 2], [3, 0]], dtype=torch.int32)
    rec = lambda m, **kw: train_eval.recommend_request(None, m, batches, titles, 4, out_file=str(tmp_path / "a.txt"), **kw)
    m = _Capped()
    m.requests = []
    out = rec(m, item_time=item_time, request_time=req, window_span=3, item_tag=tag, allow_tags=allow, adjust=(ids, delta),
              tag_caps=caps, heldout=[[2], [9], [4, 1]])
    assert [c[0] for c in m.requests] == ["recommend_request_capped"] * 2
    a, b = m.requests[0][1], m.requests[1][1]
    assert sorted(a) == ["adjust", "allow", "cap", "item_tag", "item_time", "window"] and a["item_tag"] is tag
    assert a["cap"].tolist() == [[1, 0], [2, 2]] and b["cap"].tolist() == [[0, 0]]          # a closed tag is cap 0, as in recommend()
    assert a["allow"].tolist() == allow[:2].tolist() and b["window"].tolist() == [[27, 31]]
    assert open(out).read().splitlines() == ["1 [1,2,3,4]", "2 [1,2,3,4]", "3 [1,2,3,4]"]
    st = m.last_caps_stats                                           # the stub serves 1, 2, 3, 4: tags 1, 0, 1, 0
    assert st["n_users"] == 3 and st["distinct_tags"] == 2.0 and st["largest_share"] == 0.5 and st["n_heldout"] == 4
    assert st["hit"][4] == 0.75 and st["hit"][1] == 0.25
    # the same statistics as recommend(tag_caps=) leaves
    old = _Capped()
    old.recommend_capped = lambda batch, k, catalogue, item_tag, cap, exclude_history=True, **kw: _Stub.recommend(old, batch, k, catalogue)
    train_eval.recommend(None, old, batches, titles, 4, out_file=str(tmp_path / "b.txt"), item_tag=tag, allow_tags=allow, tag_caps=caps,
                         heldout=[[2], [9], [4, 1]])
    assert old.last_caps_stats == st
    # caps alone, one row for everybody
    m.requests = []
    rec(m, item_tag=tag, tag_caps=torch.tensor([1, 1]))
    assert [sorted(c[1]) for c in m.requests] == [["cap", "item_tag"]] * 2 and m.requests[1][1]["cap"].tolist() == [[1, 1]]
    # no caps: the request method as before, and no statistics
    m.requests = []
    rec(m, item_tag=tag, allow_tags=allow, adjust=(ids, delta))
    assert [c[0] for c in m.requests] == ["recommend_request"] * 2 and m.last_caps_stats is None
    assert [sorted(c[1]) for c in m.requests] == [["adjust", "allow", "item_tag"]] * 2
    for bad, word in ((dict(tag_caps=caps), "give item_tag"), (dict(heldout=[[1], [2], [3]]), "give tag_caps"),
                      (dict(item_tag=tag, tag_caps=caps[:2]), "tag_caps rows"), (dict(item_tag=tag, tag_caps=2), "needs allow_tags")):
        with pytest.raises(ValueError, match=word):
            rec(m, **bad)
    with pytest.raises(AttributeError, match="recommend_request_capped"):
        rec(_Stub(), item_tag=tag, tag_caps=caps)                    # a model without the method fails there, not silently


# ---- 7: the command line -----------------------------------------------------------------------------------------------------
BASE = ["--model", "nrms_v0", "--dataset", "synthetic", "--negatives", "catalogue"]


def _checks(argv):
    args = run_v0.build_parser().parse_args(BASE + argv)
    run_v0.check_prior_args(args)
    run_v0.check_combine_args(args)
    run_v0.check_request_caps_args(args)
    run_v0.check_window_args(args)
    tags = run_v0.check_tag_args(args)
    run_v0.check_caps_args(args)
    seen = run_v0.check_seen_args(args)
    return args, tags, seen


def test_request_max_per_category_parses_and_keeps_the_old_refusals():
    every = ["--recommend", "10", "--catalogue_window", "5", "--mute_categories", "1,2", "--seen_discount", "0.5", "--popularity_prior", "0.1"]
    args, tags, seen = _checks(every + ["--combine_filters", "--request_max_per_category", "2"])
    assert args.request_max_per_category == 2 and args.max_per_category is None and tags == (None, (1, 2)) and seen == (0.5, 32)
    assert run_v0.build_parser().parse_args(BASE).request_max_per_category is None
    args, _, _ = _checks(["--recommend", "10", "--combine_filters", "--request_max_per_category", "1"])          # the caps alone
    assert args.request_max_per_category == 1
    with pytest.raises(SystemExit, match="--request_max_per_category M: M must be >= 1"):
        _checks(every + ["--combine_filters", "--request_max_per_category", "0"])
    for argv in (["--recommend", "10", "--request_max_per_category", "2"],
                 ["--retrieval_metrics", "10", "--combine_filters", "--request_max_per_category", "2"]):
        with pytest.raises(SystemExit, match="--request_max_per_category: caps the list of --combine_filters --recommend K"):
            _checks(argv)
    # what a request does not compose with is still refused, by --combine_filters, by name
    for extra in (["--diversity", "0.5"], ["--coarse_catalogue"], ["--explain", "3"], ["--sections", "category"]):
        with pytest.raises(SystemExit, match="--combine_filters: .*drop " + extra[0]):
            _checks(every + ["--combine_filters", "--request_max_per_category", "2"] + extra)
    with pytest.raises(SystemExit, match="--combine_filters: model 'hierec'"):
        a = run_v0.build_parser().parse_args(["--model", "hierec", "--recommend", "5", "--combine_filters", "--request_max_per_category", "2"])
        run_v0.check_combine_args(a)
    # --max_per_category keeps every refusal it has, the one beside --combine_filters included
    with pytest.raises(SystemExit, match="--combine_filters: .*drop --max_per_category"):
        _checks(every + ["--combine_filters", "--max_per_category", "2"])
    with pytest.raises(SystemExit, match="--max_per_category: .*drop --catalogue_window"):
        _checks(["--recommend", "10", "--catalogue_window", "5", "--max_per_category", "2"])
    with pytest.raises(SystemExit, match="--seen_discount: .*drop --max_per_category"):
        _checks(["--recommend", "10", "--seen_discount", "0.5", "--max_per_category", "2"])
