"""CPU-only checks of the per-category caps on the catalogue (include/nrms_hip.h nrms_topk_dot_capped): the pure-Python model of the
one-scan filter (buffer P, capped flush, the k_b threshold, S slices, merge) against the direct greedy walk, the prefix property,
the two degenerate cases against tests/topk_tags_ref.py, the C call's argument validation and workspace query (the library loads
without a GPU), the models' methods and refusals, train_eval's cap / allow composition on hand-made tensors and run_v0's
--max_per_category checks.  Parity is unpinned: the reference has no catalogue retrieval."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval

from tests import topk_caps_ref as ref
from tests import topk_tags_ref
from tests.test_topk_bias_host import _Prior, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrms_topk_dot_capped_workspace_bytes", "nrms_topk_dot_capped")
F = np.float32


# ---- 1: the filter model = the greedy walk -----------------------------------------------------------------------------------
def _case(rng, order):
    """One random user: tie-heavy lattice scores, a dominant tag, closed and out-of-range tags, sometimes sum(cap) < k."""
    N = int(rng.integers(1, 700))
    n_tags = int(rng.integers(1, 9))
    k = int(rng.integers(1, 40))
    s = rng.integers(-3, 4, size=N).astype(F)                        # heavy ties, -0.0 among them
    s[rng.integers(0, N)] = -0.0
    if rng.random() < 0.3:
        s[rng.integers(0, N)] = np.nan
    tag = rng.integers(0, n_tags, size=N)
    if rng.random() < 0.6:                                           # one dominant tag, which also holds the best scores
        dom = rng.random(N) < 0.8
        tag[dom] = 0
        s[dom] += F(2.0)
    tag[rng.random(N) < 0.05] = -1
    tag[rng.random(N) < 0.05] = n_tags
    mode = rng.integers(0, 4)
    if mode == 0:
        cap = rng.integers(-1, 4, size=n_tags)                       # closed tags, small caps: often sum(cap) < k
    elif mode == 1:
        cap = rng.integers(0, 2, size=n_tags) * (k + rng.integers(0, 3))          # {0} u [k, inf)
    elif mode == 2:
        cap = rng.integers(1, k + 2, size=n_tags)
    else:
        cap = np.full(n_tags, 1)
    ex = rng.integers(-1, N + 1, size=int(rng.integers(0, 6)))
    if order == "ascending":
        s = np.sort(s)                                               # NaN last
    elif order == "descending":
        s = np.sort(s)[::-1].copy()
    return s, tag, n_tags, cap, ex, k


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_filter_model_equals_greedy_walk(order):
    rng = np.random.default_rng({"ascending": 1, "descending": 2, "shuffled": 3}[order])
    flushes = short = refused = 0
    for _ in range(400):
        s, tag, n_tags, cap, ex, k = _case(rng, order)
        entries = ref.entries_of(ref.scores_of(s[None], None)[0], ex)           # in catalogue order
        want = ref.greedy(entries, tag, n_tags, cap, k)
        P = 128 if k + 64 <= 128 else 256
        for n_slices in (1, int(rng.integers(2, 6))):
            stats = {}
            got = ref.filter_topk(entries, tag, n_tags, cap, k, P, n_slices, stats)
            assert got == want, (order, n_slices, k, cap.tolist())
            flushes += stats.get("flushes", 0)
            refused += stats.get("refused_by_tag", 0)
        short += ref.reach(cap, k) < k
        # the prefix property: the greedy walk does not depend on k
        for k2 in (1, max(1, k // 2)):
            assert ref.greedy(entries, tag, n_tags, cap, k2) == want[:k2]
        # no tag above its cap, nothing closed or out of range
        used = {}
        for e in want:
            t = int(tag[ref.entry_id(e)])
            used[t] = used.get(t, 0) + 1
        assert all(0 <= t < n_tags and c <= cap[t] for t, c in used.items())
    assert flushes > 50 and short > 20 and (order == "ascending" or refused > 50)          # buffers did overflow; sum(cap) < k did occur


def test_filter_model_small_buffer_keeps_candidates_pending():
    """A buffer barely above k + 64 entries with 3 000 ascending scores of one tag and cap 1: every flush keeps one entry."""
    N, k = 3000, 10
    s = np.arange(N, dtype=F)
    tag = np.zeros(N, dtype=np.int64)
    tag[::7] = 1
    cap = np.array([1, 2])
    entries = ref.entries_of(s, None)
    stats = {}
    got = ref.filter_topk(entries, tag, 2, cap, k, 128, 3, stats)
    assert got == ref.greedy(entries, tag, 2, cap, k) and len(got) == 3 and stats["flushes"] > 10
    assert [ref.entry_id(e) for e in got] == [2999, 2996, 2989]      # the best of tag 0 (2996 is tag 1: 2996 = 7 * 428), then tag 1


def test_ref_topk_pads_and_restates_the_contract():
    s = np.array([[5.0, 4.0, 3.0, 2.0, 1.0, -0.0]], dtype=F)
    tag = np.array([0, 0, 1, 0, -1, 1])
    ids, sc = ref.topk(s, None, tag, 2, np.array([[1, 5]]), None, 4)
    assert ids.tolist() == [[0, 2, 5, -1]] and sc[0, :3].tolist() == [5.0, 3.0, 0.0] and sc[0, 3] == -np.inf
    assert not np.signbit(sc[0, 2])                                  # -0.0 comes back as +0.0
    assert ref.topk(s, None, tag, 2, np.array([[0, -3]]), None, 4)[0].tolist() == [[-1] * 4]
    assert ref.topk(s, None, tag, 2, np.array([[2, 1]]), np.array([[0, 9]]), 4)[0].tolist() == [[1, 2, 3, -1]]
    ids2, sc2 = ref.greedy_over_list(np.array([0, 1, 2, 3, 5, 4, -1]), np.array([5, 4, 3, 2, 0, 1, -np.inf], dtype=F), tag, 2, [1, 5], 4)
    assert ids2.tolist() == [0, 2, 5, -1] and sc2.tobytes() == sc[0].tobytes()
    assert ref.reach([1, 5], 4) == 4 and ref.reach([1, 2], 4) == 3 and ref.reach([-1, 0], 4) == 0 and ref.reach([9, 9], 4) == 4


@pytest.mark.parametrize("seed,with_bias", [(0, False), (1, True)])
def test_degenerate_caps_are_the_tagged_restatement(seed, with_bias):
    """Every cap >= k: the tagged restatement with all tags open; every cap in {0} u [k, inf): with allow = cap > 0."""
    rng = np.random.default_rng(seed)
    B, N, k, n_tags = 6, 60, 9, 5
    s = rng.integers(-3, 4, size=(B, N)).astype(F)
    s[1, 5] = np.nan
    bias = None
    if with_bias:
        bias = (rng.integers(-4, 5, size=N) * 0.5).astype(F)
        bias[[2, 11]] = np.nan
    tag = rng.integers(0, n_tags, size=N)
    tag[4], tag[9] = -1, n_tags
    ex = rng.integers(-1, N + 1, size=(B, 4))
    cap = rng.integers(k, k + 3, size=(B, n_tags))
    got = ref.topk(s, bias, tag, n_tags, cap, ex, k)
    want = topk_tags_ref.topk(s, bias, tag, n_tags, np.ones((B, n_tags), dtype=bool), ex, k)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    allow = rng.random((B, n_tags)) < 0.5
    allow[0], allow[1] = True, False
    cap = np.where(allow, cap, rng.integers(-2, 1, size=(B, n_tags)))
    got = ref.topk(s, bias, tag, n_tags, cap, ex, k)
    want = topk_tags_ref.topk(s, bias, tag, n_tags, allow, ex, k)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert (got[0][1] == -1).all()


# ---- 2: the symbols ----------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_signatures_and_library():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, name + " is not declared in include/nrms_hip.h"
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(2).count(",") + 1, name
    assert _lib.SIGNATURES["nrms_topk_dot_capped"] == _lib.SIGNATURES["nrms_topk_dot_tagged"]        # cap sits where allow sat
    assert _lib.SIGNATURES["nrms_topk_dot_capped_workspace_bytes"] == _lib.SIGNATURES["nrms_topk_dot_workspace_bytes"]
    lib = _lib.load()                                                # binds every symbol: a missing export raises here
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for word in ("served to nobody", "cap <= 0 closes the tag", "cap >= k leaves it uncapped", "(1)", "(2)", "(3)", "(4)", "(5)", "(6)",
                 "topk_dot_capped: ...", "1 <= n_tags <= 512", "C(S1 u S2) = C(C(S1) u C(S2))"):
        assert word in text, word


def test_capped_query_and_host_side_refusals():
    """The query equals the uncapped one; bad arguments are refused on the host (no GPU is needed to be told so)."""
    import ctypes as C
    lib = _lib.load()
    for B, N, d, k in ((70, 5000, 40, 10), (512, 130000, 300, 100), (1, 0, 1, 1), (0, 5, 3, 256)):
        q = lib.nrms_topk_dot_capped_workspace_bytes(B, C.c_int64(N), d, k)
        assert q == lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k) > 0
    assert lib.nrms_topk_dot_capped_workspace_bytes(70, C.c_int64(5000), 40, 257) == 0
    assert lib.nrms_topk_dot_capped_workspace_bytes(70, C.c_int64(5000), 40, 0) == 0
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)
    call = lambda B, N, d, k, tag, n_tags, cap, n_ex=0, ws=4096: lib.nrms_topk_dot_capped(
        B, C.c_int64(N), d, k, p, p, None, tag, n_tags, cap, None, n_ex, p, p, p, C.c_size_t(ws), None)
    for tag, n_tags, cap, word in ((None, 19, p, b"item_tag is null"), (p, 19, None, b"cap is null"),
                                   (odd, 19, p, b"item_tag must be 4-byte aligned"), (p, 19, odd, b"cap must be 4-byte aligned"),
                                   (p, 0, p, b"n_tags must be in [1, 512]"), (p, 513, p, b"n_tags must be in [1, 512]")):
        assert call(2, 4, 2, 2, tag, n_tags, cap) == _lib.NRMS_EINVAL
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_capped: ") and word in msg, msg
    for args, word in (((-1, 4, 2, 2), b"B must be"), ((2, -1, 2, 2), b"N must be"), ((2, 4, 0, 2), b"d must be"),
                       ((2, 4, 2, 0), b"k must be in [1, 256]"), ((2, 4, 2, 257), b"k must be in [1, 256]")):
        assert call(*args, p, 19, p) == _lib.NRMS_EINVAL
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_capped: ") and word in msg, msg
    assert call(2, 4, 2, 2, p, 19, p, n_ex=-1) == _lib.NRMS_EINVAL and b"n_exclude" in lib.nrms_last_error()
    assert call(2, 4, 2, 2, p, 19, p, ws=8) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_topk_dot_capped(0, C.c_int64(4), 2, 2, None, None, None, None, 19, None, None, 0, None, None, None,
                                    C.c_size_t(0), None) == _lib.NRMS_OK          # B = 0: a no-op


# ---- 3: the models -----------------------------------------------------------------------------------------------------------
MODELS = ("nrms_hip", "nrms_v1_hip", "nrms_naml_hip", "nrms_bert_hip", "hierec_hip", "graph_hip")


def test_every_model_says_whether_it_has_caps():
    from importlib import import_module
    sigs = set()
    for name in MODELS:
        M = import_module("pytorch_news_recommender_amd.model." + name).Model
        sigs.add(str(inspect.signature(M.recommend_capped)))
        assert M.CATALOGUE_CAPS is (name not in ("hierec_hip", "graph_hip")), name
    assert sigs == {"(self, batch, k, catalogue, item_tag, cap, exclude_history=True, *, item_bias=None, n_tags=None)"}
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip, nrms_hip
    t, c = torch.zeros(3, dtype=torch.int32), torch.ones(1, 2, dtype=torch.int32)
    for mod, who, why in ((hierec_hip, "hierec", "nrms_topk_grouped_dot"), (graph_hip, "graph", "click graph")):
        with pytest.raises(NotImplementedError, match=who + ": recommend_capped is not available") as e:
            mod.Model.recommend_capped(None, {}, 5, None, t, c)
        assert why in str(e.value)
    # the methods beside it are as they were
    assert str(inspect.signature(nrms_hip.Model.recommend_tagged)) == \
        "(self, batch, k, catalogue, item_tag, allow, exclude_history=True, *, item_bias=None)"


def test_model_cap_rows():
    """nrms_v0's own expansion of cap, on the CPU here: an int, [n_tags] and [B, n_tags]."""
    from pytorch_news_recommender_amd.model import nrms_hip
    f = nrms_hip.Model._cap_rows
    dev = torch.device("cpu")
    cap, n_tags = f(2, 19, 3, 10, dev, "recommend_capped")
    assert n_tags == 19 and cap.dtype == torch.int32 and tuple(cap.shape) == (3, 19) and (cap == 2).all()
    cap, n_tags = f(torch.tensor([1, -4, 2 ** 40]), None, 2, 10, dev, "recommend_capped")
    assert n_tags == 3 and cap.tolist() == [[1, 0, 2 ** 31 - 1]] * 2 and cap.is_contiguous()
    per_user = torch.tensor([[1, 2], [3, 4]], dtype=torch.int32)
    cap, n_tags = f(per_user, 2, 2, 10, dev, "recommend_capped")
    assert n_tags == 2 and cap.tolist() == per_user.tolist()
    for bad, nt in ((2, None), (2, 0), (2, 513), (True, 3), (2.0, 3), (torch.ones(3), None), (torch.ones(3, 2, dtype=torch.int32), None),
                    (torch.ones(2, 2, 2, dtype=torch.int32), None), (torch.ones(4, dtype=torch.int32), 5), ([1, 2], None)):
        with pytest.raises(_lib.NrmsError, match="cap|n_tags"):
            f(bad, nt, 2, 10, dev, "recommend_capped")
    rows = nrms_hip.Model._item_tag_rows(torch.arange(5), torch.zeros(5, 4), "recommend_capped")
    assert rows.tolist() == [1, 2, 3, 4]
    with pytest.raises(_lib.NrmsError, match="recommend_capped: item_tag"):
        nrms_hip.Model._item_tag_rows(torch.arange(4), torch.zeros(5, 4), "recommend_capped")


# ---- 4: the loop -------------------------------------------------------------------------------------------------------------
class _Capped(_Prior):
    """recommend_capped returns fixed ids per user so that the statistics can be worked out by hand."""
    ROWS = {2: [[1, 2, 3, 4], [5, 8, 11, -1]], 1: [[-1, -1, -1, -1]]}

    def recommend_capped(self, batch, k, catalogue, item_tag, cap, exclude_history=True, *, item_bias=None, n_tags=None):
        self.capped.append((item_tag, cap, item_bias))
        return torch.tensor(self.ROWS[batch["browsed_ids"].shape[0]]), None


def test_recommend_composes_caps_and_allow_and_reports(tmp_path):
    titles = torch.zeros(20, 3, dtype=torch.int64)
    batches = [{"candidate_ids": torch.tensor([[3, 4, 5], [6, 7, 0]]), "browsed_ids": torch.zeros(2, 2, dtype=torch.int64)},
               {"candidate_ids": torch.tensor([[8, 9, 1]]), "browsed_ids": torch.zeros(1, 2, dtype=torch.int64)}]
    tag = torch.arange(20, dtype=torch.int64) % 3
    allow = torch.tensor([[True, True, False], [True, False, False], [False, False, True]])
    rec = lambda m, **kw: train_eval.recommend(None, m, batches, titles, 4, out_file=str(tmp_path / "a.txt"), **kw)
    m = _Capped()
    m.capped = []
    p = torch.ones(20)
    out = rec(m, item_tag=tag, tag_caps=torch.tensor([2, 1, 5]), allow_tags=allow, item_bias=p, heldout=[[2, 9], [11], [7]])
    assert open(out).read().splitlines() == ["1 [1,2,3,4]", "2 [5,8,11]", "3 []"]
    assert len(m.capped) == 2 and all(c[0] is tag and c[2] is p for c in m.capped)
    # with allow_tags as well a closed tag becomes cap 0
    assert m.capped[0][1].tolist() == [[2, 1, 0], [2, 0, 0]] and m.capped[1][1].tolist() == [[0, 0, 5]]
    assert all(c[1].dtype == torch.int32 and c[1].is_contiguous() for c in m.capped)
    st = m.last_caps_stats
    # list 1: tags 1, 2, 0, 1 -> 3 distinct, largest share 2/4; list 2: tags 2, 2, 2 -> 1 distinct, share 1; list 3 is empty
    assert st["n_users"] == 2 and st["distinct_tags"] == 2.0 and st["largest_share"] == 0.75
    # held-out: 2 (place 2) and 9 (absent) for sample 1, 11 (place 3) for sample 2, 7 for the empty list
    assert st["n_heldout"] == 4 and st["hit"] == {1: 0.0, 4: 0.5} and abs(st["hit_se"][4] - 0.25) < 1e-12
    # caps alone: every sample the same row; per-sample rows; an int with allow_tags
    m.capped = []
    rec(m, item_tag=tag, tag_caps=np.array([2, 1, 5]))
    assert [c[1].tolist() for c in m.capped] == [[[2, 1, 5]] * 2, [[2, 1, 5]]] and "hit" not in m.last_caps_stats
    m.capped = []
    rec(m, item_tag=tag, tag_caps=torch.tensor([[1, 1, 1], [2, -2, 2], [3, 3, 3]]))
    assert [c[1].tolist() for c in m.capped] == [[[1, 1, 1], [2, 0, 2]], [[3, 3, 3]]]
    m.capped = []
    rec(m, item_tag=tag, tag_caps=2, allow_tags=allow)
    assert [c[1].tolist() for c in m.capped] == [[[2, 2, 0], [2, 0, 0]], [[0, 0, 2]]]
    # absent: no new keyword, the calls from before, the tag sets as before
    m.capped, m.calls = [], []
    rec(m)
    assert m.capped == [] and len(m.calls) == 2 and m.last_caps_stats is None
    rec(_Stub())
    with pytest.raises(AttributeError, match="recommend_capped"):
        rec(_Stub(), item_tag=tag, tag_caps=torch.tensor([1, 1, 1]))
    for kw, word in ((dict(tag_caps=torch.tensor([1, 1, 1])), "give item_tag"), (dict(item_tag=tag, tag_caps=2), "how many tags"),
                     (dict(item_tag=tag, tag_caps=torch.ones(3)), "tag_caps must be"),
                     (dict(item_tag=tag, tag_caps=torch.tensor([1, 1]), allow_tags=allow), "disagree on n_tags"),
                     (dict(item_tag=tag, tag_caps=torch.ones(2, 3, dtype=torch.int64)), "tag_caps rows"),
                     (dict(heldout=[[1]] * 3), "give tag_caps"),
                     (dict(item_tag=tag, tag_caps=torch.tensor([1, 1, 1]), diversity=0.5), "diversity"),
                     (dict(item_tag=tag, tag_caps=torch.tensor([1, 1, 1]), coarse=True), "coarse"),
                     (dict(item_tag=tag, tag_caps=torch.tensor([1, 1, 1]), explain=3), "explain"),
                     (dict(item_tag=tag, tag_caps=torch.tensor([1, 1, 1]), item_time=torch.arange(20, dtype=torch.int32),
                           request_time=np.array([1, 2, 3]), window_span=5), "window_span")):
        with pytest.raises(ValueError, match=word):
            rec(m, **kw)
    assert list(inspect.signature(train_eval.recommend).parameters)[-5:] == ["tag_caps", "heldout", "item_tag", "allow_tags", "explain"]


# ---- 5: the CLI's checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,want", [
    (["--recommend", "10", "--max_per_category", "2"], None),
    (["--recommend", "10", "--max_per_category", "1", "--mute_categories", "2", "--popularity_prior", "0.5", "--negatives", "catalogue"], None),
    (["--recommend", "10", "--max_per_category", "3", "--only_categories", "own"], None),
    (["--model", "nrms_v1", "--recommend", "10", "--max_per_category", "2"], None),
    (["--model", "nrms_naml", "--recommend", "10", "--max_per_category", "2"], None),
    (["--model", "nrms_bert", "--recommend", "10", "--max_per_category", "2"], None),
    (["--recommend", "10"], None),                                                                 # no flag: nothing to check
    (["--max_per_category", "2"], "--recommend"),
    (["--retrieval_metrics", "10", "--max_per_category", "2"], "--recommend"),
    (["--recommend", "10", "--max_per_category", "0"], "M must be >= 1"),
    (["--recommend", "10", "--max_per_category", "-3"], "M must be >= 1"),
    (["--model", "hierec", "--recommend", "10", "--max_per_category", "2"], "hierec"),
    (["--model", "graph", "--recommend", "10", "--max_per_category", "2"], "graph"),
    (["--recommend", "10", "--max_per_category", "2", "--diversity", "0.5"], "--diversity"),
    (["--recommend", "10", "--max_per_category", "2", "--coarse_catalogue"], "--coarse_catalogue"),
    (["--negatives", "catalogue", "--recommend", "10", "--max_per_category", "2", "--catalogue_window", "100"], "--catalogue_window"),
    (["--recommend", "10", "--max_per_category", "2", "--sections", "category"], "--sections"),
    (["--recommend_deep", "500", "--max_per_category", "2"], "--recommend"),
    (["--recommend", "10", "--recommend_deep", "500", "--max_per_category", "2"], "--recommend_deep"),
    (["--recommend", "10", "--max_per_category", "2", "--explain", "3"], "--explain"),
])
def test_check_caps_args(argv, want):
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(["--dataset", "synthetic"] + ([] if "--model" in argv else ["--model", "nrms_hip"]) + argv)
    if want is None:
        assert run_v0.check_caps_args(args) is None
        run_v0.check_tag_args(args)                                  # the flags beside it accept the combination
    else:
        with pytest.raises(SystemExit) as e:
            run_v0.check_caps_args(args)
        assert "--max_per_category" in str(e.value) and want in str(e.value)
