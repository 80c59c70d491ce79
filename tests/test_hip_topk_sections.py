"""nrms_topk_sections_dot on the GPU (include/nrms_hip.h): exact against the numpy restatement of its contract
(tests/topk_sections_ref.py) on tie-heavy lattice data over awkward partitions, at every slice length, bit-identity with
nrms_topk_dot / nrms_topk_dot_biased per section, invariance, the buffer contract between guard bands, the degenerate cases, and
the front page of nrms_v0 and nrms_naml built on it (Model.section_catalogue / recommend_sections,
train_eval.recommend_sections)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream
from tests.guarded import POISONS, Pool, assert_same_bits
from tests.topk_sections_ref import topk_sections_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
_ENG = []


def _engine():
    if not _ENG:
        _ENG.append(NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), DEV))
    return _ENG[0]


def _dev(x, dt):
    return None if x is None else torch.as_tensor(x).to(DEV, dtype=dt).contiguous()


def _sections(user, items, ids, ptr, k, exclude=None, bias=None, slice_tiles=0, eng=None):
    s, i = (eng or _engine()).top_k_sections(_dev(user, torch.float32), _dev(items, torch.float32), _dev(ids, torch.int32),
                                             _dev(ptr, torch.int64), k, _dev(exclude, torch.int64), _dev(bias, torch.float32),
                                             slice_tiles)
    return s.cpu().numpy(), i.cpu().numpy()


def _assert_exact(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0].view(np.int32), want[0].view(np.int32))


def _same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


SHORT_RUN = [1, 0, 2, 5, 0, 3]          # six consecutive sections shorter than one 32-row tile
LONG = 300                              # longer than 2 * slice_tiles * 32 rows at slice_tiles = 2


def _partition(rng, N):
    """Section sizes with empty sections, 1-item sections and sections shorter than / straddling 32- and 64-row tiles,
    shuffled; then SHORT_RUN and LONG go in at random places, so that both facts the slice tests rely on hold."""
    sizes = [0, 1, 0, 31, 32, 33, 1, 63, 64, 65, 0, 2, 97, 5]
    room = N - LONG - sum(SHORT_RUN)
    while sum(sizes) < room:
        sizes.append(int(rng.choice([0, 1, 3, 17, 40, 70, 129])))
    over = sum(sizes) - room
    for j in range(len(sizes) - 1, -1, -1):              # trim to N
        cut = min(over, sizes[j])
        sizes[j] -= cut
        over -= cut
    rng.shuffle(sizes)
    sizes = list(sizes)
    sizes.insert(int(rng.integers(0, len(sizes) + 1)), LONG)
    at = int(rng.integers(0, len(sizes) + 1))
    sizes[at:at] = SHORT_RUN                             # after LONG, so that the run stays in one piece
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert ptr[-1] == N
    return ptr


def _int_case(B, N, d, seed, n_ex=50, bias=None):
    """Lattice data: NaN rows, shuffled sparse ids, exclude lists with -1, an id past the range, 1 << 40 and a duplicate."""
    rng = np.random.default_rng(seed)
    ptr = _partition(rng, N)
    user = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    items[rng.choice(N, size=max(1, N // 97), replace=False)] = np.nan
    ids = rng.permutation(4 * N)[:N].astype(np.int32)
    ex = ids[rng.integers(0, N, size=(B, n_ex))].astype(np.int64)
    ex[:, 0], ex[:, 1], ex[:, 2], ex[:, 3] = -1, 4 * N + 7, 1 << 40, ex[:, 4]
    bv = None
    if bias == "lattice":
        bv = rng.integers(-5, 6, size=N).astype(np.float32)
    elif bias == "special":
        bv = rng.integers(-5, 6, size=N).astype(np.float32)
        pick = rng.choice(N, size=3 * (N // 40), replace=False).reshape(3, -1)
        bv[pick[0]], bv[pick[1]], bv[pick[2]] = np.nan, -np.inf, np.inf
    return user, items, ids, ptr, ex, bv


# ---- exact against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7, 64, 65, 192, 193, 256])
def test_exact_with_ties_nan_and_awkward_sections(k):
    for bias in (None, "lattice"):
        user, items, ids, ptr, ex, bv = _int_case(37, 3001, 33, seed=k, bias=bias)
        _assert_exact(_sections(user, items, ids, ptr, k, ex, bv), topk_sections_ref(user, items, ids, ptr, k, ex, bv))


@pytest.mark.parametrize("d", [1, 3, 4, 31, 33, 300])
def test_exact_at_every_width(d):
    user, items, ids, ptr, ex, bv = _int_case(35, 2003, d, seed=100 + d, n_ex=70 if d % 2 else 50, bias="lattice")
    _assert_exact(_sections(user, items, ids, ptr, 100, ex, bv), topk_sections_ref(user, items, ids, ptr, 100, ex, bv))
    _assert_exact(_sections(user, items, ids, ptr, 7), topk_sections_ref(user, items, ids, ptr, 7))


@pytest.mark.parametrize("B", [1, 31, 32, 33])
def test_exact_at_every_user_tile_edge(B):
    user, items, ids, ptr, ex, bv = _int_case(B, 1000, 33, seed=200 + B, n_ex=70, bias="lattice")
    _assert_exact(_sections(user, items, ids, ptr, 20, ex, bv), topk_sections_ref(user, items, ids, ptr, 20, ex, bv))


@pytest.mark.parametrize("k", [5, 200])
def test_bias_with_nan_and_infinities(k):
    user, items, ids, ptr, ex, bv = _int_case(37, 3001, 33, seed=300 + k, bias="special")
    assert np.isnan(bv).any() and np.isneginf(bv).any() and np.isposinf(bv).any()
    got = _sections(user, items, ids, ptr, k, ex, bv)
    _assert_exact(got, topk_sections_ref(user, items, ids, ptr, k, ex, bv))
    blocked = ids[np.isnan(bv)]
    assert not np.isin(got[1], blocked).any()                       # a NaN prior is a block-list for every user
    # NULL and all-zero priors: the same ids and score bits
    _assert_exact(_sections(user, items, ids, ptr, k, ex, np.zeros_like(bv)), _sections(user, items, ids, ptr, k, ex))


# ---- the slice logic at small shapes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,bias", [(7, None), (100, "lattice"), (193, "special")])
def test_result_does_not_depend_on_the_slice_length(k, bias):
    user, items, ids, ptr, ex, bv = _int_case(37, 3001, 33, seed=400 + k, bias=bias)
    sizes = np.diff(ptr)
    short = sizes < 32
    run = max(len(r) for r in "".join("x" if v else " " for v in short).split())
    assert run >= 5                                                 # consecutive sections that share no tile and no slice
    assert sizes.max() > 2 * 2 * 32                                 # at slice_tiles = 2 a section of more than two slices
    assert (sizes == 97).any()                                      # at slice_tiles = 1 it merges 4 one-tile lists
    want = topk_sections_ref(user, items, ids, ptr, k, ex, bv)
    for slice_tiles in (0, 1, 2, 5, 1 << 20):
        _assert_exact(_sections(user, items, ids, ptr, k, ex, bv, slice_tiles), want)


# ---- against the existing calls (Gaussian data: this pins the score bits) -------------------------------------------------
def _gauss(B, N, d, n_ex=50, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    user = torch.randn(B, d, device=DEV, generator=g)
    items = torch.randn(N, d, device=DEV, generator=g)
    ex = torch.randint(0, N, (B, n_ex), device=DEV, generator=g)
    return user, items, ex, g


def _skewed(N, G, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.zipf(1.6, size=G).astype(np.float64)
    sizes = np.floor(w / w.sum() * N).astype(np.int64)
    sizes[np.argmax(sizes)] += N - sizes.sum()
    return torch.as_tensor(np.concatenate([[0], np.cumsum(sizes)]), device=DEV)


def test_one_section_is_bitwise_nrms_topk_dot():
    user, items, ex, _ = _gauss(70, 20000, 64)
    eng = _engine()
    N = items.shape[0]
    for k in (10, 100):
        s0, i0 = eng.top_k(user, items, k, ex)
        s1, i1 = eng.top_k_sections(user, items, torch.arange(N, device=DEV, dtype=torch.int32), torch.tensor([0, N], device=DEV),
                                    k, ex)
        assert s1.shape == (70, 1, k) and _same((s0, i0), (s1[:, 0], i1[:, 0]))


@pytest.mark.parametrize("biased", [False, True])
def test_every_row_is_topk_dot_over_its_section(biased):
    B, N, d, G, k = 70, 20000, 64, 40, 100
    user, items, _, g = _gauss(B, N, d, seed=2)
    ptr = _skewed(N, G, seed=2)
    ptl = ptr.tolist()
    # sparse ids, ascending inside every section: the row order of a section is its id order, so even ties agree
    ids = torch.randperm(4 * N, device=DEV, generator=g)[:N]
    ids = torch.cat([ids[lo:hi].sort().values for lo, hi in zip(ptl[:-1], ptl[1:])])
    ex = ids[torch.randint(0, N, (B, 50), device=DEV, generator=g)]
    bias = torch.randn(N, device=DEV, generator=g) if biased else None
    eng = _engine()
    s, i = eng.top_k_sections(user, items, ids.to(torch.int32), ptr, k, ex, bias=bias)
    pos = torch.full((4 * N,), -1, dtype=torch.int64, device=DEV)
    for gi in range(G):
        lo, hi = ptl[gi], ptl[gi + 1]
        pos.fill_(-1)
        pos[ids[lo:hi]] = torch.arange(hi - lo, device=DEV)
        gs, gidx = eng.top_k(user, items[lo:hi].contiguous(), k, pos[ex].contiguous(),
                             bias=None if bias is None else bias[lo:hi].contiguous())
        gid = torch.where(gidx >= 0, ids[lo:hi][gidx.clamp(min=0)] if hi > lo else gidx, gidx)
        assert _same((gs, gid), (s[:, gi], i[:, gi])), gi


# ---- invariance -----------------------------------------------------------------------------------------------------------
def test_invariance():
    B, N, d, G, k = 200, 20000, 64, 40, 100
    user, items, _, g = _gauss(B, N, d, seed=1)
    ptr = _skewed(N, G, seed=1)
    ids = torch.randperm(4 * N, device=DEV, generator=g)[:N].to(torch.int32)
    ex = ids[torch.randint(0, N, (B, 50), device=DEV, generator=g)].long()
    bias = torch.randn(N, device=DEV, generator=g)
    eng = _engine()
    run = lambda **kw: eng.top_k_sections(user, items, ids, ptr, k, ex, bias=bias, **kw)
    base = run()
    assert _same(base, run())                                                           # the run
    # what the workspace held
    for fill in (-1, 0):
        eng._bufs["topk_ws"].fill_(fill)
        assert _same(base, run())
    # unrelated calls on the same engine in between
    eng.top_k(user, items, 33, ex)
    eng.top_k_grouped(torch.randn(B, 3, d, device=DEV, generator=g), items, ids,
                      torch.tensor([0, 100, 100, N], device=DEV), 17, ex)
    assert _same(base, run())
    # the batch: users split at 123
    a = eng.top_k_sections(user[:123].contiguous(), items, ids, ptr, k, ex[:123].contiguous(), bias=bias)
    b = eng.top_k_sections(user[123:].contiguous(), items, ids, ptr, k, ex[123:].contiguous(), bias=bias)
    assert _same(base, (torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]])))
    # k: the first 50 columns of k = 100 are k = 50
    s50 = eng.top_k_sections(user, items, ids, ptr, 50, ex, bias=bias)
    assert _same((base[0][:, :, :50].contiguous(), base[1][:, :, :50].contiguous()), s50)
    # the layout: sections in reverse order, rows shuffled inside each section
    ptl = ptr.tolist()
    rows, ptr2, order = [], [0], list(range(G))[::-1]
    for gi in order:
        lo, hi = ptl[gi], ptl[gi + 1]
        rows.append(lo + torch.randperm(hi - lo, device=DEV, generator=g))
        ptr2.append(ptr2[-1] + hi - lo)
    rows = torch.cat(rows)
    r = eng.top_k_sections(user, items[rows].contiguous(), ids[rows].contiguous(), torch.tensor(ptr2, device=DEV), k, ex,
                           bias=bias[rows].contiguous())
    assert _same(base, (r[0][:, order].contiguous(), r[1][:, order].contiguous()))
    # what other sections hold: the first 7 sections alone
    cut = ptl[7]
    r = eng.top_k_sections(user, items[:cut].contiguous(), ids[:cut].contiguous(), ptr[:8].contiguous(), k, ex,
                           bias=bias[:cut].contiguous())
    assert _same((base[0][:, :7].contiguous(), base[1][:, :7].contiguous()), r)
    # a forced small chunk cap: users in many chunks
    old = eng.retrieval_chunk_bytes
    try:
        eng.retrieval_chunk_bytes = eng.lib.nrms_topk_sections_dot_workspace_bytes(40, N, d, k, G, 0)
        assert eng.lib.nrms_topk_sections_dot_workspace_bytes(B, N, d, k, G, 0) > eng.retrieval_chunk_bytes
        assert _same(base, run())
    finally:
        eng.retrieval_chunk_bytes = old


# ---- the buffer contract --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_tiles", [0, 2])
def test_outputs_and_workspace_between_guard_bands(slice_tiles):
    B, N, d, k = 37, 3001, 33, 65
    user, items, ids, ptr, ex, bv = _int_case(B, N, d, seed=500, bias="lattice")
    G = len(ptr) - 1
    lib = _engine().lib
    t = dict(user=_dev(user, torch.float32), items=_dev(items, torch.float32), ids=_dev(ids, torch.int32), ptr=_dev(ptr, torch.int64),
             ex=_dev(ex, torch.int64), bias=_dev(bv, torch.float32))
    need = lib.nrms_topk_sections_dot_workspace_bytes(B, N, d, k, G, slice_tiles)
    assert need > 0

    def call(pool, nbytes):
        return lib.nrms_topk_sections_dot(B, C.c_int64(N), d, k, G, slice_tiles, _lib.ptr(t["user"]), _lib.ptr(t["items"]),
                                          _lib.ptr(t["ids"]), _lib.ptr(t["ptr"]), _lib.ptr(t["bias"]), _lib.ptr(t["ex"]),
                                          ex.shape[1], pool["scores"].ptr, pool["ids"].ptr, pool["ws"].ptr, C.c_size_t(nbytes),
                                          _stream())

    runs = {}
    for poison in POISONS:
        pool = Pool(poison)
        pool.new("ws", need)
        pool.elems("scores", B * G * k, torch.float32)
        pool.elems("ids", B * G * k, torch.int64)
        _lib.check(call(pool, need), "nrms_topk_sections_dot")
        pool.intact("nrms_topk_sections_dot")
        runs[poison] = {"scores": pool["scores"].numpy((B, G, k)), "ids": pool["ids"].numpy((B, G, k))}
    assert_same_bits(runs, "nrms_topk_sections_dot")
    _assert_exact((runs[POISONS[0]]["scores"], runs[POISONS[0]]["ids"]), topk_sections_ref(user, items, ids, ptr, k, ex, bv))
    # one byte short: refused, nothing written
    pool = Pool(POISONS[0])
    pool.new("ws", need)
    pool.elems("scores", B * G * k, torch.float32)
    pool.elems("ids", B * G * k, torch.int64)
    snap = pool.snapshot()
    assert call(pool, need - 1) == _lib.NRMS_EWORKSPACE
    pool.assert_unchanged(snap, "a refused nrms_topk_sections_dot")
    pool.intact("a refused nrms_topk_sections_dot")


# ---- degenerate cases -----------------------------------------------------------------------------------------------------
def test_degenerate_cases():
    rng = np.random.default_rng(9)
    B, d = 5, 12
    user = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(40, d)).astype(np.float32)
    ids = (rng.permutation(200)[:40]).astype(np.int32)
    # N = 0: all-padding rows
    s, i = _sections(user, items[:0], ids[:0], np.zeros(4, np.int64), 5)
    assert s.shape == (B, 3, 5) and (i == -1).all() and np.isneginf(s).all()
    # B = 0
    s, i = _sections(user[:0], items, ids, [0, 10, 40], 5)
    assert s.shape == (0, 2, 5) and i.shape == (0, 2, 5)
    # all sections empty but one; k above every section's size
    for ptr in ([0, 0, 0, 40, 40], [0, 3, 3, 4, 40]):
        _assert_exact(_sections(user, items, ids, ptr, 64), topk_sections_ref(user, items, ids, ptr, 64))
    s, i = _sections(user, items, ids, [0, 0, 0, 40, 40], 64)
    assert (i[:, [0, 1, 3]] == -1).all() and (i[:, 2, :40] >= 0).all() and (i[:, 2, 40:] == -1).all()
    # user 1 excludes the whole of section 1: an all-padding row there, every other row untouched
    ptr = [0, 9, 20, 40]
    ex = np.full((B, 11), -1, np.int64)
    ex[1] = ids[9:20]
    got, free = _sections(user, items, ids, ptr, 8, ex), _sections(user, items, ids, ptr, 8)
    _assert_exact(got, topk_sections_ref(user, items, ids, ptr, 8, ex))
    assert (got[1][1, 1] == -1).all() and np.isneginf(got[0][1, 1]).all()
    keep = np.ones((B, 3), bool)
    keep[1, 1] = False
    _assert_exact((got[0][keep], got[1][keep]), (free[0][keep], free[1][keep]))
    # refused
    with pytest.raises(_lib.NrmsError, match="k <= 256"):
        _sections(user, items, ids, ptr, 257)
    with pytest.raises(_lib.NrmsError, match="G=0"):
        _sections(user, items[:0], ids[:0], [0], 5)


# ---- models ---------------------------------------------------------------------------------------------------------------
def _model(kind):
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    from pytorch_news_recommender_amd.model import nrms_hip, nrms_naml_hip
    torch.manual_seed(0)
    cfg = Config(kind)
    cfg.__nrms__()
    cfg.n_words, cfg.n_words_title, cfg.n_words_abst, cfg.history_len, cfg.sample_size, cfg.max_candidate_size = 600, 12, 16, 10, 4, 24
    cfg.word_embed_size, cfg.num_attention_heads, cfg.title_heads_num, cfg.query_vector_dim = 60, 6, 3, 32
    cfg.category_nums, cfg.subcategory_nums = 8, 40
    cfg.batch_size, cfg.dropout = 32, 0.2
    corpus = SyntheticMind(cfg, n_news=200, n_topics=4, seed=1)
    table = corpus.embedding_table(cfg.word_embed_size)
    if kind == "nrms_naml":
        cfg.user_heads_num, cfg.cate_embed_size, cfg.query_vector_dim_large = 4, 20, 40
        cfg.news_feature_size = 2 * cfg.word_embed_size + 2 * cfg.cate_embed_size
        model = nrms_naml_hip.Model(cfg, pretrained_word_embedding=table).to("cuda")
    else:
        model = nrms_hip.Model(cfg, pretrained_word_embedding=table).to("cuda")
    samples, _ = corpus.eval_samples(64, max_shown=20)
    feed = DeviceFeed(cfg, samples, type=1, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict,
                      batch_size=cfg.batch_size, device=DEV)
    info = feed.news_info()
    cat = model.encode_catalogue(feed.titles, **info) if kind == "nrms_naml" else model.encode_catalogue(feed.titles)
    return cfg, model, feed, info, cat


def _filtered(full_ids, full_scores, categ, G, k):
    """recommend's full ranking cut into sections: per (user, section) its first k entries of that section."""
    ids, sc = full_ids.cpu().numpy(), full_scores.cpu().numpy()
    categ = categ.cpu().numpy()
    out_i = np.full((ids.shape[0], G, k), -1, np.int64)
    out_s = np.full((ids.shape[0], G, k), -np.inf, np.float32)
    for b in range(ids.shape[0]):
        live = ids[b] >= 0
        for g in range(G):
            at = np.nonzero(live & (categ[np.where(live, ids[b], 0)] == g))[0][:k]
            out_i[b, g, :len(at)], out_s[b, g, :len(at)] = ids[b, at], sc[b, at]
    return out_s, out_i


@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_recommend_sections_is_recommend_filtered_by_section(kind):
    cfg, model, feed, info, cat = _model(kind)
    G, k, N = cfg.category_nums, 6, feed.titles.shape[0]
    assert N - 1 <= 256
    sectioned = model.section_catalogue(cat, info["categ"], G)
    assert (np.diff(sectioned.section_ptr.cpu().numpy()) > k).sum() >= 2            # sections that are cut at k
    prior = (0.5 * torch.log1p(torch.arange(N, device=DEV, dtype=torch.float32) % 7)).contiguous()
    prior[5] = float("nan")
    batches = list(feed)
    batches.append({"browsed_ids": torch.zeros(3, cfg.history_len, dtype=torch.int64, device=DEV)})     # users without clicks
    for batch in batches:
        for exclude_history in (True, False):
            for bias in (None, prior):
                kw = {} if bias is None else {"item_bias": bias}
                full_i, full_s = model.recommend(batch, N - 1, cat, exclude_history, **kw)
                ids, scores = model.recommend_sections(batch, k, sectioned, exclude_history, **kw)
                assert ids.shape == scores.shape == (full_i.shape[0], G, k) and ids.dtype == torch.int64
                _assert_exact((scores.cpu().numpy(), ids.cpu().numpy()), _filtered(full_i, full_s, info["categ"], G, k))
                assert not (ids == 0).any() and (bias is None or not (ids == 5).any())
    model.check_recommend_ids()
    bad = {"browsed_ids": torch.tensor([[1, 2, N + 5]], device=DEV)}
    model.recommend_sections(bad, k, sectioned)
    with pytest.raises(_lib.NrmsError, match="outside the catalogue"):
        model.check_recommend_ids()
    with pytest.raises(_lib.NrmsError, match="SectionedCatalogue"):
        model.recommend_sections(batches[0], k, cat)


def test_train_eval_recommend_sections_writes_one_line_per_impression_and_section(tmp_path):
    cfg, model, feed, info, cat = _model("nrms_v0")
    G, k = cfg.category_nums, 4
    out = train_eval.recommend_sections(cfg, model, feed, feed.titles, k, (info["categ"], G), out_file=str(tmp_path / "sec.txt"))
    sectioned = model.section_catalogue(cat, info["categ"], G)
    want = []
    n = 0
    for batch in feed:
        ids, _ = model.recommend_sections(batch, k, sectioned)
        for row in ids.cpu().tolist():
            n += 1
            for g, sec in enumerate(row):
                got = [v for v in sec if v >= 0]
                if got:
                    want.append((n, g, got))
    lines = open(out).read().splitlines()
    assert n == feed.n and len(lines) == len(want) and len(want) < n * G              # empty sections are skipped
    for ln, (i, g, got) in zip(lines, want):
        m = re.fullmatch(r"(\d+) (\d+) \[(\d+(?:,\d+)*)\]", ln)
        assert m and (int(m.group(1)), int(m.group(2))) == (i, g), ln
        assert [int(v) for v in m.group(3).split(",")] == got


def test_hierec_and_graph_refuse():
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    cfg = Config("hierec")
    cfg.__nrms__()
    cfg.word_embed_size, cfg.num_attention_heads, cfg.query_vector_dim = 60, 6, 32
    cfg.category_nums, cfg.subcategory_nums = 8, 30
    table = np.random.default_rng(0).normal(0, 0.4, size=(50, 60)).astype(np.float32)
    m = hierec_hip.Model(cfg, pretrained_word_embedding=table).to("cuda")
    assert not m.CATALOGUE_SECTIONS and not graph_hip.Model.CATALOGUE_SECTIONS
    with pytest.raises(NotImplementedError, match="hierec: recommend_sections is not available"):
        m.recommend_sections({"browsed_ids": torch.zeros(2, 3, dtype=torch.int64, device=DEV)}, 5, None)
    with pytest.raises(NotImplementedError, match="graph: recommend_sections is not available"):
        graph_hip.Model.recommend_sections(None, {}, 5, None)
