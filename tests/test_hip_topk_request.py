"""nrms_topk_dot_request / nrms_rank_dot_request on the GPU (one request through a time window, a tag set, per-user adjustments and
a cursor at once; include/nrms_hip.h): exact against tests/topk_request_ref.py on the lattice data of tests/topk_request_cases.py
for every subset of two, three and four parts at every point where the kernels change path, the consequences 1 to 8 the header
states on Gaussian and on lattice data, the buffer contract and the layers above (engine.top_k_request / rank_of_request,
Model.recommend_request / rank_targets_request).  Every comparison is exact: ids, ranks and score bits; the feature needs no
tolerance.  Parity is unpinned: the reference has no catalogue retrieval."""
import ctypes as C

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream, pack_tag_mask

from tests import topk_request_cases as cases
from tests import topk_request_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
_ENG = []


def _engine():
    if not _ENG:
        _ENG.append(NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), DEV))
    return _ENG[0]


def _t(a, dt):
    return None if a is None else torch.as_tensor(np.array(a)).to(dt).to(DEV).contiguous()


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what):
    for g, w, name in zip(got, want, ("first", "second")):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg="%s (%s output)" % (what, name))


def _kw(parts, after=None):
    """The keywords of engine.top_k_request / rank_of_request for the parts that are there."""
    kw = {}
    if parts.window is not None:
        kw.update(item_time=_t(parts.item_time, torch.int32), window=_t(parts.window, torch.int32))
    if parts.allow is not None:
        kw.update(item_tag=_t(parts.item_tag, torch.int32), n_tags=parts.n_tags, allow=_t(parts.allow, torch.bool))
    if parts.adj_ids is not None:
        kw.update(adj_ids=_t(parts.adj_ids, torch.int64), adj_delta=_t(parts.adj_delta, torch.float32))
    if after is not None:
        kw.update(after_scores=_t(after[0], torch.float32), after_ids=_t(after[1], torch.int64))
    return kw


def _topk(user, items, k, ex, bias, parts, after=None):
    s, ids = _engine().top_k_request(_t(user, torch.float32), _t(items, torch.float32), k, _t(ex, torch.int64),
                                     bias=_t(bias, torch.float32), **_kw(parts, after))
    return ids.cpu().numpy(), s.cpu().numpy()


def _rank(user, items, tg, ex, bias, parts):
    r, s = _engine().rank_of_request(_t(user, torch.float32), _t(items, torch.float32), _t(tg, torch.int64), _t(ex, torch.int64),
                                     bias=_t(bias, torch.float32), **_kw(parts))
    return r.cpu().numpy(), s.cpu().numpy()


# ---- exact on lattice data: every shape x every subset -----------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(cases.CASES)))
def test_exact_on_lattice_data(case):
    B, N, d, k, T, n_tags, E, n_ex, with_bias = cases.CASES[case]
    user, items, s, bias, parts, after, ex, tg = cases.lattice(*cases.CASES[case])
    for subset in cases.SUBSETS:
        p, a = cases.select(parts, after, subset)
        _same(_topk(user, items, k, ex, bias, p, a), ref.topk(s, bias, p, ex, k, a), "request top-k %s" % (subset,))
    for subset in cases.RANK_SUBSETS:
        p, _ = cases.select(parts, after, subset)
        got = _rank(user, items, tg, ex, bias, p)
        _same(got, ref.ranks(s, bias, p, ex, tg), "request rank %s" % (subset,))
        if T >= 8 and N >= 63:
            assert (got[0][:, 3] == 0).all() and (got[0][:, 5] == 0).all() and (got[1][:, 3] == -np.inf).all()
            if ex is not None:
                assert (got[0][:, 1] == 0).all()                                       # excluded and adjusted: excluded


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("with_ex", [False, True])
def test_every_subset_with_and_without_bias_and_excludes(with_bias, with_ex):
    """One mid-sized shape (two slices, two user tiles, P = 256), every subset, the four combinations of prior and exclude list."""
    shape = (33, 2049, 32, 65, 8, 19, 16, 5, True)
    user, items, s, bias, parts, after, ex, tg = cases.lattice(*shape)
    bias, ex = (bias if with_bias else None), (ex if with_ex else None)
    for subset in cases.SUBSETS:
        p, a = cases.select(parts, after, subset)
        _same(_topk(user, items, 65, ex, bias, p, a), ref.topk(s, bias, p, ex, 65, a), "request top-k %s" % (subset,))
    for subset in cases.RANK_SUBSETS:
        p, _ = cases.select(parts, after, subset)
        _same(_rank(user, items, tg, ex, bias, p), ref.ranks(s, bias, p, ex, tg), "request rank %s" % (subset,))


# ---- the consequences, on Gaussian and on lattice data -----------------------------------------------------------------------
SHAPE = (65, 2049, 60, 10, 8, 19, 16, 5, True)


def _data(kind, shape=SHAPE):
    """The lattice case `shape`, or the same parts over Gaussian users, items and prior."""
    user, items, s, bias, parts, after, ex, tg = cases.lattice(*shape)
    if kind == "gauss":
        rng = np.random.default_rng(11)
        user = rng.normal(size=user.shape).astype(np.float32)
        items = rng.normal(size=items.shape).astype(np.float32)
        nb = rng.normal(size=items.shape[0]).astype(np.float32)
        nb[np.isnan(bias)] = np.nan
        bias = nb
    return user, items, bias, parts, ex, tg


def _dev(user, items, bias, ex, tg):
    return _t(user, torch.float32), _t(items, torch.float32), _t(bias, torch.float32), _t(ex, torch.int64), _t(tg, torch.int64)


KINDS = ["gauss", "lattice"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [10, 193])
def test_neutral_parts_are_the_biased_call(kind, k):
    """1. All parts given but neutral by value: nrms_topk_dot_biased / nrms_rank_dot_biased bit for bit, on the REQ kernels."""
    user, items, bias, parts, ex, tg = _data(kind)
    B, N = user.shape[0], items.shape[0]
    eng = _engine()
    u, it, bi, exd, tgd = _dev(user, items, bias, ex, tg)
    neutral = ref.neutral(B, N)
    begin = (np.zeros(B, dtype=np.float32), np.full(B, ref.PAGE_BEGIN, dtype=np.int64))
    for b_ in (None, bi):
        _same(eng.top_k_request(u, it, k, exd, bias=b_, **_kw(neutral, begin)), eng.top_k(u, it, k, exd, bias=b_), "neutral top-k")
        _same(eng.rank_of_request(u, it, tgd, exd, bias=b_, **_kw(neutral)), eng.rank_of(u, it, tgd, exd, bias=b_), "neutral rank")


@pytest.mark.parametrize("kind", KINDS)
def test_one_live_part_is_its_own_call(kind):
    """2. One part live, the rest neutral by value (the REQ kernels) and, separately, null (forwarded): the part's own call."""
    user, items, bias, parts, ex, tg = _data(kind)
    B, N, k = user.shape[0], items.shape[0], 10
    eng = _engine()
    u, it, bi, exd, tgd = _dev(user, items, bias, ex, tg)
    neutral = ref.neutral(B, N)
    begin = (np.zeros(B, dtype=np.float32), np.full(B, ref.PAGE_BEGIN, dtype=np.int64))
    live = _kw(parts)
    first = eng.top_k_request(u, it, 7, exd, bias=bi, **_kw(cases.select(parts, None, ("window", "adjust"))[0]))
    cursor = (first[0][:, -1].cpu().numpy().copy(), first[1][:, -1].cpu().numpy().copy())
    cursor[1][3], cursor[1][5] = ref.PAGE_BEGIN, -1
    own = {
        "window": (lambda: eng.top_k(u, it, k, exd, bias=bi, item_time=live["item_time"], window=live["window"]),
                   lambda: eng.rank_of(u, it, tgd, exd, bias=bi, item_time=live["item_time"], window=live["window"])),
        "tags": (lambda: eng.top_k_tagged(u, it, k, live["item_tag"], parts.n_tags, live["allow"], exd, bias=bi),
                 lambda: eng.rank_of_tagged(u, it, tgd, live["item_tag"], parts.n_tags, live["allow"], exd, bias=bi)),
        "adjust": (lambda: eng.top_k_adjusted(u, it, k, live["adj_ids"], live["adj_delta"], exd, bias=bi),
                   lambda: eng.rank_of_adjusted(u, it, tgd, live["adj_ids"], live["adj_delta"], exd, bias=bi)),
        "cursor": (lambda: eng.top_k_after(u, it, k, _t(cursor[0], torch.float32), _t(cursor[1], torch.int64), exd, bias=bi), None),
    }
    for name in cases.PART_NAMES:
        p, a = cases.select(parts, cursor, (name,))
        filled = ref.Parts(*[x if x is not None and not (isinstance(x, int) and x == 0) else y for x, y in zip(p, neutral)])
        want_k, want_r = own[name]
        _same(eng.top_k_request(u, it, k, exd, bias=bi, **_kw(filled, a if a is not None else begin)), want_k(), name + " live, rest neutral")
        _same(eng.top_k_request(u, it, k, exd, bias=bi, **_kw(p, a)), want_k(), name + " live, rest null")
        if want_r is not None:
            _same(eng.rank_of_request(u, it, tgd, exd, bias=bi, **_kw(filled)), want_r(), name + " live, rest neutral (rank)")
            _same(eng.rank_of_request(u, it, tgd, exd, bias=bi, **_kw(p)), want_r(), name + " live, rest null (rank)")


@pytest.mark.parametrize("kind", KINDS)
def test_row_equals_the_biased_call_with_the_parts_as_bias(kind):
    """3. Without a prior, row b is nrms_topk_dot_biased at B = 1 with the deltas scattered and NaN where a part closes the news."""
    user, items, bias, parts, ex, tg = _data(kind)
    N, k = items.shape[0], 65
    eng = _engine()
    u, it, _, exd, _ = _dev(user, items, None, ex, tg)
    p, _ = cases.select(parts, None, ("window", "tags", "adjust"))
    ids, sc = _topk(user, items, k, ex, None, p)
    for b in (0, 1, 17, 31, 32, 63, 64):
        one = eng.top_k(u[b:b + 1].contiguous(), it, k, exd[b:b + 1].contiguous(), bias=_t(ref.request_as_bias(p, b, N), torch.float32))
        _same((one[1], one[0]), (ids[b:b + 1], sc[b:b + 1]), "row %d" % b)


@pytest.mark.parametrize("kind", KINDS)
def test_served_ids_rank_one_two_three(kind):
    """4. The served ids get ranks 1, 2, ... with the same parts; closed and excluded targets get 0."""
    user, items, bias, parts, ex, tg = _data(kind)
    k = 32
    for subset in cases.RANK_SUBSETS:
        p, _ = cases.select(parts, None, subset)
        ids, sc = _topk(user, items, k, ex, bias, p)
        r, rs = _rank(user, items, np.where(ids >= 0, ids, -1), ex, bias, p)
        want = np.where(ids >= 0, np.arange(1, k + 1)[None, :], 0)
        np.testing.assert_array_equal(r, want, err_msg=str(subset))
        np.testing.assert_array_equal(_bits(rs), _bits(sc), err_msg=str(subset))
        # up to 8 news per user that the window, the tags or the exclude list close (-1 where a user has fewer)
        open_ = ref.eligible(np.zeros((user.shape[0], items.shape[0]), dtype=np.float32), ref.Parts(*p[:5]), ex)
        closed = np.full((user.shape[0], 8), -1, dtype=np.int64)
        for b in range(user.shape[0]):
            c = np.nonzero(~open_[b])[0][:8]
            closed[b, :len(c)] = c
        assert (closed >= 0).sum() > 4 * user.shape[0]
        r, rs = _rank(user, items, closed, ex, bias, p)
        assert (r == 0).all() and (rs == -np.inf).all(), subset


@pytest.mark.parametrize("kind", KINDS)
def test_pages_chain_to_exhaustion(kind):
    """5. Pages of 7 chained by `after` are the k = 256 list's prefix and then -1: nothing repeated or skipped across ties."""
    shape = (33, 300, 32, 64, 8, 19, 16, 5, True)
    user, items, bias, parts, ex, tg = _data(kind, shape)
    eng = _engine()
    u, it, bi, exd, _ = _dev(user, items, bias, ex, tg)
    B = user.shape[0]
    window = np.array(parts.window)
    window[0] = (0, 20)                        # user 0's list, too, has to end inside 256: two thirds of 300 news
    parts = parts._replace(window=window)
    for subset in (("window", "tags", "adjust"), ("window", "tags"), ("window", "adjust")):
        p, _ = cases.select(parts, None, subset)
        kw = _kw(p)
        full_s, full_i = eng.top_k_request(u, it, 256, exd, bias=bi, **kw)
        lengths = (full_i >= 0).sum(dim=1)
        assert int(lengths.max()) < 256 and int(lengths.max()) > 100, "the list has to end inside 256 for the chain to reach its end"
        a_s = torch.zeros(B, device=DEV)
        a_i = torch.full((B,), ref.PAGE_BEGIN, dtype=torch.int64, device=DEV)
        got_s, got_i = [], []
        for _ in range(256 // 7 + 1):
            s_, i_ = eng.top_k_request(u, it, 7, exd, bias=bi, after_scores=a_s, after_ids=a_i, **kw)
            got_s.append(s_)
            got_i.append(i_)
            a_s, a_i = s_[:, -1].contiguous(), i_[:, -1].contiguous()
        got_s, got_i = torch.cat(got_s, dim=1), torch.cat(got_i, dim=1)
        assert got_i.shape[1] >= 256
        _same((got_i[:, :256], got_s[:, :256]), (full_i, full_s), "chained pages %s" % (subset,))
        assert (got_i[:, 256:] == -1).all()


@pytest.mark.parametrize("kind", KINDS)
def test_row_depends_on_its_own_user_only(kind):
    """6. Rows of a B = 65 call equal 65 calls at B = 1."""
    user, items, bias, parts, ex, tg = _data(kind)
    k = 10
    first = _topk(user, items, 5, ex, bias, cases.select(parts, None, ("window", "tags", "adjust"))[0])
    after = (first[1][:, -1].copy(), first[0][:, -1].copy())
    p, a = parts, after
    ids, sc = _topk(user, items, k, ex, bias, p, a)
    r, rs = _rank(user, items, tg, ex, bias, p)
    for b in range(user.shape[0]):
        pb = ref.Parts(p.item_time, p.window[b:b + 1], p.item_tag, p.n_tags, p.allow[b:b + 1], p.adj_ids[b:b + 1], p.adj_delta[b:b + 1])
        _same(_topk(user[b:b + 1], items, k, ex[b:b + 1], bias, pb, (a[0][b:b + 1], a[1][b:b + 1])), (ids[b:b + 1], sc[b:b + 1]), "row %d" % b)
        _same(_rank(user[b:b + 1], items, tg[b:b + 1], ex[b:b + 1], bias, pb), (r[b:b + 1], rs[b:b + 1]), "rank row %d" % b)


def test_wave_skips_stay_exact():
    """7. 64-item stretches closed to a whole 32-user block by the window alone, by the tags alone, and by both together half by
    each (which neither skip may take): exact, and the one user of the second block, open to everything, is served from all."""
    B, N, d, k = 33, 513, 32, 64
    user, items, s, bias, parts, after, ex, tg = cases.lattice(B, N, d, k, 8, 19, 16, 5, True)
    item_time = np.full(N, 15, dtype=np.int32)
    item_tag = (np.arange(N) % 2).astype(np.int32)
    window = np.tile(np.array([[10, 30]], dtype=np.int32), (B, 1))
    allow = np.zeros((B, 19), dtype=bool)
    allow[:, :2] = True
    item_time[64:128] = 5                          # closed to block 0 by its window hull
    item_tag[192:256] = 2                          # closed to block 0 by its tag bitmap
    item_time[320:384:2] = 5                       # half closed by the window ...
    item_tag[321:384:2] = 2                        # ... the other half by the tags: closed, but by neither part alone
    window[32] = (0, 30)
    allow[32] = True
    p = ref.Parts(item_time, window, item_tag, 19, allow, parts.adj_ids, parts.adj_delta)
    for q in (p, ref.Parts(*p[:5])):
        want = ref.topk(s, bias, q, ex, 256)
        assert all(((want[0][32] >= lo) & (want[0][32] < lo + 64)).any() for lo in (64, 192, 320))
        assert not any(((want[0][:32] >= lo) & (want[0][:32] < lo + 64)).any() for lo in (64, 192, 320))
        _same(_topk(user, items, 256, ex, bias, q), want, "wave skips, top-k")
        tgs = np.tile(np.array([[70, 200, 320, 321, 0, 1, 500, 130]], dtype=np.int64), (B, 1))
        _same(_rank(user, items, tgs, ex, bias, q), ref.ranks(s, bias, q, ex, tgs), "wave skips, rank")


# ---- argument errors: refused on the host, before any launch; only the return codes and messages are read ---------------------
def test_argument_errors():
    lib = _lib.load()
    B, N, d, k, T, E, n_tags = 4, 100, 8, 5, 3, 4, 19
    g = torch.Generator(device="cpu").manual_seed(1)
    user, items = torch.randn(B, d, generator=g).to(DEV), torch.randn(N, d, generator=g).to(DEV)
    it_time, win = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(B, 2, dtype=torch.int32, device=DEV)
    it_tag, allow = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(B, 1, dtype=torch.int32, device=DEV)
    aid, adl = torch.zeros(B, E, dtype=torch.int64, device=DEV), torch.zeros(B, E, device=DEV)
    a_s, a_i = torch.zeros(B, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    tg = torch.zeros(B, T, dtype=torch.int64, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.int64, device=DEV)
    sc, ids = torch.full((B, k), 5.0, device=DEV), torch.full((B, k), 5, dtype=torch.int64, device=DEV)
    r, rs = torch.full((B, T), 5, dtype=torch.int32, device=DEV), torch.full((B, T), 5.0, device=DEV)
    P = _lib.ptr
    base = dict(time=P(it_time), win=P(win), tag=P(it_tag), n_tags=n_tags, allow=P(allow), aid=P(aid), adl=P(adl), E=E, a_s=P(a_s), a_i=P(a_i))

    def topk(nbytes=None, **over):
        a = dict(base, **over)
        need = int(lib.nrms_topk_dot_request_workspace_bytes(B, C.c_int64(N), d, k))
        return lib.nrms_topk_dot_request(B, C.c_int64(N), d, k, P(user), P(items), None, a["time"], a["win"], a["tag"], a["n_tags"],
                                         a["allow"], a["aid"], a["adl"], a["E"], a["a_s"], a["a_i"], None, 0, P(sc), P(ids), P(ws),
                                         C.c_size_t(need if nbytes is None else need + nbytes), _stream())

    def rank(nbytes=None, **over):
        a = dict(base, **over)
        need = int(lib.nrms_rank_dot_request_workspace_bytes(B, C.c_int64(N), d, T, 0))
        return lib.nrms_rank_dot_request(B, C.c_int64(N), d, T, P(user), P(items), None, a["time"], a["win"], a["tag"], a["n_tags"],
                                         a["allow"], a["aid"], a["adl"], a["E"], P(tg), None, 0, P(r), P(rs), P(ws),
                                         C.c_size_t(need if nbytes is None else need + nbytes), _stream())

    pairs = [(dict(time=None), b"item_time is null"), (dict(win=None), b"window is null"), (dict(tag=None), b"item_tag is null"),
             (dict(allow=None), b"allow is null"), (dict(aid=None), b"adj_ids is null"), (dict(adl=None), b"adj_delta is null"),
             (dict(n_tags=0), b"n_tags must be"), (dict(n_tags=513), b"n_tags must be"), (dict(E=257), b"n_adjust must be")]
    for call, who, extra in ((topk, b"topk_dot_request: ", [(dict(a_s=None), b"after_scores is null"), (dict(a_i=None), b"after_ids is null")]),
                             (rank, b"rank_dot_request: ", [])):
        for kw, word in pairs + extra:
            assert call(**kw) == _lib.NRMS_EINVAL, (who, kw)
            msg = lib.nrms_last_error()
            assert msg.startswith(who) and word in msg, msg
        assert call(nbytes=-1) == _lib.NRMS_EWORKSPACE                   # one byte short
        assert lib.nrms_last_error().startswith(who)
    torch.cuda.synchronize()
    assert (sc == 5.0).all() and (ids == 5).all() and (r == 5).all() and (rs == 5.0).all()        # nothing was launched
    assert topk() == _lib.NRMS_OK and rank() == _lib.NRMS_OK
    # n_adjust == 0, or null lists, count as "no adjustments"
    assert topk(E=0) == _lib.NRMS_OK and topk(aid=None, adl=None) == _lib.NRMS_OK and rank(E=0, aid=None, adl=None) == _lib.NRMS_OK
    torch.cuda.synchronize()
    eng = _engine()
    with pytest.raises(_lib.NrmsError, match="item_tag and allow go together"):
        eng.top_k_request(user, items, k, item_tag=it_tag)
    with pytest.raises(_lib.NrmsError, match="adj_ids and adj_delta go together"):
        eng.rank_of_request(user, items, tg, adj_ids=aid)
    with pytest.raises(_lib.NrmsError, match="after_scores and after_ids go together"):
        eng.top_k_request(user, items, k, after_ids=a_i)
    with pytest.raises(_lib.NrmsError, match="item_time and window go together"):
        eng.top_k_request(user, items, k, window=win)


# ---- the buffer contract -----------------------------------------------------------------------------------------------------
def test_buffer_contract():
    """Outputs and the workspace at the queried size between guard bands, the workspace poisoned three ways; every part's arrays
    are guarded too, at exactly their sizes, and come back unchanged."""
    from tests.guarded import POISONS, Pool
    from tests.test_hip_buffer_contracts import dev, ok, refuses_undersized, three_poisons
    lib = _lib.load()
    shape = cases.CASES[3]
    B, N, d, k, T, n_tags, E, n_ex, with_bias = shape
    user, items, s, bias, parts, after, ex, tg = cases.lattice(*shape)
    ud, itd, tgd, exd = dev(np.array(user)), dev(np.array(items)), dev(np.array(tg), torch.int64), dev(ex, torch.int64)
    need_k = int(lib.nrms_topk_dot_request_workspace_bytes(B, C.c_int64(N), d, k))
    need_r = int(lib.nrms_rank_dot_request_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    assert need_k > 0 and need_r > 0
    packed = pack_tag_mask(torch.from_numpy(np.array(parts.allow))).reshape(-1)
    ins = {"item_time": (parts.item_time, torch.int32), "window": (parts.window, torch.int32), "item_tag": (parts.item_tag, torch.int32),
           "adj_ids": (parts.adj_ids, torch.int64), "adj_delta": (parts.adj_delta, torch.float32),
           "after_scores": (after[0], torch.float32), "after_ids": (after[1], torch.int64)}

    def run(poison):
        P = Pool(poison)
        for name, (a, dt) in ins.items():
            P.elems(name, a.size, dt, init=torch.from_numpy(np.array(a)).reshape(-1))
        P.elems("allow", packed.numel(), torch.int32, init=packed)
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, torch.int64), P.new("ws_topk", need_k)
        P.elems("ranks", B * T, torch.int32), P.elems("target_scores", B * T), P.new("ws_rank", need_r)

        def call_k(nbytes):
            return lib.nrms_topk_dot_request(B, C.c_int64(N), d, k, _lib.ptr(ud), _lib.ptr(itd), None, P["item_time"].ptr, P["window"].ptr,
                                             P["item_tag"].ptr, n_tags, P["allow"].ptr, P["adj_ids"].ptr, P["adj_delta"].ptr, E,
                                             P["after_scores"].ptr, P["after_ids"].ptr, _lib.ptr(exd), n_ex, P["top_scores"].ptr,
                                             P["top_ids"].ptr, P["ws_topk"].ptr, C.c_size_t(nbytes), _stream())

        def call_r(nbytes):
            return lib.nrms_rank_dot_request(B, C.c_int64(N), d, T, _lib.ptr(ud), _lib.ptr(itd), None, P["item_time"].ptr, P["window"].ptr,
                                             P["item_tag"].ptr, n_tags, P["allow"].ptr, P["adj_ids"].ptr, P["adj_delta"].ptr, E,
                                             _lib.ptr(tgd), _lib.ptr(exd), n_ex, P["ranks"].ptr, P["target_scores"].ptr,
                                             P["ws_rank"].ptr, C.c_size_t(nbytes), _stream())

        names = list(ins) + ["allow"]
        snap = [P[n].snapshot() for n in names]
        ok(call_k(need_k), "nrms_topk_dot_request")
        P.intact("nrms_topk_dot_request")
        ok(call_r(need_r), "nrms_rank_dot_request")
        P.intact("nrms_rank_dot_request")
        assert all(P[n].unchanged_since(sn) for n, sn in zip(names, snap))
        if poison == POISONS[0]:
            keep = {n: P[n].numpy() for n in ("top_scores", "top_ids", "ranks", "target_scores")}
            refuses_undersized(call_k, P, need_k, "nrms_topk_dot_request")
            refuses_undersized(call_r, P, need_r, "nrms_rank_dot_request")
            assert all(np.array_equal(_bits(keep[n]), _bits(P[n].numpy())) for n in keep)
        return {"ids": P["top_ids"].numpy((B, k)), "scores": P["top_scores"].numpy((B, k)), "ranks": P["ranks"].numpy((B, T)),
                "tscores": P["target_scores"].numpy((B, T))}

    out = three_poisons(run, "the request calls")[POISONS[0]]
    _same((out["ids"], out["scores"]), ref.topk(s, None, parts, ex, k, after), "request top-k between guard bands")
    _same((out["ranks"], out["tscores"]), ref.ranks(s, None, parts, ex, tg), "request rank between guard bands")


# ---- the models --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_models_recommend_and_rank_request(kind):
    """Model.recommend_request / rank_targets_request equal the engine call on the model's own user vectors (news id n is row
    n - 1 of the catalogue without its padding row), and the served ids rank 1, 2, ..."""
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model(kind)
    N = cat.shape[0]
    rng = np.random.default_rng(7)
    prior = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(DEV)
    item_time = torch.from_numpy(rng.integers(0, 30, size=N).astype(np.int32)).to(DEV)
    item_tag = torch.from_numpy(rng.integers(0, 7, size=N).astype(np.int64)).to(DEV)
    E, k = 12, 20
    eng = model._engine
    batch = batches[0]
    B = torch.as_tensor(batch["browsed_ids"]).shape[0]
    lo = rng.integers(0, 11, size=B)
    window = torch.from_numpy(np.stack([lo, lo + 20], axis=1).astype(np.int32)).to(DEV)
    allow = torch.from_numpy(rng.random((B, 7)) < 0.7).to(DEV)
    news = rng.integers(1, N, size=(B, E)).astype(np.int64)
    news[:, 0], news[:, 1] = 0, N + 5
    delta = (rng.integers(-20, 21, size=(B, E)) * 0.25).astype(np.float32)
    delta[:, 4] = np.nan
    adjust = (torch.from_numpy(news).to(DEV), torch.from_numpy(delta).to(DEV))
    parts = dict(item_time=item_time, window=window, item_tag=item_tag, allow=allow, adjust=adjust)
    ids, sc = model.recommend_request(batch, k, cat, item_bias=prior, **parts)
    user, c, exclude = model._catalogue_query(batch, cat, True, "test")
    want_s, want_i = eng.top_k_request(user, c[1:], k, exclude, bias=prior[1:].contiguous(), item_time=item_time[1:].contiguous(),
                                       window=window, item_tag=item_tag[1:].contiguous(), n_tags=7, allow=allow,
                                       adj_ids=(adjust[0] - 1).contiguous(), adj_delta=adjust[1])
    assert torch.equal(ids, torch.where(want_i >= 0, want_i + 1, want_i)) and torch.equal(sc.view(torch.int32), want_s.view(torch.int32))
    assert int((ids > 0).sum()) > 0
    r, rs = model.rank_targets_request(batch, ids, cat, item_bias=prior, **parts)
    want = torch.where(ids > 0, torch.arange(1, k + 1, dtype=torch.int32, device=DEV).expand(B, k), torch.zeros((), dtype=torch.int32, device=DEV))
    assert torch.equal(r, want) and torch.equal(rs.view(torch.int32), sc.view(torch.int32))
    # the second page follows the first
    ids2, sc2 = model.recommend_request(batch, k, cat, item_bias=prior, after=(ids[:, -1], sc[:, -1]), **parts)
    both_i, both_s = model.recommend_request(batch, 2 * k, cat, item_bias=prior, **parts)
    assert torch.equal(torch.cat([ids, ids2], dim=1), both_i) and torch.equal(torch.cat([sc, sc2], dim=1).view(torch.int32), both_s.view(torch.int32))
    # no part: recommend, bit for bit
    a, b_ = model.recommend_request(batch, k, cat), model.recommend(batch, k, cat)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1].view(torch.int32), b_[1].view(torch.int32))
    with pytest.raises(_lib.NrmsError, match="item_tag and allow go together"):
        model.recommend_request(batch, k, cat, item_tag=item_tag)
    model.check_recommend_ids()


def test_hierec_and_graph_refuse():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    for mod, name in ((hierec_hip, "hierec"), (graph_hip, "graph")):
        with pytest.raises(NotImplementedError, match=name + ": recommend_request is not available"):
            mod.Model.recommend_request(None, {}, 5, None)
        with pytest.raises(NotImplementedError, match=name + ": rank_targets_request is not available"):
            mod.Model.rank_targets_request(None, {}, None, None)
