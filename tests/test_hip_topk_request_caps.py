"""nrms_topk_dot_request_capped on the GPU (per-category caps through the request: caps with a time window, a tag set, per-user
adjustments and a cursor; include/nrms_hip.h): exact against tests/topk_request_caps_ref.py on the lattice data of
tests/topk_request_caps_cases.py for every subset of the four parts at every point where the kernels change path, the consequences 1
to 7 the header states on Gaussian data, pages chained through remaining_caps, the split of a batch, the buffer contract and the
layers above (engine.top_k_request_capped, Model.recommend_request_capped, run_v0 --request_max_per_category).  Every comparison is
exact: ids and score bits; the feature needs no tolerance.  Parity is unpinned: the reference has no catalogue retrieval."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream, pack_tag_mask, remaining_caps

from tests import topk_caps_ref
from tests import topk_request_caps_cases as cases
from tests import topk_request_caps_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    """The keywords of engine.top_k_request_capped for the parts that are there."""
    kw = {}
    if parts.window is not None:
        kw.update(item_time=_t(parts.item_time, torch.int32), window=_t(parts.window, torch.int32))
    if parts.allow is not None:
        kw.update(allow=_t(parts.allow, torch.bool))
    if parts.adj_ids is not None:
        kw.update(adj_ids=_t(parts.adj_ids, torch.int64), adj_delta=_t(parts.adj_delta, torch.float32))
    if after is not None:
        kw.update(after_scores=_t(after[0], torch.float32), after_ids=_t(after[1], torch.int64))
    return kw


def _topk(user, items, k, item_tag, n_tags, cap, ex, bias, parts, after=None):
    s, ids = _engine().top_k_request_capped(_t(user, torch.float32), _t(items, torch.float32), k, _t(item_tag, torch.int32), n_tags,
                                            _t(cap, torch.int32), _t(ex, torch.int64), bias=_t(bias, torch.float32), **_kw(parts, after))
    return ids.cpu().numpy(), s.cpu().numpy()


# ---- exact on lattice data: every shape x every subset -----------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(cases.CASES)))
def test_exact_on_lattice_data(case):
    B, N, d, k, n_tags, E, n_ex, with_bias = cases.CASES[case]
    user, items, s, bias, item_tag, cap, parts, after, ex = cases.lattice(*cases.CASES[case])
    for subset in cases.SUBSETS:
        p, a = cases.select(parts, after, subset)
        _same(_topk(user, items, k, item_tag, n_tags, cap, ex, bias, p, a), ref.topk(s, bias, item_tag, n_tags, cap, p, ex, k, a),
              "capped request %s" % (subset,))


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("with_ex", [False, True])
def test_every_subset_with_and_without_bias_and_excludes(with_bias, with_ex):
    """One mid-sized shape (two slices, two user tiles, P = 256 with the tag thresholds), every subset, the four combinations of
    prior and exclude list."""
    shape = (33, 2049, 40, 65, 19, 16, 5, True)
    B, N, d, k, n_tags = shape[:5]
    user, items, s, bias, item_tag, cap, parts, after, ex = cases.lattice(*shape)
    bias, ex = (bias if with_bias else None), (ex if with_ex else None)
    for subset in cases.SUBSETS:
        p, a = cases.select(parts, after, subset)
        _same(_topk(user, items, k, item_tag, n_tags, cap, ex, bias, p, a), ref.topk(s, bias, item_tag, n_tags, cap, p, ex, k, a),
              "capped request %s" % (subset,))


# ---- the consequences, on Gaussian data --------------------------------------------------------------------------------------
SHAPE = (65, 2049, 60, 10, 19, 16, 5, True)
KINDS = ["gauss", "lattice"]


def _host(kind, shape):
    """The lattice case `shape` on the host, or (kind "gauss") the same parts, tags and caps over Gaussian users, items and prior,
    for which there is no reference: s is None."""
    user, items, s, bias, item_tag, cap, parts, after, ex = cases.lattice(*shape)
    if kind == "gauss":
        rng = np.random.default_rng(13)
        user = rng.normal(size=user.shape).astype(np.float32)
        items = rng.normal(size=items.shape).astype(np.float32)
        nb = rng.normal(size=items.shape[0]).astype(np.float32)
        nb[np.isnan(bias)] = np.nan
        s, bias = None, nb
    return user, items, s, bias, item_tag, cap, parts, after, ex


def _gauss(shape=SHAPE):
    """The parts, tags and caps of the lattice case `shape` over Gaussian users, items and prior, on the device."""
    user, items, s, bias, item_tag, cap, parts, after, ex = cases.lattice(*shape)
    rng = np.random.default_rng(11)
    user = rng.normal(size=user.shape).astype(np.float32)
    items = rng.normal(size=items.shape).astype(np.float32)
    nb = rng.normal(size=items.shape[0]).astype(np.float32)
    nb[np.isnan(bias)] = np.nan
    dev = dict(u=_t(user, torch.float32), it=_t(items, torch.float32), bias=_t(nb, torch.float32), ex=_t(ex, torch.int64),
               tag=_t(item_tag, torch.int32), cap=_t(cap, torch.int32))
    return dev, item_tag, cap, parts, ex, shape[4]


@pytest.mark.parametrize("k", [10, 100, 256])
def test_uncapped_is_the_request_call(k):
    """1. Every cap >= k: nrms_topk_dot_request with the same parts, bit for bit, its tag set being allow (all tags without)."""
    dev, item_tag, cap, parts, ex, n_tags = _gauss()
    eng = _engine()
    B = cap.shape[0]
    big = torch.full((B, n_tags), k, dtype=torch.int32, device=DEV)
    big[1::2] = 2 ** 31 - 1
    every = torch.ones(B, n_tags, dtype=torch.bool, device=DEV)
    first = eng.top_k_request(dev["u"], dev["it"], 7, dev["ex"], bias=dev["bias"], **_kw(cases.select(parts, None, ("window", "adjust"))[0]))
    cursor = (first[0][:, -1].cpu().numpy().copy(), first[1][:, -1].cpu().numpy().copy())
    for subset in cases.SUBSETS[1:]:
        p, a = cases.select(parts, cursor, subset)
        kw = _kw(p, a)
        got = eng.top_k_request_capped(dev["u"], dev["it"], k, dev["tag"], n_tags, big, dev["ex"], bias=dev["bias"], **kw)
        tags = dict(item_tag=dev["tag"], n_tags=n_tags, allow=kw.pop("allow", every))
        _same(got, eng.top_k_request(dev["u"], dev["it"], k, dev["ex"], bias=dev["bias"], **tags, **kw), "uncapped %s" % (subset,))


def test_no_other_part_is_the_capped_call():
    """2. No window, no adjustments, no cursor, no allow: nrms_topk_dot_capped, bit for bit."""
    dev, item_tag, cap, parts, ex, n_tags = _gauss()
    eng = _engine()
    for k in (10, 65, 256):
        for b_ in (None, dev["bias"]):
            _same(eng.top_k_request_capped(dev["u"], dev["it"], k, dev["tag"], n_tags, dev["cap"], dev["ex"], bias=b_),
                  eng.top_k_capped(dev["u"], dev["it"], k, dev["tag"], n_tags, dev["cap"], dev["ex"], bias=b_), "the caps alone, k = %d" % k)


def test_prefix_and_tag_bound():
    """3 and 6. The first k' columns of k are the call with k' (across the three P classes); no row holds more than max(cap, 0) ids
    of a tag, and none of a closed tag."""
    dev, item_tag, cap, parts, ex, n_tags = _gauss()
    eng = _engine()
    first = eng.top_k_request(dev["u"], dev["it"], 7, dev["ex"], bias=dev["bias"], **_kw(cases.select(parts, None, ("window", "adjust"))[0]))
    cursor = (first[0][:, -1].cpu().numpy().copy(), first[1][:, -1].cpu().numpy().copy())
    for subset in (("window", "allow", "adjust", "cursor"), ("window", "allow"), ("adjust", "cursor")):
        p, a = cases.select(parts, cursor, subset)
        kw = _kw(p, a)
        call = lambda kk: eng.top_k_request_capped(dev["u"], dev["it"], kk, dev["tag"], n_tags, dev["cap"], dev["ex"], bias=dev["bias"], **kw)
        sc, ids = call(256)
        for kk in (1, 10, 64, 65, 192, 193):
            s2, i2 = call(kk)          # (the same caps: the walk does not know k until it stops)
            _same((i2, s2), (ids[:, :kk], sc[:, :kk]), "prefix %d of 256 %s" % (kk, subset))
        idn = ids.cpu().numpy()
        for b in range(idn.shape[0]):
            served = idn[b][idn[b] >= 0]
            tags = item_tag[served]
            assert ((tags >= 0) & (tags < n_tags)).all()
            assert (np.bincount(tags, minlength=n_tags) <= np.maximum(cap[b], 0)).all(), (subset, b)
            if p.allow is not None:
                assert p.allow[b][tags].all(), (subset, b)


def test_row_equals_the_capped_call_with_the_parts_as_bias():
    """4. Without a prior and a cursor, row b is nrms_topk_dot_capped at B = 1 with the deltas scattered and NaN where a part closes
    the item; and (N <= 4096) the greedy walk over nrms_topk_dot_deep with that bias."""
    dev, item_tag, cap, parts, ex, n_tags = _gauss()
    eng = _engine()
    N, k = dev["it"].shape[0], 65
    p, _ = cases.select(parts, None, ("window", "allow", "adjust"))
    sc, ids = eng.top_k_request_capped(dev["u"], dev["it"], k, dev["tag"], n_tags, dev["cap"], dev["ex"], **_kw(p))
    for b in (0, 1, 2, 5, 6, 31, 32, 63, 64):
        as_bias = _t(ref.as_bias(p, b, N), torch.float32)
        u1, e1 = dev["u"][b:b + 1].contiguous(), dev["ex"][b:b + 1].contiguous()
        one = eng.top_k_capped(u1, dev["it"], k, dev["tag"], n_tags, dev["cap"][b:b + 1].contiguous(), e1, bias=as_bias)
        _same(one, (sc[b:b + 1], ids[b:b + 1]), "row %d" % b)
        deep_s, deep_i = eng.top_k_deep(u1, dev["it"], N, e1, bias=as_bias)
        walk = topk_caps_ref.greedy_over_list(deep_i[0].cpu().numpy(), deep_s[0].cpu().numpy(), item_tag, n_tags, cap[b], k)
        _same(walk, (ids[b], sc[b]), "row %d over the deep list" % b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("subset", [("window", "allow", "adjust"), ("adjust",), ("window",), ()])
def test_pages_of_seven_chain_to_the_long_list(subset, kind):
    """5. Pages of 7 chained through the cursor and remaining_caps are the k = 256 list's columns and then -1, on Gaussian data and,
    where nothing may be repeated or skipped across ties, on lattice data; rows that cannot fill and rows with a dominant tag
    included."""
    shape = (33, 513, 40, 64, 19, 16, 5, True)
    user, items, s, bias, item_tag, cap, parts, after, ex = _host(kind, shape)
    B, n_tags = shape[0], shape[4]
    eng = _engine()
    u, it, bi, exd = _t(user, torch.float32), _t(items, torch.float32), _t(bias, torch.float32), _t(ex, torch.int64)
    tag = _t(item_tag, torch.int32)
    cap = np.array(cap)
    cap[2] = 40
    cap[2, 0] = 3                                    # the dominant tag tightly capped beside uncapped ones
    cap[3] = 2
    cap[3, 0] = 200                                  # ... and the other way round
    capd = _t(cap, torch.int32)
    p, _ = cases.select(parts, None, subset)
    kw = _kw(p)
    full_s, full_i = eng.top_k_request_capped(u, it, 256, tag, n_tags, capd, exd, bias=bi, **kw)
    lengths = (full_i >= 0).sum(dim=1)
    assert int(lengths.min()) <= 2 and int(lengths.max()) == 256 and int((lengths < 256).sum()) > B // 2          # short and full rows
    a_s = torch.zeros(B, device=DEV)
    a_i = torch.full((B,), ref.PAGE_BEGIN, dtype=torch.int64, device=DEV)
    left, got_s, got_i = capd, [], []
    for _ in range(256 // 7 + 1):
        s_, i_ = eng.top_k_request_capped(u, it, 7, tag, n_tags, left, exd, bias=bi, after_scores=a_s, after_ids=a_i, **kw)
        got_s.append(s_)
        got_i.append(i_)
        a_s, a_i = s_[:, -1].contiguous(), i_[:, -1].contiguous()
        left = remaining_caps(left, i_, tag, n_tags)
    got_s, got_i = torch.cat(got_s, dim=1), torch.cat(got_i, dim=1)
    _same((got_i[:, :256], got_s[:, :256]), (full_i, full_s), "chained pages %s" % (subset,))
    assert (got_i[lengths < 256][:, 256:] == -1).all()          # a list that ended stays ended (an uncapped user's goes on)
    if s is not None:
        _same((full_i, full_s), ref.topk(s, bias, item_tag, n_tags, cap, p, ex, 256), "the long list %s" % (subset,))


@pytest.mark.parametrize("kind", KINDS)
def test_row_depends_on_its_own_rows_only_and_the_batch_splits(kind):
    """7. Rows of a B = 33 call equal the calls at B = 1 + 32 (the split of the batch, byte for byte) and, for a few rows, at B = 1
    from another position; two runs give the same bytes.  On Gaussian and on lattice data."""
    shape = (33, 2049, 40, 65, 19, 16, 5, True)
    user, items, s, bias, item_tag, cap, parts, after, ex = _host(kind, shape)
    n_tags, k = shape[4], shape[3]
    rows = lambda x, sl: x if x is None or np.ndim(x) == 0 or np.shape(x)[0] != shape[0] else x[sl]
    for subset in (("window", "allow", "adjust", "cursor"), ("allow", "adjust")):
        p, a = cases.select(parts, after, subset)
        ids, sc = _topk(user, items, k, item_tag, n_tags, cap, ex, bias, p, a)
        _same(_topk(user, items, k, item_tag, n_tags, cap, ex, bias, p, a), (ids, sc), "the second run")
        got_i, got_s = [], []
        for sl in (slice(0, 1), slice(1, 33)):
            pb = ref.Parts(*[rows(x, sl) for x in p])
            ab = None if a is None else (a[0][sl], a[1][sl])
            i_, s_ = _topk(user[sl], items, k, item_tag, n_tags, cap[sl], ex[sl], bias, pb, ab)
            got_i.append(i_)
            got_s.append(s_)
        _same((np.concatenate(got_i), np.concatenate(got_s)), (ids, sc), "33 = 1 + 32 %s" % (subset,))
        for b in (5, 6, 17, 32):
            sl = slice(b, b + 1)
            pb = ref.Parts(*[rows(x, sl) for x in p])
            ab = None if a is None else (a[0][sl], a[1][sl])
            _same(_topk(user[sl], items, k, item_tag, n_tags, cap[sl], ex[sl], bias, pb, ab), (ids[sl], sc[sl]), "row %d alone" % b)


# ---- argument errors: refused on the host, before any launch -----------------------------------------------------------------
def test_argument_errors():
    lib = _lib.load()
    B, N, d, k, E, n_tags = 4, 100, 8, 5, 4, 19
    g = torch.Generator(device="cpu").manual_seed(1)
    user, items = torch.randn(B, d, generator=g).to(DEV), torch.randn(N, d, generator=g).to(DEV)
    it_time, win = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(B, 2, dtype=torch.int32, device=DEV)
    it_tag, allow = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(B, 1, dtype=torch.int32, device=DEV)
    cap = torch.ones(B, n_tags, dtype=torch.int32, device=DEV)
    aid, adl = torch.zeros(B, E, dtype=torch.int64, device=DEV), torch.zeros(B, E, device=DEV)
    a_s, a_i = torch.zeros(B, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.int64, device=DEV)
    sc, ids = torch.full((B, k), 5.0, device=DEV), torch.full((B, k), 5, dtype=torch.int64, device=DEV)
    P = _lib.ptr
    base = dict(time=P(it_time), win=P(win), tag=P(it_tag), n_tags=n_tags, allow=P(allow), cap=P(cap), aid=P(aid), adl=P(adl), E=E,
                a_s=P(a_s), a_i=P(a_i))

    def call(nbytes=None, **over):
        a = dict(base, **over)
        need = int(lib.nrms_topk_dot_request_capped_workspace_bytes(B, C.c_int64(N), d, k))
        return lib.nrms_topk_dot_request_capped(B, C.c_int64(N), d, k, P(user), P(items), None, a["time"], a["win"], a["tag"], a["n_tags"],
                                                a["allow"], a["cap"], a["aid"], a["adl"], a["E"], a["a_s"], a["a_i"], None, 0, P(sc),
                                                P(ids), P(ws), C.c_size_t(need if nbytes is None else need + nbytes), _stream())

    for kw, word in [(dict(cap=None), b"cap is null"), (dict(tag=None), b"item_tag is null"), (dict(time=None), b"item_time is null"),
                     (dict(win=None), b"window is null"), (dict(aid=None), b"adj_ids is null"), (dict(adl=None), b"adj_delta is null"),
                     (dict(a_s=None), b"after_scores is null"), (dict(a_i=None), b"after_ids is null"), (dict(n_tags=0), b"n_tags must be"),
                     (dict(n_tags=513), b"n_tags must be"), (dict(E=257), b"n_adjust must be"),
                     (dict(cap=C.c_void_p(P(cap).value + 2)), b"cap must be 4-byte aligned")]:
        assert call(**kw) == _lib.NRMS_EINVAL, kw
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_request_capped: ") and word in msg, msg
    assert call(nbytes=-1) == _lib.NRMS_EWORKSPACE                   # one byte short
    assert lib.nrms_last_error().startswith(b"topk_dot_request_capped: ")
    torch.cuda.synchronize()
    assert (sc == 5.0).all() and (ids == 5).all()                    # nothing was launched
    assert call() == _lib.NRMS_OK
    assert call(E=0) == _lib.NRMS_OK and call(aid=None, adl=None) == _lib.NRMS_OK and call(allow=None) == _lib.NRMS_OK
    torch.cuda.synchronize()
    eng = _engine()
    for kw, word in ((dict(adj_ids=aid), "adj_ids and adj_delta go together"), (dict(after_ids=a_i), "after_scores and after_ids go together"),
                     (dict(window=win), "item_time and window go together")):
        with pytest.raises(_lib.NrmsError, match=word):
            eng.top_k_request_capped(user, items, k, it_tag, n_tags, cap, **kw)
    with pytest.raises(_lib.NrmsError, match="cap must be an int32"):
        eng.top_k_request_capped(user, items, k, it_tag, n_tags, cap[:, :5])


# ---- the buffer contract -----------------------------------------------------------------------------------------------------
def test_buffer_contract():
    """Outputs and the workspace at the queried size between guard bands, the workspace poisoned three ways; every part's arrays,
    the tags and the caps are guarded too, at exactly their sizes, and come back unchanged."""
    from tests.guarded import POISONS, Pool
    from tests.test_hip_buffer_contracts import dev, ok, refuses_undersized, three_poisons
    lib = _lib.load()
    shape = cases.CASES[4]
    B, N, d, k, n_tags, E, n_ex, with_bias = shape
    user, items, s, bias, item_tag, cap, parts, after, ex = cases.lattice(*shape)
    ud, itd, exd = dev(np.array(user)), dev(np.array(items)), dev(ex, torch.int64)
    need = int(lib.nrms_topk_dot_request_capped_workspace_bytes(B, C.c_int64(N), d, k))
    assert need > 0
    packed = pack_tag_mask(torch.from_numpy(np.array(parts.allow))).reshape(-1)
    ins = {"item_time": (parts.item_time, torch.int32), "window": (parts.window, torch.int32), "item_tag": (item_tag, torch.int32),
           "cap": (cap, torch.int32), "adj_ids": (parts.adj_ids, torch.int64), "adj_delta": (parts.adj_delta, torch.float32),
           "after_scores": (after[0], torch.float32), "after_ids": (after[1], torch.int64)}

    def run(poison):
        P = Pool(poison)
        for name, (a, dt) in ins.items():
            P.elems(name, a.size, dt, init=torch.from_numpy(np.array(a)).reshape(-1))
        P.elems("allow", packed.numel(), torch.int32, init=packed)
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, torch.int64), P.new("ws", need)

        def call(nbytes):
            return lib.nrms_topk_dot_request_capped(B, C.c_int64(N), d, k, _lib.ptr(ud), _lib.ptr(itd), None, P["item_time"].ptr,
                                                    P["window"].ptr, P["item_tag"].ptr, n_tags, P["allow"].ptr, P["cap"].ptr,
                                                    P["adj_ids"].ptr, P["adj_delta"].ptr, E, P["after_scores"].ptr, P["after_ids"].ptr,
                                                    _lib.ptr(exd), n_ex, P["top_scores"].ptr, P["top_ids"].ptr, P["ws"].ptr,
                                                    C.c_size_t(nbytes), _stream())

        names = list(ins) + ["allow"]
        snap = [P[n].snapshot() for n in names]
        ok(call(need), "nrms_topk_dot_request_capped")
        P.intact("nrms_topk_dot_request_capped")
        assert all(P[n].unchanged_since(sn) for n, sn in zip(names, snap))
        if poison == POISONS[0]:
            keep = {n: P[n].numpy() for n in ("top_scores", "top_ids")}
            refuses_undersized(call, P, need, "nrms_topk_dot_request_capped")
            assert all(np.array_equal(_bits(keep[n]), _bits(P[n].numpy())) for n in keep)
        return {"ids": P["top_ids"].numpy((B, k)), "scores": P["top_scores"].numpy((B, k))}

    out = three_poisons(run, "the capped request")[POISONS[0]]
    _same((out["ids"], out["scores"]), ref.topk(s, None, item_tag, n_tags, cap, parts, ex, k, after), "capped request between guard bands")


# ---- the models --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_models_recommend_request_capped(kind):
    """Model.recommend_request_capped equals the reference on the model's own score bits (recommend_deep's full ranking gives them:
    news id n is row n - 1 of the catalogue without its padding row), and the second page follows the first."""
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model(kind)
    N = cat.shape[0]
    rng = np.random.default_rng(7)
    n_tags, E, k = 7, 12, 20
    item_time = rng.integers(0, 30, size=N).astype(np.int32)
    item_tag = rng.integers(-1, n_tags, size=N).astype(np.int64)
    batch = batches[0]
    B = torch.as_tensor(batch["browsed_ids"]).shape[0]
    lo = rng.integers(0, 11, size=B)
    window = np.stack([lo, lo + 20], axis=1).astype(np.int32)
    allow = rng.random((B, n_tags)) < 0.7
    news = rng.integers(1, N, size=(B, E)).astype(np.int64)
    news[:, 0], news[:, 1] = 0, N + 5
    delta = (rng.integers(-20, 21, size=(B, E)) * 0.25).astype(np.float32)
    delta[:, 4] = np.nan
    cap = rng.integers(0, 4, size=(B, n_tags)).astype(np.int32)
    cap[0] = k
    td = lambda a: torch.from_numpy(a).to(DEV)
    kw = dict(item_time=td(item_time), window=td(window), allow=td(allow), adjust=(td(news), td(delta)))
    ids, sc = model.recommend_request_capped(batch, k, cat, td(item_tag), td(cap), **kw)
    # the plain score bits of every catalogue row, from the model's own user vectors
    user, c, exclude = model._catalogue_query(batch, cat, True, "test")
    deep_s, deep_i = model._engine.top_k_deep(user, c[1:], N - 1, None)
    s = np.full((B, N - 1), np.nan, dtype=np.float32)
    di, ds = deep_i.cpu().numpy(), deep_s.cpu().numpy()
    for b in range(B):
        s[b, di[b][di[b] >= 0]] = ds[b][di[b] >= 0]
    assert not np.isnan(s).any()
    p = ref.Parts(item_time[1:], window, item_tag[1:], n_tags, allow, news - 1, delta)
    want_i, want_s = ref.topk(s, None, item_tag[1:], n_tags, cap, p, exclude.cpu().numpy(), k)
    _same((ids, sc), (np.where(want_i >= 0, want_i + 1, want_i), want_s), kind)
    assert int((ids > 0).sum()) > 0 and int((ids < 0).sum()) > 0
    # the second page follows the first, through remaining_caps in news ids
    left = remaining_caps(td(cap), ids[:, :8], td(item_tag), n_tags)
    ids2, sc2 = model.recommend_request_capped(batch, k - 8, cat, td(item_tag), left, after=(ids[:, 7], sc[:, 7]), **kw)
    _same((torch.cat([ids[:, :8], ids2], dim=1), torch.cat([sc[:, :8], sc2], dim=1)), (ids, sc), "two pages")
    # no other part: recommend_capped; every cap >= k: recommend_request, bit for bit
    _same(model.recommend_request_capped(batch, k, cat, td(item_tag), td(cap)), model.recommend_capped(batch, k, cat, td(item_tag), td(cap)),
          "the caps alone")
    _same(model.recommend_request_capped(batch, k, cat, td(item_tag), k, n_tags=n_tags, **kw),
          model.recommend_request(batch, k, cat, item_tag=td(item_tag), **kw), "uncapped")
    with pytest.raises(_lib.NrmsError, match="allow must be"):
        model.recommend_request_capped(batch, k, cat, td(item_tag), td(cap), allow=td(allow)[:, :3])
    model.check_recommend_ids()


def test_hierec_and_graph_refuse():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    for mod, name in ((hierec_hip, "hierec"), (graph_hip, "graph")):
        with pytest.raises(NotImplementedError, match=name + ": recommend_request_capped is not available"):
            mod.Model.recommend_request_capped(None, {}, 5, None, None, 2)


def test_run_v0_request_max_per_category_flag(tmp_path):
    """A fresh child process with a time limit of its own; nothing is started after it."""
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    out = tmp_path / "rec.txt"
    r = subprocess.run([sys.executable, "-m", "pytorch_news_recommender_amd.run_v0", "--model", "nrms_hip", "--dataset", "synthetic",
                        "--negatives", "catalogue", "--max_batches", "2", "--epochs", "1", "--synthetic_users", "128",
                        "--batch_size", "64", "--num_workers", "0", "--description", "T", "--data_path", str(tmp_path / "data"),
                        "--save_path", str(tmp_path / "save"), "--recommend", "10", "--combine_filters", "--request_max_per_category", "2",
                        "--mute_categories", "1", "--seen_discount", "0.5", "--recommend_out", str(out)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    pat = (r"request with at most 2 per category: categories per list: ([\d.]+)  largest category share: ([\d.]+)  users: (\d+)"
           r"  hit@1: [\d.]+ \+- [\d.]+  hit@5: [\d.]+ \+- [\d.]+  hit@10: ([\d.]+) \+- ([\d.]+)")
    line = [re.fullmatch(pat, ln) for ln in r.stdout.splitlines() if ln.startswith("request with at most 2")]
    assert len(line) == 1 and line[0], r.stdout[-3000:]
    assert int(line[0].group(3)) > 0
    # ten news with at most two of a category: at least five categories, and no category above a fifth of a full list
    assert float(line[0].group(1)) >= 5.0 and float(line[0].group(2)) <= 0.2 + 1e-9
    lists = [[int(v) for v in ln.split(" ", 1)[1].strip()[1:-1].split(",") if v] for ln in open(out)]
    assert len(lists) == int(line[0].group(3)) and all(len(set(row)) == len(row) <= 10 for row in lists)
