"""nrms_topk_dot_capped on the GPU (per-category caps on the served list, include/nrms_hip.h): exact against tests/topk_caps_ref.py
on integer lattice data at every point where the kernels change path, the consequences (1) to (6) the header states, the flood
case, rows with sum(cap) < k beside ordinary rows, determinism, the buffer contract, and the layers above (engine.top_k_capped,
Model.recommend_capped, run_v0 --max_per_category).  Every comparison is exact: ids and score bits; there is no tolerance.  Parity
is unpinned: the reference has no catalogue retrieval."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream

from tests import topk_caps_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MAX = 2 ** 31 - 1
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


def _capped(user, items, k, ex, bias, tag, n_tags, cap):
    s, ids = _engine().top_k_capped(_t(user, torch.float32), _t(items, torch.float32), k, _t(tag, torch.int32), n_tags,
                                    _t(cap, torch.int32), _t(ex, torch.int64), bias=_t(bias, torch.float32))
    return ids.cpu().numpy(), s.cpu().numpy()


# ---- the data ----------------------------------------------------------------------------------------------------------------
def _tags(N, n_tags, rng):
    """One tag per item: half the catalogue carries tag 0 (a dominant tag), the rest any tag, a few -1, n_tags and INT32_MAX."""
    t = rng.integers(0, n_tags, size=N).astype(np.int64)
    t[rng.random(N) < 0.5] = 0
    if N >= 63:
        bad = rng.choice(N, size=6, replace=False)
        t[bad[:2]], t[bad[2:4]], t[bad[4:]] = -1, n_tags, I32_MAX
        t[1] = n_tags - 1
        t[2] = min(31, n_tags - 1)
        t[3] = min(32, n_tags - 1)
    return t


def _caps(B, n_tags, k, rng):
    """Row b takes cap kind b % 8: per-user caps that differ inside a block, rows with sum(cap) < k beside ordinary ones."""
    c = np.zeros((B, n_tags), dtype=np.int64)
    for b in range(B):
        kind = b % 8
        if kind == 0:
            c[b] = 1                                             # one of every tag
        elif kind == 1:
            c[b] = rng.integers(-2, 1, size=n_tags)              # everything closed: an all-padding row
        elif kind == 2:
            c[b] = rng.integers(-1, 4, size=n_tags)              # closed tags among small caps
        elif kind == 3:
            c[b] = rng.integers(k, k + 3, size=n_tags)           # uncapped
            c[b, 0] = I32_MAX
        elif kind == 4:
            c[b, 0], c[b, n_tags - 1] = 1, 2                     # sum(cap) <= 3: short rows
        elif kind == 5:
            c[b] = rng.integers(1, k + 2, size=n_tags)
        elif kind == 6:
            c[b] = np.where(rng.random(n_tags) < 0.5, 0, k)      # {0} u [k, inf)
        else:
            c[b] = 2
            c[b, 0] = max(1, k // 2)                             # the dominant tag gets half the list
    return c


@functools.lru_cache(maxsize=None)
def _lattice(B, N, d, k, n_ex, n_tags, with_bias):
    """Integer users and items in [-3, 3] (every dot product, and every sum with a multiple of 0.25 below 2^12, is exact in fp32
    whatever the order of summation; ties are abundant, so the id rule is exercised), a bias of multiples of 0.25 with NaN and
    -inf entries, exclude lists with -1, N and a duplicate."""
    rng = np.random.default_rng(100003 * d + 1009 * N + 17 * k + B + n_ex + 31 * n_tags)
    user = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)         # exact
    bias = None
    if with_bias:
        amp = int(4 * max(2.0, 4.0 * np.sqrt(d)))
        bias = (rng.integers(-amp, amp + 1, size=N) * 0.25).astype(np.float32)
        if N >= 63:
            bias[rng.integers(0, N, size=4)] = np.nan
            bias[int(rng.integers(0, N))] = -np.inf
    tag = _tags(N, n_tags, rng)
    cap = _caps(B, n_tags, k, rng)
    ex = None
    if n_ex:
        ex = rng.integers(0, max(N, 1), size=(B, n_ex)).astype(np.int64)
        ex[:, 0], ex[:, 1], ex[:, 2] = -1, N, ex[:, min(3, n_ex - 1)]
    for a in (user, items, s, tag, cap):
        a.setflags(write=False)
    return user, items, s, bias, tag, cap, ex


# (B, N, d, k, n_exclude, n_tags, bias): B {1, 32, 33}, N {0, 1, 63, 2049, 4100}, d {7, 40}, k {1, 10, 64, 65, 192, 193, 256},
# n_exclude {0, 3, 70}, n_tags {1, 19, 33, 512}
LATTICE = [
    (33, 0, 7, 10, 0, 19, False),            # an empty catalogue: all-padding rows
    (1, 1, 7, 1, 0, 1, True),                # one item, one user, one tag
    (32, 63, 7, 10, 3, 19, True),            # less than one wave step, the scalar loads
    (33, 2049, 40, 64, 70, 33, True),        # two slices, P = 128 at its largest k, two bitmap words, global excludes
    (33, 2049, 7, 65, 3, 19, False),         # P = 256 at its smallest k
    (32, 4100, 40, 192, 0, 512, True),       # three slices, P = 256 at its largest k (eight waves), the largest tag count
    (33, 4100, 40, 193, 3, 33, False),       # P = 512, the two-wave block
    (1, 4100, 7, 256, 70, 19, True),         # one user, the largest k
    (33, 4100, 7, 1, 3, 1, False),           # k = 1 with one tag
]


@pytest.mark.parametrize("B,N,d,k,n_ex,n_tags,with_bias", LATTICE)
def test_exact_on_lattice_data(B, N, d, k, n_ex, n_tags, with_bias):
    user, items, s, bias, tag, cap, ex = _lattice(B, N, d, k, n_ex, n_tags, with_bias)
    want = ref.topk(s, bias, tag, n_tags, cap, ex, k)
    if N >= 2049 and B >= 32 and n_tags > 1 and k >= 10:          # on the CPU-side data: the test cannot pass by ignoring the caps
        every = ref.topk(s, bias, tag, n_tags, np.full_like(cap, k), ex, k)
        assert (want[0][1] == -1).all() and (every[0][1] >= 0).all()                                   # the closed row
        assert sum(not np.array_equal(want[0][b], every[0][b]) for b in range(B)) >= B // 2
        assert (want[0][4] >= 0).sum() <= 3 < k                                                        # a sum(cap) < k row
    got = _capped(user, items, k, ex, bias, tag, n_tags, cap)
    _same(got, want, "capped top-k")
    # (4): no row holds more than cap[b, t] ids of tag t, and nothing out of range
    for b in range(B):
        t = tag[got[0][b][got[0][b] >= 0]]
        assert ((t >= 0) & (t < n_tags)).all()
        assert (np.bincount(t, minlength=n_tags) <= np.maximum(cap[b], 0)).all()


def test_flood_of_one_capped_tag():
    """The 3 000 best items all carry tag 0, whose cap is 1, and scores ascend with the row: every one of them beats the
    threshold, buffers overflow and candidates stay pending across several flushes; even rows have sum(cap) < k."""
    B, N, d, k, n_tags = 32, 5000, 7, 10, 5
    rng = np.random.default_rng(11)
    user = np.zeros((B, d), dtype=np.float32)
    user[:, 0] = 1 + np.arange(B) % 3
    items = rng.integers(-1, 2, size=(N, d)).astype(np.float32)
    items[:, 0] = np.concatenate([rng.integers(0, 30, size=2000), 100 + np.arange(3000)])          # ascending by row
    user[:, 1:] = 0
    s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)
    tag = np.concatenate([rng.integers(1, n_tags, size=2000), np.zeros(3000, dtype=np.int64)])
    cap = np.full((B, n_tags), 2, dtype=np.int64)
    cap[1::2, 1:] = 5
    cap[:, 0] = 1
    want = ref.topk(s, None, tag, n_tags, cap, None, k)
    assert (want[0][:, 0] == N - 1).all() and (want[0][0::2, 9] == -1).all() and (want[0][1::2, 9] >= 0).all()
    _same(_capped(user, items, k, None, None, tag, n_tags, cap), want, "flood")
    cap2 = cap.copy()
    cap2[:, 0] = 3
    _same(_capped(user, items, 193, None, None, tag, n_tags, cap2), ref.topk(s, None, tag, n_tags, cap2, None, 193), "flood, P = 512")


# ---- Gaussian data: bit for bit against the other calls ----------------------------------------------------------------------
B_REAL, N_REAL, D_REAL, TAGS_REAL = 33, 4000, 40, 19


@functools.lru_cache(maxsize=None)
def _real():
    g = torch.Generator().manual_seed(7)
    user = torch.randn(B_REAL, D_REAL, generator=g).to(DEV)
    items = torch.randn(N_REAL, D_REAL, generator=g).to(DEV)
    bias = (0.5 * torch.randn(N_REAL, generator=g)).to(DEV)
    ex = torch.randint(0, N_REAL, (B_REAL, 3), generator=g).to(DEV)
    rng = np.random.default_rng(7)
    tag = rng.integers(0, TAGS_REAL, size=N_REAL)
    tag[rng.random(N_REAL) < 0.4] = 3                                               # a dominant tag
    return user, items, bias, ex, torch.from_numpy(tag).to(torch.int32).to(DEV), rng


def test_uncapped_and_closed_caps_are_the_tagged_and_the_plain_call():
    """(1) every cap >= k: the tagged call with all tags open, and with every tag in range the plain / biased call; (2) every cap
    in {0} u [k, inf): the tagged call with allow = cap > 0."""
    user, items, bias, ex, tag, rng = _real()
    eng = _engine()
    for k in (10, 65, 193):
        for b_ in (None, bias):
            cap = torch.from_numpy(rng.integers(k, k + 4, size=(B_REAL, TAGS_REAL))).to(torch.int32).to(DEV)
            cap[:, 0] = I32_MAX
            got = eng.top_k_capped(user, items, k, tag, TAGS_REAL, cap, ex, bias=b_)
            allow = torch.ones(B_REAL, TAGS_REAL, dtype=torch.bool, device=DEV)
            _same(got, eng.top_k_tagged(user, items, k, tag, TAGS_REAL, allow, ex, bias=b_), "(1) tagged, k=%d" % k)
            _same(got, eng.top_k(user, items, k, ex, bias=b_), "(1) plain / biased, k=%d" % k)
            allow = torch.from_numpy(rng.random((B_REAL, TAGS_REAL)) < 0.5).to(DEV)
            allow[0], allow[1] = True, False
            closed = torch.from_numpy(rng.integers(-3, 1, size=(B_REAL, TAGS_REAL))).to(torch.int32).to(DEV)
            got = eng.top_k_capped(user, items, k, tag, TAGS_REAL, torch.where(allow, cap, closed), ex, bias=b_)
            _same(got, eng.top_k_tagged(user, items, k, tag, TAGS_REAL, allow, ex, bias=b_), "(2) k=%d" % k)
            assert (got[1][1] == -1).all()
    # a tag outside [0, n_tags) is served to nobody whatever the caps: the tagged call's rule
    tag2 = tag.clone()
    tag2[::5], tag2[1::7] = -1, TAGS_REAL
    cap = torch.full((B_REAL, TAGS_REAL), 10, dtype=torch.int32, device=DEV)
    _same(eng.top_k_capped(user, items, 10, tag2, TAGS_REAL, cap, ex),
          eng.top_k_tagged(user, items, 10, tag2, TAGS_REAL, torch.ones(B_REAL, TAGS_REAL, dtype=torch.bool, device=DEV), ex), "out-of-range tags")


def _real_caps(rng):
    cap = rng.integers(0, 4, size=(B_REAL, TAGS_REAL))
    cap[:, 3] = rng.integers(1, 30, size=B_REAL)                                    # the dominant tag
    cap[4] = 0
    cap[4, 3], cap[4, 5] = 2, 1                                                     # sum(cap) = 3
    return cap


def test_prefix_property():
    """(3) the first k' columns of a call with k are the call with k'."""
    user, items, bias, ex, tag, rng = _real()
    eng = _engine()
    cap = torch.from_numpy(_real_caps(rng)).to(torch.int32).to(DEV)
    sc, ids = eng.top_k_capped(user, items, 256, tag, TAGS_REAL, cap, ex, bias=bias)
    assert (ids[4, 3:] == -1).all() and (ids[4, :3] >= 0).all() and (ids[:, 0] >= 0).sum() >= B_REAL - 2
    for k in (1, 10, 64, 65, 192, 193):
        _same(eng.top_k_capped(user, items, k, tag, TAGS_REAL, cap, ex, bias=bias), (sc[:, :k], ids[:, :k]), "(3) k'=%d" % k)


def _raw(user, items, bias, tag, n_tags, cap, ex, k, ws_fill):
    lib = _lib.load()
    B, d = user.shape
    N = items.shape[0]
    need = int(lib.nrms_topk_dot_capped_workspace_bytes(B, C.c_int64(N), d, k))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    ws.view(torch.uint8).fill_(ws_fill)
    sc = torch.empty(B, k, dtype=torch.float32, device=DEV)
    ids = torch.empty(B, k, dtype=torch.int64, device=DEV)
    rc = lib.nrms_topk_dot_capped(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), _lib.ptr(bias), _lib.ptr(tag), n_tags,
                                  _lib.ptr(cap), _lib.ptr(ex), ex.shape[1], _lib.ptr(sc), _lib.ptr(ids), _lib.ptr(ws),
                                  C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_topk_dot_capped")
    return sc, ids


def test_row_depends_on_its_own_user_and_caps_only():
    """(5): two runs, the batch split 33 = 1 + 32, the user's position, the neighbours' caps, a poisoned workspace."""
    user, items, bias, ex, tag, rng = _real()
    eng = _engine()
    k, nt = 100, TAGS_REAL
    cap = torch.from_numpy(_real_caps(rng)).to(torch.int32).to(DEV)
    sc, ids = eng.top_k_capped(user, items, k, tag, nt, cap, ex, bias=bias)
    _same(eng.top_k_capped(user, items, k, tag, nt, cap, ex, bias=bias), (sc, ids), "second run")
    cut = lambda a, p: a[p].contiguous()
    parts = [slice(0, 1), slice(1, 33)]
    got = [eng.top_k_capped(cut(user, p), items, k, tag, nt, cut(cap, p), cut(ex, p), bias=bias) for p in parts]
    assert torch.cat([x[0] for x in got]).cpu().numpy().tobytes() == sc.cpu().numpy().tobytes()
    assert torch.cat([x[1] for x in got]).cpu().numpy().tobytes() == ids.cpu().numpy().tobytes()
    perm = torch.randperm(B_REAL, generator=torch.Generator().manual_seed(3)).to(DEV)
    up = lambda a: a[perm].contiguous()
    _same(eng.top_k_capped(up(user), items, k, tag, nt, up(cap), up(ex), bias=bias), (sc[perm], ids[perm]), "user permutation")
    u = 5
    for fill in (0, k):                                               # user 5 among 31 rows that are closed, then uncapped
        c2 = torch.full((32, nt), fill, dtype=torch.int32, device=DEV)
        c2[13] = cap[u]
        rows = torch.full((32,), 20, dtype=torch.int64, device=DEV)
        rows[13] = u
        s2, i2 = eng.top_k_capped(user[rows].contiguous(), items, k, tag, nt, c2, ex[rows].contiguous(), bias=bias)
        _same((s2[13:14], i2[13:14]), (sc[u:u + 1], ids[u:u + 1]), "neighbours' caps %d" % fill)
        assert fill or ((i2[:13] == -1).all() and (i2[14:] == -1).all())
    for fill in (0xFF, 0x00):
        _same(_raw(user, items, bias, tag, nt, cap, ex, k, fill), (sc, ids), "workspace 0x%02X" % fill)


def test_equals_greedy_walk_over_the_deep_list():
    """(6) N <= 4096: row b is the greedy walk over row b of nrms_topk_dot_deep (K = 4096), ids and score bits alike."""
    user, items, bias, ex, tag, rng = _real()
    eng = _engine()
    cap = _real_caps(rng)
    tag_h = tag.cpu().numpy()
    for b_ in (None, bias):
        dsc, dids = eng.top_k_deep(user, items, 4096, ex, bias=b_)
        dsc, dids = dsc.cpu().numpy(), dids.cpu().numpy()
        for k in (10, 193):
            sc, ids = eng.top_k_capped(user, items, k, tag, TAGS_REAL, _t(cap, torch.int32), ex, bias=b_)
            ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
            for b in range(B_REAL):
                wi, ws = ref.greedy_over_list(dids[b], dsc[b], tag_h, TAGS_REAL, cap[b], k)
                _same((ids[b], sc[b]), (wi, ws), "(6) row %d, k=%d" % (b, k))


def test_engine_arguments_and_empty_extents():
    user, items, bias, ex, tag, rng = _real()
    eng = _engine()
    cap = torch.full((B_REAL, TAGS_REAL), 2, dtype=torch.int32, device=DEV)
    a = eng.top_k_capped(user, items, 10, tag, TAGS_REAL, cap, ex)
    _same(eng.top_k_capped(user, items, 10, tag.long(), TAGS_REAL, cap, ex), a, "int64 tags")
    for bad in (dict(item_tag=tag[:-1].contiguous()), dict(item_tag=tag.float()), dict(item_tag=tag.cpu()), dict(cap=cap[:-1].contiguous()),
                dict(cap=cap.long()), dict(cap=cap[:, :-1].contiguous()), dict(cap=cap.cpu()), dict(cap=2), dict(n_tags=0), dict(n_tags=513)):
        kw = dict(item_tag=tag, n_tags=TAGS_REAL, cap=cap)
        kw.update(bad)
        with pytest.raises(_lib.NrmsError, match="top_k_capped: (item_tag|cap|n_tags)"):
            eng.top_k_capped(user, items, 10, kw["item_tag"], kw["n_tags"], kw["cap"], ex)
    with pytest.raises(_lib.NrmsError, match="k"):
        eng.top_k_capped(user, items, 257, tag, TAGS_REAL, cap, ex)
    sc, ids = eng.top_k_capped(user, torch.empty(0, D_REAL, device=DEV), 10, torch.empty(0, dtype=torch.int32, device=DEV), TAGS_REAL, cap, None)
    assert (ids == -1).all() and (sc == -float("inf")).all()                        # N = 0: all-padding rows
    lib = _lib.load()
    assert lib.nrms_topk_dot_capped(0, C.c_int64(N_REAL), D_REAL, 10, None, None, None, None, TAGS_REAL, None, None, 0, None, None,
                                    None, C.c_size_t(0), _stream()) == _lib.NRMS_OK      # B = 0: a no-op


# ---- the buffer contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [3, 6])
def test_buffer_contract(case):
    """Outputs and the workspace at the queried size between guard bands, the workspace poisoned three ways; bias, item_tag and cap
    are guarded too, at exactly their sizes."""
    from tests.guarded import POISONS, Pool
    from tests.test_hip_buffer_contracts import dev, ok, refuses_undersized, three_poisons
    lib = _lib.load()
    B, N, d, k, n_ex, n_tags, with_bias = LATTICE[case]
    user, items, s, bias, tag, cap, ex = _lattice(*LATTICE[case])
    ud, itd, exd = dev(np.array(user)), dev(np.array(items)), dev(ex, torch.int64)
    need = int(lib.nrms_topk_dot_capped_workspace_bytes(B, C.c_int64(N), d, k))
    assert need > 0

    def run(poison):
        P = Pool(poison)
        if with_bias:
            P.elems("bias", N, torch.float32, init=torch.from_numpy(np.array(bias)))
        P.elems("tag", N, torch.int32, init=torch.from_numpy(np.array(tag)).to(torch.int32))
        P.elems("cap", B * n_tags, torch.int32, init=torch.from_numpy(np.array(cap)).to(torch.int32).reshape(-1))
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, torch.int64), P.new("ws", need)
        read_only = ("bias", "tag", "cap") if with_bias else ("tag", "cap")

        def call(nbytes):
            return lib.nrms_topk_dot_capped(B, C.c_int64(N), d, k, _lib.ptr(ud), _lib.ptr(itd), P["bias"].ptr if with_bias else None,
                                            P["tag"].ptr, n_tags, P["cap"].ptr, _lib.ptr(exd), n_ex, P["top_scores"].ptr,
                                            P["top_ids"].ptr, P["ws"].ptr, C.c_size_t(nbytes), _stream())

        snap = [P[n].snapshot() for n in read_only]
        ok(call(need), "nrms_topk_dot_capped")
        P.intact("nrms_topk_dot_capped")
        assert all(P[n].unchanged_since(sn) for n, sn in zip(read_only, snap))
        if poison == POISONS[0]:
            keep = {n: P[n].numpy() for n in ("top_scores", "top_ids")}
            refuses_undersized(call, P, need, "nrms_topk_dot_capped")
            assert all(np.array_equal(_bits(keep[n]), _bits(P[n].numpy())) for n in keep)
        return {"ids": P["top_ids"].numpy((B, k)), "scores": P["top_scores"].numpy((B, k))}

    out = three_poisons(run, "the capped call")[POISONS[0]]
    _same((out["ids"], out["scores"]), ref.topk(s, bias, tag, n_tags, cap, ex, k), "capped top-k between guard bands")


# ---- the models --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_models_recommend_capped(kind):
    """recommend_capped equals the greedy walk over recommend_deep's full ranking; an int cap >= k is recommend."""
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model(kind)
    N = cat.shape[0]
    n_tags, k = 7, 20
    rng = np.random.default_rng(5)
    tag = torch.from_numpy(rng.integers(0, n_tags, size=N)).to(DEV)                # int64 by news id; entry 0 is never read
    tag[7], tag[9] = -1, n_tags                                                     # never served
    tag_h = tag.cpu().numpy()
    prior = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(DEV)
    for batch in batches:
        B = torch.as_tensor(batch["browsed_ids"]).shape[0]
        per_user = torch.from_numpy(rng.integers(0, 5, size=(B, n_tags))).to(DEV)
        per_user[0] = 0                                                            # everything closed
        for bias in (None, prior):
            full_ids, full_sc = model.recommend_deep(batch, N, cat, item_bias=bias)
            fi, fs = full_ids.cpu().numpy(), full_sc.cpu().numpy()
            for cap, rows in ((2, np.full((B, n_tags), 2)), (per_user[1], per_user[1].cpu().numpy()[None].repeat(B, 0)),
                              (per_user.to(torch.int32), per_user.cpu().numpy())):
                ids, sc = model.recommend_capped(batch, k, cat, tag, cap, item_bias=bias, n_tags=n_tags if isinstance(cap, int) else None)
                for b in range(B):
                    wi, wsc = ref.greedy_over_list(fi[b], fs[b], tag_h, n_tags, rows[b], k)
                    _same((ids[b], sc[b]), (wi, wsc), "%s row %d" % (kind, b))
                assert not (ids == 7).any() and not (ids == 9).any() and not (ids == 0).any()
            assert (ids[0] == -1).all()
            # an int cap >= k with every tag in range is recommend
            ids, sc = model.recommend_capped(batch, k, cat, tag.clamp(0, n_tags - 1), k, item_bias=bias, n_tags=n_tags)
            i0, s0 = model.recommend(batch, k, cat, item_bias=bias)
            _same((ids, sc), (i0, s0), "cap >= k is recommend")
        with pytest.raises(_lib.NrmsError, match="item_tag"):
            model.recommend_capped(batch, 5, cat, tag[:-1], 2, n_tags=n_tags)
        with pytest.raises(_lib.NrmsError, match="n_tags"):
            model.recommend_capped(batch, 5, cat, tag, 2)
    model.check_recommend_ids()


def test_run_v0_max_per_category_flag(tmp_path):
    """A fresh child process with a time limit of its own; nothing is started after it."""
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    out = tmp_path / "rec.txt"
    r = subprocess.run([sys.executable, "-m", "pytorch_news_recommender_amd.run_v0", "--model", "nrms_hip", "--dataset", "synthetic",
                        "--negatives", "catalogue", "--max_batches", "2", "--epochs", "1", "--synthetic_users", "128",
                        "--batch_size", "64", "--num_workers", "0", "--description", "T", "--data_path", str(tmp_path / "data"),
                        "--save_path", str(tmp_path / "save"), "--recommend", "10", "--max_per_category", "2", "--mute_categories", "1",
                        "--recommend_out", str(out)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    pat = (r"%s \(mute 1\): categories per list: ([\d.]+)  largest category share: ([\d.]+)  users: (\d+)"
           r"  hit@1: [\d.]+ \+- [\d.]+  hit@5: [\d.]+ \+- [\d.]+  hit@10: ([\d.]+) \+- ([\d.]+)")
    free = [re.fullmatch(pat % "uncapped", ln) for ln in r.stdout.splitlines() if ln.startswith("uncapped")]
    capped = [re.fullmatch(pat % "at most 2 per category", ln) for ln in r.stdout.splitlines() if ln.startswith("at most 2")]
    assert len(free) == 1 and free[0] and len(capped) == 1 and capped[0], r.stdout[-3000:]
    assert int(capped[0].group(3)) == int(free[0].group(3)) > 0
    # ten news with at most two of a category: at least five categories, and no category above a fifth of a full list
    assert float(capped[0].group(1)) >= 5.0 and float(capped[0].group(2)) <= 0.2 + 1e-9
    assert float(capped[0].group(1)) >= float(free[0].group(1)) and float(capped[0].group(2)) <= float(free[0].group(2))
    lines = open(out).read().splitlines()
    assert len(lines) == int(capped[0].group(3)) and all(re.fullmatch(r"\d+ \[[\d,]*\]", ln) for ln in lines)
