"""nrms_topk_dot_tagged / nrms_rank_dot_tagged on the GPU (a per-user set of item tags on the catalogue in retrieval and exact
ranking, include/nrms_hip.h): exact against tests/topk_tags_ref.py on integer lattice data at every point where the kernels
change path, the consequences (a) to (e) the header states on Gaussian data, the dead-wave skip, determinism, the buffer contract,
the argument errors and the layers above (engine.top_k_tagged / rank_of_tagged, Model.recommend_tagged / rank_targets_tagged,
run_v0 --only_categories).  Every comparison is exact: ids, ranks and score bits.  Parity is unpinned: the reference has no
catalogue retrieval."""
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
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream, pack_tag_mask

from tests import topk_tags_ref as ref

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


def _packed(allow, garbage=None):
    """The packed sets on the device, as the int32 tensor the engine takes (the same 32 bits as ref.pack's uint32)."""
    return torch.from_numpy(ref.pack(allow, garbage).view(np.int32)).to(DEV).contiguous()


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what):
    for g, w, name in zip(got, want, ("first", "second")):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg="%s (%s output)" % (what, name))


def _topk(user, items, k, ex, bias, tag, n_tags, allow, garbage=None):
    s, ids = _engine().top_k_tagged(_t(user, torch.float32), _t(items, torch.float32), k, _t(tag, torch.int32), n_tags,
                                    _packed(allow, garbage), _t(ex, torch.int64), bias=_t(bias, torch.float32))
    return ids.cpu().numpy(), s.cpu().numpy()


def _rank(user, items, tg, ex, bias, tag, n_tags, allow, garbage=None):
    r, s = _engine().rank_of_tagged(_t(user, torch.float32), _t(items, torch.float32), _t(tg, torch.int64), _t(tag, torch.int32), n_tags,
                                    _packed(allow, garbage), _t(ex, torch.int64), bias=_t(bias, torch.float32))
    return r.cpu().numpy(), s.cpu().numpy()


# ---- the data ----------------------------------------------------------------------------------------------------------------
def _tags(N, n_tags, kind, rng):
    """One tag per item, most in [0, n_tags), a few at -1, n_tags and INT32_MAX (open to nobody); sorted: the catalogue stored tag
    after tag, so that whole waves carry one tag; shuffled: the same tags in random row order."""
    t = rng.integers(0, n_tags, size=N).astype(np.int64)
    if N >= 63:
        bad = rng.choice(N, size=6, replace=False)
        t[bad[:2]], t[bad[2:4]], t[bad[4:]] = -1, n_tags, I32_MAX
        t[0] = 0
        t[1] = n_tags - 1
        t[2] = min(31, n_tags - 1)
        t[3] = min(32, n_tags - 1)
    return np.sort(t, kind="stable") if kind == "sorted" else t


def _allow(B, n_tags, kind, rng):
    """mixed: row b takes set kind b % 8 of the list below; few: every user of the batch allows one or two of the same three tags,
    so most tags are closed to a whole block; all: every bit set."""
    a = np.zeros((B, n_tags), dtype=bool)
    if kind == "all":
        a[:] = True
        return a
    if kind == "few":
        pool = sorted({0, n_tags // 2, n_tags - 1})
        for b in range(B):
            a[b, pool[b % len(pool)]] = True
            if b % 5 == 0:
                a[b, pool[(b + 1) % len(pool)]] = True
        return a
    for b in range(B):
        kind_b = b % 8
        if kind_b == 0:
            a[b] = True                                          # everything
        elif kind_b == 1:
            pass                                                 # nothing: an all-padding row
        elif kind_b == 2:
            a[b, 0] = True                                       # bit 0 alone
        elif kind_b == 3:
            a[b, n_tags - 1] = True                              # the last tag alone
        elif kind_b == 4:
            a[b, min(31, n_tags - 1)] = True                     # bit 31 of the first word, bit 0 of the second
            a[b, min(32, n_tags - 1)] = True
        elif kind_b == 5:
            a[b] = rng.random(n_tags) < 0.5
        elif kind_b == 6:
            a[b] = rng.random(n_tags) < 0.1
        else:
            a[b] = True
            a[b, rng.integers(0, n_tags)] = False                # one muted tag
    return a


@functools.lru_cache(maxsize=None)
def _lattice(B, N, d, k, T, n_ex, n_tags, tkind, akind, with_bias):
    """Integer users and items in [-3, 3] (every dot product, and every sum with a multiple of 0.25 below 2^12, is exact in fp32
    whatever the order of summation; ties are abundant, so the id rule is exercised), a bias of multiples of 0.25 with NaN and
    -inf entries, exclude lists with -1, N and a duplicate, and targets that name a closed id, an excluded one, a duplicate, -1, a
    NaN-prior id and N."""
    rng = np.random.default_rng(100003 * d + 1009 * N + 17 * k + B + T + n_ex + 31 * n_tags)
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
    tag = _tags(N, n_tags, tkind, rng)
    allow = _allow(B, n_tags, akind, rng)
    ex = None
    if n_ex:
        ex = rng.integers(0, max(N, 1), size=(B, n_ex)).astype(np.int64)
        ex[:, 0], ex[:, 1], ex[:, 2] = -1, N, ex[:, min(3, n_ex - 1)]
    tg = rng.integers(0, max(N, 1), size=(B, T)).astype(np.int64)
    open_ = ref.eligible(np.zeros((B, N), dtype=np.float32), tag, n_tags, allow, None) if N else np.zeros((B, 0), dtype=bool)
    for b in range(B):                                     # the first target is open to its user, where anything is
        inside = np.nonzero(open_[b])[0]
        if len(inside):
            tg[b, 0] = inside[(7 * b) % len(inside)]
    if T >= 8 and N >= 63:
        for b in range(B):
            out = np.nonzero(~open_[b])[0]
            tg[b, 1] = out[b % len(out)] if len(out) else 0
            tg[b, 2] = ex[b, min(4, n_ex - 1)] if ex is not None else tg[b, 0]
            tg[b, 3] = tg[b, 0]
            tg[b, 4] = -1
            tg[b, 5] = np.nonzero(np.isnan(bias))[0][0] if with_bias else N
            tg[b, 6] = N
    for a in (user, items, s, tag, allow, tg):
        a.setflags(write=False)
    return user, items, s, bias, tag, allow, ex, tg


# (B, N, d, k, T, n_exclude, n_tags, tags, sets, bias): every value of B {1, 31, 32, 33, 65}, N {0, 1, 63, 64, 65, 2100, 5000},
# d {1, 3, 8, 31, 64, 301}, k {1, 65, 193, 256}, T {1, 32}, n_exclude {0, 50, 70}, n_tags {1, 31, 32, 33, 64, 294, 512}
LATTICE = [
    (1, 0, 3, 1, 1, 0, 1, "shuffled", "mixed", False),            # an empty catalogue
    (1, 1, 1, 1, 1, 0, 1, "shuffled", "all", True),               # one item, one user, one tag, d = 1
    (31, 63, 3, 65, 32, 50, 31, "shuffled", "mixed", True),       # a ragged user tile, less than one wave step, the scalar path
    (32, 64, 8, 65, 1, 0, 32, "sorted", "mixed", False),          # one tile of users and one wave step; one whole allow word
    (33, 65, 31, 1, 32, 70, 33, "sorted", "mixed", True),         # a padded user tile, a tail of one item; two allow words; global excludes
    (65, 2100, 64, 193, 32, 50, 64, "sorted", "mixed", True),     # two slices, the two-wave block from k = 193, the VEC path
    (33, 2100, 301, 256, 1, 70, 294, "shuffled", "mixed", False), # MIND's sub-categories, the largest k, whole blocks of 32 and a tail
    (65, 5000, 8, 65, 32, 0, 512, "sorted", "mixed", True),       # three slices, three user tiles, the largest tag count
    (32, 5000, 64, 1, 1, 50, 19, "sorted", "few", False),         # MIND's categories, sorted: whole waves dead in a live block
    (32, 5000, 64, 1, 1, 50, 19, "shuffled", "few", False),       # the same sets on shuffled rows: the skip seldom fires
    (65, 2100, 31, 193, 32, 70, 33, "sorted", "few", True),       # dead waves in the two-wave block, ragged last tile
    (1, 5000, 301, 256, 32, 50, 294, "sorted", "mixed", True),    # one user (every tag open) against several slices
]


@pytest.mark.parametrize("B,N,d,k,T,n_ex,n_tags,tkind,akind,with_bias", LATTICE)
def test_exact_on_lattice_data(B, N, d, k, T, n_ex, n_tags, tkind, akind, with_bias):
    user, items, s, bias, tag, allow, ex, tg = _lattice(B, N, d, k, T, n_ex, n_tags, tkind, akind, with_bias)
    want = ref.topk(s, bias, tag, n_tags, allow, ex, k)
    if N >= 63 and akind == "mixed" and B >= 31:          # on the CPU-side data: the test cannot pass by ignoring the tags
        every = ref.topk(s, bias, tag, n_tags, np.ones_like(allow), ex, k)
        assert (want[0][1] == -1).all() and (every[0][1] >= 0).any()                                    # the empty set
        assert sum(not np.array_equal(want[0][b], every[0][b]) for b in range(B)) >= B // 3
    garbage = 0xFFFFFFFF if (B + N) % 2 else 0xA5A5A5A5             # the ignored bits of the last word are never zero here
    _same(_topk(user, items, k, ex, bias, tag, n_tags, allow, garbage), want, "tagged top-k")
    got = _rank(user, items, tg, ex, bias, tag, n_tags, allow, garbage)
    _same(got, ref.ranks(s, bias, tag, n_tags, allow, ex, tg), "tagged rank")
    if T >= 8 and N >= 63:
        assert (got[0][:, 4] == 0).all() and (got[0][:, 6] == 0).all() and (got[1][:, 4] == -np.inf).all()
        t1 = tag[tg[:, 1]]
        closed = ~((t1 >= 0) & (t1 < n_tags) & allow[np.arange(B), np.clip(t1, 0, n_tags - 1)])
        assert closed.any() and (got[0][closed, 1] == 0).all()                     # a target closed by its tag


def test_tag_and_bit_edges():
    """Tags at -1, n_tags and INT32_MAX are open to nobody, even with every bit (and every ignored bit) set; mask bits at positions
    0, 31, 32 and n_tags - 1 each open exactly their tag; an all-zero row gives padding and rank 0."""
    N, d, n_tags = 70, 8, 40
    rng = np.random.default_rng(7)
    user = rng.integers(-3, 4, size=(6, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)
    tag = (np.arange(N, dtype=np.int64) % n_tags)
    tag[5], tag[6], tag[7] = -1, n_tags, I32_MAX
    allow = np.zeros((6, n_tags), dtype=bool)
    allow[0] = True
    allow[1, 0] = allow[2, 31] = allow[3, 32] = allow[4, n_tags - 1] = True
    for garbage in (None, 0xFFFFFFFF):
        ids, sc = _topk(user, items, N, None, None, tag, n_tags, allow, garbage)
        _same((ids, sc), ref.topk(s, None, tag, n_tags, allow, None, N), "edges")
        assert (ids[0] >= 0).sum() == N - 3 and not np.isin([5, 6, 7], ids[0]).any()
        for row, t in ((1, 0), (2, 31), (3, 32), (4, n_tags - 1)):
            assert sorted(ids[row][ids[row] >= 0].tolist()) == [n for n in range(N) if tag[n] == t]
        assert (ids[5] == -1).all() and (sc[5] == -np.inf).all()
        tg = np.tile(np.array([[0, 31, 32, 39, 5, 6, 7, 40]]), (6, 1))
        r, rs = _rank(user, items, tg, None, None, tag, n_tags, allow, garbage)
        _same((r, rs), ref.ranks(s, None, tag, n_tags, allow, None, tg), "edges")
        assert (r[0, :4] > 0).all() and (r[:, 4:7] == 0).all() and (r[5] == 0).all()
        assert r[1, 0] > 0 and r[2, 1] > 0 and r[3, 2] > 0 and r[4, 3] > 0 and r[1, 1] == 0 and r[2, 0] == 0


def test_one_user_opens_what_the_other_31_close():
    """A block in which exactly one user opens a tag: its waves are live for that user alone, on sorted and on shuffled rows."""
    B, N, d, k, n_tags = 32, 2100, 8, 65, 19
    rng = np.random.default_rng(21)
    user = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)
    allow = np.zeros((B, n_tags), dtype=bool)
    allow[:, 3] = True
    allow[17, 3] = False
    allow[17, 11] = True
    tg = rng.integers(0, N, size=(B, 8)).astype(np.int64)
    for tag in (np.sort(rng.integers(0, n_tags, size=N)), rng.integers(0, n_tags, size=N)):
        ids, sc = _topk(user, items, k, None, None, tag, n_tags, allow)
        _same((ids, sc), ref.topk(s, None, tag, n_tags, allow, None, k), "one opener")
        assert (tag[ids[17]] == 11).all() and (tag[ids[np.arange(B) != 17]] == 3).all()
        _same(_rank(user, items, tg, None, None, tag, n_tags, allow), ref.ranks(s, None, tag, n_tags, allow, None, tg), "one opener")


# ---- Gaussian data: the consequences of the header ---------------------------------------------------------------------------
N_REAL, B_REAL, TAGS_REAL = 5000, 65, 294


@functools.lru_cache(maxsize=1)
def _real():
    """B = 65, N = 5 000, d = 300 Gaussian data with two NaN item rows (NaN scores for everybody) and duplicated item rows (equal
    scores: the id rule decides), 294 tags with a few outside their range, mixed sets, a bias with NaN and -inf entries."""
    B, N, d = B_REAL, N_REAL, 300
    g = torch.Generator(device=DEV).manual_seed(11)
    user = torch.randn(B, d, device=DEV, generator=g)
    items = torch.randn(N, d, device=DEV, generator=g)
    items[100:110] = items[2000:2010]
    items[[77, 3001]] = float("nan")
    ex = torch.randint(0, N, (B, 50), device=DEV, generator=g)
    bias = (torch.randn(N, device=DEV, generator=g) * 6.0).contiguous()
    bias[torch.randint(0, N, (20,), device=DEV, generator=g)] = float("nan")
    bias[torch.randint(0, N, (3,), device=DEV, generator=g)] = float("-inf")
    tg = torch.randint(0, N, (B, 8), device=DEV, generator=g)
    rng = np.random.default_rng(3)
    tag = _tags(N, TAGS_REAL, "shuffled", rng)
    allow = _allow(B, TAGS_REAL, "mixed", rng)
    return user, items.contiguous(), ex, bias, tg, _t(tag, torch.int32), allow


@pytest.mark.parametrize("with_bias", [False, True])
def test_all_open_is_the_untagged_call(with_bias):
    """(a)"""
    user, items, ex, bias, tg, tag, allow = _real()
    eng = _engine()
    b = bias if with_bias else None
    t = torch.clamp(tag, 0, TAGS_REAL - 1)
    every = _packed(np.ones_like(allow), 0x5A5A5A5A)
    for k in (10, 100, 256):
        _same(eng.top_k_tagged(user, items, k, t, TAGS_REAL, every, ex, bias=b), eng.top_k(user, items, k, ex, bias=b), "(a) k=%d" % k)
    _same(eng.rank_of_tagged(user, items, tg, t, TAGS_REAL, every, ex, bias=b), eng.rank_of(user, items, tg, ex, bias=b), "(a) ranks")


@pytest.mark.parametrize("with_bias", [False, True])
def test_row_equals_the_biased_call_with_nan_where_closed(with_bias):
    """(b), for one user of every set kind and the ragged last tile's user."""
    user, items, ex, bias, tg, tag, allow = _real()
    eng = _engine()
    b = bias if with_bias else None
    k = 100
    pk = _packed(allow)
    sc, ids = eng.top_k_tagged(user, items, k, tag, TAGS_REAL, pk, ex, bias=b)
    r, rs = eng.rank_of_tagged(user, items, tg, tag, TAGS_REAL, pk, ex, bias=b)
    tn = tag.cpu().numpy()
    bn = None if b is None else b.cpu().numpy()
    for u in list(range(8)) + [37, 64]:
        b1 = _t(ref.tags_as_bias(bn, tn, TAGS_REAL, allow[u], N_REAL), torch.float32)
        one = slice(u, u + 1)
        s1, i1 = eng.top_k(user[one].contiguous(), items, k, ex[one].contiguous(), bias=b1)
        _same((ids[one], sc[one]), (i1, s1), "(b) user %d" % u)
        _same((r[one], rs[one]), eng.rank_of(user[one].contiguous(), items, tg[one].contiguous(), ex[one].contiguous(), bias=b1), "(b) ranks %d" % u)
    assert (ids[0] >= 0).all() and (ids[1] == -1).all() and (ids[2] == -1).any() and (ids[2] >= 0).any()


def _raw_topk(user, items, bias, tag, n_tags, allow, ex, k, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N = items.shape[0]
    need = int(lib.nrms_topk_dot_tagged_workspace_bytes(B, C.c_int64(N), d, k))
    assert need == int(lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    sc = torch.empty(B, k, dtype=torch.float32, device=DEV)
    ids = torch.empty(B, k, dtype=torch.int64, device=DEV)
    rc = lib.nrms_topk_dot_tagged(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), _lib.ptr(bias), _lib.ptr(tag), n_tags,
                                  _lib.ptr(allow), _lib.ptr(ex), 0 if ex is None else ex.shape[1], _lib.ptr(sc), _lib.ptr(ids),
                                  _lib.ptr(ws), C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_topk_dot_tagged")
    return ids, sc


def _raw_rank(user, items, bias, tag, n_tags, allow, tg, ex, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N, T = items.shape[0], tg.shape[1]
    n_ex = 0 if ex is None else ex.shape[1]
    need = int(lib.nrms_rank_dot_tagged_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    assert need == int(lib.nrms_rank_dot_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    r = torch.empty(B, T, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, T, dtype=torch.float32, device=DEV)
    rc = lib.nrms_rank_dot_tagged(B, C.c_int64(N), d, T, _lib.ptr(user), _lib.ptr(items), _lib.ptr(bias), _lib.ptr(tag), n_tags,
                                  _lib.ptr(allow), _lib.ptr(tg), _lib.ptr(ex), n_ex, _lib.ptr(r), _lib.ptr(sc), _lib.ptr(ws),
                                  C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_rank_dot_tagged")
    return r, sc


def test_row_depends_on_its_own_user_and_set_only():
    """(c): two runs, batch splits, the user's position, the ignored bits, the neighbours' sets, a poisoned workspace."""
    user, items, ex, bias, tg, tag, allow = _real()
    eng = _engine()
    k, nt = 100, TAGS_REAL
    pk = _packed(allow)
    sc, ids = eng.top_k_tagged(user, items, k, tag, nt, pk, ex, bias=bias)
    r, rs = eng.rank_of_tagged(user, items, tg, tag, nt, pk, ex, bias=bias)
    _same(eng.top_k_tagged(user, items, k, tag, nt, pk, ex, bias=bias), (sc, ids), "second run")
    _same(eng.rank_of_tagged(user, items, tg, tag, nt, pk, ex, bias=bias), (r, rs), "second run")
    gb = _packed(allow, 0xFFFFFFFF)
    assert not torch.equal(gb, pk)
    _same(eng.top_k_tagged(user, items, k, tag, nt, gb, ex, bias=bias), (sc, ids), "ignored bits")
    _same(eng.rank_of_tagged(user, items, tg, tag, nt, gb, ex, bias=bias), (r, rs), "ignored bits")
    parts = [slice(0, 1), slice(1, 33), slice(33, 65)]
    cut = lambda a, p: a[p].contiguous()
    pkk = [eng.top_k_tagged(cut(user, p), items, k, tag, nt, cut(pk, p), cut(ex, p), bias=bias) for p in parts]
    prr = [eng.rank_of_tagged(cut(user, p), items, cut(tg, p), tag, nt, cut(pk, p), cut(ex, p), bias=bias) for p in parts]
    _same((torch.cat([x[0] for x in pkk]), torch.cat([x[1] for x in pkk])), (sc, ids), "batch split")
    _same((torch.cat([x[0] for x in prr]), torch.cat([x[1] for x in prr])), (r, rs), "batch split")
    perm = torch.randperm(B_REAL, generator=torch.Generator().manual_seed(3)).to(DEV)
    up = lambda a: a[perm].contiguous()
    _same(eng.top_k_tagged(up(user), items, k, tag, nt, up(pk), up(ex), bias=bias), (sc[perm], ids[perm]), "user permutation")
    _same(eng.rank_of_tagged(up(user), items, up(tg), tag, nt, up(pk), up(ex), bias=bias), (r[perm], rs[perm]), "user permutation")
    # user 5 (a random half of the tags) in the middle of 31 users that allow nothing, then everything: its row may not move
    u = 5
    for fill in (False, True):
        a2 = np.full((32, nt), fill, dtype=bool)
        a2[13] = allow[u]
        rows = torch.full((32,), 40, dtype=torch.int64, device=DEV)
        rows[13] = u
        s2, i2 = eng.top_k_tagged(user[rows].contiguous(), items, k, tag, nt, _packed(a2), ex[rows].contiguous(), bias=bias)
        r2, rs2 = eng.rank_of_tagged(user[rows].contiguous(), items, tg[rows].contiguous(), tag, nt, _packed(a2), ex[rows].contiguous(), bias=bias)
        _same((s2[13:14], i2[13:14]), (sc[u:u + 1], ids[u:u + 1]), "neighbours allow %s" % ("everything" if fill else "nothing"))
        _same((r2[13:14], rs2[13:14]), (r[u:u + 1], rs[u:u + 1]), "neighbours allow %s" % ("everything" if fill else "nothing"))
        if not fill:
            assert (i2[:13] == -1).all() and (i2[14:] == -1).all() and (r2[:13] == 0).all()
    for fill in (0xFF, 0x00):
        _same(_raw_topk(user, items, bias, tag, nt, pk, ex, k, fill), (ids, sc), "workspace 0x%02X" % fill)
        _same(_raw_rank(user, items, bias, tag, nt, pk, tg, ex, fill), (r, rs), "workspace 0x%02X" % fill)


def test_prefix_and_served_list_ranks():
    """(d) the first k' columns of a call with k are the call with k'; (e) the served ids rank 1, 2, ... with the same score bits."""
    user, items, ex, bias, tg, tag, allow = _real()
    eng = _engine()
    pk = _packed(allow)
    sc, ids = eng.top_k_tagged(user, items, 256, tag, TAGS_REAL, pk, ex, bias=bias)
    for k in (1, 65, 193):
        s2, i2 = eng.top_k_tagged(user, items, k, tag, TAGS_REAL, pk, ex, bias=bias)
        _same((s2, i2), (sc[:, :k], ids[:, :k]), "(d) k'=%d" % k)
    r, rs = eng.rank_of_tagged(user, items, ids, tag, TAGS_REAL, pk, ex, bias=bias)
    live = ids >= 0
    want = torch.arange(1, 257, dtype=torch.int32, device=DEV).expand(B_REAL, 256)
    assert live.any() and (~live).any() and torch.equal(r[live], want[live]) and (r[~live] == 0).all()
    _same((rs,), (sc,), "(e) scores of the served list")


def test_nothing_allowed_and_empty_extents():
    user, items, ex, bias, tg, tag, allow = _real()
    eng = _engine()
    none = _packed(np.zeros_like(allow), 0xFFFFFFFF)
    sc, ids = eng.top_k_tagged(user, items, 10, tag, TAGS_REAL, none, ex, bias=bias)
    r, rs = eng.rank_of_tagged(user, items, tg, tag, TAGS_REAL, none, ex, bias=bias)
    assert (ids == -1).all() and (sc == -float("inf")).all() and (r == 0).all() and (rs == -float("inf")).all()
    # N = 0: padding and rank 0; B = 0: a no-op
    empty = torch.empty(0, 300, device=DEV)
    no_tag = torch.empty(0, dtype=torch.int32, device=DEV)
    sc, ids = eng.top_k_tagged(user, empty, 10, no_tag, TAGS_REAL, _packed(allow), None)
    r, rs = eng.rank_of_tagged(user, empty, tg, no_tag, TAGS_REAL, _packed(allow), None)
    assert (ids == -1).all() and (sc == -float("inf")).all() and (r == 0).all() and (rs == -float("inf")).all()
    lib = _lib.load()
    ws = torch.empty(1 << 10, dtype=torch.int64, device=DEV)
    assert lib.nrms_topk_dot_tagged(0, C.c_int64(N_REAL), 300, 10, None, None, None, None, TAGS_REAL, None, None, 0, None, None,
                                    _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream()) == _lib.NRMS_OK
    assert lib.nrms_rank_dot_tagged(0, C.c_int64(N_REAL), 300, 8, None, None, None, None, TAGS_REAL, None, None, None, 0, None, None,
                                    _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream()) == _lib.NRMS_OK


# ---- the buffer contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2, 5, 10])
def test_buffer_contract(case):
    """Outputs and the workspace at the queried size between guard bands, the workspace poisoned three ways; bias, item_tag and
    allow are guarded too, at exactly their sizes."""
    from tests.guarded import POISONS, Pool
    from tests.test_hip_buffer_contracts import dev, ok, refuses_undersized, three_poisons
    lib = _lib.load()
    B, N, d, k, T, n_ex, n_tags, tkind, akind, with_bias = LATTICE[case]
    user, items, s, bias, tag, allow, ex, tg = _lattice(*LATTICE[case])
    ud, itd, tgd, exd = dev(np.array(user)), dev(np.array(items)), dev(np.array(tg), torch.int64), dev(ex, torch.int64)
    W = (n_tags + 31) // 32
    need_k = int(lib.nrms_topk_dot_tagged_workspace_bytes(B, C.c_int64(N), d, k))
    need_r = int(lib.nrms_rank_dot_tagged_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    assert need_k > 0 and need_r > 0

    def run(poison):
        P = Pool(poison)
        P.elems("bias", N, torch.float32, init=torch.from_numpy(np.array(bias)))
        P.elems("tag", N, torch.int32, init=torch.from_numpy(np.array(tag)).to(torch.int32))
        P.elems("allow", B * W, torch.int32, init=torch.from_numpy(ref.pack(allow, 0xFFFFFFFF).view(np.int32)).reshape(-1))
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, torch.int64), P.new("ws_topk", need_k)
        P.elems("ranks", B * T, torch.int32), P.elems("target_scores", B * T), P.new("ws_rank", need_r)

        def call_k(nbytes):
            return lib.nrms_topk_dot_tagged(B, C.c_int64(N), d, k, _lib.ptr(ud), _lib.ptr(itd), P["bias"].ptr, P["tag"].ptr, n_tags,
                                            P["allow"].ptr, _lib.ptr(exd), n_ex, P["top_scores"].ptr, P["top_ids"].ptr,
                                            P["ws_topk"].ptr, C.c_size_t(nbytes), _stream())

        def call_r(nbytes):
            return lib.nrms_rank_dot_tagged(B, C.c_int64(N), d, T, _lib.ptr(ud), _lib.ptr(itd), P["bias"].ptr, P["tag"].ptr, n_tags,
                                            P["allow"].ptr, _lib.ptr(tgd), _lib.ptr(exd), n_ex, P["ranks"].ptr,
                                            P["target_scores"].ptr, P["ws_rank"].ptr, C.c_size_t(nbytes), _stream())

        snap = [P[n].snapshot() for n in ("bias", "tag", "allow")]
        ok(call_k(need_k), "nrms_topk_dot_tagged")
        P.intact("nrms_topk_dot_tagged")
        ok(call_r(need_r), "nrms_rank_dot_tagged")
        P.intact("nrms_rank_dot_tagged")
        assert all(P[n].unchanged_since(sn) for n, sn in zip(("bias", "tag", "allow"), snap))
        if poison == POISONS[0]:
            keep = {n: P[n].numpy() for n in ("top_scores", "top_ids", "ranks", "target_scores")}
            refuses_undersized(call_k, P, need_k, "nrms_topk_dot_tagged")
            refuses_undersized(call_r, P, need_r, "nrms_rank_dot_tagged")
            assert all(np.array_equal(_bits(keep[n]), _bits(P[n].numpy())) for n in keep)
        return {"ids": P["top_ids"].numpy((B, k)), "scores": P["top_scores"].numpy((B, k)), "ranks": P["ranks"].numpy((B, T)),
                "tscores": P["target_scores"].numpy((B, T))}

    out = three_poisons(run, "the tagged calls")[POISONS[0]]
    _same((out["ids"], out["scores"]), ref.topk(s, bias, tag, n_tags, allow, ex, k), "tagged top-k between guard bands")
    _same((out["ranks"], out["tscores"]), ref.ranks(s, bias, tag, n_tags, allow, ex, tg), "tagged rank between guard bands")


# ---- argument errors: refused on the host, before any launch; only the return codes and messages are read ---------------------
def test_argument_errors():
    lib = _lib.load()
    user, items, ex, bias, tg, tag, allow = _real()
    pk = _packed(allow)
    B, N, d, k, T = B_REAL, N_REAL, 300, 10, 8
    ws = torch.empty(1 << 20, dtype=torch.int64, device=DEV)
    sc = torch.full((B, k), 5.0, device=DEV)
    ids = torch.full((B, k), 5, dtype=torch.int64, device=DEV)
    r = torch.full((B, T), 5, dtype=torch.int32, device=DEV)
    rs = torch.full((B, T), 5.0, device=DEV)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)

    def topk(B=B, N=N, d=d, k=k, bias=_lib.ptr(bias), tag=_lib.ptr(tag), n_tags=TAGS_REAL, allow=_lib.ptr(pk), n_ex=0, nbytes=ws.numel() * 8):
        return lib.nrms_topk_dot_tagged(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), bias, tag, n_tags, allow, None, n_ex,
                                        _lib.ptr(sc), _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(nbytes), _stream())

    def rank(B=B, N=N, d=d, T=T, bias=_lib.ptr(bias), tag=_lib.ptr(tag), n_tags=TAGS_REAL, allow=_lib.ptr(pk), n_ex=0, nbytes=ws.numel() * 8):
        return lib.nrms_rank_dot_tagged(B, C.c_int64(N), d, T, _lib.ptr(user), _lib.ptr(items), bias, tag, n_tags, allow, _lib.ptr(tg),
                                        None, n_ex, _lib.ptr(r), _lib.ptr(rs), _lib.ptr(ws), C.c_size_t(nbytes), _stream())

    for call, who, size in ((topk, b"topk_dot_tagged: ", "k"), (rank, b"rank_dot_tagged: ", "T")):
        for kw, word in ((dict(tag=None), b"item_tag is null"), (dict(allow=None), b"allow is null"),
                         (dict(tag=off(tag, 2)), b"item_tag must be 4-byte aligned"), (dict(allow=off(pk, 1)), b"allow must be 4-byte aligned"),
                         (dict(bias=off(bias, 2)), b"bias must be 4-byte aligned"), (dict(n_tags=0), b"n_tags must be"),
                         (dict(n_tags=513), b"n_tags must be"), (dict(n_tags=-1), b"n_tags must be"), (dict(B=-1), b"B must be"),
                         (dict(N=-1), b"N must be"), (dict(d=0), b"d must be"), ({size: 0}, size.encode() + b" must be"),
                         ({size: 257}, size.encode() + b" must be"), (dict(n_ex=-1), b"n_exclude must be")):
            assert call(**kw) == _lib.NRMS_EINVAL, (who, kw)
            msg = lib.nrms_last_error()
            assert msg.startswith(who) and word in msg, msg
        assert call(nbytes=8) == _lib.NRMS_EWORKSPACE
        assert lib.nrms_last_error().startswith(who)
    torch.cuda.synchronize()
    assert (sc == 5.0).all() and (ids == 5).all() and (r == 5).all() and (rs == 5.0).all()        # nothing was launched
    assert lib.nrms_topk_dot_tagged_workspace_bytes(B, C.c_int64(N), d, 257) == 0
    assert lib.nrms_rank_dot_tagged_workspace_bytes(B, C.c_int64(N), d, 33, 0) == 0
    assert topk(B=0) == _lib.NRMS_OK and rank(B=0) == _lib.NRMS_OK                                  # B = 0 is a no-op


def test_engine_arguments():
    user, items, ex, bias, tg, tag, allow = _real()
    eng = _engine()
    pk = _packed(allow)
    a = eng.top_k_tagged(user, items, 10, tag, TAGS_REAL, pk, ex)
    ab = torch.from_numpy(allow).to(DEV)
    _same(eng.top_k_tagged(user, items, 10, tag, TAGS_REAL, ab, ex), a, "a bool allow is packed by the engine")
    assert torch.equal(pack_tag_mask(ab), pk)
    far = tag.long().clone()
    far[tag.long() == TAGS_REAL] = 2 ** 40                                          # an int64 tag outside int32: open to nobody
    _same(eng.top_k_tagged(user, items, 10, far, TAGS_REAL, pk, ex), a, "int64 tags")
    _same(eng.rank_of_tagged(user, items, tg, far, TAGS_REAL, ab, ex), eng.rank_of_tagged(user, items, tg, tag, TAGS_REAL, pk, ex), "int64 tags")
    wide = torch.randint(0, N_REAL, (B_REAL, 40), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    r, rs = eng.rank_of_tagged(user, items, wide, tag, TAGS_REAL, pk, ex)            # more than 32 targets: column chunks
    _same(eng.rank_of_tagged(user, items, wide[:, 32:].contiguous(), tag, TAGS_REAL, pk, ex), (r[:, 32:], rs[:, 32:]), "chunks")
    for bad in (dict(item_tag=tag[:-1].contiguous()), dict(item_tag=tag.float()), dict(item_tag=tag.cpu()), dict(allow=pk[:-1].contiguous()),
                dict(allow=pk.long()), dict(allow=ab[:, :-1].contiguous()), dict(n_tags=0), dict(n_tags=513)):
        kw = dict(item_tag=tag, n_tags=TAGS_REAL, allow=pk)
        kw.update(bad)
        with pytest.raises(_lib.NrmsError, match="item_tag|allow|n_tags"):
            eng.top_k_tagged(user, items, 10, kw["item_tag"], kw["n_tags"], kw["allow"], ex)
        with pytest.raises(_lib.NrmsError, match="item_tag|allow|n_tags"):
            eng.rank_of_tagged(user, items, tg, kw["item_tag"], kw["n_tags"], kw["allow"], ex)


# ---- the models --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_models_recommend_and_rank_inside_a_tag_set(kind):
    """recommend_tagged / rank_targets_tagged agree with recommend_deep's full ranking filtered on the host."""
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model(kind)
    N = cat.shape[0]
    n_tags = 37
    rng = np.random.default_rng(5)
    tag = torch.from_numpy(rng.integers(0, n_tags, size=N)).to(DEV)                # int64 by news id; entry 0 is never read
    tag[7] = -1                                                                    # untagged: never served
    tag[9] = n_tags
    prior = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(DEV)
    for batch in batches:
        B = torch.as_tensor(batch["browsed_ids"]).shape[0]
        allow = torch.from_numpy(rng.random((B, n_tags)) < 0.4).to(DEV)
        allow[0] = False                                                           # nothing allowed
        if B > 1:
            allow[1] = True
        for bias in (None, prior):
            full_ids, full_sc = model.recommend_deep(batch, N, cat, item_bias=bias)         # the whole ranking, then -1
            k = 20
            for al in (allow, pack_tag_mask(allow)):
                ids, sc = model.recommend_tagged(batch, k, cat, tag, al, item_bias=bias)
                for b in range(B):
                    fi, fs = full_ids[b], full_sc[b]
                    t = tag[fi.clamp(min=0)]
                    keep = (fi > 0) & (t >= 0) & (t < n_tags) & allow[b][t.clamp(0, n_tags - 1)]
                    wi, wsc = fi[keep][:k], fs[keep][:k]
                    n = wi.shape[0]
                    assert torch.equal(ids[b, :n], wi) and torch.equal(sc[b, :n].view(torch.int32), wsc.view(torch.int32))
                    assert (ids[b, n:] == -1).all() and (sc[b, n:] == -float("inf")).all()
                assert (ids[0] == -1).all() and not (ids == 7).any() and not (ids == 9).any() and (ids > 0).any()
                r, rs = model.rank_targets_tagged(batch, ids, cat, tag, al, item_bias=bias)
                live = ids > 0
                want = torch.arange(1, k + 1, dtype=torch.int32, device=DEV).expand(B, k)
                assert torch.equal(r[live], want[live]) and (r[~live] == 0).all()
                assert torch.equal(rs.view(torch.int32), sc.view(torch.int32))
            # tagged ranks never exceed the untagged ones for eligible targets
            r0, _ = model.rank_targets(batch, ids, cat, item_bias=bias)
            assert (r[live] <= r0[live]).all()
        with pytest.raises(_lib.NrmsError, match="item_tag"):
            model.recommend_tagged(batch, 5, cat, tag[:-1], allow)
        with pytest.raises(_lib.NrmsError, match="allow"):
            model.rank_targets_tagged(batch, ids, cat, tag, allow[:-1])
    model.check_recommend_ids()


def test_run_v0_only_categories_flag(tmp_path):
    """A fresh child process with a time limit of its own; nothing is started after it."""
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "pytorch_news_recommender_amd.run_v0", "--model", "nrms_hip", "--dataset", "synthetic",
                        "--negatives", "catalogue", "--max_batches", "2", "--epochs", "1", "--synthetic_users", "128",
                        "--batch_size", "64", "--num_workers", "0", "--description", "T", "--data_path", str(tmp_path / "data"),
                        "--save_path", str(tmp_path / "save"), "--recommend", "5", "--only_categories", "own"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("recommend inside")]
    assert len(line) == 1, r.stdout[-3000:]
    m = re.fullmatch(r"recommend inside per-user categories \(only own\): (\d+) users, (\d+) of (\d+) slots filled, "
                     r"(\d+) outside the allowed categories", line[0])
    assert m, line[0]
    assert int(m.group(1)) > 0 and 0 < int(m.group(2)) <= int(m.group(3)) and int(m.group(4)) == 0
