"""nrms_topk_dot_adjusted / nrms_rank_dot_adjusted on the GPU (per-user score adjustments on the catalogue in retrieval and exact
ranking, include/nrms_hip.h): exact against tests/topk_adjust_ref.py on lattice data (small integers, deltas that are multiples of
0.25: every sum is exact in fp32) at every point where the kernels change path, the slot and delta edge cases, the consequences
(a) to (f) the header states on Gaussian data, the buffer contract, the argument errors and the layers above
(engine.top_k_adjusted / rank_of_adjusted, Model.recommend_adjusted / rank_targets_adjusted, run_v0 --seen_discount).  Every
comparison is exact: ids, ranks and score bits; the feature needs no tolerance.  Parity is unpinned: the reference has no catalogue
retrieval."""
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

from tests import topk_adjust_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX = 2 ** 63 - 1
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


def _topk(user, items, k, ex, bias, aid, adl):
    s, ids = _engine().top_k_adjusted(_t(user, torch.float32), _t(items, torch.float32), k, _t(aid, torch.int64),
                                      _t(adl, torch.float32), _t(ex, torch.int64), bias=_t(bias, torch.float32))
    return ids.cpu().numpy(), s.cpu().numpy()


def _rank(user, items, tg, ex, bias, aid, adl):
    r, s = _engine().rank_of_adjusted(_t(user, torch.float32), _t(items, torch.float32), _t(tg, torch.int64), _t(aid, torch.int64),
                                      _t(adl, torch.float32), _t(ex, torch.int64), bias=_t(bias, torch.float32))
    return r.cpu().numpy(), s.cpu().numpy()


# ---- the data ----------------------------------------------------------------------------------------------------------------
def _slots(B, N, E, rng, amp=64):
    """Random slots: most name a row of [0, N), a few are empty (-1, N, INT64_MAX), some rows name one id twice with different
    deltas; deltas are multiples of 0.25 in [-amp, amp] with +0.0, +inf, -inf and NaN sprinkled in."""
    aid = rng.integers(0, max(N, 1), size=(B, E)).astype(np.int64)
    adl = (rng.integers(-4 * amp, 4 * amp + 1, size=(B, E)) * 0.25).astype(np.float32)
    if E >= 8:
        for b in range(B):
            aid[b, rng.integers(0, E)] = (-1, N, I64_MAX)[b % 3]
            e0, e1 = rng.choice(E, size=2, replace=False)
            aid[b, e1] = aid[b, e0]                                  # one id in two slots: the lower one counts
            sp = rng.choice(E, size=4, replace=False)
            adl[b, sp[0]], adl[b, sp[1]], adl[b, sp[2]], adl[b, sp[3]] = 0.0, np.inf, -np.inf, np.nan
    return aid, adl


@functools.lru_cache(maxsize=None)
def _lattice(B, N, d, k, T, n_ex, E, with_bias):
    """Integer users and items in [-3, 3] (every dot product, and every sum with multiples of 0.25 below 2^12, is exact in fp32
    whatever the order of summation; ties are abundant, so the id rule is exercised), a bias of multiples of 0.25 with NaN and -inf
    entries, exclude lists with -1, N and a duplicate, slots from _slots (the first also excluded), and targets that name an
    adjusted id, an excluded one, a duplicate, -1, a NaN-delta id and N."""
    rng = np.random.default_rng(100003 * d + 1009 * N + 17 * k + B + T + n_ex + 31 * E)
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
    aid, adl = _slots(B, N, E, rng)
    ex = None
    if n_ex:
        ex = rng.integers(0, max(N, 1), size=(B, n_ex)).astype(np.int64)
        ex[:, 0], ex[:, 1], ex[:, 2] = -1, N, ex[:, min(3, n_ex - 1)]
        if E:
            ex[:, 4] = aid[:, 0]                                     # excluded and adjusted: excluded
    tg = rng.integers(0, max(N, 1), size=(B, T)).astype(np.int64)
    if T >= 8 and N >= 63 and E >= 8:
        for b in range(B):
            tg[b, 0] = aid[b, 1]
            tg[b, 1] = ex[b, 4] if ex is not None else aid[b, 0]
            tg[b, 2] = tg[b, 0]
            tg[b, 3] = -1
            tg[b, 4] = aid[b, np.nonzero(np.isnan(adl[b]))[0][0]]
            tg[b, 5] = N
    for a in (user, items, s, aid, adl, tg):
        a.setflags(write=False)
    return user, items, s, bias, aid, adl, ex, tg


# (B, N, d, k, T, n_exclude, E, bias).  N = 5000 is three top-k slices of 2048 rows and ten rank slices; a block stages at most 2048
# slots for k <= 192 and 1024 above, so E = 64 in a single slice comes close to filling the list and E = 65 close to overflowing it
# (a few of the random slots are empty; test_staged_list_capacity_boundary pins the boundary itself).
LATTICE = [
    (1, 0, 3, 1, 1, 0, 1, False),                # an empty catalogue
    (1, 1, 1, 1, 1, 0, 1, True),                 # one item, one user, one slot, d = 1
    (31, 63, 8, 10, 32, 50, 63, True),           # a ragged user tile, less than one wave step
    (33, 65, 301, 128, 1, 70, 64, False),        # about 32 x 64 slots in one slice: the staged list nearly full; global excludes
    (33, 65, 8, 129, 8, 0, 65, True),            # about 32 x 65 slots in one slice: at the list's capacity, either path
    (65, 5000, 300, 10, 32, 50, 64, True),       # three slices, three user tiles, the VEC chain, staged
    (65, 5000, 301, 256, 8, 70, 256, False),     # the two-wave block (1024 slots fit): every slice overflows; the longest lists
    (33, 5000, 8, 129, 1, 0, 16, True),          # P = 256, a few slots per user
    (65, 5000, 1, 128, 8, 50, 0, True),          # E = 0: the biased call
    (1, 5000, 300, 256, 32, 50, 65, False),      # one user, the two-wave block, staged
    (31, 5000, 8, 1, 8, 70, 256, True),          # P = 128: full slices overflow, the short last slice is staged
]


@pytest.mark.parametrize("B,N,d,k,T,n_ex,E,with_bias", LATTICE)
def test_exact_on_lattice_data(B, N, d, k, T, n_ex, E, with_bias):
    user, items, s, bias, aid, adl, ex, tg = _lattice(B, N, d, k, T, n_ex, E, with_bias)
    want = ref.topk(s, bias, aid, adl, ex, k)
    if N >= 63 and E >= 16:          # on the CPU-side data: the test cannot pass by ignoring the slots
        plain = ref.topk(s, bias, None, None, ex, k)
        assert sum(not np.array_equal(_bits(want[1][b]), _bits(plain[1][b])) for b in range(B)) >= (B + 1) // 2
    _same(_topk(user, items, k, ex, bias, aid, adl), want, "adjusted top-k")
    got = _rank(user, items, tg, ex, bias, aid, adl)
    _same(got, ref.ranks(s, bias, aid, adl, ex, tg), "adjusted rank")
    if T >= 8 and N >= 63 and E >= 8:
        assert (got[0][:, 3] == 0).all() and (got[0][:, 5] == 0).all() and (got[1][:, 3] == -np.inf).all()
        assert (got[0][:, 4] == 0).sum() >= B // 2          # a NaN delta: rank 0 (unless a lower slot names the id too)
        if ex is not None:
            assert (got[0][:, 1] == 0).all()                                           # excluded and adjusted: excluded


def _small(B=33, N=5000, d=8, seed=5):
    rng = np.random.default_rng(seed)
    user = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    user[user == 0] = 1.0
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)
    return user, items, s


def _check(user, items, s, aid, adl, k, ex=None, bias=None, tg=None, what=""):
    got = _topk(user, items, k, ex, bias, aid, adl)
    _same(got, ref.topk(s, bias, aid, adl, ex, k), what + " top-k")
    if tg is None:
        tg = np.where(got[0] >= 0, got[0], 0)[:, :32]
    r = _rank(user, items, tg, ex, bias, aid, adl)
    _same(r, ref.ranks(s, bias, aid, adl, ex, tg), what + " rank")
    return got, r


def test_slot_edges():
    """Empty slots at -1, N and INT64_MAX change nothing; of two slots of one id the lower counts, in either order; an id both
    excluded and adjusted is excluded; slots on the first and last row of every slice and of a wave's 64 items."""
    user, items, s = _small()
    B, N = user.shape[0], items.shape[0]
    k = 10
    plain = ref.topk(s, None, None, None, None, k)
    empty = np.tile(np.array([[-1, N, I64_MAX, -2 ** 63]], dtype=np.int64), (B, 1))
    big = np.full((B, 4), 1000.0, dtype=np.float32)
    _same(_topk(user, items, k, None, None, empty, big), plain, "empty slots")
    # the same id twice
    n0 = 4500
    for first, second in ((100.0, -100.0), (-100.0, 100.0)):
        aid = np.tile(np.array([[-1, n0, N, n0]], dtype=np.int64), (B, 1))
        adl = np.tile(np.array([[7.0, first, 7.0, second]], dtype=np.float32), (B, 1))
        got, _ = _check(user, items, s, aid, adl, k, what="two slots of one id")
        assert ((got[0][:, 0] == n0).all()) == (first > 0) and (got[0] == n0).any() == (first > 0)
    # excluded and adjusted
    aid = np.full((B, 1), n0, dtype=np.int64)
    adl = np.full((B, 1), 1000.0, dtype=np.float32)
    ex = np.full((B, 1), n0, dtype=np.int64)
    got, r = _check(user, items, s, aid, adl, k, ex=ex, tg=np.full((B, 1), n0, dtype=np.int64), what="excluded and adjusted")
    assert not (got[0] == n0).any() and (r[0] == 0).all()
    # the borders of the slices (2048 rows) and of a wave's 64 items, boosted into the list and named as targets
    rows = np.array([0, 63, 64, 127, 511, 512, 2047, 2048, 4095, 4096, N - 1], dtype=np.int64)
    aid = np.tile(rows, (B, 1))
    adl = np.tile((500.0 + np.arange(len(rows))).astype(np.float32), (B, 1))
    got, r = _check(user, items, s, aid, adl, 16, tg=aid, what="slice and wave borders")
    assert (np.sort(got[0][:, :len(rows)], axis=1) == rows).all() and (np.sort(r[0], axis=1) == np.arange(1, len(rows) + 1)).all()


def test_block_sharing_patterns():
    """All 32 users of a block adjust the same item; one user adjusts what the other 31 leave alone; and enough slots in one slice
    to overflow the staged list (32 x 256 > 2048) while another slice of the same call stays staged."""
    user, items, s = _small(B=32)
    B, N = 32, items.shape[0]
    aid = np.full((B, 1), 3000, dtype=np.int64)
    adl = (np.arange(B, dtype=np.float32)[:, None] - 10.0) * 8.0           # a different delta per user, both signs
    _check(user, items, s, aid, adl, 10, tg=aid, what="one item, 32 users")
    aid = np.full((B, 2), -1, dtype=np.int64)
    adl = np.zeros((B, 2), dtype=np.float32)
    aid[13] = (4999, 17)
    adl[13] = (999.0, -999.0)
    got, _ = _check(user, items, s, aid, adl, 10, what="one user of 32")
    plain = ref.topk(s, None, None, None, None, 10)
    assert got[0][13, 0] == 4999 and all(np.array_equal(got[0][b], plain[0][b]) for b in range(B) if b != 13)
    rng = np.random.default_rng(9)
    aid = rng.integers(0, 2048, size=(B, 256)).astype(np.int64)            # every slot in slice 0 ...
    aid[:, :3] = (4100, 4200, 2500)                                         # ... but three, in the slices that stay staged
    adl = (rng.integers(-200, 201, size=(B, 256)) * 0.25).astype(np.float32)
    for k in (10, 129, 256):
        _check(user, items, s, aid, adl, k, what="overflowing slice, k=%d" % k)


@pytest.mark.parametrize("k,per_user", [(10, 64), (129, 64), (256, 32)])
def test_staged_list_capacity_boundary(k, per_user):
    """Exactly as many valid slots in one slice as the block's LDS list holds (32 x 64 = 2048 at P = 128 and P = 256, 32 x 32 = 1024
    at P = 512: staged), then exactly one more (user 0 alone has one more slot in that slice: the block walks the global lists).
    Every slot of slice 0 names a distinct row of its user, none is empty, so the counts are what the comment says."""
    user, items, s = _small(B=32)
    B = 32
    rng = np.random.default_rng(1000 + k)
    rows = np.stack([rng.permutation(2048)[:per_user + 1] for _ in range(B)]).astype(np.int64)       # slice 0 is rows [0, 2048)
    delta = (rng.integers(-200, 201, size=(B, per_user + 1)) * 0.25).astype(np.float32)
    delta[:, 0] = 300.0                                                    # every user's first slot is served first
    for extra in (False, True):
        aid = rows.copy()
        aid[:, per_user] = 2048 + np.arange(B)                             # the last slot: in slice 1 ...
        if extra:
            aid[0, per_user] = rows[0, per_user]                           # ... but user 0's, the one slot too many in slice 0
        assert int(((aid >= 0) & (aid < 2048)).sum()) == B * per_user + int(extra)
        got, _ = _check(user, items, s, aid, delta, k, tg=aid[:, :32], what="%d slots in slice 0, k=%d" % (B * per_user + int(extra), k))
        assert (got[0][:, 0] == aid[:, 0]).all()


def test_delta_values():
    """Negative, positive, +0.0, +inf, -inf and NaN deltas; a boost on the catalogue's minimum in the LAST slice served first at
    k = 1 (an add that sat in the flush would never see it: the score lies below every threshold); a penalty on the raw top-1; a
    penalty that takes a news out of the top k after its user's buffer was flushed (P = 128: the first 128 offers fill it)."""
    user, items, s = _small()
    items = items.copy()
    B, N = user.shape[0], items.shape[0]
    for b in range(B):
        items[4096 + 7 * b] = -3.0 * np.sign(user[b])                      # user b's minimum over the catalogue, in the last slice
    s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)
    low = 4096 + 7 * np.arange(B, dtype=np.int64)
    assert all(s[b, low[b]] == s[b].min() for b in range(B))
    got, r = _check(user, items, s, low[:, None], np.full((B, 1), 1000.0, dtype=np.float32), 1, tg=low[:, None], what="boosted minimum")
    assert (got[0][:, 0] == low).all() and (r[0] == 1).all()
    plain = ref.topk(s, None, None, None, None, 10)
    top1 = plain[0][:, :1]
    got, r = _check(user, items, s, top1, np.full((B, 1), -500.0, dtype=np.float32), 10, tg=top1, what="penalised top-1")
    assert not (got[0] == top1).any() and (r[0] > 10).all()
    late = np.array([[n for n in plain[0][b] if n >= 1024][-1] for b in range(B)], dtype=np.int64)[:, None]     # met after a flush
    got, _ = _check(user, items, s, late, np.full((B, 1), -500.0, dtype=np.float32), 10, what="penalty after a flush")
    assert not (got[0] == late).any()
    vals = np.array([-2.5, 2.5, 0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    aid = np.tile(np.array([[10, 2100, 4100, 4500, 20, 2200]], dtype=np.int64), (B, 1))
    adl = np.tile(vals, (B, 1))
    got, r = _check(user, items, s, aid, adl, N if N <= 256 else 256, tg=aid, what="special deltas")
    assert (got[0][:, 0] == 4500).all() and (got[1][:, 0] == np.inf).all()
    assert (r[0][:, 3] == 1).all() and (r[0][:, 5] == 0).all() and (r[1][:, 4] == -np.inf).all() and (r[0][:, 4] == N - 1).all()
    assert (r[1][:, 2] == s[:, 4100]).all()                                # + 0.0 leaves the score where it was


# ---- Gaussian data: the consequences of the header ---------------------------------------------------------------------------
N_REAL, B_REAL, E_REAL = 5000, 65, 48


@functools.lru_cache(maxsize=1)
def _real():
    """B = 65, N = 5 000, d = 300 Gaussian data with two NaN item rows (NaN scores for everybody) and duplicated item rows (equal
    scores: the id rule decides), a bias with NaN and -inf entries, 48 slots per user with duplicates, empty slots and special
    deltas."""
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
    aid, adl = _slots(B, N, E_REAL, rng, amp=40)
    adl = (adl.astype(np.float64) * 1.0009765625).astype(np.float32)       # not lattice values any more
    aid[:, 5] = np.array([100, 2000, 77, 105, 2005])[np.arange(B) % 5]      # the duplicated rows and a NaN row
    tg[:, 0] = torch.from_numpy(aid[:, 7]).to(DEV)
    return user, items.contiguous(), ex, bias, tg, _t(aid, torch.int64), _t(adl, torch.float32)


@pytest.mark.parametrize("with_bias", [False, True])
def test_no_adjustment_is_the_unadjusted_call(with_bias):
    """(a): E = 0, NULL lists and all-empty slots."""
    user, items, ex, bias, tg, aid, adl = _real()
    eng = _engine()
    b = bias if with_bias else None
    none_i = torch.empty(B_REAL, 0, dtype=torch.int64, device=DEV)
    none_d = torch.empty(B_REAL, 0, dtype=torch.float32, device=DEV)
    empty_i = torch.full_like(aid, -1)
    empty_i[:, 1::2] = N_REAL
    for k in (10, 100, 256):
        want = eng.top_k(user, items, k, ex, bias=b)
        _same(eng.top_k_adjusted(user, items, k, none_i, none_d, ex, bias=b), want, "(a) E = 0, k=%d" % k)
        _same(eng.top_k_adjusted(user, items, k, empty_i, adl, ex, bias=b), want, "(a) empty slots, k=%d" % k)
        _same(tuple(reversed(_raw_topk(user, items, b, None, None, 48, ex, k))), want, "(a) NULL lists, k=%d" % k)
    want = eng.rank_of(user, items, tg, ex, bias=b)
    _same(eng.rank_of_adjusted(user, items, tg, none_i, none_d, ex, bias=b), want, "(a) ranks, E = 0")
    _same(eng.rank_of_adjusted(user, items, tg, empty_i, adl, ex, bias=b), want, "(a) ranks, empty slots")
    _same(_raw_rank(user, items, b, None, None, 48, tg, ex), want, "(a) ranks, NULL lists")


def test_row_equals_the_biased_call_with_the_deltas_scattered():
    """(b), bias == NULL, for ten users, the ragged last tile's among them."""
    user, items, ex, bias, tg, aid, adl = _real()
    eng = _engine()
    k = 100
    sc, ids = eng.top_k_adjusted(user, items, k, aid, adl, ex)
    r, rs = eng.rank_of_adjusted(user, items, tg, aid, adl, ex)
    an, dn = aid.cpu().numpy(), adl.cpu().numpy()
    for u in list(range(8)) + [37, 64]:
        b1 = _t(ref.adjust_as_bias(an[u], dn[u], N_REAL), torch.float32)
        one = slice(u, u + 1)
        _same((sc[one], ids[one]), eng.top_k(user[one].contiguous(), items, k, ex[one].contiguous(), bias=b1), "(b) user %d" % u)
        _same((r[one], rs[one]), eng.rank_of(user[one].contiguous(), items, tg[one].contiguous(), ex[one].contiguous(), bias=b1),
              "(b) ranks %d" % u)
    assert not torch.equal(ids, eng.top_k(user, items, k, ex)[1])


def _raw_topk(user, items, bias, aid, adl, E, ex, k, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N = items.shape[0]
    need = int(lib.nrms_topk_dot_adjusted_workspace_bytes(B, C.c_int64(N), d, k))
    assert need == int(lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    sc = torch.empty(B, k, dtype=torch.float32, device=DEV)
    ids = torch.empty(B, k, dtype=torch.int64, device=DEV)
    rc = lib.nrms_topk_dot_adjusted(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), _lib.ptr(bias), _lib.ptr(aid),
                                    _lib.ptr(adl), E, _lib.ptr(ex), 0 if ex is None else ex.shape[1], _lib.ptr(sc), _lib.ptr(ids),
                                    _lib.ptr(ws), C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_topk_dot_adjusted")
    return ids, sc


def _raw_rank(user, items, bias, aid, adl, E, tg, ex, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N, T = items.shape[0], tg.shape[1]
    n_ex = 0 if ex is None else ex.shape[1]
    need = int(lib.nrms_rank_dot_adjusted_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    assert need == int(lib.nrms_rank_dot_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    r = torch.empty(B, T, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, T, dtype=torch.float32, device=DEV)
    rc = lib.nrms_rank_dot_adjusted(B, C.c_int64(N), d, T, _lib.ptr(user), _lib.ptr(items), _lib.ptr(bias), _lib.ptr(aid),
                                    _lib.ptr(adl), E, _lib.ptr(tg), _lib.ptr(ex), n_ex, _lib.ptr(r), _lib.ptr(sc), _lib.ptr(ws),
                                    C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_rank_dot_adjusted")
    return r, sc


def test_row_depends_on_its_own_user_and_slots_only():
    """(c) and (f): two runs, batch splits, the user's position, the neighbours' slots, a poisoned workspace."""
    user, items, ex, bias, tg, aid, adl = _real()
    eng = _engine()
    k = 100
    sc, ids = eng.top_k_adjusted(user, items, k, aid, adl, ex, bias=bias)
    r, rs = eng.rank_of_adjusted(user, items, tg, aid, adl, ex, bias=bias)
    _same(eng.top_k_adjusted(user, items, k, aid, adl, ex, bias=bias), (sc, ids), "second run")
    _same(eng.rank_of_adjusted(user, items, tg, aid, adl, ex, bias=bias), (r, rs), "second run")
    parts = [slice(0, 1), slice(1, 33), slice(33, 65)]
    cut = lambda a, p: a[p].contiguous()
    pkk = [eng.top_k_adjusted(cut(user, p), items, k, cut(aid, p), cut(adl, p), cut(ex, p), bias=bias) for p in parts]
    prr = [eng.rank_of_adjusted(cut(user, p), items, cut(tg, p), cut(aid, p), cut(adl, p), cut(ex, p), bias=bias) for p in parts]
    _same((torch.cat([x[0] for x in pkk]), torch.cat([x[1] for x in pkk])), (sc, ids), "batch split")
    _same((torch.cat([x[0] for x in prr]), torch.cat([x[1] for x in prr])), (r, rs), "batch split")
    perm = torch.randperm(B_REAL, generator=torch.Generator().manual_seed(3)).to(DEV)
    up = lambda a: a[perm].contiguous()
    _same(eng.top_k_adjusted(up(user), items, k, up(aid), up(adl), up(ex), bias=bias), (sc[perm], ids[perm]), "user permutation")
    _same(eng.rank_of_adjusted(up(user), items, up(tg), up(aid), up(adl), up(ex), bias=bias), (r[perm], rs[perm]), "user permutation")
    # user 5 in the middle of 31 copies of user 40 whose slots are empty, then user 5's own negated: its row may not move
    u = 5
    rows = torch.full((32,), 40, dtype=torch.int64, device=DEV)
    rows[13] = u
    for other in ("empty", "negated"):
        a2, d2 = aid[rows].contiguous(), adl[rows].contiguous()
        if other == "empty":
            a2[:] = -1
        else:
            a2[:] = aid[u]
            d2[:] = -adl[u]
        a2[13], d2[13] = aid[u], adl[u]
        s2, i2 = eng.top_k_adjusted(user[rows].contiguous(), items, k, a2, d2, ex[rows].contiguous(), bias=bias)
        r2, rs2 = eng.rank_of_adjusted(user[rows].contiguous(), items, tg[rows].contiguous(), a2, d2, ex[rows].contiguous(), bias=bias)
        _same((s2[13:14], i2[13:14]), (sc[u:u + 1], ids[u:u + 1]), "neighbours' slots %s" % other)
        _same((r2[13:14], rs2[13:14]), (r[u:u + 1], rs[u:u + 1]), "neighbours' slots %s" % other)
    for fill in (0xFF, 0x00, 0x7F):
        _same(_raw_topk(user, items, bias, aid, adl, E_REAL, ex, k, fill), (ids, sc), "workspace 0x%02X" % fill)
        _same(_raw_rank(user, items, bias, aid, adl, E_REAL, tg, ex, fill), (r, rs), "workspace 0x%02X" % fill)


def test_prefix_and_served_list_ranks():
    """(d) the first k' columns of a call with k are the call with k'; (e) the served ids rank 1, 2, ... with the same score bits."""
    user, items, ex, bias, tg, aid, adl = _real()
    eng = _engine()
    sc, ids = eng.top_k_adjusted(user, items, 256, aid, adl, ex, bias=bias)
    for k in (1, 65, 193):
        _same(eng.top_k_adjusted(user, items, k, aid, adl, ex, bias=bias), (sc[:, :k], ids[:, :k]), "(d) k'=%d" % k)
    r, rs = eng.rank_of_adjusted(user, items, ids, aid, adl, ex, bias=bias)
    want = torch.arange(1, 257, dtype=torch.int32, device=DEV).expand(B_REAL, 256)
    assert (ids >= 0).all() and torch.equal(r, want)
    _same((rs,), (sc,), "(e) scores of the served list")


# ---- the buffer contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2, 4, 6])
def test_buffer_contract(case):
    """Outputs and the workspace at the queried size between guard bands, the workspace poisoned three ways; bias, adj_ids and
    adj_delta are guarded too, at exactly their sizes."""
    from tests.guarded import POISONS, Pool
    from tests.test_hip_buffer_contracts import dev, ok, refuses_undersized, three_poisons
    lib = _lib.load()
    B, N, d, k, T, n_ex, E, with_bias = LATTICE[case]
    user, items, s, bias, aid, adl, ex, tg = _lattice(*LATTICE[case])
    ud, itd, tgd, exd = dev(np.array(user)), dev(np.array(items)), dev(np.array(tg), torch.int64), dev(ex, torch.int64) if n_ex else None
    need_k = int(lib.nrms_topk_dot_adjusted_workspace_bytes(B, C.c_int64(N), d, k))
    need_r = int(lib.nrms_rank_dot_adjusted_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    assert need_k > 0 and need_r > 0
    ins = ("adj_ids", "adj_delta") + (("bias",) if with_bias else ())

    def run(poison):
        P = Pool(poison)
        if with_bias:
            P.elems("bias", N, torch.float32, init=torch.from_numpy(np.array(bias)))
        P.elems("adj_ids", B * E, torch.int64, init=torch.from_numpy(np.array(aid)).reshape(-1))
        P.elems("adj_delta", B * E, torch.float32, init=torch.from_numpy(np.array(adl)).reshape(-1))
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, torch.int64), P.new("ws_topk", need_k)
        P.elems("ranks", B * T, torch.int32), P.elems("target_scores", B * T), P.new("ws_rank", need_r)
        bp = P["bias"].ptr if with_bias else None

        def call_k(nbytes):
            return lib.nrms_topk_dot_adjusted(B, C.c_int64(N), d, k, _lib.ptr(ud), _lib.ptr(itd), bp, P["adj_ids"].ptr,
                                              P["adj_delta"].ptr, E, _lib.ptr(exd), n_ex, P["top_scores"].ptr, P["top_ids"].ptr,
                                              P["ws_topk"].ptr, C.c_size_t(nbytes), _stream())

        def call_r(nbytes):
            return lib.nrms_rank_dot_adjusted(B, C.c_int64(N), d, T, _lib.ptr(ud), _lib.ptr(itd), bp, P["adj_ids"].ptr,
                                              P["adj_delta"].ptr, E, _lib.ptr(tgd), _lib.ptr(exd), n_ex, P["ranks"].ptr,
                                              P["target_scores"].ptr, P["ws_rank"].ptr, C.c_size_t(nbytes), _stream())

        snap = [P[n].snapshot() for n in ins]
        ok(call_k(need_k), "nrms_topk_dot_adjusted")
        P.intact("nrms_topk_dot_adjusted")
        ok(call_r(need_r), "nrms_rank_dot_adjusted")
        P.intact("nrms_rank_dot_adjusted")
        assert all(P[n].unchanged_since(sn) for n, sn in zip(ins, snap))
        if poison == POISONS[0]:
            keep = {n: P[n].numpy() for n in ("top_scores", "top_ids", "ranks", "target_scores")}
            refuses_undersized(call_k, P, need_k, "nrms_topk_dot_adjusted")
            refuses_undersized(call_r, P, need_r, "nrms_rank_dot_adjusted")
            assert all(np.array_equal(_bits(keep[n]), _bits(P[n].numpy())) for n in keep)
        return {"ids": P["top_ids"].numpy((B, k)), "scores": P["top_scores"].numpy((B, k)), "ranks": P["ranks"].numpy((B, T)),
                "tscores": P["target_scores"].numpy((B, T))}

    out = three_poisons(run, "the adjusted calls")[POISONS[0]]
    _same((out["ids"], out["scores"]), ref.topk(s, bias, aid, adl, ex, k), "adjusted top-k between guard bands")
    _same((out["ranks"], out["tscores"]), ref.ranks(s, bias, aid, adl, ex, tg), "adjusted rank between guard bands")


# ---- argument errors: refused on the host, before any launch; only the return codes and messages are read ---------------------
def test_argument_errors():
    lib = _lib.load()
    user, items, ex, bias, tg, aid, adl = _real()
    B, N, d, k, T = B_REAL, N_REAL, 300, 10, 8
    ws = torch.empty(1 << 20, dtype=torch.int64, device=DEV)
    sc = torch.full((B, k), 5.0, device=DEV)
    ids = torch.full((B, k), 5, dtype=torch.int64, device=DEV)
    r = torch.full((B, T), 5, dtype=torch.int32, device=DEV)
    rs = torch.full((B, T), 5.0, device=DEV)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)

    def topk(B=B, N=N, d=d, k=k, bias=_lib.ptr(bias), aid=_lib.ptr(aid), adl=_lib.ptr(adl), E=E_REAL, n_ex=0, nbytes=ws.numel() * 8):
        return lib.nrms_topk_dot_adjusted(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), bias, aid, adl, E, None, n_ex,
                                          _lib.ptr(sc), _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(nbytes), _stream())

    def rank(B=B, N=N, d=d, T=T, bias=_lib.ptr(bias), aid=_lib.ptr(aid), adl=_lib.ptr(adl), E=E_REAL, n_ex=0, nbytes=ws.numel() * 8):
        return lib.nrms_rank_dot_adjusted(B, C.c_int64(N), d, T, _lib.ptr(user), _lib.ptr(items), bias, aid, adl, E, _lib.ptr(tg),
                                          None, n_ex, _lib.ptr(r), _lib.ptr(rs), _lib.ptr(ws), C.c_size_t(nbytes), _stream())

    for call, who, size in ((topk, b"topk_dot_adjusted: ", "k"), (rank, b"rank_dot_adjusted: ", "T")):
        for kw, word in ((dict(aid=None), b"adj_ids is null"), (dict(adl=None), b"adj_delta is null"),
                         (dict(aid=off(aid, 4)), b"adj_ids must be 8-byte aligned"), (dict(adl=off(adl, 2)), b"adj_delta must be 4-byte aligned"),
                         (dict(bias=off(bias, 2)), b"bias must be 4-byte aligned"), (dict(E=-1), b"n_adjust must be"),
                         (dict(E=257), b"n_adjust must be"), (dict(B=-1), b"B must be"),
                         (dict(N=-1), b"N must be"), (dict(d=0), b"d must be"), ({size: 0}, size.encode() + b" must be"),
                         ({size: 257}, size.encode() + b" must be"), (dict(n_ex=-1), b"n_exclude must be")):
            assert call(**kw) == _lib.NRMS_EINVAL, (who, kw)
            msg = lib.nrms_last_error()
            assert msg.startswith(who) and word in msg, msg
        assert call(nbytes=8) == _lib.NRMS_EWORKSPACE
        assert lib.nrms_last_error().startswith(who)
    torch.cuda.synchronize()
    assert (sc == 5.0).all() and (ids == 5).all() and (r == 5).all() and (rs == 5.0).all()        # nothing was launched
    assert lib.nrms_topk_dot_adjusted_workspace_bytes(B, C.c_int64(N), d, 257) == 0
    assert lib.nrms_rank_dot_adjusted_workspace_bytes(B, C.c_int64(N), d, 33, 0) == 0
    assert topk(B=0) == _lib.NRMS_OK and rank(B=0) == _lib.NRMS_OK                                  # B = 0 is a no-op


def test_engine_arguments():
    user, items, ex, bias, tg, aid, adl = _real()
    eng = _engine()
    wide = torch.randint(0, N_REAL, (B_REAL, 40), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    r, rs = eng.rank_of_adjusted(user, items, wide, aid, adl, ex)            # more than 32 targets: column chunks
    _same(eng.rank_of_adjusted(user, items, wide[:, 32:].contiguous(), aid, adl, ex), (r[:, 32:], rs[:, 32:]), "chunks")
    empty = torch.empty(0, 300, device=DEV)
    sc, ids = eng.top_k_adjusted(user, empty, 10, aid, adl, None)                # N = 0: padding and rank 0
    r, rs = eng.rank_of_adjusted(user, empty, tg, aid, adl, None)
    assert (ids == -1).all() and (sc == -float("inf")).all() and (r == 0).all() and (rs == -float("inf")).all()
    for bad in (dict(adj_ids=aid[:-1].contiguous()), dict(adj_ids=aid.int()), dict(adj_ids=aid.cpu()), dict(adj_delta=adl[:, :-1].contiguous()),
                dict(adj_delta=adl.double()), dict(adj_ids=aid.repeat(1, 6), adj_delta=adl.repeat(1, 6))):
        kw = dict(adj_ids=aid, adj_delta=adl)
        kw.update(bad)
        with pytest.raises(_lib.NrmsError, match="adj_ids|adj_delta|n_adjust"):
            eng.top_k_adjusted(user, items, 10, kw["adj_ids"], kw["adj_delta"], ex)
        with pytest.raises(_lib.NrmsError, match="adj_ids|adj_delta|n_adjust"):
            eng.rank_of_adjusted(user, items, tg, kw["adj_ids"], kw["adj_delta"], ex)


# ---- the models --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_models_recommend_and_rank_adjusted(kind):
    """recommend_adjusted / rank_targets_adjusted agree with recommend_deep's full ranking (the catalogue has at most 4096 news, so
    the deep list is all of it) re-scored on the host: one fp32 add per named news, NaN sums dropped, sorted again."""
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model(kind)
    N = cat.shape[0]
    assert N <= 4096
    rng = np.random.default_rng(5)
    prior = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(DEV)
    E, k = 12, 20
    for batch in batches:
        B = torch.as_tensor(batch["browsed_ids"]).shape[0]
        news = rng.integers(1, N // 2, size=(B, E)).astype(np.int64)
        news[:, 0], news[:, 1] = 0, N + 5                                          # empty slots: id 0 and one beyond the catalogue
        news[:, 3] = news[:, 2]                                                    # named twice: the first delta counts
        news[:, 4] = rng.integers(N // 2, N, size=B)                               # (named by no other slot of its row)
        delta = rng.normal(size=(B, E)).astype(np.float32) * 3.0
        delta[:, 4] = np.nan                                                       # blocked for this user
        delta[:, 5] = 50.0                                                         # a boost from anywhere to the top
        adjust = (torch.from_numpy(news).to(DEV), torch.from_numpy(delta).to(DEV))
        for bias in (None, prior):
            full_ids, full_sc = model.recommend_deep(batch, N, cat, item_bias=bias)         # the whole ranking, then -1
            ids, sc = model.recommend_adjusted(batch, k, cat, adjust, item_bias=bias)
            fi, fs = full_ids.cpu().numpy(), full_sc.cpu().numpy()
            for b in range(B):
                live = fi[b] > 0
                n, s2 = fi[b][live], fs[b][live].copy()
                for e in range(E - 1, -1, -1):
                    hit = n == news[b, e]
                    s2[hit] = fs[b][live][hit] + delta[b, e]                       # float32 + float32
                keep = ~np.isnan(s2)
                n, s2 = n[keep], s2[keep]
                o = np.lexsort((n, -s2.astype(np.float64)))[:k]
                assert np.array_equal(ids[b].cpu().numpy(), n[o]) and np.array_equal(_bits(sc[b]), _bits(s2[o])), (kind, b)
                assert news[b, 4] not in ids[b].cpu().numpy()
            r, rs = model.rank_targets_adjusted(batch, ids, cat, adjust, item_bias=bias)
            want = torch.arange(1, k + 1, dtype=torch.int32, device=DEV).expand(B, k)
            assert torch.equal(r, want) and torch.equal(rs.view(torch.int32), sc.view(torch.int32))
            r, _ = model.rank_targets_adjusted(batch, adjust[0][:, 4:5], cat, adjust, item_bias=bias)
            assert (r == 0).all()
        none = (torch.zeros(B, 3, dtype=torch.int64, device=DEV), torch.ones(B, 3, device=DEV))
        a, b_ = model.recommend_adjusted(batch, k, cat, none), model.recommend(batch, k, cat)
        assert torch.equal(a[0], b_[0]) and torch.equal(a[1].view(torch.int32), b_[1].view(torch.int32))
        with pytest.raises(_lib.NrmsError, match="adjust"):
            model.recommend_adjusted(batch, 5, cat, (adjust[0][:-1], adjust[1]))
        with pytest.raises(_lib.NrmsError, match="adjust"):
            model.rank_targets_adjusted(batch, ids, cat, adjust[0])
    model.check_recommend_ids()


def test_run_v0_seen_discount_flag(tmp_path):
    """A fresh child process with a time limit of its own; nothing is started after it."""
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "pytorch_news_recommender_amd.run_v0", "--model", "nrms_hip", "--dataset", "synthetic",
                        "--negatives", "catalogue", "--max_batches", "2", "--epochs", "1", "--synthetic_users", "128",
                        "--batch_size", "64", "--num_workers", "0", "--description", "T", "--data_path", str(tmp_path / "data"),
                        "--save_path", str(tmp_path / "save"), "--recommend", "5", "--seen_discount", "0.5"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("recommend with seen news discounted")]
    assert len(line) == 1, r.stdout[-3000:]
    m = re.fullmatch(r"recommend with seen news discounted \(beta 0\.5, (\d+) slots\): (\d+) users, (\d+) of (\d+) slots filled, "
                     r"(\d+) seen news served", line[0])
    assert m, line[0]
    assert int(m.group(1)) > 0 and int(m.group(2)) > 0 and 0 < int(m.group(3)) <= int(m.group(4))
