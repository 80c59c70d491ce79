"""nrms_topk_dot_windowed / nrms_rank_dot_windowed on the GPU (a per-user time window on the catalogue in retrieval and exact
ranking, include/nrms_hip.h): exact against tests/topk_window_ref.py on integer lattice data at every point where the kernels
change path, the consequences (a) to (d) the header states on Gaussian data, determinism, the buffer contract, the argument
errors and the layers above (engine.top_k / rank_of, Model.recommend / rank_targets).  Every comparison is exact: ids, ranks and
score bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream

from tests import topk_window_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
I32_MIN, I32_MAX = ref.I32_MIN, ref.I32_MAX
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


def _topk(user, items, k, ex, bias, time, win):
    s, ids = _engine().top_k(_t(user, torch.float32), _t(items, torch.float32), k, _t(ex, torch.int64), bias=_t(bias, torch.float32),
                             item_time=_t(time, torch.int32), window=_t(win, torch.int32))
    return ids.cpu().numpy(), s.cpu().numpy()


def _rank(user, items, tg, ex, bias, time, win):
    r, s = _engine().rank_of(_t(user, torch.float32), _t(items, torch.float32), _t(tg, torch.int64), _t(ex, torch.int64),
                             bias=_t(bias, torch.float32), item_time=_t(time, torch.int32), window=_t(win, torch.int32))
    return r.cpu().numpy(), s.cpu().numpy()


# ---- the data ----------------------------------------------------------------------------------------------------------------
def _times(N, kind, rng):
    """sorted: distinct rising ticks from a negative start (whole waves and slices fall outside a narrow window), the last two
    items "not published"; shuffled: the same ticks in random row order; constant: one tick for everybody."""
    if kind == "constant":
        return np.full(N, 7, dtype=np.int64)
    t = 3 * np.arange(N, dtype=np.int64) - 1000
    if N >= 8:
        t[-2:] = I32_MAX
    return t if kind == "sorted" else rng.permutation(t)


def _windows(B, time, kind, k, rng):
    """mixed: row b takes window kind b % 10 of the list below; disjoint: pairwise disjoint intervals, each a B-th of the ticks,
    so the block's hull covers items that no single user accepts; full: [INT32_MIN, INT32_MAX) everywhere."""
    w = np.zeros((B, 2), dtype=np.int64)
    pub = np.sort(time[time < I32_MAX]) if len(time) else np.zeros(0, dtype=np.int64)
    if kind == "full" or len(pub) == 0:
        w[:] = (I32_MIN, I32_MAX)
        if kind != "full":
            w[1::2] = (5, 5)
        return w
    n = len(pub)
    at = lambda f: int(pub[min(n - 1, int(f * n))])
    if kind == "disjoint":
        edges = np.linspace(int(pub[0]), int(pub[-1]) + 1, B + 1).astype(np.int64)
        w[:, 0], w[:, 1] = edges[:-1], edges[1:]
        return w[rng.permutation(B)]
    for b in range(B):
        f = rng.random()
        w[b] = [(I32_MIN, I32_MAX),                         # 0 full
                (at(0.5), at(0.5)),                         # 1 empty, lo == hi
                (at(0.7), at(0.2)),                         # 2 inverted
                (at(f), at(f) + 1),                         # 3 one tick wide: exactly the items of that tick
                (int(pub[min(n - 1, n // 3 | 5)]), int(pub[min(n - 1, (2 * n) // 3 | 9)])),   # 4 lo == a time (inside), hi == a time
                                                            #   (outside); both cut a 32-item tile and a 64-item step of sorted rows
                (I32_MIN, at(0.4)),                         # 5 from the first tick there is
                (at(0.6), I32_MAX),                         # 6 to the last one: the INT32_MAX items stay out
                (at(f), at(f) + 3 * max(1, k // 2)),        # 7 about k / 2 ticks: fewer than k eligible, padding
                (I32_MAX - 1, I32_MAX),                     # 8 just below "not published": nothing
                (at(0.5 * f), at(0.5 + 0.5 * f))][b % 10]   # 9 a random interval
    return w


@functools.lru_cache(maxsize=None)
def _lattice(B, N, d, k, T, n_ex, tkind, wkind, with_bias):
    """Integer users and items in [-3, 3] (every dot product, and every sum with a multiple of 0.25 below 2^12, is exact in fp32
    whatever the order of summation; ties are abundant, so the id rule is exercised), a bias of multiples of 0.25 with NaN and
    -inf entries, exclude lists with -1, N and a duplicate, and targets that name an id outside the window, an excluded one, a
    duplicate, -1, a NaN-prior id and N."""
    rng = np.random.default_rng(100003 * d + 1009 * N + 17 * k + B + T + n_ex)
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
    time = _times(N, tkind, rng)
    win = _windows(B, time, wkind, k, rng)
    ex = None
    if n_ex:
        ex = rng.integers(0, max(N, 1), size=(B, n_ex)).astype(np.int64)
        ex[:, 0], ex[:, 1], ex[:, 2] = -1, N, ex[:, min(3, n_ex - 1)]
    tg = rng.integers(0, max(N, 1), size=(B, T)).astype(np.int64)
    for b in range(B):                                     # the first target lies inside its user's window, where there is one
        inside = np.nonzero((time >= win[b, 0]) & (time < win[b, 1]))[0]
        if len(inside):
            tg[b, 0] = inside[(7 * b) % len(inside)]
    if T >= 8 and N >= 63:
        for b in range(B):
            out = np.nonzero(~((time >= win[b, 0]) & (time < win[b, 1])))[0]
            tg[b, 1] = out[b % len(out)] if len(out) else 0
            tg[b, 2] = ex[b, min(4, n_ex - 1)] if ex is not None else tg[b, 0]
            tg[b, 3] = tg[b, 0]
            tg[b, 4] = -1
            tg[b, 5] = np.nonzero(np.isnan(bias))[0][0] if with_bias else N
            tg[b, 6] = N
    for a in (user, items, s, time, win, tg):
        a.setflags(write=False)
    return user, items, s, bias, time, win, ex, tg


# (B, N, d, k, T, n_exclude, times, windows, bias): every value of B {1, 31, 32, 33, 65}, N {0, 1, 63, 64, 65, 511, 512, 513,
# 2048, 2049, 4200}, d {1, 7, 32, 36, 300}, k {1, 64, 65, 192, 193, 256}, T {1, 8, 32}, n_exclude {0, 3, 64, 65}
LATTICE = [
    (1, 0, 7, 1, 1, 0, "sorted", "mixed", False),             # an empty catalogue
    (1, 1, 1, 1, 1, 0, "constant", "full", True),             # one item, one user, d = 1
    (31, 63, 7, 64, 8, 3, "sorted", "mixed", True),           # a ragged user tile, less than one wave step, the scalar path
    (32, 64, 32, 65, 8, 0, "shuffled", "mixed", False),       # exactly one tile of users and one wave step, the second buffer size
    (33, 65, 36, 1, 1, 3, "sorted", "disjoint", True),        # one padded user tile, a tail of one item, a remainder 8-group
    (65, 511, 36, 192, 32, 64, "sorted", "mixed", True),      # one item short of a block step; the LDS exclude path at its limit
    (33, 512, 300, 193, 8, 65, "sorted", "disjoint", False),  # the two-wave block from k = 193, the global exclude path
    (65, 513, 7, 256, 32, 3, "shuffled", "mixed", True),      # one item past a block step, the largest k
    (32, 2048, 32, 64, 8, 65, "sorted", "disjoint", True),    # the shortest slice, whole waves dead inside a live block
    (33, 2049, 1, 65, 1, 0, "sorted", "mixed", False),        # two slices; d = 1: ties everywhere
    (65, 4200, 300, 256, 8, 64, "sorted", "mixed", True),     # three slices, three user tiles, whole slices dead
    (31, 4200, 36, 192, 32, 3, "constant", "mixed", False),   # one tick for every item: in or out as a whole
    (1, 4200, 32, 193, 8, 65, "sorted", "mixed", True),       # one user (a full window) against several slices
    (65, 4200, 7, 1, 1, 0, "shuffled", "disjoint", False),    # the skip seldom fires
    (33, 2049, 300, 10, 8, 3, "sorted", "mixed", True),
]


@pytest.mark.parametrize("B,N,d,k,T,n_ex,tkind,wkind,with_bias", LATTICE)
def test_exact_on_lattice_data(B, N, d, k, T, n_ex, tkind, wkind, with_bias):
    user, items, s, bias, time, win, ex, tg = _lattice(B, N, d, k, T, n_ex, tkind, wkind, with_bias)
    want = ref.topk(s, bias, time, win, ex, k)
    if N >= 63 and wkind == "mixed" and B >= 31:        # on the CPU-side data: the test cannot pass by ignoring the window
        plain = ref.topk(s, bias, time, np.tile(ref.FULL, (B, 1)), ex, k)
        assert (want[0][1] == -1).all() and (want[0][2] == -1).all() and (want[0][8] == -1).all()       # empty, inverted, none
        assert (plain[0][1] >= 0).any() and sum(not np.array_equal(want[0][b], plain[0][b]) for b in range(B)) >= B // 3
        if tkind == "sorted":
            assert k == 1 or ((want[0][7] >= 0).any() and (want[0][7] == -1).any())                     # fewer than k: padding
    _same(_topk(user, items, k, ex, bias, time, win), want, "windowed top-k")
    got = _rank(user, items, tg, ex, bias, time, win)
    _same(got, ref.ranks(s, bias, time, win, ex, tg), "windowed rank")
    if T >= 8 and N >= 63:
        assert (got[0][:, 4] == 0).all() and (got[0][:, 6] == 0).all() and (got[1][:, 4] == -np.inf).all()
        outside = ~((time[tg[:, 1]] >= win[:, 0]) & (time[tg[:, 1]] < win[:, 1]))
        assert outside.any() and (got[0][outside, 1] == 0).all()                   # a target outside its user's window


def test_window_edges():
    """lo == time is inside and hi == time outside; INT32_MIN is an ordinary tick; a time of INT32_MAX is open to nobody, not even
    to [INT32_MIN, INT32_MAX); lo >= hi gives padding and rank 0."""
    N, d = 70, 8
    rng = np.random.default_rng(7)
    user = rng.integers(-3, 4, size=(6, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)
    time = np.arange(N, dtype=np.int64) * 10
    time[0], time[1], time[69] = I32_MIN, I32_MIN + 1, I32_MAX
    win = np.array([[100, 200], [I32_MIN, I32_MIN + 1], [I32_MIN, I32_MAX], [I32_MAX, I32_MAX], [I32_MAX, I32_MIN], [I32_MAX - 1, I32_MAX]])
    ids, sc = _topk(user, items, N, None, None, time, win)
    _same((ids, sc), ref.topk(s, None, time, win, None, N), "edges")
    assert sorted(ids[0][ids[0] >= 0].tolist()) == list(range(10, 20))             # 100 in, 200 out
    assert ids[1].tolist() == [0] + [-1] * (N - 1)
    assert 69 not in ids[2] and (ids[2] >= 0).sum() == N - 1
    assert (ids[3:] == -1).all() and (sc[3:] == -np.inf).all()
    tg = np.tile(np.array([[10, 20, 0, 69]]), (6, 1))
    r, rs = _rank(user, items, tg, None, None, time, win)
    _same((r, rs), ref.ranks(s, None, time, win, None, tg), "edges")
    assert r[0, 0] > 0 and r[0, 1] == 0 and r[1, 2] == 1 and (r[:, 3] == 0).all() and (r[3:] == 0).all()


# ---- Gaussian data: the consequences of the header ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _real():
    """B = 65, N = 4 200, d = 300 Gaussian data, sorted ticks with two unpublished items, mixed windows, a bias with NaN entries."""
    B, N, d = 65, 4200, 300
    g = torch.Generator(device=DEV).manual_seed(11)
    user = torch.randn(B, d, device=DEV, generator=g)
    items = torch.randn(N, d, device=DEV, generator=g)
    ex = torch.randint(0, N, (B, 50), device=DEV, generator=g)
    bias = (torch.randn(N, device=DEV, generator=g) * 6.0).contiguous()
    bias[torch.randint(0, N, (20,), device=DEV, generator=g)] = float("nan")
    tg = torch.randint(0, N, (B, 8), device=DEV, generator=g)
    rng = np.random.default_rng(3)
    time = _times(N, "sorted", rng)
    win = _windows(B, time, "mixed", 100, rng)
    return user, items, ex, bias, tg, _t(time, torch.int32), _t(win, torch.int32)


def _full(B):
    return torch.tensor([ref.FULL], dtype=torch.int64).expand(B, 2).to(torch.int32).to(DEV).contiguous()


@pytest.mark.parametrize("with_bias", [False, True])
def test_full_window_is_the_unwindowed_call(with_bias):
    """(a)"""
    user, items, ex, bias, tg, time, win = _real()
    eng = _engine()
    b = bias if with_bias else None
    t = torch.clamp(time, max=I32_MAX - 1)
    for k in (10, 100, 256):
        _same(eng.top_k(user, items, k, ex, bias=b, item_time=t, window=_full(65)), eng.top_k(user, items, k, ex, bias=b), "(a) k=%d" % k)
    _same(eng.rank_of(user, items, tg, ex, bias=b, item_time=t, window=_full(65)), eng.rank_of(user, items, tg, ex, bias=b), "(a) ranks")


@pytest.mark.parametrize("with_bias", [False, True])
def test_row_equals_the_biased_call_with_nan_outside(with_bias):
    """(b), for one user of every window kind and the ragged last tile's user."""
    user, items, ex, bias, tg, time, win = _real()
    eng = _engine()
    b = bias if with_bias else None
    k = 100
    sc, ids = eng.top_k(user, items, k, ex, bias=b, item_time=time, window=win)
    r, rs = eng.rank_of(user, items, tg, ex, bias=b, item_time=time, window=win)
    tn, wn = time.cpu().numpy(), win.cpu().numpy()
    bn = None if b is None else b.cpu().numpy()
    for u in list(range(10)) + [37, 64]:
        b1 = _t(ref.window_as_bias(bn, tn, wn[u], 4200), torch.float32)
        one = slice(u, u + 1)
        s1, i1 = eng.top_k(user[one].contiguous(), items, k, ex[one].contiguous(), bias=b1)
        _same((ids[one], sc[one]), (i1, s1), "(b) user %d" % u)
        _same((r[one], rs[one]), eng.rank_of(user[one].contiguous(), items, tg[one].contiguous(), ex[one].contiguous(), bias=b1), "(b) ranks %d" % u)
    assert (ids[0] >= 0).all() and (ids[1] == -1).all() and (ids[7] == -1).any() and (ids[7] >= 0).any()


@pytest.mark.parametrize("k", [10, 256])
def test_served_list_ranks_one_to_k(k):
    """(c)"""
    user, items, ex, bias, tg, time, win = _real()
    eng = _engine()
    sc, ids = eng.top_k(user, items, k, ex, bias=bias, item_time=time, window=win)
    r, rs = eng.rank_of(user, items, ids, ex, bias=bias, item_time=time, window=win)
    live = ids >= 0
    want = torch.arange(1, k + 1, dtype=torch.int32, device=DEV).expand(65, k)
    assert live.any() and torch.equal(r[live], want[live]) and (r[~live] == 0).all()
    _same((rs,), (sc,), "(c) scores of the served list")


def _raw_topk(user, items, bias, time, win, ex, k, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N = items.shape[0]
    need = int(lib.nrms_topk_dot_windowed_workspace_bytes(B, C.c_int64(N), d, k))
    assert need == int(lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    sc = torch.empty(B, k, dtype=torch.float32, device=DEV)
    ids = torch.empty(B, k, dtype=torch.int64, device=DEV)
    rc = lib.nrms_topk_dot_windowed(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), _lib.ptr(bias), _lib.ptr(time), _lib.ptr(win),
                                    _lib.ptr(ex), 0 if ex is None else ex.shape[1], _lib.ptr(sc), _lib.ptr(ids), _lib.ptr(ws),
                                    C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_topk_dot_windowed")
    return ids, sc


def _raw_rank(user, items, bias, time, win, tg, ex, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N, T = items.shape[0], tg.shape[1]
    n_ex = 0 if ex is None else ex.shape[1]
    need = int(lib.nrms_rank_dot_windowed_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    assert need == int(lib.nrms_rank_dot_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    r = torch.empty(B, T, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, T, dtype=torch.float32, device=DEV)
    rc = lib.nrms_rank_dot_windowed(B, C.c_int64(N), d, T, _lib.ptr(user), _lib.ptr(items), _lib.ptr(bias), _lib.ptr(time), _lib.ptr(win),
                                    _lib.ptr(tg), _lib.ptr(ex), n_ex, _lib.ptr(r), _lib.ptr(sc), _lib.ptr(ws), C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_rank_dot_windowed")
    return r, sc


def test_invariance_and_determinism():
    """(d): two runs, batch splits, the user's position, the row order of the catalogue, a poisoned workspace."""
    user, items, ex, bias, tg, time, win = _real()
    eng = _engine()
    k = 100
    kw = dict(bias=bias, item_time=time, window=win)
    sc, ids = eng.top_k(user, items, k, ex, **kw)
    r, rs = eng.rank_of(user, items, tg, ex, **kw)
    _same(eng.top_k(user, items, k, ex, **kw), (sc, ids), "second run")
    _same(eng.rank_of(user, items, tg, ex, **kw), (r, rs), "second run")
    parts = [slice(0, 1), slice(1, 33), slice(33, 65)]
    pk = [eng.top_k(user[p].contiguous(), items, k, ex[p].contiguous(), bias=bias, item_time=time, window=win[p].contiguous()) for p in parts]
    pr = [eng.rank_of(user[p].contiguous(), items, tg[p].contiguous(), ex[p].contiguous(), bias=bias, item_time=time,
                      window=win[p].contiguous()) for p in parts]
    _same((torch.cat([x[0] for x in pk]), torch.cat([x[1] for x in pk])), (sc, ids), "batch split")
    _same((torch.cat([x[0] for x in pr]), torch.cat([x[1] for x in pr])), (r, rs), "batch split")
    perm = torch.randperm(65, generator=torch.Generator().manual_seed(3)).to(DEV)
    up = lambda a: a[perm].contiguous()
    _same(eng.top_k(up(user), items, k, up(ex), bias=bias, item_time=time, window=up(win)), (sc[perm], ids[perm]), "user permutation")
    _same(eng.rank_of(up(user), items, up(tg), up(ex), bias=bias, item_time=time, window=up(win)), (r[perm], rs[perm]), "user permutation")
    # the catalogue's rows shuffled (items, bias and times together), ids mapped back: new row j holds old row rows[j]
    rows = torch.randperm(4200, generator=torch.Generator().manual_seed(4)).to(DEV)
    inv = torch.empty_like(rows)
    inv[rows] = torch.arange(4200, device=DEV)
    skw = dict(bias=bias[rows].contiguous(), item_time=time[rows].contiguous(), window=win)
    s2, i2 = eng.top_k(user, items[rows].contiguous(), k, inv[ex].contiguous(), **skw)
    back = torch.where(i2 >= 0, rows[i2.clamp(min=0)], i2)
    _same((s2, back), (sc, ids), "row-shuffled catalogue")            # Gaussian scores: no ties for the id rule to decide
    _same(eng.rank_of(user, items[rows].contiguous(), inv[tg].contiguous(), inv[ex].contiguous(), **skw), (r, rs), "row-shuffled catalogue")
    for fill in (0xFF, 0x00, 0x7F):
        _same(_raw_topk(user, items, bias, time, win, ex, k, fill), (ids, sc), "workspace 0x%02X" % fill)
        _same(_raw_rank(user, items, bias, time, win, tg, ex, fill), (r, rs), "workspace 0x%02X" % fill)


# ---- the buffer contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [2, 7, 10])
def test_buffer_contract(case):
    """Outputs and the workspace at the queried size between guard bands, the workspace poisoned three ways; bias, item_time and
    window are guarded too, at exactly their sizes."""
    from tests.guarded import POISONS, Pool
    from tests.test_hip_buffer_contracts import dev, ok, refuses_undersized, three_poisons
    lib = _lib.load()
    B, N, d, k, T, n_ex, tkind, wkind, with_bias = LATTICE[case]
    user, items, s, bias, time, win, ex, tg = _lattice(*LATTICE[case])
    ud, itd, tgd, exd = dev(np.array(user)), dev(np.array(items)), dev(np.array(tg), torch.int64), dev(ex, torch.int64)
    need_k = int(lib.nrms_topk_dot_windowed_workspace_bytes(B, C.c_int64(N), d, k))
    need_r = int(lib.nrms_rank_dot_windowed_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    assert need_k > 0 and need_r > 0

    def run(poison):
        P = Pool(poison)
        P.elems("bias", N, torch.float32, init=torch.from_numpy(np.array(bias)))
        P.elems("time", N, torch.int32, init=torch.from_numpy(np.array(time)).to(torch.int32))
        P.elems("window", 2 * B, torch.int32, init=torch.from_numpy(np.array(win)).to(torch.int32).reshape(-1))
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, torch.int64), P.new("ws_topk", need_k)
        P.elems("ranks", B * T, torch.int32), P.elems("target_scores", B * T), P.new("ws_rank", need_r)

        def call_k(nbytes):
            return lib.nrms_topk_dot_windowed(B, C.c_int64(N), d, k, _lib.ptr(ud), _lib.ptr(itd), P["bias"].ptr, P["time"].ptr,
                                              P["window"].ptr, _lib.ptr(exd), n_ex, P["top_scores"].ptr, P["top_ids"].ptr,
                                              P["ws_topk"].ptr, C.c_size_t(nbytes), _stream())

        def call_r(nbytes):
            return lib.nrms_rank_dot_windowed(B, C.c_int64(N), d, T, _lib.ptr(ud), _lib.ptr(itd), P["bias"].ptr, P["time"].ptr,
                                              P["window"].ptr, _lib.ptr(tgd), _lib.ptr(exd), n_ex, P["ranks"].ptr,
                                              P["target_scores"].ptr, P["ws_rank"].ptr, C.c_size_t(nbytes), _stream())

        snap = [P[n].snapshot() for n in ("bias", "time", "window")]
        ok(call_k(need_k), "nrms_topk_dot_windowed")
        P.intact("nrms_topk_dot_windowed")
        ok(call_r(need_r), "nrms_rank_dot_windowed")
        P.intact("nrms_rank_dot_windowed")
        assert all(P[n].unchanged_since(sn) for n, sn in zip(("bias", "time", "window"), snap))
        if poison == POISONS[0]:
            keep = {n: P[n].numpy() for n in ("top_scores", "top_ids", "ranks", "target_scores")}
            refuses_undersized(call_k, P, need_k, "nrms_topk_dot_windowed")
            refuses_undersized(call_r, P, need_r, "nrms_rank_dot_windowed")
            assert all(np.array_equal(_bits(keep[n]), _bits(P[n].numpy())) for n in keep)
        return {"ids": P["top_ids"].numpy((B, k)), "scores": P["top_scores"].numpy((B, k)), "ranks": P["ranks"].numpy((B, T)),
                "tscores": P["target_scores"].numpy((B, T))}

    out = three_poisons(run, "the windowed calls")[POISONS[0]]
    _same((out["ids"], out["scores"]), ref.topk(s, bias, time, win, ex, k), "windowed top-k between guard bands")
    _same((out["ranks"], out["tscores"]), ref.ranks(s, bias, time, win, ex, tg), "windowed rank between guard bands")


# ---- argument errors: refused on the host, before any launch; only the return codes and messages are read ---------------------
def test_argument_errors():
    lib = _lib.load()
    user, items, ex, bias, tg, time, win = _real()
    B, N, d, k, T = 65, 4200, 300, 10, 8
    ws = torch.empty(1 << 20, dtype=torch.int64, device=DEV)
    sc = torch.full((B, k), 5.0, device=DEV)
    ids = torch.full((B, k), 5, dtype=torch.int64, device=DEV)
    r = torch.full((B, T), 5, dtype=torch.int32, device=DEV)
    rs = torch.full((B, T), 5.0, device=DEV)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)

    def topk(B=B, N=N, d=d, k=k, bias=_lib.ptr(bias), time=_lib.ptr(time), win=_lib.ptr(win), n_ex=0):
        return lib.nrms_topk_dot_windowed(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), bias, time, win, None, n_ex,
                                          _lib.ptr(sc), _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())

    def rank(B=B, N=N, d=d, T=T, bias=_lib.ptr(bias), time=_lib.ptr(time), win=_lib.ptr(win), n_ex=0):
        return lib.nrms_rank_dot_windowed(B, C.c_int64(N), d, T, _lib.ptr(user), _lib.ptr(items), bias, time, win, _lib.ptr(tg), None,
                                          n_ex, _lib.ptr(r), _lib.ptr(rs), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())

    for call, who, size in ((topk, b"topk_dot_windowed: ", "k"), (rank, b"rank_dot_windowed: ", "T")):
        for kw, word in ((dict(time=None), b"item_time is null"), (dict(win=None), b"window is null"),
                         (dict(time=off(time, 2)), b"item_time must be 4-byte aligned"), (dict(win=off(win, 1)), b"window must be 4-byte aligned"),
                         (dict(bias=off(bias, 2)), b"bias must be 4-byte aligned"), (dict(B=-1), b"B must be"), (dict(N=-1), b"N must be"),
                         (dict(d=0), b"d must be"), ({size: 0}, size.encode() + b" must be"), ({size: 257}, size.encode() + b" must be"),
                         (dict(n_ex=-1), b"n_exclude must be")):
            assert call(**kw) == _lib.NRMS_EINVAL, (who, kw)
            msg = lib.nrms_last_error()
            assert msg.startswith(who) and word in msg, msg
    torch.cuda.synchronize()
    assert (sc == 5.0).all() and (ids == 5).all() and (r == 5).all() and (rs == 5.0).all()        # nothing was launched
    assert lib.nrms_topk_dot_windowed_workspace_bytes(B, C.c_int64(N), d, 257) == 0
    assert lib.nrms_rank_dot_windowed_workspace_bytes(B, C.c_int64(N), d, 33, 0) == 0
    assert topk(B=0) == _lib.NRMS_OK and rank(B=0) == _lib.NRMS_OK                                  # B = 0 is a no-op


def test_engine_keywords():
    user, items, ex, bias, tg, time, win = _real()
    eng = _engine()
    for kw in (dict(item_time=time), dict(window=win)):                           # both or neither
        with pytest.raises(_lib.NrmsError, match="window"):
            eng.top_k(user, items, 10, ex, **kw)
        with pytest.raises(_lib.NrmsError, match="window"):
            eng.rank_of(user, items, tg, ex, **kw)
    a = eng.top_k(user, items, 10, ex, item_time=time, window=win)
    _same(eng.top_k(user, items, 10, ex, item_time=time.long(), window=win.long()), a, "int64 input that fits")
    big = win.long().clone()
    big[0, 1] = 2 ** 31
    with pytest.raises(_lib.NrmsError, match="window"):
        eng.top_k(user, items, 10, ex, item_time=time, window=big)
    far = time.long().clone()
    far[5] = -2 ** 31 - 1
    with pytest.raises(_lib.NrmsError, match="item_time"):
        eng.rank_of(user, items, tg, ex, item_time=far, window=win)
    for bad in (dict(item_time=time[:-1].contiguous(), window=win), dict(item_time=time.float(), window=win),
                dict(item_time=time, window=win[:-1].contiguous()), dict(item_time=time.cpu(), window=win)):
        with pytest.raises(_lib.NrmsError, match="item_time|window"):
            eng.top_k(user, items, 10, ex, **bad)
    # the default call makes exactly the calls it made: the unwindowed entry points, bit for bit
    _same(eng.top_k(user, items, 10, ex, item_time=None, window=None), eng.top_k(user, items, 10, ex), "defaults")
    lib = _lib.load()
    sc = torch.empty(65, 10, device=DEV)
    ids = torch.empty(65, 10, dtype=torch.int64, device=DEV)
    need = int(lib.nrms_topk_dot_workspace_bytes(65, C.c_int64(4200), 300, 10))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    _lib.check(lib.nrms_topk_dot(65, C.c_int64(4200), 300, 10, _lib.ptr(user), _lib.ptr(items), _lib.ptr(ex), 50, _lib.ptr(sc), _lib.ptr(ids),
                                 _lib.ptr(ws), C.c_size_t(need), _stream()), "nrms_topk_dot")
    _same(eng.top_k(user, items, 10, ex), (sc, ids), "the default call is nrms_topk_dot")


# ---- the models --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_models_recommend_and_rank_inside_a_window(kind):
    """recommend / rank_targets with item_time agree with recommend's full ranking filtered on the host."""
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model(kind)
    N = cat.shape[0]
    rng = np.random.default_rng(5)
    time = torch.from_numpy(rng.integers(0, 100, size=N)).to(DEV)                 # int64 by news id; entry 0 is never read
    time[0] = 50
    time[7] = I32_MAX                                                              # not published
    prior = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(DEV)
    for batch in batches:
        B = torch.as_tensor(batch["browsed_ids"]).shape[0]
        lo = torch.from_numpy(rng.integers(0, 80, size=B)).to(DEV)
        win = torch.stack([lo, lo + 30], dim=1)
        win[0] = torch.tensor([40, 40])                                            # an empty window
        if B > 1:
            win[1] = torch.tensor([I32_MIN, I32_MAX])
        for bias in (None, prior):
            # recommend's full ranking: its first 256 places, continued to the end by the exact ranks of all news
            top_ids, top_sc = model.recommend(batch, 256, cat, item_bias=bias)
            every = torch.arange(1, N, device=DEV).expand(B, -1).contiguous()
            r_all, s_all = model.rank_targets(batch, every, cat, item_bias=bias)
            place = torch.where(r_all > 0, r_all, torch.full_like(r_all, N + 1)).long()
            order = torch.argsort(place, dim=1)
            full_ids = torch.where(place.gather(1, order) <= N, every.gather(1, order), torch.full_like(every, -1))
            full_sc = s_all.gather(1, order)
            n_top = min(256, N - 1)
            assert torch.equal(full_ids[:, :n_top], top_ids[:, :n_top])
            assert torch.equal(full_sc[:, :n_top].view(torch.int32), top_sc[:, :n_top].view(torch.int32))
            k = 20
            ids, sc = model.recommend(batch, k, cat, item_bias=bias, item_time=time, window=win)
            for b in range(B):
                fi, fs = full_ids[b], full_sc[b]
                t = time[fi.clamp(min=0)]
                keep = (fi > 0) & (t >= win[b, 0]) & (t < win[b, 1])
                wi, wsc = fi[keep][:k], fs[keep][:k]
                n = wi.shape[0]
                assert torch.equal(ids[b, :n], wi) and torch.equal(sc[b, :n].view(torch.int32), wsc.view(torch.int32))
                assert (ids[b, n:] == -1).all() and (sc[b, n:] == -float("inf")).all()
            assert (ids[0] == -1).all() and not (ids == 7).any() and (ids > 0).any()
            r, rs = model.rank_targets(batch, ids, cat, item_bias=bias, item_time=time, window=win)
            live = ids > 0
            want = torch.arange(1, k + 1, dtype=torch.int32, device=DEV).expand(B, k)
            assert torch.equal(r[live], want[live]) and (r[~live] == 0).all()
            assert torch.equal(rs.view(torch.int32), sc.view(torch.int32))
            # windowed ranks never exceed the unwindowed ones for eligible targets
            r0, _ = model.rank_targets(batch, ids, cat, item_bias=bias)
            assert (r[live] <= r0[live]).all()
            # the diversity shortlist comes from the windowed top-k; lambda = 1 is the plain windowed list
            m_ids, m_sc = model.recommend(batch, k, cat, diversity=1.0, shortlist=k, item_bias=bias, item_time=time, window=win)
            assert torch.equal(m_ids, ids) and torch.equal(m_sc.view(torch.int32), sc.view(torch.int32))
        # defaults: today's bits
        a = model.recommend(batch, 20, cat)
        b_ = model.recommend(batch, 20, cat, item_time=None, window=None)
        assert torch.equal(a[0], b_[0]) and torch.equal(a[1].view(torch.int32), b_[1].view(torch.int32))
        with pytest.raises(_lib.NrmsError, match="window"):
            model.recommend(batch, 5, cat, item_time=time)
        with pytest.raises(_lib.NrmsError, match="window"):
            model.rank_targets(batch, ids, cat, window=win)
        with pytest.raises(_lib.NrmsError, match="item_time"):
            model.recommend(batch, 5, cat, item_time=time[:-1], window=win)
    model.check_recommend_ids()
