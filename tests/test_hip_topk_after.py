"""nrms_topk_dot_after / nrms_topk_dot_deep on the GPU (a cursor on the exact top-k and lists up to 4096, include/nrms_hip.h): exact
against tests/topk_after_ref.py on integer lattice data at every point where the kernels change path, the consequences (a) to (f)
the header states on Gaussian data, the buffer contract, the argument errors and the layers above (engine.top_k_after /
top_k_deep, Model.recommend_page / recommend_deep).  Every comparison is exact: ids and score bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream

from tests import topk_after_ref as ref
from tests import topk_window_ref as wref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F = np.float32
BEGIN = ref.BEGIN
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


def _kw(bias, time, win):
    return dict(bias=_t(bias, torch.float32), item_time=_t(time, torch.int32), window=_t(win, torch.int32))


def _after(user, items, k, a_s, a_i, ex, bias=None, time=None, win=None):
    """-> (ids, scores) as numpy, through the engine."""
    s, ids = _engine().top_k_after(_t(user, torch.float32), _t(items, torch.float32), k, _t(a_s, torch.float32), _t(a_i, torch.int64),
                                   _t(ex, torch.int64), **_kw(bias, time, win))
    return ids.cpu().numpy(), s.cpu().numpy()


def _deep(user, items, K, ex, bias=None, time=None, win=None):
    s, ids = _engine().top_k_deep(_t(user, torch.float32), _t(items, torch.float32), K, _t(ex, torch.int64), **_kw(bias, time, win))
    return ids.cpu().numpy(), s.cpu().numpy()


# ---- 1: lattice data ---------------------------------------------------------------------------------------------------------
# (B, N, d, k, n_exclude, bias, window): B = 33 is a full block of 32 users and a block of one; N = 5000 gives several slices; d spans
# no whole k-block (3, 31), whole blocks only (64) and blocks plus a remainder (301); k spans both P classes below 256 + 64 and both
# wave counts (k > 192: two waves); n_exclude spans TK_EX_LDS = 64.
LATTICE = [
    (1, 1, 3, 1, 0, False, False),
    (33, 63, 31, 7, 50, True, False),
    (33, 63, 3, 256, 0, True, True),          # k > N, and d = 3: almost every score ties
    (33, 700, 64, 64, 70, False, True),
    (33, 700, 301, 65, 50, True, True),
    (33, 5000, 31, 192, 0, False, False),
    (33, 5000, 64, 193, 70, True, True),
    (1, 5000, 3, 256, 50, False, False),
]


@functools.lru_cache(maxsize=None)
def _lattice(B, N, d, k, n_ex, with_bias, with_window):
    """Integer users and items in [-3, 3] (every dot product, and every sum with a multiple of 0.25 below 2^12, is exact in fp32
    whatever the order of summation; equal scores are abundant), duplicated item rows, item rows of NaN, a bias of multiples of 0.25
    with NaN, +inf and -inf entries, exclude lists with -1, N and a duplicate, shuffled times with two unpublished items and windows
    of every kind.  -> (user, items, sp, ok, bias, time, win, ex): sp the bits of s', ok the eligibility of the uncursored call."""
    rng = np.random.default_rng(100003 * d + 1009 * N + 17 * k + B + n_ex)
    user = rng.integers(-3, 4, size=(B, d)).astype(F)
    items = rng.integers(-3, 4, size=(N, d)).astype(F)
    if N >= 63:
        items[N // 2:N // 2 + 9] = items[3]                    # duplicated rows: runs of equal scores for every user
        items[[5, N - 2]] = np.nan                             # NaN rows: never returned
    with np.errstate(invalid="ignore"):
        s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(F)           # exact
    bias = None
    if with_bias:
        amp = int(4 * max(2.0, 4.0 * np.sqrt(d)))
        bias = (rng.integers(-amp, amp + 1, size=N) * 0.25).astype(F)
        if N >= 63:
            bias[rng.integers(0, N, size=3)] = np.nan
            bias[[7, 8, N // 3]] = np.inf                      # several items at +inf: a run of equal scores at the very top
            bias[[9, 10, N // 4]] = -np.inf                    # ... and at the very bottom
    time = win = None
    wt, ww = np.zeros(N, dtype=np.int64), np.tile(wref.FULL, (B, 1))
    if with_window:
        time = wt = rng.permutation(3 * np.arange(N, dtype=np.int64) - 1000)
        if N >= 8:
            wt[rng.integers(0, N, size=2)] = wref.I32_MAX
        lo = rng.integers(-1000, 3 * N - 1000, size=B)
        win = ww = np.stack([lo, lo + rng.integers(1, 3 * N, size=B)], axis=1).astype(np.int64)
        ww[0] = wref.FULL
        if B > 4:
            ww[3] = (5, 5)                                     # an empty window
    ex = None
    if n_ex:
        ex = rng.integers(0, max(N, 1), size=(B, n_ex)).astype(np.int64)
        ex[:, 0], ex[:, 1], ex[:, 2] = -1, N, ex[:, min(3, n_ex - 1)]
    sp = wref.scores_of(s, bias)
    ok = wref.eligible(sp, wt, ww, ex)
    return user, items, sp, ok, bias, time, win, ex


def _cursors(sp, ok, time, win, ex, N, seed):
    """One cursor per row, of kind b % 10; row 32, the only user of the second block, is at END, so that block exits early."""
    rng = np.random.default_rng(seed)
    B = sp.shape[0]
    a_s, a_i = np.zeros(B, dtype=F), np.full(B, BEGIN, dtype=np.int64)
    for b in range(B):
        order = ref.full_order(sp[b], ok[b])
        at = order[int(rng.integers(0, len(order)))] if len(order) else 0
        kind = b % 10
        if kind == 0:                                          # BEGIN; the score is not read
            a_s[b] = np.nan
        elif kind == 1:                                        # END
            a_s[b], a_i[b] = 1.0, -1
        elif kind == 2:                                        # on a listed item: with this data, inside a run of equal scores
            a_s[b], a_i[b] = sp[b, at], at
        elif kind == 3 and ex is not None:                     # on an excluded id
            x = int(ex[b, -1])
            a_s[b], a_i[b] = (sp[b, x] if not np.isnan(sp[b, x]) else 0.0), x
        elif kind == 4:                                        # ids at and beyond N: after everything at that score
            a_s[b], a_i[b] = sp[b, at], (N, N + 5, 2 ** 40, ref.MAX_ID + 1)[(b // 10) % 4]
        elif kind == 5 and time is not None:                   # on an item outside the window
            out = np.nonzero(~((time >= win[b, 0]) & (time < win[b, 1])) & ~np.isnan(sp[b]))[0]
            if len(out):
                a_s[b], a_i[b] = sp[b, out[0]], out[0]
        elif kind == 6:                                        # other negative ids, a NaN score: END
            a_s[b], a_i[b] = (np.nan, at) if b % 20 == 6 else (2.0, -7)
        elif kind == 7:                                        # -0.0 is +0.0; where no item scores 0 it is simply a position
            a_s[b], a_i[b] = -0.0, at
        elif kind == 8:                                        # +inf with id 0: before everything but item 0 at +inf; -inf: the last run
            a_s[b], a_i[b] = (np.inf, 0) if b % 20 == 8 else (-np.inf, 8)
        else:                                                  # a score no item has, id 0
            a_s[b], a_i[b] = sp[b, at] + 0.125, 0
    if B > 32:
        a_s[32], a_i[32] = 3.0, -1
    return a_s, a_i


@pytest.mark.parametrize("case", range(len(LATTICE)))
def test_lattice_after_and_deep_equal_the_restatement(case):
    B, N, d, k, n_ex, with_bias, with_window = LATTICE[case]
    user, items, sp, ok, bias, time, win, ex = _lattice(*LATTICE[case])
    for seed in (1, 2):
        a_s, a_i = _cursors(sp, ok, time, win, ex, N, seed)
        want = ref.after(sp, ok, a_s, a_i, k)
        _same(_after(user, items, k, a_s, a_i, ex, bias, time, win), want, "page, case %d seed %d" % (case, seed))
    # the second page of every row at once: cursors inside whatever run of equal scores the first page ended in
    p1 = ref.after(sp, ok, np.zeros(B, dtype=F), np.full(B, BEGIN), k)
    _same(_after(user, items, k, p1[1][:, -1], p1[0][:, -1], ex, bias, time, win), ref.after(sp, ok, p1[1][:, -1], p1[0][:, -1], k),
          "second page, case %d" % case)
    # a block that is all END, in every block
    got = _after(user, items, k, np.ones(B, dtype=F), np.full(B, -1), ex, bias, time, win)
    assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    for K in {1: (1, 5), 63: (63, 257), 700: (600, 4096), 5000: (257, 4096) if case == 6 else (600,)}[N]:
        _same(_deep(user, items, K, ex, bias, time, win), ref.deep(sp, ok, K), "deep, case %d K %d" % (case, K))


# ---- 2: Gaussian data, where the bits matter ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real(B=33, N=5000, d=64, n_ex=50):
    g = torch.Generator().manual_seed(7 + d + N)
    user = torch.randn(B, d, generator=g).to(DEV)
    items = torch.randn(N, d, generator=g).to(DEV)
    ex = torch.randint(0, N, (B, n_ex), generator=g).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    time = torch.randperm(N, generator=g).to(torch.int32).to(DEV)
    lo = torch.randint(0, N // 2, (B,), generator=g)
    win = torch.stack([lo, lo + torch.randint(N // 8, N, (B,), generator=g)], dim=1).to(torch.int32).to(DEV)
    win[0] = torch.tensor([wref.I32_MIN, wref.I32_MAX])
    return user, items, ex, bias, time, win


MODES = ("plain", "bias", "window", "bias+window")


def _mode_kw(mode, bias, time, win):
    return dict(bias=bias if "bias" in mode else None, item_time=time if "window" in mode else None,
                window=win if "window" in mode else None)


def _begin(B):
    return torch.zeros(B, device=DEV), torch.full((B,), BEGIN, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("d", [64, 301])
def test_all_begin_equals_the_uncursored_calls(d):
    """(a), at every k class, with the vector and the scalar chain."""
    user, items, ex, bias, time, win = _real(d=d)
    eng = _engine()
    for mode in MODES:
        kw = _mode_kw(mode, bias, time, win)
        for k in (1, 7, 64, 65, 192, 193, 256):
            _same(eng.top_k_after(user, items, k, *_begin(33), ex, **kw), eng.top_k(user, items, k, ex, **kw), "(a) %s k=%d" % (mode, k))


def _offset(t):
    """The same values at an address 4 bytes further on: no row starts on 16 bytes, the chain takes its scalar loads."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_pointers_offset_by_four_bytes():
    user, items, ex, bias, time, win = _real()
    eng = _engine()
    a_s, a_i = _begin(33)
    a_i[1::2] = 17
    a_s[1::2] = 1.5
    for k, kw in ((10, {}), (200, _mode_kw("bias+window", bias, time, win))):
        _same(eng.top_k_after(_offset(user), _offset(items), k, a_s, a_i, ex, **kw), eng.top_k_after(user, items, k, a_s, a_i, ex, **kw),
              "offset pointers, a page")
        _same(eng.top_k_deep(_offset(user), _offset(items), 300, ex, **kw), eng.top_k_deep(user, items, 300, ex, **kw), "offset pointers, deep")


@pytest.mark.parametrize("mode", MODES)
def test_pages_of_seven_chain_to_the_plain_list_and_then_pad_forever(mode):
    """(b): N <= 256, so the plain call at k = N is the whole ranking."""
    user, items, ex, bias, time, win = _real(N=200, d=31, n_ex=20)
    eng = _engine()
    kw = _mode_kw(mode, bias, time, win)
    N = 200
    full_s, full_i = eng.top_k(user, items, N, ex, **kw)
    a_s, a_i = _begin(33)
    ps, pi = [], []
    for _ in range(-(-N // 7) + 2):
        s, i = eng.top_k_after(user, items, 7, a_s, a_i, ex, **kw)
        ps.append(s)
        pi.append(i)
        a_s, a_i = s[:, -1].contiguous(), i[:, -1].contiguous()
    cs, ci = torch.cat(ps, dim=1), torch.cat(pi, dim=1)
    _same((cs[:, :N], ci[:, :N]), (full_s, full_i), "(b) %s" % mode)
    assert (ci[:, N:] == -1).all() and torch.isneginf(cs[:, N:]).all()
    assert (ci[:, 0] >= 0).all() and (full_i[:, -1] == -1).all()         # real pages, and rows that do run out (the exclude list)


@pytest.mark.parametrize("mode", MODES)
def test_deep_equals_the_plain_call_ranks_in_order_and_has_its_own_prefixes(mode):
    """(c), (d), (e), and the padding exactly where the eligible items run out."""
    user, items, ex, bias, time, win = _real()
    eng = _engine()
    kw = _mode_kw(mode, bias, time, win)
    B, N = 33, 5000
    for K in (1, 256):
        _same(eng.top_k_deep(user, items, K, ex, **kw), eng.top_k(user, items, K, ex, **kw), "(c) %s K=%d" % (mode, K))
    inside = torch.ones(B, N, dtype=torch.bool, device=DEV)
    if "window" in mode:
        inside = (time[None, :] >= win[:, :1]) & (time[None, :] < win[:, 1:])
    inside[torch.arange(B, device=DEV)[:, None], ex] = False
    n_el = inside.sum(dim=1)                                             # Gaussian scores: none is NaN
    deep = {K: eng.top_k_deep(user, items, K, ex, **kw) for K in (257, 600, 4096)}
    for K, (s, ids) in deep.items():
        r, rs = eng.rank_of(user, items, ids, ex, **kw)
        col = torch.arange(K, device=DEV).expand(B, K)
        live = col < n_el[:, None]
        assert torch.equal(ids >= 0, live), "(e) %s K=%d: the row ends where the eligible items run out" % (mode, K)
        assert torch.equal(r, torch.where(live, col + 1, torch.zeros_like(col)).to(torch.int32)), "(e) %s K=%d: ranks 1, 2, ..." % (mode, K)
        _same((rs,), (s,), "(e) %s K=%d: score bits" % (mode, K))
        assert torch.isneginf(s[~live]).all() and (ids[~live] == -1).all()
        _same((s, ids), (deep[4096][0][:, :K], deep[4096][1][:, :K]), "(d) %s K=%d" % (mode, K))
    if "window" in mode:
        assert (n_el < 4096).any() and (n_el > 600).any()
    # K > N
    u2, it2, ex2, b2, t2, w2 = _real(N=200, d=31, n_ex=20)
    s, ids = eng.top_k_deep(u2, it2, 4096, ex2, **_mode_kw(mode, b2, t2, w2))
    _same((s[:, :200], ids[:, :200]), eng.top_k(u2, it2, 200, ex2, **_mode_kw(mode, b2, t2, w2)), "K > N %s" % mode)
    assert (ids[:, 200:] == -1).all() and torch.isneginf(s[:, 200:]).all()


# ---- 3: invariance -----------------------------------------------------------------------------------------------------------
def _raw_after(user, items, bias, time, win, a_s, a_i, ex, k, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N = items.shape[0]
    need = int(lib.nrms_topk_dot_after_workspace_bytes(B, C.c_int64(N), d, k))
    assert need == int(lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    sc = torch.empty(B, k, dtype=torch.float32, device=DEV)
    ids = torch.empty(B, k, dtype=torch.int64, device=DEV)
    rc = lib.nrms_topk_dot_after(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), _lib.ptr(bias), _lib.ptr(time), _lib.ptr(win),
                                 _lib.ptr(a_s), _lib.ptr(a_i), _lib.ptr(ex), 0 if ex is None else ex.shape[1], _lib.ptr(sc), _lib.ptr(ids),
                                 _lib.ptr(ws), C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_topk_dot_after")
    return sc, ids


def _raw_deep(user, items, bias, time, win, ex, K, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N = items.shape[0]
    need = int(lib.nrms_topk_dot_deep_workspace_bytes(B, C.c_int64(N), d, K))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    sc = torch.empty(B, K, dtype=torch.float32, device=DEV)
    ids = torch.empty(B, K, dtype=torch.int64, device=DEV)
    rc = lib.nrms_topk_dot_deep(B, C.c_int64(N), d, K, _lib.ptr(user), _lib.ptr(items), _lib.ptr(bias), _lib.ptr(time), _lib.ptr(win),
                                _lib.ptr(ex), 0 if ex is None else ex.shape[1], _lib.ptr(sc), _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(need),
                                _stream())
    _lib.check(rc, "nrms_topk_dot_deep")
    return sc, ids


def test_invariance_and_determinism():
    """(f): two runs, B = 1, the row's position, the cursors around it, the row order of the catalogue, a poisoned workspace."""
    user, items, ex, bias, time, win = _real()
    eng = _engine()
    B, N, k = 33, 5000, 100
    kw = dict(bias=bias, item_time=time, window=win)
    first = eng.top_k(user, items, 40, ex, **kw)
    a_s, a_i = first[0][:, 36].contiguous(), first[1][:, 36].contiguous()      # a live cursor for every row that has 37 items
    sc, ids = eng.top_k_after(user, items, k, a_s, a_i, ex, **kw)
    assert (ids[:, 0] >= 0).sum() > 20
    _same((sc[:, :3], ids[:, :3]), (first[0][:, 37:40], first[1][:, 37:40]), "the page continues the list")
    _same(eng.top_k_after(user, items, k, a_s, a_i, ex, **kw), (sc, ids), "second run")
    for b in (0, 5, 31, 32):                                             # B = 1
        one = slice(b, b + 1)
        _same(eng.top_k_after(user[one].contiguous(), items, k, a_s[one].contiguous(), a_i[one].contiguous(), ex[one].contiguous(), bias=bias,
                              item_time=time, window=win[one].contiguous()), (sc[one], ids[one]), "B = 1, row %d" % b)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(DEV)
    up = lambda a: a[perm].contiguous()
    _same(eng.top_k_after(up(user), items, k, up(a_s), up(a_i), up(ex), bias=bias, item_time=time, window=up(win)), (sc[perm], ids[perm]),
          "user permutation")
    # the other rows on other pages: BEGIN, END, and elsewhere in their lists
    o_s, o_i = a_s.clone(), a_i.clone()
    keep = torch.arange(B, device=DEV) % 3 == 0
    o_i[~keep] = torch.tensor([BEGIN, -1, 4], device=DEV)[torch.arange(B, device=DEV) % 3][~keep]
    o_s[~keep] = 0.25
    s2, i2 = eng.top_k_after(user, items, k, o_s, o_i, ex, **kw)
    _same((s2[keep], i2[keep]), (sc[keep], ids[keep]), "other cursors around the row")
    # the catalogue's rows shuffled (items, bias and times together), ids mapped back: new row j holds old row rows[j]
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(4)).to(DEV)
    inv = torch.empty_like(rows)
    inv[rows] = torch.arange(N, device=DEV)
    skw = dict(bias=bias[rows].contiguous(), item_time=time[rows].contiguous(), window=win)
    m_i = torch.where(a_i >= 0, inv[a_i.clamp(min=0)], a_i)
    s3, i3 = eng.top_k_after(user, items[rows].contiguous(), k, a_s, m_i, inv[ex].contiguous(), **skw)
    _same((s3, torch.where(i3 >= 0, rows[i3.clamp(min=0)], i3)), (sc, ids), "row-shuffled catalogue")      # Gaussian scores: no ties
    d_s, d_i = eng.top_k_deep(user, items, 700, ex, **kw)
    s4, i4 = eng.top_k_deep(user, items[rows].contiguous(), 700, inv[ex].contiguous(), **skw)
    _same((s4, torch.where(i4 >= 0, rows[i4.clamp(min=0)], i4)), (d_s, d_i), "row-shuffled catalogue, deep")
    _same(eng.top_k_deep(user[5:6].contiguous(), items, 700, ex[5:6].contiguous(), bias=bias, item_time=time, window=win[5:6].contiguous()),
          (d_s[5:6], d_i[5:6]), "deep at B = 1")
    for fill in (0xFF, 0x00):
        _same(_raw_after(user, items, bias, time, win, a_s, a_i, ex, k, fill), (sc, ids), "workspace 0x%02X" % fill)
        _same(_raw_deep(user, items, bias, time, win, ex, 700, fill), (d_s, d_i), "workspace 0x%02X, deep" % fill)


# ---- 4: the buffer contract --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,K", [(1, 5), (4, 257), (6, 600)])
def test_buffer_contract(case, K):
    """Outputs and the workspace at the queried size between guard bands, the workspace poisoned three ways; the cursor, bias,
    item_time and window are guarded too, at exactly their sizes.  The deep call writes every element of its outputs."""
    from tests.guarded import POISONS, Pool
    from tests.test_hip_buffer_contracts import dev, ok, refuses_undersized, three_poisons
    lib = _lib.load()
    B, N, d, k, n_ex, with_bias, with_window = LATTICE[case]
    user, items, sp, okm, bias, time, win, ex = _lattice(*LATTICE[case])
    a_s, a_i = _cursors(sp, okm, time, win, ex, N, 3)
    ud, itd, exd = dev(np.array(user)), dev(np.array(items)), dev(ex, torch.int64)
    need_a = int(lib.nrms_topk_dot_after_workspace_bytes(B, C.c_int64(N), d, k))
    need_d = int(lib.nrms_topk_dot_deep_workspace_bytes(B, C.c_int64(N), d, K))
    assert need_a > 0 and need_d > 0
    ins = ["after_scores", "after_ids"] + (["bias"] if with_bias else []) + (["time", "window"] if with_window else [])

    def run(poison):
        P = Pool(poison)
        P.elems("after_scores", B, torch.float32, init=torch.from_numpy(a_s))
        P.elems("after_ids", B, torch.int64, init=torch.from_numpy(a_i))
        if with_bias:
            P.elems("bias", N, torch.float32, init=torch.from_numpy(np.array(bias)))
        if with_window:
            P.elems("time", N, torch.int32, init=torch.from_numpy(np.array(time)).to(torch.int32))
            P.elems("window", 2 * B, torch.int32, init=torch.from_numpy(np.array(win)).to(torch.int32).reshape(-1))
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, torch.int64), P.new("ws_after", need_a)
        P.elems("deep_scores", B * K), P.elems("deep_ids", B * K, torch.int64), P.new("ws_deep", need_d)
        opt = lambda n: P[n].ptr if n in ins else None

        def call_a(nbytes):
            return lib.nrms_topk_dot_after(B, C.c_int64(N), d, k, _lib.ptr(ud), _lib.ptr(itd), opt("bias"), opt("time"), opt("window"),
                                           P["after_scores"].ptr, P["after_ids"].ptr, _lib.ptr(exd), n_ex, P["top_scores"].ptr,
                                           P["top_ids"].ptr, P["ws_after"].ptr, C.c_size_t(nbytes), _stream())

        def call_d(nbytes):
            return lib.nrms_topk_dot_deep(B, C.c_int64(N), d, K, _lib.ptr(ud), _lib.ptr(itd), opt("bias"), opt("time"), opt("window"),
                                          _lib.ptr(exd), n_ex, P["deep_scores"].ptr, P["deep_ids"].ptr, P["ws_deep"].ptr,
                                          C.c_size_t(nbytes), _stream())

        snap = [P[n].snapshot() for n in ins]
        ok(call_a(need_a), "nrms_topk_dot_after")
        P.intact("nrms_topk_dot_after")
        ok(call_d(need_d), "nrms_topk_dot_deep")
        P.intact("nrms_topk_dot_deep")
        assert all(P[n].unchanged_since(sn) for n, sn in zip(ins, snap))
        if poison == POISONS[0]:
            keep = {n: P[n].numpy() for n in ("top_scores", "top_ids", "deep_scores", "deep_ids")}
            refuses_undersized(call_a, P, need_a, "nrms_topk_dot_after")
            refuses_undersized(call_d, P, need_d, "nrms_topk_dot_deep")
            assert all(np.array_equal(_bits(keep[n]), _bits(P[n].numpy())) for n in keep)
        return {"ids": P["top_ids"].numpy((B, k)), "scores": P["top_scores"].numpy((B, k)), "dids": P["deep_ids"].numpy((B, K)),
                "dscores": P["deep_scores"].numpy((B, K))}

    # the three poisons agree bit for bit, so no element of an output kept its poison: the outputs are written in full
    out = three_poisons(run, "the cursored calls")[POISONS[0]]
    _same((out["ids"], out["scores"]), ref.after(sp, okm, a_s, a_i, k), "a page between guard bands")
    _same((out["dids"], out["dscores"]), ref.deep(sp, okm, K), "the deep list between guard bands")


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    user, items, ex, bias, time, win = _real()
    B, N, d, k, K = 33, 5000, 64, 10, 300
    ws = torch.empty(1 << 20, dtype=torch.int64, device=DEV)
    sc = torch.full((B, K), 5.0, device=DEV)
    ids = torch.full((B, K), 5, dtype=torch.int64, device=DEV)
    a_s, a_i = _begin(B)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    P = _lib.ptr

    def after(B=B, N=N, d=d, k=k, bias=P(bias), time=P(time), win=P(win), a_s=P(a_s), a_i=P(a_i), n_ex=0, nbytes=ws.numel() * 8):
        return lib.nrms_topk_dot_after(B, C.c_int64(N), d, k, P(user), P(items), bias, time, win, a_s, a_i, None, n_ex, P(sc), P(ids), P(ws),
                                       C.c_size_t(nbytes), _stream())

    def deep(B=B, N=N, d=d, K=K, bias=P(bias), time=P(time), win=P(win), n_ex=0, nbytes=ws.numel() * 8):
        return lib.nrms_topk_dot_deep(B, C.c_int64(N), d, K, P(user), P(items), bias, time, win, None, n_ex, P(sc), P(ids), P(ws),
                                      C.c_size_t(nbytes), _stream())

    common = [(dict(time=None), b"item_time is null"), (dict(win=None), b"window is null"), (dict(time=off(time, 2)), b"item_time must be 4-byte aligned"),
              (dict(win=off(win, 1)), b"window must be 4-byte aligned"), (dict(bias=off(bias, 2)), b"bias must be 4-byte aligned"),
              (dict(B=-1), b"B must be"), (dict(N=-1), b"N must be"), (dict(d=0), b"d must be"), (dict(n_ex=-1), b"n_exclude must be")]
    for kw, word in common + [(dict(k=0), b"k must be"), (dict(k=257), b"k must be"), (dict(a_s=None), b"after_scores is null"),
                              (dict(a_i=None), b"after_ids is null"), (dict(a_s=off(a_s, 2)), b"after_scores must be 4-byte aligned"),
                              (dict(a_i=off(a_i, 4)), b"after_ids must be 8-byte aligned")]:
        assert after(**kw) == _lib.NRMS_EINVAL, kw
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_after: ") and word in msg, msg
    for kw, word in common + [(dict(K=0), b"K must be"), (dict(K=4097), b"K must be")]:
        assert deep(**kw) == _lib.NRMS_EINVAL, kw
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_deep: ") and word in msg, msg
    assert after(nbytes=64) == _lib.NRMS_EWORKSPACE and deep(nbytes=64) == _lib.NRMS_EWORKSPACE
    torch.cuda.synchronize()
    assert (sc == 5.0).all() and (ids == 5).all()                        # nothing was launched
    assert after(B=0) == _lib.NRMS_OK and deep(B=0) == _lib.NRMS_OK      # B = 0 is a no-op
    torch.cuda.synchronize()
    assert (sc == 5.0).all() and (ids == 5).all()
    eng = _engine()
    for bad in (dict(a_s=a_s[:-1].contiguous()), dict(a_i=a_i.to(torch.int32)), dict(a_s=a_s.cpu())):
        with pytest.raises(_lib.NrmsError, match="after_"):
            eng.top_k_after(user, items, 5, bad.get("a_s", a_s), bad.get("a_i", a_i), ex)
    with pytest.raises(_lib.NrmsError, match="1 <= k <= 256"):
        eng.top_k_after(user, items, 257, a_s, a_i, ex)
    with pytest.raises(_lib.NrmsError, match="1 <= K <= 4096"):
        eng.top_k_deep(user, items, 4097, ex)
    with pytest.raises(_lib.NrmsError, match="window"):
        eng.top_k_deep(user, items, 300, ex, item_time=time)


# ---- 5: the models -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_models_page_and_go_deep(kind):
    from pytorch_news_recommender_amd.model.nrms_hip import PAGE_BEGIN
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model(kind)
    N = cat.shape[0]
    rng = np.random.default_rng(5)
    time = torch.from_numpy(rng.integers(0, 100, size=N)).to(DEV)
    time[7] = wref.I32_MAX
    prior = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(DEV)
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    batch = batches[0]
    B = torch.as_tensor(batch["browsed_ids"]).shape[0]
    lo = torch.from_numpy(rng.integers(0, 60, size=B)).to(DEV)
    win = torch.stack([lo, lo + 50], dim=1)
    win[0] = torch.tensor([40, 40])
    K, k = 300, 64                                                       # K > 256: two pages on the device; K >= N - 1: the rows run out
    for kw in ({}, dict(item_bias=prior), dict(item_time=time, window=win), dict(item_bias=prior, item_time=time, window=win)):
        d_ids, d_sc = model.recommend_deep(batch, K, cat, **kw)
        assert same(model.recommend_page(batch, k, cat, **kw), model.recommend(batch, k, cat, **kw))          # the first page
        after, pages = None, []
        for _ in range(-(-K // k)):
            ids, sc = model.recommend_page(batch, k, cat, after, **kw)
            pages.append((ids, sc))
            after = (ids[:, -1], sc[:, -1])
        c_ids, c_sc = torch.cat([p[0] for p in pages], dim=1)[:, :K], torch.cat([p[1] for p in pages], dim=1)[:, :K]
        assert same((c_ids, c_sc), (d_ids, d_sc))
        assert same((d_ids[:, :256], d_sc[:, :256]), model.recommend(batch, 256, cat, **kw))
        r, rs = model.rank_targets(batch, d_ids, cat, **kw)
        live = d_ids > 0
        want = torch.arange(1, K + 1, dtype=torch.int32, device=DEV).expand(B, K)
        assert torch.equal(r[live], want[live]) and (r[~live] == 0).all() and (d_ids[~live] == -1).all()
        assert torch.equal(rs.view(torch.int32), d_sc.view(torch.int32))
        assert live[:, 0].any() and (~live[:, -1]).any() and not (d_ids == 0).any()
        if "window" in kw:
            assert (d_ids[0] == -1).all() and not (d_ids == 7).any()
        # rows that start over share a call with rows that go on and rows that are done
        a_ids, a_sc = pages[0][0][:, -1].clone(), pages[0][1][:, -1].clone()
        a_ids[0::3] = PAGE_BEGIN
        a_ids[1::3] = -1
        ids, sc = model.recommend_page(batch, k, cat, (a_ids, a_sc), **kw)
        assert same((ids[0::3], sc[0::3]), (pages[0][0][0::3], pages[0][1][0::3]))
        assert (ids[1::3] == -1).all() and torch.isneginf(sc[1::3]).all()
        assert same((ids[2::3], sc[2::3]), (pages[1][0][2::3], pages[1][1][2::3]))
    with pytest.raises(_lib.NrmsError, match="after"):
        model.recommend_page(batch, k, cat, (torch.zeros(B + 1, dtype=torch.int64), torch.zeros(B + 1)))
    with pytest.raises(_lib.NrmsError, match="1 <= K <= 4096"):
        model.recommend_deep(batch, 4097, cat)
