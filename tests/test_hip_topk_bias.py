"""nrms_topk_dot_biased / nrms_rank_dot_biased on the GPU (a per-news additive prior in retrieval and exact ranking,
include/nrms_hip.h): exact against tests/topk_bias_ref.py on integer lattice data at every point where the kernels change path
and on real-valued data from nrms_rank_dot's own score bits, the identities the header states, invariance and determinism, the
buffer contract, and the layers above (Model.recommend / rank_targets with item_bias, ClickFeed.popularity_prior, run_v0
--popularity_prior).  Every comparison is exact: ids, ranks and score bits."""
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

from tests import topk_bias_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _topk(user, items, k, ex, bias):
    s, ids = _engine().top_k(_t(user, torch.float32), _t(items, torch.float32), k, _t(ex, torch.int64), bias=_t(bias, torch.float32))
    return ids.cpu().numpy(), s.cpu().numpy()


def _rank(user, items, tg, ex, bias):
    r, s = _engine().rank_of(_t(user, torch.float32), _t(items, torch.float32), _t(tg, torch.int64), _t(ex, torch.int64),
                             bias=_t(bias, torch.float32))
    return r.cpu().numpy(), s.cpu().numpy()


# ---- 1: lattice data ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice(B, N, d, k, T, n_ex):
    """Integer users and items in [-3, 3] (|score| <= 9 d <= 2700: every dot product, and every sum with a multiple of 0.25 below
    2^12, is exact in fp32 whatever the order of summation), a bias of multiples of 0.25 on the scale of the scores with NaN and
    -inf entries, exclude lists with -1, N and a duplicate, targets that name NaN-bias, -inf-bias, excluded and out-of-range ids.
    The bias is then adjusted until the conditions the test asserts hold (see _conditions): never by looking at the GPU."""
    rng = np.random.default_rng(100003 * d + 1009 * N + 17 * k + B + T + n_ex)
    user = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)         # exact
    assert N == 0 or np.abs(s).max() <= 9 * d
    amp = int(4 * max(2.0, 4.0 * np.sqrt(d)))                                             # quarter steps up to about one score sigma
    bias = (rng.integers(-amp, amp + 1, size=N) * 0.25).astype(np.float32)
    ex = None
    if n_ex:
        ex = rng.integers(0, max(N, 1), size=(B, n_ex)).astype(np.int64)
        ex[:, 0], ex[:, 1], ex[:, 2] = -1, N, ex[:, 3]
    nan_ids, inf_id = np.zeros(0, dtype=np.int64), -1
    shadow = bias.copy()                                                                  # what the NaN entries would have been
    if N >= 31:
        top = ref.topk(s, bias, ex, 1)[0]
        row = min(1, B - 1)
        nan_ids = np.unique(np.concatenate([[top[row, 0]], rng.integers(0, N, size=3)]))   # one of them heads a user's list
        inf_id = int(np.setdiff1d(np.arange(N), nan_ids)[-1])
        bias[nan_ids] = np.nan
        bias[inf_id] = shadow[inf_id] = -np.inf
        frozen = set(nan_ids.tolist()) | {inf_id}
        for _ in range(200):
            b_ids, b_sc = ref.topk(s, bias, ex, min(k + 1, N))
            u_ids = ref.topk(s, None, ex, min(k + 1, N))[0]
            moved = False
            for b in range(B):                     # (a) a user whose two lists agree: its best movable item is demoted
                if b_ids[b, -1] < 0 or not np.array_equal(b_ids[b, :k], u_ids[b, :k]):
                    continue
                t = next((int(t) for t in b_ids[b, :k] if int(t) not in frozen), None)
                if t is not None:
                    bias[t] -= np.float32(0.25 * 8 * amp)
                    shadow[t] = bias[t]
                    moved = True
            if moved:
                continue
            full = [b for b in range(B) if b_ids[b, -1] >= 0 and np.isfinite(b_sc[b, k - 1]) and np.isfinite(b_sc[b, k])]
            if not full or any(b_sc[b, k - 1] == b_sc[b, k] for b in full):
                break
            b = full[0]                            # (b) the (k+1)-th of one user is raised to a tie with its k-th
            a, c = int(b_ids[b, k - 1]), int(b_ids[b, k])
            if a in frozen or c in frozen:
                frozen_free = [x for x in full if int(b_ids[x, k]) not in frozen and int(b_ids[x, k - 1]) not in frozen]
                if not frozen_free:
                    break
                b = frozen_free[0]
                a, c = int(b_ids[b, k - 1]), int(b_ids[b, k])
            bias[c] += b_sc[b, k - 1] - b_sc[b, k]
            shadow[c] = bias[c]
        assert np.array_equal(bias[np.isfinite(bias)] * 4, np.round(bias[np.isfinite(bias)] * 4)) and np.abs(bias[np.isfinite(bias)]).max() < 4096
    tg = rng.integers(0, max(N, 1), size=(B, T)).astype(np.int64)
    if N >= 31:
        for b in range(B):
            special = [int(nan_ids[b % len(nan_ids)]), inf_id, N, int(ex[b, 4]) if ex is not None else -1, int(tg[b, 0])]
            if T >= 6:
                tg[b, 1:6] = special
            else:
                tg[b, T - 1] = special[b % 5]
    for a in (user, items, s, bias, shadow, tg):
        a.setflags(write=False)
    return user, items, s, bias, shadow, ex, tg, nan_ids


def _conditions(s, bias, shadow, ex, tg, nan_ids, k):
    """On the CPU-side data, before anything is compared: the test cannot pass by ignoring the bias."""
    B, N = s.shape
    b_ids, b_sc = ref.topk(s, bias, ex, min(k + 1, N))
    u_ids = ref.topk(s, None, ex, min(k + 1, N))[0]
    full = [b for b in range(B) if b_ids.shape[1] == k + 1 and b_ids[b, k] >= 0]          # users with at least k + 1 eligible items
    assert full, "no user has k + 1 eligible items"
    for b in full:
        assert not np.array_equal(b_ids[b, :k], u_ids[b, :k]), "user %d: the biased and the unbiased list agree" % b
    tied = [b for b in full if b_sc[b, k - 1] == b_sc[b, k]]
    assert tied, "no user has a tie at the k-th place"
    assert all(b_ids[b, k - 1] < b_ids[b, k] for b in tied)                               # ... which the id rule decides
    would = ref.topk(s, shadow, ex, k)[0]
    assert np.isin(nan_ids, would).any(), "no NaN-bias item would otherwise be in a top k"
    assert np.isin(nan_ids, tg).any(), "no NaN-bias item is a target"


# (B, N, d, k, T, n_exclude): every value of B {1, 33, 70}, N {0, 1, 31, 33, 513, 5000}, d {1, 7, 32, 40, 300}, k {1, 10, 200,
# 256}, T {1, 5, 32}, n_exclude {0, 5, 70}, at the points where the kernels change path
LATTICE = [
    (1, 0, 7, 1, 1, 0),              # an empty catalogue
    (1, 1, 1, 1, 1, 0),              # one item, one user, d = 1
    (33, 31, 7, 10, 5, 5),           # fewer than 32 items, a partial user tile, the non-vector path, a remainder-only d
    (33, 33, 32, 10, 5, 0),          # a tail tile of one item, one whole block of d
    (70, 513, 40, 200, 32, 5),       # the two-wave block above k = 192, a whole block of d and a remainder group
    (70, 5000, 300, 256, 1, 70),     # more than one slice, three user tiles, the exclude list beyond the 64 that LDS holds
    (1, 5000, 32, 10, 32, 70),       # one user against several slices
    (70, 5000, 1, 1, 5, 5),          # k = 1, d = 1: ties everywhere
    (33, 513, 300, 10, 1, 0),
]


@pytest.mark.parametrize("B,N,d,k,T,n_ex", LATTICE)
def test_exact_on_lattice_data(B, N, d, k, T, n_ex):
    user, items, s, bias, shadow, ex, tg, nan_ids = _lattice(B, N, d, k, T, n_ex)
    if N >= 31:
        _conditions(s, bias, shadow, ex, tg, nan_ids, k)
    _same(_topk(user, items, k, ex, bias), ref.topk(s, bias, ex, k), "biased top-k")
    got = _rank(user, items, tg, ex, bias)
    _same(got, ref.ranks(s, bias, ex, tg), "biased rank")
    if N >= 31:
        hit = np.isin(tg, nan_ids)
        assert hit.any() and (got[0][hit] == 0).all() and (got[1][hit] == -np.inf).all()       # a NaN prior: rank 0 / -inf
        inf_id = int(np.nonzero(np.isneginf(bias))[0][0])
        at = (tg == inf_id) & (got[0] > 0)
        assert (got[1][at] == -np.inf).all()                                                   # a -inf prior: ranked, score -inf


def test_minus_inf_comes_last_and_plus_inf_first():
    user, items, s, bias, shadow, ex, tg, nan_ids = _lattice(33, 33, 32, 10, 5, 0)
    b2 = np.array(bias)
    fin = np.nonzero(np.isfinite(b2))[0]
    b2[fin[0]] = np.inf
    ids, sc = _topk(user, items, 33, None, b2)
    _same((ids, sc), ref.topk(s, b2, None, 33), "infinite priors")
    n_el = 33 - len(nan_ids)
    inf_id = int(np.nonzero(np.isneginf(b2))[0][0])
    assert (ids[:, 0] == fin[0]).all() and (sc[:, 0] == np.inf).all()
    assert (ids[:, n_el - 1] == inf_id).all() and (sc[:, n_el - 1] == -np.inf).all() and (ids[:, n_el:] == -1).all()
    # +inf + -inf: an item row of +inf against users whose entry is positive scores +inf, and a -inf prior makes it NaN
    it2 = np.array(items)
    u2 = np.abs(np.array(user)) + 1.0
    it2[5] = np.inf
    b3 = np.zeros(33, dtype=np.float32)
    b3[5] = -np.inf
    ids, sc = _topk(u2, it2, 33, None, b3)
    assert not (ids == 5).any() and (ids[:, 32] == -1).all() and (ids[:, 31] >= 0).all()
    ids0, _ = _topk(u2, it2, 1, None, None)
    assert (ids0[:, 0] == 5).all()                                                             # without the prior it is first
    r, rs = _rank(u2, it2, np.full((33, 1), 5), None, b3)
    assert (r == 0).all() and (rs == -np.inf).all()


# ---- 2: real-valued data -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _real():
    """B = 70, N = 20 000, d = 300 Gaussian data; the plain score bits of every (user, item) from nrms_rank_dot's target_scores
    over all ids, in column chunks (rank_of takes 32 targets per call), computed once and shared."""
    B, N, d = 70, 20000, 300
    g = torch.Generator(device=DEV).manual_seed(5)
    user = torch.randn(B, d, device=DEV, generator=g)
    items = torch.randn(N, d, device=DEV, generator=g)
    ex = torch.randint(0, N, (B, 50), device=DEV, generator=g)
    bias = (torch.randn(N, device=DEV, generator=g) * 6.0).contiguous()
    nan_ids = torch.randint(0, N, (40,), device=DEV, generator=g)
    bias[nan_ids] = float("nan")
    tg = torch.randint(0, N, (B, 8), device=DEV, generator=g)
    tg[:, 7] = nan_ids[torch.arange(B, device=DEV) % 40]                            # a blocked target in every row
    eng = _engine()
    cols = []
    for c0 in range(0, N, 2048):
        ids = torch.arange(c0, min(N, c0 + 2048), device=DEV).expand(B, -1).contiguous()
        r, sc = eng.rank_of(user, items, ids, None)
        assert (r > 0).all()
        cols.append(sc)
    s = torch.cat(cols, dim=1).cpu().numpy()
    return user, items, ex, bias, tg, s


def test_exact_on_real_valued_data():
    user, items, ex, bias, tg, s = _real()
    eng = _engine()
    B, k = user.shape[0], 100
    bn, exn, tgn = bias.cpu().numpy(), ex.cpu().numpy(), tg.cpu().numpy()
    sc, ids = eng.top_k(user, items, k, ex, bias=bias)
    want = ref.topk(s, bn, exn, k)
    _same((ids, sc), want, "biased top-k")
    plain = eng.top_k(user, items, k, ex)[1].cpu().numpy()
    assert all(not np.array_equal(plain[b], want[0][b]) for b in range(B))                    # the prior moved every list
    r, rs = eng.rank_of(user, items, tg, ex, bias=bias)
    _same((r, rs), ref.ranks(s, bn, exn, tgn), "biased rank")
    assert (r[:, 7] == 0).all() and (r[:, :7] > 0).any()
    r2, rs2 = eng.rank_of(user, items, ids, ex, bias=bias)                                    # the served list ranks 1 .. k
    assert torch.equal(r2, torch.arange(1, k + 1, dtype=torch.int32, device=DEV).expand(B, k))
    _same((rs2,), (sc,), "scores of the served list")


# ---- 3: identities -----------------------------------------------------------------------------------------------------------
def _raw_topk(user, items, bias_ptr, ex, k, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N = items.shape[0]
    need = int(lib.nrms_topk_dot_biased_workspace_bytes(B, C.c_int64(N), d, k))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    sc = torch.empty(B, k, dtype=torch.float32, device=DEV)
    ids = torch.empty(B, k, dtype=torch.int64, device=DEV)
    rc = lib.nrms_topk_dot_biased(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), bias_ptr, _lib.ptr(ex),
                                  0 if ex is None else ex.shape[1], _lib.ptr(sc), _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8),
                                  _stream())
    _lib.check(rc, "nrms_topk_dot_biased")
    return ids, sc


def _raw_rank(user, items, bias_ptr, tg, ex, ws_fill=None):
    lib = _lib.load()
    B, d = user.shape
    N, T = items.shape[0], tg.shape[1]
    n_ex = 0 if ex is None else ex.shape[1]
    need = int(lib.nrms_rank_dot_biased_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    r = torch.empty(B, T, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, T, dtype=torch.float32, device=DEV)
    rc = lib.nrms_rank_dot_biased(B, C.c_int64(N), d, T, _lib.ptr(user), _lib.ptr(items), bias_ptr, _lib.ptr(tg), _lib.ptr(ex), n_ex,
                                  _lib.ptr(r), _lib.ptr(sc), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
    _lib.check(rc, "nrms_rank_dot_biased")
    return r, sc


def test_null_and_zero_bias_are_the_unbiased_calls():
    user, items, ex, bias, tg, s = _real()
    eng = _engine()
    N = items.shape[0]
    sc0, ids0 = eng.top_k(user, items, 100, ex)
    r0, rs0 = eng.rank_of(user, items, tg, ex)
    zero = torch.zeros(N, device=DEV)
    for what, ptr in (("null bias", None), ("zero bias", _lib.ptr(zero))):
        _same(_raw_topk(user, items, ptr, ex, 100), (ids0, sc0), what)
        _same(_raw_rank(user, items, ptr, tg, ex), (r0, rs0), what)
    sc, ids = eng.top_k(user, items, 100, ex, bias=zero)
    _same((ids, sc), (ids0, sc0), "zero bias through the engine")
    # lattice data full of zero scores (d = 1: every zero user entry, every zero item), with a bias of +0.0 and of -0.0
    u, it, s_l, b_l, _, ex_l, tg_l, _ = _lattice(70, 5000, 1, 1, 5, 5)
    assert (s_l == 0).sum() > 5000
    for z in (np.zeros(5000, dtype=np.float32), np.full(5000, -0.0, dtype=np.float32)):
        _same(_topk(u, it, 10, ex_l, z), _topk(u, it, 10, ex_l, None), "zero bias on lattice data")
        _same(_rank(u, it, tg_l, ex_l, z), _rank(u, it, tg_l, ex_l, None), "zero bias on lattice data")


def test_constant_bias_keeps_ids_and_ranks():
    u, it, s, _, _, ex, tg, _ = _lattice(70, 513, 40, 200, 32, 5)
    for cst in (0.25, -1024.75):                                                   # exact sums: the order cannot move
        b = np.full(513, cst, dtype=np.float32)
        ids, sc = _topk(u, it, 200, ex, b)
        ids0, sc0 = _topk(u, it, 200, ex, None)
        np.testing.assert_array_equal(ids, ids0)
        np.testing.assert_array_equal(sc[ids >= 0], (sc0 + np.float32(cst))[ids >= 0])
        r, rs = _rank(u, it, tg, ex, b)
        r0, rs0 = _rank(u, it, tg, ex, None)
        np.testing.assert_array_equal(r, r0)
        np.testing.assert_array_equal(rs[r > 0], (rs0 + np.float32(cst))[r > 0])


def test_bias_needs_four_byte_alignment_only():
    user, items, ex, bias, tg, s = _real()
    eng = _engine()
    N = items.shape[0]
    buf = torch.empty(N + 1, device=DEV)
    view = buf[1:]
    view.copy_(bias)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and bias.data_ptr() % 16 == 0
    a = eng.top_k(user, items, 100, ex, bias=bias)
    b = eng.top_k(user, items, 100, ex, bias=view)
    _same(b, a, "a bias view one element into its buffer")
    _same(eng.rank_of(user, items, tg, ex, bias=view), eng.rank_of(user, items, tg, ex, bias=bias), "a bias view")


# ---- 4: invariance and determinism -------------------------------------------------------------------------------------------
def test_invariance_and_determinism():
    user, items, ex, bias, tg, s = _real()
    eng = _engine()
    k = 100
    sc, ids = eng.top_k(user, items, k, ex, bias=bias)
    r, rs = eng.rank_of(user, items, tg, ex, bias=bias)
    sc2, ids2 = eng.top_k(user, items, k, ex, bias=bias)                           # two runs
    r2, rs2 = eng.rank_of(user, items, tg, ex, bias=bias)
    _same((ids2, sc2), (ids, sc), "second run")
    _same((r2, rs2), (r, rs), "second run")
    parts = [(slice(0, 32)), (slice(32, 70))]                                      # 70 = 32 + 38
    pk = [eng.top_k(user[p].contiguous(), items, k, ex[p].contiguous(), bias=bias) for p in parts]
    pr = [eng.rank_of(user[p].contiguous(), items, tg[p].contiguous(), ex[p].contiguous(), bias=bias) for p in parts]
    _same((torch.cat([x[1] for x in pk]), torch.cat([x[0] for x in pk])), (ids, sc), "batch split")
    _same((torch.cat([x[0] for x in pr]), torch.cat([x[1] for x in pr])), (r, rs), "batch split")
    perm = torch.randperm(70, generator=torch.Generator().manual_seed(3)).to(DEV)   # row permutation
    scp, idsp = eng.top_k(user[perm].contiguous(), items, k, ex[perm].contiguous(), bias=bias)
    rp, rsp = eng.rank_of(user[perm].contiguous(), items, tg[perm].contiguous(), ex[perm].contiguous(), bias=bias)
    _same((idsp, scp), (ids[perm], sc[perm]), "row permutation")
    _same((rp, rsp), (r[perm], rs[perm]), "row permutation")
    for k2 in (10, 256):                                                           # k: a prefix
        s3, i3 = eng.top_k(user, items, k2, ex, bias=bias)
        n = min(k, k2)
        _same((i3[:, :n], s3[:, :n]), (ids[:, :n], sc[:, :n]), "k = %d" % k2)
    for fill in (0xFF, 0x00, 0x7F):                                                # a poisoned workspace
        _same(_raw_topk(user, items, _lib.ptr(bias), ex, k, fill), (ids, sc), "workspace 0x%02X" % fill)
        _same(_raw_rank(user, items, _lib.ptr(bias), tg, ex, fill), (r, rs), "workspace 0x%02X" % fill)


# ---- 5: the buffer contract --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,d,k,T,n_ex", [(33, 31, 7, 10, 5, 5), (70, 513, 40, 200, 32, 5), (1, 5000, 32, 10, 32, 70)])
def test_buffer_contract(B, N, d, k, T, n_ex):
    """Outputs and the workspace at the queried size between guard bands, the workspace poisoned three ways; the bias itself is
    guarded too, at exactly N floats."""
    from tests.guarded import POISONS, Pool
    from tests.test_hip_buffer_contracts import dev, ok, refuses_undersized, three_poisons
    lib = _lib.load()
    user, items, s, bias, shadow, ex, tg, nan_ids = _lattice(B, N, d, k, T, n_ex)
    ud, itd, tgd, exd = dev(np.array(user)), dev(np.array(items)), dev(np.array(tg), torch.int64), dev(ex, torch.int64)
    need_k = int(lib.nrms_topk_dot_biased_workspace_bytes(B, C.c_int64(N), d, k))
    need_r = int(lib.nrms_rank_dot_biased_workspace_bytes(B, C.c_int64(N), d, T, n_ex))
    assert need_k > 0 and need_r > 0

    def run(poison):
        P = Pool(poison)
        P.elems("bias", N, torch.float32, init=torch.from_numpy(np.array(bias)))
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, torch.int64), P.new("ws_topk", need_k)
        P.elems("ranks", B * T, torch.int32), P.elems("target_scores", B * T), P.new("ws_rank", need_r)

        def call_k(nbytes):
            return lib.nrms_topk_dot_biased(B, C.c_int64(N), d, k, _lib.ptr(ud), _lib.ptr(itd), P["bias"].ptr, _lib.ptr(exd), n_ex,
                                            P["top_scores"].ptr, P["top_ids"].ptr, P["ws_topk"].ptr, C.c_size_t(nbytes), _stream())

        def call_r(nbytes):
            return lib.nrms_rank_dot_biased(B, C.c_int64(N), d, T, _lib.ptr(ud), _lib.ptr(itd), P["bias"].ptr, _lib.ptr(tgd),
                                            _lib.ptr(exd), n_ex, P["ranks"].ptr, P["target_scores"].ptr, P["ws_rank"].ptr,
                                            C.c_size_t(nbytes), _stream())

        snap = P["bias"].snapshot()
        ok(call_k(need_k), "nrms_topk_dot_biased")
        P.intact("nrms_topk_dot_biased")
        ok(call_r(need_r), "nrms_rank_dot_biased")
        P.intact("nrms_rank_dot_biased")
        assert P["bias"].unchanged_since(snap)
        if poison == POISONS[0]:
            keep = {n: P[n].numpy() for n in ("top_scores", "top_ids", "ranks", "target_scores")}
            refuses_undersized(call_k, P, need_k, "nrms_topk_dot_biased")
            refuses_undersized(call_r, P, need_r, "nrms_rank_dot_biased")
            assert all(np.array_equal(_bits(keep[n]), _bits(P[n].numpy())) for n in keep)
        return {"ids": P["top_ids"].numpy((B, k)), "scores": P["top_scores"].numpy((B, k)), "ranks": P["ranks"].numpy((B, T)),
                "tscores": P["target_scores"].numpy((B, T))}

    out = three_poisons(run, "the biased calls")[POISONS[0]]
    _same((out["ids"], out["scores"]), ref.topk(s, bias, ex, k), "biased top-k between guard bands")
    _same((out["ranks"], out["tscores"]), ref.ranks(s, bias, ex, tg), "biased rank between guard bands")


def test_engine_refuses_a_wrong_bias():
    user, items, ex, bias, tg, s = _real()
    eng = _engine()
    N = items.shape[0]
    for bad in (bias[:-1].contiguous(), bias.double(), bias.cpu(), bias.view(-1, 1), torch.zeros(2 * N, device=DEV)[::2]):
        with pytest.raises(_lib.NrmsError, match="bias"):
            eng.top_k(user, items, 10, ex, bias=bad)
        with pytest.raises(_lib.NrmsError, match="bias"):
            eng.rank_of(user, items, tg, ex, bias=bad)


# ---- 6: the models -----------------------------------------------------------------------------------------------------------
def _click_feed(N):
    """A hand-made click log over news ids (0, N) with a skewed popularity, as a ClickFeed on the device: 60 users of 6 .. 25
    clicks, the last one held out."""
    from pytorch_news_recommender_amd.data_handler import ClickFeed
    from tests.test_hip_mmr import _tiny_cfg
    cfg = _tiny_cfg("nrms_hip")
    rng = np.random.default_rng(N)
    lens = rng.integers(6, 26, size=60)
    w = 1.0 / np.arange(1, N) ** 0.9
    clicks = rng.choice(rng.permutation(np.arange(1, N)), size=int(lens.sum()), p=w / w.sum()).astype(np.int64)
    user_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    titles = {i: [1 + i % 7] for i in range(N - 1)}
    return ClickFeed(cfg, user_ptr, clicks, id2title_dict=titles, id2abst_dict=titles, batch_size=8, device=DEV)


@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_v1", "nrms_naml", "nrms_bert"])
def test_models_serve_and_rank_with_a_prior(kind):
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model(kind)
    N = cat.shape[0]
    feed = _click_feed(N)
    count = feed.count.cpu().numpy()
    p = feed.popularity_prior(0.5)
    assert tuple(p.shape) == (N,) and p.device == cat.device
    blocked = p.clone()
    rank1 = torch.arange(1, 21, dtype=torch.int32, device=DEV)
    for batch in batches:
        ids0, sc0 = model.recommend(batch, 20, cat)
        ids, sc = model.recommend(batch, 20, cat, item_bias=p)
        assert (ids > 0).all() and not torch.equal(ids, ids0)
        r, rs = model.rank_targets(batch, ids, cat, item_bias=p)                   # the served list ranks 1 .. k, same score bits
        assert torch.equal(r, rank1.expand_as(r)) and torch.equal(rs.view(torch.int32), sc.view(torch.int32))
        # the score is the plain score plus the prior, one fp32 add
        _, plain = model.rank_targets(batch, ids, cat)
        assert torch.equal((plain + p[ids]).view(torch.int32), sc.view(torch.int32))
        # diversity = 1 with a bias is the biased plain list, bit for bit
        for shortlist in (None, 20, 256):
            m_ids, m_sc = model.recommend(batch, 20, cat, diversity=1.0, shortlist=shortlist, item_bias=p)
            assert torch.equal(m_ids, ids) and torch.equal(m_sc.view(torch.int32), sc.view(torch.int32))
        d_ids, d_sc, ild = model.recommend(batch, 10, cat, diversity=0.5, item_bias=p, return_ild=True)
        s_ids, _ = model.recommend(batch, 40, cat, item_bias=p)                    # picked from the biased shortlist of 4 k
        assert all(set(d_ids[b].tolist()) <= set(s_ids[b].tolist()) for b in range(d_ids.shape[0]))
        # a NaN entry blocks that news for everybody; zeros are the call as it was
        blocked[ids[:, 0]] = float("nan")
        b_ids, _ = model.recommend(batch, 20, cat, item_bias=blocked)
        assert not torch.isin(b_ids, ids[:, 0]).any()
        assert (model.rank_targets(batch, ids[:, :1].contiguous(), cat, item_bias=blocked)[0] == 0).all()
        z_ids, z_sc = model.recommend(batch, 20, cat, item_bias=torch.zeros_like(p))
        assert torch.equal(z_ids, ids0) and torch.equal(z_sc.view(torch.int32), sc0.view(torch.int32))
    # a user without clicks gets the most-clicked news, in count order
    batch = dict(batches[0])
    batch["browsed_ids"] = torch.zeros_like(torch.as_tensor(batches[0]["browsed_ids"]).to(DEV))
    all_ids = torch.arange(1, N, device=DEV).expand(batch["browsed_ids"].shape[0], -1).contiguous()
    smax = float(model.rank_targets(batch, all_ids, cat)[1][0].abs().max())
    alpha = 1.0e5
    levels = np.unique(count[1:])
    gap = alpha * float(np.min(np.diff(np.log1p(levels.astype(np.float64)))))
    assert gap > 4 * smax + 1, (gap, smax)                                         # the prior decides between two counts, whatever the scores
    k = 30
    ids, _ = model.recommend(batch, k, cat, item_bias=feed.popularity_prior(alpha))
    got = count[ids[0].cpu().numpy()]
    assert (np.diff(got) <= 0).all() and got[0] == count[1:].max() and len(set(ids[0].tolist())) == k
    assert got[-1] >= np.sort(count[1:])[::-1][k - 1]                              # nothing more popular was left out
    plain_ids, _ = model.recommend(batch, k, cat)
    assert not torch.equal(plain_ids, ids)
    # a wrong prior is refused by name
    for bad in (p[:-1], p.double(), p.cpu(), p.view(1, -1)):
        with pytest.raises(_lib.NrmsError, match="item_bias"):
            model.recommend(batches[0], 5, cat, item_bias=bad)
        with pytest.raises(_lib.NrmsError, match="item_bias"):
            model.rank_targets(batches[0], ids[:, :1].contiguous(), cat, item_bias=bad)
    model.check_recommend_ids()


def test_hierec_and_graph_refuse_a_prior():
    from pytorch_news_recommender_amd import synth
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.data_handler import SyntheticMind
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    from tests.test_hip_mmr import _tiny_cfg
    cfg = _tiny_cfg("hierec")
    corpus = SyntheticMind(cfg, n_news=50, n_topics=4, seed=1)
    hier = hierec_hip.Model(cfg, pretrained_word_embedding=corpus.embedding_table(cfg.word_embed_size)).to("cuda")
    batch = {"browsed_ids": torch.zeros(2, cfg.history_len, dtype=torch.int64, device=DEV)}
    p = torch.zeros(51, device=DEV)
    shape = synth.G1_ODD
    gcfg = Config("graph")
    gcfg.__nrms__()
    gcfg.word_embed_size, gcfg.num_attention_heads, gcfg.query_vector_dim = shape.word_embed_size, shape.num_attention_heads, shape.query_vector_dim
    params = synth.make_params_graph(shape, seed=3)
    graph = graph_hip.Model(gcfg, pretrained_word_embedding=params["news_encoder.word_embedding.0.weight"]).to("cuda")
    for model in (hier, graph):
        with pytest.raises(_lib.NrmsError, match="item_bias"):
            model.recommend(batch, 5, None, item_bias=p)
        with pytest.raises(_lib.NrmsError, match="item_bias"):
            model.rank_targets(batch, torch.ones(2, 1, dtype=torch.int64, device=DEV), None, item_bias=p)
        # without it: what they said before
        with pytest.raises(_lib.NrmsError, match="diversity"):
            model.recommend(batch, 5, None, diversity=0.5)
        with pytest.raises(NotImplementedError):
            model.recommend(batch, 5, None)
        with pytest.raises(NotImplementedError, match="rank_targets"):
            model.rank_targets(batch, torch.ones(2, 1, dtype=torch.int64, device=DEV), None)
        assert not model.CATALOGUE_RANKING and not model.CATALOGUE_SAMPLING


# ---- 7: the CLI --------------------------------------------------------------------------------------------------------------
def test_run_v0_popularity_prior_flag(tmp_path):
    """A fresh child process with a time limit of its own; nothing is started after it."""
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "pytorch_news_recommender_amd.run_v0", "--model", "nrms_hip", "--dataset", "synthetic",
                        "--negatives", "catalogue", "--max_batches", "2", "--epochs", "1", "--synthetic_users", "128",
                        "--batch_size", "64", "--num_workers", "0", "--description", "T", "--data_path", str(tmp_path / "data"),
                        "--save_path", str(tmp_path / "save"), "--retrieval_metrics", "10", "--popularity_prior", "0.5"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("retrieval over")]
    assert len(line) == 1, r.stdout[-3000:]
    m = re.fullmatch(r"retrieval over 4000 news: recall@10: ([\d.]+)  ndcg@10: ([\d.]+)  mrr: ([\d.]+)  median rank: ([\d.]+)  "
                     r"users: (\d+)  targets: (\d+)  skipped: (\d+)", line[0])
    assert m, line[0]
    assert 0.0 <= float(m.group(1)) <= 1.0 and int(m.group(6)) >= int(m.group(5)) > 0
