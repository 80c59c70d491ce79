"""nrms_attribution_dot on the GPU (a score split over the clicks of the history, include/nrms_hip.h) against
tests/attribution_ref.py: bit for bit on lattice data, where every term and partial sum is exact in fp32; on Gaussian data the
terms against nrms_rank_dot's score bits, the total against the sequential fp32 sum and a derived float64 bound; independence of
a row from everything but its own inputs; invalid ids, NaN, signed zeros and unnamed slots; the buffer contract under guard
bands; and the layers built on it (NRMSEngine.user_parts / attribution, Model.explain) on small synthetic models."""
import ctypes as C

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, synth
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream

from tests import attribution_ref as ref
from tests.guarded import POISONS, Pool, assert_same_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
_ENG = []
U = 2.0 ** -24                      # fp32 unit roundoff
I64_MIN = -2 ** 63
NAMES = ("top_slots", "top_contrib", "total", "unnamed_share", "contrib")


def _engine():
    if not _ENG:
        _ENG.append(NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), DEV))
    return _ENG[0]


def _dev(x, dt):
    return torch.as_tensor(x).to(DEV, dtype=dt).contiguous()


def _call(ctx, w, items, ids, m, named=None, t_items=None):
    out = _engine().attribution(_dev(ctx, torch.float32), _dev(w, torch.float32),
                                _dev(items, torch.float32) if t_items is None else t_items, _dev(ids, torch.int64), m,
                                slot_named=None if named is None else _dev(named, torch.uint8), return_contrib=True)
    return {n: t.cpu().numpy() for n, t in zip(NAMES, out)}


def _same(got, want, what):
    """Equal bit for bit; a NaN matches any NaN."""
    for n in NAMES:
        a, b = got[n], want[n]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, n, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float32:
            na, nb = np.isnan(a), np.isnan(b)
            ok = np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
        else:
            ok = np.array_equal(a, b)
        if not ok:
            bad = np.argwhere((a != b) & ~(np.isnan(a) & np.isnan(b)) if a.dtype == np.float32 else a != b)
            raise AssertionError("%s: %s differs at %d places, first %s: got %r, want %r"
                                 % (what, n, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def _named(B, H, seed):
    """Most slots named, user 0 at most two (so m > #named occurs), the last user none."""
    rng = np.random.default_rng(seed)
    named = (rng.random((B, H)) < 0.7).astype(np.uint8)
    named[0] = 0
    named[0, rng.integers(0, H, 2)] = 1
    named[B - 1] = 0
    return named


# ---- 1: exact on lattice data ---------------------------------------------------------------------------------------------------
#        d,   K,   B, m, slot_named
COMBOS = [(1, 1, 1, 1, False), (7, 63, 33, 3, True), (8, 64, 1, 8, False), (31, 65, 1, 3, True), (32, 256, 1, 1, False),
          (33, 1, 33, 8, True), (64, 65, 33, 3, False), (300, 256, 1, 3, True)]


@pytest.mark.parametrize("H", [1, 31, 32, 33, 50, 64])
def test_lattice_data_bit_for_bit(H):
    """Every output equals the reference's, reasons inside runs of equal contributions included.  d = 1, 7, 31, 33 take the
    scalar loads (tk_vec_ok false), the others float4; m = 3, 8 exceed H = 1 and the two named slots of user 0."""
    for i, (d, K, B, m, with_named) in enumerate(COMBOS + ([(300, 256, 33, 3, True)] if H == 50 else [])):
        N = 97 + i
        ctx, w, items, ids = ref.lattice_case(B, H, d, K, N, seed=100 * H + i)
        assert ref.lattice_is_exact(ctx, w, items, ids)
        named = _named(B, H, i) if with_named else None
        want = ref.attribution(ctx, w, items, ids, m, named)
        _same(_call(ctx, w, items, ids, m, named), want, "H=%d d=%d K=%d B=%d m=%d" % (H, d, K, B, m))


def test_a_base_pointer_that_rules_out_float4_loads():
    """d = 8, but the catalogue starts 4 bytes past a 16-byte boundary: the scalar-load instantiation, the same bits."""
    B, H, d, K, N = 3, 50, 8, 70, 120
    ctx, w, items, ids = ref.lattice_case(B, H, d, K, N, seed=7)
    flat = torch.empty(N * d + 1, dtype=torch.float32, device=DEV)
    off = flat[1:].view(N, d)
    off.copy_(torch.from_numpy(items))
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    got = _call(ctx, w, items, ids, 3, t_items=off)
    _same(got, ref.attribution(ctx, w, items, ids, 3), "offset catalogue")
    _same(got, _call(ctx, w, items, ids, 3), "offset against aligned")


# ---- 2: Gaussian data -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,d,K,N", [(3, 50, 300, 65, 500), (2, 33, 60, 10, 200), (1, 64, 7, 64, 90)])
def test_gaussian_terms_are_rank_dot_scores_times_w(B, H, d, K, N):
    rng = np.random.default_rng(B * 1000 + H)
    ctx = rng.standard_normal((B, H, d)).astype(np.float32)
    w = rng.standard_normal((B, H)).astype(np.float32)
    items = rng.standard_normal((N, d)).astype(np.float32)
    ids = rng.integers(0, N, (B, K)).astype(np.int64)
    got = _call(ctx, w, items, ids, 3)
    # the chain's score of (ctx row, item row), from the call that ranks: every ctx row as a user of its own
    eng = _engine()
    targets = np.repeat(ids[:, None, :], H, axis=1).reshape(B * H, K)
    _, s = eng.rank_of(_dev(ctx.reshape(B * H, d), torch.float32), _dev(items, torch.float32), _dev(targets, torch.int64))
    s = s.cpu().numpy().reshape(B, H, K).transpose(0, 2, 1)                      # [B, K, H]
    assert np.isfinite(s).all()
    want_c = (w[:, None, :] * s).astype(np.float32)                              # one float32 multiply
    assert got["contrib"].tobytes() == want_c.tobytes()
    assert got["total"].tobytes() == ref.seq_sum32(got["contrib"]).tobytes()
    _same(got, ref.finish(got["contrib"], ids, N, 3), "everything after the terms")
    # against float64: the forward bound of a d-term dot product, one multiply and an H-term sum (derived, not tuned)
    c64 = ref.terms64(ctx, w, items, ids)
    err = np.abs(got["total"].astype(np.float64) - c64.sum(-1))
    bound = ref.bound(ctx, w, items, ids)
    print("B=%d H=%d d=%d K=%d: max |total - f64| = %.3e, max err / bound = %.3f" % (B, H, d, K, err.max(), (err / bound).max()))
    assert (err <= bound).all()


# ---- 3: a row depends on its own inputs only --------------------------------------------------------------------------------------
def test_row_bits_do_not_depend_on_the_batch_the_position_or_the_call_before():
    rng = np.random.default_rng(3)
    H, d, N = 50, 60, 400
    items = rng.standard_normal((N, d)).astype(np.float32)
    ctx1 = rng.standard_normal((1, H, d)).astype(np.float32)
    w1 = rng.standard_normal((1, H)).astype(np.float32)
    item = 123
    base = _call(ctx1, w1, items, np.array([[item]]), 3)
    row = lambda r, b, j: {n: r[n][b, j] for n in NAMES}

    def check(r, b, j, what):
        for n in NAMES:
            assert row(r, b, j)[n].tobytes() == row(base, 0, 0)[n].tobytes(), (what, n)

    # inside B = 33, at list positions 0 and 255 of K = 256, other ids around it
    ctx = rng.standard_normal((33, H, d)).astype(np.float32)
    w = rng.standard_normal((33, H)).astype(np.float32)
    ctx[17], w[17] = ctx1[0], w1[0]
    ids = rng.integers(0, N, (33, 256)).astype(np.int64)
    ids[17, 0] = ids[17, 255] = item
    ids[17, 100] = -1
    big = _call(ctx, w, items, ids, 3)
    check(big, 17, 0, "B = 33, position 0")
    check(big, 17, 255, "B = 33, position 255")
    # another K, after a call with other shapes, and with the engine's workspace poisoned
    ids65 = rng.integers(0, N, (1, 65)).astype(np.int64)
    ids65[0, 64] = item
    check(_call(ctx1, w1, items, ids65, 3), 0, 64, "K = 65, position 64")
    _call(rng.standard_normal((2, 7, 9)).astype(np.float32), np.ones((2, 7), dtype=np.float32),
          rng.standard_normal((5, 9)).astype(np.float32), np.zeros((2, 4), dtype=np.int64), 8)
    _engine()._bufs["attribution_ws"].fill_(-1)
    check(_call(ctx1, w1, items, np.array([[item]]), 3), 0, 0, "after other shapes, poisoned workspace")
    # m changes how many reasons are listed, not which
    m8 = _call(ctx1, w1, items, np.array([[item]]), 8)
    assert m8["top_slots"][0, 0, :3].tolist() == base["top_slots"][0, 0].tolist()
    assert m8["contrib"].tobytes() == base["contrib"].tobytes() and m8["total"].tobytes() == base["total"].tobytes()
    # two runs
    again = _call(ctx, w, items, ids, 3)
    for n in NAMES:
        assert again[n].tobytes() == big[n].tobytes(), n


# ---- 4: edges ---------------------------------------------------------------------------------------------------------------------
def test_invalid_ids_duplicates_empty_catalogue_and_empty_batch():
    B, H, d, K, N = 2, 33, 20, 8, 50
    ctx, w, items, _ = ref.lattice_case(B, H, d, K, N, seed=1)
    ids = np.array([[-1, N, I64_MIN, 7, 7, N - 1, 0, 2 ** 40], [3, -1, -1, 3, N + 5, 3, -7, 49]], dtype=np.int64)
    got = _call(ctx, w, items, ids, 3, _named(B, H, 0))
    _same(got, ref.attribution(ctx, w, items, ids, 3, _named(B, H, 0)), "invalid ids")
    bad = ~ref.valid_ids(ids, N)
    assert (got["total"][bad] == -np.inf).all() and (got["top_slots"][bad] == -1).all() and (got["top_contrib"][bad] == -np.inf).all()
    assert not got["contrib"][bad].any() and not got["unnamed_share"][bad].any()
    for n in NAMES:                                                      # an id that occurs twice: two entries, the same bits
        assert got[n][0, 3].tobytes() == got[n][0, 4].tobytes() and got[n][1, 0].tobytes() == got[n][1, 5].tobytes()
    # N = 0: every entry is invalid, no item row exists
    none = _call(ctx, w, np.zeros((0, d), dtype=np.float32), ids, 3)
    _same(none, ref.attribution(ctx, w, np.zeros((0, d), dtype=np.float32), ids, 3), "N = 0")
    assert (none["total"] == -np.inf).all()
    # B = 0: a no-op
    empty = _call(ctx[:0], w[:0], items, ids[:0], 3)
    assert [empty[n].shape for n in NAMES] == [(0, K, 3), (0, K, 3), (0, K), (0, K), (0, K, H)]


def test_nan_makes_a_slot_ineligible_and_the_total_nan():
    B, H, d, K, N = 2, 50, 33, 9, 40
    ctx, w, items, ids = ref.lattice_case(B, H, d, K, N, seed=2, ties=False)
    ids[:] = np.arange(1, K + 1)
    ctx[0, 5, 17] = np.nan                                               # one ctx row of user 0
    w[1, 40] = np.nan                                                    # one weight of user 1
    items[4, 0] = np.nan                                                 # one item row, position 3 of both lists
    named = np.ones((B, H), dtype=np.uint8)
    named[1, 40] = 0                                                     # user 1's NaN slot is unnamed: its share is NaN
    got = _call(ctx, w, items, ids, 8, named)
    _same(got, ref.attribution(ctx, w, items, ids, 8, named), "NaN")
    assert np.isnan(got["total"]).all()
    assert np.isnan(got["contrib"][0, :, 5]).all() and np.isnan(got["contrib"][1, :, 40]).all() and np.isnan(got["contrib"][:, 3]).all()
    assert not (got["top_slots"][0] == 5).any() and not (got["top_slots"][1] == 40).any()
    assert (got["top_slots"][:, 3] == -1).all() and (got["top_contrib"][:, 3] == -np.inf).all()
    others = np.delete(np.arange(K), 3)
    assert (got["top_slots"][:, others] >= 0).all() and not np.isnan(got["top_contrib"][:, others]).any()
    assert not np.isnan(got["unnamed_share"][0]).any() and np.isnan(got["unnamed_share"][1]).all()


def test_signed_zeros_and_all_slots_unnamed():
    B, H, d, K, N = 1, 8, 4, 2, 3
    ctx = np.zeros((B, H, d), dtype=np.float32)
    ctx[0, 2, 0], ctx[0, 6, 0] = 1.0, -1.0
    w = np.array([[1, -1, 0.5, -0.0, 1, -1, 0.5, 1]], dtype=np.float32)
    items = np.array([[0, 0, 0, 0], [2, 0, 0, 0], [0, 5, 0, 0]], dtype=np.float32)
    ids = np.array([[1, 2]])
    got = _call(ctx, w, items, ids, 8)
    want = ref.attribution(ctx, w, items, ids, 8)
    _same(got, want, "signed zeros")
    # item 2 meets only zero dot products: terms +0.0 and -0.0 by the sign of w, one run of eight equal values in slot order
    assert np.signbit(got["contrib"][0, 1]).tolist() == [False, True, False, True, False, True, False, False]
    assert got["top_slots"][0, 1].tolist() == list(range(8)) and not np.signbit(got["top_contrib"][0, 1]).any()
    assert got["top_slots"][0, 0].tolist() == [2, 0, 1, 3, 4, 5, 7, 6]
    zero = np.zeros((B, H), dtype=np.uint8)
    un = _call(ctx, w, items, ids, 3, zero)
    _same(un, ref.attribution(ctx, w, items, ids, 3, zero), "no slot named")
    assert (un["top_slots"] == -1).all() and un["unnamed_share"].tobytes() == un["total"].tobytes()
    ctx2, w2, items2, ids2 = ref.lattice_case(4, 50, 31, 70, 60, seed=9)
    un = _call(ctx2, w2, items2, ids2, 3, np.zeros((4, 50), dtype=np.uint8))
    assert (un["top_slots"] == -1).all() and (un["top_contrib"] == -np.inf).all()
    ok = ref.valid_ids(ids2, 60)
    assert un["unnamed_share"][ok].tobytes() == un["total"][ok].tobytes() and not un["unnamed_share"][~ok].any()


# ---- 5: the buffer contract -------------------------------------------------------------------------------------------------------
def test_outputs_and_workspace_between_guard_bands():
    lib = _lib.load()
    B, H, d, K, N, m = 5, 50, 36, 70, 80, 3
    ctx, w, items, ids = ref.lattice_case(B, H, d, K, N, seed=11)
    named = _named(B, H, 1)
    want = ref.attribution(ctx, w, items, ids, m, named)
    nbytes = lib.nrms_attribution_dot_workspace_bytes(B, H, d, K, m)
    assert nbytes > 0
    f32, i32, i64, u8 = torch.float32, torch.int32, torch.int64, torch.uint8
    runs = {}
    for poison in POISONS:
        pool = Pool(poison)
        for name, n, dt, init in (("ctx", B * H * d, f32, ctx), ("w", B * H, f32, w), ("items", N * d, f32, items), ("ids", B * K, i64, ids),
                                  ("named", B * H, u8, named)):
            pool.elems(name, n, dt, init=torch.from_numpy(np.ascontiguousarray(init)).reshape(-1))
        for name, n, dt in (("contrib", B * K * H, f32), ("total", B * K, f32), ("top_slots", B * K * m, i32),
                            ("top_contrib", B * K * m, f32), ("unnamed_share", B * K, f32)):
            pool.elems(name, n, dt)
        pool.new("ws", nbytes)
        inputs = {n: pool[n].snapshot() for n in ("ctx", "w", "items", "ids", "named")}
        rc = lib.nrms_attribution_dot(B, H, C.c_int64(N), d, K, m, pool["ctx"].ptr, pool["w"].ptr, pool["items"].ptr, pool["ids"].ptr,
                                      pool["named"].ptr, pool["contrib"].ptr, pool["total"].ptr, pool["top_slots"].ptr,
                                      pool["top_contrib"].ptr, pool["unnamed_share"].ptr, pool["ws"].ptr, C.c_size_t(nbytes), _stream())
        _lib.check(rc, "nrms_attribution_dot")
        pool.intact("nrms_attribution_dot")
        for n, snap in inputs.items():
            assert pool[n].unchanged_since(snap), n
        got = {"contrib": pool["contrib"].numpy((B, K, H)), "total": pool["total"].numpy((B, K)),
               "top_slots": pool["top_slots"].numpy((B, K, m)), "top_contrib": pool["top_contrib"].numpy((B, K, m)),
               "unnamed_share": pool["unnamed_share"].numpy((B, K))}
        _same(got, want, "guarded, poison 0x%02X" % poison)
        runs[poison] = got
        # the nullable arguments as NULL: the required outputs keep their bits, nothing else is written
        pool2 = Pool(poison)
        for name, n, dt in (("total", B * K, f32), ("top_slots", B * K * m, i32), ("top_contrib", B * K * m, f32)):
            pool2.elems(name, n, dt)
        pool2.new("ws", nbytes)
        rc = lib.nrms_attribution_dot(B, H, C.c_int64(N), d, K, m, pool["ctx"].ptr, pool["w"].ptr, pool["items"].ptr, pool["ids"].ptr,
                                      None, None, pool2["total"].ptr, pool2["top_slots"].ptr, pool2["top_contrib"].ptr, None,
                                      pool2["ws"].ptr, C.c_size_t(nbytes), _stream())
        _lib.check(rc, "nrms_attribution_dot")
        pool2.intact("nrms_attribution_dot without the nullable arguments")
        pool.intact("the second call")
        all_named = ref.attribution(ctx, w, items, ids, m)
        assert pool2["total"].numpy((B, K)).tobytes() == got["total"].tobytes() == all_named["total"].tobytes()
        assert np.array_equal(pool2["top_slots"].numpy((B, K, m)), all_named["top_slots"])
    assert_same_bits(runs, "nrms_attribution_dot")
    # an undersized workspace is refused with its own code, before any launch
    pool = Pool(0xFF)
    pool.new("ws", nbytes)
    rc = lib.nrms_attribution_dot(B, H, C.c_int64(N), d, K, m, pool["ws"].ptr, pool["ws"].ptr, pool["ws"].ptr, pool["ws"].ptr, None, None,
                                  pool["ws"].ptr, pool["ws"].ptr, pool["ws"].ptr, None, pool["ws"].ptr, C.c_size_t(nbytes - 1), _stream())
    assert rc == _lib.NRMS_EWORKSPACE and lib.nrms_last_error().startswith(b"attribution_dot: workspace")
    eng = _engine()
    t = lambda a, dt: _dev(a, dt)
    for kw, word in ((dict(m=0), "m="), (dict(m=9), "m="), (dict(ids=t(ids[:, :0], i64)), "K="), (dict(ids=t(ids[:2], i64)), "ids"),
                     (dict(w=t(w[:, :7], f32)), "w"), (dict(ids=t(ids, i64).to(torch.int32)), "ids"),
                     (dict(slot_named=t(named[:, :9], u8)), "slot_named")):
        args = dict(ctx=t(ctx, f32), w=t(w, f32), items=t(items, f32), ids=t(ids, i64), m=3)
        args.update(kw)
        with pytest.raises(_lib.NrmsError, match="attribution: .*" + word):
            eng.attribution(**args)


# ---- 6: the model level -----------------------------------------------------------------------------------------------------------
def _v0(H=50, B=5, N=200, precision=None):
    """A small nrms_v0 (d = 60, 6 heads: at H = 50 the user encoder is the fused one-kernel pass), a catalogue of N news and a
    batch whose histories end in padding slots (user 0: 3 clicks; the last user: a full history)."""
    from tests.test_hip_mmr import _tiny_cfg
    from pytorch_news_recommender_amd.model.nrms_hip import Model
    torch.manual_seed(0)
    cfg = _tiny_cfg("nrms_v0")
    cfg.history_len, cfg.dropout = H, 0.2
    if precision:
        cfg.precision = precision
    rng = np.random.default_rng(21)
    table = (0.3 * rng.standard_normal((cfg.n_words, cfg.word_embed_size))).astype(np.float32)
    table[0] = 0
    model = Model(cfg, pretrained_word_embedding=table).to("cuda")
    titles = rng.integers(1, cfg.n_words, (N, cfg.n_words_title))
    titles[:, 8:] *= rng.random((N, cfg.n_words_title - 8)) < 0.5
    titles[0] = 0
    browsed = rng.integers(1, N, (B, H))
    for b, n in enumerate(np.linspace(3, H, B).astype(int)):
        browsed[b, n:] = 0
    t_titles = torch.from_numpy(titles).to(DEV)
    return cfg, model, {"browsed_ids": torch.from_numpy(browsed).to(DEV)}, model.encode_catalogue(t_titles), t_titles


def _check_explanation(model, batch, cat, ids, scores, what, masked):
    B, K = ids.shape
    browsed = batch["browsed_ids"].cpu().numpy()
    H = browsed.shape[1]
    r_ids, r_c, total, pad, contrib = (t.cpu().numpy() for t in model.explain(batch, ids, cat, 3, return_contributions=True))
    assert r_ids.shape == (B, K, 3) and r_ids.dtype == np.int64 and contrib.shape == (B, K, H)
    n_ids = ids.cpu().numpy()
    live = n_ids >= 0
    assert live.any() and (total[~live] == -np.inf).all() and (r_ids[~live] == -1).all()
    for b in range(B):
        got = set(r_ids[b][live[b]].reshape(-1).tolist()) - {-1}
        assert got <= set(browsed[b].tolist()) - {0}, (what, b)                         # the user's own clicks, never the padding id
        n_named = int((browsed[b] != 0).sum())
        assert ((r_ids[b][live[b]] >= 0).sum(-1) == min(3, n_named)).all()
    # total = the reasons + the rest, consistently with contrib: the named part and the padding share are sums over disjoint slots
    named = browsed != 0
    assert total[live].tobytes() == ref.seq_sum32(contrib)[live].tobytes()
    for b in range(B):
        assert pad[b][live[b]].tobytes() == ref.seq_sum32(contrib[b][:, ~named[b]])[live[b]].tobytes()
        order = np.argsort(-np.where(named[b][None, :], contrib[b], -np.inf), axis=-1, kind="stable")[:, :3]
        want = np.take_along_axis(contrib[b], order, -1)
        have = min(3, int(named[b].sum()))
        assert np.array_equal(r_c[b][live[b]][:, :have], want[live[b]][:, :have])
    has_pad = (~named).any(-1)
    if masked:
        # a masked slot has weight 0 from the encoder itself; only a history with no click at all, whose softmax over equal
        # masked logits is uniform, is carried by its padding slots, and then entirely
        some = named.any(-1)
        assert some.any() and not some.all()
        for b in range(B):
            if some[b]:
                assert not contrib[b][:, ~named[b]].any() and not pad[b][live[b]].any()
            else:
                assert pad[b][live[b]].tobytes() == total[b][live[b]].tobytes() and (r_ids[b] == -1).all()
    else:                                                                # nrms_v0 masks nothing: the padding slots carry score
        assert has_pad.any() and all((pad[b][live[b]] != 0).any() for b in np.nonzero(has_pad)[0])
        assert not pad[~has_pad].any()
    # against user_parts' own user . x in float64: the bound of the split sum plus (H + 1) u sum |w| |ctx| |x| for the pooling
    # sum that formed `user`
    hist = cat.index_select(0, batch["browsed_ids"].view(-1)).view(B, H, -1)
    user, ctx, w = model._catalogue_user_parts(hist, batch["browsed_ids"])
    user64, ctx, w, cat64 = user.double().cpu().numpy(), ctx.cpu().numpy(), w.cpu().numpy(), cat.double().cpu().numpy()
    safe = np.where(live, n_ids, 0)
    ux = np.einsum("bd,bkd->bk", user64, cat64[safe])
    d = cat.shape[1]
    mag = ref.bound(ctx, w, cat.cpu().numpy(), n_ids) / ((d + H + 2) * U)
    err = np.abs(total.astype(np.float64) - ux)[live]
    bound = ((d + H + 2) + (H + 1)) * U * mag[live]
    # the terms are those of user_parts' own factors: a d-term dot product and one multiply per term
    t_err = np.abs(contrib.astype(np.float64) - ref.terms64(ctx, w, cat.cpu().numpy(), n_ids))
    assert (t_err <= (d + 1) * U * ref.terms64(np.abs(ctx), np.abs(w), np.abs(cat.cpu().numpy()), n_ids)).all()
    dscore = np.abs(total[live] - scores.cpu().numpy()[live])
    print("%s: max |total - user.x| = %.3e (max err / bound %.3f); max |total - recommend's score| = %.3e, relative to "
          "sum |terms| %.3e" % (what, err.max(), (err / bound).max(), dscore.max(), (dscore / mag[live]).max()))
    assert (err <= bound).all()
    return user


def test_explain_on_recommends_own_ids_v0():
    cfg, model, batch, cat, _ = _v0()
    ids, scores = model.recommend(batch, 20, cat)
    user = _check_explanation(model, batch, cat, ids, scores, "nrms_v0 H=50 (fused user encoder)", masked=False)
    # user_parts runs recommend's own pass: the same user vector, bit for bit
    q_user, _, _ = model._catalogue_query(batch, cat, True, "recommend")
    assert torch.equal(user.view(torch.int32), q_user.view(torch.int32))
    # the re-ranked list and a padded list are explained the same way; K = 256 is the limit
    d_ids, d_scores = model.recommend(batch, 10, cat, diversity=0.5)
    _check_explanation(model, batch, cat, d_ids, d_scores, "nrms_v0, diversity 0.5", masked=False)
    few = model.recommend(batch, 256, cat)
    assert (few[0][:, -1] == -1).all()                                   # 199 news: the lists end in padding
    _check_explanation(model, batch, cat, few[0], few[1], "nrms_v0, K = 256 with padding", masked=False)
    with pytest.raises(_lib.NrmsError, match="K=257"):
        model.explain(batch, torch.zeros(5, 257, dtype=torch.int64, device=DEV), cat)
    with pytest.raises(_lib.NrmsError, match="news_ids"):
        model.explain(batch, ids[:3], cat)
    # browsed ids outside the catalogue are counted and read as padding, as in recommend
    odd = {"browsed_ids": batch["browsed_ids"].clone()}
    odd["browsed_ids"][0, 0] = 10 ** 6
    r = model.explain(odd, ids, cat)
    assert not (r[0] == 10 ** 6).any()
    with pytest.raises(_lib.NrmsError, match="1 browsed_ids outside the catalogue"):
        model.check_recommend_ids()


def test_explain_short_history_takes_the_chain():
    """H = 20 is outside the fused kernel's shapes: the GEMM -> attention -> additive chain leaves ctx and w the same way."""
    cfg, model, batch, cat, _ = _v0(H=20)
    ids, scores = model.recommend(batch, 10, cat)
    _check_explanation(model, batch, cat, ids, scores, "nrms_v0 H=20 (chain)", masked=False)


def test_explain_masked_history_bert():
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model("nrms_bert")
    batch = batches[0]
    ids, scores = model.recommend(batch, 10, cat)
    _check_explanation(model, batch, cat, ids, scores, "nrms_bert (masked history)", masked=True)


def test_hierec_and_graph_refuse():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    for mod, word in ((hierec_hip, "hierec"), (graph_hip, "graph")):
        with pytest.raises(NotImplementedError, match=word + ": explain is not available: "):
            mod.Model.explain(None, {}, None, None)


def test_explain_between_a_training_forward_and_its_backward():
    """What an engine may remember (tests/test_hip_history.py): an explain call between a training forward and its backward runs
    on buffers of its own, so the step's gradients keep their bits; so do an eval forward's scores around it."""
    shape = synth.Shape(n_words=600, word_embed_size=60, num_attention_heads=6, query_vector_dim=32, batch_size=5, history_len=50,
                        n_candidates=4, n_words_title=12)
    raw = synth.make_batch(shape, seed=4)
    grads = {}
    for precision in ("bf16x3", "fp16"):
        for twin in (False, True):
            cfg, model, ebatch, cat, _ = _v0(precision=precision)
            model.train()
            tb = {k: torch.from_numpy(v).to(DEV) for k, v in raw.items()}
            scores = model(tb)
            if not twin:
                ids, _ = model.recommend(ebatch, 10, cat)
                first = model.explain(ebatch, ids, cat, 3, return_contributions=True)
                again = model.explain(ebatch, ids, cat, 3, return_contributions=True)
                for a, b in zip(first, again):
                    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
            torch.nn.functional.cross_entropy(scores, torch.zeros(len(scores), dtype=torch.long, device=DEV)).backward()
            torch.cuda.synchronize()
            grads[(precision, twin)] = {n: p.grad.cpu().numpy().copy() for n, p in model.named_parameters() if p.grad is not None}
        a, b = grads[(precision, False)], grads[(precision, True)]
        assert a.keys() == b.keys() and len(a) >= 10
        assert any(np.abs(g).max() > 0 for g in a.values())
        for n in a:
            assert a[n].tobytes() == b[n].tobytes(), "%s: %s changed by an explain call before the backward" % (precision, n)
