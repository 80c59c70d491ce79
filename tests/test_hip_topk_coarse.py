"""The fp16 shortlist with a certificate on the GPU (include/nrms_hip.h nrms_catalogue_pack_f16 / nrms_topk_dot_coarse) against
tests/topk_coarse_ref.py and against nrms_topk_dot itself.  Every comparison is exact unless stated.

Measured on an MI355X (see DESIGN.md section 8h for the figures): the accumulation test prints its largest ratio
|short_score - float64(u16 . n16)| / (alpha_d ||u16|| ||n16||), the Gaussian and near-tied tests their smallest / largest margin, the
graded, M = k and out-of-range tests their certified share, the smallest |margin - 1| and the rows that differ from nrms_topk_dot."""
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
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, PackedCatalogue, _stream

from tests import topk_coarse_ref as ref
from tests.guarded import Pool

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
F = np.float32
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
    for g, w, name in zip(got, want, ("scores", "ids", "third", "fourth", "fifth")):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg="%s (%s)" % (what, name))


def _coarse(user, items, k, M, ex=None, packed=None):
    """-> (scores, ids, certified, short_scores, short_ids, packed) through the engine."""
    eng = _engine()
    packed = eng.pack_catalogue(items) if packed is None else packed
    return eng.top_k_coarse(user, packed, k, M, ex, return_shortlist=True) + (packed,)


# ---- 1: pack -------------------------------------------------------------------------------------------------------------------
def _raw_pack(items, poison):
    lib = _lib.load()
    N, d = items.shape
    pitch = lib.nrms_catalogue_f16_pitch(d)
    pool = Pool(poison)
    src = pool.elems("items", N * d, torch.float32, init=torch.from_numpy(items) if N else "zero")
    dst = pool.elems("items16", N * pitch, torch.int16)
    st = pool.elems("stats", 2, torch.float32)
    _lib.check(lib.nrms_catalogue_pack_f16(C.c_int64(N), d, src.ptr, dst.ptr, st.ptr, _stream()), "nrms_catalogue_pack_f16")
    pool.intact("nrms_catalogue_pack_f16")
    return dst.numpy((N, pitch)).view(np.uint16), st.numpy()


def _pack_data(N, d, kind, seed):
    rng = np.random.default_rng(seed)
    items = (rng.normal(size=(N, d)) * 10.0 ** rng.integers(-7, 6, size=(N, 1))).astype(F)
    special = np.array([0.0, -0.0, 2.0 ** -14, np.nextafter(F(2.0 ** -14), F(0)), -np.nextafter(F(2.0 ** -14), F(0)), 65504.0, 65519.9,
                        65520.0, -65520.0, 1e30, -1e30, 6.1e-5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], dtype=F)
    flat = items.reshape(-1)
    if flat.size:
        at = rng.integers(0, flat.size, size=min(flat.size, 4 * len(special)))
        flat[at] = special[np.arange(len(at)) % len(special)]
    if kind == "nonfinite" and N >= 2:
        items[0, d // 2] = np.nan
        items[N - 1, 0] = -np.inf
    return items


@pytest.mark.parametrize("d", [1, 7, 31, 32, 33, 300])
@pytest.mark.parametrize("N", [0, 1, 33, 1000])
def test_pack_bits_and_stats(N, d):
    for kind in ("finite", "nonfinite"):
        items = _pack_data(N, d, kind, seed=N + d)
        want_bits, want_stats = ref.pack(items)
        bits, stats = _raw_pack(items, 0xFF)
        np.testing.assert_array_equal(bits, want_bits)
        nrm, err = ref.true_stats(items)
        if kind == "nonfinite" and N >= 2:
            assert stats[0] == np.inf
        else:
            assert nrm <= stats[0] <= nrm * (1 + 1e-6), (stats[0], nrm)
        assert err <= stats[1] <= err * (1 + 1e-6), (stats[1], err)
        assert N > 0 or stats.tolist() == [0.0, 0.0]
        bits2, stats2 = _raw_pack(items, 0x7F)                        # a second run, other poison: bit-identical
        assert bits2.tobytes() == bits.tobytes() and stats2.tobytes() == stats.tobytes()


# ---- 2: lattice data -----------------------------------------------------------------------------------------------------------
# every value of B, N (relative to M and to the slice length 2048), d, (k, M) and n_exclude the contract names, each at least once
LATTICE = [
    # B, N, d, k, M, n_ex      (N: "M-1", "M", "M+1" are resolved against M)
    (1, 0, 8, 1, 1, 0), (31, 1, 1, 1, 1, 3), (33, "M-1", 33, 1, 8, 0), (70, "M", 40, 1, 8, 64), (1, "M+1", 300, 1, 8, 65),
    (31, 2047, 8, 5, 16, 3), (33, 2049, 33, 5, 16, 0), (70, 4100, 40, 5, 16, 65), (1, "M-1", 1, 10, 64, 3), (33, "M", 300, 10, 64, 0),
    (31, "M+1", 8, 10, 64, 64), (70, 2047, 300, 10, 64, 3), (33, 4100, 33, 10, 64, 65), (31, 2049, 40, 100, 192, 0),
    (33, "M-1", 8, 100, 192, 3), (70, 4100, 33, 100, 192, 64), (33, "M+1", 40, 100, 193, 3), (31, 2047, 1, 100, 193, 0),
    (70, 2049, 8, 100, 193, 65), (1, 0, 300, 256, 256, 3), (33, "M", 8, 256, 256, 0), (31, "M+1", 33, 256, 256, 64),
    (70, 4100, 40, 256, 256, 3), (33, 1, 300, 5, 16, 65),
    # whole superblocks of 64 halves and a last block of 32 (pitch 96, 96, 160): the slice kernel's two k loops in one row
    (33, 2049, 65, 5, 16, 65), (70, 4100, 96, 256, 256, 3), (31, "M", 150, 10, 64, 0), (1, 2047, 150, 100, 193, 64), (33, "M+1", 96, 1, 8, 3),
]


@pytest.mark.parametrize("B,N,d,k,M,n_ex", LATTICE)
def test_exact_on_lattice_data(B, N, d, k, M, n_ex):
    """Integers in [-3, 3] are exact in fp16, so coarse and exact scores are the same fp32 numbers: the shortlist is nrms_topk_dot at
    k = M, and every row, certified or not, is nrms_topk_dot at k (the shortlist is a prefix of the true order)."""
    N = {"M-1": M - 1, "M": M, "M+1": M + 1}.get(N, N)
    rng = np.random.default_rng(1000 * B + N + d)
    user = _t(rng.integers(-3, 4, size=(B, d)), torch.float32)
    items = _t(rng.integers(-3, 4, size=(N, d)), torch.float32)
    ex = None
    if n_ex:
        e = rng.integers(-1, N + 1, size=(B, n_ex))                   # -1 and N among them
        e[:, -1] = e[:, 0]                                            # a duplicate
        ex = _t(e, torch.int64)
    eng = _engine()
    sc, ids, cert, ssc, sid, _ = _coarse(user, items, k, M, ex)
    _same((ssc, sid), eng.top_k(user, items, M, ex), "the shortlist is nrms_topk_dot at k = M")
    _same((sc, ids), eng.top_k(user, items, k, ex), "every row is nrms_topk_dot at k")
    L = (sid >= 0).sum(dim=1)
    assert (cert[L < M] == 1).all() and set(cert.unique().tolist()) <= {0, 1}
    if ex is not None and N:
        assert not (sid.unsqueeze(2) == ex.clamp(min=0).unsqueeze(1)).logical_and(ex.unsqueeze(1) >= 0).any()


# ---- 3: the accumulation assumption ----------------------------------------------------------------------------------------------
def _spread(rng, n, d):
    """Magnitudes spread over 2^+-12 and heavy cancellation: pairs of nearly opposite large terms around small ones."""
    x = rng.normal(size=(n, d)) * 2.0 ** rng.integers(-12, 13, size=(n, d))
    x[:, 1::2] = -x[:, 0::2][:, :x[:, 1::2].shape[1]] * (1 + 1e-3 * rng.normal(size=x[:, 1::2].shape))
    return x.astype(F)


@pytest.mark.parametrize("d", [16, 80, 300, 416, 1024])
@pytest.mark.parametrize("kind", ["gaussian", "spread"])
def test_fp16_mfma_accumulation_is_within_alpha(kind, d):
    rng = np.random.default_rng(d)
    B, N, M = 33, 1500, 64
    if kind == "gaussian":
        user, items = rng.normal(size=(B, d)).astype(F), rng.normal(size=(N, d)).astype(F)
    else:
        user, items = _spread(rng, B, d), _spread(rng, N, d)
        if d > 1:
            user[:, 1::2] = user[:, 0::2][:, :user[:, 1::2].shape[1]]      # ... so that the item's pairs cancel in the product
    _, _, _, ssc, sid, _ = _coarse(_t(user, torch.float32), _t(items, torch.float32), 1, M)
    ssc, sid = ssc.cpu().numpy().astype(np.float64), sid.cpu().numpy()
    u16 = ref.halves(ref.pack_rows(user)[0], d)
    n16 = ref.halves(ref.pack_rows(items)[0], d)
    assert (sid >= 0).all()
    worst = 0.0
    for b in range(B):
        rows = n16[sid[b]]
        true = rows @ u16[b]
        bound = ref.alpha(d) * np.linalg.norm(u16[b]) * np.linalg.norm(rows, axis=1)
        worst = max(worst, float((np.abs(ssc[b] - true) / bound).max()))
    print("alpha ratio %s d=%d: %.3e" % (kind, d, worst))
    assert worst <= 1.0, worst


# ---- 4 and 5: Gaussian and near-tied data -----------------------------------------------------------------------------------------
SHAPES = [(33, 2500, 40, 5, 64), (33, 2500, 300, 10, 64), (70, 5000, 300, 10, 64), (33, 2500, 40, 5, 16), (33, 2500, 44, 100, 192),
          (33, 2500, 300, 1, 8), (33, 2500, 80, 5, 64), (33, 2500, 400, 10, 64)]


def _margins(user, items, k, M, out):
    """The restatement's certificate from the GPU's own shortlist and exact scores."""
    sc, ids, cert, ssc, sid, packed = out
    unorm = ref.pack_rows(user)[2]
    return ref.certificate(user.shape[1], k, M, unorm, packed.stats.cpu().numpy(), sid.cpu().numpy(), ssc.cpu().numpy(), sc.cpu().numpy())


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("B,N,d,k,M", SHAPES)
def test_gaussian_rows_are_certified_and_exact(B, N, d, k, M, seed):
    rng = np.random.default_rng(seed)
    user, items = rng.standard_normal((B, d)).astype(F), rng.standard_normal((N, d)).astype(F)
    tu, ti = _t(user, torch.float32), _t(items, torch.float32)
    out = _coarse(tu, ti, k, M)
    want_cert, margin = _margins(user, items, k, M, out)
    print("gaussian margin min %.1f" % np.nanmin(margin))
    assert (out[2] == 1).all() and want_cert.all()
    _same(out[:2], _engine().top_k(tu, ti, k), "a certified row is nrms_topk_dot's")


@functools.lru_cache(maxsize=None)
def _near_tied(B, N, d, seed):
    return ref.near_tied(B, N, d, seed)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("B,N,d,k,M", SHAPES)
def test_near_tied_rows_are_not_certified(B, N, d, k, M, seed):
    user, items = _near_tied(B, N, d, seed)
    tu, ti = _t(user, torch.float32), _t(items, torch.float32)
    out = _coarse(tu, ti, k, M)
    want_cert, margin = _margins(user, items, k, M, out)
    print("near-tied margin max %.3f" % np.nanmax(margin))
    assert (out[2] == 0).all() and not want_cert.any()
    sc, ids = _engine().top_k(tu, ti, k)
    c = out[2].bool()
    _same((out[0][c], out[1][c]), (sc[c], ids[c]), "certified => equal")


# ---- 5b: the verdict where it depends on E_b ---------------------------------------------------------------------------------------
def _verdicts(user, items, k, M):
    """One call; asserts that the GPU's verdict is the restatement's for every row whose margin is not within 1e-9 of 1 (the GPU adds
    the norms' squares in wave order, which tc_norm_up's slack of (d + 64) 2^-51 covers: E_b differs by parts in 1e-12) and that the
    certified rows are nrms_topk_dot's.  -> (certified [B] bool, margin [B], rows that differ from nrms_topk_dot [B] bool)."""
    tu, ti = _t(user, torch.float32), _t(items, torch.float32)
    out = _coarse(tu, ti, k, M)
    want_cert, margin = _margins(user, items, k, M, out)
    cert = out[2].cpu().numpy().astype(bool)
    band = np.abs(margin - 1) <= 1e-9
    assert band.sum() <= len(cert) // 100, band.sum()
    wrong = np.nonzero((cert != want_cert) & ~band)[0]
    assert len(wrong) == 0, (wrong[:10], margin[wrong[:10]])
    sc, ids = _engine().top_k(tu, ti, k)
    c = out[2].bool()
    _same((out[0][c], out[1][c]), (sc[c], ids[c]), "certified => equal")
    return cert, margin, (out[1] != ids).any(dim=1).cpu().numpy()


@pytest.mark.parametrize("B,N,d,k,M,eps,seed", ref.GRADED)
def test_graded_margins_the_verdict_is_the_restatements(B, N, d, k, M, eps, seed):
    """Margins from a third to three inside one batch.  tests/test_topk_coarse_host.py shows on the same data that leaving one term
    of E_b out changes tens of verdicts, so a coarse_finish_kernel with a wrong E_b, a wrong slot of unorm or stats, or the wrong
    shortlist entry fails here.  Measured on an MI355X: DESIGN.md section 8h."""
    user, items = ref.graded(B, N, d, eps, seed)
    cert, margin, _ = _verdicts(user, items, k, M)
    print("graded d=%d k=%d M=%d: certified %d / %d, margin %.2f ... %.2f, min |margin - 1| %.1e"
          % (d, k, M, cert.sum(), B, margin.min(), margin.max(), np.abs(margin - 1).min()))
    assert np.isfinite(margin).all() and 0.2 * B <= cert.sum() <= 0.8 * B


@pytest.mark.parametrize("B,N,d,k", ref.TIGHT)
def test_a_shortlist_of_k_on_inexact_data(B, N, d, k):
    """M = k, where the shortlist does lose true top-k items.  A full shortlist of k is never certified (the entry with the smallest
    coarse score has c_j = c_M and s_k <= s_j <= c_j + E_b), so what keeps the served answer right here is that verdict: near-tied
    rows differ from nrms_topk_dot and none of them is certified.  Dominant items: the k far ahead of the rest are the shortlist, the
    rows equal nrms_topk_dot's uncertified, and one more slot certifies every one of them."""
    user, items = _near_tied(B, N, d, 1)
    cert, margin, differ = _verdicts(user, items, k, k)
    print("near-tied d=%d M=k=%d: %d / %d rows differ from nrms_topk_dot, %d certified" % (d, k, differ.sum(), B, cert.sum()))
    assert differ.sum() >= 1 and not cert.any() and not (differ & cert).any()
    user, items = ref.dominant(B, N, d, k, 3)
    cert, margin, differ = _verdicts(user, items, k, k)
    assert not differ.any() and not cert.any()
    cert, margin, differ = _verdicts(user, items, k, k + 1)
    print("dominant d=%d k=%d M=k+1: %d / %d certified, margin %.1f ... %.1f" % (d, k, cert.sum(), B, margin.min(), margin.max()))
    assert cert.all() and not differ.any()


@pytest.mark.parametrize("d", [80, 300])
def test_out_of_range_values_end_to_end(d):
    """Clamped (|x| > 65504) and flushed (|x| < 2^-14) entries in the catalogue and in the users, through the pack, the slice kernel
    and the certificate.  Users scaled by 2^-16 have h(u) = 0: every coarse score is 0, the shortlist is the first M ids, and
    Cauchy-Schwarz itself forbids the certificate."""
    B, N, k, M = 99, 2500, 1, 8
    user, items, kind = ref.out_of_range(B, N, d, 1)
    zero = torch.as_tensor(kind == 0, device=DEV)
    _, _, _, ssc, sid, _ = _coarse(_t(user, torch.float32), _t(items, torch.float32), k, M)
    assert (ssc[zero] == 0).all() and sid[zero].tolist() == [list(range(M))] * 33
    cert, margin, differ = _verdicts(user, items, k, M)
    n_cert = [int(cert[kind == i].sum()) for i in range(3)]
    print("out of range d=%d: certified of 33 each: scaled by 2^-16 %d, an entry of 1e6 %d, untouched %d; min |margin - 1| %.1e; "
          "%d uncertified rows differ" % (d, n_cert[0], n_cert[1], n_cert[2], np.nanmin(np.abs(margin - 1)), differ.sum()))
    assert n_cert[0] == 0 and 2 <= n_cert[1] <= 31 and 2 <= n_cert[2] <= 31          # both verdicts among the other two kinds


def _as_catalogue(items):
    """Rows as a model's catalogue: news id n is row n, row 0 the padding title's."""
    return torch.cat([torch.zeros(1, items.shape[1], device=DEV), items]).contiguous()


def test_model_repairs_uncertified_rows_and_mixed_batch():
    """A near-tied catalogue through Model.recommend: the fallback runs and the result is the plain call's, bit for bit.  Then a
    mixed batch at the engine: users who see Gaussian scores beside users who see near-tied ones."""
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model("nrms_v0")
    N, d = cat.shape
    rng = np.random.default_rng(7)
    tied = _as_catalogue(_t((rng.standard_normal((1, d)) + 1e-3 * rng.standard_normal((N - 1, d))).astype(F), torch.float32))
    packed = model.pack_catalogue(tied)
    n_un = 0
    for batch in batches:
        for k in (5, 20):
            ids, sc, cert = model.recommend(batch, k, tied, coarse=packed, coarse_shortlist=max(16, k), return_certified=True)
            _same((sc, ids), model.recommend(batch, k, tied)[::-1], "recommend(coarse=...) on a near-tied catalogue")
            assert cert.dtype == torch.uint8 and tuple(cert.shape) == (ids.shape[0],)
            n_un += int((cert == 0).sum())
    assert n_un > 0                                                   # the fallback ran
    # mixed: the first half of the width carries Gaussian items, the second half near-tied ones; a user lives in one half
    B, N, d, k, M = 66, 2500, 300, 10, 64
    items = np.concatenate([rng.standard_normal((N, d // 2)), rng.standard_normal((1, d // 2)) + 1e-3 * rng.standard_normal((N, d // 2))],
                           axis=1).astype(F)
    user = rng.standard_normal((B, d)).astype(F)
    user[0::2, d // 2:] = 0
    user[1::2, :d // 2] = 0
    tu, ti = _t(user, torch.float32), _t(items, torch.float32)
    sc, ids, cert, _, _, packed = _coarse(tu, ti, k, M)
    assert (cert[0::2] == 1).all() and (cert[1::2] == 0).all()
    want = _engine().top_k(tu, ti, k)
    c = cert.bool()
    _same((sc[c], ids[c]), (want[0][c], want[1][c]), "certified => equal in a mixed batch")
    rows = (cert == 0).nonzero().view(-1)
    f = _engine().top_k(tu[rows].contiguous(), ti, k)
    sc[rows], ids[rows] = f
    _same((sc, ids), want, "the repaired mixed batch")


# ---- 6: invariance ---------------------------------------------------------------------------------------------------------------
def _raw_coarse(user, items, packed, k, M, ex, poison):
    """The C call with every output and the workspace poisoned, between guard bands."""
    lib = _lib.load()
    B, d = user.shape
    N = items.shape[0]
    need = int(lib.nrms_topk_dot_coarse_workspace_bytes(B, C.c_int64(N), d, k, M))
    pool = Pool(poison)
    ws = pool.new("workspace", need)
    sc, ids, cert = pool.elems("top_scores", B * k), pool.elems("top_ids", B * k, torch.int64), pool.elems("certified", B, torch.uint8)
    ssc, sid = pool.elems("short_scores", B * M), pool.elems("short_ids", B * M, torch.int64)
    rc = lib.nrms_topk_dot_coarse(B, C.c_int64(N), d, k, M, _lib.ptr(user), _lib.ptr(items), _lib.ptr(packed.items16), _lib.ptr(packed.stats),
                                  _lib.ptr(ex), 0 if ex is None else ex.shape[1], sc.ptr, ids.ptr, cert.ptr, ssc.ptr, sid.ptr, ws.ptr,
                                  C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_topk_dot_coarse")
    pool.intact("nrms_topk_dot_coarse")
    return sc.numpy((B, k)), ids.numpy((B, k)), cert.numpy(), ssc.numpy((B, M)), sid.numpy((B, M))


def test_invariance_and_determinism():
    for d in (300, 80):                                               # pitch 320: superblocks only; pitch 96: a superblock and the tail
        _invariance_and_determinism(d)


def _invariance_and_determinism(d):
    rng = np.random.default_rng(11)
    B, N, k, M = 70, 5000, 10, 64
    user = rng.standard_normal((B, d)).astype(F)
    user[1::2] = _near_tied(B, N, d, 1)[0][1::2]
    items = np.concatenate([rng.standard_normal((N // 2, d)), _near_tied(B, N - N // 2, d, 1)[1]]).astype(F)
    tu, ti = _t(user, torch.float32), _t(items, torch.float32)
    ex = _t(rng.integers(-1, N + 1, size=(B, 40)), torch.int64)
    eng = _engine()
    packed = eng.pack_catalogue(ti)
    run = lambda u, e: eng.top_k_coarse(u, packed, k, M, e, return_shortlist=True)
    base = run(tu, ex)
    _same(run(tu, ex), base, "second run")
    parts = [slice(0, 33), slice(33, 70)]
    got = [run(tu[p].contiguous(), ex[p].contiguous()) for p in parts]
    _same([torch.cat([g[i] for g in got]) for i in range(5)], base, "batch split 33 + 37")
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(DEV)
    _same(run(tu[perm].contiguous(), ex[perm].contiguous()), [x[perm] for x in base], "user permutation")
    for fill in (0xFF, 0x00, 0x7F):
        _same(_raw_coarse(tu, ti, packed, k, M, ex, fill), base, "poison 0x%02X" % fill)
    # excluded ids never appear, in the list or in the shortlist
    for out in (base[1], base[4]):
        assert not ((out.unsqueeze(2) == ex.unsqueeze(1)) & (ex.unsqueeze(1) >= 0)).any()
    # without the shortlist outputs: the same rows
    _same(eng.top_k_coarse(tu, packed, k, M, ex), base[:3], "short_scores / short_ids NULL")


def test_a_non_finite_catalogue_row_certifies_nobody():
    from tests.test_hip_mmr import _model
    rng = np.random.default_rng(12)
    B, N, d, k, M = 33, 2500, 40, 5, 64
    user, items = rng.standard_normal((B, d)).astype(F), rng.standard_normal((N, d)).astype(F)
    items[17, 3] = np.nan
    tu, ti = _t(user, torch.float32), _t(items, torch.float32)
    sc, ids, cert, _, _, packed = _coarse(tu, ti, k, M)
    assert packed.stats[0].item() == float("inf") and (cert == 0).all()
    sc, ids, cert, _, _, _ = _coarse(tu, ti[10:30].contiguous(), k, M)     # ... even where the shortlist holds every eligible item
    assert (cert == 0).all()
    cfg, model, batches, cat = _model("nrms_v0")
    bad = cat.clone()
    bad[11, 2] = float("inf")
    packed = model.pack_catalogue(bad)
    for batch in batches:
        ids, sc, cert = model.recommend(batch, 10, bad, coarse=packed, return_certified=True)
        assert (cert == 0).all()
        _same((sc, ids), model.recommend(batch, 10, bad)[::-1], "recommend(coarse=...) with a non-finite catalogue row")


# ---- 7: layers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_models_recommend_through_the_shortlist(kind):
    from tests.test_hip_mmr import _model
    cfg, model, batches, cat = _model(kind)
    packed = model.pack_catalogue(cat)
    assert isinstance(packed, PackedCatalogue) and tuple(packed.items16.shape) == (cat.shape[0] - 1, ref.pitch(cat.shape[1]))
    assert packed.nbytes == (cat.shape[0] - 1) * ref.pitch(cat.shape[1]) * 2
    n_cert = 0
    for batch in batches:
        B = torch.as_tensor(batch["browsed_ids"]).shape[0]
        for k, M in ((5, None), (20, 32), (100, 256)):
            ids, sc, cert = model.recommend(batch, k, cat, coarse=packed, coarse_shortlist=M, return_certified=True)
            _same((sc, ids), model.recommend(batch, k, cat)[::-1], "%s recommend(coarse=...) k=%d" % (kind, k))
            assert cert.dtype == torch.uint8 and tuple(cert.shape) == (B,)
            n_cert += int(cert.sum())
            _same(model.recommend(batch, k, cat, coarse=packed, coarse_shortlist=M)[::-1], (sc, ids), "without return_certified")
            ids2, sc2 = model.recommend(batch, k, cat, exclude_history=False, coarse=packed, coarse_shortlist=M)
            _same((sc2, ids2), model.recommend(batch, k, cat, exclude_history=False)[::-1], "exclude_history=False")
    print("%s certified rows: %d" % (kind, n_cert))
    batch = batches[0]
    # a stale pack: another tensor, or another shape
    for other in (cat.clone(), cat[:-1].contiguous()):
        with pytest.raises(_lib.NrmsError, match="packed from another catalogue"):
            model.recommend(batch, 5, other, coarse=packed)
    t = torch.zeros(cat.shape[0], dtype=torch.int32, device=DEV)
    w = torch.zeros(torch.as_tensor(batch["browsed_ids"]).shape[0], 2, dtype=torch.int32, device=DEV)
    for kw, word in ((dict(diversity=0.5), "diversity"), (dict(item_bias=torch.zeros(cat.shape[0], device=DEV)), "item_bias"),
                     (dict(item_time=t, window=w), "window")):
        with pytest.raises(_lib.NrmsError, match=word):
            model.recommend(batch, 5, cat, coarse=packed, **kw)
    with pytest.raises(_lib.NrmsError, match="coarse_shortlist"):
        model.recommend(batch, 5, cat, coarse=packed, coarse_shortlist=4)
    with pytest.raises(_lib.NrmsError, match="PackedCatalogue"):
        model.recommend(batch, 5, cat, coarse=cat)
    model.check_recommend_ids()


def test_models_without_a_plain_dot_product_refuse():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    packed = _engine().pack_catalogue(torch.zeros(4, 8, device=DEV))
    for mod in (hierec_hip, graph_hip):
        with pytest.raises(_lib.NrmsError, match="coarse"):
            mod.Model.recommend(None, {}, 5, None, coarse=packed)


def test_engine_argument_checks():
    eng = _engine()
    items = torch.zeros(100, 8, device=DEV)
    user = torch.zeros(3, 8, device=DEV)
    packed = eng.pack_catalogue(items)
    assert packed.stats.tolist() == [0.0, 0.0] and packed.source == (items.data_ptr(), (100, 8))
    for k, M in ((0, 8), (9, 8), (8, 257)):
        with pytest.raises(_lib.NrmsError, match="arguments rejected"):
            eng.top_k_coarse(user, packed, k, M)
    with pytest.raises(_lib.NrmsError, match="PackedCatalogue"):
        eng.top_k_coarse(user, items, 2, 8)
    with pytest.raises(_lib.NrmsError, match="width"):
        eng.top_k_coarse(torch.zeros(3, 9, device=DEV), packed, 2, 8)
    sc, ids, cert = eng.top_k_coarse(user, packed, 2, 8)              # all scores tie at 0: the ids decide, nothing is certified
    assert ids.tolist() == [[0, 1]] * 3 and cert.tolist() == [0, 0, 0]
    sc, ids, cert = eng.top_k_coarse(torch.zeros(0, 8, device=DEV), packed, 2, 8)
    assert tuple(ids.shape) == (0, 2) and tuple(cert.shape) == (0,)


def test_run_v0_coarse_catalogue_writes_the_same_file(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    outs = []
    for name, extra in (("plain", []), ("coarse", ["--coarse_catalogue"])):
        out = tmp_path / (name + ".txt")
        r = subprocess.run([sys.executable, "-m", "pytorch_news_recommender_amd.run_v0", "--model", "nrms_hip", "--dataset", "synthetic",
                            "--max_batches", "2", "--epochs", "1", "--synthetic_users", "128", "--batch_size", "64",
                            "--description", "T", "--data_path", str(tmp_path / "data"), "--save_path", str(tmp_path / ("save_" + name)),
                            "--recommend", "5", "--recommend_out", str(out)] + extra,
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append((out.read_text(), r.stdout))
    assert outs[0][0] == outs[1][0] and len(outs[0][0].splitlines()) == 1024
    share = re.findall(r"^coarse catalogue: certified share: (\d\.\d+)  users: (\d+)$", outs[1][1], re.M)
    assert len(share) == 1 and 0.0 <= float(share[0][0]) <= 1.0 and int(share[0][1]) == 1024, outs[1][1][-2000:]
    assert "certified share" not in outs[0][1]
