"""CPU-only checks of the fp16 shortlist with a certificate (include/nrms_hip.h nrms_catalogue_pack_f16 / nrms_topk_dot_coarse): the
numpy restatement's own properties, a C99 program compiled against the header, the signatures, the domain of the workspace query,
and the refusals of Model.recommend / run_v0 that need no GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib

from tests import topk_coarse_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrms_catalogue_f16_pitch", "nrms_catalogue_pack_f16", "nrms_topk_dot_coarse_workspace_bytes", "nrms_topk_dot_coarse")
F = np.float32


# ---- 1: the restatement ------------------------------------------------------------------------------------------------------
def test_element_rule_and_pitch():
    assert [ref.pitch(d) for d in (1, 31, 32, 33, 300)] == [32, 32, 32, 64, 320]
    just_below = np.nextafter(F(2.0 ** -14), F(0))
    x = np.array([0.0, -0.0, 2.0 ** -14, just_below, -just_below, 65504.0, 65519.9, 65520.0, -65520.0, 1e30, -1e30, 1.0 + 2.0 ** -11,
                  1.0 + 3 * 2.0 ** -11], dtype=F)
    got = ref.h(x)
    want = np.array([0.0, -0.0, 2.0 ** -14, 0.0, -0.0, 65504.0, 65504.0, 65504.0, -65504.0, 65504.0, -65504.0, 1.0, 1.0 + 2.0 ** -9],
                    dtype=np.float16)                                 # (the last two: ties to even)
    assert got.view(np.uint16).tolist() == want.view(np.uint16).tolist()
    assert np.isfinite(got).all() and not ((np.abs(got.astype(F)) > 0) & (np.abs(got.astype(F)) < 2.0 ** -14)).any()


def test_stats_bound_the_float64_maxima():
    rng = np.random.default_rng(0)
    for N, d in ((0, 5), (1, 1), (33, 7), (200, 300)):
        items = (rng.normal(size=(N, d)) * 10.0 ** rng.integers(-6, 5, size=(N, 1))).astype(F)
        bits, stats = ref.pack(items)
        nrm, err = ref.true_stats(items)
        assert bits.shape == (N, ref.pitch(d)) and (bits[:, d:] == 0).all()
        assert nrm <= stats[0] <= nrm * (1 + 1e-6) and err <= stats[1] <= err * (1 + 1e-6)
    items = rng.normal(size=(5, 9)).astype(F)
    items[2, 3], items[4, 0] = np.nan, -np.inf
    bits, stats = ref.pack(items)
    assert stats[0] == np.inf and (bits[[2, 4]] == 0).all() and bits[0].any() and np.isfinite(stats[1])


def test_the_identity_behind_the_bound():
    rng = np.random.default_rng(1)
    for d in (1, 16, 300):
        u, n = rng.normal(size=(20, d)).astype(F), rng.normal(size=(30, d)).astype(F)
        u16, n16 = ref.halves(ref.pack_rows(u)[0], d), ref.halves(ref.pack_rows(n)[0], d)
        u64, n64 = u.astype(np.float64), n.astype(np.float64)
        lhs = u64 @ n64.T - u16 @ n16.T
        rhs = (u64 - u16) @ n64.T + u16 @ (n64 - n16).T
        assert np.abs(lhs - rhs).max() <= 1e-12
        # ... and Cauchy-Schwarz with the packed norms bounds it
        _, stats = ref.pack(n)
        un = ref.pack_rows(u)[2]
        bound = un[:, 2] * float(stats[0]) + un[:, 1] * float(stats[1])
        assert (np.abs(lhs).max(axis=1) <= bound).all()


def _cases():
    rng = np.random.default_rng(2)
    for i in range(300):
        B, N, d = int(rng.integers(1, 4)), int(rng.integers(1, 60)), int(rng.integers(1, 20))
        k = int(rng.integers(1, 9))
        M = int(rng.integers(k, 17))
        kind = i % 4
        u = rng.normal(size=(B, d)).astype(F)
        if kind == 0:
            n = rng.normal(size=(N, d)).astype(F)
        elif kind == 1:                                               # near-ties
            n = (rng.normal(size=(1, d)) + 1e-3 * rng.normal(size=(N, d))).astype(F)
        elif kind == 2:                                               # exact ties and a wide spread
            n = rng.integers(-2, 3, size=(N, d)).astype(F) * F(2.0) ** rng.integers(-3, 4, size=(N, 1)).astype(F)
        else:                                                         # a few dominant items
            n = rng.normal(size=(N, d)).astype(F)
            n[rng.integers(0, N, size=min(N, k))] *= 50
        ex = rng.integers(-1, N + 1, size=(B, 3)) if i % 3 == 0 else None
        yield u, n, k, M, ex


def test_certified_rows_are_the_full_top_k():
    n_cert = n_not = 0
    for u, n, k, M, ex in _cases():
        got = ref.topk_coarse(u, n, k, M, ex)
        want_ids, want_sc = ref.ordered(ref.exact_scores64(u, n), ex, k)
        for b in range(u.shape[0]):
            if got["certified"][b]:
                n_cert += 1
                assert got["ids"][b].tolist() == want_ids[b].tolist(), (k, M, got["margin"][b])
                assert got["scores"][b].tobytes() == want_sc[b].tobytes()
            else:
                n_not += 1
                assert got["short_ids"][b, M - 1] >= 0                # an uncertified row has a full shortlist
        assert ex is None or not any(int(x) in got["short_ids"][b] for b in range(u.shape[0]) for x in ex[b] if x >= 0)
    assert n_cert > 100 and n_not > 50, (n_cert, n_not)


def test_certificate_refuses_what_it_cannot_bound():
    rng = np.random.default_rng(3)
    u, n = rng.normal(size=(2, 8)).astype(F), rng.normal(size=(40, 8)).astype(F)
    assert ref.topk_coarse(u, n, 2, 4)["certified"].all()
    bad = n.copy()
    bad[1, 1] = np.inf
    assert not ref.topk_coarse(u, bad, 2, 4, exact=ref.exact_scores64(u, n))["certified"].any()
    assert ref.topk_coarse(u, bad[:3], 2, 4, exact=ref.exact_scores64(u, n[:3]))["certified"].tolist() == [False, False]     # even with L < M
    big = (u * F(1e20)).astype(F)
    assert not ref.topk_coarse(big, (n * F(1e15)).astype(F), 2, 4)["certified"].any()          # un * NRM > 2^100
    assert ref.topk_coarse(u, n[:3], 2, 4)["certified"].all()                                  # L < M: everything is in the shortlist


# ---- 1b: the data the GPU tests pin the certificate with ------------------------------------------------------------------------
def test_e_bound_is_the_rounded_up_sum_of_its_terms():
    rng = np.random.default_rng(4)
    up = ref.up
    for _ in range(200):
        d = int(rng.integers(1, 2000))
        un, un16, ue, NRM, ERR = (float(v) for v in np.abs(rng.normal(size=5)) * 10.0 ** rng.integers(-6, 7, size=5))
        t = ref.e_terms(d, un, un16, ue, NRM, ERR)
        assert len(t) == len(ref.E_TERMS) == 5
        gamma = up(up(d * 2.0 ** -24) / (1.0 - d * 2.0 ** -24))
        want = [up(ue * NRM), up(un16 * ERR), up(gamma * up(un * NRM)), up(d * 2.0 ** -21 * up(un16 * up(NRM + ERR))), up(d * 2.0 ** -140)]
        assert [float(v) for v in t] == [float(v) for v in want]
        E = want[0]
        for v in want[1:]:
            E = up(E + v)
        assert float(ref.e_bound(d, un, un16, ue, NRM, ERR)) == float(E) > sum(float(v) for v in want[:4]) * (1 - 1e-15)
        for i, name in enumerate(ref.E_TERMS):
            rest = [v for j, v in enumerate(want) if j != i]
            E = rest[0]
            for v in rest[1:]:
                E = up(E + v)
            assert float(ref.e_bound(d, un, un16, ue, NRM, ERR, drop=name)) == float(E)


def _certified_rows_are_exact(got, user, items, k):
    """-> the number of rows whose ids differ from the exact order's, after asserting that no certified row is among them."""
    want_ids, want_sc = ref.ordered(ref.exact_scores64(user, items), None, k)
    differ = (got["ids"] != want_ids).any(axis=1)
    assert not (differ & got["certified"]).any()
    c = got["certified"]
    assert got["scores"][c].tobytes() == want_sc[c].tobytes()
    return int(differ.sum())


@pytest.mark.parametrize("B,N,d,k,M,eps,seed", ref.GRADED)
def test_graded_margins_straddle_one_and_tell_the_terms_apart(B, N, d, k, M, eps, seed):
    """What makes test_hip_topk_coarse.py::test_graded_margins_the_verdict_is_the_restatements a test of E_b: on this data the
    verdict of a tenth of the batch or more changes when one of the three large terms is left out, and of some rows with gamma_d's."""
    user, items = ref.graded(B, N, d, eps, seed)
    got = ref.topk_coarse(user, items, k, M)
    margin, cert = got["margin"], got["certified"]
    assert np.isfinite(margin).all()
    band = np.abs(margin - 1) <= 1e-9
    print("graded d=%d k=%d M=%d: certified %d / %d, margin %.2f ... %.2f, min |margin - 1| %.1e"
          % (d, k, M, cert.sum(), B, margin.min(), margin.max(), np.abs(margin - 1).min()))
    assert band.sum() <= B // 100 and 0.2 * B <= cert.sum() <= 0.8 * B
    assert (cert == (margin > 1))[~band].all()
    _certified_rows_are_exact(got, user, items, k)
    flips = {}
    for name in ref.E_TERMS[:4]:                                     # (d 2^-140 decides nothing at these magnitudes)
        wrong, _ = ref.certificate(d, k, M, got["unorm"], got["stats"], got["short_ids"], got["short_scores"], got["scores"], drop=name)
        flips[name] = int((wrong != cert).sum())
        assert not (cert & ~wrong).any()                             # a smaller bound only certifies more
    print("  rows whose verdict changes without", flips)
    assert min(flips["ue*NRM"], flips["un16*ERR"], flips["alpha"]) >= 10 and flips["gamma"] >= 2, flips


@pytest.mark.parametrize("B,N,d,k", ref.TIGHT)
def test_a_shortlist_of_k_loses_items_and_is_never_certified(B, N, d, k):
    """M = k.  A full shortlist of k cannot be certified: the entry with the smallest coarse score has c_j = c_M and s_j >= s_k, and
    s_j <= c_j + E_b is what E_b bounds, so s_k > c_M + E_b is false.  On near-tied items the shortlist does lose true top-k items;
    on dominant items it does not, and one more slot (M = k + 1) certifies every row."""
    user, items = ref.near_tied(B, N, d, 1)
    got = ref.topk_coarse(user, items, k, k)
    lost = _certified_rows_are_exact(got, user, items, k)
    print("near-tied d=%d M=k=%d: %d / %d rows differ from the exact order" % (d, k, lost, B))
    assert lost >= 1 and not got["certified"].any()
    user, items = ref.dominant(B, N, d, k, 3)
    got = ref.topk_coarse(user, items, k, k)
    assert _certified_rows_are_exact(got, user, items, k) == 0 and not got["certified"].any()
    got = ref.topk_coarse(user, items, k, k + 1)
    assert _certified_rows_are_exact(got, user, items, k) == 0 and got["certified"].all()
    print("dominant d=%d k=%d M=k+1: margin %.1f ... %.1f" % (d, k, got["margin"].min(), got["margin"].max()))


@pytest.mark.parametrize("d", [80, 300])
def test_out_of_range_values_through_the_certificate(d):
    B, N, k, M = 99, 2500, 1, 8
    user, items, kind = ref.out_of_range(B, N, d, 1)
    bits, stats = ref.pack(items)
    v16 = ref.halves(bits, d)
    assert (np.abs(v16) == 65504).sum() == 6 and (np.abs(items) > 65504).sum() == 6
    assert ((v16 == 0) & (items != 0)).sum() >= 300 and 69000 < stats[0] < 71000 and 3000 < stats[1] < 5000
    u16 = ref.halves(ref.pack_rows(user)[0], d)
    assert not u16[kind == 0].any() and (np.abs(u16[kind == 1]) == 65504).sum() == 33
    got = ref.topk_coarse(user, items, k, M)
    _certified_rows_are_exact(got, user, items, k)
    n_cert = [int(got["certified"][kind == i].sum()) for i in range(3)]
    print("out of range d=%d: certified of 33 each: scaled by 2^-16 %d, an entry of 1e6 %d, untouched %d; min |margin - 1| %.1e"
          % (d, n_cert[0], n_cert[1], n_cert[2], np.nanmin(np.abs(got["margin"] - 1))))
    assert (got["short_scores"][kind == 0] == 0).all() and n_cert[0] == 0
    assert 5 <= n_cert[1] <= 28 and 5 <= n_cert[2] <= 31 and not (np.abs(got["margin"] - 1) <= 1e-9).any()


# ---- 2: the symbols ----------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_signatures_and_library():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(size_t|int|int32_t)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, name + " is not declared in include/nrms_hip.h"
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(2).count(",") + 1, name
    assert len(_lib.SIGNATURES["nrms_topk_dot_coarse"][1]) == 19 and len(_lib.SIGNATURES["nrms_catalogue_pack_f16"][1]) == 6
    assert len(_lib.SIGNATURES["nrms_topk_dot_coarse_workspace_bytes"][1]) == len(_lib.SIGNATURES["nrms_topk_dot_workspace_bytes"][1]) + 1
    lib = _lib.load()                                                # binds every symbol: a missing export raises here
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for word in ("GUARANTEE", "bit for bit", "gamma_d", "alpha_d = d*2^-21", "2^100", "Cauchy-Schwarz", "topk_dot_coarse: ..."):
        assert word in text, word
    from pytorch_news_recommender_amd import build
    assert "topkcoarse.hip" in build.SOURCES


def test_workspace_query_domain_and_pitch():
    import ctypes as C
    lib = _lib.load()
    q = lambda B, N, d, k, M: lib.nrms_topk_dot_coarse_workspace_bytes(B, C.c_int64(N), d, k, M)
    for B, N, d, k, M in ((70, 5000, 40, 10, 64), (512, 130000, 300, 100, 256), (1, 0, 1, 1, 1), (0, 5, 3, 256, 256), (33, 2500, 44, 100, 193)):
        assert q(B, N, d, k, M) > 0
    assert q(70, 5000, 40, 11, 10) == 0                              # k > M
    assert q(70, 5000, 40, 10, 257) == 0                             # M > 256
    assert q(70, 5000, 40, 0, 64) == 0                               # k < 1
    assert q(70, 5000, 0, 10, 64) == 0 and q(-1, 5000, 40, 10, 64) == 0 and q(70, -1, 40, 10, 64) == 0
    assert q(512, 130000, 300, 10, 256) > q(512, 130000, 300, 10, 64)
    assert q(512, 130000, 300, 10, 64) < 512 * 130000 * 4 // 4       # far from a [B, N] score matrix
    assert [lib.nrms_catalogue_f16_pitch(d) for d in (1, 7, 31, 32, 33, 300, 0, -4)] == [32, 32, 32, 32, 64, 320, 0, 0]


C_PROG = r"""
#include "nrms_hip.h"
#include <stdio.h>
#include <string.h>

static float u[8], it[8], sc[8], st[2], ssc[8];
static uint16_t it16[64];
static int64_t ids[8], sid[8];
static uint8_t cert[2];
static uint64_t ws[65536];

static int expect(int rc, int want, const char* word) {
    const char* msg = nrms_last_error();
    if (rc != want || !msg || strncmp(msg, "topk_dot_coarse: ", 17) != 0 || !strstr(msg, word)) {
        printf("FAIL %s: rc=%d msg=%s\n", word, rc, msg ? msg : "(null)");
        return 1;
    }
    return 0;
}

int main(void) {
    int bad = 0;
    const size_t wb = sizeof ws;
    uint16_t* odd16 = (uint16_t*)((char*)it16 + 2);
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 0, 4, u, it, it16, st, NULL, 0, sc, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "k");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 2, u, it, it16, st, NULL, 0, sc, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "M");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 257, u, it, it16, st, NULL, 0, sc, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "M");
    bad += expect(nrms_topk_dot_coarse(2, 4, 0, 3, 4, u, it, it16, st, NULL, 0, sc, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "d");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, NULL, it, it16, st, NULL, 0, sc, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "user");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, u, NULL, it16, st, NULL, 0, sc, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "items");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, u, it, NULL, st, NULL, 0, sc, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "items16");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, u, it, odd16, st, NULL, 0, sc, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "items16 must be 16-byte aligned");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, u, it, it16, NULL, NULL, 0, sc, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "stats");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, u, it, it16, st, NULL, 0, NULL, ids, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "top_scores");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, u, it, it16, st, NULL, 0, sc, NULL, cert, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "top_ids");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, u, it, it16, st, NULL, 0, sc, ids, NULL, ssc, sid, ws, wb, NULL), NRMS_EINVAL, "certified");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, u, it, it16, st, NULL, 0, sc, ids, cert, NULL, NULL, NULL, wb, NULL), NRMS_EINVAL, "workspace");
    bad += expect(nrms_topk_dot_coarse(2, 4, 2, 3, 4, u, it, it16, st, NULL, 0, sc, ids, cert, NULL, NULL, ws, 8, NULL), NRMS_EWORKSPACE, "workspace");
    if (nrms_topk_dot_coarse(0, 4, 2, 3, 4, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL) != NRMS_OK) { printf("FAIL B=0\n"); bad++; }
    if (nrms_catalogue_pack_f16(-1, 2, it, it16, st, NULL) != NRMS_EINVAL || !strstr(nrms_last_error(), "catalogue_pack_f16: N")) { printf("FAIL pack N\n"); bad++; }
    if (nrms_catalogue_pack_f16(4, 0, it, it16, st, NULL) != NRMS_EINVAL || !strstr(nrms_last_error(), "d must")) { printf("FAIL pack d\n"); bad++; }
    if (nrms_catalogue_pack_f16(4, 2, it, it16, NULL, NULL) != NRMS_EINVAL || !strstr(nrms_last_error(), "stats is null")) { printf("FAIL pack stats\n"); bad++; }
    if (nrms_catalogue_pack_f16(4, 2, NULL, it16, st, NULL) != NRMS_EINVAL || !strstr(nrms_last_error(), "items is null")) { printf("FAIL pack items\n"); bad++; }
    if (nrms_catalogue_pack_f16(4, 2, it, odd16, st, NULL) != NRMS_EINVAL || !strstr(nrms_last_error(), "16-byte")) { printf("FAIL pack align\n"); bad++; }
    printf("WS %zu %zu %zu %zu %zu PITCH %d %d\n", nrms_topk_dot_coarse_workspace_bytes(512, 130000, 300, 11, 10),
           nrms_topk_dot_coarse_workspace_bytes(512, 130000, 300, 10, 257), nrms_topk_dot_coarse_workspace_bytes(512, 130000, 300, 0, 64),
           nrms_topk_dot_coarse_workspace_bytes(512, 130000, 300, 10, 64), nrms_topk_dot_coarse_workspace_bytes(512, 130000, 300, 100, 256),
           (int)nrms_catalogue_f16_pitch(300), (int)nrms_catalogue_f16_pitch(32));
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_coarse_c_abi_validation_and_workspace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "coarse_abi.c", tmp_path / "coarse_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    w = out.split("WS ")[1].split("\n")[0].split()
    assert [int(v) for v in w[:3]] == [0, 0, 0] and 0 < int(w[3]) < int(w[4])
    assert w[5:] == ["PITCH", "320", "32"]


# ---- 3: the refusals that need no GPU ------------------------------------------------------------------------------------------
def test_recommend_refuses_before_anything_touches_the_device():
    from pytorch_news_recommender_amd.engine import PackedCatalogue
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip, nrms_hip, nrms_naml_hip
    import inspect
    cat = torch.zeros(5, 4)
    packed = PackedCatalogue(cat[1:], torch.zeros(4, 32, dtype=torch.int16), torch.zeros(2), source=(cat.data_ptr(), (5, 4)))
    f = nrms_hip.Model._coarse_args
    none = dict(diversity=None, shortlist=None, return_ild=False, item_bias=None, item_time=None, window=None)
    call = lambda k, coarse, M=None, cert=False, **kw: f("recommend", k, coarse, M, cert, **{**none, **kw})
    assert call(10, None) is None
    assert call(10, packed) == 64 and call(20, packed) == 80 and call(100, packed) == 256 and call(10, packed, 10) == 10
    for kw, word in ((dict(diversity=0.5), "diversity"), (dict(shortlist=20), "diversity"), (dict(return_ild=True), "diversity"),
                     (dict(item_bias=torch.zeros(5)), "item_bias"), (dict(item_time=torch.zeros(5)), "item_time"),
                     (dict(window=torch.zeros(1, 2)), "window")):
        with pytest.raises(_lib.NrmsError, match=word):
            call(10, packed, **kw)
    for k, M in ((10, 9), (10, 257), (0, 64)):
        with pytest.raises(_lib.NrmsError, match="coarse_shortlist"):
            call(k, packed, M)
    with pytest.raises(_lib.NrmsError, match="PackedCatalogue"):
        call(10, cat)
    with pytest.raises(_lib.NrmsError, match="coarse"):
        call(10, None, 64)
    with pytest.raises(_lib.NrmsError, match="coarse"):
        call(10, None, None, True)
    # a pack of another tensor is told by data_ptr and shape
    other = torch.zeros(5, 4)
    with pytest.raises(_lib.NrmsError, match="packed from another catalogue"):
        nrms_hip.Model._recommend_coarse(None, None, other, None, 2, 4, packed, False)
    with pytest.raises(_lib.NrmsError, match="packed from another catalogue"):
        nrms_hip.Model._recommend_coarse(None, None, cat[:4], None, 2, 4, packed, False)
    # nrms_naml's override takes the same arguments; HieRec and the graph model refuse in their own words
    want = list(inspect.signature(nrms_hip.Model.recommend).parameters)
    assert list(inspect.signature(nrms_naml_hip.Model.recommend).parameters) == want and want[-3:] == ["coarse", "coarse_shortlist", "return_certified"]
    for mod, word in ((hierec_hip, "hierec: recommend takes no coarse"), (graph_hip, "graph: recommend takes no coarse")):
        for kw in (dict(coarse=packed), dict(coarse_shortlist=64), dict(return_certified=True)):
            with pytest.raises(_lib.NrmsError, match=word):
                mod.Model.recommend(None, {}, 5, None, **kw)


@pytest.mark.parametrize("argv,ok", [
    (["--recommend", "5", "--coarse_catalogue"], True),
    (["--recommend", "5", "--coarse_catalogue", "--coarse_shortlist", "5"], True),
    (["--recommend", "100", "--coarse_catalogue", "--coarse_shortlist", "256"], True),
    (["--model", "nrms_v1", "--recommend", "5", "--coarse_catalogue"], True),
    (["--recommend", "5"], True),
    (["--coarse_catalogue"], False),
    (["--recommend", "5", "--coarse_shortlist", "64"], False),
    (["--recommend", "5", "--coarse_catalogue", "--coarse_shortlist", "4"], False),
    (["--recommend", "5", "--coarse_catalogue", "--coarse_shortlist", "257"], False),
    (["--recommend", "5", "--coarse_catalogue", "--diversity", "0.5"], False),
    (["--negatives", "catalogue", "--recommend", "5", "--coarse_catalogue", "--popularity_prior", "0.5"], False),
    (["--negatives", "catalogue", "--recommend", "5", "--coarse_catalogue", "--catalogue_window", "100"], False),
    (["--recommend", "5", "--coarse_catalogue", "--sections", "category"], False),
])
def test_check_coarse_args(argv, ok):
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(["--dataset", "synthetic"] + ([] if "--model" in argv else ["--model", "nrms_hip"]) + argv)
    if ok:
        assert run_v0.check_coarse_args(args) is None
    else:
        with pytest.raises(SystemExit) as e:
            run_v0.check_coarse_args(args)
        assert "--coarse_" in str(e.value)


def test_run_v0_refuses_before_any_data_is_read(tmp_path):
    from pytorch_news_recommender_amd import run_v0
    data = tmp_path / "data_processed"
    for argv in (["--coarse_catalogue"], ["--recommend", "5", "--coarse_catalogue", "--diversity", "0.5"],
                 ["--model", "hierec", "--recommend", "5", "--coarse_shortlist", "64"]):
        with pytest.raises(SystemExit):
            run_v0.main((["--model", "nrms_hip"] if "--model" not in argv else []) + argv + ["--dataset", "synthetic", "--data_path", str(data)])
        assert not data.exists(), argv


def test_loop_packs_once_and_reports_the_certified_share(tmp_path):
    from pytorch_news_recommender_amd import train_eval

    class Stub:
        def __init__(self):
            self.packs, self.calls = 0, []

        def encode_catalogue(self, titles):
            return torch.zeros(20, 4)

        def pack_catalogue(self, catalogue):
            self.packs += 1
            return ("packed", catalogue)

        def recommend(self, batch, k, catalogue, exclude_history=True, **kw):
            B = batch["browsed_ids"].shape[0]
            self.calls.append(kw)
            out = (torch.arange(1, k + 1).expand(B, k), torch.zeros(B, k))
            return out + (torch.tensor([1] + [0] * (B - 1), dtype=torch.uint8),) if kw.get("return_certified") else out

        def check_recommend_ids(self):
            pass

        class engine:
            check_ids = staticmethod(lambda: None)

    batches = [{"browsed_ids": torch.zeros(3, 2, dtype=torch.int64)}, {"browsed_ids": torch.zeros(1, 2, dtype=torch.int64)}]
    m = Stub()
    a = train_eval.recommend(None, m, batches, None, 4, out_file=str(tmp_path / "a.txt"), coarse=True, coarse_shortlist=8)
    assert m.packs == 1 and m.last_coarse_stats == {"certified": 0.5, "n_users": 4}
    assert all(c["coarse"][0] == "packed" and c["coarse_shortlist"] == 8 and c["return_certified"] for c in m.calls)
    m2 = Stub()
    b = train_eval.recommend(None, m2, batches, None, 4, out_file=str(tmp_path / "b.txt"))
    assert m2.packs == 0 and m2.calls == [{}, {}] and m2.last_coarse_stats is None         # absent: no keyword at all
    assert open(a).read() == open(b).read()
    for kw in (dict(coarse_shortlist=8), dict(coarse=True, diversity=0.5), dict(coarse=True, item_bias=torch.zeros(20))):
        with pytest.raises(ValueError, match="coarse"):
            train_eval.recommend(None, m, batches, None, 4, out_file=str(tmp_path / "c.txt"), **kw)
