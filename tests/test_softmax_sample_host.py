"""Host side of the softmax negative sampler (csrc/softmaxsample.hip, Model.sample_negatives, ClickFeed(negatives="adaptive"),
run_v0 --negatives adaptive): the restatement's own statistics, its fp32 perturbation against float64, the C ABI's argument
checks from a C99 program, and the flag checks that need no GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.config import Config
from pytorch_news_recommender_amd.data_handler import ClickFeed, SyntheticMind

from tests import philox_ref as ph
from tests import softmax_sample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xC0FFEE0123456789


@pytest.fixture(scope="module")
def stat_words():
    return ref.words(SEED, ref.STAT_KEYS, len(ref.STAT_SCORES))


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
def test_words_are_the_two_level_philox_draw():
    keys = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 48 - 1], dtype=np.int64)
    w = ref.words(SEED, keys, 11)
    assert w.dtype == np.uint32 and w.shape == (5, 11)
    for b, k in enumerate(keys.tolist()):
        r = ph.philox4x32_7(SEED, np.array([k], dtype=np.uint64), 8)
        row_seed = int(r[0][0]) | (int(r[1][0]) << 32)
        for n in range(11):
            call = ph.philox4x32_7(row_seed, np.array([n >> 2], dtype=np.uint64), 9)
            assert int(w[b, n]) == int(call[n & 3][0]), (k, n)
    assert np.array_equal(ref.words(SEED, keys, 5), w[:, :5])                   # N does not move a word
    assert np.array_equal(ref.words(SEED, keys[::-1].copy(), 11), w[::-1])      # nor does the row's position
    assert not np.array_equal(ref.words(SEED + 1, keys, 11), w)


def test_u_is_exact_and_strictly_inside_the_unit_interval(stat_words):
    edge = np.array([0, 0x1FF, 0x200, 0xFFFFFFFF, 0xFFFFFE00], dtype=np.uint32)
    u = ref.uniform(edge)
    assert u.dtype == np.float32
    assert u.tolist() == [2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24, 1 - 2.0 ** -24, 1 - 2.0 ** -24]
    us = ref.uniform(stat_words)
    assert us.min() > 0.0 and us.max() < 1.0
    m = (stat_words >> np.uint32(9)).astype(np.float64)
    assert np.array_equal(us.astype(np.float64), (2 * m + 1) / 2.0 ** 24)      # no rounding anywhere
    assert float(ref.gumbel64(edge).max()) < ref.G_MAX and float(ref.gumbel32(edge).max()) < ref.G_MAX


def test_fp32_gumbel_against_float64(stat_words):
    """The restatement's own fp32 error: 5.44e-7 on these inputs (asserted: at most 5.7e-7).  tests/test_hip_softmax_sample.py takes its bar for the device's
    logf from this value (4 x, on the same words)."""
    err = float(np.abs(ref.gumbel32(stat_words).astype(np.float64) - ref.gumbel64(stat_words)).max())
    print("max |g32 - g64| over %d words: %.3e" % (stat_words.size, err))
    assert 0.0 < err <= 5.7e-7


def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(20000).astype(np.float32) * np.float32(30)
    b = rng.standard_normal(20000).astype(np.float32)
    c = rng.standard_normal(20000).astype(np.float32) * np.float32(4)
    from fractions import Fraction
    got = ref.fma32(a, b, c)
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), i
    # a case double rounding gets wrong: 1 + 2^-24 + 2^-60 lies above the fp32 midpoint, the float64 sum on it
    assert ref.fma32(np.float32(2.0 ** -30), np.float32(2.0 ** -30), np.float32(1 + 2.0 ** -23))[()] == np.float32(1 + 2.0 ** -23)
    x = ref.fma32(np.array([2.0 ** -30], np.float32), np.array([2.0 ** -30], np.float32), np.array([1.0], np.float32))
    assert x[0] == np.float32(1.0)
    assert np.isnan(ref.fma32(np.float32(np.inf), np.float32(0.0), np.float32(1.0)))
    assert ref.fma32(np.float32(np.inf), np.float32(2.0), np.float32(1.0)) == np.float32(np.inf)


def test_select_orders_by_key_then_id_and_pads():
    key = np.array([[1, 3, 3, np.nan, -0.0, 0.0, np.inf, -np.inf]], dtype=np.float32)
    ids, k = ref.select(key, 9)
    assert ids[0].tolist() == [6, 1, 2, 0, 4, 5, 7, -1, -1] and k[0, -1] == -np.inf and k[0, 6] == -np.inf and ids[0, 6] == 7
    assert not np.signbit(k[0, 4])                                               # -0.0 comes back as +0.0
    ids, _ = ref.select(key, 3, exclude=np.array([[6, 1, -1, 99]]))
    assert ids[0].tolist() == [2, 0, 4]


@pytest.mark.parametrize("inv_t", ref.STAT_INV_T)
def test_restatement_draws_from_the_softmax_in_plackett_luce_order(stat_words, inv_t):
    """65 536 rows: first picks against softmax(s / t), ordered (first, second) pairs with an expected count >= 50 against
    Plackett-Luce, all within 6 sd (the fp32 restatement stays within 2.5 sd on these inputs)."""
    scores = np.broadcast_to(ref.STAT_SCORES, (ref.STAT_ROWS, len(ref.STAT_SCORES)))
    ids, keys = ref.sample(scores, ref.STAT_KEYS, 2, inv_t, SEED, g=ref.gumbel32(stat_words))
    assert (ids >= 0).all() and (ids[:, 0] != ids[:, 1]).all() and (keys[:, 0] >= keys[:, 1]).all()
    worst, judged = ref.worst_deviation(ids, ref.STAT_SCORES, inv_t)
    print("inv_temperature %g: worst deviation %.2f sd over 8 first picks and %d pairs" % (inv_t, worst, judged))
    assert judged >= 20 and worst <= 6.0                 # (at inv_temperature 3 most pairs are too rare to be judged)
    if inv_t == 0.0:
        p, pair = ref.plackett_luce(ref.STAT_SCORES, 0.0)
        assert np.allclose(p, 1 / 8) and np.allclose(pair[~np.eye(8, dtype=bool)], 1 / 56)


# ---- 2. the C ABI from C ---------------------------------------------------------------------------------------------------------------
C_PROG = r"""
#include "nrms_hip.h"
#include <math.h>
#include <stdio.h>
#include <string.h>

static float u[4], it[8], keys[8];
static int64_t rk[2] = {0, 1}, ids[8];
static uint64_t ws[512];

static int expect(int rc, const char* word) {
    const char* msg = nrms_last_error();
    if (rc != NRMS_EINVAL && rc != NRMS_EWORKSPACE) { printf("FAIL %s: rc=%d\n", word, rc); return 1; }
    if (!msg || !strstr(msg, word)) { printf("FAIL %s: rc=%d msg=%s\n", word, rc, msg ? msg : "(null)"); return 1; }
    return 0;
}

#define CALL(B, N, d, S, user, items, key, inv_t, ex, n_ex, ids, keys, ws, wb) \
    nrms_softmax_sample_dot(B, N, d, S, user, items, key, inv_t, 7, ex, n_ex, ids, keys, ws, wb, NULL)

int main(void) {
    int bad = 0;
    const size_t wb = sizeof ws;
    bad += expect(CALL(-1, 4, 2, 3, u, it, rk, 1.0f, NULL, 0, ids, keys, ws, wb), "B");
    bad += expect(CALL(2, -1, 2, 3, u, it, rk, 1.0f, NULL, 0, ids, keys, ws, wb), "N");
    bad += expect(CALL(2, (int64_t)0x7FFF0001, 2, 3, u, it, rk, 1.0f, NULL, 0, ids, keys, ws, wb), "N");
    bad += expect(CALL(2, 4, 0, 3, u, it, rk, 1.0f, NULL, 0, ids, keys, ws, wb), "d");
    bad += expect(CALL(2, 4, 2, 0, u, it, rk, 1.0f, NULL, 0, ids, keys, ws, wb), "S=0");
    bad += expect(CALL(2, 4, 2, 257, u, it, rk, 1.0f, NULL, 0, ids, keys, ws, wb), "S=257");
    bad += expect(CALL(2, 4, 2, 3, u, it, rk, 1.0f, NULL, -1, ids, keys, ws, wb), "n_exclude");
    bad += expect(CALL(2, 4, 2, 3, u, it, rk, -0.5f, NULL, 0, ids, keys, ws, wb), "inv_temperature");
    bad += expect(CALL(2, 4, 2, 3, u, it, rk, INFINITY, NULL, 0, ids, keys, ws, wb), "inv_temperature");
    bad += expect(CALL(2, 4, 2, 3, u, it, rk, NAN, NULL, 0, ids, keys, ws, wb), "inv_temperature");
    bad += expect(CALL(2, 4, 2, 3, NULL, it, rk, 1.0f, NULL, 0, ids, keys, ws, wb), "user");
    bad += expect(CALL(2, 4, 2, 3, u, NULL, rk, 1.0f, NULL, 0, ids, keys, ws, wb), "items");
    bad += expect(CALL(2, 4, 2, 3, u, it, NULL, 1.0f, NULL, 0, ids, keys, ws, wb), "row_key");
    bad += expect(CALL(2, 4, 2, 3, u, it, rk, 1.0f, NULL, 0, NULL, keys, ws, wb), "ids");
    bad += expect(CALL(2, 4, 2, 3, u, it, rk, 1.0f, NULL, 0, ids, keys, NULL, wb), "workspace");
    bad += expect(CALL(2, 4, 2, 3, u, it, rk, 1.0f, NULL, 0, ids, keys, ws, 8), "workspace");
    bad += expect(nrms_softmax_sample_noise(-1, 4, rk, 7, NULL, keys, NULL), "B");
    bad += expect(nrms_softmax_sample_noise(2, 4, rk, 7, NULL, NULL, NULL), "null");
    bad += expect(nrms_softmax_sample_noise(2, 4, NULL, 7, NULL, keys, NULL), "row_key");
    /* B = 0: accepted, nothing launched, nothing written */
    ids[0] = -7;
    if (CALL(0, 4, 2, 3, NULL, NULL, NULL, 1.0f, NULL, 0, NULL, NULL, NULL, 0) != 0 || ids[0] != -7) { printf("FAIL B=0\n"); bad += 1; }
    if (nrms_softmax_sample_noise(0, 4, NULL, 7, NULL, keys, NULL) != 0 || nrms_softmax_sample_noise(2, 0, NULL, 7, NULL, keys, NULL) != 0) {
        printf("FAIL noise of nothing\n");
        bad += 1;
    }
    printf("WS %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", nrms_softmax_sample_dot_workspace_bytes(512, 130000, 300, 0, 0),
           nrms_softmax_sample_dot_workspace_bytes(512, 130000, 300, 257, 0), nrms_softmax_sample_dot_workspace_bytes(512, 130000, 0, 4, 0),
           nrms_softmax_sample_dot_workspace_bytes(512, 130000, 300, 4, -1), nrms_softmax_sample_dot_workspace_bytes(-1, 130000, 300, 4, 0),
           nrms_softmax_sample_dot_workspace_bytes(512, (int64_t)0x7FFF0001, 300, 4, 0),
           nrms_softmax_sample_dot_workspace_bytes(512, 130000, 300, 4, 70), nrms_softmax_sample_dot_workspace_bytes(512, 130000, 300, 4, 0),
           nrms_topk_dot_workspace_bytes(512, 130000, 300, 4));
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_softmax_sample_c_abi_validation_and_workspace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "softmax_sample_abi.c", tmp_path / "softmax_sample_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    ws = [int(v) for v in out.split("WS ")[1].split("\n")[0].split()]
    assert ws[:6] == [0, 0, 0, 0, 0, 0]                      # S = 0, S = 257, d = 0, n_exclude < 0, B < 0, N past the limit
    assert ws[6] == ws[7] == ws[8] > 0                       # the slices of nrms_topk_dot, whatever the exclude width


def test_header_binding_sites_build_list_and_capability_flags_are_in_step():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    for name, n_args in (("nrms_softmax_sample_dot_workspace_bytes", 5), ("nrms_softmax_sample_dot", 16), ("nrms_softmax_sample_noise", 7)):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    lib = _lib.load()
    assert lib.nrms_softmax_sample_dot_workspace_bytes(10, 100, 8, 4, 3) > 0
    assert lib.nrms_softmax_sample_dot_workspace_bytes(10, 100, 8, 257, 0) == 0
    common = open(os.path.join(ROOT, "pytorch_news_recommender_amd", "csrc", "common.h")).read()
    assert re.search(r"PHILOX_SITE_SOFTMAX_ROW\s*=\s*8u", common) and re.search(r"PHILOX_SITE_SOFTMAX_ITEM\s*=\s*9u", common)
    assert (ref.SITE_ROW, ref.SITE_ITEM) == (8, 9)
    sites = re.findall(r"PHILOX_SITE_\w+\s*=\s*(\d+)u", common)
    assert len(sites) == len(set(sites)) and all(int(v) > 4 for v in sites)
    build = open(os.path.join(ROOT, "pytorch_news_recommender_amd", "build.py")).read()
    assert '"softmaxsample.hip"' in build and '"topk_kernels.h"' in build
    from importlib import import_module
    for module, can in (("nrms_hip", True), ("nrms_v1_hip", True), ("nrms_naml_hip", True), ("nrms_bert_hip", True),
                        ("hierec_hip", False), ("graph_hip", False)):
        model = import_module("pytorch_news_recommender_amd.model." + module).Model
        assert model.CATALOGUE_SAMPLING is can and hasattr(model, "sample_negatives") is can, module


# ---- 3. run_v0 --negatives adaptive -------------------------------------------------------------------------------------------------
def test_run_v0_adaptive_flag_is_checked_before_any_data_is_read(tmp_path, monkeypatch):
    from pytorch_news_recommender_amd import run_v0
    p = run_v0.build_parser()
    base = p.parse_args(["--model", "nrms_hip"])
    assert base.negatives == "fixed" and base.negative_temperature == 1.0 and base.loss == "rowwise"
    for model in ("nrms_hip", "nrms_v1_hip", "nrms_naml", "nrms_bert"):
        ok = p.parse_args(["--model", model, "--negatives", "adaptive", "--dataset", "synthetic", "--negative_temperature", "0.5"])
        assert ok.negatives == "adaptive" and ok.negative_temperature == 0.5
        run_v0.check_negatives_args(ok)
    run_v0.check_negatives_args(p.parse_args(["--model", "nrms_hip", "--negatives", "adaptive", "--dataset", "synthetic", "--loss", "pooled",
                                              "--no_logq"]))
    run_v0.check_negatives_args(p.parse_args(["--model", "hierec", "--dataset", "large", "--negative_temperature", "-1"]))   # fixed: unused
    monkeypatch.chdir(tmp_path)
    data = tmp_path / "data_processed"
    syn = ["--negatives", "adaptive", "--dataset", "synthetic"]
    for argv, word in ((["--negatives", "adaptive", "--dataset", "large"], "synthetic"),
                       (["--negatives", "adaptive", "--dataset", "demo"], "synthetic"),
                       (syn + ["--feed", "loader"], "device"),
                       (syn + ["--test", "1"], "--test"),
                       (syn + ["--negative_temperature", "0"], "negative_temperature"),
                       (syn + ["--negative_temperature", "-2"], "negative_temperature"),
                       (syn + ["--negative_temperature", "inf"], "negative_temperature"),
                       (syn + ["--model", "hierec"], "hierec"),
                       (syn + ["--model", "graph"], "graph"),
                       (syn + ["--model", "graph", "--graph", "global"], "--graph global"),
                       (syn + ["--loss", "pooled"], "--no_logq")):
        with pytest.raises(SystemExit) as e:
            run_v0.main(["--model", "nrms_hip", "--data_path", str(data)] + argv)
        assert word in str(e.value), (argv, e.value)
        assert not data.exists(), argv                                                                             # nothing was read or written


# ---- 4. the feed, as far as a host goes --------------------------------------------------------------------------------------------
def test_click_feed_adaptive_arguments_and_refusals_on_a_host():
    cfg = Config("nrms_hip")
    cfg.__nrms__()
    cfg.n_words_title = 30
    corpus = SyntheticMind(cfg, n_news=120, seed=4)
    user_ptr, clicks = corpus.click_log(12, min_clicks=4, max_clicks=20)
    kw = dict(id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, batch_size=8, device="cpu")
    plain = ClickFeed(cfg, user_ptr, clicks, **kw)
    assert plain.negatives == "popularity" and plain.temperature == 1.0
    feed = ClickFeed(cfg, user_ptr, clicks, negatives="adaptive", temperature=0.25, **kw)
    assert feed.negatives == "adaptive" and feed.temperature == 0.25
    # the host copy of the set lengths the exclude matrices are sized with
    sets = np.diff(feed.set_ptr.numpy())
    assert np.array_equal(feed._row_set_len, sets[feed.row_user.numpy()]) and len(feed._row_set_len) == feed.n_samples
    for bad in (dict(negatives="hard"), dict(negatives="adaptive", temperature=0.0), dict(negatives="adaptive", temperature=float("nan"))):
        with pytest.raises(ValueError):
            ClickFeed(cfg, user_ptr, clicks, **bad, **kw)
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    for module in (graph_hip, hierec_hip):
        with pytest.raises(ValueError, match="CATALOGUE_SAMPLING"):
            feed.attach_scorer(object.__new__(module.Model))
    # candidate_logq: the popularity sampler's table, which an adaptive draw does not follow
    rows = np.arange(4)
    import torch
    b = feed.batch(torch.from_numpy(rows))
    with pytest.raises(KeyError, match="no fixed q"):
        b["candidate_logq"]
    assert b.get("candidate_logq") is None and len(b) == 13
    assert tuple(plain.batch(torch.from_numpy(rows))["candidate_logq"].shape) == (4, cfg.sample_size + 1)
