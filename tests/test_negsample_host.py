"""Host side of the per-epoch negative sampler (csrc/negsample.hip, data_handler.ImpressionFeed, run_v0 --negatives): the numpy
restatement's own properties, the C ABI's argument checks from a C99 program, and the flag and feed checks that need no GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.config import Config
from pytorch_news_recommender_amd.data_handler import ImpressionFeed, SyntheticMind

from tests import negsample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _impression(n, n_pos, rng):
    shown = rng.permutation(np.arange(1, n + 1)).astype(np.int64)            # distinct ids: a set comparison means something
    label = np.zeros(n, dtype=np.uint8)
    label[rng.choice(n, size=n_pos, replace=False)] = 1
    return shown, label


# ---- 1. the restatement's own properties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4, 5])
@pytest.mark.parametrize("n,n_pos", [(12, 4), (300, 70)])
def test_restatement_gives_disjoint_slices_of_the_impressions_negatives(n, n_pos, S):
    """n_neg = 8 or 230: with S = 4 or 5 the last positives' slices are short or empty at both sizes."""
    rng = np.random.default_rng(n * 100 + S)
    shown, label = _impression(n, n_pos, rng)
    negatives = set(shown[label == 0].tolist())
    positives = shown[label != 0].tolist()
    n_neg = len(negatives)
    imp_ptr = np.array([0, n], dtype=np.int64)
    orders = set()
    for seed in range(150):
        seed = seed * 0x1F123BB5 + 7
        rows = ref.sample_impression(shown, label, ref.words(seed, n), S)
        assert [r[0] for r in rows] == positives
        seen = set()
        for p, r in enumerate(rows):
            assert len(r) - 1 == min(S, max(0, n_neg - p * S))
            assert set(r[1:]) <= negatives and not (set(r[1:]) & seen) and len(set(r[1:])) == len(r) - 1
            seen |= set(r[1:])
        cand, clen, n_bad = ref.negative_sample(imp_ptr, shown, label, S, seed)
        assert n_bad == 0 and cand.shape == (n_pos, S + 1) and clen.tolist() == [len(r) for r in rows]
        assert [row[:c].tolist() for row, c in zip(cand, clen)] == rows and all((row[c:] == 0).all() for row, c in zip(cand, clen))
        orders.add(tuple(cand.reshape(-1).tolist()))
    assert len(orders) > 100                                                    # another seed, another draw


def test_vectorised_restatement_matches_the_loop_on_a_mixed_log():
    rng = np.random.default_rng(5)
    lens = np.concatenate([[0, 1, 1, 2, 63, 64, 65, 300], rng.integers(1, 90, size=60)])
    force = {1: [1], 2: [0], 3: [1, 1]}
    imp_ptr, shown, label = ref.random_log(lens, rng, force=force)
    for S in (1, 4, 64):
        cand, clen, n_bad = ref.negative_sample(imp_ptr, shown, label, S, seed=99, max_shown=100)
        w = ref.words(99, imp_ptr[-1])
        rows = []
        for i in range(len(lens)):
            a, b = imp_ptr[i], imp_ptr[i + 1]
            got = ref.sample_impression(shown[a:b], label[a:b], w[a:b], S)
            rows += [r[:1] for r in got] if b - a > 100 else got                # above max_shown: positives only
        assert n_bad == 1 and len(rows) == len(cand)
        for row, c, want in zip(cand, clen, rows):
            assert row[:c].tolist() == want and (row[c:] == 0).all()


@pytest.mark.parametrize("n,n_pos,n_seeds", [(12, 2, 20000), (300, 20, 20000)])
def test_every_negative_is_first_equally_often(n, n_pos, n_seeds):
    """Slot 1 of the first positive's row is the negative of rank 0.  Over n_seeds seeds a negative's count is Binomial(n_seeds,
    1 / n_neg); the bar is 6 sd, as in tests/test_philox_ref_host.py (20 000 seeds: 2 000 +- 42 expected per negative at n = 12,
    71 +- 8.4 at n = 300, about two seconds each)."""
    rng = np.random.default_rng(n)
    shown, label = _impression(n, n_pos, rng)
    neg = np.flatnonzero(label == 0)
    n_neg = len(neg)
    counts = np.zeros(n, dtype=np.int64)
    imp_ptr = np.array([0, n], dtype=np.int64)
    for s in range(n_seeds):
        seed = ref.epoch_seed(12345, s)
        w = ref.words(seed, n)[neg]
        first = neg[np.lexsort((neg, w))[0]]
        counts[first] += 1
        if s < 50:
            assert ref.negative_sample(imp_ptr, shown, label, 4, seed)[0][0, 1] == shown[first]
    q = 1.0 / n_neg
    sigma = np.sqrt(n_seeds * q * (1 - q))
    worst = float(np.abs(counts[neg] - n_seeds * q).max() / sigma)
    print("n %d: %d negatives, expected %.1f per negative, sd %.2f, worst deviation %.2f sd" % (n, n_neg, n_seeds * q, sigma, worst))
    assert counts[label != 0].sum() == 0 and counts.sum() == n_seeds
    assert worst <= 6.0


# ---- 2. the C ABI from C ---------------------------------------------------------------------------------------------------------------
C_PROG = r"""
#include "nrms_hip.h"
#include <stdio.h>
#include <string.h>

static int64_t imp_ptr[3] = {0, 2, 5}, sample_ptr[3] = {0, 1, 2}, cand[2 * 65], clen[2];
static int32_t shown[5] = {1, 2, 3, 4, 5}, n_bad;
static uint8_t label[5] = {1, 0, 0, 1, 0};
static uint64_t ws[512];

static int expect(int rc, const char* word) {
    const char* msg = nrms_last_error();
    if (rc == 0 || !msg || !strstr(msg, word)) { printf("FAIL %s: rc=%d msg=%s\n", word, rc, msg ? msg : "(null)"); return 1; }
    return 0;
}

int main(void) {
    int bad = 0;
    const size_t wb = sizeof ws;
    const size_t need = nrms_negative_sample_workspace_bytes(2, 5, 4);
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 0, 2048, 1, cand, clen, &n_bad, ws, wb, NULL), "S=0");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 65, 2048, 1, cand, clen, &n_bad, ws, wb, NULL), "S=65");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 4, 0, 1, cand, clen, &n_bad, ws, wb, NULL), "max_shown=0");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 4, 2049, 1, cand, clen, &n_bad, ws, wb, NULL), "max_shown=2049");
    bad += expect(nrms_negative_sample(-1, imp_ptr, shown, label, sample_ptr, 4, 2048, 1, cand, clen, &n_bad, ws, wb, NULL), "n_imp=-1");
    bad += expect(nrms_negative_sample(2, NULL, shown, label, sample_ptr, 4, 2048, 1, cand, clen, &n_bad, ws, wb, NULL), "null");
    bad += expect(nrms_negative_sample(2, imp_ptr, NULL, label, sample_ptr, 4, 2048, 1, cand, clen, &n_bad, ws, wb, NULL), "null");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, NULL, sample_ptr, 4, 2048, 1, cand, clen, &n_bad, ws, wb, NULL), "null");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, NULL, 4, 2048, 1, cand, clen, &n_bad, ws, wb, NULL), "null");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 4, 2048, 1, NULL, clen, &n_bad, ws, wb, NULL), "null");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 4, 2048, 1, cand, NULL, &n_bad, ws, wb, NULL), "null");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 4, 2048, 1, cand, clen, NULL, ws, wb, NULL), "null");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 4, 2048, 1, cand, clen, &n_bad, NULL, wb, NULL), "workspace");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 4, 2048, 1, cand, clen, &n_bad, ws, need - 1, NULL), "workspace");
    bad += expect(nrms_negative_sample(2, imp_ptr, shown, label, sample_ptr, 4, 2048, 1, cand, clen, &n_bad, ws, 0, NULL), "workspace");
    printf("WS %zu %zu %zu %zu %zu %zu %zu %zu\n", nrms_negative_sample_workspace_bytes(2, 5, 0), nrms_negative_sample_workspace_bytes(2, 5, 65),
           nrms_negative_sample_workspace_bytes(-1, 5, 4), nrms_negative_sample_workspace_bytes(2, -1, 4),
           nrms_negative_sample_workspace_bytes((int64_t)1 << 31, 5, 4), need, nrms_negative_sample_workspace_bytes(0, 0, 1),
           nrms_negative_sample_workspace_bytes(2200000, 81000000, 4));
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_negative_sample_c_abi_validation_and_workspace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "negsample_abi.c", tmp_path / "negsample_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    ws = [int(v) for v in out.split("WS ")[1].split("\n")[0].split()]
    assert ws[:5] == [0, 0, 0, 0, 0]                                 # S = 0, S = 65, n_imp < 0, nnz < 0, n_imp = 2^31
    assert 0 < ws[5] <= 512 * 8 and ws[6] > 0                        # (the program's own buffer holds the small case)
    assert 4 * 2200000 <= ws[7] < 8 * 2200000                        # one int32 per impression at most, plus a header


def test_header_binding_site_and_build_list_are_in_step():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    for name in ("nrms_negative_sample_workspace_bytes", "nrms_negative_sample"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert lib.nrms_negative_sample_workspace_bytes(10, 100, 4) > 0
    assert lib.nrms_negative_sample_workspace_bytes(10, 100, 65) == 0 and b"S=65" in lib.nrms_last_error()
    common = open(os.path.join(ROOT, "pytorch_news_recommender_amd", "csrc", "common.h")).read()
    assert re.search(r"PHILOX_SITE_NEG_SAMPLE\s*=\s*6u", common) and ref.SITE == 6
    sites = re.findall(r"PHILOX_SITE_\w+\s*=\s*(\d+)u", common)
    assert len(sites) == len(set(sites))                             # no two samplers share a site
    assert "negsample.hip" in open(os.path.join(ROOT, "pytorch_news_recommender_amd", "build.py")).read()


# ---- 3. run_v0 --negatives ----------------------------------------------------------------------------------------------------------------
def test_run_v0_negatives_flag_is_checked_before_any_data_is_read(tmp_path, monkeypatch):
    from pytorch_news_recommender_amd import run_v0
    p = run_v0.build_parser()
    assert p.parse_args(["--model", "nrms_hip"]).negatives == "fixed"
    ok = p.parse_args(["--model", "nrms_hip", "--negatives", "epoch", "--dataset", "synthetic"])
    assert ok.negatives == "epoch"
    run_v0.check_negatives_args(ok)
    run_v0.check_negatives_args(p.parse_args(["--model", "nrms_hip", "--dataset", "large", "--feed", "loader"]))      # fixed: anything goes
    monkeypatch.chdir(tmp_path)
    data = tmp_path / "data_processed"
    for argv, word in ((["--negatives", "sometimes", "--dataset", "synthetic"], None),                               # unknown value
                       (["--negatives", "epoch", "--dataset", "large"], "synthetic"),
                       (["--negatives", "epoch", "--dataset", "demo"], "synthetic"),
                       (["--negatives", "epoch", "--dataset", "synthetic", "--feed", "loader"], "device"),
                       (["--negatives", "epoch", "--dataset", "synthetic", "--test", "1"], "--test")):
        with pytest.raises(SystemExit) as e:
            run_v0.main(["--model", "nrms_hip", "--data_path", str(data)] + argv)
        if word is not None:
            assert word in str(e.value), (argv, e.value)
        assert not data.exists(), argv                                                                                 # nothing was read or written


# ---- 4. the feed, as far as a host goes --------------------------------------------------------------------------------------------
def _config():
    cfg = Config("nrms_hip")
    cfg.__nrms__()
    cfg.n_words_title = 30
    return cfg


def test_train_impressions_have_their_own_stream():
    cfg = _config()
    a, b = SyntheticMind(cfg, n_news=300, seed=3), SyntheticMind(cfg, n_news=300, seed=3)
    imps, labels = a.train_impressions(40, max_shown=25)
    assert a.train_samples(20) == b.train_samples(20) and a.eval_samples(10) == b.eval_samples(10)      # the old streams did not move
    assert len(imps) == len(labels) == 40
    for s, y in zip(imps, labels):
        assert 4 <= len(s[3]) <= 25 and len(y) == len(s[3]) == len(s[4]) == len(s[5]) and set(y) == {0, 1}
        assert 3 <= len(s[0]) <= cfg.history_len and len(s[1]) == len(s[2]) == len(s[0])
    assert SyntheticMind(cfg, n_news=300, seed=3).train_impressions(40, max_shown=25) == (imps, labels)


def test_impression_feed_rows_checks_and_no_cpu_path():
    cfg = _config()
    corpus = SyntheticMind(cfg, n_news=300, seed=4)
    imps, labels = corpus.train_impressions(30, max_shown=20)
    kw = dict(id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, batch_size=8, device="cpu")
    feed = ImpressionFeed(cfg, imps, labels, seed=5, **kw)
    n_pos = [sum(y) for y in labels]
    assert feed.n_imp == 30 and feed.n_samples == sum(n_pos) == feed.n and len(feed) == (sum(n_pos) + 7) // 8
    assert feed.sample_ptr.tolist() == np.concatenate([[0], np.cumsum(n_pos)]).tolist()
    assert feed.sample_ptr.tolist() == ref.sample_ptr_of(feed.imp_ptr.numpy(), feed.label.numpy()).tolist()
    assert feed.imp_ptr.dtype == torch.int64 and feed.shown.dtype == torch.int32 and feed.label.dtype == torch.uint8
    assert feed.shown.tolist() == [v for s in imps for v in s[3]] and feed.label.tolist() == [v for y in labels for v in y]
    rows = [k for k, c in enumerate(n_pos) for _ in range(c)]                  # a history row per positive
    H = cfg.history_len
    assert feed.packed["hist"].tolist() == [(list(imps[k][0]) + [0] * H)[:H] for k in rows]
    assert feed.packed["hlen"].tolist() == [len(imps[k][0]) for k in rows]
    assert tuple(feed.packed["cand"].shape) == (feed.n, cfg.sample_size + 1)
    assert feed.epoch_seed(0) == 5 and feed.epoch_seed(3) == ref.epoch_seed(5, 3) == (5 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64
    info = feed.news_info()                                                     # from every SHOWN news, sampled or not
    for s in imps:
        for j, c, sc in zip(s[3], s[4], s[5]):
            assert int(info["categ"][j]) == c and int(info["subcateg"][j]) == sc
    with pytest.raises(_lib.NrmsError, match="no CPU path"):
        next(iter(feed))
    # min_history, the rank's share, from_arrays
    short = ImpressionFeed(cfg, imps, labels, min_history=20, **kw)
    kept = [k for k, s in enumerate(imps) if len(s[0]) >= 20]
    assert 0 < len(kept) < 30 and short.n_imp == len(kept) and short.n_samples == sum(n_pos[k] for k in kept)
    assert short.shown.tolist() == [v for k in kept for v in imps[k][3]]
    r1 = ImpressionFeed(cfg, imps, labels, rank=1, world=3, **kw)
    assert (r1.row0, r1.n, r1.n_samples) == (feed.n // 3, feed.n // 3, feed.n_samples)
    hist = np.zeros((30, H), dtype=np.int64)
    for k, s in enumerate(imps):
        hist[k, :len(s[0])] = s[0]
    arr = ImpressionFeed.from_arrays(cfg, hist, feed.imp_ptr.numpy(), feed.shown.numpy(), feed.label.numpy(), **kw)
    assert torch.equal(arr.packed["hist"], feed.packed["hist"]) and torch.equal(arr.sample_ptr, feed.sample_ptr)
    assert int(arr.news_info()["categ"].abs().sum()) == 0                       # no categories given: unknown everywhere
    # refused at construction
    long_imp = [[imps[0][0], None, None, list(range(1, 2050)), None, None]]
    with pytest.raises(ValueError, match="2049 news.*at most 2048"):
        ImpressionFeed(cfg, long_imp, [[1] + [0] * 2048], **kw)
    ImpressionFeed(cfg, [[imps[0][0], None, None, [1 + v % 299 for v in range(2048)], None, None]], [[1] + [0] * 2047], **kw)
    with pytest.raises(ValueError, match="labels"):
        ImpressionFeed(cfg, imps[:1], [labels[0][:-1]], **kw)
    with pytest.raises(ValueError, match="0 or 1"):
        ImpressionFeed(cfg, imps[:1], [[2] * len(labels[0])], **kw)
    with pytest.raises(ValueError, match="imp_ptr"):
        ImpressionFeed.from_arrays(cfg, hist, feed.imp_ptr.numpy()[:-1], feed.shown.numpy(), feed.label.numpy(), **kw)
