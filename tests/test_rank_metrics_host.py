"""MRR / nDCG host restatements against the reference's own values (fixture g8), the submission scorer's input
rules, and the argument checks of nrms_impression_metrics -- all without a GPU."""
import ctypes
import io
import os

import numpy as np
import pytest

from pytorch_news_recommender_amd import _lib, evaluation


def _brute_ranks(s):
    """rank_m by definition: 1 + #{j : s_j > s_i} + #{j > i : s_j == s_i}."""
    n = len(s)
    return np.array([1 + sum(s[j] > s[i] for j in range(n)) + sum(s[j] == s[i] for j in range(i + 1, n))
                     for i in range(n)])


def test_host_mrr_and_ndcg_match_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "g8_rank_metrics.npz"))
    assert g["scores"].shape == (64, 300)
    for i, n in enumerate(g["lens"]):
        y, s = g["labels"][i, :n], g["scores"][i, :n]
        got = [evaluation.mrr_score(y, s), evaluation.ndcg_score(y, s, 5), evaluation.ndcg_score(y, s, 10)]
        want = [g["mrr"][i], g["ndcg5"][i], g["ndcg10"][i]]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, err_msg="row %d" % i)
        if y.any() and not y.all():
            assert abs(evaluation.auc_score(y, s) - g["auc"][i]) < 1e-12
        else:
            assert np.isnan(g["auc"][i])
    # the fixture holds every edge the kernel has to meet
    assert {1, 2, 5, 6, 10, 11, 63, 64, 65, 300} <= set(g["lens"].tolist())
    pos = [g["labels"][i, :n].sum() for i, n in enumerate(g["lens"])]
    assert any(p == 0 for p in pos) and any(p == n for p, n in zip(pos, g["lens"]) if n > 1)


def test_host_functions_against_brute_force_stable_ranks():
    rng = np.random.default_rng(5)
    for t in range(300):
        n = int(rng.integers(1, 40))
        s = rng.integers(0, 4, n).astype(np.float32)                   # many ties
        y = (rng.random(n) < 0.3).astype(np.int64)
        r = _brute_ranks(s)
        assert sorted(r) == list(range(1, n + 1))
        npos = y.sum()
        for k in (1, 5, 10, 300):
            dcg = sum(1.0 / np.log2(r[i] + 1) for i in range(n) if y[i] and r[i] <= k)
            ideal = sum(1.0 / np.log2(q + 1) for q in range(1, min(npos, k) + 1))
            got = evaluation.ndcg_score(y, s, k)
            if npos == 0:
                assert np.isnan(got)
            else:
                assert abs(got - dcg / ideal) < 1e-12
                assert abs(evaluation.dcg_score(y, s, k) - dcg) < 1e-12
        got = evaluation.mrr_score(y, s)
        if npos == 0:
            assert np.isnan(got)
        else:
            assert abs(got - sum(1.0 / r[i] for i in range(n) if y[i]) / npos) < 1e-12
    # all positive: nDCG 1, MRR = H_n / n
    assert abs(evaluation.ndcg_score([1, 1, 1], [0.3, 0.3, 0.1], 5) - 1.0) < 1e-15
    assert abs(evaluation.mrr_score([1] * 4, [0.0] * 4) - (1 + 1 / 2 + 1 / 3 + 1 / 4) / 4) < 1e-15


TRUTH = "1 [0,1,0]\n2 []\n3 [1,0,0,0,1]\n4 [0,1]\n"


def test_read_submission_rules():
    # line 2 (empty labels) is skipped but still consumes its prediction line; a missing last line is all ranks 1
    pred = "1 [2,1,3]\n2 [1]\n3 [5,4,3,2,1]\n"
    scores, lab, lens = evaluation.read_submission(io.StringIO(TRUTH), io.StringIO(pred))
    assert lens.tolist() == [3, 5, 2] and scores.shape == (3, 5) and scores.dtype == np.float32
    np.testing.assert_array_equal(scores[0, :3], np.float32([1 / 2, 1, 1 / 3]))
    np.testing.assert_array_equal(scores[1], np.float32([1 / 5, 1 / 4, 1 / 3, 1 / 2, 1]))
    np.testing.assert_array_equal(scores[2, :2], [1, 1])
    np.testing.assert_array_equal(lab[1], [1, 0, 0, 0, 1])
    # an empty prediction line counts as all ranks 1 too
    s2, _, _ = evaluation.read_submission(io.StringIO(TRUTH), io.StringIO("1 [2,1,3]\n2 [1]\n\n4 [1,2]\n"))
    np.testing.assert_array_equal(s2[1], [1] * 5)
    np.testing.assert_array_equal(s2[2, :2], [1, 1 / 2])


@pytest.mark.parametrize("pred, msg", [
    ("1 [2,1,3]\n2 []\n7 [5,4,3,2,1]\n", "inconsistent impression id"),
    ("1 [0,1,2]\n", "1 to 3"),
    ("1 [2,1,4]\n", "1 to 3"),
    ("1 [2,1]\n", "2 ranks for 3 labels"),
    ("1 [2,1,3]\n2 []\n3 [5,4,3,2,1.5]\n", "invalid prediction"),
    ("1 2,1,3\n", "invalid prediction"),
    ("1\n", "invalid prediction"),
])
def test_read_submission_errors(tmp_path, pred, msg):
    truth, sub = tmp_path / "truth.txt", tmp_path / "prediction.txt"
    truth.write_text(TRUTH)
    sub.write_text(pred)
    with pytest.raises(ValueError, match=msg):
        evaluation.read_submission(str(truth), str(sub))
    with pytest.raises(ValueError, match=msg):
        evaluation.score_submission(str(truth), str(sub))        # the input is refused before any device work


def test_impression_metrics_argument_validation_without_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)            # never dereferenced: validation fails first
    out = ctypes.c_void_p(0x2000)
    rc = lib.nrms_impression_metrics(4, 0, fake, fake, fake, 5, 10, out, None, None, None, None, None)
    assert rc != 0 and b"impression_metrics" in lib.nrms_last_error()
    rc = lib.nrms_impression_metrics(-1, 10, fake, fake, fake, 5, 10, out, None, None, None, None, None)
    assert rc != 0
    rc = lib.nrms_impression_metrics(4, 10, None, fake, fake, 5, 10, out, None, None, None, None, None)
    assert rc != 0
    rc = lib.nrms_impression_metrics(4, 10, fake, fake, fake, 0, 10, out, None, None, None, None, None)
    assert rc != 0 and b"cutoffs" in lib.nrms_last_error()
    rc = lib.nrms_impression_metrics(4, 10, fake, fake, fake, 5, 10, None, None, None, None, None, None)
    assert rc != 0 and b"every output is null" in lib.nrms_last_error()
    # nothing to do is not an error (and touches no device)
    assert lib.nrms_impression_metrics(0, 10, fake, fake, fake, 5, 10, out, None, None, None, None, None) == 0
    with pytest.raises(_lib.NrmsError):
        _lib.check(lib.nrms_impression_metrics(4, 10, fake, fake, fake, 5, -3, out, None, None, None, None, None),
                   "nrms_impression_metrics")
