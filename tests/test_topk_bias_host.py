"""CPU-only checks of the per-news prior (include/nrms_hip.h nrms_topk_dot_biased / nrms_rank_dot_biased): the numpy restatement
on hand-made cases, the four symbols in the header and in _lib.SIGNATURES, the C ABI's argument validation and workspace queries
from a C99 program, run_v0's --popularity_prior checks, ClickFeed.popularity_prior against numpy, and the loops' default path
against a stub model that knows no item_bias keyword."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval
from pytorch_news_recommender_amd.engine import NRMSEngine

from tests import topk_bias_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrms_topk_dot_biased_workspace_bytes", "nrms_topk_dot_biased", "nrms_rank_dot_biased_workspace_bytes", "nrms_rank_dot_biased")
F = np.float32


# ---- 1: the restatement ------------------------------------------------------------------------------------------------------
def test_ref_tie_goes_to_the_smaller_id():
    s = np.array([[1.0, 3.0, 2.0, 2.5]], dtype=F)
    bias = np.array([2.0, 0.0, 1.0, 0.5], dtype=F)                  # everything becomes 3.0
    ids, sc = ref.topk(s, bias, None, 3)
    assert ids.tolist() == [[0, 1, 2]] and sc.tolist() == [[3.0, 3.0, 3.0]]
    rk, rs = ref.ranks(s, bias, None, np.array([[3, 0, 2, 1]]))
    assert rk.tolist() == [[4, 1, 3, 2]] and rs.tolist() == [[3.0] * 4]
    # without the bias the order is by score
    assert ref.topk(s, None, None, 4)[0].tolist() == [[1, 3, 2, 0]]


def test_ref_negative_zero():
    s = np.array([[-0.0, 0.0, -1.0, 1.0]], dtype=F)
    bias = np.array([0.0, -0.0, 1.0, -1.0], dtype=F)                # sums: +0, +0, +0 (-1 + 1), +0 (1 - 1)
    ids, sc = ref.topk(s, bias, None, 4)
    assert ids.tolist() == [[0, 1, 2, 3]]
    assert sc.view(np.int32).tolist() == [[0, 0, 0, 0]]              # every zero is returned as +0.0
    # a plain -0.0 with no bias at all is canonicalised too, and ties with +0.0
    ids, sc = ref.topk(np.array([[0.0, -0.0]], dtype=F), None, None, 2)
    assert ids.tolist() == [[0, 1]] and sc.view(np.int32).tolist() == [[0, 0]]
    # -0.0 + -0.0 is -0.0 in fp32: still returned as +0.0
    ids, sc = ref.topk(np.array([[-0.0]], dtype=F), np.array([-0.0], dtype=F), None, 1)
    assert sc.view(np.int32).tolist() == [[0]]


def test_ref_nan_bias_is_a_global_block_list():
    s = np.array([[5.0, 4.0, 3.0], [1.0, 9.0, 2.0]], dtype=F)
    bias = np.array([0.0, np.nan, 0.0], dtype=F)
    ids, sc = ref.topk(s, bias, None, 3)
    assert ids.tolist() == [[0, 2, -1], [2, 0, -1]]
    assert sc[:, 2].tolist() == [-np.inf, -np.inf]
    rk, rs = ref.ranks(s, bias, None, np.array([[1, 2], [1, 0]]))
    assert rk.tolist() == [[0, 2], [0, 2]] and rs[:, 0].tolist() == [-np.inf, -np.inf]


def test_ref_inf_minus_inf_is_nan_and_minus_inf_comes_last():
    s = np.array([[np.inf, 1.0, 2.0, -np.inf, 0.5]], dtype=F)
    bias = np.array([-np.inf, -np.inf, 0.0, np.inf, -np.inf], dtype=F)     # NaN, -inf, 2, NaN, -inf
    ids, sc = ref.topk(s, bias, None, 5)
    assert ids.tolist() == [[2, 1, 4, -1, -1]]
    assert sc.tolist() == [[2.0, -np.inf, -np.inf, -np.inf, -np.inf]]
    rk, rs = ref.ranks(s, bias, None, np.array([[0, 1, 2, 3, 4]]))
    assert rk.tolist() == [[0, 2, 1, 0, 3]]                           # a -inf sum is eligible and ranked, the smaller id first
    # +inf comes first
    assert ref.topk(np.array([[1.0, 2.0]], dtype=F), np.array([np.inf, 0.0], dtype=F), None, 1)[0].tolist() == [[0]]


def test_ref_fewer_than_k_eligible_excludes_and_bad_targets():
    s = np.array([[1.0, 2.0, 3.0, 4.0]], dtype=F)
    bias = np.array([0.25, 0.0, np.nan, -4.0], dtype=F)
    ex = np.array([[1, 1, -1, 4, 99]])                               # a duplicate, and ids outside [0, N)
    ids, sc = ref.topk(s, bias, ex, 4)
    assert ids.tolist() == [[0, 3, -1, -1]] and sc.tolist() == [[1.25, 0.0, -np.inf, -np.inf]]
    rk, rs = ref.ranks(s, bias, ex, np.array([[0, 1, 2, 3, -1, 4, 0]]))
    assert rk.tolist() == [[1, 0, 0, 2, 0, 0, 1]]                     # excluded, NaN bias, padding, out of range; a duplicate
    assert rs.tolist() == [[1.25, -np.inf, -np.inf, 0.0, -np.inf, -np.inf, 1.25]]


def test_ref_the_add_is_one_fp32_rounding():
    s = np.array([[16777216.0, 1.0]], dtype=F)                        # 2^24 + 1 is not a float32
    bias = np.array([1.0, 16777216.0], dtype=F)
    sc = ref.biased(s, bias)
    assert sc.dtype == np.float32 and sc.tolist() == [[16777216.0, 16777216.0]]
    assert ref.topk(s, bias, None, 2)[0].tolist() == [[0, 1]]          # merged into a tie, decided by the id


# ---- 2: the symbols ----------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_and_signatures():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)                # prototypes without their comments
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, name + " is not declared in include/nrms_hip.h"
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == m.group(2).count(",") + 1, name
    # the biased calls take exactly one more argument than the unbiased ones, and the queries the same
    assert len(_lib.SIGNATURES["nrms_topk_dot_biased"][1]) == len(_lib.SIGNATURES["nrms_topk_dot"][1]) + 1
    assert len(_lib.SIGNATURES["nrms_rank_dot_biased"][1]) == len(_lib.SIGNATURES["nrms_rank_dot"][1]) + 1
    assert _lib.SIGNATURES["nrms_topk_dot_biased_workspace_bytes"] == _lib.SIGNATURES["nrms_topk_dot_workspace_bytes"]
    assert _lib.SIGNATURES["nrms_rank_dot_biased_workspace_bytes"] == _lib.SIGNATURES["nrms_rank_dot_workspace_bytes"]
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


C_PROG = r"""
#include "nrms_hip.h"
#include <stdio.h>
#include <string.h>

static float u[8], it[8], sc[8], bi[8];
static int64_t tg[8], ex[8], ids[8];
static int32_t rk[8];
static uint64_t ws[4096];

static int expect(int rc, int want, const char* who, const char* word) {
    const char* msg = nrms_last_error();
    if (rc != want || !msg || !strstr(msg, word) || !strstr(msg, who)) {
        printf("FAIL %s %s: rc=%d (want %d) msg=%s\n", who, word, rc, want, msg ? msg : "(null)");
        return 1;
    }
    return 0;
}

int main(void) {
    int bad = 0;
    const size_t wb = sizeof ws;
    const int64_t big = (int64_t)0x7FFF0000 + 1;
    const float* odd = (const float*)(const void*)((const char*)bi + 1);
    const char* T = "topk_dot_biased";
    const char* R = "rank_dot_biased";
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 0, u, it, bi, NULL, 0, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "k");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 257, u, it, bi, NULL, 0, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "k");
    bad += expect(nrms_topk_dot_biased(2, 4, 0, 2, u, it, bi, NULL, 0, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "d");
    bad += expect(nrms_topk_dot_biased(2, big, 2, 2, u, it, bi, NULL, 0, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "N");
    bad += expect(nrms_topk_dot_biased(2, -1, 2, 2, u, it, bi, NULL, 0, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "N");
    bad += expect(nrms_topk_dot_biased(-1, 4, 2, 2, u, it, bi, NULL, 0, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "B");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 2, u, it, bi, ex, -1, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "n_exclude");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 2, NULL, it, bi, NULL, 0, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "user");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 2, u, NULL, bi, NULL, 0, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "items");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 2, u, it, odd, NULL, 0, sc, ids, ws, wb, NULL), NRMS_EINVAL, T, "bias");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 2, u, it, bi, NULL, 0, NULL, ids, ws, wb, NULL), NRMS_EINVAL, T, "top_scores");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 2, u, it, bi, NULL, 0, sc, NULL, ws, wb, NULL), NRMS_EINVAL, T, "top_ids");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 2, u, it, bi, NULL, 0, sc, ids, NULL, wb, NULL), NRMS_EINVAL, T, "workspace");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 2, u, it, bi, NULL, 0, sc, ids, (char*)ws + 4, wb - 8, NULL), NRMS_EINVAL, T, "workspace");
    bad += expect(nrms_topk_dot_biased(2, 4, 2, 2, u, it, bi, NULL, 0, sc, ids, ws,
                                       nrms_topk_dot_biased_workspace_bytes(2, 4, 2, 2) - 1, NULL), NRMS_EWORKSPACE, T, "workspace");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 0, u, it, bi, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "T");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 33, u, it, bi, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "T");
    bad += expect(nrms_rank_dot_biased(2, 4, 0, 2, u, it, bi, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "d");
    bad += expect(nrms_rank_dot_biased(2, big, 2, 2, u, it, bi, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "N");
    bad += expect(nrms_rank_dot_biased(2, -1, 2, 2, u, it, bi, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "N");
    bad += expect(nrms_rank_dot_biased(-1, 4, 2, 2, u, it, bi, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "B");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 2, u, it, bi, tg, ex, -1, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "n_exclude");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 2, NULL, it, bi, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "user");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 2, u, NULL, bi, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "items");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 2, u, it, odd, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "bias");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 2, u, it, bi, NULL, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, R, "targets");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 2, u, it, bi, tg, NULL, 0, NULL, sc, ws, wb, NULL), NRMS_EINVAL, R, "ranks");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 2, u, it, bi, tg, NULL, 0, rk, sc, NULL, wb, NULL), NRMS_EINVAL, R, "workspace");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 2, u, it, bi, tg, NULL, 0, rk, sc, (char*)ws + 4, wb - 8, NULL), NRMS_EINVAL, R, "workspace");
    bad += expect(nrms_rank_dot_biased(2, 4, 2, 2, u, it, bi, tg, ex, 2, rk, sc, ws,
                                       nrms_rank_dot_biased_workspace_bytes(2, 4, 2, 2, 2) - 1, NULL), NRMS_EWORKSPACE, R, "workspace");
    /* B = 0 is accepted: a no-op, whatever the pointers */
    if (nrms_topk_dot_biased(0, 4, 2, 2, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL) != NRMS_OK) { printf("FAIL topk B=0\n"); ++bad; }
    if (nrms_rank_dot_biased(0, 4, 2, 2, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL) != NRMS_OK) { printf("FAIL rank B=0\n"); ++bad; }
    /* the queries are the unbiased ones, accepted and rejected arguments alike */
    {
        const int32_t Bs[] = {-1, 0, 1, 70, 512}, ds[] = {0, 1, 300}, ks[] = {0, 1, 10, 256, 257}, Ts[] = {0, 1, 8, 32, 33}, xs[] = {-1, 0, 50, 70};
        const int64_t Ns[] = {-1, 0, 1, 5000, 130000, (int64_t)0x7FFF0000, (int64_t)0x7FFF0000 + 1};
        int a, b, c, e, f, n_acc = 0, n_rej = 0;
        for (a = 0; a < 5; ++a) for (b = 0; b < 7; ++b) for (c = 0; c < 3; ++c) for (e = 0; e < 5; ++e) {
            const size_t q = nrms_topk_dot_biased_workspace_bytes(Bs[a], Ns[b], ds[c], ks[e]);
            if (q != nrms_topk_dot_workspace_bytes(Bs[a], Ns[b], ds[c], ks[e])) { printf("FAIL topk query\n"); ++bad; }
            if (q) ++n_acc; else ++n_rej;
            for (f = 0; f < 4; ++f) {
                const size_t p = nrms_rank_dot_biased_workspace_bytes(Bs[a], Ns[b], ds[c], Ts[e], xs[f]);
                if (p != nrms_rank_dot_workspace_bytes(Bs[a], Ns[b], ds[c], Ts[e], xs[f])) { printf("FAIL rank query\n"); ++bad; }
                if (p) ++n_acc; else ++n_rej;
            }
        }
        printf("QUERIES %d %d\n", n_acc, n_rej);
    }
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_biased_c_abi_validation_and_workspace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "bias_abi.c", tmp_path / "bias_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    acc, rej = (int(v) for v in out.split("QUERIES ")[1].split("\n")[0].split())
    assert acc > 0 and rej > 0, out                                     # both kinds of argument were compared


def test_biased_queries_through_ctypes():
    import ctypes as C
    lib = _lib.load()
    assert lib.nrms_topk_dot_biased_workspace_bytes(70, C.c_int64(5000), 40, 10) == lib.nrms_topk_dot_workspace_bytes(70, C.c_int64(5000), 40, 10) > 0
    assert lib.nrms_topk_dot_biased_workspace_bytes(70, C.c_int64(5000), 40, 257) == 0
    assert lib.nrms_rank_dot_biased_workspace_bytes(70, C.c_int64(5000), 40, 5, 70) == lib.nrms_rank_dot_workspace_bytes(70, C.c_int64(5000), 40, 5, 70) > 0
    assert lib.nrms_rank_dot_biased_workspace_bytes(70, C.c_int64(5000), 40, 33, 70) == 0


# ---- 3: the CLI's checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,ok", [
    (["--negatives", "catalogue", "--retrieval_metrics", "10", "--popularity_prior", "0.5"], True),
    (["--negatives", "adaptive", "--recommend", "5", "--popularity_prior", "1"], True),
    (["--negatives", "catalogue", "--recommend", "5", "--diversity", "0.5", "--popularity_prior", "0"], True),
    (["--negatives", "catalogue", "--recommend", "5", "--popularity_prior", "-0.25"], True),
    (["--model", "nrms_v1", "--negatives", "catalogue", "--recommend", "5", "--popularity_prior", "0.5"], True),
    (["--model", "nrms_naml", "--negatives", "catalogue", "--retrieval_metrics", "10", "--popularity_prior", "0.5"], True),
    (["--model", "nrms_bert", "--negatives", "catalogue", "--retrieval_metrics", "10", "--popularity_prior", "0.5"], True),
    (["--negatives", "catalogue", "--recommend", "5"], True),                                       # no prior: nothing to check
    (["--negatives", "catalogue", "--recommend", "5", "--popularity_prior", "nan"], False),
    (["--negatives", "catalogue", "--recommend", "5", "--popularity_prior", "inf"], False),
    (["--negatives", "catalogue", "--retrieval_metrics", "10", "--popularity_prior=-inf"], False),
    (["--negatives", "catalogue", "--popularity_prior", "0.5"], False),                             # nothing to apply it to
    (["--recommend", "5", "--popularity_prior", "0.5"], False),                                     # --negatives fixed: no click log
    (["--negatives", "epoch", "--recommend", "5", "--popularity_prior", "0.5"], False),             # an impression feed
    (["--model", "hierec", "--negatives", "catalogue", "--recommend", "5", "--popularity_prior", "0.5"], False),
    (["--model", "graph", "--negatives", "catalogue", "--recommend", "5", "--popularity_prior", "0.5"], False),
])
def test_check_prior_args(argv, ok):
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(["--dataset", "synthetic"] + ([] if "--model" in argv else ["--model", "nrms_hip"]) + argv)
    if ok:
        assert run_v0.check_prior_args(args) is None
    else:
        with pytest.raises(SystemExit) as e:
            run_v0.check_prior_args(args)
        assert "--popularity_prior" in str(e.value)


# ---- 4: ClickFeed.popularity_prior ---------------------------------------------------------------------------------------------
def _small_log():
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.data_handler import ClickFeed, SyntheticMind
    cfg = Config("nrms_hip")
    cfg.__nrms__()
    cfg.n_words, cfg.n_words_title, cfg.n_words_abst, cfg.history_len, cfg.sample_size = 600, 12, 16, 10, 4
    corpus = SyntheticMind(cfg, n_news=300, seed=4)
    user_ptr, clicks = corpus.click_log(30, min_clicks=6, max_clicks=70)
    clicks = clicks.copy()
    never = int(np.setdiff1d(np.arange(1, 301), clicks)[0])          # a news nobody clicked ...
    clicks[user_ptr[4] - 1] = never                                  # ... becomes the LAST click of user 3: held out only
    feed = ClickFeed(cfg, user_ptr, clicks, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, batch_size=8,
                     device="cpu", holdout=1, min_history=1)
    return feed, user_ptr, clicks, never


def test_popularity_prior_against_numpy():
    feed, user_ptr, clicks, never = _small_log()
    N = 301
    # count by hand: the distinct news of every user's training part (all but the last click)
    count = np.zeros(N, dtype=np.int64)
    for u in range(len(user_ptr) - 1):
        for n in set(clicks[user_ptr[u]:user_ptr[u + 1] - 1].tolist()):
            count[n] += 1
    assert count.max() > 1 and (count[1:] == 0).any()
    for alpha in (0.5, 1.0, -0.25, 3.0):
        p = feed.popularity_prior(alpha)
        assert p.dtype == torch.float32 and tuple(p.shape) == (N,) and p.device == feed.device and p.is_contiguous()
        want = (np.float64(alpha) * np.log1p(count.astype(np.float64))).astype(np.float32)
        want[0] = 0.0
        assert p.numpy().tobytes() == want.tobytes()
        assert p[0].item() == 0.0 and p[never].item() == 0.0         # padding; clicked in a held-out position only: no leak
    z = feed.popularity_prior(0)
    assert z.dtype == torch.float32 and tuple(z.shape) == (N,) and (z == 0).all()
    hot = int(np.argmax(count))
    assert feed.popularity_prior(1.0)[hot].item() == pytest.approx(np.log1p(count[hot]), rel=1e-6)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            feed.popularity_prior(bad)


# ---- 5: the loops' default path ---------------------------------------------------------------------------------------------
class _StubEngine:
    retrieval_metrics = staticmethod(NRMSEngine.retrieval_metrics)

    def check_ids(self):
        pass


class _Stub:
    """A model from before the prior: recommend and rank_targets take no item_bias, so the loops must not pass one."""

    def __init__(self):
        self.engine, self.calls = _StubEngine(), []

    def encode_catalogue(self, titles):
        return torch.zeros(titles.shape[0], 4)

    def recommend(self, batch, k, catalogue, exclude_history=True, *, diversity=None, shortlist=None, return_ild=False):
        self.calls.append(("recommend", diversity))
        B = batch["candidate_ids"].shape[0]
        ids = torch.arange(1, k + 1).expand(B, k).contiguous()
        out = (ids, torch.zeros(B, k))
        return out + (torch.full((B,), 0.5),) if return_ild else out

    def rank_targets(self, batch, targets, catalogue, exclude_history=True):
        self.calls.append(("rank_targets", None))
        return torch.where(targets >= 0, torch.ones_like(targets), torch.zeros_like(targets)).to(torch.int32), None

    def check_recommend_ids(self):
        pass


class _Prior(_Stub):
    def recommend(self, batch, k, catalogue, exclude_history=True, *, diversity=None, shortlist=None, return_ild=False, item_bias=None):
        self.seen = item_bias
        return _Stub.recommend(self, batch, k, catalogue, exclude_history, diversity=diversity, shortlist=shortlist, return_ild=return_ild)

    def rank_targets(self, batch, targets, catalogue, exclude_history=True, *, item_bias=None):
        self.seen = item_bias
        return _Stub.rank_targets(self, batch, targets, catalogue, exclude_history)


def test_loops_pass_no_keyword_without_a_prior(tmp_path):
    titles = torch.zeros(20, 3, dtype=torch.int64)
    batches = [{"candidate_ids": torch.tensor([[3, 4, 5], [6, 7, 0]])}, {"candidate_ids": torch.tensor([[8, 9, 1]])}]
    labels = [[0, 1, 0], [1, 1], [0, 0, 1]]
    stub = _Stub()
    out = train_eval.recommend(None, stub, batches, titles, 4, out_file=str(tmp_path / "a.txt"))
    assert open(out).read().splitlines() == ["1 [1,2,3,4]", "2 [1,2,3,4]", "3 [1,2,3,4]"]
    train_eval.recommend(None, stub, batches, titles, 4, out_file=str(tmp_path / "b.txt"), diversity=0.5)
    res = train_eval.evaluate_retrieval(None, stub, batches, titles, labels, ks=(1,), verbose=False)
    assert res["n_targets"] == 4 and res["recall@1"] == 1.0
    assert [c[0] for c in stub.calls] == ["recommend"] * 4 + ["rank_targets"] * 2
    # the stub cannot take the keyword: giving a prior reaches it and fails there, not silently
    p = torch.ones(20)
    with pytest.raises(TypeError, match="item_bias"):
        train_eval.recommend(None, stub, batches, titles, 4, out_file=str(tmp_path / "c.txt"), item_bias=p)
    with pytest.raises(TypeError, match="item_bias"):
        train_eval.evaluate_retrieval(None, stub, batches, titles, labels, ks=(1,), verbose=False, item_bias=p)
    # a model that takes it gets the very tensor, from all three call sites
    m = _Prior()
    train_eval.recommend(None, m, batches, titles, 4, out_file=str(tmp_path / "d.txt"), item_bias=p)
    assert m.seen is p
    m.seen = None
    train_eval.recommend(None, m, batches, titles, 4, out_file=str(tmp_path / "e.txt"), diversity=0.5, item_bias=p)
    assert m.seen is p
    m.seen = None
    train_eval.evaluate_retrieval(None, m, batches, titles, labels, ks=(1,), verbose=False, item_bias=p)
    assert m.seen is p


def test_models_that_cannot_take_a_prior_refuse_it():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip
    for mod in (hierec_hip, graph_hip):
        assert not mod.Model.CATALOGUE_RANKING and not mod.Model.CATALOGUE_SAMPLING
        with pytest.raises(_lib.NrmsError, match="item_bias"):
            mod.Model.rank_targets(None, {}, None, None, item_bias=torch.zeros(3))
        with pytest.raises(_lib.NrmsError, match="item_bias"):
            mod.Model.recommend(None, {}, 5, None, item_bias=torch.zeros(3))
        with pytest.raises(NotImplementedError, match="rank_targets"):      # without it: as before
            mod.Model.rank_targets(None, {}, None, None)
