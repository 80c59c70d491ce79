"""CPU-only checks of catalogue ranking (include/nrms_hip.h nrms_rank_dot): a C99 program linked against libnrms_hip.so gets
the argument validation and the workspace query, NRMSEngine.retrieval_metrics is compared with numpy float64 on hand-made
ranks, and run_v0 checks --retrieval_metrics before any data is read."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.engine import NRMSEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PROG = r"""
#include "nrms_hip.h"
#include <stdio.h>
#include <string.h>

static float u[8], it[8], sc[8];
static int64_t tg[8], ex[8];
static int32_t rk[8];
static uint64_t ws[4096];

static int expect(int rc, int want, const char* word) {
    const char* msg = nrms_last_error();
    if (rc != want || !msg || !strstr(msg, word)) {
        printf("FAIL %s: rc=%d (want %d) msg=%s\n", word, rc, want, msg ? msg : "(null)");
        return 1;
    }
    return 0;
}

int main(void) {
    int bad = 0;
    const size_t wb = sizeof ws;
    const int64_t big = (int64_t)0x7FFF0000 + 1;
    bad += expect(nrms_rank_dot(2, 4, 2, 0, u, it, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, "T");
    bad += expect(nrms_rank_dot(2, 4, 2, 33, u, it, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, "T");
    bad += expect(nrms_rank_dot(2, 4, 0, 2, u, it, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, "d");
    bad += expect(nrms_rank_dot(2, big, 2, 2, u, it, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, "N");
    bad += expect(nrms_rank_dot(2, -1, 2, 2, u, it, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, "N");
    bad += expect(nrms_rank_dot(-1, 4, 2, 2, u, it, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, "B");
    bad += expect(nrms_rank_dot(2, 4, 2, 2, u, it, tg, ex, -1, rk, sc, ws, wb, NULL), NRMS_EINVAL, "n_exclude");
    bad += expect(nrms_rank_dot(2, 4, 2, 2, u, it, tg, NULL, 0, NULL, sc, ws, wb, NULL), NRMS_EINVAL, "ranks");
    bad += expect(nrms_rank_dot(2, 4, 2, 2, u, it, NULL, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, "targets");
    bad += expect(nrms_rank_dot(2, 4, 2, 2, NULL, it, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, "user");
    bad += expect(nrms_rank_dot(2, 4, 2, 2, u, NULL, tg, NULL, 0, rk, sc, ws, wb, NULL), NRMS_EINVAL, "items");
    bad += expect(nrms_rank_dot(2, 4, 2, 2, u, it, tg, NULL, 0, rk, sc, NULL, wb, NULL), NRMS_EINVAL, "workspace");
    bad += expect(nrms_rank_dot(2, 4, 2, 2, u, it, tg, ex, 2, rk, sc, ws, 8, NULL), NRMS_EWORKSPACE, "workspace");
    bad += expect(nrms_rank_dot(2, 4, 2, 2, u, it, tg, ex, 2, rk, sc, ws,
                                nrms_rank_dot_workspace_bytes(2, 4, 2, 2, 2) - 1, NULL), NRMS_EWORKSPACE, "workspace");
    /* B = 0 is accepted: a no-op, whatever the pointers */
    if (nrms_rank_dot(0, 4, 2, 2, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL) != NRMS_OK) { printf("FAIL B=0\n"); ++bad; }
    printf("WS %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n",
           nrms_rank_dot_workspace_bytes(512, 130000, 300, 0, 50), nrms_rank_dot_workspace_bytes(512, 130000, 300, 33, 50),
           nrms_rank_dot_workspace_bytes(512, 130000, 0, 8, 50), nrms_rank_dot_workspace_bytes(512, big, 300, 8, 50),
           nrms_rank_dot_workspace_bytes(-1, 130000, 300, 8, 50), nrms_rank_dot_workspace_bytes(512, 130000, 300, 8, -1),
           nrms_rank_dot_workspace_bytes(512, 130000, 300, 8, 50), nrms_rank_dot_workspace_bytes(512, 130000, 300, 32, 50),
           nrms_rank_dot_workspace_bytes(1024, 130000, 300, 8, 50), nrms_rank_dot_workspace_bytes(512, 130000, 300, 8, 0),
           nrms_rank_dot_workspace_bytes(0, 0, 1, 1, 0));
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_rank_c_abi_validation_and_workspace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "rank_abi.c", tmp_path / "rank_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    ws = [int(v) for v in out.split("WS ")[1].split("\n")[0].split()]
    assert ws[:6] == [0] * 6                  # T = 0, T = 33, d = 0, N past the limit, B < 0, n_exclude < 0: rejected
    assert all(v > 0 for v in ws[6:])         # never 0 for accepted arguments (B = 0 and N = 0 included)
    assert ws[7] > ws[6] and ws[8] > ws[6] and ws[6] > ws[9]          # grows with T, B and n_exclude
    assert ws[7] < 512 * 130000 * 4 // 100                             # far from a [B, N] score matrix


def test_rank_signatures_are_bound():
    lib = _lib.load()
    assert lib.nrms_rank_dot_workspace_bytes(4, 100, 8, 5, 3) > 0
    assert lib.nrms_rank_dot_workspace_bytes(4, 100, 8, 0, 3) == 0
    assert lib.nrms_rank_dot_workspace_bytes(4, 100, 8, 33, 3) == 0
    assert lib.nrms_rank_dot.argtypes == _lib.SIGNATURES["nrms_rank_dot"][1]


def _host_metrics(ranks, ks):
    """The definition, user by user, in numpy float64."""
    out = {"mrr": []}
    for k in ks:
        out["recall@%d" % k], out["ndcg@%d" % k] = [], []
    for row in np.asarray(ranks):
        r = row[row > 0].astype(np.float64)
        n_t = r.size
        if n_t == 0:
            for v in out.values():
                v.append(np.nan)
            continue
        out["mrr"].append(np.sum(1.0 / r) / n_t)
        for k in ks:
            out["recall@%d" % k].append(np.sum(r <= k) / n_t)
            ideal = np.sum(1.0 / np.log2(np.arange(1, min(n_t, k) + 1, dtype=np.float64) + 1.0))
            out["ndcg@%d" % k].append(np.sum(1.0 / np.log2(r[r <= k] + 1.0)) / ideal)
    return {k: np.asarray(v) for k, v in out.items()}


def test_retrieval_metrics_against_numpy():
    ks = (1, 3, 10, 1000)
    ranks = np.array([[0, 0, 0, 0, 0],            # no ranked target: NaN everywhere
                      [3, 0, 0, 0, 0],            # a rank exactly k = 3
                      [1, 2, 3, 4, 5],            # n_t = 5 > k = 1 and 3: the ideal list is cut at k
                      [10, 11, 1000, 1001, 0],    # ranks exactly k = 10 and k = 1000, and one past each
                      [7, 0, 130000, 0, 2],       # padding between targets, a rank deep in the catalogue
                      [1, 0, 0, 0, 0]], dtype=np.int32)
    got = NRMSEngine.retrieval_metrics(torch.from_numpy(ranks), ks)
    want = _host_metrics(ranks, ks)
    assert set(got) == set(want)
    for name, w in want.items():
        g = got[name]
        assert g.dtype == torch.float64 and g.shape == (ranks.shape[0],)
        np.testing.assert_allclose(g.numpy(), w, rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
    assert np.isnan(got["mrr"][0].item()) and np.isnan(got["recall@3"][0].item()) and np.isnan(got["ndcg@10"][0].item())
    assert got["recall@3"][1].item() == 1.0 and got["recall@1"][1].item() == 0.0
    assert got["ndcg@3"][1].item() == pytest.approx(0.5, abs=1e-12)            # 1 / log2(4) over 1 / log2(2)
    assert got["ndcg@3"][2].item() == pytest.approx(1.0, abs=1e-12)            # the three best places, all hits
    assert got["recall@3"][2].item() == pytest.approx(0.6, abs=1e-12)
    assert got["ndcg@1"][5].item() == 1.0 and got["mrr"][5].item() == 1.0
    with pytest.raises(ValueError):
        NRMSEngine.retrieval_metrics(torch.from_numpy(ranks), (0,))


@pytest.mark.parametrize("model,ks,ok", [("nrms_hip", "10,100", True), ("nrms_v1", "1000", True), ("nrms_hip", "0", False),
                                         ("nrms_hip", "a,b", False), ("nrms_hip", "10,0", False), ("hierec", "10", False),
                                         ("graph", "10", False)])
def test_run_v0_checks_retrieval_metrics_before_training(model, ks, ok):
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(["--model", model, "--retrieval_metrics", ks])
    if ok:
        assert run_v0.check_retrieval_args(args) == tuple(int(v) for v in ks.split(","))
    else:
        with pytest.raises(SystemExit):
            run_v0.check_retrieval_args(args)


def test_models_say_whether_they_rank_the_catalogue():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip, nrms_bert_hip, nrms_hip, nrms_naml_hip, nrms_v1_hip
    for mod in (nrms_hip, nrms_v1_hip, nrms_naml_hip, nrms_bert_hip):
        assert mod.Model.CATALOGUE_RANKING is True and callable(mod.Model.rank_targets)
    for mod in (hierec_hip, graph_hip):
        assert not mod.Model.CATALOGUE_RANKING
        with pytest.raises(NotImplementedError, match="rank_targets"):
            mod.Model.rank_targets(None, {}, None, None)
