"""CPU-only checks of the diversified re-ranking (include/nrms_hip.h nrms_mmr_rerank): the numpy restatement's own properties, a
C99 program linked against libnrms_hip.so for the argument validation and the workspace query, the bindings, and run_v0's flags."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pytorch_news_recommender_amd import _lib
from tests import mmr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed=0, N=200, d=24, M=40):
    rng = np.random.default_rng(seed)
    items = rng.standard_normal((N, d)).astype(np.float32)
    ids = rng.choice(N, size=M, replace=False).astype(np.int64)
    scores = rng.standard_normal(M).astype(np.float32)
    return items, ids, scores


def test_reference_lambda_one_is_the_sorted_prefix():
    items, ids, scores = _case()
    order = np.argsort(-scores, kind="stable")
    ids, scores = ids[order], scores[order]                    # a shortlist as nrms_topk_dot returns it
    ids[7], scores[11] = -1, np.nan                            # two broken entries
    ids[30:], scores[30:] = -1, -np.inf
    r = mmr_ref.mmr_row(items, ids, scores, 1.0, 12)
    keep = [i for i in range(30) if i not in (7, 11)][:12]
    assert r["picks"] == keep
    assert np.array_equal(r["ids"], ids[keep]) and r["scores"].tobytes() == scores[keep].tobytes()
    r = mmr_ref.mmr_row(items, ids, scores, 1.0, 40)
    assert r["picks"] == [i for i in range(30) if i not in (7, 11)]
    assert (r["ids"][28:] == -1).all() and (r["scores"][28:] == -np.inf).all() and (r["value"][28:] == -np.inf).all()


def test_reference_is_permutation_invariant_and_handles_padding():
    items, ids, scores = _case(1)
    base = mmr_ref.mmr_row(items, ids, scores, 0.4, 15)
    perm = np.random.default_rng(2).permutation(len(ids))
    moved = mmr_ref.mmr_row(items, ids[perm], scores[perm], 0.4, 15)
    assert np.array_equal(base["ids"], moved["ids"]) and base["scores"].tobytes() == moved["scores"].tobytes()
    assert [int(perm[p]) for p in moved["picks"]] == base["picks"]
    assert abs(float(base["ild"]) - float(moved["ild"])) < 1e-12
    # padding in between changes nothing but the positions
    wide_ids = np.concatenate([[-1, 10 ** 12], ids[:20], [-5, len(items)], ids[20:], [3]])
    wide_scores = np.concatenate([[0.5, 0.5], scores[:20], [9.0, 9.0], scores[20:], [np.inf]]).astype(np.float32)
    wide = mmr_ref.mmr_row(items, wide_ids, wide_scores, 0.4, 15)
    assert np.array_equal(base["ids"], wide["ids"]) and np.array_equal(base["value"], wide["value"])
    none = mmr_ref.mmr_row(items, np.full(5, -1), np.full(5, -np.inf, dtype=np.float32), 0.4, 3)
    assert none["picks"] == [] and (none["ids"] == -1).all() and np.isnan(none["ild"])
    one = mmr_ref.mmr_row(items, ids[:1], scores[:1], 0.4, 1)
    assert one["picks"] == [0] and one["value"][0] == 0.0 and np.isnan(one["ild"])
    # ties go to the smaller position, duplicates are separate entries of cosine 1
    dup = mmr_ref.mmr_row(items, np.array([4, 4, 9]), np.array([1.0, 1.0, 0.0], dtype=np.float32), 0.5, 3)
    assert dup["picks"] == [0, 2, 1] or dup["picks"] == [0, 1, 2]
    assert dup["picks"][0] == 0 and abs(dup["value"][dup["picks"].index(1)] - (0.5 - 0.5)) < 1e-6
    gap, value, ild = mmr_ref.greedy_gap(items, ids, scores, 0.4, base["picks"])
    assert (gap == 0).all() and np.array_equal(value, base["value"]) and ild == base["ild"]
    worse = list(base["picks"])
    worse[3], worse[9] = worse[9], worse[3]
    assert mmr_ref.greedy_gap(items, ids, scores, 0.4, worse)[0].max() > 0


@pytest.mark.parametrize("M,d", [(2, 1), (33, 3), (65, 31), (256, 64)])
def test_lattice_generator_is_exact_in_fp32(M, d):
    """What tests/test_hip_mmr.py relies on: the float32 and the float64 evaluation of the reference agree bit for bit."""
    items, ids, scores = mmr_ref.lattice_case(37, M, d)
    valid = mmr_ref.valid_mask(ids, scores, len(items))
    assert not valid[min(M, 30) + 1].any() and valid[0].sum() > 0 and (ids == 2 ** 40).any() and np.isnan(scores).any()
    for lam in (0.0, 0.25, 0.5, 1.0):
        for k in sorted({1, min(7, M), M}):
            a = mmr_ref.mmr_batch(items, ids, scores, lam, k)
            b = mmr_ref.mmr_batch(items, ids, scores, lam, k, np.float32)
            assert np.array_equal(a["ids"], b["ids"]) and a["scores"].tobytes() == b["scores"].tobytes()
            assert np.array_equal(a["value"], b["value"].astype(np.float64))
            assert a["picks"] == b["picks"]


C_PROG = r"""
#include "nrms_hip.h"
#include <math.h>
#include <stdio.h>
#include <string.h>

static float it[64], sc[64], osc[64], oval[64], ild[8];
static int64_t ids[64], oids[64];
static uint64_t ws[1 << 16];

static int expect(int rc, const char* word) {
    const char* msg = nrms_last_error();
    if (rc != NRMS_EINVAL || !msg || !strstr(msg, word)) { printf("FAIL %s: rc=%d msg=%s\n", word, rc, msg ? msg : "(null)"); return 1; }
    return 0;
}

int main(void) {
    int bad = 0;
    const size_t wb = sizeof ws;
    bad += expect(nrms_mmr_rerank(-1, 8, 4, 3, 16, 0.5f, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "B");
    bad += expect(nrms_mmr_rerank(2, 0, 4, 3, 16, 0.5f, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "M");
    bad += expect(nrms_mmr_rerank(2, 257, 4, 3, 16, 0.5f, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "M");
    bad += expect(nrms_mmr_rerank(2, 8, 0, 3, 16, 0.5f, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "d");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 0, 16, 0.5f, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "k");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 9, 16, 0.5f, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "k");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, -1, 0.5f, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "N");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, -0.25f, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "lambda");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, 1.5f, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "lambda");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, (float)NAN, it, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "lambda");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, 0.5f, NULL, ids, sc, oids, osc, oval, ild, ws, wb, NULL), "items");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, 0.5f, it, NULL, sc, oids, osc, oval, ild, ws, wb, NULL), "short_ids");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, 0.5f, it, ids, NULL, oids, osc, oval, ild, ws, wb, NULL), "short_scores");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, 0.5f, it, ids, sc, NULL, osc, oval, ild, ws, wb, NULL), "out_ids");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, 0.5f, it, ids, sc, oids, NULL, oval, ild, ws, wb, NULL), "out_scores");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, 0.5f, it, ids, sc, oids, osc, oval, ild, NULL, wb, NULL), "workspace");
    bad += expect(nrms_mmr_rerank(2, 8, 4, 3, 16, 0.5f, it, ids, sc, oids, osc, oval, ild, (char*)ws + 4, wb - 4, NULL), "aligned");
    {   /* too small a workspace is its own error code, and B = 0 is a no-op that needs no pointer */
        const int rc = nrms_mmr_rerank(2, 8, 4, 3, 16, 0.5f, it, ids, sc, oids, osc, oval, ild, ws, 8, NULL);
        const char* msg = nrms_last_error();
        if (rc != NRMS_EWORKSPACE || !msg || !strstr(msg, "workspace")) { printf("FAIL small workspace: rc=%d\n", rc); ++bad; }
        if (nrms_mmr_rerank(0, 8, 4, 3, 16, 0.5f, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL) != NRMS_OK) { printf("FAIL B=0\n"); ++bad; }
    }
    printf("WS %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n",
           nrms_mmr_rerank_workspace_bytes(512, 0, 300, 1), nrms_mmr_rerank_workspace_bytes(512, 257, 300, 10),
           nrms_mmr_rerank_workspace_bytes(512, 256, 0, 10), nrms_mmr_rerank_workspace_bytes(512, 256, 300, 0),
           nrms_mmr_rerank_workspace_bytes(512, 256, 300, 257), nrms_mmr_rerank_workspace_bytes(-1, 256, 300, 10),
           nrms_mmr_rerank_workspace_bytes(512, 256, 300, 10), nrms_mmr_rerank_workspace_bytes(512, 256, 300, 256),
           nrms_mmr_rerank_workspace_bytes(1, 256, 300, 10), nrms_mmr_rerank_workspace_bytes(1, 1, 1, 1),
           nrms_mmr_rerank_workspace_bytes(0, 256, 300, 10));
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_mmr_c_abi_validation_and_workspace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "mmr_abi.c", tmp_path / "mmr_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    ws = [int(v) for v in out.split("WS ")[1].split("\n")[0].split()]
    assert ws[:6] == [0] * 6                                       # M = 0, M = 257, d = 0, k = 0, k > M, B < 0 rejected
    assert all(v > 0 for v in ws[6:])                              # ... B = 0 included: accepted arguments never report 0
    assert ws[6] == ws[7]                                          # k does not size it
    assert ws[6] > ws[8] > ws[9]                                   # grows with B and with M
    assert ws[8] <= 256 + 256 * 256 * 4                            # one Gram matrix per user, nothing of the catalogue's size


def test_mmr_signatures_are_bound():
    lib = _lib.load()
    assert lib.nrms_mmr_rerank_workspace_bytes(4, 100, 8, 10) > 0
    assert lib.nrms_mmr_rerank_workspace_bytes(4, 100, 8, 101) == 0
    assert lib.nrms_mmr_rerank.argtypes == _lib.SIGNATURES["nrms_mmr_rerank"][1] and len(lib.nrms_mmr_rerank.argtypes) == 16
    assert "mmr.hip" in open(os.path.join(ROOT, "pytorch_news_recommender_amd", "build.py")).read()


@pytest.mark.parametrize("argv,ok", [
    (["--model", "nrms_hip", "--recommend", "10", "--diversity", "0.5"], True),
    (["--model", "nrms_v1", "--recommend", "10", "--diversity", "0", "--shortlist", "10"], True),
    (["--model", "nrms_bert", "--recommend", "10", "--diversity", "1", "--shortlist", "256"], True),
    (["--model", "nrms_hip", "--recommend", "10", "--diversity", "1.5"], False),
    (["--model", "nrms_hip", "--recommend", "10", "--diversity", "-0.1"], False),
    (["--model", "nrms_hip", "--diversity", "0.5"], False),
    (["--model", "nrms_hip", "--recommend", "10", "--diversity", "0.5", "--shortlist", "9"], False),
    (["--model", "nrms_hip", "--recommend", "10", "--diversity", "0.5", "--shortlist", "257"], False),
    (["--model", "nrms_hip", "--recommend", "10", "--shortlist", "40"], False),
    (["--model", "hierec", "--recommend", "10", "--diversity", "0.5"], False),
    (["--model", "hierec", "--diversity", "0.5"], False),
    (["--model", "graph", "--recommend", "10", "--diversity", "0.5"], False),
])
def test_run_v0_checks_diversity_before_reading_data(argv, ok):
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(argv)
    if ok:
        run_v0.check_recommend_args(args)
    else:
        with pytest.raises(SystemExit) as e:
            run_v0.check_recommend_args(args)
        assert "--diversity" in str(e.value) or "--shortlist" in str(e.value)
    if not ok:
        with pytest.raises(SystemExit):                         # main() checks before it touches the GPU or any data
            run_v0.main(argv + ["--dataset", "synthetic"])
