"""CPU-only checks of the catalogue top-k entry point (include/nrms_hip.h nrms_topk_dot): a C99 program linked against
libnrms_hip.so gets the argument validation and the workspace query, and nrms_naml refuses catalogue retrieval."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pytorch_news_recommender_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PROG = r"""
#include "nrms_hip.h"
#include <stdio.h>
#include <string.h>

static float u[8], it[8], sc[8];
static int64_t ids[8];
static uint64_t ws[4096];

static int expect(int rc, const char* word) {
    const char* msg = nrms_last_error();
    if (rc == 0 || !msg || !strstr(msg, word)) { printf("FAIL %s: rc=%d msg=%s\n", word, rc, msg ? msg : "(null)"); return 1; }
    return 0;
}

int main(void) {
    int bad = 0;
    const size_t wb = sizeof ws;
    bad += expect(nrms_topk_dot(2, 4, 2, 0, u, it, NULL, 0, sc, ids, ws, wb, NULL), "k");
    bad += expect(nrms_topk_dot(2, 4, 2, 257, u, it, NULL, 0, sc, ids, ws, wb, NULL), "k");
    bad += expect(nrms_topk_dot(2, 4, 0, 3, u, it, NULL, 0, sc, ids, ws, wb, NULL), "d");
    bad += expect(nrms_topk_dot(2, 4, 2, 3, NULL, it, NULL, 0, sc, ids, ws, wb, NULL), "user");
    bad += expect(nrms_topk_dot(2, 4, 2, 3, u, NULL, NULL, 0, sc, ids, ws, wb, NULL), "items");
    bad += expect(nrms_topk_dot(2, 4, 2, 3, u, it, NULL, 0, NULL, ids, ws, wb, NULL), "top_scores");
    bad += expect(nrms_topk_dot(2, 4, 2, 3, u, it, NULL, 0, sc, NULL, ws, wb, NULL), "top_ids");
    bad += expect(nrms_topk_dot(2, 4, 2, 3, u, it, NULL, 0, sc, ids, ws, 8, NULL), "workspace");
    printf("WS %zu %zu %zu %zu %zu %zu %zu %zu %zu\n",
           nrms_topk_dot_workspace_bytes(512, 130000, 300, 0), nrms_topk_dot_workspace_bytes(512, 130000, 300, 257),
           nrms_topk_dot_workspace_bytes(512, 130000, 0, 10),
           nrms_topk_dot_workspace_bytes(512, 130000, 300, 10), nrms_topk_dot_workspace_bytes(512, 130000, 300, 100),
           nrms_topk_dot_workspace_bytes(1, 130000, 300, 100), nrms_topk_dot_workspace_bytes(100000, 130000, 300, 100),
           nrms_topk_dot_workspace_bytes(512, 1, 300, 100), nrms_topk_dot_workspace_bytes(512, 10000000, 300, 100));
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_topk_c_abi_validation_and_workspace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "topk_abi.c", tmp_path / "topk_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    ws = [int(v) for v in out.split("WS ")[1].split("\n")[0].split()]
    assert ws[:3] == [0, 0, 0]                                     # k = 0, k = 257, d = 0 rejected
    assert all(v > 0 for v in ws[3:])
    assert ws[4] > ws[3]                                           # grows with k
    assert ws[6] > ws[5]                                           # ... with B
    assert ws[8] > ws[7]                                           # ... with N
    assert ws[4] < 512 * 130000 * 4 // 4                           # far from a [B, N] score matrix


def test_top_k_signatures_are_bound():
    lib = _lib.load()
    assert lib.nrms_topk_dot_workspace_bytes(4, 100, 8, 10) > 0
    assert lib.nrms_topk_dot_workspace_bytes(4, 100, 8, 0) == 0


def test_nrms_naml_recommend_is_not_implemented(tmp_path):
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.model.nrms_naml_hip import Model
    shape = synth.G7_ODD
    params = synth.make_params_naml(shape, seed=21)
    cfg = Config("nrms_naml")
    cfg.__nrms__()
    for k in ("word_embed_size", "title_heads_num", "query_vector_dim", "category_nums", "subcategory_nums",
              "cate_embed_size", "user_heads_num", "query_vector_dim_large"):
        setattr(cfg, k, getattr(shape, k))
    cfg.news_feature_size = shape.news_feature_size
    np.savez(tmp_path / "all_word_embedding_v3.npz", embeddings=params["news_encoder.word_embedding.weight"])
    cfg.data_path = str(tmp_path) + "/"
    m = Model(cfg)
    with pytest.raises(NotImplementedError, match="category"):
        m.recommend({"browsed_ids": np.zeros((2, 3), np.int64)}, 5, None)
    with pytest.raises(NotImplementedError, match="category"):
        m.encode_catalogue(np.zeros((4, 3), np.int64))


@pytest.mark.parametrize("model,k,ok", [("nrms_hip", 10, True), ("nrms_v1", 256, True), ("nrms_hip", 0, False),
                                        ("nrms_hip", 257, False), ("nrms_naml", 10, False), ("hierec", 10, False),
                                        ("graph", 10, False)])
def test_run_v0_checks_recommend_before_training(model, k, ok):
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(["--model", model, "--recommend", str(k)])
    if ok:
        run_v0.check_recommend_args(args)
    else:
        with pytest.raises(SystemExit):
            run_v0.check_recommend_args(args)
