"""CPU-only checks of grouped catalogue retrieval: the C-ABI validation and workspace queries of nrms_topk_grouped_dot and
nrms_hier_query (include/nrms_hip.h), their ctypes bindings, DeviceFeed.news_info() and the refusals of HieRec / nrms_naml
without category tables."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PROG = r"""
#include "nrms_hip.h"
#include <stdio.h>
#include <string.h>

static float q[8], it[8], sc[8], u[8];
static int32_t iid[8], l[8];
static int64_t gp[4], ids[8], gt[4];
static uint64_t ws[4096];

static int expect(int rc, const char* word) {
    const char* msg = nrms_last_error();
    if (rc == 0 || !msg || !strstr(msg, word)) { printf("FAIL %s: rc=%d msg=%s\n", word, rc, msg ? msg : "(null)"); return 1; }
    return 0;
}

int main(void) {
    int bad = 0;
    const size_t wb = sizeof ws;
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 0, 1, q, it, iid, gp, NULL, 0, sc, ids, ws, wb, NULL), "k");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 257, 1, q, it, iid, gp, NULL, 0, sc, ids, ws, wb, NULL), "k");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 3, 0, q, it, iid, gp, NULL, 0, sc, ids, ws, wb, NULL), "G");
    bad += expect(nrms_topk_grouped_dot(-1, 4, 2, 3, 1, q, it, iid, gp, NULL, 0, sc, ids, ws, wb, NULL), "B");
    bad += expect(nrms_topk_grouped_dot(2, -4, 2, 3, 1, q, it, iid, gp, NULL, 0, sc, ids, ws, wb, NULL), "N");
    bad += expect(nrms_topk_grouped_dot(2, 4, 0, 3, 1, q, it, iid, gp, NULL, 0, sc, ids, ws, wb, NULL), "d");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 3, 1, q, it, iid, gp, NULL, -1, sc, ids, ws, wb, NULL), "n_exclude");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 3, 1, NULL, it, iid, gp, NULL, 0, sc, ids, ws, wb, NULL), "query");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 3, 1, q, NULL, iid, gp, NULL, 0, sc, ids, ws, wb, NULL), "items");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 3, 1, q, it, NULL, gp, NULL, 0, sc, ids, ws, wb, NULL), "item_ids");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 3, 1, q, it, iid, NULL, NULL, 0, sc, ids, ws, wb, NULL), "group_ptr");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 3, 1, q, it, iid, gp, NULL, 0, NULL, ids, ws, wb, NULL), "top_scores");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 3, 1, q, it, iid, gp, NULL, 0, sc, NULL, ws, wb, NULL), "top_ids");
    bad += expect(nrms_topk_grouped_dot(2, 4, 2, 3, 1, q, it, iid, gp, NULL, 0, sc, ids, ws, 8, NULL), "workspace");
    bad += expect(nrms_hier_query(2, 0, 1, 4, gt, gt, l, l, l, l, l, u, u, u, 0.7f, 0.15f, q, NULL), "H");
    bad += expect(nrms_hier_query(2, 65, 1, 4, gt, gt, l, l, l, l, l, u, u, u, 0.7f, 0.15f, q, NULL), "H");
    bad += expect(nrms_hier_query(2, 3, 0, 4, gt, gt, l, l, l, l, l, u, u, u, 0.7f, 0.15f, q, NULL), "G");
    bad += expect(nrms_hier_query(-1, 3, 1, 4, gt, gt, l, l, l, l, l, u, u, u, 0.7f, 0.15f, q, NULL), "B");
    bad += expect(nrms_hier_query(2, 3, 1, 0, gt, gt, l, l, l, l, l, u, u, u, 0.7f, 0.15f, q, NULL), "d");
    bad += expect(nrms_hier_query(2, 3, 1, 4, gt, gt, l, l, l, l, l, u, u, u, 0.7f, 0.15f, NULL, NULL), "null");
    printf("WS %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n",
           nrms_topk_grouped_dot_workspace_bytes(512, 130000, 300, 0, 294),
           nrms_topk_grouped_dot_workspace_bytes(512, 130000, 300, 257, 294),
           nrms_topk_grouped_dot_workspace_bytes(512, 130000, 300, 10, 0),
           nrms_topk_grouped_dot_workspace_bytes(512, 130000, 0, 10, 294),
           nrms_topk_grouped_dot_workspace_bytes(-1, 130000, 300, 10, 294),
           nrms_topk_grouped_dot_workspace_bytes(512, -1, 300, 10, 294),
           nrms_topk_grouped_dot_workspace_bytes(512, 130000, 300, 10, 294),
           nrms_topk_grouped_dot_workspace_bytes(512, 130000, 300, 100, 294),
           nrms_topk_grouped_dot_workspace_bytes(1, 130000, 300, 100, 294),
           nrms_topk_grouped_dot_workspace_bytes(100000, 130000, 300, 100, 294),
           nrms_topk_grouped_dot_workspace_bytes(512, 0, 300, 100, 294),
           nrms_topk_grouped_dot_workspace_bytes(512, 130000, 300, 100, 1));
    /* B = 0 is a no-op, even with null buffers */
    bad += nrms_topk_grouped_dot(0, 4, 2, 3, 1, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL) != 0;
    bad += nrms_hier_query(0, 3, 2, 4, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0.7f, 0.15f, NULL, NULL) != 0;
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_grouped_c_abi_validation_and_workspace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "grouped_abi.c", tmp_path / "grouped_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    ws = [int(v) for v in out.split("WS ")[1].split("\n")[0].split()]
    assert ws[:6] == [0] * 6                                       # k = 0, k = 257, G = 0, d = 0, B < 0, N < 0 rejected
    assert all(v > 0 for v in ws[6:])
    assert ws[7] > ws[6]                                           # grows with k
    assert ws[9] > ws[8]                                           # ... with B
    assert ws[7] > ws[10]                                          # ... with N
    assert ws[7] >= ws[11]                                         # ... with G (the tile table)
    assert ws[7] < 512 * 130000 * 4 // 4                           # far from a [B, N] score matrix


def test_grouped_signatures_are_bound():
    lib = _lib.load()
    assert lib.nrms_topk_grouped_dot_workspace_bytes(4, 100, 8, 10, 3) > 0
    assert lib.nrms_topk_grouped_dot_workspace_bytes(4, 100, 8, 10, 0) == 0
    assert lib.nrms_topk_grouped_dot_workspace_bytes(4, 100, 8, 0, 3) == 0
    for name in ("nrms_topk_grouped_dot", "nrms_hier_query"):
        assert getattr(lib, name).restype is not None and len(getattr(lib, name).argtypes) in (16, 18)
    assert lib.nrms_hier_query(0, 3, 2, 4, *([None] * 10), 0.7, 0.15, None, None) == 0


def _feed_and_corpus(**cfg_over):
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    cfg = Config("nrms_v0")
    cfg.__nrms__()
    cfg.n_words, cfg.n_words_title, cfg.history_len, cfg.sample_size, cfg.max_candidate_size = 600, 12, 10, 4, 24
    corpus = SyntheticMind(cfg, n_news=500, n_topics=6, seed=3)
    samples, _ = corpus.eval_samples(40, max_shown=20)
    return cfg, corpus, samples, DeviceFeed


def test_news_info_matches_the_corpus():
    cfg, corpus, samples, DeviceFeed = _feed_and_corpus()
    feed = DeviceFeed(cfg, samples, type=1, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict,
                      batch_size=16, device="cpu")
    n_before = {k: v.clone() for k, v in feed.packed.items()}
    info = feed.news_info()
    assert info is feed.news_info()                                # built once
    assert set(info) == {"absts", "categ", "subcateg"} and info["absts"] is feed.absts
    N = feed.titles.shape[0]
    seen = np.zeros(N, bool)
    for s in samples:
        seen[s[0]] = True
        seen[s[3]] = True
    assert not seen[0] and 0 < seen.sum() < N - 1                  # some ids never appear
    ids = np.nonzero(seen)[0]
    for name, truth in (("categ", corpus.category), ("subcateg", corpus.subcategory)):
        t = info[name]
        assert t.dtype == torch.int64 and t.shape == (N,)
        t = t.numpy()
        np.testing.assert_array_equal(t[ids], truth[ids - 1])
        assert (t[~seen] == 0).all()
    assert all(torch.equal(n_before[k], v) for k, v in feed.packed.items())


def test_news_info_unknown_and_conflicting_categories():
    cfg, corpus, samples, DeviceFeed = _feed_and_corpus()
    s0 = [list(x) for x in samples[0]]
    nid = s0[0][0]
    other = [list(x) for x in samples[1]]
    other[0] = [nid] + other[0][1:]
    other[1] = [0] + other[1][1:]                                  # 0 = unknown: no conflict
    other[2] = [0] + other[2][1:]
    feed = DeviceFeed(cfg, [s0, other], type=1, id2title_dict=corpus.id2title_dict, batch_size=2, device="cpu")
    assert int(feed.news_info()["categ"][nid]) == corpus.category[nid - 1]
    clash = [list(x) for x in other]
    clash[1] = [int(corpus.category[nid - 1]) + 1] + clash[1][1:]
    feed = DeviceFeed(cfg, [s0, clash], type=1, id2title_dict=corpus.id2title_dict, batch_size=2, device="cpu")
    with pytest.raises(ValueError, match="news id %d " % nid):
        feed.news_info()


def _hierec(tmp_path):
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.model.hierec_hip import Model
    cfg = Config("hierec")
    cfg.__nrms__()
    cfg.word_embed_size, cfg.num_attention_heads, cfg.query_vector_dim = 60, 6, 32
    cfg.category_nums, cfg.subcategory_nums = 8, 30
    table = np.random.default_rng(0).normal(0, 0.4, size=(50, 60)).astype(np.float32)
    return Model(cfg, pretrained_word_embedding=table)


def test_hierec_catalogue_needs_categories(tmp_path):
    m = _hierec(tmp_path)
    with pytest.raises(NotImplementedError, match="category"):
        m.encode_catalogue(np.zeros((4, 3), np.int64))
    with pytest.raises(NotImplementedError, match="category"):
        m.encode_catalogue(np.zeros((4, 3), np.int64), categ=np.zeros(4, np.int64))
    with pytest.raises(NotImplementedError, match="category"):
        m.recommend({"browsed_ids": np.zeros((2, 3), np.int64)}, 5, None)


def test_nrms_naml_catalogue_needs_categories(tmp_path):
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
        m.encode_catalogue(np.zeros((4, 3), np.int64), absts=np.zeros((4, 5), np.int64), subcateg=np.zeros(4, np.int64))
