"""Host side of the global click graph (click_graph.py, csrc/graphsample.hip, run_v0 --graph): what can be checked without a GPU."""
import os
import re

import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.click_graph import ClickGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("nrms_graph_sample_workspace_bytes", "nrms_graph_sample_neighbors", "nrms_graph_resolve_workspace_bytes", "nrms_graph_resolve_rows")


def test_header_declares_the_sampler_entry_points():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert "typedef struct nrms_click_graph" in text
    common = open(os.path.join(ROOT, "pytorch_news_recommender_amd", "csrc", "common.h")).read()
    assert re.search(r"PHILOX_SITE_GRAPH_SAMPLE\s*=\s*5u", common)
    assert "graphsample.hip" in open(os.path.join(ROOT, "pytorch_news_recommender_amd", "build.py")).read()


def test_run_v0_parser_accepts_graph_and_refuses_unknown_values_before_any_data_is_read(tmp_path, monkeypatch):
    from pytorch_news_recommender_amd import run_v0
    p = run_v0.build_parser()
    assert p.parse_args(["--model", "graph"]).graph == "induced"
    assert p.parse_args(["--model", "graph", "--graph", "global"]).graph == "global"
    monkeypatch.chdir(tmp_path)
    data = tmp_path / "data_processed"
    for argv in (["--model", "graph", "--graph", "whole"],                                   # unknown value
                 ["--model", "nrms_hip", "--graph", "global"],                               # a model without a graph
                 ["--model", "graph", "--graph", "global", "--feed", "loader"],              # the graph lives in the device feed
                 ["--model", "graph", "--graph", "global", "--recommend", "5"]):             # --recommend stays refused
        with pytest.raises(SystemExit):
            run_v0.main(argv + ["--dataset", "synthetic", "--data_path", str(data)])
        assert not data.exists(), argv                                                       # nothing was read or written


def test_click_graph_argument_checks_raise_without_a_gpu():
    ok = torch.tensor([[1, 2, 0], [2, 0, 0]], dtype=torch.int64)
    with pytest.raises(_lib.NrmsError, match="int32 or int64"):
        ClickGraph.from_histories(ok.to(torch.float32), 5)
    with pytest.raises(_lib.NrmsError, match=r"\[U, H\]"):
        ClickGraph.from_histories(ok.reshape(-1), 5)
    with pytest.raises(_lib.NrmsError, match="n_news"):
        ClickGraph.from_histories(ok, 2 ** 31)
    with pytest.raises(_lib.NrmsError, match="n_news"):
        ClickGraph.from_histories(ok, 0)
    with pytest.raises(_lib.NrmsError, match="degree above"):
        ClickGraph.from_histories(torch.empty(2 ** 31, 0, dtype=torch.int64), 5)             # (no storage behind an empty tensor)
    i64, i32 = (lambda *v: torch.tensor(v, dtype=torch.int64)), (lambda *v: torch.tensor(v, dtype=torch.int32))
    with pytest.raises(_lib.NrmsError, match="user_ptr"):
        ClickGraph(i32(0, 1), i32(1), i64(0, 0, 1), i32(0))
    with pytest.raises(_lib.NrmsError, match="index list"):
        ClickGraph(i64(0, 1), i64(1), i64(0, 0, 1), i32(0))
    with pytest.raises(_lib.NrmsError, match="edges"):
        ClickGraph(i64(0, 1), i32(1), i64(0, 0, 1), i32(0, 0))
    g = ClickGraph.from_histories(ok, 5)                                                     # the build itself is torch: runs anywhere
    with pytest.raises(_lib.NrmsError, match="no CPU path"):
        g.sample_neighbors(torch.tensor([1, 2], dtype=torch.int64), 4, seed=0)
    with pytest.raises(_lib.NrmsError, match=r"\[1, 64\]"):
        g.sample_neighbors(torch.tensor([1, 2], dtype=torch.int64), 65, seed=0)
    with pytest.raises(_lib.NrmsError, match="int64"):
        g.sample_neighbors(torch.tensor([1, 2], dtype=torch.int32), 4, seed=0)


def test_click_graph_build_on_the_host_matches_a_grouping_by_hand():
    hist = torch.tensor([[3, 1, 3, 0], [0, 0, 0, 0], [1, 9, -2, 4], [4, 4, 4, 4]], dtype=torch.int64)
    g = ClickGraph.from_histories(hist, 6)
    assert (g.n_users, g.n_news, g.n_edges) == (4, 6, 5)
    assert g.n_padding == 5 and g.n_out_of_range == 2
    assert g.user_ptr.tolist() == [0, 2, 2, 4, 5] and g.user_news.tolist() == [1, 3, 1, 4, 4]
    assert g.news_ptr.tolist() == [0, 0, 2, 2, 3, 5, 5] and g.news_users.tolist() == [0, 2, 0, 2, 3]
    assert g.user_ptr.dtype == torch.int64 and g.user_news.dtype == torch.int32
    assert g.nbytes() == 8 * (5 + 7) + 4 * 10
