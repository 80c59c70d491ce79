"""CPU-only checks of the score attribution (include/nrms_hip.h nrms_attribution_dot): the numpy restatement against hand-worked
cases, the symbol in the header / the ctypes table / the build list, the C ABI's argument checks (no device is touched before
they pass), CATALOGUE_EXPLAIN per model and the two refusals, run_v0's checks of --explain, and the file train_eval.recommend
writes with explain=m."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval
from tests import attribution_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = np.inf


# ---- 1: the reference against hand-worked cases ---------------------------------------------------------------------------------
def _hand():
    # H = 4 slots, d = 2, N = 3 items.  dots of item 1 = (1, 2): slot 0 -> 1, slot 1 -> 2, slot 2 -> 2, slot 3 -> -3
    ctx = np.array([[[1, 0], [0, 1], [2, 0], [-1, -1]]], dtype=F)
    w = np.array([[0.5, 0.25, 0.25, 0.5]], dtype=F)
    items = np.array([[0, 0], [1, 2], [-2, 0]], dtype=F)
    return ctx, w, items


def test_terms_total_and_order_by_hand():
    ctx, w, items = _hand()
    ids = np.array([[1, 2, -1, 3, 0]])
    r = ref.attribution(ctx, w, items, ids, 3)
    # item 1: terms (0.5, 0.5, 0.5, -1.5): three equal terms come in slot order, the negative one is listed when m reaches it
    assert r["contrib"][0, 0].tolist() == [0.5, 0.5, 0.5, -1.5] and r["total"][0, 0] == 0.0
    assert r["top_slots"][0, 0].tolist() == [0, 1, 2] and r["top_contrib"][0, 0].tolist() == [0.5, 0.5, 0.5]
    assert ref.attribution(ctx, w, items, ids, 8)["top_slots"][0, 0].tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
    # item 2 = (-2, 0): dots (-2, 0, -4, 2) -> terms (-1, 0, -1, 1)
    assert r["contrib"][0, 1].tolist() == [-1.0, 0.0, -1.0, 1.0] and r["top_slots"][0, 1].tolist() == [3, 1, 0]
    # -1 and N are invalid: total -inf, no reasons, zero terms; item 0 is a row like any other (all zero here)
    for j in (2, 3):
        assert r["total"][0, j] == -INF and r["top_slots"][0, j].tolist() == [-1] * 3
        assert r["top_contrib"][0, j].tolist() == [-INF] * 3 and not r["contrib"][0, j].any() and r["unnamed_share"][0, j] == 0
    assert r["total"][0, 4] == 0.0 and r["top_slots"][0, 4].tolist() == [0, 1, 2]
    assert not r["unnamed_share"].any()                                  # slot_named is NULL


def test_unnamed_slots_nan_and_signed_zero_by_hand():
    ctx, w, items = _hand()
    ids = np.array([[1]])
    named = np.array([[1, 0, 1, 0]], dtype=np.uint8)
    r = ref.attribution(ctx, w, items, ids, 3, named)
    assert r["top_slots"][0, 0].tolist() == [0, 2, -1] and r["top_contrib"][0, 0].tolist() == [0.5, 0.5, -INF]
    assert r["unnamed_share"][0, 0] == F(0.5) + F(-1.5) and r["total"][0, 0] == 0.0
    none = ref.attribution(ctx, w, items, ids, 2, np.zeros((1, 4), dtype=np.uint8))
    assert none["top_slots"].tolist() == [[[-1, -1]]] and none["unnamed_share"].tobytes() == none["total"].tobytes()
    # a NaN weight: that slot is no reason, the total is NaN, the other slots keep their order
    w2 = w.copy()
    w2[0, 1] = np.nan
    r = ref.attribution(ctx, w2, items, ids, 4)
    assert r["top_slots"][0, 0].tolist() == [0, 2, 3, -1] and np.isnan(r["total"][0, 0]) and np.isnan(r["contrib"][0, 0, 1])
    # -0.0 ties with +0.0 (the smaller slot first) and comes back as +0.0
    c = np.array([[[0.0, -0.0, -1.0]]], dtype=F)
    z = ref.finish(c, np.array([[0]]), 1, 3)
    assert z["top_slots"][0, 0].tolist() == [0, 1, 2] and not np.signbit(z["top_contrib"][0, 0, :2]).any()
    c = np.array([[[-0.0, 0.0, -1.0]]], dtype=F)
    z = ref.finish(c, np.array([[0]]), 1, 3)
    assert z["top_slots"][0, 0].tolist() == [0, 1, 2] and not np.signbit(z["top_contrib"][0, 0, :2]).any()
    assert np.signbit(z["contrib"][0, 0, 0])                             # contrib itself keeps the sign


def test_the_sum_is_sequential_in_slot_order():
    c = np.array([[[2.0 ** 24, 1.0, -(2.0 ** 24), 1.0]]], dtype=F)          # ((2^24 + 1) - 2^24) + 1 = 1 in fp32, 2 exactly
    assert ref.finish(c, np.array([[0]]), 1, 1)["total"][0, 0] == 1.0
    c = np.array([[[1.0, 2.0 ** 24, 1.0, -(2.0 ** 24)]]], dtype=F)          # ((1 + 2^24) + 1) - 2^24 = 0 in fp32
    assert ref.finish(c, np.array([[0]]), 1, 1)["total"][0, 0] == 0.0


@pytest.mark.parametrize("H,d,K", [(1, 1, 1), (33, 7, 65), (64, 300, 256)])
def test_lattice_cases_are_exact(H, d, K):
    ctx, w, items, ids = ref.lattice_case(3, H, d, K, 97, seed=H)
    assert ref.lattice_is_exact(ctx, w, items, ids)
    r = ref.attribution(ctx, w, items, ids, 3)
    c64 = ref.terms64(ctx, w, items, ids)
    assert np.array_equal(r["contrib"].astype(np.float64), c64)
    ok = ref.valid_ids(ids, 97)
    assert np.array_equal(r["total"][ok].astype(np.float64), c64.sum(-1)[ok])            # any order gives the same sum
    assert (ids == -1).any() and (ids == 97).any() or K == 1
    if H > 8:                                                            # runs of equal contributions do occur
        top = r["top_contrib"][ok]
        assert (top[:, 0] == top[:, 1]).any()


# ---- 2: the symbol --------------------------------------------------------------------------------------------------------------
NEW = ("nrms_attribution_dot_workspace_bytes", "nrms_attribution_dot")


def test_symbol_in_header_signatures_build_list_and_library():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, plain)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert len(_lib.SIGNATURES["nrms_attribution_dot"][1]) == 19
    from pytorch_news_recommender_amd import build
    assert "attribution.hip" in build.SOURCES
    lib = _lib.load()
    q = lib.nrms_attribution_dot_workspace_bytes
    assert q(512, 50, 300, 256, 3) > 0 and q(0, 1, 1, 1, 1) > 0 and q(1, 64, 1, 256, 8) > 0
    for bad in ((-1, 50, 300, 10, 3), (4, 0, 300, 10, 3), (4, 65, 300, 10, 3), (4, 50, 0, 10, 3), (4, 50, 300, 0, 3),
                (4, 50, 300, 257, 3), (4, 50, 300, 10, 0), (4, 50, 300, 10, 9)):
        assert q(*bad) == 0, bad
    for word in ("Term.", "Total.", "Reasons.", "Unnamed share.", "NaN.", "Invalid entries.", "Limits:", "Workspace:"):
        assert word in text[text.index("Why this item"):text.index("size_t nrms_attribution_dot_workspace_bytes")], word


C_PROG = r"""
#include "nrms_hip.h"
#include <stdio.h>
#include <string.h>

static float ctx[256], w[64], it[64], contrib[1024], total[16], tc[64], un[16];
static int64_t ids[16];
static int32_t ts[64];
static uint8_t named[64];
static uint64_t ws[64];

static int expect(int rc, const char* word) {
    const char* msg = nrms_last_error();
    if (rc != NRMS_EINVAL || !msg || strncmp(msg, "attribution_dot: ", 17) || !strstr(msg, word)) {
        printf("FAIL %s: rc=%d msg=%s\n", word, rc, msg ? msg : "(null)");
        return 1;
    }
    return 0;
}

#define CALL(B, H, N, d, K, m, c, ww, i, id, nm, co, to, s, t, u, wsp, wb) \
    nrms_attribution_dot(B, H, N, d, K, m, c, ww, i, id, nm, co, to, s, t, u, wsp, wb, NULL)

int main(void) {
    int bad = 0;
    const size_t wb = sizeof ws;
    bad += expect(CALL(-1, 4, 8, 4, 3, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "B");
    bad += expect(CALL(2, 4, -1, 4, 3, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "N");
    bad += expect(CALL(2, 4, 0x7FFF0001LL, 4, 3, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "N");
    bad += expect(CALL(2, 4, 8, 0, 3, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "d");
    bad += expect(CALL(2, 4, 8, 4, 0, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "K");
    bad += expect(CALL(2, 4, 8, 4, 257, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "K");
    bad += expect(CALL(2, 0, 8, 4, 3, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "H");
    bad += expect(CALL(2, 65, 8, 4, 3, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "H");
    bad += expect(CALL(2, 4, 8, 4, 3, 0, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "m");
    bad += expect(CALL(2, 4, 8, 4, 3, 9, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "m");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, NULL, w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "ctx");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, ctx, NULL, it, ids, named, contrib, total, ts, tc, un, ws, wb), "w is null");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, ctx, w, NULL, ids, named, contrib, total, ts, tc, un, ws, wb), "items");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, ctx, w, it, NULL, named, contrib, total, ts, tc, un, ws, wb), "ids");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, ctx, w, it, ids, named, contrib, NULL, ts, tc, un, ws, wb), "total");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, ctx, w, it, ids, named, contrib, total, NULL, tc, un, ws, wb), "top_slots");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, ctx, w, it, ids, named, contrib, total, ts, NULL, un, ws, wb), "top_contrib");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, NULL, wb), "workspace");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, (char*)ws + 4, wb - 4), "aligned");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, (float*)((char*)ctx + 2), w, it, ids, named, contrib, total, ts, tc, un, ws, wb), "ctx");
    bad += expect(CALL(2, 4, 8, 4, 3, 2, ctx, w, it, (int64_t*)((char*)ids + 4), named, contrib, total, ts, tc, un, ws, wb), "ids");
    {   /* too small a workspace is its own error code, and B = 0 is a no-op that needs no pointer */
        const int rc = CALL(2, 4, 8, 4, 3, 2, ctx, w, it, ids, named, contrib, total, ts, tc, un, ws, 8);
        const char* msg = nrms_last_error();
        if (rc != NRMS_EWORKSPACE || !msg || !strstr(msg, "workspace")) { printf("FAIL small workspace: rc=%d\n", rc); ++bad; }
        if (CALL(0, 4, 8, 4, 3, 2, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0) != NRMS_OK) { printf("FAIL B=0\n"); ++bad; }
    }
    printf("NEED %zu HAVE %zu\n", nrms_attribution_dot_workspace_bytes(2, 4, 4, 3, 2), wb);
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_c_abi_validation(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "attr_abi.c", tmp_path / "attr_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    need, have = (int(v) for v in re.search(r"NEED (\d+) HAVE (\d+)", out).groups())
    assert 0 < need <= have


# ---- 3: the models --------------------------------------------------------------------------------------------------------------
def test_catalogue_explain_per_model_and_the_two_refusals():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip, nrms_bert_hip, nrms_hip, nrms_naml_hip, nrms_v1_hip
    want = ["self", "batch", "news_ids", "catalogue", "m", "return_contributions"]
    for mod in (nrms_hip, nrms_v1_hip, nrms_naml_hip, nrms_bert_hip):
        assert mod.Model.CATALOGUE_EXPLAIN is True
        assert mod.Model.explain is nrms_hip.Model.explain
    for mod, word in ((hierec_hip, "hierec: "), (graph_hip, "graph: ")):
        assert mod.Model.CATALOGUE_EXPLAIN is False
        with pytest.raises(NotImplementedError, match=word + "explain is not available: "):
            mod.Model.explain(None, {}, None, None)
    for mod in (nrms_hip, hierec_hip, graph_hip):
        sig = inspect.signature(mod.Model.explain)
        assert list(sig.parameters) == want and sig.parameters["m"].default == 3
        assert sig.parameters["return_contributions"].kind is inspect.Parameter.KEYWORD_ONLY
    from pytorch_news_recommender_amd.bert_engine import BertEngine
    from pytorch_news_recommender_amd.engine import NRMSEngine
    from pytorch_news_recommender_amd.naml_engine import NamlEngine
    assert list(inspect.signature(NRMSEngine.user_parts).parameters) == ["self", "flat", "news_vectors", "mask", "mask_mode"]
    assert list(inspect.signature(NRMSEngine.attribution).parameters) == ["self", "ctx", "w", "items", "ids", "m", "slot_named",
                                                                          "return_contrib"]
    assert BertEngine.user_parts is not NRMSEngine.user_parts and NamlEngine.user_parts is not NRMSEngine.user_parts


# ---- 4: the CLI's checks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,ok", [
    (["--recommend", "10", "--explain", "3"], True),
    (["--recommend", "10", "--explain", "1"], True),
    (["--recommend", "256", "--explain", "8"], True),
    (["--model", "nrms_v1", "--recommend", "10", "--explain", "3"], True),
    (["--model", "nrms_bert", "--recommend", "10", "--explain", "3"], True),
    (["--recommend", "10", "--explain", "3", "--diversity", "0.5"], True),
    (["--recommend", "10", "--explain", "3", "--coarse_catalogue"], True),
    (["--negatives", "catalogue", "--recommend", "10", "--explain", "3", "--popularity_prior", "0.5"], True),
    (["--negatives", "catalogue", "--recommend", "10", "--explain", "3", "--catalogue_window", "100", "--diversity", "0.3"], True),
    (["--recommend", "10"], True),
    (["--explain", "3"], False),
    (["--recommend", "10", "--explain", "0"], False),
    (["--recommend", "10", "--explain", "9"], False),
    (["--recommend", "10", "--explain", "-1"], False),
    (["--recommend", "10", "--explain", "3", "--sections", "category"], False),
    (["--recommend_deep", "500", "--explain", "3"], False),
    (["--model", "hierec", "--recommend", "10", "--explain", "3"], False),
    (["--model", "graph", "--recommend", "10", "--explain", "3"], False),
])
def test_check_explain_args(argv, ok, monkeypatch):
    from pytorch_news_recommender_amd import data_handler, run_v0
    full = ["--dataset", "synthetic"] + ([] if "--model" in argv else ["--model", "nrms_hip"]) + argv
    args = run_v0.build_parser().parse_args(full)
    if ok:
        assert run_v0.check_explain_args(args) is None
        for check in (run_v0.check_deep_args, run_v0.check_recommend_args, run_v0.check_sections_args, run_v0.check_coarse_args,
                      run_v0.check_prior_args, run_v0.check_window_args):
            check(args)                                                  # --explain stands in no other flag's way
        return
    with pytest.raises(SystemExit) as e:
        run_v0.check_explain_args(args)
    assert "--explain" in str(e.value)
    if "hierec" in argv or "graph" in argv:
        assert "cannot split a score over the clicks" in str(e.value)

    def no_data(*a, **kw):
        raise AssertionError("data was read before the flags were checked")
    monkeypatch.setattr(run_v0, "SyntheticMind", no_data)
    monkeypatch.setattr(run_v0, "load_dataset", no_data)
    monkeypatch.setattr(data_handler, "SyntheticMind", no_data)
    with pytest.raises(SystemExit):
        run_v0.main(full)


# ---- 5: what train_eval.recommend writes ----------------------------------------------------------------------------------------
class _StubEngine:
    def check_ids(self):
        pass


class _Stub:
    """recommend returns ids 1 .. k (the last user: one slot short); explain names clicks 7 and 9, the second only for even ids."""
    CATALOGUE_EXPLAIN = True

    def __init__(self):
        self.engine, self.calls = _StubEngine(), []

    def encode_catalogue(self, titles):
        return torch.zeros(titles.shape[0], 4)

    def pack_catalogue(self, catalogue):
        return "packed"

    def recommend(self, batch, k, catalogue, exclude_history=True, **kw):
        self.calls.append(("recommend", sorted(kw)))
        B = batch["browsed_ids"].shape[0]
        ids = torch.arange(1, k + 1).expand(B, k).contiguous()
        ids[-1, -1] = -1
        out = (ids, torch.zeros(B, k))
        if kw.get("return_ild"):
            out += (torch.full((B,), 0.5),)
        if kw.get("return_certified"):
            out += (torch.ones(B, dtype=torch.uint8),)
        return out

    def explain(self, batch, news_ids, catalogue, m=3, *, return_contributions=False):
        self.calls.append(("explain", m))
        B, K = news_ids.shape
        r_ids = torch.full((B, K, m), -1, dtype=torch.int64)
        r_c = torch.full((B, K, m), -float("inf"))
        r_ids[:, :, 0], r_c[:, :, 0] = 7, 0.1
        if m > 1:
            even = news_ids % 2 == 0
            r_ids[:, :, 1] = torch.where(even, torch.full_like(news_ids, 9), torch.full_like(news_ids, -1))
            r_c[:, :, 1] = torch.where(even, torch.full((B, K), -0.25), torch.full((B, K), -float("inf")))
        total = torch.where(news_ids >= 0, news_ids.float() / 3, torch.full((B, K), -float("inf")))
        return r_ids, r_c, total, torch.full((B, K), 1.0 / 3)

    def check_recommend_ids(self):
        pass


def test_recommend_writes_the_reasons_beside_the_list(tmp_path):
    titles = torch.zeros(20, 3, dtype=torch.int64)
    batches = [{"browsed_ids": torch.tensor([[3, 4, 5], [6, 7, 0]])}, {"browsed_ids": torch.tensor([[8, 9, 1]])}]
    plain = _Stub()
    a = train_eval.recommend(None, plain, batches, titles, 3, out_file=str(tmp_path / "a.txt"))
    assert plain.last_explain_file is None and [c[0] for c in plain.calls] == ["recommend", "recommend"]
    assert plain.calls[0][1] == [] and not os.path.exists(a + ".reasons")          # the model is called exactly as before
    m = _Stub()
    b = train_eval.recommend(None, m, batches, titles, 3, out_file=str(tmp_path / "b.txt"), explain=2)
    assert open(a, "rb").read() == open(b, "rb").read()                            # the list file does not change
    assert m.last_explain_file == b + ".reasons" and [c for c in m.calls if c[0] == "explain"] == [("explain", 2)] * 2
    third = "%.9g" % np.float32(1.0 / 3)
    tot = lambda n: "%.9g" % float(torch.tensor(float(n)) / 3)
    assert open(b + ".reasons").read().splitlines() == [
        "1 1 %s %s [7:%s]" % (tot(1), third, "%.9g" % np.float32(0.1)),
        "1 2 %s %s [7:%s,9:-0.25]" % (tot(2), third, "%.9g" % np.float32(0.1)),
        "1 3 1 %s [7:%s]" % (third, "%.9g" % np.float32(0.1)),
        "2 1 %s %s [7:%s]" % (tot(1), third, "%.9g" % np.float32(0.1)),
        "2 2 %s %s [7:%s,9:-0.25]" % (tot(2), third, "%.9g" % np.float32(0.1)),
        "3 1 %s %s [7:%s]" % (tot(1), third, "%.9g" % np.float32(0.1)),
        "3 2 %s %s [7:%s,9:-0.25]" % (tot(2), third, "%.9g" % np.float32(0.1)),
    ]                                                                              # (2, 3) and (3, 3) are -1: no line
    assert np.float32("%.9g" % np.float32(0.1)) == np.float32(0.1)                 # 9 digits name the float32
    # two runs, and every path that ends in a list, give the same bytes
    c = train_eval.recommend(None, _Stub(), batches, titles, 3, out_file=str(tmp_path / "c.txt"), explain=2)
    assert open(b + ".reasons", "rb").read() == open(c + ".reasons", "rb").read()
    for name, kw in (("d", dict(diversity=0.5)), ("e", dict(coarse=True)), ("f", dict(item_bias=torch.ones(20)))):
        s = _Stub()
        out = train_eval.recommend(None, s, batches, titles, 3, out_file=str(tmp_path / (name + ".txt")), explain=2, **kw)
        assert open(out + ".reasons", "rb").read() == open(b + ".reasons", "rb").read(), name
    # refused before anything is encoded
    for bad in (0, 9):
        with pytest.raises(ValueError, match=r"\[1, 8\]"):
            train_eval.recommend(None, _Stub(), batches, titles, 3, out_file=str(tmp_path / "g.txt"), explain=bad)
    old = _Stub()
    old.CATALOGUE_EXPLAIN = False
    old.encode_catalogue = None
    with pytest.raises(ValueError, match="CATALOGUE_EXPLAIN"):
        train_eval.recommend(None, old, batches, titles, 3, out_file=str(tmp_path / "h.txt"), explain=2)
    assert list(inspect.signature(train_eval.recommend).parameters)[-1] == "explain"
    assert inspect.signature(train_eval.recommend).parameters["explain"].default is None
