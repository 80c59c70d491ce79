"""CPU-only checks of paging through the exact ranking (include/nrms_hip.h nrms_topk_dot_after / nrms_topk_dot_deep): the numpy
restatement against itself, the four symbols in the header (which still compiles as plain C), in _lib.SIGNATURES and in the library,
the refusals the library makes on the host, run_v0's --recommend_deep checks, and the two new methods on all six models."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pytorch_news_recommender_amd import _lib

from tests import topk_after_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrms_topk_dot_after_workspace_bytes", "nrms_topk_dot_after", "nrms_topk_dot_deep_workspace_bytes", "nrms_topk_dot_deep")
F = np.float32


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _lattice(seed, B=6, N=90):
    rng = np.random.default_rng(seed)
    sp = rng.integers(-3, 4, size=(B, N)).astype(F)                  # runs of equal scores everywhere
    sp[0, 3], sp[0, 4] = -0.0, 0.0
    sp[1, 5] = np.nan
    sp[2, 7], sp[2, 8] = np.inf, -np.inf
    ok = rng.random((B, N)) > 0.2
    ok[3] = False                                                    # a user with nothing eligible
    return sp, ok & ~np.isnan(sp)


# ---- 1: the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,lengths", [(0, [7] * 16), (1, [1, 2, 3, 5, 8, 13, 21, 34, 55]), (2, [256]), (3, [64, 65, 1, 192])])
def test_chained_pages_equal_the_full_sort(seed, lengths):
    sp, ok = _lattice(seed)
    want = ref.deep(sp, ok, sum(lengths))
    got = ref.chain(sp, ok, lengths)
    _same(got, want)
    for b in range(sp.shape[0]):                                     # nothing repeated, nothing skipped
        real = got[0][b][got[0][b] >= 0]
        assert len(set(real.tolist())) == len(real) == min(sum(lengths), int(ok[b].sum()))
    # the same pages, found by walking the full list
    a_s, a_i = np.zeros(sp.shape[0], dtype=F), np.full(sp.shape[0], ref.BEGIN, dtype=np.int64)
    for k in lengths:
        p = ref.after(sp, ok, a_s, a_i, k)
        _same(p, ref.after_by_position(sp, ok, a_s, a_i, k))
        a_i, a_s = p[0][:, -1].copy(), p[1][:, -1].copy()


def test_begin_end_nan_and_positions_that_are_no_items():
    sp = np.array([[5.0, 4.0, 4.0, 4.0, 2.0, 1.0]], dtype=F)
    ok = np.array([[True, True, False, True, True, True]])           # item 2 is excluded
    one = lambda s, i, k=6: ref.after(sp, ok, np.array([s], dtype=F), np.array([i], dtype=np.int64), k)[0][0].tolist()
    assert one(0.0, ref.BEGIN) == [0, 1, 3, 4, 5, -1]                # BEGIN: the score is not read
    assert one(np.nan, ref.BEGIN) == [0, 1, 3, 4, 5, -1]
    assert one(4.0, -1) == [-1] * 6 and one(4.0, -3) == [-1] * 6     # END: -1 and any other negative id
    assert one(np.nan, 1) == [-1] * 6                                # ... and a NaN score
    assert one(-np.inf, -1) == [-1] * 6                              # a finished page's last column, fed back in
    assert one(4.0, 1) == [3, 4, 5, -1, -1, -1]                      # inside a run of equal scores
    assert one(4.0, 2) == [3, 4, 5, -1, -1, -1]                      # on an excluded id: a position, not an item
    assert one(4.0, 3) == [4, 5, -1, -1, -1, -1]
    assert one(4.0, 6) == one(4.0, 10 ** 12) == one(4.0, ref.MAX_ID) == [4, 5, -1, -1, -1, -1]       # at or beyond N: after the whole run
    assert one(4.5, 0) == [1, 3, 4, 5, -1, -1]                       # a score no item has
    assert one(np.inf, 0) == [0, 1, 3, 4, 5, -1] and one(-np.inf, 0) == [-1] * 6
    assert one(1.0, 5) == [-1] * 6 and one(1.0, 4) == [5, -1, -1, -1, -1, -1]
    sc = ref.after(sp, ok, np.array([4.0], dtype=F), np.array([3], dtype=np.int64), 3)[1][0]
    assert sc.tolist() == [2.0, 1.0, -np.inf]


def test_a_tie_that_spans_a_page_boundary_and_signed_zeros():
    sp = np.zeros((1, 10), dtype=F)
    sp[0, ::2] = -0.0                                                # -0.0 and +0.0 alternate: one run of ten equal scores
    sp[0, 9] = 1.0
    ok = np.ones((1, 10), dtype=bool)
    ids, sc = ref.chain(sp, ok, [4, 4, 4])
    assert ids[0].tolist() == [9, 0, 1, 2, 3, 4, 5, 6, 7, 8, -1, -1]
    assert not np.signbit(sc[0][:10]).any()                          # returned as +0.0
    a = ref.after(sp, ok, np.array([-0.0], dtype=F), np.array([2], dtype=np.int64), 3)
    b = ref.after(sp, ok, np.array([0.0], dtype=F), np.array([2], dtype=np.int64), 3)
    _same(a, b)
    assert a[0][0].tolist() == [3, 4, 5]


def test_deep_prefixes_and_limits():
    sp, ok = _lattice(5, B=4, N=700)
    full = ref.deep(sp, ok, 4096)
    for K in (1, 256, 257, 600):
        got = ref.deep(sp, ok, K)
        assert got[0].tobytes() == full[0][:, :K].tobytes() and got[1].tobytes() == full[1][:, :K].tobytes()
    assert (full[0][:, 700:] == -1).all() and np.isneginf(full[1][:, 700:]).all()
    with pytest.raises(AssertionError):
        ref.deep(sp, ok, 4097)


# ---- 2: the symbols ----------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_signatures_and_library():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, name + " is not declared in include/nrms_hip.h"
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(2).count(",") + 1, name
    # a page takes the cursor's two arrays beside the windowed call's arguments, the deep call none; the queries are the plain one
    assert len(_lib.SIGNATURES["nrms_topk_dot_after"][1]) == len(_lib.SIGNATURES["nrms_topk_dot_windowed"][1]) + 2
    assert len(_lib.SIGNATURES["nrms_topk_dot_deep"][1]) == len(_lib.SIGNATURES["nrms_topk_dot_windowed"][1])
    for q in (NEW[0], NEW[2]):
        assert _lib.SIGNATURES[q] == _lib.SIGNATURES["nrms_topk_dot_workspace_bytes"]
    lib = _lib.load()                                                # binds every symbol: a missing export raises here
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for word in ("NRMS_CURSOR_BEGIN", "(a)", "(b)", "(c)", "(d)", "(e)", "(f)", "topk_dot_after: ...", "topk_dot_deep: ...",
                 "0x7FFF0000, which follows every item at the same score", "TK_CURSOR_EXIT"):
        assert word in text, word
    from pytorch_news_recommender_amd.model import nrms_hip
    assert re.search(r"#define\s+NRMS_CURSOR_BEGIN\s+\(-2\)", text) and nrms_hip.PAGE_BEGIN == ref.BEGIN == -2


def test_header_is_plain_c_and_exports_the_calls(tmp_path):
    src = tmp_path / "after.c"
    src.write_text("""
#include <stdio.h>
#include "nrms_hip.h"
int main(void) {
    int bad = 0;
    float x[16] = {0};
    bad += nrms_topk_dot_after(0, 5, 3, 7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != NRMS_OK;            /* B = 0: a no-op */
    bad += nrms_topk_dot_deep(0, 5, 3, 4096, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != NRMS_OK;
    bad += nrms_topk_dot_after(1, 5, 3, 257, x, x, 0, 0, 0, x, (const int64_t*)x, 0, 0, x, (int64_t*)x, x, 64, 0) != NRMS_EINVAL;
    bad += nrms_topk_dot_deep(1, 5, 3, 4097, x, x, 0, 0, 0, 0, 0, x, (int64_t*)x, x, 64, 0) != NRMS_EINVAL;
    bad += NRMS_CURSOR_BEGIN != -2;
    printf("BAD %d\\n", bad);
    printf("WS %zu %zu %zu %zu %zu %zu\\n", nrms_topk_dot_after_workspace_bytes(4, 100, 8, 257), nrms_topk_dot_deep_workspace_bytes(4, 100, 8, 0),
           nrms_topk_dot_deep_workspace_bytes(4, 100, 8, 4097), nrms_topk_dot_after_workspace_bytes(4, 100, 8, 256),
           nrms_topk_dot_deep_workspace_bytes(4, 100, 8, 4096), nrms_topk_dot_workspace_bytes(4, 100, 8, 256));
    return 0;
}
""")
    exe = tmp_path / "after"
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    _lib.load()
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    ws = [int(v) for v in out.split("WS ")[1].split("\n")[0].split()]
    assert ws[:3] == [0, 0, 0] and ws[3] == ws[4] == ws[5] > 0


def test_queries_and_host_side_refusals():
    """The queries equal the plain one (the deep call's: its longest page's); bad arguments are refused on the host, before any launch."""
    lib = _lib.load()
    for B, N, d in ((70, 5000, 40), (512, 130000, 300), (1, 0, 1), (0, 5, 3)):
        for k in (1, 10, 256):
            assert lib.nrms_topk_dot_after_workspace_bytes(B, C.c_int64(N), d, k) == lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k) > 0
        for K in (1, 100, 256, 257, 1000, 4096):
            assert lib.nrms_topk_dot_deep_workspace_bytes(B, C.c_int64(N), d, K) == lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, min(K, 256)) > 0
    for k in (0, 257):
        assert lib.nrms_topk_dot_after_workspace_bytes(70, C.c_int64(5000), 40, k) == 0
    for K in (0, 4097, -1):
        assert lib.nrms_topk_dot_deep_workspace_bytes(70, C.c_int64(5000), 40, K) == 0
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    odd2, odd4 = C.c_void_p(p.value + 2), C.c_void_p(p.value + 4)

    def after(k=2, bias=None, time=None, win=None, a_s=p, a_i=p, ws=4096, n_ex=0, B=2):
        return lib.nrms_topk_dot_after(B, C.c_int64(4), 2, k, p, p, bias, time, win, a_s, a_i, None, n_ex, p, p, p, C.c_size_t(ws), None)

    def deep(K=300, bias=None, time=None, win=None, ws=4096, n_ex=0, scores=p, ids=p):
        return lib.nrms_topk_dot_deep(2, C.c_int64(4), 2, K, p, p, bias, time, win, None, n_ex, scores, ids, p, C.c_size_t(ws), None)

    for kw, word in ((dict(k=0), b"k must be in [1, 256]"), (dict(k=257), b"k must be in [1, 256]"), (dict(a_s=None), b"after_scores is null"),
                     (dict(a_i=None), b"after_ids is null"), (dict(a_s=odd2), b"after_scores must be 4-byte aligned"),
                     (dict(a_i=odd4), b"after_ids must be 8-byte aligned"), (dict(time=p), b"window is null"),
                     (dict(win=p), b"item_time is null"), (dict(time=odd2, win=p), b"item_time must be 4-byte aligned"),
                     (dict(time=p, win=odd2), b"window must be 4-byte aligned"), (dict(bias=odd2), b"bias must be 4-byte aligned"),
                     (dict(n_ex=-1), b"n_exclude"), (dict(B=-1), b"B must be")):
        assert after(**kw) == _lib.NRMS_EINVAL, kw
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_after: ") and word in msg, msg
    for kw, word in ((dict(K=0), b"K must be in [1, 4096]"), (dict(K=4097), b"K must be in [1, 4096]"), (dict(time=p), b"window is null"),
                     (dict(win=p), b"item_time is null"), (dict(time=p, win=odd2), b"window must be 4-byte aligned"),
                     (dict(bias=odd2), b"bias must be 4-byte aligned"), (dict(scores=None), b"top_scores is null"),
                     (dict(ids=odd4), b"top_ids must be 8-byte aligned"), (dict(n_ex=-1), b"n_exclude")):
        assert deep(**kw) == _lib.NRMS_EINVAL, kw
        msg = lib.nrms_last_error()
        assert msg.startswith(b"topk_dot_deep: ") and word in msg, msg
    assert after(ws=8) == _lib.NRMS_EWORKSPACE and deep(ws=8) == _lib.NRMS_EWORKSPACE
    assert lib.nrms_last_error().startswith(b"topk_dot_deep: workspace")
    assert lib.nrms_topk_dot_after(0, C.c_int64(4), 2, 2, *([None] * 8), 0, None, None, None, C.c_size_t(0), None) == _lib.NRMS_OK
    assert lib.nrms_topk_dot_deep(0, C.c_int64(4), 2, 4096, *([None] * 6), 0, None, None, None, C.c_size_t(0), None) == _lib.NRMS_OK


# ---- 3: the CLI's checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,ok", [
    (["--recommend_deep", "1"], True),
    (["--recommend_deep", "1000"], True),
    (["--recommend_deep", "4096"], True),
    (["--model", "nrms_v1", "--recommend_deep", "500"], True),
    (["--model", "nrms_bert", "--recommend_deep", "500"], True),
    (["--negatives", "catalogue", "--recommend_deep", "500", "--popularity_prior", "0.5"], True),
    (["--negatives", "catalogue", "--recommend_deep", "500", "--catalogue_window", "100"], True),
    (["--negatives", "adaptive", "--recommend_deep", "500", "--popularity_prior", "0.5", "--catalogue_window", "100"], True),
    (["--recommend_deep", "500", "--retrieval_metrics", "1000"], True),
    (["--recommend", "257"], True),                                      # not this check's: check_recommend_args refuses it (below)
    (["--recommend_deep", "0"], False),
    (["--recommend_deep", "4097"], False),
    (["--recommend_deep", "-5"], False),
    (["--recommend_deep", "500", "--recommend", "10"], False),
    (["--recommend_deep", "500", "--diversity", "0.5"], False),
    (["--recommend_deep", "500", "--shortlist", "100"], False),
    (["--recommend_deep", "500", "--coarse_catalogue"], False),
    (["--recommend_deep", "500", "--coarse_shortlist", "100"], False),
    (["--recommend_deep", "500", "--sections", "category"], False),
    (["--model", "hierec", "--recommend_deep", "500"], False),
    (["--model", "graph", "--recommend_deep", "500"], False),
    (["--model", "nrms_naml", "--recommend_deep", "500"], False),        # as --recommend: run_v0 builds no feature-row catalogue
])
def test_check_deep_args(argv, ok, monkeypatch):
    from pytorch_news_recommender_amd import data_handler, run_v0
    args = run_v0.build_parser().parse_args(["--dataset", "synthetic"] + ([] if "--model" in argv else ["--model", "nrms_hip"]) + argv)
    if ok:
        assert run_v0.check_deep_args(args) is None
        run_v0.check_prior_args(args)                                # the prior and the window count it as a list to apply to
        run_v0.check_window_args(args)
    else:
        with pytest.raises(SystemExit) as e:
            run_v0.check_deep_args(args)
        assert "--recommend_deep" in str(e.value)
        # ... and main() says so before any data is read

        def no_data(*a, **kw):
            raise AssertionError("data was read before the flags were checked")
        monkeypatch.setattr(run_v0, "SyntheticMind", no_data)
        monkeypatch.setattr(run_v0, "load_dataset", no_data)
        monkeypatch.setattr(data_handler, "SyntheticMind", no_data)
        with pytest.raises(SystemExit) as e:
            run_v0.main(["--dataset", "synthetic"] + ([] if "--model" in argv else ["--model", "nrms_hip"]) + argv)
        assert "--recommend_deep" in str(e.value)


def test_recommend_keeps_its_own_limit():
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(["--dataset", "synthetic", "--model", "nrms_hip", "--recommend", "257"])
    with pytest.raises(SystemExit, match=r"\[1, 256\]"):
        run_v0.check_recommend_args(args)
    sig = inspect.signature(__import__("pytorch_news_recommender_amd.train_eval", fromlist=["x"]).recommend_deep)
    assert list(sig.parameters) == ["config", "model", "data_iter", "titles", "K", "out_file", "exclude_history", "news_info", "item_bias",
                                    "item_time", "request_time", "window_span"]


# ---- 4: the models -------------------------------------------------------------------------------------------------------------
def test_all_six_models_have_the_two_methods_with_one_signature_each():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip, nrms_bert_hip, nrms_hip, nrms_naml_hip, nrms_v1_hip
    page = ["self", "batch", "k", "catalogue", "after", "exclude_history", "item_bias", "item_time", "window"]
    deep = ["self", "batch", "K", "catalogue", "exclude_history", "item_bias", "item_time", "window"]
    for mod in (nrms_hip, nrms_v1_hip, nrms_naml_hip, nrms_bert_hip, hierec_hip, graph_hip):
        for name, want, n_pos in (("recommend_page", page, 6), ("recommend_deep", deep, 5)):
            sig = inspect.signature(getattr(mod.Model, name))
            assert list(sig.parameters) == want, (mod.__name__, name)
            kinds = [p.kind for p in sig.parameters.values()]
            assert all(k == inspect.Parameter.POSITIONAL_OR_KEYWORD for k in kinds[:n_pos]), (mod.__name__, name)
            assert all(k == inspect.Parameter.KEYWORD_ONLY for k in kinds[n_pos:]), (mod.__name__, name)
            assert all(sig.parameters[p].default is None for p in ("item_bias", "item_time", "window")) and sig.parameters["exclude_history"].default is True
        assert inspect.signature(mod.Model.recommend_page).parameters["after"].default is None
    # the engine's two calls, and top_k as it was
    from pytorch_news_recommender_amd.engine import NRMSEngine
    assert list(inspect.signature(NRMSEngine.top_k_after).parameters) == ["self", "user_vec", "items", "k", "after_scores", "after_ids", "exclude",
                                                                          "bias", "item_time", "window"]
    assert list(inspect.signature(NRMSEngine.top_k_deep).parameters) == ["self", "user_vec", "items", "K", "exclude", "bias", "item_time", "window"]
    assert list(inspect.signature(NRMSEngine.top_k).parameters) == ["self", "user_vec", "items", "k", "exclude", "bias", "item_time", "window"]


def test_models_that_cannot_page_refuse_without_touching_a_device():
    from pytorch_news_recommender_amd.model import graph_hip, hierec_hip, nrms_naml_hip
    for mod, word in ((hierec_hip, "hierec: "), (graph_hip, "graph: ")):
        with pytest.raises(NotImplementedError, match=word + "recommend_page is not available"):
            mod.Model.recommend_page(None, {}, 5, None)
        with pytest.raises(NotImplementedError, match=word + "recommend_deep is not available"):
            mod.Model.recommend_deep(None, {}, 500, None)
        assert mod.Model.CATALOGUE_PAGING is False
    with pytest.raises(NotImplementedError, match="cursor"):
        hierec_hip.Model.recommend_page(None, {}, 5, None, after=None, item_bias=None)
    # nrms_naml pages, over the catalogue type its recommend takes
    for call in (lambda: nrms_naml_hip.Model.recommend_page(None, {}, 5, None), lambda: nrms_naml_hip.Model.recommend_deep(None, {}, 500, None)):
        with pytest.raises(NotImplementedError, match="encode_catalogue\\(titles, absts, categ, subcateg\\)"):
            call()
