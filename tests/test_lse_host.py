"""CPU-only checks of the catalogue log-partition (include/nrms_hip.h nrms_logsumexp_dot): the numpy restatement
(tests/lse_ref.py) against closed forms and on the NaN / inf table, its float32 arithmetic held to a quarter of the GPU test's
tolerance on every GPU case's data, the symbols in the header and in _lib.SIGNATURES, the C ABI's argument validation and
workspace query from a C99 program, run_v0's --retrieval_nll checks, CATALOGUE_LIKELIHOOD on all six models with the HieRec
and graph refusals, and evaluate_retrieval(nll_temperatures=...) on a stub model."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval

from tests import lse_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrms_logsumexp_dot_workspace_bytes", "nrms_logsumexp_dot", "nrms_logsumexp_dot_mass")
F = np.float32


# ---- 1: the restatement against closed forms ------------------------------------------------------------------------------------
def _random(B=3, N=200, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, N)).astype(F) * F(3), rng.standard_normal(N).astype(F)


def test_inv_temperature_zero_is_log_of_the_count():
    s, bias = _random()
    s[0, 5] = np.nan
    ex = np.array([[1, 2, 2, -1, 200], [0, 0, 0, 0, 0], [7, 8, 9, 10, 11]])
    r = ref.reference(s, [0.0], exclude=ex)
    np.testing.assert_array_equal(r["n_eligible"][:, 0], [197, 199, 195])
    np.testing.assert_array_equal(r["mass"][:, 0, 0], r["n_eligible"][:, 0].astype(np.uint64) * np.uint64(ref.MASS_ONE))
    assert (r["mass"][:, 0, 1] == 0).all() and (r["zmax"] == 0).all() and not np.signbit(r["zmax"]).any()
    np.testing.assert_allclose(r["lse64"][:, 0], np.log([197, 199, 195]), rtol=1e-15)
    np.testing.assert_array_equal(r["lse32"][:, 0], np.log([197.0, 199.0, 195.0]).astype(F))


def test_a_constant_bias_shifts_lse_by_it():
    s, _ = _random(seed=1)
    inv_t = [1.0, 0.5, 2.0]
    base = ref.reference(s, inv_t)
    for c, scale in ((0.75, 1.0), (-2.0, 0.5)):
        r = ref.reference(s, inv_t, bias=np.full(s.shape[1], c, F), bias_scale=[scale] * 3)
        np.testing.assert_allclose(r["lse64"], base["lse64"] + c * scale, atol=5e-6)          # (the logits are rounded to fp32)
        np.testing.assert_array_equal(r["n_eligible"], base["n_eligible"])


def test_permuting_the_catalogue_changes_no_bit():
    s, bias = _random(seed=2)
    s[1, 3] = np.nan
    ex = np.array([[4, 9], [5, 5], [0, 199]])
    inv_t, scale = [1.0, 6.5, 0.05], [1.0, 0.0, -1.0]
    a = ref.reference(s, inv_t, bias, scale, ex)
    p = np.random.default_rng(3).permutation(s.shape[1])
    inv = np.argsort(p)
    b = ref.reference(s[:, p], inv_t, bias[p], scale, inv[ex])
    for k in ("zmax", "n_eligible", "lse32", "mass"):
        assert a[k].tobytes() == b[k].tobytes(), k
    doubled = ref.reference(np.concatenate([s, s], axis=1), inv_t, np.concatenate([bias, bias]), scale,
                            np.concatenate([ex, ex + s.shape[1]], axis=1))
    np.testing.assert_array_equal(doubled["mass"], 2 * a["mass"])
    np.testing.assert_array_equal(doubled["n_eligible"], 2 * a["n_eligible"])


def test_fixed_point_is_exact_down_to_2_pow_minus_40_and_truncates_below():
    t = np.array([1.0, 0.5, 2.0 ** -31, 2.0 ** -40 * (1 + 2.0 ** -23), 2.0 ** -63, 2.0 ** -64, 0.0, 1 - 2.0 ** -24], dtype=F)
    hi, lo = ref.fixed(t)
    back = [int(h) * 2 ** 32 + int(l) for h, l in zip(hi, lo)]                  # units of 2^-63
    assert back[:5] == [2 ** 63, 2 ** 62, 2 ** 32, (2 ** 23 + 1), 1] and back[5:7] == [0, 0]
    assert back[7] == (2 ** 24 - 1) * 2 ** 39 and int(hi[0]) == ref.MASS_ONE and int(lo[0]) == 0


# ---- 2: the NaN / inf table -------------------------------------------------------------------------------------------------------
def test_nan_and_inf_rules():
    inf, nan = np.inf, np.nan
    s = np.array([[1.0, nan, 2.0, -inf, 0.5, 3.0],
                  [nan, nan, nan, nan, nan, nan],
                  [-inf, -inf, -inf, -inf, -inf, -inf],
                  [1.0, inf, 2.0, 0.0, 0.0, 0.0],
                  [-0.0, -1.0, -2.0, -3.0, -4.0, -5.0]], dtype=F)
    r = ref.reference(s, [1.0, 0.0])
    # row 0: the NaN score is out, the -inf stays and adds 0; at inv_temperature 0 the -inf score is 0 * inf = NaN and is out too
    np.testing.assert_array_equal(r["n_eligible"], [[5, 4], [0, 0], [6, 0], [6, 5], [6, 6]])
    np.testing.assert_allclose(r["lse64"][0, 0], np.log(np.exp([1.0, 2.0, 0.5, 3.0]).sum()), rtol=1e-15)
    assert r["lse64"][0, 1] == np.log(4.0)
    assert np.isneginf(r["lse32"][1]).all() and np.isneginf(r["zmax"][1]).all()                  # nothing eligible
    assert np.isneginf(r["lse32"][2]).all() and np.isneginf(r["zmax"][2]).all()                  # only -inf logits / none
    assert r["lse32"][3, 0] == inf and r["zmax"][3, 0] == inf and r["lse64"][3, 1] == np.log(5.0)
    assert r["zmax"][4, 0] == 0 and not np.signbit(r["zmax"][4, 0])                              # -0.0 comes back as +0.0
    # the prior: NaN removes the item for every user and variant; scale 0 times an infinite prior is NaN; -inf stays and adds 0
    bias = np.array([0.0, 0.0, nan, 0.0, -inf, inf], dtype=F)
    r = ref.reference(s[[0, 4]], [1.0, 1.0], bias=bias, bias_scale=[1.0, 0.0])
    np.testing.assert_array_equal(r["n_eligible"], [[4, 2], [5, 3]])
    assert r["lse32"][0, 0] == inf and r["lse32"][1, 0] == inf                                    # the +inf prior wins
    np.testing.assert_allclose(r["lse64"][0, 1], np.log(np.exp(1.0) + 0.0), rtol=1e-15)           # items 0 and 3 (-inf) are left
    # an excluded +inf leaves no trace
    r = ref.reference(s[[3]], [1.0], exclude=np.array([[1, 1, 99, -5]]))
    assert r["n_eligible"][0, 0] == 5 and r["zmax"][0, 0] == 2.0


# ---- 3: the float32 restatement holds its share of the GPU test's tolerance, on that test's data ---------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: "B%d-N%d-d%d-J%d-x%d-%s" % (c[:5] + ("prior" if c[5] else "plain",)))
def test_lse32_within_a_quarter_of_the_bar(case):
    user, items, bias, ex, inv_t, scale = ref.case_data(case)
    r = ref.reference(ref.host_scores(user, items), inv_t, bias, scale, ex)
    bar, own = ref.bar(r["lse32"], r["lse64"])
    fin = np.isfinite(r["lse64"])
    np.testing.assert_array_equal(r["lse32"][~fin].astype(np.float64), r["lse64"][~fin])
    err = np.abs(r["lse32"].astype(np.float64)[fin] - r["lse64"][fin])
    print("own error %.3e, smallest bar %.3e" % (own, float(bar[fin].min()) if fin.any() else 0.0))
    assert (err <= bar[fin] / 4).all()
    assert own < 1e-5                          # (a few 1e-6 absolute at |lse| up to ~100: the output's own rounding)


# ---- 4: the symbols and the C ABI --------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_signatures_and_build_list():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, name + " is not declared in include/nrms_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(2).count(",") + 1, name
    assert re.search(r"#define\s+NRMS_LSE_MASS_ONE\s+0x80000000ull", text) and ref.MASS_ONE == 0x80000000
    assert "PARITY UNPINNED" in text.split("nrms_logsumexp_dot_workspace_bytes")[0].rsplit("/* ----", 1)[1]
    build = open(os.path.join(ROOT, "pytorch_news_recommender_amd", "build.py")).read()
    assert '"lsedot.hip"' in build
    lib = _lib.load()
    q = lib.nrms_logsumexp_dot_workspace_bytes
    assert q(10, 100, 8, 4, 3) > 0 and q(10, 100, 8, 4, 3) == q(10, 5000, 300, 4, 70)          # O(B J), whatever N, d, n_exclude
    assert q(512, 130000, 300, 8, 50) >= 512 * 8 * 24
    for bad in ((10, 100, 8, 0, 0), (10, 100, 8, 9, 0), (10, 100, 0, 1, 0), (-1, 100, 8, 1, 0), (10, 0x7FFF0001, 8, 1, 0), (10, 100, 8, 1, -1)):
        assert q(*bad) == 0, bad
    assert q(0, 0, 1, 1, 0) > 0 and q(10, 0x7FFF0000, 8, 8, 0) > 0


C_PROG = r"""
#include "nrms_hip.h"
#include <math.h>
#include <stdio.h>
#include <string.h>

static float u[8], it[8], bi[8], lse[16], zm[16];
static int64_t ex[8];
static int32_t ne[16];
static uint64_t ws[1024], mass[32];

static int expect(int rc, int want, const char* word) {
    const char* msg = nrms_last_error();
    if (rc != want) { printf("FAIL %s: rc=%d\n", word, rc); return 1; }
    if (!msg || !strstr(msg, "logsumexp_dot") || !strstr(msg, word)) { printf("FAIL %s: msg=%s\n", word, msg ? msg : "(null)"); return 1; }
    return 0;
}

#define CALL(B, N, d, J, user, items, bias, t, s, nx, out, w, wb) \
    nrms_logsumexp_dot(B, N, d, J, user, items, bias, t, s, ex, nx, out, zm, ne, w, wb, NULL)

int main(void) {
    float t1[2] = {1.0f, 0.5f}, s1[2] = {1.0f, 0.0f}, tneg[2] = {1.0f, -0.5f}, tinf[2] = {INFINITY, 1.0f}, snan[2] = {1.0f, NAN};
    size_t need = nrms_logsumexp_dot_workspace_bytes(2, 2, 4, 2, 2);
    int bad = 0;
    bad += expect(CALL(-1, 2, 4, 2, u, it, bi, t1, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "B must");
    bad += expect(CALL(2, -1, 4, 2, u, it, bi, t1, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "N must");
    bad += expect(CALL(2, (int64_t)0x7FFF0001, 4, 2, u, it, bi, t1, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "N must");
    bad += expect(CALL(2, 2, 0, 2, u, it, bi, t1, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "d must");
    bad += expect(CALL(2, 2, 4, 0, u, it, bi, t1, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "J must");
    bad += expect(CALL(2, 2, 4, 9, u, it, bi, t1, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "J must");
    bad += expect(CALL(2, 2, 4, 2, u, it, bi, t1, s1, -1, lse, ws, sizeof ws), NRMS_EINVAL, "n_exclude must");
    bad += expect(CALL(2, 2, 4, 2, u, it, bi, NULL, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "inv_temperature is null");
    bad += expect(CALL(2, 2, 4, 2, u, it, bi, tneg, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "inv_temperature must");
    bad += expect(CALL(2, 2, 4, 2, u, it, bi, tinf, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "inv_temperature must");
    bad += expect(CALL(2, 2, 4, 2, u, it, bi, t1, snan, 2, lse, ws, sizeof ws), NRMS_EINVAL, "bias_scale must");
    bad += expect(CALL(2, 2, 4, 2, NULL, it, bi, t1, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "user is null");
    bad += expect(CALL(2, 2, 4, 2, u, NULL, bi, t1, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "items is null");
    bad += expect(CALL(2, 2, 4, 2, u, it, (const float*)((const char*)bi + 2), t1, s1, 2, lse, ws, sizeof ws), NRMS_EINVAL, "bias must be 4-byte aligned");
    bad += expect(CALL(2, 2, 4, 2, u, it, bi, t1, s1, 2, NULL, ws, sizeof ws), NRMS_EINVAL, "lse is null");
    bad += expect(CALL(2, 2, 4, 2, u, it, bi, t1, s1, 2, lse, NULL, sizeof ws), NRMS_EINVAL, "workspace is null");
    bad += expect(CALL(2, 2, 4, 2, u, it, bi, t1, s1, 2, lse, ws, need - 1), NRMS_EWORKSPACE, "workspace");
    bad += expect(CALL(2, 2, 4, 2, u, it, bi, t1, s1, 2, lse, (char*)ws + 4, sizeof ws - 4), NRMS_EINVAL, "workspace must be 8-byte aligned");
    bad += expect(nrms_logsumexp_dot_mass(2, 2, 4, 2, u, it, bi, t1, s1, ex, 2, NULL, ws, sizeof ws, NULL), NRMS_EINVAL, "mass is null");
    bad += expect(nrms_logsumexp_dot_mass(2, 2, 4, 9, u, it, bi, t1, s1, ex, 2, mass, ws, sizeof ws, NULL), NRMS_EINVAL, "logsumexp_dot_mass: J must");
    /* B = 0 is a no-op, whatever else is null; a bad variant is still refused */
    if (nrms_logsumexp_dot(0, 2, 4, 2, NULL, NULL, NULL, t1, NULL, NULL, 0, NULL, NULL, NULL, NULL, 0, NULL) != NRMS_OK) { printf("FAIL B=0\n"); bad++; }
    bad += expect(nrms_logsumexp_dot(0, 2, 4, 2, NULL, NULL, NULL, tneg, NULL, NULL, 0, NULL, NULL, NULL, NULL, 0, NULL), NRMS_EINVAL, "inv_temperature must");
    printf("ONE %llu NEED %lu\n", (unsigned long long)NRMS_LSE_MASS_ONE, (unsigned long)need);
    printf("BAD %d\n", bad);
    return 0;
}
"""


def test_c_abi_validation_and_workspace(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    src, exe = tmp_path / "lse_abi.c", tmp_path / "lse_abi"
    src.write_text(C_PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", lib_dir, "-lnrms_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "BAD 0" in out, out
    assert "ONE %d NEED %d" % (ref.MASS_ONE, 256 + 2 * 2 * 24) in out, out


# ---- 5: the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,ok,word", [
    (["--retrieval_metrics", "10", "--retrieval_nll", "1"], True, None),
    (["--retrieval_metrics", "10", "--retrieval_nll", "0.05,0.5,1,2,inf"], True, None),
    (["--model", "nrms_naml", "--retrieval_metrics", "10", "--retrieval_nll", "1"], True, None),
    (["--model", "nrms_bert", "--retrieval_metrics", "10", "--retrieval_nll", "1"], True, None),
    ([], True, None),
    (["--retrieval_nll", "1"], False, "--retrieval_metrics"),
    (["--retrieval_metrics", "10", "--retrieval_nll", "1,x"], False, "numbers"),
    (["--retrieval_metrics", "10", "--retrieval_nll", "0"], False, "> 0"),
    (["--retrieval_metrics", "10", "--retrieval_nll", "1,-2"], False, "> 0"),
    (["--retrieval_metrics", "10", "--retrieval_nll", "nan"], False, "> 0"),
    (["--retrieval_metrics", "10", "--retrieval_nll", "1,2,3,4,5,6,7,8,9"], False, "1 to 8"),
    (["--retrieval_metrics", "10", "--retrieval_nll", "1", "--negatives", "catalogue", "--catalogue_window", "5"], False, "--catalogue_window"),
    (["--model", "hierec", "--retrieval_metrics", "10", "--retrieval_nll", "1"], False, "hierec"),
    (["--model", "graph", "--retrieval_metrics", "10", "--retrieval_nll", "1"], False, "graph"),
])
def test_check_nll_args(argv, ok, word):
    from pytorch_news_recommender_amd import run_v0
    args = run_v0.build_parser().parse_args(["--dataset", "synthetic"] + ([] if "--model" in argv else ["--model", "nrms_hip"]) + argv)
    if ok:
        got = run_v0.check_nll_args(args)
        assert (got is None) == ("--retrieval_nll" not in argv)
        if got is not None:
            assert got == tuple(float(v) for v in argv[argv.index("--retrieval_nll") + 1].split(","))
    else:
        with pytest.raises(SystemExit) as e:
            run_v0.check_nll_args(args)
        assert "--retrieval_nll" in str(e.value) and word in str(e.value)


# ---- 6: the models -----------------------------------------------------------------------------------------------------------------
def test_catalogue_likelihood_on_all_six_models():
    from importlib import import_module
    want = {"nrms_hip": True, "nrms_v1_hip": True, "nrms_naml_hip": True, "nrms_bert_hip": True, "hierec_hip": False, "graph_hip": False}
    base = import_module("pytorch_news_recommender_amd.model.nrms_hip").Model
    for name, flag in want.items():
        M = import_module("pytorch_news_recommender_amd.model." + name).Model
        assert M.CATALOGUE_LIKELIHOOD is flag, name
        if flag:          # inherited, not re-implemented
            assert M.log_partition is base.log_partition and M.log_prob is base.log_prob, name
        else:
            with pytest.raises(NotImplementedError, match="log_partition is not available"):
                M.log_partition(None, {}, None)
            with pytest.raises(NotImplementedError, match="log_prob is not available"):
                M.log_prob(None, {}, None, None)


def test_temperature_and_bias_scale_checks():
    from pytorch_news_recommender_amd.model.nrms_hip import Model
    f = Model._likelihood_variants
    assert f("x", 2.0, None, None) == ([0.5], None)
    assert f("x", [1.0, float("inf"), 4.0], None, None) == ([1.0, 0.0, 0.25], None)
    assert f("x", [1.0, 2.0], 0.5, torch.zeros(3)) == ([1.0, 0.5], [0.5, 0.5])
    assert f("x", [1.0, 2.0], [0.0, -1.0], torch.zeros(3)) == ([1.0, 0.5], [0.0, -1.0])
    for bad in (0.0, -1.0, float("nan"), [1.0] * 9, []):
        with pytest.raises(_lib.NrmsError, match="temperature"):
            f("x", bad, None, None)
    for scale, bias in (([1.0], torch.zeros(3)), ([1.0, float("inf")], torch.zeros(3)), ([1.0, 2.0], None)):
        with pytest.raises(_lib.NrmsError, match="bias_scale"):
            f("x", [1.0, 2.0], scale, bias)


def test_fma32_on_torch_is_the_restatements():
    from pytorch_news_recommender_amd.model.nrms_hip import _fma32
    from tests.softmax_sample_ref import fma32
    rng = np.random.default_rng(5)
    a = rng.standard_normal(20000).astype(F) * F(100)
    b = rng.standard_normal(20000).astype(F)
    c = rng.standard_normal(20000).astype(F) * F(1e-3)
    a[:6], b[:6], c[:6] = [np.inf, 1, 0, np.nan, -np.inf, 16777216.0], [0, np.inf, 5, 1, 1, 1], [1, -np.inf, -0.0, 1, np.inf, 1.0]
    got = _fma32(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c)).numpy()
    np.testing.assert_array_equal(got.view(np.int32)[~np.isnan(got)], fma32(a, b, c).view(np.int32)[~np.isnan(got)])
    assert np.isnan(fma32(a, b, c)[np.isnan(got)]).all()


# ---- 7: evaluate_retrieval ---------------------------------------------------------------------------------------------------------
class _Engine:
    def retrieval_metrics(self, ranks, ks):
        z = torch.zeros(ranks.shape[0], dtype=torch.float64)
        return dict([("recall@%d" % k, z) for k in ks] + [("ndcg@%d" % k, z) for k in ks] + [("mrr", z)])

    def check_ids(self):
        pass


class _Likely:
    """rank_targets ranks every target but news 7; log_prob gives -id / T."""
    CATALOGUE_LIKELIHOOD = True

    def __init__(self):
        self.engine, self.calls = _Engine(), []

    def encode_catalogue(self, titles):
        return torch.zeros(titles.shape[0], 4)

    def rank_targets(self, batch, targets, catalogue, exclude_history=True, *, item_bias=None):
        return torch.where((targets >= 0) & (targets != 7), torch.ones_like(targets), torch.zeros_like(targets)).to(torch.int32), None

    def log_prob(self, batch, targets, catalogue, temperature=1.0, exclude_history=True, *, item_bias=None, bias_scale=None):
        self.calls.append((tuple(temperature), item_bias, bias_scale))
        t = torch.tensor(temperature, dtype=torch.float32)
        out = -targets.to(torch.float32).unsqueeze(-1) / t
        return torch.where((targets >= 0).unsqueeze(-1) & (targets != 7).unsqueeze(-1), out, torch.full_like(out, float("nan")))

    def check_recommend_ids(self):
        pass


class _Unlikely(_Likely):
    CATALOGUE_LIKELIHOOD = False


def test_evaluate_retrieval_nll_on_a_stub():
    titles = torch.zeros(20, 3, dtype=torch.int64)
    batches = [{"candidate_ids": torch.tensor([[3, 4, 5], [6, 7, 0]])}, {"candidate_ids": torch.tensor([[8, 9, 1]])}]
    labels = [[0, 1, 0], [1, 1], [0, 0, 1]]                # targets 4, 6, 7 (not ranked), 1
    m = _Likely()
    res = train_eval.evaluate_retrieval(None, m, batches, titles, labels, ks=(1,), verbose=False)
    assert "nll" not in res and m.calls == []               # the default: nothing changes, the keyword is not passed on
    p = torch.ones(20)
    res = train_eval.evaluate_retrieval(None, m, batches, titles, labels, ks=(1,), verbose=False, nll_temperatures=(1.0, 2.0), item_bias=p)
    assert res["n_targets"] == 3 and res["n_skipped"] == 1
    assert res["nll"] == {1.0: pytest.approx(11 / 3), 2.0: pytest.approx(11 / 6)}
    assert all(c[0] == (1.0, 2.0) and c[1] is p and c[2] is None for c in m.calls) and len(m.calls) == 2
    with pytest.raises(ValueError, match="windowed"):
        train_eval.evaluate_retrieval(None, m, batches, titles, labels, ks=(1,), verbose=False, nll_temperatures=(1.0,),
                                      item_time=torch.zeros(20, dtype=torch.int32), request_time=[0, 0, 0], window_span=3)
    with pytest.raises(NotImplementedError, match="CATALOGUE_LIKELIHOOD"):
        train_eval.evaluate_retrieval(None, _Unlikely(), batches, titles, labels, ks=(1,), verbose=False, nll_temperatures=(1.0,))
