"""nrms_logsumexp_dot on the GPU (the exact log-partition of the served softmax over the catalogue, include/nrms_hip.h): the
maximum and the count bit for bit against the restatement (tests/lse_ref.py) formed from nrms_rank_dot's score bits, lse
against float64 within a bar set by the float32 restatement's own error, the integer identities of the mass, invariance bit
for bit (batch, order, geometry, workspace contents, run), exclusion ahead of the maximum, every NaN / inf rule, the buffer
contract, and the layers built on it (NRMSEngine.log_partition, Model.log_partition / log_prob, evaluate_retrieval)."""
import ctypes as C

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, train_eval
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine

from tests import lse_ref as ref
from tests.guarded import POISONS, Pool, assert_same_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
_ENG = []
_SCORES = {}


def _engine():
    if not _ENG:
        _ENG.append(NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), DEV))
    return _ENG[0]


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lse(user, items, inv_t, bias=None, scale=None, ex=None):
    """(lse, zmax, n_eligible) as numpy [B, J], through the engine."""
    out = _engine().log_partition(_dev(user), _dev(items), list(map(float, inv_t)), _dev(ex, torch.int64), bias=_dev(bias),
                                  bias_scale=None if scale is None else list(map(float, scale)))
    return tuple(t.cpu().numpy() for t in out)


def _mass(user, items, inv_t, bias=None, scale=None, ex=None):
    m = _engine().log_partition(_dev(user), _dev(items), list(map(float, inv_t)), _dev(ex, torch.int64), bias=_dev(bias),
                                bias_scale=None if scale is None else list(map(float, scale)), return_mass=True)
    return m.cpu().numpy().view(np.uint64)


def _score_bits(user, items):
    """float32 [B, N]: nrms_rank_dot's target_scores for every (user, item) pair, NaN where the chain gives NaN."""
    B, N = user.shape[0], items.shape[0]
    if N == 0:
        return np.zeros((B, 0), np.float32)
    targets = np.broadcast_to(np.arange(N, dtype=np.int64), (B, N))
    _, sc = _engine().rank_of(_dev(user), _dev(items), _dev(targets, torch.int64))
    sc = sc.cpu().numpy()
    sc[:, np.isnan(items).any(axis=1)] = np.nan               # (rank_dot reports a NaN score as -inf)
    return sc


def _case(case):
    """The case's data, its score bits and the restatement on them: computed once, shared, never changed."""
    if case not in _SCORES:
        data = ref.case_data(case)
        user, items, bias, ex, inv_t, scale = data
        scores = _score_bits(user, items)
        _SCORES[case] = (data, scores, ref.reference(scores, inv_t, bias, scale, ex))
    return _SCORES[case]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def _same(a, b, what):
    for x, y, name in zip(a, b, ("lse", "zmax", "n_eligible")):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg="%s: %s" % (what, name))


def _check_lse(lse, r, what):
    """Infinite entries exactly, finite ones within the case's bar; prints the figures first."""
    fin = np.isfinite(r["lse64"])
    bar, own = ref.bar(r["lse32"], r["lse64"])
    with np.errstate(invalid="ignore"):
        err = np.abs(lse.astype(np.float64) - r["lse64"])
    worst = float(err[fin].max()) if fin.any() else 0.0
    print("%s: max |lse - lse64| device %.3e, fp32 restatement %.3e, smallest bar %.3e"
          % (what, worst, own, float(bar[fin].min()) if fin.any() else 0.0))
    np.testing.assert_array_equal(lse[~fin].astype(np.float64), r["lse64"][~fin], err_msg=what)
    assert np.isfinite(lse[fin]).all() and (err[fin] <= bar[fin]).all(), what
    return worst


# ---- 1. every shape at which the kernels take another path ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: "B%d-N%d-d%d-J%d-x%d-%s" % (c[:5] + ("prior" if c[5] else "plain",)))
def test_against_the_restatement_on_rank_dot_score_bits(case):
    (user, items, bias, ex, inv_t, scale), scores, r = _case(case)
    lse, zmax, n_el = _lse(user, items, inv_t, bias, scale, ex)
    np.testing.assert_array_equal(n_el, r["n_eligible"])
    np.testing.assert_array_equal(_bits(zmax), _bits(r["zmax"]))
    _check_lse(lse, r, "case %s" % (case,))
    if items.shape[0]:
        # variant 0 has inv_temperature 1 and scale 1: fmaf(s, 1, c) is s + c rounded once, which is the (biased) top-k's score
        top, _ = _engine().top_k(_dev(user), _dev(items), 1, _dev(ex, torch.int64), bias=_dev(bias))
        np.testing.assert_array_equal(_bits(zmax[:, 0]), _bits(top.cpu().numpy()[:, 0]))
    # inv_temperature 0 without a prior: every logit is +0, so every eligible item weighs exactly one
    m = _mass(user, items, [0.0], ex=ex)
    z0 = ref.reference(scores, [0.0], exclude=ex)
    np.testing.assert_array_equal(m[:, 0, 0], z0["n_eligible"][:, 0].astype(np.uint64) * np.uint64(ref.MASS_ONE))
    assert (m[:, 0, 1] == 0).all()


def test_a_catalogue_stored_twice_doubles_the_mass_exactly():
    (user, items, bias, ex, inv_t, scale), _, r = _case(ref.CASES[7])
    N = items.shape[0]
    items2, bias2 = np.concatenate([items, items]), np.concatenate([bias, bias])
    ex2 = np.concatenate([ex, np.where((ex >= 0) & (ex < N), ex + N, -1)], axis=1)          # the same news, in both copies
    once, twice = _mass(user, items, inv_t, bias, scale, ex), _mass(user, items2, inv_t, bias2, scale, ex2)
    fin = np.isfinite(r["lse64"])
    assert fin.any() and (once[fin] > 0).any()
    np.testing.assert_array_equal(twice, 2 * once)
    a, b = _lse(user, items, inv_t, bias, scale, ex), _lse(user, items2, inv_t, bias2, scale, ex2)
    np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]))
    np.testing.assert_array_equal(2 * a[2], b[2])
    # log(2 m) - log(m) = log 2 up to the two roundings of the outputs, half an ulp each
    assert np.abs((b[0][fin].astype(np.float64) - a[0][fin]) - np.log(2.0)).max() <= np.spacing(np.abs(b[0][fin]).max())


# ---- 2. invariance, bit for bit -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inv_case():
    """65 users x 50 011 items: one row alone runs 98 slices of 512 items, the batch 49 slices of 1 024."""
    rng = np.random.default_rng(21)
    B, N, d = 65, 50011, 12
    user = rng.standard_normal((B, d)).astype(np.float32)
    items = (rng.standard_normal((N, d)) * 0.6).astype(np.float32)
    items[rng.choice(N, size=40, replace=False)] = np.nan
    bias = rng.standard_normal(N).astype(np.float32)
    bias[rng.choice(N, size=7, replace=False)] = np.nan
    ex = rng.integers(0, N, size=(B, 50)).astype(np.int64)
    ex[:, 0], ex[:, 1] = -1, N
    inv_t, scale = [1.0, 4.0, 0.0, 0.37], [1.0, 0.0, -0.5, 2.0]
    return user, items, bias, ex, inv_t, scale, _lse(user, items, inv_t, bias, scale, ex)


def test_a_row_does_not_depend_on_its_batch(inv_case):
    user, items, bias, ex, inv_t, scale, full = inv_case
    for b in (0, 31, 32, 64):
        alone = _lse(user[b:b + 1], items, inv_t, bias, scale, ex[b:b + 1])
        _same(alone, tuple(x[b:b + 1] for x in full), "row %d alone" % b)
    for lo, hi in ((0, 33), (33, 65), (1, 32)):
        _same(_lse(user[lo:hi], items, inv_t, bias, scale, ex[lo:hi]), tuple(x[lo:hi] for x in full), "rows %d..%d" % (lo, hi))
    _same(_lse(user[::-1], items, inv_t, bias, scale, ex[::-1]), tuple(x[::-1] for x in full), "rows reversed")


def test_permuted_and_padded_catalogues_and_variants_one_by_one(inv_case):
    user, items, bias, ex, inv_t, scale, full = inv_case
    N = items.shape[0]
    p = np.random.default_rng(22).permutation(N)
    inv = np.argsort(p)
    ex_p = np.where((ex >= 0) & (ex < N), inv[np.clip(ex, 0, N - 1)], ex)
    _same(_lse(user, items[p], inv_t, bias[p], scale, ex_p), full, "permuted catalogue")
    # 3 000 more rows nobody can get: a NaN prior each (and real vectors, which must not matter)
    pad = np.random.default_rng(23).standard_normal((3000, items.shape[1])).astype(np.float32) * 50
    _same(_lse(user, np.concatenate([items, pad]), inv_t, np.concatenate([bias, np.full(3000, np.nan, np.float32)]), scale, ex), full,
          "catalogue padded with NaN-prior rows")
    for j in range(len(inv_t)):
        one = _lse(user, items, inv_t[j:j + 1], bias, scale[j:j + 1], ex)
        _same(one, tuple(x[:, j:j + 1] for x in full), "variant %d on its own" % j)
    _same(_lse(user, items, inv_t[::-1], bias, scale[::-1], ex), tuple(x[:, ::-1] for x in full), "variants reversed")
    _same(_lse(user, items, inv_t, bias, scale, ex), full, "a second run")


def test_guard_bands_and_poisoned_workspaces():
    """The C ABI directly, every buffer between guard bands, the workspace and the outputs poisoned three ways."""
    (user, items, bias, ex, inv_t, scale), _, r = _case(ref.CASES[8])
    B, d = user.shape
    N, J, n_ex = items.shape[0], len(inv_t), ex.shape[1]
    lib = _lib.load()
    nbytes = lib.nrms_logsumexp_dot_workspace_bytes(B, N, d, J, n_ex)
    assert nbytes == 256 + B * J * 24
    it_arr, sc_arr = (C.c_float * J)(*map(float, inv_t)), (C.c_float * J)(*map(float, scale))
    runs = {}
    for poison in POISONS:
        pool = Pool(poison)
        u = pool.elems("user", B * d, init=_dev(user).view(-1))
        it = pool.elems("items", N * d, init=_dev(items).view(-1))
        bi = pool.elems("bias", N, init=_dev(bias))
        x = pool.elems("exclude", B * n_ex, torch.int64, init=_dev(ex, torch.int64).view(-1))
        lse, zmax = pool.elems("lse", B * J), pool.elems("zmax", B * J)
        n_el = pool.elems("n_eligible", B * J, torch.int32)
        mass = pool.elems("mass", B * J * 2, torch.int64)
        ws = pool.new("workspace", nbytes)
        snap = {n: pool[n].snapshot() for n in ("user", "items", "bias", "exclude")}
        rc = lib.nrms_logsumexp_dot(B, C.c_int64(N), d, J, u.ptr, it.ptr, bi.ptr, it_arr, sc_arr, x.ptr, n_ex, lse.ptr, zmax.ptr, n_el.ptr,
                                    ws.ptr, C.c_size_t(nbytes), _stream())
        _lib.check(rc, "nrms_logsumexp_dot")
        rc = lib.nrms_logsumexp_dot_mass(B, C.c_int64(N), d, J, u.ptr, it.ptr, bi.ptr, it_arr, sc_arr, x.ptr, n_ex, mass.ptr, ws.ptr,
                                         C.c_size_t(nbytes), _stream())
        _lib.check(rc, "nrms_logsumexp_dot_mass")
        pool.intact("nrms_logsumexp_dot")
        for n, s in snap.items():
            assert pool[n].unchanged_since(s), n
        runs[poison] = {"lse": lse.numpy((B, J)), "zmax": zmax.numpy((B, J)), "n_eligible": n_el.numpy((B, J)), "mass": mass.numpy((B, J, 2))}
        # the nullable outputs left out: lse is the same
        lse2 = pool.elems("lse2", B * J)
        rc = lib.nrms_logsumexp_dot(B, C.c_int64(N), d, J, u.ptr, it.ptr, bi.ptr, it_arr, sc_arr, x.ptr, n_ex, lse2.ptr, None, None,
                                    ws.ptr, C.c_size_t(nbytes), _stream())
        _lib.check(rc, "nrms_logsumexp_dot")
        pool.intact("nrms_logsumexp_dot without zmax / n_eligible")
        assert lse2.numpy((B, J)).tobytes() == runs[poison]["lse"].tobytes()
    assert_same_bits(runs, "nrms_logsumexp_dot")
    np.testing.assert_array_equal(runs[POISONS[0]]["n_eligible"], r["n_eligible"])
    np.testing.assert_array_equal(_bits(runs[POISONS[0]]["zmax"]), _bits(r["zmax"]))


# ---- 3. exclusion comes before the maximum ---------------------------------------------------------------------------------------
def test_an_excluded_item_far_above_the_rest_leaves_no_trace():
    """Temperature 0.05: taken back out AFTER a maximum that includes it, every eligible term would have underflowed to 0."""
    rng = np.random.default_rng(31)
    B, N, d = 33, 700, 32
    user = rng.standard_normal((B, d)).astype(np.float32)
    items = (rng.standard_normal((N, d)) * 0.2).astype(np.float32)
    hot = rng.choice(N, size=B, replace=False)
    for b in range(B):          # user b's own hot item scores 8 |user b|^2, a hundred and more above every cold item
        items[hot[b]] = user[b] * 8
    ex = np.broadcast_to(hot.astype(np.int64), (B, B)).copy()               # nobody may get a hot item
    scores = _score_bits(user, items)
    inv_t = [20.0, 1.0]
    r = ref.reference(scores, inv_t, exclude=ex)
    with_hot = ref.reference(scores, inv_t)
    assert ((with_hot["zmax"][:, 0] - r["zmax"][:, 0]) > 200).all()          # exp(-200) is 0 in fp32: the broken scheme gives log 0
    lse, zmax, n_el = _lse(user, items, inv_t, ex=ex)
    np.testing.assert_array_equal(_bits(zmax), _bits(r["zmax"]))
    np.testing.assert_array_equal(n_el, r["n_eligible"])
    _check_lse(lse, r, "excluded hot item")
    m = _mass(user, items, inv_t, ex=ex)
    assert (m[:, :, 0] >= ref.MASS_ONE).all()                                 # the maximum itself always weighs one


# ---- 4. NaN and inf -------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_rules_on_the_device():
    inf, nan = np.inf, np.nan
    rows = np.array([[1.0, nan, 2.0, -inf, 0.5, 3.0], [nan] * 6, [-inf] * 6, [1.0, inf, 2.0, 0.0, 0.0, 0.0],
                     [-0.0, -1.0, -2.0, -3.0, -4.0, -5.0]], dtype=np.float32)
    bias = np.array([0.0, 0.0, nan, 0.0, -inf, inf], dtype=np.float32)
    user = np.ones((1, 1), np.float32)
    for i, row in enumerate(rows):          # d = 1 and user = 1: the scores are the row itself
        items = row.reshape(-1, 1)
        for kw in ({}, {"bias": bias, "scale": [1.0, 0.0]}, {"ex": np.array([[1, 1, 99, -5]])}):
            r = ref.reference(row[None, :], [1.0, 0.0], kw.get("bias"), kw.get("scale"), kw.get("ex"))
            lse, zmax, n_el = _lse(user, items, [1.0, 0.0], **kw)
            np.testing.assert_array_equal(n_el, r["n_eligible"], err_msg="row %d %s" % (i, sorted(kw)))
            np.testing.assert_array_equal(_bits(zmax), _bits(r["zmax"]), err_msg="row %d %s" % (i, sorted(kw)))
            _check_lse(lse, r, "row %d %s" % (i, sorted(kw)))
            assert not np.isnan(lse).any()


# ---- 5. argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    eng = _engine()
    user, items = torch.zeros(4, 8, device=DEV), torch.zeros(10, 8, device=DEV)
    for inv_t in ([-1.0], [float("inf")], [float("nan")]):
        with pytest.raises(_lib.NrmsError, match="inv_temperature"):
            eng.log_partition(user, items, inv_t)
    with pytest.raises(_lib.NrmsError, match="bias_scale"):
        eng.log_partition(user, items, [1.0], bias=torch.zeros(10, device=DEV), bias_scale=[float("inf")])
    with pytest.raises(_lib.NrmsError, match="bias_scale"):
        eng.log_partition(user, items, [1.0, 2.0], bias=torch.zeros(10, device=DEV), bias_scale=[1.0])
    with pytest.raises(_lib.NrmsError, match="J="):
        eng.log_partition(user, items, [1.0] * 9)
    with pytest.raises(_lib.NrmsError, match="bias"):
        eng.log_partition(user, items, [1.0], bias=torch.zeros(9, device=DEV))
    with pytest.raises(_lib.NrmsError, match="width"):
        eng.log_partition(user, torch.zeros(10, 7, device=DEV), [1.0])
    lib = _lib.load()
    out = torch.zeros(4, device=DEV)
    ws = torch.zeros(64, dtype=torch.int64, device=DEV)
    need = lib.nrms_logsumexp_dot_workspace_bytes(4, 10, 8, 1, 0)
    rc = lib.nrms_logsumexp_dot(4, C.c_int64(10), 8, 1, _lib.ptr(user), _lib.ptr(items), None, (C.c_float * 1)(1.0), None, None, 0,
                                _lib.ptr(out), None, None, _lib.ptr(ws), C.c_size_t(need - 1), _stream())
    assert rc == _lib.NRMS_EWORKSPACE and b"logsumexp_dot: workspace" in lib.nrms_last_error()
    # B = 0 and N = 0
    lse, zmax, n_el = eng.log_partition(torch.zeros(0, 8, device=DEV), items, [1.0, 2.0])
    assert lse.shape == (0, 2)
    lse, zmax, n_el = eng.log_partition(user, torch.zeros(0, 8, device=DEV), [1.0, 2.0])
    assert bool(torch.isneginf(lse).all()) and bool(torch.isneginf(zmax).all()) and int(n_el.abs().sum()) == 0


# ---- 6. the model and the evaluation loop -----------------------------------------------------------------------------------------
def _model(kind):
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    from tests.test_hip_mmr import _tiny_cfg
    torch.manual_seed(0)
    cfg = _tiny_cfg(kind)
    corpus = SyntheticMind(cfg, n_news=300, n_topics=4, seed=1)
    if kind == "nrms_naml":
        from pytorch_news_recommender_amd.model.nrms_naml_hip import Model
        cfg.user_heads_num, cfg.cate_embed_size, cfg.query_vector_dim_large = 4, 20, 40
        cfg.news_feature_size = 2 * cfg.word_embed_size + 2 * cfg.cate_embed_size
    else:
        from pytorch_news_recommender_amd.model.nrms_hip import Model
    model = Model(cfg, pretrained_word_embedding=corpus.embedding_table(cfg.word_embed_size)).to("cuda")
    samples, labels = corpus.eval_samples(64, max_shown=20)
    feed = DeviceFeed(cfg, samples, type=1, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict,
                      batch_size=cfg.batch_size, device=DEV)
    info = feed.news_info() if kind == "nrms_naml" else None
    return cfg, model, feed, labels, info


@pytest.mark.parametrize("kind", ["nrms_v0", "nrms_naml"])
def test_model_log_partition_log_prob_and_evaluate_retrieval(kind):
    cfg, model, feed, labels, info = _model(kind)
    cat = model.encode_catalogue(feed.titles, **(info or {}))
    N = cat.shape[0]
    temps = [1.0, 0.25, float("inf")]
    prior = torch.randn(N, device=DEV)
    prior[5] = float("nan")
    batch = next(iter(feed))
    B = batch["browsed_ids"].shape[0]
    every = torch.arange(0, N + 1, device=DEV).expand(B, N + 1).contiguous()          # id 0 and id N: never valid
    for kw in ({}, {"item_bias": prior, "bias_scale": [1.0, 0.5, 2.0]}, {"item_bias": prior}):
        lse, zmax, n_el = model.log_partition(batch, cat, temps, return_stats=True, **kw)
        assert lse.shape == (B, 3) and torch.equal(lse, model.log_partition(batch, cat, temps, **kw))
        lp = model.log_prob(batch, every, cat, temps, **kw)
        ranks, _ = model.rank_targets(batch, every, cat, **({"item_bias": prior} if kw else {}))
        assert lp.shape == (B, N + 1, 3) and lp.dtype == torch.float32
        valid = ranks > 0
        assert torch.equal(torch.isnan(lp[..., 0]), ~valid) and torch.equal(valid.sum(1).to(torch.int32), n_el[:, 0])
        assert bool((lp[valid] <= 0).all())
        total = torch.where(valid.unsqueeze(-1), lp.double().exp(), torch.zeros_like(lp, dtype=torch.float64)).sum(1)
        print("%s %s: max |sum exp(log_prob) - 1| = %.3e" % (kind, sorted(kw), float((total - 1).abs().max())))
        # every term carries the roundings of lse and of the difference, half an fp32 ulp each: below 3.1e-5 relative to the
        # term for |lse| < 256, and the sum of the terms is 1; the device's lse itself is a few 1e-6 off (docs/EXPERIMENTS.md)
        assert float((total - 1).abs().max()) < 1e-4
        if not kw:            # the uniform variant: log n_eligible, and the history counts
            assert torch.allclose(lse[:, 2].double(), n_el[:, 2].double().log(), atol=1e-6, rtol=0)
            wide = model.log_partition(batch, cat, temps, exclude_history=False, return_stats=True)
            assert bool((wide[2] >= n_el).all()) and bool((wide[2] == N - 1).all()) and bool((wide[0][:, 2] >= lse[:, 2]).all())
    # a scalar temperature is J = 1
    assert model.log_partition(batch, cat, 0.25).shape == (B, 1)
    with pytest.raises(_lib.NrmsError, match="temperature"):
        model.log_partition(batch, cat, 0.0)
    model.check_recommend_ids()
    # the evaluation loop: the mean of -log_prob over the ranked targets, one temperature at a time or all at once
    news_info = {} if info is None else {"news_info": info}
    base = train_eval.evaluate_retrieval(cfg, model, feed, feed.titles, labels, ks=(10,), verbose=False, **news_info)
    res = train_eval.evaluate_retrieval(cfg, model, feed, feed.titles, labels, ks=(10,), verbose=False, nll_temperatures=(1.0, 0.25), **news_info)
    assert "nll" not in base and {k: v for k, v in res.items() if k != "nll"} == base
    assert set(res["nll"]) == {1.0, 0.25} and all(np.isfinite(v) and v > 0 for v in res["nll"].values())
    tg = model.last_retrieval_metrics["targets"]
    want, n, done = 0.0, 0, 0
    for b in feed:
        rows = tg[done:done + b["browsed_ids"].shape[0]]
        done += rows.shape[0]
        lp = model.log_prob(b, rows, cat, [1.0])[..., 0]
        want -= float(lp[~torch.isnan(lp)].double().sum())
        n += int((~torch.isnan(lp)).sum())
    assert n == res["n_targets"] and res["nll"][1.0] == pytest.approx(want / n, rel=1e-9)
    one = train_eval.evaluate_retrieval(cfg, model, feed, feed.titles, labels, ks=(10,), verbose=False, nll_temperatures=(0.25,), **news_info)
    assert one["nll"][0.25] == res["nll"][0.25]
    with pytest.raises(ValueError, match="windowed"):
        train_eval.evaluate_retrieval(cfg, model, feed, feed.titles, labels, ks=(10,), verbose=False, nll_temperatures=(1.0,),
                                      item_time=torch.zeros(N, dtype=torch.int32, device=DEV), request_time=[0] * len(labels), window_span=3,
                                      **news_info)
