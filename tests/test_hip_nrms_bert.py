"""nrms_bert on the GPU (model/nrms_bert_hip.py; the reference's model/nrms.py): fixture g9 (outputs of the imported
reference at a small shape and at the real widths 512 / 1024), the fused train step and the autograd path against the
reference's Adam record, a dropout replay into a float64 torch restatement, the benchmarked size against that restatement,
bit-reproducibility, the distinct-id grouping of csrc/newsvec.hip, id validation, evaluation, retrieval, data parallelism and
the run_v0 entry.

Tolerances: scores 2e-5 (fp32) / 1e-4 (bf16x3) absolute; everything else |got - ref| <= rtol |ref| + atol + scale * max|ref|
per tensor (fp32: summation order; bf16x3: ~2^-16 relative per product)."""
import math
import os

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import synth

pytestmark = pytest.mark.gpu

MODES = ["fp32", "bf16x3"]
TOL = {"fp32": dict(score=2e-5, rtol=1e-3, atol=1e-6, scale=2e-5),
       "bf16x3": dict(score=1e-4, rtol=1e-3, atol=1e-6, scale=1e-4)}
SHAPES = {"small": synth.G9_SMALL, "e512": synth.G9_E512, "e1024": synth.G9_E1024}
PARAM_SEED, BATCH_SEED = 31, 32          # tests/golden/gen_nrms_bert.py


def make_config(shape, dropout=0.0, precision="fp32"):
    from pytorch_news_recommender_amd.config import Config
    cfg = Config("nrms_bert")
    cfg.__nrms__()
    cfg.bert_embed_size = shape.bert_embed_size
    cfg.user_heads_num = shape.user_heads_num
    cfg.query_vector_dim_large = shape.query_vector_dim_large
    cfg.dropout = dropout
    cfg.precision = precision
    return cfg


def make_model(shape, params, dropout=0.0, precision="fp32"):
    from pytorch_news_recommender_amd.model.nrms_bert_hip import Model
    m = Model(make_config(shape, dropout, precision), pretrained_news_vectors=params["news_encoder.news_embedding.weight"])
    res = m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    assert not res.missing_keys and not res.unexpected_keys
    return m.to("cuda")


def tbatch(batch, dev="cpu"):
    return {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in batch.items()}


def fwd_bwd(model, batch):
    model.zero_grad()
    scores = model(tbatch(batch))
    loss = torch.nn.CrossEntropyLoss()(scores, torch.zeros(len(scores), dtype=torch.long, device=scores.device))
    loss.backward()
    grads = {n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters()}
    return scores.detach().cpu().numpy(), float(loss.detach()), grads


def close(got, ref, t, name):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = t["rtol"] * np.abs(ref) + t["atol"] + t["scale"] * float(np.abs(ref).max() if ref.size else 0.0)
    diff = np.abs(got - ref)
    worst = float((diff - bound).max()) if diff.size else 0.0
    assert worst <= 0.0, "%s: max |diff| %.3e exceeds the bound by %.3e (scale %.3e)" % (
        name, float(diff.max()), worst, float(np.abs(ref).max()))
    return float(diff.max())


def sample_rows(n_rows, seed=91):
    rows = np.random.default_rng(seed).choice(np.arange(1, n_rows - 1), size=min(6, n_rows - 2), replace=False)
    return np.sort(np.concatenate([[0, n_rows - 1], rows]))


def check_grads(grads, g, tag, t):
    for n, got in grads.items():
        if tag + "/grad/" + n in g:
            close(got, g[tag + "/grad/" + n], t, n)
        else:
            close(got[sample_rows(got.shape[0])], g[tag + "/grad_rows/" + n], t, n + " rows")
            close(got.sum(1, dtype=np.float64), g[tag + "/grad_rowsum/" + n], t, n + " rowsum")
            close(got.sum(0, dtype=np.float64), g[tag + "/grad_colsum/" + n], t, n + " colsum")


# ---- float64 torch restatement of model/nrms.py (the test's own oracle) --------------------------------------------------
def restate(P, batch, heads, keep_nv=None, keep_attn=None, p=0.0):
    """P: name -> float64 tensor (requires_grad as the caller wants), batch: device tensors.  keep_nv [N, E] / keep_attn
    [B, h, H, H] (1 = kept) replay a training forward's dropout.  -> (scores [B, C], news vectors [N, E], user [B, E])."""
    bi, ci, bm, cm = batch["browsed_ids"], batch["candidate_ids"], batch["browsed_mask"], batch["candidate_mask"]
    B, H = bi.shape
    ids = torch.cat([bi.reshape(-1), ci.reshape(-1)])
    nv = P["news_encoder.news_embedding.weight"][ids] @ P["news_encoder.news_dense.0.weight"].T + P["news_encoder.news_dense.0.bias"]
    if keep_nv is not None:
        nv = nv * keep_nv.double() / (1.0 - p)
    E = nv.shape[1]
    hist, cand = nv[:B * H].view(B, H, E), nv[B * H:].view(B, -1, E)
    a = "user_encoder.multi_head_self_attention."
    dk = E // heads
    q, k, v = [(hist @ P[a + "linear_layers.%d.weight" % i].T + P[a + "linear_layers.%d.bias" % i]).view(B, H, heads, dk).transpose(1, 2)
               for i in range(3)]
    s = q @ k.transpose(-2, -1) / math.sqrt(dk)
    m = bm.double()
    s = s.masked_fill((m.unsqueeze(1) * m.unsqueeze(2)).unsqueeze(1) == 0, -1e9)
    pa = torch.softmax(s, -1)
    if keep_attn is not None:
        pa = pa * keep_attn.double() / (1.0 - p)
    x = (pa @ v).transpose(1, 2).reshape(B, H, E) @ P[a + "output_linear.weight"].T + P[a + "output_linear.bias"]
    ad = "user_encoder.additive_attention."
    sc = torch.tanh(x @ P[ad + "linear.weight"].T + P[ad + "linear.bias"]) @ P[ad + "query_vector"]
    w = torch.softmax(sc.masked_fill(bm == 0, -1e9), 1)
    user = (w.unsqueeze(2) * x).sum(1)
    scores = (user.unsqueeze(1) * cand).sum(-1).masked_fill(cm == 0, -1e9)
    return scores, nv, user


def restate_grads(params, batch, heads, **kw):
    dev = "cuda"
    P = {k: torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for k, v in params.items()}
    scores, _, _ = restate(P, tbatch(batch, dev), heads, **kw)
    loss = torch.nn.functional.cross_entropy(scores, torch.zeros(len(scores), dtype=torch.long, device=dev))
    loss.backward()
    return scores.detach().cpu().numpy(), float(loss), {k: P[k].grad.cpu().numpy() for k in params}


# ---- 1, 2: g9 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", ["small", "e512", "e1024"])
def test_g9_forward_backward(golden_dir, tag, mode):
    g = np.load(os.path.join(golden_dir, "g9_nrms_bert.npz"))
    shape = SHAPES[tag]
    params = synth.make_params_bert(shape, seed=PARAM_SEED)
    batch = synth.make_batch_bert(shape, seed=BATCH_SEED)
    model = make_model(shape, params, precision=mode).train()
    assert list(model.state_dict().keys()) == list(g["param_names"])
    t = TOL[mode]
    scores, loss, grads = fwd_bwd(model, batch)
    live = batch["candidate_mask"] != 0
    np.testing.assert_allclose(scores[live], g[tag + "/scores"][live], rtol=0, atol=t["score"])
    assert (scores[~live] == np.float32(-1e9)).all()
    assert abs(loss - float(g[tag + "/loss"])) < t["score"]
    check_grads(grads, g, tag, t)
    if tag == "small":
        # the empty-history user (1) trains row 0 through its padding slots: the row's gradient is not zero
        assert np.abs(grads["news_encoder.news_embedding.weight"][0]).max() > 1e-4
    # the news and user vectors (eval mode equals train mode at dropout 0)
    eng = model.engine
    B, H, Cn, E = shape.batch_size, shape.history_len, shape.n_candidates, shape.bert_embed_size
    nv = eng._saved["nv"].cpu().numpy()
    close(nv[B * H:].reshape(B, Cn, E), g[tag + "/cand"], t, "cand")
    close(eng._saved["user"].cpu().numpy(), g[tag + "/user"], t, "user")
    if tag == "small":
        close(nv[:B * H].reshape(B, H, E), g[tag + "/hist"], t, "hist")
    else:
        close(nv[:B * H][sample_rows(B * H)], g[tag + "/hist_rows"], t, "hist rows")
        close(nv[:B * H].sum(1, dtype=np.float64), g[tag + "/hist_rowsum"], t, "hist rowsum")


# ---- 3: Adam --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "autograd"])
@pytest.mark.parametrize("tag", ["small", "e1024"])
def test_g9_adam(golden_dir, tag, path):
    g = np.load(os.path.join(golden_dir, "g9_nrms_bert.npz"))
    shape = SHAPES[tag]
    params = synth.make_params_bert(shape, seed=PARAM_SEED)
    batch = synth.make_batch_bert(shape, seed=BATCH_SEED)
    model = make_model(shape, params).train()
    tb = tbatch(batch)
    t = dict(TOL["fp32"], scale=5e-5)
    losses, step_scores = [], []
    opt = torch.optim.Adam(model.parameters(), lr=1e-3) if path == "autograd" else None
    for _ in range(3):
        if path == "fused":
            losses.append(float(model.train_step(tb, lr=1e-3)) / shape.batch_size)
            step_scores.append(model._last_scores.cpu().numpy())
        else:
            s = model(tb)
            loss = torch.nn.functional.cross_entropy(s, torch.zeros(len(s), dtype=torch.long, device=s.device))
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss))
            step_scores.append(s.detach().cpu().numpy())
    np.testing.assert_allclose(losses, g[tag + "/adam_loss"], rtol=0, atol=1e-5)
    live = batch["candidate_mask"] != 0
    for i in range(3):
        np.testing.assert_allclose(step_scores[i][live], g[tag + "/adam_scores"][i][live], rtol=0, atol=5e-5)
    if tag == "small":
        # where the reference's first gradient is ~0 (|g| near Adam's eps) fp32 noise may flip an update's sign: those
        # elements are held to the 3 lr an element can move in three steps
        sd = model.state_dict()
        for n in params:
            got, ref = sd[n].cpu().numpy(), g[tag + "/adam_param/" + n]
            firm = np.abs(g[tag + "/grad/" + n]) > 1e-6
            if firm.any():
                close(got[firm], ref[firm], t, n)
            assert (np.abs(got - ref)[~firm] <= 3.1e-3).all(), n


# ---- 4: dropout replay ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["small", "e512"])
def test_dropout_replay(tag):
    from pytorch_news_recommender_amd import _lib
    from pytorch_news_recommender_amd.bert_engine import USER_SEED_SALT
    shape = SHAPES[tag]
    params = synth.make_params_bert(shape, seed=5)
    batch = synth.make_batch_bert(shape, seed=6)
    p = 0.3
    model = make_model(shape, params, dropout=p).train()
    scores, loss, grads = fwd_bwd(model, batch)
    eng = model.engine
    seed = eng._saved["seed"]
    assert seed != 0
    B, H, Cn, E, h = shape.batch_size, shape.history_len, shape.n_candidates, shape.bert_embed_size, shape.user_heads_num
    N = B * (H + Cn)
    keep_nv = eng.dropout_keep_mask(seed, _lib.NRMS_DROPOUT_SITE_NEWSVEC, N, p, d=E)
    keep_attn = eng.dropout_keep_mask(seed ^ USER_SEED_SALT, 2, B * h * H * H // 4, p, d=4).view(B, h, H, H)
    assert 0 < float(keep_nv.float().mean()) < 1 and 0 < float(keep_attn.float().mean()) < 1
    r_scores, r_loss, r_grads = restate_grads(params, batch, h, keep_nv=keep_nv, keep_attn=keep_attn, p=p)
    t = TOL["fp32"]
    live = batch["candidate_mask"] != 0
    np.testing.assert_allclose(scores[live], r_scores[live], rtol=0, atol=t["score"])
    assert abs(loss - r_loss) < t["score"]
    for n in params:
        close(grads[n], r_grads[n], t, n)


# ---- 5: the benchmarked size -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_bench_size_against_float64(mode):
    shape = synth.BertShape(n_news=130000, bert_embed_size=1024, batch_size=512, history_len=50, n_candidates=5)
    params = synth.make_params_bert(shape, seed=11)
    batch = synth.make_batch_bert(shape, seed=12)
    model = make_model(shape, params, precision=mode).train()
    scores, loss, grads = fwd_bwd(model, batch)
    r_scores, r_loss, r_grads = restate_grads(params, batch, shape.user_heads_num)
    live = batch["candidate_mask"] != 0
    err = float(np.abs(scores[live] - r_scores[live]).max())
    bar = 1e-4 if mode == "fp32" else max(1e-4, 1e-5 * float(np.abs(r_scores[live]).max()))
    t = TOL[mode]
    worst = {n: close(grads[n], r_grads[n], t, n) for n in params}
    print("\nnrms_bert B=512 E=1024 %s: max|dscore| %.3e (max|score| %.3f, bar %.1e), |dloss| %.2e, worst gradient %s %.3e"
          % (mode, err, float(np.abs(r_scores[live]).max()), bar, abs(loss - r_loss), max(worst, key=worst.get), max(worst.values())))
    assert err <= bar


# ---- 6: bit-reproducibility -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_train_step_bit_identical(mode):
    shape = synth.BertShape(n_news=5000, bert_embed_size=512, batch_size=64, history_len=50, n_candidates=5)
    params = synth.make_params_bert(shape, seed=3)
    batch = synth.make_batch_bert(shape, seed=4)
    out = []
    for _ in range(2):
        torch.manual_seed(7)
        model = make_model(shape, params, dropout=0.2, precision=mode).train()
        tb = tbatch(batch)
        model.train_step(tb)
        model.train_step(tb)
        out.append(model._flat.detach().clone())
    assert torch.equal(out[0], out[1])


# ---- 7: distinct ids and the table gradient -----------------------------------------------------------------------------------
def test_distinct_ids_and_table_rows():
    shape = synth.BertShape(n_news=2000, bert_embed_size=64, user_heads_num=8, query_vector_dim_large=16, batch_size=32,
                            history_len=20, n_candidates=5)
    params = synth.make_params_bert(shape, seed=8)
    batch = synth.make_batch_bert(shape, seed=9)
    batch["browsed_ids"][:, 10:] = batch["browsed_ids"][:, :10]             # heavy repetition
    model = make_model(shape, params).train()
    _, _, grads = fwd_bwd(model, batch)
    ids = np.concatenate([batch["browsed_ids"].ravel(), batch["candidate_ids"].ravel()])
    uniq = np.unique(ids)
    n, dist = model.engine.distinct_ids(ids.size)
    assert int(n.item()) == uniq.size
    assert np.array_equal(dist[:uniq.size].cpu().numpy(), uniq)
    gt = grads["news_encoder.news_embedding.weight"]
    outside = np.setdiff1d(np.arange(shape.n_news), uniq)
    assert (gt[outside] == 0).all()
    _, _, r_grads = restate_grads(params, batch, shape.user_heads_num)
    close(gt[uniq], r_grads["news_encoder.news_embedding.weight"][uniq], TOL["fp32"], "table rows")


# ---- 8: id validation -------------------------------------------------------------------------------------------------------
def test_out_of_range_ids_counted():
    from pytorch_news_recommender_amd import _lib
    shape = synth.G9_SMALL
    params = synth.make_params_bert(shape, seed=1)
    batch = synth.make_batch_bert(shape, seed=2)
    model = make_model(shape, params).eval()
    good = model(tbatch(batch)).detach().cpu().numpy()
    model.engine.check_ids()
    bad = {k: v.copy() for k, v in batch.items()}
    bad["candidate_ids"][2, 1] = shape.n_news + 5
    bad["browsed_ids"][0, 0] = -3
    with torch.no_grad():
        s = model(tbatch(bad)).cpu().numpy()
    with pytest.raises(_lib.NrmsError, match="2 news id"):
        model.engine.check_ids()
    # read as id 0: the same scores as a batch holding id 0 there
    zero = {k: v.copy() for k, v in batch.items()}
    zero["candidate_ids"][2, 1] = 0
    zero["browsed_ids"][0, 0] = 0
    with torch.no_grad():
        z = model(tbatch(zero)).cpu().numpy()
    np.testing.assert_array_equal(s, z)
    assert not np.array_equal(good, z)


# ---- 9: evaluation ----------------------------------------------------------------------------------------------------------
def test_evaluate_metrics_on_device_feed(tmp_path):
    from pytorch_news_recommender_amd import evaluation, train_eval
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    shape = synth.BertShape(n_news=401, bert_embed_size=512, batch_size=16)
    cfg = make_config(shape)
    cfg.batch_size = 16
    corpus = SyntheticMind(cfg, n_news=400, seed=3)
    samples, labels = corpus.eval_samples(40)
    params = synth.make_params_bert(shape, seed=13)
    params["news_encoder.news_embedding.weight"] = corpus.news_vectors(512)
    model = make_model(shape, params)
    feed = DeviceFeed(cfg, samples, type=1, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict,
                      batch_size=16, device="cuda")
    m = train_eval.evaluate_metrics(cfg, model, feed, labels, verbose=False)
    assert model.last_eval_cache["encoded"] == shape.n_news           # each news id through news_dense once
    model.eval()
    with torch.no_grad():
        per_batch = torch.cat([model(b) for b in feed]).cpu().numpy()
    net, scores, _, _ = train_eval._eval_scores(cfg, model, feed, labels)
    np.testing.assert_allclose(scores.cpu().numpy(), per_batch, rtol=0, atol=1e-6)
    s = scores.cpu().numpy()
    auc = np.mean([evaluation.auc_score(y, s[i, :len(y)]) for i, y in enumerate(labels)])
    mrr = np.mean([evaluation.mrr_score(y, s[i, :len(y)]) for i, y in enumerate(labels)])
    n5 = np.mean([evaluation.ndcg_score(y, s[i, :len(y)], 5) for i, y in enumerate(labels)])
    n10 = np.mean([evaluation.ndcg_score(y, s[i, :len(y)], 10) for i, y in enumerate(labels)])
    assert abs(m["auc"] - auc) < 1e-9 and abs(m["mrr"] - mrr) < 1e-9
    assert abs(m["ndcg5"] - n5) < 1e-9 and abs(m["ndcg10"] - n10) < 1e-9


# ---- 10: retrieval ----------------------------------------------------------------------------------------------------------
def test_catalogue_and_recommend():
    shape = synth.BertShape(n_news=3000, bert_embed_size=512, batch_size=64)
    params = synth.make_params_bert(shape, seed=14)
    batch = synth.make_batch_bert(shape, seed=15)
    model = make_model(shape, params).train()
    cat = model.encode_catalogue(None)
    P = {k: torch.tensor(v, dtype=torch.float64, device="cuda") for k, v in params.items()}
    ref = P["news_encoder.news_embedding.weight"] @ P["news_encoder.news_dense.0.weight"].T + P["news_encoder.news_dense.0.bias"]
    assert float((cat.double() - ref).abs().max()) < 1e-5
    k = 20
    ids, sc = model.recommend(tbatch(batch, "cuda"), k, cat)
    model.check_recommend_ids()
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    browsed = batch["browsed_ids"]
    hist = cat.index_select(0, torch.from_numpy(browsed).cuda().view(-1)).view(64, -1, 512)
    user = model.engine.encode_users(model._flat, hist, torch.from_numpy(browsed != 0).to(torch.uint8).cuda())
    full = (user.double() @ cat.double().T).cpu().numpy()
    bound = 1e-6 * (np.abs(user.double().cpu().numpy()) @ np.abs(cat.double().cpu().numpy()).T)
    for b in range(64):
        excl = set(browsed[b].tolist()) | {0}
        assert not (set(ids[b].tolist()) & excl)
        elig = np.array([i for i in range(shape.n_news) if i not in excl])
        order = elig[np.lexsort((elig, -full[b, elig]))][:k]
        np.testing.assert_allclose(sc[b], full[b, ids[b]], rtol=0, atol=float(bound[b].max()))
        # equal up to ties: every returned id scores at least the k-th best minus the bound
        assert (full[b, ids[b]] >= full[b, order[-1]] - 2 * bound[b, ids[b]]).all()
        mism = ids[b] != order
        assert (np.abs(full[b, ids[b][mism]] - full[b, order[mism]]) <= 2 * bound[b].max()).all()


# ---- 11: data parallelism ---------------------------------------------------------------------------------------------------
def test_two_shard_all_reduce():
    shape = synth.BertShape(n_news=500, bert_embed_size=512, batch_size=8)
    params = synth.make_params_bert(shape, seed=16)
    batch = synth.make_batch_bert(shape, seed=17)
    whole = make_model(shape, params).train()
    whole.train_step(tbatch(batch))
    a, b = make_model(shape, params).train(), make_model(shape, params).train()
    half = lambda lo, hi: {k: v[lo:hi] for k, v in batch.items()}
    ga = {}

    def reduce_a(g):           # shard A runs its backward first; its gradient waits for B's
        ga["g"] = g.clone()

    a.train_step(tbatch(half(0, 4)), world_size=2, all_reduce=reduce_a)
    gb = {}

    def reduce_b(g):
        g += ga["g"]
        gb["g"] = g.clone()

    b.train_step(tbatch(half(4, 8)), world_size=2, all_reduce=reduce_b)
    torch.testing.assert_close(b._flat, whole._flat, rtol=0, atol=2e-6)


# ---- 12: run_v0 ---------------------------------------------------------------------------------------------------------------
def test_run_v0_synthetic_trains_and_recommends(tmp_path, monkeypatch):
    """run_v0 end to end on the synthetic corpus.  The initial dev AUC is that of the same model before its first step:
    run_v0's corpus, dev split and seeded construction, rebuilt here and evaluated."""
    from types import SimpleNamespace

    from pytorch_news_recommender_amd import run_v0, train_eval
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    from pytorch_news_recommender_amd.model import Model
    monkeypatch.chdir(tmp_path)
    data = str(tmp_path / "data")
    out = tmp_path / "rec.txt"
    hist = run_v0.main(["--model", "nrms_bert", "--dataset", "synthetic", "--synthetic_users", "4096", "--batch_size", "128",
                        "--data_path", data, "--save_path", str(tmp_path / "save"), "--epochs", "2", "--recommend", "10",
                        "--recommend_out", str(out)])
    cfg = Config("nrms_bert")
    cfg.batch_size, cfg.data_path, cfg.n_words_title = 128, data + "/", 30
    cfg.__nrms__()
    corpus = SyntheticMind(cfg, n_news=4000, seed=0)
    corpus.train_samples(4096)
    dev, labels = corpus.eval_samples(1024)
    torch.manual_seed(422)
    model = Model(cfg, SimpleNamespace(model="nrms_bert"))
    feed = DeviceFeed(cfg, dev, type=1, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, batch_size=128,
                      device="cuda")
    a0 = train_eval.evaluate(cfg, model, feed, labels, verbose=False)
    a1 = hist["aucs"][-1][1]
    print("\nnrms_bert synthetic dev AUC: initial %.4f, after two epochs (64 steps) %.4f" % (a0, a1))
    assert a1 >= 0.6 and a1 > a0 + 0.05
    lines = out.read_text().splitlines()
    assert len(lines) == 1024 and all(len(eval(l.split(" ", 1)[1])) == 10 for l in lines)
