"""Host side of the pooled loss (csrc/poolce.hip, NRMSEngine.pooled_ce_loss, ClickFeed's candidate_logq, run_v0 --loss pooled): the
float64 restatement the GPU tests compare against, the library's symbols and domain, the logQ table, the CLI and the autograd
refusal.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.config import Config
from pytorch_news_recommender_amd.data_handler import ClickFeed, SyntheticMind
from tests.pooled_ce_ref import inclusion, pooled_ce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(B, Cn, d, R, seed, masked, bias):
    rng = np.random.default_rng(seed)
    M = B * Cn
    cand, user = rng.standard_normal((M, d)), rng.standard_normal((B, d))
    ids = rng.integers(0, max(4, M // 2), size=M).astype(np.int64)
    mask = (rng.random(M) < 0.7).astype(np.uint8) if masked else None
    rej = rng.integers(-1, max(4, M // 2), size=(B, R)).astype(np.int64) if R else None
    cb = rng.standard_normal(M) * 2 if bias else None
    return cand, user, ids, mask, rej, cb


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cn,d,R,masked,bias", [(1, 1, 3, 0, False, False), (2, 2, 1, 1, False, True), (7, 5, 16, 4, True, True),
                                                  (33, 3, 8, 50, True, False), (12, 5, 30, 9, False, True)])
def test_restatement_gradients_equal_torch_float64_autograd(B, Cn, d, R, masked, bias):
    cand, user, ids, mask, rej, cb = _inputs(B, Cn, d, R, 100 * B + d, masked, bias)
    gs = 0.37
    ref = pooled_ce(cand, user, ids, Cn, mask, rej, cb, gs)
    # the same masked logsumexp in torch, the inclusion rule written out with Python loops
    inc = np.zeros((B, B * Cn), dtype=bool)
    for b in range(B):
        own = b * Cn
        if mask is not None and mask[own] == 0:
            continue
        for j in range(B * Cn):
            if j == own:
                inc[b, j] = True
            elif (mask is None or mask[j] != 0) and ids[j] != ids[own] and not (rej is not None and ids[j] > 0 and ids[j] in rej[b].tolist()):
                inc[b, j] = True
    assert np.array_equal(inc, ref["inc"]) and np.array_equal(inc, inclusion(B, Cn, ids, mask, rej))
    c, u = torch.tensor(cand, requires_grad=True), torch.tensor(user, requires_grad=True)
    z = u @ c.T
    if cb is not None:
        z = z + torch.tensor(cb)[None, :]
    live = torch.from_numpy(inc.any(1))
    total = torch.zeros((), dtype=torch.float64)
    losses = np.zeros(B)
    for b in range(B):
        if not bool(live[b]):
            continue
        cols = torch.from_numpy(np.flatnonzero(inc[b]))
        lb = torch.logsumexp(z[b, cols], 0) - z[b, b * Cn]
        losses[b] = float(lb.detach())
        total = total + lb
    (total * gs).backward()
    assert abs(ref["loss_sum"] - float(total.detach())) <= 1e-12 * max(1.0, abs(float(total.detach())))
    np.testing.assert_allclose(ref["loss"], losses, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["duser"], u.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["dcand"], c.grad.numpy(), rtol=0, atol=1e-12)
    not_own = np.ones_like(inc)
    not_own[np.arange(B), np.arange(B) * Cn] = False
    assert ref["n_pairs"] == int((inc & not_own).sum())
    assert not ref["g"][~inc].any()


@pytest.mark.parametrize("B,Cn,d", [(1, 5, 4), (6, 5, 12), (9, 2, 3)])
def test_restatement_reduces_to_rowwise_cross_entropy(B, Cn, d):
    """Reject lists that name every other row's ids leave each row its own C candidates."""
    rng = np.random.default_rng(B)
    M = B * Cn
    cand, user = rng.standard_normal((M, d)), rng.standard_normal((B, d))
    ids = (rng.permutation(M) + 1).astype(np.int64)
    idm = ids.reshape(B, Cn)
    rej = np.stack([np.delete(idm, b, axis=0).reshape(-1) for b in range(B)]) if B > 1 else None
    ref = pooled_ce(cand, user, ids, Cn, None, rej, None, 1.0 / B)
    s = torch.tensor(np.einsum("bcd,bd->bc", cand.reshape(B, Cn, d), user), requires_grad=True)
    loss = torch.nn.functional.cross_entropy(s, torch.zeros(B, dtype=torch.long), reduction="sum")
    (loss / B).backward()
    assert abs(ref["loss_sum"] - float(loss.detach())) <= 1e-12 * max(1.0, float(loss.detach()))
    g = np.zeros((B, M))
    for b in range(B):
        g[b, b * Cn:(b + 1) * Cn] = s.grad.numpy()[b]
    np.testing.assert_allclose(ref["g"], g, rtol=0, atol=1e-12)
    assert ref["n_pairs"] == B * (Cn - 1)


# ---- 2. the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_symbols_and_the_query_knows_the_domain():
    text = open(os.path.join(ROOT, "include", "nrms_hip.h")).read()
    for name in ("nrms_pooled_ce_workspace_bytes", "nrms_pooled_ce_fwd_bwd"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["nrms_pooled_ce_fwd_bwd"][1]) == 18
    assert '"poolce.hip"' in open(os.path.join(ROOT, "pytorch_news_recommender_amd", "build.py")).read()
    lib = _lib.load()
    query = lib.nrms_pooled_ce_workspace_bytes
    for args, word in (((0, 5, 300, 50), b"B=0"), ((512, 65, 300, 50), b"C=65"), ((4097, 8, 300, 50), b"B=4097"), ((32769, 1, 300, 0), b"B=32769"),
                       ((512, 5, 1025, 50), b"d=1025"), ((512, 5, 300, 257), b"R=257"), ((512, 5, 0, 0), b"d=0"), ((512, 5, 300, -1), b"R=-1")):
        assert query(*args) == 0, args
        assert word in lib.nrms_last_error(), (args, lib.nrms_last_error())
    assert query(3641, 9, 8, 0) == 0                                   # B*C = 32 769 with B and C each inside their range
    assert query(4096, 8, 8, 0) > 0                                    # B*C = 32 768
    need = query(512, 5, 300, 50)
    assert need >= 512 * 2560 * 4                                      # the [B, M] matrix is materialised
    assert need <= 512 * 2560 * 4 + 8 * 512 * 300 * 4 + 512 * 4 + 4 * 256
    assert query(1, 1, 1, 0) > 0 and query(4096, 8, 1024, 256) > 0


# ---- 3. the logQ table ------------------------------------------------------------------------------------------------------------
def _config():
    cfg = Config("nrms_hip")
    cfg.__nrms__()
    cfg.n_words_title = 30
    return cfg


@pytest.mark.parametrize("power", [0.75, 0.0, 1.0])
def test_click_feed_logq_table_is_the_formula(power):
    cfg = _config()
    corpus = SyntheticMind(cfg, n_news=300, seed=4)
    user_ptr, clicks = corpus.click_log(30, min_clicks=6, max_clicks=70)
    feed = ClickFeed(cfg, user_ptr, clicks, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, batch_size=8, device="cpu",
                     popularity_power=power)
    N, S = feed.n_news, cfg.sample_size
    assert feed.logq.dtype == torch.float32 and tuple(feed.logq.shape) == (N,)
    # by hand: the positives of the rows, the sampler's own weights
    pos = np.zeros(N)
    for k in feed.row_key.numpy():
        pos[clicks[k]] += 1
    w = feed.weights.numpy().astype(np.float64)
    q = (pos / feed.n_samples + S * w / w.sum()) / (1 + S)
    assert abs(q.sum() - 1.0) <= 1e-12
    with np.errstate(divide="ignore"):
        want = np.log(q).astype(np.float32)
    assert np.array_equal(feed.logq.numpy().view(np.uint32), want.view(np.uint32))
    assert q[0] == 0.0 and feed.logq[0] == float("-inf")               # the padding slot
    count = feed.count.numpy()
    nobody = count == 0
    assert nobody[1:].any()                                            # the log leaves some of the catalogue unclicked
    if power > 0:
        assert (q[nobody] == 0.0).all() and np.isneginf(feed.logq.numpy()[nobody]).all()
    else:
        assert (q[1:] > 0).all()
    assert np.isfinite(feed.logq.numpy()[count > 0]).all()
    # the batch key: gathered by candidate id, lazily
    feed.packed["cand"][:] = torch.from_numpy(np.random.default_rng(0).integers(1, N, size=tuple(feed.packed["cand"].shape)))
    b = feed.batch(torch.arange(5))
    assert "candidate_logq" not in list(b) and len(b) == 13 and not b._vals      # the 13 keys of the reference's layout; nothing gathered yet
    assert "candidate_logq" in b and b.get("candidate_logq") is b["candidate_logq"]
    lq = b["candidate_logq"]
    assert lq.dtype == torch.float32 and tuple(lq.shape) == (5, S + 1)
    assert torch.equal(lq, feed.logq[b["candidate_ids"]])
    assert "ignored" in ClickFeed.__doc__ and "candidate_logq" in ClickFeed.__doc__


def test_other_feeds_do_not_provide_the_key():
    from pytorch_news_recommender_amd.data_handler import DeviceFeed
    cfg = _config()
    corpus = SyntheticMind(cfg, n_news=100, seed=1)
    feed = DeviceFeed(cfg, corpus.train_samples(4), type=0, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict,
                      batch_size=4, device="cpu")
    b = feed.batch(torch.arange(4))
    assert "candidate_logq" not in b and b.get("candidate_logq") is None and len(b) == 13


# ---- 4. run_v0 --loss -------------------------------------------------------------------------------------------------------------
def test_run_v0_loss_flag_is_checked_before_any_data_is_read(tmp_path, monkeypatch):
    from pytorch_news_recommender_amd import run_v0
    p = run_v0.build_parser()
    base = p.parse_args(["--model", "nrms_hip"])
    assert base.loss == "rowwise" and base.no_logq is False
    for model in ("nrms_hip", "nrms_v0", "nrms_v1", "nrms_bert", "nrms_naml"):
        for neg in ("fixed", "epoch", "catalogue"):
            ok = p.parse_args(["--model", model, "--loss", "pooled", "--no_logq", "--negatives", neg, "--dataset", "synthetic"])
            assert ok.loss == "pooled" and ok.no_logq is True
            run_v0.check_loss_args(ok)
            run_v0.check_negatives_args(ok)
    run_v0.check_loss_args(p.parse_args(["--model", "hierec", "--test", "1"]))          # row-wise: nothing to refuse
    monkeypatch.chdir(tmp_path)
    data = tmp_path / "data_processed"
    for argv, word in ((["--model", "nrms_hip", "--loss", "pool"], None),                                              # unknown value
                       (["--model", "hierec", "--loss", "pooled", "--dataset", "synthetic"], "pooled loss"),
                       (["--model", "graph", "--loss", "pooled", "--dataset", "synthetic"], "pooled loss"),
                       (["--model", "gnn", "--loss", "pooled", "--dataset", "synthetic"], "pooled loss"),
                       (["--model", "nrms_hip", "--loss", "pooled", "--dataset", "synthetic", "--test", "1"], "--test")):
        with pytest.raises(SystemExit) as e:
            run_v0.main(["--data_path", str(data)] + argv)
        if word is not None:
            assert word in str(e.value) and "--loss pooled" in str(e.value), (argv, e.value)
        assert not data.exists(), argv


# ---- 5. the autograd path ---------------------------------------------------------------------------------------------------------
def test_autograd_training_refuses_the_pooled_loss():
    from pytorch_news_recommender_amd import train_eval

    class Net(torch.nn.Module):
        def forward(self, batch):
            raise AssertionError("the refusal comes before any batch is read")

    cfg = _config()
    cfg.train_loss = "pooled"

    def batches():
        raise AssertionError("the refusal comes before any batch is read")
        yield

    with pytest.raises(ValueError, match="pooled"):
        train_eval.train(cfg, Net(), batches(), use_autograd=True, verbose=False)


def test_train_loss_names_are_checked():
    from pytorch_news_recommender_amd.model._flat_model import FlatHipModel

    class M(FlatHipModel):
        def __init__(self, cfg):
            torch.nn.Module.__init__(self)
            self.config = cfg

    cfg = _config()
    assert cfg.train_loss == "rowwise" and cfg.logq_correction is True
    assert M(cfg)._train_loss() == "rowwise"
    del cfg.train_loss
    assert M(cfg)._train_loss() == "rowwise"                           # a config written before the field existed
    cfg.train_loss = "pooled"
    assert M(cfg)._train_loss() == "pooled"
    cfg.train_loss = "listwise"
    with pytest.raises(ValueError, match="train_loss"):
        M(cfg)._train_loss()
