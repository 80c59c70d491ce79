"""The pooled loss through the engines and the fused train step (config.train_loss = "pooled"): nrms_v0, nrms_v1, nrms_bert and
nrms_naml at the small shapes of their own parity tests, precision fp32, dropout 0.

Gradient parity: the flat gradient one pooled train_step leaves, against a reference in which the oracle's torch encoders
(oracle/nrms_oracle.py, oracle/naml_oracle.py; for nrms_bert the float64 restatement of tests/test_hip_nrms_bert.py) produce the
candidate and user vectors with autograd, the pooled loss on them is written in torch (masked logsumexp over the inclusion rule of
tests/pooled_ce_ref.py), and .backward() gives the gradient.  Bars: TOL["fp32"] of tests/test_hip_parity.py."""
import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, synth
from tests.pooled_ce_ref import inclusion
from tests.test_hip_parity import TOL, assert_grad_close

pytestmark = pytest.mark.gpu

V0_SHAPE = synth.G1_ODD
V1_SHAPE = synth.Shape(n_words=90, word_embed_size=48, num_attention_heads=4, query_vector_dim=16, batch_size=3, history_len=5,
                       n_candidates=2, n_words_title=7)                       # tests/test_hip_v1.py
V1_TITLE_HEADS = 2


def tbatch(batch, dev="cpu"):
    return {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in batch.items()}


def add_pool_keys(batch, B, H, Cn, seed, dead_row=True, n_ids=None):
    """The keys the pooled loss reads, for batches whose models do not use news ids: ids from a small range (n_ids, by default half
    the pool: columns repeat positives and sit in histories), histories padded with 0, a logQ per slot; and one row whose positive
    is masked."""
    rng = np.random.default_rng(seed)
    n_ids = max(4, B * Cn // 2) if n_ids is None else n_ids
    batch = dict(batch)
    batch["candidate_ids"] = rng.integers(1, n_ids + 1, size=(B, Cn)).astype(np.int64)
    hist = rng.integers(1, n_ids + 1, size=(B, H)).astype(np.int64)
    batch["browsed_ids"] = np.where(np.asarray(batch["browsed_mask"]) != 0, hist, 0)
    batch["candidate_logq"] = np.log(rng.uniform(0.01, 0.5, size=(B, Cn))).astype(np.float32)
    if dead_row and B > 1:
        m = np.array(batch["candidate_mask"], copy=True)
        m[B - 1, 0] = 0
        batch["candidate_mask"] = m
    return batch


def torch_pooled_loss(cand, user, batch, logq=True):
    """cand [B, C, d], user [B, d] (autograd tensors) -> the mean over the batch of the pooled loss, in torch."""
    B, Cn, d = cand.shape
    M = B * Cn
    inc = torch.from_numpy(inclusion(B, Cn, np.asarray(batch["candidate_ids"]).reshape(-1), np.asarray(batch["candidate_mask"]).reshape(-1),
                                     np.asarray(batch["browsed_ids"]))).to(cand.device)
    z = user @ cand.reshape(M, d).T
    if logq and "candidate_logq" in batch:
        z = z - torch.from_numpy(np.asarray(batch["candidate_logq"]).reshape(-1)).to(z)[None, :]
    zm = torch.where(inc, z, torch.full_like(z, float("-inf")))
    own = torch.arange(B, device=cand.device) * Cn
    live = inc[torch.arange(B), own]
    loss = (torch.logsumexp(zm[live], dim=1) - z[live, own[live]]).sum()
    return loss / B


def pooled_step(model, batch):
    """One pooled train_step -> (mean loss, {name: gradient}) -- the flat gradient buffer the optimizer consumed."""
    model.config.train_loss = "pooled"
    model.train()
    loss_sum = model.train_step(tbatch(batch), lr=1e-3)
    B = np.asarray(batch["candidate_mask"]).shape[0]
    g = model._opt["g"]
    return float(loss_sum) / B, {n: model._layout.view(g, n).detach().cpu().numpy().copy() for n in model._names}


def grads_of(p):
    return {k: (v.grad.detach().cpu().numpy() if v.grad is not None else np.zeros(tuple(v.shape), np.float32)) for k, v in p.items()}


def compare(loss, grads, ref_loss, ref_grads, names=None):
    print("pooled step: loss %.7f reference %.7f" % (loss, ref_loss))
    assert abs(loss - ref_loss) < TOL["fp32"]["score"]
    worst = 0.0
    for name, ref in ref_grads.items():
        got = grads[name if names is None else names[name]]
        assert_grad_close(got, ref, "fp32", name)
        worst = max(worst, float(np.abs(got - ref).max()))
    print("pooled step: largest gradient difference %.2e over %d tensors" % (worst, len(ref_grads)))
    assert sum(bool(np.abs(r).max() > 1e-6) for r in ref_grads.values()) >= len(ref_grads) // 2        # the reference is not trivially zero


def test_nrms_v0_pooled_gradient():
    from oracle import nrms_oracle as orc
    from tests.test_hip_parity import make_model
    shape = V0_SHAPE
    params = synth.make_params(shape, seed=101)
    batch = add_pool_keys(synth.make_batch(shape, seed=102, ragged=True, min_title=1, mask_some_candidates=True), shape.batch_size,
                          shape.history_len, shape.n_candidates, seed=5)
    loss, grads = pooled_step(make_model(shape, params), batch)
    p = orc.to_torch(params, torch.float32, requires_grad=True)
    _, aux = orc.forward(p, batch, shape.num_attention_heads)
    ref = torch_pooled_loss(aux["cand"], aux["user"], batch)
    ref.backward()
    compare(loss, grads, float(ref.detach()), grads_of(p))


def test_nrms_v0_pooled_gradient_without_the_correction_and_without_histories():
    """config.logq_correction = False ignores candidate_logq; a batch without browsed_ids rejects nothing."""
    from oracle import nrms_oracle as orc
    from tests.test_hip_parity import make_model
    shape = V0_SHAPE
    params = synth.make_params(shape, seed=103)
    batch = add_pool_keys(synth.make_batch(shape, seed=104, ragged=True, min_title=1), shape.batch_size, shape.history_len,
                          shape.n_candidates, seed=6, dead_row=False)
    del batch["browsed_ids"]
    model = make_model(shape, params)
    model.config.logq_correction = False
    loss, grads = pooled_step(model, batch)
    p = orc.to_torch(params, torch.float32, requires_grad=True)
    _, aux = orc.forward(p, batch, shape.num_attention_heads)
    ref = torch_pooled_loss(aux["cand"], aux["user"], dict(batch, browsed_ids=np.zeros((shape.batch_size, 1), np.int64)), logq=False)
    ref.backward()
    compare(loss, grads, float(ref.detach()), grads_of(p))
    with pytest.raises(KeyError, match="candidate_ids"):
        model.train_step(tbatch({k: v for k, v in batch.items() if k != "candidate_ids"}))


def test_nrms_v1_pooled_gradient():
    from oracle import nrms_oracle as orc
    from tests.test_hip_v1 import make_v1
    shape = V1_SHAPE
    params = synth.make_params_v1(shape, seed=71)
    batch = add_pool_keys(synth.make_batch(shape, seed=72, ragged=True, min_title=1, mask_some_candidates=True), shape.batch_size,
                          shape.history_len, shape.n_candidates, seed=7)
    loss, grads = pooled_step(make_v1(shape, params, V1_TITLE_HEADS), batch)
    v0 = orc.v1_to_v0_names(params)
    p = orc.to_torch(v0, torch.float32, requires_grad=True)
    _, aux = orc.forward(p, batch, shape.num_attention_heads, news_heads=V1_TITLE_HEADS, embed_dropout=False)
    ref = torch_pooled_loss(aux["cand"], aux["user"], batch)
    ref.backward()
    compare(loss, grads, float(ref.detach()), grads_of(p), names={v: k for k, v in zip(params.keys(), v0.keys())})


def test_nrms_naml_pooled_gradient():
    from oracle import naml_oracle as nml
    from oracle import nrms_oracle as orc
    from tests.test_hip_naml import make_model
    shape = synth.G7_ODD
    params = synth.make_params_naml(shape, seed=21)
    batch = add_pool_keys(synth.make_batch_naml(shape, seed=22), shape.batch_size, shape.history_len, shape.n_candidates, seed=8)
    loss, grads = pooled_step(make_model(shape, params), batch)
    p = orc.to_torch(params, torch.float32, requires_grad=True)
    _, parts = nml.forward(p, tbatch({k: v for k, v in batch.items() if k != "candidate_logq"}), shape.title_heads_num, shape.user_heads_num,
                           parts=True)
    ref = torch_pooled_loss(parts["cand"], parts["user"], batch)
    ref.backward()
    compare(loss, grads, float(ref.detach()), grads_of(p))


def test_nrms_bert_pooled_gradient():
    """The ids are the model's own: two slots with one id hold one vector, and a user's history is the reject list."""
    from tests.test_hip_nrms_bert import make_model, restate
    shape = synth.G9_SMALL
    params = synth.make_params_bert(shape, seed=31)
    batch = synth.make_batch_bert(shape, seed=32)
    batch["candidate_logq"] = np.log(np.random.default_rng(9).uniform(0.01, 0.5, size=batch["candidate_ids"].shape)).astype(np.float32)
    loss, grads = pooled_step(make_model(shape, params), batch)
    P = {k: torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for k, v in params.items()}
    B, H, Cn = shape.batch_size, shape.history_len, shape.n_candidates
    _, nv, user = restate(P, tbatch({k: v for k, v in batch.items() if k != "candidate_logq"}, "cuda"), shape.user_heads_num)
    ref = torch_pooled_loss(nv[B * H:].view(B, Cn, -1), user, batch)
    ref.backward()
    compare(loss, grads, float(ref.detach()), grads_of(P))


def test_rowwise_default_does_not_depend_on_the_new_config_field():
    """A row-wise train_step gives the same bits whether config.train_loss is "rowwise" or does not exist, and launches no pooled
    kernel."""
    from tests.test_hip_parity import make_model
    shape = V0_SHAPE
    params = synth.make_params(shape, seed=101)
    batch = add_pool_keys(synth.make_batch(shape, seed=102, ragged=True, min_title=1, mask_some_candidates=True), shape.batch_size,
                          shape.history_len, shape.n_candidates, seed=5, dead_row=False)
    outs = []
    for variant in ("field", "no_field"):
        model = make_model(shape, params).train()
        assert model.config.train_loss == "rowwise"
        if variant == "no_field":
            del model.config.train_loss, model.config.logq_correction
        eng = model.engine
        eng.timing(True)
        eng.timing_reset()
        loss = model.train_step(tbatch(batch), lr=1e-3)
        torch.cuda.synchronize()
        assert eng.timing_read("pooled_ce")[1] == 0 and eng.timing_read("ce_loss")[1] == 1 and eng.timing_read("click_bwd")[1] == 1
        eng.timing(False)
        outs.append((loss.cpu().numpy(), model._opt["g"].cpu().numpy(), model._flat.detach().cpu().numpy()))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    # and the pooled step launches the pooled kernels in place of ce_loss and click_bwd
    model = make_model(shape, params).train()
    model.config.train_loss = "pooled"
    eng = model.engine
    eng.timing(True)
    eng.timing_reset()
    model.train_step(tbatch(batch), lr=1e-3)
    torch.cuda.synchronize()
    assert eng.timing_read("pooled_ce")[1] >= 4 and eng.timing_read("ce_loss")[1] == 0 and eng.timing_read("click_bwd")[1] == 0
    eng.timing(False)
    eng.timing_reset()
    assert int(eng.pooled_pairs.cpu()[0]) > 0


def test_backward_without_a_pooled_loss_for_that_forward_is_refused():
    from tests.test_hip_parity import make_model
    shape = V0_SHAPE
    params = synth.make_params(shape, seed=101)
    batch = add_pool_keys(synth.make_batch(shape, seed=102, ragged=True, min_title=1), shape.batch_size, shape.history_len,
                          shape.n_candidates, seed=5)
    model = make_model(shape, params).train()
    eng = model.engine
    g = torch.zeros_like(model._flat)
    model.train_step(tbatch(batch), lr=1e-3)                                  # a row-wise step: a training forward, no pooled loss
    with pytest.raises(_lib.NrmsError, match="pooled_ce_loss"):
        eng.backward(model._flat, g, None)
    model.config.train_loss = "pooled"
    model.train_step(tbatch(batch), lr=1e-3)                                  # forward #2 with its pooled loss
    eng.backward(model._flat, g, None, gen=eng._saved["gen"])                 # allowed: the gradients of forward #2 are in place
    model.config.train_loss = "rowwise"
    model.train_step(tbatch(batch), lr=1e-3)                                  # forward #3 replaces the activations
    with pytest.raises(_lib.NrmsError, match="pooled_ce_loss"):
        eng.backward(model._flat, g, None)
    # loss only: nothing for a backward to use
    loss = eng.pooled_ce_loss(torch.from_numpy(batch["candidate_ids"]), want_grad=False)
    assert np.isfinite(float(loss))
    with pytest.raises(_lib.NrmsError, match="pooled_ce_loss"):
        eng.backward(model._flat, g, None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["hierec", "graph"])
def test_models_without_the_pooled_loss_say_so(name):
    shape = V0_SHAPE
    if name == "hierec":
        from tests.test_hip_hierec import N_SUB, N_TOP, make_hierec
        model = make_hierec(shape, synth.make_params_hierec(shape, N_SUB, N_TOP, seed=3))
        batch = synth.make_batch_hierec(shape, N_SUB, N_TOP, seed=4)
    else:
        from tests.test_hip_graph import make_graph
        model = make_graph(shape, synth.make_params_graph(shape, seed=3))
        batch = synth.make_batch_graph(shape, 8, seed=4)
    batch = dict(batch, candidate_ids=np.arange(1, shape.batch_size * shape.n_candidates + 1, dtype=np.int64).reshape(shape.batch_size, -1))
    model.config.train_loss = "pooled"
    with pytest.raises(NotImplementedError, match="pooled loss"):
        model.train().train_step(tbatch(batch))
    torch.cuda.synchronize()
    model.config.train_loss = "rowwise"                                       # and the model still trains
    assert np.isfinite(float(model.train_step(tbatch(batch))))


def test_fp16_pooled_steps_stay_finite():
    from tests.test_hip_parity import make_model
    shape = V0_SHAPE
    model = make_model(shape, synth.make_params(shape, seed=51), precision="fp16").train()
    model.config.train_loss = "pooled"
    losses = []
    for t in range(3):
        # (ids from 50 values: with the default handful a 7-slot history rejects the whole 9-column pool and the loss is 0)
        batch = add_pool_keys(synth.make_batch(shape, seed=52 + t, ragged=True, min_title=1), shape.batch_size, shape.history_len,
                              shape.n_candidates, seed=60 + t, n_ids=50)
        losses.append(float(model.train_step(tbatch(batch), lr=1e-3)) / shape.batch_size)
    eng = model.engine
    print("fp16 pooled losses", losses)
    assert np.isfinite(losses).all() and min(losses) > 0.0
    assert eng.poll_grad_overflow(block=True) == 0 and eng.grad_overflow_steps == 0
    assert bool(torch.isfinite(model._flat).all())


def test_run_v0_with_the_pooled_loss_is_reproducible(tmp_path, monkeypatch):
    from pytorch_news_recommender_amd import run_v0
    monkeypatch.chdir(tmp_path)
    runs = []
    for r in range(2):
        hist = run_v0.main(["--model", "nrms_hip", "--dataset", "synthetic", "--negatives", "catalogue", "--loss", "pooled", "--max_batches", "3",
                            "--epochs", "1", "--synthetic_users", "260", "--num_workers", "0", "--description", "T",
                            "--data_path", str(tmp_path / "data_processed"), "--save_path", str(tmp_path / ("save%d" % r))])
        runs.append(hist["losses"])
    print("pooled run_v0 losses", runs[0])
    assert len(runs[0]) == 3 and np.isfinite(runs[0]).all()
    assert runs[0] == runs[1]
