"""The fp16 news encoder's forward builds the context of an all-padding title once -- b_v under the title's own dropout mask --
keeps its 20 fragments in registers through the additive stage and the pooling, and writes the ctx16 block the backward reads
afterwards (csrc/fused16.hip, fwd16p_closed).  These tests stress that class: batches in which whole users, every history or
no title at all is padding, with 30-word titles and shorter ones, with and without dropout, the training step and the inference
forward, against oracle/nrms_oracle.py with the kernels' own keep masks and the bars of tests/test_hip_fp16.py.  The
gradients the all-padding titles feed through their stored context (d(W_add), d(b_add), d(q_vec), d(b_v)) are checked one by
one, runs are compared bit for bit, and one case runs with the helper streams off."""
import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import synth

CASES = ["pad_users", "no_all_pad", "pad_histories", "pad_users_short_titles"]
P_DROP = [0.2, 0.0]
NEWS = "news_encoder."
FED_BY_PADDING = [NEWS + "additive_attention.linear.weight", NEWS + "additive_attention.linear.bias",
                  NEWS + "additive_attention.attention_query_vector", NEWS + "multihead_self_attention.W_V.bias"]


def make_case(case):
    """(shape, batch, MIND-shaped).  Titles are ragged from one word on; a padding history slot is an all-padding title.
    pad_users: users 0 and 3 have nothing but padding in their histories (plus the usual empty tails of the others);
    no_all_pad: full histories, no title without a word; pad_histories: EVERY history title is padding, the candidates live;
    pad_users_short_titles: pad_users with 17-word titles and 6 heads of 20 (heads the 10-head layout does not have)."""
    if case == "pad_users_short_titles":
        shape = synth.Shape(n_words=300, word_embed_size=120, num_attention_heads=6, query_vector_dim=64, batch_size=7,
                            history_len=20, n_candidates=4, n_words_title=17)
    else:
        shape = synth.Shape(n_words=1000, word_embed_size=300, num_attention_heads=10, query_vector_dim=200, batch_size=7,
                            history_len=20, n_candidates=5, n_words_title=30)
    batch = synth.make_batch(shape, seed=202, ragged=case != "no_all_pad", min_title=1, mask_some_candidates=True)
    if case == "no_all_pad":
        # full histories; ragged titles by hand (make_batch's ragged also shortens the histories)
        rng = np.random.default_rng(203)
        for key in ("browsed_titles", "candidate_titles"):
            t = batch[key]
            n = rng.integers(1, shape.n_words_title + 1, size=t.shape[:2])
            t[np.arange(shape.n_words_title)[None, None, :] >= n[..., None]] = 0
    elif case == "pad_histories":
        batch["browsed_titles"][:] = 0
    else:
        batch["browsed_titles"][0] = 0
        batch["browsed_titles"][3] = 0
    return shape, batch, case != "pad_users_short_titles"


def all_padding_fraction(batch):
    t = np.concatenate([batch["browsed_titles"].reshape(-1, batch["browsed_titles"].shape[-1]),
                        batch["candidate_titles"].reshape(-1, batch["candidate_titles"].shape[-1])])
    return float((t == 0).all(axis=1).mean())


@pytest.mark.parametrize("case", CASES)
def test_case_generator(case):
    """CPU: the batches are what their names say (the GPU tests below are only as good as these)."""
    shape, batch, _ = make_case(case)
    bt, ct = batch["browsed_titles"], batch["candidate_titles"]
    assert bt.shape == (shape.batch_size, shape.history_len, shape.n_words_title) and bt.dtype == np.int64
    assert (ct != 0).any(axis=-1).all(), "every candidate has a word"
    frac = all_padding_fraction(batch)
    hist_pad = (bt == 0).all(axis=-1)
    if case == "no_all_pad":
        assert frac == 0.0
    elif case == "pad_histories":
        assert hist_pad.all() and frac == shape.history_len / (shape.history_len + shape.n_candidates)
    else:
        assert hist_pad[0].all() and hist_pad[3].all() and not hist_pad[1].all()
        assert 0.3 < frac < 0.8
    # long, short (a prefix of at most 15 words) and all-padding titles all occur, except where the case excludes a class
    n_words = (np.concatenate([bt.reshape(-1, bt.shape[-1]), ct.reshape(-1, ct.shape[-1])]) != 0).sum(axis=1)
    assert (n_words > 15).any() and ((n_words > 0) & (n_words <= 15)).any()


def _keep_masks(model, shape, seed, p_drop):
    from tests.test_hip_fp16 import _padded_to_model_cols
    n_titles = shape.batch_size * (shape.history_len + shape.n_candidates)
    L, d, h = shape.n_words_title, shape.word_embed_size, shape.num_attention_heads
    ke = model.engine.dropout_keep_mask(seed, 0, n_titles * L, p_drop).cpu().view(n_titles, L, d)
    kc = model.engine.dropout_keep_mask(seed, 1, n_titles * L, p_drop, fp16_ctx=True).cpu().numpy()
    return {"embed": ke, "ctx": torch.from_numpy(_padded_to_model_cols(kc, h, d // h)).view(n_titles, L, d)}


@pytest.mark.gpu
@pytest.mark.parametrize("p_drop", P_DROP)
@pytest.mark.parametrize("case", CASES)
def test_allpad_train_step_and_inference_against_oracle(case, p_drop):
    from oracle import nrms_oracle as orc
    from tests.test_hip_fp16 import GRAD_ABS, VEC_TOL, _grad_report, score_bar, score_terms
    from tests.test_hip_parity import fwd_bwd, make_model, tbatch
    shape, batch, mind_shaped = make_case(case)
    params = synth.make_params(shape, seed=201)
    model = make_model(shape, params, dropout=p_drop, precision="fp16").train()
    scores, loss, grads = fwd_bwd(model, batch)
    assert model.engine.pad_row_zero is True
    keep = _keep_masks(model, shape, model.engine._saved["seed"], p_drop) if p_drop > 0 else None
    o_scores, o_loss, o_grads, aux = orc.loss_and_grads(params, batch, shape.num_attention_heads, p_drop=p_drop, keep=keep)
    valid = batch["candidate_mask"] == 1
    err = float(np.abs(scores - o_scores)[valid].max())
    print("allpad %s p=%.1f train: max |score - oracle| = %.3e, |loss diff| %.2e, all-padding titles %.0f %%"
          % (case, p_drop, err, abs(loss - o_loss), 100 * all_padding_fraction(batch)))
    terms = None if mind_shaped else score_terms(aux, valid)
    assert err < score_bar(o_scores[valid], False, terms), (err, terms)
    # the gradients the all-padding titles feed, one by one, then the rest
    _grad_report(grads, o_grads, FED_BY_PADDING, case + " fed", abs_floor=GRAD_ABS)
    _grad_report(grads, o_grads, [n for n in synth.param_names() if n not in FED_BY_PADDING], case, abs_floor=GRAD_ABS)
    assert not grads["news_encoder.word_embedding.0.weight"][0].any()

    # inference forward (no dropout, TRAIN = false kernels): scores and the news vectors of the histories
    model = model.eval()
    model.dedup_inference = False
    B, H, L = batch["browsed_titles"].shape
    with torch.no_grad():
        s = model(tbatch(batch)).cpu().numpy()
        nv = model.get_news_vector(torch.from_numpy(batch["browsed_titles"]).reshape(B * H, L)).view(B, H, -1).cpu().numpy()
        o_s, o_aux = orc.forward(orc.to_torch(params), batch, shape.num_attention_heads)
    o_s = o_s.numpy()
    ierr = float(np.abs(s - o_s)[valid].max())
    verr = float(np.abs(nv - o_aux["hist"].numpy()).max())
    print("allpad %s inference: max |score - oracle| = %.3e, max |news vector - oracle| = %.3e" % (case, ierr, verr))
    assert ierr < score_bar(o_s[valid], False, None if mind_shaped else score_terms(o_aux, valid))
    assert verr < VEC_TOL
    assert (s[~valid] == np.float32(-1e9)).all()


def _engine_step(model, tb, shape, p_drop, seed):
    eng, flat = model.engine, model._flat
    sc = eng.forward(flat, tb["browsed_titles"], tb["candidate_titles"], tb["candidate_mask"], training=True, p_drop=p_drop, seed=seed)
    _, dsc = eng.ce_loss(sc, grad_scale=1.0 / shape.batch_size)
    g = torch.zeros_like(flat)
    eng.backward(flat, g, dsc)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), g.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("p_drop", P_DROP)
def test_allpad_step_is_bit_identical_run_to_run_and_without_helper_streams(p_drop, monkeypatch):
    """Same seed, same batch: scores and the whole flat gradient agree bit for bit between two runs and with the helper
    streams off (the d(W_add) product then runs behind the attention backward instead of beside it)."""
    from tests.test_hip_parity import make_model, tbatch
    shape, batch, _ = make_case("pad_users")
    params = synth.make_params(shape, seed=201)
    tb = {k: v.cuda() for k, v in tbatch(batch).items()}
    res = []
    for no_side in (False, False, True):
        if no_side:
            monkeypatch.setenv("NRMS_NO_SIDE_STREAMS", "1")
        else:
            monkeypatch.delenv("NRMS_NO_SIDE_STREAMS", raising=False)
        model = make_model(shape, params, dropout=p_drop, precision="fp16").train()
        res.append(_engine_step(model, tb, shape, p_drop, seed=0x51DE5))
    assert np.isfinite(res[0][1]).all() and res[0][1].any()
    for sc, g in res[1:]:
        assert np.array_equal(res[0][0], sc)
        assert np.array_equal(res[0][1], g)
