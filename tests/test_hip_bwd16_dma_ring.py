"""The fp16 attention backward on the LDS-DMA tile ring (csrc/fused16_bwd.hip, fused_bwd16_attn_kernel<1, true>) against the
register-staged ring it replaced (NRMS_BWD_ATTN_STAGED=1, read per call): the two kernels issue the same MFMAs on the same
operands and add in the same order, so every gradient of the engine's backward must be the same bits -- at the title mixes
where the ring's bookkeeping can go wrong (idle waves, partial groups, unpaired short titles, no group at all, a workgroup
that walks several groups of different classes, 6 and 30 tiles per group, a ring restarted by the next launch)."""
import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import synth
from tests.test_hip_parity import make_model

pytestmark = pytest.mark.gpu

SWITCH = "NRMS_BWD_ATTN_STAGED"
H10 = dict(word_embed_size=300, num_attention_heads=10, query_vector_dim=200)      # 30 head tiles per group (the benchmarked geometry)
H2 = dict(word_embed_size=60, num_attention_heads=2, query_vector_dim=32)          # 6 head tiles per group
N_CAND = 2

# real words per title, in title order (history slots first, then the candidates); 0 = an all-padding title, 1 .. 15 = a short
# title (two share a tile), 16 .. = a long one; a negative length -n = n words with a padding token in the middle (long class)
ONE_TITLE = [20, 0, 0, 0]
FIVE_LONG = [30, 16, 25, 0, 18, 22]
THREE_SHORT = [3, 15, 0, 1]
MIX = [30, 4, 0, 9, -20, 1, 0, 15, 16, 0, 7, 2, 0, 12, 27, 0, 5, 0, 3]              # 4 long, 9 short, 6 all-padding
ALL_PAD = [0, 0, 0, 0]
SHORT_S7 = [7, 3, 1, 0, 5, 7, 2, 6, 4]                                              # S = 7: full and short, an unpaired one


def _many_groups():
    """More groups than the kernel's 512 workgroups: 800 short titles (100 pair groups), 2 000 long ones (500 groups) and 60
    all-padding ones -- workgroups 0 .. 87 walk a pair group and then a group of long titles on one running ring."""
    rng = np.random.default_rng(5)
    lens = np.concatenate([rng.integers(1, 16, size=800), rng.integers(16, 31, size=2000), np.zeros(60, dtype=np.int64)])
    return [int(x) for x in rng.permutation(lens)]


def _titles(lengths, S, n_words, rng):
    ids = np.zeros((len(lengths), S), dtype=np.int64)
    for i, n in enumerate(lengths):
        ids[i, :abs(n)] = rng.integers(1, n_words, size=abs(n))
        if n < 0:
            ids[i, abs(n) // 2] = 0
    return ids


def _setup(lengths, S, geom, users=1):
    assert len(lengths) % users == 0 and len(lengths) // users > N_CAND
    per_user = len(lengths) // users
    shape = synth.Shape(n_words=400, batch_size=users, history_len=per_user - N_CAND, n_candidates=N_CAND, n_words_title=S, **geom)
    params = synth.make_params(shape, seed=31)
    ids = _titles(lengths, S, shape.n_words, np.random.default_rng(32)).reshape(users, per_user, S)
    hist = torch.from_numpy(np.ascontiguousarray(ids[:, :per_user - N_CAND])).cuda()
    cand = torch.from_numpy(np.ascontiguousarray(ids[:, per_user - N_CAND:])).cuda()
    return shape, params, hist, cand


def _backward(model, hist, cand, p_drop, seed, staged, monkeypatch):
    """One training forward + backward of the engine on given title ids, with an upstream gradient that does not sum to zero
    over a user's candidates (equal all-padding candidates still send a gradient into the history) -> the flat gradient."""
    if staged:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    model._prepare()
    eng, flat = model._engine, model._flat
    scores = eng.forward(flat, hist, cand, None, training=True, p_drop=p_drop, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    dscores = (torch.rand(tuple(scores.shape), generator=g) - 0.3).to(scores.device)
    gflat = torch.zeros_like(flat)
    eng.backward(flat, gflat, dscores)
    torch.cuda.synchronize()
    monkeypatch.delenv(SWITCH, raising=False)
    return gflat.cpu()


def _assert_same(model, got, want, live):
    lay = model._layout
    for name in lay.names:
        a, b = lay.view(got, name).numpy(), lay.view(want, name).numpy()
        assert np.array_equal(a, b), (name, float(np.abs(a - b).max()))
    assert np.array_equal(got.numpy(), want.numpy())
    assert np.isfinite(got.numpy()).all()
    table = lay.view(got, lay.names[0]).numpy()
    assert not table[0].any()
    if live:                                        # not vacuous: the attention backward produced a table gradient
        assert np.abs(table).max() > 0


CASES = {
    "one_title": (ONE_TITLE, 30, H10, 1),
    "five_long": (FIVE_LONG, 30, H10, 1),
    "three_short": (THREE_SHORT, 30, H10, 1),
    "mix": (MIX, 30, H10, 1),
    "all_padding": (ALL_PAD, 30, H10, 1),
    "mix_h2": (MIX, 30, H2, 1),
    "short_s7": (SHORT_S7, 7, H10, 1),
    "short_s7_h2": (SHORT_S7, 7, H2, 1),
}


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("case", list(CASES))
def test_dma_ring_gradients_equal_the_staged_ring(case, p_drop, monkeypatch):
    lengths, S, geom, users = CASES[case]
    shape, params, hist, cand = _setup(lengths, S, geom, users)
    model = make_model(shape, params, dropout=p_drop, precision="fp16").train()
    dma = _backward(model, hist, cand, p_drop, 11, False, monkeypatch)
    staged = _backward(model, hist, cand, p_drop, 11, True, monkeypatch)
    _assert_same(model, dma, staged, live=any(lengths))


def test_dma_ring_runs_through_the_groups_of_a_workgroup(monkeypatch):
    lengths = _many_groups()
    shape, params, hist, cand = _setup(lengths, 30, H10, users=52)
    model = make_model(shape, params, dropout=0.2, precision="fp16").train()
    dma = _backward(model, hist, cand, 0.2, 13, False, monkeypatch)
    staged = _backward(model, hist, cand, 0.2, 13, True, monkeypatch)
    _assert_same(model, dma, staged, live=True)


def test_dma_ring_restarts_between_launches(monkeypatch):
    """Two consecutive backward calls on one engine, on different title mixes: the second launch starts its ring from tile 0
    whatever the first one left in LDS, and equals the staged kernel's second call."""
    shape, params, hist, cand = _setup(MIX, 30, H10)
    _, _, hist2, cand2 = _setup(MIX[::-1], 30, H10)
    out = {}
    for staged in (False, True):
        model = make_model(shape, params, dropout=0.2, precision="fp16").train()
        first = _backward(model, hist, cand, 0.2, 17, staged, monkeypatch)
        second = _backward(model, hist2, cand2, 0.2, 19, staged, monkeypatch)
        out[staged] = (model, first, second)
    _assert_same(out[False][0], out[False][1], out[True][1], live=True)
    _assert_same(out[False][0], out[False][2], out[True][2], live=True)
    assert not np.array_equal(out[False][1].numpy(), out[False][2].numpy())


def test_dma_ring_gradients_against_the_float64_oracle():
    """The default path (DMA ring) at the benchmarked geometry against the float64 oracle, at the bars of tests/test_hip_fp16.py."""
    from oracle import nrms_oracle as orc
    from tests.test_hip_fp16 import _grad_report, score_bar
    from tests.test_hip_parity import fwd_bwd
    shape = synth.Shape(n_words=1000, batch_size=5, history_len=9, n_candidates=4, n_words_title=30, **H10)
    params = synth.make_params(shape, seed=41)
    batch = synth.make_batch(shape, seed=42, ragged=True, min_title=1, empty_history_user=True, all_pad_title=True)
    model = make_model(shape, params, precision="fp16").train()
    scores, loss, grads = fwd_bwd(model, batch)
    o_scores, o_loss, o_grads, _ = orc.loss_and_grads(params, batch, shape.num_attention_heads)
    err = float(np.abs(scores - o_scores).max())
    print("dma ring: max |score - oracle| = %.3e, |loss diff| %.2e" % (err, abs(loss - o_loss)))
    assert err < score_bar(o_scores)
    _grad_report(grads, o_grads, synth.param_names(), "dma ring")
    assert not grads["news_encoder.word_embedding.0.weight"][0].any()
