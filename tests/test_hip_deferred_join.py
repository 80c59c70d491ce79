"""The user encoder's weight-gradient GEMMs left on their helper stream past the end of nrms_encoder_bwd
(NRMS_FLAG_DEFER_USER_JOIN, include/nrms_hip.h: Engine.backward sets it in front of the fp16 news backward, which joins them at
its end), and the column split of the split-bf16 NT GEMM at few rows (csrc/gemm_bf16.hip launch_bf_mode, NRMS_NT_WIDE_TILES forces
the wide tile).  Neither changes the order of any sum: every comparison here is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, synth
from tests.test_hip_parity import make_model, tbatch

gpu = pytest.mark.gpu
D, HEADS, Q = 300, 10, 200          # the tests/test_hip_user64.py geometry


def test_flag_is_known_and_the_next_bit_is_not():
    lib = _lib.load()
    base = dict(n_seq=3, seq_len=50, d_model=D, n_heads=HEADS, q_dim=Q, vocab=0, p_drop_embed=0.0, p_drop_ctx=0.0,
                precision=_lib.NRMS_PRECISION_BF16X3, use_output_proj=0, mask_mode=0, seed=0, loss_scale=0.0, p_drop_attn=0.0)
    plain = lib.nrms_encoder_bwd_workspace_bytes(C.byref(_lib.EncoderDesc(flags=0, **base)))
    assert plain > 0
    assert lib.nrms_encoder_bwd_workspace_bytes(C.byref(_lib.EncoderDesc(flags=_lib.NRMS_FLAG_DEFER_USER_JOIN, **base))) == plain
    assert lib.nrms_encoder_bwd_workspace_bytes(C.byref(_lib.EncoderDesc(flags=32, **base))) == 0
    assert b"flags" in lib.nrms_last_error()
    assert lib.nrms_encoder_join(None) == 0          # nothing outstanding (and no device needed to say so)


def _user_setup(B, H):
    shape = synth.Shape(n_words=50, word_embed_size=D, num_attention_heads=HEADS, query_vector_dim=Q, batch_size=B,
                        history_len=H, n_candidates=2, n_words_title=4)
    params = synth.make_params(shape, seed=17)
    g = torch.Generator().manual_seed(18)
    x = torch.randn(B, H, D, generator=g) * 0.3
    dout = torch.randn(B, D, generator=g) * 1e-2
    model = make_model(shape, params, precision="bf16x3")
    return model, x.cuda(), dout.cuda()


def _user_bwd(model, xd, dd, fused, defer=False, poison=False):
    """forward + backward of the user encoder alone; poison: NaN over the workspace the NEXT backward of a train step would use
    (Engine's shared "bwd_ws"), before the call and again between the deferred call's return and the join."""
    eng, flat = model.engine, model._flat
    eng.fused_user_encoder = fused
    B, H, d = xd.shape
    desc = eng._desc("user_encoder", B, H, training=True)
    assert bool(desc.flags & _lib.NRMS_FLAG_FUSED_SEQ64) is fused
    out = eng.encode_users(flat, xd, save=True, tag="dj").clone()
    gf = torch.zeros_like(flat)
    dx = torch.empty(B * H, d, dtype=torch.float32, device=xd.device)
    shared = eng._bwd_workspace(desc)
    if poison:
        shared.fill_(float("nan"))
    eng.encode_users_backward(flat, gf, xd, dd, dx=dx, tag="dj", defer_join=defer)
    if poison:
        shared.fill_(float("nan"))
    if defer:
        eng.join_backward()
    torch.cuda.synchronize()
    grads = {n: model._layout.view(gf, n).cpu().numpy().copy() for n in model._layout.names if n.startswith("user_encoder.")}
    return out.cpu().numpy(), dx.cpu().numpy(), grads


def _assert_same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "out")
    assert np.array_equal(a[1], b[1]), (what, "dx")
    assert sorted(a[2]) == sorted(b[2]) and len(a[2]) >= 6
    for n in a[2]:
        assert np.isfinite(a[2][n]).all(), (what, n)
        assert np.array_equal(a[2][n], b[2][n]), (what, n)


@gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("H", [33, 50, 64])
@pytest.mark.parametrize("B", [3, 5])
def test_deferred_user_join_gradients_and_workspace_isolation(B, H, fused):
    """With and without the flag: dx and every user-encoder gradient equal (the odd user counts leave a half-filled workgroup in
    the fused kernels).  Then with NaN over the shared workspace between the deferred call and its join: a deferred GEMM that
    still read the shared buffer -- where the news backward writes from offset 0 -- would show it."""
    model, xd, dd = _user_setup(B, H)
    joined = _user_bwd(model, xd, dd, fused)
    assert np.abs(joined[1]).max() > 0 and all(np.abs(g).max() > 0 for n, g in joined[2].items() if not n.endswith("W_K.bias"))
    _assert_same(joined, _user_bwd(model, xd, dd, fused, defer=True), "deferred")
    _assert_same(joined, _user_bwd(model, xd, dd, fused, defer=True, poison=True), "deferred, shared workspace poisoned")
    _assert_same(joined, _user_bwd(model, xd, dd, fused), "joined again")


@gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B,H", [(1, 33), (5, 50), (6, 50), (10, 52)])
def test_nt_column_split_does_not_change_a_bit(B, H, fused, monkeypatch):
    """M = 33, 250, 300, 520 rows (the last two end in a partial row tile): at so few rows launch_bf_mode splits the 300 columns
    of the dX GEMM into two blocks of 10 tiles -- the second one partial, 140 of 160 columns -- instead of one of 19;
    NRMS_NT_WIDE_TILES forces the wide tile.  The unfused chain sends its other projections through the same choice."""
    model, xd, dd = _user_setup(B, H)
    monkeypatch.delenv("NRMS_NT_WIDE_TILES", raising=False)
    split = _user_bwd(model, xd, dd, fused)
    monkeypatch.setenv("NRMS_NT_WIDE_TILES", "1")
    wide = _user_bwd(model, xd, dd, fused)
    monkeypatch.delenv("NRMS_NT_WIDE_TILES", raising=False)
    assert np.abs(split[1]).max() > 0
    _assert_same(wide, split, "column split")


STEP_SHAPE = synth.Shape(n_words=600, word_embed_size=D, num_attention_heads=HEADS, query_vector_dim=Q, batch_size=4,
                         history_len=50, n_candidates=5, n_words_title=30)


def _three_steps(autograd):
    torch.manual_seed(1234)                                   # (the dropout seeds derive from it)
    model = make_model(STEP_SHAPE, synth.make_params(STEP_SHAPE, seed=43), dropout=0.2, precision="fp16").train()
    losses = []
    opt = None
    if autograd:
        model.reuse_grad_buffer = True
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for step in range(3):
        batch = tbatch(synth.make_batch(STEP_SHAPE, seed=50 + step, ragged=True, min_title=1))
        if autograd:
            opt.zero_grad(set_to_none=True)
            scores = model(batch)
            loss = torch.nn.functional.cross_entropy(scores, torch.zeros(len(scores), dtype=torch.long, device=scores.device))
            loss.backward()
            opt.step()
            losses.append(loss.detach().cpu().numpy().copy())
        else:
            losses.append(model.train_step(batch).cpu().numpy().copy())
    torch.cuda.synchronize()
    eng = model.engine
    assert eng._desc("user_encoder", 4, 50, training=True).flags & _lib.NRMS_FLAG_FUSED_SEQ64
    params = {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters()}
    return losses, params


@gpu
@pytest.mark.parametrize("autograd", [False, True], ids=["train_step", "autograd"])
def test_three_steps_are_the_same_with_and_without_helper_streams(autograd, monkeypatch):
    """Three consecutive fp16 steps (4 users, 50 x 30 histories, dropout 0.2): the loss of every step and every parameter after
    the third, default against NRMS_NO_SIDE_STREAMS against default again.  A join that leaked into the next step -- Adam or the
    next step's zeroing overtaking a weight-gradient GEMM -- shows from step 2 on.  Once through Model.train_step, once through
    autograd + torch.optim.Adam (reuse_grad_buffer), which shares Engine.backward."""
    runs = []
    for no_side in (False, True, False):
        if no_side:
            monkeypatch.setenv("NRMS_NO_SIDE_STREAMS", "1")
        else:
            monkeypatch.delenv("NRMS_NO_SIDE_STREAMS", raising=False)
        runs.append(_three_steps(autograd))
    monkeypatch.delenv("NRMS_NO_SIDE_STREAMS", raising=False)
    assert all(np.isfinite(l).all() for l in runs[0][0])
    moved = max(float(np.abs(runs[0][1][n] - v).max())
                for n, v in synth.make_params(STEP_SHAPE, seed=43).items() if n.startswith("user_encoder."))
    assert moved > 0                                          # (the user encoder did train)
    for other, what in ((runs[1], "NRMS_NO_SIDE_STREAMS"), (runs[2], "default, repeated")):
        for step in range(3):
            assert np.array_equal(runs[0][0][step], other[0][step]), (what, "loss of step %d" % (step + 1))
        for n in runs[0][1]:
            assert np.array_equal(runs[0][1][n], other[1][n]), (what, n)
