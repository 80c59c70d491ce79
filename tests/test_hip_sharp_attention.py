"""The NRMS encoders where a trained model is: attention that is PEAKED, not the near-uniform softmax of the initial weights
every other encoder test runs at (news self-attention logit std 0.08, user 0.004: exp(x) ~ 1 + x, attention = mean pooling).

Weights come from tests/sharp_ref.sharpen (self-attention logit std 1.6 `warm` / 2.75 `peaked`: at `peaked` 5 % of the rows put
more than 0.99 on one key, logits span 54, probabilities go down to 1e-24).  Everything is compared with the FLOAT64 oracle
under sharp_ref.bar = max(the suite's existing bar for the mode and quantity, 8 x the error of a float64 emulation of the mode's
operand roundings) -- conditions on that bar (wrong models are far outside it) are checked on the CPU by
tests/test_sharp_ref_host.py.  Every check prints: GPU error, emulated error, bar, existing bar."""
import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, synth
from tests import sharp_ref as sr
from tests.test_hip_parity import fwd_bwd, make_model, tbatch

pytestmark = pytest.mark.gpu

LEVELS = ["warm", "peaked"]
TRAIN = [(c, m) for c in sr.CASES for m in sr.modes_of(c)]
INFER = [(c, m) for c in ("mind_small", "hist50") for m in sr.MODES]
TABLE = "news_encoder.word_embedding.0.weight"


class Report:
    """Collects every comparison of a test, prints them all, then fails on the worst: a failing run still shows every figure."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def check(self, what, kind, mode, got, exact, emu, name="", refs=None, times=1.0):
        got, exact, emu = (np.asarray(a, dtype=np.float64) for a in (got, exact, emu))
        bound = sr.bar(kind, mode, exact, emu, name, refs) * times
        old = sr.existing_bar(kind, mode, exact, name, refs) * times
        err = float(np.abs(got - exact).max()) if got.size else 0.0
        emu_err = float(np.abs(emu - exact).max()) if got.size else 0.0
        ratio = sr.excess(got, exact, bound)
        print("sharp %-34s %-46s gpu %.2e  emulated %.2e  bar %.2e  existing %.2e  (scale %.2e)  gpu/bar %.2f" % (
            self.tag, what, err, emu_err, float(np.max(bound)), float(np.max(old)), float(np.abs(exact).max()) if got.size else 0.0, ratio))
        if not ratio <= 1.0:
            self.bad.append((what, err, float(np.max(bound)), ratio))

    def done(self):
        assert not self.bad, "%s: outside the bar: %s" % (self.tag, self.bad)


def _model_for(case, level, mode, dropout=0.0):
    shape, params, batch = sr.sharp_case(case, level)
    base, user16 = mode.split("+")[0], mode.endswith("+user16")
    return shape, params, batch, make_model(shape, params, dropout=dropout, precision=base, fp16_user=user16)


def _check_step(rep, mode, batch, scores, loss, grads, ex, em):
    valid = batch["candidate_mask"] == 1
    assert (scores[~valid] == np.float32(-1e9)).all()
    rep.check("scores", "score", mode, scores[valid], ex["scores"][valid], em["scores"][valid])
    rep.check("loss", "loss", mode, loss, ex["loss"], em["loss"])
    for n in synth.param_names():
        rep.check(n, "grad", mode, grads[n], ex["grads"][n], em["grads"][n], n, ex["grads"])
    assert not grads[TABLE][0].any()                                   # padding_idx = 0: exactly zero


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case,mode", TRAIN)
def test_training_forward_backward(case, mode, level):
    shape, params, batch, model = _model_for(case, level, mode)
    scores, loss, grads = fwd_bwd(model.train(), batch)
    assert model.engine.pad_row_zero is True
    rep = Report("train %s %s %s" % (case, mode, level))
    _check_step(rep, mode, batch, scores, loss, grads, sr.exact_case(case, level), sr.emulated_case(case, level, mode))
    rep.done()


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case,mode", INFER)
def test_inference_instantiations(case, mode, level):
    """The kernels' inference instantiations (no saved activations): eval forward with and without title deduplication,
    get_news_vector, get_user_vector on the model's own news vectors; fp16 modes with fp16_inference on."""
    shape, params, batch, model = _model_for(case, level, mode)
    ex, em = sr.exact_case(case, level), sr.emulated_case(case, level, mode)
    model.eval()
    valid = batch["candidate_mask"] == 1
    B, H, L = batch["browsed_titles"].shape
    rep = Report("infer %s %s %s" % (case, mode, level))
    with torch.no_grad():
        for dedup in (True, False):
            model.dedup_inference = dedup
            s = model(tbatch(batch)).cpu().numpy()
            assert (s[~valid] == np.float32(-1e9)).all()
            rep.check("scores dedup=%s" % dedup, "score", mode, s[valid], ex["scores"][valid], em["scores"][valid])
        hist = model.get_news_vector(torch.from_numpy(batch["browsed_titles"]).reshape(B * H, L)).view(B, H, -1)
        user = model.get_user_vector(hist)
    rep.check("news vectors", "vec", mode, hist.cpu().numpy(), ex["hist"], em["hist"])
    rep.check("user vectors", "vec", mode, user.cpu().numpy(), ex["user"], em["user"])
    rep.done()


# ---- the fused user encoder called directly (csrc/user64.hip), as tests/test_hip_user64.py does -------------------------
def _user_hip(model, x, dout, fused):
    eng, flat = model.engine, model._flat
    eng.fused_user_encoder = fused
    desc = eng._desc("user_encoder", x.shape[0], x.shape[1], training=True)
    assert bool(desc.flags & _lib.NRMS_FLAG_FUSED_SEQ64) is fused
    xd, dd = x.cuda(), dout.cuda()
    out = eng.encode_users(flat, xd, save=True, tag="s64").clone()
    inf = eng.encode_users(flat, xd, tag="s64i").clone()
    gf = torch.zeros_like(flat)
    dx = eng.encode_users_backward(flat, gf, xd, dd, tag="s64").clone()
    torch.cuda.synchronize()
    grads = {n: model._layout.view(gf, n).cpu().numpy().copy() for n in model._layout.names if n.startswith("user_encoder.")}
    return out.cpu().numpy(), inf.cpu().numpy(), dx.cpu().numpy(), grads


def _histories(level, rows):
    """Sharpened news vectors of `hist50` as click histories of 50, 33 or 64 rows (64: a user's 50 followed by the first 14
    of the next user's)."""
    hist = sr.exact_case("hist50", level)["hist"].astype(np.float32)            # [4, 50, 300]
    if rows <= 50:
        return np.ascontiguousarray(hist[:, :rows])
    return np.ascontiguousarray(np.concatenate([hist, np.roll(hist, -1, axis=0)[:, :rows - 50]], axis=1))


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("rows", [50, 33, 64])
def test_fused_user_encoder_directly(rows, level):
    shape, params, _ = sr.sharp_case("hist50", level)
    h = shape.num_attention_heads
    x = _histories(level, rows)
    params = sr.sharpen_user(sr.case_inputs("hist50")[1], x, h, level)          # calibrated on these very rows
    g = torch.Generator().manual_seed(18)
    dout = (torch.randn(x.shape[0], x.shape[2], generator=g) * 1e-2).numpy()
    ex = sr.user_alone(params, x, dout, h, "exact")
    model = make_model(shape, params, precision="bf16x3")
    scale = max(1.0, float(np.abs(ex["out"]).max()))
    for fused, kind in ((True, "bf16x3_fused"), (False, "bf16x3")):
        em = sr.user_alone(params, x, dout, h, kind)
        out, inf, dx, grads = _user_hip(model, torch.from_numpy(x), torch.from_numpy(dout), fused)
        rep = Report("user %d rows %s %s" % (rows, "fused" if fused else "chain", level))
        rep.check("out", "score", "bf16x3", out, ex["out"], em["out"], times=scale)        # (test_hip_user64: x max(1, scale))
        rep.check("dX", "grad", "bf16x3", dx, ex["dx"], em["dx"])
        for n in grads:
            rep.check(n, "grad", "bf16x3", grads[n], ex["grads"][n], em["grads"][n], n, ex["grads"])
        assert float(np.abs(inf - out).max()) <= 2e-7 * scale                    # the inference instantiation: same arithmetic
        rep.done()


# ---- dropout: the kernels' own keep masks replayed through the oracle -----------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_dropout_replayed_at_warm(mode):
    from tests.test_hip_fp16 import _padded_to_model_cols
    case, level, p_drop = "mind_small", "warm", 0.2
    shape, params, batch, model = _model_for(case, level, mode, dropout=p_drop)
    scores, loss, grads = fwd_bwd(model.train(), batch)
    sv = model.engine._saved
    n_titles = shape.batch_size * (shape.history_len + shape.n_candidates)
    L, d, h = shape.n_words_title, shape.word_embed_size, shape.num_attention_heads
    ke = model.engine.dropout_keep_mask(sv["seed"], 0, n_titles * L, p_drop).cpu().view(n_titles, L, d)
    if mode == "fp16":
        kc = model.engine.dropout_keep_mask(sv["seed"], 1, n_titles * L, p_drop, fp16_ctx=True).cpu().numpy()
        kc = torch.from_numpy(_padded_to_model_cols(kc, h, d // h)).view(n_titles, L, d)
    else:
        kc = model.engine.dropout_keep_mask(sv["seed"], 1, n_titles * L, p_drop).cpu().view(n_titles, L, d)
    assert 0.77 < float(ke.float().mean()) < 0.83 and 0.77 < float(kc.float().mean()) < 0.83
    keep = {"embed": ke, "ctx": kc}
    ex = sr.exact(params, batch, h, p_drop=p_drop, keep=keep)
    em = sr.emulated(params, batch, h, mode, p_drop=p_drop, keep=keep)
    rep = Report("dropout %s" % mode)
    _check_step(rep, mode, batch, scores, loss, grads, ex, em)
    rep.done()


# ---- nrms_v1: W_O, six title heads of 50, pair mask, masked additive pooling (fp32 / bf16x3) ------------------------------
V1_SHAPE = synth.Shape(n_words=500, word_embed_size=300, num_attention_heads=10, query_vector_dim=200,
                       batch_size=3, history_len=50, n_candidates=3, n_words_title=30)
V1_TITLE_HEADS = 6
_v1_cache = {}


def _v1(level):
    from oracle import nrms_oracle as orc
    if level not in _v1_cache:
        p1 = synth.make_params_v1(V1_SHAPE, seed=71)
        batch = synth.make_batch(V1_SHAPE, seed=72, **sr.BATCH_KW)
        back = {v0: v1 for v1, v0 in zip(p1.keys(), orc.v1_to_v0_names(p1).keys())}
        kw = dict(news_heads=V1_TITLE_HEADS, embed_dropout=False)
        p0 = sr.sharpen(orc.v1_to_v0_names(p1), batch, V1_SHAPE.num_attention_heads, level, **kw)
        ex = sr.exact(p0, batch, V1_SHAPE.num_attention_heads, **kw)
        _v1_cache[level] = (p0, {back[k]: v for k, v in p0.items()}, batch, back, kw, ex)
    return _v1_cache[level]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_v1_forward_backward(mode, level):
    from tests.test_hip_v1 import fwd_bwd as fwd_bwd_v1, make_v1
    p0, p1, batch, back, kw, ex = _v1(level)
    em = sr.emulated(p0, batch, V1_SHAPE.num_attention_heads, mode, **kw)
    model = make_v1(V1_SHAPE, p1, V1_TITLE_HEADS, precision=mode).train()
    scores, loss, grads = fwd_bwd_v1(model, batch)
    valid = batch["candidate_mask"] == 1
    rep = Report("v1 %s %s" % (mode, level))
    rep.check("scores", "score", mode, scores[valid], ex["scores"][valid], em["scores"][valid])
    rep.check("loss", "loss", mode, loss, ex["loss"], em["loss"])
    for n in p0:
        rep.check(n, "grad", mode, grads[back[n]], ex["grads"][n], em["grads"][n], n, ex["grads"])
    assert not grads[back[TABLE]][0].any()
    rep.done()


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_v1_masked_user_encoder(mode, level):
    """UserEncoder.forward(news_vectors, attn_masks) with both masks (mask_mode 3) on sharpened news vectors whose masked
    slots hold LOUD rows (4 x a real row): for some real queries the largest raw logit belongs to a masked key, which must
    get probability 0 -- a kernel that took its row maximum or its sum over masked keys, or masked after the softmax,
    is off by the whole attention."""
    from tests.test_hip_v1 import make_v1
    p0, p1, batch, back, kw, ex_model = _v1(level)
    h = V1_SHAPE.num_attention_heads
    x = ex_model["hist"].astype(np.float32).copy()                               # [3, 50, 300]
    lens = np.array([50, 33, 7])
    mask = (np.arange(50)[None, :] < lens[:, None]).astype(np.uint8)
    for b, n in enumerate(lens):
        x[b, n:] = 4.0 * x[b, np.arange(50 - n) % n]
    p0 = sr.sharpen_user(p0, x, h, level, mask, 3)
    st = sr.user_stats(p0, x, h, mask, 3)
    print("v1 masked %s: self std %.3f add std %.3f, real queries whose largest raw logit is a masked key: %d (oracle probability there %.1e)"
          % (level, st["self_std"], st["add_std"], st["masked_argmax_rows"], st["masked_argmax_prob"]))
    assert st["masked_argmax_rows"] > 0 and st["masked_argmax_prob"] == 0.0
    dout = np.random.default_rng(5).normal(0, 1e-2, size=(3, 300)).astype(np.float32)
    ex = sr.user_alone(p0, x, dout, h, "exact", mask, 3)
    em = sr.user_alone(p0, x, dout, h, mode, mask, 3)
    model = make_v1(V1_SHAPE, {back[k]: v for k, v in p0.items()}, V1_TITLE_HEADS, precision=mode)
    eng, flat = model.engine, model._flat
    xd, md, dd = (torch.from_numpy(a).cuda() for a in (x, mask, dout))
    out = eng.encode_users(flat, xd, save=True, mask=md, mask_mode=3)
    gflat = torch.zeros_like(flat)
    dx = eng.encode_users_backward(flat, gflat, xd, dd, mask=md, mask_mode=3)
    rep = Report("v1 masked user %s %s" % (mode, level))
    rep.check("out", "score", mode, out.cpu().numpy(), ex["out"], em["out"], times=max(1.0, float(np.abs(ex["out"]).max())))
    rep.check("dX", "grad", mode, dx.cpu().numpy(), ex["dx"], em["dx"])
    for n in ex["grads"]:
        rep.check(n, "grad", mode, model._layout.view(gflat, back[n]).cpu().numpy(), ex["grads"][n], em["grads"][n], n, ex["grads"])
    rep.done()
