"""Peaked-attention reference for the NRMS encoders: plain torch / numpy on the CPU, float64, no GPU.

At the weights of `synth.make_params` every softmax of the model is almost uniform (news self-attention logit std 0.08,
user self-attention 0.004): exp(x) ~ 1 + x and attention is mean pooling.  This module moves the weights to where a trained
model is and says how far a correct implementation of each precision mode may be from float64 there.

  sharpen(params, batch, n_heads, level)   weights whose four attentions hit the logit stds of LEVELS[level]
  emulated(params, batch, n_heads, mode)   the float64 model with the mode's operand roundings inserted, nothing else changed
  bar(kind, mode, exact, emu)              max(the suite's existing bar, 8 x |emu - exact|)
  MUTANTS                                  wrong models a test must tell from a right one (tests/test_sharp_ref_host.py)

The model itself is restated once (`_encoder`, `_model`) with hooks where a mode rounds; with no hook active it is
oracle/nrms_oracle.py in float64 (checked to 1e-12 by the host test), which stays the reference the GPU is compared with.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nrms_oracle as orc
from pytorch_news_recommender_amd import synth

FACTOR = 8.0                      # bar = max(existing, FACTOR x emulated error); fixed, see docs/EXPERIMENTS.md
# Target logit stds: self-attention (both encoders), additive pooling (both encoders).  Chosen so that every condition of
# tests/test_sharp_ref_host.py holds on every case below (the scan is in docs/EXPERIMENTS.md); if one fails after a change,
# move these (self-attention std within [1, 3]), never FACTOR or the 2 x of the teeth.
LEVELS = {
    "warm": dict(self_std=1.6, add_std=0.6),
    "peaked": dict(self_std=2.75, add_std=0.8),
}
BATCH_KW = dict(ragged=True, min_title=1, empty_history_user=True, all_pad_title=True, mask_some_candidates=True)
CASES = {
    "mind_small": dict(shape=synth.Shape(n_words=500, word_embed_size=300, num_attention_heads=10, query_vector_dim=200,
                                         batch_size=5, history_len=9, n_candidates=4, n_words_title=30), seeds=(41, 42)),
    "hist50": dict(shape=synth.Shape(n_words=500, word_embed_size=300, num_attention_heads=10, query_vector_dim=200,
                                     batch_size=4, history_len=50, n_candidates=3, n_words_title=30), seeds=(43, 44)),
    "dk6_odd": dict(shape=synth.G1_ODD, seeds=(45, 46)),
    "l40_dk50": dict(shape=synth.Shape(n_words=200, word_embed_size=100, num_attention_heads=2, query_vector_dim=32,
                                       batch_size=3, history_len=6, n_candidates=2, n_words_title=40), seeds=(47, 48)),
}
MODES = ("fp32", "bf16x3", "fp16", "fp16+user16")
MUTANTS = {
    "M1": "logits divided by the square root of the PADDED head width (32, or 64 for heads of 33 ... 64 columns), not of d_k",
    "M2": "logits rounded to fp16 before the softmax",
    "M3": "the softmax backward's row sum over the first block of keys only (_cut_for)",
}
MA, AA = ".multihead_self_attention.", ".additive_attention."


def case_inputs(case):
    c = CASES[case]
    params = synth.make_params(c["shape"], seed=c["seeds"][0])
    batch = synth.make_batch(c["shape"], seed=c["seeds"][1], **BATCH_KW)
    return c["shape"], params, batch


def modes_of(case):
    """l40_dk50 is outside the fused fp16 kernels (heads of 50 columns, 40-word titles)."""
    return MODES[:2] if case == "l40_dk50" else MODES


# ---------------------------------------------------------------------------------------------------------------
# rounding hooks
# ---------------------------------------------------------------------------------------------------------------
class _Ste16(torch.autograd.Function):
    """Straight-through fp16 storage: forward x.half(); backward the gradient as an fp16 tensor under a power-of-two
    scale that puts max |g| into [1, 2) (the kernels' loss scale is derived the same way, fused16_bwd.hip dout16_kernel)."""

    @staticmethod
    def forward(ctx, x):
        return x.half().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        m = float(g.abs().max())
        if m == 0.0 or not math.isfinite(m):
            return g
        s = 2.0 ** (-math.floor(math.log2(m)))
        return (g * s).half().to(g.dtype) / s


def ste16(x):
    return _Ste16.apply(x)


def _split(x):
    hi = x.float().bfloat16().to(x.dtype)
    lo = (x - hi).float().bfloat16().to(x.dtype)
    return hi, lo


def _mm3_raw(a, b):
    """(Ahi + Alo)(Bhi + Blo) - Alo Blo: the three products of the split-bf16 mode, accumulated exactly."""
    ah, al = _split(a)
    bh, bl = _split(b)
    return torch.matmul(ah + al, bh + bl) - torch.matmul(al, bl)


class _MM3(torch.autograd.Function):
    """Split-bf16 product whose two gradient products run in split-bf16 as well (gemm_bf16.hip serves both directions).
    Operands of equal rank: no broadcasting."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _mm3_raw(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return _mm3_raw(g, b.transpose(-1, -2)), _mm3_raw(a.transpose(-1, -2), g)


def mm3(a, b):
    return _MM3.apply(a, b)


class _Softmax(torch.autograd.Function):
    """softmax over the last axis; `cut` > 0 is mutant M3: the backward's row sum over the first `cut` keys only."""

    @staticmethod
    def forward(ctx, s, cut):
        p = F.softmax(s, dim=-1)
        ctx.save_for_backward(p)
        ctx.cut = cut
        return p

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        pg = p * g
        if ctx.cut > 0:
            pg = pg[..., :ctx.cut]
        return p * (g - pg.sum(-1, keepdim=True)), None


class _TanhScore16(torch.autograd.Function):
    """The fused fp16 additive stage: the forward's logit uses tanh(.) as computed (fused16.hip:276-278), the backward
    reads the stored fp16 copy T16 (fused16.hip:279 -> fused16_bwd.hip:166-167: dZ = ds q (1 - T16^2), d(q) = sum ds T16)
    and hands dZ on as an fp16 operand (fused16_bwd.hip:166)."""

    @staticmethod
    def forward(ctx, z, qv):
        t = torch.tanh(z)
        ctx.save_for_backward(t.half().to(z.dtype), qv)
        return torch.matmul(t, qv)

    @staticmethod
    def backward(ctx, g):
        t16, qv = ctx.saved_tensors
        dz = g.unsqueeze(-1) * qv * (1.0 - t16 * t16)
        dq = (g.unsqueeze(-1) * t16).reshape(-1, t16.shape[-1]).sum(0)
        return _Ste16.backward(None, dz), dq


class Hooks:
    """What one run of the restated model changes about the float64 arithmetic."""

    def __init__(self, mode="f64", fp16_user=False, mutant=None):
        assert mode in ("f64", "bf16x3", "fp16") and (mutant is None or mutant in MUTANTS)
        self.mode, self.fp16_user, self.mutant = mode, fp16_user, mutant


def _cut_for(S):
    """M3's row-sum extent: the largest block edge below the row length (32 = the two blocks of a 64-row history,
    16 / 8 = lane halves of shorter rows)."""
    for c in (32, 16, 8, 4, 2, 1):
        if c < S:
            return c
    return 0


# ---------------------------------------------------------------------------------------------------------------
# the model, restated once (oracle/nrms_oracle.py: multihead_self_attention, additive_attention, forward)
# ---------------------------------------------------------------------------------------------------------------
def _encoder(p, enc, X, n_heads, hk, kind, mask=None, mask_mode=0, keep_ctx=None, p_drop=0.0, want_probs=False):
    """`kind`: "f64" plain; "bf16x3" split projections; "bf16x3_fused" split attention products too (csrc/user64.hip:12-15);
    "fp16" the fused fp16 kernels' storage roundings."""
    N, S, d = X.shape
    dk = d // n_heads
    a, b = enc + MA, enc + AA
    fp16 = kind == "fp16"
    r = ste16 if fp16 else (lambda t: t)
    split = kind in ("bf16x3", "bf16x3_fused")

    def lin(x2, w, bias):
        y = mm3(x2, w.t().contiguous()) if split else torch.matmul(x2, w.t())
        return y + bias

    qscale = 1.0 / math.sqrt((32.0 if dk <= 32 else 64.0) if hk.mutant == "M1" else dk)
    X = r(X)                                                      # x16: fused16.hip:870,886 (gather16, after the embedding dropout)
    X2 = X.reshape(N * S, d)

    def proj(name, scale):
        # wqkv16, bias in the ones column: fused16.hip:728-730 (W_Q and b_Q pre-scaled by 1/sqrt(d_k), then rounded)
        w, bias = p[a + name + ".weight"], p[a + name + ".bias"]
        if fp16:
            y = lin(X2, r(w * scale), r(bias * scale))
        else:
            y = lin(X2, w, bias) * scale
        y = y.view(N, S, n_heads, dk).transpose(1, 2)
        return r(y)                                               # Q / K / V as MFMA operands: fused16.h:19 (acc_frag), fused16.hip:172-173,198

    q, k, v = proj("W_Q", qscale), proj("W_K", 1.0), proj("W_V", 1.0)
    amm = mm3 if kind == "bf16x3_fused" else torch.matmul
    s = amm(q, k.transpose(-1, -2).contiguous())
    if hk.mutant == "M2":
        s = ste16(s)
    raw = s
    if mask is not None and (mask_mode & 1):
        m = mask.to(X.dtype)
        s = s.masked_fill((m.unsqueeze(1) * m.unsqueeze(2)).unsqueeze(1) == 0, -1e9)
    P = _Softmax.apply(s, _cut_for(S) if hk.mutant == "M3" else 0)
    ctx = amm(r(P), v)                                            # P as an fp16 operand: fused16.hip:197-199
    ctx = ctx.transpose(1, 2).contiguous().view(N, S, d)
    if a + "W_O.weight" in p:
        ctx = lin(ctx.reshape(N * S, d), p[a + "W_O.weight"], p[a + "W_O.bias"]).view(N, S, d)
    if keep_ctx is not None and p_drop > 0:
        ctx = ctx * keep_ctx.to(ctx.dtype) / (1.0 - p_drop)
    ctx = r(ctx)                                                  # ctx16: fused16.hip:219,225-226 (after the context dropout)
    z = lin(ctx.reshape(N * S, d), r(p[b + "linear.weight"]), p[b + "linear.bias"]).view(N, S, -1)      # wadd16: fused16.hip:740
    qv = p[b + "attention_query_vector"]
    sc = _TanhScore16.apply(z, qv) if fp16 else torch.matmul(torch.tanh(z), qv)                        # T16: fused16.hip:279
    if mask is not None and (mask_mode & 2):
        sc = sc.masked_fill(mask == 0, -1e9)
    w = F.softmax(sc, dim=1)
    out = torch.bmm(w.unsqueeze(1), ctx).squeeze(1)
    if want_probs:
        return out, dict(logits=raw, probs=P, add_logits=sc, add_probs=w)
    return out


def _kinds(hk, shape_H, n_heads, d, q):
    """Which arithmetic each encoder runs in (engine._desc / engine._fp16_ok)."""
    if hk.mode == "f64":
        return "f64", "f64"
    fused = 32 < shape_H <= 64 and d <= 300 and d % n_heads == 0 and (d // n_heads) <= 32 and (d // n_heads) % 2 == 0 \
        and n_heads <= 10 and q <= 224
    user_x3 = "bf16x3_fused" if fused else "bf16x3"
    if hk.mode == "bf16x3":
        return "bf16x3", user_x3
    return "fp16", ("fp16" if hk.fp16_user else user_x3)


def _model(p, batch, n_heads, hk, news_heads=None, embed_dropout=True, keep=None, p_drop=0.0, want_probs=False):
    bt = torch.as_tensor(batch["browsed_titles"]).long()
    ct = torch.as_tensor(batch["candidate_titles"]).long()
    B, H, L = bt.shape
    C = ct.shape[1]
    table = p["news_encoder.word_embedding.0.weight"]
    d = table.shape[1]
    q = p["news_encoder" + AA + "attention_query_vector"].shape[0]
    kn, ku = _kinds(hk, H, n_heads, d, q)
    ids = torch.cat([bt.reshape(B * H, L), ct.reshape(B * C, L)], dim=0)
    X = F.embedding(ids, table, padding_idx=0)
    if embed_dropout and keep is not None and keep.get("embed") is not None and p_drop > 0:
        X = X * keep["embed"].to(X.dtype) / (1.0 - p_drop)
    kc = None if keep is None else keep.get("ctx")
    nv = _encoder(p, "news_encoder", X, n_heads if news_heads is None else news_heads, hk, kn, keep_ctx=kc, p_drop=p_drop,
                  want_probs=want_probs)
    pr = {}
    if want_probs:
        nv, pr["news"] = nv
    hist, cand = nv[:B * H].view(B, H, -1), nv[B * H:].view(B, C, -1)
    user = _encoder(p, "user_encoder", hist, n_heads, hk, ku, want_probs=want_probs)
    if want_probs:
        user, pr["user"] = user
    cm = batch.get("candidate_mask")
    scores = orc.click_scores(cand, user, None if cm is None else torch.as_tensor(cm))
    return scores, dict(hist=hist, cand=cand, user=user, probs=pr)


def _pack(scores, loss, p, aux):
    grads = {k: (v.grad.detach().numpy().copy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in p.items()}
    return dict(scores=scores.detach().numpy().astype(np.float64), loss=float(loss.detach()), grads=grads,
                hist=aux["hist"].detach().numpy().astype(np.float64), cand=aux["cand"].detach().numpy().astype(np.float64),
                user=aux["user"].detach().numpy().astype(np.float64))


def run(params, batch, n_heads, hk, **kw):
    """Scores, loss, all gradients, news and user vectors of the restated model under `hk`."""
    p = orc.to_torch(params, torch.float64, requires_grad=True)
    scores, aux = _model(p, batch, n_heads, hk, **kw)
    loss = orc.loss_fn(scores)
    loss.backward()
    return _pack(scores, loss, p, aux)


def exact(params, batch, n_heads, **kw):
    """The float64 ORACLE (oracle/nrms_oracle.py itself, not the restatement)."""
    scores, loss, grads, aux = orc.loss_and_grads(params, batch, n_heads, dtype=torch.float64, **kw)
    return dict(scores=scores, loss=loss, grads=grads, hist=aux["hist"], cand=aux["cand"], user=aux["user"])


def emulated(params, batch, n_heads, mode, mutant=None, **kw):
    """The oracle with `mode`'s operand roundings.  fp32: the existing oracle run in torch float32.  `mutant` (M1 / M2 / M3)
    is applied on top of the mode's roundings; for fp32 on top of float64, whose own error (1e-7) is far below any mutant's."""
    user16 = mode.endswith("+user16")
    base = mode.split("+")[0]
    if base == "fp32" and mutant is None:
        scores, loss, grads, aux = orc.loss_and_grads(params, batch, n_heads, dtype=torch.float32, **kw)
        return dict(scores=scores.astype(np.float64), loss=loss, grads={k: v.astype(np.float64) for k, v in grads.items()},
                    hist=aux["hist"].astype(np.float64), cand=aux["cand"].astype(np.float64), user=aux["user"].astype(np.float64))
    hk = Hooks("f64" if base == "fp32" else base, fp16_user=user16, mutant=mutant)
    return run(params, batch, n_heads, hk, **kw)


# ---------------------------------------------------------------------------------------------------------------
# sharpening
# ---------------------------------------------------------------------------------------------------------------
def row_std(logits, valid=None):
    """What a softmax sees of its logits: the RMS over rows of the standard deviation over a row's keys (a constant per
    row changes nothing).  `valid` [..., keys] (0/1) leaves masked keys out; rows with fewer than two keys do not count."""
    x = logits.detach().double()
    if valid is None:
        valid = torch.ones_like(x)
    valid = valid.to(x.dtype).expand_as(x)
    n = valid.sum(-1, keepdim=True)
    mean = (x * valid).sum(-1, keepdim=True) / n.clamp(min=1)
    var = (((x - mean) ** 2) * valid).sum(-1) / n.squeeze(-1).clamp(min=1)
    rows = n.squeeze(-1) >= 2
    return float(torch.sqrt(var[rows].mean()))


def attention_stats(params, batch, n_heads, news_heads=None, embed_dropout=True):
    """Logit stds and max-probability statistics of the four attentions, float64."""
    p = orc.to_torch(params, torch.float64)
    with torch.no_grad():
        _, aux = _model(p, batch, n_heads, Hooks(), news_heads=news_heads, embed_dropout=embed_dropout, want_probs=True)
    out = {}
    for enc in ("news", "user"):
        pr = aux["probs"][enc]
        pm = pr["probs"].max(-1).values
        out[enc] = dict(self_std=row_std(pr["logits"]), add_std=row_std(pr["add_logits"]),
                        self_pmax_mean=float(pm.mean()), self_pmax_99=float((pm > 0.99).double().mean()),
                        self_range=float((pr["logits"].max(-1).values - pr["logits"].min(-1).values).max()),
                        add_pmax_mean=float(pr["add_probs"].max(-1).values.mean()),
                        min_p=float(pr["probs"].min()))
    return out


_GAINED = ("W_Q.weight", "W_Q.bias", "W_K.weight", "W_K.bias")


def sharpen(params, batch, n_heads, level, news_heads=None, embed_dropout=True):
    """A copy of `params` (v0 names) whose four attentions have the logit stds of LEVELS[level] on this batch.  W_Q / W_K
    weight and bias of an encoder times g scale its self-attention logits by exactly g^2, the query vector times c its
    pooling logits by exactly c, so each gain is one ratio; the order news self -> news additive -> user self -> user
    additive calibrates every attention on the already sharpened stages before it.  Deterministic, no randomness."""
    t = LEVELS[level]
    out = {k: np.array(v, dtype=np.float32, copy=True) for k, v in params.items()}
    gains = {}
    for enc in ("news", "user"):
        pre = enc + "_encoder"
        st = attention_stats(out, batch, n_heads, news_heads, embed_dropout)[enc]
        g = math.sqrt(t["self_std"] / st["self_std"])
        for n in _GAINED:
            out[pre + MA + n] = (out[pre + MA + n].astype(np.float64) * g).astype(np.float32)
        st = attention_stats(out, batch, n_heads, news_heads, embed_dropout)[enc]
        c = t["add_std"] / st["add_std"]
        out[pre + AA + "attention_query_vector"] = (out[pre + AA + "attention_query_vector"].astype(np.float64) * c).astype(np.float32)
        gains[enc] = (g, c)
    sharpen.last_gains = gains
    return out


# ---------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------
def existing_bar(kind, mode, ref=None, name="", refs=None):
    """The suite's bar for this mode and quantity, imported, not copied.  Scores / loss / vectors: absolute.  Gradients:
    an ELEMENT-WISE array for fp32 / bf16x3 (test_hip_parity.TOL: g_rtol |ref| + g_atol + g_scale max |ref|), one number
    per tensor for fp16 (test_hip_fp16: GRAD_REL max |ref| + GRAD_ABS).  The analytically-zero W_K.bias keeps the floor
    rules the suite already has for it: a share of d(W_Q.bias)'s scale (test_hip_fp16._grad_report; for fp32 / bf16x3
    test_hip_v1.test_masked_primitives_forward_backward)."""
    from tests import test_hip_fp16 as t16
    from tests.test_hip_parity import TOL
    base = mode.split("+")[0]
    user16 = mode.endswith("+user16")
    if kind in ("score", "loss"):
        return (1.5 if user16 else 1.0) * t16.SCORE_TOL if base == "fp16" else TOL[base]["score"]
    if kind == "vec":
        return t16.VEC_TOL if base == "fp16" else TOL[base]["score"]
    assert kind == "grad"
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    qb = None
    if name.endswith("W_K.bias") and refs is not None and name.replace("W_K", "W_Q") in refs:
        qb = float(np.abs(np.asarray(refs[name.replace("W_K", "W_Q")])).max())
    if base == "fp16":
        floor = t16.GRAD_ABS if qb is None else max(t16.GRAD_ABS, t16.GRAD_REL * qb)
        return t16.GRAD_REL * scale + floor
    t = TOL[base]
    bound = t["g_rtol"] * np.abs(ref) + t["g_atol"] + t["g_scale"] * scale
    if qb is not None:
        bound = np.maximum(bound, t["g_atol"] + (t["g_rtol"] + t["g_scale"]) * qb)
    return bound


def bar(kind, mode, exact_v, emu_v, name="", refs=None):
    """max(existing bar, FACTOR x max |emu - exact|).  Scores absolute; gradients per tensor (the emulated term is one
    number per tensor, the existing term as `existing_bar` gives it)."""
    e = float(np.abs(np.asarray(emu_v, dtype=np.float64) - np.asarray(exact_v, dtype=np.float64)).max()) if np.size(exact_v) else 0.0
    return np.maximum(existing_bar(kind, mode, exact_v, name, refs), FACTOR * e)


def excess(got, exact_v, bound):
    """max over elements of |got - exact| / bound: <= 1 passes."""
    diff = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(exact_v, dtype=np.float64))
    return float((diff / bound).max()) if diff.size else 0.0


# ---------------------------------------------------------------------------------------------------------------
# cached results per (case, level) and (case, level, mode)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sharp_case(case, level):
    shape, params, batch = case_inputs(case)
    if level != "init":
        params = sharpen(params, batch, shape.num_attention_heads, level)
    return shape, params, batch


@functools.lru_cache(maxsize=None)
def exact_case(case, level):
    shape, params, batch = sharp_case(case, level)
    return exact(params, batch, shape.num_attention_heads)


@functools.lru_cache(maxsize=None)
def emulated_case(case, level, mode, mutant=None):
    shape, params, batch = sharp_case(case, level)
    return emulated(params, batch, shape.num_attention_heads, mode, mutant=mutant)


# ---------------------------------------------------------------------------------------------------------------
# the user encoder on its own (tests of csrc/user64.hip and of the fp16 SB = 2 kernels called directly)
# ---------------------------------------------------------------------------------------------------------------
def user_alone(params, x, dout, n_heads, kind="f64", mask=None, mask_mode=0, mutant=None):
    """out, d(x) and the user encoder's parameter gradients of <out, dout>.  `kind`: "exact" = the ORACLE's user_encoder in
    float64, "fp32" = the same in torch float32, else the restated `_encoder` in float64 with that arithmetic."""
    dt = torch.float32 if kind == "fp32" else torch.float64
    p = orc.to_torch({k: v for k, v in params.items() if k.startswith("user_encoder.")}, dt, requires_grad=True)
    xt = torch.as_tensor(np.asarray(x)).to(dt).clone().requires_grad_(True)
    m = None if mask is None else torch.as_tensor(np.asarray(mask))
    if kind in ("exact", "fp32"):
        out = orc.user_encoder(p, xt, n_heads, mask=m, mask_mode=mask_mode)
    else:
        hk = Hooks("f64" if kind == "f64" else kind.split("_")[0], fp16_user=True, mutant=mutant)
        out = _encoder(p, "user_encoder", xt, n_heads, hk, kind, mask=m, mask_mode=mask_mode)
    (out * torch.as_tensor(np.asarray(dout)).to(dt)).sum().backward()
    f8 = lambda t: t.detach().numpy().astype(np.float64)
    return dict(out=f8(out), dx=f8(xt.grad),
                grads={k: (f8(v.grad) if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in p.items()})


def user_stats(params, x, n_heads, mask=None, mask_mode=0):
    """Logit stds of the user encoder's two attentions on inputs `x`, masked keys / slots left out; and whether some
    real query's LARGEST raw logit belongs to a masked key (which the mask must then send to probability 0)."""
    p = orc.to_torch({k: v for k, v in params.items() if k.startswith("user_encoder.")}, torch.float64)
    xt = torch.as_tensor(np.asarray(x)).double()
    m = None if mask is None else torch.as_tensor(np.asarray(mask))
    with torch.no_grad():
        _, pr = _encoder(p, "user_encoder", xt, n_heads, Hooks(), "f64", mask=m, mask_mode=mask_mode, want_probs=True)
    if m is None:
        return dict(self_std=row_std(pr["logits"]), add_std=row_std(pr["add_logits"]), masked_argmax_rows=0)
    md = m.double()
    logits, S = pr["logits"], m.shape[1]                                        # raw (unmasked) logits [N,h,S,S]
    key_ok = md[:, None, None, :].expand_as(logits)
    pair = key_ok * md[:, None, :, None]                                        # rows of masked queries count no key: left out
    top = logits.argmax(-1, keepdim=True)
    hit = (key_ok.gather(-1, top).squeeze(-1) == 0) & (md[:, None, :].expand(-1, logits.shape[1], -1) > 0)
    p_top = pr["probs"].gather(-1, top).squeeze(-1)
    add_raw = torch.where(md > 0, pr["add_logits"], torch.zeros_like(pr["add_logits"]))      # (-1e9 where masked)
    return dict(self_std=row_std(logits, pair), add_std=row_std(add_raw, md), masked_argmax_rows=int(hit.sum()),
                masked_argmax_prob=float(p_top[hit].max()) if bool(hit.any()) else 0.0)


def sharpen_user(params, x, n_heads, level, mask=None, mask_mode=0):
    """`sharpen` for the user encoder alone on inputs `x`, calibrated with the masks applied."""
    t = LEVELS[level]
    out = {k: np.array(v, dtype=np.float32, copy=True) for k, v in params.items()}
    pre = "user_encoder"
    g = math.sqrt(t["self_std"] / user_stats(out, x, n_heads, mask, mask_mode)["self_std"])
    for n in _GAINED:
        out[pre + MA + n] = (out[pre + MA + n].astype(np.float64) * g).astype(np.float32)
    c = t["add_std"] / user_stats(out, x, n_heads, mask, mask_mode)["add_std"]
    out[pre + AA + "attention_query_vector"] = (out[pre + AA + "attention_query_vector"].astype(np.float64) * c).astype(np.float32)
    return out
