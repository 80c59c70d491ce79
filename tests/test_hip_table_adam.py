"""NRMS_FLAG_TABLE_ADAM (include/nrms_hip.h): the news encoder's grouped scatter applies Adam to each table row it has just summed
(csrc/embed.hip scatter_grouped_adam_kernel).  The reference is the path that stays in the tree -- zeroed gradient buffer,
nrms_encoder_bwd, nrms_adam_step_guarded over the table -- and the comparison is byte for byte: parameter, both moments, the stored
gradient and the non-finite counter, over two consecutive steps (so that m and v are nonzero in the second).  Then the guard, a
float64 restatement (bucket sums in float64, oracle.adam_step) at the bars the Adam and table-gradient tests already use, and the
model level: train_step with and without NRMS_NO_FUSED_TABLE_ADAM.

Shapes: vocabularies of 2, 4, 5, 257 and 1031 words (one wave per row, four rows per block: less than a block, a block and a row,
259 blocks with a row left over); d_model 4 (one lane of the first slice), 300 (75 float4: the second slice has 11 live lanes) and
the widest each precision's grouped scatter takes -- fp32 / bf16x3: 512 (both slices full) and 1024 (four slices); fp16: 300, the
widest d_model <= 316 that divides into at most ten heads of at most 32 columns.  Buckets: 1 200 tokens over three words (each
crosses the 256-entry chunk), words that occur 0, 1, 64 and 65 times, all-padding titles, row 0.

The long buckets.  A bucket of more than 256 entries is summed chunk by chunk in the order the placement's atomics filled it: the
reference path does not reproduce ITS OWN last bits from run to run there (csrc/embed.hip, bucket_sum), so two runs cannot be
compared byte for byte on arbitrary data.  The "hot4" case therefore gives a nonzero upstream gradient to one short title only
(each hot word twice, in the last rows of its 400-entry bucket): every other term of the bucket is an exact zero, a sum of two
nonzero terms does not depend on their order, and the comparison is byte for byte again while the walk still crosses the chunks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, synth
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream
from tests.test_hip_parity import TOL, assert_grad_close, make_model, tbatch
from tests.test_hip_step_tail import assert_adam_close

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
L = 30


def ids_case(name):
    """-> (vocab, ids [N, L] int64, titles that receive a nonzero dout or None = all)."""
    rng = np.random.default_rng(len(name) * 7919 + ord(name[-1]))
    if name == "v2":                        # one real word; an all-padding title; a full title
        ids = np.zeros((6, L), dtype=np.int64)
        ids[0, :3] = 1
        ids[2, :] = 1
        ids[5, :1] = 1
        return 2, ids, None
    if name == "hot4":                      # 1 200 live tokens over words 1..3 (about 400 each), the one title with a gradient
        ids = np.zeros((42, L), dtype=np.int64)                             # (see the module docstring), an all-padding title
        ids[:40] = rng.integers(1, 4, size=(40, L))
        ids[40, :6] = [1, 2, 3, 3, 1, 2]
        return 4, ids, [40]
    if name == "v5":
        ids = rng.integers(0, 5, size=(7, L))
        ids[3] = 0
        return 5, np.sort(ids, axis=1)[:, ::-1].copy(), None
    if name == "counts257":                 # word 5: never, 6: once, 7: 64 times, 8: 65 times; the rest at random
        ids = rng.integers(9, 257, size=(12, L))
        ids[4, 10:] = 0
        ids[9] = 0
        flat = ids.reshape(-1)
        pos = rng.permutation(np.flatnonzero(flat))[:130]
        flat[pos[:1]] = 6
        flat[pos[1:65]] = 7
        flat[pos[65:130]] = 8
        assert [(ids == w).sum() for w in (5, 6, 7, 8)] == [0, 1, 64, 65]
        return 257, ids, None
    if name == "pairs":                     # no word more than twice: a bucket sum is one correctly rounded addition
        words = rng.permutation(np.arange(1, 1031))[:100]
        toks = np.concatenate([words, words[:60]])
        ids = np.zeros((9, L), dtype=np.int64)
        ids[:8, :20] = rng.permutation(toks).reshape(8, 20)
        assert np.unique(ids[ids != 0], return_counts=True)[1].max() == 2
        return 1031, ids, None
    assert name == "v1031"
    ids = rng.integers(0, 1031, size=(9, L))
    ids[:, 20:] = 0
    ids[0, :] = 1030                        # the last row of the table, in the last (partial) block
    return 1031, ids, None


def widths(prec):
    """(d_model, heads, q_dim)"""
    if prec == "fp16":
        return [(4, 2, 4), (300, 10, 200)]
    return [(4, 2, 4), (300, 10, 200), (512, 8, 64), (1024, 16, 64)]


CASES = [(p, c, w) for p in ("fp16", "bf16x3", "fp32") for w in widths(p)
         for c in (("v2", "hot4", "v5", "counts257", "v1031") if w[0] <= 300 else ("v5", "counts257"))]


class Setup:
    def __init__(self, prec, vocab, d, heads, q, seed=5):
        self.eng = NRMSEngine(ModelDims(n_words=vocab, word_embed_size=d, num_attention_heads=heads, query_vector_dim=q), "cuda",
                              precision=prec)
        self.eng.pad_row_zero = True
        lay = self.eng.layout
        g = torch.Generator().manual_seed(seed)
        flat = torch.randn(lay.total, generator=g) * (0.3 / np.sqrt(d))
        self.n_table = vocab * d
        flat[:self.n_table] = torch.randn(self.n_table, generator=g) * 0.3
        flat[:d] = 0                                                        # the padding row (NRMS_FLAG_PAD_ROW_ZERO)
        self.flat0 = flat.cuda()
        self.gen = g
        self.d = d


def run_steps(su, ids, douts, fused, p_drop, seeds, guard=True, loss_scales=(0.0, 0.0)):
    """Two (len(douts)) steps of the news encoder alone + the table's Adam.  -> list per step of dict(p, m, v, g, rest, cnt) (host
    arrays; rest = the other gradients).  loss_scales: nrms_encoder_desc.loss_scale per step (fp16; 0 = chosen on the device)."""
    eng, n_table = su.eng, su.n_table
    flat = su.flat0.clone()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    N = ids.shape[0]
    out = []
    for step, (dout, seed) in enumerate(zip(douts, seeds), start=1):
        eng.loss_scale = float(loss_scales[step - 1])
        eng.encode_titles(flat, ids, p_embed=p_drop, p_ctx=p_drop, seed=seed, save=True, tag="ta", trusted_ids=True)
        desc = eng._desc("news_encoder", N, L, p_drop, p_drop, seed, training=True)
        assert desc.precision == _lib.PRECISIONS[eng.precision] and desc.flags & _lib.NRMS_FLAG_PAD_ROW_ZERO
        if desc.precision == _lib.NRMS_PRECISION_FP16:
            desc.flags |= _lib.NRMS_FLAG_FWD_SCRATCH_KEPT
        acts = eng._acts("ta", N * L, True, gather=True, desc=desc)
        ws = eng._bwd_workspace(desc)
        w = eng._weights(flat, "news_encoder")
        g = torch.zeros_like(flat)
        if fused:
            g[:n_table] = float("nan")                                      # the table region needs no zero fill
        gn = eng._grads(g, "news_encoder")
        tail = [C.byref(gn), None, _lib.ptr(ws), C.c_size_t(ws.numel() * 4)]
        head = [C.byref(w), _lib.ptr(ids), None, None, C.byref(acts), _lib.ptr(dout)]
        if fused:
            desc.flags |= _lib.NRMS_FLAG_TABLE_ADAM
            ta = _lib.TableAdam(param=flat.data_ptr(), exp_avg=m.data_ptr(), exp_avg_sq=v.data_ptr(), lr=HP["lr"], beta1=HP["b1"],
                                beta2=HP["b2"], eps=HP["eps"], step=step, grad_scale=1.0, n_nonfinite=cnt.data_ptr() if guard else None)
            _lib.check(eng.lib.nrms_encoder_bwd_adam(C.byref(desc), *head, *tail, C.byref(ta), _stream()), "nrms_encoder_bwd_adam")
        else:
            _lib.check(eng.lib.nrms_encoder_bwd(C.byref(desc), *head, *tail, _stream()), "nrms_encoder_bwd")
            args = [C.c_size_t(n_table), _lib.ptr(flat), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), C.c_double(HP["lr"]), C.c_double(HP["b1"]),
                    C.c_double(HP["b2"]), C.c_double(HP["eps"]), step, C.c_float(1.0)]
            if guard:
                _lib.check(eng.lib.nrms_adam_step_guarded(*args, _lib.ptr(cnt), _stream()), "nrms_adam_step_guarded")
            else:
                _lib.check(eng.lib.nrms_adam_step(*args, _stream()), "nrms_adam_step")
        torch.cuda.synchronize()
        out.append(dict(p=flat[:n_table].cpu().numpy(), m=m[:n_table].cpu().numpy(), v=v[:n_table].cpu().numpy(),
                        g=g[:n_table].cpu().numpy(), rest=g[n_table:].cpu().numpy(), cnt=int(cnt.item()),
                        m_rest=m[n_table:].cpu().numpy(), ws=ws, desc=desc))
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bytes(a, b, what):
    for k in ("p", "m", "v", "g", "rest"):
        assert np.array_equal(bits(a[k]), bits(b[k])), "%s: %s differs in %d elements" % (
            what, k, int((bits(a[k]) != bits(b[k])).sum()))
    assert a["cnt"] == b["cnt"], (what, a["cnt"], b["cnt"])


def make_douts(su, N, scale=1e-2, n=2, titles=None):
    douts = [torch.randn(N, su.d, generator=su.gen) * scale for _ in range(n)]
    if titles is not None:
        keep = torch.zeros(N, 1)
        keep[titles] = 1.0
        douts = [x * keep for x in douts]
    return [x.cuda() for x in douts]


@pytest.mark.parametrize("prec,case,width", CASES, ids=["%s-%s-d%d" % (p, c, w[0]) for p, c, w in CASES])
def test_fused_table_adam_equals_scatter_then_adam_bit_for_bit(prec, case, width):
    vocab, ids_np, titles = ids_case(case)
    d, heads, q = width
    su = Setup(prec, vocab, d, heads, q)
    ids = torch.from_numpy(ids_np).cuda()
    douts = make_douts(su, ids.shape[0], titles=titles)
    for p_drop in (0.0, 0.2):
        seeds = (0, 0) if p_drop == 0.0 else (0x1234567, 0x89ABCDEF01)
        ref = run_steps(su, ids, douts, False, p_drop, seeds)
        got = run_steps(su, ids, douts, True, p_drop, seeds)
        for step in (0, 1):
            assert_same_bytes(got[step], ref[step], "%s %s d=%d p=%.1f step %d" % (prec, case, d, p_drop, step + 1))
        g = ref[1]["g"].reshape(vocab, d)
        assert (g[0] == 0).all() and not np.signbit(got[1]["g"].reshape(vocab, d)[0]).any()          # row 0: +0
        used = np.unique((ids_np if titles is None else ids_np[titles])[...].reshape(-1))
        used = used[used != 0]
        assert (np.abs(g[used]).sum(axis=1) > 0).all(), "a word of the batch without a gradient: the case tests nothing"
        absent = np.setdiff1d(np.arange(vocab), np.unique(ids_np))
        assert (g[absent] == 0).all()
        # rows without a token still took their step: m and v of the second step decay what the first left (zero here), p stays
        assert np.isfinite(got[1]["p"]).all() and (got[1]["m"].reshape(vocab, d)[used] != 0).any()
        # the unguarded kernel (fp32 / bf16x3 models run it): the same bits on finite gradients
        if prec != "fp16" and p_drop == 0.0:
            ung = run_steps(su, ids, douts, True, p_drop, seeds, guard=False)
            for step in (0, 1):
                assert_same_bytes(ung[step], ref[step], "unguarded step %d" % (step + 1))


def test_flag_is_refused_where_the_table_gradient_is_another_kernel(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("NRMS_ATOMIC_SCATTER", raising=False)
    base = dict(n_seq=4, seq_len=L, d_model=300, n_heads=10, q_dim=200, p_drop_embed=0.0, p_drop_ctx=0.0, use_output_proj=0,
                mask_mode=0, seed=0, loss_scale=0.0, p_drop_attn=0.0)
    F = _lib.NRMS_FLAG_TABLE_ADAM
    ok = _lib.EncoderDesc(vocab=50, precision=_lib.NRMS_PRECISION_FP16, flags=F | _lib.NRMS_FLAG_PAD_ROW_ZERO, **base)
    assert lib.nrms_encoder_bwd_workspace_bytes(C.byref(ok)) > 0
    for kw in (dict(vocab=50, precision=_lib.NRMS_PRECISION_FP16, flags=F),                                   # dense rows, atomics
               dict(vocab=50, precision=_lib.NRMS_PRECISION_FP16, flags=F | _lib.NRMS_FLAG_PAD_ROW_ZERO | _lib.NRMS_FLAG_DEFER_WQKV),
               dict(vocab=50, precision=_lib.NRMS_PRECISION_FP32, flags=F | _lib.NRMS_FLAG_DEFER_WQKV),
               dict(vocab=0, precision=_lib.NRMS_PRECISION_BF16X3, flags=F)):
        assert lib.nrms_encoder_bwd_workspace_bytes(C.byref(_lib.EncoderDesc(**kw, **base))) == 0
        assert b"NRMS_FLAG_TABLE_ADAM" in lib.nrms_last_error()
    # the flag without its operands (nrms_encoder_bwd has none), and operands without the flag
    w, acts, gn = _lib.EncoderWeights(), _lib.EncoderActs(), _lib.EncoderGrads()
    rc = lib.nrms_encoder_bwd(C.byref(ok), C.byref(w), None, None, None, C.byref(acts), None, C.byref(gn), None, None, 0, None)
    assert rc == _lib.NRMS_EINVAL and b"go together" in lib.nrms_last_error()
    # the other entry points have no use for the flag
    rc = lib.nrms_encoder_fwd(C.byref(ok), C.byref(w), None, None, None, C.byref(acts), None, None)
    assert rc == _lib.NRMS_EINVAL and b"NRMS_FLAG_TABLE_ADAM" in lib.nrms_last_error()
    rc = lib.nrms_encoder_bwd_wqkv(C.byref(ok), None, None, C.byref(acts), C.byref(gn), None, 0, None)
    assert rc == _lib.NRMS_EINVAL and b"NRMS_FLAG_TABLE_ADAM" in lib.nrms_last_error()
    plain = _lib.EncoderDesc(vocab=50, precision=_lib.NRMS_PRECISION_FP16, flags=_lib.NRMS_FLAG_PAD_ROW_ZERO, **base)
    rc = lib.nrms_encoder_bwd_adam(C.byref(plain), C.byref(w), None, None, None, C.byref(acts), None, C.byref(gn), None, None, 0,
                                   C.byref(_lib.TableAdam()), None)
    assert rc == _lib.NRMS_EINVAL and b"go together" in lib.nrms_last_error()
    # fp32 chain with the atomic scatter asked for by the environment (refused before anything is launched: the pointers are never read)
    monkeypatch.setenv("NRMS_ATOMIC_SCATTER", "1")
    chain = _lib.EncoderDesc(vocab=50, precision=_lib.NRMS_PRECISION_FP32, flags=F, **base)
    w2, g2 = _lib.EncoderWeights(table=4096), _lib.EncoderGrads(table=8192)
    ta = _lib.TableAdam(param=4096, exp_avg=12288, exp_avg_sq=16384, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=1.0)
    rc = lib.nrms_encoder_bwd_adam(C.byref(chain), C.byref(w2), None, None, None, C.byref(acts), None, C.byref(g2), None, None, 0,
                                   C.byref(ta), None)
    assert rc == _lib.NRMS_EINVAL and b"NRMS_ATOMIC_SCATTER" in lib.nrms_last_error()


def test_guard_skips_the_overflowed_element_and_counts_as_the_unfused_path():
    """fp16: in the second step the loss scale is fixed at 2^10 (max |dout| 0.04 -> 40: every title far inside the fp16 range; measured:
    nothing overflows below 2^22) and the upstream gradient of title 0 alone is 2^14 times larger: its loss-scaled fp16 tensors
    overflow, the table-gradient rows of ITS words come out non-finite, every other row is finite.  Those elements keep p, m, v;
    the count is the unfused path's; everything else matches bit for bit."""
    vocab, ids_np, _ = ids_case("counts257")
    su = Setup("fp16", vocab, 300, 10, 200)
    ids = torch.from_numpy(ids_np).cuda()
    N = ids.shape[0]
    douts = make_douts(su, N)
    douts[1] = douts[1].clone()
    douts[1][0] *= 2.0 ** 14
    scales = (0.0, 2.0 ** 10)
    ref = run_steps(su, ids, douts, False, 0.0, (0, 0), loss_scales=scales)
    got = run_steps(su, ids, douts, True, 0.0, (0, 0), loss_scales=scales)
    assert ref[0]["cnt"] == 0
    bad = ~np.isfinite(ref[1]["g"])
    rows_bad = np.flatnonzero(bad.reshape(vocab, 300).any(axis=1))
    print("guard: %d non-finite table-gradient elements in %d rows, counter %d" % (int(bad.sum()), rows_bad.size, ref[1]["cnt"]))
    assert 0 < bad.sum() and ref[1]["cnt"] == int(bad.sum())
    assert set(rows_bad) <= set(ids_np[0]), "a non-finite row outside title 0's words"
    others = np.setdiff1d(np.unique(ids_np[1:]), ids_np[0])
    assert others.size > 50 and np.isfinite(ref[1]["g"].reshape(vocab, 300)[others]).all()
    for step in (0, 1):
        assert_same_bytes(got[step], ref[step], "guard step %d" % (step + 1))
    for k in ("p", "m", "v"):
        assert np.array_equal(bits(got[1][k])[bad], bits(got[0][k])[bad]), k            # skipped: the first step's values
    assert (bits(got[1]["m"])[~bad] != bits(got[0]["m"])[~bad]).any()


def f64_bucket_sums(su, got, ids_np, vocab, d, p_drop, seed):
    """float64 bucket sums from the compact dX rows of the fp32 chain's backward and the embedding-dropout keep mask (site 0).
    White box: the backward writes the compact dX [n_live, d] into the d(ctx) buffer, the FIRST segment of its workspace
    (csrc/capi.hip: BwdWorkspace::dctx == 0 in bwd_layout, `g.C = gather ? dctx : dx` in step 6).  If that layout moves, the
    gradient comparison of the caller fails on every row at once -- look here first."""
    live = np.flatnonzero(ids_np.reshape(-1))
    assert got["desc"].precision == _lib.NRMS_PRECISION_FP32 and got["ws"].numel() >= live.size * d
    dx = got["ws"][:live.size * d].cpu().numpy().astype(np.float64).reshape(live.size, d)
    if p_drop:
        inv_keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop)))
        dx = dx * su.eng.dropout_keep_mask(seed, 0, ids_np.size, p_drop, d=d).cpu().numpy()[live] * inv_keep
    g64 = np.zeros((vocab, d))
    np.add.at(g64, ids_np.reshape(-1)[live], dx)
    return g64


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("case", ["counts257", "hot4_full", "pairs"])
def test_fused_table_adam_against_a_float64_restatement(case, p_drop):
    """fp32 chain, two steps, every row of the table:
    (1) the stored gradient against the bucket sums restated in float64, at the table-gradient bars of tests/test_hip_parity.py --
        buckets of up to 65 terms (counts257), and hot4 with a gradient for EVERY title: three buckets of about 400 real terms
        across the 256-entry chunks, which no byte comparison can cover (module docstring);
    (2) p, m, v against oracle.adam_step in float64 fed the STORED fp32 gradient, at the Adam bars of tests/test_hip_step_tail.py:
        both sides see the same gradient, the condition those bars were set for, so the Adam arithmetic of the fused kernel is
        checked on every bucket independently of the unfused path;
    (3) p, m, v against oracle.adam_step on the float64 SUMS, at the same bars, where the fp32 gradient is the correctly rounded
        float64 sum (case "pairs" without dropout: at most two terms, one addition).  On longer buckets the scatter's fp32
        summation error -- the same bits fused or not -- comes on top and Adam amplifies it without bound where a sum cancels to
        |g| ~ eps (tests/test_hip_parity.py assert_params_close); measured on counts257: step 2, 3 of 77 100 m elements off by
        2.8e-10 absolute (2.2e-5 relative; the bar's absolute part is 1.7e-10), p_drop 0.2 step 1: max |dp| 2.09e-7 against
        1.5e-7.  Those figures are printed, not asserted."""
    from oracle import nrms_oracle as orc
    d = 300
    vocab, ids_np, _ = ids_case("hot4" if case == "hot4_full" else case)
    su = Setup("fp32", vocab, d, 10, 200)
    ids = torch.from_numpy(ids_np).cuda()
    douts = make_douts(su, ids.shape[0])                       # (hot4_full: every title has a gradient)
    seeds = (77, 78) if p_drop else (0, 0)
    everything = np.ones(su.n_table, dtype=bool)
    ps = su.flat0[:su.n_table].cpu().numpy().astype(np.float64)        # stepped on the float64 sums
    ms, vs = np.zeros_like(ps), np.zeros_like(ps)
    for step in (1, 2):
        # (one run per step: the workspace holds the dX of the last backward only)
        # (and the state BEFORE the step is taken from the same run: a bucket of more than 256 entries has other last bits in another)
        runs = run_steps(su, ids, douts[:step], True, p_drop, seeds[:step])
        got, prev = runs[-1], (runs[-2] if step > 1 else None)
        g64 = f64_bucket_sums(su, got, ids_np, vocab, d, p_drop, seeds[step - 1])
        assert np.abs(g64).max() > 0
        assert_grad_close(got["g"].reshape(vocab, d), g64, "fp32", "table gradient, %s step %d" % (case, step))
        # (2) the kernel's own previous state and its own stored gradient through the float64 oracle
        if prev is None:
            p, m, v = su.flat0[:su.n_table].cpu().numpy().astype(np.float64), np.zeros(su.n_table), np.zeros(su.n_table)
        else:
            p, m, v = (prev[k].astype(np.float64) for k in ("p", "m", "v"))
        orc.adam_step(p, got["g"].astype(np.float64), m, v, step, lr=HP["lr"], b1=HP["b1"], b2=HP["b2"], eps=HP["eps"])
        errs = assert_adam_close((got["p"], got["m"], got["v"]), (p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)),
                                 everything, "%s step %d, stored gradient" % (case, step))
        print("float64 Adam on the stored gradient, %s p=%.1f step %d: |dp| %.2e, rel m %.2e, rel v %.2e" % ((case, p_drop, step) + errs))
        # (3) the float64 sums through the float64 oracle
        orc.adam_step(ps, g64.reshape(-1), ms, vs, step, lr=HP["lr"], b1=HP["b1"], b2=HP["b2"], eps=HP["eps"])
        want = (ps.astype(np.float32), ms.astype(np.float32), vs.astype(np.float32))
        if case == "pairs" and p_drop == 0.0:
            assert_adam_close((got["p"], got["m"], got["v"]), want, everything, "%s step %d, float64 sums" % (case, step))
        print("float64 Adam on the float64 sums, %s p=%.1f step %d: max abs |dp| %.2e, |dm| %.2e, |dv| %.2e" % (
            case, p_drop, step, float(np.abs(got["p"] - want[0]).max()), float(np.abs(got["m"] - want[1]).max()),
            float(np.abs(got["v"] - want[2]).max())))


# ---- model level -------------------------------------------------------------------------------------------------------------
SMALL = synth.Shape(n_words=300, word_embed_size=60, num_attention_heads=6, query_vector_dim=32, batch_size=5, history_len=9,
                    n_candidates=4, n_words_title=11)


def _train(precision, fused, monkeypatch, steps=3):
    if fused:
        monkeypatch.delenv("NRMS_NO_FUSED_TABLE_ADAM", raising=False)
    else:
        monkeypatch.setenv("NRMS_NO_FUSED_TABLE_ADAM", "1")
    torch.manual_seed(1234)
    params = synth.make_params(SMALL, seed=111)
    model = make_model(SMALL, params, dropout=0.2, precision=precision).train()
    eng = model.engine
    eng.timing(True)
    eng.timing_reset()
    losses = []
    for i in range(steps):
        batch = synth.make_batch(SMALL, seed=200 + i, ragged=True, min_title=1)
        losses.append(model.train_step(tbatch(batch), lr=1e-3).cpu().numpy().copy())
    torch.cuda.synchronize()
    timers = {k: eng.timing_read(k)[1] for k in ("adam", "rest_adam", "scatter_dropout")}
    eng.timing(False)
    st = model._opt
    return dict(flat=model._flat.detach().cpu().numpy(), g=st["g"].cpu().numpy(), m=st["m"].cpu().numpy(), v=st["v"].cpu().numpy(),
                loss=np.concatenate(losses), timers=timers, step=st["step"])


@pytest.mark.parametrize("precision", ["fp16", "bf16x3", "fp32"])
def test_train_step_with_and_without_the_fused_table_adam(precision, monkeypatch):
    a = _train(precision, True, monkeypatch)
    b = _train(precision, False, monkeypatch)
    assert a["step"] == b["step"] == 3
    for k in ("flat", "g", "m", "v", "loss"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (precision, k, int((bits(a[k]) != bits(b[k])).sum()))
    # "adam" is read by prefix: 3 fused kernels, no "adam_*" beside them; the remainder under its own name; no scatter launch
    assert a["timers"] == {"adam": 3, "rest_adam": 3, "scatter_dropout": 0}, a["timers"]
    assert b["timers"] == {"adam": 3, "rest_adam": 0, "scatter_dropout": 3}, b["timers"]


def test_nrms_naml_keeps_the_separate_optimizer(monkeypatch):
    """Title and abstract both scatter into the one table: NamlEngine overrides backward(), fuses_table_adam() is False."""
    monkeypatch.delenv("NRMS_NO_FUSED_TABLE_ADAM", raising=False)
    from tests.test_hip_naml import make_model as make_naml
    s = synth.G7_ODD
    params = synth.make_params_naml(s, seed=3)
    model = make_naml(s, params, precision="bf16x3").train()
    batch = synth.make_batch_naml(s, seed=4)
    eng = model.engine
    eng.timing(True)
    eng.timing_reset()
    model.train_step(tbatch(batch), lr=1e-3)
    torch.cuda.synchronize()
    n_adam, n_rest = eng.timing_read("adam")[1], eng.timing_read("rest_adam")[1]
    n_scatter = eng.timing_read("scatter_dropout")[1]
    eng.timing(False)
    assert not eng.fuses_table_adam()
    assert (n_adam, n_rest) == (1, 0) and n_scatter >= 2, (n_adam, n_rest, n_scatter)
