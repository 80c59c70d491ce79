"""The dropout generator against a restatement that does not come from the library (tests/philox_ref.py, pinned to the published
Random123 known answers and checked for its statistics in tests/test_philox_ref_host.py).

The replay tests of the models take their keep masks from nrms_dropout_keep_mask -- the same philox4x32_7 and drop_threshold the
encoder kernels use -- so a wrong round function, key schedule, threshold or 1 / (1 - p) would leave kernels and exported mask in
agreement.  Here (1) the exported mask is bit-equal to the restatement, and (2) the fp32 / bf16x3 news encoder applies exactly
that mask and exactly the fp32 scale 1 / (1 - p): acts.x after the embedding dropout, acts.ctx after the context dropout.

Not covered: counters with a nonzero high group word (a mask above 16 GB); the fp16 layouts inside the fused kernels (the
column permutation philox_ref.fp16_column_source restates) stay with the replay tests of tests/test_hip_fp16.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib

from tests import philox_ref as ph

pytestmark = pytest.mark.gpu

F16 = _lib.NRMS_DROPOUT_FIELDS16
SITES = [0, 1, 2, 3, 4, 1 | F16]
PS = [0.0, 1e-10, 0.1, 0.5, 0.9, 1.0 - 1e-7, 1.0]
SHAPES = [(1, 4), (1, 8), (3, 12), (257, 60), (4096, 256), (1031, 320)]          # groups below, at and off the 256-thread block
SEEDS = [0, 1, 2 ** 32, 2 ** 64 - 1, ph.next_seed(1234, 7)]                     # both key words; one FlatHipModel._next_seed value
PAD0 = _lib.NRMS_FLAG_PAD_ROW_ZERO


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def export(seed, site, n_rows, d, p, buf=None):
    """(return code, uint8 [n_rows * d + 8] with the mask in front of eight bytes of 0xA5)."""
    n = n_rows * d
    buf = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda") if buf is None else buf
    rc = _lib.load().nrms_dropout_keep_mask(C.c_uint64(seed), site, C.c_int64(n_rows), d, C.c_float(p), _lib.ptr(buf), _stream())
    return rc, buf.cpu().numpy()


@pytest.mark.parametrize("n_rows,d", SHAPES)
@pytest.mark.parametrize("site", SITES, ids=lambda s: "site%x" % s)
def test_exported_mask_is_bit_equal_to_the_restatement(site, n_rows, d):
    n = n_rows * d
    if site & F16 and d % 8:
        rc, out = export(SEEDS[1], site, n_rows, d, 0.5)
        assert rc == _lib.NRMS_EINVAL and (out == 0xA5).all()                     # the 16-bit scheme needs d % 8 == 0
        return
    for seed in SEEDS:
        raw = ph.fields16(seed, site, n) if site & F16 else ph.words32(seed, site, n)
        for p in PS:
            thresh = ph.drop_threshold16(p) if site & F16 else ph.drop_threshold(p)
            want = (raw >= np.uint64(thresh)).astype(np.uint8)
            rc, out = export(seed, site, n_rows, d, p)
            assert rc == 0
            assert np.array_equal(out[:n], want), (hex(seed), p, int((out[:n] != want).sum()))
            assert (out[n:] == 0xA5).all()
            if p in (0.0, 1e-10):
                assert out[:n].all()                                              # p = 0 (and a p below 2^-32) keeps everything
            if p == 1.0 and not site & F16:
                assert out[:n].sum() == int((raw == np.uint64(0xFFFFFFFF)).sum())   # keep <=> the word is 2^32 - 1


@pytest.mark.parametrize("scheme", ["u32", "u16"])
def test_an_element_whose_word_equals_the_threshold_is_kept(scheme):
    """keep <=> r >= threshold: p is chosen so that the threshold equals the word of one element exactly (a word whose low 8 bits
    are zero is a float32 p times 2^32; a 16-bit field always is) -- `>` in place of `>=` drops that element."""
    seed, n_rows, d = SEEDS[4], 64, 64
    n = n_rows * d
    if scheme == "u32":
        site, raw, full = 0, ph.words32(seed, 0, n), 2.0 ** 32
        hit = int(np.flatnonzero(((raw & np.uint64(0xFF)) == 0) & (raw > 0))[0])
    else:
        site, raw, full = 1 | F16, ph.fields16(seed, 1, n), 2.0 ** 16
        hit = int(np.flatnonzero((raw > 1000) & (raw < 60000))[0])
    p = float(raw[hit]) / full
    thresh = ph.drop_threshold(p) if scheme == "u32" else ph.drop_threshold16(p)
    assert float(np.float32(p)) == p and thresh == int(raw[hit])
    want = (raw >= np.uint64(thresh)).astype(np.uint8)
    rc, out = export(seed, site, n_rows, d, p)
    assert rc == 0 and want[hit] == 1 and out[hit] == 1 and np.array_equal(out[:n], want)


def test_export_edges():
    rc, out = export(5, 0, 0, 8, 0.5)                                             # n_rows = 0: the buffer keeps its poison
    assert rc == 0 and (out == 0xA5).all()
    rc, out = export(5, 1 | F16, 0, 8, 0.5)
    assert rc == 0 and (out == 0xA5).all()
    for site, d in ((0, 6), (0, 1), (1 | F16, 12), (1 | F16, 4), (2, 0)):
        rc, out = export(5, site, 4, d, 0.5, buf=torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda"))
        assert rc == _lib.NRMS_EINVAL and (out == 0xA5).all(), (site, d)


# ---- the kernels apply that mask and that scale ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """model(V, d, h, q) -> (NRMSEngine, flat parameter buffer, embedding table): one fp32 engine per geometry, on its own flat
    buffer (v0 names, synthetic weights), kept for this module only."""
    from pytorch_news_recommender_amd import synth
    from pytorch_news_recommender_amd.engine import FlatLayout, ModelDims, NRMSEngine
    made = {}

    def get(V, d, h, q):
        if (V, d, h, q) not in made:
            params = synth.make_params(synth.Shape(n_words=V, word_embed_size=d, num_attention_heads=h, query_vector_dim=q), seed=11)
            dims = ModelDims(V, d, h, q, output_proj=False)
            layout = FlatLayout(dims)
            flat = torch.zeros(layout.total, dtype=torch.float32, device="cuda")
            for n, v in params.items():
                layout.view(flat, n).copy_(torch.from_numpy(v))
            table = params["news_encoder.word_embedding.0.weight"]
            assert not table[0].any() and np.abs(table[1:]).min() > 0            # the padding row is zero, no other entry is
            made[(V, d, h, q)] = (NRMSEngine(dims, "cuda", precision="fp32", layout=layout), flat, table)
        return made[(V, d, h, q)]
    yield get
    made.clear()


def ragged_ids(n_seq, S, V):
    """Right-padded titles of every length class -- full, empty (all padding), one word, a hole in the middle -- with two ids out
    of range, passed through nrms_sanitize_ids as untrusted input is."""
    rng = np.random.default_rng(S * 100 + n_seq)
    ids = rng.integers(1, V, size=(n_seq, S)).astype(np.int64)
    lens = rng.integers(1, S + 1, size=n_seq)
    lens[0], lens[1], lens[2] = S, 0, 1
    ids[np.arange(S)[None, :] >= lens[:, None]] = 0
    ids[0, 1], ids[3, 0], ids[4, 0] = 0, V + 5, -3                               # a hole; two ids the sanitizer sends to padding
    raw = torch.from_numpy(ids).cuda()
    clean, n_bad = torch.empty_like(raw), torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.load().nrms_sanitize_ids(_lib.ptr(raw), _lib.ptr(clean), ids.size, V, _lib.ptr(n_bad), _stream())
    assert rc == 0 and int(n_bad.item()) == 2
    want = np.where((ids >= 0) & (ids < V), ids, 0)
    assert np.array_equal(clean.cpu().numpy(), want)
    return clean, want


def encoder_forward(eng, flat, ids_d, n_seq, S, d, h, q, V, precision, flags, p_embed, p_ctx, seed):
    """nrms_encoder_fwd through the C ABI on poisoned activation buffers -> (acts.x, acts.ctx) as numpy [M, d]."""
    lib, M = eng.lib, n_seq * S
    desc = _lib.EncoderDesc(n_seq=n_seq, seq_len=S, d_model=d, n_heads=h, q_dim=q, vocab=V, p_drop_embed=p_embed, p_drop_ctx=p_ctx,
                            precision=_lib.PRECISIONS[precision], use_output_proj=0, mask_mode=0, flags=flags, seed=seed, loss_scale=0.0,
                            p_drop_attn=0.0, seq_index=None)
    nan = lambda n: torch.full((n,), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    bufs = dict(x=nan(M * d), qkv=nan(M * 3 * d), ctx=nan(M * d), t=nan(M * q), w=nan(M))
    ns = int(lib.nrms_encoder_fwd_scratch_bytes(C.byref(desc)))
    assert ns > 0, lib.nrms_last_error()
    bufs["scratch"] = torch.zeros((ns + 3) // 4, dtype=torch.int32, device="cuda")
    acts = _lib.EncoderActs(attn=None, **{k: v.data_ptr() for k, v in bufs.items()})
    out = nan(n_seq * d)
    w = eng._weights(flat, "news_encoder")
    rc = lib.nrms_encoder_fwd(C.byref(desc), C.byref(w), _lib.ptr(ids_d), None, None, C.byref(acts), _lib.ptr(out), _stream())
    _lib.check(rc, "nrms_encoder_fwd")
    assert np.isfinite(out.cpu().numpy()).all()
    return bufs["x"].cpu().numpy().reshape(M, d), bufs["ctx"].cpu().numpy().reshape(M, d)


CASES = [(p, S, d, h, V, n_seq, q) for (S, d, h, V, n_seq, q) in ((5, 12, 2, 37, 9, 8), (30, 300, 10, 500, 8, 200)) for p in (0.1, 0.5, 0.9)]


@pytest.mark.parametrize("flags", [0, PAD0], ids=["dense", "pad0"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("p,S,d,h,V,n_seq,q", CASES, ids=["p%.1f-S%d-d%d" % c[:3] for c in CASES])
def test_the_news_encoder_applies_that_mask_and_scale(model, p, S, d, h, V, n_seq, q, precision, flags):
    eng, flat, table = model(V, d, h, q)
    ids_d, ids = ragged_ids(n_seq, S, V)
    M = n_seq * S
    seed = ph.next_seed(1234, 3)
    flat_ids = ids.reshape(M)
    live = np.flatnonzero(flat_ids != 0)
    scale = ph.inv_keep(p)
    assert scale.dtype == np.float32
    run = lambda pe, pc: encoder_forward(eng, flat, ids_d, n_seq, S, d, h, q, V, precision, flags, pe, pc, seed)

    # embedding dropout (site 0): acts.x = table[ids] * keep * float32(1 / (1 - p)), exactly
    x, _ = run(p, 0.0)
    keep0 = ph.keep_mask(seed, 0, M, d, p)                                       # counters: the token's position in the full [M, d]
    want = table[flat_ids] * (keep0.astype(np.float32) * scale)
    assert want.dtype == np.float32
    if flags & PAD0:                                                              # compact: the live tokens in ascending order
        assert np.array_equal(x[:len(live)], want[live])
    else:
        assert np.array_equal(x, want)
    kept = want[live] != 0
    assert 0 < kept.sum() < kept.size                                             # the case does drop and does keep

    # context dropout (site 1): ctx_p = ctx_0 * keep * inv_keep to 1 ulp, zero exactly where the mask says
    _, ctx0 = run(0.0, 0.0)
    _, ctxp = run(0.0, p)
    assert np.isfinite(ctx0).all() and np.isfinite(ctxp).all()
    keep1 = ph.keep_mask(seed, 1, M, d, p)
    nz = ctx0 != 0
    assert nz.mean() > 0.9
    assert np.array_equal((ctxp != 0)[nz], keep1[nz] != 0)
    assert not ctxp[~nz].any()
    want = ctx0 * (keep1.astype(np.float32) * scale)
    assert (np.abs(ctxp.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_the_encoder_keeps_an_element_whose_word_equals_the_threshold(model, precision):
    """The compare inside the kernels (dropout_scale4 / dropout_scale1, csrc/common.h) is >=: p is the word of one element of
    the [M, d] layout over 2^32 (a word whose low 8 bits are zero is a float32 p), so the threshold equals that word and the
    element is kept; `>` would drop it.  Sites 0 and 1."""
    S, d, h, V, n_seq, q = 30, 300, 10, 500, 8, 200
    eng, flat, table = model(V, d, h, q)
    ids_d, ids = ragged_ids(n_seq, S, V)
    M = n_seq * S
    seed = ph.next_seed(1234, 3)
    flat_ids = ids.reshape(M)
    run = lambda pe, pc: encoder_forward(eng, flat, ids_d, n_seq, S, d, h, q, V, precision, 0, pe, pc, seed)
    _, ctx0 = run(0.0, 0.0)
    for site in (0, 1):
        raw = ph.words32(seed, site, M * d).reshape(M, d)
        ok = ((raw & np.uint64(0xFF)) == 0) & (raw > np.uint64(1 << 29)) & (raw < np.uint64(7 << 29))      # 1/8 < p < 7/8
        ok &= (flat_ids != 0)[:, None] if site == 0 else ctx0 != 0
        r, c = (int(v) for v in np.argwhere(ok)[0])
        p = float(raw[r, c]) / 2.0 ** 32
        assert float(np.float32(p)) == p and ph.drop_threshold(p) == int(raw[r, c])
        keep = (raw >= raw[r, c]).astype(np.float32)
        assert keep[r, c] == 1 and np.array_equal(keep, ph.keep_mask(seed, site, M, d, p))
        if site == 0:
            x, _ = run(p, 0.0)
            want = table[flat_ids] * (keep * ph.inv_keep(p))
            assert want[r, c] != 0 and x[r, c] == want[r, c] and np.array_equal(x, want)
        else:
            _, ctxp = run(0.0, p)
            nz = ctx0 != 0
            assert ctxp[r, c] != 0 and np.array_equal((ctxp != 0)[nz], (keep != 0)[nz])
