"""Every buffer a C ABI call writes, between guard bands and with poisoned prior contents (tests/guarded.py).

The library allocates nothing: a caller sizes workspace / scratch / saved by the *_bytes queries and every activation, output and
gradient buffer by the extent include/nrms_hip.h states; torch's caching allocator then puts other live tensors right behind
them and hands back recycled blocks.  Each case here asserts

  (a) bands intact    after EVERY call of its sequence, around every buffer the callee writes;
  (b) independence    the same sequence under the poisons 0xFF / 0x00 / 0x7F (written before the first call; the fp16
                      acts.scratch between a forward and its NRMS_FLAG_FWD_SCRATCH_KEPT backward and every `saved` buffer
                      keep what the forward left: that content is contract) gives bit-identical outputs and gradients;
  (c) parity          with the float64 / numpy reference the entry point's own test uses, at that test's tolerance
                      (imported, not restated), so a kernel that returns early cannot pass (a) and (b) vacuously.

Inputs stay inside the documented reproducibility claims: word ids occur at most 64 times per call (csrc/embed.hip),
NRMS_ATOMIC_SCATTER is unset.  ONE path is reproducible by no documented claim: the fp16 news encoder WITHOUT
NRMS_FLAG_PAD_ROW_ZERO scatters its table gradient with float atomics (launch_scatter_dense_rows); there the table gradient is
held to (c) in every poisoned run instead of to bit equality (test_news_encoder, fp16, pad0).  Accumulated / caller-initialised
buffers (gradient structs, n_bad, n_dropped, newsvec d_table, du1 / du2) are guarded and initialised as documented.

Found by these tests and fixed with them: launch_scatter_prepare (csrc/embed.hip) kept the ceil(vocab / 1024) block totals of its
scan in the M + 64 ints of the token buckets -- the last segment of the backward workspace; from ceil(vocab / 1024) > M + 127 on it
stored past the end of nrms_encoder_bwd_workspace_bytes (test_large_vocabulary_tiny_batch: at vocab = 300 000, M = 8 the helper
reports the overwritten range, docs/EXPERIMENTS.md).  nrms_encoder_bwd_wqkv, nrms_newsvec_rows_fwd and nrms_hier_tree_build
answered an undersized workspace with NRMS_EINVAL; they now return NRMS_EWORKSPACE like every other entry point.
And by (b): the fp16 backward of titles longer than 32 words (csrc/fused16_bwd.hip, the 64-row kernels) was handed the three
title lists of the 32-row kernels, walked the long titles only and never wrote the dQKV rows of a short title (a prefix of 1 .. 15
words): that title's share of the table gradient and of d(W_qkv) was whatever the workspace held -- 0 after a zeroed block, NaN
after 0xFF (test_news_encoder[fp16-f1-n3-S33]: table row 133, the one-word title).  The 64-row kernels now take the titles in
index order, as the forward does.

Entry point / size query                                  -> cases
  nrms_encoder_fwd / _bwd / _bwd_wqkv
    nrms_encoder_fwd_scratch_bytes, _bwd_workspace_bytes     test_news_encoder (4 precisions x pad / defer / kept x 5 shapes),
                                                             test_large_vocabulary_tiny_batch, test_block_boundaries_tokens,
                                                             test_block_boundaries_vocab, test_all_padding_and_no_padding,
                                                             test_user_encoder, test_user_encoder_v1_masks, test_wide_paths
    nrms_encoder_fused_qkv_bytes                             test_user_encoder[fused33 / fused64]
    need - 1                                                 test_encoder_undersized_workspace
  nrms_sequence_partition, nrms_encoder_empty_fwd / _bwd
    nrms_encoder_empty_workspace_bytes, _saved_bytes         test_empty_sequences (0, 1, all sequences empty; need - 1 of the
                                                             workspace in both directions; `saved` has no size parameter)
  nrms_topk_dot (nrms_topk_dot_workspace_bytes)              test_topk_dot (need - 1 inside)
  nrms_topk_grouped_dot (..._grouped_dot_workspace_bytes)    test_topk_grouped_dot (need - 1 inside)
  nrms_layernorm_bwd (nrms_layernorm_bwd_workspace_bytes)    test_layernorm_bwd (need - 1 inside)
  nrms_segment_pool_fwd / _bwd, nrms_csr_from_padded
    nrms_segment_pool_workspace_bytes                        test_segment_pool, test_csr_from_padded (need - 1 in test_segment_pool)
  nrms_graph_sample_neighbors / nrms_graph_resolve_rows
    nrms_graph_sample_workspace_bytes (0), _resolve_...      test_graph_sample_and_resolve (need - 1 inside)
  nrms_hier_tree_build (nrms_hier_tree_scratch_bytes)        test_hier_tree_build (need - 1 inside)
  nrms_hier_add_embedding_bwd (..._bwd_workspace_bytes)      test_hier_add_embedding_bwd (need - 1 inside)
  nrms_newsvec_fwd / _bwd / _distinct
    nrms_newsvec_saved_bytes, nrms_newsvec_workspace_bytes   test_newsvec (need - 1 for saved and workspace, both directions)
  nrms_newsvec_rows_fwd (nrms_newsvec_rows_workspace_bytes)  test_newsvec_rows (need - 1 inside)
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib

from tests.guarded import POISONS, Pool, assert_same_bits
from tests.test_hip_parity import TOL, assert_grad_close

pytestmark = pytest.mark.gpu

F32, F16, I32, I64, U8 = torch.float32, torch.float16, torch.int32, torch.int64, torch.uint8
EWS = _lib.NRMS_EWORKSPACE
PAD0, DEFER, KEPT, FUSED = _lib.NRMS_FLAG_PAD_ROW_ZERO, _lib.NRMS_FLAG_DEFER_WQKV, _lib.NRMS_FLAG_FWD_SCRATCH_KEPT, _lib.NRMS_FLAG_FUSED_SEQ64


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda().contiguous()


def ok(rc, what):
    _lib.check(rc, what)


def three_poisons(run, what, not_bitwise=()):
    """run(poison) -> {name: ndarray} (it checks its own bands).  -> the 0xFF run, after (b)."""
    runs = {p: run(p) for p in POISONS}
    assert_same_bits({p: {k: v for k, v in r.items() if k not in not_bitwise} for p, r in runs.items()}, what)
    return runs


def refuses_undersized(call, pool, need, what):
    """call(bytes) with need - 1: the workspace error, and no byte of any guarded buffer changes (a host-side check)."""
    assert need > 0, what
    snap = pool.snapshot()
    rc = call(need - 1)
    assert rc == EWS, "%s with %d of %d bytes returned %d, not NRMS_EWORKSPACE" % (what, need - 1, need, rc)
    assert b"<" in _lib.load().nrms_last_error()
    pool.assert_unchanged(snap, what + " (undersized)")
    pool.intact(what + " (undersized)")


# ---- encoder chain --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def _model(V, d, h, q, wo):
    from tests.test_hip_extents import make_engine
    return make_engine(max(V, 4), d, h, q, "fp32", wo=wo, seed=5)


def make_ids(n_seq, S, V, kind):
    """Right-padded titles with a hole; every id at most 64 times (the reproducibility limit of the grouped scatter).  A vocabulary
    much larger than the batch is sampled at the ends and on both sides of the 1 024-id blocks of the scan."""
    M = n_seq * S
    k = np.arange(M)
    if V > 4 * M + 4096:
        nb = (V + 1023) // 1024
        cand = [1, V - 1, V - 2, V // 2] + [b * 1024 + o for b in (1, 2, nb // 2, nb - 1) for o in (-1, 0, 1)]
        cand = np.unique([c for c in cand if 0 < c < V])
        tok = cand[k % len(cand)]
    else:
        tok = 1 + (k * 37) % (V - 1)
    lens = (5 * np.arange(n_seq) + 2) % (S + 1)
    lens[0] = S
    if n_seq > 1:
        lens[1] = 0
    if n_seq > 2:
        lens[2] = 1
    if kind == "nopad":
        lens[:] = S
    if kind == "allpad":
        lens[:] = 0
    ids = np.where(np.arange(S)[None, :] < lens[:, None], tok.reshape(n_seq, S), 0).astype(np.int64)
    if S >= 3 and kind == "mix":
        ids[0, 1] = 0
    if (ids > 0).any():
        assert np.bincount(ids[ids > 0]).max() <= 64
    return ids


class Enc:
    """One encoder case: model, inputs and (lazily, once) its float64 reference, shared by the three poisoned runs."""

    def __init__(self, mode, V, d, h, q, n_seq, S, flags=0, wo=False, mask_mode=0, kind="mix"):
        self.mode, self.V, self.d, self.h, self.q, self.n_seq, self.S = mode, V, d, h, q, n_seq, S
        self.flags, self.wo, self.mask_mode, self.kind = flags, wo, mask_mode, kind
        self.news = V > 0
        self.enc = "news_encoder" if self.news else "user_encoder"
        self.eng, self.flat, self.layout, self.params = _model(V, d, h, q, wo)
        rng = np.random.default_rng(1000 * S + n_seq)
        self.dout = rng.normal(0.1, 1.0, size=(n_seq, d)).astype(np.float32)
        self.mask = None
        if self.news:
            self.xin = make_ids(n_seq, S, V, kind)
        else:
            self.xin = rng.normal(0.1, 0.5, size=(n_seq, S, d)).astype(np.float32)
            if mask_mode:
                lens = np.array([S, max(1, (2 * S) // 3), 1, 0, max(1, S - 2), S])[:n_seq]
                self.mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.uint8)

    def desc(self, extra=0):
        return _lib.EncoderDesc(n_seq=self.n_seq, seq_len=self.S, d_model=self.d, n_heads=self.h, q_dim=self.q,
                                vocab=self.V if self.news else 0, p_drop_embed=0.0, p_drop_ctx=0.0, precision=_lib.PRECISIONS[self.mode],
                                use_output_proj=int(self.wo), mask_mode=self.mask_mode, flags=(self.flags & (PAD0 | FUSED)) | extra,
                                seed=0, loss_scale=0.0, p_drop_attn=0.0, seq_index=None)

    def buffers(self, poison):
        """Every buffer of the pass at its documented extent (include/nrms_hip.h, nrms_encoder_acts)."""
        lib, P = self.eng.lib, Pool(poison)
        M, d, q, n_seq = self.n_seq * self.S, self.d, self.q, self.n_seq
        desc = self.desc()
        a = {}
        if self.mode == "fp16":
            Mp = n_seq * (32 if self.S <= 32 else 64)
            a["x"] = P.elems("acts.x", (M + 1) * _lib.NRMS_FP16_KP, F16)
            a["ctx"] = P.elems("acts.ctx", Mp * _lib.NRMS_FP16_DP, F16)
            a["t"] = P.elems("acts.t", Mp * _lib.NRMS_FP16_QP, F16)
            if self.wo:
                a["attn"] = P.elems("acts.attn", Mp * _lib.NRMS_FP16_DP, F16)
        else:
            if self.news:
                a["x"] = P.elems("acts.x", M * d)
            if self.flags & FUSED:
                nb = int(lib.nrms_encoder_fused_qkv_bytes(C.byref(desc)))
                assert nb > 0
                a["qkv"] = P.new("acts.qkv", nb)
            else:
                a["qkv"] = P.elems("acts.qkv", M * 3 * d)
            if self.wo:
                a["attn"] = P.elems("acts.attn", M * d)
            a["ctx"] = P.elems("acts.ctx", M * d)
            a["t"] = P.elems("acts.t", M * q)
        a["w"] = P.elems("acts.w", M)
        ns = int(lib.nrms_encoder_fwd_scratch_bytes(C.byref(desc)))
        assert ns > 0, lib.nrms_last_error()
        a["scratch"] = P.new("acts.scratch", ns)
        P.elems("out", n_seq * d)
        if not self.news:
            P.elems("dx", M * d)
        self.need = int(lib.nrms_encoder_bwd_workspace_bytes(C.byref(desc)))
        assert self.need > 0, lib.nrms_last_error()
        P.new("workspace", self.need)
        P.elems("grads", self.layout.total, init="zero")                   # ACCUMULATED: zeroed, as model.zero_grad() does
        acts = _lib.EncoderActs(**{k: g.ptr.value for k, g in a.items()})
        return P, acts

    def forward(self, P, acts):
        lib = self.eng.lib
        self.w = self.eng._weights(self.flat, self.enc)
        self.g = self.eng._grads(P["grads"].view, self.enc)
        self.xd, self.dd = dev(self.xin), dev(self.dout)
        self.md = None if self.mask is None else dev(self.mask)
        desc = self.desc()
        ok(lib.nrms_encoder_fwd(C.byref(desc), C.byref(self.w), _lib.ptr(self.xd) if self.news else None,
                                None if self.news else _lib.ptr(self.xd), _lib.ptr(self.md), C.byref(acts), P["out"].ptr, _stream()),
           "nrms_encoder_fwd")
        P.intact("nrms_encoder_fwd")

    def backward_call(self, P, acts, extra, nbytes):
        desc = self.desc(extra)
        return self.eng.lib.nrms_encoder_bwd(C.byref(desc), C.byref(self.w), _lib.ptr(self.xd) if self.news else None,
                                             None if self.news else _lib.ptr(self.xd), _lib.ptr(self.md), C.byref(acts), _lib.ptr(self.dd),
                                             C.byref(self.g), None if self.news else P["dx"].ptr, P["workspace"].ptr, C.c_size_t(nbytes),
                                             _stream())

    def wqkv_call(self, P, acts, extra, nbytes):
        desc = self.desc(extra)
        return self.eng.lib.nrms_encoder_bwd_wqkv(C.byref(desc), _lib.ptr(self.xd) if self.news else None,
                                                  None if self.news else _lib.ptr(self.xd), C.byref(acts), C.byref(self.g),
                                                  P["workspace"].ptr, C.c_size_t(nbytes), _stream())

    def run(self, poison, refill=None):
        """refill {buffer name: byte}: a diagnostic's way to poison one buffer differently from the others."""
        P, acts = self.buffers(poison)
        for name, byte in (refill or {}).items():
            P[name].fill(byte)
        self.forward(P, acts)
        extra = self.flags & (DEFER | KEPT)
        ok(self.backward_call(P, acts, extra, self.need), "nrms_encoder_bwd")
        P.intact("nrms_encoder_bwd")
        if extra & DEFER:
            ok(self.wqkv_call(P, acts, extra, self.need), "nrms_encoder_bwd_wqkv")
            P.intact("nrms_encoder_bwd_wqkv")
        res = {"out": P["out"].numpy((self.n_seq, self.d))}
        if not self.news:
            res["dx"] = P["dx"].numpy((self.n_seq, self.S, self.d))
        gflat = P["grads"].view.clone()
        for name in self.names():
            res[name] = self.layout.view(gflat, name).cpu().numpy().copy()
        return res

    def names(self):
        return [k for k in self.params if k.startswith(self.enc) or (self.news and "word_embedding" in k)]

    TABLE = "news_encoder.word_embedding.0.weight"

    @functools.cached_property
    def ref(self):
        from tests.test_hip_extents import reference
        return reference(self.params, self.enc, self.h, self.xin, self.dout, mask=self.mask, mask_mode=self.mask_mode)

    def parity(self, res, only=None):
        """The bars of the precision: TOL (tests/test_hip_parity.py) for fp32 / bf16x3 as tests/test_hip_extents.py applies them;
        fp16: VEC_TOL and twice GRAD_REL of a tensor's scale + 1e-4 of the largest (tests/test_hip_fp16.py, as
        tests/test_hip_fuzz.py / test_hip_extents.py apply them to single encoder passes); bf16: the score and gradient bars of
        tests/test_hip_parity.py (BF16_*; test_reduced_precision_modes leaves the table and W_K.bias out) with the floor for
        cancelling sums reasoned there."""
        from tests.test_hip_fp16 import GRAD_ABS, GRAD_REL, VEC_TOL
        from tests.test_hip_parity import BF16_CANCEL_FLOOR, BF16_GRAD_RTOL, BF16_SCORE_TOL
        r_out, r_dx, r_grads = self.ref
        what = "%s %s n_seq=%d S=%d d=%d V=%d flags=%d" % (self.mode, self.enc, self.n_seq, self.S, self.d, self.V, self.flags)
        names = [n for n in r_grads if only is None or n in only]
        kb = lambda n: float(np.abs(r_grads[n.replace("W_K.bias", "W_Q.bias")]).max())
        if self.mode in TOL:
            t = TOL[self.mode]
            if only is None:
                np.testing.assert_allclose(res["out"], r_out, rtol=0, atol=t["score"], err_msg=what)
                if r_dx is not None:
                    assert_grad_close(res["dx"], r_dx, self.mode, what + " dx")
            for n in names:
                if n.endswith("W_K.bias"):          # analytically zero: bounded by the scale of d(b_Q) (tests/test_hip_extents.py)
                    err = float(np.abs(res[n] - r_grads[n]).max())
                    assert err <= t["g_atol"] + (t["g_rtol"] + t["g_scale"]) * kb(n), (what, n, err)
                else:
                    assert_grad_close(res[n], r_grads[n], self.mode, what + " " + n)
            return
        big = max(float(np.abs(v).max()) for v in r_grads.values())
        floor = 1e-4 * big + GRAD_ABS
        if self.mode == "fp16":
            vec, rel, skip = VEC_TOL, 2 * GRAD_REL, ()
        else:
            # (bf16 operands carry 8 significant bits, fewer than fp16's 11: the floor for the tensors whose terms cancel -- here
            # b_add, |gradient| ~ 3e-5 beside tensors of 1e-1 -- cannot be smaller than the one the fp16 bars grant)
            vec, rel, floor = BF16_SCORE_TOL, BF16_GRAD_RTOL, BF16_CANCEL_FLOOR * big + GRAD_ABS
            skip = (self.TABLE, "W_K.bias")
        if only is None:
            assert float(np.abs(res["out"] - r_out).max()) <= vec, (what, float(np.abs(res["out"] - r_out).max()))
            if r_dx is not None:
                assert float(np.abs(res["dx"] - r_dx).max()) <= rel * float(np.abs(r_dx).max()) + floor, what
        for n in names:
            if any(n.endswith(s) for s in skip):
                continue
            sc = float(np.abs(r_grads[n]).max())
            if n.endswith("W_K.bias"):
                sc = max(sc, kb(n))
            err = float(np.abs(res[n] - r_grads[n]).max())
            assert err <= rel * sc + floor, (what, n, err, sc)


def check_encoder(case):
    atomic = case.mode == "fp16" and case.news and not (case.flags & PAD0)       # float atomics: see the module docstring
    runs = three_poisons(case.run, "%s %s" % (case.mode, case.enc), not_bitwise=(Enc.TABLE,) if atomic else ())
    case.parity(runs[POISONS[0]])
    if atomic:
        for p in POISONS[1:]:
            case.parity(runs[p], only=(Enc.TABLE,))
    if case.news:
        assert not runs[POISONS[0]][Enc.TABLE][0].any()                          # the padding row takes no gradient


SHAPES = [(1, 1), (3, 17), (5, 32), (3, 33), (5, 64)]
VARIANTS = {"fp32": [0, PAD0, DEFER, PAD0 | DEFER], "bf16x3": [0, PAD0, DEFER, PAD0 | DEFER], "bf16": [0, PAD0, DEFER, PAD0 | DEFER],
            "fp16": [0, PAD0, PAD0 | KEPT, PAD0 | KEPT | DEFER]}
NEWS = [(m, f, n, S) for m in VARIANTS for f in VARIANTS[m] for (n, S) in SHAPES]


@pytest.mark.parametrize("mode,flags,n_seq,S", NEWS, ids=["%s-f%d-n%d-S%d" % c for c in NEWS])
def test_news_encoder(mode, flags, n_seq, S):
    """The news encoder in all four precisions: dense / NRMS_FLAG_PAD_ROW_ZERO, with NRMS_FLAG_DEFER_WQKV + nrms_encoder_bwd_wqkv,
    fp16 with and without NRMS_FLAG_FWD_SCRATCH_KEPT.  Width 64 (q 60): the fp16 bars are meant for widths from 60 up
    (tests/test_hip_fuzz.py)."""
    check_encoder(Enc(mode, 211, 64, 4, 60, n_seq, S, flags=flags))


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "fp16"])
@pytest.mark.parametrize("V", [300000, 1024 * (8 + 128), 1024 * (8 + 128) + 1])
def test_large_vocabulary_tiny_batch(V, mode):
    """One title of 8 words over a vocabulary whose scan has more block totals (ceil(V / 1024) = 293, 136, 137) than the batch has
    tokens: the totals used to be stored in the M + 64 ints of the token buckets, the LAST segment of the backward workspace."""
    check_encoder(Enc(mode, V, 4, 2, 4, 1, 8, flags=PAD0 if mode == "fp16" else 0))


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("n_seq,S", [(33, 31), (32, 32), (41, 25)], ids=["M1023", "M1024", "M1025"])
def test_block_boundaries_tokens(n_seq, S, mode):
    """M = 1023, 1024, 1025 tokens, padding and live mixed: CP_BLOCK of the compaction kernels (csrc/embed.hip)."""
    assert n_seq * S in (1023, 1024, 1025)
    check_encoder(Enc(mode, 211, 64, 4, 60, n_seq, S, flags=PAD0))


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("V", [1023, 1024, 1025, 2049])
def test_block_boundaries_vocab(V, mode):
    """The 1 024-id blocks of scan_local_kernel / scan_add_kernel."""
    check_encoder(Enc(mode, V, 64, 4, 60, 3, 17, flags=PAD0))


@pytest.mark.parametrize("mode,flags", [("fp32", 0), ("fp32", PAD0), ("bf16x3", PAD0), ("fp16", PAD0)])
@pytest.mark.parametrize("kind", ["allpad", "nopad"])
def test_all_padding_and_no_padding(kind, mode, flags):
    check_encoder(Enc(mode, 211, 64, 4, 60, 5, 17, flags=flags, kind=kind))


USER = {"plain_fp32": ("fp32", 5, 32, 0), "plain_bf16x3": ("bf16x3", 3, 17, 0), "plain_one_row": ("fp32", 1, 1, 0),
        "chain33": ("bf16x3", 3, 33, 0), "fused33": ("bf16x3", 3, 33, FUSED), "fused64": ("bf16x3", 5, 64, FUSED)}


@pytest.mark.parametrize("case", list(USER))
def test_user_encoder(case):
    """vocab = 0: the chain, and NRMS_FLAG_FUSED_SEQ64 (csrc/user64.hip) with acts.qkv = nrms_encoder_fused_qkv_bytes bytes."""
    mode, n_seq, S, flags = USER[case]
    check_encoder(Enc(mode, 0, 64, 4, 60, n_seq, S, flags=flags))


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("mask_mode", [1, 2, 3])
def test_user_encoder_v1_masks(mask_mode, mode):
    """The v1 topology (output projection W_O, acts.attn) with the pairwise and pooling masks; one history is fully masked."""
    check_encoder(Enc(mode, 0, 64, 4, 60, 5, 17, wo=True, mask_mode=mask_mode))


WIDE = {"d1024_news": (211, 1024, 16, 256, 3, 17, PAD0), "odd_dk_news": (211, 20, 4, 12, 3, 17, 0), "odd_dk_user": (0, 20, 4, 12, 5, 33, 0),
        "q512_user": (0, 256, 2, 512, 3, 17, 0)}


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(WIDE))
def test_wide_paths(case, mode):
    """d_model = 1024 (the SL = 4 grouped scatter, the wide additive attention), odd d_k and d_k = 128 (csrc/wide.hip)."""
    V, d, h, q, n_seq, S, flags = WIDE[case]
    check_encoder(Enc(mode, V, d, h, q, n_seq, S, flags=flags))


@pytest.mark.parametrize("mode,V,flags", [("fp32", 211, PAD0), ("bf16x3", 0, 0), ("fp16", 211, PAD0), ("bf16x3", 0, FUSED)])
def test_encoder_undersized_workspace(mode, V, flags):
    """nrms_encoder_bwd (and, on the chain, nrms_encoder_bwd_wqkv) with one byte less than the query asked for."""
    case = Enc(mode, V, 64, 4, 60, 3, 33 if flags & FUSED else 17, flags=flags)
    P, acts = case.buffers(0xFF)
    case.forward(P, acts)
    refuses_undersized(lambda n: case.backward_call(P, acts, 0, n), P, case.need, "nrms_encoder_bwd")
    if mode != "fp16":                             # (fp16: the call only orders the helper streams and takes no workspace)
        refuses_undersized(lambda n: case.wqkv_call(P, acts, DEFER, n), P, case.need, "nrms_encoder_bwd_wqkv")


# ---- all-padding sequences in closed form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["none", "one", "all"])
def test_empty_sequences(rule):
    """nrms_sequence_partition into guarded order [2 n_seq] / counts, then nrms_encoder_empty_fwd / _bwd on the all-padding list
    (seq_index = the second list, where the partition left it) with 0, 1 and all of 7 sequences empty.  `saved` keeps what the
    forward wrote; the workspace is poisoned again before the backward.  Parity: an all-padding title through the float64 oracle
    of the same topology (oracle/nrms_oracle.py with the output projection -- the function oracle/naml_oracle.py's text_vector
    states, without its dropout), at TOL fp32 as the encoder cases apply it.  Entries of `order` outside the two lists are not
    defined and not compared."""
    lib = _lib.load()
    n_seq, S, V, d, h, q = 7, 17, 211, 64, 4, 60
    eng, flat, layout, params = _model(V, d, h, q, True)
    ids = make_ids(n_seq, S, V, "nopad")
    empty = {"none": [], "one": [3], "all": list(range(n_seq))}[rule]
    ids[empty] = 0
    ids[5 % n_seq, 2:] = 0 if rule != "all" else ids[5 % n_seq, 2:]            # a padding tail does not make a sequence empty
    n_e = len(empty)
    case = Enc("fp32", V, d, h, q, n_e, S, flags=PAD0, wo=True, kind="allpad") if n_e else None
    dout = case.dout if n_e else np.zeros((0, d), np.float32)
    idd, dd = dev(ids), dev(dout if n_e else np.zeros((1, d), np.float32))
    desc = _lib.EncoderDesc(n_seq=n_e, seq_len=S, d_model=d, n_heads=h, q_dim=q, vocab=V, p_drop_embed=0.0, p_drop_ctx=0.0,
                            precision=_lib.NRMS_PRECISION_FP32, use_output_proj=1, mask_mode=0, flags=PAD0, seed=0, loss_scale=0.0,
                            p_drop_attn=0.0, seq_index=None)
    need, n_saved = int(lib.nrms_encoder_empty_workspace_bytes(C.byref(desc))), int(lib.nrms_encoder_empty_saved_bytes(C.byref(desc)))
    assert need > 0 and (n_saved > 0) == (n_e > 0), lib.nrms_last_error()
    w = eng._weights(flat, "news_encoder")
    names = [k for k in params if k.startswith("news_encoder") or "word_embedding" in k]

    def run(poison):
        P = Pool(poison)
        P.elems("order", 2 * n_seq, I32), P.elems("counts", int(lib.nrms_sequence_partition_count_ints(n_seq)), I32)
        P.elems("out", n_e * d), P.new("saved", n_saved), P.new("workspace", need)
        P.elems("grads", layout.total, init="zero")                            # ACCUMULATED
        g = eng._grads(P["grads"].view, "news_encoder")
        ok(lib.nrms_sequence_partition(_lib.ptr(idd), n_seq, S, P["order"].ptr, P["counts"].ptr, _stream()), "nrms_sequence_partition")
        P.intact("nrms_sequence_partition")
        order, counts = P["order"].numpy(), P["counts"].numpy()
        assert (int(counts[0]), int(counts[1])) == (n_seq - n_e, n_e)
        sidx = C.c_void_p(P["order"].ptr.value + 4 * n_seq)                   # the all-padding list

        def fwd(nbytes):
            return lib.nrms_encoder_empty_fwd(C.byref(desc), C.byref(w), sidx, P["out"].ptr, P["saved"].ptr, P["workspace"].ptr,
                                              C.c_size_t(nbytes), _stream())

        def bwd(nbytes):
            return lib.nrms_encoder_empty_bwd(C.byref(desc), C.byref(w), sidx, _lib.ptr(dd), P["saved"].ptr, C.byref(g), P["workspace"].ptr,
                                              C.c_size_t(nbytes), _stream())

        if n_e and poison == POISONS[0]:
            refuses_undersized(fwd, P, need, "nrms_encoder_empty_fwd")
        ok(fwd(need), "nrms_encoder_empty_fwd")
        P.intact("nrms_encoder_empty_fwd")
        P["workspace"].fill(poison)
        if n_e and poison == POISONS[0]:
            refuses_undersized(bwd, P, need, "nrms_encoder_empty_bwd")
        ok(bwd(need), "nrms_encoder_empty_bwd")
        P.intact("nrms_encoder_empty_bwd")
        res = {"live": order[:n_seq - n_e], "empty": order[n_seq:n_seq + n_e], "counts": counts[:2], "out": P["out"].numpy((n_e, d))}
        gflat = P["grads"].view.clone()
        for name in names:
            res[name] = layout.view(gflat, name).cpu().numpy().copy()
        return res

    r = three_poisons(run, "empty sequences")[POISONS[0]]
    assert r["empty"].tolist() == empty and r["live"].tolist() == [i for i in range(n_seq) if i not in empty]
    if n_e:
        case.parity(r)
    else:
        assert not any(r[name].any() for name in names)


# ---- top-k ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,d,k", [(1, 0, 8, 1), (1, 1, 8, 256), (3, 31, 20, 1), (2, 32, 20, 256), (3, 33, 7, 5), (1, 33, 300, 256)])
def test_topk_dot(B, N, d, k):
    from tests.test_hip_topk import _assert_exact, _host_topk, _int_data
    lib = _lib.load()
    if N:
        user, items, ex = _int_data(B, N, d, seed=N + k, n_ex=6)
    else:
        user, items, ex = np.ones((B, d), np.float32), np.zeros((0, d), np.float32), None
    ud, itd, exd = dev(user), dev(items if N else np.zeros((1, d), np.float32)), None if ex is None else dev(ex, I64)
    need = int(lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k))
    assert need > 0

    def call(P, nbytes):
        return lib.nrms_topk_dot(B, C.c_int64(N), d, k, _lib.ptr(ud), _lib.ptr(itd), _lib.ptr(exd), 0 if ex is None else ex.shape[1],
                                 P["top_scores"].ptr, P["top_ids"].ptr, P["workspace"].ptr, C.c_size_t(nbytes), _stream())

    def run(poison):
        P = Pool(poison)
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, I64), P.new("workspace", need)
        ok(call(P, need), "nrms_topk_dot")
        P.intact("nrms_topk_dot")
        if poison == POISONS[0]:
            refuses_undersized(lambda n: call(P, n), P, need, "nrms_topk_dot")
        return {"scores": P["top_scores"].numpy((B, k)), "ids": P["top_ids"].numpy((B, k))}

    r = three_poisons(run, "nrms_topk_dot")[POISONS[0]]
    _assert_exact((r["scores"], r["ids"]), _host_topk(user, items, k, ex))


@pytest.mark.parametrize("B,N,d,k", [(1, 0, 8, 1), (1, 1, 8, 256), (3, 31, 20, 1), (2, 32, 20, 256), (3, 33, 7, 5), (1, 200, 300, 256)])
def test_topk_grouped_dot(B, N, d, k):
    """Groups include empty ones, before, between and behind the items; N smaller than k; N = 0."""
    from tests.test_hip_topk_grouped import _assert_exact, _host
    lib = _lib.load()
    rng = np.random.default_rng(N + k)
    sizes = [0, N // 3, 0, 0, N - N // 3 - N // 4, N // 4, 0]
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    G = len(sizes)
    assert gp[-1] == N
    query = rng.integers(-3, 4, size=(B, G, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    ids = rng.permutation(4 * N + 4)[:N].astype(np.int32)
    ex = None
    if N > 4:
        items[N // 2] = np.nan
        ex = ids[rng.integers(0, N, size=(B, 5))].astype(np.int64)
        ex[:, 0] = -1
    qd, itd, idd = dev(query), dev(items if N else np.zeros((1, d), np.float32)), dev(ids if N else np.zeros(1, np.int32))
    gpd, exd = dev(gp), None if ex is None else dev(ex)
    need = int(lib.nrms_topk_grouped_dot_workspace_bytes(B, C.c_int64(N), d, k, G))
    assert need > 0

    def call(P, nbytes):
        return lib.nrms_topk_grouped_dot(B, C.c_int64(N), d, k, G, _lib.ptr(qd), _lib.ptr(itd), _lib.ptr(idd), _lib.ptr(gpd), _lib.ptr(exd),
                                         0 if ex is None else ex.shape[1], P["top_scores"].ptr, P["top_ids"].ptr, P["workspace"].ptr,
                                         C.c_size_t(nbytes), _stream())

    def run(poison):
        P = Pool(poison)
        P.elems("top_scores", B * k), P.elems("top_ids", B * k, I64), P.new("workspace", need)
        ok(call(P, need), "nrms_topk_grouped_dot")
        P.intact("nrms_topk_grouped_dot")
        if poison == POISONS[0]:
            refuses_undersized(lambda n: call(P, n), P, need, "nrms_topk_grouped_dot")
        return {"scores": P["top_scores"].numpy((B, k)), "ids": P["top_ids"].numpy((B, k))}

    r = three_poisons(run, "nrms_topk_grouped_dot")[POISONS[0]]
    _assert_exact((r["scores"], r["ids"]), _host(query, items, ids, gp, k, ex))


# ---- layer norm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,d", [(1, 4), (257, 4), (1, 1024), (257, 1024), (257, 100)])
def test_layernorm_bwd(n_rows, d):
    """Against torch's layer_norm in float64 at LN_TOL, the absolute tolerances of tests/test_hip_naml.py::test_layernorm_alone.
    That test sums 37 rows of unit-variance dy into d(gamma) / d(beta) with norm weights near 1; the inputs here keep those
    scales (gamma in 0.8 .. 1.2, beta in -0.1 .. 0.1, dy scaled by sqrt(37 / n_rows) beyond 37 rows), so the same bounds apply."""
    from tests.test_hip_naml import LN_TOL
    lib = _lib.load()
    rng = np.random.default_rng(d + n_rows)
    x = (rng.standard_normal((n_rows, d)) * 3 + 1).astype(np.float32)
    gamma, beta = rng.uniform(0.8, 1.2, d).astype(np.float32), rng.uniform(-0.1, 0.1, d).astype(np.float32)
    dy = (rng.standard_normal((n_rows, d)) * min(1.0, np.sqrt(37.0 / n_rows))).astype(np.float32)
    xd, gd, bd, dyd = dev(x), dev(gamma), dev(beta), dev(dy)
    need = int(lib.nrms_layernorm_bwd_workspace_bytes(d))
    assert need > 0

    def bwd(P, nbytes):
        return lib.nrms_layernorm_bwd(C.c_int64(n_rows), d, _lib.ptr(xd), _lib.ptr(gd), P["stats"].ptr, _lib.ptr(dyd), P["dx"].ptr,
                                      P["dgamma_dbeta"].ptr, P["workspace"].ptr, C.c_size_t(nbytes), _stream())

    def run(poison):
        P = Pool(poison)
        P.elems("y", n_rows * d), P.elems("stats", n_rows * 2), P.elems("dx", n_rows * d), P.new("workspace", need)
        P.elems("dgamma_dbeta", 2 * d, init="zero")                            # ACCUMULATED
        ok(lib.nrms_layernorm_fwd(C.c_int64(n_rows), d, _lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), C.c_float(1e-5), P["y"].ptr, P["stats"].ptr,
                                  _stream()), "nrms_layernorm_fwd")
        P.intact("nrms_layernorm_fwd")
        if poison == POISONS[0]:
            refuses_undersized(lambda n: bwd(P, n), P, need, "nrms_layernorm_bwd")
        ok(bwd(P, need), "nrms_layernorm_bwd")
        P.intact("nrms_layernorm_bwd")
        return {"y": P["y"].numpy((n_rows, d)), "dx": P["dx"].numpy((n_rows, d)), "dgb": P["dgamma_dbeta"].numpy()}

    r = three_poisons(run, "nrms_layernorm")[POISONS[0]]
    xr, wr, br = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, gamma, beta))
    yr = torch.nn.functional.layer_norm(xr, (d,), wr, br, 1e-5)
    yr.backward(torch.from_numpy(dy).double())
    np.testing.assert_allclose(r["y"], yr.detach().numpy(), rtol=0, atol=LN_TOL["y"])
    np.testing.assert_allclose(r["dx"], xr.grad.numpy(), rtol=LN_TOL["rtol"], atol=LN_TOL["dx"])
    np.testing.assert_allclose(r["dgb"][:d], wr.grad.numpy(), rtol=LN_TOL["rtol"], atol=LN_TOL["dgb"])
    np.testing.assert_allclose(r["dgb"][d:], br.grad.numpy(), rtol=LN_TOL["rtol"], atol=LN_TOL["dgb"])


# ---- segment pool ---------------------------------------------------------------------------------------------------------------
SEG = {"partition": (77, 13, 20, 8, True), "shared_rows": (64, 20, 300, 200, False), "one_hot_row": (9, 40, 20, 8, False), "nnz0": (5, 3, 20, 8, True)}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(SEG))
def test_segment_pool(case, precision):
    """With and without NRMS_SEGPOOL_ROWS_UNIQUE, empty segments, one row listed by every segment, nnz = 0; against
    oracle/segpool_oracle.py at the bounds of tests/test_hip_segpool.py."""
    from oracle import segpool_oracle as orc
    from tests.test_hip_segpool import OUT_TOL, _case, grad_bound
    lib = _lib.load()
    R, n_seg, d, q, unique = SEG[case]
    x, w, b, qv, ptr, idx = _case(R, n_seg, d, q, seed=5, partition=unique)
    if case == "one_hot_row":
        idx = np.where(np.arange(len(idx)) % 2 == 0, 4, idx).astype(np.int32)          # row 4: a member of (nearly) every segment
    if case == "nnz0":
        ptr, idx = np.zeros(n_seg + 1, np.int32), np.zeros(0, np.int32)
    nnz = int(ptr[-1])
    dout = (np.random.default_rng(9).standard_normal((n_seg, d)) * 1e-2).astype(np.float32)
    desc = _lib.SegPoolDesc(n_rows=R, n_seg=n_seg, nnz=nnz, d=d, q=q, precision=_lib.PRECISIONS[precision],
                            flags=_lib.NRMS_SEGPOOL_ROWS_UNIQUE if unique else 0)
    need = int(lib.nrms_segment_pool_workspace_bytes(C.byref(desc)))
    xd, wd, bd, qd, pd, idd, dd = dev(x), dev(w), dev(b), dev(qv), dev(ptr), dev(idx if nnz else np.zeros(1, np.int32)), dev(dout)

    def fwd(P, nbytes):
        return lib.nrms_segment_pool_fwd(C.byref(desc), _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(qd), _lib.ptr(pd), _lib.ptr(idd),
                                         P["t"].ptr, P["logit"].ptr, P["alpha"].ptr, P["out"].ptr, P["workspace"].ptr, C.c_size_t(nbytes),
                                         _stream())

    def bwd(P, nbytes):
        return lib.nrms_segment_pool_bwd(C.byref(desc), _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(qd), _lib.ptr(pd), _lib.ptr(idd), P["t"].ptr,
                                         P["alpha"].ptr, _lib.ptr(dd), P["dx"].ptr, P["dw_add"].ptr, P["db_add"].ptr, P["dq_vec"].ptr,
                                         P["workspace"].ptr, C.c_size_t(nbytes), _stream())

    def run(poison):
        P = Pool(poison)
        P.elems("t", R * q), P.elems("logit", R), P.elems("alpha", nnz), P.elems("out", n_seg * d), P.elems("dx", R * d)
        P.new("workspace", need)
        for name, n in (("dw_add", q * d), ("db_add", q), ("dq_vec", q)):
            P.elems(name, n, init="zero")                                      # ACCUMULATED
        if need and poison == POISONS[0]:
            refuses_undersized(lambda n: fwd(P, n), P, need, "nrms_segment_pool_fwd")
        ok(fwd(P, need), "nrms_segment_pool_fwd")
        P.intact("nrms_segment_pool_fwd")
        P["workspace"].fill(poison)                                            # (t and alpha are the saved state; the workspace is not)
        if need and poison == POISONS[0]:
            snap_t = P["t"].snapshot()
            refuses_undersized(lambda n: bwd(P, n), P, need, "nrms_segment_pool_bwd")
            assert P["t"].unchanged_since(snap_t)
        ok(bwd(P, need), "nrms_segment_pool_bwd")
        P.intact("nrms_segment_pool_bwd")
        return {"out": P["out"].numpy((n_seg, d)), "dx": P["dx"].numpy((R, d)), "dW": P["dw_add"].numpy((q, d)), "db": P["db_add"].numpy(),
                "dq": P["dq_vec"].numpy()}

    r = three_poisons(run, "nrms_segment_pool")[POISONS[0]]
    to = lambda a: torch.from_numpy(a).clone().requires_grad_(True)
    ox, ow, ob, oq = to(x), to(w), to(b), to(qv)
    o_out = orc.segment_pool(ox, ow, ob, oq, ptr.tolist(), idx.tolist())
    if nnz:                                                                    # (no member anywhere: every gradient is zero)
        (o_out * torch.from_numpy(dout)).sum().backward()
    o_out = o_out.detach()
    tol = OUT_TOL[precision]
    assert float(np.abs(r["out"] - o_out.numpy()).max()) < tol * max(1.0, float(o_out.abs().max()))
    for name, o in (("dx", ox), ("dW", ow), ("db", ob), ("dq", oq)):
        ref = (o.grad if o.grad is not None else torch.zeros_like(o)).numpy()
        bound = grad_bound(torch.from_numpy(ref)).numpy()
        assert (np.abs(r[name] - ref) <= bound).all(), (case, precision, name, float(np.abs(r[name] - ref).max()))


@pytest.mark.parametrize("n_seg,K,n_rows", [(1, 1, 1), (37, 7, 50), (300, 64, 1000), (5, 3, 0)])
def test_csr_from_padded(n_seg, K, n_rows):
    """seg_ptr [n_seg + 1] and idx [n_seg * K] (a capacity: entries from seg_ptr[n_seg] on are not defined and not compared)."""
    lib = _lib.load()
    rng = np.random.default_rng(n_seg + K)
    lists = rng.integers(-1, max(n_rows, 1) + 3, size=(n_seg, K)).astype(np.int64)
    lists[rng.random((n_seg, K)) < 0.3] = -1
    ld = dev(lists)
    keep = (lists >= 0) & (lists < n_rows)
    want_ptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int32)
    want_idx = lists[keep].astype(np.int32)

    def run(poison):
        P = Pool(poison)
        P.elems("seg_ptr", n_seg + 1, I32), P.elems("idx", n_seg * K, I32)
        ok(lib.nrms_csr_from_padded(C.c_int64(n_seg), K, _lib.ptr(ld), C.c_int64(n_rows), P["seg_ptr"].ptr, P["idx"].ptr, _stream()),
           "nrms_csr_from_padded")
        P.intact("nrms_csr_from_padded")
        return {"seg_ptr": P["seg_ptr"].numpy(), "idx": P["idx"].numpy()[:int(want_ptr[-1])]}

    r = three_poisons(run, "nrms_csr_from_padded")[POISONS[0]]
    assert np.array_equal(r["seg_ptr"], want_ptr) and np.array_equal(r["idx"], want_idx)


# ---- click graph ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap_rule", ["one", "at", "below"])
@pytest.mark.parametrize("n_news", [33, 1025])
def test_graph_sample_and_resolve(n_news, cap_rule):
    """nrms_graph_sample_neighbors (a zero-byte workspace query: a zero-length guarded view, bands still checked) and
    nrms_graph_resolve_rows with cap = 1, exactly the number of distinct out-of-batch ids and one fewer; against the numpy
    restatements of tests/test_hip_graph_sampler.py (bit equality)."""
    from tests.test_hip_graph_sampler import arrays, build, resolve_ref, sample_ref, zipf_histories, _slots
    lib = _lib.load()
    K, N, seed = 8, 11, 0xDEADBEEF12345678
    hist = zipf_histories(60, 6, n_news, seed=7, min_len=1)
    g = build(hist, n_news)
    slot_np = _slots(n_news, N, seed=3)
    clicked = np.unique(hist[hist > 0])
    slot_np[3:] = clicked[::max(1, len(clicked) // (N - 3))][:N - 3]           # clicked news: their neighbours are mostly out of batch
    slot_np[:3] = [0, n_news + 3, -2]
    want_nbr = sample_ref(arrays(g), slot_np, K, seed)
    n_distinct = resolve_ref(slot_np, want_nbr, 0, n_news)[3]
    assert n_distinct > 1
    cap = {"one": 1, "at": n_distinct, "below": n_distinct - 1}[cap_rule]
    slots = dev(slot_np)
    gd = _lib.ClickGraphDesc(n_users=g.n_users, n_news=g.n_news, n_edges=g.n_edges, user_ptr=g.user_ptr.data_ptr(),
                             user_news=g.user_news.data_ptr(), news_ptr=g.news_ptr.data_ptr(), news_users=g.news_users.data_ptr())
    need_s = int(lib.nrms_graph_sample_workspace_bytes(C.c_int64(N), K))
    need_r = int(lib.nrms_graph_resolve_workspace_bytes(C.c_int64(n_news)))
    assert need_s == 0 and need_r > 0

    def resolve(P, nbytes):
        return lib.nrms_graph_resolve_rows(C.c_int64(N), K, C.c_int64(n_news), _lib.ptr(slots), P["neighbor_ids"].ptr, cap,
                                           P["neighbor_rows"].ptr, P["extra_ids"].ptr, P["n_extra"].ptr, P["n_dropped"].ptr,
                                           P["resolve_ws"].ptr, C.c_size_t(nbytes), _stream())

    def run(poison):
        P = Pool(poison)
        P.elems("neighbor_ids", N * K, I32), P.new("sample_ws", need_s), P.elems("neighbor_rows", N * K, I64)
        P.elems("extra_ids", cap, I32), P.elems("n_extra", 1, I32), P.new("resolve_ws", need_r)
        P.elems("n_bad", 1, I32, init="zero"), P.elems("n_dropped", 1, I32, init=np.array([5], np.int32))     # counters accumulate
        ok(lib.nrms_graph_sample_neighbors(C.byref(gd), C.c_int64(N), K, _lib.ptr(slots), C.c_uint64(seed), P["neighbor_ids"].ptr,
                                           P["n_bad"].ptr, P["sample_ws"].ptr, C.c_size_t(need_s), _stream()), "nrms_graph_sample_neighbors")
        P.intact("nrms_graph_sample_neighbors")
        if poison == POISONS[0]:
            refuses_undersized(lambda n: resolve(P, n), P, need_r, "nrms_graph_resolve_rows")
        ok(resolve(P, need_r), "nrms_graph_resolve_rows")
        P.intact("nrms_graph_resolve_rows")
        return {k: P[k].numpy() for k in ("neighbor_ids", "neighbor_rows", "extra_ids", "n_extra", "n_bad", "n_dropped")}

    r = three_poisons(run, "click graph")[POISONS[0]]
    w_rows, w_extra, w_keep, w_dropped = resolve_ref(slot_np, want_nbr, cap, n_news)
    assert np.array_equal(r["neighbor_ids"].reshape(N, K), want_nbr) and int(r["n_bad"][0]) == 2
    assert np.array_equal(r["neighbor_rows"].reshape(N, K), w_rows) and np.array_equal(r["extra_ids"], w_extra)
    assert int(r["n_extra"][0]) == w_keep and int(r["n_dropped"][0]) == 5 + w_dropped


# ---- HieRec index side ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,valid_rule", [(3, 1, "some"), (5, 64, "some"), (2, 64, "none"), (130, 33, "some")])
def test_hier_tree_build(B, H, valid_rule):
    """H = 1 and 64, users without a valid click (all of them under "none"); the lists against python_tree of
    tests/test_hip_hierec.py.  l*_idx are capacities [B * H]: entries from l*_ptr[-1] on are not defined and not compared, nor
    are the ids of empty group slots (count 0)."""
    from tests.test_hip_hierec import python_tree
    lib = _lib.load()
    rng = np.random.default_rng(B * 100 + H)
    valid = (rng.random((B, H)) < 0.7).astype(np.uint8)
    if B > 1:
        valid[1] = 0
    if valid_rule == "none":
        valid[:] = 0
    sub = rng.integers(1, 9, size=(B, H)).astype(np.int64)
    topic = (sub + 1) // 2
    vd, td, sd = dev(valid), dev(topic), dev(sub)
    n = B * H
    names = ("l1_ptr", "l1_idx", "l1_sub", "l1_top", "l1_cnt", "l2_ptr", "l2_idx", "l2_top", "l2_cnt", "l3_ptr", "l3_idx", "n_valid")
    sizes = {"l1_ptr": n + 1, "l2_ptr": n + 1, "l3_ptr": B + 1, "n_valid": B}
    need = int(lib.nrms_hier_tree_scratch_bytes(B, H))
    assert need > 0

    def call(P, nbytes):
        return lib.nrms_hier_tree_build(B, H, _lib.ptr(vd), _lib.ptr(td), _lib.ptr(sd), *[P[k].ptr for k in names], P["scratch"].ptr,
                                        C.c_size_t(nbytes), _stream())

    def run(poison):
        P = Pool(poison)
        for k in names:
            P.elems(k, sizes.get(k, n), I32)
        P.new("scratch", need)
        if poison == POISONS[0]:
            refuses_undersized(lambda nb: call(P, nb), P, need, "nrms_hier_tree_build")
        ok(call(P, need), "nrms_hier_tree_build")
        P.intact("nrms_hier_tree_build")
        g = {k: P[k].numpy() for k in names}
        for lvl in ("l1", "l2", "l3"):
            g[lvl + "_idx"] = g[lvl + "_idx"][:int(g[lvl + "_ptr"][-1])]
        g["l1_sub"], g["l1_top"] = np.where(g["l1_cnt"] > 0, g["l1_sub"], 0), np.where(g["l1_cnt"] > 0, g["l1_top"], 0)
        g["l2_top"] = np.where(g["l2_cnt"] > 0, g["l2_top"], 0)
        return g

    g = three_poisons(run, "nrms_hier_tree_build")[POISONS[0]]
    seg = lambda ptr, idx, s: list(idx[ptr[s]:ptr[s + 1]])
    for b in range(B):
        subs, tops = python_tree(valid[b], topic[b], sub[b])
        assert g["n_valid"][b] == int(valid[b].sum())
        for s in range(H):
            slot = b * H + s
            if s < len(subs):
                assert sorted(seg(g["l1_ptr"], g["l1_idx"], slot)) == [b * H + k for k in subs[s][2]]
                assert (g["l1_sub"][slot], g["l1_top"][slot], g["l1_cnt"][slot]) == (subs[s][0], subs[s][1], len(subs[s][2]))
            else:
                assert seg(g["l1_ptr"], g["l1_idx"], slot) == [] and g["l1_cnt"][slot] == 0
            if s < len(tops):
                assert sorted(seg(g["l2_ptr"], g["l2_idx"], slot)) == [b * H + gi for gi in tops[s][1]]
                assert g["l2_top"][slot] == tops[s][0] and g["l2_cnt"][slot] == sum(len(subs[gi][2]) for gi in tops[s][1])
            else:
                assert seg(g["l2_ptr"], g["l2_idx"], slot) == [] and g["l2_cnt"][slot] == 0
        assert sorted(seg(g["l3_ptr"], g["l3_idx"], b)) == [b * H + s for s in range(len(tops))]


@pytest.mark.parametrize("n_slots,d,n_ids", [(1, 8, 1), (63, 8, 5), (64, 8, 5), (65, 20, 5), (129, 300, 7)])
def test_hier_add_embedding_bwd(n_slots, d, n_ids):
    """n_ids = 1 and n_slots across the 64-slot chunks of the partial sums; dtable is ACCUMULATED (it starts from a known value).
    Reference: the float64 sum; a row sums at most n_slots fp32 terms in a fixed order: rtol 1e-3 + atol 2e-6, the gradient bound
    of tests/test_hip_parity.py (TOL fp32)."""
    lib = _lib.load()
    rng = np.random.default_rng(n_slots + d)
    ids = rng.integers(-1, n_ids + 1, size=n_slots).astype(np.int32)           # one below and one above the table: no gradient
    cnt = (rng.random(n_slots) < 0.8).astype(np.int32) * 3
    du = rng.standard_normal((n_slots, d)).astype(np.float32)
    start = rng.standard_normal((n_ids, d)).astype(np.float32)
    idd, cd, dud = dev(ids), dev(cnt), dev(du)
    need = int(lib.nrms_hier_add_embedding_bwd_workspace_bytes(C.c_int64(n_slots), d, n_ids))
    assert need > 0

    def call(P, nbytes):
        return lib.nrms_hier_add_embedding_bwd(C.c_int64(n_slots), d, n_ids, _lib.ptr(idd), _lib.ptr(cd), _lib.ptr(dud), P["dtable"].ptr,
                                               P["workspace"].ptr, C.c_size_t(nbytes), _stream())

    def run(poison):
        P = Pool(poison)
        P.elems("dtable", n_ids * d, init=start), P.new("workspace", need)
        if poison == POISONS[0]:
            refuses_undersized(lambda n: call(P, n), P, need, "nrms_hier_add_embedding_bwd")
        ok(call(P, need), "nrms_hier_add_embedding_bwd")
        P.intact("nrms_hier_add_embedding_bwd")
        return {"dtable": P["dtable"].numpy((n_ids, d))}

    r = three_poisons(run, "nrms_hier_add_embedding_bwd")[POISONS[0]]
    ref = start.astype(np.float64)
    for s in range(n_slots):
        if cnt[s] > 0 and 0 <= ids[s] < n_ids:
            ref[ids[s]] += du[s]
    assert_grad_close(r["dtable"], ref, "fp32", "dtable")


# ---- nrms_bert's news-vector layer -----------------------------------------------------------------------------------------------
NEWSVEC = {"same_id": (40, 16, 20, "same"), "distinct": (40, 64, 20, "distinct"), "one_slot": (1, 16, 20, "mixed"), "d1024": (33, 50, 1024, "mixed")}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", list(NEWSVEC))
def test_newsvec(case, precision):
    """nrms_newsvec_fwd / _bwd / _distinct: all slots one id, all ids distinct, one slot, d = 1024.  `saved` keeps what the forward
    wrote; the workspace is poisoned again before the backward.  d_table is caller-zeroed (the rows of the batch's ids are
    overwritten), d_w / d_b accumulate.  Reference: float64 numpy; bounds TOL of tests/test_hip_nrms_bert.py."""
    from tests.test_hip_nrms_bert import TOL as BTOL, close
    lib = _lib.load()
    n, V, d, rule = NEWSVEC[case]
    rng = np.random.default_rng(n + d)
    ids = {"same": np.full(n, 7), "distinct": rng.permutation(V)[:n], "mixed": rng.integers(0, V, size=n)}[rule].astype(np.int64)
    if n > 4:
        ids[3] = V + 5 if rule != "distinct" else ids[3]                        # out of range: read as id 0, counted
    table = (rng.standard_normal((V, d)) * 0.5).astype(np.float32)
    w = (rng.uniform(-1, 1, (d, d)) * np.sqrt(3.0 / d)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, d).astype(np.float32)
    dout = rng.standard_normal((n, d)).astype(np.float32)
    desc = _lib.NewsvecDesc(n_slots=n, n_rows=V, d=d, precision=_lib.PRECISIONS[precision], p_drop=0.0, seed=0)
    ns, nw = int(lib.nrms_newsvec_saved_bytes(C.byref(desc))), int(lib.nrms_newsvec_workspace_bytes(C.byref(desc)))
    assert ns > 0 and nw > 0
    idd, td, wd, bd, dd = dev(ids), dev(table), dev(w), dev(b), dev(dout)

    def fwd(P, s_bytes, w_bytes):
        return lib.nrms_newsvec_fwd(C.byref(desc), _lib.ptr(idd), _lib.ptr(td), _lib.ptr(wd), _lib.ptr(bd), P["out"].ptr, P["saved"].ptr,
                                    C.c_size_t(s_bytes), P["n_bad"].ptr, P["workspace"].ptr, C.c_size_t(w_bytes), _stream())

    def bwd(P, s_bytes, w_bytes):
        return lib.nrms_newsvec_bwd(C.byref(desc), _lib.ptr(td), _lib.ptr(wd), _lib.ptr(dd), P["saved"].ptr, C.c_size_t(s_bytes),
                                    P["d_table"].ptr, P["d_w"].ptr, P["d_b"].ptr, P["workspace"].ptr, C.c_size_t(w_bytes), _stream())

    def run(poison):
        P = Pool(poison)
        P.elems("out", n * d), P.new("saved", ns), P.new("workspace", nw), P.elems("n_unique", 1, I32), P.elems("distinct", n, I32)
        P.elems("n_bad", 1, I32, init="zero")
        for name, m in (("d_table", V * d), ("d_w", d * d), ("d_b", d)):
            P.elems(name, m, init="zero")
        if poison == POISONS[0]:
            refuses_undersized(lambda k: fwd(P, k, nw), P, ns, "nrms_newsvec_fwd (saved)")
            refuses_undersized(lambda k: fwd(P, ns, k), P, nw, "nrms_newsvec_fwd (workspace)")
        ok(fwd(P, ns, nw), "nrms_newsvec_fwd")
        P.intact("nrms_newsvec_fwd")
        ok(lib.nrms_newsvec_distinct(C.byref(desc), P["saved"].ptr, P["n_unique"].ptr, P["distinct"].ptr, _stream()), "nrms_newsvec_distinct")
        P.intact("nrms_newsvec_distinct")
        P["workspace"].fill(poison)
        if poison == POISONS[0]:
            refuses_undersized(lambda k: bwd(P, k, nw), P, ns, "nrms_newsvec_bwd (saved)")
            refuses_undersized(lambda k: bwd(P, ns, k), P, nw, "nrms_newsvec_bwd (workspace)")
        ok(bwd(P, ns, nw), "nrms_newsvec_bwd")
        P.intact("nrms_newsvec_bwd")
        nu = int(P["n_unique"].numpy()[0])
        return {"out": P["out"].numpy((n, d)), "n_unique": np.array([nu]), "distinct": P["distinct"].numpy()[:nu], "n_bad": P["n_bad"].numpy(),
                "d_table": P["d_table"].numpy((V, d)), "d_w": P["d_w"].numpy((d, d)), "d_b": P["d_b"].numpy()}

    r = three_poisons(run, "nrms_newsvec")[POISONS[0]]
    idc = np.where((ids >= 0) & (ids < V), ids, 0)
    t64, w64, d64 = table.astype(np.float64), w.astype(np.float64), dout.astype(np.float64)
    t = BTOL[precision]
    assert np.array_equal(r["distinct"], np.unique(idc)) and int(r["n_bad"][0]) == int((ids != idc).sum())
    ref_out = t64[idc] @ w64.T + b
    assert float(np.abs(r["out"] - ref_out).max()) <= t["score"] * max(1.0, float(np.abs(ref_out).max()))
    dy = np.zeros((V, d))
    np.add.at(dy, idc, d64)
    close(r["d_table"], dy @ w64, t, "d_table")
    u = np.unique(idc)
    close(r["d_w"], dy[u].T @ t64[u], t, "d_w")
    close(r["d_b"], dy[u].sum(0), t, "d_b")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("n_rows,d", [(1, 8), (257, 20), (33, 1024)])
def test_newsvec_rows(n_rows, d, precision):
    from tests.test_hip_nrms_bert import TOL as BTOL
    lib = _lib.load()
    rng = np.random.default_rng(n_rows + d)
    table = (rng.standard_normal((n_rows, d)) * 0.5).astype(np.float32)
    w = (rng.uniform(-1, 1, (d, d)) * np.sqrt(3.0 / d)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, d).astype(np.float32)
    td, wd, bd = dev(table), dev(w), dev(b)
    prec = _lib.PRECISIONS[precision]
    need = int(lib.nrms_newsvec_rows_workspace_bytes(C.c_int64(n_rows), d, prec))
    assert need > 0

    def call(P, nbytes):
        return lib.nrms_newsvec_rows_fwd(C.c_int64(n_rows), d, prec, _lib.ptr(td), _lib.ptr(wd), _lib.ptr(bd), P["out"].ptr, P["workspace"].ptr,
                                         C.c_size_t(nbytes), _stream())

    def run(poison):
        P = Pool(poison)
        P.elems("out", n_rows * d), P.new("workspace", need)
        if poison == POISONS[0]:
            refuses_undersized(lambda n: call(P, n), P, need, "nrms_newsvec_rows_fwd")
        ok(call(P, need), "nrms_newsvec_rows_fwd")
        P.intact("nrms_newsvec_rows_fwd")
        return {"out": P["out"].numpy((n_rows, d))}

    r = three_poisons(run, "nrms_newsvec_rows_fwd")[POISONS[0]]
    ref = table.astype(np.float64) @ w.astype(np.float64).T + b
    assert float(np.abs(r["out"] - ref).max()) <= BTOL[precision]["score"] * max(1.0, float(np.abs(ref).max()))
