"""Host-side driver of the HIP hot path: owns the device buffers (via torch, which is only
plumbing here: allocator + streams) and issues the C-ABI calls of include/nrms_hip.h in the
order of one NRMS step.

Layout in HBM (all fp32, row-major):
  flat parameter buffer  [ table V*d | news: Wqkv 3d*d, bqkv 3d, Wa q*d, ba q, qv q | user: same ]
  flat gradient buffer   same layout (one RCCL all-reduce / one fused Adam pass over it)
  titles                 ids [N, L] int64, N = B*H history titles (user-major) then B*C candidates
  news vectors           [N, d]: rows [0, B*H) are the user-encoder input, rows [B*H, N) the candidates
  saved activations      qkv [M,3d], ctx [M,d], t [M,q], w [M] per encoder (M = sequences * length)
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass

import torch

from . import _lib
from .synth import ENCODERS


@dataclass(frozen=True)
class ModelDims:
    n_words: int
    word_embed_size: int
    num_attention_heads: int            # user-encoder heads (and news-encoder heads unless news_heads is set)
    query_vector_dim: int
    news_heads: int = 0                 # nrms_v1: config.title_heads_num for the news encoder
    output_proj: bool = False           # nrms_v1 topology: MHSA ends in output_linear (W_O)
    style: str = "v0"                   # parameter naming: "v0" (model/nrms_v0.py) or "v1" (model/nrms_v1.py)

    def heads(self, enc):
        return self.news_heads if (enc == "news_encoder" and self.news_heads) else self.num_attention_heads


def role_names(style: str, output_proj: bool):
    """Ordered (parameter name, encoder, role) triples; the order IS the flat-buffer order."""
    out = []
    if style == "v0":
        out.append(("news_encoder.word_embedding.0.weight", "news_encoder", "table"))
    else:
        out.append(("news_encoder.word_embedding.weight", "news_encoder", "table"))
    for enc in ENCODERS:
        if style == "v0":
            a = enc + ".multihead_self_attention."
            qkv = [a + "W_Q", a + "W_K", a + "W_V"]
            wo = a + "W_O"
            qv = enc + ".additive_attention.attention_query_vector"
        else:
            a = enc + ".multi_head_self_attention."
            qkv = [a + "linear_layers.%d" % i for i in range(3)]
            wo = a + "output_linear"
            qv = enc + ".additive_attention.query_vector"
        out += [(n + ".weight", enc, r) for n, r in zip(qkv, ("wq", "wk", "wv"))]
        out += [(n + ".bias", enc, r) for n, r in zip(qkv, ("bq", "bk", "bv"))]
        if output_proj:
            out += [(wo + ".weight", enc, "wo"), (wo + ".bias", enc, "bo")]
        out += [(enc + ".additive_attention.linear.weight", enc, "wa"),
                (enc + ".additive_attention.linear.bias", enc, "ba"), (qv, enc, "qv")]
    return out


def nrms_entries(dims: ModelDims):
    """The (name, shape, encoder, role) entries of v0 / v1 in flat-buffer order (role_names with their shapes)."""
    V, d, q = dims.n_words, dims.word_embed_size, dims.query_vector_dim
    if d % 4 or q % 4:
        raise ValueError("word_embed_size and query_vector_dim must be multiples of 4")
    shapes = {"table": (V, d), "wq": (d, d), "wk": (d, d), "wv": (d, d), "bq": (d,), "bk": (d,), "bv": (d,),
              "wo": (d, d), "bo": (d,), "wa": (q, d), "ba": (q,), "qv": (q,)}
    return [(name, shapes[role], enc, role) for name, enc, role in role_names(dims.style, dims.output_proj)]


class FlatLayout:
    """Offsets (in floats) of the reference-named tensors inside the flat buffer, from an ordered list of
    (name, shape, encoder, role) entries (encoder and role None for a tensor outside the encoder descriptors;
    default: nrms_entries(dims)).  The embedding table comes first; W_Q/W_K/W_V (and their biases) are adjacent
    so the kernels see one [3w, w] matrix."""

    def __init__(self, dims, entries=None):
        self.dims = dims
        self.entries, self.blocks, widths = {}, {}, {}
        off = 0
        for name, shape, enc, role in (nrms_entries(dims) if entries is None else entries):
            n = 1
            for x in shape:
                n *= x
            self.entries[name] = (off, tuple(shape), n)
            if enc is not None:
                self.blocks.setdefault(enc, {})[role] = off
                if role == "wq":
                    widths[enc] = shape[0]
            off += n
        self.total = off
        self.names = list(self.entries)
        for enc, w in widths.items():
            b = self.blocks[enc]
            assert b["wk"] == b["wq"] + w * w and b["wv"] == b["wq"] + 2 * w * w      # adjacency the kernels rely on
            assert b["bk"] == b["bq"] + w and b["bv"] == b["bq"] + 2 * w
        self.table = self.blocks["news_encoder"]["table"]
        assert self.table == 0, "the embedding table must be the first entry"

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        off, shp, n = self.entries[name]
        return flat[off:off + n].view(shp)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


MAX_TAGS = 512          # nrms_topk_dot_tagged / nrms_rank_dot_tagged: 1 <= n_tags <= 512
MAX_ADJUST = 256        # nrms_topk_dot_adjusted / nrms_rank_dot_adjusted: 0 <= n_adjust <= 256 (NRMS_ADJ_MAX)


def pack_tag_mask(allow):
    """allow bool [B, n_tags] -> int32 [B, ceil(n_tags / 32)], the packed sets nrms_topk_dot_tagged reads: tag t of user b is bit
    t & 31 of word [b, t >> 5] (bit 31 is the int32's sign bit); the bits past n_tags in the last word are zero.  Torch ops on
    allow's device, no host synchronisation."""
    if not torch.is_tensor(allow) or allow.dim() != 2 or allow.dtype != torch.bool:
        raise ValueError("pack_tag_mask: allow must be a bool [B, n_tags] tensor (got %s)"
                         % (("%s %s" % (tuple(allow.shape), allow.dtype)) if torch.is_tensor(allow) else type(allow).__name__))
    B, n_tags = allow.shape
    W = (n_tags + 31) // 32
    bits = torch.zeros(B, W * 32, dtype=torch.int64, device=allow.device)
    bits[:, :n_tags] = allow
    word = (bits.view(B, W, 32) << torch.arange(32, dtype=torch.int64, device=allow.device)).sum(dim=2)      # in [0, 2^32)
    return (word - ((word >> 31) << 32)).to(torch.int32)


def remaining_caps(cap, served_ids, item_tag, n_tags):
    """The caps of the next page of a capped request -> int32 [B, n_tags]: ``cap`` minus, per user and tag, the number of
    ``served_ids`` [B, K] (everything served on the pages so far; -1 is padding and ignored) that carry the tag, read off
    ``item_tag`` [N] by id.  cap: int [B, n_tags], or [n_tags] for every user.  Ids and tags are in one convention, the one the
    call that served them uses (catalogue rows with the engine, news ids with a model).  An id whose tag lies outside [0, n_tags)
    was never served and is ignored.  The result may go below zero where a caller counts more than the cap allowed: a cap <= 0
    closes the tag.  Torch ops on cap's device, no host synchronisation."""
    if not (torch.is_tensor(cap) and torch.is_tensor(served_ids) and torch.is_tensor(item_tag)):
        raise ValueError("remaining_caps: cap, served_ids and item_tag must be tensors")
    n_tags = int(n_tags)
    if served_ids.dim() != 2 or item_tag.dim() != 1 or cap.dim() not in (1, 2) or cap.shape[-1] != n_tags:
        raise ValueError("remaining_caps: cap must be [B, %d] or [%d], served_ids [B, K] and item_tag [N] (got %s, %s, %s)"
                         % (n_tags, n_tags, tuple(cap.shape), tuple(served_ids.shape), tuple(item_tag.shape)))
    B = served_ids.shape[0]
    if cap.dim() == 1:
        cap = cap.unsqueeze(0).expand(B, -1)
    if cap.shape[0] != B:
        raise ValueError("remaining_caps: cap has %d rows, served_ids %d" % (cap.shape[0], B))
    dev = cap.device
    ids = served_ids.to(dev, dtype=torch.int64)
    N = item_tag.shape[0]
    real = (ids >= 0) & (ids < N)
    tags = item_tag.to(dev, dtype=torch.int64)[ids.clamp(0, max(N - 1, 0))] if N else torch.zeros_like(ids)
    real = real & (tags >= 0) & (tags < n_tags)
    counts = torch.zeros(B, n_tags, dtype=torch.int64, device=dev)
    counts.scatter_add_(1, torch.where(real, tags, torch.zeros_like(tags)), real.to(torch.int64))
    return (cap.to(torch.int64) - counts).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous()


def impression_metrics(lib, device, scores, labels, lens, ks=(5, 10), ranks=False):
    """NRMSEngine.impression_metrics without an engine (evaluation.score_submission): ``lib`` is _lib.load()."""
    k_a, k_b = (int(k) for k in ks)
    n, cmax = scores.shape
    f64 = dict(dtype=torch.float64, device=device)
    out = dict(auc=torch.empty(n, **f64), mrr=torch.empty(n, **f64))
    nd_a, nd_b = torch.empty(n, **f64), torch.empty(n, **f64)
    rk = torch.empty(n, cmax, dtype=torch.int32, device=device) if ranks else None
    scores, labels, lens = scores.contiguous(), labels.contiguous(), lens.contiguous()
    rc = lib.nrms_impression_metrics(n, cmax, _lib.ptr(scores), _lib.ptr(labels), _lib.ptr(lens), k_a, k_b,
                                     _lib.ptr(out["auc"]), _lib.ptr(out["mrr"]), _lib.ptr(nd_a), _lib.ptr(nd_b),
                                     _lib.ptr(rk), _stream())
    _lib.check(rc, "nrms_impression_metrics")
    out["ndcg@%d" % k_a], out["ndcg@%d" % k_b] = nd_a, nd_b
    if ranks:
        out["ranks"] = rk
    return out


class PackedCatalogue:
    """What NRMSEngine.pack_catalogue returns and top_k_coarse reads: items [N, d] fp32, the rows it was made from (kept: the exact
    re-scoring reads them); items16 [N, pitch] int16, their fp16 bits (include/nrms_hip.h nrms_catalogue_pack_f16); stats [2] fp32
    on the device: the bounds NRM and ERR of the certificate.  source: (data_ptr, shape) of the tensor the caller named (for
    Model.pack_catalogue the whole catalogue, whose rows 1.. are ``items``), by which a stale pack is told."""

    def __init__(self, items, items16, stats, source=None):
        self.items, self.items16, self.stats = items, items16, stats
        self.source = source if source is not None else (items.data_ptr(), tuple(items.shape))

    @property
    def nbytes(self):
        return self.items16.numel() * 2


class NRMSEngine:
    """One NRMS forward / backward / optimizer step on one GPU."""

    def __init__(self, dims, device, precision="fp32", layout=None):
        self.lib = _lib.load()
        self.dims = dims
        self.set_precision(precision)
        self.layout = FlatLayout(dims) if layout is None else layout
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.NrmsError("the NRMS HIP engine needs a GPU device (got %s); there is no CPU path" % device)
        self._bufs = {}
        self._saved = None
        self._fuse_table_adam = os.environ.get("NRMS_NO_FUSED_TABLE_ADAM", "0") in ("", "0")
        self.fp16_user_encoder = False     # precision "fp16": the user encoder runs in bf16x3 unless this is set
        self.fp16_backward = True          # training in fp16 mode runs the fused fp16 backward (csrc/fused16_bwd.hip)
        self.loss_scale = 0.0              # fp16 backward: 0 = chosen on the device from max |dout| per call (nrms_hip.h)
        # precision "fp16", nrms_v1's W_O + wide-head news encoder on csrc/fused16_v1.hip: OPT-IN (config.fp16_v1_news_encoder).
        # Its scores sit up to 1.56e-4 from fp32 on a 512-user batch (2 % of them beyond north_star's absolute 1e-4),
        # so the default keeps v1's news encoder in bf16x3 (1e-6)
        self.fp16_wide_heads = False
        # precision "fp16": passes that keep nothing for a backward (evaluate / test, get_news_vector, forward under no_grad) run
        # in bf16x3 unless this is set (config.fp16_inference): evaluation scores then sit ~1e-6 from the reference and the
        # per-impression AUC cannot move by rank flips of near-tied candidates (round 3 measured 1.4e-4 on 1 024 impressions)
        self.fp16_inference = False
        # the user encoder's bf16x3 passes (33..64-slot histories, d <= 300, heads <= 32 wide, no mask / W_O) as ONE kernel per
        # direction (csrc/user64.hip, NRMS_FLAG_FUSED_SEQ64) instead of the GEMM -> attention -> additive chain; False = the chain
        self.fused_user_encoder = True
        self.fp16_wide_heads_backward = True    # ... its training step too (csrc/fused16_v1_bwd.hip); False: training in bf16x3
        self._gen = 0                      # generation stamp of _saved (checked by the autograd backward)
        # out-of-range word ids: counted on the device by nrms_sanitize_ids, surfaced without a host sync
        # (the count is copied to pinned memory behind the kernel and looked at on a later call)
        self._bad_ids = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._bad_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._bad_event = None
        self._news_cache = None
        # fp16 backward: non-finite gradient elements (an overflow of the loss-scaled fp16 tensors) are skipped and counted on
        # the device by the guarded optimizer / grad_guard; the count reaches the host asynchronously (like the id check) and
        # lowers the loss scale for the following steps: desc.loss_scale = -loss_scale_backoff (include/nrms_hip.h)
        self._grad_bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._grad_bad_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._grad_bad_event = None
        self.loss_scale_backoff = 0        # extra powers of two of head room below the default [64, 128) target
        self.grad_overflow_steps = 0       # steps whose gradient held non-finite elements (seen so far)
        self._clean_polls = 0

    FP16_LIMITS = dict(seq_len=64, d_model=316, d_k=32, n_heads=10, q_dim=224)

    def _fp16_ok(self, enc, seq_len, mask_mode, training):
        """The fused fp16 kernels cover the shapes of include/nrms_hip.h (NRMS_PRECISION_FP16); an encoder pass
        outside them runs in bf16x3 instead.  So does the user encoder unless fp16_user_encoder is set: it is 3 % of
        the flops, and with it in split-bf16 (~2^-16 relative) the scores keep a margin inside north_star's 1e-4
        and the user encoder's additive-attention gradients (cancelling sums) are no longer fp16 noise."""
        d, L = self.dims, self.FP16_LIMITS
        h = d.heads(enc)
        if enc == "user_encoder" and not self.fp16_user_encoder:
            return False
        if not training and not self.fp16_inference:
            return False
        if d.word_embed_size % h:
            return False
        if d.output_proj:
            # nrms_v1's news encoder (heads of 33..50 columns + W_O): csrc/fused16_v1.hip, padding-skipping path only
            dk = d.word_embed_size // h
            return (enc == "news_encoder" and self.fp16_wide_heads and self.pad_row_zero and not mask_mode
                    and seq_len <= 32 and d.word_embed_size <= L["d_model"] and d.word_embed_size % 10 == 0
                    and d.word_embed_size // 10 <= 32 and 32 < dk <= 50 and 3 * h + 1 <= 19 and h * max(dk - 48, 0) <= 16
                    and d.query_vector_dim <= L["q_dim"] and (not training or self.fp16_wide_heads_backward))
        return (seq_len <= L["seq_len"] and d.word_embed_size <= L["d_model"] and h <= L["n_heads"]
                and d.word_embed_size // h <= L["d_k"] and d.query_vector_dim <= L["q_dim"]
                and not d.output_proj and not mask_mode and (not training or self.fp16_backward))

    def set_precision(self, precision):
        """"fp32" (exact f32 MFMA), "bf16x3" (split-bf16 projections, ~2^-16 relative), "bf16", or "fp16"
        (fused one-wave-per-sequence kernels on fp16 MFMA, fp16 activations -- v0's news encoder and, with output_proj, nrms_v1's
        six-heads-of-50 + W_O news encoder; bf16x3 where a shape, a mask or the user encoder is outside them)."""
        if precision not in _lib.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(_lib.PRECISIONS))
        self.precision = precision
        # NRMS_FLAG_PAD_ROW_ZERO: set by the owner of the parameters when embedding row 0 is all zeros
        # (include/nrms_hip.h); False = dense path
        self.pad_row_zero = False

    # ---- buffers ----------------------------------------------------------------------
    def _buf(self, key, numel, dtype=torch.float32):
        t = self._bufs.get(key)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.empty(max(int(numel), 1), dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t

    def _desc(self, enc, n_seq, seq_len, p_embed=0.0, p_ctx=0.0, seed=0, mask_mode=0, training=False):
        d = self.dims
        prec = self.precision
        if prec == "fp16" and not self._fp16_ok(enc, seq_len, mask_mode, training):
            prec = "bf16x3"
        flags = _lib.NRMS_FLAG_PAD_ROW_ZERO if (self.pad_row_zero and enc == "news_encoder") else 0
        h = d.heads(enc)
        if (enc == "user_encoder" and self.fused_user_encoder and prec == "bf16x3" and not d.output_proj and not mask_mode
                and 32 < seq_len <= 64 and d.word_embed_size <= 300 and d.word_embed_size % h == 0
                and (d.word_embed_size // h) <= 32 and (d.word_embed_size // h) % 2 == 0 and h <= 10 and d.query_vector_dim <= 224):
            flags |= _lib.NRMS_FLAG_FUSED_SEQ64
        return _lib.EncoderDesc(n_seq=n_seq, seq_len=seq_len, d_model=d.word_embed_size, n_heads=h,
                                q_dim=d.query_vector_dim, vocab=d.n_words if enc == "news_encoder" else 0,
                                p_drop_embed=float(p_embed), p_drop_ctx=float(p_ctx),
                                precision=_lib.PRECISIONS[prec], use_output_proj=int(d.output_proj),
                                mask_mode=int(mask_mode),
                                flags=flags,
                                seed=int(seed), loss_scale=float(self.loss_scale), p_drop_attn=0.0)

    def _ptrs(self, cls, flat, enc):
        b = self.layout.blocks[enc]
        base = flat.data_ptr()
        p = lambda role: (base + 4 * b[role]) if role in b else None
        return cls(table=p("table"), w_qkv=p("wq"), b_qkv=p("bq"), w_o=p("wo"), b_o=p("bo"), w_add=p("wa"),
                   b_add=p("ba"), q_vec=p("qv"))

    def _weights(self, flat, enc):
        return self._ptrs(_lib.EncoderWeights, flat, enc)

    def _grads(self, gflat, enc):
        return self._ptrs(_lib.EncoderGrads, gflat, enc)

    def _acts(self, tag, M, need_bwd, gather=False, desc=None):
        d, q = self.dims.word_embed_size, self.dims.query_vector_dim
        if desc is not None and desc.precision == _lib.NRMS_PRECISION_FP16:
            # fp16 activations with padded pitches (include/nrms_hip.h, nrms_encoder_acts)
            KP, DP, QP = _lib.NRMS_FP16_KP, _lib.NRMS_FP16_DP, _lib.NRMS_FP16_QP
            h = torch.float16
            x = self._buf(tag + ".x16", (M + 1) * KP, h)          # + the padding token's row
            Mp = desc.n_seq * (32 if desc.seq_len <= 32 else 64)      # whole 32-row blocks per sequence
            ctx = self._buf(tag + ".ctx16", Mp * DP, h)
            t = self._buf(tag + ".t16", Mp * QP, h) if need_bwd else None
            w = self._buf(tag + ".w", M) if need_bwd else None
            nbytes = int(self.lib.nrms_encoder_fwd_scratch_bytes(C.byref(desc)))
            # one scratch per tag: a training forward's token / title lists stay untouched until its backward reads them
            # (NRMS_FLAG_FWD_SCRATCH_KEPT), whatever inference or user-encoder passes run in between
            scratch = self._buf(tag + ".scratch16", (nbytes + 3) // 4)
            attn = self._buf(tag + ".attn16", Mp * DP, h) if desc.use_output_proj else None   # head concatenation (fused16_v1.hip)
            dp = lambda z: None if z is None else z.data_ptr()
            return _lib.EncoderActs(x=dp(x), qkv=None, attn=dp(attn), ctx=dp(ctx), t=dp(t), w=dp(w), scratch=dp(scratch))
        x = self._buf(tag + ".x", M * d) if gather else None
        if desc is not None and desc.flags & _lib.NRMS_FLAG_FUSED_SEQ64:
            # acts.qkv = operand fragments of the fused user-encoder kernels (include/nrms_hip.h, NRMS_FLAG_FUSED_SEQ64)
            nb = int(self.lib.nrms_encoder_fused_qkv_bytes(C.byref(desc)))
            qkv = self._buf(tag + ".qkvf", (nb + 3) // 4)
            ctx = self._buf(tag + ".ctx", M * d) if need_bwd else None
            t = self._buf(tag + ".t", M * q) if need_bwd else None
            w = self._buf(tag + ".w", M) if need_bwd else None
            ns = int(self.lib.nrms_encoder_fwd_scratch_bytes(C.byref(desc)))
            scratch = self._buf("fwd_scratch64", (ns + 3) // 4)
            dp = lambda z: None if z is None else z.data_ptr()
            return _lib.EncoderActs(x=None, qkv=dp(qkv), attn=None, ctx=dp(ctx), t=dp(t), w=dp(w), scratch=dp(scratch))
        qkv = self._buf(tag + ".qkv", M * 3 * d)
        attn = self._buf(tag + ".attn", M * d) if self.dims.output_proj else None
        ctx = self._buf(tag + ".ctx", M * d)
        t = self._buf(tag + ".t", M * q) if need_bwd else None
        w = self._buf(tag + ".w", M) if need_bwd else None
        # head-major W_qkv / b_qkv copies + bf16 weight planes: an upper bound of nrms_encoder_fwd_scratch_bytes
        scratch = self._buf("fwd_scratch", 3 * d * d + 3 * d + 256 + (3 * d + 32) * (d + 32) + (M + M // 1024 + 512 if gather else 0))
        dp = lambda z: None if z is None else z.data_ptr()
        return _lib.EncoderActs(x=dp(x), qkv=dp(qkv), attn=dp(attn), ctx=dp(ctx), t=dp(t), w=dp(w), scratch=dp(scratch))

    # ---- word-id validation (nn.Embedding raises on an out-of-range index; here: device-side, deferred) ----
    def sanitize_ids(self, src, dst):
        """dst = src with ids outside [0, n_words) replaced by the padding id 0 (so no kernel can index out of
        bounds), counting them on the device.  The count reaches the host asynchronously: poll_ids() on a later
        call, or check_ids() (synchronises), raises NrmsError."""
        n = src.numel()
        if n == 0:
            return dst
        fn = self.lib.nrms_sanitize_ids_i32 if src.dtype == torch.int32 else self.lib.nrms_sanitize_ids
        rc = fn(_lib.ptr(src), _lib.ptr(dst), C.c_int64(n), int(self.dims.n_words), _lib.ptr(self._bad_ids), _stream())
        _lib.check(rc, "nrms_sanitize_ids")
        self._bad_host.copy_(self._bad_ids, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._bad_event = ev
        return dst

    def note_bad_ids(self):
        """After nrms_sanitize_ids calls made outside sanitize_ids (category tables): their count reaches the host as
        sanitize_ids' does, for poll_ids / check_ids."""
        self._bad_host.copy_(self._bad_ids, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._bad_event = ev

    def _raise_bad_ids(self):
        n = int(self._bad_host.item())
        if n:
            self._bad_ids.zero_()
            self._bad_host.zero_()
            raise _lib.NrmsError("%d word id(s) outside [0, %d) reached the embedding gather (treated as the padding "
                                 "id on the device; the vocabulary and the embedding table disagree)" % (n, self.dims.n_words))

    def poll_ids(self):
        """Non-blocking: raises if an earlier call's id check has completed and found out-of-range ids."""
        if self._bad_event is not None and self._bad_event.query():
            self._bad_event = None
            self._raise_bad_ids()

    def check_ids(self):
        """Blocking form of poll_ids(): waits for the pending id checks."""
        if self._bad_event is not None:
            self._bad_event.synchronize()
            self._bad_event = None
        self._raise_bad_ids()

    # ---- news vectors for an arbitrary list of titles (a-5, a-9 get_news_vector) ---------
    def encode_titles(self, flat, ids, out=None, p_embed=0.0, p_ctx=0.0, seed=0, save=False, tag=None,
                      chunk_titles=32768, mask=None, mask_mode=0, trusted_ids=False):
        """ids [N, L] int64 on the device -> news vectors [N, d].  With save=True (training) the
        activations are kept for the backward and the call is not chunked.  mask [N, L] uint8 with
        mask_mode bits (1 = attention pairs, 2 = pooling) gives nrms_v1's masked primitives."""
        N, L = ids.shape
        d = self.dims.word_embed_size
        if tag is None:
            tag = "news" if save else "news_eval"
        if out is None:
            out = torch.empty(N, d, dtype=torch.float32, device=self.device)
        if trusted_ids:
            ids = ids.contiguous()
        else:
            self.poll_ids()
            ids = self.sanitize_ids(ids.contiguous(), self._buf(tag + ".ids", N * L, torch.int64)[:N * L].view(N, L))
        if mask is not None:
            mask = mask.contiguous()
        w = self._weights(flat, "news_encoder")
        step = N if save else min(N, chunk_titles)
        for s0 in range(0, N, max(step, 1)):
            n = min(step, N - s0)
            desc = self._desc("news_encoder", n, L, p_embed, p_ctx, seed, mask_mode if mask is not None else 0, training=save)
            acts = self._acts(tag, n * L, save, gather=True, desc=desc)
            mp = None if mask is None else C.c_void_p(mask[s0:].data_ptr())
            rc = self.lib.nrms_encoder_fwd(C.byref(desc), C.byref(w), C.c_void_p(ids[s0:].data_ptr()), None, mp,
                                           C.byref(acts), C.c_void_p(out[s0:].data_ptr()), _stream())
            _lib.check(rc, "nrms_encoder_fwd(news)")
        return out

    def encode_users(self, flat, news_vectors, out=None, save=False, tag=None, mask=None, mask_mode=0):
        """news_vectors [B, H, d] -> user vectors [B, d] (a-6, a-9 get_user_vector)."""
        B, H, d = news_vectors.shape
        if tag is None:
            tag = "user" if save else "user_eval"
        if out is None:
            out = torch.empty(B, d, dtype=torch.float32, device=self.device)
        w = self._weights(flat, "user_encoder")
        desc = self._desc("user_encoder", B, H, mask_mode=mask_mode if mask is not None else 0, training=save)
        acts = self._acts(tag, B * H, save, desc=desc)
        rc = self.lib.nrms_encoder_fwd(C.byref(desc), C.byref(w), None, C.c_void_p(news_vectors.data_ptr()),
                                       _lib.ptr(None if mask is None else mask.contiguous()), C.byref(acts),
                                       C.c_void_p(out.data_ptr()), _stream())
        _lib.check(rc, "nrms_encoder_fwd(user)")
        return out

    def _parts_of(self, tag, B, H, d):
        """Copies of what the tag's last user-encoder pass left in acts.ctx / acts.w: (ctx [B, H, d], w [B, H])."""
        M = B * H
        return self._bufs[tag + ".ctx"][:M * d].view(B, H, d).clone(), self._bufs[tag + ".w"][:M].view(B, H).clone()

    def user_parts(self, flat, news_vectors, mask=None, mask_mode=0):
        """news_vectors [B, H, d] -> (user [B, d], ctx [B, H, d], w [B, H]): an inference pass of the user encoder (evaluation
        precision, no dropout) that also hands out the two factors of its pooling sum, user[b] = sum_h w[b, h] ctx[b, h]
        (nrms_encoder_acts.ctx and .w; the input of `attribution`).  It is the pass encode_users runs for this shape, the fused
        one-kernel pass included, which stores ctx and w row-major like the chain: `user` has encode_users' bits.  (Only an fp16
        user encoder, whose activations are fp16 with padded pitches, is replaced by the bf16x3 pass here.)  The buffers are the
        tag "user_parts"'s own: neither a training forward's saved activations nor user_eval's are touched."""
        B, H, d = news_vectors.shape
        tag = "user_parts"
        out = torch.empty(B, d, dtype=torch.float32, device=self.device)
        wts = self._weights(flat, "user_encoder")
        desc = self._desc("user_encoder", B, H, mask_mode=mask_mode if mask is not None else 0, training=False)
        if desc.precision == _lib.NRMS_PRECISION_FP16:
            desc.precision = _lib.PRECISIONS["bf16x3"]
        acts = self._acts(tag, B * H, True, desc=desc)
        rc = self.lib.nrms_encoder_fwd(C.byref(desc), C.byref(wts), None, C.c_void_p(news_vectors.data_ptr()),
                                       _lib.ptr(None if mask is None else mask.contiguous()), C.byref(acts),
                                       C.c_void_p(out.data_ptr()), _stream())
        _lib.check(rc, "nrms_encoder_fwd(user parts)")
        return (out,) + self._parts_of(tag, B, H, d)

    def click_scores(self, cand_vec, user_vec, cand_mask=None, out=None):
        B, Cn, d = cand_vec.shape
        if out is None:
            out = torch.empty(B, Cn, dtype=torch.float32, device=self.device)
        rc = self.lib.nrms_click_score_fwd(B, Cn, d, _lib.ptr(cand_vec), _lib.ptr(user_vec), _lib.ptr(cand_mask),
                                           _lib.ptr(out), _stream())
        _lib.check(rc, "nrms_click_score_fwd")
        return out

    # ---- full model forward (a-8) -------------------------------------------------------
    def forward(self, flat, hist_ids, cand_ids, cand_mask, training, p_drop=0.0, seed=0, user_mask=None,
                user_mask_mode=0):
        """hist_ids [B,H,L], cand_ids [B,C,L] int64 and cand_mask [B,C] uint8 (or None) on the
        device -> scores [B,C].  training=True keeps what backward() needs; p_drop is applied as given
        (the caller passes 0 in eval mode; a train-mode forward under no_grad still drops, as nn.Dropout does)."""
        B, H, L = hist_ids.shape
        Cn = cand_ids.shape[1]
        d = self.dims.word_embed_size
        N = B * (H + Cn)
        # training activations and inference scratch live under different tags: an inference call (get_news_vector,
        # an eval forward) between a training forward and its backward must not overwrite what the backward reads
        sfx = "" if training else "_eval"
        self.poll_ids()
        ids = self._buf("ids" + sfx, N * L, torch.int64)[:N * L].view(N, L)
        self.sanitize_ids(hist_ids.reshape(B * H, L).contiguous(), ids[:B * H])
        self.sanitize_ids(cand_ids.reshape(B * Cn, L).contiguous(), ids[B * H:])
        nv = self._buf("news_vec" + sfx, N * d)[:N * d].view(N, d)
        p = float(p_drop)
        p_embed = 0.0 if self.dims.style == "v1" else p        # nrms_v1 has no embedding dropout (nrms_v1.py:159-161)
        self.encode_titles(flat, ids, out=nv, p_embed=p_embed, p_ctx=p, seed=seed, save=training, tag="news" + sfx,
                           trusted_ids=True)
        hist = nv[:B * H].view(B, H, d)
        cand = nv[B * H:].view(B, Cn, d)
        user = self._buf("user_vec" + sfx, B * d)[:B * d].view(B, d)
        self.encode_users(flat, hist, out=user, save=training, tag="user" + sfx, mask=user_mask, mask_mode=user_mask_mode)
        if cand_mask is not None:
            cand_mask = cand_mask.contiguous()
        scores = torch.empty(B, Cn, dtype=torch.float32, device=self.device)
        self.click_scores(cand, user, cand_mask, out=scores)
        if training:
            self._gen += 1
            self._saved = dict(B=B, H=H, C=Cn, L=L, ids=ids, nv=nv, user=user, mask=cand_mask, p=p, p_embed=p_embed,
                               seed=seed, user_mask=user_mask, user_mask_mode=user_mask_mode if user_mask is not None else 0,
                               gen=self._gen)
        return scores

    def ce_loss(self, scores, grad_scale=None, want_grad=True):
        """Sum over the batch of -log_softmax(scores)[:,0] (device scalar) and, optionally,
        dscores = (softmax - onehot0) * grad_scale."""
        B, Cn = scores.shape
        loss_sum = torch.zeros(1, dtype=torch.float32, device=self.device)
        dscores = torch.empty_like(scores) if want_grad else None
        gs = (1.0 / B) if grad_scale is None else grad_scale
        rc = self.lib.nrms_ce_loss_fwd_bwd(B, Cn, _lib.ptr(scores), _lib.ptr(loss_sum), _lib.ptr(dscores),
                                           C.c_float(gs), _stream())
        _lib.check(rc, "nrms_ce_loss_fwd_bwd")
        return loss_sum, dscores

    def _bwd_workspace(self, *descs):
        nbytes = max(self.lib.nrms_encoder_bwd_workspace_bytes(C.byref(d)) for d in descs)
        return self._buf("bwd_ws", (nbytes + 3) // 4)

    def encode_users_backward(self, flat, gflat, news_vectors, dout, dx=None, tag="user", mask=None, mask_mode=0,
                              defer_join=False):
        """Backward of encode_users(save=True): accumulates the user-encoder parameter gradients into
        gflat and returns d(news_vectors) [B, H, d].

        defer_join (Engine.backward only): NRMS_FLAG_DEFER_USER_JOIN -- the weight-gradient GEMMs are still running on a helper
        stream when this returns (d(news_vectors) is complete in stream order); the fp16 news-encoder backward that follows
        joins them, or join_backward().  Their inputs then live in a workspace of this call's own, not in the shared one."""
        B, H, d = news_vectors.shape
        if dx is None:
            dx = torch.empty(B * H, d, dtype=torch.float32, device=self.device)
        desc = self._desc("user_encoder", B, H, mask_mode=mask_mode if mask is not None else 0, training=True)
        if defer_join and desc.precision != _lib.NRMS_PRECISION_FP16:
            desc.flags |= _lib.NRMS_FLAG_DEFER_USER_JOIN
            nbytes = self.lib.nrms_encoder_bwd_workspace_bytes(C.byref(desc))
            ws = self._buf("bwd_ws_user", (nbytes + 3) // 4)
        else:
            ws = self._bwd_workspace(desc)
        w, g = self._weights(flat, "user_encoder"), self._grads(gflat, "user_encoder")
        acts = self._acts(tag, B * H, True, desc=desc)
        rc = self.lib.nrms_encoder_bwd(C.byref(desc), C.byref(w), None, _lib.ptr(news_vectors),
                                       _lib.ptr(None if mask is None else mask.contiguous()), C.byref(acts),
                                       _lib.ptr(dout.contiguous()), C.byref(g), _lib.ptr(dx), _lib.ptr(ws),
                                       C.c_size_t(ws.numel() * 4), _stream())
        _lib.check(rc, "nrms_encoder_bwd(user)")
        return dx[:B * H].view(B, H, d)

    def join_backward(self):
        """Order the current stream behind whatever an earlier backward left on the library's helper streams."""
        _lib.check(self.lib.nrms_encoder_join(_stream()), "nrms_encoder_join")

    # ---- the scoring head's backward, shared by every engine whose candidate vectors are the tail of a [B*(H+C), width] buffer ----
    POOLED_VEC = ("nv", "d_news_vec")      # (key of that buffer in _saved, name of its gradient buffer); NamlEngine: feat / d_feat

    def _head_buffers(self, sv, width):
        """(cand [B*C, width], user [B, width], d(vectors) [B*(H+C), width], d(user) [B, width]) of the saved training forward."""
        B, H, Cn = sv["B"], sv["H"], sv["C"]
        N = B * (H + Cn)
        key, dkey = self.POOLED_VEC
        dvec = self._buf(dkey, N * width)[:N * width].view(N, width)
        duser = self._buf("d_user_vec", B * width)[:B * width].view(B, width)
        return sv[key][B * H:], sv["user"], dvec, duser

    def _head_backward(self, dscores, gen, width):
        """The front of every backward(): the saved forward (checked against ``gen``) and d(candidate vectors) -- the tail of the
        returned d(vectors) buffer -- and d(user vectors): from dscores [B, C] through nrms_click_score_bwd, or, with dscores None,
        what pooled_ce_loss() left there for this forward.  -> (saved, d(vectors), d(user))."""
        sv = self._saved
        if sv is None:
            raise _lib.NrmsError("backward() without a training forward()")
        if gen is not None and gen != sv["gen"]:
            raise _lib.NrmsError("backward() for training forward #%d, but the saved activations belong to forward #%d: "
                                 "a later training forward replaced them (one forward/backward pair at a time)" % (gen, sv["gen"]))
        B, H, Cn = sv["B"], sv["H"], sv["C"]
        cand, user, dvec, duser = self._head_buffers(sv, width)
        if dscores is None:
            if getattr(self, "_pooled_gen", None) != sv["gen"]:
                raise _lib.NrmsError("backward(dscores=None) needs the gradients of pooled_ce_loss(), and none was computed for "
                                     "training forward #%d" % sv["gen"])
        else:
            rc = self.lib.nrms_click_score_bwd(B, Cn, width, _lib.ptr(cand), _lib.ptr(user), _lib.ptr(sv["mask"]),
                                               _lib.ptr(dscores.contiguous()), C.c_void_p(dvec[B * H:].data_ptr()), _lib.ptr(duser),
                                               _stream())
            _lib.check(rc, "nrms_click_score_bwd")
        return sv, dvec, duser

    def pooled_ce_loss(self, cand_ids, reject=None, col_bias=None, grad_scale=None, want_grad=True):
        """In-batch sampled softmax of the saved training forward (nrms_pooled_ce_fwd_bwd, include/nrms_hip.h): every user against
        the B*C candidate vectors of the whole batch.  cand_ids [B, C] int64 news ids of the candidate slots; reject [B, R] int64
        or None: ids that are no negatives for that user (0 = padding); col_bias [B, C] fp32 or None, added to the scores of a
        column (the logQ correction: -log q).  Returns the loss sum over the batch (device scalar).  With want_grad the gradients
        land where backward(dscores=None) reads them; the pair count of the call is kept in ``pooled_pairs`` (device int64)."""
        sv = self._saved
        if sv is None:
            raise _lib.NrmsError("pooled_ce_loss() without a training forward()")
        B, Cn = sv["B"], sv["C"]
        key, _ = self.POOLED_VEC
        width = sv[key].shape[1]
        cand, user, dvec, duser = self._head_buffers(sv, width)
        dev = self.device
        ids = torch.as_tensor(cand_ids).to(dev, torch.int64).contiguous()
        if ids.numel() != B * Cn:
            raise _lib.NrmsError("pooled_ce_loss: cand_ids must be [%d, %d] (got %s)" % (B, Cn, tuple(ids.shape)))
        R = 0
        if reject is not None:
            reject = torch.as_tensor(reject).to(dev, torch.int64).contiguous()
            if reject.dim() != 2 or reject.shape[0] != B:
                raise _lib.NrmsError("pooled_ce_loss: reject must be [%d, R] (got %s)" % (B, tuple(reject.shape)))
            R = reject.shape[1]
            if R == 0:
                reject = None
        if col_bias is not None:
            col_bias = torch.as_tensor(col_bias).to(dev, torch.float32).contiguous()
            if col_bias.numel() != B * Cn:
                raise _lib.NrmsError("pooled_ce_loss: col_bias must be [%d, %d] (got %s)" % (B, Cn, tuple(col_bias.shape)))
        nbytes = self.lib.nrms_pooled_ce_workspace_bytes(B, Cn, width, R)
        if nbytes == 0:
            raise _lib.NrmsError("pooled_ce_loss: arguments rejected (B=%d, C=%d, d=%d, R=%d; B <= 4096, C <= 64, B*C <= 32768, "
                                 "d <= 1024, R <= 256)" % (B, Cn, width, R))
        ws = self._buf("pooled_ce_ws", (nbytes + 3) // 4)
        loss_sum = torch.zeros(1, dtype=torch.float32, device=dev)
        self.pooled_pairs = torch.zeros(1, dtype=torch.int64, device=dev)
        gs = (1.0 / B) if grad_scale is None else grad_scale
        H = sv["H"]
        rc = self.lib.nrms_pooled_ce_fwd_bwd(B, Cn, width, R, _lib.ptr(cand), _lib.ptr(user), _lib.ptr(ids), _lib.ptr(sv["mask"]),
                                             _lib.ptr(reject), _lib.ptr(col_bias), C.c_float(gs), _lib.ptr(loss_sum),
                                             C.c_void_p(dvec[B * H:].data_ptr()) if want_grad else None,
                                             _lib.ptr(duser) if want_grad else None, _lib.ptr(self.pooled_pairs), _lib.ptr(ws),
                                             C.c_size_t(ws.numel() * 4), _stream())
        _lib.check(rc, "nrms_pooled_ce_fwd_bwd")
        if want_grad:
            self._pooled_gen = sv["gen"]
        return loss_sum

    # ---- full model backward ------------------------------------------------------------
    # Exactly one table scatter feeds the word-embedding table in a step of THIS class's backward().  A subclass does not inherit
    # the claim: it is False there unless the subclass states it itself.
    single_table_scatter = True

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        if "single_table_scatter" not in cls.__dict__:
            cls.single_table_scatter = False

    def fuses_table_adam(self):
        """True when the saved training forward's backward can update the word-embedding table inside its scatter kernel
        (NRMS_FLAG_TABLE_ADAM, include/nrms_hip.h): exactly ONE table scatter feeds the table in a step -- the class says so
        (single_table_scatter; subclasses such as nrms_naml's engine, with its title and abstract passes, default to False and keep
        the separate optimizer) -- and that scatter is the grouped one.  NRMS_NO_FUSED_TABLE_ADAM=1 (read when the engine is
        built) forces the separate path."""
        sv = self._saved
        if (sv is None or not type(self).single_table_scatter or type(self).backward is not NRMSEngine.backward
                or not self._fuse_table_adam or os.environ.get("NRMS_ATOMIC_SCATTER") is not None):
            return False
        # (the fp16 news encoder scatters dense rows with atomics unless the padding row is zero; every other precision groups)
        return (self.pad_row_zero or self.precision != "fp16"
                or not self._fp16_ok("news_encoder", sv["L"], 0, True))

    def backward(self, flat, gflat, dscores=None, table_grad_ready=None, gen=None, table_adam=None):
        """Accumulates d(loss)/d(params) into gflat (same layout as flat) given dscores [B,C]; dscores None: the gradient of the
        pooled loss that pooled_ce_loss() computed for this training forward (NrmsError if it did not).
        gen: the generation stamp of the training forward this backward belongs to (saved activations are one
        slot: a later training forward replaces them, and a backward for the earlier one must not run on them).

        table_grad_ready: optional callable invoked as soon as the embedding-table gradient (95 % of the
        gradient bytes) is complete on the stream; the news encoder's d(W_qkv) GEMM is then deferred behind
        it (NRMS_FLAG_DEFER_WQKV) so that a data-parallel caller can start the table all-reduce underneath.

        table_adam: dict(m, v, step, lr, betas, eps[, guard]) -- only where fuses_table_adam() holds and without
        table_grad_ready: the news encoder's scatter kernel applies this Adam step to the table rows (NRMS_FLAG_TABLE_ADAM);
        the table region of gflat is then written, not accumulated, and the caller steps the other parameters with
        adam_step(..., rest=True)."""
        d = self.dims.word_embed_size
        sv, dnv, duser = self._head_backward(dscores, gen, d)
        B, H, Cn, L = sv["B"], sv["H"], sv["C"], sv["L"]
        N = B * (H + Cn)
        # fp16 mode: the loss scale is derived on the device from the gradient each encoder receives (any loss reduction,
        # batch size or world size); a fixed value only for experiments (tools/fp16_grad_stats.py)
        self.poll_grad_overflow()
        self.loss_scale = float(getattr(self, "loss_scale_override", None) or -float(self.loss_scale_backoff))
        nv = sv["nv"]
        hist = nv[:B * H]
        # user encoder: its input gradient lands directly in the history rows of d(news vectors)
        desc_u = self._desc("user_encoder", B, H, mask_mode=sv["user_mask_mode"], training=True)
        desc_n = self._desc("news_encoder", N, L, sv["p_embed"], sv["p"], sv["seed"], training=True)
        ws = self._bwd_workspace(desc_u, desc_n)
        # the user encoder's weight gradients feed nothing before the optimizer: where the fp16 news backward follows (it joins
        # them at its end) they stay on their helper stream, reading a workspace of their own (the news backward overwrites `ws`)
        defer_user = desc_n.precision == _lib.NRMS_PRECISION_FP16 and not self.dims.output_proj
        self.encode_users_backward(flat, gflat, hist.view(B, H, d), duser, dx=dnv, tag="user", mask=sv["user_mask"],
                                   mask_mode=sv["user_mask_mode"], defer_join=defer_user)
        wn, gn = self._weights(flat, "news_encoder"), self._grads(gflat, "news_encoder")
        acts_n = self._acts("news", N * L, True, gather=True, desc=desc_n)
        if desc_n.precision == _lib.NRMS_PRECISION_FP16:
            desc_n.flags |= _lib.NRMS_FLAG_FWD_SCRATCH_KEPT     # acts_n.scratch is this step's forward scratch (its own buffer)
        if table_grad_ready is not None:
            desc_n.flags |= _lib.NRMS_FLAG_DEFER_WQKV
        ta = None
        if table_adam is not None:
            if (table_grad_ready is not None or type(self).backward is not NRMSEngine.backward
                    or (desc_n.precision == _lib.NRMS_PRECISION_FP16 and not desc_n.flags & _lib.NRMS_FLAG_PAD_ROW_ZERO)):
                raise _lib.NrmsError("backward(table_adam=...) needs fuses_table_adam() and no table_grad_ready")
            lo, _, n_table = self.layout.entries[self.layout.names[0]]
            if lo != 0 or wn.table != flat.data_ptr():
                raise _lib.NrmsError("backward(table_adam=...): the word-embedding table must open the flat buffer")
            guard = table_adam.get("guard")
            guard = self.precision == "fp16" if guard is None else guard
            betas = table_adam.get("betas", (0.9, 0.999))
            ta = _lib.TableAdam(param=flat.data_ptr(), exp_avg=table_adam["m"].data_ptr(), exp_avg_sq=table_adam["v"].data_ptr(),
                                lr=float(table_adam["lr"]), beta1=float(betas[0]), beta2=float(betas[1]),
                                eps=float(table_adam.get("eps", 1e-8)), step=int(table_adam["step"]),
                                grad_scale=float(table_adam.get("grad_scale", 1.0)),
                                n_nonfinite=self._grad_bad.data_ptr() if guard else None)
            desc_n.flags |= _lib.NRMS_FLAG_TABLE_ADAM
        rc_join = 0
        try:
            rc = self.lib.nrms_encoder_bwd_adam(C.byref(desc_n), C.byref(wn), _lib.ptr(sv["ids"]), None, None, C.byref(acts_n),
                                                _lib.ptr(dnv), C.byref(gn), None, _lib.ptr(ws),
                                                C.c_size_t(ws.numel() * 4), None if ta is None else C.byref(ta), _stream())
            _lib.check(rc, "nrms_encoder_bwd(news)")
            if table_grad_ready is not None:
                table_grad_ready()
                rc = self.lib.nrms_encoder_bwd_wqkv(C.byref(desc_n), _lib.ptr(sv["ids"]), None, C.byref(acts_n), C.byref(gn),
                                                    _lib.ptr(ws), C.c_size_t(ws.numel() * 4), _stream())
                _lib.check(rc, "nrms_encoder_bwd_wqkv(news)")
        finally:
            if defer_user:      # joined already unless the news backward failed or had no title to run on: a no-op then
                rc_join = self.lib.nrms_encoder_join(_stream())
        _lib.check(rc_join, "nrms_encoder_join")

    def adam_step(self, flat, gflat, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                  grad_scale=1.0, guard=None, rest=False):
        """torch.optim.Adam's update on flat buffers.  guard (default: on in the fp16 mode): elements with a non-finite
        gradient are left out of the update and counted (nrms_adam_step_guarded); note_grad_check() afterwards lets the
        count reach the host without a sync.  rest: the parameters behind a table that backward(table_adam=...) stepped
        (nrms_adam_step_rest: the same kernels under a timer of their own)."""
        if guard is None:
            guard = self.precision == "fp16"
        if rest:
            rc = self.lib.nrms_adam_step_rest(C.c_size_t(flat.numel()), _lib.ptr(flat), _lib.ptr(gflat), _lib.ptr(exp_avg),
                                              _lib.ptr(exp_avg_sq), C.c_double(lr), C.c_double(betas[0]), C.c_double(betas[1]),
                                              C.c_double(eps), int(step), C.c_float(grad_scale),
                                              _lib.ptr(self._grad_bad) if guard else None, _stream())
            _lib.check(rc, "nrms_adam_step_rest")
            return
        if guard:
            rc = self.lib.nrms_adam_step_guarded(C.c_size_t(flat.numel()), _lib.ptr(flat), _lib.ptr(gflat), _lib.ptr(exp_avg),
                                                 _lib.ptr(exp_avg_sq), C.c_double(lr), C.c_double(betas[0]), C.c_double(betas[1]),
                                                 C.c_double(eps), int(step), C.c_float(grad_scale), _lib.ptr(self._grad_bad), _stream())
            _lib.check(rc, "nrms_adam_step_guarded")
            return
        rc = self.lib.nrms_adam_step(C.c_size_t(flat.numel()), _lib.ptr(flat), _lib.ptr(gflat), _lib.ptr(exp_avg),
                                     _lib.ptr(exp_avg_sq), C.c_double(lr), C.c_double(betas[0]), C.c_double(betas[1]),
                                     C.c_double(eps), int(step), C.c_float(grad_scale), _stream())
        _lib.check(rc, "nrms_adam_step")

    # ---- fp16 gradient overflow: device-side count, host-side back-off of the loss scale, no sync ----------------------
    def grad_guard(self, gflat):
        """inf / nan elements of a gradient buffer -> 0, counted (for callers that run their own optimizer: the autograd path)."""
        rc = self.lib.nrms_grad_guard(C.c_size_t(gflat.numel()), _lib.ptr(gflat), _lib.ptr(self._grad_bad), _stream())
        _lib.check(rc, "nrms_grad_guard")

    def note_grad_check(self):
        """Behind the guarded optimizer / grad_guard of a step: start the asynchronous read-back of the counter."""
        if self._grad_bad_event is not None and not self._grad_bad_event.query():
            return                                       # the previous read-back is still in flight: its count covers this step too
        self._grad_bad_host.copy_(self._grad_bad, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._grad_bad_event = ev

    def poll_grad_overflow(self, block=False):
        """Non-blocking (unless block): if a finished read-back shows non-finite gradient elements, give the fp16 backward two
        more powers of two of head room from the next step on (and warn once per event); after 2 000 clean checks take one back."""
        ev = self._grad_bad_event
        if ev is None:
            return self.loss_scale_backoff
        if block:
            ev.synchronize()
        elif not ev.query():
            return self.loss_scale_backoff
        self._grad_bad_event = None
        n = int(self._grad_bad_host.item())
        if n:
            self._grad_bad.zero_()
            self._grad_bad_host.zero_()
            self.grad_overflow_steps += 1
            self._clean_polls = 0
            if self.loss_scale_backoff < 24:
                self.loss_scale_backoff = min(24, self.loss_scale_backoff + 2)
            import warnings
            warnings.warn("NRMS fp16 backward: %d non-finite gradient element(s) were skipped by the optimizer (an fp16 overflow of "
                          "the loss-scaled gradient tensors, or an inf / nan loss); loss-scale head room raised to 2^%d below the "
                          "default" % (n, self.loss_scale_backoff), RuntimeWarning, stacklevel=2)
        else:
            self._clean_polls += 1
            if self._clean_polls >= 2000 and self.loss_scale_backoff > 0:
                self.loss_scale_backoff -= 1
                self._clean_polls = 0
        return self.loss_scale_backoff

    def impression_auc(self, scores, labels, lens):
        """scores [n, Cmax] fp32, labels [n, Cmax] uint8, lens [n] int32 (device) -> float64 AUC per impression."""
        n, cmax = scores.shape
        auc = torch.empty(n, dtype=torch.float64, device=self.device)
        rc = self.lib.nrms_impression_auc(n, cmax, _lib.ptr(scores.contiguous()), _lib.ptr(labels.contiguous()),
                                          _lib.ptr(lens.contiguous()), _lib.ptr(auc), _stream())
        _lib.check(rc, "nrms_impression_auc")
        return auc

    def impression_metrics(self, scores, labels, lens, ks=(5, 10), ranks=False):
        """scores [n, Cmax] fp32, labels [n, Cmax] uint8, lens [n] int32 (device) -> dict of device tensors:
        float64 [n] ``auc``, ``mrr``, ``ndcg@<k>`` for both cutoffs of ``ks``, and with ranks=True the int32 [n, Cmax]
        submission ranks ``ranks`` (0 past each prefix).  Tie rule and NaN cases: include/nrms_hip.h
        nrms_impression_metrics."""
        return impression_metrics(self.lib, self.device, scores, labels, lens, ks, ranks)

    # ---- retrieval over a whole catalogue ---------------------------------------------------------
    def _cuda_device(self):
        """The engine's device with its index resolved: what the .device of a tensor on it compares equal to."""
        return self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())

    def _check_tensor(self, who, name, t, dtype, ndim):
        """Raises unless t is a contiguous ndim-D tensor of dtype on the engine's device."""
        if t.dim() != ndim or t.dtype != dtype or t.device != self._cuda_device() or not t.is_contiguous():
            raise _lib.NrmsError("%s: %s must be a contiguous %d-D %s tensor on %s (got %s %s on %s%s)"
                                 % (who, name, ndim, dtype, self.device, tuple(t.shape), t.dtype, t.device,
                                    "" if t.is_contiguous() else ", not contiguous"))

    def _exclude_arg(self, who, exclude, B):
        """The checked exclude list of a retrieval call -> (exclude, n_exclude): a contiguous [B, n] int64 tensor on the device,
        or (None, 0) for None and for n = 0."""
        if exclude is None:
            return None, 0
        if (exclude.dim() != 2 or exclude.shape[0] != B or exclude.dtype != torch.int64 or exclude.device != self._cuda_device()
                or not exclude.is_contiguous()):
            raise _lib.NrmsError("%s: exclude must be a contiguous [B, n] int64 tensor on %s (got %s %s on %s)"
                                 % (who, self.device, tuple(exclude.shape), exclude.dtype, exclude.device))
        n_ex = exclude.shape[1]
        return (exclude, n_ex) if n_ex else (None, 0)

    def _item_bias(self, who, bias, N, dev):
        """The checked per-item prior of top_k / rank_of: a contiguous float32 [N] tensor on the device."""
        if (not torch.is_tensor(bias) or bias.dim() != 1 or bias.shape[0] != N or bias.dtype != torch.float32 or bias.device != dev
                or not bias.is_contiguous()):
            got = ("%s %s on %s" % (tuple(bias.shape), bias.dtype, bias.device)) if torch.is_tensor(bias) else type(bias).__name__
            raise _lib.NrmsError("%s: bias must be a contiguous [%d] float32 tensor on %s (got %s)" % (who, N, self.device, got))
        return bias

    def _time_window(self, who, item_time, window, N, B, dev):
        """The checked time window of top_k / rank_of: (item_time [N], window [B, 2]) as contiguous int32 tensors on the device,
        or (None, None) when neither is given.  int64 tensors are accepted when every value fits int32 (one host check)."""
        if item_time is None and window is None:
            return None, None
        if item_time is None or window is None:
            raise _lib.NrmsError("%s: item_time and window go together (window %s, item_time %s)"
                                 % (who, "missing" if window is None else "given", "missing" if item_time is None else "given"))
        out = []
        for name, t, shape in (("item_time", item_time, (N,)), ("window", window, (B, 2))):
            if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype not in (torch.int32, torch.int64) or t.device != dev):
                got = ("%s %s on %s" % (tuple(t.shape), t.dtype, t.device)) if torch.is_tensor(t) else type(t).__name__
                raise _lib.NrmsError("%s: %s must be an int32 (or int64) %s tensor on %s (got %s)" % (who, name, list(shape), self.device, got))
            if t.dtype == torch.int64:
                if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) > 2 ** 31 - 1):
                    raise _lib.NrmsError("%s: %s holds values outside int32 (min %d, max %d)" % (who, name, int(t.min()), int(t.max())))
                t = t.to(torch.int32)
            out.append(t.contiguous())
        return out[0], out[1]

    def top_k(self, user_vec, items, k, exclude=None, bias=None, *, item_time=None, window=None):
        """user_vec [B, d], items [N, d] fp32, exclude [B, n_exclude] int64 or None (device, contiguous) -> (scores [B, k]
        fp32, ids [B, k] int64): per user the k items of largest user . item, no [B, N] matrix (nrms_topk_dot).  Order:
        score descending, then the smaller id; rows with fewer than k eligible items end in id -1 / score -inf; excluded
        ids and NaN scores are never returned.  bias [N] fp32 (device, contiguous) or None: a per-item prior, the order and
        the returned scores are those of user . item + bias[n] (one fp32 add; a NaN bias removes the item for every user;
        nrms_topk_dot_biased).  None calls nrms_topk_dot as before.  item_time [N] int32 and window [B, 2] int32 (device; both
        or neither): user b only gets items with window[b, 0] <= item_time[n] < window[b, 1] (signed, half-open; lo >= hi is an
        all-padding row; a time of INT32_MAX is never eligible; nrms_topk_dot_windowed, with the bias when one is given).
        include/nrms_hip.h states the contract."""
        k = int(k)
        dev = self._cuda_device()
        self._check_tensor("top_k", "user_vec", user_vec, torch.float32, 2)
        self._check_tensor("top_k", "items", items, torch.float32, 2)
        B, d = user_vec.shape
        N = items.shape[0]
        if items.shape[1] != d:
            raise _lib.NrmsError("top_k: items width %d != user_vec width %d" % (items.shape[1], d))
        exclude, n_ex = self._exclude_arg("top_k", exclude, B)
        if bias is not None:
            self._item_bias("top_k", bias, N, dev)
        item_time, window = self._time_window("top_k", item_time, window, N, B, dev)
        nbytes = self.lib.nrms_topk_dot_workspace_bytes(B, N, d, k)
        if nbytes == 0:
            raise _lib.NrmsError("top_k: arguments rejected (B=%d, N=%d, d=%d, k=%d; 1 <= k <= 256)" % (B, N, d, k))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        if window is not None:
            rc = self.lib.nrms_topk_dot_windowed(B, C.c_int64(N), d, k, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                                 _lib.ptr(item_time), _lib.ptr(window), _lib.ptr(exclude), n_ex, _lib.ptr(scores),
                                                 _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
            _lib.check(rc, "nrms_topk_dot_windowed")
            return scores, ids
        if bias is not None:
            rc = self.lib.nrms_topk_dot_biased(B, C.c_int64(N), d, k, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                               _lib.ptr(exclude), n_ex, _lib.ptr(scores), _lib.ptr(ids), _lib.ptr(ws),
                                               C.c_size_t(ws.numel() * 8), _stream())
            _lib.check(rc, "nrms_topk_dot_biased")
            return scores, ids
        rc = self.lib.nrms_topk_dot(B, C.c_int64(N), d, k, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(exclude), n_ex,
                                    _lib.ptr(scores), _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_topk_dot")
        return scores, ids

    def _tag_args(self, who, item_tag, n_tags, allow, N, B, dev):
        """The checked tag set of top_k_tagged / rank_of_tagged -> (item_tag [N] int32, allow [B, W] int32), contiguous, on the
        device.  item_tag may be int64 (values outside int32 become -1, which is open to nobody, on the device); allow may be the
        bool [B, n_tags] matrix (packed here by pack_tag_mask) or the packed int32 [B, W], W = ceil(n_tags / 32)."""
        item_tag, n_tags = self._item_tag_arg(who, item_tag, n_tags, N, dev)
        W = (n_tags + 31) // 32
        ok = torch.is_tensor(allow) and allow.dim() == 2 and allow.shape[0] == B and allow.device == dev
        if ok and allow.dtype == torch.bool and allow.shape[1] == n_tags:
            allow = pack_tag_mask(allow)
        elif not (ok and allow.dtype == torch.int32 and allow.shape[1] == W):
            got = ("%s %s on %s" % (tuple(allow.shape), allow.dtype, allow.device)) if torch.is_tensor(allow) else type(allow).__name__
            raise _lib.NrmsError("%s: allow must be a bool [%d, %d] or a packed int32 [%d, %d] tensor on %s (got %s)"
                                 % (who, B, n_tags, B, W, self.device, got))
        return item_tag, allow.contiguous(), n_tags

    def _item_tag_arg(self, who, item_tag, n_tags, N, dev):
        """The checked n_tags and item_tag of the tagged and the capped calls -> (item_tag [N] int32, contiguous, n_tags)."""
        n_tags = int(n_tags)
        if not 1 <= n_tags <= MAX_TAGS:
            raise _lib.NrmsError("%s: n_tags must be in [1, %d] (n_tags=%d)" % (who, MAX_TAGS, n_tags))
        if (not torch.is_tensor(item_tag) or tuple(item_tag.shape) != (N,) or item_tag.dtype not in (torch.int32, torch.int64)
                or item_tag.device != dev):
            got = ("%s %s on %s" % (tuple(item_tag.shape), item_tag.dtype, item_tag.device)) if torch.is_tensor(item_tag) else type(item_tag).__name__
            raise _lib.NrmsError("%s: item_tag must be an int32 (or int64) [%d] tensor on %s (got %s)" % (who, N, self.device, got))
        if item_tag.dtype == torch.int64:
            item_tag = torch.where((item_tag < 0) | (item_tag >= n_tags), torch.full_like(item_tag, -1), item_tag).to(torch.int32)
        return item_tag.contiguous(), n_tags

    def top_k_tagged(self, user_vec, items, k, item_tag, n_tags, allow, exclude=None, bias=None):
        """top_k inside a per-user set of item tags -> (scores [B, k] fp32, ids [B, k] int64).  item_tag [N] int32 (device): one tag
        per item; allow: bool [B, n_tags] or the packed int32 [B, ceil(n_tags / 32)] of pack_tag_mask (device): user b only gets
        items with 0 <= item_tag[n] < n_tags whose tag b allows (a tag outside that range, e.g. -1, is open to nobody; an all-False
        row is all padding).  Scores, order, padding, exclude and bias are top_k's, bit for bit; 1 <= n_tags <= 512
        (nrms_topk_dot_tagged; include/nrms_hip.h states the contract)."""
        who = "top_k_tagged"
        k = int(k)
        B, N, d, exclude, n_ex, _, _ = self._top_k_args(who, user_vec, items, exclude, bias, None, None)
        item_tag, allow, n_tags = self._tag_args(who, item_tag, n_tags, allow, N, B, self._cuda_device())
        nbytes = self.lib.nrms_topk_dot_tagged_workspace_bytes(B, N, d, k)
        if nbytes == 0:
            raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, k=%d; 1 <= k <= 256)" % (who, B, N, d, k))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        rc = self.lib.nrms_topk_dot_tagged(B, C.c_int64(N), d, k, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                           _lib.ptr(item_tag), n_tags, _lib.ptr(allow), _lib.ptr(exclude), n_ex, _lib.ptr(scores),
                                           _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_topk_dot_tagged")
        return scores, ids

    def top_k_capped(self, user_vec, items, k, item_tag, n_tags, cap, exclude=None, bias=None):
        """top_k with per-tag caps -> (scores [B, k] fp32, ids [B, k] int64): walking user b's full ranking (top_k's: the same
        score bits, order, exclude and bias), item n with tag t = item_tag[n] is taken iff 0 <= t < n_tags and fewer than cap[b, t]
        items of tag t were taken before it; the first k taken items are row b, then -1 / -inf.  item_tag [N] int32 (device), as in
        top_k_tagged (a tag outside [0, n_tags), e.g. -1, is served to nobody); cap int32 [B, n_tags] (device): <= 0 closes the tag
        for that user, >= k leaves it uncapped.  Every cap >= k is top_k_tagged with all tags open, bit for bit;
        1 <= n_tags <= 512 (nrms_topk_dot_capped; include/nrms_hip.h states the contract)."""
        who = "top_k_capped"
        k = int(k)
        B, N, d, exclude, n_ex, _, _ = self._top_k_args(who, user_vec, items, exclude, bias, None, None)
        dev = self._cuda_device()
        item_tag, n_tags = self._item_tag_arg(who, item_tag, n_tags, N, dev)
        if (not torch.is_tensor(cap) or tuple(cap.shape) != (B, n_tags) or cap.dtype != torch.int32 or cap.device != dev):
            got = ("%s %s on %s" % (tuple(cap.shape), cap.dtype, cap.device)) if torch.is_tensor(cap) else type(cap).__name__
            raise _lib.NrmsError("%s: cap must be an int32 [%d, %d] tensor on %s (got %s)" % (who, B, n_tags, self.device, got))
        cap = cap.contiguous()
        nbytes = self.lib.nrms_topk_dot_capped_workspace_bytes(B, N, d, k)
        if nbytes == 0:
            raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, k=%d; 1 <= k <= 256)" % (who, B, N, d, k))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        rc = self.lib.nrms_topk_dot_capped(B, C.c_int64(N), d, k, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                           _lib.ptr(item_tag), n_tags, _lib.ptr(cap), _lib.ptr(exclude), n_ex, _lib.ptr(scores),
                                           _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_topk_dot_capped")
        return scores, ids

    def rank_of_tagged(self, user_vec, items, targets, item_tag, n_tags, allow, exclude=None, bias=None):
        """rank_of inside a per-user set of item tags -> (ranks [B, T] int32, scores [B, T] fp32): the exact 1-based position of
        every target in top_k_tagged's order.  item_tag, n_tags and allow are top_k_tagged's; ranks count the items open to user b
        only, and a target closed by its tag gets rank 0 / -inf like an excluded one.  Wider ``targets`` go in column chunks of 32
        (nrms_rank_dot_tagged; include/nrms_hip.h states the contract)."""
        who = "rank_of_tagged"
        self._check_tensor(who, "targets", targets, torch.int64, 2)
        B, N, d, exclude, n_ex, _, _ = self._top_k_args(who, user_vec, items, exclude, bias, None, None)
        if targets.shape[0] != B:
            raise _lib.NrmsError("%s: targets must be [%d, T] (got %s)" % (who, B, tuple(targets.shape)))
        item_tag, allow, n_tags = self._tag_args(who, item_tag, n_tags, allow, N, B, self._cuda_device())
        T_all = targets.shape[1]
        ranks = torch.empty(B, T_all, dtype=torch.int32, device=self.device)
        scores = torch.empty(B, T_all, dtype=torch.float32, device=self.device)
        for t0 in range(0, T_all, 32):
            T = min(32, T_all - t0)
            whole = T == T_all
            tg = targets if whole else targets[:, t0:t0 + T].contiguous()
            rk = ranks if whole else torch.empty(B, T, dtype=torch.int32, device=self.device)
            sc = scores if whole else torch.empty(B, T, dtype=torch.float32, device=self.device)
            nbytes = self.lib.nrms_rank_dot_tagged_workspace_bytes(B, N, d, T, n_ex)
            if nbytes == 0:
                raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, T=%d, n_exclude=%d)" % (who, B, N, d, T, n_ex))
            ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
            rc = self.lib.nrms_rank_dot_tagged(B, C.c_int64(N), d, T, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                               _lib.ptr(item_tag), n_tags, _lib.ptr(allow), _lib.ptr(tg), _lib.ptr(exclude), n_ex,
                                               _lib.ptr(rk), _lib.ptr(sc), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
            _lib.check(rc, "nrms_rank_dot_tagged")
            if not whole:
                ranks[:, t0:t0 + T] = rk
                scores[:, t0:t0 + T] = sc
        return ranks, scores

    def _adjust_args(self, who, adj_ids, adj_delta, B, dev):
        """The checked slots of top_k_adjusted / rank_of_adjusted -> (adj_ids [B, E] int64, adj_delta [B, E] fp32, E), contiguous,
        on the device; 0 <= E <= 256."""
        for name, t, dt in (("adj_ids", adj_ids, torch.int64), ("adj_delta", adj_delta, torch.float32)):
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != B or t.dtype != dt or t.device != dev:
                got = ("%s %s on %s" % (tuple(t.shape), t.dtype, t.device)) if torch.is_tensor(t) else type(t).__name__
                raise _lib.NrmsError("%s: %s must be a%s %s [%d, E] tensor on %s (got %s)"
                                     % (who, name, "n" if dt == torch.int64 else "", str(dt).replace("torch.", ""), B, self.device, got))
        if adj_ids.shape != adj_delta.shape:
            raise _lib.NrmsError("%s: adj_ids %s and adj_delta %s must have one shape"
                                 % (who, tuple(adj_ids.shape), tuple(adj_delta.shape)))
        E = adj_ids.shape[1]
        if E > MAX_ADJUST:
            raise _lib.NrmsError("%s: n_adjust must be in [0, %d] (n_adjust=%d)" % (who, MAX_ADJUST, E))
        return adj_ids.contiguous(), adj_delta.contiguous(), E

    def top_k_adjusted(self, user_vec, items, k, adj_ids, adj_delta, exclude=None, bias=None):
        """top_k with per-user score adjustments -> (scores [B, k] fp32, ids [B, k] int64).  adj_ids int64 [B, E], adj_delta fp32
        [B, E] (device), 0 <= E <= 256: slot (b, e) moves the score of catalogue row adj_ids[b, e] for user b by adj_delta[b, e], one
        fp32 add on the finished (biased) score; an id outside [0, N), e.g. -1, is an empty slot; of several slots of a row that name
        one item the lowest e counts; a NaN delta closes the item for that user.  The returned scores are the adjusted ones.  Order,
        padding, exclude and bias are top_k's, and all-empty slots give top_k bit for bit (nrms_topk_dot_adjusted; include/nrms_hip.h
        states the contract)."""
        who = "top_k_adjusted"
        k = int(k)
        B, N, d, exclude, n_ex, _, _ = self._top_k_args(who, user_vec, items, exclude, bias, None, None)
        adj_ids, adj_delta, E = self._adjust_args(who, adj_ids, adj_delta, B, self._cuda_device())
        nbytes = self.lib.nrms_topk_dot_adjusted_workspace_bytes(B, N, d, k)
        if nbytes == 0:
            raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, k=%d; 1 <= k <= 256)" % (who, B, N, d, k))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        rc = self.lib.nrms_topk_dot_adjusted(B, C.c_int64(N), d, k, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                             _lib.ptr(adj_ids), _lib.ptr(adj_delta), E, _lib.ptr(exclude), n_ex, _lib.ptr(scores),
                                             _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_topk_dot_adjusted")
        return scores, ids

    def rank_of_adjusted(self, user_vec, items, targets, adj_ids, adj_delta, exclude=None, bias=None):
        """rank_of with per-user score adjustments -> (ranks [B, T] int32, scores [B, T] fp32): the exact 1-based position of every
        target in top_k_adjusted's order, and its adjusted score.  adj_ids and adj_delta are top_k_adjusted's; a target whose delta
        is NaN gets rank 0 / -inf like an excluded one.  Wider ``targets`` go in column chunks of 32 (nrms_rank_dot_adjusted;
        include/nrms_hip.h states the contract)."""
        who = "rank_of_adjusted"
        self._check_tensor(who, "targets", targets, torch.int64, 2)
        B, N, d, exclude, n_ex, _, _ = self._top_k_args(who, user_vec, items, exclude, bias, None, None)
        if targets.shape[0] != B:
            raise _lib.NrmsError("%s: targets must be [%d, T] (got %s)" % (who, B, tuple(targets.shape)))
        adj_ids, adj_delta, E = self._adjust_args(who, adj_ids, adj_delta, B, self._cuda_device())
        T_all = targets.shape[1]
        ranks = torch.empty(B, T_all, dtype=torch.int32, device=self.device)
        scores = torch.empty(B, T_all, dtype=torch.float32, device=self.device)
        for t0 in range(0, T_all, 32):
            T = min(32, T_all - t0)
            whole = T == T_all
            tg = targets if whole else targets[:, t0:t0 + T].contiguous()
            rk = ranks if whole else torch.empty(B, T, dtype=torch.int32, device=self.device)
            sc = scores if whole else torch.empty(B, T, dtype=torch.float32, device=self.device)
            nbytes = self.lib.nrms_rank_dot_adjusted_workspace_bytes(B, N, d, T, n_ex)
            if nbytes == 0:
                raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, T=%d, n_exclude=%d)" % (who, B, N, d, T, n_ex))
            ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
            rc = self.lib.nrms_rank_dot_adjusted(B, C.c_int64(N), d, T, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                                 _lib.ptr(adj_ids), _lib.ptr(adj_delta), E, _lib.ptr(tg), _lib.ptr(exclude), n_ex,
                                                 _lib.ptr(rk), _lib.ptr(sc), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
            _lib.check(rc, "nrms_rank_dot_adjusted")
            if not whole:
                ranks[:, t0:t0 + T] = rk
                scores[:, t0:t0 + T] = sc
        return ranks, scores

    def _top_k_args(self, who, user_vec, items, exclude, bias, item_time, window):
        """The checks top_k_after and top_k_deep share with top_k -> (B, N, d, exclude, n_exclude, item_time, window)."""
        dev = self._cuda_device()
        self._check_tensor(who, "user_vec", user_vec, torch.float32, 2)
        self._check_tensor(who, "items", items, torch.float32, 2)
        B, d = user_vec.shape
        N = items.shape[0]
        if items.shape[1] != d:
            raise _lib.NrmsError("%s: items width %d != user_vec width %d" % (who, items.shape[1], d))
        exclude, n_ex = self._exclude_arg(who, exclude, B)
        if bias is not None:
            self._item_bias(who, bias, N, dev)
        item_time, window = self._time_window(who, item_time, window, N, B, dev)
        return B, N, d, exclude, n_ex, item_time, window

    def top_k_after(self, user_vec, items, k, after_scores, after_ids, exclude=None, bias=None, *, item_time=None, window=None):
        """One page of top_k's ranking: per user the k items that come strictly AFTER the position (after_scores[b], after_ids[b])
        in top_k's order (score descending, then the smaller id) -> (scores [B, k] fp32, ids [B, k] int64).  after_scores [B] fp32,
        after_ids [B] int64 (device, contiguous): the last column of the page before.  after_ids[b] = -2 (PAGE_BEGIN): no cursor,
        the row is top_k's bit for bit; -1, any other negative id or a NaN score: the list is exhausted, the row is all padding
        (-1 / -inf, which is what a page leaves in the columns it could not fill); >= 0: a position, the id need not be an
        eligible item.  Every other argument is top_k's (nrms_topk_dot_after; include/nrms_hip.h states the contract)."""
        who = "top_k_after"
        k = int(k)
        B, N, d, exclude, n_ex, item_time, window = self._top_k_args(who, user_vec, items, exclude, bias, item_time, window)
        for name, t, dtype in (("after_scores", after_scores, torch.float32), ("after_ids", after_ids, torch.int64)):
            if not torch.is_tensor(t) or tuple(t.shape) != (B,):
                raise _lib.NrmsError("%s: %s must be a [%d] %s tensor (got %s)"
                                     % (who, name, B, dtype, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
            self._check_tensor(who, name, t, dtype, 1)
        nbytes = self.lib.nrms_topk_dot_after_workspace_bytes(B, N, d, k)
        if nbytes == 0:
            raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, k=%d; 1 <= k <= 256)" % (who, B, N, d, k))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        rc = self.lib.nrms_topk_dot_after(B, C.c_int64(N), d, k, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                          _lib.ptr(item_time), _lib.ptr(window), _lib.ptr(after_scores), _lib.ptr(after_ids),
                                          _lib.ptr(exclude), n_ex, _lib.ptr(scores), _lib.ptr(ids), _lib.ptr(ws),
                                          C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_topk_dot_after")
        return scores, ids

    def top_k_deep(self, user_vec, items, K, exclude=None, bias=None, *, item_time=None, window=None):
        """top_k at a depth of up to 4096: (scores [B, K] fp32, ids [B, K] int64), per user the first K items of top_k's order, then
        -1 / -inf.  ceil(K / 256) pages of top_k_after chained on the device, each reading its cursor from the page before: no
        host synchronisation (nrms_topk_dot_deep).  K <= 256 is top_k, bit for bit; the arguments are top_k's."""
        who = "top_k_deep"
        K = int(K)
        B, N, d, exclude, n_ex, item_time, window = self._top_k_args(who, user_vec, items, exclude, bias, item_time, window)
        nbytes = self.lib.nrms_topk_dot_deep_workspace_bytes(B, N, d, K)
        if nbytes == 0:
            raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, K=%d; 1 <= K <= 4096)" % (who, B, N, d, K))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        scores = torch.empty(B, K, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, K, dtype=torch.int64, device=self.device)
        rc = self.lib.nrms_topk_dot_deep(B, C.c_int64(N), d, K, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                         _lib.ptr(item_time), _lib.ptr(window), _lib.ptr(exclude), n_ex, _lib.ptr(scores),
                                         _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_topk_dot_deep")
        return scores, ids

    def _request_args(self, who, user_vec, items, exclude, bias, item_time, window, item_tag, n_tags, allow, adj_ids, adj_delta):
        """The checked parts of top_k_request / rank_of_request: every pair is both or neither ->
        (B, N, d, exclude, n_exclude, item_time, window, item_tag, n_tags, allow, adj_ids, adj_delta, E), absent parts None / 0."""
        B, N, d, exclude, n_ex, item_time, window = self._top_k_args(who, user_vec, items, exclude, bias, item_time, window)
        dev = self._cuda_device()
        if (item_tag is None) != (allow is None):
            raise _lib.NrmsError("%s: item_tag and allow go together (item_tag %s, allow %s)"
                                 % (who, "missing" if item_tag is None else "given", "missing" if allow is None else "given"))
        if item_tag is not None:
            if n_tags is None:
                if not (torch.is_tensor(allow) and allow.dtype == torch.bool and allow.dim() == 2):
                    raise _lib.NrmsError("%s: a packed allow needs n_tags=" % who)
                n_tags = allow.shape[1]
            item_tag, allow, n_tags = self._tag_args(who, item_tag, n_tags, allow, N, B, dev)
        else:
            n_tags = 0
        if (adj_ids is None) != (adj_delta is None):
            raise _lib.NrmsError("%s: adj_ids and adj_delta go together (adj_ids %s, adj_delta %s)"
                                 % (who, "missing" if adj_ids is None else "given", "missing" if adj_delta is None else "given"))
        E = 0
        if adj_ids is not None:
            adj_ids, adj_delta, E = self._adjust_args(who, adj_ids, adj_delta, B, dev)
            if E == 0:
                adj_ids = adj_delta = None
        return B, N, d, exclude, n_ex, item_time, window, item_tag, n_tags, allow, adj_ids, adj_delta, E

    def top_k_request(self, user_vec, items, k, exclude=None, bias=None, *, item_time=None, window=None, item_tag=None, n_tags=None,
                      allow=None, adj_ids=None, adj_delta=None, after_scores=None, after_ids=None):
        """top_k through several catalogue filters at once -> (scores [B, k] fp32, ids [B, k] int64): a time window (item_time,
        window: top_k's), a tag set (item_tag, n_tags, allow: top_k_tagged's), per-user adjustments (adj_ids, adj_delta:
        top_k_adjusted's) and a cursor (after_scores, after_ids: top_k_after's), each pair both or neither, each with the rules of
        its own call.  The score is (user . item + bias[n]) + delta, two fp32 adds in that order; item n is eligible for user b iff
        it is not excluded, that score is not NaN, b's window is open to it and b allows its tag; the cursor compares the adjusted
        score, so a client that pages passes the same adjustments on every page.  No part or one part is the part's own call, bit
        for bit (nrms_topk_dot_request; include/nrms_hip.h states the contract)."""
        who = "top_k_request"
        k = int(k)
        (B, N, d, exclude, n_ex, item_time, window, item_tag, n_tags, allow, adj_ids, adj_delta, E) = self._request_args(
            who, user_vec, items, exclude, bias, item_time, window, item_tag, n_tags, allow, adj_ids, adj_delta)
        if (after_scores is None) != (after_ids is None):
            raise _lib.NrmsError("%s: after_scores and after_ids go together (after_scores %s, after_ids %s)"
                                 % (who, "missing" if after_scores is None else "given", "missing" if after_ids is None else "given"))
        if after_ids is not None:
            for name, t, dtype in (("after_scores", after_scores, torch.float32), ("after_ids", after_ids, torch.int64)):
                if not torch.is_tensor(t) or tuple(t.shape) != (B,):
                    raise _lib.NrmsError("%s: %s must be a [%d] %s tensor (got %s)"
                                         % (who, name, B, dtype, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
                self._check_tensor(who, name, t, dtype, 1)
        nbytes = self.lib.nrms_topk_dot_request_workspace_bytes(B, N, d, k)
        if nbytes == 0:
            raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, k=%d; 1 <= k <= 256)" % (who, B, N, d, k))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        rc = self.lib.nrms_topk_dot_request(B, C.c_int64(N), d, k, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                            _lib.ptr(item_time), _lib.ptr(window), _lib.ptr(item_tag), n_tags, _lib.ptr(allow),
                                            _lib.ptr(adj_ids), _lib.ptr(adj_delta), E, _lib.ptr(after_scores), _lib.ptr(after_ids),
                                            _lib.ptr(exclude), n_ex, _lib.ptr(scores), _lib.ptr(ids), _lib.ptr(ws),
                                            C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_topk_dot_request")
        return scores, ids

    def top_k_request_capped(self, user_vec, items, k, item_tag, n_tags, cap, exclude=None, bias=None, *, item_time=None,
                             window=None, allow=None, adj_ids=None, adj_delta=None, after_scores=None, after_ids=None):
        """top_k_capped over the items top_k_request leaves eligible -> (scores [B, k] fp32, ids [B, k] int64): the request's
        adjusted score and eligibility (window, tag set, adjustments, cursor: each pair both or neither, each with the rules of its
        own call; ``allow`` is the tag set over the same item_tag and n_tags), walked in order, item n with tag t taken iff 0 <= t <
        n_tags and fewer than cap[b, t] items of tag t were taken before it in this call.  cap int32 [B, n_tags] (device): <= 0
        closes the tag, >= k leaves it uncapped.  Every cap >= k is top_k_request, no other part is top_k_capped, bit for bit.
        Pages chain through the cursor and ``remaining_caps`` (nrms_topk_dot_request_capped; include/nrms_hip.h states the
        contract)."""
        who = "top_k_request_capped"
        k = int(k)
        B, N, d, exclude, n_ex, item_time, window = self._top_k_args(who, user_vec, items, exclude, bias, item_time, window)
        dev = self._cuda_device()
        if allow is not None:
            item_tag, allow, n_tags = self._tag_args(who, item_tag, n_tags, allow, N, B, dev)
        else:
            item_tag, n_tags = self._item_tag_arg(who, item_tag, n_tags, N, dev)
        if (not torch.is_tensor(cap) or tuple(cap.shape) != (B, n_tags) or cap.dtype != torch.int32 or cap.device != dev):
            got = ("%s %s on %s" % (tuple(cap.shape), cap.dtype, cap.device)) if torch.is_tensor(cap) else type(cap).__name__
            raise _lib.NrmsError("%s: cap must be an int32 [%d, %d] tensor on %s (got %s)" % (who, B, n_tags, self.device, got))
        cap = cap.contiguous()
        if (adj_ids is None) != (adj_delta is None):
            raise _lib.NrmsError("%s: adj_ids and adj_delta go together (adj_ids %s, adj_delta %s)"
                                 % (who, "missing" if adj_ids is None else "given", "missing" if adj_delta is None else "given"))
        E = 0
        if adj_ids is not None:
            adj_ids, adj_delta, E = self._adjust_args(who, adj_ids, adj_delta, B, dev)
            if E == 0:
                adj_ids = adj_delta = None
        if (after_scores is None) != (after_ids is None):
            raise _lib.NrmsError("%s: after_scores and after_ids go together (after_scores %s, after_ids %s)"
                                 % (who, "missing" if after_scores is None else "given", "missing" if after_ids is None else "given"))
        if after_ids is not None:
            for name, t, dtype in (("after_scores", after_scores, torch.float32), ("after_ids", after_ids, torch.int64)):
                if not torch.is_tensor(t) or tuple(t.shape) != (B,):
                    raise _lib.NrmsError("%s: %s must be a [%d] %s tensor (got %s)"
                                         % (who, name, B, dtype, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
                self._check_tensor(who, name, t, dtype, 1)
        nbytes = self.lib.nrms_topk_dot_request_capped_workspace_bytes(B, N, d, k)
        if nbytes == 0:
            raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, k=%d; 1 <= k <= 256)" % (who, B, N, d, k))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        rc = self.lib.nrms_topk_dot_request_capped(B, C.c_int64(N), d, k, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                                   _lib.ptr(item_time), _lib.ptr(window), _lib.ptr(item_tag), n_tags,
                                                   _lib.ptr(allow), _lib.ptr(cap), _lib.ptr(adj_ids), _lib.ptr(adj_delta), E,
                                                   _lib.ptr(after_scores), _lib.ptr(after_ids), _lib.ptr(exclude), n_ex,
                                                   _lib.ptr(scores), _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8),
                                                   _stream())
        _lib.check(rc, "nrms_topk_dot_request_capped")
        return scores, ids

    def rank_of_request(self, user_vec, items, targets, exclude=None, bias=None, *, item_time=None, window=None, item_tag=None,
                        n_tags=None, allow=None, adj_ids=None, adj_delta=None):
        """rank_of through several catalogue filters at once -> (ranks [B, T] int32, scores [B, T] fp32): the exact 1-based position
        of every target in top_k_request's order with the same parts, and its adjusted score.  A target closed by any part (its
        time, its tag, a NaN delta), excluded or out of range gets rank 0 / -inf; otherwise 1 + the number of eligible items before
        it.  Wider ``targets`` go in column chunks of 32 (nrms_rank_dot_request; include/nrms_hip.h states the contract)."""
        who = "rank_of_request"
        self._check_tensor(who, "targets", targets, torch.int64, 2)
        (B, N, d, exclude, n_ex, item_time, window, item_tag, n_tags, allow, adj_ids, adj_delta, E) = self._request_args(
            who, user_vec, items, exclude, bias, item_time, window, item_tag, n_tags, allow, adj_ids, adj_delta)
        if targets.shape[0] != B:
            raise _lib.NrmsError("%s: targets must be [%d, T] (got %s)" % (who, B, tuple(targets.shape)))
        T_all = targets.shape[1]
        ranks = torch.empty(B, T_all, dtype=torch.int32, device=self.device)
        scores = torch.empty(B, T_all, dtype=torch.float32, device=self.device)
        for t0 in range(0, T_all, 32):
            T = min(32, T_all - t0)
            whole = T == T_all
            tg = targets if whole else targets[:, t0:t0 + T].contiguous()
            rk = ranks if whole else torch.empty(B, T, dtype=torch.int32, device=self.device)
            sc = scores if whole else torch.empty(B, T, dtype=torch.float32, device=self.device)
            nbytes = self.lib.nrms_rank_dot_request_workspace_bytes(B, N, d, T, n_ex)
            if nbytes == 0:
                raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, T=%d, n_exclude=%d)" % (who, B, N, d, T, n_ex))
            ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
            rc = self.lib.nrms_rank_dot_request(B, C.c_int64(N), d, T, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                                _lib.ptr(item_time), _lib.ptr(window), _lib.ptr(item_tag), n_tags, _lib.ptr(allow),
                                                _lib.ptr(adj_ids), _lib.ptr(adj_delta), E, _lib.ptr(tg), _lib.ptr(exclude), n_ex,
                                                _lib.ptr(rk), _lib.ptr(sc), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
            _lib.check(rc, "nrms_rank_dot_request")
            if not whole:
                ranks[:, t0:t0 + T] = rk
                scores[:, t0:t0 + T] = sc
        return ranks, scores

    def pack_catalogue(self, items):
        """items [N, d] fp32 (device, contiguous) -> PackedCatalogue: the fp16 copy top_k_coarse scans (N * pitch * 2 bytes, pitch =
        32 ceil(d / 32)) and its two norm bounds, beside the fp32 rows it was made from (nrms_catalogue_pack_f16).  Pack again
        whenever the rows change."""
        self._check_tensor("pack_catalogue", "items", items, torch.float32, 2)
        N, d = items.shape
        pitch = self.lib.nrms_catalogue_f16_pitch(d)
        if pitch == 0:
            raise _lib.NrmsError("pack_catalogue: arguments rejected (N=%d, d=%d; d >= 1)" % (N, d))
        items16 = torch.empty(N, pitch, dtype=torch.int16, device=self.device)
        stats = torch.empty(2, dtype=torch.float32, device=self.device)
        rc = self.lib.nrms_catalogue_pack_f16(C.c_int64(N), d, _lib.ptr(items), _lib.ptr(items16), _lib.ptr(stats), _stream())
        _lib.check(rc, "nrms_catalogue_pack_f16")
        return PackedCatalogue(items, items16, stats)

    def top_k_coarse(self, user_vec, packed, k, M, exclude=None, return_shortlist=False):
        """user_vec [B, d] fp32, packed: pack_catalogue(items), exclude as top_k's -> (scores [B, k] fp32, ids [B, k] int64, certified
        [B] uint8), with return_shortlist also the coarse shortlist (short_scores [B, M] fp32, short_ids [B, M] int64).  A row with
        certified = 1 is top_k's row bit for bit; a row with certified = 0 is the exact top k of its fp16 shortlist only and has to go
        through top_k (nrms_topk_dot_coarse; include/nrms_hip.h states the certificate).  1 <= k <= M <= 256."""
        k, M = int(k), int(M)
        if not isinstance(packed, PackedCatalogue):
            raise _lib.NrmsError("top_k_coarse: packed must be a PackedCatalogue (pack_catalogue(items)), got %s" % type(packed).__name__)
        items = packed.items
        self._check_tensor("top_k_coarse", "user_vec", user_vec, torch.float32, 2)
        self._check_tensor("top_k_coarse", "items", items, torch.float32, 2)
        B, d = user_vec.shape
        N = items.shape[0]
        if items.shape[1] != d:
            raise _lib.NrmsError("top_k_coarse: items width %d != user_vec width %d" % (items.shape[1], d))
        exclude, n_ex = self._exclude_arg("top_k_coarse", exclude, B)
        nbytes = self.lib.nrms_topk_dot_coarse_workspace_bytes(B, N, d, k, M)
        if nbytes == 0:
            raise _lib.NrmsError("top_k_coarse: arguments rejected (B=%d, N=%d, d=%d, k=%d, M=%d; 1 <= k <= M <= 256)" % (B, N, d, k, M))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        cert = torch.empty(B, dtype=torch.uint8, device=self.device)
        ss = torch.empty(B, M, dtype=torch.float32, device=self.device) if return_shortlist else None
        si = torch.empty(B, M, dtype=torch.int64, device=self.device) if return_shortlist else None
        rc = self.lib.nrms_topk_dot_coarse(B, C.c_int64(N), d, k, M, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(packed.items16),
                                           _lib.ptr(packed.stats), _lib.ptr(exclude), n_ex, _lib.ptr(scores), _lib.ptr(ids),
                                           _lib.ptr(cert), _lib.ptr(ss), _lib.ptr(si), _lib.ptr(ws), C.c_size_t(ws.numel() * 8),
                                           _stream())
        _lib.check(rc, "nrms_topk_dot_coarse")
        return (scores, ids, cert, ss, si) if return_shortlist else (scores, ids, cert)

    def softmax_sample(self, user_vec, items, row_key, S, inv_temperature, seed, exclude=None, return_keys=False):
        """user_vec [B, d], items [N, d] fp32, row_key [B] int64 in [0, 2^48), exclude [B, n_exclude] int64 or None (device,
        contiguous) -> ids [B, S] int64 (with return_keys also the perturbed keys [B, S] fp32): per user S items drawn without
        replacement from softmax(user . item * inv_temperature) over the eligible items, in Plackett-Luce order, no [B, N]
        matrix (nrms_softmax_sample_dot: Gumbel-top-S on top_k's kernels).  The draw of a row is a function of (its user
        vector, items, row key, inv_temperature, seed, its exclude list) only; rows with fewer than S eligible items end in
        id -1 / key -inf.  inv_temperature 0 is the uniform draw.  include/nrms_hip.h states the contract."""
        S = int(S)
        for name, t, dt, nd in (("user_vec", user_vec, torch.float32, 2), ("items", items, torch.float32, 2), ("row_key", row_key, torch.int64, 1)):
            self._check_tensor("softmax_sample", name, t, dt, nd)
        B, d = user_vec.shape
        N = items.shape[0]
        if items.shape[1] != d:
            raise _lib.NrmsError("softmax_sample: items width %d != user_vec width %d" % (items.shape[1], d))
        if row_key.shape[0] != B:
            raise _lib.NrmsError("softmax_sample: row_key must be [%d] (got %s)" % (B, tuple(row_key.shape)))
        exclude, n_ex = self._exclude_arg("softmax_sample", exclude, B)
        nbytes = self.lib.nrms_softmax_sample_dot_workspace_bytes(B, N, d, S, n_ex)
        if nbytes == 0:
            raise _lib.NrmsError("softmax_sample: arguments rejected (B=%d, N=%d, d=%d, S=%d; 1 <= S <= 256)" % (B, N, d, S))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        ids = torch.empty(B, S, dtype=torch.int64, device=self.device)
        keys = torch.empty(B, S, dtype=torch.float32, device=self.device) if return_keys else None
        rc = self.lib.nrms_softmax_sample_dot(B, C.c_int64(N), d, S, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(row_key),
                                              C.c_float(float(inv_temperature)), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                              _lib.ptr(exclude), n_ex, _lib.ptr(ids), _lib.ptr(keys), _lib.ptr(ws),
                                              C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_softmax_sample_dot")
        return (ids, keys) if return_keys else ids

    def log_partition(self, user_vec, items, inv_temperature, exclude=None, bias=None, bias_scale=None, return_mass=False):
        """user_vec [B, d], items [N, d] fp32, exclude [B, n_exclude] int64 or None, bias [N] fp32 or None (device, contiguous);
        inv_temperature: a float or a sequence of J <= 8 floats, each finite and >= 0; bias_scale: None (all 1) or J finite
        floats -> (lse [B, J] fp32, zmax [B, J] fp32, n_eligible [B, J] int32): per user and variant j the exact
        log sum over the eligible items of exp(fmaf(user . item, inv_temperature[j], bias_scale[j] * bias[n])), its largest
        logit and the number of eligible items, no [B, N] matrix, one pass pair over the catalogue for all J variants
        (nrms_logsumexp_dot).  Excluded ids never enter the maximum or the sum; a NaN bias removes the item for every user.
        A row's result is bit for bit a function of its user vector, its eligible logits and the variant's parameters.
        return_mass (the test hook nrms_logsumexp_dot_mass): the raw integer mass [B, J, 2] int64 instead.
        include/nrms_hip.h states the contract."""
        who = "log_partition"
        dev = self._cuda_device()
        self._check_tensor(who, "user_vec", user_vec, torch.float32, 2)
        self._check_tensor(who, "items", items, torch.float32, 2)
        B, d = user_vec.shape
        N = items.shape[0]
        if items.shape[1] != d:
            raise _lib.NrmsError("%s: items width %d != user_vec width %d" % (who, items.shape[1], d))
        exclude, n_ex = self._exclude_arg(who, exclude, B)
        if bias is not None:
            self._item_bias(who, bias, N, dev)
        inv_t = [float(v) for v in (inv_temperature if hasattr(inv_temperature, "__len__") else [inv_temperature])]
        J = len(inv_t)
        scale = None if bias_scale is None else [float(v) for v in (bias_scale if hasattr(bias_scale, "__len__") else [bias_scale])]
        if scale is not None and len(scale) != J:
            raise _lib.NrmsError("%s: bias_scale has %d entries for %d inv_temperature" % (who, len(scale), J))
        nbytes = self.lib.nrms_logsumexp_dot_workspace_bytes(B, N, d, J, n_ex)
        if nbytes == 0:
            raise _lib.NrmsError("%s: arguments rejected (B=%d, N=%d, d=%d, J=%d; 1 <= J <= 8)" % (who, B, N, d, J))
        ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
        it_arr = (C.c_float * J)(*inv_t)
        sc_arr = None if scale is None else (C.c_float * J)(*scale)
        if return_mass:
            mass = torch.empty(B, J, 2, dtype=torch.int64, device=self.device)
            rc = self.lib.nrms_logsumexp_dot_mass(B, C.c_int64(N), d, J, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias), it_arr,
                                                  sc_arr, _lib.ptr(exclude), n_ex, _lib.ptr(mass), _lib.ptr(ws),
                                                  C.c_size_t(ws.numel() * 8), _stream())
            _lib.check(rc, "nrms_logsumexp_dot_mass")
            return mass
        lse = torch.empty(B, J, dtype=torch.float32, device=self.device)
        zmax = torch.empty(B, J, dtype=torch.float32, device=self.device)
        n_el = torch.empty(B, J, dtype=torch.int32, device=self.device)
        rc = self.lib.nrms_logsumexp_dot(B, C.c_int64(N), d, J, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias), it_arr, sc_arr,
                                         _lib.ptr(exclude), n_ex, _lib.ptr(lse), _lib.ptr(zmax), _lib.ptr(n_el), _lib.ptr(ws),
                                         C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_logsumexp_dot")
        return lse, zmax, n_el

    MMR_WORKSPACE_CAP = 256 << 20      # bytes of Gram workspace per nrms_mmr_rerank call: larger batches go in row chunks

    def mmr_rerank(self, items, short_ids, short_scores, k, lam, return_value=False, return_ild=False):
        """items [N, d] fp32, short_ids [B, M] int64, short_scores [B, M] fp32 (device, contiguous; e.g. top_k's output at
        k = M) -> (ids [B, k] int64, scores [B, k] fp32), then with return_value the value v of every pick [B, k] fp32 and with
        return_ild the intra-list diversity [B] fp32: per user k entries of the shortlist picked greedily by maximal marginal
        relevance, v = lam * rel - (1 - lam) * (largest cosine to the picks so far) (nrms_mmr_rerank).  Entries whose id is
        outside [0, N) or whose score is not finite are padding and are never picked; rows with fewer than k valid entries
        end in id -1 / score -inf / value -inf; the ILD of fewer than two picks is NaN.  lam = 1 keeps a sorted shortlist's
        order.  A row's result does not depend on the rest of the batch, so batches whose workspace would pass
        MMR_WORKSPACE_CAP go in row chunks.  include/nrms_hip.h states the contract."""
        k, lam = int(k), float(lam)
        for name, t, dt in (("items", items, torch.float32), ("short_ids", short_ids, torch.int64),
                            ("short_scores", short_scores, torch.float32)):
            self._check_tensor("mmr_rerank", name, t, dt, 2)
        N, d = items.shape
        B, M = short_ids.shape
        if short_scores.shape != short_ids.shape:
            raise _lib.NrmsError("mmr_rerank: short_scores must be [%d, %d] like short_ids (got %s)" % (B, M, tuple(short_scores.shape)))
        if not 0.0 <= lam <= 1.0:
            raise _lib.NrmsError("mmr_rerank: lam must be in [0, 1] (got %r)" % (lam,))
        per_row = self.lib.nrms_mmr_rerank_workspace_bytes(1, M, d, k)
        if per_row == 0:
            raise _lib.NrmsError("mmr_rerank: arguments rejected (B=%d, M=%d, d=%d, k=%d; 1 <= k <= M <= 256, d >= 1)" % (B, M, d, k))
        chunk = max(1, self.MMR_WORKSPACE_CAP // per_row)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        value = torch.empty(B, k, dtype=torch.float32, device=self.device) if return_value else None
        ild = torch.empty(B, dtype=torch.float32, device=self.device) if return_ild else None
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            nbytes = self.lib.nrms_mmr_rerank_workspace_bytes(nb, M, d, k)
            ws = self._buf("mmr_ws", (nbytes + 7) // 8, torch.int64)
            part = lambda t: None if t is None else t[b0:b0 + nb]
            rc = self.lib.nrms_mmr_rerank(nb, M, d, k, C.c_int64(N), C.c_float(lam), _lib.ptr(items), _lib.ptr(short_ids[b0:b0 + nb]),
                                          _lib.ptr(short_scores[b0:b0 + nb]), _lib.ptr(ids[b0:b0 + nb]), _lib.ptr(scores[b0:b0 + nb]),
                                          _lib.ptr(part(value)), _lib.ptr(part(ild)), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
            _lib.check(rc, "nrms_mmr_rerank")
        out = (ids, scores)
        if return_value:
            out += (value,)
        if return_ild:
            out += (ild,)
        return out

    def attribution(self, ctx, w, items, ids, m, slot_named=None, return_contrib=False):
        """ctx [B, H, d], w [B, H] fp32 (user_parts), items [N, d] fp32, ids [B, K] int64, slot_named [B, H] uint8 or None
        (device, contiguous) -> (top_slots [B, K, m] int32, top_contrib [B, K, m] fp32, total [B, K] fp32, unnamed_share [B, K]
        fp32), then with return_contrib the terms [B, K, H] fp32: the score of item ids[b, j] for user b split over the H history
        slots, c = w[b, h] * (ctx[b, h] . item) (nrms_attribution_dot).  total is their ordered sum; the m largest terms of the
        named slots come first to last, slot -1 / -inf where there are fewer; unnamed_share is the sum over the slots with
        slot_named == 0.  Ids outside [0, N) get total -inf, no reasons and zero terms.  include/nrms_hip.h states the contract."""
        m = int(m)
        self._check_tensor("attribution", "ctx", ctx, torch.float32, 3)
        self._check_tensor("attribution", "w", w, torch.float32, 2)
        self._check_tensor("attribution", "items", items, torch.float32, 2)
        self._check_tensor("attribution", "ids", ids, torch.int64, 2)
        B, H, d = ctx.shape
        N, K = items.shape[0], ids.shape[1]
        if tuple(w.shape) != (B, H) or items.shape[1] != d or ids.shape[0] != B:
            raise _lib.NrmsError("attribution: ctx %s needs w [%d, %d], items [N, %d] and ids [%d, K] (got %s, %s, %s)"
                                 % (tuple(ctx.shape), B, H, d, B, tuple(w.shape), tuple(items.shape), tuple(ids.shape)))
        if slot_named is not None:
            self._check_tensor("attribution", "slot_named", slot_named, torch.uint8, 2)
            if tuple(slot_named.shape) != (B, H):
                raise _lib.NrmsError("attribution: slot_named must be [%d, %d] (got %s)" % (B, H, tuple(slot_named.shape)))
        nbytes = self.lib.nrms_attribution_dot_workspace_bytes(B, H, d, K, m)
        if nbytes == 0:
            raise _lib.NrmsError("attribution: arguments rejected (B=%d, H=%d, d=%d, K=%d, m=%d; 1 <= H <= 64, 1 <= K <= 256, "
                                 "1 <= m <= 8, d >= 1)" % (B, H, d, K, m))
        ws = self._buf("attribution_ws", (nbytes + 7) // 8, torch.int64)
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        top_slots, top_contrib = new((B, K, m), torch.int32), new((B, K, m), torch.float32)
        total, unnamed = new((B, K), torch.float32), new((B, K), torch.float32)
        contrib = new((B, K, H), torch.float32) if return_contrib else None
        rc = self.lib.nrms_attribution_dot(B, H, C.c_int64(N), d, K, m, _lib.ptr(ctx), _lib.ptr(w), _lib.ptr(items), _lib.ptr(ids),
                                           _lib.ptr(slot_named), _lib.ptr(contrib), _lib.ptr(total), _lib.ptr(top_slots),
                                           _lib.ptr(top_contrib), _lib.ptr(unnamed), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
        _lib.check(rc, "nrms_attribution_dot")
        out = (top_slots, top_contrib, total, unnamed)
        return out + (contrib,) if return_contrib else out

    def rank_of(self, user_vec, items, targets, exclude=None, bias=None, *, item_time=None, window=None):
        """user_vec [B, d], items [N, d] fp32, targets [B, T] int64, exclude [B, n_exclude] int64 or None (device, contiguous)
        -> (ranks [B, T] int32, scores [B, T] fp32): the exact 1-based position of every target in top_k's order over the
        whole catalogue (the same score bits, exclude list, NaN rule and tie rule), at any depth and without a [B, N] matrix
        (nrms_rank_dot).  A target outside [0, N) (-1 is the padding value), an excluded one and one with a NaN score come
        back as rank 0 / score -inf; targets do not remove each other.  The kernel takes 32 targets per call: wider
        ``targets`` go in column chunks of 32.  bias [N] fp32 (device, contiguous) or None: top_k's per-item prior, ranks and
        scores are those of user . item + bias[n] (a target whose bias is NaN gets rank 0 / -inf; nrms_rank_dot_biased).  None
        calls nrms_rank_dot as before.  item_time [N] int32 and window [B, 2] int32 (device; both or neither): top_k's time window,
        ranks count the items inside user b's window only and a target outside it gets rank 0 / -inf (nrms_rank_dot_windowed).
        include/nrms_hip.h states the contract."""
        dev = self._cuda_device()
        for name, t, dt in (("user_vec", user_vec, torch.float32), ("items", items, torch.float32), ("targets", targets, torch.int64)):
            self._check_tensor("rank_of", name, t, dt, 2)
        B, d = user_vec.shape
        N = items.shape[0]
        if items.shape[1] != d:
            raise _lib.NrmsError("rank_of: items width %d != user_vec width %d" % (items.shape[1], d))
        if targets.shape[0] != B:
            raise _lib.NrmsError("rank_of: targets must be [%d, T] (got %s)" % (B, tuple(targets.shape)))
        exclude, n_ex = self._exclude_arg("rank_of", exclude, B)
        if bias is not None:
            self._item_bias("rank_of", bias, N, dev)
        item_time, window = self._time_window("rank_of", item_time, window, N, B, dev)
        T_all = targets.shape[1]
        ranks = torch.empty(B, T_all, dtype=torch.int32, device=self.device)
        scores = torch.empty(B, T_all, dtype=torch.float32, device=self.device)
        for t0 in range(0, T_all, 32):
            T = min(32, T_all - t0)
            whole = T == T_all
            tg = targets if whole else targets[:, t0:t0 + T].contiguous()
            rk = ranks if whole else torch.empty(B, T, dtype=torch.int32, device=self.device)
            sc = scores if whole else torch.empty(B, T, dtype=torch.float32, device=self.device)
            nbytes = self.lib.nrms_rank_dot_workspace_bytes(B, N, d, T, n_ex)
            if nbytes == 0:
                raise _lib.NrmsError("rank_of: arguments rejected (B=%d, N=%d, d=%d, T=%d, n_exclude=%d)" % (B, N, d, T, n_ex))
            ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
            if window is not None:
                rc = self.lib.nrms_rank_dot_windowed(B, C.c_int64(N), d, T, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                                     _lib.ptr(item_time), _lib.ptr(window), _lib.ptr(tg), _lib.ptr(exclude), n_ex,
                                                     _lib.ptr(rk), _lib.ptr(sc), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
                _lib.check(rc, "nrms_rank_dot_windowed")
            elif bias is not None:
                rc = self.lib.nrms_rank_dot_biased(B, C.c_int64(N), d, T, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(bias),
                                                   _lib.ptr(tg), _lib.ptr(exclude), n_ex, _lib.ptr(rk), _lib.ptr(sc), _lib.ptr(ws),
                                                   C.c_size_t(ws.numel() * 8), _stream())
                _lib.check(rc, "nrms_rank_dot_biased")
            else:
                rc = self.lib.nrms_rank_dot(B, C.c_int64(N), d, T, _lib.ptr(user_vec), _lib.ptr(items), _lib.ptr(tg), _lib.ptr(exclude),
                                            n_ex, _lib.ptr(rk), _lib.ptr(sc), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
                _lib.check(rc, "nrms_rank_dot")
            if not whole:
                ranks[:, t0:t0 + T] = rk
                scores[:, t0:t0 + T] = sc
        return ranks, scores

    @staticmethod
    def retrieval_metrics(ranks, ks=(10, 100)):
        """ranks [B, T] integer (rank_of: 0 = not ranked) -> dict of float64 [B] device tensors ``recall@<k>`` and
        ``ndcg@<k>`` for every k of ``ks``, and ``mrr``, over each user's n_t = #{j : rank_j > 0} ranked targets:
            recall@k = #{0 < rank_j <= k} / n_t,        mrr = (sum_j 1 / rank_j) / n_t,
            ndcg@k   = sum_{0 < rank_j <= k} 1 / log2(rank_j + 1)  /  sum_{r=1}^{min(n_t, k)} 1 / log2(r + 1).
        This is nrms_impression_metrics's MRR / nDCG with the whole catalogue in place of the impression's shown list.  Every
        value is NaN for a user with n_t = 0.  Callers pass distinct targets (a duplicate would count twice).  Torch ops on
        the ranks' device, no host synchronisation."""
        r = ranks.to(torch.float64)
        ok = ranks > 0
        n_t = ok.sum(dim=1)
        nan = torch.full((), float("nan"), dtype=torch.float64, device=ranks.device)
        none = n_t == 0
        den = n_t.clamp(min=1).to(torch.float64)
        safe = torch.where(ok, r, torch.ones_like(r))
        out = {"mrr": torch.where(none, nan, torch.where(ok, 1.0 / safe, torch.zeros_like(r)).sum(dim=1) / den)}
        gain = 1.0 / torch.log2(safe + 1.0)
        for k in ks:
            k = int(k)
            if k < 1:
                raise ValueError("retrieval_metrics: every k must be >= 1 (got %d)" % k)
            hit = ok & (ranks <= k)
            out["recall@%d" % k] = torch.where(none, nan, hit.sum(dim=1).to(torch.float64) / den)
            # the ideal list puts the n_t targets first: positions 1 .. min(n_t, k); T bounds n_t
            kk = min(k, max(1, ranks.shape[1]))
            ideal = torch.cumsum(1.0 / torch.log2(torch.arange(1, kk + 1, dtype=torch.float64, device=ranks.device) + 1.0), 0)
            idcg = ideal[(n_t.clamp(min=1, max=kk) - 1)]
            out["ndcg@%d" % k] = torch.where(none, nan, torch.where(hit, gain, torch.zeros_like(r)).sum(dim=1) / idcg)
        return out

    # user chunks of top_k_grouped (and of the HieRec query that feeds it) keep the query plus the workspace under this
    retrieval_chunk_bytes = 256 << 20

    def grouped_chunk_users(self, B, N, d, k, G):
        """Users per chunk of a grouped top-k: the most (at least 1) whose [b, G, d] fp32 query and kernel workspace fit in
        ``retrieval_chunk_bytes``."""
        per_user = 4 * G * d + 8 * k * max(1, -(-(N + 31 * G) // 2048))     # query row + at most one k-list per 2048 items
        b = max(1, min(int(B), int(self.retrieval_chunk_bytes) // per_user))
        return b if b < 32 or b == B else b // 32 * 32          # whole 32-user tiles

    def top_k_grouped(self, query, items, item_ids, group_ptr, k, exclude=None):
        """query [B, G, d] fp32, items [N, d] fp32 stored group after group (group g = rows group_ptr[g] .. group_ptr[g + 1]),
        item_ids [N] int32 (distinct, >= 0), group_ptr [G + 1] int64, exclude [B, n_exclude] int64 ids or None (device,
        contiguous) -> (scores [B, k] fp32, ids [B, k] int64): per user the k items of largest query[b, g(n)] . items[n], no
        [B, N] matrix (nrms_topk_grouped_dot).  Order and padding as top_k, with item ids in place of rows.  Users go in
        chunks of grouped_chunk_users; the result does not depend on the chunking."""
        k = int(k)
        for name, t, dt, nd in (("query", query, torch.float32, 3), ("items", items, torch.float32, 2),
                                ("item_ids", item_ids, torch.int32, 1), ("group_ptr", group_ptr, torch.int64, 1)):
            self._check_tensor("top_k_grouped", name, t, dt, nd)
        B, G, d = query.shape
        N = items.shape[0]
        if items.shape[1] != d:
            raise _lib.NrmsError("top_k_grouped: items width %d != query width %d" % (items.shape[1], d))
        if item_ids.shape[0] != N or group_ptr.shape[0] != G + 1:
            raise _lib.NrmsError("top_k_grouped: item_ids must be [%d] and group_ptr [%d] (got %s, %s)"
                                 % (N, G + 1, tuple(item_ids.shape), tuple(group_ptr.shape)))
        exclude, n_ex = self._exclude_arg("top_k_grouped", exclude, B)
        if self.lib.nrms_topk_grouped_dot_workspace_bytes(B, N, d, k, G) == 0:
            raise _lib.NrmsError("top_k_grouped: arguments rejected (B=%d, N=%d, d=%d, k=%d, G=%d; 1 <= k <= 256, G >= 1)"
                                 % (B, N, d, k, G))
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=self.device)
        step = self.grouped_chunk_users(B, N, d, k, G)
        for b0 in range(0, B, step):
            b1 = min(B, b0 + step)
            nbytes = self.lib.nrms_topk_grouped_dot_workspace_bytes(b1 - b0, N, d, k, G)
            ws = self._buf("topk_ws", (nbytes + 7) // 8, torch.int64)
            ex = None if exclude is None else exclude[b0:b1]
            rc = self.lib.nrms_topk_grouped_dot(b1 - b0, C.c_int64(N), d, k, G, _lib.ptr(query[b0:b1]), _lib.ptr(items),
                                                _lib.ptr(item_ids), _lib.ptr(group_ptr), _lib.ptr(ex), n_ex,
                                                _lib.ptr(scores[b0:b1]), _lib.ptr(ids[b0:b1]), _lib.ptr(ws),
                                                C.c_size_t(ws.numel() * 8), _stream())
            _lib.check(rc, "nrms_topk_grouped_dot")
        return scores, ids

    def top_k_sections(self, user, items, item_ids, section_ptr, k, exclude=None, bias=None, slice_tiles=0):
        """user [B, d] fp32, items [N, d] fp32 stored section after section (section g = rows section_ptr[g] ..
        section_ptr[g + 1]), item_ids [N] int32 (distinct, >= 0), section_ptr [G + 1] int64, exclude [B, n_exclude] int64 ids or
        None, bias [N] fp32 BY ROW or None (device, contiguous) -> (scores [B, G, k] fp32, ids [B, G, k] int64): per user and
        section the k items of largest user . item (+ bias[row]), no [B, N] matrix (nrms_topk_sections_dot).  Order and
        padding as top_k, with item ids in place of rows; an empty section gives an all-padding row.  slice_tiles: 0 (the
        library chooses) or the 32-row tiles per slice of the launch geometry; the result does not depend on it.  Users go in
        chunks whose workspace stays under ``retrieval_chunk_bytes``; the result does not depend on the chunking."""
        k, slice_tiles = int(k), int(slice_tiles)
        for name, t, dt, nd in (("user", user, torch.float32, 2), ("items", items, torch.float32, 2),
                                ("item_ids", item_ids, torch.int32, 1), ("section_ptr", section_ptr, torch.int64, 1)):
            self._check_tensor("top_k_sections", name, t, dt, nd)
        B, d = user.shape
        N = items.shape[0]
        G = section_ptr.shape[0] - 1
        if items.shape[1] != d:
            raise _lib.NrmsError("top_k_sections: items width %d != user width %d" % (items.shape[1], d))
        if item_ids.shape[0] != N:
            raise _lib.NrmsError("top_k_sections: item_ids must be [%d] (got %s)" % (N, tuple(item_ids.shape)))
        exclude, n_ex = self._exclude_arg("top_k_sections", exclude, B)
        if bias is not None:
            self._item_bias("top_k_sections", bias, N, self._cuda_device())
        query = self.lib.nrms_topk_sections_dot_workspace_bytes
        if G < 1 or query(B, N, d, k, G, slice_tiles) == 0:
            raise _lib.NrmsError("top_k_sections: arguments rejected (B=%d, N=%d, d=%d, k=%d, G=%d, slice_tiles=%d; 1 <= k <= 256, "
                                 "1 <= G <= 4096, B * G * k < 2^31)" % (B, N, d, k, G, slice_tiles))
        scores = torch.empty(B, G, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(B, G, k, dtype=torch.int64, device=self.device)
        # the most users (at least 1, whole 32-user tiles) whose workspace fits: the entries grow with b, the tables do not
        step = B
        while step > 1 and query(step, N, d, k, G, slice_tiles) > int(self.retrieval_chunk_bytes):
            step = max(1, step // 2)
        if 32 <= step < B:
            step = step // 32 * 32
        for b0 in range(0, B, max(1, step)):
            b1 = min(B, b0 + step)
            nbytes = query(b1 - b0, N, d, k, G, slice_tiles)
            ws = self._buf("topk_ws", (nbytes + 15) // 16 * 2, torch.int64)
            ex = None if exclude is None else exclude[b0:b1]
            rc = self.lib.nrms_topk_sections_dot(b1 - b0, C.c_int64(N), d, k, G, slice_tiles, _lib.ptr(user[b0:b1]), _lib.ptr(items),
                                                 _lib.ptr(item_ids), _lib.ptr(section_ptr), _lib.ptr(bias), _lib.ptr(ex), n_ex,
                                                 _lib.ptr(scores[b0:b1]), _lib.ptr(ids[b0:b1]), _lib.ptr(ws),
                                                 C.c_size_t(ws.numel() * 8), _stream())
            _lib.check(rc, "nrms_topk_sections_dot")
        return scores, ids

    # ---- inference with unique-title caching (SURVEY f-1) -------------------------------------
    def group_rows(self, rows):
        """rows [N, L] int64 (device) -> (inverse [N] int32, rep_rows [U] int32, U): exact grouping of equal rows
        by a device hash table (nrms_title_dedup): rows[rep_rows[inverse[t]]] == rows[t].  One host read-back (U)."""
        N, L = rows.shape
        size = 1 << max(int(2 * N - 1).bit_length(), 4)
        table = self._buf("dedup_table", size, torch.int32)
        inverse = torch.empty(N, dtype=torch.int32, device=self.device)
        rep = self._buf("dedup_rep", N, torch.int32)
        n_unique = self._buf("dedup_count", 1, torch.int32)
        rc = self.lib.nrms_title_dedup(_lib.ptr(rows), C.c_int64(N), int(L), _lib.ptr(table), C.c_int64(size),
                                       _lib.ptr(inverse), _lib.ptr(rep), _lib.ptr(n_unique), _stream())
        _lib.check(rc, "nrms_title_dedup")
        U = int(n_unique.item())
        return inverse, rep[:U], U

    def unique_titles(self, ids):
        """ids [N, L] -> (one title per group [U, L], inverse [N] int32) with ids == uniq[inverse]."""
        inverse, rep, _ = self.group_rows(ids)
        return ids.index_select(0, rep), inverse

    def click_scores_indexed(self, news_vec, index, user_vec, B, Cn, cand_mask=None):
        """scores [B, Cn] with candidate slot (b, c) = row index[b*Cn + c] of news_vec [n, d]."""
        out = torch.empty(B, Cn, dtype=torch.float32, device=self.device)
        rc = self.lib.nrms_click_score_indexed(B, Cn, news_vec.shape[1], _lib.ptr(news_vec), C.c_int64(news_vec.shape[0]),
                                               _lib.ptr(index), _lib.ptr(user_vec), _lib.ptr(cand_mask), _lib.ptr(out),
                                               _stream())
        _lib.check(rc, "nrms_click_score_indexed")
        return out

    def forward_dedup(self, flat, hist_ids, cand_ids, cand_mask):
        """Same scores as forward(training=False), but every distinct title of the batch is encoded
        once (the reference encodes all B*(H+C) slots, 350 per user at C=300, most of them padding
        or repeats: train_eval.py:229-273 / data_handler.py:174-177); candidate vectors are read by index."""
        B, H, L = hist_ids.shape
        Cn = cand_ids.shape[1]
        d = self.dims.word_embed_size
        N = B * (H + Cn)
        self.poll_ids()
        ids = self._buf("ids_eval", N * L, torch.int64)[:N * L].view(N, L)
        self.sanitize_ids(hist_ids.reshape(B * H, L).contiguous(), ids[:B * H])
        self.sanitize_ids(cand_ids.reshape(B * Cn, L).contiguous(), ids[B * H:])
        uniq, inverse = self.unique_titles(ids)
        vec = self.encode_titles(flat, uniq, tag="news_eval", trusted_ids=True)
        hist = vec.index_select(0, inverse[:B * H]).view(B, H, d)
        user = self.encode_users(flat, hist, tag="user_eval")
        if cand_mask is not None:
            cand_mask = cand_mask.contiguous()
        return self.click_scores_indexed(vec, inverse[B * H:], user, B, Cn, cand_mask), int(uniq.shape[0])

    # persistent news-vector cache across evaluation batches, keyed by the news ids the batch dict carries
    # (browsed_ids / candidate_ids, data_handler.py:204-222; 0 = padding slot = all-padding title)
    def news_cache_begin(self, capacity=1 << 14):
        d = self.dims.word_embed_size
        old = getattr(self, "_news_cache_store", None)
        if old is not None and old[0].shape[1] == d:                  # buffers are kept between evaluations; only the
            vec, have = old                                           # validity bits are cleared (weights changed)
            have.zero_()
        else:
            vec = torch.empty(capacity, d, dtype=torch.float32, device=self.device)
            have = torch.zeros(capacity, dtype=torch.bool, device=self.device)
        self._news_cache = dict(vec=vec, have=have, encoded=0, hits=0)

    def news_cache_end(self):
        st = getattr(self, "_news_cache", None)
        self._news_cache = None
        if st is None:
            return None
        self._news_cache_store = (st["vec"], st["have"])
        return dict(encoded=st["encoded"], lookups=st["hits"])

    def forward_cached(self, flat, hist_ids, cand_ids, hist_news, cand_news, cand_mask):
        """forward(training=False) for batches that carry news ids: a news item is encoded the first time it is
        seen during the evaluation (weights are constant between news_cache_begin / news_cache_end) and looked up
        afterwards -- the offline news-vector caching get_news_vector exists for (nrms_v0.py:278-289)."""
        st = self._news_cache
        B, H, L = hist_ids.shape
        Cn = cand_ids.shape[1]
        d = self.dims.word_embed_size
        N = B * (H + Cn)
        news = torch.cat([hist_news.reshape(-1), cand_news.reshape(-1)]).to(torch.int64).contiguous()
        inverse, rep, _ = self.group_rows(news.view(N, 1))
        u = news.index_select(0, rep)                                  # the distinct news ids of the batch
        lo, top = (int(v) for v in torch.stack([u.min(), u.max()]).tolist()) if N else (0, 0)
        if lo < 0:
            raise _lib.NrmsError("negative news id in browsed_ids / candidate_ids")
        if top + 1 > st["vec"].shape[0]:                              # grow (amortised doubling)
            cap = max(top + 1, 2 * st["vec"].shape[0])
            vec = torch.empty(cap, d, dtype=torch.float32, device=self.device)
            have = torch.zeros(cap, dtype=torch.bool, device=self.device)
            vec[:st["vec"].shape[0]] = st["vec"]
            have[:st["have"].shape[0]] = st["have"]
            st["vec"], st["have"] = vec, have
        need = ~st["have"].index_select(0, u)
        rows = rep[need].to(torch.int64)                               # a slot of the batch holding each news item not cached yet
        if rows.numel():
            missing = u[need]
            titles = torch.where((rows < B * H).unsqueeze(1),
                                 hist_ids.reshape(B * H, L).index_select(0, rows.clamp(max=B * H - 1)),
                                 cand_ids.reshape(B * Cn, L).index_select(0, (rows - B * H).clamp(min=0)))
            st["vec"].index_copy_(0, missing, self.encode_titles(flat, titles.contiguous(), tag="news_eval"))
            st["have"][missing] = True
            st["encoded"] += int(missing.numel())
        st["hits"] += N
        hist = st["vec"].index_select(0, news[:B * H]).view(B, H, d)
        user = self.encode_users(flat, hist, tag="user_eval")
        if cand_mask is not None:
            cand_mask = cand_mask.contiguous()
        return self.click_scores_indexed(st["vec"], news[B * H:].to(torch.int32), user, B, Cn, cand_mask)

    def dropout_keep_mask(self, seed, site, n_rows, p_drop, d=None, fp16_ctx=False):
        """Keep mask of a dropout site over [n_rows, d] (d defaults to the model width).  fp16_ctx: the context dropout
        of the fp16 mode -- padded width 320 (32 columns per head), 16-bit-field scheme, the two middle index bits of a
        column inside its head block swapped (include/nrms_hip.h, NRMS_DROPOUT_FIELDS16); returned in natural column order."""
        d = self.dims.word_embed_size if d is None else int(d)
        if fp16_ctx:
            d, site = _lib.NRMS_FP16_DP, site | _lib.NRMS_DROPOUT_FIELDS16
        keep = torch.empty(n_rows * d, dtype=torch.uint8, device=self.device)
        rc = self.lib.nrms_dropout_keep_mask(C.c_uint64(seed), site, C.c_int64(n_rows), d, C.c_float(p_drop),
                                             _lib.ptr(keep), _stream())
        _lib.check(rc, "nrms_dropout_keep_mask")
        keep = keep.view(n_rows, d)
        if fp16_ctx:
            col = torch.arange(d, device=self.device)
            a, b, c, e = col >> 4, (col >> 3) & 1, (col >> 2) & 1, col & 3
            keep = keep.index_select(1, 16 * a + 8 * c + 4 * b + e)
        return keep

    # ---- timing (bench.py roofline leg) --------------------------------------------------
    def timing(self, enable: bool):
        self.lib.nrms_timing_enable(1 if enable else 0)

    def timing_reset(self):
        self.lib.nrms_timing_reset()

    def timing_read(self, prefix: str):
        ms, n = C.c_double(0.0), C.c_int64(0)
        _lib.check(self.lib.nrms_timing_read(prefix.encode(), C.byref(ms), C.byref(n)), "nrms_timing_read")
        return ms.value, n.value
