"""Host-side driver of nrms_bert (the reference's model/nrms.py: Model :297-366, BertNewsEncoder :216-256,
UserEncoder :258-272) over the C ABI (include/nrms_hip.h): the news-vector layer (nrms_newsvec_fwd / _bwd, csrc/newsvec.hip),
the user encoder on the encoder chain (MHSA with output_linear, pairwise and pooling masks, dropout on the attention
probabilities), click scores.

Layout in HBM (fp32):
  flat parameter / gradient buffer
      [ news table n_news*E | news_dense.0 W (E*E), b | user: Wq|Wk|Wv (3E*E), bq|bk|bv, Wo, bo, Wa (Q*E), ba, qv ]
  slots   N = B*H history slots (user-major) then B*C candidate slots
  nv      [N, E]: rows [0, B*H) are the user encoder's input, rows [B*H, N) the candidate vectors
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .engine import FlatLayout, NRMSEngine, _stream

# the user encoder's attention-probability dropout (site 2) draws from the step's seed xor this, the news vectors (site 4)
# from the seed itself
USER_SEED_SALT = 0x2545F4914F6CDD1D


@dataclass(frozen=True)
class BertDims:
    """The table's shape and config.py:72,77 as nrms.py reads them (every width is the table's E)."""
    n_news: int
    width: int
    user_heads_num: int
    query_vector_dim_large: int
    style: str = "bert"

    @property
    def n_words(self):                  # rows the id checks validate against (NRMSEngine.sanitize_ids)
        return self.n_news

    @property
    def word_embed_size(self):          # NRMSEngine.dropout_keep_mask's default width
        return self.width


def bert_entries(dims: BertDims):
    """(name, shape, encoder, role) in flat-buffer order: the table first, W_Q | W_K | W_V adjacent (the chain's [3E, E])."""
    E, Q = dims.width, dims.query_vector_dim_large
    if E % 4 or Q % 4:
        raise ValueError("the news-vector width and query_vector_dim_large must be multiples of 4 (got %d, %d)" % (E, Q))
    out = [("news_encoder.news_embedding.weight", (dims.n_news, E), "news_encoder", "table"),
           ("news_encoder.news_dense.0.weight", (E, E), None, None),
           ("news_encoder.news_dense.0.bias", (E,), None, None)]
    a = "user_encoder.multi_head_self_attention."
    out += [(a + "linear_layers.%d.weight" % i, (E, E), "user_encoder", r) for i, r in enumerate(("wq", "wk", "wv"))]
    out += [(a + "linear_layers.%d.bias" % i, (E,), "user_encoder", r) for i, r in enumerate(("bq", "bk", "bv"))]
    out += [(a + "output_linear.weight", (E, E), "user_encoder", "wo"), (a + "output_linear.bias", (E,), "user_encoder", "bo"),
            ("user_encoder.additive_attention.linear.weight", (Q, E), "user_encoder", "wa"),
            ("user_encoder.additive_attention.linear.bias", (Q,), "user_encoder", "ba"),
            ("user_encoder.additive_attention.query_vector", (Q,), "user_encoder", "qv")]
    return out


class BertEngine(NRMSEngine):
    """One nrms_bert forward / backward on one GPU.  Inherits the shape-independent pieces of the NRMS engine (buffers, id
    counter, click scores, CE, Adam, metrics, top-k, dropout replay, timers)."""

    def __init__(self, dims: BertDims, device, precision="fp32"):
        super().__init__(dims, device, precision=precision, layout=FlatLayout(dims, bert_entries(dims)))

    def set_precision(self, precision):
        """fp32, bf16x3 or bf16 dense products; there are no fused fp16 kernels for this model, so "fp16" runs in bf16x3."""
        if precision not in _lib.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(_lib.PRECISIONS))
        self.precision = "bf16x3" if precision == "fp16" else precision
        self.pad_row_zero = False

    def _off(self, name):
        return self.layout.entries[name][0]

    def _raise_bad_ids(self):
        n = int(self._bad_host.item())
        if n:
            self._bad_ids.zero_()
            self._bad_host.zero_()
            raise _lib.NrmsError("%d news id(s) outside [0, %d) reached the news-vector lookup (read as news id 0 on the "
                                 "device; the data and the vector table disagree)" % (n, self.dims.n_news))

    # ---- news vectors ------------------------------------------------------------------------------------------------
    def _nv_desc(self, n_slots, p_drop, seed):
        return _lib.NewsvecDesc(n_slots=int(n_slots), n_rows=self.dims.n_news, d=self.dims.width,
                                precision=_lib.PRECISIONS[self.precision], p_drop=float(p_drop), seed=int(seed) & 0xFFFFFFFFFFFFFFFF)

    def _nv_ptrs(self, base):
        return (C.c_void_p(base + 4 * self._off("news_encoder.news_embedding.weight")),
                C.c_void_p(base + 4 * self._off("news_encoder.news_dense.0.weight")),
                C.c_void_p(base + 4 * self._off("news_encoder.news_dense.0.bias")))

    def _nv_bufs(self, desc, tag):
        ns = int(self.lib.nrms_newsvec_saved_bytes(C.byref(desc)))
        nw = int(self.lib.nrms_newsvec_workspace_bytes(C.byref(desc)))
        if ns == 0 or nw == 0:
            _lib.check(-1, "nrms_newsvec_*_bytes")
        # torch's allocator hands out 512-byte aligned blocks: the 256-byte alignment the library asks for
        return self._buf(tag + ".nv_saved", (ns + 3) // 4, torch.int32), ns, self._buf("nv_ws", (nw + 3) // 4), nw

    def news_vectors(self, flat, ids, p_drop=0.0, seed=0, tag="news", out=None):
        """ids [N] int64 news ids (device) -> dropout(table[ids] W^T + b) [N, E]; the distinct ids and slot maps stay in the tag's
        saved buffer for news_vectors_backward.  Ids outside the table are read as id 0 and counted (poll_ids / check_ids)."""
        N = ids.numel()
        if out is None:
            out = torch.empty(N, self.dims.width, dtype=torch.float32, device=self.device)
        self.poll_ids()
        desc = self._nv_desc(N, p_drop, seed)
        saved, ns, ws, nw = self._nv_bufs(desc, tag)
        table, w, b = self._nv_ptrs(flat.data_ptr())
        rc = self.lib.nrms_newsvec_fwd(C.byref(desc), _lib.ptr(ids.contiguous()), table, w, b, _lib.ptr(out), _lib.ptr(saved),
                                       C.c_size_t(ns), _lib.ptr(self._bad_ids), _lib.ptr(ws), C.c_size_t(nw), _stream())
        _lib.check(rc, "nrms_newsvec_fwd")
        self.note_bad_ids()
        return out

    def news_vectors_backward(self, flat, gflat, dout, p_drop, seed, tag="news"):
        desc = self._nv_desc(dout.shape[0], p_drop, seed)
        saved, ns, ws, nw = self._nv_bufs(desc, tag)
        table, w, _ = self._nv_ptrs(flat.data_ptr())
        gt, gw, gb = self._nv_ptrs(gflat.data_ptr())
        rc = self.lib.nrms_newsvec_bwd(C.byref(desc), table, w, _lib.ptr(dout.contiguous()), _lib.ptr(saved), C.c_size_t(ns), gt, gw, gb,
                                       _lib.ptr(ws), C.c_size_t(nw), _stream())
        _lib.check(rc, "nrms_newsvec_bwd")

    def distinct_ids(self, n_slots, tag="news"):
        """(n_unique int32 [1], distinct ids int32 [n_slots], the first n_unique valid, ascending) of the tag's last forward."""
        desc = self._nv_desc(n_slots, 0.0, 0)
        saved, _, _, _ = self._nv_bufs(desc, tag)
        n = torch.empty(1, dtype=torch.int32, device=self.device)
        ids = torch.empty(max(int(n_slots), 1), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.nrms_newsvec_distinct(C.byref(desc), _lib.ptr(saved), _lib.ptr(n), _lib.ptr(ids), _stream()),
                   "nrms_newsvec_distinct")
        return n, ids

    def encode_rows(self, flat, out=None):
        """Every row of the table through news_dense, no dropout -> [n_news, E] (catalogue, evaluation cache)."""
        V, E = self.dims.n_news, self.dims.width
        if out is None:
            out = torch.empty(V, E, dtype=torch.float32, device=self.device)
        prec = _lib.PRECISIONS[self.precision]
        nb = int(self.lib.nrms_newsvec_rows_workspace_bytes(C.c_int64(V), E, prec))
        ws = self._buf("nv_rows_ws", (nb + 3) // 4)
        table, w, b = self._nv_ptrs(flat.data_ptr())
        rc = self.lib.nrms_newsvec_rows_fwd(C.c_int64(V), E, prec, table, w, b, _lib.ptr(out), _lib.ptr(ws), C.c_size_t(ws.numel() * 4),
                                            _stream())
        _lib.check(rc, "nrms_newsvec_rows_fwd")
        return out

    # ---- user encoder ------------------------------------------------------------------------------------------------
    def _udesc(self, B, H, p_attn, seed):
        d = self.dims
        return _lib.EncoderDesc(n_seq=B, seq_len=H, d_model=d.width, n_heads=d.user_heads_num, q_dim=d.query_vector_dim_large,
                                vocab=0, p_drop_embed=0.0, p_drop_ctx=0.0, precision=_lib.PRECISIONS[self.precision],
                                use_output_proj=1, mask_mode=3, flags=0, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, loss_scale=0.0,
                                p_drop_attn=float(p_attn))

    def _uacts(self, tag, desc):
        M, E, Q = desc.n_seq * desc.seq_len, desc.d_model, desc.q_dim
        dp = lambda z: z.data_ptr()
        nbytes = int(self.lib.nrms_encoder_fwd_scratch_bytes(C.byref(desc)))
        return _lib.EncoderActs(x=None, qkv=dp(self._buf(tag + ".qkv", M * 3 * E)), attn=dp(self._buf(tag + ".attn", M * E)),
                                ctx=dp(self._buf(tag + ".ctx", M * E)), t=dp(self._buf(tag + ".t", M * Q)), w=dp(self._buf(tag + ".w", M)),
                                scratch=dp(self._buf("fwd_scratch", (nbytes + 3) // 4)))

    def encode_users(self, flat, x, mask, p_attn=0.0, seed=0, tag="user_eval", out=None):
        """x [B, H, E] history vectors, mask [B, H] uint8 (browsed_mask) -> [B, E] (UserEncoder.forward, nrms.py:269-272)."""
        B, H, E = x.shape
        if out is None:
            out = torch.empty(B, E, dtype=torch.float32, device=self.device)
        desc = self._udesc(B, H, p_attn, seed)
        w = self._ptrs(_lib.EncoderWeights, flat, "user_encoder")
        rc = self.lib.nrms_encoder_fwd(C.byref(desc), C.byref(w), None, _lib.ptr(x.contiguous()), _lib.ptr(mask.contiguous()),
                                       C.byref(self._uacts(tag, desc)), _lib.ptr(out), _stream())
        _lib.check(rc, "nrms_encoder_fwd(user)")
        return out

    def user_parts(self, flat, x, mask):
        """encode_users' inference pass on buffers of its own -> (user [B, E], ctx [B, H, E], w [B, H]): user[b] = sum_h w[b, h]
        ctx[b, h], masked slots with w = 0 (NRMSEngine.user_parts; the input of `attribution`)."""
        B, H, E = x.shape
        return (self.encode_users(flat, x, mask, tag="user_parts"),) + self._parts_of("user_parts", B, H, E)

    # ---- full model ----------------------------------------------------------------------------------------------------
    def forward(self, flat, browsed_ids, cand_ids, browsed_mask, cand_mask, training, p_drop=0.0, seed=0):
        """Model.forward (nrms.py:317-366).  browsed_ids [B, H], cand_ids [B, C] int64, browsed_mask [B, H] uint8, cand_mask
        [B, C] uint8 or None (device) -> scores [B, C]."""
        B, H = browsed_ids.shape
        Cn = cand_ids.shape[1]
        E = self.dims.width
        N = B * (H + Cn)
        sfx = "" if training else "_eval"
        ids = self._buf("slot_ids" + sfx, N, torch.int64)[:N]
        ids[:B * H].copy_(browsed_ids.reshape(-1))
        ids[B * H:].copy_(cand_ids.reshape(-1))
        nv = self._buf("news_vec" + sfx, N * E)[:N * E].view(N, E)
        self.news_vectors(flat, ids, p_drop, seed, "news" + sfx, out=nv)
        bmask = browsed_mask.contiguous()
        user = self._buf("user_vec" + sfx, B * E)[:B * E].view(B, E)
        self.encode_users(flat, nv[:B * H].view(B, H, E), bmask, p_drop, seed ^ USER_SEED_SALT, "user" + sfx, out=user)
        if cand_mask is not None:
            cand_mask = cand_mask.contiguous()
        scores = self.click_scores(nv[B * H:].view(B, Cn, E), user, cand_mask)
        if training:
            self._gen += 1
            self._saved = dict(B=B, H=H, C=Cn, N=N, nv=nv, user=user, bmask=bmask, mask=cand_mask, p=float(p_drop), seed=seed,
                               gen=self._gen)
        return scores

    def backward(self, flat, gflat, dscores=None, gen=None, table_grad_ready=None):
        """Every parameter gradient of the saved training forward into gflat (same layout as flat; the table rows of the
        batch's news are stored, the rest accumulated).  dscores None: the pooled loss's gradient (NRMSEngine.backward)."""
        E = self.dims.width
        sv, dnv, duser = self._head_backward(dscores, gen, E)
        B, H, Cn, N = sv["B"], sv["H"], sv["C"], sv["N"]
        p, seed = sv["p"], sv["seed"]
        nv = sv["nv"]
        desc_u = self._udesc(B, H, p, seed ^ USER_SEED_SALT)
        ws = self._bwd_workspace(desc_u)
        wu, gu = self._ptrs(_lib.EncoderWeights, flat, "user_encoder"), self._ptrs(_lib.EncoderGrads, gflat, "user_encoder")
        rc = self.lib.nrms_encoder_bwd(C.byref(desc_u), C.byref(wu), None, C.c_void_p(nv.data_ptr()), _lib.ptr(sv["bmask"]),
                                       C.byref(self._uacts("user", desc_u)), _lib.ptr(duser), C.byref(gu), C.c_void_p(dnv.data_ptr()),
                                       _lib.ptr(ws), C.c_size_t(ws.numel() * 4), _stream())
        _lib.check(rc, "nrms_encoder_bwd(user)")
        self.news_vectors_backward(flat, gflat, dnv, p, seed, "news")
        if table_grad_ready is not None:
            table_grad_ready()

    # ---- evaluation: every news id through news_dense once per evaluation ------------------------------------------------
    def news_cache_begin(self, capacity=None):
        self._news_cache = dict(vec=None, encoded=0, hits=0)

    def news_cache_end(self):
        st = getattr(self, "_news_cache", None)
        self._news_cache = None
        return None if st is None else dict(encoded=st["encoded"], lookups=st["hits"])

    def forward_cached(self, flat, browsed_ids, cand_ids, browsed_mask, cand_mask):
        """forward(training=False, p_drop=0) from the table encoded once (encode_rows, at the first batch after
        news_cache_begin: weights are constant until news_cache_end)."""
        st = self._news_cache
        if st["vec"] is None:
            st["vec"] = self.encode_rows(flat, out=self._buf("news_cache_rows", self.dims.n_news * self.dims.width)
                                         [:self.dims.n_news * self.dims.width].view(self.dims.n_news, self.dims.width))
            st["encoded"] = self.dims.n_news
        vec = st["vec"]
        B, H = browsed_ids.shape
        Cn = cand_ids.shape[1]
        N = B * (H + Cn)
        self.poll_ids()
        ids = self._buf("slot_ids_cached", N, torch.int64)[:N]
        self.sanitize_ids(browsed_ids.reshape(-1).contiguous(), ids[:B * H])
        self.sanitize_ids(cand_ids.reshape(-1).contiguous(), ids[B * H:])
        st["hits"] += N
        user = self.encode_users(flat, vec.index_select(0, ids[:B * H]).view(B, H, self.dims.width), browsed_mask)
        if cand_mask is not None:
            cand_mask = cand_mask.contiguous()
        return self.click_scores_indexed(vec, ids[B * H:].to(torch.int32), user, B, Cn, cand_mask)
