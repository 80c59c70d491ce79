"""``nrms_bert`` on MI355X: NRMS over pretrained per-news vectors -- the reference's model/nrms.py: Model
(:297-366), BertNewsEncoder (:216-256), UserEncoder (:258-272), MultiHeadSelfAttention (:52-83), Attention (:24-49),
AdditiveAttention (:86-112); the reference's results table lists it as NRMS-bert1024.

Each news id looks up a fine-tunable row of ``np.load(config.data_path + config.bert_embedding_pretrained)["embeddings"]``
([n_news, E] float32, row r = news id r, NO padding_idx: row 0 is an ordinary trainable row and the padding slots of an
empty history train it), goes through ``news_dense`` (one Linear(E, E)) and dropout; the user encoder is MHSA with
output_linear and additive attention, both masked by ``browsed_mask`` (pairwise mask_i * mask_j in the attention, dropout on
the attention probabilities).  Every width is the table's E: ``config.bert_embed_size`` must equal it, heads come from
``config.user_heads_num``, the additive width from ``config.query_vector_dim_large``.  ``config.news_feature_size`` is NOT
read: the reference sizes its user encoder by it (nrms.py:263) and crashes at the first forward whenever it differs from E
(``__nrms__`` sets it to 800 for nrms_naml).

Same plugin contract as the other models (``Model(config)``, ``forward(batch) -> scores [B, C]`` with masked candidates at
-1e9, ``train_step``, the autograd path); the 14 parameter names and ``state_dict()`` order are the reference's, so
checkpoints interchange.  Batch keys read: ``browsed_ids``, ``candidate_ids`` (0 = padding slot), ``browsed_mask`` and
``candidate_mask`` (nrms.py:317-346), as data_handler.MyDataset / DeviceFeed emit them.

Precision: "fp32", "bf16x3" or "bf16" dense products; there are no fused fp16 kernels for this model, so "fp16" is served as
bf16x3 (as nrms_naml does).  The hot path is HIP: csrc/newsvec.hip for the news vectors, the encoder chain for the user
encoder.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..bert_engine import BertDims, BertEngine, bert_entries
from ..engine import FlatLayout
from ._flat_model import FlatHipModel
from . import nrms_hip


class _BertNewsEncoderParams(nn.Module):
    """nrms.py:219-229: Embedding.from_pretrained(freeze=False) -- no padding_idx -- and Sequential(Linear(E, E))."""

    def __init__(self, table):
        super().__init__()
        E = table.shape[1]
        self.news_embedding = nn.Embedding.from_pretrained(table, freeze=False)
        self.news_dense = nn.Sequential(nn.Linear(E, E))


class _MultiHeadSelfAttentionParams(nn.Module):
    """nrms.py:57-70: three Linear(E, E) in a ModuleList + output_linear, torch's default initialisation."""

    def __init__(self, h, d_model):
        super().__init__()
        self.h = h
        self.linear_layers = nn.ModuleList([nn.Linear(d_model, d_model) for _ in range(3)])
        self.output_linear = nn.Linear(d_model, d_model)


class _AdditiveAttentionParams(nn.Module):
    """nrms.py:87-96."""

    def __init__(self, query_vector_dim, input_vector_dim):
        super().__init__()
        self.linear = nn.Linear(input_vector_dim, query_vector_dim)
        self.query_vector = nn.Parameter(torch.empty(query_vector_dim).uniform_(-0.1, 0.1))


class _UserEncoderParams(nn.Module):
    """nrms.py:260-266 with the table's width in place of news_feature_size."""

    def __init__(self, h, width, q):
        super().__init__()
        self.multi_head_self_attention = _MultiHeadSelfAttentionParams(h, width)
        self.additive_attention = _AdditiveAttentionParams(q, width)


def load_news_vectors(config):
    """[n_news, E] float32 of config.data_path + config.bert_embedding_pretrained (nrms.py:223-225)."""
    path = config.data_path + config.bert_embedding_pretrained
    try:
        arr = np.load(path)["embeddings"]
    except FileNotFoundError:
        raise FileNotFoundError("nrms_bert: the pretrained news-vector file %s (config.data_path + config.bert_embedding_pretrained, "
                                "an .npz with 'embeddings' [n_news, E]) does not exist" % path) from None
    return torch.tensor(np.asarray(arr, dtype=np.float32))


class Model(nrms_hip.Model):
    """nrms.Model: candidate and history news ids -> click logits.  Shares nrms_hip.Model's catalogue retrieval (recommend,
    check_recommend_ids) through the _catalogue_width / _catalogue_users hooks."""

    def __init__(self, config, pretrained_news_vectors=None):
        FlatHipModel.__init__(self)
        self.config = config
        table = (load_news_vectors(config) if pretrained_news_vectors is None
                 else torch.as_tensor(np.asarray(pretrained_news_vectors, dtype=np.float32)).clone())
        if table.dim() != 2:
            raise ValueError("nrms_bert: the news-vector table must be [n_news, E], got %s" % (tuple(table.shape),))
        V, E = (int(x) for x in table.shape)
        if int(config.bert_embed_size) != E:
            raise ValueError("nrms_bert: config.bert_embed_size %d != the news-vector table's width %d (%s)"
                             % (config.bert_embed_size, E, config.bert_embedding_pretrained))
        h, q = int(config.user_heads_num), int(config.query_vector_dim_large)
        if E % h:
            raise ValueError("nrms_bert: the width %d is not a multiple of user_heads_num %d" % (E, h))
        self.news_encoder = _BertNewsEncoderParams(table)
        self.user_encoder = _UserEncoderParams(h, E, q)
        self._dims = BertDims(n_news=V, width=E, user_heads_num=h, query_vector_dim_large=q)
        self._finish(FlatLayout(self._dims, bert_entries(self._dims)), table.device)

    def _make_engine(self, device, precision):
        return BertEngine(self._dims, device, precision=precision)

    def _engine_args(self, batch, dev):
        """'browsed_ids' [B, H], 'candidate_ids' [B, C], 'browsed_mask' [B, H] and 'candidate_mask' [B, C] (nrms.py:317-346;
        without a browsed_mask the non-zero browsed ids are the history)."""
        get = batch.get if hasattr(batch, "get") else batch.__getitem__
        bi = torch.as_tensor(get("browsed_ids")).to(dev, dtype=torch.int64, non_blocking=True)
        ci = torch.as_tensor(get("candidate_ids")).to(dev, dtype=torch.int64, non_blocking=True)
        bm = get("browsed_mask")
        bm = (bi != 0) if bm is None else torch.as_tensor(bm).to(dev, non_blocking=True)
        cm = get("candidate_mask")
        if cm is not None:
            cm = torch.as_tensor(cm).to(dev, dtype=torch.uint8, non_blocking=True)
        return bi, ci, bm.to(torch.uint8), cm

    def _infer(self, batch, args, p_drop, seed):
        if p_drop == 0.0 and self._engine._news_cache is not None:
            return self._engine.forward_cached(self._flat, *args)       # inside train_eval.evaluate / test
        return self._engine.forward(self._flat, *args, training=False, p_drop=p_drop, seed=seed)

    def get_news_vector(self, *a, **k):
        raise _lib.NrmsError("nrms_bert has no get_news_vector / get_user_vector / get_prediction (nrms.py:297-366); "
                             "encode_catalogue gives every news vector")

    get_user_vector = get_prediction = get_news_vector

    # ---- retrieval over the whole catalogue (recommend itself is nrms_hip.Model's) ------------------------------------------
    @torch.no_grad()
    def encode_catalogue(self, titles=None, **unused):
        """Every row of the news-vector table through news_dense, no dropout, whatever the train / eval mode -> [n_news, E]
        (row r = news id r).  ``titles`` (what train_eval.recommend passes) is ignored: the table is the catalogue."""
        self._prepare()
        return self._engine.encode_rows(self._flat)

    def _catalogue_width(self):
        return self._dims.width

    def _catalogue_users(self, hist, browsed=None):
        mask = (browsed != 0).to(torch.uint8)
        return self._engine.encode_users(self._flat, hist, mask)

    def _catalogue_user_parts(self, hist, browsed=None):
        mask = (browsed != 0).to(torch.uint8)
        return self._engine.user_parts(self._flat, hist, mask)
