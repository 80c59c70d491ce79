"""``nrms_naml`` on MI355X: NRMS over title + abstract + category / sub-category embeddings with a
LayerNorm on the history and an 800-wide user encoder -- /root/reference/MIND_2020/model/nrms_naml.py:
14-41 (attention with dropout on the probabilities), 42-75 (MHSA with output_linear), 77-100 (additive attention),
103-177 (NewsEncoder), 179-191 (UserEncoder), 196-257 (Model).

Same plugin contract as the other models (``model.nrms_naml_hip.Model(config)``, model/__init__.py:22-23); parameter names
and ``state_dict()`` order are the reference's, so checkpoints interchange with ``model.nrms_naml``.  The batch keys read
are the reference's (nrms_naml.py:217-228,245): ``browsed_titles / _absts / _categ_ids / _subcateg_ids``, the four
``candidate_*`` counterparts and ``candidate_mask`` -- all emitted by data_handler.MyDataset.
"""
import ctypes as C

import torch
import torch.nn as nn

from .. import _lib
from ..engine import FlatLayout, _stream
from ..naml_engine import NamlDims, NamlEngine, naml_entries
from . import nrms_hip

ID_KEYS = ("browsed_titles", "browsed_absts", "browsed_categ_ids", "browsed_subcateg_ids",
           "candidate_titles", "candidate_absts", "candidate_categ_ids", "candidate_subcateg_ids")


class _MultiHeadSelfAttentionParams(nn.Module):
    """nrms_naml.py:47-59: three Linear(d, d) in a ModuleList + output_linear, torch's default initialisation."""

    def __init__(self, h, d_model):
        super().__init__()
        assert d_model % h == 0
        self.h = h
        self.linear_layers = nn.ModuleList([nn.Linear(d_model, d_model) for _ in range(3)])
        self.output_linear = nn.Linear(d_model, d_model)


class _AdditiveAttentionParams(nn.Module):
    """nrms_naml.py:78-82."""

    def __init__(self, query_vector_dim, input_vector_dim):
        super().__init__()
        self.linear = nn.Linear(input_vector_dim, query_vector_dim)
        self.query_vector = nn.Parameter(torch.empty(query_vector_dim).uniform_(-0.1, 0.1))


class _NewsEncoderParams(nn.Module):
    """nrms_naml.py:104-119."""

    def __init__(self, config, table):
        super().__init__()
        self.category_embedding = nn.Embedding(config.category_nums, config.cate_embed_size, padding_idx=0)
        self.subcategory_embedding = nn.Embedding(config.subcategory_nums, config.cate_embed_size, padding_idx=0)
        self.word_embedding = nn.Embedding.from_pretrained(table, freeze=False, padding_idx=0)
        self.multi_head_self_attention = _MultiHeadSelfAttentionParams(config.title_heads_num, config.word_embed_size)
        self.additive_attention = _AdditiveAttentionParams(config.query_vector_dim, config.word_embed_size)


class _UserEncoderParams(nn.Module):
    """nrms_naml.py:181-186."""

    def __init__(self, config):
        super().__init__()
        self.multi_head_self_attention = _MultiHeadSelfAttentionParams(config.user_heads_num, config.news_feature_size)
        self.additive_attention = _AdditiveAttentionParams(config.query_vector_dim_large, config.news_feature_size)


class Model(nrms_hip.Model):
    def _build_modules(self, config, table):
        if int(config.news_feature_size) != 2 * int(config.word_embed_size) + 2 * int(config.cate_embed_size):
            raise ValueError("news_feature_size %d != 2 * word_embed_size + 2 * cate_embed_size (nrms_naml.py:174 concatenates "
                             "[title | abstract | category | sub-category])" % config.news_feature_size)
        self.news_encoder = _NewsEncoderParams(config, table)
        self.user_encoder = _UserEncoderParams(config)
        self.norm = nn.LayerNorm(config.news_feature_size)

    def _make_dims(self, config, V, d):
        return NamlDims(n_words=V, word_embed_size=d, title_heads_num=int(config.title_heads_num),
                        query_vector_dim=int(config.query_vector_dim), category_nums=int(config.category_nums),
                        subcategory_nums=int(config.subcategory_nums), cate_embed_size=int(config.cate_embed_size),
                        user_heads_num=int(config.user_heads_num), query_vector_dim_large=int(config.query_vector_dim_large))

    def _make_layout(self, dims):
        return FlatLayout(dims, naml_entries(dims))

    def _make_engine(self, device, precision):
        return NamlEngine(self._dims, device, precision=precision)

    def _engine_args(self, batch, dev):
        ids = {k: torch.as_tensor(batch[k]).to(dev, dtype=torch.int64, non_blocking=True) for k in ID_KEYS}
        mask = batch.get("candidate_mask") if hasattr(batch, "get") else batch["candidate_mask"]
        if mask is not None:
            mask = torch.as_tensor(mask).to(dev, dtype=torch.uint8, non_blocking=True)
        return ids, mask

    def _infer(self, batch, args, p_drop, seed):
        # evaluation: every distinct news item of the batch is encoded once (model.dedup_inference = False: every slot)
        self._engine.dedup_inference = bool(getattr(self, "dedup_inference", True))
        return self._engine.forward(self._flat, *args, training=False, p_drop=p_drop, seed=seed)

    def get_news_vector(self, *a, **k):
        raise _lib.NrmsError("nrms_naml has no get_news_vector / get_user_vector / get_prediction (nrms_naml.py:196-257)")

    get_user_vector = get_prediction = get_news_vector

    # ---- retrieval over the whole catalogue (recommend itself is nrms_hip.Model's, with the two hooks below) ------------
    @torch.no_grad()
    def encode_catalogue(self, titles, absts=None, categ=None, subcateg=None):
        """titles [N, Lt], absts [N, La] word ids (None: empty abstracts), categ / subcateg [N] category and sub-category ids,
        row r = news id r (``DeviceFeed.titles`` and ``DeviceFeed.news_info()``) -> news feature rows [N, F]
        (NewsEncoder.forward, nrms_naml.py:121-177, no dropout), in chunks of 32 768.  Ids outside their tables are read as
        padding and counted (engine.check_ids raises)."""
        if categ is None or subcateg is None:
            raise NotImplementedError("nrms_naml: catalogue retrieval needs the category and sub-category of every news item: "
                                      "encode_catalogue(titles, absts, categ, subcateg), e.g. with DeviceFeed.news_info()")
        dev = self._prepare()
        eng, d = self._engine, self._dims
        titles = torch.as_tensor(titles).to(dev, dtype=torch.int64)
        N = titles.shape[0]
        if absts is None:
            absts = torch.zeros(N, int(self.config.n_words_abst), dtype=torch.int64, device=dev)
        ids = []
        for src, vocab in ((titles, d.n_words), (absts, d.n_words), (categ, d.category_nums), (subcateg, d.subcategory_nums)):
            src = torch.as_tensor(src).to(dev, dtype=torch.int64).contiguous()
            if src.shape[0] != N:
                raise _lib.NrmsError("encode_catalogue: %d rows of ids for %d titles" % (src.shape[0], N))
            dst = torch.empty_like(src)
            _lib.check(eng.lib.nrms_sanitize_ids(_lib.ptr(src), _lib.ptr(dst), C.c_int64(src.numel()), int(vocab),
                                                 _lib.ptr(eng._bad_ids), _stream()), "nrms_sanitize_ids")
            ids.append(dst)
        eng.note_bad_ids()
        ids_t, ids_a, cat, sub = ids[0], ids[1], ids[2].view(N), ids[3].view(N)
        out = torch.empty(N, d.news_feature_size, dtype=torch.float32, device=dev)
        for c0 in range(0, N, 32768):
            c1 = min(N, c0 + 32768)
            eng.news_features(self._flat, ids_t[c0:c1], ids_a[c0:c1], cat[c0:c1], sub[c0:c1], 0.0, 0, "_cat", out=out[c0:c1])
        return out

    def recommend(self, batch, k, catalogue, exclude_history=True, *, diversity=None, shortlist=None, return_ild=False,
                  item_bias=None, item_time=None, window=None, coarse=None, coarse_shortlist=None, return_certified=False):
        """nrms_hip.Model.recommend over encode_catalogue's feature rows: the user vector is the LayerNorm of the history's
        catalogue rows through the user encoder (_forward_dedup's path), the score a plain dot product (click_scores); with
        ``diversity`` the cosine of the re-ranking is between feature rows.  ``item_bias`` is nrms_hip.Model.recommend's
        per-news prior, ``item_time`` / ``window`` its time window, ``coarse`` / ``coarse_shortlist`` / ``return_certified`` its
        fp16 shortlist path (pack_catalogue over the feature rows)."""
        if catalogue is None:
            raise NotImplementedError("nrms_naml: recommend needs a catalogue built with the per-news category tables: "
                                      "encode_catalogue(titles, absts, categ, subcateg)")
        return super().recommend(batch, k, catalogue, exclude_history, diversity=diversity, shortlist=shortlist,
                                 return_ild=return_ild, item_bias=item_bias, item_time=item_time, window=window, coarse=coarse,
                                 coarse_shortlist=coarse_shortlist, return_certified=return_certified)

    def recommend_page(self, batch, k, catalogue, after=None, exclude_history=True, *, item_bias=None, item_time=None, window=None):
        """nrms_hip.Model.recommend_page over encode_catalogue's feature rows (the user vector and the score are recommend's)."""
        if catalogue is None:
            raise NotImplementedError("nrms_naml: recommend_page needs a catalogue built with the per-news category tables: "
                                      "encode_catalogue(titles, absts, categ, subcateg)")
        return super().recommend_page(batch, k, catalogue, after, exclude_history, item_bias=item_bias, item_time=item_time,
                                      window=window)

    def recommend_deep(self, batch, K, catalogue, exclude_history=True, *, item_bias=None, item_time=None, window=None):
        """nrms_hip.Model.recommend_deep over encode_catalogue's feature rows (the user vector and the score are recommend's)."""
        if catalogue is None:
            raise NotImplementedError("nrms_naml: recommend_deep needs a catalogue built with the per-news category tables: "
                                      "encode_catalogue(titles, absts, categ, subcateg)")
        return super().recommend_deep(batch, K, catalogue, exclude_history, item_bias=item_bias, item_time=item_time, window=window)

    def _catalogue_width(self):
        return self._dims.news_feature_size

    def _catalogue_users(self, hist, browsed=None):
        B, H, F = hist.shape
        normed = self._engine.layernorm(self._flat, hist.reshape(B * H, F))
        return self._engine.encode_users(self._flat, normed.view(B, H, F), 0.0, 0, "user_eval")

    def _catalogue_user_parts(self, hist, browsed=None):
        B, H, F = hist.shape
        normed = self._engine.layernorm(self._flat, hist.reshape(B * H, F))
        return self._engine.user_parts(self._flat, normed.view(B, H, F))

    CATALOGUE_RETRIEVAL = False

