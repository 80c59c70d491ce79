"""NRMS on MI355X: drop-in for the reference's ``model.nrms_v0.Model``.

Same constructor (``Model(config)``), same ``forward(batch_dict) -> FloatTensor[B, C]`` of raw
logits with masked candidates at -1e9, same 19 parameter names (so ``state_dict`` files
interchange), same helper API (``get_news_vector`` / ``get_user_vector`` / ``get_prediction``)
as /root/reference/MIND_2020/model/nrms_v0.py:218-312 -- but every op runs in the
hand-written HIP kernels of libnrms_hip.so through the C ABI (include/nrms_hip.h).
There is no PyTorch/CPU fallback: without the library or a GPU, forward raises.

The module tree below only *names and initialises* parameters the way the reference does
(same construction order and initialisers, so ``torch.manual_seed(s)`` gives the same initial
weights); the nn.Linear / nn.Embedding forwards are never called.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..engine import (FlatLayout, ModelDims, NRMSEngine, PackedCatalogue, pack_tag_mask,  # noqa: F401 (pack_tag_mask and
                      remaining_caps)                                                     # remaining_caps: for callers)
from ._flat_model import FlatHipModel

PAGE_BEGIN = -2          # recommend_page: the cursor id of a row that starts over (include/nrms_hip.h NRMS_CURSOR_BEGIN)


class _MultiHeadSelfAttentionParams(nn.Module):
    """Parameter holder mirroring nrms_v0.py:26-44 (W_Q, W_K, W_V Linear(d,d), xavier-uniform weights)."""

    def __init__(self, d_model, num_attention_heads):
        super().__init__()
        assert d_model % num_attention_heads == 0
        self.d_model = d_model
        self.num_attention_heads = num_attention_heads
        self.W_Q = nn.Linear(d_model, d_model)
        self.W_K = nn.Linear(d_model, d_model)
        self.W_V = nn.Linear(d_model, d_model)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight, gain=1)


class _AdditiveAttentionParams(nn.Module):
    """Parameter holder mirroring nrms_v0.py:84-93."""

    def __init__(self, query_vector_dim, candidate_vector_dim):
        super().__init__()
        self.linear = nn.Linear(candidate_vector_dim, query_vector_dim)
        self.attention_query_vector = nn.Parameter(torch.empty(query_vector_dim).uniform_(-0.1, 0.1))


class _NewsEncoderParams(nn.Module):
    """nrms_v0.py:130-152: Sequential(Embedding.from_pretrained(freeze=False, padding_idx=0), Dropout)."""

    def __init__(self, config, table):
        super().__init__()
        self.word_embedding = nn.Sequential(
            nn.Embedding.from_pretrained(table, freeze=False, padding_idx=0),
            nn.Dropout(p=config.dropout, inplace=False))
        self.multihead_self_attention = _MultiHeadSelfAttentionParams(config.word_embed_size,
                                                                      config.num_attention_heads)
        self.additive_attention = _AdditiveAttentionParams(config.query_vector_dim, config.word_embed_size)


class _UserEncoderParams(nn.Module):
    """nrms_v0.py:179-186."""

    def __init__(self, config):
        super().__init__()
        self.multihead_self_attention = _MultiHeadSelfAttentionParams(config.word_embed_size,
                                                                      config.num_attention_heads)
        self.additive_attention = _AdditiveAttentionParams(config.query_vector_dim, config.word_embed_size)


def _load_table(config, pretrained_word_embedding):
    if pretrained_word_embedding is None:
        path = config.data_path + config.word_embedding_pretrained        # nrms_v0.py:134-135
        arr = np.load(path)["embeddings"].astype("float32")
        return torch.tensor(arr)
    return torch.as_tensor(np.asarray(pretrained_word_embedding, dtype=np.float32)).clone()


def _fma32(a, b, c):
    """The correctly rounded fp32 a * b + c of float32 tensors, on their device: the product is exact in float64, and the one
    case in which rounding the float64 sum to fp32 differs from rounding the exact value (the sum sits on a fp32 midpoint the
    exact value is not on) is decided by the sum's error term (TwoSum)."""
    a, b, c = torch.broadcast_tensors(a.double(), b.double(), c.double())
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = torch.isfinite(s) & torch.isfinite(err) & (err != 0) & ((s.contiguous().view(torch.int64) & 0x1FFFFFFF) == 0x10000000)
    toward = torch.where(err > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    return torch.where(tie, torch.nextafter(s, toward), s).float()


def _target_log_prob(ranks, scores, rows, lse, inv_t, scale, bias):
    """log_prob's last step: ranks, scores [B, T] of rank_of (no prior), rows [B, T] the targets' rows, lse [B, J] ->
    [B, T, J] fp32, fmaf(score, inv_t[j], scale[j] * bias[row]) - lse[b, j], NaN where the rank is 0."""
    dev = scores.device
    it = torch.tensor(inv_t, dtype=torch.float32, device=dev)
    if bias is None:
        c = torch.zeros((), dtype=torch.float32, device=dev)
    else:
        sc = torch.tensor([1.0] * len(inv_t) if scale is None else scale, dtype=torch.float32, device=dev)
        c = bias[rows.clamp(0, bias.shape[0] - 1)].unsqueeze(-1) * sc          # one fp32 multiply, as in the kernel
    z = _fma32(scores.unsqueeze(-1), it, c)
    out = z - lse.unsqueeze(1)
    return torch.where((ranks > 0).unsqueeze(-1), out, torch.full_like(out, float("nan")))


def _ids_on(dev, x):
    """Word ids on the device: int32 feeds stay int32 over PCIe (the library validates either width into its own
    int64 copy), anything else becomes the reference's int64."""
    t = torch.as_tensor(x)
    return t.to(dev, dtype=torch.int32 if t.dtype == torch.int32 else torch.int64, non_blocking=True)


class SectionedCatalogue:
    """A catalogue cut into sections for Model.recommend_sections (Model.section_catalogue builds it): row r = news id r.
    vectors [N, width]: the catalogue as given, in id order (the user vectors are built from it); items [N - 1, width]: rows 1..
    (the padding title is never a candidate) sorted stably by section, ids ascending inside a section; item_ids int32 [N - 1]:
    their news ids; section_ptr int64 [G + 1]; n_sections: G."""

    def __init__(self, vectors, section_of, n_sections):
        dev = vectors.device
        self.vectors, self.n_sections = vectors, int(n_sections)
        sec = section_of[1:]
        order = torch.sort(sec, stable=True).indices + 1
        self.items = vectors.index_select(0, order)
        self.item_ids = order.to(torch.int32)
        counts = torch.bincount(sec, minlength=self.n_sections)
        self.section_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0)])


class Model(FlatHipModel):
    """NRMS network: 1+K candidate titles and the clicked-title history -> click logits."""

    def __init__(self, config, pretrained_word_embedding=None):
        super().__init__()
        self.config = config
        table = _load_table(config, pretrained_word_embedding)
        V, d = table.shape
        if d != config.word_embed_size:
            raise ValueError("embedding width %d != config.word_embed_size %d" % (d, config.word_embed_size))
        self._build_modules(config, table)
        self._dims = self._make_dims(config, int(V), int(d))
        self._finish(self._make_layout(self._dims), table.device)

    # ---- topology hooks (overridden by model/nrms_v1_hip.py) ---------------------------------------
    def _build_modules(self, config, table):
        self.news_encoder = _NewsEncoderParams(config, table)
        self.user_encoder = _UserEncoderParams(config)

    def _make_dims(self, config, V, d):
        return ModelDims(n_words=V, word_embed_size=d, num_attention_heads=int(config.num_attention_heads),
                         query_vector_dim=int(config.query_vector_dim))

    def _make_layout(self, dims):
        return FlatLayout(dims)

    def _make_engine(self, device, precision):
        return NRMSEngine(self._dims, device, precision=precision, layout=self._layout)

    def _engine_args(self, batch, dev):
        """Only 'browsed_titles' [B,H,L], 'candidate_titles' [B,C,L] and 'candidate_mask' [B,C] are read
        (nrms_v0.py:248,250,272)."""
        bt, ct = _ids_on(dev, batch["browsed_titles"]), _ids_on(dev, batch["candidate_titles"])
        mask = batch.get("candidate_mask") if hasattr(batch, "get") else batch["candidate_mask"]
        if mask is not None:
            mask = torch.as_tensor(mask).to(dev, dtype=torch.uint8, non_blocking=True)
        return bt, ct, mask

    def _infer(self, batch, args, p_drop, seed):
        if p_drop == 0.0 and getattr(self, "dedup_inference", True):
            bt, ct, mask = args
            get = batch.get if hasattr(batch, "get") else (lambda k: None)
            bn, cn = get("browsed_ids"), get("candidate_ids")
            if self._engine._news_cache is not None and bn is not None and cn is not None:
                # inside train_eval.evaluate / test: news vectors are cached across batches by news id
                dev = self._flat.device
                return self._engine.forward_cached(self._flat, bt, ct, torch.as_tensor(bn).to(dev), torch.as_tensor(cn).to(dev), mask)
            scores, self.last_unique_titles = self._engine.forward_dedup(self._flat, bt, ct, mask)
            return scores
        return super()._infer(batch, args, p_drop, seed)

    # ---- reference API (beside forward) ---------------------------------------------------
    def get_news_vector(self, news):
        """news [N, L] title ids -> [N, d] (nrms_v0.py:278-289); inference only."""
        dev = self._prepare()
        ids = _ids_on(dev, news)
        p_drop = float(self.config.dropout) if self.training else 0.0
        p_embed = 0.0 if self._dims.style == "v1" else p_drop
        return self._engine.encode_titles(self._flat, ids, p_embed=p_embed, p_ctx=p_drop,
                                          seed=self._next_seed() if p_drop else 0)

    def get_user_vector(self, clicked_news_vector):
        """[B, H, d] -> [B, d] (nrms_v0.py:291-299); inference only."""
        dev = self._prepare()
        x = torch.as_tensor(clicked_news_vector).to(dev, dtype=torch.float32).contiguous()
        return self._engine.encode_users(self._flat, x)

    def get_prediction(self, news_vector, user_vector):
        """news_vector [C, d], user_vector [d] -> [C] (nrms_v0.py:301-312)."""
        dev = self._prepare()
        nv = torch.as_tensor(news_vector).to(dev, dtype=torch.float32).contiguous().unsqueeze(0)
        uv = torch.as_tensor(user_vector).to(dev, dtype=torch.float32).contiguous().unsqueeze(0)
        return self._engine.click_scores(nv, uv).squeeze(0)

    # ---- retrieval over the whole catalogue ----------------------------------------------------
    @torch.no_grad()
    def encode_catalogue(self, titles):
        """titles [N, L] word ids, row r = news id r (e.g. ``DeviceFeed.titles``, row 0 = the padding title) -> news
        vectors [N, d]: the evaluation-precision, dropout-free vectors forward_cached keeps per news id, whatever the
        module's train / eval mode.  encode_titles works through the table in chunks of 32 768 titles."""
        dev = self._prepare()
        return self._engine.encode_titles(self._flat, _ids_on(dev, titles), tag="news_eval")

    @torch.no_grad()
    def pack_catalogue(self, catalogue):
        """catalogue: encode_catalogue's [N, width] (contiguous) -> a PackedCatalogue for recommend(coarse=...): the fp16 copy of
        rows 1.., as recommend reads them ((N - 1) * 32 ceil(width / 32) * 2 bytes), and its norm bounds (include/nrms_hip.h
        nrms_catalogue_pack_f16).  It belongs to this very tensor: pack again after every encode_catalogue."""
        dev = self._prepare()
        cat = torch.as_tensor(catalogue)
        d = self._catalogue_width()
        if cat.dim() != 2 or cat.shape[1] != d or cat.dtype != torch.float32 or cat.device != dev or cat.shape[0] < 1 or not cat.is_contiguous():
            raise _lib.NrmsError("pack_catalogue: catalogue must be a contiguous [N >= 1, %d] float32 tensor on %s (encode_catalogue), got %s %s on %s"
                                 % (d, dev, tuple(cat.shape), cat.dtype, cat.device))
        packed = self._engine.pack_catalogue(cat[1:])
        packed.source = (cat.data_ptr(), tuple(cat.shape))
        return packed

    @staticmethod
    def _coarse_args(who, k, coarse, coarse_shortlist, return_certified, diversity, shortlist, return_ild, item_bias, item_time, window):
        """recommend's checks of the coarse path that need no device -> the shortlist length M (None without ``coarse``)."""
        if coarse is None:
            if coarse_shortlist is not None or return_certified:
                raise _lib.NrmsError("%s: coarse_shortlist / return_certified belong to the fp16 shortlist path (give coarse=pack_catalogue(catalogue))" % who)
            return None
        if diversity is not None or shortlist is not None or return_ild:
            raise _lib.NrmsError("%s: coarse takes no diversity / shortlist / return_ild: the certificate covers the plain top-k only" % who)
        if item_bias is not None:
            raise _lib.NrmsError("%s: coarse takes no item_bias: the certificate covers the plain dot product only" % who)
        if item_time is not None or window is not None:
            raise _lib.NrmsError("%s: coarse takes no item_time / window: the certificate covers the whole catalogue only" % who)
        if not isinstance(coarse, PackedCatalogue):
            raise _lib.NrmsError("%s: coarse must be a PackedCatalogue (pack_catalogue(catalogue)), got %s" % (who, type(coarse).__name__))
        k = int(k)
        M = min(256, max(64, 4 * k)) if coarse_shortlist is None else int(coarse_shortlist)
        if not 1 <= k <= M <= 256:
            raise _lib.NrmsError("%s: with coarse, 1 <= k <= coarse_shortlist <= 256 (k=%d, coarse_shortlist=%d)" % (who, k, M))
        return M

    def _recommend_coarse(self, user, cat, exclude, k, M, packed, return_certified):
        """The plain list through the fp16 shortlist: certified rows are top_k's bit for bit, the others are run through top_k."""
        if packed.source != (cat.data_ptr(), tuple(cat.shape)):
            raise _lib.NrmsError("recommend: coarse was packed from another catalogue tensor (packed %s at 0x%x, catalogue %s at 0x%x): "
                                 "pack_catalogue again after every encode_catalogue"
                                 % (packed.source[1], packed.source[0], tuple(cat.shape), cat.data_ptr()))
        scores, ids, cert = self._engine.top_k_coarse(user, packed, k, M, exclude)
        rows = (cert == 0).nonzero().view(-1)          # the one host synchronisation of the coarse path
        if rows.numel():
            f_scores, f_ids = self._engine.top_k(user.index_select(0, rows), packed.items, k,
                                                 None if exclude is None else exclude.index_select(0, rows))
            scores.index_copy_(0, rows, f_scores)
            ids.index_copy_(0, rows, f_ids)
        out = (torch.where(ids >= 0, ids + 1, ids), scores)
        return out + (cert,) if return_certified else out

    @torch.no_grad()
    def recommend(self, batch, k, catalogue, exclude_history=True, *, diversity=None, shortlist=None, return_ild=False,
                  item_bias=None, item_time=None, window=None, coarse=None, coarse_shortlist=None, return_certified=False):
        """The k news ids of the whole catalogue each user of ``batch`` should see -> (news_ids [B, k] int64, scores
        [B, k] fp32), best first (score descending, then the smaller id; include/nrms_hip.h nrms_topk_dot).

        catalogue: encode_catalogue(titles) [N, d].  Only ``browsed_ids`` [B, H] (news ids, 0 = padding slot) is read:
        the user vector is encode_users over catalogue rows browsed_ids, the vectors forward_cached scores with (ids
        outside the catalogue are read as padding and counted: check_recommend_ids raises on them).  News
        id 0, the padding title, is never returned; with exclude_history neither is a browsed id.  A user with fewer
        than k eligible news gets id -1 / score -inf in the remaining slots.

        diversity = lambda in [0, 1]: the list is re-ranked for diversity instead (include/nrms_hip.h nrms_mmr_rerank): the
        ``shortlist`` best news (default min(256, 4 k); k <= shortlist <= 256) are retrieved as above and k of them are
        picked greedily by maximal marginal relevance, lambda * (score scaled to [0, 1] over the shortlist) - (1 - lambda) *
        (largest cosine between catalogue rows to the news picked so far), in pick order; the scores returned are still the
        dot products.  lambda = 1 is the plain list, bit for bit.  return_ild appends the intra-list diversity [B] fp32 of the
        returned list (1 - mean pairwise cosine of its catalogue rows, NaN with fewer than two news), from the same kernel
        with or without ``diversity``.

        item_bias: float32 [N] on the model's device, indexed by news id like the catalogue (row 0, the padding title's, is
        never read), or None.  A per-news prior: the list is ordered by, and the scores returned are, dot product +
        item_bias[id] (one fp32 add; include/nrms_hip.h nrms_topk_dot_biased), e.g. ``ClickFeed.popularity_prior``, a
        freshness decay or an editorial boost.  A NaN entry removes that news for every user (a global block-list); -inf
        puts it last.  With ``diversity`` the shortlist comes from the biased top-k and the re-ranker scales the biased
        scores to relevance; diversity = 1 with a bias is the biased plain list, bit for bit.  None is the call as it was.

        item_time: int [N] on the model's device, one tick per news id like the catalogue (entry 0 is never read); window:
        int [B, 2].  Both or neither.  User b only gets news with window[b, 0] <= item_time[id] < window[b, 1] (signed int32,
        half-open; lo >= hi gives an all-padding row; a time of INT32_MAX, "not published", is never eligible;
        include/nrms_hip.h nrms_topk_dot_windowed), e.g. ``ClickFeed.news_first_seen()`` and a request time per user.  With
        ``diversity`` the shortlist comes from the windowed top-k and the re-ranker is untouched.  None is the call as it was.

        coarse: pack_catalogue(catalogue), or None (the call as it was).  The same ids and score bits, always, for less than
        the exact scan where the certificate holds: an fp16 pass picks ``coarse_shortlist`` news per user (default
        min(256, max(64, 4 k)); k <= coarse_shortlist <= 256), the exact chain re-scores them, and a per-user certificate proves
        that nothing outside the shortlist can reach the top k (include/nrms_hip.h nrms_topk_dot_coarse).  The rows it cannot
        certify are gathered and run through the exact call (one ``nonzero``: the one host synchronisation, with ``coarse``
        only).  return_certified appends the mask [B] uint8 as it stood before that fallback.  A pack made from another
        catalogue tensor raises NrmsError.  Out of scope here: with ``diversity``, ``item_bias`` or ``item_time`` / ``window``,
        ``coarse`` raises NrmsError."""
        M_coarse = self._coarse_args("recommend", k, coarse, coarse_shortlist, return_certified, diversity, shortlist, return_ild,
                                     item_bias, item_time, window)
        if M_coarse is not None:
            user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, "recommend")
            return self._recommend_coarse(user, cat, exclude, int(k), M_coarse, coarse, return_certified)
        if diversity is None and shortlist is not None:
            raise _lib.NrmsError("recommend: shortlist is the candidate count of the diversity re-ranking (give diversity)")
        if diversity is not None:
            k, lam = int(k), float(diversity)
            if not 0.0 <= lam <= 1.0:
                raise _lib.NrmsError("recommend: diversity must be in [0, 1] (got %r)" % (diversity,))
            M = min(256, 4 * k) if shortlist is None else int(shortlist)
            if not 1 <= k <= M <= 256:
                raise _lib.NrmsError("recommend: with diversity, 1 <= k <= shortlist <= 256 (k=%d, shortlist=%d)" % (k, M))
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, "recommend")
        bias = self._item_bias_rows(item_bias, cat, "recommend")
        win = self._time_window_rows(item_time, window, cat, user.shape[0], "recommend")
        if diversity is None:
            scores, ids = self._engine.top_k(user, cat[1:], k, exclude, bias=bias, **win)
            out = (torch.where(ids >= 0, ids + 1, ids), scores)
            if return_ild:      # the plain list's ILD is the re-ranker's at lambda = 1, which keeps the list as it is
                out += (self._engine.mmr_rerank(cat[1:], ids, scores, ids.shape[1], 1.0, return_ild=True)[2],)
            return out
        s_scores, s_ids = self._engine.top_k(user, cat[1:], M, exclude, bias=bias, **win)
        res = self._engine.mmr_rerank(cat[1:], s_ids, s_scores, k, lam, return_ild=return_ild)
        return (torch.where(res[0] >= 0, res[0] + 1, res[0]), res[1]) + tuple(res[2:])

    @torch.no_grad()
    def recommend_page(self, batch, k, catalogue, after=None, exclude_history=True, *, item_bias=None, item_time=None, window=None):
        """One page of recommend's ranking -> (news_ids [B, k] int64, scores [B, k] fp32): per user the k news that follow the
        position ``after`` in recommend's list were it unbounded (the same user vector, score bits, exclusions and tie rule;
        include/nrms_hip.h nrms_topk_dot_after).  1 <= k <= 256.

        after: None, the first page (recommend(k), bit for bit), or (ids [B], scores [B]): the LAST COLUMN of the page before,
        in news ids, as this method returned it.  No state is kept between pages: a feed that scrolls sends back the last news it
        showed.  Id -1 (what a page leaves in the slots its list did not reach) means exhausted: the row is all padding, id -1 /
        score -inf, and stays so.  ``PAGE_BEGIN`` as an id marks a row that starts over (its score is not read), so users on
        different pages share a batch.  Any id >= 1 is a position, not an item: it need not be recommendable.  Id 0, the padding
        title, is read as -1.

        catalogue, ``browsed_ids``, exclude_history, item_bias, item_time and window are recommend's, and have to be the same
        from page to page for the pages to chain."""
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, "recommend_page")
        bias = self._item_bias_rows(item_bias, cat, "recommend_page")
        win = self._time_window_rows(item_time, window, cat, user.shape[0], "recommend_page")
        B, dev = user.shape[0], user.device
        if after is None:
            a_ids = torch.full((B,), PAGE_BEGIN, dtype=torch.int64, device=dev)
            a_scores = torch.zeros(B, dtype=torch.float32, device=dev)
        else:
            cur = self._after_rows(after, B, dev, "recommend_page")
            a_scores, a_ids = cur["after_scores"], cur["after_ids"]
        scores, ids = self._engine.top_k_after(user, cat[1:], k, a_scores, a_ids, exclude, bias=bias, **win)
        return torch.where(ids >= 0, ids + 1, ids), scores

    @torch.no_grad()
    def recommend_deep(self, batch, K, catalogue, exclude_history=True, *, item_bias=None, item_time=None, window=None):
        """recommend at a depth of up to 4096 (candidates for a re-ranker) -> (news_ids [B, K] int64, scores [B, K] fp32): the
        first K news of recommend's ranking, then id -1 / score -inf; ceil(K / 256) pages chained on the device without a host
        synchronisation (include/nrms_hip.h nrms_topk_dot_deep).  K <= 256 is recommend(K), bit for bit; rank_targets of row b's
        ids gives 1, 2, ...  The arguments are recommend's (no diversity re-ranking and no fp16 shortlist at this depth)."""
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, "recommend_deep")
        bias = self._item_bias_rows(item_bias, cat, "recommend_deep")
        win = self._time_window_rows(item_time, window, cat, user.shape[0], "recommend_deep")
        scores, ids = self._engine.top_k_deep(user, cat[1:], K, exclude, bias=bias, **win)
        return torch.where(ids >= 0, ids + 1, ids), scores

    @staticmethod
    @torch.no_grad()
    def section_catalogue(catalogue, section_of, n_sections):
        """catalogue: encode_catalogue's [N, width]; section_of int64 [N]: the section of every news id (e.g.
        ``DeviceFeed.news_info()["categ"]``; section 0, "unknown", is an ordinary section; entry 0, the padding title's, is not
        read); n_sections: G -> a SectionedCatalogue for recommend_sections, on the catalogue's device (torch ops only).  A
        value outside [0, n_sections) raises NrmsError here (one host synchronisation)."""
        cat = torch.as_tensor(catalogue)
        G = int(n_sections)
        sec = torch.as_tensor(section_of).to(cat.device, dtype=torch.int64).reshape(-1)
        if cat.dim() != 2 or cat.dtype != torch.float32 or sec.shape[0] != cat.shape[0] or cat.shape[0] < 1:
            raise _lib.NrmsError("section_catalogue: catalogue must be [N >= 1, width] float32 and section_of [N] (got %s %s, %s)"
                                 % (tuple(cat.shape), cat.dtype, tuple(sec.shape)))
        if G < 1:
            raise _lib.NrmsError("section_catalogue: n_sections must be >= 1 (got %d)" % G)
        n_bad = int(((sec[1:] < 0) | (sec[1:] >= G)).sum().item())
        if n_bad:
            raise _lib.NrmsError("section_catalogue: %d section ids outside [0, %d)" % (n_bad, G))
        return SectionedCatalogue(cat.contiguous(), sec, G)

    @torch.no_grad()
    def recommend_sections(self, batch, k, sectioned, exclude_history=True, *, item_bias=None):
        """The front page by section: for each user of ``batch`` the k best news of EVERY section -> (news_ids [B, G, k]
        int64, scores [B, G, k] fp32), row (b, g) best first (score descending, then the smaller id), in one call over the
        catalogue (include/nrms_hip.h nrms_topk_sections_dot).  Row (b, g) is recommend's full ranking for user b filtered
        to section g and cut at k, ids and score bits.

        sectioned: section_catalogue(...).  The user vector, ``browsed_ids``, the counting of ids outside the catalogue
        (check_recommend_ids), the id-0 rule, ``exclude_history`` and ``item_bias`` (float32 [N] by news id, NaN = a global
        block-list) are recommend's.  A section with fewer than k eligible news ends in id -1 / score -inf; an empty one is
        all padding."""
        if not isinstance(sectioned, SectionedCatalogue):
            raise _lib.NrmsError("recommend_sections: needs a SectionedCatalogue (section_catalogue(catalogue, section_of, n_sections))")
        user, cat, exclude = self._catalogue_query(batch, sectioned.vectors, exclude_history, "recommend_sections")
        bias = self._item_bias_rows(item_bias, cat, "recommend_sections")
        if bias is not None:          # by news id -> by row of the sectioned layout
            bias = item_bias.index_select(0, sectioned.item_ids)
        if exclude is not None:       # the kernel's ids are news ids here, not rows of cat[1:]; the padding slots become id 0, no item's
            exclude = exclude + 1
        scores, ids = self._engine.top_k_sections(user, sectioned.items, sectioned.item_ids, sectioned.section_ptr, k, exclude, bias=bias)
        return ids, scores

    @torch.no_grad()
    def rank_targets(self, batch, targets, catalogue, exclude_history=True, *, item_bias=None, item_time=None, window=None):
        """The exact position of given news in each user's ranking of the whole catalogue -> (ranks [B, T] int32, scores
        [B, T] fp32): ranks[b, j] is the 1-based place news id targets[b, j] would take in recommend()'s list for user b
        were k unbounded (the same user vector, score bits, exclusions and tie rule; include/nrms_hip.h nrms_rank_dot), so
        the ids recommend(k) returns rank 1 .. k.

        targets [B, T] news ids, any T, -1 = padding.  A target that cannot be recommended comes back as rank 0 / score
        -inf: id 0 (the padding title), an id outside the catalogue, a NaN score and, with exclude_history, a browsed id.
        catalogue and ``browsed_ids`` as in recommend (ids outside the catalogue are read as padding and counted:
        check_recommend_ids raises on them).

        item_bias: recommend's per-news prior (float32 [N] by news id, or None).  Ranks and scores are then those of dot
        product + item_bias[id] (include/nrms_hip.h nrms_rank_dot_biased), so with the same ``item_bias`` the ids
        recommend(k) returns still rank 1 .. k; a target whose prior is NaN is rank 0 / score -inf.

        item_time, window: recommend's time window (int [N] by news id, int [B, 2]; both or neither).  Ranks then count the
        news inside user b's window only (include/nrms_hip.h nrms_rank_dot_windowed), so with the same arguments the ids
        recommend(k) returns still rank 1 .. k; a target outside its user's window is rank 0 / score -inf."""
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, "rank_targets")
        bias = self._item_bias_rows(item_bias, cat, "rank_targets")
        win = self._time_window_rows(item_time, window, cat, user.shape[0], "rank_targets")
        tg = torch.as_tensor(targets).to(user.device, dtype=torch.int64)
        if tg.dim() != 2 or tg.shape[0] != user.shape[0]:
            raise _lib.NrmsError("rank_targets: targets must be [%d, T] news ids (got %s)" % (user.shape[0], tuple(tg.shape)))
        # rows 1.. as in recommend: news id n is row n - 1, so id 0 (and -1) fall out of range and get rank 0
        return self._engine.rank_of(user, cat[1:], (tg - 1).contiguous(), exclude, bias=bias, **win)

    @staticmethod
    def _tag_rows(item_tag, allow, cat, B, who):
        """The kernels' view of a per-user tag set -> (item_tag rows 1.. like the catalogue's, n_tags, allow) for
        engine.top_k_tagged / rank_of_tagged (which check dtypes and pack a bool ``allow``).  n_tags is read off a bool ``allow``;
        a packed int32 [B, W] one stands for n_tags = 32 W."""
        rows = Model._item_tag_rows(item_tag, cat, who)
        if (not torch.is_tensor(allow) or allow.dim() != 2 or allow.shape[0] != B or allow.shape[1] < 1
                or allow.dtype not in (torch.bool, torch.int32) or allow.device != cat.device):
            got = ("%s %s on %s" % (tuple(allow.shape), allow.dtype, allow.device)) if torch.is_tensor(allow) else type(allow).__name__
            raise _lib.NrmsError("%s: allow must be a bool [%d, n_tags] tensor, or pack_tag_mask's int32 [%d, W], on %s (got %s)"
                                 % (who, B, B, cat.device, got))
        n_tags = allow.shape[1] * (1 if allow.dtype == torch.bool else 32)
        return rows, n_tags, allow

    @staticmethod
    def _item_tag_rows(item_tag, cat, who):
        """The checked item_tag of recommend_tagged / recommend_capped -> its rows 1.. like the catalogue's."""
        N = cat.shape[0]
        if (not torch.is_tensor(item_tag) or tuple(item_tag.shape) != (N,) or item_tag.dtype not in (torch.int32, torch.int64)
                or item_tag.device != cat.device):
            got = ("%s %s on %s" % (tuple(item_tag.shape), item_tag.dtype, item_tag.device)) if torch.is_tensor(item_tag) \
                else type(item_tag).__name__
            raise _lib.NrmsError("%s: item_tag must be an int32 or int64 [%d] tensor on %s, indexed by news id like the catalogue "
                                 "(got %s)" % (who, N, cat.device, got))
        return item_tag.contiguous()[1:]

    @torch.no_grad()
    def recommend_tagged(self, batch, k, catalogue, item_tag, allow, exclude_history=True, *, item_bias=None):
        """recommend inside a per-user set of news tags -> (news_ids [B, k] int64, scores [B, k] fp32): "never show me sports",
        "only the topics I follow", an edition, a publisher block (include/nrms_hip.h nrms_topk_dot_tagged).  Parity is unpinned:
        the reference has no catalogue retrieval.

        item_tag: int [N] on the model's device, one tag per news id like the catalogue (entry 0 is never read), e.g.
        ``DeviceFeed.news_info()["categ"]``; a tag outside [0, n_tags), e.g. -1, is served to nobody.  allow: bool [B, n_tags]
        (user b may see tag t iff allow[b, t]), or its packed form pack_tag_mask(allow), int32 [B, W]; n_tags <= 512.  An
        all-False row gives an all-padding row.  Row b is recommend's full ranking for user b filtered to the tags b allows and
        cut at k: the same user vector, score bits, exclusions, tie rule and ``item_bias``; rank_targets_tagged of its ids gives
        1, 2, ...  Not combined with a time window, the diversity re-ranking, paging or the fp16 shortlist."""
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, "recommend_tagged")
        bias = self._item_bias_rows(item_bias, cat, "recommend_tagged")
        tags, n_tags, allow = self._tag_rows(item_tag, allow, cat, user.shape[0], "recommend_tagged")
        scores, ids = self._engine.top_k_tagged(user, cat[1:], k, tags, n_tags, allow, exclude, bias=bias)
        return torch.where(ids >= 0, ids + 1, ids), scores

    @staticmethod
    def _cap_rows(cap, n_tags, B, k, dev, who):
        """The kernels' view of the caps -> (cap int32 [B, n_tags] on dev, n_tags).  cap: an int (the same cap for every tag and
        user; n_tags is then the keyword), an int tensor [n_tags] (the same caps for every user) or [B, n_tags].  Expanded on the
        device; values are clamped to [0, 2^31 - 1] (a cap <= 0 closes the tag, one >= k leaves it uncapped)."""
        if isinstance(cap, bool) or not (isinstance(cap, int) or torch.is_tensor(cap)):
            raise _lib.NrmsError("%s: cap must be an int, or an int tensor [n_tags] or [%d, n_tags] (got %s)" % (who, B, type(cap).__name__))
        if isinstance(cap, int):
            if n_tags is None:
                raise _lib.NrmsError("%s: an int cap needs n_tags= (the number of tags item_tag runs over)" % who)
            n_tags = int(n_tags)
            if not 1 <= n_tags <= 512:
                raise _lib.NrmsError("%s: n_tags must be in [1, 512] (n_tags=%d)" % (who, n_tags))
            return torch.full((B, n_tags), min(max(cap, 0), 2 ** 31 - 1), dtype=torch.int32, device=dev), n_tags
        if (cap.dtype not in (torch.int32, torch.int64) or cap.dim() not in (1, 2) or cap.shape[-1] < 1
                or (cap.dim() == 2 and cap.shape[0] != B) or cap.device != dev):
            raise _lib.NrmsError("%s: cap must be an int32 or int64 tensor [n_tags] or [%d, n_tags] on %s (got %s %s on %s)"
                                 % (who, B, dev, tuple(cap.shape), cap.dtype, cap.device))
        if n_tags is not None and int(n_tags) != cap.shape[-1]:
            raise _lib.NrmsError("%s: n_tags=%d does not match cap %s" % (who, int(n_tags), tuple(cap.shape)))
        cap = cap.clamp(0, 2 ** 31 - 1).to(torch.int32)
        if cap.dim() == 1:
            cap = cap.unsqueeze(0).expand(B, -1)
        return cap.contiguous(), cap.shape[1]

    @torch.no_grad()
    def recommend_capped(self, batch, k, catalogue, item_tag, cap, exclude_history=True, *, item_bias=None, n_tags=None):
        """recommend with a hard cap per news tag -> (news_ids [B, k] int64, scores [B, k] fp32): "at most two stories per category
        in my ten", "one politics story at most for this user" (include/nrms_hip.h nrms_topk_dot_capped).  Parity is unpinned: the
        reference has no catalogue retrieval.

        item_tag: int [N] on the model's device, one tag per news id like the catalogue (entry 0 is never read), exactly
        recommend_tagged's; a tag outside [0, n_tags), e.g. -1, is served to nobody.  cap: an int (every tag, every user; give
        ``n_tags=``), an int tensor [n_tags] (every user) or [B, n_tags]; cap <= 0 closes the tag for that user, cap >= k leaves it
        uncapped.  Row b is recommend's full ranking for user b (the same user vector, score bits, exclusions, tie rule and
        ``item_bias``) walked greedily: a news is taken iff its tag has room left; the first k taken are the row, then id -1 / score
        -inf.  With every cap >= k and every tag in range this is recommend, bit for bit.  Not combined with a time window, paging,
        the fp16 shortlist, sections, the diversity re-ranking or the log-partition."""
        who = "recommend_capped"
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, who)
        bias = self._item_bias_rows(item_bias, cat, who)
        B = user.shape[0]
        caps, n_tags = self._cap_rows(cap, n_tags, B, int(k), cat.device, who)
        tags = self._item_tag_rows(item_tag, cat, who)
        scores, ids = self._engine.top_k_capped(user, cat[1:], k, tags, n_tags, caps, exclude, bias=bias)
        return torch.where(ids >= 0, ids + 1, ids), scores

    @torch.no_grad()
    def rank_targets_tagged(self, batch, targets, catalogue, item_tag, allow, exclude_history=True, *, item_bias=None):
        """rank_targets among the news each user may see -> (ranks [B, T] int32, scores [B, T] fp32): the 1-based place of news id
        targets[b, j] in recommend_tagged's list for user b were k unbounded (include/nrms_hip.h nrms_rank_dot_tagged).  A target
        whose tag user b does not allow comes back as rank 0 / score -inf, like every target rank_targets cannot rank.  item_tag
        and allow are recommend_tagged's, every other argument is rank_targets'."""
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, "rank_targets_tagged")
        bias = self._item_bias_rows(item_bias, cat, "rank_targets_tagged")
        tags, n_tags, allow = self._tag_rows(item_tag, allow, cat, user.shape[0], "rank_targets_tagged")
        tg = torch.as_tensor(targets).to(user.device, dtype=torch.int64)
        if tg.dim() != 2 or tg.shape[0] != user.shape[0]:
            raise _lib.NrmsError("rank_targets_tagged: targets must be [%d, T] news ids (got %s)" % (user.shape[0], tuple(tg.shape)))
        return self._engine.rank_of_tagged(user, cat[1:], (tg - 1).contiguous(), tags, n_tags, allow, exclude, bias=bias)

    @staticmethod
    def _adjust_rows(adjust, cat, B, who):
        """The kernels' view of per-user adjustments -> (adj_ids int64 [B, E] of catalogue rows, adj_delta fp32 [B, E]) for
        engine.top_k_adjusted / rank_of_adjusted.  ``adjust`` = (news_ids [B, E], delta [B, E]) in _catalogue_query's convention:
        news id n is row n - 1, so id 0 (and anything beyond the catalogue) becomes an empty slot."""
        if not isinstance(adjust, (tuple, list)) or len(adjust) != 2:
            raise _lib.NrmsError("%s: adjust must be a pair (news_ids [%d, E], delta [%d, E]) (got %s)"
                                 % (who, B, B, type(adjust).__name__))
        ids = torch.as_tensor(adjust[0]).to(cat.device, dtype=torch.int64)
        delta = torch.as_tensor(adjust[1]).to(cat.device, dtype=torch.float32)
        if ids.dim() != 2 or ids.shape[0] != B or delta.shape != ids.shape:
            raise _lib.NrmsError("%s: adjust must be (news_ids [%d, E], delta [%d, E]) of one shape (got %s and %s)"
                                 % (who, B, B, tuple(ids.shape), tuple(delta.shape)))
        if ids.shape[1] > 256:
            raise _lib.NrmsError("%s: adjust holds %d slots per user, at most 256 fit (NRMS_ADJ_MAX)" % (who, ids.shape[1]))
        return (ids - 1).contiguous(), delta.contiguous()

    @torch.no_grad()
    def recommend_adjusted(self, batch, k, catalogue, adjust, exclude_history=True, *, item_bias=None):
        """recommend with per-user score adjustments -> (news_ids [B, k] int64, scores [B, k] fp32): a story already shown to this
        user three times without a click goes down by 3 beta (data_handler.seen_adjustment builds that), a followed publisher's
        goes up, a NaN delta blocks a story for one user (include/nrms_hip.h nrms_topk_dot_adjusted).  Parity is unpinned: the
        reference has no catalogue retrieval.

        adjust = (news_ids [B, E], delta [B, E]), E <= 256, news ids as in the catalogue: id 0 and ids beyond the catalogue are
        empty slots; of several slots of a row that name one news the first counts.  Row b is recommend's ranking for user b (the
        same user vector, score bits, exclusions, tie rule and ``item_bias``) with delta added, one fp32 add, to the scores of the
        named news; the returned scores are the adjusted ones, and rank_targets_adjusted of the ids gives 1, 2, ...  With every
        slot empty this is recommend, bit for bit.  Not combined with a time window, tags, caps, paging, sections, the diversity
        re-ranking, the log-partition or the fp16 shortlist (whose certificate bounds raw scores; a boost breaks it)."""
        who = "recommend_adjusted"
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, who)
        bias = self._item_bias_rows(item_bias, cat, who)
        adj_ids, adj_delta = self._adjust_rows(adjust, cat, user.shape[0], who)
        scores, ids = self._engine.top_k_adjusted(user, cat[1:], k, adj_ids, adj_delta, exclude, bias=bias)
        return torch.where(ids >= 0, ids + 1, ids), scores

    @torch.no_grad()
    def rank_targets_adjusted(self, batch, targets, catalogue, adjust, exclude_history=True, *, item_bias=None):
        """rank_targets under per-user score adjustments -> (ranks [B, T] int32, scores [B, T] fp32): the 1-based place of news id
        targets[b, j] in recommend_adjusted's list for user b were k unbounded, and its adjusted score (include/nrms_hip.h
        nrms_rank_dot_adjusted).  A target whose delta is NaN comes back as rank 0 / score -inf, like every target rank_targets
        cannot rank.  adjust is recommend_adjusted's, every other argument is rank_targets'."""
        who = "rank_targets_adjusted"
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, who)
        bias = self._item_bias_rows(item_bias, cat, who)
        adj_ids, adj_delta = self._adjust_rows(adjust, cat, user.shape[0], who)
        tg = torch.as_tensor(targets).to(user.device, dtype=torch.int64)
        if tg.dim() != 2 or tg.shape[0] != user.shape[0]:
            raise _lib.NrmsError("%s: targets must be [%d, T] news ids (got %s)" % (who, user.shape[0], tuple(tg.shape)))
        return self._engine.rank_of_adjusted(user, cat[1:], (tg - 1).contiguous(), adj_ids, adj_delta, exclude, bias=bias)

    def _request_rows(self, cat, B, item_time, window, item_tag, allow, adjust, who):
        """The kernels' view of a request's parts -> the keywords of engine.top_k_request / rank_of_request (absent parts are left
        out).  Each part is checked by its own helper, in its own words."""
        kw = dict(self._time_window_rows(item_time, window, cat, B, who))
        if (item_tag is None) != (allow is None):
            raise _lib.NrmsError("%s: item_tag and allow go together (item_tag %s, allow %s)"
                                 % (who, "missing" if item_tag is None else "given", "missing" if allow is None else "given"))
        if item_tag is not None:
            tags, n_tags, allow = self._tag_rows(item_tag, allow, cat, B, who)
            kw.update(item_tag=tags, n_tags=n_tags, allow=allow)
        if adjust is not None:
            adj_ids, adj_delta = self._adjust_rows(adjust, cat, B, who)
            kw.update(adj_ids=adj_ids, adj_delta=adj_delta)
        return kw

    @torch.no_grad()
    def recommend_request(self, batch, k, catalogue, exclude_history=True, *, item_bias=None, item_time=None, window=None,
                          item_tag=None, allow=None, adjust=None, after=None):
        """One front-page request through several catalogue filters at once -> (news_ids [B, k] int64, scores [B, k] fp32): news
        that is still live (item_time, window: recommend's), outside the topics this user muted (item_tag, allow:
        recommend_tagged's), with what they were already shown pushed down (adjust: recommend_adjusted's), after the page they
        have just seen (after: recommend_page's (ids [B], scores [B]), None = the first page).  Every part is optional and keeps
        the rules of its own method; include/nrms_hip.h nrms_topk_dot_request states how they compose: the score is (dot product +
        item_bias) + delta, a news is served iff every part leaves it open, and the cursor compares the adjusted score, so the
        same ``adjust`` goes with every page.  rank_targets_request of the ids gives 1, 2, ...  With no part or one part this is
        that part's own method, bit for bit.  Caps go with every part in recommend_request_capped.  Not combined with the fp16
        shortlist, sections, the diversity re-ranking, the log-partition, explain or recommend_deep."""
        who = "recommend_request"
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, who)
        bias = self._item_bias_rows(item_bias, cat, who)
        B, dev = user.shape[0], user.device
        kw = self._request_rows(cat, B, item_time, window, item_tag, allow, adjust, who)
        if after is not None:
            kw.update(self._after_rows(after, B, dev, who))
        scores, ids = self._engine.top_k_request(user, cat[1:], k, exclude, bias=bias, **kw)
        return torch.where(ids >= 0, ids + 1, ids), scores

    @staticmethod
    def _after_rows(after, B, dev, who):
        """The cursor (ids [B], scores [B]) of recommend_page, recommend_request and recommend_request_capped -> the after_scores /
        after_ids keywords of the engine.  News id n is row n - 1 of cat[1:], as in recommend; -1, PAGE_BEGIN and every other
        negative id pass through unshifted.  Id 0, the padding title, is no row and no page returns it: it is read as -1, exhausted."""
        try:
            a_ids, a_scores = after
        except (TypeError, ValueError):
            raise _lib.NrmsError("%s: after must be None or (ids [B], scores [B]), the last column of the page before" % who)
        a_ids = torch.as_tensor(a_ids).to(dev, dtype=torch.int64).reshape(-1)
        a_scores = torch.as_tensor(a_scores).to(dev, dtype=torch.float32).reshape(-1).contiguous()
        if a_ids.shape[0] != B or a_scores.shape[0] != B:
            raise _lib.NrmsError("%s: after must be (ids [%d], scores [%d]) (got %s, %s)"
                                 % (who, B, B, tuple(a_ids.shape), tuple(a_scores.shape)))
        a_ids = torch.where(a_ids > 0, a_ids - 1, torch.where(a_ids == 0, torch.full_like(a_ids, -1), a_ids)).contiguous()
        return dict(after_scores=a_scores, after_ids=a_ids)

    @torch.no_grad()
    def recommend_request_capped(self, batch, k, catalogue, item_tag, cap, exclude_history=True, *, item_bias=None, n_tags=None,
                                 item_time=None, window=None, allow=None, adjust=None, after=None):
        """recommend_capped through recommend_request's filters -> (news_ids [B, k] int64, scores [B, k] fp32): a rationed front
        page ("at most two stories per category in my ten") that also expires news per user (item_time, window), mutes topics
        (allow, over the same item_tag), pushes down what was already shown (adjust) and serves page 2 (after)
        (include/nrms_hip.h nrms_topk_dot_request_capped).  Parity is unpinned: the reference has no catalogue retrieval.

        item_tag and cap are recommend_capped's (cap: an int with ``n_tags=``, an int tensor [n_tags] or [B, n_tags]); every other
        part is recommend_request's, optional, with the rules of its own method; ``allow`` is bool [B, n_tags] or its packed form
        and needs no item_tag of its own.  The walk is recommend_capped's over the news every part leaves open, in the order of the
        adjusted score: a news is taken iff its tag has room left in this call.  With every cap >= k this is recommend_request,
        with no other part recommend_capped, bit for bit.

        Paging: page j + 1 takes ``after`` = the last (id, score) column of page j and ``cap`` = remaining_caps(cap, every id
        served so far, item_tag, n_tags), the other parts unchanged; the pages laid end to end are then the columns of one call
        with k = the sum of the page lengths (<= 256), with nothing repeated or skipped across ties.  There is no rank under caps.
        Not combined with the fp16 shortlist, sections, the diversity re-ranking, the log-partition, explain or recommend_deep."""
        who = "recommend_request_capped"
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, who)
        bias = self._item_bias_rows(item_bias, cat, who)
        B, dev = user.shape[0], user.device
        caps, n_tags = self._cap_rows(cap, n_tags, B, int(k), cat.device, who)
        tags = self._item_tag_rows(item_tag, cat, who)
        kw = dict(self._time_window_rows(item_time, window, cat, B, who))
        if allow is not None:
            if (not torch.is_tensor(allow) or allow.dim() != 2 or allow.shape[0] != B or allow.device != cat.device
                    or not ((allow.dtype == torch.bool and allow.shape[1] == n_tags)
                            or (allow.dtype == torch.int32 and allow.shape[1] == (n_tags + 31) // 32))):
                got = ("%s %s on %s" % (tuple(allow.shape), allow.dtype, allow.device)) if torch.is_tensor(allow) else type(allow).__name__
                raise _lib.NrmsError("%s: allow must be a bool [%d, %d] tensor, or pack_tag_mask's int32 [%d, %d], on %s (got %s)"
                                     % (who, B, n_tags, B, (n_tags + 31) // 32, cat.device, got))
            kw.update(allow=allow)
        if adjust is not None:
            adj_ids, adj_delta = self._adjust_rows(adjust, cat, B, who)
            kw.update(adj_ids=adj_ids, adj_delta=adj_delta)
        if after is not None:
            kw.update(self._after_rows(after, B, dev, who))
        scores, ids = self._engine.top_k_request_capped(user, cat[1:], k, tags, n_tags, caps, exclude, bias=bias, **kw)
        return torch.where(ids >= 0, ids + 1, ids), scores

    @torch.no_grad()
    def rank_targets_request(self, batch, targets, catalogue, exclude_history=True, *, item_bias=None, item_time=None, window=None,
                             item_tag=None, allow=None, adjust=None):
        """rank_targets through recommend_request's filters -> (ranks [B, T] int32, scores [B, T] fp32): the 1-based place of news
        id targets[b, j] in recommend_request's list for user b were k unbounded, and its adjusted score (include/nrms_hip.h
        nrms_rank_dot_request).  A target closed by any part (outside the window, a muted tag, a NaN delta) comes back as rank 0 /
        score -inf, like every target rank_targets cannot rank.  The parts are recommend_request's, every other argument is
        rank_targets'."""
        who = "rank_targets_request"
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, who)
        bias = self._item_bias_rows(item_bias, cat, who)
        kw = self._request_rows(cat, user.shape[0], item_time, window, item_tag, allow, adjust, who)
        tg = torch.as_tensor(targets).to(user.device, dtype=torch.int64)
        if tg.dim() != 2 or tg.shape[0] != user.shape[0]:
            raise _lib.NrmsError("%s: targets must be [%d, T] news ids (got %s)" % (who, user.shape[0], tuple(tg.shape)))
        return self._engine.rank_of_request(user, cat[1:], (tg - 1).contiguous(), exclude, bias=bias, **kw)

    @torch.no_grad()
    def explain(self, batch, news_ids, catalogue, m=3, *, return_contributions=False):
        """Why these news: each score split exactly over the clicks of the user's history -> (reason_ids [B, K, m] int64,
        reason_contrib [B, K, m] fp32, total [B, K] fp32, padding_share [B, K] fp32), then with return_contributions the terms
        contrib [B, K, H] fp32 (include/nrms_hip.h nrms_attribution_dot).

        The user vector is the additive-attention sum over the history, user = sum_h w[h] ctx[h], so the score of news x is
        sum_h w[h] (ctx[h] . x): term h is what click h contributes, with no approximation.  news_ids [B, K] int64, K <= 256:
        what recommend / recommend_page / recommend_deep (256 columns per call) or the diversity re-ranking returned, news ids
        with -1 in the unfilled slots.  reason_ids[b, j] are the ``browsed_ids`` of the m history slots with the largest terms
        for news_ids[b, j], largest first (equal terms: the earlier slot), reason_contrib their terms; -1 / -inf where the user
        has fewer than m named clicks.  Negative terms are listed like any other: cut at 0 for "because you read".  1 <= m <= 8.

        total is the ordered sum of all H terms: the model's score of that news WITHOUT any ``item_bias``, equal to recommend's
        score up to the rounding of the two orders of summation (DESIGN.md section 8h has the measured difference).
        padding_share is the part of total carried by the slots that name no news: padding slots (``browsed_ids`` 0, or an id
        outside the catalogue, counted for check_recommend_ids as in recommend).  nrms_v0 masks nothing, so a padding slot has
        a context row of its own and carries part of the score; models that mask their history (nrms_bert) give those slots
        weight 0, except for a user without any click, whose softmax over equally masked slots is uniform: that score is all
        padding share.
        An entry of news_ids outside [0, N) gets total -inf, no reasons and zero terms.  Id 0, the padding title, is a
        catalogue row like any other here.  catalogue and ``browsed_ids`` as in recommend."""
        get = batch.get if hasattr(batch, "get") else batch.__getitem__
        browsed = get("browsed_ids")
        if browsed is None:
            raise KeyError("explain: the batch dict lacks 'browsed_ids' (the news ids of the clicked history)")
        dev = self._prepare()
        cat = torch.as_tensor(catalogue)
        d = self._catalogue_width()
        if cat.dim() != 2 or cat.shape[1] != d or cat.dtype != torch.float32 or cat.device != dev:
            raise _lib.NrmsError("explain: catalogue must be [N, %d] float32 on %s (encode_catalogue), got %s %s on %s"
                                 % (d, dev, tuple(cat.shape), cat.dtype, cat.device))
        cat = cat.contiguous()
        browsed = torch.as_tensor(browsed).to(dev, dtype=torch.int64).contiguous()
        B, H = browsed.shape
        ids = torch.as_tensor(news_ids).to(dev, dtype=torch.int64).contiguous()
        if ids.dim() != 2 or ids.shape[0] != B:
            raise _lib.NrmsError("explain: news_ids must be [%d, K] news ids (got %s)" % (B, tuple(ids.shape)))
        bad = (browsed < 0) | (browsed >= cat.shape[0])          # as _catalogue_query: counted, read as padding
        browsed = browsed.masked_fill(bad, 0)
        if self._bad_browsed is None or self._bad_browsed.device != dev:
            self._bad_browsed = torch.zeros((), dtype=torch.int64, device=dev)
        self._bad_browsed += bad.sum()
        _, ctx, w = self._catalogue_user_parts(cat.index_select(0, browsed.view(-1)).view(B, H, d), browsed)
        # the kernel's rows are catalogue rows, row 0 the padding title's: the whole catalogue and the ids as they are
        res = self._engine.attribution(ctx, w, cat, ids, m, slot_named=(browsed != 0).to(torch.uint8),
                                       return_contrib=return_contributions)
        slots = res[0].to(torch.int64)
        reason_ids = torch.where(slots >= 0, browsed.gather(1, slots.clamp(min=0).view(B, -1)).view_as(slots), slots)
        return (reason_ids,) + tuple(res[1:])

    def _catalogue_user_parts(self, hist, browsed=None):
        """_catalogue_users' pass with its pooling factors: (user [B, width], ctx [B, H, width], w [B, H])."""
        return self._engine.user_parts(self._flat, hist)

    @torch.no_grad()
    def sample_negatives(self, batch, row_key, S, catalogue, temperature, seed, exclude=None):
        """S negatives per user of ``batch`` drawn from the model's own softmax over the whole catalogue -> news ids [B, S]
        int64, -1 in an empty slot: a draw without replacement from softmax(score / temperature) over the eligible news, in
        Plackett-Luce order (slot 0 a draw from the softmax, slot 1 a draw from the rest, ...; include/nrms_hip.h
        nrms_softmax_sample_dot).  temperature > 0: large values approach the uniform draw, small ones "the S hardest".

        The user vector, the catalogue (encode_catalogue), the id-0 convention and the counting of bad ``browsed_ids`` are
        recommend's.  row_key [B] int64 in [0, 2^48) names each row's draw (e.g. the click's position in its log): a row's
        negatives are a function of (the weights, its history, its key, temperature, seed, its exclude list) only, whatever
        else is in the batch.  exclude [B, n] news ids padded with -1: news the user must not get (ClickFeed: the user's own
        clicks, which contain the positive); None: the browsed ids.  News id 0, the padding title, is never drawn."""
        if not float(temperature) > 0.0 or not np.isfinite(float(temperature)):
            raise _lib.NrmsError("sample_negatives: temperature must be finite and > 0 (got %r)" % (temperature,))
        user, cat, browsed_rows = self._catalogue_query(batch, catalogue, exclude is None, "sample_negatives")
        dev = user.device
        if exclude is not None:
            ex = torch.as_tensor(exclude).to(dev, dtype=torch.int64)
            if ex.dim() != 2 or ex.shape[0] != user.shape[0]:
                raise _lib.NrmsError("sample_negatives: exclude must be [%d, n] news ids (got %s)" % (user.shape[0], tuple(ex.shape)))
            browsed_rows = (ex - 1).contiguous()          # rows 1.. as in recommend: -1 and id 0 fall out of range
        key = torch.as_tensor(row_key).to(dev, dtype=torch.int64).contiguous()
        ids = self._engine.softmax_sample(user, cat[1:], key, S, 1.0 / float(temperature), seed, browsed_rows)
        return torch.where(ids >= 0, ids + 1, ids)

    @staticmethod
    def _likelihood_variants(who, temperature, bias_scale, item_bias):
        """(inv_temperature [J], bias_scale [J] or None) of log_partition / log_prob from their ``temperature`` / ``bias_scale``."""
        temps = [float(t) for t in (temperature if hasattr(temperature, "__len__") else [temperature])]
        if not 1 <= len(temps) <= 8:
            raise _lib.NrmsError("%s: temperature must be a float or 1 .. 8 floats (got %d)" % (who, len(temps)))
        for t in temps:
            if not t > 0.0:          # (refuses NaN too; inf is the uniform distribution)
                raise _lib.NrmsError("%s: every temperature must be > 0 (inf: the uniform distribution); got %r" % (who, t))
        inv_t = [0.0 if np.isinf(t) else 1.0 / t for t in temps]
        if bias_scale is None:
            return inv_t, None
        if item_bias is None:
            raise _lib.NrmsError("%s: bias_scale scales item_bias (give item_bias)" % who)
        scale = [float(v) for v in (bias_scale if hasattr(bias_scale, "__len__") else [bias_scale] * len(temps))]
        if len(scale) != len(temps) or not all(np.isfinite(v) for v in scale):
            raise _lib.NrmsError("%s: bias_scale must be one finite float per temperature (got %r for %d temperatures)"
                                 % (who, bias_scale, len(temps)))
        return inv_t, scale

    @torch.no_grad()
    def log_partition(self, batch, catalogue, temperature=1.0, exclude_history=True, *, item_bias=None, bias_scale=None,
                      return_stats=False):
        """The log-partition of the served softmax over the whole catalogue -> lse [B, J] fp32 (with return_stats: (lse, zmax
        [B, J] fp32, n_eligible [B, J] int32)): lse[b, j] = log sum over the news user b could be recommended of
        exp(score / temperature[j] + bias_scale[j] * item_bias[id]), exactly and without a [B, N] matrix, all J variants in one
        pass pair over the catalogue (include/nrms_hip.h nrms_logsumexp_dot).  Parity is unpinned: the reference scores shown
        candidates only.

        temperature: a float or up to 8 floats, each > 0; ``float('inf')`` is the uniform distribution (lse = log n_eligible).
        item_bias: recommend's per-news prior (float32 [N] by news id; a NaN entry removes that news for everybody); bias_scale:
        None (scale 1) or one finite float per temperature, e.g. a grid of ``--popularity_prior`` ALPHA over one log-popularity.
        The user vector, the catalogue, the id-0 rule (the padding title never competes), ``exclude_history`` and the counting
        of bad ``browsed_ids`` are recommend's.  There is no time window here yet."""
        inv_t, scale = self._likelihood_variants("log_partition", temperature, bias_scale, item_bias)
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, "log_partition")
        bias = self._item_bias_rows(item_bias, cat, "log_partition")
        lse, zmax, n_el = self._engine.log_partition(user, cat[1:], inv_t, exclude, bias=bias, bias_scale=scale)
        return (lse, zmax, n_el) if return_stats else lse

    @torch.no_grad()
    def log_prob(self, batch, targets, catalogue, temperature=1.0, exclude_history=True, *, item_bias=None, bias_scale=None):
        """The log-probability of given news under the served softmax over the whole catalogue -> [B, T, J] fp32:
        z_j(target) - lse_j with log_partition's lse and z_j(target) = fmaf(score, 1 / temperature[j], bias_scale[j] *
        item_bias[id]) formed from rank_targets' score bits (the plain dot product, without the prior).  NaN where rank_targets
        gives rank 0 (id 0, an id outside the catalogue, a NaN score or prior and, with exclude_history, a browsed id); <= 0
        for every other target, and exp of it sums to 1 over a user's eligible catalogue.  The arguments are log_partition's and
        rank_targets'."""
        inv_t, scale = self._likelihood_variants("log_prob", temperature, bias_scale, item_bias)
        user, cat, exclude = self._catalogue_query(batch, catalogue, exclude_history, "log_prob")
        bias = self._item_bias_rows(item_bias, cat, "log_prob")
        tg = torch.as_tensor(targets).to(user.device, dtype=torch.int64)
        if tg.dim() != 2 or tg.shape[0] != user.shape[0]:
            raise _lib.NrmsError("log_prob: targets must be [%d, T] news ids (got %s)" % (user.shape[0], tuple(tg.shape)))
        rows = (tg - 1).contiguous()
        ranks, scores = self._engine.rank_of(user, cat[1:], rows, exclude)
        lse, _, _ = self._engine.log_partition(user, cat[1:], inv_t, exclude, bias=bias, bias_scale=scale)
        return _target_log_prob(ranks, scores, rows, lse, inv_t, scale, bias)

    @staticmethod
    def _item_bias_rows(item_bias, cat, who):
        """The kernels' view of a per-news prior: rows 1.. like the catalogue's (None stays None)."""
        if item_bias is None:
            return None
        N = cat.shape[0]
        if (not torch.is_tensor(item_bias) or item_bias.dim() != 1 or item_bias.shape[0] != N or item_bias.dtype != torch.float32
                or item_bias.device != cat.device):
            got = ("%s %s on %s" % (tuple(item_bias.shape), item_bias.dtype, item_bias.device)) if torch.is_tensor(item_bias) \
                else type(item_bias).__name__
            raise _lib.NrmsError("%s: item_bias must be [%d] float32 on %s, indexed by news id like the catalogue (got %s)"
                                 % (who, N, cat.device, got))
        return item_bias.contiguous()[1:]

    @staticmethod
    def _time_window_rows(item_time, window, cat, B, who):
        """The kernels' view of a time window: {} when neither is given, else item_time rows 1.. like the catalogue's and the
        window, as keywords of engine.top_k / rank_of (which check dtype and range)."""
        if item_time is None and window is None:
            return {}
        if item_time is None or window is None:
            raise _lib.NrmsError("%s: item_time and window go together (window %s, item_time %s)"
                                 % (who, "missing" if window is None else "given", "missing" if item_time is None else "given"))
        N = cat.shape[0]
        for name, t, shape in (("item_time", item_time, (N,)), ("window", window, (B, 2))):
            if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype not in (torch.int32, torch.int64) or t.device != cat.device):
                got = ("%s %s on %s" % (tuple(t.shape), t.dtype, t.device)) if torch.is_tensor(t) else type(t).__name__
                raise _lib.NrmsError("%s: %s must be an int32 or int64 %s tensor on %s%s (got %s)"
                                     % (who, name, list(shape), cat.device, ", indexed by news id like the catalogue" if name == "item_time" else "", got))
        return {"item_time": item_time.contiguous()[1:], "window": window}

    def _catalogue_query(self, batch, catalogue, exclude_history, who):
        """What recommend and rank_targets share: (user vectors [B, width], the checked catalogue, the exclude list in
        the kernel's row numbering or None)."""
        get = batch.get if hasattr(batch, "get") else batch.__getitem__
        browsed = get("browsed_ids")
        if browsed is None:
            raise KeyError("%s: the batch dict lacks 'browsed_ids' (the news ids of the clicked history)" % who)
        dev = self._prepare()
        cat = torch.as_tensor(catalogue)
        d = self._catalogue_width()
        if cat.dim() != 2 or cat.shape[1] != d or cat.dtype != torch.float32 or cat.device != dev:
            raise _lib.NrmsError("%s: catalogue must be [N, %d] float32 on %s (encode_catalogue), got %s %s on %s"
                                 % (who, d, dev, tuple(cat.shape), cat.dtype, cat.device))
        cat = cat.contiguous()
        browsed = torch.as_tensor(browsed).to(dev, dtype=torch.int64).contiguous()
        B, H = browsed.shape
        N = cat.shape[0]
        # ids outside the catalogue are counted on the device and read as padding (no host synchronisation per batch);
        # check_recommend_ids() raises on them
        bad = (browsed < 0) | (browsed >= N)
        browsed = browsed.masked_fill(bad, 0)
        if self._bad_browsed is None or self._bad_browsed.device != dev:
            self._bad_browsed = torch.zeros((), dtype=torch.int64, device=dev)
        self._bad_browsed += bad.sum()
        user = self._catalogue_users(cat.index_select(0, browsed.view(-1)).view(B, H, d), browsed)
        # the kernel runs on rows 1.. (the padding title is never a candidate); history ids shift with them, which sends
        # the padding slots (id 0) out of range, where the kernel ignores them
        return user, cat, (browsed - 1 if exclude_history else None)

    def _catalogue_width(self):
        return self._dims.word_embed_size

    def _catalogue_users(self, hist, browsed=None):
        """Catalogue rows of the history [B, H, width] (browsed: their ids, 0 = padding slot) -> user vectors [B, width]."""
        return self._engine.encode_users(self._flat, hist, tag="user_eval")

    _bad_browsed = None
    CATALOGUE_RETRIEVAL = True          # recommend / encode_catalogue are available (run_v0 --recommend checks this)
    CATALOGUE_RANKING = True            # the catalogue score is a plain dot product: rank_targets (run_v0 --retrieval_metrics)
    CATALOGUE_SAMPLING = True           # ... so negatives can be drawn from its softmax: sample_negatives (run_v0 --negatives adaptive)
    CATALOGUE_SECTIONS = True           # ... and selected per section: recommend_sections (run_v0 --sections)
    CATALOGUE_PAGING = True             # ... and paged through with a cursor: recommend_page / recommend_deep (run_v0 --recommend_deep)
    CATALOGUE_EXPLAIN = True            # ... and split over the clicks of the history: explain (run_v0 --explain)
    CATALOGUE_LIKELIHOOD = True         # ... and normalised over the catalogue: log_partition / log_prob (run_v0 --retrieval_nll)
    CATALOGUE_CAPS = True               # ... and rationed by a hard cap per tag: recommend_capped (run_v0 --max_per_category)
    CATALOGUE_TAGS = True               # ... and restricted to a per-user tag set: recommend_tagged / rank_targets_tagged (run_v0 --only_categories)
    CATALOGUE_ADJUST = True             # ... and moved per (user, news) by a finite amount: recommend_adjusted / rank_targets_adjusted (run_v0 --seen_discount)

    def check_recommend_ids(self):
        """Raises if a recommend() or rank_targets() call since the last check met browsed_ids outside its catalogue (those slots were read
        as padding).  One host synchronisation."""
        n = 0 if self._bad_browsed is None else int(self._bad_browsed.item())
        if n:
            self._bad_browsed.zero_()
            raise _lib.NrmsError("recommend: %d browsed_ids outside the catalogue were read as padding" % n)

