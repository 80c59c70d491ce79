"""User-news graph encoder on MI355X (BASELINE configs[4]): neighbour gather + attention aggregate.

PARITY UNPINNED.  The reference repository holds no graph model (``/root/reference/README.md:3`` names Adressa, no code follows;
``model/tanr.py`` is empty), so there is nothing of the reference's to match; the model is specified here, as a two-layer
attention aggregation over a sampled sub-graph of the bipartite click graph (the aggregation of GERL, Ge et al., WWW 2020, with
the reference's additive attention, ``model/nrms_v0.py:100-126``, as the aggregator), and checked against
``oracle/segpool_oracle.py``.  It keeps the reference's plugin API -- ``Model(config)``, ``forward(batch_dict) -> [B, C]`` with
masked candidates at -1e9 -- and reads, beside the NRMS keys of ``data_handler.py:236-250`` (``browsed_titles``,
``browsed_mask``, ``candidate_titles``, ``candidate_mask``), one new key:

  ``neighbor_rows`` [B * (H + C), K] int64 -- for every news slot of the batch (row r < B * H: history slot (r // H, r % H); row
  B * H + b * C + c: candidate c of user b) up to K sampled neighbour news (news clicked by the users who clicked it), as ROWS of
  the same numbering; -1 = none.  The sampler draws neighbours from the batch's own news (an induced sub-graph), so a
  data-parallel rank needs no remote rows: users -- and their sub-graphs -- shard across GPUs, gradients all-reduce (RCCL).

Specification (n_r = NRMS news encoder of slot r's title, ``nrms_v0.py:154-176``; AddPool as in model/hierec_hip.py):
  news layer:  g_r = n_r + AddPool({n_k : k in neighbor_rows[r]}; neighbor_attention)          (no neighbours: g_r = n_r)
  user layer:  h_b = AddPool({g_r : r a history slot of b with browsed_mask = 1}; user_attention)  (no click: 0)
  score(b, c) = <g_cand(b, c), h_b>                                                               (``nrms_v0.py:205-216``)
Both aggregations are ``nrms_segment_pool_fwd / _bwd`` (csrc/segpool.hip) over index lists built on the device by
``nrms_csr_from_padded``; a news row is listed by many segments, so the news layer's backward sorts the list entries by row and
adds a row's shares in list order (no atomics: bit-reproducible, include/nrms_hip.h).  A batch without ``neighbor_rows`` (the
reference's loader knows no graph) gets them from ``graph_sampler.induced_neighbor_rows``.  No CPU fallback.

Neighbours outside the batch.  The batch may also carry

  ``neighbor_vectors`` [M, d] fp32 -- CONSTANT news vectors; ``neighbor_rows`` may then index [0, N + M), N = B * (H + C): row
  N + e is ``neighbor_vectors[e]``.  The news layer pools over the N + M rows into the N slots; the constant rows take no
  gradient (the backward drops the last M rows of dx) but do feed the gradients of ``neighbor_attention.*``.

``Model.attach_click_graph(graph, titles)`` (click_graph.ClickGraph, e.g. ``DeviceFeed.click_graph()`` with ``DeviceFeed.titles``)
replaces the induced sampler: from then on a batch without ``neighbor_rows`` gets both keys on the device, from its
``browsed_ids``, ``browsed_mask`` and ``candidate_ids`` (a KeyError names them when they are missing), the graph and a seed --
``nrms_graph_sample_neighbors`` draws every slot's ``config.graph_neighbors`` neighbours from the click graph of the WHOLE data
set as a function of (graph, news id, draw, seed), ``nrms_graph_resolve_rows`` turns them into rows (a neighbour the batch shows:
its first slot; any other: row N + e) and ``neighbor_vectors`` = the catalogue gathered at the call's ``extra_ids``, always
``config.graph_extra_rows`` rows (no per-batch host read; distinct out-of-batch neighbours beyond that many are dropped, largest
ids first, and counted: ``check_click_graph``).  The training seed is the train-step counter: the number of batches trained on
so far (``train_step`` calls and train-mode forwards with autograd enabled; a train-mode forward under ``no_grad`` draws with the
current value and leaves it).  It is not part of ``state_dict()``: a run resumed from a checkpoint starts again at 0 (set
``_graph_step`` to continue the sequence).  The evaluation seed is the constant ``EVAL_SEED``, so an evaluation is a function of
weights and data alone.

Staleness rule (part of this specification).  The catalogue is ``encode_catalogue(titles)``: the dropout-free,
evaluation-precision news vectors n_r of every news.  It is recomputed on attach, by ``refresh_neighbor_vectors()``
(``train_eval.train`` calls it at every epoch start) and lazily on the first eval-mode forward after the parameters changed, so
evaluation always sees current vectors, while TRAINING sees out-of-batch neighbour vectors at most one epoch stale -- on purpose:
historical embeddings for out-of-batch neighbours, which carry no gradient.  "Changed" = a ``train_step``, a forward that autograd
will differentiate, or a ``load_state_dict``; after writing into parameters by hand call ``refresh_neighbor_vectors()``.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from ..engine import FlatLayout, ModelDims, NRMSEngine, _stream
from ..segpool import SegmentPool
from . import nrms_hip
from ._flat_model import FlatHipModel, additive_entries, news_encoder_entries

LEVELS = ("neighbor_attention", "user_attention")


class GraphEngine(NRMSEngine):
    """Forward / backward of the graph encoder on one GPU: the NRMS engine's news encoder, two segment pools, click scores."""

    def _csr(self, key, lists, n_rows):
        n_seg, K = lists.shape
        ptr = self._buf(key + "_ptr", n_seg + 1, torch.int32)[:n_seg + 1]
        idx = self._buf(key + "_idx", n_seg * K, torch.int32)[:n_seg * K]
        rc = self.lib.nrms_csr_from_padded(C.c_int64(n_seg), int(K), _lib.ptr(lists), C.c_int64(n_rows), _lib.ptr(ptr), _lib.ptr(idx), _stream())
        _lib.check(rc, "nrms_csr_from_padded")
        return ptr, idx

    def forward(self, flat, batch, training, p_drop=0.0, seed=0):
        bt, ct = batch["browsed_titles"], batch["candidate_titles"]
        B, H, L = bt.shape
        Cn = ct.shape[1]
        d, q = self.dims.word_embed_size, self.dims.query_vector_dim
        N = B * (H + Cn)
        nbr = batch["neighbor_rows"].to(torch.int64).contiguous()
        if nbr.dim() != 2 or nbr.shape[0] != N:
            raise _lib.NrmsError("graph: neighbor_rows must be [B * (H + C) = %d, K], got %s" % (N, tuple(nbr.shape)))
        sfx = "" if training else "_eval"
        self.poll_ids()
        ids = self._buf("ids" + sfx, N * L, torch.int64)[:N * L].view(N, L)
        self.sanitize_ids(bt.reshape(B * H, L).contiguous(), ids[:B * H])
        self.sanitize_ids(ct.reshape(B * Cn, L).contiguous(), ids[B * H:])
        ext = batch.get("neighbor_vectors")
        M = 0
        if ext is not None:
            if ext.dim() != 2 or ext.shape[1] != d or ext.dtype != torch.float32:
                raise _lib.NrmsError("graph: neighbor_vectors must be [M, %d] float32, got %s %s" % (d, tuple(ext.shape), ext.dtype))
            M = ext.shape[0]
        # rows [0, N): the slots' own vectors; rows [N, N + M): the constant vectors of out-of-batch neighbours
        x = self._buf("news_vec" + sfx, (N + M) * d)[:(N + M) * d].view(N + M, d)
        nv = x[:N]
        if M:
            x[N:].copy_(ext)
        p = float(p_drop)
        self.encode_titles(flat, ids, out=nv, p_embed=p, p_ctx=p, seed=seed, save=training, tag="news" + sfx, trusted_ids=True)
        # ---- index lists: every slot's neighbours; every user's clicked slots (history rows with browsed_mask = 1)
        n_ptr, n_idx = self._csr("nbr" + sfx, nbr, N + M)
        slots = torch.arange(B * H, device=self.device, dtype=torch.int64).view(B, H)
        hist = torch.where(batch["browsed_mask"].to(torch.bool), slots, torch.full_like(slots, -1)).contiguous()
        u_ptr, u_idx = self._csr("hist" + sfx, hist, B * H)
        lay = self.layout
        W = {lv: (lay.view(flat, lv + ".linear.weight"), lay.view(flat, lv + ".linear.bias"), lay.view(flat, lv + ".attention_query_vector"))
             for lv in LEVELS}
        prec = "fp32" if self.precision == "fp32" else "bf16x3"
        pool_n = SegmentPool(d, q, prec, rows_unique=False)
        pool_u = SegmentPool(d, q, prec, rows_unique=True)
        g = pool_n.forward(x, *W[LEVELS[0]], n_ptr, n_idx)           # [N, d]: the neighbour aggregate ...
        g += nv                                                      # ... + the slot's own vector
        h = pool_u.forward(g, *W[LEVELS[1]], u_ptr, u_idx)           # [B, d]
        mask = batch.get("candidate_mask")
        if mask is not None:
            mask = mask.to(torch.uint8).contiguous()
        scores = torch.empty(B, Cn, dtype=torch.float32, device=self.device)
        self.click_scores(g[B * H:].view(B, Cn, d), h, mask, out=scores)
        self._bad_host.copy_(self._bad_ids, non_blocking=True)
        if training:
            self._gen += 1
            self._saved = dict(B=B, H=H, C=Cn, L=L, ids=ids, g=g, h=h, mask=mask, pools=(pool_n, pool_u), p=p, seed=seed, gen=self._gen)
        return scores

    def pooled_ce_loss(self, *args, **kwargs):
        raise NotImplementedError("GraphEngine has no pooled loss (config.train_loss = 'pooled'): its candidate vectors are not the tail of one vector buffer")

    def backward(self, flat, gflat, dscores, gen=None, table_grad_ready=None):
        sv = self._saved
        if sv is None:
            raise _lib.NrmsError("backward() without a training forward()")
        if gen is not None and gen != sv["gen"]:
            raise _lib.NrmsError("backward() for training forward #%d, but the saved activations belong to forward #%d" % (gen, sv["gen"]))
        B, H, Cn, L = sv["B"], sv["H"], sv["C"], sv["L"]
        d = self.dims.word_embed_size
        n, N = B * H, B * (H + Cn)
        lay = self.layout
        self.poll_grad_overflow()
        self.loss_scale = float(getattr(self, "loss_scale_override", None) or -float(self.loss_scale_backoff))
        g, h = sv["g"], sv["h"]
        dcand = self._buf("d_cand", B * Cn * d)[:B * Cn * d].view(B * Cn, d)
        dh = self._buf("d_user_vec", B * d)[:B * d].view(B, d)
        rc = self.lib.nrms_click_score_bwd(B, Cn, d, C.c_void_p(g[n:].data_ptr()), _lib.ptr(h), _lib.ptr(sv["mask"]), _lib.ptr(dscores.contiguous()),
                                           _lib.ptr(dcand), _lib.ptr(dh), _stream())
        _lib.check(rc, "nrms_click_score_bwd")
        gv = lambda name: lay.view(gflat, name)
        fv = lambda name: lay.view(flat, name)
        pool_n, pool_u = sv["pools"]

        def level(pool, lv, dout):
            return pool.backward(fv(lv + ".linear.weight"), fv(lv + ".attention_query_vector"), dout, gv(lv + ".linear.weight"),
                                 gv(lv + ".linear.bias"), gv(lv + ".attention_query_vector"))

        dg = level(pool_u, LEVELS[1], dh)                            # [N, d] (rows outside every history list: 0)
        dg[n:] += dcand
        dnv = level(pool_n, LEVELS[0], dg)[:N]                       # through the neighbour aggregate (constant rows dropped) ...
        dnv += dg                                                    # ... and the slot's own vector
        desc_n = self._desc("news_encoder", N, L, sv["p"], sv["p"], sv["seed"], training=True)
        ws = self._bwd_workspace(desc_n)
        wn, gn = self._weights(flat, "news_encoder"), self._grads(gflat, "news_encoder")
        acts_n = self._acts("news", N * L, True, gather=True, desc=desc_n)
        if desc_n.precision == _lib.NRMS_PRECISION_FP16:
            desc_n.flags |= _lib.NRMS_FLAG_FWD_SCRATCH_KEPT
        rc = self.lib.nrms_encoder_bwd(C.byref(desc_n), C.byref(wn), _lib.ptr(sv["ids"]), None, None, C.byref(acts_n), _lib.ptr(dnv),
                                       C.byref(gn), None, _lib.ptr(ws), C.c_size_t(ws.numel() * 4), _stream())
        _lib.check(rc, "nrms_encoder_bwd(news)")
        if table_grad_ready is not None:
            table_grad_ready()


class Model(FlatHipModel):
    """User-news graph encoder: ``Model(config)``, ``forward(batch) -> scores [B, C]`` (``model/__init__.py:22-23,38``)."""
    KEYS = ("browsed_titles", "browsed_mask", "candidate_titles", "candidate_mask", "neighbor_rows", "neighbor_vectors")
    OPTIONAL = ("candidate_mask", "neighbor_vectors")
    EVAL_SEED = 0x6A09E667F3BCC908          # the sampler's seed of every eval-mode forward (any constant would do)

    def __init__(self, config, pretrained_word_embedding=None):
        super().__init__()
        self.config = config
        table = nrms_hip._load_table(config, pretrained_word_embedding)
        V, d = table.shape
        q = int(config.query_vector_dim)
        self.news_encoder = nrms_hip._NewsEncoderParams(config, table)
        self.neighbor_attention = nrms_hip._AdditiveAttentionParams(q, d)
        self.user_attention = nrms_hip._AdditiveAttentionParams(q, d)
        self._dims = ModelDims(n_words=int(V), word_embed_size=int(d), num_attention_heads=int(config.num_attention_heads), query_vector_dim=q)
        extra = []
        for lv in LEVELS:
            extra += additive_entries(lv, q, d)
        self._graph = self._graph_titles = self._catalogue = None
        self._catalogue_stale = False
        self._graph_step = 0
        self._finish(FlatLayout(self._dims, news_encoder_entries(self._dims, extra)), table.device)
        self.register_load_state_dict_post_hook(Model._mark_catalogue_stale)

    def _make_engine(self, device, precision):
        return GraphEngine(self._dims, device, precision=precision, layout=self._layout)

    # ---- the global click graph ------------------------------------------------------------------------
    @staticmethod
    def _mark_catalogue_stale(module, incompatible_keys=None):
        module._catalogue_stale = True

    @torch.no_grad()
    def encode_catalogue(self, titles):
        """titles [N, L] word ids, row r = news id r (``DeviceFeed.titles``) -> news vectors n_r [N, d]: dropout-free, in the
        precision evaluation runs in, whatever the module's train / eval mode (as ``nrms_hip.Model.encode_catalogue``)."""
        dev = self._prepare()
        return self._engine.encode_titles(self._flat, nrms_hip._ids_on(dev, titles), tag="news_eval")

    CATALOGUE_RANKING = False
    CATALOGUE_SAMPLING = False          # the catalogue score is not one dot product per user: no sample_negatives

    def rank_targets(self, batch, targets, catalogue, exclude_history=True, *, item_bias=None, item_time=None, window=None):
        if item_time is not None or window is not None:
            raise _lib.NrmsError("graph: rank_targets takes no item_time / window: the model cannot rank a catalogue at all, a "
                                 "candidate's score depends on its neighbours in the click graph")
        if item_bias is not None:
            raise _lib.NrmsError("graph: rank_targets takes no item_bias: the model cannot rank a catalogue at all, a candidate's "
                                 "score depends on its neighbours in the click graph")
        raise NotImplementedError("graph: rank_targets is not available: a candidate's score depends on its neighbours in the "
                                  "click graph, not on a catalogue row alone (no recommend either)")

    def recommend(self, batch, k, catalogue, exclude_history=True, *, diversity=None, shortlist=None, return_ild=False,
                  item_bias=None, item_time=None, window=None, coarse=None, coarse_shortlist=None, return_certified=False):
        if coarse is not None or coarse_shortlist is not None or return_certified:
            raise _lib.NrmsError("graph: recommend takes no coarse / coarse_shortlist / return_certified: the model cannot "
                                 "recommend from a catalogue at all, a candidate's score depends on its neighbours in the click graph")
        if item_time is not None or window is not None:
            raise _lib.NrmsError("graph: recommend takes no item_time / window: the model cannot recommend from a catalogue at "
                                 "all, a candidate's score depends on its neighbours in the click graph")
        if item_bias is not None:
            raise _lib.NrmsError("graph: recommend takes no item_bias: the model cannot recommend from a catalogue at all, a "
                                 "candidate's score depends on its neighbours in the click graph")
        if diversity is not None or shortlist is not None or return_ild:
            raise _lib.NrmsError("graph: recommend has no diversity re-ranking (diversity / shortlist / return_ild): the model "
                                 "cannot recommend from a catalogue at all, a candidate's score depends on its neighbours in the "
                                 "click graph")
        raise NotImplementedError("graph: recommend is not available: a candidate's score depends on its neighbours in the "
                                  "click graph, not on a catalogue row alone")

    CATALOGUE_PAGING = False

    def recommend_page(self, batch, k, catalogue, after=None, exclude_history=True, *, item_bias=None, item_time=None, window=None):
        raise NotImplementedError("graph: recommend_page is not available: a candidate's score depends on its neighbours in the "
                                  "click graph, not on a catalogue row alone (no recommend either, so no ranking to page through)")

    def recommend_deep(self, batch, K, catalogue, exclude_history=True, *, item_bias=None, item_time=None, window=None):
        raise NotImplementedError("graph: recommend_deep is not available: a candidate's score depends on its neighbours in the "
                                  "click graph, not on a catalogue row alone (no recommend either, at any depth)")

    CATALOGUE_SECTIONS = False

    def recommend_sections(self, batch, k, sectioned, exclude_history=True, *, item_bias=None):
        raise NotImplementedError("graph: recommend_sections is not available: a candidate's score depends on its neighbours in "
                                  "the click graph, not on a catalogue row alone (no recommend either)")

    CATALOGUE_TAGS = False

    def recommend_tagged(self, batch, k, catalogue, item_tag, allow, exclude_history=True, *, item_bias=None):
        raise NotImplementedError("graph: recommend_tagged is not available: a candidate's score depends on its neighbours in the "
                                  "click graph, not on a catalogue row alone (no recommend either, inside a tag set or outside)")

    def rank_targets_tagged(self, batch, targets, catalogue, item_tag, allow, exclude_history=True, *, item_bias=None):
        raise NotImplementedError("graph: rank_targets_tagged is not available: a candidate's score depends on its neighbours in "
                                  "the click graph, not on a catalogue row alone (no rank_targets either)")

    CATALOGUE_CAPS = False

    def recommend_capped(self, batch, k, catalogue, item_tag, cap, exclude_history=True, *, item_bias=None, n_tags=None):
        raise NotImplementedError("graph: recommend_capped is not available: a candidate's score depends on its neighbours in the "
                                  "click graph, not on a catalogue row alone (no recommend either, with caps or without)")

    CATALOGUE_ADJUST = False

    def recommend_adjusted(self, batch, k, catalogue, adjust, exclude_history=True, *, item_bias=None):
        raise NotImplementedError("graph: recommend_adjusted is not available: a candidate's score depends on its neighbours in the "
                                  "click graph, not on a catalogue row alone (no recommend either, adjusted or not)")

    def rank_targets_adjusted(self, batch, targets, catalogue, adjust, exclude_history=True, *, item_bias=None):
        raise NotImplementedError("graph: rank_targets_adjusted is not available: a candidate's score depends on its neighbours in "
                                  "the click graph, not on a catalogue row alone (no rank_targets either)")

    def recommend_request(self, batch, k, catalogue, exclude_history=True, **parts):
        raise NotImplementedError("graph: recommend_request is not available: a candidate's score depends on its neighbours in the "
                                  "click graph, not on a catalogue row alone (no recommend either, through a request or not)")

    def recommend_request_capped(self, batch, k, catalogue, item_tag, cap, exclude_history=True, **parts):
        raise NotImplementedError("graph: recommend_request_capped is not available: a candidate's score depends on its neighbours "
                                  "in the click graph, not on a catalogue row alone (no recommend either, with caps or without)")

    def rank_targets_request(self, batch, targets, catalogue, exclude_history=True, **parts):
        raise NotImplementedError("graph: rank_targets_request is not available: a candidate's score depends on its neighbours in "
                                  "the click graph, not on a catalogue row alone (no rank_targets either)")

    CATALOGUE_LIKELIHOOD = False        # the catalogue score is not one dot product per user: no log_partition / log_prob

    def log_partition(self, batch, catalogue, temperature=1.0, exclude_history=True, *, item_bias=None, bias_scale=None,
                      return_stats=False):
        raise NotImplementedError("graph: log_partition is not available: a candidate's score depends on its neighbours in the click graph, so there is no softmax over one dot product per user to normalise (no recommend either)")

    def log_prob(self, batch, targets, catalogue, temperature=1.0, exclude_history=True, *, item_bias=None, bias_scale=None):
        raise NotImplementedError("graph: log_prob is not available: a candidate's score depends on its neighbours in the click graph, so there is no softmax over one dot product per user to normalise (no recommend either)")

    CATALOGUE_EXPLAIN = False

    def explain(self, batch, news_ids, catalogue, m=3, *, return_contributions=False):
        raise NotImplementedError("graph: explain is not available: a candidate's score depends on its neighbours in the click "
                                  "graph, so it is no sum of one term per click of the history (no recommend either)")

    def attach_click_graph(self, graph, titles):
        """From now on a batch without ``neighbor_rows`` takes its neighbours from ``graph`` (click_graph.ClickGraph on the
        model's device) instead of the batch-induced host sampler; titles [graph.n_news, L]: the word ids of every news, row r =
        news id r.  The catalogue is encoded here (module docstring: staleness rule)."""
        dev = self._prepare()
        titles = nrms_hip._ids_on(dev, titles)
        if graph.device != dev:
            raise _lib.NrmsError("attach_click_graph: the graph is on %s, the model on %s" % (graph.device, dev))
        if titles.dim() != 2 or titles.shape[0] != graph.n_news:
            raise _lib.NrmsError("attach_click_graph: titles must be [n_news = %d, L], got %s" % (graph.n_news, tuple(titles.shape)))
        K, cap = int(getattr(self.config, "graph_neighbors", 8)), int(getattr(self.config, "graph_extra_rows", 16384))
        if not 1 <= K <= 64 or cap < 0:
            raise _lib.NrmsError("attach_click_graph: config.graph_neighbors = %d must be in [1, 64], config.graph_extra_rows = %d >= 0" % (K, cap))
        self._graph, self._graph_titles = graph, titles
        self._graph_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self._graph_dropped = torch.zeros(1, dtype=torch.int32, device=dev)
        self.refresh_neighbor_vectors()

    def refresh_neighbor_vectors(self):
        """Re-encode the catalogue the out-of-batch neighbour vectors are gathered from (no-op without an attached graph)."""
        if self._graph is None:
            return None
        self._catalogue = self.encode_catalogue(self._graph_titles)
        self._catalogue_stale = False
        return self._catalogue

    def check_click_graph(self):
        """One host synchronisation.  Raises if a batch since the last check held browsed_ids / candidate_ids outside the graph's
        [0, n_news) (their slots got no neighbours); returns how many distinct out-of-batch neighbours were dropped since the
        last check because a batch had more than config.graph_extra_rows of them (0: none; raise the field otherwise)."""
        if self._graph is None:
            return 0
        bad, dropped = int(self._graph_bad.item()), int(self._graph_dropped.item())
        self._graph_bad.zero_()
        self._graph_dropped.zero_()
        if bad:
            raise _lib.NrmsError("graph: %d news id(s) outside the click graph's [0, %d) among browsed_ids / candidate_ids" % (bad, self._graph.n_news))
        return dropped

    def _global_neighbors(self, batch, dev):
        get = batch.get if hasattr(batch, "get") else (lambda k: batch[k])
        missing = [k for k in ("browsed_ids", "candidate_ids") if get(k) is None]
        if missing:
            raise KeyError("%s: with an attached click graph the batch dict needs %s (the news ids of its slots)"
                           % (type(self).__module__, " and ".join(repr(k) for k in missing)))
        ids = lambda k: torch.as_tensor(get(k)).to(dev, dtype=torch.int64)
        bi, ci = ids("browsed_ids"), ids("candidate_ids")
        valid = torch.as_tensor(batch["browsed_mask"]).to(dev) != 0
        slot_ids = torch.cat([torch.where(valid, bi, torch.zeros_like(bi)).reshape(-1), ci.reshape(-1)])
        if self.training:
            # the train-step counter: it advances with the batches that are trained on (train_step, or a forward that
            # autograd will differentiate), not with a train-mode forward under no_grad
            seed = self._graph_step
            if torch.is_grad_enabled():
                self._graph_step += 1
        else:
            seed = self.EVAL_SEED
            if self._catalogue_stale:
                self.refresh_neighbor_vectors()
        g = self._graph
        nbr = g.sample_neighbors(slot_ids, int(getattr(self.config, "graph_neighbors", 8)), seed, n_bad=self._graph_bad)
        rows, extra_ids, _ = g.resolve_rows(slot_ids, nbr, int(getattr(self.config, "graph_extra_rows", 16384)), n_dropped=self._graph_dropped)
        out = {k: get(k) for k in self.KEYS if k not in ("neighbor_rows", "neighbor_vectors") and get(k) is not None}
        out["neighbor_rows"] = rows
        out["neighbor_vectors"] = self._catalogue.index_select(0, extra_ids.to(torch.int64))
        return out

    def train_step(self, batch, **kw):
        out = super().train_step(batch, **kw)
        self._catalogue_stale = True
        return out

    def forward(self, batch):
        out = super().forward(batch)
        if out.requires_grad:
            self._catalogue_stale = True            # an optimizer step follows
        return out

    def _engine_args(self, batch, dev):
        if (batch.get("neighbor_rows") if hasattr(batch, "get") else None) is None:
            if self._graph is not None:
                return super()._engine_args(self._global_neighbors(batch, dev), dev)
            # a loader that knows no graph (data_handler.MyDataset): sample the neighbours from the click graph induced on this batch
            from ..graph_sampler import induced_neighbor_rows
            self._sampled = getattr(self, "_sampled", 0) + 1
            cpu = lambda v: torch.as_tensor(v).cpu().numpy()
            batch = dict(batch)
            batch["neighbor_rows"] = induced_neighbor_rows(cpu(batch["browsed_titles"]), cpu(batch["browsed_mask"]), cpu(batch["candidate_titles"]),
                                                           int(getattr(self.config, "graph_neighbors", 8)), seed=self._sampled)
        return super()._engine_args(batch, dev)
