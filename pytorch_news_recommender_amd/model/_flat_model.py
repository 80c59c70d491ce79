"""Shared host plumbing of every HIP model (nrms_v0 / nrms_v1 / nrms_naml, and the row f-4 models of SURVEY section 8 that have
no counterpart in the reference, model/hierec_hip.py, model/graph_hip.py): parameters as views of one flat fp32 buffer (one
Adam launch, one gradient all-reduce), one autograd node around the engine, the fused training step, and the reference's plugin
contract -- ``Model(config)``, ``forward(batch_dict) -> FloatTensor[B, C]`` (model/__init__.py:22-23,38) -- around an engine
with ``forward(flat, *args, training, p_drop, seed)`` / ``backward(flat, gflat, dscores, gen, table_grad_ready)``.
No CPU fallback."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .. import _lib
from ..engine import nrms_entries


def news_encoder_entries(dims, extra):
    """Layout entries of a row f-4 model: the NRMS news encoder's ten tensors (nrms_v0 names, table first, W_Q | W_K | W_V
    adjacent as the kernels need), then the model's own tensors in the order given: extra = [(name, shape), ...]."""
    return [e for e in nrms_entries(dims) if e[2] == "news_encoder"] + [(name, shape, None, None) for name, shape in extra]


def additive_entries(prefix, q, d):
    return [(prefix + ".linear.weight", (q, d)), (prefix + ".linear.bias", (q,)), (prefix + ".attention_query_vector", (q,))]


class _FlatFunction(torch.autograd.Function):
    """scores = model(batch; params) with the backward in HIP (autograd sees one node)."""

    @staticmethod
    def forward(ctx, model, args, p_drop, seed, *params):
        ctx.model = model
        scores = model._engine.forward(model._flat, *args, training=True, p_drop=p_drop, seed=seed)
        ctx.gen = model._engine._saved["gen"]
        return scores

    @staticmethod
    def backward(ctx, dscores):
        model = ctx.model
        # Default: a fresh flat gradient buffer per backward -- autograd adopts the returned views as .grad, and a tensor
        # the caller kept from an earlier step (a saved p.grad, a hook's argument) must keep its values, as torch guarantees.
        # model.reuse_grad_buffer = True (set by train_eval.train for the reference's loop, which zeroes the gradients
        # before every backward, train_eval.py:115, and keeps nothing) opts into ONE persistent buffer instead;
        # even then a fresh buffer is used while gradients are being accumulated (.grad still set).
        reuse = bool(getattr(model, "reuse_grad_buffer", False)) and not any(p.grad is not None for p in model.parameters())
        gflat = model._autograd_grad if reuse else None
        if gflat is None or gflat.shape != model._flat.shape or gflat.device != model._flat.device:
            gflat = torch.empty_like(model._flat)
            if reuse:
                model._autograd_grad = gflat
        gflat.zero_()
        model._backward(gflat, dscores, gen=ctx.gen)
        if model._engine.precision == "fp16":
            # the caller's own optimizer follows (torch.optim.Adam, train_eval.py:127): inf / nan elements of an overflowing
            # fp16 backward become 0 and are counted; the engine lowers its loss scale when the count reaches the host
            model._engine.grad_guard(gflat)
            model._engine.note_grad_check()
        return (None, None, None, None) + tuple(model._layout.view(gflat, n) for n in model._names)


class FlatHipModel(nn.Module):
    """Subclasses create their nn.Parameters, then call ``_finish(layout, device)``.  They provide ``_make_engine(device,
    precision)`` and, where the defaults do not fit, ``_engine_args(batch, dev)`` (the batch dict -> the engine's forward
    arguments; default: the ``KEYS`` tensors as one dict, those in ``OPTIONAL`` may be absent), ``_infer(batch, args, p_drop,
    seed)`` (a forward without autograd) and ``_zero_frozen_rows(gflat)`` (padding_idx rows outside the word table)."""
    KEYS = ()
    OPTIONAL = ("candidate_mask",)

    def _finish(self, layout, device):
        self._layout = layout
        self._names = layout.names
        named = dict(self.named_parameters())
        assert sorted(named) == sorted(self._names), sorted(set(named) ^ set(self._names))
        self._flat = self._engine = self._opt = None
        self._pad_zero = None
        self._calls = self._prepare_calls = 0
        self._autograd_grad = None
        self.reuse_grad_buffer = False      # autograd path: see _FlatFunction.backward
        self._flatten(device)
        # a load through ANY parent (the dispatch wrapper of model/__init__.py included) may change the embedding
        # table: nn.Module.load_state_dict recurses via _load_from_state_dict and never calls a child's
        # load_state_dict, so the reset lives in a post-hook, which fires on recursive loads too
        self.register_load_state_dict_post_hook(FlatHipModel._reset_pad_flag)

    # ---- flat parameter storage ----------------------------------------------------------
    def _flatten(self, device):
        """(Re)build the flat parameter buffer on `device` and point every Parameter at its slice."""
        named = dict(self.named_parameters())
        flat = torch.empty(self._layout.total, dtype=torch.float32, device=device)
        for n in self._names:
            v = self._layout.view(flat, n)
            v.copy_(named[n].data)
            named[n].data = v
        self._flat, self._opt, self._pad_zero = flat, None, None

    @staticmethod
    def _reset_pad_flag(module, incompatible_keys):
        module._pad_zero = None                    # the embedding table may have changed

    def refresh_pad_row_flag(self):
        """Re-evaluate NRMS_FLAG_PAD_ROW_ZERO (include/nrms_hip.h) after writing into the embedding table by
        hand.  Training never needs it: row 0 has an identically zero gradient (padding_idx), so Adam leaves
        it where it was when the weights were loaded."""
        self._pad_zero = None

    def _views_intact(self):
        base = self._flat.data_ptr()
        named = dict(self.named_parameters())
        for n in self._names:
            p = named[n]
            if p.data_ptr() != base + 4 * self._layout.entries[n][0] or p.device != self._flat.device:
                return False
        return True

    def _zero_frozen_rows(self, gflat):
        pass

    def _backward(self, gflat, dscores, gen=None, table_grad_ready=None, table_adam=None):
        """The engine's backward into gflat, then the frozen rows' gradients zeroed (before any all-reduce sees them).  dscores
        None: the gradient the engine's pooled_ce_loss() left for this forward.  table_adam: see _fuses_table_adam."""
        if table_adam is not None:
            self._engine.backward(self._flat, gflat, dscores, gen=gen, table_adam=table_adam)
        else:
            self._engine.backward(self._flat, gflat, dscores, gen=gen, table_grad_ready=table_grad_ready)
        self._zero_frozen_rows(gflat)

    def _fuses_table_adam(self, world_size, all_reduce):
        """The word-embedding table (the layout's first entry, 95 % of the parameters) takes its Adam step inside the news
        encoder's scatter kernel (NRMS_FLAG_TABLE_ADAM) when nothing has to happen to its gradient between the backward and the
        optimizer -- one rank, no all-reduce, no frozen rows to zero -- and the engine says that exactly one table scatter
        feeds the table in a step (engine.fuses_table_adam)."""
        fuses = getattr(self._engine, "fuses_table_adam", None)
        return (world_size == 1 and all_reduce is None and type(self)._zero_frozen_rows is FlatHipModel._zero_frozen_rows
                and fuses is not None and fuses() and self._layout.entries[self._names[0]][0] == 0)

    def _prepare(self):
        """Make sure parameters live in one flat GPU buffer (``.to(device)`` replaces tensors) and the engine is current."""
        dev = next(self.parameters()).device
        if not self._views_intact():
            self._flatten(dev)
        if self._flat.device.type != "cuda":
            raise _lib.NrmsError("%s: parameters are on %s; move the model to a GPU (there is no CPU fallback)"
                                 % (type(self).__module__, self._flat.device))
        prec = getattr(self.config, "precision", "fp32")
        if self._engine is None or self._engine.device != self._flat.device:
            self._engine = self._make_engine(self._flat.device, prec)
        elif self._engine.precision != prec:
            self._engine.set_precision(prec)
        self._prepare_calls += 1
        if self._pad_zero is None or self._prepare_calls % 256 == 0:
            # one host sync per weight load (and a cheap re-validation every 256 calls, should somebody write
            # into the table by hand without refresh_pad_row_flag()): is the padding row all zeros?
            self._pad_zero = bool((self._layout.view(self._flat, self._names[0])[0] == 0).all().item())
        self._engine.fp16_user_encoder = bool(getattr(self.config, "fp16_user_encoder", False))
        self._engine.fp16_inference = bool(getattr(self.config, "fp16_inference", False))
        self._engine.fp16_wide_heads = bool(getattr(self.config, "fp16_v1_news_encoder", False))
        self._engine.pad_row_zero = self._pad_zero and bool(getattr(self.config, "skip_padding_tokens", True))
        return self._flat.device

    def _next_seed(self):
        self._calls += 1
        # (_rank_salt: set by run_v0 per data-parallel rank, so that the ranks draw different dropout masks)
        return (int(torch.initial_seed()) * 0x9E3779B97F4A7C15 + self._calls * 0xD1B54A32D192ED03
                + getattr(self, "_rank_salt", 0)) & 0xFFFFFFFFFFFFFFFF

    # ---- model hooks -----------------------------------------------------------------------
    def _engine_args(self, batch, dev):
        out = {}
        for k in self.KEYS:
            v = batch.get(k) if hasattr(batch, "get") else batch[k]
            if v is None:
                if k in self.OPTIONAL:
                    continue
                raise KeyError("%s: the batch dict lacks %r" % (type(self).__module__, k))
            out[k] = torch.as_tensor(v).to(dev, non_blocking=True)
        return (out,)

    def _infer(self, batch, args, p_drop, seed):
        return self._engine.forward(self._flat, *args, training=False, p_drop=p_drop, seed=seed)

    TRAIN_LOSSES = ("rowwise", "pooled")

    def _train_loss(self):
        """config.train_loss: "rowwise" (default; each user against the user's own C candidates) or "pooled" (each user against
        the candidates of the whole batch, engine.pooled_ce_loss)."""
        name = getattr(self.config, "train_loss", "rowwise")
        if name not in self.TRAIN_LOSSES:
            raise ValueError("config.train_loss must be one of %s (got %r)" % (self.TRAIN_LOSSES, name))
        return name

    def _pooled_loss(self, batch, grad_scale):
        """The pooled loss of the training forward just run: pool ids = the batch's ``candidate_ids`` [B, C]; a user's own history
        ``browsed_ids`` [B, H] (0 = padding; absent: nothing) is no negative for that user; ``candidate_logq`` [B, C] (log of the
        probability that a pool slot holds that news; optional, ClickFeed provides it) is subtracted from the scores unless
        config.logq_correction is False.  Leaves the gradients for _backward(dscores=None)."""
        get = batch.get if hasattr(batch, "get") else (lambda k: batch[k] if k in batch else None)
        ids = get("candidate_ids")
        if ids is None:
            raise KeyError("%s: config.train_loss = 'pooled' needs the batch key 'candidate_ids' (the news id of every candidate "
                           "slot)" % type(self).__module__)
        logq = get("candidate_logq") if getattr(self.config, "logq_correction", True) else None
        dev = self._flat.device
        bias = None if logq is None else -torch.as_tensor(logq).to(dev, torch.float32)
        return self._engine.pooled_ce_loss(ids, reject=get("browsed_ids"), col_bias=bias, grad_scale=grad_scale)

    # ---- reference API ----------------------------------------------------------------------
    def forward(self, batch):
        """batch: the collated dict of data_handler.MyDataset (CPU or GPU tensors).  Returns click logits [B, C] on the GPU."""
        dev = self._prepare()
        args = self._engine_args(batch, dev)
        p_drop = float(self.config.dropout) if self.training else 0.0
        seed = self._next_seed() if p_drop > 0 else 0
        named = dict(self.named_parameters())
        params = [named[n] for n in self._names]
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _FlatFunction.apply(self, args, p_drop, seed, *params)
        return self._infer(batch, args, p_drop, seed)

    # ---- fused training step (the build's own loop; same math as train_eval.py:111-127) -----
    def train_step(self, batch, lr=None, betas=(0.9, 0.999), eps=1e-8, world_size=1, all_reduce=None, global_batch=None):
        """forward + CE(label 0) + backward + [gradient all-reduce] + Adam, all in HIP on flat
        buffers, no host sync.  Returns the local loss SUM over the batch as a device scalar
        (divide by the batch size for the reference's mean loss).  With config.train_loss = "pooled" the loss is the in-batch
        sampled softmax over this rank's own batch (_pooled_loss) instead of the row-wise cross-entropy; the rest of the step is
        the same.

        all_reduce: callable(flat_grad_tensor) that sums gradients over data-parallel ranks
        (RCCL; parallel.GradAllReduce), or a parallel.ShardedGradSync; gradients are scaled by 1/global_batch so the
        summed result is the gradient of the mean loss over the global batch."""
        dev = self._prepare()
        eng = self._engine
        pooled = self._train_loss() == "pooled"
        args = self._engine_args(batch, dev)
        if self._opt is None:
            self._opt = dict(step=0, g=torch.zeros_like(self._flat), m=torch.zeros_like(self._flat),
                             v=torch.zeros_like(self._flat))
        st = self._opt
        p_drop = float(self.config.dropout) if self.training else 0.0
        seed = self._next_seed() if p_drop > 0 else 0
        scores = eng.forward(self._flat, *args, training=True, p_drop=p_drop, seed=seed)
        gb = scores.shape[0] * world_size if global_batch is None else global_batch
        if pooled:
            loss_sum, dscores = self._pooled_loss(batch, 1.0 / gb), None
        else:
            loss_sum, dscores = eng.ce_loss(scores, grad_scale=1.0 / gb)
        lr_ = float(self.config.learning_rate if lr is None else lr)
        if self._fuses_table_adam(world_size, all_reduce):
            # the table region of g is written by the fused kernel (every row): no zero fill, no second pass over it
            n_table = self._layout.entries[self._names[0]][2]
            st["g"][n_table:].zero_()
            self._backward(st["g"], dscores, table_adam=dict(m=st["m"], v=st["v"], step=st["step"] + 1, lr=lr_, betas=betas, eps=eps))
            st["step"] += 1
            eng.adam_step(self._flat[n_table:], st["g"][n_table:], st["m"][n_table:], st["v"][n_table:], st["step"], lr=lr_,
                          betas=betas, eps=eps, rest=True)
            if eng.precision == "fp16":
                eng.note_grad_check()
            self._last_scores = scores
            return loss_sum
        st["g"].zero_()
        overlap = not os.environ.get("NRMS_NO_OVERLAP")
        if all_reduce is not None and hasattr(all_reduce, "owned"):
            # parallel.ShardedGradSync: reduce-scatter (the table region underneath the deferred weight-gradient GEMMs),
            # Adam on the 1/world of the parameters this rank owns, all-gather of the updated parameters
            pending = []
            if overlap:
                self._backward(st["g"], dscores, table_grad_ready=lambda: pending.append(all_reduce.start(st["g"], 0)))
            else:
                self._backward(st["g"], dscores)
                pending.append(all_reduce.start(st["g"], 0))
            pending.append(all_reduce.start(st["g"], 1))
            for h in pending:
                h.wait()
            st["step"] += 1
            for lo, hi, gshard in all_reduce.owned():
                eng.adam_step(self._flat[lo:hi], gshard, st["m"][lo:hi], st["v"][lo:hi], st["step"], lr=lr_, betas=betas, eps=eps)
            if eng.precision == "fp16":
                eng.note_grad_check()
            all_reduce.gather(self._flat)
            self._last_scores = scores
            return loss_sum
        if all_reduce is not None and hasattr(all_reduce, "start") and overlap:
            # the table gradient (the layout's first entry: 95 % of the bytes at the bench shape) is reduced underneath
            # the deferred d(W_qkv) GEMM; the rest follows when the backward has been enqueued
            n_table = self._layout.entries[self._names[0]][2]
            pending = []
            self._backward(st["g"], dscores, table_grad_ready=lambda: pending.append(all_reduce.start(st["g"][:n_table])))
            all_reduce(st["g"][n_table:])
            for h in pending:
                h.wait()
        else:
            self._backward(st["g"], dscores)
            if all_reduce is not None:
                all_reduce(st["g"])
        st["step"] += 1
        eng.adam_step(self._flat, st["g"], st["m"], st["v"], st["step"], lr=lr_, betas=betas, eps=eps)
        if eng.precision == "fp16":
            eng.note_grad_check()
        self._last_scores = scores
        return loss_sum

    @property
    def engine(self):
        self._prepare()
        return self._engine
