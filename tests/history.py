"""A long-lived model against a fresh twin (tests/test_hip_history.py on the GPU, tests/test_history_host.py for the inputs).

Every other GPU test builds a model, makes one call and throws it away, so every buffer the Python engines hand to the library is
a first allocation of exactly the needed size.  A real run keeps ONE engine alive: `_buf` never shrinks a buffer, keys are shared
between tags, caches and counters carry over.  Here a SCRIPT of calls runs on one live model; before each step the model's logical
state is snapshotted (weights, Adam moments and step, the dropout call counter), afterwards the same step runs on a TWIN -- a
fresh model of the same class and config put into that state from outside -- and the two must agree bit for bit
(guarded.assert_same_bits).  Between steps every tensor of the live engine's `_bufs`, and the news-cache store's vectors, are
filled with a poison of guarded.POISONS: whatever a step reads without having written it shows up as a difference.

Never poisoned: anything between a training forward and its backward (the saved activations and the fp16 forward's token lists
are the backward's input, include/nrms_hip.h NRMS_FLAG_FWD_SCRATCH_KEPT), and anything inside an evaluation (news_cache_begin ..
news_cache_end).  KEEP lists the keys whose content is meant to survive a step boundary.

The generators at the top need numpy only, so that the host test can check the inputs without a GPU."""
from dataclasses import dataclass, field

import numpy as np

from pytorch_news_recommender_amd import synth

N_WORDS = 30000          # large enough that no word id occurs more than MAX_OCCURRENCES times in any call of the script
MAX_OCCURRENCES = 64     # the grouped embedding scatter sums longer buckets chunk by chunk (csrc/embed.hip): not bit-reproducible
N_NEWS = 300             # news ids of the evaluation batches (s7) and of the pooled step
ABST_WORDS = 17          # nrms_naml: words per abstract
TWIN = 0x100             # the twin's key in assert_same_bits' {poison: results} (no byte value)

# (B users, H history slots, C candidates, L words per title)
GEOM = {
    "s0": (6, 50, 5, 30),      # largest first: every later buffer is an oversized reuse
    "s1": (1, 50, 5, 30),      # one user; the fp16 padding-token row moves from row 9900 to row 1650
    "s2": (3, 50, 24, 30),     # eval forward: C = 24 makes the inference buffers larger than the training ones
    "s3": (5, 33, 3, 12),      # H = 33: the smallest history on the fused user-encoder kernel; short titles
    "s3p": (5, 33, 3, 12),     # the pooled loss at the same geometry
    "s4": (4, 32, 5, 33),      # H = 32: the chain / the 32-row kernels; L = 33: the 64-row title kernels in fp16
    "s5": (6, 50, 5, 30),      # back to the first shape, in buffers that have held every other one
    "s6": (6, 50, 5, 30),      # autograd forward / interleaved inference / backward
    "s6e": (3, 50, 24, 30),    # ... the interleaved eval forward
    "s7": (5, 50, 5, 30),      # the train step between the two evaluations
    "s8": (4, 32, 5, 12),      # the padding row flips to non-zero and back
}
S6_TITLES = (40, 400)          # get_news_vector between forward and backward: smaller, then larger than the 6 * 55 training titles
S7_BATCHES = (8, 3)            # users of the two evaluation batches (H = 50, C = 24, L = 30)
S7_C = 24
_SEEDS = {name: 1000 + 17 * i for i, name in enumerate(GEOM)}

# engine._bufs keys whose content is meant to survive a step boundary: none today.  (Every key is rewritten by the call that reads
# it; `_saved` keeps views of ids / news_vec / user_vec, but a backward only ever follows its own forward inside one step.)
KEEP = ()


def titles(n, L, seed, n_words=N_WORDS):
    """n ragged titles [n, L] int64 (right-zero-padded, at least one word), for get_news_vector."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, n_words, size=(n, L), dtype=np.int64)
    ln = rng.integers(1, L + 1, size=(n,))
    return np.where(np.arange(L)[None, :] < ln[:, None], ids, 0)


def _shape(geom, n_words=N_WORDS):
    B, H, C, L = geom
    return synth.Shape(n_words=n_words, batch_size=B, history_len=H, n_candidates=C, n_words_title=L)


def add_news_ids(batch, seed):
    """candidate_ids / browsed_ids (0 = padding slot) for the pooled loss: the ids only name the slots, the titles stay random."""
    rng = np.random.default_rng(seed + 5)
    B, H = batch["browsed_mask"].shape
    Cn = batch["candidate_mask"].shape[1]
    batch["candidate_ids"] = rng.integers(1, N_NEWS, size=(B, Cn)).astype(np.int64)
    batch["browsed_ids"] = np.where(batch["browsed_mask"] != 0, rng.integers(1, N_NEWS, size=(B, H)), 0).astype(np.int64)
    return batch


def nrms_batch(step, with_ids=False):
    """The batch of one script step for the title models (nrms_hip, nrms_v1_hip)."""
    geom = GEOM[step]
    b = synth.make_batch(_shape(geom), seed=_SEEDS[step], ragged=True, min_title=1, empty_history_user=True, all_pad_title=True,
                         mask_some_candidates=geom[2] > 1)
    return add_news_ids(b, _SEEDS[step]) if with_ids else b


def hierec_batch(step, n_sub, n_top):
    geom = GEOM[step]
    return synth.make_batch_hierec(_shape(geom), n_sub=n_sub, n_top=n_top, seed=_SEEDS[step], empty_history_user=True,
                                   mask_some_candidates=geom[2] > 1)


def naml_shape(geom, base):
    B, H, C, L = geom
    from dataclasses import replace
    return replace(base, n_words=N_WORDS, batch_size=B, history_len=H, n_candidates=C, n_words_title=L, n_words_abst=ABST_WORDS)


def naml_batch(step, base):
    return synth.make_batch_naml(naml_shape(GEOM[step], base), seed=_SEEDS[step])


def bert_batch(step, base):
    from dataclasses import replace
    B, H, C, _ = GEOM[step]
    return synth.make_batch_bert(replace(base, batch_size=B, history_len=H, n_candidates=C), seed=_SEEDS[step])


def eval_set(seed=4242, L=30, H=50):
    """s7: two evaluation batches (B = 8 and B = 3, C = 24) over N_NEWS news.  Every slot carries the news id AND that news item's
    title, so that forward_cached's per-id cache is consistent with the titles; the two batches share news ids, and the same
    batches serve both evaluations, so a cache whose validity bits survive would be hit.  -> (batches, labels, catalogue)."""
    rng = np.random.default_rng(seed)
    cat = titles(N_NEWS, L, seed + 1)
    cat[0] = 0                                                    # news id 0 = the padding slot = the all-padding title
    batches, labels = [], []
    for B in S7_BATCHES:
        hist_len = rng.integers(5, H + 1, size=(B,))
        live = np.arange(H)[None, :] < hist_len[:, None]
        bids = np.where(live, rng.integers(1, N_NEWS, size=(B, H)), 0).astype(np.int64)
        cids = rng.integers(1, N_NEWS, size=(B, S7_C)).astype(np.int64)
        cmask = np.ones((B, S7_C), dtype=np.uint8)
        cmask[0, S7_C - 3:] = 0                                   # a shorter impression
        cids = np.where(cmask != 0, cids, 0)
        batches.append({"browsed_ids": bids, "candidate_ids": cids, "browsed_titles": cat[bids], "candidate_titles": cat[cids],
                        "browsed_mask": live.astype(np.uint8), "candidate_mask": cmask, "browsed_lens": hist_len.astype(np.int64)})
        for b in range(B):
            n = int(cmask[b].sum())
            y = (rng.random(n) < 0.3).astype(np.int64)
            y[0], y[1] = 1, 0
            labels.append(y.tolist())
    return batches, labels, cat


def word_id_arrays(batch):
    """The word-id arrays of one call (whatever the family): every int64 array whose name says titles / absts."""
    return [np.asarray(v) for k, v in batch.items() if k.endswith("titles") or k.endswith("absts")]


def max_word_occurrences(*arrays):
    """The largest number of times one non-padding word id occurs in the arrays of ONE call."""
    ids = np.concatenate([np.asarray(a).reshape(-1) for a in arrays])
    ids = ids[ids != 0]
    return int(np.bincount(ids).max()) if ids.size else 0


# ======================================================================================================================
# the GPU side
# ======================================================================================================================
@dataclass
class Step:
    name: str
    kind: str                  # train | pooled | eval_forward | autograd | evaluate | load
    batch: object = None       # a batch dict (numpy); `evaluate`: (batches, labels); `load`: "nonzero_pad_row" | "zero_pad_row"
    extra: dict = field(default_factory=dict)


def tb(batch):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()}


class Family:
    """What the runner needs to know about one (model family, precision): how to build a fresh model, the batches of the script,
    and the float64 oracle of a training step at the tolerance of the family's own test file."""
    name = ""
    has_pooled = True
    has_pad_flag = True            # the word table's padding row drives NRMS_FLAG_PAD_ROW_ZERO: s8 applies
    has_eval_cache = True          # train_eval.evaluate runs on this family: s7 applies
    oracle_without_dropout = False # the family's oracle cannot replay dropout: the steps held to it run with config.dropout = 0
    precision = "fp32"
    table_name = None              # state_dict key of the word-embedding table

    def fresh(self):               # a new model on the GPU, in train mode, dropout 0.2, initial weights
        raise NotImplementedError

    def batch(self, step, with_ids=False):
        raise NotImplementedError

    def eval_set(self):
        return eval_set()[:2]

    def inference(self, model):
        """s6: the inference calls between the autograd forward and its backward -> {name: tensor}."""
        raise NotImplementedError

    def oracle(self, model, state, batch, out):
        """Hold the training step that just ran on `model` (from weights `state`, results `out`) to the float64 oracle."""
        raise NotImplementedError

    def bitwise_with_dense_rows(self, model, step):
        """s8b, the table's padding row non-zero: is the step still bit-reproducible?  (nrms_hip in fp16 is not.)"""
        return True

    def extra_state(self, model):
        return None

    def set_extra_state(self, twin, extra):
        pass

    # ---- the script -------------------------------------------------------------------------------------------------
    def script(self):
        s = [Step("s0", "train", self.batch("s0")), Step("s1", "train", self.batch("s1")),
             Step("s2", "eval_forward", self.batch("s2")), Step("s3", "train", self.batch("s3"))]
        if self.has_pooled:
            s.append(Step("s3p", "pooled", self.batch("s3p", with_ids=True)))
        s += [Step("s4", "train", self.batch("s4")), Step("s5", "train", self.batch("s5")),
              Step("s6", "autograd", self.batch("s6"))]
        last = "s5"
        if self.has_eval_cache:
            ev = self.eval_set()
            s += [Step("s7a", "evaluate", ev), Step("s7b", "train", self.batch("s7")), Step("s7c", "evaluate", ev)]
            last = "s7b"
        if self.has_pad_flag:
            s += [Step("s8a", "load", "nonzero_pad_row"), Step("s8b", "train", self.batch("s8"), extra=dict(pad_row=False)),
                  Step("s8c", "load", "zero_pad_row"), Step("s8d", "train", self.batch("s8"), extra=dict(pad_row=True))]
            last = "s8d"
        for st in s:
            st.extra["oracle"] = st.name == last          # the last training step of the script: non-vacuity
            atomic = self.precision == "fp16" and st.extra.get("pad_row") is False
            if self.oracle_without_dropout and (st.extra["oracle"] or atomic):
                st.extra["dropout"] = 0.0
        return s

    def before_step(self, model, step):
        """On the live model, before the step's snapshot."""


def eval_forwards(model, batch):
    """The eval forward on the distinct titles of the batch (model.dedup_inference, the default) and on every slot: only the
    second goes through the engine's forward(training=False), whose buffers differ from the training ones by a suffix alone."""
    out = {}
    for dedup in (True, False):
        model.dedup_inference = dedup
        out["scores_dedup_%s" % dedup] = model(tb(batch))
    model.dedup_inference = True
    return out


def bits(t):
    import torch
    return t.detach().contiguous().view(-1).view(torch.uint8)


def compare(live, twin, what, poison):
    """{name: tensor} of the live model against the twin's, bit for bit.  Large tensors (the flat parameter / moment buffers) are
    compared on the device and only brought to the host, for assert_same_bits' report, when they differ."""
    import torch
    from tests.guarded import assert_same_bits
    assert live.keys() == twin.keys(), (what, sorted(live), sorted(twin))
    what = "%s [live model, buffers poisoned 0x%02X, against its twin = 0x%X]" % (what, poison, TWIN)
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    small = [k for k, v in live.items() if not isinstance(v, torch.Tensor) or v.numel() <= 1 << 16]
    assert_same_bits({poison: {k: host(live[k]) for k in small}, TWIN: {k: host(twin[k]) for k in small}}, what)
    for k in live:
        if k in small:
            continue
        a, b = live[k], twin[k]
        if a.shape != b.shape or a.dtype != b.dtype or not torch.equal(bits(a), bits(b)):
            assert_same_bits({poison: {k: host(a)}, TWIN: {k: host(b)}}, what)
            raise AssertionError("%s: %s differs in shape or dtype" % (what, k))


def snapshot(fam, model):
    st = dict(sd={k: v.detach().clone() for k, v in model.state_dict().items()}, calls=model._calls, opt=None,
              extra=fam.extra_state(model))
    if model._opt is not None:
        st["opt"] = dict(step=model._opt["step"], m=model._opt["m"].clone(), v=model._opt["v"].clone())
    return st


def make_twin(fam, st):
    """A fresh model of the same class and config in the logical state `st`."""
    import torch
    twin = fam.fresh()
    twin.load_state_dict({k: v.clone() for k, v in st["sd"].items()})
    twin.engine                                  # flat buffer + engine: _opt below must be laid out like _flat
    if st["opt"] is not None:
        twin._opt = dict(step=st["opt"]["step"], g=torch.zeros_like(twin._flat), m=st["opt"]["m"].clone(), v=st["opt"]["v"].clone())
        assert twin._opt["m"].shape == twin._flat.shape
    twin._calls = st["calls"]
    fam.set_extra_state(twin, st["extra"])
    return twin


def poison_engine(model, byte):
    """Every tensor of the engine's _bufs (bar KEEP) and the news-cache store's vectors <- byte."""
    eng = model._engine
    assert getattr(eng, "_news_cache", None) is None, "never poison inside an evaluation"
    n = 0
    for key, t in eng._bufs.items():
        if key in KEEP:
            continue
        bits(t).fill_(byte)
        n += 1
    for store in (getattr(eng, "_news_cache_store", None),):
        if store is not None:
            bits(store[0]).fill_(byte)
            n += 1
    return n


def run_step(fam, model, step, live):
    """One script step on `model` -> {name: tensor or array} of what the step produced.  live: the long-lived model (it gets the
    interleaved inference calls of s6 between forward and backward; the twin runs them after its backward)."""
    import torch
    from pytorch_news_recommender_amd import train_eval
    out = {}
    if step.kind in ("train", "pooled"):
        model.train()
        model.config.train_loss = "pooled" if step.kind == "pooled" else "rowwise"
        before = model._opt["step"] if model._opt is not None else 0
        p_drop = model.config.dropout
        model.config.dropout = step.extra.get("dropout", p_drop)
        model.engine                                 # (the flat buffer exists from here on)
        flat0 = model._flat.clone()
        loss = model.train_step(tb(step.batch))
        model.config.train_loss, model.config.dropout = "rowwise", p_drop
        st = model._opt
        out = dict(scores=model._last_scores, loss=loss, flat=model._flat, g=st["g"], m=st["m"], v=st["v"])
        # two models that agree because both returned early must still fail
        assert st["step"] == before + 1, step.name
        assert bool(torch.isfinite(loss).all()) and float(loss) > 0.0, (step.name, float(loss))
        assert not torch.equal(flat0, model._flat), "%s: the step moved no parameter" % step.name
        assert bool((st["g"] != 0).any()), "%s: the gradient is all zeros" % step.name
    elif step.kind == "eval_forward":
        model.eval()
        with torch.no_grad():
            out = eval_forwards(model, step.batch)
        model.train()
        assert bool(torch.isfinite(out["scores_dedup_False"]).all())
    elif step.kind == "autograd":
        model.train()
        model.zero_grad(set_to_none=True)
        scores = model(tb(step.batch))
        if live:
            inf = fam.inference(model)
        loss = torch.nn.functional.cross_entropy(scores, torch.zeros(len(scores), dtype=torch.long, device=scores.device))
        loss.backward()
        if not live:
            inf = fam.inference(model)
        out = dict(scores=scores.detach(), loss=loss.detach())
        for n, p in model.named_parameters():
            assert p.grad is not None, n
            out["grad/" + n] = p.grad
        out.update({"inference/" + k: v for k, v in inf.items()})
        assert any(bool((p.grad != 0).any()) for p in model.parameters())
    elif step.kind == "evaluate":
        batches, labels = step.batch
        auc = train_eval.evaluate(model.config, model, [tb(b) for b in batches], labels, verbose=False)
        assert model.training
        out = dict(last_eval_scores=model.last_eval_scores, last_eval_aucs=model.last_eval_aucs, auc=np.float64(auc))
        assert model.last_eval_scores.shape == (sum(len(b["candidate_mask"]) for b in batches), batches[0]["candidate_mask"].shape[1])
    else:
        raise ValueError(step.kind)
    torch.cuda.synchronize()
    return out


def load_step(fam, model, step, st, zero_state):
    """s8: load weights into the LIVE model.  nonzero_pad_row: the current weights with a non-zero padding row of the word table
    (the pad-row flag must drop); zero_pad_row: the weights the model had before s8 (the flag must come back)."""
    import torch
    if step.batch == "nonzero_pad_row":
        sd = {k: v.clone() for k, v in st["sd"].items()}
        g = torch.Generator().manual_seed(7)
        sd[fam.table_name][0] = (0.3 * torch.randn(sd[fam.table_name].shape[1], generator=g)).to(sd[fam.table_name].device)
    else:
        sd = {k: v.clone() for k, v in zero_state["sd"].items()}
    model.load_state_dict(sd)


def run_script(fam, poison, report=None):
    """The whole script on one live model under one poison.  report: dict that receives per-step notes (for the summary)."""
    import torch
    live = fam.fresh()
    prev_eval = None
    zero_state = None
    n_poisoned = 0
    for step in fam.script():
        fam.before_step(live, step)
        st = snapshot(fam, live)
        if step.kind == "load":
            if step.batch == "nonzero_pad_row":
                zero_state = st
            load_step(fam, live, step, st, zero_state)
            continue                                     # (no poison here either: the next step's snapshot is the loaded state)
        out = run_step(fam, live, step, live=True)
        what = "%s %s %s" % (fam.name, step.name, step.kind)
        bitwise = True
        if "pad_row" in step.extra:
            assert live._engine.pad_row_zero is step.extra["pad_row"], (what, live._engine.pad_row_zero)
            bitwise = fam.bitwise_with_dense_rows(live, step)
        twin = make_twin(fam, st)
        ref = run_step(fam, twin, step, live=False)
        if bitwise:
            compare(out, ref, what, poison)
        else:
            # the documented exception (fp16 news encoder without NRMS_FLAG_PAD_ROW_ZERO: float atomics in the table scatter):
            # the forward is still bit-reproducible, the step is held to the oracle instead
            compare({k: out[k] for k in ("scores", "loss")}, {k: ref[k] for k in ("scores", "loss")}, what, poison)
            fam.oracle(live, st, step.batch, out)
        if step.extra.get("oracle") and bitwise:
            fam.oracle(live, st, step.batch, out)
        if step.kind == "evaluate":
            scores = out["last_eval_scores"].clone()
            if prev_eval is not None:
                # the weights moved in between: the second evaluation must not return the first one's scores
                assert not torch.equal(scores, prev_eval), "%s: the second evaluation returned the first one's scores" % what
            prev_eval = scores
        assert live._engine.loss_scale_backoff == 0, what       # no poison may reach a gradient (and overflow it)
        del twin, ref, out
        n_poisoned += poison_engine(live, poison)
    assert n_poisoned > 0
    live._engine.check_ids()
    return live


# ======================================================================================================================
# families
# ======================================================================================================================
def _np_state(st):
    return {k: v.detach().cpu().numpy() for k, v in st["sd"].items()}


def _grads_of(model, out):
    return {n: model._layout.view(out["g"], n).detach().cpu().numpy() for n in model._names}


class NrmsFamily(Family):
    """nrms_hip.  Oracle and bars: tests/test_hip_parity.py (fp32, bf16x3), tests/test_hip_fp16.py (fp16)."""
    table_name = "news_encoder.word_embedding.0.weight"

    def __init__(self, precision, d=60, heads=6, q=32, fp16_user=False):
        self.precision, self.fp16_user = precision, fp16_user
        self.shape = synth.Shape(n_words=N_WORDS, word_embed_size=d, num_attention_heads=heads, query_vector_dim=q)
        self.name = "nrms_hip d=%d %s%s" % (d, precision, " fp16_user_encoder" if fp16_user else "")
        self._params = None

    def params(self):
        if self._params is None:
            self._params = synth.make_params(self.shape, seed=3)
        return self._params

    def fresh(self):
        from tests.test_hip_parity import make_model
        # fp16_inference False, the product default: the fp16 mode evaluates in bf16x3
        return make_model(self.shape, self.params(), dropout=0.2, precision=self.precision, fp16_user=self.fp16_user,
                          fp16_inference=False).train()

    def batch(self, step, with_ids=False):
        return nrms_batch(step, with_ids)

    def inference(self, model):
        import torch
        out = {}
        model.eval()
        with torch.no_grad():
            for n in S6_TITLES:
                out["news_vec_%d" % n] = model.get_news_vector(torch.from_numpy(titles(n, GEOM["s6"][3], 77 + n)))
            out.update(eval_forwards(model, self.batch("s6e")))
        model.train()
        return out

    def bitwise_with_dense_rows(self, model, step):
        """False where the step's table scatter runs on float atomics: the fp16 news encoder without NRMS_FLAG_PAD_ROW_ZERO."""
        from pytorch_news_recommender_amd import _lib
        eng = model._engine
        B, H, C, L = GEOM["s8"]
        fp16 = eng._desc("news_encoder", B * (H + C), L, training=True).precision == _lib.NRMS_PRECISION_FP16
        return eng.pad_row_zero or not fp16

    # ---- oracle -------------------------------------------------------------------------------------------------------
    V1 = False

    def _keep(self, model, batch):
        import torch
        from pytorch_news_recommender_amd import _lib
        eng, sv = model._engine, model._engine._saved
        B, H, L = batch["browsed_titles"].shape
        n_titles = B * (H + batch["candidate_titles"].shape[1])
        d, h = self.shape.word_embed_size, eng.dims.heads("news_encoder")
        assert sv["p"] == 0.2 and sv["B"] == B and sv["L"] == L
        fp16 = eng._desc("news_encoder", n_titles, L, sv["p_embed"], sv["p"], sv["seed"], training=True).precision == _lib.NRMS_PRECISION_FP16
        keep = {}
        if not self.V1:
            keep["embed"] = eng.dropout_keep_mask(sv["seed"], 0, n_titles * L, 0.2).cpu().view(n_titles, L, d)
        if fp16:
            kc = eng.dropout_keep_mask(sv["seed"], 1, n_titles * L, 0.2, fp16_ctx=True).cpu().numpy()
            if self.V1:
                kc = kc.reshape(-1, 10, 32)[:, :, :d // 10].reshape(n_titles, L, d).copy()
            else:
                from tests.test_hip_fp16 import _padded_to_model_cols
                kc = _padded_to_model_cols(kc, h, d // h).reshape(n_titles, L, d)
            keep["ctx"] = torch.from_numpy(np.ascontiguousarray(kc))
        else:
            keep["ctx"] = eng.dropout_keep_mask(sv["seed"], 1, n_titles * L, 0.2).cpu().view(n_titles, L, d)
        return keep, fp16

    def oracle(self, model, st, batch, out):
        import torch
        from oracle import nrms_oracle as orc
        params = _np_state(st)
        keep, fp16 = self._keep(model, batch)
        o_scores, o_loss, o_grads, aux = orc.loss_and_grads(params, batch, self.shape.num_attention_heads, dtype=torch.float64,
                                                            p_drop=0.2, keep=keep)
        scores = out["scores"].detach().cpu().numpy()
        loss = float(out["loss"]) / scores.shape[0]
        grads = _grads_of(model, out)
        valid = batch["candidate_mask"] == 1
        err = float(np.abs(scores - o_scores)[valid].max())
        print("%s: last step against the float64 oracle: max |score| err %.3e, |loss| err %.3e" % (self.name, err, abs(loss - o_loss)))
        if self.precision == "fp16":
            from tests.test_hip_fp16 import _grad_report, score_bar, score_terms
            assert err < score_bar(o_scores[valid], self.fp16_user, score_terms(aux, valid)), err
            _grad_report(grads, o_grads, synth.param_names(), self.name)
        else:
            from tests.test_hip_parity import TOL, assert_grad_close
            assert err <= TOL[self.precision]["score"], err
            assert abs(loss - o_loss) < TOL[self.precision]["score"]
            for n in synth.param_names():
                assert_grad_close(grads[n], o_grads[n], self.precision, n)
        assert not grads[self.table_name][0].any()


class V1Family(NrmsFamily):
    """nrms_v1_hip at the widths of test_hip_v1_fp16's small shape (dk50_h4).  Oracle and bars: tests/test_hip_v1.py (bf16x3),
    tests/test_hip_v1_fp16.py (fp16 with config.fp16_v1_news_encoder).  s4 (L = 33) is outside the fused fp16 v1 kernels
    (seq_len <= 32): the news encoder reroutes to bf16x3 for that step and comes back."""
    table_name = "news_encoder.word_embedding.weight"
    V1 = True
    TITLE_HEADS = 4

    def __init__(self, precision):
        self.precision, self.fp16_user = precision, False
        self.shape = synth.Shape(n_words=N_WORDS, word_embed_size=200, num_attention_heads=4, query_vector_dim=100)
        self.name = "nrms_v1_hip %s" % precision
        self._params = None

    def params(self):
        if self._params is None:
            self._params = synth.make_params_v1(self.shape, seed=3)
        return self._params

    def fresh(self):
        from tests.test_hip_v1 import make_v1
        return make_v1(self.shape, self.params(), self.TITLE_HEADS, dropout=0.2, precision=self.precision,
                       fp16_news=self.precision == "fp16", fp16_inference=False).train()

    def oracle(self, model, st, batch, out):
        import torch
        from oracle import nrms_oracle as orc
        params = _np_state(st)
        keep, fp16 = self._keep(model, batch)
        v0 = orc.v1_to_v0_names(params)
        o_scores, o_loss, o_grads, _ = orc.loss_and_grads(v0, batch, self.shape.num_attention_heads, dtype=torch.float64, p_drop=0.2,
                                                          keep=keep, news_heads=self.TITLE_HEADS, embed_dropout=False)
        back = {v: k for k, v in zip(params.keys(), v0.keys())}
        scores = out["scores"].detach().cpu().numpy()
        grads = _grads_of(model, out)
        valid = batch["candidate_mask"] == 1
        err = float(np.abs(scores - o_scores)[valid].max())
        print("%s: last step against the float64 oracle: max |score| err %.3e (news encoder fp16: %s)" % (self.name, err, fp16))
        if fp16:
            from tests.test_hip_v1_fp16 import _v1_grad_report, v1_bar
            assert err < v1_bar(o_scores[valid]), err
            _v1_grad_report(grads, o_grads, back, self.name)
        else:
            from tests.test_hip_parity import TOL, assert_grad_close
            assert err <= TOL["bf16x3"]["score"], err
            for v0name, g in o_grads.items():
                assert_grad_close(grads[back[v0name]], g, "bf16x3", v0name)
        assert not grads[self.table_name][0].any()


class NamlFamily(Family):
    """nrms_naml_hip (abstracts of ABST_WORDS words; attention-probability dropout; the partition of empty sequences changes with
    every batch).  Oracle and bars: tests/test_hip_naml.py.  The model has no get_news_vector: s6 interleaves encode_catalogue over
    40 and 400 news (titles, abstracts, categories) and an eval forward instead.  Its evaluation does not cache news vectors by
    id, so s7 checks the inference buffers only."""
    table_name = "news_encoder.word_embedding.weight"
    BASE = synth.NamlShape(n_words=N_WORDS, word_embed_size=96, title_heads_num=6, query_vector_dim=40, category_nums=7,
                           subcategory_nums=11, cate_embed_size=32, user_heads_num=8, query_vector_dim_large=72,
                           n_words_abst=ABST_WORDS)

    def __init__(self, precision):
        self.precision = precision
        self.name = "nrms_naml_hip %s" % precision
        self._params = None

    def fresh(self):
        from tests.test_hip_naml import make_model
        if self._params is None:
            self._params = synth.make_params_naml(self.BASE, seed=3)
        return make_model(self.BASE, self._params, dropout=0.2, precision=self.precision).train()

    def batch(self, step, with_ids=False):
        b = naml_batch(step, self.BASE)
        return add_news_ids(b, _SEEDS[step]) if with_ids else b

    def news(self, n, seed):
        """n news items: titles, abstracts, category and sub-category ids."""
        rng = np.random.default_rng(seed)
        s = self.BASE
        return (titles(n, GEOM["s6"][3], seed + 1), titles(n, ABST_WORDS, seed + 2), rng.integers(1, s.category_nums, size=(n,)),
                rng.integers(1, s.subcategory_nums, size=(n,)))

    def eval_set(self):
        batches, labels, cat = eval_set()
        _, absts, categ, sub = self.news(N_NEWS, 99)
        absts[0], categ[0], sub[0] = 0, 0, 0
        for b in batches:
            for side, ids in (("browsed", b["browsed_ids"]), ("candidate", b["candidate_ids"])):
                b[side + "_absts"], b[side + "_categ_ids"], b[side + "_subcateg_ids"] = absts[ids], categ[ids], sub[ids]
        return batches, labels

    def inference(self, model):
        import torch
        out = {}
        model.eval()
        with torch.no_grad():
            for n in S6_TITLES:
                out["catalogue_%d" % n] = model.encode_catalogue(*[torch.from_numpy(np.ascontiguousarray(a)) for a in self.news(n, 77 + n)])
            out.update(eval_forwards(model, self.batch("s6e")))
        model.train()
        return out

    def oracle(self, model, st, batch, out):
        import torch
        from oracle import naml_oracle as nml
        from tests.test_hip_naml import TOL, close, naml_keep_masks
        B, H, L = batch["browsed_titles"].shape
        shape = naml_shape((B, H, batch["candidate_titles"].shape[1], L), self.BASE)
        sv = model._engine._saved
        assert sv["p"] == 0.2 and sv["B"] == B
        keep = naml_keep_masks(model, shape, batch, sv["seed"], 0.2)
        params = _np_state(st)
        o_scores, o_loss, o_grads = nml.loss_and_grads(params, batch, shape.title_heads_num, shape.user_heads_num, dtype=torch.float64,
                                                       p_drop=0.2, keep=keep)
        t = TOL[self.precision]
        scores = out["scores"].detach().cpu().numpy()
        live = batch["candidate_mask"] != 0
        err = float(np.abs(scores - o_scores)[live].max())
        print("%s: last step against the float64 oracle: max |score| err %.3e" % (self.name, err))
        assert err <= t["score"], err
        assert abs(float(out["loss"]) / B - o_loss) < t["score"]
        grads = _grads_of(model, out)
        for n in params:
            close(grads[n], o_grads[n], t, n)


class BertFamily(Family):
    """nrms_bert_hip (news ids in place of titles: no L).  Oracle and bars: tests/test_hip_nrms_bert.py (its float64 restatement).
    No get_news_vector: s6 interleaves encode_catalogue and an eval forward.  No word table, hence no pad-row flag: s8 is left out.
    s7 runs on the bert engine's own cache (`news_cache_rows`, a _bufs entry, poisoned like the others)."""
    has_pad_flag = False
    table_name = "news_encoder.news_embedding.weight"
    BASE = synth.BertShape(n_news=N_NEWS, bert_embed_size=64, user_heads_num=8, query_vector_dim_large=16)

    def __init__(self, precision):
        self.precision = precision
        self.name = "nrms_bert_hip %s" % precision
        self._params = None

    def fresh(self):
        from tests.test_hip_nrms_bert import make_model
        if self._params is None:
            self._params = synth.make_params_bert(self.BASE, seed=3)
        return make_model(self.BASE, self._params, dropout=0.2, precision=self.precision).train()

    def batch(self, step, with_ids=False):
        return bert_batch(step, self.BASE)

    def eval_set(self):
        batches, labels, _ = eval_set()
        keys = ("browsed_ids", "candidate_ids", "browsed_mask", "candidate_mask", "browsed_lens")
        return [{k: b[k] for k in keys} for b in batches], labels

    def inference(self, model):
        import torch
        model.eval()
        with torch.no_grad():
            out = {"catalogue": model.encode_catalogue()}
            out.update(eval_forwards(model, self.batch("s6e")))
        model.train()
        return out

    def oracle(self, model, st, batch, out):
        from pytorch_news_recommender_amd import _lib
        from pytorch_news_recommender_amd.bert_engine import USER_SEED_SALT
        from tests.test_hip_nrms_bert import TOL, close, restate_grads
        eng, s = model._engine, self.BASE
        sv = eng._saved
        B, H = batch["browsed_ids"].shape
        Cn, E, h, p = batch["candidate_ids"].shape[1], s.bert_embed_size, s.user_heads_num, 0.2
        assert sv["p"] == p and sv["B"] == B
        N = B * (H + Cn)
        keep_nv = eng.dropout_keep_mask(sv["seed"], _lib.NRMS_DROPOUT_SITE_NEWSVEC, N, p, d=E)
        assert (B * h * H * H) % 4 == 0
        keep_attn = eng.dropout_keep_mask(sv["seed"] ^ USER_SEED_SALT, 2, B * h * H * H // 4, p, d=4).view(B, h, H, H)
        params = _np_state(st)
        o_scores, o_loss, o_grads = restate_grads(params, batch, h, keep_nv=keep_nv, keep_attn=keep_attn, p=p)
        t = TOL[self.precision]
        scores = out["scores"].detach().cpu().numpy()
        live = batch["candidate_mask"] != 0
        err = float(np.abs(scores - o_scores)[live].max())
        print("%s: last step against the float64 restatement: max |score| err %.3e" % (self.name, err))
        assert err <= t["score"], err
        assert abs(float(out["loss"]) / B - o_loss) < t["score"]
        grads = _grads_of(model, out)
        for n in params:
            close(grads[n], o_grads[n], t, n)


class HieRecFamily(NrmsFamily):
    """hierec_hip.  Oracle: oracle/segpool_oracle.py, bars: tests/test_hip_hierec.py.  The model refuses the pooled loss (s3p is
    left out) and has no get_news_vector: s6 interleaves encode_catalogue over 40 and 400 news and an eval forward.  Its oracle
    has no dropout replay, so the steps held to it (the last one; in fp16 also s8b, atomic) run with config.dropout = 0."""
    has_pooled = False
    oracle_without_dropout = True
    N_SUB, N_TOP = 23, 7

    def __init__(self, precision):
        self.precision, self.fp16_user = precision, False
        self.shape = synth.Shape(n_words=N_WORDS, word_embed_size=64, num_attention_heads=4, query_vector_dim=32)
        self.name = "hierec_hip %s" % precision
        self._params = None

    def params(self):
        if self._params is None:
            self._params = synth.make_params_hierec(self.shape, self.N_SUB, self.N_TOP, seed=3)
        return self._params

    def fresh(self):
        from tests.test_hip_hierec import make_hierec
        m = make_hierec(self.shape, self.params(), precision=self.precision, n_sub=self.N_SUB, n_top=self.N_TOP)
        m.config.dropout = 0.2
        return m.train()

    def batch(self, step, with_ids=False):
        return hierec_batch(step, self.N_SUB, self.N_TOP)

    def news(self, n, seed):
        rng = np.random.default_rng(seed)
        return titles(n, GEOM["s6"][3], seed + 1), rng.integers(1, self.N_TOP, size=(n,)), rng.integers(1, self.N_SUB, size=(n,))

    def eval_set(self):
        batches, labels, _ = eval_set()
        _, categ, sub = self.news(N_NEWS, 99)
        categ[0], sub[0] = 0, 0
        for b in batches:
            for side, ids in (("browsed", b["browsed_ids"]), ("candidate", b["candidate_ids"])):
                b[side + "_categ_ids"], b[side + "_subcateg_ids"] = categ[ids], sub[ids]
        return batches, labels

    def inference(self, model):
        import torch
        out = {}
        model.eval()
        with torch.no_grad():
            for n in S6_TITLES:
                out["catalogue_%d" % n] = model.encode_catalogue(*[torch.from_numpy(np.ascontiguousarray(a)) for a in self.news(n, 77 + n)]).vectors
            out.update(eval_forwards(model, self.batch("s6e")))
        model.train()
        return out

    def _oracle_forward(self, pt, batch, st):
        from oracle import segpool_oracle as so
        return so.hierec_forward(pt, batch, self.shape.num_attention_heads)

    def _bars(self):
        from tests.test_hip_hierec import grad_bound, score_bar
        return score_bar, grad_bound

    def oracle(self, model, st, batch, out):
        import torch
        from oracle import nrms_oracle as orc
        assert model._engine._saved["p"] == 0.0
        score_bar, grad_bound = self._bars()
        pt = orc.to_torch(_np_state(st), dtype=torch.float64, requires_grad=True)
        s = self._oracle_forward(pt, batch, st)
        loss = orc.loss_fn(s)
        loss.backward()
        o_scores = s.detach().numpy()
        scores = out["scores"].detach().cpu().numpy()
        live = batch["candidate_mask"] != 0
        err, scale = float(np.abs(scores - o_scores)[live].max()), float(np.abs(o_scores[live]).max())
        fp16 = self.precision == "fp16"
        print("%s: last step against the float64 oracle: max |score| err %.3e (scale %.2f)" % (self.name, err, scale))
        assert err <= score_bar(fp16, scale), err
        assert abs(float(out["loss"]) / len(scores) - float(loss)) <= score_bar(fp16, scale)
        grads = _grads_of(model, out)
        o_grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in pt.items()}
        gscale = max(float(np.abs(g).max()) for k, g in o_grads.items() if not k.endswith("word_embedding.0.weight"))
        for n, ref in o_grads.items():
            g = grads[n]
            if n.endswith("_embedding.weight"):
                ref, g = ref.copy(), g.copy()         # F.embedding-free oracle: row 0 (padding_idx) takes no gradient in the model
                ref[0], g[0] = 0, 0
            bad = float((np.abs(g - ref) - grad_bound(ref, fp16, gscale)).max())
            assert bad <= 0.0, (self.name, n, float(np.abs(g - ref).max()), float(np.abs(ref).max()))


class GraphFamily(HieRecFamily):
    """graph_hip with an attached click graph over N_NEWS news (the sampler's seed is the train-step counter `_graph_step`, the
    out-of-batch neighbour vectors come from `_catalogue`, which may be stale on purpose: both travel to the twin; the twin calls
    refresh_neighbor_vectors() only where the live model's catalogue is current).  Oracle and bars:
    tests/test_hip_graph_sampler.py.  No pooled loss (s3p left out), no get_news_vector: s6 interleaves encode_catalogue over 40
    and 400 titles and an eval forward.  The oracle has no dropout replay and encodes the out-of-batch constants with the
    current weights: the steps held to it run with config.dropout = 0 on a freshly encoded catalogue."""
    K, CAP = 8, 256

    def __init__(self, precision):
        self.precision, self.fp16_user = precision, False
        self.shape = synth.Shape(n_words=N_WORDS, word_embed_size=64, num_attention_heads=4, query_vector_dim=32)
        self.name = "graph_hip %s" % precision
        self._params = self._graph = None
        self.titles = eval_set()[2]

    def params(self):
        if self._params is None:
            self._params = synth.make_params_graph(self.shape, seed=3)
        return self._params

    def graph(self):
        if self._graph is None:
            from tests.test_hip_graph_sampler import build, zipf_histories
            self._graph = build(zipf_histories(60, 50, N_NEWS, 11, zipf=0.9, min_len=2), N_NEWS)
        return self._graph

    def fresh(self):
        import torch
        from tests.test_hip_graph_sampler import make_graph_model
        m = make_graph_model(self.shape, self.params(), self.K, self.precision, self.CAP)
        m.config.dropout = 0.2
        m.attach_click_graph(self.graph(), torch.from_numpy(self.titles))
        return m.train()

    def batch(self, step, with_ids=False):
        return nrms_batch(step, with_ids=True)

    def eval_set(self):
        return eval_set()[:2]

    def inference(self, model):
        import torch
        out = {}
        model.eval()
        with torch.no_grad():
            for n in S6_TITLES:
                out["catalogue_%d" % n] = model.encode_catalogue(torch.from_numpy(titles(n, GEOM["s6"][3], 77 + n)))
            out.update(eval_forwards(model, self.batch("s6e")))
        model.train()
        return out

    def before_step(self, model, step):
        if "dropout" in step.extra:               # an oracle step: the oracle's constants are encoded with the current weights
            model.refresh_neighbor_vectors()

    def extra_state(self, model):
        return dict(step=model._graph_step, stale=model._catalogue_stale, catalogue=model._catalogue.clone())

    def set_extra_state(self, twin, extra):
        twin._graph_step = extra["step"]
        if extra["stale"]:
            twin._catalogue, twin._catalogue_stale = extra["catalogue"].clone(), True
        else:
            twin.refresh_neighbor_vectors()

    def _oracle_forward(self, pt, batch, st):
        from tests.test_hip_graph_sampler import expected_neighbors, oracle_scores
        assert not st["extra"]["stale"]
        rows, extra_ids, n_extra, dropped = expected_neighbors(self.graph(), batch, self.K, st["extra"]["step"], self.CAP, N_NEWS)
        assert dropped == 0 and n_extra >= 1
        return oracle_scores(pt, batch, self.titles, rows, extra_ids, n_extra, self.shape.num_attention_heads)

    def _bars(self):
        from tests.test_hip_graph_sampler import grad_bound, score_bar
        return score_bar, grad_bound
