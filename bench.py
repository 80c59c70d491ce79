#!/usr/bin/env python3
"""NRMS train-step throughput on MI355X (BASELINE.json metric: users/sec, train step,
MIND shapes hist=50 cand=5 title_len=30 d=300 V=45800, 512 users per GPU).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One step = forward + CE(label 0) + backward + [RCCL all-reduce of the flat gradient] + fused
Adam over all 14.4 M parameters, dropout 0.2 on, synthetic batch already resident in HBM.
Rank 0 prints ONE JSON line: `value` users/s over the K timed steps, `ms_per_step`, `loss`, the workload.

A plain run does only what that figure needs (set-up, 1 + 2K + W untimed steps, the K timed steps,
--dump-outputs).  With --full the line also carries: `roofline` for the dominant kernel (HIP events on
the launch stream, a separate pass over the same K steps, run before the warm-up and the timed region),
`roofline.step_frac` the whole step against the dense fp16/bf16 MFMA peak by BASELINE.md's formula,
`config.score_parity_vs_reference`, `data_parallel` (N > 1), and for N = 1 `modes` (the other precision
modes and the drop-in autograd + torch.optim.Adam loop on the same batch), `variants`, `eval_path` and
`cpu_baseline`, the oracle's reference-shaped train step timed on the host's cores (bounded sample).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from pytorch_news_recommender_amd import parallel, synth
from pytorch_news_recommender_amd.config import Config
from pytorch_news_recommender_amd.model.nrms_hip import Model

PEAK_F32_MFMA_TFLOPS = 157.3        # MI355X_MICROARCH.md: f32-input MFMA, dense
PEAK_16_MFMA_TFLOPS = 2500.0        # dense bf16 / fp16 MFMA
PEAK_HBM_GBPS = 8000.0              # HBM3E spec (6300 measured achievable)
# split-bf16 spends 3 bf16 MFMAs per fp32-equivalent MFMA step BY CONSTRUCTION: its kernels are priced against peak / 3
PEAKS = {"fp32": PEAK_F32_MFMA_TFLOPS, "bf16x3": PEAK_16_MFMA_TFLOPS / 3.0, "bf16": PEAK_16_MFMA_TFLOPS,
         "fp16": PEAK_16_MFMA_TFLOPS}
DTYPES = {"fp32": "f32", "bf16x3": "bf16x3 (split-bf16 MFMA inputs hi+lo, fp32 accumulate, fp32 storage)",
          "bf16": "bf16 (MFMA inputs), fp32 accumulate, fp32 storage",
          "fp16": "f16 (MFMA inputs and saved activations; fp32 accumulate, softmax, loss, master weights and Adam)"}
# bars asserted against the ORACLE at the bench size (tests/test_hip_fullsize.py::test_every_mode_against_the_oracle_at_full_size)
PARITY = {"fp32": "<= 1e-5 (asserted vs the oracle at this size)", "bf16x3": "<= 2e-5 (asserted vs the oracle at this size)",
          "bf16": "~3e-4 (fails 1e-4; never a default)", "fp16": "<= 1e-4 (asserted vs the oracle at this size; measured value in config)"}
FLOP_PER_USER_TRAIN = 3558309000.0  # BASELINE.md section 2 / SURVEY 8d: nrms_v0, H=50, C=5, L=30, d=300, h=10, q=200


def kernel_work(shape, B, live_frac, compact, allpad_frac, fp16_news, fp16_user=False):
    """Per kernel timer: (declared bound, algorithmic flop per step, algorithmic HBM bytes per step).
    flop = 2mnk of the contractions the kernel owns, counted on what cannot be skipped exactly:
    Q|K|V projection / d(w_qkv) / dX on the non-padding token rows, attention on the titles with a real token, the
    additive projection on every token.  bytes = every tensor the kernel must read or write once."""
    H, C, L = shape.history_len, shape.n_candidates, shape.n_words_title
    d, q, h = shape.word_embed_size, shape.query_vector_dim, shape.num_attention_heads
    Mn, Mu = B * (H + C) * L, B * H                       # token rows: news encoder, user encoder
    Nn = B * (H + C)
    ap = allpad_frac if compact else 0.0
    lf = live_frac if compact else 1.0
    att_n = Nn * (1.0 - ap) * 2.0 * 2 * L * L * d           # QK^T + PV, all heads
    att_u = B * 2.0 * 2 * H * H * d
    qkv_n, qkv_u = 2.0 * Mn * lf * d * 3 * d, 2.0 * Mu * d * 3 * d
    add_n, add_u = 2.0 * Mn * d * q, 2.0 * Mu * d * q
    dx_n = 2.0 * Mn * live_frac * d * 3 * d
    n_params = shape.n_words * d + 2 * (3 * d * d + 3 * d + q * d + 2 * q)
    live_rows = Mn * live_frac
    w = {}
    if fp16_news:
        # news encoder in the fused fp16 kernels (fp16 activations: 2 B per element, padded pitches 320 / 224)
        w["fused_fwd16"] = ("mfma", qkv_n + att_n + add_n, 2.0 * (live_rows * 320 + Mn * 320 + Mn * 224))
        # backward, kernel 1: pooling backward + d(ctx) (reads ctx16, t16; writes dZ16, d(ctx)16); kernel 2: attention backward
        # of the titles with a real token (reads x16, d(ctx)16; writes dQKV16); recomputed Q|K|V / P are not algorithmic work
        w["fused_bwd16_pool"] = ("mfma", add_n, 2.0 * (2 * Mn * 320 + 2 * Mn * 224))
        w["fused_bwd16_attn"] = ("mfma", 2.0 * att_n, 2.0 * (live_rows * 320 + Mn * (1.0 - ap) * 320 + live_rows * 960))
        w["dwqkv_bwd"] = ("mfma", qkv_n + qkv_u, 2.0 * (live_rows + Mu) * (960 + 320))
        w["dx_bwd"] = ("mfma", dx_n + qkv_u, (live_rows + Mu) * (2.0 * 960 + 4.0 * d))
        w["dwadd_bwd"] = ("mfma", add_n + add_u, 2.0 * (Mn + Mu) * (224 + 320))
        w["gather_dropout"] = ("hbm", 0.0, live_rows * (4.0 * d + 2.0 * 320))
        if fp16_user:
            # user encoder (histories of 50 rows): the 64-row variants of the same kernels
            w["fused64_fwd16"] = ("mfma", qkv_u + att_u + add_u, 2.0 * Mu * (320 + 320 + 224))
            w["fused64_bwd16_pool"] = ("mfma", add_u, 2.0 * Mu * (2 * 320 + 2 * 224))
            w["fused64_bwd16_attn"] = ("mfma", 2.0 * att_u, 2.0 * Mu * (320 + 320 + 960))
        else:
            # user encoder in bf16x3 (the default of the fp16 mode): ONE fused split-bf16 kernel per direction (csrc/user64.hip;
            # algorithmic bytes: x in, ctx / T out, the Q|K|V + context fragments out; backward: those in, ds + dQKV out) and, as
            # before, its TN / dX GEMMs on the dwqkv_bwd / dx_bwd / dwadd_bwd timers next to the news encoder's fp16 GEMMs.
            # The unfused chain's timers stay listed for engine.fused_user_encoder = False
            Mdu, Mqu = 4.0 * Mu * d, 4.0 * Mu * q
            frag = B * (h * 2 * 12 * 1024 + 2 * 20 * 2048)
            w["user64_fwd"] = ("mfma", qkv_u + att_u + add_u, 2 * Mdu + Mqu + frag)
            w["user64_bwd"] = ("mfma", add_u + 2.0 * att_u, Mqu + frag + 3 * Mdu)
            w["qkv_proj_fwd"] = ("mfma", qkv_u, 4.0 * Mdu)
            w["addattn_fwd"] = ("mfma", add_u, Mdu + Mqu)
            w["dctx_bwd"] = ("mfma", add_u, Mqu + Mdu)
            w["attn_fwd"] = ("hbm", att_u, 4 * Mdu)
            w["attn_bwd"] = ("hbm", 2.5 * att_u, 8 * Mdu)
            w["addattn_bwd_rows"] = ("hbm", 0.0, Mdu + Mqu)
    else:
        M = float(Mn + Mu)
        Md, Mq = 4.0 * M * d, 4.0 * M * q
        Ml = Mn * lf + Mu
        Md_live = 4.0 * (Mn * (1.0 - ap) + Mu) * d
        w["qkv_proj_fwd"] = ("mfma", qkv_n + qkv_u, 4.0 * Ml * d + 3 * Md)
        w["dwqkv_bwd"] = ("mfma", qkv_n + qkv_u, 16.0 * Ml * d)
        w["dx_bwd"] = ("mfma", dx_n + qkv_u, 16.0 * (Mn * live_frac + Mu) * d)
        w["addattn_fwd"] = ("mfma", add_n + add_u, Md + Mq)
        w["dctx_bwd"] = ("mfma", add_n + add_u, Mq + Md)
        w["dwadd_bwd"] = ("mfma", add_n + add_u, Mq + Md)
        w["attn_fwd"] = ("hbm", att_n + att_u, 3 * Md_live + Md)
        w["attn_bwd"] = ("hbm", 2.5 * (att_n + att_u), 3 * Md_live + Md + 12.0 * Ml * d)
        w["addattn_bwd_rows"] = ("hbm", 0.0, Md + Mq)
        w["gather_dropout"] = ("hbm", 0.0, 8.0 * Mn * d * lf)
    w["scatter_dropout"] = ("hbm", 0.0, 8.0 * Mn * d * live_frac)
    w["adam"] = ("hbm", 0.0, 28.0 * n_params)
    return w


OTHER_TIMERS = ("user64_prep", "grad_guard", "tn_reduce", "red16", "prep16", "title_order", "cast16", "split_planes", "click", "ce_loss", "transpose", "colsum",
                "permute_rows", "compact_rows", "sanitize_ids", "fill_pad_rows", "padsum")


_T0 = time.time()


def log(msg):
    print("[bench %6.1fs] %s" % (time.time() - _T0, msg), file=sys.stderr, flush=True)


def host_threads():
    """Threads for the CPU baseline: this process's CPU share (the GPU box gives one GPU's
    slice of the host, far fewer cores than os.cpu_count() reports)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    # a container's CPU quota (cgroup v2 cpu.max / v1 cfs quota) can be far below its affinity set: more threads than that
    # only fight each other
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    log("host cores: os.cpu_count %s, affinity %d, cgroup quota %s" % (os.cpu_count(), n, quota))
    if quota is not None:
        n = min(n, max(1, int(quota + 0.5)))
    return max(1, n)


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(shape, budget_s=60.0):
    """The oracle's reference-shaped train step (the op sequence of nrms_v0.py:255-260 + train_eval.py:111-127: per-slot
    encoder loop, dropout on, dense per-slot embedding grads, torch Adam) on this box's host cores, as BASELINE.md
    section 3 plans it: B = 32 (BASELINE config 0's batch) and the largest B of 512 / 256 / 128 / 64 whose 3 warm-up + 5
    timed steps fit `budget_s`, estimated from the B = 32 rate."""
    from oracle import nrms_oracle as orc
    threads = host_threads()
    torch.set_num_threads(threads)
    params = synth.make_params(shape, seed=0)

    def run(users, warm, steps):
        trainer = orc.ReferenceShapedTrainer(params, shape.num_attention_heads, p_drop=0.2, lr=1e-3)
        batch = synth.make_batch(shape, seed=1, batch_size=users)
        for _ in range(warm):
            trainer.step(batch)
        t0 = time.perf_counter()
        for _ in range(steps):
            trainer.step(batch)
        return (time.perf_counter() - t0) / steps

    dt32 = run(32, 3, 5)
    log("cpu baseline: B=32 %.2f s/step on %d threads" % (dt32, threads))
    # the bench's own batch (512 users) when 1 warm-up + 3 timed steps of it fit the budget; a step gets cheaper per user as B
    # grows (measured 0.35 ... 0.45 of the B = 32 cost per user at B = 256), estimated at 0.5 to stay on the safe side
    big = 64
    for cand in (512, 256, 128):
        if dt32 * cand / 32.0 * 0.5 * 4 <= budget_s:
            big = cand
            break
    dtb = run(big, 1, 3)
    log("cpu baseline: B=%d %.2f s/step" % (big, dtb))
    best = max((32 / dt32, 32, dt32), (big / dtb, big, dtb))
    return {"value": best[0], "unit": "users/s", "cores": threads, "kind": "port", "cpu": cpu_model_name(),
            "sample": "3 warm-up + 5 timed train steps at B=32 and 1 warm-up + 3 timed at B=%d (the largest of 512/256/128/64 "
                      "estimated to fit %.0f s), same H/C/L/d/V, dropout 0.2, per-slot encoder loop + torch Adam, fp32, torch %s CPU, "
                      "%d threads = min(affinity set, cgroup CPU quota) of this process, i.e. every core it may use; value = the better of the two (B=%d)" % (
                          big, budget_s, torch.__version__, threads, best[1]),
            "by_batch": {"32": {"users_per_s": 32 / dt32, "ms_per_step": dt32 * 1e3},
                         str(big): {"users_per_s": big / dtb, "ms_per_step": dtb * 1e3}},
            "ms_per_step": best[2] * 1e3}


DUMP_TABLE_ROWS = 4096              # --dump-outputs: seeded sample of embedding-table rows (the whole table is 55 MB)


def dump_outputs(out_dir, model, loss_sum):
    """--dump-outputs: what the last timed step handed its caller -- the loss sum Model.train_step returned, the click
    scores of that step's forward and every parameter after its Adam update -- as <out_dir>/<name>.npy (float64 loss,
    float32 otherwise).  The word-embedding table is sampled: DUMP_TABLE_ROWS rows drawn without replacement by
    numpy.random.default_rng(0), in ascending order; every other parameter is written whole (about 8 MB in all)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss_sum": np.asarray(float(loss_sum), dtype=np.float64),
              "scores": model._last_scores.detach().float().cpu().numpy()}
    for name, p in model.state_dict().items():
        p = p.detach()
        if name == "news_encoder.word_embedding.0.weight":
            rows = np.sort(np.random.default_rng(0).choice(p.shape[0], size=min(DUMP_TABLE_ROWS, p.shape[0]), replace=False))
            p, name = p[torch.from_numpy(rows).to(p.device)], name + ".sampled_rows"
        arrays["param." + name] = p.float().cpu().numpy()
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    log("dumped %d outputs of the last timed step to %s (%.1f MB)" % (len(arrays), out_dir, sum(a.nbytes for a in arrays.values()) / 1e6))


def timed(fn, n, sync=True):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    if sync:
        torch.cuda.synchronize()
    return time.perf_counter() - t0


def eval_path_leg(model, dev):
    """SURVEY f-1: evaluation impressions padded to max_candidate_size = 300 (data_handler.py:174-177), 4 batches of 512
    impressions (the reference's dev loader uses config.batch_size = 512, run_v0.py:46,81-82) drawn from a 4000-news
    corpus: every slot encoded (as the reference does), distinct titles per batch (device hash table), and the
    persistent news-vector cache keyed by the batch dict's news ids."""
    from torch.utils.data import DataLoader
    from pytorch_news_recommender_amd.data_handler import MyDataset, SyntheticMind
    cfg = model.config
    cfg.max_candidate_size, cfg.history_len = 300, 50
    corpus = SyntheticMind(cfg, n_news=4000, seed=3)
    n_imp, per_batch = 2048, 512
    samples, _ = corpus.eval_samples(n_imp, max_shown=70)
    ds = MyDataset(cfg, samples, type=1, id2title_dict=corpus.id2title_dict)
    batches = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
               for b in DataLoader(ds, batch_size=per_batch, shuffle=False, num_workers=0)]
    model.eval()
    eng = model.engine

    def measure():
        ev = {}
        with torch.no_grad():
            def run_all():
                for b in batches:
                    model(b)
            model.dedup_inference = False
            run_all()
            ev["all_slots_impressions_per_s"] = n_imp * 3 / timed(run_all, 3)
            model.dedup_inference = True
            strip = [{k: v for k, v in b.items() if k not in ("browsed_ids", "candidate_ids")} for b in batches]

            def run_hash():
                for b in strip:
                    model(b)
            run_hash()
            ev["unique_titles_impressions_per_s"] = n_imp * 3 / timed(run_hash, 3)
            ev["unique_title_fraction"] = model.last_unique_titles / float(per_batch * 350)

            def run_cached():
                eng.news_cache_begin()
                for b in batches:
                    model(b)
                return eng.news_cache_end()
            run_cached()
            t = timed(run_cached, 3)
            stats = run_cached()
            ev["news_cache_impressions_per_s"] = n_imp * 3 / t
            ev["news_cache_encoded_titles"] = stats["encoded"]
            ev["news_cache_lookups"] = stats["lookups"]
        return ev

    # precision "fp16" evaluates in bf16x3 unless config.fp16_inference is set (AUC parity: evaluation scores 2e-6 from the oracle)
    keep = bool(getattr(cfg, "fp16_inference", False))
    cfg.fp16_inference = False
    ev = {"impressions": n_imp, "batch": per_batch, "slots_per_impression": 350,
          "inference_precision": "bf16x3" if cfg.precision in ("fp16", "bf16x3") else cfg.precision}
    ev.update(measure())
    if cfg.precision == "fp16":
        cfg.fp16_inference = True
        ev["fp16_inference_opt_in"] = measure()
    cfg.fp16_inference = keep
    model.train()
    return ev


def naml_leg(dev, B):
    """SURVEY f-3: one nrms_naml train step (model/nrms_naml.py) at the reference's own shapes -- title 20 and abstract
    40 words through the shared word-level encoder (6 heads, W_O), 100-wide category embeddings, LayerNorm, the 800-wide
    user encoder (8 heads, q = 400), dropout 0.2 -- in the bf16x3 mode (no fused fp16 kernels for this topology yet).  The
    all-padding title / abstract sequences (history padding slots, 41 % of the batch) take the closed form of csrc/empty_seq.hip;
    the kernel chain runs on the others, compacted."""
    from pytorch_news_recommender_amd.model.nrms_naml_hip import Model as NamlModel
    shape = synth.NamlShape(batch_size=B)
    cfg = Config("nrms_naml")
    cfg.__nrms__()
    cfg.dropout, cfg.learning_rate, cfg.precision = 0.2, 1e-3, "bf16x3"
    params = synth.make_params_naml(shape, seed=0)
    m = NamlModel(cfg, pretrained_word_embedding=params["news_encoder.word_embedding.weight"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev).train()
    batch = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_batch_naml(shape, seed=1).items()}
    for _ in range(3):
        m.train_step(batch)
    n = 10
    t = timed(lambda: m.train_step(batch), n)
    return {"users_per_s": B * n / t, "ms_per_step": t / n * 1e3, "steps": n, "precision": "bf16x3",
            "workload": "B=%d, H=50, C=5, title 20 + abstract 40 words, d=300, news_feature_size=800" % B}


def hierec_leg(dev, B):
    """SURVEY f-4 / BASELINE configs[3]: one train step of the HieRec-style hierarchical interest model (model/hierec_hip.py) at
    MIND shapes -- the headline's news encoder over B * 55 titles (fp16 mode), then three gather + additive-attention aggregates
    over index lists built on the device (clicks -> sub-topic interests -> topic interests -> user) and hierarchical matching.
    PARITY UNPINNED: the reference holds no implementation of this model (model/tanr.py is empty); the numbers are checked
    against oracle/segpool_oracle.py only (tests/test_hip_hierec.py)."""
    from pytorch_news_recommender_amd.model.hierec_hip import Model as HieRec
    n_sub, n_top = 285 + 1, 18 + 1                    # MIND-large: 18 categories, 285 sub-categories (+ the padding id)
    shape = synth.Shape(n_words=synth.BENCH.n_words, word_embed_size=300, num_attention_heads=10, query_vector_dim=200, batch_size=B,
                        history_len=50, n_candidates=5, n_words_title=30)
    cfg = Config("hierec")
    cfg.__nrms__()
    cfg.dropout, cfg.learning_rate, cfg.precision = 0.2, 1e-3, "fp16"
    cfg.subcategory_nums, cfg.category_nums = n_sub, n_top
    params = synth.make_params_hierec(shape, n_sub, n_top, seed=0)
    m = HieRec(cfg, pretrained_word_embedding=params["news_encoder.word_embedding.0.weight"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev).train()
    batch = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in synth.make_batch_hierec(shape, n_sub, n_top, seed=1, batch_size=B).items()}
    for _ in range(10):
        m.train_step(batch)
    n = 30
    t = timed(lambda: m.train_step(batch), n)
    eng = m.engine
    eng.timing(True)
    eng.timing_reset()
    k = 5
    for _ in range(k):
        m.train_step(batch)
    torch.cuda.synchronize()
    parts = {}
    for name in ("hier_tree", "hier_match", "hier_addemb", "hier_embgrad", "hier_score_fwd", "hier_score_bwd", "segpool_logit",
                 "segpool_fwd", "segpool_da", "segpool_dq", "segpool_scatter", "segpool_proj_fwd", "segpool_dwadd", "segpool_dx"):
        ms, cnt = eng.timing_read(name)
        parts[name] = round(ms / k, 4)
    eng.timing(False)
    tree_ms = sum(parts.values())
    return {"users_per_s": B * n / t, "ms_per_step": t / n * 1e3, "steps": n, "precision": "fp16 news encoder, bf16x3 aggregates",
            "interest_tree_kernels_ms_per_step": parts, "interest_tree_ms_per_step": round(tree_ms, 4),
            "parity": "UNPINNED: no reference implementation (model/tanr.py is empty); checked against oracle/segpool_oracle.py -- at this size the "
                      "training forward (fp16 news encoder) sits 6.0e-5 from it on scores up to 0.27, the bf16x3 inference routing 6.7e-7 "
                      "(tests/test_hip_hierec.py::test_f4_models_against_the_oracle_at_the_benchmarked_size)",
            "workload": "B=%d, H=50, C=5, title 30 words, d=300, 285 sub-topics / 18 topics (MIND-large), dropout 0.2" % B}


def graph_leg(dev, B):
    """SURVEY f-4 / BASELINE configs[4]: one train step of the user-news graph encoder (model/graph_hip.py) -- the headline's news
    encoder over B * 55 titles (fp16 mode), then the news layer (every slot gathers up to 8 sampled neighbour news of the batch's
    induced sub-graph and aggregates them by additive attention) and the user layer (a user's clicked slots), dot-product scores.
    One rank's share of a data-parallel job: users and their sampled sub-graphs shard across GPUs, gradients all-reduce.
    PARITY UNPINNED: the reference holds no graph model; checked against oracle/segpool_oracle.py (tests/test_hip_graph.py)."""
    from pytorch_news_recommender_amd.model.graph_hip import Model as Graph
    K = 8
    shape = synth.Shape(n_words=synth.BENCH.n_words, word_embed_size=300, num_attention_heads=10, query_vector_dim=200, batch_size=B,
                        history_len=50, n_candidates=5, n_words_title=30)
    cfg = Config("graph")
    cfg.__nrms__()
    cfg.dropout, cfg.learning_rate, cfg.precision = 0.2, 1e-3, "fp16"
    params = synth.make_params_graph(shape, seed=0)
    m = Graph(cfg, pretrained_word_embedding=params["news_encoder.word_embedding.0.weight"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev).train()
    batch = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in synth.make_batch_graph(shape, K, seed=1, batch_size=B).items()}
    for _ in range(10):
        m.train_step(batch)
    n = 30
    t = timed(lambda: m.train_step(batch), n)
    eng = m.engine
    eng.timing(True)
    eng.timing_reset()
    k = 5
    for _ in range(k):
        m.train_step(batch)
    torch.cuda.synchronize()
    parts = {}
    for name in ("csr_build", "segpool_logit", "segpool_fwd", "segpool_da", "segpool_rowlists", "segpool_dq", "segpool_scatter", "segpool_proj_fwd",
                 "segpool_dwadd", "segpool_dx"):
        ms, cnt = eng.timing_read(name)
        parts[name] = round(ms / k, 4)
    eng.timing(False)
    nnz = int(((batch["neighbor_rows"] >= 0).sum() + batch["browsed_mask"].sum()).item())
    return {"users_per_s": B * n / t, "ms_per_step": t / n * 1e3, "steps": n, "precision": "fp16 news encoder, bf16x3 aggregates",
            "aggregation_kernels_ms_per_step": parts, "aggregation_ms_per_step": round(sum(parts.values()), 4), "list_entries": nnz,
            "parity": "UNPINNED: no reference implementation; checked against oracle/segpool_oracle.py -- at this size the training forward (fp16 "
                      "news encoder) sits 1.3e-4 from it on scores up to 1.5 (its vectors are twice an NRMS news vector: 8.6e-5 relative), the "
                      "bf16x3 inference routing 2.2e-6 (tests/test_hip_hierec.py::test_f4_models_against_the_oracle_at_the_benchmarked_size)",
            "workload": "B=%d, H=50, C=5, title 30 words, d=300, up to %d sampled neighbours per news slot (induced sub-graph), dropout 0.2" % (B, K)}


def v1_leg(dev, B):
    """SURVEY a-3' / f-3: one nrms_v1 train step (model/nrms_v1.py: W_O, per-encoder heads, candidate mask; like the
    reference's forward, nrms_v1.py:286, the model applies no attention mask -- the masked primitives are tested apart) with
    the reference's v1 configuration (config.py: 20-word titles, 6 title heads of 50 / 10 user heads of 30), dropout 0.2,
    in the fp16 mode (csrc/fused16_v1.hip + fused16_v1_bwd.hip for the news encoder; the user encoder in bf16x3 as in the
    headline configuration) and, beside it, with both encoders in bf16x3."""
    from pytorch_news_recommender_amd.model.nrms_v1_hip import Model as V1Model
    shape = synth.Shape(n_words=synth.BENCH.n_words, word_embed_size=300, num_attention_heads=10, query_vector_dim=200,
                        batch_size=B, history_len=50, n_candidates=5, n_words_title=20)
    params = synth.make_params_v1(shape, seed=0)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_batch(shape, seed=1, batch_size=B).items()}
    res = {}
    # "default": config.precision = "fp16" as the headline uses it -- for nrms_v1 that keeps the W_O news encoder in bf16x3 (its
    # fused fp16 form is outside the absolute 1e-4 at this size, so it is opt-in: config.fp16_v1_news_encoder)
    for tag, opt_in in (("default", False), ("fp16_news_encoder_opt_in", True)):
        cfg = Config("nrms_v1")
        cfg.__nrms__()
        cfg.num_attention_heads, cfg.title_heads_num = 10, 6
        cfg.dropout, cfg.learning_rate, cfg.precision, cfg.fp16_v1_news_encoder = 0.2, 1e-3, "fp16", opt_in
        m = V1Model(cfg, pretrained_word_embedding=params["news_encoder.word_embedding.weight"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        m = m.to(dev).train()
        for _ in range(10):
            m.train_step(batch)
        n = 30
        t = timed(lambda: m.train_step(batch), n)
        res[tag] = {"users_per_s": B * n / t, "ms_per_step": t / n * 1e3, "steps": n}
        del m
    out = dict(res["default"])
    out.update({"precision": "bf16x3 (what config.precision = 'fp16' selects for nrms_v1: scores 2e-6 from the oracle at this size, "
                             "tests/test_hip_v1_fp16.py::test_v1_default_routing_against_the_oracle_at_the_benchmarked_size)",
                "fp16_news_encoder_opt_in": dict(res["fp16_news_encoder_opt_in"], score_parity=(
                    "OUTSIDE north_star's absolute 1e-4: max 1.56e-4 over the 2 555 scores of this batch, 2 % of them beyond 1e-4 "
                    "(score rms 0.092, max 0.36) -- config.fp16_v1_news_encoder = True, never a default")),
                "workload": "B=%d, H=50, C=5, title 20 words, d=300, 6 title heads / 10 user heads, W_O, candidate mask" % B})
    return out


def kernel_report(eng, args, shape, world, live_frac, compact, allpad_frac, dt_instr, per_gpu):
    """--full: `roofline`, `kernels` and `top_mfma_kernel` from the per-kernel HIP-event timers of the instrumented pass
    (args.steps recorded steps), plus the measured HBM traffic of the dominant kernel and of the whole step."""
    B = args.users_per_gpu
    fp16_news = args.precision == "fp16"
    work = kernel_work(shape, B, live_frac, compact, allpad_frac, fp16_news, bool(args.fp16_user_encoder))
    # which arithmetic each timer's kernels run in (fp16 mode: the user encoder's kernels are bf16x3)
    kprec = {k: args.precision for k in work}
    if fp16_news and not args.fp16_user_encoder:
        for k in ("user64_fwd", "user64_bwd", "qkv_proj_fwd", "addattn_fwd", "dctx_bwd", "attn_fwd", "attn_bwd", "addattn_bwd_rows"):
            kprec[k] = "bf16x3"
    kernels = {}
    for name, (bound, fl, by) in work.items():
        ms, n = eng.timing_read(name)
        if n == 0:
            continue
        sec = ms / args.steps * 1e-3
        kernels[name] = {"ms_per_step": ms / args.steps, "launches_per_step": n / args.steps, "bound": bound,
                         "tflops": fl / sec / 1e12, "gbps": by / sec / 1e9}
        if bound == "mfma":
            kernels[name]["frac_of_mfma_peak"] = fl / sec / 1e12 / PEAKS[kprec[name]]
        else:
            kernels[name]["frac_of_hbm_peak"] = by / sec / 1e9 / PEAK_HBM_GBPS
    for name in OTHER_TIMERS:
        ms, n = eng.timing_read(name)
        if n:
            kernels[name] = {"ms_per_step": ms / args.steps, "launches_per_step": n / args.steps}
    dom = max((k for k in kernels if "bound" in kernels[k]), key=lambda k: kernels[k]["ms_per_step"])
    dom_ms, dom_n = eng.timing_read(dom)
    bound, fl, by = work[dom]
    peak = PEAKS[kprec[dom]] if bound == "mfma" else PEAK_HBM_GBPS
    achieved = (fl / 1e12 if bound == "mfma" else by / 1e9) / (dom_ms / args.steps * 1e-3)
    # measured HBM bytes per step of that kernel and of the whole step: rocprofv3 PMC FETCH_SIZE x 2 + WRITE_SIZE in separate
    # passes (tools/hbm_traffic.py).  A committed profile is used only if it was measured on EXACTLY this kernel source
    # (hash of csrc/ + include/); otherwise the two passes run now, as child processes, on the code that was just timed.
    traffic, step_traffic, traffic_src = None, None, "unavailable"
    if B == 512 and world == 1:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import hbm_traffic
        sha = hbm_traffic.csrc_sha16()
        tfile = os.path.join(ROOT, "profiles", "r04_%s_hbm_traffic.json" % args.precision)
        prof = None
        if os.path.exists(tfile) and not args.fp16_user_encoder:
            try:
                cand = json.load(open(tfile))
                if cand.get("csrc_sha16") == sha:
                    prof, traffic_src = cand, "profiles/%s (same kernel source: csrc sha %s)" % (os.path.basename(tfile), sha)
                else:
                    traffic_src = "profiles/%s is stale (csrc sha %s != %s)" % (os.path.basename(tfile), cand.get("csrc_sha16"), sha)
            except Exception as e:
                traffic_src = "unreadable profile: %r" % (e,)
        if prof is None and not args.no_live_traffic:
            try:
                log("measuring HBM traffic live (two rocprofv3 --pmc passes as child processes)")
                torch.cuda.synchronize()
                prof = hbm_traffic.collect(os.path.join(tempfile.gettempdir(), "nrms_traffic_%d" % os.getpid()), steps=3,
                                           precision=args.precision, extra=["--fp16-user-encoder"] if args.fp16_user_encoder else [])
                traffic_src = "measured in this run (tools/hbm_traffic.py, 3 steps per pass)"
            except Exception as e:
                traffic_src += "; live measurement failed: %r" % (e,)
        if prof is not None:
            traffic = prof["by_timer"].get(dom, {}).get("hbm_bytes_per_step")
            step_traffic = prof.get("step_bytes")
    out = {
        "roofline": {"bound": bound, "kernel": dom, "achieved": achieved, "peak": peak,
                     "unit": "TFLOP/s" if bound == "mfma" else "GB/s", "frac": achieved / peak, "traffic": traffic,
                     "traffic_note": "HBM bytes per step of that kernel, rocprofv3 FETCH_SIZE x 2 + WRITE_SIZE (separate passes); "
                                     "source: " + traffic_src,
                     "step_traffic": step_traffic,
                     "step_traffic_note": "HBM bytes of ALL kernels of one train step, same measurement; algorithmic: 4.87 MB/user x %d = "
                                          "%.2f GB (SURVEY 8d)" % (B, 4.87e6 * B / 1e9),
                     "peak_note": ("HBM3E spec 8 TB/s (6.3 TB/s measured achievable)" if bound == "hbm" else
                                   {"fp32": "f32-input MFMA dense peak", "bf16": "bf16 MFMA dense peak", "fp16": "fp16 MFMA dense peak",
                                    "bf16x3": "bf16 dense peak / 3 (3 bf16 MFMAs per fp32-equivalent step by construction)"}[kprec[dom]]),
                     "avg_launch_ms": dom_ms / max(dom_n, 1),
                     "timing_note": "kernel durations: HIP events on the launch stream, recorded in a separate pass of the "
                                    "same %d steps (after as many unrecorded settling steps) before the warm-up and the (un-instrumented) timed region, with the helper streams off "
                                    "(NRMS_NO_SIDE_STREAMS) so that no two kernels share the GPU; that pass ran at "
                                    "%.2f ms/step" % (args.steps, dt_instr / args.steps * 1e3),
                     "algorithmic_per_step": by if bound == "hbm" else fl,
                     # the WHOLE step by BASELINE.md section 2: users/s x 3.558309e9 flop / peak (per GPU)
                     "step_frac": per_gpu * FLOP_PER_USER_TRAIN / (PEAK_16_MFMA_TFLOPS * 1e12),
                     "step_frac_note": "users/s per GPU x 3 558 309 000 flop (reference algorithm, padding included) / 2.5e15 "
                                       "(dense fp16/bf16 MFMA peak, undivided)",
                     "step_tflops_equiv": per_gpu * FLOP_PER_USER_TRAIN / 1e12},
        "kernels": kernels,
    }
    mf = [k for k in kernels if kernels[k].get("bound") == "mfma"]
    if mf:
        k = max(mf, key=lambda kk: kernels[kk]["ms_per_step"])
        out["top_mfma_kernel"] = {"kernel": k, "tflops": kernels[k]["tflops"], "peak": PEAKS[kprec[k]],
                                  "frac": kernels[k]["tflops"] / PEAKS[kprec[k]]}
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: steady state -- with 5 warm-up + 20 timed steps (0.09 s in all) the same box reads 2.5 ... 3.5 % lower (clocks, caches
    # and the allocator are still settling: 150.4 ... 152.5 k against 155.8 ... 156.0 k users/s on one box, three runs each)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--users-per-gpu", type=int, default=512)
    ap.add_argument("--resident-batches", type=int, default=32,
                    help="distinct synthetic batches resident in HBM that the steps cycle over (1 = replay one batch)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: per-kernel timers and roofline, HBM "
                         "traffic, score parity against the exact fp32 mode, the data-parallel facts (N > 1) and, N = 1, the "
                         "secondary legs (other precision modes, model variants, evaluation path) and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the secondary legs")
    ap.add_argument("--dense-padding", action="store_true",
                    help="diagnostics: process padding tokens densely (as if embedding row 0 were not zero)")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="with --full: do not run the two rocprofv3 --pmc child passes when the committed traffic profile is stale")
    ap.add_argument("--cpu-budget-s", type=float, default=60.0, help="with --full: wall-clock budget of the larger CPU-baseline batch")
    ap.add_argument("--grad-sync", default="allreduce", choices=["allreduce", "sharded"],
                    help="N > 1: one all-reduce of the flat gradient + full Adam on every rank (default), or reduce-scatter -> "
                         "Adam on the owned 1/N of the parameters -> all-gather (parallel.ShardedGradSync)")
    ap.add_argument("--grad-compress", default=None, choices=["bf16"],
                    help="--grad-sync sharded only: the table gradient travels as bf16 (opt-in; parity delta reported)")
    ap.add_argument("--fp16-user-encoder", action="store_true",
                    help="precision fp16: run the user encoder (3 %% of the flops) on the fused fp16 kernels too instead of "
                         "bf16x3 -- faster, but the scores then sit AT the 1e-4 bar on 512-user batches")
    ap.add_argument("--precision", default="fp16", choices=["fp32", "bf16x3", "bf16", "fp16"],
                    help="fp16 (default): fused one-wave-per-title kernels, scores inside 1e-4 of the oracle at 512 users "
                         "(the --full JSON line has the measured maximum); bf16x3: split-bf16 projections (2e-6); fp32 = exact f32 MFMA; "
                         "bf16 misses the bar (3e-4)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed region, write what its last step computed (loss sum, click scores, updated "
                         "parameters; a fixed sample of the embedding table) as DIR/<name>.npy (rank 0)")
    return ap.parse_args(argv)


def main():
    args = parse_args()
    # the dropout seeds derive from torch.initial_seed(), which torch otherwise draws afresh per process: fixed here so that
    # the same arguments give the same inputs, dropout masks included, from run to run
    torch.manual_seed(0)

    # N > 1 with --full: have RCCL write its topology / algorithm choices (rings, trees, channels, transports) to a per-rank
    # file so the multi-GPU record says what it ran on (parsed into data_parallel.rccl_info below)
    nccl_log = None
    if args.full and int(os.environ.get("WORLD_SIZE", "1")) > 1 and "NCCL_DEBUG" not in os.environ:
        nccl_log = "/tmp/nrms_rccl_%s_rank%s.log" % (os.environ.get("MASTER_PORT", "0"), os.environ.get("RANK", "0"))
        os.environ["NCCL_DEBUG"] = "INFO"
        os.environ["NCCL_DEBUG_SUBSYS"] = "INIT,GRAPH,ENV,TUNING"
        os.environ["NCCL_DEBUG_FILE"] = nccl_log
    rank, local_rank, world = parallel.init_process_group(os.environ.get("NRMS_DIST_BACKEND"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    dev_index = local_rank % max(torch.cuda.device_count(), 1)   # identity on a full node
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)

    shape = synth.BENCH
    B = args.users_per_gpu
    cfg = Config("nrms_hip")
    cfg.__nrms__()
    cfg.n_words_title = shape.n_words_title
    cfg.sample_size = shape.n_candidates - 1
    cfg.batch_size = B
    cfg.dropout = 0.2
    cfg.learning_rate = 1e-3
    cfg.precision = args.precision
    cfg.fp16_user_encoder = bool(args.fp16_user_encoder)
    cfg.skip_padding_tokens = not args.dense_padding
    cfg.word_embed_size = shape.word_embed_size
    params = synth.make_params(shape, seed=0)
    model = Model(cfg, pretrained_word_embedding=params["news_encoder.word_embedding.0.weight"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.to(dev).train()
    model._rank_salt = rank * 0x632BE59BD9B4E019
    eng = model.engine
    parallel.broadcast_parameters(model._flat)
    # each rank: its own users; the timed loop cycles over N_BATCHES distinct resident batches, so word ids, scatter groups,
    # title classes and cache state differ from step to step and `loss` stays a training loss (one replayed batch is memorised
    # within a few dozen steps)
    N_BATCHES = max(1, args.resident_batches)
    batches_np = [synth.make_batch(shape, seed=1 + rank + 1000 * i, batch_size=B) for i in range(N_BATCHES)]
    batches = [{k: torch.from_numpy(v).to(dev) for k, v in b.items()} for b in batches_np]
    batch_np, batch = batches_np[0], batches[0]
    reduce = None
    if world > 1:
        if args.grad_sync == "sharded":
            reduce = parallel.ShardedGradSync(model._flat.numel(), shape.n_words * shape.word_embed_size, compress=args.grad_compress)
        else:
            reduce = parallel.GradAllReduce()

    counter = [0]

    def step():
        b = batches[counter[0] % N_BATCHES]
        counter[0] += 1
        return model.train_step(b, world_size=world, all_reduce=reduce)

    # ---- --full: score parity of the timed mode, measured here (outside every timed region): the training forward of the timed
    # precision against the library's exact fp32 mode (itself pinned to the oracle at this size by
    # tests/test_hip_fullsize.py::test_every_mode_against_the_oracle_at_full_size) on timed batch 0, dropout off, initial weights
    def score_gap():
        p_keep, prec_keep = cfg.dropout, cfg.precision
        cfg.dropout = 0.0
        try:
            with torch.no_grad():
                bt, ct, cm = batch["browsed_titles"], batch["candidate_titles"], batch["candidate_mask"]
                cfg.precision = "fp32"
                ref = model.engine.forward(model._flat, bt, ct, cm, training=True).clone()
                cfg.precision = prec_keep
                got = model.engine.forward(model._flat, bt, ct, cm, training=True)
                e = (got - ref)[cm == 1].abs()
                return float(e.max()), float(ref[cm == 1].abs().max())
        finally:
            cfg.dropout, cfg.precision = p_keep, prec_keep
            model.engine        # re-applies config.precision

    parity_init = score_gap() if rank == 0 and args.full else None

    log("model ready on %s (rank %d/%d), %d users/GPU, precision %s" % (dev, rank, world, B, args.precision))
    # ---- the instrumented pass FIRST: K steps with the helper streams off (a kernel's duration under the timed region's
    # overlap is not its own) and, with --full, the per-kernel HIP-event timers on (two events created and recorded around
    # each launch slow a step by a few %, so they are NOT on during the timed region); `kernels` / `roofline` come from this
    # pass, on every rank so collectives stay aligned.  It runs before the W warm-up steps and the timed region, not after
    # them, and in a plain run too: a process that has stepped for only W = 5 steps is still 2.5 ... 3.5 % below its steady
    # state (clocks, caches; same box: 150.4 ... 152.5 k users/s after 5 steps, 155.8 ... 156.0 k after 30 or 50), sustained
    # training is what `value` stands for, and these steps are part of the training that the dumped outputs record.
    step()
    torch.cuda.synchronize()
    log("first step done")
    os.environ["NRMS_NO_SIDE_STREAMS"] = "1"
    for _ in range(args.steps):            # K settling steps in the same configuration, not recorded (the kernels' durations
        step()                             # are also 5 % longer in a process that has only just started stepping)
    if args.full:
        eng.timing_reset()
        eng.timing(True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    parallel.barrier()
    dt_instr = time.perf_counter() - t1
    eng.timing(False)
    os.environ.pop("NRMS_NO_SIDE_STREAMS", None)
    log("instrumented pass: %d settling + %d %s steps, the latter in %.3f s" % (
        args.steps, args.steps, "recorded" if args.full else "unrecorded", dt_instr))
    for i in range(args.warmup):
        step()
    torch.cuda.synchronize()
    log("warm-up done")
    # ---- the timed region: EXACTLY K un-instrumented steps
    parallel.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss_sum = step()
    torch.cuda.synchronize()
    parallel.barrier()
    dt = time.perf_counter() - t0
    dt_local = dt
    dt = parallel.max_over_ranks(dt, dev)
    loss = float(loss_sum) / B
    log("timed region: %d steps in %.3f s" % (args.steps, dt))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, loss_sum)      # before any later step changes the model
    eng.check_ids()             # the timed steps' word ids were all inside the vocabulary (one event wait)

    # ---- --full: data-parallel facts (every rank takes part; rank 0 reports)
    dp = None
    if world > 1 and args.full:
        import torch.distributed as dist
        ref = model._flat.clone()
        dist.broadcast(ref, src=0)
        diff = torch.tensor([float((model._flat - ref).abs().max())], device=dev)
        dist.all_reduce(diff, op=dist.ReduceOp.MAX)
        per_rank = [None] * world
        dist.all_gather_object(per_rank, dt_local / args.steps * 1e3)
        g = torch.zeros_like(model._flat)
        ar = parallel.GradAllReduce()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ar(g)
        torch.cuda.synchronize()
        parallel.barrier()
        evs[0].record()
        for _ in range(5):
            ar(g)
        evs[1].record()
        torch.cuda.synchronize()
        ar_ms = evs[0].elapsed_time(evs[1]) / 5
        # the two halves of the same exchange, as the sharded path issues them
        sh = parallel.ShardedGradSync(model._flat.numel(), shape.n_words * shape.word_embed_size)
        for hnd in (sh.start(g, 0), sh.start(g, 1)):
            hnd.wait()
        torch.cuda.synchronize()
        parallel.barrier()
        evs[2].record()
        for _ in range(5):
            for hnd in (sh.start(g, 0), sh.start(g, 1)):
                hnd.wait()
        evs[3].record()
        torch.cuda.synchronize()
        rs_ms = evs[2].elapsed_time(evs[3]) / 5
        scratch = model._flat.clone()
        sh.gather(scratch)
        torch.cuda.synchronize()
        parallel.barrier()
        evs[2].record()
        for _ in range(5):
            sh.gather(scratch)
        evs[3].record()
        torch.cuda.synchronize()
        ag_ms = evs[2].elapsed_time(evs[3]) / 5
        os.environ["NRMS_NO_OVERLAP"] = "1"
        for _ in range(2):
            step()
        parallel.barrier()
        t_no = parallel.max_over_ranks(timed(step, max(3, args.steps // 2)), dev) / max(3, args.steps // 2)
        del os.environ["NRMS_NO_OVERLAP"]
        parallel.barrier()
        rccl_info = None
        if nccl_log and os.path.exists(nccl_log):
            import re
            keep = re.compile(r"(nranks|Channel|Ring|Tree|channels|Algo|Proto|XGMI|xgmi|P2P|via|NCCL_|RCCL|Using network|Init COMPLETE|comm 0x)")
            lines = [ln.strip() for ln in open(nccl_log, errors="replace") if keep.search(ln)]
            rccl_info = {"log_lines": len(lines), "head": lines[:40], "tail": lines[-12:]}
        dp = {"rccl_ranks": dist.get_world_size(), "backend": dist.get_backend(), "grad_sync": args.grad_sync,
              "grad_compress": args.grad_compress, "per_rank_ms_per_step": per_rank,
              "reduce_scatter_ms": rs_ms, "all_gather_ms": ag_ms, "rccl_info": rccl_info,
              "allreduce_ms": ar_ms, "allreduce_bytes": int(model._flat.numel() * 4),
              "allreduce_algbw_GBps": model._flat.numel() * 4 / ar_ms / 1e6,
              "ms_per_step_without_overlap": t_no * 1e3, "overlap_ms": t_no * 1e3 - dt / args.steps * 1e3,
              "replicas_identical_after_timed_region": bool(diff.item() == 0.0),
              "max_abs_param_diff_vs_rank0": float(diff.item())}

    out = None
    if rank == 0:
        live = float(sum((b["browsed_titles"] != 0).sum() + (b["candidate_titles"] != 0).sum() for b in batches_np))
        live_frac = live / float(N_BATCHES * B * (shape.history_len + shape.n_candidates) * shape.n_words_title)
        compact = bool(eng.pad_row_zero)
        titles = np.concatenate([b[k].reshape(-1, shape.n_words_title) for b in batches_np for k in ("browsed_titles", "candidate_titles")])
        allpad_frac = 1.0 - float((titles != 0).any(axis=1).mean())
        total_users = B * world * args.steps
        users_per_s = total_users / dt
        per_gpu = users_per_s / world
        out = {
            "metric": "users/sec (train step) NRMS MIND-small hist=50 cand=5",
            "value": users_per_s, "unit": "users/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "warmup_effective": 1 + 2 * args.steps + args.warmup,
            "warmup_note": "steps this process had run when the timed region started: 1 first step + K settling + K instrumented "
                           "(helper streams off; per-kernel timers with --full) + W warm-up; steady state is what `value` reports -- a "
                           "process that has stepped only W = 5 times reads 2.5 ... 3.5 % lower (DESIGN 6)",
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": DTYPES[args.precision], "data": "synthetic",
            "config": {"workload": "configs[1] shapes: NRMS(nrms_v0) train step, %d users/GPU, hist=50, "
                                   "cand=5, title_len=30, d=300, h=10, q=200, V=45800, dropout=0.2, Adam(lr=1e-3)" % B,
                       "users_per_gpu": B, "global_batch": B * world,
                       "non_padding_token_fraction": round(live_frac, 4),
                       "all_padding_title_fraction": round(allpad_frac, 4),
                       "padding_tokens_skipped": ("dX + embedding scatter (dead values); Q|K|V projection and d(w_qkv) too: "
                                                  "embedding row 0 is zero" if compact else
                                                  "dX + embedding scatter (dead values)"),
                       "parallelism": "dp%d" % world, "precision": args.precision,
                       "resident_batches": N_BATCHES},
            "loss": loss,
        }
        if args.full:
            out["config"]["score_parity_vs_reference"] = (
                "max |score - exact fp32 mode| = %.2e over the valid scores of timed batch 0 (max |score| %.3f), training "
                "forward, dropout off, initial weights, measured in this run; the fp32 mode is pinned to the oracle at this "
                "size to 1e-5 and this mode to 1e-4 by tests/test_hip_fullsize.py" % parity_init)
            out["config"]["score_parity_max_abs"] = parity_init[0]
            out.update(kernel_report(eng, args, shape, world, live_frac, compact, allpad_frac, dt_instr, per_gpu))
        if dp is not None:
            out["data_parallel"] = dp
    # --full, secondary (N = 1, outside the timed region of `value`): the other modes on the same batch
    if world == 1 and args.full and not args.no_cpu_baseline and rank == 0:
        modes = {}
        n = max(3, args.steps // 2)
        log("secondary legs: modes")
        try:
            for prec in ("bf16x3", "fp32", "fp16"):
                if prec == args.precision:
                    continue
                cfg.precision = prec
                for _ in range(2):
                    step()
                modes[prec] = {"users_per_s": B * n / timed(step, n), "steps": n, "score_parity_vs_reference": PARITY[prec]}
            cfg.precision = args.precision
            # dense padding (as for a table whose row 0 is not zero: only the dead dX rows are skipped)
            cfg.skip_padding_tokens = False
            for _ in range(2):
                step()
            modes["dense_padding"] = {"users_per_s": B * n / timed(step, n), "steps": n, "precision": args.precision}
            cfg.skip_padding_tokens = not args.dense_padding
            # the drop-in loop of train_eval.py:111-127: model(batch) -> CE -> loss.backward() -> torch.optim.Adam.step
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            crit = torch.nn.CrossEntropyLoss()
            model.reuse_grad_buffer = True           # as train_eval.train(use_autograd=True) sets it

            def ref_loop():
                outp = model(batch)
                model.zero_grad()
                crit(outp, torch.zeros(len(outp), dtype=torch.long, device=outp.device)).backward()
                opt.step()
            for _ in range(2):
                ref_loop()
            modes["autograd_torch_adam"] = {"users_per_s": B * n / timed(ref_loop, n), "steps": n, "precision": args.precision,
                                            "note": "reference-compatible sequence (INTEGRATION.md section 2) through the same kernels"}
        except Exception as e:
            modes["error"] = repr(e)
        out["modes"] = modes
        log("secondary legs: variants (nrms_naml, nrms_v1, hierec, graph)")
        try:
            out["variants"] = {"nrms_naml": naml_leg(dev, B), "nrms_v1": v1_leg(dev, B), "hierec": hierec_leg(dev, B), "graph": graph_leg(dev, B)}
        except Exception as e:       # secondary leg only
            out["variants"] = {"error": repr(e)}
        log("secondary legs: evaluation path")
        try:
            out["eval_path"] = eval_path_leg(model, dev)
        except Exception as e:       # secondary leg only: never lose the headline line
            out["eval_path"] = {"error": repr(e)}
    # the CPU baseline LAST: its OpenMP worker threads keep spinning for a while after each parallel region, which starves the
    # host thread that launches the GPU legs above (the ~50-launch bf16x3 step measured 58 k instead of 72 k users/s behind it)
    if world == 1 and args.full and not args.no_cpu_baseline and rank == 0:
        torch.cuda.synchronize()
        log("cpu baseline")
        out["cpu_baseline"] = cpu_baseline(shape, budget_s=args.cpu_budget_s)
        log("done")
    if rank == 0:
        print(json.dumps(out), flush=True)
    parallel.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
