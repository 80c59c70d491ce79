"""Timing of nrms_bert (model/nrms_bert_hip.py): B = 512 users, H = 50, C = 5, N = 130 000 news, E in {512, 1024}, dropout 0.2,
8 distinct resident batches cycled (MIND-like popularity: ids drawn Zipf-like, so popular news repeat across histories).
Reports per width: users/s of the fused train step in fp32 and bf16x3; the same step as a torch-eager fp32 restatement of
the model (nn.Embedding dense gradient, F.linear / matmul / softmax, autograd, torch.optim.Adam) in the same process on the
same GPU, as the baseline; evaluation impressions/s (300 candidate slots per impression, the news table encoded once per
evaluation as train_eval does); recommend ms per 512-user batch (k = 10 over the whole catalogue); the executed GFLOP of one
train step.  Device-event timing after a warm-up.  Prints one JSON line.

Usage: python tools/bench_nrms_bert.py [steps] [warmup]"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from pytorch_news_recommender_amd import synth
from pytorch_news_recommender_amd.config import Config
from pytorch_news_recommender_amd.model.nrms_bert_hip import Model

B, H, C, N, P_DROP, N_BATCHES = 512, 50, 5, 130000, 0.2, 8


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(reps):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def batches(n, c, seed, dev):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, N) ** 0.9
    w /= w.sum()
    out = []
    for _ in range(n):
        hl = rng.integers(1, H + 1, size=B)
        live = np.arange(H)[None, :] < hl[:, None]
        hist = np.where(live, rng.choice(np.arange(1, N), size=(B, H), p=w), 0)
        cand = rng.choice(np.arange(1, N), size=(B, c), p=w)
        cm = np.ones((B, c), dtype=np.uint8)
        if c > C:
            cl = rng.integers(2, 60, size=B)
            cm = (np.arange(c)[None, :] < cl[:, None]).astype(np.uint8)
            cand = np.where(cm != 0, cand, 0)
        out.append({"browsed_ids": torch.from_numpy(hist).to(dev), "candidate_ids": torch.from_numpy(cand).to(dev),
                    "browsed_mask": torch.from_numpy(live.astype(np.uint8)).to(dev), "candidate_mask": torch.from_numpy(cm).to(dev)})
    return out


def eager_step_fn(params, heads, dev):
    """The model restated in torch eager fp32 with autograd and torch.optim.Adam (the baseline)."""
    P = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in params.items()}
    opt = torch.optim.Adam(P.values(), lr=1e-3)
    a, ad = "user_encoder.multi_head_self_attention.", "user_encoder.additive_attention."

    def step(b):
        bi, ci, bm, cm = b["browsed_ids"], b["candidate_ids"], b["browsed_mask"], b["candidate_mask"]
        Bn, Hn = bi.shape
        nv = F.linear(F.embedding(torch.cat([bi.reshape(-1), ci.reshape(-1)]), P["news_encoder.news_embedding.weight"]),
                      P["news_encoder.news_dense.0.weight"], P["news_encoder.news_dense.0.bias"])
        nv = F.dropout(nv, P_DROP, True)
        E = nv.shape[1]
        hist, cand = nv[:Bn * Hn].view(Bn, Hn, E), nv[Bn * Hn:].view(Bn, -1, E)
        q, k, v = [F.linear(hist, P[a + "linear_layers.%d.weight" % i], P[a + "linear_layers.%d.bias" % i]).view(Bn, Hn, heads, -1)
                   .transpose(1, 2) for i in range(3)]
        s = q @ k.transpose(-2, -1) / math.sqrt(E // heads)
        s = s.masked_fill((bm.unsqueeze(1) * bm.unsqueeze(2)).unsqueeze(1) == 0, -1e9)
        pa = F.dropout(torch.softmax(s, -1), P_DROP, True)
        x = F.linear((pa @ v).transpose(1, 2).reshape(Bn, Hn, E), P[a + "output_linear.weight"], P[a + "output_linear.bias"])
        sc = torch.tanh(F.linear(x, P[ad + "linear.weight"], P[ad + "linear.bias"])) @ P[ad + "query_vector"]
        w = torch.softmax(sc.masked_fill(bm == 0, -1e9), 1)
        user = (w.unsqueeze(2) * x).sum(1)
        scores = (user.unsqueeze(1) * cand).sum(-1).masked_fill(cm == 0, -1e9)
        loss = F.cross_entropy(scores, torch.zeros(Bn, dtype=torch.long, device=scores.device))
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def step_gflop(E, Q, U):
    """Executed GEMM / attention flops of one train step (forward + backward), U = distinct news of the batch."""
    nv = 3 * 2 * U * E * E                                   # dense: forward, d(W), dX
    M = B * H
    user_fwd = 2 * M * 3 * E * E + 2 * 2 * B * H * H * E + 2 * M * E * E + 2 * M * Q * E + 2 * B * C * E
    return (nv + 3 * user_fwd) / 1e9


def bench_width(E, steps, warmup, dev):
    shape = synth.BertShape(n_news=N, bert_embed_size=E, batch_size=B)
    params = synth.make_params_bert(shape, seed=1)
    train = batches(N_BATCHES, C, 2, dev)
    res = {}
    for prec in ("fp32", "bf16x3"):
        cfg = Config("nrms_bert")
        cfg.__nrms__()
        cfg.bert_embed_size, cfg.dropout, cfg.precision = E, P_DROP, prec
        m = Model(cfg, pretrained_news_vectors=params["news_encoder.news_embedding.weight"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        m = m.to(dev).train()
        run = lambda i: m.train_step(train[i % N_BATCHES])
        event_ms(run, warmup)
        ms = event_ms(run, steps)
        res["train_users_per_s_" + prec] = B / ms * 1e3
        res["train_ms_" + prec] = ms
        if prec == "fp32":
            n, _ = m.engine.distinct_ids(B * (H + C))
            U = int(n.item())
            res["distinct_news_per_batch"] = U
            res["step_gflop"] = step_gflop(E, cfg.query_vector_dim_large, U)
            # evaluation: 300 candidate slots per impression, the table through news_dense once per evaluation
            ev = batches(4, 300, 3, dev)
            m.eval()
            eng = m.engine

            def evaluate(i):
                eng.news_cache_begin()
                with torch.no_grad():
                    for b in ev:
                        m(b)
                eng.news_cache_end()
            event_ms(evaluate, 1)
            ms_eval = event_ms(evaluate, max(1, steps // 10))
            res["eval_impressions_per_s"] = len(ev) * B / ms_eval * 1e3
            cat = m.encode_catalogue(None)
            rec = lambda i: m.recommend(train[i % N_BATCHES], 10, cat)
            event_ms(rec, warmup)
            res["recommend_ms_per_512_users"] = event_ms(rec, steps)
        del m
        torch.cuda.empty_cache()
    step = eager_step_fn(params, 8, dev)
    run = lambda i: step(train[i % N_BATCHES])
    event_ms(run, warmup)
    ms = event_ms(run, steps)
    res["torch_eager_fp32_users_per_s"] = B / ms * 1e3
    res["torch_eager_fp32_ms"] = ms
    res["speedup_bf16x3_vs_eager"] = res["train_users_per_s_bf16x3"] / res["torch_eager_fp32_users_per_s"]
    res["speedup_fp32_vs_eager"] = res["train_users_per_s_fp32"] / res["torch_eager_fp32_users_per_s"]
    return res


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda")
    out = dict(tool="bench_nrms_bert", B=B, H=H, C=C, N=N, dropout=P_DROP, resident_batches=N_BATCHES, steps=steps, warmup=warmup,
               device=torch.cuda.get_device_name(0))
    for E in (512, 1024):
        out["E%d" % E] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in bench_width(E, steps, warmup, dev).items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
