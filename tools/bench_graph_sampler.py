"""Timing of the global click-graph sampler (click_graph.py, csrc/graphsample.hip) at the bench geometry: B = 512 users, H = 50,
C = 5, K = 8 neighbours per slot, over a synthetic Zipf-skewed click graph of 130 000 news whose node and edge counts are printed.
PARITY UNPINNED: the reference has no graph model; none of these figures enters the headline.

Reports, per 512-user batch (device-event timing after a warm-up, 8 distinct resident batches cycled):
  * sample + resolve + gather (nrms_graph_sample_neighbors, nrms_graph_resolve_rows, the catalogue rows of extra_ids), and the
    three parts on their own;
  * the path this replaces on the same batches: graph_sampler.induced_neighbor_rows with the copies it needs (titles and mask
    to the host, neighbor_rows back), wall clock;
  * the train step (fp16 news encoder, dropout 0.2) with the global graph attached against the same step on prebuilt
    neighbor_rows (bench.py's graph leg), and how many out-of-batch rows a batch uses of config.graph_extra_rows;
  * the graph's HBM footprint and the cost of one catalogue refresh (encode_catalogue over every title).
Prints one JSON line; with an argument, also writes it there.

Usage: python tools/bench_graph_sampler.py [steps] [warmup] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pytorch_news_recommender_amd import synth
from pytorch_news_recommender_amd.click_graph import ClickGraph
from pytorch_news_recommender_amd.config import Config
from pytorch_news_recommender_amd.graph_sampler import induced_neighbor_rows
from pytorch_news_recommender_amd.model.graph_hip import Model

B, H, C, L, K, N_NEWS, N_USERS, N_BATCHES, ZIPF = 512, 50, 5, 30, 8, 130000, 100000, 8, 1.05


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(reps):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def world(shape, dev, seed=1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, N_NEWS) ** ZIPF
    ids = rng.permutation(np.arange(1, N_NEWS))[rng.choice(N_NEWS - 1, size=(N_USERS, H), p=w / w.sum())]
    lens = rng.integers(3, H + 1, size=N_USERS)
    hist = np.where(np.arange(H)[None, :] < lens[:, None], ids, 0).astype(np.int64)
    titles = rng.integers(1, shape.n_words, size=(N_NEWS, L)).astype(np.int64)
    titles[np.arange(L)[None, :] >= rng.integers(5, L + 1, size=N_NEWS)[:, None]] = 0
    titles[0] = 0
    titles_d = torch.from_numpy(titles).to(dev)
    batches = []
    for _ in range(N_BATCHES):
        users = rng.choice(N_USERS, size=B, replace=False)
        bi = torch.from_numpy(hist[users]).to(dev)
        ci = torch.from_numpy(rng.integers(1, N_NEWS, size=(B, C)).astype(np.int64)).to(dev)
        batches.append({"browsed_ids": bi, "candidate_ids": ci, "browsed_mask": (bi != 0).to(torch.uint8),
                        "candidate_mask": torch.ones(B, C, dtype=torch.uint8, device=dev),
                        "browsed_titles": titles_d[bi.reshape(-1)].view(B, H, L), "candidate_titles": titles_d[ci.reshape(-1)].view(B, C, L)})
    return torch.from_numpy(hist), titles_d, batches


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda")
    shape = synth.Shape(n_words=synth.BENCH.n_words, word_embed_size=300, num_attention_heads=10, query_vector_dim=200, batch_size=B,
                        history_len=H, n_candidates=C, n_words_title=L)
    hist, titles, batches = world(shape, dev)
    t = time.perf_counter()
    graph = ClickGraph.from_histories(hist, N_NEWS, dev)
    torch.cuda.synchronize()
    out = dict(tool="bench_graph_sampler", parity="UNPINNED: the reference has no graph model", B=B, H=H, C=C, K=K, zipf=ZIPF,
               device=torch.cuda.get_device_name(0), steps=steps, warmup=warmup, resident_batches=N_BATCHES,
               graph=dict(users=graph.n_users, news=graph.n_news, edges=graph.n_edges, hbm_mb=round(graph.nbytes() / 1e6, 2),
                          build_ms=round((time.perf_counter() - t) * 1e3, 1), news_without_clicks=int((graph.news_ptr.diff() == 0).sum())))

    cfg = Config("graph")
    cfg.__nrms__()
    cfg.dropout, cfg.learning_rate, cfg.precision, cfg.graph_neighbors = 0.2, 1e-3, "fp16", K
    cap = int(cfg.graph_extra_rows)
    params = synth.make_params_graph(shape, seed=0)

    def model():
        m = Model(cfg, pretrained_word_embedding=params["news_encoder.word_embedding.0.weight"])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        return m.to(dev).train()

    m = model()
    t_attach = wall_ms(lambda i: m.attach_click_graph(graph, titles), 1)            # first call: allocations included
    out["catalogue_refresh_ms"] = round(wall_ms(lambda i: m.refresh_neighbor_vectors(), 3), 3)
    out["attach_ms_first_call"] = round(t_attach, 1)
    out["catalogue_mb"] = round(m._catalogue.numel() * 4 / 1e6, 1)

    # ---- the sampler on its own
    # (the slot ids exactly as Model._global_neighbors forms them: history slots outside browsed_mask count as padding)
    def slot_ids(b):
        bi = b["browsed_ids"]
        return torch.cat([torch.where(b["browsed_mask"] != 0, bi, torch.zeros_like(bi)).reshape(-1), b["candidate_ids"].reshape(-1)])

    slots = [slot_ids(b) for b in batches]
    cat = m._catalogue
    state = {}

    def sample(i):
        state["nbr"] = graph.sample_neighbors(slots[i % N_BATCHES], K, seed=i)

    def resolve(i):
        state["res"] = graph.resolve_rows(slots[i % N_BATCHES], state["nbr"], cap)

    def gather(i):
        state["vec"] = cat.index_select(0, state["res"][1].to(torch.int64))

    def all_three(i):
        sample(i), resolve(i), gather(i)

    event_ms(all_three, warmup)
    sampler = {"sample_ms": event_ms(sample, steps), "resolve_ms": event_ms(resolve, steps), "gather_ms": event_ms(gather, steps),
               "sample_resolve_gather_ms": event_ms(all_three, steps), "sample_resolve_gather_wall_ms": wall_ms(all_three, steps)}
    used = []
    for i in range(N_BATCHES):
        all_three(i)
        used.append(int(state["res"][2].item()))
    sampler["out_of_batch_rows_per_batch"] = dict(min=min(used), max=max(used), cap=cap, dropped=int(graph.dropped_extra.item()))
    sampler["draws_with_a_neighbour"] = round(float((state["nbr"] >= 0).float().mean()), 4)
    out["global_sampler"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in sampler.items()}

    # ---- the host path it replaces, on the same batches
    def induced(i):
        b = batches[i % N_BATCHES]
        cpu = lambda v: v.cpu().numpy()
        rows = induced_neighbor_rows(cpu(b["browsed_titles"]), cpu(b["browsed_mask"]), cpu(b["candidate_titles"]), K, seed=i)
        state["rows"] = torch.from_numpy(rows).to(dev)

    induced(0)
    out["induced_host_sampler_wall_ms"] = round(wall_ms(induced, max(3, steps // 5)), 3)

    # ---- the train step: global graph against prebuilt neighbor_rows
    run = lambda i: m.train_step(batches[i % N_BATCHES])
    event_ms(run, warmup)
    ms_global = event_ms(run, steps)
    wall_global = wall_ms(run, steps)
    dropped = m.check_click_graph()
    del m
    torch.cuda.empty_cache()
    m2 = model()
    pre = []
    for i, b in enumerate(batches):
        nbr = graph.sample_neighbors(slots[i], K, seed=i)
        rows = graph.resolve_rows(slots[i], nbr, 0)[0]                          # in-batch rows only: bench.py's kind of batch
        pre.append(dict(b, neighbor_rows=rows))
    run2 = lambda i: m2.train_step(pre[i % N_BATCHES])
    event_ms(run2, warmup)
    ms_pre = event_ms(run2, steps)
    wall_pre = wall_ms(run2, steps)
    out["train_step"] = dict(global_graph_ms=round(ms_global, 4), global_graph_wall_ms=round(wall_global, 4), prebuilt_rows_ms=round(ms_pre, 4),
                             prebuilt_rows_wall_ms=round(wall_pre, 4), global_users_per_s=round(B / wall_global * 1e3, 1),
                             prebuilt_users_per_s=round(B / wall_pre * 1e3, 1), dropped_out_of_batch_neighbours=dropped,
                             note="prebuilt rows keep in-batch neighbours only (N rows pooled); the global step pools N + %d rows" % cap)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
