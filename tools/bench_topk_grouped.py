"""Timing of grouped catalogue retrieval (docs/EXPERIMENTS.md): nrms_topk_grouped_dot (NRMSEngine.top_k_grouped), with
nrms_topk_dot at the same shape as its floor, against the torch composition it replaces -- G torch.mm into a preallocated
[N, B] fp32 buffer, scatter_ of -inf over the history rows, torch.topk -- plus nrms_hier_query and the whole HieRec
Model.recommend per batch.  B = 512 users, N = 130 000 news, d = 300, k in {10, 100}, G in {1, 18, 294} groups of skewed
sizes (Zipf-like, as MIND's sub-categories), 50 history ids per user.  Device-event timing; every path is warmed up first
and the paths alternate.  Usage: python tools/bench_topk_grouped.py [B] [N] [reps]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pytorch_news_recommender_amd import _lib, synth
from pytorch_news_recommender_amd.config import Config
from pytorch_news_recommender_amd.engine import _stream
from pytorch_news_recommender_amd.model.hierec_hip import Model


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def group_sizes(N, G, rng):
    w = 1.0 / np.arange(1, G + 1) ** 1.1
    sizes = np.maximum(1, np.floor(w / w.sum() * N)).astype(np.int64)
    sizes[0] += N - sizes.sum()
    return rng.permutation(sizes)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 130000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    d, H, L = 300, 50, 30
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    cfg = Config("hierec")
    cfg.__nrms__()
    cfg.word_embed_size, cfg.num_attention_heads, cfg.query_vector_dim = d, 10, 200
    cfg.category_nums, cfg.subcategory_nums = 19, 295
    shape = synth.Shape(n_words=30000, word_embed_size=d, num_attention_heads=10, query_vector_dim=200, batch_size=8,
                        history_len=H, n_candidates=5, n_words_title=L)
    params = synth.make_params(shape, seed=1)
    model = Model(cfg, pretrained_word_embedding=params["news_encoder.word_embedding.0.weight"]).to(dev)
    titles = torch.randint(1, shape.n_words, (N + 1, L), device=dev, generator=g)
    titles[:, 20:] = 0
    titles[0] = 0
    print("B=%d N=%d d=%d history=%d" % (B, N, d, H))
    for G in (1, 18, 294):
        sizes = group_sizes(N, G, rng)
        pair = np.repeat(np.arange(G), sizes)[rng.permutation(N)]          # news id n + 1 -> its group
        categ = torch.as_tensor(np.concatenate([[0], 1 + pair % 18]), device=dev)
        sub = torch.as_tensor(np.concatenate([[0], 1 + pair]), device=dev)
        cat = model.encode_catalogue(titles, categ, sub)
        eng = model.engine
        assert cat.group_topic.shape[0] == G
        browsed = torch.randint(1, N + 1, (B, H), device=dev, generator=g)
        batch = {"browsed_ids": browsed}
        query = torch.randn(B, G, d, device=dev, generator=g)
        user = query[:, 0].contiguous()
        # history rows in the grouped order (the torch path scatters by row)
        pos = torch.empty(N + 1, dtype=torch.int64, device=dev)
        pos[cat.item_ids.long()] = torch.arange(N, device=dev)
        hist_rows = pos[browsed]
        buf = torch.empty(N, B, device=dev)
        gp = cat.group_ptr.tolist()

        def torch_path(k):
            for gi in range(G):
                if gp[gi + 1] > gp[gi]:
                    torch.mm(cat.items[gp[gi]:gp[gi + 1]], query[:, gi].T, out=buf[gp[gi]:gp[gi + 1]])
            buf.scatter_(0, hist_rows.T, float("-inf"))
            s, r = torch.topk(buf, k, dim=0)
            return s, cat.item_ids[r]

        # nrms_hier_query on one batch's interests
        slots = browsed.reshape(-1)
        t, u1, u2, ug, _ = eng._interests(model._flat, cat.vectors.index_select(0, slots), (browsed != 0).to(torch.uint8),
                                          cat.categ.index_select(0, slots), cat.subcateg.index_select(0, slots), B, H, "_bench")
        hq = torch.empty(B, G, d, device=dev)

        def hier_query():
            _lib.check(eng.lib.nrms_hier_query(B, H, G, d, _lib.ptr(cat.group_topic), _lib.ptr(cat.group_sub),
                                               *[_lib.ptr(t[x]) for x in ("l1_sub", "l1_cnt", "l2_top", "l2_cnt", "n_valid")],
                                               _lib.ptr(u1), _lib.ptr(u2), _lib.ptr(ug), C.c_float(eng.lambda_sub),
                                               C.c_float(eng.lambda_top), _lib.ptr(hq), _stream()), "nrms_hier_query")

        big = sizes.max()
        print("G=%d: groups of %d .. %d news (median %d), %d tiles of 32 for %d news"
              % (G, sizes.min(), big, int(np.median(sizes)), int(np.sum((sizes + 31) // 32)), N))
        for k in (10, 100):
            paths = [("nrms_topk_grouped_dot", lambda: eng.top_k_grouped(query, cat.items, cat.item_ids, cat.group_ptr, k, browsed)),
                     ("nrms_topk_dot (floor)", lambda: eng.top_k(user, cat.items, k, hist_rows)),
                     ("nrms_hier_query", hier_query),
                     ("HieRec recommend", lambda: model.recommend(batch, k, cat)),
                     ("torch G mm+scatter+topk", lambda: torch_path(k))]
            for _, fn in paths:
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in paths}
            for _ in range(3):
                for name, fn in paths:
                    times[name].append(event_ms(fn, reps))
            for name, ts in times.items():
                print("G=%-3d k=%-3d %-24s %8.3f ms (runs %s)" % (G, k, name, min(ts), " ".join("%.3f" % x for x in ts)))
            ratio = min(times["nrms_topk_grouped_dot"]) / min(times["nrms_topk_dot (floor)"])
            print("G=%-3d k=%-3d grouped / floor = %.2f, torch / grouped = %.2f" % (G, k, ratio, min(times["torch G mm+scatter+topk"])
                                                                               / min(times["nrms_topk_grouped_dot"])))


if __name__ == "__main__":
    main()
