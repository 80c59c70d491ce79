"""Timing of the per-user tag sets in retrieval and ranking at B = 512 users, N = 130 000 news, d = 300,
50 excluded ids, k = 10 / 100, T = 1 / 8, 19 tags, in one process:
  (i)   nrms_topk_dot_tagged / nrms_rank_dot_tagged with every tag open beside this tree's plain nrms_topk_dot / nrms_rank_dot: the
        pure overhead of the filter (the tag load, the LDS word, the bit test, the bitmap built once per block).
  (ii)  every user open to a random half of the 19 tags, tags in random row order.
  (iii) every user open to 2 of the 19 tags: tags in random row order (a wave's 64 items carry most tags, the dead-wave skip
        cannot fire), and the catalogue sorted by tag with the batch sorted by its first tag (the users of a block share few
        tags, whole waves are dead: what the skip buys).
  (iv)  a torch restatement: mm, a per-user mask gathered from the tags, scatter_ of the excluded ids, topk.
Device-event timing; every path is warmed up first, the paths alternate, each window is `reps` calls and every window's time is
kept: the record holds the minimum and the spread (max - min over the windows) of every path, and the overhead of (i) beside the
plain call's own spread.  This is a record, not a gate.  Parity is unpinned: the reference has no catalogue retrieval.
Usage: python tools/bench_topk_tags.py [B] [N] [reps] [--windows W] [--json FILE]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, pack_tag_mask


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def opt(argv, name, default, conv):
    if name in argv:
        i = argv.index(name)
        v = conv(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def main():
    argv = list(sys.argv[1:])
    out = opt(argv, "--json", None, str)
    windows = opt(argv, "--windows", 5, int)
    B = int(argv[0]) if len(argv) > 0 else 512
    N = int(argv[1]) if len(argv) > 1 else 130000
    reps = int(argv[2]) if len(argv) > 2 else 20
    d, H, n_tags = 300, 50, 19
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    user = torch.randn(B, d, device=dev, generator=g)
    items = torch.randn(N, d, device=dev, generator=g)
    hist = torch.randint(0, N, (B, H), device=dev, generator=g)
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)

    tag = torch.randint(0, n_tags, (N,), device=dev, generator=g).to(torch.int32)        # tags in random row order
    order = torch.argsort(tag.long(), stable=True)                                       # the same catalogue stored tag after tag
    items_so, tag_so = items[order].contiguous(), tag[order].contiguous()
    inv = torch.empty_like(order)
    inv[order] = torch.arange(N, device=dev)
    hist_so = inv[hist].contiguous()

    every = torch.ones(B, n_tags, dtype=torch.bool, device=dev)
    half = torch.rand(B, n_tags, device=dev, generator=g) < 0.5
    two = torch.zeros(B, n_tags, dtype=torch.bool, device=dev)
    first = torch.randint(0, n_tags, (B,), device=dev, generator=g).sort().values       # the batch sorted by its first tag
    two[torch.arange(B, device=dev), first] = True
    two[torch.arange(B, device=dev), (first + 1) % n_tags] = True
    sets = {"all open": pack_tag_mask(every), "half of 19": pack_tag_mask(half), "2 of 19": pack_tag_mask(two)}
    neg_inf = torch.full((B, H), float("-inf"), device=dev)

    def torch_topk(k, t, allow, it, ex):
        s = torch.mm(user, it.T)
        s.masked_fill_(~allow[:, t.long()], float("-inf"))
        s.scatter_(1, ex, neg_inf)
        return torch.topk(s, k, dim=1)

    paths = {}
    for k in (10, 100):
        paths["topk k=%d plain" % k] = lambda k=k: eng.top_k(user, items, k, hist)
        for name, a in sets.items():
            paths["topk k=%d %s" % (k, name)] = lambda k=k, a=a: eng.top_k_tagged(user, items, k, tag, n_tags, a, hist)
        paths["topk k=%d 2 of 19 sorted by tag" % k] = lambda k=k: eng.top_k_tagged(user, items_so, k, tag_so, n_tags, sets["2 of 19"], hist_so)
        paths["topk k=%d torch mm+mask+scatter+topk half of 19" % k] = lambda k=k: torch_topk(k, tag, half, items, hist)
    for T in (1, 8):
        tg = torch.randint(0, N, (B, T), device=dev, generator=g)
        tg_so = inv[tg].contiguous()
        paths["rank T=%d plain" % T] = lambda tg=tg: eng.rank_of(user, items, tg, hist)
        for name, a in sets.items():
            paths["rank T=%d %s" % (T, name)] = lambda tg=tg, a=a: eng.rank_of_tagged(user, items, tg, tag, n_tags, a, hist)
        paths["rank T=%d 2 of 19 sorted by tag" % T] = lambda tg=tg_so: eng.rank_of_tagged(user, items_so, tg, tag_so, n_tags, sets["2 of 19"], hist_so)

    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
        fn()
    torch.cuda.synchronize()
    # what is timed is what it should be: all open is the plain list, sorted and shuffled catalogues agree, torch too
    a, b = eng.top_k(user, items, 10, hist), eng.top_k_tagged(user, items, 10, tag, n_tags, sets["all open"], hist)
    open_equal = bool(torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))
    s_ids = eng.top_k_tagged(user, items, 10, tag, n_tags, sets["2 of 19"], hist)[1]
    so_ids = eng.top_k_tagged(user, items_so, 10, tag_so, n_tags, sets["2 of 19"], hist_so)[1]
    sorted_equal = bool(torch.equal(s_ids, order[so_ids]))
    h_ids = eng.top_k_tagged(user, items, 10, tag, n_tags, sets["half of 19"], hist)[1]
    agree = float((h_ids == torch_topk(10, tag, half, items, hist).indices).float().mean())
    print("all open == plain call: %s; catalogue sorted by tag == shuffled: %s; top-10 ids equal to torch's in %.4f of the slots"
          % (open_equal, sorted_equal, agree))

    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, max(1, reps // 4) if "torch" in name else reps))
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "parity": "unpinned (the reference has no catalogue retrieval)",
           "B": B, "N": N, "d": d, "n_exclude": H, "n_tags": n_tags, "reps": reps, "windows": windows,
           "all_open_equals_plain": open_equal, "sorted_equals_shuffled": sorted_equal, "torch_top10_agreement": round(agree, 4),
           "ms": {}, "spread_ms": {}, "windows_ms": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-52s %8.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    rec["ratio"], rec["all_open_overhead"] = {}, {}
    for what in ("topk k=10", "topk k=100", "rank T=1", "rank T=8"):
        b0 = rec["ms"]["%s plain" % what]
        for name in ("all open", "half of 19", "2 of 19", "2 of 19 sorted by tag"):
            rec["ratio"]["%s %s / plain" % (what, name)] = round(rec["ms"]["%s %s" % (what, name)] / b0, 4)
            print("%-10s %-24s / plain = %.4f" % (what, name, rec["ratio"]["%s %s / plain" % (what, name)]))
        over = rec["ms"]["%s all open" % what] - b0
        rec["all_open_overhead"][what] = {"ms": round(over, 4), "plain_spread_ms": rec["spread_ms"]["%s plain" % what],
                                          "inside_plain_spread": bool(over <= rec["spread_ms"]["%s plain" % what])}
        print("%-10s all open - plain = %+.4f ms (the plain call's own spread: %.4f ms)" % (what, over, rec["spread_ms"]["%s plain" % what]))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
