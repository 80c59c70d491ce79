"""Timing of the per-category caps in retrieval at B = 512 users, N = 130 000 news, d = 300, 50 excluded ids,
19 Zipf-sized tags, k = 10 / 100, in one process.  Items are their tag's centroid plus unit noise, so a user aligned with one
centroid ranks that tag's news first.
  (i)   nrms_topk_dot_capped with every cap >= k beside this tree's plain nrms_topk_dot and nrms_topk_dot_tagged (all open): what the
        capped flush costs when it rations nothing.
  (ii)  cap = 2 at k = 10 and cap = 10 at k = 100, on Gaussian users and on users aligned with one tag's centroid (the entries that
        end up capped out flood the buffers).
  (iii) cap = 2 at k = 100: sum(cap) = 38 < k, the threshold only rises once every tag is saturated.
  (iv)  three restatements of the same list: nrms_topk_sections_dot (k = cap) over the catalogue re-laid-out by tag + torch topk over
        [B, G cap] (the re-layout timed apart); nrms_topk_dot_deep (K = 256) + a torch greedy filter, with the share of rows it
        leaves short of the exact list; torch mm + scatter_ + two sorts (a per-tag rank) + mask + topk.
Device-event timing; every path is warmed up first, the paths alternate, each window is `reps` calls and every window's time is
kept: the record holds the minimum and the spread (max - min over the windows) of every path.  This is a record, not a gate: the
comparison is written down whichever way it falls.  Parity is unpinned: the reference has no catalogue retrieval.
Usage: python tools/bench_topk_caps.py [B] [N] [reps] [--windows W] [--json FILE]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine


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
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)

    zipf = 1.0 / torch.arange(1, n_tags + 1, dtype=torch.float64, device=dev)
    tag = torch.multinomial(zipf / zipf.sum(), N, replacement=True, generator=g).to(torch.int32)        # tags in random row order
    centroid = torch.randn(n_tags, d, device=dev, generator=g)
    items = (centroid[tag.long()] + torch.randn(N, d, device=dev, generator=g)).contiguous()
    users = {"gaussian": torch.randn(B, d, device=dev, generator=g),
             "aligned": (centroid[torch.randint(0, n_tags, (B,), device=dev, generator=g)]
                         + 0.1 * torch.randn(B, d, device=dev, generator=g)).contiguous()}
    hist = torch.randint(0, N, (B, H), device=dev, generator=g)
    neg_inf = torch.full((B, H), float("-inf"), device=dev)
    every = torch.ones(B, n_tags, dtype=torch.bool, device=dev)
    caps = lambda c: torch.full((B, n_tags), c, dtype=torch.int32, device=dev)
    tag_l = tag.long()

    # the catalogue re-laid-out section after section, for nrms_topk_sections_dot
    def relayout():
        order = torch.argsort(tag_l, stable=True)
        ptr = torch.zeros(n_tags + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.bincount(tag_l, minlength=n_tags).cumsum(0)
        return items[order].contiguous(), order.to(torch.int32).contiguous(), ptr
    items_so, ids_so, ptr = relayout()

    def by_sections(user, k, cap):
        sc, ids = eng.top_k_sections(user, items_so, ids_so, ptr, cap, hist)
        top = torch.topk(sc.reshape(B, -1), min(k, n_tags * cap), dim=1)
        return top.values, ids.reshape(B, -1).gather(1, top.indices)

    def by_deep(user, k, cap):
        sc, ids = eng.top_k_deep(user, items, 256, hist)
        t = tag_l[ids.clamp(min=0)]
        oh = torch.nn.functional.one_hot(t, n_tags) * (ids >= 0).unsqueeze(2)
        keep = ((oh.cumsum(1) * oh).sum(2) <= cap) & (ids >= 0)
        place = keep.cumsum(1)
        keep &= place <= k
        res = torch.full((B, k + 1), -1, dtype=torch.int64, device=dev)
        res.scatter_(1, torch.where(keep, place - 1, torch.full_like(place, k)), ids)
        return res[:, :k]

    def by_torch(user, k, cap):
        s = torch.mm(user, items.T)
        s.scatter_(1, hist, neg_inf)
        order = torch.argsort(s, dim=1, descending=True, stable=True)
        t = tag_l[order]
        by_tag = torch.argsort(t, dim=1, stable=True)                 # positions of the score order, tag after tag, best first
        start = torch.zeros(B, n_tags + 1, dtype=torch.int64, device=dev)
        start[:, 1:] = torch.zeros(B, n_tags, dtype=torch.int64, device=dev).scatter_add_(1, t, torch.ones_like(t)).cumsum(1)
        rank = torch.arange(N, device=dev).expand(B, N) - start.gather(1, t.gather(1, by_tag))
        capped_out = torch.zeros(B, N, dtype=torch.bool, device=dev).scatter_(1, order.gather(1, by_tag), rank >= cap)
        s.masked_fill_(capped_out, float("-inf"))
        return torch.topk(s, k, dim=1)

    paths, heavy = {}, set()
    for k, cap in ((10, 2), (100, 10)):
        u = users["gaussian"]
        paths["k=%d plain" % k] = lambda k=k, u=u: eng.top_k(u, items, k, hist)
        paths["k=%d tagged all open" % k] = lambda k=k, u=u: eng.top_k_tagged(u, items, k, tag, n_tags, every, hist)
        paths["k=%d capped cap>=k" % k] = lambda k=k, u=u, c=caps(k): eng.top_k_capped(u, items, k, tag, n_tags, c, hist)
        for who, u in users.items():
            paths["k=%d capped cap=%d %s" % (k, cap, who)] = lambda k=k, u=u, c=caps(cap): eng.top_k_capped(u, items, k, tag, n_tags, c, hist)
            paths["k=%d plain %s" % (k, who)] = lambda k=k, u=u: eng.top_k(u, items, k, hist)
            paths["k=%d cap=%d sections+topk %s" % (k, cap, who)] = lambda k=k, u=u, cap=cap: by_sections(u, k, cap)
            paths["k=%d cap=%d deep256+greedy %s" % (k, cap, who)] = lambda k=k, u=u, cap=cap: by_deep(u, k, cap)
        paths["k=%d cap=%d torch mm+sorts+topk gaussian" % (k, cap)] = lambda k=k, cap=cap: by_torch(users["gaussian"], k, cap)
        heavy.add("k=%d cap=%d torch mm+sorts+topk gaussian" % (k, cap))
    for who, u in users.items():
        paths["k=100 capped cap=2 (sum(cap)=38<k) %s" % who] = lambda u=u, c=caps(2): eng.top_k_capped(u, items, 100, tag, n_tags, c, hist)
    paths["re-layout by tag (argsort, gather, bincount)"] = relayout
    heavy.add("re-layout by tag (argsort, gather, bincount)")

    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
        fn()
    torch.cuda.synchronize()

    # what is timed is what it should be
    checks = {}
    a = eng.top_k(users["gaussian"], items, 10, hist)
    b = eng.top_k_capped(users["gaussian"], items, 10, tag, n_tags, caps(10), hist)
    checks["uncapped_equals_plain"] = bool(torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))
    for k, cap in ((10, 2), (100, 10)):
        for who, u in users.items():
            sc, ids = eng.top_k_capped(u, items, k, tag, n_tags, caps(cap), hist)
            s_sc, s_ids = by_sections(u, k, cap)
            kk = s_ids.shape[1]
            checks["k=%d cap=%d %s sections ids equal" % (k, cap, who)] = round(float((ids[:, :kk] == s_ids).float().mean()), 6)
            d_ids = by_deep(u, k, cap)
            short = ((d_ids >= 0).sum(1) < (ids >= 0).sum(1)).float().mean()
            wrong = ((d_ids != ids).any(1)).float().mean()
            checks["k=%d cap=%d %s deep256 rows short" % (k, cap, who)] = round(float(short), 6)
            checks["k=%d cap=%d %s deep256 rows differing" % (k, cap, who)] = round(float(wrong), 6)
            checks["k=%d cap=%d %s largest tag share capped / plain" % (k, cap, who)] = [
                round(float(torch.nn.functional.one_hot(tag_l[x.clamp(min=0)], n_tags).sum(1).max(1).values.float().mean()) / k, 4)
                for x in (ids, eng.top_k(u, items, k, hist)[1])]
        t_ids = by_torch(users["gaussian"], k, cap).indices
        ids = eng.top_k_capped(users["gaussian"], items, k, tag, n_tags, caps(cap), hist)[1]
        checks["k=%d cap=%d gaussian torch ids equal" % (k, cap)] = round(float((ids == t_ids).float().mean()), 6)
    for name, v in checks.items():
        print("%-60s %s" % (name, v))

    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, max(1, reps // 10) if name in heavy else reps))
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "parity": "unpinned (the reference has no catalogue retrieval)",
           "B": B, "N": N, "d": d, "n_exclude": H, "n_tags": n_tags, "tag_sizes": torch.bincount(tag_l, minlength=n_tags).tolist(),
           "reps": reps, "windows": windows, "checks": checks, "ms": {}, "spread_ms": {}, "windows_ms": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-60s %9.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    rec["ratio"] = {}
    for k, cap in ((10, 2), (100, 10)):
        b0 = rec["ms"]["k=%d plain" % k]
        for name in ("tagged all open", "capped cap>=k"):
            rec["ratio"]["k=%d %s / plain" % (k, name)] = round(rec["ms"]["k=%d %s" % (k, name)] / b0, 4)
        over = rec["ms"]["k=%d capped cap>=k" % k] - b0
        rec["ratio"]["k=%d capped cap>=k - plain, ms (plain spread %.4f)" % (k, rec["spread_ms"]["k=%d plain" % k])] = round(over, 4)
        for who in users:
            c0 = rec["ms"]["k=%d capped cap=%d %s" % (k, cap, who)]
            rec["ratio"]["k=%d cap=%d %s capped / plain" % (k, cap, who)] = round(c0 / rec["ms"]["k=%d plain %s" % (k, who)], 4)
            for other in ("sections+topk", "deep256+greedy"):
                rec["ratio"]["k=%d cap=%d %s %s / capped" % (k, cap, who, other)] = round(rec["ms"]["k=%d cap=%d %s %s" % (k, cap, other, who)] / c0, 4)
        rec["ratio"]["k=%d cap=%d gaussian torch / capped" % (k, cap)] = round(
            rec["ms"]["k=%d cap=%d torch mm+sorts+topk gaussian" % (k, cap)] / rec["ms"]["k=%d capped cap=%d gaussian" % (k, cap)], 4)
    for who in users:
        rec["ratio"]["k=100 cap=2 %s capped / plain" % who] = round(
            rec["ms"]["k=100 capped cap=2 (sum(cap)=38<k) %s" % who] / rec["ms"]["k=100 plain %s" % who], 4)
    for name, v in rec["ratio"].items():
        print("%-72s %s" % (name, v))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
