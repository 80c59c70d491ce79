"""Timing of one request through several catalogue filters at once at B = 512 users, N = 130 000 news,
d = 300, 50 excluded ids, k = 10 / 100, T = 1 / 8, in one process:
  (1) nrms_topk_dot_request / nrms_rank_dot_request with a window (1/16 of a catalogue stored in time order, and the full window),
      19 tags of which every user allows half, and E = 16 and E = 64 random slots per user: the REQ kernels.
  (2) this tree's nrms_topk_dot_windowed, _tagged and _adjusted (and their rank forms) alone, on the same data: what each part costs
      by itself.
  (3) a torch restatement: mm, the time mask, the tag mask, scatter_add_ of the deltas (distinct ids per user, so the add is the
      lowest-slot rule), scatter_ of the excluded ids, topk.
  (4) the single-part requests, which forward to the calls of (2) and must therefore sit inside those calls' own spread.
Before timing, the tool checks that the request's top-10 ids agree with torch's and that a forwarded request returns its part's
bytes.  Device-event timing; every path is warmed up first, the paths alternate, each window is `reps` calls and every window's time
is kept: the record holds the minimum and the spread (max - min over the windows) of every path, the combined call beside the
slowest single part with that part's spread, and each forwarded request beside its part.  This is a record, not a gate.  Parity is
unpinned: the reference has no catalogue retrieval.
Usage: python tools/bench_topk_request.py [B] [N] [reps] [--windows W] [--json FILE]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


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

    # the catalogue in time order: item n was published at tick n; the requests in time order too
    item_time = torch.arange(N, dtype=torch.int32, device=dev)
    span = N // 16
    lo = torch.randint(0, N - span + 1, (B,), device=dev, generator=g).sort().values
    wins = {"1/16": torch.stack([lo, lo + span], dim=1).to(torch.int32).contiguous(),
            "full": torch.tensor([[I32_MIN, I32_MAX]], dtype=torch.int64).expand(B, 2).to(torch.int32).to(dev).contiguous()}
    item_tag = torch.randint(0, n_tags, (N,), device=dev, generator=g).to(torch.int32)
    allow = torch.rand(B, n_tags, device=dev, generator=g) < 0.5

    def slots(E):          # E distinct random rows per user, deltas of a few score standard deviations
        ids = torch.rand(B, N, device=dev, generator=g).topk(E, dim=1).indices.contiguous()
        return ids, (torch.randn(B, E, device=dev, generator=g) * 20.0).contiguous()

    adj = {"E=16": slots(16), "E=64": slots(64)}
    neg_inf = torch.full((B, H), float("-inf"), device=dev)

    def torch_topk(k, w, a, dl):
        s = torch.mm(user, items.T)
        t = item_time.unsqueeze(0)
        s.masked_fill_(~((t >= w[:, :1]) & (t < w[:, 1:])), float("-inf"))
        s.masked_fill_(~allow[:, item_tag.long()], float("-inf"))
        s.scatter_add_(1, a, dl)
        s.scatter_(1, hist, neg_inf)
        return torch.topk(s, k, dim=1)

    tag_kw = dict(item_tag=item_tag, n_tags=n_tags, allow=allow)
    paths, single_of = {}, {}
    for what, sizes in (("topk", (10, 100)), ("rank", (1, 8))):
        for size in sizes:
            tg = torch.randint(0, N, (B, size), device=dev, generator=g)
            if what == "topk":
                head = "topk k=%d" % size
                req = lambda size=size, tg=tg, **kw: eng.top_k_request(user, items, size, hist, **kw)
                own = {"window": lambda w, size=size: eng.top_k(user, items, size, hist, item_time=item_time, window=w),
                       "tags": lambda size=size: eng.top_k_tagged(user, items, size, item_tag, n_tags, allow, hist),
                       "adjust": lambda a, dl, size=size: eng.top_k_adjusted(user, items, size, a, dl, hist)}
            else:
                head = "rank T=%d" % size
                req = lambda size=size, tg=tg, **kw: eng.rank_of_request(user, items, tg, hist, **kw)
                own = {"window": lambda w, tg=tg: eng.rank_of(user, items, tg, hist, item_time=item_time, window=w),
                       "tags": lambda tg=tg: eng.rank_of_tagged(user, items, tg, item_tag, n_tags, allow, hist),
                       "adjust": lambda a, dl, tg=tg: eng.rank_of_adjusted(user, items, tg, a, dl, hist)}
            for wn, w in wins.items():
                paths["%s windowed %s" % (head, wn)] = lambda w=w, own=own: own["window"](w)
                paths["%s request window %s only" % (head, wn)] = lambda w=w, req=req: req(item_time=item_time, window=w)
                single_of["%s request window %s only" % (head, wn)] = "%s windowed %s" % (head, wn)
            paths["%s tagged" % head] = lambda own=own: own["tags"]()
            paths["%s request tags only" % head] = lambda req=req: req(**tag_kw)
            single_of["%s request tags only" % head] = "%s tagged" % head
            for en, (a, dl) in adj.items():
                paths["%s adjusted %s" % (head, en)] = lambda a=a, dl=dl, own=own: own["adjust"](a, dl)
                paths["%s request adjust %s only" % (head, en)] = lambda a=a, dl=dl, req=req: req(adj_ids=a, adj_delta=dl)
                single_of["%s request adjust %s only" % (head, en)] = "%s adjusted %s" % (head, en)
            for wn, w in wins.items():
                for en, (a, dl) in adj.items():
                    paths["%s request window %s + tags + %s" % (head, wn, en)] = (
                        lambda w=w, a=a, dl=dl, req=req: req(item_time=item_time, window=w, adj_ids=a, adj_delta=dl, **tag_kw))
            if what == "topk":
                a, dl = adj["E=64"]
                paths["%s torch mm+masks+scatter_add+scatter+topk window 1/16 E=64" % head] = (
                    lambda size=size, a=a, dl=dl: torch_topk(size, wins["1/16"], a, dl))

    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
        fn()
    torch.cuda.synchronize()
    # what is timed is what it should be: the request agrees with torch, a forwarded request is its part's call
    a, dl = adj["E=64"]
    r_ids = eng.top_k_request(user, items, 10, hist, item_time=item_time, window=wins["1/16"], adj_ids=a, adj_delta=dl, **tag_kw)[1]
    agree = float((r_ids == torch_topk(10, wins["1/16"], a, dl).indices).float().mean())
    fwd_equal = True
    for name, single in single_of.items():
        x, y = paths[name](), paths[single]()
        fwd_equal = fwd_equal and all(bool(torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p,
                                                       q.view(torch.int32) if q.dtype == torch.float32 else q)) for p, q in zip(x, y))
    if not fwd_equal:
        raise SystemExit("a single-part request does not return its part's ids and score bits: nothing is timed")
    print("single-part requests == their parts' calls: %s; request top-10 ids equal to torch's in %.4f of the slots" % (fwd_equal, agree))

    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, max(1, reps // 4) if "torch" in name else reps))
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "parity": "unpinned (the reference has no catalogue retrieval)",
           "B": B, "N": N, "d": d, "n_exclude": H, "n_tags": n_tags, "reps": reps, "windows": windows,
           "forwarded_equals_part": fwd_equal, "torch_top10_agreement": round(agree, 4), "ms": {}, "spread_ms": {}, "windows_ms": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-72s %8.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    rec["forwarded"], rec["combined"] = {}, {}
    for name, single in single_of.items():
        over = rec["ms"][name] - rec["ms"][single]
        rec["forwarded"][name] = {"ms_over_part": round(over, 4), "part_spread_ms": rec["spread_ms"][single],
                                  "inside_part_spread": bool(abs(over) <= rec["spread_ms"][single])}
        print("%-72s - its part = %+.4f ms (the part's own spread: %.4f ms)" % (name, over, rec["spread_ms"][single]))
    for name in paths:
        if " + tags + " not in name:
            continue
        head = " ".join(name.split(" ")[:2])
        wn, en = name.split("window ")[1].split(" ")[0], name.rsplit(" ", 1)[1]
        parts = ["%s windowed %s" % (head, wn), "%s tagged" % head, "%s adjusted %s" % (head, en)]
        slowest = max(parts, key=lambda p: rec["ms"][p])
        over = rec["ms"][name] - rec["ms"][slowest]
        rec["combined"][name] = {"slowest_part": slowest, "slowest_part_ms": rec["ms"][slowest], "ms_over_slowest_part": round(over, 4),
                                 "slowest_part_spread_ms": rec["spread_ms"][slowest],
                                 "slower_than_slowest_part": bool(over > rec["spread_ms"][slowest]),
                                 "ratio_to_slowest_part": round(rec["ms"][name] / rec["ms"][slowest], 4)}
        print("%-72s / %-28s = %.4f (%+.4f ms; that part's spread: %.4f ms)"
              % (name, slowest, rec["ms"][name] / rec["ms"][slowest], over, rec["spread_ms"][slowest]))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
