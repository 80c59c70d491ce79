"""Timing of per-category caps through the request at B = 512 users, N = 130 000 news, d = 300, 50 excluded
ids, 19 Zipf-sized tags, k = 10 (cap 2) and k = 100 (cap 10), in one process:
  (1) nrms_topk_dot_request_capped with every cap >= k beside nrms_topk_dot_request with the same window and slots (whose device code
      is the parent commit's: profiles/topk_request_caps_compare_parent.json): what the REQ + CAPS kernel form costs when nothing is
      rationed.
  (2) the capped request with no other part beside nrms_topk_dot_capped: the routed path, the same bytes and the same time.
  (3) cap = 2 at k = 10 and cap = 10 at k = 100 with a window of 1/16 of a catalogue stored in time order and E = 16 slots, and
      with the full window and E = 64 slots: rationing.
  (4) a page-2 call: the cursor after page 1 and the caps that remaining_caps leaves.
  (5) a torch restatement: mm, the time mask, scatter_add_ of the deltas, scatter_ of the excluded ids, then per tag the best `cap`
      (topk of the tag's masked scores) and the best k of their union, which is the greedy walk's list when every tag has one cap.
Before timing, the tool checks that the routed call returns nrms_topk_dot_capped's bytes, that the uncapped call returns the
request's bytes (both abort the run on a mismatch) and reports the share of rationed ids equal to torch's, which is informational:
torch sums a score in another order, so two news a rounding apart may swap.  Device-event timing; every path is warmed up first, the paths
alternate, each window is `reps` calls and every window's time is kept: the record holds the minimum and the spread (max - min over
the windows) of every path.  This is a record, not a gate.  Parity is unpinned: the reference has no catalogue retrieval.
Usage: python tools/bench_topk_request_caps.py [B] [N] [reps] [--windows W] [--json FILE]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, remaining_caps

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


def same_bits(x, y):
    return all(bool(torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p, q.view(torch.int32) if q.dtype == torch.float32 else q))
               for p, q in zip(x, y))


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

    item_time = torch.arange(N, dtype=torch.int32, device=dev)           # the catalogue in time order
    span = N // 16
    lo = torch.randint(0, N - span + 1, (B,), device=dev, generator=g).sort().values
    wins = {"1/16": torch.stack([lo, lo + span], dim=1).to(torch.int32).contiguous(),
            "full": torch.tensor([[I32_MIN, I32_MAX]], dtype=torch.int64).expand(B, 2).to(torch.int32).to(dev).contiguous()}
    zipf = 1.0 / torch.arange(1, n_tags + 1, dtype=torch.float64, device=dev)        # tag t holds a share ~ 1 / (t + 1) of the news
    item_tag = torch.multinomial(zipf / zipf.sum(), N, replacement=True, generator=g).to(torch.int32)

    def slots(E):          # E distinct random rows per user, deltas of a few score standard deviations
        ids = torch.rand(B, N, device=dev, generator=g).topk(E, dim=1).indices.contiguous()
        return ids, (torch.randn(B, E, device=dev, generator=g) * 20.0).contiguous()

    settings = {"window 1/16 + E=16": (wins["1/16"], slots(16)), "full window + E=64": (wins["full"], slots(64))}
    neg_inf = torch.full((B, H), float("-inf"), device=dev)
    tag_long = item_tag.long()

    def torch_capped(k, cap, w, a, dl):
        s = torch.mm(user, items.T)
        t = item_time.unsqueeze(0)
        s.masked_fill_(~((t >= w[:, :1]) & (t < w[:, 1:])), float("-inf"))
        s.scatter_add_(1, a, dl)
        s.scatter_(1, hist, neg_inf)
        best_s, best_i = [], []
        for tag in range(n_tags):
            v, i = torch.topk(s.masked_fill(tag_long.unsqueeze(0) != tag, float("-inf")), cap, dim=1)
            best_s.append(v)
            best_i.append(i)
        best_s, best_i = torch.cat(best_s, dim=1), torch.cat(best_i, dim=1)
        best_i = torch.where(best_s == float("-inf"), torch.full_like(best_i, -1), best_i)      # a tag with fewer than cap live news
        # the kernels' order: the score, then the smaller id
        order = torch.argsort(best_i, dim=1, stable=True)
        best_s, best_i = best_s.gather(1, order), best_i.gather(1, order)
        order = torch.argsort(best_s, dim=1, descending=True, stable=True)[:, :k]
        return best_s.gather(1, order), best_i.gather(1, order)          # (-inf slots carry id -1, like the kernels' padding)

    paths, pairs = {}, {}
    caps_of = {10: 2, 100: 10}
    for k, c in caps_of.items():
        head = "k=%d" % k
        free = torch.full((B, n_tags), k, dtype=torch.int32, device=dev)
        cap = torch.full((B, n_tags), c, dtype=torch.int32, device=dev)
        paths["%s capped (nrms_topk_dot_capped) cap=%d" % (head, c)] = lambda k=k, cap=cap: eng.top_k_capped(user, items, k, item_tag, n_tags, cap, hist)
        paths["%s capped request, no other part, cap=%d" % (head, c)] = (
            lambda k=k, cap=cap: eng.top_k_request_capped(user, items, k, item_tag, n_tags, cap, hist))
        pairs["%s capped request, no other part, cap=%d" % (head, c)] = "%s capped (nrms_topk_dot_capped) cap=%d" % (head, c)
        for name, (w, (a, dl)) in settings.items():
            kw = dict(item_time=item_time, window=w, adj_ids=a, adj_delta=dl)
            paths["%s request %s" % (head, name)] = lambda k=k, kw=kw: eng.top_k_request(user, items, k, hist, **kw)
            paths["%s capped request %s every cap=k" % (head, name)] = (
                lambda k=k, kw=kw, free=free: eng.top_k_request_capped(user, items, k, item_tag, n_tags, free, hist, **kw))
            pairs["%s capped request %s every cap=k" % (head, name)] = "%s request %s" % (head, name)
            paths["%s capped request %s cap=%d" % (head, name, c)] = (
                lambda k=k, kw=kw, cap=cap: eng.top_k_request_capped(user, items, k, item_tag, n_tags, cap, hist, **kw))
            pairs["%s capped request %s cap=%d" % (head, name, c)] = "%s request %s" % (head, name)
        w, (a, dl) = settings["window 1/16 + E=16"]
        kw = dict(item_time=item_time, window=w, adj_ids=a, adj_delta=dl)
        s1, i1 = eng.top_k_request_capped(user, items, k, item_tag, n_tags, cap, hist, **kw)
        left = remaining_caps(cap, i1, item_tag, n_tags)
        a_s, a_i = s1[:, -1].contiguous(), i1[:, -1].contiguous()
        paths["%s capped request window 1/16 + E=16 cap=%d page 2" % (head, c)] = (
            lambda k=k, kw=kw, left=left, a_s=a_s, a_i=a_i: eng.top_k_request_capped(user, items, k, item_tag, n_tags, left, hist,
                                                                                      after_scores=a_s, after_ids=a_i, **kw))
        pairs["%s capped request window 1/16 + E=16 cap=%d page 2" % (head, c)] = "%s capped request window 1/16 + E=16 cap=%d" % (head, c)
        paths["%s torch mm+masks+scatter_add+scatter+per-tag topk+topk window 1/16 + E=16 cap=%d" % (head, c)] = (
            lambda k=k, c=c, w=w, a=a, dl=dl: torch_capped(k, c, w, a, dl))

    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
        fn()
    torch.cuda.synchronize()
    # what is timed is what it should be
    routed_equal = uncapped_equal = True
    agree = {}
    for k, c in caps_of.items():
        head = "k=%d" % k
        routed_equal = routed_equal and same_bits(paths["%s capped request, no other part, cap=%d" % (head, c)](),
                                                  paths["%s capped (nrms_topk_dot_capped) cap=%d" % (head, c)]())
        for name in settings:
            uncapped_equal = uncapped_equal and same_bits(paths["%s capped request %s every cap=k" % (head, name)](),
                                                          paths["%s request %s" % (head, name)]())
        ours = paths["%s capped request window 1/16 + E=16 cap=%d" % (head, c)]()[1]
        theirs = paths["%s torch mm+masks+scatter_add+scatter+per-tag topk+topk window 1/16 + E=16 cap=%d" % (head, c)]()[1]
        agree[head] = round(float((ours == theirs).float().mean()), 4)
    if not (routed_equal and uncapped_equal):
        raise SystemExit("routed == capped: %s, uncapped == request: %s: nothing is timed" % (routed_equal, uncapped_equal))
    print("routed call == nrms_topk_dot_capped: %s; every cap = k == nrms_topk_dot_request: %s; rationed ids equal to torch's: %s"
          % (routed_equal, uncapped_equal, agree))

    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, max(1, reps // 4) if "torch" in name else reps))
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "parity": "unpinned (the reference has no catalogue retrieval)",
           "B": B, "N": N, "d": d, "n_exclude": H, "n_tags": n_tags, "tag_sizes": "Zipf, share ~ 1 / (t + 1)", "reps": reps, "windows": windows,
           "routed_equals_capped": routed_equal, "uncapped_equals_request": uncapped_equal, "torch_ids_agreement": agree,
           "ms": {}, "spread_ms": {}, "windows_ms": {}, "ratios": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-92s %8.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    for name, base in pairs.items():
        over = rec["ms"][name] - rec["ms"][base]
        rec["ratios"][name] = {"beside": base, "beside_ms": rec["ms"][base], "ms_over": round(over, 4), "beside_spread_ms": rec["spread_ms"][base],
                               "ratio": round(rec["ms"][name] / rec["ms"][base], 4)}
        print("%-92s / %-44s = %.4f (%+.4f ms; its spread: %.4f ms)" % (name, base, rec["ms"][name] / rec["ms"][base], over, rec["spread_ms"][base]))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
