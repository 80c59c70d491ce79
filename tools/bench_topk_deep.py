"""Timing of paging through the exact ranking at B = 512 users, N = 130 000 news, d = 300, 50 excluded ids, in
one process:
  (i)   nrms_topk_dot_after with every cursor at BEGIN, at k = 10 / 100 / 256, beside the uncursored nrms_topk_dot: what the cursor's
        compare costs on a single page.  With --parent_lib FILE (a libnrms_hip.so built from the parent commit) the uncursored calls
        are made into THAT library, in the same session; without it, into this tree's.
  (ii)  nrms_topk_dot_deep at K = 256 / 512 / 1024 / 4096: ceil(K / 256) pages chained on the device.
  (iii) a torch restatement at the same K: mm, scatter_ of the excluded ids, topk(K).
Device-event timing; every path is warmed up first, the paths alternate, each window is `reps` calls and every window's time is
kept: the record holds the minimum and the spread (max - min over the windows) of every path.  This is a record, not a gate.
Usage: python tools/bench_topk_deep.py [B] [N] [reps] [--windows W] [--parent_lib FILE] [--json FILE]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_topk_window import event_ms, opt, parent_calls
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine

KS = (10, 100, 256)
DEEP = (256, 512, 1024, 4096)


def main():
    argv = list(sys.argv[1:])
    out = opt(argv, "--json", None, str)
    parent_lib = opt(argv, "--parent_lib", None, str)
    windows = opt(argv, "--windows", 5, int)
    B = int(argv[0]) if len(argv) > 0 else 512
    N = int(argv[1]) if len(argv) > 1 else 130000
    reps = int(argv[2]) if len(argv) > 2 else 20
    d, H = 300, 50
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    user = torch.randn(B, d, device=dev, generator=g)
    items = torch.randn(N, d, device=dev, generator=g)
    hist = torch.randint(0, N, (B, H), device=dev, generator=g)
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)
    base_topk = lambda u, i, k, ex: eng.top_k(u, i, k, ex)          # noqa: E731
    if parent_lib:
        base_topk = parent_calls(parent_lib, dev)[0]
    base = "parent" if parent_lib else "uncursored"
    a_s = torch.zeros(B, device=dev)
    a_i = torch.full((B,), -2, dtype=torch.int64, device=dev)
    neg_inf = torch.full((B, H), float("-inf"), device=dev)

    def torch_topk(K):
        s = torch.mm(user, items.T)
        s.scatter_(1, hist, neg_inf)
        return torch.topk(s, K, dim=1)

    paths = {}
    for k in KS:
        paths["topk k=%d %s" % (k, base)] = lambda k=k: base_topk(user, items, k, hist)
        paths["after k=%d all BEGIN" % k] = lambda k=k: eng.top_k_after(user, items, k, a_s, a_i, hist)
    for K in DEEP:
        paths["deep K=%d" % K] = lambda K=K: eng.top_k_deep(user, items, K, hist)
        paths["torch mm+scatter+topk K=%d" % K] = lambda K=K: torch_topk(K)

    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
        fn()
    torch.cuda.synchronize()
    # what is timed is what it should be: all-BEGIN is the baseline's list, the deep list starts with it and agrees with torch's
    same = lambda a, b: bool(torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))      # noqa: E731
    begin_equal = all(same(base_topk(user, items, k, hist), eng.top_k_after(user, items, k, a_s, a_i, hist)) for k in KS)
    deep = eng.top_k_deep(user, items, 4096, hist)
    first = base_topk(user, items, 256, hist)
    deep_prefix = same((deep[0][:, :256], deep[1][:, :256]), first)
    agree = float((deep[1] == torch_topk(4096).indices).float().mean())
    print("all-BEGIN == %s call: %s; deep(4096)[:, :256] == %s call at k = 256: %s; deep ids equal to torch's in %.4f of the slots"
          % (base, begin_equal, base, deep_prefix, agree))

    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, max(1, reps // 4) if ("torch" in name or "deep" in name) else reps))
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "B": B, "N": N, "d": d, "n_exclude": H,
           "reps": reps, "windows": windows, "baseline": base, "all_begin_equals_baseline": begin_equal,
           "deep_prefix_equals_baseline": deep_prefix, "torch_top4096_agreement": round(agree, 4), "ms": {}, "spread_ms": {},
           "windows_ms": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-40s %8.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    rec["ratio"] = {}
    for k in KS:
        b0 = rec["ms"]["topk k=%d %s" % (k, base)]
        key = "after k=%d all BEGIN / %s" % (k, base)
        rec["ratio"][key] = round(rec["ms"]["after k=%d all BEGIN" % k] / b0, 4)
        # the cursor's cost on a single page against the baseline's own window-to-window spread
        rec["ratio"]["after k=%d all BEGIN - %s, ms" % (k, base)] = round(rec["ms"]["after k=%d all BEGIN" % k] - b0, 4)
        print("%-40s = %.4f  (difference %.4f ms, %s spread %.4f ms)" % (key, rec["ratio"][key], rec["ms"]["after k=%d all BEGIN" % k] - b0,
                                                                      base, rec["spread_ms"]["topk k=%d %s" % (k, base)]))
    page = rec["ms"]["topk k=256 %s" % base]
    for K in DEEP:
        pages = -(-K // 256)
        rec["ratio"]["deep K=%d / (%d x topk k=256 %s)" % (K, pages, base)] = round(rec["ms"]["deep K=%d" % K] / (pages * page), 4)
        rec["ratio"]["deep K=%d / torch" % K] = round(rec["ms"]["deep K=%d" % K] / rec["ms"]["torch mm+scatter+topk K=%d" % K], 4)
        print("deep K=%-5d / (%2d x topk k=256 %s) = %.4f   / torch = %.4f" % (K, pages, base, rec["ratio"]["deep K=%d / (%d x topk k=256 %s)" % (K, pages, base)],
                                                                             rec["ratio"]["deep K=%d / torch" % K]))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
