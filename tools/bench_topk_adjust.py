"""Timing of the per-user score adjustments in retrieval and ranking at B = 512 users, N = 130 000 news,
d = 300, 50 excluded ids, k = 10 / 100, T = 1 / 8, in one process:
  (i)   nrms_topk_dot_adjusted / nrms_rank_dot_adjusted with every slot empty (E = 16, ids -1) beside this tree's plain nrms_topk_dot
        / nrms_rank_dot: the pure overhead (the slots read once per block, the extra barrier, the LDS list and mask rows).
  (ii)  E = 16 and E = 64 random slots per user: the staged path (the per-step scan of the block's list, the marks, the deltas read
        on a hit).
  (iii) E = 256 random slots per user: the longest lists.  At this geometry (16 user tiles x 16 slices) a block meets about 512 of
        its 8192 slots in its slice, so the list still fits in LDS; the global walk is what a block falls back to when more than
        2048 (k <= 192) or 1024 slots land in ONE slice, which random slots over 130 000 news do not do.  So the walk is timed on
        slots that all name one of the first 4096 rows: slow on purpose.
  (iv)  a torch restatement: mm, scatter_add_ of the deltas (distinct ids per user, so the add is the lowest-slot rule), scatter_
        of the excluded ids, topk.
Before timing, the tool checks that all-empty slots return the plain call's ids and score bits.  Device-event timing; every path is
warmed up first, the paths alternate, each window is `reps` calls and every window's time is kept: the record holds the minimum and
the spread (max - min over the windows) of every path, and the overhead of (i) beside the plain call's own spread.  This is a
record, not a gate.  Parity is unpinned: the reference has no catalogue retrieval.
Usage: python tools/bench_topk_adjust.py [B] [N] [reps] [--windows W] [--json FILE]"""
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
    d, H = 300, 50
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    user = torch.randn(B, d, device=dev, generator=g)
    items = torch.randn(N, d, device=dev, generator=g)
    hist = torch.randint(0, N, (B, H), device=dev, generator=g)
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)

    def slots(E):          # E distinct random rows per user, deltas of a few score standard deviations
        ids = torch.rand(B, N, device=dev, generator=g).topk(E, dim=1).indices.contiguous()
        return ids, (torch.randn(B, E, device=dev, generator=g) * 20.0).contiguous()

    sets = {"all empty (E=16)": (torch.full((B, 16), -1, dtype=torch.int64, device=dev), torch.ones(B, 16, device=dev)),
            "E=16": slots(16), "E=64": slots(64), "E=256": slots(256)}
    # every slot among the first 4096 rows: 8192 slots of a block in one slice overflow its LDS list, the block walks the global lists
    sets["E=256 in 4096 rows (global walk)"] = (torch.rand(B, 4096, device=dev, generator=g).topk(256, dim=1).indices.contiguous(),
                                                sets["E=256"][1])
    neg_inf = torch.full((B, H), float("-inf"), device=dev)

    def torch_topk(k, ids, delta, ex):
        s = torch.mm(user, items.T)
        s.scatter_add_(1, ids, delta)
        s.scatter_(1, ex, neg_inf)
        return torch.topk(s, k, dim=1)

    paths = {}
    for k in (10, 100):
        paths["topk k=%d plain" % k] = lambda k=k: eng.top_k(user, items, k, hist)
        for name, (a, dl) in sets.items():
            paths["topk k=%d %s" % (k, name)] = lambda k=k, a=a, dl=dl: eng.top_k_adjusted(user, items, k, a, dl, hist)
        paths["topk k=%d torch mm+scatter_add+scatter+topk E=64" % k] = lambda k=k: torch_topk(k, sets["E=64"][0], sets["E=64"][1], hist)
    for T in (1, 8):
        tg = torch.randint(0, N, (B, T), device=dev, generator=g)
        paths["rank T=%d plain" % T] = lambda tg=tg: eng.rank_of(user, items, tg, hist)
        for name, (a, dl) in sets.items():
            paths["rank T=%d %s" % (T, name)] = lambda tg=tg, a=a, dl=dl: eng.rank_of_adjusted(user, items, tg, a, dl, hist)

    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
        fn()
    torch.cuda.synchronize()
    # what is timed is what it should be: all-empty slots are the plain list, ids and score bits; torch agrees on E = 64
    empty = sets["all empty (E=16)"]
    empty_equal = True
    for k in (10, 100):
        a, b = eng.top_k(user, items, k, hist), eng.top_k_adjusted(user, items, k, empty[0], empty[1], hist)
        empty_equal = empty_equal and bool(torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))
    tg = torch.randint(0, N, (B, 8), device=dev, generator=g)
    a, b = eng.rank_of(user, items, tg, hist), eng.rank_of_adjusted(user, items, tg, empty[0], empty[1], hist)
    empty_equal = empty_equal and bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
    if not empty_equal:
        raise SystemExit("all-empty slots do not return the plain call's ids and score bits: nothing is timed")
    h_ids = eng.top_k_adjusted(user, items, 10, sets["E=64"][0], sets["E=64"][1], hist)[1]
    agree = float((h_ids == torch_topk(10, sets["E=64"][0], sets["E=64"][1], hist).indices).float().mean())
    moved = float((h_ids != eng.top_k(user, items, 10, hist)[1]).any(dim=1).float().mean())
    print("all-empty slots == plain call: %s; E=64 top-10 ids equal to torch's in %.4f of the slots; lists the slots change: %.4f"
          % (empty_equal, agree, moved))

    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, max(1, reps // 4) if "torch" in name else reps))
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "parity": "unpinned (the reference has no catalogue retrieval)",
           "B": B, "N": N, "d": d, "n_exclude": H, "reps": reps, "windows": windows,
           "all_empty_equals_plain": empty_equal, "torch_top10_agreement": round(agree, 4), "lists_changed_E64": round(moved, 4),
           "ms": {}, "spread_ms": {}, "windows_ms": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-56s %8.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    rec["ratio"], rec["all_empty_overhead"] = {}, {}
    for what in ("topk k=10", "topk k=100", "rank T=1", "rank T=8"):
        b0 = rec["ms"]["%s plain" % what]
        for name in sets:
            rec["ratio"]["%s %s / plain" % (what, name)] = round(rec["ms"]["%s %s" % (what, name)] / b0, 4)
            print("%-10s %-24s / plain = %.4f" % (what, name, rec["ratio"]["%s %s / plain" % (what, name)]))
        over = rec["ms"]["%s all empty (E=16)" % what] - b0
        rec["all_empty_overhead"][what] = {"ms": round(over, 4), "plain_spread_ms": rec["spread_ms"]["%s plain" % what],
                                           "inside_plain_spread": bool(abs(over) <= rec["spread_ms"]["%s plain" % what])}
        print("%-10s all empty - plain = %+.4f ms (the plain call's own spread: %.4f ms)" % (what, over, rec["spread_ms"]["%s plain" % what]))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
