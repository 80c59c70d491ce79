"""Timing of the sectioned front page: nrms_topk_sections_dot beside what a caller could do without it, at
B = 512 users, N = 130 000 news, d = 300, 50 excluded ids, k = 10 / 100, Zipf-skewed section sizes at G = 18 (MIND's categories)
and G = 270 (its sub-categories), in one process.  Per (G, k) four paths:
  (a) sections     one nrms_topk_sections_dot call;
  (b) per-range    G calls of nrms_topk_dot, one per section's contiguous row range (exclude lists mapped to the range's rows
                   beforehand, outside the timing): the strongest thing a caller can do without the new call;
  (c) nan-mask     G calls of nrms_topk_dot_biased over the whole catalogue with a NaN mask per section: what
                   recommend(item_bias=...) offers;
  (d) plain        one nrms_topk_dot at the same k: the floor, the same flops with one selection.
Device-event timing; every path is warmed up first, the paths alternate, each window is `reps` calls ((b) and (c) at G = 270
fewer, they are G calls each) and every window's time is kept: the record holds the minimum and the spread (max - min over the
windows) of every path.

The bar: at G = 18, k = 10 the minimum of (a) lies below the minimum of (b) by more than the larger of the two spreads.  (a) / (d)
is reported as a ratio, without a gate.
Usage: python tools/bench_topk_sections.py [B] [N] [reps] [--windows W] [--json FILE]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
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


def skewed_sections(N, G, seed=0):
    """Zipf-skewed section sizes that sum to N (a few large sections, a long tail of small and empty ones)."""
    rng = np.random.default_rng(seed)
    w = rng.zipf(1.6, size=G).astype(np.float64)
    sizes = np.floor(w / w.sum() * N).astype(np.int64)
    sizes[np.argmax(sizes)] += N - sizes.sum()
    return np.concatenate([[0], np.cumsum(sizes)])


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
    ids = torch.arange(N, device=dev, dtype=torch.int32)
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)

    paths, path_reps, sizes_of = {}, {}, {}
    for G in (18, 270):
        ptr_host = skewed_sections(N, G)
        ptr = torch.as_tensor(ptr_host, device=dev)
        live = [(int(lo), int(hi)) for lo, hi in zip(ptr_host[:-1], ptr_host[1:]) if hi > lo]
        sizes_of[G] = {"nonempty": len(live), "largest": int(np.diff(ptr_host).max()), "median": int(np.median(np.diff(ptr_host)))}
        parts = [items[lo:hi].contiguous() for lo, hi in live]
        # (b)'s exclude lists in each range's row numbering; ids outside the range fall out of [0, hi - lo) and are ignored
        part_ex = [(hist - lo).contiguous() for lo, hi in live]
        masks = torch.full((len(live), N), float("nan"), device=dev)
        for j, (lo, hi) in enumerate(live):
            masks[j, lo:hi] = 0.0
        few = max(1, reps * 18 // (4 * G))
        for k in (10, 100):
            tag = "G=%d k=%d " % (G, k)
            paths[tag + "(a) sections"] = lambda k=k, ptr=ptr: eng.top_k_sections(user, items, ids, ptr, k, hist)
            paths[tag + "(b) per-range topk_dot"] = lambda k=k, parts=parts, part_ex=part_ex: [
                eng.top_k(user, p, k, e) for p, e in zip(parts, part_ex)]
            paths[tag + "(c) nan-mask topk_dot_biased"] = lambda k=k, masks=masks: [
                eng.top_k(user, items, k, hist, bias=m) for m in masks]
            paths[tag + "(d) plain topk_dot"] = lambda k=k: eng.top_k(user, items, k, hist)
            path_reps.update({tag + "(a) sections": reps, tag + "(b) per-range topk_dot": max(1, reps * 18 // (2 * G)),
                              tag + "(c) nan-mask topk_dot_biased": few, tag + "(d) plain topk_dot": reps})
        # what is timed is one result: (a) equals (b) section by section (ids are rows, so (b)'s rows shift by lo)
        sa, ia = eng.top_k_sections(user, items, ids, ptr, 10, hist)
        nonempty = [j for j, (lo, hi) in enumerate(zip(ptr_host[:-1], ptr_host[1:])) if hi > lo]
        for j, (lo, hi), p, e in zip(nonempty, live, parts, part_ex):
            sb, ib = eng.top_k(user, p, 10, e)
            assert torch.equal(torch.where(ib >= 0, ib + lo, ib), ia[:, j]) and torch.equal(sb, sa[:, j]), (G, j)
        print("G=%d: (a) equals (b) in every section, ids and score bits" % G)

    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, path_reps[name]))
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "B": B, "N": N, "d": d, "n_exclude": H,
           "reps": path_reps, "windows": windows, "sections": {str(G): v for G, v in sizes_of.items()}, "ms": {}, "spread_ms": {},
           "windows_ms": {}, "ratio": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-44s %10.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    for G in (18, 270):
        for k in (10, 100):
            tag = "G=%d k=%d " % (G, k)
            a = rec["ms"][tag + "(a) sections"]
            for other in ("(b) per-range topk_dot", "(c) nan-mask topk_dot_biased", "(d) plain topk_dot"):
                rec["ratio"][tag + "(a) / " + other[:3]] = round(a / rec["ms"][tag + other], 4)
            print("%s (a)/(b) = %.4f  (a)/(c) = %.4f  (a)/(d) = %.4f" % (tag, rec["ratio"][tag + "(a) / (b)"],
                                                                       rec["ratio"][tag + "(a) / (c)"], rec["ratio"][tag + "(a) / (d)"]))
    a, b = "G=18 k=10 (a) sections", "G=18 k=10 (b) per-range topk_dot"
    margin = max(rec["spread_ms"][a], rec["spread_ms"][b])
    rec["bar"] = {"statement": "min (a) < min (b) - max(spread (a), spread (b)) at G = 18, k = 10", "a_ms": rec["ms"][a],
                  "b_ms": rec["ms"][b], "margin_ms": margin, "met": bool(rec["ms"][a] < rec["ms"][b] - margin)}
    print("bar at G=18 k=10: (a) %.4f ms, (b) %.4f ms, margin %.4f ms: %s" % (rec["ms"][a], rec["ms"][b], margin,
                                                                              "MET" if rec["bar"]["met"] else "MISSED"))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
