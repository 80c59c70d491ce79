"""Timing of the per-news prior in retrieval and ranking: nrms_topk_dot_biased beside nrms_topk_dot at
k = 10 / 100, nrms_rank_dot_biased beside nrms_rank_dot at T = 1 / 8, and a torch-eager restatement of the biased top-k (mm,
+ bias, scatter_ of the excluded ids, topk) at B = 512 users, N = 130 000 news, d = 300, 50 excluded ids, in one process.
Device-event timing; every path is warmed up first, the paths alternate, each window is `reps` calls and every window's time is
kept: the record holds the minimum and the spread (max - min over the windows) of every path, so that a difference can be held
against the run-to-run spread.

The expectation from the code: the epilogue adds two 128-byte loads and 32 adds per lane to a wave step of about 300 MFMAs, so
the biased call should sit inside the unbiased call's spread.  This is a record, not a gate.

Run from a tree whose library has no biased symbols (the parent commit) the tool times the unbiased calls and torch only; that
record, given back with --parent FILE, is stored beside this tree's figures under "parent".
Usage: python tools/bench_topk_bias.py [B] [N] [reps] [--windows W] [--parent FILE] [--json FILE]"""
import inspect
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
    parent = opt(argv, "--parent", None, str)
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
    bias = (torch.randn(N, device=dev, generator=g) * 4.0).contiguous()
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)
    has_bias = "bias" in inspect.signature(eng.top_k).parameters
    neg_inf = torch.full((B, H), float("-inf"), device=dev)

    def torch_topk(k):
        s = torch.mm(user, items.T)
        s += bias
        s.scatter_(1, hist, neg_inf)
        return torch.topk(s, k, dim=1)

    paths = {}
    for k in (10, 100):
        paths["topk k=%d unbiased" % k] = lambda k=k: eng.top_k(user, items, k, hist)
        if has_bias:
            paths["topk k=%d biased" % k] = lambda k=k: eng.top_k(user, items, k, hist, bias=bias)
        paths["topk k=%d torch mm+bias+scatter+topk" % k] = lambda k=k: torch_topk(k)
    for T in (1, 8):
        tg = torch.randint(0, N, (B, T), device=dev, generator=g)
        paths["rank T=%d unbiased" % T] = lambda tg=tg: eng.rank_of(user, items, tg, hist)
        if has_bias:
            paths["rank T=%d biased" % T] = lambda tg=tg: eng.rank_of(user, items, tg, hist, bias=bias)

    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
        fn()
    torch.cuda.synchronize()
    if has_bias:                                                      # what is timed is what torch computes, up to fp32 rounding
        ids = eng.top_k(user, items, 10, hist, bias=bias)[1]
        agree = float((ids == torch_topk(10).indices).float().mean())
        print("biased top-10 ids equal to torch's in %.4f of the slots" % agree)
    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, max(1, reps // 4) if "torch" in name else reps))
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "B": B, "N": N, "d": d, "n_exclude": H,
           "reps": reps, "windows": windows, "biased_symbols": has_bias, "ms": {}, "spread_ms": {}, "windows_ms": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-40s %8.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    if has_bias:
        for what in ("topk k=10", "topk k=100", "rank T=1", "rank T=8"):
            rec["ms"][what + " biased / unbiased"] = round(rec["ms"][what + " biased"] / rec["ms"][what + " unbiased"], 4)
            print("%-10s biased / unbiased = %.4f" % (what, rec["ms"][what + " biased / unbiased"]))
    if parent:
        with open(parent) as f:
            p = json.load(f)
        rec["parent"] = {"ms": p["ms"], "spread_ms": p["spread_ms"], "windows_ms": p["windows_ms"]}
        for what in ("topk k=10", "topk k=100", "rank T=1", "rank T=8"):
            name = what + " unbiased"
            if has_bias and name in p["ms"]:
                diff = rec["ms"][what + " biased"] - p["ms"][name]
                rec["ms"][what + " biased - parent unbiased"] = round(diff, 4)
                print("%-10s biased %.4f ms, the parent's unbiased %.4f ms (spread %.4f): %+.4f ms, %s its spread"
                      % (what, rec["ms"][what + " biased"], p["ms"][name], p["spread_ms"][name], diff,
                         "inside" if diff <= p["spread_ms"][name] else "OUTSIDE"))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
