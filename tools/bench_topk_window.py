"""Timing of the per-user time window in retrieval and ranking at B = 512 users, N = 130 000 news, d = 300,
50 excluded ids, k = 10 / 100, T = 1 / 8, in one process:
  (i)   nrms_topk_dot_windowed / nrms_rank_dot_windowed with the full window beside the unwindowed nrms_topk_dot / nrms_rank_dot.
        With --parent_lib FILE (a libnrms_hip.so built from the parent commit) the unwindowed calls are made into THAT library,
        in the same session; without it, into this tree's.
  (ii)  a catalogue stored in time order, every user's window covering 1/16 and 1/2 of it, each from a start of its own, with the
        requests of the batch in time order (a replayed day: the 32 users of a block ask at about the same moment, so their hull
        is little wider than one window): what the dead-tile skip buys.  "scattered": the same windows with the batch in random
        order, where the hull of a block's 32 windows covers most of the catalogue and the skip can only seldom fire.
  (iii) the time-ordered requests over a row-shuffled catalogue, where a wave's 64 items are scattered over time and the skip
        seldom fires.
  (iv)  a torch restatement: mm, a per-user mask from the times, scatter_ of the excluded ids, topk.
Device-event timing; every path is warmed up first, the paths alternate, each window is `reps` calls and every window's time is
kept: the record holds the minimum and the spread (max - min over the windows) of every path.  This is a record, not a gate.
Usage: python tools/bench_topk_window.py [B] [N] [reps] [--windows W] [--parent_lib FILE] [--json FILE]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream

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


def parent_calls(path, dev):
    """nrms_topk_dot / nrms_rank_dot of another build of the library, with buffers of their own."""
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)       # its own kernels and launch stubs, whatever else is loaded
    for name in ("nrms_topk_dot_workspace_bytes", "nrms_topk_dot", "nrms_rank_dot_workspace_bytes", "nrms_rank_dot"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    keep = {}

    def top_k(user, items, k, ex):
        B, d = user.shape
        N = items.shape[0]
        if ("k", k) not in keep:
            need = lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k)
            keep["k", k] = (torch.empty((need + 7) // 8, dtype=torch.int64, device=dev), torch.empty(B, k, device=dev),
                            torch.empty(B, k, dtype=torch.int64, device=dev))
        ws, sc, ids = keep["k", k]
        rc = lib.nrms_topk_dot(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), _lib.ptr(ex), ex.shape[1], _lib.ptr(sc),
                               _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
        assert rc == 0, rc
        return sc, ids

    def rank_of(user, items, tg, ex):
        B, d = user.shape
        N, T = items.shape[0], tg.shape[1]
        if ("T", T) not in keep:
            need = lib.nrms_rank_dot_workspace_bytes(B, C.c_int64(N), d, T, ex.shape[1])
            keep["T", T] = (torch.empty((need + 7) // 8, dtype=torch.int64, device=dev), torch.empty(B, T, dtype=torch.int32, device=dev),
                            torch.empty(B, T, device=dev))
        ws, rk, sc = keep["T", T]
        rc = lib.nrms_rank_dot(B, C.c_int64(N), d, T, _lib.ptr(user), _lib.ptr(items), _lib.ptr(tg), _lib.ptr(ex), ex.shape[1],
                               _lib.ptr(rk), _lib.ptr(sc), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
        assert rc == 0, rc
        return rk, sc

    return top_k, rank_of


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
    base_topk, base_rank = (lambda u, i, k, ex: eng.top_k(u, i, k, ex)), (lambda u, i, t, ex: eng.rank_of(u, i, t, ex))
    if parent_lib:
        base_topk, base_rank = parent_calls(parent_lib, dev)
    base = "parent" if parent_lib else "unwindowed"

    # the catalogue in time order: item n was published at tick n; and the same catalogue with its rows shuffled
    t_sorted = torch.arange(N, dtype=torch.int32, device=dev)
    rows = torch.randperm(N, device=dev, generator=g)
    items_sh, t_shuf = items[rows].contiguous(), t_sorted[rows].contiguous()
    inv = torch.empty_like(rows)
    inv[rows] = torch.arange(N, device=dev)
    hist_sh = inv[hist].contiguous()
    full = torch.tensor([[I32_MIN, I32_MAX]], dtype=torch.int64).expand(B, 2).to(torch.int32).to(dev).contiguous()

    def frac_window(frac):            # user b's window covers N * frac ticks, from a start of its own
        span = int(N * frac)
        lo = torch.randint(0, N - span + 1, (B,), device=dev, generator=g).sort().values      # the requests in time order
        return torch.stack([lo, lo + span], dim=1).to(torch.int32).contiguous()

    wins = {"1/16": frac_window(1 / 16), "1/2": frac_window(1 / 2)}
    scatter = torch.randperm(B, device=dev, generator=g)
    user_sc, hist_sc = user[scatter].contiguous(), hist[scatter].contiguous()
    neg_inf = torch.full((B, H), float("-inf"), device=dev)

    def torch_topk(k, t, w, it, ex):
        s = torch.mm(user, it.T)
        s.masked_fill_(~((t[None, :] >= w[:, :1]) & (t[None, :] < w[:, 1:])), float("-inf"))
        s.scatter_(1, ex, neg_inf)
        return torch.topk(s, k, dim=1)

    paths = {}
    for k in (10, 100):
        paths["topk k=%d %s" % (k, base)] = lambda k=k: base_topk(user, items, k, hist)
        paths["topk k=%d full window" % k] = lambda k=k: eng.top_k(user, items, k, hist, item_time=t_sorted, window=full)
        for name, w in wins.items():
            paths["topk k=%d sorted window %s" % (k, name)] = lambda k=k, w=w: eng.top_k(user, items, k, hist, item_time=t_sorted, window=w)
            paths["topk k=%d sorted scattered window %s" % (k, name)] = lambda k=k, w=w: eng.top_k(user_sc, items, k, hist_sc, item_time=t_sorted, window=w[scatter].contiguous())
            paths["topk k=%d shuffled window %s" % (k, name)] = lambda k=k, w=w: eng.top_k(user, items_sh, k, hist_sh, item_time=t_shuf, window=w)
        paths["topk k=%d torch mm+mask+scatter+topk window 1/16" % k] = lambda k=k: torch_topk(k, t_sorted, wins["1/16"], items, hist)
    for T in (1, 8):
        tg = torch.randint(0, N, (B, T), device=dev, generator=g)
        tg_sh = inv[tg].contiguous()
        paths["rank T=%d %s" % (T, base)] = lambda tg=tg: base_rank(user, items, tg, hist)
        paths["rank T=%d full window" % T] = lambda tg=tg: eng.rank_of(user, items, tg, hist, item_time=t_sorted, window=full)
        for name, w in wins.items():
            paths["rank T=%d sorted window %s" % (T, name)] = lambda tg=tg, w=w: eng.rank_of(user, items, tg, hist, item_time=t_sorted, window=w)
            paths["rank T=%d sorted scattered window %s" % (T, name)] = lambda tg=tg, w=w: eng.rank_of(user_sc, items, tg[scatter].contiguous(), hist_sc, item_time=t_sorted, window=w[scatter].contiguous())
            paths["rank T=%d shuffled window %s" % (T, name)] = lambda tg=tg_sh, w=w: eng.rank_of(user, items_sh, tg, hist_sh, item_time=t_shuf, window=w)

    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
        fn()
    torch.cuda.synchronize()
    # what is timed is what it should be: the full window is the baseline's list, sorted and shuffled catalogues agree, torch too
    a, b = base_topk(user, items, 10, hist), eng.top_k(user, items, 10, hist, item_time=t_sorted, window=full)
    full_equal = bool(torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))
    w = wins["1/16"]
    s_ids = eng.top_k(user, items, 10, hist, item_time=t_sorted, window=w)[1]
    sh_ids = eng.top_k(user, items_sh, 10, hist_sh, item_time=t_shuf, window=w)[1]
    shuffle_equal = bool(torch.equal(s_ids, rows[sh_ids]))
    agree = float((s_ids == torch_topk(10, t_sorted, w, items, hist).indices).float().mean())
    print("full window == %s call: %s; shuffled catalogue == sorted: %s; top-10 ids equal to torch's in %.4f of the slots"
          % (base, full_equal, shuffle_equal, agree))

    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, max(1, reps // 4) if "torch" in name else reps))
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "B": B, "N": N, "d": d, "n_exclude": H,
           "reps": reps, "windows": windows, "baseline": base, "full_window_equals_baseline": full_equal,
           "shuffled_equals_sorted": shuffle_equal, "torch_top10_agreement": round(agree, 4), "ms": {}, "spread_ms": {}, "windows_ms": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-52s %8.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    rec["ratio"] = {}
    for what in ("topk k=10", "topk k=100", "rank T=1", "rank T=8"):
        b0 = rec["ms"]["%s %s" % (what, base)]
        for name in ("full window", "sorted window 1/16", "sorted window 1/2", "sorted scattered window 1/16", "sorted scattered window 1/2",
                     "shuffled window 1/16", "shuffled window 1/2"):
            rec["ratio"]["%s %s / %s" % (what, name, base)] = round(rec["ms"]["%s %s" % (what, name)] / b0, 4)
            print("%-10s %-30s / %s = %.4f" % (what, name, base, rec["ratio"]["%s %s / %s" % (what, name, base)]))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
