"""Two builds of libnrms_hip.so in one process: every catalogue entry point (nrms_topk_dot, _biased, _windowed, nrms_topk_grouped_dot,
nrms_topk_sections_dot, nrms_softmax_sample_dot, nrms_rank_dot, _biased, _windowed) called in both on the same device tensors.

Default: compare the outputs byte for byte over the smallest shapes that reach every path of the kernels (B in {1, 33},
N in {1, 63, 2100}, d in {3, 31, 64, 301}, k in {1, 65, 193, 256}, n_exclude in {0, 50, 70}, T in {1, 32}, G in {1, 5} with an empty
group and one of 33 rows, and one call with user and item pointers offset by 4 bytes).  Inputs are seeded normal fp32 with NaN
scores, duplicated item rows, -0.0 and one user with an empty window.  Prints one summary line; exit status 1 on any difference.

--bench: time the two builds instead, alternating, at B = 512, N = 130 000, d = 300, 50 excluded ids: the minimum of `--windows`
windows of `--reps` calls per path and build, and the parent's own window-to-window spread (max - min) as the margin.

Usage: python tools/compare_catalogue_libs.py --parent_lib FILE [--bench] [--windows 5] [--reps 20] [--json FILE]
(FILE: a libnrms_hip.so built from the parent commit; this tree's own library is the other one)."""
import ctypes as C
import itertools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_news_recommender_amd import _lib

CALLS = ("nrms_topk_dot", "nrms_topk_dot_biased", "nrms_topk_dot_windowed", "nrms_topk_grouped_dot", "nrms_topk_sections_dot",
         "nrms_softmax_sample_dot", "nrms_rank_dot", "nrms_rank_dot_biased", "nrms_rank_dot_windowed")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
P = _lib.ptr


class Lib:
    """One build: its own kernels and launch stubs, whatever else is loaded.  Every method returns the call's output tensors."""

    def __init__(self, path, dev):
        import torch  # noqa: F401  (torch's HIP runtime is resident before the library binds to it)
        self.lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        for name in CALLS:
            for n in (name, name + "_workspace_bytes"):
                getattr(self.lib, n).restype, getattr(self.lib, n).argtypes = _lib.SIGNATURES[n]
        self.lib.nrms_last_error.restype = C.c_char_p
        self.dev, self.keep = dev, {}

    def buf(self, key, shape, dtype):
        """An output (or workspace) buffer of this build, kept per key and poisoned before every use."""
        k = (key, tuple(shape), dtype)
        if k not in self.keep:
            self.keep[k] = torch.empty(shape, dtype=dtype, device=self.dev)
        t = self.keep[k]
        if not self.timing:
            t.view(torch.uint8).fill_(0xCD)
        return t

    timing = False

    def ws(self, nbytes):
        assert nbytes > 0, "arguments rejected"
        return self.buf("ws", ((nbytes + 15) // 16 * 2,), torch.int64)

    def ok(self, rc, what):
        assert rc == 0, "%s: rc %d: %s" % (what, rc, self.lib.nrms_last_error())

    def top_k(self, user, items, k, ex, bias=None, item_time=None, window=None):
        (B, d), N, L = user.shape, items.shape[0], self.lib
        ws = self.ws(L.nrms_topk_dot_workspace_bytes(B, N, d, k))
        sc, ids = self.buf("sc", (B, k), torch.float32), self.buf("ids", (B, k), torch.int64)
        tail = (P(ex), 0 if ex is None else ex.shape[1], P(sc), P(ids), P(ws), ws.numel() * 8, None)
        if window is not None:
            self.ok(L.nrms_topk_dot_windowed(B, N, d, k, P(user), P(items), P(bias), P(item_time), P(window), *tail), "topk_dot_windowed")
        elif bias is not None:
            self.ok(L.nrms_topk_dot_biased(B, N, d, k, P(user), P(items), P(bias), *tail), "topk_dot_biased")
        else:
            self.ok(L.nrms_topk_dot(B, N, d, k, P(user), P(items), *tail), "topk_dot")
        return sc, ids

    def top_k_grouped(self, query, items, item_ids, group_ptr, k, ex):
        (B, G, d), N, L = query.shape, items.shape[0], self.lib
        ws = self.ws(L.nrms_topk_grouped_dot_workspace_bytes(B, N, d, k, G))
        sc, ids = self.buf("sc", (B, k), torch.float32), self.buf("ids", (B, k), torch.int64)
        self.ok(L.nrms_topk_grouped_dot(B, N, d, k, G, P(query), P(items), P(item_ids), P(group_ptr), P(ex), 0 if ex is None else ex.shape[1],
                                        P(sc), P(ids), P(ws), ws.numel() * 8, None), "topk_grouped_dot")
        return sc, ids

    def top_k_sections(self, user, items, item_ids, section_ptr, k, ex, bias=None, slice_tiles=0):
        (B, d), N, G, L = user.shape, items.shape[0], section_ptr.shape[0] - 1, self.lib
        ws = self.ws(L.nrms_topk_sections_dot_workspace_bytes(B, N, d, k, G, slice_tiles))
        sc, ids = self.buf("sc", (B, G, k), torch.float32), self.buf("ids", (B, G, k), torch.int64)
        self.ok(L.nrms_topk_sections_dot(B, N, d, k, G, slice_tiles, P(user), P(items), P(item_ids), P(section_ptr), P(bias), P(ex),
                                         0 if ex is None else ex.shape[1], P(sc), P(ids), P(ws), ws.numel() * 8, None), "topk_sections_dot")
        return sc, ids

    def softmax_sample(self, user, items, row_key, S, inv_t, seed, ex):
        (B, d), N, L = user.shape, items.shape[0], self.lib
        n_ex = 0 if ex is None else ex.shape[1]
        ws = self.ws(L.nrms_softmax_sample_dot_workspace_bytes(B, N, d, S, n_ex))
        ids, keys = self.buf("ids", (B, S), torch.int64), self.buf("sc", (B, S), torch.float32)
        self.ok(L.nrms_softmax_sample_dot(B, N, d, S, P(user), P(items), P(row_key), inv_t, seed, P(ex), n_ex, P(ids), P(keys), P(ws),
                                          ws.numel() * 8, None), "softmax_sample_dot")
        return ids, keys

    def rank_of(self, user, items, tg, ex, bias=None, item_time=None, window=None):
        (B, d), N, T, L = user.shape, items.shape[0], tg.shape[1], self.lib
        n_ex = 0 if ex is None else ex.shape[1]
        ws = self.ws(L.nrms_rank_dot_workspace_bytes(B, N, d, T, n_ex))
        rk, sc = self.buf("rk", (B, T), torch.int32), self.buf("sc", (B, T), torch.float32)
        tail = (P(tg), P(ex), n_ex, P(rk), P(sc), P(ws), ws.numel() * 8, None)
        if window is not None:
            self.ok(L.nrms_rank_dot_windowed(B, N, d, T, P(user), P(items), P(bias), P(item_time), P(window), *tail), "rank_dot_windowed")
        elif bias is not None:
            self.ok(L.nrms_rank_dot_biased(B, N, d, T, P(user), P(items), P(bias), *tail), "rank_dot_biased")
        else:
            self.ok(L.nrms_rank_dot(B, N, d, T, P(user), P(items), *tail), "rank_dot")
        return rk, sc


def group_ptr(N, G, dev):
    """G = 1: one group.  G = 5: 33 rows (or all), an empty group, and three thirds of the rest."""
    if G == 1:
        return torch.tensor([0, N], dtype=torch.int64, device=dev)
    a = min(33, N)
    return torch.tensor([0, a, a, a + (N - a) // 3, a + 2 * (N - a) // 3, N], dtype=torch.int64, device=dev)


def catalogue(B, N, d, gen, dev, offset=False):
    """Seeded inputs with the awkward values in: a NaN score column, a duplicated row (ties), a row of -0.0, NaN in the bias,
    out-of-range ids.  offset: user and items start 4 bytes past a 16-byte boundary (the scalar-load path at any d)."""
    def randn(n, m):
        flat = torch.randn(n * m + 4, device=dev, generator=gen)
        return flat[1:1 + n * m].view(n, m) if offset else flat[:n * m].view(n, m)
    user, items = randn(B, d), randn(N, d)
    if N >= 4:
        items[1, 0] = float("nan")
        items[N - 1] = items[0]
        items[2] = -0.0
    if B > 1 and d > 3:
        user[B - 1, 0] = float("nan")              # a user all of whose scores are NaN
    bias = torch.randn(N, device=dev, generator=gen)
    if N >= 8:
        bias[5] = float("nan")
    item_time = torch.randint(0, 1000, (N,), device=dev, generator=gen).to(torch.int32)
    lo = torch.randint(0, 600, (B,), device=dev, generator=gen)
    window = torch.stack([lo, lo + 300], dim=1).to(torch.int32)
    window[0, 1] = window[0, 0]                    # user 0: an empty window
    if B > 2:
        window[2] = torch.tensor([I32_MIN, I32_MAX], dtype=torch.int64).to(torch.int32)
    return user, items, bias, item_time.contiguous(), window.contiguous()


def differing_bytes(a, b):
    return sum(int((x.contiguous().view(torch.uint8) != y.contiguous().view(torch.uint8)).sum()) for x, y in zip(a, b))


def compare(parent, new, dev):
    gen = torch.Generator(device=dev).manual_seed(20260101)
    calls = diff = 0
    worst = []

    def both(what, fn):
        nonlocal calls, diff
        a, b = fn(parent), fn(new)
        assert not bool((a[0].view(torch.uint8) == 0xCD).all()), what + ": the call wrote nothing"
        n = differing_bytes(a, b)
        calls += 1
        diff += n
        if n:
            worst.append("%s: %d bytes" % (what, n))

    cases = list(itertools.product((1, 33), (1, 63, 2100), (3, 31, 64, 301), (1, 65, 193, 256), (0, 50, 70)))
    data = {}
    for i, (B, N, d, k, n_ex) in enumerate(cases):
        if (B, N, d) not in data:
            data[B, N, d] = catalogue(B, N, d, gen, dev)
        user, items, bias, item_time, window = data[B, N, d]
        T, G = (1, 32)[i % 2], (1, 5)[(i // 2) % 2]
        ex = torch.randint(-2, N + 3, (B, n_ex), device=dev, generator=gen) if n_ex else None
        tg = torch.randint(-1, N + 1, (B, T), device=dev, generator=gen)
        gptr = group_ptr(N, G, dev)
        item_ids = (torch.randperm(N, device=dev, generator=gen) + 7).to(torch.int32)
        query = torch.randn(B, G, d, device=dev, generator=gen)
        row_key = torch.arange(B, dtype=torch.int64, device=dev) * 977 + 3
        tag = "B=%d N=%d d=%d k=%d n_exclude=%d T=%d G=%d" % (B, N, d, k, n_ex, T, G)
        both("topk_dot " + tag, lambda L: L.top_k(user, items, k, ex))
        both("topk_dot_biased " + tag, lambda L: L.top_k(user, items, k, ex, bias))
        both("topk_dot_windowed " + tag, lambda L: L.top_k(user, items, k, ex, None, item_time, window))
        both("topk_dot_windowed+bias " + tag, lambda L: L.top_k(user, items, k, ex, bias, item_time, window))
        both("topk_grouped_dot " + tag, lambda L: L.top_k_grouped(query, items, item_ids, gptr, k, ex))
        both("topk_sections_dot " + tag, lambda L: L.top_k_sections(user, items, item_ids, gptr, k, ex, None, int(i % 3 == 0)))
        both("topk_sections_dot+bias " + tag, lambda L: L.top_k_sections(user, items, item_ids, gptr, k, ex, bias, int(i % 3 == 1)))
        both("softmax_sample_dot " + tag, lambda L: L.softmax_sample(user, items, row_key, k, 0.7, 1234 + i, ex))
        both("rank_dot " + tag, lambda L: L.rank_of(user, items, tg, ex))
        both("rank_dot_biased " + tag, lambda L: L.rank_of(user, items, tg, ex, bias))
        both("rank_dot_windowed " + tag, lambda L: L.rank_of(user, items, tg, ex, bias if i % 2 else None, item_time, window))
    # user and item pointers 4 bytes past a 16-byte boundary: the scalar loads at a d that would take the vector loads
    B, N, d, k = 33, 2100, 64, 65
    user, items, bias, item_time, window = catalogue(B, N, d, gen, dev, offset=True)
    assert user.data_ptr() % 16 == 4 and items.data_ptr() % 16 == 4
    ex = torch.randint(0, N, (B, 50), device=dev, generator=gen)
    tg = torch.randint(0, N, (B, 8), device=dev, generator=gen)
    gptr, item_ids = group_ptr(N, 5, dev), torch.arange(N, dtype=torch.int32, device=dev)
    both("topk_dot offset", lambda L: L.top_k(user, items, k, ex))
    both("topk_dot_windowed+bias offset", lambda L: L.top_k(user, items, k, ex, bias, item_time, window))
    both("topk_sections_dot offset", lambda L: L.top_k_sections(user, items, item_ids, gptr, k, ex))
    both("softmax_sample_dot offset", lambda L: L.softmax_sample(user, items, torch.arange(B, device=dev), k, 0.7, 99, ex))
    both("rank_dot offset", lambda L: L.rank_of(user, items, tg, ex))
    return calls, diff, worst


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def bench(parent, new, dev, windows, reps):
    B, N, d, H, G = 512, 130000, 300, 50, 18
    gen = torch.Generator(device=dev).manual_seed(0)
    user = torch.randn(B, d, device=dev, generator=gen)
    items = torch.randn(N, d, device=dev, generator=gen)
    hist = torch.randint(0, N, (B, H), device=dev, generator=gen)
    t_sorted = torch.arange(N, dtype=torch.int32, device=dev)           # the catalogue in time order
    full = torch.tensor([[I32_MIN, I32_MAX]], dtype=torch.int64).expand(B, 2).to(torch.int32).to(dev).contiguous()
    lo = torch.randint(0, N - N // 16 + 1, (B,), device=dev, generator=gen).sort().values
    w16 = torch.stack([lo, lo + N // 16], dim=1).to(torch.int32).contiguous()
    gptr = (torch.arange(G + 1, device=dev) * N // G).to(torch.int64)
    item_ids = torch.arange(N, dtype=torch.int32, device=dev)
    query = torch.randn(B, G, d, device=dev, generator=gen)
    row_key = torch.arange(B, dtype=torch.int64, device=dev)
    tg = {T: torch.randint(0, N, (B, T), device=dev, generator=gen) for T in (1, 8)}
    paths = {
        "topk_dot k=10": lambda L: L.top_k(user, items, 10, hist),
        "topk_dot k=100": lambda L: L.top_k(user, items, 100, hist),
        "topk_dot_windowed k=10 full window": lambda L: L.top_k(user, items, 10, hist, None, t_sorted, full),
        "topk_dot_windowed k=10 window 1/16": lambda L: L.top_k(user, items, 10, hist, None, t_sorted, w16),
        "topk_grouped_dot k=10 G=18": lambda L: L.top_k_grouped(query, items, item_ids, gptr, 10, hist),
        "topk_sections_dot k=10 G=18": lambda L: L.top_k_sections(user, items, item_ids, gptr, 10, hist),
        "softmax_sample_dot S=4": lambda L: L.softmax_sample(user, items, row_key, 4, 1.0, 7, hist),
        "rank_dot T=1": lambda L: L.rank_of(user, items, tg[1], hist),
        "rank_dot T=8": lambda L: L.rank_of(user, items, tg[8], hist),
    }
    equal = all(differing_bytes(fn(parent), fn(new)) == 0 for fn in paths.values())     # also the warm-up of every shape
    for fn in paths.values():
        fn(parent), fn(new)
    torch.cuda.synchronize()
    Lib.timing = True                     # no poisoning of the outputs inside the timed windows
    ts = {(name, who): [] for name in paths for who in ("parent", "new")}
    for _ in range(windows):
        for name, fn in paths.items():
            for who, L in (("parent", parent), ("new", new)):
                ts[name, who].append(event_ms(lambda: fn(L), reps))
    Lib.timing = False
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "B": B, "N": N, "d": d, "n_exclude": H,
           "reps": reps, "windows": windows, "outputs_equal": equal, "paths": {}}
    print("%-38s %10s %10s %10s %8s" % ("call", "parent ms", "new ms", "spread ms", "verdict"))
    for name in paths:
        p, n = ts[name, "parent"], ts[name, "new"]
        spread = max(p) - min(p)
        ok = min(n) <= min(p) + spread
        rec["paths"][name] = {"parent_ms": round(min(p), 4), "new_ms": round(min(n), 4), "parent_spread_ms": round(spread, 4),
                              "within_margin": ok, "parent_windows_ms": [round(v, 4) for v in p], "new_windows_ms": [round(v, 4) for v in n]}
        print("%-38s %10.4f %10.4f %10.4f %8s" % (name, min(p), min(n), spread, "ok" if ok else "SLOWER"))
    rec["all_within_margin"] = all(v["within_margin"] for v in rec["paths"].values())
    print("outputs equal: %s; every call within the parent's spread: %s" % (equal, rec["all_within_margin"]))
    return rec


def main():
    argv = list(sys.argv[1:])

    def opt(name, default, conv):
        if name in argv:
            i = argv.index(name)
            v = conv(argv[i + 1])
            del argv[i:i + 2]
            return v
        return default

    parent_lib = opt("--parent_lib", None, str)
    out = opt("--json", None, str)
    windows, reps = opt("--windows", 5, int), opt("--reps", 20, int)
    if not parent_lib:
        sys.exit(__doc__)
    dev = torch.device("cuda", 0)
    parent, new = Lib(parent_lib, dev), Lib(_lib.LIB_PATH, dev)
    if "--bench" in argv:
        rec = bench(parent, new, dev, windows, reps)
        bad = not (rec["outputs_equal"] and rec["all_within_margin"])
    else:
        t0 = time.time()
        calls, diff, worst = compare(parent, new, dev)
        rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "calls": calls, "differing_bytes": diff,
               "differing_calls": worst[:20]}
        for w in worst[:20]:
            print("DIFFERS", w)
        print("compare_catalogue_libs: %d calls into each library, %d differing bytes (%.1f s)" % (calls, diff, time.time() - t0))
        bad = diff != 0
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
