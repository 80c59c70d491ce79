"""Timing of the score attribution: nrms_attribution_dot (NRMSEngine.attribution, m = 3, without and with
the [B, K, H] terms) over the list nrms_topk_dot returns at K = 10, 100 and 256, beside that nrms_topk_dot call (the call it
follows) and a torch-eager fp32 restatement on the same GPU in the same run: index_select the K rows, torch.bmm against the
history's context rows for the [B, K, H] products, scale by w, topk(m) over the named slots and the two sums (no tie rule and no
ordered sum: it is there for its time; its totals are compared with the kernel's as a sanity check, not bit for bit).
B = 512 users, H = 50 history slots, d = 300, N = 130 000 news.  No bar is fixed: the ratio to the torch restatement is
reported as measured.  Device-event timing, every shape warmed up first, the paths alternate, the minimum of the repeated
runs is kept.
Usage: python tools/bench_attribution.py [B] [N] [reps] [--json FILE]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine

PEAK_TF = 157.3        # fp32 MFMA peak of the MI355X (v_mfma_f32_32x32x2_f32)


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def torch_attribution(ctx, w, items, ids, m, named):
    """The contract in torch-eager fp32 (topk's ties, torch's sums) -> (top_slots, top_contrib, total, unnamed_share)."""
    B, K = ids.shape
    N = items.shape[0]
    valid = (ids >= 0) & (ids < N)
    x = items.index_select(0, ids.clamp(0, N - 1).reshape(-1)).view(B, K, -1)
    c = torch.bmm(x, ctx.transpose(1, 2)) * w[:, None, :]                  # [B, K, H]
    c = torch.where(valid[:, :, None], c, torch.zeros_like(c))
    nm = named[:, None, :] != 0
    top_c, top_s = torch.where(nm, c, torch.full_like(c, -float("inf"))).topk(m, dim=2)
    total = torch.where(valid, c.sum(2), torch.full_like(c[:, :, 0], -float("inf")))
    unnamed = torch.where(nm, torch.zeros_like(c), c).sum(2)
    return top_s, top_c, total, unnamed


def main():
    argv = list(sys.argv[1:])
    out = None
    if "--json" in argv:
        i = argv.index("--json")
        out = argv[i + 1]
        del argv[i:i + 2]
    B = int(argv[0]) if len(argv) > 0 else 512
    N = int(argv[1]) if len(argv) > 1 else 130000
    reps = int(argv[2]) if len(argv) > 2 else 20
    H, d, m = 50, 300, 3
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    items = torch.randn(N, d, device=dev, generator=g)
    ctx = torch.randn(B, H, d, device=dev, generator=g)
    w = torch.softmax(torch.randn(B, H, device=dev, generator=g), dim=1)
    user = torch.bmm(w[:, None, :], ctx).squeeze(1).contiguous()          # the user vector the list is retrieved with
    named = (torch.arange(H, device=dev)[None, :] < torch.randint(5, H + 1, (B, 1), device=dev, generator=g)).to(torch.uint8)
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)

    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "B": B, "H": H, "N": N, "d": d, "m": m,
           "reps": reps, "ms": {}, "gflop": {}, "max_abs_total_diff_vs_torch": {}}
    for K in (10, 100, 256):
        scores, ids = eng.top_k(user, items, K)
        topk = lambda: eng.top_k(user, items, K)                                          # noqa: E731
        attr = lambda: eng.attribution(ctx, w, items, ids, m, slot_named=named)           # noqa: E731
        attr_c = lambda: eng.attribution(ctx, w, items, ids, m, slot_named=named, return_contrib=True)   # noqa: E731
        ref = lambda: torch_attribution(ctx, w, items, ids, m, named)                     # noqa: E731
        got, want = attr(), ref()
        attr_c()
        topk()
        torch.cuda.synchronize()
        rec["max_abs_total_diff_vs_torch"]["K=%d" % K] = float((got[2] - want[2]).abs().max())
        rec["max_abs_total_diff_vs_topk_score"] = rec.get("max_abs_total_diff_vs_topk_score", {})
        rec["max_abs_total_diff_vs_topk_score"]["K=%d" % K] = float((got[2] - scores).abs().max())
        gf = 2.0 * B * K * H * d / 1e9
        rec["gflop"]["K=%d" % K] = round(gf, 2)
        names = ("nrms_attribution_dot", "nrms_attribution_dot + contrib", "nrms_topk_dot", "torch index_select+bmm+topk+sums")
        ts = {n: [] for n in names}
        for _ in range(3):                                                # alternate the paths
            ts[names[0]].append(event_ms(attr, reps))
            ts[names[1]].append(event_ms(attr_c, reps))
            ts[names[2]].append(event_ms(topk, reps))
            ts[names[3]].append(event_ms(ref, max(2, reps // 2)))
        for name, t in ts.items():
            ms = min(t)
            rec["ms"]["K=%d %s" % (K, name)] = round(ms, 4)
            print("K=%-3d %-36s %8.3f ms (runs %s)" % (K, name, ms, " ".join("%.3f" % v for v in t)))
        a, t, r = min(ts[names[0]]), min(ts[names[2]]), min(ts[names[3]])
        rec["ms"]["K=%d torch / attribution" % K] = round(r / a, 2)
        rec["ms"]["K=%d attribution / topk" % K] = round(a / t, 3)
        print("K=%-3d torch / nrms_attribution_dot = %.2f   attribution / the nrms_topk_dot before it = %.3f   %.2f GFLOP: %.0f %% of "
              "the %.0f TF fp32 MFMA peak   max |total - torch| %.2e" % (K, r / a, a / t, gf, 100 * gf / a / PEAK_TF, PEAK_TF,
                                                                        rec["max_abs_total_diff_vs_torch"]["K=%d" % K]))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
