"""Timing of the diversified re-ranking: nrms_mmr_rerank (NRMSEngine.mmr_rerank, ILD included) at k = 10
and k = 100 over the shortlist nrms_topk_dot returns at k = M = 256, beside that nrms_topk_dot call (the call it follows) and a
torch-eager fp32 restatement on the same GPU in the same run: gather the M rows, normalise, torch.bmm for the [B, M, M] cosines,
then k steps of masked argmax + torch.maximum (no tie rule and no ILD: it is there for its time, and its picks are compared with
the kernel's as a sanity check, not bit for bit).  B = 512 users, N = 130 000 news, d = 300.  k = 1 is timed too: it is the Gram
kernel plus one greedy step, which separates the two kernels' shares.
The bar: at both k the kernel is no slower than the torch restatement.  Device-event timing, every shape warmed up first, the
paths alternate, the minimum of the repeated runs is kept.
Usage: python tools/bench_mmr.py [B] [N] [reps] [--json FILE]"""
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


def torch_mmr(items, ids, scores, k, lam):
    """The contract in torch-eager fp32 (ties by argmax's choice) -> picked ids [B, k]."""
    B, M = ids.shape
    N = items.shape[0]
    valid = (ids >= 0) & (ids < N) & torch.isfinite(scores)
    x = items.index_select(0, ids.clamp(0, N - 1).reshape(-1)).view(B, M, -1)
    x = x / x.norm(dim=2, keepdim=True).clamp_min(1e-30)
    sim = torch.bmm(x, x.transpose(1, 2))
    lo = torch.where(valid, scores, torch.full_like(scores, float("inf"))).amin(dim=1, keepdim=True)
    hi = torch.where(valid, scores, torch.full_like(scores, -float("inf"))).amax(dim=1, keepdim=True)
    rel = torch.where(valid, (scores - lo) / (hi - lo), torch.zeros_like(scores))
    live = valid.clone()
    rows = torch.arange(B, device=ids.device)
    picks = torch.empty(B, k, dtype=torch.int64, device=ids.device)
    maxsim = torch.zeros_like(scores)
    ninf = torch.full_like(scores, -float("inf"))
    for t in range(k):
        v = torch.where(live, lam * rel - (1.0 - lam) * maxsim, ninf)
        p = v.argmax(dim=1)
        picks[:, t] = p
        live[rows, p] = False
        row = sim[rows, p]
        maxsim = row if t == 0 else torch.maximum(maxsim, row)
    return ids.gather(1, picks)


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
    d, M, lam = 300, 256, 0.5
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    user = torch.randn(B, d, device=dev, generator=g)
    items = torch.randn(N, d, device=dev, generator=g)
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)
    s_scores, s_ids = eng.top_k(user, items, M)

    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "B": B, "N": N, "d": d, "M": M, "lambda": lam,
           "reps": reps, "gram_gflop": round(2.0 * B * M * M * d / 1e9, 2),
           "gathered_mb": round(B * M * d * 4 / 1e6, 1), "workspace_mb": round(B * M * M * 4 / 1e6, 1), "ms": {}, "agreement": {}}
    topk = lambda: eng.top_k(user, items, M)                          # noqa: E731
    for k in (1, 10, 100):
        mmr = lambda: eng.mmr_rerank(items, s_ids, s_scores, k, lam, return_ild=True)       # noqa: E731
        ref = lambda: torch_mmr(items, s_ids, s_scores, k, lam)                            # noqa: E731
        got, want = mmr()[0], ref()
        topk()
        torch.cuda.synchronize()
        rec["agreement"]["k=%d" % k] = round(float((got == want).float().mean()), 4)
        ts = {"nrms_mmr_rerank": [], "nrms_topk_dot k=%d" % M: [], "torch gather+normalise+bmm+k steps": []}
        for _ in range(3):                                            # alternate the paths
            ts["nrms_mmr_rerank"].append(event_ms(mmr, reps))
            ts["nrms_topk_dot k=%d" % M].append(event_ms(topk, reps))
            ts["torch gather+normalise+bmm+k steps"].append(event_ms(ref, max(2, reps // 4)))
        for name, t in ts.items():
            ms = min(t)
            rec["ms"]["k=%d %s" % (k, name)] = round(ms, 4)
            print("k=%-3d %-36s %8.3f ms (runs %s)  %10.0f users/s" % (k, name, ms, " ".join("%.3f" % v for v in t), B / ms * 1e3))
        ratio = min(ts["torch gather+normalise+bmm+k steps"]) / min(ts["nrms_mmr_rerank"])
        rec["ms"]["k=%d torch / mmr" % k] = round(ratio, 2)
        print("k=%-3d torch / nrms_mmr_rerank = %.2f   picks equal to torch's: %.1f %%" % (k, ratio, 100 * rec["agreement"]["k=%d" % k]))
    gram_ms = rec["ms"]["k=1 nrms_mmr_rerank"]
    print("Gram share (k = 1): %.3f ms for %.1f GFLOP of full-matrix work (%.0f %% of the %.0f TF fp32 MFMA peak; the kernel forms "
          "the upper block triangle only)" % (gram_ms, rec["gram_gflop"], 100 * rec["gram_gflop"] / gram_ms / PEAK_TF, PEAK_TF))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
