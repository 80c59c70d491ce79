"""Timing of full-catalogue ranking: nrms_rank_dot (NRMSEngine.rank_of) at T = 1 and 8 targets per
user, beside nrms_topk_dot at k = 10 on the same data in the same run, and a torch restatement of the rank -- torch.mm in
8192-column blocks, compare with the gathered target score, sum (it ignores the id tie rule and the exclude list's
correction: it is there for its time, not its bits) -- at B = 512 users, N = 130 000 news, d = 300, 50 excluded ids.
The structural expectation: one catalogue pass, so a time of the order of nrms_topk_dot's, not a multiple of it.
Device-event timing; every shape is warmed up first and the paths alternate.
Usage: python tools/bench_rank.py [B] [N] [reps] [--json FILE]"""
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
    d, H = 300, 50
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    user = torch.randn(B, d, device=dev, generator=g)
    items = torch.randn(N, d, device=dev, generator=g)
    hist = torch.randint(0, N, (B, H), device=dev, generator=g)
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)

    def torch_rank(tg):
        st = torch.einsum("bd,btd->bt", user, items.index_select(0, tg.reshape(-1)).view(B, tg.shape[1], d))
        cnt = torch.zeros(tg.shape, dtype=torch.int64, device=dev)
        for c0 in range(0, N, 8192):
            s = torch.mm(user, items[c0:c0 + 8192].T)
            cnt += (s.unsqueeze(1) > st.unsqueeze(2)).sum(dim=2)
        return cnt + 1

    flops = 2.0 * B * N * d
    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "B": B, "N": N, "d": d, "n_exclude": H,
           "reps": reps, "ms": {}}
    topk = lambda: eng.top_k(user, items, 10, hist)                   # noqa: E731
    for T in (1, 8):
        tg = torch.randint(0, N, (B, T), device=dev, generator=g)
        rank = lambda: eng.rank_of(user, items, tg, hist)             # noqa: E731
        ref = lambda: torch_rank(tg)                                  # noqa: E731
        for fn in (rank, topk, ref):
            fn()
        torch.cuda.synchronize()
        ts = {"nrms_rank_dot": [], "nrms_topk_dot k=10": [], "torch mm blocks+compare+sum": []}
        for _ in range(3):                                            # alternate the paths
            ts["nrms_rank_dot"].append(event_ms(rank, reps))
            ts["nrms_topk_dot k=10"].append(event_ms(topk, reps))
            ts["torch mm blocks+compare+sum"].append(event_ms(ref, max(1, reps // 4)))
        for name, t in ts.items():
            ms = min(t)
            rec["ms"]["T=%d %s" % (T, name)] = round(ms, 4)
            print("T=%-2d %-28s %8.3f ms (runs %s)  %10.0f users/s  %6.1f TF/s (%.0f %% of %.0f TF fp32 peak)"
                  % (T, name, ms, " ".join("%.3f" % v for v in t), B / ms * 1e3, flops / ms / 1e9,
                     100 * flops / ms / 1e9 / PEAK_TF, PEAK_TF))
        rec["ms"]["T=%d rank / topk" % T] = round(min(ts["nrms_rank_dot"]) / min(ts["nrms_topk_dot k=10"]), 3)
        print("T=%-2d nrms_rank_dot / nrms_topk_dot = %.2f" % (T, rec["ms"]["T=%d rank / topk" % T]))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
