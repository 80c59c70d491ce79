"""Timing of the exact catalogue log-partition (csrc/lsedot.hip, nrms_logsumexp_dot; DESIGN.md section 8k, docs/EXPERIMENTS.md).

B = 512 users, N = 130 000 items, d = 300, 50 excluded ids per user, J = 1 / 4 / 8 variants, with and without a prior, beside
nrms_topk_dot at k = 10 on the same data in the same process (the cost of one scan of the catalogue) and a torch restatement
-- torch.mm into a preallocated [B, N] matrix, the excluded ids set to -inf, then per variant a scaled copy (plus the scaled
prior) and torch.logsumexp.  Alternating, the minimum of `rounds` windows of `reps` calls each.  Reported: the ratio to one scan
(two are expected: the maxima and the masses each read the catalogue once) and what the epilogue adds per variant, the slope
from J = 1 to J = 8.  No target was set in advance.

Usage: python tools/bench_log_partition.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine

B, N_NEWS, D, N_EX, SEED = 512, 130000, 300, 50, 20201107
INV_T = [1.0, 0.5, 2.0, 4.0, 0.25, 8.0, 0.125, 20.0]
SCALE = [1.0, 0.0, 0.25, 0.5, 0.75, 1.5, 2.0, -0.5]


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main(rounds=5, reps=5):
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    if not torch.cuda.is_available():
        raise SystemExit("bench_log_partition: no GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda")
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=60, num_attention_heads=6, query_vector_dim=32), dev)
    g = torch.Generator(device=dev).manual_seed(SEED)
    user = torch.randn(B, D, device=dev, generator=g)
    items = torch.randn(N_NEWS, D, device=dev, generator=g) * 0.1          # scores of standard deviation about 1.7
    prior = torch.randn(N_NEWS, device=dev, generator=g)
    hist = torch.randint(0, N_NEWS, (B, N_EX), device=dev, generator=g)
    scores = torch.empty(B, N_NEWS, device=dev)
    z = torch.empty(B, N_NEWS, device=dev)

    def restatement(J, bias):
        def run():
            torch.mm(user, items.t(), out=scores)
            scores.scatter_(1, hist, float("-inf"))
            out = []
            for j in range(J):
                torch.mul(scores, INV_T[j], out=z)
                if bias is not None:
                    z.add_(bias, alpha=SCALE[j])
                out.append(torch.logsumexp(z, dim=1))
            return out
        return run

    fns = {"nrms_topk_dot k=10": lambda: eng.top_k(user, items, 10, hist)}
    for J in (1, 4, 8):
        for name, bias in (("plain", None), ("prior", prior)):
            fns["nrms_logsumexp_dot J=%d %s" % (J, name)] = (
                lambda J=J, bias=bias: eng.log_partition(user, items, INV_T[:J], hist, bias=bias, bias_scale=None if bias is None else SCALE[:J]))
            fns["torch mm+logsumexp J=%d %s" % (J, name)] = restatement(J, bias)
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn, reps))
    best = {k: round(min(v), 4) for k, v in ms.items()}
    scan = best["nrms_topk_dot k=10"]
    derived = {}
    for name in ("plain", "prior"):
        t = {J: best["nrms_logsumexp_dot J=%d %s" % (J, name)] for J in (1, 4, 8)}
        derived[name] = dict(scans={J: round(t[J] / scan, 3) for J in t},
                             epilogue_ms_per_variant=round((t[8] - t[1]) / 7, 4),
                             over_torch={J: round(t[J] / best["torch mm+logsumexp J=%d %s" % (J, name)], 3) for J in t})
    # agreement of the two on this data (float32 torch against the kernel), for the record
    lse = eng.log_partition(user, items, INV_T, hist, bias=prior, bias_scale=SCALE)[0]
    want = torch.stack(restatement(8, prior)(), dim=1)
    out = dict(tool="bench_log_partition", device=torch.cuda.get_device_name(0), B=B, N=N_NEWS, d=D, n_exclude=N_EX, rounds=rounds,
               reps=reps, ms=best, all_ms={k: [round(x, 4) for x in v] for k, v in ms.items()}, derived=derived,
               max_abs_diff_to_torch=float((lse - want).abs().max()))
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
