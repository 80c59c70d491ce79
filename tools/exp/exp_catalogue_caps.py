"""What a hard cap per category does to the served list (docs/EXPERIMENTS.md).  Parity is unpinned: the reference has no catalogue
retrieval.

One run_v0 training over the synthetic click log; the live users are then served their top 10 uncapped and with at most 1, 2 and 3
news per category, by the very call run_v0 --max_per_category makes (train_eval.recommend(tag_caps=...)), on the one trained
model.  Recorded per cap: the mean number of distinct categories per list, the mean largest share of one category, and the share of
the held-out clicks found in the list at 1, 5 and 10 with its binomial standard error.  A record with no bar.
Usage: python tools/exp/exp_catalogue_caps.py [--json FILE] [--users N] [--epochs E]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from pytorch_news_recommender_amd import run_v0

K = 10


def main():
    argv = list(sys.argv[1:])

    def opt(name, default, conv):
        if name in argv:
            i = argv.index(name)
            v = conv(argv[i + 1])
            del argv[i:i + 2]
            return v
        return default

    out, users, epochs = opt("--json", None, str), opt("--users", 4096, int), opt("--epochs", 3, int)
    real = run_v0.recommend
    rec = {}

    def recommend(config, model, data_iter, titles, k, **kw):
        net = model.model if hasattr(model, "model") else model
        cap = int(kw["tag_caps"].max())
        if cap >= k:                                                  # run_v0's own uncapped pass
            res = real(config, model, data_iter, titles, k, **kw)
            rec["uncapped"] = dict(net.last_caps_stats)
            return res
        for m in (1, 2, 3):                                           # in place of run_v0's one capped pass
            res = real(config, model, data_iter, titles, k, **dict(kw, tag_caps=torch.full_like(kw["tag_caps"], m), out_file=os.devnull))
            rec["at most %d" % m] = dict(net.last_caps_stats)
        return real(config, model, data_iter, titles, k, **kw)

    run_v0.recommend = recommend
    tmp = tempfile.mkdtemp()
    run_v0.main(["--model", "nrms_hip", "--dataset", "synthetic", "--negatives", "catalogue", "--recommend", str(K),
                 "--max_per_category", "2", "--synthetic_users", str(users), "--epochs", str(epochs), "--precision", "fp16",
                 "--num_workers", "0", "--description", "caps", "--data_path", os.path.join(tmp, "data"),
                 "--save_path", os.path.join(tmp, "save"), "--recommend_out", os.path.join(tmp, "rec.txt")])
    print("| per category | categories per list | largest share | hit@1 | hit@5 | hit@10 | users |")
    print("|---|---|---|---|---|---|---|")
    for name in ("uncapped", "at most 3", "at most 2", "at most 1"):
        r = rec[name]
        print("| %s | %.3f | %.4f | %s | %d |" % (name, r["distinct_tags"], r["largest_share"],
                                                 " | ".join("%.4f ± %.4f" % (r["hit"][kk], r["hit_se"][kk]) for kk in (1, 5, 10)), r["n_users"]))
    if out:
        with open(out, "w") as f:
            json.dump({"date": time.strftime("%Y-%m-%d"), "parity": "unpinned (the reference has no catalogue retrieval)", "users": users,
                       "epochs": epochs, "news": 4000, "k": K,
                       "rows": {n: {**{a: b for a, b in r.items() if a not in ("hit", "hit_se")},
                                    "hit": {str(a): b for a, b in r["hit"].items()},
                                    "hit_se": {str(a): b for a, b in r["hit_se"].items()}} for n, r in rec.items()}}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
