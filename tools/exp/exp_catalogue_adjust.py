"""Retrieval quality when seen-but-not-clicked news is demoted (docs/EXPERIMENTS.md).  Parity is unpinned: the reference has no
catalogue retrieval.

One run_v0 training over the synthetic click log with its seen log (SyntheticMind.seen_log); the held-out clicks are then ranked
against the whole catalogue without any adjustment and with the seen-news discount at beta in {0, 0.25, 0.5, 1}, by the very call
run_v0 --seen_discount makes (train_eval.evaluate_retrieval(adjust=...)), on the one trained model.  The slots are those of
--seen_discount 0.5; the other betas rescale their deltas (delta = -beta * count, exact for these betas).  Every figure comes with
its standard error over users (std / sqrt(n)).  Asserted: beta = 0 reproduces the plain ranks, every one of them, and no rank gets
worse under a discount (the synthetic seen log never holds a clicked news, so a discount can only move other news down: on this
corpus the figures can only rise, which is a property of the corpus, not a finding).  The figures are a record with no bar.
Usage: python tools/exp/exp_catalogue_adjust.py [--json FILE] [--users N] [--epochs E]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from pytorch_news_recommender_amd import run_v0

NAMES = ("recall@10", "recall@100", "mrr")
BETAS = (0.0, 0.25, 0.5, 1.0)


def mean_se(v):
    v = v[~torch.isnan(v)].double()
    n = int(v.numel())
    if n < 2:
        return {"mean": float(v.mean()) if n else float("nan"), "se": float("nan"), "n": n}
    return {"mean": float(v.mean()), "se": float(v.std(unbiased=True) / n ** 0.5), "n": n}


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
    real_eval = run_v0.evaluate_retrieval
    rec = {}

    def evaluate(config, model, data_iter, titles, y_true, **kw):
        net = model.model if hasattr(model, "model") else model
        ids, delta = kw.pop("adjust")                                 # the slots of --seen_discount 0.5
        plain = real_eval(config, model, data_iter, titles, y_true, **kw)
        pm = dict(net.last_retrieval_metrics)
        rec["no adjustment"] = {n: mean_se(pm[n]) for n in NAMES}
        res = plain
        for beta in BETAS:
            res = real_eval(config, model, data_iter, titles, y_true, adjust=(ids, delta * (beta / 0.5)), **kw)
            am = dict(net.last_retrieval_metrics)
            assert bool(((am["ranks"] > 0) == (pm["ranks"] > 0)).all()) and bool((am["ranks"] <= pm["ranks"]).all())
            if beta == 0.0:
                assert torch.equal(am["ranks"], pm["ranks"]), "a discount of 0 moved a rank"
                assert all(torch.equal(am[n].isnan(), pm[n].isnan()) and torch.equal(am[n].nan_to_num(), pm[n].nan_to_num()) for n in NAMES)
            rec["seen_discount %g" % beta] = dict({n: mean_se(am[n]) for n in NAMES},
                                                  ranks_improved=int((am["ranks"] < pm["ranks"]).sum()),
                                                  median_rank=float(am["ranks"][am["ranks"] > 0].double().median()))
        rec["counts"] = {"targets": plain["n_targets"], "skipped": plain["n_skipped"], "slots_per_user": int(ids.shape[1]),
                         "mean_seen_news_per_user": float((ids > 0).float().sum(dim=1).mean()),
                         "median_rank_no_adjustment": float(pm["ranks"][pm["ranks"] > 0].double().median())}
        return res

    run_v0.evaluate_retrieval = evaluate
    tmp = tempfile.mkdtemp()
    run_v0.main(["--model", "nrms_hip", "--dataset", "synthetic", "--negatives", "catalogue", "--retrieval_metrics", "10,100",
                 "--seen_discount", "0.5", "--synthetic_users", str(users), "--epochs", str(epochs), "--precision", "fp16",
                 "--num_workers", "0", "--description", "adjust", "--data_path", os.path.join(tmp, "data"),
                 "--save_path", os.path.join(tmp, "save")])
    print("| ranked with | Recall@10 | Recall@100 | MRR | users |")
    print("|---|---|---|---|---|")
    for name in ("no adjustment",) + tuple("seen_discount %g" % b for b in BETAS):
        r = rec[name]
        print("| %s | %s | %d |" % (name, " | ".join("%.4f ± %.4f" % (r[n]["mean"], r[n]["se"]) for n in NAMES), r["mrr"]["n"]))
    print({k: v for k, v in rec.items() if k == "counts"}, {k: (v["ranks_improved"], v["median_rank"]) for k, v in rec.items() if "ranks_improved" in v})
    if out:
        with open(out, "w") as f:
            json.dump({"date": time.strftime("%Y-%m-%d"), "parity": "unpinned (the reference has no catalogue retrieval)", "users": users,
                       "epochs": epochs, "news": 4000, "rows": rec}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
