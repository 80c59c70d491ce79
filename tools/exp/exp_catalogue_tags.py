"""Retrieval quality against the whole catalogue and inside each user's own categories (docs/EXPERIMENTS.md).  Parity is unpinned:
the reference has no catalogue retrieval.

One run_v0 training over the synthetic click log; the held-out clicks are then ranked once against the whole catalogue and once
against the news of the categories the user clicked in the training part, by the very call run_v0 --only_categories own makes
(train_eval.evaluate_retrieval), on the one trained model.  A held-out click outside the user's own categories is skipped by the
restricted call: its share is recorded.  The whole-catalogue figures are given twice: over all users, and over the users whose
held-out click lies inside their own categories (the population the restricted figures describe).  Every figure comes with its
standard error over users (std / sqrt(n)).  A target that is open to its user is asserted to rank no worse inside the set than
against the whole catalogue: that is a property, the figures are a record with no bar.
Usage: python tools/exp/exp_catalogue_tags.py [--json FILE] [--users N] [--epochs E]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from pytorch_news_recommender_amd import run_v0

NAMES = ("recall@10", "recall@100", "mrr")


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
        plain_kw = {k: v for k, v in kw.items() if k not in ("item_tag", "allow_tags")}
        plain = real_eval(config, model, data_iter, titles, y_true, **plain_kw)
        pm = dict(net.last_retrieval_metrics)
        own = real_eval(config, model, data_iter, titles, y_true, **kw)
        om = dict(net.last_retrieval_metrics)
        inside = om["ranks"] > 0
        assert bool((om["ranks"][inside] <= pm["ranks"][inside]).all()), "a rank inside the set exceeds the whole-catalogue one"
        assert bool((pm["ranks"][inside] > 0).all())
        kept = inside.any(dim=1)                                      # the users whose held-out click is open to them
        nan = torch.full_like(pm["mrr"], float("nan"))
        rec["whole catalogue, all users"] = {n: mean_se(pm[n]) for n in NAMES}
        rec["whole catalogue, users whose click is inside"] = {n: mean_se(torch.where(kept, pm[n], nan)) for n in NAMES}
        rec["own categories"] = {n: mean_se(om[n]) for n in NAMES}
        rec["counts"] = {"targets_whole": plain["n_targets"], "skipped_whole": plain["n_skipped"], "targets_own": own["n_targets"],
                         "skipped_own": own["n_skipped"], "closed_by_tag": own["n_closed"],
                         "share_closed": own["n_closed"] / max(1, plain["n_targets"]),
                         "ranks_lower_inside": int((om["ranks"][inside] < pm["ranks"][inside]).sum()),
                         "median_rank_whole_same_users": float(pm["ranks"][inside].double().median()),
                         "median_rank_own": float(om["ranks"][inside].double().median()),
                         "mean_rank_whole_same_users": float(pm["ranks"][inside].double().mean()),
                         "mean_rank_own": float(om["ranks"][inside].double().mean()),
                         "mean_open_categories": float(kw["allow_tags"].float().sum(dim=1).mean()),
                         "categories": int(kw["allow_tags"].shape[1])}
        return own

    run_v0.evaluate_retrieval = evaluate
    tmp = tempfile.mkdtemp()
    run_v0.main(["--model", "nrms_hip", "--dataset", "synthetic", "--negatives", "catalogue", "--retrieval_metrics", "10,100",
                 "--only_categories", "own", "--synthetic_users", str(users), "--epochs", str(epochs), "--precision", "fp16",
                 "--num_workers", "0", "--description", "tags", "--data_path", os.path.join(tmp, "data"),
                 "--save_path", os.path.join(tmp, "save")])
    print("| ranked against | Recall@10 | Recall@100 | MRR | users |")
    print("|---|---|---|---|---|")
    for name in ("whole catalogue, all users", "whole catalogue, users whose click is inside", "own categories"):
        r = rec[name]
        print("| %s | %s | %d |" % (name, " | ".join("%.4f ± %.4f" % (r[n]["mean"], r[n]["se"]) for n in NAMES), r["mrr"]["n"]))
    print(rec["counts"])
    if out:
        with open(out, "w") as f:
            json.dump({"date": time.strftime("%Y-%m-%d"), "parity": "unpinned (the reference has no catalogue retrieval)", "users": users,
                       "epochs": epochs, "news": 4000, "rows": rec}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
