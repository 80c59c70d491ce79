"""Does the held-out NLL separate settings that Recall@K cannot?  (docs/EXPERIMENTS.md)

One run_v0 training (row-wise loss, catalogue negatives, 3 epochs) over the synthetic click log of 4 000 news.  The held-out clicks
are then scored (a) by the very call run_v0 --retrieval_nll makes, over a grid of temperatures T, and (b) over a grid of ALPHA,
the amount of log-popularity put back at serving time, in ONE pass per batch: Model.log_prob with item_bias =
ClickFeed.popularity_prior(1) and bias_scale = the ALPHA grid.  Recall@10 / @100 per ALPHA come from evaluate_retrieval with
item_bias = popularity_prior(ALPHA), as in tools/exp/exp_popularity_prior.py.  A record, no bar.
Usage: python tools/exp/exp_retrieval_nll.py [--json FILE] [--users N] [--epochs E]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from pytorch_news_recommender_amd import run_v0
from pytorch_news_recommender_amd.train_eval import _inner

TEMPS = (0.05, 0.1, 0.25, 0.5, 1.0, 2.0, 4.0, float("inf"))
ALPHAS = (0.0, 0.125, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0)


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
    feeds, real_feed, real_eval = [], run_v0.ClickFeed, run_v0.evaluate_retrieval
    rec = {}

    def click_feed(*a, **kw):
        feeds.append(real_feed(*a, **kw))
        return feeds[-1]

    def evaluate(config, model, data_iter, titles, y_true, **kw):
        res = real_eval(config, model, data_iter, titles, y_true, **kw)                  # (a): nll over the T grid
        rec["temperature"] = [dict(T=t, nll=v) for t, v in res["nll"].items()]
        rec["plain"] = {k: res[k] for k in ("recall@10", "recall@100", "mrr", "median_rank", "n_targets")}
        net = _inner(model)
        targets = net.last_retrieval_metrics["targets"]
        ranked = net.last_retrieval_metrics["ranks"] > 0
        best_t = min(res["nll"], key=res["nll"].get)
        prior = feeds[-1].popularity_prior(1.0)
        cat = net.encode_catalogue(titles, **(kw.get("news_info") or {}))
        total, done = torch.zeros(len(ALPHAS), dtype=torch.float64, device=cat.device), 0
        for batch in data_iter:                                                         # (b): nll over the ALPHA grid, one pass
            B = batch["browsed_ids"].shape[0]
            lp = net.log_prob(batch, targets[done:done + B], cat, [best_t] * len(ALPHAS), item_bias=prior, bias_scale=list(ALPHAS))
            total -= torch.where(ranked[done:done + B].unsqueeze(-1), lp, torch.zeros_like(lp)).double().sum(dim=(0, 1))
            done += B
        nll = (total / ranked.sum()).cpu().tolist()
        rows = []
        for alpha, v in zip(ALPHAS, nll):
            kw2 = dict(kw, item_bias=feeds[-1].popularity_prior(alpha), verbose=False)
            kw2.pop("nll_temperatures", None)
            r = real_eval(config, model, data_iter, titles, y_true, **kw2)
            rows.append(dict(alpha=alpha, T=best_t, nll=v, **{k: r[k] for k in ("recall@10", "recall@100", "mrr", "median_rank")}))
        rec["alpha"] = rows
        return res

    run_v0.ClickFeed, run_v0.evaluate_retrieval = click_feed, evaluate
    tmp = tempfile.mkdtemp()
    run_v0.main(["--model", "nrms_hip", "--dataset", "synthetic", "--negatives", "catalogue", "--retrieval_metrics", "10,100",
                 "--retrieval_nll", ",".join("%g" % t for t in TEMPS), "--synthetic_users", str(users), "--epochs", str(epochs),
                 "--precision", "fp16", "--loss", "rowwise", "--num_workers", "0", "--description", "retrieval_nll",
                 "--data_path", os.path.join(tmp, "data"), "--save_path", os.path.join(tmp, "save")])
    print("| T | nll |\n|---|---|")
    for r in rec["temperature"]:
        print("| %g | %.4f |" % (r["T"], r["nll"]))
    print("| ALPHA | nll at T=%g | Recall@10 | Recall@100 | MRR | median rank |\n|---|---|---|---|---|---|" % rec["alpha"][0]["T"])
    for r in rec["alpha"]:
        print("| %g | %.4f | %.4f | %.4f | %.4f | %.0f |" % (r["alpha"], r["nll"], r["recall@10"], r["recall@100"], r["mrr"], r["median_rank"]))
    if out:
        with open(out, "w") as f:
            json.dump(dict(rec, date=time.strftime("%Y-%m-%d"), users=users, epochs=epochs), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
