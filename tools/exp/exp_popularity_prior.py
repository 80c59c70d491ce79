"""Retrieval quality against the amount of popularity prior put back at serving time (docs/EXPERIMENTS.md).

One run_v0 training per loss (row-wise, pooled with the logQ correction) over the synthetic click log, 3 epochs; the held-out
clicks are then ranked against the whole catalogue once per ALPHA with item_bias = ClickFeed.popularity_prior(ALPHA), by the
very call run_v0 --popularity_prior ALPHA makes (train_eval.evaluate_retrieval), on the one trained model.  A record, no bar.
Usage: python tools/exp/exp_popularity_prior.py [--json FILE] [--users N] [--epochs E]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from pytorch_news_recommender_amd import run_v0

ALPHAS = (0.0, 0.25, 0.5, 1.0)


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

    def click_feed(*a, **kw):
        feeds.append(real_feed(*a, **kw))
        return feeds[-1]

    rows = []

    def evaluate(config, model, data_iter, titles, y_true, **kw):
        res = None
        for alpha in ALPHAS:
            kw["item_bias"] = feeds[-1].popularity_prior(alpha)
            res = real_eval(config, model, data_iter, titles, y_true, **kw)
            rows.append(dict(res, alpha=alpha, loss=loss))
        return res

    run_v0.ClickFeed, run_v0.evaluate_retrieval = click_feed, evaluate
    tmp = tempfile.mkdtemp()
    for loss in ("rowwise", "pooled"):
        run_v0.main(["--model", "nrms_hip", "--dataset", "synthetic", "--negatives", "catalogue", "--retrieval_metrics", "10,100",
                     "--synthetic_users", str(users), "--epochs", str(epochs), "--precision", "fp16", "--loss", loss,
                     "--popularity_prior", "0", "--num_workers", "0", "--description", "prior_" + loss,
                     "--data_path", os.path.join(tmp, "data"), "--save_path", os.path.join(tmp, "save_" + loss)])
    print("| loss | ALPHA | Recall@10 | Recall@100 | nDCG@10 | MRR | median rank |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %g | %.4f | %.4f | %.4f | %.4f | %.0f |" % (r["loss"], r["alpha"], r["recall@10"], r["recall@100"], r["ndcg@10"],
                                                                  r["mrr"], r["median_rank"]))
    if out:
        with open(out, "w") as f:
            json.dump({"date": time.strftime("%Y-%m-%d"), "users": users, "epochs": epochs, "alphas": list(ALPHAS), "rows": rows}, f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
