"""Retrieval quality inside and outside a time window of the catalogue (docs/EXPERIMENTS.md).

One run_v0 training over the timed synthetic click log (--catalogue_window gives the log its ticks); the held-out clicks are then
ranked once against the whole catalogue and once per SPAN against the news first clicked in the SPAN ticks up to the moment of the
held-out click, by the very call run_v0 --catalogue_window SPAN makes (train_eval.evaluate_retrieval), on the one trained model.
A target that is eligible inside its window is asserted to rank no worse there than against the whole catalogue: that is a
property, the figures are a record with no bar.
Usage: python tools/exp/exp_catalogue_window.py [--json FILE] [--users N] [--epochs E]"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from pytorch_news_recommender_amd import run_v0

SPANS = (None, 50000, 20000, 5000)


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
    rows = []

    def evaluate(config, model, data_iter, titles, y_true, **kw):
        net = model.model if hasattr(model, "model") else model
        res, plain = None, None
        for span in SPANS:
            args = dict(kw)
            if span is None:
                for name in ("item_time", "request_time", "window_span"):
                    args.pop(name)
            else:
                args["window_span"] = span
            res = real_eval(config, model, data_iter, titles, y_true, **args)
            ranks = net.last_retrieval_metrics["ranks"]
            if span is None:
                plain = ranks
            else:
                inside = ranks > 0
                assert bool((ranks[inside] <= plain[inside]).all()), "a windowed rank exceeds the unwindowed one"
                assert bool((plain[inside] > 0).all())
            rows.append(dict(res, window_span=span))
        return res

    run_v0.evaluate_retrieval = evaluate
    tmp = tempfile.mkdtemp()
    run_v0.main(["--model", "nrms_hip", "--dataset", "synthetic", "--negatives", "catalogue", "--retrieval_metrics", "10,100",
                 "--synthetic_users", str(users), "--epochs", str(epochs), "--precision", "fp16", "--catalogue_window", "1",
                 "--num_workers", "0", "--description", "window", "--data_path", os.path.join(tmp, "data"),
                 "--save_path", os.path.join(tmp, "save")])
    print("| SPAN | Recall@10 | Recall@100 | nDCG@10 | MRR | median rank | targets | skipped |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.4f | %.4f | %.4f | %.4f | %.0f | %d | %d |" % ("none" if r["window_span"] is None else r["window_span"], r["recall@10"],
                                                                       r["recall@100"], r["ndcg@10"], r["mrr"], r["median_rank"],
                                                                       r["n_targets"], r["n_skipped"]))
    if out:
        with open(out, "w") as f:
            json.dump({"date": time.strftime("%Y-%m-%d"), "users": users, "epochs": epochs, "news": 4000,
                       "spans": ["none" if s is None else s for s in SPANS], "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
