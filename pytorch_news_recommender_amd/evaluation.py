"""The MIND scores with the reference's signatures (/root/reference/MIND_2020/evaluation.py:6-27): ``auc_score``,
``dcg_score``, ``ndcg_score``, ``mrr_score``, and ``score_submission``, the leaderboard scorer the reference keeps
commented out (evaluation.py:29-117).

``auc_score`` is what ``evaluate`` reports (train_eval.py:219-227); the reference delegates to
sklearn.metrics.roc_auc_score -- here it is the same Mann-Whitney statistic in numpy float64.  The ranking
metrics are host restatements in float64.  On the device all four are one HIP kernel,
``nrms_impression_metrics`` (train_eval.evaluate_metrics, test() and score_submission); ``nrms_impression_auc``
serves ``evaluate``.

Tie rule of MRR and nDCG: among equal scores the LATER slot ranks first, i.e. the reference's
``np.argsort(y_score)[::-1]`` with a stable sort (NumPy's default sort is not stable, so the reference's own
result on tied scores depends on the NumPy build).  The rule is stated once, for host and device, in
include/nrms_hip.h at nrms_impression_metrics."""
import json

import numpy as np


def auc_score(y_true, y_pred):
    y_true = np.asarray(y_true)
    s = np.asarray(y_pred, dtype=np.float64)
    pos, neg = s[y_true == 1], s[y_true != 1]
    if pos.size == 0 or neg.size == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    neg_sorted = np.sort(neg)
    greater = np.searchsorted(neg_sorted, pos, side="left")          # negatives strictly below each positive
    equal = np.searchsorted(neg_sorted, pos, side="right") - greater
    return float((greater.sum() + 0.5 * equal.sum()) / (pos.size * neg.size))


def _metric_ranks(y_score):
    """rank_m (1 = best) of every slot: descending score, the later slot first among equal scores."""
    order = np.argsort(np.asarray(y_score, dtype=np.float64), kind="stable")[::-1]
    ranks = np.empty(order.size, dtype=np.int64)
    ranks[order] = np.arange(1, order.size + 1)
    return ranks


def dcg_score(y_true, y_score, k=10):
    """Discounted cumulative gain of the top k: sum over slots with rank_m <= k of (2^y - 1) / log2(rank_m + 1)."""
    y = np.asarray(y_true, dtype=np.float64)
    r = _metric_ranks(y_score)
    top = r <= k
    return float(np.sum((np.exp2(y[top]) - 1.0) / np.log2(r[top] + 1.0)))


def ndcg_score(y_true, y_score, k=10):
    """dcg_score over the dcg of the ideal order; NaN when y_true has no positive (the reference's 0 / 0)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(dcg_score(y_true, y_score, k)) / np.float64(dcg_score(y_true, y_true, k)))


def mrr_score(y_true, y_score):
    """Mean reciprocal rank of the positives: sum y / rank_m over sum y; NaN when y_true has no positive."""
    y = np.asarray(y_true, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.sum(y / _metric_ranks(y_score)) / np.sum(y))


def _lines(f):
    if hasattr(f, "readline"):
        return f.read().splitlines()
    with open(f) as fh:
        return fh.read().splitlines()


def _parse_line(line, line_no, what):
    parts = line.split()
    try:
        if len(parts) != 2:
            raise ValueError
        values = json.loads(parts[1])
        if not isinstance(values, list) or not all(isinstance(v, int) and not isinstance(v, bool) for v in values):
            raise ValueError
    except ValueError:
        raise ValueError("line-{}: invalid {} line {!r}".format(line_no, what, line)) from None
    return parts[0], values


def read_submission(truth_file, prediction_file):
    """Parse a truth file (``impid [labels]`` per line) and a prediction file (``impid [ranks]``, the format test()
    writes) line by line, as the reference's scorer does: an impression with empty labels is skipped, a missing or
    empty prediction line counts as all ranks 1, the score of a rank is 1 / rank.  Raises ValueError on a malformed
    line, an impression-id mismatch, a rank list of the wrong length or a rank outside 1..len.
    Returns padded numpy arrays (scores f32 [n, Cmax], labels u8 [n, Cmax], lens i32 [n])."""
    truth, pred = _lines(truth_file), _lines(prediction_file)
    rows = []
    for idx, lt in enumerate(truth):
        line_no = idx + 1
        impid, labels = _parse_line(lt, line_no, "truth")
        ls = pred[idx] if idx < len(pred) else ""
        if not labels:
            continue
        if ls.strip() == "":
            sub_impid, sub_ranks = impid, [1] * len(labels)
        else:
            sub_impid, sub_ranks = _parse_line(ls, line_no, "prediction")
        if sub_impid != impid:
            raise ValueError("line-{}: inconsistent impression id {} and {}".format(line_no, sub_impid, impid))
        if len(sub_ranks) != len(labels):
            raise ValueError("line-{}: {} ranks for {} labels".format(line_no, len(sub_ranks), len(labels)))
        if any(r < 1 or r > len(labels) for r in sub_ranks):
            raise ValueError("line-{}: ranks must be integers from 1 to {}".format(line_no, len(labels)))
        rows.append((labels, sub_ranks))
    max_c = max([len(lab) for lab, _ in rows] + [1])
    scores = np.zeros((len(rows), max_c), dtype=np.float32)
    lab = np.zeros((len(rows), max_c), dtype=np.uint8)
    lens = np.zeros(len(rows), dtype=np.int32)
    for i, (labels, ranks) in enumerate(rows):
        n = len(labels)
        scores[i, :n] = 1.0 / np.asarray(ranks, dtype=np.float64)    # distinct ranks stay distinct (and ordered) in f32
        lab[i, :n] = np.asarray(labels) != 0
        lens[i] = n
    return scores, lab, lens


def score_submission(truth_file, prediction_file):
    """The reference's leaderboard scorer (evaluation.py:29-117): (auc, mrr, ndcg5, ndcg10), each the mean over the
    scored impressions, computed on the GPU by nrms_impression_metrics.  An impression whose labels hold one class
    only has an undefined AUC (NaN, where sklearn raises), and the mean is then NaN.  Input rules: read_submission."""
    import torch
    from . import _lib
    from .engine import impression_metrics
    scores, lab, lens = read_submission(truth_file, prediction_file)
    dev = torch.device("cuda")
    m = impression_metrics(_lib.load(), dev, torch.from_numpy(scores).to(dev), torch.from_numpy(lab).to(dev),
                           torch.from_numpy(lens).to(dev), ks=(5, 10))
    return tuple(float(v) for v in torch.stack([m[k].mean() for k in ("auc", "mrr", "ndcg@5", "ndcg@10")]).cpu())
