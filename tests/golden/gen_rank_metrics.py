#!/usr/bin/env python3
"""Generate g8_rank_metrics.npz by running the IMPORTED REFERENCE's metric functions on CPU.

Run only in the build container (it needs /root/reference, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_rank_metrics.py

  g8_rank_metrics.npz  64 padded impressions (``scores`` f32 [64, 300], ``labels`` u8, ``lens`` i32) and, per
                impression, the reference's ``auc_score`` (NaN where sklearn refuses a single class), ``mrr_score``,
                ``ndcg_score(k=5)`` and ``ndcg_score(k=10)`` (evaluation.py:6-27).  Rows 0..31 are tie-free, rows
                32..63 carry ties, some of them between a positive and a negative across ranks 5 and 10.  Lengths
                include 1, 2, 5, 6, 10, 11, 63, 64, 65 and 300; there are all-negative and all-positive rows.

The reference ranks with ``np.argsort(y_score)[::-1]``, and NumPy's default sort is not stable, so its result on tied
scores depends on the NumPy build.  The values here are computed with the module's ``np`` replaced by a shim whose
``argsort`` is ``kind="stable"`` (the tie rule of include/nrms_hip.h nrms_impression_metrics); on the tie-free rows the
shim is checked to change nothing.  The reference is imported, never copied.
"""
import os
import sys
import warnings

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/MIND_2020"
MAX_C = 300
LENGTHS = [1, 2, 5, 6, 10, 11, 63, 64, 65, 300]


class StableArgsortNumpy:
    """numpy, except that argsort is stable."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kwargs):
        kwargs["kind"] = "stable"
        return np.argsort(a, *args, **kwargs)


def make_rows():
    rng = np.random.default_rng(2024)
    rows = []                                        # (scores f32, labels u8)
    # rows 0..31: tie-free
    lens = LENGTHS * 3 + [7, 40]
    for i, n in enumerate(lens):
        while True:
            s = rng.standard_normal(n).astype(np.float32)
            if np.unique(s).size == n:
                break
        y = (rng.random(n) < 0.25).astype(np.uint8)
        if n > 1 and i < 20 and y.sum() == 0:
            y[rng.integers(n)] = 1
        rows.append((s, y))
    rows[10] = (rows[10][0], np.zeros(len(rows[10][0]), np.uint8))           # n = 1, all negative
    rows[13] = (rows[13][0], np.zeros(len(rows[13][0]), np.uint8))           # n = 6, all negative
    rows[17] = (rows[17][0], np.zeros(len(rows[17][0]), np.uint8))           # n = 64, all negative
    rows[12] = (rows[12][0], np.ones(len(rows[12][0]), np.uint8))            # n = 5, all positive
    rows[15] = (rows[15][0], np.ones(len(rows[15][0]), np.uint8))            # n = 11, all positive
    rows[20] = (rows[20][0], np.ones(len(rows[20][0]), np.uint8))            # n = 1, all positive
    # rows 32..63: ties (scores on a coarse grid)
    for i, n in enumerate(LENGTHS * 3 + [12, 16]):
        s = (np.round(rng.standard_normal(n) * 2.0) / 2.0).astype(np.float32)
        y = (rng.random(n) < 0.3).astype(np.uint8)
        if n > 1 and y.sum() == 0:
            y[rng.integers(n)] = 1
        rows.append((s, y))
    # tie groups between a positive and a negative that straddle rank 5 (ranks 4..6) and rank 10 (ranks 9..11)
    crafted = [
        ([9, 8, 7, 5, 5, 5, 4, 3, 2, 2, 2, 1], [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0]),
        ([9, 8, 7, 5, 5, 5, 4, 3, 2, 2, 2, 1], [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]),
        ([5, 9, 5, 8, 7, 5, 4, 2, 3, 2, 1, 2, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0]),
        ([1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1] + [0] * 8),
    ]
    for r, (s, y) in enumerate(crafted):
        rows[60 + r] = (np.asarray(s, np.float32), np.asarray(y, np.uint8))
    rows[42] = (rows[42][0], np.zeros(len(rows[42][0]), np.uint8))           # ties, all negative (n = 1)
    rows[44] = (np.full(5, 0.5, np.float32), np.ones(5, np.uint8))           # ties, all positive (n = 5)
    assert len(rows) == 64
    return rows


def main():
    assert os.path.isdir(REF), "reference not present: fixtures can only be generated in the build container"
    sys.path.insert(0, REF)
    ev = __import__("evaluation")
    rows = make_rows()
    n_imp = len(rows)
    scores = np.zeros((n_imp, MAX_C), np.float32)
    labels = np.zeros((n_imp, MAX_C), np.uint8)
    lens = np.zeros(n_imp, np.int32)
    for i, (s, y) in enumerate(rows):
        scores[i, :len(s)] = s
        labels[i, :len(s)] = y
        lens[i] = len(s)
    assert set(LENGTHS) <= set(lens.tolist())

    def ref_values(i):
        n = lens[i]
        y, s = labels[i, :n].astype(np.int64), scores[i, :n].astype(np.float64)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")              # newer sklearn warns and returns NaN instead of raising
                auc = ev.auc_score(y, s)
        except ValueError:
            auc = np.nan
        with np.errstate(invalid="ignore", divide="ignore"):
            return auc, ev.mrr_score(y, s), ev.ndcg_score(y, s, k=5), ev.ndcg_score(y, s, k=10)

    plain = np.array([ref_values(i) for i in range(32)], dtype=np.float64)
    orig_np = ev.np
    ev.np = StableArgsortNumpy()
    try:
        vals = np.array([ref_values(i) for i in range(n_imp)], dtype=np.float64)
    finally:
        ev.np = orig_np
    # the shim changes nothing where there is no tie
    assert np.array_equal(plain, vals[:32], equal_nan=True)
    for i in range(32):
        assert np.unique(scores[i, :lens[i]]).size == lens[i]
    ties = [i for i in range(32, n_imp) if np.unique(scores[i, :lens[i]]).size < lens[i]]
    assert len(ties) >= 24, ties
    np.savez_compressed(os.path.join(HERE, "g8_rank_metrics.npz"), scores=scores, labels=labels, lens=lens,
                        auc=vals[:, 0], mrr=vals[:, 1], ndcg5=vals[:, 2], ndcg10=vals[:, 3])
    print("g8", n_imp, "impressions; nan auc / mrr:", int(np.isnan(vals[:, 0]).sum()), int(np.isnan(vals[:, 1]).sum()))


if __name__ == "__main__":
    main()
