"""Numpy restatement of nrms_negative_sample (include/nrms_hip.h, "Impression log") on top of tests/philox_ref.py, independent of
the library.  ``sample_impression`` is the contract read aloud for ONE impression; ``negative_sample`` is the same for a whole
log without a Python loop (one lexsort), for logs of millions of impressions; tests/test_negsample_host.py holds the two against
each other."""
import numpy as np

from tests.philox_ref import MASK64, words32

SITE = 6                                         # PHILOX_SITE_NEG_SAMPLE (csrc/common.h)
EPOCH_SEED_STEP = 0x9E3779B97F4A7C15
MAX_SHOWN = 2048


def epoch_seed(seed, epoch):
    """data_handler.ImpressionFeed.epoch_seed."""
    return (int(seed) + int(epoch) * EPOCH_SEED_STEP) & MASK64


def words(seed, nnz):
    """uint64 [nnz]: w(e) = word e & 3 of philox4x32_7(seed, e >> 2, site 6) for every position e of the log."""
    return words32(seed, SITE, (int(nnz) + 3) // 4 * 4)[:int(nnz)]


def sample_impression(shown, label, w, S):
    """One impression (its ids, labels and words) -> [[positive, negatives ...], ...], one list per positive in shown order."""
    shown, label = [int(v) for v in shown], [int(v) for v in label]
    negatives = [j for j in range(len(shown)) if label[j] == 0]
    ranked = sorted(negatives, key=lambda j: (int(w[j]), j))                 # r(j) = index in this list
    positives = [j for j in range(len(shown)) if label[j] != 0]
    return [[shown[j]] + [shown[k] for k in ranked[p * S:(p + 1) * S]] for p, j in enumerate(positives)]


def sample_ptr_of(imp_ptr, label):
    imp_ptr, label = np.asarray(imp_ptr, dtype=np.int64), np.asarray(label)
    imp_of = np.repeat(np.arange(len(imp_ptr) - 1, dtype=np.int64), np.diff(imp_ptr))
    n_pos = np.bincount(imp_of[label != 0], minlength=len(imp_ptr) - 1).astype(np.int64)
    return np.concatenate([[0], np.cumsum(n_pos)]).astype(np.int64)


def negative_sample(imp_ptr, shown, label, S, seed, max_shown=MAX_SHOWN):
    """-> (cand [n_samples, S + 1] int64, clen [n_samples] int64, n_bad)."""
    imp_ptr, shown, label = np.asarray(imp_ptr, dtype=np.int64), np.asarray(shown, dtype=np.int64), np.asarray(label)
    n_imp, nnz = len(imp_ptr) - 1, int(imp_ptr[-1])
    lens = np.diff(imp_ptr)
    imp_of = np.repeat(np.arange(n_imp, dtype=np.int64), lens)
    j = np.arange(nnz, dtype=np.int64) - imp_ptr[imp_of]
    pos = label != 0
    w = words(seed, nnz)
    sample_ptr = sample_ptr_of(imp_ptr, label)
    n_pos = np.diff(sample_ptr)
    too_long = lens > max_shown
    cand = np.zeros((int(sample_ptr[-1]), S + 1), dtype=np.int64)
    at = np.flatnonzero(pos)                                                  # positives in log order = in row order
    row_imp = imp_of[at]
    cand[:, 0] = shown[at]
    neg = np.flatnonzero(~pos & ~too_long[imp_of])
    neg = neg[np.lexsort((j[neg], w[neg], imp_of[neg]))]                      # by impression, then word, then position
    neg_imp = imp_of[neg]
    n_neg = np.bincount(neg_imp, minlength=n_imp).astype(np.int64)
    r = np.arange(len(neg), dtype=np.int64) - (np.cumsum(n_neg) - n_neg)[neg_imp]
    p = r // S
    keep = p < n_pos[neg_imp]
    cand[sample_ptr[neg_imp[keep]] + p[keep], 1 + r[keep] - p[keep] * S] = shown[neg[keep]]
    p_row = np.arange(len(at), dtype=np.int64) - sample_ptr[row_imp]
    clen = 1 + np.clip(n_neg[row_imp] - p_row * S, 0, S)
    return cand, clen.astype(np.int64), int(too_long.sum())


def random_log(lens, rng, n_news=5000, p_pos=0.12, force=None):
    """A log of impressions of the given lengths with random ids and labels.  force: {impression: label list} overrides."""
    lens = np.asarray(lens, dtype=np.int64)
    imp_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(imp_ptr[-1])
    shown = rng.integers(1, n_news, size=nnz).astype(np.int32)
    label = (rng.random(nnz) < p_pos).astype(np.uint8)
    for i, y in (force or {}).items():
        assert len(y) == lens[i]
        label[imp_ptr[i]:imp_ptr[i + 1]] = y
    return imp_ptr, shown, label
