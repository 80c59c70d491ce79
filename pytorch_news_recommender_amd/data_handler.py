"""Online data feed: the batch-dict contract of the reference's ``MyDataset``
(/root/reference/MIND_2020/data_handler.py:161-250) without its numpy-1 ``np.int`` (removed in
numpy 2) and without pandas/nltk at import time.

A *sample* is the tuple the reference indexes positionally (data_handler.py:206-231):
    sample[0] history news ids (1-based, 0 = pad)      sample[3] impression news ids
    sample[1] history category ids                      sample[4] impression category ids
    sample[2] history sub-category ids                  sample[5] impression sub-category ids
``id2title_dict[news_id - 1]`` is the padded word-id list of a title (data_handler.py:212).
Only the keys the NRMS path reads are always filled; abstract / category keys are emitted (zeros
unless the dictionaries are given) so the collated dict has the reference's full key set.

MIND itself is not available offline, so ``SyntheticMind`` fabricates a corpus + behaviours with
the same structure; ``load_dataset`` / ``get_Words_Infos`` / ``read_dev_labels`` / ``get_Test_List`` read the
files the reference's own preprocessing writes under ``config.data_path`` when they exist (the user's own
data: nothing of the kind ships with the reference).
"""
from __future__ import annotations

import csv
import os
import pickle
from ast import literal_eval
from collections.abc import Mapping

import numpy as np
import torch
from torch.utils.data import Dataset


def _words_infos(config, title_pkl, abst_pkl, words_csv):
    """news index -> padded word-id list, for titles and abstracts: the pickled dicts when they exist, otherwise
    built from the headerless ``news_id,title,abstract`` csv (list literals) and cached as pickles, exactly as
    the reference does (data_handler.py:113-135)."""
    base = config.data_path
    tp, ap = os.path.join(base, title_pkl), os.path.join(base, abst_pkl)
    if os.path.exists(tp):
        with open(tp, 'rb') as f:
            title_dict = pickle.load(f)
        abst_dict = None
        if os.path.exists(ap):
            with open(ap, 'rb') as f:
                abst_dict = pickle.load(f)
        return title_dict, abst_dict
    src = os.path.join(base, words_csv)
    if not os.path.exists(src):
        raise FileNotFoundError("neither %s nor %s exists: run the reference's data_processor first, or pass "
                                "id2title_dict / use --dataset synthetic" % (tp, src))
    title_dict, abst_dict = {}, {}
    csv.field_size_limit(1 << 30)
    with open(src, newline='') as f:
        for i, row in enumerate(csv.reader(f)):          # columns: news_id, title, abstract (no header)
            title_dict[i] = literal_eval(row[1])
            abst_dict[i] = literal_eval(row[2])
    with open(tp, 'wb') as f:
        pickle.dump(title_dict, f)
    with open(ap, 'wb') as f:
        pickle.dump(abst_dict, f)
    return title_dict, abst_dict


def get_Words_Infos(config):
    """data_handler.py:113-135."""
    return _words_infos(config, 'news_title.pkl', 'news_abst.pkl', 'news_words.csv')


def get_Demo_Words_Infos(config):
    """data_handler.py:137-159."""
    return _words_infos(config, 'demo_news_title.pkl', 'demo_news_abst.pkl', 'demo_news_words.csv')


def read_dev_labels(config, file=None):
    """Per-impression 0/1 label lists from the ``y_true`` column (space-separated) of dev_behaviors.csv
    (train_eval.py:36-39; demo mode: small_dev_behaviors.csv, train_eval.py:156-158)."""
    if file is None:
        file = 'small_dev_behaviors.csv' if getattr(config, 'mode', 'large') == 'demo' else 'dev_behaviors.csv'
    path = os.path.join(config.data_path, file)
    csv.field_size_limit(1 << 30)
    with open(path, newline='') as f:
        return [[int(v) for v in row['y_true'].split(' ')] for row in csv.DictReader(f)]


def get_Test_List(config):
    """Number of shown candidates per test impression (train_eval.py:287-298): the cached
    test_imps_list.pkl, or counted from the 4th (impressions) column of test/behaviors.tsv and cached."""
    cache = os.path.join(config.data_path, 'test_imps_list.pkl')
    if os.path.exists(cache):
        with open(cache, 'rb') as f:
            return pickle.load(f)
    lens = []
    with open(os.path.join(config.test_path, 'behaviors.tsv')) as f:
        for line in f:
            cols = line.rstrip('\n').split('\t')
            lens.append(len(cols[-1].split(' ')))
    with open(cache, 'wb') as f:
        pickle.dump(lens, f)
    return lens


class MyDataset(Dataset):
    def __init__(self, config, datas, type=0, id2title_dict=None, id2abst_dict=None):
        super().__init__()
        self.config = config
        self.data_type = type
        self.bacthes = datas                       # (sic) attribute name of the reference
        if id2title_dict is None:
            # the reference's constructor (data_handler.py:162-170): the word dictionaries come from config.data_path
            if getattr(config, 'mode', 'large') == 'demo':
                id2title_dict, id2abst_dict = get_Demo_Words_Infos(config)
            else:
                id2title_dict, id2abst_dict = get_Words_Infos(config)
        self.id2title_dict = id2title_dict
        self.id2abst_dict = id2abst_dict
        # training: 1 positive + sample_size negatives; evaluation: padded to max_candidate_size
        self.sample_size = config.sample_size + 1 if type < 1 else config.max_candidate_size   # :174-177

    def __len__(self):
        return len(self.bacthes)

    def __getitem__(self, index):
        cfg = self.config
        data = self.bacthes[index]
        H, L, A, S = cfg.history_len, cfg.n_words_title, cfg.n_words_abst, self.sample_size
        i64 = np.int64
        browsed_ids = np.zeros(H, dtype=i64)
        browsed_titles = np.zeros((H, L), dtype=i64)
        browsed_absts = np.zeros((H, A), dtype=i64)
        browsed_categ_ids = np.zeros(H, dtype=i64)
        browsed_subcateg_ids = np.zeros(H, dtype=i64)
        candidate_ids = np.zeros(S, dtype=i64)
        candidate_titles = np.zeros((S, L), dtype=i64)
        candidate_absts = np.zeros((S, A), dtype=i64)
        candidate_categ_ids = np.zeros(S, dtype=i64)
        candidate_subcateg_ids = np.zeros(S, dtype=i64)

        hist = list(data[0])[:H]
        x = len(hist)
        browsed_ids[:x] = hist
        browsed_mask = torch.zeros(H, dtype=torch.uint8)
        browsed_mask[:x] = 1
        if x:
            browsed_titles[:x] = np.asarray([self.id2title_dict[i - 1] for i in hist], dtype=i64)[:, :L]
            if self.id2abst_dict is not None:
                browsed_absts[:x] = np.asarray([self.id2abst_dict[i - 1] for i in hist], dtype=i64)[:, :A]
            if len(data) > 2 and data[1] is not None:
                browsed_categ_ids[:x] = np.asarray(data[1])[:x]
                browsed_subcateg_ids[:x] = np.asarray(data[2])[:x]

        imps = list(data[3])[:S]
        y = len(imps)
        candidate_ids[:y] = imps
        if y:
            candidate_titles[:y] = np.asarray([self.id2title_dict[i - 1] for i in imps], dtype=i64)[:, :L]
            if self.id2abst_dict is not None:
                candidate_absts[:y] = np.asarray([self.id2abst_dict[i - 1] for i in imps], dtype=i64)[:, :A]
            if len(data) > 5 and data[4] is not None:
                ss = min(len(data[4]), S)
                candidate_categ_ids[:ss] = np.asarray(data[4])[:ss]
                candidate_subcateg_ids[:ss] = np.asarray(data[5])[:ss]
        candidate_mask = torch.zeros(S, dtype=torch.uint8)
        candidate_mask[:y] = 1

        return {'browsed_lens': x,
                'browsed_ids': browsed_ids,
                'browsed_titles': browsed_titles,
                'browsed_absts': browsed_absts,
                'browsed_categ_ids': browsed_categ_ids,
                'browsed_subcateg_ids': browsed_subcateg_ids,
                'browsed_mask': browsed_mask,
                'candidate_ids': candidate_ids,
                'candidate_titles': candidate_titles,
                'candidate_absts': candidate_absts,
                'candidate_categ_ids': candidate_categ_ids,
                'candidate_subcateg_ids': candidate_subcateg_ids,
                'candidate_mask': candidate_mask}


def load_dataset(config, file, path, _type=0):
    """Index lists from the reference's preprocessed pickles (data_handler.py:43-110 caches them as
    ``idx_<file>``).  Only the cached, already-indexed form is read here: rebuilding it needs the
    MIND tsv files and the reference's offline ETL (data_processor.py), which is out of scope."""
    cache = os.path.join(path, 'idx_' + file)
    if not os.path.exists(cache):
        raise FileNotFoundError(
            "%s not found: run the reference's data_processor / load_dataset once to build it, or use "
            "--dataset synthetic" % cache)
    with open(cache, 'rb') as f:
        return pickle.load(f)


def seen_adjustment(seen_ptr, seen_ids, beta, max_slots, device=None):
    """Impression discounting as ``Model.recommend_adjusted``'s ``adjust``: a per-user CSR of seen-but-not-clicked news ->
    ``(ids int64 [n_users, max_slots], delta float32 [n_users, max_slots])``.  seen_ids[seen_ptr[u]:seen_ptr[u + 1]] are the news
    user u was shown; a news listed c times was seen c times and gets delta = -beta * c, in one slot.  A user with more than
    max_slots distinct news keeps the most-seen, ties to the smaller id; the slots of a row are in that order.  Unused slots hold
    id 0 / delta 0.0 (id 0 names no news).  Torch ops on ``device`` (default: seen_ids' own when it is a tensor, else the CPU)."""
    max_slots = int(max_slots)
    if not 0 <= max_slots <= 256:
        raise ValueError("seen_adjustment: max_slots = %r must be in [0, 256]" % (max_slots,))
    if device is None:
        device = seen_ids.device if torch.is_tensor(seen_ids) else "cpu"
    ptr = torch.as_tensor(seen_ptr).to(device, dtype=torch.int64).reshape(-1)
    news = torch.as_tensor(seen_ids).to(device, dtype=torch.int64).reshape(-1)
    if ptr.numel() < 1 or int(ptr[0]) != 0 or int(ptr[-1]) != news.numel() or bool((ptr[1:] < ptr[:-1]).any()):
        raise ValueError("seen_adjustment: seen_ptr must rise from 0 to len(seen_ids) = %d" % news.numel())
    n_users = ptr.numel() - 1
    ids = torch.zeros(n_users, max_slots, dtype=torch.int64, device=device)
    delta = torch.zeros(n_users, max_slots, dtype=torch.float32, device=device)
    if news.numel() == 0 or max_slots == 0:
        return ids, delta
    if int(news.min()) < 0:
        raise ValueError("seen_adjustment: news ids must be >= 0")
    span = int(news.max()) + 1
    user = torch.repeat_interleave(torch.arange(n_users, device=device), ptr[1:] - ptr[:-1])
    pair, count = torch.unique(user * span + news, return_counts=True)              # the distinct (user, news), and how often
    p_user, p_news = pair // span, pair % span
    top = int(count.max())
    order = torch.argsort((p_user * (top + 1) + (top - count)) * span + p_news)      # user, then most seen, then the smaller id
    p_user, p_news, count = p_user[order], p_news[order], count[order]
    first = torch.cumsum(torch.bincount(p_user, minlength=n_users), 0) - torch.bincount(p_user, minlength=n_users)
    place = torch.arange(p_user.numel(), device=device) - first[p_user]
    keep = place < max_slots
    ids[p_user[keep], place[keep]] = p_news[keep]
    delta[p_user[keep], place[keep]] = count[keep].to(torch.float32) * (-float(beta))
    return ids, delta


class SyntheticMind:
    """A MIND-shaped corpus + click behaviours with learnable structure: every news item and
    every user belongs to a latent topic; users click mostly in-topic news, and titles draw
    their words from topic-specific vocabularies -- so AUC rises above 0.5 when training works."""

    def __init__(self, config, n_news=2000, n_topics=8, seed=0, vocab=None):
        rng = np.random.default_rng(seed)
        self.config = config
        self.n_news = n_news
        V = int(vocab if vocab is not None else config.n_words)
        L = config.n_words_title
        self.topic = rng.integers(0, n_topics, size=n_news)
        span = (V - 1) // n_topics
        titles = np.zeros((n_news, L), dtype=np.int64)
        for i in range(n_news):
            n = int(rng.integers(min(5, L), L + 1))
            lo = 1 + self.topic[i] * span
            topical = rng.integers(lo, lo + span, size=n)
            noise = rng.integers(1, V, size=n)
            titles[i, :n] = np.where(rng.random(n) < 0.7, topical, noise)
        self.id2title_dict = {i: titles[i].tolist() for i in range(n_news)}
        # abstracts (same topical vocabulary, config.n_words_abst words) and category / sub-category ids for nrms_naml:
        # category = 1 + topic (0 is the padding slot), sub-category = a fixed refinement of it
        # (their own generator: the title / behaviour streams stay what they were before the abstracts existed)
        A = int(getattr(config, "n_words_abst", 40))
        absts = np.zeros((n_news, A), dtype=np.int64)
        rng2 = np.random.default_rng(seed + 1000003)
        for i in range(n_news):
            n = int(rng2.integers(min(8, A), A + 1))
            lo = 1 + self.topic[i] * span
            absts[i, :n] = np.where(rng2.random(n) < 0.6, rng2.integers(lo, lo + span, size=n), rng2.integers(1, V, size=n))
        self.id2abst_dict = {i: absts[i].tolist() for i in range(n_news)}
        n_cat, n_sub = int(getattr(config, "category_nums", 19)), int(getattr(config, "subcategory_nums", 294))
        self.category = 1 + self.topic % max(n_cat - 1, 1)
        self.subcategory = 1 + (self.topic * 7 + rng2.integers(0, 5, size=n_news)) % max(n_sub - 1, 1)
        self.n_topics = n_topics
        self.rng = rng
        self.imp_rng = np.random.default_rng(seed + 2000003)       # train_impressions' own stream, as the abstracts have theirs
        self.click_rng = np.random.default_rng(seed + 3000003)     # click_log's own stream
        self.tick_seed = seed + 4000003                            # click_ticks' own generator, made anew by every call
        self.by_topic = [np.flatnonzero(self.topic == t) + 1 for t in range(n_topics)]   # 1-based ids

    def embedding_table(self, d, seed=0):
        t = np.random.default_rng(seed).normal(0, 0.4, size=(self.config.n_words, d)).astype(np.float32)
        t[0] = 0
        return t

    def news_vectors(self, E, seed=0, noise=1.0):
        """Pretrained-style news vectors for nrms_bert: [n_news + 1, E] float32, row r = news id r (ids are 1-based; row 0,
        the padding slot's id, is noise only).  A news item's row is its topic's centroid (N(0, 1) per component) plus noise
        (N(0, noise^2)), so that ids of one topic are correlated and synthetic training can learn."""
        rng = np.random.default_rng(seed + 7919)
        centroids = rng.normal(0.0, 1.0, size=(self.n_topics, E))
        out = rng.normal(0.0, noise, size=(self.n_news + 1, E))
        out[1:] += centroids[self.topic]
        return out.astype(np.float32)

    def _pick(self, topic, n, p_in=0.8, rng=None):
        rng = self.rng if rng is None else rng
        out = []
        for _ in range(n):
            t = topic if rng.random() < p_in else int(rng.integers(0, self.n_topics))
            out.append(int(rng.choice(self.by_topic[t])))
        return out

    def train_samples(self, n_users):
        """[history, its categories, its sub-categories, [positive] + negatives, their categories, their sub-categories] per
        user (data_handler.py:40; positive first, as the CE-with-label-0 loss of train_eval.py:116-117 expects)."""
        cfg = self.config
        samples = []
        for _ in range(n_users):
            t = int(self.rng.integers(0, self.n_topics))
            hist = self._pick(t, int(self.rng.integers(3, cfg.history_len + 1)))
            pos = self._pick(t, 1, p_in=1.0)
            neg = [int(x) for x in self.rng.integers(1, self.n_news + 1, size=cfg.sample_size)]
            imps = pos + neg
            samples.append([hist, self._cat(hist), self._sub(hist), imps, self._cat(imps), self._sub(imps)])
        return samples

    def _cat(self, news_ids):
        return [int(self.category[i - 1]) for i in news_ids]

    def _sub(self, news_ids):
        return [int(self.subcategory[i - 1]) for i in news_ids]

    def eval_samples(self, n_imps, max_shown=40):
        """Impressions with 0/1 labels (>=1 of each), shown list shorter than max_candidate_size."""
        cfg = self.config
        samples, labels = [], []
        for _ in range(n_imps):
            t = int(self.rng.integers(0, self.n_topics))
            hist = self._pick(t, int(self.rng.integers(3, cfg.history_len + 1)))
            n = int(self.rng.integers(4, min(max_shown, cfg.max_candidate_size) + 1))
            npos = int(self.rng.integers(1, max(2, n // 4)))
            shown = self._pick(t, npos, p_in=1.0) + [int(x) for x in self.rng.integers(1, self.n_news + 1, size=n - npos)]
            y = [1] * npos + [0] * (n - npos)
            perm = self.rng.permutation(n)
            imps = [shown[i] for i in perm]
            samples.append([hist, self._cat(hist), self._sub(hist), imps, self._cat(imps), self._sub(imps)])
            labels.append([y[i] for i in perm])
        return samples, labels

    def train_impressions(self, n_imps, max_shown=40):
        """Training data in the impression form of ``eval_samples`` -- (samples, labels), 4 .. max_shown shown news per
        impression, at least one clicked and one not -- for ``ImpressionFeed``, which draws every clicked item's negatives from
        the impression's own non-clicked news.  Drawn from a generator of its own: the streams of ``train_samples`` and
        ``eval_samples`` are what they were, however often this is called."""
        cfg, rng = self.config, self.imp_rng
        samples, labels = [], []
        for _ in range(n_imps):
            t = int(rng.integers(0, self.n_topics))
            hist = self._pick(t, int(rng.integers(3, cfg.history_len + 1)), rng=rng)
            n = int(rng.integers(4, max(int(max_shown), 4) + 1))
            npos = int(rng.integers(1, max(2, n // 4)))
            shown = self._pick(t, npos, p_in=1.0, rng=rng) + [int(x) for x in rng.integers(1, self.n_news + 1, size=n - npos)]
            perm = rng.permutation(n)
            imps = [shown[i] for i in perm]
            samples.append([hist, self._cat(hist), self._sub(hist), imps, self._cat(imps), self._sub(imps)])
            labels.append([1 if i < npos else 0 for i in perm])
        return samples, labels

    def click_log(self, n_users, min_clicks=6, max_clicks=80):
        """A click log without impressions for ``ClickFeed``: ``(user_ptr int64 [n_users + 1], clicks int64)``, user u's clicks in
        time order at ``clicks[user_ptr[u]:user_ptr[u + 1]]``, min_clicks .. max_clicks each; every user has a topic and clicks
        mostly inside it (``_pick``).  Drawn from a generator of its own, as ``train_impressions`` is: no other stream moves."""
        rng = self.click_rng
        lens, clicks = [], []
        for _ in range(n_users):
            t = int(rng.integers(0, self.n_topics))
            n = int(rng.integers(int(min_clicks), int(max_clicks) + 1))
            clicks += self._pick(t, n, rng=rng)
            lens.append(n)
        return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(clicks, dtype=np.int64)

    def seen_log(self, user_ptr, clicks, n_seen=12, seed=0):
        """News a user was SHOWN and did not click, for an existing ``click_log``: ``(seen_ptr int64 [n_users + 1], seen_ids
        int64)``, user u's at ``seen_ids[seen_ptr[u]:seen_ptr[u + 1]]``.  Per user up to n_seen draws around the topic most of the
        user's clicks belong to (``_pick``; a draw that hits a news the user clicked, held-out clicks included, is dropped); a news
        drawn twice was seen twice.  A function of (the corpus, user_ptr, clicks, n_seen, seed) alone: the generator is made anew by
        every call, and neither ``click_log`` nor any other stream moves."""
        user_ptr = np.asarray(user_ptr, dtype=np.int64).reshape(-1)
        clicks = np.asarray(clicks, dtype=np.int64).reshape(-1)
        rng = np.random.default_rng([5000003, int(seed)])
        lens, seen = [], []
        for u in range(user_ptr.size - 1):
            own = clicks[user_ptr[u]:user_ptr[u + 1]]
            t = int(np.bincount(self.topic[own - 1], minlength=self.n_topics).argmax()) if own.size else int(rng.integers(0, self.n_topics))
            clicked = set(own.tolist())
            shown = [n for n in self._pick(t, int(n_seen), rng=rng) if n not in clicked]
            seen += shown
            lens.append(len(shown))
        return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(seen, dtype=np.int64)

    def click_ticks(self, user_ptr, horizon=100000, max_step=200):
        """Ticks for an existing ``click_log``: int64 [len(clicks)] for ``ClickFeed(click_time=...)``.  Every user gets a start tick
        in [0, horizon) and rising increments in [1, max_step] from click to click, so the ticks rise strictly inside a user and
        stay below horizon + max_step * (the longest log).  A function of (the corpus seed, user_ptr, horizon, max_step) alone:
        the generator is made anew by every call, and neither ``click_log`` nor any other stream moves."""
        user_ptr = np.asarray(user_ptr, dtype=np.int64).reshape(-1)
        rng = np.random.default_rng(self.tick_seed)
        lens = np.diff(user_ptr)
        total = int(user_ptr[-1])
        start = rng.integers(0, int(horizon), size=lens.size)
        step = rng.integers(1, int(max_step) + 1, size=total)
        first = user_ptr[:-1][lens > 0]
        step[first] = 0
        run = np.cumsum(step)
        ticks = run - np.repeat(run[first], lens[lens > 0]) + np.repeat(start[lens > 0], lens[lens > 0])
        assert ticks.size == 0 or ticks.max() < 2 ** 31 - 1
        return ticks.astype(np.int64)


class LazyBatch(Mapping):
    """A read-only batch dict whose values are produced on first access and kept (keys, order and ``len`` are those of the
    eager dict; ``items()`` / ``values()`` materialise everything).  ``extra``: keys beyond the reference's batch layout that a
    consumer asks for by name (``batch["candidate_logq"]``, ``batch.get(...)``, ``in``); iteration and ``len`` do not list them."""

    def __init__(self, makers, extra=None):
        self._makers, self._vals, self._extra = makers, {}, extra or {}

    def __getitem__(self, key):
        if key not in self._vals:
            self._vals[key] = (self._makers[key] if key in self._makers else self._extra[key])()
        return self._vals[key]

    def __iter__(self):
        return iter(self._makers)

    def __len__(self):
        return len(self._makers)


class DeviceFeed:
    """The same batch dicts as ``DataLoader(MyDataset(config, samples, type), batch_size)`` -- same 13 keys, dtypes, padding
    and sample order -- assembled ON THE DEVICE: the news corpus (title and abstract word ids, 31 MB for MIND's 130 k news at
    30 words) lives in HBM once, the samples are packed into padded id arrays once, and a batch is two row gathers.
    ``MyDataset.__getitem__`` builds every sample in Python (55 dictionary lookups each, data_handler.py:185-250): eight
    loader workers deliver a few thousand users per second, the train step consumes a hundred and fifty thousand.

    Iterable like a DataLoader (``len()`` = batches per epoch); ``shuffle`` draws a fresh permutation per epoch from ``seed``.
    """

    def __init__(self, config, samples, type=0, id2title_dict=None, id2abst_dict=None, batch_size=None, device="cuda",
                 shuffle=False, drop_last=False, seed=0):
        self.config, self.data_type = config, type
        if id2title_dict is None:
            if getattr(config, 'mode', 'large') == 'demo':
                id2title_dict, id2abst_dict = get_Demo_Words_Infos(config)
            else:
                id2title_dict, id2abst_dict = get_Words_Infos(config)
        self.device = torch.device(device)
        self.batch_size = int(batch_size or config.batch_size)
        self.shuffle, self.drop_last, self.seed, self.epoch = bool(shuffle), bool(drop_last), int(seed), 0
        H, L, A = config.history_len, config.n_words_title, config.n_words_abst
        S = config.sample_size + 1 if type < 1 else config.max_candidate_size
        self.S = S

        def table(d, width):
            n = (max(d) + 1) if len(d) else 0                       # news index i lives in row i + 1 (0 = padding slot)
            t = np.zeros((n + 1, width), dtype=np.int64)
            for i, words in d.items():
                w = list(words)[:width]
                t[i + 1, :len(w)] = w
            return torch.from_numpy(t).to(self.device)

        self.titles = table(id2title_dict, L)
        self.absts = table(id2abst_dict, A) if id2abst_dict is not None else None
        n = len(samples)
        hist = np.zeros((n, H), dtype=np.int64)
        hcat, hsub = np.zeros((n, H), dtype=np.int64), np.zeros((n, H), dtype=np.int64)
        cand = np.zeros((n, S), dtype=np.int64)
        ccat, csub = np.zeros((n, S), dtype=np.int64), np.zeros((n, S), dtype=np.int64)
        hlen, clen = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for k, data in enumerate(samples):
            h = list(data[0])[:H]
            x = len(h)
            hist[k, :x] = h
            hlen[k] = x
            if x and len(data) > 2 and data[1] is not None:
                hcat[k, :x] = np.asarray(data[1])[:x]
                hsub[k, :x] = np.asarray(data[2])[:x]
            c = list(data[3])[:S]
            y = len(c)
            cand[k, :y] = c
            clen[k] = y
            if y and len(data) > 5 and data[4] is not None:
                ss = min(len(data[4]), S)
                ccat[k, :ss] = np.asarray(data[4])[:ss]
                csub[k, :ss] = np.asarray(data[5])[:ss]
        dev = lambda a: torch.from_numpy(a).to(self.device)
        self.packed = dict(hist=dev(hist), hcat=dev(hcat), hsub=dev(hsub), cand=dev(cand), ccat=dev(ccat), csub=dev(csub),
                           hlen=dev(hlen), clen=dev(clen))
        self.n = n

    def __len__(self):
        return self.n // self.batch_size if self.drop_last else (self.n + self.batch_size - 1) // self.batch_size

    def _news_info_source(self):
        """(news ids, {"categ": ..., "subcateg": ...}): every slot of the samples with the category pair it carries, flat."""
        p = self.packed
        flat = lambda a, b: torch.cat([p[a].reshape(-1), p[b].reshape(-1)])
        return flat("hist", "cand"), {"categ": flat("hcat", "ccat"), "subcateg": flat("hsub", "csub")}

    def news_info(self):
        """Per-news tables for catalogue retrieval, rows aligned with ``titles`` (row r = news id r): ``{"absts": [N, A]
        word ids or None, "categ": int64 [N], "subcateg": int64 [N]}``.  The samples carry a category and sub-category per
        history / candidate slot; they are scattered to their news ids on the device once, on the first call.  0 means
        unknown: row 0, ids no sample shows and slots without categories stay 0.  In the reference the category is a function
        of the news id (MIND_2020/data_handler.py:71-77), so two different non-zero values for one id raise ValueError."""
        if getattr(self, "_news_info", None) is None:
            N = self.titles.shape[0]
            ids, values = self._news_info_source()
            live = (ids > 0) & (ids < N)
            ids = ids[live]
            tables = {}
            for name in ("categ", "subcateg"):
                v = values[name][live]
                known = v != 0
                big = torch.iinfo(torch.int64).max
                hi = torch.full((N,), -big, dtype=torch.int64, device=self.device).scatter_reduce_(0, ids[known], v[known], "amax")
                lo = torch.full((N,), big, dtype=torch.int64, device=self.device).scatter_reduce_(0, ids[known], v[known], "amin")
                seen = lo != big
                clash = torch.nonzero(seen & (lo != hi))
                if clash.numel():
                    r = int(clash[0, 0])
                    raise ValueError("news_info: news id %d has %s %d and %d in different samples" % (r, name, int(lo[r]), int(hi[r])))
                tables[name] = torch.where(seen, hi, torch.zeros_like(hi))
            self._news_info = {"absts": self.absts, "categ": tables["categ"], "subcateg": tables["subcateg"]}
        return self._news_info

    def click_graph(self):
        """The click graph of this feed's own samples (click_graph.ClickGraph, on the feed's device) for
        ``model.graph_hip.Model.attach_click_graph``: one user node per DISTINCT history row (a training feed repeats a user's
        history once per positive impression), news ids = rows of ``titles``.  Built on the first call, then kept."""
        if getattr(self, "_click_graph", None) is None:
            from .click_graph import ClickGraph
            self._click_graph = ClickGraph.from_histories(torch.unique(self.packed["hist"], dim=0), int(self.titles.shape[0]), self.device)
        return self._click_graph

    def batch(self, rows):
        """rows: int64 device tensor of sample indices -> the batch dict (device tensors).  The dict is LAZY: a value is
        gathered when it is first read (nrms_v0 reads 3 of the 13 keys, nrms_naml 9; gathering all of them cost 0.6 ms of GPU
        time per 512-user batch against a 3.3 ms train step)."""
        p, cfg = self.packed, self.config
        H, S, A = cfg.history_len, self.S, cfg.n_words_abst
        B = rows.shape[0]
        memo = {}

        def sel(name):                                                # rows of one packed array, gathered once
            if name not in memo:
                memo[name] = self._rows_of(name, rows)
            return memo[name]

        def text(table, slots, width):
            if table is None:
                return torch.zeros(B, sel(slots).shape[1], width, dtype=torch.int64, device=self.device)
            return table.index_select(0, sel(slots).reshape(-1)).view(B, sel(slots).shape[1], -1)

        def mask(n_slots, lens):
            return (torch.arange(n_slots, device=self.device)[None, :] < sel(lens)[:, None]).to(torch.uint8)

        return LazyBatch({'browsed_lens': lambda: sel("hlen"),
                          'browsed_ids': lambda: sel("hist"),
                          'browsed_titles': lambda: text(self.titles, "hist", cfg.n_words_title),
                          'browsed_absts': lambda: text(self.absts, "hist", A),
                          'browsed_categ_ids': lambda: sel("hcat"),
                          'browsed_subcateg_ids': lambda: sel("hsub"),
                          'browsed_mask': lambda: mask(H, "hlen"),
                          'candidate_ids': lambda: sel("cand"),
                          'candidate_titles': lambda: text(self.titles, "cand", cfg.n_words_title),
                          'candidate_absts': lambda: text(self.absts, "cand", A),
                          'candidate_categ_ids': lambda: sel("ccat"),
                          'candidate_subcateg_ids': lambda: sel("csub"),
                          'candidate_mask': lambda: mask(S, "clen")})

    def _rows_of(self, name, rows):
        return self.packed[name].index_select(0, rows)

    def __iter__(self):
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            order = torch.randperm(self.n, generator=g).to(self.device)
            self.epoch += 1
        else:
            order = torch.arange(self.n, device=self.device)
        for b in range(len(self)):
            yield self.batch(order[b * self.batch_size:(b + 1) * self.batch_size])


IMPRESSION_MAX_SHOWN = 2048                      # nrms_negative_sample: max_shown <= 2048 (include/nrms_hip.h)
EPOCH_SEED_STEP = 0x9E3779B97F4A7C15


class ImpressionFeed(DeviceFeed):
    """A training ``DeviceFeed`` over IMPRESSIONS (shown news + 0/1 labels) whose negatives are redrawn at the start of every
    epoch, on the device.  The reference shuffles an impression's non-clicked news once, offline, and gives the i-th clicked
    item the slice [i * sample_size, (i + 1) * sample_size) of that shuffle (data_processor.py:519-528); every epoch then shows a
    user the same few negatives.  Here the impression log stays in HBM as a CSR and ``nrms_negative_sample`` (include/nrms_hip.h)
    makes the same slices of a fresh shuffle per epoch: one call, keyed by

        epoch_seed = (seed + epoch * 0x9E3779B97F4A7C15) mod 2^64,

    refills the candidate side (``candidate_ids``, ``candidate_mask`` and, from the per-news tables of ``news_info()``, the
    candidate categories).  One row per clicked item, the impression's history repeated for each, as in the reference's training
    set; a clicked item whose slice is empty keeps its row with the candidates masked out.  The draw is a function of the log, the
    seed and the epoch only: not of the batch size, the shuffle or the rank.  There is no CPU path for the draw.

    samples / labels: the ``[hist, hcat, hsub, imps, icat, isub]`` + 0/1 lists form of ``SyntheticMind.eval_samples``;
    ``from_arrays`` takes the same as arrays.  ``min_history``: impressions whose history is shorter are left out (default 0:
    keep all; the reference's training set uses 5, MIND_2020/data_handler.py:92).  ``resample=False`` keeps epoch 0's draw.
    ``rank`` / ``world``: every rank of a data-parallel job builds the SAME feed from all impressions with the same seed and
    iterates over its own contiguous share of the rows (n_samples // world each)."""

    def __init__(self, config, samples, labels, id2title_dict=None, id2abst_dict=None, batch_size=None, device="cuda", shuffle=False,
                 drop_last=False, seed=0, resample=True, min_history=0, rank=0, world=1):
        if len(samples) != len(labels):
            raise ValueError("ImpressionFeed: %d impressions but %d label lists" % (len(samples), len(labels)))
        H, n = config.history_len, len(samples)
        hist, hcat, hsub = (np.zeros((n, H), dtype=np.int64) for _ in range(3))
        hlen = np.zeros(n, dtype=np.int64)
        shown, label, scat, ssub = [], [], [], []
        with_cat = n > 0 and all(len(d) > 5 and d[1] is not None and d[4] is not None for d in samples)
        for k, (data, y) in enumerate(zip(samples, labels)):
            h = list(data[0])[:H]
            x = len(h)
            hist[k, :x], hlen[k] = h, x
            if x and with_cat:
                hcat[k, :x] = np.asarray(data[1])[:x]
                hsub[k, :x] = np.asarray(data[2])[:x]
            if len(data[3]) != len(y):
                raise ValueError("ImpressionFeed: impression %d shows %d news but has %d labels" % (k, len(data[3]), len(y)))
            shown.append(np.asarray(data[3], dtype=np.int64).reshape(-1))
            label.append(np.asarray(y, dtype=np.int64).reshape(-1))
            if with_cat:
                if len(data[4]) != len(y) or len(data[5]) != len(y):
                    raise ValueError("ImpressionFeed: impression %d: one category pair per shown news expected" % k)
                scat.append(np.asarray(data[4], dtype=np.int64).reshape(-1))
                ssub.append(np.asarray(data[5], dtype=np.int64).reshape(-1))
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        imp_ptr = np.concatenate([[0], np.cumsum([len(s) for s in shown])]).astype(np.int64)
        self._setup(config, hist, hlen, hcat if with_cat else None, hsub if with_cat else None, imp_ptr, cat(shown), cat(label),
                    cat(scat) if with_cat else None, cat(ssub) if with_cat else None, id2title_dict, id2abst_dict, batch_size, device,
                    shuffle, drop_last, seed, resample, min_history, rank, world)

    @classmethod
    def from_arrays(cls, config, hist, imp_ptr, shown, label, hist_categ=None, hist_subcateg=None, shown_categ=None,
                    shown_subcateg=None, hist_len=None, id2title_dict=None, id2abst_dict=None, batch_size=None, device="cuda",
                    shuffle=False, drop_last=False, seed=0, resample=True, min_history=0, rank=0, world=1):
        """hist [n_imp, history_len] news ids, left-aligned, 0 = padding (hist_len [n_imp]: the lengths, default the non-zero
        count); imp_ptr [n_imp + 1], shown [nnz], label [nnz] (0 / 1): the impressions as a CSR; the four category arrays are
        shaped like hist and shown and are given together or not at all."""
        cats = (hist_categ, hist_subcateg, shown_categ, shown_subcateg)
        if any(c is None for c in cats) and not all(c is None for c in cats):
            raise ValueError("ImpressionFeed.from_arrays: give all four category arrays or none")
        hist = np.asarray(hist, dtype=np.int64)
        if hist.ndim != 2 or hist.shape[1] != config.history_len:
            raise ValueError("ImpressionFeed.from_arrays: hist must be [n_imp, history_len = %d], got %s" % (config.history_len, hist.shape))
        hlen = (hist != 0).sum(axis=1) if hist_len is None else np.asarray(hist_len, dtype=np.int64)
        self = cls.__new__(cls)
        i64 = lambda a: None if a is None else np.asarray(a, dtype=np.int64)
        self._setup(config, hist, hlen.astype(np.int64), i64(hist_categ), i64(hist_subcateg), i64(imp_ptr), i64(shown), i64(label),
                    i64(shown_categ), i64(shown_subcateg), id2title_dict, id2abst_dict, batch_size, device, shuffle, drop_last, seed,
                    resample, min_history, rank, world)
        return self

    def _setup(self, config, hist, hlen, hcat, hsub, imp_ptr, shown, label, scat, ssub, id2title_dict, id2abst_dict, batch_size, device,
               shuffle, drop_last, seed, resample, min_history, rank, world):
        n_imp = hist.shape[0]
        if imp_ptr.shape != (n_imp + 1,) or imp_ptr[0] != 0 or (np.diff(imp_ptr) < 0).any() or shown.shape != (int(imp_ptr[-1]),) \
                or label.shape != shown.shape or hlen.shape != (n_imp,):
            raise ValueError("ImpressionFeed: imp_ptr must rise from 0 over n_imp = %d impressions to len(shown) = len(label)" % n_imp)
        if ((label != 0) & (label != 1)).any():
            raise ValueError("ImpressionFeed: labels must be 0 or 1")
        if shown.size and (shown.min() < 0 or shown.max() >= 2 ** 31):
            raise ValueError("ImpressionFeed: shown news ids must be in [0, 2^31)")
        for name, a, like in (("hist_categ", hcat, hist), ("hist_subcateg", hsub, hist), ("shown_categ", scat, shown), ("shown_subcateg", ssub, shown)):
            if a is not None and a.shape != like.shape:
                raise ValueError("ImpressionFeed: %s has shape %s, expected %s" % (name, a.shape, like.shape))
        lens = np.diff(imp_ptr)
        if n_imp and lens.max() > IMPRESSION_MAX_SHOWN:
            k = int(lens.argmax())
            raise ValueError("ImpressionFeed: impression %d shows %d news; negatives are sampled from at most %d shown news per "
                             "impression (nrms_negative_sample, max_shown): split or truncate it" % (k, int(lens[k]), IMPRESSION_MAX_SHOWN))
        if not 0 <= int(rank) < int(world):
            raise ValueError("ImpressionFeed: rank = %r of world = %r" % (rank, world))
        keep = hlen >= int(min_history)
        if not keep.all():                                                   # the CSR of the impressions that stay
            entry = np.repeat(keep, lens)
            hist, hlen, lens = hist[keep], hlen[keep], lens[keep]
            hcat, hsub = (None if a is None else a[keep] for a in (hcat, hsub))
            shown, label = shown[entry], label[entry]
            scat, ssub = (None if a is None else a[entry] for a in (scat, ssub))
            imp_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            n_imp = hist.shape[0]
        DeviceFeed.__init__(self, config, [], type=0, id2title_dict=id2title_dict, id2abst_dict=id2abst_dict, batch_size=batch_size,
                            device=device, shuffle=shuffle, drop_last=drop_last, seed=seed)
        self.resample, self.min_history, self.rank, self.world = bool(resample), int(min_history), int(rank), int(world)
        imp_of = np.repeat(np.arange(n_imp, dtype=np.int64), lens)
        n_pos = np.bincount(imp_of[label != 0], minlength=n_imp).astype(np.int64)
        sample_ptr = np.concatenate([[0], np.cumsum(n_pos)]).astype(np.int64)
        row_imp = np.repeat(np.arange(n_imp, dtype=np.int64), n_pos)          # the impression of every training row
        n, S = int(sample_ptr[-1]), self.S
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        zeros = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=self.device)
        rep = lambda a: dev(a[row_imp]) if a is not None else zeros(n, hist.shape[1])
        self.packed = dict(hist=dev(hist[row_imp]), hcat=rep(hcat), hsub=rep(hsub), cand=zeros(n, S), ccat=zeros(n, S), csub=zeros(n, S),
                           hlen=dev(np.minimum(hlen, hist.shape[1])[row_imp]), clen=zeros(n))
        self.n_imp, self.nnz, self.n_samples = n_imp, int(imp_ptr[-1]), n
        self.imp_ptr, self.sample_ptr = dev(imp_ptr), dev(sample_ptr)
        self.shown, self.label = dev(shown.astype(np.int32)), dev(label.astype(np.uint8))
        self._shown_cat = None if scat is None else (dev(hist), dev(hcat), dev(hsub), dev(scat), dev(ssub))
        per_rank = n // self.world
        self.row0, self.n = (self.rank * per_rank, per_rank) if self.world > 1 else (0, n)
        self.draws, self.drawn_seed = 0, None
        self._n_bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ws = None

    def _news_info_source(self):
        # every shown news, sampled or not, and every history slot once per impression
        if self._shown_cat is None:
            ids = torch.cat([self.packed["hist"].reshape(-1), self.shown.to(torch.int64)])
            return ids, {"categ": torch.zeros_like(ids), "subcateg": torch.zeros_like(ids)}
        hist, hcat, hsub, scat, ssub = self._shown_cat
        flat = lambda a, b: torch.cat([a.reshape(-1), b])
        return flat(hist, self.shown.to(torch.int64)), {"categ": flat(hcat, scat), "subcateg": flat(hsub, ssub)}

    def epoch_seed(self, epoch):
        return (self.seed + int(epoch) * EPOCH_SEED_STEP) & 0xFFFFFFFFFFFFFFFF

    def draw(self, seed):
        """Refill the candidate side with the draw of ``seed`` (one ``nrms_negative_sample`` call and two table look-ups on the
        feed's stream); raises if the library counted an impression it could not sample."""
        import ctypes as C
        from . import _lib
        if self.device.type != "cuda":
            raise _lib.NrmsError("ImpressionFeed: the feed is on %s; negatives are sampled on a GPU (there is no CPU path)" % self.device)
        lib = _lib.load()
        S = self.S - 1
        need = int(lib.nrms_negative_sample_workspace_bytes(C.c_int64(self.n_imp), C.c_int64(self.nnz), S))
        if need == 0:
            _lib.check(-1, "nrms_negative_sample_workspace_bytes")
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=self.device)
        p = self.packed
        self._n_bad.zero_()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = lib.nrms_negative_sample(C.c_int64(self.n_imp), _lib.ptr(self.imp_ptr), _lib.ptr(self.shown), _lib.ptr(self.label),
                                          _lib.ptr(self.sample_ptr), S, IMPRESSION_MAX_SHOWN, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                          _lib.ptr(p["cand"]), _lib.ptr(p["clen"]), _lib.ptr(self._n_bad), _lib.ptr(self._ws),
                                          C.c_size_t(self._ws.numel() * 4), stream)
        _lib.check(rc, "nrms_negative_sample")
        if self._shown_cat is not None:
            info = self.news_info()
            flat = p["cand"].reshape(-1)
            torch.index_select(info["categ"], 0, flat, out=p["ccat"].view(-1))
            torch.index_select(info["subcateg"], 0, flat, out=p["csub"].view(-1))
        bad = int(self._n_bad.item())                                         # the epoch's one host synchronisation
        if bad:
            raise _lib.NrmsError("ImpressionFeed: nrms_negative_sample could not sample %d impression(s) (longer than %d shown news, "
                                 "or a damaged log)" % (bad, IMPRESSION_MAX_SHOWN))
        self.drawn_seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def __iter__(self):
        if self.resample or self.drawn_seed is None:
            self.draw(self.epoch_seed(self.draws))
        self.draws += 1
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch + 1000003 * self.rank)
            order = torch.randperm(self.n, generator=g).to(self.device) + self.row0
            self.epoch += 1
        else:
            order = torch.arange(self.row0, self.row0 + self.n, device=self.device)
        for b in range(len(self)):
            yield self.batch(order[b * self.batch_size:(b + 1) * self.batch_size])


CLICK_WEIGHT_ONE = 65536                         # ClickFeed: w(n) = floor(count(n) ** popularity_power * 65536)


class ClickFeed(DeviceFeed):
    """A training ``DeviceFeed`` over a CLICK LOG -- who clicked what, in what order, and no impressions -- whose negatives are
    drawn from the whole catalogue at the start of every epoch, on the device (``nrms_catalogue_negative_sample``,
    include/nrms_hip.h "Click log").  ``clicks[user_ptr[u]:user_ptr[u + 1]]`` are user u's clicks in time order, ids in (0, N),
    N = the rows of the title table.  A user's last ``holdout`` clicks are held out (``heldout_samples()``); the rest is the
    user's training part, and a user with fewer than ``min_history + 1`` training clicks gives no rows, no held-out targets and
    counts for nothing.  Every training position t >= min_history is one row: positive ``clicks[t]``, history the up to
    ``config.history_len`` clicks before t (oldest first, left-aligned), key = the click's position in the log
    ``user_ptr[u] + t`` -- so a click's draw does not depend on which other rows exist.  Histories are not stored per row: a
    batch gathers them from the resident log by index arithmetic (16 bytes per row instead of 8 * history_len).

    Negatives: S = config.sample_size per row by weight w(n) = floor(count(n) ** popularity_power * 65536), count(n) = the
    training users who clicked n (power 0: w = 1 for every n >= 1, a uniform draw; ``weights`` int64 [N] overrides both), never a
    news of the user's own training part (the held-out clicks are NOT rejected: that would leak them), never twice in a row.
    A slot whose eight attempts all fail stays empty (masked out) and is counted in ``n_short``.

    ``epoch_seed``, ``draw``, ``resample``, ``rank`` / ``world`` and ``news_info()`` as in ``ImpressionFeed``: the draw is a
    function of the log, the seed and the epoch only; one host synchronisation per epoch reads the two counters.  There is no
    CPU path for the draw.  ``news_categ`` / ``news_subcateg``: int64 [N] per-news tables for the category keys (zeros without).

    Beside DeviceFeed's 13 keys a batch answers to the lazy key ``candidate_logq`` float32 [B, S + 1] (by name: iterating the batch
    still lists the 13): log q of every candidate slot's news, for the logQ correction of the pooled loss (config.train_loss = "pooled").  q(n) is the probability that a slot of a
    batch's candidate pool holds n when positives and negatives are pooled together,
        q(n) = (pos_rows(n) / n_rows + S w(n) / W) / (1 + S),
    pos_rows(n) = the training rows whose positive is n, w / W = the sampler's weights and their sum, S = config.sample_size.  The
    table ``logq`` [N] is built once, in float64, and kept as float32; a news with q = 0 (nobody's positive and weight 0) holds
    -inf and cannot occur in a pool.  The rejection of a user's own clicks by the sampler is ignored in q: it renormalises a row's
    draw over the catalogue minus a few dozen news, a relative change of about (the weight share of those news), far below what
    the correction is for.

    ``click_time``: int64 [len(clicks)] ticks (any unit), non-decreasing inside every user, in [0, 2^31 - 1), or None.  With it
    ``news_first_seen()`` gives the per-news timestamp and ``heldout_times()`` the request tick of every held-out sample, for
    ranking inside a time window of the catalogue (``evaluate_retrieval(item_time=..., request_time=..., window_span=...)``);
    nothing else reads it, and without it everything is as it was.

    ``negatives="adaptive"`` (default ``"popularity"``, everything above) draws a row's S negatives from the MODEL's own softmax
    over the catalogue instead, softmax(score / ``temperature``) without replacement (``Model.sample_negatives``,
    ``nrms_softmax_sample_dot``), with the weights of the model named by ``attach_scorer(model)`` as they are when the epoch
    starts: the catalogue is encoded once per draw (dropout-free, in the evaluation precision), then this rank's rows go
    through the user encoder and the sampler in chunks of ``draw_chunk`` rows.  ``packed`` has the layout of the popularity draw.
      * A row's negatives are a function of (the model's weights, the log, seed, epoch, the row's key) only: not of the batch
        size, the chunk size, the order of the rows or the rank.
      * A negative is never a news of the user's own training part (which contains the positive) and never repeated in a row.
      * Held-out clicks are not rejected, for the same reason as above.
      * The negatives are as stale as one epoch, on purpose: the weights move during the epoch and the draw does not follow
        (the staleness rule of the graph model's neighbour vectors).
    A slot is left empty (masked out, counted in ``n_short``) only when fewer than S news are eligible.  ``candidate_logq`` is
    the log-probability of the popularity sampler and an adaptive draw has no fixed q: with ``negatives="adaptive"`` the key
    raises ``KeyError``.  Still one host synchronisation per epoch."""

    def __init__(self, config, user_ptr, clicks, id2title_dict=None, id2abst_dict=None, news_categ=None, news_subcateg=None, holdout=1,
                 min_history=1, popularity_power=0.75, weights=None, batch_size=None, device="cuda", shuffle=False, drop_last=False, seed=0,
                 resample=True, rank=0, world=1, negatives="popularity", temperature=1.0, click_time=None, seen=None):
        user_ptr, clicks = np.asarray(user_ptr, dtype=np.int64).reshape(-1), np.asarray(clicks, dtype=np.int64).reshape(-1)
        self._seen, self._seen_slots = self._checked_seen(seen, user_ptr), None
        self.click_time = self._checked_click_time(click_time, user_ptr, clicks)
        if negatives not in ("popularity", "adaptive"):
            raise ValueError("ClickFeed: negatives = %r must be 'popularity' or 'adaptive'" % (negatives,))
        if not (float(temperature) > 0.0 and np.isfinite(float(temperature))):
            raise ValueError("ClickFeed: temperature = %r must be finite and > 0" % (temperature,))
        self.negatives, self.temperature, self.draw_chunk, self._scorer = negatives, float(temperature), 8192, None
        if user_ptr.size < 1 or user_ptr[0] != 0 or (np.diff(user_ptr) < 0).any() or int(user_ptr[-1]) != clicks.size:
            raise ValueError("ClickFeed: user_ptr must rise from 0 to len(clicks) = %d" % clicks.size)
        if int(holdout) < 0 or int(min_history) < 0:
            raise ValueError("ClickFeed: holdout = %r and min_history = %r must be >= 0" % (holdout, min_history))
        if not 0 <= int(rank) < int(world):
            raise ValueError("ClickFeed: rank = %r of world = %r" % (rank, world))
        if not float(popularity_power) >= 0.0:
            raise ValueError("ClickFeed: popularity_power = %r must be >= 0" % (popularity_power,))
        if clicks.size >= 2 ** 48:
            raise ValueError("ClickFeed: a row's key is its log position, below 2^48")
        DeviceFeed.__init__(self, config, [], type=0, id2title_dict=id2title_dict, id2abst_dict=id2abst_dict, batch_size=batch_size,
                            device=device, shuffle=shuffle, drop_last=drop_last, seed=seed)
        N, H, S = int(self.titles.shape[0]), int(config.history_len), self.S
        if clicks.size and (clicks.min() <= 0 or clicks.max() >= N):
            raise ValueError("ClickFeed: clicked news ids must be in (0, N = %d)" % N)
        if not 2 <= N < 2 ** 31:
            raise ValueError("ClickFeed: the catalogue must have 2 <= N < 2^31 rows, got %d" % N)
        for name, a in (("news_categ", news_categ), ("news_subcateg", news_subcateg), ("weights", weights)):
            if a is not None and tuple(np.shape(a)) != (N,):
                raise ValueError("ClickFeed: %s must be [N = %d], got %s" % (name, N, np.shape(a)))
        if (news_categ is None) != (news_subcateg is None):
            raise ValueError("ClickFeed: give news_categ and news_subcateg together or not at all")
        self.holdout, self.min_history, self.popularity_power = int(holdout), int(min_history), float(popularity_power)
        self.resample, self.rank, self.world = bool(resample), int(rank), int(world)
        n_users = user_ptr.size - 1
        train_len = np.maximum(np.diff(user_ptr) - self.holdout, 0)
        live = train_len >= self.min_history + 1                               # the users that train
        self.n_users, self.n_news, self.live_users = n_users, N, live
        # rows: positions min_history .. train_len - 1 of every live user
        per_user = np.where(live, train_len - self.min_history, 0)
        row_user = np.repeat(np.arange(n_users, dtype=np.int64), per_user)
        first = np.concatenate([[0], np.cumsum(per_user)])[:-1]
        t = np.arange(int(per_user.sum()), dtype=np.int64) - np.repeat(first, per_user) + self.min_history
        row_key = user_ptr[row_user] + t
        # rejection sets and popularity: the distinct (user, news) pairs of the live users' training parts
        in_train = np.arange(clicks.size, dtype=np.int64) - np.repeat(user_ptr[:-1], np.diff(user_ptr)) < np.repeat(np.where(live, train_len, 0), np.diff(user_ptr))
        user_of = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(user_ptr))
        pairs = np.unique(user_of[in_train] * N + clicks[in_train])
        set_user, set_news = pairs // N, pairs % N
        set_ptr = np.concatenate([[0], np.cumsum(np.bincount(set_user, minlength=n_users))]).astype(np.int64)
        count = np.bincount(set_news, minlength=N).astype(np.int64)
        if weights is not None:
            w = np.asarray(weights, dtype=np.int64).copy()
            if (w < 0).any() or w[0] != 0:
                raise ValueError("ClickFeed: weights must be >= 0 and weights[0] (the padding slot) 0")
        elif self.popularity_power == 0.0:
            w = np.ones(N, dtype=np.int64)
        else:
            w = np.floor(count.astype(np.float64) ** self.popularity_power * CLICK_WEIGHT_ONE).astype(np.int64)
        w[0] = 0
        if float(w.astype(np.float64).sum()) > 2.0 ** 62 or int(w.sum()) < 1:
            raise ValueError("ClickFeed: the weights must sum to a value in [1, 2^62]")
        cum = np.concatenate([[0], np.cumsum(w)]).astype(np.int64)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.logq = dev(self.pool_logq(np.bincount(clicks[row_key], minlength=N), w, S - 1))
        zeros = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=self.device)
        n = int(row_key.size)
        self.user_ptr, self.clicks = dev(user_ptr), dev(clicks)
        self.row_key, self.row_user = dev(row_key), dev(row_user.astype(np.int32))
        self.row_pos = dev(clicks[row_key].astype(np.int32))
        self.row_hlen = dev(np.minimum(t, H))
        self.set_ptr, self.set_news, self.count, self.weights, self.cum = dev(set_ptr), dev(set_news.astype(np.int32)), dev(count), dev(w), dev(cum)
        # (the library refuses null pointers: a log in which nobody trains still hands it one element)
        self._set_news_arg = self.set_news if self.set_news.numel() else torch.zeros(1, dtype=torch.int32, device=self.device)
        self._train_len = train_len
        self._row_set_len = np.diff(set_ptr)[row_user]             # host copy: the adaptive draw sizes its exclude matrices with it
        self._categ = None if news_categ is None else (dev(np.asarray(news_categ, dtype=np.int64)), dev(np.asarray(news_subcateg, dtype=np.int64)))
        self.packed = dict(cand=zeros(n, S), ccat=zeros(n, S), csub=zeros(n, S), clen=zeros(n))
        self.n_samples = n
        per_rank = n // self.world
        self.row0, self.n = (self.rank * per_rank, per_rank) if self.world > 1 else (0, n)
        self.draws, self.drawn_seed, self.n_short = 0, None, None
        self._counters = torch.zeros(2, dtype=torch.int32, device=self.device)     # n_short, n_bad
        self._ws = None

    @staticmethod
    def _checked_seen(seen, user_ptr):
        """None, or the seen log (seen_ptr int64 [n_users + 1], seen_ids int64) as host arrays."""
        if seen is None:
            return None
        if not isinstance(seen, (tuple, list)) or len(seen) != 2:
            raise ValueError("ClickFeed: seen must be a pair (seen_ptr [n_users + 1], seen_ids) (got %s)" % type(seen).__name__)
        ptr, ids = np.asarray(seen[0], dtype=np.int64).reshape(-1), np.asarray(seen[1], dtype=np.int64).reshape(-1)
        if ptr.size != user_ptr.size or ptr.size < 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or int(ptr[-1]) != ids.size:
            raise ValueError("ClickFeed: seen_ptr must have one entry per user and one more (%d) and rise from 0 to len(seen_ids) = %d"
                             % (user_ptr.size, ids.size))
        if ids.size and ids.min() < 0:
            raise ValueError("ClickFeed: seen news ids must be >= 0")
        return ptr, ids

    def seen_adjustment(self, beta, max_slots=32, users=None):
        """``data_handler.seen_adjustment`` of the feed's seen log (``seen=`` of the constructor; ValueError without one), on the
        feed's device -> (ids int64 [n, max_slots], delta float32 [n, max_slots]): the ``adjust`` of ``Model.recommend_adjusted`` /
        ``train_eval.recommend(adjust=...)``.  users: the user of every row wanted, e.g. ``heldout_users()`` for the samples of
        ``heldout_samples()``, or a batch's users; None: one row per user of the log.  The whole log's slots are built once per
        (beta, max_slots) and kept on the device, so a call per batch costs one gather."""
        if self._seen is None:
            raise ValueError("ClickFeed.seen_adjustment: the feed has no seen log (give seen=(seen_ptr, seen_ids))")
        key = (float(beta), int(max_slots))
        if self._seen_slots is None or self._seen_slots[0] != key:
            self._seen_slots = (key, seen_adjustment(self._seen[0], self._seen[1], beta, max_slots, device=self.device))
        ids, delta = self._seen_slots[1]
        if users is None:
            return ids, delta
        u = torch.as_tensor(users).to(self.device, dtype=torch.int64).reshape(-1)
        return ids[u].contiguous(), delta[u].contiguous()

    @staticmethod
    def _checked_click_time(click_time, user_ptr, clicks):
        """None, or the log's ticks as an int64 host array: one per click, non-decreasing inside every user, in [0, 2^31 - 1)."""
        if click_time is None:
            return None
        t = np.asarray(click_time)
        if t.dtype.kind not in "iu" or t.shape != (clicks.size,):
            raise ValueError("ClickFeed: click_time must be an integer array of len(clicks) = %d ticks, got %s %s"
                             % (clicks.size, t.dtype, t.shape))
        t = t.astype(np.int64)
        if t.size and (t.min() < 0 or t.max() >= 2 ** 31 - 1):
            raise ValueError("ClickFeed: click_time must lie in [0, 2^31 - 1) (2^31 - 1 is the 'not published' value), got [%d, %d]"
                             % (t.min(), t.max()))
        if t.size > 1 and user_ptr.size >= 1 and user_ptr[0] == 0 and int(user_ptr[-1]) == t.size:
            falls = np.diff(t) < 0
            starts = user_ptr[1:-1][(user_ptr[1:-1] > 0) & (user_ptr[1:-1] < t.size)]
            falls[starts - 1] = False                        # a new user may start earlier than the last one ended
            if falls.any():
                raise ValueError("ClickFeed: click_time must not decrease inside a user (it does at log position %d)"
                                 % (int(np.flatnonzero(falls)[0]) + 1))
        return t

    def _need_click_time(self, who):
        if self.click_time is None:
            raise ValueError("ClickFeed.%s: the feed was built without click_time" % who)
        return self.click_time

    def news_first_seen(self):
        """int32 [N] on the feed's device: the earliest tick at which anyone clicked the news, over the WHOLE log, held-out clicks
        included (when a news appeared is catalogue metadata, not a label); a never-clicked news and entry 0, the padding
        title's, hold INT32_MAX, "not published".  The ``item_time`` of ``Model.recommend`` / ``rank_targets``."""
        t = self._need_click_time("news_first_seen")
        first = np.full(self.n_news, 2 ** 31 - 1, dtype=np.int64)
        np.minimum.at(first, self.clicks.cpu().numpy(), t)
        first[0] = 2 ** 31 - 1
        return torch.from_numpy(first.astype(np.int32)).to(self.device)

    def heldout_times(self):
        """int64 host array: the request tick of every sample of ``heldout_samples()``, in the same order: the tick of the user's
        first held-out click."""
        t = self._need_click_time("heldout_times")
        user_ptr = self.user_ptr.cpu().numpy()
        out = []
        for u in np.flatnonzero(self.live_users):
            end = int(user_ptr[u] + self._train_len[u])
            if end < int(user_ptr[u + 1]):
                out.append(int(t[end]))
        return np.asarray(out, dtype=np.int64)

    @staticmethod
    def pool_logq(pos_rows, weights, sample_size):
        """float32 [N] log q (the class docstring's formula), from the rows per positive and the sampler's weights."""
        pos, w = np.asarray(pos_rows, dtype=np.float64), np.asarray(weights, dtype=np.float64)
        n_rows, S = pos.sum(), float(sample_size)
        q = ((pos / n_rows if n_rows > 0 else np.zeros_like(pos)) + S * w / w.sum()) / (1.0 + S)
        with np.errstate(divide="ignore"):
            return np.log(q).astype(np.float32)

    def popularity_prior(self, alpha):
        """float32 [N] on the feed's device: prior[n] = float32(alpha * log1p(count[n])), formed in float64 from the resident
        ``count`` (the number of training users who clicked n; held-out clicks are not counted, so the prior cannot leak them),
        prior[0] = 0.  The per-news prior ``Model.recommend(item_bias=...)`` and ``rank_targets(item_bias=...)`` take: what
        ``--loss pooled``'s logQ correction trains out of the scores, put back at serving time in a tunable amount.  alpha must
        be finite (ValueError); alpha = 0 gives zeros."""
        alpha = float(alpha)
        if not np.isfinite(alpha):
            raise ValueError("ClickFeed.popularity_prior: alpha = %r must be finite" % (alpha,))
        prior = (alpha * np.log1p(self.count.cpu().numpy().astype(np.float64))).astype(np.float32)
        prior[0] = 0.0
        return torch.from_numpy(prior).to(self.device)

    def clicked_tags(self, item_tag, n_tags):
        """bool [n_users, n_tags] on the feed's device: out[u, t] iff user u's TRAINING part holds a click on a news with
        item_tag[id] == t (item_tag: int [N] by news id, e.g. ``news_info()["categ"]``; a tag outside [0, n_tags) sets nothing).
        Built from the resident rejection sets, so a held-out click is never counted (the set cannot leak it) and a user who does
        not train has an all-False row.  The ``allow`` of ``Model.recommend_tagged`` / ``rank_targets_tagged`` for "only the
        topics I follow": index it with ``heldout_users()`` for the samples of ``heldout_samples()``."""
        n_tags = int(n_tags)
        if n_tags < 1:
            raise ValueError("ClickFeed.clicked_tags: n_tags = %r must be >= 1" % (n_tags,))
        tag = torch.as_tensor(item_tag).to(self.device, dtype=torch.int64).reshape(-1)
        if tag.shape[0] != self.n_news:
            raise ValueError("ClickFeed.clicked_tags: item_tag must be [N = %d], got %s" % (self.n_news, tuple(tag.shape)))
        out = torch.zeros(self.n_users, n_tags, dtype=torch.bool, device=self.device)
        if self.set_news.numel():
            user = torch.repeat_interleave(torch.arange(self.n_users, device=self.device), self.set_ptr[1:] - self.set_ptr[:-1])
            t = tag[self.set_news.long()]
            ok = (t >= 0) & (t < n_tags)
            out[user[ok], t[ok]] = True
        return out

    def heldout_users(self):
        """int64 host array: the user of every sample of ``heldout_samples()``, in the same order."""
        user_ptr = self.user_ptr.cpu().numpy()
        return np.asarray([u for u in np.flatnonzero(self.live_users) if int(user_ptr[u] + self._train_len[u]) < int(user_ptr[u + 1])],
                          dtype=np.int64)

    def batch(self, rows):
        b = DeviceFeed.batch(self, rows)
        if self.negatives == "adaptive":
            def no_logq():
                raise KeyError("candidate_logq: an adaptive draw follows the model and has no fixed q (the table is the popularity "
                               "sampler's log-probability); train without the logQ correction")
            b._extra['candidate_logq'] = no_logq
        else:
            b._extra['candidate_logq'] = lambda: self.logq.index_select(0, b['candidate_ids'].reshape(-1)).view(b['candidate_ids'].shape)
        return b

    def _rows_of(self, name, rows):
        if name in self.packed:
            return self.packed[name].index_select(0, rows)
        hlen = self.row_hlen.index_select(0, rows)
        if name == "hlen":
            return hlen
        # the history of a row: the hlen clicks in front of its own, gathered from the log
        H = self.config.history_len
        j = torch.arange(H, device=self.device)[None, :]
        at = (self.row_key.index_select(0, rows) - hlen)[:, None] + j
        ids = torch.where(j < hlen[:, None], self.clicks[at.clamp_(0, max(self.clicks.numel() - 1, 0))], torch.zeros_like(at)) \
            if self.clicks.numel() else torch.zeros_like(at)
        if name == "hist":
            return ids
        if self._categ is None:
            return torch.zeros_like(ids)
        return self._categ[0 if name == "hcat" else 1][ids]

    def news_info(self):
        if getattr(self, "_news_info", None) is None:
            z = torch.zeros(self.n_news, dtype=torch.int64, device=self.device)
            categ, sub = (z, z.clone()) if self._categ is None else self._categ
            self._news_info = {"absts": self.absts, "categ": categ, "subcateg": sub}
        return self._news_info

    def click_graph(self):
        raise NotImplementedError("ClickFeed: no click graph is built from a click log yet (click_graph.ClickGraph.from_histories takes history rows)")

    def epoch_seed(self, epoch):
        return (self.seed + int(epoch) * EPOCH_SEED_STEP) & 0xFFFFFFFFFFFFFFFF

    def attach_scorer(self, model):
        """Names the model whose softmax ``negatives="adaptive"`` draws from (a model with ``CATALOGUE_SAMPLING``, or the
        ``model.Model`` wrapper around one)."""
        net = model.model if hasattr(model, "model") and not hasattr(model, "sample_negatives") else model
        if not getattr(type(net), "CATALOGUE_SAMPLING", False):
            raise ValueError("ClickFeed.attach_scorer: %s cannot sample negatives from its catalogue scores (no CATALOGUE_SAMPLING)"
                             % type(net).__module__)
        self._scorer = net

    def _draw_adaptive(self, seed):
        """The adaptive draw of this rank's rows [row0, row0 + n) into ``packed``; returns the device count of empty slots."""
        import inspect
        net = self._scorer
        if net is None:
            raise RuntimeError("ClickFeed: negatives='adaptive' needs attach_scorer(model) before the first epoch")
        needs_info = 'categ' in inspect.signature(net.encode_catalogue).parameters           # nrms_naml's feature rows
        catalogue = net.encode_catalogue(self.titles, **(self.news_info() if needs_info else {}))
        p, S = self.packed, self.S - 1
        short = torch.zeros((), dtype=torch.int64, device=self.device)
        for c0 in range(self.row0, self.row0 + self.n, self.draw_chunk):
            c1 = min(self.row0 + self.n, c0 + self.draw_chunk)
            rows = torch.arange(c0, c1, device=self.device)
            # the user's training-part clicks (they contain the positive), padded with -1 to the chunk's longest set
            width = max(int(self._row_set_len[c0:c1].max()), 1)
            user = self.row_user[c0:c1].long()
            first, count = self.set_ptr[user], self.set_ptr[user + 1] - self.set_ptr[user]
            j = torch.arange(width, device=self.device)[None, :]
            at = (first[:, None] + j).clamp_(max=max(self.set_news.numel() - 1, 0))
            exclude = torch.where(j < count[:, None], self._set_news_arg[at].long(), torch.full_like(at, -1))
            ids = net.sample_negatives({"browsed_ids": self._rows_of("hist", rows)}, self.row_key[c0:c1], S, catalogue, self.temperature,
                                       seed, exclude=exclude)
            got = ids >= 0                                   # the valued slots come first: the kernel pads at the end
            p["cand"][c0:c1, 0] = self.row_pos[c0:c1].long()
            p["cand"][c0:c1, 1:] = torch.where(got, ids, torch.zeros_like(ids))
            p["clen"][c0:c1] = 1 + got.sum(1)
            short += (~got).sum()
        return short

    def draw(self, seed):
        """Refill the candidate side with the draw of ``seed`` (one ``nrms_catalogue_negative_sample`` call and two table look-ups on
        the feed's stream); raises if the library counted a row it could not sample; ``n_short`` = the slots left empty.
        ``negatives="adaptive"``: the catalogue encode and, per chunk of rows, the user encoder and ``nrms_softmax_sample_dot``."""
        import ctypes as C
        from . import _lib
        if self.device.type != "cuda":
            raise _lib.NrmsError("ClickFeed: the feed is on %s; negatives are sampled on a GPU (there is no CPU path)" % self.device)
        if self.negatives == "adaptive":
            short = self._draw_adaptive(seed)
            if self._categ is not None:
                flat = self.packed["cand"].reshape(-1)
                torch.index_select(self._categ[0], 0, flat, out=self.packed["ccat"].view(-1))
                torch.index_select(self._categ[1], 0, flat, out=self.packed["csub"].view(-1))
            # (the histories are the feed's own checked clicks, so the model's count of ids outside the catalogue stays untouched)
            self.n_short = int(short.item())                                         # the epoch's one host synchronisation
            self.drawn_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            return
        lib = _lib.load()
        S, n = self.S - 1, self.n_samples
        need = int(lib.nrms_catalogue_negative_sample_workspace_bytes(C.c_int64(n), C.c_int64(self.n_news), S))
        if need == 0:
            _lib.check(-1, "nrms_catalogue_negative_sample_workspace_bytes")
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=self.device)
        p = self.packed
        self._counters.zero_()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            sample = lib.nrms_catalogue_negative_sample
            rc = 0 if n == 0 else sample(C.c_int64(n), _lib.ptr(self.row_key), _lib.ptr(self.row_user), _lib.ptr(self.row_pos),
                                         C.c_int64(self.n_users), _lib.ptr(self.set_ptr), _lib.ptr(self._set_news_arg), C.c_int64(self.n_news),
                                         _lib.ptr(self.cum), S, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _lib.ptr(p["cand"]),
                                         _lib.ptr(p["clen"]), _lib.ptr(self._counters[0:]), _lib.ptr(self._counters[1:]),
                                         _lib.ptr(self._ws), C.c_size_t(self._ws.numel() * 4), stream)
        _lib.check(rc, "nrms_catalogue_negative_sample")
        if self._categ is not None:
            flat = p["cand"].reshape(-1)
            torch.index_select(self._categ[0], 0, flat, out=p["ccat"].view(-1))
            torch.index_select(self._categ[1], 0, flat, out=p["csub"].view(-1))
        self.n_short, bad = self._counters.tolist()                              # the epoch's one host synchronisation
        if bad:
            raise _lib.NrmsError("ClickFeed: nrms_catalogue_negative_sample could not sample %d row(s) (a user or a positive outside "
                                 "its range: a damaged log)" % bad)
        self.drawn_seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def __iter__(self):
        if self.resample or self.drawn_seed is None:
            self.draw(self.epoch_seed(self.draws))
        self.draws += 1
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch + 1000003 * self.rank)
            order = torch.randperm(self.n, generator=g).to(self.device) + self.row0
            self.epoch += 1
        else:
            order = torch.arange(self.row0, self.row0 + self.n, device=self.device)
        for b in range(len(self)):
            yield self.batch(order[b * self.batch_size:(b + 1) * self.batch_size])

    def heldout_samples(self):
        """``(samples, labels)`` of the live users' held-out clicks in the ``[hist, hcat, hsub, imps, icat, isub]`` + 0/1 form:
        imps = the user's last ``holdout`` clicks (every label 1), hist = the user's last ``config.history_len`` training clicks --
        ready for ``DeviceFeed(type=1)`` and ``evaluate_retrieval``."""
        user_ptr, clicks = self.user_ptr.cpu().numpy(), self.clicks.cpu().numpy()
        H = self.config.history_len
        categ = None if self._categ is None else tuple(c.cpu().numpy() for c in self._categ)
        look = lambda k, ids: [0] * len(ids) if categ is None else [int(categ[k][i]) for i in ids]
        samples, labels = [], []
        for u in np.flatnonzero(self.live_users):
            end = int(user_ptr[u] + self._train_len[u])
            hist = clicks[max(int(user_ptr[u]), end - H):end].tolist()
            imps = clicks[end:int(user_ptr[u + 1])].tolist()
            if not imps:
                continue
            samples.append([hist, look(0, hist), look(1, hist), imps, look(0, imps), look(1, imps)])
            labels.append([1] * len(imps))
        return samples, labels
