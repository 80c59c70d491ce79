"""Per-epoch negative sampling on the device (csrc/negsample.hip, data_handler.ImpressionFeed, run_v0 --negatives epoch): cand and clen
bit for bit against the numpy restatement tests/negsample_ref.py of the contract in include/nrms_hip.h, the buffers' extents between
guard bands, and the feed and a training run on top."""
import ctypes as C

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.config import Config
from pytorch_news_recommender_amd.data_handler import DeviceFeed, ImpressionFeed, SyntheticMind

from tests import negsample_ref as ref
from tests.guarded import POISONS, Pool, assert_same_bits

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567890
KEYS = ("browsed_lens", "browsed_ids", "browsed_titles", "browsed_absts", "browsed_categ_ids", "browsed_subcateg_ids", "browsed_mask",
        "candidate_ids", "candidate_titles", "candidate_absts", "candidate_categ_ids", "candidate_subcateg_ids", "candidate_mask")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sample(imp_ptr, shown, label, S, seed, max_shown=ref.MAX_SHOWN, pool=None):
    """One nrms_negative_sample call on numpy inputs -> (cand, clen, n_bad).  pool: a tests.guarded.Pool that provides the outputs
    and the workspace between guard bands."""
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n_imp, nnz = len(imp_ptr) - 1, int(imp_ptr[-1])
    sample_ptr = ref.sample_ptr_of(imp_ptr, label)
    n = int(sample_ptr[-1])
    d = [dev(np.asarray(imp_ptr, dtype=np.int64)), dev(np.asarray(shown, dtype=np.int32)), dev(np.asarray(label, dtype=np.uint8)), dev(sample_ptr)]
    need = int(lib.nrms_negative_sample_workspace_bytes(C.c_int64(n_imp), C.c_int64(nnz), S))
    assert need > 0 and need % 4 == 0
    if pool is None:
        cand = torch.full((n, S + 1), -7, dtype=torch.int64, device="cuda")
        clen = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        n_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = torch.empty(need // 4, dtype=torch.int32, device="cuda")
        ptrs = [_lib.ptr(cand), _lib.ptr(clen), _lib.ptr(n_bad), _lib.ptr(ws)]
    else:
        g = [pool.elems("cand", n * (S + 1), torch.int64), pool.elems("clen", n, torch.int64), pool.elems("n_bad", 1, torch.int32, init="zero"),
             pool.new("workspace", need)]
        ptrs = [b.ptr for b in g]
    rc = lib.nrms_negative_sample(C.c_int64(n_imp), *[_lib.ptr(t) for t in d], S, max_shown, C.c_uint64(seed), ptrs[0], ptrs[1], ptrs[2],
                                  ptrs[3], C.c_size_t(need), _stream())
    _lib.check(rc, "nrms_negative_sample")
    if pool is not None:
        pool.intact("nrms_negative_sample")
        return g[0].numpy((n, S + 1)), g[1].numpy(), int(g[2].numpy()[0])
    torch.cuda.synchronize()
    return cand.cpu().numpy(), clen.cpu().numpy(), int(n_bad.item())


def edge_log(S, n_random, seed, with_2048=True):
    """Both paths and their boundary (1, 2, 63, 64 | 65, 128, 300, 2048 shown), and per S: no positive, only positives, one negative
    and three positives, n_neg = k S and k S + 1 under k + 1 positives (the last slice empty, or one long) on either path."""
    rng = np.random.default_rng(seed)
    lens = [1, 1, 2, 63, 64, 65, 128, 300] + ([2048] if with_2048 else [])
    force = {0: [1], 1: [0]}
    def add(y):
        force[len(lens)] = y
        lens.append(len(y))
    add([0] * 10), add([0] * 70)                                                # no positive: no row
    add([1] * 7), add([1] * 66)                                                 # only positives
    add([1, 0, 1, 1]), add([1] + [0] + [1, 1] + [1] * 62)                        # one negative: empty slices
    k = max(2, -(-66 // S))                                                      # k (S + 1) >= 66: the workgroup path
    for extra in (0, 1):
        if 3 + 2 * S + extra <= 64:
            add(rng.permutation([1] * 3 + [0] * (2 * S + extra)).tolist())       # one wave
        add(rng.permutation([1] * (k + 1) + [0] * (k * S + extra)).tolist())
    w = 1.0 / np.arange(1, 301) ** 1.2                                           # short impressions, a tail to 300
    lens += rng.choice(np.arange(1, 301), size=n_random, p=w / w.sum()).tolist()
    return ref.random_log(lens, rng, force=force)


def assert_equal(got, want, what):
    for name, g, w in zip(("cand", "clen", "n_bad"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)
            raise AssertionError("%s: %s differs in %d places, first at %s: got %s, want %s" % (what, name, len(at), at[0], g[tuple(at[0])], w[tuple(at[0])]))


# ---- 1. bit equality --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4, 5, 64])
def test_cand_and_clen_are_bit_equal_to_the_restatement(S):
    imp_ptr, shown, label = edge_log(S, n_random=3000, seed=S)
    want = ref.negative_sample(imp_ptr, shown, label, S, SEED + S)
    assert want[2] == 0 and (want[1] == 1).any() and (want[1] == S + 1).any()
    assert_equal(sample(imp_ptr, shown, label, S, SEED + S), want, "S = %d" % S)


@pytest.mark.parametrize("n,S", [(1, 4), (40, 4), (64, 1), (65, 5), (300, 4), (2048, 64)])
def test_a_single_impression(n, S):
    imp_ptr, shown, label = ref.random_log([n], np.random.default_rng(n), p_pos=0.2, force={0: [1]} if n == 1 else None)
    label[0] = 1
    assert_equal(sample(imp_ptr, shown, label, S, SEED), ref.negative_sample(imp_ptr, shown, label, S, SEED), "n = %d" % n)


@pytest.mark.parametrize("max_shown,long_len", [(2048, 2049), (10, 11), (10, 64), (64, 300)])
def test_an_impression_above_max_shown_keeps_its_positives_only_and_is_counted(max_shown, long_len):
    rng = np.random.default_rng(long_len)
    lens = [5, long_len, max_shown, 9]
    imp_ptr, shown, label = ref.random_log(lens, rng, p_pos=0.1, force={0: [1, 0, 0, 0, 0], 3: [0, 1, 0, 1, 0, 0, 0, 0, 0]})
    label[imp_ptr[1]] = label[imp_ptr[2] - 1] = 1                                # the long one has positives at both ends
    label[imp_ptr[2]:imp_ptr[3]] = 0
    label[imp_ptr[2]] = 1                                                        # the one of exactly max_shown: one positive
    want = ref.negative_sample(imp_ptr, shown, label, 4, SEED, max_shown=max_shown)
    got = sample(imp_ptr, shown, label, 4, SEED, max_shown=max_shown)
    assert_equal(got, want, "max_shown = %d" % max_shown)
    sp = ref.sample_ptr_of(imp_ptr, label)
    rows = slice(sp[1], sp[2])
    a, b = imp_ptr[1], imp_ptr[2]
    assert got[2] == 1 and (got[1][rows] == 1).all() and (got[0][rows, 1:] == 0).all()
    assert got[0][rows, 0].tolist() == shown[a:b][label[a:b] != 0].tolist()
    assert got[1][sp[2]] == 5                                                    # an impression of exactly max_shown is sampled


# ---- 2. extents, determinism, seeds ---------------------------------------------------------------------------------------------------
def test_outputs_and_workspace_between_guard_bands_whatever_they_held():
    imp_ptr, shown, label = edge_log(4, n_random=200, seed=11)
    want = ref.negative_sample(imp_ptr, shown, label, 4, SEED)
    runs = {}
    for poison in POISONS:
        got = sample(imp_ptr, shown, label, 4, SEED, pool=Pool(poison))
        assert_equal(got, want, "poison 0x%02X" % poison)
        runs[poison] = {"cand": got[0], "clen": got[1]}
    assert_same_bits(runs, "nrms_negative_sample")


def test_two_calls_give_the_same_bytes_and_a_seed_changes_the_negatives_only():
    imp_ptr, shown, label = edge_log(4, n_random=1000, seed=12)
    a, b = sample(imp_ptr, shown, label, 4, SEED), sample(imp_ptr, shown, label, 4, SEED)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = sample(imp_ptr, shown, label, 4, SEED + 1)
    assert np.array_equal(a[0][:, 0], c[0][:, 0]) and np.array_equal(a[1], c[1])
    assert (a[0][:, 1:] != c[0][:, 1:]).mean() > 0.5
    assert_equal(c, ref.negative_sample(imp_ptr, shown, label, 4, SEED + 1), "second seed")


# ---- 3. the feed ------------------------------------------------------------------------------------------------------------------------------
def _config():
    cfg = Config("nrms_hip")
    cfg.__nrms__()
    cfg.n_words_title = 30
    return cfg


@pytest.fixture(scope="module")
def world():
    cfg = _config()
    corpus = SyntheticMind(cfg, n_news=500, seed=1)
    imps, labels = corpus.train_impressions(150, max_shown=90)                   # one-wave and workgroup impressions
    h = imps[0][0]
    ids = [3, 4, 5, 6]                                                           # one negative, three positives: empty slices
    imps.append([h, corpus._cat(h), corpus._sub(h), ids, corpus._cat(ids), corpus._sub(ids)])
    labels.append([1, 0, 1, 1])
    imp_ptr = np.concatenate([[0], np.cumsum([len(y) for y in labels])]).astype(np.int64)
    shown = np.concatenate([s[3] for s in imps]).astype(np.int32)
    label = np.concatenate(labels).astype(np.uint8)
    row_imp = np.repeat(np.arange(len(imps)), [sum(y) for y in labels])
    return dict(cfg=cfg, corpus=corpus, imps=imps, labels=labels, csr=(imp_ptr, shown, label), row_imp=row_imp, cache={})


def expected_batches(w, seed, batch_size):
    """The batch dicts of a DeviceFeed over the restatement's rows for `seed` (built once per seed)."""
    if seed not in w["cache"]:
        cfg, corpus = w["cfg"], w["corpus"]
        cand, clen, n_bad = ref.negative_sample(*w["csr"], cfg.sample_size, seed)
        assert n_bad == 0
        samples = []
        for k, row, c in zip(w["row_imp"], cand, clen):
            ids = row[:c].tolist()
            s = w["imps"][k]
            samples.append([s[0], s[1], s[2], ids, corpus._cat(ids), corpus._sub(ids)])
        feed = DeviceFeed(cfg, samples, type=0, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, batch_size=batch_size)
        w["cache"][seed] = ([{k: b[k].clone() for k in KEYS} for b in feed], cand, clen)
    return w["cache"][seed]


def _feed(w, batch_size=64, **kw):
    corpus = w["corpus"]
    return ImpressionFeed(w["cfg"], w["imps"], w["labels"], id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict,
                          batch_size=batch_size, seed=77, **kw)


def _epoch(feed):
    return [{k: b[k].clone() for k in KEYS} for b in feed]


def assert_batches(got, want, what):
    assert len(got) == len(want) > 1
    for i, (g, x) in enumerate(zip(got, want)):
        assert list(g) == list(x) == list(KEYS)
        for k in KEYS:
            assert g[k].dtype == x[k].dtype and torch.equal(g[k], x[k]), "%s: batch %d, %s" % (what, i, k)


def test_feed_epoch_0_yields_the_device_feeds_batches_over_the_restatements_rows(world):
    feed = _feed(world)
    want, cand, clen = expected_batches(world, ref.epoch_seed(77, 0), 64)
    assert (clen == 1).any() and (clen == world["cfg"].sample_size + 1).any()
    assert_batches(_epoch(feed), want, "epoch 0")
    assert feed.drawn_seed == ref.epoch_seed(77, 0) and len(feed) == len(want)


def test_feed_epoch_1_redraws_the_negatives_and_nothing_else(world):
    feed = _feed(world)
    e0, e1 = _epoch(feed), _epoch(feed)
    assert feed.drawn_seed == ref.epoch_seed(77, 1)
    same, differ = 0, 0
    for a, b in zip(e0, e1):
        for k in KEYS:
            if k.startswith("browsed_"):
                assert torch.equal(a[k], b[k]), k
        assert torch.equal(a["candidate_ids"][:, 0], b["candidate_ids"][:, 0]) and torch.equal(a["candidate_mask"], b["candidate_mask"])
        differ += int((a["candidate_ids"][:, 1:] != b["candidate_ids"][:, 1:]).sum())
        same += int((a["candidate_ids"][:, 1:] == b["candidate_ids"][:, 1:]).sum())
    assert differ > same
    assert_batches(e1, expected_batches(world, ref.epoch_seed(77, 1), 64)[0], "epoch 1")
    assert_batches(e0, expected_batches(world, ref.epoch_seed(77, 0), 64)[0], "epoch 0")


def test_feed_without_resampling_repeats_epoch_0_and_a_rank_takes_its_own_rows(world):
    feed = _feed(world, resample=False)
    e0, e1 = _epoch(feed), _epoch(feed)
    assert_batches(e1, e0, "resample=False")
    assert_batches(e0, expected_batches(world, ref.epoch_seed(77, 0), 64)[0], "epoch 0")
    # the draw does not depend on the rank or the batch size: rank 1 of 2 sees rows [n // 2, 2 (n // 2)) of the same draw
    cand = expected_batches(world, ref.epoch_seed(77, 0), 64)[1]
    half = len(cand) // 2
    r1 = _feed(world, batch_size=32, rank=1, world=2, drop_last=True)
    got = torch.cat([b["candidate_ids"] for b in r1]).cpu().numpy()
    assert len(got) == half // 32 * 32 and np.array_equal(got, cand[half:half + len(got)])
    # a shuffled epoch is a permutation of the same rows
    sh = _feed(world, shuffle=True)
    rows = torch.cat([b["candidate_ids"] for b in sh]).cpu().numpy()
    assert not np.array_equal(rows, cand) and sorted(map(tuple, rows)) == sorted(map(tuple, cand))


# ---- 4. training ------------------------------------------------------------------------------------------------------------------------------
def test_run_v0_with_epoch_negatives_is_reproducible_and_learns(tmp_path, monkeypatch):
    """20 batches of 64 rows over 260 synthetic impressions: the second epoch, with its own draw, starts inside them.  Loss:
    finite, and the mean of the last five batches below the mean of the first five (which start at ln 5 = 1.61)."""
    from pytorch_news_recommender_amd import run_v0
    monkeypatch.chdir(tmp_path)
    draws = []
    real = ImpressionFeed.draw
    monkeypatch.setattr(ImpressionFeed, "draw", lambda self, seed: (draws.append(seed), real(self, seed))[1])
    runs = []
    for r in range(2):
        hist = run_v0.main(["--model", "nrms_hip", "--dataset", "synthetic", "--negatives", "epoch", "--epochs", "3", "--synthetic_users", "260",
                            "--batch_size", "64", "--max_batches", "20", "--num_workers", "0", "--description", "T",
                            "--data_path", str(tmp_path / "data_processed"), "--save_path", str(tmp_path / ("save%d" % r))])
        runs.append(hist["losses"])
    print("losses", runs[0])
    assert len(runs[0]) == 20 and np.isfinite(runs[0]).all()
    assert runs[0] == runs[1]
    assert len(draws) % 2 == 0 and len(draws) >= 4 and draws[:len(draws) // 2] == draws[len(draws) // 2:]
    assert draws[0] == ref.epoch_seed(422, 0) and draws[1] == ref.epoch_seed(422, 1)
    assert np.mean(runs[0][-5:]) < np.mean(runs[0][:5])
