"""The lattice data of the request tests (tests/test_hip_topk_request.py on the GPU, tests/test_topk_request_host.py on the CPU, which
asserts on this data alone that no (shape, subset) is left empty).  numpy only.

Integer users and items in [-3, 3], a bias and deltas of multiples of 0.25 (every sum is exact in fp32 whatever the order of
summation; ties are abundant, so the id rule is exercised) with NaN and +-inf sprinkled in.  Times in [0, 30) against windows 20
wide, tags against allow rows two thirds open: each closes roughly a third of the pairs on its own, so about a ninth is closed by
both at once.  User 0 is wide open (the widest window, every tag, finite deltas, no cursor), the last user is closed by every
part the subset holds that can close a row (an empty window, no tag, a cursor at END), the one before it is nearly closed."""
import functools
import itertools

import numpy as np

from tests import topk_request_ref as ref

I64_MAX = 2 ** 63 - 1
PART_NAMES = ("window", "tags", "adjust", "cursor")
# every subset of two, three and four parts (window + cursor is forwarded to nrms_topk_dot_after; the other ten run the REQ kernels)
SUBSETS = [s for n in (2, 3, 4) for s in itertools.combinations(PART_NAMES, n)]
RANK_SUBSETS = [s for s in SUBSETS if "cursor" not in s]

# (B, N, d, k, T, n_tags, E, n_exclude, bias).  Top-k slices are 2048 rows (TK_MIN_SLICE), so N = 2049 is two and N = 4100 three
# with a last step of 4 rows; k <= 64 / <= 192 / above are the three P classes (the last with two waves per block and the reduced
# slot capacity); 33 users x 256 slots in the one slice of N = 513 overflow every staged list (at most 2048 words) and walk the
# global lists; n_exclude = 70 is past the staged excludes (64).
CASES = [
    (1, 0, 5, 1, 1, 1, 1, 0, False),               # an empty catalogue
    (1, 1, 5, 1, 1, 1, 1, 0, True),                # one item
    (33, 63, 60, 64, 8, 19, 16, 5, True),          # a ragged user tile, less than one wave step, P = 128 at its largest k
    (33, 513, 68, 65, 1, 33, 16, 70, False),       # P = 256 at its smallest k, tail waves, global excludes
    (65, 2049, 32, 192, 8, 512, 16, 5, True),      # P = 256 at its largest k, two slices, the most tags
    (65, 4100, 5, 193, 8, 19, 16, 0, False),       # P = 512 at its smallest k, three slices, a partial last step, the non-VEC chain
    (33, 4100, 60, 256, 1, 33, 1, 5, True),        # the longest list, one slot per user
    (33, 513, 32, 64, 8, 19, 256, 5, True),        # 33 x 256 slots inside one slice: the staged list overflows (2048 words)
    (33, 513, 32, 193, 8, 19, 256, 5, False),      # the same at the reduced capacity of P = 512 (512 words)
    (65, 4100, 32, 10, 8, 1, 16, 5, True),         # the workload's k, one tag
]


def _slots(B, N, E, rng, amp=64):
    aid = rng.integers(0, max(N, 1), size=(B, E)).astype(np.int64)
    adl = (rng.integers(-4 * amp, 4 * amp + 1, size=(B, E)) * 0.25).astype(np.float32)
    if E >= 8:
        for b in range(B):
            aid[b, rng.integers(0, E)] = (-1, N, I64_MAX)[b % 3]
            e0, e1 = rng.choice(E, size=2, replace=False)
            aid[b, e1] = aid[b, e0]                                  # one id in two slots: the lower one counts
            sp = rng.choice(E, size=4, replace=False)
            adl[b, sp[0]], adl[b, sp[1]], adl[b, sp[2]], adl[b, sp[3]] = 0.0, np.inf, -np.inf, np.nan
    return aid, adl


@functools.lru_cache(maxsize=None)
def lattice(B, N, d, k, T, n_tags, E, n_ex, with_bias):
    """-> (user, items, s, bias, parts (all three pairs), after, exclude, targets), read-only."""
    rng = np.random.default_rng(100003 * d + 1009 * N + 17 * k + B + T + n_ex + 31 * E + 7 * n_tags)
    user = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    items = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)         # exact
    bias = None
    if with_bias:
        amp = int(4 * max(2.0, 4.0 * np.sqrt(d)))
        bias = (rng.integers(-amp, amp + 1, size=N) * 0.25).astype(np.float32)
        if N >= 63:
            bias[rng.integers(0, N, size=4)] = np.nan
            bias[int(rng.integers(0, N))] = -np.inf
    # the window
    item_time = rng.integers(0, 30, size=N).astype(np.int32)
    if N >= 63:
        item_time[rng.integers(0, N, size=3)] = ref.I32_MAX                 # never eligible
        item_time[rng.integers(0, N, size=3)] = ref.I32_MIN
    lo = rng.integers(0, 11, size=B)
    window = np.stack([lo, lo + 20], axis=1).astype(np.int32)
    # the tags
    item_tag = rng.integers(0, n_tags, size=N).astype(np.int32)
    if N >= 63:
        item_tag[rng.integers(0, N, size=3)] = -1                           # served to nobody
        item_tag[rng.integers(0, N, size=3)] = n_tags
    allow = rng.random((B, n_tags)) < 2.0 / 3.0
    # the adjustments
    aid, adl = _slots(B, N, E, rng)
    adl = adl.copy()
    # the cursor: a position drawn from the user's own scores (it need not be an eligible item), some rows at BEGIN and at END
    a_ids = rng.integers(0, max(N, 1), size=B).astype(np.int64)
    a_scores = np.zeros(B, dtype=np.float32)
    if N:
        spp = ref.scores_of(s, bias, ref.Parts(adj_ids=aid, adj_delta=adl))
        a_scores = np.nan_to_num(spp[np.arange(B), a_ids], nan=0.0, posinf=1000.0, neginf=-1000.0).astype(np.float32)
        med = np.nanmedian(np.where(np.isfinite(spp), spp, np.nan), axis=1)
        a_scores = np.where(rng.random(B) < 0.5, np.maximum(a_scores, np.nan_to_num(med).astype(np.float32)), a_scores).astype(np.float32)
    else:
        a_ids[:] = ref.PAGE_BEGIN
    for b in range(B):
        if b % 7 == 3:
            a_ids[b] = ref.PAGE_BEGIN
        if b % 11 == 5:
            a_ids[b] = -1
        if b % 13 == 6:
            a_scores[b] = np.nan
    # user 0 wide open, the last user closed, the one before nearly
    window[0] = (ref.I32_MIN, ref.I32_MAX)
    allow[0] = True
    adl[0] = np.where(np.isfinite(adl[0]), adl[0], 1.0)
    a_ids[0] = ref.PAGE_BEGIN
    if B >= 2:
        window[B - 1] = (7, 7)
        allow[B - 1] = False
        a_ids[B - 1] = -1
    if B >= 3:
        window[B - 2] = (3, 4)
        allow[B - 2] = False
        allow[B - 2, 0] = True
    ex = None
    if n_ex:
        ex = rng.integers(0, max(N, 1), size=(B, n_ex)).astype(np.int64)
        ex[:, 0], ex[:, 1], ex[:, 2] = -1, N, ex[:, min(3, n_ex - 1)]
        ex[:, 4] = aid[:, 0]                                                # excluded and adjusted: excluded
    tg = rng.integers(0, max(N, 1), size=(B, T)).astype(np.int64)
    if T >= 8 and N >= 63:
        for b in range(B):
            tg[b, 1] = ex[b, 4] if ex is not None else aid[b, 0]
            tg[b, 2] = aid[b, 1]
            tg[b, 3] = -1
            tg[b, 5] = N
    parts = ref.Parts(item_time, window, item_tag, n_tags, allow, aid, adl)
    after = (a_scores, a_ids)
    for a in (user, items, s, item_time, window, item_tag, allow, aid, adl, a_scores, a_ids, tg):
        a.setflags(write=False)
    return user, items, s, bias, parts, after, ex, tg


def select(parts, after, subset):
    """The parts of `subset` only -> (Parts, after or None)."""
    p = ref.Parts(*(parts[:2] if "window" in subset else (None, None)),
                  *(parts[2:5] if "tags" in subset else (None, 0, None)),
                  *(parts[5:7] if "adjust" in subset else (None, None)))
    return p, (after if "cursor" in subset else None)


def can_fill(B, N, k):
    """Shapes on which one user can have a full list of k and another a short one."""
    return B >= 2 and N >= 2 * k
