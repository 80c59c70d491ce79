"""The lattice data of the capped-request tests (tests/test_hip_topk_request_caps.py on the GPU, tests/test_topk_request_caps_host.py
on the CPU, which asserts on this data alone that a cap rations in every (shape, subset)).  numpy only.

The users, items, prior, window, allow rows, slots, cursor and exclude lists are tests/topk_request_cases.py's (integer users and
items, a bias and deltas of multiples of 0.25: every sum is exact in fp32, ties are abundant).  The tags are drawn anew: half of the
items fall into the first four tags, so that a cap of 1, 2 or 3 is reached long before a list is full, and the caps differ from
user to user inside a block: every fourth user is uncapped (every cap >= k), every fourth has cap 1 everywhere, the others draw
each tag's cap from {0, 1, 2, 3, 5, k}."""
import functools
import itertools

import numpy as np

from tests import topk_request_caps_ref as ref
from tests import topk_request_cases as request_cases

PART_NAMES = ("window", "allow", "adjust", "cursor")
# every subset of the four parts beside the caps; the empty one is routed to nrms_topk_dot_capped
SUBSETS = [s for n in range(5) for s in itertools.combinations(PART_NAMES, n)]

# (B, N, d, k, n_tags, E, n_exclude, bias).  k <= 64 / <= 192 / above are the three P classes.  The tag thresholds fit beside a
# request's parts for every n_tags at P = 128, for n_tags <= 43 at P = 256 (tk_request_caps_table) and never at P = 512: 43 and 44
# are the two sides of that edge, 45 and 46 lie past it.  Slices are 2048 rows: N = 2049 is two, N = 4100 three with a last step of
# four rows.  33 users x 256 slots in the one slice of N = 513 overflow the staged slot list; n_exclude = 70 is past the staged
# excludes (64).  d = 5 takes the chain's scalar loads.
CASES = [
    (1, 0, 5, 1, 1, 1, 0, False),                  # an empty catalogue
    (1, 1, 5, 1, 1, 1, 0, True),                   # one item
    (33, 63, 40, 64, 19, 16, 5, True),             # a ragged user tile, less than one wave step, P = 128 at its largest k
    (33, 513, 5, 65, 43, 16, 5, True),             # P = 256 at its smallest k: the last n_tags whose thresholds fit
    (33, 513, 40, 65, 44, 16, 70, False),          # ... and the first that do not; global excludes
    (33, 2049, 40, 192, 45, 16, 5, True),          # P = 256 at its largest k, two slices
    (33, 2049, 40, 192, 46, 1, 5, False),          # one slot per user
    (33, 4100, 5, 193, 19, 16, 0, False),          # P = 512 at its smallest k, three slices, a partial last step
    (33, 4100, 40, 256, 512, 1, 5, True),          # the longest list, the most tags
    (33, 513, 40, 64, 512, 256, 5, True),          # P = 128 with the full table; the staged slot list overflows
    (33, 2049, 40, 1, 19, 16, 5, True),            # k = 1: a cap is 0 or >= k, nothing is rationed
    (1, 2049, 40, 64, 19, 16, 5, True),            # one user
]


def can_ration(B, N, k):
    """Shapes on which a cap can ration at all: a cap below k exists only for k >= 2, and a tag needs a second item."""
    return k >= 2 and N >= 63


@functools.lru_cache(maxsize=None)
def lattice(B, N, d, k, n_tags, E, n_ex, with_bias):
    """-> (user, items, s, bias, item_tag, cap, parts (window, allow over item_tag, slots), after, exclude), read-only."""
    user, items, s, bias, parts, after, ex, _ = request_cases.lattice(B, N, d, k, 1, n_tags, E, n_ex, with_bias)
    rng = np.random.default_rng(7919 * N + 101 * k + 13 * n_tags + B)
    head = rng.integers(0, min(4, n_tags), size=N)
    item_tag = np.where(rng.random(N) < 0.5, head, rng.integers(0, n_tags, size=N)).astype(np.int32)
    if N >= 63:
        item_tag[rng.integers(0, N, size=3)] = -1                           # served to nobody
        item_tag[rng.integers(0, N, size=3)] = n_tags
    cap = rng.choice(np.array([0, 1, 2, 3, 5, k], dtype=np.int32), size=(B, n_tags)).astype(np.int32)
    for b in range(B):
        if b % 4 == 0 and B > 1:
            cap[b] = k + (b % 3)                                            # uncapped: this row is the request's
        elif b % 4 == 1:
            cap[b] = 1
    if B >= 8:
        cap[5, 0] = -3                                                      # a negative cap closes the tag
        cap[6] = 0
        cap[6, min(1, n_tags - 1)] = 2                                      # sum of the caps below k: the list cannot fill
    parts = parts._replace(item_tag=item_tag)
    for a in (item_tag, cap):
        a.setflags(write=False)
    return user, items, s, bias, item_tag, cap, parts, after, ex


def select(parts, after, subset):
    """The parts of `subset` only -> (Parts, after or None); `allow` is the tag set over the caps' item_tag."""
    p = ref.Parts(*(parts[:2] if "window" in subset else (None, None)),
                  *(parts[2:5] if "allow" in subset else (None, 0, None)),
                  *(parts[5:7] if "adjust" in subset else (None, None)))
    return p, (after if "cursor" in subset else None)


def uncapped(cap, k):
    """The caps with every open tag left uncapped: what the row would be were nothing rationed."""
    return np.where(np.asarray(cap) > 0, k, 0).astype(np.int32)
